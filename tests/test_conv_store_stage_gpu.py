"""GPU: the store stage of the LDS-patch kernels with its side tables in LDS (SSD_EPI_PREFETCH, default 1) against the same
stage without them (0): the ReLU sign bytes of a k_conv3x3_p512 data-gradient tile fetched by LDS-DMA in the prologue, the
row map (tile row -> output pixel) of k_conv3x3_p512 and of k_conv3x3_patch32's strips, and k_conv3x3_p512's bias.

Every case runs under the strict harness (tests/strict.py): operands are small integers, so the fp32 reference is exact and each
comparison is torch.equal -- tighter than the 2^-7 (2^-6 with accumulation) the random-operand tests allow a data gradient;
outputs and guards are poisoned, twice.  The result under SSD_EPI_PREFETCH=0 must have the same bits.

Kernels: the dispatch query is asserted for every case.  N below is the GEMM's N (the data gradient's output channels):
N = 128 fills the 128-channel tile (sign bytes by DMA), N = 192 leaves the second tile partial and the rows of the sign map at
a 24-byte pitch (no DMA: the global read stays), N = 64 is below what k_conv3x3_p512 takes under any knob (its rule is
N > 64), so that case is k_conv3x3_patch32<64>, which it names.  10x10 is below the 16x16 the patch family starts at: the
generic GEMM serves it, the case stays to show that the knob does not reach it."""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                             # noqa: E402
from tests.conv_cases import WS_BYTES, plan_name                     # noqa: E402

BF, U8, I32 = torch.bfloat16, torch.uint8, torch.int32


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


class knobs:
    """Set development knobs for a block and put their defaults back."""
    DEFAULTS = {"SSD_CONV_PATCH_FLAT": 1, "SSD_CONV_P512": 1, "SSD_EPI_PREFETCH": 1}

    def __init__(self, L, **kv):
        self.L, self.kv = L, kv

    def __enter__(self):
        for k, v in self.kv.items():
            assert self.L.ssd_dev_knob(k.encode(), v) == 0

    def __exit__(self, *exc):
        for k in self.kv:
            self.L.ssd_dev_knob(k.encode(), self.DEFAULTS[k])


def arena_for(r):
    total = sum(t.numel() * t.element_size() for t in r.values() if torch.is_tensor(t))
    return strict.Arena("cuda", 2 * total + 2 * WS_BYTES + 32 * (2 * strict.GUARD + 2 * strict.ALIGN))


@functools.lru_cache(maxsize=None)
def reference(case):
    """strict.conv_case of a (B, H, W, Cin, Cout, 3, 1, "same") case, computed once and shared (read-only)"""
    return strict.conv_case(case)


def both(L, a, fn, want):
    """fn under SSD_EPI_PREFETCH = 1 and 0, each in the arena against the exact reference; the two results bit for bit"""
    with knobs(L, SSD_EPI_PREFETCH=1):
        new = a.run(fn, want)
    with knobs(L, SSD_EPI_PREFETCH=0):
        old = a.run(fn, want)
    for n, o in zip(new, old):
        assert torch.equal(n.view(-1).view(strict._INT[n.element_size()]), o.view(-1).view(strict._INT[o.element_size()]))


# ---------------------------------------------------------------- data gradient
# (SSD_CONV_P512, N): k_conv3x3_p512 with a full tile, the N = 64 case (see above), a partial second tile;
# k_conv3x3_patch32<128> and <64>.  The GEMM's K side (dy) has 64 channels, one chunk pair, the smallest the kernels take (128
# where N = 64: 64 -> 64 belongs to k_conv3x3_c64b).
DG_KERNELS = [(2, 128), (2, 64), (2, 192), (1, 128), (1, 64)]
# (SSD_CONV_PATCH_FLAT, B, H, W): 33x33 as the dispatch decides (16x16 / 32x16 blocks; N = 192 goes to strips), then strips
# forced: batch 3 at 19x19 -- 1200 positions, so a 512-position block holds an image boundary and the last block is partial --
# and 10x10
DG_MAPS = [(1, 2, 33, 33), (2, 3, 19, 19), (2, 3, 10, 10)]
# block form of k_conv3x3_patch32 (strips off), for the cases of DG_KERNELS that are not k_conv3x3_p512
DG_BLOCK_MAP = (0, 2, 33, 33)


def expected_kernel(p512, N, H):
    if H < 16:
        return "k_conv_igemm_dma"
    return "k_conv3x3_p512" if (p512 == 2 and N > 64) else "k_conv3x3_patch32<%d>" % (128 if N > 64 else 64)


def run_dgrad(ops, L, kern, m, mode):
    (p512, N), (flat, B, H, W) = kern, m
    C = 128 if N == 64 else 64                                      # (64 -> 64 is k_conv3x3_c64b's)
    case = (B, H, W, N, C, 3, 1, "same")
    r = reference(case)
    a = arena_for(r)
    dy, w_t, ws = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t"), a.workspace()
    bits, src = a.put(r["x_bits"], "mask bits"), a.put(r["mask_src"], "relu_src")
    dx, acc = a.out((B, H, W, N), BF, "dx"), a.inout(r["base"], "dx (accumulated onto)")
    shape = (B, H, W, N)
    with knobs(L, SSD_CONV_P512=p512, SSD_CONV_PATCH_FLAT=flat):
        for accumulate in (0, 1):
            name = plan_name(L, L.ssd_conv2d_bwd_data_plan(B, H, W, N, C, 3, 1, 1, 1, H, W, accumulate, WS_BYTES))
            assert name.startswith(expected_kernel(p512, N, H)), name
            assert ("+flat" in name) == (H >= 16 and (flat == 2 or (flat == 1 and N == 192))), name
        if "+splitk" in name:                                       # (10x10: split-K carries no sign bytes, the bf16 source it does)
            mode = "src"
        if mode == "bits":
            both(L, a, lambda: ops.conv2d_bwd_data_bits(dy, w_t, bits, shape, 1, 1, 1, out=dx, ws=ws), [(dx, r["dx_masked"].to(BF))])
            both(L, a, lambda: ops.conv2d_bwd_data_bits(dy, w_t, bits, shape, 1, 1, 1, accumulate=True, out=acc, ws=ws),
                 [(acc, r["dx_acc"].to(BF))])
        else:                                                       # the bf16 mask source: the global reads of before, in both runs
            both(L, a, lambda: ops.conv2d_bwd_data(dy, w_t, src, shape, 1, 1, 1, out=dx, ws=ws), [(dx, r["dx_masked"].to(BF))])
            both(L, a, lambda: ops.conv2d_bwd_data(dy, w_t, src, shape, 1, 1, 1, accumulate=True, out=acc, ws=ws),
                 [(acc, r["dx_acc"].to(BF))])
            both(L, a, lambda: ops.conv2d_bwd_data(dy, w_t, None, shape, 1, 1, 1, out=dx, ws=ws), [(dx, r["dx"].to(BF))])


@pytest.mark.parametrize("m", DG_MAPS, ids=str)
@pytest.mark.parametrize("kern", DG_KERNELS, ids=str)
def test_dgrad_sign_bytes_and_row_map(ops, L, kern, m):
    """sign bytes given as bits, without and with accumulation"""
    run_dgrad(ops, L, kern, m, "bits")


@pytest.mark.parametrize("kern", [k for k in DG_KERNELS if not (k[0] == 2 and k[1] > 64)], ids=str)
def test_dgrad_patch32_block_form(ops, L, kern):
    run_dgrad(ops, L, kern, DG_BLOCK_MAP, "bits")


@pytest.mark.parametrize("m", DG_MAPS[:2], ids=str)
@pytest.mark.parametrize("kern", DG_KERNELS, ids=str)
def test_dgrad_mask_src_keeps_the_global_reads(ops, L, kern, m):
    """the bf16 mask source instead of bits (and no mask at all): the old path, with the row map under it"""
    run_dgrad(ops, L, kern, m, "src")


# ---------------------------------------------------------------- forward: bias from LDS, row map under the sign-bit store
# (SSD_CONV_P512, Cout): k_conv3x3_p512 with a full tile and with a partial second one (bias past N: zeros), k_conv3x3_patch32<128>
FWD_KERNELS = [(2, 128), (2, 192), (1, 128)]


@pytest.mark.parametrize("m", DG_MAPS[:2], ids=str)
@pytest.mark.parametrize("kern", FWD_KERNELS, ids=str)
def test_fwd_bias_relu_sign_bits(ops, L, kern, m):
    (p512, Cout), (flat, B, H, W) = kern, m
    r = reference((B, H, W, 64, Cout, 3, 1, "same"))
    a = arena_for(r)
    x, w, bias, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.workspace()
    y, bits = a.out((B, H, W, Cout), BF, "y"), a.out((B, H, W, Cout // 8), U8, "relu_bits")
    with knobs(L, SSD_CONV_P512=p512, SSD_CONV_PATCH_FLAT=flat):
        name = plan_name(L, L.ssd_conv2d_fwd_plan(B, H, W, 64, Cout, 3, 1, 1, 1, H, W, 0, WS_BYTES))
        assert name.startswith("k_conv3x3_p512" if p512 == 2 else "k_conv3x3_patch32<128>"), name
        both(L, a, lambda: ops.conv2d_fwd_relubits(x, w, bias, 1, 1, 1, H, W, bits, out=y, ws=ws),
             [(y, r["y_relu"].to(BF)), (bits, r["y_bits"])])
        both(L, a, lambda: ops.conv2d_fwd(x, w, bias, 1, 1, 1, H, W, False, out=y, ws=ws), [(y, r["y"].to(BF))])
        both(L, a, lambda: ops.conv2d_fwd(x, w, None, 1, 1, 1, H, W, True, out=y, ws=ws),          # no bias: zeros in the table
             [(y, (r["y"] - r["bias"]).relu().to(BF))])


@pytest.mark.parametrize("kern", [(2, 128), (1, 128)], ids=str)
def test_fwd_fused_pooling_on_row_strips(ops, L, kern):
    """the pooling loop asks the row map which candidates lie inside the map: 33 rows, image pitch 34, blocks straddle images"""
    p512, Cout = kern
    B, H, W, same = 3, 33, 33, True
    case = (B, H, W, 64, Cout, 3, 1, "same")
    r = dict(reference(case))
    Hp, Wp = (H + 1) // 2, (W + 1) // 2
    yp_ref, code_ref = strict.ref_pool(r["y_relu"], 2, 2, 0, 0, Hp, Wp, 4)
    a = arena_for(r)
    x, w, bias, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.workspace()
    y, yp, code = a.out((B, H, W, Cout), BF, "y"), a.out((B, Hp, Wp, Cout), BF, "y_pool"), a.out((B, Hp, Wp, Cout // 8), I32, "pool_code")
    want = [(y, r["y_relu"].to(BF)), (yp, yp_ref.to(BF)), (code, strict.pack_codes(code_ref))]
    with knobs(L, SSD_CONV_P512=p512):
        name = plan_name(L, L.ssd_conv2d_fwd_plan(B, H, W, 64, Cout, 3, 1, 1, 1, H, W, 1, WS_BYTES))
        assert name == ("k_conv3x3_p512" if p512 == 2 else "k_conv3x3_patch32<128>") + "+rowflat+poolfused", name
        both(L, a, lambda: ops.conv2d_fwd_pool(x, w, bias, 1, 1, 1, H, W, True, same, out=y, pool_out=yp, code=code, ws=ws), want)
        both(L, a, lambda: ops.conv2d_fwd_pool(x, w, bias, 1, 1, 1, H, W, True, same, pool_out=yp, code=code, ws=ws, pool_only=True),
             want[1:])


@pytest.mark.parametrize("p512", [2, 1])
def test_head_layout_store_on_strips(ops, L, p512):
    B, H, W, Cin, n = 3, 19, 19, 64, 6
    r = strict.head_case(B, H, W, Cin, n)
    strict.check_regime(r)
    C, off, A = r["classes"], r["off"], r["loc"].shape[1]
    a = arena_for(r)
    x, w, bias, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.workspace()
    loc, conf = a.out((B, A, 4), BF, "loc"), a.out((B, A, C), BF, "conf")
    with knobs(L, SSD_CONV_P512=p512):
        name = plan_name(L, L.ssd_conv2d_head_fwd_plan(B, H, W, Cin, n, C, WS_BYTES))
        assert name == ("k_conv3x3_p512+flat" if p512 == 2 else "k_conv3x3_patch32<128>+flat"), name
        both(L, a, lambda: ops.conv2d_head_fwd(x, w, bias, loc, conf, n, C, off, ws=ws),
             [(loc, r["loc"].to(BF), r["loc_written"]), (conf, r["conf"].to(BF), r["conf_written"])])
