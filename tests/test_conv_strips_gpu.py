"""GPU: the two strip tilings of the LDS-patch kernels (k_conv3x3_patch32, k_conv3x3_p512) are tuning choices only.
  * Position strips at row pitch W + 1 (ONE zero column between consecutive rows, one zero row between images): forward
    with bias + ReLU + sign bits, the head layout, the data gradient with ReLU mask + accumulation and with the un-pooling
    store -- bit-equal to the 16x16-block form (SSD_CONV_PATCH_FLAT=0) wherever both run a patch kernel (same chunk / tap
    order), and within the bf16 output rounding (2^-7 relative, as tests/test_conv_gpu.py) of the fp32 reference.  Widths
    16, 19, 38, 39 (the narrowest and widest maps the strip serves, and the two SSD300 sizes), three or more images so that
    blocks span image boundaries.
  * Row strips under fused pooling (even image pitch): conv2d_fwd_pool, with the full-resolution store and pool-only, is
    bit-equal to conv2d_fwd + maxpool2x2_fwd_argmax -- pooled values AND winner codes -- and to the per-image tiling
    (SSD_CONV_PATCH_ROWFLAT=0), for odd and even heights, SAME and VALID pooling, blocks straddling two images."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
import torch.nn.functional as F                                     # noqa: E402

from tests.conv_cases import plan_name                              # noqa: E402

WS = 1 << 25


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
    DEFAULTS = {b"SSD_CONV_PATCH_FLAT": 1, b"SSD_CONV_PATCH_ROWFLAT": 1, b"SSD_CONV_P512": 1}

    def __init__(self, L, **kv):
        self.L, self.kv = L, {k.encode(): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            assert self.L.ssd_dev_knob(k, v) == 0

    def __exit__(self, *exc):
        for k in self.kv:
            self.L.ssd_dev_knob(k, self.DEFAULTS[k])


def ref_conv3x3(x, w, bias, relu):
    y = F.conv2d(x.float().cpu().permute(0, 3, 1, 2), w.float().cpu().permute(0, 3, 1, 2), None if bias is None else bias.cpu(), padding=1)
    return (y.relu() if relu else y).permute(0, 2, 3, 1).contiguous()


def pack_bits(y):
    b = (y > 0).to(torch.uint8).reshape(*y.shape[:-1], y.shape[-1] // 8, 8)
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=y.device)
    return (b * w).sum(-1).to(torch.uint8)


# (B, H, W): widths 16, 19, 38, 39; heights differ from the widths so that a row / column mix-up cannot cancel
STRIP_MAPS = [(4, 17, 16), (5, 19, 19), (3, 38, 38), (3, 21, 39)]
# (Cin, Cout): forward / data gradient on k_conv3x3_patch32<128> / <64>, <64> / <128>, k_conv3x3_p512 (>= 256 input channels
# of the GEMM) / patch32<128> with two channel tiles, and the reverse
STRIP_CHANNELS = [(64, 128), (128, 64), (256, 128), (128, 256)]


@pytest.mark.parametrize("ch", STRIP_CHANNELS, ids=str)
@pytest.mark.parametrize("m", STRIP_MAPS, ids=str)
def test_position_strips_pitch_w_plus_1(ops, L, m, ch):
    (B, H, W), (Cin, Cout) = m, ch
    g = torch.Generator(device="cuda").manual_seed(1000 * W + Cin)
    x = torch.randn((B, H, W, Cin), generator=g, device="cuda").bfloat16()
    w = (torch.randn((Cout, 3, 3, Cin), generator=g, device="cuda") / np.sqrt(9 * Cin)).bfloat16()
    bias = torch.randn((Cout,), generator=g, device="cuda") * 0.1
    dy = torch.randn((B, H, W, Cout), generator=g, device="cuda").bfloat16()
    mask = torch.randn((B, H, W, Cin), generator=g, device="cuda").bfloat16()
    base = torch.randn((B, H, W, Cin), generator=g, device="cuda").bfloat16()
    # the map is the POOLED one of the un-pooling store: full-resolution map (2H - 1) x 2W, SAME rows / exact columns
    full = torch.randn((B, 2 * H - 1, 2 * W, Cin), generator=g, device="cuda").bfloat16()
    pooled, code = ops.maxpool2x2_fwd_argmax(full, same=True)
    assert pooled.shape == (B, H, W, Cin)
    w_t = ops.weight_transpose(w)
    fwd_plan = lambda: plan_name(L, L.ssd_conv2d_fwd_plan(B, H, W, Cin, Cout, 3, 1, 1, 1, H, W, 0, WS))
    dg_plan = lambda: plan_name(L, L.ssd_conv2d_bwd_data_plan(B, H, W, Cin, Cout, 3, 1, 1, 1, H, W, 1, WS))

    def forward():
        bits = torch.full((B, H, W, Cout // 8), 0xA5, dtype=torch.uint8, device="cuda")
        y = ops.conv2d_fwd_relubits(x, w, bias, 1, 1, 1, H, W, bits)
        return y, bits, ops.conv2d_fwd(x, w, bias, 1, 1, 1, H, W, False)

    def backward():
        acc = base.clone()
        ops.conv2d_bwd_data(dy, w_t, mask, (B, H, W, Cin), 1, 1, 1, accumulate=True, out=acc)
        up = torch.full_like(full, 7.0)                      # every element must be written
        ops.conv2d_bwd_data_unpool(dy, w_t, mask, code, full.shape, out=up)
        return acc, up, ops.conv2d_bwd_data(dy, w_t, mask, (B, H, W, Cin), 1, 1, 1)

    with knobs(L, SSD_CONV_PATCH_FLAT=2):                    # position strips wherever W <= 39
        assert fwd_plan().startswith("k_conv3x3_p") and fwd_plan().endswith("+flat"), fwd_plan()
        assert dg_plan().startswith("k_conv3x3_p") and dg_plan().endswith("+flat"), dg_plan()
        fwd_flat, bwd_flat = forward(), backward()
    compared = 0
    with knobs(L, SSD_CONV_PATCH_FLAT=0):                    # 16x16 blocks / row strips
        # where this form runs a patch kernel too the summation order is the same: same bits.  (More than 128 output
        # channels on a map that 16x16 blocks tile badly go to the generic GEMM instead: the fp32 reference below judges.)
        if fwd_plan().startswith("k_conv3x3_p"):
            assert "+flat" not in fwd_plan()
            for a, b in zip(fwd_flat, forward()):
                assert torch.equal(a, b)
            compared += 1
        if dg_plan().startswith("k_conv3x3_p"):
            assert "+flat" not in dg_plan()
            for a, b in zip(bwd_flat, backward()):
                assert torch.equal(a, b)
            compared += 1
    assert compared >= 1
    (y, bits, ylin), (acc, up, dplain) = fwd_flat, bwd_flat
    assert torch.equal(bits, pack_bits(y.float()))
    assert torch.equal(up, ops.maxpool2x2_bwd_argmax(code, dplain, full.shape))
    for relu, got in ((True, y), (False, ylin)):
        yr = ref_conv3x3(x, w, bias, relu)
        assert (got.float().cpu() - yr).abs().max().item() <= 2 ** -7 * max(1.0, yr.abs().max().item()), relu
    # data gradient = the convolution of dy with the flipped, transposed weights
    wf = w.float().cpu().flip(1, 2).permute(3, 1, 2, 0).contiguous()          # [Cin][3][3][Cout]
    dxr = ref_conv3x3(dy, wf, None, False)
    keep = (mask.float().cpu() > 0)
    assert (dplain.float().cpu() - dxr * keep).abs().max().item() <= 2 ** -7 * max(1.0, dxr.abs().max().item())
    # mask + accumulate: one more bf16 rounding of the sum (2^-6 as tests/test_conv_gpu.py)
    want = (dxr + base.float().cpu()) * keep
    assert (acc.float().cpu() - want).abs().max().item() <= 2 ** -6 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("case", [(3, 17, 16, 128, 4, 1), (4, 19, 19, 128, 6, 1), (3, 38, 38, 64, 4, 1), (3, 21, 39, 64, 6, 1),
                                  (3, 19, 19, 256, 6, 2), (3, 20, 38, 256, 4, 2)], ids=str)
def test_position_strips_head_layout(ops, L, case):
    """The fused loc + conf head (N = 340 / 510 filters: position strips on every narrow map) on k_conv3x3_patch32 and, with
    SSD_CONV_P512=2, on k_conv3x3_p512: the reference's Reshape / Concatenate layout, anchors before the level untouched."""
    (B, H, W, Cin, n, p512), C = case, 81
    A, off = 200 + H * W * n, 200
    g = torch.Generator(device="cuda").manual_seed(W + Cin)
    x = torch.randn((B, H, W, Cin), generator=g, device="cuda").bfloat16()
    w = (torch.randn((n * (4 + C), 3, 3, Cin), generator=g, device="cuda") / np.sqrt(9 * Cin)).bfloat16()
    bias = torch.randn((n * (4 + C),), generator=g, device="cuda") * 0.1
    loc = torch.zeros((B, A, 4), dtype=torch.bfloat16, device="cuda")
    conf = torch.zeros((B, A, C), dtype=torch.bfloat16, device="cuda")
    with knobs(L, SSD_CONV_P512=p512):
        name = plan_name(L, L.ssd_conv2d_head_fwd_plan(B, H, W, Cin, n, C, WS))
        ops.conv2d_head_fwd(x, w, bias, loc, conf, n, C, off)
    assert name == ("k_conv3x3_p512+flat" if p512 == 2 else "k_conv3x3_patch32<128>+flat")
    yr = ref_conv3x3(x, w, bias, False)
    loc_r = yr[..., :n * 4].reshape(B, H * W * n, 4)
    conf_r = yr[..., n * 4:].reshape(B, H * W * n, C)
    assert (loc[:, off:].float().cpu() - loc_r).abs().max().item() <= 2 ** -7 * max(1, loc_r.abs().max().item())
    assert (conf[:, off:].float().cpu() - conf_r).abs().max().item() <= 2 ** -7 * max(1, conf_r.abs().max().item())
    assert float(loc[:, :off].abs().max()) == 0 and float(conf[:, :off].abs().max()) == 0


# 75 and 150: the two pooled SSD300 layers this tiling serves; 33 and 46: an odd and an even height with partial blocks
POOL_H = [75, 150, 33, 46]
# (Cin, Cout, SSD_CONV_P512): k_conv3x3_patch32<128>, k_conv3x3_patch32<64> and (forced: 64 input channels keep the big maps cheap) k_conv3x3_p512
POOL_KERNELS = [(64, 128, 1), (128, 64, 1), (64, 128, 2)]


@pytest.mark.parametrize("kern", POOL_KERNELS, ids=str)
@pytest.mark.parametrize("same", [True, False], ids=["same", "valid"])
@pytest.mark.parametrize("B", [2, 3, 5])
@pytest.mark.parametrize("H", POOL_H)
def test_pooled_row_strips(ops, L, H, B, same, kern):
    Cin, Cout, p512 = kern
    W = H if H < 100 else 40                                 # the big heights on a narrower map: rows are what the strip tiles
    g = torch.Generator(device="cuda").manual_seed(H * 10 + B)
    x = torch.randn((B, H, W, Cin), generator=g, device="cuda").bfloat16()
    w = (torch.randn((Cout, 3, 3, Cin), generator=g, device="cuda") / np.sqrt(9 * Cin)).bfloat16()
    bias = torch.randn((Cout,), generator=g, device="cuda") * 0.1
    runs, names = [], []
    for rowflat in (1, 0):
        with knobs(L, SSD_CONV_PATCH_ROWFLAT=rowflat, SSD_CONV_P512=p512):
            names.append(plan_name(L, L.ssd_conv2d_fwd_plan(B, H, W, Cin, Cout, 3, 1, 1, 1, H, W, 1, WS)))
            for relu in (True, False):                       # (the pooling has an integer path after ReLU and a float path without)
                y, yp, code = ops.conv2d_fwd_pool(x, w, bias, 1, 1, 1, H, W, relu, same)
                y_ref = ops.conv2d_fwd(x, w, bias, 1, 1, 1, H, W, relu)
                yp_ref, code_ref = ops.maxpool2x2_fwd_argmax(y_ref, same=same)
                assert torch.equal(y, y_ref), (rowflat, relu)
                assert torch.equal(yp, yp_ref), (rowflat, relu)
                assert torch.equal(code, code_ref), (rowflat, relu)
                yp2 = torch.full_like(yp, 7.0)
                code2 = torch.full_like(code, 0x55555555)
                none, _, _ = ops.conv2d_fwd_pool(x, w, bias, 1, 1, 1, H, W, relu, same, pool_out=yp2, code=code2, pool_only=True)
                assert none is None and torch.equal(yp2, yp_ref) and torch.equal(code2, code_ref), (rowflat, relu)
                runs.append((rowflat, relu, yp, code))
    base = "k_conv3x3_p512" if p512 == 2 else "k_conv3x3_patch32<%d>" % Cout
    # row strips are taken when they need fewer blocks than per-image tiling: image pitch H + 1, even (H + 2 for an even H)
    rows, pitch = (32 if p512 == 2 else 16), H + 1 + (H + 1) % 2
    strip = -(-B * pitch // rows) < B * -(-H // rows)
    assert names == [base + ("+rowflat" if strip else "") + "+poolfused", base + "+poolfused"], names
    for (_, _, a, ca), (_, _, b, cb) in zip(runs[:2], runs[2:]):
        assert torch.equal(a, b) and torch.equal(ca, cb)
    yr = ref_conv3x3(x, w, bias, True)
    yr = yr.permute(0, 3, 1, 2)
    if same:
        yr = F.pad(yr, (0, W % 2, 0, H % 2), value=float("-inf"))
    pr = F.max_pool2d(yr, 2, 2).permute(0, 2, 3, 1)
    got = runs[0][2].float().cpu()
    assert got.shape == pr.shape and (got - pr).abs().max().item() <= 2 ** -7 * max(1.0, pr.abs().max().item())
