"""GPU: the three entry points of the pooled layers (block1_conv2, block2_conv2, block3_conv3) under the strict harness
(tests/strict.py), on every kernel form the cases of tests/pooled_cases.py name:

  ssd_conv2d_fwd_pool             k_conv3x3_c64b, k_conv3x3_patch32<64>, <128>, k_conv3x3_p512 as blocks and as row strips; SAME and
                                  VALID pooling, relu 1 and 0, with and without y; the two-launch fallback on position strips
  ssd_conv2d_bwd_data_unpool      the three LDS-patch kernels as blocks, row strips and position strips; without mask, with
                                  relu_src, with dx_pooled; store stage with and without its LDS side tables; the refusals
  ssd_conv2d_bwd_weight_unpooled  one to sixteen channel groups, one and two blocks per workgroup, clipped and uncovered edges,
                                  with and without dbias, a workspace of exactly the queried bytes; the refusals

Operands are small integers (tests/test_pooled_cases_cpu.py asserts their regime, what they exercise, and that three wrong
references differ from the right one), every tensor lives in strict.Arena, every run happens under two poisons, and every
comparison is torch.equal against the CPU reference: ref_pool, ref_unpool and _wgrad of tests/strict.py.  No tolerances."""
import ctypes
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                                                         # noqa: E402
from tests import pooled_cases as P                                                              # noqa: E402
from tests.test_conv_strict_gpu import arena_for, knobs as _knobs                                # noqa: E402

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


class knobs(_knobs):
    DEFAULTS = dict(_knobs.DEFAULTS, SSD_EPI_PREFETCH=1)


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def _id(c):
    return str(tuple(v for v in c if not isinstance(v, (str, tuple))))


@functools.lru_cache(maxsize=None)
def conv_ref(case):
    """the convolution's reference, shared by the four (pooling, relu) runs of a forward case and never modified"""
    return strict.conv_case(case + (3, 1, "same"))


# ---------------------------------------------------------------- convolution + pooling
@pytest.mark.parametrize("same", [True, False], ids=["same", "valid"])
@pytest.mark.parametrize("case", P.FWD_POOL_CASES, ids=_id)
def test_fwd_pool_strict(ops, L, case, same):
    B, H, W, Cin, Cout = case[:5]
    plans = P.fwd_pool_plans(L, case)
    assert plans == case[5:7], "the dispatch rules moved: this case no longer tests the kernel it names"
    fused = "poolfused" in plans[0]
    base = conv_ref(case[:5])
    Hp, Wp = P.pooled_size(H, same), P.pooled_size(W, same)
    a = arena_for(base, 2 * P.WS_BYTES)
    x, w, bias, ws = a.put(base["x"], "x"), a.put(base["w"], "w"), a.put(base["bias"], "bias"), a.workspace()
    y, yp, code = a.out((B, H, W, Cout), BF, "y"), a.out((B, Hp, Wp, Cout), BF, "y_pool"), a.out((B, Hp, Wp, Cout // 8), I32, "pool_code")
    for relu in (True, False):
        r = strict.fwd_pool_case(case[:5] + (3, 1, "same"), same, relu, r=base)
        want = [(y, r["y_relu" if relu else "y"].to(BF)), (yp, r["yp"].to(BF)), (code, strict.pack_codes(r["code"]))]
        a.run(lambda: ops.conv2d_fwd_pool(x, w, bias, 1, 1, 1, H, W, relu, same, out=y, pool_out=yp, code=code, ws=ws), want)

        def pool_only():
            return ops.conv2d_fwd_pool(x, w, bias, 1, 1, 1, H, W, relu, same, pool_out=yp, code=code, ws=ws, pool_only=True)
        if fused:                                    # y == NULL: y is not listed and must keep its poison
            a.run(pool_only, want[1:])
        else:                                        # no kernel pools this layer in its store stage: refused, nothing written
            def refused():
                with pytest.raises(ValueError):
                    pool_only()
            a.run(refused, [])


# ---------------------------------------------------------------- data gradient carried through the pooling
@pytest.mark.parametrize("case", P.UNPOOL_CASES, ids=_id)
def test_bwd_data_unpool_strict(ops, L, case):
    B, Hf, Wf, C, Cout, same = case[:6]
    for has_src in (0, 1):
        assert P.unpool_plan(L, case, has_src) == case[6], "the dispatch rules moved: this case no longer tests the kernel it names"
    r = strict.unpool_case(B, Hf, Wf, C, Cout, same)
    H, W = r["geom"][:2]
    a = arena_for(r, 2 * P.WS_BYTES)
    dy, w_t, mask, ws = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t"), a.put(r["mask_src"], "relu_src"), a.workspace()
    code = a.put(strict.pack_codes(r["code"]), "pool_code")
    full, pooled = a.out((B, Hf, Wf, C), BF, "dx_full"), a.out((B, H, W, C), BF, "dx_pooled")
    runs = [(None, None, [(full, r["dfull"].to(BF))]),
            (mask, None, [(full, r["dfull_masked"].to(BF))]),
            (None, pooled, [(full, r["dfull"].to(BF)), (pooled, r["dx"].to(BF))]),
            (mask, pooled, [(full, r["dfull_masked"].to(BF)), (pooled, r["dx_masked"].to(BF))])]
    got = {}
    for prefetch in (1, 0):                          # the store stage with and without its LDS side tables: the same bits
        with knobs(L, SSD_EPI_PREFETCH=prefetch):
            got[prefetch] = [a.run(lambda: ops.conv2d_bwd_data_unpool(dy, w_t, src, code, (B, Hf, Wf, C), out=full, ws=ws, pooled_out=po), want)
                             for src, po, want in runs]
    for one, two in zip(got[1], got[0]):
        for t1, t0 in zip(one, two):
            assert torch.equal(t1.view(torch.int16), t0.view(torch.int16))


@pytest.mark.parametrize("case", P.UNPOOL_REFUSED, ids=str)
def test_bwd_data_unpool_refusals_strict(ops, L, case):
    """VALID pooling of an odd size, and a pooled map no LDS-patch kernel serves: NotImplementedError, nothing written"""
    from ssd_object_detection_amd._lib import SSD_ERR_UNSUPPORTED
    B, Hf, Wf, C, Cout, same = case
    assert P.unpool_plan(L, case) == "error %d" % SSD_ERR_UNSUPPORTED
    H, W = P.pooled_size(Hf, same), P.pooled_size(Wf, same)
    r = strict.conv_case((B, H, W, C, Cout, 3, 1, "same"))
    a = arena_for(r, 2 * P.WS_BYTES)
    dy, w_t, mask, ws = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t"), a.put(r["mask_src"], "relu_src"), a.workspace()
    code = a.put(torch.zeros((B, H, W, C // 8), dtype=I32), "pool_code")
    full, pooled = a.out((B, Hf, Wf, C), BF, "dx_full"), a.out((B, H, W, C), BF, "dx_pooled")

    def refused():
        for src in (None, mask):
            for po in (None, pooled):
                with pytest.raises(NotImplementedError):
                    ops.conv2d_bwd_data_unpool(dy, w_t, src, code, (B, Hf, Wf, C), out=full, ws=ws, pooled_out=po)
    a.run(refused, [])


# ---------------------------------------------------------------- weight gradient from the pooled gradient
@pytest.mark.parametrize("case", P.WGRAD_UNPOOLED_CASES, ids=_id)
def test_bwd_weight_unpooled_strict(ops, L, case):
    B, H, W, Cin, Cout, same = case[:6]
    ns, tiles, _ = P.wgrad_unpooled_splits(L, case)
    assert (ns, tiles) == case[6], "the split plan moved: this case no longer reaches what it names"
    r = strict.wgrad_unpooled_case(B, H, W, Cin, Cout, same)
    strict.check_regime(r)
    nbytes = ns * (Cout * 9 * Cin + Cout) * 4
    a = arena_for(r, 2 * nbytes)
    x, dp, code, ws = a.put(r["x"], "x"), a.put(r["dp"], "dpool"), a.put(strict.pack_codes(r["code"]), "pool_code"), a.workspace()
    dw, db = a.out((Cout, 3, 3, Cin), F32, "dw"), a.out((Cout,), F32, "dbias")
    a.run(lambda: ops.conv2d_bwd_weight_unpooled(x, dp, code, dw=dw, dbias=db, ws=ws), [(dw, r["dw"]), (db, r["dbias"])])
    a.run(lambda: ops.conv2d_bwd_weight_unpooled(x, dp, code, dw=dw, want_bias=False, ws=ws), [(dw, r["dw"])])
    assert list(ws.slots) == [nbytes]                # one workspace, of exactly the queried bytes


class _ShortWorkspace:
    """hands out one byte less than asked for"""

    def __init__(self, ws):
        self.ws = ws

    def get(self, nbytes, device):
        return self.ws.get(nbytes - 1, device)


def test_bwd_weight_unpooled_refusals_strict(ops, L):
    from ssd_object_detection_amd._lib import SSD_ERR_UNSUPPORTED, SSD_ERR_WORKSPACE
    g = torch.Generator().manual_seed(7)
    for B, H, W, Cin, Cout, Hp, Wp in P.WGRAD_UNPOOLED_REFUSED:
        a = strict.Arena("cuda", 1 << 26)
        x, dp = a.put(strict.ints(g, (B, H, W, Cin), (0, 1, 2)), "x"), a.put(strict.ints(g, (B, Hp, Wp, Cout), (-1, 1)), "dpool")
        code = a.put(torch.zeros((B, Hp, Wp, Cout // 8), dtype=I32), "pool_code")
        dw, db = a.out((Cout, 3, 3, Cin), F32, "dw"), a.out((Cout,), F32, "dbias")
        scratch = a.workspace().get(1 << 20, "cuda")

        def refused():
            with pytest.raises(NotImplementedError):
                ops.conv2d_bwd_weight_unpooled(x, dp, code, dw=dw, dbias=db, ws=a.workspace())
            p = [ctypes.c_void_p(t.data_ptr()) for t in (x, dp, code, dw, db, scratch)]       # the entry itself, given a workspace
            assert L.ssd_conv2d_bwd_weight_unpooled(*p[:5], B, H, W, Cin, Cout, Hp, Wp, p[5], scratch.numel(), None) == SSD_ERR_UNSUPPORTED
        a.run(refused, [])
    # a workspace one byte short of the queried size
    B, H, W, Cin, Cout, same = P.WGRAD_UNPOOLED_CASES[1][:6]
    r = strict.wgrad_unpooled_case(B, H, W, Cin, Cout, same)
    nbytes = L.ssd_conv2d_bwd_weight_unpooled_workspace_bytes(B, H, W, Cin, Cout, *r["dp"].shape[1:3])
    a = arena_for(r, 2 * nbytes)
    x, dp, code = a.put(r["x"], "x"), a.put(r["dp"], "dpool"), a.put(strict.pack_codes(r["code"]), "pool_code")
    dw, db = a.out((Cout, 3, 3, Cin), F32, "dw"), a.out((Cout,), F32, "dbias")
    short = _ShortWorkspace(a.workspace())

    def too_small():
        with pytest.raises(RuntimeError, match="status %d" % SSD_ERR_WORKSPACE):
            ops.conv2d_bwd_weight_unpooled(x, dp, code, dw=dw, dbias=db, ws=short)
    a.run(too_small, [])
    assert list(short.ws.slots) == [nbytes - 1]
