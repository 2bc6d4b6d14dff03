"""CPU suite of the depthwise 3x3 convolution: the oracle (tests/depthwise_oracle.py) against independent restatements, the
exact-arithmetic regime of every GPU case of tests/test_depthwise_strict_gpu.py, and the host-side refusals of the C ABI (decided
before any launch: callable without a GPU, with pointers that are never dereferenced)."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

from tests import strict                                                                                    # noqa: E402
from tests.depthwise_oracle import (CASES, REALISTIC, SEPARABLE, dw_case, gather_loop, geometry, nine_tap_loop,    # noqa: E402
                                    realistic_case, ref_dwconv, separable_case)


# ---------------------------------------------------------------- the oracle
@pytest.mark.parametrize("case", CASES, ids=str)
def test_regime_and_fp32_equals_float64(case):
    r = dw_case(case)
    strict.check_regime(r)
    assert float(r["y"].abs().max()) <= 21 and float(r["dx"].abs().max()) <= 18 and float(r["dx_acc"].abs().max()) <= 20
    r64 = dw_case(case, torch.float64)
    for name in ("y", "y_relu", "dx", "dx_masked", "dx_acc", "dw", "dbias"):
        assert torch.equal(r[name].double(), r64[name]), (case, name)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_oracle_equals_the_nine_tap_loop(case):
    B, H, W, C, stride, padding = case
    r = dw_case(case)
    Ho, Wo, pt, pl = r["geom"]
    assert torch.equal(nine_tap_loop(r["x"], r["w"], r["bias"], stride, pt, pl, Ho, Wo), r["y"])
    assert torch.equal(ref_dwconv(r["x"], r["w"], r["bias"], stride, pt, pl, Ho, Wo, True), r["y_relu"])
    # the weight gradient, tap by tap: the same shifted slices times dy, summed over the pixels
    xp = torch.zeros((B, (Ho - 1) * stride + 3, (Wo - 1) * stride + 3, C))
    xp[:, pt:pt + H, pl:pl + W] = r["x"].float()
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            assert torch.equal((sl * r["dy"].float()).sum((0, 1, 2)), r["dw"][ky, kx]), (ky, kx)
    assert torch.equal(r["dy"].float().sum((0, 1, 2)), r["dbias"])


@pytest.mark.parametrize("case", [c for c in CASES if c[0] * c[1] * c[2] <= 400], ids=str)
def test_data_gradient_equals_the_gather_loop(case):
    B, H, W, C, stride, padding = case
    r = dw_case(case)
    _, _, pt, pl = r["geom"]
    assert torch.equal(gather_loop(r["dy"], r["w"], (B, H, W, C), stride, pt, pl), r["dx"])


def test_geometry_of_the_cases():
    """even map at stride 2: TF SAME pads 0 above and 1 below, torch's padding 1 pads 1 above and 0 below, the same 5 x 5 output"""
    assert geometry(10, 10, 2, "same") == (5, 5, 0, 0) and geometry(10, 10, 2, "pad1") == (5, 5, 1, 1)
    assert geometry(19, 19, 2, "same") == (10, 10, 1, 1) and geometry(75, 75, 2, "same") == (38, 38, 1, 1)
    assert geometry(2, 9, 1, "same") == (2, 9, 1, 1) and geometry(1, 1, 1, "same") == (1, 1, 1, 1)
    a, b = dw_case((2, 10, 10, 40, 2, "same")), dw_case((2, 10, 10, 40, 2, "pad1"))
    assert a["y"].shape == b["y"].shape


@pytest.mark.parametrize("case", REALISTIC, ids=str)
def test_realistic_bounds_are_tight_and_positive(case):
    r = realistic_case(case)
    for name in ("y", "dx", "dw", "dbias"):
        bound = r[name + "_bound"]
        assert bool((bound >= 0).all()) and bool(torch.isfinite(bound).all())
        # dominated by the one bf16 rounding (2^-8 relative) for y and dx, by (P + 16) 2^-24 for the fp32 sums
        assert float(bound.max()) <= 2.0 ** -7 * max(1.0, float(r[name].abs().max()))


@pytest.mark.parametrize("case", SEPARABLE, ids=str)
def test_separable_block_is_in_the_exact_regime(case):
    r = separable_case(case)
    strict.check_regime(r)
    assert float(r["y2"].abs().max()) <= 171 and float(r["g1"].abs().max()) <= 4 and float(r["dx"].abs().max()) <= 36


# ---------------------------------------------------------------- the C ABI, host side
@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib, _lib.lib()


def P(i):
    """distinct pointers 256 MiB apart, never dereferenced on a refused call"""
    return ctypes.c_void_p(0x10000000 * (i + 1))


GEOMETRY_VALUE = (dict(B=0), dict(H=0), dict(W=-1), dict(C=0), dict(Ho=0), dict(Wo=0), dict(s=0), dict(s=3), dict(pt=2), dict(pt=-1),
                  dict(pl=2), dict(pl=-1),
                  dict(Ho=17), dict(Ho=21), dict(Wo=17), dict(Wo=21),      # 19 rows, stride 1, pad 1: the rest would be -1 / 3
                  dict(pt=0, Ho=19, pl=0, Wo=20),                          # ... pad_l = 0, Wo = 20: 3 columns after the map
                  dict(s=2, Ho=9, Wo=9), dict(s=2, Ho=11, Wo=11))          # stride 2, pad 1: 10 is the only size
GEOMETRY_UNSUPPORTED = (dict(C=12), dict(C=36), dict(B=1 << 11, H=256, W=256, Ho=256, Wo=256, C=8),      # 2^31 bytes exactly
                        dict(B=1 << 20, H=1 << 20, W=1 << 20, Ho=1 << 20, Wo=1 << 20, C=8))
OK = dict(B=2, H=19, W=19, C=72, s=1, pt=1, pl=1, Ho=19, Wo=19)


def test_fwd_refuses_on_the_host(lib):
    _lib, L = lib
    V, U = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    ok = dict(OK, x=P(0), w=P(1), bias=P(2), y=P(3))

    def call(**kv):
        a = dict(ok, **kv)
        return L.ssd_dwconv3x3_fwd(a["x"], a["w"], a["bias"], a["y"], a["B"], a["H"], a["W"], a["C"], a["s"], a["pt"], a["pl"], a["Ho"],
                                   a["Wo"], 1, None)

    for kv in (dict(x=None), dict(w=None), dict(y=None), dict(y=ok["x"]), dict(y=ok["w"]), dict(y=ok["bias"]),
               dict(y=ctypes.c_void_p(ok["x"].value + 64)), dict(y=ctypes.c_void_p(ok["x"].value - 64))) + GEOMETRY_VALUE:
        assert call(**kv) == V, kv
    for kv in GEOMETRY_UNSUPPORTED:
        assert call(**kv) == U, kv
    # served geometries that a refusal must not catch: valid (no padding), TF SAME and torch's padding at stride 2
    for kv in (dict(x=None, pt=0, pl=0, Ho=17, Wo=17), dict(x=None, s=2, Ho=10, Wo=10), dict(x=None, H=10, W=10, s=2, pt=0, pl=0, Ho=5, Wo=5),
               dict(x=None, H=10, W=10, s=2, Ho=5, Wo=5), dict(x=None, pt=0, Ho=18)):
        assert call(**kv) == V, kv                     # (refused for the NULL x alone ...)
        assert call(**dict(kv, x=ok["x"], C=12)) == U, kv     # ... and for the channel count alone: the geometry passed


def test_bwd_data_refuses_on_the_host(lib):
    _lib, L = lib
    V, U = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    ok = dict(OK, dy=P(0), w=P(1), src=None, dx=P(3))

    def call(**kv):
        a = dict(ok, **kv)
        return L.ssd_dwconv3x3_bwd_data(a["dy"], a["w"], a["src"], a["dx"], a["B"], a["H"], a["W"], a["C"], a["s"], a["pt"], a["pl"],
                                        a["Ho"], a["Wo"], 0, None)

    for kv in (dict(dy=None), dict(w=None), dict(dx=None), dict(dx=ok["dy"]), dict(dx=ok["w"]),
               dict(src=ctypes.c_void_p(ok["dx"].value + 64))) + GEOMETRY_VALUE:      # relu_src may BE dx, not straddle it
        assert call(**kv) == V, kv
    for kv in GEOMETRY_UNSUPPORTED:
        assert call(**kv) == U, kv
    assert call(C=12, src=ok["dx"]) == U               # relu_src aliasing dx is no refusal: the channel count is what is refused


def test_bwd_weight_refuses_on_the_host(lib):
    _lib, L = lib
    V, U, WS = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED, _lib.SSD_ERR_WORKSPACE
    ok = dict(OK, x=P(0), dy=P(1), dw=P(2), db=P(3), ws=P(4), short=0)
    q = L.ssd_dwconv3x3_bwd_weight_workspace_bytes
    need = q(2, 19, 19, 72, 1, 19, 19)
    assert need > 0 and need % (10 * 72 * 4) == 0                      # whole slabs of [10][C] fp32

    def query(a):
        return q(a["B"], a["H"], a["W"], a["C"], a["s"], a["Ho"], a["Wo"])

    def call(**kv):
        a = dict(ok, **kv)
        return L.ssd_dwconv3x3_bwd_weight(a["x"], a["dy"], a["dw"], a["db"], a["B"], a["H"], a["W"], a["C"], a["s"], a["pt"], a["pl"],
                                          a["Ho"], a["Wo"], a["ws"], max(query(a) - a["short"], 0), None)

    for kv in (dict(x=None), dict(dy=None), dict(dw=None), dict(dw=ok["x"]), dict(dw=ok["dy"]), dict(db=ok["dy"]), dict(db=ok["x"]),
               dict(db=ok["dw"])) + GEOMETRY_VALUE:
        assert call(**kv) == V, kv
    # the size query returns 0 exactly where the call is unsupported
    for kv in GEOMETRY_UNSUPPORTED:
        assert call(**kv) == U and query(dict(ok, **kv)) == 0, kv
    for kv in (dict(), dict(s=2, Ho=10, Wo=10), dict(C=8), dict(B=64, H=150, W=150, C=32, Ho=150, Wo=150), dict(db=None)):
        a = dict(ok, **kv)
        assert query(a) > 0 and call(**kv, short=1) == WS and call(**kv, ws=None) == WS, kv
    assert call(db=None, short=1) == WS


def test_wrappers_and_prototypes_exist(lib):
    _lib, L = lib
    import ssd_object_detection_amd.ops as ops
    for name in ("dwconv3x3_fwd", "dwconv3x3_bwd_data", "dwconv3x3_bwd_weight"):
        assert callable(getattr(ops, name))
    assert L.ssd_dwconv3x3_bwd_weight_workspace_bytes.restype is ctypes.c_size_t
