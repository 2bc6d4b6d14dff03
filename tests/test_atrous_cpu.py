"""CPU suite of the atrous convolution / 3x3 stride-1 pooling: the oracle (tests/atrous_oracle.py) against independent
statements, the exact-arithmetic regime of every GPU case of tests/test_atrous_strict_gpu.py, and the host-side refusals of the
C ABI (decided before any launch: callable without a GPU, with pointers that are never dereferenced)."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F                                                    # noqa: E402

from tests import strict                                                           # noqa: E402
from tests.atrous_oracle import CASES, POOL_CASES, atrous_case, pool3x3s1_case, ref_atrous   # noqa: E402


# ---------------------------------------------------------------- the oracle
def test_dilation_one_is_the_ordinary_convolution():
    a = atrous_case((2, 5, 5, 64, 64, 1))
    r = strict.conv_reference((2, 5, 5, 64, 64, 3, 1, "same"))
    for name in ("x", "w", "dy", "y", "y_relu", "dx", "dx_acc", "dw", "dbias", "w_t", "dy_pad"):
        assert torch.equal(a[name], r[name]), name


def test_dilation_six_is_nine_shifted_matmuls():
    B, H, W, Cin, Cout, d = case = (1, 7, 7, 64, 64, 6)
    a = atrous_case(case)
    x, w = a["x"].float(), a["w"].float()
    xp = F.pad(x, (0, 0, d, d, d, d))
    y = a["bias"].expand(B, H, W, Cout).clone()
    for ty in range(3):
        for tx in range(3):
            y += xp[:, ty * d:ty * d + H, tx * d:tx * d + W, :] @ w[:, ty, tx, :].t()
    assert torch.equal(y, a["y"])
    assert torch.equal(ref_atrous(a["x"], a["w"], a["bias"], d, True, torch.float32), a["y_relu"])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_regime_and_fp32_equals_float64(case):
    r = atrous_case(case)
    strict.check_regime(r)
    r64 = atrous_case(case, torch.float64)
    for name in ("y", "y_relu", "dx", "dx_masked", "dx_acc", "dw", "dbias"):
        assert torch.equal(r[name].double(), r64[name]), (case, name)
    B, H, W, Cin, Cout, d = case
    dead = [(ty, tx) for ty in range(3) for tx in range(3) if (ty != 1 and d >= H) or (tx != 1 and d >= W)]
    for ty, tx in dead:
        assert not r["dw"][:, ty, tx, :].any()
    if d >= max(H, W):
        assert len(dead) == 8 and r["dw"][:, 1, 1, :].any()


@pytest.mark.parametrize("shape", POOL_CASES, ids=str)
def test_pool_oracle(shape):
    r = pool3x3s1_case(*shape)
    strict.check_regime(r)
    want = F.max_pool2d(r["x"].float().permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1)
    assert torch.equal(r["y"], want)
    assert float(r["dx"].abs().max()) <= 18
    assert bool(((r["code"] == 15) == (r["y"] <= 0)).all())


# ---------------------------------------------------------------- the C ABI, host side
@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib, _lib.lib()


def P(i):
    """distinct pointers 256 MiB apart, never dereferenced on a refused call"""
    return ctypes.c_void_p(0x10000000 * (i + 1))


def test_atrous_fwd_refuses_on_the_host(lib):
    _lib, L = lib
    V, U = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    ok = dict(x=P(0), w=P(1), bias=P(2), y=P(3), B=2, H=19, W=19, Cin=64, Cout=72, d=6)

    def call(**kv):
        a = dict(ok, **kv)
        return L.ssd_conv2d_atrous_fwd(a["x"], a["w"], a["bias"], a["y"], a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["d"], 1, None)

    for kv in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(H=0), dict(W=-1), dict(d=0), dict(y=ok["x"]),
               dict(y=ok["w"]), dict(y=ok["bias"]), dict(y=ctypes.c_void_p(ok["x"].value + 64))):
        assert call(**kv) == V, kv
    for kv in (dict(Cin=96), dict(Cin=32), dict(Cout=12), dict(B=1 << 14, H=64, W=64, Cin=1024)):
        assert call(**kv) == U, kv


def test_atrous_bwd_data_refuses_on_the_host(lib):
    _lib, L = lib
    V, U = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    ok = dict(dy=P(0), w_t=P(1), src=None, dx=P(3), B=2, H=19, W=19, Cin=64, cp=72, d=6)

    def call(**kv):
        a = dict(ok, **kv)
        return L.ssd_conv2d_atrous_bwd_data(a["dy"], a["w_t"], a["src"], a["dx"], a["B"], a["H"], a["W"], a["Cin"], a["cp"], a["d"], 0, None)

    for kv in (dict(dy=None), dict(w_t=None), dict(dx=None), dict(B=0), dict(H=0), dict(W=0), dict(d=0), dict(dx=ok["dy"]),
               dict(dx=ok["w_t"])):
        assert call(**kv) == V, kv
    for kv in (dict(Cin=96), dict(cp=76), dict(B=1 << 14, H=64, W=64, cp=1024)):
        assert call(**kv) == U, kv


def test_atrous_bwd_weight_refuses_on_the_host(lib):
    _lib, L = lib
    V, U, WS = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED, _lib.SSD_ERR_WORKSPACE
    ok = dict(x=P(0), dy=P(1), dw=P(2), db=P(3), B=2, H=19, W=19, Cin=64, Cout=72, ldy=72, d=6, ws=P(4), short=0)
    q = L.ssd_conv2d_atrous_bwd_weight_workspace_bytes
    need = q(2, 19, 19, 64, 72, 72, 6)
    assert need > 0 and need % 4 == 0
    assert q(2, 19, 19, 96, 72, 72, 6) == 0 and q(2, 19, 19, 64, 76, 76, 6) == 0 and q(2, 19, 19, 64, 72, 64, 6) == 0
    assert q(2, 19, 19, 64, 72, 72, 0) == 0
    # beyond the map only the centre tap is live: one tap's columns instead of nine
    assert q(2, 19, 19, 64, 72, 72, 19) < need and q(2, 19, 19, 64, 72, 72, 19) == q(2, 19, 19, 64, 72, 72, 1000)

    def call(**kv):
        a = dict(ok, **kv)
        size = q(a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["ldy"], a["d"]) - a["short"]
        return L.ssd_conv2d_atrous_bwd_weight(a["x"], a["dy"], a["dw"], a["db"], a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["ldy"],
                                              a["d"], a["ws"], max(size, 0), None)

    for kv in (dict(x=None), dict(dy=None), dict(dw=None), dict(B=0), dict(H=0), dict(W=0), dict(d=0), dict(dw=ok["x"]),
               dict(dw=ok["dy"]), dict(db=ok["dy"])):
        assert call(**kv) == V, kv
    for kv in (dict(Cin=96), dict(Cout=76, ldy=80), dict(ldy=64)):
        assert call(**kv) == U, kv
    assert call(short=1) == WS and call(ws=None) == WS          # the code ssd_conv2d_bwd_weight returns for a short workspace


def test_maxpool3x3s1_refuses_on_the_host(lib):
    _lib, L = lib
    V, U = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    a, b, c = P(0), P(1), P(2)
    f, g = L.ssd_maxpool3x3s1_fwd, L.ssd_maxpool3x3s1_bwd
    for args in ((None, b, c, 2, 19, 19, 64), (a, None, c, 2, 19, 19, 64), (a, b, None, 2, 19, 19, 64), (a, b, c, 0, 19, 19, 64),
                 (a, b, c, 2, 0, 19, 64), (a, b, c, 2, 19, 0, 64), (a, a, c, 2, 19, 19, 64), (a, b, a, 2, 19, 19, 64), (a, b, b, 2, 19, 19, 64)):
        assert f(*args, None) == V, args
    for args in ((None, b, c, 2, 19, 19, 64), (a, None, c, 2, 19, 19, 64), (a, b, None, 2, 19, 19, 64), (a, b, c, 0, 19, 19, 64),
                 (a, b, c, 2, 0, 19, 64), (a, b, c, 2, 19, 0, 64), (a, b, b, 2, 19, 19, 64), (a, b, a, 2, 19, 19, 64)):
        assert g(*args, None) == V, args
    for fn in (f, g):
        assert fn(a, b, c, 2, 19, 19, 12, None) == U
        assert fn(a, b, c, 1 << 12, 64, 64, 1024, None) == U
