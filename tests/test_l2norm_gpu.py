"""GPU: the L2 normalisation kernels (ssd_l2norm_fwd / ssd_l2norm_bwd, csrc/l2norm.hip) against the float64 oracle of
tests/l2norm_oracle.py under that module's derived bounds, inside strict.Arena: outputs and workspace between guard bands,
every run under both poisons.  The arena compares bits, the oracle comparison has bounds, so each test runs the call once,
holds that result to the bounds, and then hands it to Arena.run as the reference: guards, inputs, every element written, and
the same bits under the other poison and from a second run.

Shapes: one pixel; pixel counts that leave partial workgroups (4 waves = 4 pixels per round) and lanes without channels
(C = 128, 256); two 16-byte vectors per lane (C = 1024); the engine's own two-image map; and l2norm_oracle.EXTRA_SHAPES, three
trips of both capped grids (tests/sweep_cases.py)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import l2norm_oracle as O                                 # noqa: E402
from tests import strict                                             # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
ALL_SHAPES = O.SHAPES + O.EXTRA_SHAPES
_CASES = {}


def case(shape):
    """inputs, float64 references and bounds of a shape, computed once (of the large extra shapes only the latest is kept)"""
    if shape not in _CASES:
        for old in [s for s in _CASES if s in O.EXTRA_SHAPES]:
            del _CASES[old]
        k = O.make_case(*shape)
        k["y64"], k["r64"], _ = O.fwd64(k["x"], k["s"])
        for name, old in (("", None), ("_acc", k["old"])):
            k["dx64" + name], k["ds64"] = O.bwd64(k["dy"], k["x"], k["s"], old=old)
            k["bounds" + name] = O.bounds(k["dy"], k["x"], k["s"], old=old)
        _CASES[shape] = k
    return _CASES[shape]


def t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def f64(x):
    return x.float().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops
    return ops


def first_run(a, fn, outs):
    a.poison(False)
    fn()
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs]


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_forward(ops, shape):
    k = case(shape)
    P, C = shape
    a = strict.Arena("cuda", strict.Arena.bytes_for(2 * P * C, 4 * C, 2 * P * C, 4 * P))
    x, s = a.put(t(k["x"], BF), "x"), a.put(t(k["s"], F32), "scale")
    y, r = a.out((P, C), BF, "y"), a.out((P,), F32, "rnorm")
    fn = lambda: ops.l2norm_fwd(x, s, out=y, rnorm=r)
    got_y, got_r = first_run(a, fn, (y, r))
    b = k["bounds"]
    figures = dict(y=O.worst(f64(got_y), k["y64"], b["y"]), r=O.worst(f64(got_r), k["r64"], b["r"]))
    print(shape, figures, "y not bit-equal to bf16(y64): %.2e" % float((f64(got_y) != O.bf16_round(k["y64"].astype(np.float32))).mean()))
    assert all(v <= 1.0 for v in figures.values()), figures
    if P > 1:
        assert float(got_y[P // 2].float().abs().max()) == 0.0          # the all-zero pixel
    a.run(fn, [(y, got_y), (r, got_r)])
    # without rnorm: the same y, and the rnorm tensor keeps its poison
    a.run(lambda: ops.l2norm_fwd(x, s, out=y), [(y, got_y)])


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_backward(ops, shape, accumulate):
    k = case(shape)
    P, C = shape
    sfx = "_acc" if accumulate else ""
    L = ops._lib.lib()
    wsb = L.ssd_l2norm_ws_bytes(P, C)
    assert wsb > 0
    a = strict.Arena("cuda", strict.Arena.bytes_for(2 * P * C, 2 * P * C, 4 * C, 4 * P, 2 * P * C, 4 * C, wsb))
    dy, x, s = a.put(t(k["dy"], BF), "dy"), a.put(t(k["x"], BF), "x"), a.put(t(k["s"], F32), "scale")
    _, r_fwd = ops.l2norm_fwd(t(k["x"], BF).cuda(), t(k["s"], F32).cuda(), rnorm=True)      # what the forward pass saves
    r = a.put(r_fwd, "rnorm")
    dx = a.inout(t(k["old"], BF), "dx") if accumulate else a.out((P, C), BF, "dx")
    ds = a.out((C,), F32, "dscale")
    ws = a.workspace()                                                  # exactly ssd_l2norm_ws_bytes, poisoned
    saved = lambda: ops.l2norm_bwd(dy, x, s, rnorm=r, out=dx, accumulate=accumulate, dscale=ds, ws=ws)
    got_dx, got_ds = first_run(a, saved, (dx, ds))
    b = k["bounds" + sfx]
    figures = dict(dx=O.worst(f64(got_dx), k["dx64" + sfx], b["dx"]), ds=O.worst(f64(got_ds), k["ds64"], b["ds"]))
    print(shape, "accumulate" if accumulate else "write", figures)
    assert all(v <= 1.0 for v in figures.values()), figures
    a.run(saved, [(dx, got_dx), (ds, got_ds)])
    # rnorm recomputed from x: the same bits as with the forward pass's
    a.run(lambda: ops.l2norm_bwd(dy, x, s, rnorm=None, out=dx, accumulate=accumulate, dscale=ds, ws=ws),
          [(dx, got_dx), (ds, got_ds)])


def test_two_runs_are_bit_identical(ops):
    """ds is a sum over all pixels by 722 workgroups: fixed-order partials, no atomics -- plain tensors, three runs"""
    k = case((2 * 1444, 512))
    dy, x, s = t(k["dy"], BF).cuda(), t(k["x"], BF).cuda(), t(k["s"], F32).cuda()
    runs = []
    for _ in range(3):
        y, r = ops.l2norm_fwd(x, s, rnorm=True)
        dx, ds = ops.l2norm_bwd(dy, x, s, rnorm=r)
        runs.append((y, r, dx, ds))
    torch.cuda.synchronize()
    for other in runs[1:]:
        for u, v in zip(runs[0], other):
            assert torch.equal(u, v)


@pytest.mark.parametrize("C", [64, 192, 1152])
def test_unsupported_widths_launch_nothing(ops, C):
    P = 5
    a = strict.Arena("cuda", strict.Arena.bytes_for(2 * P * C, 2 * P * C, 4 * C, 2 * P * C, 4 * P, 2 * P * C, 4 * C, 4096))
    g = torch.Generator().manual_seed(C)
    x, dy = a.put(torch.rand((P, C), generator=g).to(BF), "x"), a.put(torch.rand((P, C), generator=g).to(BF), "dy")
    s = a.put(torch.full((C,), 20.0), "scale")
    y, r, dx, ds = a.out((P, C), BF, "y"), a.out((P,), F32, "rnorm"), a.out((P, C), BF, "dx"), a.out((C,), F32, "dscale")
    assert ops._lib.lib().ssd_l2norm_ws_bytes(P, C) == 0
    ws = a.workspace()

    def fn():
        with pytest.raises(NotImplementedError):
            ops.l2norm_fwd(x, s, out=y, rnorm=r)
        with pytest.raises(NotImplementedError):
            ops.l2norm_bwd(dy, x, s, out=dx, dscale=ds, ws=ws)
    a.run(fn, [])                                                       # no output listed: every one keeps its poison


def test_missing_pointers_and_small_workspace(ops):
    _lib = ops._lib
    L = _lib.lib()
    P, C = 6, 128
    x = torch.rand((P, C), device="cuda").to(BF)
    dy = torch.rand((P, C), device="cuda").to(BF)
    s = torch.full((C,), 20.0, device="cuda")
    with pytest.raises(ValueError):
        ops.l2norm_fwd(x, None)
    with pytest.raises(ValueError):
        ops.l2norm_bwd(dy, x, None)
    with pytest.raises(ValueError):
        ops.l2norm_fwd(x, s, out=x)                                      # y may not alias x
    p = lambda v: ctypes.c_void_p(v.data_ptr())
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    y, dx, ds = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(s)
    wsb = L.ssd_l2norm_ws_bytes(P, C)
    ws = torch.zeros((wsb,), dtype=torch.uint8, device="cuda")
    for args in ((null, p(s), p(y)), (p(x), null, p(y)), (p(x), p(s), null)):
        assert L.ssd_l2norm_fwd(*args, null, P, C, 1e-10, st) == _lib.SSD_ERR_VALUE
    good = [p(dy), p(x), p(s), null, p(dx), 0, p(ds), p(ws), wsb]
    for i in (0, 1, 2, 4, 6, 7):
        args = list(good)
        args[i] = null
        assert L.ssd_l2norm_bwd(*args, P, C, 1e-10, st) == _lib.SSD_ERR_VALUE, i
    assert L.ssd_l2norm_bwd(*good[:8], wsb - 1, P, C, 1e-10, st) == _lib.SSD_ERR_VALUE
    assert L.ssd_l2norm_bwd(*good, 0, C, 1e-10, st) == _lib.SSD_ERR_VALUE
    assert L.ssd_l2norm_bwd(*good, P, C, 1e-10, st) == _lib.SSD_OK
    torch.cuda.synchronize()
    assert float(y.float().abs().max()) == 0.0                           # (no refused forward call wrote it)
