"""GPU: the optimizer kernels (csrc/optim.hip) through the C ABI on one flat buffer of three tensors of 1, 257 and 2 optimizer
blocks (257 blocks: more than the 256 threads of k_clip_scale's loop, so its strided path runs), in strict.Arena with guards and
two poisons, against oracle.ssd_oracle.clip_by_norm / adam_step and a restatement of p -= lr * g * scale, all in float64.

Every comparison is an equality, which the operands are chosen for:
  * clipping: gradients are integers times a power of two whose squared norm is a power of four, and clip is a power of two, so
    norms, scales (1 for the all-zero tensor and the one below the clip norm, 2^-11 above it) and clipped gradients are exact;
  * SGD: lr and grad_scale * scale are powers of two.  With scale == NULL and grad_scale = float32(1/3) the gradients are
    multiples of 3 with few bits: g * float32(1/3) = (g/3)(1 + 2^-25) rounds to g/3 in fp32, and with |p| >= 4 >> lr * g the same
    holds for p - lr * g * float32(1/3) whether or not the compiler fuses it, and for the float64 result rounded to fp32;
  * Adam: beta1 = 0.5, beta2 = 0 (v = g^2, sqrt(v) = |g|), eps = 2^-10 and effective gradients 0 or +-(2^j - 2^-10), so
    sqrt(v) + eps is a power of two and m / (sqrt(v) + eps) exact; lr is chosen per step so that lr_t = lr sqrt(1 - beta2^t) /
    (1 - beta1^t) = 2^-6 exactly.  Parameters stay below 2^4 on a grid of 2^-19: 23 bits.  In the step with scale == NULL and
    grad_scale = float32(1/3) the oracle is given the fp32 product g * grad_scale (the kernel's documented first operation), which
    is exactly the intended gradient by the rounding argument above.
tests/test_engine_gpu.py::test_optimizer_vs_oracle keeps the realistic hyper-parameters with its bounds."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import ssd_oracle as O                                   # noqa: E402
from tests import strict                                             # noqa: E402

F32, BF, I32 = torch.float32, torch.bfloat16, torch.int32
BLOCKS = (1, 257, 2)
EPS = 2.0 ** -10


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ok(status):
    assert status == 0, status


class Flat:
    """the flat buffer's geometry: tensor t owns blocks off[t] .. off[t+1]"""

    def __init__(self, L):
        self.blk = L.ssd_opt_block_elems()
        self.off = np.concatenate([[0], np.cumsum(BLOCKS)]).astype(np.int32)
        self.nb = int(self.off[-1])
        self.n = self.nb * self.blk
        self.block_tensor = np.repeat(np.arange(len(BLOCKS)), BLOCKS).astype(np.int32)
        self.sl = [slice(int(a) * self.blk, int(b) * self.blk) for a, b in zip(self.off[:-1], self.off[1:])]

    def per_element(self, per_tensor):
        return np.repeat(np.asarray(per_tensor, np.float64), [b * self.blk for b in BLOCKS])


def clip_gradient(F, g, second):
    """tensor 0: all zero (norm 0).  tensor 1: 2^18 (or 2^16) entries of +-1 (+-2) spread over all 257 blocks: norm 2^9.
    tensor 2: four (sixteen) entries of 2^-5 (2^-6): norm 2^-4, below clip = 2^-2."""
    out = np.zeros(F.n, np.float64)
    n1 = F.sl[1].stop - F.sl[1].start
    count, mag = (2 ** 16, 2.0) if second else (2 ** 18, 1.0)
    pos = torch.randperm(n1, generator=g)[:count].numpy()
    out[F.sl[1].start + pos] = mag * (torch.randint(0, 2, (count,), generator=g).numpy() * 2 - 1)
    n2 = F.sl[2].stop - F.sl[2].start
    count, mag = (16, 2.0 ** -6) if second else (4, 2.0 ** -5)
    out[F.sl[2].start + torch.randperm(n2, generator=g)[:count].numpy()] = mag
    return out


def f32(a):
    return torch.from_numpy(np.asarray(a, np.float64).astype(np.float32))


def test_clip_scales_accumulate_apply(L):
    F = Flat(L)
    g = torch.Generator().manual_seed(5)
    gA, gB = clip_gradient(F, g, False), clip_gradient(F, g, True)
    clip = 0.25
    norms = [np.sqrt((gA[s] ** 2).sum()) for s in F.sl]
    assert norms == [0.0, 512.0, 0.0625]
    want_scale = [clip / max(n, clip) for n in norms]
    assert want_scale == [1.0, 2.0 ** -11, 1.0]
    clippedA = np.concatenate([O.clip_by_norm(gA[s], clip) for s in F.sl])
    clippedB = np.concatenate([O.clip_by_norm(gB[s], clip) for s in F.sl])
    assert [float(np.linalg.norm(clippedA[s])) for s in F.sl] == [0.0, 0.25, 0.0625]        # above the clip norm: exactly at it

    a = strict.Arena("cuda", strict.Arena.bytes_for(*[4 * F.n] * 6) + (64 << 20))
    grad, off, bt = a.put(f32(gA), "grad"), a.put(torch.from_numpy(F.off), "tensor_block_off"), a.put(torch.from_numpy(F.block_tensor), "block_tensor")
    scale, nrm, ws = a.out((3,), F32, "scale"), a.out((3,), F32, "norms"), a.workspace()

    def clip_scales(c, with_norms=True):
        part = ws.get(8 * F.nb, grad.device)
        ok(L.ssd_grad_clip_scales(ptr(grad), F.n, ptr(off), 3, c, ptr(part), ptr(scale), ptr(nrm) if with_norms else None, stream()))
    a.run(lambda: clip_scales(clip), [(scale, f32(want_scale)), (nrm, f32(norms))])
    a.run(lambda: clip_scales(clip, False), [(scale, f32(want_scale))])                    # norms == NULL
    for c in (0.0, -1.0):                                                                    # clip <= 0: no clipping
        a.run(lambda: clip_scales(c), [(scale, torch.ones(3)), (nrm, f32(norms))])

    # two micro-batches: acc = clip(gA), then acc += clip(gB) with gB's own scales; then acc += gA unscaled (scale == NULL)
    sc = a.put(f32(want_scale), "scale (operand)")
    acc = a.inout(torch.full((F.n,), float("nan")), "acc")
    a.run(lambda: ok(L.ssd_grad_accumulate(ptr(acc), ptr(grad), F.n, ptr(bt), ptr(sc), 1, stream())), [(acc, f32(clippedA))])
    a.set(acc, f32(clippedA))
    a.set(grad, f32(gB))
    normsB = [np.sqrt((gB[s] ** 2).sum()) for s in F.sl]
    scaleB = [clip / max(n, clip) for n in normsB]
    assert normsB == [0.0, 512.0, 0.0625]
    a.run(lambda: clip_scales(clip), [(scale, f32(scaleB)), (nrm, f32(normsB))])
    a.set(sc, f32(scaleB))
    a.run(lambda: ok(L.ssd_grad_accumulate(ptr(acc), ptr(grad), F.n, ptr(bt), ptr(sc), 0, stream())), [(acc, f32(clippedA + clippedB))])
    a.run(lambda: ok(L.ssd_grad_accumulate(ptr(acc), ptr(grad), F.n, None, None, 0, stream())), [(acc, f32(clippedA + gB))])
    # in place: grad *= scale[tensor]
    gio = a.inout(f32(gB), "grad (scaled in place)")
    a.run(lambda: ok(L.ssd_grad_apply_scale(ptr(gio), F.n, ptr(bt), ptr(sc), stream())), [(gio, f32(clippedB))])


def test_sgd_step(L):
    F = Flat(L)
    g = torch.Generator().manual_seed(6)
    p0 = (torch.randint(32, 64, (F.n,), generator=g).double() / 8).numpy()                  # 4 .. 8 on a grid of 1/8
    gr = (torch.randint(-4, 5, (F.n,), generator=g).double() * 3 / 16).numpy()              # multiples of 3/16, |g| <= 3/4
    gr[F.sl[0]] = 0.0
    scales = np.array([1.0, 2.0 ** -3, 0.5])
    lr = 2.0 ** -4
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[4 * F.n] * 4) + (16 << 20))
    grad, bt, sc = a.put(f32(gr), "grad"), a.put(torch.from_numpy(F.block_tensor), "block_tensor"), a.put(f32(scales), "scale")
    p, pb = a.inout(f32(p0), "param"), a.out((F.n,), BF, "param_bf16")
    want = p0 - lr * gr * 0.5 * F.per_element(scales)
    a.run(lambda: ok(L.ssd_sgd_step(ptr(p), ptr(grad), ptr(pb), F.n, ptr(bt), ptr(sc), 0.5, lr, stream())), [(p, f32(want)), (pb, f32(want).to(BF))])
    third = float(np.float32(1.0 / 3.0))
    want = p0 - lr * gr * third                                                             # scale == NULL
    assert np.array_equal(want.astype(np.float32), (p0 - lr * gr / 3).astype(np.float32))
    a.run(lambda: ok(L.ssd_sgd_step(ptr(p), ptr(grad), ptr(pb), F.n, None, None, third, lr, stream())), [(p, f32(want)), (pb, f32(want).to(BF))])
    a.run(lambda: ok(L.ssd_sgd_step(ptr(p), ptr(grad), None, F.n, None, None, third, lr, stream())), [(p, f32(want))])       # param_bf16 == NULL


def test_adam_steps(L):
    F = Flat(L)
    g = torch.Generator().manual_seed(7)
    b1, b2, lr_t = 0.5, 0.0, 2.0 ** -6
    mags = torch.tensor([0.5 - EPS, 1.0 - EPS, 2.0 - EPS], dtype=torch.float64)

    def effective():                     # what the moments must see: 0 on tensor 0, +-(2^j - eps) elsewhere
        e = mags[torch.randint(0, 3, (F.n,), generator=g)] * (torch.randint(0, 2, (F.n,), generator=g) * 2 - 1)
        e = e.numpy()
        e[F.sl[0]] = 0.0
        return e

    scales = np.array([1.0, 2.0 ** -11, 1.0])
    third = float(np.float32(1.0 / 3.0))
    # (what the kernel is given: grad, scale or None, grad_scale, param_bf16 or not), per step
    e1, e2, e3 = effective(), effective(), effective()
    steps = [(e1 / (0.5 * F.per_element(scales)), True, 0.5, True),
             (e2 * 3.0, False, third, True),
             (e3 / F.per_element(scales), True, 1.0, False)]
    p = (torch.randint(-64, 65, (F.n,), generator=g).double() / 8).numpy()
    m, v = np.zeros(F.n), np.zeros(F.n)

    a = strict.Arena("cuda", strict.Arena.bytes_for(*[4 * F.n] * 6) + (16 << 20))
    grad, bt, sc = a.put(f32(steps[0][0]), "grad"), a.put(torch.from_numpy(F.block_tensor), "block_tensor"), a.put(f32(scales), "scale")
    pd, md, vd, pb = a.inout(f32(p), "param"), a.inout(f32(m), "m"), a.inout(f32(v), "v"), a.out((F.n,), BF, "param_bf16")
    for t, (gk, use_scale, gs, want_bf16) in enumerate(steps, 1):
        assert np.array_equal(gk.astype(np.float32).astype(np.float64), gk)                 # the gradient handed over is exact in fp32
        geff = gk * gs * (F.per_element(scales) if use_scale else 1.0)
        if not use_scale:
            geff = (gk.astype(np.float32) * np.float32(gs)).astype(np.float64)              # the kernel's fp32 product g * grad_scale
        assert np.array_equal(geff, (e1, e2, e3)[t - 1])
        lr = lr_t * (1 - b1 ** t)                                                           # so that the oracle's lr_t is 2^-6 exactly
        p, m, v = O.adam_step(p, geff, m, v, t, lr, beta1=b1, beta2=b2, eps=EPS)
        for arr in (p, m, v):
            assert np.array_equal(arr.astype(np.float32).astype(np.float64), arr)           # the regime: the oracle's state is exact in fp32
        a.set(grad, f32(gk))
        want = [(pd, f32(p)), (md, f32(m)), (vd, f32(v))] + ([(pb, f32(p).to(BF))] if want_bf16 else [])
        a.run(lambda: ok(L.ssd_adam_step(ptr(pd), ptr(grad), ptr(md), ptr(vd), ptr(pb) if want_bf16 else None, F.n, ptr(bt) if use_scale else None,
                                      ptr(sc) if use_scale else None, gs, lr_t, b1, b2, EPS, stream())), want)
        for tns, arr in ((pd, p), (md, m), (vd, v)):
            a.set(tns, f32(arr))
    assert len(np.unique(f32(p).to(BF).float().numpy() - p)) > 100                          # the bf16 copy does round
