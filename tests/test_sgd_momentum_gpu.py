"""GPU: momentum SGD with weight decay (ssd_sgd_momentum_step, csrc/optim.hip) from the kernel up to the trainer.

test_momentum_steps_exact runs the kernel through the C ABI on the flat buffer of tests/test_optim_gpu.py (three tensors of 1, 257
and 2 optimizer blocks) in strict.Arena with guards and two poisons; every comparison is an equality against tests/sgd_oracle.py
(float64) rounded to fp32, which the operands are chosen for:
  * momentum = 1/2, lr, grad_scale * scale[t] and decay[t] are powers of two; parameters start on a grid of 2^-3 below 2^3,
    gradients on a grid of 2^-2 (multiples of 3/16 where grad_scale = float32(1/3): g * float32(1/3) = (g/3)(1 + 2^-25) rounds to
    g/3, the argument of test_optim_gpu.test_sgd_step);
  * a step without decay refines the grid of p and v by one bit (momentum * v) -- two with Nesterov; decay * p refines it by
    lr * decay = 2^-4 per step besides.  Three carried steps from the coarsest operand grid 2^-6 stay above 2^-19: with
    |p| < 2^4 that is 23 bits, and every intermediate (ge, lr * ge, momentum * v', their sums) is a sum of two such numbers.
    So no operation rounds, and the result is the same whether or not the compiler contracts a multiply-add.
The regime is asserted on the oracle, never on what the kernel returned: after each step p, v and the intermediates must
round-trip through fp32 unchanged.  The state is re-seeded between sequences.

The other tests drive the engine and the model: realistic hyper-parameters against the oracle with a derived bound, the
per-bucket update inside the backward pass against the whole-buffer one, the clip setting, checkpoints, the paper's recipe end to
end and one data-parallel rank."""
import ctypes
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import ssd_oracle as O                                   # noqa: E402
from tests import strict                                             # noqa: E402
from tests.sgd_oracle import sgd_momentum_step                       # noqa: E402

F32, BF = torch.float32, torch.bfloat16
BLOCKS = (1, 257, 2)
U = 2.0 ** -24                                                       # one fp32 rounding, relative to its result


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


def f32(a):
    return torch.from_numpy(np.asarray(a, np.float64).astype(np.float32))


def exact32(a):
    a = np.asarray(a, np.float64)
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


class Flat:
    """the flat buffer's geometry: tensor t owns blocks off[t] .. off[t+1]"""

    def __init__(self, blk):
        self.blk = blk
        self.off = np.concatenate([[0], np.cumsum(BLOCKS)]).astype(np.int32)
        self.n = int(self.off[-1]) * blk
        self.block_tensor = np.repeat(np.arange(len(BLOCKS)), BLOCKS).astype(np.int32)
        self.sl = [slice(int(a) * blk, int(b) * blk) for a, b in zip(self.off[:-1], self.off[1:])]

    def per_element(self, per_tensor):
        return np.repeat(np.asarray(per_tensor, np.float64), [b * self.blk for b in BLOCKS])


THIRD = float(np.float32(1.0 / 3.0))
SCALES = np.array([1.0, 2.0 ** -3, 0.5])
# name -> momentum, nesterov, lr, grad_scale, scale table?, decay table or None, param_bf16?, carried steps
SEQUENCES = {
    "plain": dict(mom=0.5, nesterov=False, lr=2.0 ** -4, gs=0.5, scale=True, decay=None, bf16=True, steps=3),
    "nesterov": dict(mom=0.5, nesterov=True, lr=2.0 ** -4, gs=1.0, scale=True, decay=None, bf16=False, steps=3),
    "decay": dict(mom=0.5, nesterov=False, lr=2.0 ** -2, gs=0.5, scale=True, decay=[0.0, 2.0 ** -2, 0.0], bf16=True, steps=3),
    "nesterov decay": dict(mom=0.5, nesterov=True, lr=2.0 ** -2, gs=0.5, scale=True, decay=[0.0, 2.0 ** -2, 2.0 ** -1], bf16=False,
                           steps=3),
    "decay only": dict(mom=0.5, nesterov=False, lr=2.0 ** -2, gs=1.0, scale=False, decay=[2.0 ** -1, 2.0 ** -2, 0.0], bf16=True,
                       steps=2),                     # tensor 0 (no gradient) decays: the L2 term alone moves it
    "no tables, 1/3": dict(mom=0.5, nesterov=False, lr=2.0 ** -4, gs=THIRD, scale=False, decay=None, bf16=True, steps=2,
                           no_block_tensor=True),
    "no momentum": dict(mom=0.0, nesterov=False, lr=2.0 ** -4, gs=0.5, scale=True, decay=None, bf16=True, steps=2),
}


def sequence(F, name):
    """The operands and the oracle's states of a sequence: p0, [(g, p, v)] per step, asserting the exact regime on the way."""
    q = SEQUENCES[name]
    g = torch.Generator().manual_seed(11 + sorted(SEQUENCES).index(name))
    p = (torch.randint(-64, 65, (F.n,), generator=g).double() / 8).numpy()               # |p| <= 8 on a grid of 1/8
    v = np.zeros(F.n)
    third = q["gs"] == THIRD
    sc_tab = F.per_element(SCALES) if q["scale"] else 1.0
    dec = F.per_element(q["decay"]) if q["decay"] is not None else None
    p0, out = p, []
    for _ in range(q["steps"]):
        if third:
            gr = (torch.randint(-4, 5, (F.n,), generator=g).double() * 3 / 16).numpy()   # multiples of 3/16
        else:
            gr = (torch.randint(-4, 5, (F.n,), generator=g).double() / 4).numpy()        # grid 1/4, |g| <= 1
        gr[F.sl[0]] = 0.0                                                                # tensor 0: no gradient
        assert exact32(gr)
        if third:       # the kernel's fp32 product g * grad_scale, which is exactly the intended g / 3
            sc_g = (gr.astype(np.float32) * np.float32(THIRD)).astype(np.float64)
            assert np.array_equal(sc_g, gr / 3)
            ge = sc_g
        else:
            ge = gr * (q["gs"] * sc_tab)
        p1, v1 = sgd_momentum_step(p, ge, v, q["lr"], q["mom"], q["nesterov"], 1.0, dec)
        # the regime: the state and every intermediate of the documented order are fp32 numbers
        full = ge + dec * p if dec is not None else ge
        for arr in (p1, v1, ge, full, q["lr"] * full, q["mom"] * v, q["mom"] * v1, q["mom"] * v1 - q["lr"] * full):
            assert exact32(arr), name
        out.append((gr, p1, v1))
        p, v = p1, v1
    return p0, out


def test_momentum_steps_exact(L):
    F = Flat(L.ssd_opt_block_elems())
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[4 * F.n] * 8) + (16 << 20))
    grad = a.put(torch.zeros(F.n), "grad")
    bt = a.put(torch.from_numpy(F.block_tensor), "block_tensor")
    sc = a.put(f32(SCALES), "scale")
    dc = a.put(torch.zeros(3), "decay")
    pd, vd = a.inout(torch.zeros(F.n), "param"), a.inout(torch.zeros(F.n), "velocity")
    pb = a.out((F.n,), BF, "param_bf16")
    ps = a.inout(torch.zeros(F.n), "param (ssd_sgd_step)")
    rounds = False
    for name, q in SEQUENCES.items():
        p0, steps = sequence(F, name)
        a.set(pd, f32(p0))                                        # re-seeded: every sequence starts from its own state
        a.set(vd, torch.zeros(F.n))
        if q["decay"] is not None:
            a.set(dc, f32(q["decay"]))
        use_bt = not q.get("no_block_tensor", False)
        p_prev = p0
        for k, (gr, p, v) in enumerate(steps):
            a.set(grad, f32(gr))
            want = [(pd, f32(p)), (vd, f32(v))] + ([(pb, f32(p).to(BF))] if q["bf16"] else [])
            a.run(lambda: ok(L.ssd_sgd_momentum_step(
                ptr(pd), ptr(grad), ptr(vd), ptr(pb) if q["bf16"] else None, F.n, ptr(bt) if use_bt else None,
                ptr(sc) if q["scale"] else None, ptr(dc) if q["decay"] is not None else None, q["gs"], q["lr"], q["mom"],
                1 if q["nesterov"] else 0, stream())), want)
            if k >= 1 and q["mom"] > 0:                              # a carried step depends on the velocity
                p_cold, _ = sgd_momentum_step(p_prev, gr, np.zeros(F.n), q["lr"], q["mom"], q["nesterov"],
                                              q["gs"] * (F.per_element(SCALES) if q["scale"] else 1.0),
                                              F.per_element(q["decay"]) if q["decay"] is not None else None)
                assert not np.array_equal(p_cold[F.sl[1]], p[F.sl[1]]), name
            if q["decay"] is None or q["decay"][0] == 0.0:           # zero gradient, no decay: p unchanged, v stays 0
                assert np.array_equal(p[F.sl[0]], p0[F.sl[0]]) and not v[F.sl[0]].any(), name
            else:                                                    # zero gradient, decay: every non-zero p shrinks, v follows
                moved = p[F.sl[0]] != p_prev[F.sl[0]]
                assert np.array_equal(moved, p_prev[F.sl[0]] != 0) and moved.sum() > F.blk // 2, name
                assert (np.abs(p[F.sl[0]]) <= np.abs(p_prev[F.sl[0]])).all() and np.array_equal(v[F.sl[0]] != 0, moved), name
            if name == "no momentum":
                # momentum 0, no decay: ssd_sgd_step on the same operands, bit for bit; v' = -lr * ge is still written
                a.set(ps, f32(p_prev))
                a.run(lambda: ok(L.ssd_sgd_step(ptr(ps), ptr(grad), None, F.n, ptr(bt), ptr(sc), q["gs"], q["lr"], stream())),
                      [(ps, f32(p))])
                assert np.array_equal(v, -q["lr"] * gr * q["gs"] * F.per_element(SCALES)) and v[F.sl[1]].any()
            if q["bf16"]:
                rounds = rounds or len(np.unique(f32(p).to(BF).double().numpy() - p)) > 100
            a.set(pd, f32(p))
            a.set(vd, f32(v))
            p_prev = p
    assert rounds                                                    # the bf16 copy does round


# ---- the engine -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine():
    from ssd_object_detection_amd.engine import SSDEngine
    return SSDEngine(classes=81, seed=3)


def realistic_bound(steps, nesterov, lr, mom, wd, pmax, gemax, vmax):
    """The bound of test_momentum_vs_oracle_realistic from the oracle's magnitudes (its docstring)."""
    e_ge = 8 * U * gemax
    e_step = lr * e_ge + 2 * U * lr * gemax
    e_v = e_p = 0.0
    for _ in range(steps):
        e_step_k = e_step + lr * wd * e_p
        e_v = mom * e_v + e_step_k + 3 * U * vmax
        e_p = e_p + (mom * e_v + e_step_k + 3 * U * vmax if nesterov else e_v) + U * pmax
    return e_p


@pytest.mark.parametrize("nesterov", [False, True])
def test_momentum_vs_oracle_realistic(engine, nesterov):
    """clip 0.01 + momentum 0.9 + weight decay 5e-4 on the filters + lr 1e-3 over the engine's flat buffer, three steps, against
    the float64 oracle with the partition taken from the reference's layer list (test_engine_gpu.reference_variables).

    The bound, from the fp32 roundings of one step (each at most U = 2^-24 of its result) and the ORACLE's magnitudes pmax = max|p|,
    gemax = max|ge|, vmax = max|v| over the steps:
      ge    the clip scale carries 3 roundings (the norm, the quotient, grad_scale * scale), g * sc one, decay * p and the sum
            one each; fp32(decay) one more, one spare:            e_ge <= 8 U gemax
      lr*ge the product and fp32(lr):                             e_step <= lr e_ge + 2 U lr gemax (+ lr decay e_p: the error
            of p that the decay term feeds back)
      v'    fp32(momentum), the product and the difference:       e_v' <= momentum e_v + e_step + 3 U vmax
      p'    the last sum rounds at |p|:                           e_p' <= e_p + e_v' + U pmax
            (Nesterov: momentum * v' - lr * ge first:             e_p' <= e_p + momentum e_v' + e_step + 3 U vmax + U pmax)
    With |p| < 0.1, |ge| <= 0.0101, |v| < 3e-5 the last term dominates: about 3 x 6e-9 = 2e-8, a hundredth of the 2e-6 that
    test_optimizer_vs_oracle holds Adam to at the same parameter scale (asserted below)."""
    from tests.test_engine_gpu import reference_variables
    lr, mom, wd, steps = 1e-3, 0.9, 5e-4, 3
    g = torch.Generator().manual_seed(2)
    engine.init_params(seed=3)
    ref = reference_variables(engine)
    grad = torch.zeros(engine.n_flat)
    bias0 = torch.zeros(engine.n_flat)
    for i, (name, off, numel) in enumerate(ref):
        scale = 10.0 ** (-(i % 5))                                    # some variables above, some below the 0.01 clip norm
        grad[off:off + numel] = torch.randn(numel, generator=g) * scale / np.sqrt(numel)
        if name.endswith("bias"):                                     # (Keras starts biases at 0: decay could not show on them)
            bias0[off:off + numel] = (torch.rand(numel, generator=g) - 0.5) * 0.2
    try:
        engine.param.add_(bias0.cuda())
        engine.refresh_weights(cast=True)
        p0 = engine.param.cpu().numpy().astype(np.float64)
        engine.grad.copy_(grad)
        engine.clip_scales(0.01)
        table = engine.decay_table(wd)
        assert table is engine.decay_table(wd, False) and table is not engine.decay_table(wd, True)
        want_tab = [np.float32(wd) if t.name.endswith("kernel") else np.float32(0) for t in engine.tensors]
        assert table.dtype == torch.float32 and table.cpu().numpy().tolist() == want_tab
        assert engine.decay_table(wd, True).cpu().numpy().tolist() == [np.float32(wd)] * len(engine.tensors)
        v_before = engine.adam_v.clone()
        for _ in range(steps):
            engine.sgd_momentum(lr, engine.grad, 1.0, True, mom, nesterov, table)
        got = engine.param.cpu().numpy().astype(np.float64)
        assert torch.equal(engine.param_bf16, engine.param.bfloat16())    # the bf16 copy the convolutions read: one rounding
        assert torch.equal(engine.adam_v, v_before) and engine.slots == "sgd_momentum"
        gnp = grad.numpy().astype(np.float64)
        p, pb = p0.copy(), p0.copy()                                   # the oracle, and the oracle that decays the biases too
        v, vb = np.zeros_like(p0), np.zeros_like(p0)
        pmax = gemax = vmax = 0.0
        for _ in range(steps):
            for name, off, numel in ref:
                sl = slice(off, off + numel)
                clipped = O.clip_by_norm(gnp[sl], 0.01)
                kernel = name.endswith("kernel")
                gemax = max(gemax, float(np.abs(clipped + (wd * p[sl] if kernel else 0.0)).max()))
                p[sl], v[sl] = sgd_momentum_step(p[sl], clipped, v[sl], lr, mom, nesterov, 1.0, wd if kernel else None)
                pb[sl], vb[sl] = sgd_momentum_step(pb[sl], clipped, vb[sl], lr, mom, nesterov, 1.0, wd)
            pmax, vmax = max(pmax, float(np.abs(p).max())), max(vmax, float(np.abs(v).max()))
        bound = realistic_bound(steps, nesterov, lr, mom, wd, pmax, gemax, vmax)
        err = float(np.abs(got - p).max())
        print("nesterov %s: max|p - oracle| %.3e, bound %.3e (pmax %.3g gemax %.3g vmax %.3g)" % (nesterov, err, bound, pmax, gemax, vmax))
        assert bound <= 2e-6
        assert err <= bound
        # biases received no decay: the oracle that decays them is another function, further from the kernel than the bound
        is_bias = np.zeros(engine.n_flat, bool)
        for name, off, numel in ref:
            if name.endswith("bias"):
                is_bias[off:off + numel] = True
        assert float(np.abs(pb - p)[is_bias].max()) > 4 * bound
        assert float(np.abs(got - pb)[is_bias].max()) > 2 * bound and np.array_equal(pb[~is_bias], p[~is_bias])
    finally:
        engine.init_params(seed=3)
        engine.slots = "adam"


# ---- the model ---------------------------------------------------------------------------------------------------------
def make_model(tmp_path, seed=1, **kw):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    return SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path), seed=seed, timestamp_dir=False, **kw)


def fixed_batch(model, B=4, first=900):
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    cls_l, box_l = synth_batch_gt(first, B)
    image, (cls, loc, mask) = model.make_batch([synth_image(first + i) for i in range(B)], cls_l, box_l)
    return image, cls, loc, mask


def same_state(a, b, names=("param", "adam_m", "adam_v", "param_bf16")):
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for i in a.w_t:
        assert torch.equal(a.w_t[i], b.w_t[i]), i
    for x, y in zip(a.head_w_t, b.head_w_t):
        assert torch.equal(x, y)


def test_fused_equals_unfused_bitwise(tmp_path):
    """Momentum SGD per bucket inside the backward pass (engine.backward(fused_adam=dict(kind="sgd_momentum", ...)) -> sgd_range)
    changes when the kernels run, not what they compute: after two steps parameters, velocity, bf16 and transposed copies equal
    those of clip_scales() -> sgd_momentum() over the whole buffer -- what
    test_bucketed_optimizer_and_async_targets_are_bitwise_neutral states for Adam."""
    from ssd_object_detection_amd import optimizers

    def run(fused):
        model = make_model(tmp_path)
        model.fused_optimizer = fused
        batch = fixed_batch(model)
        opt = optimizers.SGD(1e-3, momentum=0.9, weight_decay=5e-4)
        for _ in range(2):
            model._train_step(*batch, opt)
        torch.cuda.synchronize()
        assert opt.iterations == 2
        return model.get_engine()

    a, b = run(False), run(True)
    assert a.step_count == b.step_count == 2 and a.slots == b.slots == "sgd_momentum"
    same_state(a, b, ("param", "adam_m", "adam_v", "param_bf16", "clip_scale", "grad_norms"))
    assert float(a.adam_m.abs().max()) > 0 and float(a.adam_v.abs().max()) == 0          # a velocity; Adam's second slot untouched


def test_clip_setting(tmp_path):
    """TrainConfig(clip=...): None runs the clip kernels with clip 0 -- one step equals, bit for bit, the same step with
    clip_scale forced to 1, and grad_norms are still written; 0.01 through the new plumbing is the default step."""
    from ssd_object_detection_amd import ops, optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    TC = SSDObjectDetectionModel.TrainConfig

    def step(cfg, fused=True):
        model = make_model(tmp_path)
        model.fused_optimizer = fused
        model._train_step(*fixed_batch(model), optimizers.Adam(1e-3), cfg=cfg)
        torch.cuda.synchronize()
        return model.get_engine()

    # the restatement: forward, loss, backward, the norms, every scale 1, Adam over the whole buffer
    model = make_model(tmp_path)
    eng = model.get_engine()
    image, cls, loc, mask = fixed_batch(model)
    pred_loc, pred_conf = eng.forward(ops.image_prep(image.contiguous(), normalize=False))
    _, info = model._ssd_loss((cls, loc, mask), (pred_loc, pred_conf), eng.head_grad_buffers(image.shape[0]))
    eng.backward(info["dloc"], info["dconf"], heads=info["heads"])
    eng.clip_scales(0.01)
    assert float(eng.clip_scale.min()) < 1.0                              # (clipping at 0.01 would have changed this step)
    eng.clip_scale.fill_(1.0)
    eng.adam(1e-3, eng.grad, 1.0, True, 0.9, 0.999, 1e-7)
    torch.cuda.synchronize()

    for fused in (True, False):
        off = step(TC(1, 4, None, warmup=False, clip=None), fused)
        same_state(off, eng)
        assert torch.equal(off.grad_norms, eng.grad_norms) and float(off.grad_norms.max()) > 0.01
        assert torch.equal(off.clip_scale, torch.ones_like(off.clip_scale))
    default = step(None)
    assert not torch.equal(default.param, eng.param)
    same_state(step(TC(1, 4, None, warmup=False, clip=0.01)), default, ("param", "adam_m", "adam_v", "param_bf16", "clip_scale"))
    same_state(step(TC(1, 4, None, warmup=False)), default, ("param", "adam_m", "adam_v", "param_bf16", "clip_scale"))


def test_checkpoint_resume_momentum(tmp_path, caplog):
    """Two steps, save, load into a fresh model, one step == the third step of the uninterrupted run, bit for bit; the checkpoint
    names its slots.  A checkpoint saved under Adam and adopted by a momentum SGD starts from zero velocity."""
    from ssd_object_detection_amd import optimizers

    def sgd():
        return optimizers.SGD(optimizers.PiecewiseConstantDecay([1], [1e-3, 5e-4]), momentum=0.9, nesterov=True, weight_decay=5e-4)

    full = make_model(tmp_path)
    batch = fixed_batch(full)
    opt = sgd()
    for _ in range(2):
        full._train_step(*batch, opt)
    ckpt = str(tmp_path / "two_steps.pt")
    full.save(ckpt, extra=dict(iterations=opt.iterations))
    assert full.get_engine().state_dict()["slots"] == "sgd_momentum"
    full._train_step(*batch, opt)

    resumed = make_model(tmp_path, seed=99)
    extra = resumed.load(ckpt)
    assert resumed.get_engine().slots == "sgd_momentum"
    opt2 = sgd()
    opt2.iterations = int(extra["iterations"])
    _, _, info = resumed._train_step(*fixed_batch(resumed), opt2)
    torch.cuda.synchronize()
    assert info["lr"] == 5e-4
    same_state(resumed.get_engine(), full.get_engine())
    assert resumed.get_engine().step_count == full.get_engine().step_count == 3

    # Adam moments are not a velocity
    adam_model = make_model(tmp_path)
    adam_model._train_step(*batch, optimizers.Adam(1e-3))
    sd = adam_model.get_engine().state_dict()
    assert sd["slots"] == "adam" and float(sd["adam_m"].abs().max()) > 0
    ckpt_adam = str(tmp_path / "adam.pt")
    adam_model.save(ckpt_adam)
    old = {k: v for k, v in sd.items() if k != "slots"}                  # a checkpoint from before the key loads as Adam's
    adam_model.get_engine().load_state_dict(old)
    assert adam_model.get_engine().slots == "adam"

    adopted = make_model(tmp_path, seed=99)
    adopted.load(ckpt_adam)
    adopted._train_step(*fixed_batch(adopted), sgd())
    by_hand = make_model(tmp_path, seed=99)
    by_hand.load(ckpt_adam)
    by_hand.get_engine().adam_m.zero_()
    by_hand.get_engine().adam_v.zero_()
    opt3 = sgd()
    by_hand._slot_owner = opt3                                            # the slots are this optimizer's: nothing to adopt
    by_hand._train_step(*fixed_batch(by_hand), opt3)
    torch.cuda.synchronize()
    same_state(adopted.get_engine(), by_hand.get_engine())
    assert adopted.get_engine().slots == "sgd_momentum" and float(adopted.get_engine().adam_v.abs().max()) == 0

    def warnings():
        return [r for r in caplog.records if r.levelname == "WARNING" and "starting from zero slots" in r.getMessage()]

    # ... and a velocity is not Adam's first moment: the other direction, warned about once
    def adam_on(ckpt_path, by_hand_zero):
        m = make_model(tmp_path, seed=99)
        m.load(ckpt_path)
        opt_a = optimizers.Adam(1e-3)
        if by_hand_zero:
            m.get_engine().adam_m.zero_()
            m._slot_owner = opt_a
        for _ in range(2):
            m._train_step(*fixed_batch(m), opt_a)
        torch.cuda.synchronize()
        return m.get_engine()

    caplog.clear()
    with caplog.at_level("WARNING"):
        got = adam_on(ckpt, False)
    assert len(warnings()) == 1 and "sgd_momentum" in warnings()[0].getMessage()          # two steps, one warning
    same_state(got, adam_on(ckpt, True))
    assert got.slots == "adam"
    # all-zero slots are nobody's: a never-trained model's checkpoint (saved as "adam") adopted by a momentum SGD, no warning
    fresh = make_model(tmp_path)
    ckpt_fresh = str(tmp_path / "fresh.pt")
    fresh.save(ckpt_fresh)
    caplog.clear()
    with caplog.at_level("WARNING"):
        m = make_model(tmp_path, seed=99)
        m.load(ckpt_fresh)
        m._train_step(*fixed_batch(m), sgd())
        torch.cuda.synchronize()
    assert not warnings() and m.get_engine().slots == "sgd_momentum"


def test_training_with_paper_recipe_reduces_loss(tmp_path):
    """The SSD paper's recipe on one fixed batch (the synthetic data of test_training_reduces_loss_and_detect_runs): MultiBox loss,
    momentum SGD with weight decay, a piecewise-constant learning rate, no clipping."""
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = make_model(tmp_path)
    batch = fixed_batch(model)
    sched = optimizers.PiecewiseConstantDecay([6], [1e-3, 1e-4])
    opt = optimizers.SGD(sched, momentum=0.9, weight_decay=5e-4)
    cfg = SSDObjectDetectionModel.TrainConfig(1, 4, opt, warmup=False, loss="multibox", clip=None)
    losses, lrs, status = [], [], []
    for _ in range(12):
        _, _, info = model._train_step(*batch, opt, cfg=cfg)
        losses.append(float(info["loc loss"]) + float(info["cls loss pos"]) + float(info["cls loss neg"]))
        lrs.append(info["lr"])
        status.append(float(info["status"]))
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert status == [0.0] * 12
    assert lrs == [sched(k) for k in range(12)] and lrs[6] == 1e-3 and lrs[7] == 1e-4
    assert torch.equal(model.get_engine().clip_scale, torch.ones_like(model.get_engine().clip_scale))


# ---- data parallel -------------------------------------------------------------------------------------------------
def _dp_inputs(model):
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    cls_l, box_l = synth_batch_gt(300, 4)
    return model.make_batch([synth_image(300 + i) for i in range(4)], cls_l, box_l)


def _dp_optimizer():
    from ssd_object_detection_amd import optimizers
    return optimizers.SGD(0.1, momentum=0.9, weight_decay=5e-4)


def _nccl_rank_main(port, q, log_dir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = SSDObjectDetectionModel(classes=80, log_dir=log_dir, seed=5, distributed=True, timestamp_dir=False)
    image, (cls, loc, mask) = _dp_inputs(model)
    opt = _dp_optimizer()
    for _ in range(2):
        model._train_step(image, cls, loc, mask, opt)
    torch.cuda.synchronize()
    q.put((model.get_engine().param.cpu().numpy(), model.get_engine().adam_m.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_single_rank_momentum_equals_the_local_step(tmp_path):
    """test_rccl_backend_single_rank_equals_the_local_step with momentum SGD: a model built with distributed=True under an
    initialised RCCL process group of ONE rank reproduces the non-distributed step, within that test's own bounds on the
    parameter difference.  With world == 1 the step takes the single-device fused path (no GradReducer, no exchange): this
    checks that a process group does not disturb it; the bucketed exchange with the update behind it is
    test_two_ranks_momentum_equal_split_batch."""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_rank_main, args=(port, q, str(tmp_path)))
    p.start()
    dp_param, dp_vel = q.get(timeout=600)
    p.join(timeout=120)
    assert p.exitcode == 0

    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path), seed=5, timestamp_dir=False)
    p0 = model.get_engine().param.cpu().numpy().copy()
    image, (cls, loc, mask) = _dp_inputs(model)
    opt = _dp_optimizer()
    for _ in range(2):
        model._train_step(image, cls, loc, mask, opt)
    ref = model.get_engine().param.cpu().numpy()
    moved = np.abs(ref - p0).max()
    assert moved > 1e-4
    diff = np.abs(dp_param - ref)
    assert float(diff.mean()) < 1e-7 and float((diff > 1e-6).mean()) < 0.02 and diff.max() <= 0.5 * moved
    assert np.abs(dp_vel).max() > 0 and np.abs(dp_vel - model.get_engine().adam_m.cpu().numpy()).max() <= 0.5 * moved


PER_RANK, WORLD = 2, 2


def _gloo_rank_main(rank, world, port, q, log_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = SSDObjectDetectionModel(classes=80, log_dir=log_dir, seed=5, distributed=True, timestamp_dir=False)
    cls_l, box_l = synth_batch_gt(300, PER_RANK * world)
    lo, hi = rank * PER_RANK, (rank + 1) * PER_RANK
    image, (cls, loc, mask) = model.make_batch([synth_image(300 + i) for i in range(lo, hi)], cls_l[lo:hi], box_l[lo:hi])
    model._train_step(image, cls, loc, mask, _dp_optimizer())
    torch.cuda.synchronize()
    eng = model.get_engine()
    if rank == 0:
        q.put((eng.grad.cpu().numpy(), eng.param.cpu().numpy(), eng.adam_m.cpu().numpy(), model._reducer is not None, eng.slots))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_momentum_equal_split_batch(tmp_path):
    """tests/test_dp_gpu.py::test_two_ranks_equal_split_batch with momentum SGD and weight decay: two ranks (gloo, both on the one
    visible GPU) each run their image shard with the bucketed, overlapped exchange -- clip per bucket through the GradReducer's
    clip_fn, all-reduce, then sgd_range(clip=None, grad_scale=1/world) as the bucket's `post` -- and must equal ONE process
    running the whole batch with split_batch (accumulate_clipped -> sgd_momentum).  That test's bounds on the exchanged gradient
    and on the parameters.  The velocity besides: v' = -lr (grad_scale * sum + decay * p) differs between the two only through
    the summed gradient, which that test bounds by 1e-6 of its largest entry, so |dv| <= lr * 1e-6 * max|sum| plus the fp32
    roundings of v itself (4 U max|v|) -- a wrong learning rate, grad_scale or a dropped decay table is orders above that."""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank_main, args=(r, WORLD, port, q, str(tmp_path))) for r in range(WORLD)]
    for p in procs:
        p.start()
    dp_grad, dp_param, dp_vel, had_reducer, slots = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert had_reducer and slots == "sgd_momentum"                 # the overlapped exchange ran, with the momentum update

    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path), seed=5, timestamp_dir=False)
    eng = model.get_engine()
    p0 = eng.param.cpu().numpy().copy()
    image, (cls, loc, mask) = _dp_inputs(model)
    cfg = SSDObjectDetectionModel.TrainConfig(epoch=1, batch_size=PER_RANK * WORLD, optimizer=None, warmup=False,
                                              split_batch=True, split_batch_size=PER_RANK)
    opt = _dp_optimizer()
    model._train_step(image, cls, loc, mask, opt, cfg=cfg)
    ref_grad, ref, ref_vel = eng.grad_acc.cpu().numpy(), eng.param.cpu().numpy(), eng.adam_m.cpu().numpy()
    moved = np.abs(ref - p0).max()
    assert moved > 1e-4                                            # the step did something
    scale = np.abs(ref_grad).max()
    assert scale > 0
    assert np.abs(dp_grad - ref_grad).max() <= 1e-6 * scale
    diff = np.abs(dp_param - ref)
    assert float(diff.mean()) < 1e-7 and float((diff > 1e-6).mean()) < 0.02 and diff.max() <= 0.5 * moved
    vmax = np.abs(ref_vel).max()
    dv = np.abs(dp_vel - ref_vel).max()
    print("moved %.3e, max|dv| %.3e, bound %.3e" % (moved, dv, opt.lr() * 1e-6 * scale + 4 * U * vmax))
    assert vmax > 0 and dv <= opt.lr() * 1e-6 * scale + 4 * U * vmax
    # the decay term is in it: without it the velocity of the filters would be lr * decay * p away
    wd_shift = opt.lr() * opt.weight_decay * np.abs(p0).max()
    assert wd_shift > 100 * (opt.lr() * 1e-6 * scale + 4 * U * vmax)
