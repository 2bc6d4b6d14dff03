"""GPU: the L2 normalisation of feature map 0 inside the SSD300 engine and model (SSDEngine(l2norm=...)): the parameter plan, the
forward composition bit for bit, forward and backward against the torch oracle with the layer (tests/l2norm_oracle.py), the
dense head path against the sparse one, schedule neutrality, the gradient exchange's bookkeeping, train steps, checkpoints,
and the default network left as it was.  Bounds are those of the tests these mirror (tests/test_engine_gpu.py,
tests/test_sgd_momentum_gpu.py)."""
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import l2norm_oracle as LO                                                              # noqa: E402
from tests.test_engine_gpu import gemm_arrays, oracle_params, rel_l2                               # noqa: E402
from tests.test_sgd_momentum_gpu import fixed_batch, make_model, same_state                        # noqa: E402


@pytest.fixture(scope="module")
def engines():
    """(the default engine, the engine with the layer), same seed"""
    from ssd_object_detection_amd.engine import SSDEngine
    return SSDEngine(classes=81, seed=3), SSDEngine(classes=81, seed=3, l2norm=True)


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops
    return ops


def inputs(ops, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = ops.image_prep(torch.rand((B, 300, 300, 3), generator=g).cuda())
    dloc = (torch.randn((B, 8732, 4), generator=g) * 1e-3).bfloat16()
    dconf = (torch.randn((B, 8732, 81), generator=g) * 1e-3).bfloat16()
    return x, dloc, dconf


def test_plan(engines):
    default, eng = engines
    assert len(default.tensors) == 64 and len(eng.tensors) == 65 and default.l2norm is None and default.l2norm_scale is None
    t = eng.tensors[-1]
    assert t is eng.l2norm_scale and t.name == "l2norm0/scale" and t.shape == (512,) and t.index == 64
    assert torch.equal(eng.view(t, eng.param), torch.full((512,), 20.0, device="cuda"))
    key = lambda v: (v.name, v.shape, v.offset, v.block0, v.nblocks)
    assert [key(v) for v in eng.tensors[:64]] == [key(v) for v in default.tensors]
    assert eng.n_params == default.n_params + 512 and eng.n_flat == default.n_flat + t.nblocks * eng.block
    assert torch.equal(eng.param[:default.n_flat], default.param) and torch.equal(eng.param_bf16[:default.n_flat], default.param_bf16)
    # the heads' optimizer bucket ends behind the new tensor; the trunk's buckets are the default engine's
    assert eng.opt_buckets()[0] == (default.opt_buckets()[0][0], 65, None) and eng.opt_buckets()[1:] == default.opt_buckets()[1:]
    # weight decay: the scale counts as a bias
    assert float(eng.decay_table(5e-4)[64]) == 0.0 and float(eng.decay_table(5e-4, decay_bias=True)[64]) == pytest.approx(5e-4)
    assert float(eng.decay_table(5e-4)[eng.head_params[0][0].index]) == pytest.approx(5e-4)
    from ssd_object_detection_amd.engine import SSDEngine, SSD300_TRUNK
    assert float(SSDEngine(classes=81, seed=3, l2norm={"init": 10.0}).param[t.offset]) == 10.0
    with pytest.raises(ValueError):
        SSDEngine(classes=81, l2norm=-1.0)
    with pytest.raises(ValueError):                                       # a first feature map the kernels do not serve
        trunk = list(SSD300_TRUNK)
        trunk[11] = ("conv", 512, 320, 3, 1, "same", False)
        trunk[12] = ("conv", 320, 320, 1, 1, "same", True)
        trunk[13] = ("conv", 320, 1024, 3, 2, "same", False)
        SSDEngine(classes=81, trunk=trunk, l2norm=True)


@pytest.mark.parametrize("precision", ["bf16", "mxfp8"])
def test_forward_composition_bit_for_bit(engines, ops, precision):
    default, eng = engines
    x, _, _ = inputs(ops, 2, 1)
    loc_d, conf_d = (v.clone() for v in default.forward(x, precision))
    loc, conf = eng.forward(x, precision)
    torch.cuda.synchronize()
    n0 = eng.level_off[1]
    assert torch.equal(loc[:, n0:], loc_d[:, n0:]) and torch.equal(conf[:, n0:], conf_d[:, n0:])
    assert not torch.equal(loc[:, :n0], loc_d[:, :n0])
    fmap = eng._acts(2)["acts"][eng.fm[0][0] + 1]                       # this forward's own feature map 0
    assert torch.equal(fmap, default._acts(2)["acts"][eng.fm[0][0] + 1])
    y = ops.l2norm_fwd(fmap, eng.view(eng.l2norm_scale, eng.param))
    wt, bt = eng.head_params[0]
    loc2, conf2 = torch.zeros_like(loc), torch.zeros_like(conf)
    ops.conv2d_head_fwd(y, eng.view(wt, eng.param_bf16), eng.view(bt, eng.param), loc2, conf2, eng.num_priors[0], 81, 0)
    torch.cuda.synchronize()
    assert torch.equal(loc[:, :n0], loc2[:, :n0]) and torch.equal(conf[:, :n0], conf2[:, :n0])
    eng.forward(x)
    default.forward(x)                                                   # (leave both engines behind a bf16 forward)


@pytest.mark.parametrize("scale", ["initial", "perturbed"])
def test_forward_backward_vs_oracle(engines, ops, scale):
    """test_engine_gpu.test_forward_backward_vs_oracle's inputs and bounds with the layer in both networks; the scale's
    gradient under the heads' bound.  "perturbed": another value per channel and one negative -- a gradient that ignores the
    scale or treats it as one number fails."""
    from ssd_object_detection_amd.engine import SSD300_TRUNK, SSD300_NUM_PRIORS
    _, eng = engines
    t = eng.l2norm_scale
    try:
        if scale == "perturbed":
            v = 20.0 + 5.0 * torch.randn(512, generator=torch.Generator().manual_seed(5))
            v[7] = -v[7].abs()
            eng.view(t, eng.param).copy_(v.cuda())
        B = 2
        g = torch.Generator().manual_seed(1)
        x = ops.image_prep(torch.rand((B, 300, 300, 3), generator=g).cuda())
        loc, conf = eng.forward(x)
        params = oracle_params(eng, requires_grad=True)
        s = eng.view(t, eng.param).cpu().clone().requires_grad_(True)
        loc_r, conf_r = LO.forward_torch(SSD300_TRUNK, SSD300_NUM_PRIORS, 81, params, x.float().cpu(), s, eng.l2norm.eps)
        assert rel_l2(loc.float().cpu(), loc_r.detach()) < 1e-2
        assert rel_l2(conf.float().cpu(), conf_r.detach()) < 1e-2
        dloc = (torch.randn((B, 8732, 4), generator=g) * 1e-3).bfloat16()
        dconf = (torch.randn((B, 8732, 81), generator=g) * 1e-3).bfloat16()
        eng.backward(dloc.cuda(), dconf.cuda())
        (loc_r * dloc.float()).sum().add((conf_r * dconf.float()).sum()).backward()
        gflat = eng.grad.cpu()
        for name, shape, off, numel, want in [(a.name, a.shape, a.offset, a.numel, params[a.name].grad) for a in gemm_arrays(eng)] + \
                                             [(t.name, t.shape, t.offset, t.numel, s.grad)]:
            got = gflat[off:off + numel].view(shape)
            err = rel_l2(got, want)
            cos = float((got * want).sum() / (got.norm() * want.norm() + 1e-30))
            print("%-16s rel L2 err %.4f  cos %.5f" % (name, err, cos))
            assert err < (1e-2 if name.startswith(("head", "l2norm")) else 0.15) and cos > 0.985, (name, err, cos)
    finally:
        eng.init_params(seed=3)


def test_dense_head_backward_matches_the_sparse_path(ops):
    """test_engine_gpu.test_dense_head_backward_matches_the_sparse_path with the layer: its inputs, its bounds; the scale's
    gradient under the heads'"""
    from ssd_object_detection_amd.engine import SSDEngine
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    B = 4
    sparse = SSDEngine(classes=81, seed=5, sparse_heads=True, l2norm=True)
    dense = SSDEngine(classes=81, seed=5, sparse_heads=False, l2norm=True)
    assert sparse.sparse_heads and not dense.sparse_heads and torch.equal(sparse.param, dense.param)
    g = torch.Generator().manual_seed(23)
    x = ops.image_prep(torch.rand((B, 300, 300, 3), generator=g).cuda())
    cls_l, box_l = synth_batch_gt(300, B)
    targets = ops.match_encode(*ops.pack_gt(box_l, cls_l), ops.build_priors(), 0.5)
    loc_s, conf_s = sparse.forward(x)
    loc_d, conf_d = dense.forward(x)
    assert torch.equal(loc_s, loc_d) and torch.equal(conf_s, conf_d)
    out, dconf, dloc = ops.ssd_loss(conf_d, loc_d, *targets, grad_scale=64.0)
    hgb = sparse.head_grad_buffers(B)
    ops.ssd_loss_heads(conf_s, loc_s, *targets, hgb, grad_scale=64.0)
    dense.backward(dloc, dconf)
    sparse.backward(None, None, heads=hgb)
    torch.cuda.synchronize()
    gs, gd = sparse.grad.cpu(), dense.grad.cpu()
    for t in gemm_arrays(sparse) + [sparse.l2norm_scale]:
        a, b = gs[t.offset:t.offset + t.numel], gd[t.offset:t.offset + t.numel]
        err = rel_l2(a, b)
        print("%-16s rel L2 %.2e" % (t.name, err))
        assert err < (2e-3 if t.name.startswith(("head", "l2norm")) else 2e-2), (t.name, err)
    t = sparse.l2norm_scale
    assert float(gd[t.offset:t.offset + t.numel].norm()) > 0
    for ni, _, _ in sparse.fm:
        a = sparse._acts(B)["gacts"][ni + 1].float()
        b = dense._acts(B)["gacts"][ni + 1].float()
        assert (a - b).abs().max() <= 2.0 ** -6 * b.abs().max() + 1e-12, ni


@pytest.mark.parametrize("B", [8, 12])
def test_stream_schedule_is_bitwise_neutral(engines, ops, B):
    """test_engine_gpu.test_two_stream_schedule_is_bitwise_neutral with the layer.  B = 8 is that test's batch (l2norm_bwd on the
    main stream behind all heads' data gradient); from B = 12 on the 38x38 level's data gradient and l2norm_bwd behind it run on
    the third stream, in front of the event the trunk's accumulation waits for."""
    _, eng = engines
    x, dloc, dconf = inputs(ops, B, 17)
    dloc, dconf = dloc.cuda(), dconf.cuda()

    def run(overlap):
        eng.overlap_heads = overlap
        eng.grad.zero_()
        loc, conf = eng.forward(x)
        eng.backward(dloc, dconf)
        torch.cuda.synchronize()
        return eng.grad.clone(), loc.clone(), conf.clone()

    saved = eng.overlap_heads
    try:
        ref = run(False)
        t = eng.l2norm_scale
        assert float(ref[0][t.offset:t.offset + t.numel].abs().max()) > 0
        for _ in range(3):
            got = run(True)
            assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
            assert torch.equal(got[0], ref[0])
    finally:
        eng.overlap_heads = saved


@pytest.mark.parametrize("overlap", [True, False], ids=["streams", "one stream"])
@pytest.mark.parametrize("B", [2, 12])
def test_on_ready_reports_every_tensor_once(engines, ops, B, overlap):
    _, eng = engines
    x, dloc, dconf = inputs(ops, B, 3)
    saved = eng.overlap_heads
    try:
        eng.overlap_heads = overlap
        eng.forward(x)
        seen = []
        eng.backward(dloc.cuda(), dconf.cuda(), on_ready=lambda idx: seen.extend(idx))
        torch.cuda.synchronize()
        assert sorted(seen) == list(range(65))
    finally:
        eng.overlap_heads = saved


def sgd_recipe():
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    return optimizers.SGD(1e-3, momentum=0.9, weight_decay=5e-4), SSDObjectDetectionModel.TrainConfig(
        1, 4, None, warmup=False, clip=None, loss="multibox")


def adam_recipe():
    from ssd_object_detection_amd import optimizers
    return optimizers.Adam(1e-3), None


def two_steps(tmp_path, recipe, fused=True):
    model = make_model(tmp_path, l2norm=True)
    model.fused_optimizer = fused
    batch = fixed_batch(model)
    opt, cfg = recipe()
    for _ in range(2):
        model._train_step(*batch, opt, cfg=cfg)
        assert bool(torch.isfinite(model._last_raw).all())
    torch.cuda.synchronize()
    return model


@pytest.mark.parametrize("recipe", [sgd_recipe, adam_recipe], ids=["sgd multibox", "adam"])
def test_train_steps(tmp_path, recipe):
    a = two_steps(tmp_path, recipe).get_engine()
    t = a.l2norm_scale
    s = a.view(t, a.param)
    assert bool(torch.isfinite(a.param).all()) and bool((s != 20.0).any()) and bool(torch.isfinite(s).all())
    assert torch.equal(a.view(t, a.param_bf16), s.bfloat16())
    b = two_steps(tmp_path, recipe).get_engine()
    for name in ("param", "adam_m", "param_bf16"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    c = two_steps(tmp_path, recipe, fused=False).get_engine()
    same_state(a, c, ("param", "adam_m", "adam_v", "param_bf16", "clip_scale", "grad_norms"))


def test_checkpoint(tmp_path):
    a = two_steps(tmp_path, adam_recipe)
    path = os.path.join(str(tmp_path), "l2norm.pt")
    a.save(path)
    b = make_model(tmp_path, seed=9, l2norm=True)
    b.load(path)
    same_state(a.get_engine(), b.get_engine())
    assert a.get_engine().state_dict()["names"][-1] == "l2norm0/scale" and b.get_engine().step_count == 2
    plain = make_model(tmp_path)
    with pytest.raises(ValueError, match="l2norm0/scale"):
        plain.load(path)
    plain_path = os.path.join(str(tmp_path), "plain.pt")
    plain.save(plain_path)
    with pytest.raises(ValueError, match="l2norm0/scale"):
        b.load(plain_path)
    same_state(a.get_engine(), b.get_engine())                           # (the refused load changed nothing)


def test_default_model_never_calls_the_layer(tmp_path, monkeypatch, ops):
    from ssd_object_detection_amd import optimizers
    calls = []
    fwd, bwd = ops.l2norm_fwd, ops.l2norm_bwd
    monkeypatch.setattr(ops, "l2norm_fwd", lambda *a, **k: (calls.append("fwd"), fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "l2norm_bwd", lambda *a, **k: (calls.append("bwd"), bwd(*a, **k))[1])
    model = make_model(tmp_path)
    image, cls, loc, mask = fixed_batch(model)
    for fused in (True, False):
        model.fused_optimizer = fused
        model._train_step(image, cls, loc, mask, optimizers.Adam(1e-3))
    for precision in ("bf16", "mxfp8"):
        model.detect(image, precision=precision)
    torch.cuda.synchronize()
    assert calls == [] and len(model.get_engine().state_dict()["names"]) == 64
    # the same calls with the layer: the wrappers do count, and inference runs through it in both precisions
    model = make_model(tmp_path, l2norm=True)
    model._train_step(image, cls, loc, mask, optimizers.Adam(1e-3))
    assert calls == ["fwd", "bwd"]
    for precision in ("bf16", "mxfp8"):
        score, _, box, _ = model.detect(image, precision=precision)
        assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(box).all())
    assert calls == ["fwd", "bwd", "fwd", "fwd"]
