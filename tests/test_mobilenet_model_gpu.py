"""GPU: the MobileNet-v1 SSD300 network behind the model class -- SSDObjectDetectionModel(network="mobilenet_v1_ssd300") at batch
2 with 20 classes (+ background): one model step against the hand-composed engine sequence bit for bit (Adam with the
reference's loss; momentum SGD with the MultiBox loss), a few steps on one batch, checkpoints and their refusal across the other
three networks, inference shapes with 2268 anchors, and a one-rank distributed step against the local one (the mechanics of
tests/test_dp_gpu.py)."""
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B, CLASSES, NET = 2, 20, "mobilenet_v1_ssd300"


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def make_model(log_dir, seed=17, **kw):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    kw.setdefault("network", NET)
    return SSDObjectDetectionModel(classes=CLASSES, log_dir=str(log_dir), seed=seed, timestamp_dir=False, **kw)


def make_engine(seed=17):
    from ssd_object_detection_amd.engine import SSDEngine, MOBILENET_V1_SSD300_TRUNK, MOBILENET_V1_SSD300_NUM_PRIORS
    return SSDEngine(classes=CLASSES + 1, seed=seed, trunk=MOBILENET_V1_SSD300_TRUNK, num_priors=MOBILENET_V1_SSD300_NUM_PRIORS)


def fixed_batch(ops, first=0, batch=B, seed=21):
    """(prepared bf16 input, packed ground truth) of one fixed synthetic batch, classes folded into 0 .. 19"""
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    cls_l, box_l = synth_batch_gt(first, batch)
    cls_l = [np.mod(c, CLASSES).astype(np.float32) for c in cls_l]
    x = ops.image_prep(torch.rand((batch, 300, 300, 3), generator=torch.Generator().manual_seed(seed)).cuda(), normalize=True)
    return x, ops.pack_gt(box_l, cls_l)


def assert_same_state(a, b, names=("param", "adam_m", "adam_v", "param_bf16")):
    for n in names:
        assert torch.equal(getattr(a, n), getattr(b, n)), n


def test_construction(ops, tmp_path):
    from ssd_object_detection_amd.engine import SSDEngine, MOBILENET_V1_SSD300_TRUNK
    m = make_model(tmp_path)
    eng = m.get_engine()
    assert type(eng) is SSDEngine and eng.trunk == list(MOBILENET_V1_SSD300_TRUNK) and eng.A == 2268 and eng.classes == CLASSES + 1
    assert eng.bucket_optimizer and m.fused_optimizer and m.high_priority_main and m.cfg.input_shape == (300, 300, 3)
    assert m.network.as_dict()["kind"] == NET and eng.l2norm is None and eng.bf16_only and len(eng.tensors) == 94
    # the default boxes: six levels on grids 19 .. 1 with the scales 60 .. 330, built by the library as for every network
    pri = m.get_prior_box()
    want = ops.build_priors(grids=eng.grids, s_ref=ops.MOBILENET_SSD300_S_REF).priors.cpu().numpy()
    assert pri.shape == (2268, 4) and np.array_equal(pri.view(np.uint64), want.view(np.uint64))
    w0, w1 = np.unique(pri[:4, 2]), np.unique(pri[1444:1450, 2])          # the box widths of a cell of levels 0 and 1
    assert np.isclose(w1[:, None] / w0[None, :], 105.0 / 60.0).any() and not np.array_equal(
        pri[:4].view(np.uint64), ops.build_priors(grids=eng.grids).priors.cpu().numpy()[:4].view(np.uint64))
    with pytest.raises(ValueError, match="l2norm"):
        make_model(tmp_path, l2norm=True)
    with pytest.raises(ValueError, match="fp8_inference"):
        make_model(tmp_path, fp8_inference=True)


@pytest.mark.parametrize("recipe", ["adam-reference", "sgd-multibox"])
def test_model_step_equals_the_hand_composed_step(ops, tmp_path, recipe):
    """Two steps: model._train_step (optimizer per bucket inside backward(), on the high-priority stream) against forward,
    loss, backward, clip_scales(0.01) and ONE optimizer launch over the flat buffer on an engine of the same seed."""
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    paper = recipe != "adam-reference"
    model, eng = make_model(tmp_path), make_engine()
    assert_same_state(model.get_engine(), eng)
    x, gt = fixed_batch(ops)
    tgt = ops.match_encode(*gt, model._pset, 0.5)
    cfg = SSDObjectDetectionModel.TrainConfig(epoch=1, batch_size=B, optimizer=None, warmup=False, loss="multibox" if paper else None)
    opt = optimizers.SGD(1e-3, momentum=0.9, weight_decay=5e-4) if paper else optimizers.Adam(1e-3)
    calls = []
    real = model.get_engine().backward
    model.get_engine().backward = lambda *a, **k: (calls.append(sorted(k)), real(*a, **k))[1]
    for step in range(2):
        tm = model.match_async(gt)
        for a, b in zip(tm, tgt):
            assert torch.equal(a, b)
        conf_m, loc_m, info = model._train_step(x, *tm, opt, cfg=cfg)
        ploc, pconf = eng.forward(x)
        assert torch.equal(ploc, loc_m) and torch.equal(pconf, conf_m)
        hg = eng.head_grad_buffers(B)
        out8 = ops.multibox_loss_heads(pconf, ploc, *tgt, hg, 3, 1.0) if paper else ops.ssd_loss_heads(pconf, ploc, *tgt, hg)
        eng.backward(None, None, heads=hg)
        eng.clip_scales(0.01)
        if paper:
            eng.sgd_momentum(1e-3, eng.grad, 1.0, True, 0.9, False, eng.decay_table(5e-4, False))
        else:
            eng.adam(1e-3, eng.grad, 1.0, True)
        torch.cuda.synchronize()
        assert torch.equal(out8[3], model._last_raw[3]) and float(info["status"]) == 0.0
        assert torch.equal(eng.grad, model.get_engine().grad)
        assert_same_state(model.get_engine(), eng)
    assert calls == [["fused_adam", "heads"]] * 2                          # the ssd300 branch of the step
    assert model.get_engine().step_count == eng.step_count == opt.iterations == 2
    assert model.get_engine().slots == ("sgd_momentum" if paper else "adam")
    wt = model.get_engine().conv_params[1][0]                             # the depthwise filters are trained like every other variable
    assert wt.name == "dwconv1/kernel"
    assert not torch.equal(model.get_engine().view(wt, model.get_engine().param), make_engine().view(wt, make_engine().param))


def test_four_steps_on_one_batch_lower_the_loss(ops, tmp_path):
    """The SSD paper's recipe, as tests/test_sgd_momentum_gpu.py runs it on SSD300: MultiBox loss, momentum SGD at 1e-3 with weight
    decay, no clipping."""
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = make_model(tmp_path)
    x, gt = fixed_batch(ops)
    tgt = model.match_async(gt)
    cfg = SSDObjectDetectionModel.TrainConfig(epoch=1, batch_size=B, optimizer=None, warmup=False, loss="multibox", clip=None)
    opt = optimizers.SGD(1e-3, momentum=0.9, weight_decay=5e-4)
    rows = []
    for _ in range(4):
        _, _, info = model._train_step(x, *tgt, opt, cfg=cfg)
        rows.append(model._last_raw.cpu().numpy().copy())
        assert float(info["status"]) == 0.0
    rows = np.stack(rows)
    print("total loss per step:", rows[:, 3])
    assert np.isfinite(rows).all() and rows[-1, 3] < rows[0, 3]
    assert bool(torch.isfinite(model.get_engine().param).all())


def test_checkpoints_round_trip_and_refuse_other_networks(ops, tmp_path):
    from ssd_object_detection_amd import optimizers
    model = make_model(tmp_path, seed=31)
    x, gt = fixed_batch(ops)
    model._train_step(x, *model.match_async(gt), optimizers.Adam(1e-3))
    path = str(tmp_path / "mobilenet.pt")
    model.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sd["network"] == model.network.as_dict() and sd["network"]["kind"] == NET
    twin = make_model(tmp_path, seed=77)
    assert not torch.equal(twin.get_engine().param, model.get_engine().param)
    twin.load(path)
    assert_same_state(twin.get_engine(), model.get_engine())
    assert twin.get_engine().step_count == model.get_engine().step_count == 1
    loc_a, conf_a = (t.clone() for t in model.get_engine().forward(x))
    loc_b, conf_b = twin.get_engine().forward(x)
    assert torch.equal(loc_a, loc_b) and torch.equal(conf_a, conf_b)
    others = {"ssd300": make_model(tmp_path, seed=32, network=None),
              "vgg16_ssd300": make_model(tmp_path, seed=34, network="vgg16_ssd300"),
              "resnet50_ssd512": make_model(tmp_path, seed=33, network=dict(kind="resnet50_ssd512", in_size=256))}
    for name, other in others.items():
        before = other.get_engine().param.clone()
        with pytest.raises(ValueError) as e:
            other.load(path)
        assert NET in str(e.value) and name in str(e.value), str(e.value)
        assert torch.equal(other.get_engine().param, before)
        theirs = str(tmp_path / (name + ".pt"))
        other.save(theirs)
        before = model.get_engine().param.clone()
        with pytest.raises(ValueError) as e:
            model.load(theirs)
        assert NET in str(e.value) and name in str(e.value), str(e.value)
        assert torch.equal(model.get_engine().param, before)


def test_inference_shapes(ops, tmp_path):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    model = make_model(tmp_path, seed=4)
    eng = model.get_engine()
    g = torch.Generator().manual_seed(0)                                  # conf biases spread: scores cover a range, NMS has work
    for lvl, (wt, bt) in enumerate(eng.head_params):
        n = eng.num_priors[lvl]
        b = torch.zeros(bt.numel)
        cb = torch.randn((n, CLASSES + 1), generator=g) * 1.5
        cb[:, CLASSES] += 2.0
        b[n * 4:] = cb.reshape(-1)
        eng.param[bt.offset:bt.offset + bt.numel] = b.cuda()
    A = eng.A
    image = (torch.rand((B, 300, 300, 3), generator=g).cuda() - 0.5) * 2
    score, cls, box, keep = model.detect(image, score_thresh=0.2)
    assert score.shape == (B, A) and cls.shape == (B, A) and box.shape == (B, A, 4) and keep.shape == (B, A)
    assert (score.dtype, cls.dtype, box.dtype, keep.dtype) == (torch.float32, torch.int32, torch.float32, torch.uint8)
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(box).all()) and int(keep.sum()) > 0
    assert int(cls.max()) < CLASSES
    d = model.detections(image, score_thresh=0.2, keep_top_k=50)
    assert d.score.shape == (B, 50) and d.box.shape == (B, 50, 4) and d.n_det.shape == (B,) and d.anchor.shape == (B, 50)
    assert int(d.n_det.min()) > 0 and int(d.anchor.max()) < A and bool(torch.isfinite(d.score).all())
    assert A == 2268
    with pytest.raises(NotImplementedError, match="depthwise"):
        model.detect(image, precision="mxfp8")
    _, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=50).get_dataset()
    samples = [(img, np.mod(c, CLASSES).astype(np.float32), b) for img, c, b in list(val)[:3]]
    r = model.evaluate(samples, batch_size=2, score_thresh=0.2, metric="device")
    assert set(r) == {"mAP", "AP50", "AP75", "per_class"} and all(0.0 <= r[k] <= 1.0 for k in ("mAP", "AP50", "AP75"))


# ---------------------------------------------------------------------------------------------------- data parallel, one rank
def _nccl_rank_main(port, log_dir, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    import ssd_object_detection_amd.ops as ops
    from ssd_object_detection_amd import optimizers
    try:
        model = make_model(log_dir, seed=5, distributed=True)
        model._assert_replicas_identical()
        x, gt = fixed_batch(ops, first=300, seed=9)
        tgt = ops.match_encode(*gt, model._pset, 0.5)
        opt = optimizers.Adam(1e-3)
        for _ in range(2):
            model._train_step(x, *tgt, opt)
        torch.cuda.synchronize()
        q.put(("ok", model.get_engine().param.cpu().numpy()))
    except BaseException as e:                                            # the parent must not wait for its time limit
        q.put(("error", repr(e)))
        raise
    dist.barrier()
    dist.destroy_process_group()


def test_one_rank_distributed_step_equals_the_local_step(ops, tmp_path):
    """tests/test_dp_gpu.py's RCCL case for this network: a model built with distributed=True under an initialised one-rank
    `nccl` process group (a fresh child process) takes two Adam steps and must reproduce the local model's: that file's
    comparison."""
    import torch.multiprocessing as mp
    from ssd_object_detection_amd import optimizers
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_rank_main, args=(port, str(tmp_path / "rank0"), q))
    p.start()
    try:
        status, dp_param = q.get(timeout=240)
        assert status == "ok", dp_param
        p.join(timeout=60)
        assert p.exitcode == 0
    finally:
        if p.is_alive():
            p.kill()
            p.join(timeout=10)
    model = make_model(tmp_path / "local", seed=5)
    p0 = model.get_engine().param.cpu().numpy().copy()
    x, gt = fixed_batch(ops, first=300, seed=9)
    tgt = ops.match_encode(*gt, model._pset, 0.5)
    opt = optimizers.Adam(1e-3)
    for _ in range(2):
        model._train_step(x, *tgt, opt)
    ref = model.get_engine().param.cpu().numpy()
    moved = np.abs(ref - p0).max()
    diff = np.abs(dp_param - ref)
    print("moved %.3e  mean |diff| %.3e  above 1e-6 %.3e  max %.3e" % (moved, diff.mean(), (diff > 1e-6).mean(), diff.max()))
    assert moved > 1e-4
    assert float(diff.mean()) < 1e-7 and float((diff > 1e-6).mean()) < 0.02 and diff.max() <= 0.5 * moved
