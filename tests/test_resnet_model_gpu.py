"""GPU: the ResNet-50 SSD512 network behind the model class -- SSDObjectDetectionModel(network=...) at a 256 x 256 input,
batch 2, 80 classes (the smallest configuration with all seven levels, every kernel family of the trunk and the odd bottom
maps 2x2, 1x1, 1x1): construction, one model step against the hand-composed engine sequence bit for bit, tools.train end to
end with validation, checkpoints and resume, inference and both metric modes, the folded fp8 inference of a batchnorm model
and its cache, checkpoints of different networks refusing each other, no per-step host synchronisation, data parallelism
over gloo against split_batch, and the default model left as it was.  No reference counterpart (the reference hard-codes
the 300 x 300 network)."""
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

IN, B, CLASSES = 256, 2, 80
VARIANTS = {
    "default": dict(kind="resnet50_ssd512", in_size=IN),
    "batchnorm": dict(kind="resnet50_ssd512", in_size=IN, batchnorm=dict(momentum=0.1)),
    "mxfp8": dict(kind="resnet50_ssd512", in_size=IN, precision="mxfp8"),
}


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def make_model(log_dir, variant="default", seed=17, **kw):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    network = VARIANTS[variant] if isinstance(variant, str) else variant
    return SSDObjectDetectionModel(classes=CLASSES, log_dir=str(log_dir), seed=seed, timestamp_dir=False, network=network, **kw)


def make_engine(ops, variant, seed=17):
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    return ResNet50SSDEngine(classes=CLASSES + 1, in_size=IN, seed=seed, batchnorm=VARIANTS[variant].get("batchnorm"))


def fixed_batch(ops, first=0, batch=B, seed=21):
    """(prepared bf16 input, packed ground truth) of one fixed synthetic batch."""
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    cls_l, box_l = synth_batch_gt(first, batch)
    x = ops.image_prep(torch.rand((batch, IN, IN, 3), generator=torch.Generator().manual_seed(seed)).cuda(), normalize=True)
    return x, ops.pack_gt(box_l, cls_l)


def state_of(eng):
    names = ["param", "adam_m", "adam_v", "param_bf16"]
    if getattr(eng, "batchnorm", None) is not None:
        names += ["bn_running_mean", "bn_running_var"]
    return {n: getattr(eng, n) for n in names}


def assert_same_state(a, b):
    sa, sb = state_of(a), state_of(b)
    assert set(sa) == set(sb)
    for n in sa:
        assert torch.equal(sa[n], sb[n]), n


def spread_biases(model):
    """conf biases background +2, classes N(0, 1.5): scores cover a range and NMS has work (an untrained net scores 1/81)."""
    eng = model.get_engine()
    g = torch.Generator().manual_seed(0)
    for lvl, (wt, bt) in enumerate(eng.head_params):
        n = eng.num_priors[lvl]
        b = torch.zeros(bt.numel)
        cb = torch.randn((n, CLASSES + 1), generator=g) * 1.5
        cb[:, CLASSES] += 2.0
        b[n * 4:] = cb.reshape(-1)
        eng.param[bt.offset:bt.offset + bt.numel] = b.cuda()


# ---------------------------------------------------------------------------------------------------- 1. construction
@pytest.mark.parametrize("variant", ["default", "batchnorm"])
def test_construction(ops, tmp_path, variant):
    from oracle import ssd_oracle as O
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    model = make_model(tmp_path, variant)
    eng = model.get_engine()
    assert type(eng) is ResNet50SSDEngine and eng.in_size == IN and eng.classes == CLASSES + 1
    assert (eng.batchnorm is not None) == (variant == "batchnorm")
    assert model.cfg.input_shape == (IN, IN, 3) and model.cfg.classes == CLASSES + 1
    assert eng.grids == tuple((h, h) for h in (32, 16, 8, 4, 2, 1, 1))
    s_ref = tuple(v * IN / 512.0 for v in ops.SSD512_S_REF)
    want = O.priors(eng.grids, s_ref, ops.SSD512_RATIOS, IN)
    got = model.get_prior_box()
    assert got.dtype == np.float64 and got.shape == (eng.A, 4) and model._pset.A == eng.A == want.shape[0]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert model.network.as_dict()["kind"] == "resnet50_ssd512" and not eng.bucket_optimizer


# ---------------------------------------------------------------------------------------------------- 2. one step, bit for bit
@pytest.mark.parametrize("variant", ["default", "batchnorm", "mxfp8"])
def test_model_step_equals_the_hand_composed_step(ops, tmp_path, variant):
    """Two Adam steps: model._train_step against match_encode, forward(train=True), ssd_loss_heads, backward,
    clip_scales(0.01), adam on an engine of the same seed."""
    from ssd_object_detection_amd import optimizers
    model = make_model(tmp_path, variant)
    eng = make_engine(ops, variant)
    assert_same_state(model.get_engine(), eng)                           # same seed, same start
    x, gt = fixed_batch(ops)
    precision = VARIANTS[variant].get("precision", "bf16")
    ps = ops.build_priors(grids=eng.grids, s_ref=tuple(v * IN / 512.0 for v in (20, 51, 133, 215, 297, 379, 461, 543)),
                          ratios=((2,), (2, 3), (2, 3), (2, 3), (2, 3), (2,), (2,)), in_size=IN)
    tgt = ops.match_encode(*gt, ps, 0.5)
    opt = optimizers.Adam(1e-3)
    for step in range(2):
        tm = model.match_async(gt)
        for a, b in zip(tm, tgt):
            assert torch.equal(a, b)
        conf_m, loc_m, info = model._train_step(x, *tm, opt)
        ploc, pconf = eng.forward(x, precision, train=True)
        assert torch.equal(ploc, loc_m) and torch.equal(pconf, conf_m)
        hg = eng.head_grad_buffers(B)
        out8 = ops.ssd_loss_heads(pconf, ploc, *tgt, hg)
        reported = []
        eng.backward(None, None, heads=hg, on_ready=reported.append)
        assert reported == eng.ready_order()                              # what the CPU reducer test feeds GradReducer
        eng.clip_scales(0.01)
        eng.adam(1e-3, eng.grad, 1.0, True)
        assert torch.equal(out8[3], model._last_raw[3]) and float(info["status"]) == 0.0
        assert torch.equal(eng.grad, model.get_engine().grad)
        assert_same_state(model.get_engine(), eng)
    assert model.get_engine().step_count == eng.step_count == opt.iterations == 2
    if variant == "mxfp8":                                                # the fp8 path really ran
        assert model.get_engine().last_forward == "mxfp8_train" and model.get_engine().mx_filters_t.allocated


def test_mxfp8_step_with_bf16_data_gradients(ops, tmp_path):
    from ssd_object_detection_amd import optimizers
    model = make_model(tmp_path, dict(VARIANTS["mxfp8"], dgrad_precision="bf16"))
    eng = make_engine(ops, "mxfp8")
    x, gt = fixed_batch(ops)
    tgt = model.match_async(gt)
    model._train_step(x, *tgt, optimizers.Adam(1e-3))
    ploc, pconf = eng.forward(x, "mxfp8", train=True)
    hg = eng.head_grad_buffers(B)
    ops.ssd_loss_heads(pconf, ploc, *tgt, hg)
    eng.backward(None, None, heads=hg, dgrad_precision="bf16")
    eng.clip_scales(0.01)
    eng.adam(1e-3, eng.grad, 1.0, True)
    assert_same_state(model.get_engine(), eng)
    assert not model.get_engine().mx_filters_t.allocated                            # no fp8 data gradient quantised its filters


def test_momentum_sgd_step_without_clipping(ops, tmp_path):
    """Momentum SGD with weight decay and clip=None on the batchnorm network: the clip kernels run with clip 0 (every scale 1),
    gamma / beta and the biases take no L2 term."""
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = make_model(tmp_path, "batchnorm")
    eng = make_engine(ops, "batchnorm")
    x, gt = fixed_batch(ops)
    tgt = model.match_async(gt)
    cfg = SSDObjectDetectionModel.TrainConfig(epoch=1, batch_size=B, optimizer=None, warmup=False, clip=None)
    opt = optimizers.SGD(1e-2, momentum=0.9, weight_decay=5e-4)
    for step in range(2):
        model._train_step(x, *tgt, opt, cfg=cfg)
        ploc, pconf = eng.forward(x, train=True)
        hg = eng.head_grad_buffers(B)
        ops.ssd_loss_heads(pconf, ploc, *tgt, hg)
        eng.backward(None, None, heads=hg)
        eng.clip_scales(0.0)
        eng.sgd_momentum(1e-2, eng.grad, 1.0, True, 0.9, False, eng.decay_table(5e-4, False))
        assert_same_state(model.get_engine(), eng)
    assert bool((model.get_engine().clip_scale == 1.0).all()) and model.get_engine().slots == "sgd_momentum"
    # plain SGD too (no slot, ssd_sgd_step)
    plain = optimizers.SGD(1e-2)
    model._train_step(x, *tgt, plain, cfg=cfg)
    ploc, pconf = eng.forward(x, train=True)
    ops.ssd_loss_heads(pconf, ploc, *tgt, eng.head_grad_buffers(B))
    eng.backward(None, None, heads=eng.head_grad_buffers(B))
    eng.clip_scales(0.0)
    eng.sgd(1e-2, eng.grad, 1.0, True)
    assert torch.equal(model.get_engine().param, eng.param)


def test_split_batch_and_multibox_loss(ops, tmp_path):
    """split_batch micro-batches (a batchnorm engine normalises and updates its running statistics per micro-batch) and the
    SSD paper's loss go through the same step.  The ResNet accumulates as the data-parallel exchange sums: every micro-batch's
    gradient clipped in place (rounded to fp32), then added -- restated here with torch's own addition."""
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = make_model(tmp_path, "batchnorm")
    eng = make_engine(ops, "batchnorm")
    x, gt = fixed_batch(ops, batch=4)
    tgt = model.match_async(gt)
    cfg = SSDObjectDetectionModel.TrainConfig(epoch=1, batch_size=4, optimizer=None, warmup=False, split_batch=True,
                                              split_batch_size=2, loss="multibox")
    model._train_step(x, *tgt, optimizers.Adam(1e-3), cfg=cfg)
    for k, i in enumerate((0, 2)):
        ploc, pconf = eng.forward(x[i:i + 2], train=True)
        hg = eng.head_grad_buffers(2)
        ops.multibox_loss_heads(pconf, ploc, *(t[i:i + 2] for t in tgt), hg, 3, 1.0)
        eng.backward(None, None, heads=hg)
        eng.clip_scales(0.01)
        eng.apply_clip_in_place()
        acc = eng.grad.clone() if k == 0 else acc + eng.grad
    assert torch.equal(acc, model.get_engine().grad_acc)
    eng.adam(1e-3, acc, 0.5, False)
    assert_same_state(model.get_engine(), eng)


# ---------------------------------------------------------------------------------------------------- 3. tools.train end to end
def _train_cfg(tmp_path, sub, variant, epochs, resume=None):
    from ssd_object_detection_amd.tools import train as T
    cfg = T.load_config(os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml"))
    cfg["data"]["mini_batch"]["num_data"] = 8
    cfg["data"]["shuffle"] = False
    cfg["model"]["log_dir"] = str(tmp_path / sub)
    cfg["model"]["train"]["batch_size"] = 2
    cfg["model"]["train"]["epoch"] = epochs
    cfg["model"]["split_train"]["enable"] = False
    cfg["model"]["warmup"]["enable"] = True
    cfg["model"]["warmup"]["step"] = 1
    cfg["model"]["log_interval"] = 100
    cfg["model"]["eval"] = dict(enable=True, every=1, batch_size=2, num_data=4)
    net = dict(VARIANTS[variant])
    if "batchnorm" in net:
        net["batchnorm"] = dict(enable=True, **net["batchnorm"])
    cfg["model"]["network"] = net
    if resume:
        cfg["model"]["resume"] = resume
    return cfg


@pytest.mark.parametrize("variant", ["default", "batchnorm"])
def test_train_cli_end_to_end_and_resume(tmp_path, variant):
    import json
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    from ssd_object_detection_amd.tools import train as T
    from ssd_object_detection_amd.utils.scalar_log import TAGS, read_scalars
    full = T.train(_train_cfg(tmp_path, "full", variant, 2))
    run = full.get_log_dir()
    assert type(full.get_engine()) is ResNet50SSDEngine and full.cfg.input_shape == (IN, IN, 3)
    got = read_scalars(os.path.join(run, "scalars.jsonl"))
    assert set(got) == {s + "/" + t for s in ("warmup", "train") for t in TAGS} | {"val/mAP", "val/AP50", "val/AP75"}
    assert [s for s, _ in got["train/loss"]] == list(range(1, 9)) and len(got["warmup/loss"]) == 1
    losses = [v for _, v in got["train/loss"]]
    print("train/loss:", ["%.4f" % v for v in losses])
    assert len(losses) == 8 and all(np.isfinite(losses))
    for tag in ("val/mAP", "val/AP50", "val/AP75"):
        assert [s for s, _ in got[tag]] == [4, 8] and all(0.0 <= v <= 1.0 for _, v in got[tag])
    with open(os.path.join(run, "config.json")) as f:
        saved = json.load(f)
    assert saved["model"]["network"] == _train_cfg(tmp_path, "full", variant, 2)["model"]["network"]
    for f in ("model_last.pt", os.path.join("model_weight", "model_weight_epoch_0.pt"),
              os.path.join("model_weight", "model_weight_epoch_1.pt")):
        assert os.path.exists(os.path.join(run, f)), f
    sd = torch.load(os.path.join(run, "model_last.pt"), map_location="cpu", weights_only=True)
    assert sd["network"] == full.network.as_dict() and sd["network"]["in_size"] == IN
    # 2 epochs in one go == 1 epoch, checkpoint, resume for the 2nd
    first = T.train(_train_cfg(tmp_path, "first", variant, 1))
    ckpt = os.path.join(first.get_log_dir(), "model_weight", "model_weight_epoch_0.pt")
    resumed = T.train(_train_cfg(tmp_path, "resumed", variant, 2, resume=ckpt))
    assert resumed.get_engine().step_count == full.get_engine().step_count
    assert_same_state(resumed.get_engine(), full.get_engine())
    if variant == "batchnorm":
        assert not torch.equal(full.get_engine().bn_running_mean, torch.zeros_like(full.get_engine().bn_running_mean))


# ---------------------------------------------------------------------------------------------------- 4. inference
def assert_same_result(dev, host, tol=1e-12):
    assert set(dev) == set(host) and set(dev["per_class"]) == set(host["per_class"])
    for k in ("mAP", "AP50", "AP75"):
        assert abs(dev[k] - host[k]) <= tol, (k, dev[k], host[k])
    for c, v in host["per_class"].items():
        assert abs(dev["per_class"][c] - v) <= tol, (c, dev["per_class"][c], v)


def top_cut(dets, max_dets):
    out = []
    for s, c, b in dets:
        order = np.argsort(-np.asarray(s, np.float64), kind="mergesort")[:max_dets]
        out.append((s[order], c[order], b[order]))
    return out


@pytest.mark.parametrize("variant", ["default", "batchnorm"])
def test_inference_and_both_metric_modes(ops, tmp_path, variant):
    from oracle import ssd_oracle as O
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    model = make_model(tmp_path, variant, seed=4)
    spread_biases(model)
    eng = model.get_engine()
    A = eng.A
    _, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=50, input_size=IN).get_dataset()
    samples = list(val)
    assert len(samples) == 5 and samples[0][0].shape == (IN, IN, 3)
    image = (torch.from_numpy(np.stack([s[0] for s in samples[:B]], 0)).cuda() - 0.5) * 2
    score, cls, box, keep = model.detect(image, score_thresh=0.2)
    assert score.shape == (B, A) and cls.shape == (B, A) and box.shape == (B, A, 4) and keep.shape == (B, A)
    assert (score.dtype, cls.dtype, box.dtype, keep.dtype) == (torch.float32, torch.int32, torch.float32, torch.uint8)
    assert bool(torch.isfinite(score).all()) and bool(torch.isfinite(box).all()) and int(keep.sum()) > 20 * B
    # pixels of the 256 input: the oracle's decoding of the same head outputs
    loc, conf = eng.forward(ops.image_prep(image.contiguous(), normalize=False))
    lf = loc.float().cpu().numpy()
    for i in range(B):                                                    # (rows that are no candidates hold a zero box)
        k = keep[i].bool().cpu().numpy()
        np.testing.assert_allclose(box[i].cpu().numpy()[k], O.decode(lf[i], model.get_prior_box(), IN)[k], rtol=3e-7)
    centres = box[..., :2]
    assert float(centres.min()) > -0.25 * IN and float(centres.max()) < 1.25 * IN and float(centres.max()) > 0.5 * IN
    d = model.detections(image, score_thresh=0.2, keep_top_k=50)
    assert d.score.shape == (B, 50) and d.box.shape == (B, 50, 4) and d.n_det.shape == (B,) and d.anchor.shape == (B, 50)
    assert bool(torch.isfinite(d.score).all()) and bool(torch.isfinite(d.box).all())
    assert int(d.n_det.min()) > 0 and int(d.anchor.max()) < A
    # device metric against host metric, with ground truth the detections hit
    host0, hdets = model.evaluate(samples, batch_size=2, score_thresh=0.2, return_detections=True)
    hit = []
    for (img, _, _), (s, c, b) in zip(samples, hdets):
        pick = np.arange(0, len(s), max(1, len(s) // 5))[:5]
        hit.append((img, c[pick].astype(np.float32), (b[pick] / np.float32(IN)).astype(np.float32)))
    for scoring in ("best", "all"):
        host, hdets = model.evaluate(hit, batch_size=2, score_thresh=0.2, return_detections=True, scoring=scoring)
        dev, ddets = model.evaluate(hit, batch_size=2, score_thresh=0.2, return_detections=True, metric="device",
                                    scoring=scoring)
        print(variant, scoring, "host", host["mAP"], host["AP50"], "device", dev["mAP"], dev["AP50"])
        assert host["AP50"] > 0.0
        assert_same_result(dev, host)
        for (s, c, b), (ws, wc, wb) in zip(ddets, top_cut(hdets, 100)):
            assert np.array_equal(s, ws) and np.array_equal(c, wc) and np.array_equal(b, wb)
    with pytest.raises(ValueError):
        model.detect(image, precision="fp8")


def test_mxfp8_inference_of_a_plain_resnet_model(ops, tmp_path):
    model = make_model(tmp_path, "default", seed=4)
    spread_biases(model)
    x, _ = fixed_batch(ops)
    got = model._detect_prepared(x, 0.2, 0.45, precision="mxfp8")
    loc, conf = model.get_engine().forward(x, "mxfp8")
    score, cls, box, cand = ops.score_decode(conf, loc, model._pset, 0.2, float(IN))
    want = (score, cls, box, ops.nms(score, cls, box, cand, 0.45, 400))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert model.folds_built == 0 and model.get_engine().last_forward.startswith("mxfp8")


# ---------------------------------------------------------------------------------------------------- 5. folded fp8 inference
def test_folded_fp8_inference_follows_the_training_state(ops, tmp_path):
    from ssd_object_detection_amd import optimizers
    model = make_model(tmp_path, "batchnorm", seed=4)
    spread_biases(model)
    x, gt = fixed_batch(ops)
    image = (torch.rand((B, IN, IN, 3), generator=torch.Generator().manual_seed(3)).cuda() - 0.5) * 2
    xi = ops.image_prep(image.contiguous(), normalize=False)

    def by_hand():
        loc, conf = model.get_engine().folded().forward(xi, "mxfp8")
        score, cls, box, cand = ops.score_decode(conf, loc, model._pset, 0.2, float(IN))
        return [t.clone() for t in (score, cls, box, ops.nms(score, cls, box, cand, 0.45, 400))]

    opt = optimizers.Adam(1e-3)
    tgt = model.match_async(gt)
    model._train_step(x, *tgt, opt)                                       # running statistics away from (0, 1)
    assert model.folds_built == 0
    first = [t.clone() for t in model.detect(image, score_thresh=0.2, precision="mxfp8")]
    assert model.folds_built == 1
    for a, b in zip(first, by_hand()):
        assert torch.equal(a, b)
    again = model.detect(image, score_thresh=0.2, precision="mxfp8")
    model.detections(image, score_thresh=0.2, precision="mxfp8")
    assert model.folds_built == 1                                         # no step in between: the cached engine
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    model.detect(image, score_thresh=0.2)                                 # a bf16 pass neither uses nor invalidates it
    assert model.folds_built == 1
    model._train_step(x, *tgt, opt)
    second = [t.clone() for t in model.detect(image, score_thresh=0.2, precision="mxfp8")]
    assert model.folds_built == 2
    assert not torch.equal(second[0], first[0])
    for a, b in zip(second, by_hand()):
        assert torch.equal(a, b)
    path = str(tmp_path / "m.pt")
    model.save(path)
    model.load(path)
    model.detect(image, score_thresh=0.2, precision="mxfp8")
    assert model.folds_built == 3                                         # load() counts as a change
    r = model.evaluate([(np.zeros((IN, IN, 3), np.float32), np.zeros((0,), np.float32), np.zeros((0, 4), np.float32))] * 3,
                       batch_size=2, metric="device", precision="mxfp8")
    assert model.folds_built == 3 and set(r) == {"mAP", "AP50", "AP75", "per_class"}


# ---------------------------------------------------------------------------------------------------- 6. checkpoints
def test_checkpoints_of_different_networks_refuse_each_other(tmp_path):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    specs = {
        "ssd300": None,
        "resnet256": VARIANTS["default"],
        "resnet256bn": VARIANTS["batchnorm"],
        "resnet512": dict(kind="resnet50_ssd512", in_size=512),
    }
    models, paths = {}, {}
    for k, (name, net) in enumerate(specs.items()):
        models[name] = SSDObjectDetectionModel(classes=CLASSES, log_dir=str(tmp_path), seed=30 + k, timestamp_dir=False,
                                               network=net)
        paths[name] = str(tmp_path / (name + ".pt"))
        models[name].save(paths[name])
    for target, model in models.items():
        before = {n: t.clone() for n, t in state_of(model.get_engine()).items()}
        for source in models:
            if source == target:
                continue
            with pytest.raises(ValueError) as e:
                model.load(paths[source])
            msg = str(e.value)
            assert models[source].network.describe() in msg and model.network.describe() in msg, msg
        for n, t in before.items():
            assert torch.equal(getattr(model.get_engine(), n), t), (target, n)
    # a checkpoint without the key is an ssd300 one
    sd = torch.load(paths["ssd300"], map_location="cpu", weights_only=True)
    assert sd.pop("network")["kind"] == "ssd300"
    old = str(tmp_path / "old.pt")
    torch.save(sd, old)
    fresh = SSDObjectDetectionModel(classes=CLASSES, log_dir=str(tmp_path), seed=99, timestamp_dir=False)
    fresh.load(old)
    assert torch.equal(fresh.get_engine().param, models["ssd300"].get_engine().param)
    with pytest.raises(ValueError, match="ssd300"):
        models["resnet256"].load(old)
    # its own network loads, whatever precision it is trained in, running statistics included
    twin = make_model(tmp_path, dict(VARIANTS["batchnorm"], batchnorm=dict(momentum=0.5)), seed=77)
    models["resnet256bn"].get_engine().bn_running_mean.fill_(0.25)
    models["resnet256bn"].save(paths["resnet256bn"])
    twin.load(paths["resnet256bn"])
    assert_same_state(twin.get_engine(), models["resnet256bn"].get_engine())
    fp8 = make_model(tmp_path, "mxfp8", seed=78)
    fp8.load(paths["resnet256"])
    assert torch.equal(fp8.get_engine().param, models["resnet256"].get_engine().param)


# ---------------------------------------------------------------------------------------------------- 7. no per-step sync
def test_batchnorm_steps_and_scalar_log_never_synchronise(ops, tmp_path):
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.utils.scalar_log import ScalarLog
    model = make_model(tmp_path, "batchnorm")
    opt = optimizers.Adam(optimizers.ExponentialDecay(1e-3, 100, 0.9))
    batches = [fixed_batch(ops, first=4 * k, seed=50 + k) for k in range(2)]
    outs = [None, None]
    model._scalars = ScalarLog(model.get_log_dir(), model.device, capacity=64)
    outs[0] = model.match_async(batches[0][1])
    model._train_step(batches[0][0], *outs[0], opt)                       # first step builds caches (allocations sync)
    outs[1] = model.match_async(batches[1][1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                               # any torch-side host sync now raises
    try:
        for step in range(1, 5):
            x, gt = batches[step % 2]
            outs[step % 2] = model.match_async(gt, out=outs[step % 2])
            _, _, info = model._train_step(x, *outs[step % 2], opt)
            model._log(step, info, None, "train")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    rows = model._scalars.flush()
    model._scalars.close()
    assert [r[1] for r in rows] == [1, 2, 3, 4] and all(np.isfinite(r[2][:4]).all() for r in rows)
    assert model.get_engine().step_count == 5


# ---------------------------------------------------------------------------------------------------- 8. data parallel
PER_RANK, WORLD = 2, 2


def _dp_batch(ops):
    return fixed_batch(ops, first=300, batch=PER_RANK * WORLD, seed=9)


def _dp_rank_main(rank, world, port, out_dir, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import ssd_object_detection_amd.ops as ops
    from ssd_object_detection_amd import optimizers
    model = make_model(os.path.join(out_dir, "rank%d" % rank), "default", seed=5, distributed=True)
    model._assert_replicas_identical()
    x, gt = _dp_batch(ops)
    cls, loc, mask = ops.match_encode(*gt, model._pset, 0.5)
    lo, hi = rank * PER_RANK, (rank + 1) * PER_RANK
    opt = optimizers.Adam(1e-3)
    eng = model.get_engine()
    for step in range(2):
        model._train_step(x[lo:hi].contiguous(), cls[lo:hi], loc[lo:hi], mask[lo:hi], opt)
        torch.cuda.synchronize()
        if rank == 0 and step == 0:
            np.save(os.path.join(out_dir, "grad1.npy"), eng.grad.cpu().numpy())
            np.save(os.path.join(out_dir, "m1.npy"), eng.adam_m.cpu().numpy())
            np.save(os.path.join(out_dir, "param1.npy"), eng.param.cpu().numpy())
    if rank == 0:
        np.save(os.path.join(out_dir, "grad2.npy"), eng.grad.cpu().numpy())
        for name in ("param", "adam_m", "adam_v"):
            np.save(os.path.join(out_dir, name + "2.npy"), getattr(eng, name).cpu().numpy())
    q.put((rank, eng.step_count, list(model._reducer.buckets)))
    dist.barrier()
    dist.destroy_process_group()


def _three_part(diff, scale):
    """The figures of tests/test_dp_gpu.py's comparison for two Adam steps (mean < 2e-7, fraction above 2e-6 under 3 %,
    maximum one flipped step) in units of the quantity's own scale: there `moved` = 2e-3 is the scale, so the three bounds
    are 1e-4, 1e-3 and 1."""
    return dict(mean=float(diff.mean()) / scale, frac=float((diff > 1e-3 * scale).mean()), top=float(diff.max()) / scale,
                scale=float(scale))


def _within_three_part(f, what):
    print("%s: mean %.3e  fraction %.3e  max %.3e  (of scale %.3e)" % (what, f["mean"], f["frac"], f["top"], f["scale"]))
    return f["mean"] < 1e-4 and f["frac"] < 0.03 and f["top"] <= 1.0


@pytest.fixture(scope="module")
def dp_run(ops, tmp_path_factory):
    """Two ranks over gloo on the one GPU (fresh child processes, started before this process runs the reference; each under
    its own time limit), each its image shard as one micro-batch with the bucketed exchange, and ONE process running the whole
    batch with split_batch at the rank's batch: two Adam steps each.  Returns the figures the tests below assert on (the flat
    buffers themselves, 96 MB each, are compared here and dropped)."""
    import torch.multiprocessing as mp
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    tmp_path = tmp_path_factory.mktemp("dp")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    out_dir = str(tmp_path)
    procs = [ctx.Process(target=_dp_rank_main, args=(r, WORLD, port, out_dir, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        res = dict((r[0], r[1:]) for r in (q.get(timeout=300) for _ in range(WORLD)))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:                                                   # none outlives its limit
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert res[0][0] == res[1][0] == 2 and res[0][1] == res[1][1] and len(res[0][1]) > 1

    model = make_model(tmp_path / "single", "default", seed=5)
    eng = model.get_engine()
    p0 = eng.param.cpu().numpy().copy()
    x, gt = _dp_batch(ops)
    tgt = ops.match_encode(*gt, model._pset, 0.5)
    cfg = SSDObjectDetectionModel.TrainConfig(epoch=1, batch_size=PER_RANK * WORLD, optimizer=None, warmup=False,
                                              split_batch=True, split_batch_size=PER_RANK)
    opt = optimizers.Adam(1e-3)

    def load(name):
        path = os.path.join(out_dir, name + ".npy")
        a = np.load(path)
        os.remove(path)
        return a

    f = {}
    model._train_step(x, *tgt, opt, cfg=cfg)
    for name, ref in (("grad1", eng.grad_acc), ("m1", eng.adam_m)):
        ref = ref.cpu().numpy()
        f[name] = dict(err=float(np.abs(load(name) - ref).max()), scale=float(np.abs(ref).max()))
    ref = eng.param.cpu().numpy()
    diff = np.abs(load("param1") - ref)
    f["param1"] = dict(differ=int((diff > 0).sum()), size=diff.size, mean=float(diff.mean()), above=float((diff > 1e-6).mean()),
                       top=float(diff.max()), moved=float(np.abs(ref - p0).max()))
    model._train_step(x, *tgt, opt, cfg=cfg)
    g2, r2 = load("grad2"), eng.grad_acc.cpu().numpy()
    f["grad2"] = dict(rel_l2=float(np.linalg.norm(g2 - r2) / np.linalg.norm(r2)), err=float(np.abs(g2 - r2).max()),
                      scale=float(np.abs(r2).max()))
    ref = eng.param.cpu().numpy()
    f["param2"] = _three_part(np.abs(load("param2") - ref), np.abs(ref - p0).max())
    for name in ("adam_m", "adam_v"):
        ref = getattr(eng, name).cpu().numpy()
        f[name + "2"] = _three_part(np.abs(load(name + "2") - ref), np.abs(ref).max())
    return f


def test_two_ranks_equal_split_batch_after_one_step(dp_run):
    """The exchanged quantity -- the sum over ranks of the per-rank clipped gradients against the sum over micro-batches --
    under tests/test_dp_gpu.py's bound, 1e-6 of the largest element; Adam's first moment m1 = (1 - beta1) * sum / world is
    linear in it, plus its own fp32 rounding; the parameters after the step under that file's one-step comparison.
    Those are the bounds.  What ResNet50SSDEngine.accumulate_clipped is there for is more: both sides round the clipped
    gradient to fp32 and then add, so for two ranks they hold the same bits -- asserted as well."""
    for name, bound in (("grad1", 1e-6), ("m1", 1e-6 + 2.0 ** -23)):
        f = dp_run[name]
        print("%s: max |diff| %.3e of scale %.3e" % (name, f["err"], f["scale"]))
        assert f["scale"] > 0 and f["err"] <= bound * f["scale"], name
    f = dp_run["param1"]
    print("param after step 1: %d of %d elements differ, mean %.3e, above 1e-6 %.3e, max %.3e (moved %.3e)" % (
        f["differ"], f["size"], f["mean"], f["above"], f["top"], f["moved"]))
    assert f["moved"] > 1e-4 and f["mean"] < 1e-7 and f["above"] < 0.02 and f["top"] <= 0.5 * f["moved"]
    assert dp_run["grad1"]["err"] == 0.0 and dp_run["m1"]["err"] == 0.0 and f["differ"] == 0


def test_two_ranks_moments_after_two_steps(dp_run):
    """Both Adam moments after two steps, under tests/test_dp_gpu.py's two-step comparison in units of their own scale."""
    assert dp_run["adam_m2"]["scale"] > 0 and dp_run["adam_v2"]["scale"] > 0
    assert _within_three_part(dp_run["adam_m2"], "adam_m") and _within_three_part(dp_run["adam_v2"], "adam_v")


def test_two_ranks_parameters_after_two_steps(dp_run):
    """The parameters after two steps, under tests/test_dp_gpu.py's two-step comparison for SSD300 (mean |diff| < 2e-7,
    under 3 % of the elements above 2e-6, maximum one flipped step = the largest move).

    This network does not absorb last-bit differences of the first step the way SSD300 does.  With SSDEngine's accumulation
    (fma(g, scale, acc): one rounding where the exchange has two) this comparison failed on one MI355X, 2026-10-20: after
    step 1 64 280 of 23 917 568 parameters differed, by at most 1.5e-8; the second pass (50 bf16 layers, hard-negative mining)
    put the exchanged gradients 1.25e-2 apart in relative l2, and the parameters came out at mean |diff| 4.6e-4 of `moved`
    (bound 1e-4) with 8.5 % above 1e-3 of it (bound 3 %).  ResNet50SSDEngine.accumulate_clipped rounds as the exchange does."""
    f = dp_run["grad2"]                                                   # (a figure, not a check)
    print("exchanged gradient of step 2: |diff| / |ref| in l2 %.3e, max |diff| %.3e of scale %.3e" % (
        f["rel_l2"], f["err"], f["scale"]))
    assert dp_run["param2"]["scale"] > 1e-4                               # the steps did something
    assert _within_three_part(dp_run["param2"], "param")


# ---------------------------------------------------------------------------------------------------- 9. the default model
def test_the_default_model_is_untouched(ops, tmp_path):
    from oracle import ssd_oracle as O
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    from ssd_object_detection_amd.engine import SSDEngine
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    plain = SSDObjectDetectionModel(CLASSES, str(tmp_path), timestamp_dir=False)
    named = SSDObjectDetectionModel(CLASSES, str(tmp_path), timestamp_dir=False, network="ssd300")
    cls_l, box_l = synth_batch_gt(0, B)
    imgs = [synth_image(i) for i in range(B)]
    calls = []
    for m in (plain, named):
        eng = m.get_engine()
        assert type(eng) is SSDEngine and eng.bucket_optimizer and m.fused_optimizer
        assert m.cfg.input_shape == (300, 300, 3) and eng.A == 8732 and m.network.kind == "ssd300"
        assert np.array_equal(m.get_prior_box().view(np.uint64), O.priors().view(np.uint64))
        real = eng.backward

        def spy(*a, _real=real, **k):
            calls.append(sorted(k))
            return _real(*a, **k)

        eng.backward = spy
        image, (cls, loc, mask) = m.make_batch(imgs, cls_l, box_l)
        assert image.shape == (B, 300, 300, 3)
        m._train_step(image, cls, loc, mask, optimizers.Adam(1e-3))
    assert calls == [["fused_adam", "heads"], ["fused_adam", "heads"]]    # Adam per bucket inside backward, nothing new passed
    a, b = plain.get_engine(), named.get_engine()
    for n in ("param", "adam_m", "adam_v", "param_bf16", "grad"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert a.step_count == b.step_count == 1
