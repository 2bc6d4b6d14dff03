"""GPU: the IoU box terms through the model and the engines -- model._train_step with LossSpec("multibox", box="giou") and
LossSpec("softmax_focal", box="ciou") against the hand-composed engine sequence bit for bit at batch 2, on the default network and
on network="vgg16_ssd300" (the model hands its own priors to the loss); the steps of the default loss and of the smooth-L1
MultiBox loss against the calls they made before; and a tools/train.py run from a config with `box: diou`."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import test_vgg16_model_gpu as V                            # noqa: E402
from tests.test_multibox_train_gpu import fixed_batch                  # noqa: E402

STATE = ("param", "adam_m", "adam_v", "param_bf16")


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def setup(ops, network, tmp_path):
    """(model, engine of the same seed, prepared input, targets, what _train_step takes as its image)"""
    if network == "ssd300":
        from ssd_object_detection_amd.engine import SSDEngine
        from ssd_object_detection_amd.models import SSDObjectDetectionModel
        model = SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path), seed=1, timestamp_dir=False)
        eng = SSDEngine(classes=81, seed=1)
        image, tgt = fixed_batch(model, 2)
        return model, eng, ops.image_prep(image.contiguous(), normalize=False), tuple(tgt), image
    model, eng = V.make_model(tmp_path), V.make_engine()
    x, gt = V.fixed_batch(ops)
    return model, eng, x, tuple(ops.match_encode(*gt, model._pset, 0.5)), x


def loss_rows(ops, spec, pconf, ploc, tgt, hg, priors):
    """the loss call a step of `spec` makes, spelled out"""
    if spec is None:
        return ops.ssd_loss_heads(pconf, ploc, *tgt, hg)
    if spec.kind == "multibox":
        if spec.box == "smooth_l1":
            return ops.multibox_loss_heads(pconf, ploc, *tgt, hg, spec.neg_pos_ratio, spec.loc_weight)      # the call as it was
        return ops.multibox_loss_heads(pconf, ploc, *tgt, hg, spec.neg_pos_ratio, spec.loc_weight, box=spec.box, priors=priors)
    return ops.softmax_focal_loss_heads(pconf, ploc, *tgt, hg, spec.gamma, spec.alpha, spec.loc_weight, box=spec.box, priors=priors)


def two_steps(ops, network, tmp_path, spec):
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model, eng, x, tgt, image = setup(ops, network, tmp_path)
    opt = optimizers.Adam(1e-3)
    cfg = SSDObjectDetectionModel.TrainConfig(1, 2, opt, warmup=False, loss=spec)
    raws = []
    for step in range(2):
        conf_m, loc_m, info = model._train_step(image, *tgt, opt, cfg=cfg)
        ploc, pconf = eng.forward(x)
        assert torch.equal(ploc, loc_m) and torch.equal(pconf, conf_m)
        hg = eng.head_grad_buffers(2)
        out8 = loss_rows(ops, spec, pconf, ploc, tgt, hg, model._pset.priors)
        eng.backward(None, None, heads=hg)
        eng.clip_scales(0.01)
        eng.adam(1e-3, eng.grad, 1.0, True)
        torch.cuda.synchronize()
        assert torch.equal(out8.view(torch.int32), model._last_raw.view(torch.int32)), (step, out8, model._last_raw)
        assert float(info["status"]) == 0.0 and bool(torch.isfinite(out8).all())
        for name, i in (("loc loss", 0), ("cls loss pos", 1), ("cls loss neg", 2)):
            assert float(info[name]) == float(out8[i])
        for name in STATE:
            assert torch.equal(getattr(model.get_engine(), name), getattr(eng, name)), (step, name)
        raws.append(out8.clone())
    assert opt.iterations == 2
    return raws


@pytest.mark.parametrize("network", ["ssd300", "vgg16_ssd300"])
@pytest.mark.parametrize("loss,box", [("multibox", "giou"), ("softmax_focal", "ciou")])
def test_model_step_equals_the_hand_composed_step(ops, tmp_path, network, loss, box):
    spec = ops.LossSpec(loss, loc_weight=0.5, box=box)
    raws = two_steps(ops, network, tmp_path, spec)
    # an IoU loss of a positive lies in [0, 2] (CIoU: [0, 3]), so L_loc = loc_weight * mean lies in [0, 1] ([0, 1.5])
    assert 0.0 < float(raws[0][0]) <= (1.5 if box == "ciou" else 1.0)


@pytest.mark.parametrize("network", ["ssd300", "vgg16_ssd300"])
@pytest.mark.parametrize("loss", [None, "multibox"], ids=["default", "multibox"])
def test_default_and_smooth_l1_steps_are_what_they_were(ops, tmp_path, network, loss):
    """the step of the default loss against ssd_loss_heads, and of LossSpec("multibox") against multibox_loss_heads called
    without box / priors: the priors the model now hands to _ssd_loss change nothing"""
    two_steps(ops, network, tmp_path, None if loss is None else ops.LossSpec(loss))


def test_ssd_loss_without_priors_keeps_working_and_refuses_an_iou_kind(ops, tmp_path):
    """the staticmethod's existing call shapes; an IoU kind without priors is a ValueError, not a launch"""
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model, eng, x, tgt, image = setup(ops, "ssd300", tmp_path)
    ploc, pconf = eng.forward(x)
    cls, loc, mask = tgt
    a = SSDObjectDetectionModel._ssd_loss((cls, loc, mask), (ploc, pconf), None, "multibox")
    b = SSDObjectDetectionModel._ssd_loss((cls, loc, mask), (ploc, pconf), None, "multibox", model._pset)
    assert torch.equal(a[1]["raw"].view(torch.int32), b[1]["raw"].view(torch.int32)) and torch.equal(a[1]["dloc"], b[1]["dloc"])
    with pytest.raises(ValueError):
        SSDObjectDetectionModel._ssd_loss((cls, loc, mask), (ploc, pconf), None, ops.LossSpec("multibox", box="giou"))
    c = SSDObjectDetectionModel._ssd_loss((cls, loc, mask), (ploc, pconf), None, ops.LossSpec("multibox", box="giou"), model._pset)
    assert float(c[1]["status"]) == 0.0 and not torch.equal(c[1]["dloc"], a[1]["dloc"])
    assert torch.equal(c[1]["dconf"].view(torch.int16), a[1]["dconf"].view(torch.int16))


def test_yaml_run_with_box_diou(tmp_path):
    from ssd_object_detection_amd.tools import train as T
    cfg = T.load_config(os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml"))
    cfg["data"]["mini_batch"]["num_data"] = 16
    cfg["model"]["log_dir"] = str(tmp_path)
    cfg["model"]["train"]["batch_size"] = 8
    cfg["model"]["train"]["loss"] = {"kind": "multibox", "box": "diou", "loc_weight": 1.0}
    cfg["model"]["split_train"]["batch_size"] = 4
    cfg["model"]["warmup"]["step"] = 2
    cfg["model"]["log_interval"] = 1
    model = T.train(cfg)
    info = {k: float(v) for k, v in model.last_info.items()}
    assert info["status"] == 0 and all(np.isfinite(v) for v in info.values())
    rows = [json.loads(line) for line in open(os.path.join(model.get_log_dir(), "scalars.jsonl")) if line.strip()]
    loc = [r["value"] for r in rows if r["tag"] == "train/loc loss"]
    assert len(loc) >= 2 and all(np.isfinite(r["value"]) for r in rows)   # two steps or more
    assert all(0.0 < v <= 2.0 for v in loc), loc                          # a mean of DIoU losses, each in [0, 2], weight 1
    saved = json.load(open(os.path.join(model.get_log_dir(), "config.json")))
    assert saved["model"]["train"]["loss"] == {"kind": "multibox", "box": "diou", "loc_weight": 1.0}
