"""GPU: the MultiBox loss through the model -- TrainConfig(loss="multibox") in _train_step, and the YAML path of tools/train."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import multibox_oracle as M                               # noqa: E402


def fixed_batch(model, B=4, first=900):
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    cls_l, box_l = synth_batch_gt(first, B)
    return model.make_batch([synth_image(first + i) for i in range(B)], cls_l, box_l)


def test_train_step_logs_the_oracles_scalars_and_lowers_the_loss(tmp_path):
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path), seed=1, timestamp_dir=False)
    image, (cls, loc, mask) = fixed_batch(model)
    opt = optimizers.Adam(1e-3)
    cfg = SSDObjectDetectionModel.TrainConfig(1, 4, opt, warmup=False, loss="multibox")
    totals = []
    for step in range(20):
        pred_conf, pred_loc, info = model._train_step(image, cls, loc, mask, opt, cfg=cfg)
        raw = model._last_raw.cpu().numpy()
        assert raw[7] == 0.0
        totals.append(float(raw[3]))
        if step in (0, 19):
            ref = M.multibox_loss(cls.cpu().numpy(), loc.cpu().numpy(), mask.cpu().numpy(), pred_loc.float().cpu().numpy(),
                                  pred_conf.float().cpu().numpy())
            print("step", step, "out8", raw.tolist(), "oracle", ref["loc"], ref["pos"], ref["neg"], ref["total"])
            for i, key in enumerate(("loc", "pos", "neg", "total")):
                assert abs(raw[i] - ref[key]) <= 1e-4 * abs(ref[key]), (step, key, raw[i], ref[key])
            assert int(raw[4]) == ref["num_pos"] and abs(int(raw[5]) - ref["num_neg"]) <= 2 * image.shape[0]
            for name, i in (("loc loss", 0), ("cls loss pos", 1), ("cls loss neg", 2)):
                assert float(info[name]) == raw[i]
    assert totals[-1] < totals[0], totals


def test_fused_and_unfused_optimizer_agree_bitwise(tmp_path):
    """as tests/test_train_gpu.py checks for the reference loss: Adam per bucket inside the backward pass changes when kernels
    run, not what they compute"""
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel

    def run(fused):
        model = SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path), timestamp_dir=False)
        model.fused_optimizer = fused
        image, (cls, loc, mask) = fixed_batch(model, 4, 300)
        opt = optimizers.Adam(optimizers.ExponentialDecay(1e-3, 100, 0.9))
        cfg = SSDObjectDetectionModel.TrainConfig(1, 4, opt, warmup=False, loss="multibox")
        raws = []
        for _ in range(3):
            model._train_step(image, cls, loc, mask, opt, cfg=cfg)
            raws.append(model._last_raw.clone())
        torch.cuda.synchronize()
        return model.get_engine(), raws

    a, ra = run(False)
    b, rb = run(True)
    for name in ("param", "adam_m", "adam_v", "param_bf16"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(ra, rb))
    assert float(ra[0][7]) == 0.0


def test_yaml_run_with_the_loss_section(tmp_path):
    from ssd_object_detection_amd.tools import train as T
    cfg = T.load_config(os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml"))
    cfg["data"]["mini_batch"]["num_data"] = 16
    cfg["model"]["log_dir"] = str(tmp_path)
    cfg["model"]["train"]["batch_size"] = 8
    cfg["model"]["train"]["loss"] = {"kind": "multibox", "neg_pos_ratio": 3, "loc_weight": 1.0}
    cfg["model"]["split_train"]["batch_size"] = 4
    cfg["model"]["warmup"]["step"] = 2
    cfg["model"]["log_interval"] = 1
    model = T.train(cfg)
    info = {k: float(v) for k, v in model.last_info.items()}
    assert info["status"] == 0 and all(np.isfinite(v) for v in info.values())
    path = os.path.join(model.get_log_dir(), "scalars.jsonl")
    rows = [json.loads(line) for line in open(path) if line.strip()]
    assert rows
    assert {r["tag"] for r in rows} >= {"train/loc loss", "train/cls loss pos", "train/cls loss neg", "train/loss"}
    assert all(np.isfinite(r["value"]) for r in rows)                   # (a status other than 0 raises in ScalarLog.flush)
    saved = json.load(open(os.path.join(model.get_log_dir(), "config.json")))
    assert saved["model"]["train"]["loss"]["kind"] == "multibox"
