"""GPU, model level: PASCAL VOC through SSDObjectDetectionModel on a small VOCdevkit tree built from the JPEG fixtures --
evaluate(protocol="voc07" | "voc12") with metric="device" against metric="host" for SSD300 and the VGG-16 SSD300 network, both
scoring modes; the batch loop without synchronisation; encoded samples against decoded ones; a tools.train run on the tree.

The host metric, utils.metrics.voc_map, is build-defined: a numpy restatement of the published VOCdevkit procedure, unpinned
(see tests/voc_cases.py).  Bound: 1e-12 between the two metric modes (the project's bound for its AP kernels); equality where
the same rows go through the same code."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import jpeg_cases as C                                     # noqa: E402
from tests import voc_cases as V                                      # noqa: E402

CLASSES = 20


@pytest.fixture(scope="module")
def voc(tmp_path_factory):
    root = tmp_path_factory.mktemp("voc")
    return str(root), V.build_devkit(root)


def spread_biases(model):
    """conf biases background +2, classes N(0, 1.5): scores cover a range and NMS has work (tests/test_eval_device_gpu.py's,
    for 20 classes)"""
    eng = model.get_engine()
    g = torch.Generator().manual_seed(0)
    for lvl, (wt, bt) in enumerate(eng.head_params):
        n = eng.num_priors[lvl]
        b = torch.zeros(bt.numel)
        cb = torch.randn((n, CLASSES + 1), generator=g) * 1.5
        cb[:, CLASSES] += 2.0
        b[n * 4:] = cb.reshape(-1)
        eng.param[bt.offset:bt.offset + bt.numel] = b.cuda()


def make_model(log_dir, network=None, **kw):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = SSDObjectDetectionModel(classes=CLASSES, log_dir=str(log_dir), seed=4, timestamp_dir=False, network=network, **kw)
    spread_biases(model)
    return model


class DecodedReader:
    """The reader contract over the tree's layout, yielding the committed decoded arrays"""

    def __init__(self, layout):
        self.layout = layout

    def _split(self, pairs):
        out = []
        for pair in pairs:
            for image_id, objs in self.layout[pair]:
                if not objs:
                    continue
                box = np.array([(o[1] - 1 + (o[3] - o[1] + 1) / 2, o[2] - 1 + (o[4] - o[2] + 1) / 2, o[3] - o[1] + 1,
                                 o[4] - o[2] + 1) for o in objs], np.float32)
                out.append((C.decoded(image_id), np.array([V.VOC_NAMES.index(o[0]) for o in objs], np.float32), box,
                            np.array([o[5] for o in objs], np.uint8)))
        return out

    def get_dataset(self):
        return self._split((("2007", "trainval"), ("2012", "trainval"))), self._split((("2007", "test"),))


def hit_samples(samples, hdets, size):
    """ground truth the detections hit, as reader-contract samples: eight of every image's own detections as top-left source
    pixel boxes, the second and the fifth difficult, the third a near copy of the first with the first's class (a second box
    that the first box's detections also pass: duplicates)"""
    out = []
    for smp, (s, c, b) in zip(samples, hdets):
        pick = np.arange(0, len(s), max(1, len(s) // 8))[:8]
        h, w = smp[0].shape[:2]
        box = b[pick].astype(np.float64) * np.array([w, h, w, h]) / size
        cls = c[pick].astype(np.float32)
        box[2], cls[2] = box[0] * np.array([1.02, 1.0, 1.0, 1.0]), cls[0]
        box[:, :2] -= box[:, 2:] / 2
        hard = np.zeros(len(pick), np.uint8)
        hard[[1, 4]] = 1
        out.append((smp[0], cls, box.astype(np.float32), hard))
    return out


def assert_same_voc(dev, host, tol=1e-12):
    assert set(dev) == set(host) == {"mAP", "per_class", "n_pos"}
    assert dev["n_pos"] == host["n_pos"] and set(dev["per_class"]) == set(host["per_class"])
    print("mAP", dev["mAP"], host["mAP"])
    assert abs(dev["mAP"] - host["mAP"]) <= tol
    for c, v in host["per_class"].items():
        assert abs(dev["per_class"][c] - v) <= tol, (c, dev["per_class"][c], v)


def check_network(model, voc, precisions=("bf16",)):
    from ssd_object_detection_amd import ops
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    from ssd_object_detection_amd.models.ssd_model import _RawList
    root, layout = voc
    _, val = SSDDataLoader(root, dataset="pascal_voc", shuffle=False).get_dataset()
    samples = list(val)
    assert len(samples) == 5 and all(isinstance(s[0], ops.EncodedImage) for s in samples)
    kw = dict(batch_size=3, score_thresh=0.2)
    # the tree's own boxes: both modes see the same positives and agree (random weights: the APs are whatever they are)
    for protocol in ("voc07", "voc12"):
        host = model.evaluate(val, protocol=protocol, **kw)
        dev = model.evaluate(val, protocol=protocol, metric="device", **kw)
        assert_same_voc(dev, host)
        want = {}
        for _, objs in layout[("2007", "test")]:
            for o in objs:
                if not o[5]:
                    want[V.VOC_NAMES.index(o[0])] = want.get(V.VOC_NAMES.index(o[0]), 0) + 1
        assert host["n_pos"] == dict(sorted(want.items()))
    # boxes the detections hit
    _, hdets = model.evaluate(val, return_detections=True, **kw)
    assert min(len(d[0]) for d in hdets) >= 16
    hit = _RawList(hit_samples(samples, hdets, 300.0))
    results = {}
    for precision in precisions:
        for scoring in ("best", "all"):
            for protocol in ("voc07", "voc12"):
                k2 = dict(kw, scoring=scoring, protocol=protocol, precision=precision)
                host, hd = model.evaluate(hit, return_detections=True, **k2)
                dev, dd = model.evaluate(hit, return_detections=True, metric="device", **k2)
                assert_same_voc(dev, host)
                assert 0.0 < host["mAP"] < 1.0 and sum(host["n_pos"].values()) == 6 * len(hit)
                results[(precision, scoring, protocol)] = host["mAP"]
                # the rows that were scored: the best max_dets of the host's list, in the device's order
                assert len(hd) == len(dd) == len(hit)
                for (hs, hc, hb), (ds, dc, db) in zip(hd, dd):
                    order = np.argsort(-hs.astype(np.float64), kind="mergesort")[:100]
                    assert np.array_equal(hs[order], ds) and np.array_equal(hc[order], dc) and np.array_equal(hb[order], db)
    assert results[("bf16", "best", "voc07")] != results[("bf16", "best", "voc12")]
    # the difficult flags matter: the same boxes as ordinary ground truth score differently
    plain = model.evaluate(_RawList([h[:3] for h in hit]), protocol="voc07", metric="device", **kw)
    assert plain["n_pos"] != dev["n_pos"] and sum(plain["n_pos"].values()) == 8 * len(hit)
    return hit


def test_evaluate_voc_device_equals_host_ssd300(voc, tmp_path):
    from ssd_object_detection_amd import ops
    from ssd_object_detection_amd.utils.device_map import DeviceVocAccumulator
    model = make_model(tmp_path)
    hit = check_network(model, voc, precisions=("bf16", "mxfp8"))
    kw = dict(batch_size=3, score_thresh=0.2)
    # max_dets beyond the other protocols' 128: SSD's detection output keeps 200
    assert ops.eval_max_dets() == 128 and ops.eval_voc_max_dets() == 256 and ops.detect_max_keep() >= 200
    for scoring in ("best", "all"):
        host = model.evaluate(hit, protocol="voc07", max_dets=200, scoring=scoring, **kw)
        dev = model.evaluate(hit, protocol="voc07", max_dets=200, scoring=scoring, metric="device", **kw)
        assert_same_voc(dev, host)
    with pytest.raises(ValueError):
        model.evaluate(hit, protocol="voc07", max_dets=257, metric="device", **kw)
    with pytest.raises(ValueError):
        model.evaluate(hit, max_dets=200, metric="device", **kw)      # the default protocol keeps its own limit
    for metric in ("host", "device"):
        with pytest.raises(ValueError):
            model.evaluate(hit, protocol="pascal", metric=metric)
        with pytest.raises(ValueError):
            model.evaluate(hit, protocol="voc", metric=metric)
    # the batch loop enqueues only
    host = model.evaluate(hit, protocol="voc12", **kw)
    acc = DeviceVocAccumulator(CLASSES, 100, model.device, year="12")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                            # any torch-side host sync now raises
    try:
        model.evaluate_into(acc, hit, batch_size=3, score_thresh=0.2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_same_voc(acc.result(), host)
    assert len(acc.detections()) == len(hit)


def test_evaluate_voc_device_equals_host_vgg16_ssd300(voc, tmp_path):
    check_network(make_model(tmp_path, network="vgg16_ssd300"), voc)


def test_encoded_samples_equal_decoded_samples(voc, tmp_path):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    root, layout = voc
    model = make_model(tmp_path)
    enc_train, enc_val = SSDDataLoader(root, dataset="pascal_voc", shuffle=False).get_dataset()
    dec_train, dec_val = SSDDataLoader(root, dataset=DecodedReader(layout), shuffle=False).get_dataset()
    enc, dec = list(enc_train)[:4], list(dec_train)[:4]
    for e, d in zip(enc, dec):
        assert isinstance(d[0], np.ndarray) and all(np.array_equal(e[k], d[k]) for k in (1, 2, 3))
    xe, te = model.make_batch_raw([s[0] for s in enc], [s[1] for s in enc], [s[2] for s in enc])
    xd, td = model.make_batch_raw([s[0] for s in dec], [s[1] for s in dec], [s[2] for s in dec])
    assert xe.shape == (4, 300, 300, 8) and torch.equal(xe, xd) and all(torch.equal(a, b) for a, b in zip(te, td))
    assert model.last_decode_stats.fallback == 0 and model.last_decode_stats.device == 4
    for metric in ("device", "host"):
        kw = dict(batch_size=3, score_thresh=0.05, protocol="voc07", metric=metric)
        assert model.evaluate(enc_val, **kw) == model.evaluate(dec_val, **kw)


def _train_config(root, log_dir, protocol="voc07"):
    from ssd_object_detection_amd.tools import train as T
    cfg = T.load_config(os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml"))
    cfg["data"].update(dataset="pascal_voc", dataset_root=root, num_classes=20, shuffle=False, decode_workers=2)
    cfg["data"]["mini_batch"]["enable"] = False
    cfg["model"]["log_dir"] = log_dir
    cfg["model"]["train"]["batch_size"] = 4
    cfg["model"]["train"]["epoch"] = 2
    cfg["model"]["split_train"]["enable"] = False
    cfg["model"]["warmup"]["enable"] = False
    cfg["model"]["log_interval"] = 100
    cfg["model"]["eval"].update(enable=True, batch_size=4, score_thresh=0.2, protocol=protocol)
    return cfg


def test_training_run_on_the_tree_writes_val_map_only(voc, tmp_path):
    from ssd_object_detection_amd.tools import train as T
    from ssd_object_detection_amd.utils.scalar_log import TAGS, read_scalars
    root, _ = voc
    model = T.train(_train_config(root, str(tmp_path / "run")))
    assert model.decode_workers == 2 and model.last_decode_stats.fallback == 0 and model.cfg.classes == 21
    got = read_scalars(os.path.join(model.get_log_dir(), "scalars.jsonl"))
    assert set(got) == {"train/" + t for t in TAGS} | {"val/mAP"}
    assert [s for s, _ in got["val/mAP"]] == [2, 4] and all(0.0 <= v <= 1.0 for _, v in got["val/mAP"])
    for tag, rows in got.items():
        assert all(np.isfinite(v) for _, v in rows), (tag, rows)
    bad = _train_config(root, str(tmp_path / "bad"))
    bad["data"]["num_classes"] = 21
    with pytest.raises(ValueError, match="20 classes"):
        T.train(bad)
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    assert T.val_from_config(_train_config(root, "unused", "voc12"))["protocol"] == "voc12"
    with pytest.raises(ValueError, match="protocol"):
        T.val_from_config(_train_config(root, "unused", protocol="pascal"))
    kw = dict(epoch=1, batch_size=4, optimizer=None, warmup=False)
    assert SSDObjectDetectionModel.TrainConfig(val=dict(protocol="voc07"), **kw).val["protocol"] == "voc07"
    with pytest.raises(ValueError, match="protocol"):
        SSDObjectDetectionModel.TrainConfig(val=dict(protocol="pascal"), **kw)
