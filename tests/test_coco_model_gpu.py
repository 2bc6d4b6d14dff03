"""GPU, model level: SSD300 fed from a COCO directory whose samples are still JPEG (dataset="coco", decode on the device)
against the same samples as decoded arrays -- training batches, evaluation, and a tools.train run."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import jpeg_cases as C                                      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def coco(tmp_path_factory):
    root = tmp_path_factory.mktemp("coco")
    return str(root), C.build_coco(root, categories=C.CATEGORIES_80)


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    return SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path_factory.mktemp("log")), timestamp_dir=False)


def _splits(root, layout):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    enc = SSDDataLoader(root, dataset="coco", shuffle=False)
    dec = SSDDataLoader(root, dataset=C.DecodedReader(layout, C.CATEGORIES_80), shuffle=False)
    assert enc.get_names_and_colors()[0] == dec.get_names_and_colors()[0] and len(enc.get_names_and_colors()[0]) == 80
    return enc.get_dataset(), dec.get_dataset()


@pytest.mark.parametrize("augment", [False, True])
def test_make_batch_raw_on_encoded_samples_equals_decoded(coco, model, augment):
    from ssd_object_detection_amd import ops
    (enc_train, _), (dec_train, _) = _splits(*coco)
    enc, dec = list(enc_train)[:4], list(dec_train)[:4]
    assert all(isinstance(s[0], ops.EncodedImage) for s in enc) and all(isinstance(s[0], np.ndarray) for s in dec)
    for e, d in zip(enc, dec):
        assert np.array_equal(e[1], d[1]) and np.array_equal(e[2], d[2])
    spec = ops.AugmentSpec(seed=0) if augment else None
    xe, te = model.make_batch_raw([s[0] for s in enc], [s[1] for s in enc], [s[2] for s in enc], augment=spec)
    xd, td = model.make_batch_raw([s[0] for s in dec], [s[1] for s in dec], [s[2] for s in dec], augment=spec)
    assert xe.shape == (4, 300, 300, 8) and torch.equal(xe, xd)
    for a, b in zip(te, td):
        assert torch.equal(a, b)
    assert model.last_decode_stats.fallback == 0 and model.last_decode_stats.device == 4
    # a mix of encoded and decoded samples gives the same batch again
    mixed = [enc[0][0], dec[1][0], enc[2][0], dec[3][0]]
    xm, tm = model.make_batch_raw(mixed, [s[1] for s in enc], [s[2] for s in enc], augment=spec)
    assert torch.equal(xm, xd) and all(torch.equal(a, b) for a, b in zip(tm, td))


def test_get_train_set_batches_encoded_samples(coco, model):
    (enc_train, _), (dec_train, _) = _splits(*coco)
    be = list(model.get_train_set(enc_train, batch_size=4))
    bd = list(model.get_train_set(dec_train, batch_size=4))
    assert len(be) == len(bd) == 1                                     # seven samples: one batch, the remainder dropped
    assert torch.equal(be[0][0], bd[0][0]) and all(torch.equal(a, b) for a, b in zip(be[0][1], bd[0][1]))
    # a data-parallel rank reads only its own files
    half = list(model.get_train_set(enc_train, batch_size=4, shard=(1, 2)))
    assert torch.equal(half[0][0], be[0][0][2:4])


def test_evaluate_through_the_coco_loader_equals_decoded_samples(coco, model):
    from ssd_object_detection_amd.utils.metrics import COCO_SUMMARY_KEYS
    (_, enc_val), (_, dec_val) = _splits(*coco)
    kw = dict(batch_size=4, score_thresh=0.0001, protocol="coco", metric="device")
    re, rd = model.evaluate(enc_val, **kw), model.evaluate(dec_val, **kw)
    for key in COCO_SUMMARY_KEYS:
        assert re[key] == rd[key] or (np.isnan(re[key]) and np.isnan(rd[key])), (key, re[key], rd[key])
    he = model.evaluate(enc_val, batch_size=3, score_thresh=0.0001, protocol="map", metric="host")
    hd = model.evaluate(dec_val, batch_size=3, score_thresh=0.0001, protocol="map", metric="host")
    assert all(he[k] == hd[k] for k in ("mAP", "AP50", "AP75"))


def _train_config(root, log_dir, decode):
    from ssd_object_detection_amd.tools import train as T
    cfg = T.load_config(os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml"))
    cfg["data"].update(dataset="coco", dataset_root=root, num_classes=80, decode=decode, decode_workers=2)
    cfg["data"]["mini_batch"]["enable"] = False
    cfg["model"]["log_dir"] = log_dir
    cfg["model"]["train"]["batch_size"] = 4
    cfg["model"]["split_train"]["batch_size"] = 4
    cfg["model"]["warmup"]["step"] = 1
    cfg["model"]["log_interval"] = 1
    cfg["model"]["eval"].update(enable=True, batch_size=4, protocol="coco")
    return cfg


def test_training_run_decode_device_equals_decode_host(coco, tmp_path):
    """tools.train on the directory: one warm-up step and one training step of four images, then validation; the scalars of
    the run that decodes on the device equal those of the run that decodes with Pillow"""
    from ssd_object_detection_amd.tools import train as T
    from ssd_object_detection_amd.utils.scalar_log import read_scalars
    root, _ = coco
    model = T.train(_train_config(root, str(tmp_path / "device"), "device"))
    assert model.decode_workers == 2 and model.last_decode_stats.fallback == 0
    dev = read_scalars(os.path.join(model.get_log_dir(), "scalars.jsonl"))
    assert any(t.startswith("train/") for t in dev) and any(t.startswith("warmup/") for t in dev) and "val/mAP" in dev
    for tag, rows in dev.items():
        if not tag.startswith("val/"):
            assert all(np.isfinite(v) for _, v in rows), (tag, rows)
    with pytest.raises(ValueError, match="num_classes"):
        bad = _train_config(root, str(tmp_path / "bad"), "device")
        bad["data"]["num_classes"] = 79
        T.train(bad)
    try:
        import PIL  # noqa: F401
    except ImportError:
        pytest.skip("Pillow is not installed: no decode='host' run to compare with (the device run above passed)")
    host_model = T.train(_train_config(root, str(tmp_path / "host"), "host"))
    host = read_scalars(os.path.join(host_model.get_log_dir(), "scalars.jsonl"))
    assert set(host) == set(dev)
    for tag in dev:
        assert len(dev[tag]) == len(host[tag])
        for (s1, v1), (s2, v2) in zip(dev[tag], host[tag]):
            assert s1 == s2 and (v1 == v2 or (np.isnan(v1) and np.isnan(v2))), (tag, dev[tag], host[tag])
