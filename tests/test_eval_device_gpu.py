"""GPU: the evaluation metric on the device.  ssd_eval_match against its plain-Python restatement (tests/eval_cases.py) bit
for bit, ssd_eval_ap against utils.metrics (host restatement of the same stage), evaluate(metric="device") against
evaluate(metric="host"), reader-contract validation splits, and validation inside a training run."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import eval_cases as E                                    # noqa: E402

M = E.M


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def dense_batch(dets, gts, anchors, A=E.A, seed=0):
    """The dense [B, A] maps ssd_score_decode + ssd_nms would leave for these detections (kept anchors at the given sorted
    positions; everything else random scores / classes / boxes with keep = 0) and the CSR ground truth, on the device."""
    rng = np.random.default_rng(seed)
    B = len(dets)
    score = rng.uniform(0.0, 1.0, (B, A)).astype(np.float32)
    cls = rng.integers(0, E.N_CLS + 2, (B, A)).astype(np.int32)
    box = rng.uniform(1.0, 299.0, (B, A, 4)).astype(np.float32)
    keep = np.zeros((B, A), np.uint8)
    for i, ((s, c, b), anc) in enumerate(zip(dets, anchors)):
        score[i, anc], cls[i, anc], box[i, anc], keep[i, anc] = s, c, b, 1
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(g[0]) for g in gts])
    gcls = np.concatenate([g[0] for g in gts]).astype(np.int32)
    gbox = np.concatenate([g[1].reshape(-1, 4) for g in gts]).astype(np.float64)
    return [torch.from_numpy(x).cuda() for x in (score, cls, box, keep, gcls, gbox, off)]


def check_match(ops, dets, gts, anchors, max_dets, A=E.A):
    want, _ = E.match_reference(dets, gts, max_dets)
    n_det, d_score, d_cls, d_box, d_flags = [t.cpu().numpy() for t in ops.eval_match(*dense_batch(dets, gts, anchors, A), max_dets)]
    d_flags = d_flags.view(np.uint16)
    assert d_score.shape == (len(dets), max_dets) and d_box.shape == (len(dets), max_dets, 4)
    for i, (s, c, b, f) in enumerate(want):
        k = len(s)
        assert n_det[i] == k, (i, n_det[i], k)
        assert np.array_equal(d_cls[i, :k], c), i
        assert np.array_equal(d_score[i, :k].view(np.uint32), s.view(np.uint32)), i
        assert np.array_equal(d_box[i, :k].view(np.uint32), b.view(np.uint32)), i
        assert np.array_equal(d_flags[i, :k], f), (i, np.nonzero(d_flags[i, :k] != f)[0], d_flags[i, :k] ^ f)
        assert (d_score[i, k:] == 0).all() and (d_cls[i, k:] == -1).all() and (d_box[i, k:] == 0).all() and (d_flags[i, k:] == 0).all()
    return want


@pytest.mark.parametrize("name", sorted(E.REGIMES))
def test_eval_match_equals_the_restatement(ops, name):
    """n_det, classes, the bits of scores and boxes and every flag of every threshold, no case left out, no tolerance."""
    dets, gts, anchors = E.regime(name)
    want = check_match(ops, dets, gts, anchors, 100)
    if name != "sparse":
        assert sum(int(np.count_nonzero(w[3])) for w in want) > 40             # true positives exist
    if name == "cut_in_ties":
        check_match(ops, dets, gts, anchors, 20)
        check_match(ops, dets, gts, anchors, ops.eval_max_dets())
        check_match(ops, dets, gts, anchors, 1)


def test_eval_match_any_number_of_ground_truths_and_kept_anchors(ops):
    """More ground truths per image than the kernel caches in LDS (0 .. 150, so both of its paths run in one batch), and more
    kept anchors than its sort holds (the exact radix cut, with quantised scores so that the cut falls inside ties)."""
    rng = np.random.default_rng(77)
    dets, gts, anchors = E.gen(rng, 12, 60, 128, quant=20, n_gt_hi=150)
    assert max(len(g[0]) for g in gts) > 64 and min(len(g[0]) for g in gts) < 48
    check_match(ops, dets, gts, anchors, 100)
    dets, gts, anchors = E.gen(rng, 6, 900, 1600, quant=50)
    assert max(len(d[0]) for d in dets) > 1024 > min(len(d[0]) for d in dets)
    check_match(ops, dets, gts, anchors, 100)
    check_match(ops, dets, gts, anchors, 128)
    # an anchor count that is not a multiple of four (the byte-wise sweep of the keep map)
    dets, gts, anchors = E.gen(rng, 3, 20, 40)
    inside = [a < 8731 for a in anchors]
    dets = [(s[m], c[m], b[m]) for (s, c, b), m in zip(dets, inside)]
    check_match(ops, dets, gts, [a[m] for a, m in zip(anchors, inside)], 100, A=8731)


def sorted_rows(rows, C):
    cls, score, flags = rows
    order = np.lexsort((np.arange(len(cls)), -score.astype(np.float64), cls))
    seg = np.zeros(C + 1, np.int32)
    seg[1:] = np.cumsum(np.bincount(cls, minlength=C)[:C])
    return flags[order], seg


@pytest.mark.parametrize("name", sorted(E.REGIMES))
def test_eval_ap_equals_the_host_stage(ops, name):
    dets, gts, _ = E.regime(name)
    _, rows = E.match_reference(dets, gts, 100)
    C = E.N_CLS + 2
    n_gt = np.zeros(C, np.int32)
    for c, n in E.gt_counts(gts).items():
        n_gt[c] = n
    flags, seg = sorted_rows(rows, C)
    ap = ops.eval_ap(torch.from_numpy(flags.view(np.int16)).cuda(), torch.from_numpy(seg).cuda(), torch.from_numpy(n_gt).cuda())
    ap = ap.cpu().numpy()
    table = M.ap_table_from_flags(rows, n_gt)
    assert set(table) == set(np.nonzero(n_gt)[0].tolist())
    for c in range(C):
        want = table.get(c, [0.0] * 10)
        print(name, c, float(np.abs(ap[c] - want).max()))
        assert np.abs(ap[c] - np.asarray(want)).max() <= 1e-12, (c, ap[c], want)


def test_eval_ap_long_segments(ops):
    """A class segment far longer than one chunk of the scan (and than LDS), beside an empty one."""
    rng = np.random.default_rng(5)
    C, N = 3, 300000
    cls = np.sort(rng.choice([0, 2], N, p=[0.9, 0.1])).astype(np.int64)
    score = rng.uniform(0, 1, N).astype(np.float32)
    flags = (rng.integers(0, 1024, N) & rng.integers(0, 1024, N)).astype(np.uint16)
    n_gt = np.array([200000, 5, 40000], np.int32)                    # class 1: ground truth, no detections -> AP 0
    rows = (cls, score, flags)
    fs, seg = sorted_rows(rows, C)
    ap = ops.eval_ap(torch.from_numpy(fs.view(np.int16)).cuda(), torch.from_numpy(seg).cuda(), torch.from_numpy(n_gt).cuda())
    ap = ap.cpu().numpy()
    table = M.ap_table_from_flags(rows, n_gt)
    for c in range(C):
        assert np.abs(ap[c] - np.asarray(table[c])).max() <= 1e-12, (c, ap[c], table[c])
    assert (ap[1] == 0).all() and ap[0].min() > 0


def spread_model(tmp_path, seed=4):
    """The network of test_evaluate_scores_exactly_what_the_oracle_keeps: conf biases background +2, classes N(0, 1.5), so
    that scores cover a range and NMS has work."""
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = SSDObjectDetectionModel(classes=80, log_dir=str(tmp_path), timestamp_dir=False, seed=seed)
    spread_biases(model)
    return model


def spread_biases(model):
    eng = model.get_engine()
    g = torch.Generator().manual_seed(0)
    for lvl, (wt, bt) in enumerate(eng.head_params):
        n = eng.num_priors[lvl]
        b = torch.zeros(bt.numel)
        cb = torch.randn((n, 81), generator=g) * 1.5
        cb[:, 80] += 2.0
        b[n * 4:] = cb.reshape(-1)
        eng.param[bt.offset:bt.offset + bt.numel] = b.cuda()


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


def test_evaluate_device_equals_host(tmp_path):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    _, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=70).get_dataset()
    samples = list(val)
    assert len(samples) == 7
    model = spread_model(tmp_path)
    for max_dets in (100, 20):
        host, hdets = model.evaluate(samples, batch_size=4, score_thresh=0.2, max_dets=max_dets, return_detections=True)
        dev, ddets = model.evaluate(samples, batch_size=4, score_thresh=0.2, max_dets=max_dets, return_detections=True,
                                    metric="device")
        assert min(len(d[0]) for d in hdets) >= 20
        assert_same_result(dev, host)
        for (s, c, b), (ws, wc, wb) in zip(ddets, top_cut(hdets, max_dets)):
            assert np.array_equal(s, ws) and np.array_equal(c, wc) and np.array_equal(b, wb)
    # the same with ground truth that the detections hit (a random network finds none of the synthetic boxes: AP 0 on both
    # sides): every image's ground truth = five of its own detections, so that true positives, ties and the cut all count
    hit = []
    for (img, _, _), (s, c, b) in zip(samples, hdets):
        pick = np.arange(0, len(s), max(1, len(s) // 5))[:5]
        hit.append((img, c[pick].astype(np.float32), (b[pick] / np.float32(300.0)).astype(np.float32)))
    for max_dets in (100, 20):
        host = model.evaluate(hit, batch_size=4, score_thresh=0.2, max_dets=max_dets)
        dev = model.evaluate(hit, batch_size=4, score_thresh=0.2, max_dets=max_dets, metric="device")
        print("max_dets", max_dets, "host", host["mAP"], host["AP50"], "device", dev["mAP"], dev["AP50"])
        assert host["AP50"] > 0.0                                  # some detection is a true positive
        assert_same_result(dev, host)
    with pytest.raises(ValueError):
        model.evaluate(samples, metric="gpu")
    with pytest.raises(ValueError):
        model.evaluate(samples, metric="device", max_dets=1000)


def test_device_batch_loop_never_synchronises(tmp_path):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    from ssd_object_detection_amd.utils.device_map import DeviceMapAccumulator
    _, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=90).get_dataset()
    samples = list(val)
    model = spread_model(tmp_path)
    host = model.evaluate(samples, batch_size=4, score_thresh=0.2)
    model.evaluate(samples, batch_size=4, score_thresh=0.2, metric="device")          # builds caches (allocations sync)
    acc = DeviceMapAccumulator(80, 100, model.device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                        # any torch-side host sync now raises
    try:
        model.evaluate_into(acc, samples, batch_size=4, score_thresh=0.2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_same_result(acc.result(), host)


def test_reader_contract_validation_split(tmp_path):
    """Images of different sizes, uint8, COCO top-left boxes -> SSDDataLoader(dataset=reader) -> evaluate(val split): both
    metric modes work and agree."""
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    from ssd_object_detection_amd.data_loaders.synthetic import synth_raw_sample

    class Reader:
        def _gen(self, first, n):
            for i in range(first, first + n):
                img, cls, tlwh = synth_raw_sample(i)
                box = tlwh.copy()
                box[:, :2] += box[:, 2:] / 2
                yield img, cls, box

        def get_dataset(self):
            return list(self._gen(0, 4)), list(self._gen(100, 6))

    _, val = SSDDataLoader("unused", dataset=Reader()).get_dataset()
    assert getattr(val, "raw", False)
    model = spread_model(tmp_path)
    host, hdets = model.evaluate(val, batch_size=4, score_thresh=0.2, return_detections=True)
    dev, ddets = model.evaluate(val, batch_size=4, score_thresh=0.2, return_detections=True, metric="device")
    assert len(hdets) == 6 and min(len(d[0]) for d in hdets) >= 20
    assert_same_result(dev, host)
    for (s, c, b), (ws, wc, wb) in zip(ddets, top_cut(hdets, 100)):
        assert np.array_equal(s, ws) and np.array_equal(c, wc) and np.array_equal(b, wb)


def test_validation_inside_a_training_run(tmp_path, monkeypatch):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    from ssd_object_detection_amd.tools import train as T
    from ssd_object_detection_amd.utils.scalar_log import TAGS, read_scalars

    # an untrained network scores 1/81 everywhere: give the run's network the spread biases, so that the metric has work
    real_init = SSDObjectDetectionModel.__init__

    def init(self, *a, **k):
        real_init(self, *a, **k)
        spread_biases(self)

    monkeypatch.setattr(SSDObjectDetectionModel, "__init__", init)

    def cfg_for(sub, validate):
        cfg = T.load_config(os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml"))
        cfg["data"]["mini_batch"]["num_data"] = 40
        cfg["data"]["shuffle"] = False
        cfg["model"]["log_dir"] = str(tmp_path / sub)
        cfg["model"]["train"]["batch_size"] = 4
        cfg["model"]["train"]["epoch"] = 2
        cfg["model"]["train"]["lr"]["initial"] = 1e-5
        cfg["model"]["split_train"]["enable"] = False
        cfg["model"]["warmup"]["enable"] = False
        cfg["model"]["log_interval"] = 100
        if validate:
            cfg["model"]["eval"] = dict(enable=True, every=1, batch_size=4, score_thresh=0.2, num_data=3)
        return cfg

    with_val = T.train(cfg_for("val", True))
    without = T.train(cfg_for("plain", False))
    # the pass does not disturb the training state
    assert with_val.get_engine().step_count == without.get_engine().step_count == 20
    for name in ("param", "adam_m", "adam_v"):
        assert torch.equal(getattr(with_val.get_engine(), name), getattr(without.get_engine(), name)), name
    plain = read_scalars(os.path.join(without.get_log_dir(), "scalars.jsonl"))
    assert set(plain) == {"train/" + t for t in TAGS}                       # validation off: exactly today's tags
    got = read_scalars(os.path.join(with_val.get_log_dir(), "scalars.jsonl"))
    assert set(got) == set(plain) | {"val/mAP", "val/AP50", "val/AP75"}
    assert {k: v for k, v in got.items() if k in plain} == plain
    lines = [l for l in open(os.path.join(with_val.get_log_dir(), "scalars.jsonl"))]
    tags = [l.split('"tag": "')[1].split('"')[0] for l in lines]
    assert tags[50:53] == ["val/mAP", "val/AP50", "val/AP75"] and tags[-3:] == tags[50:53]   # behind each epoch's train lines
    # values: evaluate(metric="host") on the epoch checkpoints, same samples
    _, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=40).get_dataset()
    samples = list(val)[:3]
    for epoch in range(2):
        m = real_model(real_init, tmp_path / ("ck%d" % epoch))
        m.load(os.path.join(with_val.get_log_dir(), "model_weight", "model_weight_epoch_%d.pt" % epoch))
        host = m.evaluate(samples, batch_size=4, score_thresh=0.2)
        for tag, key in (("val/mAP", "mAP"), ("val/AP50", "AP50"), ("val/AP75", "AP75")):
            step, value = got[tag][epoch]
            assert step == 10 * (epoch + 1)
            assert abs(value - host[key]) <= 1e-12, (epoch, tag, value, host[key])


def real_model(real_init, log_dir):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    m = SSDObjectDetectionModel.__new__(SSDObjectDetectionModel)
    real_init(m, classes=80, log_dir=str(log_dir), timestamp_dir=False, seed=9)
    return m
