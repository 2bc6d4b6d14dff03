"""GPU: COCO's twelve box metrics on the device.  ssd_eval_match_coco against utils.metrics.coco_match_image bit for bit and
ssd_eval_ap_coco against the host stage, both through the C ABI under tests/strict.py (guarded arena, outputs poisoned twice);
the tie to ssd_eval_match where no box is crowd; evaluate(protocol="coco", metric="device") against metric="host" for both
networks, prepared and reader-contract samples; the batch loop without synchronisation; validation inside a training run.

Bounds: bit equality for every output of the match kernel and for tp_count; 1e-12 for AP and for the twelve summary values (the
bound of the existing device metric: the kernel sums the 101 samples in numpy's order, the difference is the envelope's
division order)."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import coco_eval_cases as CC                              # noqa: E402
from tests import strict                                             # noqa: E402

M = CC.M
CASES = [(name, index) for name in sorted(CC.SETS) for index in range(len(CC.BATCHES))]


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


RANGES = np.ascontiguousarray(np.asarray(M.COCO_AREA_RANGES, np.float64).reshape(-1))


def want_tensors(ref):
    return [T(ref["n_det"]), T(ref["score"]), T(ref["cls"]), T(ref["box"]), T(ref["flags"].view(np.int16)),
            T(ref["tp"].view(np.int16)), T(ref["ig"].view(np.int16)), T(ref["pos"]), T(ref["gt_ignore"])]


@pytest.mark.parametrize("name,index", CASES)
def test_eval_match_coco_equals_the_restatement(L, name, index):
    """every output bit for bit, slots beyond n_det zero, nothing written outside the outputs; the crowd and the scale pointer
    non-NULL (the batch as generated) and NULL (one of the three other combinations per batch)"""
    case = CC.case_set(name)[index]
    d = CC.dense_batch(case)
    B, A, md = case["B"], case["A"], case["max_dets"]
    G = len(d["gt_cls"])
    arena = strict.Arena("cuda", strict.Arena.bytes_for(B * A * 4, B * A * 4, B * A * 16, B * A, G * 4, G * 32, 64, G, 64,
                                                        *[B * md * 16] * 8, G))
    ins = {k: arena.put(T(d[k]), k) for k in ("score", "cls", "box", "keep", "gt_cls", "gt_box", "gt_off", "gt_crowd",
                                              "area_scale")}
    outs = [arena.out((B,), torch.int32, "n_det"), arena.out((B, md), torch.float32, "det_score"),
            arena.out((B, md), torch.int32, "det_cls"), arena.out((B, md, 4), torch.float32, "det_box"),
            arena.out((B, md), torch.int16, "det_flags"), arena.out((B, md, 4), torch.int16, "det_tp"),
            arena.out((B, md, 4), torch.int16, "det_ig"), arena.out((B, md), torch.int32, "det_pos"),
            arena.out((G,), torch.uint8, "gt_ignore")]
    thr = dp(M.IOU_THRESHOLDS)

    def call(with_crowd, with_scale):
        status = L.ssd_eval_match_coco(P(ins["score"]), P(ins["cls"]), P(ins["box"]), P(ins["keep"]), B, A, P(ins["gt_cls"]),
                                       P(ins["gt_box"]), P(ins["gt_off"]), P(ins["gt_crowd"] if with_crowd else None),
                                       P(ins["area_scale"] if with_scale else None), dp(RANGES), thr, md,
                                       *[P(t) for t in outs], stream())
        assert status == 0, status

    other = ((False, True), (True, False), (False, False))[index % 3]
    for with_crowd, with_scale in ((True, True), other):
        ref = CC.match_reference(name, index, with_crowd, with_scale)
        assert int(ref["n_det"].max()) == min(md, max(len(x[0]) for x in case["dets"]))
        arena.run(lambda: call(with_crowd, with_scale), list(zip(outs, want_tensors(ref))))


def test_eval_match_coco_without_crowd_is_eval_match(ops):
    """no crowd pointer, no scale, COCO's ranges: det_tp of range "all" and det_flags are ssd_eval_match's flags, det_ig of
    range "all" is 0, and the detection rows are the same"""
    for name, index in (("a", 2), ("b", 3), ("a", 5)):
        case = CC.case_set(name)[index]
        d = {k: T(v).cuda() for k, v in CC.dense_batch(case).items()}
        args = [d[k] for k in ("score", "cls", "box", "keep", "gt_cls", "gt_box", "gt_off")]
        old = ops.eval_match(*args, case["max_dets"])
        new = ops.eval_match_coco(*args, case["max_dets"])
        for a, b in zip(old[:4], new[:4]):
            assert torch.equal(a, b)
        assert torch.equal(new.tp[:, :, 0], old[4]) and torch.equal(new.flags, old[4])
        assert int(new.ig[:, :, 0].abs().max()) == 0 and int(old[4].abs().max()) > 0


def test_eval_ap_coco_equals_the_host_stage(L):
    """AP within 1e-12 and tp_count exact, on matched rows of a generated batch and on rows where two whole chunks of the scan
    are ignored, a class has ground truth and no row, and a class has no ground truth"""
    work = [CC.ap_rows_case()]
    for name, index in (("a", 2), ("b", 4)):
        case, ref = CC.case_set(name)[index], CC.match_reference(name, index)
        C = case["n_cls"] + 2
        work.append(dict(rows=CC.rows_of(ref), n_gt=CC.n_gt_of(case, ref, C), C=C, max_dets=case["max_dets"]))
    for w in work:
        C, md = w["C"], w["max_dets"]
        tp, ig, pos, seg = CC.sorted_rows(w["rows"], C)
        N = len(pos)
        arena = strict.Arena("cuda", strict.Arena.bytes_for(N * 8, N * 8, N * 4, 64, 256, C * 320, C * 480))
        a_tp, a_ig = arena.put(T(tp.view(np.int16)), "tp"), arena.put(T(ig.view(np.int16)), "ig")
        a_pos, a_seg, a_ngt = arena.put(T(pos), "pos"), arena.put(T(seg), "seg_off"), arena.put(T(w["n_gt"]), "n_gt")
        ap = arena.out((C, 4, 10), torch.float64, "ap")
        cnt = arena.out((C, 4, 3, 10), torch.int32, "tp_count")

        def call():
            status = L.ssd_eval_ap_coco(P(a_tp), P(a_ig), P(a_pos), P(a_seg), P(a_ngt), C, md, dp(M.RECALL_POINTS), P(ap), P(cnt),
                                        stream())
            assert status == 0, status

        arena.poison(False)
        call()
        torch.cuda.synchronize()
        got_ap, got_cnt = ap.cpu().numpy().copy(), cnt.cpu().numpy().copy()
        want_ap, want_cnt = M.coco_tables_from_rows(w["rows"], w["n_gt"], md)
        print("max AP difference", float(np.abs(got_ap - want_ap).max()), "true positives", int(want_cnt[:, :, 2].sum()))
        assert np.abs(got_ap - want_ap).max() <= 1e-12
        assert np.array_equal(got_cnt, want_cnt) and want_cnt[:, :, 2].sum() > 0 and want_ap.max() > 0
        assert (want_cnt[:, :, 0] <= want_cnt[:, :, 1]).all() and (want_cnt[:, :, 0] < want_cnt[:, :, 2]).any()
        arena.run(call, [(ap, T(got_ap)), (cnt, T(want_cnt))])


def test_entry_points_refuse_before_any_launch(L):
    from ssd_object_detection_amd import _lib
    d = ctypes.c_void_p(0x1000)                                       # never dereferenced on these paths
    thr, pts = dp(M.IOU_THRESHOLDS), dp(M.RECALL_POINTS)

    def match(B=2, A=61, md=100, score=d, ranges=dp(RANGES), tp=d):
        return L.ssd_eval_match_coco(score, d, d, d, B, A, d, d, d, None, None, ranges, thr, md, d, d, d, d, d, tp, d, d, d, None)

    assert match(B=0) == match(A=0) == match(md=0) == match(md=L.ssd_eval_max_dets() + 1) == _lib.SSD_ERR_VALUE
    assert match(score=None) == match(ranges=None) == match(tp=None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, d, d, d, d, 0, 100, pts, d, d, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, d, d, d, d, 4, 0, pts, d, d, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, None, d, d, d, 4, 100, pts, d, d, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, d, d, d, d, 4, 100, pts, d, None, None) == _lib.SSD_ERR_VALUE


# ------------------------------------------------------------------------------------------------------------ the model
def assert_same_summary(dev, host, tol=1e-12):
    assert set(dev) == set(host) and set(M.COCO_SUMMARY_KEYS) <= set(dev)
    for k in M.COCO_SUMMARY_KEYS:
        print(k, dev[k], host[k])
        if host[k] == -1.0 or dev[k] == -1.0:
            assert dev[k] == host[k], (k, dev[k], host[k])
        assert abs(dev[k] - host[k]) <= tol, (k, dev[k], host[k])
    assert set(dev["per_class"]) == set(host["per_class"])
    for c, v in host["per_class"].items():
        assert abs(dev["per_class"][c] - v) <= tol
    for name, table in host["per_class_area"].items():
        assert set(dev["per_class_area"][name]) == set(table)
        for c, v in table.items():
            assert abs(dev["per_class_area"][name][c] - v) <= tol


def hit_samples(samples, hdets, size, raw=False):
    """ground truth the detections hit: six of every image's own detections, the second and the fifth of them crowd regions"""
    out = []
    for smp, (s, c, b) in zip(samples, hdets):
        pick = np.arange(0, len(s), max(1, len(s) // 6))[:6]
        box = b[pick].astype(np.float64)
        if raw:                                                       # back to COCO top-left boxes in source pixels
            h, w = smp[0].shape[:2]
            box = box * np.array([w, h, w, h]) / size
            box[:, :2] -= box[:, 2:] / 2
        else:
            box = box / size
        crowd = np.zeros(len(pick), bool)
        crowd[[i for i in (1, 4) if i < len(pick)]] = True
        out.append((smp[0], c[pick].astype(np.float32), box.astype(np.float32), crowd))
    return out


def check_protocol(model, samples, size, batch_size, raw=False, **kw):
    from ssd_object_detection_amd.models.ssd_model import _RawList
    _, hdets = model.evaluate(samples, batch_size=batch_size, score_thresh=0.2, return_detections=True, **kw)
    assert min(len(d[0]) for d in hdets) >= 12
    hit = hit_samples(list(samples), hdets, size, raw)
    hit = _RawList(hit) if raw else hit
    host = model.evaluate(hit, batch_size=batch_size, score_thresh=0.2, protocol="coco", **kw)
    dev = model.evaluate(hit, batch_size=batch_size, score_thresh=0.2, protocol="coco", metric="device", **kw)
    assert host["AP50"] > 0.0 and host["AR100"] > 0.0
    assert_same_summary(dev, host)
    return host, hit


def test_evaluate_coco_device_equals_host_ssd300(tmp_path):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    from tests.test_eval_device_gpu import spread_model
    _, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=60).get_dataset()
    samples = list(val)
    model = spread_model(tmp_path)
    host, hit = check_protocol(model, samples, 300.0, 4)
    # crowd flags change the result: the same boxes as ordinary ground truth score differently
    plain = model.evaluate([h[:3] for h in hit], batch_size=4, score_thresh=0.2, protocol="coco")
    assert plain["mAP"] != host["mAP"] or plain["AR100"] != host["AR100"]
    # without crowd flags the first three are the default protocol's, on both sides
    default = model.evaluate([h[:3] for h in hit], batch_size=4, score_thresh=0.2, metric="device")
    dev_plain = model.evaluate([h[:3] for h in hit], batch_size=4, score_thresh=0.2, metric="device", protocol="coco")
    for k in ("mAP", "AP50", "AP75"):
        assert abs(default[k] - dev_plain[k]) <= 1e-12 and abs(default[k] - plain[k]) <= 1e-12
    check_protocol(model, samples, 300.0, 4, scoring="all")
    with pytest.raises(ValueError):
        model.evaluate(samples, protocol="pascal")
    with pytest.raises(ValueError):
        model.evaluate(samples, protocol="pascal", metric="device")


def test_evaluate_coco_reader_contract_two_source_sizes(tmp_path):
    """RawSplit samples of two source sizes: areas are in source pixels (area_scale = W H / S^2), both modes agree"""
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    from ssd_object_detection_amd.data_loaders.synthetic import synth_raw_sample
    from tests.test_eval_device_gpu import spread_model

    class Reader:
        def _gen(self, first, n):
            for i in range(first, first + n):
                img, cls, tlwh = synth_raw_sample(i)
                if i % 2:                                             # a second source size: half the rows
                    img = np.ascontiguousarray(img[:img.shape[0] // 2])
                    tlwh = tlwh.copy()
                    tlwh[:, 1] /= 2
                    tlwh[:, 3] /= 2
                box = tlwh.copy()
                box[:, :2] += box[:, 2:] / 2
                yield img, cls, box

        def get_dataset(self):
            return list(self._gen(0, 2)), list(self._gen(100, 5))

    _, val = SSDDataLoader("unused", dataset=Reader()).get_dataset()
    assert getattr(val, "raw", False)
    samples = list(val)
    assert len({s[0].shape[:2] for s in samples}) >= 2
    model = spread_model(tmp_path)
    host, hit = check_protocol(model, val, 300.0, 4, raw=True)
    # the scale matters: the same list scored as prepared-size areas differs in some area column
    crowd, scale = model._coco_batch_extras(hit, True)
    assert len(set(scale.tolist())) >= 2 and crowd is not None and crowd.sum() > 0


def test_evaluate_coco_resnet(tmp_path):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    from tests.test_resnet_model_gpu import IN, make_model, spread_biases
    _, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=40, input_size=IN).get_dataset()
    samples = list(val)
    model = make_model(tmp_path)
    spread_biases(model)
    assert IN == 256
    check_protocol(model, samples, float(IN), 2)
    check_protocol(model, samples, float(IN), 2, precision="mxfp8")


def test_coco_batch_loop_never_synchronises(tmp_path):
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    from ssd_object_detection_amd.utils.device_map import DeviceCocoAccumulator
    from tests.test_eval_device_gpu import spread_model
    _, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=60).get_dataset()
    samples = list(val)
    model = spread_model(tmp_path)
    host, hit = check_protocol(model, samples, 300.0, 4)               # builds caches (allocations sync)
    acc = DeviceCocoAccumulator(80, 100, model.device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                            # any torch-side host sync now raises
    try:
        model.evaluate_into(acc, hit, batch_size=4, score_thresh=0.2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert_same_summary(acc.result(), host)
    assert len(acc.detections()) == len(hit)


def test_coco_validation_inside_a_training_run(tmp_path, monkeypatch):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    from ssd_object_detection_amd.tools import train as T_
    from ssd_object_detection_amd.utils.scalar_log import TAGS, read_scalars
    from tests.test_eval_device_gpu import spread_biases

    real_init = SSDObjectDetectionModel.__init__

    def init(self, *a, **k):
        real_init(self, *a, **k)
        spread_biases(self)

    monkeypatch.setattr(SSDObjectDetectionModel, "__init__", init)

    def cfg_for(sub, protocol):
        cfg = T_.load_config(os.path.join(os.path.dirname(T_.__file__), "..", "config", "default.yml"))
        cfg["data"]["mini_batch"]["num_data"] = 40
        cfg["data"]["shuffle"] = False
        cfg["model"]["log_dir"] = str(tmp_path / sub)
        cfg["model"]["train"]["batch_size"] = 4
        cfg["model"]["train"]["epoch"] = 2
        cfg["model"]["train"]["lr"]["initial"] = 1e-5
        cfg["model"]["split_train"]["enable"] = False
        cfg["model"]["warmup"]["enable"] = False
        cfg["model"]["log_interval"] = 100
        cfg["model"]["eval"] = dict(enable=True, every=1, batch_size=4, score_thresh=0.2, num_data=3)
        if protocol:
            cfg["model"]["eval"]["protocol"] = protocol
        return cfg

    assert T_.val_from_config(cfg_for("x", "coco"))["protocol"] == "coco" and "protocol" not in T_.val_from_config(cfg_for("x", None))
    with pytest.raises(ValueError):
        T_.val_from_config(cfg_for("x", "pascal"))
    coco = T_.train(cfg_for("coco", "coco"))
    default = T_.train(cfg_for("default", None))
    got = read_scalars(os.path.join(coco.get_log_dir(), "scalars.jsonl"))
    plain = read_scalars(os.path.join(default.get_log_dir(), "scalars.jsonl"))
    train_tags = {"train/" + t for t in TAGS}
    assert set(plain) == train_tags | {"val/mAP", "val/AP50", "val/AP75"}
    assert set(got) == train_tags | {"val/" + k for k in M.COCO_SUMMARY_KEYS} and len(M.COCO_SUMMARY_KEYS) == 12
    tags = [l.split('"tag": "')[1].split('"')[0] for l in open(os.path.join(coco.get_log_dir(), "scalars.jsonl"))]
    assert tags[-12:] == ["val/" + k for k in M.COCO_SUMMARY_KEYS] and tags[-12:-9] == ["val/mAP", "val/AP50", "val/AP75"]
    for k in ("val/mAP", "val/AP50", "val/AP75"):                       # the synthetic split has no crowd box
        assert len(got[k]) == 2 and got[k] == plain[k], (k, got[k], plain[k])
    for k in M.COCO_SUMMARY_KEYS:
        assert [s for s, _ in got["val/" + k]] == [10, 20]
