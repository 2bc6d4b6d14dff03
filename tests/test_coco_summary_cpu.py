"""CPU: utils.metrics.coco_summary, the definition of COCO's twelve box metrics (area ranges, crowd boxes, average recall) and
the oracle of ssd_eval_match_coco / ssd_eval_ap_coco: tied to coco_map where no box is crowd, hand-worked cases with known
answers, and the census of the generated case sets the GPU tests run on."""
import numpy as np
import pytest

from tests import coco_eval_cases as CC
from tests import eval_cases as E

M = E.M
F32 = np.float32


def det(*rows):
    """rows of (score, cls, cx, cy, w, h)"""
    a = np.asarray(rows, np.float64).reshape(-1, 6)
    return a[:, 0].astype(F32), a[:, 1].astype(np.int32), a[:, 2:].astype(F32)


def gt(*rows, crowd=None):
    """rows of (cls, cx, cy, w, h)"""
    a = np.asarray(rows, np.float64).reshape(-1, 5)
    g = (a[:, 0].astype(np.int32), a[:, 1:].copy())
    return g if crowd is None else g + (np.asarray(crowd, bool),)


@pytest.mark.parametrize("name", sorted(E.REGIMES))
def test_without_crowd_equals_coco_map_exactly(name):
    dets, gts, _ = E.regime(name)
    want = M.coco_map(dets, gts, 100)
    got = M.coco_summary(dets, gts, 100)
    assert want["mAP"] > 0 or name == "sparse"
    for k in ("mAP", "AP50", "AP75"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["per_class"] == want["per_class"]
    assert got["per_class_area"]["all"] == want["per_class"]
    assert set(M.COCO_SUMMARY_KEYS) <= set(got)
    with_flags = M.coco_summary(dets, [g + (np.zeros(len(g[0]), bool),) for g in gts], 100)
    assert with_flags == got


def test_crowd_box_claimed_by_three_detections():
    """one ordinary box and one crowd region of class 0; one detection on the box, three inside the crowd region: the three
    are ignored (not false positives), so AP = 1 and recall = 1 with n_gt = 1"""
    g = gt((0, 50, 50, 40, 40), (0, 200, 200, 150, 150), crowd=[False, True])
    d = det((0.9, 0, 50, 50, 40, 40), (0.8, 0, 180, 180, 40, 40), (0.7, 0, 220, 220, 40, 40), (0.6, 0, 200, 200, 40, 40))
    census = {}
    _, _, _, tp, ig, pos, gi = M.coco_match_image(*d, g[0], g[1], g[2], census=census)
    assert tp[:, 0].tolist() == [0x3ff] * 4 and ig[:, 0].tolist() == [0, 0x3ff, 0x3ff, 0x3ff]
    assert pos.tolist() == [0, 1, 2, 3] and gi.tolist() == [0b1010, 0b1111]      # 40x40 = 1600: medium only; crowd: everywhere
    assert census["crowd_rematch"] == 2 * 10 * 4
    r = M.coco_summary([d], [g])
    assert r["mAP"] == r["AP50"] == r["AP75"] == 1.0 and r["AR1"] == r["AR100"] == 1.0
    without = M.coco_summary([d], [g[:2]])                    # the same boxes as ordinary ground truth: two false positives
    assert without["mAP"] < 1.0


def test_valid_box_is_preferred_over_a_better_ignored_one():
    """range medium: the detection overlaps a large (ignored) box with IoU 1 and a medium one with IoU 0.64; it takes the
    medium one and is a true positive there, not an ignored row"""
    g = gt((0, 100, 100, 100, 100), (0, 100, 100, 80, 80))
    d = det((0.9, 0, 100, 100, 100, 100))
    _, _, _, tp, ig, _, gi = M.coco_match_image(*d, g[0], g[1])
    assert gi.tolist() == [0b0110, 0b1010]                    # 10000: large; 6400: medium
    # matched to the valid box up to 0.60; above, no valid box is left and the ignored one (IoU 1) takes it: ignored there
    assert tp[0, 2] == 0x3ff and ig[0, 2] == 0b1111111000
    assert tp[0, 3] == 0x3ff and ig[0, 3] == 0                # range large: the 100x100 box is valid, IoU 1
    assert tp[0, 0] == 0x3ff and ig[0, 0] == 0                # all: both valid, the higher IoU wins


def test_unmatched_detection_outside_the_range_is_dropped():
    """a small false positive lowers AP in 'all' and 'small', and leaves 'medium' alone"""
    g = gt((0, 100, 100, 50, 50))
    d = det((0.9, 0, 250, 250, 10, 10), (0.8, 0, 100, 100, 50, 50))
    r = M.coco_summary([d], [g])
    assert abs(r["mAP"] - 0.5) < 1e-12 and r["AP_medium"] == 1.0 and r["AP_small"] == -1.0 and r["AP_large"] == -1.0
    _, _, _, tp, ig, _, _ = M.coco_match_image(*d, g[0], g[1])
    assert ig[0].tolist() == [0, 0, 0x3ff, 0x3ff] and tp[0].tolist() == [0, 0, 0, 0]


def test_boundary_box_belongs_to_both_ranges():
    g = gt((0, 100, 100, 32, 32))
    d = det((0.9, 0, 100, 100, 32, 32))
    census = {}
    gi = M.coco_match_image(*d, g[0], g[1], census=census)[6]
    assert gi.tolist() == [0b1000] and census["boundary_area"] == 2
    r = M.coco_summary([d], [g])
    assert r["AP_small"] == 1.0 and r["AP_medium"] == 1.0 and r["AP_large"] == -1.0
    assert r["AR_small"] == 1.0 and r["AR_medium"] == 1.0 and r["AR_large"] == -1.0
    scaled = M.coco_summary([d], [g], area_scale=np.array([4.0]))             # 4096 source pixels: medium only
    assert scaled["AP_small"] == -1.0 and scaled["AP_medium"] == 1.0


def test_large_class_is_left_out_of_ap_small():
    g = gt((0, 100, 100, 20, 20), (1, 150, 150, 120, 120))
    d = det((0.9, 0, 100, 100, 20, 20), (0.8, 1, 150, 150, 120, 120))
    r = M.coco_summary([d], [g])
    assert set(r["per_class_area"]["small"]) == {0} and set(r["per_class_area"]["large"]) == {1}
    assert r["AP_small"] == 1.0 and r["AP_large"] == 1.0 and r["AP_medium"] == -1.0 and r["AR_medium"] == -1.0
    only_large = M.coco_summary([(d[0][1:], d[1][1:], d[2][1:])], [gt((1, 150, 150, 120, 120))])
    assert only_large["AP_small"] == -1.0 and only_large["AR_small"] == -1.0 and only_large["mAP"] == 1.0


def test_average_recall_grows_with_the_detection_limit():
    """three objects of one class, thirteen detections: hits at positions 0, 5 and 12, misses between them: AR1 = 1/3,
    AR10 = 2/3, AR100 = 1"""
    g = gt((0, 50, 50, 40, 40), (0, 150, 150, 40, 40), (0, 250, 250, 40, 40))
    rows = [(0.99, 0, 50, 50, 40, 40)]
    rows += [(0.9 - 0.01 * i, 0, 20 + 5 * i, 280, 10, 10) for i in range(4)]
    rows += [(0.8, 0, 150, 150, 40, 40)]
    rows += [(0.7 - 0.01 * i, 0, 280, 20 + 5 * i, 10, 10) for i in range(6)]
    rows += [(0.5, 0, 250, 250, 40, 40)]
    r = M.coco_summary([det(*rows)], [g])
    assert abs(r["AR1"] - 1 / 3) < 1e-12 and abs(r["AR10"] - 2 / 3) < 1e-12 and r["AR100"] == 1.0
    assert r["AR1"] < r["AR10"] < r["AR100"]


@pytest.mark.parametrize("name", sorted(CC.SETS))
def test_generated_case_sets_exercise_every_event(name):
    """the sets the GPU tests run on: every event of the protocol at least five times in each (seeds fixed so that it holds)"""
    total = dict.fromkeys(CC.EVENTS, 0)
    for index in range(len(CC.case_set(name))):
        for k, v in CC.match_reference(name, index)["census"].items():
            total[k] += v
    print(name, total)
    CC.assert_census(total)
    cases = CC.case_set(name)
    assert {c["A"] for c in cases} == {61, 256, 2000} and {c["max_dets"] for c in cases} == {1, 7, 100, 128}
    assert max(len(d[0]) for c in cases for d in c["dets"]) > 1024
    assert all(3 <= c["B"] <= 8 and 3 <= c["n_cls"] <= 6 for c in cases)


def test_a_case_set_that_exercises_nothing_fails_the_census():
    """the census is a count on the oracle's own arrays: plain boxes of one size, far apart, produce none of the events"""
    census = dict.fromkeys(CC.EVENTS, 0)
    g = gt((0, 60, 60, 50, 50), (1, 200, 200, 50, 50))
    d = det((0.9, 0, 60, 60, 50, 50), (0.8, 1, 200, 200, 50, 50))
    M.coco_match_image(*d, g[0], g[1], census=census)
    assert census["crowd_rematch"] == census["iou_tie"] == census["boundary_area"] == census["unmatched_out_of_range"] == 0
    with pytest.raises(AssertionError):
        CC.assert_census(census)


def test_host_second_stage_equals_the_summary():
    """coco_tables_from_rows + coco_summary_from_tables (what the device metric restates) on a generated batch = coco_summary"""
    case = CC.case_set("a")[2]
    ref = CC.match_reference("a", 2)
    C = case["n_cls"] + 2
    ap, cnt = M.coco_tables_from_rows(CC.rows_of(ref), CC.n_gt_of(case, ref, C), case["max_dets"])
    got = M.coco_summary_from_tables(ap, cnt, CC.n_gt_of(case, ref, C))
    want = M.coco_summary(case["dets"], case["gts"], case["max_dets"], area_scale=case["scale"])
    assert got == want
    assert want["AP_small"] >= 0 and want["AP_medium"] >= 0 and want["AP_large"] >= 0


def test_entry_points_refuse_on_the_host():
    """ssd_eval_match_coco / ssd_eval_ap_coco return SSD_ERR_VALUE before any launch on the conditions of the existing pair:
    callable without a GPU"""
    import ctypes

    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    d = ctypes.c_void_p(0x1000)                                       # never dereferenced on these paths
    dp = ctypes.POINTER(ctypes.c_double)
    thr, pts = M.IOU_THRESHOLDS.ctypes.data_as(dp), M.RECALL_POINTS.ctypes.data_as(dp)
    ranges = np.ascontiguousarray(np.asarray(M.COCO_AREA_RANGES, np.float64).reshape(-1))

    def match(B=2, A=61, md=100, score=d, rng=ranges.ctypes.data_as(dp), tp=d, n_det=d):
        return L.ssd_eval_match_coco(score, d, d, d, B, A, d, d, d, None, None, rng, thr, md, n_det, d, d, d, d, tp, d, d, d, None)

    for status in (match(B=0), match(A=0), match(md=0), match(md=L.ssd_eval_max_dets() + 1), match(score=None), match(rng=None),
                   match(tp=None), match(n_det=None)):
        assert status == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, d, d, d, d, 0, 100, pts, d, d, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, d, d, d, d, 4, 0, pts, d, d, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, d, d, d, d, 4, L.ssd_eval_max_dets() + 1, pts, d, d, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, None, d, d, d, 4, 100, pts, d, d, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, d, d, d, d, 4, 100, None, d, d, None) == _lib.SSD_ERR_VALUE
    assert L.ssd_eval_ap_coco(d, d, d, d, d, 4, 100, pts, d, None, None) == _lib.SSD_ERR_VALUE
