"""CPU: the PASCAL VOC metric on the host (utils.metrics.voc_map, voc_match_image, voc_ap_from_rows).

voc_map is build-defined: a numpy restatement of the published VOCdevkit procedure (VOCevaldet), unpinned -- the devkit is not
available to run.  It is checked against hand-computed values and against tests/voc_cases.devkit, a second restatement of the
same published procedure that shares no code with it.

Bounds: 1e-15 for the hand-computed APs (a handful of correctly rounded quotients and at most eleven additions), 1e-12 for the
per-class APs against the second restatement (the same operations in the same order: the observed difference is 0), equality
for flags and counts."""
import numpy as np
import pytest

from tests import voc_cases as V

M = V.M


@pytest.mark.parametrize("case", V.HAND, ids=[c["name"] for c in V.HAND])
def test_hand_cases(case):
    want = case["want"]
    ref = V.match_reference(case)
    for i, (flags, gt) in enumerate(zip(want["flags"], want["gt"])):
        assert ref["n_det"][i] == len(flags)
        assert ref["flags"][i, :len(flags)].tolist() == flags and ref["gt"][i, :len(gt)].tolist() == gt
    for year, key in (("07", "ap07"), ("12", "ap12")):
        r = M.voc_map(case["dets"], case["gts"], year, case["iou_thresh"], case["max_dets"])
        assert set(r) == {"mAP", "per_class", "n_pos"} and r["n_pos"] == want["n_pos"]
        assert set(r["per_class"]) == set(want[key])
        for c, v in want[key].items():
            print(case["name"], year, c, r["per_class"][c], v)
            assert abs(r["per_class"][c] - v) <= 1e-15
        assert abs(r["mAP"] - np.mean(list(want[key].values()))) <= 1e-15
        other = V.devkit(case["dets"], case["gts"], year, case["iou_thresh"], case["max_dets"])
        assert other[1] == want["n_pos"] and [f.tolist() for f in other[2]] == want["flags"]


def test_hand_example_values():
    case = V.HAND[0]
    assert case["name"] == "hand"
    assert abs(M.voc_map(case["dets"], case["gts"], "07")["mAP"] - 28.0 / 33.0) <= 1e-15
    assert abs(M.voc_map(case["dets"], case["gts"], "12")["mAP"] - 5.0 / 6.0) <= 1e-15


def test_duplicate_is_where_voc_and_coco_differ():
    case = next(c for c in V.HAND if c["name"] == "duplicate")
    _, _, _, tp, ign, gt = M.voc_match_image(*case["dets"][0], *case["gts"][0])
    assert tp.tolist() == [True, False] and not ign.any() and gt.tolist() == [0, 0]
    # both boxes pass for the second detection too: the greedy rule hands it the unclaimed one
    iou = M.iou_matrix(case["dets"][0][2], case["gts"][0][1])
    assert (iou >= 0.5).all() and (iou.argmax(1) == 0).all()
    coco = M.coco_map(case["dets"], [g[:2] for g in case["gts"]])
    assert coco["AP50"] == 1.0
    assert M.voc_map(case["dets"], case["gts"], "12")["mAP"] == 0.5


def test_first_index_not_last():
    case = next(c for c in V.HAND if c["name"] == "first_index_tie")
    gt = M.voc_match_image(*case["dets"][0], *case["gts"][0])[5]
    assert gt.tolist() == [0, 0]                                      # coco_match_image would take index 1, then index 0
    r = M.coco_match_image(*case["dets"][0], *case["gts"][0][:2])
    assert (r[3][:, 0] & 1).tolist() == [1, 1]


def test_threshold_is_inclusive_and_validated():
    case = next(c for c in V.HAND if c["name"] == "at_threshold")
    assert M.iou_matrix(case["dets"][0][2], case["gts"][0][1])[0, 0] == 0.5
    assert M.voc_map(case["dets"], case["gts"], "07", iou_thresh=0.5)["mAP"] == 1.0
    assert M.voc_map(case["dets"], case["gts"], "07", iou_thresh=np.nextafter(0.5, 1.0))["mAP"] == 0.0
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            M.voc_map(case["dets"], case["gts"], "07", iou_thresh=bad)
    for bad in ("2007", 2012, "10", None):
        with pytest.raises(ValueError):
            M.voc_map(case["dets"], case["gts"], bad)
        with pytest.raises(ValueError):
            M.voc_ap_from_rows((np.zeros(1), np.zeros(1), np.zeros(1)), {0: 1}, bad)


def test_recall_points_are_exact_tenths():
    assert M.VOC_RECALL_POINTS.tolist() == [k / 10.0 for k in range(11)] and M.VOC_RECALL_POINTS[3] == 0.3
    assert np.linspace(0, 1, 11)[3] != 0.3                            # the quirk of the widely copied port
    for n_pos in (10, 20, 30, 70, 1990):                              # a recall that is k/10 as a rational reaches point k
        for k in range(11):
            assert (k * n_pos // 10) / float(n_pos) >= M.VOC_RECALL_POINTS[k]
    # three true positives of ten: recall 0.3 counts for the points 0, 0.1, 0.2 and 0.3
    rows = (np.zeros(3, int), np.array([0.9, 0.8, 0.7]), np.ones(3, np.uint8))
    assert abs(M.voc_ap_from_rows(rows, {0: 10}, "07")[0] - 4.0 / 11.0) <= 1e-15


def test_ap_from_rows_edges():
    none = (np.zeros(0, int), np.zeros(0), np.zeros(0, np.uint8))
    assert M.voc_ap_from_rows(none, {0: 3, 1: 0}, "07") == {0: 0.0} and M.voc_ap_from_rows(none, {}, "12") == {}
    rows = (np.zeros(4, int), np.array([0.9, 0.8, 0.7, 0.6]), np.array([2, 2, 3, 2], np.uint8))
    for year in ("07", "12", 7, 12):                                  # every row ignored (bit 1 wins over bit 0)
        assert M.voc_ap_from_rows(rows, {0: 2}, year) == {0: 0.0}
    rows = (np.zeros(3, int), np.array([0.9, 0.8, 0.7]), np.array([2, 1, 0], np.uint8))
    assert M.voc_ap_from_rows(rows, np.array([1]), "12") == {0: 1.0}  # the ignored row in front costs no precision
    assert M.voc_map([], [], "07") == dict(mAP=0.0, per_class={}, n_pos={})


def test_max_dets_cut_keeps_the_best():
    case = next(c for c in V.HAND if c["name"] == "max_dets_cut")
    s = M.voc_match_image(*case["dets"][0], *case["gts"][0], max_dets=2)[0]
    assert s.tolist() == [np.float32(0.9), np.float32(0.8)]
    assert M.voc_map(case["dets"], case["gts"], "12", max_dets=100)["mAP"] > M.voc_map(case["dets"], case["gts"], "12",
                                                                                     max_dets=2)["mAP"]


@pytest.mark.parametrize("year", ["07", "12"])
def test_random_images_against_the_second_restatement(year):
    case = V.random_set()
    assert len(case["dets"]) == 200
    got = M.voc_map(case["dets"], case["gts"], year, case["iou_thresh"], case["max_dets"])
    per_class, n_pos, flags = V.devkit(case["dets"], case["gts"], year, case["iou_thresh"], case["max_dets"])
    assert got["n_pos"] == n_pos and set(got["per_class"]) == set(per_class) and len(per_class) == 5
    worst = max(abs(got["per_class"][c] - per_class[c]) for c in per_class)
    print("mAP", got["mAP"], "largest per-class difference", worst)
    assert worst <= 1e-12 and 0.05 < got["mAP"] < 0.95
    ref = V.match_reference(case)
    kinds = np.zeros(3, int)
    for i, f in enumerate(flags):
        assert ref["n_det"][i] == len(f) and np.array_equal(ref["flags"][i, :len(f)], f)
        kinds += np.bincount(f, minlength=3)[:3]
    assert (kinds >= 100).all(), kinds                                # false positives, true positives, ignored
    # duplicates and the cut occur
    dup = sum(int(((ref["gt"][i] >= 0) & (ref["flags"][i] == 0)).sum()) for i in range(len(flags)))
    assert dup >= 20 and max(len(d[0]) for d in case["dets"]) > case["max_dets"]
