"""CPU: the conditions the strict anchor-side cases (tests/anchor_cases.py) rest on -- asserted on the inputs and on the
oracles' values, never on what a kernel returned."""
import numpy as np
import pytest

from oracle import ssd_oracle as O
from tests import anchor_cases as AC
from tests import eval_cases as E


def test_geometries_have_the_stated_anchor_counts():
    for name, A in AC.ANCHORS.items():
        P = AC.priors(name)
        assert P.shape == (A, 4) and P.dtype == np.float64, name
        assert (P[:, 2] * P[:, 3] >= 1e-3).all(), name                 # what ssd_prior_grid_verify asks of a verified grid
    assert AC.ANCHORS == {"G4": 4, "G190": 190, "G790": 790, "G380": 380}
    assert 190 % 4 == 2 and 790 % 4 == 2 and 790 == 3 * 256 + 22 and 380 % 4 == 0 and 380 // 4 < 1024


def test_matcher_batches():
    counts = {k: [len(i["gt_box"]) for i in AC.match_batch(*k)] for k in AC.MATCH_BATCHES}
    assert counts[("G4", "main")] == [4, 1, 0] and counts[("G190", "main")] == [0, 1, 7, 64]
    assert counts[("G790", "main")] == [512, 513, 600, 3] and max(counts[("G790", "small")]) == 64
    seven = AC.match_batch("G190")[2]["gt_box"]
    assert np.array_equal(seven[3], seven[1]) and (seven[5, 2:] == 0).all()
    full = AC.match_batch("G4")[0]
    assert full["mask"].all()                                           # n_t == A: every column is taken in phase 1
    for key in AC.MATCH_BATCHES:
        for img in AC.match_batch(*key):
            assert img["mask"].sum() >= len(img["gt_box"])              # every box owns an anchor
            assert np.isfinite(img["enc"]).all()


def test_literal_equals_closed_form_on_the_large_images():
    P = AC.priors("G790")
    for which in ("main", "small"):
        for img in AC.match_batch("G790", which):
            if len(img["gt_box"]) == 0:
                continue
            c, b, m = O.match_closed_form(img["gt_cls"], img["gt_box"], P, 0.5)
            assert np.array_equal(m, img["mask"]) and np.array_equal(c, img["cls"])
            assert np.array_equal(b.view(np.uint32), img["box"].view(np.uint32))


@pytest.mark.parametrize("A", [190, 790])
@pytest.mark.parametrize("C,dt", AC.SCORE_CASES)
def test_score_cases(A, C, dt):
    case = AC.score_case(A, C, dt)
    conf = case["conf"]
    flat = conf.reshape(-1, C)
    if dt == "bf16":
        assert np.array_equal(AC.bf16_round(conf), conf) and np.array_equal(AC.bf16_round(case["loc"]), case["loc"])
    # every tie row really has two bit-equal maxima at the stated indices, and the oracle names the lower one
    pairs = AC.tie_pairs(C)
    assert len(case["ties"]) == 4 * len(pairs)
    h = (C - 1 + 1) // 2
    if C >= 6:
        assert any(hi < h for lo, hi in pairs) and any(lo < h <= hi for lo, hi in pairs) and any(lo >= h for lo, hi in pairs)
        assert (h - 1, h) in pairs and (0, h) in pairs
    if C == 81:
        assert {(3, 50), (0, 40), (39, 40), (50, 79)} <= set(pairs)
    if C == 3:
        assert pairs == [(0, 1)]
    if C == 2:
        assert pairs == []
    rows = [r for r, _, _ in case["ties"]]
    assert len(set(rows)) == len(rows)
    for row, lo, hi in case["ties"]:
        z = flat[row, :-1]
        assert z[lo].view(np.uint32) == z[hi].view(np.uint32) and z[lo] == z.max()
        assert np.nonzero(z == z.max())[0].tolist() == [lo, hi]
        assert case["cls_oracle"].reshape(-1)[row] == lo and case["cand"].reshape(-1)[row]
    assert np.array_equal(case["cls"], case["cls_oracle"])              # the exact argmax of the logits is the oracle's class
    # the candidate set away from the border: at most 0.1 % of the rows lie within 1e-6 of the threshold
    assert case["border"].mean() <= 1e-3
    assert case["cand"].sum() > 10 and (~case["cand"]).sum() > 10


@pytest.mark.parametrize("A", [190, 790])
@pytest.mark.parametrize("C,dt", AC.SCORE_CASES)
def test_threshold_cases(A, C, dt):
    case = AC.threshold_case(A, C, dt)
    conf = case["conf"]
    assert np.array_equal(AC.bf16_round(conf), conf)                    # exact in bf16 as well
    best, bg = conf[..., :-1].max(-1), conf[..., -1]
    tie = case["tie"]
    assert np.array_equal(bg[tie].view(np.uint32), best[tie].view(np.uint32))
    assert np.array_equal(bg[~tie], best[~tie] - np.float32(30.0))
    assert np.array_equal((best - np.float32(30.0)).astype(np.float64), best.astype(np.float64) - 30.0)     # no rounding
    assert tie.sum() > 20 and (~tie).sum() > 20
    flat = conf.reshape(-1, C)
    assert not tie.reshape(-1)[case["src"]] and not tie.reshape(-1)[case["dups"]].any()
    assert len(set(case["dups"].tolist()) | {case["src"]}) == 4
    for d in case["dups"]:
        assert np.array_equal(flat[d], flat[case["src"]])


@pytest.mark.parametrize("A", AC.NMS_ANCHORS)
def test_nms_cases(A):
    case = AC.nms_case(A)
    assert case["B"] in (2, 3) and case["cand"][1].sum() == 0
    order, s = AC.nms_order(case, 0)
    total = len(order)
    assert min(A, 1500) <= total <= min(A, 1502) and np.isfinite(s).all() and (s > 0).all()
    if A >= 3:
        assert order[0] == 0 and order[1] == A - 1 and s[0] == s[1]      # the tied top pair, the lower anchor first
        assert case["cls"][0, 0] == case["cls"][0, A - 1]
        assert O.iou_f32_rows(case["box"][0, 0], case["box"][0, A - 1:A])[0] > AC.NMS_IOU
        assert 0 < case["cand"][2].sum() <= 9
    for mc in AC.NMS_MAX_CAND:
        if total > mc:                                                  # ties on both sides of the cut
            assert s[mc - 1] == s[mc], (A, mc)
        keep, count = case["want"][mc]
        assert keep[0].sum() == count[0] <= min(total, mc) and count[1] == 0
        assert not keep[~case["cand"].astype(bool)].any()
    if A >= 190:
        part = order[:1024]
        seg = np.bincount(case["cls"][0][part])
        assert seg.max() > 64 and (seg[seg > 0] <= 64).sum() >= 3        # a segment longer than a wave beside short ones
        keep = case["want"][1024][0][0].astype(bool)
        assert 0 < keep.sum() < len(part)                               # something is suppressed
    if A >= 4099:
        assert total > 1024                                             # total > 1024 >= max_cand
    if A == 65536:
        assert case["cand"][0, 0] and case["cand"][0, 65535]
        assert case["want"][1024][0][0, 0] == 1 and case["want"][1024][0][0, 65535] == 0


@pytest.mark.parametrize("A", AC.EVAL_ANCHORS)
def test_eval_cases(A):
    case = AC.eval_case(A)
    counts = np.diff(case["gt_off"])
    assert counts.max() > 48 and 0 < counts.min() <= 48 and counts.max() <= 62
    kept = case["keep"].sum(1)
    assert kept[1] == 0 and kept.max() <= A
    if A == 4099:
        assert kept.max() > 1024
        s = np.sort(case["score"][0][case["keep"][0] > 0])[::-1]
        assert all(s[md - 1] == s[md] for md in (100, 128))             # the cut falls inside ties
    if A == 190:
        assert kept.max() > 128
    # the planted pair: equal IoUs, the last index wins -- the second detection misses 0.5 .. 0.6 and matches from 0.65 on
    iou = E.M.iou_matrix(np.asarray(AC.PLANT_DET, np.float32), np.asarray(AC.PLANT_GT, np.float64))
    assert iou[0, 0] == iou[0, 1] >= 0.6 and iou[1, 1] == 1.0 and iou[1, 0] < 0.5
    n_det, d_score, d_cls, d_box, d_flags = case["want"][128]
    rows = [int(np.nonzero((d_box[0] == np.asarray(b, np.float32)).all(1) & (d_cls[0] == AC.PLANT_CLS))[0][0]) for b in AC.PLANT_DET]
    assert rows[0] < rows[1] < n_det[0]
    assert d_flags[0, rows[0]] & 0b11 == 0b11 and d_flags[0, rows[1]] & 0b11 == 0 and d_flags[0, rows[1]] >> 9 == 1
    for md in AC.EVAL_MAX_DETS:
        n_det = case["want"][md][0]
        assert n_det.tolist() == np.minimum(kept, md).tolist()
    assert sum(int(np.count_nonzero(case["want"][128][4][i])) for i in range(case["B"])) > (2 if A == 3 else 20)   # true positives


def test_ap_case():
    case = AC.ap_case()
    seg, n_gt = case["seg_off"], case["n_gt"]
    sizes = np.diff(seg)
    assert sizes[0] > 2 * 256 and sizes[1] == 0 and n_gt[1] > 0 and sizes[2] > 0 and n_gt[2] == 0
    assert set(case["table"]) == set(np.nonzero(n_gt)[0].tolist())
    assert (case["ap"][1] == 0).all() and (case["ap"][2] == 0).all() and case["ap"][0].min() > 0
