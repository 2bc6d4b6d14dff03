"""CPU: the cases of tests/detect_cases.py -- everything tests/test_detect_strict_gpu.py relies on that can be shown without a
GPU.
  * Regime.  Logits and offsets are exact in bf16, priors are multiples of 1/8, the float64 decode fits float32; NMS boxes have
    integer corners; what a case is named after (totals around max_cand, a tie group across the cut in three strides, segments
    of exactly 63 / 64 / 65 / 1024, ground-truth and kept counts) holds for its inputs.
  * Agreement.  The score reference stated from the design equals oracle.ssd_oracle.score within the project's tolerance, and
    class and candidate flag wherever score and p_background are further than 1e-6 from the threshold; every hand-written keep
    set equals oracle.ssd_oracle.nms.
  * Border.  Every random-logit case leaves out at most 0.1 % of its rows, by the float64 reference alone.
  * Power.  Wrong references built from the same inputs differ from the right one: `>=` for `>` in the IoU test (segments of at
    most 64 and of more), the upper lane winning an argmax tie, the maximum not subtracted."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import ssd_oracle as O                                   # noqa: E402
from tests import detect_cases as D                                  # noqa: E402

ALL_C = D.GENERIC_C + (81,) + D.LDS_C + (D.LDS_REFUSED_C,)


# ------------------------------------------------------------------------------------------------------------------ scores
@pytest.mark.parametrize("C", ALL_C)
def test_score_patterns_cover_what_the_issue_lists(C):
    pats = D.score_patterns(C)
    nfg, bg, sp = C - 1, C - 1, D.lane_split(C)
    tops = [t for t, _ in pats]
    for n in (1, 2, 3, 4, 8):
        if n <= nfg:
            assert any(len(t) == n and bg not in t for t in tops), n
        if n - 1 <= nfg:
            assert any(len(t) == n and bg in t for t in tops), n
    for k in {0, nfg - 1, sp - 1, sp} & set(range(nfg)):
        assert (k,) in tops and (k, bg) in tops, k
    if sp < nfg:                                             # a top in either lane's range: the lower index is the class
        both = [t for t in tops if min(t) < sp <= max(k for k in t if k < bg)]
        assert len(both) >= 2 and (sp - 1, sp) in tops
    assert (bg,) in tops
    assert {t for _, t in pats} <= {0.0, 80.0, 96.0} and (len(pats) < 3 or {t for _, t in pats} == {0.0, 80.0, 96.0})
    _, score, cls, p_bg = D.pattern_reference(C)
    i = tops.index((bg,))
    assert score[i] == 0 and cls[i] == 0 and p_bg[i] == 1


@pytest.mark.parametrize("C", ALL_C)
def test_score_design_is_exact(C):
    B, A = D.SCORE_SHAPES[-1]
    for in_size in D.IN_SIZES:
        c = D.score_case(C, B, A, in_size)
        assert np.array_equal(D.through(c["conf"], "bf16"), c["conf"]) and np.array_equal(D.through(c["loc"], "bf16"), c["loc"])
        assert np.array_equal(c["priors"] * 8, np.round(c["priors"] * 8)) and len(np.unique(c["priors"], axis=0)) == A
        assert np.array_equal(c["loc"][..., :2] * 4, np.round(c["loc"][..., :2] * 4)) and not c["loc"][..., 2:].any()
        d = c["priors"][None]
        xy = (c["loc"][..., :2].astype(np.float64) * d[..., 2:] + d[..., :2]) * in_size
        wh = d[..., 2:] * in_size * np.ones_like(xy)
        box64 = np.concatenate([xy, wh], -1)
        assert np.array_equal(c["box"].astype(np.float64), box64)          # the float64 decode fits float32
        assert len(np.unique(c["box"].reshape(-1, 4), axis=0)) > B * A // 2
    # exp(-200) is 0 and exp(0) is 1 in float32: the sum of a row is its number of tops
    assert np.exp(np.float32(-D.LOW)) == 0 and np.exp(np.float32(0)) == 1
    big = D.score_case(81, *D.BIG_SHAPE)
    assert big["B"] * big["A"] == 768 * 128 + 129 and big["conf"].nbytes < 33 << 20


@pytest.mark.parametrize("C", ALL_C)
def test_score_reference_agrees_with_the_oracle(C):
    B, A = D.SCORE_SHAPES[-1]
    c = D.score_case(C, B, A)
    p = np.exp(O._log_softmax(c["conf"]))
    np.testing.assert_allclose(c["prob"], p[..., :-1], rtol=2e-6, atol=1e-9)
    at_threshold = 0
    for thresh in D.THRESHOLDS:
        s_ref, c_ref, cand_ref = O.score(c["conf"], thresh)
        np.testing.assert_allclose(c["score"], s_ref, rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(c["p_bg"], p[..., -1], rtol=2e-6, atol=1e-9)
        clear = (np.abs(s_ref - thresh) > D.BORDER) & (np.abs(p[..., -1] - thresh) > D.BORDER)
        cand = D.candidates(c, thresh)
        assert np.array_equal(cand[clear], cand_ref[clear]) and np.array_equal(c["cls"][clear], c_ref[clear])
        assert np.array_equal(c["cls"], c_ref)               # the lowest top is numpy's argmax too
        at = c["score"] == np.float32(thresh)
        at_threshold += int(at.sum())
        assert not cand[at].any()                            # `>` is strict
        assert not cand[(c["p_bg"] > np.float32(thresh))].any()
        below = c["score"] == np.float32(np.nextafter(np.float32(thresh), np.float32(1)))
        if below.any():                                      # the same rows one float32 above the threshold: candidates without
            assert cand[below & (c["p_bg"] == 0)].all() and not cand[below & (c["p_bg"] > 0)].any()   # the background
    if C >= 3:
        assert at_threshold > 0
    if C >= 9:
        for n in (2, 4, 8):                                  # score == p_background == threshold, and score alone
            rows = c["score"] == np.float32(1.0 / n)
            assert (rows & (c["p_bg"] == c["score"])).any() and (rows & (c["p_bg"] == 0)).any()


@pytest.mark.parametrize("C", [c for c in ALL_C if c >= 3])
def test_score_design_sees_a_wrong_tie_rule_and_a_missing_maximum(C):
    B, A = D.SCORE_SHAPES[-1]
    c = D.score_case(C, B, A)
    conf, sp = c["conf"], D.lane_split(C)
    fg = conf[..., :-1]
    lower, upper = fg[..., :sp], fg[..., sp:]
    if upper.shape[-1]:
        # wrong: on equal maxima of the two lanes the upper lane's index is taken
        lo_i, up_i = lower.argmax(-1), upper.argmax(-1) + sp
        wrong = np.where(upper.max(-1) >= lower.max(-1), up_i, lo_i)
        assert not np.array_equal(wrong, c["cls"])
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(conf.astype(np.float32))                  # wrong: the row's maximum is not subtracted
        s = (e[..., :-1].max(-1) / e.sum(-1)).astype(np.float32)
    assert not np.isfinite(s).all()


@pytest.mark.parametrize("C", D.GENERIC_C)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_random_cases_leave_out_at_most_a_thousandth(C, dt):
    c = D.random_case(C, dt)
    rows = c["border"].size
    assert rows == 3 * 190 and c["border"].sum() <= 0.001 * rows
    assert c["cand"].sum() > 10 and (~c["cand"]).sum() > 10
    assert np.array_equal(D.through(c["conf"], dt), c["conf"]) and np.array_equal(D.through(c["loc"], dt), c["loc"])
    assert c["loc"][..., 2:].any()                           # the exp branch of the decode


# --------------------------------------------------------------------------------------------------------------------- NMS
def nms_ge(score_, cls_, box_, cand_, iou_thresh, max_cand):
    """wrong: oracle.ssd_oracle.nms with `>=` for `>`"""
    idx = np.nonzero(cand_)[0]
    order = idx[np.lexsort((idx, -score_[idx].astype(np.float64)))][:max_cand]
    keep, kept = np.zeros(len(score_), bool), []
    for i in order:
        same = [j for j in kept if cls_[j] == cls_[i]]
        if same and (O.iou_f32_rows(box_[i], box_[same]) >= np.float32(iou_thresh)).any():
            continue
        kept.append(i)
        keep[i] = True
    return keep


@pytest.mark.parametrize("name", D.NMS_NAMES)
def test_nms_case_regime(name):
    case = D.nms_case(name)
    A = case["A"]
    for variant in (0, 1):
        score, cls, box, cand = D.nms_inputs(case, variant)
        assert score.dtype == np.float32 and cls.dtype == np.int32 and box.dtype == np.float32 and cand.dtype == np.uint8
        assert score.shape == (case["B"], A) and box.shape == (case["B"], A, 4)
        on = cand != 0
        b = box[on].astype(np.float64)
        corners = np.concatenate([b[:, :2] - b[:, 2:] / 2, b[:, :2] + b[:, 2:] / 2], 1)
        assert np.array_equal(corners, np.round(corners)) and (b[:, 2:] >= 0).all()         # the integer pixel grid
        assert np.isfinite(score[on]).all() and (score[on] > 0).all() and (cls[on] >= 0).all() and (cls[on] < 65536).all()
        assert set(np.unique(cand)) <= {0, *D.CAND_BYTES}
        for b_, img in enumerate(case["images"]):
            assert int(on[b_].sum()) == len(img["anchors"]) == len(np.unique(img["anchors"]))
            assert (img["anchors"] >= 0).all() and (img["anchors"] < A).all()
    (score, cls, _, cand), other = D.nms_inputs(case, 0), D.nms_inputs(case, 1)
    off = cand == 0
    if off.any():                                            # the two fills differ in every non-candidate row
        assert not (np.nan_to_num(score[off]) == other[0][off]).any() and not np.array_equal(cls[off], other[1][off])
    assert max(len(i["anchors"]) for i in case["images"]) <= 1100          # the oracle's Python loop stays quick


@pytest.mark.parametrize("name", [n for n in D.NMS_NAMES if "hand" in D.nms_case(n)])
def test_hand_keep_sets_equal_the_oracle(name):
    case = D.nms_case(name)
    keep, count = D.nms_want(name, D.NMS_CAP)
    assert np.array_equal(keep, D.hand_keep(case)), (name, np.nonzero(keep[0])[0], case["hand"]["keep"])
    assert count[0] == len(case["hand"]["keep"])


def test_hand_cases_cover_what_the_issue_lists():
    names = {h["name"] for h in D.HAND}
    assert len(names) == len(D.HAND) and all(len(h["rows"]) <= 16 for h in D.HAND)
    assert {h["iou"] for h in D.HAND} >= {0.0, 0.5, 1.0, float(D.pred32(0.5))}
    nested = D.HAND[[h["name"] for h in D.HAND].index("nested-at-the-threshold")]
    iou = O.iou_f32_rows(np.array(nested["rows"][0][2], np.float32), np.array([nested["rows"][1][2]], np.float32))
    assert iou[0] == np.float32(0.5) and iou.dtype == np.float32
    zero = np.array([[5, 5, 0, 0]], np.float32)
    assert O.iou_f32_rows(zero[0], zero)[0] == 0
    assert len({D.nms_case("embedded-%d" % i)["images"][0]["anchors"][0] for i in range(len(D.HAND))}) > len(D.HAND) // 2


def test_nms_sizes_counts_cuts_segments_are_what_they_are_named():
    used = set()
    for A in D.NMS_SIZES:
        case = D.nms_case("size-%d" % A)
        n = [len(i["anchors"]) for i in case["images"]]
        assert case["B"] == 3 and n[0] == 0 and n[1] == 1 and n[2] == min(A, 300), (A, n)
        used |= set(np.unique(case["images"][2]["bytes"]).tolist())
        if A == 65536:
            assert set(range(65532, 65536)) <= set(case["images"][2]["anchors"].tolist())
    assert used == set(D.CAND_BYTES)
    assert {a % 4 for a in D.NMS_SIZES} >= {0, 1, 3} and 24564 // 4 > 3 * 1024 and 24564 // 4 % (3 * 1024) != 0
    for mc in D.COUNT_MAX_CANDS:
        case = D.nms_case("count-%d" % mc)
        assert [len(i["anchors"]) for i in case["images"]] == case["totals"] and case["totals"][:3] == [mc - 1, mc, mc + 1]
        if mc == D.NMS_CAP:
            assert case["totals"][3:] == [1025, case["A"]]
        img = case["images"][2]                              # mc + 1 candidates: the cut falls inside a tie (mc > 1)
        s = np.sort(img["score"])[::-1]
        assert mc == 1 or s[mc - 1] == s[mc]
    for name in D.CUT_NAMES:
        case = D.nms_case(name)
        img = case["images"][0]
        order = np.lexsort((img["anchors"], -img["score"].astype(np.float64)))
        cut = img["score"][order[D.CUT_MAX_CAND - 1]]
        tie = img["anchors"][img["score"] == cut]
        taken = img["anchors"][order[:D.CUT_MAX_CAND]]
        inside, outside = np.intersect1d(tie, taken), np.setdiff1d(tie, taken)
        assert len(inside) and len(outside)                  # the tie group straddles the cut
        if name != "cut-low-byte":
            assert len(set((tie // 1024).tolist())) >= 3 and len(set((inside // 1024).tolist())) >= 3
        bits = img["score"].view(np.uint32)
        if name == "cut-zero-digits":
            assert set(bits.tolist()) == {0x3F000000, 0x3F800000, 0x3F400000}
        if name == "cut-low-byte":
            assert len(set((bits >> 8).tolist())) == 1 and len(set(bits.tolist())) > 100
    for n in (63, 64, 65, 1024):
        img = D.nms_case("seg-%d" % n)["images"][0]
        assert len(img["anchors"]) == n and len(set(img["cls"].tolist())) == 1
        assert (np.diff(img["anchors"]) > 0).all()
    img = D.nms_case("seg-80-classes")["images"][0]
    assert len(set(img["cls"].tolist())) == 80 and np.bincount(img["cls"]).min() >= 2
    assert len(D.nms_case("seg-65-chain")["images"][0]["anchors"]) == 65


@pytest.mark.parametrize("name", ["hand-6", "hand-13", "seg-63", "seg-64", "seg-65", "seg-1024"])
def test_nms_cases_see_a_greater_or_equal(name):
    """an IoU exactly at the threshold, in a hand case, in segments that fit a wave and in longer ones"""
    case = D.nms_case(name)
    score, cls, box, cand = D.nms_inputs(case, 0)
    right = D.nms_want(name, D.NMS_CAP)[0][0].astype(bool)
    wrong = nms_ge(score[0], cls[0], box[0], cand[0], case["iou"], D.NMS_CAP)
    assert not np.array_equal(wrong, right)
    assert 0 < right.sum() and (name.startswith("hand") or right.sum() < cand[0].astype(bool).sum())      # something is suppressed


def test_nms_suppression_happens_in_the_generated_cases():
    for name in D.NMS_NAMES:
        if name.startswith(("size-", "count-", "cut-", "seg-")):
            case = D.nms_case(name)
            for mc in case["max_cands"]:
                keep, count = D.nms_want(name, mc)
                for b, img in enumerate(case["images"]):
                    assert count[b] <= min(mc, len(img["anchors"]))
                    assert (count[b] > 0) == (len(img["anchors"]) > 0)
            n = len(case["images"][-1]["anchors"])
            if n > 12:
                assert D.nms_want(name, D.NMS_CAP)[1][-1] < n, name


# -------------------------------------------------------------------------------------------------------------- eval-match
@pytest.mark.parametrize("A", D.EVAL_ANCHORS)
@pytest.mark.parametrize("md", D.EVAL_MAX_DETS)
def test_eval_case_counts(A, md):
    c = D.eval_case(A, md)
    assert c["B"] == 5 and [len(g[0]) for g in c["gts"]] == [0, 1, 48, 49, 6]
    kept = [len(a) for a in c["anchors"]]
    assert kept == [min(k, A) for k in (1, 0, md, md + 1, 1024 + (md % 2 == 0))]
    assert [int((c["keep"][i] != 0).sum()) for i in range(5)] == kept
    assert A % 4 and all(c["keep"][i, A - 1] != 0 for i in range(5) if kept[i])   # the tail a four-byte sweep would not reach
    n_det, d_score, d_cls, d_box, d_flags = c["want"]
    assert n_det.tolist() == [min(k, md) for k in kept]
    for i in range(5):
        assert (d_score[i, n_det[i]:] == 0).all() and (d_cls[i, n_det[i]:] == -1).all() and not d_box[i, n_det[i]:].any()
        assert not d_flags[i, n_det[i]:].any()
    gcls, gbox = c["gts"][4]
    assert gcls[0] == gcls[1] and np.array_equal(gbox[0], gbox[1])                # identical ground truths ...
    assert d_flags[4, 0] == 0x3FF and d_cls[4, 0] == gcls[0]                      # ... and a detection exactly on them
    s = c["dets"][4][0]
    if len(s) > D.EVAL_CAP:                                                       # the radix cut falls inside a tie
        top = np.sort(s)[::-1]
        assert md == 1 or top[md - 1] == top[md]
    assert sum(int(np.count_nonzero(f)) for f in d_flags) >= min(md, 2)


def test_eval_cases_reach_both_readers_and_the_radix_cut():
    assert {a % 4 for a in D.EVAL_ANCHORS} == {1, 2, 3}
    kept = {len(a) for md in D.EVAL_MAX_DETS for a in D.eval_case(4097, md)["anchors"]}
    assert {0, 1, 1024, 1025, 128, 129} <= kept
