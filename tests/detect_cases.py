"""Cases and exact references for the single-label detection path -- ssd_score_decode, ssd_nms, ssd_eval_match (and the dense
ssd_class_scores where it shares the LDS bound) -- shared by test_detect_cases_cpu.py and test_detect_strict_gpu.py.  Plain
Python: importable without a GPU.  Deterministic (seeded); every builder is cached, treat what it returns as read-only.

Scores.  A logit row holds two values only, t at its `tops` and t - 200 elsewhere, t = 0, 80 or 96: all exact in bf16, and
exp(96) overflows float32 where the row's maximum is not subtracted (exp(80) = 5.5e34 does not yet).  With n tops: exp(0) = 1,
exp(-200) is 0 in float32, the sum is n and every top's probability is the float32 quotient 1/n.  The reference is stated
from that, not through the float64 oracle (whose exp(log_softmax) round trip gives 0.12500000000000003 for eight tops): score = 1/n, or 0 where no foreground class is a top; class = the lowest foreground top, or 0; p_background = 1/n
where the background is a top, else 0; candidate = score > thresh and not p_background > thresh, in float32.
Boxes.  Offsets are multiples of 1/4 with t_w = t_h = 0, priors multiples of 1/8 that differ from anchor to anchor: the float64
decode is exact and fits float32, so boxes are compared bit for bit.
NMS.  score / cls / box / cand are built directly, boxes on an integer pixel grid.  The reference is oracle.ssd_oracle.nms; the
HAND cases also state their keep set, so that kernel and oracle cannot be wrong together.
Eval-match.  Images with a stated number of ground truths and of kept anchors (tests.eval_cases.gen draws both at random, so
its recipe is restated here with the counts pinned); the reference is tests.eval_cases.match_reference."""
import functools

import numpy as np
import torch

from oracle import ssd_oracle as O
from tests import eval_cases as E

F32 = np.float32
LOW = 200.0                                                   # a top's logit minus every other logit


def pred32(x):
    """the float32 neighbour just below x"""
    return F32(np.nextafter(F32(x), F32(0)))


# 0.5, 0.25, 0.125 and the float32 just below each: a row of 2, 4, 8 tops scores exactly the threshold / just above it
THRESHOLDS = tuple(float(v) for t in (0.5, 0.25, 0.125) for v in (F32(t), pred32(t)))
IN_SIZES = (300.0, 512.0)
GENERIC_C = (2, 3, 6, 82)                                     # k_score_decode<T, 0>; 82: an odd foreground count next to 81
SCORE_SHAPES = ((1, 1), (1, 127), (1, 128), (1, 129), (3, 190))      # (B, A): whole and partial 128-row blocks
BIG_SHAPE = (3, 32811)                                        # 768 * 128 + 129 rows: a second, prefetched block; a partial last one
LDS_SHAPE = (2, 130)
LDS_C = (129, 300)                                            # 66 048 and 153 600 bytes of dynamic LDS
LDS_REFUSED_C = 301


def lane_split(C):
    """the first foreground class of the second lane of a row: (C - 1 + 1) / 2"""
    return (C - 1 + 1) // 2


@functools.lru_cache(maxsize=None)
def score_patterns(C):
    """[(tops, t)]: the sets of tied top classes (background = C - 1) a row can hold, and the row's top logit"""
    nfg, bg, sp = C - 1, C - 1, lane_split(C)
    pats = []

    def add(tops):
        tops = tuple(sorted(set(tops)))
        if tops not in pats:
            pats.append(tops)

    for k in (0, sp - 1, sp, nfg - 1):                       # index 0, either side of the lane split, the last foreground class
        if 0 <= k < nfg:
            add([k])
            add([k, bg])
    if sp < nfg:                                             # both lanes hold a top: the lower index must win
        for pair in ((sp - 1, sp), (0, nfg - 1), (0, sp), (sp - 1, nfg - 1)):
            add(pair)
            add(pair + (bg,))
    for n in (2, 3, 4, 8):
        for with_bg in (0, 1):
            k = n - with_bg
            if 1 <= k <= nfg:
                low = [(j * nfg) // k for j in range(k)]     # spread over the row, from class 0
                high = [nfg - 1 - v for v in low]            # ... and up to the last foreground class
                add(low + [bg] * with_bg)
                add(high + [bg] * with_bg)
    add([bg])                                                # every foreground class low: score 0, class 0
    return tuple((tops, (0.0, 96.0, 80.0)[i % 3]) for i, tops in enumerate(pats))


def pattern_reference(C):
    """per pattern: n, score f32, class, p_background f32 -- stated from the design"""
    pats = score_patterns(C)
    n = np.array([len(t) for t, _ in pats])
    fg = [[k for k in t if k < C - 1] for t, _ in pats]
    has_fg = np.array([len(f) > 0 for f in fg])
    has_bg = np.array([C - 1 in t for t, _ in pats])
    inv = F32(1) / n.astype(F32)
    score = np.where(has_fg, inv, F32(0)).astype(F32)
    cls = np.array([min(f) if f else 0 for f in fg], np.int32)
    p_bg = np.where(has_bg, inv, F32(0)).astype(F32)
    return n, score, cls, p_bg


def dyadic_priors(A):
    """float64 [A, 4] (cx, cy, w, h): multiples of 1/8, no two anchors below 65536 alike"""
    a = np.arange(A)
    return np.stack([(a % 16 + 1) / 8, (a // 16 % 16 + 1) / 8, ((a * 5 + a // 256) % 16 + 1) / 8,
                     ((a * 3 + a // 4096) % 16 + 1) / 8], 1).astype(np.float64)


def dyadic_loc(n):
    """float32 [n, 4]: t_x, t_y multiples of 1/4 in -1/2 .. 1/2, t_w = t_h = 0"""
    g = np.arange(n)
    loc = np.zeros((n, 4), F32)
    loc[:, 0] = (g % 5 - 2) / 4
    loc[:, 1] = (g // 5 % 5 - 2) / 4
    return loc


@functools.lru_cache(maxsize=None)
def score_case(C, B, A, in_size=300.0):
    """The exact design at (B, A, C): conf f32 [B,A,C], loc f32 [B,A,4], priors f64 [A,4], the per-row pattern index, and the
    references score f32, cls i32, p_bg f32, box f32 (of every row: a non-candidate's is 0 in the kernel's output)."""
    pats = score_patterns(C)
    n = B * A
    idx = (np.arange(n) + 5) % len(pats)
    block = np.empty((len(pats), C), F32)
    for i, (tops, t) in enumerate(pats):
        block[i] = t - LOW
        block[i, list(tops)] = t
    _, p_score, p_cls, p_bg = pattern_reference(C)
    loc, pri = dyadic_loc(n).reshape(B, A, 4), dyadic_priors(A)
    return dict(B=B, A=A, C=C, in_size=in_size, idx=idx, conf=block[idx].reshape(B, A, C), loc=loc, priors=pri,
                score=p_score[idx].reshape(B, A), cls=p_cls[idx].reshape(B, A), p_bg=p_bg[idx].reshape(B, A),
                box=O.decode(loc, pri[None], in_size), prob=class_scores_reference(C)[idx].reshape(B, A, C - 1))


@functools.lru_cache(maxsize=None)
def class_scores_reference(C):
    """per pattern: ssd_class_scores' dense row, 1/n at the foreground tops and 0 elsewhere"""
    pats = score_patterns(C)
    out = np.zeros((len(pats), C - 1), F32)
    for i, (tops, _) in enumerate(pats):
        out[i, [k for k in tops if k < C - 1]] = F32(1) / F32(len(tops))
    return out


def candidates(case, thresh):
    """the candidate flags of the design at a threshold: the two float32 comparisons"""
    t = F32(thresh)
    return (case["score"] > t) & ~(case["p_bg"] > t)


def boxes_of(case, cand):
    return np.where(cand[..., None], case["box"], F32(0)).astype(F32)


def through(a, dt):
    """float32 values after a round trip through the input type"""
    return a if dt == "f32" else torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


RANDOM_SHAPE = (3, 190)
RANDOM_THRESH = 0.3
BORDER = 1e-6
RANDOM_SEED = {2: 11, 3: 12, 6: 13, 82: 14}


@functools.lru_cache(maxsize=None)
def random_case(C, dt):
    """Random logits (background-dominated, boosted entries) and random offsets at B = 3, A = 190, as the input type holds them,
    with the float64 oracle's score / class / candidate / box and the rows within 1e-6 of the threshold (`border`)."""
    B, A = RANDOM_SHAPE
    rng = np.random.default_rng(RANDOM_SEED[C])
    conf = rng.normal(0, 1, (B, A, C)).astype(F32)
    conf[..., C - 1] += 2.0
    hot = rng.random((B, A)) < 0.3
    k = rng.integers(0, C - 1, (B, A))
    boost = rng.uniform(2, 8, (B, A)).astype(F32)
    np.put_along_axis(conf, k[..., None], np.take_along_axis(conf, k[..., None], -1) + (boost * hot)[..., None], -1)
    loc = rng.normal(0, 0.2, (B, A, 4)).astype(F32)
    conf, loc = through(conf, dt), through(loc, dt)
    pri = O.priors()[:A]
    score, cls, cand = O.score(conf, RANDOM_THRESH)
    p_bg = np.exp(O._log_softmax(conf))[..., -1]
    border = (np.abs(score - RANDOM_THRESH) < BORDER) | (np.abs(p_bg - RANDOM_THRESH) < BORDER)
    return dict(B=B, A=A, C=C, conf=conf, loc=loc, priors=pri, score=score, cls=cls, cand=cand, border=border,
                box=O.decode(loc, pri[None], 300))


# ---------------------------------------------------------------------------------------------------------------------- NMS
CAND_BYTES = (1, 2, 0x80, 0xFF)
NMS_CAP = 1024


def box_xyxy(x0, y0, x1, y1):
    return ((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0)


_SQ = box_xyxy(20, 20, 30, 30)
_CHAIN = (box_xyxy(0, 0, 10, 10), box_xyxy(4, 0, 14, 10), box_xyxy(8, 0, 18, 10))     # IoU 3/7 between neighbours, 1/9 end to end
# rows: (score, class, box) in anchor order; keep: the rows that survive, written out by hand
HAND = (
    dict(name="chain", iou=0.4, rows=[(0.9, 3, _CHAIN[0]), (0.8, 3, _CHAIN[1]), (0.7, 3, _CHAIN[2])], keep=[0, 2]),
    dict(name="chain-from-the-last-anchor", iou=0.4, rows=[(0.7, 3, _CHAIN[0]), (0.8, 3, _CHAIN[1]), (0.9, 3, _CHAIN[2])],
         keep=[0, 2]),
    dict(name="no-chain-above-the-overlap", iou=0.45, rows=[(0.9, 3, _CHAIN[0]), (0.8, 3, _CHAIN[1]), (0.7, 3, _CHAIN[2])],
         keep=[0, 1, 2]),
    dict(name="identical", iou=0.45, rows=[(0.9, 1, _SQ), (0.8, 1, _SQ)], keep=[0]),
    dict(name="identical-zero-area", iou=0.45, rows=[(0.9, 1, (5, 5, 0, 0)), (0.8, 1, (5, 5, 0, 0))], keep=[0, 1]),
    dict(name="identical-zero-width", iou=0.0, rows=[(0.9, 1, (5, 5, 0, 10)), (0.8, 1, (5, 5, 0, 10))], keep=[0, 1]),
    # outer 10 x 10, inner 10 x 5 inside it: 50 / (100 + 50 - 50 + 1e-10) is 0.5 exactly in float32
    dict(name="nested-at-the-threshold", iou=0.5, rows=[(0.9, 2, (5, 5, 10, 10)), (0.8, 2, (5, 2.5, 10, 5))], keep=[0, 1]),
    dict(name="nested-above-the-threshold", iou=float(pred32(0.5)), rows=[(0.9, 2, (5, 5, 10, 10)), (0.8, 2, (5, 2.5, 10, 5))],
         keep=[0]),
    dict(name="touching", iou=0.0, rows=[(0.9, 0, box_xyxy(0, 0, 10, 10)), (0.8, 0, box_xyxy(10, 0, 20, 10)),
                                         (0.7, 0, box_xyxy(0, 10, 10, 20)), (0.6, 0, box_xyxy(10, 10, 20, 20))], keep=[0, 1, 2, 3]),
    dict(name="two-classes", iou=0.45, rows=[(0.9, 4, _SQ), (0.8, 5, _SQ), (0.7, 4, _SQ)], keep=[0, 1]),
    dict(name="equal-scores", iou=0.45, rows=[(0.75, 1, _SQ), (0.75, 1, _SQ), (0.75, 1, _SQ)], keep=[0]),
    dict(name="equal-scores-behind-a-better-one", iou=0.45, rows=[(0.5, 1, _SQ), (0.5, 1, _SQ), (1.0, 1, _SQ)], keep=[2]),
    # one pixel of overlap is suppressed at 0; the box that merely touches the first survives (its only overlap is with a
    # suppressed box)
    dict(name="iou-zero", iou=0.0, rows=[(0.9, 0, box_xyxy(0, 0, 10, 10)), (0.8, 0, box_xyxy(9, 9, 19, 19)),
                                         (0.7, 0, box_xyxy(10, 10, 20, 20))], keep=[0, 2]),
    dict(name="iou-one", iou=1.0, rows=[(0.9, 0, _SQ), (0.8, 0, _SQ), (0.7, 0, (25, 22.5, 10, 5))], keep=[0, 1, 2]),
)
HAND_BIG_A = 2051                                             # the larger row a hand case is embedded in (odd: the byte-wise sweep)


def _image(anchors, score, cls, box, rng):
    anchors = np.asarray(anchors, np.int64)
    return dict(anchors=anchors, score=np.asarray(score, F32), cls=np.asarray(cls, np.int32),
                box=np.asarray(box, F32).reshape(len(anchors), 4), bytes=rng.choice(CAND_BYTES, len(anchors)).astype(np.uint8))


def random_image(rng, A, n, n_cls, scores=None, anchors=None):
    """n candidates: classes below n_cls, integer boxes in clusters of about six (so that suppression happens)"""
    if anchors is None:
        anchors = np.sort(rng.choice(A, n, replace=False))
    cl = rng.integers(0, max(1, n // 6), n)
    box = np.stack([40 * (cl % 8) + rng.integers(0, 10, n), 40 * (cl // 8) + rng.integers(0, 10, n), 2 * rng.integers(5, 15, n),
                    2 * rng.integers(5, 15, n)], 1)                      # even sides: integer corners
    if scores is None:
        scores = rng.uniform(0.05, 1.0, n)
    return _image(anchors, scores, rng.integers(0, n_cls, n), box, rng)


def hand_image(h, rng, anchors=None):
    rows = h["rows"]
    return _image(np.arange(len(rows)) if anchors is None else anchors, [r[0] for r in rows], [r[1] for r in rows],
                  [r[2] for r in rows], rng)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _empty(rng):
    return _image([], [], [], np.zeros((0, 4)), rng)


def _case(name, A, images, iou, max_cands, **more):
    return dict(name=name, A=A, B=len(images), images=images, iou=float(iou), max_cands=tuple(max_cands), **more)


NMS_SIZES = (1, 3, 190, 1023, 1025, 4097, 12292, 24564, 65536)
COUNT_MAX_CANDS = (1, 64, 400, 1024)
COUNT_A = 1099
CUT_A, CUT_TOTAL, CUT_MAX_CAND = 4097, 600, 400
SEG_A = 1100
CUT_NAMES = ("cut-all-equal", "cut-zero-digits", "cut-low-byte")
SEG_NAMES = ("seg-63", "seg-64", "seg-65", "seg-1024", "seg-80-classes", "seg-65-chain")


def _exact_pair(rng, cls):
    """two more rows for a segment: a nested pair whose IoU is exactly 0.5, away from every cluster"""
    return [(0.3, cls, (1000, 1000, 10, 10)), (0.2, cls, (1000, 997.5, 10, 5))]


@functools.lru_cache(maxsize=None)
def nms_case(name):
    kind, _, arg = name.partition("-")
    if kind == "hand":                                       # hand-<i>: the case alone, A = its rows
        h = HAND[int(arg)]
        return _case(name, len(h["rows"]), [hand_image(h, _rng(1, int(arg)))], h["iou"], (NMS_CAP, len(h["rows"])), hand=h)
    if kind == "embedded":                                   # the same rows at random anchors of a larger image
        h, rng = HAND[int(arg)], _rng(2, int(arg))
        anchors = np.sort(rng.choice(HAND_BIG_A, len(h["rows"]), replace=False))
        return _case(name, HAND_BIG_A, [hand_image(h, rng, anchors)], h["iou"], (NMS_CAP,), hand=h)
    if kind == "size":                                       # image 0: no candidate, image 1: one, image 2: the case
        A = int(arg)
        rng = _rng(3, A)
        n = min(A, 300)
        anchors = np.sort(rng.choice(A, n, replace=False))
        if A > n:
            anchors[0], anchors[-1] = 0, A - 1               # the first and the last anchor of the row
        if A == 65536:
            anchors[-4:] = np.arange(65532, 65536)           # anchors that need all 16 bits of the key
        anchors = np.unique(anchors)
        main = random_image(rng, A, len(anchors), 5, anchors=anchors)
        one = random_image(rng, A, 1, 5, anchors=np.array([A - 1]))
        return _case(name, A, [_empty(rng), one, main], 0.45, (NMS_CAP, 100))
    if kind == "count":                                      # totals around max_cand, quantised scores: the cut falls in a tie
        mc = int(arg)
        rng = _rng(4, mc)
        totals = [mc - 1, mc, mc + 1] + ([1025, COUNT_A] if mc == NMS_CAP else [])
        images = [random_image(rng, COUNT_A, t, 3, scores=rng.integers(1, 16, t) / 16) if t else _empty(rng) for t in totals]
        return _case(name, COUNT_A, images, 0.45, (mc,), totals=totals)
    if name in CUT_NAMES:
        rng = _rng(5, CUT_NAMES.index(name))
        if name == "cut-all-equal":
            scores = np.full(CUT_TOTAL, 0.75, F32)
        elif name == "cut-zero-digits":                      # 0x3F000000, 0x3F800000, 0x3F400000: three radix digits are 0
            scores = rng.choice(np.array([0.5, 1.0, 0.75], F32), CUT_TOTAL)
        else:                                                # bits that differ in the lowest byte only
            scores = (np.uint32(0x3F400000) | rng.integers(0, 256, CUT_TOTAL).astype(np.uint32)).view(F32)
        return _case(name, CUT_A, [random_image(rng, CUT_A, CUT_TOTAL, 4, scores=scores)], 0.45, (CUT_MAX_CAND, 1, NMS_CAP - 1))
    if name == "seg-80-classes":                             # more segments than the workgroup has waves
        rng = _rng(6, 80)
        img = random_image(rng, SEG_A, 400, 1)
        img["cls"] = (np.arange(400) % 80).astype(np.int32)
        return _case(name, SEG_A, [img], 0.45, (NMS_CAP,))
    if name == "seg-65-chain":
        # box 0 suppresses 1 .. 63 (each shifted by one more pixel: IoU >= 37/163 > 0.2); box 64 overlaps box 0 by 17/183 only
        # and box 63 by 2/3: it survives because box 63 did not
        rng = _rng(6, 65)
        rows = [(1.0 - i / 128, 7, (100 + i, 100, 100, 100)) for i in range(64)] + [(0.25, 7, (183, 100, 100, 100))]
        h = dict(rows=rows, keep=[0, 64], iou=0.2)
        anchors = np.sort(rng.choice(SEG_A, 65, replace=False))
        return _case(name, SEG_A, [hand_image(h, rng, anchors)], 0.2, (NMS_CAP,), hand=h)
    if kind == "seg":                                        # one class with exactly n candidates
        n = int(arg)
        rng = _rng(6, n)
        img = random_image(rng, SEG_A, n - 2, 1)
        extra = _exact_pair(rng, 0)
        free = np.setdiff1d(np.arange(SEG_A), img["anchors"])[-2:]
        img = _image(np.concatenate([img["anchors"], free]), np.concatenate([img["score"], [e[0] for e in extra]]),
                     np.concatenate([img["cls"], [e[1] for e in extra]]), np.concatenate([img["box"], [e[2] for e in extra]]), rng)
        order = np.argsort(img["anchors"])
        img = {k: v[order] for k, v in img.items()}
        return _case(name, SEG_A, [img], 0.5, (NMS_CAP,))
    raise KeyError(name)


NMS_NAMES = tuple(["hand-%d" % i for i in range(len(HAND))] + ["embedded-%d" % i for i in range(len(HAND))] +
                  ["size-%d" % a for a in NMS_SIZES] + ["count-%d" % m for m in COUNT_MAX_CANDS] + list(CUT_NAMES) + list(SEG_NAMES))


def nms_inputs(case, variant):
    """score f32 [B,A], cls i32 [B,A], box f32 [B,A,4], cand u8 [B,A].  The rows of non-candidates hold junk that must never
    reach the result -- variant 0: NaN / huge scores and boxes, negative and >= 2^16 classes; variant 1: plausible values, a
    score above every candidate's, a class in use and a box on top of the clusters."""
    B, A = case["B"], case["A"]
    a = np.arange(A)
    if variant == 0:
        score = np.where(a % 2 == 0, F32(np.nan), F32(3e38)).astype(F32)
        cls = np.where(a % 2 == 0, -7, 70000 + a % 5).astype(np.int32)
        box = np.where((a % 3 == 0)[:, None], F32(np.nan), F32(1e30)).astype(F32) * np.ones((1, 4), F32)
    else:
        score = np.full(A, 2.0, F32)
        cls = (a % 3).astype(np.int32)
        box = np.tile(np.array([25, 25, 60, 60], F32), (A, 1))
    score, cls, box = np.tile(score, (B, 1)), np.tile(cls, (B, 1)), np.tile(box, (B, 1, 1))
    cand = np.zeros((B, A), np.uint8)
    for b, img in enumerate(case["images"]):
        an = img["anchors"]
        score[b, an], cls[b, an], box[b, an], cand[b, an] = img["score"], img["cls"], img["box"], img["bytes"]
    return score, cls, box, cand


@functools.lru_cache(maxsize=None)
def nms_want(name, max_cand, iou=None):
    """(keep u8 [B,A], keep_count i32 [B]) by oracle.ssd_oracle.nms on the inputs of variant 0"""
    case = nms_case(name)
    score, cls, box, cand = nms_inputs(case, 0)
    keep = np.stack([O.nms(score[b], cls[b], box[b], cand[b], case["iou"] if iou is None else iou, max_cand)
                     for b in range(case["B"])])
    return keep.astype(np.uint8), keep.sum(1).astype(np.int32)


def hand_keep(case):
    """the keep row of a hand case from its hand-written keep list"""
    keep = np.zeros((1, case["A"]), np.uint8)
    keep[0, case["images"][0]["anchors"][case["hand"]["keep"]]] = 1
    return keep


# ---------------------------------------------------------------------------------------------------------------- eval-match
EVAL_ANCHORS = (190, 1023, 4097)
EVAL_MAX_DETS = (1, 100, 127, 128)
EVAL_QUANT = 20
EVAL_GL = 48                                                  # ground truths per image the kernel caches in LDS
EVAL_CAP = 1024                                               # kept anchors it sorts without the radix cut


def eval_image(rng, n_gt, k, A, dup_gt, size=300.0):
    """tests.eval_cases.gen's recipe for one image with n_gt ground truths and k kept anchors (quantised scores); dup_gt: ground
    truths 0 and 1 are identical and detections 0 and 1 sit exactly on them (the last index must be claimed first)"""
    gcls = rng.integers(0, E.N_CLS, n_gt)
    gbox = np.concatenate([rng.uniform(0.15, 0.85, (n_gt, 2)), rng.uniform(0.05, 0.3, (n_gt, 2))], 1)
    if dup_gt:
        gbox[1], gcls[1] = gbox[0], gcls[0]
    anc = np.sort(rng.choice(A, k, replace=False))
    if k:
        anc[-1] = A - 1                                      # the last anchor of the row is kept: a four-byte sweep of an odd row
    score = (np.round(rng.uniform(0.05, 1.0, k) * EVAL_QUANT) / EVAL_QUANT).astype(F32)      # that stops at A & ~3 misses it
    cls = rng.integers(0, E.N_CLS + 2, k).astype(np.int32)
    box = np.concatenate([rng.uniform(30, 270, (k, 2)), rng.uniform(10, 90, (k, 2))], 1).astype(F32)
    if n_gt:
        on = rng.random(k) < 0.7
        g = rng.integers(0, n_gt, k)
        jitter = rng.normal(0, 6.0, (k, 4)) * (rng.random((k, 1)) < 0.8)
        box = np.where(on[:, None], (gbox[g] * size + jitter).astype(F32), box)
        cls = np.where(on & (rng.random(k) < 0.8), gcls[g], cls).astype(np.int32)
    box[:, 2:] = np.abs(box[:, 2:]) + 1
    if dup_gt and k >= 2:
        box[:2], cls[:2] = (gbox[0] * size).astype(F32), gcls[0]
        score[:2] = 1.0
    return (score, cls, box), (gcls.astype(np.int32), gbox.astype(np.float64) * size), anc


def eval_counts(A, md):
    """(ground truths, kept anchors, identical ground truths) of the five images: ground truths 0, 1, 48 (the LDS-cached limit),
    49; kept 0, 1, max_dets, max_dets + 1, and 1024 or 1025 (the sort's limit and the radix cut), as far as A holds them"""
    big = EVAL_CAP + (md % 2 == 0)
    return [(0, 1, False), (1, 0, False), (EVAL_GL, min(md, A), False), (EVAL_GL + 1, min(md + 1, A), False),
            (6, min(big, A), True)]


@functools.lru_cache(maxsize=None)
def eval_case(A, md):
    rng = _rng(7, A, md)
    dets, gts, anchors = [], [], []
    for n_gt, k, dup in eval_counts(A, md):
        d, g, a = eval_image(rng, n_gt, k, A, dup)
        dets.append(d), gts.append(g), anchors.append(a)
    B = len(dets)
    score = rng.uniform(0.0, 1.0, (B, A)).astype(F32)
    cls = rng.integers(0, E.N_CLS + 2, (B, A)).astype(np.int32)
    box = rng.uniform(1.0, 299.0, (B, A, 4)).astype(F32)
    keep = np.zeros((B, A), np.uint8)
    for i, ((s, c, b), anc) in enumerate(zip(dets, anchors)):
        score[i, anc], cls[i, anc], box[i, anc], keep[i, anc] = s, c, b, rng.choice(CAND_BYTES, len(anc))
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(g[0]) for g in gts])
    ref, _ = E.match_reference(dets, gts, md)
    n_det = np.array([len(r[0]) for r in ref], np.int32)
    d_score, d_cls = np.zeros((B, md), F32), np.full((B, md), -1, np.int32)
    d_box, d_flags = np.zeros((B, md, 4), F32), np.zeros((B, md), np.uint16)
    for i, (s, c, b, f) in enumerate(ref):
        d_score[i, :len(s)], d_cls[i, :len(s)], d_box[i, :len(s)], d_flags[i, :len(s)] = s, c, b, f
    return dict(A=A, B=B, md=md, dets=dets, gts=gts, anchors=anchors, score=score, cls=cls, box=box, keep=keep,
                gt_cls=np.concatenate([g[0] for g in gts]).astype(np.int32),
                gt_box=np.concatenate([g[1].reshape(-1, 4) for g in gts]).astype(np.float64), gt_off=off,
                want=(n_det, d_score, d_cls, d_box, d_flags))
