"""Inputs and expected values of the strict anchor-side tests (tests/test_anchor_strict_gpu.py): small prior geometries, ragged
matcher batches, logits with exact class ties and exactly decided thresholds, NMS inputs with ties on the max_cand cut, and
evaluation batches at several anchor counts.  Plain numpy, importable without a GPU; every expected value comes from
oracle/ssd_oracle.py, tests/eval_cases.py:match_reference or utils/metrics.py.  tests/test_anchor_cases_cpu.py asserts the
conditions the cases rest on.  Everything is seeded and cached: treat what these functions return as read-only."""
import functools

import numpy as np

from oracle import ssd_oracle as O
from tests import detect_pairs_oracle as R
from tests import eval_cases as E

M = E.M
F32 = np.float32

# ---- prior geometries ------------------------------------------------------------------------------------------------------------
GEOMETRIES = {
    "G4": dict(grids=((1, 1),), s_ref=(120, 210), ratios=((2,),), in_size=300),                          # one cell
    "G190": dict(R.SMALL_GEOMETRY, in_size=300),                                                         # A % 4 == 2, A < 256
    "G790": dict(grids=((10, 10), (5, 5), (3, 3), (1, 1)), s_ref=(60, 111, 162, 213, 264),
                 ratios=((2, 3), (2, 3), (2,), (2,)), in_size=300),                                       # 3 * 256 + 22, A % 4 == 2
    "G380": dict(grids=((8, 8), (4, 4), (2, 2), (1, 1)), s_ref=(45, 99, 153, 207, 261),
                 ratios=((2,), (2, 3), (2, 3), (2,)), in_size=300),                                       # A % 4 == 0, < 1024 quads
}
ANCHORS = {"G4": 4, "G190": 190, "G790": 790, "G380": 380}
GEOMETRY_OF_A = {190: "G190", 790: "G790"}


@functools.lru_cache(None)
def priors(name):
    return O.priors(**GEOMETRIES[name])


def random_boxes(rng, n):
    """centres in [0.05, 0.95], log-uniform sizes in [0.05, 0.7]"""
    c = rng.uniform(0.05, 0.95, (n, 2))
    wh = np.exp(rng.uniform(np.log(0.05), np.log(0.7), (n, 2)))
    return np.concatenate([c, wh], 1).astype(F32)


# ---- case 1: the helpers ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def helper_case(name, n):
    """n paired rows for ssd_iou_n / ssd_apply_anchor_box: float32 boxes against the geometry's priors (cycled)"""
    P = priors(name)
    rng = np.random.default_rng(7000 + 13 * n + len(P))
    pri = np.ascontiguousarray(P[np.arange(n) % len(P)])
    box = random_boxes(rng, n)
    if n > 8:
        box[1] = pri[1].astype(F32)                       # the prior itself (rounded): log terms next to 0
        box[2, 2:] = 0.0                                  # zero area: both 1e-10 clamps of iou_n, the 1e-5 clamp of the encoding
        box[3, 2:] = 1e-7
        box[4, :2] = (3.0, -2.0)                          # far outside: no overlap
        box[5] = box[6]                                   # a duplicate
    return dict(box=box, pri=pri, iou=O.iou_n(box, pri), enc=O.encode(box, pri))


@functools.lru_cache(None)
def enc_zero(name):
    P = priors(name)
    return O.encode(np.zeros((len(P), 4), F32), P).astype(F32)


# ---- cases 2 and 3: the matcher ---------------------------------------------------------------------------------------------------
def match_expected(gt_cls, gt_box, P, thresh=0.5):
    """what tests.test_match_gpu.check_image compares one image with: O.match_literal + O.encode"""
    A = len(P)
    if len(gt_box) == 0:                                  # the reference's generator never sees one; all rows stay unmatched
        cls, box, mask = np.zeros(A, np.int32), np.zeros((A, 4), F32), np.zeros(A, bool)
    else:
        cls, box, mask = O.match_literal(gt_cls, gt_box, P, thresh)
    return dict(mask=mask, cls=cls, box=box, enc=O.encode(box, P).astype(F32), gt_box=gt_box, gt_cls=gt_cls)


MATCH_BATCHES = {("G4", "main"): (4, 1, 0), ("G190", "main"): (0, 1, 7, 64), ("G790", "main"): (512, 513, 600, 3),
                 ("G790", "small"): (3, 64, 33, 0)}


@functools.lru_cache(None)
def match_batch(name, which="main"):
    """One ragged batch: list of match_expected dicts.  "main" batches are the three-launch cases of the issue; ("G790",
    "small") stays within the single-launch path's 64 boxes per image."""
    from tests.test_cfg5_gpu import _conflict_heavy
    P = priors(name)
    rng = np.random.default_rng(4100 + 17 * len(P) + (5 if which == "small" else 0))
    images = []
    for n in MATCH_BATCHES[(name, which)]:
        if n == 64:
            box = _conflict_heavy(rng, n)                 # rows share their best prior: the literal phase-1 order
        else:
            box = random_boxes(rng, n) if n else np.zeros((0, 4), F32)
        if n == 7:
            box[3] = box[1]                               # a duplicate
            box[5, 2:] = 0.0                              # a zero-area box
        cls = rng.integers(0, 80, n).astype(F32)
        images.append(match_expected(cls, box, P))
    return images


def pack_gt(images):
    """(gt_box f32 [total,4], gt_cls f32 [total], gt_off i32 [B+1], total, max_nt) as numpy"""
    counts = [len(i["gt_box"]) for i in images]
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    box = np.concatenate([i["gt_box"].reshape(-1, 4) for i in images], 0).astype(F32)
    cls = np.concatenate([i["gt_cls"].reshape(-1) for i in images], 0).astype(F32)
    return box, cls, off, int(off[-1]), max(counts)


# ---- case 4: score / decode -----------------------------------------------------------------------------------------------------------
SCORE_THRESH = 0.3
SCORE_CASES = [(C, "f32") for C in (2, 3, 6, 80, 81)] + [(6, "bf16"), (81, "bf16")]
TIE_LOGIT = 20.0


def bf16_round(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, F32)).to(torch.bfloat16).float().numpy()


def tie_pairs(C):
    """(lo, hi) foreground indices that tie: within the first half-row of k_score_decode, across the two halves (inner, first of
    each, last of the first with first of the second) and within the second half.  C = 81: (3, 50), (0, 40), (39, 40), (50, 79),
    (0, 39).  C = 3 has the one pair (0, 1); C = 2 has a single foreground class and no pair."""
    nfg = C - 1
    h = (nfg + 1) // 2                                     # the first half is [0, h), the second [h, nfg)
    want = [(min(3, h - 1), min(h + 10, nfg - 1)), (0, h), (h - 1, h), (min(h + 10, nfg - 2), nfg - 1), (0, h - 1)]
    out = []
    for lo, hi in want:
        if 0 <= lo < hi < nfg and (lo, hi) not in out:
            out.append((lo, hi))
    return out


@functools.lru_cache(None)
def score_case(A, C, dt, B=3):
    """Random background-dominated logits with hot anchors (detect_pairs_oracle.synth_logits2) plus rows whose best foreground
    logit appears twice, bit-equal.  conf / loc hold bf16-exact values for dt == "bf16".  With the float64 oracle's values."""
    conf, loc = R.synth_logits2(B, A, C, max(16, A // 6), 900 + A + 7 * C + (1 if dt == "bf16" else 0), per_anchor=1)
    n = B * A
    flat = conf.reshape(n, C)
    ties = []
    for k, (lo, hi) in enumerate(tie_pairs(C)):
        for m in range(4):
            row = (17 + 37 * k + 131 * m) % n              # every 128-row block of the sweep, and both images' borders
            flat[row, lo] = flat[row, hi] = TIE_LOGIT
            ties.append((row, lo, hi))
    if dt == "bf16":
        conf, loc = bf16_round(conf), bf16_round(loc)
    s, c, cand = O.score(conf, SCORE_THRESH)
    p_bg = np.exp(O._log_softmax(conf))[..., -1]
    border = (np.abs(s - SCORE_THRESH) < 1e-6) | (np.abs(p_bg - SCORE_THRESH) < 1e-6)
    cls = conf[..., :-1].argmax(-1).astype(np.int32)       # first index of the best foreground logit: exact on exact inputs
    box = O.decode(loc, priors(GEOMETRY_OF_A[A])[None], 300)
    return dict(conf=conf, loc=loc, ties=ties, score=s, cls_oracle=c, cls=cls, cand=cand, border=border, box=box)


@functools.lru_cache(None)
def threshold_case(A, C, dt, B=3):
    """Logits whose background term is decided without rounding in every row: the background logit equals the best foreground
    logit bit for bit (tie rows: p_bg == score exactly, never a candidate) or lies 30 below it (p_bg ~ 1e-13).  All values are
    multiples of 0.25 of magnitude below 64: exact in bf16.  One non-tie row (`src`) is copied over `dups`: rows whose score
    equals the threshold the test takes from src."""
    rng = np.random.default_rng(1300 + A + 7 * C + (1 if dt == "bf16" else 0))
    conf = (rng.integers(-16, 17, (B, A, C)) * 0.25).astype(F32)
    best = conf[..., :-1].max(-1)
    tie = rng.random((B, A)) < 0.3
    conf[..., -1] = np.where(tie, best, best - F32(30.0))
    flat = conf.reshape(B * A, C)
    nontie = np.nonzero(~tie.reshape(-1))[0]
    src = int(nontie[len(nontie) // 2])
    dups = nontie[[1, len(nontie) // 3, len(nontie) - 2]]
    flat[dups] = flat[src]
    loc = rng.normal(0, 0.2, (B, A, 4)).astype(F32)
    if dt == "bf16":
        loc = bf16_round(loc)
    cls = conf[..., :-1].argmax(-1).astype(np.int32)
    box = O.decode(loc, priors(GEOMETRY_OF_A[A])[None], 300)
    return dict(conf=conf, loc=loc, tie=tie, src=src, dups=dups, cls=cls, box=box)


# ---- case 5: NMS ------------------------------------------------------------------------------------------------------------------
NMS_ANCHORS = (1, 3, 190, 380, 1023, 4099, 65536)
NMS_MAX_CAND = (1, 50, 1024)
NMS_IOU = 0.45


@functools.lru_cache(None)
def nms_case(A):
    """score / cls / box / cand built directly.  Image 0: up to 1500 candidates with scores on 32 levels (exact ties everywhere,
    also across every max_cand cut), a third of them of class 0 (a segment longer than a wave), the others spread over eleven
    short segments; anchors 0 and A - 1 are candidates of one class with the tied top score and nearly the same box: the lower
    anchor survives, the higher is suppressed.  Image 1: no candidate.  Image 2 (A >= 3): nine candidates at most.  Entries of
    non-candidates are NaN / class -7: nothing may depend on them."""
    B = 3 if A >= 3 else 2
    rng = np.random.default_rng(5200 + A)
    score = np.full((B, A), np.nan, F32)
    cls = np.full((B, A), -7, np.int32)
    box = np.full((B, A, 4), np.nan, F32)
    cand = np.zeros((B, A), np.uint8)

    def fill(b, idx):
        k = len(idx)
        cand[b, idx] = 1
        score[b, idx] = (rng.integers(1, 33, k) / 64.0 + 0.25).astype(F32)
        cls[b, idx] = np.where(rng.random(k) < 0.34, 0, rng.integers(1, 12, k)).astype(np.int32)
        centres = rng.uniform(40, 260, (24, 2))
        box[b, idx, :2] = (centres[rng.integers(0, 24, k)] + rng.normal(0, 14, (k, 2))).astype(F32)
        box[b, idx, 2:] = rng.uniform(20, 60, (k, 2)).astype(F32)

    fill(0, np.sort(rng.choice(A, min(A, 1500), replace=False)))
    if A >= 3:
        ends = np.array([0, A - 1])
        cand[0, ends] = 1
        score[0, ends] = F32(0.99)
        cls[0, ends] = 5
        box[0, 0] = (150.0, 150.0, 50.0, 40.0)
        box[0, A - 1] = (151.0, 150.0, 50.0, 40.0)
        fill(2, np.sort(rng.choice(A, min(A, 9), replace=False)))
    want = {}
    for mc in NMS_MAX_CAND:
        keep = np.stack([O.nms(score[b], cls[b], box[b], cand[b], NMS_IOU, mc) for b in range(B)]).astype(np.uint8)
        want[mc] = (keep, keep.sum(1).astype(np.int32))
    return dict(score=score, cls=cls, box=box, cand=cand, want=want, B=B)


def nms_order(case, b):
    """candidate anchors of image b in (score desc, anchor asc) order, and their scores"""
    idx = np.nonzero(case["cand"][b])[0]
    order = idx[np.lexsort((idx, -case["score"][b][idx].astype(np.float64)))]
    return order, case["score"][b][order]


# ---- case 6: evaluation -----------------------------------------------------------------------------------------------------------
EVAL_ANCHORS = (3, 190, 4099)
EVAL_MAX_DETS = (1, 100, 128)
_EVAL_KEPT = {3: (0, 3, 4), 190: (100, 190, 20), 4099: (900, 1600, 50)}       # kept lo, kept hi, score quantisation
PLANT_CLS = E.N_CLS + 1                                    # a detection class that E.gen gives no ground truth
PLANT_GT = ((100.0, 100.0, 40.0, 40.0), (120.0, 100.0, 40.0, 40.0))
PLANT_DET = ((110.0, 100.0, 40.0, 40.0), (120.0, 100.0, 40.0, 40.0))


@functools.lru_cache(None)
def eval_case(A, B=4):
    """E.gen at A anchors with 0 .. 60 ground truths per image and quantised scores; image 1 has no kept anchor.  Returns the
    dense [B, A] maps (as tests.test_eval_device_gpu.dense_batch makes them), the CSR ground truth and per max_dets the five
    dense outputs of E.match_reference."""
    lo, hi, quant = _EVAL_KEPT[A]
    for seed in range(6100 + A, 6200 + A):                # the first draw with ground-truth counts on both sides of the LDS limit
        rng = np.random.default_rng(seed)
        dets, gts, anchors = E.gen(rng, B, lo, hi, quant=quant, n_gt_hi=60, n_anchors=A)
        counts = [len(g[0]) for g in gts]
        if max(counts[2:]) > 48 and 0 < min(counts[2:]) <= 46 and counts[0] <= 46:
            break
    else:
        raise AssertionError("no draw with the wanted ground-truth counts")
    # image 0: two ground truths of one class at equal IoU (0.6, exact in float64) from the best detection, the second-best
    # detection exactly on the later one.  "The last index wins": the best claims the later box at 0.5 .. 0.6, the second-best
    # finds it taken there (its IoU with the earlier box is 1/3) and claims it only from 0.65 on.
    s, c, b = dets[0]
    anc = anchors[0]
    if len(s) < 2:
        s, c, b, anc = np.zeros(2, F32), np.zeros(2, np.int32), np.zeros((2, 4), F32), np.array([0, A - 1])
    s, c, b = s.copy(), c.copy(), b.copy()
    s[:2], c[:2] = (F32(0.97), F32(0.96)), PLANT_CLS
    b[0], b[1] = PLANT_DET
    dets[0], anchors[0] = (s, c, b), anc
    gts[0] = (np.concatenate([gts[0][0], [PLANT_CLS, PLANT_CLS]]).astype(np.int32),
              np.concatenate([gts[0][1].reshape(-1, 4), np.asarray(PLANT_GT, np.float64)]))
    dets[1] = (np.zeros(0, F32), np.zeros(0, np.int32), np.zeros((0, 4), F32))
    anchors[1] = np.zeros(0, np.int64)
    score = rng.uniform(0.0, 1.0, (B, A)).astype(F32)
    cls = rng.integers(0, E.N_CLS + 2, (B, A)).astype(np.int32)
    box = rng.uniform(1.0, 299.0, (B, A, 4)).astype(F32)
    keep = np.zeros((B, A), np.uint8)
    for i, ((s, c, b), anc) in enumerate(zip(dets, anchors)):
        score[i, anc], cls[i, anc], box[i, anc], keep[i, anc] = s, c, b, 1
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(g[0]) for g in gts])
    gcls = np.concatenate([g[0] for g in gts]).astype(np.int32)
    gbox = np.concatenate([g[1].reshape(-1, 4) for g in gts]).astype(np.float64)
    want = {}
    for md in EVAL_MAX_DETS:
        ref, _ = E.match_reference(dets, gts, md)
        n_det = np.zeros(B, np.int32)
        d_score, d_cls = np.zeros((B, md), F32), np.full((B, md), -1, np.int32)
        d_box, d_flags = np.zeros((B, md, 4), F32), np.zeros((B, md), np.uint16)
        for i, (s, c, b, f) in enumerate(ref):
            k = len(s)
            n_det[i], d_score[i, :k], d_cls[i, :k], d_box[i, :k], d_flags[i, :k] = k, s, c, b, f
        want[md] = (n_det, d_score, d_cls, d_box, d_flags)
    return dict(score=score, cls=cls, box=box, keep=keep, gt_cls=gcls, gt_box=gbox, gt_off=off, want=want, dets=dets, gts=gts, B=B)


@functools.lru_cache(None)
def ap_case():
    """Rows for ssd_eval_ap: class 0 with 700 rows (several chunks of the scan), class 1 empty with ground truth, class 2 with
    rows and no ground truth, class 3 with 300 rows, class 4 with a single row."""
    rng = np.random.default_rng(6400)
    C = 5
    n_rows = (700, 0, 40, 300, 1)
    n_gt = np.array([300, 7, 0, 90, 2], np.int32)
    cls = np.concatenate([np.full(n, c, np.int64) for c, n in enumerate(n_rows)])
    perm = rng.permutation(len(cls))                      # rows arrive in (image, rank) order, not by class
    cls = cls[perm]
    score = (np.round(rng.uniform(0.05, 1.0, len(cls)) * 50) / 50).astype(F32)
    flags = (rng.integers(0, 1024, len(cls)) & rng.integers(0, 1024, len(cls))).astype(np.uint16)
    rows = (cls, score, flags)
    order = np.lexsort((np.arange(len(cls)), -score.astype(np.float64), cls))
    seg = np.zeros(C + 1, np.int32)
    seg[1:] = np.cumsum(np.bincount(cls, minlength=C)[:C])
    table = M.ap_table_from_flags(rows, n_gt)
    ap = np.zeros((C, 10), np.float64)
    for c, v in table.items():
        ap[c] = v
    return dict(C=C, flags_sorted=flags[order], seg_off=seg, n_gt=n_gt, ap=ap, table=table, rows=rows)
