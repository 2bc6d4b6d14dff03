"""Cases for the COCO protocol of the device metric (ssd_eval_match_coco / ssd_eval_ap_coco), shared by
test_coco_summary_cpu.py and test_coco_eval_gpu.py.  Deterministic (seeded).  The restatement of the first stage is
utils.metrics.coco_match_image (the function coco_summary itself is made of); this module only arranges its results in the
kernel's output layout and counts, on its intermediate arrays, how often each event of the protocol occurs."""
import functools

import numpy as np

from tests.eval_cases import M

SCALES = (1.0, 4.0, 0.25)
# (B, A, classes with ground truth, max_dets, kept lo, kept hi, score quantisation): A not divisible by 4, max_dets 1 and 128,
# more than 1024 kept anchors (batch 3), 0 and 49 .. 60 boxes per image in every batch
BATCHES = ((3, 61, 3, 1, 10, 40, None), (5, 256, 4, 7, 20, 120, 20), (8, 2000, 6, 100, 30, 160, None),
           (4, 2000, 5, 128, 1100, 1500, 50), (6, 256, 6, 100, 60, 200, 10), (3, 61, 4, 128, 30, 61, None))
SETS = {"a": 4100, "b": 4200}                                 # case set -> seed
EVENTS = ("crowd_rematch", "ignored_match", "unmatched_out_of_range", "iou_tie", "boundary_area", "empty_image", "big_image")


def _sides(rng, scale):
    """(w, h) of one box in evaluation pixels: small / medium / large in source pixels, or exactly on a range boundary"""
    r = 1.0 / np.sqrt(scale)
    kind = rng.integers(0, 5)
    if kind == 0:
        return rng.uniform(8, 30, 2) * r
    if kind == 1:
        return rng.uniform(34, 90, 2) * r
    if kind == 2:
        return rng.uniform(100, 190, 2) * r
    side = (32.0 if kind == 3 else 96.0) * r                 # 16, 32, 64 or 48, 96, 192: the area is exactly 32^2 or 96^2
    return np.array([side, side])


def gen_batch(rng, B, A, n_cls, kept_lo, kept_hi, quant):
    """One batch: per image detections (score f32, cls i32, box f32 [k,4]) in anchor order, their anchors, ground truth
    (cls i32 [n], box f64 [n,4] pixels, crowd bool [n]) and the area scale.  Image 0 has no box, image 1 has 49 .. 60."""
    dets, gts, anchors, scales = [], [], [], []
    for i in range(B):
        scale = SCALES[int(rng.integers(0, len(SCALES)))]
        n = 0 if i == 0 else int(rng.integers(49, 61)) if i == 1 else int(rng.integers(1, 10))
        gcls = rng.integers(0, n_cls, n).astype(np.int32)
        gbox = np.zeros((n, 4), np.float64)
        for j in range(n):
            gbox[j] = np.concatenate([rng.uniform(60, 240, 2), _sides(rng, scale)])
        crowd = rng.random(n) < 0.2
        if n >= 2 and rng.random() < 0.6:
            gbox[1], gcls[1], crowd[1] = gbox[0], gcls[0], crowd[0]      # identical ground truths: the last index wins
        k = int(rng.integers(kept_lo, min(kept_hi, A) + 1))
        anc = np.sort(rng.choice(A, k, replace=False))
        score = rng.uniform(0.05, 1.0, k).astype(np.float32)
        if quant:
            score = (np.round(score * quant) / quant).astype(np.float32)
        cls = rng.integers(0, n_cls + 2, k).astype(np.int32)
        box = np.empty((k, 4), np.float32)
        for j in range(k):
            if n and rng.random() < 0.75:
                g = int(rng.integers(0, n))
                cls[j] = gcls[g] if rng.random() < 0.85 else cls[j]
                box[j] = (gbox[g] + rng.normal(0, 3.0, 4) * (rng.random() < 0.7)).astype(np.float32)
            else:
                box[j] = np.concatenate([rng.uniform(30, 270, 2), _sides(rng, scale)]).astype(np.float32)
        box[:, 2:] = np.abs(box[:, 2:]) + np.float32(0.0)
        if n >= 2 and k >= 2:
            box[0], cls[0] = gbox[0].astype(np.float32), gcls[0]         # an exact copy: IoU 1 with both identical boxes
            gbox[0] = gbox[1] = box[0].astype(np.float64)
        dets.append((score, cls, box))
        gts.append((gcls, gbox, crowd))
        anchors.append(anc)
        scales.append(scale)
    return dets, gts, anchors, np.asarray(scales, np.float64)


@functools.lru_cache(maxsize=None)
def case_set(name):
    """The batches of a case set: a list of dict(B, A, n_cls, max_dets, dets, gts, anchors, scale)."""
    rng = np.random.default_rng(SETS[name])
    out = []
    for B, A, n_cls, max_dets, lo, hi, quant in BATCHES:
        dets, gts, anchors, scale = gen_batch(rng, B, A, n_cls, lo, hi, quant)
        out.append(dict(B=B, A=A, n_cls=n_cls, max_dets=max_dets, dets=dets, gts=gts, anchors=anchors, scale=scale))
    return out


@functools.lru_cache(maxsize=None)
def match_reference(name, index, with_crowd=True, with_scale=True, max_dets=None):
    """What ssd_eval_match_coco is to compute for batch `index` of a set, in its output layout (slots beyond n_det zero, class
    -1), and the census of events.  Returns dict(n_det, score, cls, box, flags, tp, ig, pos, gt_ignore, census)."""
    case = case_set(name)[index]
    md = case["max_dets"] if max_dets is None else max_dets
    B = case["B"]
    out = dict(n_det=np.zeros(B, np.int32), score=np.zeros((B, md), np.float32), cls=np.full((B, md), -1, np.int32),
               box=np.zeros((B, md, 4), np.float32), tp=np.zeros((B, md, 4), np.uint16), ig=np.zeros((B, md, 4), np.uint16),
               pos=np.zeros((B, md), np.int32))
    census = dict.fromkeys(EVENTS, 0)
    ignore = []
    for i, ((s, c, b), (gc, gb, crowd)) in enumerate(zip(case["dets"], case["gts"])):
        r = M.coco_match_image(s, c, b, gc, gb, crowd if with_crowd else None, md, M.COCO_AREA_RANGES,
                               case["scale"][i] if with_scale else 1.0, census)
        k = len(r[0])
        out["n_det"][i] = k
        out["score"][i, :k], out["cls"][i, :k], out["box"][i, :k] = r[0], r[1], r[2]
        out["tp"][i, :k], out["ig"][i, :k], out["pos"][i, :k] = r[3], r[4], r[5]
        ignore.append(r[6])
        census["empty_image"] += int(len(gc) == 0)
        census["big_image"] += int(len(gc) > 48)
    out["flags"] = (out["tp"][:, :, 0] & ~out["ig"][:, :, 0]).astype(np.uint16)
    out["gt_ignore"] = np.concatenate(ignore).astype(np.uint8)
    out["census"] = census
    return out


def assert_census(total):
    """every event of the protocol occurs at least five times in a case set's summed census"""
    for k in EVENTS:
        assert total[k] >= 5, (k, total)


def dense_batch(case, seed=0):
    """The dense [B, A] maps ssd_score_decode + ssd_nms would leave for the batch's detections (kept anchors at the given
    positions; everything else random with keep = 0) and the CSR ground truth: numpy arrays score, cls, box, keep, gt_cls,
    gt_box, gt_off, gt_crowd (u8), area_scale."""
    rng = np.random.default_rng(seed)
    B, A = case["B"], case["A"]
    score = rng.uniform(0.0, 1.0, (B, A)).astype(np.float32)
    cls = rng.integers(0, case["n_cls"] + 2, (B, A)).astype(np.int32)
    box = rng.uniform(1.0, 299.0, (B, A, 4)).astype(np.float32)
    keep = np.zeros((B, A), np.uint8)
    for i, ((s, c, b), anc) in enumerate(zip(case["dets"], case["anchors"])):
        score[i, anc], cls[i, anc], box[i, anc], keep[i, anc] = s, c, b, 1
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(g[0]) for g in case["gts"]])
    return dict(score=score, cls=cls, box=box, keep=keep, gt_cls=np.concatenate([g[0] for g in case["gts"]]).astype(np.int32),
                gt_box=np.concatenate([g[1].reshape(-1, 4) for g in case["gts"]]).astype(np.float64), gt_off=off,
                gt_crowd=np.concatenate([g[2] for g in case["gts"]]).astype(np.uint8), area_scale=case["scale"].copy())


def rows_of(ref):
    """(cls, score, tp, ig, pos) of a match_reference result's live slots, in (image, rank) order"""
    live = np.arange(ref["cls"].shape[1])[None, :] < ref["n_det"][:, None]
    return ref["cls"][live], ref["score"][live], ref["tp"][live], ref["ig"][live], ref["pos"][live]


def n_gt_of(case, ref, C):
    """non-ignored ground truths per (area range, class) int32 [4, C]"""
    gcls = np.concatenate([g[0] for g in case["gts"]]).astype(int)
    n = np.zeros((4, C), np.int32)
    for a in range(4):
        for c in gcls[((ref["gt_ignore"] >> a) & 1) == 0]:
            n[a, c] += 1
    return n


def ap_rows_case(seed=9):
    """Rows for ssd_eval_ap_coco that no matching produced: class 0 with 1500 rows of which rows 256 .. 767 (two whole chunks
    of the scan) are ignored at every threshold in ranges 1 and 2; class 1 empty, with ground truth; class 2 with 300 rows
    ignored throughout in range 3; class 3 without ground truth.  Returns dict(rows, n_gt [4,C], C, max_dets)."""
    rng = np.random.default_rng(seed)
    C, max_dets = 4, 100
    cls = np.concatenate([np.zeros(1500, np.int64), np.full(300, 2, np.int64), np.full(40, 3, np.int64)])
    N = len(cls)
    score = (np.round(rng.uniform(0, 1, N) * 200) / 200).astype(np.float32)          # many equal scores
    tp = (rng.integers(0, 1024, (N, 4)) & rng.integers(0, 1024, (N, 4))).astype(np.uint16)
    ig = (rng.integers(0, 1024, (N, 4)) & rng.integers(0, 1024, (N, 4)) & rng.integers(0, 1024, (N, 4))).astype(np.uint16)
    pos = np.minimum(rng.geometric(0.15, N) - 1, max_dets - 1).astype(np.int32)
    n_gt = np.array([[900, 5, 200, 0], [300, 5, 0, 0], [700, 0, 90, 0], [400, 2, 120, 0]], np.int32)
    # whole chunks ignored: sort order is by score within class 0, so mark by rank in that order
    order0 = np.lexsort((np.arange(1500), -score[:1500].astype(np.float64)))
    ig[order0[256:768], 1] = 0x3ff
    ig[order0[256:768], 2] = 0x3ff
    ig[1500:1800, 3] = 0x3ff
    return dict(rows=(cls, score, tp, ig, pos), n_gt=n_gt, C=C, max_dets=max_dets)


def sorted_rows(rows, C):
    """rows in ssd_eval_ap_coco's order (class asc, score desc, image, rank) and seg_off"""
    cls, score, tp, ig, pos = rows
    order = np.lexsort((np.arange(len(cls)), -score.astype(np.float64), np.where(cls < C, cls, C)))
    order = order[np.asarray(cls)[order] < C] if len(order) else order
    seg = np.zeros(C + 1, np.int32)
    seg[1:] = np.cumsum(np.bincount(np.asarray(cls)[np.asarray(cls) < C].astype(int), minlength=C)[:C])
    return tp[order], ig[order], pos[order], seg
