"""Cases for the PASCAL VOC metric (utils.metrics.voc_map, ssd_eval_match_voc / ssd_eval_ap_voc), shared by
test_voc_metric_cpu.py and test_voc_eval_gpu.py.  Deterministic (seeded).

voc_map is build-defined: it restates the published VOCdevkit procedure (VOCevaldet) in numpy and is unpinned -- the devkit is
not available to run.  `devkit` below is a second, independent restatement of the same published procedure, written the way
the devkit is laid out (per class, one global score sort, a `det` array per image, plain loops and scalar arithmetic) and
sharing no code with voc_map; agreement of the two shows that neither has a slip of its own, not that either equals a run
of the devkit."""
import functools

import numpy as np

from tests.eval_cases import M


# ---- the independent restatement ---------------------------------------------------------------------------------------------
def _iou(d, g):
    """two (cx, cy, w, h) boxes, scalar float64 arithmetic in iou_matrix's order of operations"""
    a0, a1, a2, a3 = d[0] - d[2] / 2, d[1] - d[3] / 2, d[0] + d[2] / 2, d[1] + d[3] / 2
    b0, b1, b2, b3 = g[0] - g[2] / 2, g[1] - g[3] / 2, g[0] + g[2] / 2, g[1] + g[3] / 2
    w = max(min(a2, b2) - max(a0, b0), 0.0)
    h = max(min(a3, b3) - max(a1, b1), 0.0)
    inter = w * h
    union = (a2 - a0) * (a3 - a1) + (b2 - b0) * (b3 - b1) - inter
    return inter / union if union > 0 else 0.0


def devkit(detections, ground_truths, year="07", iou_thresh=0.5, max_dets=100):
    """(per_class {cls: AP}, n_pos {cls: count}, flags per image: uint8 [k] over the image's scored detections in (score desc,
    index asc) order, bit 0 true positive, bit 1 ignored)"""
    cut = []                                                          # per image: its scored detections, best first
    for score, cls, box in detections:
        idx = sorted(range(len(score)), key=lambda i: (-float(score[i]), i))[:max_dets]
        cut.append([(float(score[i]), int(cls[i]), [float(v) for v in np.asarray(box[i], np.float64)]) for i in idx])
    flags = [np.zeros(len(c), np.uint8) for c in cut]
    classes = sorted({int(c) for g in ground_truths for c in np.asarray(g[0]).reshape(-1)})
    per_class, n_pos = {}, {}
    for c in classes:
        gt, npos = [], 0                                              # per image: boxes, difficult, det
        for g in ground_truths:
            gcls = np.asarray(g[0]).reshape(-1)
            hard = np.zeros(len(gcls), bool) if len(g) < 3 or g[2] is None else np.asarray(g[2]).astype(bool).reshape(-1)
            own = [j for j in range(len(gcls)) if int(gcls[j]) == c]
            gt.append(dict(box=[[float(v) for v in np.asarray(g[1], np.float64).reshape(-1, 4)[j]] for j in own],
                           hard=[bool(hard[j]) for j in own], det=[False] * len(own)))
            npos += sum(1 for j in own if not hard[j])
        rows = [(s, img, rank) for img, dets in enumerate(cut) for rank, (s, k, _) in enumerate(dets) if k == c]
        rows.sort(key=lambda r: (-r[0], r[1], r[2]))
        tp, fp = [], []
        for s, img, rank in rows:
            ovmax, jmax = -np.inf, -1
            for j, gb in enumerate(gt[img]["box"]):
                ov = _iou(cut[img][rank][2], gb)
                if ov > ovmax:
                    ovmax, jmax = ov, j
            t = f = 0
            if ovmax >= iou_thresh:
                if gt[img]["hard"][jmax]:
                    flags[img][rank] = 2
                elif not gt[img]["det"][jmax]:
                    t, gt[img]["det"][jmax] = 1, True
                    flags[img][rank] = 1
                else:
                    f = 1
            else:
                f = 1
            tp.append(t)
            fp.append(f)
        if npos == 0:
            continue
        n_pos[c] = npos
        rec, prec, ctp, cfp = [], [], 0, 0
        for t, f in zip(tp, fp):
            ctp, cfp = ctp + t, cfp + f
            rec.append(ctp / npos)
            prec.append(ctp / max(ctp + cfp, 1))
        if year == "07":
            ap = 0.0
            for k in range(11):
                p = 0.0
                for r, q in zip(rec, prec):
                    if r >= k / 10.0 and q > p:
                        p = q
                ap += p
            per_class[c] = ap / 11.0
        else:
            mrec, mpre = [0.0] + rec + [1.0], [0.0] + prec + [0.0]
            for i in range(len(mpre) - 2, -1, -1):
                mpre[i] = max(mpre[i], mpre[i + 1])
            ap = 0.0
            for i in range(len(mrec) - 1):
                if mrec[i + 1] != mrec[i]:
                    ap += (mrec[i + 1] - mrec[i]) * mpre[i + 1]
            per_class[c] = ap
    return per_class, n_pos, flags


# ---- hand-made cases -----------------------------------------------------------------------------------------------------------
def _img(dets, gts):
    """dets: [(score, cls, box)], gts: [(cls, box, difficult)] -> the arrays of one image"""
    d = (np.array([x[0] for x in dets], np.float32), np.array([x[1] for x in dets], np.int32),
         np.array([x[2] for x in dets], np.float32).reshape(-1, 4))
    g = (np.array([x[0] for x in gts], np.int32), np.array([x[1] for x in gts], np.float64).reshape(-1, 4),
         np.array([x[2] for x in gts], bool))
    return d, g


def _case(name, images, max_dets=100, iou_thresh=0.5, **want):
    pairs = [_img(d, g) for d, g in images]
    return dict(name=name, dets=[p[0] for p in pairs], gts=[p[1] for p in pairs], max_dets=max_dets, iou_thresh=iou_thresh,
                want=want)


G0, G1 = (100.0, 100.0, 40.0, 40.0), (110.0, 100.0, 40.0, 40.0)      # IoU 0.6 with each other
FAR = (220.0, 220.0, 30.0, 30.0)
TEN = [(0, (20.0 + 28.0 * j, 40.0, 20.0, 20.0), False) for j in range(10)]

# want: flags per image (bit 0 true positive, bit 1 ignored), gt per image (det_gt), ap07 / ap12 {cls: AP}, n_pos
HAND = [
    # (TP, FP, TP), n_pos 2: precision 1, 1/2, 2/3 at recall 1/2, 1/2, 1
    _case("hand", [([(0.9, 0, G0), (0.8, 0, (30.0, 30.0, 10.0, 10.0)), (0.7, 0, FAR)], [(0, G0, False), (0, FAR, False)])],
          flags=[[1, 0, 1]], gt=[[0, -1, 1]], ap07={0: 28.0 / 33.0}, ap12={0: 5.0 / 6.0}, n_pos={0: 2}),
    # both detections overlap both boxes at >= 0.5 and both have G0 as their best box: VOC scores TP, FP (a duplicate), the
    # greedy COCO rule TP, TP
    _case("duplicate", [([(0.9, 0, G0), (0.8, 0, (102.0, 100.0, 40.0, 40.0))], [(0, G0, False), (0, G1, False)])],
          flags=[[1, 0]], gt=[[0, 0]], ap07={0: 6.0 / 11.0}, ap12={0: 0.5}, n_pos={0: 2}),
    # two identical boxes: the first index is taken, by the later detection too
    _case("first_index_tie", [([(0.9, 0, G0), (0.8, 0, G0)], [(0, G0, False), (0, G0, False)])],
          flags=[[1, 0]], gt=[[0, 0]], ap07={0: 6.0 / 11.0}, ap12={0: 0.5}, n_pos={0: 2}),
    # the best box is difficult: ignored although the non-difficult G1 also passes; then a detection that is G1's
    _case("difficult_best", [([(0.9, 0, G0), (0.8, 0, G1)], [(0, G0, True), (0, G1, False)])],
          flags=[[2, 1]], gt=[[0, 1]], ap07={0: 1.0}, ap12={0: 1.0}, n_pos={0: 1}),
    # an unmatched difficult box does not lower recall; class 1 has only difficult boxes and is absent
    _case("difficult_unmatched", [([(0.9, 0, G0), (0.5, 1, FAR)], [(0, G0, False), (0, FAR, True), (1, FAR, True)])],
          flags=[[1, 2]], gt=[[0, 2]], ap07={0: 1.0}, ap12={0: 1.0}, n_pos={0: 1}),
    # ovmax exactly 0.5 (every operation exact): a box of half the area inside the ground truth
    _case("at_threshold", [([(0.9, 0, (100.0, 100.0, 40.0, 20.0))], [(0, G0, False)])],
          flags=[[1]], gt=[[0]], ap07={0: 1.0}, ap12={0: 1.0}, n_pos={0: 1}),
    # recall exactly 3/10 reaches recall point 3: four points at precision 1
    _case("recall_three_tenths", [([(0.9 - 0.1 * j, 0, TEN[j][1]) for j in range(3)], TEN)],
          flags=[[1, 1, 1]], gt=[[0, 1, 2]], ap07={0: 4.0 / 11.0}, ap12={0: 0.3}, n_pos={0: 10}),
    # max_dets 2: the three lower-scored detections (one of them right) are never scored
    _case("max_dets_cut", [([(0.3, 0, FAR), (0.9, 0, (30.0, 30.0, 10.0, 10.0)), (0.8, 0, G0), (0.2, 0, G0), (0.1, 0, G1)],
                           [(0, G0, False), (0, FAR, False)])], max_dets=2,
          flags=[[0, 1]], gt=[[-1, 0]], ap07={0: 6.0 / 11.0 * 0.5}, ap12={0: 0.25}, n_pos={0: 2}),
    # an image without detections, one without boxes, and a class (2) that is detected but has no box anywhere
    _case("empty_sides", [([], [(0, G0, False)]), ([(0.9, 0, G0), (0.8, 2, G0)], [])],
          flags=[[], [0, 0]], gt=[[], [-1, -1]], ap07={0: 0.0}, ap12={0: 0.0}, n_pos={0: 1}),
]


# ---- random images -------------------------------------------------------------------------------------------------------------
def gen_images(rng, n_img, n_cls=5, kept_lo=0, kept_hi=40, quant=20, n_gt_hi=8, n_gt_lo=0):
    """Per image detections (score f32, cls i32, box f32 [k,4]) and ground truth (cls i32 [n], box f64 [n,4], difficult bool
    [n]).  About 70 % of the detections are jittered or exact copies of a box; a quarter of the boxes are difficult; 30 % of the
    images carry two identical boxes; detections also use two classes without any box; scores are quantised (ties)."""
    dets, gts = [], []
    for _ in range(n_img):
        n = int(rng.integers(n_gt_lo, n_gt_hi + 1))
        gcls = rng.integers(0, n_cls, n).astype(np.int32)
        gbox = np.concatenate([rng.uniform(40, 260, (n, 2)), rng.uniform(16, 120, (n, 2))], 1)
        gbox = gbox.astype(np.float32).astype(np.float64)             # float32 values: an exact copy then has IoU exactly 1
        hard = rng.random(n) < 0.25
        if n >= 2 and rng.random() < 0.3:
            gbox[1], gcls[1] = gbox[0], gcls[0]
        if n >= 3 and rng.random() < 0.5:                             # a close neighbour of the same class: duplicates
            gbox[2], gcls[2] = gbox[0] + np.array([float(rng.integers(2, 13)), 0.0, 0.0, 0.0]), gcls[0]
        k = int(rng.integers(kept_lo, kept_hi + 1))
        score = rng.uniform(0.05, 1.0, k).astype(np.float32)
        if quant:
            score = (np.round(score * quant) / quant).astype(np.float32)
        cls = rng.integers(0, n_cls + 2, k).astype(np.int32)
        box = np.concatenate([rng.uniform(30, 270, (k, 2)), rng.uniform(16, 120, (k, 2))], 1).astype(np.float32)
        for j in range(k):
            if n and rng.random() < 0.7:
                g = int(rng.integers(0, n))
                cls[j] = gcls[g] if rng.random() < 0.9 else cls[j]
                box[j] = (gbox[g] + rng.normal(0, 4.0, 4) * (rng.random() < 0.7)).astype(np.float32)
        box[:, 2:] = np.abs(box[:, 2:]) + np.float32(1.0)
        dets.append((score, cls, box))
        gts.append((gcls, gbox, hard))
    return dets, gts


@functools.lru_cache(maxsize=None)
def random_set(seed=7100, n_img=200):
    dets, gts = gen_images(np.random.default_rng(seed), n_img)
    return dict(name="random%d" % seed, dets=dets, gts=gts, max_dets=20, iou_thresh=0.5, want={})


# ---- the kernels' layouts ------------------------------------------------------------------------------------------------------
def dense_batch(case, A, seed=0, all_kept=False):
    """The dense [B, A] maps ssd_score_decode + ssd_nms would leave for the case's detections, each image's detections at
    random anchors in their list order (everything else random with keep = 0), and the CSR ground truth.  all_kept: every
    image must bring exactly A detections, which sit at anchors 0 .. A-1.  numpy arrays score, cls, box, keep, gt_cls, gt_box,
    gt_off, gt_difficult."""
    rng = np.random.default_rng(seed)
    B = len(case["dets"])
    score = rng.uniform(0.0, 1.0, (B, A)).astype(np.float32)
    cls = rng.integers(0, 7, (B, A)).astype(np.int32)
    box = rng.uniform(1.0, 299.0, (B, A, 4)).astype(np.float32)
    keep = np.zeros((B, A), np.uint8)
    for i, (s, c, b) in enumerate(case["dets"]):
        assert len(s) <= A and (not all_kept or len(s) == A)
        anc = np.sort(rng.choice(A, len(s), replace=False))
        score[i, anc], cls[i, anc], box[i, anc], keep[i, anc] = s, c, b, 1
    off = np.zeros(B + 1, np.int32)
    off[1:] = np.cumsum([len(g[0]) for g in case["gts"]])
    cat = lambda k, dt, tail: np.concatenate([np.asarray(g[k]).reshape((-1,) + tail) for g in case["gts"]]).astype(dt) \
        if B else np.zeros((0,) + tail, dt)
    return dict(score=score, cls=cls, box=box, keep=keep, gt_cls=cat(0, np.int32, ()), gt_box=cat(1, np.float64, (4,)),
                gt_off=off, gt_difficult=cat(2, np.uint8, ()))


def match_reference(case, max_dets=None, with_difficult=True):
    """What ssd_eval_match_voc is to compute for the case as one batch, in its output layout (slots beyond n_det: score 0,
    class -1, box 0, flags 0, gt -1), from utils.metrics.voc_match_image."""
    md = case["max_dets"] if max_dets is None else max_dets
    B = len(case["dets"])
    out = dict(n_det=np.zeros(B, np.int32), score=np.zeros((B, md), np.float32), cls=np.full((B, md), -1, np.int32),
               box=np.zeros((B, md, 4), np.float32), flags=np.zeros((B, md), np.uint8), gt=np.full((B, md), -1, np.int32))
    for i, ((s, c, b), g) in enumerate(zip(case["dets"], case["gts"])):
        r = M.voc_match_image(s, c, b, g[0], g[1], g[2] if with_difficult else None, case["iou_thresh"], md)
        k = len(r[0])
        out["n_det"][i] = k
        out["score"][i, :k], out["cls"][i, :k], out["box"][i, :k] = r[0], r[1], r[2]
        out["flags"][i, :k] = r[3].astype(np.uint8) | (r[4].astype(np.uint8) << 1)
        out["gt"][i, :k] = r[5]
    return out


def sorted_flags(rows, C):
    """rows (cls, score, flags) in (image, rank) order -> (flags in ssd_eval_ap_voc's order (class asc, score desc, image,
    rank), seg_off i32 [C+1])"""
    cls, score, flags = (np.asarray(r) for r in rows)
    order = np.lexsort((np.arange(len(cls)), -score.astype(np.float64), np.where((cls >= 0) & (cls < C), cls, C)))
    order = order[(cls[order] >= 0) & (cls[order] < C)] if len(order) else order
    seg = np.zeros(C + 1, np.int32)
    seg[1:] = np.cumsum(np.bincount(cls[(cls >= 0) & (cls < C)].astype(int), minlength=C)[:C])
    return flags[order].astype(np.uint8), seg


def ap_rows_case(seed=11):
    """Rows for ssd_eval_ap_voc that no matching produced.  Class 0: 1500 rows (six chunks of the scan), rows 256 .. 767 of its
    sorted order ignored (two whole chunks); class 1: no row, with positives; class 2: 300 rows, all ignored; class 3: 40 rows,
    no positives; class 4: 700 rows whose precision rises late (the envelope reaches across chunks); class 5: one true
    positive.  Returns dict(rows=(cls, score, flags), n_pos i32 [C], C)."""
    rng = np.random.default_rng(seed)
    sizes = (1500, 0, 300, 40, 700, 1)
    cls = np.concatenate([np.full(n, c, np.int64) for c, n in enumerate(sizes)])
    N = len(cls)
    score = (np.round(rng.uniform(0, 1, N) * 200) / 200).astype(np.float32)          # many equal scores
    flags = (rng.random(N) < 0.45).astype(np.uint8)
    flags[rng.random(N) < 0.1] = 2
    flags[rng.random(N) < 0.02] = 3                                                   # both bits: ignored wins
    order0 = np.lexsort((np.arange(1500), -score[:1500].astype(np.float64)))
    flags[order0[256:768]] = 2
    flags[1500:1800] |= 2
    lo = 1840
    order4 = lo + np.lexsort((np.arange(700), -score[lo:lo + 700].astype(np.float64)))
    flags[order4[:300]] = (rng.random(300) < 0.1).astype(np.uint8)                    # poor precision first,
    flags[order4[300:]] = (rng.random(400) < 0.95).astype(np.uint8)                   # then nearly all right
    flags[-1] = 1
    n_pos = np.array([900, 5, 200, 0, 450, 3], np.int32)
    return dict(rows=(cls, score, flags), n_pos=n_pos, C=len(sizes))


def long_segment_case(n=2048 * 256 + 300 * 256 + 17, seed=13):
    """One class whose segment is longer than the slots of ssd_eval_ap_voc's year-12 pass hold one chunk each (2048 chunks of
    256 rows), with precision that rises again far behind: the envelope crosses slots and the chunks inside a slot."""
    rng = np.random.default_rng(seed)
    p = np.where((np.arange(n) // 40000) % 2 == 0, 0.2, 0.9)
    flags = (rng.random(n) < p).astype(np.uint8)
    flags[rng.random(n) < 0.05] = 2
    score = np.linspace(1.0, 0.0, n).astype(np.float32)              # non-increasing: the rows are in sorted order already
    return dict(rows=(np.zeros(n, np.int64), score, flags), n_pos=np.array([int((flags == 1).sum()) + 1000], np.int32), C=1)


# ---- a small VOCdevkit tree ----------------------------------------------------------------------------------------------------
VOC_NAMES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog", "horse",
             "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
# (year, set) -> image ids (JPEG fixtures of tests/golden/jpeg).  ALL_DIFFICULT: every object difficult; NO_OBJECT: none at all
DEVKIT = {("2007", "trainval"): ("c83x61_444", "c24x40_q100", "c83x61_420_rst", "c31x16_422", "c33x20_grey", "c8x8", "c83x61_422"),
          ("2012", "trainval"): ("c17x9_420", "c83x61_422", "c24x40_q1"),
          ("2007", "test"): ("c83x61_422", "c24x40_q1", "c33x20_grey", "c17x9_420", "c83x61_444")}
ALL_DIFFICULT = ("c33x20_grey",)
NO_OBJECT = ("c8x8",)


def devkit_objects(year, image_id):
    """[(name, xmin, ymin, xmax, ymax, difficult)] of an image: 1-based inclusive integer corners inside the image"""
    from tests import jpeg_cases as C
    if image_id in NO_OBJECT:
        return []
    h, w = C.decoded(image_id).shape[:2]
    rng = np.random.default_rng(int(year) * 1000 + sum(image_id.encode()))
    out = []
    for _ in range(int(rng.integers(2, 6))):
        x0, y0 = int(rng.integers(1, w)), int(rng.integers(1, h))
        x1, y1 = int(rng.integers(x0, w + 1)), int(rng.integers(y0, h + 1))
        out.append((VOC_NAMES[int(rng.integers(0, 20))], x0, y0, x1, y1, 1 if image_id in ALL_DIFFICULT or rng.random() < 0.3
                    else 0))
    if image_id not in ALL_DIFFICULT:
        out[0] = out[0][:5] + (0,)                                    # at least one object that is not difficult ...
        out[1] = out[1][:5] + (1,)                                    # ... and one that is
    return out


def build_devkit(root, missing=(), unknown=None, skip_sets=()):
    """writes VOC<year>/{ImageSets/Main/<set>.txt, Annotations/<id>.xml, JPEGImages/<id>.jpg} under root.  missing: image ids
    whose JPEG is left out; unknown: an image id one of whose objects gets a name that is no VOC class; skip_sets: (year, set)
    pairs whose list file is left out.  Returns {(year, set): [(id, objects)]} in list order."""
    import os
    from tests import jpeg_cases as C
    layout = {}
    for (year, name), ids in DEVKIT.items():
        base = os.path.join(str(root), "VOC" + year)
        for sub in ("ImageSets/Main", "Annotations", "JPEGImages"):
            os.makedirs(os.path.join(base, sub), exist_ok=True)
        if (year, name) not in skip_sets:
            with open(os.path.join(base, "ImageSets", "Main", name + ".txt"), "w") as f:
                f.write("".join("%s\n" % i for i in ids))
        layout[(year, name)] = []
        for image_id in ids:
            objs = devkit_objects(year, image_id)
            layout[(year, name)].append((image_id, objs))
            h, w = C.decoded(image_id).shape[:2]
            body = "".join("<object><name>%s</name><pose>Unspecified</pose><truncated>0</truncated><difficult>%d</difficult>"
                           "<bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax></bndbox></object>\n"
                           % (("gryphon" if unknown == image_id and k == 0 else o[0]), o[5], o[1], o[2], o[3], o[4])
                           for k, o in enumerate(objs))
            with open(os.path.join(base, "Annotations", image_id + ".xml"), "w") as f:
                f.write("<annotation><folder>VOC%s</folder><filename>%s.jpg</filename><size><width>%d</width><height>%d</height>"
                        "<depth>3</depth></size>\n%s</annotation>\n" % (year, image_id, w, h, body))
            if image_id not in missing:
                with open(os.path.join(base, "JPEGImages", image_id + ".jpg"), "wb") as f:
                    f.write(C.data(image_id))
    return layout
