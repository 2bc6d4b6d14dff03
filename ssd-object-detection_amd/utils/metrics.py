"""COCO-style mean average precision.

The reference fetches a validation split and drops it (models/ssd_model.py:291) and has no evaluation; this module is
build-defined, like the NMS it gives a consumer to.  It follows the published COCO protocol for boxes without crowd
regions: per class and per IoU threshold t in {0.50, 0.55, ..., 0.95}, detections are taken in order of decreasing score,
each claims the still-unmatched ground truth of its image with the highest IoU >= t, precision is made monotone from the
right and sampled at the 101 recall points 0, 0.01, ..., 1; AP = mean of the samples; mAP = mean over thresholds and over
the classes that have ground truth.  Boxes are (cx, cy, w, h) in any common unit; at most `max_dets` detections per image.

coco_summary (second half of the module) is the full protocol -- area ranges, crowd regions, average recall: COCO's twelve
columns -- and equals coco_map in mAP / AP50 / AP75 / per_class when no box is crowd.

voc_map (last part of the module) is PASCAL VOC's protocol instead: one IoU threshold, VOCdevkit's non-greedy matching with
`difficult` boxes, the 11-point AP of VOC2007 or the area under the envelope of VOC2010 onward."""
import numpy as np

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)
RECALL_POINTS = np.linspace(0.0, 1.0, 101)


def _corners(b):
    b = np.asarray(b, np.float64).reshape(-1, 4)
    return np.stack([b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2], 1)


def iou_matrix(a, b):
    """IoU of every box of a [n,4] with every box of b [m,4] (cx, cy, w, h) -> [n, m] float64."""
    ca, cb = _corners(a), _corners(b)
    lt = np.maximum(ca[:, None, :2], cb[None, :, :2])
    rb = np.minimum(ca[:, None, 2:], cb[None, :, 2:])
    wh = np.clip(rb - lt, 0.0, None)
    inter = wh[..., 0] * wh[..., 1]
    area_a = (ca[:, 2] - ca[:, 0]) * (ca[:, 3] - ca[:, 1])
    area_b = (cb[:, 2] - cb[:, 0]) * (cb[:, 3] - cb[:, 1])
    union = area_a[:, None] + area_b[None, :] - inter
    return np.where(union > 0, inter / np.maximum(union, 1e-300), 0.0)


def average_precision(scores, matched, n_gt):
    """AP (101-point) of one class at one threshold: scores [k], matched bool [k] (true positive flags), n_gt > 0."""
    if len(scores) == 0:
        return 0.0
    order = np.argsort(-np.asarray(scores, np.float64), kind="mergesort")
    tp = np.asarray(matched, bool)[order]
    ctp = np.cumsum(tp)
    cfp = np.cumsum(~tp)
    recall = ctp / float(n_gt)
    precision = ctp / np.maximum(ctp + cfp, 1)
    for i in range(len(precision) - 2, -1, -1):               # monotone envelope from the right
        precision[i] = max(precision[i], precision[i + 1])
    idx = np.searchsorted(recall, RECALL_POINTS, side="left")
    sampled = np.where(idx < len(precision), precision[np.minimum(idx, len(precision) - 1)], 0.0)
    return float(sampled.mean())


def ap_table_from_flags(rows, n_gt):
    """AP per (class, threshold) from matched rows -- the second stage of the device metric (ssd_eval_ap) on the host.
    rows = (cls [N], score [N], flags [N]): every detection that was scored, in (image, rank within image) order -- the
    order coco_map appends in -- with bit t of flags = true positive at IOU_THRESHOLDS[t] (ssd_eval_match's det_flags).
    n_gt: ground truths per class, a {class: count} mapping or a 1-D array indexed by class.
    Returns {class: [AP at each threshold]} for the classes with ground truth."""
    cls = np.asarray(rows[0]).astype(int).reshape(-1)
    score = np.asarray(rows[1], np.float64).reshape(-1)
    flags = np.asarray(rows[2]).astype(np.int64).reshape(-1) & 0xffff
    counts = dict(n_gt) if hasattr(n_gt, "items") else {c: int(n) for c, n in enumerate(np.asarray(n_gt).reshape(-1))}
    table = {}
    for c in sorted(int(c) for c, n in counts.items() if n > 0):
        sel = cls == c
        sc, fl = score[sel], flags[sel]                       # average_precision's stable sort keeps (image, rank) order
        table[c] = [average_precision(sc, (fl >> ti) & 1, counts[c]) for ti in range(len(IOU_THRESHOLDS))]
    return table


def map_from_ap_table(table):
    """coco_map's result dict from {class: [AP per threshold]} (classes with ground truth only)."""
    if not table:
        return dict(mAP=0.0, AP50=0.0, AP75=0.0, per_class={})
    classes = sorted(table)
    per_class = {c: float(np.mean(table[c])) for c in classes}
    return dict(mAP=float(np.mean(list(per_class.values()))), AP50=float(np.mean([table[c][0] for c in classes])),
                AP75=float(np.mean([table[c][5] for c in classes])), per_class=per_class)


def map_from_flags(rows, n_gt):
    """coco_map's result from rows that are already matched (see ap_table_from_flags): equal to coco_map on the same
    detections when the flags are its greedy matches."""
    return map_from_ap_table(ap_table_from_flags(rows, n_gt))


def coco_map(detections, ground_truths, max_dets=100):
    """detections: per image (score [k], cls [k], box [k,4]); ground_truths: per image (cls [n], box [n,4]).
    Returns dict(mAP=..., AP50=..., AP75=..., per_class={cls: AP@[.5:.95]})."""
    per_class_dets, per_class_ngt = {}, {}
    for img, (gcls, gbox) in enumerate(ground_truths):
        for c in np.asarray(gcls).astype(int):
            per_class_ngt[c] = per_class_ngt.get(c, 0) + 1
    ap = {}                                                   # (cls, threshold index) -> AP
    classes = sorted(per_class_ngt)
    flags = {c: [[] for _ in IOU_THRESHOLDS] for c in classes}
    scores = {c: [] for c in classes}
    for img, (dscore, dcls, dbox) in enumerate(detections):
        dscore = np.asarray(dscore, np.float64)
        dcls = np.asarray(dcls).astype(int)
        dbox = np.asarray(dbox, np.float64).reshape(-1, 4)
        keep = np.argsort(-dscore, kind="mergesort")[:max_dets]
        dscore, dcls, dbox = dscore[keep], dcls[keep], dbox[keep]
        gcls = np.asarray(ground_truths[img][0]).astype(int)
        gbox = np.asarray(ground_truths[img][1], np.float64).reshape(-1, 4)
        for c in np.unique(dcls):
            if c not in per_class_ngt:
                continue                                      # class without ground truth anywhere: not part of the mean
            d_idx = np.nonzero(dcls == c)[0]
            g_idx = np.nonzero(gcls == c)[0]
            iou = iou_matrix(dbox[d_idx], gbox[g_idx]) if len(g_idx) else np.zeros((len(d_idx), 0))
            scores[c].extend(dscore[d_idx].tolist())
            for ti, thr in enumerate(IOU_THRESHOLDS):
                taken = np.zeros(len(g_idx), bool)
                for k in range(len(d_idx)):                   # already in decreasing score order
                    best, best_j = thr, -1
                    for j in range(len(g_idx)):
                        if not taken[j] and iou[k, j] >= best:
                            best, best_j = iou[k, j], j
                    if best_j >= 0:
                        taken[best_j] = True
                    flags[c][ti].append(best_j >= 0)
    per_class = {}
    ap50, ap75 = [], []
    for c in classes:
        aps = [average_precision(scores[c], flags[c][ti], per_class_ngt[c]) for ti in range(len(IOU_THRESHOLDS))]
        per_class[c] = float(np.mean(aps))
        ap50.append(aps[0])
        ap75.append(aps[5])
    if not classes:
        return dict(mAP=0.0, AP50=0.0, AP75=0.0, per_class={})
    return dict(mAP=float(np.mean(list(per_class.values()))), AP50=float(np.mean(ap50)), AP75=float(np.mean(ap75)),
                per_class=per_class)


# ------------------------------------------------------------------------------------------------------------------------
# The full COCO box protocol: area ranges, crowd boxes, average recall
# ------------------------------------------------------------------------------------------------------------------------
COCO_AREA_RANGES = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))
COCO_AREA_NAMES = ("all", "small", "medium", "large")
COCO_SUMMARY_KEYS = ("mAP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "AR100", "AR_small",
                     "AR_medium", "AR_large")


def iou_matrix_crowd(a, b, crowd):
    """iou_matrix with COCO's crowd form in the columns where `crowd` [m] is set: intersection / area of the detection
    (the corner-form area iou_matrix computes), 0 where that area is not positive."""
    iou = iou_matrix(a, b)
    crowd = np.asarray(crowd, bool).reshape(-1)
    if not crowd.any():
        return iou
    ca, cb = _corners(a), _corners(b)
    lt = np.maximum(ca[:, None, :2], cb[None, :, :2])
    rb = np.minimum(ca[:, None, 2:], cb[None, :, 2:])
    wh = np.clip(rb - lt, 0.0, None)
    inter = wh[..., 0] * wh[..., 1]
    area_a = ((ca[:, 2] - ca[:, 0]) * (ca[:, 3] - ca[:, 1]))[:, None]
    ioa = np.where(area_a > 0, inter / np.maximum(area_a, 1e-300), 0.0)
    return np.where(crowd[None, :], ioa, iou)


def coco_match_image(dscore, dcls, dbox, gcls, gbox, gcrowd=None, max_dets=100, area_ranges=COCO_AREA_RANGES, scale=1.0,
                     census=None):
    """Steps 1-6 of coco_summary for one image (what ssd_eval_match_coco computes).  Returns (score [k], cls [k], box [k,4],
    tp u16 [k,4], ig u16 [k,4], pos i32 [k], gt_ignore u8 [n]) for the first max_dets detections by (score desc, index asc):
    bit t of tp[r, a] = true positive at IOU_THRESHOLDS[t] in area range a, bit t of ig[r, a] = ignored there, bit a of
    gt_ignore[j] = ground truth j ignored in range a.  census: a dict that receives counts of the protocol's events
    (crowd_rematch, ignored_match, unmatched_out_of_range, iou_tie, boundary_area)."""
    dscore, dcls, dbox = np.asarray(dscore), np.asarray(dcls).astype(int), np.asarray(dbox).reshape(-1, 4)
    keep = np.argsort(-dscore.astype(np.float64), kind="mergesort")[:max_dets]
    dscore, dcls, dbox = dscore[keep], dcls[keep], dbox[keep]
    gcls = np.asarray(gcls).astype(int).reshape(-1)
    gbox = np.asarray(gbox, np.float64).reshape(-1, 4)
    n, k = len(gcls), len(dscore)
    crowd = np.zeros(n, bool) if gcrowd is None else np.asarray(gcrowd).astype(bool).reshape(-1)
    scale = np.float64(scale)
    b64 = dbox.astype(np.float64)
    darea = b64[:, 2] * b64[:, 3] * scale
    garea = gbox[:, 2] * gbox[:, 3] * scale
    n_a = len(area_ranges)
    gt_ignore = np.zeros(n, np.uint8)
    for a, (lo, hi) in enumerate(area_ranges):
        ign = crowd | (garea < lo) | (garea > hi)
        gt_ignore |= (ign.astype(np.uint8) << a).astype(np.uint8)
        if census is not None:
            census["boundary_area"] = census.get("boundary_area", 0) + int(((garea == lo) | (garea == hi)).sum())
    tp = np.zeros((k, n_a), np.uint16)
    ig = np.zeros((k, n_a), np.uint16)
    pos = np.zeros(k, np.int32)
    for c in np.unique(dcls):
        d_idx = np.nonzero(dcls == c)[0]
        g_idx = np.nonzero(gcls == c)[0]
        pos[d_idx] = np.arange(len(d_idx))
        iou = iou_matrix_crowd(b64[d_idx], gbox[g_idx], crowd[g_idx]) if len(g_idx) else np.zeros((len(d_idx), 0))
        for a, (lo, hi) in enumerate(area_ranges):
            g_ign = ((gt_ignore[g_idx] >> a) & 1).astype(bool)
            for ti, thr in enumerate(IOU_THRESHOLDS):
                taken = np.zeros(len(g_idx), bool)
                for r, d in enumerate(d_idx):
                    best, bj, tie = thr, -1, False
                    for j in range(len(g_idx)):                               # the non-ignored ground truths first
                        if not g_ign[j] and not taken[j] and iou[r, j] >= best:
                            tie = bj >= 0 and iou[r, j] == best
                            best, bj = iou[r, j], j
                    if bj < 0:                                                # only otherwise the ignored ones
                        best = thr
                        for j in range(len(g_idx)):
                            if g_ign[j] and (not taken[j] or crowd[g_idx[j]]) and iou[r, j] >= best:
                                tie = bj >= 0 and iou[r, j] == best
                                best, bj = iou[r, j], j
                    if bj >= 0:
                        if census is not None:
                            census["crowd_rematch"] = census.get("crowd_rematch", 0) + int(taken[bj])
                            census["ignored_match"] = census.get("ignored_match", 0) + int(g_ign[bj])
                            census["iou_tie"] = census.get("iou_tie", 0) + int(tie)
                        taken[bj] = True
                        tp[d, a] |= np.uint16(1 << ti)
                        if g_ign[bj]:
                            ig[d, a] |= np.uint16(1 << ti)
                    elif darea[d] < lo or darea[d] > hi:
                        ig[d, a] |= np.uint16(1 << ti)
                        if census is not None:
                            census["unmatched_out_of_range"] = census.get("unmatched_out_of_range", 0) + 1
    return dscore, dcls, dbox, tp, ig, pos, gt_ignore


def coco_tables_from_rows(rows, n_gt, max_dets=100):
    """AP and true-positive counts from matched rows -- the second stage of the device metric (ssd_eval_ap_coco) on the host.
    rows = (cls [N], score [N], tp [N,4], ig [N,4], pos [N]) in (image, rank) order; n_gt int [4, C]: non-ignored ground
    truths per (area range, class).  Returns (ap f64 [C,4,10], tp_count i32 [C,4,3,10]); classes without ground truth in a
    range hold zeros there.  tp_count[c, a, m, t]: true positives not ignored with pos < (1, 10, max_dets)[m]."""
    cls = np.asarray(rows[0]).astype(int).reshape(-1)
    score = np.asarray(rows[1], np.float64).reshape(-1)
    tp = np.asarray(rows[2]).astype(np.int64).reshape(-1, 4) & 0xffff
    ig = np.asarray(rows[3]).astype(np.int64).reshape(-1, 4) & 0xffff
    pos = np.asarray(rows[4]).astype(np.int64).reshape(-1)
    n_gt = np.asarray(n_gt).astype(np.int64)
    C = n_gt.shape[1]
    ap = np.zeros((C, 4, len(IOU_THRESHOLDS)), np.float64)
    cnt = np.zeros((C, 4, 3, len(IOU_THRESHOLDS)), np.int32)
    for c in range(C):
        sel = cls == c
        for a in range(4):
            if n_gt[a, c] <= 0:
                continue
            for ti in range(len(IOU_THRESHOLDS)):
                live = ((ig[sel, a] >> ti) & 1) == 0
                hit = (((tp[sel, a] >> ti) & 1) == 1) & live
                ap[c, a, ti] = average_precision(score[sel][live], hit[live], int(n_gt[a, c]))
                for m, lim in enumerate((1, 10, max_dets)):
                    cnt[c, a, m, ti] = int((hit & (pos[sel] < lim)).sum())
    return ap, cnt


def coco_summary_from_tables(ap, tp_count, n_gt):
    """coco_summary's result from ap [C,4,10], tp_count [C,4,3,10] and n_gt [4,C] (see coco_tables_from_rows): shared by the
    host and the device metric, so that both sum in the same order."""
    ap, tp_count, n_gt = np.asarray(ap, np.float64), np.asarray(tp_count), np.asarray(n_gt).astype(np.int64)
    C = n_gt.shape[1]
    live = [[c for c in range(C) if n_gt[a, c] > 0] for a in range(4)]
    out = map_from_ap_table({c: ap[c, 0].tolist() for c in live[0]})

    def mean_ap(a):
        return float(np.mean([float(np.mean(ap[c, a].tolist())) for c in live[a]])) if live[a] else -1.0

    def mean_ar(a, m):
        if not live[a]:
            return -1.0
        return float(np.mean([float(np.mean((tp_count[c, a, m].astype(np.float64) / float(n_gt[a, c])).tolist()))
                              for c in live[a]]))

    out["AP_small"], out["AP_medium"], out["AP_large"] = mean_ap(1), mean_ap(2), mean_ap(3)
    out["AR1"], out["AR10"], out["AR100"] = mean_ar(0, 0), mean_ar(0, 1), mean_ar(0, 2)
    out["AR_small"], out["AR_medium"], out["AR_large"] = mean_ar(1, 2), mean_ar(2, 2), mean_ar(3, 2)
    out["per_class_area"] = {COCO_AREA_NAMES[a]: {c: float(np.mean(ap[c, a].tolist())) for c in live[a]} for a in range(4)}
    return out


def coco_summary(detections, ground_truths, max_dets=100, area_ranges=COCO_AREA_RANGES, area_scale=None):
    """COCO's twelve box metrics: a plain numpy restatement of COCOeval's published box procedure.  pycocotools is not a
    dependency and was not available to compare against, so this oracle is unpinned: it follows the published description,
    not a run of that code.

    detections: per image (score [k], cls [k], box [k,4]); ground_truths: per image (cls [n], box [n,4][, crowd bool [n]]);
    boxes (cx, cy, w, h) in evaluation pixels.  area_scale[i] (float64, 1 when absent) = (source width x source height) /
    (S x S) of image i, which turns evaluation-pixel areas into source-pixel areas.  area_ranges: four (lo, hi) pairs named
    all / small / medium / large.

    Per image the first max_dets detections by (score desc, index asc) are scored; per class and area range a:
    the area of a box is float64(w) * float64(h) * area_scale[i] -- there are no segmentation masks here, so the box area
    stands in for COCO's `area`; a ground truth is ignored in a when it is crowd or its area is < lo or > hi (bounds
    inclusive: a box on a boundary belongs to both ranges); IoU is iou_matrix, against a crowd box intersection / detection
    area; per threshold the class's detections, in list order, each take the unclaimed non-ignored ground truth of highest
    IoU >= t (last index among equals), and only when there is none an ignored one by the same rule, where a crowd box may
    be claimed again; a matched detection is a true positive and inherits the ignore flag of its match, an unmatched one
    whose own area lies outside a is ignored.  AP(class, a, t) is average_precision over the rows not ignored with n_gt = the
    non-ignored ground truths of (class, a); Recall(class, a, m, t) = true positives not ignored among the first m
    detections of their (image, class) / n_gt -- the matches of a prefix do not depend on what follows, so AR1 and AR10 come
    from the same pass.  Classes with n_gt == 0 are left out of a column; a column with no class left is -1.0.

    Returns dict(mAP, AP50, AP75, per_class: as coco_map over range "all" (bit for bit its values when no box is crowd);
    AP_small, AP_medium, AP_large; AR1, AR10, AR100 (range all; AR100 is at max_dets); AR_small, AR_medium, AR_large (at
    max_dets); per_class_area = {range name: {class: AP}})."""
    assert len(area_ranges) == 4
    classes = set()
    for g in ground_truths:
        classes.update(int(c) for c in np.asarray(g[0]).astype(int).reshape(-1))
    C = max(classes) + 1 if classes and max(classes) >= 0 else 0
    n_gt = np.zeros((4, max(C, 1)), np.int64)
    cls_rows, score_rows, tp_rows, ig_rows, pos_rows = [], [], [], [], []
    for i, (dscore, dcls, dbox) in enumerate(detections):
        g = ground_truths[i]
        scale = 1.0 if area_scale is None else area_scale[i]
        s, c, _, tp, ig, pos, gi = coco_match_image(dscore, dcls, dbox, g[0], g[1], g[2] if len(g) > 2 else None, max_dets,
                                                    area_ranges, scale)
        gc = np.asarray(g[0]).astype(int).reshape(-1)
        for a in range(4):
            for cc in gc[((gi >> a) & 1) == 0]:
                if 0 <= cc < C:
                    n_gt[a, cc] += 1
        cls_rows.append(c); score_rows.append(s); tp_rows.append(tp); ig_rows.append(ig); pos_rows.append(pos)
    if not detections:
        cls_rows, score_rows, pos_rows = [np.zeros(0, int)], [np.zeros(0)], [np.zeros(0, np.int32)]
        tp_rows, ig_rows = [np.zeros((0, 4), np.uint16)], [np.zeros((0, 4), np.uint16)]
    rows = (np.concatenate(cls_rows), np.concatenate(score_rows), np.concatenate(tp_rows), np.concatenate(ig_rows),
            np.concatenate(pos_rows))
    ap, cnt = coco_tables_from_rows(rows, n_gt, max_dets)
    return coco_summary_from_tables(ap, cnt, n_gt)


# ------------------------------------------------------------------------------------------------------------------------
# PASCAL VOC: VOCdevkit's VOCevaldet
# ------------------------------------------------------------------------------------------------------------------------
VOC_RECALL_POINTS = np.arange(11) / 10.0           # not linspace(0, 1, 11) / arange(0, 1.1, 0.1): those hold 0.30000000000000004
VOC_YEARS = {"07": 7, "12": 12, 7: 7, 12: 12}


def voc_match_image(dscore, dcls, dbox, gcls, gbox, gdifficult=None, iou_thresh=0.5, max_dets=100):
    """The per-image stage of voc_map (what ssd_eval_match_voc computes).  Returns (score [k], cls [k], box [k,4], tp bool [k],
    ignored bool [k], gt i32 [k]) for the first max_dets detections by (score desc, index asc): gt = jmax as an index into the
    image's boxes, -1 when ovmax < iou_thresh (or the class has no box in the image)."""
    dscore, dcls, dbox = np.asarray(dscore), np.asarray(dcls).astype(int), np.asarray(dbox).reshape(-1, 4)
    keep = np.argsort(-dscore.astype(np.float64), kind="mergesort")[:max_dets]
    dscore, dcls, dbox = dscore[keep], dcls[keep], dbox[keep]
    gcls = np.asarray(gcls).astype(int).reshape(-1)
    gbox = np.asarray(gbox, np.float64).reshape(-1, 4)
    hard = np.zeros(len(gcls), bool) if gdifficult is None else np.asarray(gdifficult).astype(bool).reshape(-1)
    k = len(dscore)
    tp, ignored, gt = np.zeros(k, bool), np.zeros(k, bool), np.full(k, -1, np.int32)
    b64 = dbox.astype(np.float64)
    claimed = np.zeros(len(gcls), bool)
    for r in range(k):                                                # already in decreasing score order
        g_idx = np.nonzero(gcls == dcls[r])[0]
        if not len(g_idx):
            continue
        iou = iou_matrix(b64[r:r + 1], gbox[g_idx])[0]
        j = int(np.argmax(iou))                                       # the first index attaining ovmax
        if not iou[j] >= iou_thresh:
            continue
        gt[r] = g_idx[j]
        if hard[g_idx[j]]:
            ignored[r] = True
        elif not claimed[g_idx[j]]:
            tp[r] = claimed[g_idx[j]] = True
    return dscore, dcls, dbox, tp, ignored, gt


def voc_ap_from_rows(rows, n_pos, year="07"):
    """AP per class from matched rows -- the second stage of the device metric (ssd_eval_ap_voc) on the host.
    rows = (cls [N], score [N], flags [N]) in (image, rank) order, bit 0 of flags = true positive, bit 1 = ignored (such a row
    counts as neither; it wins over bit 0); n_pos: non-difficult boxes per class, a {class: count} mapping or a 1-D array.
    Returns {class: AP} for the classes with n_pos > 0."""
    if year not in VOC_YEARS:
        raise ValueError("year must be '07' or '12', not %r" % (year,))
    year = VOC_YEARS[year]
    cls = np.asarray(rows[0]).astype(int).reshape(-1)
    score = np.asarray(rows[1], np.float64).reshape(-1)
    flags = np.asarray(rows[2]).astype(np.int64).reshape(-1)
    counts = dict(n_pos) if hasattr(n_pos, "items") else {c: int(n) for c, n in enumerate(np.asarray(n_pos).reshape(-1))}
    out = {}
    for c in sorted(int(c) for c, n in counts.items() if n > 0):
        sel = cls == c
        order = np.argsort(-score[sel], kind="mergesort")             # stable: keeps (image, rank) among equal scores
        fl = flags[sel][order]
        ign = (fl & 2) != 0
        ctp = np.cumsum(((fl & 1) != 0) & ~ign)
        cfp = np.cumsum(((fl & 1) == 0) & ~ign)
        recall = ctp / float(counts[c])
        precision = ctp / np.maximum(ctp + cfp, 1)
        if year == 7:
            ap = 0.0
            for t in VOC_RECALL_POINTS:
                reached = recall >= t
                ap += float(precision[reached].max()) if reached.any() else 0.0
            out[c] = ap / 11.0
            continue
        mrec = np.concatenate([[0.0], recall, [1.0]])
        mpre = np.concatenate([[0.0], precision, [0.0]])
        mpre = np.maximum.accumulate(mpre[::-1])[::-1]                # monotone from the right
        ap = 0.0
        for i in np.nonzero(mrec[1:] != mrec[:-1])[0]:
            ap += float((mrec[i + 1] - mrec[i]) * mpre[i + 1])
        out[c] = ap
    return out


def voc_result(per_class, n_pos):
    """voc_map's result dict from {class: AP} and the per-class counts of non-difficult boxes."""
    per_class = {int(c): float(v) for c, v in sorted(per_class.items())}
    mean = 0.0
    for v in per_class.values():
        mean += v
    return dict(mAP=mean / len(per_class) if per_class else 0.0, per_class=per_class,
                n_pos={int(c): int(n) for c, n in sorted(dict(n_pos).items())})


def voc_map(detections, ground_truths, year="07", iou_thresh=0.5, max_dets=100):
    """PASCAL VOC detection mAP: a plain numpy restatement of the published VOCdevkit procedure (VOCevaldet).  The devkit was
    not available to compare against, so this definition is unpinned: it follows the published description, not a run of that
    code.

    detections: per image (score [k], cls [k], box [k,4]), as for coco_map; ground_truths: per image (cls [n], box [n,4][,
    difficult bool [n]]); boxes (cx, cy, w, h) in any common unit.  Returns dict(mAP, per_class={cls: AP}, n_pos={cls: count}).

    Per image the first max_dets detections by (score desc, index asc) are scored.  Per detection, among ALL boxes of its class
    in its image -- claimed or not, difficult ones included -- ovmax is the highest IoU and jmax the first index attaining it.
    IoU is iou_matrix: float64 over continuous coordinates.  VOCdevkit's `+1` pixel convention (widths as xmax - xmin + 1 of
    integer pixel indices) is NOT applied, because boxes here live in network-input coordinates, not on a pixel grid.  When
    ovmax >= iou_thresh (inclusive, as the devkit's): the detection is ignored if box jmax is difficult; else a true positive
    if no earlier detection of the image has the same jmax with its own ovmax >= iou_thresh; else a false positive -- a
    duplicate, even where a second box would also pass, which is where this differs from coco_map's greedy rule.  Otherwise
    it is a false positive.  n_pos[c] counts the non-difficult boxes of class c; classes with n_pos == 0 are left out of the
    mean and of per_class.  Per class the rows are sorted by (score desc, image asc, rank asc); ignored rows add to neither
    count; recall = ctp / n_pos, precision = ctp / max(ctp + cfp, 1).
    year="07": AP = (sum over k = 0..10, in that order, of max{precision[i] : recall[i] >= k / 10.0}, 0 where none) / 11.0.
    year="12": mrec = [0, recall, 1], mpre = [0, precision, 0] made monotone from the right; AP = the sum in index order of
    (mrec[i+1] - mrec[i]) * mpre[i+1] where mrec[i+1] != mrec[i].  mAP sums the classes in ascending order."""
    if year not in VOC_YEARS:
        raise ValueError("year must be '07' or '12', not %r" % (year,))
    if not (np.isfinite(iou_thresh) and iou_thresh > 0):
        raise ValueError("iou_thresh must be finite and > 0, not %r" % (iou_thresh,))
    n_pos = {}
    for g in ground_truths:
        gc = np.asarray(g[0]).astype(int).reshape(-1)
        hard = np.zeros(len(gc), bool) if len(g) < 3 or g[2] is None else np.asarray(g[2]).astype(bool).reshape(-1)
        for c in gc[~hard]:
            n_pos[int(c)] = n_pos.get(int(c), 0) + 1
    cls_rows, score_rows, flag_rows = [np.zeros(0, int)], [np.zeros(0)], [np.zeros(0, np.uint8)]
    for i, (dscore, dcls, dbox) in enumerate(detections):
        g = ground_truths[i]
        s, c, _, tp, ign, _ = voc_match_image(dscore, dcls, dbox, g[0], g[1], g[2] if len(g) > 2 else None, iou_thresh, max_dets)
        cls_rows.append(c); score_rows.append(s); flag_rows.append(tp.astype(np.uint8) | (ign.astype(np.uint8) << 1))
    rows = (np.concatenate(cls_rows), np.concatenate(score_rows), np.concatenate(flag_rows))
    return voc_result(voc_ap_from_rows(rows, n_pos, year), n_pos)
