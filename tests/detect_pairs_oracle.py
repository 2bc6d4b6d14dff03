"""Reference and input generators for the multi-label detection output (ops.detect_pairs).  A helper, not a test; plain numpy,
importable without a GPU.

pairs_reference restates steps 2-6 of the definition in include/ssd_hip.h on GIVEN float32 scores and boxes: candidates
p > thresh (no background test), order (score desc, anchor asc, class asc), the first max_cand take part, per-class greedy
suppression with oracle.ssd_oracle.iou_f32_rows, the kept pairs in the same order cut to keep_top_k, padding rows behind them.
Run on the device's own scores and boxes, every discrete result is compared bit for bit; float tolerance belongs to the
softmax and the decode alone."""
import numpy as np

from oracle import ssd_oracle as O

SMALL_GEOMETRY = dict(grids=((5, 5), (3, 3), (1, 1)), s_ref=(153, 207, 261, 315), ratios=((2, 3), (2,), (2,)))      # A = 190


def pairs_reference(prob, box, score_thresh, iou_thresh, max_cand, keep_top_k):
    """prob f32 [A,F], box f32 [A,4] (cx,cy,w,h) -> dict(n_cand, n_det, score f32 [K], cls i32 [K], anchor i32 [K],
    box f32 [K,4], valid u8 [K]) for one image."""
    prob = np.asarray(prob, np.float32)
    box = np.asarray(box, np.float32)
    a, c = np.nonzero(prob > np.float32(score_thresh))
    s = prob[a, c]
    order = np.lexsort((c, a, -s.astype(np.float64)))[:max_cand]
    thr = np.float32(iou_thresh)
    kept_of = {}
    rows = []
    for i in order:
        same = kept_of.setdefault(int(c[i]), [])
        if same and (O.iou_f32_rows(box[a[i]], box[same]) > thr).any():
            continue
        same.append(int(a[i]))
        rows.append(i)
    K = int(keep_top_k)
    rows = rows[:K]
    n = len(rows)
    out = dict(n_cand=int(a.size), n_det=n, score=np.zeros(K, np.float32), cls=np.full(K, -1, np.int32),
               anchor=np.full(K, -1, np.int32), box=np.zeros((K, 4), np.float32), valid=np.zeros(K, np.uint8))
    out["score"][:n], out["cls"][:n], out["anchor"][:n] = s[rows], c[rows], a[rows]
    out["box"][:n] = box[a[rows]]
    out["valid"][:n] = 1
    return out


def pairs_brute_force(prob, box, score_thresh, iou_thresh, max_cand, keep_top_k):
    """The same definition without lexsort or per-class lists: repeated selection of the best remaining pair, then a scan of
    ALL earlier participants.  O(n^2); returns [(score, class, anchor)] of the output rows."""
    prob = np.asarray(prob, np.float32)
    box = np.asarray(box, np.float32)
    A, F = prob.shape
    pairs = [(a, c) for a in range(A) for c in range(F) if prob[a, c] > np.float32(score_thresh)]
    chosen = []
    while pairs and len(chosen) < max_cand:
        best = pairs[0]
        for p in pairs[1:]:
            sb, sp = prob[best], prob[p]
            if sp > sb or (sp == sb and (p[0] < best[0] or (p[0] == best[0] and p[1] < best[1]))):
                best = p
        pairs.remove(best)
        chosen.append(best)
    kept = []
    for a, c in chosen:
        ok = True
        for ka, kc in kept:
            if kc == c and O.iou_f32_rows(box[a], box[ka][None])[0] > np.float32(iou_thresh):
                ok = False
        if ok:
            kept.append((a, c))
    return [(prob[a, c], c, a) for a, c in kept[:keep_top_k]]


def synth_logits2(B, A, C, n_hot, seed, per_anchor=2):
    """tests/test_detect_gpu.py's synth_logits (background-dominated logits, clusters of 8 boosted anchors among 40 neighbours)
    with `per_anchor` boosted classes per hot anchor: with two, many anchors pass a threshold under both of their classes."""
    rng = np.random.default_rng(seed)
    conf = rng.normal(0, 1, (B, A, C)).astype(np.float32)
    conf[..., C - 1] += 4.0
    span = min(40, A)
    for b in range(B):
        centres = rng.integers(0, max(A - span, 1), max(1, n_hot // 8))
        for c0 in centres:
            ks = rng.choice(C - 1, size=min(per_anchor, C - 1), replace=False)
            idx = c0 + rng.integers(0, span, 8)
            for k in ks:
                conf[b, idx, k] += rng.uniform(7, 11, 8).astype(np.float32)
    loc = rng.normal(0, 0.2, (B, A, 4)).astype(np.float32)
    return conf, loc


def add_score_ties(conf, first=5, last=400, step=3):
    """exact score ties: one hot row copied over many hot anchors (as test_nms_max_cand_cut_with_ties)"""
    for b in range(conf.shape[0]):
        hot = np.nonzero(conf[b, :, :-1].max(-1) > 8)[0]
        if hot.size > first:
            conf[b, hot[first:last:step]] = conf[b, hot[0]]
    return conf


def softmax_f32(conf):
    """float32 foreground probabilities from the float64 softmax (CPU stand-in for ops.class_scores in the CPU tests)"""
    return np.exp(O._log_softmax(conf))[..., :-1].astype(np.float32)
