"""Float64 numpy evaluation of the SSD paper's MultiBox loss as include/ssd_hip.h defines ssd_multibox_loss_fwd_bwd
(Liu et al. 2016, eq. 1-3; mining key and per-image rule of ssd.pytorch's MultiBoxLoss).  Plain numpy: runs without a GPU.

  CE(a, c) = logsumexp(conf[a]) - conf[a, c];  key(a) = CE(a, C-1)
  image b: P_b positives, candidates = the other anchors, k_b = min(ratio * P_b, A - P_b); k_b == 0 mines nothing, else
           tau_b = k_b-th largest candidate key, neg_b = candidates with key >= tau_b (ties kept)
  P = sum P_b, N = sum |neg_b|
  pos = sum_pos CE(a, gt_cls) / P;  neg = sum_neg key / P;  loc = alpha * sum_pos sum_4 smoothL1(loc - gt_loc) / P
  dcls = [pos * (softmax - onehot(gt_cls)) + neg * (softmax - onehot(C-1))] / P;  dbox = alpha * pos * clamp(d, -1, 1) / P
"""
import numpy as np


def log_softmax(conf):
    z = np.asarray(conf, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(-1, keepdims=True)))


def keys(conf):
    """float64 mining key of every anchor: the background cross entropy"""
    return -log_softmax(conf)[..., -1]


def smooth_l1(d):
    a = np.abs(d)
    return np.where(a < 1.0, 0.5 * d * d, a - 0.5)


def select(key, mask, ratio=3):
    """(tau f64[B] (nan where the image mined nothing), neg_mask bool[B,A]) from keys [B,A] and positives [B,A]"""
    key = np.asarray(key, dtype=np.float64)
    mask = np.asarray(mask).astype(bool)
    B, A = key.shape
    tau = np.full(B, np.nan)
    neg = np.zeros((B, A), dtype=bool)
    for b in range(B):
        P_b = int(mask[b].sum())
        k_b = min(int(ratio) * P_b, A - P_b)
        if k_b == 0:
            continue
        cand = np.sort(key[b][~mask[b]])[::-1]
        tau[b] = cand[k_b - 1]
        neg[b] = ~mask[b] & (key[b] >= tau[b])
    return tau, neg


def multibox_loss(gt_cls, gt_loc, gt_mask, loc, conf, neg_pos_ratio=3, loc_weight=1.0, grad_scale=1.0):
    """All arrays [B, A, ...].  Returns a dict: loc, pos, neg, total, num_pos, num_neg, tau [B], neg_mask [B,A], key [B,A],
    dcls [B,A,C], dbox [B,A,4] (the gradients of grad_scale * total), status (0, or 1 when there is no positive)."""
    conf = np.asarray(conf, dtype=np.float64)
    loc = np.asarray(loc, dtype=np.float64)
    gt_loc = np.asarray(gt_loc, dtype=np.float64)
    mask = np.asarray(gt_mask).astype(bool)
    gt_cls = np.asarray(gt_cls).astype(np.int64)
    B, A, C = conf.shape
    logp = log_softmax(conf)
    key = -logp[..., -1]
    tau, neg = select(key, mask, neg_pos_ratio)
    P, N = int(mask.sum()), int(neg.sum())
    out = dict(num_pos=P, num_neg=N, tau=tau, neg_mask=neg, key=key, status=0 if P else 1,
               dcls=np.zeros((B, A, C)), dbox=np.zeros((B, A, 4)), loc=0.0, pos=0.0, neg=0.0, total=0.0)
    if P == 0:
        return out
    ce_lab = -np.take_along_axis(logp, np.where(mask, gt_cls, 0)[..., None], -1)[..., 0]
    d = loc - gt_loc
    out["pos"] = float(ce_lab[mask].sum() / P)
    out["neg"] = float(key[neg].sum() / P)
    out["loc"] = float(loc_weight * smooth_l1(d[mask]).sum() / P)
    out["total"] = out["loc"] + out["pos"] + out["neg"]
    p = np.exp(logp)
    onehot_lab = np.zeros((B, A, C))
    np.put_along_axis(onehot_lab, np.where(mask, gt_cls, 0)[..., None], 1.0, -1)
    onehot_bg = np.zeros((B, A, C))
    onehot_bg[..., -1] = 1.0
    out["dcls"] = grad_scale / P * (mask[..., None] * (p - onehot_lab) + neg[..., None] * (p - onehot_bg))
    out["dbox"] = grad_scale * loc_weight / P * mask[..., None] * np.clip(d, -1.0, 1.0)
    return out
