"""Float64 numpy definition of the softmax focal loss (include/ssd_hip.h, ssd_softmax_focal_loss_fwd_bwd) in its stable forms.

Per anchor, with the target t (gt_cls where gt_mask, the background C-1 elsewhere), m = max_j z_j, e_j = exp(z_j - m):
    Q = sum_{j != t} e_j,  S = Q + e_t,  q = Q / S (= 1 - p_t, never formed as that difference),  p_j = e_j / S
    log p_t = log1p(-q) where q < 0.5, (z_t - m) - log S elsewhere
    FL = -alpha_t q^gamma log p_t;   alpha_t = alpha for t != C-1, 1 - alpha for the background, 1 everywhere with alpha == -1
    dFL/dz_j = alpha_t (delta_tj - p_j) (gamma p_t q^(gamma-1) log p_t - q^gamma)
             = alpha_t (delta_tj - p_j) * -(q^gamma (gamma p_t h + 1)),  h = -log p_t / q  (h = 1 at q == 0: finite there),
    with delta_tt - p_t taken as q.
rows() evaluates this in any float dtype and, for the tests that show the stable forms are needed, in two naive variants."""
import numpy as np


def rows(z, t, gamma, alpha, dtype=np.float64, variant="stable"):
    """z [n, C], t [n] -> (FL [n], dFL/dz [n, C], q [n]), every operation in `dtype`.
    variant "stable": the forms above; "one_minus_pt": q = 1 - p_t; "lse": log p_t = z_t - logsumexp(z)."""
    z = np.asarray(z, dtype=dtype)
    n, C = z.shape
    idx = np.arange(n)
    g, one = dtype(gamma), dtype(1.0)
    m = z.max(axis=1)
    e = np.exp(z - m[:, None])
    et = e[idx, t]
    rest = e.copy()
    rest[idx, t] = 0
    Q = rest.sum(axis=1, dtype=dtype)
    S = Q + et
    pt = et / S
    zt = z[idx, t]
    q = Q / S if variant != "one_minus_pt" else one - pt
    if variant == "lse":
        logpt = zt - (m + np.log(S))
    else:
        with np.errstate(divide="ignore"):                               # (log1p(-1) on rows that take the other branch)
            logpt = np.where(q < dtype(0.5), np.log1p(-q), (zt - m) - np.log(S))
    qg = np.power(q, g)                                                   # (0 ** 0 == 1)
    h = np.where(q > 0, -logpt / np.where(q > 0, q, one), one)
    if alpha == -1:
        alpha_t = np.ones(n, dtype=dtype)
    else:
        alpha_t = np.where(t != C - 1, dtype(alpha), one - dtype(alpha)).astype(dtype)
    coef = alpha_t * -(qg * (g * pt * h + one))
    d = -(e / S[:, None])
    d[idx, t] = q
    return (-alpha_t * qg * logpt).astype(dtype), (coef[:, None] * d).astype(dtype), q.astype(dtype)


def smooth_l1(d):
    a = np.abs(d)
    return np.where(a < 1.0, 0.5 * d * d, a - 0.5)


def softmax_focal_loss(gt_cls, gt_loc, gt_mask, loc, conf, gamma=2.0, alpha=0.25, loc_weight=1.0, grad_scale=1.0):
    """gt_cls [B,A] int, gt_loc [B,A,4], gt_mask [B,A] bool, loc [B,A,4], conf [B,A,C] -> dict: the scalars loc / pos / neg /
    total, num_pos, num_neg = B*A - P, dcls [B,A,C], dbox [B,A,4] (float64), status (0; 1: no positive, everything 0;
    3: a logit, or an offset of a positive, is not finite -- reported first) and the per-anchor q [B,A]."""
    conf = np.asarray(conf, np.float64)
    loc, gt_loc = np.asarray(loc, np.float64), np.asarray(gt_loc, np.float64)
    mask = np.asarray(gt_mask).astype(bool)
    B, A, C = conf.shape
    P = int(mask.sum())
    bad = not (np.isfinite(conf).all() and np.isfinite(loc[mask]).all() and np.isfinite(gt_loc[mask]).all())
    out = dict(num_pos=P, num_neg=B * A - P, status=3 if bad else (1 if P == 0 else 0))
    if P == 0 or bad:
        zero = 0.0 if not bad else np.nan
        out.update(loc=zero, pos=zero, neg=zero, total=zero, dcls=np.full(conf.shape, zero), dbox=np.full(loc.shape, zero),
                   q=np.full((B, A), zero))
        return out
    t = np.where(mask, np.asarray(gt_cls), C - 1).reshape(-1).astype(np.int64)
    fl, dz, q = rows(conf.reshape(-1, C), t, gamma, alpha)
    flat = mask.reshape(-1)
    d = loc - gt_loc
    l_pos, l_neg = fl[flat].sum() / P, fl[~flat].sum() / P
    l_loc = loc_weight * smooth_l1(d)[mask].sum() / P
    out.update(loc=l_loc, pos=l_pos, neg=l_neg, total=(l_loc + l_pos) + l_neg,
               dcls=(grad_scale / P) * dz.reshape(B, A, C),
               dbox=(grad_scale * loc_weight / P) * mask[..., None] * np.clip(d, -1.0, 1.0), q=q.reshape(B, A))
    return out
