"""Numpy definition of the IoU box terms (include/ssd_hip.h, the _box entries of the MultiBox and softmax focal losses): GIoU,
DIoU and CIoU of one positive's decoded boxes with the analytic gradient, in float64 or -- the f32 restatement -- in any float
dtype, and full-loss wrappers that take the classification part from tests/multibox_oracle.py / softmax_focal_oracle.py.

Per positive, prior size (d_w, d_h), prediction t, target g, W = log(1000 / 16); both boxes relative to the prior's centre:
    cx = t0 d_w, cy = t1 d_h, w = d_w exp(clamp(t2, -W, W)), h = d_h exp(clamp(t3, -W, W));  (gx, gy, gw, gh) from g alike
    x1 = cx - w/2, x2 = cx + w/2, ...;  X1 = gx - gw/2, ...
    iw = max(0, min(x2, X2) - max(x1, X1)), ih alike;  I = iw ih;  U = w h + gw gh - I;  IoU = I / U
    cw = max(x2, X2) - min(x1, X1), ch alike
    giou: L = 1 - IoU + (cw ch - U) / (cw ch)
    diou: L = 1 - IoU + rho2 / c2, rho2 = (cx - gx)^2 + (cy - gy)^2, c2 = cw^2 + ch^2
    ciou: L = diou + alpha v, v = (4 / pi^2) (atan(gw / gh) - atan(w / h))^2, alpha = v / ((1 - IoU) + v) where v > 0 else 0,
          alpha a constant in the gradient, dv/dw and dv/dh the true derivatives
The tie rule: max(p, q) and min(p, q) pass the gradient to the predicted coordinate (p) only under the strict comparison
(p > q, p < q); max(0, .) only where its argument is > 0; the clamp only where |t| < W.  No epsilons.

rows(..., relax=) restates the rule with ONE comparison family made non-strict (RELAX): what a kernel with a `>=` for a `>` would
compute.  tests/test_box_iou_edges_cpu.py uses it to show that the inputs of tests/box_iou_edge_cases.py tell such a kernel from
the rule; nothing else may pass it."""
import numpy as np

from tests import multibox_oracle as M
from tests import softmax_focal_oracle as F

KINDS = ("giou", "diou", "ciou")
W = float(np.log(1000.0 / 16.0))
RELAX = ("intersection", "hull", "positive", "clamp")     # the corner indicators a, the corner indicators b, iwr / ihr >= 0, |t| <= W


def rows(kind, prior_wh, t, g, dtype=np.float64, relax=None):
    """prior_wh [n,2], t [n,4], g [n,4] -> (L [n], dL/dt [n,4]), every operation in `dtype`.  relax: None (the rule) or one of
    RELAX, the family of comparisons that also passes the gradient at equality (a mutation, for the tests of the tests)."""
    assert kind in KINDS, kind
    assert relax is None or relax in RELAX, relax
    lt, gt = (np.less_equal, np.greater_equal) if relax == "intersection" else (np.less, np.greater)
    hlt, hgt = (np.less_equal, np.greater_equal) if relax == "hull" else (np.less, np.greater)
    pos = np.greater_equal if relax == "positive" else np.greater
    inside = np.less_equal if relax == "clamp" else np.less
    f = dtype
    prior_wh, t, g = (np.asarray(x, dtype=f) for x in (prior_wh, t, g))
    half, one, two, zero, Wf = f(0.5), f(1.0), f(2.0), f(0.0), f(W)
    dw, dh = prior_wh[:, 0], prior_wh[:, 1]
    with np.errstate(all="ignore"):
        cx, cy = t[:, 0] * dw, t[:, 1] * dh
        w, h = dw * np.exp(np.clip(t[:, 2], -Wf, Wf)), dh * np.exp(np.clip(t[:, 3], -Wf, Wf))
        gx, gy = g[:, 0] * dw, g[:, 1] * dh
        gw, gh = dw * np.exp(np.clip(g[:, 2], -Wf, Wf)), dh * np.exp(np.clip(g[:, 3], -Wf, Wf))
        x1, x2, y1, y2 = cx - half * w, cx + half * w, cy - half * h, cy + half * h
        X1, X2, Y1, Y2 = gx - half * gw, gx + half * gw, gy - half * gh, gy + half * gh
        iwr, ihr = np.minimum(x2, X2) - np.maximum(x1, X1), np.minimum(y2, Y2) - np.maximum(y1, Y1)
        iw, ih = np.maximum(zero, iwr), np.maximum(zero, ihr)
        I = iw * ih
        U = (w * h + gw * gh) - I
        iou = I / U
        cw, ch = np.maximum(x2, X2) - np.minimum(x1, X1), np.maximum(y2, Y2) - np.minimum(y1, Y1)
        ind = lambda c: np.where(c, one, zero).astype(f)
        ax2, ax1 = ind(pos(iwr, zero) & lt(x2, X2)), ind(pos(iwr, zero) & gt(x1, X1))
        ay2, ay1 = ind(pos(ihr, zero) & lt(y2, Y2)), ind(pos(ihr, zero) & gt(y1, Y1))
        bx2, bx1, by2, by1 = ind(hgt(x2, X2)), ind(hlt(x1, X1)), ind(hgt(y2, Y2)), ind(hlt(y1, Y1))
        z = np.zeros_like(w)
        # derivatives with respect to cx, cy, w, h
        dI = [ih * (ax2 - ax1), iw * (ay2 - ay1), half * ih * (ax2 + ax1), half * iw * (ay2 + ay1)]
        dA = [z, z, h, w]
        dcw = [bx2 - bx1, z, half * (bx2 + bx1), z]
        dch = [z, by2 - by1, z, half * (by2 + by1)]
        L = one - iou
        dq = [-((dI[k] * U - I * (dA[k] - dI[k])) / (U * U)) for k in range(4)]
        if kind == "giou":
            Cc = cw * ch
            L = L + (Cc - U) / Cc
            for k in range(4):
                dq[k] = dq[k] + (U * (dcw[k] * ch + cw * dch[k]) - Cc * (dA[k] - dI[k])) / (Cc * Cc)
        else:
            ex, ey = cx - gx, cy - gy
            rho2, c2 = ex * ex + ey * ey, cw * cw + ch * ch
            L = L + rho2 / c2
            dr = [two * ex, two * ey, z, z]
            for k in range(4):
                dq[k] = dq[k] + (dr[k] * c2 - rho2 * (two * cw * dcw[k] + two * ch * dch[k])) / (c2 * c2)
            if kind == "ciou":
                kpi = f(4.0 / np.pi ** 2)
                da = np.arctan(gw / gh) - np.arctan(w / h)
                v = kpi * da * da
                alpha = np.where(v > 0, v / ((one - iou) + v), zero).astype(f)
                L = L + alpha * v
                s = alpha * (two * kpi) * da / (w * w + h * h)
                dq[2] = dq[2] - s * h
                dq[3] = dq[3] + s * w
        grad = np.stack([dw * dq[0], dh * dq[1], np.where(inside(np.abs(t[:, 2]), Wf), w * dq[2], zero),
                         np.where(inside(np.abs(t[:, 3]), Wf), h * dq[3], zero)], axis=1).astype(f)
    return L.astype(f), grad


def box_term(kind, priors, gt_loc, gt_mask, loc, loc_weight=1.0, grad_scale=1.0, dtype=np.float64):
    """priors [A,4], gt_loc / loc [B,A,4], gt_mask [B,A] -> (L_loc, dbox [B,A,4], bad): the sums in float64 whatever `dtype`
    the rows are evaluated in; bad: a positive's offsets, prior size, loss or gradient are not finite (status 3)."""
    mask = np.asarray(gt_mask).astype(bool)
    B, A = mask.shape
    P = int(mask.sum())
    dbox = np.zeros((B, A, 4))
    if P == 0:
        return 0.0, dbox, False
    b, a = np.nonzero(mask)
    wh = np.asarray(priors, np.float64)[a, 2:]
    t, g = np.asarray(loc)[b, a], np.asarray(gt_loc)[b, a]
    L, grad = rows(kind, wh, t, g, dtype)
    L, grad = L.astype(np.float64), grad.astype(np.float64)
    bad = not (np.isfinite(t).all() and np.isfinite(g).all() and (wh > 0).all() and np.isfinite(wh).all()
               and np.isfinite(L).all() and np.isfinite(grad).all())
    dbox[b, a] = grad_scale * loc_weight / P * grad
    return float(loc_weight * L.sum() / P), dbox, bad


def _with_box(out, kind, priors, gt_loc, gt_mask, loc, loc_weight, grad_scale, dtype):
    l_loc, dbox, bad = box_term(kind, priors, gt_loc, gt_mask, loc, loc_weight, grad_scale, dtype)
    out = dict(out)
    if bad:
        out["status"] = 3
    out["loc"], out["dbox"] = l_loc, dbox
    out["total"] = (l_loc + out["pos"]) + out["neg"]
    return out


def multibox_loss(kind, priors, gt_cls, gt_loc, gt_mask, loc, conf, neg_pos_ratio=3, loc_weight=1.0, grad_scale=1.0,
                  dtype=np.float64):
    """tests/multibox_oracle.multibox_loss with the box term `kind`: the same dict (loc, total, dbox and status replaced)."""
    zeros = np.zeros(np.asarray(loc).shape)                              # (the classification part does not read the offsets)
    out = M.multibox_loss(gt_cls, zeros, gt_mask, zeros, conf, neg_pos_ratio, loc_weight, grad_scale)
    return _with_box(out, kind, priors, gt_loc, gt_mask, loc, loc_weight, grad_scale, dtype)


def softmax_focal_loss(kind, priors, gt_cls, gt_loc, gt_mask, loc, conf, gamma=2.0, alpha=0.25, loc_weight=1.0, grad_scale=1.0,
                       dtype=np.float64):
    """tests/softmax_focal_oracle.softmax_focal_loss with the box term `kind`: the same dict (loc, total, dbox, status replaced)."""
    zeros = np.zeros(np.asarray(loc).shape)
    out = F.softmax_focal_loss(gt_cls, zeros, gt_mask, zeros, conf, gamma, alpha, loc_weight, grad_scale)
    return _with_box(out, kind, priors, gt_loc, gt_mask, loc, loc_weight, grad_scale, dtype)
