"""Inputs of the IoU box term tests (CPU and GPU share them).  Priors are random: centres in [0, 1], sizes the SSD300 scales times
the aspect ratios.  `loc` lies on the bf16 grid (so the f32 and bf16 calls see the same values), `gt_loc` is float32; the targets
spread by about 0.5 and the predictions by about 1.0, so boxes that overlap, that are disjoint on one axis or on both, and
that contain one another all occur.  About 10 % of the anchors are positives; with B >= 2 image B - 2 has none, and the last
anchor of the last image is one (a positive in the last row of a ragged last row block).

The losses have kinks where the gradient jumps: the four corner ties (x1 = X1, ...), iw = 0, ih = 0 and |t2|, |t3| = W.  A float32
evaluation may fall on the other side of one, so a positive closer to a kink than 1e-3 of the smallest of (w, h, gw, gh) --
1e-3 absolute for the clamp -- is drawn again.  make_case asserts that fewer than 2 % of the first draws needed it.

So these cases never hand a kernel a tie, a touching pair, pred == target or a clamped log-size.  tests/box_iou_edge_cases.py is
where the kinks are met on purpose, with operands that decide every comparison exactly (tests/test_box_iou_edges_gpu.py)."""
import functools

import numpy as np

from tests.box_iou_oracle import W
from tests.softmax_focal_cases import to_bf16

SHAPES = [(2, 150, 4), (3, 300, 21)]
GRAD_SCALES = (1.0, 0.25)
LOC_WEIGHT = 0.5
SCALES = (0.1, 0.2, 0.375, 0.55, 0.725, 0.9)
RATIOS = (1.0, 2.0, 0.5, 3.0, 1.0 / 3.0)
KINK = 1e-3


def random_priors(rng, A):
    """[A,4] float64 (cx, cy, w, h)"""
    s = np.asarray(SCALES)[rng.integers(0, len(SCALES), A)]
    r = np.asarray(RATIOS)[rng.integers(0, len(RATIOS), A)]
    return np.stack([rng.random(A), rng.random(A), s * np.sqrt(r), s / np.sqrt(r)], axis=1)


def near_kink(prior_wh, t, g):
    """bool [n]: the row is closer than KINK to a kink (float64)"""
    prior_wh, t, g = (np.asarray(x, np.float64) for x in (prior_wh, t, g))
    dw, dh = prior_wh[:, 0], prior_wh[:, 1]
    cx, cy, gx, gy = t[:, 0] * dw, t[:, 1] * dh, g[:, 0] * dw, g[:, 1] * dh
    w, h = dw * np.exp(np.clip(t[:, 2], -W, W)), dh * np.exp(np.clip(t[:, 3], -W, W))
    gw, gh = dw * np.exp(np.clip(g[:, 2], -W, W)), dh * np.exp(np.clip(g[:, 3], -W, W))
    x1, x2, y1, y2 = cx - w / 2, cx + w / 2, cy - h / 2, cy + h / 2
    X1, X2, Y1, Y2 = gx - gw / 2, gx + gw / 2, gy - gh / 2, gy + gh / 2
    iwr, ihr = np.minimum(x2, X2) - np.maximum(x1, X1), np.minimum(y2, Y2) - np.maximum(y1, Y1)
    gaps = np.abs(np.stack([x1 - X1, x2 - X2, y1 - Y1, y2 - Y2, iwr, ihr], axis=1)).min(axis=1)
    unit = np.minimum(np.minimum(w, h), np.minimum(gw, gh))
    clamp = np.abs(np.abs(t[:, 2:]) - W).min(axis=1)
    return (gaps < KINK * unit) | (clamp < KINK)


def draw_loc(rng, shape):
    return to_bf16(rng.standard_normal(shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def make_case(B, A, C, seed=0):
    """dict: priors [A,4] f64, conf [B,A,C] f32 on the bf16 grid, loc [B,A,4] f32 on the bf16 grid, gt_loc [B,A,4] f32,
    gt_cls [B,A] i32 (garbage off the mask), gt_mask [B,A] u8, redrawn (the fraction of positives drawn again)."""
    rng = np.random.default_rng(7000 * C + A + seed)
    priors = random_priors(rng, A)
    conf = to_bf16(np.clip(3.0 * rng.standard_normal((B, A, C)), -16.0, 16.0).astype(np.float32))
    loc = draw_loc(rng, (B, A, 4))
    gt_loc = (0.5 * rng.standard_normal((B, A, 4))).astype(np.float32)
    mask = rng.random((B, A)) < 0.1
    if B >= 2:
        mask[B - 2] = False
    mask[B - 1, A - 1] = True
    gt_cls = rng.integers(0, C - 1, (B, A)).astype(np.int32)
    gt_cls[~mask] = 0x7fffff
    b, a = np.nonzero(mask)
    first = None
    for _ in range(20):
        bad = near_kink(priors[a, 2:], loc[b, a], gt_loc[b, a])
        first = float(bad.mean()) if first is None else first
        if not bad.any():
            break
        loc[b[bad], a[bad]] = draw_loc(rng, (int(bad.sum()), 4))
    assert not near_kink(priors[a, 2:], loc[b, a], gt_loc[b, a]).any()
    assert first < 0.02, first
    for arr in (priors, conf, loc, gt_loc, gt_cls):
        arr.setflags(write=False)
    return dict(B=B, A=A, C=C, priors=priors, conf=conf, loc=loc, gt_loc=gt_loc, gt_cls=gt_cls, gt_mask=mask.astype(np.uint8),
                redrawn=first)


def positives(c):
    """(prior_wh [n,2], t [n,4], g [n,4]) of a case's positives"""
    b, a = np.nonzero(c["gt_mask"])
    return c["priors"][a, 2:], c["loc"][b, a], c["gt_loc"][b, a]


def dloc_bound(ref, bf16=False):
    """The bound on dloc [..., 4]: per anchor 1e-4 of the anchor's largest reference component in f32 (an elementwise relative
    bound is not achievable: a component near zero is a difference of terms of the size of the largest); a bf16 output adds its
    rounding, the project's 4e-3 |ref| per element.  0 off the positives: exact zeros."""
    return 1e-4 * np.abs(ref).max(axis=-1, keepdims=True) + (4e-3 * np.abs(ref) if bf16 else 0.0)


def dloc_bound_floored(ref, scale, bf16=False):
    """dloc_bound with a floor, for the inputs of tests/box_iou_edge_cases.py: per anchor 1e-4 * scale * max(largest |component| of
    the row's gradient, 1), where ref [..., 4] = scale * gradient and scale = grad_scale * loc_weight / P.  The floor is derived:
    at identical boxes GIoU's gradient is the difference of two terms that are each w dIoU/dw = 1 (DIoU's value there), so the
    row's own largest component is about 0 and says nothing about the size of what was subtracted.  Where a row's largest
    component is 1 or more this is dloc_bound.  bf16 adds its rounding, 4e-3 |ref| per element."""
    return 1e-4 * np.maximum(np.abs(ref).max(axis=-1, keepdims=True), scale) + (4e-3 * np.abs(ref) if bf16 else 0.0)
