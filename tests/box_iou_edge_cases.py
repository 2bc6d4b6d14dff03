"""Inputs that meet the kinks of the IoU box terms on purpose (CPU and GPU share them): where tests/box_iou_cases.py draws every
positive away from a corner tie, iw == 0, ih == 0 and |t| == W, the positives here sit on them, with operands for which the
comparison a kernel makes cannot depend on rounding.  The regime is asserted on the oracle (tests/test_box_iou_edges_cpu.py),
never on what a kernel returned.

Lattice rows.  Prior sizes from {1/8, 1/4, 1/2} per axis, t2 = t3 = g2 = g3 = 0 (exp(0) is exactly 1, so w = gw = d_w and h = gh =
d_h), t0, t1 multiples of 1/4 in [-2, 2], g0, g1 multiples of 1/4 in [-1, 1]: every centre, corner, iwr and ihr is a small multiple
of a power of two, exact in float32 and the same in a bf16 and an f32 call.  In units of the prior the boxes are unit squares at
distance (t0 - g0, t1 - g1), so a distance of 0 ties both corners of an axis, 1 makes the boxes touch, more leaves a gap.  The draw
is uniform with g0 copied into t0 for a quarter of the rows (t1 alike), and then stratified: a pool is drawn and each of the nine
geometric CLASSES takes its share of rows from it in turn, so none is rare.

Designed rows (designed()) are fixed: identical boxes (zero log-sizes, and bf16 log-sizes with t == g bitwise: w == gw bitwise
whatever exp returns -- their centres are 0, so that the corners +-w/2 and with them I == U == cw ch are exact too and GIoU's
cancellation does not depend on exp's last bit), touching from each side and at a corner, ties on one axis with a partial overlap
on the other, strictly inside / containing with a common centre, disjoint, t2 / t3 at the bf16 neighbours of W (4.125 < W <
4.15625) and far beyond it (8, 100), targets beyond the clamp, and -- `exact_w`, the f32 case only, these values are not on the
bf16 grid -- t2 / t3 at float32(W) itself, which is > W and so clamped under the rule in float64 and in float32 alike, and one ulp
inside it (the bf16 case holds +-4 and +-4.25 in their place, so that both cases have the same layout).  The rows off the lattice
keep their distance from every other kink (asserted on the CPU).

Layout.  The SHAPES of tests/box_iou_cases.py; with B >= 2 image B - 2 has no positives, every other anchor is a positive (the
box term is what is under test), gt_cls is garbage off the mask.  The designed rows lie, each twice, at fixed anchors: from the
first positive anchor on (anchor 0 of image 0, or of image 1 where B == 2 empties image 0), on both sides of a 128-row block
boundary, and up to the last anchor of the last image; the lattice rows fill the rest."""
import functools

import numpy as np

from tests.box_iou_cases import SHAPES, GRAD_SCALES, LOC_WEIGHT, dloc_bound_floored             # noqa: F401
from tests.box_iou_oracle import W
from tests.softmax_focal_cases import to_bf16

SIZES = (0.125, 0.25, 0.5)
WF = np.float32(W)                                                        # the kernel's constant: float32(W) > W
WF_IN = np.nextafter(WF, np.float32(0))                                   # one ulp inside
ROW_BLOCK = 128
GEOMETRIC = ("identical", "x ties only", "y ties only", "touch x", "touch y", "touch corner", "touch one axis, gap on the other",
             "disjoint", "partial on both axes")
CLASSES = GEOMETRIC + ("clamped t2", "clamped t3", "clamped target")
assert float(WF) > W > float(WF_IN) and 4.125 < W < 4.15625


def corners(prior_wh, t, g):
    """float64: (x1, x2, y1, y2, X1, X2, Y1, Y2, iwr, ihr) of rows"""
    prior_wh, t, g = (np.asarray(x, np.float64) for x in (prior_wh, t, g))
    dw, dh = prior_wh[:, 0], prior_wh[:, 1]
    cx, cy, gx, gy = t[:, 0] * dw, t[:, 1] * dh, g[:, 0] * dw, g[:, 1] * dh
    w, h = dw * np.exp(np.clip(t[:, 2], -W, W)), dh * np.exp(np.clip(t[:, 3], -W, W))
    gw, gh = dw * np.exp(np.clip(g[:, 2], -W, W)), dh * np.exp(np.clip(g[:, 3], -W, W))
    x1, x2, y1, y2 = cx - w / 2, cx + w / 2, cy - h / 2, cy + h / 2
    X1, X2, Y1, Y2 = gx - gw / 2, gx + gw / 2, gy - gh / 2, gy + gh / 2
    iwr, ihr = np.minimum(x2, X2) - np.maximum(x1, X1), np.minimum(y2, Y2) - np.maximum(y1, Y1)
    return x1, x2, y1, y2, X1, X2, Y1, Y2, iwr, ihr


def classes_of(prior_wh, t, g):
    """{class: bool [n]} of rows, in float64 from the operands alone"""
    t, g = np.asarray(t, np.float64), np.asarray(g, np.float64)
    x1, x2, y1, y2, X1, X2, Y1, Y2, iwr, ihr = corners(prior_wh, t, g)
    xt, yt = (x1 == X1) | (x2 == X2), (y1 == Y1) | (y2 == Y2)
    ident = (x1 == X1) & (x2 == X2) & (y1 == Y1) & (y2 == Y2)
    over = (iwr > 0) & (ihr > 0)
    return {"identical": ident, "x ties only": xt & ~yt & over, "y ties only": yt & ~xt & over,
            "touch x": (iwr == 0) & (ihr > 0), "touch y": (ihr == 0) & (iwr > 0), "touch corner": (iwr == 0) & (ihr == 0),
            "touch one axis, gap on the other": ((iwr == 0) & (ihr < 0)) | ((ihr == 0) & (iwr < 0)),
            "disjoint": ((iwr < 0) | (ihr < 0)) & (iwr != 0) & (ihr != 0), "partial on both axes": over & ~xt & ~yt,
            "clamped t2": np.abs(t[:, 2]) >= W, "clamped t3": np.abs(t[:, 3]) >= W,
            "clamped target": (np.abs(g[:, 2:]) >= W).any(axis=1)}


def nearest_kink(prior_wh, t, g):
    """float64 [n]: the smallest non-zero |corner difference|, |iwr| or |ihr| of a row, in units of the smallest of its four box
    sides (inf where all are zero).  An exact zero is a tie met on purpose; anything else has to be far from one."""
    x1, x2, y1, y2, X1, X2, Y1, Y2, iwr, ihr = corners(prior_wh, t, g)
    gaps = np.abs(np.stack([x1 - X1, x2 - X2, y1 - Y1, y2 - Y2, iwr, ihr], axis=1))
    unit = np.minimum(np.minimum(x2 - x1, y2 - y1), np.minimum(X2 - X1, Y2 - Y1))
    return np.where(gaps > 0, gaps, np.inf).min(axis=1) / unit


def on_lattice(t, g):
    """bool [n]: zero log-sizes and offsets on the lattice"""
    t, g = np.asarray(t, np.float64), np.asarray(g, np.float64)
    quarters = (np.round(4 * t[:, :2]) == 4 * t[:, :2]).all(axis=1) & (np.round(4 * g[:, :2]) == 4 * g[:, :2]).all(axis=1)
    return quarters & (t[:, 2:] == 0).all(axis=1) & (g[:, 2:] == 0).all(axis=1) & (np.abs(t[:, :2]) <= 2).all(axis=1) & \
        (np.abs(g[:, :2]) <= 1).all(axis=1)


def designed(exact_w):
    """(t [n,4], g [n,4]) float32: the fixed rows, the same number with and without exact_w"""
    z = 0.0
    geo = [((0.5, -0.75, z, z), (0.5, -0.75, z, z)),                     # identical, zero log-sizes
           ((z, z, 0.40625, -0.3125), (z, z, 0.40625, -0.3125)),         # identical, bf16 log-sizes, centres 0
           ((-0.75, 0.5, z, z), (0.25, 0.25, z, z)),                     # touching in x from the left, partial in y
           ((1.0, -0.25, z, z), (z, 0.25, z, z)),                        # ... from the right
           ((0.25, -1.5, z, z), (0.75, -0.5, z, z)),                     # touching in y from below, partial in x
           ((-0.5, 1.75, z, z), (-0.25, 0.75, z, z)),                    # ... from above
           ((1.25, -0.5, z, z), (0.25, 0.5, z, z)),                      # touching at a corner
           ((0.75, -0.25, z, z), (0.75, 0.25, z, z)),                    # x corners tied, partial in y
           ((-1.0, 0.5, z, z), (-0.25, 0.5, z, z)),                      # y corners tied, partial in x
           ((0.25, -0.5, -0.5, -0.75), (0.25, -0.5, z, z)),              # strictly inside, common centre
           ((-0.5, 0.25, 0.5, 0.75), (-0.5, 0.25, z, z)),                # strictly containing, common centre
           ((-1.75, 2.0, z, z), (0.25, -0.5, z, z)),                     # disjoint on both axes
           ((-0.75, 1.75, z, z), (0.25, 0.25, z, z))]                    # touching in x, a gap in y

    # The clamp, one axis at a time, with non-zero offsets elsewhere and the other log-size unclamped.  Past +W the prediction is
    # 62.5 priors wide: the target is 33 wide (g = 3.5) and inside it, so IoU is about a half and w dL/dw -- the component the
    # clamp must zero -- about a half too.  Past -W it is 0.016 wide and inside a target of 0.135 (g = -2) with a partial overlap
    # on the other axis: the component is IoU itself, several percent.  So just inside the clamp the component is far above
    # the bound, just outside it is exactly 0, and a `<=` for the `<` shows.
    def clamp_row(axis, v):
        big = float(v) > 0
        t = [0.375, -0.625, 0.5, 0.5] if big else [0.03125, -0.015625, -2.5, -2.5]
        g = [-0.25, 0.125, 0.25, 0.25] if big else [-0.015625, 0.03125, -2.0, -2.0]
        if not big and axis == 1:                                        # the partial overlap lies on the axis that is not clamped
            t[:2], g[:2] = t[1::-1], g[1::-1]
        t[2 + axis], g[2 + axis] = v, (3.5 if big else -2.0)
        return tuple(t), tuple(g)

    lo, hi = 4.125, 4.15625                                              # the bf16 neighbours of W
    values = [lo, hi, -lo, -hi, 8.0, -8.0, 100.0, -100.0] + ([WF, WF_IN, -WF, -WF_IN] if exact_w else [4.0, 4.25, -4.0, -4.25])
    clamp = [clamp_row(axis, v) for v in values for axis in (0, 1)]
    clamp += [((0.375, -0.625, 100.0, -100.0), (-0.25, 0.125, 0.25, -0.125)),      # both clamped
              ((0.375, -0.625, -hi, hi), (-0.25, 0.125, 0.25, -0.125))]
    target = [((0.375, -0.625, 0.75, -0.5), (-0.25, 0.125, 5.0, -5.0)), ((-0.125, 0.625, -1.0, 1.5), (0.25, 0.375, -5.0, 5.0)),
              ((0.375, 0.125, 2.0, 0.25), (-0.25, -0.5, 5.0, 0.5)), ((-0.625, 0.375, 0.5, -2.0), (0.125, -0.25, -0.25, -5.0))]
    rows_ = geo + clamp + target
    t = np.array([r[0] for r in rows_], np.float32)
    g = np.array([r[1] for r in rows_], np.float32)
    assert exact_w or (np.array_equal(to_bf16(t), t) and np.array_equal(to_bf16(g), g))
    return t, g


def lattice(n, seed):
    """(t [n,4], g [n,4]) f32: n lattice rows, the nine geometric classes in turn.  Every comparison of the box term is made
    within one axis and both boxes scale with the prior's size on it, so a row's class does not depend on the prior it meets."""
    rng = np.random.default_rng(seed)
    M = 400 * max(n, 9)
    t, g = np.zeros((M, 4), np.float32), np.zeros((M, 4), np.float32)
    t[:, :2] = rng.integers(-8, 9, (M, 2)) / 4.0
    g[:, :2] = rng.integers(-4, 5, (M, 2)) / 4.0
    for k in (0, 1):
        copy = rng.random(M) < 0.25
        t[copy, k] = g[copy, k]
    cls = classes_of(np.ones((M, 2)), t, g)
    pick = []
    for i, name in enumerate(GEOMETRIC):
        need = n // 9 + (1 if i < n % 9 else 0)
        idx = np.nonzero(cls[name])[0]
        assert len(idx) >= need, (name, len(idx), need)
        pick.append(idx[:need])
    pick = np.sort(np.concatenate(pick))                                  # pool order: the classes interleave
    return t[pick], g[pick]


def edge_rows(n, fixed, seed, exact_w):
    """(t [n,4], g [n,4]) f32: the designed rows in turn at the indices `fixed`, lattice rows elsewhere"""
    dt, dg = designed(exact_w)
    fixed = np.asarray(fixed, np.int64)
    free = np.setdiff1d(np.arange(n), fixed)
    t, g = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    t[free], g[free] = lattice(len(free), seed + 1)
    which = np.arange(len(fixed)) % len(dt)
    t[fixed], g[fixed] = dt[which], dg[which]
    return t, g


def dyadic_sizes(rng, n):
    """[n,2] f64 prior sizes from SIZES"""
    return np.asarray(SIZES)[rng.integers(0, 3, (n, 2))]


def n_designed():
    return len(designed(False)[0])


@functools.lru_cache(maxsize=None)
def make_case(B, A, C, exact_w=False, seed=0):
    """The dict of tests/box_iou_cases.make_case (priors [A,4] f64, conf on the bf16 grid, loc, gt_loc f32, gt_cls i32, gt_mask
    u8).  loc and gt_loc lie on the bf16 grid unless exact_w (the f32 case).  Every image but B - 2 is all positives.  The priors'
    sizes are drawn from SIZES per anchor, independently of the rows (lattice(): a row's regime does not depend on them)."""
    rng = np.random.default_rng(9000 * C + A + seed)
    mask = np.ones((B, A), bool)
    if B >= 2:
        mask[B - 2] = False
    nd = n_designed()
    half = nd // 2
    b, a = np.nonzero(mask)
    flat = b * A + a
    n = len(flat)
    # the last row-block boundary of the last image with room for the run across it between the runs at both ends
    boundary = max(x for x in range(ROW_BLOCK, B * A, ROW_BLOCK)
                   if (B - 1) * A + half <= x - half and x + (nd - half) <= B * A - (nd - half))
    mid = int(np.nonzero(flat == boundary)[0][0])
    fixed = np.concatenate([np.arange(0, half), np.arange(mid - half, mid + (nd - half)), np.arange(n - (nd - half), n)])
    assert len(np.unique(fixed)) == 2 * nd and fixed.max() == n - 1
    t, g = edge_rows(n, fixed, 9000 * C + A + seed, exact_w)
    priors = np.concatenate([rng.random((A, 2)), dyadic_sizes(rng, A)], axis=1)
    loc = to_bf16(rng.standard_normal((B, A, 4)).astype(np.float32))     # off the mask: not read by the box term
    gt_loc = to_bf16((0.5 * rng.standard_normal((B, A, 4))).astype(np.float32))
    loc[b, a], gt_loc[b, a] = t, g
    conf = to_bf16(np.clip(3.0 * rng.standard_normal((B, A, C)), -16.0, 16.0).astype(np.float32))
    gt_cls = rng.integers(0, C - 1, (B, A)).astype(np.int32)
    gt_cls[~mask] = 0x7fffff
    for arr in (priors, conf, loc, gt_loc, gt_cls):
        arr.setflags(write=False)
    return dict(B=B, A=A, C=C, priors=priors, conf=conf, loc=loc, gt_loc=gt_loc, gt_cls=gt_cls, gt_mask=mask.astype(np.uint8),
                fixed=fixed, boundary=boundary, exact_w=exact_w)


@functools.lru_cache(maxsize=None)
def identical_case(B, A, C):
    """make_case with every positive the identical zero-log-size row: loc == gt_loc, offsets on the lattice, log-sizes 0"""
    c = dict(make_case(B, A, C))
    mask = c["gt_mask"].astype(bool)
    rng = np.random.default_rng(31 * A + C)
    loc = c["loc"].copy()
    loc[..., :2] = rng.integers(-4, 5, (B, A, 2)) / 4.0
    loc[..., 2:] = 0.0
    gt_loc = c["gt_loc"].copy()
    gt_loc[mask] = loc[mask]
    loc.setflags(write=False)
    gt_loc.setflags(write=False)
    c["loc"], c["gt_loc"] = loc, gt_loc
    return c


def positives(c):
    """(prior_wh [n,2], t [n,4], g [n,4]) of a case's positives, in flat anchor order"""
    b, a = np.nonzero(c["gt_mask"])
    return c["priors"][a, 2:], c["loc"][b, a], c["gt_loc"][b, a]


def classes(c):
    """{class: bool [n]} over the case's positives"""
    return classes_of(*positives(c))


def scale_of(c, grad_scale, loc_weight=LOC_WEIGHT):
    """grad_scale * loc_weight / P: the factor of every dloc element"""
    return grad_scale * loc_weight / float(c["gt_mask"].sum())
