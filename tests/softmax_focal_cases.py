"""Inputs of the softmax focal loss tests (CPU and GPU share them): random logits N(0, 3) clipped to |z| <= 16 with designed rows
at the front of image 0 -- each once as a positive and once as a background anchor:
    "above"   z_t 12 above every other logit (confident and correct: q ~ (C-1) e^-12, where 1 - p_t and z_t - lse cancel)
    "below"   z_t 12 below every other logit (confident and wrong)
    "equal"   all logits equal
    "twomax"  two equal maxima, one of them the target
and, with B >= 2, a last image without positives beside images with them.
extreme_case: rows beyond the +-16 clip -- logit gaps of 30 .. 120, where q == 0 and p_t == 0 exactly in float32."""
import functools

import numpy as np

SHAPES = [(2, 37, 3), (1, 129, 2), (3, 300, 21), (2, 1100, 81), (1, 200, 303)]
GAMMAS, ALPHAS, GRAD_SCALES = (0.0, 0.5, 2.0, 3.0), (-1.0, 0.25, 0.5), (1.0, 0.25)
DESIGNED = ("above", "below", "equal", "twomax")


def to_bf16(x):
    """float32 array rounded to bfloat16 (round to nearest even), returned as float32."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((u >> 16) & 1) + 0x7fff
    return ((u + r) & 0xffff0000).astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def make_case(B, A, C, bf16=False, seed=0):
    """dict: conf [B,A,C] f32, loc, gt_loc [B,A,4] f32, gt_cls [B,A] i32, gt_mask [B,A] u8, designed {name: (pos anchor, bg anchor)}
    (anchors of image 0).  bf16: conf and loc hold bfloat16 values.  Unmasked anchors carry a gt_cls that must not be read."""
    rng = np.random.default_rng(1000 * C + A + seed)
    conf = np.clip(3.0 * rng.standard_normal((B, A, C)), -16.0, 16.0).astype(np.float32)
    loc = (1.5 * rng.standard_normal((B, A, 4))).astype(np.float32)
    gt_loc = rng.standard_normal((B, A, 4)).astype(np.float32)
    mask = rng.random((B, A)) < 0.1
    gt_cls = rng.integers(0, C - 1, (B, A)).astype(np.int32)
    designed = {}
    for k, name in enumerate(DESIGNED):
        for which, a in enumerate((2 * k, 2 * k + 1)):                    # positive, then background
            mask[0, a] = which == 0
            t = int(gt_cls[0, a]) if which == 0 else C - 1
            z = conf[0, a]
            others = np.arange(C) != t
            if name == "above":
                z[others] = np.clip(z[others], -16.0, 4.0)
                z[t] = z[others].max() + 12.0
            elif name == "below":
                z[others] = np.clip(z[others], -4.0, 16.0)
                z[t] = z[others].min() - 12.0
            elif name == "equal":
                z[:] = 1.5
            else:
                z[:] = np.clip(z, -16.0, 8.0)
                z[t] = z.max() + 1.0
                z[(t + 1) % C] = z[t]
        designed[name] = (2 * k, 2 * k + 1)
    mask[:, -1] = True                                                    # every image has a positive ...
    if B >= 2:
        mask[B - 1] = False                                               # ... but the last one, with B >= 2
    gt_cls[~mask] = 0x7fffff                                              # garbage where the mask is off
    if bf16:
        conf, loc = to_bf16(conf), to_bf16(loc)
    for arr in (conf, loc, gt_loc, gt_cls):
        arr.setflags(write=False)
    return dict(B=B, A=A, C=C, conf=conf, loc=loc, gt_loc=gt_loc, gt_cls=gt_cls, gt_mask=mask.astype(np.uint8), designed=designed)


EXTREME_GAPS = (30.0, 88.0, 104.0, 120.0)                                # all exact in bf16 next to logits that are multiples of 1/2
EXTREME_CLASSES = (2, 3, 21, 81, 303)
EXTREME_GAMMAS, EXTREME_ALPHAS = (0.0, 0.5, 1.0, 2.0, 8.0), (-1.0, 0.0, 0.25, 1.0)


@functools.lru_cache(maxsize=None)
def extreme_case(C, seed=0):
    """B = 1, A = 16: for every gap of EXTREME_GAPS a row whose target logit lies that far ABOVE every other logit (at 104 and 120
    Q underflows and q == 0 exactly in float32: the h = 1 branch; at 30 q ~ 1e-11 on the log1p branch) and one whose target lies
    that far BELOW (p_t == 0 exactly, q == 1), each once as a positive and once as a background anchor.  The other logits are
    multiples of 1/2 in [-4, 4], so every logit is a bfloat16 value.  P = 8.  Adds "rows": [(anchor, gap, side, positive)]."""
    rng = np.random.default_rng(7000 + C + seed)
    A = 4 * len(EXTREME_GAPS)
    conf = (rng.integers(-8, 9, (1, A, C)) / 2.0).astype(np.float32)
    loc = (rng.integers(-8, 9, (1, A, 4)) / 4.0).astype(np.float32)
    gt_loc = (rng.integers(-8, 9, (1, A, 4)) / 4.0).astype(np.float32)
    mask = np.zeros((1, A), dtype=bool)
    gt_cls = rng.integers(0, C - 1, (1, A)).astype(np.int32)
    rows = []
    a = 0
    for gap in EXTREME_GAPS:
        for side in ("above", "below"):
            for positive in (True, False):
                mask[0, a] = positive
                t = int(gt_cls[0, a]) if positive else C - 1
                z = conf[0, a]
                others = np.arange(C) != t
                z[t] = z[others].max() + gap if side == "above" else z[others].min() - gap
                rows.append((a, gap, side, positive))
                a += 1
    gt_cls[~mask] = 0x7fffff
    assert np.array_equal(to_bf16(conf), conf) and np.array_equal(to_bf16(loc), loc)
    for arr in (conf, loc, gt_loc, gt_cls):
        arr.setflags(write=False)
    return dict(B=1, A=A, C=C, conf=conf, loc=loc, gt_loc=gt_loc, gt_cls=gt_cls, gt_mask=mask.astype(np.uint8), rows=tuple(rows))


def dconf_bound(ref, bf16=False):
    """The elementwise bound on dconf: 1e-4 |ref| + 2^-100 in f32 (the stable form's worst-case fp32 error is about
    gamma (C + 40) 2^-24 <= 6.2e-5 for C <= 303, gamma <= 3); a bf16 output adds its rounding, the project's 4e-3 |ref|."""
    return (1e-4 + (4e-3 if bf16 else 0.0)) * np.abs(ref) + 2.0 ** -100
