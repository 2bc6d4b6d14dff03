"""numpy restatement of the device data augmentation (include/ssd_hip.h, "SSD data augmentation"; csrc/augment.hip).

TEST INFRASTRUCTURE.  Every float32 operation is rounded where the kernel rounds it (numpy float32 arithmetic, no fused
multiply-add).  Unlike the kernel, the oracle materialises what the recipe describes: it distorts the whole source image,
builds the expanded canvas, cuts the patch out as an array and resizes it with oracle.ssd_oracle.resize_bilinear, then
mirrors the result.  The kernel never stores canvas or patch; equality of the two is what the GPU tests check."""
import numpy as np

from oracle.ssd_oracle import resize_bilinear

PHOTO, EXPAND, CROP, FLIP = 1, 2, 4, 8
ALL = PHOTO | EXPAND | CROP | FLIP
PH_BRIGHT, PH_CONTRAST, PH_CONTRAST_FIRST, PH_SAT, PH_HUE = 1, 2, 4, 8, 16
TRIALS = 50
MIN_IOU = {1: 0.1, 2: 0.3, 3: 0.5, 4: 0.7, 5: 0.9}
MEAN = np.array([123 / 255, 117 / 255, 104 / 255]).astype(np.float32)

F = np.float32
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


# --------------------------------------------------------------------------------------------- Philox-4x32-10
def philox4x32_10(ctr, key):
    """Random123 philox4x32 with 10 rounds.  ctr uint32 [..., 4], key uint32 [..., 2] -> uint32 [..., 4]."""
    c = [np.asarray(ctr, np.uint64)[..., i] for i in range(4)]
    k0 = np.asarray(key, np.uint64)[..., 0].copy()
    k1 = np.asarray(key, np.uint64)[..., 1].copy()
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(_W0)) & _MASK
            k1 = (k1 + np.uint64(_W1)) & _MASK
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
    return np.stack(c, -1).astype(np.uint32)


def draws(seed, index, slot, block=0):
    """The four words of (sample index, slot, block) under `seed` (include/ssd_hip.h slot layout).  slot may be an array."""
    slot = np.asarray(slot, np.uint64)
    index = int(index)
    ctr = np.stack(np.broadcast_arrays(np.uint64(index & 0xFFFFFFFF), np.uint64(index >> 32), slot, np.uint64(block)), -1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(key, ctr.shape[:-1] + (2,)))


def u01(w):
    return ((np.asarray(w, np.uint32) >> np.uint32(8)).astype(np.float32) * F(2.0 ** -24)).astype(np.float32)


def below(w, n):
    return ((np.asarray(w, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def coin(w):
    return int(np.uint32(w) >> np.uint32(31))


# --------------------------------------------------------------------------------------------- plan
def _canvas_boxes(box, W, H, left, top):
    """Boxes (relative cx,cy,w,h, f32 [n,4]) in canvas pixels: x1, y1, x2, y2, ccx, ccy, each f32 [n]."""
    b = np.asarray(box, np.float32).reshape(-1, 4)
    cx, cy, w, h = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    Wf, Hf, lf, tf = F(W), F(H), F(left), F(top)
    hw, hh = w * F(0.5), h * F(0.5)
    x1 = (cx - hw) * Wf + lf
    x2 = (cx + hw) * Wf + lf
    y1 = (cy - hh) * Hf + tf
    y2 = (cy + hh) * Hf + tf
    return x1, y1, x2, y2, cx * Wf + lf, cy * Hf + tf


def _inside(cb, px, py, pw, ph):
    """[..., n] centre strictly inside the patch (px, py, pw, ph broadcast against the boxes)."""
    ccx, ccy = cb[4], cb[5]
    return (F(px) < ccx) & (ccx < F(px + pw)) & (F(py) < ccy) & (ccy < F(py + ph))


def _iou(cb, px, py, pw, ph):
    x1, y1, x2, y2 = cb[:4]
    qx1, qx2 = np.asarray(px, np.float32), np.asarray(px + pw, np.float32)
    qy1, qy2 = np.asarray(py, np.float32), np.asarray(py + ph, np.float32)
    iw = np.maximum(np.minimum(x2, qx2) - np.maximum(x1, qx1), F(0))
    ih = np.maximum(np.minimum(y2, qy2) - np.maximum(y1, qy1), F(0))
    inter = iw * ih
    ab = (x2 - x1) * (y2 - y1)
    ap = np.asarray(pw, np.float32) * np.asarray(ph, np.float32)
    return inter / ((ab + ap) - inter)


def plan(box, cls, src_hw, stages, seed, index):
    """One image: box f32 [n,4] relative (cx,cy,w,h) against src_hw = (H, W).  Returns (params dict with the fields of
    ssd_augment_params, kept boxes f32 [m,4], kept classes f32 [m])."""
    H, W = int(src_hw[0]), int(src_hw[1])
    box = np.asarray(box, np.float32).reshape(-1, 4)
    cls = np.asarray(cls, np.float32).reshape(-1)
    n = box.shape[0]
    p = dict(stages=stages & PHOTO, reserved0=0, reserved1=0)
    a, c, h = draws(seed, index, 0, 0), draws(seed, index, 0, 1), draws(seed, index, 0, 2)
    p["delta"] = (F(-32) + u01(a[1]) * F(64)) / F(255)
    p["alpha"] = F(0.5) + u01(a[3])
    p["saturation"] = F(0.5) + u01(c[2])
    p["hue"] = F(-18) + u01(h[0]) * F(36)
    photo = 0
    if stages & PHOTO:
        photo = (coin(a[0]) * PH_BRIGHT | coin(a[2]) * PH_CONTRAST | coin(c[0]) * PH_CONTRAST_FIRST |
                 coin(c[1]) * PH_SAT | coin(c[3]) * PH_HUE)
        if not photo & PH_CONTRAST:
            photo &= ~PH_CONTRAST_FIRST
    p["photo"] = photo
    e = draws(seed, index, 1)
    CW, CH, left, top = W, H, 0, 0
    if stages & EXPAND and coin(e[0]):
        ratio = F(1) + u01(e[1]) * F(3)
        CW, CH = int(ratio * F(W)), int(ratio * F(H))
        left, top = int(below(e[2], CW - W + 1)), int(below(e[3], CH - H + 1))
        p["stages"] |= EXPAND
    p.update(canvas_w=CW, canvas_h=CH, off_x=left, off_y=top)
    m = draws(seed, index, 2)
    mode = int(below(m[0], 7)) if stages & CROP else 0
    p["mode"] = mode
    p["flip"] = 1 if (stages & FLIP and coin(m[1])) else 0
    if p["flip"]:
        p["stages"] |= FLIP
    px, py, pw, ph, trial = 0, 0, CW, CH, -1
    cb = _canvas_boxes(box, W, H, left, top)
    if mode != 0 and n > 0:
        r = draws(seed, index, 3 + np.arange(TRIALS))                              # [50, 4]
        tw = np.minimum(np.maximum(((F(0.3) + u01(r[:, 0]) * F(0.7)) * F(CW)).astype(np.int64), 1), CW)
        th = np.minimum(np.maximum(((F(0.3) + u01(r[:, 1]) * F(0.7)) * F(CH)).astype(np.int64), 1), CH)
        tx, ty = below(r[:, 2], CW - tw + 1), below(r[:, 3], CH - th + 1)
        ok = (2 * th >= tw) & (th <= 2 * tw)
        col = lambda v: v[:, None]                                                  # noqa: E731  trials x boxes
        ctr = _inside(cb, col(tx), col(ty), col(tw), col(th)).any(1)
        if mode == 6:
            good = np.ones(TRIALS, bool)
        else:
            good = (_iou(cb, col(tx), col(ty), col(tw), col(th)) >= F(MIN_IOU[mode])).any(1)
        acc = np.flatnonzero(ok & ctr & good)
        if acc.size:                                                                # the first accepted trial wins
            trial = int(acc[0])
            px, py, pw, ph = int(tx[trial]), int(ty[trial]), int(tw[trial]), int(th[trial])
            p["stages"] |= CROP
    p.update(trial=trial, patch_x=px, patch_y=py, patch_w=pw, patch_h=ph)
    keep = _inside(cb, px, py, pw, ph) if trial >= 0 else np.ones(n, bool)
    out = box.copy()
    if p["stages"] & (EXPAND | CROP):
        x1, y1, x2, y2 = cb[:4]
        fpx, fpy, fpw, fph = F(px), F(py), F(pw), F(ph)
        rx1 = (np.maximum(x1, fpx) - fpx) / fpw
        rx2 = (np.minimum(x2, F(px + pw)) - fpx) / fpw
        ry1 = (np.maximum(y1, fpy) - fpy) / fph
        ry2 = (np.minimum(y2, F(py + ph)) - fpy) / fph
        out = np.stack([(rx1 + rx2) * F(0.5), (ry1 + ry2) * F(0.5), rx2 - rx1, ry2 - ry1], 1).astype(np.float32)
    if p["flip"]:
        out[:, 0] = F(1) - out[:, 0]
    p["n_boxes"] = int(keep.sum())
    return p, out[keep].reshape(-1, 4), cls[keep]


def plan_batch(boxes, classes, src_hw, stages, seed, first_index):
    """The batch form of ssd_augment_plan: (list of params dicts, box_out [total,4] with zero rows after the kept ones,
    cls_out [total], off_out [B+1])."""
    total = sum(np.asarray(b).reshape(-1, 4).shape[0] for b in boxes)
    ps, bo, co = [], [], []
    for i, (b, c) in enumerate(zip(boxes, classes)):
        p, nb, nc = plan(b, c, src_hw[i], stages, seed, first_index + i)
        ps.append(p)
        bo.append(nb)
        co.append(nc)
    off = np.zeros(len(ps) + 1, np.int32)
    off[1:] = np.cumsum([p["n_boxes"] for p in ps])
    box_out = np.zeros((total, 4), np.float32)
    cls_out = np.zeros((total,), np.float32)
    if off[-1]:
        box_out[:off[-1]] = np.concatenate(bo, 0)
        cls_out[:off[-1]] = np.concatenate(co, 0)
    return ps, box_out, cls_out, off


# --------------------------------------------------------------------------------------------- image
def _clamp(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def distort(img, p):
    """Photometric distortion of an f32 [H,W,3] image in [0,1] (ssd_hip.h step 1)."""
    photo = p["photo"]
    r, g, b = (np.array(img[..., i], np.float32) for i in range(3))
    if photo & PH_BRIGHT:
        d = F(p["delta"])
        r, g, b = _clamp(r + d), _clamp(g + d), _clamp(b + d)
    alpha = F(p["alpha"])
    if photo & PH_CONTRAST and photo & PH_CONTRAST_FIRST:
        r, g, b = _clamp(r * alpha), _clamp(g * alpha), _clamp(b * alpha)
    if photo & (PH_SAT | PH_HUE):
        v = np.maximum(np.maximum(r, g), b)
        mn = np.minimum(np.minimum(r, g), b)
        d = v - mn
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(v > 0, d / np.where(v > 0, v, F(1)), F(0)).astype(np.float32)
            dd = np.where(d == 0, F(1), d)
            hr = F(60) * ((g - b) / dd)
            hg = F(120) + F(60) * ((b - r) / dd)
            hb = F(240) + F(60) * ((r - g) / dd)
        h = np.where(d == 0, F(0), np.where(v == r, hr, np.where(v == g, hg, hb))).astype(np.float32)
        h = np.where(h < 0, h + F(360), h).astype(np.float32)
        if photo & PH_SAT:
            s = _clamp(s * F(p["saturation"]))
        if photo & PH_HUE:
            h = h + F(p["hue"])
            h = np.where(h >= F(360), h - F(360), np.where(h < 0, h + F(360), h)).astype(np.float32)
        q6 = h / F(60)
        i = np.floor(q6).astype(np.int64)
        f = q6 - i.astype(np.float32)
        i[i >= 6] = 0
        pp = v * (F(1) - s)
        qq = v * (F(1) - s * f)
        tt = v * (F(1) - s * (F(1) - f))
        sel = [(v, tt, pp), (qq, v, pp), (pp, v, tt), (pp, qq, v), (tt, pp, v), (v, pp, qq)]
        r = np.select([i == k for k in range(6)], [t[0] for t in sel])
        g = np.select([i == k for k in range(6)], [t[1] for t in sel])
        b = np.select([i == k for k in range(6)], [t[2] for t in sel])
        r, g, b = _clamp(r.astype(np.float32)), _clamp(g.astype(np.float32)), _clamp(b.astype(np.float32))
    if photo & PH_CONTRAST and not photo & PH_CONTRAST_FIRST:
        r, g, b = _clamp(r * alpha), _clamp(g * alpha), _clamp(b * alpha)
    return np.stack([r, g, b], -1).astype(np.float32)


def to_unit(img):
    """uint8 -> /255 in float64 rounded to float32 (ssd_image_resize_prep's table); f32 passes through."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return (img.astype(np.float64) / 255.0).astype(np.float32)
    return np.asarray(img, np.float32)


def image(img, p, S=300, normalize=True):
    """One image (uint8 [H,W,3] or f32 in [0,1]) under its params -> f32 [S,S,3] before the bf16 rounding."""
    x = to_unit(img)
    H, W = x.shape[:2]
    if p["photo"]:
        x = distort(x, p)
    canvas = np.empty((p["canvas_h"], p["canvas_w"], 3), np.float32)
    canvas[...] = MEAN
    canvas[p["off_y"]:p["off_y"] + H, p["off_x"]:p["off_x"] + W] = x
    patch = canvas[p["patch_y"]:p["patch_y"] + p["patch_h"], p["patch_x"]:p["patch_x"] + p["patch_w"]]
    out = resize_bilinear(np.ascontiguousarray(patch), S)
    if p["flip"]:
        out = out[:, ::-1]
    if normalize:
        out = ((out - F(0.5)) * F(2)).astype(np.float32)
    return np.ascontiguousarray(out)


def params_equal(dev_rec, p):
    """Field-by-field comparison of a device record (numpy structured scalar) with an oracle dict; returns the differing
    field names."""
    bad = []
    for name in dev_rec.dtype.names:
        a, b = dev_rec[name], p[name]
        if isinstance(b, (float, np.floating)):
            same = np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)
        else:
            same = int(a) == int(b)
        if not same:
            bad.append(name)
    return bad
