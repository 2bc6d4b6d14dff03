"""Device-tensor wrappers over the C ABI (include/ssd_hip.h).  torch supplies device memory and the
current HIP stream only; every computation runs in libssd_hip.so."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib

# SSD300 geometry of the reference (models/ssd_model.py:153,164,176-177)
SSD300_GRIDS = ((38, 38), (19, 19), (10, 10), (5, 5), (3, 3), (1, 1))
SSD300_S_REF = (21, 45, 99, 153, 207, 261, 315)
SSD300_RATIOS = ((2,), (2, 3), (2, 3), (2, 3), (2,), (2,))
# SSD512 geometry of the ResNet-50 network (resnet_engine.py; seven levels, 24 564 anchors at a 512 x 512 input).  The scales
# are pixels of a 512 input: at input S they are S_REF * S / 512 (ssd512_s_ref)
SSD512_S_REF = (20, 51, 133, 215, 297, 379, 461, 543)
SSD512_RATIOS = ((2,), (2, 3), (2, 3), (2, 3), (2, 3), (2,), (2,))
# MobileNet-v1 SSD300 (engine.MOBILENET_V1_SSD300_TRUNK; grids 19, 10, 5, 3, 2, 1 = 2268 anchors): scales 0.2 .. 0.95 of 300 in equal
# steps and one beyond, the MobileNet-SSD convention; the ratios are SSD300_RATIOS
MOBILENET_SSD300_S_REF = (60, 105, 150, 195, 240, 285, 330)


def ssd512_s_ref(in_size):
    """SSD512_S_REF scaled to an input of in_size pixels."""
    return tuple(v * in_size / 512.0 for v in SSD512_S_REF)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype):
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return t


class PriorSet:
    """Default boxes on the device + everything derived from them once (unmatched-row encodings,
    the geometry hint for the matcher)."""

    def __init__(self, priors, enc_zero, grid=None):
        self.priors = priors            # f64 [A,4] device
        self.enc_zero = enc_zero        # f32 [A,4] device
        self.grid = grid                # _lib.PriorGrid or None
        self.A = priors.shape[0]

    def verify_grid(self):
        """Check the geometry against the prior array on the device (one host sync, at build time): a verified grid lets
        ssd_match_encode take its single-launch path.  Returns whether it was verified."""
        if self.grid is None:
            return False
        scratch = torch.zeros((1,), dtype=torch.int32, device=self.priors.device)
        _lib.check(_lib.lib().ssd_prior_grid_verify(_ptr(self.priors), self.A, ctypes.byref(self.grid), _ptr(scratch), _stream()))
        return self.grid.verified != 0


def make_grid(grids, ratios):
    g = _lib.PriorGrid()
    g.levels = len(grids)
    for i, ((h, w), r) in enumerate(zip(grids, ratios)):
        g.grid_h[i], g.grid_w[i], g.per_cell[i] = h, w, 2 + 2 * len(r)
    return g


def build_priors(grids=SSD300_GRIDS, s_ref=SSD300_S_REF, ratios=SSD300_RATIOS, in_size=300, device="cuda"):
    """ssd_priors + ssd_encode_zero (replaces _build_prior_box, models/ssd_model.py:173-194)."""
    L = _lib.lib()
    levels = len(grids)
    hw = (ctypes.c_int * (2 * levels))(*[v for g in grids for v in g])
    sref = (ctypes.c_double * (levels + 1))(*[float(s) for s in s_ref])
    flat = [r for rr in ratios for r in rr]
    rat = (ctypes.c_int * max(len(flat), 1))(*flat)
    off = [0]
    for rr in ratios:
        off.append(off[-1] + len(rr))
    roff = (ctypes.c_int * (levels + 1))(*off)
    A = L.ssd_priors_count(hw, levels, roff)
    if A <= 0:
        _lib.check(A if A < 0 else _lib.SSD_ERR_VALUE)
    pri = torch.empty((A, 4), dtype=torch.float64, device=device)
    _lib.check(L.ssd_priors(hw, levels, sref, rat, roff, float(in_size), _ptr(pri), _stream()))
    return prior_set_from(pri, make_grid(grids, ratios))


def prior_set_from(priors, grid=None, verify=False):
    """Wrap an existing device f64 [A,4] prior array (any geometry).  verify=True also checks `grid` against the array on the
    device (PriorSet.verify_grid: one launch + one host synchronisation) -- only the opt-in single-launch matcher needs a
    verified grid, so the default construction neither launches nor synchronises for it."""
    L = _lib.lib()
    priors = _dev(priors, torch.float64)
    A = priors.shape[0]
    enc0 = torch.empty((A, 4), dtype=torch.float32, device=priors.device)
    _lib.check(L.ssd_encode_zero(_ptr(priors), A, _ptr(enc0), _stream()))
    ps = PriorSet(priors, enc0, grid)
    if verify:
        ps.verify_grid()
    return ps


class MatchWorkspace:
    """Caller-owned scratch, grown on demand."""

    def __init__(self):
        self.buf = None

    def get(self, nbytes, device):
        if self.buf is None or self.buf.numel() < nbytes or self.buf.device != device:
            self.buf = torch.empty((max(nbytes, 256),), dtype=torch.uint8, device=device)
        return self.buf


_default_ws = MatchWorkspace()


def match_encode(gt_box, gt_cls, gt_off, total_gt, max_nt, pset, thresh=0.5, out=None, ws=None, owner=None):
    """Batched match_bbox + apply_anchor_box (utils/bbox.py:44-101) on the device.

    gt_box f32[total_gt,4], gt_cls f32[total_gt], gt_off i32[B+1] device tensors; total_gt / max_nt are
    host ints.  `owner` (optional i32[B,A]) receives the matched gt row per anchor (-1 = none).
    Returns (cls i32[B,A], loc f32[B,A,4], mask u8[B,A])."""
    L = _lib.lib()
    B = gt_off.numel() - 1
    A = pset.A
    dev = pset.priors.device
    _dev(gt_off, torch.int32)
    if total_gt > 0:
        _dev(gt_box, torch.float32)
        _dev(gt_cls, torch.float32)
    if out is None:
        out = (torch.empty((B, A), dtype=torch.int32, device=dev),
               torch.empty((B, A, 4), dtype=torch.float32, device=dev),
               torch.empty((B, A), dtype=torch.uint8, device=dev))
    o_cls, o_loc, o_mask = out
    nbytes = L.ssd_match_encode_workspace_bytes(B, A, total_gt)
    wbuf = (ws or _default_ws).get(nbytes, dev)
    grid = ctypes.byref(pset.grid) if pset.grid is not None else None
    _lib.check(L.ssd_match_encode(_ptr(gt_box), _ptr(gt_cls), _ptr(gt_off), B, int(total_gt), int(max_nt),
                                  _ptr(pset.priors), _ptr(pset.enc_zero), A, grid, float(thresh),
                                  _ptr(o_cls), _ptr(o_loc), _ptr(o_mask), _ptr(owner), _ptr(wbuf), wbuf.numel(),
                                  _stream()))
    return o_cls, o_loc, o_mask


def pack_gt(boxes_list, cls_list, device="cuda"):
    """Concatenate per-image numpy gts into the (gt_box, gt_cls, gt_off, total, max_nt) batch form."""
    counts = [int(np.shape(b)[0]) for b in boxes_list]
    off = np.zeros(len(counts) + 1, np.int32)
    off[1:] = np.cumsum(counts)
    total = int(off[-1])
    if total:
        box = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in boxes_list], 0)
        cls = np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in cls_list], 0)
    else:
        box, cls = np.zeros((0, 4), np.float32), np.zeros((0,), np.float32)
    return (torch.from_numpy(box).to(device), torch.from_numpy(cls).to(device),
            torch.from_numpy(off).to(device), total, max(counts) if counts else 0)


def iou_n(b1, b2):
    """ssd_iou_n: f32 [n,4] vs f64 [n,4] device tensors -> f64 [n]."""
    L = _lib.lib()
    _dev(b1, torch.float32)
    _dev(b2, torch.float64)
    n = b1.shape[0]
    out = torch.empty((n,), dtype=torch.float64, device=b1.device)
    _lib.check(L.ssd_iou_n(_ptr(b1), _ptr(b2), n, _ptr(out), _stream()))
    return out


def apply_anchor_box(box, priors):
    """ssd_apply_anchor_box: f32 [n,4] vs f64 [n,4] device tensors -> f64 [n,4]."""
    L = _lib.lib()
    _dev(box, torch.float32)
    _dev(priors, torch.float64)
    n = box.shape[0]
    out = torch.empty((n, 4), dtype=torch.float64, device=box.device)
    _lib.check(L.ssd_apply_anchor_box(_ptr(box), _ptr(priors), n, _ptr(out), _stream()))
    return out


_loss_ws = MatchWorkspace()


def ssd_loss(conf, loc, gt_cls, gt_loc, gt_mask, grad_scale=1.0, ws=None):
    """ssd_loss_fwd_bwd (replaces _ssd_loss, models/ssd_model.py:341-396, and its gradient).

    conf [B,A,C], loc [B,A,4] (both f32 or both bf16); gt_* from match_encode.
    Returns (out8 f32[8] device tensor, dconf, dloc).  out8 = loc, pos, neg, total, P, N, tau, status."""
    L = _lib.lib()
    B, A, C = conf.shape
    assert conf.dtype == loc.dtype and conf.dtype in (torch.float32, torch.bfloat16)
    assert conf.is_cuda and conf.is_contiguous() and loc.is_contiguous()
    assert loc.shape == (B, A, 4) and gt_loc.shape == (B, A, 4)          # models/ssd_model.py:347-351
    assert gt_cls.shape == (B, A) and gt_mask.shape == (B, A)
    _dev(gt_cls, torch.int32); _dev(gt_loc, torch.float32); _dev(gt_mask, torch.uint8)
    dtype = 0 if conf.dtype == torch.float32 else 1
    out = torch.empty((8,), dtype=torch.float32, device=conf.device)
    dconf = torch.empty_like(conf)
    dloc = torch.empty_like(loc)
    nbytes = L.ssd_loss_workspace_bytes(B, A, C)
    wsobj = ws or _loss_ws
    wbuf = wsobj.get(nbytes, conf.device)
    wsobj.clean_key = None                         # (this form leaves the histogram words dirty: see ssd_loss_heads)
    _lib.check(L.ssd_loss_fwd_bwd(_ptr(conf), _ptr(loc), dtype, _ptr(gt_cls), _ptr(gt_loc), _ptr(gt_mask), B, A, C,
                                  float(grad_scale), _ptr(out), _ptr(dconf), _ptr(dloc), _ptr(wbuf), wbuf.numel(),
                                  _stream()))
    return out, dconf, dloc


class HeadGradBuffers:
    """Device buffers behind an ssd_head_grads: per level the compact gradient rows [B*hw, npad] bf16, both index maps
    and the row counts.  `hw`, `per_cell`, `npad` are per-level lists; sum(hw*per_cell) == A."""

    def __init__(self, B, hw, per_cell, npad, device="cuda"):
        self.B, self.hw, self.per_cell, self.npad = B, list(hw), list(per_cell), list(npad)
        self.levels = len(self.hw)
        assert self.levels <= _lib.SSD_MAX_LEVELS
        self.rows = [torch.empty((B * h, p), dtype=torch.bfloat16, device=device) for h, p in zip(self.hw, self.npad)]
        self.row_of_pixel = [torch.empty((B * h,), dtype=torch.int32, device=device) for h in self.hw]
        self.pixel_of_row = [torch.empty((B * h,), dtype=torch.int32, device=device) for h in self.hw]
        self.count = torch.zeros((_lib.SSD_MAX_LEVELS,), dtype=torch.int32, device=device)
        c = _lib.HeadGrads()
        c.levels = self.levels
        for l in range(self.levels):
            c.hw[l], c.per_cell[l], c.npad[l] = self.hw[l], self.per_cell[l], self.npad[l]
            c.rows[l], c.row_of_pixel[l], c.pixel_of_row[l] = (self.rows[l].data_ptr(), self.row_of_pixel[l].data_ptr(),
                                                               self.pixel_of_row[l].data_ptr())
        c.count = self.count.data_ptr()
        self.c = c

    def dense(self, classes):
        """(dloc [B,A,4], dconf [B,A,classes]) scattered back from the rows (tests; one host sync)."""
        B = self.B
        counts = self.count.cpu().tolist()
        locs, confs = [], []
        for l in range(self.levels):
            h, n, p = self.hw[l], self.per_cell[l], self.npad[l]
            full = torch.zeros((B * h, p), dtype=torch.bfloat16, device=self.rows[l].device)
            k = counts[l]
            full[self.pixel_of_row[l][:k].long()] = self.rows[l][:k]
            locs.append(full[:, :n * 4].reshape(B, h * n, 4))
            confs.append(full[:, n * 4:n * (4 + classes)].reshape(B, h * n, classes))
        return torch.cat(locs, 1), torch.cat(confs, 1)


def ssd_loss_heads(conf, loc, gt_cls, gt_loc, gt_mask, hgb, grad_scale=1.0, ws=None):
    """ssd_loss_fwd_bwd_heads: the loss of ssd_loss with its gradient as compact per-level pixel rows in `hgb`
    (HeadGradBuffers).  Returns out8 (device f32[8])."""
    L = _lib.lib()
    B, A, C = conf.shape
    assert conf.dtype == loc.dtype == torch.bfloat16 and conf.is_cuda and conf.is_contiguous() and loc.is_contiguous()
    assert loc.shape == (B, A, 4) and gt_loc.shape == (B, A, 4)          # models/ssd_model.py:347-351
    assert gt_cls.shape == (B, A) and gt_mask.shape == (B, A) and hgb.B == B
    _dev(gt_cls, torch.int32); _dev(gt_loc, torch.float32); _dev(gt_mask, torch.uint8)
    out = torch.empty((8,), dtype=torch.float32, device=conf.device)
    nbytes = L.ssd_loss_heads_workspace_bytes(B, A, C)
    wsobj = ws or _loss_ws
    wbuf = wsobj.get(nbytes, conf.device)
    # ws_clean: a completed call leaves the histogram words of this layout zeroed (its last launch does it), so the next call on
    # the same buffer, same B * A and same stream order needs no memset node; anything else in between resets the claim
    key = (B * A, wbuf.data_ptr(), wbuf.numel())
    clean = getattr(wsobj, "clean_key", None) == key
    wsobj.clean_key = None
    _lib.check(L.ssd_loss_fwd_bwd_heads(_ptr(conf), _ptr(loc), 1, _ptr(gt_cls), _ptr(gt_loc), _ptr(gt_mask), B, A, C,
                                        float(grad_scale), _ptr(out), ctypes.byref(hgb.c), _ptr(wbuf), wbuf.numel(),
                                        1 if clean else 0, _stream()))
    wsobj.clean_key = key
    return out


class LossSpec:
    """Which training loss a step uses.  kind "reference": the reference's _ssd_loss (ssd_loss / ssd_loss_heads; the other
    fields are not used).  kind "multibox": the SSD paper's loss (multibox_loss / multibox_loss_heads) with
    `neg_pos_ratio` mined negatives per positive, per image, and the box term weighted by `loc_weight`.  kind
    "softmax_focal": the softmax focal loss (softmax_focal_loss / softmax_focal_loss_heads) over every anchor with the
    focusing exponent `gamma` in [0, 8], the class balance `alpha` in [0, 1] (-1: off) and `loc_weight`; it mines nothing.
    `box`: the box term of "multibox" and "softmax_focal" -- "smooth_l1" of the four offsets, or the "giou" / "diou" / "ciou"
    loss of the decoded boxes (include/ssd_hip.h), which needs the priors at the call; the reference's loss has its L1 only."""
    KINDS = ("reference", "multibox", "softmax_focal")
    BOXES = ("smooth_l1", "giou", "diou", "ciou")                  # SSD_BOX_* in this order

    def __init__(self, kind="reference", neg_pos_ratio=3, loc_weight=1.0, gamma=2.0, alpha=0.25, box="smooth_l1"):
        if kind not in self.KINDS:
            raise ValueError("loss kind must be one of %s, not %r" % (", ".join(self.KINDS), kind))
        if not isinstance(box, str) or box not in self.BOXES:
            raise ValueError("box must be one of %s, not %r" % (", ".join(self.BOXES), box))
        if box != "smooth_l1" and kind == "reference":
            raise ValueError("box=%r needs the loss kind multibox or softmax_focal: the reference's loss has no such term" % (box,))
        if isinstance(neg_pos_ratio, bool) or not isinstance(neg_pos_ratio, (int, np.integer)) or neg_pos_ratio < 1:
            raise ValueError("neg_pos_ratio must be an integer >= 1, not %r" % (neg_pos_ratio,))
        for name, value in (("loc_weight", loc_weight), ("gamma", gamma), ("alpha", alpha)):
            if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
                raise ValueError("%s must be a number, not %r" % (name, value))
        if not (np.isfinite(loc_weight) and loc_weight >= 0):
            raise ValueError("loc_weight must be finite and >= 0, not %r" % (loc_weight,))
        if not (np.isfinite(gamma) and 0 <= gamma <= 8):
            raise ValueError("gamma must be finite and in [0, 8], not %r" % (gamma,))
        if not (0 <= alpha <= 1 or alpha == -1):
            raise ValueError("alpha must be in [0, 1], or -1 for no class balance, not %r" % (alpha,))
        self.kind = kind
        self.neg_pos_ratio = int(neg_pos_ratio)
        self.loc_weight = float(loc_weight)
        self.gamma = float(gamma)
        self.alpha = float(alpha)
        self.box = box

    @property
    def box_kind(self):
        """SSD_BOX_* of `box`."""
        return self.BOXES.index(self.box)

    @classmethod
    def of(cls, loss):
        """None / a kind name / a LossSpec -> LossSpec."""
        if loss is None:
            return cls()
        if isinstance(loss, cls):
            return loss
        if isinstance(loss, str):
            return cls(kind=loss)
        raise ValueError("loss must be None, a kind name or an ops.LossSpec, not %r" % (loss,))

    def __repr__(self):
        box = "" if self.box == "smooth_l1" else ", box=%r" % self.box
        if self.kind == "softmax_focal":
            return "LossSpec(kind=%r, gamma=%r, alpha=%r, loc_weight=%r%s)" % (self.kind, self.gamma, self.alpha, self.loc_weight, box)
        return "LossSpec(kind=%r, neg_pos_ratio=%d, loc_weight=%r%s)" % (self.kind, self.neg_pos_ratio, self.loc_weight, box)


class L2NormSpec:
    """The SSD paper's L2 normalisation of the first feature map (l2norm_fwd / l2norm_bwd): the learned per-channel scale
    starts at `init` (the paper's 20), `eps` is added to the sum of squares under the root (Caffe SSD's Normalize: 1e-10)."""

    def __init__(self, init=20.0, eps=1e-10):
        for name, v in (("init", init), ("eps", eps)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("l2norm %s must be a number, not %r" % (name, v))
            if not (np.isfinite(v) and v > 0):
                raise ValueError("l2norm %s must be finite and > 0, not %r" % (name, v))
        self.init = float(init)
        self.eps = float(eps)

    @classmethod
    def of(cls, v):
        """None / False -> None (the layer is off); True -> the defaults; a positive number -> that init; an L2NormSpec ->
        itself; a dict with the keys init / eps -> a spec.  ValueError for anything else."""
        if v is None or v is False:
            return None
        if v is True:
            return cls()
        if isinstance(v, cls):
            return v
        if isinstance(v, dict):
            unknown = sorted(set(v) - {"init", "eps"}, key=str)
            if unknown:
                raise ValueError("l2norm: unknown key(s) %s (known: init, eps)" % ", ".join(repr(k) for k in unknown))
            return cls(**v)
        if isinstance(v, (int, float, np.integer, np.floating)):
            return cls(init=v)
        raise ValueError("l2norm must be None, a bool, a positive number, a dict(init, eps) or an ops.L2NormSpec, not %r" % (v,))

    def __repr__(self):
        return "L2NormSpec(init=%r, eps=%r)" % (self.init, self.eps)


_l2norm_ws = MatchWorkspace()


def l2norm_fwd(x, scale, out=None, rnorm=None, eps=1e-10):
    """ssd_l2norm_fwd: y = bf16(scale_c x_pc / sqrt(sum_k x_pk^2 + eps)) over the last axis of x (bf16 [..., C]); scale fp32
    [C].  rnorm: None, an fp32 tensor of one element per pixel that receives 1 / sqrt(...), or True to allocate one -- then
    (y, rnorm) is returned instead of y.  NotImplementedError (SSD_ERR_UNSUPPORTED, nothing launched) unless C % 128 == 0 and
    128 <= C <= 1024."""
    L = _lib.lib()
    _bf(x)
    C = x.shape[-1]
    P = x.numel() // C
    if scale is not None:
        _dev(scale, torch.float32)
        assert scale.numel() == C
    if out is None:
        out = torch.empty_like(x)
    assert _bf(out).shape == x.shape
    want = rnorm is True
    if want:
        rnorm = torch.empty((P,), dtype=torch.float32, device=x.device)
    if rnorm is not None:
        assert _dev(rnorm, torch.float32).numel() == P
    rc = L.ssd_l2norm_fwd(_ptr(x), _ptr(scale), _ptr(out), _ptr(rnorm), P, C, float(eps), _stream())
    _lib.check(rc, unsupported="l2norm serves multiples of 128 channels in 128 .. 1024, not C = %d" % C)
    return (out, rnorm) if want else out


def l2norm_bwd(dy, x, scale, rnorm=None, out=None, accumulate=False, dscale=None, ws=None, eps=1e-10):
    """ssd_l2norm_bwd: the gradients of l2norm_fwd w.r.t. x (bf16 like x, into `out`; accumulate: added to its contents in fp32
    before the rounding) and w.r.t. scale (fp32 [C], written; bitwise reproducible).  rnorm: what l2norm_fwd saved, or None to
    recompute it from x (the same bits).  Returns (dx, dscale)."""
    L = _lib.lib()
    _bf(dy); _bf(x)
    assert dy.shape == x.shape
    C = x.shape[-1]
    P = x.numel() // C
    if scale is not None:
        _dev(scale, torch.float32)
        assert scale.numel() == C
    if rnorm is not None:
        assert _dev(rnorm, torch.float32).numel() == P
    if out is None:
        assert not accumulate
        out = torch.empty_like(x)
    assert _bf(out).shape == x.shape
    if dscale is None:
        dscale = torch.empty((C,), dtype=torch.float32, device=x.device)
    assert _dev(dscale, torch.float32).numel() == C
    wbuf = (ws or _l2norm_ws).get(L.ssd_l2norm_ws_bytes(P, C), x.device)
    rc = L.ssd_l2norm_bwd(_ptr(dy), _ptr(x), _ptr(scale), _ptr(rnorm), _ptr(out), 1 if accumulate else 0, _ptr(dscale),
                          _ptr(wbuf), wbuf.numel(), P, C, float(eps), _stream())
    _lib.check(rc, unsupported="l2norm serves multiples of 128 channels in 128 .. 1024, not C = %d" % C)
    return out, dscale


class BatchNormSpec:
    """Batch normalisation of the ResNet-50 SSD512 trunk in training mode (batchnorm_fwd_train / batchnorm_fwd_infer /
    batchnorm_bwd): `momentum` is the weight of the batch statistics in the running ones (PyTorch's convention and default),
    `eps` is added to the variance under the root."""

    def __init__(self, momentum=0.1, eps=1e-5):
        for name, v in (("momentum", momentum), ("eps", eps)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError("batchnorm %s must be a number, not %r" % (name, v))
            if not (np.isfinite(v) and v > 0):
                raise ValueError("batchnorm %s must be finite and > 0, not %r" % (name, v))
        if momentum > 1:
            raise ValueError("batchnorm momentum must lie in (0, 1], not %r" % (momentum,))
        self.momentum = float(momentum)
        self.eps = float(eps)

    @classmethod
    def of(cls, v):
        """None / False -> None (no batch normalisation); True -> the defaults; a BatchNormSpec -> itself; a dict with the
        keys momentum / eps -> a spec.  ValueError for anything else."""
        if v is None or v is False:
            return None
        if v is True:
            return cls()
        if isinstance(v, cls):
            return v
        if isinstance(v, dict):
            unknown = sorted(set(v) - {"momentum", "eps"}, key=str)
            if unknown:
                raise ValueError("batchnorm: unknown key(s) %s (known: momentum, eps)" % ", ".join(repr(k) for k in unknown))
            return cls(**v)
        raise ValueError("batchnorm must be None, a bool, a dict(momentum, eps) or an ops.BatchNormSpec, not %r" % (v,))

    def __repr__(self):
        return "BatchNormSpec(momentum=%r, eps=%r)" % (self.momentum, self.eps)


class NetworkSpec:
    """Which network SSDObjectDetectionModel builds and how it trains it.
      kind             "ssd300": the reference's 300 x 300 network (SSDEngine), the default; "vgg16_ssd300": the SSD paper's
                       VGG-16 SSD300 (SSDEngine on engine.VGG16_SSD300_TRUNK; bf16, no batchnorm); "mobilenet_v1_ssd300":
                       MobileNet-v1 SSD300 (SSDEngine on engine.MOBILENET_V1_SSD300_TRUNK: depthwise 3x3 + 1x1 blocks, 2268
                       anchors; bf16, no batchnorm, no l2norm, no fp8); "resnet50_ssd512": the ResNet-50 SSD512 network
                       (ResNet50SSDEngine)
      in_size          300 for ssd300, vgg16_ssd300 and mobilenet_v1_ssd300; 512 (default) or 256 for the ResNet
      batchnorm        ResNet only: anything BatchNormSpec.of takes (None / False: the folded network)
      precision        of the TRAINING forward: "bf16" or "mxfp8" (ResNet only; not together with batchnorm, whose engine has no
                       fp8 plan)
      dgrad_precision  of the data gradients behind an mxfp8 training forward: None (fp8 where planned), "bf16" or "mxfp8"
    """
    KINDS = ("ssd300", "resnet50_ssd512", "vgg16_ssd300", "mobilenet_v1_ssd300")
    FIELDS = ("kind", "in_size", "batchnorm", "precision", "dgrad_precision")
    IN_SIZES = {"ssd300": (300,), "resnet50_ssd512": (512, 256), "vgg16_ssd300": (300,), "mobilenet_v1_ssd300": (300,)}   # the first one is the default
    ENGINE_KINDS = ("ssd300", "vgg16_ssd300", "mobilenet_v1_ssd300")      # the networks SSDEngine runs: bf16 training, no batchnorm
    L2NORM_KINDS = ("ssd300", "vgg16_ssd300")                              # the networks SSDEngine runs: l2norm is its option

    def __init__(self, kind="ssd300", in_size=None, batchnorm=None, precision="bf16", dgrad_precision=None):
        if not isinstance(kind, str) or kind not in self.KINDS:
            raise ValueError("network kind must be one of %s, not %r" % (", ".join(self.KINDS), kind))
        sizes = self.IN_SIZES[kind]
        if in_size is None:
            in_size = sizes[0]
        if isinstance(in_size, bool) or not isinstance(in_size, (int, np.integer)) or int(in_size) not in sizes:
            raise ValueError("network in_size of %s must be %s, not %r" % (kind, " or ".join(str(s) for s in sizes), in_size))
        batchnorm = BatchNormSpec.of(batchnorm)
        if not isinstance(precision, str) or precision not in ("bf16", "mxfp8"):
            raise ValueError("network precision must be 'bf16' or 'mxfp8', not %r" % (precision,))
        if dgrad_precision is not None and (not isinstance(dgrad_precision, str) or dgrad_precision not in ("bf16", "mxfp8")):
            raise ValueError("network dgrad_precision must be None, 'bf16' or 'mxfp8', not %r" % (dgrad_precision,))
        if kind in self.ENGINE_KINDS:
            if batchnorm is not None:
                raise ValueError("network batchnorm: the %s network has no batch normalisation" % kind)
            if precision != "bf16" or dgrad_precision is not None:
                raise ValueError("network precision / dgrad_precision: the %s network trains in bf16 (precision=%r, "
                                 "dgrad_precision=%r)" % (kind, precision, dgrad_precision))
        if batchnorm is not None and precision == "mxfp8":
            raise ValueError("network batchnorm together with precision='mxfp8': a batchnorm engine has no fp8 training "
                             "forward (its fp8 inference runs on the folded network)")
        if dgrad_precision == "mxfp8" and precision != "mxfp8":
            raise ValueError("network dgrad_precision='mxfp8' needs precision='mxfp8': fp8 data gradients read what the fp8 "
                             "training forward writes")
        self.kind, self.in_size, self.batchnorm = kind, int(in_size), batchnorm
        self.precision, self.dgrad_precision = precision, dgrad_precision

    @classmethod
    def of(cls, v, l2norm=None):
        """None -> the ssd300 default; a kind name; a dict with keys of FIELDS; a NetworkSpec -> itself.  l2norm: the model's
        l2norm argument, which the ssd300 and vgg16_ssd300 networks serve (off unless asked for).  ValueError (naming the key
        or value) for anything else."""
        if v is None:
            spec = cls()
        elif isinstance(v, cls):
            spec = v
        elif isinstance(v, str):
            spec = cls(kind=v)
        elif isinstance(v, dict):
            unknown = sorted(set(v) - set(cls.FIELDS), key=str)
            if unknown:
                raise ValueError("network: unknown key(s) %s (known: %s)" % (", ".join(repr(k) for k in unknown),
                                                                            ", ".join(cls.FIELDS)))
            spec = cls(**v)
        else:
            raise ValueError("network must be None, a kind name, a dict or an ops.NetworkSpec, not %r" % (v,))
        if spec.kind not in cls.L2NORM_KINDS and L2NormSpec.of(l2norm) is not None:
            raise ValueError("l2norm together with network kind %r: L2Norm is wired for the networks %s only"
                             % (spec.kind, ", ".join(cls.L2NORM_KINDS)))
        return spec

    def as_dict(self):
        """Plain values only (what a checkpoint and config.json carry); NetworkSpec.of(d) gives the spec back."""
        bn = None if self.batchnorm is None else dict(momentum=self.batchnorm.momentum, eps=self.batchnorm.eps)
        return dict(kind=self.kind, in_size=self.in_size, batchnorm=bn, precision=self.precision,
                    dgrad_precision=self.dgrad_precision)

    def identity(self):
        """What makes two specs the same NETWORK (a checkpoint of one loads into the other): kind, input size and whether
        batch normalisation is live.  The precisions are how a run trains it, not what it is."""
        return (self.kind, self.in_size, self.batchnorm is not None)

    def describe(self):
        return "%s(in_size=%d%s)" % (self.kind, self.in_size, ", batchnorm" if self.batchnorm is not None else "")

    def __repr__(self):
        return "NetworkSpec(kind=%r, in_size=%d, batchnorm=%r, precision=%r, dgrad_precision=%r)" % (
            self.kind, self.in_size, self.batchnorm, self.precision, self.dgrad_precision)


_bn_ws = MatchWorkspace()
_BN_SHAPES = "batchnorm serves multiples of 64 channels in 64 .. 2048, not C = %d"


def _bn_vec(t, C):
    if t is not None:
        assert _dev(t, torch.float32).numel() == C
    return t


def batchnorm_fwd_train(x, gamma, beta, out=None, mean=None, rstd=None, running_mean=None, running_var=None, momentum=0.1,
                        eps=1e-5, relu=False, ws=None):
    """ssd_bn_fwd_train: y = bf16(gamma_c (x_pc - mu_c) rstd_c + beta_c), through max(., 0) where relu, with the statistics of
    the rows of x (bf16 [..., C]; mu the mean, rstd = 1 / sqrt(biased variance + eps), fp32, bitwise reproducible).  mean /
    rstd: fp32 [C] tensors that receive what batchnorm_bwd needs (allocated when None).  running_mean / running_var: both or
    neither; updated in place with weight `momentum` for the batch (the variance unbiased, P / (P - 1): PyTorch's
    convention).  Returns (y, mean, rstd).  NotImplementedError (SSD_ERR_UNSUPPORTED, nothing launched) unless C % 64 == 0
    and 64 <= C <= 2048."""
    L = _lib.lib()
    _bf(x)
    C = x.shape[-1]
    P = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    assert _bf(out).shape == x.shape
    if mean is None:
        mean = torch.empty((C,), dtype=torch.float32, device=x.device)
    if rstd is None:
        rstd = torch.empty((C,), dtype=torch.float32, device=x.device)
    for t in (gamma, beta, mean, rstd, running_mean, running_var):
        _bn_vec(t, C)
    wbuf = (ws or _bn_ws).get(L.ssd_bn_ws_bytes(P, C), x.device)
    rc = L.ssd_bn_fwd_train(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(mean), _ptr(rstd), _ptr(running_mean),
                            _ptr(running_var), float(momentum), float(eps), 1 if relu else 0, _ptr(wbuf), wbuf.numel(), P, C,
                            _stream())
    _lib.check(rc, unsupported=_BN_SHAPES % C)
    return out, mean, rstd


def batchnorm_fwd_infer(x, gamma, beta, running_mean, running_var, out=None, eps=1e-5, relu=False):
    """ssd_bn_fwd_infer: y = bf16(x a_c + b_c), through max(., 0) where relu, with a = gamma / sqrt(running_var + eps) and
    b = beta - running_mean a: one pass, no workspace.  Shapes and errors as batchnorm_fwd_train."""
    L = _lib.lib()
    _bf(x)
    C = x.shape[-1]
    P = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    assert _bf(out).shape == x.shape
    for t in (gamma, beta, running_mean, running_var):
        _bn_vec(t, C)
    rc = L.ssd_bn_fwd_infer(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(out), float(eps),
                            1 if relu else 0, P, C, _stream())
    _lib.check(rc, unsupported=_BN_SHAPES % C)
    return out


def batchnorm_bwd(dy, x, gamma, mean, rstd, out=None, dgamma=None, dbeta=None, ws=None):
    """ssd_bn_bwd: the gradients of batchnorm_fwd_train w.r.t. x (bf16 like x, into `out`), gamma and beta (fp32 [C], written,
    bitwise reproducible) from dy -- which the caller has masked by the layer's own ReLU already -- x and the mean / rstd the
    forward pass saved.  Returns (dx, dgamma, dbeta)."""
    L = _lib.lib()
    _bf(dy); _bf(x)
    assert dy.shape == x.shape
    C = x.shape[-1]
    P = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    assert _bf(out).shape == x.shape
    if dgamma is None:
        dgamma = torch.empty((C,), dtype=torch.float32, device=x.device)
    if dbeta is None:
        dbeta = torch.empty((C,), dtype=torch.float32, device=x.device)
    for t in (gamma, mean, rstd, dgamma, dbeta):
        _bn_vec(t, C)
    wbuf = (ws or _bn_ws).get(L.ssd_bn_ws_bytes(P, C), x.device)
    rc = L.ssd_bn_bwd(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(out), _ptr(dgamma), _ptr(dbeta), _ptr(wbuf),
                      wbuf.numel(), P, C, _stream())
    _lib.check(rc, unsupported=_BN_SHAPES % C)
    return out, dgamma, dbeta


_multibox_ws = MatchWorkspace()


def _box_priors(spec, priors, A, device):
    """The priors argument of the _box entries: a PriorSet or an f64 [A,4] device tensor, required by the IoU kinds (ValueError
    without it, or with another shape); None stays None for smooth L1, which does not read it."""
    if priors is None:
        if spec.box != "smooth_l1":
            raise ValueError("box=%r needs priors (a PriorSet or an f64 [A,4] device tensor)" % (spec.box,))
        return None
    t = priors.priors if isinstance(priors, PriorSet) else priors
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (A, 4):
        raise ValueError("priors must be a PriorSet or a tensor of shape [%d, 4], not %r" % (A, getattr(t, "shape", t)))
    if t.dtype != torch.float64 or not t.is_contiguous() or t.device != device:
        raise ValueError("priors must be a contiguous float64 tensor on %s, not %s on %s" % (device, t.dtype, t.device))
    return t


def _multibox_args(conf, loc, gt_cls, gt_loc, gt_mask, neg_pos_ratio, loc_weight, box="smooth_l1"):
    B, A, C = conf.shape
    assert conf.is_cuda and conf.is_contiguous() and loc.is_contiguous()
    assert loc.shape == (B, A, 4) and gt_loc.shape == (B, A, 4)
    assert gt_cls.shape == (B, A) and gt_mask.shape == (B, A)
    _dev(gt_cls, torch.int32); _dev(gt_loc, torch.float32); _dev(gt_mask, torch.uint8)
    spec = LossSpec("multibox", neg_pos_ratio, loc_weight, box=box)     # ValueError for bad values, before anything is allocated
    return B, A, C, spec


def multibox_loss(conf, loc, gt_cls, gt_loc, gt_mask, neg_pos_ratio=3, loc_weight=1.0, grad_scale=1.0, ws=None,
                  box="smooth_l1", priors=None):
    """ssd_multibox_loss_box_fwd_bwd: the SSD paper's loss (per-image hard-negative mining, smooth L1, every term over P) and its
    gradient.  Arguments as ssd_loss.  Returns (out8 f32[8] device tensor, dconf, dloc); out8 = loc, pos, neg, total, P, N,
    tau_min, status.  box: "smooth_l1", or "giou" / "diou" / "ciou" of the boxes decoded with `priors` (a PriorSet or an f64
    [A,4] device tensor; ValueError without them)."""
    L = _lib.lib()
    B, A, C, spec = _multibox_args(conf, loc, gt_cls, gt_loc, gt_mask, neg_pos_ratio, loc_weight, box)
    pri = _box_priors(spec, priors, A, conf.device)
    assert conf.dtype == loc.dtype and conf.dtype in (torch.float32, torch.bfloat16)
    dtype = 0 if conf.dtype == torch.float32 else 1
    out = torch.empty((8,), dtype=torch.float32, device=conf.device)
    dconf = torch.empty_like(conf)
    dloc = torch.empty_like(loc)
    wsobj = ws or _multibox_ws
    wbuf = wsobj.get(L.ssd_multibox_loss_workspace_bytes(B, A, C), conf.device)
    wsobj.clean_key = None                         # (a buffer shared with ssd_loss_heads no longer holds its zeroed words)
    _lib.check(L.ssd_multibox_loss_box_fwd_bwd(_ptr(conf), _ptr(loc), dtype, _ptr(gt_cls), _ptr(gt_loc), _ptr(gt_mask), B, A, C,
                                               spec.neg_pos_ratio, spec.loc_weight, float(grad_scale), _ptr(out), _ptr(dconf),
                                               _ptr(dloc), _ptr(wbuf), wbuf.numel(), _stream(), spec.box_kind,
                                               None if pri is None else _ptr(pri)))
    return out, dconf, dloc


def multibox_loss_heads(conf, loc, gt_cls, gt_loc, gt_mask, hgb, neg_pos_ratio=3, loc_weight=1.0, grad_scale=1.0, ws=None,
                        box="smooth_l1", priors=None):
    """ssd_multibox_loss_box_fwd_bwd_heads: the loss of multibox_loss with its gradient as compact per-level pixel rows in `hgb`
    (HeadGradBuffers; bf16 only).  Returns out8 (device f32[8])."""
    L = _lib.lib()
    B, A, C, spec = _multibox_args(conf, loc, gt_cls, gt_loc, gt_mask, neg_pos_ratio, loc_weight, box)
    pri = _box_priors(spec, priors, A, conf.device)
    assert conf.dtype == loc.dtype == torch.bfloat16 and hgb.B == B
    out = torch.empty((8,), dtype=torch.float32, device=conf.device)
    wsobj = ws or _multibox_ws
    wbuf = wsobj.get(L.ssd_multibox_loss_heads_workspace_bytes(B, A, C), conf.device)
    wsobj.clean_key = None
    _lib.check(L.ssd_multibox_loss_box_fwd_bwd_heads(_ptr(conf), _ptr(loc), 1, _ptr(gt_cls), _ptr(gt_loc), _ptr(gt_mask), B, A,
                                                     C, spec.neg_pos_ratio, spec.loc_weight, float(grad_scale), _ptr(out),
                                                     ctypes.byref(hgb.c), _ptr(wbuf), wbuf.numel(), _stream(), spec.box_kind,
                                                     None if pri is None else _ptr(pri)))
    return out


_focal_ws = MatchWorkspace()


def _softmax_focal_args(conf, loc, gt_cls, gt_loc, gt_mask, gamma, alpha, loc_weight, box="smooth_l1"):
    B, A, C = conf.shape
    assert conf.is_cuda and conf.is_contiguous() and loc.is_contiguous()
    assert loc.shape == (B, A, 4) and gt_loc.shape == (B, A, 4)
    assert gt_cls.shape == (B, A) and gt_mask.shape == (B, A)
    _dev(gt_cls, torch.int32); _dev(gt_loc, torch.float32); _dev(gt_mask, torch.uint8)
    spec = LossSpec("softmax_focal", loc_weight=loc_weight, gamma=gamma, alpha=alpha, box=box)   # ValueError before anything is allocated
    return B, A, C, spec


def softmax_focal_loss(conf, loc, gt_cls, gt_loc, gt_mask, gamma=2.0, alpha=0.25, loc_weight=1.0, grad_scale=1.0, ws=None,
                       box="smooth_l1", priors=None):
    """ssd_softmax_focal_loss_box_fwd_bwd: the softmax focal loss over every anchor (background = class C-1; alpha=-1: no class
    balance), the MultiBox box term (`box`, `priors`: as multibox_loss), every term over P, and its gradient.  Arguments as
    ssd_loss.  Returns (out8 f32[8] device tensor, dconf, dloc); out8 = loc, pos, neg, total, P, N = B*A - P, 0, status."""
    L = _lib.lib()
    B, A, C, spec = _softmax_focal_args(conf, loc, gt_cls, gt_loc, gt_mask, gamma, alpha, loc_weight, box)
    pri = _box_priors(spec, priors, A, conf.device)
    assert conf.dtype == loc.dtype and conf.dtype in (torch.float32, torch.bfloat16)
    dtype = 0 if conf.dtype == torch.float32 else 1
    out = torch.empty((8,), dtype=torch.float32, device=conf.device)
    dconf = torch.empty_like(conf)
    dloc = torch.empty_like(loc)
    wsobj = ws or _focal_ws
    wbuf = wsobj.get(L.ssd_softmax_focal_loss_workspace_bytes(B, A, C), conf.device)
    wsobj.clean_key = None                         # (a buffer shared with ssd_loss_heads no longer holds its zeroed words)
    _lib.check(L.ssd_softmax_focal_loss_box_fwd_bwd(_ptr(conf), _ptr(loc), dtype, _ptr(gt_cls), _ptr(gt_loc), _ptr(gt_mask), B, A,
                                                    C, spec.gamma, spec.alpha, spec.loc_weight, float(grad_scale), _ptr(out),
                                                    _ptr(dconf), _ptr(dloc), _ptr(wbuf), wbuf.numel(), _stream(), spec.box_kind,
                                                    None if pri is None else _ptr(pri)))
    return out, dconf, dloc


def softmax_focal_loss_heads(conf, loc, gt_cls, gt_loc, gt_mask, hgb, gamma=2.0, alpha=0.25, loc_weight=1.0, grad_scale=1.0,
                             ws=None, box="smooth_l1", priors=None):
    """ssd_softmax_focal_loss_box_fwd_bwd_heads: the loss of softmax_focal_loss with its gradient as per-level pixel rows in `hgb`
    (HeadGradBuffers; bf16 only): every pixel is a row, the maps are the identity.  Returns out8 (device f32[8])."""
    L = _lib.lib()
    B, A, C, spec = _softmax_focal_args(conf, loc, gt_cls, gt_loc, gt_mask, gamma, alpha, loc_weight, box)
    pri = _box_priors(spec, priors, A, conf.device)
    assert conf.dtype == loc.dtype == torch.bfloat16 and hgb.B == B
    out = torch.empty((8,), dtype=torch.float32, device=conf.device)
    wsobj = ws or _focal_ws
    wbuf = wsobj.get(L.ssd_softmax_focal_loss_heads_workspace_bytes(B, A, C), conf.device)
    wsobj.clean_key = None
    _lib.check(L.ssd_softmax_focal_loss_box_fwd_bwd_heads(_ptr(conf), _ptr(loc), 1, _ptr(gt_cls), _ptr(gt_loc), _ptr(gt_mask), B,
                                                          A, C, spec.gamma, spec.alpha, spec.loc_weight, float(grad_scale),
                                                          _ptr(out), ctypes.byref(hgb.c), _ptr(wbuf), wbuf.numel(), _stream(),
                                                          spec.box_kind, None if pri is None else _ptr(pri)))
    return out


def head_layers(x, w_tap, dx, dw, dbias, cout, relu_bits=None, relu_src=None):
    """ssd_head_layers from per-level lists of tensors (x bf16 [B,H,W,Cin]; w_tap bf16 [3,3,Cin,npad]; dx like x; dw f32
    [cout,3,3,Cin]; dbias f32 [cout] or None).  Returns (struct, keep-alive list)."""
    c = _lib.HeadLayers()
    c.levels = len(x)
    keep = []
    for l, xl in enumerate(x):
        _bf(xl); _bf(w_tap[l]); _bf(dx[l])
        _, H, W, Cin = xl.shape
        assert w_tap[l].shape[:3] == (3, 3, Cin) and dx[l].shape == xl.shape and dw[l].is_contiguous()
        c.H[l], c.W[l], c.Cin[l], c.cout[l] = H, W, Cin, cout[l]
        c.x[l], c.w_tap[l], c.dx[l], c.dw[l] = xl.data_ptr(), w_tap[l].data_ptr(), dx[l].data_ptr(), dw[l].data_ptr()
        c.dbias[l] = dbias[l].data_ptr() if dbias is not None and dbias[l] is not None else None
        rb = relu_bits[l] if relu_bits is not None else None
        rs = relu_src[l] if relu_src is not None else None
        c.relu_bits[l] = rb.data_ptr() if rb is not None else None
        c.relu_src[l] = rs.data_ptr() if rs is not None else None
        keep += [xl, w_tap[l], dx[l], dw[l], rb, rs]
    return c, keep


_heads_z_ws = MatchWorkspace()
_heads_w_ws = MatchWorkspace()


def heads_bwd_data_sparse(hgb, hl, ws=None, levels=None):
    """levels: None = every level, else the levels of this call (ssd_heads_bwd_data_sparse_levels; calls with disjoint sets may
    share `ws` on two streams)."""
    L = _lib.lib()
    nbytes = L.ssd_heads_bwd_data_sparse_workspace_bytes(hgb.B, ctypes.byref(hl))
    wbuf = (ws or _heads_z_ws).get(nbytes, hgb.count.device)
    if levels is None:
        _lib.check(L.ssd_heads_bwd_data_sparse(ctypes.byref(hgb.c), ctypes.byref(hl), hgb.B, _ptr(wbuf), wbuf.numel(), _stream()))
        return
    mask = 0
    for l in levels:
        mask |= 1 << int(l)
    _lib.check(L.ssd_heads_bwd_data_sparse_levels(ctypes.byref(hgb.c), ctypes.byref(hl), hgb.B, mask, _ptr(wbuf), wbuf.numel(), _stream()))


def heads_bwd_weight_sparse(hgb, hl, ws=None):
    L = _lib.lib()
    nbytes = L.ssd_heads_bwd_weight_sparse_workspace_bytes(hgb.B, ctypes.byref(hgb.c), ctypes.byref(hl))
    wbuf = (ws or _heads_w_ws).get(nbytes, hgb.count.device)
    _lib.check(L.ssd_heads_bwd_weight_sparse(ctypes.byref(hgb.c), ctypes.byref(hl), hgb.B, _ptr(wbuf), wbuf.numel(), _stream()))


def weight_transpose_tap(w, cout_pad=None, out=None):
    """w bf16 [Cout,3,3,Cin] -> tap-major transposed copy [3,3,Cin,Cout_pad] (not flipped): the operand of the sparse head
    data gradient.  One-tensor call of ssd_weight_transpose_batched."""
    L = _lib.lib()
    _bf(w)
    Cout, k, _, Cin = w.shape
    cout_pad = cout_pad or (Cout + 7) // 8 * 8
    if out is None:
        out = torch.empty((k, k, Cin, cout_pad), dtype=torch.bfloat16, device=w.device)
    desc = torch.tensor([[w.data_ptr(), out.data_ptr(), Cout, k | 0x100, Cin, cout_pad]], dtype=torch.int64, device=w.device)
    tiles = ((cout_pad + 31) // 32) * ((Cin + 31) // 32) * k * k
    _lib.check(L.ssd_weight_transpose_batched(_ptr(desc), 1, tiles, _stream()))
    return out


def score_decode(conf, loc, pset, score_thresh=0.5, in_size=300.0):
    """ssd_score_decode (replaces visualize's scoring, models/ssd_model.py:479-488, + decode :466-467).
    Returns (score f32[B,A], cls i32[B,A], box f32[B,A,4] pixels, cand u8[B,A])."""
    L = _lib.lib()
    B, A, C = conf.shape
    assert conf.dtype == loc.dtype and conf.dtype in (torch.float32, torch.bfloat16)
    assert conf.is_cuda and conf.is_contiguous() and loc.is_contiguous() and A == pset.A
    dev = conf.device
    score = torch.empty((B, A), dtype=torch.float32, device=dev)
    cls = torch.empty((B, A), dtype=torch.int32, device=dev)
    box = torch.empty((B, A, 4), dtype=torch.float32, device=dev)
    cand = torch.empty((B, A), dtype=torch.uint8, device=dev)
    _lib.check(L.ssd_score_decode(_ptr(conf), _ptr(loc), 0 if conf.dtype == torch.float32 else 1, _ptr(pset.priors),
                                  B, A, C, float(score_thresh), float(in_size), _ptr(score), _ptr(cls), _ptr(box),
                                  _ptr(cand), _stream()))
    return score, cls, box, cand


def nms(score, cls, box, cand, iou_thresh=0.45, max_cand=400, want_count=False):
    """ssd_nms: per-image per-class greedy NMS (build-defined; the reference has none).
    Returns keep u8[B,A] (and keep_count i32[B] if want_count)."""
    L = _lib.lib()
    B, A = score.shape
    _dev(score, torch.float32); _dev(cls, torch.int32); _dev(box, torch.float32); _dev(cand, torch.uint8)
    keep = torch.empty((B, A), dtype=torch.uint8, device=score.device)
    count = torch.empty((B,), dtype=torch.int32, device=score.device) if want_count else None
    _lib.check(L.ssd_nms(_ptr(score), _ptr(cls), _ptr(box), _ptr(cand), B, A, float(iou_thresh), int(max_cand),
                         _ptr(keep), _ptr(count), _stream()))
    return (keep, count) if want_count else keep


def class_scores(conf):
    """ssd_class_scores: the float32 softmax probability of every foreground class, prob f32 [B,A,C-1] -- bit for bit the
    scores detect_pairs reports for the same (anchor, class)."""
    L = _lib.lib()
    B, A, C = conf.shape
    assert conf.dtype in (torch.float32, torch.bfloat16) and conf.is_cuda and conf.is_contiguous()
    prob = torch.empty((B, A, max(C - 1, 0)), dtype=torch.float32, device=conf.device)
    _lib.check(L.ssd_class_scores(_ptr(conf), 0 if conf.dtype == torch.float32 else 1, B, A, C, _ptr(prob), _stream()))
    return prob


def detect_max_candidates():
    return int(_lib.lib().ssd_detect_max_candidates())


def detect_max_keep():
    return int(_lib.lib().ssd_detect_max_keep())


DetectPairs = collections.namedtuple("DetectPairs", "n_det score cls anchor box valid n_cand")
_detect_ws = MatchWorkspace()


def detect_pairs(conf, loc, pset, score_thresh=0.01, iou_thresh=0.45, max_cand=None, keep_top_k=200, in_size=300.0, ws=None):
    """ssd_detect_pairs: the multi-label detection output (build-defined; the reference has none).  Every (anchor, class) pair
    with softmax probability > score_thresh is a candidate (no background test); the first max_cand (None: the library
    maximum) by (score desc, anchor asc, class asc) go through per-class greedy NMS; the kept pairs come out in that order,
    cut to keep_top_k = K rows per image.  Returns DetectPairs(n_det i32 [B], score f32 [B,K], cls i32 [B,K], anchor i32 [B,K],
    box f32 [B,K,4] pixels, valid u8 [B,K], n_cand i32 [B]); rows at or beyond n_det hold score 0, class -1, anchor -1,
    box 0, valid 0.  Raises ValueError for max_cand / keep_top_k out of range."""
    L = _lib.lib()
    B, A, C = conf.shape
    assert conf.dtype == loc.dtype and conf.dtype in (torch.float32, torch.bfloat16)
    assert conf.is_cuda and conf.is_contiguous() and loc.is_contiguous() and A == pset.A
    dev = conf.device
    max_cand = detect_max_candidates() if max_cand is None else int(max_cand)
    K = int(keep_top_k)
    rows = max(K, 1)
    n_cand = torch.empty((B,), dtype=torch.int32, device=dev)
    n_det = torch.empty((B,), dtype=torch.int32, device=dev)
    score = torch.empty((B, rows), dtype=torch.float32, device=dev)
    cls = torch.empty((B, rows), dtype=torch.int32, device=dev)
    anchor = torch.empty((B, rows), dtype=torch.int32, device=dev)
    box = torch.empty((B, rows, 4), dtype=torch.float32, device=dev)
    valid = torch.empty((B, rows), dtype=torch.uint8, device=dev)
    nbytes = L.ssd_detect_pairs_workspace_bytes(B, A, C)
    wbuf = (ws or _detect_ws).get(nbytes, dev)
    _lib.check(L.ssd_detect_pairs(_ptr(conf), _ptr(loc), 0 if conf.dtype == torch.float32 else 1, _ptr(pset.priors), B, A, C,
                                  float(score_thresh), float(in_size), float(iou_thresh), max_cand, K, _ptr(n_cand),
                                  _ptr(n_det), _ptr(score), _ptr(cls), _ptr(anchor), _ptr(box), _ptr(valid), _ptr(wbuf),
                                  wbuf.numel(), _stream()))
    return DetectPairs(n_det, score, cls, anchor, box, valid, n_cand)


def eval_max_dets():
    return int(_lib.lib().ssd_eval_max_dets())


_EVAL_THRESHOLDS = np.linspace(0.5, 0.95, 10)          # utils.metrics.IOU_THRESHOLDS / RECALL_POINTS: passed in, not recomputed
_EVAL_RECALL_POINTS = np.linspace(0.0, 1.0, 101)


def eval_match(score, cls, box, keep, gt_cls, gt_box, gt_off, max_dets=100):
    """ssd_eval_match: top-max_dets kept detections per image + greedy COCO matching at the ten thresholds, behind
    score_decode + nms.  gt_cls i32 [total], gt_box f64 [total,4] pixels, gt_off i32 [B+1].  Returns (n_det i32 [B],
    det_score f32 [B,max_dets], det_cls i32 [B,max_dets], det_box f32 [B,max_dets,4], det_flags int16 [B,max_dets] holding the
    uint16 flag words: bit t = true positive at threshold t)."""
    L = _lib.lib()
    B, A = score.shape
    _dev(score, torch.float32); _dev(cls, torch.int32); _dev(box, torch.float32); _dev(keep, torch.uint8)
    _dev(gt_cls, torch.int32); _dev(gt_box, torch.float64); _dev(gt_off, torch.int32)
    assert gt_off.numel() == B + 1 and gt_box.shape[0] == gt_cls.shape[0]
    max_dets = int(max_dets)
    dev = score.device
    md = max(max_dets, 1)
    n_det = torch.empty((B,), dtype=torch.int32, device=dev)
    det_score = torch.empty((B, md), dtype=torch.float32, device=dev)
    det_cls = torch.empty((B, md), dtype=torch.int32, device=dev)
    det_box = torch.empty((B, md, 4), dtype=torch.float32, device=dev)
    det_flags = torch.empty((B, md), dtype=torch.int16, device=dev)
    thr = _EVAL_THRESHOLDS.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    _lib.check(L.ssd_eval_match(_ptr(score), _ptr(cls), _ptr(box), _ptr(keep), B, A, _ptr(gt_cls), _ptr(gt_box), _ptr(gt_off),
                                thr, max_dets, _ptr(n_det), _ptr(det_score), _ptr(det_cls), _ptr(det_box), _ptr(det_flags),
                                _stream()))
    return n_det, det_score, det_cls, det_box, det_flags


def eval_ap(flags_sorted, seg_off, n_gt):
    """ssd_eval_ap: flags int16 [N] (uint16 words) sorted by (class, score desc, image, rank), seg_off i32 [C+1], n_gt i32 [C]
    -> AP f64 [C,10] (101-point, per class and threshold; 0 for classes without ground truth)."""
    L = _lib.lib()
    _dev(flags_sorted, torch.int16); _dev(seg_off, torch.int32); _dev(n_gt, torch.int32)
    C = n_gt.numel()
    assert seg_off.numel() == C + 1
    if flags_sorted.numel() == 0:                      # the entry point wants a pointer even when there is nothing to read
        flags_sorted = torch.zeros((1,), dtype=torch.int16, device=n_gt.device)
    ap = torch.empty((C, 10), dtype=torch.float64, device=n_gt.device)
    pts = _EVAL_RECALL_POINTS.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    _lib.check(L.ssd_eval_ap(_ptr(flags_sorted), _ptr(seg_off), _ptr(n_gt), C, pts, _ptr(ap), _stream()))
    return ap


COCO_AREA_RANGES = ((0, 1e10), (0, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e10))     # utils.metrics.COCO_AREA_RANGES
EvalMatchCoco = collections.namedtuple("EvalMatchCoco", "n_det score cls box flags tp ig pos gt_ignore")


def eval_match_coco(score, cls, box, keep, gt_cls, gt_box, gt_off, max_dets=100, gt_crowd=None, area_scale=None,
                    area_ranges=COCO_AREA_RANGES):
    """ssd_eval_match_coco: eval_match with COCO's area ranges and crowd boxes (utils.metrics.coco_match_image).  gt_crowd u8
    [total] or None (no crowd box), area_scale f64 [B] or None (1), area_ranges four (lo, hi) pairs.  Returns
    EvalMatchCoco(n_det i32 [B], score f32 [B,max_dets], cls i32 [B,max_dets], box f32 [B,max_dets,4], flags int16
    [B,max_dets], tp int16 [B,max_dets,4], ig int16 [B,max_dets,4], pos i32 [B,max_dets], gt_ignore u8 [total]); the int16
    tensors hold uint16 words: bit t = threshold t; the last axis of tp / ig is the area range; bit a of gt_ignore = range a."""
    L = _lib.lib()
    B, A = score.shape
    _dev(score, torch.float32); _dev(cls, torch.int32); _dev(box, torch.float32); _dev(keep, torch.uint8)
    _dev(gt_cls, torch.int32); _dev(gt_box, torch.float64); _dev(gt_off, torch.int32)
    assert gt_off.numel() == B + 1 and gt_box.shape[0] == gt_cls.shape[0]
    if gt_crowd is not None:
        _dev(gt_crowd, torch.uint8)
        assert gt_crowd.numel() == gt_cls.numel()
    if area_scale is not None:
        _dev(area_scale, torch.float64)
        assert area_scale.numel() == B
    rng = np.ascontiguousarray(np.asarray(area_ranges, np.float64).reshape(-1))
    assert rng.size == 8
    max_dets = int(max_dets)
    dev = score.device
    md = max(max_dets, 1)
    n_det = torch.empty((B,), dtype=torch.int32, device=dev)
    det_score = torch.empty((B, md), dtype=torch.float32, device=dev)
    det_cls = torch.empty((B, md), dtype=torch.int32, device=dev)
    det_box = torch.empty((B, md, 4), dtype=torch.float32, device=dev)
    det_flags = torch.empty((B, md), dtype=torch.int16, device=dev)
    det_tp = torch.empty((B, md, 4), dtype=torch.int16, device=dev)
    det_ig = torch.empty((B, md, 4), dtype=torch.int16, device=dev)
    det_pos = torch.empty((B, md), dtype=torch.int32, device=dev)
    gt_ignore = torch.empty((gt_cls.numel(),), dtype=torch.uint8, device=dev)
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(L.ssd_eval_match_coco(_ptr(score), _ptr(cls), _ptr(box), _ptr(keep), B, A, _ptr(gt_cls), _ptr(gt_box),
                                     _ptr(gt_off), _ptr(gt_crowd) if gt_crowd is not None else None,
                                     _ptr(area_scale) if area_scale is not None else None, rng.ctypes.data_as(dp),
                                     _EVAL_THRESHOLDS.ctypes.data_as(dp), max_dets, _ptr(n_det), _ptr(det_score), _ptr(det_cls),
                                     _ptr(det_box), _ptr(det_flags), _ptr(det_tp), _ptr(det_ig), _ptr(det_pos), _ptr(gt_ignore),
                                     _stream()))
    return EvalMatchCoco(n_det, det_score, det_cls, det_box, det_flags, det_tp, det_ig, det_pos, gt_ignore)


def eval_ap_coco(tp_sorted, ig_sorted, pos_sorted, seg_off, n_gt, max_dets=100):
    """ssd_eval_ap_coco: tp / ig int16 [N,4] (uint16 words per area range) and pos i32 [N] sorted by (class, score desc, image,
    rank), seg_off i32 [C+1], n_gt i32 [4,C] (non-ignored ground truths per range and class) -> (ap f64 [C,4,10], tp_count i32
    [C,4,3,10]: true positives not ignored with pos < (1, 10, max_dets)); zeros where n_gt == 0."""
    L = _lib.lib()
    _dev(tp_sorted, torch.int16); _dev(ig_sorted, torch.int16); _dev(pos_sorted, torch.int32)
    _dev(seg_off, torch.int32); _dev(n_gt, torch.int32)
    C = n_gt.shape[1]
    assert n_gt.shape[0] == 4 and seg_off.numel() == C + 1
    assert tp_sorted.shape == ig_sorted.shape == (pos_sorted.numel(), 4)
    dev = n_gt.device
    if pos_sorted.numel() == 0:                        # the entry point wants pointers even when there is nothing to read
        tp_sorted = ig_sorted = torch.zeros((1, 4), dtype=torch.int16, device=dev)
        pos_sorted = torch.zeros((1,), dtype=torch.int32, device=dev)
    ap = torch.empty((C, 4, 10), dtype=torch.float64, device=dev)
    tp_count = torch.empty((C, 4, 3, 10), dtype=torch.int32, device=dev)
    pts = _EVAL_RECALL_POINTS.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    _lib.check(L.ssd_eval_ap_coco(_ptr(tp_sorted), _ptr(ig_sorted), _ptr(pos_sorted), _ptr(seg_off), _ptr(n_gt), C, int(max_dets),
                                  pts, _ptr(ap), _ptr(tp_count), _stream()))
    return ap, tp_count


def eval_voc_max_dets():
    return int(_lib.lib().ssd_eval_voc_max_dets())


_EVAL_VOC_RECALL_POINTS = np.arange(11) / 10.0         # utils.metrics.VOC_RECALL_POINTS: passed in, not recomputed
EvalMatchVoc = collections.namedtuple("EvalMatchVoc", "n_det score cls box flags gt")


def eval_match_voc(score, cls, box, keep, gt_cls, gt_box, gt_off, max_dets=100, gt_difficult=None, iou_thresh=0.5):
    """ssd_eval_match_voc: eval_match's selection, then VOCdevkit's matching at one threshold (utils.metrics.voc_match_image).
    gt_difficult u8 [total] or None (no difficult box).  Returns EvalMatchVoc(n_det i32 [B], score f32 [B,max_dets], cls i32
    [B,max_dets], box f32 [B,max_dets,4], flags u8 [B,max_dets]: bit 0 true positive, bit 1 ignored, gt i32 [B,max_dets]: the
    box of highest IoU as an index into the image's boxes, -1 when that IoU is below iou_thresh)."""
    L = _lib.lib()
    B, A = score.shape
    _dev(score, torch.float32); _dev(cls, torch.int32); _dev(box, torch.float32); _dev(keep, torch.uint8)
    _dev(gt_cls, torch.int32); _dev(gt_box, torch.float64); _dev(gt_off, torch.int32)
    assert gt_off.numel() == B + 1 and gt_box.shape[0] == gt_cls.shape[0]
    if gt_difficult is not None:
        _dev(gt_difficult, torch.uint8)
        assert gt_difficult.numel() == gt_cls.numel()
    max_dets = int(max_dets)
    dev = score.device
    md = max(max_dets, 1)
    n_det = torch.empty((B,), dtype=torch.int32, device=dev)
    det_score = torch.empty((B, md), dtype=torch.float32, device=dev)
    det_cls = torch.empty((B, md), dtype=torch.int32, device=dev)
    det_box = torch.empty((B, md, 4), dtype=torch.float32, device=dev)
    det_flags = torch.empty((B, md), dtype=torch.uint8, device=dev)
    det_gt = torch.empty((B, md), dtype=torch.int32, device=dev)
    _lib.check(L.ssd_eval_match_voc(_ptr(score), _ptr(cls), _ptr(box), _ptr(keep), B, A, _ptr(gt_cls), _ptr(gt_box), _ptr(gt_off),
                                    _ptr(gt_difficult) if gt_difficult is not None else None, float(iou_thresh), max_dets,
                                    _ptr(n_det), _ptr(det_score), _ptr(det_cls), _ptr(det_box), _ptr(det_flags), _ptr(det_gt),
                                    _stream()))
    return EvalMatchVoc(n_det, det_score, det_cls, det_box, det_flags, det_gt)


def eval_ap_voc(flags_sorted, seg_off, n_pos, year="07"):
    """ssd_eval_ap_voc: flags u8 [N] sorted by (class, score desc, image, rank), seg_off i32 [C+1], n_pos i32 [C] (non-difficult
    boxes per class), year "07" (11-point) or "12" (area under the monotone envelope) -> AP f64 [C]; 0 where n_pos == 0."""
    L = _lib.lib()
    _dev(flags_sorted, torch.uint8); _dev(seg_off, torch.int32); _dev(n_pos, torch.int32)
    C = n_pos.numel()
    assert seg_off.numel() == C + 1
    if flags_sorted.numel() == 0:                      # the entry point wants a pointer even when there is nothing to read
        flags_sorted = torch.zeros((1,), dtype=torch.uint8, device=n_pos.device)
    ap = torch.empty((C,), dtype=torch.float64, device=n_pos.device)
    pts = _EVAL_VOC_RECALL_POINTS.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    _lib.check(L.ssd_eval_ap_voc(_ptr(flags_sorted), _ptr(seg_off), _ptr(n_pos), C, {"07": 7, "12": 12, 7: 7, 12: 12}.get(year, 0),
                                 pts, _ptr(ap), _stream()))
    return ap


# ------------------------------------------------------------------------------------------------
# convolution stack (NHWC bf16)
# ------------------------------------------------------------------------------------------------
_conv_ws = MatchWorkspace()


def same_pad(n, k, s):
    """TF 'SAME': out = ceil(n/s); pad_total = max((out-1)*s + k - n, 0); returns (out, pad_before)."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2


def valid_out(n, k, s):
    return (n - k) // s + 1


def _bf(t):
    assert t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


def image_prep(img, normalize=True, out=None):
    """f32 [B,H,W,3] in [0,1] -> bf16 [B,H,W,8] with (x-0.5)*2 (models/ssd_model.py:214), zero-padded channels."""
    L = _lib.lib()
    _dev(img, torch.float32)
    B, H, W, _ = img.shape
    if out is None:
        out = torch.empty((B, H, W, 8), dtype=torch.bfloat16, device=img.device)
    assert out.shape == (B, H, W, 8) and out.dtype == torch.bfloat16 and out.is_contiguous()
    _lib.check(L.ssd_image_prep(_ptr(img), _ptr(out), B, H, W, 1 if normalize else 0, _stream()))
    return out


def _splitk_ws(ws):
    buf = (ws or _conv_ws).get(1 << 25, torch.device("cuda", torch.cuda.current_device()))   # >= 32 MiB of scratch
    return buf


def conv2d_fwd(x, w, bias, stride, pad_t, pad_l, Ho, Wo, relu, out=None, ws=None):
    L = _lib.lib()
    _bf(x); _bf(w)
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    assert w.shape == (Cout, k, k, Cin)
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.bfloat16, device=x.device)
    wbuf = _splitk_ws(ws)
    _lib.check(L.ssd_conv2d_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), B, H, W, Cin, Cout, k, stride, pad_t, pad_l,
                                Ho, Wo, 1 if relu else 0, _ptr(wbuf), wbuf.numel(), _stream()))
    return out


def _pooled_shapes(bhw, *buffers):
    """The pooled outputs a caller hands in, (tensor, channels) each: contiguous [B, Hp, Wp, channels] of the window grid this
    call computes, or ValueError -- the kernels write that grid whatever the buffer's size."""
    for t, ch in buffers:
        if tuple(t.shape) != tuple(bhw) + (ch,) or not t.is_contiguous():
            raise ValueError("pooled output of shape %s, contiguous %s: this call writes %s" % (tuple(t.shape), t.is_contiguous(), tuple(bhw) + (ch,)))


def conv2d_fwd_pool(x, w, bias, stride, pad_t, pad_l, Ho, Wo, relu, same, out=None, pool_out=None, code=None, ws=None,
                    pool_only=False):
    """conv2d_fwd followed by maxpool2x2_fwd_argmax of its output, fused on chip where the kernel allows.
    pool_only=True: the full-resolution map is not stored (returned as None); raises ValueError (SSD_ERR_VALUE) for a layer
    shape that no pooling kernel serves (nothing is launched then)."""
    L = _lib.lib()
    _bf(x); _bf(w)
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    Hp, Wp = ((Ho + 1) // 2, (Wo + 1) // 2) if same else (Ho // 2, Wo // 2)
    if pool_only:
        out = None
    elif out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.bfloat16, device=x.device)
    if pool_out is None:
        pool_out = torch.empty((B, Hp, Wp, Cout), dtype=torch.bfloat16, device=x.device)
    if code is None:
        code = torch.empty((B, Hp, Wp, Cout // 8), dtype=torch.int32, device=x.device)
    _pooled_shapes((B, Hp, Wp), (pool_out, Cout), (code, Cout // 8))
    wbuf = _splitk_ws(ws)
    _lib.check(L.ssd_conv2d_fwd_pool(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(pool_out), _ptr(code), B, H, W, Cin, Cout, k,
                                     stride, pad_t, pad_l, Ho, Wo, 1 if relu else 0, Hp, Wp, _ptr(wbuf), wbuf.numel(), _stream()))
    return out, pool_out, code


def conv2d_head_fwd(x, w, bias, loc, conf, per_cell, classes, level_off, ws=None):
    L = _lib.lib()
    _bf(x); _bf(w); _bf(loc); _bf(conf)
    B, H, W, Cin = x.shape
    A = loc.shape[1]
    assert w.shape == (per_cell * (4 + classes), 3, 3, Cin)
    wbuf = _splitk_ws(ws)
    _lib.check(L.ssd_conv2d_head_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(loc), _ptr(conf), B, H, W, Cin, per_cell,
                                     classes, A, level_off, _ptr(wbuf), wbuf.numel(), _stream()))


def weight_transpose(w, cout_pad=None, out=None):
    L = _lib.lib()
    _bf(w)
    Cout, k, _, Cin = w.shape
    cout_pad = cout_pad or (Cout + 7) // 8 * 8
    if out is None:
        out = torch.empty((Cin, k, k, cout_pad), dtype=torch.bfloat16, device=w.device)
    _lib.check(L.ssd_weight_transpose(_ptr(w), _ptr(out), Cout, k, Cin, cout_pad, _stream()))
    return out


def conv2d_bwd_data(dy, w_t, relu_src, x_shape, stride, pad_t, pad_l, accumulate=False, out=None, ws=None):
    L = _lib.lib()
    _bf(dy); _bf(w_t)
    B, H, W, Cin = x_shape
    _, Ho, Wo, cpad = dy.shape
    k = w_t.shape[1]
    assert w_t.shape == (Cin, k, k, cpad)
    if out is None:
        assert not accumulate
        out = torch.empty(x_shape, dtype=torch.bfloat16, device=dy.device)
    wbuf = _splitk_ws(ws)
    _lib.check(L.ssd_conv2d_bwd_data(_ptr(dy), _ptr(w_t), _ptr(relu_src), _ptr(out), B, H, W, Cin, cpad, k, stride,
                                     pad_t, pad_l, Ho, Wo, 1 if accumulate else 0, _ptr(wbuf), wbuf.numel(), _stream()))
    return out


def chain_pack_weights(pairs):
    """ssd_chain_pack_weights: [(w, packed)] with w bf16 [N,k,k,C] (forward filters, or weight_transpose's copy for the data
    gradient) and packed a bf16 tensor of the same shape and element count that receives the fragment-packed copy conv_chain reads
    (None: allocated).  Returns the packed tensors.  One launch for up to 16 tensors."""
    L = _lib.lib()
    out = []
    for i0 in range(0, len(pairs), _lib.SSD_CHAIN_PACK_MAX):
        chunk = pairs[i0:i0 + _lib.SSD_CHAIN_PACK_MAX]
        arr = (_lib.ChainPack * len(chunk))()
        for d, (w, packed) in zip(arr, chunk):
            _bf(w)
            if packed is None:
                packed = torch.empty_like(w)
            _bf(packed)
            assert packed.numel() == w.numel()
            d.src, d.dst, d.N, d.K = _ptr(w), _ptr(packed), w.shape[0], w.numel() // w.shape[0]
            out.append(packed)
        _lib.check(L.ssd_chain_pack_weights(arr, len(chunk), _stream()))
    return out


def chain_prefetch(packed_list):
    """ssd_chain_prefetch: read the packed filter copies into every XCD's L2 (call on a second stream shortly before conv_chain)."""
    L = _lib.lib()
    arr = (_lib.ChainPack * len(packed_list))()
    for d, t in zip(arr, packed_list):
        _bf(t)
        d.src, d.dst, d.N, d.K = None, _ptr(t), t.shape[0], t.numel() // t.shape[0]
    _lib.check(L.ssd_chain_prefetch(arr, len(packed_list), _stream()))


def chain_layer_fwd(w, packed, bias, out, stride, pad_t, pad_l, relu=True, relu_bits=None):
    """One forward convolution of conv_chain: w bf16 [Cout,k,k,Cin] (shape only), packed = its chain_pack_weights copy (the
    operand), out bf16 [B,Ho,Wo,Cout]."""
    return dict(w=packed, bias=bias, out=out, ksize=w.shape[1], mul=stride, div=1, pad_t=pad_t, pad_l=pad_l, relu=relu,
                relu_bits=relu_bits, Kc=w.shape[3], N=w.shape[0])


def chain_layer_dgrad(w_t, packed, out, stride, pad_t, pad_l, accumulate=False, mask_bits=None, mask_src=None):
    """One data gradient of conv_chain: w_t bf16 [Cin,k,k,Cout_pad] (weight_transpose; shape only), packed = its
    chain_pack_weights copy, out bf16 [B,H,W,Cin] = the gradient w.r.t. the convolution's input (accumulated onto when
    `accumulate`), masked by the input activation's ReLU sign."""
    k = w_t.shape[1]
    return dict(w=packed, bias=None, out=out, ksize=k, mul=1, div=stride, pad_t=k - 1 - pad_t, pad_l=k - 1 - pad_l, relu=False,
                accumulate=accumulate, mask_bits=mask_bits, mask_src=mask_src, Kc=w_t.shape[3], N=w_t.shape[0])


def conv_chain(in0, layers):
    """ssd_conv_chain: layers (chain_layer_fwd / chain_layer_dgrad dicts) applied one after the other to in0 bf16 [B,H,W,C], one
    workgroup per image, in one launch; every layer's `out` is written.  NotImplementedError (SSD_ERR_UNSUPPORTED, nothing
    launched) where a layer does not fit the kernel."""
    L = _lib.lib()
    _bf(in0)
    B, Hi, Wi, Kc = in0.shape
    arr = (_lib.ChainLayer * len(layers))()
    for d, s in zip(arr, layers):
        out = s["out"]
        _bf(s["w"]); _bf(out)
        assert out.shape[0] == B and out.shape[3] == s["N"] and s["Kc"] == Kc, (tuple(out.shape), s["N"], s["Kc"], Kc)
        d.w, d.bias, d.out = _ptr(s["w"]), _ptr(s.get("bias")), _ptr(out)
        d.mask_bits, d.mask_src, d.relu_bits = _ptr(s.get("mask_bits")), _ptr(s.get("mask_src")), _ptr(s.get("relu_bits"))
        d.Hi, d.Wi, d.Kc, d.Ho, d.Wo, d.N = Hi, Wi, Kc, out.shape[1], out.shape[2], s["N"]
        d.ksize, d.mul, d.div, d.pad_t, d.pad_l = s["ksize"], s["mul"], s["div"], s["pad_t"], s["pad_l"]
        d.relu, d.accumulate = int(bool(s.get("relu"))), int(bool(s.get("accumulate")))
        Hi, Wi, Kc = out.shape[1], out.shape[2], s["N"]
    rc = L.ssd_conv_chain(_ptr(in0), arr, len(layers), B, _stream())
    _lib.check(rc, unsupported="ssd_conv_chain does not serve these layers")


CHAIN_LDS_MAX = 160 * 1024                   # csrc/chain.hip: CH_LDS_MAX


def chain_lds_bytes(layers):
    """LDS bytes of one ssd_conv_chain launch, the host code's own arithmetic: layers = [(input pixels, input channels, output
    pixels, output channels)] in launch order.  An image of P pixels and C channels takes P (2 C + 16) bytes; image l (0: the
    chain's input, l: the output of layer l - 1; the last output goes to memory only) lives in region l & 1; both regions round
    up to 16 bytes, and one zero row of the widest input follows them.  The launch is refused above CHAIN_LDS_MAX."""
    region = [0, 0]
    for l, (pin, cin, pout, cout) in enumerate(layers):
        region[l & 1] = max(region[l & 1], pin * (2 * cin + 16))
        if l + 1 < len(layers):
            region[(l + 1) & 1] = max(region[(l + 1) & 1], pout * (2 * cout + 16))
    return sum((r + 15) // 16 * 16 for r in region) + max(2 * cin for _, cin, _, _ in layers)


def conv2d_fwd_relubits(x, w, bias, stride, pad_t, pad_l, Ho, Wo, bits, out=None, ws=None):
    """conv2d_fwd with ReLU that also writes the sign bits of its output (uint8 [B,Ho,Wo,Cout/8]).  NotImplementedError
    (SSD_ERR_UNSUPPORTED, nothing launched) where the layer's kernel has no staged store."""
    L = _lib.lib()
    _bf(x); _bf(w)
    B, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    assert bits.dtype == torch.uint8 and bits.shape == (B, Ho, Wo, Cout // 8) and bits.is_contiguous()
    if out is None:
        out = torch.empty((B, Ho, Wo, Cout), dtype=torch.bfloat16, device=x.device)
    wbuf = _splitk_ws(ws)
    rc = L.ssd_conv2d_fwd_relubits(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(bits), B, H, W, Cin, Cout, k, stride, pad_t, pad_l,
                                   Ho, Wo, _ptr(wbuf), wbuf.numel(), _stream())
    _lib.check(rc, unsupported="this layer's kernel does not write sign bits")
    return out


def conv2d_bwd_data_bits(dy, w_t, bits, x_shape, stride, pad_t, pad_l, accumulate=False, out=None, ws=None):
    """conv2d_bwd_data with the ReLU mask given as the sign bits of conv2d_fwd_relubits (same result, 16x fewer mask bytes)."""
    L = _lib.lib()
    _bf(dy); _bf(w_t)
    B, H, W, Cin = x_shape
    _, Ho, Wo, cpad = dy.shape
    k = w_t.shape[1]
    assert w_t.shape == (Cin, k, k, cpad) and bits.dtype == torch.uint8 and bits.shape == (B, H, W, Cin // 8)
    if out is None:
        assert not accumulate
        out = torch.empty(x_shape, dtype=torch.bfloat16, device=dy.device)
    wbuf = _splitk_ws(ws)
    rc = L.ssd_conv2d_bwd_data_bits(_ptr(dy), _ptr(w_t), _ptr(bits), _ptr(out), B, H, W, Cin, cpad, k, stride, pad_t, pad_l, Ho, Wo,
                                    1 if accumulate else 0, _ptr(wbuf), wbuf.numel(), _stream())
    _lib.check(rc, unsupported="this layer's kernel does not read sign bits")
    return out


def conv2d_bwd_data_wgrad_first(dy, w_t, bits, image, dw=None, dbias=None, ws=None):
    """Data gradient of the second trunk layer (64 -> 64) fused with the weight gradient of the first (image -> 64): returns
    (dw0 [64,3,3,8] f32, dbias0 [64] f32); the gradient w.r.t. the first layer's output is consumed inside the kernel and never
    stored.  Same result as conv2d_bwd_data_bits + conv2d_bwd_weight up to fp32 summation order."""
    L = _lib.lib()
    _bf(dy); _bf(w_t); _bf(image)
    B, H, W, c = dy.shape
    assert c == 64 and w_t.shape == (64, 3, 3, 64) and image.shape == (B, H, W, 8)
    assert bits.dtype == torch.uint8 and bits.shape == (B, H, W, 8)
    if dw is None:
        dw = torch.empty((64, 3, 3, 8), dtype=torch.float32, device=dy.device)
    if dbias is None:
        dbias = torch.empty((64,), dtype=torch.float32, device=dy.device)
    assert dw.dtype == torch.float32 and dw.numel() == 64 * 72 and dw.is_contiguous() and dbias.dtype == torch.float32
    wbuf = (ws or _conv_ws).get(L.ssd_conv2d_bwd_data_wgrad_first_workspace_bytes(B, H, W), dy.device)
    rc = L.ssd_conv2d_bwd_data_wgrad_first(_ptr(dy), _ptr(w_t), _ptr(bits), _ptr(image), _ptr(dw), _ptr(dbias), B, H, W, _ptr(wbuf),
                                           wbuf.numel(), _stream())
    _lib.check(rc, unsupported="maps smaller than 16x16 take the two separate calls")
    return dw, dbias


def conv2d_bwd_data_unpool(dy, w_t, relu_src, pool_code, full_shape, out=None, ws=None, pooled_out=None):
    """conv2d_bwd_data (3x3 / stride 1 / pad 1) w.r.t. a pooled map followed by maxpool2x2_bwd_argmax, in one launch: returns the
    gradient of the map BEFORE the pooling ([B,Hf,Wf,Cin]).  Raises NotImplementedError (SSD_ERR_UNSUPPORTED, nothing launched)
    when the layer is not served by an LDS-patch kernel: use the two calls then."""
    L = _lib.lib()
    _bf(dy); _bf(w_t)
    B, Hf, Wf, Cin = full_shape
    _, H, W, cpad = dy.shape
    assert w_t.shape == (Cin, 3, 3, cpad) and pool_code.shape == (B, H, W, Cin // 8) and pool_code.dtype == torch.int32
    if out is None:
        out = torch.empty(full_shape, dtype=torch.bfloat16, device=dy.device)
    wbuf = _splitk_ws(ws)
    if pooled_out is not None:                     # also keep the gradient of the pooled map (conv2d_bwd_weight_unpooled reads it)
        _bf(pooled_out)
        assert pooled_out.shape == (B, H, W, Cin)
    rc = L.ssd_conv2d_bwd_data_unpool(_ptr(dy), _ptr(w_t), _ptr(relu_src), _ptr(pool_code), _ptr(pooled_out), _ptr(out), B, H, W, Cin,
                                      cpad, Hf, Wf, _ptr(wbuf), wbuf.numel(), _stream())
    _lib.check(rc, unsupported="no LDS-patch kernel for this layer")
    return out


def conv2d_bwd_weight(x, dy, Cout, k, stride, pad_t, pad_l, dw=None, dbias=None, want_bias=True, ws=None):
    L = _lib.lib()
    _bf(x); _bf(dy)
    B, H, W, Cin = x.shape
    _, Ho, Wo, ldy = dy.shape
    if dw is None:
        dw = torch.empty((Cout, k, k, Cin), dtype=torch.float32, device=x.device)
    if dbias is None and want_bias:
        dbias = torch.empty((Cout,), dtype=torch.float32, device=x.device)
    nbytes = L.ssd_conv2d_bwd_weight_workspace_bytes(B, Ho, Wo, Cin, Cout, ldy, k)
    wbuf = (ws or _conv_ws).get(nbytes, x.device)
    _lib.check(L.ssd_conv2d_bwd_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(dbias), B, H, W, Cin, Cout, ldy, k, stride,
                                       pad_t, pad_l, Ho, Wo, _ptr(wbuf), wbuf.numel(), _stream()))
    return dw, dbias


def conv2d_bwd_weight_batched(layers, ws=None):
    """ssd_conv2d_bwd_weight_batched: layers = [(x, dy, Cout, k, stride, pad_t, pad_l, dw, dbias)] (arguments of conv2d_bwd_weight,
    dw / dbias given) in two launches; bit-identical to the separate calls.  NotImplementedError (SSD_ERR_UNSUPPORTED, nothing
    launched) when a layer is not one the generic small-layer kernel serves."""
    L = _lib.lib()
    arr = (_lib.WgradItem * len(layers))()
    for d, (x, dy, Cout, k, stride, pad_t, pad_l, dw, dbias) in zip(arr, layers):
        _bf(x); _bf(dy)
        B, H, W, Cin = x.shape
        _, Ho, Wo, ldy = dy.shape
        assert dw.dtype == torch.float32 and dw.shape == (Cout, k, k, Cin) and dw.is_contiguous()
        d.x, d.dy, d.dw, d.dbias = _ptr(x), _ptr(dy), _ptr(dw), _ptr(dbias)
        d.B, d.H, d.W, d.Cin, d.Cout, d.ldy, d.ksize, d.stride, d.pad_t, d.pad_l, d.Ho, d.Wo = B, H, W, Cin, Cout, ldy, k, stride, pad_t, pad_l, Ho, Wo
    nbytes = L.ssd_conv2d_bwd_weight_batched_workspace_bytes(arr, len(layers))
    wbuf = (ws or _conv_ws).get(nbytes, layers[0][0].device)
    rc = L.ssd_conv2d_bwd_weight_batched(arr, len(layers), _ptr(wbuf), wbuf.numel(), _stream())
    _lib.check(rc, unsupported="ssd_conv2d_bwd_weight_batched does not serve these layers")


def conv2d_bwd_weight_unpooled(x, dpool, pool_code, dw=None, dbias=None, want_bias=True, ws=None):
    """Weight gradient of a 3x3 / stride 1 / pad 1 convolution whose output was 2x2 max-pooled, from the gradient of the pooled
    map and the winner codes (== conv2d_bwd_weight(x, maxpool2x2_bwd_argmax(pool_code, dpool, ...)) without the un-pooled zeros:
    structured-sparse MFMA).  Raises NotImplementedError (SSD_ERR_UNSUPPORTED, nothing launched) for shapes it does not serve."""
    L = _lib.lib()
    _bf(x); _bf(dpool)
    B, H, W, Cin = x.shape
    _, Hp, Wp, Cout = dpool.shape
    assert pool_code.shape == (B, Hp, Wp, Cout // 8) and pool_code.dtype == torch.int32
    if dw is None:
        dw = torch.empty((Cout, 3, 3, Cin), dtype=torch.float32, device=x.device)
    if dbias is None and want_bias:
        dbias = torch.empty((Cout,), dtype=torch.float32, device=x.device)
    nbytes = L.ssd_conv2d_bwd_weight_unpooled_workspace_bytes(B, H, W, Cin, Cout, Hp, Wp)
    if nbytes == 0:
        raise NotImplementedError("no structured-sparse weight-gradient kernel for this layer")
    wbuf = (ws or _conv_ws).get(nbytes, x.device)
    rc = L.ssd_conv2d_bwd_weight_unpooled(_ptr(x), _ptr(dpool), _ptr(pool_code), _ptr(dw), _ptr(dbias), B, H, W, Cin, Cout, Hp, Wp,
                                          _ptr(wbuf), wbuf.numel(), _stream())
    _lib.check(rc, unsupported="no structured-sparse weight-gradient kernel for this layer")
    return dw, dbias


def image_resize_prep(src, src_off, src_hw, S=300, normalize=True, out=None):
    """Ragged batch of uint8 RGB images (src: flat u8 buffer, src_off i64 [B] byte offsets, src_hw i32 [B,2]) ->
    network input bf16 [B,S,S,8]: /255, cv2.resize INTER_LINEAR, (x-0.5)*2  (reference lines in include/ssd_hip.h)."""
    L = _lib.lib()
    _dev(src, torch.uint8); _dev(src_off, torch.int64); _dev(src_hw, torch.int32)
    B = src_hw.shape[0]
    if out is None:
        out = torch.empty((B, S, S, 8), dtype=torch.bfloat16, device=src.device)
    _lib.check(L.ssd_image_resize_prep(_ptr(src), _ptr(src_off), _ptr(src_hw), _ptr(out), B, S, 1 if normalize else 0, _stream()))
    return out


def box_prep(box_tlwh, gt_off, src_hw):
    """COCO [x,y,w,h] pixel boxes of a batch (concatenated) -> relative centre form, per image size."""
    L = _lib.lib()
    _dev(box_tlwh, torch.float32); _dev(gt_off, torch.int32); _dev(src_hw, torch.int32)
    total = box_tlwh.shape[0]
    out = torch.empty_like(box_tlwh)
    _lib.check(L.ssd_box_prep(_ptr(box_tlwh), _ptr(gt_off), _ptr(src_hw), _ptr(out), src_hw.shape[0], total, _stream()))
    return out


AUG_PHOTO, AUG_EXPAND, AUG_CROP, AUG_FLIP, AUG_ALL = (_lib.CONSTANTS["SSD_AUG_" + n] for n in ("PHOTO", "EXPAND", "CROP", "FLIP", "ALL"))


def _record_dtype(struct):
    """A header struct of scalars as a numpy record dtype at the struct's own offsets; `reserved[2]` -> reserved0, reserved1."""
    names, formats, offsets = [], [], []
    for name, ctype in struct._fields_:
        array = hasattr(ctype, "_length_")
        elem = ctype._type_ if array else ctype
        for i in range(ctype._length_ if array else 1):
            names.append(name + str(i) if array else name)
            formats.append(np.dtype(elem))
            offsets.append(getattr(struct, name).offset + i * ctypes.sizeof(elem))
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": ctypes.sizeof(struct)})


AUG_PARAM_DTYPE = _record_dtype(_lib.AugmentParams)               # one ssd_augment_params record
AUG_PARAM_FIELDS = AUG_PARAM_DTYPE.names


class AugmentSpec:
    """Training-batch augmentation (include/ssd_hip.h has the recipe): Philox seed, stage mask (AUG_* bits, default all four)
    and the global stream index of the batch's first sample.  get_train_set fills in first_index per batch."""

    def __init__(self, seed=0, stages=AUG_ALL, first_index=0):
        if int(stages) & ~AUG_ALL:
            raise ValueError("unknown augmentation stage bits %#x" % int(stages))
        self.seed = int(seed)
        self.stages = int(stages)
        self.first_index = int(first_index)

    def at(self, first_index):
        return AugmentSpec(self.seed, self.stages, first_index)

    def __repr__(self):
        return "AugmentSpec(seed=%d, stages=%d, first_index=%d)" % (self.seed, self.stages, self.first_index)


def augment_plan(box, cls, gt_off, src_hw, total_gt, stages, seed, first_index):
    """ssd_augment_plan: per-image augmentation draws, crop search and box transform on the device, no host sync.
    box f32 [total_gt,4] relative (cx,cy,w,h), cls f32 [total_gt], gt_off i32 [B+1], src_hw i32 [B,2] (h, w).
    Returns (params u8 [B, 80] ssd_augment_params records, box_out f32 [total_gt,4], cls_out f32 [total_gt], off_out i32 [B+1]):
    the kept boxes compacted per image, zero rows after off_out[B]."""
    L = _lib.lib()
    _dev(gt_off, torch.int32); _dev(src_hw, torch.int32)
    B = src_hw.shape[0]
    dev = src_hw.device
    if total_gt > 0:
        _dev(box, torch.float32); _dev(cls, torch.float32)
    params = torch.empty((B, AUG_PARAM_DTYPE.itemsize), dtype=torch.uint8, device=dev)
    box_out = torch.empty((total_gt, 4), dtype=torch.float32, device=dev)
    cls_out = torch.empty((total_gt,), dtype=torch.float32, device=dev)
    off_out = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    _lib.check(L.ssd_augment_plan(_ptr(box if total_gt > 0 else None), _ptr(cls if total_gt > 0 else None), _ptr(gt_off),
                                  _ptr(src_hw), B, int(total_gt), int(stages), int(seed) & (2 ** 64 - 1), int(first_index),
                                  _ptr(params), _ptr(box_out if total_gt > 0 else None),
                                  _ptr(cls_out if total_gt > 0 else None), _ptr(off_out), _stream()))
    return params, box_out, cls_out, off_out


def augment_params_numpy(params):
    """Device params records (augment_plan) -> numpy structured array of AUG_PARAM_DTYPE."""
    return params.cpu().numpy().view(AUG_PARAM_DTYPE).reshape(-1)


def augment_image(src, src_kind, src_off, src_hw, params, S=300, normalize=True, out=None):
    """ssd_augment_image: the planned augmentation of every image, resized to S x S -> bf16 [B,S,S,8].
    src_kind 0: flat uint8 buffer of the ragged batch with src_off i64 [B] byte offsets (as image_resize_prep);
    src_kind 1: f32 [B,H,W,3] in [0,1] (src_off None)."""
    L = _lib.lib()
    _dev(src_hw, torch.int32); _dev(params, torch.uint8)
    if src_kind == 0:
        _dev(src, torch.uint8); _dev(src_off, torch.int64)
    elif src_kind == 1:
        _dev(src, torch.float32)
    B = src_hw.shape[0]
    assert params.shape == (B, AUG_PARAM_DTYPE.itemsize)
    if out is None:
        out = torch.empty((B, S, S, 8), dtype=torch.bfloat16, device=src_hw.device)
    assert out.shape == (B, S, S, 8) and out.dtype == torch.bfloat16 and out.is_contiguous()
    _lib.check(L.ssd_augment_image(_ptr(src), int(src_kind), _ptr(src_off), _ptr(src_hw), _ptr(params), _ptr(out), B, int(S),
                                   1 if normalize else 0, _stream()))
    return out


# ---- JPEG: Huffman on host threads, everything arithmetic on the device (include/ssd_hip.h) ------------------------------------
JPEG_REC_WORDS = _lib.CONSTANTS["SSD_JPEG_REC_WORDS"]
JPEG_KINDS = ("grey", "4:4:4", "4:2:2", "4:2:0")                   # SSD_JPEG_GREY .. SSD_JPEG_420
JpegStats = collections.namedtuple("JpegStats", "images device fallback")
_JPEG_UNSUPPORTED = ("not a stream the device decoder serves (baseline 8-bit Huffman, one scan, grey or YCbCr 4:4:4 / 4:2:2 / "
                     "4:2:0 only; progressive, arithmetic, 12-bit, lossless, CMYK, RGB-marked and multi-scan streams are refused)")


class EncodedImage:
    """An image still encoded as JPEG: what COCODataLoader(decode="device") yields in place of the decoded array.  `shape` is
    (H, W, 3) from the frame header, so code that only asks for a sample's size works on it unchanged."""
    __slots__ = ("data", "height", "width")

    def __init__(self, data, height, width):
        self.data, self.height, self.width = bytes(data), int(height), int(width)

    @property
    def shape(self):
        return (self.height, self.width, 3)

    def __repr__(self):
        return "EncodedImage(%d bytes, %dx%d)" % (len(self.data), self.width, self.height)


def _jpeg_record(rec):
    g = _lib.CONSTANTS
    nc = int(rec[g["SSD_JPEG_NCOMP"]])
    return dict(width=int(rec[g["SSD_JPEG_WIDTH"]]), height=int(rec[g["SSD_JPEG_HEIGHT"]]), ncomp=nc,
                kind=int(rec[g["SSD_JPEG_KIND"]]), blocks_w=rec[g["SSD_JPEG_BLOCKS_W"]:][:nc].tolist(),
                blocks_h=rec[g["SSD_JPEG_BLOCKS_H"]:][:nc].tolist(), ncoef=int(rec[g["SSD_JPEG_NCOEF"]]),
                restart=int(rec[g["SSD_JPEG_RESTART"]]), coef_off=rec[g["SSD_JPEG_COEF_OFF"]:][:nc].tolist(),
                qt=rec[g["SSD_JPEG_QT"]:][:64 * nc].reshape(nc, 64).copy(), rec=rec)


def jpeg_info(data):
    """ssd_jpeg_info (host only): the frame of a JPEG byte string as a dict -- width, height, ncomp, kind (index into
    JPEG_KINDS), blocks_w / blocks_h per component (padded to whole MCUs), ncoef, restart, coef_off, qt int32 [ncomp, 64] in
    natural order, rec (the int32 record).  NotImplementedError for a stream the decoder does not serve, ValueError for a
    corrupt one."""
    data = bytes(data)
    rec = np.zeros(JPEG_REC_WORDS, np.int32)
    _lib.check(_lib.lib().ssd_jpeg_info(data, len(data), rec.ctypes.data), unsupported=_JPEG_UNSUPPORTED)
    return _jpeg_record(rec)


def jpeg_entropy_decode(data, capacity=None):
    """ssd_jpeg_entropy_decode (host only, no HIP call): (coef int16 [ncoef], header dict as jpeg_info).  capacity: the size
    of the buffer offered, in coefficients (default: what jpeg_info asks for); too small raises RuntimeError (SSD_ERR_WORKSPACE)."""
    data = bytes(data)
    need = jpeg_info(data)["ncoef"] if capacity is None else int(capacity)
    coef = np.empty(max(need, 1), np.int16)
    rec = np.zeros(JPEG_REC_WORDS, np.int32)
    _lib.check(_lib.lib().ssd_jpeg_entropy_decode(data, len(data), coef.ctypes.data, need, rec.ctypes.data),
               unsupported=_JPEG_UNSUPPORTED)
    h = _jpeg_record(rec)
    return coef[:h["ncoef"]], h


def jpeg_reconstruct(coef, desc, dst, dst_off, scratch=None):
    """ssd_jpeg_reconstruct: coef int16 [total] and desc int32 [B, JPEG_REC_WORDS] (absolute coefficient offsets) on the device
    -> H*W*3 bytes of RGB per image at dst_off[b] (int64 [B]) of the uint8 buffer dst; nothing else is written.  scratch: uint8
    [>= total] or None.  Returns dst."""
    L = _lib.lib()
    _dev(coef, torch.int16); _dev(desc, torch.int32); _dev(dst, torch.uint8); _dev(dst_off, torch.int64)
    B, total = desc.shape[0], coef.numel()
    assert desc.shape == (B, JPEG_REC_WORDS) and dst_off.shape == (B,)
    need = L.ssd_jpeg_reconstruct_workspace_bytes(total)
    if scratch is None:
        scratch = torch.empty((max(need, 1),), dtype=torch.uint8, device=coef.device)
    _dev(scratch, torch.uint8)
    _lib.check(L.ssd_jpeg_reconstruct(_ptr(coef), _ptr(desc), B, _ptr(dst), _ptr(dst_off), dst.numel(), _ptr(scratch),
                                      scratch.numel(), total, _stream()))
    return dst


_JPEG_STAGE = {}                   # device -> [pinned uint8 buffer, event behind the last copy out of it]
_JPEG_POOLS = {}                   # workers -> ThreadPoolExecutor


def _jpeg_pool(workers):
    workers = int(workers)
    if workers < 1:
        raise ValueError("workers must be >= 1, not %r" % (workers,))
    if workers not in _JPEG_POOLS:
        import concurrent.futures
        _JPEG_POOLS[workers] = concurrent.futures.ThreadPoolExecutor(workers, thread_name_prefix="ssd-jpeg")
    return _JPEG_POOLS[workers]


def _jpeg_stage(device, nbytes):
    """The reused pinned staging buffer of a device, at least nbytes long and no longer read by an earlier copy."""
    slot = _JPEG_STAGE.get(device)
    if slot is not None and slot[1] is not None:
        slot[1].synchronize()
    if slot is None or slot[0].numel() < nbytes:
        slot = [torch.empty((max(int(nbytes) * 5 // 4, 1 << 20),), dtype=torch.uint8).pin_memory(), None]
        _JPEG_STAGE[device] = slot
    return slot


def _pil_decode(data):
    import io
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), np.uint8))


def image_arena(items, device, workers=8, fallback="pil"):
    """The ragged uint8 arena of ssd_image_resize_prep / ssd_augment_image (source kind 0) from a batch of images that are
    JPEG byte strings (or EncodedImage), decoded uint8 arrays [H,W,3], or a mix.  Encoded images are entropy-decoded on a pool
    of `workers` host threads (the C function releases the GIL) straight into one reused pinned buffer, copied with one
    non-blocking transfer and reconstructed by one ssd_jpeg_reconstruct call on the current stream.  Returns
    (arena u8 [sum H*W*3], off i64 [B], hw i32 [B,2], JpegStats).  See decode_jpeg_batch for refusals."""
    L = _lib.lib()
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    B = len(items)
    if B == 0:
        raise ValueError("an empty batch")
    if fallback not in ("pil", None):
        raise ValueError("fallback must be 'pil' or None, not %r" % (fallback,))
    g = _lib.CONSTANTS
    host = {}                                              # index -> decoded array that is copied into its slot
    enc = []                                               # (index, bytes, record)
    hw = np.zeros((B, 2), np.int32)
    for i, item in enumerate(items):
        if isinstance(item, np.ndarray):
            if item.dtype != np.uint8 or item.ndim != 3 or item.shape[2] != 3:
                raise ValueError("sample %d: a decoded image must be uint8 [H,W,3], not %s %s" % (i, item.dtype, item.shape))
            host[i] = np.ascontiguousarray(item)
            hw[i] = item.shape[:2]
            continue
        data = item.data if isinstance(item, EncodedImage) else bytes(item)
        rec = np.zeros(JPEG_REC_WORDS, np.int32)
        rc = L.ssd_jpeg_info(data, len(data), rec.ctypes.data)
        if rc == _lib.SSD_ERR_UNSUPPORTED:
            if fallback is None:
                raise NotImplementedError("sample %d: %s" % (i, _JPEG_UNSUPPORTED))
            try:
                host[i] = _pil_decode(data)
            except ImportError:
                raise NotImplementedError("sample %d: %s, and Pillow is not installed to decode it on the host"
                                          % (i, _JPEG_UNSUPPORTED)) from None
            hw[i] = host[i].shape[:2]
            continue
        if rc != _lib.SSD_OK:
            raise ValueError("sample %d: corrupt JPEG stream (%s)" % (i, L.ssd_status_string(rc).decode()))
        enc.append((i, data, rec))
        hw[i] = (rec[g["SSD_JPEG_HEIGHT"]], rec[g["SSD_JPEG_WIDTH"]])
    n_fallback = sum(1 for i in host if not isinstance(items[i], np.ndarray))
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1].astype(np.int64) * 3
    off = np.zeros(B, np.int64)
    off[1:] = np.cumsum(sizes[:-1])
    total_bytes = int(sizes.sum())
    E = len(enc)
    base = np.zeros(E + 1, np.int64)
    base[1:] = np.cumsum([int(r[g["SSD_JPEG_NCOEF"]]) for _, _, r in enc])
    total_coef = int(base[E])
    if total_coef > 0x7fffffff:
        raise ValueError("the batch holds %d coefficients: more than one reconstruct call addresses" % total_coef)
    # staging layout (bytes): coef int16 [total_coef] | desc int32 [E, REC] | dst_off int64 [E] | off int64 [B] | hw int32 [B,2]
    o_desc = (2 * total_coef + 15) // 16 * 16
    o_dst = o_desc + 4 * JPEG_REC_WORDS * E
    o_off = o_dst + 8 * E
    o_hw = o_off + 8 * B
    nbytes = o_hw + 8 * B
    slot = _jpeg_stage(device, nbytes)
    stage = slot[0]
    view = stage.numpy()
    desc_h = view[o_desc:o_dst].view(np.int32).reshape(E, JPEG_REC_WORDS)
    view[o_dst:o_off].view(np.int64)[:] = off[[i for i, _, _ in enc]] if E else 0
    view[o_off:o_hw].view(np.int64)[:] = off
    view[o_hw:nbytes].view(np.int32)[:] = hw.reshape(-1)
    p0 = stage.data_ptr()

    def work(k):
        i, data, _ = enc[k]
        return L.ssd_jpeg_entropy_decode(data, len(data), p0 + 2 * int(base[k]), int(base[k + 1] - base[k]),
                                         p0 + o_desc + 4 * JPEG_REC_WORDS * k)

    if E:
        codes = list(_jpeg_pool(workers).map(work, range(E))) if workers > 1 and E > 1 else [work(k) for k in range(E)]
        for k, rc in enumerate(codes):
            if rc != _lib.SSD_OK:
                raise ValueError("sample %d: corrupt JPEG stream (%s)" % (enc[k][0], L.ssd_status_string(rc).decode()))
        c0 = g["SSD_JPEG_COEF_OFF"]
        desc_h[:, c0:c0 + 3] += base[:E, None].astype(np.int32)
    dev_buf = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    dev_buf.copy_(stage[:nbytes], non_blocking=True)
    slot[1] = torch.cuda.Event()
    slot[1].record()
    arena = torch.empty((total_bytes,), dtype=torch.uint8, device=device)
    if E:
        jpeg_reconstruct(dev_buf[:2 * total_coef].view(torch.int16), dev_buf[o_desc:o_dst].view(torch.int32).view(E, JPEG_REC_WORDS),
                         arena, dev_buf[o_dst:o_off].view(torch.int64))
    for i, image in host.items():
        flat = image.reshape(-1) if image.flags.writeable else image.reshape(-1).copy()     # (from_numpy wants a writable array)
        arena[int(off[i]):int(off[i] + sizes[i])].copy_(torch.from_numpy(flat), non_blocking=False)
    return (arena, dev_buf[o_off:o_hw].view(torch.int64), dev_buf[o_hw:nbytes].view(torch.int32).view(B, 2),
            JpegStats(images=B, device=E, fallback=n_fallback))


def decode_jpeg_batch(encoded, device, workers=8, fallback="pil"):
    """A batch of JPEG byte strings -> (arena u8, off i64 [B], hw i32 [B,2] (h, w), JpegStats(images, device, fallback)): the
    decoded RGB images back to back on `device`, as image_resize_prep and augment_image (source kind 0) take them.  Huffman
    decoding runs on `workers` host threads; dequantisation, IDCT, chroma upsampling and colour conversion on the device.  The
    pixels equal libjpeg's default decode (what Pillow returns) bit for bit.
    A stream the library refuses as unsupported is decoded by Pillow on the host and copied into its slot (stats.fallback counts
    them); with fallback=None, or without Pillow, it raises NotImplementedError.  A corrupt stream raises ValueError.  Both name
    the sample."""
    for i, e in enumerate(encoded):
        if not isinstance(e, (bytes, bytearray, memoryview, EncodedImage)):
            raise ValueError("sample %d: expected JPEG bytes, not %s" % (i, type(e).__name__))
    return image_arena(list(encoded), device, workers, fallback)


def maxpool2x2_fwd(x, same=False, out=None):
    L = _lib.lib()
    _bf(x)
    B, H, W, C = x.shape
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if same else (H // 2, W // 2)
    y = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device) if out is None else out
    assert y.shape == (B, Ho, Wo, C) and y.dtype == torch.bfloat16 and y.is_contiguous()
    _lib.check(L.ssd_maxpool2x2_fwd(_ptr(x), _ptr(y), B, H, W, C, Ho, Wo, _stream()))
    return y


def maxpool2x2_fwd_argmax(x, same=False, out=None, code=None):
    """Pooling that also records the winner of every window (4-bit codes, u32 per 8 channels) for maxpool2x2_bwd_argmax."""
    L = _lib.lib()
    _bf(x)
    B, H, W, C = x.shape
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if same else (H // 2, W // 2)
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    if code is None:
        code = torch.empty((B, Ho, Wo, C // 8), dtype=torch.int32, device=x.device)
    _pooled_shapes((B, Ho, Wo), (out, C), (code, C // 8))
    _lib.check(L.ssd_maxpool2x2_fwd_argmax(_ptr(x), _ptr(out), _ptr(code), B, H, W, C, Ho, Wo, _stream()))
    return out, code


def maxpool2x2_bwd_argmax(code, dy, x_shape, out=None, accumulate=False):
    """Un-pooling from the recorded winners.  accumulate=True adds onto `out` (required: it holds the gradient that reached the
    same activation on another path) with one fp32 addition and one rounding; elements that no window routes to keep their bits."""
    L = _lib.lib()
    _bf(dy)
    B, H, W, C = x_shape
    _, Ho, Wo, _ = dy.shape
    if accumulate:
        if out is None:
            raise ValueError("maxpool2x2_bwd_argmax: accumulate=True adds onto `out`, which must be given")
        _bf(out)
        assert tuple(out.shape) == tuple(x_shape) and out.is_contiguous()
        _lib.check(L.ssd_maxpool2x2_bwd_argmax_accumulate(_ptr(code), _ptr(dy), _ptr(out), B, H, W, C, Ho, Wo, _stream()))
        return out
    if out is None:
        out = torch.empty(tuple(x_shape), dtype=torch.bfloat16, device=dy.device)
    _lib.check(L.ssd_maxpool2x2_bwd_argmax(_ptr(code), _ptr(dy), _ptr(out), B, H, W, C, Ho, Wo, _stream()))
    return out


def maxpool2x2_bwd(x, y, dy, out=None):
    L = _lib.lib()
    _bf(x); _bf(y); _bf(dy)
    B, H, W, C = x.shape
    _, Ho, Wo, _ = y.shape
    if out is None:
        out = torch.empty_like(x)
    _lib.check(L.ssd_maxpool2x2_bwd(_ptr(x), _ptr(y), _ptr(dy), _ptr(out), B, H, W, C, Ho, Wo, _stream()))
    return out


def _mx_pair(shape, device):
    """Uninitialised (q, scale) uint8 tensors of the MX-fp8 form of a [..., C] map: one e4m3 byte per element, one E8M0 scale
    byte per 32 channels (at least one: a C the kernels do not serve still gets its refusal from them).  mx.pair is the
    checked form; the only other place that spells this allocation."""
    shape = tuple(shape)
    return (torch.empty(shape, dtype=torch.uint8, device=device),
            torch.empty(shape[:-1] + (max(shape[-1] // 32, 1),), dtype=torch.uint8, device=device))


def _mx_default(shape, device, q, scale):
    """(q, scale) as handed in; whichever is None from a fresh _mx_pair."""
    if q is None or scale is None:
        fresh = _mx_pair(shape, device)
        q, scale = fresh[0] if q is None else q, fresh[1] if scale is None else scale
    return q, scale


def _mx_operands(xq, xs, wq, ws, bhwk, wshape):
    """Check the operand quadruple of an fp8 convolution: (xq, xs) the MX-fp8 form of a [B,H,W,K] map, (wq, ws) that of
    filters [N,k,k,K]; K is the GEMM's reduction, one scale byte per 32 of it."""
    bhwk, wshape = tuple(bhwk), tuple(wshape)
    K = bhwk[3]
    assert xq.shape == bhwk and wq.shape == wshape and xs.shape == bhwk[:3] + (K // 32,) and ws.shape == wshape[:3] + (K // 32,)
    for t in (xq, xs, wq, ws):
        _dev(t, torch.uint8)


def _mx_outputs(shape, device, want_bf16, want_fp8, out, out_q, out_scale):
    """The outputs of an fp8 convolution with a bf16 epilogue, an fp8 one or both: (out, out_q, out_scale, result) -- an
    output that is not wanted comes back as None (the C call's null), a wanted one that was not handed in is allocated;
    result is what the wrapper returns: the bf16 map, (q, scale), or (bf16, q, scale) when both are wanted."""
    assert want_bf16 or want_fp8
    if not want_bf16:
        out = None
    elif out is None:
        out = torch.empty(tuple(shape), dtype=torch.bfloat16, device=device)
    out_q, out_scale = _mx_default(shape, device, out_q, out_scale) if want_fp8 else (None, None)
    return out, out_q, out_scale, (out if not want_fp8 else (out, out_q, out_scale) if want_bf16 else (out_q, out_scale))


def quantize_mx_fp8(x, q=None, scale=None):
    """bf16 tensor (last dimension a multiple of 32) -> (q uint8 same shape: OCP e4m3 bytes, scale uint8 [..., C/32]: E8M0).
    A block that holds a NaN or an infinity comes out as 32 NaN bytes (0x7F) under the scale byte 127."""
    L = _lib.lib()
    _bf(x)
    assert x.shape[-1] % 32 == 0
    q, scale = _mx_default(x.shape, x.device, q, scale)
    assert q.numel() == x.numel() and scale.numel() == x.numel() // 32
    _lib.check(L.ssd_quantize_mx_fp8(_ptr(x), _ptr(q), _ptr(scale), x.numel(), _stream()))
    return q, scale


def dequantize_mx_fp8(q, scale):
    """The float32 values an MX-fp8 pair stands for (tests / reports; torch's float8_e4m3fn is the same OCP encoding)."""
    v = q.view(torch.float8_e4m3fn).float()
    s = torch.exp2(scale.float() - 127.0)
    return (v.view(*scale.shape, 32) * s.unsqueeze(-1)).view(q.shape)


def conv3x3_fwd_mxfp8(xq, xs, wq, ws, bias, relu=True, out=None):
    """3x3 / stride 1 / SAME forward on block-scaled fp8 operands (quantize_mx_fp8 of x [B,H,W,Cin] and w [Cout,3,3,Cin])."""
    L = _lib.lib()
    B, H, W, Cin = xq.shape
    Cout = wq.shape[0]
    assert wq.shape == (Cout, 3, 3, Cin) and xs.shape == (B, H, W, Cin // 32) and ws.shape == (Cout, 3, 3, Cin // 32)
    for t in (xq, xs, wq, ws):
        _dev(t, torch.uint8)
    if out is None:
        out = torch.empty((B, H, W, Cout), dtype=torch.bfloat16, device=xq.device)
    rc = L.ssd_conv3x3_fwd_mxfp8(_ptr(xq), _ptr(xs), _ptr(wq), _ptr(ws), _ptr(bias), _ptr(out), B, H, W, Cin, Cout, 1 if relu else 0,
                                 _stream())
    _lib.check(rc, unsupported="block-scaled fp8 forward needs Cin % 128 == 0")
    return out


def conv2d_fwd_mxfp8(xq, xs, wq, ws, bias, stride, pad_t, pad_l, Ho, Wo, relu, want_bf16=True, want_fp8=False, out=None,
                     out_q=None, out_scale=None):
    """k x k (1 or 3) / stride 1 or 2 forward on block-scaled fp8 operands (quantize_mx_fp8 of x [B,H,W,Cin] and w
    [Cout,k,k,Cin]), TF-SAME pads as conv2d_fwd.  Returns the outputs asked for: the bf16 map, (q, scale) = its
    quantize_mx_fp8, or (bf16, q, scale) when both are wanted."""
    L = _lib.lib()
    B, H, W, Cin = xq.shape
    Cout, k = wq.shape[0], wq.shape[1]
    _mx_operands(xq, xs, wq, ws, (B, H, W, Cin), (Cout, k, k, Cin))
    out, out_q, out_scale, result = _mx_outputs((B, Ho, Wo, Cout), xq.device, want_bf16, want_fp8, out, out_q, out_scale)
    rc = L.ssd_conv2d_fwd_mxfp8(_ptr(xq), _ptr(xs), _ptr(wq), _ptr(ws), _ptr(bias), _ptr(out), _ptr(out_q), _ptr(out_scale),
                                B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo, 1 if relu else 0, _stream())
    _lib.check(rc, unsupported="block-scaled fp8 forward needs Cin % 128 == 0, k in (1, 3), stride in (1, 2), Cout % 8 == 0 "
                               "and Cout % 32 == 0 for an fp8 output")
    return result


def conv2d_fwd_pool_mxfp8(xq, xs, wq, ws, bias, stride, pad_t, pad_l, Ho, Wo, relu, same, want_bf16=True, want_fp8=False,
                          out=None, out_q=None, out_scale=None):
    """conv2d_fwd_mxfp8 (3x3, stride 1) followed by the 2x2 / stride-2 max pool (same: TF-SAME windows clipped at the edge,
    else VALID) in one launch that never stores the [B,Ho,Wo,Cout] map: maxpool2x2_fwd(conv2d_fwd_mxfp8(...), same) bit for
    bit.  Returns the pooled outputs asked for: the bf16 map, (q, scale) = its quantize_mx_fp8, or (bf16, q, scale)."""
    L = _lib.lib()
    B, H, W, Cin = xq.shape
    Cout, k = wq.shape[0], wq.shape[1]
    _mx_operands(xq, xs, wq, ws, (B, H, W, Cin), (Cout, k, k, Cin))
    Hp, Wp = ((Ho + 1) // 2, (Wo + 1) // 2) if same else (Ho // 2, Wo // 2)
    out, out_q, out_scale, result = _mx_outputs((B, Hp, Wp, Cout), xq.device, want_bf16, want_fp8, out, out_q, out_scale)
    _pooled_shapes((B, Hp, Wp), *((t, ch) for t, ch in ((out, Cout), (out_q, Cout), (out_scale, max(Cout // 32, 1))) if t is not None))
    rc = L.ssd_conv2d_fwd_pool_mxfp8(_ptr(xq), _ptr(xs), _ptr(wq), _ptr(ws), _ptr(bias), _ptr(out), _ptr(out_q), _ptr(out_scale),
                                     B, H, W, Cin, Cout, k, stride, pad_t, pad_l, Ho, Wo, 1 if relu else 0, Hp, Wp, _stream())
    _lib.check(rc, unsupported="pooled block-scaled fp8 forward needs k = 3, stride 1, Cin % 128 == 0 and Cout % 32 == 0")
    return result


def conv2d_bwd_data_mxfp8(dyq, dys, wtq, wts, relu_src, x_shape, stride, pad_t, pad_l, accumulate=False, want_bf16=True,
                          want_fp8=False, out=None, out_q=None, out_scale=None):
    """conv2d_bwd_data at stride 1 on block-scaled fp8 operands: quantize_mx_fp8 of dy [B,Ho,Wo,Cout] and of the transposed
    filters w_t [Cin,k,k,Cout] (k = 1 or 3); pad_t / pad_l are the forward's.  accumulate: out (bf16) += the result before
    the mask; relu_src (bf16 [B,H,W,Cin] or None): zero where it is <= 0.  Returns the outputs asked for: the bf16 dx,
    (q, scale) = its quantize_mx_fp8, or (bf16, q, scale) when both are wanted."""
    L = _lib.lib()
    B, H, W, Cin = x_shape
    _, Ho, Wo, Cout = dyq.shape
    k = wtq.shape[1]
    _mx_operands(dyq, dys, wtq, wts, (B, Ho, Wo, Cout), (Cin, k, k, Cout))
    if relu_src is not None:
        _bf(relu_src)
        assert relu_src.shape == tuple(x_shape)
    if stride != 1:
        raise NotImplementedError("block-scaled fp8 data gradient: stride 1 only (stride-2 layers use conv2d_bwd_data)")
    assert out is not None or not (want_bf16 and accumulate)
    out, out_q, out_scale, result = _mx_outputs(x_shape, dyq.device, want_bf16, want_fp8, out, out_q, out_scale)
    rc = L.ssd_conv2d_bwd_data_mxfp8(_ptr(dyq), _ptr(dys), _ptr(wtq), _ptr(wts), _ptr(relu_src), _ptr(out), _ptr(out_q),
                                     _ptr(out_scale), B, H, W, Cin, Cout, k, pad_t, pad_l, Ho, Wo, 1 if accumulate else 0, _stream())
    _lib.check(rc, unsupported="block-scaled fp8 data gradient needs Cout % 128 == 0, Cin % 32 == 0 and k in (1, 3)")
    return result


def add_relu_fwd_mxfp8(a, b, out=None, q=None, scale=None):
    """(out, q, scale): out = relu(a + b) exactly as add_relu_fwd, (q, scale) = quantize_mx_fp8(out), in one pass."""
    L = _lib.lib()
    _bf(a); _bf(b)
    assert a.shape == b.shape and a.shape[-1] % 32 == 0
    if out is None:
        out = torch.empty_like(a)
    q, scale = _mx_default(a.shape, a.device, q, scale)
    _caller_buffer("out", out, a.shape, torch.bfloat16)
    _caller_buffer("q", q, a.shape, torch.uint8)
    _caller_buffer("scale", scale, tuple(a.shape[:-1]) + (a.shape[-1] // 32,), torch.uint8)
    rc = L.ssd_add_relu_fwd_mxfp8(_ptr(a), _ptr(b), _ptr(out), _ptr(q), _ptr(scale), a.numel(), _stream())
    _lib.check(rc, unsupported="add_relu_fwd_mxfp8")
    return out, q, scale


def add_relu_fwd(a, b, out=None):
    """out = relu(a + b): the residual add of a ResNet bottleneck (bf16, any equal shapes with a multiple of 8 elements)."""
    L = _lib.lib()
    _bf(a); _bf(b)
    assert a.shape == b.shape
    if out is None:
        out = torch.empty_like(a)
    _caller_buffer("out", out, a.shape, torch.bfloat16)
    _lib.check(L.ssd_add_relu_fwd(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()))
    return out


def relu_mask_bwd(g, act, out=None, accumulate=False):
    """out (+)= g * (act > 0): the gradient of relu(a + b) w.r.t. an identity-skip input whose own activation is `act`."""
    L = _lib.lib()
    _bf(g); _bf(act)
    assert g.shape == act.shape
    if out is None:
        assert not accumulate
        out = torch.empty_like(g)
    _caller_buffer("out", out, g.shape, torch.bfloat16)
    _lib.check(L.ssd_relu_mask_bwd(_ptr(g), _ptr(act), _ptr(out), 1 if accumulate else 0, g.numel(), _stream()))
    return out


def maxpool3x3s2_fwd(x, out=None, code=None):
    """MaxPooling2D(3, strides=2, padding="same") (TF padding: the odd cell goes to the bottom / right); returns (y, code)."""
    L = _lib.lib()
    _bf(x)
    B, H, W, C = x.shape
    Ho, pt = same_pad(H, 3, 2)
    Wo, pl = same_pad(W, 3, 2)
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    if code is None:
        code = torch.empty((B, Ho, Wo, C // 8), dtype=torch.int32, device=x.device)
    _caller_buffer("out", out, (B, Ho, Wo, C), torch.bfloat16)
    _caller_buffer("code", code, (B, Ho, Wo, C // 8), torch.int32)
    _lib.check(L.ssd_maxpool3x3s2_fwd(_ptr(x), _ptr(out), _ptr(code), B, H, W, C, Ho, Wo, pt, pl, _stream()))
    return out, code


def maxpool3x3s2_bwd(code, dy, x_shape, out=None):
    L = _lib.lib()
    _bf(dy)
    B, H, W, C = x_shape
    Ho, pt = same_pad(H, 3, 2)
    Wo, pl = same_pad(W, 3, 2)
    assert dy.shape == (B, Ho, Wo, C) and code.shape == (B, Ho, Wo, C // 8)
    if out is None:
        out = torch.empty(x_shape, dtype=torch.bfloat16, device=dy.device)
    _caller_buffer("out", out, x_shape, torch.bfloat16)
    _lib.check(L.ssd_maxpool3x3s2_bwd(_ptr(code), _ptr(dy), _ptr(out), B, H, W, C, Ho, Wo, pt, pl, _stream()))
    return out


# ---- the SSD paper's VGG-16 pieces: dilated fc6 and the 3x3 / stride-1 pool5 (engine.VGG16_SSD300_TRUNK) --------------------
_ATROUS_RANGE = ("atrous 3x3 convolution: Cin must be a multiple of 64, Cout / Cout_pad / ldy multiples of 8, ldy >= Cout, "
                 "every tensor below 2^31 bytes; got %s")
_POOL3S1_RANGE = "3x3 / stride-1 max pooling: C must be a multiple of 8 and the map below 2^31 elements; got %s"


def _same_shape(name, t, shape):
    """A caller's output buffer: contiguous and of the shape this call writes, or ValueError (as _pooled_shapes)."""
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s of shape %s, contiguous %s: this call writes %s" % (name, tuple(t.shape), t.is_contiguous(), tuple(shape)))


def _caller_buffer(name, t, shape, dtype):
    """_same_shape, and of the element type this call writes: a device tensor of `dtype`, or ValueError."""
    _same_shape(name, t, shape)
    if t.dtype != dtype or not t.is_cuda:
        raise ValueError("%s is %s on %s: this call writes %s on the device" % (name, t.dtype, t.device, dtype))


def conv2d_atrous_fwd(x, w, bias, dilation, relu, out=None):
    """Conv2D(3, dilation_rate=dilation, padding="same") + bias (+ ReLU): x bf16 [B,H,W,Cin], w bf16 [Cout,3,3,Cin]."""
    L = _lib.lib()
    _bf(x); _bf(w)
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    assert w.shape == (Cout, 3, 3, Cin)
    if out is None:
        out = torch.empty((B, H, W, Cout), dtype=torch.bfloat16, device=x.device)
    _same_shape("out", out, (B, H, W, Cout))
    _lib.check(L.ssd_conv2d_atrous_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), B, H, W, Cin, Cout, dilation, 1 if relu else 0,
                                       _stream()),
               unsupported=_ATROUS_RANGE % ((B, H, W, Cin, Cout),))
    return out


def conv2d_atrous_bwd_data(dy, w_t, relu_src, x_shape, dilation, accumulate=False, out=None):
    """Its data gradient: dy bf16 [B,H,W,Cout_pad], w_t = weight_transpose(w) [Cin,3,3,Cout_pad]; out (+)= conv_T, then zeroed
    where relu_src <= 0 (relu_src may be `out` itself)."""
    L = _lib.lib()
    _bf(dy); _bf(w_t)
    B, H, W, Cin = x_shape
    cpad = dy.shape[3]
    assert dy.shape == (B, H, W, cpad) and w_t.shape == (Cin, 3, 3, cpad)
    if out is None:
        assert not accumulate
        out = torch.empty(tuple(x_shape), dtype=torch.bfloat16, device=dy.device)
    _same_shape("out", out, x_shape)
    _lib.check(L.ssd_conv2d_atrous_bwd_data(_ptr(dy), _ptr(w_t), _ptr(relu_src), _ptr(out), B, H, W, Cin, cpad, dilation,
                                            1 if accumulate else 0, _stream()),
               unsupported=_ATROUS_RANGE % ((B, H, W, Cin, cpad),))
    return out


def conv2d_atrous_bwd_weight(x, dy, Cout, dilation, dw=None, dbias=None, want_bias=True, ws=None):
    """Its weight and bias gradient (fp32, written): x bf16 [B,H,W,Cin], dy bf16 [B,H,W,ldy] (first Cout channels used)."""
    L = _lib.lib()
    _bf(x); _bf(dy)
    B, H, W, Cin = x.shape
    ldy = dy.shape[3]
    assert dy.shape == (B, H, W, ldy)
    if dw is None:
        dw = torch.empty((Cout, 3, 3, Cin), dtype=torch.float32, device=x.device)
    if dbias is None and want_bias:
        dbias = torch.empty((Cout,), dtype=torch.float32, device=x.device)
    _same_shape("dw", dw, (Cout, 3, 3, Cin))
    if dbias is not None:
        _same_shape("dbias", dbias, (Cout,))
    nbytes = L.ssd_conv2d_atrous_bwd_weight_workspace_bytes(B, H, W, Cin, Cout, ldy, dilation)
    wbuf = (ws or _conv_ws).get(nbytes, x.device)
    _lib.check(L.ssd_conv2d_atrous_bwd_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(dbias), B, H, W, Cin, Cout, ldy, dilation,
                                              _ptr(wbuf), wbuf.numel(), _stream()),
               unsupported=_ATROUS_RANGE % ((B, H, W, Cin, Cout, ldy),))
    return dw, dbias


def maxpool3x3s1_fwd(x, out=None, code=None):
    """MaxPooling2D(3, strides=1, padding="same"); returns (y, code), code int32 [B,H,W,C/8] in maxpool3x3s2_fwd's packing."""
    L = _lib.lib()
    _bf(x)
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, H, W, C), dtype=torch.bfloat16, device=x.device)
    if code is None:
        code = torch.empty((B, H, W, C // 8), dtype=torch.int32, device=x.device)
    _pooled_shapes((B, H, W), (out, C), (code, C // 8))
    _lib.check(L.ssd_maxpool3x3s1_fwd(_ptr(x), _ptr(out), _ptr(code), B, H, W, C, _stream()), unsupported=_POOL3S1_RANGE % ((B, H, W, C),))
    return out, code


def maxpool3x3s1_bwd(code, dy, x_shape, out=None):
    L = _lib.lib()
    _bf(dy)
    B, H, W, C = x_shape
    assert dy.shape == (B, H, W, C) and code.shape == (B, H, W, C // 8) and code.is_contiguous()
    if out is None:
        out = torch.empty(tuple(x_shape), dtype=torch.bfloat16, device=dy.device)
    _pooled_shapes((B, H, W), (out, C))
    _lib.check(L.ssd_maxpool3x3s1_bwd(_ptr(code), _ptr(dy), _ptr(out), B, H, W, C, _stream()), unsupported=_POOL3S1_RANGE % ((B, H, W, C),))
    return out


# ---- depthwise 3x3 convolution (MobileNet-SSD / SSDLite's other half: engine.MOBILENET_V1_SSD300_TRUNK's "dwconv" nodes) ---------
_DW_RANGE = "depthwise 3x3 convolution: C must be a multiple of 8 and every tensor below 2^31 bytes; got %s"


def dwconv3x3_fwd(x, w, bias, stride, pad_t, pad_l, Ho, Wo, relu, out=None):
    """DepthwiseConv2D(3, strides=stride, depth_multiplier=1) + bias (+ ReLU): x bf16 [B,H,W,C], w bf16 [3,3,C], bias fp32 [C] or
    None; explicit top / left padding (0 or 1), the rest implied by (Ho, Wo) as for conv2d_fwd."""
    L = _lib.lib()
    _bf(x); _bf(w)
    B, H, W, C = x.shape
    assert w.shape == (3, 3, C)
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    _caller_buffer("out", out, (B, Ho, Wo, C), torch.bfloat16)
    _lib.check(L.ssd_dwconv3x3_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), B, H, W, C, stride, pad_t, pad_l, Ho, Wo,
                                   1 if relu else 0, _stream()),
               unsupported=_DW_RANGE % ((B, H, W, C, stride),))
    return out


def dwconv3x3_bwd_data(dy, w, relu_src, x_shape, stride, pad_t, pad_l, accumulate=False, out=None):
    """Its data gradient: dy bf16 [B,Ho,Wo,C], w the forward filters [3,3,C]; out (+)= the gathered gradient, then zeroed where
    relu_src <= 0 (relu_src may be `out` itself)."""
    L = _lib.lib()
    _bf(dy); _bf(w)
    B, H, W, C = x_shape
    _, Ho, Wo, _ = dy.shape
    assert dy.shape == (B, Ho, Wo, C) and w.shape == (3, 3, C)
    if out is None:
        assert not accumulate
        out = torch.empty(tuple(x_shape), dtype=torch.bfloat16, device=dy.device)
    _caller_buffer("out", out, x_shape, torch.bfloat16)
    if relu_src is not None:
        _caller_buffer("relu_src", relu_src, x_shape, torch.bfloat16)
    _lib.check(L.ssd_dwconv3x3_bwd_data(_ptr(dy), _ptr(w), _ptr(relu_src), _ptr(out), B, H, W, C, stride, pad_t, pad_l, Ho, Wo,
                                        1 if accumulate else 0, _stream()),
               unsupported=_DW_RANGE % ((B, H, W, C, stride),))
    return out


def dwconv3x3_fwd_relubits(x, w, bias, stride, pad_t, pad_l, Ho, Wo, bits, out=None):
    """dwconv3x3_fwd with ReLU that also writes the sign bytes of its output (uint8 [B,Ho,Wo,C/8], conv2d_fwd_relubits's layout)."""
    L = _lib.lib()
    _bf(x); _bf(w)
    B, H, W, C = x.shape
    assert w.shape == (3, 3, C)
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=torch.bfloat16, device=x.device)
    _caller_buffer("out", out, (B, Ho, Wo, C), torch.bfloat16)
    _caller_buffer("bits", bits, (B, Ho, Wo, C // 8), torch.uint8)
    _lib.check(L.ssd_dwconv3x3_fwd_relubits(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), _ptr(bits), B, H, W, C, stride, pad_t, pad_l,
                                            Ho, Wo, _stream()),
               unsupported=_DW_RANGE % ((B, H, W, C, stride),))
    return out


def dwconv3x3_bwd_data_bits(dy, w, bits, x_shape, stride, pad_t, pad_l, accumulate=False, out=None):
    """dwconv3x3_bwd_data with the ReLU mask given as the sign bytes of the layer in front (uint8 [B,H,W,C/8]): same result, one
    mask byte per 16-byte group instead of sixteen."""
    L = _lib.lib()
    _bf(dy); _bf(w)
    B, H, W, C = x_shape
    _, Ho, Wo, _ = dy.shape
    assert dy.shape == (B, Ho, Wo, C) and w.shape == (3, 3, C)
    if out is None:
        assert not accumulate
        out = torch.empty(tuple(x_shape), dtype=torch.bfloat16, device=dy.device)
    _caller_buffer("out", out, x_shape, torch.bfloat16)
    _caller_buffer("bits", bits, (B, H, W, C // 8), torch.uint8)
    _lib.check(L.ssd_dwconv3x3_bwd_data_bits(_ptr(dy), _ptr(w), _ptr(bits), _ptr(out), B, H, W, C, stride, pad_t, pad_l, Ho, Wo,
                                             1 if accumulate else 0, _stream()),
               unsupported=_DW_RANGE % ((B, H, W, C, stride),))
    return out


def dwconv3x3_bwd_weight(x, dy, stride, pad_t, pad_l, dw=None, dbias=None, want_bias=True, ws=None):
    """Its weight and bias gradient (fp32 [3,3,C] and [C], written): x bf16 [B,H,W,C], dy bf16 [B,Ho,Wo,C]."""
    L = _lib.lib()
    _bf(x); _bf(dy)
    B, H, W, C = x.shape
    _, Ho, Wo, _ = dy.shape
    assert dy.shape == (B, Ho, Wo, C)
    if dw is None:
        dw = torch.empty((3, 3, C), dtype=torch.float32, device=x.device)
    if dbias is None and want_bias:
        dbias = torch.empty((C,), dtype=torch.float32, device=x.device)
    _caller_buffer("dw", dw, (3, 3, C), torch.float32)
    if dbias is not None:
        _caller_buffer("dbias", dbias, (C,), torch.float32)
    nbytes = L.ssd_dwconv3x3_bwd_weight_workspace_bytes(B, H, W, C, stride, Ho, Wo)
    wbuf = (ws or _conv_ws).get(nbytes, x.device)
    _lib.check(L.ssd_dwconv3x3_bwd_weight(_ptr(x), _ptr(dy), _ptr(dw), _ptr(dbias), B, H, W, C, stride, pad_t, pad_l, Ho, Wo,
                                          _ptr(wbuf), wbuf.numel(), _stream()),
               unsupported=_DW_RANGE % ((B, H, W, C, stride),))
    return dw, dbias


# ---- ... and their inference fp8 forms (engine.SSDEngine(fp8_inference=True)) --------------------------------------------------
def conv2d_atrous_fwd_mxfp8(xq, xs, wq, ws, bias, dilation, relu, want_bf16=True, want_fp8=False, out=None, out_q=None,
                            out_scale=None):
    """conv2d_atrous_fwd on block-scaled fp8 operands (quantize_mx_fp8 of x [B,H,W,Cin] and w [Cout,3,3,Cin]); outputs as
    conv2d_fwd_mxfp8: the bf16 map, (q, scale) = its quantize_mx_fp8, or (bf16, q, scale).  At dilation 1 it is
    conv2d_fwd_mxfp8 at 3x3 / stride 1 / pads 1 bit for bit."""
    L = _lib.lib()
    B, H, W, Cin = xq.shape
    Cout = wq.shape[0]
    _mx_operands(xq, xs, wq, ws, (B, H, W, Cin), (Cout, 3, 3, Cin))
    out, out_q, out_scale, result = _mx_outputs((B, H, W, Cout), xq.device, want_bf16, want_fp8, out, out_q, out_scale)
    for name, t, ch in (("out", out, Cout), ("out_q", out_q, Cout), ("out_scale", out_scale, max(Cout // 32, 1))):
        if t is not None:
            _same_shape(name, t, (B, H, W, ch))
    rc = L.ssd_conv2d_atrous_fwd_mxfp8(_ptr(xq), _ptr(xs), _ptr(wq), _ptr(ws), _ptr(bias), _ptr(out), _ptr(out_q), _ptr(out_scale),
                                       B, H, W, Cin, Cout, dilation, 1 if relu else 0, _stream())
    _lib.check(rc, unsupported="block-scaled fp8 atrous forward needs Cin %% 128 == 0, Cout %% 8 == 0, Cout %% 32 == 0 for an fp8 "
                               "output and every tensor below 2^31 bytes; got %s" % ((B, H, W, Cin, Cout),))
    return result


_POOL_MX_RANGE = "quantising max pooling: C must be a multiple of 32 and the map below 2^31 elements; got %s"


def _pool_mx_outputs(x, shape, want_bf16, out, q, scale):
    _bf(x)
    if want_bf16 and out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=x.device)
    q, scale = _mx_default(shape, x.device, q, scale)
    _pooled_shapes(shape[:3], *((t, ch) for t, ch in ((out if want_bf16 else None, shape[3]), (q, shape[3]),
                                                     (scale, max(shape[3] // 32, 1))) if t is not None))
    return (out if want_bf16 else None), q, scale


def maxpool2x2_fwd_mxfp8(x, same=False, want_bf16=False, out=None, q=None, scale=None):
    """(q, scale) = quantize_mx_fp8(maxpool2x2_fwd(x, same)) bit for bit, in one pass over the bf16 map x [B,H,W,C]; with
    want_bf16 (out, q, scale): the pooled bf16 map as well.  Inference only: no winner codes."""
    L = _lib.lib()
    B, H, W, C = x.shape
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if same else (H // 2, W // 2)
    out, q, scale = _pool_mx_outputs(x, (B, Ho, Wo, C), want_bf16, out, q, scale)
    _lib.check(L.ssd_maxpool2x2_fwd_mxfp8(_ptr(x), _ptr(out), _ptr(q), _ptr(scale), B, H, W, C, Ho, Wo, _stream()),
               unsupported=_POOL_MX_RANGE % ((B, H, W, C),))
    return (out, q, scale) if want_bf16 else (q, scale)


def maxpool3x3s1_fwd_mxfp8(x, want_bf16=False, out=None, q=None, scale=None):
    """(q, scale) = quantize_mx_fp8(maxpool3x3s1_fwd(x)[0]) bit for bit, in one pass; with want_bf16 (out, q, scale)."""
    L = _lib.lib()
    B, H, W, C = x.shape
    out, q, scale = _pool_mx_outputs(x, (B, H, W, C), want_bf16, out, q, scale)
    _lib.check(L.ssd_maxpool3x3s1_fwd_mxfp8(_ptr(x), _ptr(out), _ptr(q), _ptr(scale), B, H, W, C, _stream()),
               unsupported=_POOL_MX_RANGE % ((B, H, W, C),))
    return (out, q, scale) if want_bf16 else (q, scale)


def head_grad_pack(dloc, dconf, hw, per_cell, classes, npad, level_off, out=None):
    L = _lib.lib()
    _bf(dloc); _bf(dconf)
    B, A, _ = dloc.shape
    if out is None:
        out = torch.empty((B, hw, npad), dtype=torch.bfloat16, device=dloc.device)
    _lib.check(L.ssd_head_grad_pack(_ptr(dloc), _ptr(dconf), _ptr(out), B, hw, per_cell, classes, npad, A, level_off,
                                    _stream()))
    return out


def cast_bf16(src, dst=None):
    L = _lib.lib()
    _dev(src, torch.float32)
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.bfloat16, device=src.device)
    _lib.check(L.ssd_cast_bf16(_ptr(src), _ptr(dst), src.numel(), _stream()))
    return dst


class EmaSpec:
    """An exponential moving average of the weights, kept beside them for validation, detection and the saved model
    (ema_step): e' = decay e + (1 - decay) p after every optimizer step.  warmup: TF ExponentialMovingAverage's num_updates rule,
    decay_t = min(decay, (1 + t) / (10 + t)) at the t-th update from 0 -- the first updates follow the weights closely instead
    of remembering the random initialisation for 1 / (1 - decay) steps.  decay in (0, 1), else ValueError."""

    def __init__(self, decay=0.9998, warmup=True):
        if isinstance(decay, bool) or not isinstance(decay, (int, float, np.integer, np.floating)) or not 0.0 < decay < 1.0:
            raise ValueError("ema decay must be a number in (0, 1), not %r" % (decay,))
        if not isinstance(warmup, bool):
            raise ValueError("ema warmup must be True or False, not %r" % (warmup,))
        self.decay = float(decay)
        self.warmup = warmup

    @classmethod
    def of(cls, v):
        """None -> None (no average); a number -> that decay; an EmaSpec -> itself; a dict with the keys decay / warmup -> a
        spec.  ValueError for anything else."""
        if v is None:
            return None
        if isinstance(v, cls):
            return v
        if isinstance(v, dict):
            unknown = sorted(set(v) - {"decay", "warmup"}, key=str)
            if unknown:
                raise ValueError("ema: unknown key(s) %s (known: decay, warmup)" % ", ".join(repr(k) for k in unknown))
            return cls(**v)
        if not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)):
            return cls(decay=v)
        raise ValueError("ema must be None, a decay in (0, 1), a dict(decay, warmup) or an ops.EmaSpec, not %r" % (v,))

    def decay_at(self, t):
        """The decay of update t (t = the updates made before it), a Python float (double)."""
        if t < 0:
            raise ValueError("ema update index must be >= 0, not %r" % (t,))
        return min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay

    def one_minus_decay(self, t):
        """What ema_step gets for update t: float32(1 - decay_at(t)), the difference taken in double."""
        return float(np.float32(1.0 - self.decay_at(t)))

    def __repr__(self):
        return "EmaSpec(decay=%r, warmup=%r)" % (self.decay, self.warmup)


def ema_step(ema, param, one_minus_decay):
    """ssd_ema_step: ema += one_minus_decay * (param - ema) in place (both fp32, contiguous, the same element count, a multiple
    of the optimizer block); 1 copies param bit for bit, 0 leaves ema as it is.  ValueError (SSD_ERR_VALUE, nothing launched)
    for a factor outside [0, 1], a count that is no multiple of the block or overlapping operands."""
    L = _lib.lib()
    _dev(ema, torch.float32); _dev(param, torch.float32)
    assert ema.numel() == param.numel(), (ema.numel(), param.numel())
    _lib.check(L.ssd_ema_step(_ptr(ema), _ptr(param), ema.numel(), float(one_minus_decay), _stream()))
    return ema
