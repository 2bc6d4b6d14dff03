"""CPU: the IoU box terms (GIoU / DIoU / CIoU; include/ssd_hip.h, the _box entries).  The oracle of tests/box_iou_oracle.py against
torch autograd and central differences, its invariances and edge properties, its f32 restatement against the GPU test's bounds,
the case builder, LossSpec / YAML validation, and the host-side refusals of the four new entries."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import box_iou_cases as K
from tests import box_iou_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def big_rows(n=20000, seed=11):
    """n kink-free rows drawn as the cases draw them (and the fraction of first draws that lay near a kink)"""
    rng = np.random.default_rng(seed)
    wh = K.random_priors(rng, n)[:, 2:]
    t = K.draw_loc(rng, (n, 4))
    g = (0.5 * rng.standard_normal((n, 4))).astype(np.float32)
    bad = K.near_kink(wh, t, g)
    return wh[~bad], t[~bad], g[~bad], float(bad.mean())


# ---------------------------------------------------------------------------------------------------- the case builder
def test_cases_are_what_the_tests_need():
    *_, frac = big_rows()
    print("first draws near a kink:", frac)
    assert frac < 0.02
    for shape in K.SHAPES:
        c = K.make_case(*shape)
        B, A, C = shape
        mask = c["gt_mask"].astype(bool)
        assert not mask[B - 2].any() and mask[B - 1, A - 1] and mask.sum() >= 10
        assert (B * A) % 128 != 0 and B * A > 256                        # three or more row blocks, the last ragged
        assert np.array_equal(K.to_bf16(c["loc"]), c["loc"]) and np.array_equal(K.to_bf16(c["conf"]), c["conf"])
        assert (c["gt_cls"][~mask] >= C).all() and (c["priors"][:, 2:] > 0).all()
        wh, t, g = K.positives(c)
        assert not K.near_kink(wh, t, g).any()
        # overlapping and disjoint pairs both occur
        L, _ = O.rows("giou", wh, t, g)
        assert (L < 1.0).any() and (L > 1.0).any()


# ---------------------------------------------------------------------------------------------------- the gradient
def torch_loss(kind, wh, t, g):
    """the definition in torch float64, for autograd (max / min / clamp as torch has them: the rows are kink-free)"""
    import torch
    dw, dh = wh[:, 0], wh[:, 1]
    cx, cy = t[:, 0] * dw, t[:, 1] * dh
    w, h = dw * torch.exp(t[:, 2].clamp(-O.W, O.W)), dh * torch.exp(t[:, 3].clamp(-O.W, O.W))
    gx, gy = g[:, 0] * dw, g[:, 1] * dh
    gw, gh = dw * torch.exp(g[:, 2].clamp(-O.W, O.W)), dh * torch.exp(g[:, 3].clamp(-O.W, O.W))
    x1, x2, y1, y2 = cx - w / 2, cx + w / 2, cy - h / 2, cy + h / 2
    X1, X2, Y1, Y2 = gx - gw / 2, gx + gw / 2, gy - gh / 2, gy + gh / 2
    iw = (torch.minimum(x2, X2) - torch.maximum(x1, X1)).clamp(min=0)
    ih = (torch.minimum(y2, Y2) - torch.maximum(y1, Y1)).clamp(min=0)
    I = iw * ih
    U = w * h + gw * gh - I
    iou = I / U
    cw, ch = torch.maximum(x2, X2) - torch.minimum(x1, X1), torch.maximum(y2, Y2) - torch.minimum(y1, Y1)
    if kind == "giou":
        return 1 - iou + (cw * ch - U) / (cw * ch)
    L = 1 - iou + ((cx - gx) ** 2 + (cy - gy) ** 2) / (cw ** 2 + ch ** 2)
    if kind == "ciou":
        v = 4 / np.pi ** 2 * (torch.atan(gw / gh) - torch.atan(w / h)) ** 2
        alpha = torch.where(v > 0, v / ((1 - iou) + v), torch.zeros_like(v)).detach()
        L = L + alpha * v
    return L


@pytest.mark.parametrize("kind", O.KINDS)
def test_oracle_gradient_is_autograd(kind):
    torch = pytest.importorskip("torch")
    wh, t, g, _ = big_rows(4000)
    tt = torch.tensor(t, dtype=torch.float64, requires_grad=True)
    L = torch_loss(kind, torch.tensor(wh), tt, torch.tensor(g, dtype=torch.float64))
    L.sum().backward()
    L0, d0 = O.rows(kind, wh, t, g)
    assert np.abs(L.detach().numpy() - L0).max() <= 1e-12
    err = np.abs(tt.grad.numpy() - d0).max()
    print(kind, "oracle gradient against autograd:", err)
    assert err <= 1e-10


@pytest.mark.parametrize("kind", O.KINDS)
def test_oracle_gradient_is_the_central_difference(kind):
    """CIoU's alpha is held constant, as in the definition: the difference is taken of L with alpha frozen at the point"""
    wh, t, g, _ = big_rows(4000)
    t = t.astype(np.float64)
    L0, d0 = O.rows(kind, wh, t, g)
    eps = 1e-6

    def v_of(tp):
        w, h = wh[:, 0] * np.exp(np.clip(tp[:, 2], -O.W, O.W)), wh[:, 1] * np.exp(np.clip(tp[:, 3], -O.W, O.W))
        gw, gh = wh[:, 0] * np.exp(np.clip(g[:, 2], -O.W, O.W)), wh[:, 1] * np.exp(np.clip(g[:, 3], -O.W, O.W))
        return 4 / np.pi ** 2 * (np.arctan(gw / gh) - np.arctan(w / h)) ** 2

    v0 = v_of(t)
    alpha0 = np.where(v0 > 0, (L0 - O.rows("diou", wh, t, g)[0]) / np.where(v0 > 0, v0, 1.0), 0.0) if kind == "ciou" else None

    def loss(tp):
        if kind != "ciou":
            return O.rows(kind, wh, tp, g)[0]
        return O.rows("diou", wh, tp, g)[0] + alpha0 * v_of(tp)

    worst = 0.0
    for k in range(4):
        e = np.zeros(4)
        e[k] = eps
        num = (loss(t + e) - loss(t - e)) / (2 * eps)
        scale = np.abs(d0).max(axis=1) + 1e-3
        worst = max(worst, float((np.abs(num - d0[:, k]) / scale).max()))
    print(kind, "central difference, relative to the row's largest component:", worst)
    assert worst <= 1e-5                                                  # O(eps^2 L''') with eps = 1e-6, curvature up to ~1e3 / unit


# ---------------------------------------------------------------------------------------------------- properties
def test_invariances_and_edges():
    wh, t, g, _ = big_rows(3000)
    rng = np.random.default_rng(3)
    for kind in O.KINDS:
        L0, d0 = O.rows(kind, wh, t, g)
        # translation: the priors' centres do not enter (the full-loss wrapper takes [A,4] priors)
        A = 64
        pri = np.concatenate([rng.random((A, 2)), wh[:A]], axis=1)
        mask = np.ones((1, A), np.uint8)
        a = O.box_term(kind, pri, g[None, :A], mask, t[None, :A])
        pri2 = pri.copy()
        pri2[:, :2] += rng.standard_normal((A, 2)) * 100.0
        b = O.box_term(kind, pri2, g[None, :A], mask, t[None, :A])
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and not a[2]
        # pred == target: zero loss
        Lz, dz = O.rows(kind, wh, g, g)
        assert np.abs(Lz).max() <= 1e-6, (kind, np.abs(Lz).max())
        Lz32, _ = O.rows(kind, wh, g, g, np.float32)
        assert np.abs(Lz32).max() <= 1e-6, (kind, np.abs(Lz32).max())
        # bounded: IoU losses lie in [0, 2] (GIoU, DIoU) or [0, 3] (CIoU)
        assert L0.min() >= 0 and L0.max() <= (3.0 if kind == "ciou" else 2.0)
    # GIoU under anisotropic scaling of the priors
    s = np.array([3.0, 0.25])
    L0, d0 = O.rows("giou", wh, t, g)
    L1, d1 = O.rows("giou", wh * s, t, g)
    assert np.abs(L1 - L0).max() <= 1e-12 and np.abs(d1 - d0).max() <= 1e-9 * np.abs(d0).max()
    # DIoU / CIoU under isotropic scaling
    for kind in ("diou", "ciou"):
        L0, d0 = O.rows(kind, wh, t, g)
        L1, d1 = O.rows(kind, wh * 7.0, t, g)
        assert np.abs(L1 - L0).max() <= 1e-12 and np.abs(d1 - d0).max() <= 1e-9 * np.abs(d0).max()
    # CIoU == DIoU where the aspect ratios agree: t2 - g2 == t3 - g3
    t2 = t.astype(np.float64).copy()
    t2[:, 3] = g[:, 3].astype(np.float64) + (t2[:, 2] - g[:, 2])
    keep = (np.abs(t2[:, 2:]) < O.W - 0.01).all(axis=1)
    Lc, dc = O.rows("ciou", wh[keep], t2[keep], g[keep])
    Ld, dd = O.rows("diou", wh[keep], t2[keep], g[keep])
    assert np.abs(Lc - Ld).max() <= 1e-12 and np.abs(dc - dd).max() <= 1e-9
    # the clamp: a zero gradient component, and the loss does not move beyond W
    tc = t.astype(np.float64).copy()
    tc[:, 2], tc[::2, 3] = O.W + 0.5, -O.W - 1.0
    for kind in O.KINDS:
        Lc, dc = O.rows(kind, wh, tc, g)
        assert (dc[:, 2] == 0).all() and (dc[::2, 3] == 0).all() and (dc[1::2, 3] != 0).any()
        tc2 = tc.copy()
        tc2[:, 2] += 1.0
        assert np.array_equal(O.rows(kind, wh, tc2, g)[0], Lc)
        assert np.isfinite(Lc).all() and np.isfinite(dc).all()


def test_ties_follow_the_strict_rule():
    """equal boxes: every corner ties, so no max / min passes a gradient to the prediction and only the box's own area moves
    IoU (dL/dw = I h / U^2 = 1 / w at w == gw: the strict rule's one-sided derivative); touching boxes (iw == 0 exactly):
    max(0, .) passes nothing, so IoU's gradient is zero and only the hull / centre terms pull"""
    wh = np.array([[0.2, 0.3]])
    g = np.array([[0.1, -0.2, 0.3, 0.1]])
    for kind in O.KINDS:
        L, d = O.rows(kind, wh, g, g)
        assert L[0] == 0.0 and d[0, 0] == 0.0 and d[0, 1] == 0.0
        want = 0.0 if kind == "giou" else 1.0           # w dL/dw = w I h / U^2 = 1; GIoU's hull term -U h / (cw ch)^2 cancels it
        assert abs(d[0, 2] - want) <= 1e-12 and abs(d[0, 3] - want) <= 1e-12
    t = np.array([[1.0, 0.0, 0.0, 0.0]])                                  # x1 = 0.1 = X2
    g = np.array([[0.0, 0.0, 0.0, 0.0]])
    L, d = O.rows("giou", wh, t, g)
    assert abs(L[0] - 1.0) <= 1e-12 and d[0, 0] > 0.0 and d[0, 1] == 0.0  # the hull grows with cx: bx2 = 1, bx1 = 0
    assert abs(d[0, 0] - 0.2 * (0.12 * 0.3) / 0.12 ** 2) <= 1e-12          # d_w U ch / Cc^2 with U == Cc == 0.12
    L, d = O.rows("diou", wh, t, g)
    assert d[0, 0] > 0.0 and d[0, 1] == 0.0


def test_status_3_in_the_oracle():
    c = K.make_case(*K.SHAPES[0])
    pri = c["priors"].copy()
    b, a = np.nonzero(c["gt_mask"])
    assert not O.box_term("giou", pri, c["gt_loc"], c["gt_mask"], c["loc"])[2]
    pri[a[0], 2] = 0.0
    for kind in O.KINDS:
        assert O.box_term(kind, pri, c["gt_loc"], c["gt_mask"], c["loc"])[2]
    loc = c["loc"].copy()
    loc[b[0], a[0], 1] = np.inf
    assert O.box_term("ciou", c["priors"], c["gt_loc"], c["gt_mask"], loc)[2]
    r = O.multibox_loss("ciou", c["priors"], c["gt_cls"], c["gt_loc"], c["gt_mask"], loc, c["conf"])
    assert r["status"] == 3


# ---------------------------------------------------------------------------------------------------- the f32 restatement
@pytest.mark.parametrize("kind", O.KINDS)
def test_f32_restatement_meets_the_gpu_bounds_with_a_factor_of_three(kind):
    wh, t, g, _ = big_rows()
    L64, d64 = O.rows(kind, wh, t, g)
    L32, d32 = O.rows(kind, wh, t, g, np.float32)
    assert L32.dtype == np.float32 and d32.dtype == np.float32
    rel = np.abs(d32.astype(np.float64) - d64).max(axis=1) / np.abs(d64).max(axis=1)
    scal = abs(L32.astype(np.float64).sum() - L64.sum()) / L64.sum()
    print(kind, "f32 gradient error / row's largest component:", rel.max(), "sum of the losses, relative:", scal)
    assert rel.max() <= 1e-4 / 3 and scal <= 1e-4 / 3
    for shape in K.SHAPES:
        c = K.make_case(*shape)
        a = O.box_term(kind, c["priors"], c["gt_loc"], c["gt_mask"], c["loc"], K.LOC_WEIGHT)
        b = O.box_term(kind, c["priors"], c["gt_loc"], c["gt_mask"], c["loc"], K.LOC_WEIGHT, dtype=np.float32)
        assert abs(a[0] - b[0]) <= 1e-4 / 3 * abs(a[0])
        assert (np.abs(a[1] - b[1]) <= K.dloc_bound(a[1]) / 3).all()


# ---------------------------------------------------------------------------------------------------- configuration
def test_loss_spec_box():
    from ssd_object_detection_amd import ops
    assert ops.LossSpec.BOXES == ("smooth_l1", "giou", "diou", "ciou")
    assert ops.LossSpec().box == "smooth_l1" and ops.LossSpec("multibox").box_kind == 0
    for k, name in enumerate(ops.LossSpec.BOXES):
        for kind in ("multibox", "softmax_focal"):
            s = ops.LossSpec(kind, box=name)
            assert s.box == name and s.box_kind == k
    # the repr is what it was for smooth L1 and names the box otherwise
    assert repr(ops.LossSpec("multibox", 2, 0.5)) == "LossSpec(kind='multibox', neg_pos_ratio=2, loc_weight=0.5)"
    assert repr(ops.LossSpec()) == "LossSpec(kind='reference', neg_pos_ratio=3, loc_weight=1.0)"
    assert repr(ops.LossSpec("softmax_focal")) == "LossSpec(kind='softmax_focal', gamma=2.0, alpha=0.25, loc_weight=1.0)"
    assert repr(ops.LossSpec("multibox", box="giou")) == "LossSpec(kind='multibox', neg_pos_ratio=3, loc_weight=1.0, box='giou')"
    assert repr(ops.LossSpec("softmax_focal", box="ciou")).endswith("loc_weight=1.0, box='ciou')")
    for bad in (dict(kind="multibox", box="iou"), dict(kind="multibox", box=1), dict(kind="multibox", box=None),
                dict(kind="softmax_focal", box="GIoU"), dict(kind="reference", box="giou"), dict(box="ciou")):
        with pytest.raises(ValueError):
            ops.LossSpec(**bad)
    assert ops.LossSpec("reference", box="smooth_l1").box == "smooth_l1"
    # the module constants are the header's
    from ssd_object_detection_amd import _lib
    assert (_lib.SSD_BOX_SMOOTH_L1, _lib.SSD_BOX_GIOU, _lib.SSD_BOX_DIOU, _lib.SSD_BOX_CIOU) == (0, 1, 2, 3)


def test_loss_from_config_box():
    from ssd_object_detection_amd.tools.train import loss_from_config, load_config

    def cfg(section):
        return {"model": {"train": {"loss": section}}}

    s = loss_from_config(cfg({"kind": "multibox", "box": "giou", "neg_pos_ratio": 2}))
    assert (s.kind, s.box, s.neg_pos_ratio) == ("multibox", "giou", 2)
    s = loss_from_config(cfg({"kind": "softmax_focal", "box": "ciou", "gamma": 1.5}))
    assert (s.kind, s.box, s.gamma) == ("softmax_focal", "ciou", 1.5)
    assert loss_from_config(cfg({"kind": "multibox"})).box == "smooth_l1"
    assert loss_from_config(cfg({"kind": "multibox", "box": "smooth_l1"})).box == "smooth_l1"
    for bad in ({"kind": "reference", "box": "giou"}, {"box": "giou"}, {"kind": "reference", "box": "smooth_l1"},
                {"kind": "multibox", "box": "iou"}, {"kind": "softmax_focal", "box": 2}, {"kind": "multibox", "boxes": "giou"}):
        with pytest.raises(ValueError):
            loss_from_config(cfg(bad))
    path = os.path.join(ROOT, "ssd-object-detection_amd", "config", "default.yml")
    assert loss_from_config(load_config(path)) is None


def test_ssd_loss_stays_a_staticmethod_with_priors_last():
    import inspect
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    assert isinstance(inspect.getattr_static(SSDObjectDetectionModel, "_ssd_loss"), staticmethod)
    params = list(inspect.signature(SSDObjectDetectionModel._ssd_loss).parameters.values())
    assert [p.name for p in params] == ["y_true", "y_pred", "heads", "loss", "priors"] and params[-1].default is None


# ---------------------------------------------------------------------------------------------------- the library
def test_box_entries_are_declared_and_refuse_on_the_host():
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    names = ("ssd_multibox_loss_box_fwd_bwd", "ssd_multibox_loss_box_fwd_bwd_heads", "ssd_softmax_focal_loss_box_fwd_bwd",
             "ssd_softmax_focal_loss_box_fwd_bwd_heads")
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib._SIGNATURES and hasattr(L, n), n
        old = n.replace("_box_", "_")
        assert _lib._SIGNATURES[n] == (_lib._SIGNATURES[old][0], _lib._SIGNATURES[old][1] + [ctypes.c_int, ctypes.c_void_p])
    d = ctypes.c_void_p(0x1000)                                         # never dereferenced on these paths
    V, U, Wk = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED, _lib.SSD_ERR_WORKSPACE
    hg = _lib.HeadGrads()
    hg.levels = 2
    for l, (hw, n) in enumerate(((1444, 4), (361, 6))):
        hg.hw[l], hg.per_cell[l], hg.npad[l] = hw, n, (n * 85 + 7) // 8 * 8
        hg.rows[l], hg.row_of_pixel[l], hg.pixel_of_row[l] = 0x1000, 0x1000, 0x1000
    hg.count = 0x1000
    A2 = 1444 * 4 + 361 * 6
    hgp = ctypes.byref(hg)

    def mb(kind, pri, ws_bytes=0, **kw):
        return L.ssd_multibox_loss_box_fwd_bwd(d, d, kw.get("dtype", 0), d, d, d, 2, 8732, kw.get("C", 81), kw.get("ratio", 3), 1.0, 1.0,
                                               d, d, d, d, ws_bytes, None, kind, pri)

    def mbh(kind, pri, ws_bytes=0, **kw):
        return L.ssd_multibox_loss_box_fwd_bwd_heads(d, d, kw.get("dtype", 1), d, d, d, 2, A2, kw.get("C", 81), kw.get("ratio", 3),
                                                     1.0, 1.0, d, hgp, d, ws_bytes, None, kind, pri)

    def sf(kind, pri, ws_bytes=0, **kw):
        return L.ssd_softmax_focal_loss_box_fwd_bwd(d, d, kw.get("dtype", 0), d, d, d, 2, 8732, kw.get("C", 81), kw.get("gamma", 2.0),
                                                    0.25, 1.0, 1.0, d, d, d, d, ws_bytes, None, kind, pri)

    def sfh(kind, pri, ws_bytes=0, **kw):
        return L.ssd_softmax_focal_loss_box_fwd_bwd_heads(d, d, kw.get("dtype", 1), d, d, d, 2, A2, kw.get("C", 81),
                                                          kw.get("gamma", 2.0), 0.25, 1.0, 1.0, d, hgp, d, ws_bytes, None, kind, pri)

    for fn in (mb, mbh, sf, sfh):
        for kind in (-1, 4, 100):
            assert fn(kind, d) == V, (fn.__name__, kind)                 # an unknown kind
        for kind in (1, 2, 3):
            assert fn(kind, None) == V, (fn.__name__, kind)              # an IoU kind without priors
            assert fn(kind, d) == Wk, (fn.__name__, kind)                # accepted up to the workspace (ws_bytes = 0)
        assert fn(0, None) == Wk and fn(0, d) == Wk                      # kind 0 does not need them
        assert fn(4, d, C=304) == V and fn(1, d, C=304) == U             # the kind is checked with the values, before the bounds
    assert mb(1, d, ratio=0) == V and sf(1, d, gamma=9.0) == V and mb(1, d, dtype=2) == V
    assert mbh(1, d, dtype=0) == U and sfh(1, d, dtype=0) == U           # the rows forms stay bf16 only
