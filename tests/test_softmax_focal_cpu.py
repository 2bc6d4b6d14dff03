"""CPU suite for the opt-in softmax focal loss: the float64 oracle against hand-worked values and finite differences, the
designed rows of the GPU test against float32 evaluations (the stable form meets the GPU test's bound, the two naive forms do
not), the configuration plumbing, and the host-side refusals of the new entry points (no launch: callable without a GPU)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import softmax_focal_cases as K
from tests import softmax_focal_oracle as F

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_case(B=2, A=20, C=5, seed=4):
    rng = np.random.default_rng(seed)
    conf = rng.standard_normal((B, A, C))
    loc, gt_loc = 1.5 * rng.standard_normal((B, A, 4)), rng.standard_normal((B, A, 4))
    mask = rng.random((B, A)) < 0.3
    mask[0, 0] = True
    gt_cls = rng.integers(0, C - 1, (B, A)).astype(np.int32)
    return gt_cls, gt_loc, mask, loc, conf


# ---------------------------------------------------------------------------------------------------- the oracle
def test_oracle_hand_worked_values():
    """C = 2, logits (0, 0), gamma 2, alpha 0.25: p_t = q = 1/2, so a positive gives 0.25 * 0.25 * ln 2 and a background anchor
    0.75 * 0.25 * ln 2; the gradient row follows from the definition by hand as well."""
    conf = np.zeros((1, 2, 2))
    mask = np.array([[True, False]])
    z4 = np.zeros((1, 2, 4))
    r = F.softmax_focal_loss(np.zeros((1, 2), np.int32), z4, mask, z4, conf, gamma=2.0, alpha=0.25)
    ln2 = math.log(2.0)
    assert r["status"] == 0 and r["num_pos"] == 1 and r["num_neg"] == 1 and r["loc"] == 0.0
    np.testing.assert_allclose(r["pos"], 0.25 * 0.25 * ln2, rtol=1e-15)
    np.testing.assert_allclose(r["neg"], 0.75 * 0.25 * ln2, rtol=1e-15)
    np.testing.assert_allclose(r["total"], 0.25 * ln2, rtol=1e-15)
    np.testing.assert_array_equal(r["q"], [[0.5, 0.5]])
    # alpha_t (delta - p_j) (gamma p_t q^(gamma-1) log p_t - q^gamma) with p = q = 1/2, gamma = 2: the factor is -(ln 2 + 1/2) / 2
    f = 2.0 * 0.5 * 0.5 * -ln2 - 0.25
    np.testing.assert_allclose(r["dcls"][0, 0], 0.25 * f * np.array([0.5, -0.5]), rtol=1e-15)
    np.testing.assert_allclose(r["dcls"][0, 1], 0.75 * f * np.array([-0.5, 0.5]), rtol=1e-15)


def test_oracle_gamma_zero_is_cross_entropy_over_all_anchors():
    gt_cls, gt_loc, mask, loc, conf = small_case()
    r = F.softmax_focal_loss(gt_cls, gt_loc, mask, loc, conf, gamma=0.0, alpha=-1.0, grad_scale=0.5)
    B, A, C = conf.shape
    t = np.where(mask, gt_cls, C - 1)
    lse = np.log(np.exp(conf).sum(-1))
    ce = lse - np.take_along_axis(conf, t[..., None], -1)[..., 0]
    P = mask.sum()
    np.testing.assert_allclose(r["pos"], ce[mask].sum() / P, rtol=1e-13)
    np.testing.assert_allclose(r["neg"], ce[~mask].sum() / P, rtol=1e-13)
    soft = np.exp(conf - lse[..., None])
    onehot = np.eye(C)[t]
    np.testing.assert_allclose(r["dcls"], 0.5 / P * (soft - onehot), rtol=1e-12, atol=1e-16)
    d = loc - gt_loc
    np.testing.assert_allclose(r["dbox"], 0.5 / P * mask[..., None] * np.clip(d, -1, 1), rtol=1e-15)


def test_oracle_status_values():
    gt_cls, gt_loc, mask, loc, conf = small_case()
    r = F.softmax_focal_loss(gt_cls, gt_loc, np.zeros_like(mask), loc, conf)
    assert r["status"] == 1 and r["total"] == 0.0 and r["num_pos"] == 0 and r["num_neg"] == conf.shape[0] * conf.shape[1]
    assert not r["dcls"].any() and not r["dbox"].any()
    bad = conf.copy()
    bad[1, 3, 2] = np.nan
    assert F.softmax_focal_loss(gt_cls, gt_loc, mask, loc, bad)["status"] == 3
    assert F.softmax_focal_loss(gt_cls, gt_loc, np.zeros_like(mask), loc, bad)["status"] == 3      # reported first
    badloc = loc.copy()
    badloc[0, 0, 1] = np.inf                                              # anchor (0, 0) is a positive
    assert F.softmax_focal_loss(gt_cls, gt_loc, mask, badloc, conf)["status"] == 3
    a = int(np.flatnonzero(~mask[0])[0])
    okloc = loc.copy()
    okloc[0, a, 1] = np.inf                                               # ... an offset nobody reads
    assert F.softmax_focal_loss(gt_cls, gt_loc, mask, okloc, conf)["status"] == 0
    # a saturated row: q == 0 exactly, FL and the gradient row are 0 and finite for every gamma
    sat = conf.copy()
    sat[0, 0] = -800.0
    sat[0, 0, gt_cls[0, 0]] = 800.0
    for gamma in (0.0, 0.5, 1.0, 2.0):
        r = F.softmax_focal_loss(gt_cls, gt_loc, mask, loc, sat, gamma=gamma)
        assert r["q"][0, 0] == 0.0 and not r["dcls"][0, 0].any() and np.isfinite(r["total"])


@pytest.mark.parametrize("gamma,alpha", [(2.0, 0.25), (0.5, -1.0), (0.0, 0.5), (3.0, 0.75)])
def test_oracle_gradients_equal_central_differences(gamma, alpha):
    """d total / d conf and d total / d loc by central differences (h = 1e-5) on 50 sampled elements against dcls / dbox:
    relative error <= 1e-6.  Sampled where |gradient| >= 1e-3 of the largest and, for loc, away from smooth L1's kinks."""
    gt_cls, gt_loc, mask, loc, conf = small_case()
    lw, gs, h = 0.5, 2.0, 1e-5
    ref = F.softmax_focal_loss(gt_cls, gt_loc, mask, loc, conf, gamma, alpha, lw, gs)
    rng = np.random.default_rng(9)

    def total(c, l):
        return gs * F.softmax_focal_loss(gt_cls, gt_loc, mask, l, c, gamma, alpha, lw, 1.0)["total"]

    worst = 0.0
    for name, arr, grad, count in (("conf", conf, ref["dcls"], 35), ("loc", loc, ref["dbox"], 15)):
        ok = np.abs(grad) >= 1e-3 * np.abs(grad).max()
        if name == "loc":
            ok &= np.abs(np.abs(loc - gt_loc) - 1.0) > 1e-3
        picks = rng.choice(np.flatnonzero(ok.reshape(-1)), count, replace=False)
        for i in picks:
            lo, hi = arr.copy(), arr.copy()
            lo.reshape(-1)[i] -= h
            hi.reshape(-1)[i] += h
            fd = (total(hi, loc) - total(lo, loc)) / (2 * h) if name == "conf" else (total(conf, hi) - total(conf, lo)) / (2 * h)
            g = grad.reshape(-1)[i]
            worst = max(worst, abs(fd - g) / abs(g))
    assert worst <= 1e-6, worst


# ---------------------------------------------------------------------------------------------------- the GPU test's rows
def _designed(C):
    c = K.make_case(*[s for s in K.SHAPES if s[2] == C][0])
    B, A = c["B"], c["A"]
    mask = c["gt_mask"].astype(bool)
    t = np.where(mask, c["gt_cls"], C - 1).reshape(-1).astype(np.int64)
    return c, c["conf"].reshape(-1, C), t


@pytest.mark.parametrize("C", [3, 21, 81])
@pytest.mark.parametrize("gamma", [0.5, 2.0, 3.0])
def test_float32_stable_form_meets_the_bound_and_the_naive_forms_do_not(C, gamma):
    """On the GPU test's inputs a plain float32 numpy evaluation of the stable form is inside the GPU test's elementwise bound
    on every row; with q = 1 - p_t, or with log p_t = z_t - lse, the confident-correct rows ("above") are outside it."""
    c, z, t = _designed(C)
    _, ref, q = F.rows(z, t, gamma, 0.25)
    bound = K.dconf_bound(ref)
    _, got, _ = F.rows(z, t, gamma, 0.25, np.float32, "stable")
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    print("C", C, "gamma", gamma, "stable f32: worst error / bound", ratio.max())
    assert ratio.max() <= 1.0
    above = list(c["designed"]["above"])                                 # rows of image 0: flat index == anchor index
    assert q[above].max() < 1e-3
    for variant in ("one_minus_pt", "lse"):
        _, naive, _ = F.rows(z, t, gamma, 0.25, np.float32, variant)
        r = (np.abs(naive.astype(np.float64) - ref) / bound)[above]
        print("C", C, "gamma", gamma, variant, "worst error / bound on the confident-correct rows", r.max())
        assert r.max() > 1.0, variant


@pytest.mark.parametrize("C", K.EXTREME_CLASSES)
def test_float32_stable_form_meets_the_bound_on_the_extreme_rows(C):
    """Logit gaps of 30 .. 120 (K.extreme_case): a plain float32 evaluation of the stable form stays finite and inside the GPU
    test's bound, 1e-4 |ref| + 2^-100 on the gradient and the same form on FL, for every gamma (0 and the bound 8 included) and
    every alpha (0 and 1: one side's weight exactly zero).  In float32 the rows hold q == 0 exactly (the h = 1 branch) and
    p_t == 0 exactly (q == 1)."""
    c = K.extreme_case(C)
    z = c["conf"].reshape(-1, C)
    mask = c["gt_mask"].astype(bool).reshape(-1)
    t = np.where(mask, c["gt_cls"].reshape(-1), C - 1).astype(np.int64)
    idx = np.arange(z.shape[0])
    for a, gap, side, positive in c["rows"]:
        rest = np.delete(z[a], t[a])
        assert bool(mask[a]) == positive and np.abs(rest).max() <= 4.0
        assert (z[a, t[a]] - rest.max() == gap) if side == "above" else (rest.min() - z[a, t[a]] == gap)
    e32 = np.exp(z - z.max(1, keepdims=True))                            # float32
    pt32 = e32[idx, t] / e32.sum(1, dtype=np.float32)
    worst = 0.0
    for gamma in K.EXTREME_GAMMAS:
        for alpha in K.EXTREME_ALPHAS:
            fl, ref, _ = F.rows(z, t, gamma, alpha)
            with np.errstate(all="raise", under="ignore"):                # no overflow, no invalid operation, no division by zero
                fl32, got, q32 = F.rows(z, t, gamma, alpha, np.float32)
            assert np.isfinite(fl32).all() and np.isfinite(got).all() and np.isfinite(ref).all()
            assert (q32 == 0).any() and (pt32 == 0).any() and (q32[pt32 == 0] == 1).all()
            r = max(float((np.abs(got.astype(np.float64) - ref) / K.dconf_bound(ref)).max()),
                    float((np.abs(fl32.astype(np.float64) - fl) / K.dconf_bound(fl)).max()))
            worst = max(worst, r)
            assert r <= 1.0, (gamma, alpha, r)
            if alpha in (0.0, 1.0):                                       # the zero-weight side: exact zeros in both evaluations
                side = mask if alpha == 0.0 else ~mask
                assert not got[side].any() and not ref[side].any() and not fl32[side].any()
    print("C", C, "extreme rows, stable f32: worst error / bound", worst)


def test_cases_hold_the_designed_rows():
    for shape in K.SHAPES:
        for bf16 in (False, True):
            c = K.make_case(*shape, bf16=bf16)
            B, A, C = shape
            mask = c["gt_mask"].astype(bool)
            assert np.abs(c["conf"]).max() <= 16.0 and mask[0].any() and (B == 1 or not mask[B - 1].any())
            for name, (p, n) in c["designed"].items():
                assert mask[0, p] and not mask[0, n]
                for a, t in ((p, int(c["gt_cls"][0, p])), (n, C - 1)):
                    z = c["conf"][0, a]
                    rest = np.delete(z, t)
                    if name == "above":
                        assert z[t] - rest.max() >= 11.9
                    elif name == "below":
                        assert rest.min() - z[t] >= 11.9
                    elif name == "equal":
                        assert (z == z[0]).all()
                    else:
                        assert z[t] == z.max() and (z == z.max()).sum() >= 2
            assert (c["gt_cls"][~mask] >= C).all()                       # garbage where the mask is off


# ---------------------------------------------------------------------------------------------------- configuration
def test_loss_spec_and_train_config():
    from ssd_object_detection_amd import ops, optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    assert ops.LossSpec.KINDS == ("reference", "multibox", "softmax_focal")
    s = ops.LossSpec("softmax_focal")
    assert (s.kind, s.gamma, s.alpha, s.loc_weight) == ("softmax_focal", 2.0, 0.25, 1.0)
    s = ops.LossSpec("softmax_focal", gamma=0, alpha=-1, loc_weight=0.5)
    assert (s.gamma, s.alpha, s.loc_weight) == (0.0, -1.0, 0.5) and isinstance(s.gamma, float)
    assert ops.LossSpec("softmax_focal", gamma=8, alpha=1).gamma == 8.0 and ops.LossSpec("softmax_focal", alpha=0).alpha == 0.0
    assert ops.LossSpec.of("softmax_focal").kind == "softmax_focal" and ops.LossSpec.of(s) is s
    assert "gamma=0.0" in repr(s) and "alpha=-1.0" in repr(s)
    # the existing kinds: positional fields, defaults and repr as they were
    m = ops.LossSpec("multibox", 2, 0.5)
    assert (m.neg_pos_ratio, m.loc_weight, m.gamma, m.alpha) == (2, 0.5, 2.0, 0.25)
    assert repr(m) == "LossSpec(kind='multibox', neg_pos_ratio=2, loc_weight=0.5)"
    assert repr(ops.LossSpec()) == "LossSpec(kind='reference', neg_pos_ratio=3, loc_weight=1.0)"
    for bad in (dict(kind="focal"), dict(gamma=-1), dict(gamma=9), dict(gamma=float("nan")), dict(gamma=float("inf")),
                dict(gamma=True), dict(gamma="2"), dict(gamma=None), dict(alpha=1.5), dict(alpha=-0.5), dict(alpha=float("nan")),
                dict(alpha=True), dict(alpha="0.25"), dict(loc_weight=-1.0), dict(loc_weight=True)):
        with pytest.raises(ValueError):
            ops.LossSpec(**dict(dict(kind="softmax_focal"), **bad))
    opt = optimizers.Adam(optimizers.ExponentialDecay(1e-3, 100, 0.99))
    TC = SSDObjectDetectionModel.TrainConfig
    assert TC(1, 4, opt, loss="softmax_focal").loss.kind == "softmax_focal"
    assert TC(1, 4, opt, loss=s).loss is s
    with pytest.raises(ValueError):
        TC(1, 4, opt, loss="focal")


def test_loss_from_config():
    from ssd_object_detection_amd.tools.train import background_prior_from_config, loss_from_config, load_config

    def cfg(section):
        return {"model": {"train": {"loss": section}}}

    s = loss_from_config(cfg({"kind": "softmax_focal"}))
    assert (s.kind, s.gamma, s.alpha, s.loc_weight) == ("softmax_focal", 2.0, 0.25, 1.0)
    full = {"kind": "softmax_focal", "gamma": 1.5, "alpha": -1, "loc_weight": 0.5, "background_prior": 0.01}
    s = loss_from_config(cfg(full))
    assert (s.kind, s.gamma, s.alpha, s.loc_weight) == ("softmax_focal", 1.5, -1.0, 0.5)
    assert background_prior_from_config(cfg(full)) == 0.01
    assert background_prior_from_config(cfg({"kind": "softmax_focal"})) is None
    assert background_prior_from_config({}) is None and background_prior_from_config(cfg({"kind": "multibox"})) is None
    for bad in ({"kind": "softmax_focal", "neg_pos_ratio": 3}, {"kind": "softmax_focal", "gamma": 9}, {"kind": "softmax_focal", "alpha": 2},
                {"kind": "softmax_focal", "beta": 1}, {"kind": "focal"}, {"kind": "multibox", "gamma": 2.0}, {"kind": "multibox", "alpha": 0.25},
                {"kind": "multibox", "background_prior": 0.01}, {"kind": "reference", "gamma": 2.0}, {"gamma": 2.0},
                {"background_prior": 0.01}):
        with pytest.raises(ValueError):
            loss_from_config(cfg(bad))
    for bad in (0, 1, 1.5, -0.01, True, "0.01", float("nan")):
        with pytest.raises(ValueError):
            background_prior_from_config(cfg({"kind": "softmax_focal", "background_prior": bad}))
    with pytest.raises(ValueError):
        background_prior_from_config(cfg({"kind": "multibox", "background_prior": 0.01}))
    # the shipped configuration stays on the reference's loss; its commented-out example names the new kind and its keys
    path = os.path.join(ROOT, "ssd-object-detection_amd", "config", "default.yml")
    assert loss_from_config(load_config(path)) is None and background_prior_from_config(load_config(path)) is None
    text = open(path).read()
    for key in ("kind: softmax_focal", "gamma:", "alpha:", "background_prior:"):
        assert re.search(r"#\s*%s" % re.escape(key), text), key


def test_background_prior_refuses_bad_values_without_a_device():
    from ssd_object_detection_amd.engine import SSDEngine
    eng = SSDEngine.planned()
    for bad in (0, 1, 0.0, 1.0, -0.1, 1.5, True, "0.01", None, float("nan")):
        with pytest.raises(ValueError):
            eng.set_background_prior(bad)


# ---------------------------------------------------------------------------------------------------- the library
def test_entries_are_declared_and_refuse_on_the_host():
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    names = ("ssd_softmax_focal_loss_workspace_bytes", "ssd_softmax_focal_loss_fwd_bwd",
             "ssd_softmax_focal_loss_heads_workspace_bytes", "ssd_softmax_focal_loss_fwd_bwd_heads")
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib._SIGNATURES and hasattr(L, n), n
    need = L.ssd_softmax_focal_loss_workspace_bytes(2, 8732, 81)
    assert need > 0 and L.ssd_softmax_focal_loss_workspace_bytes(0, 8732, 81) == 0
    assert L.ssd_softmax_focal_loss_heads_workspace_bytes(2, 8732, 81) >= need
    assert L.ssd_softmax_focal_loss_workspace_bytes(64, 100000, 81) > 0           # no anchor bound
    d = ctypes.c_void_p(0x1000)                                         # never dereferenced on these paths
    V, U, W = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED, _lib.SSD_ERR_WORKSPACE

    def dense(dtype=0, B=2, A=8732, C=81, gamma=2.0, alpha=0.25, lw=1.0, gs=1.0, ws=d, ws_bytes=1 << 40, conf=d, dconf=d):
        return L.ssd_softmax_focal_loss_fwd_bwd(conf, d, dtype, d, d, d, B, A, C, gamma, alpha, lw, gs, d, dconf, d, ws, ws_bytes,
                                                None)

    for gamma in (-1.0, 9.0, float("nan"), float("inf")):
        assert dense(gamma=gamma) == V, gamma
    for alpha in (1.5, -0.5, float("nan"), -2.0):
        assert dense(alpha=alpha) == V, alpha
    assert dense(lw=-1.0) == V and dense(lw=float("inf")) == V and dense(gs=float("nan")) == V
    assert dense(dtype=2) == V and dense(conf=None) == V and dense(dconf=None) == V
    assert dense(B=0) == V and dense(A=0) == V and dense(C=1) == V
    assert dense(C=304) == U
    assert dense(gamma=9.0, C=304) == V                                 # a bad value is reported before the class bound
    assert dense(ws=None) == W and dense(ws_bytes=need - 1) == W

    hg = _lib.HeadGrads()
    hg.levels = 2
    for l, (hw, n) in enumerate(((1444, 4), (361, 6))):
        hg.hw[l], hg.per_cell[l], hg.npad[l] = hw, n, (n * 85 + 7) // 8 * 8
        hg.rows[l], hg.row_of_pixel[l], hg.pixel_of_row[l] = 0x1000, 0x1000, 0x1000
    hg.count = 0x1000
    A2 = 1444 * 4 + 361 * 6

    def heads(dtype=1, A=A2, gamma=2.0, alpha=0.25, ws_bytes=1 << 40, hgp=ctypes.byref(hg)):
        return L.ssd_softmax_focal_loss_fwd_bwd_heads(d, d, dtype, d, d, d, 2, A, 81, gamma, alpha, 1.0, 1.0, d, hgp, d, ws_bytes,
                                                      None)

    assert heads(dtype=0) == U and heads(dtype=5) == V                   # the rows form is bf16 only
    assert heads(hgp=None) == V
    assert heads(A=A2 + 1) == _lib.SSD_ERR_ASSERT and heads(A=A2 - 6) == _lib.SSD_ERR_ASSERT     # levels do not sum to A
    assert heads(gamma=-1.0) == V and heads(alpha=1.5) == V
    assert heads(ws_bytes=16) == W
    hg.npad[1] = 6 * 85                                                 # not a multiple of 8
    assert heads() == V
