"""CPU suite for the opt-in MultiBox loss: the float64 oracle against torch.autograd and against ssd.pytorch's selection rule,
the configuration plumbing, and the host-side refusals of the new entry points (no launch: callable without a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import multibox_oracle as M

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_case(B, A, C, P_b, seed):
    rng = np.random.default_rng(seed)
    conf = 3.0 * rng.standard_normal((B, A, C))
    conf[..., -1] += 2.0
    loc = 1.5 * rng.standard_normal((B, A, 4))
    gt_loc = rng.standard_normal((B, A, 4))
    mask = np.zeros((B, A), dtype=bool)
    for b, p in enumerate(P_b):
        mask[b, rng.choice(A, p, replace=False)] = True
    gt_cls = rng.integers(0, C - 1, (B, A)).astype(np.int32)
    return gt_cls, gt_loc, mask, loc, conf


@pytest.mark.parametrize("ratio,alpha,gs", [(3, 1.0, 1.0), (1, 0.5, 0.25)])
def test_oracle_gradients_equal_autograd(ratio, alpha, gs):
    """dcls / dbox are what torch.autograd returns, in float64, for F.cross_entropy and F.smooth_l1_loss(beta=1) summed over
    the oracle's own masks and divided by P."""
    import torch.nn.functional as F
    gt_cls, gt_loc, mask, loc, conf = random_case(3, 157, 11, (4, 0, 30), 1)
    loc[0, np.flatnonzero(mask[0])[0], :3] = gt_loc[0, np.flatnonzero(mask[0])[0], :3] + np.array([0.0, 0.999, -1.001])
    ref = M.multibox_loss(gt_cls, gt_loc, mask, loc, conf, ratio, alpha, gs)
    tconf = torch.tensor(conf, dtype=torch.float64, requires_grad=True)
    tloc = torch.tensor(loc, dtype=torch.float64, requires_grad=True)
    pos, neg = torch.from_numpy(mask), torch.from_numpy(ref["neg_mask"])
    P = int(mask.sum())
    lab = torch.from_numpy(gt_cls.astype(np.int64))
    l_pos = F.cross_entropy(tconf[pos], lab[pos], reduction="sum") / P
    l_neg = F.cross_entropy(tconf[neg], torch.full((int(neg.sum()),), conf.shape[-1] - 1), reduction="sum") / P
    l_loc = alpha * F.smooth_l1_loss(tloc[pos], torch.from_numpy(gt_loc)[pos], reduction="sum", beta=1.0) / P
    total = l_loc + l_pos + l_neg
    (gs * total).backward()
    for name, want in (("loc", l_loc), ("pos", l_pos), ("neg", l_neg), ("total", total)):
        assert abs(ref[name] - want.item()) <= 1e-12 * max(1.0, abs(want.item())), name
    assert np.abs(ref["dcls"] - tconf.grad.numpy()).max() <= 1e-12
    assert np.abs(ref["dbox"] - tloc.grad.numpy()).max() <= 1e-12
    assert ref["num_pos"] == P and ref["num_neg"] == int(neg.sum())


def ssd_pytorch_selection(key, mask, ratio):
    """ssd.pytorch MultiBoxLoss, literally: the positives' loss zeroed, a descending sort, the rank of every anchor by a second
    sort, neg = rank < num_neg with num_neg clamped to the candidates of the image."""
    loss_c = np.where(mask, 0.0, key)
    loss_idx = np.argsort(-loss_c, axis=1, kind="stable")
    idx_rank = np.argsort(loss_idx, axis=1, kind="stable")
    num_pos = mask.sum(1, keepdims=True)
    num_neg = np.minimum(ratio * num_pos, mask.shape[1] - num_pos)
    return idx_rank < num_neg


@pytest.mark.parametrize("ratio", [1, 3])
def test_oracle_selection_is_ssd_pytorch_rule_without_ties(ratio):
    gt_cls, gt_loc, mask, loc, conf = random_case(4, 300, 21, (0, 5, 40, 120), 2)
    key = M.keys(conf)
    assert np.unique(key).size == key.size and (key > 0).all()        # no ties; a positive's zeroed loss ranks below all
    tau, neg = M.select(key, mask, ratio)
    want = ssd_pytorch_selection(key, mask, ratio)
    assert np.array_equal(neg, want)
    # where ratio * P_b <= A - P_b the literal rule never reaches a positive; image 3 at ratio 3 (360 > 180) takes every candidate
    assert np.array_equal(neg.sum(1), np.minimum(ratio * mask.sum(1), 300 - mask.sum(1)))


def test_oracle_edge_images():
    gt_cls, gt_loc, mask, loc, conf = random_case(3, 64, 5, (0, 20, 3), 3)
    ref = M.multibox_loss(gt_cls, gt_loc, mask, loc, conf)
    assert np.isnan(ref["tau"][0]) and not ref["neg_mask"][0].any()            # P_b = 0 mines nothing
    assert ref["neg_mask"][1].sum() == 44 and ref["tau"][1] == ref["key"][1][~mask[1]].min()   # 60 > 44: every candidate
    assert ref["neg_mask"][2].sum() == 9
    assert not (ref["neg_mask"] & mask).any()
    assert (ref["dcls"][0] == 0).all() and (ref["dbox"][0] == 0).all()
    # all keys equal: ties are kept, every candidate of an image with a positive is selected
    conf0 = np.zeros_like(conf)
    ref = M.multibox_loss(gt_cls, gt_loc, mask, loc, conf0)
    assert np.array_equal(ref["neg_mask"].sum(1), [0, 44, 61])
    np.testing.assert_allclose(ref["pos"], np.log(5.0), rtol=1e-14)
    np.testing.assert_allclose(ref["neg"], 105 * np.log(5.0) / 23, rtol=1e-14)
    # no positive at all: status 1, zeros
    ref = M.multibox_loss(gt_cls, gt_loc, np.zeros_like(mask), loc, conf)
    assert ref["status"] == 1 and ref["total"] == 0.0 and ref["num_neg"] == 0 and not ref["dcls"].any()


def test_loss_spec_and_train_config():
    from ssd_object_detection_amd import ops, optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    s = ops.LossSpec()
    assert (s.kind, s.neg_pos_ratio, s.loc_weight) == ("reference", 3, 1.0)
    s = ops.LossSpec("multibox", 2, 0.5)
    assert (s.kind, s.neg_pos_ratio, s.loc_weight) == ("multibox", 2, 0.5)
    assert ops.LossSpec.of(None).kind == "reference" and ops.LossSpec.of("multibox").kind == "multibox"
    assert ops.LossSpec.of(s) is s
    for bad in (dict(kind="focal"), dict(kind=None), dict(neg_pos_ratio=0), dict(neg_pos_ratio=2.5), dict(neg_pos_ratio=True),
                dict(loc_weight=-1.0), dict(loc_weight=float("nan")), dict(loc_weight=float("inf")), dict(loc_weight="1")):
        with pytest.raises(ValueError):
            ops.LossSpec(**bad)
    with pytest.raises(ValueError):
        ops.LossSpec.of(3)
    opt = optimizers.Adam(optimizers.ExponentialDecay(1e-3, 100, 0.99))
    TC = SSDObjectDetectionModel.TrainConfig
    assert TC(1, 4, opt).loss.kind == "reference"
    assert TC(1, 4, opt, loss="reference").loss.kind == "reference"
    assert TC(1, 4, opt, loss="multibox").loss.kind == "multibox"
    assert TC(1, 4, opt, loss=s).loss is s
    with pytest.raises(ValueError):
        TC(1, 4, opt, loss="hinge")
    with pytest.raises(ValueError):
        TC(1, 4, opt, loss={"kind": "multibox"})


def test_loss_from_config():
    from ssd_object_detection_amd.tools.train import loss_from_config, load_config
    assert loss_from_config({}) is None
    assert loss_from_config({"model": {"train": {"epoch": 1}}}) is None
    s = loss_from_config({"model": {"train": {"loss": {"kind": "multibox"}}}})
    assert (s.kind, s.neg_pos_ratio, s.loc_weight) == ("multibox", 3, 1.0)
    s = loss_from_config({"model": {"train": {"loss": {"kind": "multibox", "neg_pos_ratio": 1, "loc_weight": 0.5}}}})
    assert (s.kind, s.neg_pos_ratio, s.loc_weight) == ("multibox", 1, 0.5)
    assert loss_from_config({"model": {"train": {"loss": {"kind": "reference"}}}}).kind == "reference"
    assert loss_from_config({"model": {"train": {"loss": {}}}}).kind == "reference"
    for bad in ({"kind": "multibox", "ratio": 3}, {"kind": "smooth"}, {"kind": "multibox", "neg_pos_ratio": 0},
                {"kind": "multibox", "loc_weight": -0.5}, "multibox"):
        with pytest.raises(ValueError):
            loss_from_config({"model": {"train": {"loss": bad}}})
    # the shipped configuration trains with the reference's loss; its commented-out example names the section
    path = os.path.join(ROOT, "ssd-object-detection_amd", "config", "default.yml")
    assert loss_from_config(load_config(path)) is None
    assert re.search(r"#\s*loss:", open(path).read())


def test_multibox_entries_are_declared_and_refuse_on_the_host():
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    names = ("ssd_multibox_loss_max_anchors", "ssd_multibox_loss_workspace_bytes", "ssd_multibox_loss_fwd_bwd",
             "ssd_multibox_loss_heads_workspace_bytes", "ssd_multibox_loss_fwd_bwd_heads")
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib._SIGNATURES and hasattr(L, n), n
    amax = L.ssd_multibox_loss_max_anchors()
    assert amax >= 24564
    assert re.search(r"#define\s+SSD_MULTIBOX_MAX_ANCHORS\s+%d\b" % amax, header)
    need = L.ssd_multibox_loss_workspace_bytes(2, 8732, 81)
    assert need >= 2 * 8732 * 8 and L.ssd_multibox_loss_workspace_bytes(0, 8732, 81) == 0
    assert L.ssd_multibox_loss_heads_workspace_bytes(2, 8732, 81) >= need
    d = ctypes.c_void_p(0x1000)                                         # never dereferenced on these paths

    def dense(dtype=0, B=2, A=8732, C=81, ratio=3, alpha=1.0, gs=1.0, ws=d, ws_bytes=1 << 40, conf=d):
        return L.ssd_multibox_loss_fwd_bwd(conf, d, dtype, d, d, d, B, A, C, ratio, alpha, gs, d, d, d, ws, ws_bytes, None)

    assert dense(dtype=2) == _lib.SSD_ERR_VALUE
    assert dense(conf=None) == _lib.SSD_ERR_VALUE
    assert dense(B=0) == _lib.SSD_ERR_VALUE and dense(C=1) == _lib.SSD_ERR_VALUE
    assert dense(C=304) == _lib.SSD_ERR_UNSUPPORTED
    assert dense(A=amax + 1) == _lib.SSD_ERR_UNSUPPORTED
    assert dense(ratio=0) == _lib.SSD_ERR_VALUE
    assert dense(alpha=-1.0) == _lib.SSD_ERR_VALUE
    assert dense(alpha=float("nan")) == _lib.SSD_ERR_VALUE and dense(alpha=float("inf")) == _lib.SSD_ERR_VALUE
    assert dense(ws=None) == _lib.SSD_ERR_WORKSPACE and dense(ws_bytes=need - 1) == _lib.SSD_ERR_WORKSPACE

    hg = _lib.HeadGrads()
    hg.levels = 2
    for l, (hw, n) in enumerate(((1444, 4), (361, 6))):
        hg.hw[l], hg.per_cell[l], hg.npad[l] = hw, n, (n * 85 + 7) // 8 * 8
        hg.rows[l], hg.row_of_pixel[l], hg.pixel_of_row[l] = 0x1000, 0x1000, 0x1000
    hg.count = 0x1000
    A2 = 1444 * 4 + 361 * 6

    def heads(dtype=1, A=A2, ratio=3, alpha=1.0, ws_bytes=1 << 40, hgp=ctypes.byref(hg)):
        return L.ssd_multibox_loss_fwd_bwd_heads(d, d, dtype, d, d, d, 2, A, 81, ratio, alpha, 1.0, d, hgp, d, ws_bytes, None)

    assert heads(dtype=0) == _lib.SSD_ERR_UNSUPPORTED and heads(dtype=5) == _lib.SSD_ERR_VALUE
    assert heads(hgp=None) == _lib.SSD_ERR_VALUE
    assert heads(A=A2 + 1) == _lib.SSD_ERR_ASSERT and heads(A=A2 - 6) == _lib.SSD_ERR_ASSERT     # levels do not sum to A
    assert heads(ratio=-3) == _lib.SSD_ERR_VALUE and heads(alpha=float("nan")) == _lib.SSD_ERR_VALUE
    assert heads(A=amax + 1) == _lib.SSD_ERR_UNSUPPORTED
    assert heads(ws_bytes=16) == _lib.SSD_ERR_WORKSPACE
    hg.npad[1] = 6 * 85                                                 # not a multiple of 8
    assert heads() == _lib.SSD_ERR_VALUE


def test_exact_cases_are_in_their_regime():
    """tests/multibox_cases.py asserts, while it builds a case, that the float64 oracle's results are exact and convert to the
    output dtype without rounding; the designed ranks, ties and counts are asserted there too"""
    from tests import multibox_cases as K
    r = K.ranks_case()
    assert r["P"] == 32 and r["N"] == 102 and r["status"] == 0
    for dt in (torch.float32, torch.bfloat16):
        r = K.boundary_case(dt)
        assert r["P"] == 8 and list(r["N_b"]) == [16, 13]
        assert K.saturated_case(dt)["out8"][6] == 0.0
        r = K.empty_case(dt)
        assert r["status"] == 1 and not r["dconf"].any() and not r["out8"][:7].any()
    for name in ("GEOM1 B=3 C=21", "GEOM7 B=3 C=81", "GEOM8 B=1 C=21", "SSD300 B=2 C=81"):
        r = K.cached(name, K.HEADS_CASES[name])
        assert sum(l["count"] for l in r["levels"]) > 0
