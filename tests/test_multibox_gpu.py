"""GPU: the opt-in MultiBox loss (ssd_multibox_loss_fwd_bwd / _heads) against the float64 oracle tests/multibox_oracle.py.
Targets are hand-made masks, so that the positives per image P_b are chosen.  Tolerances: the ones tests/test_loss_gpu.py uses
for this kernel family -- scalars 1e-4 relative; dconf within 2e-5 of its largest magnitude (+ 4e-3 of it for bf16); dloc within
1e-6 (f32) / 4e-3 (bf16) of its largest magnitude; P exact; the selection per image: a row may differ from the oracle's only if
its float64 key lies within 1e-5 * max(1, tau_b) of the float64 tau_b, at most 2 rows per image."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import multibox_cases as K                                # noqa: E402
from tests import strict                                             # noqa: E402

F32, BF = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def dev(r):
    return [r[k].cuda() for k in ("conf", "loc", "gt_cls", "gt_loc", "gt_mask")]


def check_against_oracle(ops, r, ratio=3, alpha=1.0, gs=1.0):
    conf, loc, cls, gloc, mask = dev(r)
    out, dconf, dloc = ops.multibox_loss(conf, loc, cls, gloc, mask, ratio, alpha, gs)
    out = out.cpu().numpy()
    ref = K.oracle_of(r, ratio, alpha, gs)
    B, A = r["B"], r["A"]
    pos = r["gt_mask"].numpy().astype(bool)
    print("out8", out.tolist(), "oracle", [ref[k] for k in ("loc", "pos", "neg", "total", "num_pos", "num_neg")])
    assert out[7] == 0.0
    assert int(out[4]) == ref["num_pos"]
    d = dconf.float().cpu().numpy().astype(np.float64)
    rows_got = (np.abs(d).sum(-1) > 0) & ~pos                          # a mined row carries a gradient (softmax < 1 at the background)
    flips = rows_got != ref["neg_mask"]
    for b in range(B):
        n_flip = int(flips[b].sum())
        if n_flip:
            tau_b = ref["tau"][b]
            assert not np.isnan(tau_b) and n_flip <= 2, (b, n_flip)
            assert (np.abs(ref["key"][b][flips[b]] - tau_b) <= 1e-5 * max(1.0, tau_b)).all(), (b, ref["key"][b][flips[b]], tau_b)
        else:
            assert int(rows_got[b].sum()) == int(ref["neg_mask"][b].sum()), b
    assert int(out[5]) == int(rows_got.sum())
    for i, key in enumerate(["loc", "pos", "neg", "total"]):
        assert abs(out[i] - ref[key]) <= 1e-4 * abs(ref[key]), (key, out[i], ref[key])
    mined = ~np.isnan(ref["tau"])
    tau_min = ref["tau"][mined].min() if mined.any() else 0.0
    assert abs(out[6] - tau_min) <= 1e-5 * max(1.0, tau_min)
    same = ~flips
    scale = np.abs(ref["dcls"]).max()
    err = np.abs(d[same] - ref["dcls"][same]).max()
    print("dconf err / scale", err / scale, "flips", int(flips.sum()))
    assert err <= 2e-5 * scale + (0 if r["dtype"] == F32 else 4e-3 * scale)
    dl = dloc.float().cpu().numpy().astype(np.float64)
    lscale = np.abs(ref["dbox"]).max()
    print("dloc err / scale", np.abs(dl - ref["dbox"]).max() / lscale)
    print("error / bound: scalars", max(abs(out[i] - ref[k]) / max(1e-4 * abs(ref[k]), 1e-300) for i, k in enumerate(["loc", "pos", "neg", "total"])),
          "dconf", err / (2e-5 * scale + (0 if r["dtype"] == F32 else 4e-3 * scale)),
          "dloc", np.abs(dl - ref["dbox"]).max() / ((1e-6 if r["dtype"] == F32 else 4e-3) * lscale))
    assert np.abs(dl - ref["dbox"]).max() <= (1e-6 if r["dtype"] == F32 else 4e-3) * lscale
    assert not dl[~pos].any() and not d[~pos & ~rows_got].any()        # exact zeros everywhere else
    return out, ref


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_against_oracle_ssd300(ops, dtype, seed):
    """B=5, A=8732, C=81, P_b = (0, 7, 60, 400, 2500): an image without positives, and one whose 3 P_b exceeds its candidates"""
    r = K.hand_case(5, 8732, 81, (0, 7, 60, 400, 2500), seed, dtype)
    out, ref = check_against_oracle(ops, r)
    assert list(ref["neg_mask"].sum(1)) == [0, 21, 180, 1200, 6232]


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [2, 21, 81, 288])
def test_small_awkward_shapes(ops, C, dtype):
    """B=3, A=200: 128-row blocks straddle the images, the last block is ragged; both instances of the row pass (C = 81 and any
    other); offsets on both sides of |d| = 1, at |d| = 1 and at d = 0 exactly"""
    r = K.hand_case(3, 200, C, (5, 0, 40), 10 + C, dtype, offsets="edges")
    check_against_oracle(ops, r)


@pytest.mark.parametrize("ratio,alpha,gs", [(1, 1.0, 1.0), (3, 0.5, 0.25), (1, 0.5, 0.25)])
@pytest.mark.parametrize("B", [1, 3])
def test_parameters(ops, B, ratio, alpha, gs):
    r = K.hand_case(B, 200, 21, (9, 0, 60)[:B], 20 + B, F32, offsets="edges")
    out, ref = check_against_oracle(ops, r, ratio, alpha, gs)
    assert list(ref["neg_mask"].sum(1)) == [min(ratio * p, 200 - p) for p in (9, 0, 60)[:B]]


def test_ties(ops):
    """all-zero logits: every key equals log C, ties are kept -- every candidate of images 0 and 2, none of image 1"""
    B, A, C = 3, 200, 81
    r = K.hand_case(B, A, C, (5, 0, 9), 30)
    conf = torch.zeros((B, A, C), device="cuda")
    _, loc, cls, gloc, mask = dev(r)
    out, dconf, dloc = ops.multibox_loss(conf, loc, cls, gloc, mask)
    out = out.cpu().numpy()
    P, N = 14, (A - 5) + (A - 9)
    assert int(out[4]) == P and int(out[5]) == N and out[7] == 0
    np.testing.assert_allclose(out[1], np.log(81.0), rtol=1e-6)
    np.testing.assert_allclose(out[2], N * np.log(81.0) / P, rtol=1e-6)
    np.testing.assert_allclose(out[6], np.log(81.0), rtol=1e-6)
    rows = dconf.abs().sum(-1) > 0
    assert bool(rows[0].all()) and bool(rows[2].all()) and not bool(rows[1].any())


def ssd300_buffers(ops, B, C=81):
    hw, npc = (1444, 361, 100, 25, 9, 1), (4, 6, 6, 6, 4, 4)
    return ops.HeadGradBuffers(B, hw, npc, tuple((n * (4 + C) + 7) // 8 * 8 for n in npc))


def test_resnet_ssd512_anchor_count(ops):
    """A = 24 564 (96 KB of keys in LDS), B=2, against the oracle"""
    r = K.hand_case(2, 24564, 81, (300, 1), 40, BF)
    check_against_oracle(ops, r)


def test_largest_anchor_count_runs(ops):
    """A = ssd_multibox_loss_max_anchors(): the header's bound is the code's -- 144 KB of keys beside the select's static LDS"""
    from ssd_object_detection_amd import _lib
    amax = _lib.lib().ssd_multibox_loss_max_anchors()
    out, ref = check_against_oracle(ops, K.hand_case(2, amax, 5, (50, 3), 41, F32))
    assert list(ref["neg_mask"].sum(1)) == [150, 9]


def test_anchor_bound_is_refused_with_nothing_written(ops):
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    amax = L.ssd_multibox_loss_max_anchors()
    assert amax >= 24564
    B, A, C = 1, amax + 1, 3
    a = strict.Arena("cuda", strict.Arena.bytes_for(32, B * A * C * 4, B * A * 16, 1 << 22))
    out8, dconf, dloc = a.out((8,), F32, "out8"), a.out((B, A, C), F32, "dconf"), a.out((B, A, 4), F32, "dloc")
    ws = a.out((1 << 22,), torch.uint8, "ws")
    conf = torch.zeros((B, A, C), device="cuda")
    loc = torch.zeros((B, A, 4), device="cuda")
    cls = torch.zeros((B, A), dtype=torch.int32, device="cuda")
    mask = torch.ones((B, A), dtype=torch.uint8, device="cuda")
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def fn():
        st = L.ssd_multibox_loss_fwd_bwd(p(conf), p(loc), 0, p(cls), p(loc), p(mask), B, A, C, 3, 1.0, 1.0, p(out8), p(dconf),
                                         p(dloc), p(ws), ws.numel(), None)
        assert st == _lib.SSD_ERR_UNSUPPORTED, st
    a.run(fn, [])                                                       # every output keeps its poison, every guard too
    with pytest.raises(ValueError):
        ops.multibox_loss(conf, loc, cls, loc, mask)


def test_status_codes_in_both_forms(ops):
    """P == 0: status 1, zero scalars and gradients, no rows.  A NaN / Inf logit anywhere, or a NaN offset of a positive:
    status 3 (also where P == 0 otherwise).  The same inputs give 0 when clean."""
    B, A, C = 2, 8732, 81
    r = K.hand_case(B, A, C, (30, 4), 50, BF)
    conf, loc, cls, gloc, mask = dev(r)
    hgb = ssd300_buffers(ops, B)

    def status(conf, loc, mask):
        s1 = float(ops.multibox_loss(conf, loc, cls, gloc, mask)[0][7])
        s2 = float(ops.multibox_loss_heads(conf, loc, cls, gloc, mask, hgb)[7])
        assert s1 == s2
        return s1

    assert status(conf, loc, mask) == 0.0
    none = torch.zeros_like(mask)
    out, dconf, dloc = ops.multibox_loss(conf, loc, cls, gloc, none)
    assert out.cpu().tolist() == [0, 0, 0, 0, 0, 0, 0, 1.0]
    assert not bool(dconf.view(torch.int16).any()) and not bool(dloc.view(torch.int16).any())
    hgb.count.fill_(77)
    assert ops.multibox_loss_heads(conf, loc, cls, gloc, none, hgb).cpu().tolist() == [0, 0, 0, 0, 0, 0, 0, 1.0]
    assert hgb.count[:6].cpu().tolist() == [0] * 6 and all(bool((t == -1).all()) for t in hgb.row_of_pixel)
    for where in ("logit_nan", "logit_inf", "offset_nan"):
        c2, l2 = conf.clone(), loc.clone()
        if where == "logit_nan":
            c2[1, 5000, 17] = float("nan")
        elif where == "logit_inf":
            c2[0, 8731, 80] = float("inf")
        else:
            l2[1, mask[1].nonzero()[0, 0], 2] = float("nan")
        assert status(c2, l2, mask) == 3.0, where
    c2 = conf.clone()
    c2[0, 3, 5] = float("nan")
    assert status(c2, loc, none) == 3.0                                 # reported first, as the reference loss does
    assert status(conf, loc, mask) == 0.0


def test_reproducible_workspace_free_and_sync_free(ops):
    """two calls are bitwise equal; a workspace full of 0xFF gives what a zeroed one gives (the workspace needs no initial
    contents); no call synchronises the host"""
    B, A, C = 3, 8732, 81
    r = K.hand_case(B, A, C, (100, 0, 900), 60, BF)
    conf, loc, cls, gloc, mask = dev(r)
    L = __import__("ssd_object_detection_amd._lib", fromlist=["x"]).lib()
    nbytes = max(L.ssd_multibox_loss_workspace_bytes(B, A, C), L.ssd_multibox_loss_heads_workspace_bytes(B, A, C))
    hgb = ssd300_buffers(ops, B)

    class Ws:
        def __init__(self, fill):
            self.buf = torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")

        def get(self, n, device):
            assert n <= self.buf.numel()
            return self.buf

    def rows_state():
        k = hgb.count.cpu().tolist()
        return [t[:k[i]].clone() for i, t in enumerate(hgb.rows)] + [t.clone() for t in hgb.row_of_pixel] + \
               [t[:k[i]].clone() for i, t in enumerate(hgb.pixel_of_row)] + [hgb.count.clone()]

    results = []
    for fill in (0x00, 0xFF, 0xFF):
        ws = Ws(fill)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            dense = ops.multibox_loss(conf, loc, cls, gloc, mask, ws=ws)
            ws.buf.fill_(fill)
            out_h = ops.multibox_loss_heads(conf, loc, cls, gloc, mask, hgb, ws=ws)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        results.append([dense[0].view(torch.int32), dense[1].view(torch.int16), dense[2].view(torch.int16),
                        out_h.view(torch.int32)] + rows_state())
    for other in results[1:]:
        assert len(other) == len(results[0])
        for x, y in zip(results[0], other):
            assert torch.equal(x.view(torch.uint8) if x.dtype == BF else x, y.view(torch.uint8) if y.dtype == BF else y)
    assert torch.equal(results[0][0], results[0][3])                    # both forms write the same out8
    sl, sc = hgb.dense(C)
    assert torch.equal(sl.view(torch.int16), results[0][2]) and torch.equal(sc.view(torch.int16), results[0][1])
