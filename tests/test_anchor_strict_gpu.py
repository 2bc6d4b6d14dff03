"""GPU: the anchor-side kernels (match.hip, the single-label half of detect.hip, evalmap.hip) under tests/strict.py -- every
tensor in a guarded arena, outputs and workspace poisoned twice, through the C ABI -- at the anchor counts, class counts,
box counts, ties and thresholds the other tests do not reach (tests/anchor_cases.py builds the cases from the oracles).

Bounds are the project's own: bit equality for priors, IoU, indices, classes, masks, owners, keep masks, flags and the
division terms of the encoding; <= 1 float32 ulp for its log terms (rtol 4e-16 for ssd_apply_anchor_box's float64 result);
rtol 2e-6 / atol 1e-9 for scores; rtol 3e-7 for decoded boxes; 1e-12 for AP.  Where the bound is not bit equality a plain call
is checked against the oracle with it, and the arena run must then reproduce those bits under both poisons.

Which test reaches which path:
  k_nms scalar sweep, (A & 3) != 0, and its keep clearing           test_nms[1], [3], [190], [1023], [4099]
  k_nms aligned sweep below 1024 quads (clamped load index)         test_nms[380]
  anchor 65535 in the 16-bit key; A = 65537 refused                 test_nms[65536]
  total > 1024 >= max_cand, ties across the cut, segment > 64       test_nms[4099], [65536]
  k_eval_match scalar sweep, > 48 ground truths, > 1024 kept        test_eval_match[3], [190], [4099]
  k_score_decode<T, 0>: even C, C = 2, score / class / flag / box   test_score_decode_*[2-..], [3-..], [6-..], [80-..]
  class ties within and across the half rows                        test_score_decode_random_logits_and_class_ties
  strict threshold, p_background == score                           test_score_decode_exact_threshold
  phase 1 with row state in global memory (n_t > 512)               test_match_three_launch_path[G790]
  n_t == A, A < 256, a grid of one cell                             test_match_three_launch_path[G4], [G190]
  workspace read before written, guards, unlisted outputs           every arena.run here (the match workspace: test_match_*)
  k_match_local on small grids, without a workspace                 test_match_single_launch_path"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import anchor_cases as AC                                 # noqa: E402
from tests import strict                                             # noqa: E402
from tests.test_match_gpu import check_image, ulp_diff_f32           # noqa: E402

_PSETS = {}


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def pset_of(ops, name):
    """ops.build_priors of a geometry (once), checked against the oracle's bits"""
    if name not in _PSETS:
        ps = ops.build_priors(**AC.GEOMETRIES[name])
        assert ps.A == AC.ANCHORS[name]
        assert np.array_equal(ps.priors.cpu().numpy().view(np.uint64), AC.priors(name).view(np.uint64))
        _PSETS[name] = ps
    return _PSETS[name]


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def plain(arena, fn, outs):
    """one call on freshly poisoned tensors; the outputs as numpy"""
    arena.poison(False)
    fn()
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy() for t in outs]


def ok(status):
    assert status == 0, status


# ---------------------------------------------------------------------------------------------------------- 1. priors and helpers
@pytest.mark.parametrize("geo", ["G4", "G190", "G790"])
def test_priors_and_helpers(L, geo):
    g = AC.GEOMETRIES[geo]
    pri = AC.priors(geo)
    A = len(pri)
    levels = len(g["grids"])
    hw = (ctypes.c_int * (2 * levels))(*[v for gr in g["grids"] for v in gr])
    sref = (ctypes.c_double * (levels + 1))(*[float(s) for s in g["s_ref"]])
    flat = [r for rr in g["ratios"] for r in rr]
    rat = (ctypes.c_int * len(flat))(*flat)
    roff = (ctypes.c_int * (levels + 1))(*np.concatenate([[0], np.cumsum([len(rr) for rr in g["ratios"]])]).tolist())
    assert L.ssd_priors_count(hw, levels, roff) == A
    rows = {n: AC.helper_case(geo, n) for n in (1, 257)}
    arena = strict.Arena("cuda", strict.Arena.bytes_for(*[A * 32] * 3, *[257 * 32] * 8))
    a_pri = arena.put(T(pri), "priors")
    o_pri = arena.out((A, 4), torch.float64, "priors_out")
    o_enc0 = arena.out((A, 4), torch.float32, "enc_zero")
    io = {}
    for n, r in rows.items():
        io[n] = (arena.put(T(r["box"]), "box%d" % n), arena.put(T(r["pri"]), "pri%d" % n),
                 arena.out((n,), torch.float64, "iou%d" % n), arena.out((n, 4), torch.float64, "enc%d" % n))

    def call():
        ok(L.ssd_priors(hw, levels, sref, rat, roff, float(g["in_size"]), P(o_pri), stream()))
        ok(L.ssd_encode_zero(P(a_pri), A, P(o_enc0), stream()))
        for n, (b, p, o_iou, o_enc) in io.items():
            ok(L.ssd_iou_n(P(b), P(p), n, P(o_iou), stream()))
            ok(L.ssd_apply_anchor_box(P(b), P(p), n, P(o_enc), stream()))

    got = plain(arena, call, [o_enc0] + [io[n][3] for n in rows])
    want0 = AC.enc_zero(geo)
    assert np.array_equal(got[0][:, :2].view(np.uint32), want0[:, :2].view(np.uint32))
    assert ulp_diff_f32(got[0][:, 2:], want0[:, 2:]).max() <= 1
    for enc, (n, r) in zip(got[1:], rows.items()):
        assert np.array_equal(enc[:, :2].view(np.uint64), r["enc"][:, :2].view(np.uint64)), n
        np.testing.assert_allclose(enc[:, 2:], r["enc"][:, 2:], rtol=4e-16, atol=0)
    expect = [(o_pri, T(pri)), (o_enc0, T(got[0]))]
    for enc, (n, r) in zip(got[1:], rows.items()):
        expect += [(io[n][2], T(r["iou"])), (io[n][3], T(enc))]
    arena.run(call, expect)


# ------------------------------------------------------------------------------------------------------------------ 2, 3. matcher
class MatchCall:
    """One ragged batch in an arena: inputs, the four outputs, a workspace of exactly ssd_match_encode_workspace_bytes."""

    def __init__(self, ops, L, geo, which):
        self.L, self.ps = L, pset_of(ops, geo)
        self.images = AC.match_batch(geo, which)
        box, cls, off, self.total, self.max_nt = AC.pack_gt(self.images)
        self.B, self.A = len(self.images), self.ps.A
        B, A = self.B, self.A
        self.need = L.ssd_match_encode_workspace_bytes(B, A, self.total)
        assert self.need > 0
        self.arena = ar = strict.Arena("cuda", strict.Arena.bytes_for(box.nbytes, cls.nbytes, off.nbytes, A * 32, A * 16, B * A * 4,
                                                                      B * A * 16, B * A, B * A * 4, self.need))
        self.gt_box, self.gt_cls, self.gt_off = ar.put(T(box), "gt_box"), ar.put(T(cls), "gt_cls"), ar.put(T(off), "gt_off")
        self.pri, self.enc0 = ar.put(self.ps.priors, "priors"), ar.put(self.ps.enc_zero, "enc_zero")
        self.cls, self.loc = ar.out((B, A), torch.int32, "out_cls"), ar.out((B, A, 4), torch.float32, "out_loc")
        self.mask, self.owner = ar.out((B, A), torch.uint8, "out_mask"), ar.out((B, A), torch.int32, "out_owner")
        self.ws = ar.workspace().get(self.need, self.cls.device)
        assert self.ws.numel() == self.need

    def call(self, grid, owner=True, ws=True):
        return self.L.ssd_match_encode(P(self.gt_box), P(self.gt_cls), P(self.gt_off), self.B, self.total, self.max_nt, P(self.pri),
                                       P(self.enc0), self.A, ctypes.byref(grid) if grid is not None else None, 0.5, P(self.cls),
                                       P(self.loc), P(self.mask), P(self.owner if owner else None), P(self.ws if ws else None),
                                       self.need if ws else 0, stream())

    def check(self, outs, tag):
        cls, loc, mask, owner = outs
        for i, img in enumerate(self.images):
            check_image("%s image %d" % (tag, i), img, cls[i], loc[i], mask[i], owner[i])

    def want(self, first):
        """the oracle's arrays where it is bit-exact (classes, masks); the checked plain call's bits for loc and owner"""
        w_cls = np.stack([i["cls"] for i in self.images]).astype(np.int32)
        w_mask = np.stack([i["mask"] for i in self.images]).astype(np.uint8)
        return [(self.cls, T(w_cls)), (self.loc, T(first[1])), (self.mask, T(w_mask)), (self.owner, T(first[3]))]


def wrong_grid():
    from ssd_object_detection_amd import _lib
    bad = _lib.PriorGrid()
    bad.levels = 3
    for i, (h, w, k) in enumerate([(7, 5, 3), (40, 40, 5), (2, 9, 1)]):
        bad.grid_h[i], bad.grid_w[i], bad.per_cell[i] = h, w, k
    return bad


@pytest.mark.parametrize("geo", ["G4", "G190", "G790"])
def test_match_three_launch_path(ops, L, geo):
    """n_t == A, one partial chunk, more than P1_LDS_ROWS boxes in an image; with the hint, without, with a wrong one; the
    workspace poisoned; owner == NULL."""
    m = MatchCall(ops, L, geo, "main")
    outs = [m.cls, m.loc, m.mask, m.owner]
    hint = ops.make_grid(AC.GEOMETRIES[geo]["grids"], AC.GEOMETRIES[geo]["ratios"])
    assert hint.verified == 0
    first = None
    for tag, grid in (("hint", hint), ("no hint", None), ("wrong hint", wrong_grid())):
        got = plain(m.arena, lambda: ok(m.call(grid)), outs)
        m.check(got, tag)
        if first is None:
            first = got
        for a, b in zip(first, got):                                       # the hint can never change a result
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), tag
    want = m.want(first)
    m.arena.run(lambda: ok(m.call(hint)), want)
    m.arena.run(lambda: ok(m.call(None, owner=False)), want[:3])          # owner == NULL: out_owner keeps its poison


@pytest.mark.parametrize("geo,which", [("G190", "main"), ("G790", "small")])
def test_match_single_launch_path(ops, L, geo, which):
    m = MatchCall(ops, L, geo, which)
    outs = [m.cls, m.loc, m.mask, m.owner]
    ps = m.ps
    assert ps.verify_grid() is True and m.max_nt <= 64
    assert m.call(ps.grid, ws=False) == -3                                # SSD_ERR_WORKSPACE: the three-launch path needs one
    try:
        ok(L.ssd_dev_knob(b"SSD_MATCH_FUSED", 1))
        fused = lambda: ok(m.call(ps.grid, ws=False))                      # noqa: E731  success without a workspace: the path was taken
        got = plain(m.arena, fused, outs)
        m.check(got, "fused")
        m.arena.run(fused, m.want(got))
    finally:
        L.ssd_dev_knob(b"SSD_MATCH_FUSED", 0)
    three = plain(m.arena, lambda: ok(m.call(ps.grid)), outs)
    for a, b in zip(got, three):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# -------------------------------------------------------------------------------------------------------------- 4. score / decode
class ScoreCall:
    def __init__(self, ops, L, A, C, dt, conf, loc):
        self.L, self.A, self.C, self.B = L, A, C, conf.shape[0]
        dtype = torch.float32 if dt == "f32" else torch.bfloat16
        self.code = 0 if dt == "f32" else 1
        ps = pset_of(ops, AC.GEOMETRY_OF_A[A])
        B = self.B
        self.arena = ar = strict.Arena("cuda", strict.Arena.bytes_for(B * A * C * 4, B * A * 16, A * 32, B * A * 4, B * A * 4,
                                                                      B * A * 16, B * A))
        self.conf, self.loc = ar.put(T(conf).to(dtype), "conf"), ar.put(T(loc).to(dtype), "loc")
        assert torch.equal(self.conf.float().cpu(), T(conf)) and torch.equal(self.loc.float().cpu(), T(loc))
        self.pri = ar.put(ps.priors, "priors")
        self.score, self.cls = ar.out((B, A), torch.float32, "score"), ar.out((B, A), torch.int32, "cls")
        self.box, self.cand = ar.out((B, A, 4), torch.float32, "box"), ar.out((B, A), torch.uint8, "cand")
        self.outs = [self.score, self.cls, self.box, self.cand]

    def call(self, thresh):
        ok(self.L.ssd_score_decode(P(self.conf), P(self.loc), self.code, P(self.pri), self.B, self.A, self.C, thresh, 300.0,
                                   P(self.score), P(self.cls), P(self.box), P(self.cand), stream()))


def check_boxes(box, cand, box64):
    np.testing.assert_allclose(box[cand], box64[cand], rtol=3e-7, atol=0)
    assert (box[~cand].view(np.uint32) == 0).all()                       # +0 exactly where the row is no candidate


@pytest.mark.parametrize("A", [190, 790])
@pytest.mark.parametrize("C,dt", AC.SCORE_CASES)
def test_score_decode_random_logits_and_class_ties(ops, L, A, C, dt):
    case = AC.score_case(A, C, dt)
    s = ScoreCall(ops, L, A, C, dt, case["conf"], case["loc"])
    score, cls, box, cand = plain(s.arena, lambda: s.call(AC.SCORE_THRESH), s.outs)
    cand = cand.astype(bool)
    print("A", A, "C", C, dt, "max score error", float(np.abs(score - case["score"]).max()), "border rows", int(case["border"].sum()))
    np.testing.assert_allclose(score, case["score"], rtol=2e-6, atol=1e-9)
    assert np.array_equal(cand[~case["border"]], case["cand"][~case["border"]]) and cand.sum() > 10
    assert np.array_equal(cls[cand], case["cls_oracle"][cand])
    for row, lo, hi in case["ties"]:                                      # the first index wins, within and across the half rows
        assert cls.reshape(-1)[row] == lo and cand.reshape(-1)[row], (row, lo, hi, cls.reshape(-1)[row])
    check_boxes(box, cand, case["box"])
    s.arena.run(lambda: s.call(AC.SCORE_THRESH),
                [(s.score, T(score)), (s.cls, T(case["cls"])), (s.box, T(box)), (s.cand, T(cand.astype(np.uint8)))])


@pytest.mark.parametrize("A", [190, 790])
@pytest.mark.parametrize("C,dt", AC.SCORE_CASES)
def test_score_decode_exact_threshold(ops, L, A, C, dt):
    """score_thresh = the bits of a row's own score: `>` is strict, and p_background == score is never a candidate."""
    case = AC.threshold_case(A, C, dt)
    s = ScoreCall(ops, L, A, C, dt, case["conf"], case["loc"])
    score0 = plain(s.arena, lambda: s.call(0.5), s.outs)[0]
    t = float(score0.reshape(-1)[case["src"]])
    assert np.float32(t) == score0.reshape(-1)[case["src"]]
    score, cls, box, cand = plain(s.arena, lambda: s.call(t), s.outs)
    cand = cand.astype(bool)
    assert np.array_equal(score.view(np.uint32), score0.view(np.uint32))
    tie = case["tie"]
    at = (score == np.float32(t)) & ~tie
    assert at.reshape(-1)[case["dups"]].all() and at.sum() >= 4            # rows exactly at the threshold
    if C >= 3:
        assert ((score > np.float32(t)) & ~tie).any() and ((score < np.float32(t)) & ~tie).any()
    assert np.array_equal(cand, (score > np.float32(t)) & ~tie)           # every row: none is left out
    assert np.array_equal(cls, case["cls"])
    check_boxes(box, cand, case["box"])
    s.arena.run(lambda: s.call(t), [(s.score, T(score)), (s.cls, T(case["cls"])), (s.box, T(box)), (s.cand, T(cand.astype(np.uint8)))])


# ------------------------------------------------------------------------------------------------------------------------ 5. NMS
@pytest.mark.parametrize("A", AC.NMS_ANCHORS)
def test_nms(L, A):
    case = AC.nms_case(A)
    B = case["B"]
    assert L.ssd_nms_max_candidates() == 1024
    arena = strict.Arena("cuda", strict.Arena.bytes_for(B * A * 4, B * A * 4, B * A * 16, B * A, B * A, B * 4))
    score, cls = arena.put(T(case["score"]), "score"), arena.put(T(case["cls"]), "cls")
    box, cand = arena.put(T(case["box"]), "box"), arena.put(T(case["cand"]), "cand")
    keep, count = arena.out((B, A), torch.uint8, "keep"), arena.out((B,), torch.int32, "keep_count")

    def call(mc, with_count=True, anchors=A):
        return L.ssd_nms(P(score), P(cls), P(box), P(cand), B, anchors, AC.NMS_IOU, mc, P(keep), P(count if with_count else None),
                         stream())

    for mc in AC.NMS_MAX_CAND:
        w_keep, w_count = case["want"][mc]
        arena.run(lambda: ok(call(mc)), [(keep, T(w_keep)), (count, T(w_count))])
    arena.run(lambda: ok(call(50, with_count=False)), [(keep, T(case["want"][50][0]))])      # keep_count == NULL
    if A == 65536:                                                          # one more anchor than the key holds: refused, nothing runs
        def refused():
            assert call(1024, anchors=65537) == -2
        arena.run(refused, [])


# ------------------------------------------------------------------------------------------------------- 6. eval-match and eval-AP
@pytest.mark.parametrize("A", AC.EVAL_ANCHORS)
def test_eval_match(L, A):
    case = AC.eval_case(A)
    B = case["B"]
    mds = AC.EVAL_MAX_DETS
    arena = strict.Arena("cuda", strict.Arena.bytes_for(B * A * 4, B * A * 4, B * A * 16, B * A, case["gt_cls"].nbytes,
                                                        case["gt_box"].nbytes, 64, *[8192] * (5 * len(mds))))
    ins = [arena.put(T(case[k]), k) for k in ("score", "cls", "box", "keep", "gt_cls", "gt_box", "gt_off")]
    outs = {md: [arena.out((B,), torch.int32, "n_det%d" % md), arena.out((B, md), torch.float32, "det_score%d" % md),
                 arena.out((B, md), torch.int32, "det_cls%d" % md), arena.out((B, md, 4), torch.float32, "det_box%d" % md),
                 arena.out((B, md), torch.int16, "det_flags%d" % md)] for md in mds}
    thr = AC.M.IOU_THRESHOLDS.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def call(md):
        ok(L.ssd_eval_match(*[P(t) for t in ins[:4]], B, A, *[P(t) for t in ins[4:]], thr, md, *[P(t) for t in outs[md]], stream()))

    for md in mds:
        n_det, d_score, d_cls, d_box, d_flags = case["want"][md]
        want = [T(n_det), T(d_score), T(d_cls), T(d_box), T(d_flags.view(np.int16))]
        arena.run(lambda: call(md), list(zip(outs[md], want)))             # the other max_dets' outputs keep their poison


def test_eval_ap(L):
    case = AC.ap_case()
    C = case["C"]
    flags = case["flags_sorted"].view(np.int16)
    arena = strict.Arena("cuda", strict.Arena.bytes_for(flags.nbytes, 64, 64, C * 80))
    a_flags, a_seg, a_ngt = arena.put(T(flags), "flags"), arena.put(T(case["seg_off"]), "seg_off"), arena.put(T(case["n_gt"]), "n_gt")
    ap = arena.out((C, 10), torch.float64, "ap")
    pts = AC.M.RECALL_POINTS.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def call():
        ok(L.ssd_eval_ap(P(a_flags), P(a_seg), P(a_ngt), C, pts, P(ap), stream()))

    got = plain(arena, call, [ap])[0]
    print("max AP difference", float(np.abs(got - case["ap"]).max()), "bit-equal", np.array_equal(got, case["ap"]))
    assert np.abs(got - case["ap"]).max() <= 1e-12
    assert (got[1] == 0).all() and (got[2] == 0).all()                    # no detections; no ground truth
    arena.run(call, [(ap, T(got))])
