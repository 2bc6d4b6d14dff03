"""GPU: the single-label detection path -- ssd_score_decode, ssd_nms, ssd_eval_match -- through the C ABI under tests/strict.py:
every tensor in a guarded arena, every call twice over two poisons, every comparison an equality (tests/detect_cases.py builds
the cases and states the references; tests/test_detect_cases_cpu.py shows on the CPU that they are what they claim).

Which test reaches which path:
  k_score_decode<T, 0>, C = 2, 3, 6, 82 and <T, 81>; whole and partial row blocks      test_score_decode_exact_design
  ties of the argmax in and across the two lanes; class of every row; strict `>`;
  score == p_background == threshold; the maximum subtracted (t = 96)                  test_score_decode_exact_design
  a second, prefetched block per workgroup and a partial last block (98 433 rows)      test_score_decode_second_block
  the exp branch of the decode; random logits against the float64 oracle               test_score_decode_random_offsets, _random_logits
  more than 64 KiB of dynamic LDS (C = 129, 300) and the refusal one past it           test_class_counts_above_64k_of_lds
  k_nms: both sweeps, rows at unaligned offsets, anchor 65535, the radix cut and its
  ties, segments in registers and in LDS, more segments than waves, chains, the IoU
  at the threshold, cand bytes, junk in non-candidate rows, keep_count == NULL         test_nms
  refusals that write nothing                                                          test_nms_refusals
  k_eval_match: the byte-wise sweep, 48 / 49 ground truths, 1024 / 1025 kept anchors   test_eval_match

Outcome on an MI355X: every test passes against the kernels as they were; nothing in detect.hip or evalmap.hip had to change.
The launches with 66 048 and 153 600 bytes of dynamic LDS (C = 129, 300) succeed without a
hipFuncAttributeMaxDynamicSharedMemorySize registration, and C = 301 is refused with every output still poisoned.
Three one-line mutations of the kernels, tried on a scratch copy, turn these tests red: `>=` for `>` behind iou_f32 (test_nms:
the nested pair at the threshold, seg-63 / 64 in registers, seg-65 / 1024 in LDS, and others), the `oi < mi` tie rule dropped
(test_score_decode_exact_design for every C >= 3), the four-byte reader forced for every A (test_nms at every A % 4 != 0,
test_eval_match in every case)."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import ssd_oracle as O                                   # noqa: E402
from tests import detect_cases as D                                  # noqa: E402
from tests import strict                                             # noqa: E402

ERR_VALUE, ERR_UNSUPPORTED = -2, -5
DT = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1)}


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def ok(status):
    assert status == 0, status


def plain(arena, fn, outs):
    """one call on freshly poisoned tensors; the outputs as numpy"""
    arena.poison(False)
    fn()
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy() for t in outs]


# ------------------------------------------------------------------------------------------------------------ 1. score / decode
class ScoreCall:
    def __init__(self, L, conf, loc, priors, dt, in_size=300.0):
        self.L, self.in_size = L, float(in_size)
        self.B, self.A, self.C = conf.shape
        dtype, self.code = DT[dt]
        B, A, C = conf.shape
        self.arena = ar = strict.Arena("cuda", strict.Arena.bytes_for(B * A * C * 4, B * A * 16, A * 32, B * A * 4, B * A * 4,
                                                                      B * A * 16, B * A, B * A * (C - 1) * 4))
        self.conf, self.loc = ar.put(T(conf).to(dtype), "conf"), ar.put(T(loc).to(dtype), "loc")
        assert torch.equal(self.conf.float().cpu(), T(conf)) and torch.equal(self.loc.float().cpu(), T(loc))
        self.pri = ar.put(T(priors), "priors")
        self.score, self.cls = ar.out((B, A), torch.float32, "score"), ar.out((B, A), torch.int32, "cls")
        self.box, self.cand = ar.out((B, A, 4), torch.float32, "box"), ar.out((B, A), torch.uint8, "cand")
        self.outs = [self.score, self.cls, self.box, self.cand]

    def call(self, thresh, C=None):
        return self.L.ssd_score_decode(P(self.conf), P(self.loc), self.code, P(self.pri), self.B, self.A, C or self.C, thresh,
                                       self.in_size, P(self.score), P(self.cls), P(self.box), P(self.cand), stream())

    def run_design(self, case, thresholds):
        for th in thresholds:
            cand = D.candidates(case, th)
            self.arena.run(lambda: ok(self.call(th)), [(self.score, T(case["score"])), (self.cls, T(case["cls"])),
                                                       (self.box, T(D.boxes_of(case, cand))), (self.cand, T(cand.astype(np.uint8)))])


def design_call(L, C, B, A, dt, in_size=300.0):
    case = D.score_case(C, B, A, in_size)
    return case, ScoreCall(L, case["conf"], case["loc"], case["priors"], dt, in_size)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", D.GENERIC_C + (81,))
def test_score_decode_exact_design(L, C, dt):
    """Rows of n tied tops: score 1/n bit for bit, the lowest top as the class of EVERY row, candidates by the two strict
    float32 comparisons at 1/2, 1/4, 1/8 and the float32 below each, boxes bit for bit and 0 for non-candidates."""
    for i, (B, A) in enumerate(D.SCORE_SHAPES):
        case, s = design_call(L, C, B, A, dt, D.IN_SIZES[i % 2])
        s.run_design(case, D.THRESHOLDS)


def test_score_decode_second_block(L):
    """768 * 128 + 129 rows at C = 81: workgroups 0 and 1 take a second block (requested while the first is scored), the last
    block holds one row"""
    case, s = design_call(L, 81, *D.BIG_SHAPE, "f32")
    s.run_design(case, (D.THRESHOLDS[2], D.THRESHOLDS[5]))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", [6, 81])
def test_score_decode_random_offsets(L, C, dt):
    """t_w, t_h != 0: the exponential of the decode, rtol 3e-7 against the float64 oracle; candidates stay exact"""
    B, A = D.RANDOM_SHAPE
    case = D.score_case(C, B, A)
    loc = D.random_case(6, dt)["loc"]
    s = ScoreCall(L, case["conf"], loc, case["priors"], dt)
    th = D.THRESHOLDS[3]
    score, cls, box, cand = plain(s.arena, lambda: ok(s.call(th)), s.outs)
    want_cand = D.candidates(case, th)
    assert np.array_equal(cand.astype(bool), want_cand) and want_cand.sum() > 50
    want = O.decode(loc, case["priors"][None], 300)
    print("C", C, dt, "max relative box error", float(np.abs(box[want_cand] / want[want_cand] - 1).max()))
    np.testing.assert_allclose(box[want_cand], want[want_cand], rtol=3e-7, atol=0)
    assert (box[~want_cand].view(np.uint32) == 0).all()
    s.arena.run(lambda: ok(s.call(th)), [(s.score, T(case["score"])), (s.cls, T(case["cls"])), (s.box, T(box)),
                                         (s.cand, T(want_cand.astype(np.uint8)))])


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", D.GENERIC_C)
def test_score_decode_random_logits(L, C, dt):
    """the project's tolerances against oracle.ssd_oracle.score / decode; no row is left out (test_detect_cases_cpu.py: the
    float64 reference has no row within 1e-6 of the threshold); the class of every row is the oracle's"""
    case = D.random_case(C, dt)
    s = ScoreCall(L, case["conf"], case["loc"], case["priors"], dt)
    th = D.RANDOM_THRESH
    score, cls, box, cand = plain(s.arena, lambda: ok(s.call(th)), s.outs)
    cand = cand.astype(bool)
    print("C", C, dt, "max score error", float(np.abs(score - case["score"]).max()), "border rows", int(case["border"].sum()))
    np.testing.assert_allclose(score, case["score"], rtol=2e-6, atol=1e-9)
    assert np.array_equal(cand[~case["border"]], case["cand"][~case["border"]])
    assert np.array_equal(cls, case["cls"])
    np.testing.assert_allclose(box[cand], case["box"][cand], rtol=3e-7, atol=0)
    assert (box[~cand].view(np.uint32) == 0).all()
    s.arena.run(lambda: ok(s.call(th)), [(s.score, T(score)), (s.cls, T(case["cls"])), (s.box, T(box)),
                                         (s.cand, T(cand.astype(np.uint8)))])


# --------------------------------------------------------------------------------------------- 2. more than 64 KiB of dynamic LDS
@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C", D.LDS_C)
def test_class_counts_above_64k_of_lds(L, C, dt):
    """128 rows of C floats: 66 048 bytes at C = 129, 153 600 (the host bound exactly) at C = 300 -- ssd_score_decode,
    ssd_class_scores and (status and pair count only) ssd_detect_pairs, which share the bound"""
    B, A = D.LDS_SHAPE
    case, s = design_call(L, C, B, A, dt)
    s.run_design(case, (D.THRESHOLDS[2], D.THRESHOLDS[3]))
    prob = s.arena.out((B, A, C - 1), torch.float32, "prob")
    s.arena.run(lambda: ok(L.ssd_class_scores(P(s.conf), s.code, B, A, C, P(prob), stream())), [(prob, T(case["prob"]))])
    # the listing form of the same sweep
    K, th = 8, D.THRESHOLDS[3]
    need = L.ssd_detect_pairs_workspace_bytes(B, A, C)
    dev = s.conf.device
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    n_cand, n_det = torch.full((B,), -1, dtype=torch.int32, device=dev), torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_score, d_cls = torch.empty((B, K), device=dev), torch.empty((B, K), dtype=torch.int32, device=dev)
    d_anchor, d_box = torch.empty((B, K), dtype=torch.int32, device=dev), torch.empty((B, K, 4), device=dev)
    d_valid = torch.empty((B, K), dtype=torch.uint8, device=dev)
    s.arena.poison(False)
    ok(L.ssd_detect_pairs(P(s.conf), P(s.loc), s.code, P(s.pri), B, A, C, th, 300.0, 0.45, 1024, K, P(n_cand), P(n_det),
                          P(d_score), P(d_cls), P(d_anchor), P(d_box), P(d_valid), P(ws), need, stream()))
    torch.cuda.synchronize()
    want = (case["prob"] > np.float32(th)).sum((1, 2))
    nd = n_det.cpu().numpy()
    assert n_cand.cpu().numpy().tolist() == want.tolist() and want.min() > K and (nd > 0).all() and (nd <= K).all()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_class_count_one_past_the_lds_bound_is_refused(L, dt):
    C = D.LDS_REFUSED_C
    B, A = D.LDS_SHAPE
    case, s = design_call(L, C, B, A, dt)
    prob = s.arena.out((B, A, C - 1), torch.float32, "prob")

    def refused():
        assert s.call(0.25) == ERR_UNSUPPORTED
        assert L.ssd_class_scores(P(s.conf), s.code, B, A, C, P(prob), stream()) == ERR_UNSUPPORTED

    s.arena.run(refused, [])                                              # every output keeps its poison


# ------------------------------------------------------------------------------------------------------------------------ 3. NMS
class NmsCall:
    def __init__(self, L, case):
        self.L, self.case = L, case
        self.B, self.A = B, A = case["B"], case["A"]
        self.arena = ar = strict.Arena("cuda", strict.Arena.bytes_for(B * A * 4, B * A * 4, B * A * 16, B * A, B * A, B * 4))
        score, cls, box, cand = D.nms_inputs(case, 0)
        self.score, self.cls = ar.put(T(score), "score"), ar.put(T(cls), "cls")
        self.box, self.cand = ar.put(T(box), "box"), ar.put(T(cand), "cand")
        self.keep, self.count = ar.out((B, A), torch.uint8, "keep"), ar.out((B,), torch.int32, "keep_count")

    def other_junk(self):
        score, cls, box, cand = D.nms_inputs(self.case, 1)
        self.arena.set(self.score, T(score)), self.arena.set(self.cls, T(cls)), self.arena.set(self.box, T(box))

    def call(self, iou, mc, with_count=True, A=None, null=None):
        args = dict(score=self.score, cls=self.cls, box=self.box, cand=self.cand, keep=self.keep,
                    count=self.count if with_count else None)
        if null:
            args[null] = None
        return self.L.ssd_nms(P(args["score"]), P(args["cls"]), P(args["box"]), P(args["cand"]), self.B, A or self.A, iou, mc,
                              P(args["keep"]), P(args["count"]), stream())

    def run(self, iou, mc, want):
        self.arena.run(lambda: ok(self.call(iou, mc)), [(self.keep, T(want[0])), (self.count, T(want[1]))])


@pytest.mark.parametrize("name", D.NMS_NAMES)
def test_nms(L, name):
    """keep and keep_count bit for bit against oracle.ssd_oracle.nms -- and, for the hand cases, against the keep set written
    out in tests/detect_cases.py -- for every max_cand of the case, then again with other junk in the rows of non-candidates
    (NaN and huge values first; then a score above every candidate's, a class in use, a box on top of the clusters), and once
    with keep_count == NULL, where the count tensor keeps its poison."""
    case = D.nms_case(name)
    n = NmsCall(L, case)
    assert L.ssd_nms_max_candidates() == D.NMS_CAP
    for junk in (0, 1):
        if junk:
            n.other_junk()
        for mc in case["max_cands"]:
            want = D.nms_want(name, mc)
            if "hand" in case and mc >= len(case["hand"]["rows"]):
                assert np.array_equal(want[0], D.hand_keep(case))
                want = (D.hand_keep(case), np.array([len(case["hand"]["keep"])], np.int32))
            n.run(case["iou"], mc, want)
        if "hand" in case:
            for iou in (0.0, 1.0):
                n.run(iou, D.NMS_CAP, D.nms_want(name, D.NMS_CAP, iou))
    mc = case["max_cands"][0]
    n.arena.run(lambda: ok(n.call(case["iou"], mc, with_count=False)), [(n.keep, T(D.nms_want(name, mc)[0]))])


def test_nms_refusals(L):
    """A = 65537, max_cand 0 and 1025, each NULL pointer: SSD_ERR_VALUE and nothing written"""
    n = NmsCall(L, D.nms_case("size-190"))

    def refused():
        assert n.call(0.45, 1024, A=65537) == ERR_VALUE
        assert n.call(0.45, 0) == ERR_VALUE and n.call(0.45, 1025) == ERR_VALUE and n.call(0.45, -1) == ERR_VALUE
        for null in ("score", "cls", "box", "cand", "keep"):
            assert n.call(0.45, 1024, null=null) == ERR_VALUE, null

    n.arena.run(refused, [])


# ----------------------------------------------------------------------------------------------------------------- 4. eval-match
@pytest.mark.parametrize("md", D.EVAL_MAX_DETS)
@pytest.mark.parametrize("A", D.EVAL_ANCHORS)
def test_eval_match(L, A, md):
    """n_det, scores, classes, boxes and flags bit for bit against tests.eval_cases.match_reference; rows at or beyond n_det
    hold score 0, class -1, box 0, flags 0 (they are part of the reference); all five outputs between guard bands"""
    case = D.eval_case(A, md)
    B = case["B"]
    arena = strict.Arena("cuda", strict.Arena.bytes_for(B * A * 4, B * A * 4, B * A * 16, B * A, case["gt_cls"].nbytes,
                                                        case["gt_box"].nbytes, 64, *[8192] * 5))
    ins = [arena.put(T(case[k]), k) for k in ("score", "cls", "box", "keep", "gt_cls", "gt_box", "gt_off")]
    outs = [arena.out((B,), torch.int32, "n_det"), arena.out((B, md), torch.float32, "det_score"),
            arena.out((B, md), torch.int32, "det_cls"), arena.out((B, md, 4), torch.float32, "det_box"),
            arena.out((B, md), torch.int16, "det_flags")]
    thr = D.E.M.IOU_THRESHOLDS.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    n_det, d_score, d_cls, d_box, d_flags = case["want"]
    want = [T(n_det), T(d_score), T(d_cls), T(d_box), T(d_flags.view(np.int16))]

    def call():
        ok(L.ssd_eval_match(*[P(t) for t in ins[:4]], B, A, *[P(t) for t in ins[4:]], thr, md, *[P(t) for t in outs], stream()))

    got = arena.run(call, list(zip(outs, want)))
    assert np.array_equal(got[1].cpu().numpy().view(np.uint32), d_score.view(np.uint32))       # bits: -0 is not +0
    assert np.array_equal(got[3].cpu().numpy().view(np.uint32), d_box.view(np.uint32))
