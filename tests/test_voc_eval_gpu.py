"""GPU: PASCAL VOC's AP on the device.  ssd_eval_match_voc against utils.metrics.voc_match_image bit for bit and
ssd_eval_ap_voc against utils.metrics.voc_ap_from_rows, both through the C ABI under tests/strict.py (guarded arena, outputs
poisoned twice); the refusals; ops.eval_match_voc / ops.eval_ap_voc and DeviceVocAccumulator against voc_map.

utils.metrics.voc_map is build-defined: a numpy restatement of the published VOCdevkit procedure, unpinned (see
tests/voc_cases.py).

Bounds: bit equality for every output of the match kernel (the device's own selected rows included); 1e-12 for AP, the
project's bound for its AP kernels -- ssd_eval_ap_voc performs the definition's divisions and adds in the definition's order, so
the observed difference is expected to be 0."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                             # noqa: E402
from tests import voc_cases as V                                     # noqa: E402

M = V.M


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


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


def dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ---- the batches ---------------------------------------------------------------------------------------------------------------
def _take(case, idx, **kw):
    return dict(case, dets=[case["dets"][i] for i in idx], gts=[case["gts"][i] for i in idx], **kw)


def small_case(max_dets):
    """B = 3, A = 37 (A % 4 != 0: the byte path of the keep scan); image 0 has no box; quantised scores tie across anchors"""
    dets, gts = V.gen_images(np.random.default_rng(7300), 3, kept_lo=20, kept_hi=37, quant=10, n_gt_lo=3)
    gts[0] = (np.zeros(0, np.int32), np.zeros((0, 4)), np.zeros(0, bool))
    return dict(name="small", dets=dets, gts=gts, max_dets=max_dets, iou_thresh=0.5, A=37)


def radix_case(max_dets):
    """A = 1100 and every anchor kept: more kept anchors than sort slots, the exact radix cut, inside runs of equal scores"""
    dets, gts = V.gen_images(np.random.default_rng(7400), 2, kept_lo=1100, kept_hi=1100, quant=50, n_gt_lo=6, n_gt_hi=12)
    return dict(name="radix", dets=dets, gts=gts, max_dets=max_dets, iou_thresh=0.5, A=1100, all_kept=True)


def big_case():
    """Image 0 has 90 boxes (the path without the LDS arrays); images 1 and 2 are the same image split by class, 2 and 3
    classes each and at most 64 boxes: per class nothing changes, so every detection must get the same flags and, counted inside
    its class, the same box on both paths."""
    rng = np.random.default_rng(7500)
    (d,), (g,) = V.gen_images(rng, 1, n_cls=5, kept_lo=120, kept_hi=120, quant=20, n_gt_lo=90, n_gt_hi=90)
    parts = []
    for classes in ((0, 1), (2, 3, 4, 5, 6)):
        dm, gm = np.isin(d[1], classes), np.isin(g[0], classes)
        assert gm.sum() <= 64
        parts.append(((d[0][dm], d[1][dm], d[2][dm]), (g[0][gm], g[1][gm], g[2][gm]), np.nonzero(dm)[0], np.nonzero(gm)[0]))
    case = dict(name="big", dets=[d] + [p[0] for p in parts], gts=[g] + [p[1] for p in parts], max_dets=128, iou_thresh=0.5, A=256)
    return case, parts


def hand_batches():
    return [dict(c, A=37) for c in V.HAND]


def random_batch():
    return dict(V.random_set(), A=61)


MATCH_CASES = ([("small", md) for md in (1, 100, 200, 256)] + [("radix", md) for md in (100, 200, 256)]
               + [("big", 128), ("random", 20)] + [("hand:" + c["name"], c["max_dets"]) for c in V.HAND])


def _case_of(name, md):
    if name == "small":
        return small_case(md)
    if name == "radix":
        return radix_case(md)
    if name == "big":
        return big_case()[0]
    if name == "random":
        return random_batch()
    return next(c for c in hand_batches() if "hand:" + c["name"] == name)


def run_match(L, case, with_difficult=True):
    """ssd_eval_match_voc on the case as one batch under the strict arena, every output against the restatement; returns the
    reference"""
    md, A = case["max_dets"], case["A"]
    d = V.dense_batch(case, A, all_kept=case.get("all_kept", False))
    B, G = len(case["dets"]), len(d["gt_cls"])
    arena = strict.Arena("cuda", strict.Arena.bytes_for(B * A * 4, B * A * 4, B * A * 16, B * A, G * 4 + 4, G * 32 + 32, B * 4 + 4,
                                                        G + 1, 64, *[B * md * 16] * 5))
    ins = {k: arena.put(T(d[k]), k) for k in ("score", "cls", "box", "keep", "gt_cls", "gt_box", "gt_off", "gt_difficult")}
    outs = [arena.out((B,), torch.int32, "n_det"), arena.out((B, md), torch.float32, "det_score"),
            arena.out((B, md), torch.int32, "det_cls"), arena.out((B, md, 4), torch.float32, "det_box"),
            arena.out((B, md), torch.uint8, "det_flags"), arena.out((B, md), torch.int32, "det_gt")]
    ref = V.match_reference(case, with_difficult=with_difficult)

    def call():
        status = L.ssd_eval_match_voc(P(ins["score"]), P(ins["cls"]), P(ins["box"]), P(ins["keep"]), B, A, P(ins["gt_cls"]),
                                      P(ins["gt_box"]), P(ins["gt_off"]), P(ins["gt_difficult"] if with_difficult else None),
                                      ctypes.c_double(case["iou_thresh"]), md, *[P(t) for t in outs], stream())
        assert status == 0, status

    arena.run(call, list(zip(outs, [T(ref[k]) for k in ("n_det", "score", "cls", "box", "flags", "gt")])))
    return ref


@pytest.mark.parametrize("name,md", MATCH_CASES)
def test_eval_match_voc_equals_the_restatement(L, name, md):
    """every output bit for bit, slots beyond n_det empty, nothing written outside the outputs, under two poisons"""
    case = _case_of(name, md)
    ref = run_match(L, case)
    assert int(ref["n_det"].max()) == min(md, max(len(x[0]) for x in case["dets"]))
    if name == "small":
        assert ref["n_det"][0] > 0 and (ref["gt"][0] == -1).all() and (ref["flags"][0] == 0).all()      # the image without boxes
        if md >= 100:
            sc = ref["score"][1, :ref["n_det"][1]]
            assert len(np.unique(sc)) < len(sc)                       # equal scores across anchors
            run_match(L, case, with_difficult=False)                  # the NULL pointer: no box is difficult
    if name == "radix":
        assert all(len(x[0]) == 1100 for x in case["dets"])
        cut = ref["score"][0, md - 1]
        assert (case["dets"][0][0] == cut).sum() > (ref["score"][0] == cut).sum()        # the cut falls inside a run of ties
    if name in ("random", "big"):
        kinds = np.bincount(ref["flags"].reshape(-1), minlength=3)
        dup = int(((ref["gt"] >= 0) & (ref["flags"] == 0)).sum())
        print(name, "false / true / ignored", kinds[:3], "duplicates", dup)
        assert (kinds[:3] > 0).all() and dup > 0


def test_both_paths_agree_on_an_image_split_by_class(L):
    case, parts = big_case()
    assert len(case["gts"][0][0]) == 90 and all(len(p[1][0]) <= 64 for p in parts)
    ref = run_match(L, case)                                          # (the kernel's outputs equal ref: checked in there)
    n0 = int(ref["n_det"][0])
    assert n0 == 120
    # detections of the whole image, by their index in its list
    order0 = np.argsort(-case["dets"][0][0].astype(np.float64), kind="mergesort")
    whole = {int(order0[r]): (int(ref["flags"][0, r]), int(ref["gt"][0, r])) for r in range(n0)}
    seen = 0
    for k, (dets, _, det_idx, gt_idx) in enumerate(parts, start=1):
        order = np.argsort(-dets[0].astype(np.float64), kind="mergesort")
        for r in range(int(ref["n_det"][k])):
            flags, gt = whole[int(det_idx[order[r]])]
            assert flags == int(ref["flags"][k, r])
            assert gt == (int(gt_idx[ref["gt"][k, r]]) if ref["gt"][k, r] >= 0 else -1)
            seen += 1
    assert seen == n0


def test_entry_points_refuse_before_any_launch(L):
    from ssd_object_detection_amd import _lib
    case = small_case(100)
    d = V.dense_batch(case, 37)
    B, A, md, G = 3, 37, 100, len(d["gt_cls"])
    arena = strict.Arena("cuda", strict.Arena.bytes_for(*[B * md * 16] * 18))      # eight inputs, six outputs, the AP call's four
    ins = {k: arena.put(T(d[k]), k) for k in ("score", "cls", "box", "keep", "gt_cls", "gt_box", "gt_off", "gt_difficult")}
    outs = [arena.out((B,), torch.int32, "n_det"), arena.out((B, md), torch.float32, "det_score"),
            arena.out((B, md), torch.int32, "det_cls"), arena.out((B, md, 4), torch.float32, "det_box"),
            arena.out((B, md), torch.uint8, "det_flags"), arena.out((B, md), torch.int32, "det_gt")]
    fl, seg, npos = arena.put(T(np.zeros(8, np.uint8)), "flags"), arena.put(T(np.array([0, 8], np.int32)), "seg_off"), \
        arena.put(T(np.array([4], np.int32)), "n_pos")
    ap = arena.out((1,), torch.float64, "ap")
    assert L.ssd_eval_voc_max_dets() == 256 and L.ssd_eval_max_dets() == 128

    def match(B=B, A=A, md=md, thr=0.5, score=ins["score"], gt_off=ins["gt_off"], flags=outs[4], gt=outs[5]):
        o = [P(t) for t in outs[:4]] + [P(flags), P(gt)]
        return L.ssd_eval_match_voc(P(score), P(ins["cls"]), P(ins["box"]), P(ins["keep"]), B, A, P(ins["gt_cls"]),
                                    P(ins["gt_box"]), P(gt_off), P(ins["gt_difficult"]), ctypes.c_double(thr), md, *o, stream())

    def apv(C=1, year=7, flags=fl, pts=dp(M.VOC_RECALL_POINTS), out=ap):
        return L.ssd_eval_ap_voc(P(flags), P(seg), P(npos), C, year, pts, P(out), stream())

    def refusals():
        bad = [match(B=0), match(A=0), match(md=0), match(md=257), match(thr=0.0), match(thr=-0.5), match(thr=float("inf")),
               match(thr=float("nan")), match(score=None), match(gt_off=None), match(flags=None), match(gt=None),
               apv(C=0), apv(year=2007), apv(year=10), apv(year=0), apv(flags=None), apv(pts=None), apv(out=None)]
        assert bad == [_lib.SSD_ERR_VALUE] * len(bad), bad

    arena.run(refusals, [])                                           # no output listed: every one must keep its poison
    assert match() == 0 and apv() == 0 and apv(year=12) == 0
    torch.cuda.synchronize()


# ---- ssd_eval_ap_voc -----------------------------------------------------------------------------------------------------------
def ap_work():
    work = [("rows", V.ap_rows_case()), ("long", V.long_segment_case())]
    case = random_batch()
    ref = V.match_reference(case)
    live = np.arange(ref["cls"].shape[1])[None, :] < ref["n_det"][:, None]
    C = 8
    n_pos = np.zeros(C, np.int32)
    for g in case["gts"]:
        np.add.at(n_pos, g[0][~g[2]], 1)
    work.append(("matched", dict(rows=(ref["cls"][live], ref["score"][live], ref["flags"][live]), n_pos=n_pos, C=C)))
    return work


@pytest.mark.parametrize("year", ["07", "12"])
def test_eval_ap_voc_equals_the_host_stage(L, year):
    """AP within 1e-12 on: rows with whole chunks ignored, an empty segment with positives, a class whose rows are all ignored,
    a class without positives, an envelope that reaches across chunks; one segment longer than the kernel's slot table holds
    one chunk each (the path with several chunks per slot); the matched rows of the 200 random images"""
    for name, w in ap_work():
        C = w["C"]
        flags, seg = V.sorted_flags(w["rows"], C)
        N = len(flags)
        arena = strict.Arena("cuda", strict.Arena.bytes_for(N + 1, 256, 256, C * 8))
        a_fl = arena.put(T(flags if N else np.zeros(1, np.uint8)), "flags")
        a_seg, a_np = arena.put(T(seg), "seg_off"), arena.put(T(w["n_pos"]), "n_pos")
        ap = arena.out((C,), torch.float64, "ap")

        def call():
            status = L.ssd_eval_ap_voc(P(a_fl), P(a_seg), P(a_np), C, int(year), dp(M.VOC_RECALL_POINTS), P(ap), stream())
            assert status == 0, status

        arena.poison(False)
        call()
        torch.cuda.synchronize()
        got = ap.cpu().numpy().copy()
        table = M.voc_ap_from_rows(w["rows"], w["n_pos"], year)
        want = np.array([table.get(c, 0.0) for c in range(C)])
        print(name, year, "largest AP difference", float(np.abs(got - want).max()), "AP", want.round(4).tolist())
        assert np.abs(got - want).max() <= 1e-12 and want.max() > 0.05
        assert all(got[c] == 0.0 for c in range(C) if w["n_pos"][c] <= 0 or seg[c + 1] == seg[c])
        if name == "rows":
            assert got[2] == 0.0 and w["n_pos"][2] > 0 and seg[3] - seg[2] == 300       # all rows ignored
            assert got[1] == 0.0 and got[3] == 0.0 and 0 < got[5] <= 1.0
        if name == "long":
            assert seg[1] > 2048 * 256
        arena.run(call, [(ap, T(got))])                               # fully written and deterministic under both poisons


# ---- the Python surface --------------------------------------------------------------------------------------------------------
def test_ops_wrappers_and_the_accumulator_equal_voc_map(ops):
    from ssd_object_detection_amd.utils.device_map import DeviceVocAccumulator
    assert ops.eval_voc_max_dets() == 256
    case = random_batch()
    want = {y: M.voc_map(case["dets"], case["gts"], y, 0.5, case["max_dets"]) for y in ("07", "12")}
    accs = {y: DeviceVocAccumulator(7, case["max_dets"], "cuda", year=y) for y in ("07", "12")}
    assert all(a.protocol == "voc" for a in accs.values())
    ref = V.match_reference(case)
    for lo in range(0, 200, 64):                                      # four batches, the last one short
        idx = list(range(lo, min(lo + 64, 200)))
        d = {k: T(v).cuda() for k, v in V.dense_batch(_take(case, idx), 61, seed=lo).items()}
        args = [d[k] for k in ("score", "cls", "box", "keep", "gt_cls", "gt_box", "gt_off")]
        r = ops.eval_match_voc(*args, case["max_dets"], d["gt_difficult"], 0.5)
        assert r._fields == ("n_det", "score", "cls", "box", "flags", "gt")
        for got, key in zip(r, ("n_det", "score", "cls", "box", "flags", "gt")):
            assert np.array_equal(got.cpu().numpy(), ref[key][idx]), key
        for a in accs.values():
            a.add(*args, d["gt_difficult"])
    for y, a in accs.items():
        got = a.result()
        print(y, got["mAP"], want[y]["mAP"])
        assert set(got) == {"mAP", "per_class", "n_pos"} and got["n_pos"] == want[y]["n_pos"]
        assert set(got["per_class"]) == set(want[y]["per_class"])
        assert abs(got["mAP"] - want[y]["mAP"]) <= 1e-12
        for c, v in want[y]["per_class"].items():
            assert abs(got["per_class"][c] - v) <= 1e-12
        dets = a.detections()
        assert len(dets) == 200 and all(len(x[0]) == n for x, n in zip(dets, ref["n_det"]))
    assert want["07"]["mAP"] != want["12"]["mAP"]
    assert DeviceVocAccumulator(7, 20, "cuda").result() == dict(mAP=0.0, per_class={}, n_pos={})
    # without flags no box is difficult
    d = {k: T(v).cuda() for k, v in V.dense_batch(_take(case, [1, 2, 3]), 61).items()}
    args = [d[k] for k in ("score", "cls", "box", "keep", "gt_cls", "gt_box", "gt_off")]
    assert int((ops.eval_match_voc(*args, 20).flags & 2).sum()) == 0 and int((ops.eval_match_voc(*args, 20, d["gt_difficult"]).flags & 2).sum()) > 0
    for bad in (dict(max_dets=0), dict(max_dets=257), dict(year="2007"), dict(iou_thresh=0.0), dict(iou_thresh=float("nan"))):
        with pytest.raises(ValueError):
            DeviceVocAccumulator(7, **dict(dict(max_dets=100), **bad))
    with pytest.raises(ValueError):
        ops.eval_match_voc(*args, 257)
    with pytest.raises(ValueError):
        ops.eval_match_voc(*args, 100, None, -1.0)
    with pytest.raises(ValueError):
        ops.eval_ap_voc(torch.zeros(4, dtype=torch.uint8, device="cuda"), torch.tensor([0, 4], dtype=torch.int32, device="cuda"),
                        torch.tensor([2], dtype=torch.int32, device="cuda"), "10")
