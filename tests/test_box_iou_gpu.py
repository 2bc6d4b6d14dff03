"""GPU: the IoU box terms (GIoU / DIoU / CIoU) of the MultiBox and softmax focal losses -- the four _box entries of
include/ssd_hip.h -- against the float64 oracle of tests/box_iou_oracle.py on the inputs of tests/box_iou_cases.py, kind 0
against the entries without _box bit for bit, the strict harness (tests/strict.py), the rows forms against the dense ones bit
for bit, statuses 1 and 3, reproducibility and the absence of host synchronisation.

Bounds: the scalars within 1e-4 relative (the header's rule for the loss kernels), P and N exact, f32 dloc per anchor within
1e-4 of the anchor's largest reference component (tests/test_box_iou_cpu.py shows that a float32 evaluation meets a third of it),
bf16 adds 4e-3 |ref| per element (tests/test_multibox_gpu.py's figure), dconf bit-identical to the smooth-L1 call's.

The inputs here keep away from the losses' kinks (box_iou_cases.near_kink), so the header's tie rule -- strict comparisons, the
clamp's zero gradient, the guard at pred == target -- is not what these tests run: tests/test_box_iou_edges_gpu.py meets the
kinks on purpose, on the inputs of tests/box_iou_edge_cases.py."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import box_iou_cases as K                                                              # noqa: E402
from tests import box_iou_oracle as O                                                             # noqa: E402
from tests import strict                                                                          # noqa: E402
from tests.test_softmax_focal_gpu import SSD300, SSD512, heads_case                               # noqa: E402

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
LOSSES = ("multibox", "softmax_focal")
RATIO, GAMMA, ALPHA = 3, 2.0, 0.25


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def upload(c, dtype):
    return (torch.from_numpy(c["conf"]).cuda().to(dtype), torch.from_numpy(c["loc"]).cuda().to(dtype),
            torch.from_numpy(c["gt_cls"]).cuda(), torch.from_numpy(c["gt_loc"]).cuda(), torch.from_numpy(c["gt_mask"]).cuda())


def dense(ops, loss, inp, lw=1.0, gs=1.0, ws=None, box="smooth_l1", priors=None):
    if loss == "multibox":
        return ops.multibox_loss(*inp, RATIO, lw, gs, ws, box=box, priors=priors)
    return ops.softmax_focal_loss(*inp, GAMMA, ALPHA, lw, gs, ws, box=box, priors=priors)


def rows(ops, loss, inp, hgb, lw=1.0, gs=1.0, ws=None, box="smooth_l1", priors=None):
    if loss == "multibox":
        return ops.multibox_loss_heads(*inp, hgb, RATIO, lw, gs, ws, box=box, priors=priors)
    return ops.softmax_focal_loss_heads(*inp, hgb, GAMMA, ALPHA, lw, gs, ws, box=box, priors=priors)


def oracle(loss, kind, c, gs):
    if loss == "multibox":
        return O.multibox_loss(kind, c["priors"], c["gt_cls"], c["gt_loc"], c["gt_mask"], c["loc"], c["conf"], RATIO, K.LOC_WEIGHT, gs)
    return O.softmax_focal_loss(kind, c["priors"], c["gt_cls"], c["gt_loc"], c["gt_mask"], c["loc"], c["conf"], GAMMA, ALPHA,
                                K.LOC_WEIGHT, gs)


# ---------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", K.SHAPES, ids=str)
@pytest.mark.parametrize("loss", LOSSES)
def test_dense_against_the_oracle(ops, loss, shape, dtype):
    """three IoU kinds x two grad scales on one set of inputs: scalars, counts, dloc per anchor, exact zeros off the positives,
    dconf bit for bit the smooth-L1 call's; both shapes hold three or more row blocks with a ragged last one, a positive in the
    last row and an image without positives"""
    bf16 = dtype == BF
    c = K.make_case(*shape)
    inp = upload(c, dtype)
    assert np.array_equal(inp[0].float().cpu().numpy(), c["conf"]) and np.array_equal(inp[1].float().cpu().numpy(), c["loc"])
    pri = torch.from_numpy(c["priors"]).cuda()
    mask = c["gt_mask"].astype(bool)
    worst = 0.0
    for gs in K.GRAD_SCALES:
        out0, dconf0, _ = dense(ops, loss, inp, K.LOC_WEIGHT, gs)
        for kind in O.KINDS:
            where = (loss, shape, kind, gs)
            ref = oracle(loss, kind, c, gs)
            assert ref["status"] == 0
            out8, dconf, dloc = dense(ops, loss, inp, K.LOC_WEIGHT, gs, box=kind, priors=pri)
            o = out8.cpu().numpy().astype(np.float64)
            print(where, "out8", o.tolist(), "oracle", [ref[k] for k in ("loc", "pos", "neg", "total", "num_pos", "num_neg")])
            for i, key in enumerate(("loc", "pos", "neg", "total")):
                assert abs(o[i] - ref[key]) <= 1e-4 * abs(ref[key]), (where, key, o[i], ref[key])
            assert o[4] == ref["num_pos"] and o[5] == ref["num_neg"] and o[7] == 0.0, (where, o)
            assert torch.equal(out8[1:3].view(I32), out0[1:3].view(I32)) and torch.equal(out8[4:].view(I32), out0[4:].view(I32))
            assert torch.equal(bits(dconf), bits(dconf0)), where
            got = dloc.float().cpu().numpy().astype(np.float64)
            err, bound = np.abs(got - ref["dbox"]), K.dloc_bound(ref["dbox"], bf16)
            assert (got[~mask] == 0).all() and not np.signbit(got[~mask]).any(), where
            ratio = (err[mask] / bound[mask]).max()
            worst = max(worst, float(ratio))
            print(where, "dloc error / bound", float(ratio))
            assert ratio <= 1.0, (where, float(ratio))
            assert (np.abs(ref["dbox"][mask]).max(axis=-1) > 0).all()
    print(loss, shape, "bf16" if bf16 else "f32", "worst dloc error / bound", worst)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_both_losses_share_dloc_bit_for_bit(ops, dtype):
    c = K.make_case(*K.SHAPES[1])
    inp = upload(c, dtype)
    pri = torch.from_numpy(c["priors"]).cuda()
    for kind in O.KINDS:
        a = dense(ops, "multibox", inp, K.LOC_WEIGHT, 0.25, box=kind, priors=pri)
        b = dense(ops, "softmax_focal", inp, K.LOC_WEIGHT, 0.25, box=kind, priors=pri)
        assert torch.equal(bits(a[2]), bits(b[2])) and bool(a[2].any()), kind
        assert torch.equal(a[0][0].view(I32), b[0][0].view(I32)), kind       # L_loc: the same fixed-order f64 sum


# ---------------------------------------------------------------------------------------------------- kind 0
def raw_calls(L, loss, old):
    """(dense, rows) callables on raw pointers: the entries without _box (old) or with it"""
    def f(form):
        name = "ssd_%s_loss%s_fwd_bwd%s" % (loss, "" if old else "_box", "_heads" if form == "rows" else "")
        return getattr(L, name)
    mid = (RATIO,) if loss == "multibox" else (GAMMA, ALPHA)

    def dense_(inp, dt, B, A, C, lw, gs, out8, dconf, dloc, ws, ws_bytes, *box):
        conf, loc, cls, gloc, mask = inp
        return f("dense")(ptr(conf), ptr(loc), dt, ptr(cls), ptr(gloc), ptr(mask), B, A, C, *mid, lw, gs, ptr(out8), ptr(dconf),
                          ptr(dloc), ptr(ws), ws_bytes, stream(), *box)

    def rows_(inp, B, A, C, lw, gs, out8, hgb, ws, ws_bytes, *box):
        conf, loc, cls, gloc, mask = inp
        return f("rows")(ptr(conf), ptr(loc), 1, ptr(cls), ptr(gloc), ptr(mask), B, A, C, *mid, lw, gs, ptr(out8),
                         ctypes.byref(hgb.c), ptr(ws), ws_bytes, stream(), *box)
    return dense_, rows_


@pytest.mark.parametrize("loss", LOSSES)
def test_kind_0_through_the_new_entries_is_the_old_entries(ops, lib, loss):
    """out8, dconf, dloc and the rows, bit for bit, with and without a priors pointer (kind 0 does not read it)"""
    L = lib.lib()
    old_d, old_r = raw_calls(L, loss, True)
    new_d, new_r = raw_calls(L, loss, False)
    c = K.make_case(*K.SHAPES[1])
    B, A, C = K.SHAPES[1]
    pri = torch.from_numpy(c["priors"]).cuda()
    ws = torch.empty((1 << 20,), dtype=torch.uint8, device="cuda")
    for dtype in (F32, BF):
        inp = upload(c, dtype)
        dt = 0 if dtype == F32 else 1
        res = []
        for call, box in ((old_d, ()), (new_d, (0, None)), (new_d, (0, ptr(pri)))):
            out8 = torch.full((8,), -7.0, device="cuda")
            dconf, dloc = torch.full_like(inp[0], 3.0), torch.full_like(inp[1], 3.0)
            ws.fill_(0x5a)
            assert call(inp, dt, B, A, C, 0.5, 0.25, out8, dconf, dloc, ws, ws.numel(), *box) == 0
            res.append((out8, dconf, dloc))
        for other in res[1:]:
            for x, y in zip(res[0], other):
                assert torch.equal(bits(x), bits(y))
        assert float(res[0][0][7]) == 0.0 and bool(res[0][2].any())
    # the rows form, on the SSD300 geometry
    inp, hgb, (hw, per, npad, A) = heads_case(ops, SSD300, 2, 21)
    pri = torch.from_numpy(K.random_priors(np.random.default_rng(1), A)).cuda()
    res = []
    for call, box in ((old_r, ()), (new_r, (0, None)), (new_r, (0, ptr(pri)))):
        out8 = torch.full((8,), -7.0, device="cuda")
        for t in hgb.rows:
            t.view(torch.int16).fill_(0x7f7f)
        ws.fill_(0x5a)
        assert call(inp, 2, A, 21, 0.5, 0.25, out8, hgb, ws, ws.numel(), *box) == 0
        res.append([out8] + [t.clone() for t in hgb.rows + hgb.row_of_pixel + hgb.pixel_of_row] + [hgb.count.clone()])
    for other in res[1:]:
        for x, y in zip(res[0], other):
            assert torch.equal(bits(x), bits(y))
    assert float(res[0][0][7]) == 0.0


# ---------------------------------------------------------------------------------------------------- the strict harness
@pytest.mark.parametrize("loss,dtype,kind", [("multibox", F32, "giou"), ("multibox", BF, "ciou"), ("softmax_focal", F32, "diou"),
                                             ("softmax_focal", BF, "ciou"), ("softmax_focal", F32, "giou"), ("multibox", BF, "diou")],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_under_the_strict_harness(lib, ops, loss, dtype, kind):
    """the plain call of test_dense_against_the_oracle (checked against the oracle there), repeated under both poisons with
    guard bands round every tensor and a workspace of exactly the queried size: every output element is written, nothing outside
    is, the inputs and the priors keep their bits, no unwritten workspace word reaches a result.  A refused call (unknown kind,
    NULL priors) leaves every poison in place."""
    L = lib.lib()
    shape = K.SHAPES[0]
    B, A, C = shape
    c = K.make_case(*shape)
    plain = upload(c, dtype)
    pri_plain = torch.from_numpy(c["priors"]).cuda()
    gs = 0.25
    want8, want_dconf, want_dloc = dense(ops, loss, plain, K.LOC_WEIGHT, gs, box=kind, priors=pri_plain)
    assert float(want8[7]) == 0.0
    names = ("conf", "loc", "gt_cls", "gt_loc", "gt_mask")
    nb = lambda t: t.numel() * t.element_size()
    ws_bytes = getattr(L, "ssd_%s_loss_workspace_bytes" % loss)(B, A, C)
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[nb(t) for t in plain], nb(pri_plain), 32, nb(want_dconf), nb(want_dloc), ws_bytes))
    inp = [a.put(t, k) for t, k in zip(plain, names)]
    pri = a.put(pri_plain, "priors")
    out8, dconf, dloc = a.out((8,), F32, "out8"), a.out((B, A, C), dtype, "dconf"), a.out((B, A, 4), dtype, "dloc")
    ws = a.workspace().get(ws_bytes, "cuda")
    call, _ = raw_calls(L, loss, False)
    dt = 0 if dtype == F32 else 1
    k = O.KINDS.index(kind) + 1

    def fn():
        assert call(inp, dt, B, A, C, K.LOC_WEIGHT, gs, out8, dconf, dloc, ws, ws_bytes, k, ptr(pri)) == 0
    a.run(fn, [(out8, want8), (dconf, want_dconf), (dloc, want_dloc)])

    def refused():
        assert call(inp, dt, B, A, C, K.LOC_WEIGHT, gs, out8, dconf, dloc, ws, ws_bytes, 4, ptr(pri)) == lib.SSD_ERR_VALUE
        assert call(inp, dt, B, A, C, K.LOC_WEIGHT, gs, out8, dconf, dloc, ws, ws_bytes, -1, ptr(pri)) == lib.SSD_ERR_VALUE
        assert call(inp, dt, B, A, C, K.LOC_WEIGHT, gs, out8, dconf, dloc, ws, ws_bytes, k, None) == lib.SSD_ERR_VALUE
    a.run(refused, [])                                                    # every output keeps its poison


def test_python_wrappers_refuse_before_anything_runs(ops):
    c = K.make_case(*K.SHAPES[0])
    inp = upload(c, F32)
    pri = torch.from_numpy(c["priors"]).cuda()
    for loss in LOSSES:
        with pytest.raises(ValueError):
            dense(ops, loss, inp, box="giou")                              # no priors
        with pytest.raises(ValueError):
            dense(ops, loss, inp, box="iou", priors=pri)
        with pytest.raises(ValueError):
            dense(ops, loss, inp, box="giou", priors=pri[:-1])             # not [A,4]
        with pytest.raises(ValueError):
            dense(ops, loss, inp, box="giou", priors=pri.float())
        with pytest.raises(ValueError):
            dense(ops, loss, inp, box="giou", priors=pri.cpu())
        a = dense(ops, loss, inp, box="diou", priors=ops.prior_set_from(pri))     # a PriorSet
        b = dense(ops, loss, inp, box="diou", priors=pri)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- the rows form
@pytest.mark.parametrize("geom,B", [(SSD300, 2), (SSD512, 1)], ids=["SSD300 B=2", "SSD512 B=1"])
@pytest.mark.parametrize("loss", LOSSES)
def test_rows_form_is_the_dense_form(ops, loss, geom, B):
    """scattered back, the rows are the dense bf16 call's gradients bit for bit, and out8 is equal, for every IoU kind"""
    C = 21
    inp, hgb, (hw, per, npad, A) = heads_case(ops, geom, B, C)
    pri = torch.from_numpy(K.random_priors(np.random.default_rng(2), A)).cuda()
    seen = []
    for kind in O.KINDS:
        for t in hgb.rows:
            t.view(torch.int16).fill_(0x7f7f)
        out_r = rows(ops, loss, inp, hgb, 1.0, 0.5, box=kind, priors=pri)
        out_d, dconf, dloc = dense(ops, loss, inp, 1.0, 0.5, box=kind, priors=pri)
        assert torch.equal(out_r.view(I32), out_d.view(I32)) and float(out_d[7]) == 0.0, kind
        sl, sc = hgb.dense(C)
        assert torch.equal(sl.view(torch.int16), dloc.view(torch.int16)) and torch.equal(sc.view(torch.int16), dconf.view(torch.int16)), kind
        assert bool(dloc.any())
        seen.append(dloc.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])     # the kinds are three different losses


# ---------------------------------------------------------------------------------------------------- statuses
@pytest.mark.parametrize("loss", LOSSES)
def test_status_1_and_3_in_both_forms(ops, loss):
    C = 21
    A = sum(h * n for h, n in zip(*SSD300))
    pri_ok = torch.from_numpy(K.random_priors(np.random.default_rng(4), A)).cuda()
    # no positives: status 1, scalars 0, exact zeros
    inp, hgb, (hw, per, npad, _) = heads_case(ops, SSD300, 2, C, no_pos=True)
    for kind in O.KINDS:
        out_r = rows(ops, loss, inp, hgb, box=kind, priors=pri_ok)
        out_d, dconf, dloc = dense(ops, loss, inp, box=kind, priors=pri_ok)
        for out in (out_r, out_d):
            o = out.cpu().tolist()
            assert o[0] == 0.0 and o[3] == 0.0 and o[4] == 0.0 and o[7] == 1.0, (kind, o)
        assert not bool(dloc.any()) and not bool(dconf.any())
        assert hgb.count.cpu().tolist()[:len(hw)] == [0] * len(hw)
    # a positive's offset that is not finite (prediction or target), reported also where the clamp would hide it
    for which, idx, value in ((1, (0, -1, 2), float("inf")), (1, (0, -1, 3), float("nan")), (1, (1, -1, 0), float("-inf")),
                              (3, (0, -1, 2), float("nan")), (3, (1, -1, 1), float("inf"))):
        inp, hgb, _ = heads_case(ops, SSD300, 2, C)
        inp[which][idx] = value
        for kind in O.KINDS:
            assert float(rows(ops, loss, inp, hgb, box=kind, priors=pri_ok)[7]) == 3.0, (which, idx, kind)
            assert float(dense(ops, loss, inp, box=kind, priors=pri_ok)[0][7]) == 3.0, (which, idx, kind)
    # a prior with zero width under a positive (the last anchor is one) -- and under a non-positive, which is not read
    inp, hgb, _ = heads_case(ops, SSD300, 2, C)
    mask = inp[4]
    free = int((mask == 0).all(dim=0).nonzero()[0])
    for column in (2, 3):
        pri = pri_ok.clone()
        pri[free, column] = 0.0
        assert float(dense(ops, loss, inp, box="giou", priors=pri)[0][7]) == 0.0
        pri[A - 1, column] = 0.0
        for kind in O.KINDS:
            assert float(rows(ops, loss, inp, hgb, box=kind, priors=pri)[7]) == 3.0, (column, kind)
            assert float(dense(ops, loss, inp, box=kind, priors=pri)[0][7]) == 3.0, (column, kind)
        pri[A - 1, column] = -0.25
        assert float(dense(ops, loss, inp, box="ciou", priors=pri)[0][7]) == 3.0


# ---------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("loss", LOSSES)
def test_reproducible_on_a_poisoned_workspace_and_no_host_sync(ops, loss):
    """two calls, each on a workspace filled with another byte pattern, give equal bits in both forms; neither form synchronises
    the host"""
    C = 81
    inp, hgb, (hw, per, npad, A) = heads_case(ops, SSD300, 2, C, seed=8)
    pri = torch.from_numpy(K.random_priors(np.random.default_rng(5), A)).cuda()
    ws = ops.MatchWorkspace()
    runs = []
    for fill in (0xff, 0x00):
        ws.get(1 << 20, inp[0].device).fill_(fill)
        out_d, dconf, dloc = dense(ops, loss, inp, ws=ws, box="ciou", priors=pri)
        ws.buf.fill_(fill)
        out_r = rows(ops, loss, inp, hgb, ws=ws, box="ciou", priors=pri)
        runs.append([out_d.clone(), dconf.clone(), dloc.clone(), out_r.clone()] + [t.clone() for t in hgb.rows])
    for x, y in zip(*runs):
        assert torch.equal(bits(x), bits(y))
    assert float(runs[0][0][7]) == 0.0
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        dense(ops, loss, inp, ws=ws, box="giou", priors=pri)
        rows(ops, loss, inp, hgb, ws=ws, box="diou", priors=pri)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
