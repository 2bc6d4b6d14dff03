"""GPU: the IoU box terms (csrc/boxterm.h through the four _box entries of include/ssd_hip.h) on the kinks that
tests/test_box_iou_gpu.py stays away from -- the inputs of tests/box_iou_edge_cases.py: corner ties, touching boxes, identical
boxes (CIoU's guard against 0 / 0), t2 / t3 on both sides of the clamp and at float32(W) itself, targets beyond the clamp --
against the float64 oracle of tests/box_iou_oracle.py, whose tie rule is the header's.  tests/test_box_iou_edges_cpu.py shows that
these inputs decide every comparison by the operands alone, and that a `>=` for a `>` in any one family of comparisons would
leave the bound below by more than a hundredfold on eight rows or more.

Bounds: status 0, P and N exact, the scalars within 1e-4 relative (an L_loc of exactly 0 is exactly 0), dloc per positive within
1e-4 * scale * max(the row's largest reference component, 1) with scale = grad_scale * loc_weight / P (the floor:
box_iou_edge_cases.dloc_bound_floored), bf16 adds 4e-3 |ref|; where the oracle's component is exactly 0 the kernel's is 0 (-0.0
allowed on a positive, +0 off the positives); dconf bit-identical to the smooth-L1 call's.

Measured on an MI355X, the kernel as it stood (csrc/boxterm.h unchanged: it follows the rule on every class of row), worst dloc
error / bound over the kinds and grad scales, the same for both losses and both shapes:
    dense f32 0.0013    dense bf16 0.897    SSD300 rows (bf16) 0.840 giou, 0.812 diou, 0.815 ciou
The bf16 figures are the output's own rounding and no more: 0.897 is what rounding the float64 oracle to bf16 costs on that
element (a value just above a power of two loses 2^-8 of itself, against the bound's 4e-3).  The all-identical batch gave L_loc
== 0.0, status 0 and exact zeros for GIoU in both dtypes."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import box_iou_cases as K                                                              # noqa: E402
from tests import box_iou_edge_cases as E                                                         # noqa: E402
from tests import box_iou_oracle as O                                                             # noqa: E402
from tests import strict                                                                          # noqa: E402
from tests.test_box_iou_gpu import BF, F32, I32, LOSSES, RATIO, GAMMA, ALPHA, ptr, bits, upload, dense, rows, raw_calls  # noqa: E402
from tests.test_softmax_focal_gpu import SSD300, heads_case                                       # noqa: E402

LW = E.LOC_WEIGHT


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib


def oracle(loss, kind, c, gs, lw=LW):
    if loss == "multibox":
        return O.multibox_loss(kind, c["priors"], c["gt_cls"], c["gt_loc"], c["gt_mask"], c["loc"], c["conf"], RATIO, lw, gs)
    return O.softmax_focal_loss(kind, c["priors"], c["gt_cls"], c["gt_loc"], c["gt_mask"], c["loc"], c["conf"], GAMMA, ALPHA, lw, gs)


def hold_to_oracle(where, c, ref, gs, out8, dloc, bf16, lw=LW):
    """one call's out8 and dloc against the oracle's dict; returns the worst dloc error / bound"""
    mask = c["gt_mask"].astype(bool)
    assert ref["status"] == 0
    o = out8.cpu().numpy().astype(np.float64)
    print(where, "out8", o.tolist(), "oracle", [ref[k] for k in ("loc", "pos", "neg", "total", "num_pos", "num_neg")])
    assert o[7] == 0.0, (where, o)
    for i, key in enumerate(("loc", "pos", "neg", "total")):
        assert abs(o[i] - ref[key]) <= 1e-4 * abs(ref[key]), (where, key, o[i], ref[key])
    assert o[4] == ref["num_pos"] == mask.sum() and o[5] == ref["num_neg"], (where, o)
    got = dloc.float().cpu().numpy().astype(np.float64)
    want = ref["dbox"]
    assert np.isfinite(got).all(), where
    assert (got[~mask] == 0).all() and not np.signbit(got[~mask]).any(), where
    zero = want == 0
    assert zero[mask].any() and (got[zero] == 0).all(), (where, "a rule-zero is not zero", np.argwhere(zero & (got != 0))[:8].tolist())
    s = gs * lw / float(mask.sum())
    err, bound = np.abs(got - want), E.dloc_bound_floored(want, s, bf16)
    ratio = float((err[mask] / bound[mask]).max())
    print(where, "dloc error / bound", ratio)
    assert ratio <= 1.0, (where, ratio, np.argwhere((err > bound) & mask[..., None])[:8].tolist())
    return ratio


# ---------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
@pytest.mark.parametrize("loss", LOSSES)
def test_dense_against_the_oracle(ops, loss, shape, dtype):
    """three kinds x two grad scales on the edge case (the f32 call's also holds t2 / t3 == +-float32(W) and its neighbour)"""
    bf16 = dtype == BF
    c = E.make_case(*shape, not bf16)
    inp = upload(c, dtype)
    assert np.array_equal(inp[0].float().cpu().numpy(), c["conf"]) and np.array_equal(inp[1].float().cpu().numpy(), c["loc"])
    pri = torch.from_numpy(c["priors"]).cuda()
    worst = 0.0
    for gs in E.GRAD_SCALES:
        out0, dconf0, _ = dense(ops, loss, inp, LW, gs)
        for kind in O.KINDS:
            where = (loss, shape, kind, gs)
            out8, dconf, dloc = dense(ops, loss, inp, LW, gs, box=kind, priors=pri)
            worst = max(worst, hold_to_oracle(where, c, oracle(loss, kind, c, gs), gs, out8, dloc, bf16))
            assert torch.equal(out8[1:3].view(I32), out0[1:3].view(I32)) and torch.equal(out8[4:].view(I32), out0[4:].view(I32))
            assert torch.equal(bits(dconf), bits(dconf0)), where
    print(loss, shape, "bf16" if bf16 else "f32", "worst dloc error / bound", worst)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("loss", LOSSES)
def test_all_identical_batch(ops, loss, dtype):
    """every positive predicts its target, log-sizes 0: L_loc is exactly 0 and the status 0 (CIoU's alpha is 0 / 0 without its
    guard), GIoU's dloc is all zeros, DIoU's and CIoU's is (0, 0, s, s)"""
    bf16 = dtype == BF
    for shape in E.SHAPES:
        c = E.identical_case(*shape)
        inp = upload(c, dtype)
        pri = torch.from_numpy(c["priors"]).cuda()
        mask = c["gt_mask"].astype(bool)
        for gs in E.GRAD_SCALES:
            s = E.scale_of(c, gs)
            for kind in O.KINDS:
                where = (loss, shape, kind, gs, "identical")
                out8, dconf, dloc = dense(ops, loss, inp, LW, gs, box=kind, priors=pri)
                assert float(out8[0]) == 0.0 and float(out8[7]) == 0.0, (where, out8.cpu().tolist())
                hold_to_oracle(where, c, oracle(loss, kind, c, gs), gs, out8, dloc, bf16)
                got = dloc.float().cpu().numpy().astype(np.float64)
                want = np.zeros(4) if kind == "giou" else np.array([0.0, 0.0, s, s])
                assert (got[..., :2] == 0).all() and (got[~mask] == 0).all(), where
                if kind == "giou":
                    assert (got == 0).all(), where
                else:
                    bound = E.dloc_bound_floored(np.broadcast_to(want, got[mask].shape), s, bf16)
                    assert (np.abs(got[mask] - want) <= bound).all(), (where, np.abs(got[mask] - want).max() / s)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_both_losses_share_dloc_bit_for_bit_on_the_edges(ops, dtype):
    c = E.make_case(*E.SHAPES[1], dtype == F32)
    inp = upload(c, dtype)
    pri = torch.from_numpy(c["priors"]).cuda()
    for kind in O.KINDS:
        a = dense(ops, "multibox", inp, LW, 0.25, box=kind, priors=pri)
        b = dense(ops, "softmax_focal", inp, LW, 0.25, box=kind, priors=pri)
        assert torch.equal(bits(a[2]), bits(b[2])) and bool(a[2].any()), kind
        assert torch.equal(a[0][0].view(I32), b[0][0].view(I32)) and float(a[0][7]) == 0.0 == float(b[0][7]), kind


# ---------------------------------------------------------------------------------------------------- the rows form
@pytest.mark.parametrize("loss", LOSSES)
def test_rows_form_on_the_edges(ops, loss):
    """the SSD300 geometry with every positive an edge row (made per anchor, since the images share the priors; the designed
    rows first and last, so the last anchor holds one) under dyadic prior sizes: the scattered rows are the dense bf16 call's
    gradients bit for bit and out8 is equal, for every kind, and that dense call meets the oracle"""
    C, gs, lw = 21, 0.5, 1.0
    inp, hgb, (hw, per, npad, A) = heads_case(ops, SSD300, 2, C)
    mask = inp[4].cpu().numpy().astype(bool)
    b, a = np.nonzero(mask)
    ua, inv = np.unique(a, return_inverse=True)
    n, nd = len(ua), E.n_designed()
    assert 200 <= n and ua[-1] == A - 1 and mask[:, A - 1].all()
    t, g = E.edge_rows(n, np.concatenate([np.arange(nd), np.arange(n - nd, n)]), 5, False)
    rng = np.random.default_rng(6)
    priors = K.random_priors(rng, A)
    priors[ua, 2:] = E.dyadic_sizes(rng, n)
    loc, gloc = inp[1].cpu().float().numpy(), inp[3].cpu().numpy()
    loc[b, a], gloc[b, a] = t[inv], g[inv]
    inp[1], inp[3] = torch.from_numpy(loc).to(BF).cuda(), torch.from_numpy(gloc).cuda()
    c = dict(priors=priors, conf=inp[0].float().cpu().numpy(), loc=loc, gt_loc=gloc, gt_cls=inp[2].cpu().numpy(),
             gt_mask=mask.astype(np.uint8))
    assert np.array_equal(inp[1].float().cpu().numpy(), loc)
    counts = {k: int(v.sum()) for k, v in E.classes(c).items()}
    print(loss, "positives", len(b), "classes", counts)
    assert min(counts.values()) >= 8, counts
    pri = torch.from_numpy(priors).cuda()
    for kind in O.KINDS:
        for x in hgb.rows:
            x.view(torch.int16).fill_(0x7f7f)
        out_r = rows(ops, loss, inp, hgb, lw, gs, box=kind, priors=pri)
        out_d, dconf, dloc = dense(ops, loss, inp, lw, gs, box=kind, priors=pri)
        assert torch.equal(out_r.view(I32), out_d.view(I32)) and float(out_d[7]) == 0.0, kind
        sl, sc = hgb.dense(C)
        assert torch.equal(sl.view(torch.int16), dloc.view(torch.int16)) and torch.equal(sc.view(torch.int16), dconf.view(torch.int16)), kind
        hold_to_oracle((loss, "SSD300 rows", kind, gs), c, oracle(loss, kind, c, gs, lw), gs, out_d, dloc, True, lw)


# ---------------------------------------------------------------------------------------------------- the strict harness
@pytest.mark.parametrize("loss,dtype,kind", [("multibox", F32, "giou"), ("softmax_focal", BF, "giou"), ("softmax_focal", F32, "diou"),
                                             ("multibox", BF, "diou"), ("multibox", F32, "ciou"), ("softmax_focal", BF, "ciou")],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_under_the_strict_harness(lib, ops, loss, dtype, kind):
    """inside strict.Arena -- guard bands round every tensor, a workspace of exactly the queried size: one run, held to the oracle's
    bounds, is the reference of Arena.run: every output element written, nothing outside, inputs and priors unchanged, the same
    bits under the other poison"""
    L = lib.lib()
    shape = E.SHAPES[0]
    B, A, C = shape
    bf16 = dtype == BF
    c = E.make_case(*shape, not bf16)
    plain = upload(c, dtype)
    pri_plain = torch.from_numpy(c["priors"]).cuda()
    gs = 0.25
    names = ("conf", "loc", "gt_cls", "gt_loc", "gt_mask")
    nb = lambda t: t.numel() * t.element_size()
    ws_bytes = getattr(L, "ssd_%s_loss_workspace_bytes" % loss)(B, A, C)
    size = torch.empty((), dtype=dtype).element_size()
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[nb(t) for t in plain], nb(pri_plain), 32, B * A * C * size, B * A * 4 * size, ws_bytes))
    inp = [a.put(t, k) for t, k in zip(plain, names)]
    pri = a.put(pri_plain, "priors")
    out8, dconf, dloc = a.out((8,), F32, "out8"), a.out((B, A, C), dtype, "dconf"), a.out((B, A, 4), dtype, "dloc")
    ws = a.workspace().get(ws_bytes, "cuda")
    call, _ = raw_calls(L, loss, False)
    k = O.KINDS.index(kind) + 1

    def fn():
        assert call(inp, 1 if bf16 else 0, B, A, C, LW, gs, out8, dconf, dloc, ws, ws_bytes, k, ptr(pri)) == 0
    a.poison(False)
    fn()
    torch.cuda.synchronize()
    got = [x.detach().clone() for x in (out8, dconf, dloc)]
    hold_to_oracle((loss, shape, kind, gs, "arena"), c, oracle(loss, kind, c, gs), gs, got[0], got[2], bf16)
    assert torch.equal(bits(got[1]), bits(dense(ops, loss, plain, LW, gs)[1]))          # dconf: the smooth-L1 call's
    a.run(fn, list(zip((out8, dconf, dloc), got)))
