"""GPU: the softmax focal loss (ssd_softmax_focal_loss_fwd_bwd and its rows form) against the float64 oracle of
tests/softmax_focal_oracle.py on the inputs of tests/softmax_focal_cases.py, an exact case under the strict harness
(tests/strict.py) in both forms, the rows form against the dense one bit for bit, rows with logit gaps up to 120 over the edges
of gamma and alpha, reproducibility and the absence of host synchronisation.

Bounds: the scalars within 1e-4 relative (the header's rule for the loss kernels), P and N exact, f32 dconf elementwise within
1e-4 |ref| + 2^-100 (tests/test_softmax_focal_cpu.py shows that a float32 evaluation of the stable form meets it and the naive
forms do not), bf16 adds 4e-3 |ref| (tests/test_multibox_gpu.py's figure), dloc bit-identical to ops.multibox_loss's."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import softmax_focal_cases as K                                                       # noqa: E402
from tests import softmax_focal_oracle as F                                                      # noqa: E402
from tests import strict                                                                         # noqa: E402

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
SSD300 = ([38 * 38, 19 * 19, 10 * 10, 5 * 5, 3 * 3, 1], [4, 6, 6, 6, 4, 4])
SSD512 = ([64 * 64, 32 * 32, 16 * 16, 8 * 8, 4 * 4, 2 * 2, 1], [4, 6, 6, 6, 6, 4, 4])


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def upload(c, dtype):
    return (torch.from_numpy(c["conf"]).cuda().to(dtype), torch.from_numpy(c["loc"]).cuda().to(dtype),
            torch.from_numpy(c["gt_cls"]).cuda(), torch.from_numpy(c["gt_loc"]).cuda(), torch.from_numpy(c["gt_mask"]).cuda())


def check_scalars(out8, ref, where):
    for i, key in enumerate(("loc", "pos", "neg", "total")):
        assert abs(out8[i] - ref[key]) <= 1e-4 * abs(ref[key]), (where, key, out8[i], ref[key])
    assert out8[4] == ref["num_pos"] and out8[5] == ref["num_neg"] and out8[6] == 0.0 and out8[7] == ref["status"], (where, out8)


# ---------------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", K.SHAPES, ids=str)
def test_dense_against_the_oracle(ops, shape, dtype):
    """every (gamma, alpha, grad_scale) of the catalogue on one set of inputs: scalars, counts, dconf elementwise, dloc against
    MultiBox's bit for bit.  The shapes hold a ragged last row block, more than one block and the LDS bound (C = 303)."""
    bf16 = dtype == BF
    c = K.make_case(*shape, bf16=bf16)
    conf, loc, cls, gloc, mask = upload(c, dtype)
    assert np.array_equal(conf.float().cpu().numpy(), c["conf"])           # (bf16 inputs convert without rounding)
    cls_mb = torch.where(mask != 0, cls, torch.zeros_like(cls))
    worst = 0.0
    for gs in K.GRAD_SCALES:
        _, _, dloc_mb = ops.multibox_loss(conf, loc, cls_mb, gloc, mask, 3, 0.5, gs)
        for gamma in K.GAMMAS:
            for alpha in K.ALPHAS:
                where = (shape, gamma, alpha, gs)
                ref = F.softmax_focal_loss(c["gt_cls"], c["gt_loc"], c["gt_mask"], c["loc"], c["conf"], gamma, alpha, 0.5, gs)
                out8, dconf, dloc = ops.softmax_focal_loss(conf, loc, cls, gloc, mask, gamma, alpha, 0.5, gs)
                check_scalars(out8.cpu().numpy().astype(np.float64), ref, where)
                got = dconf.float().cpu().numpy().astype(np.float64)
                ratio = np.abs(got - ref["dcls"]) / K.dconf_bound(ref["dcls"], bf16)
                worst = max(worst, float(ratio.max()))
                assert ratio.max() <= 1.0, (where, np.unravel_index(ratio.argmax(), ratio.shape), ratio.max())
                assert torch.equal(dloc.view(-1).view(torch.int16 if bf16 else I32), dloc_mb.view(-1).view(torch.int16 if bf16 else I32)), where
                if c["B"] >= 2:                                           # the image without positives still has its gradient
                    assert bool((dloc[-1] == 0).all()) and bool((dconf[-1] != 0).any())
    print(shape, "bf16" if bf16 else "f32", "worst dconf error / bound", worst)


# ---------------------------------------------------------------------------------------------------- the exact case, strict
def exact_case(dtype, gs):
    """C = 4, all logits zero, gamma 0, alpha -1, P = 8 over B = 2, A = 150 (three row blocks, the last ragged): p = 1/4 on every
    row, so dconf = (1/4 - delta) / 8 * grad_scale exactly; offsets multiples of 1/4, so dloc is exact as well."""
    B, A, C = 2, 150, 4
    g = torch.Generator().manual_seed(5)
    conf = torch.zeros((B, A, C), dtype=dtype)
    loc = (torch.randint(-8, 9, (B, A, 4), generator=g).float() / 4).to(dtype)
    gloc = torch.randint(-8, 9, (B, A, 4), generator=g).float() / 4
    mask = torch.zeros((B, A), dtype=torch.uint8)
    pos = [(0, 0), (0, 1), (0, 127), (0, 128), (0, 149), (1, 0), (1, 106), (1, 149)]
    cls = torch.full((B, A), 0x7fffff, dtype=I32)
    for k, (b, a) in enumerate(pos):
        mask[b, a] = 1
        cls[b, a] = k % (C - 1)
    t = torch.where(mask != 0, cls, torch.full_like(cls, C - 1)).long()
    dconf = ((0.25 - torch.nn.functional.one_hot(t, C).float()) / 8 * gs).to(dtype)
    dloc = (mask[..., None].float() * (loc.float() - gloc).clamp(-1, 1) * (gs / 8)).to(dtype)
    assert torch.equal(dconf.float(), (0.25 - torch.nn.functional.one_hot(t, C).float()) / 8 * gs)      # exact in the dtype
    return dict(B=B, A=A, C=C, conf=conf, loc=loc, gt_cls=cls, gt_loc=gloc, gt_mask=mask, dconf=dconf, dloc=dloc, gs=gs)


@pytest.mark.parametrize("dtype,gs", [(F32, 1.0), (F32, 0.25), (BF, 1.0), (BF, 0.25)], ids=["f32", "f32 gs=0.25", "bf16", "bf16 gs=0.25"])
def test_exact_case_under_the_strict_harness(lib, ops, dtype, gs):
    """dconf and dloc bit for bit under both poisons with guard bands round every tensor and a workspace of exactly the queried
    size: every output element is written, nothing outside is, no input is modified, no unwritten workspace word is read
    (the two poisons would then disagree).  out8 must repeat a call outside the arena bit for bit; a refused call writes nothing."""
    L = lib.lib()
    r = exact_case(dtype, gs)
    B, A, C = r["B"], r["A"], r["C"]
    names = ("conf", "loc", "gt_cls", "gt_loc", "gt_mask")
    plain = [r[k].cuda() for k in names]
    want8, d0, l0 = ops.softmax_focal_loss(*plain, 0.0, -1.0, 1.0, gs)
    w = want8.cpu().numpy().astype(np.float64)
    ln4 = float(np.log(4.0))
    assert abs(w[1] - ln4) <= 1e-4 * ln4 and abs(w[2] - (B * A - 8) * ln4 / 8) <= 1e-4 * w[2]
    assert w[4] == 8 and w[5] == B * A - 8 and w[6] == 0 and w[7] == 0
    nb = lambda t: t.numel() * t.element_size()
    ws_bytes = L.ssd_softmax_focal_loss_workspace_bytes(B, A, C)
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[nb(r[k]) for k in names], 32, nb(r["dconf"]), nb(r["dloc"]), ws_bytes))
    conf, loc, cls, gloc, mask = [a.put(r[k], k) for k in names]
    out8, dconf, dloc = a.out((8,), F32, "out8"), a.out((B, A, C), dtype, "dconf"), a.out((B, A, 4), dtype, "dloc")
    ws = a.workspace().get(ws_bytes, "cuda")

    def call(gamma):
        return L.ssd_softmax_focal_loss_fwd_bwd(ptr(conf), ptr(loc), 0 if dtype == F32 else 1, ptr(cls), ptr(gloc), ptr(mask), B,
                                                A, C, gamma, -1.0, 1.0, gs, ptr(out8), ptr(dconf), ptr(dloc), ptr(ws), ws_bytes,
                                                stream())

    def fn():
        assert call(0.0) == 0
    a.run(fn, [(out8, want8), (dconf, r["dconf"]), (dloc, r["dloc"])])

    def refused():
        assert call(9.0) == lib.SSD_ERR_VALUE
    a.run(refused, [])                                                    # every output keeps its poison


# ---------------------------------------------------------------------------------------------------- the rows form
def heads_case(ops, geom, B, C=21, seed=3, no_pos=False, nan_at=None):
    hw, per = geom
    A = sum(h * n for h, n in zip(hw, per))
    g = torch.Generator().manual_seed(seed)
    conf = (3.0 * torch.randn((B, A, C), generator=g)).clamp(-16, 16).to(BF)
    loc = (1.5 * torch.randn((B, A, 4), generator=g)).to(BF)
    gloc = torch.randn((B, A, 4), generator=g)
    mask = (torch.rand((B, A), generator=g) < 0.02).to(torch.uint8)
    mask[:, -1] = 1                                                       # the 1x1 level's last anchor
    if no_pos:
        mask.zero_()
    cls = torch.randint(0, C - 1, (B, A), generator=g).to(I32)
    if nan_at is not None:
        conf[nan_at] = float("nan")
    npad = [(n * (4 + C) + 7) // 8 * 8 for n in per]
    hgb = ops.HeadGradBuffers(B, hw, per, npad)
    for t in hgb.rows:
        t.view(torch.int16).fill_(0x7f7f)                                 # a NaN pattern: every element must be overwritten
    for t in hgb.row_of_pixel + hgb.pixel_of_row:
        t.fill_(-7)
    hgb.count.fill_(-7)
    return [t.cuda() for t in (conf, loc, cls, gloc, mask)], hgb, (hw, per, npad, A)


def check_rows_form(ops, geom, B, C, seed=3):
    """the body of test_rows_form_is_the_dense_form on heads_case(geom, B, C, seed); returns the inputs and the dense call's
    (out8, dconf, dloc) for further checks of the same case"""
    inp, hgb, (hw, per, npad, A) = heads_case(ops, geom, B, C, seed)
    out_r = ops.softmax_focal_loss_heads(*inp, hgb, 2.0, 0.25, 1.0, 0.5)
    out_d, dconf, dloc = ops.softmax_focal_loss(*inp, 2.0, 0.25, 1.0, 0.5)
    assert torch.equal(out_r.view(I32), out_d.view(I32)) and float(out_d[7]) == 0.0
    counts = hgb.count.cpu().tolist()
    assert counts[:len(hw)] == [B * h for h in hw] and counts[len(hw):] == [-7] * (8 - len(hw))
    for l, h in enumerate(hw):
        ident = torch.arange(B * h, dtype=I32, device="cuda")
        assert torch.equal(hgb.row_of_pixel[l], ident) and torch.equal(hgb.pixel_of_row[l], ident)
        assert bool((hgb.rows[l][:, per[l] * (4 + C):] == 0).all())       # the padding
    sl, sc = hgb.dense(C)
    assert torch.equal(sl.view(torch.int16), dloc.view(torch.int16)) and torch.equal(sc.view(torch.int16), dconf.view(torch.int16))
    assert bool((dconf != 0).any(dim=2).all())                            # every anchor carries a gradient
    return inp, out_d, dconf, dloc


@pytest.mark.parametrize("geom,B", [(SSD300, 2), (SSD512, 1)], ids=["SSD300 B=2", "SSD512 B=1"])
def test_rows_form_is_the_dense_form(ops, geom, B):
    """every pixel is a row: identity maps, count == B * hw, channels in the head GEMM's order with zero padding; scattered back
    the rows are the dense bf16 call's gradients bit for bit, and out8 is the same"""
    check_rows_form(ops, geom, B, 21)


STRICT_LEVELS = ((25, 4, 0), (9, 4, 8), (2, 6, 0), (1, 2, 0))             # (hw, per_cell, npad above its minimum): 150 anchors


@pytest.mark.parametrize("gs", [1.0, 0.25], ids=["gs=1", "gs=0.25"])
def test_rows_form_exact_under_the_strict_harness(lib, ops, gs):
    """exact_case (B = 2, A = 150, C = 4, bf16) through ssd_softmax_focal_loss_fwd_bwd_heads into a strict.Arena: rows,
    row_of_pixel, pixel_of_row, count and out8 are arena outputs, the workspace is exactly the queried size.  Expected bit for
    bit: the rows are the dense exact gradients in the head order, the padding is zeros (level 1 has 8 padding channels although
    4 + C = 8), both maps are the identity, count[l] = B * hw[l] and count[4:8] is untouched.  A refused call (gamma = 9; the
    f32 dtype, which this form does not take) writes nothing."""
    from tests.test_loss_strict_gpu import HeadBuffers
    L = lib.lib()
    r = exact_case(BF, gs)
    B, A, C = r["B"], r["A"], r["C"]
    levels = [dict(hw=hw, n=n, npad=(n * (4 + C) + 7) // 8 * 8 + extra) for hw, n, extra in STRICT_LEVELS]
    assert sum(l["hw"] * l["n"] for l in levels) == A and levels[1]["npad"] == levels[1]["n"] * (4 + C) + 8
    names = ("conf", "loc", "gt_cls", "gt_loc", "gt_mask")
    want8, d0, l0 = ops.softmax_focal_loss(*[r[k].cuda() for k in names], 0.0, -1.0, 1.0, gs)
    assert torch.equal(d0.cpu(), r["dconf"]) and torch.equal(l0.cpu(), r["dloc"])       # (by value, as the arena compares)
    w = want8.cpu().numpy().astype(np.float64)
    ln4 = float(np.log(4.0))
    assert abs(w[1] - ln4) <= 1e-4 * ln4 and abs(w[2] - (B * A - 8) * ln4 / 8) <= 1e-4 * w[2] and w[4] == 8 and w[7] == 0
    # the expectation: anchor off_l + pixel * n + slot of image b lives in row b * hw + pixel of level l
    want_rows, off = [], 0
    for l in levels:
        hw, n, npad = l["hw"], l["n"], l["npad"]
        rows = torch.zeros((B, hw, npad), dtype=BF)
        rows[:, :, :n * 4] = r["dloc"][:, off:off + hw * n].reshape(B, hw, n * 4)
        rows[:, :, n * 4:n * (4 + C)] = r["dconf"][:, off:off + hw * n].reshape(B, hw, n * C)
        want_rows.append(rows.reshape(B * hw, npad))
        off += hw * n
    nb = lambda t: t.numel() * t.element_size()
    ws_bytes = L.ssd_softmax_focal_loss_heads_workspace_bytes(B, A, C)
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[nb(r[k]) for k in names], *HeadBuffers.bytes(dict(B=B, levels=levels)), ws_bytes))
    conf, loc, cls, gloc, mask = [a.put(r[k], k) for k in names]
    out8 = a.out((8,), F32, "out8")
    hb = HeadBuffers(a, lib, dict(B=B, levels=levels))
    ws = a.workspace().get(ws_bytes, "cuda")

    def call(gamma, dtype=1):
        return L.ssd_softmax_focal_loss_fwd_bwd_heads(ptr(conf), ptr(loc), dtype, ptr(cls), ptr(gloc), ptr(mask), B, A, C, gamma,
                                                      -1.0, 1.0, gs, ptr(out8), ctypes.byref(hb.c), ptr(ws), ws_bytes, stream())

    def fn():
        assert call(0.0) == 0
    counts = torch.zeros((8,), dtype=I32)
    counts[:len(levels)] = torch.tensor([B * l["hw"] for l in levels], dtype=I32)
    expect = [(out8, want8), (hb.count, counts, torch.arange(8) < len(levels))]
    for i, l in enumerate(levels):
        ident = torch.arange(B * l["hw"], dtype=I32)
        expect += [(hb.rop[i], ident), (hb.por[i], ident), (hb.rows[i], want_rows[i])]
    a.run(fn, expect)

    def refused():
        assert call(9.0) == lib.SSD_ERR_VALUE
        assert call(0.0, dtype=0) == lib.SSD_ERR_UNSUPPORTED
    a.run(refused, [])                                                    # every output keeps its poison


# ---------------------------------------------------------------------------------------------------- extreme rows
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", K.EXTREME_CLASSES)
def test_extreme_rows_stay_finite_and_inside_the_bound(ops, C, dtype):
    """K.extreme_case: logit gaps of 30 .. 120, the target above (q == 0 exactly at 104 and 120: the h = 1 branch the header
    promises to be finite) or below (p_t == 0, q == 1), over gamma 0 .. 8 (the bound) and alpha -1, 0, 0.25, 1.  Every scalar and
    gradient element is finite, the status is 0, the bounds are those of test_dense_against_the_oracle.  With alpha == 1 the
    background rows of dconf are exact zeros and L_neg == 0; with alpha == 0 the same holds for the positives and L_pos.
    The device's expf may flush the denormal e^-88 (and the e^-104 that numpy rounds up to the smallest one): the difference
    reaches dconf as less than 1e-37, which the bound's 2^-100 floor covers -- nothing is widened for it."""
    bf16 = dtype == BF
    c = K.extreme_case(C)
    conf, loc, cls, gloc, mask = upload(c, dtype)
    assert np.array_equal(conf.float().cpu().numpy(), c["conf"]) and np.array_equal(loc.float().cpu().numpy(), c["loc"])
    pos = c["gt_mask"].astype(bool)
    worst = 0.0
    for gamma in K.EXTREME_GAMMAS:
        for alpha in K.EXTREME_ALPHAS:
            where = (C, gamma, alpha)
            ref = F.softmax_focal_loss(c["gt_cls"], c["gt_loc"], c["gt_mask"], c["loc"], c["conf"], gamma, alpha, 0.5, 1.0)
            out8, dconf, dloc = ops.softmax_focal_loss(conf, loc, cls, gloc, mask, gamma, alpha, 0.5, 1.0)
            o = out8.cpu().numpy().astype(np.float64)
            got = dconf.float().cpu().numpy().astype(np.float64)
            assert np.isfinite(o).all() and np.isfinite(got).all() and bool(torch.isfinite(dloc.float()).all()), (where, o)
            check_scalars(o, ref, where)
            assert o[7] == 0.0 and ref["status"] == 0
            ratio = np.abs(got - ref["dcls"]) / K.dconf_bound(ref["dcls"], bf16)
            worst = max(worst, float(ratio.max()))
            assert ratio.max() <= 1.0, (where, np.unravel_index(ratio.argmax(), ratio.shape), ratio.max())
            if alpha == 1.0:
                assert not got[~pos].any() and o[2] == 0.0 and got[pos].any(), where
            if alpha == 0.0:
                assert not got[pos].any() and o[1] == 0.0 and got[~pos].any(), where
    print("C", C, "bf16" if bf16 else "f32", "extreme rows: worst dconf error / bound", worst)


def test_status_1_and_3_in_both_forms(ops):
    C = 21
    inp, hgb, (hw, per, npad, A) = heads_case(ops, SSD300, 2, C, no_pos=True)
    out_r = ops.softmax_focal_loss_heads(*inp, hgb)
    out_d, dconf, dloc = ops.softmax_focal_loss(*inp)
    for out in (out_r, out_d):
        assert out.cpu().tolist() == [0.0, 0.0, 0.0, 0.0, 0.0, 2.0 * A, 0.0, 1.0]
    assert not bool(dconf.any()) and not bool(dloc.any())                # exact zeros
    assert hgb.count.cpu().tolist()[:len(hw)] == [0] * len(hw)
    assert all(bool((t == -1).all()) for t in hgb.row_of_pixel)
    # a NaN logit: status 3 in both forms, also without positives (reported first)
    for no_pos in (False, True):
        inp, hgb, _ = heads_case(ops, SSD300, 2, C, no_pos=no_pos, nan_at=(1, 4000, 7))
        assert float(ops.softmax_focal_loss_heads(*inp, hgb)[7]) == 3.0
        assert float(ops.softmax_focal_loss(*inp)[0][7]) == 3.0
    # a positive's offset that is not finite
    inp, hgb, _ = heads_case(ops, SSD300, 2, C)
    inp[1][0, -1, 2] = float("inf")
    assert float(ops.softmax_focal_loss_heads(*inp, hgb)[7]) == 3.0 and float(ops.softmax_focal_loss(*inp)[0][7]) == 3.0


# ---------------------------------------------------------------------------------------------------- reproducibility
def test_reproducible_on_a_poisoned_workspace_and_no_host_sync(ops):
    """two calls, each on a workspace filled with another byte pattern, give equal bits in both forms (nothing is read before
    it is written, no atomics); and neither form synchronises the host"""
    C = 81
    inp, hgb, _ = heads_case(ops, SSD300, 2, C, seed=8)
    ws = ops.MatchWorkspace()
    runs = []
    for fill in (0xff, 0x00):
        ws.get(1 << 20, inp[0].device).fill_(fill)
        out_d, dconf, dloc = ops.softmax_focal_loss(*inp, ws=ws)
        ws.buf.fill_(fill)
        out_r = ops.softmax_focal_loss_heads(*inp, hgb, ws=ws)
        runs.append([out_d.clone(), dconf.clone(), dloc.clone(), out_r.clone()] + [t.clone() for t in hgb.rows])
    for x, y in zip(*runs):
        assert torch.equal(x.view(-1).view(torch.uint8), y.view(-1).view(torch.uint8))
    assert float(runs[0][0][7]) == 0.0
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.softmax_focal_loss(*inp, ws=ws)
        ops.softmax_focal_loss_heads(*inp, hgb, ws=ws)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
