"""GPU: the streaming row passes of the losses and of ssd_class_scores beyond one sweep of their persistent grid
(tests/persistent_cases.py: more than 768 * 128 rows), where the in-loop prefetch, the reuse of the LDS tile, the partial sums
at blk >= 768 and a ragged last block reached through the in-loop prefetch exist at all.

Two kinds of check.  Against the float64 oracles at full size, through the helpers of the entries' own tests and with their
bounds (nothing is restated here): tests/test_softmax_focal_gpu.py (check_scalars, dconf_bound, dloc against MultiBox's bit for
bit, the rows form's body), tests/test_multibox_gpu.py (check_against_oracle), tests/test_loss_gpu.py (run_case),
tests/test_detect_pairs_gpu.py (check_class_scores).  And position independence, bit for bit: a row's result depends on the row
and on P only, so a small case that passes its oracle check, tiled 128 times along the batch axis with grad_scale * 128
(grad_scale / P and the box scale keep their bits: 128 P0 is exact), must give the small call's gradients in every copy.
The seeds with a flip cap are checked against the oracle's own keys in tests/test_persistent_cases_cpu.py."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import persistent_cases as PC                                                         # noqa: E402
from tests import softmax_focal_cases as FK                                                      # noqa: E402
from tests import softmax_focal_oracle as F                                                      # noqa: E402
from tests import test_detect_pairs_gpu as DG                                                    # noqa: E402
from tests import test_loss_gpu as LG                                                            # noqa: E402
from tests import test_multibox_gpu as MG                                                        # noqa: E402
from tests import test_softmax_focal_gpu as FG                                                   # noqa: E402

BF, F32, I32, I16 = torch.bfloat16, torch.float32, torch.int32, torch.int16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def bits(t):
    return t.contiguous().view(-1).view(I16 if t.element_size() == 2 else I32)


# ---------------------------------------------------------------------------------------------------- softmax focal, dense
def focal_dense_vs_oracle(ops, c, dtype, gamma, alpha, gs, mb_view):
    """one (gamma, alpha, grad_scale) of tests/test_softmax_focal_gpu.py::test_dense_against_the_oracle on the case `c`.
    MultiBox bounds A by ssd_multibox_loss_max_anchors(); its dloc depends on the row and on P only, so it is handed the same
    rows as `mb_view` = (B', A') with B' A' == B A.  Returns the device outputs."""
    bf16 = dtype == BF
    B, A, C = c["B"], c["A"], c["C"]
    conf, loc, cls, gloc, mask = FG.upload(c, dtype)
    assert np.array_equal(conf.float().cpu().numpy(), c["conf"])          # (bf16 inputs convert without rounding)
    Bv, Av = mb_view
    assert Bv * Av == B * A
    cls_mb = torch.where(mask != 0, cls, torch.zeros_like(cls))
    _, _, dloc_mb = ops.multibox_loss(conf.view(Bv, Av, C), loc.view(Bv, Av, 4), cls_mb.view(Bv, Av), gloc.view(Bv, Av, 4),
                                      mask.view(Bv, Av), 3, 0.5, gs)
    ref = F.softmax_focal_loss(c["gt_cls"], c["gt_loc"], c["gt_mask"], c["loc"], c["conf"], gamma, alpha, 0.5, gs)
    out8, dconf, dloc = ops.softmax_focal_loss(conf, loc, cls, gloc, mask, gamma, alpha, 0.5, gs)
    where = ((B, A, C), gamma, alpha, gs)
    FG.check_scalars(out8.cpu().numpy().astype(np.float64), ref, where)
    got = dconf.float().cpu().numpy().astype(np.float64)
    ratio = np.abs(got - ref["dcls"]) / FK.dconf_bound(ref["dcls"], bf16)
    o = out8.cpu().numpy().astype(np.float64)
    print(where, "bf16" if bf16 else "f32", "error / bound: dconf", float(ratio.max()), "scalars",
          max(abs(o[i] - ref[k]) / (1e-4 * abs(ref[k])) for i, k in enumerate(("loc", "pos", "neg", "total"))))
    assert ratio.max() <= 1.0, (where, np.unravel_index(ratio.argmax(), ratio.shape), ratio.max())
    assert torch.equal(bits(dloc), bits(dloc_mb)), where
    if B >= 2:                                                            # the image without positives still has its gradient
        assert bool((dloc[-1] == 0).all()) and bool((dconf[-1] != 0).any())
    return out8, dconf, dloc


@DTYPES
@pytest.mark.parametrize("gamma,alpha,gs", [(2.0, 0.25, 1.0), (0.5, -1.0, 0.25)], ids=["g2 a.25", "g.5 a-1 gs.25"])
def test_focal_dense_three_trips_c81(ops, dtype, gamma, alpha, gs):
    """S81: 1 541 blocks, workgroups 0..4 make three trips, the 31-row last block is workgroup 4's third; k_sf_scalars' strided
    sum over the partials makes seven trips"""
    print(PC.describe("S81", PC.S81))
    B, A, C = PC.S81
    focal_dense_vs_oracle(ops, FK.make_case(B, A, C, bf16=dtype == BF), dtype, gamma, alpha, gs, (A, B))


def test_focal_dense_ten_trips_runtime_c(ops):
    """SGEN: 8 225 blocks (ten or eleven per workgroup) of the runtime-C instance, a 5-row last block, and 258 count chunks:
    sf_total_pos makes a second trip"""
    print(PC.describe("SGEN", PC.SGEN), "count chunks", PC.walk(PC.SGEN[1])["chunks"])
    B, A, C = PC.SGEN
    focal_dense_vs_oracle(ops, FK.make_case(B, A, C), F32, 2.0, 0.25, 1.0, (61, A // 61))


def test_focal_rows_form_c81_second_trip(ops):
    """SHEADS: the body of test_rows_form_is_the_dense_form with C = 81 at B = 12 (819 blocks: workgroups 0..50 make two trips,
    the last block has 80 rows), and the dense call of the same case against the oracle"""
    print(PC.describe("SHEADS", PC.SHEADS))
    B, A, C = PC.SHEADS
    inp, out_d, dconf, dloc = FG.check_rows_form(ops, FG.SSD300, B, C, seed=21)
    conf, loc, cls, gloc, mask = [t.cpu() for t in inp]
    assert tuple(conf.shape) == (B, A, C)
    ref = F.softmax_focal_loss(cls.numpy(), gloc.numpy(), mask.numpy(), loc.float().numpy(), conf.float().numpy(), 2.0, 0.25, 1.0, 0.5)
    FG.check_scalars(out_d.cpu().numpy().astype(np.float64), ref, "SHEADS rows")
    ratio = np.abs(dconf.float().cpu().numpy().astype(np.float64) - ref["dcls"]) / FK.dconf_bound(ref["dcls"], True)
    print("SHEADS bf16 error / bound: dconf", float(ratio.max()))
    assert ratio.max() <= 1.0, (np.unravel_index(ratio.argmax(), ratio.shape), ratio.max())
    _, _, dloc_mb = ops.multibox_loss(*inp, 3, 1.0, 0.5)
    assert torch.equal(bits(dloc), bits(dloc_mb))


# ---------------------------------------------------------------------------------------------------- MultiBox
@DTYPES
def test_multibox_against_oracle_second_trip(ops, dtype):
    """B = 12 of SSD300 (819 blocks) through check_against_oracle; P_b holds an image without positives and one whose 3 P_b
    exceeds its candidates"""
    print(PC.describe("SHEADS", PC.SHEADS))
    A = PC.SHEADS[1]
    out, ref = MG.check_against_oracle(ops, PC.multibox_hand(dtype))
    assert list(ref["neg_mask"].sum(1)) == [min(3 * p, A - p) for p in PC.MB_P_B]


def test_multibox_rows_form_second_trip(ops):
    """the exact 12-image case (tests/multibox_cases.heads_case, P = 512): multibox_loss_heads scattered back is the dense call
    bit for bit, and the dense call is the case's exact expectation"""
    r = PC.multibox_heads()
    B, A, C = r["B"], r["A"], r["C"]
    assert (B, A, C) == PC.SHEADS
    inp = MG.dev(r)
    hgb = ops.HeadGradBuffers(B, [h * w for h, w, _ in r["geom"]], [k for _, _, k in r["geom"]], list(r["npad"]))
    out_r = ops.multibox_loss_heads(*inp, hgb, r["ratio"], r["alpha"], r["grad_scale"])
    out_d, dconf, dloc = ops.multibox_loss(*inp, r["ratio"], r["alpha"], r["grad_scale"])
    assert torch.equal(out_r.view(I32), out_d.view(I32)) and torch.equal(out_d.cpu().view(I32), r["out8"].view(I32))
    assert hgb.count.cpu().tolist()[:len(r["levels"])] == [l["count"] for l in r["levels"]]
    sl, sc = hgb.dense(C)
    assert torch.equal(bits(sl), bits(dloc)) and torch.equal(bits(sc), bits(dconf))
    assert torch.equal(bits(dconf.cpu()), bits(r["dconf"])) and torch.equal(bits(dloc.cpu()), bits(r["dloc"]))


# ---------------------------------------------------------------------------------------------------- the reference loss
@pytest.mark.parametrize("C,dtype", sorted(PC.LOSS_SEED, key=str), ids=lambda v: str(v).replace("torch.", ""))
def test_reference_loss_second_trip(ops, C, dtype):
    """run_case at B = 12, A = 8732 (819 blocks): C = 81 in both dtypes and C = 21, the runtime-C instance; about 1 % positives"""
    print(PC.describe("SHEADS", PC.SHEADS[:2] + (C,)))
    r = PC.loss_full(C, dtype)
    LG.run_case(ops, *MG.dev(r))


# ---------------------------------------------------------------------------------------------------- ssd_class_scores
@DTYPES
@pytest.mark.parametrize("shape", [PC.SHEADS, PC.SCORES_SMALL], ids=str)
def test_class_scores_second_trip(ops, shape, dtype):
    print(PC.describe("scores", shape))
    B, A, C = shape
    DG.check_class_scores(ops, B, A, C, dtype, 300 if C == 81 else 64)


# ---------------------------------------------------------------------------------------------------- position independence
TILE_PARAMS = pytest.mark.parametrize("C,dtype", [(81, BF), (21, F32)], ids=["C=81 bf16", "C=21 f32"])


def check_tiling(small, big):
    """(out8, dconf, dloc) of the small call and of its TILE_K-fold tiling: every copy's gradients bit for bit, the counts times
    TILE_K, the loss scalars within the entries' 1e-4 relative (the f64 sums are taken in another order), status 0"""
    k = PC.TILE_K
    print(PC.describe("STILE", PC.STILE + (small[1].shape[2],)))
    for name, s, b in (("dconf", small[1], big[1]), ("dloc", small[2], big[2])):
        assert b.shape[0] == k * s.shape[0] and b.shape[1:] == s.shape[1:]
        same = bits(b).view(k, -1) == bits(s).view(1, -1)
        assert bool(same.all()), (name, "copies that differ:", (~same.all(1)).nonzero().view(-1).tolist()[:8])
    o0, o1 = small[0].cpu().numpy().astype(np.float64), big[0].cpu().numpy().astype(np.float64)
    assert o0[7] == 0.0 and o1[7] == 0.0
    assert o1[4] == k * o0[4] and o1[5] == k * o0[5] and o1[6] == o0[6], (o0, o1)
    for i in range(4):
        assert abs(o1[i] - o0[i]) <= 1e-4 * abs(o0[i]), (i, o0, o1)
    print("tiled outputs bit-equal in all", k, "copies; out8", o0.tolist(), o1.tolist())


@TILE_PARAMS
def test_focal_is_position_independent(ops, C, dtype):
    small, big = PC.focal_tiled(C, dtype == BF)
    gamma, alpha, gs = 2.0, 0.25, 0.25
    got0 = focal_dense_vs_oracle(ops, small, dtype, gamma, alpha, gs, (small["B"], small["A"]))
    got1 = ops.softmax_focal_loss(*FG.upload(big, dtype), gamma, alpha, 0.5, gs * PC.TILE_K)
    check_tiling(got0, got1)


@TILE_PARAMS
def test_multibox_is_position_independent(ops, C, dtype):
    small, big = PC.multibox_tiled(C, dtype)
    alpha, gs = 0.5, 0.25
    MG.check_against_oracle(ops, small, 3, alpha, gs)                      # anchors the bit comparison
    got0 = ops.multibox_loss(*MG.dev(small), 3, alpha, gs)
    got1 = ops.multibox_loss(*MG.dev(big), 3, alpha, gs * PC.TILE_K)
    check_tiling(got0, got1)


@TILE_PARAMS
def test_reference_loss_is_position_independent(ops, C, dtype):
    """the batch-wide threshold includes ties at tau, so it selects the same anchors in every copy"""
    small, big = PC.loss_tiled(C, dtype)
    LG.run_case(ops, *MG.dev(small))                                      # anchors the bit comparison (grad_scale 1)
    got0 = ops.ssd_loss(*MG.dev(small), 1.0)
    got1 = ops.ssd_loss(*MG.dev(big), float(PC.TILE_K))
    check_tiling(got0, got1)
