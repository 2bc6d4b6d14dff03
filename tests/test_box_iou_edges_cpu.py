"""CPU: the inputs of tests/box_iou_edge_cases.py are what tests/test_box_iou_edges_gpu.py needs.  The regime (every comparison a
kernel makes on them is decided by the operands, not by rounding), the class counts, the floored bound against the oracle's f32
restatement, the power of the case -- an oracle with one comparison family relaxed (box_iou_oracle.RELAX) leaves the bound by
more than a hundredfold on enough rows -- and the closed forms at identical boxes.  Nothing here looks at a kernel."""
import numpy as np
import pytest

from tests import box_iou_cases as K
from tests import box_iou_edge_cases as E
from tests import box_iou_oracle as O

CASES = [(shape, exact_w) for shape in E.SHAPES for exact_w in (False, True)]
IDS = ["%s %s" % (s, "f32" if e else "bf16") for s, e in CASES]


def f32_exact(x):
    return np.array_equal(x.astype(np.float32).astype(np.float64), x)


# ---------------------------------------------------------------------------------------------------- the regime
@pytest.mark.parametrize("shape,exact_w", CASES, ids=IDS)
def test_layout(shape, exact_w):
    B, A, C = shape
    c = E.make_case(B, A, C, exact_w)
    mask = c["gt_mask"].astype(bool)
    assert (B * A) % E.ROW_BLOCK != 0 and B * A > 2 * E.ROW_BLOCK        # three or more row blocks, the last ragged
    assert not mask[B - 2].any() and all(mask[b].all() for b in range(B) if b != B - 2)
    assert (c["gt_cls"][~mask] >= C).all() and (c["gt_cls"][mask] < C - 1).all()
    assert np.isin(c["priors"][:, 2:], E.SIZES).all()
    assert np.array_equal(K.to_bf16(c["conf"]), c["conf"])
    on_grid = np.array_equal(K.to_bf16(c["loc"]), c["loc"]) and np.array_equal(K.to_bf16(c["gt_loc"]), c["gt_loc"])
    assert on_grid == (not exact_w)
    # the designed rows: from the first positive anchor on, on both sides of a row-block boundary, up to the last anchor
    b, a = np.nonzero(mask)
    flat = (b * A + a)[c["fixed"]]
    first = 0 if B != 2 else A
    nd = E.n_designed()
    assert len(flat) == 2 * nd and flat[0] == first and flat[-1] == B * A - 1
    assert c["boundary"] % E.ROW_BLOCK == 0 and {c["boundary"] - 1, c["boundary"]} <= set(flat.tolist())
    wh, t, g = E.positives(c)
    dt, dg = E.designed(exact_w)
    assert np.array_equal(t[c["fixed"]], np.concatenate([dt, dt])) and np.array_equal(g[c["fixed"]], np.concatenate([dg, dg]))
    free = np.setdiff1d(np.arange(len(t)), c["fixed"])
    assert E.on_lattice(t[free], g[free]).all()
    # the values at the clamp
    assert {4.125, 4.15625, -4.125, -4.15625, 8.0, -8.0, 100.0, -100.0} <= set(t[:, 2].tolist()) & set(t[:, 3].tolist())
    at_w = {float(E.WF), float(E.WF_IN), -float(E.WF), -float(E.WF_IN)}
    assert (at_w <= set(t[:, 2].tolist()) & set(t[:, 3].tolist())) == exact_w
    assert (g[:, 2] == 5).any() and (g[:, 3] == -5).any()


@pytest.mark.parametrize("shape,exact_w", CASES, ids=IDS)
def test_regime_and_class_counts(shape, exact_w):
    c = E.make_case(*shape, exact_w)
    wh, t, g = E.positives(c)
    lat = E.on_lattice(t, g)
    assert lat.sum() >= len(t) // 2
    # lattice rows: every corner, iwr and ihr is exact in float32 -- no rounding can move a comparison
    for v in E.corners(wh[lat], t[lat], g[lat]):
        assert f32_exact(v)
    # every other row: an exact tie (by construction: identical operands) or far from one
    assert E.nearest_kink(wh, t, g).min() >= 0.05
    # the clamp is never approached except on purpose: 4.125 and 4.15625 are 1e-2 away, float32(W) and its neighbour are the point
    d = np.abs(np.abs(np.concatenate([t[:, 2:], g[:, 2:]], axis=1).astype(np.float64)) - O.W)
    at_w = np.isin(np.abs(t[:, 2:]), [E.WF, E.WF_IN])
    assert (d[:, :2][~at_w] >= 1e-2).all() and (d[:, 2:] >= 1e-2).all() and at_w.any() == exact_w
    counts = {k: int(v.sum()) for k, v in E.classes(c).items()}
    print(shape, "exact_w" if exact_w else "bf16 grid", counts)
    assert set(counts) == set(E.CLASSES) and min(counts.values()) >= 8, counts
    # the f32 restatement has exactly the float64 zero pattern, and both are finite: status 0
    for kind in O.KINDS:
        L64, d64 = O.rows(kind, wh, t, g)
        L32, d32 = O.rows(kind, wh, t, g, np.float32)
        assert np.isfinite(L64).all() and np.isfinite(d64).all() and np.isfinite(L32).all() and np.isfinite(d32).all()
        assert np.array_equal(d64 == 0, d32 == 0), kind
        assert (d64 == 0).any(axis=1).sum() >= 8 * 6                    # zeros are what is under test: ties, touches, clamps
        # clamped components are exactly zero, and the components next to the clamp are not
        cl = np.abs(t[:, 2:].astype(np.float64)) >= O.W
        assert (d64[:, 2:][cl] == 0).all()
        near = np.isin(np.abs(t[:, 2:]), [np.float32(4.125), E.WF_IN])
        assert near.sum() >= 8 and (np.abs(d64[:, 2:][near]) > 1e-2).all()
    assert not O.box_term("ciou", c["priors"], c["gt_loc"], c["gt_mask"], c["loc"])[2]


# ---------------------------------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("shape,exact_w", CASES, ids=IDS)
def test_f32_restatement_meets_the_floored_bound_with_a_factor_of_three(shape, exact_w, kind):
    c = E.make_case(*shape, exact_w)
    for gs in E.GRAD_SCALES:
        s = E.scale_of(c, gs)
        a = O.box_term(kind, c["priors"], c["gt_loc"], c["gt_mask"], c["loc"], E.LOC_WEIGHT, gs)
        b = O.box_term(kind, c["priors"], c["gt_loc"], c["gt_mask"], c["loc"], E.LOC_WEIGHT, gs, dtype=np.float32)
        assert not a[2] and not b[2]
        ratio = (np.abs(a[1] - b[1]) / E.dloc_bound_floored(a[1], s)).max()
        print(shape, kind, gs, "f32 restatement, error / floored bound:", ratio, "loss, relative:", abs(a[0] - b[0]) / a[0])
        assert ratio <= 1.0 / 3
        assert abs(a[0] - b[0]) <= 1e-4 / 3 * abs(a[0])
    # the floor is needed: on the identical rows the unfloored bound is zero or next to it
    mask = c["gt_mask"].astype(bool)
    ident = E.classes(c)["identical"]
    if kind == "giou":
        assert (K.dloc_bound(a[1])[mask][ident] <= 1e-12 * s).all()
    # ... and it is the old bound wherever a row's gradient is of order one or more
    big = np.abs(a[1]).max(axis=-1) >= s
    assert big[mask].sum() >= 8 and (E.dloc_bound_floored(a[1], s)[big] == K.dloc_bound(a[1])[big]).all()
    assert (E.dloc_bound_floored(a[1], s, True) >= E.dloc_bound_floored(a[1], s)).all()


# ---------------------------------------------------------------------------------------------------- the power
def test_relax_none_is_the_rule_bit_for_bit():
    """the keyword's default leaves rows() as it was: the same bits as an evaluation that never names it, on kink-free rows and
    on the edge rows, and each family changes only rows that meet one of its kinks"""
    c = E.make_case(*E.SHAPES[1], True)
    k = K.make_case(*K.SHAPES[1])
    for wh, t, g in (E.positives(c), K.positives(k)):
        for kind in O.KINDS:
            for dtype in (np.float64, np.float32):
                L0, d0 = O.rows(kind, wh, t, g, dtype)
                L1, d1 = O.rows(kind, wh, t, g, dtype, relax=None)
                assert L0.tobytes() == L1.tobytes() and d0.tobytes() == d1.tobytes()
    wh, t, g = K.positives(k)                                            # no kink, no difference
    for kind in O.KINDS:
        for relax in O.RELAX:
            assert O.rows(kind, wh, t, g, relax=relax)[1].tobytes() == O.rows(kind, wh, t, g)[1].tobytes()
    with pytest.raises(AssertionError):
        O.rows("giou", wh, t, g, relax="everything")


@pytest.mark.parametrize("relax", O.RELAX)
@pytest.mark.parametrize("kind", O.KINDS)
@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_a_relaxed_comparison_leaves_the_bound_a_hundredfold(shape, kind, relax):
    """What a kernel with one family of comparisons non-strict would return -- the f32 restatement under relax= -- differs from
    the rule by more than 100 bounds on 8 positives or more: the GPU test would fail on it.  The clamp's `<=` can show only where
    |t| is the kernel's own constant float32(W) (that value is > W: float64 clamps it under either comparison, a float32
    evaluation under `<` only), so it is evaluated on the f32 case and every row that holds the value has to show it; the other
    families on the bf16-grid case, which the f32 call shares.  The loss itself does not move: the rule is about gradients."""
    clamp = relax == "clamp"
    c = E.make_case(*shape, clamp)
    wh, t, g = E.positives(c)
    L64, d64 = O.rows(kind, wh, t, g)
    Lm, dm = O.rows(kind, wh, t, g, np.float32, relax=relax)
    bound = 1e-4 * np.maximum(np.abs(d64).max(axis=1), 1.0)             # dloc_bound_floored over scale
    far = np.abs(dm - d64).max(axis=1) / bound
    print(shape, kind, relax, "rows beyond 100 bounds:", int((far > 100).sum()), "the smallest of them:", far[far > 100].min())
    assert (far > 100).sum() >= 8
    assert np.abs(Lm - L64).max() <= 1e-6
    cl = E.classes(c)
    if clamp:
        at_w = (np.abs(t[:, 2:]) == E.WF).any(axis=1)
        assert at_w.sum() >= 8 and (far[at_w] > 100).all() and (far[~at_w] <= 1.0 / 3).all()
    elif relax == "positive":                                            # shows where boxes touch on one axis and overlap on the other
        assert (far > 100).sum() == (far[cl["touch x"] | cl["touch y"]] > 100).sum()
    else:                                                                # shows only where a corner ties
        x1, x2, y1, y2, X1, X2, Y1, Y2, _, _ = E.corners(wh, t, g)
        tie = (x1 == X1) | (x2 == X2) | (y1 == Y1) | (y2 == Y2)
        assert (far[~tie] <= 1.0 / 3).all()
        if relax == "intersection" or kind == "giou":                    # (DIoU's hull term carries rho2, which is 0 there)
            assert (far[cl["identical"]] > 100).all()


# ---------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_closed_forms_at_identical_boxes_and_on_the_lattice(dtype):
    eps = float(np.finfo(dtype).eps)
    for shape in E.SHAPES:
        c = E.make_case(*shape)
        wh, t, g = E.positives(c)
        cl = E.classes(c)
        zero_sizes = (t[:, 2:] == 0).all(axis=1)
        idz = cl["identical"] & zero_sizes
        assert idz.sum() >= 8 and (cl["identical"] & ~zero_sizes).sum() >= 2
        lat = E.on_lattice(t, g)
        res = {kind: O.rows(kind, wh, t, g, dtype) for kind in O.KINDS}
        for kind, (L, d) in res.items():
            assert L.dtype == dtype and (L[idz] == 0.0).all(), kind      # I == U == Cc bitwise, rho2 == 0, v == 0
            assert (d[cl["identical"]][:, :2] == 0).all(), kind          # every corner ties: no max / min passes anything
            if kind == "giou":
                assert (d[cl["identical"]] == 0).all()                   # two terms with bitwise equal operands cancel
            else:
                assert np.abs(d[idz][:, 2:] - 1.0).max() <= 4 * eps, (kind, np.abs(d[idz][:, 2:] - 1.0).max())
                nz = cl["identical"] & ~zero_sizes                       # w == gw whatever exp gave: w I h / U^2 == 1 to a few ulp
                assert np.abs(d[nz][:, 2:] - 1.0).max() <= 8 * eps
                assert np.abs(L[nz]).max() <= 8 * eps
        # CIoU is DIoU on every lattice row: atan(w / h) == atan(gw / gh), v == 0, and alpha's guard is what keeps 0 / 0 out
        assert res["ciou"][0][lat].tobytes() == res["diou"][0][lat].tobytes()
        assert res["ciou"][1][lat].tobytes() == res["diou"][1][lat].tobytes()
        assert (res["diou"][0][idz] == 0).all()                          # (1 - IoU) + v == 0 there: unguarded, alpha were 0 / 0


@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_identical_case(shape):
    c = E.identical_case(*shape)
    assert np.array_equal(c["gt_mask"], E.make_case(*shape)["gt_mask"])
    wh, t, g = E.positives(c)
    assert np.array_equal(t, g) and E.on_lattice(t, g).all() and E.classes(c)["identical"].all()
    assert len(np.unique(t[:, :2], axis=0)) > 8
    for kind in O.KINDS:
        for dtype in (np.float64, np.float32):
            l_loc, dbox, bad = O.box_term(kind, c["priors"], c["gt_loc"], c["gt_mask"], c["loc"], E.LOC_WEIGHT, 0.25, dtype)
            s = E.scale_of(c, 0.25)
            mask = c["gt_mask"].astype(bool)
            assert l_loc == 0.0 and not bad
            want = np.zeros(4) if kind == "giou" else np.array([0.0, 0.0, s, s])
            assert (np.abs(dbox[mask] - want) <= 1e-6 * s).all() and (dbox[mask][:, :2] == 0).all()
