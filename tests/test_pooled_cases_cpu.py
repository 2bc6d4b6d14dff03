"""CPU: the cases of tests/pooled_cases.py -- everything tests/test_pooled_layers_strict_gpu.py relies on that can be shown
without a GPU.
  * Regime.  Every operand set is in the exact regime of tests/strict.py, and the fp32 references equal their float64 run.
  * Dispatch.  Every case names the kernel it reaches (the dispatch queries are host functions).
  * Census.  A torch.equal against a reference proves only what the operands can see.  The conditions here are asserted on the
    REFERENCE's inputs, never on a kernel's output: every winner code in interior windows, clipped windows with a winner, ties
    that the first maximum must break, negative and mixed-sign windows for relu = 0, a gradient in the last pooled row and column
    of every image, and for the weight gradient a routed gradient per filter tap whose pixel lies in the zero halo / in the
    neighbouring 16x16 block.
  * Power.  Three deliberately wrong references, built from the same operands, must differ from the right one: winner positions
    1 and 2 exchanged; clipped windows treated as full (memory read and written on past the map's edge: the next row's first
    pixel, the next image's first row); the pooled map taken at pitch Wp + 1.  The second can differ only where a case HAS clipped
    windows (SAME pooling of an odd size): there it must, elsewhere it must equal the right reference (which checks the wrong
    reference itself)."""
import functools

import pytest

torch = pytest.importorskip("torch")

from tests import strict                                                                         # noqa: E402
from tests import pooled_cases as P                                                              # noqa: E402
from tests.conv_cases import WS_BYTES, plan_name                                                 # noqa: E402

NEG = float("-inf")


def _id(c):
    return str(tuple(v for v in c if not isinstance(v, (str, tuple))))


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------- references, computed once and never modified
@functools.lru_cache(maxsize=None)
def conv_ref(case):
    return strict.conv_case(case + (3, 1, "same"))


@functools.lru_cache(maxsize=None)
def fwd_ref(case, same, relu):
    return strict.fwd_pool_case(case + (3, 1, "same"), same, relu, r=conv_ref(case))


@functools.lru_cache(maxsize=None)
def unpool_ref(case):
    return strict.unpool_case(*case)


@functools.lru_cache(maxsize=None)
def wgrad_ref(case):
    return strict.wgrad_unpooled_case(*case)


# ---------------------------------------------------------------- windows, and the three wrong references
def window_values(x, Hp, Wp):
    """x [B,H,W,C] -> (v [B,Hp,Wp,C,4] with -inf at the positions past the map's edge, full [Hp,Wp]: the window has all four)"""
    B, H, W, C = x.shape
    v = torch.full((B, Hp, Wp, C, 4), NEG)
    for p in range(4):
        iy, ix = torch.arange(Hp) * 2 + p // 2, torch.arange(Wp) * 2 + p % 2
        ok = ((iy < H)[:, None] & (ix < W)[None, :])[None, :, :, None]
        v[..., p] = torch.where(ok, x[:, iy.clamp(max=H - 1)][:, :, ix.clamp(max=W - 1)], torch.tensor(NEG))
    full = ((torch.arange(Hp) * 2 + 1 < H)[:, None] & (torch.arange(Wp) * 2 + 1 < W)[None, :])
    return v, full


def swap12(code):
    """wrong: winner positions 1 (dx) and 2 (dy) exchanged"""
    return torch.where(code == 1, torch.tensor(2), torch.where(code == 2, torch.tensor(1), code))


def _flat_index(B, H, W, Hp, Wp, p):
    b, wy, wx = torch.arange(B)[:, None, None], torch.arange(Hp)[None, :, None], torch.arange(Wp)[None, None, :]
    idx = (b * H + 2 * wy + p // 2) * W + 2 * wx + p % 2
    return idx.clamp(max=B * H * W - 1), idx < B * H * W


def pool_flat(x, Hp, Wp):
    """wrong: clipped windows treated as full -- the map read on through memory past its edge"""
    B, H, W, C = x.shape
    flat = x.reshape(B * H * W, C)
    best, pos = torch.full((B, Hp, Wp, C), NEG), torch.full((B, Hp, Wp, C), 4, dtype=torch.int64)
    for p in range(4):
        idx, ok = _flat_index(B, H, W, Hp, Wp, p)
        v = torch.where(ok[..., None], flat[idx], torch.tensor(NEG))
        better = v > best
        best, pos = torch.where(better, v, best), torch.where(better, torch.tensor(p), pos)
    return best, torch.where(best > 0, pos, torch.tensor(4))


def unpool_flat(code, dy, x_shape):
    """un-pooling by linear addresses: with codes of clipped-as-full windows a gradient lands in the next row / the next image"""
    B, H, W, C = x_shape
    _, Hp, Wp, _ = dy.shape
    out = torch.zeros((B * H * W, C), dtype=dy.dtype)
    for p in range(4):
        idx, ok = _flat_index(B, H, W, Hp, Wp, p)
        g = dy * (code == p) * ok[..., None]
        out.index_add_(0, idx.reshape(-1), g.reshape(-1, C))
    return out.view(x_shape)


def repitch(t):
    """wrong: the pooled map [B,Hp,Wp,C] taken at pitch Wp + 1 (zeros past the end)"""
    B, Hp, Wp, C = t.shape
    b, wy, wx = torch.arange(B)[:, None, None], torch.arange(Hp)[None, :, None], torch.arange(Wp)[None, None, :]
    idx = (b * Hp + wy) * (Wp + 1) + wx
    ok = idx < B * Hp * Wp
    return torch.where(ok[..., None], t.reshape(-1, C)[idx.clamp(max=B * Hp * Wp - 1)], torch.zeros((), dtype=t.dtype))


def has_clipped(H, W, same):
    return same and (H % 2 == 1 or W % 2 == 1)


# ---------------------------------------------------------------- the census of a pooled map's input
def pool_census(x, code, same, what):
    """the conditions on the map `x` that is pooled and on its winner codes"""
    B, H, W, C = x.shape
    Hp, Wp = code.shape[1:3]
    v, full = window_values(x, Hp, Wp)
    interior = code[:, full]
    for c in range(5):
        assert bool((interior == c).any()), "%s: no interior window with the winner code %d" % (what, c)
    if same and H % 2:
        assert bool((code[:, -1, :Wp - (W % 2)] < 4).any()), "%s: no clipped window of the last row has a winner" % what
    if same and W % 2:
        assert bool((code[:, :Hp - (H % 2), -1] < 4).any()), "%s: no clipped window of the last column has a winner" % what
    if same and H % 2 and W % 2:
        assert bool((code[:, -1, -1] == 0).any()), "%s: the corner window never has a winner" % what
    # ties at the maximum, broken towards the first: winner 0, 1 and 2 each with a later position of the same value
    best = v.amax(-1)
    for first in range(3):
        later = (v[..., first + 1:] == best[..., None]).any(-1)
        assert bool(((code == first) & later).any()), "%s: no tie that the winner %d must win as the first maximum" % (what, first)


def signed_census(y, yp, code, what):
    """relu = 0: a negative maximum is kept under the code 4; windows mix signs"""
    v, _ = window_values(y, *code.shape[1:3])
    assert bool(((yp < 0) & (code == 4)).any()), "%s: no window with a negative maximum" % what
    lo = torch.where(v == NEG, torch.tensor(float("inf")), v).amin(-1)
    assert bool(((lo < 0) & (yp > 0)).any()), "%s: no window that mixes signs" % what
    assert bool(((yp == 0) & (code == 4)).any()), "%s: no window whose maximum is an exact zero" % what


# ---------------------------------------------------------------- forward
FWD_PARAMS = [(c[:5], same, relu) for c in P.FWD_POOL_CASES for same in (True, False) for relu in (True, False)]


@pytest.mark.parametrize("case", P.FWD_POOL_CASES, ids=_id)
def test_fwd_pool_dispatch(L, case):
    assert P.fwd_pool_plans(L, case) == case[5:7], "the dispatch rules moved: this case no longer tests the kernel it names"


@pytest.mark.parametrize("case", [c[:5] for c in P.FWD_POOL_CASES], ids=str)
def test_fwd_pool_regime(case):
    r = conv_ref(case)                                               # conv_case asserts check_conv_regime
    r64 = strict.conv_reference(case + (3, 1, "same"), dtype=torch.float64)
    for name in ("y", "y_relu"):
        assert torch.equal(r[name].double(), r64[name]), name
    for same in (True, False):
        for relu in (True, False):
            rp = fwd_ref(case, same, relu)
            strict.check_regime(rp)
            Hp, Wp = rp["yp"].shape[1:3]
            yp64, code64 = strict.ref_pool(r64["y_relu" if relu else "y"].float(), 2, 2, 0, 0, Hp, Wp, 4)
            assert torch.equal(rp["yp"], yp64) and torch.equal(rp["code"], code64)


@pytest.mark.parametrize("case,same,relu", FWD_PARAMS, ids=str)
def test_fwd_pool_census(case, same, relu):
    r = fwd_ref(case, same, relu)
    y = r["y_relu" if relu else "y"]
    pool_census(y, r["code"], same, "y")
    if not relu:
        signed_census(y, r["yp"], r["code"], "y")


@pytest.mark.parametrize("case,same,relu", FWD_PARAMS, ids=str)
def test_fwd_pool_power(case, same, relu):
    r = fwd_ref(case, same, relu)
    y, yp, code = r["y_relu" if relu else "y"], r["yp"], r["code"]
    assert not torch.equal(swap12(code), code)
    yp_f, code_f = pool_flat(y, *yp.shape[1:3])
    differs = not (torch.equal(yp_f, yp) and torch.equal(code_f, code))
    assert differs == has_clipped(case[1], case[2], same)
    assert not torch.equal(repitch(yp), yp) and not torch.equal(repitch(code), code)


# ---------------------------------------------------------------- data gradient with un-pooling
@pytest.mark.parametrize("case", P.UNPOOL_CASES, ids=_id)
def test_unpool_dispatch(L, case):
    for has_src in (0, 1):
        assert P.unpool_plan(L, case, has_src) == case[6], "the dispatch rules moved: this case no longer tests the kernel it names"


def test_unpool_plan_models_the_unpooling_store(L):
    """64 -> 64: the plain data-gradient query answers the register-weight kernel, which has no un-pooling store"""
    B, Hf, Wf, C, Cout, same = P.UNPOOL_CASES[0][:6]
    H, W = P.pooled_size(Hf, same), P.pooled_size(Wf, same)
    assert plan_name(L, L.ssd_conv2d_bwd_data_plan(B, H, W, C, Cout, 3, 1, 1, 1, H, W, 0, WS_BYTES)) == P.C64B
    assert P.unpool_plan(L, P.UNPOOL_CASES[0]).startswith(P.P32_64)


def test_unpool_plan_refusals(L):
    from ssd_object_detection_amd import _lib
    for case in P.UNPOOL_REFUSED:
        assert P.unpool_plan(L, case) == "error %d" % _lib.SSD_ERR_UNSUPPORTED, case
    q = L.ssd_conv2d_bwd_data_unpool_plan
    assert q(2, 20, 20, 64, 64, 41, 40, 0, WS_BYTES) == _lib.SSD_ERR_UNSUPPORTED        # VALID pooling, odd Hf only
    assert q(2, 20, 20, 64, 64, 40, 41, 0, WS_BYTES) == _lib.SSD_ERR_UNSUPPORTED        # odd Wf only
    assert q(2, 20, 20, 64, 64, 43, 40, 0, WS_BYTES) == _lib.SSD_ERR_VALUE              # H is neither Hf / 2 nor (Hf + 1) / 2
    assert q(2, 20, 20, 60, 64, 40, 40, 0, WS_BYTES) == _lib.SSD_ERR_VALUE              # Cin % 8
    assert q(2, 20, 20, 64, 96, 40, 40, 0, WS_BYTES) == _lib.SSD_ERR_UNSUPPORTED        # 96 gradient channels: the generic kernel


@pytest.mark.parametrize("case", [c[:6] for c in P.UNPOOL_CASES], ids=str)
def test_unpool_regime(case):
    B, Hf, Wf, C, Cout, same = case
    r = unpool_ref(case)
    strict.check_regime(r)
    H, W = r["geom"][:2]
    r64 = strict.conv_reference((B, H, W, C, Cout, 3, 1, "same"), dtype=torch.float64)
    assert torch.equal(r["dx"].double(), r64["dx"])
    for name, src in (("dfull", r64["dx"]), ("dfull_masked", strict.masked(r64["dx"], r["mask_src"].double() > 0))):
        assert torch.equal(r[name].double(), strict.ref_unpool(r["code"], src, r["full_shape"], 2, 2, 0, 0)), name


@pytest.mark.parametrize("case", [c[:6] for c in P.UNPOOL_CASES], ids=str)
def test_unpool_census(case):
    B, Hf, Wf, C, Cout, same = case
    r = unpool_ref(case)
    pool_census(r["full"].float(), r["code"], same, "the map before the pooling")
    for name in ("dx", "dx_masked"):
        routed = (r[name] != 0) & (r["code"] < 4)
        assert bool(routed[:, -1].flatten(1).any(1).all()), "%s: an image without a routed gradient in the last pooled row" % name
        assert bool(routed[:, :, -1].flatten(1).any(1).all()), "%s: an image without a routed gradient in the last pooled column" % name
    assert bool(((r["mask_src"].float() <= 0) & (r["dx"] != 0)).any()), "the mask never removes a gradient"


@pytest.mark.parametrize("case", [c[:6] for c in P.UNPOOL_CASES], ids=str)
def test_unpool_power(case):
    B, Hf, Wf, C, Cout, same = case
    r = unpool_ref(case)
    code, shape = r["code"], r["full_shape"]
    assert torch.equal(unpool_flat(code, r["dx"], shape), r["dfull"])           # the linear un-pooling itself is right
    _, code_f = pool_flat(r["full"].float(), *code.shape[1:3])
    for name, src in (("dfull", r["dx"]), ("dfull_masked", r["dx_masked"])):
        assert not torch.equal(strict.ref_unpool(swap12(code), src, shape, 2, 2, 0, 0), r[name]), name
        assert torch.equal(unpool_flat(code_f, src, shape), r[name]) != has_clipped(Hf, Wf, same), name
        assert not torch.equal(strict.ref_unpool(repitch(code), repitch(src), shape, 2, 2, 0, 0), r[name]), name


# ---------------------------------------------------------------- weight gradient from the pooled gradient
@pytest.mark.parametrize("case", P.WGRAD_UNPOOLED_CASES, ids=_id)
def test_wgrad_unpooled_dispatch(L, case):
    ns, tiles, tps = P.wgrad_unpooled_splits(L, case)
    assert (ns, tiles) == case[6], "the split plan moved: this case no longer reaches what it names"
    if case is P.LARGEST_WGRAD_CASE:
        B, H, W = case[:3]
        per_image = ((H + 15) // 16) * ((W + 15) // 16)
        assert tiles / ns >= 2, "no workgroup walks a second block"
        spans = [s for s in range(ns) if (s * tps) // per_image != (min((s + 1) * tps, tiles) - 1) // per_image]
        assert spans, "no split holds blocks of two images"
        assert (case[3] // 64) * (case[4] // 64) == 16


def test_wgrad_unpooled_refusals_answer_no_workspace(L):
    for shape in P.WGRAD_UNPOOLED_REFUSED:
        assert L.ssd_conv2d_bwd_weight_unpooled_workspace_bytes(*shape) == 0, shape


@pytest.mark.parametrize("case", [c[:6] for c in P.WGRAD_UNPOOLED_CASES], ids=str)
def test_wgrad_unpooled_regime(case):
    """fp32 == float64 for every case; the float64 run of the largest one happens here and nowhere else"""
    r = wgrad_ref(case)
    strict.check_regime(r)
    r64 = r["f64"]()
    for key in r["exact"]:
        assert torch.equal(r[key].double(), r64[key].double()), key


def tap_census(dyf, Hp, Wp, what):
    """per filter tap (kh, kw): a routed gradient at a pixel (y, x) whose tap pixel (y + kh - 1, x + kw - 1) lies in the zero
    halo, and one whose tap pixel lies in the neighbouring 16x16 block.  The centre tap reads the pixel itself: neither exists.
    Under VALID pooling of an odd size no window covers the last row / column, so no gradient sits next to the halo there: a
    tap that can reach the halo on that side only must instead read the uncovered row / column under a gradient."""
    B, H, W, _ = dyf.shape
    live = (dyf != 0).any(-1).any(0)                                     # [H, W]
    yy, xx = torch.arange(H)[:, None].expand(H, W), torch.arange(W)[None, :].expand(H, W)
    covered = (yy < 2 * Hp) & (xx < 2 * Wp)                              # pixels that lie in a window
    assert not bool((live & ~covered).any())
    for kh in range(3):
        for kw in range(3):
            if (kh, kw) == (1, 1):
                continue
            ty, tx = yy + kh - 1, xx + kw - 1
            inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
            other = inside & ((ty // 16 != yy // 16) | (tx // 16 != xx // 16))
            if bool((covered & ~inside).any()):
                assert bool((live & ~inside).any()), "%s: tap (%d,%d) never reads the zero halo under a gradient" % (what, kh, kw)
            else:
                uncovered = inside & ((ty >= 2 * Hp) | (tx >= 2 * Wp))
                assert bool((live & uncovered).any()), "%s: tap (%d,%d) never reads the uncovered edge under a gradient" % (what, kh, kw)
            if H > 16 or W > 16:
                assert bool((live & other).any()), "%s: tap (%d,%d) never reads the neighbouring block under a gradient" % (what, kh, kw)


@pytest.mark.parametrize("case", [c[:6] for c in P.WGRAD_UNPOOLED_CASES], ids=str)
def test_wgrad_unpooled_census(case):
    B, H, W, Cin, Cout, same = case
    r = wgrad_ref(case)
    pool_census(r["y"].float(), r["code"], same, "the map before the pooling")
    tap_census(r["dy_full"], r["code"].shape[1], r["code"].shape[2], "the routed gradient")
    if not same and (H % 2 or W % 2):                      # the row / column no window covers: no gradient, but read as a neighbour
        if H % 2:
            assert not bool(r["dy_full"][:, -1].any()) and bool(r["x"][:, -1].float().any())
        if W % 2:
            assert not bool(r["dy_full"][:, :, -1].any()) and bool(r["x"][:, :, -1].float().any())


@pytest.mark.parametrize("case", [c[:6] for c in P.WGRAD_UNPOOLED_CASES], ids=str)
def test_wgrad_unpooled_power(case):
    """The wrong references of the large cases are compared on the slice dw[:64, :, :, :64] (the weight gradient of the first 64
    input and output channels is that slice exactly), and on dbias."""
    B, H, W, Cin, Cout, same = case
    r = wgrad_ref(case)
    code, dp, shape = r["code"], r["dp"].float(), tuple(r["y"].shape)
    x = r["x"][..., :64]

    def grads(dyf):
        dw, _ = strict._wgrad(x, dyf[..., :64], 3, 1, 1, 1)
        return dw, dyf.sum((0, 1, 2))

    right = grads(r["dy_full"])
    assert torch.equal(right[0], r["dw"][:64, :, :, :64]) and torch.equal(right[1], r["dbias"])
    assert torch.equal(unpool_flat(code, dp, shape), r["dy_full"])
    _, code_f = pool_flat(r["y"].float(), *code.shape[1:3])
    wrong = {"1 <-> 2": strict.ref_unpool(swap12(code), dp, shape, 2, 2, 0, 0),
             "clipped as full": unpool_flat(code_f, dp, shape),
             "pitch Wp + 1": strict.ref_unpool(repitch(code), repitch(dp), shape, 2, 2, 0, 0)}
    for name, dyf in wrong.items():
        dw, db = grads(dyf)
        expect_equal = name == "clipped as full" and not has_clipped(H, W, same)
        assert torch.equal(dw, right[0]) == expect_equal, name
        if name == "pitch Wp + 1":
            assert not torch.equal(db, right[1]), name
