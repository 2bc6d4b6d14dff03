"""GPU: ssd_maxpool2x2_bwd_argmax_accumulate under the strict harness (tests/strict.py).

The un-pooling that adds onto a gradient map another path has written (conv4_3 of the VGG-16 SSD300 feeds a head and pool4).
Expected value, computed in fp32 on the CPU: (dx0.float() + ref_unpool(code, dy).float()).to(bfloat16) -- one addition, one
rounding -- compared BIT FOR BIT.  dx0 is random finite bf16 over many binades, so most sums are inexact in bf16 and the rounding
is exercised; codes are random in 0..4 with at least 10 % of the windows at 4 (they add nothing).  dx lives in strict.Arena as an
in-out tensor: 1 MiB guards that touch it, the call run under two poisons.  For a VALID pooling of an odd map the last row and
column are outside the documented extent and must keep their preset bits."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                              # noqa: E402

BF, I32 = torch.bfloat16, torch.int32
# (B, H, W, C, same)
CASES = [(2, 6, 6, 8, False),             # VALID, even
         (2, 7, 7, 16, False),            # VALID, odd: row 6 and column 6 keep their bits
         (2, 7, 7, 8, True),              # SAME, Ho = 4: clipped windows
         (1, 38, 38, 512, False),         # pool4's own shape
         (3, 21, 21, 512, False)]         # VALID, odd, wide
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def make_case(case):
    """operands and the expected map, once per case"""
    if case in _CACHE:
        return _CACHE[case]
    B, H, W, C, same = case
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if same else (H // 2, W // 2)
    g = torch.Generator().manual_seed(1000 + 7 * H + C + (3 if same else 0) + B)
    code = torch.randint(0, 5, (B, Ho, Wo, C), generator=g)
    # whole windows (all channels of a pixel) at 4 as well: a thread that has nothing to add
    code = torch.where(torch.rand((B, Ho, Wo, 1), generator=g) < 0.1, torch.tensor(4), code)
    share = float((code == 4).float().mean())
    assert share >= 0.10, share
    mag = lambda shape: torch.exp2(torch.randint(-12, 6, shape, generator=g).float())     # noqa: E731
    dy = (torch.randn((B, Ho, Wo, C), generator=g) * mag((B, Ho, Wo, C))).to(BF)
    dx0 = (torch.randn((B, H, W, C), generator=g) * mag((B, H, W, C))).to(BF)
    assert bool(torch.isfinite(dy.float()).all()) and bool(torch.isfinite(dx0.float()).all())
    route = strict.ref_unpool(code, dy.float(), (B, H, W, C), 2, 2, 0, 0)
    want = (dx0.float() + route.float()).to(BF)
    # the sums are not all exact in bf16: the rounding is part of what is compared
    named = route != 0
    exact = (dx0.float() + route.float()) == want.float()
    assert float((~exact[named]).float().mean()) > 0.25
    covered = torch.zeros((B, H, W, C), dtype=torch.bool)
    covered[:, :min(H, 2 * Ho), :min(W, 2 * Wo)] = True
    assert torch.equal(bits(want)[~covered], bits(dx0)[~covered])
    r = dict(code=code, words=strict.pack_codes(code), dy=dy, dx0=dx0, route=route, want=want, covered=covered, Ho=Ho, Wo=Wo)
    _CACHE[case] = r
    return r


def arena_of(r):
    total = sum(t.numel() * t.element_size() for t in (r["words"], r["dy"], r["dx0"]))
    return strict.Arena("cuda", 2 * total + 16 * (2 * strict.GUARD + 2 * strict.ALIGN))


@pytest.mark.parametrize("case", CASES, ids=str)
def test_accumulate_matches_one_fp32_addition_bit_for_bit(ops, case):
    B, H, W, C, same = case
    r = make_case(case)
    a = arena_of(r)
    words, dy = a.put(r["words"], "code"), a.put(r["dy"], "dy")
    dx = a.inout(r["dx0"], "dx")
    got = a.run(lambda: ops.maxpool2x2_bwd_argmax(words, dy, (B, H, W, C), out=dx, accumulate=True),
                [(dx, r["want"], r["covered"])])[0]
    assert torch.equal(bits(got), bits(r["want"])), strict.first_diff(bits(got), bits(r["want"]))
    if not same and H % 2:                                        # the uncovered row and column: preset bits
        assert torch.equal(bits(got[:, H - 1]), bits(r["dx0"][:, H - 1]))
        assert torch.equal(bits(got[:, :, W - 1]), bits(r["dx0"][:, :, W - 1]))
    # windows at code 4 and the losers of a window keep their bits as well
    keep = r["route"] == 0
    assert torch.equal(bits(got)[keep], bits(r["dx0"])[keep])


@pytest.mark.parametrize("case", CASES, ids=str)
def test_onto_zeros_equals_the_overwrite_form_and_repeats(ops, case):
    B, H, W, C, same = case
    r = make_case(case)
    words, dy = r["words"].cuda(), r["dy"].cuda()
    plain = ops.maxpool2x2_bwd_argmax(words, dy, (B, H, W, C))
    acc = [ops.maxpool2x2_bwd_argmax(words, dy, (B, H, W, C), out=torch.zeros((B, H, W, C), dtype=BF, device="cuda"), accumulate=True)
           for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(bits(acc[0]), bits(plain)), strict.first_diff(bits(acc[0]), bits(plain))
    assert torch.equal(bits(acc[0]), bits(acc[1]))
    two = [ops.maxpool2x2_bwd_argmax(words, dy, (B, H, W, C), out=r["dx0"].cuda(), accumulate=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(bits(two[0]), bits(two[1]))
    assert torch.equal(bits(two[0]), bits(r["want"]))


def test_refusals_leave_dx_untouched(ops, lib):
    L = lib.lib()
    B, H, W, C = 2, 6, 6, 16
    words = torch.zeros((B, 3, 3, C // 8), dtype=I32, device="cuda")
    dy = torch.ones((B, 3, 3, C), dtype=BF, device="cuda")
    dx = torch.full((B, H, W, C), 3.0, dtype=BF, device="cuda")
    before = bits(dx).clone()
    p, s = ops._ptr, ops._stream()
    null = ctypes.c_void_p(0)
    fn = L.ssd_maxpool2x2_bwd_argmax_accumulate
    assert fn(null, p(dy), p(dx), B, H, W, C, 3, 3, s) == lib.SSD_ERR_VALUE
    assert fn(p(words), null, p(dx), B, H, W, C, 3, 3, s) == lib.SSD_ERR_VALUE
    assert fn(p(words), p(dy), null, B, H, W, C, 3, 3, s) == lib.SSD_ERR_VALUE
    assert fn(p(words), p(dy), p(dx), B, H, W, 12, 3, 3, s) == lib.SSD_ERR_VALUE
    assert fn(p(words), p(dy), p(dx), 0, H, W, C, 3, 3, s) == lib.SSD_ERR_VALUE
    torch.cuda.synchronize()
    assert torch.equal(bits(dx), before)
    with pytest.raises(ValueError):
        ops.maxpool2x2_bwd_argmax(words, dy, (B, H, W, C), accumulate=True)          # nothing to add onto
