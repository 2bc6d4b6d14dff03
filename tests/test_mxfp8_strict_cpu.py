"""CPU: the MX-fp8 operand designs of tests/strict.py (what tests/test_mxfp8_strict_gpu.py runs).
  * The regime of every case: the operands survive MX e4m3 exactly, every term is a multiple of the grid, the absolute sum stays
    below 2^24 grids (so the fp32 accumulator adds exactly in any order), and the fp32 reference equals the float64 one.
  * The proof that the designs can fail: the reference recomputed from the same BYTES under wrongly routed scale arrays -- blocks
    swapped inside a k-step, k-steps swapped, the scale of the neighbouring pixel, tap or filter -- differs from the expected
    bf16 map in at least a quarter of its elements, for every case and every mutation.  (mx_conv_case's uniform scales fail
    this: tests/test_mxfp8_strict_cpu.py::test_uniform_scales_cannot_fail states it.)
  * The reference quantiser on the edges the GPU test sweeps, against an integer restatement of the rule."""
import math

import pytest

torch = pytest.importorskip("torch")

from tests import strict                                                              # noqa: E402

BF = torch.bfloat16
FWD = [(c, d, False) for c in strict.MX_FWD_CASES for d in "AB"] + [(strict.MX_WIDE_FWD_CASE, "A", True)]
DGRAD = [(c, d, False) for c in strict.MX_DGRAD_CASES for d in "AB"] + [(strict.MX_WIDE_DGRAD_CASE, "A", True)]


def ident(p):
    return "%s %s%s" % (str(p[0][:7]).replace(" ", ""), p[1], " wide" if p[2] else "")


def share(a, b):
    return float((a.float() != b.float()).float().mean())


def check_scales_differ(r, a_s, f_s):
    """neighbouring blocks, k-steps, pixels, taps and filters carry different scale bytes"""
    a, f = a_s.int(), f_s.int()
    assert share(a[..., 1:], a[..., :-1]) > 0.8 and share(a[:, :, 1:], a[:, :, :-1]) > 0.5
    assert share(f[..., 1:], f[..., :-1]) > 0.8 and share(f[1:], f[:-1]) > 0.5
    assert not bool((a_s == 255).any()) and not bool((f_s == 255).any())
    if r["wide"]:
        assert int(a.min()) < 90 and int(a.max()) > 155 and int(f[f != 127].min()) < 90 and int(f.max()) > 155


@pytest.mark.parametrize("p", FWD, ids=ident)
def test_forward_design(p):
    case, design, wide = p
    B, H, W, Cin, Cout, k, stride, mode = case
    r = strict.mx_fwd_design(case, design, wide)                 # asserts the exact round trip and check_mx_regime
    Ho, Wo, pt, pl = r["geom"]
    print("bound 2^%.1f" % math.log2(r["bound"]))
    y32 = strict.ref_conv(r["x"].float(), r["w"].float(), r["bias"], k, stride, pt, pl, Ho, Wo, False)
    assert torch.equal(y32.double(), r["y64"])
    check_scales_differ(r, r["x_s"], r["w_s_op"])
    assert torch.equal(strict.mx_fwd_from_scales(r, r["x_s"], r["w_s_op"]), r["y"])
    # the fused quantiser's scales are not uniform either
    _, s = strict.ref_quantize_mx(r["y_relu"][..., :Cout // 32 * 32].contiguous())
    assert len(s.unique()) >= 3
    for name, xs, ws in strict.mx_scale_mutations(r, r["x_s"], r["w_s_op"], k, design):
        changed = share(strict.mx_fwd_from_scales(r, xs, ws), r["y"])
        print("%-22s %.2f" % (name, changed))
        assert changed >= 0.25, (name, changed)


@pytest.mark.parametrize("p", DGRAD, ids=ident)
def test_data_gradient_design(p):
    case, design, wide = p
    B, H, W, Cin, Cout, k, stride, mode = case
    r = strict.mx_dgrad_design(case, design, wide)
    Ho, Wo, pt, pl = r["geom"]
    print("bound 2^%.1f" % math.log2(r["bound"]))
    xr = torch.zeros((B, H, W, Cin), requires_grad=True)
    w32 = r["w_t"].permute(3, 1, 2, 0).flip(1, 2).contiguous().float()
    strict.ref_conv(xr, w32, None, k, 1, pt, pl, Ho, Wo, False).backward(r["dy"].float())
    assert torch.equal(xr.grad.double(), r["dx64"])
    check_scales_differ(r, r["dy_s"], r["w_t_s_op"])
    assert torch.equal(strict.mx_dgrad_from_scales(r, r["dy_s"], r["w_t_s_op"]), r["dx"])
    assert int((r["dx_masked"].float() != r["dx"].float()).sum()) > 0 and int((r["dx_acc"].float() != r["dx_masked"].float()).sum()) > 0
    for name, ds, ws in strict.mx_scale_mutations(r, r["dy_s"], r["w_t_s_op"], k, design):
        changed = share(strict.mx_dgrad_from_scales(r, ds, ws), r["dx"])
        print("%-22s %.2f" % (name, changed))
        assert changed >= 0.25, (name, changed)


def test_design_b_isolates_one_block_per_instruction():
    r = strict.mx_fwd_design(strict.MX_CONV3X3_CASES[0], "B")
    Cout, k, _, Cin = r["w"].shape
    nz = r["w"].float().view(Cout, 9, Cin // 128, 4, 32).abs().amax(-1) > 0            # [n, tap, k-step, block]
    assert int(nz.sum(-1).max()) == 1
    n, tap, ks, blk = nz.nonzero(as_tuple=True)
    assert torch.equal(blk, (n + tap + ks) % 4)
    decoys = r["w_s_op"].view(Cout, 9, Cin // 128, 4)[~nz]
    assert int(decoys.min()) >= strict.DECOY[0] and int(decoys.max()) <= strict.DECOY[1] and len(decoys.unique()) > 20


def test_uniform_scales_cannot_fail():
    """the gap this file closes: under mx_conv_case's operands a swap of two activation scale blocks changes no output"""
    case = (2, 7, 7, 512, 64, 1, 1, "same")
    r = strict.mx_conv_case(case)
    r.update(case=case)
    perm = torch.tensor([1, 0] + list(range(2, 16)))
    assert share(strict.mx_fwd_from_scales(r, r["x_s"][..., perm], r["w_s"]), r["y"].to(BF)) == 0.0


def test_eltwise_design():
    r = strict.mx_eltwise_case((3, 17, 19, 256))
    _, s = strict.ref_quantize_mx(r["out"].to(BF))
    assert len(s.unique()) >= 40


# ---------------------------------------------------------------- the reference quantiser, against integers
def rule_by_integers(bits):
    """(scale byte, e4m3 byte of element 0) for a block whose maximum is its element 0 = the finite bf16 pattern `bits`: the stated
    rule in exact integer arithmetic (no frexp, no float division)"""
    mant, ex = bits & 0x7F, (bits >> 7) & 0xFF
    if ex == 0 and mant == 0:
        return 127, (bits >> 8) & 0x80
    m, p = (mant, -133) if ex == 0 else (mant | 0x80, ex - 134)                      # |v| = m 2^p
    e = -200
    while m * 2 ** (p + 200) > 448 * 2 ** (e + 200):                                  # the smallest e with |v| <= 448 2^e
        e += 1
    e = max(e, -127)
    # |v| / 2^e on e4m3's grid: normals (8 + f) 2^(E - 10) for E = 1..15, subnormals f 2^-9; round to nearest even
    num, shift = m, p - e                                                             # |v| / 2^e = num 2^shift
    best = None
    for code in range(0x7F):
        E, f = code >> 3, code & 7
        val_num, val_shift = ((8 + f), E - 10) if E else (f, -9)
        lo = min(shift, val_shift)
        diff = abs(num * 2 ** (shift - lo) - val_num * 2 ** (val_shift - lo)) * 2 ** (lo + 400)
        if best is None or diff < best[0] or (diff == best[0] and code % 2 == 0 and best[1] % 2 == 1):
            best = (diff, code)
    return e + 127, best[1] | ((bits >> 8) & 0x80)


def test_reference_quantiser_on_the_edges():
    pats = [0x0001, 0x007F, 0x0080, 0x0100, 0x3F80, 0x43E0, 0x43E1, 0x43DF, 0x7F7F, 0x7F00, 0xC3E0, 0x8001, 0x0240, 0x0260, 0x02E0,
            0x0360, 0x03E0, 0x0460] + list(range(0x0040, 0x7F80, 0x0123))
    for bits in pats:
        blk = torch.zeros(32, dtype=torch.int16)
        blk[0] = strict._signed(bits, 2)
        q, s = strict.ref_quantize_mx(blk.view(BF))
        want_s, want_q = rule_by_integers(bits)
        assert (int(s[0]), int(q[0])) == (want_s, want_q), (hex(bits), int(s[0]), int(q[0]), want_s, want_q)


def test_reference_quantiser_non_finite_rule():
    t = torch.ones((4, 64), dtype=BF)
    t[0, 0], t[1, 40], t[2, 63] = float("nan"), float("inf"), float("-inf")
    q, s = strict.ref_quantize_mx(t)
    bad = torch.tensor([[True, False], [False, True], [False, True], [False, False]])
    assert torch.equal(torch.isnan(strict.ref_dequantize_mx(q, s)).view(4, 2, 32).all(-1), bad)
    assert torch.equal(q.view(4, 2, 32)[bad], torch.full((3, 32), 0x7F, dtype=torch.uint8)) and bool((s[bad] == 127).all())
    assert torch.equal(strict.ref_dequantize_mx(q, s)[3], t[3].float())
