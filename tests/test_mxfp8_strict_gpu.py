"""GPU: the MX-fp8 kernels on operands whose block scales DIFFER, and the quantiser over its whole domain.

tests/test_conv_strict_gpu.py's MX-fp8 cases have one activation scale byte and one filter scale byte, so they cannot see
whether a scale byte reaches the block it belongs to.  Here every case runs under the two operand designs of tests/strict.py
(A "cancelling", B "block-isolated"; tests/test_mxfp8_strict_cpu.py shows that every wrong scale routing changes at least a
quarter of their expected outputs) through the strict harness: arena, guard bands, two poisons, every comparison torch.equal.
The kernels get the reference's bytes and scales directly -- after ssd_quantize_mx_fp8 has reproduced them through the arena --
and every fused quantisation must equal ref_quantize_mx of the expected bf16 map.

The quantiser: one block for each of the 65 280 finite bf16 patterns as its maximum (the clamp at scale byte 0, bf16 denormals,
e up to +120, both signs, m == 0.5 at every exponent; ties, e4m3 subnormals and underflow among the other elements), and the
non-finite rule of csrc/mxfp8.h, stand-alone and fused."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                                                         # noqa: E402

BF, U8 = torch.bfloat16, torch.uint8
DESIGNS = [("A", False), ("B", False)]


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def ident(c):
    return str(c[:7]).replace(" ", "")


def dname(d):
    return d[0] + (" wide" if d[1] else "")


def arena_for(*tensors):
    total = sum(t.numel() * t.element_size() for t in tensors)
    return strict.Arena("cuda", 8 * total + 48 * (2 * strict.GUARD + 2 * strict.ALIGN))


def put_mx(ops, a, t, q_ref, s_ref, s_op, name):
    """the reference's bytes and scales as a kernel operand -- after ssd_quantize_mx_fp8 (through the arena) has reproduced them;
    s_op: the scale bytes the kernel gets (design B: s_ref with decoys on the all-zero blocks)"""
    src = a.put(t, name + " (bf16)")
    q, s = a.out(tuple(t.shape), U8, name + " q"), a.out(tuple(s_ref.shape), U8, name + " scale")
    a.run(lambda: ops.quantize_mx_fp8(src, q=q, scale=s), [(q, q_ref), (s, s_ref)])
    assert torch.equal(ops.dequantize_mx_fp8(q_ref, s_op), t.float())
    return a.put(q_ref, name + " q (operand)"), a.put(s_op, name + " scale (operand)")


def fwd_operands(ops, r):
    a = arena_for(r["x"], r["w"], r["y64"], r["y64"])
    xq, xs = put_mx(ops, a, r["x"], r["x_q"], r["x_s"], r["x_s"], "x")
    wq, ws = put_mx(ops, a, r["w"], r["w_q"], r["w_s"], r["w_s_op"], "w")
    return a, xq, xs, wq, ws, a.put(r["bias"], "bias")


FWD = [(c, d) for c in strict.MX_CONV3X3_CASES + strict.MX_CONV2D_CASES for d in DESIGNS] + [(strict.MX_WIDE_FWD_CASE, ("A", True))]
POOL = [(c, d, s) for c in strict.MX_POOL_CASES for d in DESIGNS for s in (True, False)]
DGRAD = [(c, d) for c in strict.MX_DGRAD_CASES for d in DESIGNS] + [(strict.MX_WIDE_DGRAD_CASE, ("A", True))]


def pid(p):
    return "%s %s" % (ident(p[0]), dname(p[1])) + ("" if len(p) < 3 else (" same" if p[2] else " valid"))


def run_conv2d_fwd(ops, case, design, wide, also_conv3x3=False):
    B, H, W, Cin, Cout, k, stride, _ = case
    r = strict.mx_fwd_design(case, design, wide)
    Ho, Wo, pt, pl = r["geom"]
    a, xq, xs, wq, ws, bias = fwd_operands(ops, r)
    y, q, sc = a.out((B, Ho, Wo, Cout), BF, "y"), a.out((B, Ho, Wo, Cout), U8, "y8"), a.out((B, Ho, Wo, Cout // 32), U8, "yscale")
    for relu in (True, False):
        yr = r["y_relu" if relu else "y"]
        qr, sr = strict.ref_quantize_mx(yr)
        args = (xq, xs, wq, ws, bias, stride, pt, pl, Ho, Wo, relu)
        a.run(lambda: ops.conv2d_fwd_mxfp8(*args, want_bf16=True, want_fp8=True, out=y, out_q=q, out_scale=sc), [(y, yr), (q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_fwd_mxfp8(*args, want_bf16=False, want_fp8=True, out_q=q, out_scale=sc), [(q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_fwd_mxfp8(*args, out=y), [(y, yr)])
        if also_conv3x3:
            a.run(lambda: ops.conv3x3_fwd_mxfp8(xq, xs, wq, ws, bias, relu=relu, out=y), [(y, yr)])


@pytest.mark.parametrize("p", FWD, ids=pid)
def test_conv_fwd(ops, p):
    """conv2d_fwd_mxfp8 with its three output combinations, ReLU on and off; at 3x3 / stride 1 conv3x3_fwd_mxfp8 as well, against
    the same expectation: the two launches are equal bit for bit"""
    case, (design, wide) = p
    run_conv2d_fwd(ops, case, design, wide, also_conv3x3=(case[5], case[6]) == (3, 1))


@pytest.mark.parametrize("p", POOL, ids=pid)
def test_conv2d_fwd_pool(ops, p):
    case, (design, wide), same = p
    B, H, W, Cin, Cout, k, stride, _ = case
    r = strict.mx_fwd_design(case, design, wide)
    Hp, Wp = ((H + 1) // 2, (W + 1) // 2) if same else (H // 2, W // 2)
    pr, _ = strict.ref_pool(r["y_relu"].float(), 2, 2, 0, 0, Hp, Wp, 4)       # on the bf16-rounded conv map
    pr = pr.to(BF)
    qr, sr = strict.ref_quantize_mx(pr)
    a, xq, xs, wq, ws, bias = fwd_operands(ops, r)
    o, q, sc = a.out((B, Hp, Wp, Cout), BF, "y_pool"), a.out((B, Hp, Wp, Cout), U8, "y_pool8"), a.out((B, Hp, Wp, Cout // 32), U8, "y_pool_scale")
    args = (xq, xs, wq, ws, bias, 1, 1, 1, H, W, True, same)
    a.run(lambda: ops.conv2d_fwd_pool_mxfp8(*args, want_bf16=True, want_fp8=True, out=o, out_q=q, out_scale=sc), [(o, pr), (q, qr), (sc, sr)])
    a.run(lambda: ops.conv2d_fwd_pool_mxfp8(*args, want_bf16=False, want_fp8=True, out_q=q, out_scale=sc), [(q, qr), (sc, sr)])
    a.run(lambda: ops.conv2d_fwd_pool_mxfp8(*args, out=o), [(o, pr)])


@pytest.mark.parametrize("p", DGRAD, ids=pid)
def test_conv2d_bwd_data(ops, p):
    case, (design, wide) = p
    B, H, W, Cin, Cout, k, stride, _ = case
    r = strict.mx_dgrad_design(case, design, wide)
    Ho, Wo, pt, pl = r["geom"]
    a = arena_for(r["dy"], r["w_t"], r["dx64"], r["dx64"])
    dyq, dys = put_mx(ops, a, r["dy"], r["dy_q"], r["dy_s"], r["dy_s"], "dy")
    wtq, wts = put_mx(ops, a, r["w_t"], r["w_t_q"], r["w_t_s"], r["w_t_s_op"], "w_t")
    mask = a.put(r["mask_src"], "relu_src")
    dx, q, sc = a.out((B, H, W, Cin), BF, "dx"), a.out((B, H, W, Cin), U8, "dx8"), a.out((B, H, W, Cin // 32), U8, "dxscale")
    args, shape = (dyq, dys, wtq, wts), (B, H, W, Cin)
    for src, name in ((None, "dx"), (mask, "dx_masked")):
        want = r[name]
        qr, sr = strict.ref_quantize_mx(want)
        a.run(lambda: ops.conv2d_bwd_data_mxfp8(*args, src, shape, 1, pt, pl, want_bf16=True, want_fp8=True, out=dx, out_q=q, out_scale=sc),
              [(dx, want), (q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_bwd_data_mxfp8(*args, src, shape, 1, pt, pl, want_bf16=False, want_fp8=True, out_q=q, out_scale=sc),
              [(q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_bwd_data_mxfp8(*args, src, shape, 1, pt, pl, out=dx), [(dx, want)])
    acc = a.inout(r["base"], "dx (accumulated onto)")
    want = r["dx_acc"]
    qr, sr = strict.ref_quantize_mx(want)
    a.run(lambda: ops.conv2d_bwd_data_mxfp8(*args, mask, shape, 1, pt, pl, accumulate=True, want_bf16=True, want_fp8=True, out=acc,
                                            out_q=q, out_scale=sc), [(acc, want), (q, qr), (sc, sr)])


def test_add_relu(ops):
    shape = (3, 17, 19, 256)
    r = strict.mx_eltwise_case(shape)
    want = r["out"].to(BF)
    qr, sr = strict.ref_quantize_mx(want)
    a = arena_for(r["a"], r["b"], r["out"])
    x, y = a.put(r["a"], "a"), a.put(r["b"], "b")
    out, q, sc = a.out(shape, BF, "out"), a.out(shape, U8, "q"), a.out(shape[:-1] + (shape[-1] // 32,), U8, "scale")
    a.run(lambda: ops.add_relu_fwd_mxfp8(x, y, out=out, q=q, scale=sc), [(out, want), (q, qr), (sc, sr)])


# ---------------------------------------------------------------- the quantiser over its whole domain
MULT = (-1.0, 0.5, 0.46875, 0.4375, 2.0 ** -4, 2.0 ** -9, 0.0, -0.0, 0.3)


def amax_sweep():
    """[65280, 32] bf16: block i has the i-th finite bf16 pattern v as element 0 (its maximum); the others are v times MULT rounded
    to bf16 -- -1, ties and their neighbours on the e4m3 grid, e4m3 subnormals and underflow, 0.3 -- and literal +0 / -0; the
    second and third pass over MULT with the other sign, so every factor meets several byte positions of the packed words"""
    bits = torch.arange(1 << 16, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    v = bits.to(torch.int16).view(BF).float()
    assert v.numel() == 65280 and bool(torch.isfinite(v).all())
    cols = [v]
    for j in range(31):
        m = MULT[j % len(MULT)]
        col = (v * (m if (j // len(MULT)) % 2 == 0 else -m)).to(BF).float()
        if m == 0.0:                                        # literal zeros of both signs, whatever v's sign
            col = torch.full_like(v, m if (j // len(MULT)) % 2 == 0 else -m)
        cols.append(col)
    return torch.stack(cols, 1).to(BF)


def test_quantize_every_block_maximum(ops):
    t = amax_sweep()
    qr, sr = strict.ref_quantize_mx(t)
    assert int(sr.min()) == 0 and int(sr.max()) == 247 and len(sr.unique()) == 248          # the clamp at byte 0; e = +120
    a = arena_for(t, t)
    src = a.put(t, "blocks")
    q, s = a.out(tuple(t.shape), U8, "q"), a.out((t.shape[0], 1), U8, "scale")
    a.run(lambda: ops.quantize_mx_fp8(src, q=q, scale=s), [(q, qr), (s, sr)])


def zero_gradient(a, pixels, cout=128, cin=64):
    """MX operands of an all-zero 1x1 data gradient over `pixels` pixels: with accumulate, dx = 0 + base"""
    return (a.put(torch.zeros((1, 1, pixels, cout), dtype=U8), "dy q"), a.put(torch.full((1, 1, pixels, cout // 32), 127, dtype=U8), "dy scale"),
            a.put(torch.zeros((cin, 1, 1, cout), dtype=U8), "w_t q"), a.put(torch.full((cin, 1, 1, cout // 32), 127, dtype=U8), "w_t scale"))


def test_fused_quantisers_on_every_block_maximum(ops):
    """mx_block_exp / mx_pack4 inside k_add_relu_mxfp8 on relu(sweep + 0) -- the ReLU leaves every |v| as a block maximum, under
    the -1 factor where v < 0 -- and inside the data-gradient epilogue on all of the sweep: a zero gradient accumulated onto it"""
    t = amax_sweep()
    want = (t.float() + 0.0).relu().to(BF)
    qr, sr = strict.ref_quantize_mx(want)
    assert len(sr.unique()) == 248
    a = arena_for(t, t, t, t)
    x, z = a.put(t, "blocks"), a.put(torch.zeros_like(t), "zeros")
    out, q, s = a.out(tuple(t.shape), BF, "out"), a.out(tuple(t.shape), U8, "q"), a.out((t.shape[0], 1), U8, "scale")
    a.run(lambda: ops.add_relu_fwd_mxfp8(x, z, out=out, q=q, scale=s), [(out, want), (q, qr), (s, sr)])

    shape = (1, 1, t.shape[0] // 2, 64)                     # two blocks per pixel: both block columns of a wave
    base = t.view(shape)
    want = (base.float() + 0.0).to(BF)                      # -0 + 0 = +0
    qr, sr = strict.ref_quantize_mx(want)
    b = arena_for(base, base, base, base, base)
    args = zero_gradient(b, shape[2])
    acc = b.inout(base, "dx (accumulated onto)")
    q, s = b.out(shape, U8, "dx8"), b.out(shape[:3] + (2,), U8, "dxscale")
    b.run(lambda: ops.conv2d_bwd_data_mxfp8(*args, None, shape, 1, 0, 0, accumulate=True, want_bf16=True, want_fp8=True, out=acc,
                                            out_q=q, out_scale=s), [(acc, want), (q, qr), (s, sr)])


def nonfinite_blocks(values):
    """[3 len(values) + 2, 96] bf16: the leading rows hold one non-finite value in the first, a middle or the last position of
    their MIDDLE block; the blocks around it and the last two rows are finite and must come out as if nothing had happened"""
    g = torch.Generator().manual_seed(11)
    rows = 3 * len(values) + 2
    t = strict.ints(g, (rows, 96), (-3, -2, -1, 1, 2, 3), scale=0.25)
    bad = torch.zeros((rows, 3), dtype=torch.bool)
    for i, value in enumerate(values):
        for j, pos in enumerate((0, 13, 31)):
            t[3 * i + j, 32 + pos] = value
            bad[3 * i + j, 1] = True
    return t, bad


def check_nonfinite_rule(ops, q, s, bad, t):
    """the rule of csrc/mxfp8.h: a block with a NaN or an infinity dequantises to at least one NaN, no scale byte is 255"""
    q, s = q.cpu().view(t.shape), s.cpu().view(bad.shape)
    deq = ops.dequantize_mx_fp8(q, s).view(*bad.shape, 32)
    assert bool(torch.isnan(deq[bad]).any(-1).all()) and int(bad.sum()) > 0
    assert not bool((s == 255).any())
    assert torch.equal(deq[~bad], t.float().view(*bad.shape, 32)[~bad])               # finite blocks are untouched


NAN, INF = float("nan"), float("inf")


def test_quantize_non_finite(ops):
    t, bad = nonfinite_blocks((NAN, INF, -INF))
    qr, sr = strict.ref_quantize_mx(t)
    check_nonfinite_rule(ops, qr, sr, bad, t)
    a = arena_for(t, t)
    src = a.put(t, "blocks")
    q, s = a.out(tuple(t.shape), U8, "q"), a.out(tuple(bad.shape), U8, "scale")
    gq, gs = a.run(lambda: ops.quantize_mx_fp8(src, q=q, scale=s), [(q, qr), (s, sr)])
    check_nonfinite_rule(ops, gq, gs, bad, t)


def test_fused_quantisers_non_finite(ops):
    """the same rule behind the data-gradient epilogue (a zero gradient accumulated onto the non-finite map) and behind add +
    ReLU, where only +inf reaches the quantiser: fmaxf(NaN, 0) = 0 and relu(-inf) = 0, as in add_relu_fwd"""
    t, bad = nonfinite_blocks((INF, -INF))
    shape = (1, 1, t.shape[0], 96)
    qr, sr = strict.ref_quantize_mx(t)
    a = arena_for(t, t, t)
    args = zero_gradient(a, t.shape[0], cin=96)
    acc = a.inout(t.view(shape), "dx (accumulated onto)")
    q, s = a.out(shape, U8, "dx8"), a.out(shape[:3] + (3,), U8, "dxscale")

    def dgrad(out, out_q, out_scale):
        return ops.conv2d_bwd_data_mxfp8(*args, None, shape, 1, 0, 0, accumulate=True, want_bf16=True, want_fp8=True, out=out,
                                         out_q=out_q, out_scale=out_scale)
    _, gq, gs = a.run(lambda: dgrad(acc, q, s), [(acc, t.view(shape)), (q, qr.view(shape)), (s, sr.view(shape[:3] + (3,)))])
    check_nonfinite_rule(ops, gq, gs, bad, t)

    # NaN: torch.equal cannot compare the bf16 map, so this launch runs on plain tensors; the bytes are still compared exactly
    tn, badn = nonfinite_blocks((NAN,))
    shape_n = (1, 1, tn.shape[0], 96)
    qr, sr = strict.ref_quantize_mx(tn)
    dev = acc.device
    argsn = (torch.zeros((1, 1, tn.shape[0], 128), dtype=U8, device=dev), torch.full((1, 1, tn.shape[0], 4), 127, dtype=U8, device=dev),
             torch.zeros((96, 1, 1, 128), dtype=U8, device=dev), torch.full((96, 1, 1, 4), 127, dtype=U8, device=dev))
    accn = tn.view(shape_n).to(dev)
    _, gq, gs = ops.conv2d_bwd_data_mxfp8(*argsn, None, shape_n, 1, 0, 0, accumulate=True, want_bf16=True, want_fp8=True, out=accn)
    assert torch.equal(gq.cpu().view(tn.shape), qr) and torch.equal(gs.cpu().view(badn.shape), sr)
    assert torch.equal(accn.cpu().view(tn.shape).float().nan_to_num(nan=12345.0), tn.float().nan_to_num(nan=12345.0))
    check_nonfinite_rule(ops, gq, gs, badn, tn)

    ti, badi = nonfinite_blocks((INF,))
    qr, sr = strict.ref_quantize_mx(ti)
    b = arena_for(ti, ti, ti, ti)
    x, z = b.put(ti.relu(), "a"), b.put(torch.zeros_like(ti), "b")
    out, q2, s2 = b.out(tuple(ti.shape), BF, "out"), b.out(tuple(ti.shape), U8, "q"), b.out(tuple(badi.shape), U8, "scale")
    qr, sr = strict.ref_quantize_mx(ti.relu())
    _, gq, gs = b.run(lambda: ops.add_relu_fwd_mxfp8(x, z, out=out, q=q2, scale=s2), [(out, ti.relu()), (q2, qr), (s2, sr)])
    check_nonfinite_rule(ops, gq, gs, badi, ti.relu())
