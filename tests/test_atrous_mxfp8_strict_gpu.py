"""GPU: ssd_conv2d_atrous_fwd_mxfp8 (the dilated fc6 of the VGG-16 SSD300's inference fp8 forward) under the strict harness of
tests/test_mxfp8_strict_gpu.py: arena, guard bands, two poisons, every comparison torch.equal, operands whose block scales
DIFFER (designs A "cancelling" and B "block-isolated" of tests/strict.py, one wide-A case) and that ssd_quantize_mx_fp8 first
reproduces through the arena.  Expectation: the float64 oracle of tests/atrous_oracle.py (Keras Conv2D(3, dilation_rate=d,
padding="same")) rounded ONCE to bf16, and strict.ref_quantize_mx of that for the fp8 pair.  The exact-arithmetic precondition
(every term a multiple of the grid, absolute sums below 2^24 grid) is asserted on the reference, never on what a kernel returned.

Cases (B, H, W, Cin, Cout, d) and what each can catch:
  (1,7,7,128,64,6)       only the corner taps reach the map
  (2,5,5,128,96,1)       d = 1: equality with conv2d_fwd_mxfp8 (k = 3, stride 1, pads 1) bit for bit
  (1,10,10,128,64,12)    d beyond the map: the centre tap alone
  (2,13,11,256,160,2)    two k-steps per tap, a Cout tail tile
  (3,19,19,128,96,6)     a pixel tail tile, images sharing a tile
  (2,13,5,128,64,6)      W <= d < H: one live column of taps
  (1,19,19,512,1024,6)   fc6's own channels"""
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import atrous_oracle as AO                                                            # noqa: E402
from tests import strict                                                                         # noqa: E402

BF, U8, F64 = torch.bfloat16, torch.uint8, torch.float64
CASES = [(1, 7, 7, 128, 64, 6), (2, 5, 5, 128, 96, 1), (1, 10, 10, 128, 64, 12), (2, 13, 11, 256, 160, 2), (3, 19, 19, 128, 96, 6),
         (2, 13, 5, 128, 64, 6), (1, 19, 19, 512, 1024, 6)]
WIDE_CASE = CASES[3]
PARAMS = [(c, d, False) for c in CASES for d in ("A", "B")] + [(WIDE_CASE, "A", True)]


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def pid(p):
    return "%s %s%s" % (str(p[0]).replace(" ", ""), p[1], " wide" if p[2] else "")


@functools.lru_cache(maxsize=None)
def design(case, which, wide):
    """strict.mx_fwd_design for the dilated convolution: conv_operands' integers under design A or B, the float64 oracle and the
    expected bf16 maps; `bound` = the largest sum of |terms| over the grid.  Cached: treat as read-only."""
    B, H, W, Cin, Cout, d = case
    c8 = (B, H, W, Cin, Cout, 3, 1, "same")
    o = strict.conv_operands(c8)
    g = strict._design_gen(c8, which, wide, 16 + d)
    w_int = o["w"] if which == "A" else strict.isolated_filters(g, (Cout, 3, 3, Cin), 9 * Cin)
    m = strict.mx_design_operands(o["x"], w_int, which, wide, g)
    r = dict(case=case, design=which, wide=wide, grid=m["grid"], bias=o["bias"], x=m["a"], w=m["f"], x_q=m["a_q"], x_s=m["a_s"],
             w_q=m["f_q"], w_s=m["f_s"], w_s_op=m["f_s_op"])
    r["y64"] = AO.ref_atrous(r["x"], r["w"], r["bias"], d, False, F64)
    r["bound"] = float(AO.ref_atrous(r["x"].abs(), r["w"].abs(), r["bias"].abs(), d, False, F64).max()) / r["grid"]
    strict.check_mx_regime(r)
    r["y"], r["y_relu"] = strict._to_bf16_once(r["y64"]), strict._to_bf16_once(r["y64"].relu())
    return r


def arena_for(*tensors):
    total = sum(t.numel() * t.element_size() for t in tensors)
    return strict.Arena("cuda", 8 * total + 48 * (2 * strict.GUARD + 2 * strict.ALIGN))


def put_mx(ops, a, t, q_ref, s_ref, s_op, name):
    """the reference's bytes and scales as a kernel operand -- after ssd_quantize_mx_fp8 (through the arena) has reproduced them"""
    src = a.put(t, name + " (bf16)")
    q, s = a.out(tuple(t.shape), U8, name + " q"), a.out(tuple(s_ref.shape), U8, name + " scale")
    a.run(lambda: ops.quantize_mx_fp8(src, q=q, scale=s), [(q, q_ref), (s, s_ref)])
    assert torch.equal(ops.dequantize_mx_fp8(q_ref, s_op), t.float())
    return a.put(q_ref, name + " q (operand)"), a.put(s_op, name + " scale (operand)")


@pytest.mark.parametrize("p", PARAMS, ids=pid)
def test_atrous_fwd(ops, p):
    """the three output combinations, ReLU on and off; at d = 1 conv2d_fwd_mxfp8 against the same expectation"""
    case, which, wide = p
    B, H, W, Cin, Cout, d = case
    r = design(case, which, wide)
    # the designs do their work: the expected map is dense and its blocks carry several scales
    qy, sy = strict.ref_quantize_mx(r["y"]) if Cout % 32 == 0 else (None, None)
    assert float((r["y"] != 0).float().mean()) >= 0.9 and (sy is None or len(sy.unique()) >= 3)
    a = arena_for(r["x"], r["w"], r["y64"], r["y64"])
    xq, xs = put_mx(ops, a, r["x"], r["x_q"], r["x_s"], r["x_s"], "x")
    wq, ws = put_mx(ops, a, r["w"], r["w_q"], r["w_s"], r["w_s_op"], "w")
    bias = a.put(r["bias"], "bias")
    y, q, sc = a.out((B, H, W, Cout), BF, "y"), a.out((B, H, W, Cout), U8, "y8"), a.out((B, H, W, Cout // 32), U8, "yscale")
    for relu in (True, False):
        yr = r["y_relu" if relu else "y"]
        qr, sr = strict.ref_quantize_mx(yr)
        args = (xq, xs, wq, ws, bias, d, relu)
        a.run(lambda: ops.conv2d_atrous_fwd_mxfp8(*args, want_bf16=True, want_fp8=True, out=y, out_q=q, out_scale=sc),
              [(y, yr), (q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_atrous_fwd_mxfp8(*args, want_bf16=False, want_fp8=True, out_q=q, out_scale=sc), [(q, qr), (sc, sr)])
        a.run(lambda: ops.conv2d_atrous_fwd_mxfp8(*args, out=y), [(y, yr)])
        if d == 1:
            a.run(lambda: ops.conv2d_fwd_mxfp8(xq, xs, wq, ws, bias, 1, 1, 1, H, W, relu, want_bf16=True, want_fp8=True, out=y, out_q=q,
                                               out_scale=sc), [(y, yr), (q, qr), (sc, sr)])


def test_dilation_one_equals_the_plain_kernel_on_arbitrary_bytes(ops):
    """... and on operands that are NOT exact -- random e4m3 bytes (no NaN byte) under random scales, so fp32 sums round and the
    order of the k-steps shows: still bit for bit, with and without dead rows of taps (H = 1)."""
    g = torch.Generator().manual_seed(77)
    for B, H, W, Cin, Cout in ((2, 9, 7, 256, 160), (3, 1, 11, 128, 96)):
        def rand8(shape):
            t = torch.randint(0, 256, shape, generator=g, dtype=torch.int32)
            return torch.where((t & 0x7F) == 0x7F, t & 0x80, t).to(U8).cuda()
        xq, wq = rand8((B, H, W, Cin)), rand8((Cout, 3, 3, Cin))
        xs = torch.randint(120, 131, (B, H, W, Cin // 32), generator=g).to(U8).cuda()
        ws = torch.randint(118, 126, (Cout, 3, 3, Cin // 32), generator=g).to(U8).cuda()
        bias = torch.randn((Cout,), generator=g).cuda()
        want = ops.conv2d_fwd_mxfp8(xq, xs, wq, ws, bias, 1, 1, 1, H, W, True, want_bf16=True, want_fp8=True)
        got = ops.conv2d_atrous_fwd_mxfp8(xq, xs, wq, ws, bias, 1, True, want_bf16=True, want_fp8=True)
        assert bool(torch.isfinite(want[0].float()).all()) and float(want[0].float().abs().max()) > 0
        for a_, b_ in zip(got, want):
            assert torch.equal(a_, b_), strict.first_diff(a_, b_)


def test_refusals_leave_the_outputs_untouched(ops):
    a = strict.Arena("cuda", 64 << 20)
    B, H, W = 1, 4, 4

    def operands(Cin, Cout):
        return (a.put(torch.zeros((B, H, W, Cin), dtype=U8), "x q"), a.put(torch.full((B, H, W, max(Cin // 32, 1)), 127, dtype=U8), "x scale"),
                a.put(torch.zeros((Cout, 3, 3, Cin), dtype=U8), "w q"), a.put(torch.full((Cout, 3, 3, max(Cin // 32, 1)), 127, dtype=U8), "w scale"))
    ok, cin64, cout40 = operands(128, 64), operands(64, 64), operands(128, 40)
    y, q, sc = a.out((B, H, W, 64), BF, "y"), a.out((B, H, W, 64), U8, "y8"), a.out((B, H, W, 2), U8, "yscale")
    y40, q40, sc40 = a.out((B, H, W, 40), BF, "y40"), a.out((B, H, W, 40), U8, "y8 40"), a.out((B, H, W, 1), U8, "yscale 40")
    L = ops._lib.lib()

    def refused():
        with pytest.raises(NotImplementedError):                       # Cin % 128
            ops.conv2d_atrous_fwd_mxfp8(*cin64, None, 6, True, want_bf16=True, want_fp8=True, out=y, out_q=q, out_scale=sc)
        with pytest.raises(NotImplementedError):                       # an fp8 output of 40 channels
            ops.conv2d_atrous_fwd_mxfp8(*cout40, None, 6, True, want_bf16=True, want_fp8=True, out=y40, out_q=q40, out_scale=sc40)
        with pytest.raises(ValueError):                                # dilation 0
            ops.conv2d_atrous_fwd_mxfp8(*ok, None, 0, True, want_bf16=True, want_fp8=True, out=y, out_q=q, out_scale=sc)
        p = [ops._ptr(t) for t in ok]
        assert L.ssd_conv2d_atrous_fwd_mxfp8(*p, None, ops._ptr(y), ops._ptr(q), None, B, H, W, 128, 64, 6, 1, ops._stream()) == ops._lib.SSD_ERR_VALUE
        assert L.ssd_conv2d_atrous_fwd_mxfp8(*p, None, None, None, None, B, H, W, 128, 64, 6, 1, ops._stream()) == ops._lib.SSD_ERR_VALUE
    a.run(refused, [])
    # ... and the same call with nothing wrong writes all three (zeros: relu(0 + no bias))
    qz, sz = strict.ref_quantize_mx(torch.zeros((B, H, W, 64), dtype=BF))
    a.run(lambda: ops.conv2d_atrous_fwd_mxfp8(*ok, None, 6, True, want_bf16=True, want_fp8=True, out=y, out_q=q, out_scale=sc),
          [(y, torch.zeros((B, H, W, 64), dtype=BF)), (q, qz), (sc, sz)])


def test_realistic_operands_within_the_family_bound(ops):
    """random bf16 operands of tests/atrous_oracle.realistic_case (x = relu(randn), He filters): the project's rule for this
    kernel family, 2^-7 of the tensor maximum against the fp32 convolution of the DEQUANTISED operands -- what is left is the
    summation order and the one bf16 rounding; the quantisation error itself is stated at network level"""
    B, H, W, Cin, Cout, d = AO.REALISTIC
    r = AO.realistic_case()
    xq, xs = ops.quantize_mx_fp8(r["x"].cuda())
    wq, ws = ops.quantize_mx_fp8(r["w"].cuda())
    bias = r["bias"].cuda()
    y = ops.conv2d_atrous_fwd_mxfp8(xq, xs, wq, ws, bias, d, True)
    ya = AO.ref_atrous(ops.dequantize_mx_fp8(xq, xs).cpu(), ops.dequantize_mx_fp8(wq, ws).cpu(), r["bias"], d, True, torch.float32)
    err, top = float((y.float().cpu() - ya).abs().max()), float(ya.abs().max())
    print("atrous mxfp8 vs fp32 on the dequantised operands: max error %.5f, tensor maximum %.3f" % (err, top))
    assert err <= 2 ** -7 * max(1.0, top), (err, top)
    # and against the float64 oracle of the bf16 operands, the quantisation error of one layer, reported
    e64 = float((y.double().cpu() - r["y_relu"]).norm() / r["y_relu"].norm())
    print("relative L2 against the float64 oracle of the bf16 operands: %.4f" % e64)
