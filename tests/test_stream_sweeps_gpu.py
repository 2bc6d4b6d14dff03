"""GPU: the capped stream kernels beyond the first sweep of their grid (tests/sweep_cases.py: the audit, the shapes and their
arithmetic; tests/test_sweep_cases_cpu.py: the constants read back from the sources, and that the references alone tell a
second trip from a repeated first one).

Every case is a small exact case of tests/strict.py's constructors tiled along the batch or flat axis with copy b scaled by
2^(b mod 4), run through ops.* with caller-provided buffers inside strict.Arena: guards, both poisons, every element written,
inputs unchanged, the same bits from both runs.  Every comparison is bit equality against the tiled reference.  The batch-norm
and L2Norm shapes past one sweep ride on tests/test_batchnorm_gpu.py and tests/test_l2norm_gpu.py.

The last test gives the five element-wise and pooling wrappers a too-small, a mis-shaped, a non-contiguous and a wrongly typed
buffer: each must be refused with ValueError before anything is launched."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                                                         # noqa: E402
from tests import sweep_cases as SC                                                              # noqa: E402

BF, U8, I32 = torch.bfloat16, torch.uint8, torch.int32


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def nbytes(t):
    return t.numel() * t.element_size()


def arena_of(*sizes):
    return strict.Arena("cuda", strict.Arena.bytes_for(*sizes))


# ---------------------------------------------------------------------------------------------------- element-wise
def test_add_relu_and_relu_mask_second_trip(ops):
    """ELT_NVEC = 2 097 152 + 256 * 37 + 5 vectors: 37 full workgroups and a 5-lane tail on the second trip; k_add_relu, and
    k_relu_mask writing and accumulating"""
    print(SC.describe("add_relu / relu_mask", SC.walk(SC.ELT_NVEC)))
    r = SC.eltwise_tiled()
    n = r["n"]
    a = arena_of(*([2 * n] * 6))
    x, y, g, act = a.put(r["a"], "a"), a.put(r["b"], "b"), a.put(r["g"], "g"), a.put(r["out"], "act")
    out = a.out((n,), BF, "out")
    a.run(lambda: ops.add_relu_fwd(x, y, out=out), [(out, r["out"])])
    a.run(lambda: ops.relu_mask_bwd(g, act, out=out), [(out, r["masked"])])
    acc = a.inout(r["base"], "out (accumulated onto)")
    a.run(lambda: ops.relu_mask_bwd(g, act, out=acc, accumulate=True), [(acc, r["acc"])])


def test_add_relu_mxfp8_second_trip(ops):
    """MX_NVEC = 2 097 152 + 256 * 37 + 4 vectors: the last four-lane shuffle group is the only live one of its wave"""
    print(SC.describe("add_relu_mxfp8", SC.walk(SC.MX_NVEC)))
    r = SC.mx_eltwise_tiled()
    n, shape = r["n"], tuple(r["out"].shape)
    a = arena_of(2 * n, 2 * n, 2 * n, n, n // 32)
    x, y = a.put(r["a"], "a"), a.put(r["b"], "b")
    out, q, sc = a.out(shape, BF, "out"), a.out(shape, U8, "q"), a.out((shape[0], 1), U8, "scale")
    a.run(lambda: ops.add_relu_fwd_mxfp8(x, y, out=out, q=q, scale=sc), [(out, r["out"]), (q, r["q"]), (sc, r["s"])])


# ---------------------------------------------------------------------------------------------------- pooling
def run_pool(r, fwd, bwd):
    B, H, W, C = r["x"].shape
    Ho, Wo = r["y"].shape[1:3]
    print(SC.describe("forward", SC.walk(B * Ho * Wo * C // 8)))
    print(SC.describe("backward", SC.walk(B * H * W * C // 8)))
    a = arena_of(nbytes(r["x"]), nbytes(r["dy"]), nbytes(r["y"]), nbytes(r["code"]), nbytes(r["dx"]), nbytes(r["code"]))
    x, dy = a.put(r["x"], "x"), a.put(r["dy"], "dy")
    y, code, dx = a.out((B, Ho, Wo, C), BF, "y"), a.out((B, Ho, Wo, C // 8), I32, "code"), a.out((B, H, W, C), BF, "dx")
    a.run(lambda: fwd(x, out=y, code=code), [(y, r["y"]), (code, r["code"])])
    codes = a.put(r["code"], "code (operand)")
    a.run(lambda: bwd(codes, dy, (B, H, W, C), out=dx), [(dx, r["dx"])])


def test_maxpool3x3s2_second_trip(ops):
    """(1,37,50,16) x 2209 images: 2 098 550 forward items (two trips), 8 173 300 backward items (four); y, the codes and dx"""
    run_pool(SC.pool3x3s2_tiled(), ops.maxpool3x3s2_fwd, ops.maxpool3x3s2_bwd)


def test_maxpool3x3s1_second_trip(ops):
    """(1,19,19,64) x 727 images: 2 099 576 items in both passes"""
    run_pool(SC.pool3x3s1_tiled(), ops.maxpool3x3s1_fwd, ops.maxpool3x3s1_bwd)


@pytest.mark.parametrize("ksize", [2, 3])
def test_maxpool_mxfp8_second_trip(ops, ksize):
    """k_maxpool_mxfp8<3> on (1,19,19,64) x 727 images and <2> (SAME, 19 -> 10) x 2622: with and without the bf16 map"""
    r = SC.poolq_tiled(ksize)
    print(SC.describe("maxpool_mxfp8<%d>" % ksize, SC.walk(r["y"].numel() // 8)))
    shape = tuple(r["y"].shape)
    a = arena_of(nbytes(r["x"]), nbytes(r["y"]), nbytes(r["q"]), nbytes(r["s"]))
    src = a.put(r["x"], "x")
    y, q, sc = a.out(shape, BF, "y"), a.out(shape, U8, "q"), a.out(shape[:3] + (shape[3] // 32,), U8, "scale")
    if ksize == 3:
        def call(**kw):
            return ops.maxpool3x3s1_fwd_mxfp8(src, **kw)
    else:
        def call(**kw):
            return ops.maxpool2x2_fwd_mxfp8(src, same=True, **kw)
    a.run(lambda: call(want_bf16=True, out=y, q=q, scale=sc), [(y, r["y"]), (q, r["q"]), (sc, r["s"])])
    a.run(lambda: call(q=q, scale=sc), [(q, r["q"]), (sc, r["s"])])              # (the unlisted bf16 buffer keeps its poison)


# ---------------------------------------------------------------------------------------------------- the stand-alone quantiser
def test_quantize_mx_fp8_second_trip(ops):
    """QUANT_NBLK = 4 194 304 + 256 * 37 + 5 blocks: the ResNet-50 SSD512's fp8 backward quantises two sweeps at batch 64"""
    print(SC.describe("quantize_mx_fp8", SC.walk(SC.QUANT_NBLK, SC.QUANT_CAP)))
    r = SC.quantize_tiled()
    a = arena_of(nbytes(r["x"]), nbytes(r["q"]), nbytes(r["s"]))
    src = a.put(r["x"], "blocks")
    q, s = a.out(tuple(r["q"].shape), U8, "q"), a.out(tuple(r["s"].shape), U8, "scale")
    a.run(lambda: ops.quantize_mx_fp8(src, q=q, scale=s), [(q, r["q"]), (s, r["s"])])


# ---------------------------------------------------------------------------------------------------- the sparse heads' GEMM
def test_sparse_data_gradient_second_trip():
    """SPARSE_SWEEP: 2106 tiles of k_hz_gemm on 2048 workgroups; the second trip holds 40 tiles of level 0's ragged last row
    tile and all of level 1.  The body of tests/test_heads_strict_gpu.py::test_sparse_data_gradient_exact"""
    from ssd_object_detection_amd import _lib
    from tests import test_heads_strict_gpu as HG
    print(SC.describe("k_hz_gemm", SC.walk_hz(SC.SPARSE_SWEEP[0], SC.SPARSE_SWEEP[2])))
    case = SC.sparse_sweep_case()
    L, a, hg, hl, zws, zb, _, _ = HG.setup(_lib, case)

    def fn():
        st = L.ssd_heads_bwd_data_sparse(ctypes.byref(hg.c), ctypes.byref(hl.c), case["B"], HG.ptr(zws), zb, HG.stream())
        assert st == 0, st
    a.run(fn, [(hl.dx[i], l["dx"].to(BF)) for i, l in enumerate(case["levels"])])


# ---------------------------------------------------------------------------------------------------- caller buffers
def wrong_buffers(a, shape, dtype, name):
    """[(label, tensor)]: too small, the right size in another shape, the right shape but not contiguous, another element type"""
    shape = tuple(shape)
    wide = a.out(shape[:-1] + (2 * shape[-1],), dtype, name + " (twice as wide)")
    other = {BF: torch.float16, U8: I32, I32: U8}[dtype]
    return [("too small", a.out(shape[:-1] + (shape[-1] // 2,), dtype, name + " (half)")),
            ("mis-shaped", a.out(shape[-1:] + shape[:-1], dtype, name + " (axes rolled)")),
            ("not contiguous", wide[..., ::2]),
            ("wrong type", a.out(shape, other, name + " (other type)"))]


def test_caller_buffers_are_checked(ops):
    """ops.add_relu_fwd, add_relu_fwd_mxfp8, relu_mask_bwd, maxpool3x3s2_fwd and maxpool3x3s2_bwd refuse a caller's buffer that
    is not the contiguous tensor they write; an arena run with no listed output shows that nothing was written"""
    shape = (2, 9, 11, 64)
    r = strict.eltwise_case(shape)
    p = strict.pool3x3_case(*shape)
    Ho, Wo = p["geom"][:2]
    pooled, cshape, sshape = (2, Ho, Wo, 64), (2, Ho, Wo, 8), shape[:3] + (2,)
    a = strict.Arena("cuda", 96 << 20)
    x, y, g, act = a.put(r["a"], "a"), a.put(r["b"], "b"), a.put(r["g"], "g"), a.put(r["out"].to(BF), "act")
    px, pdy, pcode = a.put(p["x"], "x"), a.put(p["dy"], "dy"), a.put(strict.pack_codes(p["code"]), "code (operand)")
    good = dict(out=a.out(shape, BF, "out"), q=a.out(shape, U8, "q"), scale=a.out(sshape, U8, "scale"),
                y=a.out(pooled, BF, "y"), code=a.out(cshape, I32, "code"))
    acc = a.inout(r["base"], "out (accumulated onto)")
    bad = dict(out=wrong_buffers(a, shape, BF, "out"), q=wrong_buffers(a, shape, U8, "q"), scale=wrong_buffers(a, sshape, U8, "scale"),
               y=wrong_buffers(a, pooled, BF, "y"), code=wrong_buffers(a, cshape, I32, "code"))
    calls = []
    for label, t in bad["out"]:
        calls += [("add_relu_fwd out " + label, lambda t=t: ops.add_relu_fwd(x, y, out=t)),
                  ("relu_mask_bwd out " + label, lambda t=t: ops.relu_mask_bwd(g, act, out=t)),
                  ("relu_mask_bwd accumulate out " + label, lambda t=t: ops.relu_mask_bwd(g, act, out=t, accumulate=True)),
                  ("add_relu_fwd_mxfp8 out " + label, lambda t=t: ops.add_relu_fwd_mxfp8(x, y, out=t, q=good["q"], scale=good["scale"])),
                  ("maxpool3x3s2_bwd out " + label, lambda t=t: ops.maxpool3x3s2_bwd(pcode, pdy, shape, out=t))]
    for label, t in bad["q"]:
        calls.append(("add_relu_fwd_mxfp8 q " + label, lambda t=t: ops.add_relu_fwd_mxfp8(x, y, out=good["out"], q=t, scale=good["scale"])))
    for label, t in bad["scale"]:
        calls.append(("add_relu_fwd_mxfp8 scale " + label, lambda t=t: ops.add_relu_fwd_mxfp8(x, y, out=good["out"], q=good["q"], scale=t)))
    for label, t in bad["y"]:
        calls.append(("maxpool3x3s2_fwd out " + label, lambda t=t: ops.maxpool3x3s2_fwd(px, out=t, code=good["code"])))
    for label, t in bad["code"]:
        calls.append(("maxpool3x3s2_fwd code " + label, lambda t=t: ops.maxpool3x3s2_fwd(px, out=good["y"], code=t)))
    assert len(calls) == 4 * 9

    def refused():
        for label, call in calls:
            try:
                call()
            except ValueError:
                continue
            raise AssertionError("accepted: " + label)
    a.run(refused, [])                                                   # no output listed: every buffer keeps its poison
    # ... and the right buffers are accepted and written
    a.run(lambda: ops.add_relu_fwd(x, y, out=good["out"]), [(good["out"], r["out"].to(BF))])
    a.run(lambda: ops.relu_mask_bwd(g, act, out=acc, accumulate=True), [(acc, r["acc"].to(BF))])
    a.run(lambda: ops.maxpool3x3s2_fwd(px, out=good["y"], code=good["code"]),
          [(good["y"], p["y"].to(BF)), (good["code"], strict.pack_codes(p["code"]))])
