"""GPU: the atrous 3x3 convolution (ssd_conv2d_atrous_*) and the 3x3 / stride-1 max pooling (ssd_maxpool3x3s1_*) under the
strict harness (tests/strict.py), through ops.

Operands of the exact cases are small integers (strict.conv_operands), so every expected output is exact whatever the summation
order, the tile or the slab count: each comparison is torch.equal against the CPU reference of tests/atrous_oracle.py, whose
regime tests/test_atrous_cpu.py asserts.  Inputs, outputs and the workspace live in strict.Arena: guards touching each tensor,
a workspace of exactly the bytes the query asks for, every call under two poisons -- a run-to-run difference is a finding.

The library has ONE forward / data-gradient kernel with ONE tile (128 pixels x 128 channels) and one weight-gradient kernel;
nothing in the dispatch depends on the batch, so the fc6-sized cases run at the smallest batch that still has several pixel
tiles and weight-gradient slabs.

Cases (B, H, W, Cin, Cout, d) and what each can catch:
  (1, 7, 7, 64, 64, 6)        only border pixels see an off-centre tap; one partial pixel tile
  (2, 5, 5, 64, 64, 1)        equals the ordinary 3x3 SAME convolution: also run against ops.conv2d_*, bit for bit
  (1, 10, 10, 64, 64, 12)     d beyond the map: only the centre tap is live; dead taps of dw are written zeros
  (2, 13, 11, 128, 64, 2)     H != W, two k-chunks, rows of a tile cross an image boundary
  (3, 19, 19, 64, 72, 6)      1083 rows (no tile multiple); Cout = Cout_pad = 72: a partial k-chunk in the data gradient
  (5, 19, 19, 128, 136, 6)    several pixel tiles and weight-gradient slabs, partial channel tile
  (2, 19, 19, 512, 1024, 6)   fc6's own channels
  (1, 19, 19, 1024, 512, 6)   the data gradient's orientation at fc6's size
  (2, 13, 5, 64, 64, 6)       W <= d < H: three live taps (the centre column), six dead ones"""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                                                                   # noqa: E402
from tests.atrous_oracle import CASES, POOL_CASES, REALISTIC, atrous_case, pool3x3s1_case, realistic_case   # noqa: E402
from tests.conv_cases import WS_BYTES                                                                      # noqa: E402

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def arena_for(r, *ws_bytes):
    total = sum(v.numel() * v.element_size() for v in r.values() if torch.is_tensor(v))
    return strict.Arena("cuda", 2 * total + sum(ws_bytes) + 64 * (2 * strict.GUARD + 2 * strict.ALIGN))


def bits(t):
    return t.contiguous().view(-1).view({2: torch.int16, 4: torch.int32}[t.element_size()])


def run_atrous_case(ops, L, case, r):
    """forward with and without ReLU; data gradient plain, and accumulated + masked on an in-out tensor; weight gradient with and
    without dbias, dy handed in at ldy = Cout_pad.  Returns the first run's outputs by name."""
    B, H, W, Cin, Cout, d = case
    cp = (Cout + 7) // 8 * 8
    need = L.ssd_conv2d_atrous_bwd_weight_workspace_bytes(B, H, W, Cin, Cout, cp, d)
    assert need > 0
    a = arena_for(r, 2 * need)
    x, w, bias = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias")
    dyp, mask, w_t = a.put(r["dy_pad"], "dy"), a.put(r["mask_src"], "relu_src"), a.put(r["w_t"], "w_t")
    ws = a.workspace()
    got = {}
    y = a.out((B, H, W, Cout), BF, "y")
    for relu in (True, False):
        name = "y_relu" if relu else "y"
        got[name], = a.run(lambda: ops.conv2d_atrous_fwd(x, w, bias, d, relu, out=y), [(y, r[name].to(BF))])
    dx = a.out((B, H, W, Cin), BF, "dx")
    got["dx"], = a.run(lambda: ops.conv2d_atrous_bwd_data(dyp, w_t, None, (B, H, W, Cin), d, out=dx), [(dx, r["dx"].to(BF))])
    got["dx_masked"], = a.run(lambda: ops.conv2d_atrous_bwd_data(dyp, w_t, mask, (B, H, W, Cin), d, out=dx), [(dx, r["dx_masked"].to(BF))])
    acc = a.inout(r["base"], "dx (accumulated onto)")
    got["dx_acc"], = a.run(lambda: ops.conv2d_atrous_bwd_data(dyp, w_t, mask, (B, H, W, Cin), d, accumulate=True, out=acc),
                           [(acc, r["dx_acc"].to(BF))])
    dw, db = a.out((Cout, 3, 3, Cin), F32, "dw"), a.out((Cout,), F32, "dbias")
    got["dw"], got["dbias"] = a.run(lambda: ops.conv2d_atrous_bwd_weight(x, dyp, Cout, d, dw=dw, dbias=db, ws=ws),
                                    [(dw, r["dw"]), (db, r["dbias"])])
    a.run(lambda: ops.conv2d_atrous_bwd_weight(x, dyp, Cout, d, dw=dw, want_bias=False, ws=ws), [(dw, r["dw"])])
    return got


@pytest.mark.parametrize("case", CASES, ids=str)
def test_atrous_strict(ops, L, case):
    r = atrous_case(case)
    strict.check_regime(r)
    run_atrous_case(ops, L, case, r)


def test_atrous_in_place_relu_source_strict(ops, L):
    """relu_src follows the ssd_conv2d_bwd_data contract: the forward activation may be stored in dx's place"""
    B, H, W, Cin, Cout, d = case = (2, 13, 11, 128, 64, 2)
    r = atrous_case(case)
    a = arena_for(r)
    dyp, w_t = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t")
    act = a.inout(r["mask_src"], "activation, overwritten by dx")
    a.run(lambda: ops.conv2d_atrous_bwd_data(dyp, w_t, act, (B, H, W, Cin), d, out=act), [(act, r["dx_masked"].to(BF))])


def test_atrous_dilation_one_equals_conv2d_bits(ops, L):
    """d = 1 is the ordinary 3x3 SAME convolution: the same operands through ops.conv2d_* give the same bits"""
    B, H, W, Cin, Cout, d = case = (2, 5, 5, 64, 64, 1)
    r = atrous_case(case)
    got = run_atrous_case(ops, L, case, r)
    cp = (Cout + 7) // 8 * 8
    a = arena_for(r, 2 * WS_BYTES, 2 * L.ssd_conv2d_bwd_weight_workspace_bytes(B, H, W, Cin, Cout, cp, 3))
    x, w, bias = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias")
    dyp, mask, w_t, ws = a.put(r["dy_pad"], "dy"), a.put(r["mask_src"], "relu_src"), a.put(r["w_t"], "w_t"), a.workspace()
    y, dx = a.out((B, H, W, Cout), BF, "y"), a.out((B, H, W, Cin), BF, "dx")
    acc = a.inout(r["base"], "dx (accumulated onto)")
    dw, db = a.out((Cout, 3, 3, Cin), F32, "dw"), a.out((Cout,), F32, "dbias")
    ref = {}
    ref["y_relu"], = a.run(lambda: ops.conv2d_fwd(x, w, bias, 1, 1, 1, H, W, True, out=y, ws=ws), [(y, r["y_relu"].to(BF))])
    ref["y"], = a.run(lambda: ops.conv2d_fwd(x, w, bias, 1, 1, 1, H, W, False, out=y, ws=ws), [(y, r["y"].to(BF))])
    ref["dx"], = a.run(lambda: ops.conv2d_bwd_data(dyp, w_t, None, (B, H, W, Cin), 1, 1, 1, out=dx, ws=ws), [(dx, r["dx"].to(BF))])
    ref["dx_acc"], = a.run(lambda: ops.conv2d_bwd_data(dyp, w_t, mask, (B, H, W, Cin), 1, 1, 1, accumulate=True, out=acc, ws=ws),
                           [(acc, r["dx_acc"].to(BF))])
    ref["dw"], ref["dbias"] = a.run(lambda: ops.conv2d_bwd_weight(x, dyp, Cout, 3, 1, 1, 1, dw=dw, dbias=db, ws=ws),
                                    [(dw, r["dw"]), (db, r["dbias"])])
    for name, t in ref.items():
        assert torch.equal(bits(t), bits(got[name])), name


def test_atrous_realistic_operands_within_derived_bounds(ops, L):
    """Random bf16 operands against the float64 oracle of those operands; the bounds are derived in atrous_oracle.realistic_case
    and are a few thousand times looser than the exact cases.  The results then go through the arena as their own reference:
    guards, both poisons, run-to-run reproducibility."""
    B, H, W, Cin, Cout, d = REALISTIC
    r = realistic_case()
    cp = (Cout + 7) // 8 * 8
    need = L.ssd_conv2d_atrous_bwd_weight_workspace_bytes(B, H, W, Cin, Cout, cp, d)
    a = arena_for(r, 2 * need)
    x, w, bias = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias")
    dyp, w_t, ws = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t"), a.workspace()
    y, dx = a.out((B, H, W, Cout), BF, "y"), a.out((B, H, W, Cin), BF, "dx")
    dw, db = a.out((Cout, 3, 3, Cin), F32, "dw"), a.out((Cout,), F32, "dbias")

    def within(name, got, bound):
        err = (got.double().cpu() - r[name]).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("%s: max |error| %.3e, largest error / bound %.3e" % (name, float(err.max()), worst))
        assert bool((err <= bound).all()), (name, worst)

    calls = [
        ("y", lambda: ops.conv2d_atrous_fwd(x, w, bias, d, False, out=y), [("y", y, "y_bound")]),
        ("y_relu", lambda: ops.conv2d_atrous_fwd(x, w, bias, d, True, out=y), [("y_relu", y, "y_bound")]),
        ("dx", lambda: ops.conv2d_atrous_bwd_data(dyp, w_t, None, (B, H, W, Cin), d, out=dx), [("dx", dx, "dx_bound")]),
        ("dw", lambda: ops.conv2d_atrous_bwd_weight(x, dyp, Cout, d, dw=dw, dbias=db, ws=ws), [("dw", dw, "dw_bound"), ("dbias", db, "dbias_bound")]),
    ]
    for _, fn, outs in calls:
        fn()
        torch.cuda.synchronize()
        first = [(t, t.detach().clone()) for _, t, _ in outs]
        for (name, _, bound), (_, g) in zip(outs, first):
            within(name, g, r[bound])
        a.run(fn, first)


@pytest.mark.parametrize("shape", POOL_CASES, ids=str)
def test_maxpool3x3s1_strict(ops, L, shape):
    B, H, W, C = shape
    r = pool3x3s1_case(*shape)
    strict.check_regime(r)
    a = arena_for(r)
    x, dy = a.put(r["x"], "x"), a.put(r["dy"], "dy")
    y, code, dx = a.out((B, H, W, C), BF, "y"), a.out((B, H, W, C // 8), I32, "code"), a.out((B, H, W, C), BF, "dx")
    a.run(lambda: ops.maxpool3x3s1_fwd(x, out=y, code=code), [(y, r["y"].to(BF)), (code, strict.pack_codes(r["code"]))])
    codes = a.put(strict.pack_codes(r["code"]), "code (operand)")
    a.run(lambda: ops.maxpool3x3s1_bwd(codes, dy, (B, H, W, C), out=dx), [(dx, r["dx"].to(BF))])


def test_refusals_leave_the_outputs_untouched(ops, L):
    """every refusal is decided on the host: the call raises and the poisoned outputs keep their poison"""
    B, H, W, C = 2, 5, 5, 64
    r = atrous_case((B, H, W, C, C, 1))
    g = torch.Generator().manual_seed(5)
    a = arena_for(r, 1 << 22)
    x, w, bias, dyp, w_t = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t")
    x96 = a.put(strict.ints(g, (B, H, W, 96), (-1, 1)), "x, 96 channels")
    w96 = a.put(strict.ints(g, (C, 3, 3, 96), (-1, 1)), "w, 96 input channels")
    w12 = a.put(strict.ints(g, (12, 3, 3, C), (-1, 1)), "w, 12 filters")
    x12 = a.put(strict.ints(g, (B, H, W, 12), (-1, 1)), "x, 12 channels")
    dy56 = a.put(strict.ints(g, (B, H, W, 56), (-1, 1)), "dy, 56 channels")
    ws = a.workspace()
    y, y12, dx = a.out((B, H, W, C), BF, "y"), a.out((B, H, W, 12), BF, "y, 12 channels"), a.out((B, H, W, C), BF, "dx")
    y_wrong = a.out((B, H, W + 1, C), BF, "y of the wrong shape")
    dw, db = a.out((C, 3, 3, C), F32, "dw"), a.out((C,), F32, "dbias")
    dw96 = a.out((C, 3, 3, 96), F32, "dw, 96 input channels")
    code1 = a.out((B, H, W, 1), I32, "code, 12 channels")
    code, code_wrong = a.out((B, H, W, C // 8), I32, "code"), a.out((B, H, W, C // 8 + 1), I32, "code of the wrong shape")
    refusals = [
        (NotImplementedError, lambda: ops.conv2d_atrous_fwd(x96, w96, bias, 6, True, out=y)),                   # Cin % 64
        (NotImplementedError, lambda: ops.conv2d_atrous_fwd(x, w12, None, 6, True, out=y12)),                   # Cout % 8
        (ValueError, lambda: ops.conv2d_atrous_fwd(x, w, bias, 0, True, out=y)),                                # dilation < 1
        (ValueError, lambda: ops.conv2d_atrous_fwd(x, w, bias, 6, True, out=x)),                                # y aliases x
        (ValueError, lambda: ops.conv2d_atrous_fwd(x, w, bias, 6, True, out=y_wrong)),
        (ValueError, lambda: ops.conv2d_atrous_fwd(x, w, bias, 6, True, out=y.permute(0, 2, 1, 3))),            # not contiguous
        (ValueError, lambda: ops.conv2d_atrous_bwd_data(dyp, w_t, None, (B, H, W, C), 0, out=dx)),
        (ValueError, lambda: ops.conv2d_atrous_bwd_data(dyp, w_t, None, (B, H, W, C), 6, out=dyp)),             # dx aliases dy
        (ValueError, lambda: ops.conv2d_atrous_bwd_data(dyp, w_t, None, (B, H, W, C), 6, out=y_wrong)),
        (NotImplementedError, lambda: ops.conv2d_atrous_bwd_weight(x96, dyp, C, 6, dw=dw96, dbias=db, ws=ws)),  # Cin % 64
        (NotImplementedError, lambda: ops.conv2d_atrous_bwd_weight(x, dy56, C, 6, dw=dw, dbias=db, ws=ws)),     # ldy < Cout
        (ValueError, lambda: ops.conv2d_atrous_bwd_weight(x, dyp, C, 0, dw=dw, dbias=db, ws=ws)),
        (ValueError, lambda: ops.conv2d_atrous_bwd_weight(x, dyp, C, 6, dw=dw96, dbias=db, ws=ws)),             # dw of the wrong shape
        (NotImplementedError, lambda: ops.maxpool3x3s1_fwd(x12, out=y12, code=code1)),                          # C % 8
        (NotImplementedError, lambda: ops.maxpool3x3s1_bwd(code1, x12, (B, H, W, 12), out=y12)),
        (ValueError, lambda: ops.maxpool3x3s1_fwd(x, out=x, code=code)),                                        # y aliases x
        (ValueError, lambda: ops.maxpool3x3s1_fwd(x, out=y, code=code_wrong)),
        (ValueError, lambda: ops.maxpool3x3s1_fwd(x, out=y_wrong, code=code)),
        (ValueError, lambda: ops.maxpool3x3s1_bwd(code, dyp, (B, H, W, C), out=dyp)),                           # dx aliases dy
    ]

    def all_refused():
        for exc, call in refusals:
            with pytest.raises(exc):
                call()
    a.run(all_refused, [])
