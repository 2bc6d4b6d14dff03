"""GPU: the depthwise 3x3 convolution (ssd_dwconv3x3_*) under the strict harness (tests/strict.py), through ops.

Operands of the exact cases are small integers (tests/depthwise_oracle.py), so every expected output is exact whatever the
summation order or the slab count: each comparison is torch.equal against the CPU reference, whose regime
tests/test_depthwise_cpu.py asserts.  Inputs, outputs and the workspace live in strict.Arena: guards touching each tensor, a
workspace of exactly the bytes the query asks for, every call under two poisons -- a run-to-run difference is a finding.

A lane owns 8 channels of one pixel column and walks a strip of 8 rows (4 in the weight gradient); lanes run over channel groups,
then columns, then strips, then images.  Cases (B, H, W, C, stride, padding) and what each can catch:
  (1, 1, 1, 8, 1, same)       the centre tap alone: every other tap, and both halo rows of the strip, lie outside the map
  (1, 2, 9, 8, 1, same)       a map thinner than the window: a row is above AND below the map's edge at once
  (2, 5, 7, 24, 1, same)      H != W; C no multiple of 16: three lanes per pixel, so no power of two divides the wave
  (3, 19, 19, 64, 1, same)    odd map; strips of 8, 8 and 3 rows; waves that cross rows, strips and image boundaries
  (1, 4, 6, 520, 1, same)     65 channel groups: a pixel spans more than one wave; the weight gradient's workgroup is 65 x 7 = 455
                              threads, no multiple of a wave
  (2, 10, 10, 40, 2, same)    even map at stride 2: asymmetric padding 0 / 1, input rows of either parity under one strip
  (2, 19, 19, 72, 2, same)    odd map at stride 2, padding 1 / 1
  (2, 10, 10, 40, 2, pad1)    torch-style padding 1 / 0 on the same map: the other parity of every tap
  (4, 38, 38, 32, 1, same)    MobileNet's narrow early layers: four lanes per pixel, 16 pixels per wave
  (2, 75, 75, 32, 2, same)    ... at stride 2, ten strips per column
  (3, 11, 13, 64, 1, same)    weight-gradient slabs: 8 channel groups, so 32 column strips side by side, one each: a slab is 32
                              strips; 11 rows are 3 strips of 4 rows, 3 * 3 * 13 = 117 strips = slabs of 32, 32, 32 and 21: four
                              slabs, the last one partial"""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                                                                   # noqa: E402
from tests.conv_cases import WS_BYTES                                                                      # noqa: E402
from tests.depthwise_oracle import CASES, REALISTIC, SEPARABLE, dw_case, realistic_case, separable_case     # noqa: E402

BF, F32 = torch.bfloat16, torch.float32


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


@pytest.mark.parametrize("case", CASES, ids=str)
def test_depthwise_strict(ops, L, case):
    """forward with and without ReLU; data gradient plain, masked, accumulated + masked onto an in-out tensor, and with relu_src
    stored in dx's place; weight gradient with and without dbias"""
    B, H, W, C, stride, padding = case
    r = dw_case(case)
    strict.check_regime(r)
    Ho, Wo, pt, pl = r["geom"]
    need = L.ssd_dwconv3x3_bwd_weight_workspace_bytes(B, H, W, C, stride, Ho, Wo)
    assert need > 0
    a = arena_for(r, 2 * need)
    x, w, bias = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias")
    dy, mask = a.put(r["dy"], "dy"), a.put(r["mask_src"], "relu_src")
    ws = a.workspace()
    y = a.out((B, Ho, Wo, C), BF, "y")
    for relu in (True, False):
        a.run(lambda: ops.dwconv3x3_fwd(x, w, bias, stride, pt, pl, Ho, Wo, relu, out=y), [(y, r["y_relu" if relu else "y"].to(BF))])
    a.run(lambda: ops.dwconv3x3_fwd(x, w, None, stride, pt, pl, Ho, Wo, False, out=y), [(y, (r["y"] - r["bias"]).to(BF))])
    dx = a.out((B, H, W, C), BF, "dx")
    a.run(lambda: ops.dwconv3x3_bwd_data(dy, w, None, (B, H, W, C), stride, pt, pl, out=dx), [(dx, r["dx"].to(BF))])
    a.run(lambda: ops.dwconv3x3_bwd_data(dy, w, mask, (B, H, W, C), stride, pt, pl, out=dx), [(dx, r["dx_masked"].to(BF))])
    acc = a.inout(r["base"], "dx (accumulated onto)")
    a.run(lambda: ops.dwconv3x3_bwd_data(dy, w, mask, (B, H, W, C), stride, pt, pl, accumulate=True, out=acc), [(acc, r["dx_acc"].to(BF))])
    act = a.inout(r["mask_src"], "activation, overwritten by dx")
    a.run(lambda: ops.dwconv3x3_bwd_data(dy, w, act, (B, H, W, C), stride, pt, pl, out=act), [(act, r["dx_masked"].to(BF))])
    dw, db = a.out((3, 3, C), F32, "dw"), a.out((C,), F32, "dbias")
    a.run(lambda: ops.dwconv3x3_bwd_weight(x, dy, stride, pt, pl, dw=dw, dbias=db, ws=ws), [(dw, r["dw"]), (db, r["dbias"])])
    a.run(lambda: ops.dwconv3x3_bwd_weight(x, dy, stride, pt, pl, dw=dw, want_bias=False, ws=ws), [(dw, r["dw"])])


@pytest.mark.parametrize("case", REALISTIC, ids=str)
def test_depthwise_realistic_operands_within_derived_bounds(ops, L, case):
    """Random bf16 operands against the float64 oracle of those operands; the bounds are derived in
    depthwise_oracle.realistic_case.  The results then go through the arena as their own reference: guards, both poisons,
    run-to-run reproducibility."""
    B, H, W, C, stride, padding = case
    r = realistic_case(case)
    Ho, Wo, pt, pl = r["geom"]
    need = L.ssd_dwconv3x3_bwd_weight_workspace_bytes(B, H, W, C, stride, Ho, Wo)
    a = arena_for(r, 2 * need)
    x, w, bias, dy, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.put(r["dy"], "dy"), a.workspace()
    y, dx = a.out((B, Ho, Wo, C), BF, "y"), a.out((B, H, W, C), BF, "dx")
    dw, db = a.out((3, 3, C), F32, "dw"), a.out((C,), F32, "dbias")

    def within(name, got, bound):
        err = (got.double().cpu() - r[name]).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print("%s: max |error| %.3e, largest error / bound %.3e" % (name, float(err.max()), worst))
        assert bool((err <= bound).all()), (name, worst)

    calls = [
        (lambda: ops.dwconv3x3_fwd(x, w, bias, stride, pt, pl, Ho, Wo, False, out=y), [("y", y, "y_bound")]),
        (lambda: ops.dwconv3x3_fwd(x, w, bias, stride, pt, pl, Ho, Wo, True, out=y), [("y_relu", y, "y_bound")]),
        (lambda: ops.dwconv3x3_bwd_data(dy, w, None, (B, H, W, C), stride, pt, pl, out=dx), [("dx", dx, "dx_bound")]),
        (lambda: ops.dwconv3x3_bwd_weight(x, dy, stride, pt, pl, dw=dw, dbias=db, ws=ws), [("dw", dw, "dw_bound"), ("dbias", db, "dbias_bound")]),
    ]
    for fn, outs in calls:
        fn()
        torch.cuda.synchronize()
        first = [(t, t.detach().clone()) for _, t, _ in outs]
        for (name, _, bound), (_, g) in zip(outs, first):
            within(name, g, r[bound])
        a.run(fn, first)


@pytest.mark.parametrize("case", SEPARABLE, ids=str)
def test_separable_block_equals_autograd_bits(ops, L, case):
    """dwconv3x3_fwd(relu) -> conv2d_fwd (1x1) -> loss gradient -> conv2d_bwd_data(relu_src = the depthwise output) ->
    dwconv3x3_bwd_data and dwconv3x3_bwd_weight, bit for bit against torch autograd: the new operators' mask and padding
    conventions are those of the existing ones they sit between."""
    B, H, W, C, N, stride = case
    r = separable_case(case)
    strict.check_regime(r)
    Ho, Wo, pt, pl = r["geom"]
    need = L.ssd_dwconv3x3_bwd_weight_workspace_bytes(B, H, W, C, stride, Ho, Wo)
    a = arena_for(r, 2 * WS_BYTES, 2 * need)
    x, w1, b1 = a.put(r["x"], "x"), a.put(r["w1"], "w1"), a.put(r["b1"], "b1")
    w2, b2, w2_t, dy2 = a.put(r["w2"], "w2"), a.put(r["b2"], "b2"), a.put(r["w2_t"], "w2_t"), a.put(r["dy2"], "dy2")
    ws = a.workspace()
    y1, y2 = a.out((B, Ho, Wo, C), BF, "y1"), a.out((B, Ho, Wo, N), BF, "y2")
    g1, dx = a.out((B, Ho, Wo, C), BF, "g1"), a.out((B, H, W, C), BF, "dx")
    dw1, db1 = a.out((3, 3, C), F32, "dw1"), a.out((C,), F32, "db1")

    def block():
        ops.dwconv3x3_fwd(x, w1, b1, stride, pt, pl, Ho, Wo, True, out=y1)
        ops.conv2d_fwd(y1, w2, b2, 1, 0, 0, Ho, Wo, False, out=y2, ws=ws)
        ops.conv2d_bwd_data(dy2, w2_t, y1, (B, Ho, Wo, C), 1, 0, 0, out=g1, ws=ws)
        ops.dwconv3x3_bwd_data(g1, w1, None, (B, H, W, C), stride, pt, pl, out=dx)
        ops.dwconv3x3_bwd_weight(x, g1, stride, pt, pl, dw=dw1, dbias=db1, ws=ws)

    a.run(block, [(y1, r["y1"].to(BF)), (y2, r["y2"].to(BF)), (g1, r["g1"].to(BF)), (dx, r["dx"].to(BF)), (dw1, r["dw1"]), (db1, r["db1"])])


def test_refusals_leave_the_outputs_untouched(ops, L):
    """every refusal is decided on the host: the call raises and the poisoned outputs keep their poison"""
    B, H, W, C = 2, 5, 7, 24
    r = dw_case((B, H, W, C, 1, "same"))
    g = torch.Generator().manual_seed(5)
    a = arena_for(r, 1 << 22)
    x, w, bias, dy = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.put(r["dy"], "dy")
    x12 = a.put(strict.ints(g, (B, H, W, 12), (-1, 1)), "x, 12 channels")
    w12 = a.put(strict.ints(g, (3, 3, 12), (-1, 1)), "w, 12 channels")
    ws = a.workspace()
    y, dx = a.out((B, H, W, C), BF, "y"), a.out((B, H, W, C), BF, "dx")
    y12 = a.out((B, H, W, 12), BF, "y, 12 channels")
    y_wrong = a.out((B, H, W + 1, C), BF, "y of the wrong shape")
    y_f32 = a.out((B, H, W, C), F32, "y of the wrong type")
    dw, db = a.out((3, 3, C), F32, "dw"), a.out((C,), F32, "dbias")
    dw12 = a.out((3, 3, 12), F32, "dw, 12 channels")
    dw_wrong = a.out((C, 3, 3), F32, "dw of the wrong shape")
    shape = (B, H, W, C)
    refusals = [
        (NotImplementedError, lambda: ops.dwconv3x3_fwd(x12, w12, None, 1, 1, 1, H, W, True, out=y12)),             # C % 8
        (ValueError, lambda: ops.dwconv3x3_fwd(x, w, bias, 3, 1, 1, H, W, True, out=y)),                            # stride
        (ValueError, lambda: ops.dwconv3x3_fwd(x, w, bias, 1, 2, 1, H, W, True, out=y)),                            # pad_t
        (ValueError, lambda: ops.dwconv3x3_fwd(x, w, bias, 2, 1, 1, H, W, True, out=y)),                            # Ho, Wo break the rule
        (ValueError, lambda: ops.dwconv3x3_fwd(x, w, bias, 1, 1, 1, H, W, True, out=x)),                            # y aliases x
        (ValueError, lambda: ops.dwconv3x3_fwd(x, w, bias, 1, 1, 1, H, W, True, out=y_wrong)),
        (ValueError, lambda: ops.dwconv3x3_fwd(x, w, bias, 1, 1, 1, H, W, True, out=y_f32)),
        (ValueError, lambda: ops.dwconv3x3_fwd(x, w, bias, 1, 1, 1, H, W, True, out=y.permute(0, 2, 1, 3))),        # not contiguous
        (NotImplementedError, lambda: ops.dwconv3x3_bwd_data(x12, w12, None, (B, H, W, 12), 1, 1, 1, out=y12)),
        (ValueError, lambda: ops.dwconv3x3_bwd_data(dy, w, None, shape, 0, 1, 1, out=dx)),
        (ValueError, lambda: ops.dwconv3x3_bwd_data(dy, w, None, shape, 1, 1, 1, out=dy)),                          # dx aliases dy
        (ValueError, lambda: ops.dwconv3x3_bwd_data(dy, w, None, shape, 2, 1, 1, out=dx)),                          # Ho, Wo break the rule
        (ValueError, lambda: ops.dwconv3x3_bwd_data(dy, w, None, shape, 1, 1, 1, out=y_wrong)),
        (NotImplementedError, lambda: ops.dwconv3x3_bwd_weight(x12, x12, 1, 1, 1, dw=dw12, ws=ws, want_bias=False)),
        (ValueError, lambda: ops.dwconv3x3_bwd_weight(x, dy, 3, 1, 1, dw=dw, dbias=db, ws=ws)),
        (ValueError, lambda: ops.dwconv3x3_bwd_weight(x, dy, 1, 1, 1, dw=dw_wrong, dbias=db, ws=ws)),
        (ValueError, lambda: ops.dwconv3x3_bwd_weight(x, dy, 1, 1, 1, dw=dw, dbias=dw, ws=ws)),                     # dbias of the wrong shape
    ]

    def all_refused():
        for exc, call in refusals:
            with pytest.raises(exc):
                call()
    a.run(all_refused, [])
