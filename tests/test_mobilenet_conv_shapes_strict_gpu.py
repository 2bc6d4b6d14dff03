"""GPU: ssd_conv2d_* at the MobileNet-v1 SSD300 trunk's own convolution shapes, under the strict harness (tests/strict.py: small
integer operands, so every comparison is torch.equal; arena, guard bands, two poisons).

The trunk sends shapes through the library that no other network does: the 3x3 / stride-2 stem on 8 (3 + 5 padded) input channels
with 32 filters, 1x1 layers with 32 and 64 input channels (a quarter and a half of a 128-channel k-step), and 1x1 1024 -> 1024 on
the 10x10 map.  Each is run at batch 1 or 2 on the smallest maps that reach the kernels the training batch reaches
(conv_cases.plan_names is the host-side dispatch query; the expected names are written down, so a moved dispatch rule fails
here instead of silently testing another kernel), and on a few odd / even maps at the small-problem kernels the tests' own
batches reach:

  stem 8 -> 32, 3x3 / 2   batch 64 at 300: 256-row LDS-DMA tiles forward and data gradient, wide weight-gradient reduction.
                          (2, 223, 223) reaches the data-gradient tile and the wide reduction, (2, 443, 443) the forward tile
                          (run forward only); (2, 11, 9) and (1, 10, 10): odd and even maps under SAME at stride 2 (padding 1 / 1
                          and 0 / 1)
  1x1 32 -> 64            batch 64 at 150: the same kernels; (2, 223, 223) reaches all three
  1x1 64 -> 128           batch 64 at 75: <256,128> forward, <256,64> data gradient; (2, 223, 223) reaches all three
  1x1 1024 -> 1024        batch 64 at 10: <128,128> without split-K and the tiled weight gradient: (2, 35, 35); (2, 10, 10) is what
                          a batch of 2 runs: split-K forward and data gradient, which carry no sign bytes -- the sign-byte calls
                          must refuse and write nothing

Every case runs forward (with and without ReLU), the data gradient plain and accumulated + masked, the weight gradient with and
without dbias (tests/test_conv_strict_gpu.run_conv_case), then both sign-byte forms: forward with sign bytes, data gradient masked
by sign bytes, plain and accumulated."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                                                         # noqa: E402
from tests.conv_cases import WS_BYTES, plan_names                                                # noqa: E402
from tests.test_conv_strict_gpu import arena_for, run_conv_case                                  # noqa: E402

BF, U8 = torch.bfloat16, torch.uint8
D = "k_conv_igemm_dma<%s>"
CASES = [
    ((2, 223, 223, 8, 32, 3, 2, "same"), (D % "128,64", D % "256,64", "k_conv_wgrad+rwide"), "all"),
    ((2, 443, 443, 8, 32, 3, 2, "same"), (D % "256,64", D % "256,64", "k_conv_wgrad+rwide"), "forward"),
    ((2, 11, 9, 8, 32, 3, 2, "same"), (D % "128,64", D % "128,64", "k_conv_wgrad"), "all"),
    ((1, 10, 10, 8, 32, 3, 2, "same"), (D % "128,64", D % "128,64", "k_conv_wgrad"), "all"),
    ((2, 223, 223, 32, 64, 1, 1, "same"), (D % "256,64", D % "256,64", "k_conv_wgrad+rwide"), "all"),
    ((2, 11, 9, 32, 64, 1, 1, "same"), (D % "128,64", D % "128,64", "k_conv_wgrad"), "all"),
    ((2, 223, 223, 64, 128, 1, 1, "same"), (D % "256,128", D % "256,64", "k_conv_wgrad+rwide"), "all"),
    ((1, 5, 7, 64, 128, 1, 1, "same"), (D % "128,128", D % "128,64", "k_conv_wgrad"), "all"),
    ((2, 35, 35, 1024, 1024, 1, 1, "same"), (D % "128,128", D % "128,128", "k_conv_wgrad_tile"), "all"),
    ((2, 10, 10, 1024, 1024, 1, 1, "same"), (D % "128,128" + "+splitk", D % "128,128" + "+splitk", "k_conv_wgrad"), "all"),
]
# the kernels the trunk's layers resolve to at the training batch: each is reached by a case above
AT_BATCH_64 = [((64, 300, 300, 8, 32, 3, 2, "same"), (D % "256,64", D % "256,64", "k_conv_wgrad+rwide")),
               ((64, 150, 150, 32, 64, 1, 1, "same"), (D % "256,64", D % "256,64", "k_conv_wgrad+rwide")),
               ((64, 75, 75, 64, 128, 1, 1, "same"), (D % "256,128", D % "256,64", "k_conv_wgrad+rwide")),
               ((64, 10, 10, 1024, 1024, 1, 1, "same"), (D % "128,128", D % "128,128", "k_conv_wgrad_tile"))]


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def test_the_cases_reach_the_training_batch_kernels():
    for full, names in AT_BATCH_64:
        assert plan_names(full) == names, full
        mine = [n for c, n, _ in CASES if c[3:] == full[3:]]
        for p in range(3):
            assert any(n[p] == names[p] for n in mine), (full, names[p])


@pytest.mark.parametrize("case,names,what", CASES, ids=[str(c[0]) for c in CASES])
def test_conv_shape_strict(ops, L, case, names, what):
    assert plan_names(case) == names, "the dispatch rules moved: this case no longer tests the kernels it names"
    B, H, W, Cin, Cout, k, stride, mode = case
    r = strict.conv_case(case)
    run_conv_case(ops, L, case, r=r, dgrad=what == "all", wgrad=what == "all")
    # ---- the sign-byte forms
    Ho, Wo, pt, pl = r["geom"]
    a = arena_for(r, 2 * WS_BYTES)
    x, w, bias, ws = a.put(r["x"], "x"), a.put(r["w"], "w"), a.put(r["bias"], "bias"), a.workspace()
    y, bits = a.out((B, Ho, Wo, Cout), BF, "y"), a.out((B, Ho, Wo, Cout // 8), U8, "relu_bits")
    splitk = names[0].endswith("+splitk")

    def refused(fn):
        def call():
            with pytest.raises(NotImplementedError):
                fn()
        return call

    fwd = lambda: ops.conv2d_fwd_relubits(x, w, bias, stride, pt, pl, Ho, Wo, bits, out=y, ws=ws)      # noqa: E731
    if splitk:
        a.run(refused(fwd), [])
    else:
        a.run(fwd, [(y, r["y_relu"].to(BF)), (bits, r["y_bits"])])
    if what != "all" or Cin == 8:
        return                                              # (the stem: no data gradient w.r.t. the image, so none masked by it)
    dyp, w_t, xbits = a.put(r["dy_pad"], "dy"), a.put(r["w_t"], "w_t"), a.put(r["x_bits"], "mask bits")
    dx = a.out((B, H, W, Cin), BF, "dx")
    acc = a.inout(r["base"], "dx (accumulated onto)")
    plain = lambda: ops.conv2d_bwd_data_bits(dyp, w_t, xbits, (B, H, W, Cin), stride, pt, pl, out=dx, ws=ws)      # noqa: E731
    accum = lambda: ops.conv2d_bwd_data_bits(dyp, w_t, xbits, (B, H, W, Cin), stride, pt, pl, accumulate=True, out=acc, ws=ws)   # noqa: E731
    if names[1].endswith("+splitk"):
        a.run(refused(plain), [])
        a.run(refused(accum), [])
        # what the engine then runs: the mask from the bf16 map
        mask = a.put(r["mask_src"], "relu_src")
        a.run(lambda: ops.conv2d_bwd_data(dyp, w_t, mask, (B, H, W, Cin), stride, pt, pl, out=dx, ws=ws), [(dx, r["dx_masked"].to(BF))])
    else:
        a.run(plain, [(dx, r["dx_masked"].to(BF))])
        a.run(accum, [(acc, r["dx_acc"].to(BF))])
