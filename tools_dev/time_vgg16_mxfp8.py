"""Dev: what the VGG-16 SSD300's inference fp8 forward (SSDEngine(..., fp8_inference=True)) costs and saves, on one MI355X, in
one process, by device events.  Every comparison alternates its two forms inside each repeat; reported is the median of
--repeats (7) with min..max beside it.  Kernel operands rotate through sets of more than 256 MiB together, so no launch finds
its operands in the Infinity Cache (inside a forward a layer never does).

(a) fc6's shape (BATCH, 19, 19, 512 -> 1024), dilation 6: ops.conv2d_atrous_fwd_mxfp8 with the output the plan asks of it (the
    fp8 pair only) against ops.conv2d_atrous_fwd; the fp8 launch with a bf16 store besides.
(b) the two quantising poolings at pool4's (BATCH, 38, 38, 512) and pool5's (BATCH, 19, 19, 512) shapes against what they
    replace, the bf16 pooling (its inference form without codes for 2x2, ops.maxpool3x3s1_fwd for 3x3 / 1) followed by
    ops.quantize_mx_fp8.  Bytes a call must move are printed beside the times.
(c) the whole forward and SSDObjectDetectionModel.detect (forward + score / decode + NMS) at each --batches size, mxfp8 against
    bf16 on the same model; the fp8 forward's filter quantisation is timed on its own as well.

usage: python tools_dev/time_vgg16_mxfp8.py [--batches 64,32] [--repeats 7] [--calls 20] [--skip-network]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import ops                            # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,32")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--skip-network", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
BF, U8, CACHE = torch.bfloat16, torch.uint8, 256 << 20


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def spread(name, us, tail=""):
    med = statistics.median(us)
    print("%-58s median %9.1f us   min..max %.1f..%.1f   (%d repeats)%s" % (name, med, min(us), max(us), len(us), tail), flush=True)
    return med


def alternate(variants, nsets, calls=None):
    """variants: {name: fn(i)}, i the running call index (the operand set is i % nsets).  Returns {name: [us per call]}."""
    calls = calls or args.calls

    def timed(fn):
        e0, e1 = events()
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / calls

    for fn in variants.values():
        for i in range(max(2, 2 * nsets)):
            fn(i)
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            us[name].append(timed(fn))
    return us


def nsets_for(per_set):
    return max(2, -(-(CACHE + (32 << 20)) // per_set))


# ---- (a) fc6
def fc6(B):
    H, Cin, Cout, d = 19, 512, 1024, 6
    g = torch.Generator(device="cuda").manual_seed(2)
    w = (torch.randn((Cout, 3, 3, Cin), generator=g, device="cuda") * (2.0 / (9 * Cin)) ** 0.5).to(BF)
    wq, ws = ops.quantize_mx_fp8(w)
    bias = torch.randn((Cout,), generator=g, device="cuda") * 0.1
    per_set = B * H * H * (2 * Cin + 2 * Cout)
    sets = []
    for _ in range(nsets_for(per_set)):
        x = torch.randn((B, H, H, Cin), generator=g, device="cuda").relu().to(BF)
        xq, xs = ops.quantize_mx_fp8(x)
        sets.append(dict(x=x, xq=xq, xs=xs, y=torch.empty((B, H, H, Cout), dtype=BF, device="cuda"), q=ops._mx_pair((B, H, H, Cout), "cuda")))

    def S(i):
        return sets[i % len(sets)]
    variants = {
        "conv2d_atrous_fwd (bf16)": lambda i: ops.conv2d_atrous_fwd(S(i)["x"], w, bias, d, True, out=S(i)["y"]),
        "conv2d_atrous_fwd_mxfp8 -> fp8 pair": lambda i: ops.conv2d_atrous_fwd_mxfp8(S(i)["xq"], S(i)["xs"], wq, ws, bias, d, True, want_bf16=False,
                                                                                   want_fp8=True, out_q=S(i)["q"][0], out_scale=S(i)["q"][1]),
        "conv2d_atrous_fwd_mxfp8 -> bf16 + fp8 pair": lambda i: ops.conv2d_atrous_fwd_mxfp8(S(i)["xq"], S(i)["xs"], wq, ws, bias, d, True, want_bf16=True,
                                                                                          want_fp8=True, out=S(i)["y"], out_q=S(i)["q"][0],
                                                                                          out_scale=S(i)["q"][1]),
    }
    us = alternate(variants, len(sets))
    flops = 2.0 * B * H * H * Cout * 9 * Cin
    print("(a) fc6 at (%d, 19, 19, 512 -> 1024), dilation 6: %d calls per repeat over %d operand sets; %.1f GFLOP with the padding's taps"
          % (B, args.calls, len(sets), flops / 1e9))
    med = {k: spread("    " + k, v) for k, v in us.items()}
    base = med["conv2d_atrous_fwd (bf16)"]
    for k, v in med.items():
        print("    %-54s x%.3f of the bf16 launch, %.0f TFLOP/s" % (k, v / base, flops / v / 1e6))


# ---- (b) the quantising poolings
def poolings(B):
    g = torch.Generator(device="cuda").manual_seed(3)
    for name, H, ks in (("pool4 2x2 / 2", 38, 2), ("pool5 3x3 / 1", 19, 3)):
        C = 512
        Ho = H // 2 if ks == 2 else H
        n_in, n_out = B * H * H * C, B * Ho * Ho * C
        sets = []
        for _ in range(nsets_for(2 * n_in + 3 * n_out)):
            x = torch.randn((B, H, H, C), generator=g, device="cuda").relu().to(BF)
            sets.append(dict(x=x, y=torch.empty((B, Ho, Ho, C), dtype=BF, device="cuda"), q=ops._mx_pair((B, Ho, Ho, C), "cuda"),
                             code=torch.empty((B, Ho, Ho, C // 8), dtype=torch.int32, device="cuda")))

        def S(i):
            return sets[i % len(sets)]
        if ks == 2:
            def two(i):
                ops.quantize_mx_fp8(ops.maxpool2x2_fwd(S(i)["x"], out=S(i)["y"]), q=S(i)["q"][0], scale=S(i)["q"][1])

            def one(i):
                ops.maxpool2x2_fwd_mxfp8(S(i)["x"], q=S(i)["q"][0], scale=S(i)["q"][1])
            two_bytes = 2 * n_in + 2 * n_out + 2 * n_out + n_out + n_out // 32
        else:
            def two(i):
                y, _ = ops.maxpool3x3s1_fwd(S(i)["x"], out=S(i)["y"], code=S(i)["code"])
                ops.quantize_mx_fp8(y, q=S(i)["q"][0], scale=S(i)["q"][1])

            def one(i):
                ops.maxpool3x3s1_fwd_mxfp8(S(i)["x"], q=S(i)["q"][0], scale=S(i)["q"][1])
            two_bytes = 2 * n_in + 2 * n_out + n_out // 2 + 2 * n_out + n_out + n_out // 32
        one_bytes = 2 * n_in + n_out + n_out // 32
        us = alternate({"bf16 pooling + quantize_mx_fp8": two, "quantising pooling": one}, len(sets))
        print("(b) %s at (%d, %d, %d, %d): %d calls per repeat over %d operand sets" % (name, B, H, H, C, args.calls, len(sets)))
        m2 = spread("    bf16 pooling + quantize_mx_fp8 (two launches)", us["bf16 pooling + quantize_mx_fp8"], "   %.1f MB" % (two_bytes / 1e6))
        m1 = spread("    quantising pooling (one launch)", us["quantising pooling"], "   %.1f MB" % (one_bytes / 1e6))
        print("    time ratio x%.3f, byte ratio x%.3f; the one launch moves %.2f TB/s" % (m1 / m2, one_bytes / two_bytes, one_bytes / m1 / 1e6))


# ---- (c) the network
def network(model, B):
    eng = model.get_engine()
    img = (torch.rand((B, 300, 300, 3), generator=torch.Generator().manual_seed(B)) * 2 - 1).cuda()
    x = ops.image_prep(img, normalize=False)
    eng.forward(x, "mxfp8")
    us = alternate({"filter quantisation (every fp8 forward)": lambda i: eng._quantize_filters()}, 1)
    spread("(c) batch %d: filter quantisation, %d elements" % (B, eng._mx_range[1] - eng._mx_range[0]), us["filter quantisation (every fp8 forward)"])
    for what, fns in (("forward", {"bf16": lambda i: eng.forward(x), "mxfp8": lambda i: eng.forward(x, "mxfp8")}),
                      ("detect", {"bf16": lambda i: model.detect(img), "mxfp8": lambda i: model.detect(img, precision="mxfp8")})):
        us = alternate(fns, 1, calls=5)
        m16 = spread("(c) batch %d %s bf16 (5 calls per repeat)" % (B, what), us["bf16"])
        m8 = spread("(c) batch %d %s mxfp8" % (B, what), us["mxfp8"])
        gap = max(us["bf16"]) - min(us["bf16"])
        verdict = "faster than bf16 by more than bf16's own spread" if m16 - m8 > gap else "NOT faster than bf16 by more than bf16's own spread"
        print("    mxfp8 / bf16 x%.3f; bf16 min..max spread %.1f us, difference of medians %.1f us: %s" % (m8 / m16, gap, m16 - m8, verdict),
              flush=True)


def main():
    print("device", torch.cuda.get_device_name(0))
    batches = [int(b) for b in args.batches.split(",")]
    fc6(batches[0])
    poolings(batches[0])
    if args.skip_network:
        return
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(), timestamp_dir=False, network="vgg16_ssd300", l2norm=True,
                                    fp8_inference=True)
    p = model.get_engine().mxfp8_plan()
    print("fp8 layers", sorted(p.fp8), "| pooled", sorted(p.pooled), "| quantising poolings", sorted(p.qpool), "| standalone quantise of node", sorted(p.quant))
    for B in batches:
        network(model, B)


if __name__ == "__main__":
    main()
