"""Forward time of the ResNet-50 SSD512 network, bf16 vs block-scaled fp8 (ResNet50SSDEngine.forward(x, "mxfp8")).

  python tools_dev/time_resnet_fp8.py [--batches 16,64] [--reps 20] [--no-layers]

Whole network: the two precisions alternate in one process after a warm-up, each repetition timed by device events; the median is
reported.  Per layer (batch 16): every fp8 layer's ssd_conv2d_fwd_mxfp8 launch (with the outputs the plan asks of it) against
the bf16 ssd_conv2d_fwd of the same layer, each timed over --reps back-to-back launches.  Also the filter quantisation that every
fp8 forward starts with.  For kernel-level totals run it under `rocprofv3 --kernel-trace --stats -- python ...` as well."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                            # noqa: E402

import ssd_object_detection_amd.ops as ops                                              # noqa: E402
from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine                    # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps                                              # us


def whole_network(eng, B, reps):
    x = ops.image_prep(torch.rand((B, 512, 512, 3), generator=torch.Generator().manual_seed(B)).cuda())
    for _ in range(3):                                                                  # warm-up (allocations, LDS registration)
        eng.forward(x)
        eng.forward(x, "mxfp8")
    torch.cuda.synchronize()
    t = {"bf16": [], "mxfp8": []}
    for _ in range(reps):
        for prec in ("bf16", "mxfp8"):
            t[prec].append(timed(lambda: eng.forward(x, prec), 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    print("batch %3d  forward  bf16 %8.0f us   mxfp8 %8.0f us   ratio %.3f   (median of %d, alternated)" % (
        B, med["bf16"], med["mxfp8"], med["mxfp8"] / med["bf16"], reps), flush=True)
    return x


def per_layer(eng, B, reps):
    c = eng._acts(B)
    acts, mx = c["acts"], eng.mxfp8_acts(B)
    print("\nper layer, batch %d (us per launch, mean of %d):" % (B, reps))
    print("%4s %-22s %-10s %9s %9s %7s" % ("node", "layer", "writes", "bf16", "mxfp8", "ratio"))
    tot = [0.0, 0.0]
    for i in sorted(eng.mx_fp8):
        nd, w = eng.nodes[i], eng.mx_writes[i]
        wt, bt = eng.conv_params[i]
        bias = eng.view(bt, eng.param)
        geo = (nd["stride"], nd["pt"], nd["pl"], nd["hout"], nd["hout"], nd["relu"])
        xb, wb = eng._in(acts, nd["src"]), eng.view(wt, eng.param_bf16)
        y = torch.empty_like(acts[i + 1])
        xq, xs = mx[nd["src"]]
        wq, ws = eng.mxfp8_weights(i)
        q, sc = mx.get(i, (None, None))
        t16 = timed(lambda: ops.conv2d_fwd(xb, wb, bias, *geo, out=y, ws=eng._ws), reps)
        t8 = timed(lambda: ops.conv2d_fwd_mxfp8(xq, xs, wq, ws, bias, *geo, want_bf16="bf16" in w, want_fp8="fp8" in w, out=y,
                                                out_q=q, out_scale=sc), reps)
        tot[0] += t16
        tot[1] += t8
        name = "%dx%d/%d %d->%d @%d" % (nd["k"], nd["k"], nd["stride"], nd["cin"], nd["cout"], nd["hin"])
        print("%4d %-22s %-10s %9.1f %9.1f %7.2f" % (i, name, "+".join(sorted(w)), t16, t8, t8 / t16), flush=True)
    print("%4s %-22s %-10s %9.1f %9.1f %7.2f" % ("", "sum of the 44 layers", "", tot[0], tot[1], tot[1] / tot[0]))
    adds = [i for i in range(len(eng.nodes)) if "fp8" in eng.mx_writes[i] and eng.nodes[i]["kind"] == "add"]
    ta = tq = 0.0
    for i in adds:
        a, s = eng.nodes[i]["src"]
        out = torch.empty_like(acts[i + 1])
        ta += timed(lambda: ops.add_relu_fwd(acts[a + 1], acts[s + 1], out=out), reps)
        tq += timed(lambda: ops.add_relu_fwd_mxfp8(acts[a + 1], acts[s + 1], out=out, q=mx[i][0], scale=mx[i][1]), reps)
    print("%d adds feeding fp8 layers: add_relu_fwd %.1f us, add_relu_fwd_mxfp8 %.1f us" % (len(adds), ta, tq))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-layers", action="store_true")
    a = ap.parse_args()
    eng = ResNet50SSDEngine(classes=81, seed=0)
    print("device", torch.cuda.get_device_name(0), "| fp8 layers", len(eng.mx_fp8))
    eng._quantize_filters()
    tw = timed(eng._quantize_filters, a.reps)
    print("filter quantisation (one ssd_quantize_mx_fp8 over %d trunk elements, every fp8 forward): %.1f us" % (eng._mx_range[1], tw))
    batches = [int(v) for v in a.batches.split(",")]
    for B in batches:
        whole_network(eng, B, a.reps)
        if not a.no_layers and B == batches[0]:
            per_layer(eng, B, a.reps)


if __name__ == "__main__":
    main()
