"""Forward and detect time of the SSD300 network, bf16 vs block-scaled fp8 (SSDEngine.forward(x, "mxfp8"), detect(precision=)).

  python tools_dev/time_vgg_fp8.py [--batch 64] [--reps 20] [--no-layers]

Whole network: the two precisions alternate in one process after a warm-up, each repetition timed by device events; the median is
reported, for the forward and for SSDObjectDetectionModel.detect (forward + score / decode + NMS).  The fp8 forward starts with
the filter quantisation and contains the plan's one standalone activation quantise: both are timed on their own and the forward
is also reported without them.  Per layer: every fp8 launch (with the outputs the plan asks of it) against the bf16 launch of the
same layer in the bf16 forward, each timed over --reps back-to-back launches; for block3_conv3 + pool also against the unfused
fp8 chain conv2d_fwd_mxfp8 (full-resolution bf16 store) + maxpool2x2_fwd + quantize_mx_fp8.  For kernel-level totals run it
under `rocprofv3 --kernel-trace --stats -- python ...` as well."""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                            # noqa: E402

import ssd_object_detection_amd.ops as ops                                              # noqa: E402
from ssd_object_detection_amd.models import SSDObjectDetectionModel                     # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps                                              # us


def alternated(fns, reps):
    for _ in range(3):                                                                  # warm-up (allocations, LDS registration)
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(timed(fn, 1))
    return {k: statistics.median(v) for k, v in t.items()}


def per_layer(eng, B, reps):
    c = eng._acts(B)
    acts, mx = c["acts"], eng.mxfp8_acts(B)
    fp8, pooled, _, writes = eng.vgg_mxfp8_plan()
    print("\nper layer, batch %d (us per launch, mean of %d):" % (B, reps))
    print("%4s %-24s %-10s %9s %9s %7s" % ("node", "layer", "writes", "bf16", "mxfp8", "ratio"))
    tot = [0.0, 0.0]
    for i in sorted(fp8):
        nd = eng.nodes[i]
        wt, bt = eng.conv_params[i]
        bias = eng.view(bt, eng.param)
        geo = (nd["stride"], nd["pt"], nd["pl"], nd["hout"], nd["hout"], True)
        xb, wb = acts[i], eng.view(wt, eng.param_bf16)
        xq, xs = mx[i - 1]
        wq, ws = eng.mxfp8_weights(i)
        o = i + 1 if i + 1 in pooled else i
        w = writes[o]
        q, sc = mx.get(o, (None, None))
        if o != i:
            same = eng.nodes[o]["hout"] * 2 != eng.nodes[o]["hin"]
            pb, code = torch.empty_like(acts[o + 1]), c["pool_code"][o]
            t16 = timed(lambda: ops.conv2d_fwd_pool(xb, wb, bias, *geo, same, pool_out=pb, code=code, ws=eng._ws, pool_only=True),
                        reps)
            t8 = timed(lambda: ops.conv2d_fwd_pool_mxfp8(xq, xs, wq, ws, bias, *geo, same, want_bf16="bf16" in w,
                                                         want_fp8="fp8" in w, out=pb, out_q=q, out_scale=sc), reps)
            y = torch.empty((B, nd["hout"], nd["hout"], nd["cout"]), dtype=torch.bfloat16, device="cuda")

            def unfused():
                ops.conv2d_fwd_mxfp8(xq, xs, wq, ws, bias, *geo, out=y)
                ops.quantize_mx_fp8(ops.maxpool2x2_fwd(y, same), q=q, scale=sc)
            tu = timed(unfused, reps)
        else:
            y = torch.empty_like(acts[i + 1])
            t16 = timed(lambda: ops.conv2d_fwd(xb, wb, bias, *geo, out=y, ws=eng._ws), reps)
            t8 = timed(lambda: ops.conv2d_fwd_mxfp8(xq, xs, wq, ws, bias, *geo, want_bf16="bf16" in w, want_fp8="fp8" in w, out=y,
                                                    out_q=q, out_scale=sc), reps)
        tot[0] += t16
        tot[1] += t8
        name = "%dx%d/%d %d->%d @%d%s" % (nd["k"], nd["k"], nd["stride"], nd["cin"], nd["cout"], nd["hin"], " +pool" if o != i else "")
        print("%4d %-24s %-10s %9.1f %9.1f %7.2f" % (i, name, "+".join(sorted(w)), t16, t8, t8 / t16), flush=True)
        if o != i:
            print("%4s %-24s %-10s %9s %9.1f %7.2f   (pooled launch / unfused)" % ("", "  unfused fp8 chain", "", "", tu, t8 / tu))
    print("%4s %-24s %-10s %9.1f %9.1f %7.2f" % ("", "sum of the %d launches" % len(fp8), "", tot[0], tot[1], tot[1] / tot[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-layers", action="store_true")
    a = ap.parse_args()
    B = a.batch
    model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(), timestamp_dir=False)
    eng = model.get_engine()
    fp8, _, quant, _ = eng.vgg_mxfp8_plan()
    print("device", torch.cuda.get_device_name(0), "| fp8 layers", sorted(fp8), "| standalone quantise of node", sorted(quant))
    img = (torch.rand((B, 300, 300, 3), generator=torch.Generator().manual_seed(B)) * 2 - 1).cuda()
    x = ops.image_prep(img, normalize=False)
    eng.forward(x, "mxfp8")
    lo, hi = eng._mx_range
    tw = timed(eng._quantize_filters, a.reps)
    mx, acts = eng.mxfp8_acts(B), eng._acts(B)["acts"]
    qn = sorted(quant)[0]
    tq = timed(lambda: ops.quantize_mx_fp8(acts[qn + 1], q=mx[qn][0], scale=mx[qn][1]), a.reps)
    print("filter quantisation (one ssd_quantize_mx_fp8 over %d elements, every fp8 forward): %.1f us" % (hi - lo, tw))
    print("standalone quantise of node %d's map (%s): %.1f us" % (qn, "x".join(map(str, acts[qn + 1].shape)), tq))
    med = alternated({"bf16": lambda: eng.forward(x), "mxfp8": lambda: eng.forward(x, "mxfp8")}, a.reps)
    print("batch %3d  forward  bf16 %8.0f us   mxfp8 %8.0f us   ratio %.3f   (median of %d, alternated)" % (
        B, med["bf16"], med["mxfp8"], med["mxfp8"] / med["bf16"], a.reps))
    rest = med["mxfp8"] - tw - tq
    print("           mxfp8 without the two quantise launches %8.0f us   ratio %.3f" % (rest, rest / med["bf16"]))
    med = alternated({"bf16": lambda: model.detect(img), "mxfp8": lambda: model.detect(img, precision="mxfp8")}, a.reps)
    print("batch %3d  detect   bf16 %8.0f us   mxfp8 %8.0f us   ratio %.3f   (median of %d, alternated)" % (
        B, med["bf16"], med["mxfp8"], med["mxfp8"] / med["bf16"], a.reps), flush=True)
    if not a.no_layers:
        per_layer(eng, B, a.reps)


if __name__ == "__main__":
    main()
