"""Backward and train-step time of the ResNet-50 SSD512 network, bf16 vs fp8 training (forward(x, "mxfp8", train=True), then
backward() with the stride-1 data gradients of mxfp8_bwd_plan in block-scaled fp8).

  python tools_dev/time_resnet_fp8_train.py [--batch 16] [--reps 20] [--no-layers]

Per layer: every fp8 data gradient's ssd_conv2d_bwd_data_mxfp8 launch (with the fp8 output the plan asks of it) against the
bf16 ssd_conv2d_bwd_data of the same layer, each over --reps back-to-back launches.  Also the standalone quantisations of the
gradient maps whose last writer is a bf16 kernel, and the transposed-filter quantisation every fp8 backward starts with.
Whole backward and train step (match + prep + forward + loss + backward + clip + Adam): the two precisions alternate after a
warm-up, each repetition timed by device events; medians.  For kernel totals run it once under
`rocprofv3 --kernel-trace --stats -- python ...` as well (no counters in that run)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                                            # noqa: E402

import ssd_object_detection_amd.ops as ops                                              # noqa: E402
from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt              # noqa: E402
from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine                    # noqa: E402

GRIDS = ((64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1))
RATIOS = ((2,), (2, 3), (2, 3), (2, 3), (2, 3), (2,), (2,))
S_REF = (20, 51, 133, 215, 297, 379, 461, 543)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps                                              # us


def whole_step(eng, B, reps):
    ps = ops.build_priors(grids=GRIDS, s_ref=S_REF, ratios=RATIOS, in_size=512)
    cls_l, box_l = synth_batch_gt(0, B)
    gts = ops.pack_gt(box_l, cls_l)
    tgt = ops.match_encode(*gts, ps, 0.5)
    img = torch.rand((B, 512, 512, 3), generator=torch.Generator().manual_seed(B)).cuda()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

    def step(fp8):
        ops.match_encode(*gts, ps, 0.5, out=tgt)
        x = ops.image_prep(img, normalize=True)
        ploc, pconf = eng.forward(x, "mxfp8", train=True) if fp8 else eng.forward(x)
        _, dconf, dloc = ops.ssd_loss(pconf, ploc, *tgt)
        e[1].record()
        eng.backward(dloc, dconf)
        e[2].record()
        eng.clip_scales(0.01)
        eng.adam(1e-3, eng.grad, 1.0, True)
        e[3].record()

    for _ in range(3):                                                                  # warm-up (allocations, LDS registration)
        step(False)
        step(True)
    torch.cuda.synchronize()
    t = {k: [] for k in ("step bf16", "step mxfp8", "backward bf16", "backward mxfp8")}
    for _ in range(reps):
        for fp8, name in ((False, "bf16"), (True, "mxfp8")):
            e[0].record()
            step(fp8)
            torch.cuda.synchronize()
            t["step " + name].append(e[0].elapsed_time(e[3]) * 1e3)
            t["backward " + name].append(e[1].elapsed_time(e[2]) * 1e3)
    med = {k: statistics.median(v) for k, v in t.items()}
    for what in ("backward", "step"):
        print("batch %3d  %-8s  bf16 %8.0f us   mxfp8 %8.0f us   ratio %.3f   (median of %d, alternated)"
              % (B, what, med[what + " bf16"], med[what + " mxfp8"], med[what + " mxfp8"] / med[what + " bf16"], reps), flush=True)
    return ops.image_prep(img, normalize=True), tgt


def per_layer(eng, x, tgt, B, reps):
    ploc, pconf = eng.forward(x, "mxfp8", train=True)
    _, dconf, dloc = ops.ssd_loss(pconf, ploc, *tgt)
    eng.backward(dloc, dconf)                                                           # fills the fp8 operands
    c = eng._acts(B)
    acts, gacts, g8 = c["acts"], c["gacts"], eng.mxfp8_grads(B)
    print("\nper data gradient, batch %d (us per launch, mean of %d):" % (B, reps))
    print("%4s %-22s %-6s %9s %9s %7s" % ("node", "layer", "fp8out", "bf16", "mxfp8", "ratio"))
    tot = [0.0, 0.0]
    for i in sorted(eng.mx_dgrad):
        nd = eng.nodes[i]
        src = nd["src"]
        relu_src = acts[src + 1] if eng.nodes[src]["relu"] else None
        shape = acts[src + 1].shape
        dy = gacts[eng.mx_groot[i] + 1]
        dyq, dys = g8[eng.mx_groot[i]]
        wtq, wts = eng.mxfp8_wt(i)
        q, sc = g8[src] if eng.mx_gmaps.get(src) == ("fp8", i) else (None, None)
        out = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
        t16 = timed(lambda: ops.conv2d_bwd_data(dy, eng.w_t[i], relu_src, shape, 1, nd["pt"], nd["pl"], out=out, ws=eng._ws), reps)
        t8 = timed(lambda: ops.conv2d_bwd_data_mxfp8(dyq, dys, wtq, wts, relu_src, shape, 1, nd["pt"], nd["pl"], want_fp8=q is not None,
                                                     out=out, out_q=q, out_scale=sc), reps)
        tot[0] += t16
        tot[1] += t8
        name = "%dx%d %d->%d @%d" % (nd["k"], nd["k"], nd["cout"], nd["cin"], nd["hout"])
        print("%4d %-22s %-6s %9.1f %9.1f %7.2f" % (i, name, "yes" if q is not None else "", t16, t8, t8 / t16), flush=True)
    print("%4s %-22s %-6s %9.1f %9.1f %7.2f" % ("", "sum of the %d" % len(eng.mx_dgrad), "", tot[0], tot[1], tot[1] / tot[0]))
    tq = 0.0
    for r, (kind, w) in sorted(eng.mx_gmaps.items()):
        if kind != "fp8":
            t = timed(lambda: ops.quantize_mx_fp8(gacts[r + 1], q=g8[r][0], scale=g8[r][1]), reps)
            tq += t
            print("standalone quantise of map %d (%s, last writer %s %d): %.1f us" % (r, "x".join(map(str, gacts[r + 1].shape)), kind, w, t))
    print("standalone quantisations: %.1f us in all" % tq)
    tw = timed(eng._quantize_wt, reps)
    print("transposed-filter quantisation (one ssd_quantize_mx_fp8 over %d elements, every fp8 backward): %.1f us" % (eng.n_wt8, tw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-layers", action="store_true")
    a = ap.parse_args()
    eng = ResNet50SSDEngine(classes=81, seed=0)
    print("device", torch.cuda.get_device_name(0), "| fp8 data gradients", len(eng.mx_dgrad))
    x, tgt = whole_step(eng, a.batch, a.reps)
    if not a.no_layers:
        per_layer(eng, x, tgt, a.batch, a.reps)


if __name__ == "__main__":
    main()
