"""Dev: the L2 normalisation kernels and what the layer costs the train step, in one process.

Kernel: ssd_l2norm_fwd (per pixel: reads x, writes y and 1 / norm: 2 C bf16 + 4 bytes = 2 KB + 4 B at C = 512) and
ssd_l2norm_bwd (reads dy, x and 1 / norm, writes dx: 3 C bf16 + 4 bytes = 3 KB + 4 B; the workgroups' fp32 partial sums of the
scale's gradient and their reduction are counted too) at the batch-BATCH shape of SSD300's first feature map (P = BATCH * 1444,
C = 512).  One call's operands (95 MB per map at batch 64) would stay in the 256 MiB Infinity Cache from call to call, which
the layer never sees inside a step: the calls rotate through SETS operand sets, > 256 MiB together.  Device events around CALLS
calls after warm-up, forward and backward alternating inside every repeat; median of the REPEATS per-call times, min..max
beside it, and the achieved bytes/s from the traffic above.

Step (--step): the batch-BATCH fused train step (default Adam) of a model with the layer against one without, blocks of STEPS
steps alternating in one process.  Median per block; the plain model's own min..max over its blocks is the spread a difference
has to exceed.

usage: python tools_dev/time_l2norm.py [--calls 200] [--repeats 7] [--sets 4] [--step] [--batch 64] [--steps 30]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import _lib, ops, optimizers          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--step", action="store_true")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=30)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"


def timed(issue, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        issue(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                                  # ms per call


def report(name, ms, bytes_per_call=None):
    med = statistics.median(ms)
    rate = "  %.2f TB/s" % (bytes_per_call / (med * 1e-3) / 1e12) if bytes_per_call else ""
    print("%-34s median %9.4f ms   min..max %.4f..%.4f   (%d repeats)%s" % (name, med, min(ms), max(ms), len(ms), rate))
    return med


if not args.step:
    L = _lib.lib()
    P, C = args.batch * 1444, 512
    g = torch.Generator(device="cuda").manual_seed(1)
    scale = 20.0 + 5.0 * torch.randn(C, generator=g, device="cuda")
    sets = []
    for _ in range(args.sets):
        x = (torch.randn((P, C), generator=g, device="cuda").relu() * 3.0).bfloat16()
        dy = (torch.randn((P, C), generator=g, device="cuda") * 1e-3).bfloat16()
        sets.append(dict(x=x, dy=dy, y=torch.empty_like(x), dx=torch.empty_like(x),
                         r=torch.empty((P,), dtype=torch.float32, device="cuda")))
    ds = torch.empty((C,), dtype=torch.float32, device="cuda")
    wsb = L.ssd_l2norm_ws_bytes(P, C)
    ws = torch.empty((wsb,), dtype=torch.uint8, device="cuda")
    Pt, S = ops._ptr, ops._stream

    def fwd(i):
        s = sets[i % len(sets)]
        _lib.check(L.ssd_l2norm_fwd(Pt(s["x"]), Pt(scale), Pt(s["y"]), Pt(s["r"]), P, C, 1e-10, S()))

    def bwd(i):
        s = sets[i % len(sets)]
        _lib.check(L.ssd_l2norm_bwd(Pt(s["dy"]), Pt(s["x"]), Pt(scale), Pt(s["r"]), Pt(s["dx"]), 0, Pt(ds), Pt(ws), wsb, P, C,
                                    1e-10, S()))

    variants = {"ssd_l2norm_fwd": fwd, "ssd_l2norm_bwd": bwd}
    traffic = {"ssd_l2norm_fwd": P * (2 * C * 2 + 4), "ssd_l2norm_bwd": P * (3 * C * 2 + 4) + 2 * wsb + 4 * C}
    for fn in variants.values():
        for i in range(2 * len(sets)):
            fn(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            ms[name].append(timed(fn, args.calls))
    print("P = %d pixels x C = %d; %d calls per repeat over %d operand sets (%.0f MB each)" % (
        P, C, args.calls, len(sets), 4 * P * C * 2 / 1e6))
    for name in variants:
        print("%s: %.0f bytes per pixel" % (name, traffic[name] / P))
        report(name, ms[name], traffic[name])
else:
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    B = args.batch
    log_dir = tempfile.TemporaryDirectory(prefix="time_l2norm_")   # (nothing is logged; removed at exit)
    models = {"plain": SSDObjectDetectionModel(classes=80, log_dir=log_dir.name, seed=1, timestamp_dir=False),
              "l2norm": SSDObjectDetectionModel(classes=80, log_dir=log_dir.name, seed=1, timestamp_dir=False, l2norm=True)}
    cls_l, box_l = synth_batch_gt(0, B)
    image, (cls, loc, mask) = models["plain"].make_batch([synth_image(i) for i in range(B)], cls_l, box_l)
    image = ops.image_prep(image.contiguous(), normalize=False)     # the prepared bf16 input: the step alone is timed
    opts = {name: optimizers.Adam(1e-4) for name in models}
    ms = {k: [] for k in models}
    for name, model in models.items():
        with torch.cuda.stream(model.main_stream() or torch.cuda.current_stream()):
            for _ in range(3):
                model._train_step(image, cls, loc, mask, opts[name])
            torch.cuda.synchronize()
    for _ in range(args.repeats):
        for name, model in models.items():
            with torch.cuda.stream(model.main_stream() or torch.cuda.current_stream()):
                ms[name].append(timed(lambda i: model._train_step(image, cls, loc, mask, opts[name]), args.steps))
    print("batch %d fused train step, %d steps per block" % (B, args.steps))
    meds = {name: report(name, ms[name]) for name in models}
    a = ms["plain"]
    print("l2norm - plain = %+.4f ms; the plain step's own spread over its blocks %.4f ms" % (
        meds["l2norm"] - meds["plain"], max(a) - min(a)))
    log_dir.cleanup()
