"""Dev: what the exponential moving average of the weights costs, kernel and train step, alternated in one process.

Kernel: ssd_ema_step (12 bytes per element: reads p and e, writes e) over the default SSD300 engine's flat buffer (n_flat
elements) against ssd_sgd_momentum_step as the yardstick (22 bytes per element: reads p, g, v, writes p, v, bf16; clip-scale and
decay tables).  Both launches walk SETS copies of their operands in turn, so that a call finds none of its operands in the 256 MB
Infinity Cache: between two uses of a set at least (SETS - 1) x 200 MB of other operands pass.  Device events around CALLS calls
after warm-up, the two kernels alternating inside every repeat; median of the REPEATS per-call times, min..max beside it, and the
achieved bytes/s from the traffic above.

Step (--step): the batch-BATCH fused train step (Adam per bucket inside the backward pass) with the average on and off -- one
model that keeps the average; "off" sets no factor, so the optimizer launches are followed by nothing, as on a model without
one -- blocks of STEPS steps alternating.  Median per block; the off step's own min..max over its blocks is the
spread a difference has to exceed.

usage: python tools_dev/time_ema.py [--calls 60] [--repeats 7] [--sets 3] [--step] [--batch 64] [--steps 50]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import _lib, ops, optimizers          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=60)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--step", action="store_true")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=50)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"


def timed(issue, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(n):
        issue(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                                  # ms per call


def report(name, ms, bytes_per_call=None):
    med = statistics.median(ms)
    rate = "  %.2f TB/s" % (bytes_per_call / (med * 1e-3) / 1e12) if bytes_per_call else ""
    print("%-34s median %9.4f ms   min..max %.4f..%.4f   (%d repeats)%s" % (name, med, min(ms), max(ms), len(ms), rate))
    return med


if not args.step:
    from ssd_object_detection_amd.engine import SSDEngine
    eng = SSDEngine(classes=81, seed=3)
    L, n, K = eng.L, eng.n_flat, args.sets
    g = torch.Generator(device="cuda").manual_seed(1)
    eng.grad.copy_(torch.randn(n, generator=g, device="cuda") * 1e-4)
    eng.clip_scales(0.01)
    decay = eng.decay_table(5e-4)
    P, S = ops._ptr, ops._stream
    # SETS copies of every large operand; the tables (a few hundred bytes) are shared
    p = [eng.param.clone() for _ in range(K)]
    e = [eng.param.clone() for _ in range(K)]
    gr = [eng.grad.clone() for _ in range(K)]
    v = [torch.zeros_like(eng.param) for _ in range(K)]
    bf = [torch.empty_like(eng.param_bf16) for _ in range(K)]
    variants = {
        "ssd_ema_step": lambda k: _lib.check(L.ssd_ema_step(P(e[k % K]), P(p[k % K]), n, 2e-4, S())),
        "ssd_sgd_momentum_step": lambda k: _lib.check(L.ssd_sgd_momentum_step(
            P(p[k % K]), P(gr[k % K]), P(v[k % K]), P(bf[k % K]), n, P(eng.block_tensor), P(eng.clip_scale), P(decay), 1.0, 1e-3,
            0.9, 0, S())),
    }
    traffic = {"ssd_ema_step": 12 * n, "ssd_sgd_momentum_step": 22 * n}
    for fn in variants.values():
        for k in range(2 * K):
            fn(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            ms[name].append(timed(fn, args.calls))
    print("%s; n_flat = %d elements; %d calls per repeat over %d operand sets" % (torch.cuda.get_device_name(0), n, args.calls, K))
    med = {name: report(name, ms[name], traffic[name]) for name in variants}
    print("ema / sgd_momentum = %.3f of the time at %.3f of the bytes" % (med["ssd_ema_step"] / med["ssd_sgd_momentum_step"], 12 / 22))
else:
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    B = args.batch
    log_dir = tempfile.TemporaryDirectory(prefix="time_ema_")       # (nothing is logged; removed at exit)
    model = SSDObjectDetectionModel(classes=80, log_dir=log_dir.name, seed=1, timestamp_dir=False)
    cls_l, box_l = synth_batch_gt(0, B)
    image, (cls, loc, mask) = model.make_batch([synth_image(i) for i in range(B)], cls_l, box_l)
    image = ops.image_prep(image.contiguous(), normalize=False)     # the prepared bf16 input: the step alone is timed
    opt, spec = optimizers.Adam(1e-4), ops.EmaSpec(0.9998)
    model.enable_ema(spec)                                          # ONE model: off = no factor set, the launches are not followed
    runs = {"average off": None, "average on (decay 0.9998)": spec}
    ms_main = model.main_stream()
    ctx = torch.cuda.stream(ms_main) if ms_main is not None else torch.cuda.stream(torch.cuda.current_stream())

    def step(name):
        def issue(k):
            model.ema_spec = runs[name]
            model._train_step(image, cls, loc, mask, opt)
        return issue

    with ctx:
        for name in runs:
            for k in range(3):
                step(name)(k)
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(args.repeats):
            for name in runs:
                ms[name].append(timed(step(name), args.steps))
    print("%s; batch %d fused train step, %d steps per block" % (torch.cuda.get_device_name(0), B, args.steps))
    meds = {name: report(name, ms[name]) for name in runs}
    off = ms["average off"]
    print("on - off = %+.4f ms; the off step's own spread over its blocks %.4f ms" % (
        meds["average on (decay 0.9998)"] - meds["average off"], max(off) - min(off)))
    log_dir.cleanup()
