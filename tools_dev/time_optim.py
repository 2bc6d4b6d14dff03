"""Dev: the momentum SGD update against Adam, kernel and train step, alternated in one process.

Kernel: ssd_adam_step (30 bytes per element: reads p, g, m, v, writes p, m, v, bf16) and ssd_sgd_momentum_step (22 bytes per
element: reads p, g, v, writes p, v, bf16) over the SSD300 engine's flat buffer (n_flat elements), with the clip-scale table and,
for SGD, the decay table.  Device events around CALLS calls after warm-up, the two alternating inside every repeat; median of the
REPEATS per-call times, min..max beside it, and the achieved bytes/s from the traffic above.

Step (--step): the batch-BATCH fused train step (the optimizer per bucket inside the backward pass) with momentum SGD
(momentum 0.9, weight decay 5e-4, clip 0.01) against the same step with Adam, one model, blocks of STEPS steps alternating; one
untimed step after every switch (it zeroes the slots).  Median per block; Adam's own min..max over its blocks is the spread a
difference has to exceed.

usage: python tools_dev/time_optim.py [--calls 500] [--repeats 7] [--step] [--batch 64] [--steps 50]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import _lib, ops, optimizers          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=500)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--step", action="store_true")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=50)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"


def timed(issue, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        issue()
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
    L, n = eng.L, eng.n_flat
    g = torch.Generator(device="cuda").manual_seed(1)
    eng.grad.copy_(torch.randn(n, generator=g, device="cuda") * 1e-4)
    eng.clip_scales(0.01)
    decay = eng.decay_table(5e-4)
    P, S = ops._ptr, ops._stream
    variants = {
        "ssd_adam_step": lambda: _lib.check(L.ssd_adam_step(P(eng.param), P(eng.grad), P(eng.adam_m), P(eng.adam_v), P(eng.param_bf16),
                                                           n, P(eng.block_tensor), P(eng.clip_scale), 1.0, 1e-3, 0.9, 0.999, 1e-7, S())),
        "ssd_sgd_momentum_step": lambda: _lib.check(L.ssd_sgd_momentum_step(P(eng.param), P(eng.grad), P(eng.adam_m), P(eng.param_bf16),
                                                                           n, P(eng.block_tensor), P(eng.clip_scale), P(decay), 1.0,
                                                                           1e-3, 0.9, 0, S())),
        "ssd_sgd_momentum_step (nesterov)": lambda: _lib.check(L.ssd_sgd_momentum_step(
            P(eng.param), P(eng.grad), P(eng.adam_m), P(eng.param_bf16), n, P(eng.block_tensor), P(eng.clip_scale), P(decay), 1.0, 1e-3,
            0.9, 1, S())),
    }
    traffic = {"ssd_adam_step": 30 * n, "ssd_sgd_momentum_step": 22 * n, "ssd_sgd_momentum_step (nesterov)": 22 * n}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            ms[name].append(timed(fn, args.calls))
    print("n_flat = %d elements; %d calls per repeat" % (n, args.calls))
    for name in variants:
        report(name, ms[name], traffic[name])
else:
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt, synth_image
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    B = args.batch
    log_dir = tempfile.TemporaryDirectory(prefix="time_optim_")    # (nothing is logged; removed at exit)
    model = SSDObjectDetectionModel(classes=80, log_dir=log_dir.name, seed=1, timestamp_dir=False)
    cls_l, box_l = synth_batch_gt(0, B)
    image, (cls, loc, mask) = model.make_batch([synth_image(i) for i in range(B)], cls_l, box_l)
    image = ops.image_prep(image.contiguous(), normalize=False)     # the prepared bf16 input: the step alone is timed
    opts = {"Adam": optimizers.Adam(1e-4), "SGD momentum 0.9, decay 5e-4": optimizers.SGD(1e-4, momentum=0.9, weight_decay=5e-4)}
    ms_main = model.main_stream()
    ctx = torch.cuda.stream(ms_main) if ms_main is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        for opt in opts.values():
            for _ in range(3):
                model._train_step(image, cls, loc, mask, opt)
        torch.cuda.synchronize()
        ms = {k: [] for k in opts}
        for _ in range(args.repeats):
            for name, opt in opts.items():
                model._train_step(image, cls, loc, mask, opt)       # untimed: the switch zeroes the slots
                ms[name].append(timed(lambda: model._train_step(image, cls, loc, mask, opt), args.steps))
    print("batch %d fused train step, %d steps per block" % (B, args.steps))
    meds = {name: report(name, ms[name]) for name in opts}
    a = ms["Adam"]
    print("SGD - Adam = %+.4f ms; Adam's own spread over its blocks %.4f ms" % (
        meds["SGD momentum 0.9, decay 5e-4"] - meds["Adam"], max(a) - min(a)))
    log_dir.cleanup()
