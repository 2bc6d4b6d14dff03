"""Dev: the fused train step of the MobileNet-v1 SSD300 network, next to tools_dev/time_vgg16_step.py.

The step (model._train_step: Adam per bucket inside backward(), reference loss, targets assigned up front) of
SSDObjectDetectionModel(network="mobilenet_v1_ssd300") and of the default network at each --batches size: blocks of STEPS steps
alternating between the two models in one process; median per block, min..max beside it, images / s.
The depthwise passes' share: in a run of its own, device events around every ops.dwconv3x3_* call of the step, on the stream the
call runs on (forward and data gradient: the step's main stream; weight gradient: the side stream, beside the main stream's
work), summed per pass and set against the step's time.  A launch between two events is not overlapped by the next launch
of its stream, so the sums are an upper estimate of what the passes cost inside the undisturbed step.

usage: python tools_dev/time_mobilenet_step.py [--batches 64] [--steps 5] [--repeats 7]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import ops, optimizers                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
NET = "mobilenet_v1_ssd300"


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def spread(name, ms, tail=""):
    med = statistics.median(ms)
    print("%-40s median %9.4f ms   min..max %.4f..%.4f   (%d repeats)%s" % (name, med, min(ms), max(ms), len(ms), tail), flush=True)
    return med


class DepthwiseSpans:
    """Device events around every ops.dwconv3x3_* call while `on`."""
    PASSES = {"dwconv3x3_fwd": "forward", "dwconv3x3_fwd_relubits": "forward", "dwconv3x3_bwd_data": "data gradient",
              "dwconv3x3_bwd_data_bits": "data gradient", "dwconv3x3_bwd_weight": "weight gradient"}

    def __init__(self):
        self.on, self.spans = False, []
        for name, what in self.PASSES.items():
            setattr(ops, name, self._wrap(getattr(ops, name), what))

    def _wrap(self, fn, what):
        def call(*a, **kw):
            if not self.on:
                return fn(*a, **kw)
            e0, e1 = events()
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            self.spans.append((what, e0, e1))
            return out
        return call

    def totals(self, steps):
        out = {}
        for what, e0, e1 in self.spans:
            out[what] = out.get(what, 0.0) + e0.elapsed_time(e1) / steps
        return out


def step_loops(B, spans):
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    cls_l, box_l = synth_batch_gt(5000, B)
    gt = ops.pack_gt(box_l, cls_l)
    img = ops.image_prep(torch.rand((B, 300, 300, 3), device="cuda"), normalize=True)
    log_dir = tempfile.mkdtemp()
    loops = {}
    for name, kw in ((NET, dict(network=NET)), ("ssd300 (default)", {})):
        model = SSDObjectDetectionModel(80, log_dir, seed=0, timestamp_dir=False, **kw)
        opt = optimizers.Adam(1e-4)
        tgt = model.match_async(gt)
        loops[name] = (lambda i, model=model, opt=opt, tgt=tgt: model._train_step(img, *tgt, opt), model.main_stream())
        if kw:
            eng = model.get_engine()

    def timed(loop, n):
        issue, stream = loop
        e0, e1 = events()
        with torch.cuda.stream(stream):
            e0.record()
            for i in range(n):
                issue(i)
            e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for loop in loops.values():
        timed(loop, 3)
    ms = {k: [] for k in loops}
    for _ in range(args.repeats):
        for name, loop in loops.items():
            ms[name].append(timed(loop, args.steps))
    print("fused train step at batch %d: %d steps per block, %d blocks, the two models alternating" % (B, args.steps, args.repeats))
    med = {k: spread(k, v, "  %.0f images/s" % (B / (statistics.median(v) * 1e-3))) for k, v in ms.items()}
    print("%s / ssd300: %.2f; chain %s, dw data gradients from %s" % (NET, med[NET] / med["ssd300 (default)"], sorted(eng.chain),
                                                                      "sign bytes" if eng.dw_dgrad_bits else "relu_src"))
    spans.on, spans.spans = True, []                                # (events inside the step: a run of their own)
    t = timed(loops[NET], args.steps)
    spans.on = False
    tot = spans.totals(args.steps)
    print("depthwise passes of a %.3f ms step (with events): %s; main stream (forward + data gradient) %.3f ms = %.0f %%, with the "
          "side stream's weight gradients %.3f ms = %.0f %%" % (
              t, ", ".join("%s %.3f ms" % kv for kv in sorted(tot.items())), tot["forward"] + tot["data gradient"],
              100.0 * (tot["forward"] + tot["data gradient"]) / t, sum(tot.values()), 100.0 * sum(tot.values()) / t), flush=True)
    del loops


spans = DepthwiseSpans()
for B in [int(v) for v in args.batches.split(",")]:
    step_loops(B, spans)
    torch.cuda.empty_cache()
