"""Dev: the VGG-16 SSD300 network's two new costs, in one process.

1. ssd_maxpool2x2_bwd_argmax_accumulate against ssd_maxpool2x2_bwd_argmax at pool4's training shape (BATCH, 38, 38, 512): the
   calls alternate inside every repeat and rotate through operand sets of more than 256 MiB together (a layer never finds its
   operands in the Infinity Cache inside a step).  Bytes a call must move: the overwrite form writes dx (2 B per element) and
   reads, per POOLED element, dy (2 B) and its code nibble (1/2 B); the accumulating form also reads dx (2 B more per dx
   element).  The time ratio is printed beside that byte ratio.
2. The fused train step (model._train_step: Adam per bucket inside backward(), reference loss, targets assigned up front) of
   SSDObjectDetectionModel(network="vgg16_ssd300", l2norm=True) and of the default network, at each --batches size: blocks of
   STEPS steps alternating between the two models in one process; median per block, min..max beside it, images / s.  The ten
   new nodes' share (conv4_1 .. fc7): device events on the step's main stream around the forward walk of nodes 10 .. 19 and
   around the backward walk of nodes 19 .. 10 (their weight gradients run beside it on the side stream and are not in the
   span), as a fraction of the step.

usage: python tools_dev/time_vgg16_step.py [--batches 64,32] [--steps 5] [--repeats 7] [--calls 20] [--skip-step]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import engine as E, ops, optimizers   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,32")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
BF, CACHE = torch.bfloat16, 256 << 20


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def spread(name, ms, tail=""):
    med = statistics.median(ms)
    print("%-40s median %9.4f ms   min..max %.4f..%.4f   (%d repeats)%s" % (name, med, min(ms), max(ms), len(ms), tail))
    return med


# ---- 1. the kernel
def kernel(B):
    H = W = 38
    C, Ho = 512, 19
    g = torch.Generator(device="cuda").manual_seed(1)
    n_dx, n_dy = B * H * W * C, B * Ho * Ho * C
    per_set = 2 * n_dx + 2 * n_dy + n_dy // 2
    sets = []
    for _ in range(max(2, -(-(CACHE + (32 << 20)) // per_set))):
        x = torch.randn((B, H, W, C), generator=g, device="cuda").relu().to(BF)
        _, code = ops.maxpool2x2_fwd_argmax(x)
        dy = (torch.randn((B, Ho, Ho, C), generator=g, device="cuda") * 1e-2).to(BF)
        sets.append(dict(code=code, dy=dy, dx=(torch.randn((B, H, W, C), generator=g, device="cuda") * 1e-2).to(BF)))
        del x

    def S(i):
        return sets[i % len(sets)]

    variants = {
        "maxpool2x2_bwd_argmax (overwrite)": lambda i: ops.maxpool2x2_bwd_argmax(S(i)["code"], S(i)["dy"], (B, H, W, C), out=S(i)["dx"]),
        "maxpool2x2_bwd_argmax (accumulate)": lambda i: ops.maxpool2x2_bwd_argmax(S(i)["code"], S(i)["dy"], (B, H, W, C), out=S(i)["dx"],
                                                                                  accumulate=True),
    }
    nbytes = {"maxpool2x2_bwd_argmax (overwrite)": 2 * n_dx + 2 * n_dy + n_dy // 2,
              "maxpool2x2_bwd_argmax (accumulate)": 4 * n_dx + 2 * n_dy + n_dy // 2}

    def timed(fn):
        e0, e1 = events()
        e0.record()
        for i in range(args.calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls

    for fn in variants.values():
        for i in range(2 * len(sets)):
            fn(i)
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            ms[name].append(timed(fn))
    print("pool4 backward at (%d, %d, %d, %d): %d calls per repeat over %d operand sets (%.0f MB each)" % (
        B, H, W, C, args.calls, len(sets), per_set / 1e6))
    med = {k: spread(k, v, "  %.2f TB/s of %.1f MB" % (nbytes[k] / (statistics.median(v) * 1e-3) / 1e12, nbytes[k] / 1e6))
           for k, v in ms.items()}
    a, o = "maxpool2x2_bwd_argmax (accumulate)", "maxpool2x2_bwd_argmax (overwrite)"
    print("accumulate / overwrite: time %.2f, bytes %.2f" % (med[a] / med[o], nbytes[a] / nbytes[o]))


# ---- 2. the step
class Spans:
    """Device events on the current stream around trunk nodes lo .. hi of one engine's forward and backward walks."""

    def __init__(self, eng, lo, hi):
        self.eng, self.lo, self.hi, self.on = eng, lo, hi, False
        self.fwd, self.bwd = [], []
        real_fwd = eng._bf16_node

        def fwd(i, c):
            if self.on and i == lo:
                self.fwd.append(list(events()))
                self.fwd[-1][0].record()
            real_fwd(i, c)
            if self.on and i == hi:
                self.fwd[-1][1].record()
        eng._bf16_node = fwd
        spans, real_bwd = self, E._BackwardPass.node

        def bwd(p, i):
            mine = spans.on and p.eng is eng
            if mine and i == hi:
                spans.bwd.append(list(events()))
                spans.bwd[-1][0].record()
            real_bwd(p, i)
            if mine and i == lo:
                spans.bwd[-1][1].record()
        E._BackwardPass.node = bwd

    def totals(self):
        f = sum(a.elapsed_time(b) for a, b in self.fwd) / max(1, len(self.fwd))
        b = sum(a.elapsed_time(b) for a, b in self.bwd) / max(1, len(self.bwd))
        return f, b


def step_loops(B):
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    cls_l, box_l = synth_batch_gt(5000, B)
    gt = ops.pack_gt(box_l, cls_l)
    img = ops.image_prep(torch.rand((B, 300, 300, 3), device="cuda"), normalize=True)
    log_dir = tempfile.mkdtemp()
    loops, spans = {}, None
    for name, kw in (("vgg16_ssd300 + l2norm", dict(network="vgg16_ssd300", l2norm=True)), ("ssd300 (default)", {})):
        model = SSDObjectDetectionModel(80, log_dir, seed=0, timestamp_dir=False, **kw)
        opt = optimizers.Adam(1e-4)
        tgt = model.match_async(gt)
        if kw:
            spans = Spans(model.get_engine(), 10, 19)
        loops[name] = (lambda i, model=model, opt=opt, tgt=tgt: model._train_step(img, *tgt, opt), model.main_stream())

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
    print("vgg16_ssd300 / ssd300: %.2f" % (med["vgg16_ssd300 + l2norm"] / med["ssd300 (default)"]))
    spans.on = True                                                 # (events inside the step: a run of their own)
    t = timed(loops["vgg16_ssd300 + l2norm"], args.steps)
    spans.on = False
    f, b = spans.totals()
    print("nodes 10 .. 19 on the main stream: forward %.3f ms + backward %.3f ms = %.3f ms of a %.3f ms step (%.0f %%)" % (
        f, b, f + b, t, 100.0 * (f + b) / t))
    del loops


kernel(64)
if not args.skip_step:
    for B in [int(v) for v in args.batches.split(",")]:
        step_loops(B)
        torch.cuda.empty_cache()
