"""Dev: the box term's kinds (smooth L1, GIoU, DIoU, CIoU) in the MultiBox and softmax focal losses, kernels and train step, in
one process.

kernels: B=64, A=8732, C=81, matcher targets of the synthetic set, logits N(0, 3) clipped to |z| <= 16, predicted offsets
N(0, 1).  The four loss entries (MultiBox / softmax focal, dense bf16 / rows form; --f32 adds the dense f32 calls) for each of
the four kinds on the same inputs.  Per variant: device events around CALLS calls, median of REPEATS repeats with min..max, the
variants alternating inside every repeat.  Every call takes the next of several copies of its operands and outputs, enough of
them that more than the 256 MiB Infinity Cache passes before a copy is used again.

step: the batch-64 fused train step of the default network (match_async + image_prep + _train_step, Adam) with loss multibox,
box="ciou" against box="smooth_l1", alternating on one model.

usage: python tools_dev/time_box_loss.py [--part kernels|step|all] [--f32] [--calls 50] [--repeats 7] [--steps 20] [--batch 64]"""
import argparse
import collections
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
import ssd_object_detection_amd.ops as ops                          # noqa: E402
from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=("kernels", "step", "all"))
ap.add_argument("--f32", action="store_true")
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
B, A, C = args.batch, 8732, 81
CACHE = 256 << 20
BOXES = ops.LossSpec.BOXES


def timed(issue, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        issue()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def report(title, results):
    print(title)
    for name, r in results.items():
        print("  %-44s %10.1f  (%.1f..%.1f)" % (name, statistics.median(r), min(r), max(r)), flush=True)


def kernels():
    pset = ops.build_priors()
    cls_l, box_l = synth_batch_gt(0, B)
    tgt = ops.match_encode(*ops.pack_gt(box_l, cls_l), pset, 0.5)
    print("positives: %d of %d anchors" % (int(tgt[2].sum()), B * A))
    g = torch.Generator(device="cuda").manual_seed(1)
    hw, npc = (1444, 361, 100, 25, 9, 1), (4, 6, 6, 6, 4, 4)
    npad = tuple((n * (4 + C) + 7) // 8 * 8 for n in npc)
    variants = {}
    for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        if dtype == torch.float32 and not args.f32:
            continue
        size = B * A * C * (4 if dtype == torch.float32 else 2)
        copies = CACHE // (2 * size) + 2                                # conf + dconf per call
        confs = [(3.0 * torch.randn((B, A, C), generator=g, device="cuda")).clamp(-16, 16).to(dtype) for _ in range(copies)]
        loc = torch.randn((B, A, 4), generator=g, device="cuda").to(dtype)
        ws = ops.MatchWorkspace()
        state = {"i": 0}

        def nxt(confs=confs, state=state):
            state["i"] = (state["i"] + 1) % len(confs)
            return confs[state["i"]]

        hgbs, hstate = None, {"i": 0}
        if dtype == torch.bfloat16:
            rows_bytes = sum(B * h * p * 2 for h, p in zip(hw, npad))
            hgbs = [ops.HeadGradBuffers(B, hw, npc, npad) for _ in range(CACHE // (size + rows_bytes) + 2)]

        def nxth(hgbs=hgbs, hstate=hstate):
            hstate["i"] = (hstate["i"] + 1) % len(hgbs)
            return hgbs[hstate["i"]]

        # (the outputs are allocated per call; `keep` in the timing loop holds the last few, so their blocks rotate as well)
        for box in BOXES:
            kw = dict(ws=ws, box=box, priors=pset)
            variants["multibox      dense %s %s" % (tag, box)] = lambda nxt=nxt, loc=loc, kw=kw: ops.multibox_loss(nxt(), loc, *tgt, **kw)
            variants["softmax_focal dense %s %s" % (tag, box)] = lambda nxt=nxt, loc=loc, kw=kw: ops.softmax_focal_loss(nxt(), loc, *tgt, **kw)
            if hgbs is not None:
                variants["multibox      rows  %s %s" % (tag, box)] = \
                    lambda nxt=nxt, loc=loc, kw=kw, nxth=nxth: ops.multibox_loss_heads(nxt(), loc, *tgt, nxth(), **kw)
                variants["softmax_focal rows  %s %s" % (tag, box)] = \
                    lambda nxt=nxt, loc=loc, kw=kw, nxth=nxth: ops.softmax_focal_loss_heads(nxt(), loc, *tgt, nxth(), **kw)
    keep = collections.deque(maxlen=3)
    for fn in variants.values():
        for _ in range(4):
            keep.append(fn())
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            res[name].append(timed(lambda fn=fn: keep.append(fn()), args.calls))
    report("loss entries at (%d, %d, %d) by box kind: us per call, median of %d x %d calls (min..max)" % (
        B, A, C, args.repeats, args.calls), dict(sorted(res.items())))


def step():
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    gen = torch.Generator(device="cuda").manual_seed(1234)
    img = torch.rand((B, 300, 300, 3), generator=gen, device="cuda")
    gt = ops.pack_gt(*reversed(synth_batch_gt(0, B)))
    xbuf = torch.empty((B, 300, 300, 8), dtype=torch.bfloat16, device="cuda")
    # ONE model for both kinds, its TrainConfig swapped between the repeats: a second model in the process has streams of its
    # own and measured 1.0-1.4 ms per step slower than the first whatever its loss, which would be
    # charged to whichever kind came second
    model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(prefix="time_box_loss_"), seed=0, timestamp_dir=False)
    opt = optimizers.Adam(1e-3)
    state = {"out": None}
    runs = {}
    for box in ("smooth_l1", "ciou"):
        cfg = SSDObjectDetectionModel.TrainConfig(1, B, opt, warmup=False, loss=ops.LossSpec("multibox", box=box))

        def one(cfg=cfg):
            state["out"] = model.match_async(gt, out=state["out"])
            x = ops.image_prep(img, normalize=True, out=xbuf)
            model._train_step(x, *state["out"], opt, cfg=cfg)

        runs["multibox box=%s" % box] = one
    for one in runs.values():
        for _ in range(3):
            one()
    torch.cuda.synchronize()
    res = {k: [] for k in runs}
    for _ in range(args.repeats):
        for name, one in runs.items():
            res[name].append(timed(one, args.steps) / 1e3)
            assert float(model._last_raw[7]) == 0.0, (name, model._last_raw.tolist())
    report("batch-%d fused train step, default network, one model: ms per step, median of %d x %d steps (min..max)" % (
        B, args.repeats, args.steps), res)


if args.part in ("kernels", "all"):
    kernels()
if args.part in ("step", "all"):
    step()
