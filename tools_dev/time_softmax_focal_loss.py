"""Dev: the opt-in softmax focal loss against the MultiBox loss, kernels and train step, in one process.

kernels: B=64, A=8732, C=81, matcher targets of the synthetic set, logits N(0, 3) clipped to |z| <= 16.  Dense f32, dense bf16
and the rows form of both losses on the same inputs.  Per variant: device events around CALLS calls, median of REPEATS repeats
with min..max, the variants alternating inside every repeat.  Every call takes the next of several copies of its operands and
outputs, enough of them that more than the 256 MiB Infinity Cache passes before a copy is used again.  Bytes moved are counted
from the shapes (what the algorithm needs: conf read once and dconf written once for the focal loss; MultiBox reads conf once,
re-reads the selected rows and writes dconf once -- its own count is printed as the focal loss's, for comparison only).

step: the batch-64 fused train step of the default network (match_async + image_prep + _train_step, Adam) with loss
softmax_focal against multibox, each with the engine's sparse-row head path (at full density for the focal loss) and with
sparse_heads=False (the dense head kernels).

usage: python tools_dev/time_softmax_focal_loss.py [--part kernels|step|all] [--calls 50] [--repeats 7] [--steps 20] [--batch 64]"""
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
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
B, A, C = args.batch, 8732, 81
CACHE = 256 << 20


def timed(issue, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        issue()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def report(title, results, extra=lambda name, med: ""):
    print(title)
    for name, r in results.items():
        med = statistics.median(r)
        print("  %-44s %10.1f  (%.1f..%.1f)%s" % (name, med, min(r), max(r), extra(name, med)), flush=True)


def kernels():
    pset = ops.build_priors()
    cls_l, box_l = synth_batch_gt(0, B)
    tgt = ops.match_encode(*ops.pack_gt(box_l, cls_l), pset, 0.5)
    g = torch.Generator(device="cuda").manual_seed(1)
    hw, npc = (1444, 361, 100, 25, 9, 1), (4, 6, 6, 6, 4, 4)
    npad = tuple((n * (4 + C) + 7) // 8 * 8 for n in npc)
    variants, traffic = {}, {}
    for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        size = B * A * C * (4 if dtype == torch.float32 else 2)
        copies = CACHE // (2 * size) + 2                                # conf + dconf per call
        confs = [(3.0 * torch.randn((B, A, C), generator=g, device="cuda")).clamp(-16, 16).to(dtype) for _ in range(copies)]
        loc = (0.05 * torch.randn((B, A, 4), generator=g, device="cuda")).to(dtype)
        ws = ops.MatchWorkspace()
        state = {"i": 0}

        def nxt(confs=confs, state=state):
            state["i"] = (state["i"] + 1) % len(confs)
            return confs[state["i"]]

        # (the outputs are allocated per call; `keep` in the timing loop holds the last few, so their blocks rotate as well)
        variants["softmax_focal dense %s" % tag] = lambda nxt=nxt, loc=loc, ws=ws: ops.softmax_focal_loss(nxt(), loc, *tgt, ws=ws)
        variants["multibox      dense %s" % tag] = lambda nxt=nxt, loc=loc, ws=ws: ops.multibox_loss(nxt(), loc, *tgt, ws=ws)
        traffic["softmax_focal dense %s" % tag] = traffic["multibox      dense %s" % tag] = 2 * size
        if dtype == torch.bfloat16:
            rows_bytes = sum(B * h * p * 2 for h, p in zip(hw, npad))
            hgbs = [ops.HeadGradBuffers(B, hw, npc, npad) for _ in range(CACHE // (size + rows_bytes) + 2)]
            hstate = {"i": 0}

            def nxth(hgbs=hgbs, hstate=hstate):
                hstate["i"] = (hstate["i"] + 1) % len(hgbs)
                return hgbs[hstate["i"]]

            variants["softmax_focal rows  bf16"] = lambda nxt=nxt, loc=loc, ws=ws, nxth=nxth: ops.softmax_focal_loss_heads(nxt(), loc, *tgt, nxth(), ws=ws)
            variants["multibox      rows  bf16"] = lambda nxt=nxt, loc=loc, ws=ws, nxth=nxth: ops.multibox_loss_heads(nxt(), loc, *tgt, nxth(), ws=ws)
            traffic["softmax_focal rows  bf16"] = traffic["multibox      rows  bf16"] = size + rows_bytes
    keep = collections.deque(maxlen=3)                                  # 3 x (dconf f32 181 MB | bf16 91 MB) stay allocated
    for fn in variants.values():
        for _ in range(4):
            keep.append(fn())
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            res[name].append(timed(lambda fn=fn: keep.append(fn()), args.calls))
    report("loss kernels at (%d, %d, %d): us per call, median of %d x %d calls (min..max); bytes from the shapes" % (
        B, A, C, args.repeats, args.calls), res,
        lambda name, med: "   %6.1f MB  %5.2f TB/s" % (traffic[name] / 1e6, traffic[name] / med / 1e6))


def step():
    from ssd_object_detection_amd import optimizers
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    gen = torch.Generator(device="cuda").manual_seed(1234)
    img = torch.rand((B, 300, 300, 3), generator=gen, device="cuda")
    gt = ops.pack_gt(*reversed(synth_batch_gt(0, B)))
    xbuf = torch.empty((B, 300, 300, 8), dtype=torch.bfloat16, device="cuda")
    runs = {}
    for heads in ("sparse rows", "dense heads"):
        os.environ["SSD_SPARSE_HEADS"] = "1" if heads == "sparse rows" else "0"      # read by the engine's constructor
        for loss in ("multibox", "softmax_focal"):
            model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(prefix="time_softmax_focal_"), seed=0, timestamp_dir=False)
            assert model.get_engine().sparse_heads == (heads == "sparse rows")
            if loss == "softmax_focal":
                model.set_background_prior(0.01)
            opt = optimizers.Adam(1e-3)
            cfg = SSDObjectDetectionModel.TrainConfig(1, B, opt, warmup=False, loss=loss)
            state = {"out": None}

            def one(model=model, opt=opt, cfg=cfg, state=state):
                state["out"] = model.match_async(gt, out=state["out"])
                x = ops.image_prep(img, normalize=True, out=xbuf)
                model._train_step(x, *state["out"], opt, cfg=cfg)

            runs["%-13s %s" % (loss, heads)] = (one, model)
    os.environ.pop("SSD_SPARSE_HEADS")
    for one, _ in runs.values():
        for _ in range(3):
            one()
    torch.cuda.synchronize()
    res = {k: [] for k in runs}
    for _ in range(args.repeats):
        for name, (one, _) in runs.items():
            res[name].append(timed(one, args.steps) / 1e3)
    for name, (_, model) in runs.items():
        assert float(model._last_raw[7]) == 0.0, (name, model._last_raw.tolist())
    report("batch-%d fused train step, default network: ms per step, median of %d x %d steps (min..max)" % (
        B, args.repeats, args.steps), res)


if args.part in ("kernels", "all"):
    kernels()
if args.part in ("step", "all"):
    step()
