"""Dev: the reference loss against the opt-in MultiBox loss, both forms, in one process.

B=64, A=8732, C=81, bf16, matcher targets of the synthetic set, near-uniform logits as a freshly initialised network gives.
Per variant: device events around CALLS calls after warm-up, median of REPEATS repeats, the variants alternating inside every
repeat.  Two ways of issuing the calls: one launch sequence per call from the host ("eager": includes whatever the host cannot
hide), and a captured graph of 10 calls replayed ("graph": the device side alone, which is what a captured training step pays).

usage: python tools_dev/time_multibox_loss.py [--calls 200] [--repeats 5] [--batch 64]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
import ssd_object_detection_amd.ops as ops                          # noqa: E402
from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--batch", type=int, default=64)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
B, PER_GRAPH = args.batch, 10

pset = ops.build_priors()
cls_l, box_l = synth_batch_gt(0, B)
tgt = ops.match_encode(*ops.pack_gt(box_l, cls_l), pset, 0.5)
g = torch.Generator(device="cuda").manual_seed(1)
conf = (0.05 * torch.randn((B, 8732, 81), generator=g, device="cuda")).bfloat16()
loc = (0.05 * torch.randn((B, 8732, 4), generator=g, device="cuda")).bfloat16()
hw, npc = (1444, 361, 100, 25, 9, 1), (4, 6, 6, 6, 4, 4)
hgb = ops.HeadGradBuffers(B, hw, npc, tuple((n * 85 + 7) // 8 * 8 for n in npc))

ws = [ops.MatchWorkspace() for _ in range(4)]       # one per variant: the reference rows form keeps its workspace's state
variants = {
    "reference rows  (ssd_loss_heads)": lambda: ops.ssd_loss_heads(conf, loc, *tgt, hgb, ws=ws[0]),
    "multibox  rows  (multibox_loss_heads)": lambda: ops.multibox_loss_heads(conf, loc, *tgt, hgb, ws=ws[1]),
    "reference dense (ssd_loss)": lambda: ops.ssd_loss(conf, loc, *tgt, ws=ws[2]),
    "multibox  dense (multibox_loss)": lambda: ops.multibox_loss(conf, loc, *tgt, ws=ws[3]),
}
out = ops.multibox_loss_heads(conf, loc, *tgt, hgb).cpu().tolist()
ref = ops.ssd_loss_heads(conf, loc, *tgt, hgb).cpu().tolist()
print("P = %d; mined negatives: reference %d, multibox %d; status %d / %d" % (out[4], ref[5], out[5], ref[7], out[7]))

side = torch.cuda.Stream()
graphs = {}
for name, fn in variants.items():
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(gr, stream=side):
            for _ in range(PER_GRAPH):
                fn()
    gr.replay()
    torch.cuda.synchronize()
    graphs[name] = gr


def timed(issue, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        issue()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


eager = {k: [] for k in variants}
graph = {k: [] for k in variants}
for _ in range(args.repeats):
    for name, fn in variants.items():
        eager[name].append(timed(fn, args.calls) / args.calls)
        graph[name].append(timed(graphs[name].replay, args.calls // PER_GRAPH) / (args.calls // PER_GRAPH * PER_GRAPH))
print("%-40s %12s %12s   (us per call, median of %d x %d calls; min..max)" % ("", "eager", "graph", args.repeats, args.calls))
for name in variants:
    e, gq = eager[name], graph[name]
    print("%-40s %12.1f %12.1f   eager %.1f..%.1f  graph %.1f..%.1f" % (name, statistics.median(e), statistics.median(gq), min(e), max(e), min(gq), max(gq)))
