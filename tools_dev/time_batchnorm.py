"""Dev: the batch normalisation kernels and what live batch normalisation costs the ResNet-50 SSD512 train step, in one process.

Kernels: ssd_bn_fwd_train, ssd_bn_fwd_infer and ssd_bn_bwd at the maps of the engine at batch 16 (P rows x C channels):
(1 048 576, 64) behind the stem, (262 144, 256) in conv2_x, (16 384, 1024) in conv4_x.  Bytes a call must move, per element of
the map (bf16 = 2 bytes): training forward 6 (x is read twice -- statistics, then normalisation -- and y written), inference 4
(x read, y written), backward 10 (dy and x are read twice -- sums, then dx -- and dx written); the slab partials (written and
read once: 2 x ssd_bn_ws_bytes) are counted on top, the per-channel vectors are not.  One call's operands would stay in the
256 MiB Infinity Cache from call to call, which a layer never sees inside a step: the calls rotate through operand sets of
more than 256 MiB together.  Device events around CALLS calls after warm-up, the three passes alternating inside every
repeat; median of the REPEATS per-call times, min..max beside it, and the achieved bytes/s from the traffic above.

Step (--step): the batch-BATCH train step (forward(train=True), ssd_loss_heads, backward, clip, Adam) of a batchnorm engine
against the default engine's, blocks of STEPS steps alternating in one process.  Median per block; each engine's own min..max
over its blocks is the spread a difference has to exceed.

usage: python tools_dev/time_batchnorm.py [--calls 50] [--repeats 7] [--step] [--batch 16] [--steps 5]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import _lib, ops                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--step", action="store_true")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--steps", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

SHAPES = ((1048576, 64), (262144, 256), (16384, 1024))
CACHE = 256 << 20


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
    Pt, S = ops._ptr, ops._stream
    for P, C in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        gamma = 1.0 + 0.1 * torch.randn(C, generator=g, device="cuda")
        beta = 0.1 * torch.randn(C, generator=g, device="cuda")
        mean, rstd, rm, dg, db = (torch.zeros(C, device="cuda") for _ in range(5))
        rv = torch.ones(C, device="cuda")
        nsets = max(2, -(-(CACHE + (32 << 20)) // (4 * P * C * 2)))
        sets = []
        for _ in range(nsets):
            x = torch.randn((P, C), generator=g, device="cuda").bfloat16()
            dy = (torch.randn((P, C), generator=g, device="cuda") * 1e-3).bfloat16()
            sets.append(dict(x=x, dy=dy, y=torch.empty_like(x), dx=torch.empty_like(x)))
        wsb = L.ssd_bn_ws_bytes(P, C)
        ws = torch.empty((wsb,), dtype=torch.uint8, device="cuda")

        def fwd_train(i):
            s = sets[i % len(sets)]
            _lib.check(L.ssd_bn_fwd_train(Pt(s["x"]), Pt(gamma), Pt(beta), Pt(s["y"]), Pt(mean), Pt(rstd), Pt(rm), Pt(rv), 0.1, 1e-5,
                                          1, Pt(ws), wsb, P, C, S()))

        def fwd_infer(i):
            s = sets[i % len(sets)]
            _lib.check(L.ssd_bn_fwd_infer(Pt(s["x"]), Pt(gamma), Pt(beta), Pt(rm), Pt(rv), Pt(s["y"]), 1e-5, 1, P, C, S()))

        def bwd(i):
            s = sets[i % len(sets)]
            _lib.check(L.ssd_bn_bwd(Pt(s["dy"]), Pt(s["x"]), Pt(gamma), Pt(mean), Pt(rstd), Pt(s["dx"]), Pt(dg), Pt(db), Pt(ws), wsb,
                                    P, C, S()))

        variants = {"ssd_bn_fwd_train": fwd_train, "ssd_bn_fwd_infer": fwd_infer, "ssd_bn_bwd": bwd}
        traffic = {"ssd_bn_fwd_train": 3 * P * C * 2 + 2 * wsb, "ssd_bn_fwd_infer": 2 * P * C * 2, "ssd_bn_bwd": 5 * P * C * 2 + 2 * wsb}
        for fn in variants.values():
            for i in range(2 * len(sets)):
                fn(i)
        torch.cuda.synchronize()
        ms = {k: [] for k in variants}
        for _ in range(args.repeats):
            for name, fn in variants.items():
                ms[name].append(timed(fn, args.calls))
        print("P = %d rows x C = %d; %d calls per repeat over %d operand sets (%.0f MB each); slab partials %.2f MB" % (
            P, C, args.calls, len(sets), 4 * P * C * 2 / 1e6, wsb / 1e6))
        for name in variants:
            report(name, ms[name], traffic[name])
        del sets
else:
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    B = args.batch
    grids = ((64, 64), (32, 32), (16, 16), (8, 8), (4, 4), (2, 2), (1, 1))
    ps = ops.build_priors(grids=grids, s_ref=(20, 51, 133, 215, 297, 379, 461, 543),
                          ratios=((2,), (2, 3), (2, 3), (2, 3), (2, 3), (2,), (2,)), in_size=512)
    cls_l, box_l = synth_batch_gt(5000, B)
    tgt = ops.match_encode(*ops.pack_gt(box_l, cls_l), ps, 0.5)
    img = ops.image_prep(torch.rand((B, 512, 512, 3), device="cuda"), normalize=True)
    engines = {"default": ResNet50SSDEngine(classes=81, seed=0), "batchnorm": ResNet50SSDEngine(classes=81, seed=0, batchnorm=True)}

    def step(eng):
        ploc, pconf = eng.forward(img, train=True)
        hg = eng.head_grad_buffers(B)
        ops.ssd_loss_heads(pconf, ploc, *tgt, hg)
        eng.backward(None, None, heads=hg)
        eng.clip_scales(0.01)
        eng.adam(1e-4, eng.grad, 1.0, True)

    for eng in engines.values():
        for _ in range(2):
            step(eng)
    torch.cuda.synchronize()
    ms = {k: [] for k in engines}
    for _ in range(args.repeats):
        for name, eng in engines.items():
            ms[name].append(timed(lambda i: step(eng), args.steps))
    print("ResNet-50 SSD512 batch %d train step, %d steps per block" % (B, args.steps))
    meds = {name: report(name, ms[name]) for name in engines}
    print("batchnorm - default = %+.3f ms; own spread over the blocks: default %.3f ms, batchnorm %.3f ms" % (
        meds["batchnorm"] - meds["default"], max(ms["default"]) - min(ms["default"]), max(ms["batchnorm"]) - min(ms["batchnorm"])))
