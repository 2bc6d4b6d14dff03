"""Time the PASCAL VOC protocol of the device metric beside the default one: evaluate(metric="device",
protocol="map") and protocol="voc07" alternated in one process over the synthetic validation samples of tools_dev/time_eval.py
(512 samples, batch 64, threshold 0.05, head biases spread, no difficult box), wall time per image, median of `--passes` with
the spread; and the two match kernels (per batch of 64) and the AP kernels (once per pass: k_eval_ap_voc for both years) alone,
by device events (median of `--passes` blocks of `--calls` launches), on the maps and rows of the same samples.
Usage: python tools_dev/time_voc_eval.py [--samples 512] [--batch 64] [--passes 7] [--calls 200] [--out FILE.json]"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ssd_object_detection_amd import _lib, ops                                                 # noqa: E402
from ssd_object_detection_amd.data_loaders.synthetic import synth_gt, synth_image            # noqa: E402
from ssd_object_detection_amd.models import SSDObjectDetectionModel                          # noqa: E402


def events_us(fn, calls, passes):
    """median, min, max over `passes` blocks of the mean time of `calls` launches, microseconds"""
    out = []
    for _ in range(passes + 1):                                               # the first block warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    out = out[1:]
    return [float(np.median(out)), float(min(out)), float(max(out))]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


THR, PTS, PTS_VOC = np.linspace(0.5, 0.95, 10), np.linspace(0.0, 1.0, 101), np.arange(11) / 10.0


def bound_match(rec, voc, max_dets=100):
    """a launch of ssd_eval_match / ssd_eval_match_voc through the C ABI on preallocated outputs: no allocation and no
    wrapper between two launches, so that the events time the kernel and not the host"""
    L = _lib.lib()
    score, cls, box, keep, gt_cls, gt_box, gt_off = rec
    B, A = score.shape
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device="cuda")                        # noqa: E731
    outs = [e((B,), torch.int32), e((B, max_dets), torch.float32), e((B, max_dets), torch.int32), e((B, max_dets, 4), torch.float32)]
    outs += [e((B, max_dets), torch.uint8), e((B, max_dets), torch.int32)] if voc else [e((B, max_dets), torch.int16)]
    ins = [_p(score), _p(cls), _p(box), _p(keep), B, A, _p(gt_cls), _p(gt_box), _p(gt_off)]
    ptrs = [_p(t) for t in outs]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if voc:
        return lambda _keep=outs: _lib.check(L.ssd_eval_match_voc(*ins, None, 0.5, max_dets, *ptrs, st))
    return lambda _keep=outs: _lib.check(L.ssd_eval_match(*ins, _dp(THR), max_dets, *ptrs, st))


def bound_ap(inputs, C, year):
    """year None: ssd_eval_ap; 7 / 12: ssd_eval_ap_voc"""
    L = _lib.lib()
    ap = torch.empty((C, 10), dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = [_p(t) for t in inputs]
    if year:
        return lambda _keep=(inputs, ap): _lib.check(L.ssd_eval_ap_voc(*ptrs, C, year, _dp(PTS_VOC), _p(ap), st))
    return lambda _keep=(inputs, ap): _lib.check(L.ssd_eval_ap(*ptrs, C, _dp(PTS), _p(ap), st))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(prefix="time_voc_eval_"), timestamp_dir=False, seed=4)
    eng = model.get_engine()
    g = torch.Generator().manual_seed(0)
    for lvl, (wt, bt) in enumerate(eng.head_params):
        n = eng.num_priors[lvl]
        b = torch.zeros(bt.numel)
        cb = torch.randn((n, 81), generator=g) * 1.5
        cb[:, 80] += 2.0
        b[n * 4:] = cb.reshape(-1)
        eng.param[bt.offset:bt.offset + bt.numel] = b.cuda()
    samples = [(synth_image((1 << 20) + i),) + synth_gt((1 << 20) + i) for i in range(args.samples)]
    modes = ["map", "voc07"]

    def run(mode):
        t0 = time.perf_counter()
        r = model.evaluate(samples, batch_size=args.batch, score_thresh=0.05, metric="device", protocol=mode)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    results = {m: run(m)[1] for m in modes}                                   # warm-up of both
    times = {m: [] for m in modes}
    for _ in range(args.passes):
        for m in modes:
            times[m].append(run(m)[0])

    # the kernels alone: the first batch's dense maps, and the rows of all batches
    size = float(model.cfg.input_shape[0])
    C = model.cfg.classes - 1
    recs = []
    for b0 in range(0, args.samples, args.batch):
        buf = samples[b0:b0 + args.batch]
        img = torch.from_numpy(np.stack([np.asarray(s[0], np.float32) for s in buf], 0)).cuda()
        x = ops.image_prep(((img - 0.5) * 2).contiguous(), normalize=False)
        score, cls, box, keep = model._detect_prepared(x, 0.05, 0.45)
        off = np.zeros(len(buf) + 1, np.int32)
        off[1:] = np.cumsum([len(s[1]) for s in buf])
        gt_cls = torch.from_numpy(np.concatenate([np.asarray(s[1]).reshape(-1) for s in buf]).astype(np.int32)).cuda()
        gt_box = torch.from_numpy(np.concatenate([np.asarray(s[2], np.float32).reshape(-1, 4) for s in buf])).cuda().double() * size
        recs.append((score, cls, box, keep, gt_cls, gt_box, torch.from_numpy(off).cuda()))
    first = recs[0]
    kernels = {"k_eval_match": events_us(bound_match(first, False), args.calls, args.passes),
               "k_eval_match_voc": events_us(bound_match(first, True), args.calls, args.passes)}
    old = [ops.eval_match(*r, 100) for r in recs]
    new = [ops.eval_match_voc(*r, 100) for r in recs]
    assert all(torch.equal(o[1], n.score) and torch.equal(o[2], n.cls) for o, n in zip(old, new))     # the same rows
    score = torch.cat([o[1] for o in old]).reshape(-1)
    cls = torch.cat([o[2] for o in old]).reshape(-1)
    bits = (score + 0.0).view(torch.int32).to(torch.int64)
    ordered = torch.where(bits < 0, bits ^ 0x7fffffff, bits)
    cls_key = torch.where(cls < 0, torch.full_like(cls, C), cls).to(torch.int64)
    order = torch.sort((cls_key << 32) | (0x7fffffff - ordered), stable=True).indices
    seg_off = torch.zeros((C + 1,), dtype=torch.int32, device="cuda")
    seg_off[1:] = torch.cumsum(torch.bincount(cls_key, minlength=C + 1)[:C], 0).to(torch.int32)
    gt = torch.cat([r[4] for r in recs]).to(torch.int64)
    n_gt = torch.bincount(gt, minlength=C)[:C].to(torch.int32)
    flags = torch.cat([o[4] for o in old]).reshape(-1)[order].contiguous()
    flags_voc = torch.cat([n.flags for n in new]).reshape(-1)[order].contiguous()
    kernels["k_eval_ap"] = events_us(bound_ap((flags, seg_off, n_gt), C, None), args.calls, args.passes)
    kernels["k_eval_ap_voc_07"] = events_us(bound_ap((flags_voc, seg_off, n_gt), C, 7), args.calls, args.passes)
    kernels["k_eval_ap_voc_12"] = events_us(bound_ap((flags_voc, seg_off, n_gt), C, 12), args.calls, args.passes)
    rows_per_class = (seg_off[1:] - seg_off[:-1]).cpu().numpy()

    res = {"samples": args.samples, "batch": args.batch, "passes": args.passes, "device": torch.cuda.get_device_name(0),
           "ms_per_image_median": {m: float(np.median(v)) / args.samples * 1e3 for m, v in times.items()},
           "ms_per_image_min_max": {m: [min(v) / args.samples * 1e3, max(v) / args.samples * 1e3] for m, v in times.items()},
           "kernel_us_median_min_max": kernels, "rows": int(flags.numel()),
           "rows_per_class_max": int(rows_per_class.max()),
           "summary": {m: {k: v for k, v in r.items() if not k.startswith("per_class")} for m, r in results.items()}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
