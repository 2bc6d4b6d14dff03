"""Time the device data augmentation against the plain input preparation it replaces.

Batch of `--batch` synth_raw_sample images (bench.py's roofline_prep input), S = 300:
  * kernels: augment_plan + augment_image against box_prep + image_resize_prep, the two alternated, device events, medians;
    augment_image alone, with all stages and without the photometric one;
  * end to end: make_batch_raw with and without augmentation (host packing, copies, kernels, match_encode), host clock around
    work that ends in a device synchronise.
Kernel-only times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python tools_dev/time_augment.py`.
Usage: python tools_dev/time_augment.py [--batch 64] [--iters 50] [--out FILE.json]   (the JSON line is printed either way)"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ssd_object_detection_amd.ops as ops                                                   # noqa: E402
from ssd_object_detection_amd.data_loaders.synthetic import synth_raw_sample                 # noqa: E402
from ssd_object_detection_amd.models import SSDObjectDetectionModel                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    B, S = args.batch, 300
    samples = [synth_raw_sample(i) for i in range(B)]
    imgs, cls_l, box_l = map(list, zip(*samples))
    hw = np.array([im.shape[:2] for im in imgs], np.int32)
    off = np.cumsum([0] + [im.size for im in imgs[:-1]]).astype(np.int64)
    flat = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).cuda()
    off_d, hw_d = torch.from_numpy(off).cuda(), torch.from_numpy(hw).cuda()
    gt_box, gt_cls, gt_off, total, max_nt = ops.pack_gt(box_l, cls_l)
    rel = ops.box_prep(gt_box, gt_off, hw_d)
    out = torch.empty((B, S, S, 8), dtype=torch.bfloat16, device="cuda")

    def plain():
        ops.box_prep(gt_box, gt_off, hw_d)
        ops.image_resize_prep(flat, off_d, hw_d, S, True, out=out)

    def plan_only():
        ops.augment_plan(rel, gt_cls, gt_off, hw_d, total, ops.AUG_ALL, 1, 0)

    params = ops.augment_plan(rel, gt_cls, gt_off, hw_d, total, ops.AUG_ALL, 1, 0)[0]

    params_geom = ops.augment_plan(rel, gt_cls, gt_off, hw_d, total, ops.AUG_EXPAND | ops.AUG_CROP | ops.AUG_FLIP, 1, 0)[0]

    def image_only():
        ops.augment_image(flat, 0, off_d, hw_d, params, S, True, out=out)

    def image_geometry():                                                 # the same draws without the photometric stage
        ops.augment_image(flat, 0, off_d, hw_d, params_geom, S, True, out=out)

    def augmented():
        p = ops.augment_plan(rel, gt_cls, gt_off, hw_d, total, ops.AUG_ALL, 1, 0)[0]
        ops.augment_image(flat, 0, off_d, hw_d, p, S, True, out=out)

    fns = {"plain_prep": plain, "augment": augmented, "augment_plan": plan_only, "augment_image": image_only,
           "augment_image_geometry_only": image_geometry}
    for f in fns.values():                                                # warm-up of every shape
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.iters):                                           # alternated, one event pair per call
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {"batch": B, "S": S, "boxes": total, "device_us_median": {k: float(np.median(v)) for k, v in times.items()},
           "device_us_p10_p90": {k: [float(np.percentile(v, 10)), float(np.percentile(v, 90))] for k, v in times.items()}}

    model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(prefix="time_augment_"), timestamp_dir=False)
    spec = ops.AugmentSpec(seed=1)
    e2e = {"make_batch_raw": lambda: model.make_batch_raw(imgs, cls_l, box_l),
           "make_batch_raw_augment": lambda: model.make_batch_raw(imgs, cls_l, box_l, augment=spec)}
    for f in e2e.values():
        f()
    torch.cuda.synchronize()
    wall = {k: [] for k in e2e}
    for _ in range(max(5, args.iters // 5)):
        for k, f in e2e.items():
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    res["end_to_end_ms_median"] = {k: float(np.median(v)) for k, v in wall.items()}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
