"""Time the evaluation pass: evaluate() over synthetic validation samples, wall time per image.

512 samples, batch 64, score threshold 0.05, head biases spread as in tests/test_eval_device_gpu.py (conf: background +2,
classes N(0, 1.5)) so that scoring and NMS have work; one warm-up pass, then the median of `--passes` passes per metric mode,
the modes alternated.  A tree without the device metric (no `metric` argument) is timed in its only mode; one with the
multi-label detection output (a `scoring` argument) also in "host+all" and "device+all" (evaluate(scoring="all")).
Kernel times: a run of its own under `rocprofv3 --kernel-trace --stats -- python tools_dev/time_eval.py --passes 1`.
Usage: python tools_dev/time_eval.py [--samples 512] [--batch 64] [--passes 5] [--out FILE.json]"""
import argparse
import inspect
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ssd_object_detection_amd.data_loaders.synthetic import synth_gt, synth_image            # noqa: E402
from ssd_object_detection_amd.models import SSDObjectDetectionModel                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the result to this JSON file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(prefix="time_eval_"), timestamp_dir=False, seed=4)
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
    modes = ["host", "device"] if "metric" in inspect.signature(model.evaluate).parameters else [None]
    if "scoring" in inspect.signature(model.evaluate).parameters:
        modes += ["host+all", "device+all"]

    def run(mode):
        kw = {} if mode is None else {"metric": mode.split("+")[0]}
        if mode is not None and mode.endswith("+all"):
            kw["scoring"] = "all"
        t0 = time.perf_counter()
        r = model.evaluate(samples, batch_size=args.batch, score_thresh=0.05, **kw)     # ends in a device-to-host read
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    results = {m: run(m)[1] for m in modes}                                   # warm-up of every mode
    times = {m: [] for m in modes}
    for _ in range(args.passes):
        for m in modes:
            times[m].append(run(m)[0])
    res = {"samples": args.samples, "batch": args.batch, "device": torch.cuda.get_device_name(0),
           "ms_per_image_median": {str(m): float(np.median(v)) / args.samples * 1e3 for m, v in times.items()},
           "ms_per_image_min_max": {str(m): [min(v) / args.samples * 1e3, max(v) / args.samples * 1e3] for m, v in times.items()},
           "mAP": {str(m): r["mAP"] for m, r in results.items()}}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
