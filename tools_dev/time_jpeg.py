"""Measure the hybrid JPEG decode (ops.decode_jpeg_batch: Huffman on host threads, the rest on the GPU) against Pillow.

    python tools_dev/time_jpeg.py [--batch 64] [--workers 8] [--reps 7] [--inner 4] [--out FILE.json]

One process, one GPU, at most `workers` (<= 16) busy host threads.  The batch is synthesised and encoded here: 640x480
images of gradients, blobs and noise, 4:2:0, quality 90 (needs Pillow, for the encode and for the comparison).  Alternated,
`reps` times each, `inner` batches per timing, host clock around work that ends in a device synchronise:
    pillow    every image decoded by Pillow on a pool of `workers` threads, concatenated, one host-to-device copy
    hybrid    ops.decode_jpeg_batch(workers)
    entropy   the host Huffman stage alone on the same pool (no device work)
and, from device events, the two reconstruct kernels alone; then the batch's SSD300 train step (make_batch_raw + forward,
loss, backward, Adam) fed from the encoded samples against the same step fed from pre-decoded arrays.
Prints one JSON object (medians with min..max); the bytes are checked equal to Pillow's before anything is timed."""
import argparse
import concurrent.futures
import io
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(i, h=480, w=640):
    rng = np.random.default_rng(i)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([xx * (255.0 / w), yy * (255.0 / h), (xx + yy) * (255.0 / (w + h))], -1)
    for _ in range(12):                                              # soft blobs: edges and flat areas, like a photograph
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(20, 160)
        m = ((xx - cx) ** 2 + (yy - cy) ** 2 < r * r)[..., None]
        img = np.where(m, rng.uniform(0, 255, 3).astype(np.float32), img)
    img += rng.normal(0, 6, img.shape).astype(np.float32)            # sensor-like noise: the entropy stage has work to do
    return np.clip(img, 0, 255).astype(np.uint8)


def summary(times, images):
    rate = sorted(images / t for t in times)
    return dict(images_per_s=round(statistics.median(rate), 1), min=round(rate[0], 1), max=round(rate[-1], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    assert 1 <= args.workers <= 16
    import torch
    from PIL import Image
    from ssd_object_detection_amd import _lib, ops
    assert torch.cuda.is_available(), "time_jpeg.py measures on the GPU: no fallback"
    dev = torch.device("cuda", 0)
    L = _lib.lib()

    enc = []
    for i in range(args.batch):
        buf = io.BytesIO()
        Image.fromarray(synth(i)).save(buf, "JPEG", quality=90, subsampling=2)
        enc.append(buf.getvalue())
    pool = concurrent.futures.ThreadPoolExecutor(args.workers)

    def pil_one(data):
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert("RGB"))

    pinned = torch.empty((args.batch * 480 * 640 * 3,), dtype=torch.uint8).pin_memory()

    def run_pillow():
        images = list(pool.map(pil_one, enc))
        np.concatenate([im.reshape(-1) for im in images], out=pinned.numpy())
        return pinned.to(dev, non_blocking=True)

    def run_hybrid():
        return ops.decode_jpeg_batch(enc, dev, workers=args.workers)[0]

    need = [ops.jpeg_info(d)["ncoef"] for d in enc]
    coefs = [np.empty(n, np.int16) for n in need]

    def entropy_one(k):
        return L.ssd_jpeg_entropy_decode(enc[k], len(enc[k]), coefs[k].ctypes.data, need[k], None)

    def run_entropy():
        assert not any(pool.map(entropy_one, range(args.batch)))

    want, got = run_pillow(), run_hybrid()
    torch.cuda.synchronize()
    assert torch.equal(want, got), "the hybrid decode differs from Pillow's"
    times = {"pillow": [], "hybrid": [], "entropy": []}
    for fn in (run_pillow, run_hybrid, run_entropy):                 # warm-up
        fn()
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for name, fn in (("pillow", run_pillow), ("hybrid", run_hybrid), ("entropy", run_entropy)):
            t0 = time.perf_counter()
            for _ in range(args.inner):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.inner)
    result = {k: summary(v, args.batch) for k, v in times.items()}
    result.update(batch=args.batch, workers=args.workers, reps=args.reps, inner=args.inner,
                  encoded_mb=round(sum(map(len, enc)) / 1e6, 2), coef_mb=round(2 * sum(need) / 1e6, 1),
                  pixel_mb=round(args.batch * 480 * 640 * 3 / 1e6, 1), device=torch.cuda.get_device_name(0))

    # the reconstruct kernels alone, from device events
    total = sum(need)
    g = _lib.CONSTANTS
    desc = np.zeros((args.batch, ops.JPEG_REC_WORDS), np.int32)
    base = 0
    for k, d in enumerate(enc):
        desc[k] = ops.jpeg_info(d)["rec"]
        desc[k, g["SSD_JPEG_COEF_OFF"]:g["SSD_JPEG_COEF_OFF"] + 3] += base
        base += need[k]
    run_entropy()
    coef_d = torch.from_numpy(np.concatenate(coefs)).to(dev)
    desc_d = torch.from_numpy(desc).to(dev)
    off_d = torch.arange(args.batch, dtype=torch.int64, device=dev) * (480 * 640 * 3)
    dst = torch.empty_like(want)
    scratch = torch.empty((total,), dtype=torch.uint8, device=dev)
    ops.jpeg_reconstruct(coef_d, desc_d, dst, off_d, scratch)
    assert torch.equal(dst, want)
    ev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            ops.jpeg_reconstruct(coef_d, desc_d, dst, off_d, scratch)
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b) / 20)
    result["reconstruct_ms"] = dict(median=round(statistics.median(ev), 4), min=round(min(ev), 4), max=round(max(ev), 4))
    moved = 2 * total + 2 * total + want.numel()                     # coefficients in, planes out and in again, pixels out
    result["reconstruct_gb_per_s"] = round(moved / (statistics.median(ev) * 1e-3) / 1e9, 1)

    if not args.no_train:
        from ssd_object_detection_amd import optimizers
        from ssd_object_detection_amd.data_loaders.synthetic import synth_gt
        from ssd_object_detection_amd.models import SSDObjectDetectionModel
        import tempfile
        model = SSDObjectDetectionModel(classes=80, log_dir=tempfile.mkdtemp(prefix="time_jpeg_"), timestamp_dir=False)
        model.decode_workers = args.workers
        opt = optimizers.Adam(1e-4)
        gt = [synth_gt(i) for i in range(args.batch)]
        cls = [c for c, _ in gt]
        box = [np.asarray(b, np.float32) * np.float32([640, 480, 640, 480]) for _, b in gt]
        box = [np.concatenate([b[:, :2] - b[:, 2:] / 2, b[:, 2:]], 1) for b in box]       # centre -> top-left pixels
        encoded = [ops.EncodedImage(d, 480, 640) for d in enc]
        decoded = [pil_one(d) for d in enc]

        def step(images):
            x, (c, l, m) = model.make_batch_raw(images, cls, box)
            model._train_step(x, c, l, m, opt)

        steps = {"step_encoded": [], "step_decoded": []}
        for images in (encoded, decoded):
            step(images)
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, images in (("step_encoded", encoded), ("step_decoded", decoded)):
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    step(images)
                torch.cuda.synchronize()
                steps[name].append((time.perf_counter() - t0) / args.inner)
        result.update({k: summary(v, args.batch) for k, v in steps.items()})
    text = json.dumps(result)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    pool.shutdown()


if __name__ == "__main__":
    main()
