"""Dev: the atrous 3x3 convolution and the 3x3 / stride-1 max pooling at fc6 / pool5's training shape, in one process.

Atrous: ssd_conv2d_atrous_fwd / _bwd_data / _bwd_weight at (BATCH, 19, 19, 512 -> 1024, dilation 6).  The yardstick is the
project's tuned ordinary convolution -- ops.conv2d_fwd / conv2d_bwd_data / conv2d_bwd_weight on the same shape at dilation 1
(3x3, stride 1, pad 1): the same FLOPs and the same bytes -- alternated with the atrous calls inside every repeat.  Pooling:
ssd_maxpool3x3s1_fwd / _bwd at (BATCH, 19, 19, 512), with the bytes a call must move (forward: x read, y and code written;
backward: dy and code read, dx written).  One call's operands would stay in the 256 MiB Infinity Cache from call to call, which
a layer never sees inside a step: the calls rotate through operand sets of more than 256 MiB together.  Device events around
CALLS calls after warm-up; median of the REPEATS per-call times, min..max beside it.  The MFMA calibration loop of bench.py
(ssd_dev_mfma_calibration) runs in the same process: the atrous rates are also given as a fraction of it.

usage: python tools_dev/time_atrous.py [--batch 64] [--calls 20] [--repeats 7]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import _lib, ops                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

B, H, W, CIN, COUT, D = args.batch, 19, 19, 512, 1024, 6
CACHE = 256 << 20
BF = torch.bfloat16


def timed(issue, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        issue(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                                  # ms per call


def report(name, ms, flop=None, nbytes=None, calib=None):
    med = statistics.median(ms)
    tail = ""
    if flop:
        tf = flop / (med * 1e-3) / 1e12
        tail += "  %.0f TFLOP/s" % tf
        if calib:
            tail += " (%.2f of the calibration loop)" % (tf / calib)
    if nbytes:
        tail += "  %.2f TB/s" % (nbytes / (med * 1e-3) / 1e12)
    print("%-30s median %8.4f ms   min..max %.4f..%.4f   (%d repeats)%s" % (name, med, min(ms), max(ms), len(ms), tail))
    return med


def calibration(target_ms=60.0):
    L = _lib.lib()
    nwg = L.ssd_dev_mfma_calibration_workgroups()
    stamps = torch.zeros((2 * nwg,), dtype=torch.int64, device="cuda")
    sink = torch.empty((512 * nwg,), dtype=torch.float32, device="cuda")

    def run(iters):
        _lib.check(L.ssd_dev_mfma_calibration(iters, ops._ptr(stamps), ops._ptr(sink), ops._stream()))
    it0 = 2000
    for _ in range(2):
        run(it0)
    t = timed(lambda i: run(it0), 3) * 1e-3
    iters = max(it0, int(it0 * target_ms * 1e-3 / t))
    t = timed(lambda i: run(iters), 1) * 1e-3
    return L.ssd_dev_mfma_calibration_flops(iters) / t / 1e12


g = torch.Generator(device="cuda").manual_seed(1)
per_set = 2 * (B * H * W * (2 * CIN + 2 * COUT) + 2 * COUT * 9 * CIN) + 4 * COUT * 9 * CIN
nsets = max(2, -(-(CACHE + (32 << 20)) // per_set))
sets = []
for _ in range(nsets):
    x = torch.randn((B, H, W, CIN), generator=g, device="cuda").relu().to(BF)
    w = (torch.randn((COUT, 3, 3, CIN), generator=g, device="cuda") * (2.0 / (9 * CIN)) ** 0.5).to(BF)
    dy = (torch.randn((B, H, W, COUT), generator=g, device="cuda") * 1e-2).to(BF)
    sets.append(dict(x=x, w=w, w_t=ops.weight_transpose(w), dy=dy, bias=torch.zeros(COUT, device="cuda"), y=torch.empty_like(dy),
                     dx=torch.empty_like(x), dw=torch.empty((COUT, 3, 3, CIN), device="cuda"), db=torch.empty(COUT, device="cuda")))


def S(i):
    return sets[i % len(sets)]


variants = {
    "atrous fwd  (d = 6)": lambda i: ops.conv2d_atrous_fwd(S(i)["x"], S(i)["w"], S(i)["bias"], D, True, out=S(i)["y"]),
    "conv2d fwd  (d = 1)": lambda i: ops.conv2d_fwd(S(i)["x"], S(i)["w"], S(i)["bias"], 1, 1, 1, H, W, True, out=S(i)["y"]),
    "atrous dgrad (d = 6)": lambda i: ops.conv2d_atrous_bwd_data(S(i)["dy"], S(i)["w_t"], S(i)["x"], (B, H, W, CIN), D, out=S(i)["dx"]),
    "conv2d dgrad (d = 1)": lambda i: ops.conv2d_bwd_data(S(i)["dy"], S(i)["w_t"], S(i)["x"], (B, H, W, CIN), 1, 1, 1, out=S(i)["dx"]),
    "atrous wgrad (d = 6)": lambda i: ops.conv2d_atrous_bwd_weight(S(i)["x"], S(i)["dy"], COUT, D, dw=S(i)["dw"], dbias=S(i)["db"]),
    "conv2d wgrad (d = 1)": lambda i: ops.conv2d_bwd_weight(S(i)["x"], S(i)["dy"], COUT, 3, 1, 1, 1, dw=S(i)["dw"], dbias=S(i)["db"]),
}
for fn in variants.values():
    for i in range(2 * len(sets)):
        fn(i)
torch.cuda.synchronize()
calib = calibration()
ms = {k: [] for k in variants}
for _ in range(args.repeats):
    for name, fn in variants.items():
        ms[name].append(timed(fn, args.calls))
flop = 2.0 * B * H * W * 9 * CIN * COUT
print("fc6: (%d, %d, %d, %d -> %d), %.1f GFLOP per pass; %d calls per repeat over %d operand sets (%.0f MB each); "
      "MFMA calibration loop %.0f TFLOP/s" % (B, H, W, CIN, COUT, flop / 1e9, args.calls, len(sets), per_set / 1e6, calib))
med = {name: report(name, ms[name], flop=flop, calib=calib) for name in variants}
for p in ("fwd ", "dgrad", "wgrad"):
    a, c = ("atrous %s (d = 6)" % p, "conv2d %s (d = 1)" % p)
    print("%s: atrous / conv2d = %.2f; spreads (max - min): atrous %.4f ms, conv2d %.4f ms" % (
        p.strip(), med[a] / med[c], max(ms[a]) - min(ms[a]), max(ms[c]) - min(ms[c])))
del sets

# ---- pool5
C = 512
n = B * H * W * C
psets = []
for _ in range(max(2, -(-(CACHE + (32 << 20)) // (n * 2 * 4 + n // 2)))):
    x = torch.randn((B, H, W, C), generator=g, device="cuda").relu().to(BF)
    dy = (torch.randn((B, H, W, C), generator=g, device="cuda") * 1e-2).to(BF)
    y, code = ops.maxpool3x3s1_fwd(x)
    psets.append(dict(x=x, dy=dy, y=y, code=code, dx=torch.empty_like(x)))


def Q(i):
    return psets[i % len(psets)]


pool = {
    "maxpool3x3s1 fwd": lambda i: ops.maxpool3x3s1_fwd(Q(i)["x"], out=Q(i)["y"], code=Q(i)["code"]),
    "maxpool3x3s1 bwd": lambda i: ops.maxpool3x3s1_bwd(Q(i)["code"], Q(i)["dy"], (B, H, W, C), out=Q(i)["dx"]),
}
for fn in pool.values():
    for i in range(2 * len(psets)):
        fn(i)
torch.cuda.synchronize()
pms = {k: [] for k in pool}
for _ in range(args.repeats):
    for name, fn in pool.items():
        pms[name].append(timed(fn, args.calls))
print("pool5: (%d, %d, %d, %d); %d operand sets" % (B, H, W, C, len(psets)))
for name in pool:
    report(name, pms[name], nbytes=2 * n * 2 + n // 2)
