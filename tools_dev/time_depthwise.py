"""Dev: the depthwise 3x3 convolution's three passes at the batch-64 depthwise shapes of a MobileNet-v1 trunk at 300 x 300, and the
forward / data gradient against the 3x3 / stride-1 max pooling at (BATCH, 19, 19, 512).

Per shape (H, W, C, stride): ssd_dwconv3x3_fwd (bias + ReLU), ssd_dwconv3x3_bwd_data (no relu_src; at the yardstick shape also
with one) and ssd_dwconv3x3_bwd_weight (with dbias), in microseconds and in achieved bytes per second of the bytes a call must
move: x + y for the forward pass, dy + dx (+ relu_src) for the data gradient, x + dy for the weight gradient.  The yardsticks,
ops.maxpool3x3s1_fwd / _bwd, have the same 3x3 access pattern and move 4.5 bytes per element (x, y and the code; dy, dx and the
code) where the depthwise passes move 4; they are alternated with the stride-1 depthwise calls inside every repeat.
One call's operands would stay in the 256 MiB Infinity Cache from call to call, which a layer never sees inside a step: the calls
rotate through operand sets of more than 256 MiB together.  Device events around CALLS calls after warm-up; median of the REPEATS
per-call times, min..max beside it.  Every shape runs in a child process of its own under a time limit; the first failure ends
the run.

--forms: the sign-byte forms instead.  Per shape, alternated in one process: ssd_dwconv3x3_fwd against ssd_dwconv3x3_fwd_relubits, and
the data gradient plain, masked from relu_src (6 bytes per element) and masked from sign bytes (ssd_dwconv3x3_bwd_data_bits: 4.125).
Then the sums over the trunk's masked depthwise data gradients: the twelve behind a 1x1 layer (and, beside them, all thirteen: the
first is masked by the stem), per form, with the summed min and max -- the sign-byte form is the engine's default only if it is
faster in the sum of the twelve by more than the relu_src form's own min..max.

usage: python tools_dev/time_depthwise.py [--forms] [--batch 64] [--calls 20] [--repeats 7] [--limit 120]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (H, W, C, stride): the depthwise layers of MobileNet-v1 at 300 x 300
SHAPES = [(150, 150, 32, 1), (150, 150, 64, 2), (75, 75, 128, 1), (75, 75, 128, 2), (38, 38, 256, 1), (38, 38, 256, 2),
          (19, 19, 512, 1), (19, 19, 512, 2), (10, 10, 1024, 1)]
YARDSTICK = (19, 19, 512, 1)
# how often the trunk runs each shape's data gradient behind a 1x1 layer (the first depthwise layer sits behind the stem)
BEHIND_1X1 = [0, 1, 1, 1, 1, 1, 5, 1, 1]
CACHE = 256 << 20

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--limit", type=int, default=120, help="seconds per child process")
ap.add_argument("--only", type=int, default=None, help="(child) index into SHAPES, or -1 for the yardstick comparison")
ap.add_argument("--forms", action="store_true", help="the sign-byte forms against their siblings, and the trunk's sums")
args = ap.parse_args()

if args.only is None and args.forms:
    rows = []
    for i in range(len(SHAPES)):
        cmd = [sys.executable, os.path.abspath(__file__), "--forms", "--batch", str(args.batch), "--calls", str(args.calls), "--repeats",
               str(args.repeats), "--only", str(i)]
        done = subprocess.run(cmd, timeout=args.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.exit("step %d ended with status %d: stopping" % (i, done.returncode))
        rows.append(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith("FORMS ")][-1][6:]))
    for title, mult in (("the twelve behind a 1x1 layer", BEHIND_1X1), ("all thirteen", [m + (i == 0) for i, m in enumerate(BEHIND_1X1)])):
        print("masked depthwise data gradients of one step, %s (us: median, summed min..max):" % title)
        tot = {k: [sum(m * r[k][j] for m, r in zip(mult, rows)) for j in range(3)] for k in ("dgrad", "dgrad + relu_src", "dgrad + bits")}
        for k, (med, lo, hi) in tot.items():
            print("  %-20s %8.1f   %.1f..%.1f" % (k, med, lo, hi))
        src, bits = tot["dgrad + relu_src"], tot["dgrad + bits"]
        print("  relu_src - bits = %.1f us; relu_src's own min..max = %.1f us -> %s" % (
            src[0] - bits[0], src[2] - src[1], "sign bytes" if src[0] - bits[0] > src[2] - src[1] else "relu_src"), flush=True)
    sys.exit(0)

if args.only is None:
    for i in list(range(len(SHAPES))) + [-1]:
        cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--calls", str(args.calls), "--repeats",
               str(args.repeats), "--only", str(i)]
        rc = subprocess.run(cmd, timeout=args.limit).returncode
        if rc != 0:
            sys.exit("step %d ended with status %d: stopping" % (i, rc))
    sys.exit(0)

import torch                                                        # noqa: E402
from ssd_object_detection_amd import ops                            # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the GPU"
BF = torch.bfloat16
B = args.batch


def timed(issue, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        issue(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3                            # us per call


def report(name, us, nbytes):
    med = statistics.median(us)
    print("  %-28s median %8.1f us   min..max %.1f..%.1f   %.2f TB/s of %.1f MB" % (name, med, min(us), max(us), nbytes / (med * 1e-6) / 1e12,
                                                                                  nbytes / 1e6), flush=True)
    return med


def operand_sets(H, W, C, stride, pool):
    Ho, pt = ops.same_pad(H, 3, stride)
    Wo, pl = ops.same_pad(W, 3, stride)
    g = torch.Generator(device="cuda").manual_seed(1)
    nx, ny = B * H * W * C, B * Ho * Wo * C
    per_set = 2 * (nx + ny)                                         # the smallest pass's bytes: every pass must rotate past the cache
    sets = []
    for _ in range(max(2, -(-(CACHE + (32 << 20)) // per_set))):
        x = torch.randn((B, H, W, C), generator=g, device="cuda").relu().to(BF)
        dy = (torch.randn((B, Ho, Wo, C), generator=g, device="cuda") * 1e-2).to(BF)
        s = dict(x=x, dy=dy, y=torch.empty_like(dy), dx=torch.empty_like(x),
                 w=(torch.randn((3, 3, C), generator=g, device="cuda") * (2.0 / 9) ** 0.5).to(BF), bias=torch.zeros(C, device="cuda"),
                 dw=torch.empty((3, 3, C), device="cuda"), db=torch.empty(C, device="cuda"))
        if pool:
            s["code"] = torch.empty((B, H, W, C // 8), dtype=torch.int32, device="cuda")
            ops.maxpool3x3s1_fwd(x, out=s["y"], code=s["code"])
        sets.append(s)
    return sets, (Ho, Wo, pt, pl), nx, ny


def measure(variants):
    for fn in variants.values():
        for i in range(2 * len(sets)):
            fn(i)
    torch.cuda.synchronize()
    us = {k: [] for k in variants}
    for _ in range(args.repeats):
        for name, fn in variants.items():
            us[name].append(timed(fn, args.calls))
    return us


if args.only >= 0 and args.forms:
    H, W, C, stride = SHAPES[args.only]
    sets, (Ho, Wo, pt, pl), nx, ny = operand_sets(H, W, C, stride, False)
    for s in sets:                                                  # the map in front (about half of it positive) and its sign bytes
        s["src"] = torch.randn((B, H, W, C), device="cuda").relu().to(BF)
        s["xbits"] = ((s["src"] > 0).view(B, H, W, C // 8, 8).int() << torch.arange(8, device="cuda", dtype=torch.int32)).sum(-1).to(torch.uint8)
        s["ybits"] = torch.empty((B, Ho, Wo, C // 8), dtype=torch.uint8, device="cuda")
    S = lambda i: sets[i % len(sets)]                               # noqa: E731
    us = measure({
        "fwd": lambda i: ops.dwconv3x3_fwd(S(i)["x"], S(i)["w"], S(i)["bias"], stride, pt, pl, Ho, Wo, True, out=S(i)["y"]),
        "fwd_relubits": lambda i: ops.dwconv3x3_fwd_relubits(S(i)["x"], S(i)["w"], S(i)["bias"], stride, pt, pl, Ho, Wo, S(i)["ybits"],
                                                             out=S(i)["y"]),
        "dgrad": lambda i: ops.dwconv3x3_bwd_data(S(i)["dy"], S(i)["w"], None, (B, H, W, C), stride, pt, pl, out=S(i)["dx"]),
        "dgrad + relu_src": lambda i: ops.dwconv3x3_bwd_data(S(i)["dy"], S(i)["w"], S(i)["src"], (B, H, W, C), stride, pt, pl, out=S(i)["dx"]),
        "dgrad + bits": lambda i: ops.dwconv3x3_bwd_data_bits(S(i)["dy"], S(i)["w"], S(i)["xbits"], (B, H, W, C), stride, pt, pl, out=S(i)["dx"]),
    })
    print("(%d, %d, %d, %d) stride %d -> %d x %d; %d operand sets" % (B, H, W, C, stride, Ho, Wo, len(sets)), flush=True)
    nbytes = {"fwd": 2 * (nx + ny), "fwd_relubits": 2 * (nx + ny) + ny // 8, "dgrad": 2 * (nx + ny), "dgrad + relu_src": 4 * nx + 2 * ny,
              "dgrad + bits": 2 * (nx + ny) + nx // 8}
    for name in us:
        report("dwconv3x3 " + name, us[name], nbytes[name])
    print("FORMS " + json.dumps({k: [statistics.median(v), min(v), max(v)] for k, v in us.items()}), flush=True)
elif args.only >= 0:
    H, W, C, stride = SHAPES[args.only]
    sets, (Ho, Wo, pt, pl), nx, ny = operand_sets(H, W, C, stride, False)
    S = lambda i: sets[i % len(sets)]                               # noqa: E731
    us = measure({
        "fwd": lambda i: ops.dwconv3x3_fwd(S(i)["x"], S(i)["w"], S(i)["bias"], stride, pt, pl, Ho, Wo, True, out=S(i)["y"]),
        "dgrad": lambda i: ops.dwconv3x3_bwd_data(S(i)["dy"], S(i)["w"], None, (B, H, W, C), stride, pt, pl, out=S(i)["dx"]),
        "wgrad": lambda i: ops.dwconv3x3_bwd_weight(S(i)["x"], S(i)["dy"], stride, pt, pl, dw=S(i)["dw"], dbias=S(i)["db"]),
    })
    print("(%d, %d, %d, %d) stride %d -> %d x %d; %d operand sets" % (B, H, W, C, stride, Ho, Wo, len(sets)), flush=True)
    for name in us:
        report("dwconv3x3 " + name, us[name], 2 * (nx + ny))
else:
    H, W, C, stride = YARDSTICK
    sets, (Ho, Wo, pt, pl), nx, ny = operand_sets(H, W, C, stride, True)
    S = lambda i: sets[i % len(sets)]                               # noqa: E731
    us = measure({
        "maxpool3x3s1 fwd": lambda i: ops.maxpool3x3s1_fwd(S(i)["x"], out=S(i)["y"], code=S(i)["code"]),
        "dwconv3x3 fwd": lambda i: ops.dwconv3x3_fwd(S(i)["x"], S(i)["w"], S(i)["bias"], 1, pt, pl, Ho, Wo, True, out=S(i)["y"]),
        "maxpool3x3s1 bwd": lambda i: ops.maxpool3x3s1_bwd(S(i)["code"], S(i)["dy"], (B, H, W, C), out=S(i)["dx"]),
        "dwconv3x3 dgrad": lambda i: ops.dwconv3x3_bwd_data(S(i)["dy"], S(i)["w"], None, (B, H, W, C), 1, pt, pl, out=S(i)["dx"]),
        "dwconv3x3 dgrad + relu_src": lambda i: ops.dwconv3x3_bwd_data(S(i)["dy"], S(i)["w"], S(i)["x"], (B, H, W, C), 1, pt, pl,
                                                                       out=S(i)["dx"]),
    })
    print("yardsticks, alternated in one process at (%d, %d, %d, %d); %d operand sets" % (B, H, W, C, len(sets)), flush=True)
    nbytes = {"maxpool3x3s1 fwd": 4 * nx + nx // 2, "dwconv3x3 fwd": 4 * nx, "maxpool3x3s1 bwd": 4 * nx + nx // 2, "dwconv3x3 dgrad": 4 * nx,
              "dwconv3x3 dgrad + relu_src": 6 * nx}
    med = {name: report(name, us[name], nbytes[name]) for name in us}
    for a, b in (("dwconv3x3 fwd", "maxpool3x3s1 fwd"), ("dwconv3x3 dgrad", "maxpool3x3s1 bwd")):
        print("  %s / %s = %.2f; the yardstick's max: %.1f us" % (a, b, med[a] / med[b], max(us[b])), flush=True)
