"""Dev: what the model class costs the ResNet-50 SSD512 train step, in one process, on one fixed batch with default Adam.

  (a) the hand-composed loop of tools_dev/time_batchnorm.py --step: forward(train=True), ssd_loss_heads, backward,
      clip_scales, adam on a ResNet50SSDEngine -- engine calls only;
  (b) SSDObjectDetectionModel(network=...)._train_step on the same batch, targets assigned up front (a ResNet model steps
      on the caller's stream: its engine has no side streams);
  (c) (b) with match_async in the loop (target assignment of every step);
  (b-prio) (b) with model.high_priority_main forced on, the loop issued inside `with torch.cuda.stream(model.main_stream())`
      as model.train() issues the SSD300 loop;
  (b-prio-caller) the same issued from the caller's stream: _train_step hands over to its priority stream and back, every step.

For ONE network per process (--network default | batchnorm: a forced-on model owns a high-priority stream, and more streams
than hardware queues in one process measure the queue sharing instead): each loop on its own engine of the same seed, blocks of
STEPS steps alternating in one process.  Median per block; a loop's own min..max over its blocks is the spread a difference
has to exceed.

usage: python tools_dev/time_resnet_model_step.py [--network default] [--batch 16] [--in-size 512] [--steps 5] [--repeats 7]"""
import argparse
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                        # noqa: E402
from ssd_object_detection_amd import ops, optimizers                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--network", choices=("default", "batchnorm"), default="default")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--in-size", type=int, default=512)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"

from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt        # noqa: E402
from ssd_object_detection_amd.models import SSDObjectDetectionModel               # noqa: E402
from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine              # noqa: E402

B, S = args.batch, args.in_size
cls_l, box_l = synth_batch_gt(5000, B)
gt = ops.pack_gt(box_l, cls_l)
img = ops.image_prep(torch.rand((B, S, S, 3), device="cuda"), normalize=True)
log_dir = tempfile.mkdtemp()


def timed(loop, n):
    issue, stream = loop
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):                                 # (None: the caller's stream)
        e0.record()
        for i in range(n):
            issue(i)
        e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                                  # ms per step


def hand_loop(batchnorm):
    eng = ResNet50SSDEngine(classes=81, in_size=S, seed=0, batchnorm=batchnorm)
    ps = ops.build_priors(grids=eng.grids, s_ref=ops.ssd512_s_ref(S), ratios=ops.SSD512_RATIOS, in_size=S)
    tgt = ops.match_encode(*gt, ps, 0.5)

    def step(i):
        ploc, pconf = eng.forward(img, train=True)
        hg = eng.head_grad_buffers(B)
        ops.ssd_loss_heads(pconf, ploc, *tgt, hg)
        eng.backward(None, None, heads=hg)
        eng.clip_scales(0.01)
        eng.adam(1e-4, eng.grad, 1.0, True)
    return step, None


def model_loop(batchnorm, match=False, on_main=True, prio=False):
    model = SSDObjectDetectionModel(80, log_dir, seed=0, timestamp_dir=False,
                                    network=dict(kind="resnet50_ssd512", in_size=S, batchnorm=batchnorm))
    assert not model.high_priority_main
    model.high_priority_main = prio
    opt = optimizers.Adam(1e-4)
    out = [model.match_async(gt)]

    def step(i):
        if match:
            out[0] = model.match_async(gt, out=out[0])
        model._train_step(img, *out[0], opt)
    return step, (model.main_stream() if on_main else None)


bn = True if args.network == "batchnorm" else None
loops = {
    "(a) engine calls": hand_loop(bn),
    "(b) model._train_step": model_loop(bn),
    "(c) (b) + match_async": model_loop(bn, match=True),
    "(b-prio) on a priority stream": model_loop(bn, prio=True),
    "(b-prio-caller) ... handed over": model_loop(bn, prio=True, on_main=False),
}
for loop in loops.values():
    timed(loop, 2)
ms = {k: [] for k in loops}
for _ in range(args.repeats):
    for name, fn in loops.items():
        ms[name].append(timed(fn, args.steps))
print("ResNet-50 SSD512 (%s) train step, batch %d, input %d, %d steps per block, %d blocks" % (
    args.network, B, S, args.steps, args.repeats))
med = {}
for name, v in ms.items():
    med[name] = statistics.median(v)
    print("%-36s median %9.4f ms   min..max %.4f..%.4f   spread %.4f" % (name, med[name], min(v), max(v), max(v) - min(v)))
a = "(a) engine calls"
for other in loops:
    if other != a:
        print("%-36s - (a) = %+.4f ms   ((a)'s own spread %.4f ms)" % (other, med[other] - med[a], max(ms[a]) - min(ms[a])))
