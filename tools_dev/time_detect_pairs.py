"""Dev helper: the multi-label detection output (ops.detect_pairs) at batch 64 on the bench's NMS input, beside the single-label
pair score_decode + nms on the same tensors in the same run (fp32 and bf16 logits).  Thresholds 0.3 (every pair listed, no
cut), 0.05 (the exact cut from the list) and 0.01 (the list overflows: rescan of the logits).  With AB_LIB naming a
-DSSD_DEV_ABLATE build of the library, also the time up to each stage of k_detect_pairs."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from ssd_object_detection_amd import _lib
if os.environ.get('AB_LIB'):
    _lib.LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), os.environ['AB_LIB'])
import ssd_object_detection_amd.ops as ops
B = 64
pset = ops.build_priors()
L = _lib.lib()
for dt in (torch.float32, torch.bfloat16):
    conf, loc = bench.nms_inputs(torch, B, pset.A, dt)
    sd = ops.score_decode(conf, loc, pset, 0.3)
    t_sd = bench.graph_timed(torch, lambda: ops.score_decode(conf, loc, pset, 0.3), 30)
    t_nms = bench.graph_timed(torch, lambda: ops.nms(sd[0], sd[1], sd[2], sd[3], 0.45, 400), 30)
    t_cs = bench.graph_timed(torch, lambda: ops.class_scores(conf), 30)
    print(dt, "score_decode %.1f us + nms %.1f us = %.1f us   class_scores %.1f us" % (t_sd * 1e6, t_nms * 1e6, (t_sd + t_nms) * 1e6,
          t_cs * 1e6), flush=True)
    for thresh in (0.3, 0.05, 0.01):
        d = ops.detect_pairs(conf, loc, pset, thresh)
        nc = d.n_cand.float()
        t = bench.graph_timed(torch, lambda: ops.detect_pairs(conf, loc, pset, thresh), 30)
        print("   detect_pairs thresh %.2f: %.1f us  (x%.2f of the pair)  candidates per image %.0f .. %.0f, rows %.0f" % (
              thresh, t * 1e6, t / (t_sd + t_nms), nc.min().item(), nc.max().item(), d.n_det.float().mean().item()), flush=True)
        if os.environ.get('AB_LIB'):
            for a, name in ((1, "k_score_pairs alone"), (2, "+ cut and admission"), (4, "+ decode and sort"), (8, "+ greedy pass")):
                L.ssd_dev_knob(b"SSD_ABLATE", a)
                ta = bench.graph_timed(torch, lambda: ops.detect_pairs(conf, loc, pset, thresh), 30)
                print("      %-22s %.1f us" % (name, ta * 1e6), flush=True)
            L.ssd_dev_knob(b"SSD_ABLATE", 0)
