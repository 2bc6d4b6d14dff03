"""The bench line as the driver invokes it: one rank, and two ranks sharing this box's GPU over gloo (the launcher's rehearsal
mode) -- with `--full` and the kernel-timing sections ON, which rank 0 runs alone: its probe steps must not enter a collective
the other ranks never join (a round-4 regression test: the in-step probe of the dominant kernel once did, and `--gpus 2`
hung).  And the plain line: the timed steps and the headline only, `--dump-outputs` the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra, timeout):
    env = dict(os.environ, SSD_BENCH_WATCHDOG=str(timeout - 20))     # a hang dumps every thread's stack instead of timing out silently
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, cwd=ROOT, env=env, capture_output=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


def test_bench_line_one_rank():
    d = run_bench(["--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"], 420)
    assert d["n_gpus"] == 1 and d["unit"] == "images/sec" and d["value"] > 0 and d["dtype"] == "bf16"
    r = d["roofline"]
    assert r["bound"] == "mfma" and 0 < r["frac"] < 1 and r["us_per_step_in_step"] >= r["us_per_step"] * 0.9
    assert d["loss_check"]["status"] == 0.0


def test_bench_line_two_ranks_rehearsal():
    d = run_bench(["--full", "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"], 600)
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 128
    assert "comm" in d and d["comm"]["backend"].startswith("gloo") and "roofline" in d


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run times exactly --steps steps and prints the headline without the --full sections; --dump-outputs writes the
    last timed step's outputs (float32 / float64, under 64 MB), and a second run with the same arguments writes the same
    files bit for bit (same inputs, same sample positions, a deterministic step)."""
    dumps = []
    for k in range(2):
        out = tmp_path / ("run%d" % k)
        d = run_bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(out)], 300)
        assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"] == "bf16"
        assert d["unit"] == "images/sec" and d["higher_is_better"] is True and d["value"] > 0
        assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 64) < 0.1          # value = batch 64 / ms_per_step
        assert not {"roofline", "calibration", "m2", "cfg5_anchors", "cpu_baseline", "config3_train_plus_eval"} & set(d)
        files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
        assert set(files) == {"loss", "pred_conf", "pred_loc", "params", "target_cls", "target_loc", "target_mask"}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64e6
        assert files["pred_loc"].shape == (64, 8732, 4) and files["target_mask"].shape == (64, 8732)
        lc = d["loss_check"]
        assert list(files["loss"]) == [lc["loc loss"], lc["cls loss pos"], lc["cls loss neg"], lc["status"]] and lc["status"] == 0
        dumps.append(files)
    for name, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][name]), name
