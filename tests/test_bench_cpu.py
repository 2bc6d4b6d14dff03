"""CPU suite: bench.py's --dump-outputs writer on host tensors of the benchmark's shapes (batch 64, 8732 anchors, 81 classes):
float32 / float64 files under 64 MB, whole arrays below their cap, a fixed seeded sample of the larger ones."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def step_outputs(B, A=8732, classes=81, n_param=1 << 22, seed=0):
    g = torch.Generator().manual_seed(seed)
    conf = torch.randn((B, A, classes), generator=g).bfloat16()
    loc = torch.randn((B, A, 4), generator=g).bfloat16()
    param = torch.randn((n_param,), generator=g)
    targets = (torch.randint(0, 81, (B, A), generator=g, dtype=torch.int32), torch.randn((B, A, 4), generator=g),
               torch.randint(0, 2, (B, A), generator=g, dtype=torch.uint8))
    info = {"loc loss": 0.75, "cls loss pos": 4.4, "cls loss neg": 4.5, "status": 0.0}
    return conf, loc, info, param, targets


def test_dump_outputs_files(tmp_path):
    conf, loc, info, param, targets = step_outputs(64)
    bench.dump_outputs(np, torch, str(tmp_path), conf, loc, info, param, targets)
    files = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(files) == {"loss", "pred_conf", "pred_loc", "params", "target_cls", "target_loc", "target_mask"}
    assert files["loss"].dtype == np.float64 and list(files["loss"]) == [0.75, 4.4, 4.5, 0.0]
    assert all(a.dtype == np.float32 for k, a in files.items() if k != "loss")
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64e6
    # below the cap: the whole array, exactly
    assert np.array_equal(files["pred_loc"], loc.float().numpy())
    assert np.array_equal(files["target_cls"], targets[0].float().numpy())
    assert np.array_equal(files["target_loc"], targets[1].numpy())
    assert np.array_equal(files["target_mask"], targets[2].float().numpy())
    # above it: the values at sorted seeded positions
    for name, t in (("pred_conf", conf), ("params", param)):
        cap = dict(bench.DUMP_CAPS)[name]
        pos = np.unique(np.random.default_rng([n for n, _ in bench.DUMP_CAPS].index(name)).integers(0, t.numel(), cap))
        assert cap // 2 < pos.size <= cap
        assert np.array_equal(files[name], t.reshape(-1)[torch.from_numpy(pos)].float().numpy())


def test_dump_outputs_same_positions_and_cap_at_larger_batch(tmp_path):
    a = bench.dump_outputs(np, torch, str(tmp_path / "a"), *step_outputs(8, seed=1))
    b = bench.dump_outputs(np, torch, str(tmp_path / "b"), *step_outputs(8, seed=1))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    big = bench.dump_outputs(np, torch, str(tmp_path / "c"), *step_outputs(160, classes=2))
    assert big["pred_loc"].ndim == 1 and big["target_loc"].ndim == 1            # above their caps at batch 160
    assert sum(x.nbytes for x in big.values()) <= bench.DUMP_LIMIT_BYTES
