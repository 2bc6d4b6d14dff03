"""CPU: the shapes of tests/persistent_cases.py do what tests/test_row_passes_persistent_gpu.py relies on.  The launch constants
restated there are read back from the four .hip files, every shape's walk over the persistent grid is asserted, the three case
constructors give tensors of the requested shape, and for every seed used against a float64 oracle with a flip cap the oracle
itself has no second key within the flip distance of its threshold."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import multibox_cases as MK                                   # noqa: E402
from tests import persistent_cases as PC                                 # noqa: E402

F32, BF = torch.float32, torch.bfloat16


def source(name):
    with open(os.path.join(PC.CSRC, name)) as f:
        return f.read()


def constant(text, name):
    m = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert len(m) == 1, (name, m)
    return int(m[0])


def test_restated_launch_constants_are_the_sources():
    for name in PC.ROW_PASS_FILES:
        text = source(name)
        assert constant(text, "ROWS") == PC.ROWS, name
        assert len(re.findall(r"for \(size_t blk = blockIdx\.x; blk < nblk; blk \+= gridDim\.x\)", text)) >= 1, name
        if name == "detect.hip":
            grids = re.findall(r"nblk < (\d+) \? nblk : (\d+)", text)
            assert len(grids) == 2 and all(int(a) == int(b) == PC.MAX_PERSIST for a, b in grids), grids
        else:
            assert constant(text, "MAX_PERSIST") == PC.MAX_PERSIST, name
            assert re.search(r"min\(\(size_t\)MAX_PERSIST,", text), name
    focal = source("softmax_focal.hip")
    assert constant(focal, "CNT_CHUNK") == PC.CNT_CHUNK
    assert re.search(r"static_assert\(WG == %d," % PC.REDUCE_WG, focal)
    assert re.search(r"for \(int i = threadIdx\.x; i < nc; i \+= WG\)", focal)                  # sf_total_pos
    assert re.search(r"for \(size_t i = threadIdx\.x; i < p\.nblk; i \+= WG\)", focal)          # k_sf_scalars
    # the specialised instances are the C == 81 ones
    for name in ("loss.hip", "multibox.hip", "softmax_focal.hip"):
        assert re.search(r"C == 81 \?", source(name)), name
    assert PC.MAX_PERSIST * PC.ROWS == 98304


def test_walks_of_the_shapes():
    w = PC.walk(PC.S81[0] * PC.S81[1])
    assert PC.S81[0] * PC.S81[1] == 197151 and PC.S81[2] == 81
    assert (w["nblk"], w["grid"], w["trips"], w["min_trips"], w["busiest"]) == (1541, 768, 3, 2, 5)     # workgroups 0..4: three trips
    assert (w["last_rows"], w["last_wg"], w["last_trip"]) == (31, 4, 3)
    assert w["nblk"] > PC.REDUCE_WG                                      # k_sf_scalars' strided sum makes further trips

    w = PC.walk(PC.SGEN[0] * PC.SGEN[1])
    assert PC.SGEN[2] == 3 and (w["nblk"], w["grid"], w["min_trips"], w["trips"]) == (8225, 768, 10, 11)
    assert (w["last_rows"], w["last_wg"], w["last_trip"]) == (5, 8224 % 768, 11)
    assert w["chunks"] == 258 and w["chunks"] > PC.REDUCE_WG             # sf_total_pos makes a second trip

    assert PC.SSD300_A == 8732
    w = PC.walk(PC.SHEADS[0] * PC.SHEADS[1])
    assert PC.SHEADS[0] * PC.SHEADS[1] == 104784 and PC.SHEADS[2] == 81
    assert (w["nblk"], w["trips"], w["min_trips"], w["busiest"]) == (819, 2, 1, 51)                      # workgroups 0..50: two trips
    assert (w["last_rows"], w["last_wg"], w["last_trip"]) == (80, 50, 2)

    w = PC.walk(PC.STILE[0] * PC.STILE[1])
    assert PC.STILE == (384, 300) and (w["nblk"], w["trips"], w["busiest"], w["last_rows"]) == (900, 2, 132, 128)
    # images straddle the 128-row blocks at every offset a multiple of gcd(300, 128) = 4 allows
    assert {(b * PC.STILE[1]) % PC.ROWS for b in range(PC.STILE[0])} == set(range(0, PC.ROWS, 4))
    # ... and every copy of the small case starts at another place of a block within a period of 32 copies
    assert len({(k * PC.TILE_SMALL[0] * PC.TILE_SMALL[1]) % PC.ROWS for k in range(PC.TILE_K)}) == 32

    w = PC.walk(PC.SCORES_SMALL[0] * PC.SCORES_SMALL[1])
    assert (w["nblk"], w["trips"], w["busiest"], w["last_rows"], w["last_trip"]) == (774, 2, 6, 56, 2)
    for name in ("S81", "SGEN", "SHEADS", "SCORES_SMALL"):
        print(PC.describe(name, getattr(PC, name)))
    print(PC.describe("STILE", PC.STILE))


def test_constructors_give_the_requested_shapes():
    B, A, C = PC.SHEADS
    for dtype in (F32, BF):
        r = PC.multibox_hand(dtype)                                       # multibox_cases.hand_case
        assert r["conf"].shape == (B, A, C) and r["conf"].dtype == dtype and r["loc"].shape == (B, A, 4)
        assert r["gt_cls"].shape == (B, A) and r["gt_loc"].shape == (B, A, 4) and r["gt_mask"].shape == (B, A)
        assert tuple(r["gt_mask"].sum(1).tolist()) == PC.MB_P_B and not r["conf"].is_cuda
    assert 0 in PC.MB_P_B and any(3 * p > A - p for p in PC.MB_P_B)
    for (Cl, dtype) in PC.LOSS_SEED:                                      # test_loss_gpu.hand_targets
        r = PC.loss_full(Cl, dtype)
        assert r["conf"].shape == (B, A, Cl) and r["conf"].dtype == dtype and r["loc"].shape == (B, A, 4)
        assert r["gt_cls"].shape == (B, A) and r["gt_loc"].shape == (B, A, 4) and r["gt_mask"].shape == (B, A)
        assert int(r["gt_mask"].sum()) == PC.LOSS_P and not r["gt_mask"].is_cuda
        assert int(r["gt_cls"].min()) >= 0 and int(r["gt_cls"].max()) <= Cl - 2
    assert 0.009 < PC.LOSS_P / (B * A) < 0.011
    Bt, At = PC.STILE
    for Cl, bf16 in ((81, True), (21, False)):                            # the tiled focal case
        small, big = PC.focal_tiled(Cl, bf16)
        assert big["B"] == Bt and big["conf"].shape == (Bt, At, Cl) and big["loc"].shape == (Bt, At, 4)
        assert big["gt_cls"].shape == (Bt, At) and big["gt_loc"].shape == (Bt, At, 4) and big["gt_mask"].shape == (Bt, At)
        assert int(big["gt_mask"].sum()) == PC.TILE_K * int(small["gt_mask"].sum()) > 0
        for k in (0, 1, PC.TILE_K - 1):
            assert np.array_equal(big["conf"][3 * k:3 * k + 3], small["conf"]) and np.array_equal(big["gt_mask"][3 * k:3 * k + 3], small["gt_mask"])
        # 128 P0 and grad_scale * 128 are exact in float32: grad_scale / P keeps its bits
        P0 = int(small["gt_mask"].sum())
        assert float(np.float32(PC.TILE_K * P0)) == PC.TILE_K * P0
        for gs in (1.0, 0.25):
            assert np.float32(gs * PC.TILE_K) / np.float32(PC.TILE_K * P0) == np.float32(gs) / np.float32(P0)
    for Cl, dtype in ((81, BF), (21, F32)):
        for small, big in (PC.multibox_tiled(Cl, dtype), PC.loss_tiled(Cl, dtype)):
            assert big["conf"].shape == (Bt, At, Cl) and big["conf"].dtype == dtype and big["gt_mask"].shape == (Bt, At)
            assert torch.equal(big["conf"][-3:], small["conf"]) and torch.equal(big["gt_cls"][3:6], small["gt_cls"])
            assert int(big["gt_mask"].sum()) == PC.TILE_K * int(small["gt_mask"].sum())


def test_float64_oracles_have_one_key_at_their_thresholds():
    """The flip caps of test_loss_gpu.run_case (two per call) and test_multibox_gpu.check_against_oracle (two per image, each
    within 1e-5 max(1, tau) of tau) are not raised for the larger batches: for the seeds used, the float64 oracle's own keys
    have tau and nothing else within that distance, so a flip on the device needs an error of the size of the distance."""
    for dtype in (F32, BF):
        m = PC.multibox_margins(PC.multibox_hand(dtype))
        print("multibox", dtype, "keys at tau_b per mined image", m)
        assert len(m) == sum(1 for p in PC.MB_P_B if p) and set(m) == {1}
    for (C, dtype) in PC.LOSS_SEED:
        m = PC.loss_margin(PC.loss_full(C, dtype))
        print("reference loss C", C, dtype, "keys at tau", m)
        assert m == 1
    for C, dtype in ((81, BF), (21, F32)):
        assert set(PC.multibox_margins(PC.multibox_tiled(C, dtype)[0])) == {1}
        assert PC.loss_margin(PC.loss_tiled(C, dtype)[0]) == 1


def test_exact_rows_form_case_is_built_for_twelve_images():
    assert len(PC.MB_HEADS_P_B) == PC.SHEADS[0] and sum(PC.MB_HEADS_P_B) == 512 and 0 in PC.MB_HEADS_P_B
    assert MK.strict.anchors_of(MK.SSD300_GEOM) == PC.SHEADS[1]
