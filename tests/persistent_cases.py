"""Shapes at which the streaming row passes of the loss and detection kernels go beyond one sweep of their persistent grid, and
the arithmetic behind them.  Plain Python / numpy / CPU torch: importable without a GPU.

The four row passes (k_loss_rows and its gradient pass, k_mb_rows / k_mb_grad, k_sf_rows, k_score_decode / k_score_pairs) walk
blocks of ROWS anchor rows with `for (blk = blockIdx.x; blk < nblk; blk += gridDim.x)` on a grid of min(nblk, MAX_PERSIST)
workgroups.  Only from a workgroup's second trip onwards does the code issue the in-loop stage_load, reuse the LDS tile after
another block's gradient has left it, write per-block partials at blk >= MAX_PERSIST and reach a ragged last block through the
in-loop prefetch: that begins at B * A > MAX_PERSIST * ROWS = 98 304 rows.  The constants are restated here (the sources are
named beside them) and tests/test_persistent_cases_cpu.py reads them back from the .hip files, so a retune that moves a
threshold fails there instead of hollowing out tests/test_row_passes_persistent_gpu.py."""
import functools
import os

import numpy as np
import torch

from tests import multibox_cases as MK
from tests import softmax_focal_cases as FK

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ssd-object-detection_amd", "csrc")
ROW_PASS_FILES = ("loss.hip", "multibox.hip", "softmax_focal.hip", "detect.hip")

ROWS = 128              # anchor rows per block: `constexpr int ROWS = 128;` in each of ROW_PASS_FILES
MAX_PERSIST = 768       # the persistent grid: `constexpr int MAX_PERSIST = 768;` in loss / multibox / softmax_focal.hip,
#                         the literal in `nblk < 768 ? nblk : 768` of detect.hip's two launches
CNT_CHUNK = 4096        # mask bytes per count chunk: `constexpr int CNT_CHUNK = 4096;` in softmax_focal.hip (k_sf_count)
REDUCE_WG = 256         # sf_total_pos and k_sf_scalars loop `i += WG` with WG == 256 (static_assert in softmax_focal.hip)

SSD300_A = MK.strict.anchors_of(MK.SSD300_GEOM)

# name: (B, A, C).  The smallest shapes at which each path exists, not the workload's own.
S81 = (3, 65717, 81)            # three trips of the specialised (C == 81) instances, a 31-row last block on a third trip
SGEN = (1, 1052677, 3)          # >= ten trips of the runtime-C instance, a 5-row last block, 258 count chunks
SHEADS = (12, SSD300_A, 81)     # SSD300's own geometry: the rows forms need real levels
SCORES_SMALL = (3, 33000, 6)    # ssd_class_scores, runtime C
TILE_SMALL, TILE_K = (3, 300), 128                                        # STILE: 128 copies of (3, 300, C) along the batch axis
STILE = (TILE_K * TILE_SMALL[0], TILE_SMALL[1])


def walk(n):
    """How a row pass covers n rows: dict(nblk, grid, trips (of the busiest workgroup), min_trips, busiest (how many workgroups
    make `trips` trips: they are workgroups 0 .. busiest-1), last_rows, last_wg, last_trip (1-based), chunks)."""
    nblk = (n + ROWS - 1) // ROWS
    grid = min(nblk, MAX_PERSIST)
    trips = (nblk + grid - 1) // grid
    return dict(nblk=nblk, grid=grid, trips=trips, min_trips=nblk // grid, busiest=nblk - (trips - 1) * grid,
                last_rows=n - (nblk - 1) * ROWS, last_wg=(nblk - 1) % grid, last_trip=(nblk - 1) // grid + 1,
                chunks=(n + CNT_CHUNK - 1) // CNT_CHUNK)


def describe(name, shape):
    w = walk(shape[0] * shape[1])
    return "%s %s: %d rows, %d blocks on %d workgroups, %d..%d blocks per workgroup, last block %d rows" % (
        name, tuple(shape), shape[0] * shape[1], w["nblk"], w["grid"], w["min_trips"], w["trips"], w["last_rows"])


def tile_batch(case, k):
    """`case` (a dict of tests/softmax_focal_cases.make_case, tests/multibox_cases.hand_case or loss_case below) repeated k times
    along the batch axis: every array or tensor with a leading batch axis is tiled, B is multiplied."""
    B = case["B"]
    out = dict(case)
    for key, v in case.items():
        if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[0] == B:
            out[key] = np.tile(v, (k,) + (1,) * (v.ndim - 1))
        elif isinstance(v, torch.Tensor) and v.ndim >= 2 and v.shape[0] == B:
            out[key] = v.repeat(k, *([1] * (v.ndim - 1)))
    out["B"] = k * B
    return out


@functools.lru_cache(maxsize=None)
def focal_tiled(C, bf16):
    """(small, tiled): make_case(3, 300, C) and its TILE_K-fold tiling.  P of the tiling is TILE_K * P0."""
    small = FK.make_case(TILE_SMALL[0], TILE_SMALL[1], C, bf16=bf16)
    return small, tile_batch(small, TILE_K)


# --------------------------------------------------------------------------------------------------------- MultiBox
# positives per image of the 12-image hand case: an image without any, one whose 3 P_b exceeds its candidates (as
# tests/test_multibox_gpu.py::test_against_oracle_ssd300 has), the rest spread over three orders of magnitude
MB_P_B = (0, 7, 60, 400, 2500, 30, 1, 900, 128, 15, 250, 3)
MB_SEED = {torch.float32: 70, torch.bfloat16: 74}                        # (bf16 seeds 71..73 put a second key at some tau_b)
MB_TILE_P_B, MB_TILE_SEED = (5, 0, 40), 80
# the exact 12-image rows-form case: P = 512 (a power of two, tests/multibox_cases.exact_case), one image without positives
MB_HEADS_P_B = (128, 64, 64, 64, 32, 32, 32, 32, 32, 16, 16, 0)


def multibox_hand(dtype):
    return MK.cached("persistent hand %s" % dtype, lambda: MK.hand_case(SHEADS[0], SHEADS[1], SHEADS[2], MB_P_B, MB_SEED[dtype], dtype))


def multibox_tiled(C, dtype):
    small = MK.cached("persistent tile %d %s" % (C, dtype),
                      lambda: MK.hand_case(TILE_SMALL[0], TILE_SMALL[1], C, MB_TILE_P_B, MB_TILE_SEED + C, dtype))
    return small, MK.cached("persistent tiled %d %s" % (C, dtype), lambda: tile_batch(small, TILE_K))


def multibox_heads():
    return MK.cached("persistent heads", lambda: MK.heads_case(SHEADS[0], MK.SSD300_GEOM, SHEADS[2], MB_HEADS_P_B, full=(5,),
                                                                empty=(4,), seed=12))


# --------------------------------------------------------------------------------------------------------- the reference loss
LOSS_P = 1048                                                            # about 1 % of 12 * 8732 anchors
# (seeds chosen by the float64 oracle alone: with 10^5 keys about every other seed puts a second key within 1e-5 tau of tau)
LOSS_SEED = {(81, torch.bfloat16): 92, (81, torch.float32): 91, (21, torch.float32): 90}
LOSS_TILE_P, LOSS_TILE_SEED = 40, 95


@functools.lru_cache(maxsize=None)
def loss_case(B, A, C, P, seed, dtype):
    """background-heavy random logits and offsets on the CPU (in `dtype`), targets of tests/test_loss_gpu.hand_targets"""
    from tests.test_loss_gpu import hand_targets
    g = torch.Generator().manual_seed(1000 + seed)
    conf = 3.0 * torch.randn((B, A, C), generator=g)
    conf[..., C - 1] += 2.0
    loc = 0.5 * torch.randn((B, A, 4), generator=g)
    cls, gloc, mask = hand_targets(B, A, C, P, seed, device="cpu")
    return dict(B=B, A=A, C=C, dtype=dtype, conf=conf.to(dtype), loc=loc.to(dtype), gt_cls=cls, gt_loc=gloc, gt_mask=mask)


def loss_full(C, dtype):
    return loss_case(SHEADS[0], SHEADS[1], C, LOSS_P, LOSS_SEED[(C, dtype)], dtype)


def loss_tiled(C, dtype):
    small = loss_case(TILE_SMALL[0], TILE_SMALL[1], C, LOSS_TILE_P, LOSS_TILE_SEED + C, dtype)
    return small, tile_batch(small, TILE_K)


# --------------------------------------------------------------------------------------------------------- threshold margins
def keys_at_tau(key, tau):
    """how many of `key` (float64, candidates only) lie within the tests' flip distance 1e-5 * max(1, tau) of tau.  tau is one of
    them; a second one could flip on the device and count against the caps of run_case / check_against_oracle."""
    return int((np.abs(np.asarray(key, np.float64) - tau) <= 1e-5 * max(1.0, abs(tau))).sum())


def multibox_margins(r):
    """per image with mined negatives: keys_at_tau of the float64 oracle's candidate keys (tests/multibox_oracle.py)"""
    conf = r["conf"].float().numpy()
    mask = r["gt_mask"].numpy().astype(bool)
    key = MK.M.keys(conf)
    tau, _ = MK.M.select(key, mask, 3)
    return [keys_at_tau(key[b][~mask[b]], tau[b]) for b in range(r["B"]) if not np.isnan(tau[b])]


def loss_margin(r):
    """keys_at_tau of the reference loss's batch-wide threshold (oracle/ssd_oracle.ssd_loss: the masked background CE)"""
    from oracle import ssd_oracle as O
    conf = r["conf"].float().numpy()
    pos = r["gt_mask"].numpy().astype(bool)
    ref = O.ssd_loss(r["gt_cls"].numpy(), r["gt_loc"].numpy(), pos, r["loc"].float().numpy(), conf)
    key = -O._log_softmax(conf.astype(np.float64))[..., r["C"] - 1]
    return keys_at_tau(key[~pos], ref["tau"])
