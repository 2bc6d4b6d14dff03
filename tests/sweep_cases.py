"""Shapes at which the capped stream kernels go beyond the first sweep of their grid, the arithmetic behind them, and large cases
built by tiling small exact ones.  Plain Python / CPU torch: importable without a GPU.

Every HBM-bound stream kernel launches a capped grid and walks the rest of its work in a loop `for (i = blockIdx.x ...; i <
total; i += gridDim.x ...)`.  Only an input past one sweep reaches a second trip, where a wrong stride, a tail that is dropped or
written twice, per-thread state carried from trip to trip, a shuffle group split by the loop bound, slab_rows() for a slab of
three chunks, or workspace rows written only on later trips could show.  tests/persistent_cases.py does this for the loss and
detection row passes; this module does it for every other grid-stride loop under csrc/.  The constants are restated here (the
sources are named beside them) and tests/test_sweep_cases_cpu.py reads them back from the .hip files, so a retune that moves a
cap fails there instead of hollowing out the GPU tests.

The audit (caps and loop bodies read from the sources; "items" are what one lane, wave or workgroup takes per trip; G =
tests/test_stream_sweeps_gpu.py):

kernel(s)                        file           cap                          first shape with a second trip        largest before     workload (batch 64 unless said)      covered by
-------------------------------  -------------  ---------------------------  ------------------------------------  -----------------  -----------------------------------  ---------------------------------------------
k_add_relu, k_relu_mask (write   eltwise.hip    grid_for: 8192 wg x 256      n / 8 > 2 097 152                     (3,17,19,256):     ResNet layer1 from batch 5           G::test_add_relu_and_relu_mask_second_trip
  and accumulate)                                                                                                  31 008 vectors
k_add_relu_mxfp8                 eltwise.hip    same                         n / 8 > 2 097 152                     same               same                                 G::test_add_relu_mxfp8_second_trip
k_maxpool3x3s2_fwd / _bwd        eltwise.hip    same                         B Ho Wo C / 8, B H W C / 8            (2,37,50,64)       stem pool from batch 17              G::test_maxpool3x3s2_second_trip (bwd: four)
                                                                               > 2 097 152
k_maxpool_mxfp8<2>, <3>          poolq.hip      same                         nout / 8 > 2 097 152                  (2,19,19,64)       pool1 from batch 12                  G::test_maxpool_mxfp8_second_trip[2], [3]
k_maxpool3x3s1_fwd / _bwd        atrous.hip     same                         B H W C / 8 > 2 097 152               (2,19,19,64)       pool5 only from batch 91             G::test_maxpool3x3s1_second_trip
k_bn_apply<true/false>,          batchnorm.hip  kApplyBlocks = 2048 chunks   P > 2048 (2048 / C)                   1032 chunks,       stem BN: 64 trips                    test_batchnorm_gpu.py::test_forward_train,
  k_bn_bwd_dx                                     of 2048 / C rows                                                 (33000,64)                                                test_forward_infer, test_backward_on_what_
                                                                                                                                                                            the_forward_saved at BN_SHAPES
k_bn_stats, k_bn_bwd_sums        batchnorm.hip  kMaxSlabs = 1024             a slab's third chunk: P > 65 536      two chunks, on 8   as above                             the same tests: (65703,64) three chunks on
                                                                               at C = 64                           slabs only                                                slabs 0..5, (2085,2048) 31 or 32 per slab
k_l2norm_fwd<1/2>                l2norm.hip     kFwdBlocks 4 = 8192 pixels   P > 8192                              P = 2888           12 trips                             test_l2norm_gpu.py::test_forward at L2_SHAPES
k_l2norm_bwd<1/2>                l2norm.hip     kBwdBlocks 4 = 6144 pixels   P > 6144                              P = 2888           16 trips                             test_l2norm_gpu.py::test_backward at L2_SHAPES
k_quant_mx_fp8                   fp8conv.hip    16384 wg x 256 blocks        n > 134 217 728                       65 280 blocks      268 435 456: the gradient maps of    G::test_quantize_mx_fp8_second_trip
                                                                                                                                      ResNet nodes 6 and 10 (128x128x256)
                                                                                                                                      in the fp8 backward: exactly two
                                                                                                                                      sweeps (QUANT_CALLS below)
k_chain_pack                     chain.hip      256 wg x 256 pieces of 16 B  N K / 8 > 65 536                      36 864 pieces      36 864 pieces (a 3x3 128 -> 256      none needed: the largest filter of every
                                                                                                                                      extras layer), whatever the batch    trunk's chain is 0.5625 of one sweep
k_hz_gemm                        sparse.hip     2048 tiles of 128 x 128      sum ceil(rows_l / 128) 9 Cin_l / 128  162 tiles ("B=4    level 0 alone: 36 column tiles, so   G::test_sparse_data_gradient_second_trip
                                                                               > 2048                              splits")           from 7 169 compact rows
k_conv0_fwd                      conv.hip       768 wg, one 16 x 16 block    B ceil(H/16) ceil(W/16) > 768         1444 blocks        23 104 blocks                        test_conv_gpu.py::test_first_layer_kernels_
  (the `t += gridDim.x` loop;                     each                                                                                                                     full_size (4 x 19 x 19 blocks: two trips)
  k_conv3x3_p512 has none: it
  returns at pblock >= nblocks)
k_loss_hist<2/3>                 loss.hip       256 wg x 256 keys            B A > 65 536                          104 784            558 848                              test_row_passes_persistent_gpu.py::
                                                                                                                                                                            test_reference_loss_second_trip
k_loss_grad_rows' zeroing of     loss.hip       none: one workgroup per      fewer blocks of rows than             --                 one trip (4366 workgroups)           every rows-form loss test of a few blocks of
  the histograms                                  block of rows x 256 words    hist_words / 256                                                                              rows (tests/test_loss_strict_gpu.py) makes
                                                                                                                                                                            several; the next call reads the zeros
k_loss_rows .. k_score_pairs     loss.hip, multibox.hip, softmax_focal.hip, detect.hip: tests/persistent_cases.py and tests/test_row_passes_persistent_gpu.py
k_jpeg_idct                      jpeg.hip       64 wg x 256 8x8 blocks       more than 16 384 blocks per image     264 blocks         7 200 (VGA 4:2:0): one trip, any     test_jpeg_gpu.py::test_reconstruct_past_one_
                                                                                                                                      batch (blockIdx.y is the image)      stride_of_the_loops[444]: 16 632 blocks
k_jpeg_rgb                       jpeg.hip       128 wg x 256 pixels          more than 32 768 pixels per image     5 063 pixels       307 200 (VGA): ten trips             the same test: [444] eleven trips, [420] three

The two JPEG loops stride by a constant (IDCT_GRID_X, RGB_GRID_X) that is also their launch's grid.  Their large images are
no new files: tests/jpeg_cases.tiled repeats a fixture's grid of coefficient blocks, and the expectation is the numpy oracle's
reconstruction of those coefficients.  The persistent kernels that walk a block list without a `+= gridDim.x` loop
(k_conv3x3_c64b's block_of(), k_pw_gemm's tile queue) are not grid-stride loops in this sense and are not part of this table.

Large cases are built by tiling, never by running a reference over 10^8 elements: a small case of the project's own
constructors is repeated along the batch (or flat) axis and copy b is multiplied by 2^(b mod 4).  Max, ReLU, masking,
un-pooling and addition commute with a positive power of two and winner codes do not change, so the expected output is the
small reference tiled and scaled the same way; quantisation is block-wise, so the bytes tile and the scale byte of a non-zero
block moves by the copy's exponent (the fused MX outputs take strict.ref_quantize_mx of the tiled bf16 map instead: 1.7 10^7
elements).  One sweep is no multiple of any small case's size, so an element and the one a sweep earlier come from different
places of different copies: tests/test_sweep_cases_cpu.py asserts that at least half of the non-zero second-trip reference
elements differ from the element one sweep earlier -- a kernel that re-read the first sweep could not pass."""
import os

import torch

from tests import atrous_oracle
from tests import pool_mxfp8_cases as PQ
from tests import strict

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ssd-object-detection_amd", "csrc")
BF, U8, I32 = torch.bfloat16, torch.uint8, torch.int32

# ---- the launch constants, restated (tests/test_sweep_cases_cpu.py reads them back) ---------------------------------------------
GRID_FOR_FILES = ("eltwise.hip", "poolq.hip", "atrous.hip")
WG = 256                    # lanes per workgroup: the literal 256 of the loop headers and launches of GRID_FOR_FILES
VEC = 8                     # bf16 elements per item: one 16-byte vector per lane
GRID_FOR_CAP = 8192         # `g > 8192 ? 8192 : g` in grid_for() of each of GRID_FOR_FILES
SWEEP_ITEMS = GRID_FOR_CAP * WG
BN_THREADS, BN_MAX_SLABS, BN_SLAB_ROWS, BN_APPLY_BLOCKS = 256, 1024, 32, 2048      # kThreads, kMaxSlabs, kSlabRows, kApplyBlocks: batchnorm.hip
L2_THREADS, L2_WAVE, L2_FWD_BLOCKS, L2_BWD_BLOCKS = 256, 64, 2048, 1536            # kThreads, SSD_WAVE (common.h), kFwdBlocks, kBwdBlocks: l2norm.hip
L2_WAVES = L2_THREADS // L2_WAVE                                                   # kWaves: one pixel per wave and trip
QUANT_CAP, QUANT_BLOCK = 16384, 32                                                 # `gridl > 16384 ? 16384 : gridl` of ssd_quantize_mx_fp8, fp8conv.hip
QUANT_SWEEP = QUANT_CAP * WG                                                       # blocks of 32 elements
CHAIN_PACK_CAP = 256                                                               # `< 256 ? ... : 256` of ssd_chain_pack_weights, chain.hip
HZ_CAP, HZ_TILE = 2048, 128                                                        # `min(cap_tiles, 2048)`, ZT: sparse.hip
CONV0_CAP, CONV0_BLOCK = 768, 16                                                   # `p->nblocks < 768 ? p->nblocks : 768`, 16 x 16 blocks: conv.hip
LOSS_HIST_CAP = 256                                                                # `min((size_t)256, (n + WG - 1) / WG)`: loss.hip

# ---- the shapes -------------------------------------------------------------------------------------------------------------------
TAIL_WGS = 37               # full workgroups on the second trip of the flat cases, then a partial one
ELT_NVEC = SWEEP_ITEMS + WG * TAIL_WGS + 5           # k_add_relu, k_relu_mask: a 5-lane tail
MX_NVEC = SWEEP_ITEMS + WG * TAIL_WGS + 4            # k_add_relu_mxfp8: n % 32 == 0, the last shuffle group is the only live one of its wave
ELT_BASE = (3, 17, 19, 64)                           # strict.eltwise_case / strict.mx_eltwise_case: 62 016 elements = 1938 blocks
POOL3S2_BASE, POOL3S2_COPIES = (1, 37, 50, 16), 2209  # fwd 2 098 550 items, bwd 8 173 300: four trips
POOL3S1_BASE, POOL3S1_COPIES = (1, 19, 19, 64), 727   # 2 099 576 items
POOLQ_BASE = (1, 19, 19, 64)                          # pool_mxfp8_cases.case, SAME
POOLQ_COPIES = {3: 727, 2: 2622}                      # <3>: 2 099 576 items; <2>: 19 x 19 -> 10 x 10, 2 097 600 items
QUANT_NBLK = QUANT_SWEEP + WG * TAIL_WGS + 5         # ssd_quantize_mx_fp8: 4 203 781 blocks, a 5-lane tail
# batchnorm_oracle.EXTRA_SHAPES / l2norm_oracle.EXTRA_SHAPES hold these (asserted in tests/test_sweep_cases_cpu.py)
BN_SHAPES = [(65703, 64), (2085, 2048)]
L2_SHAPES = [(16397, 128), (16397, 1024)]
# k_hz_gemm: B, ReLU mask, levels (H, W, Cin, per_cell, classes, npad, rows) as strict.SPARSE_CASES.  Level 0: 29 row tiles (the
# last of 26 rows) x 72 column tiles = 2088 tiles; level 1: 1 x 18.  2106 tiles on 2048 workgroups: the second trip holds 40
# tiles of level 0's ragged last row tile and the whole of level 1
SPARSE_SWEEP = (10, "bits", [(19, 19, 1024, 4, 5, 40, 3610), (3, 3, 256, 4, 5, 40, 7)])
# the largest stand-alone ssd_quantize_mx_fp8 calls the engines make at batch 64, in elements (asserted against the engines' own
# plans in tests/test_sweep_cases_cpu.py): the fp8 backward of the ResNet-50 SSD512 quantises the gradient maps a bf16 kernel
# wrote last -- nodes 6 and 10, 128 x 128 x 256 each; the VGG trunks' inference forward quantises block2's pooled map
QUANT_CALLS = {"resnet50 ssd512 backward": 64 * 128 * 128 * 256, "ssd512 forward": 64 * 128 * 128 * 128, "ssd300 forward": 64 * 75 * 75 * 128}
CHAIN_PACK_LARGEST = 256 * 9 * 128 // 8              # 16-byte pieces of a 3x3 128 -> 256 extras layer (strict.EXTRA_LAYERS)
FIRST_LAYER_BLOCKS = 4 * 19 * 19                     # conv_cases.FIRST_LAYER_CASE


# ---- walks ---------------------------------------------------------------------------------------------------------------------------
def walk(items, cap=GRID_FOR_CAP, per_wg=WG):
    """How `for (i = blockIdx.x * per_wg + lane; i < items; i += gridDim.x * per_wg)` on min(ceil(items / per_wg), cap)
    workgroups covers `items`: dict(units (workgroup-sized pieces), grid, sweep (items per trip of the grid), trips (of the busiest
    workgroup), min_trips (of the idlest), busiest (how many workgroups make `trips` trips: workgroups 0 .. busiest-1),
    last_size (items of the last piece), last_wg, last_trip (1-based): which workgroup reaches the last piece, and when).
    per_wg = 1: one item per workgroup and trip (`for (t = blockIdx.x; t < items; t += gridDim.x)`)."""
    units = -(-items // per_wg)
    grid = max(1, min(units, cap))
    trips = -(-units // grid)
    return dict(items=items, units=units, grid=grid, sweep=grid * per_wg, trips=trips, min_trips=units // grid,
                busiest=units - (trips - 1) * grid, last_size=items - (units - 1) * per_wg, last_wg=(units - 1) % grid,
                last_trip=(units - 1) // grid + 1)


def walk_bn(P, C):
    """batchnorm.hip's layout(P, C) and its two loops over chunks of rpp rows: dict(rpp, chunks, slabs, last_rows, stats = walk
    of k_bn_stats / k_bn_bwd_sums on `slabs` workgroups, apply = walk of k_bn_apply / k_bn_bwd_dx on min(chunks, kApplyBlocks))"""
    rpp = BN_THREADS // (C // 8)
    chunks = -(-P // rpp)
    slabs = min(-(-P // max(rpp, BN_SLAB_ROWS)), BN_MAX_SLABS)
    return dict(rpp=rpp, chunks=chunks, slabs=slabs, last_rows=P - (chunks - 1) * rpp, stats=walk(chunks, slabs, 1),
                apply=walk(chunks, BN_APPLY_BLOCKS, 1))


def walk_l2(P):
    """l2norm.hip: one pixel per wave and trip, kWaves waves per workgroup.  dict(fwd, bwd): walks in pixels; `busiest` waves make
    the last trip"""
    return dict(fwd=walk(P, L2_FWD_BLOCKS * L2_WAVES, 1), bwd=walk(P, L2_BWD_BLOCKS * L2_WAVES, 1),
                fwd_grid=min(-(-P // L2_WAVES), L2_FWD_BLOCKS), bwd_grid=min(-(-P // L2_WAVES), L2_BWD_BLOCKS))


def walk_hz(B, levels):
    """sparse.hip's k_hz_gemm: tiles of the compact rows (the loop's bound) and of all pixels (the launch's cap_tiles)"""
    tiles = sum(-(-rows // HZ_TILE) * (9 * Cin // HZ_TILE) for _, _, Cin, _, _, _, rows in levels)
    cap_tiles = sum(-(-(B * H * W) // HZ_TILE) * (9 * Cin // HZ_TILE) for H, W, Cin, _, _, _, _ in levels)
    return dict(walk(tiles, min(cap_tiles, HZ_CAP), 1), cap_tiles=cap_tiles)


def describe(name, w):
    return "%s: %d items in %d pieces on %d workgroups, %d..%d trips, last piece of %d on workgroup %d's trip %d" % (
        name, w["items"], w["units"], w["grid"], w["min_trips"], w["trips"], w["last_size"], w["last_wg"], w["last_trip"])


# ---- tiling ---------------------------------------------------------------------------------------------------------------------------
def copy_exponents(k):
    return torch.arange(k) % 4


def bf16_exact(t):
    out = t.to(BF)
    assert torch.equal(out.float(), t.float())
    return out


def tile_scaled(t, k):
    """t [B0, ...] (values exact in bf16) -> bf16 [k B0, ...]: copy b is t times 2^(b mod 4), exactly"""
    t = bf16_exact(t)
    s = torch.exp2(copy_exponents(k).float()).to(BF).view(k, *([1] * t.dim()))
    return (t.unsqueeze(0) * s).reshape(k * t.shape[0], *t.shape[1:])


def tile_plain(t, k):
    return t.repeat(k, *([1] * (t.dim() - 1)))


def tile_flat(t, n):
    """the elements of t, flat, repeated to n elements (the last copy cut short) and scaled per copy as tile_scaled"""
    m = t.numel()
    return tile_scaled(t.reshape(1, m), -(-n // m)).reshape(-1)[:n].contiguous()


_LAST = [None, None]


def _one(name, fn):
    """the case `name`, built by fn(); only the most recent case is kept (each is 0.1 .. 0.4 GB; treat as read-only)"""
    if _LAST[0] != name:
        _LAST[0], _LAST[1] = None, None
        _LAST[1] = fn()
        _LAST[0] = name
    return _LAST[1]


def eltwise_tiled():
    """strict.eltwise_case(ELT_BASE) flat, tiled to ELT_NVEC vectors: a, b, out = relu(a + b), g, base, masked = g where out > 0,
    acc = base + masked.  `sweeps`: reference name -> elements per sweep of the grid"""
    def build():
        r = strict.eltwise_case(ELT_BASE)
        strict.check_regime(r)
        n = ELT_NVEC * VEC
        t = {k: tile_flat(r[k], n) for k in ("a", "b", "out", "g", "base", "masked", "acc")}
        t.update(n=n, bf16=r["bf16"], sweeps={k: SWEEP_ITEMS * VEC for k in ("out", "masked", "acc")}, small=r)
        strict.check_regime(t)
        return t
    return _one("eltwise", build)


def mx_eltwise_tiled():
    """strict.mx_eltwise_case(ELT_BASE) as rows of one 32-element block, tiled to MX_NVEC vectors: a, b, out [n / 32, 32] and
    (q, s) = strict.ref_quantize_mx(out)"""
    def build():
        r = strict.mx_eltwise_case(ELT_BASE)
        n = MX_NVEC * VEC
        assert n % 32 == 0 and r["out"].numel() % 32 == 0               # copies are whole blocks
        t = {k: tile_flat(r[k], n).view(n // 32, 32) for k in ("a", "b", "out")}
        t["q"], t["s"] = strict.ref_quantize_mx(t["out"])
        t.update(n=n, bf16=("out",), small=r,
                 sweeps=dict(out=SWEEP_ITEMS * VEC, q=SWEEP_ITEMS * VEC, s=SWEEP_ITEMS * VEC // 32))
        strict.check_regime(t)
        return t
    return _one("mx eltwise", build)


def _pool_tiled(r, k, geom):
    strict.check_regime(r)
    t = dict(x=tile_scaled(r["x"], k), y=tile_scaled(r["y"], k), dy=tile_scaled(r["dy"], k), dx=tile_scaled(r["dx"], k),
             code=tile_plain(strict.pack_codes(r["code"]), k), bf16=r["bf16"], small=r, copies=k, geom=geom)
    t["sweeps"] = dict(y=SWEEP_ITEMS * VEC, code=SWEEP_ITEMS, dx=SWEEP_ITEMS * VEC)
    strict.check_regime(t)
    return t


def pool3x3s2_tiled():
    """strict.pool3x3_case(POOL3S2_BASE) x POOL3S2_COPIES images: x, y, code (packed int32), dy, dx"""
    def build():
        r = strict.pool3x3_case(*POOL3S2_BASE)
        return _pool_tiled(r, POOL3S2_COPIES, r["geom"])
    return _one("pool3x3s2", build)


def pool3x3s1_tiled():
    """atrous_oracle.pool3x3s1_case(POOL3S1_BASE) x POOL3S1_COPIES images"""
    return _one("pool3x3s1", lambda: _pool_tiled(atrous_oracle.pool3x3s1_case(*POOL3S1_BASE), POOL3S1_COPIES, None))


def poolq_tiled(ksize):
    """pool_mxfp8_cases.case(POOLQ_BASE, ksize, SAME) x POOLQ_COPIES[ksize] images: x, y and (q, s) = ref_quantize_mx(y)"""
    def build():
        r = PQ.case(POOLQ_BASE, ksize, True)
        k = POOLQ_COPIES[ksize]
        t = dict(x=tile_scaled(r["x"], k), y=tile_scaled(r["y"], k), bf16=("y",), small=r, copies=k)
        t["q"], t["s"] = strict.ref_quantize_mx(t["y"])
        t["sweeps"] = dict(y=SWEEP_ITEMS * VEC, q=SWEEP_ITEMS * VEC, s=SWEEP_ITEMS * VEC // 32)
        strict.check_regime(t)
        return t
    return _one("poolq %d" % ksize, build)


def quantize_tiled():
    """The bf16 map `out` of strict.mx_eltwise_case(ELT_BASE) as blocks [1938, 32], every 97th of them zeroed, tiled to QUANT_NBLK
    blocks: x, and the expectation by tiling alone -- q is the small case's bytes in every copy, the scale byte of a non-zero block is the small
    case's plus the copy's exponent, an all-zero block keeps 127"""
    def build():
        small = strict.mx_eltwise_case(ELT_BASE)["out"].to(BF).reshape(-1, 32).clone()
        small[::97] = 0                                                 # all-zero blocks: their scale byte does not move
        q0, s0 = strict.ref_quantize_mx(small)
        m = small.shape[0]
        k = -(-QUANT_NBLK // m)
        x = tile_scaled(small.unsqueeze(0), k).reshape(-1, 32)[:QUANT_NBLK].contiguous()
        q = q0.repeat(k, 1)[:QUANT_NBLK].contiguous()
        live = (small.float().abs().amax(-1, keepdim=True) > 0).to(torch.int32)            # [m, 1]
        assert bool(torch.isfinite(small.float()).all()) and 0 < int(live.sum()) < m      # zero blocks and live ones
        s = (s0.to(torch.int32).unsqueeze(0) + copy_exponents(k).to(torch.int32).view(k, 1, 1) * live.unsqueeze(0))
        assert int(s.min()) > 0 and int(s.max()) < 255
        s = s.to(U8).reshape(-1, 1)[:QUANT_NBLK].contiguous()
        return dict(x=x, q=q, s=s, small=small, copies=k, sweeps=dict(q=QUANT_SWEEP * QUANT_BLOCK, s=QUANT_SWEEP))
    return _one("quantize", build)


def sparse_sweep_case():
    """SPARSE_SWEEP through the constructors of strict.sparse_case (hand_rows, sparse_level)"""
    def build():
        B, relu, levels = SPARSE_SWEEP
        g = strict._gen(B, len(levels), len(relu), 2048)
        out = []
        for H, W, Cin, n, C, npad, count in levels:
            hg = strict.hand_rows(g, B, H, W, n, C, npad, count)
            lv = strict.sparse_level(g, B, H, W, Cin, n * (4 + C), npad, hg["dense"], relu)
            lv.update(hw=H * W, n=n, **{k: hg[k] for k in ("rows", "pixel_of_row", "row_of_pixel", "count")})
            out.append(lv)
        return dict(B=B, relu=relu, levels=out)
    return _one("sparse", build)


# ---- what the references alone must show ------------------------------------------------------------------------------------------
def differs_across_sweep(ref, sweep):
    """(fraction, count): among the elements of `ref` (flat) past the first `sweep` whose value is non-zero, the fraction that
    differs from the element exactly one sweep earlier, and how many such elements there are"""
    flat = ref.reshape(-1)
    later, earlier = flat[sweep:], flat[:flat.numel() - sweep]
    nz = later != 0
    count = int(nz.sum())
    return (float((later[nz] != earlier[nz]).float().mean()) if count else 0.0), count
