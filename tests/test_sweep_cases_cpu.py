"""CPU: the shapes of tests/sweep_cases.py do what tests/test_stream_sweeps_gpu.py and the extended batch-norm and L2Norm
parametrisations rely on.  The launch constants restated there are read back from the .hip files with their loop headers, every
shape's walk over its capped grid is asserted, every tiled reference is the operation of its tiled inputs and by itself tells a
second trip from a repeated first one, the audit's arithmetic for the loops without a new case is asserted, and the fp32
emulations of the batch-norm and L2Norm oracles stay inside those modules' own bounds at the new shapes."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import batchnorm_oracle as BO                                 # noqa: E402
from tests import conv_cases                                             # noqa: E402
from tests import l2norm_oracle as LO                                    # noqa: E402
from tests import persistent_cases as PC                                 # noqa: E402
from tests import strict                                                 # noqa: E402
from tests import sweep_cases as SC                                      # noqa: E402

BF = torch.bfloat16


def source(name):
    with open(os.path.join(SC.CSRC, name)) as f:
        return f.read()


def constant(text, name):
    m = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert len(m) == 1, (name, m)
    return int(m[0])


STREAM_LOOP = r"for \(long long (?:i|idx) = \(long long\)blockIdx\.x \* 256 \+ threadIdx\.x; (?:i|idx) < (?:nvec|total|nblocks); (?:i|idx) \+= \(long long\)gridDim\.x \* 256\)"


def test_restated_launch_constants_are_the_sources():
    loops = {"eltwise.hip": 5, "poolq.hip": 1, "atrous.hip": 2}
    for name in SC.GRID_FOR_FILES:
        text = source(name)
        body = re.findall(r"inline unsigned grid_for\(long long items\) \{\s*const long long g = \(items \+ (\d+)\) / (\d+);\s*"
                          r"return \(unsigned\)\(g < 1 \? 1 : \(g > (\d+) \? (\d+) : g\)\);", text)
        assert body == [(str(SC.WG - 1), str(SC.WG), str(SC.GRID_FOR_CAP), str(SC.GRID_FOR_CAP))], (name, body)
        assert len(re.findall(STREAM_LOOP, text)) == loops[name], name
        assert len(re.findall(r"dim3\(grid_for\([^;]*\)\), dim3\(256\)", text)) >= loops[name], name
    assert SC.SWEEP_ITEMS == 2097152

    bn = source("batchnorm.hip")
    for name, value in (("kThreads", SC.BN_THREADS), ("kMaxSlabs", SC.BN_MAX_SLABS), ("kSlabRows", SC.BN_SLAB_ROWS),
                        ("kApplyBlocks", SC.BN_APPLY_BLOCKS)):
        assert constant(bn, name) == value, name
    assert len(re.findall(r"for \(long long t = blockIdx\.x; t < chunks; t \+= gridDim\.x\)", bn)) == 4       # stats, apply, sums, dx
    assert re.search(r"l\.rpp = kThreads / l\.c8;", bn) and re.search(r"const int per = l\.rpp > kSlabRows \? l\.rpp : kSlabRows;", bn)
    assert re.search(r"l\.slabs = \(int\)\(s < kMaxSlabs \? s : kMaxSlabs\);", bn)
    assert re.search(r"return \(int\)\(l\.chunks < kApplyBlocks \? l\.chunks : kApplyBlocks\);", bn)
    assert len(re.findall(r"<<<l\.slabs, kThreads, 0, s>>>", bn)) == 2 and len(re.findall(r"<<<apply_blocks\(l\), kThreads,", bn)) == 3

    l2 = source("l2norm.hip")
    for name, value in (("kThreads", SC.L2_THREADS), ("kFwdBlocks", SC.L2_FWD_BLOCKS), ("kBwdBlocks", SC.L2_BWD_BLOCKS)):
        assert constant(l2, name) == value, name
    assert re.search(r"constexpr int kWaves = kThreads / SSD_WAVE;", l2)
    assert re.search(r"#define\s+SSD_WAVE\s+%d\b" % SC.L2_WAVE, source("common.h")) or \
        re.search(r"SSD_WAVE\s*=\s*%d\b" % SC.L2_WAVE, source("common.h"))
    assert len(re.findall(r"for \(long long p = \(long long\)blockIdx\.x \* kWaves \+ (?:wave|\(threadIdx\.x >> 6\)); p < P; p \+= waves\)", l2)) == 2
    assert len(re.findall(r"const long long waves = \(long long\)gridDim\.x \* kWaves;", l2)) == 2
    assert re.search(r"const int grid = \(int\)\(b < kFwdBlocks \? b : kFwdBlocks\);", l2)
    assert re.search(r"return \(int\)\(b < kBwdBlocks \? b : kBwdBlocks\);", l2)
    assert SC.L2_WAVES == 4

    fp8 = source("fp8conv.hip")
    assert len(re.findall(STREAM_LOOP, fp8)) == 1
    assert re.search(r"dim3\(\(unsigned\)\(gridl > %d \? %d : gridl\)\), dim3\(256\)" % (SC.QUANT_CAP, SC.QUANT_CAP), fp8)
    assert re.search(r"const long long nb = n / %d;" % SC.QUANT_BLOCK, fp8) and SC.QUANT_SWEEP * SC.QUANT_BLOCK == 134217728

    chain = source("chain.hip")
    assert len(re.findall(STREAM_LOOP, chain)) == 1
    assert re.search(r"\(most \+ 255\) / 256 < %d \? \(most \+ 255\) / 256 : %d\);" % (SC.CHAIN_PACK_CAP, SC.CHAIN_PACK_CAP), chain)

    sparse = source("sparse.hip")
    assert constant(sparse, "ZT") == SC.HZ_TILE
    assert re.search(r"for \(int t = blockIdx\.x; t < total; t \+= gridDim\.x\)", sparse)
    assert re.search(r"k_hz_gemm, dim3\(min\(cap_tiles, %d\)\)" % SC.HZ_CAP, sparse)
    assert re.search(r"t = \(\(a\.count\[l\] \+ ZT - 1\) / ZT\) \* \(a\.lv\[l\]\.N / ZT\);", sparse)
    assert re.search(r"cap_tiles \+= \(\(B \* hw \+ ZT - 1\) / ZT\) \* \(N / ZT\);", sparse)

    conv = source("conv.hip")
    assert len(re.findall(r"for \(int t = blockIdx\.x; t < nblocks; t \+= gridDim\.x, \+\+it\)", conv)) == 1
    head = conv[:conv.index("for (int t = blockIdx.x; t < nblocks; t += gridDim.x, ++it)")]
    assert head.rindex("void k_conv0_fwd(") > head.rindex("void k_conv3x3_p512(")         # the loop is the image layer's
    assert re.search(r"p->wgs = p->nblocks < %d \? p->nblocks : %d;" % (SC.CONV0_CAP, SC.CONV0_CAP), conv)

    loss = source("loss.hip")
    assert re.search(r"const unsigned hgrid = \(unsigned\)min\(\(size_t\)%d, \(n \+ WG - 1\) / WG\);" % SC.LOSS_HIST_CAP, loss)
    jpeg = source("jpeg.hip")
    assert constant(jpeg, "IDCT_GRID_X") == 64 and constant(jpeg, "RGB_GRID_X") == 128


def test_every_grid_stride_loop_is_in_the_audit():
    """a new `+= gridDim.x` loop under csrc/ must get its row (and its second trip) too"""
    audited = {"eltwise.hip": 5, "poolq.hip": 1, "atrous.hip": 2, "batchnorm.hip": 4, "l2norm.hip": 0, "fp8conv.hip": 1, "chain.hip": 1,
               "sparse.hip": 1, "conv.hip": 1, "loss.hip": 3, "multibox.hip": 1, "softmax_focal.hip": 1, "detect.hip": 2}
    found = {}
    for name in sorted(os.listdir(SC.CSRC)):
        if name.endswith((".hip", ".h")):
            n = len(re.findall(r"for \([^;]*;[^;]*;[^)]*\+= (?:\([a-z_ ]+\))?gridDim\.x", source(name)))
            if n:
                found[name] = n
    # l2norm.hip strides by `waves` = gridDim.x * kWaves and jpeg.hip by its grid constants: counted by their own patterns above
    assert found == {k: v for k, v in audited.items() if v}, found
    doc = SC.__doc__
    for kernel in ("k_add_relu", "k_relu_mask", "k_add_relu_mxfp8", "k_maxpool3x3s2_fwd", "k_maxpool_mxfp8", "k_maxpool3x3s1_fwd",
                   "k_bn_apply", "k_bn_bwd_dx", "k_bn_stats", "k_bn_bwd_sums", "k_l2norm_fwd", "k_l2norm_bwd", "k_quant_mx_fp8",
                   "k_chain_pack", "k_hz_gemm", "k_conv0_fwd", "k_loss_hist", "k_loss_grad_rows", "k_jpeg_idct", "k_jpeg_rgb"):
        assert kernel in doc, kernel


def test_walks_of_the_flat_and_pooling_shapes():
    w = SC.walk(SC.ELT_NVEC)
    assert SC.ELT_NVEC == 2097152 + 256 * 37 + 5 and (w["grid"], w["trips"], w["min_trips"], w["busiest"]) == (8192, 2, 1, 38)
    assert (w["last_size"], w["last_wg"], w["last_trip"]) == (5, 37, 2)                 # 37 full workgroups, then five lanes
    w = SC.walk(SC.MX_NVEC)
    assert (w["trips"], w["busiest"], w["last_size"], w["last_wg"], w["last_trip"]) == (2, 38, 4, 37, 2)
    assert (SC.MX_NVEC * SC.VEC) % 32 == 0 and SC.MX_NVEC % 64 == 4                     # one shuffle group alone in the last wave

    B, H, W, C = SC.POOL3S2_BASE
    Ho, Wo, _, _ = strict.geometry(H, W, 3, 2, "same")
    k = SC.POOL3S2_COPIES
    fwd, bwd = SC.walk(k * Ho * Wo * C // 8), SC.walk(k * H * W * C // 8)
    assert (Ho, Wo) == (19, 25) and fwd["items"] == 2098550 and bwd["items"] == 8173300
    assert (fwd["trips"], fwd["last_trip"], fwd["busiest"], fwd["last_size"]) == (2, 2, 6, 118)
    assert (bwd["trips"], bwd["min_trips"], bwd["last_trip"], bwd["last_size"]) == (4, 3, 4, 244)
    assert SC.walk((k - 2) * Ho * Wo * C // 8)["trips"] == 1                            # (one image fewer leaves a second trip of 448 items)

    B, H, W, C = SC.POOL3S1_BASE
    w = SC.walk(SC.POOL3S1_COPIES * H * W * C // 8)
    assert w["items"] == 2099576 and (w["trips"], w["last_trip"], w["busiest"], w["last_size"]) == (2, 2, 10, 120)
    assert SC.walk((SC.POOL3S1_COPIES - 1) * H * W * C // 8)["trips"] == 1

    B, H, W, C = SC.POOLQ_BASE
    w3 = SC.walk(SC.POOLQ_COPIES[3] * H * W * C // 8)
    w2 = SC.walk(SC.POOLQ_COPIES[2] * ((H + 1) // 2) * ((W + 1) // 2) * C // 8)
    assert w3["items"] == 2099576 and w2["items"] == 2097600
    for w, copies, per in ((w3, SC.POOLQ_COPIES[3], H * W * C // 8), (w2, SC.POOLQ_COPIES[2], 100 * C // 8)):
        assert (w["trips"], w["last_trip"]) == (2, 2) and w["items"] % 4 == 0 and SC.walk((copies - 1) * per)["trips"] == 1
    assert w2["last_size"] == 192 and w2["busiest"] == 2

    w = SC.walk(SC.QUANT_NBLK, SC.QUANT_CAP)
    assert (w["grid"], w["sweep"], w["trips"], w["busiest"], w["last_size"], w["last_wg"], w["last_trip"]) == (16384, 4194304, 2, 38, 5, 37, 2)
    for name, w in (("add_relu", SC.walk(SC.ELT_NVEC)), ("maxpool3x3s2 fwd", fwd), ("maxpool3x3s2 bwd", bwd), ("maxpool_mxfp8<2>", w2)):
        print(SC.describe(name, w))


def test_walks_of_the_batchnorm_and_l2norm_shapes():
    assert SC.BN_SHAPES == BO.EXTRA_SHAPES[-2:] and SC.L2_SHAPES == LO.EXTRA_SHAPES
    w = SC.walk_bn(65703, 64)
    assert (w["rpp"], w["chunks"], w["slabs"], w["last_rows"]) == (32, 2054, 1024, 7)
    s = w["stats"]
    assert (s["grid"], s["trips"], s["min_trips"], s["busiest"], s["last_wg"], s["last_trip"]) == (1024, 3, 2, 6, 5, 3)   # slabs 0..5: three chunks
    a = w["apply"]
    assert (a["grid"], a["trips"], a["busiest"], a["last_wg"], a["last_trip"]) == (2048, 2, 6, 5, 2)
    w = SC.walk_bn(2085, 2048)
    assert (w["rpp"], w["chunks"], w["slabs"], w["last_rows"]) == (1, 2085, 66, 1)
    s, a = w["stats"], w["apply"]
    assert (s["grid"], s["trips"], s["min_trips"], s["busiest"]) == (66, 32, 31, 39)
    assert (a["grid"], a["trips"], a["busiest"], a["last_trip"]) == (2048, 2, 37, 2)
    # the shape the suite had: two chunks on eight slabs, one apply trip
    old = SC.walk_bn(33000, 64)
    assert (old["chunks"], old["stats"]["trips"], old["stats"]["busiest"], old["apply"]["trips"]) == (1032, 2, 8, 1)
    # the stem's map at batch 64 (256 x 256 x 64 per image): 131 072 chunks, every apply workgroup makes 64 trips, every slab 128
    stem = SC.walk_bn(64 * 256 * 256, 64)
    assert (stem["chunks"], stem["apply"]["min_trips"], stem["apply"]["trips"], stem["stats"]["trips"]) == (131072, 64, 64, 128)

    for P, C in SC.L2_SHAPES:
        w = SC.walk_l2(P)
        f, b = w["fwd"], w["bwd"]
        assert (w["fwd_grid"], f["sweep"], f["trips"], f["min_trips"], f["busiest"]) == (2048, 8192, 3, 2, 13)   # 13 waves: a third trip
        assert (w["bwd_grid"], b["sweep"], b["trips"], b["min_trips"], b["busiest"]) == (1536, 6144, 3, 2, 4109)
        assert LO.SHAPES[-1][0] == 2888 and SC.walk_l2(2888)["fwd"]["trips"] == 1 and SC.walk_l2(2888)["bwd"]["trips"] == 1
    assert {C <= 512 for _, C in SC.L2_SHAPES} == {True, False}                         # both NV instances
    w = SC.walk_l2(64 * 38 * 38)
    assert (w["fwd"]["trips"], w["bwd"]["trips"]) == (12, 16)


def test_audit_rows_without_a_tiled_case():
    # ssd_quantize_mx_fp8: the engines' largest stand-alone calls at batch 64, from their own plans
    from ssd_object_detection_amd import engine as E, ops
    from ssd_object_detection_amd.resnet_engine import mxfp8_bwd_plan, resnet50_ssd512_graph
    g = resnet50_ssd512_graph()
    size = {-1: 512}
    for i, nd in enumerate(g):
        src = nd["src"][0] if nd["op"] == "add" else nd["src"]
        size[i] = size[src] if nd["op"] not in ("conv", "pool3") else ops.same_pad(size[src], nd["k"], nd["stride"])[0]
    _, _, maps = mxfp8_bwd_plan(g)
    alone = {r: 64 * size[r] ** 2 * g[r]["cout"] for r, (kind, _) in maps.items() if kind != "fp8"}
    sweep = SC.QUANT_SWEEP * SC.QUANT_BLOCK
    assert max(alone.values()) == SC.QUANT_CALLS["resnet50 ssd512 backward"] == 2 * sweep
    assert sorted(r for r, n in alone.items() if n > sweep) == [6, 10] and (size[6], g[6]["cout"]) == (128, 256)
    for name, trunk, pri, res in (("ssd300 forward", E.SSD300_TRUNK, E.SSD300_NUM_PRIORS, 300),
                                  ("ssd512 forward", E.SSD512_TRUNK, E.SSD512_NUM_PRIORS, 512)):
        e = E.SSDEngine.planned(81, res, trunk, pri)
        plan = E.mxfp8_trunk_plan(e.nodes, e.chain_start)
        (q,) = plan.quant
        assert 64 * e.nodes[q]["hout"] ** 2 * e.nodes[q]["cout"] == SC.QUANT_CALLS[name] <= sweep
        # the filters' one flat quantise and the chain's largest pack, whatever the batch
        filters = sum(e.conv_params[i][0].numel for i in plan.fp8)
        assert filters < sweep // 8
        pieces = max(nd["cout"] * nd["k"] ** 2 * nd["cin"] // 8 for nd in e.nodes[e.chain_start:] if nd["kind"] == "conv")
        assert pieces == SC.CHAIN_PACK_LARGEST == 36864 and SC.walk(pieces, SC.CHAIN_PACK_CAP)["trips"] == 1
    assert max(c * k * k * ci // 8 for ci, c, k, _, _ in strict.EXTRA_LAYERS) == SC.CHAIN_PACK_LARGEST
    assert SC.CHAIN_PACK_CAP * SC.WG == 65536

    # k_conv0_fwd: tests/test_conv_gpu.py::test_first_layer_kernels_full_size
    B, H, W = conv_cases.FIRST_LAYER_CASE[:3]
    blocks = B * -(-H // SC.CONV0_BLOCK) * -(-W // SC.CONV0_BLOCK)
    w = SC.walk(blocks, SC.CONV0_CAP, 1)
    assert blocks == SC.FIRST_LAYER_BLOCKS == 1444 and (w["grid"], w["trips"], w["busiest"]) == (768, 2, 676)
    # k_loss_hist: tests/test_row_passes_persistent_gpu.py::test_reference_loss_second_trip
    w = SC.walk(PC.SHEADS[0] * PC.SHEADS[1], SC.LOSS_HIST_CAP)
    assert (w["grid"], w["sweep"], w["trips"]) == (256, 65536, 2)

    # k_hz_gemm: the suite's largest case stays on one trip, the new one does not
    B, _, levels = strict.SPARSE_CASES["B=4 splits"]
    w = SC.walk_hz(B, levels)
    assert (w["items"], w["cap_tiles"], w["trips"]) == (162, 216, 1)
    assert all(SC.walk_hz(b, lv)["trips"] == 1 for b, _, lv in strict.SPARSE_CASES.values())
    B, _, levels = SC.SPARSE_SWEEP
    w = SC.walk_hz(B, levels)
    assert (w["items"], w["cap_tiles"], w["grid"], w["trips"], w["busiest"]) == (2106, 2106, 2048, 2, 58)
    assert levels[0][6] - 28 * SC.HZ_TILE == 26 and 29 * 72 == 2088                     # the second trip: 40 tiles of the ragged row tile + level 1


def test_jpeg_images_past_one_stride():
    """tests/jpeg_cases.LARGE: the strides are the sources', the tiling with one copy is the fixture itself (Pillow's decode),
    and the oracle's image alone tells a later trip of k_jpeg_rgb from a repeated first one"""
    from tests import jpeg_cases as JC
    from tests import jpeg_oracle as J
    jpeg = source("jpeg.hip")
    assert constant(jpeg, "IDCT_GRID_X") * 256 == JC.IDCT_STRIDE and constant(jpeg, "RGB_GRID_X") * 256 == JC.RGB_STRIDE
    assert re.search(r"i < nblk; i \+= \(long long\)IDCT_GRID_X \* 256\)", jpeg) and re.search(r"i < npix; i \+= \(long long\)RGB_GRID_X \* 256\)", jpeg)
    assert re.search(r"dim3\(IDCT_GRID_X, \(unsigned\)B\)", jpeg) and re.search(r"dim3\(RGB_GRID_X, \(unsigned\)B\)", jpeg)
    most_blocks = max(JC.oracle(n)[0].size // 64 for n in JC.SUPPORTED)
    most_pixels = max(JC.decoded(n).shape[0] * JC.decoded(n).shape[1] for n in JC.SUPPORTED)
    assert (most_blocks, most_pixels) == (264, 5063)                      # one trip of either loop in every test so far
    for name, _, _, _, _ in JC.LARGE.values():
        w, h = JC.decoded(name).shape[1], JC.decoded(name).shape[0]
        assert np.array_equal(J.reconstruct(*JC.tiled(name, 1, 1, w, h)), JC.decoded(name))
    for key, trips_idct, trips_rgb in (("444", 2, 11), ("420", 1, 3)):
        coef, h = JC.tiled(*JC.LARGE[key])
        assert SC.walk(coef.size // 64, 64)["trips"] == trips_idct and SC.walk(h["width"] * h["height"], 128)["trips"] == trips_rgb
        img = J.reconstruct(coef, h)
        assert img.shape == (h["height"], h["width"], 3) and h["width"] % 8 and h["height"] % 8
        frac, count = SC.differs_across_sweep(torch.from_numpy(img), 3 * JC.RGB_STRIDE)
        print("jpeg %s: %d non-zero bytes past one stride, %.3f differ from the byte one stride earlier" % (key, count, frac))
        assert frac >= 0.5
    coef, h = JC.tiled(*JC.LARGE["444"])
    assert coef.size // 64 == 16632 and coef.size // 64 - JC.IDCT_STRIDE == 248
    # the blocks of the second trip are the last of the Cr plane (its last block rows: 4 x 11 blocks of the fixture), not all alike
    late = coef[64 * JC.IDCT_STRIDE:].reshape(-1, 64)
    assert len(np.unique(late, axis=0)) >= 40


# ---------------------------------------------------------------------------------------------------- the tiled references
def check_differs(t, floor=0.5):
    for name, sweep in t["sweeps"].items():
        frac, count = SC.differs_across_sweep(t[name], sweep)
        print("   %-6s %9d non-zero elements past one sweep, %.3f differ from the element one sweep earlier" % (name, count, frac))
        assert count > 0 and frac >= floor, (name, frac, count)


def test_eltwise_tiling():
    t = SC.eltwise_tiled()
    assert t["n"] == SC.ELT_NVEC * 8 and all(t[k].shape == (t["n"],) and t[k].dtype == BF for k in ("a", "b", "out", "g", "base", "masked", "acc"))
    # the tiled reference is the operation of the tiled inputs (element-wise: the whole tensor is cheap)
    out = (t["a"].float() + t["b"].float()).relu()
    assert torch.equal(out, t["out"].float())
    masked = strict.masked(t["g"].float(), out > 0)
    assert torch.equal(masked, t["masked"].float()) and torch.equal(t["base"].float() + masked, t["acc"].float())
    m = t["small"]["a"].numel()
    assert torch.equal(t["a"][5 * m:6 * m].float(), 2.0 * t["small"]["a"].reshape(-1).float()) and (SC.SWEEP_ITEMS * 8) % m != 0
    check_differs(t)


def test_mx_eltwise_tiling():
    t = SC.mx_eltwise_tiled()
    n = SC.MX_NVEC * 8
    assert t["out"].shape == (n // 32, 32) and t["q"].shape == (n // 32, 32) and t["s"].shape == (n // 32, 1)
    assert torch.equal((t["a"].float() + t["b"].float()).relu(), t["out"].float())
    zero = t["out"].float().abs().amax(-1) == 0
    assert bool((t["s"][zero] == 127).all())                                            # an all-zero block's byte does not move
    assert len(t["s"].unique()) > 40
    check_differs(t)


@pytest.mark.parametrize("which", ["3x3s2", "3x3s1"])
def test_pool_tiling(which):
    t = SC.pool3x3s2_tiled() if which == "3x3s2" else SC.pool3x3s1_tiled()
    k, small = t["copies"], t["small"]
    stride, (Ho, Wo, pt, pl) = (2, t["geom"]) if which == "3x3s2" else (1, small["x"].shape[1:3] + (1, 1))
    assert t["x"].shape[0] == k and t["y"].shape == (k, Ho, Wo, t["x"].shape[3]) and t["code"].dtype == torch.int32
    # the tiled reference is the reference of the tiled inputs: copies with each exponent, and the last one
    pick = torch.tensor([0, 1, 2, 3, 4, k - 1])
    y, code = strict.ref_pool(t["x"][pick].float(), 3, stride, pt, pl, Ho, Wo, 15)
    assert torch.equal(y, t["y"][pick].float()) and torch.equal(strict.pack_codes(code), t["code"][pick])
    dx = strict.ref_unpool(code, t["dy"][pick].float(), t["x"][pick].shape, 3, stride, pt, pl)
    assert torch.equal(dx, t["dx"][pick].float())
    assert torch.equal(t["x"][3].float(), 8.0 * small["x"][0].float()) and torch.equal(t["code"][3], t["code"][0])
    check_differs(t)


@pytest.mark.parametrize("ksize", [3, 2])
def test_quantising_pool_tiling(ksize):
    from tests import pool_mxfp8_cases as PQ
    t = SC.poolq_tiled(ksize)
    k = t["copies"]
    pick = torch.tensor([0, 1, 2, 3, 4, k - 1])
    y = PQ.ref(t["x"][pick], ksize, True)
    assert torch.equal(y.float(), t["y"][pick].float())
    q, s = strict.ref_quantize_mx(y)
    assert torch.equal(q, t["q"][pick]) and torch.equal(s, t["s"][pick])
    assert t["y"].shape[0] == k and t["y"].numel() // 8 == (2099576 if ksize == 3 else 2097600)
    check_differs(t)


def test_quantiser_tiling():
    t = SC.quantize_tiled()
    assert t["x"].shape == (SC.QUANT_NBLK, 32) and t["q"].shape == (SC.QUANT_NBLK, 32) and t["s"].shape == (SC.QUANT_NBLK, 1)
    m = t["small"].shape[0]
    assert (SC.QUANT_SWEEP % m) != 0
    # the expectation by tiling is the reference quantiser's: the first copies, copies around one sweep, and the cut last one
    for lo, hi in ((0, 6 * m), (SC.QUANT_SWEEP - m, SC.QUANT_SWEEP + m), (SC.QUANT_NBLK - 2 * m, SC.QUANT_NBLK)):
        q, s = strict.ref_quantize_mx(t["x"][lo:hi])
        assert torch.equal(q, t["q"][lo:hi]) and torch.equal(s, t["s"][lo:hi]), (lo, hi)
    check_differs(t)


def test_sparse_sweep_case_regime():
    case = SC.sparse_sweep_case()
    strict.check_sparse_regime(case["levels"])
    for l, (H, W, Cin, n, C, npad, count) in zip(case["levels"], SC.SPARSE_SWEEP[2]):
        k, por, rop = l["count"], l["pixel_of_row"], l["row_of_pixel"]
        assert k == count and tuple(l["x"].shape) == (case["B"], H, W, Cin) and l["cout"] == n * (4 + C)
        assert bool((por[:k][1:] > por[:k][:-1]).all()) and int((rop >= 0).sum()) == k
        assert bool((l["rows"][k:].float() == strict.UNREAD).all()) and bool((l["dx"] != 0).any())
    # the tiles of the second trip hold gradient: rows 3584.. of level 0 reach pixels, and level 1 has rows
    l0 = case["levels"][0]
    late = l0["pixel_of_row"][28 * SC.HZ_TILE:l0["count"]].long()
    assert bool((l0["rows"][28 * SC.HZ_TILE:l0["count"]].float() != 0).any()) and len(late) == 26


# ---------------------------------------------------------------------------------------------------- fp32 emulations, new shapes
@pytest.mark.parametrize("order", ["sequential", "pairwise"])
@pytest.mark.parametrize("shape", SC.BN_SHAPES, ids=str)
def test_batchnorm_bounds_admit_fp32_at_the_new_shapes(shape, order):
    """tests/test_batchnorm_cpu.py::test_bounds_admit_fp32_in_any_order's figures at BN_SHAPES: the bounds are the oracle's own"""
    k = BO.make_case(*shape)
    run = (k["rm"], k["rv"])
    r64 = BO.fwd64(k["x"], k["gamma"], k["beta"], relu=True, running=run)
    b = BO.fwd_bounds(k["x"], k["gamma"], k["beta"], running=run)
    r32 = BO.fwd32(k["x"], k["gamma"], k["beta"], relu=True, running=run, order=order)
    figures = {n: BO.worst(r32[n], r64[n], b[n]) for n in ("y", "mean", "var", "rstd", "rm", "rv")}
    a32 = k["gamma"] / np.sqrt(k["rv"] + np.float32(BO.EPS))
    yi = BO.bf16_round(np.maximum(k["x"] * a32 + (k["beta"] - k["rm"] * a32), np.float32(0)))
    figures["infer"] = BO.worst(yi, BO.infer64(k["x"], k["gamma"], k["beta"], k["rm"], k["rv"], relu=True),
                                BO.infer_bound(k["x"], k["gamma"], k["beta"], k["rm"], k["rv"]))
    dx, dg, db = BO.bwd32(k["dy"], k["x"], k["gamma"], r32["mean"], r32["rstd"], order=order)
    m64, s64 = r32["mean"].astype(np.float64), r32["rstd"].astype(np.float64)
    want = BO.bwd64(k["dy"], k["x"], k["gamma"], m64, s64)
    bb = BO.bwd_bounds(k["dy"], k["x"], k["gamma"], m64, s64)
    for n, got, w in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), want):
        figures[n] = BO.worst(got, w, bb[n])
    print(shape, order, figures)
    assert all(v <= 1.0 for v in figures.values()), figures


@pytest.mark.parametrize("order", ["sequential", "pairwise"])
@pytest.mark.parametrize("shape", SC.L2_SHAPES, ids=str)
def test_l2norm_bounds_admit_fp32_at_the_new_shapes(shape, order):
    """tests/test_l2norm_cpu.py::test_float32_restatement_is_inside_the_bounds' figures at L2_SHAPES"""
    k = LO.make_case(*shape)
    y64, r64, _ = LO.fwd64(k["x"], k["s"])
    y, r, _ = LO.fwd32(k["x"], k["s"], order=order)
    figures = {}
    for old in (None, k["old"]):
        b = LO.bounds(k["dy"], k["x"], k["s"], old=old)
        dx64, ds64 = LO.bwd64(k["dy"], k["x"], k["s"], old=old)
        dx, ds = LO.bwd32(k["dy"], k["x"], k["s"], old=old, order=order)
        figures["dx acc" if old is not None else "dx"] = LO.worst(dx, dx64, b["dx"])
        figures["ds"] = LO.worst(ds, ds64, b["ds"])
    figures["y"] = LO.worst(y, y64, b["y"])
    print(shape, order, {n: round(v, 3) for n, v in figures.items()}, "r / (4 u r64): %.3f" % LO.worst(r, r64, b["r"]))
    assert all(v <= 1.0 for v in figures.values()), figures
