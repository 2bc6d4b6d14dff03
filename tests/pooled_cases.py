"""Shapes of the three pooled-layer entry points under the strict harness, shared by tests/test_pooled_cases_cpu.py (regime,
dispatch, census of the operands, power against wrong references: CPU) and tests/test_pooled_layers_strict_gpu.py (the kernels
in a guarded arena, -m gpu).  As tests/conv_cases.py: every case names the kernel it is there for, as the library's dispatch
queries report it at default knobs (host functions: they run without a GPU), and both test files assert the names.

  ssd_conv2d_fwd_pool             convolution + 2x2 pooling in the store stage        FWD_POOL_CASES
  ssd_conv2d_bwd_data_unpool      data gradient un-pooled in the store stage          UNPOOL_CASES, UNPOOL_REFUSED
  ssd_conv2d_bwd_weight_unpooled  weight gradient from the pooled gradient + codes    WGRAD_UNPOOLED_CASES, WGRAD_UNPOOLED_REFUSED

Every convolution is 3x3 / stride 1 / SAME."""
from tests.conv_cases import WS_BYTES, plan_name

C64B, P32_64, P32_128, P512 = "k_conv3x3_c64b", "k_conv3x3_patch32<64>", "k_conv3x3_patch32<128>", "k_conv3x3_p512"
FUSED = "+poolfused"

# (B, H, W, Cin, Cout, plan with y (pool = 1), plan without y (pool = 2)).  Each runs with SAME and VALID pooling, relu 1 and 0;
# a fused case also without y; the last case has no pooling kernel: two launches with y, refused without.
FWD_POOL_CASES = [
    (2, 21, 37, 64, 64, C64B + FUSED, C64B + FUSED),                                    # odd both ways, ragged 8x16 blocks
    (2, 20, 36, 64, 64, C64B + FUSED, C64B + FUSED),                                    # even both ways
    (3, 17, 19, 64, 64, C64B + FUSED, C64B + FUSED),                                    # the smallest odd map
    (3, 33, 35, 128, 64, P32_64 + "+rowflat" + FUSED, P32_64 + "+rowflat" + FUSED),     # row strip at image pitch H + 1
    (2, 32, 48, 128, 64, P32_64 + FUSED, P32_64 + FUSED),                               # blocks; even H: pitch H + 2
    (3, 33, 33, 64, 128, P32_128 + "+rowflat" + FUSED, P32_128 + "+rowflat" + FUSED),
    (2, 32, 32, 64, 128, P32_128 + FUSED, P32_128 + FUSED),
    (2, 33, 35, 256, 128, P512 + "+rowflat" + FUSED, P512 + "+rowflat" + FUSED),
    (2, 64, 32, 256, 128, P512 + FUSED, P512 + FUSED),
    (2, 19, 19, 64, 192, P32_128 + "+flat", "error -2"),                                # position strips never pool: the fallback
]

# (B, Hf, Wf, C of the pooled map, Cout of the convolution behind it, SAME pooling, plan of ssd_conv2d_bwd_data_unpool_plan)
UNPOOL_CASES = [
    (2, 41, 66, 64, 64, True, P32_64 + "+rowflat"),        # -> 21x33; 64 -> 64 that must NOT reach k_conv3x3_c64b
    (2, 42, 66, 64, 64, False, P32_64 + "+rowflat"),       # -> 21x33
    (3, 65, 66, 128, 64, True, P32_128 + "+rowflat"),      # -> 33x33
    (3, 64, 64, 128, 64, False, P32_128),                  # -> 32x32: blocks
    (2, 65, 66, 128, 256, True, P512 + "+rowflat"),        # -> 33x33
    (2, 38, 37, 128, 256, True, P512),                     # -> 19x19: one 32-row block per image
    (3, 37, 38, 192, 64, True, P32_128 + "+flat"),         # -> 19x19: position strips, blocks spanning images, ragged second channel tile
    (3, 38, 38, 64, 128, False, P32_64 + "+rowflat"),      # -> 19x19
]
# refused with SSD_ERR_UNSUPPORTED, dx_full and dx_pooled untouched: VALID pooling of an odd size (the uncovered row / column would
# not be written); a 10x10 pooled map (below 16: the generic kernel, which has no un-pooling store)
UNPOOL_REFUSED = [(2, 41, 41, 64, 64, False), (2, 20, 20, 64, 64, True)]

# (B, H, W, Cin, Cout, SAME pooling, (splits, 16x16 blocks)); splits = workspace bytes / ((Cout * 9 * Cin + Cout) * 4)
WGRAD_UNPOOLED_CASES = [
    (1, 16, 16, 64, 64, False, (1, 1)),        # one block, one split, one channel group
    (2, 21, 37, 64, 64, True, (12, 12)),       # odd both ways: windows clipped on both edges; Hp = 11: windows 11 .. 15 of the second tile row are out of range
    (2, 21, 37, 64, 64, False, (12, 12)),      # row 20 and column 36 get no gradient but are read as neighbours
    (3, 17, 19, 64, 128, True, (12, 12)),      # two output-channel tiles; one pixel over the 16-pixel block
    (3, 33, 33, 128, 256, True, (27, 27)),     # eight channel groups
    (4, 33, 33, 256, 256, True, (18, 36)),     # two blocks per workgroup; a split over two images; sixteen channel groups
]
LARGEST_WGRAD_CASE = WGRAD_UNPOOLED_CASES[-1]
# (B, H, W, Cin, Cout, Hp, Wp): SSD_ERR_UNSUPPORTED, dw / dbias untouched
WGRAD_UNPOOLED_REFUSED = [(1, 15, 16, 64, 64, 7, 8), (1, 16, 16, 96, 64, 8, 8), (1, 16, 16, 64, 64, 9, 8)]


def pooled_size(n, same):
    return (n + 1) // 2 if same else n // 2


def fwd_pool_plans(L, case):
    B, H, W, Cin, Cout = case[:5]
    return tuple(plan_name(L, L.ssd_conv2d_fwd_plan(B, H, W, Cin, Cout, 3, 1, 1, 1, H, W, pool, WS_BYTES)) for pool in (1, 2))


def unpool_plan(L, case, has_relu_src=0):
    B, Hf, Wf, C, Cout, same = case[:6]
    return plan_name(L, L.ssd_conv2d_bwd_data_unpool_plan(B, pooled_size(Hf, same), pooled_size(Wf, same), C, (Cout + 7) // 8 * 8, Hf, Wf,
                                                          has_relu_src, WS_BYTES))


def wgrad_unpooled_splits(L, case):
    """(splits, blocks, blocks per split) of a weight-gradient case, from the workspace query"""
    B, H, W, Cin, Cout, same = case[:6]
    nbytes = L.ssd_conv2d_bwd_weight_unpooled_workspace_bytes(B, H, W, Cin, Cout, pooled_size(H, same), pooled_size(W, same))
    per = (Cout * 9 * Cin + Cout) * 4
    assert nbytes > 0 and nbytes % per == 0
    ns, tiles = nbytes // per, B * ((H + 15) // 16) * ((W + 15) // 16)
    return ns, tiles, -(-tiles // ns)
