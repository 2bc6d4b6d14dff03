"""CPU suite: launch sizes of the LDS-patch convolution kernels at batch 64 (ssd_conv2d_*_workgroups, include/ssd_hip.h: the
dispatch code with launching switched off, so no GPU is needed).  k_conv3x3_p512 runs ONE workgroup per CU (256 CUs) and
k_conv3x3_patch32 two, so the number of active workgroups decides how many rounds a launch takes and how full the last
one is.  The counts are arithmetic:
  * position strips at row pitch W + 1: 64 x 39 x 39 positions = 190.1 -> 191 blocks of 512, x 4 channel tiles = 764 <= 768,
    three whole rounds (pitch W + 2 gave 195 blocks = 780 workgroups, a fourth round for 12 of them);
  * row strips under fused pooling, image pitch even: 75 rows -> pitch 76, ceil(64 x 76 / 32) = 152 strips x 5 column tiles
    x 2 channel tiles = 1520 (per-image blocks: 3 x 64 x 5 x 2 = 1920); 150 rows -> pitch 152, 64 x 152 / 16 = 608 strips
    x 10 column tiles = 6080 (per-image blocks: 10 x 64 x 10 = 6400)."""
import pytest

from tests.conv_cases import WS_BYTES, plan_name

F_ROWFLAT, F_POOL = 0x200, 0x800


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def fwd(L, B, H, Cin, Cout, pool=0):
    a = (B, H, H, Cin, Cout, 3, 1, 1, 1, H, H, pool, WS_BYTES)
    return L.ssd_conv2d_fwd_plan(*a), L.ssd_conv2d_fwd_workgroups(*a)


def dgrad(L, B, H, Cin, Cout):
    a = (B, H, H, Cin, Cout, 3, 1, 1, 1, H, H, 0, WS_BYTES)
    return L.ssd_conv2d_bwd_data_plan(*a), L.ssd_conv2d_bwd_data_workgroups(*a)


@pytest.mark.parametrize("Cin", [512, 256])
def test_position_strips_at_38x38_fill_three_whole_rounds(L, Cin):
    plan, wgs = fwd(L, 64, 38, Cin, 512)
    assert plan_name(L, plan) == "k_conv3x3_p512+flat"
    assert wgs == 764 and wgs <= 3 * 256


def test_data_gradient_at_38x38_fills_three_whole_rounds(L):
    plan, wgs = dgrad(L, 64, 38, 512, 512)
    assert plan_name(L, plan) == "k_conv3x3_p512+flat"
    assert wgs == 764


@pytest.mark.parametrize("pool", [1, 2])
def test_pooled_block3_conv3_runs_on_row_strips(L, pool):
    plan, wgs = fwd(L, 64, 75, 256, 256, pool)
    assert plan_name(L, plan) == "k_conv3x3_p512+rowflat+poolfused"
    assert plan & F_ROWFLAT and plan & F_POOL
    assert wgs == 1520
    assert fwd(L, 64, 75, 256, 256, 0)[1] == 1520             # the same tiling as the layer before it, which does not pool


@pytest.mark.parametrize("pool", [1, 2])
def test_pooled_block2_conv2_runs_on_row_strips(L, pool):
    plan, wgs = fwd(L, 64, 150, 128, 128, pool)
    assert plan_name(L, plan) == "k_conv3x3_patch32<128>+rowflat+poolfused"
    assert plan & F_ROWFLAT and plan & F_POOL
    assert wgs == 6080
    assert fwd(L, 64, 150, 128, 128, 0)[1] == 64 * 151 // 16 * 10   # without pooling the pitch stays H + 1: 604 strips


def test_row_strips_are_taken_only_when_they_need_fewer_blocks(L):
    # 64 rows: per-image blocks tile the map exactly (4 x 16), a strip with zero rows between images would need more
    plan, wgs = fwd(L, 8, 64, 128, 128, 1)
    assert plan_name(L, plan) == "k_conv3x3_patch32<128>+poolfused"
    assert wgs == 8 * 4 * 4


def test_counts_of_the_other_launch_sites(L):
    # generic implicit GEMM: pixel tiles x channel tiles (x split-K slices); a call that is rejected stays rejected
    plan, wgs = fwd(L, 64, 19, 1024, 256, 0)
    assert plan > 0 and wgs > 0
    from ssd_object_detection_amd import _lib
    assert L.ssd_conv2d_fwd_workgroups(0, 38, 38, 64, 64, 3, 1, 1, 1, 38, 38, 0, WS_BYTES) == _lib.SSD_ERR_VALUE
    # the persistent pointwise GEMM sizes its grid by the device, not by the shape
    assert L.ssd_conv2d_fwd_workgroups(64, 38, 38, 512, 512, 1, 1, 0, 0, 38, 38, 0, WS_BYTES) == _lib.SSD_ERR_UNSUPPORTED
