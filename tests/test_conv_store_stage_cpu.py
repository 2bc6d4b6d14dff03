"""CPU suite: the LDS a convolution launch asks for (ssd_conv2d_*_lds_bytes, include/ssd_hip.h: the dispatch code with
launching switched off, so no GPU is needed).  k_conv3x3_p512 keeps the side tables of its store stage (sign bytes, row map,
bias) above everything its main loop uses, inside the 163840 bytes a gfx950 workgroup may have; k_conv3x3_patch32 must keep
its 81920 (two workgroups per CU), so its row map reuses the weight buffers instead."""
import pytest

from tests.conv_cases import CASES, FULL_SIZE_CASES, RESNET_CASES, FIRST_LAYER_CASE, WS_BYTES, _geom, plan_name

WORKGROUP_LDS = 160 * 1024
P512_LOOP = 2 * 58 * 1024 + 4 * 128 * 64 + 1024             # two patch buffers, four weight slots, the dummy zone
P512_SIDE = 512 * 16 + 512 * 4 + 128 * 4                    # sign bytes, row map, bias


@pytest.fixture(scope="module")
def L():
    from ssd_object_detection_amd import _lib
    return _lib.lib()


def launches(L, case, **knobs):
    """(kernel name, LDS bytes) of the forward, the pooled forward and both data gradients of a conv_cases shape"""
    B, H, W, Cin, Cout, k, stride, mode = case[:8]
    Ho, Wo, pt, pl = _geom(H, W, k, stride, mode)
    cp = (Cout + 7) // 8 * 8
    out = []
    for pool in (0, 1, 2):
        a = (B, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo, pool, WS_BYTES)
        out.append((L.ssd_conv2d_fwd_plan(*a), L.ssd_conv2d_fwd_lds_bytes(*a)))
    for acc in (0, 1):
        a = (B, H, W, Cin, cp, k, stride, pt, pl, Ho, Wo, acc, WS_BYTES)
        out.append((L.ssd_conv2d_bwd_data_plan(*a), L.ssd_conv2d_bwd_data_lds_bytes(*a)))
    return [(plan_name(L, p), n) for p, n in out if p >= 0]


ALL = CASES + FULL_SIZE_CASES + RESNET_CASES + [FIRST_LAYER_CASE]


@pytest.mark.parametrize("p512", [1, 2])
def test_p512_lds_fits_a_workgroup_for_every_conv_case(L, p512):
    seen = 0
    assert L.ssd_dev_knob(b"SSD_CONV_P512", p512) == 0
    try:
        for case in ALL:
            for name, lds in launches(L, case):
                if name.startswith("k_conv3x3_p512"):
                    assert lds == P512_LOOP + P512_SIDE and lds <= WORKGROUP_LDS, (case[:8], name, lds)
                    seen += 1
                elif name.startswith("k_conv3x3_patch32"):
                    assert lds == 80 * 1024, (case[:8], name, lds)           # two workgroups per CU: no byte more than before
                elif name != "k_pw_gemm":
                    assert 0 <= lds <= WORKGROUP_LDS, (case[:8], name, lds)
    finally:
        L.ssd_dev_knob(b"SSD_CONV_P512", 1)
    assert seen >= 8                                             # the cases of conv_cases.py that name the kernel


def test_lds_query_follows_the_plan_query(L):
    from ssd_object_detection_amd import _lib
    assert L.ssd_conv2d_fwd_lds_bytes(0, 38, 38, 64, 64, 3, 1, 1, 1, 38, 38, 0, WS_BYTES) == _lib.SSD_ERR_VALUE
    assert L.ssd_conv2d_fwd_lds_bytes(64, 38, 38, 512, 512, 1, 1, 0, 0, 38, 38, 0, WS_BYTES) == _lib.SSD_ERR_UNSUPPORTED   # k_pw_gemm
    assert L.ssd_conv2d_fwd_lds_bytes(4, 300, 300, 8, 64, 3, 1, 1, 1, 300, 300, 0, WS_BYTES) == 0                          # k_conv0_fwd: static LDS


def test_store_stage_knob_exists(L):
    assert L.ssd_dev_knob(b"SSD_EPI_PREFETCH", 0) == 0
    assert L.ssd_dev_knob(b"SSD_EPI_PREFETCH", 1) == 0
