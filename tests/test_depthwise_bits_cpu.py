"""CPU suite of the sign-byte forms of the depthwise 3x3 convolution (ssd_dwconv3x3_fwd_relubits, ssd_dwconv3x3_bwd_data_bits):
every host-side refusal through the C ABI.  A refusal is decided before any launch, so the calls run without a GPU, and their
pointers are either never dereferenced (distinct addresses 256 MiB apart) or host buffers whose bytes must come back untouched."""
import ctypes

import pytest

torch = pytest.importorskip("torch")

from tests.test_depthwise_cpu import GEOMETRY_UNSUPPORTED, GEOMETRY_VALUE, OK, P                              # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib, _lib.lib()


def at(p, delta):
    return ctypes.c_void_p(p.value + delta)


def fwd(L, a):
    return L.ssd_dwconv3x3_fwd_relubits(a["x"], a["w"], a["bias"], a["y"], a["bits"], a["B"], a["H"], a["W"], a["C"], a["s"], a["pt"],
                                        a["pl"], a["Ho"], a["Wo"], None)


def bwd(L, a):
    return L.ssd_dwconv3x3_bwd_data_bits(a["dy"], a["w"], a["bits"], a["dx"], a["B"], a["H"], a["W"], a["C"], a["s"], a["pt"], a["pl"],
                                         a["Ho"], a["Wo"], a["acc"], None)


def test_fwd_relubits_refuses_on_the_host(lib):
    _lib, L = lib
    V, U = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    ok = dict(OK, x=P(0), w=P(1), bias=P(2), y=P(3), bits=P(4))
    ybytes = 2 * 19 * 19 * 72 * 2
    # what the sibling refuses, the NULL sign bytes, and sign bytes that touch the other output or an input
    for kv in (dict(x=None), dict(w=None), dict(y=None), dict(y=ok["x"]), dict(y=ok["w"]), dict(y=ok["bias"]),
               dict(y=at(ok["x"], 64)), dict(y=at(ok["x"], -64)),
               dict(bits=None), dict(bits=ok["y"]), dict(bits=at(ok["y"], ybytes - 1)), dict(bits=at(ok["y"], 1 - ybytes // 16)),
               dict(bits=ok["x"]), dict(bits=ok["w"]), dict(bits=ok["bias"])) + GEOMETRY_VALUE:
        assert fwd(L, dict(ok, **kv)) == V, kv
    for kv in GEOMETRY_UNSUPPORTED:
        assert fwd(L, dict(ok, **kv)) == U, kv
    # sign bytes that END where y begins, or begin where it ends, overlap nothing: refused for the channel count alone
    y12 = 2 * 19 * 19 * 12 * 2                                             # (the sizes at C = 12)
    for kv in (dict(bits=at(ok["y"], y12)), dict(bits=at(ok["y"], -(y12 // 16)))):
        assert fwd(L, dict(ok, C=12, **kv)) == U, kv
    # served geometries that a refusal must not catch (refused for the NULL x alone, then for the channel count alone)
    for kv in (dict(pt=0, pl=0, Ho=17, Wo=17), dict(s=2, Ho=10, Wo=10), dict(H=10, W=10, s=2, pt=0, pl=0, Ho=5, Wo=5)):
        assert fwd(L, dict(ok, x=None, **kv)) == V, kv
        assert fwd(L, dict(ok, C=12, **kv)) == U, kv


def test_bwd_data_bits_refuses_on_the_host(lib):
    _lib, L = lib
    V, U = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    ok = dict(OK, dy=P(0), w=P(1), bits=P(2), dx=P(3), acc=0)
    dxbytes = 2 * 19 * 19 * 72 * 2
    for acc in (0, 1):
        for kv in (dict(dy=None), dict(w=None), dict(dx=None), dict(dx=ok["dy"]), dict(dx=ok["w"]),
                   dict(bits=None), dict(bits=ok["dx"]),                   # unlike relu_src, the sign bytes may not BE dx
                   dict(bits=at(ok["dx"], dxbytes - 1)), dict(bits=at(ok["dx"], 1 - dxbytes // 16))) + GEOMETRY_VALUE:
            assert bwd(L, dict(ok, acc=acc, **kv)) == V, kv
        for kv in GEOMETRY_UNSUPPORTED:
            assert bwd(L, dict(ok, acc=acc, **kv)) == U, kv
        x12 = 2 * 19 * 19 * 12 * 2                                         # (the sizes at C = 12: touching is no overlap)
        for kv in (dict(bits=at(ok["dx"], x12)), dict(bits=at(ok["dx"], -(x12 // 16)))):
            assert bwd(L, dict(ok, acc=acc, C=12, **kv)) == U, kv


def test_nothing_is_written_on_a_refusal(lib):
    """Real host buffers, so a write would land: every refusal of both entry points leaves every byte of every buffer as it was."""
    _lib, L = lib
    B, H, W, C = 1, 4, 4, 8
    big = {k: torch.full((B * H * W * C,), 0x5a5a, dtype=torch.int16) for k in ("x", "y", "dy", "dx")}
    small = {"w": torch.full((9 * C,), 0x5a5a, dtype=torch.int16), "bias": torch.full((C,), 3.0), "bits": torch.full((B * H * W,), 0x5a, dtype=torch.uint8)}
    bufs = dict(big, **small)
    before = {k: v.clone() for k, v in bufs.items()}
    p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in bufs.items()}
    # Every call carries C = 12 as a second, independent reason to be refused (SSD_ERR_UNSUPPORTED, decided after the NULL and
    # geometry checks), so no single missing check can launch a kernel on these host buffers; the code returned shows which
    # check spoke.  The overlap refusals are decided last and have no such second reason: they run on the pointers above only.
    V, U = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    ok = dict(p, B=B, H=H, W=W, C=12, s=1, pt=1, pl=1, Ho=H, Wo=W, acc=1)
    common = (dict(bits=None), dict(s=3), dict(pt=2), dict(Ho=H + 2), dict(B=0))
    for kv in common + (dict(x=None), dict(w=None), dict(y=None)):
        assert fwd(L, dict(ok, **kv)) == V, kv
    for kv in common + (dict(dy=None), dict(w=None), dict(dx=None)):
        assert bwd(L, dict(ok, **kv)) == V, kv
    assert fwd(L, ok) == U and bwd(L, ok) == U and bwd(L, dict(ok, acc=0)) == U
    for k, v in bufs.items():
        assert torch.equal(v, before[k]), k


def test_wrappers_and_prototypes_exist(lib):
    _lib, L = lib
    import ssd_object_detection_amd.ops as ops
    for name in ("dwconv3x3_fwd_relubits", "dwconv3x3_bwd_data_bits"):
        assert callable(getattr(ops, name))
    assert L.ssd_dwconv3x3_fwd_relubits.restype is ctypes.c_int and L.ssd_dwconv3x3_bwd_data_bits.restype is ctypes.c_int
