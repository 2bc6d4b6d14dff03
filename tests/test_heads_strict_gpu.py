"""GPU: the sparse head backward kernels (ssd_heads_bwd_data_sparse[_levels], ssd_heads_bwd_weight_sparse) under the strict
harness (tests/strict.py), through the C ABI.

The compact rows are hand made in the pattern the loss produces (a few entries of +-2^-6 and +-2^-8 per row), x holds integers
of {-2..2} and the head filters {-1, 0, 1}: the torch CPU fp32 conv gradients of the scattered dense dy are exact, dx is
bf16-exact (tests/test_strict_cpu.py asserts the regime) and every comparison is torch.equal.  Row counts sit around
k_hz_gemm's 128-row tile and k_hw_gather's split threshold, B * hw is no multiple of k_hz_col2im's four pixels, the maps are
not square, and rows past count hold 2^100: a read of them reaches the result.  Everything lives in strict.Arena with
workspaces of exactly *_workspace_bytes.  The chained case runs an exact loss case and both backward kernels on the rows it
leaves, as the engines do."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import strict                                                                         # noqa: E402
from tests.test_loss_strict_gpu import INPUTS, HeadBuffers, heads_call, nbytes, put_inputs       # noqa: E402

BF, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32


@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Given:
    """hand-made ssd_head_grads contents as inputs of an arena"""

    def __init__(self, a, lib, levels):
        self.rows = [a.put(l["rows"], "rows[%d]" % i) for i, l in enumerate(levels)]
        self.rop = [a.put(l["row_of_pixel"], "row_of_pixel[%d]" % i) for i, l in enumerate(levels)]
        self.por = [a.put(l["pixel_of_row"], "pixel_of_row[%d]" % i) for i, l in enumerate(levels)]
        counts = torch.full((lib.SSD_MAX_LEVELS,), -12345, dtype=I32)              # count[levels..7] is never read
        counts[:len(levels)] = torch.tensor([l["count"] for l in levels], dtype=I32)
        self.count = a.put(counts, "count")
        c = lib.HeadGrads()
        c.levels = len(levels)
        for i, l in enumerate(levels):
            c.hw[i], c.per_cell[i], c.npad[i] = l["hw"], l["n"], l["npad"]
            c.rows[i], c.row_of_pixel[i], c.pixel_of_row[i] = self.rows[i].data_ptr(), self.rop[i].data_ptr(), self.por[i].data_ptr()
        c.count = self.count.data_ptr()
        self.c = c


class Layers:
    """ssd_head_layers in an arena: operands as inputs, dx / dw / dbias as outputs"""

    def __init__(self, a, lib, B, levels, relu, bias=True):
        self.x = [a.put(l["x"], "x[%d]" % i) for i, l in enumerate(levels)]
        self.w = [a.put(l["w_tap"], "w_tap[%d]" % i) for i, l in enumerate(levels)]
        self.bits = [a.put(l["bits"], "relu_bits[%d]" % i) for i, l in enumerate(levels)] if relu == "bits" else None
        self.dx = [a.out(tuple(l["x"].shape), BF, "dx[%d]" % i) for i, l in enumerate(levels)]
        self.dw = [a.out(tuple(l["w"].shape), F32, "dw[%d]" % i) for i, l in enumerate(levels)]
        self.db = [a.out((l["cout"],), F32, "dbias[%d]" % i) for i, l in enumerate(levels)] if bias else None
        c = lib.HeadLayers()
        c.levels = len(levels)
        for i, l in enumerate(levels):
            c.H[i], c.W[i], c.Cin[i], c.cout[i] = l["H"], l["W"], l["Cin"], l["cout"]
            c.x[i], c.w_tap[i], c.dx[i], c.dw[i] = self.x[i].data_ptr(), self.w[i].data_ptr(), self.dx[i].data_ptr(), self.dw[i].data_ptr()
            c.dbias[i] = self.db[i].data_ptr() if bias else None
            c.relu_bits[i] = self.bits[i].data_ptr() if relu == "bits" else None
            c.relu_src[i] = self.x[i].data_ptr() if relu == "src" else None
        self.c = c

    @staticmethod
    def bytes(levels):
        out = []
        for l in levels:
            out += [nbytes(l["x"]), nbytes(l["w_tap"]), nbytes(l["bits"]), nbytes(l["x"]), 4 * l["w"].numel(), 4 * l["cout"]]
        return out


def given_bytes(levels):
    out = [32]
    for l in levels:
        out += [nbytes(l["rows"]), nbytes(l["row_of_pixel"]), nbytes(l["pixel_of_row"])]
    return out


def setup(lib, case, bias=True):
    L = lib.lib()
    B, levels, relu = case["B"], case["levels"], case["relu"]
    sizes = given_bytes(levels) + Layers.bytes(levels)
    # the workspace sizes depend on the structs' geometry only: ask with throw-away structs
    hl0, hg0 = lib.HeadLayers(), lib.HeadGrads()
    hl0.levels = hg0.levels = len(levels)
    for i, l in enumerate(levels):
        hl0.H[i], hl0.W[i], hl0.Cin[i], hl0.cout[i] = l["H"], l["W"], l["Cin"], l["cout"]
        hg0.hw[i], hg0.per_cell[i], hg0.npad[i] = l["hw"], l["n"], l["npad"]
    zb = L.ssd_heads_bwd_data_sparse_workspace_bytes(B, ctypes.byref(hl0))
    wb = L.ssd_heads_bwd_weight_sparse_workspace_bytes(B, ctypes.byref(hg0), ctypes.byref(hl0))
    a = strict.Arena("cuda", strict.Arena.bytes_for(*sizes, zb, wb))
    hg = Given(a, lib, levels)
    hl = Layers(a, lib, B, levels, relu, bias)
    ws = a.workspace()
    return L, a, hg, hl, ws.get(zb, "cuda"), zb, ws.get(wb, "cuda"), wb


@pytest.mark.parametrize("name", sorted(strict.SPARSE_CASES), ids=str)
def test_sparse_data_gradient_exact(lib, name):
    """every dx element written -- zeros where no row reaches -- and equal to the fp32 reference, ReLU-masked by bits / by the
    activation / not at all"""
    case = strict.sparse_cached(name)
    L, a, hg, hl, zws, zb, _, _ = setup(lib, case)

    def fn():
        st = L.ssd_heads_bwd_data_sparse(ctypes.byref(hg.c), ctypes.byref(hl.c), case["B"], ptr(zws), zb, stream())
        assert st == 0, st
    a.run(fn, [(hl.dx[i], l["dx"].to(BF)) for i, l in enumerate(case["levels"])])


@pytest.mark.parametrize("bias", [True, False], ids=["dbias", "no dbias"])
@pytest.mark.parametrize("name", sorted(strict.SPARSE_CASES), ids=str)
def test_sparse_weight_gradient_exact(lib, name, bias):
    """dw and dbias (present or NULL) equal to the fp32 reference: one and two active pixel splits, a level without rows"""
    case = strict.sparse_cached(name)
    L, a, hg, hl, _, _, wws, wb = setup(lib, case, bias)

    def fn():
        st = L.ssd_heads_bwd_weight_sparse(ctypes.byref(hg.c), ctypes.byref(hl.c), case["B"], ptr(wws), wb, stream())
        assert st == 0, st
    expect = [(hl.dw[i], l["dw"]) for i, l in enumerate(case["levels"])]
    if bias:
        expect += [(hl.db[i], l["dbias"]) for i, l in enumerate(case["levels"])]
    a.run(fn, expect)


@pytest.mark.parametrize("levels", [(0,), (4,), (0, 4), (1, 2, 3), (0, 1, 2, 3, 4)], ids=str)
def test_level_subsets_write_their_levels_only(lib, levels):
    """ssd_heads_bwd_data_sparse_levels: the levels of the mask equal the whole call's, the others are not touched"""
    case = strict.sparse_cached("B=1 bits")
    L, a, hg, hl, zws, zb, _, _ = setup(lib, case)
    mask = sum(1 << l for l in levels)

    def fn():
        st = L.ssd_heads_bwd_data_sparse_levels(ctypes.byref(hg.c), ctypes.byref(hl.c), case["B"], mask, ptr(zws), zb, stream())
        assert st == 0, st
    a.run(fn, [(hl.dx[i], case["levels"][i]["dx"].to(BF)) for i in levels])
    assert L.ssd_heads_bwd_data_sparse_levels(ctypes.byref(hg.c), ctypes.byref(hl.c), case["B"], 0, ptr(zws), zb, stream()) == lib.SSD_ERR_VALUE


def test_loss_feeds_both_backward_kernels(lib):
    """An exact loss case in the compact-row form, then the data and the weight gradient of seven head levels from the rows it
    left in place -- nothing is copied out in between -- all in one arena run."""
    c = strict.chained_case()
    r, levels = c["loss"], c["levels"]
    L = lib.lib()
    B = r["B"]
    hl0, hg0 = lib.HeadLayers(), lib.HeadGrads()
    hl0.levels = hg0.levels = len(levels)
    for i, l in enumerate(levels):
        hl0.H[i], hl0.W[i], hl0.Cin[i], hl0.cout[i] = l["H"], l["W"], l["Cin"], l["cout"]
        hg0.hw[i], hg0.per_cell[i], hg0.npad[i] = l["H"] * l["W"], r["levels"][i]["n"], l["npad"]
    lb = L.ssd_loss_heads_workspace_bytes(B, r["A"], r["C"])
    zb = L.ssd_heads_bwd_data_sparse_workspace_bytes(B, ctypes.byref(hl0))
    wb = L.ssd_heads_bwd_weight_sparse_workspace_bytes(B, ctypes.byref(hg0), ctypes.byref(hl0))
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[nbytes(r[k]) for k in INPUTS], *HeadBuffers.bytes(r), *Layers.bytes(levels), lb, zb, wb))
    inp = put_inputs(a, r)
    out8 = a.out((8,), F32, "out8")
    hb = HeadBuffers(a, lib, r)
    hl = Layers(a, lib, B, levels, "bits")
    ws = a.workspace()
    lws, zws, wws = ws.get(lb, "cuda"), ws.get(zb, "cuda"), ws.get(wb, "cuda")

    def fn():
        heads_call(L, inp, r, out8, hb, lws, lb, 0)
        assert L.ssd_heads_bwd_data_sparse(ctypes.byref(hb.c), ctypes.byref(hl.c), B, ptr(zws), zb, stream()) == 0
        assert L.ssd_heads_bwd_weight_sparse(ctypes.byref(hb.c), ctypes.byref(hl.c), B, ptr(wws), wb, stream()) == 0
    expect = [(out8, r["out8"])] + hb.expect(r)
    for i, l in enumerate(levels):
        expect += [(hl.dx[i], l["dx"].to(BF)), (hl.dw[i], l["dw"]), (hl.db[i], l["dbias"])]
    a.run(fn, expect)
