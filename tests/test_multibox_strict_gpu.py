"""GPU: the MultiBox loss under the strict harness (tests/strict.py), both forms, through the C ABI.

The cases of tests/multibox_cases.py are exact (one maximum per row, every other logit at most m - 1024, offsets multiples of
1/4, P / loc_weight / grad_scale powers of two; tests/test_multibox_cpu.py asserts the regime): out8, dconf, dloc, the counts,
both index maps and the rows are compared bit for bit.  Inputs, outputs and a workspace of exactly
ssd_multibox_loss_workspace_bytes live in strict.Arena, run under both poisons: a store outside the documented extent (rows or
pixel_of_row past count[l], count[levels..7]), an element never written, a modified input or a read of unwritten workspace are
all failures."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import multibox_cases as K                                                            # noqa: E402
from tests import strict                                                                         # noqa: E402
from tests.test_loss_strict_gpu import HeadBuffers, INPUTS, nbytes, ptr, put_inputs, scatter, stream   # noqa: E402

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def lib():
    from ssd_object_detection_amd import _lib
    return _lib


def run_dense(lib, r):
    L = lib.lib()
    B, A, C, dt = r["B"], r["A"], r["C"], r["dtype"]
    ws_bytes = L.ssd_multibox_loss_workspace_bytes(B, A, C)
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[nbytes(r[k]) for k in INPUTS], 32, nbytes(r["dconf"]), nbytes(r["dloc"]), ws_bytes))
    conf, loc, cls, gloc, mask = put_inputs(a, r)
    out8, dconf, dloc = a.out((8,), F32, "out8"), a.out((B, A, C), dt, "dconf"), a.out((B, A, 4), dt, "dloc")
    ws = a.workspace().get(ws_bytes, "cuda")

    def fn():
        st = L.ssd_multibox_loss_fwd_bwd(ptr(conf), ptr(loc), 0 if dt == F32 else 1, ptr(cls), ptr(gloc), ptr(mask), B, A, C,
                                         r["ratio"], r["alpha"], r["grad_scale"], ptr(out8), ptr(dconf), ptr(dloc), ptr(ws),
                                         ws_bytes, stream())
        assert st == 0, st
    return a.run(fn, [(out8, r["out8"]), (dconf, r["dconf"]), (dloc, r["dloc"])])


DENSE = {
    "ranks: first / middle / last of a tie group; tau_b differ in high, middle, low bits f32": K.ranks_case,
    "ties across a 128-row block boundary f32": lambda: K.boundary_case(F32),
    "ties across a 128-row block boundary bf16 gs=0.25 alpha=0.5": lambda: K.boundary_case(BF, alpha=0.5, gs=0.25),
    "ties across a 128-row block boundary C=21 f32": lambda: K.boundary_case(F32, C=21),
    "every candidate mined, tau_b = 0 f32": lambda: K.saturated_case(F32),
    "every candidate mined, tau_b = 0 bf16": lambda: K.saturated_case(BF),
    "no positive: status 1 f32": lambda: K.empty_case(F32),
    "no positive: status 1 bf16": lambda: K.empty_case(BF),
}


@pytest.mark.parametrize("name", sorted(DENSE), ids=str)
def test_dense_exact(lib, name):
    """out8[0..7], dconf and dloc of ssd_multibox_loss_fwd_bwd, bit for bit"""
    r = K.cached(name, DENSE[name])
    out8, _, _ = run_dense(lib, r)
    assert float(out8[7]) == r["status"]


@pytest.mark.parametrize("name", sorted(K.HEADS_CASES), ids=str)
def test_rows_exact(lib, ops, name):
    """count, both maps, the rows and out8 of ssd_multibox_loss_fwd_bwd_heads, bit for bit, nothing written past count[l] rows
    or past count[levels - 1]; then the rows scattered back against ssd_multibox_loss_fwd_bwd on the same inputs"""
    L = lib.lib()
    r = K.cached(name, K.HEADS_CASES[name])
    B, A, C = r["B"], r["A"], r["C"]
    ws_bytes = L.ssd_multibox_loss_heads_workspace_bytes(B, A, C)
    a = strict.Arena("cuda", strict.Arena.bytes_for(*[nbytes(r[k]) for k in INPUTS], *HeadBuffers.bytes(r), ws_bytes))
    inp = put_inputs(a, r)
    out8 = a.out((8,), F32, "out8")
    hb = HeadBuffers(a, lib, r)
    ws = a.workspace().get(ws_bytes, "cuda")

    def fn():
        st = L.ssd_multibox_loss_fwd_bwd_heads(ptr(inp[0]), ptr(inp[1]), 1, ptr(inp[2]), ptr(inp[3]), ptr(inp[4]), B, A, C,
                                               r["ratio"], r["alpha"], r["grad_scale"], ptr(out8), ctypes.byref(hb.c), ptr(ws),
                                               ws_bytes, stream())
        assert st == 0, st
    got = a.run(fn, [(out8, r["out8"])] + hb.expect(r))
    counts = [l["count"] for l in r["levels"]]
    for i, l in enumerate(r["levels"]):                                 # (implied by the expectation; stated for the reader)
        por, rop = got[2 + 3 * i + 1][:counts[i]], got[2 + 3 * i]
        assert bool((por[1:] > por[:-1]).all()) and torch.equal(rop[por.long()], torch.arange(counts[i], dtype=I32, device="cuda"))
        assert int((rop == -1).sum()) == rop.numel() - counts[i]
    out_d, dconf, dloc = ops.multibox_loss(inp[0], inp[1], inp[2], inp[3], inp[4], r["ratio"], r["alpha"], r["grad_scale"])
    assert torch.equal(out_d.view(I32), got[0].view(I32))
    sl, sc = scatter(r, [got[2 + 3 * i + 2] for i in range(len(counts))], [got[2 + 3 * i + 1] for i in range(len(counts))], counts)
    assert torch.equal(sl.view(torch.int16), dloc.view(torch.int16)) and torch.equal(sc.view(torch.int16), dconf.view(torch.int16))


def test_rows_cover_the_designed_situations():
    """over the catalogue: a level with no selected pixel, an image with none, a level where every pixel is selected"""
    seen = set()
    for name in K.HEADS_CASES:
        r = K.cached(name, K.HEADS_CASES[name])
        P_b = r["gt_mask"].sum(1).tolist()
        for l in r["levels"]:
            seen.add("empty level" if l["count"] == 0 else "")
            seen.add("full level" if l["count"] == sum(1 for p in P_b if p) * l["hw"] else "")
        seen.add("empty image" if 0 in P_b else "")
    assert {"empty level", "full level", "empty image"} <= seen
