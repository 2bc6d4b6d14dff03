"""CPU suite: the slice arithmetic of the MX-fp8 operand stores (ssd_object_detection_amd/mx.py).  A FlatStore adopts CPU
buffers whose bytes tell their own position, and every fp8 layer's (q, scale) view of both planned engines is compared with the
elements the tensor table says it must hold -- re-derived here from names, offsets and blocks alone."""
import pytest

torch = pytest.importorskip("torch")

from ssd_object_detection_amd import mx                               # noqa: E402
from ssd_object_detection_amd.engine import SSDEngine                 # noqa: E402
from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine  # noqa: E402

P = 251                                       # byte i holds i % P (P prime: a slice shifted by less than P bytes shows)


def positions(lo, hi):
    return (torch.arange(lo, hi) % P).to(torch.uint8)


def indexed_store(n):
    """A store over n elements whose q byte i is i % P and whose scale byte j is j % P."""
    return mx.FlatStore().adopt(positions(0, n), positions(0, n // 32))


def check_view(pair, start, shape, what):
    """pair = the view of a tensor of `shape` that starts `start` elements into the stored range."""
    q, sc = pair
    n = 1
    for d in shape:
        n *= d
    assert tuple(q.shape) == tuple(shape) and tuple(sc.shape) == tuple(shape[:-1]) + (shape[-1] // 32,), what
    assert q.is_contiguous() and sc.is_contiguous(), what
    assert q.storage_offset() == start and sc.storage_offset() == start // 32, what      # (a shift by a multiple of P as well)
    assert torch.equal(q.reshape(-1), positions(start, start + n)), what
    assert start % 32 == 0 and torch.equal(sc.reshape(-1), positions(start // 32, (start + n) // 32)), what


def test_pair():
    q, sc = mx.pair((2, 5, 7, 96), "cpu")
    assert q.dtype == sc.dtype == torch.uint8 and q.shape == (2, 5, 7, 96) and sc.shape == (2, 5, 7, 3)
    with pytest.raises(AssertionError):
        mx.pair((2, 5, 7, 48), "cpu")


def test_store_is_lazy_and_refuses_bad_slices():
    s = mx.FlatStore()
    assert not s.allocated
    s = indexed_store(64 * 40)
    assert s.allocated
    check_view(s.view(64, (3, 1, 1, 64)), 64, (3, 1, 1, 64), "plain")
    check_view(s.view(64 * 39, (1, 64)), 64 * 39, (1, 64), "the last tensor of the range")
    with pytest.raises(AssertionError):
        s.view(16, (3, 1, 1, 64))                                     # not on a 32-element block
    with pytest.raises(AssertionError):
        s.view(64 * 39, (2, 64))                                      # runs past the range
    with pytest.raises(AssertionError):
        s.view(0, (4, 48))                                            # rows that are no whole blocks
    with pytest.raises(AssertionError):
        mx.FlatStore().adopt(positions(0, 64), positions(0, 3))       # scale is not one byte per 32


def filter_range(eng, fp8):
    """(lo, hi) of the flat buffers that holds the filters of nodes fp8, from the tensor table: the first kernel's offset up
    to the end of the last optimizer block of any of their variables."""
    byname = {t.name: t for t in eng.tensors}
    mine = [byname["conv%d/%s" % (i, part)] for i in fp8 for part in ("kernel", "bias")]
    return byname, min(t.offset for t in mine), max(t.block0 + t.nblocks for t in mine) * eng.block


def test_ssd300_filter_views():
    eng = SSDEngine.planned()
    fp8 = eng.vgg_mxfp8_plan()[0]
    byname, lo, hi = filter_range(eng, fp8)
    assert len(fp8) == 10 and eng._mx_range == (lo, hi) and lo > 0
    eng.mx_filters.adopt(positions(0, hi - lo), positions(0, (hi - lo) // 32))
    for i in sorted(fp8):
        t, nd = byname["conv%d/kernel" % i], eng.nodes[i]
        assert t.shape == (nd["cout"], nd["k"], nd["k"], nd["cin"])
        check_view(eng.mxfp8_weights(i), t.offset - lo, t.shape, "SSD300 node %d" % i)


def test_resnet_filter_views():
    eng = ResNet50SSDEngine.planned()
    assert len(eng.mx_fp8) == 44
    byname, lo, hi = filter_range(eng, [i for i, nd in enumerate(eng.nodes) if nd["kind"] == "conv"])
    assert lo == 0 and eng._mx_range == (0, hi)
    eng.mx_filters.adopt(positions(0, hi), positions(0, hi // 32))
    for i in sorted(eng.mx_fp8):
        t, nd = byname["conv%d/kernel" % i], eng.nodes[i]
        assert t.shape == (nd["cout"], nd["k"], nd["k"], nd["cin"])
        check_view(eng.mxfp8_weights(i), t.offset, t.shape, "ResNet node %d" % i)


def test_resnet_transposed_filter_views():
    """w_t order: the fp8 data gradients' transposed filters first, each group by node index; the store covers the front."""
    eng = ResNet50SSDEngine.planned()
    convs = [i for i, nd in enumerate(eng.nodes) if nd["kind"] == "conv" and i > 0]
    order = sorted(i for i in convs if i in eng.mx_dgrad) + sorted(i for i in convs if i not in eng.mx_dgrad)
    start, off = {}, 0
    for i in order:
        nd = eng.nodes[i]
        start[i] = off
        off += nd["cin"] * nd["k"] * nd["k"] * nd["cout"]
    front = sum(eng.nodes[i]["cin"] * eng.nodes[i]["k"] ** 2 * eng.nodes[i]["cout"] for i in eng.mx_dgrad)
    assert eng.mx_dgrad and eng.wt_off == start and eng.n_wt8 == front and eng.n_wt == off
    eng.mx_filters_t.adopt(positions(0, front), positions(0, front // 32))
    for i in sorted(eng.mx_dgrad):
        nd = eng.nodes[i]
        check_view(eng.mxfp8_wt(i), start[i], (nd["cin"], nd["k"], nd["k"], nd["cout"]), "ResNet data gradient %d" % i)
    last = max(eng.mx_dgrad)
    assert start[last] + eng.nodes[last]["cin"] * eng.nodes[last]["k"] ** 2 * eng.nodes[last]["cout"] == front
