"""CPU suite: the plan of the SSD300 VGG trunk's inference fp8 forward (engine.mxfp8_vgg_plan) and the host-side refusals of
its pooled C entry point (ssd_conv2d_fwd_pool_mxfp8) -- no device is touched."""
import ctypes

import pytest


def _nodes(trunk, size):
    """The engine's planned nodes and chain start for a trunk, without allocating anything."""
    from ssd_object_detection_amd import engine as E
    eng = E.SSDEngine.__new__(E.SSDEngine)
    eng.trunk, eng.in_size, eng.sparse_heads = list(trunk), size, True
    eng.num_priors = E.SSD300_NUM_PRIORS if size == 300 else E.SSD512_NUM_PRIORS
    eng._plan_shapes()
    return eng.nodes, eng.chain_start


def _plan(trunk="300"):
    from ssd_object_detection_amd import engine as E
    nodes, cs = _nodes(E.SSD300_TRUNK, 300) if trunk == "300" else _nodes(E.SSD512_TRUNK, 512)
    return nodes, cs, *E.mxfp8_vgg_plan(nodes, cs)


B, F, BF, NONE = frozenset({"bf16"}), frozenset({"fp8"}), frozenset({"bf16", "fp8"}), frozenset()


def test_ssd300_plan():
    nodes, cs, fp8, pooled, quant, writes = _plan()
    assert cs == 17 and len(nodes) == 23
    assert fp8 == {6, 7, 8, 10, 11, 12, 13, 14, 15, 16}
    # block3_conv3 + the SAME 75 -> 38 pool: one pooled fp8 launch that stores the pooled fp8 map only
    assert pooled == {9} and nodes[9]["kind"] == "pool" and nodes[9]["hin"] == 75 and nodes[9]["hout"] == 38
    assert writes[8] == NONE and writes[9] == F
    # the ONE standalone quantise: block2's pooled map (75x75x128), which its bf16 pool_only launch writes
    assert quant == {5} and (nodes[5]["hout"], nodes[5]["cout"]) == (75, 128) and writes[5] == BF
    # the front stays as today
    assert all(writes[i] == B for i in range(5))
    # feature maps 0 and 1 feed their head and the next fp8 layer; feature map 2 feeds its head and the bf16 chain
    assert writes[12] == BF and writes[14] == BF and writes[16] == B
    for i in (6, 7, 10, 11, 13, 15):
        assert writes[i] == F, i
    # the chain and every head stay bf16
    assert all(writes[i] == B for i in range(cs, len(nodes)))
    assert all(i < cs for i in fp8)


def test_ssd300_plan_covers_two_thirds_of_the_trunk():
    nodes, _, fp8, _, _, _ = _plan()
    macs = {i: nd["hout"] ** 2 * nd["cout"] * nd["k"] ** 2 * nd["cin"] for i, nd in enumerate(nodes) if nd["kind"] == "conv"}
    share = sum(macs[i] for i in fp8) / sum(macs.values())
    assert 0.63 <= share <= 0.67, share
    # block2_conv2 is eligible, but fp8 there would quantise its 150x150x128 input: larger than block3_conv1's
    assert nodes[4]["cin"] == 128 and 4 not in fp8


@pytest.mark.parametrize("trunk", ["300", "512"])
def test_plan_is_self_consistent(trunk):
    nodes, cs, fp8, pooled, quant, writes = _plan(trunk)
    assert len(quant) == 1
    for i, nd in enumerate(nodes):
        if i == 0:
            continue
        # the reader of node i - 1's map: a fused pool reads it in registers, an fp8 layer the fp8 form, the rest bf16
        if i in pooled:
            assert i - 1 in fp8 and nd["kind"] == "pool" and nodes[i - 1]["k"] == 3 and nodes[i - 1]["stride"] == 1
            assert writes[i - 1] == NONE
        elif i in fp8:
            assert "fp8" in writes[i - 1], i
            assert (i - 1) in fp8 or (i - 1) in pooled or (i - 1) in quant, "fp8 reader %d has no fp8 writer" % i
        else:
            assert "bf16" in writes[i - 1], i
    for i, w in writes.items():
        assert w or (i in fp8 and i + 1 in pooled), "node %d has no consumer" % i
        if nodes[i]["feature"]:
            assert "bf16" in w, i
    for i in fp8:
        nd = nodes[i]
        assert nd["kind"] == "conv" and nd["cin"] % 128 == 0 and nd["cout"] % 32 == 0 and i < cs
    assert all(writes[i] == B for i in range(cs, len(nodes)))


def test_ssd512_plan():
    nodes, cs, fp8, pooled, quant, writes = _plan("512")
    # the same first 13 nodes as SSD300 at 512: the same front, one more 3x3/2 stage before the chain
    assert fp8 == {6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 18} and cs == 19
    assert pooled == {9} and quant == {5} and nodes[9]["hout"] == 64
    assert writes[16] == BF and writes[18] == B


def _lib():
    from ssd_object_detection_amd import _lib as L
    return L, L.lib()


def test_conv2d_fwd_pool_mxfp8_refuses_on_the_host():
    L, lib = _lib()
    d = ctypes.c_void_p(0x1000)                                       # never dereferenced on these paths

    def call(y=d, y8=None, ys=None, B=2, H=16, W=16, Cin=256, Cout=256, k=3, s=1, pt=1, pl=1, Ho=16, Wo=16, Hp=8, Wp=8, x8=d,
             w8=d):
        return lib.ssd_conv2d_fwd_pool_mxfp8(x8, d, w8, d, None, y, y8, ys, B, H, W, Cin, Cout, k, s, pt, pl, Ho, Wo, 1, Hp, Wp,
                                             None)

    assert call(y=None) == L.SSD_ERR_VALUE                           # no output
    assert call(y8=d) == L.SSD_ERR_VALUE                             # q without its scales
    assert call(ys=d) == L.SSD_ERR_VALUE
    assert call(y=None, ys=d) == L.SSD_ERR_VALUE
    assert call(x8=None) == L.SSD_ERR_VALUE
    assert call(w8=None) == L.SSD_ERR_VALUE
    assert call(B=0) == L.SSD_ERR_VALUE
    assert call(Ho=0) == L.SSD_ERR_VALUE
    assert call(pt=-1) == L.SSD_ERR_VALUE
    assert call(pt=3) == L.SSD_ERR_VALUE                             # pads of a 3x3 window
    assert call(Ho=20, Hp=10) == L.SSD_ERR_VALUE                     # windows beyond the map
    assert call(Hp=7) == L.SSD_ERR_VALUE                             # neither VALID nor SAME pooling of 16
    assert call(Wp=9) == L.SSD_ERR_VALUE
    assert call(Hp=0) == L.SSD_ERR_VALUE
    assert call(k=1, pt=0, pl=0) == L.SSD_ERR_UNSUPPORTED
    assert call(s=2, Ho=8, Wo=8, Hp=4, Wp=4) == L.SSD_ERR_UNSUPPORTED
    assert call(Cin=64) == L.SSD_ERR_UNSUPPORTED
    assert call(Cin=192) == L.SSD_ERR_UNSUPPORTED
    assert call(Cout=48) == L.SSD_ERR_UNSUPPORTED                    # whole 32-channel blocks, bf16 output too
    assert call(Cout=48, y=None, y8=d, ys=d) == L.SSD_ERR_UNSUPPORTED
    assert call(B=64, H=256, W=256, Cin=512, Ho=256, Wo=256, Hp=128, Wp=128) == L.SSD_ERR_UNSUPPORTED    # 2^31-byte operand
    # odd maps: both pooled sizes pass the host checks (refused here only by the Cout % 32 rule behind them)
    assert call(H=75, W=75, Ho=75, Wo=75, Hp=38, Wp=37, Cout=40) == L.SSD_ERR_UNSUPPORTED
