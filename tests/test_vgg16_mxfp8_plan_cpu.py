"""CPU suite: the plan of the VGG-16 SSD300's inference fp8 forward (engine.mxfp8_trunk_plan: quantising poolings, the dilated
fc6 in fp8), the construction switch that turns it on, its YAML key, and the host-side refusals of the three entry points it
launches -- no device is touched."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
yaml = pytest.importorskip("yaml")

B, F, BF, NONE = frozenset({"bf16"}), frozenset({"fp8"}), frozenset({"bf16", "fp8"}), frozenset()


@pytest.fixture(scope="module")
def E():
    from ssd_object_detection_amd import engine
    return engine


def vgg16(E, size=300, **kw):
    trunk, pri = (E.VGG16_SSD300_TRUNK, E.VGG16_SSD300_NUM_PRIORS) if size == 300 else (E.VGG16_SSD300_TRUNK[:-2], E.VGG16_SSD300_NUM_PRIORS[:5])
    return E.SSDEngine.planned(81, size, trunk, pri, **kw)


def test_plan_at_300(E):
    e = vgg16(E, fp8_inference=True)
    assert e.chain_start == 22 and not e.bf16_only
    p = E.mxfp8_trunk_plan(e.nodes, e.chain_start)
    assert p.fp8 == {6, 7, 8, 10, 11, 12, 14, 15, 16, 18, 19, 20, 21}
    assert p.pooled == {9} and p.qpool == {13, 17} and p.quant == {5}
    assert (e.nodes[13]["kind"], e.nodes[17]["kind"], e.nodes[18]["dilation"]) == ("pool", "pool3s1", 6)
    want = {12: B, 13: F, 16: B, 17: F, 18: F, 19: BF, 20: F, 21: B}
    assert {i: p.writes[i] for i in want} == want
    # the front is the default trunk's: the pooled block3_conv3 launch, the one standalone quantise of block2's pooled map
    assert p.writes[8] == NONE and p.writes[9] == F and p.writes[5] == BF and all(p.writes[i] == B for i in range(5))
    assert all(p.writes[i] == B for i in range(e.chain_start, len(e.nodes)))
    # the engine's accessors: the named plan, its 4-tuple, and the filters' stretch of param_bf16 over every fp8 node
    assert e.mxfp8_plan() == p and e.vgg_mxfp8_plan() == (p.fp8, p.pooled, p.quant, p.writes)
    assert E.mxfp8_vgg_plan(e.nodes, e.chain_start) == (p.fp8, p.pooled, p.quant, p.writes)
    lo, hi = e._mx_range
    for i in p.fp8:
        wt = e.conv_params[i][0]
        assert lo <= wt.offset and wt.offset + wt.numel <= hi and (wt.offset - lo) % 32 == 0


@pytest.mark.parametrize("size", [300, 174, 164])
def test_plan_structure(E, size):
    """What the walk relies on, wherever the chain starts (174: chain from node 22 on 6x6 maps; 164: pool4 is VALID of an odd map)."""
    e = vgg16(E, size, fp8_inference=True)
    nodes, cs = e.nodes, e.chain_start
    p = e.mxfp8_plan()
    end = len(nodes) if cs is None else cs
    assert len(p.quant) == 1 and min(p.fp8) == next(iter(p.quant)) + 1 and 18 in p.fp8
    for i in p.fp8:
        assert E.mxfp8_eligible(nodes[i]) and i < end, i
    run = range(min(p.fp8), end)
    for i in run:
        kind = nodes[i]["kind"]
        assert (kind == "conv") == (i in p.fp8)
        assert (kind in ("pool", "pool3s1")) == ((i in p.pooled) != (i in p.qpool)) and not (i in p.pooled and i in p.qpool)
    assert not (p.pooled | p.qpool) - set(run)
    for i in p.pooled:                                   # inside the launch of a 3x3 / stride-1 convolution that no head reads
        nd = nodes[i - 1]
        assert nodes[i]["kind"] == "pool" and (nd["k"], nd["stride"], nd["dilation"], nd["feature"]) == (3, 1, 1, False)
        assert p.writes[i - 1] == NONE
    for i in p.qpool:                                    # reads the bf16 map in front of it, is its own quantiser
        assert "bf16" in p.writes[i - 1] and "fp8" in p.writes[i] and (i - 1) in p.fp8
        assert nodes[i]["kind"] == "pool3s1" or nodes[i - 1]["feature"] or nodes[i - 1]["k"] != 3 or nodes[i - 1]["stride"] != 1
    assert all(i in p.qpool for i in run if nodes[i]["kind"] == "pool3s1")
    for i, nd in enumerate(nodes):
        if nd["feature"]:
            assert "bf16" in p.writes[i], i
        if i > 0 and i not in p.pooled:                  # every reader finds the form it reads
            assert ("fp8" if i in p.fp8 else "bf16") in p.writes[i - 1], i
        if "fp8" in p.writes[i]:                         # no standalone activation quantise but the one
            assert i in p.fp8 or i in p.pooled or i in p.qpool or i in p.quant, i
    assert all(p.writes[i] == B for i in range(end, len(nodes)))


def test_eligibility_of_dilated_nodes(E):
    nd = dict(kind="conv", cin=512, cout=1024, k=3, stride=1, dilation=6)
    assert E.mxfp8_eligible(nd) and E.mxfp8_eligible(dict(nd, dilation=1))
    assert not E.mxfp8_eligible(dict(nd, stride=2)) and not E.mxfp8_eligible(dict(nd, k=1)) and not E.mxfp8_eligible(dict(nd, cin=64))
    assert E.mxfp8_eligible(dict(op="conv", cin=256, cout=64, k=1, stride=2))          # a ResNet graph node: no such key


def test_default_trunk_plan_is_unchanged(E):
    for switch in (False, True):                         # no effect on a trunk that has its plan anyway
        e = E.SSDEngine.planned(fp8_inference=switch)
        assert not e.bf16_only
        fp8, pooled, quant, writes = e.vgg_mxfp8_plan()
        assert fp8 == {6, 7, 8, 10, 11, 12, 13, 14, 15, 16} and pooled == {9} and quant == {5}
        p = E.mxfp8_trunk_plan(e.nodes, e.chain_start)
        assert (p.fp8, p.pooled, p.quant, p.writes) == (fp8, pooled, quant, writes) == E.mxfp8_vgg_plan(e.nodes, e.chain_start)
        assert p.qpool == set()
        assert writes[8] == NONE and writes[9] == F and writes[5] == BF and writes[12] == BF and writes[14] == BF and writes[16] == B
    a, b = E.SSDEngine.planned(), E.SSDEngine.planned(fp8_inference=True)
    assert [(t.name, t.shape, t.offset) for t in a.tensors] == [(t.name, t.shape, t.offset) for t in b.tensors]


def test_without_the_switch_the_vgg16_stays_bf16_only(E):
    e = vgg16(E)
    assert e.bf16_only and not e.fp8_inference
    s = vgg16(E, fp8_inference=True)
    assert not s.bf16_only and s.fp8_inference
    assert [(t.name, t.shape, t.offset) for t in e.tensors] == [(t.name, t.shape, t.offset) for t in s.tensors]
    assert e.nodes == s.nodes and e.chain_start == s.chain_start


def test_yaml_key_and_model_switch():
    from ssd_object_detection_amd.tools import train as T
    assert T.fp8_inference_from_config(yaml.safe_load("model: {network: {kind: vgg16_ssd300}, fp8_inference: true}")) is True
    assert T.fp8_inference_from_config(yaml.safe_load("model: {fp8_inference: false}")) is False
    assert T.fp8_inference_from_config(yaml.safe_load("model: {network: {kind: vgg16_ssd300}}")) is False
    assert T.fp8_inference_from_config({}) is False
    for bad in ("model: {fp8_inference: 1}", "model: {fp8_inference: 'yes'}", "model: {fp8_inference: {enable: true}}",
                "model: {fp8_inference: null}"):
        with pytest.raises(ValueError, match="fp8_inference"):
            T.fp8_inference_from_config(yaml.safe_load(bad))
    # the switch is no field of the network spec: a checkpoint's identity does not know it
    import ssd_object_detection_amd.ops as ops
    assert "fp8_inference" not in ops.NetworkSpec.FIELDS
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    with pytest.raises(ValueError, match="fp8_inference"):               # before any engine is built
        SSDObjectDetectionModel(20, "unused", device="cpu", timestamp_dir=False, network="resnet50_ssd512", fp8_inference=True)
    with pytest.raises(ValueError, match="fp8_inference"):
        SSDObjectDetectionModel(20, "unused", device="cpu", timestamp_dir=False, network="vgg16_ssd300", fp8_inference="yes")


def _lib():
    from ssd_object_detection_amd import _lib as L
    return L, L.lib()


def test_atrous_fwd_mxfp8_refuses_on_the_host():
    L, lib = _lib()
    d = ctypes.c_void_p(0x1000)                                       # never dereferenced on these paths

    def call(y=d, y8=None, ys=None, B=2, H=19, W=19, Cin=512, Cout=1024, dil=6, x8=d, xs=d, w8=d, ws=d):
        return lib.ssd_conv2d_atrous_fwd_mxfp8(x8, xs, w8, ws, None, y, y8, ys, B, H, W, Cin, Cout, dil, 1, None)

    assert call(y=None) == L.SSD_ERR_VALUE                           # no output
    assert call(y8=d) == L.SSD_ERR_VALUE and call(ys=d) == L.SSD_ERR_VALUE          # q without its scales, and the reverse
    for missing in ("x8", "xs", "w8", "ws"):
        assert call(**{missing: None}) == L.SSD_ERR_VALUE
    assert call(B=0) == L.SSD_ERR_VALUE and call(H=0) == L.SSD_ERR_VALUE and call(dil=0) == L.SSD_ERR_VALUE
    assert call(Cin=64) == L.SSD_ERR_UNSUPPORTED and call(Cin=192) == L.SSD_ERR_UNSUPPORTED
    assert call(Cout=1020) == L.SSD_ERR_UNSUPPORTED
    assert call(Cout=40, y=None, y8=d, ys=d) == L.SSD_ERR_UNSUPPORTED               # whole 32-channel blocks for an fp8 output
    assert call(B=64, H=256, W=256) == L.SSD_ERR_UNSUPPORTED                        # a 2^31-byte operand
    assert call(B=1024, H=38, W=38, Cin=128, Cout=1024) == L.SSD_ERR_UNSUPPORTED    # a 2^31-byte bf16 output


def test_quantising_poolings_refuse_on_the_host():
    L, lib = _lib()
    d, q, s = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x4000000), ctypes.c_void_p(0x8000000)

    def p2(x=d, y=None, q=q, s=s, B=2, H=38, W=38, C=512, Ho=19, Wo=19):
        return lib.ssd_maxpool2x2_fwd_mxfp8(x, y, q, s, B, H, W, C, Ho, Wo, None)

    def p3(x=d, y=None, q=q, s=s, B=2, H=19, W=19, C=512):
        return lib.ssd_maxpool3x3s1_fwd_mxfp8(x, y, q, s, B, H, W, C, None)

    for f in (p2, p3):
        assert f(x=None) == L.SSD_ERR_VALUE and f(q=None) == L.SSD_ERR_VALUE and f(s=None) == L.SSD_ERR_VALUE
        assert f(B=0) == L.SSD_ERR_VALUE and f(C=0) == L.SSD_ERR_VALUE
        assert f(C=24) == L.SSD_ERR_UNSUPPORTED and f(C=48) == L.SSD_ERR_UNSUPPORTED
        assert f(q=d) == L.SSD_ERR_VALUE                              # the output on top of the input
    assert p2(Ho=18) == L.SSD_ERR_VALUE and p2(Wo=20) == L.SSD_ERR_VALUE and p2(H=1, W=1, Ho=0, Wo=0) == L.SSD_ERR_VALUE
    assert p2(B=4096, H=64, W=64, C=128, Ho=32, Wo=32) == L.SSD_ERR_UNSUPPORTED     # 2^31 elements
    assert p3(B=4096, H=64, W=64, C=128) == L.SSD_ERR_UNSUPPORTED
