"""CPU suite: the VGG-16 SSD300 graph as planned (engine.VGG16_SSD300_TRUNK through SSDEngine.planned: no device), its network
spec and YAML block, and the test oracle of its backward pass against torch.autograd on a small geometry."""
import os

import pytest

torch = pytest.importorskip("torch")
yaml = pytest.importorskip("yaml")


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def E():
    from ssd_object_detection_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ the graph
def test_trunk_keeps_the_ends_of_the_ssd300_trunk(E):
    t = E.VGG16_SSD300_TRUNK
    assert len(t) == 28 and t[:10] == E.SSD300_TRUNK[:10] and t[-8:] == E.SSD300_TRUNK[-8:] == E.SSD300_TRUNK[15:]
    assert E.VGG16_SSD300_NUM_PRIORS == (4, 6, 6, 6, 4, 4)
    # the existing trunks are untouched 7-tuples
    for trunk in (E.SSD300_TRUNK, E.SSD512_TRUNK):
        for kind, cin, cout, k, stride, mode, feat in trunk:
            assert kind in ("conv", "pool")
    assert len(E.SSD300_TRUNK) == 23 and len(E.SSD512_TRUNK) == 25
    # only fc6 carries an eighth element
    assert [i for i, n in enumerate(t) if len(n) != 7] == [18] and t[18] == ("conv", 512, 1024, 3, 1, "same", False, 6)
    assert [n[0] for n in t[10:20]] == ["conv"] * 3 + ["pool"] + ["conv"] * 3 + ["pool3s1", "conv", "conv"]
    assert [i for i, n in enumerate(t) if n[6]] == [12, 19, 21, 23, 25, 27]


def test_planned_geometry_at_300(E):
    e = E.SSDEngine.planned(81, 300, E.VGG16_SSD300_TRUNK, E.VGG16_SSD300_NUM_PRIORS)
    assert e.grids == tuple((h, h) for h in (38, 19, 10, 5, 3, 1)) and e.A == 8732
    assert e.level_off == [0, 5776, 7942, 8542, 8692, 8728, 8732]
    assert [(ni, h, c) for ni, h, c in e.fm] == [(12, 38, 512), (19, 19, 1024), (21, 10, 512), (23, 5, 256), (25, 3, 256), (27, 1, 256)]
    geo = {i: (nd["hin"], nd["hout"], nd["pt"], nd["dilation"]) for i, nd in enumerate(e.nodes)}
    assert geo[9] == (75, 38, 0, 1)                                     # the SAME pooling, as in SSD300_TRUNK
    assert geo[10] == geo[11] == geo[12] == (38, 38, 1, 1)              # conv4_1 .. conv4_3
    assert geo[13] == (38, 19, 0, 1)                                    # pool4, VALID
    assert geo[14] == geo[15] == geo[16] == (19, 19, 1, 1)              # conv5_1 .. conv5_3
    assert geo[17] == (19, 19, 1, 1) and e.nodes[17]["kind"] == "pool3s1"
    assert geo[18] == (19, 19, 6, 6) and e.nodes[18]["pl"] == 6         # fc6: dilation 6, padding 6
    assert geo[19] == (19, 19, 0, 1) and e.nodes[19]["k"] == 1          # fc7
    assert [geo[i][:2] for i in range(20, 28)] == [(19, 19), (19, 10), (10, 10), (10, 5), (5, 5), (5, 3), (3, 3), (3, 1)]
    assert (e.nodes[23]["pt"], e.nodes[21]["pt"]) == (0, 1)             # Keras SAME at stride 2: 10 -> 5 pads bottom / right only
    assert all(nd["dilation"] == 1 for i, nd in enumerate(e.nodes) if i != 18)
    assert e.chain_start == 22 and e.bf16_only and e.first_pair
    # parameters are named by node; the l2norm scale, where asked for, follows every other tensor
    names = [t.name for t in e.tensors]
    assert names[:2] == ["conv0/kernel", "conv0/bias"] and "conv18/kernel" in names and "conv13/kernel" not in names and "conv17/kernel" not in names
    assert e.conv_params[18][0].shape == (1024, 3, 3, 512) and e.conv_params[19][0].shape == (1024, 1, 1, 1024)
    assert len(names) == 2 * 23 + 4 * 6                                 # 28 nodes, five of them poolings; six levels
    n = E.SSDEngine.planned(81, 300, E.VGG16_SSD300_TRUNK, E.VGG16_SSD300_NUM_PRIORS, l2norm=True)
    assert [t.name for t in n.tensors] == names + ["l2norm0/scale"] and n.l2norm_scale.shape == (512,)
    # the optimizer buckets cover every tensor once, heads first, and each is gated by a convolution
    b = e.opt_buckets()
    assert b[0][2] is None and sorted(t for t0, t1, _ in b for t in range(t0, t1)) == list(range(len(names)))
    assert all(e.nodes[node]["kind"] == "conv" for _, _, node in b[1:])
    assert e.bucket_gates([(t0, t1) for t0, t1, _ in b]) == [node for _, _, node in b]
    assert e.decay_table(5e-4).tolist() == [pytest.approx(5e-4) if nm.endswith("kernel") else 0.0 for nm in names]


def test_reduced_geometries(E):
    for size, grids, pools in ((174, (22, 11, 6, 3, 1), [(174, 87), (87, 43), (43, 22), (22, 11), (11, 11)]),
                               (164, (21, 10, 5, 3, 1), [(164, 82), (82, 41), (41, 21), (21, 10), (10, 10)])):
        e = E.SSDEngine.planned(81, size, E.VGG16_SSD300_TRUNK[:-2], E.VGG16_SSD300_NUM_PRIORS[:5])
        assert e.grids == tuple((h, h) for h in grids)
        assert [(nd["hin"], nd["hout"]) for nd in e.nodes if nd["kind"] != "conv"] == pools
    assert e.nodes[13]["hin"] % 2 == 1 and e.nodes[13]["hout"] * 2 < e.nodes[13]["hin"]     # 164: pool4 is VALID of an odd map


def test_default_plan_is_unchanged(E):
    e = E.SSDEngine.planned()
    assert e.grids == tuple((h, h) for h in (38, 19, 10, 5, 3, 1)) and e.A == 8732 and e.chain_start == 17
    assert not e.bf16_only and len(e.tensors) == 64 and all(nd["dilation"] == 1 for nd in e.nodes)
    assert [(nd["kind"], nd["pt"]) for nd in e.nodes[9:15]] == [("pool", 0), ("conv", 1), ("conv", 1), ("conv", 0), ("conv", 0), ("conv", 0)]
    with pytest.raises(ValueError, match="no launch"):
        E.SSDEngine.planned(trunk=E.SSD300_TRUNK[:3] + [("conv", 64, 128, 3, 2, "same", False, 2)] + E.SSD300_TRUNK[4:])
    with pytest.raises(ValueError, match="no launch"):
        E.SSDEngine.planned(trunk=[("pool5", 8, 8, 3, 1, "same", False)] + E.SSD300_TRUNK)


# ------------------------------------------------------------------------------------------------ the spec
def test_network_spec_of_the_vgg16(ops):
    for v in ("vgg16_ssd300", dict(kind="vgg16_ssd300"), dict(kind="vgg16_ssd300", in_size=300)):
        s = ops.NetworkSpec.of(v)
        assert (s.kind, s.in_size, s.batchnorm, s.precision, s.dgrad_precision) == ("vgg16_ssd300", 300, None, "bf16", None)
        d = s.as_dict()
        assert set(d) == set(ops.NetworkSpec.FIELDS) and ops.NetworkSpec.of(d).as_dict() == d
        assert ops.NetworkSpec.of(d).identity() == s.identity()
    ids = {ops.NetworkSpec.of(k).identity() for k in ("ssd300", "vgg16_ssd300", "resnet50_ssd512")}
    assert len(ids) == 3 and s.describe().startswith("vgg16_ssd300")
    for l2 in (None, False, True, 20.0, dict(init=10.0), ops.L2NormSpec()):
        assert ops.NetworkSpec.of("vgg16_ssd300", l2norm=l2).kind == "vgg16_ssd300"


@pytest.mark.parametrize("bad, word", [
    (dict(kind="vgg16_ssd300", batchnorm=True), "batchnorm"),
    (dict(kind="vgg16_ssd300", batchnorm=dict(momentum=0.1)), "batchnorm"),
    (dict(kind="vgg16_ssd300", precision="mxfp8"), "precision"),
    (dict(kind="vgg16_ssd300", dgrad_precision="bf16"), "precision"),
    (dict(kind="vgg16_ssd300", in_size=512), "512"),
    (dict(kind="vgg16_ssd300", in_size="300"), "300"),
    (dict(kind="vgg16_ssd300", dilation=6), "dilation"),
    (dict(kind="vgg16_ssd512"), "vgg16_ssd512"),
])
def test_bad_vgg16_specs_name_the_offender(ops, bad, word):
    with pytest.raises(ValueError, match=word):
        ops.NetworkSpec.of(bad)


def test_the_other_specs_behave_as_before(ops):
    s = ops.NetworkSpec.of(None)
    assert (s.kind, s.in_size, s.batchnorm, s.precision, s.dgrad_precision) == ("ssd300", 300, None, "bf16", None)
    assert s.identity() == ("ssd300", 300, False)
    r = ops.NetworkSpec.of(dict(kind="resnet50_ssd512", in_size=256, batchnorm=True))
    assert r.identity() == ("resnet50_ssd512", 256, True) and r.batchnorm.momentum == 0.1
    for l2 in (True, 20.0):
        with pytest.raises(ValueError, match="l2norm"):
            ops.NetworkSpec.of("resnet50_ssd512", l2norm=l2)
        assert ops.NetworkSpec.of(None, l2norm=l2).kind == "ssd300"
    with pytest.raises(ValueError, match="precision"):
        ops.NetworkSpec.of(dict(kind="ssd300", precision="mxfp8"))
    with pytest.raises(ValueError, match="vgg"):
        ops.NetworkSpec.of("vgg")
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    with pytest.raises(ValueError, match="batchnorm"):                   # the model's own check, before any engine is built
        SSDObjectDetectionModel(20, "unused", device="cpu", timestamp_dir=False, network=dict(kind="vgg16_ssd300", batchnorm=True))


def test_yaml_block(ops):
    from ssd_object_detection_amd.tools import train as T
    cfg = yaml.safe_load("model: {network: {kind: vgg16_ssd300}, l2norm: {enable: true, init: 20.0}}")
    s = T.network_from_config(cfg)
    assert s.kind == "vgg16_ssd300" and s.in_size == 300 and T.l2norm_from_config(cfg).init == 20.0
    assert T.network_from_config(yaml.safe_load("model: {network: {kind: vgg16_ssd300, in_size: 300, precision: bf16}}")).kind == "vgg16_ssd300"
    for text, word in (("model: {network: {kind: vgg16_ssd300, in_size: 512}}", "512"),
                       ("model: {network: {kind: vgg16_ssd300, precision: mxfp8}}", "precision"),
                       ("model: {network: {kind: vgg16_ssd300, batchnorm: {enable: true}}}", "batchnorm")):
        with pytest.raises(ValueError, match=word):
            T.network_from_config(yaml.safe_load(text))
    path = os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml")
    assert T.network_from_config(T.load_config(path)) is None            # the example is a comment: the default is built
    with open(path) as f:
        comments = "\n".join(ln.lstrip()[1:] for ln in f.read().splitlines() if ln.lstrip().startswith("#"))
    assert "kind: vgg16_ssd300" in comments


# ------------------------------------------------------------------------------------------------ the oracle's own walk
def test_teacher_forced_walk_equals_autograd_on_a_small_geometry(E):
    """tests/vgg16_oracle.backward_chain, fed the state of a float64 forward (maps, strict.ref_pool's codes), gives the gradients
    torch.autograd gives for the same forward: the walk's wiring (head + pooling into conv4_3's map, the un-masked data
    gradients behind the two poolings, the dilated vjp) is right before any engine is compared with it.  Trunk through the first
    stride-2 extra at 44 x 44: maps 6, 3, 2; pool4 is 6 -> 3 and pool5 / fc6 (dilation 6: eight of nine taps in the padding) run
    on 3 x 3."""
    from tests import strict as S
    from tests import vgg16_oracle as VO
    from tests.forced_oracle import F64, rel_l2
    trunk, pri, classes, B = E.VGG16_SSD300_TRUNK[:22], E.VGG16_SSD300_NUM_PRIORS[:3], 5, 2
    e = E.SSDEngine.planned(classes, 44, trunk, pri)
    assert e.grids == ((6, 6), (3, 3), (2, 2))
    g = torch.Generator().manual_seed(4)
    params = {}
    for t in [t for i in sorted(e.conv_params) for t in e.conv_params[i]] + [t for pair in e.head_params for t in pair]:
        if t.name.endswith("kernel"):
            fan = t.shape[1] * t.shape[2] * t.shape[3]
            params[t.name] = (torch.randn(t.shape, generator=g, dtype=F64) * (2.0 / fan) ** 0.5).requires_grad_(True)
        else:
            params[t.name] = (torch.randn(t.shape, generator=g, dtype=F64) * 0.05).requires_grad_(True)
    x = torch.randn((B, 44, 44, 8), generator=g, dtype=F64)
    keep = {}
    loc, conf = VO.forward(trunk, pri, classes, params, x, emulate_bf16=False, dtype=F64, keep=keep)
    dloc, dconf = torch.randn(loc.shape, generator=g, dtype=F64), torch.randn(conf.shape, generator=g, dtype=F64)
    names = sorted(params)
    want = dict(zip(names, torch.autograd.grad((loc * dloc).sum() + (conf * dconf).sum(), [params[n] for n in names])))
    acts = [x] + [keep[i].detach() for i in range(len(trunk))]
    codes = {}
    for i, nd in enumerate(e.nodes):
        if nd["kind"] == "pool":
            y, codes[i] = S.ref_pool(acts[i], 2, 2, 0, 0, nd["hout"], nd["hout"], 4)
        elif nd["kind"] == "pool3s1":
            y, codes[i] = S.ref_pool(acts[i], 3, 1, 1, 1, nd["hout"], nd["hout"], 15)
        else:
            continue
        assert torch.equal(y.clamp(min=0).to(F64), acts[i + 1])           # (a window of zeros: -inf never wins, the map holds 0)
    weights = {n: p.detach() for n, p in params.items()}
    T = VO.backward_chain(e.nodes, e.fm, pri, classes, weights, acts, codes, dloc, dconf)
    for n in names:
        assert rel_l2(T[n], want[n]) < 1e-12, (n, rel_l2(T[n], want[n]))
    # and the three wiring errors the GPU tests seed are errors of this walk
    for defect in (("overwrite", (13, 13)), ("no_head", 0), ("no_mask", 19)):
        D = VO.backward_chain(e.nodes, e.fm, pri, classes, weights, acts, codes, dloc, dconf, defect=defect)
        assert max(rel_l2(D[n], want[n]) for n in names) > 1e-2, defect
