"""CPU suite: the MobileNet-v1 SSD300 graph as planned (engine.MOBILENET_V1_SSD300_TRUNK through SSDEngine.planned: no device),
the chain's LDS rule in the planning, the plans of the three older networks (unchanged: values written here from the commit
before this network), the network spec and YAML block, and the test oracle of the backward pass (tests/mobilenet_oracle.py)
against torch.autograd on a small geometry."""
import ctypes
import hashlib
import os

import pytest

torch = pytest.importorskip("torch")
yaml = pytest.importorskip("yaml")

KIND = "mobilenet_v1_ssd300"


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


@pytest.fixture(scope="module")
def E():
    from ssd_object_detection_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ the graph
def test_trunk(E):
    t = E.MOBILENET_V1_SSD300_TRUNK
    assert len(t) == 35 and all(len(n) == 7 and n[5] == "same" for n in t)
    assert t[0] == ("conv", 8, 32, 3, 2, "same", False)
    dw = [i for i, n in enumerate(t) if n[0] == "dwconv"]
    assert dw == list(range(1, 26, 2)) and all(t[i][1] == t[i][2] == t[i + 1][1] and t[i + 1][3] == 1 for i in dw)
    assert [(t[i][1], t[i][4]) for i in dw] == [(32, 1), (64, 2), (128, 1), (128, 2), (256, 1), (256, 2)] + [(512, 1)] * 5 + [(512, 2), (1024, 1)]
    assert [t[i + 1][2] for i in dw] == [64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024]
    assert [i for i, n in enumerate(t) if n[6]] == [22, 26, 28, 30, 32, 34]
    assert [(n[1], n[2], n[3], n[4]) for n in t[27:]] == [(1024, 256, 1, 1), (256, 512, 3, 2), (512, 128, 1, 1), (128, 256, 3, 2),
                                                         (256, 128, 1, 1), (128, 256, 3, 2), (256, 128, 1, 1), (128, 256, 3, 2)]
    assert E.MOBILENET_V1_SSD300_NUM_PRIORS == (4, 6, 6, 6, 4, 4)


def test_planned_geometry_at_300(E, ops):
    e = E.SSDEngine.planned(81, 300, E.MOBILENET_V1_SSD300_TRUNK, E.MOBILENET_V1_SSD300_NUM_PRIORS)
    assert e.grids == tuple((h, h) for h in (19, 10, 5, 3, 2, 1)) and e.A == 2268
    assert e.level_off == [0, 1444, 2044, 2194, 2248, 2264, 2268]
    assert [(ni, h, c) for ni, h, c in e.fm] == [(22, 19, 512), (26, 10, 1024), (28, 5, 512), (30, 3, 256), (32, 2, 256), (34, 1, 256)]
    assert [nd["hout"] for nd in e.nodes] == [150] * 3 + [75] * 4 + [38] * 4 + [19] * 12 + [10] * 5 + [5, 5, 3, 3, 2, 2, 1]
    # Keras SAME at stride 2: an even map pads bottom / right only, an odd one a row on each side
    assert [(i, nd["hin"], nd["pt"]) for i, nd in enumerate(e.nodes) if nd["stride"] == 2] == [
        (0, 300, 0), (3, 150, 0), (7, 75, 1), (11, 38, 0), (23, 19, 1), (28, 10, 0), (30, 5, 1), (32, 3, 1), (34, 2, 0)]
    assert e.chain_start == 28 and e.sparse_heads and e.bf16_only and e.has_dw and not e.first_pair
    names = [t.name for t in e.tensors]
    assert len(names) == 2 * 35 + 4 * 6
    assert names[:6] == ["conv0/kernel", "conv0/bias", "dwconv1/kernel", "dwconv1/bias", "conv2/kernel", "conv2/bias"]
    assert names[2 * 25:2 * 27] == ["dwconv25/kernel", "dwconv25/bias", "conv26/kernel", "conv26/bias"] and names[70] == "head0/loc_kernel"
    for i, nd in enumerate(e.nodes):
        wt, bt = e.conv_params[i]
        if nd["kind"] == "dwconv":
            assert wt.shape == (3, 3, nd["cout"]) and bt.shape == (nd["cout"],) and wt.name == "dwconv%d/kernel" % i
        else:
            assert wt.shape == (nd["cout"], nd["k"], nd["k"], nd["cin"]) and wt.name == "conv%d/kernel" % i
    assert [t.index for t in e.tensors] == list(range(len(names))) and all(t.offset % 8 == 0 for t in e.tensors)
    # the optimizer buckets cover every tensor once, heads first; every bucket is gated by its lowest node, whatever its kind
    b = e.opt_buckets()
    assert b[0][2] is None and sorted(t for t0, t1, _ in b for t in range(t0, t1)) == list(range(len(names)))
    assert e.bucket_gates([(t0, t1) for t0, t1, _ in b]) == [node for _, _, node in b]
    assert e.decay_table(5e-4).tolist() == [pytest.approx(5e-4) if nm.endswith("kernel") else 0.0 for nm in names]
    assert e.decay_table(5e-4, True).tolist() == [pytest.approx(5e-4)] * len(names)
    with pytest.raises(ValueError, match="fp8_inference"):
        E.SSDEngine.planned(81, 300, E.MOBILENET_V1_SSD300_TRUNK, E.MOBILENET_V1_SSD300_NUM_PRIORS, fp8_inference=True)
    for bad in (("dwconv", 32, 64, 3, 1, "same", False), ("dwconv", 32, 32, 5, 1, "same", False), ("dwconv", 32, 32, 3, 1, "valid", False),
                ("dwconv", 12, 12, 3, 1, "same", False), ("dwconv", 32, 32, 3, 3, "same", False)):
        with pytest.raises(ValueError, match="depthwise"):
            E.SSDEngine.planned(trunk=[E.MOBILENET_V1_SSD300_TRUNK[0], bad] + E.MOBILENET_V1_SSD300_TRUNK[2:],
                                num_priors=E.MOBILENET_V1_SSD300_NUM_PRIORS)


def test_reduced_geometry_at_140(E):
    e = E.SSDEngine.planned(81, 140, E.MOBILENET_V1_SSD300_TRUNK[:-2], E.MOBILENET_V1_SSD300_NUM_PRIORS[:5])
    assert e.grids == tuple((h, h) for h in (9, 5, 3, 2, 1)) and e.A == 4 * 81 + 6 * (25 + 9 + 4) + 4
    # even and odd maps under stride 2
    assert [(nd["hin"], nd["hout"], nd["pt"]) for nd in e.nodes if nd["stride"] == 2][:5] == [(140, 70, 0), (70, 35, 0), (35, 18, 1), (18, 9, 0), (9, 5, 1)]
    assert e.chain_start == 27 and e.sparse_heads                       # 5x5x1024 fits: here the first extra is in the chain


def test_chain_lds_rule(E, ops):
    """ops.chain_lds_bytes restates ssd_conv_chain's arithmetic: pinned by hand-computed figures and, for the one run that
    does not fit, by the library's own refusal (decided on the host before any launch; the pointers are never read)."""
    e = E.SSDEngine.planned(81, 300, E.MOBILENET_V1_SSD300_TRUNK, E.MOBILENET_V1_SSD300_NUM_PRIORS)

    def fwd(j):
        return [(nd["hin"] ** 2, nd["cin"], nd["hout"] ** 2, nd["cout"]) for nd in e.nodes[j:]]

    assert ops.CHAIN_LDS_MAX == 160 * 1024
    # nodes 27 .. 34: the input 10x10x1024 alone is 100 (2048 + 16) = 206400 B; region 1 holds 10x10x256, one zero row 2048 B
    assert ops.chain_lds_bytes(fwd(27)) == 206400 + 100 * (512 + 16) + 2048 > ops.CHAIN_LDS_MAX
    # nodes 28 .. 34: regions 10x10x256 (52800) and 5x5x512 (25 * 1040 = 26000), zero row 1024 B
    assert ops.chain_lds_bytes(fwd(28)) == 52800 + 26000 + 1024
    assert not e._chain_fits(27) and e._chain_fits(28)
    # the default network's chain (nodes 17 .. 22): 10x10x512 (104000) and 10x10x128 (27200), zero row 1024 B
    d = E.SSDEngine.planned()
    assert ops.chain_lds_bytes([(nd["hin"] ** 2, nd["cin"], nd["hout"] ** 2, nd["cout"]) for nd in d.nodes[17:]]) == 104000 + 27200 + 1024
    # the library: the eight layers 27 .. 34 are refused with SSD_ERR_UNSUPPORTED (every other check passes first)
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    arr = (_lib.ChainLayer * 8)()
    for l, nd in enumerate(e.nodes[27:]):
        s = arr[l]
        s.w, s.out = ctypes.c_void_p(0x10000000 * (l + 1)), ctypes.c_void_p(0x10000000 * (l + 9))
        s.Hi = s.Wi = nd["hin"]
        s.Ho = s.Wo = nd["hout"]
        s.Kc, s.N, s.ksize, s.mul, s.div, s.pad_t, s.pad_l, s.relu = nd["cin"], nd["cout"], nd["k"], nd["stride"], 1, nd["pt"], nd["pl"], 1
    assert L.ssd_conv_chain(ctypes.c_void_p(0x70000000), arr, 8, 2, None) == _lib.SSD_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the older networks
PARENT = {   # (chain_start, tensors, n_flat, A, sha1 of [(name, shape, offset, block0, nblocks)]) as planned by the commit before
    "ssd300": (17, 64, 25155584, 8732, "2054cd8dc90c08e5ffbdab7dabb56d4f7aca8381"),
    "ssd512": (19, 72, 26662912, 24564, "4d71dc7a2e690ba0bc3f4d17c24be466c3288bed"),
    "vgg16_ssd300": (22, 70, 34333696, 8732, "7669faaec7f8eb35d0cb954283717734b1dc03e5"),
}


def test_older_plans_are_unchanged(E):
    graphs = {"ssd300": (300, E.SSD300_TRUNK, E.SSD300_NUM_PRIORS), "ssd512": (512, E.SSD512_TRUNK, E.SSD512_NUM_PRIORS),
              "vgg16_ssd300": (300, E.VGG16_SSD300_TRUNK, E.VGG16_SSD300_NUM_PRIORS)}
    for name, (size, trunk, pri) in graphs.items():
        e = E.SSDEngine.planned(81, size, trunk, pri)
        digest = hashlib.sha1(repr([(t.name, tuple(t.shape), t.offset, t.block0, t.nblocks) for t in e.tensors]).encode()).hexdigest()
        assert (e.chain_start, len(e.tensors), e.n_flat, e.A, digest) == PARENT[name], name
        assert not e.has_dw and [t.offset for t in e.tensors[:4]] == [0, 5120, 6144, 43008]
    assert not E.SSDEngine.planned().bf16_only
    # a reduced VGG-16 geometry whose planned chain the kernel refuses keeps its plan (the refusal is learned at the launch)
    assert E.SSDEngine.planned(81, 164, E.VGG16_SSD300_TRUNK[:-2], E.VGG16_SSD300_NUM_PRIORS[:5]).chain_start == 19


# ------------------------------------------------------------------------------------------------ the spec
def test_network_spec(ops):
    for v in (KIND, dict(kind=KIND), dict(kind=KIND, in_size=300)):
        s = ops.NetworkSpec.of(v)
        assert (s.kind, s.in_size, s.batchnorm, s.precision, s.dgrad_precision) == (KIND, 300, None, "bf16", None)
        d = s.as_dict()
        assert set(d) == set(ops.NetworkSpec.FIELDS) and ops.NetworkSpec.of(d).as_dict() == d
    ids = {ops.NetworkSpec.of(k).identity() for k in ops.NetworkSpec.KINDS}
    assert len(ids) == 4 and s.describe().startswith(KIND) and KIND not in ops.NetworkSpec.L2NORM_KINDS
    assert ops.NetworkSpec.of(KIND, l2norm=None).kind == ops.NetworkSpec.of(KIND, l2norm=False).kind == KIND
    assert ops.MOBILENET_SSD300_S_REF == (60, 105, 150, 195, 240, 285, 330)
    assert [round(v / 300.0, 4) for v in ops.MOBILENET_SSD300_S_REF[:6]] == [0.2, 0.35, 0.5, 0.65, 0.8, 0.95]


@pytest.mark.parametrize("bad, word", [
    (dict(kind=KIND, batchnorm=True), "batchnorm"),
    (dict(kind=KIND, precision="mxfp8"), "precision"),
    (dict(kind=KIND, dgrad_precision="bf16"), "precision"),
    (dict(kind=KIND, in_size=512), "512"),
    (dict(kind=KIND, in_size=224), "224"),
    (dict(kind=KIND, width=0.5), "width"),
    (dict(kind="mobilenet_v2_ssd300"), "mobilenet_v2_ssd300"),
])
def test_bad_specs_name_the_offender(ops, bad, word):
    with pytest.raises(ValueError, match=word):
        ops.NetworkSpec.of(bad)


def test_l2norm_and_fp8_inference_are_refused(ops):
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    for l2 in (True, 20.0, dict(init=10.0)):
        with pytest.raises(ValueError, match="l2norm"):
            ops.NetworkSpec.of(KIND, l2norm=l2)
    with pytest.raises(ValueError, match="l2norm"):                      # the model's own checks, before any engine is built
        SSDObjectDetectionModel(20, "unused", device="cpu", timestamp_dir=False, network=KIND, l2norm=True)
    with pytest.raises(ValueError, match="fp8_inference"):
        SSDObjectDetectionModel(20, "unused", device="cpu", timestamp_dir=False, network=KIND, fp8_inference=True)
    with pytest.raises(ValueError, match="batchnorm"):
        SSDObjectDetectionModel(20, "unused", device="cpu", timestamp_dir=False, network=dict(kind=KIND, batchnorm=True))


def test_yaml_block(ops):
    from ssd_object_detection_amd.tools import train as T
    s = T.network_from_config(yaml.safe_load("model: {network: {kind: mobilenet_v1_ssd300}}"))
    assert s.kind == KIND and s.in_size == 300
    assert T.network_from_config(yaml.safe_load("model: {network: {kind: mobilenet_v1_ssd300, in_size: 300, precision: bf16}}")).kind == KIND
    for text, word in (("model: {network: {kind: mobilenet_v1_ssd300, in_size: 512}}", "512"),
                       ("model: {network: {kind: mobilenet_v1_ssd300, precision: mxfp8}}", "precision"),
                       ("model: {network: {kind: mobilenet_v1_ssd300, batchnorm: {enable: true}}}", "batchnorm"),
                       ("model: {network: {kind: mobilenet_v1_ssd300}, l2norm: {enable: true}}", "l2norm")):
        with pytest.raises(ValueError, match=word):
            T.network_from_config(yaml.safe_load(text))
    path = os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml")
    assert T.network_from_config(T.load_config(path)) is None            # the example is a comment: the default is built
    with open(path) as f:
        comments = "\n".join(ln.lstrip()[1:] for ln in f.read().splitlines() if ln.lstrip().startswith("#"))
    assert "kind: mobilenet_v1_ssd300" in comments
    assert "mobilenet_v1_ssd300" in T.__doc__ or "mobilenet_v1_ssd300" in T.network_from_config.__doc__


# ------------------------------------------------------------------------------------------------ the oracle's own walk
def _init_like_the_engine(e, seed, dtype):
    """the engine's init_params on the CPU: He-uniform over fan-in 9 for the depthwise filters, glorot for the others"""
    import numpy as np
    rng = np.random.default_rng(seed)
    params = {}
    for t in e.tensors:
        if not t.name.endswith("kernel"):
            continue
        if t.name.startswith("dwconv"):
            lim = (6.0 / 9.0) ** 0.5
        else:
            cout, k, _, cin = t.shape
            lim = (6.0 / (k * k * (3 if t.name == "conv0/kernel" else cin) + k * k * cout)) ** 0.5
        w = rng.uniform(-lim, lim, t.shape)
        if t.name == "conv0/kernel":
            w[..., 3:] = 0.0
        params[t.name] = torch.from_numpy(w).to(dtype)
    return params


def test_init_keeps_the_reduced_forward_alive(E):
    """Every stored map of the reduced geometry (140, trunk[:-2]) has at least a tenth of its elements positive under the
    engine's initialisation, for the seeds the GPU tests use: a condition on the chosen init (He-uniform over the depthwise
    layers' true fan-in), asserted, not measured.  The host restatement of init_params above draws the same numbers."""
    from tests import mobilenet_oracle as MO
    trunk, pri = E.MOBILENET_V1_SSD300_TRUNK[:-2], E.MOBILENET_V1_SSD300_NUM_PRIORS[:5]
    e = E.SSDEngine.planned(81, 140, trunk, pri)
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    for seed in (3, 7):
        params = _init_like_the_engine(e, seed, torch.float32)
        for pair in list(e.conv_params.values()) + [(None, b) for _, b in e.head_params]:
            params[pair[1].name] = torch.zeros(pair[1].shape)
        for wt, _ in e.head_params:
            a, b = wt.parts
            params[wt.name] = torch.cat([params[a.name], params[b.name]], 0)
        x = torch.rand((2, 140, 140, 3), generator=torch.Generator().manual_seed(1))
        x = torch.cat([x, torch.zeros(2, 140, 140, 5)], -1).bfloat16().float()
        keep = {}
        MO.forward(trunk, pri, 81, params, x, keep=keep)
        frac = MO.alive(keep)
        assert len(frac) == 33 and min(frac.values()) >= 0.1, (seed, sorted(frac.items(), key=lambda kv: kv[1])[:3])


def test_teacher_forced_walk_equals_autograd_on_a_small_geometry(E):
    """tests/mobilenet_oracle.backward_chain, fed the state of a float64 forward, gives the gradients torch.autograd gives for
    the same forward: the depthwise vjp, the masks, and the head + trunk sum into a feature map that a stride-2 depthwise node
    reads are right before any engine is compared with it.  A cut-down trunk at 20 x 20: maps 10, 10, 5 (dw s2 on an even
    map), 5, 3 (dw s2 on an odd map), 3, and one stride-2 extra; feature maps on nodes 4, 6 and 8."""
    from tests import mobilenet_oracle as MO
    from tests.forced_oracle import F64, rel_l2
    trunk = [("conv", 8, 16, 3, 2, "same", False), ("dwconv", 16, 16, 3, 1, "same", False), ("conv", 16, 32, 1, 1, "same", False),
             ("dwconv", 32, 32, 3, 2, "same", False), ("conv", 32, 128, 1, 1, "same", True),
             ("dwconv", 128, 128, 3, 2, "same", False), ("conv", 128, 128, 1, 1, "same", True),
             ("conv", 128, 128, 1, 1, "same", False), ("conv", 128, 128, 3, 2, "same", True)]
    pri, classes, B = (4, 6, 4), 5, 2
    e = E.SSDEngine.planned(classes, 20, trunk, pri)
    assert e.grids == ((5, 5), (3, 3), (2, 2)) and [nd["pt"] for nd in e.nodes if nd["kind"] == "dwconv"] == [1, 0, 1]
    g = torch.Generator().manual_seed(4)
    params = {}
    for t in [t for i in sorted(e.conv_params) for t in e.conv_params[i]] + [t for pair in e.head_params for t in pair]:
        if t.name.endswith("kernel"):
            fan = 9 if t.name.startswith("dwconv") else t.shape[1] * t.shape[2] * t.shape[3]
            params[t.name] = (torch.randn(t.shape, generator=g, dtype=F64) * (2.0 / fan) ** 0.5).requires_grad_(True)
        else:
            params[t.name] = (torch.randn(t.shape, generator=g, dtype=F64) * 0.05).requires_grad_(True)
    x = torch.randn((B, 20, 20, 8), generator=g, dtype=F64)
    keep = {}
    loc, conf = MO.forward(trunk, pri, classes, params, x, emulate_bf16=False, dtype=F64, keep=keep)
    assert min(MO.alive(keep).values()) > 0.1
    dloc, dconf = torch.randn(loc.shape, generator=g, dtype=F64), torch.randn(conf.shape, generator=g, dtype=F64)
    names = sorted(params)
    want = dict(zip(names, torch.autograd.grad((loc * dloc).sum() + (conf * dconf).sum(), [params[n] for n in names])))
    acts = [x] + [keep[i].detach() for i in range(len(trunk))]
    weights = {n: p.detach() for n, p in params.items()}
    T = MO.backward_chain(e.nodes, e.fm, pri, classes, weights, acts, {}, dloc, dconf)
    for n in names:
        assert rel_l2(T[n], want[n]) < 1e-12, (n, rel_l2(T[n], want[n]))
    # and the three wiring errors the GPU tests seed are errors of this walk
    for defect in (("overwrite", (5, 5)), ("no_head", 0), ("no_mask", 6)):
        D = MO.backward_chain(e.nodes, e.fm, pri, classes, weights, acts, {}, dloc, dconf, defect=defect)
        assert max(rel_l2(D[n], want[n]) for n in names) > 1e-2, defect
