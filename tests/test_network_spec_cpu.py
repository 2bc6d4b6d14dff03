"""CPU suite: the network spec (ops.NetworkSpec), its YAML block (tools.train.network_from_config), the package's SSD512 anchor
geometry, momentum SGD's decay table for the batch-normalised ResNet-50 SSD512 plan, and the data-parallel gradient exchange
(parallel.GradReducer, world 2 over gloo) fed the order in which ResNet50SSDEngine.backward reports its tensors.  No device
is touched: the ResNet plans come from ResNet50SSDEngine.planned()."""
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
yaml = pytest.importorskip("yaml")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


# ------------------------------------------------------------------------------------------------ NetworkSpec.of
def test_default_forms(ops):
    for v in (None, "ssd300", dict(), dict(kind="ssd300"), dict(kind="ssd300", in_size=300), ops.NetworkSpec()):
        s = ops.NetworkSpec.of(v)
        assert (s.kind, s.in_size, s.batchnorm, s.precision, s.dgrad_precision) == ("ssd300", 300, None, "bf16", None)
    s = ops.NetworkSpec()
    assert ops.NetworkSpec.of(s) is s


def test_resnet_forms_and_defaults(ops):
    s = ops.NetworkSpec.of("resnet50_ssd512")
    assert (s.kind, s.in_size, s.batchnorm, s.precision, s.dgrad_precision) == ("resnet50_ssd512", 512, None, "bf16", None)
    s = ops.NetworkSpec.of(dict(kind="resnet50_ssd512", in_size=256, batchnorm=dict(momentum=0.25)))
    assert s.in_size == 256 and s.batchnorm.momentum == 0.25 and s.batchnorm.eps == 1e-5
    assert ops.NetworkSpec.of(dict(kind="resnet50_ssd512", batchnorm=True)).batchnorm.momentum == 0.1
    assert ops.NetworkSpec.of(dict(kind="resnet50_ssd512", batchnorm=False)).batchnorm is None
    bn = ops.BatchNormSpec(momentum=0.5)
    assert ops.NetworkSpec.of(dict(kind="resnet50_ssd512", batchnorm=bn)).batchnorm is bn
    s = ops.NetworkSpec.of(dict(kind="resnet50_ssd512", precision="mxfp8", dgrad_precision="bf16"))
    assert (s.precision, s.dgrad_precision) == ("mxfp8", "bf16")
    assert ops.NetworkSpec.of(dict(kind="resnet50_ssd512", precision="mxfp8", dgrad_precision="mxfp8")).dgrad_precision == "mxfp8"
    assert ops.NetworkSpec.of(dict(kind="resnet50_ssd512", precision="bf16", dgrad_precision="bf16")).dgrad_precision == "bf16"


def test_round_trip_through_the_plain_dict(ops):
    for v in (None, "resnet50_ssd512", dict(kind="resnet50_ssd512", in_size=256, batchnorm=dict(momentum=0.2, eps=1e-4)),
              dict(kind="resnet50_ssd512", precision="mxfp8", dgrad_precision="bf16")):
        s = ops.NetworkSpec.of(v)
        d = s.as_dict()
        assert set(d) == set(ops.NetworkSpec.FIELDS)
        assert all(isinstance(x, (str, int, float, type(None), dict)) for x in d.values())
        assert ops.NetworkSpec.of(d).as_dict() == d and ops.NetworkSpec.of(d).identity() == s.identity()
    a = ops.NetworkSpec.of(dict(kind="resnet50_ssd512", in_size=256))
    ids = {a.identity(), ops.NetworkSpec.of(None).identity(), ops.NetworkSpec.of("resnet50_ssd512").identity(),
           ops.NetworkSpec.of(dict(kind="resnet50_ssd512", in_size=256, batchnorm=True)).identity()}
    assert len(ids) == 4
    # how a run trains the network is not which network it is
    assert ops.NetworkSpec.of(dict(kind="resnet50_ssd512", in_size=256, precision="mxfp8")).identity() == a.identity()


@pytest.mark.parametrize("bad, word", [
    ("vgg512", "vgg512"),
    (3, "3"),
    (["resnet50_ssd512"], "resnet50_ssd512"),
    (dict(kind="resnet50"), "resnet50"),
    (dict(kind="resnet50_ssd512", size=512), "size"),
    (dict(kind="ssd300", in_size=512), "512"),
    (dict(kind="resnet50_ssd512", in_size=300), "300"),
    (dict(kind="resnet50_ssd512", in_size=384), "384"),
    (dict(kind="resnet50_ssd512", in_size="512"), "512"),
    (dict(kind="resnet50_ssd512", in_size=True), "True"),
    (dict(kind="resnet50_ssd512", in_size=512.0), "512.0"),
    (dict(kind="resnet50_ssd512", precision="fp16"), "fp16"),
    (dict(kind="resnet50_ssd512", precision=None), "None"),
    (dict(kind="resnet50_ssd512", dgrad_precision="fp8"), "fp8"),
    (dict(kind="resnet50_ssd512", dgrad_precision="mxfp8"), "dgrad_precision"),      # behind a bf16 forward
    (dict(kind="resnet50_ssd512", batchnorm=dict(momentun=0.1)), "momentun"),
    (dict(kind="resnet50_ssd512", batchnorm=dict(momentum=2.0)), "momentum"),
    (dict(kind="resnet50_ssd512", batchnorm=0.1), "batchnorm"),
    (dict(kind="resnet50_ssd512", batchnorm=True, precision="mxfp8"), "batchnorm"),
    (dict(kind="ssd300", batchnorm=True), "batchnorm"),
    (dict(kind="ssd300", precision="mxfp8"), "precision"),
    (dict(kind="ssd300", dgrad_precision="bf16"), "precision"),
])
def test_bad_specs_name_the_offender(ops, bad, word):
    with pytest.raises(ValueError, match=word):
        ops.NetworkSpec.of(bad)


def test_l2norm_with_the_resnet_is_refused(ops):
    for l2 in (True, 20.0, dict(init=10.0), ops.L2NormSpec()):
        with pytest.raises(ValueError, match="l2norm"):
            ops.NetworkSpec.of("resnet50_ssd512", l2norm=l2)
        assert ops.NetworkSpec.of(None, l2norm=l2).kind == "ssd300"
    assert ops.NetworkSpec.of("resnet50_ssd512", l2norm=None).kind == "resnet50_ssd512"
    assert ops.NetworkSpec.of("resnet50_ssd512", l2norm=False).kind == "resnet50_ssd512"
    from ssd_object_detection_amd.models import SSDObjectDetectionModel
    with pytest.raises(ValueError, match="l2norm"):                      # the model's own check, before any engine is built
        SSDObjectDetectionModel(80, "unused", device="cpu", timestamp_dir=False, l2norm=True, network="resnet50_ssd512")
    with pytest.raises(ValueError, match="vgg"):
        SSDObjectDetectionModel(80, "unused", device="cpu", timestamp_dir=False, network="vgg")


# ------------------------------------------------------------------------------------------------ the YAML block
def _cfg(text):
    return yaml.safe_load(text)


def test_network_from_config(ops):
    from ssd_object_detection_amd.tools import train as T
    assert T.network_from_config(_cfg("model: {log_dir: x}")) is None
    assert T.network_from_config(_cfg("data: {}")) is None
    assert T.network_from_config(_cfg("model:\n  network:\n")) is None
    s = T.network_from_config(_cfg("""
model:
  network:
    kind: resnet50_ssd512
    in_size: 512
    batchnorm: {enable: true, momentum: 0.1, eps: 0.00001}
    precision: bf16
    dgrad_precision: null
"""))
    assert isinstance(s, ops.NetworkSpec)
    assert s.as_dict() == dict(kind="resnet50_ssd512", in_size=512, batchnorm=dict(momentum=0.1, eps=0.00001), precision="bf16",
                               dgrad_precision=None)
    s = T.network_from_config(_cfg("model: {network: {kind: resnet50_ssd512, in_size: 256, batchnorm: {enable: false, momentum: 0.3}}}"))
    assert s.in_size == 256 and s.batchnorm is None                       # disabled: the folded network
    assert T.network_from_config(_cfg("model: {network: {kind: resnet50_ssd512, batchnorm: {momentum: 0.3}}}")).batchnorm is None
    assert T.network_from_config(_cfg("model: {network: {kind: resnet50_ssd512, batchnorm: null}}")).batchnorm is None
    s = T.network_from_config(_cfg("model: {network: {kind: resnet50_ssd512, precision: mxfp8, dgrad_precision: bf16}}"))
    assert (s.precision, s.dgrad_precision, s.in_size) == ("mxfp8", "bf16", 512)
    assert T.network_from_config(_cfg("model: {network: {kind: ssd300}}")).kind == "ssd300"
    assert T.network_from_config(_cfg("model: {network: {}}")).kind == "ssd300"


@pytest.mark.parametrize("text, word", [
    ("model: {network: resnet50_ssd512}", "mapping"),
    ("model: {network: [resnet50_ssd512]}", "mapping"),
    ("model: {network: {kind: resnet50_ssd512, input: 512}}", "input"),
    ("model: {network: {kind: resnet50_ssd512, in_size: '512'}}", "512"),
    ("model: {network: {kind: resnet50_ssd512, in_size: 300}}", "300"),
    ("model: {network: {kind: 512}}", "512"),
    ("model: {network: {kind: resnet50_ssd512, batchnorm: true}}", "mapping"),
    ("model: {network: {kind: resnet50_ssd512, batchnorm: {enable: yes please}}}", "enable"),
    ("model: {network: {kind: resnet50_ssd512, batchnorm: {enable: 1}}}", "enable"),
    ("model: {network: {kind: resnet50_ssd512, batchnorm: {enable: true, decay: 0.9}}}", "decay"),
    ("model: {network: {kind: resnet50_ssd512, batchnorm: {enable: false, momentum: fast}}}", "momentum"),
    ("model: {network: {kind: resnet50_ssd512, batchnorm: {enable: true, eps: 1e-5}}}", "eps"),      # YAML 1.1: a string
    ("model: {network: {kind: resnet50_ssd512, batchnorm: {enable: true}, precision: mxfp8}}", "batchnorm"),
    ("model: {network: {kind: resnet50_ssd512, precision: 8}}", "8"),
    ("model: {network: {kind: resnet50_ssd512}, l2norm: {enable: true}}", "l2norm"),
])
def test_network_from_config_refuses(text, word):
    from ssd_object_detection_amd.tools import train as T
    with pytest.raises(ValueError, match=word):
        T.network_from_config(_cfg(text))


def test_default_yml_documents_the_block_and_builds_the_default():
    from ssd_object_detection_amd.tools import train as T
    path = os.path.join(os.path.dirname(T.__file__), "..", "config", "default.yml")
    assert T.network_from_config(T.load_config(path)) is None
    with open(path) as f:
        text = f.read()
    block = [ln for ln in text.splitlines() if ln.lstrip().startswith("#")]
    joined = "\n".join(ln.lstrip()[1:] for ln in block)
    for key in ("network:", "kind: resnet50_ssd512", "in_size:", "batchnorm:", "precision:", "dgrad_precision:"):
        assert key in joined, key


def test_loader_takes_the_input_size():
    from ssd_object_detection_amd.data_loaders import SSDDataLoader
    train, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=3).get_dataset()
    assert next(iter(train))[0].shape == (300, 300, 3)
    train, val = SSDDataLoader("unused", dataset="synthetic", shuffle=False, mini_batch=3, input_size=256).get_dataset()
    assert next(iter(train))[0].shape == (256, 256, 3) and next(iter(val))[0].shape == (256, 256, 3)
    for bad in (0, -4, 2.5, "256", True, None):
        with pytest.raises(ValueError):
            SSDDataLoader("unused", dataset="synthetic", input_size=bad)


# ------------------------------------------------------------------------------------------------ anchor geometry
def test_ssd512_constants_equal_the_benchmarks(ops):
    assert ops.SSD512_S_REF == bench.CFG5_S_REF and ops.SSD512_RATIOS == bench.CFG5_RATIOS
    assert ops.ssd512_s_ref(512) == tuple(float(v) for v in bench.CFG5_S_REF)
    assert ops.ssd512_s_ref(256) == tuple(v * 256 / 512.0 for v in bench.CFG5_S_REF)
    from ssd_object_detection_amd.engine import SSD512_NUM_PRIORS
    assert tuple(2 + 2 * len(r) for r in ops.SSD512_RATIOS) == tuple(SSD512_NUM_PRIORS)


def test_planned_resnet_geometry():
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    assert ResNet50SSDEngine.bucket_optimizer is False
    from ssd_object_detection_amd.engine import SSDEngine
    assert SSDEngine.bucket_optimizer is True
    e512, e256 = ResNet50SSDEngine.planned(81, 512), ResNet50SSDEngine.planned(81, 256)
    assert e512.A == 24564 and e512.grids == tuple((h, h) for h in (64, 32, 16, 8, 4, 2, 1))
    assert e256.grids == tuple((h, h) for h in (32, 16, 8, 4, 2, 1, 1))
    assert [t.name for t in e512.tensors] == [t.name for t in e256.tensors]     # the same layout: only the spec tells them apart
    bn = ResNet50SSDEngine.planned(81, 256, batchnorm=True)
    assert len(bn.tensors) == len(e256.tensors) + 86


# ------------------------------------------------------------------------------------------------ decay table
def _parent_table(names, weight_decay, decay_bias):
    """engine.decay_table as the commit before this suite computed it."""
    return torch.tensor([float(weight_decay) if (n.endswith("kernel") or decay_bias) else 0.0 for n in names], dtype=torch.float32)


def test_decay_table_of_a_batchnorm_resnet():
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    eng = ResNet50SSDEngine.planned(81, 256, batchnorm=True)
    names = [t.name for t in eng.tensors]
    assert sum(n.endswith("/gamma") for n in names) == 43 and sum(n.endswith("/beta") for n in names) == 43
    tab = eng.decay_table(5e-4)
    assert tab.dtype == torch.float32 and tab.shape == (len(names),)
    wd = float(np.float32(5e-4))
    for n, v in zip(names, tab.tolist()):
        if n.endswith("kernel"):
            assert v == wd, n
        else:
            assert n.endswith(("bias", "/gamma", "/beta")) and v == 0.0, n
    assert eng.decay_table(5e-4, decay_bias=True).tolist() == [wd] * len(names)
    assert eng.decay_table(5e-4) is tab                                   # cached per (weight_decay, decay_bias)
    plain = ResNet50SSDEngine.planned(81, 256)
    assert torch.equal(plain.decay_table(5e-4), _parent_table([t.name for t in plain.tensors], 5e-4, False))


def test_decay_table_of_ssd300_is_unchanged(ops):
    from ssd_object_detection_amd import engine as E
    from ssd_object_detection_amd import _lib
    for l2norm in (None, True):
        eng = E.SSDEngine.__new__(E.SSDEngine)
        eng.L = _lib.lib()
        eng.l2norm = ops.L2NormSpec.of(l2norm)
        eng.classes, eng.in_size, eng.device = 81, 300, torch.device("cpu")
        eng.trunk, eng.num_priors, eng.sparse_heads = list(E.SSD300_TRUNK), tuple(E.SSD300_NUM_PRIORS), True
        eng.block = eng.L.ssd_opt_block_elems()
        eng._plan_shapes()
        eng._plan_params()
        names = [t.name for t in eng.tensors]
        assert len(names) == 64 + (l2norm is True)
        for wd, db in ((5e-4, False), (5e-4, True), (0.0, False), (1e-2, False)):
            assert torch.equal(eng.decay_table(wd, db), _parent_table(names, wd, db)), (l2norm, wd, db)


# ------------------------------------------------------------------------------------------------ reducer order
def test_ready_order_covers_every_tensor_once():
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    for bn in (None, True):
        eng = ResNet50SSDEngine.planned(81, 256, batchnorm=bn)
        calls = eng.ready_order()
        flat = [i for c in calls for i in c]
        assert sorted(flat) == list(range(len(eng.tensors)))
        first_head = eng.head_params[0][0].index
        assert min(calls[-1]) == first_head and len(calls[-1]) == 28     # the heads: last, all at once
        assert flat != sorted(flat, reverse=True)                         # not "from the end of the buffer"
        if bn:                                                            # gamma / beta behind the heads, reported throughout
            assert all(eng.tensors[i].name.startswith("bn") for i in range(first_head + 28, len(eng.tensors)))
            at = [k for k, c in enumerate(calls) if eng.tensors[c[0]].name.startswith("bn")]
            assert len(at) == 43 and at[0] == 10 and at[-1] == len(calls) - 3     # behind the ten extras .. in front of the stem


def _layout(batchnorm):
    """The ResNet's tensors with ONE element per optimizer block: its order, indices and bucket plan at a size a CPU exchange
    handles in milliseconds."""
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    eng = ResNet50SSDEngine.planned(81, 256, batchnorm=batchnorm)
    blocks = [t.nblocks for t in eng.tensors]
    offs = [t.block0 for t in eng.tensors]
    return eng.ready_order(), offs, blocks, eng.n_flat // eng.block


def _rank_grad(rank, total):
    return np.random.default_rng(40 + rank).normal(0, 0.05, total).astype(np.float32)


def _clip(seg, clip=0.01):
    n = float(np.sqrt(np.sum(seg.astype(np.float64) ** 2)))
    return (seg * np.float32(clip / max(n, clip))).astype(np.float32)


def _order_worker(rank, world, port, batchnorm, out):
    import torch.distributed as dist
    from ssd_object_detection_amd.parallel import GradReducer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls, offs, blocks, total = _layout(batchnorm)
    flat = torch.from_numpy(_rank_grad(rank, total))
    reported, launches = set(), []

    def clip_fn(t0, t1):
        launches.append((t0, t1, all(t in reported for t in range(t0, t1))))
        for t in range(t0, t1):
            seg = flat[offs[t]:offs[t] + blocks[t]]
            seg.copy_(torch.from_numpy(_clip(seg.numpy())))

    red = GradReducer(flat, offs, blocks, 1, clip_fn)
    for step in range(2):                                   # twice: begin() resets what the first pass left
        if step:
            flat.copy_(torch.from_numpy(_rank_grad(rank, total)))
            del launches[:]
            reported.clear()
        red.begin(None, None)
        for c in calls:
            reported.update(c)
            red.tensor_ready(c)
        red.finish()                                        # asserts that every bucket was launched
    if rank == 0:
        out.put((flat.numpy().copy(), list(red.buckets), launches))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("batchnorm", [None, True], ids=["folded", "batchnorm"])
def test_reducer_is_correct_under_the_resnets_report_order(batchnorm):
    """The reducer plans its buckets from the end of the buffer; the ResNet reports its heads last and a batchnorm engine's
    gamma / beta (behind the heads) throughout.  Every bucket must still be clipped and summed exactly once, only after all of
    its tensors were reported, and the result must be the sum over ranks of the per-rank clipped gradients."""
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_order_worker, args=(r, 2, port, batchnorm, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got, buckets, launches = q.get(timeout=120)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    calls, offs, blocks, total = _layout(batchnorm)
    n = len(offs)
    assert len(buckets) > 1 and sorted(t for t0, t1 in buckets for t in range(t0, t1)) == list(range(n))
    assert [(t0, t1) for t0, t1, _ in launches] == buckets                # once each, in bucket order
    assert all(ok for _, _, ok in launches)                               # never before its last tensor was reported
    want = np.zeros(total, np.float64)
    for r in range(2):
        g = _rank_grad(r, total)
        for t in range(n):
            want[offs[t]:offs[t] + blocks[t]] += _clip(g[offs[t]:offs[t] + blocks[t]])
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-9)
