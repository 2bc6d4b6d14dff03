"""CPU: the batch normalisation oracle (tests/batchnorm_oracle.py) against torch autograd, its bounds against fp32 emulations
(any summation order passes, the naive variance does not), the batch-normalised graph, folding, and the C ABI's refusals
(host-side: nothing is launched, no GPU needed)."""
import ctypes

import numpy as np
import pytest

from tests import batchnorm_oracle as O

torch = pytest.importorskip("torch")
import torch.nn.functional as F                                      # noqa: E402

_CASES = {}


def case(shape):
    if shape not in _CASES:
        _CASES[shape] = O.make_case(*shape)
    return _CASES[shape]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", O.SHAPES, ids=str)
def test_oracle_matches_autograd(shape, relu):
    k = case(shape)
    P, C = shape
    x = torch.from_numpy(k["x"]).double().requires_grad_(True)
    gamma = torch.from_numpy(k["gamma"]).double().requires_grad_(True)
    beta = torch.from_numpy(k["beta"]).double().requires_grad_(True)
    rm, rv = torch.from_numpy(k["rm"]).double(), torch.from_numpy(k["rv"]).double()
    y = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=O.MOMENTUM, eps=O.EPS)     # updates rm, rv in place
    if relu:
        y = y.relu()
    r = O.fwd64(k["x"], k["gamma"], k["beta"], relu=relu, running=(k["rm"], k["rv"]))

    scale = max(1.0, float(np.abs(k["x"]).max()))                        # both sides round x - mu at the magnitude of x (300)

    def close(got, want):
        assert np.abs(got - want).max() <= 1e-12 * max(scale, np.abs(want).max()), np.abs(got - want).max()
    close(r["y"], y.detach().numpy())
    close(r["rm"], rm.numpy())
    close(r["rv"], rv.numpy())
    dy = torch.from_numpy(k["dy"]).double()
    dy_masked = dy * (y.detach() > 0) if relu else dy                    # the engine's convention: the consumer masks
    y.backward(dy)
    dx, dgamma, dbeta = O.bwd64(dy_masked.numpy(), k["x"], k["gamma"], r["mean"], r["rstd"])
    close(dx, x.grad.numpy())
    close(dgamma, gamma.grad.numpy())
    close(dbeta, beta.grad.numpy())
    yi = F.batch_norm(torch.from_numpy(k["x"]).double(), torch.from_numpy(k["rm"]).double(), torch.from_numpy(k["rv"]).double(),
                      gamma.detach(), beta.detach(), training=False, eps=O.EPS)
    close(O.infer64(k["x"], k["gamma"], k["beta"], k["rm"], k["rv"], relu=relu), (yi.relu() if relu else yi).numpy())


@pytest.mark.parametrize("order", ["sequential", "pairwise"])
@pytest.mark.parametrize("shape", O.SHAPES, ids=str)
def test_bounds_admit_fp32_in_any_order(shape, order):
    k = case(shape)
    run = (k["rm"], k["rv"])
    r64 = O.fwd64(k["x"], k["gamma"], k["beta"], relu=True, running=run)
    b = O.fwd_bounds(k["x"], k["gamma"], k["beta"], running=run)
    r32 = O.fwd32(k["x"], k["gamma"], k["beta"], relu=True, running=run, order=order)
    figures = {n: O.worst(r32[n], r64[n], b["var" if n == "var" else n]) for n in ("y", "mean", "var", "rstd", "rm", "rv")}
    a32 = k["gamma"] / np.sqrt(k["rv"] + np.float32(O.EPS))
    yi = O.bf16_round(np.maximum(k["x"] * a32 + (k["beta"] - k["rm"] * a32), np.float32(0)))
    assert yi.dtype == np.float32 and a32.dtype == np.float32
    figures["infer"] = O.worst(yi, O.infer64(k["x"], k["gamma"], k["beta"], k["rm"], k["rv"], relu=True),
                               O.infer_bound(k["x"], k["gamma"], k["beta"], k["rm"], k["rv"]))
    dx, dg, db = O.bwd32(k["dy"], k["x"], k["gamma"], r32["mean"], r32["rstd"], order=order)
    m64, s64 = r32["mean"].astype(np.float64), r32["rstd"].astype(np.float64)
    want = O.bwd64(k["dy"], k["x"], k["gamma"], m64, s64)
    bb = O.bwd_bounds(k["dy"], k["x"], k["gamma"], m64, s64)
    for n, got, w in zip(("dx", "dgamma", "dbeta"), (dx, dg, db), want):
        figures[n] = O.worst(got, w, bb[n])
    print(shape, order, figures)
    assert all(v <= 1.0 for v in figures.values()), figures
    zero = [c for c in range(k["C"]) if O.kind_of(c) == "zero"]
    assert np.array_equal(r32["y"][:, zero], np.broadcast_to(O.bf16_round(np.maximum(k["beta"][zero], 0)), (k["P"], len(zero))))
    assert (dg[zero] == 0).all()


@pytest.mark.parametrize("order", ["sequential", "pairwise"])
@pytest.mark.parametrize("shape", [s for s in O.SHAPES if s[0] >= 65], ids=str)
def test_naive_variance_breaks_the_bound(shape, order):
    """E[x^2] - mu^2 in fp32 on the offset channels (|mean| / std = 128 and 150): x^2 ~ 4096 and ~ 90000 carry absolute
    roundings of ~ 2^-12 and ~ 2^-8 per term against variances of 0.25 and 4.  (At P = 2 and 3 the squares of these bf16 values and their
    sums are exact in fp32, so the naive form is exact there too: those shapes cannot discriminate.)  The bound is a worst-case
    one: its d^2 term grows as P^2 while a pairwise sum's error grows as log P, so at P = 8192 the naive form under PAIRWISE
    summation slips below it (printed, not asserted); summed row after row, as a streaming kernel accumulates, it breaks the
    bound on every shape."""
    k = case(shape)
    v64 = O.fwd64(k["x"], k["gamma"], k["beta"])["var"]
    b = O.fwd_bounds(k["x"], k["gamma"], k["beta"])["var"]
    naive = O.fwd32(k["x"], k["gamma"], k["beta"], order=order, variance="naive")["var"]
    twop = O.fwd32(k["x"], k["gamma"], k["beta"], order=order)["var"]
    offset = [c for c in range(k["C"]) if O.kind_of(c) in ("offset64", "offset-300")]
    q_naive = np.abs(naive[offset] - v64[offset]) / b[offset]
    q_two = np.abs(twop[offset] - v64[offset]) / b[offset]
    print(shape, order, "naive: worst %.3g, fraction of offset channels over the bound %.2f; two-pass worst %.3g"
          % (q_naive.max(), (q_naive > 1).mean(), q_two.max()))
    assert q_two.max() <= 1.0
    if order == "sequential" or shape[0] < 8192:
        assert q_naive.max() > 1.0


def test_graph_structure():
    from ssd_object_detection_amd.resnet_engine import resnet50_ssd512_graph
    g0, gb = resnet50_ssd512_graph(), resnet50_ssd512_graph(batchnorm=True)
    assert g0 == resnet50_ssd512_graph(batchnorm=False)
    count = lambda g, op: sum(nd["op"] == op for nd in g)
    assert (count(g0, "conv"), count(g0, "add"), count(g0, "pool3"), count(g0, "bn"), len(g0)) == (53, 13, 1, 0, 67)
    assert (count(gb, "conv"), count(gb, "add"), count(gb, "pool3"), count(gb, "bn")) == (53, 13, 1, 43)
    assert [nd["cout"] for nd in g0 if nd["feature"]] == [512, 1024, 512, 256, 256, 256, 256]
    assert [nd["cout"] for nd in gb if nd["feature"]] == [512, 1024, 512, 256, 256, 256, 256]
    convs0, convsb = [nd for nd in g0 if nd["op"] == "conv"], [i for i, nd in enumerate(gb) if nd["op"] == "conv"]
    normed = {nd["src"] for nd in gb if nd["op"] == "bn"}
    assert len(normed) == 43 and normed == set(convsb[:43])              # the trunk; the ten extras follow it
    for k, i in enumerate(convsb):
        nd, old = gb[i], convs0[k]
        assert {n: nd[n] for n in ("cin", "cout", "k", "stride")} == {n: old[n] for n in ("cin", "cout", "k", "stride")}
        if i in normed:
            bn = gb[i + 1]
            assert bn["op"] == "bn" and bn["src"] == i and bn["relu"] == old["relu"] and bn["cout"] == nd["cout"] and not nd["relu"]
        else:
            assert nd["relu"] and nd == dict(old, src=nd["src"])
    for i, nd in enumerate(gb):                                          # every reader of a normalised convolution is its bn node
        srcs = nd["src"] if nd["op"] == "add" else (nd["src"],)
        for s in srcs:
            assert s < i and (s not in normed or nd["op"] == "bn")
        if nd["op"] == "add":
            assert all(gb[s]["op"] in ("bn", "add") for s in srcs)


def _random_bn_params(graph, num_priors, classes, g):
    params, running = {}, {}
    for i, nd in enumerate(graph):
        if nd["op"] == "conv":
            fan = nd["k"] * nd["k"] * nd["cin"]
            params["conv%d/kernel" % i] = torch.randn((nd["cout"], nd["k"], nd["k"], nd["cin"]), generator=g, dtype=torch.float64) * (2.0 / fan) ** 0.5
            params["conv%d/bias" % i] = torch.randn((nd["cout"],), generator=g, dtype=torch.float64) * 0.1
        elif nd["op"] == "bn":
            c = nd["cout"]
            params["bn%d/gamma" % i] = 1.0 + 0.3 * torch.randn((c,), generator=g, dtype=torch.float64)
            params["bn%d/beta" % i] = 0.2 * torch.randn((c,), generator=g, dtype=torch.float64)
            running[i] = (0.3 * torch.randn((c,), generator=g, dtype=torch.float64),
                          0.5 + torch.rand((c,), generator=g, dtype=torch.float64))
    for lvl, (nd, n) in enumerate(zip([nd for nd in graph if nd["feature"]], num_priors)):
        params["head%d/kernel" % lvl] = torch.randn((n * (4 + classes), 3, 3, nd["cout"]), generator=g, dtype=torch.float64) * 0.02
        params["head%d/bias" % lvl] = torch.randn((n * (4 + classes),), generator=g, dtype=torch.float64) * 0.1
    return params, running


def test_folding_equals_inference_mode():
    """the real graph at a 64 x 64 input in float64: forward_graph_bn(train=False) == forward_graph on the folded parameters"""
    from oracle import net_oracle as N
    from ssd_object_detection_amd.engine import SSD512_NUM_PRIORS
    from ssd_object_detection_amd.resnet_engine import fold_batchnorm_params, resnet50_ssd512_graph
    g = torch.Generator().manual_seed(11)
    g0, gb = resnet50_ssd512_graph(), resnet50_ssd512_graph(batchnorm=True)
    classes = 5
    params, running = _random_bn_params(gb, SSD512_NUM_PRIORS, classes, g)
    x = torch.randn((2, 64, 64, 8), generator=g, dtype=torch.float64)
    loc, conf, stats = O.forward_graph_bn(gb, SSD512_NUM_PRIORS, classes, params, x, running=running, train=False, emulate_bf16=False)
    assert stats == {}
    order = sorted(running)
    flat = (torch.cat([running[i][0] for i in order]), torch.cat([running[i][1] for i in order]))
    folded = fold_batchnorm_params(gb, params, flat, O.EPS)
    assert sorted(n for n in folded if n.startswith("conv")) == sorted("conv%d/%s" % (i, s) for i, nd in enumerate(g0)
                                                                       if nd["op"] == "conv" for s in ("kernel", "bias"))
    loc_f, conf_f = N.forward_graph(g0, SSD512_NUM_PRIORS, classes, folded, x, emulate_bf16=False)
    for a, b in ((loc, loc_f), (conf, conf_f)):
        assert float(b.abs().max()) > 1e-3 and bool(torch.isfinite(b).all())
        assert float((a - b).norm() / b.norm()) <= 1e-9
    # training mode differs (batch statistics), and reports them
    loc_t, _, stats = O.forward_graph_bn(gb, SSD512_NUM_PRIORS, classes, params, x, running=running, train=True, emulate_bf16=False)
    assert len(stats) == 43 and all(len(v) == 4 for v in stats.values())
    assert float((loc_t - loc).norm() / loc.norm()) > 1e-3


def test_spec():
    from ssd_object_detection_amd.ops import BatchNormSpec
    assert BatchNormSpec.of(None) is None and BatchNormSpec.of(False) is None
    s = BatchNormSpec.of(True)
    assert (s.momentum, s.eps) == (0.1, 1e-5) and BatchNormSpec.of(s) is s
    s = BatchNormSpec.of(dict(momentum=1.0, eps=1e-3))
    assert (s.momentum, s.eps) == (1.0, 1e-3) and repr(s) == "BatchNormSpec(momentum=1.0, eps=0.001)"
    for bad in (dict(momentum=0.0), dict(momentum=1.5), dict(eps=0.0), dict(eps=float("nan")), dict(momentum=True),
                dict(decay=0.9), 0.1, "on"):
        with pytest.raises(ValueError):
            BatchNormSpec.of(bad)


def test_refusals_through_the_c_abi():
    """every refusal is decided on the host, before any launch: callable without a GPU, on pointers that are never dereferenced"""
    from ssd_object_detection_amd import _lib
    L = _lib.lib()
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(10)]
    P, C = 4099, 64
    wsb = L.ssd_bn_ws_bytes(P, C)
    assert wsb > 0 and wsb % (2 * C * 4) == 0
    for c in (0, 32, 96, 100, 2048 + 64, -64):
        assert L.ssd_bn_ws_bytes(P, c) == 0
    assert L.ssd_bn_ws_bytes(0, C) == 0 and L.ssd_bn_ws_bytes(1, C) > 0 and L.ssd_bn_ws_bytes(2, 2048) > 0

    def train(x=p[0], gamma=p[1], beta=p[2], y=p[3], mean=p[4], rstd=p[5], rm=p[6], rv=p[7], momentum=0.1, eps=1e-5, relu=1,
              ws=p[8], ws_bytes=wsb, P=P, C=C):
        return L.ssd_bn_fwd_train(x, gamma, beta, y, mean, rstd, rm, rv, momentum, eps, relu, ws, ws_bytes, P, C, st)

    def infer(x=p[0], gamma=p[1], beta=p[2], rm=p[6], rv=p[7], y=p[3], eps=1e-5, relu=0, P=P, C=C):
        return L.ssd_bn_fwd_infer(x, gamma, beta, rm, rv, y, eps, relu, P, C, st)

    def bwd(dy=p[9], x=p[0], gamma=p[1], mean=p[4], rstd=p[5], dx=p[3], dgamma=p[6], dbeta=p[7], ws=p[8], ws_bytes=wsb, P=P, C=C):
        return L.ssd_bn_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, ws, ws_bytes, P, C, st)

    V, UNS = _lib.SSD_ERR_VALUE, _lib.SSD_ERR_UNSUPPORTED
    for c in (32, 96, 2112):
        assert train(C=c, ws_bytes=0) == UNS and infer(C=c) == UNS and bwd(C=c, ws_bytes=0) == UNS
    assert train(P=1) == V and bwd(P=1) == V and train(P=0) == V and infer(P=0) == V
    for name in ("x", "gamma", "beta", "y", "mean", "rstd", "ws"):
        assert train(**{name: null}) == V, name
    assert train(rm=null) == V and train(rv=null) == V                   # only one of the two running pointers
    for name in ("x", "gamma", "beta", "rm", "rv", "y"):
        assert infer(**{name: null}) == V, name
    for name in ("dy", "x", "gamma", "mean", "rstd", "dx", "dgamma", "dbeta", "ws"):
        assert bwd(**{name: null}) == V, name
    assert train(y=p[0]) == V and infer(y=p[0]) == V                     # y aliases x
    assert bwd(dx=p[0]) == V and bwd(dx=p[9]) == V                       # dx aliases x / dy
    assert train(momentum=0.0) == V and train(momentum=1.5) == V and train(momentum=-0.1) == V
    assert train(eps=0.0) == V and train(eps=-1e-5) == V and infer(eps=0.0) == V
    assert train(ws_bytes=wsb - 1) == V and bwd(ws_bytes=wsb - 1) == V
