"""GPU: the ResNet-50 SSD512 engine with live batch normalisation (ResNet50SSDEngine(batchnorm=...)) at a 256 x 256 input,
batch 2, momentum 1 (one training forward makes the running statistics the batch's): plan, training-mode forward and backward
against the plain-PyTorch restatement (tests/batchnorm_oracle.py:forward_graph_bn) and its autograd, every bn launch on the
operands the engine stored under the oracle's derived bounds, inference mode, folding, modes, checkpoints, a few steps.
No reference counterpart (the reference has neither this network nor batch normalisation).

Bounds.  The per-launch test holds every bn launch to the bounds derived in tests/batchnorm_oracle.py: that is the tight check.
The whole-network comparisons start from the project's figures for this depth (tests/test_resnet_gpu.py: 2e-2 forward; heads
2e-2 / cos 0.999; trunk 0.2 / 0.975, 0.45 / 0.9 on maps narrower than 8).  This network misses them under bf16 storage alone
(measured on an MI355X: training forward 0.060 engine vs restatement, with the restatement WITH against WITHOUT bf16 emulation
at 0.155 on the same input; gradients up to 0.79 against 1.13; DESIGN.md section 2 has the figures and the reason), so each such
bound is max(the project's figure, twice the distance between the two restatements), computed here on the CPU for the same
input and never from the engine's output."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import net_oracle as N                                   # noqa: E402
from tests import batchnorm_oracle as O                              # noqa: E402

IN, B, CLASSES = 256, 2, 81


def rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def ops():
    import ssd_object_detection_amd.ops as ops_
    return ops_


def make_engine(ops, seed, batchnorm=True):
    from ssd_object_detection_amd.resnet_engine import ResNet50SSDEngine
    return ResNet50SSDEngine(classes=CLASSES, in_size=IN, seed=seed,
                             batchnorm=ops.BatchNormSpec(momentum=1.0) if batchnorm else None)


def variables(eng):
    return ([t for i in sorted(eng.conv_params) for t in eng.conv_params[i]] + [t for pair in eng.head_params for t in pair]
            + [t for i in sorted(eng.bn_params) for t in eng.bn_params[i]])


def host_params(eng, grad=False):
    """{name: tensor} as the kernels read them: filters from the bf16 copy, everything else fp32"""
    host, host32 = eng.param_bf16.float().cpu(), eng.param.cpu()
    out = {}
    for t in variables(eng):
        src = host if t.name.endswith("kernel") else host32
        out[t.name] = src[t.offset:t.offset + t.numel].view(t.shape).clone().requires_grad_(grad)
    return out


def running_of(eng):
    rm, rv = eng.bn_running_mean.cpu(), eng.bn_running_var.cpu()
    return {i: (rm[o:o + eng.nodes[i]["cout"]], rv[o:o + eng.nodes[i]["cout"]]) for i, o in eng.bn_off.items()}


@pytest.fixture(scope="module")
def run(ops):
    """One training-mode forward + backward of a batchnorm engine and of the restatement, everything the tests read cloned."""
    from ssd_object_detection_amd.engine import SSD512_NUM_PRIORS
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    eng = make_engine(ops, 5)
    g = torch.Generator().manual_seed(3)
    for gamma, beta in eng.bn_params.values():                          # away from (1, 0): a swapped or dropped gamma / beta shows
        eng.view(gamma, eng.param).copy_(1.0 + 0.1 * torch.randn(gamma.shape, generator=g))
        eng.view(beta, eng.param).copy_(0.1 * torch.randn(beta.shape, generator=g))
    eng.refresh_weights(cast=True)
    x = ops.image_prep(torch.rand((B, IN, IN, 3), generator=g).cuda())
    r = dict(eng=eng, x=x, priors=SSD512_NUM_PRIORS, params=host_params(eng, grad=True))
    loc, conf = eng.forward(x, train=True)
    r["loc"], r["conf"] = loc.float().cpu(), conf.float().cpu()
    dloc = (torch.randn(loc.shape, generator=g) * 1e-3).bfloat16()
    dconf = (torch.randn(conf.shape, generator=g) * 1e-3).bfloat16()
    eng.backward(dloc.cuda(), dconf.cuda())
    torch.cuda.synchronize()
    c = eng._acts(B)
    r["acts"] = [None] + [a.float().cpu() for a in c["acts"][1:]]
    r["gacts"] = [None] + [a.float().cpu() for a in c["gacts"][1:]]
    r["grad"] = eng.grad.cpu().clone()
    r["mean"], r["rstd"] = eng._bn_mean.cpu().clone(), eng._bn_rstd.cpu().clone()
    r["running"] = running_of(eng)
    zero = {i: (torch.zeros(nd["cout"]), torch.ones(nd["cout"])) for i, nd in enumerate(eng.graph) if nd["op"] == "bn"}
    loc_r, conf_r, stats = O.forward_graph_bn(eng.graph, SSD512_NUM_PRIORS, CLASSES, r["params"], x.float().cpu(), running=zero,
                                              train=True, emulate_bf16=True, momentum=1.0)
    (loc_r * dloc.float()).sum().add((conf_r * dconf.float()).sum()).backward()
    r["loc_r"], r["conf_r"], r["stats"] = loc_r.detach(), conf_r.detach(), stats
    # the same restatement WITHOUT the bf16 rounding of the stored maps, same input, parameters and upstream gradient: its
    # distance from the rounded one is what bf16 storage alone does to this network (the yardstick of the bounds below)
    r["params_x"] = {n: t.detach().clone().requires_grad_(True) for n, t in r["params"].items()}
    loc_x, conf_x, _ = O.forward_graph_bn(eng.graph, SSD512_NUM_PRIORS, CLASSES, r["params_x"], x.float().cpu(), running=zero,
                                          train=True, emulate_bf16=False, momentum=1.0)
    (loc_x * dloc.float()).sum().add((conf_x * dconf.float()).sum()).backward()
    r["loc_x"], r["conf_x"] = loc_x.detach(), conf_x.detach()
    return r


def test_plan(ops, run):
    eng = run["eng"]
    plain = make_engine(ops, 5, batchnorm=False)
    assert len(eng.tensors) == len(plain.tensors) + 86
    extra = eng.tensors[-86:]
    bn_nodes = [i for i, nd in enumerate(eng.nodes) if nd["kind"] == "bn"]
    assert len(bn_nodes) == 43
    assert [t.name for t in extra] == [n for i in bn_nodes for n in ("bn%d/gamma" % i, "bn%d/beta" % i)]
    assert not any(t.name.startswith("bn") for t in eng.tensors[:-86])
    assert eng.bn_running_mean.numel() == eng.bn_running_var.numel() == sum(eng.nodes[i]["cout"] for i in bn_nodes)
    # the default engine: the names, offsets and state_dict keys of the parent commit (no bn anywhere)
    from ssd_object_detection_amd.resnet_engine import resnet50_ssd512_graph
    assert plain.graph == resnet50_ssd512_graph() and plain.batchnorm is None
    names = ["conv%d/%s" % (i, s) for i, nd in enumerate(plain.graph) if nd["op"] == "conv" for s in ("kernel", "bias")]
    names += ["head%d/%s" % (l, s) for l in range(7) for s in ("loc_kernel", "conf_kernel", "loc_bias", "conf_bias")]
    assert [t.name for t in plain.tensors] == names
    off = 0
    for t in plain.tensors:                                             # every variable alone in its optimizer blocks, in order
        assert t.block0 * plain.block == off and off <= t.offset and t.offset + t.numel <= off + t.nblocks * plain.block
        off += t.nblocks * plain.block
    assert off == plain.n_flat
    assert sorted(plain.state_dict()) == sorted(["param", "adam_m", "adam_v", "step", "names", "shapes", "offsets",
                                                  "layout_version", "slots"])
    assert sorted(set(eng.state_dict()) - set(plain.state_dict())) == ["bn", "bn_running_mean", "bn_running_var"]
    assert eng.state_dict()["bn"] == dict(momentum=1.0, eps=1e-5)
    # in a batchnorm engine the variables of the convolutions and heads keep their shapes and order, bn variables behind them
    assert [(t.shape, t.index) for t in eng.tensors[:-86]] == [(t.shape, t.index) for t in plain.tensors]
    assert [t.offset for t in eng.tensors[:-86]] == [t.offset for t in plain.tensors]
    dec = eng.decay_table(5e-4, False).cpu()
    assert all(float(dec[t.index]) == 0.0 for t in extra) and float(eng.decay_table(5e-4, True).cpu()[extra[0].index]) > 0


def test_training_forward_vs_restatement(run):
    fl, fc = rel_l2(run["loc"], run["loc_r"]), rel_l2(run["conf"], run["conf_r"])
    ol, oc = rel_l2(run["loc_r"], run["loc_x"]), rel_l2(run["conf_r"], run["conf_x"])
    print("training-mode forward, relative L2: engine vs restatement loc %.4g conf %.4g; restatement with vs without bf16 "
          "emulation loc %.4g conf %.4g" % (fl, fc, ol, oc))
    assert run["loc"].shape == (B, run["eng"].A, 4)
    assert fl < max(2e-2, 2 * ol) and fc < max(2e-2, 2 * oc)


def test_every_bn_launch_on_its_own_operands(run):
    """mean, rstd, y and the running update recomputed in float64 from the convolution output the engine stored; dx, dgamma,
    dbeta from the gradient map the engine stored (an un-ReLU'd bn node reads its add's) -- under the oracle's bounds"""
    eng = run["eng"]
    gsrc = {}                                                           # bn node -> the node whose gradient buffer it reads
    for k, nd in enumerate(eng.nodes):
        if nd["kind"] == "add":
            for s in nd["src"]:
                if eng.nodes[s]["kind"] == "bn" and not eng.nodes[s]["relu"]:
                    gsrc[s] = k
    worst = {}
    for i, o in eng.bn_off.items():
        nd = eng.nodes[i]
        C, conv = nd["cout"], nd["src"]
        x = run["acts"][conv + 1].reshape(-1, C).numpy()
        P = x.shape[0]
        assert P == B * nd["hout"] ** 2
        gamma, beta = (run["params"]["bn%d/%s" % (i, s)].detach().numpy() for s in ("gamma", "beta"))
        zero, one = np.zeros(C, np.float32), np.ones(C, np.float32)
        r = O.fwd64(x, gamma, beta, relu=nd["relu"], running=(zero, one), momentum=1.0)
        b = O.fwd_bounds(x, gamma, beta, running=(zero, one), momentum=1.0)
        mean, rstd = run["mean"][o:o + C].numpy().astype(np.float64), run["rstd"][o:o + C].numpy().astype(np.float64)
        got = dict(mean=mean, rstd=rstd, y=run["acts"][i + 1].reshape(-1, C).numpy(), rm=run["running"][i][0].numpy(),
                   rv=run["running"][i][1].numpy())
        fig = {n: O.worst(got[n], r[n], b[n]) for n in got}
        dy = run["gacts"][gsrc.get(i, i) + 1].reshape(-1, C).numpy()
        if nd["relu"]:
            assert not (dy[got["y"] <= 0] != 0).any(), "bn%d: its gradient map is not masked by its own ReLU" % i
        want = O.bwd64(dy, x, gamma, mean, rstd)
        bb = O.bwd_bounds(dy, x, gamma, mean, rstd)
        tg, tb = eng.bn_params[i]
        gotb = (run["gacts"][conv + 1].reshape(-1, C).numpy(), run["grad"][tg.offset:tg.offset + C].numpy(),
                run["grad"][tb.offset:tb.offset + C].numpy())
        for n, gv, w in zip(("dx", "dgamma", "dbeta"), gotb, want):
            fig[n] = O.worst(gv, w, bb[n])
            assert np.abs(w).max() > 0, (i, n)
        for n, v in fig.items():
            worst[n] = max(worst.get(n, 0.0), v)
        assert all(v <= 1.0 for v in fig.values()), (i, nd, fig)
    print("worst |error| / bound over the 43 bn nodes:", {n: round(v, 4) for n, v in worst.items()})


def test_normalised_biases_never_move(ops):
    eng = make_engine(ops, 7)
    g = torch.Generator().manual_seed(9)
    x = ops.image_prep(torch.rand((B, IN, IN, 3), generator=g).cuda())
    loc, conf = eng.forward(x, train=True)
    eng.backward((torch.randn(loc.shape, generator=g) * 1e-3).bfloat16().cuda(), (torch.randn(conf.shape, generator=g) * 1e-3).bfloat16().cuda())
    biases = [eng.conv_params[i][1] for i in sorted(eng.bn_convs)]
    assert len(biases) == 43
    other = [eng.conv_params[i][1] for i in sorted(eng.conv_params) if i not in eng.bn_convs]
    assert all(float(eng.view(t, eng.grad).abs().max()) > 0 for t in other)            # the extras' biases do get gradients
    before = [eng.view(t, eng.param).clone() for t in biases]
    moved = eng.view(eng.bn_params[min(eng.bn_params)][1], eng.param).clone()
    for t in biases:
        assert float(eng.view(t, eng.grad).abs().max()) == 0.0, t.name
    eng.clip_scales(0.01)
    eng.adam(1e-3, eng.grad, 1.0, True)
    eng.sgd_momentum(1e-3, eng.grad, 1.0, True, momentum=0.9, decay=eng.decay_table(5e-4, True))
    torch.cuda.synchronize()
    for t, b0 in zip(biases, before):
        assert torch.equal(eng.view(t, eng.param).view(torch.int32), b0.view(torch.int32)), t.name
    assert not torch.equal(eng.view(eng.bn_params[min(eng.bn_params)][1], eng.param), moved)   # a beta does move


def test_whole_network_gradients_vs_autograd(run):
    eng, gflat = run["eng"], run["grad"]
    worst, rows = {}, []
    for t in variables(eng):
        got, want = gflat[t.offset:t.offset + t.numel].view(t.shape), run["params"][t.name].grad
        if t.name.startswith("conv") and t.name.endswith("bias") and int(t.name[4:].split("/")[0]) in eng.bn_convs:
            assert float(got.abs().max()) == 0.0                        # (autograd's is zero up to roundoff; never written here)
            continue
        err = rel_l2(got, want)
        cos = float((got * want).sum() / (got.norm() * want.norm() + 1e-30))
        exact = run["params_x"][t.name].grad
        oerr, ocos = rel_l2(want, exact), float((want * exact).sum() / (want.norm() * exact.norm() + 1e-30))
        print("%-18s rel L2 err %.4f  cos %.5f | restatement with vs without bf16 emulation %.4f  %.5f" % (t.name, err, cos, oerr, ocos))
        if t.name.startswith("head"):
            tol, cmin, kind = 2e-2, 0.999, "heads"
        else:
            node = int(re.sub(r"\D", "", t.name.split("/")[0]))
            small = eng.nodes[node]["hout"] < 8
            tol, cmin = (0.45, 0.9) if small else (0.2, 0.975)
            kind = ("bn" if t.name.startswith("bn") else "conv") + (" (small maps)" if small else "")
        w = worst.setdefault(kind, [0.0, 1.0, 0.0, 1.0])
        w[0], w[1], w[2], w[3] = max(w[0], err), min(w[1], cos), max(w[2], oerr), min(w[3], ocos)
        # the project's figures, or twice the restatement's own distance under bf16 storage where that is larger
        tol, cmin = max(tol, 2 * oerr), min(cmin, 1 - 2 * (1 - ocos))
        if not (err < tol and cos > cmin):
            rows.append((t.name, err, cos, tol, cmin))
    print("worst per class (engine: relative L2, cosine; restatement with vs without bf16 emulation: the same):", worst)
    assert not rows, rows


def test_inference_and_folding(ops, run):
    eng, x = run["eng"], run["x"]
    loc, conf = (t.float().cpu() for t in eng.forward(x))
    params = {n: t.detach() for n, t in run["params"].items()}
    with torch.no_grad():
        loc_r, conf_r, _ = O.forward_graph_bn(eng.graph, run["priors"], CLASSES, params, x.float().cpu(), running=run["running"],
                                              train=False, emulate_bf16=True)
        loc_x, conf_x, _ = O.forward_graph_bn(eng.graph, run["priors"], CLASSES, params, x.float().cpu(), running=run["running"],
                                              train=False, emulate_bf16=False)
    fi = (rel_l2(loc, loc_r), rel_l2(conf, conf_r))
    oo = (rel_l2(loc_r, loc_x), rel_l2(conf_r, conf_x))
    print("inference forward, relative L2: engine vs restatement %s; restatement with vs without bf16 emulation %s" % (fi, oo))
    assert fi[0] < max(2e-2, 2 * oo[0]) and fi[1] < max(2e-2, 2 * oo[1]), (fi, oo)
    fold = eng.folded()
    assert fold.batchnorm is None and [t.shape for t in fold.tensors] == [t.shape for t in eng.tensors[:-86]]
    lf, cf = (t.float().cpu() for t in fold.forward(x))
    ff = (rel_l2(lf, loc), rel_l2(cf, conf))
    # the folded engine is a default engine: against forward_graph on ITS parameters it meets the folded network's own figure
    fh, fh32 = fold.param_bf16.float().cpu(), fold.param.cpu()
    fparams = {}
    for t in [t for i in sorted(fold.conv_params) for t in fold.conv_params[i]] + [t for pair in fold.head_params for t in pair]:
        fparams[t.name] = (fh if t.name.endswith("kernel") else fh32)[t.offset:t.offset + t.numel].view(t.shape)
    with torch.no_grad():
        lfr, cfr = N.forward_graph(fold.graph, run["priors"], CLASSES, fparams, x.float().cpu())
        lfx, cfx = N.forward_graph(fold.graph, run["priors"], CLASSES, fparams, x.float().cpu(), emulate_bf16=False)
    fr, fo = (rel_l2(lf, lfr), rel_l2(cf, cfr)), (rel_l2(lfr, lfx), rel_l2(cfr, cfx))
    print("folded engine vs forward_graph on the folded parameters %s; forward_graph with vs without bf16 emulation %s" % (fr, fo))
    assert fr[0] < max(2e-2, 2 * fo[0]) and fr[1] < max(2e-2, 2 * fo[1]), (fr, fo)
    print("inference vs restatement %s; folded vs batchnorm engine %s" % (fi, ff))
    assert ff[0] < 2 * max(2e-2, 2 * oo[0]) and ff[1] < 2 * max(2e-2, 2 * oo[1]), (ff, oo)      # the triangle inequality
    l8, c8 = fold.forward(x, "mxfp8")
    assert bool(torch.isfinite(l8.float()).all()) and bool(torch.isfinite(c8.float()).all())
    assert rel_l2(l8.float().cpu(), lf) < 1.0                            # the fp8 path computes the same network


def test_modes_and_state(ops, run):
    eng, x = run["eng"], run["x"]
    loc, conf = (t.clone() for t in eng.forward(x))
    dloc, dconf = torch.zeros_like(loc), torch.zeros_like(conf)
    with pytest.raises(RuntimeError):
        eng.backward(dloc, dconf)
    with pytest.raises(ValueError):
        eng.forward(x, "mxfp8")
    with pytest.raises(ValueError):
        eng.forward(x, "mxfp8", train=True)
    sd = eng.state_dict()
    fresh = make_engine(ops, 23)
    assert not torch.equal(fresh.forward(x)[0], loc)
    fresh.load_state_dict(sd)
    l2, c2 = fresh.forward(x)
    assert torch.equal(l2, loc) and torch.equal(c2, conf)
    plain = make_engine(ops, 5, batchnorm=False)
    with pytest.raises(ValueError):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError):
        fresh.load_state_dict(plain.state_dict())
    with pytest.raises(ValueError):
        plain.folded()


def test_a_few_training_steps(ops):
    """eight steps of forward(train=True), ssd_loss_heads, backward, clip, Adam on one fixed synthetic batch"""
    from ssd_object_detection_amd.data_loaders.synthetic import synth_batch_gt
    eng = make_engine(ops, 17)
    s_ref = tuple(v * IN / 512.0 for v in (20, 51, 133, 215, 297, 379, 461, 543))       # bench.py's cfg5 scales at this input
    ps = ops.build_priors(grids=eng.grids, s_ref=s_ref, ratios=((2,), (2, 3), (2, 3), (2, 3), (2, 3), (2,), (2,)), in_size=IN)
    assert ps.A == eng.A
    cls_l, box_l = synth_batch_gt(0, B)
    tgt = ops.match_encode(*ops.pack_gt(box_l, cls_l), ps, 0.5)
    img = ops.image_prep(torch.rand((B, IN, IN, 3), generator=torch.Generator().manual_seed(21)).cuda(), normalize=True)
    losses = []
    for _ in range(8):
        ploc, pconf = eng.forward(img, train=True)
        hg = eng.head_grad_buffers(B)
        out8 = ops.ssd_loss_heads(pconf, ploc, *tgt, hg)
        eng.backward(None, None, heads=hg)
        eng.clip_scales(0.01)
        eng.adam(1e-3, eng.grad, 1.0, True)
        losses.append(float(out8[3]))
    print("loss over eight steps:", ["%.4f" % v for v in losses])
    assert all(np.isfinite(losses)) and losses[7] < losses[0], losses
    assert bool(torch.isfinite(eng.param).all()) and bool(torch.isfinite(eng.bn_running_var).all())
