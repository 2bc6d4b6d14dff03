"""The MobileNet-v1 SSD300 graph (engine.MOBILENET_V1_SSD300_TRUNK) on the CPU -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

forward()          plain torch, Keras semantics: TF 'SAME' padding made explicit (asymmetric at stride 2 on an even map), a
                   "dwconv" node as F.conv2d(groups=C) on the node's [3][3][C] kernel, ReLU behind every node.  emulate_bf16
                   rounds every stored map (straight-through), as oracle/net_oracle.forward does; float64 with
                   emulate_bf16=False is the exact walk.
backward_chain()   tests/forced_oracle.py's teacher-forced float64 walk in the shape of tests/vgg16_oracle.backward_chain: its T
                   and R modes, its rounding model, its bound (forced_oracle.bounds) and its defects, for the node kinds conv |
                   dwconv.  Every node but the first sits behind a ReLU, so every data gradient is masked by the stored map it
                   flows into; a feature map's gradient is its head's part first, then what the trunk adds.
Defects used here: ("overwrite", (a, node)), ("no_head", level), ("no_mask", node).
alive()            the fraction of positive elements of every stored map: the tests assert that no map of the reduced geometry
                   has died out under the engine's initialisation (a condition on that init, not a measurement)."""
import torch
import torch.nn.functional as F

from oracle.net_oracle import _RoundBF16, _same_pad
from tests.forced_oracle import F64, to_bf16
from tests.vgg16_oracle import conv_vjp

RELU_KINDS = ("conv", "dwconv")


def _padded(x, k, stride):
    _, pt, pb = _same_pad(x.shape[2], k, stride)
    _, pl, pr = _same_pad(x.shape[3], k, stride)
    return F.pad(x, (pl, pr, pt, pb))


def forward(trunk, num_priors, classes, params, image_nhwc, emulate_bf16=True, dtype=torch.float32, keep=None):
    """params: name -> tensor ("conv<node>/kernel" [Cout,k,k,Cin], "dwconv<node>/kernel" [3,3,C], ".../bias",
    "head<level>/kernel|bias").  Returns (loc [B,A,4], conf [B,A,classes]) in `dtype`.  keep: a dict that receives node ->
    stored map (NHWC)."""
    rnd = _RoundBF16.apply if emulate_bf16 else (lambda t: t)
    p = {k: v.to(dtype) for k, v in params.items()}
    x = image_nhwc.to(dtype).permute(0, 3, 1, 2)
    feats = []
    for i, (kind, cin, cout, k, stride, mode, feat) in enumerate(trunk):
        assert mode == "same" and kind in RELU_KINDS
        if kind == "dwconv":
            w = p["dwconv%d/kernel" % i].permute(2, 0, 1).unsqueeze(1)          # [C,1,3,3]
            y = F.conv2d(_padded(x, 3, stride), w, p["dwconv%d/bias" % i], stride=stride, groups=cin)
        else:
            y = F.conv2d(_padded(x, k, stride), p["conv%d/kernel" % i].permute(0, 3, 1, 2), p["conv%d/bias" % i], stride=stride)
        x = rnd(y.relu())
        if keep is not None:
            keep[i] = x.permute(0, 2, 3, 1)
        if feat:
            feats.append(x)
    locs, confs = [], []
    B = x.shape[0]
    for lvl, (f, n) in enumerate(zip(feats, num_priors)):
        y = F.conv2d(F.pad(f, (1, 1, 1, 1)), p["head%d/kernel" % lvl].permute(0, 3, 1, 2), p["head%d/bias" % lvl])
        y = rnd(y).permute(0, 2, 3, 1)
        locs.append(y[..., :n * 4].reshape(B, -1, 4))
        confs.append(y[..., n * 4:].reshape(B, -1, classes))
    return torch.cat(locs, 1), torch.cat(confs, 1)


def alive(keep):
    """node -> fraction of positive elements of its stored map"""
    return {i: float((m > 0).double().mean()) for i, m in keep.items()}


def dw_vjp(x, w, g, nd):
    """(dx, dw [3,3,C], db) of depthwise node nd against g, float64"""
    xr = x.to(F64).detach().requires_grad_(True)
    wr = w.to(F64).detach().requires_grad_(True)
    xp = F.pad(xr.permute(0, 3, 1, 2), (nd["pl"], 2 + (g.shape[2] - 1) * nd["stride"] - x.shape[2] - nd["pl"] + 1,
                                        nd["pt"], 2 + (g.shape[1] - 1) * nd["stride"] - x.shape[1] - nd["pt"] + 1))
    y = F.conv2d(xp, wr.permute(2, 0, 1).unsqueeze(1), None, stride=nd["stride"], groups=x.shape[3]).permute(0, 2, 3, 1)
    assert y.shape == g.shape, (y.shape, g.shape)
    dx, dw = torch.autograd.grad(y, [xr, wr], g.to(F64))
    return dx, dw, g.to(F64).sum((0, 1, 2))


def backward_chain(nodes, fm, num_priors, classes, weights, acts, pool_codes, dloc, dconf, round_maps=False, defect=None, first_node=0):
    """forced_oracle.backward_chain for SSDEngine.nodes of a conv | dwconv trunk.  Same arguments (pool_codes is unused: the
    trunk has no pooling), same result: {name: float64 tensor} of every parameter gradient and gradient map."""
    rnd = to_bf16 if round_maps else (lambda t: t)
    defect = tuple(defect) if defect else (None, None)
    B = dloc.shape[0]
    G, grads = {}, {}

    def add(a, g, writer):
        if a in G and defect != ("overwrite", (a, writer)):
            g = G[a] + g
        G[a] = rnd(g)

    off = 0
    for lvl, ((ni, h, c), n) in enumerate(zip(fm, num_priors)):
        a, cnt = ni + 1, h * h * n
        dy = torch.cat([dloc[:, off:off + cnt].to(F64).reshape(B, h, h, n * 4),
                        dconf[:, off:off + cnt].to(F64).reshape(B, h, h, n * classes)], -1)
        off += cnt
        dx, dw, db = conv_vjp(acts[a], weights["head%d/kernel" % lvl], dy, dict(k=3, stride=1, pt=1, pl=1))
        grads["head%d/kernel" % lvl], grads["head%d/bias" % lvl] = dw, db
        dx = dx * (acts[a] > 0)
        add(a, torch.zeros_like(dx) if defect == ("no_head", lvl) else dx, "head")
    assert off == dloc.shape[1] == dconf.shape[1]

    for i in range(len(nodes) - 1, first_node - 1, -1):
        nd, g = nodes[i], G[i + 1]
        assert nd["kind"] in RELU_KINDS
        if nd["kind"] == "dwconv":
            dx, dw, db = dw_vjp(acts[i], weights["dwconv%d/kernel" % i], g, nd)
            grads["dwconv%d/kernel" % i], grads["dwconv%d/bias" % i] = dw, db
        else:
            dx, dw, db = conv_vjp(acts[i], weights["conv%d/kernel" % i], g, nd, need_dx=i > 0)
            grads["conv%d/kernel" % i], grads["conv%d/bias" % i] = dw, db
        if i == 0:
            continue                                       # no gradient w.r.t. the image
        assert nodes[i - 1]["kind"] in RELU_KINDS
        if defect != ("no_mask", i):
            dx = dx * (acts[i] > 0)
        add(i, dx, i)
    out = dict(grads)
    out.update(("gact%d" % a, g) for a, g in G.items() if a > first_node)
    return out
