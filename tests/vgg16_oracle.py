"""The VGG-16 SSD300 graph (engine.VGG16_SSD300_TRUNK) on the CPU -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

forward()          plain torch, Keras semantics: TF 'SAME' padding made explicit (asymmetric at stride 2), Conv2D(3,
                   dilation_rate=6, padding="same") for fc6, MaxPooling2D(3, strides=1, padding="same") for pool5, the VALID
                   2x2 poolings, optionally the L2 normalisation in front of head 0.  emulate_bf16 rounds every stored map
                   (straight-through), as oracle/net_oracle.forward does; dtype float64 with emulate_bf16=False is the exact walk
                   the forward tolerance is derived from.
backward_chain()   tests/forced_oracle.py's teacher-forced float64 walk for this graph: its T and R modes, its rounding
                   model, its bound (forced_oracle.bounds: 3 * rel_l2(R, T) + 1e-3) and its defects, extended by the two node
                   kinds the VGG-16 trunk adds: a dilated convolution's vjp and the 3x3 / stride-1 un-pooling
                   (strict.ref_unpool(..., 3, 1, 1, 1), code 15 = no gradient).  A pooled activation that also feeds a head
                   (conv4_3) needs nothing new in the walk: add() sums what reaches a map, the head's part first.
Defects used here: ("overwrite", (a, node)), ("no_head", level), ("no_mask", node), ("pool_first", node)."""
import torch
import torch.nn.functional as F

from oracle.net_oracle import _RoundBF16, _same_pad
from tests import strict as S
from tests import l2norm_oracle as LO
from tests.forced_oracle import F64, to_bf16

L2N_EPS = 1e-10


def _node(t):
    kind, cin, cout, k, stride, mode, feat = t[:7]
    return kind, cin, cout, k, stride, mode, feat, (t[7] if len(t) > 7 else 1)


def forward(trunk, num_priors, classes, params, image_nhwc, emulate_bf16=True, dtype=torch.float32, l2norm_scale=None,
            eps=L2N_EPS, keep=None):
    """params: name -> tensor ("conv<node>/kernel" [Cout,k,k,Cin], "conv<node>/bias", "head<level>/kernel|bias").  Returns (loc
    [B,A,4], conf [B,A,classes]) in `dtype`.  keep: a dict that receives node -> stored map (NHWC)."""
    rnd = _RoundBF16.apply if emulate_bf16 else (lambda t: t)
    p = {k: v.to(dtype) for k, v in params.items()}
    x = image_nhwc.to(dtype).permute(0, 3, 1, 2)
    feats = []
    for i, t in enumerate(trunk):
        kind, cin, cout, k, stride, mode, feat, d = _node(t)
        if kind == "conv":
            w, b = p["conv%d/kernel" % i].permute(0, 3, 1, 2), p["conv%d/bias" % i]
            if d != 1:
                assert (k, stride, mode) == (3, 1, "same")
                y = F.conv2d(x, w, b, padding=d, dilation=d)
            else:
                if mode == "same":
                    _, pt, pb = _same_pad(x.shape[2], k, stride)
                    _, pl, pr = _same_pad(x.shape[3], k, stride)
                    x = F.pad(x, (pl, pr, pt, pb))
                y = F.conv2d(x, w, b, stride=stride)
            x = rnd(y.relu())
        elif kind == "pool3s1":
            x = F.max_pool2d(x, 3, 1, padding=1)           # (-inf padding: windows clipped at the edge)
        else:
            assert kind == "pool"
            if mode == "same" and x.shape[2] % 2:
                x = F.pad(x, (0, 1, 0, 1), value=float("-inf"))
            x = F.max_pool2d(x, 2, 2)
        if keep is not None:
            keep[i] = x.permute(0, 2, 3, 1)
        if feat:
            feats.append(x)
    locs, confs = [], []
    B = x.shape[0]
    for lvl, (f, n) in enumerate(zip(feats, num_priors)):
        if lvl == 0 and l2norm_scale is not None:
            r = torch.rsqrt((f * f).sum(1, keepdim=True) + eps)
            f = rnd(f * r * l2norm_scale.to(dtype).view(1, -1, 1, 1))
        y = F.conv2d(F.pad(f, (1, 1, 1, 1)), p["head%d/kernel" % lvl].permute(0, 3, 1, 2), p["head%d/bias" % lvl])
        y = rnd(y).permute(0, 2, 3, 1)
        locs.append(y[..., :n * 4].reshape(B, -1, 4))
        confs.append(y[..., n * 4:].reshape(B, -1, classes))
    return torch.cat(locs, 1), torch.cat(confs, 1)


def conv_vjp(x, w, g, nd, need_dx=True):
    """(dx or None, dw, db) of node nd's convolution against g, float64; dilation from nd["dilation"]"""
    d = nd.get("dilation", 1)
    xr = x.to(F64).detach().requires_grad_(need_dx)
    wr = w.to(F64).detach().requires_grad_(True)
    if d == 1:
        y = S.ref_conv(xr, wr, None, nd["k"], nd["stride"], nd["pt"], nd["pl"], g.shape[1], g.shape[2], False)
    else:
        assert nd["k"] == 3 and nd["stride"] == 1 and nd["pt"] == nd["pl"] == d
        y = F.conv2d(xr.permute(0, 3, 1, 2), wr.permute(0, 3, 1, 2), None, padding=d, dilation=d).permute(0, 2, 3, 1)
    grads = torch.autograd.grad(y, [xr, wr] if need_dx else [wr], g.to(F64))
    return (grads[0] if need_dx else None), grads[-1], g.to(F64).sum((0, 1, 2))


def backward_chain(nodes, fm, num_priors, classes, weights, acts, pool_codes, dloc, dconf, l2norm=None, round_maps=False,
                   defect=None, first_node=0):
    """forced_oracle.backward_chain for SSDEngine.nodes of the VGG-16 trunk (kind conv | pool | pool3s1, `dilation` on the
    convolutions).  Same arguments, same result: {name: float64 tensor} of every parameter gradient and gradient map."""
    rnd = to_bf16 if round_maps else (lambda t: t)
    defect = tuple(defect) if defect else (None, None)
    B = dloc.shape[0]
    G, grads = {}, {}

    def masked(a, g):
        return g * (acts[a] > 0)

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
        normed = l2norm is not None and lvl == 0
        head = dict(k=3, stride=1, pt=1, pl=1)
        dx, dw, db = conv_vjp(l2norm["y"] if normed else acts[a], weights["head%d/kernel" % lvl], dy, head)
        grads["head%d/kernel" % lvl], grads["head%d/bias" % lvl] = dw, db
        dx = masked(a, dx)
        if normed:
            dx = rnd(dx)                                   # the gradient w.r.t. the normalised map is a stored bf16 map
            s = l2norm["scale"].to(F64)
            gx, ds = LO.bwd64(dx.reshape(-1, c).numpy(), acts[a].to(F64).reshape(-1, c).numpy(), s.numpy(), l2norm["eps"])
            grads["l2norm0/scale"] = torch.from_numpy(ds)
            dx = torch.from_numpy(gx).reshape(dx.shape)
        add(a, torch.zeros_like(dx) if defect == ("no_head", lvl) else dx, "head")
    assert off == dloc.shape[1] == dconf.shape[1]

    for i in range(len(nodes) - 1, first_node - 1, -1):
        nd, g = nodes[i], G[i + 1]
        kind = nd["kind"]
        if kind in ("pool", "pool3s1"):
            ks, stride, pad, none = (2, 2, 0, 4) if kind == "pool" else (3, 1, 1, 15)
            code = pool_codes[i]
            if defect == ("pool_first", i):
                code = torch.where(code != none, torch.zeros_like(code), code)
            add(i, S.ref_unpool(code, g, (B, nd["hin"], nd["hin"], nd["cin"]), ks, stride, pad, pad), i)
            continue
        assert kind == "conv"
        dx, dw, db = conv_vjp(acts[i], weights["conv%d/kernel" % i], g, nd, need_dx=i > 0)
        grads["conv%d/kernel" % i], grads["conv%d/bias" % i] = dw, db
        if i == 0:
            continue                                       # no gradient w.r.t. the image
        if nodes[i - 1]["kind"] == "conv" and defect != ("no_mask", i):
            dx = masked(i, dx)                             # (behind a pooling the route alone decides: its code carries the ReLU)
        add(i, dx, i)
    out = dict(grads)
    out.update(("gact%d" % a, g) for a, g in G.items() if a > first_node)
    return out
