"""CPU: the teacher-forced oracle (tests/forced_oracle.py) tested on its own, on two tiny float64 networks with their own
forward pass: with the masks and routes of that forward, the exact walk (T) IS torch.autograd's gradient of the same network
(1e-10 relative L2 per tensor: float64 summation order, not a tolerance on any kernel); the storage model (R) moves every trunk
tensor and leaves every level's head alone; every seeded defect moves a tensor it touches beyond twice that tensor's bound.
A third network, the graph with 128-channel maps ("graph_mx": the product's mxfp8_dgrad_eligible holds on it as it stands),
does the same for the walk's mx= mode: handed its own exact maps and unquantised filters it is still autograd's gradient;
handed quantised operands it moves every tensor below the first fp8 data gradient and nothing above; every graph defect and
the two fp8 ones move a tensor beyond twice its bound."""
import pytest

torch = pytest.importorskip("torch")

from tests import strict as S                                        # noqa: E402
from tests import forced_oracle as FO                                # noqa: E402

F64 = torch.float64
CLASSES = 3
# the SSD300 node kinds: SAME / VALID 3x3, 1x1, stride 2, a VALID pooling of an odd map (23 -> 11), a SAME one (11 -> 6), each
# behind a convolution; three feature levels 6, 3, 1; node 1 and node 6 keep the shape (the "mask_output" defect)
CHAIN = [("conv", 8, 8, 3, 1, "same", False), ("conv", 8, 8, 3, 1, "same", False), ("pool", 8, 8, 2, 2, "valid", False),
         ("conv", 8, 16, 3, 1, "same", False), ("pool", 16, 16, 2, 2, "same", False), ("conv", 16, 16, 3, 1, "same", False),
         ("conv", 16, 16, 1, 1, "same", True), ("conv", 16, 16, 3, 2, "same", True), ("conv", 16, 8, 1, 1, "same", False),
         ("conv", 8, 16, 3, 1, "valid", True)]
CHAIN_SIZE, CHAIN_PRIORS = 23, (2, 3, 2)


def chain_nodes():
    nodes, fm, s = [], [], CHAIN_SIZE
    for kind, cin, cout, k, stride, mode, feat in CHAIN:
        ho, _, pt, _ = S.geometry(s, s, k, stride, mode)
        if kind == "pool" and mode == "same":
            ho, pt = (s + 1) // 2, 0
        nodes.append(dict(kind=kind, cin=cin, cout=cout, k=k, stride=stride, pt=pt, pl=pt, hin=s, hout=ho, feature=feat))
        s = ho
        if feat:
            fm.append((len(nodes) - 1, ho, cout))
    return nodes, fm


def graph_nodes(mid=8, wide=16):
    """stem 7x7/2 (33 -> 17), 3x3/2 pooling (-> 9), a bottleneck with a projection and stride 2 (-> 5, feature map 0, which also
    feeds the next block twice), one with an identity shortcut (feature map 1), an extra stage (-> 3, feature map 2); `mid`
    channels inside the blocks, `wide` at their outputs"""
    g = []

    def conv(src, cin, cout, k, stride, relu=True, feature=False):
        g.append(dict(kind="conv", src=src, cin=cin, cout=cout, k=k, stride=stride, relu=relu, feature=feature))
        return len(g) - 1

    x = conv(-1, 8, mid, 7, 2)
    g.append(dict(kind="pool3", src=x, cin=mid, cout=mid, k=3, stride=2, relu=False, feature=False))
    x = 1
    a = conv(conv(conv(x, mid, mid, 1, 1), mid, mid, 3, 2), mid, wide, 1, 1, relu=False)
    sc = conv(x, mid, wide, 1, 2, relu=False)
    g.append(dict(kind="add", src=(a, sc), cin=wide, cout=wide, k=0, stride=1, relu=True, feature=True))
    x = len(g) - 1
    a = conv(conv(conv(x, wide, mid, 1, 1), mid, mid, 3, 1), mid, wide, 1, 1, relu=False)
    g.append(dict(kind="add", src=(a, x), cin=wide, cout=wide, k=0, stride=1, relu=True, feature=True))
    x = len(g) - 1
    conv(conv(x, wide, mid, 1, 1), mid, wide, 3, 2, feature=True)
    sizes, fm = {-1: 33}, []
    for i, nd in enumerate(g):
        hin = sizes[nd["src"][0] if nd["kind"] == "add" else nd["src"]]
        ho, pt = (hin, 0) if nd["kind"] == "add" else S.geometry(hin, hin, nd["k"], nd["stride"], "same")[::2]
        sizes[i] = ho
        nd.update(hin=hin, hout=ho, pt=pt, pl=pt)
        if nd["feature"]:
            fm.append((i, ho, nd["cout"]))
    return g, fm


def make_params(nodes, fm, priors, g):
    P = {}
    for i, nd in enumerate(nodes):
        if nd["kind"] == "conv":
            fan = nd["k"] ** 2 * nd["cin"]
            P["conv%d/kernel" % i] = torch.randn((nd["cout"], nd["k"], nd["k"], nd["cin"]), generator=g, dtype=F64) * (2.0 / fan) ** 0.5
            P["conv%d/bias" % i] = torch.randn((nd["cout"],), generator=g, dtype=F64) * 0.1
    for lvl, ((_, _, c), n) in enumerate(zip(fm, priors)):
        P["head%d/kernel" % lvl] = torch.randn((n * (4 + CLASSES), 3, 3, c), generator=g, dtype=F64) * (1.0 / (9 * c)) ** 0.5
        P["head%d/bias" % lvl] = torch.randn((n * (4 + CLASSES),), generator=g, dtype=F64) * 0.1
    return {k: v.requires_grad_(True) for k, v in P.items()}


def forward(nodes, fm, priors, P, x, scale=None, eps=1e-10):
    """The network's own float64 forward, with autograd: (loc, conf, activations, pre-activations, codes, normalised map)"""
    acts, pre, codes = [x], [None], {}
    for i, nd in enumerate(nodes):
        src = nd.get("src", i - 1)
        if nd["kind"] == "conv":
            y = S.ref_conv(acts[src + 1], P["conv%d/kernel" % i], P["conv%d/bias" % i], nd["k"], nd["stride"], nd["pt"], nd["pl"],
                           nd["hout"], nd["hout"], False)
        elif nd["kind"] == "add":
            y = acts[src[0] + 1] + acts[src[1] + 1]
        else:
            ks, none = (2, 4) if nd["kind"] == "pool" else (3, 15)
            y, codes[i] = S.ref_pool(acts[src + 1], ks, 2, nd["pt"], nd["pl"], nd["hout"], nd["hout"], none)
        y.retain_grad()
        pre.append(y)
        acts.append(y.relu() if nd.get("relu", nd["kind"] == "conv") else y)
    locs, confs, y0 = [], [], None
    B = x.shape[0]
    for lvl, ((ni, h, c), n) in enumerate(zip(fm, priors)):
        f = acts[ni + 1]
        if scale is not None and lvl == 0:
            f = y0 = scale * f * torch.rsqrt((f * f).sum(-1, keepdim=True) + eps)
        y = S.ref_conv(f, P["head%d/kernel" % lvl], P["head%d/bias" % lvl], 3, 1, 1, 1, h, h, False)
        locs.append(y[..., :n * 4].reshape(B, -1, 4))
        confs.append(y[..., n * 4:].reshape(B, -1, CLASSES))
    return torch.cat(locs, 1), torch.cat(confs, 1), acts, pre, codes, y0


class Net:
    """One tiny network, its forward and autograd's gradients, and the oracle's T and R on that forward's masks and routes"""

    def __init__(self, kind, l2norm=False, drop_fullres=False, seed=0):
        g = torch.Generator().manual_seed(seed)
        graph = {"graph": graph_nodes, "graph_mx": lambda: graph_nodes(128, 128)}
        (self.nodes, self.fm), self.priors = (chain_nodes(), CHAIN_PRIORS) if kind == "chain" else (graph[kind](), (2, 2, 2))
        size = CHAIN_SIZE if kind == "chain" else 33
        self.P = make_params(self.nodes, self.fm, self.priors, g)
        x = torch.randn((2, size, size, 8), generator=g, dtype=F64)
        c0 = self.fm[0][2]
        scale = None
        if l2norm:
            scale = (2.0 + 0.5 * torch.randn(c0, generator=g, dtype=F64))
            scale[3] = -scale[3].abs()
            scale.requires_grad_(True)
        loc, conf, acts, pre, codes, y0 = forward(self.nodes, self.fm, self.priors, self.P, x, scale)
        self.dloc, self.dconf = torch.randn(loc.shape, generator=g, dtype=F64), torch.randn(conf.shape, generator=g, dtype=F64)
        ((loc * self.dloc).sum() + (conf * self.dconf).sum()).backward()
        self.auto = {k: v.grad for k, v in self.P.items()}
        self.auto.update(("gact%d" % a, pre[a].grad) for a in range(1, len(pre)))
        if l2norm:
            self.auto["l2norm0/scale"] = scale.grad
        self.acts = [a.detach() for a in acts]
        if drop_fullres:                                   # as the engine's pool_only: the map in front of a pooling is not stored
            for i, nd in enumerate(self.nodes):
                if nd["kind"] == "pool":
                    self.acts[i] = None
        self.codes = codes
        self.l2norm = dict(scale=scale.detach(), y=y0.detach(), eps=1e-10) if l2norm else None
        self.weights = {k: v.detach() for k, v in self.P.items()}
        self.chain = kind == "chain"
        self.T, self.R = self.run(), self.run(round_maps=True)
        self.bound = FO.bounds(self.T, self.R)

    def run(self, **kw):
        args = (self.nodes, self.fm, self.priors, CLASSES, self.weights, self.acts, self.codes, self.dloc, self.dconf)
        return FO.backward_chain(*args, l2norm=self.l2norm, **kw) if self.chain else FO.backward_graph(*args, **kw)


NETS = {}


def net(*key):
    if key not in NETS:
        NETS[key] = Net(*key)
    return NETS[key]


@pytest.mark.parametrize("key", [("chain",), ("chain", True), ("chain", True, True), ("graph",), ("graph_mx",)])
def test_exact_walk_is_autograd(key):
    n = net(*key)
    assert set(n.T) == set(n.auto)
    for name, want in n.auto.items():
        assert float(want.norm()) > 0, name
        assert FO.rel_l2(n.T[name], want) <= 1e-10, (name, FO.rel_l2(n.T[name], want))


@pytest.mark.parametrize("key", [("chain",), ("chain", True), ("graph",), ("graph_mx",)])
def test_storage_model_moves_the_trunk_only(key):
    n = net(*key)
    for name in n.T:
        err = FO.rel_l2(n.R[name], n.T[name])
        if name.startswith("head"):                         # every level's head reads dy and a stored map: no rounded gradient map
            assert err == 0.0, (name, err)
        elif name.startswith(("conv", "gact")):
            assert 0.0 < err < 0.1, (name, err)            # bf16 roundings a handful deep; a bias gradient is a sum that cancels
        else:
            assert name == "l2norm0/scale" and 0.0 < err < 0.1, (name, err)   # (it reads the rounded gradient w.r.t. the normalised map)


def test_codes_unpack_as_they_pack():
    g = torch.Generator().manual_seed(3)
    for top in (4, 15):                                     # 2x2 codes 0 .. 3 and none = 4; 3x3 codes 0 .. 8 and none = 15
        code = torch.randint(0, top + 1, (2, 5, 7, 16), generator=g)
        code[0, 0, 0] = top
        code[1, 4, 6] = torch.tensor([top, 0] * 8)          # a word whose highest nibble is set and one whose is not
        packed = S.pack_codes(code)
        assert packed.dtype == torch.int32 and packed.shape == (2, 5, 7, 2)
        assert torch.equal(FO.unpack_codes(packed), code)
        assert int(packed.min()) < 0 or top == 4            # (15 in the top nibble makes the int32 word negative)


CHAIN_DEFECTS = [("no_head", 0), ("no_head", 1), ("no_head", 2), ("mask_output", 1), ("no_mask", 1), ("mask_output", 6), ("no_mask", 6),
                 ("no_mask", 9), ("pool_first", 2), ("pool_first", 4), ("pool_pitch", 2), ("wgrad_before_head", 1), ("l2norm_scale_only", None),
                 ("overwrite", (7, 7))]
GRAPH_DEFECTS = [("no_head", 0), ("no_head", 1), ("no_head", 2), ("mask_output", 8), ("no_mask", 8), ("pool_first", 1), ("wgrad_before_head", 2),
                 ("no_identity", 10), ("no_projection", 6), ("no_shortcut_mask", 10), ("overwrite", (7, 7))]


@pytest.mark.parametrize("kind,defect", [("chain", d) for d in CHAIN_DEFECTS] + [("graph", d) for d in GRAPH_DEFECTS], ids=str)
def test_seeded_defect_moves_the_exact_walk(kind, defect):
    n = net("chain", True) if kind == "chain" else net("graph")
    D = n.run(defect=defect)
    hit = FO.moved(n.T, D, n.bound)
    print(defect, sorted(hit, key=lambda r: -r[1] / r[2])[:4])
    assert hit, (defect, "moves no tensor to twice its bound")
    untouched = [k for k in n.T if FO.rel_l2(D[k], n.T[k]) == 0.0]
    assert untouched, defect                               # ONE wiring error: what lies behind it in the walk stays exact


# ---- the mx= mode, on the graph with 128-channel maps ----------------------------------------------------------------------
MX_NET = {}
MX_DEFECTS = GRAPH_DEFECTS + [("mx_wrong_dy", 4), ("mx_wrong_dy", 9), ("mx_stale_dy", 6), ("mx_stale_dy", 10)]


def mx_net():
    """The network, the fp8 data gradients the product's rule gives it, the roots the walk derived, and T / R under mx with
    operands quantised (strict.ref_quantize_mx) from the network's own R maps and filters"""
    if not MX_NET:
        from ssd_object_detection_amd.resnet_engine import mxfp8_dgrad_eligible, mxfp8_bwd_plan
        n = net("graph_mx")
        dgrad = {i for i, nd in enumerate(n.nodes) if mxfp8_dgrad_eligible(nd)}
        trace = {}
        again = n.run(trace=trace)
        assert all(torch.equal(again[k], n.T[k]) for k in n.T)             # (trace changes nothing)
        root = trace["root"]
        plan = mxfp8_bwd_plan(n.nodes)
        assert plan[0] == dgrad == {2, 4, 7, 8, 9, 11} and list(plan[1]) == root, (dgrad, root)
        roots = sorted({root[i] for i in dgrad})
        assert roots == sorted(plan[2]) == [2, 6, 7, 8, 10, 11]
        # feature map 0 (node 6): written by its head, by the identity shortcut of add 10 and last by fp8 data gradient 7
        assert n.nodes[6]["feature"] and n.nodes[10]["src"][1] == 6 and n.nodes[7]["src"] == 6 and plan[2][6] == ("fp8", 7)
        mx = dict(dgrad=dgrad, dy={r: FO.mx_round(n.R["gact%d" % (r + 1)]) for r in roots},
                  wt={i: FO.mx_filters(n.weights["conv%d/kernel" % i]) for i in dgrad})
        T, R = n.run(mx=mx), n.run(mx=mx, round_maps=True)
        MX_NET.update(n=n, dgrad=dgrad, roots=roots, mx=mx, T=T, R=R, bound=FO.bounds(T, R))
    return MX_NET


def test_mx_walk_on_exact_operands_is_autograd():
    m = mx_net()
    n = m["n"]
    mx = dict(dgrad=m["dgrad"], dy={r: n.T["gact%d" % (r + 1)] for r in m["roots"]},
              wt={i: n.weights["conv%d/kernel" % i] for i in m["dgrad"]})
    T = n.run(mx=mx)
    assert set(T) == set(n.auto)
    for name, want in n.auto.items():
        assert FO.rel_l2(T[name], want) <= 1e-10, (name, FO.rel_l2(T[name], want))


def test_mx_operands_move_what_lies_below_them():
    m = mx_net()
    n, top = m["n"], max(m["dgrad"])                        # the first fp8 data gradient of the walk: the extra stage's 1x1,
    for name in n.T:                                        # in the network's linear tail, so every earlier node lies below it
        err = FO.rel_l2(m["T"][name], n.T[name])
        idx = int(name.split("/")[0][4:])                   # "conv7/kernel" -> node 7, "gact7" -> activation 7 = node 6's output
        if (name.startswith("conv") and idx < top) or (name.startswith("gact") and idx <= top):
            assert 0.0 < err < 0.2, (name, err)            # e4m3 operands: 2^-4 per element at the worst
        else:
            assert err == 0.0, (name, err)
    assert {k for k in n.T if k.startswith("head")} and FO.rel_l2(m["T"]["gact%d" % (top + 2)], n.T["gact%d" % (top + 2)]) == 0.0


@pytest.mark.parametrize("defect", MX_DEFECTS, ids=str)
def test_seeded_defect_moves_the_mx_walk(defect):
    m = mx_net()
    D = m["n"].run(mx=m["mx"], defect=defect)
    hit = FO.moved(m["T"], D, m["bound"])
    print(defect, sorted(hit, key=lambda r: -r[1] / r[2])[:4])
    assert hit, (defect, "moves no tensor to twice its bound")
    untouched = [k for k in m["T"] if FO.rel_l2(D[k], m["T"][k]) == 0.0]
    assert untouched, defect


def test_engine_tells_same_from_valid_pooling():
    """SSDEngine took `hout * 2 != hin` for "SAME": true for a VALID pooling of an odd map too (87 -> 43), whose kernels then
    wrote 44 x 44 windows into buffers planned for 43 x 43.  The flag, on the planned nodes, without a device."""
    from ssd_object_detection_amd.engine import SSDEngine
    for hin, hout, same in [(300, 150, False), (150, 75, False), (75, 38, True), (87, 43, False), (43, 22, True), (64, 32, False)]:
        assert SSDEngine._pool_same(dict(hin=hin, hout=hout)) is same, (hin, hout)
