"""Teacher-forced float64 backward pass of the SSD networks -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The oracle's backward is LINEAR: every data-dependent decision is an input, taken from a forward pass that somebody else ran
(the engine's on the GPU, or a float64 one on the CPU): ReLU masks are `act > 0` of the stored activations, pooling routes are the
stored winner codes, the weight gradients multiply the stored activations, the L2 normalisation works on the stored map.  What is
left is float64 arithmetic on the CPU (strict.ref_conv through autograd, strict.ref_unpool, l2norm_oracle.bwd64) and the wiring of
the network.  No mask can flip, so a missing or doubled contribution, a wrong mask source, a wrong route or an overwrite where an
accumulate belongs shows at full size.

Two modes of one walk:
  T  exact float64;
  R  (round_maps=True) the engine's storage: a gradient map is rounded to bf16 every time a contribution has been added to it
     (the head's first, then its consumers from the last node to the first), the rounded value is what is read downstream, and
     the map the L2 normalisation's backward reads (the head's data gradient w.r.t. the normalised map) is rounded as well; weight
     gradients are computed from rounded maps and not rounded.  R never sees what a kernel returned: rel_l2(R, T) is the size of
     the bf16 storage noise, and the bound of a tensor is 3 * rel_l2(R_t, T_t) + 1e-3 (bounds()).

Activation index a = node + 1 (index 0 is the image); gradient maps are named "gact<a>", parameters as the engines name them
("conv<node>/kernel", "head<level>/bias", "l2norm0/scale").

defect=(kind, arg) seeds ONE wiring error into the same walk:
  ("no_head", level)            the head's data gradient is not added to its feature map
  ("mask_output", node)         the convolution's data gradient is masked by its OUTPUT's sign (a shape-preserving layer)
  ("no_mask", node)             ... is not masked at all
  ("pool_first", node)          the pooling routes every window to position 0
  ("pool_pitch", node)          a VALID pooling of an odd map un-pooled at the SAME pooling's pitch, ceil(hin / 2): the pooled
                                gradient and its codes read as rows of one more window (the bug the engine had)
  ("wgrad_before_head", level)  the weight gradient of the layer that produces the level is computed without the head's part
  ("l2norm_scale_only", None)   the normalisation's backward is a multiplication with the scale
  ("overwrite", (a, node))      node's contribution to map a replaces what the map held
  ("no_identity", add) ("no_projection", add) ("no_shortcut_mask", add)   the shortcut term of an add dropped / not masked

mx=dict(dgrad, dy, wt): the MX-fp8 training backward of ResNet50SSDEngine, the same walk with one more forced operand.  A
bf16 rounding that differs between engine and oracle flips e4m3 roundings of the next fp8 operand (measured on the CPU: 1.6e-2
relative L2 per layer, against 1.7e-3 of bf16 storage noise), so the oracle does not quantise its own maps: the
data gradient of a convolution i in mx["dgrad"] is the float64 one of
  g := mx["dy"][root(i)]   the stored fp8 gradient map the launch read, dequantised (strict.ref_dequantize_mx): forward-like
                           state, taken as given like a mask or a route;
  w := mx["wt"][i]         the filters [Cout,k,k,Cin] as mx_filters() quantises them (the oracle's own: exact bf16 in, so
                           nothing can flip),
root(i) = the node whose gradient buffer node i's output shares, derived HERE from the adds the walk has passed (an add
gives its buffer to its block output and to a linear projection shortcut), never from the product's plan.  Weight and bias
gradients still come from the oracle's own map and the stored activation; mask, accumulate and rounding are unchanged.
trace: a dict the walk fills with "root" (node -> root), for the caller to compare with the engine's plan.  Two more defects:
  ("mx_wrong_dy", node)         fp8 data gradient `node` reads the stored fp8 map of the nearest other root of the same shape
  ("mx_stale_dy", root)         every reader of `root` reads the oracle's own quantisation of that map as it stood after its
                                FIRST writer, not its last"""
import time

import torch

from tests import strict as S
from tests import l2norm_oracle as LO

F64 = torch.float64
SUM_ORDER = 1e-3                       # fp32 summation order of a weight gradient (tests/test_wgrad_unpooled_gpu.py)
PAD_BITS = 0x4B1D5EED                  # a finite fp32 (about 1.03e7) no gradient comes near: the padding between tensors


def rel_l2(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / (b.norm() + 1e-300))


def to_bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def unpack_codes(words):
    """int32 [..., C/8] of eight 4-bit codes -> int64 [..., C] (the inverse of strict.pack_codes)"""
    w = words.to(torch.int64) & 0xFFFFFFFF
    return ((w[..., None] >> (4 * torch.arange(8, dtype=torch.int64))) & 15).reshape(*words.shape[:-1], words.shape[-1] * 8)


def conv_vjp(x, w, g, k, stride, pt, pl, need_dx=True):
    """(dx or None, dw, db): the gradients of strict.ref_conv(x, w) against g, float64"""
    xr = x.to(F64).detach().requires_grad_(need_dx)
    wr = w.to(F64).detach().requires_grad_(True)
    y = S.ref_conv(xr, wr, None, k, stride, pt, pl, g.shape[1], g.shape[2], False)
    grads = torch.autograd.grad(y, [xr, wr] if need_dx else [wr], g)
    return (grads[0] if need_dx else None), grads[-1], g.sum((0, 1, 2))


def conv_dx(x, w, g, k, stride, pt, pl):
    """conv_vjp's dx alone (the input's values do not enter it: the convolution is linear)"""
    xr = x.to(F64).detach().requires_grad_(True)
    y = S.ref_conv(xr, w.to(F64).detach(), None, k, stride, pt, pl, g.shape[1], g.shape[2], False)
    return torch.autograd.grad(y, [xr], g.to(F64))[0]


def mx_round(t):
    """What an MX-fp8 operand holds of a map: the bf16 value quantised by the CPU rule (strict.ref_quantize_mx: blocks of 32
    along the last axis) and dequantised, float64"""
    return S.ref_dequantize_mx(*S.ref_quantize_mx(t.to(torch.float32).to(torch.bfloat16).contiguous())).to(F64)


def flipped_transpose(w):
    """[Cout,k,k,Cin] -> [Cin,k,k,Cout] with both spatial axes mirrored: the layout of the engines' w_t"""
    return w.permute(3, 1, 2, 0).flip(1, 2).contiguous()


def mx_filters(w):
    """bf16 filters [Cout,k,k,Cin] as an fp8 data gradient holds them: quantised along Cout in blocks of 32 (the last axis of
    the transposed filters), dequantised, back in [Cout,k,k,Cin]"""
    return mx_round(w.permute(3, 1, 2, 0)).permute(3, 1, 2, 0).contiguous()


def _walk(nodes, fm, num_priors, classes, weights, acts, pool_codes, dloc, dconf, l2norm, round_maps, defect, first_node=0,
          mx=None, trace=None):
    rnd = to_bf16 if round_maps else (lambda t: t)
    defect = tuple(defect) if defect else (None, None)
    B = dloc.shape[0]
    G, grads, head_part = {}, {}, {}
    root, first = {}, {}                   # node -> the node whose gradient buffer it shares; map -> its value after its first writer

    def masked(a, g):
        return g * (acts[a] > 0)

    def add(a, g, writer):
        if a in G and defect != ("overwrite", (a, writer)):
            g = G[a] + g
        G[a] = rnd(g)
        first.setdefault(a, G[a])

    def mx_operand(i):                                     # the dy of fp8 data gradient i
        r = root.get(i, i)
        dy = mx["dy"][r]
        if defect == ("mx_wrong_dy", i):
            other = [q for q in sorted(mx["dy"]) if q != r and mx["dy"][q].shape == dy.shape]
            assert other, "mx_wrong_dy needs another root of the same shape"
            dy = mx["dy"][min(other, key=lambda q: abs(q - r))]
        if defect == ("mx_stale_dy", r):
            dy = mx_round(first[r + 1])
        assert dy.shape == G[i + 1].shape, (i, r)
        return dy

    off = 0
    for lvl, ((ni, h, c), n) in enumerate(zip(fm, num_priors)):
        a, cnt = ni + 1, h * h * n
        dy = torch.cat([dloc[:, off:off + cnt].to(F64).reshape(B, h, h, n * 4),
                        dconf[:, off:off + cnt].to(F64).reshape(B, h, h, n * classes)], -1)
        off += cnt
        normed = l2norm is not None and lvl == 0
        dx, dw, db = conv_vjp(l2norm["y"] if normed else acts[a], weights["head%d/kernel" % lvl], dy, 3, 1, 1, 1)
        grads["head%d/kernel" % lvl], grads["head%d/bias" % lvl] = dw, db
        dx = masked(a, dx)
        if normed:
            dx = rnd(dx)                                   # the gradient w.r.t. the normalised map is a stored bf16 map
            s = l2norm["scale"].to(F64)
            gx, ds = LO.bwd64(dx.reshape(-1, c).numpy(), acts[a].to(F64).reshape(-1, c).numpy(), s.numpy(), l2norm["eps"])
            grads["l2norm0/scale"] = torch.from_numpy(ds)
            dx = dx * s if defect[0] == "l2norm_scale_only" else torch.from_numpy(gx).reshape(dx.shape)
        head_part[a] = dx
        add(a, torch.zeros_like(dx) if defect == ("no_head", lvl) else dx, "head")
    assert off == dloc.shape[1] == dconf.shape[1]

    for i in range(len(nodes) - 1, first_node - 1, -1):
        nd, g = nodes[i], G[i + 1]
        kind, src = nd["kind"], nd.get("src", i - 1)
        if kind == "add":
            a_, sc = src
            add(a_ + 1, g, i)                              # the block output takes the gradient unchanged
            root[a_] = root.get(i, i)
            if nodes[sc]["kind"] == "conv" and not nodes[sc].get("relu", True):
                add(sc + 1, torch.zeros_like(g) if defect == ("no_projection", i) else g, i)
                root[sc] = root.get(i, i)
            else:                                          # identity shortcut: the source's own ReLU, summed with its other uses
                t = g if defect == ("no_shortcut_mask", i) else masked(sc + 1, g)
                add(sc + 1, torch.zeros_like(g) if defect == ("no_identity", i) else t, i)
            continue
        if kind in ("pool", "pool3"):
            ks, pad, none = (2, 0, 4) if kind == "pool" else (3, nd["pt"], 15)
            code = pool_codes[i]
            if defect == ("pool_first", i):
                code = torch.where(code != none, torch.zeros_like(code), code)
            if defect == ("pool_pitch", i):
                ho, hs = g.shape[1], (nd["hin"] + 1) // 2
                assert kind == "pool" and hs == ho + 1, "pool_pitch needs a VALID pooling of an odd map"

                def repitch(t):                            # the same bytes per image, read at the other pitch
                    flat = torch.cat([t.reshape(B, -1), torch.zeros((B, (hs * hs - ho * ho) * t.shape[-1]), dtype=t.dtype)], 1)
                    return flat.reshape(B, hs, hs, t.shape[-1])[:, :ho, :ho].contiguous()
                g, code = repitch(g), repitch(code)
            add(src + 1, S.ref_unpool(code, g, (B, nd["hin"], nd["hin"], nd["cin"]), ks, 2, pad, pad), i)
            continue
        assert kind == "conv"
        x, w = acts[src + 1], weights["conv%d/kernel" % i]
        fp8 = mx is not None and i in mx["dgrad"]
        dx, dw, db = conv_vjp(x, w, g, nd["k"], nd["stride"], nd["pt"], nd["pl"], need_dx=src >= 0 and not fp8)
        if fp8:
            dx = conv_dx(x, mx["wt"][i], mx_operand(i), nd["k"], nd["stride"], nd["pt"], nd["pl"])
        if defect[0] == "wgrad_before_head" and fm[defect[1]][0] == i:
            _, dw, db = conv_vjp(x, w, g - head_part[i + 1], nd["k"], nd["stride"], nd["pt"], nd["pl"], need_dx=False)
        grads["conv%d/kernel" % i], grads["conv%d/bias" % i] = dw, db
        if src < 0:
            continue                                       # no gradient w.r.t. the image
        if nodes[src].get("relu", nodes[src]["kind"] == "conv"):
            if defect == ("mask_output", i):
                assert dx.shape == g.shape, "mask_output needs a shape-preserving layer"
                dx = masked(i + 1, dx)
            elif defect != ("no_mask", i):
                dx = masked(src + 1, dx)
        add(src + 1, dx, i)                                # (behind a pooling the route alone decides: code `none` = no gradient)
    if trace is not None:
        trace["root"] = [root.get(i, i) for i in range(len(nodes))]
    out = dict(grads)
    out.update(("gact%d" % a, g) for a, g in G.items() if a > first_node)     # (below it the maps are incomplete)
    return out


def backward_chain(nodes, fm, num_priors, classes, weights, acts, pool_codes, dloc, dconf, l2norm=None, round_maps=False,
                   defect=None, first_node=0):
    """The VGG-style engines (SSDEngine.nodes: node i reads node i - 1).  weights: name -> tensor; acts: activation index ->
    stored map, None where the forward stored none (pool_only); pool_codes: node -> int64 [B,Ho,Wo,C] winner codes;
    l2norm: None or dict(scale, y = the stored normalised map, eps).  Returns {name: float64 tensor} of every parameter
    gradient and every gradient map.  first_node: the walk ends behind that node (what it returns is complete: the gradients
    of the nodes it visited, the maps above them) -- a defect deep in the network need not pay for the wide layers."""
    return _walk(nodes, fm, num_priors, classes, weights, acts, pool_codes, dloc, dconf, l2norm, round_maps, defect, first_node)


def backward_graph(nodes, fm, num_priors, classes, weights, acts, pool_codes, dloc, dconf, round_maps=False, defect=None,
                   first_node=0, mx=None, trace=None):
    """The same for ResNet50SSDEngine.nodes (kind conv | pool3 | add with src and relu).  An add hands its gradient to the block
    output unchanged, to a projection shortcut unchanged, to an identity shortcut masked by the source's ReLU and summed with
    the source's other uses.  mx, trace: the MX-fp8 training backward (module docstring)."""
    return _walk(nodes, fm, num_priors, classes, weights, acts, pool_codes, dloc, dconf, None, round_maps, defect, first_node,
                 mx, trace)


# ---- the rule --------------------------------------------------------------------------------------------------------------
def bounds(T, R):
    """name -> 3 * rel_l2(R, T) + 1e-3: both terms from the reference side (module docstring)"""
    return {k: 3.0 * rel_l2(R[k], T[k]) + SUM_ORDER for k in T}


def compare(got, T, R, title, out=print):
    """Prints one row per tensor of `got` (name, error against T, R's error against T, bound); returns the rows beyond their
    bound as [(name, err, r_err, bound)] and the worst row by err / bound."""
    bad, worst, bound = [], None, bounds(T, R)
    out("%s\n%-22s %11s %11s %11s" % (title, "tensor", "err vs T", "R vs T", "bound"))
    for name in got:
        row = (name, rel_l2(got[name], T[name]), rel_l2(R[name], T[name]), bound[name])
        err = row[1]
        out("%-22s %11.3e %11.3e %11.3e%s" % (row + ("" if err <= row[3] else "   <-- FAIL",)))
        if not err <= row[3]:
            bad.append(row)
        if worst is None or err / row[3] > worst[1] / worst[3]:
            worst = row
    out("worst: %s err %.3e R %.3e bound %.3e" % worst)
    return bad, worst


def moved(T, D, bound):
    """The tensors a seeded defect moved to at least twice their bound: [(name, rel_l2(D, T), bound)]"""
    return [(k, rel_l2(D[k], T[k]), bound[k]) for k in D if rel_l2(D[k], T[k]) >= 2.0 * bound[k]]


# ---- the engine's side (GPU tensors in, CPU tensors out) -------------------------------------------------------------------
def poison(engine, c):
    """NaN in every gradient map and every gradient tensor, PAD_BITS in the padding between the tensors.  Behind a training-mode
    fp8 forward also byte 0x7F (e4m3 NaN; as a scale 2^0) in every fp8 gradient map and in the fp8 transposed filters, where
    allocated: an fp8 map nobody wrote turns its reader's output non-finite."""
    for g in c["gacts"][1:]:
        g.fill_(float("nan"))
    engine.grad.view(torch.int32).fill_(PAD_BITS)
    for t in engine.tensors:
        engine.grad[t.offset:t.offset + t.numel].fill_(float("nan"))
    if engine.last_forward == "mxfp8_train":
        stale = [t for pair in engine.mxfp8_grads(c["acts"][1].shape[0]).values() for t in pair]
        for t in stale + ([engine.mx_filters_t.q, engine.mx_filters_t.scale] if engine.mx_filters_t.allocated else []):
            t.fill_(0x7F)


def padding_untouched(engine, grad_cpu):
    pad = torch.ones(engine.n_flat, dtype=torch.bool)
    for t in engine.tensors:
        pad[t.offset:t.offset + t.numel] = False
    return bool((grad_cpu.view(torch.int32)[pad] == PAD_BITS).all())


def gemm_arrays(engine):
    """The arrays the network computes with: conv kernels / biases, the fused per-level head arrays, the l2norm scale"""
    out = [t for i in sorted(engine.conv_params) for t in engine.conv_params[i]] + [t for pair in engine.head_params for t in pair]
    return out + ([engine.l2norm_scale] if engine.l2norm_scale is not None else [])


def engine_weights(engine):
    bf, f32 = engine.param_bf16.float().cpu(), engine.param.cpu()
    return {t.name: (bf if t.name.endswith("kernel") else f32)[t.offset:t.offset + t.numel].view(t.shape).to(F64)
            for t in gemm_arrays(engine)}


def engine_grads(engine, c, maps):
    """name -> CPU tensor: every parameter gradient and the gradient maps of activation indices `maps`"""
    flat = engine.grad.cpu()
    got = {t.name: flat[t.offset:t.offset + t.numel].view(t.shape) for t in gemm_arrays(engine)}
    got.update(("gact%d" % a, c["gacts"][a].float().cpu()) for a in maps)
    return got, flat


def check_outputs(engine, c, got, flat, maps):
    """What backward() must leave behind a poison(): everything it writes finite, nothing else touched"""
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), "%s is not finite: no launch produced it, or one accumulated into an unwritten map" % name
    for a in range(1, len(c["gacts"])):
        if a not in maps:
            assert bool(torch.isnan(c["gacts"][a].float()).all()), "gact%d: the configuration does not write it, yet it changed" % a
    assert padding_untouched(engine, flat), "the padding between gradient tensors changed"
    assert float(got["conv0/kernel"][..., 3:].abs().max()) == 0.0, "conv0/kernel: the padded input channels got a gradient"


class Forced:
    """One engine, one forward + backward on it behind a poison(), and the oracle's T and R on what that forward stored.  A
    subclass says which gradient maps the configuration writes (written_maps), what the forward stored (stored_forward ->
    activations, codes, l2norm) and which walk is the engine's (walk); it may run another forward (run_forward), pass
    backward() keywords (backward_kwargs) and hand the walk its forced MX-fp8 operands (mx_operands).  run() does all of it
    again on the same engine and inputs (a test that changed how the engine runs)."""
    backward_kwargs = {}

    def __init__(self, engine, B, seed, classes=81, level_scale=None):
        import ssd_object_detection_amd.ops as ops
        torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
        self.engine, self.B, self.classes = engine, B, classes
        g = torch.Generator().manual_seed(seed)
        s = engine.in_size
        self.x = ops.image_prep(torch.rand((B, s, s, 3), generator=g).cuda())
        self.dloc = (torch.randn((B, engine.A, 4), generator=g) * 1e-3).bfloat16()
        self.dconf = (torch.randn((B, engine.A, classes), generator=g) * 1e-3).bfloat16()
        for lvl, f in enumerate(level_scale or ()):                     # a power of two per level: still bf16 values
            lo, hi = engine.level_off[lvl], engine.level_off[lvl + 1]
            self.dloc[:, lo:hi] *= f
            self.dconf[:, lo:hi] *= f
        self.run()

    def run_forward(self, engine, x):
        engine.forward(x)

    def mx_operands(self):
        return None

    def run(self):
        engine = self.engine
        self.run_forward(engine, self.x)
        self.c = c = engine._acts(self.B)
        poison(engine, c)
        engine.backward(self.dloc.cuda(), self.dconf.cuda(), **self.backward_kwargs)
        torch.cuda.synchronize()
        self.maps = self.written_maps()
        self.got, self.flat = engine_grads(engine, c, self.maps)
        self.stored, self.codes, self.l2norm = self.stored_forward()
        self.weights = engine_weights(engine)
        self.mx = self.mx_operands()
        t0 = time.time()
        self.T, self.R = self.oracle(), self.oracle(round_maps=True)
        self.bound = bounds(self.T, self.R)
        print("oracle: T + R in %.1f s" % (time.time() - t0))

    def oracle(self, **kw):
        e = self.engine
        if self.mx is not None:
            kw = dict(kw, mx=self.mx)
        return self.walk(e.nodes, e.fm, e.num_priors, self.classes, self.weights, self.stored, self.codes, self.dloc, self.dconf, **kw)

    def check_forward_state(self):
        raise NotImplementedError

    def check(self, title):
        self.check_forward_state()
        check_outputs(self.engine, self.c, self.got, self.flat, self.maps)
        bad, self.worst = compare(self.got, self.T, self.R, title)
        assert not bad, "beyond 3 * rel_l2(R, T) + 1e-3: " + ", ".join("%s %.3e > %.3e" % (n, e, b) for n, e, _, b in bad)
