"""Strict kernel checks: exact operands, an arena with guard bands, two poisons.  Plain Python: importable without a GPU.

Exact operands.  Every operand is a small integer times a power of two, so bf16 products are exact and fp32 sums are exact in
any order: the expected bits do not depend on rounding mode, summation order or split count, and every comparison is
torch.equal.  The regime is a condition on the INPUTS, asserted on the fp32 reference (in_bf16_regime / in_fp32_regime), never
on what a kernel returned.

Arena.  Tensors are carved from one byte buffer: each starts on a 256-byte boundary, has 1 MiB of guard in front, and its
trailing 1 MiB guard begins at its exact last byte.  (1 MiB is derived, not measured: the largest store tile of any kernel is
256 x 256 fp32 = 256 KiB, so a stray tile row stays inside the guard.)  Arena.run executes an operation twice, with outputs,
workspace and every guard -- those around the inputs too -- filled with a poison pattern P (0x7FA5 as bf16, 0x7FA5A5A5 as fp32:
both NaN) and then with ~P, and reports: a guard byte that changed (a write outside the documented extent), an input that
changed, an output element that differs from the reference (which includes every element never written: no poison equals the
reference under both patterns), and outputs that differ between the two runs (a read of a guard or of unwritten scratch that
reached the result)."""
import numpy as np
import torch
import torch.nn.functional as F

GUARD = 1 << 20
ALIGN = 256
POISON = {1: 0xA5, 2: 0x7FA5, 4: 0x7FA5A5A5, 8: 0x7FA5A5A57FA5A5A5}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class StrictError(AssertionError):
    pass


def _signed(pattern, size):
    """the two's-complement value torch's signed integer dtypes take for a bit pattern"""
    if size == 1:
        return pattern
    return pattern - (1 << (8 * size)) if pattern >> (8 * size - 1) else pattern


def _pattern(size, inverted):
    p = POISON[size]
    return _signed(p ^ ((1 << (8 * size)) - 1) if inverted else p, size)


def first_diff(got, want):
    """'index, got, want, count' of the first differing element (for messages)"""
    g, w = got.detach().cpu(), want.detach().cpu()
    if g.shape != w.shape:
        return "shape %s != %s" % (tuple(g.shape), tuple(w.shape))
    bad = (g != w) | (g != g)
    n = int(bad.sum())
    if n == 0:
        return "no difference"
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return "%d of %d elements differ, first at %s: got %r, want %r" % (n, g.numel(), idx, g[idx].item(), w[idx].item())


class _Slot:
    def __init__(self, name, start, nbytes, size, tensor, kind):
        self.name, self.start, self.nbytes, self.size, self.tensor, self.kind = name, start, nbytes, size, tensor, kind
        self.keep = None           # inputs / in-out tensors: the contents every run starts from (held outside the arena)
        self.want = None           # outputs: the reference of the current run
        self.untouched = None      # outputs the current run does not list: their bytes before it
        self.written = None        # outputs of which a call writes a part only: bool mask of the documented extent


class _Workspace:
    """What ops.py expects of ws=: get(nbytes, device) -> uint8 tensor; here a guarded slice of EXACTLY nbytes."""

    def __init__(self, arena):
        self.arena = arena
        self.slots = {}

    def get(self, nbytes, device):
        nbytes = int(nbytes)
        if nbytes not in self.slots:
            self.slots[nbytes] = self.arena._carve("workspace[%d]" % nbytes, (nbytes,), torch.uint8, "ws")
            self.arena._fill_slot(self.arena._slot_of(self.slots[nbytes]))
        return self.slots[nbytes]


class Arena:
    def __init__(self, device, capacity=256 << 20):
        self.device = torch.device(device)
        self.capacity = (int(capacity) + ALIGN - 1) // ALIGN * ALIGN
        self.buf = torch.empty((self.capacity,), dtype=torch.uint8, device=self.device)
        base = self.buf.data_ptr()
        self.origin = (-base) % ALIGN                       # offset of the first 256-byte boundary
        self.cursor = self.origin
        self.slots = []
        self.inverted = False
        self.buf.fill_(POISON[1])

    # ---- carving --------------------------------------------------------------------------------------------------
    def _carve(self, name, shape, dtype, kind):
        size = torch.empty((), dtype=dtype).element_size()
        numel = int(np.prod(shape)) if len(shape) else 1
        nbytes = numel * size
        start = self.cursor + GUARD                                     # cursor and GUARD are multiples of 256
        end = start + nbytes + GUARD
        if end > self.capacity:
            raise MemoryError("strict.Arena: %d bytes needed for %s, capacity %d" % (end, name, self.capacity))
        t = self.buf[start:start + nbytes].view(dtype).view(*shape) if numel else self.buf[start:start].view(dtype).view(*shape)
        assert t.data_ptr() % ALIGN == 0 or numel == 0
        # the guards are filled with the element-size pattern of their tensor; a workspace counts as fp32 where it can
        psize = size if kind != "ws" else (4 if nbytes % 4 == 0 else 1)
        self.slots.append(_Slot(name, start, nbytes, psize, t, kind))
        self.cursor = self.origin + (end - self.origin + ALIGN - 1) // ALIGN * ALIGN
        return t

    def _slot_of(self, t):
        for s in self.slots:
            if s.tensor is t:
                return s
        raise KeyError("not a tensor of this arena")

    def put(self, value, name="input"):
        """an input: `value` (any device) copied into the arena; must be unchanged after every run"""
        t = self._carve(name, tuple(value.shape), value.dtype, "in")
        s = self.slots[-1]
        s.keep = value.detach().to(self.device).clone()
        self._fill_slot(s)
        return t

    def out(self, shape, dtype, name="output"):
        """an output: poisoned before every run, compared with the reference given to run()"""
        t = self._carve(name, tuple(shape), dtype, "out")
        self._fill_slot(self.slots[-1])
        return t

    def inout(self, value, name="accumulator"):
        """read and written: starts every run from `value`, compared with the reference given to run()"""
        t = self._carve(name, tuple(value.shape), value.dtype, "inout")
        s = self.slots[-1]
        s.keep = value.detach().to(self.device).clone()
        self._fill_slot(s)
        return t

    def set(self, t, value):
        """new contents that an input / in-out tensor starts every later run from (a state carried from step to step)"""
        s = self._slot_of(t)
        assert s.keep is not None and tuple(value.shape) == tuple(t.shape) and value.dtype == t.dtype
        s.keep = value.detach().to(self.device).clone()
        self._fill_slot(s)

    def workspace(self):
        return _Workspace(self)

    @staticmethod
    def bytes_for(*nbytes):
        """capacity that holds tensors of these byte counts"""
        return sum((int(n) + ALIGN - 1) // ALIGN * ALIGN + 2 * GUARD + ALIGN for n in nbytes) + 4 * ALIGN

    # ---- poison ---------------------------------------------------------------------------------------------------
    def _region(self, s):
        """the slot's guard + body + guard as integers of its pattern size"""
        return self.buf[s.start - GUARD:s.start + s.nbytes + GUARD].view(_INT[s.size])

    def _fill_slot(self, s):
        self._region(s).fill_(_pattern(s.size, self.inverted))
        if s.keep is not None:
            s.tensor.copy_(s.keep)

    def poison(self, inverted):
        self.inverted = inverted
        for s in self.slots:
            self._fill_slot(s)

    # ---- checks ---------------------------------------------------------------------------------------------------
    def _guard_findings(self, s):
        reg = self._region(s)
        g = GUARD // s.size
        pat = _pattern(s.size, self.inverted)
        out = []
        for side, part, off0 in (("before the start of", reg[:g], -g), ("past the end of", reg[g + s.nbytes // s.size:], 0)):
            bad = part != pat
            if bool(bad.any()):
                i = int(bad.nonzero()[0]) if side.startswith("past") else int(bad.nonzero()[-1])
                dist = (i + 1) * s.size if side.startswith("past") else (g - i) * s.size
                out.append("write %s %s: %d guard words changed, nearest within %d bytes" % (side, s.name, int(bad.sum()), dist))
        return out

    def findings(self):
        out = []
        for s in self.slots:
            out += self._guard_findings(s)
            if s.kind == "in" and not torch.equal(s.tensor, s.keep):
                out.append("input %s was modified: %s" % (s.name, first_diff(s.tensor, s.keep)))
            if s.kind in ("out", "inout") and s.want is not None:
                want = s.want
                if s.written is None:
                    if not torch.equal(s.tensor, want):
                        out.append("%s differs from the reference: %s" % (s.name, first_diff(s.tensor, want)))
                else:                                  # the documented extent only; the rest keeps what it started with
                    m = s.written.to(self.device)
                    if not torch.equal(s.tensor[m], want[m]):
                        out.append("%s differs from the reference: %s" % (s.name, first_diff(s.tensor[m], want[m])))
                    bits = s.tensor.contiguous().view(-1).view(_INT[s.tensor.element_size()])
                    start = s.keep.contiguous().view(-1).view(bits.dtype) if s.keep is not None else \
                        torch.full_like(bits, _pattern(s.tensor.element_size(), self.inverted))
                    rest = ~m.reshape(-1)
                    if not torch.equal(bits[rest], start[rest]):
                        out.append("%s was written outside its documented extent: %s" % (s.name, first_diff(bits[rest], start[rest])))
            if s.kind in ("out", "inout") and s.untouched is not None:
                body = self.buf[s.start:s.start + s.nbytes]
                if not torch.equal(body, s.untouched):
                    out.append("%s was written although the call does not list it: %s" % (s.name, first_diff(body, s.untouched)))
        return out

    def run(self, fn, expect):
        """fn() under poison P, then under ~P.  expect: [(arena tensor, reference tensor[, bool mask of the elements the C ABI
        documents as written: all when absent])] for every output fn writes; an
        output or in-out tensor of the arena that is not listed must keep its poison / its start value.  Raises StrictError
        listing every finding; returns the outputs of the first run (clones, in the order of `expect`)."""
        expect = [tuple(e) + (None,) * (3 - len(e)) for e in expect]
        listed = {id(e[0]) for e in expect}
        for s in self.slots:
            s.want = s.written = None
        for t, want, written in expect:
            s = self._slot_of(t)
            s.written = written
            assert s.kind in ("out", "inout"), s.name
            assert tuple(want.shape) == tuple(t.shape) and want.dtype == t.dtype, (s.name, want.shape, want.dtype, t.shape, t.dtype)
            s.want = want.to(self.device)
        runs, problems = [], []
        for inverted in (False, True):
            self.poison(inverted)
            for s in self.slots:                   # an unlisted output must stay as it starts
                if s.kind in ("out", "inout"):
                    s.untouched = None if id(s.tensor) in listed else self.buf[s.start:s.start + s.nbytes].clone()
            fn()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            problems += ["[poison %s] %s" % ("~P" if inverted else "P", f) for f in self.findings()]
            runs.append([e[0].detach().clone() for e in expect])
        for (t, _, written), a, b in zip(expect, *runs):
            if written is not None:
                a, b = a[written.to(self.device)], b[written.to(self.device)]
            ia, ib = a.contiguous().view(-1).view(_INT[a.element_size()]), b.contiguous().view(-1).view(_INT[b.element_size()])
            if not torch.equal(ia, ib):
                problems.append("%s differs between the two poisons (a guard or unwritten scratch reached it): %s"
                                % (self._slot_of(t).name, first_diff(ia, ib)))
        if problems:
            raise StrictError("\n".join(problems))
        return runs[0]


# ---- exact operands ------------------------------------------------------------------------------------------------
def geometry(H, W, k, stride, mode):
    """(Ho, Wo, pad_t, pad_l): TF 'SAME' or 'VALID' (as ops.same_pad / ops.valid_out)"""
    if mode == "same":
        def sp(n):
            o = -(-n // stride)
            return o, max((o - 1) * stride + k - n, 0) // 2
        (Ho, pt), (Wo, pl) = sp(H), sp(W)
    else:
        Ho, Wo, pt, pl = (H - k) // stride + 1, (W - k) // stride + 1, 0, 0
    return Ho, Wo, pt, pl


def ints(g, shape, values, density=1.0, scale=1.0, dtype=torch.bfloat16):
    """a tensor of `values` (drawn uniformly), thinned to `density` (the rest exact zeros), times `scale` (a power of two)"""
    vals = torch.tensor(values, dtype=torch.float32)
    t = vals[torch.randint(0, len(values), shape, generator=g)]
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density)
    return (t * scale).to(dtype)


def case_seed(case):
    return int(sum((i + 1) * int(v) for i, v in enumerate(case[:7]))) % 100003


def conv_operands(case, seed=None):
    """The exact operands of a (B, H, W, Cin, Cout, k, stride, mode) case, in the project's layouts (NHWC, [Cout,k,k,Cin]):
    x dense in {-2,-1,1,2}; w in {-1,0,1} thinned to min(1, 256/K), K = k*k*Cin; dy in {-2,-1,1,2} thinned the same way against
    k*k*Cout; bias small fp32 integers; a mask source of integers with many zeros; an accumulation base of small integers."""
    B, H, W, Cin, Cout, k, stride, mode = case[:8]
    Ho, Wo, pt, pl = geometry(H, W, k, stride, mode)
    g = torch.Generator().manual_seed(case_seed(case) if seed is None else seed)
    x = ints(g, (B, H, W, Cin), (-2, -1, 1, 2))
    w = ints(g, (Cout, k, k, Cin), (-1, 1), min(1.0, 256.0 / (k * k * Cin)))
    dy = ints(g, (B, Ho, Wo, Cout), (-2, -1, 1, 2), min(1.0, 256.0 / (k * k * Cout)))
    bias = ints(g, (Cout,), (-3, -2, -1, 0, 1, 2, 3), dtype=torch.float32)
    mask_src = ints(g, (B, H, W, Cin), (-1, 0, 0, 1, 2))
    base = ints(g, (B, H, W, Cin), (-2, -1, 0, 1, 2))
    return dict(x=x, w=w, dy=dy, bias=bias, mask_src=mask_src, base=base, geom=(Ho, Wo, pt, pl))


def ref_conv(x, w, bias, k, stride, pad_t, pad_l, Ho, Wo, relu):
    """x [B,H,W,C] f32, w [Cout,k,k,Cin] f32 -> [B,Ho,Wo,Cout] f32 with explicit (possibly asymmetric) padding."""
    B, H, W, C = x.shape
    pad_b = max((Ho - 1) * stride + k - H - pad_t, 0)
    pad_r = max((Wo - 1) * stride + k - W - pad_l, 0)
    xn = F.pad(x.permute(0, 3, 1, 2), (pad_l, pad_r, pad_t, pad_b))
    y = F.conv2d(xn, w.permute(0, 3, 1, 2), bias, stride=stride)
    assert y.shape[2] == Ho and y.shape[3] == Wo
    if relu:
        y = y.relu()
    return y.permute(0, 2, 3, 1).contiguous()


def in_bf16_regime(t):
    """every value of the fp32 reference is exactly representable in bf16 (an integer of at most 8 bits times a power of two)
    and finite"""
    return bool(torch.isfinite(t).all()) and torch.equal(t.to(torch.bfloat16).to(t.dtype), t)


def in_fp32_regime(k_total, a, b):
    """a sum of k_total products a*b of integer-valued operands is exact in fp32 in any order: k_total * max|a| * max|b| < 2^24"""
    a, b = a.float(), b.float()
    assert torch.equal(a, a.round()) and torch.equal(b, b.round())
    return k_total * float(a.abs().max()) * float(b.abs().max()) < 2 ** 24


def masked(t, keep):
    """t where keep, +0 elsewhere (a product with the mask would leave -0 under negative values: equal as a number, another
    byte once quantised)"""
    return torch.where(keep, t, torch.zeros((), dtype=t.dtype))


def conv_reference(case, ops_=None, dtype=torch.float32):
    """fp32 (or float64) reference of everything the strict conv test runs on a case: forward with and without ReLU, data
    gradient plain and (dx + base) * (mask_src > 0), weight and bias gradient, the transposed filters.  Returns a dict; the
    regime conditions are asserted by check_conv_regime."""
    B, H, W, Cin, Cout, k, stride, mode = case[:8]
    o = dict(ops_ or conv_operands(case))
    Ho, Wo, pt, pl = o["geom"]
    xr = o["x"].to(dtype).requires_grad_(True)
    wr = o["w"].to(dtype).requires_grad_(True)
    br = o["bias"].to(dtype).requires_grad_(True)
    y = ref_conv(xr, wr, br, k, stride, pt, pl, Ho, Wo, False)
    y.backward(o["dy"].to(dtype))
    o["y"] = y.detach()
    o["y_relu"] = y.detach().relu()
    o["dx"] = xr.grad
    o["dx_acc"] = masked(xr.grad + o["base"].to(dtype), o["mask_src"].to(dtype) > 0)
    o["dw"], o["dbias"] = wr.grad, br.grad
    cp = (Cout + 7) // 8 * 8
    w_t = torch.zeros((Cin, k, k, cp), dtype=torch.bfloat16)
    w_t[..., :Cout] = o["w"].flip(1, 2).permute(3, 1, 2, 0)
    o["w_t"] = w_t
    dyp = torch.zeros((B, Ho, Wo, cp), dtype=torch.bfloat16)
    dyp[..., :Cout] = o["dy"]
    o["dy_pad"] = dyp
    return o


def check_conv_regime(case, r):
    """the regime conditions of the issue, on the reference `r` of conv_reference"""
    B, H, W, Cin, Cout, k, stride, mode = case[:8]
    Ho, Wo = r["geom"][:2]
    for name in ("y", "y_relu", "dx", "dx_acc"):
        assert in_bf16_regime(r[name]), (case[:8], name, float(r[name].abs().max()))
    assert in_fp32_regime(B * Ho * Wo, r["x"], r["dy"]), (case[:8], "dw")
    assert in_fp32_regime(B * Ho * Wo, r["dy"], torch.ones(1)), (case[:8], "dbias")
    assert in_fp32_regime(k * k * Cin, r["x"], r["w"]) and in_fp32_regime(k * k * Cout, r["dy"], r["w"]), (case[:8], "accumulators")


# ---- the project's stated conventions, restated ----------------------------------------------------------------------
def pack_bits(positive):
    """bool [..., C] -> uint8 [..., C/8]: bit k of byte c = channel 8c + k (the ReLU sign bytes: y > 0)"""
    b = positive.to(torch.int32).reshape(*positive.shape[:-1], positive.shape[-1] // 8, 8)
    return (b << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)


def pack_codes(code):
    """int [..., C] of 4-bit codes -> int32 [..., C/8]: nibble k of word c = channel 8c + k"""
    c = code.to(torch.int64).reshape(*code.shape[:-1], code.shape[-1] // 8, 8)
    word = (c << (4 * torch.arange(8, dtype=torch.int64))).sum(-1)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)


def ref_pool(x, ksize, stride, pad_t, pad_l, Ho, Wo, none_code):
    """Max pooling with winner codes, by the stated conventions: windows clipped at the map's edge; the code is the index
    (ksize * dy + dx) of the FIRST maximum in window order, or `none_code` when the maximum is <= 0.  x f32 [B,H,W,C] ->
    (y f32 [B,Ho,Wo,C], code int64 [B,Ho,Wo,C])."""
    B, H, W, C = x.shape
    best = torch.full((B, Ho, Wo, C), float("-inf"))
    pos = torch.full((B, Ho, Wo, C), none_code, dtype=torch.int64)
    oy = torch.arange(Ho) * stride - pad_t
    ox = torch.arange(Wo) * stride - pad_l
    for dy in range(ksize):
        for dx in range(ksize):
            iy, ix = oy + dy, ox + dx
            oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            v = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            v = torch.where((oky[:, None] & okx[None, :])[None, :, :, None], v, torch.tensor(float("-inf")))
            better = v > best                                              # strict: the first maximum wins
            best = torch.where(better, v, best)
            pos = torch.where(better, torch.tensor(ksize * dy + dx), pos)
    pos = torch.where(best > 0, pos, torch.tensor(none_code))
    return best, pos


def ref_unpool(code, dy, x_shape, ksize, stride, pad_t, pad_l):
    """Un-pooling routes by the code: dx[p] = sum of dy over the windows whose code names p.  code int64, dy f32."""
    B, H, W, C = x_shape
    _, Ho, Wo, _ = dy.shape
    dx = torch.zeros(x_shape, dtype=dy.dtype)
    oy = torch.arange(Ho) * stride - pad_t
    ox = torch.arange(Wo) * stride - pad_l
    for ddy in range(ksize):
        for ddx in range(ksize):
            iy, ix = oy + ddy, ox + ddx
            oky, okx = (iy >= 0) & (iy < H), (ix >= 0) & (ix < W)
            g = dy * (code == ksize * ddy + ddx)
            g = g[:, oky][:, :, okx]
            dx[:, iy[oky][:, None], ix[okx][None, :]] += g
    return dx


# ---- MX-fp8, by the stated rule -----------------------------------------------------------------------------------------
def ref_quantize_mx(t):
    """bf16 [..., C] (C % 32 == 0) -> (q uint8 [..., C] OCP e4m3 bytes, scale uint8 [..., C/32] E8M0): per block of 32 the scale
    2^e with e the smallest integer such that amax / 2^e <= 448 (0 for an all-zero block), elements v / 2^e rounded to nearest"""
    v = t.float().reshape(*t.shape[:-1], t.shape[-1] // 32, 32)
    amax = v.abs().amax(-1)
    m, ex = torch.frexp(amax / 448.0)
    e = torch.where(amax > 0, torch.where(m == 0.5, ex - 1, ex), torch.zeros_like(ex)).clamp(-127, 127)
    q = (v * torch.exp2(-e.float()).unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8).reshape(t.shape)
    return q, (e + 127).to(torch.uint8)


def ref_dequantize_mx(q, scale):
    v = q.view(torch.float8_e4m3fn).float()
    return (v.view(*scale.shape, 32) * torch.exp2(scale.float() - 127.0).unsqueeze(-1)).view(q.shape)


# ---- full-size cases at the smallest batch that still reaches their kernels ---------------------------------------------------
def smallest_batch(case):
    """the smallest batch in {1, 2, 4, 8, 16, 32} for which the dispatch query still names the case's kernels (a host function);
    the case's own batch if none does"""
    from tests.conv_cases import plan_names
    for b in (1, 2, 4, 8, 16, 32):
        if b < case[0] and plan_names((b,) + tuple(case[1:8])) == case[8]:
            return b
    return case[0]


# ---- the other entry points: operands and references --------------------------------------------------------------------------
def check_regime(r):
    """r["bf16"]: names of the reference tensors a kernel returns in bf16; r["fp32"]: (k_total, a, b) of every fp32 sum"""
    for name in r.get("bf16", ()):
        assert in_bf16_regime(r[name].float()), (name, float(r[name].float().abs().max()))
    for k_total, a, b in r.get("fp32", ()):
        assert in_fp32_regime(k_total, a, b), (k_total, float(a.float().abs().max()), float(b.float().abs().max()))


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 3) * int(v) for i, v in enumerate(key))) % 100003)


def pool2x2_case(B, H, W, C, same):
    g = _gen(B, H, W, C, same)
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if same else (H // 2, W // 2)
    x = ints(g, (B, H, W, C), (-2, -1, 0, 0, 1, 1, 2, 3))               # exact zeros, ties, windows whose maximum is <= 0
    x[:, ::3, ::5] = ints(g, x[:, ::3, ::5].shape, (-1, 0))
    y, code = ref_pool(x.float(), 2, 2, 0, 0, Ho, Wo, 4)
    dy = ints(g, (B, Ho, Wo, C), (-2, -1, 1, 2))
    dx = ref_unpool(code, dy.float(), x.shape, 2, 2, 0, 0)
    return dict(x=x, y=y, code=code, dy=dy, dx=dx, bf16=("y", "dx"))


def pool3x3_case(B, H, W, C):
    g = _gen(B, H, W, C, 3)
    Ho, Wo, pt, pl = geometry(H, W, 3, 2, "same")
    x = ints(g, (B, H, W, C), (-2, -1, 0, 0, 1, 1, 2, 3))
    x[:, ::4, ::3] = ints(g, x[:, ::4, ::3].shape, (-1, 0))
    y, code = ref_pool(x.float(), 3, 2, pt, pl, Ho, Wo, 15)
    dy = ints(g, (B, Ho, Wo, C), (-2, -1, 1, 2))
    dx = ref_unpool(code, dy.float(), x.shape, 3, 2, pt, pl)              # up to four windows meet in a pixel: |dx| <= 8
    return dict(x=x, y=y, code=code, dy=dy, dx=dx, geom=(Ho, Wo, pt, pl), bf16=("y", "dx"))


def eltwise_case(shape):
    g = _gen(*shape)
    a, b = ints(g, shape, (-3, -2, -1, 0, 1, 2, 3)), ints(g, shape, (-3, -2, -1, 0, 1, 2, 3))
    out = (a.float() + b.float()).relu()                                 # many exact zeros before the ReLU
    gr, base = ints(g, shape, (-2, -1, 1, 2)), ints(g, shape, (-2, -1, 0, 1, 2))
    masked_g = masked(gr.float(), out > 0)
    return dict(a=a, b=b, out=out, g=gr, base=base, masked=masked_g, acc=base.float() + masked_g, bf16=("out", "masked", "acc"))


def head_case(B, H, W, Cin, n, classes=81, off=200, npad=512):
    g = _gen(B, H, W, Cin, n)
    N, A = n * (4 + classes), off + H * W * n
    x = ints(g, (B, H, W, Cin), (-2, -1, 1, 2))
    w = ints(g, (N, 3, 3, Cin), (-1, 1), min(1.0, 256.0 / (9 * Cin)))
    bias = ints(g, (N,), (-3, -2, -1, 0, 1, 2, 3), dtype=torch.float32)
    yr = ref_conv(x.float(), w.float(), bias, 3, 1, 1, 1, H, W, False)
    loc, conf = torch.zeros((B, A, 4)), torch.zeros((B, A, classes))
    loc[:, off:] = yr[..., :n * 4].reshape(B, H * W * n, 4)
    conf[:, off:] = yr[..., n * 4:].reshape(B, H * W * n, classes)
    written = torch.zeros((B, A, 1), dtype=torch.bool)
    written[:, off:] = True                                              # anchors before the level belong to other levels
    dloc, dconf = ints(g, (B, A, 4), (-2, -1, 1, 2)), ints(g, (B, A, classes), (-2, -1, 1, 2))
    packed = torch.zeros((B, H * W, npad), dtype=torch.bfloat16)
    packed[..., :n * 4] = dloc[:, off:].reshape(B, H * W, n * 4)
    packed[..., n * 4:N] = dconf[:, off:].reshape(B, H * W, n * classes)
    return dict(x=x, w=w, bias=bias, loc=loc, conf=conf, loc_written=written.expand(B, A, 4).clone(),
                conf_written=written.expand(B, A, classes).clone(), dloc=dloc, dconf=dconf, packed=packed, n=n, classes=classes,
                off=off, npad=npad, bf16=("loc", "conf"), fp32=((9 * Cin, x, w),))


def conv_case(case):
    """conv_reference plus what the fused forms return: sign bytes, the non-accumulating masked data gradient"""
    r = conv_reference(case)
    check_conv_regime(case, r)
    r["y_bits"] = pack_bits(r["y_relu"] > 0)
    r["x_bits"] = pack_bits(r["mask_src"].float() > 0)
    r["dx_masked"] = masked(r["dx"], r["mask_src"].float() > 0)
    r["bf16"] = ("y", "y_relu", "dx", "dx_acc", "dx_masked")
    return r


def fwd_pool_case(case, same):
    r = conv_case(case)
    Ho, Wo = r["geom"][:2]
    Hp, Wp = ((Ho + 1) // 2, (Wo + 1) // 2) if same else (Ho // 2, Wo // 2)
    r["yp"], r["code"] = ref_pool(r["y_relu"], 2, 2, 0, 0, Hp, Wp, 4)
    r["bf16"] += ("yp",)
    return r


def unpool_case(B, Hf, Wf, C, Cout, same):
    """the data gradient w.r.t. a pooled map [B,H,W,C] of the 3x3 convolution behind it, carried on through the pooling"""
    g = _gen(B, Hf, Wf, C, Cout, same)
    H, W = ((Hf + 1) // 2, (Wf + 1) // 2) if same else (Hf // 2, Wf // 2)
    full = ints(g, (B, Hf, Wf, C), (-1, 0, 0, 1, 1, 2, 3))
    _, code = ref_pool(full.float(), 2, 2, 0, 0, H, W, 4)
    r = conv_case((B, H, W, C, Cout, 3, 1, "same"))
    r["code"], r["full_shape"] = code, (B, Hf, Wf, C)
    r["dfull"] = ref_unpool(code, r["dx"], r["full_shape"], 2, 2, 0, 0)
    r["dfull_masked"] = ref_unpool(code, r["dx_masked"], r["full_shape"], 2, 2, 0, 0)
    r["bf16"] += ("dfull", "dfull_masked")
    return r


def _wgrad(x, dy, k, stride, pt, pl, dtype=torch.float32):
    B, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    w = torch.zeros((Cout, k, k, Cin), dtype=dtype, requires_grad=True)
    ref_conv(x.to(dtype), w, None, k, stride, pt, pl, Ho, Wo, False).backward(dy.to(dtype))
    return w.grad, dy.to(dtype).sum((0, 1, 2))


def wgrad_unpooled_case(B, H, W, Cin, Cout, same, dtype=torch.float32):
    g = _gen(B, H, W, Cin, Cout, same)
    Hp, Wp = ((H + 1) // 2, (W + 1) // 2) if same else (H // 2, W // 2)
    x = ints(g, (B, H, W, Cin), (0, 0, 1, 2, 3))                          # post-ReLU activations
    y = ints(g, (B, H, W, Cout), (0, 0, 1, 1, 2, 3))                      # the pre-pool map: zeros and ties
    y[:, ::3, ::5] = 0                                                    # whole windows of zeros: code 4 = no gradient
    _, code = ref_pool(y.float(), 2, 2, 0, 0, Hp, Wp, 4)
    dp = ints(g, (B, Hp, Wp, Cout), (-2, -1, 1, 2))
    dyf = ref_unpool(code, dp.float(), y.shape, 2, 2, 0, 0)
    dw, db = _wgrad(x, dyf, 3, 1, 1, 1, dtype)
    return dict(x=x, code=code, dp=dp, dw=dw, dbias=db, fp32=((B * H * W, x, dp),), exact=("dw", "dbias"),
                f64=lambda: wgrad_unpooled_case(B, H, W, Cin, Cout, same, torch.float64))


def wgrad_first_case(B, H, W, dtype=torch.float32):
    """block1_conv2's data gradient (64 -> 64, masked by block1_conv1's sign bytes) times the image patch"""
    g = _gen(B, H, W, 8)
    img = torch.zeros((B, H, W, 8), dtype=torch.bfloat16)
    img[..., :3] = ints(g, (B, H, W, 3), (-2, -1, 1, 2))
    a1 = ints(g, (B, H, W, 64), (0, 0, 1, 2))                             # block1_conv1's activation: only its sign is used
    w1 = ints(g, (64, 3, 3, 64), (-1, 1), 256.0 / 576)
    dy = ints(g, (B, H, W, 64), (-2, -1, 1, 2), 256.0 / 576)
    xr = a1.to(dtype).requires_grad_(True)
    ref_conv(xr, w1.to(dtype), None, 3, 1, 1, 1, H, W, False).backward(dy.to(dtype))
    dx = masked(xr.grad, a1.to(dtype) > 0)                                    # held in bf16 by the kernel: must be bf16-exact
    dw, db = _wgrad(img, dx, 3, 1, 1, 1, dtype)
    w_t = w1.flip(1, 2).permute(3, 1, 2, 0).contiguous()
    return dict(img=img, bits=pack_bits(a1.float() > 0), w_t=w_t, dy=dy, dx=dx, dw=dw, dbias=db, bf16=("dx",),
                fp32=((B * H * W, img, dx), (576, dy, w1)), exact=("dx", "dw", "dbias"),
                f64=lambda: wgrad_first_case(B, H, W, torch.float64))


# (cin, cout, k, stride, mode) of the six layers behind the 19x19 map; input 10x10x512
EXTRA_LAYERS = [(512, 128, 1, 1, "same"), (128, 256, 3, 2, "same"), (256, 128, 1, 1, "same"), (128, 256, 3, 1, "valid"),
                (256, 128, 1, 1, "same"), (128, 256, 3, 1, "valid")]


def extras_geometry(h=10):
    out = []
    for cin, cout, k, s, mode in EXTRA_LAYERS:
        ho, _, pt, _ = geometry(h, h, k, s, mode)
        out.append(dict(cin=cin, cout=cout, k=k, s=s, pt=pt, hin=h, hout=ho))
        h = ho
    return out


def wgrad_batched_case(B, dtype=torch.float32):
    g = _gen(B, 6)
    layers, fp32 = [], []
    for d in extras_geometry():
        x = ints(g, (B, d["hin"], d["hin"], d["cin"]), (0, 1, 2, 3))
        dy = ints(g, (B, d["hout"], d["hout"], d["cout"]), (-2, -1, 1, 2))
        dw, db = _wgrad(x, dy, d["k"], d["s"], d["pt"], d["pt"], dtype)
        layers.append(dict(d, x=x, dy=dy, dw=dw, dbias=db))
        fp32.append((B * d["hout"] ** 2, x, dy))
    r = dict(layers=layers, fp32=fp32, exact=[], f64=lambda: wgrad_batched_case(B, torch.float64))
    for i, l in enumerate(layers):
        r["dw%d" % i], r["db%d" % i] = l["dw"], l["dbias"]
        r["exact"] += ["dw%d" % i, "db%d" % i]
    return r


def chain_case(B, dtype=torch.float32):
    """The six extras as one chain, forward and data gradient.  A layer's output is the next layer's operand, so it must be
    bf16-exact again: the first layer's filters are thinned to 16 taps, the later ones to 2 taps per filter (sums of two
    bf16-exact integers below 128 stay below 256), with a bias that pulls the ReLU's input to exact zeros and negatives."""
    g = _gen(B, 17)
    geo = extras_geometry()
    x = ints(g, (B, 10, 10, 512), (0, 0, 1, 2))
    layers, inp = [], x.to(dtype)
    for i, d in enumerate(geo):
        K = d["k"] * d["k"] * d["cin"]
        w = ints(g, (d["cout"], d["k"], d["k"], d["cin"]), (-1, 1), (16.0 if i == 0 else 2.0) / K)
        bias = ints(g, (d["cout"],), (-2, -1, 0, 1), dtype=torch.float32)
        y = ref_conv(inp, w.to(dtype), bias.to(dtype), d["k"], d["s"], d["pt"], d["pt"], d["hout"], d["hout"], True)
        layers.append(dict(d, w=w, bias=bias, x=inp, y=y, bits=pack_bits(y > 0)))
        inp = y
    # data gradients from the last layer back; the maps that feed a head (inputs of layers 0, 2, 4) already hold a gradient
    gin = ints(g, tuple(layers[-1]["y"].shape), (-2, -1, 1, 2)).to(dtype)
    for i in range(len(geo) - 1, -1, -1):
        l = layers[i]
        xr = l["x"].clone().requires_grad_(True)
        ref_conv(xr, l["w"].to(dtype), None, l["k"], l["s"], l["pt"], l["pt"], l["hout"], l["hout"], False).backward(gin)
        l["head"] = ints(g, tuple(l["x"].shape), (-1, 0, 1)) if i % 2 == 0 else None
        l["gin"] = gin
        l["gout"] = masked(xr.grad + (l["head"].to(dtype) if l["head"] is not None else 0), l["x"] > 0)
        cp = l["cout"]
        l["w_t"] = l["w"].flip(1, 2).permute(3, 1, 2, 0).contiguous()
        gin = l["gout"]
    r = dict(x=x, layers=layers, bf16=[], exact=[], f64=(lambda: chain_case(B, torch.float64)) if dtype == torch.float32 else None)
    for i, l in enumerate(layers):
        r["y%d" % i], r["g%d" % i] = l["y"], l["gout"]
        r["bf16"] += ["y%d" % i, "g%d" % i]
        r["exact"] += ["y%d" % i, "g%d" % i]
    return r


def mx_conv_case(case):
    """conv_case on operands that MX e4m3 holds exactly (checked by the round trip): + the quantised operands and outputs"""
    r = conv_case(case)
    for name in ("x", "w", "dy", "w_t"):
        q, s = ref_quantize_mx(r[name] if name != "w_t" else r["w_t"][..., :case[4]].contiguous())
        assert torch.equal(ref_dequantize_mx(q, s), (r[name] if name != "w_t" else r["w_t"][..., :case[4]]).float()), name
        r[name + "_q"], r[name + "_s"] = q, s
    return r


EXTRAS = {
    "pool2x2 (2,20,20,64) valid": lambda: pool2x2_case(2, 20, 20, 64, False),
    "pool2x2 (2,21,23,64) same": lambda: pool2x2_case(2, 21, 23, 64, True),
    "pool3x3s2 (2,9,9,64)": lambda: pool3x3_case(2, 9, 9, 64),
    "pool3x3s2 (2,37,50,64)": lambda: pool3x3_case(2, 37, 50, 64),
    "eltwise (3,17,19,64)": lambda: eltwise_case((3, 17, 19, 64)),
    "eltwise mxfp8 (3,17,19,256)": lambda: eltwise_case((3, 17, 19, 256)),
    "head (2,5,5,64,6)": lambda: head_case(2, 5, 5, 64, 6),
    "head (2,19,19,256,4)": lambda: head_case(2, 19, 19, 256, 4),
    "head (2,19,19,1024,6)": lambda: head_case(2, 19, 19, 1024, 6),
    "head p512 (3,19,19,256,6)": lambda: head_case(3, 19, 19, 256, 6),
    "relubits image layer (2,40,40,8,64)": lambda: conv_case((2, 40, 40, 8, 64, 3, 1, "same")),
    "relubits (2,30,30,64,64)": lambda: conv_case((2, 30, 30, 64, 64, 3, 1, "same")),
    "fwd_pool (1,33,33,64,96) same": lambda: fwd_pool_case((1, 33, 33, 64, 96, 3, 1, "same"), True),
    "fwd_pool (2,19,19,128,128) valid": lambda: fwd_pool_case((2, 19, 19, 128, 128, 3, 1, "same"), False),
    "fwd_pool p512 (2,33,33,64,128) same": lambda: fwd_pool_case((2, 33, 33, 64, 128, 3, 1, "same"), True),
    "unpool (2,37,45,64,128) same": lambda: unpool_case(2, 37, 45, 64, 128, True),
    "wgrad_unpooled (1,16,16,64,64) valid": lambda: wgrad_unpooled_case(1, 16, 16, 64, 64, False),
    "wgrad_first (3,37,52)": lambda: wgrad_first_case(3, 37, 52),
    "wgrad_first (1,16,16)": lambda: wgrad_first_case(1, 16, 16),
    "wgrad_batched B=16": lambda: wgrad_batched_case(16),
    "chain B=1": lambda: chain_case(1),
    "chain B=5": lambda: chain_case(5),
    "wgrad patch shapes (2,23,45,64,80)": lambda: conv_case((2, 23, 45, 64, 80, 3, 1, "same")),
    "forced strips (2,30,30,64,64)": lambda: conv_case((2, 30, 30, 64, 64, 3, 1, "same")),
    "forced strips (3,17,23,128,96)": lambda: conv_case((3, 17, 23, 128, 96, 3, 1, "same")),
    "forced strips (1,38,38,64,136)": lambda: conv_case((1, 38, 38, 64, 136, 3, 1, "same")),
    "mxfp8 conv3x3 (2,19,19,256,256)": lambda: mx_conv_case((2, 19, 19, 256, 256, 3, 1, "same")),
    "mxfp8 conv2d_fwd (2,19,19,256,64,1)": lambda: mx_conv_case((2, 19, 19, 256, 64, 1, 1, "same")),
    "mxfp8 fwd_pool (1,7,7,128,128) same": lambda: mx_conv_case((1, 7, 7, 128, 128, 3, 1, "same")),
    "mxfp8 bwd_data (2,19,19,64,256,1)": lambda: mx_conv_case((2, 19, 19, 64, 256, 1, 1, "same")),
}
