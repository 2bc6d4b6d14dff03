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


def _bits(t):
    return t.contiguous().view(-1).view(_INT[t.element_size()])


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
            if s.kind == "in" and not torch.equal(_bits(s.tensor), _bits(s.keep)):      # bit for bit: an input may hold a NaN
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
    2^e with e the smallest integer such that amax / 2^e <= 448, clamped to -127 .. 127 (0 for an all-zero block), elements
    v / 2^e rounded to nearest.  A block that holds a NaN or an infinity: 32 bytes 0x7F (NaN) under the scale byte 127."""
    v = t.float().reshape(*t.shape[:-1], t.shape[-1] // 32, 32)
    bad = ~torch.isfinite(v).all(-1)
    v = torch.where(bad.unsqueeze(-1), torch.zeros(()), v)
    amax = v.abs().amax(-1)
    m, ex = torch.frexp(amax / 448.0)
    e = torch.where(amax > 0, torch.where(m == 0.5, ex - 1, ex), torch.zeros_like(ex)).clamp(-127, 127)
    q = (v * torch.exp2(-e.float()).unsqueeze(-1)).to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where(bad.unsqueeze(-1), torch.tensor(0x7F, dtype=torch.uint8), q).reshape(t.shape)
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


def fwd_pool_case(case, same, relu=True, r=None):
    """conv_case plus the pooled map and the winner codes of its output -- of y_relu, or with relu=False of y: a window whose
    maximum is <= 0 then keeps its (negative) value under the code 4.  r: a conv_case of `case` to build on (it is copied)."""
    r = dict(r) if r is not None else conv_case(case)
    Ho, Wo = r["geom"][:2]
    Hp, Wp = ((Ho + 1) // 2, (Wo + 1) // 2) if same else (Ho // 2, Wo // 2)
    r["yp"], r["code"] = ref_pool(r["y_relu" if relu else "y"], 2, 2, 0, 0, Hp, Wp, 4)
    r["bf16"] = tuple(r["bf16"]) + ("yp",)
    return r


def unpool_case(B, Hf, Wf, C, Cout, same):
    """the data gradient w.r.t. a pooled map [B,H,W,C] of the 3x3 convolution behind it, carried on through the pooling"""
    g = _gen(B, Hf, Wf, C, Cout, same)
    H, W = ((Hf + 1) // 2, (Wf + 1) // 2) if same else (Hf // 2, Wf // 2)
    full = ints(g, (B, Hf, Wf, C), (-1, 0, 0, 1, 1, 2, 3))
    _, code = ref_pool(full.float(), 2, 2, 0, 0, H, W, 4)
    r = conv_case((B, H, W, C, Cout, 3, 1, "same"))
    r["code"], r["full_shape"], r["full"] = code, (B, Hf, Wf, C), full
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
    return dict(x=x, y=y, code=code, dp=dp, dy_full=dyf, dw=dw, dbias=db, fp32=((B * H * W, x, dp),), exact=("dw", "dbias"),
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


# ---- MX-fp8 operands whose block scales differ ------------------------------------------------------------------------------------
# mx_conv_case's operands have ONE activation scale byte (120) and one filter scale byte (119), so a kernel that takes the scale of
# a neighbouring block, k-step, tap, pixel or filter passes it.  The two designs below give neighbouring blocks different scales
# and still have ONE exact expected result, whatever the matrix instruction does inside one issue:
#
# A, "cancelling":  x' = x 2^(u(j) + alpha(p)),  w' = w 2^(-u(j) + beta(n) + gamma(t))  for the integer operands x, w of
#    conv_operands, block j, pixel p, filter n, tap t.  Every product of one instruction (one pixel, filter, tap, 128 channels) is
#    x w 2^(alpha + beta + gamma): one power-of-two grid, so any order of accumulation inside the instruction is exact.  Catches
#    a scale taken from another pixel, tap, filter or k-step, and any mis-routing of the blocks of ONE operand -- but not the same
#    block permutation applied to both operands (the u cancel).
# B, "block-isolated":  w is non-zero in one block of each 128-channel k-step only, block (n + tap + kstep) mod 4; every block of
#    x and of w has an independent exponent in -3 .. 3; the all-zero blocks of w carry decoy scale bytes.  An instruction sums
#    products of a single scale pair.  Catches a block permutation common to both operands.
# Across instructions the fp32 accumulator adds multiples of `grid` whose absolute sum stays below 2^24 grid (asserted), so the
# sum is exact in any order and the kernel's ONE bf16 rounding gives the float64 reference rounded once to nearest-even.
U_TABLE = (-3, 2, -1, 3, 1, -2, 3, 0, -2, 0, 2, -3, 3, -1, -3, 1)   # neighbours differ; blocks i, i + 4, i + 8, i + 12 differ
GAMMA = (0, 2, 1, 0, 1, 2, 1, 0, 2)                                  # per tap: consecutive taps differ, rows and columns differ
WIDE = 13                                                            # the wide variant: u spans +-39
# Scale bytes of w's all-zero blocks under design B.  Any byte but 255 is legal there (0 * 2^any = 0); they stay at or below 126 so
# that a zero product's exponent (activation scale <= 123, a zero element 14 binades under a live one) never rises above the live
# products' (scales >= 116 + 117): the expected bits then do not depend on whether the instruction's alignment looks at zeros.
DECOY = (100, 126)


def _pow2_blocks(t, e):
    """integer-valued t [..., C] times 2^e per 32-channel block (e [..., C/32]), in bf16 -- exactly"""
    v = t.float() * torch.exp2(e.float()).repeat_interleave(32, -1)
    out = v.to(torch.bfloat16)
    assert torch.equal(out.float(), v) and bool(torch.isfinite(v).all())
    return out


def isolated_filters(g, shape, reduce_k):
    """filters [N,k,k,C] in {-1,0,1}, non-zero in block (n + tap + kstep) mod 4 of each 128-channel k-step only, there at the
    density of conv_operands times 4"""
    N, k, _, C = shape
    w = ints(g, shape, (-1, 1), min(1.0, 4 * 256.0 / reduce_k))
    j = torch.arange(C) // 32
    n, tap = torch.arange(N).view(N, 1, 1), torch.arange(k * k).view(1, k * k, 1)
    keep = (j % 4).view(1, 1, C) == (n + tap + (j // 4).view(1, 1, C)) % 4
    return (w.float() * keep.view(N, k, k, C)).to(torch.bfloat16)


def mx_design_operands(act, filt, design, wide, g):
    """act [B,h,w,K] and filt [N,k,k,K] (integers, bf16) -> the designed pair with their reference bytes and scales.  Returns
    a dict: a, f (bf16), a_q, a_s, f_q, f_s (ref_quantize_mx), f_s_op (f_s with design B's decoys), grid."""
    B, h, w_, K = act.shape
    N, k = filt.shape[:2]
    nb = K // 32
    if design == "A":
        u = torch.tensor([U_TABLE[j % 16] for j in range(nb)]) * (WIDE if wide else 1)
        alpha = torch.randint(0, 3, (B, h, w_, 1), generator=g)
        beta = torch.randint(0, 3, (N, 1, 1, 1), generator=g)
        gamma = torch.tensor(GAMMA[:k * k]).view(1, k, k, 1)
        ea, ef, grid = u + alpha, -u + beta + gamma, 1.0
    else:
        assert design == "B" and not wide
        ea = torch.randint(-3, 4, (B, h, w_, nb), generator=g)
        ef = torch.randint(-3, 4, (N, k, k, nb), generator=g)
        grid = 2.0 ** -6
    d = dict(a=_pow2_blocks(act, ea), f=_pow2_blocks(filt, ef), grid=grid)
    for name in ("a", "f"):
        q, s = ref_quantize_mx(d[name])
        assert torch.equal(ref_dequantize_mx(q, s), d[name].float()), name        # MX e4m3 holds the operand exactly
        d[name + "_q"], d[name + "_s"] = q, s
    d["f_s_op"] = d["f_s"]
    if design == "B":                                      # decoys: the kernel gets bytes and scales directly, 0 * 2^any = 0
        zero = d["f"].float().view(N, k, k, nb, 32).abs().amax(-1) == 0
        decoy = torch.randint(DECOY[0], DECOY[1] + 1, zero.shape, generator=g).to(torch.uint8)
        d["f_s_op"] = torch.where(zero, decoy, d["f_s"])
        assert torch.equal(ref_dequantize_mx(d["f_q"], d["f_s_op"]), d["f"].float()) and int(zero.sum()) >= 3 * zero.numel() // 4
    return d


def _to_bf16_once(t64):
    """the float64 reference rounded ONCE to bf16: it is exactly an fp32 number (asserted), so float64 -> fp32 does not round"""
    assert torch.equal(t64.float().double(), t64)
    return t64.float().to(torch.bfloat16)


def _dgrad64(dy, w_t, x_shape, k, pt, pl):
    """data gradient (stride 1) of dy [B,Ho,Wo,Cout] through the filters given TRANSPOSED, w_t [Cin,k,k,Cout]; float64"""
    xr = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    w = w_t.permute(3, 1, 2, 0).flip(1, 2).contiguous().double()
    ref_conv(xr, w, None, k, 1, pt, pl, dy.shape[1], dy.shape[2], False).backward(dy.double())
    return xr.grad


def mx_fwd_from_scales(r, xs, ws):
    """the forward of r's BYTES under the scale arrays xs, ws (no ReLU), rounded to bf16: r["y"] for r's own scales"""
    B, H, W, Cin, Cout, k, stride, mode = r["case"]
    Ho, Wo, pt, pl = r["geom"]
    y = ref_conv(ref_dequantize_mx(r["x_q"], xs).double(), ref_dequantize_mx(r["w_q"], ws).double(), r["bias"].double(), k, stride,
                 pt, pl, Ho, Wo, False)
    return y.float().to(torch.bfloat16)


def mx_dgrad_from_scales(r, dys, wts):
    B, H, W, Cin, Cout, k, stride, mode = r["case"]
    Ho, Wo, pt, pl = r["geom"]
    dx = _dgrad64(ref_dequantize_mx(r["dy_q"], dys), ref_dequantize_mx(r["w_t_q"], wts), (B, H, W, Cin), k, pt, pl)
    return dx.float().to(torch.bfloat16)


def _design_gen(case, design, wide, salt):
    return torch.Generator().manual_seed((case_seed(case) * 31 + {"A": 1, "B": 2}[design] + (4 if wide else 0) + salt) % 100003)


_MX_CACHE = {}


def mx_fwd_design(case, design, wide=False):
    """Forward operands of design A or B for a (B,H,W,Cin,Cout,k,stride,mode) case (cached: treat as read-only): x, w (bf16),
    x_q, x_s, w_q, w_s = ref_quantize_mx of them, w_s_op = the scale bytes the kernel gets (design B: with decoys), bias, the
    float64 reference y64 and the expected bf16 maps y, y_relu, and `bound` = max sum |terms| / grid."""
    key = ("fwd", tuple(case[:8]), design, wide)
    if key in _MX_CACHE:
        return _MX_CACHE[key]
    B, H, W, Cin, Cout, k, stride, mode = case[:8]
    o = conv_operands(case)
    Ho, Wo, pt, pl = o["geom"]
    g = _design_gen(case, design, wide, 0)
    w_int = o["w"] if design == "A" else isolated_filters(g, (Cout, k, k, Cin), k * k * Cin)
    d = mx_design_operands(o["x"], w_int, design, wide, g)
    r = dict(case=tuple(case[:8]), design=design, wide=wide, geom=o["geom"], bias=o["bias"], grid=d["grid"], x=d["a"], w=d["f"],
             x_q=d["a_q"], x_s=d["a_s"], w_q=d["f_q"], w_s=d["f_s"], w_s_op=d["f_s_op"])
    x64, w64, b64 = r["x"].double(), r["w"].double(), r["bias"].double()
    r["y64"] = ref_conv(x64, w64, b64, k, stride, pt, pl, Ho, Wo, False)
    r["bound"] = float(ref_conv(x64.abs(), w64.abs(), b64.abs(), k, stride, pt, pl, Ho, Wo, False).max()) / r["grid"]
    r["y"], r["y_relu"] = _to_bf16_once(r["y64"]), _to_bf16_once(r["y64"].relu())
    check_mx_regime(r)
    _MX_CACHE[key] = r
    return r


def mx_dgrad_design(case, design, wide=False):
    """Data-gradient operands of design A or B (stride 1; the blocks run over Cout): dy, w_t [Cin,k,k,Cout] (bf16), dy_q, dy_s,
    w_t_q, w_t_s, w_t_s_op, the accumulate base and ReLU mask source of conv_operands, the float64 reference dx64 and the expected
    bf16 maps dx, dx_masked = dx where mask_src > 0, dx_acc = (dx + base) where mask_src > 0, as conv_reference."""
    key = ("dgrad", tuple(case[:8]), design, wide)
    if key in _MX_CACHE:
        return _MX_CACHE[key]
    B, H, W, Cin, Cout, k, stride, mode = case[:8]
    assert stride == 1 and Cout % 128 == 0
    o = conv_operands(case)
    Ho, Wo, pt, pl = o["geom"]
    g = _design_gen(case, design, wide, 8)
    wt_int = o["w"].flip(1, 2).permute(3, 1, 2, 0).contiguous() if design == "A" else isolated_filters(g, (Cin, k, k, Cout), k * k * Cin)
    d = mx_design_operands(o["dy"], wt_int, design, wide, g)
    r = dict(case=tuple(case[:8]), design=design, wide=wide, geom=o["geom"], grid=d["grid"], dy=d["a"], w_t=d["f"], dy_q=d["a_q"],
             dy_s=d["a_s"], w_t_q=d["f_q"], w_t_s=d["f_s"], w_t_s_op=d["f_s_op"], mask_src=o["mask_src"], base=o["base"])
    keep = r["mask_src"].float() > 0
    r["dx64"] = _dgrad64(r["dy"], r["w_t"], (B, H, W, Cin), k, pt, pl)
    r["bound"] = float((_dgrad64(r["dy"].abs(), r["w_t"].abs(), (B, H, W, Cin), k, pt, pl) + r["base"].double().abs()).max()) / r["grid"]
    r["dx"], r["dx_masked"] = _to_bf16_once(r["dx64"]), _to_bf16_once(masked(r["dx64"], keep))
    r["dx_acc"] = _to_bf16_once(masked(r["dx64"] + r["base"].double(), keep))
    check_mx_regime(r)
    _MX_CACHE[key] = r
    return r


def check_mx_regime(r):
    """the accumulator adds exactly: every term is a multiple of grid and the absolute sum stays below 2^24 grid"""
    assert r["bound"] < 2 ** 24, (r["case"], r["design"], r["bound"])
    ref = r["y64"] if "y64" in r else r["dx64"]
    assert torch.equal((ref / r["grid"]).round(), ref / r["grid"]) and torch.equal(ref.float().double(), ref)


def mx_eltwise_case(shape):
    """eltwise_case's integers times a power of two per 32-channel block (both addends the same one): sums exact in bf16, block
    maxima over 2^-20 .. 2^22"""
    r = eltwise_case(shape)
    e = torch.randint(-20, 21, tuple(shape[:-1]) + (shape[-1] // 32,), generator=_gen(*shape, 5))
    a, b = _pow2_blocks(r["a"], e), _pow2_blocks(r["b"], e)
    out = (a.float() + b.float()).relu()
    assert in_bf16_regime(out)
    return dict(a=a, b=b, out=out, bf16=("out",))


def mx_scale_mutations(r, a_s, f_s, k, design):
    """[(name, mutated a_s, mutated f_s)]: the wrong scale routings the designs must expose.  a_s [B,h,w,nb] activation scales,
    f_s [N,k,k,nb] filter scales (the operand ones).  Swaps of blocks inside every k-step on ONE operand under design A, on
    both under design B; two k-steps swapped; the scale of the pixel to the right / below, of the next tap, of the next filter."""
    nb = a_s.shape[-1]

    def perm(t, p):
        return t[..., torch.tensor(p)]
    out = []
    for i in range(3):
        p = list(range(nb))
        for s in range(0, nb, 4):
            p[s + i], p[s + i + 1] = p[s + i + 1], p[s + i]
        if design == "A":
            out += [("x blocks %d<->%d" % (i, i + 1), perm(a_s, p), f_s), ("w blocks %d<->%d" % (i, i + 1), a_s, perm(f_s, p))]
        else:
            out.append(("both blocks %d<->%d" % (i, i + 1), perm(a_s, p), perm(f_s, p)))
    if nb >= 8:
        p = list(range(4, 8)) + list(range(0, 4)) + list(range(8, nb))
        out.append(("k-steps 0<->1", perm(a_s, p), f_s if design == "A" else perm(f_s, p)))
    out.append(("pixel to the right", a_s.roll(-1, 2), f_s))
    out.append(("pixel below", a_s.roll(-1, 1), f_s))
    if k == 3:
        out.append(("next tap", a_s, f_s.reshape(f_s.shape[0], 9, nb).roll(-1, 1).reshape(f_s.shape)))
    out.append(("next filter", a_s, f_s.roll(-1, 0)))
    return out


def _same(*cases):
    return [tuple(c) + ("same",) for c in cases]


# the cases of tests/test_mxfp8_strict_gpu.py (B, H, W, Cin, Cout, k, stride, mode): the smallest shapes that reach each path
MX_CONV3X3_CASES = _same((2, 19, 19, 256, 256, 3, 1), (1, 5, 5, 512, 96, 3, 1))      # a tail tile of pixels; 4 k-steps, a Cout tail
MX_CONV2D_CASES = _same((2, 7, 7, 512, 64, 1, 1), (2, 9, 11, 256, 160, 1, 2), (3, 17, 13, 128, 160, 3, 1), (1, 9, 11, 128, 96, 3, 2),
                        (2, 8, 8, 256, 128, 3, 2))                                       # the last: TF-SAME pad 0 at top and left
MX_POOL_CASES = _same((1, 7, 7, 128, 128, 3, 1), (3, 8, 8, 256, 160, 3, 1))           # 48 windows: a tail tile, images share a tile
MX_DGRAD_CASES = _same((2, 15, 15, 96, 256, 3, 1), (2, 19, 19, 64, 256, 1, 1), (1, 9, 11, 256, 512, 3, 1))
MX_WIDE_FWD_CASE, MX_WIDE_DGRAD_CASE = MX_CONV2D_CASES[0], MX_DGRAD_CASES[1]
MX_FWD_CASES = MX_CONV3X3_CASES + MX_CONV2D_CASES + MX_POOL_CASES


EXTRAS = {
    "pool2x2 (2,20,20,64) valid": lambda: pool2x2_case(2, 20, 20, 64, False),
    "pool2x2 (2,21,23,64) same": lambda: pool2x2_case(2, 21, 23, 64, True),
    "pool2x2 (2,21,23,64) valid": lambda: pool2x2_case(2, 21, 23, 64, False),   # the last row / column lies in no window
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


# ---- the SSD loss: exact logits ------------------------------------------------------------------------------------------------
# Every row has one maximum m (a small integer) and every other logit is at most m - 1024, so exp(z - m) is exactly 0 in fp32 and
# in float64, the row sum is exactly 1, its log exactly 0 and lse = m.  The background key m - z[C-1] and a positive's label CE
# m - z[label] are then exact fp32 numbers that the case CHOOSES, the softmax is exactly one-hot, and every gradient entry is 0 or
# +-grad_scale / P or +-grad_scale / N: oracle.ssd_oracle.ssd_loss (float64) returns values that convert to the output dtype
# without rounding, and the mining threshold can be put on any bit pattern at or above 1024.
FILL = (-2048.0, -4096.0, -8192.0, -1048576.0)                 # the logits that are neither the maximum nor chosen: <= m - 1024


def f32_bits(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _low_bit_exponent(v):
    """exponent e of the lowest set bit 2^e of every (positive, normal) fp32 value"""
    b = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    mant = (b & 0x7FFFFF) | 0x800000
    tz = np.log2((mant & -mant).astype(np.float64)).astype(np.int64)
    return ((b >> 23) & 0xFF) - 127 - 23 + tz


def sums_exactly(values):
    """a float64 sum of these non-negative fp32 values is exact in any order: all are multiples of a quantum q = 2^e and the total
    is below 2^53 q, so no partial sum of any grouping rounds"""
    v = np.asarray(values, dtype=np.float32).astype(np.float64)
    v = v[v != 0]
    if v.size == 0:
        return True
    assert (v > 0).all()
    q = 2.0 ** int(_low_bit_exponent(v.astype(np.float32)).min())
    import math
    return math.fsum(v / q) < 2.0 ** 53


def _holds(v32, dtype):
    """the fp32 values survive the cast to `dtype`"""
    if dtype == torch.float32:
        return np.ones(v32.shape, dtype=bool)
    return (np.ascontiguousarray(v32, dtype=np.float32).view(np.uint32) & 0xFFFF) == 0


def scatter_keys(n, P, keys, seed):
    """(mask bool[n], key f32[n]): P positives at seeded random places, `keys` (n - P of them) on the other rows in a seeded
    random order, so that the selected rows fall into many blocks"""
    keys = np.asarray(keys, dtype=np.float32)
    assert keys.shape == (n - P,), (keys.shape, n, P)
    rng = np.random.default_rng(seed)
    mask = np.zeros(n, dtype=bool)
    mask[rng.choice(n, P, replace=False)] = True
    key = np.zeros(n, dtype=np.float32)
    key[~mask] = rng.permutation(keys)
    return mask, key


def loss_case(B, A, C, mask, key, pos_ce=None, dtype=torch.float32, grad_scale=1.0, seed=0, design=None):
    """An exact case of ssd_loss_fwd_bwd.  mask bool[B*A]: the positives; key f32[B*A]: the background CE of every other row, 0
    (the background is the row's maximum) or >= 1024; pos_ce f32[B*A]: a positive's label CE, 0 (the label is the maximum: an
    all-zero gradient row that is still selected) or >= 1024 (default: a seeded mix of 0, 1024, 1536 and 2048).
    Returns the inputs (torch, CPU) and the expected out8 / dconf / dloc: oracle.ssd_oracle.ssd_loss on the same inputs, the
    scalars cast to fp32 (out8[3] their fp32 sum in k_loss_final's order), the gradient's entries -- the oracle's signs -- scaled
    by the fp32 quotients grad_scale / P and grad_scale / N and cast to `dtype`.  P == 0 or 3P > B*A: status 1, zero gradients."""
    from oracle import ssd_oracle as O
    n = B * A
    rng = np.random.default_rng(1000 + seed)
    mask = np.asarray(mask, dtype=bool).reshape(n)
    key = np.where(mask, 0, np.asarray(key, dtype=np.float32).reshape(n)).astype(np.float32)
    if pos_ce is None:
        pos_ce = rng.choice(np.array([0.0, 1024.0, 1536.0, 2048.0], dtype=np.float32), n)
    pos_ce = np.where(mask, np.asarray(pos_ce, dtype=np.float32).reshape(n), 0).astype(np.float32)
    chosen = np.where(mask, pos_ce, key)                        # the one logit below the maximum that the case chooses: m - chosen
    assert ((chosen == 0) | (chosen >= 1024)).all()
    label = rng.integers(0, C - 1, n)                           # foreground classes 0 .. C-2
    other = (label + 1 + rng.integers(0, C - 1, n)) % C         # any class but the label
    fg = rng.integers(0, C - 1, n)
    # the class that holds the maximum / the class that holds m - chosen
    top = np.where(mask, np.where(pos_ce == 0, label, other), np.where(key == 0, C - 1, fg))
    low = np.where(mask, label, C - 1)
    m_pref = rng.choice(np.array([0.0, 4.0, -4.0, 0.0, 256.0] if dtype == torch.bfloat16 else [0.0, 4.0, -4.0]), n)
    z64 = m_pref - chosen.astype(np.float64)
    z32 = z64.astype(np.float32)
    ok = (z32.astype(np.float64) == z64) & _holds(z32, dtype) & (m_pref - z32.astype(np.float64) == chosen)
    m = np.where(ok | (chosen == 0), m_pref, 0.0)
    conf = rng.choice(np.array(FILL, dtype=np.float32), (n, C))
    rows = np.arange(n)
    has_low = chosen != 0
    conf[rows[has_low], low[has_low]] = (m - chosen.astype(np.float64))[has_low].astype(np.float32)
    conf[rows, top] = m.astype(np.float32)
    loc = rng.integers(-8, 9, (n, 4)).astype(np.float32) / 4
    gt_loc = rng.integers(-8, 9, (n, 4)).astype(np.float32) / 4
    gt_loc[~mask] = 12345.0                                     # never read
    gt_loc[rows[mask][::3], 1] = loc[rows[mask][::3], 1]        # exact zeros of the difference: sign 0
    gt_cls = np.where(mask, label, rng.integers(0, C, n)).astype(np.int32)
    r = dict(B=B, A=A, C=C, dtype=dtype, grad_scale=float(grad_scale), design=design or {}, m=m, key=key, pos_ce=pos_ce,
             conf=torch.from_numpy(conf).view(B, A, C).to(dtype), loc=torch.from_numpy(loc).view(B, A, 4).to(dtype),
             gt_cls=torch.from_numpy(gt_cls).view(B, A), gt_loc=torch.from_numpy(gt_loc).view(B, A, 4),
             gt_mask=torch.from_numpy(mask.astype(np.uint8)).view(B, A))
    assert torch.equal(r["conf"].float(), torch.from_numpy(conf).view(B, A, C)), "a logit does not survive the cast"
    P = int(mask.sum())
    out8 = np.zeros(8, dtype=np.float32)
    out8[4] = P
    if P == 0 or 3 * P > n:
        out8[7] = 1.0
        r.update(status=1, P=P, N=0, selected=np.zeros(n, dtype=bool), ref=None,
                 dconf=torch.zeros((B, A, C), dtype=dtype), dloc=torch.zeros((B, A, 4), dtype=dtype))
    else:
        ref = O.ssd_loss(gt_cls.reshape(B, A), gt_loc.reshape(B, A, 4), mask.reshape(B, A), loc.reshape(B, A, 4),
                         conf.reshape(B, A, C), want_grad=True)
        N = ref["num_neg"]
        gs = np.float32(grad_scale)
        inv_p, inv_n = gs / np.float32(P), gs / np.float32(N)
        scale = np.where(mask, inv_p, inv_n).astype(np.float32).reshape(B, A, 1)
        dconf = (np.sign(ref["dcls"]).astype(np.float32) * scale + np.float32(0)).astype(np.float32)
        dloc = (np.sign(ref["dbox"]).astype(np.float32) * inv_p + np.float32(0)).astype(np.float32)
        out8[0], out8[1], out8[2] = np.float32(ref["loc"]), np.float32(ref["pos"]), np.float32(ref["neg"])
        out8[3] = (out8[0] + out8[1]) + out8[2]
        out8[5], out8[6] = N, np.float32(ref["tau"])
        r.update(status=0, P=P, N=N, ref=ref, selected=mask | ref["neg_mask"].reshape(n), inv_p=inv_p, inv_n=inv_n,
                 dconf=torch.from_numpy(dconf).to(dtype), dloc=torch.from_numpy(dloc).to(dtype))
    r["out8"] = torch.from_numpy(out8)
    return r


def check_loss_regime(r):
    """The conditions under which the expected outputs of loss_case are exact, on the inputs and the float64 reference."""
    B, A, C, dtype = r["B"], r["A"], r["C"], r["dtype"]
    n = B * A
    z = r["conf"].float().numpy().reshape(n, C)
    mask = r["gt_mask"].numpy().reshape(n).astype(bool)
    m = z.max(-1)
    assert np.array_equal(m, r["m"].astype(np.float32)) and ((z == m[:, None]).sum(-1) == 1).all(), "one maximum per row"
    assert (np.exp((z - m[:, None]).astype(np.float32)).astype(np.float32).sum(-1, dtype=np.float32) == 1).all()
    assert (np.exp(z.astype(np.float64) - m[:, None]).sum(-1) == 1).all()
    # the kernel's fp32 formulas restated: the keys and the label CEs are the chosen numbers, bit for bit
    key32 = np.where(mask, np.float32(0), (m - z[:, C - 1]) + np.log(np.float32(1)))
    assert np.array_equal(key32.view(np.uint32), r["key"].view(np.uint32))
    lab = r["gt_cls"].numpy().reshape(n)
    ce32 = (m - z[np.arange(n), lab])[mask]
    assert np.array_equal(ce32, r["pos_ce"][mask])
    assert len(set(np.unique(m[~mask]))) > 1 or n < 8 or dtype == torch.bfloat16, "the maximum varies between rows"
    loc, gl = r["loc"].float().numpy().reshape(n, 4), r["gt_loc"].numpy().reshape(n, 4)
    assert np.array_equal(loc * 4, np.round(loc * 4)) and np.array_equal(gl[mask] * 4, np.round(gl[mask] * 4))
    if r["status"] != 0:
        return
    ref, P, N, gs = r["ref"], r["P"], r["N"], r["grad_scale"]
    neg = ref["neg_mask"].reshape(n)
    assert not (neg & mask).any() and ref["tau"] >= 1024 and int(neg.sum()) == N
    tau32 = np.float32(ref["tau"])
    assert float(tau32) == ref["tau"]
    # rank and ties as designed; no key lies within the tie by accident
    keys = r["key"][~mask]
    above, tie = int((keys > tau32).sum()), int((keys == tau32).sum())
    assert above < 3 * P <= above + tie and N == above + tie
    d = r["design"]
    for name, got in (("N", N), ("tie", tie), ("rank_in_tie", 3 * P - above), ("tau_bits", int(tau32.view(np.uint32)))):
        if name in d:
            assert d[name] == got, (name, d[name], got)
    # the three sums are exact in float64 whatever their order
    assert sums_exactly(keys[keys >= tau32]) and sums_exactly(r["pos_ce"][mask]) and sums_exactly(np.abs(loc - gl)[mask].sum(-1))
    # the gradient: the oracle's entries are 0 or +-1/P or +-1/N; where P, N and grad_scale are powers of two the scaled float64
    # reference converts to the output dtype without rounding and equals the expected tensor
    pow2 = all(v > 0 and float(np.log2(v)).is_integer() for v in (P, N, gs))
    r["pow2"] = pow2
    vals = np.unique(np.abs(ref["dcls"]))
    assert set(vals) <= {0.0, 1.0 / P, 1.0 / N}
    if pow2:
        for name, key in (("dconf", "dcls"), ("dloc", "dbox")):
            want = torch.from_numpy(ref[key] * gs)
            assert torch.equal(want.to(dtype).double(), want), name
            assert torch.equal(r[name].double(), want), name
    for i, name in enumerate(("loc", "pos", "neg")):
        assert np.isfinite(r["out8"][i].item())
    assert np.isfinite(r["out8"][3].item())


# (H, W, per_cell) per level
GEOM8 = ((19, 19, 4), (7, 5, 6), (5, 7, 6), (3, 3, 6), (2, 3, 4), (2, 2, 4), (1, 2, 4), (1, 1, 4))
GEOM7 = ((8, 8, 4), (4, 4, 6), (3, 4, 6), (2, 2, 6), (2, 1, 6), (1, 1, 4), (1, 1, 4))
GEOM1 = ((6, 7, 4),)


def anchors_of(geom):
    return sum(h * w * n for h, w, n in geom)


def heads_expected(r, geom, npad):
    """The compact-row form of a loss_case by the header's contract, from the oracle's selection: per level count, pixel_of_row
    (ascending flat pixel b*hw + pix), row_of_pixel (-1 where unselected) and the rows [per_cell*4 loc | per_cell*C conf | 0]"""
    B, A, C = r["B"], r["A"], r["C"]
    assert anchors_of(geom) == A and r["dtype"] == torch.bfloat16
    sel = torch.from_numpy(r["selected"]).view(B, A)
    out, off = [], 0
    for (h, w, n), p in zip(geom, npad):
        hw = h * w
        assert p % 8 == 0 and p >= n * (4 + C)
        pix = sel[:, off:off + hw * n].reshape(B * hw, n).any(-1)
        por = pix.nonzero()[:, 0].to(torch.int32)
        rop = torch.full((B * hw,), -1, dtype=torch.int32)
        rop[por.long()] = torch.arange(por.numel(), dtype=torch.int32)
        full = torch.zeros((B * hw, p), dtype=torch.bfloat16)
        full[:, :n * 4] = r["dloc"][:, off:off + hw * n].reshape(B * hw, n * 4)
        full[:, n * 4:n * (4 + C)] = r["dconf"][:, off:off + hw * n].reshape(B * hw, n * C)
        rows = torch.zeros((B * hw, p), dtype=torch.bfloat16)
        rows[:por.numel()] = full[por.long()]
        assert not bool((full[~pix] != 0).any())                    # an unselected pixel carries no gradient
        out.append(dict(hw=hw, H=h, W=w, n=n, npad=p, off=off, count=int(por.numel()), pixel_of_row=por, row_of_pixel=rop,
                        rows=rows, dense=full.view(B, h, w, p)))
        off += hw * n
    return out


# ---- the catalogue of exact loss cases ------------------------------------------------------------------------------------------
def _fill_keys(count, seed, dtype=torch.float32):
    """`count` keys that stay below every threshold of the catalogue (all thresholds are >= 1536): exact zeros (the background is
    the maximum) and values of [1024, 1536) that differ in their low bits"""
    rng = np.random.default_rng(77 + seed)
    step = 8 if dtype == torch.bfloat16 else 1
    lo = f32_bits(0x44800000 + step * 0x10000 * rng.integers(0, 0x400000 // (step * 0x10000), count)) if dtype == torch.bfloat16 \
        else f32_bits(0x44800000 + rng.integers(0, 0x400000, count))
    assert ((lo >= 1024) & (lo < 1536)).all()
    return np.where(rng.random(count) < 0.3, np.float32(0), lo).astype(np.float32)


def tie_case(B, A, C, P, top, tie_value, tie, rank_in_tie, dtype=torch.float32, grad_scale=1.0, seed=0, below=()):
    """3P - rank_in_tie keys of `top` (all above tie_value, the smallest of them) above a tie group of `tie` keys at tie_value; the
    threshold is member rank_in_tie of the group, N = 3P - rank_in_tie + tie.  `below`: keys under tie_value that share its
    radix prefix; the remaining rows hold keys below 1536."""
    n = B * A
    above = 3 * P - rank_in_tie
    top = np.sort(np.asarray(top, dtype=np.float32))[:above]
    below = np.asarray(below, dtype=np.float32)
    assert top.size == above and (top > tie_value).all() and tie_value >= 1536 and 1 <= rank_in_tie <= tie
    assert (below < tie_value).all()
    rest = n - P - above - tie - below.size
    keys = np.concatenate([top, np.full(tie, tie_value, dtype=np.float32), below, _fill_keys(rest, seed, dtype)])
    mask, key = scatter_keys(n, P, keys, seed)
    design = dict(N=above + tie, tie=tie, rank_in_tie=rank_in_tie, tau_bits=int(np.float32(tie_value).view(np.uint32)))
    return loss_case(B, A, C, mask, key, dtype=dtype, grad_scale=grad_scale, seed=seed, design=design)


def level3_keys():
    """1024 consecutive floats that share their top 22 bits (one level-2 bin of the radix select): only the low digit differs"""
    return f32_bits(0x45000400 + np.arange(1024))


def level2_keys(seed=0):
    """one key in each of 1500 level-2 bins of one level-1 bin (top 11 bits shared), random low digits"""
    rng = np.random.default_rng(5 + seed)
    bins = rng.choice(2048, 1500, replace=False)
    return np.sort(f32_bits(0x45000000 + (bins << 10) + rng.integers(0, 1024, 1500)))


def level1_keys():
    """four keys per binade from 2^10 to 2^127 -- one per level-1 bin, 472 bins, owned by 59 threads of find_bin -- and FLT_MAX"""
    e = np.repeat(np.arange(10, 128), 4)
    q = np.tile(np.arange(4), 118)
    return np.concatenate([((1 + q / 4.0) * 2.0 ** e).astype(np.float32), f32_bits([0x7F7FFFFF])])        # ascending


def bf16_keys(count):
    """the `count` smallest bf16 values above 1536"""
    return f32_bits((0x44C00000 + 0x10000 * (1 + np.arange(count))).astype(np.uint32))


def _dense_catalogue():
    f32, bf = torch.float32, torch.bfloat16
    c = {}
    # radix level 3 decides: the threshold's key is the first / a middle / the last member of its level-3 bin (one fp32 value)
    k3, k2, k1 = level3_keys(), level2_keys(), level1_keys()
    for name, rank in (("first", 1), ("middle", 3), ("last", 5)):
        c["level3 %s (2,300,21) f32" % name] = lambda rank=rank: tie_case(2, 300, 21, 16, k3[500:], k3[499], 5, rank, seed=rank, below=k3[:499])
    c["level3 all 1024 low digits (4,500,21) f32"] = lambda: tie_case(4, 500, 21, 300, k3[125:], k3[124], 2, 1, seed=4, below=k3[:124])
    c["level2 (4,500,5) f32"] = lambda: tie_case(4, 500, 5, 200, k2[901:], k2[900], 3, 2, seed=6, below=k2[:900])
    # (the selected keys start at 1.5 * 2^104: their float64 sum is exact, see sums_exactly)
    c["level1 (3,301,21) f32"] = lambda: tie_case(3, 301, 21, 32, k1[379:], k1[378], 2, 2, seed=7, below=k1[:378])
    for dt, tag in ((f32, "f32"), (bf, "bf16")):
        c["tie straddles 3P (2,300,21) %s" % tag] = lambda dt=dt: tie_case(2, 300, 21, 16, bf16_keys(64)[1:], bf16_keys(64)[0], 21, 5, dtype=dt, seed=8)
        c["tie ends at 3P (2,300,21) %s" % tag] = lambda dt=dt: tie_case(2, 300, 21, 16, bf16_keys(64)[1:], bf16_keys(64)[0], 6, 6, dtype=dt, seed=9)
        # every negative selected: 3P = n - P, the threshold is the smallest key
        c["every negative (2,128,21) %s" % tag] = lambda dt=dt: tie_case(2, 128, 21, 64, bf16_keys(200)[1:], bf16_keys(200)[0], 1, 1, dtype=dt, seed=10)
        c["n=4 P=1 (1,4,21) %s" % tag] = lambda dt=dt: tie_case(1, 4, 21, 1, bf16_keys(3)[1:], bf16_keys(3)[0], 1, 1, dtype=dt, seed=11)
        c["odd tail (3,301,21) %s" % tag] = lambda dt=dt: tie_case(3, 301, 21, 32, bf16_keys(128)[1:], bf16_keys(128)[0], 40, 7, dtype=dt, seed=12)
        for C in (2, 5, 81, 112, 288, 303):
            c["C=%d (3,301,%d) %s" % (C, C, tag)] = lambda dt=dt, C=C: tie_case(3, 301, C, 32, bf16_keys(128)[1:], bf16_keys(128)[0], 40, 7, dtype=dt, seed=13 + C)
        c["status 1: P=0 (2,150,21) %s" % tag] = lambda dt=dt: loss_case(2, 150, 21, np.zeros(300, dtype=bool), _fill_keys(300, 1, dt), dtype=dt, seed=14)
        c["status 1: 3P>n (2,150,21) %s" % tag] = lambda dt=dt: loss_case(2, 150, 21, np.arange(300) % 3 != 1, bf16_keys(300), dtype=dt, seed=15)
    # more rows than persistent workgroups of k_loss_rows (768 x 128) and than one stride of k_loss_hist (256 x 256 keys)
    c["persistent (5,19661,81) bf16"] = lambda: tie_case(5, 19661, 81, 512, bf16_keys(1700)[1:], bf16_keys(1700)[0], 600, 88, dtype=bf, seed=16)
    c["persistent (5,19661,4) f32"] = lambda: tie_case(5, 19661, 4, 512, level3_keys()[100:].repeat(2), level3_keys()[99], 3, 2, seed=17, below=level3_keys()[:99])
    return c


LOSS_CASES = _dense_catalogue()
_LOSS_CACHE = {}


def loss_cached(name, table=None):
    """a case of the catalogue, built once per process and never modified"""
    table = LOSS_CASES if table is None else table
    if name not in _LOSS_CACHE:
        _LOSS_CACHE[name] = table[name]()
    return _LOSS_CACHE[name]


# ---- exact loss cases for the compact-row form: P, N = 4P and grad_scale are powers of two ------------------------------------
def heads_loss_case(B, geom, C, P, full=(), empty=(), empty_img=(), grad_scale=1.0, seed=0, rank_in_tie=1):
    """5P selected anchors at chosen places: one per pixel of every level in `full` (every pixel gets a row), none in the levels
    of `empty`, none in (image, level) of `empty_img`, the rest at seeded random places.  P of them are positives, 3P -
    rank_in_tie hold distinct keys above a tie group of P + rank_in_tie at 1544: N = 4P.  bf16."""
    A = anchors_of(geom)
    n = B * A
    rng = np.random.default_rng(300 + seed)
    allowed = np.ones((B, A), dtype=bool)
    chosen = np.zeros((B, A), dtype=bool)
    off = 0
    for l, (h, w, k) in enumerate(geom):
        sl = slice(off, off + h * w * k)
        if l in empty:
            allowed[:, sl] = False
        for b, le in empty_img:
            if le == l:
                allowed[b, sl] = False
        if l in full:
            pick = off + np.arange(h * w) * k + rng.integers(0, k, (B, h * w))
            chosen[np.arange(B)[:, None], pick] = True
        for b in range(B):                                      # at least one selected anchor wherever any is allowed
            if allowed[b, off]:
                chosen[b, off + rng.integers(0, h * w * k)] = True
        off += h * w * k
    need = 5 * P - int(chosen.sum())
    free = np.flatnonzero((allowed & ~chosen).reshape(n))
    assert 0 <= need <= free.size, (need, free.size)
    chosen.reshape(n)[rng.choice(free, need, replace=False)] = True
    sel = rng.permutation(np.flatnonzero(chosen.reshape(n)))
    mask = np.zeros(n, dtype=bool)
    mask[sel[:P]] = True
    above, tie = 3 * P - rank_in_tie, P + rank_in_tie
    keys = bf16_keys(above + 1)
    key = np.zeros(n, dtype=np.float32)
    key[sel[P:P + above]] = keys[1:]
    key[sel[P + above:]] = keys[0]
    rest = np.flatnonzero(~chosen.reshape(n))
    key[rest] = _fill_keys(rest.size, seed, torch.bfloat16)
    design = dict(N=4 * P, tie=tie, rank_in_tie=rank_in_tie)
    r = loss_case(B, A, C, mask, key, dtype=torch.bfloat16, grad_scale=grad_scale, seed=seed, design=design)
    assert np.array_equal(r["selected"], chosen.reshape(n))
    r["geom"] = geom
    r["npad"] = tuple((k * (4 + C) + 7) // 8 * 8 + (8 if C == 5 else 0) + (16 if C == 5 and k == 6 else 0) for _, _, k in geom)
    r["levels"] = heads_expected(r, geom, r["npad"])
    return r


HEADS_LOSS_CASES = {
    # a level with every pixel selected (19 x 19: two chunks of k_hg_assign), one without any, an image without any in a level
    "8 levels B=3 C=81": lambda: heads_loss_case(3, GEOM8, 81, 256, full=(0,), empty=(5,), empty_img=((1, 2), (0, 7)), grad_scale=4.0, seed=1),
    "8 levels B=1 C=5": lambda: heads_loss_case(1, GEOM8, 5, 64, empty=(7,), seed=2),
    "7 levels B=3 C=81": lambda: heads_loss_case(3, GEOM7, 81, 64, full=(0, 3), empty_img=((1, 1),), seed=3, rank_in_tie=5),
    "1 level B=1 C=5": lambda: heads_loss_case(1, GEOM1, 5, 8, grad_scale=0.5, seed=4),
    "1 level B=3 C=81": lambda: heads_loss_case(3, GEOM1, 81, 32, full=(0,), seed=5),
    # a second batch of the first geometry: the inputs Y of the ws_clean cases
    "8 levels B=3 C=81 second": lambda: heads_loss_case(3, GEOM8, 81, 128, empty=(1,), seed=6),
}


def heads_cached(name):
    return loss_cached(name, HEADS_LOSS_CASES)


# ---- the sparse head backward kernels: hand-made compact rows ---------------------------------------------------------------------
UNREAD = 2.0 ** 100                                            # (finite: the arena compares inputs with torch.equal)


def hand_rows(g, B, H, W, n, C, npad, count):
    """ssd_head_grads contents of one level with `count` rows, as the loss writes them: ascending pixel_of_row that holds the
    four corners and an edge pixel of image 0 first (as far as count allows), the inverse map, and rows with the entries of one
    or two selected anchors -- a positive's +-2^-6 on its offsets, its label and the row maximum, a mined negative's +-2^-8 on
    the row maximum and the background.  Rows and indices past `count` hold what must never be read (2^100; pixel 0)."""
    hw, total = H * W, B * H * W
    assert 0 <= count <= total
    must = [0, W - 1, (H - 1) * W, hw - 1, (H // 2) * W, W // 2, (H // 2) * W + W - 1, (H - 1) * W + W // 2]
    must = list(dict.fromkeys(must))[:count]
    rest = [p for p in torch.randperm(total, generator=g).tolist() if p not in must][:count - len(must)]
    por = torch.tensor(sorted(must + rest), dtype=torch.int32)
    rop = torch.full((total,), -1, dtype=torch.int32)
    rop[por.long()] = torch.arange(count, dtype=torch.int32)
    rows = torch.zeros((total, npad), dtype=torch.float32)
    for r in range(count):
        for a in set(torch.randint(0, n, (2,), generator=g).tolist()):
            c0, c1 = torch.randperm(C - 1, generator=g)[:2].tolist() if C > 2 else (0, 0)
            if int(torch.randint(0, 2, (1,), generator=g)):                       # a positive: offsets, label and maximum
                for j in torch.randperm(4, generator=g)[:2].tolist():
                    rows[r, a * 4 + j] = 2.0 ** -6 * (1 if int(torch.randint(0, 2, (1,), generator=g)) else -1)
                rows[r, n * 4 + a * C + c0] = -2.0 ** -6
                rows[r, n * 4 + a * C + (c1 if c1 != c0 else C - 1)] = 2.0 ** -6
            else:                                                                  # a mined negative: maximum and background
                rows[r, n * 4 + a * C + c0] = 2.0 ** -8
                rows[r, n * 4 + a * C + C - 1] = -2.0 ** -8
    dense = torch.zeros((total, npad), dtype=torch.float32)
    dense[por.long()] = rows[:count]
    rows[count:] = UNREAD
    por_full = torch.zeros((total,), dtype=torch.int32)
    por_full[:count] = por
    return dict(rows=rows.to(torch.bfloat16), pixel_of_row=por_full, row_of_pixel=rop, count=count, dense=dense.view(B, H, W, npad))


def head_bwd_reference(x, w, dy):
    """fp32 gradients of y = conv3x3_same(x, w) + b for dL/dy = dy on the CPU (torch autograd), NHWC / [cout,3,3,Cin]"""
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.permute(0, 3, 1, 2).clone().requires_grad_(True)
    br = torch.zeros(w.shape[0], dtype=w.dtype, requires_grad=True)
    F.conv2d(xr, wr, br, padding=1).backward(dy.permute(0, 3, 1, 2))
    return xr.grad.permute(0, 2, 3, 1).contiguous(), wr.grad.permute(0, 2, 3, 1).contiguous(), br.grad


def sparse_level(g, B, H, W, Cin, cout, npad, dense, relu):
    """operands and references of one head level for dL/dy = dense[..., :cout]: x in {-2..2} (clamped at 0 where a ReLU mask is
    derived from it), filters in {-1, 0, 1} thinned until the fp32 data gradient is bf16-exact"""
    x = ints(g, (B, H, W, Cin), (-2, -1, 0, 1, 2))
    if relu != "none":
        x = x.clamp_min(0)
    dy = dense[..., :cout].contiguous()
    density = 0.5
    while True:
        w = ints(g, (cout, 3, 3, Cin), (-1, 1), density)
        dx, dw, db = head_bwd_reference(x.float(), w.float(), dy)
        if in_bf16_regime(dx):
            break
        density /= 2
        assert density > 1e-3
    if relu != "none":
        dx = masked(dx, x.float() > 0)
    w_tap = torch.zeros((3, 3, Cin, npad), dtype=torch.bfloat16)
    w_tap[..., :cout] = w.permute(1, 2, 3, 0)
    units = dy.abs()[dy != 0].min() if bool((dy != 0).any()) else torch.tensor(1.0)
    return dict(H=H, W=W, Cin=Cin, cout=cout, npad=npad, x=x, w=w, w_tap=w_tap, bits=pack_bits(x.float() > 0), dx=dx, dw=dw, dbias=db,
                density=density, fp32=((B * H * W, x, dy / units),))


# name -> (B, relu, [(H, W, Cin, per_cell, classes, npad, rows)]); cout = per_cell * (4 + classes) = 36, 340, 510
SPARSE_CASES = {
    # B * hw = 361, 35, 35, 9, 1: no multiple of k_hz_col2im's four pixels; one row more than k_hz_gemm's tile; every pixel of a
    # non-square map; one row; none
    "B=1 bits": (1, "bits", [(19, 19, 128, 4, 81, 344, 129), (7, 5, 256, 6, 81, 512, 35), (5, 7, 128, 4, 5, 48, 1),
                             (3, 3, 256, 4, 5, 40, 0), (1, 1, 128, 4, 81, 344, 1)]),
    "B=1 src": (1, "src", [(19, 19, 128, 4, 81, 344, 129), (7, 5, 256, 6, 81, 512, 35), (5, 7, 128, 4, 5, 48, 1),
                           (3, 3, 256, 4, 5, 40, 0), (1, 1, 128, 4, 81, 344, 1)]),
    # exactly one tile of rows, one row fewer, and a map with every pixel selected
    "B=3 none": (3, "none", [(16, 8, 128, 4, 81, 344, 128), (8, 16, 256, 4, 5, 40, 127), (3, 3, 128, 6, 81, 512, 27)]),
    # 1444 rows: two active pixel splits of the weight gradient; 768 rows on the same shape: one
    "B=4 splits": (4, "bits", [(19, 19, 128, 4, 81, 344, 1444), (19, 19, 128, 4, 81, 344, 768)]),
}


def sparse_case(name):
    B, relu, levels = SPARSE_CASES[name]
    g = _gen(B, len(levels), len(relu))
    out = []
    for H, W, Cin, n, C, npad, count in levels:
        hg = hand_rows(g, B, H, W, n, C, npad, count)
        lv = sparse_level(g, B, H, W, Cin, n * (4 + C), npad, hg["dense"], relu)
        lv.update(hw=H * W, n=n, **{k: hg[k] for k in ("rows", "pixel_of_row", "row_of_pixel", "count")})
        out.append(lv)
    return dict(B=B, relu=relu, levels=out)


def sparse_cached(name):
    if ("sparse", name) not in _LOSS_CACHE:
        _LOSS_CACHE[("sparse", name)] = sparse_case(name)
    return _LOSS_CACHE[("sparse", name)]


def chained_case(name="7 levels B=3 C=81", Cin=128):
    """an exact loss case in the compact-row form and, per level, the operands and references of the head convolutions' backward
    pass for the gradient that loss produces"""
    if ("chained", name) not in _LOSS_CACHE:
        r = heads_cached(name)
        g = _gen(r["B"], r["A"], 9)
        lv = [sparse_level(g, r["B"], l["H"], l["W"], Cin, l["n"] * (4 + r["C"]), l["npad"], l["dense"].float(), "bits") for l in r["levels"]]
        _LOSS_CACHE[("chained", name)] = dict(loss=r, levels=lv)
    return _LOSS_CACHE[("chained", name)]


def check_sparse_regime(levels):
    for lv in levels:
        assert in_bf16_regime(lv["dx"]), "dx"
        for k_total, a, b in lv["fp32"]:
            assert in_fp32_regime(k_total, a, b)
