"""Oracle of the depthwise 3x3 convolution (ssd_dwconv3x3_*): plain helpers, importable without a GPU.  Semantics: Keras
DepthwiseConv2D(3, strides=s, depth_multiplier=1) + bias (+ ReLU) and its tape.gradient, stated with torch on the CPU as
F.conv2d(groups=C) on an explicitly padded map (as strict.ref_conv pads).  Operands of the exact cases are small integers
(strict.ints): x and dy in {-2,-1,1,2}, w in {-1,0,1}, bias in -3..3, so |y| <= 9*2 + 3 = 21 and |dx + base| <= 9*2 + 2 = 20, both
exact in bf16, and every dw / dbias sum is at most 4 P, far below 2^24: every expected tensor is exact and every comparison is
torch.equal."""
import functools

import torch
import torch.nn.functional as F

from tests import strict

# (B, H, W, C, stride, padding): what each can catch is in tests/test_depthwise_strict_gpu.py.  padding "same" is TF SAME;
# "pad1" is torch's padding=1: pad_t = pad_l = 1, Ho = (H - 1) // stride + 1.
CASES = [
    (1, 1, 1, 8, 1, "same"),
    (1, 2, 9, 8, 1, "same"),
    (2, 5, 7, 24, 1, "same"),
    (3, 19, 19, 64, 1, "same"),
    (1, 4, 6, 520, 1, "same"),
    (2, 10, 10, 40, 2, "same"),
    (2, 19, 19, 72, 2, "same"),
    (2, 10, 10, 40, 2, "pad1"),
    (4, 38, 38, 32, 1, "same"),
    (2, 75, 75, 32, 2, "same"),
    # weight-gradient slabs: C = 64 is 8 channel groups, so a workgroup walks 32 column strips side by side, one each (the shape
    # is far too small for more): a slab is 32 strips.  11 rows are 3 strips of 4 rows, so 3 * 3 * 13 = 117 strips (429 pixels) =
    # slabs of 32, 32, 32 and 21: four slabs, the last one partial.
    (3, 11, 13, 64, 1, "same"),
]
REALISTIC = [(2, 19, 19, 136, 1, "same"), (2, 19, 19, 136, 2, "same")]
SEPARABLE = [(2, 10, 10, 64, 64, 1), (2, 10, 10, 64, 64, 2)]


def geometry(H, W, stride, padding):
    """(Ho, Wo, pad_t, pad_l)"""
    if padding == "same":
        return strict.geometry(H, W, 3, stride, "same")
    assert padding == "pad1"
    return (H - 1) // stride + 1, (W - 1) // stride + 1, 1, 1


def ref_dwconv(x, w, bias, stride, pad_t, pad_l, Ho, Wo, relu, dtype=torch.float32):
    """x [B,H,W,C], w [3,3,C], bias [C] or None -> [B,Ho,Wo,C] in `dtype`; what lies outside the map reads as zero."""
    B, H, W, C = x.shape
    pad_b, pad_r = (Ho - 1) * stride + 3 - H - pad_t, (Wo - 1) * stride + 3 - W - pad_l
    assert 0 <= pad_b <= 2 and 0 <= pad_r <= 2 and pad_t in (0, 1) and pad_l in (0, 1)
    xn = F.pad(x.to(dtype).permute(0, 3, 1, 2), (pad_l, pad_r, pad_t, pad_b))
    y = F.conv2d(xn, w.to(dtype).permute(2, 0, 1).unsqueeze(1), None if bias is None else bias.to(dtype), stride=stride, groups=C)
    assert y.shape[2] == Ho and y.shape[3] == Wo
    if relu:
        y = y.relu()
    return y.permute(0, 2, 3, 1).contiguous()


def dw_grads(x, w, bias, dy, stride, pad_t, pad_l, dtype):
    """(y, dx, dw, dbias) of ref_dwconv by autograd, all in `dtype`; dw in w's layout [3,3,C]."""
    xr = x.to(dtype).requires_grad_(True)
    wr = w.to(dtype).requires_grad_(True)
    br = bias.to(dtype).requires_grad_(True)
    y = ref_dwconv(xr, wr, br, stride, pad_t, pad_l, dy.shape[1], dy.shape[2], False, dtype)
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, wr.grad, br.grad


def nine_tap_loop(x, w, bias, stride, pad_t, pad_l, Ho, Wo):
    """The forward pass restated without F.conv2d: nine shifted, strided slices of the zero-padded map, in tap order."""
    B, H, W, C = x.shape
    xp = torch.zeros((B, (Ho - 1) * stride + 3, (Wo - 1) * stride + 3, C))
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x.float()
    y = bias.float().expand(B, Ho, Wo, C).clone()
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride] * w[ky, kx].float()
    return y


def gather_loop(dy, w, x_shape, stride, pad_t, pad_l):
    """The data gradient restated as the header states it: per input pixel, the taps whose output coordinate is integral and in
    range."""
    B, H, W, C = x_shape
    _, Ho, Wo, _ = dy.shape
    dx = torch.zeros(x_shape)
    for iy in range(H):
        for ix in range(W):
            for ky in range(3):
                for kx in range(3):
                    ty, tx = iy + pad_t - ky, ix + pad_l - kx
                    if ty < 0 or tx < 0 or ty % stride or tx % stride or ty // stride >= Ho or tx // stride >= Wo:
                        continue
                    dx[:, iy, ix] += dy[:, ty // stride, tx // stride].float() * w[ky, kx].float()
    return dx


@functools.lru_cache(maxsize=None)
def dw_case(case, dtype=torch.float32):
    """Every expected tensor of a (B, H, W, C, stride, padding) case, with the regime lists bf16= / fp32= of strict.check_regime.
    Cached: the tests share one reference and leave it unchanged."""
    B, H, W, C, stride, padding = case
    Ho, Wo, pt, pl = geometry(H, W, stride, padding)
    g = strict._gen(B, H, W, C, stride, len(padding), 7)
    o = dict(geom=(Ho, Wo, pt, pl))
    o["x"] = strict.ints(g, (B, H, W, C), (-2, -1, 1, 2))
    o["w"] = strict.ints(g, (3, 3, C), (-1, 0, 1))
    o["dy"] = strict.ints(g, (B, Ho, Wo, C), (-2, -1, 1, 2))
    o["bias"] = strict.ints(g, (C,), (-3, -2, -1, 0, 1, 2, 3), dtype=torch.float32)
    o["mask_src"] = strict.ints(g, (B, H, W, C), (-1, 0, 0, 1, 2))
    o["base"] = strict.ints(g, (B, H, W, C), (-2, -1, 0, 1, 2))
    y, dx, dw, dbias = dw_grads(o["x"], o["w"], o["bias"], o["dy"], stride, pt, pl, dtype)
    keep = o["mask_src"].to(dtype) > 0
    o.update(y=y, y_relu=y.relu(), dx=dx, dx_masked=strict.masked(dx, keep), dx_acc=strict.masked(dx + o["base"].to(dtype), keep),
             dw=dw, dbias=dbias)
    o["bf16"] = ("y", "y_relu", "dx", "dx_masked", "dx_acc")
    P = B * Ho * Wo
    o["fp32"] = [(P, o["x"], o["dy"]), (P, o["dy"], torch.ones(1)), (9, o["x"], o["w"]), (9, o["dy"], o["w"])]
    return o


@functools.lru_cache(maxsize=None)
def realistic_case(case):
    """x = relu(randn), w = randn sqrt(2 / 9), dy = randn, all rounded to bf16 first; the float64 oracle OF THOSE bf16 operands
    and the derived bounds.  The products of two bf16 numbers are exact in fp32 and the vector unit's fp32 additions round to
    nearest: half an ulp, 2^-24 relative, per operation, at most 10 of them per element (nine taps and the bias; the data
    gradient has nine and no bias).  From the oracle run on absolute values:
      y, y_relu: |y - y64| <= E + 2^-8 (|y64| + E), E = 10 2^-24 (sum |x||w| + |bias|)   (the ReLU is 1-Lipschitz)
      dx:        the same form with E = 10 2^-24 sum |dy||w|
      dw, dbias: (P + 16) 2^-24 of their absolute sums, P = B Ho Wo, the form batchnorm_oracle and l2norm_oracle use"""
    B, H, W, C, stride, padding = case
    Ho, Wo, pt, pl = geometry(H, W, stride, padding)
    g = torch.Generator().manual_seed(20161 + stride)
    f64, bf = torch.float64, torch.bfloat16
    x = torch.randn((B, H, W, C), generator=g).relu().to(bf)
    w = (torch.randn((3, 3, C), generator=g) * (2.0 / 9) ** 0.5).to(bf)
    dy = torch.randn((B, Ho, Wo, C), generator=g).to(bf)
    bias = torch.randn((C,), generator=g) * 0.1
    y, dx, dw, dbias = dw_grads(x, w, bias, dy, stride, pt, pl, f64)
    ya, dxa, dwa, dba = dw_grads(x.abs(), w.abs(), bias.abs(), dy.abs(), stride, pt, pl, f64)
    u, P = 2.0 ** -8, B * Ho * Wo
    Ey, Ex = 10 * 2.0 ** -24 * ya, 10 * 2.0 ** -24 * dxa
    return dict(x=x, w=w, dy=dy, bias=bias, geom=(Ho, Wo, pt, pl), y=y, y_relu=y.relu(), dx=dx, dw=dw, dbias=dbias,
                y_bound=Ey + u * (y.abs() + Ey), dx_bound=Ex + u * (dx.abs() + Ex),
                dw_bound=(P + 16) * 2.0 ** -24 * dwa, dbias_bound=(P + 16) * 2.0 ** -24 * dba)


@functools.lru_cache(maxsize=None)
def separable_case(case):
    """A separable block, y1 = relu(depthwise(x)), y2 = pointwise(y1), and torch autograd's gradients of it, kept exact by
    construction: the pointwise filters have at most 8 non-zeros (+-1) per output channel, so |y2| <= 8 * 21 + 3 = 171; dy2 has at
    most 2 non-zero channels per pixel, so the gradient that enters the depthwise layer is at most 2 * 2 = 4 and |dx| <= 36."""
    B, H, W, C, N, stride = case
    Ho, Wo, pt, pl = geometry(H, W, stride, "same")
    g = strict._gen(B, H, W, C, N, stride, 11)
    x = strict.ints(g, (B, H, W, C), (-2, -1, 1, 2))
    w1 = strict.ints(g, (3, 3, C), (-1, 0, 1))
    b1 = strict.ints(g, (C,), (-3, -2, -1, 0, 1, 2, 3), dtype=torch.float32)
    w2 = torch.zeros((N, 1, 1, C))
    for n in range(N):
        idx = torch.randperm(C, generator=g)[:8]
        w2[n, 0, 0, idx] = strict.ints(g, (8,), (-1, 1)).float()
    w2 = w2.to(torch.bfloat16)
    b2 = strict.ints(g, (N,), (-3, -2, -1, 0, 1, 2, 3), dtype=torch.float32)
    dy2 = torch.zeros((B, Ho, Wo, N))
    for _ in range(2):
        ch = torch.randint(0, N, (B, Ho, Wo, 1), generator=g)
        dy2.scatter_(3, ch, strict.ints(g, (B, Ho, Wo, 1), (-2, -1, 1, 2)).float())
    dy2 = dy2.to(torch.bfloat16)
    xr, w1r, b1r = x.float().requires_grad_(True), w1.float().requires_grad_(True), b1.clone().requires_grad_(True)
    y1 = ref_dwconv(xr, w1r, b1r, stride, pt, pl, Ho, Wo, True)
    y1.retain_grad()
    y2 = strict.ref_conv(y1, w2.float(), b2, 1, 1, 0, 0, Ho, Wo, False)
    y2.backward(dy2.float())
    g1 = strict.masked(y1.grad, y1.detach() > 0)                   # what conv2d_bwd_data(relu_src = y1) hands on
    assert float(y2.detach().abs().max()) <= 171 and float(g1.abs().max()) <= 4 and float(xr.grad.abs().max()) <= 36
    assert int((dy2 != 0).sum(-1).max()) <= 2 and int((w2 != 0).sum(-1).max()) <= 8
    P = B * Ho * Wo
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dy2=dy2, w2_t=w2.flip(1, 2).permute(3, 1, 2, 0).contiguous(), geom=(Ho, Wo, pt, pl),
                y1=y1.detach(), y2=y2.detach(), g1=g1, dx=xr.grad, dw1=w1r.grad, db1=b1r.grad,
                bf16=("y1", "y2", "g1", "dx"), fp32=[(P, x, g1), (P, g1, torch.ones(1)), (9, x, w1), (9, g1, w1), (C, y1.detach(), w2), (N, dy2, w2)])
