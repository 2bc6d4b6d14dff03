"""Oracle of the atrous 3x3 convolution and the 3x3 / stride-1 max pooling (ssd_conv2d_atrous_*, ssd_maxpool3x3s1_*): plain
helpers, importable without a GPU.  Semantics: Keras Conv2D(3, dilation_rate=d, padding="same"), MaxPooling2D(3, strides=1,
padding="same") and their tape.gradient, stated with torch on the CPU.  Operands of the exact cases are strict.conv_operands':
integers times powers of two, so every expected tensor is exact and every comparison is torch.equal."""
import functools

import torch
import torch.nn.functional as F

from tests import strict

# (B, H, W, Cin, Cout, d): what each can catch is in tests/test_atrous_strict_gpu.py
CASES = [
    (1, 7, 7, 64, 64, 6),
    (2, 5, 5, 64, 64, 1),
    (1, 10, 10, 64, 64, 12),
    (2, 13, 11, 128, 64, 2),
    (3, 19, 19, 64, 72, 6),
    (5, 19, 19, 128, 136, 6),
    (2, 19, 19, 512, 1024, 6),
    (1, 19, 19, 1024, 512, 6),
    (2, 13, 5, 64, 64, 6),          # W <= d < H: the three taps of the centre column are live, the other six dead
]
POOL_CASES = [(2, 19, 19, 64), (3, 5, 7, 24), (1, 2, 9, 8), (1, 1, 1, 8)]
REALISTIC = (2, 19, 19, 128, 136, 6)


def ref_atrous(x, w, bias, d, relu, dtype):
    """x [B,H,W,Cin], w [Cout,3,3,Cin], bias [Cout] or None -> [B,H,W,Cout] in `dtype`: F.conv2d(padding=d, dilation=d)."""
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(0, 3, 1, 2), None if bias is None else bias.to(dtype),
                 padding=d, dilation=d)
    if relu:
        y = y.relu()
    return y.permute(0, 2, 3, 1).contiguous()


def atrous_grads(x, w, bias, dy, d, dtype):
    """(y, dx, dw, dbias) of ref_atrous by autograd, all in `dtype`."""
    xr = x.to(dtype).requires_grad_(True)
    wr = w.to(dtype).requires_grad_(True)
    br = bias.to(dtype).requires_grad_(True)
    y = ref_atrous(xr, wr, br, d, False, dtype)
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, wr.grad, br.grad


def pad_channels(t, cp):
    """[..., C] -> [..., cp] bf16, zero-filled"""
    out = torch.zeros(tuple(t.shape[:-1]) + (cp,), dtype=torch.bfloat16)
    out[..., :t.shape[-1]] = t
    return out


def transposed_filters(w, cp):
    """ssd_weight_transpose, restated: [Cout,3,3,Cin] -> [Cin,3,3,cp], spatially flipped, zero-padded"""
    return pad_channels(w.flip(1, 2).permute(3, 1, 2, 0), cp)


@functools.lru_cache(maxsize=None)
def atrous_case(case, dtype=torch.float32):
    """Every expected tensor of a (B, H, W, Cin, Cout, d) case, as strict.conv_reference builds them, with the regime lists
    bf16= / fp32= of strict.check_regime.  Cached: the tests share one reference and leave it unchanged."""
    B, H, W, Cin, Cout, d = case
    o = dict(strict.conv_operands((B, H, W, Cin, Cout, 3, 1, "same")))
    y, dx, dw, dbias = atrous_grads(o["x"], o["w"], o["bias"], o["dy"], d, dtype)
    keep = o["mask_src"].to(dtype) > 0
    o.update(y=y, y_relu=y.relu(), dx=dx, dx_masked=strict.masked(dx, keep), dx_acc=strict.masked(dx + o["base"].to(dtype), keep),
             dw=dw, dbias=dbias)
    cp = (Cout + 7) // 8 * 8
    o["w_t"] = transposed_filters(o["w"], cp)
    o["dy_pad"] = pad_channels(o["dy"], cp)
    o["bf16"] = ("y", "y_relu", "dx", "dx_masked", "dx_acc")
    P = B * H * W
    o["fp32"] = [(P, o["x"], o["dy"]), (P, o["dy"], torch.ones(1)), (9 * Cin, o["x"], o["w"]), (9 * Cout, o["dy"], o["w"])]
    return o


@functools.lru_cache(maxsize=None)
def pool3x3s1_case(B, H, W, C):
    """strict.pool3x3_case at stride 1, padding 1: exact zeros, ties, windows whose maximum is <= 0.  Up to nine windows meet
    in a pixel: |dx| <= 18."""
    g = strict._gen(B, H, W, C, 31)
    x = strict.ints(g, (B, H, W, C), (-2, -1, 0, 0, 1, 1, 2, 3))
    x[:, ::4, ::3] = strict.ints(g, x[:, ::4, ::3].shape, (-1, 0))
    y, code = strict.ref_pool(x.float(), 3, 1, 1, 1, H, W, 15)
    dy = strict.ints(g, (B, H, W, C), (-2, -1, 1, 2))
    dx = strict.ref_unpool(code, dy.float(), x.shape, 3, 1, 1, 1)
    return dict(x=x, y=y, code=code, dy=dy, dx=dx, bf16=("y", "dx"))


@functools.lru_cache(maxsize=None)
def realistic_case(case=REALISTIC):
    """x = relu(randn), w = randn sqrt(2 / K), dy = randn, all rounded to bf16 first; the float64 oracle OF THOSE bf16 operands
    and the derived bounds.  u = 2^-8 (bf16); the accumulation term is (K + 1) 2^-23 (sum |x||w| + |bias|), elementwise, from the
    oracle run on absolute values -- 2^-23, not 2^-24: the rounding of the matrix unit's internal additions is not documented as
    nearest, so one ulp per addition is what can be derived.
      y, y_relu: |y - y64| <= E + u (|y64| + E), K = 9 Cin (the ReLU is 1-Lipschitz)
      dx:        the same form, K = 9 Cout_pad
      dw:        |dw - dw64| <= (P + 16) 2^-23 sum |x||dy|, P = B H W; dbias likewise"""
    B, H, W, Cin, Cout, d = case
    g = torch.Generator().manual_seed(20161)
    f64, bf = torch.float64, torch.bfloat16
    x = torch.randn((B, H, W, Cin), generator=g).relu().to(bf)
    w = (torch.randn((Cout, 3, 3, Cin), generator=g) * (2.0 / (9 * Cin)) ** 0.5).to(bf)
    dy = torch.randn((B, H, W, Cout), generator=g).to(bf)
    bias = torch.randn((Cout,), generator=g) * 0.1
    y, dx, dw, dbias = atrous_grads(x, w, bias, dy, d, f64)
    ya, dxa, dwa, dba = atrous_grads(x.abs(), w.abs(), bias.abs(), dy.abs(), d, f64)
    cp = (Cout + 7) // 8 * 8
    u, P = 2.0 ** -8, B * H * W
    Ey = (9 * Cin + 1) * 2.0 ** -23 * ya
    Ex = (9 * cp + 1) * 2.0 ** -23 * dxa
    return dict(x=x, w=w, dy=dy, bias=bias, w_t=transposed_filters(w, cp), dy_pad=pad_channels(dy, cp),
                y=y, y_relu=y.relu(), dx=dx, dw=dw, dbias=dbias,
                y_bound=Ey + u * (y.abs() + Ey), dx_bound=Ex + u * (dx.abs() + Ex),
                dw_bound=(P + 16) * 2.0 ** -23 * dwa, dbias_bound=(P + 16) * 2.0 ** -23 * dba)
