"""The inputs and expectations of the quantising poolings' strict tests (tests/test_pool_mxfp8_strict_gpu.py) and of their tiled
form beyond one grid sweep (tests/sweep_cases.py).  Plain Python: importable without a GPU.

Inputs are small integers times a power of two PER 32-CHANNEL BLOCK AND PIXEL (exponents over -20 .. 20, as
strict.mx_eltwise_case), so the pixels of one window have different block scales.  Expectation: strict.ref_quantize_mx of
strict.ref_pool's map (a pooled value is one of the inputs: exact in bf16)."""
import functools

import torch

from tests import strict

BF = torch.bfloat16


def pooled_shape(shape, ksize, same):
    B, H, W, C = shape
    if ksize == 3:
        return B, H, W, C
    return (B, (H + 1) // 2, (W + 1) // 2, C) if same else (B, H // 2, W // 2, C)


def ref(x, ksize, same):
    """strict.ref_pool's map of x (bf16) by the stated conventions, back in bf16 exactly"""
    _, Ho, Wo, _ = pooled_shape(x.shape, ksize, same)
    y, _ = strict.ref_pool(x.float(), 3, 1, 1, 1, Ho, Wo, 15) if ksize == 3 else strict.ref_pool(x.float(), 2, 2, 0, 0, Ho, Wo, 4)
    out = y.to(BF)
    assert torch.equal(out.float(), y)
    return out


@functools.lru_cache(maxsize=None)
def case(shape, ksize, same):
    g = strict._gen(*shape, ksize, 41)
    x_int = strict.ints(g, shape, (-2, -1, 0, 0, 1, 1, 2, 3))
    x_int[:, ::3, ::4] = strict.ints(g, x_int[:, ::3, ::4].shape, (-3, -1, 0))       # windows whose maximum is <= 0
    e = torch.randint(-20, 21, tuple(shape[:-1]) + (shape[-1] // 32,), generator=g)
    x = strict._pow2_blocks(x_int, e)
    y = ref(x, ksize, same)
    q, s = strict.ref_quantize_mx(y)
    # the regime: pooled values are inputs (exact in bf16).  A pooled block mixes the scales of up to nine pixels, so its small
    # elements round or underflow under its own scale: ref_quantize_mx states those bytes, the quantiser's strict tests cover
    # the rounding itself
    assert bool(torch.isfinite(y.float()).all())
    if x.shape[1] * x.shape[2] > 1:
        # the case can tell the pooled block's own scale from the scale of the window's first / centre pixel
        qc, sc_ = strict.ref_quantize_mx(x)
        centre = sc_ if ksize == 3 else sc_[:, ::2, ::2][:, :y.shape[1], :y.shape[2]]
        assert float((centre != s).float().mean()) > 0.3
    return dict(x=x, y=y, q=q, s=s)
