"""Test-side oracle of the L2 normalisation layer (include/ssd_hip.h, ssd_l2norm_*) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Three forms of the same mathematics, per pixel p over C channels:
    r_p = 1 / sqrt(sum_k x_pk^2 + eps)     xh_pc = x_pc r_p     y_pc = s_c xh_pc
    t_pc = s_c dy_pc     D_p = sum_k t_pk xh_pk     dx_pc = r_p (t_pc - xh_pc D_p) [+ old_pc]     ds_c = sum_p dy_pc xh_pc
- fwd64 / bwd64: float64 numpy, nothing rounded -- the reference of every bound below;
- fwd32 / bwd32: float32 numpy with bf16-rounded outputs, sums strictly sequential or in numpy's pairwise order: shows that
  the bounds admit any correct fp32 kernel (tests/test_l2norm_cpu.py);
- forward_torch: oracle.net_oracle.forward's walk with the layer, as autograd operations, between feature map 0 and its head.

The bounds are derived, not measured.  ulp(v) = 2^(floor(log2 |v|) - 7) is one bf16 ulp, u = 2^-24:
    y    |y - y64|   <= ulp(y64)                   (the fp32 error is far below half a bf16 ulp: one of the two neighbours)
    dx   |dx - dx64| <= ulp(dx64) + (C + 16) u r_p (|t_pc| + |xh_pc| sum_k |t_pk xh_pk|)
                                                   (bf16 rounding + an fp32 sum of C products in any order)
         accumulate: + ulp(old + dx64) + |old| u   (the rounding moves to the sum, and the fp32 addition)
    ds   |ds - ds64| <= (P + 16) u sum_p |dy_pc xh_pc|, exactly 0 where that sum is 0
    r    |r - r64|   <= 4 u r64"""
import numpy as np

U = 2.0 ** -24
EPS = 1e-10
SHAPES = [(1, 128), (7, 256), (130, 512), (67, 1024), (2 * 1444, 512)]
# past one sweep of both grids (tests/sweep_cases.py has the arithmetic): three trips of the forward's 8192 waves (13 waves make
# the third) and of the backward's 6144, whose 1536 workgroups write every row of partials; one and two vectors per lane
EXTRA_SHAPES = [(16397, 128), (16397, 1024)]


def bf16_round(a):
    """float32 array rounded to the nearest bf16 (ties to even), as float32"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    b = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return b.view(np.float32)


def ulp_bf16(v):
    v = np.abs(np.asarray(v, np.float64))
    out = np.zeros_like(v)
    nz = v > 0
    out[nz] = 2.0 ** (np.floor(np.log2(v[nz])) - 7)
    return out


def make_case(P, C, seed=0):
    """Inputs as the layer sees them behind a ReLU convolution and in front of a head: x post-ReLU (about half of each pixel's
    channels zero) with per-pixel magnitudes over 0.01 .. 30 and one all-zero pixel (where P > 1), s ~ N(20, 5) with one
    negative entry, dy ~ 1e-3 with half its entries zero, old ~ 1e-2: x, dy, old bf16 values held in float32, s float32."""
    g = np.random.default_rng(1000 * seed + 7 * P + C)
    mag = 10.0 ** g.uniform(np.log10(0.01), np.log10(30.0), (P, 1))
    x = np.maximum(g.standard_normal((P, C)), 0.0) * mag
    if P > 1:
        x[P // 2] = 0.0
    s = (20.0 + 5.0 * g.standard_normal(C)).astype(np.float32)
    s[3] = -abs(s[3])
    dy = g.standard_normal((P, C)) * 1e-3 * (g.random((P, C)) < 0.5)
    old = g.standard_normal((P, C)) * 1e-2
    x, dy, old = (bf16_round(v.astype(np.float32)) for v in (x, dy, old))
    tiny = 2.0 ** -126
    for v in (x, dy, old):
        assert not ((v != 0) & (np.abs(v) < tiny)).any()               # bf16's normal range
    return dict(P=P, C=C, x=x, s=s, dy=dy, old=old)


# ---- float64 -----------------------------------------------------------------------------------------------------------
def fwd64(x, s, eps=EPS):
    """-> (y [P,C], r [P], xh [P,C]) in float64"""
    x, s = np.asarray(x, np.float64), np.asarray(s, np.float64)
    r = 1.0 / np.sqrt((x * x).sum(1) + eps)
    xh = x * r[:, None]
    return s[None, :] * xh, r, xh


def bwd64(dy, x, s, eps=EPS, old=None):
    """-> (dx [P,C] (+ old), ds [C]) in float64"""
    dy, s = np.asarray(dy, np.float64), np.asarray(s, np.float64)
    _, r, xh = fwd64(x, s, eps)
    t = s[None, :] * dy
    D = (t * xh).sum(1)
    dx = r[:, None] * (t - xh * D[:, None])
    if old is not None:
        dx = dx + np.asarray(old, np.float64)
    return dx, (dy * xh).sum(0)


def bounds(dy, x, s, eps=EPS, old=None):
    """-> dict(y, dx, ds, r): the element-wise error bounds of the module docstring, from float64 quantities only"""
    dy64, s64 = np.asarray(dy, np.float64), np.asarray(s, np.float64)
    P, C = dy64.shape
    y, r, xh = fwd64(x, s, eps)
    t = s64[None, :] * dy64
    dx, _ = bwd64(dy, x, s, eps)
    sum_abs = np.abs(t * xh).sum(1)
    b_dx = ulp_bf16(dx) + (C + 16) * U * r[:, None] * (np.abs(t) + np.abs(xh) * sum_abs[:, None])
    if old is not None:
        old64 = np.asarray(old, np.float64)
        b_dx = b_dx + ulp_bf16(old64 + dx) + np.abs(old64) * U
    return dict(y=ulp_bf16(y), dx=b_dx, ds=(P + 16) * U * np.abs(dy64 * xh).sum(0), r=4 * U * r)


def worst(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0, x / 0 as inf): <= 1 passes"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max())


# ---- float32 restatement -----------------------------------------------------------------------------------------------
def _sum32(a, axis, order):
    a = np.asarray(a, np.float32)
    if order == "pairwise":
        return np.add.reduce(np.ascontiguousarray(np.moveaxis(a, axis, -1)), axis=-1, dtype=np.float32)
    acc = np.zeros(np.delete(a.shape, axis), np.float32)
    for k in range(a.shape[axis]):                                     # strictly sequential: the worst order
        acc = acc + np.take(a, k, axis)
    return acc


def fwd32(x, s, eps=EPS, order="sequential"):
    """-> (y bf16-rounded, r, xh) with every operation in float32"""
    x, s = np.asarray(x, np.float32), np.asarray(s, np.float32)
    r = np.float32(1.0) / np.sqrt(_sum32(x * x, 1, order) + np.float32(eps))
    xh = x * r[:, None]
    return bf16_round(s[None, :] * xh), r, xh


def bwd32(dy, x, s, eps=EPS, old=None, order="sequential"):
    dy, s = np.asarray(dy, np.float32), np.asarray(s, np.float32)
    _, r, xh = fwd32(x, s, eps, order)
    t = s[None, :] * dy
    D = _sum32(t * xh, 1, order)
    dx = r[:, None] * (t - xh * D[:, None])
    if old is not None:
        dx = dx + np.asarray(old, np.float32)
    return bf16_round(dx), _sum32(dy * xh, 0, order)


# ---- the network with the layer ------------------------------------------------------------------------------------------
def forward_torch(trunk, num_priors, classes, params, image_nhwc, scale, eps=EPS):
    """oracle.net_oracle.forward (emulate_bf16=True) with y = bf16(scale_c f / sqrt(sum_k f_k^2 + eps)) between feature map 0
    and its head; scale: tensor [C] (a leaf that wants a gradient gets one).  Returns (loc, conf)."""
    import torch
    import torch.nn.functional as F
    from oracle.net_oracle import _RoundBF16, conv_tf
    rnd = _RoundBF16.apply
    x = image_nhwc.permute(0, 3, 1, 2)
    feats = []
    for i, (kind, cin, cout, k, stride, mode, feat) in enumerate(trunk):
        if kind == "conv":
            x = rnd(conv_tf(x, params["conv%d/kernel" % i], params["conv%d/bias" % i], k, stride, mode == "same", True))
        else:
            if mode == "same" and x.shape[2] % 2:
                x = F.pad(x, (0, 1, 0, 1), value=float("-inf"))
            x = F.max_pool2d(x, 2, 2)
        if feat:
            feats.append(x)
    f = feats[0]
    feats[0] = rnd(scale.view(1, -1, 1, 1) * (f * torch.rsqrt((f * f).sum(1, keepdim=True) + eps)))
    locs, confs = [], []
    B = x.shape[0]
    for lvl, (f, n) in enumerate(zip(feats, num_priors)):
        y = conv_tf(f, params["head%d/kernel" % lvl], params["head%d/bias" % lvl], 3, 1, True, False)
        y = rnd(y).permute(0, 2, 3, 1)
        locs.append(y[..., :n * 4].reshape(B, -1, 4))
        confs.append(y[..., n * 4:].reshape(B, -1, classes))
    return torch.cat(locs, 1), torch.cat(confs, 1)
