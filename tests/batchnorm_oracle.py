"""Test-side oracle of the batch normalisation kernels (include/ssd_hip.h, ssd_bn_*) -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The mathematics, per channel c over the P rows of x [P, C]:
    mu = (1/P) sum_p x_pc     v = (1/P) sum_p (x_pc - mu)^2     rstd = 1 / sqrt(v + eps)     xh = (x - mu) rstd
    y = gamma xh + beta  [max(., 0)]          running_mean' = (1 - m) running_mean + m mu
                                              running_var'  = (1 - m) running_var + m v P / (P - 1)
    inference: a = gamma / sqrt(running_var + eps)     b = beta - running_mean a     y = x a + b  [max(., 0)]
    backward (dy already masked by the layer's ReLU; mean, rstd as the forward pass SAVED them):
    dbeta = sum_p dy     dgamma = sum_p dy xh     dx = gamma rstd (dy - dbeta / P - xh dgamma / P)
- fwd64 / infer64 / bwd64: float64 numpy, nothing rounded -- the reference of every bound below;
- fwd32 / bwd32: float32 numpy with bf16-rounded maps, sums strictly sequential or in numpy's pairwise order, the variance in
  two passes or (variance="naive") as E[x^2] - mu^2: shows that the bounds admit any correct fp32 kernel and refuse the naive
  form (tests/test_batchnorm_cpu.py);
- forward_graph_bn: oracle.net_oracle.forward_graph's walk for the batch-normalised graph, as autograd operations.

The bounds are derived, not measured.  U = 2^-24 is fp32's unit roundoff; ulp(v) = 2^(floor(log2 |v|) - 7) one bf16 ulp; a
sum of n fp32 terms t_i in ANY order errs by at most (n - 1) U sum |t_i| (+ the terms' own roundings: the "+ 16" below).
    mu    |mu - mu64| <= d := (P + 16) U mean_p |x_pc|
    v     |v - v64|   <= bv := 4 (P + 16) U v64 + d^2
          (sum_p (x - mu')^2 = P v64 + P (mu' - mu64)^2 exactly: a mean that is off by <= d adds <= d^2; the sum of the squares,
          each with three roundings, errs by <= (P + 16) U sum (x - mu')^2; 4 covers both and Chan-merged partials, whose every
          merge adds a few U relative to quantities that are themselves <= P v)
    rstd  relative error <= rho := max(sqrt((v64 + eps) / (max(v64 - bv, 0) + eps)) - 1, 1 - sqrt((v64 + eps) / (v64 + bv + eps))) + 3 U
          (the exact effect on 1 / sqrt of a variance in [max(v64 - bv, 0), v64 + bv] -- a sum of squares is never negative --
          plus the add, the root and the divide)
    y     |y - y64| <= ulp(y64) + (1 + 2^-8) s_y,   s_y = |gamma| rstd64 (1 + rho) d + |gamma xh64| rho
                                                            + 4 U (|gamma| (|xh64| + rstd64 d) (1 + rho) + |beta|)
          (z = the fp32 value before the bf16 rounding differs from y64 by <= s_y: the mean's error times gamma rstd, the
          rstd's relative error times gamma xh, four roundings on the magnitudes of the summands; then ONE bf16 rounding of
          z, <= 2^-8 |z| <= ulp(y64) + 2^-8 s_y.  max(., 0) is 1-Lipschitz: the same bound after the ReLU)
    running_mean'  <= m d + 3 U (|(1 - m) running_mean| + |m mu64|);   running_var' likewise with bv P / (P - 1)
    inference y    <= ulp(y64) + (1 + 2^-8) 6 U (|x a| + |running_mean a| + |beta|)    (a: three roundings; products, fma)
    dbeta   |dbeta - dbeta64|   <= eb := (P + 16) U sum_p |dy|
    dgamma  |dgamma - dgamma64| <= eg := (P + 16) U sum_p |dy xh|       (exactly 0 where that sum is 0: the all-zero channel)
    dx      |dx - dx64| <= ulp(dx64) + (1 + 2^-8) s_dx,
            s_dx = |gamma rstd| (eb / P + |xh| eg / P + 6 U (|dy| + |dbeta64| / P + |xh dgamma64| / P))
The backward bounds take mean and rstd as GIVEN (float32 numbers, the forward pass's own output, exact in float64): the
backward pass is tested on what the forward pass saved, the forward pass's statistics against their own bounds above."""
import numpy as np

U = 2.0 ** -24
EPS = 1e-5
MOMENTUM = 0.1
# (2, 64) one partial chunk; (3, 128) odd rows; (65, 64) three slabs, the last one one row; (130, 1024) two rows per pass, one
# channel per finalize lane and four channels per workgroup-merge thread; (1007, 192) a width that does not divide the workgroup
# (idle lanes) and slabs of unequal chunk counts; (4099, 64) 129 slabs, the last of three rows; (8192, 256) several passes per slab
SHAPES = [(2, 64), (3, 128), (65, 64), (130, 1024), (1007, 192), (4099, 64), (8192, 256)]
# past the cap of 1024 slabs: the first slabs take two chunks (kernel tests only).  Past one sweep of the apply grid as well
# (tests/sweep_cases.py has the arithmetic): (65703, 64) 2054 chunks on 1024 slabs, slabs 0..5 take a third chunk, the 7-row last
# chunk is slab 5's third, six workgroups of the 2048 apply workgroups make a second trip; (2085, 2048) one row per chunk, 66 slabs
# of 31 or 32 chunks, 37 apply workgroups make a second trip
EXTRA_SHAPES = [(33000, 64), (65703, 64), (2085, 2048)]
KINDS = ("unit", "offset64", "offset-300", "small", "constant", "zero")


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


def kind_of(c):
    return KINDS[c % len(KINDS)]


def make_case(P, C, seed=0):
    """x [P, C] with channel c of kind KINDS[c % 6]: N(0, 1); N(64, 0.5); N(-300, 2); N(0, 2^-6); the constant 3.5; zero.
    gamma ~ N(1, 0.25) with one negative entry, beta ~ N(0, 0.5); dy ~ 1e-3 with half its entries zero (masked by a ReLU);
    running_mean ~ N(0, 1), running_var ~ U(0.5, 1.5).  x, dy: bf16 values held in float32; the rest float32."""
    g = np.random.default_rng(1000 * seed + 7 * P + C)
    x = g.standard_normal((P, C))
    for c in range(C):
        k = kind_of(c)
        if k == "offset64":
            x[:, c] = 64.0 + 0.5 * x[:, c]
        elif k == "offset-300":
            x[:, c] = -300.0 + 2.0 * x[:, c]
        elif k == "small":
            x[:, c] *= 2.0 ** -6
        elif k == "constant":
            x[:, c] = 3.5
        elif k == "zero":
            x[:, c] = 0.0
    gamma = (1.0 + 0.25 * g.standard_normal(C)).astype(np.float32)
    gamma[3] = -abs(gamma[3])
    beta = (0.5 * g.standard_normal(C)).astype(np.float32)
    dy = g.standard_normal((P, C)) * 1e-3 * (g.random((P, C)) < 0.5)
    rm = g.standard_normal(C).astype(np.float32)
    rv = g.uniform(0.5, 1.5, C).astype(np.float32)
    x, dy = bf16_round(x.astype(np.float32)), bf16_round(dy.astype(np.float32))
    return dict(P=P, C=C, x=x, gamma=gamma, beta=beta, dy=dy, rm=rm, rv=rv)


# ---- float64 -----------------------------------------------------------------------------------------------------------
def fwd64(x, gamma, beta, eps=EPS, relu=False, running=None, momentum=MOMENTUM):
    """-> dict(y, mean, var (biased), rstd, xh[, rm, rv: the updated running statistics]) in float64"""
    x, gamma, beta = (np.asarray(v, np.float64) for v in (x, gamma, beta))
    P = x.shape[0]
    mu = x.mean(0)
    v = ((x - mu) ** 2).mean(0)
    rstd = 1.0 / np.sqrt(v + eps)
    xh = (x - mu) * rstd
    y = gamma * xh + beta
    out = dict(y=np.maximum(y, 0.0) if relu else y, mean=mu, var=v, rstd=rstd, xh=xh)
    if running is not None:
        rm, rv = (np.asarray(t, np.float64) for t in running)
        out["rm"] = (1.0 - momentum) * rm + momentum * mu
        out["rv"] = (1.0 - momentum) * rv + momentum * v * P / (P - 1)
    return out


def infer64(x, gamma, beta, rm, rv, eps=EPS, relu=False):
    x, gamma, beta, rm, rv = (np.asarray(v, np.float64) for v in (x, gamma, beta, rm, rv))
    a = gamma / np.sqrt(rv + eps)
    y = x * a + (beta - rm * a)
    return np.maximum(y, 0.0) if relu else y


def bwd64(dy, x, gamma, mean, rstd):
    """-> (dx [P, C], dgamma [C], dbeta [C]) in float64, from the mean / rstd given (what a forward pass saved)"""
    dy, x, gamma, mean, rstd = (np.asarray(v, np.float64) for v in (dy, x, gamma, mean, rstd))
    P = x.shape[0]
    xh = (x - mean) * rstd
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    return gamma * rstd * (dy - dbeta / P - xh * dgamma / P), dgamma, dbeta


def fwd_bounds(x, gamma, beta, eps=EPS, running=None, momentum=MOMENTUM):
    """-> dict(mean, var, rstd, y[, rm, rv]): the element-wise bounds of the module docstring, from float64 quantities only"""
    x64, g64, b64 = (np.asarray(v, np.float64) for v in (x, gamma, beta))
    P = x64.shape[0]
    r = fwd64(x, gamma, beta, eps)
    d = (P + 16) * U * np.abs(x64).mean(0)
    bv = 4 * (P + 16) * U * r["var"] + d * d
    ve = r["var"] + eps
    rho = np.maximum(np.sqrt(ve / (np.maximum(r["var"] - bv, 0.0) + eps)) - 1.0, 1.0 - np.sqrt(ve / (ve + bv))) + 3 * U
    axh = np.abs(r["xh"])
    s_y = (np.abs(g64) * r["rstd"] * (1 + rho) * d + np.abs(g64) * axh * rho
           + 4 * U * (np.abs(g64) * (axh + r["rstd"] * d) * (1 + rho) + np.abs(b64)))
    out = dict(mean=d, var=bv, rstd=rho * r["rstd"], y=ulp_bf16(r["y"]) + (1 + 2.0 ** -8) * s_y)
    if running is not None:
        rm, rv = (np.asarray(t, np.float64) for t in running)
        out["rm"] = momentum * d + 3 * U * (np.abs((1 - momentum) * rm) + np.abs(momentum * r["mean"]))
        out["rv"] = momentum * bv * P / (P - 1) + 3 * U * (np.abs((1 - momentum) * rv) + momentum * r["var"] * P / (P - 1))
    return out


def infer_bound(x, gamma, beta, rm, rv, eps=EPS):
    x, gamma, beta, rm, rv = (np.asarray(v, np.float64) for v in (x, gamma, beta, rm, rv))
    a = gamma / np.sqrt(rv + eps)
    y = x * a + (beta - rm * a)
    return ulp_bf16(y) + (1 + 2.0 ** -8) * 6 * U * (np.abs(x * a) + np.abs(rm * a) + np.abs(beta))


def bwd_bounds(dy, x, gamma, mean, rstd):
    """-> dict(dx, dgamma, dbeta)"""
    dy64, x64, g64, mean, rstd = (np.asarray(v, np.float64) for v in (dy, x, gamma, mean, rstd))
    P = x64.shape[0]
    xh = (x64 - mean) * rstd
    dx, dgamma, dbeta = bwd64(dy, x, gamma, mean, rstd)
    eb = (P + 16) * U * np.abs(dy64).sum(0)
    eg = (P + 16) * U * np.abs(dy64 * xh).sum(0)
    s_dx = np.abs(g64 * rstd) * (eb / P + np.abs(xh) * eg / P
                                 + 6 * U * (np.abs(dy64) + np.abs(dbeta) / P + np.abs(xh * dgamma) / P))
    return dict(dx=ulp_bf16(dx) + (1 + 2.0 ** -8) * s_dx, dgamma=eg, dbeta=eb)


def worst(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0, x / 0 as inf): <= 1 passes"""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(q.max())


# ---- float32 restatement -----------------------------------------------------------------------------------------------
def _sum32(a, order):
    """sum over axis 0 in float32: "pairwise" = numpy's order over a contiguous axis, "sequential" = row after row"""
    a = np.asarray(a, np.float32)
    if order == "pairwise":
        return np.add.reduce(np.ascontiguousarray(a.T), axis=-1, dtype=np.float32)
    acc = np.zeros(a.shape[1:], np.float32)
    for k in range(a.shape[0]):
        acc = acc + a[k]
    return acc


def fwd32(x, gamma, beta, eps=EPS, relu=False, running=None, momentum=MOMENTUM, order="sequential", variance="two-pass"):
    """fwd64's dict with every operation in float32 and y rounded to bf16.  variance="naive": E[x^2] - mu^2."""
    x, gamma, beta = (np.asarray(v, np.float32) for v in (x, gamma, beta))
    P = np.float32(x.shape[0])
    mu = _sum32(x, order) / P
    if variance == "naive":
        v = _sum32(x * x, order) / P - mu * mu
    else:
        dlt = x - mu
        v = _sum32(dlt * dlt, order) / P
    rstd = np.float32(1.0) / np.sqrt(v + np.float32(eps))
    xh = (x - mu) * rstd
    y = gamma * xh + beta
    out = dict(y=bf16_round(np.maximum(y, np.float32(0)) if relu else y), mean=mu, var=v, rstd=rstd, xh=xh)
    if running is not None:
        rm, rv = (np.asarray(t, np.float32) for t in running)
        m = np.float32(momentum)
        out["rm"] = (np.float32(1) - m) * rm + m * mu
        out["rv"] = (np.float32(1) - m) * rv + m * (v * P / (P - np.float32(1)))
    return out


def bwd32(dy, x, gamma, mean, rstd, order="sequential"):
    dy, x, gamma, mean, rstd = (np.asarray(v, np.float32) for v in (dy, x, gamma, mean, rstd))
    P = np.float32(x.shape[0])
    xh = (x - mean) * rstd
    dbeta, dgamma = _sum32(dy, order), _sum32(dy * xh, order)
    return bf16_round(gamma * rstd * (dy - dbeta / P - xh * (dgamma / P))), dgamma, dbeta


# ---- the network with batch normalisation ----------------------------------------------------------------------------------
def forward_graph_bn(graph, num_priors, classes, params, image_nhwc, running=None, train=True, emulate_bf16=True, eps=EPS,
                     momentum=MOMENTUM):
    """oracle.net_oracle.forward_graph for resnet50_ssd512_graph(batchnorm=True): a node op="bn" normalises the (bf16-rounded)
    output of the convolution in front of it, with the batch's statistics (train=True) or with running[i] = (mean, var) of bn
    node i, then its ReLU, then the rounding of the stored map.  params: conv{i} / head{l} as forward_graph, bn{i}/gamma and
    bn{i}/beta by bn-node index.  Returns (loc, conf, stats): stats[i] = (mean, biased var, updated running mean, updated
    running var) of bn node i in training mode (the running pair only where `running` is given), {} otherwise."""
    import torch
    import torch.nn.functional as F
    from oracle.net_oracle import _RoundBF16, _same_pad, conv_tf
    rnd = _RoundBF16.apply if emulate_bf16 else (lambda t: t)
    outs = {-1: image_nhwc.permute(0, 3, 1, 2)}
    feats, stats = [], {}
    for i, nd in enumerate(graph):
        if nd["op"] == "conv":
            y = conv_tf(outs[nd["src"]], params["conv%d/kernel" % i], params["conv%d/bias" % i], nd["k"], nd["stride"], True,
                        nd["relu"])
        elif nd["op"] == "bn":
            x = outs[nd["src"]]
            gamma, beta = params["bn%d/gamma" % i].view(1, -1, 1, 1), params["bn%d/beta" % i].view(1, -1, 1, 1)
            if train:
                P = x.numel() // x.shape[1]
                mu = x.mean((0, 2, 3))
                var = ((x - mu.view(1, -1, 1, 1)) ** 2).mean((0, 2, 3))
                st = (mu.detach(), var.detach())
                if running is not None:
                    rm, rv = running[i]
                    st += ((1 - momentum) * rm + momentum * st[0], (1 - momentum) * rv + momentum * st[1] * P / (P - 1))
                stats[i] = st
            else:
                mu, var = running[i]
            y = gamma * ((x - mu.view(1, -1, 1, 1)) * torch.rsqrt(var + eps).view(1, -1, 1, 1)) + beta
            if nd["relu"]:
                y = y.relu()
        elif nd["op"] == "pool3":
            x = outs[nd["src"]]
            _, pt, pb = _same_pad(x.shape[2], 3, 2)
            _, pl, pr = _same_pad(x.shape[3], 3, 2)
            y = F.max_pool2d(F.pad(x, (pl, pr, pt, pb), value=float("-inf")), 3, 2)
        else:
            a, sc = nd["src"]
            y = (outs[a] + outs[sc]).relu()
        outs[i] = rnd(y)
        if nd["feature"]:
            feats.append(outs[i])
    locs, confs = [], []
    B = image_nhwc.shape[0]
    for lvl, (f, n) in enumerate(zip(feats, num_priors)):
        y = conv_tf(f, params["head%d/kernel" % lvl], params["head%d/bias" % lvl], 3, 1, True, False)
        y = rnd(y).permute(0, 2, 3, 1)
        locs.append(y[..., :n * 4].reshape(B, -1, 4))
        confs.append(y[..., n * 4:].reshape(B, -1, classes))
    return torch.cat(locs, 1), torch.cat(confs, 1), stats
