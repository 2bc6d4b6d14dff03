// Batch normalisation over the rows of an NHWC map, training and inference forward and the backward pass (no reference
// counterpart: the reference's VGG network has no normalisation; the ResNet-50 SSD512 trunk trains with it, resnet_engine.py).
// x, y, dy, dx: bf16 [P][C]; everything per channel fp32 [C]; all arithmetic fp32.  Per channel c over the P rows:
//   mu = mean x     v = mean (x - mu)^2     rstd = 1 / sqrt(v + eps)     y = bf16(gamma (x - mu) rstd + beta)  [max(., 0)]
//   xh = (x - mu) rstd     dbeta = sum dy     dgamma = sum dy xh     dx = bf16(gamma rstd (dy - dbeta / P - xh dgamma / P))
// All five kernels are HBM-bound streams with one thread layout: a lane owns 8 channels of a row (one 16-byte load), the
// C / 8 lanes of a row sit side by side, a workgroup of 256 threads covers rpp = 256 / (C / 8) rows per pass (a "chunk": 4 KiB
// of contiguous memory where C / 8 divides 256) and walks chunks blockIdx, blockIdx + gridDim, ...
// Statistics without cancellation: a thread sums d = x - K and d^2 with K the first value it sees of the channel (differences
// of bf16 values: exact in fp32 within 16 binades), which gives its (n, mean, M2) = (n, K + s / n, q - s^2 / n) with |K - mean|
// of the order of the spread, not of the offset; threads, then slabs, merge by Chan's formula
//   n = na + nb   d = mb - ma   mean = ma + d nb / n   M2 = M2a + M2b + d^2 na nb / n.
// Reproducibility: a workgroup merges its rows in row order through LDS and writes ONE row of partials per slab (every row of
// the workspace is written: no initial contents needed), the finalize kernels merge the slabs in a fixed order (group g takes
// slabs g, g + 32, ... in ascending order, then the 32 groups in group order).  No atomics; the grids depend on (P, C) only.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxC = 2048;
constexpr int kMaxSlabs = 1024;               // 4 workgroups per CU; 2048 measured 10 - 20 % slower on the large maps
constexpr int kSlabRows = 32;                 // rows per slab at least (where P has them): a slab's partials are 8 C bytes against 2 C per row
constexpr int kApplyBlocks = 2048;            // 8 workgroups per CU
constexpr int kRedGroups = 32;                // finalize: 32 channels x 32 slab groups per workgroup

__device__ __forceinline__ unsigned pack2(float a, float b) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, b2));
}
__device__ __forceinline__ void unpack8(const uint4 v, float* f) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = __uint_as_float(w[k] << 16);
        f[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
}

struct Layout {
    int c8, rpp, slabs;
    long long chunks;
};

Layout layout(long long P, int C) {
    Layout l;
    l.c8 = C / 8;
    l.rpp = kThreads / l.c8;
    l.chunks = (P + l.rpp - 1) / l.rpp;
    const int per = l.rpp > kSlabRows ? l.rpp : kSlabRows;
    const long long s = (P + per - 1) / per;
    l.slabs = (int)(s < kMaxSlabs ? s : kMaxSlabs);
    return l;
}

// rows of slab b: its chunks are b, b + slabs, ... < chunks, each rpp rows but the last chunk of the map
__device__ __forceinline__ float slab_rows(int b, int slabs, long long chunks, int rpp, long long P) {
    if (b >= chunks) return 0.f;
    const long long mine = (chunks - 1 - b) / slabs + 1;
    long long n = mine * rpp;
    if ((chunks - 1) % slabs == b) n -= chunks * rpp - P;
    return (float)n;
}

__device__ __forceinline__ void chan_merge(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
    if (nb == 0.f) return;
    if (na == 0.f) {
        na = nb; ma = mb; Ma = Mb;
        return;
    }
    const float n = na + nb, d = mb - ma, f = nb / n;
    ma = fmaf(d, f, ma);
    Ma = (Ma + Mb) + d * d * (na * f);
    na = n;
}

// one row of partials per slab: part[b][0][c] = mean, part[b][1][c] = M2 of the slab's rows
__global__ __launch_bounds__(kThreads) void k_bn_stats(const uint4* __restrict__ x, float* __restrict__ part, long long P, int C,
                                                       int rpp, long long chunks) {
    __shared__ __attribute__((aligned(16))) float sm[2][kThreads * 8];       // [mean | M2][row of the pass][channel]
    __shared__ float sn[kThreads];
    const int c8 = C >> 3;
    const int rr = threadIdx.x / c8, j = threadIdx.x - rr * c8;
    float K[8], s[8], q[8], n = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) K[k] = s[k] = q[k] = 0.f;
    if (rr < rpp) {
        for (long long t = blockIdx.x; t < chunks; t += gridDim.x) {
            const long long row = t * rpp + rr;
            if (row >= P) break;
            float xv[8];
            unpack8(x[row * c8 + j], xv);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (n == 0.f) K[k] = xv[k];
                const float d = xv[k] - K[k];
                s[k] += d;
                q[k] = fmaf(d, d, q[k]);
            }
            n += 1.f;
        }
        const float inv = n > 0.f ? 1.0f / n : 0.f;
        float m[8], M[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float ds = s[k] * inv;
            m[k] = K[k] + ds;
            M[k] = fmaxf(fmaf(-s[k], ds, q[k]), 0.f);
        }
        float4* pm = (float4*)&sm[0][rr * C + 8 * j];
        float4* pM = (float4*)&sm[1][rr * C + 8 * j];
        pm[0] = make_float4(m[0], m[1], m[2], m[3]);
        pm[1] = make_float4(m[4], m[5], m[6], m[7]);
        pM[0] = make_float4(M[0], M[1], M[2], M[3]);
        pM[1] = make_float4(M[4], M[5], M[6], M[7]);
        if (j == 0) sn[rr] = n;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kThreads) {
        float na = 0.f, ma = 0.f, Ma = 0.f;
        for (int r = 0; r < rpp; ++r) chan_merge(na, ma, Ma, sn[r], sm[0][r * C + c], sm[1][r * C + c]);
        part[((long long)blockIdx.x * 2) * C + c] = ma;
        part[((long long)blockIdx.x * 2 + 1) * C + c] = Ma;
    }
}

__global__ __launch_bounds__(32 * kRedGroups) void k_bn_stats_finalize(const float* __restrict__ part, int slabs, long long chunks,
                                                                        int rpp, long long P, int C, float eps, float momentum,
                                                                        float* __restrict__ mean, float* __restrict__ rstd,
                                                                        float* running_mean, float* running_var) {
    __shared__ float rn[kRedGroups][32], rm[kRedGroups][32], rM[kRedGroups][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float na = 0.f, ma = 0.f, Ma = 0.f;
    for (int b = g; b < slabs; b += kRedGroups)
        chan_merge(na, ma, Ma, slab_rows(b, slabs, chunks, rpp, P), part[((long long)b * 2) * C + c],
                   part[((long long)b * 2 + 1) * C + c]);
    rn[g][cl] = na; rm[g][cl] = ma; rM[g][cl] = Ma;
    __syncthreads();
    if (g == 0) {
        for (int k = 1; k < kRedGroups; ++k) chan_merge(na, ma, Ma, rn[k][cl], rm[k][cl], rM[k][cl]);
        const float v = Ma / (float)P;
        mean[c] = ma;
        rstd[c] = 1.0f / sqrtf(v + eps);
        if (running_mean != nullptr) {
            const float keep = 1.0f - momentum;
            running_mean[c] = fmaf(momentum, ma, keep * running_mean[c]);
            running_var[c] = fmaf(momentum, Ma / (float)(P - 1), keep * running_var[c]);
        }
    }
}

// TRAIN: y = (x - p0) p1 + p2 with (p0, p1, p2) = (mean, gamma rstd, beta); else y = x p1 + p2 with p1 = gamma / sqrt(rv + eps),
// p2 = beta - rm p1
template <bool TRAIN>
__global__ __launch_bounds__(kThreads) void k_bn_apply(const uint4* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ s0,
                                                       const float* __restrict__ s1, uint4* __restrict__ y, float eps, int relu,
                                                       long long P, int C, int rpp, long long chunks) {
    const int c8 = C >> 3;
    const int rr = threadIdx.x / c8, j = threadIdx.x - rr * c8;
    if (rr >= rpp) return;
    float p0[8], p1[8], p2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = 8 * j + k;
        if (TRAIN) {
            p0[k] = s0[c];
            p1[k] = gamma[c] * s1[c];
            p2[k] = beta[c];
        } else {
            p0[k] = 0.f;
            p1[k] = gamma[c] / sqrtf(s1[c] + eps);
            p2[k] = fmaf(-s0[c], p1[k], beta[c]);
        }
    }
    for (long long t = blockIdx.x; t < chunks; t += gridDim.x) {
        const long long row = t * rpp + rr;
        if (row >= P) break;
        float xv[8], o[8];
        unpack8(x[row * c8 + j], xv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            o[k] = fmaf(TRAIN ? xv[k] - p0[k] : xv[k], p1[k], p2[k]);
            if (relu) o[k] = fmaxf(o[k], 0.f);
        }
        y[row * c8 + j] = pack8(o);
    }
}

// part[b][0][c] = sum dy, part[b][1][c] = sum dy xh over the slab's rows
__global__ __launch_bounds__(kThreads) void k_bn_bwd_sums(const uint4* __restrict__ dy, const uint4* __restrict__ x,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          float* __restrict__ part, long long P, int C, int rpp, long long chunks) {
    __shared__ __attribute__((aligned(16))) float sm[2][kThreads * 8];
    const int c8 = C >> 3;
    const int rr = threadIdx.x / c8, j = threadIdx.x - rr * c8;
    if (rr < rpp) {
        float mu[8], rs[8], db[8], dg[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            mu[k] = mean[8 * j + k];
            rs[k] = rstd[8 * j + k];
            db[k] = dg[k] = 0.f;
        }
        for (long long t = blockIdx.x; t < chunks; t += gridDim.x) {
            const long long row = t * rpp + rr;
            if (row >= P) break;
            float xv[8], g[8];
            unpack8(x[row * c8 + j], xv);
            unpack8(dy[row * c8 + j], g);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                db[k] += g[k];
                dg[k] = fmaf(g[k], (xv[k] - mu[k]) * rs[k], dg[k]);
            }
        }
        float4* pb = (float4*)&sm[0][rr * C + 8 * j];
        float4* pg = (float4*)&sm[1][rr * C + 8 * j];
        pb[0] = make_float4(db[0], db[1], db[2], db[3]);
        pb[1] = make_float4(db[4], db[5], db[6], db[7]);
        pg[0] = make_float4(dg[0], dg[1], dg[2], dg[3]);
        pg[1] = make_float4(dg[4], dg[5], dg[6], dg[7]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kThreads) {
        float b = sm[0][c], g = sm[1][c];
        for (int r = 1; r < rpp; ++r) {
            b += sm[0][r * C + c];
            g += sm[1][r * C + c];
        }
        part[((long long)blockIdx.x * 2) * C + c] = b;
        part[((long long)blockIdx.x * 2 + 1) * C + c] = g;
    }
}

__global__ __launch_bounds__(32 * kRedGroups) void k_bn_bwd_finalize(const float* __restrict__ part, int slabs, int C,
                                                                      float* __restrict__ dbeta, float* __restrict__ dgamma) {
    __shared__ float rb[kRedGroups][32], rg[kRedGroups][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float b = 0.f, q = 0.f;
    for (int r = g; r < slabs; r += kRedGroups) {
        b += part[((long long)r * 2) * C + c];
        q += part[((long long)r * 2 + 1) * C + c];
    }
    rb[g][cl] = b; rg[g][cl] = q;
    __syncthreads();
    if (g == 0) {
        for (int k = 1; k < kRedGroups; ++k) {
            b += rb[k][cl];
            q += rg[k][cl];
        }
        dbeta[c] = b;
        dgamma[c] = q;
    }
}

__global__ __launch_bounds__(kThreads) void k_bn_bwd_dx(const uint4* __restrict__ dy, const uint4* __restrict__ x,
                                                        const float* __restrict__ gamma, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const float* __restrict__ dbeta,
                                                        const float* __restrict__ dgamma, uint4* __restrict__ dx, long long P, int C,
                                                        int rpp, long long chunks) {
    const int c8 = C >> 3;
    const int rr = threadIdx.x / c8, j = threadIdx.x - rr * c8;
    if (rr >= rpp) return;
    float mu[8], rs[8], a[8], mb[8], mg[8];
    const float fP = (float)P;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = 8 * j + k;
        mu[k] = mean[c];
        rs[k] = rstd[c];
        a[k] = gamma[c] * rs[k];
        mb[k] = dbeta[c] / fP;
        mg[k] = dgamma[c] / fP;
    }
    for (long long t = blockIdx.x; t < chunks; t += gridDim.x) {
        const long long row = t * rpp + rr;
        if (row >= P) break;
        float xv[8], g[8], o[8];
        unpack8(x[row * c8 + j], xv);
        unpack8(dy[row * c8 + j], g);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float xh = (xv[k] - mu[k]) * rs[k];
            o[k] = a[k] * ((g[k] - mb[k]) - xh * mg[k]);
        }
        dx[row * c8 + j] = pack8(o);
    }
}

bool shape_ok(int C) { return C >= 64 && C <= kMaxC && C % 64 == 0; }

int apply_blocks(const Layout& l) { return (int)(l.chunks < kApplyBlocks ? l.chunks : kApplyBlocks); }

}  // namespace

extern "C" size_t ssd_bn_ws_bytes(long long P, int C) {
    if (P < 1 || !shape_ok(C)) return 0;
    return (size_t)layout(P, C).slabs * 2 * (size_t)C * sizeof(float);
}

extern "C" int ssd_bn_fwd_train(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                float* running_mean, float* running_var, float momentum, float eps, int relu, void* ws,
                                size_t ws_bytes, long long P, int C, void* stream) {
    if (x == nullptr || gamma == nullptr || beta == nullptr || y == nullptr || mean == nullptr || rstd == nullptr || x == y ||
        (running_mean == nullptr) != (running_var == nullptr) || !(eps > 0.f) || !(momentum > 0.f && momentum <= 1.f))
        return SSD_ERR_VALUE;
    if (!shape_ok(C)) return SSD_ERR_UNSUPPORTED;
    if (P < 2 || ws == nullptr || ws_bytes < ssd_bn_ws_bytes(P, C)) return SSD_ERR_VALUE;
    const Layout l = layout(P, C);
    hipStream_t s = (hipStream_t)stream;
    k_bn_stats<<<l.slabs, kThreads, 0, s>>>((const uint4*)x, (float*)ws, P, C, l.rpp, l.chunks);
    k_bn_stats_finalize<<<C / 32, 32 * kRedGroups, 0, s>>>((const float*)ws, l.slabs, l.chunks, l.rpp, P, C, eps, momentum, mean,
                                                           rstd, running_mean, running_var);
    k_bn_apply<true><<<apply_blocks(l), kThreads, 0, s>>>((const uint4*)x, gamma, beta, mean, rstd, (uint4*)y, eps, relu ? 1 : 0,
                                                          P, C, l.rpp, l.chunks);
    return ssd_launch_status();
}

extern "C" int ssd_bn_fwd_infer(const void* x, const float* gamma, const float* beta, const float* running_mean,
                                const float* running_var, void* y, float eps, int relu, long long P, int C, void* stream) {
    if (x == nullptr || gamma == nullptr || beta == nullptr || running_mean == nullptr || running_var == nullptr ||
        y == nullptr || x == y || !(eps > 0.f))
        return SSD_ERR_VALUE;
    if (!shape_ok(C)) return SSD_ERR_UNSUPPORTED;
    if (P < 1) return SSD_ERR_VALUE;
    const Layout l = layout(P, C);
    k_bn_apply<false><<<apply_blocks(l), kThreads, 0, (hipStream_t)stream>>>((const uint4*)x, gamma, beta, running_mean,
                                                                             running_var, (uint4*)y, eps, relu ? 1 : 0, P, C,
                                                                             l.rpp, l.chunks);
    return ssd_launch_status();
}

extern "C" int ssd_bn_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx,
                          float* dgamma, float* dbeta, void* ws, size_t ws_bytes, long long P, int C, void* stream) {
    if (dy == nullptr || x == nullptr || gamma == nullptr || mean == nullptr || rstd == nullptr || dx == nullptr ||
        dgamma == nullptr || dbeta == nullptr || dx == x || dx == dy)
        return SSD_ERR_VALUE;
    if (!shape_ok(C)) return SSD_ERR_UNSUPPORTED;
    if (P < 2 || ws == nullptr || ws_bytes < ssd_bn_ws_bytes(P, C)) return SSD_ERR_VALUE;
    const Layout l = layout(P, C);
    hipStream_t s = (hipStream_t)stream;
    k_bn_bwd_sums<<<l.slabs, kThreads, 0, s>>>((const uint4*)dy, (const uint4*)x, mean, rstd, (float*)ws, P, C, l.rpp, l.chunks);
    k_bn_bwd_finalize<<<C / 32, 32 * kRedGroups, 0, s>>>((const float*)ws, l.slabs, C, dbeta, dgamma);
    k_bn_bwd_dx<<<apply_blocks(l), kThreads, 0, s>>>((const uint4*)dy, (const uint4*)x, gamma, mean, rstd, dbeta, dgamma,
                                                     (uint4*)dx, P, C, l.rpp, l.chunks);
    return ssd_launch_status();
}
