// L2 normalisation of a feature map over its channels with a learned per-channel scale (SSD paper section 3.1, after ParseNet;
// Caffe SSD's Normalize layer on conv4_3) -- no reference counterpart: the reference feeds the 38x38 map to its head as it is.
// Per pixel p over C channels, operands bf16, arithmetic fp32:
//   r_p = 1 / sqrt(sum_k x_pk^2 + eps)     xh_pc = x_pc r_p     y_pc = bf16(s_c xh_pc)
//   t_pc = s_c dy_pc     D_p = sum_k t_pk xh_pk     dx_pc = bf16(r_p (t_pc - xh_pc D_p))     ds_c = sum_p dy_pc xh_pc
// Both passes are HBM-bound streams.  One wave per pixel: lane l holds channels 8 (l + 64 v) .. + 7 (16-byte loads; v < 2
// covers C <= 1024, lanes past C / 8 idle), the per-pixel sums are xor butterflies over the 64 lanes, s stays in registers, no
// LDS on the per-pixel path.  A wave walks pixels wave, wave + waves, ...
// ds is bitwise reproducible: every wave sums its pixels in ascending order in registers, a workgroup adds its four waves in
// wave order through LDS and writes one row of partials (every row of the workspace is written, so it needs no initial
// contents), and k_l2norm_dscale adds the rows in a fixed order.  The grid is a function of (P, C) alone.
#include "common.h"

namespace {

constexpr int kThreads = 256;                 // 4 waves
constexpr int kWaves = kThreads / SSD_WAVE;
constexpr int kMaxC = 1024;
constexpr int kFwdBlocks = 2048;              // 8 workgroups per CU
constexpr int kBwdBlocks = 1536;              // = rows of ds partials; 6 per CU: k_l2norm_bwd<1> (72 VGPRs) fits 7, so one round
constexpr int kRedGroups = 32;                // k_l2norm_dscale: 32 channels x 32 row groups per workgroup

__device__ __forceinline__ float bf2f_(unsigned v16) { return __uint_as_float(v16 << 16); }
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
        f[2 * k] = bf2f_(w[k] & 0xffffu);
        f[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    return make_uint4(pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7]));
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 1; m < SSD_WAVE; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// 1 / sqrt(sum x^2 + eps) of the pixel whose channels the wave's lanes hold (zeros in idle lanes).  The squares of bf16 values
// are exact in fp32; the sum is a pairwise tree (in the lane, over v, then the butterfly) written out with explicit fmaf so that
// the forward pass and a backward pass that recomputes it produce the same bits.
template <int NV>
__device__ __forceinline__ float pixel_rnorm(const float (*x)[8], float eps) {
    float ss = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const float a = fmaf(x[v][1], x[v][1], x[v][0] * x[v][0]), b = fmaf(x[v][3], x[v][3], x[v][2] * x[v][2]);
        const float c = fmaf(x[v][5], x[v][5], x[v][4] * x[v][4]), d = fmaf(x[v][7], x[v][7], x[v][6] * x[v][6]);
        ss += (a + b) + (c + d);
    }
    ss = wave_sum(ss);
    return 1.0f / sqrtf(ss + eps);
}

template <int NV>
__global__ __launch_bounds__(kThreads) void k_l2norm_fwd(const uint4* __restrict__ x, const float* __restrict__ scale,
                                                         uint4* __restrict__ y, float* __restrict__ rnorm, long long P, int C,
                                                         float eps) {
    const int lane = threadIdx.x & (SSD_WAVE - 1);
    const int c8 = C >> 3;
    float s[NV][8];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int j = lane + SSD_WAVE * v;
#pragma unroll
        for (int k = 0; k < 8; ++k) s[v][k] = j < c8 ? scale[8 * j + k] : 0.f;
    }
    const long long waves = (long long)gridDim.x * kWaves;
    for (long long p = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); p < P; p += waves) {
        float xv[NV][8];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int j = lane + SSD_WAVE * v;
            unpack8(j < c8 ? x[p * c8 + j] : make_uint4(0, 0, 0, 0), xv[v]);
        }
        const float r = pixel_rnorm<NV>(xv, eps);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int j = lane + SSD_WAVE * v;
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = s[v][k] * (xv[v][k] * r);
            if (j < c8) y[p * c8 + j] = pack8(o);
        }
        if (rnorm != nullptr && lane == 0) rnorm[p] = r;
    }
}

// dx and one row of ds partials per workgroup: partial[blockIdx.x][c] = sum over the workgroup's pixels of dy_pc xh_pc.
template <int NV>
__global__ __launch_bounds__(kThreads) void k_l2norm_bwd(const uint4* __restrict__ dy, const uint4* __restrict__ x,
                                                         const float* __restrict__ scale, const float* __restrict__ rnorm,
                                                         uint4* dx, int accumulate, float* __restrict__ partial, long long P, int C,
                                                         float eps) {
    __shared__ float red[kWaves][kMaxC];
    const int lane = threadIdx.x & (SSD_WAVE - 1), wave = threadIdx.x >> 6;
    const int c8 = C >> 3;
    float s[NV][8], acc[NV][8];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int j = lane + SSD_WAVE * v;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s[v][k] = j < c8 ? scale[8 * j + k] : 0.f;
            acc[v][k] = 0.f;
        }
    }
    const long long waves = (long long)gridDim.x * kWaves;
    for (long long p = (long long)blockIdx.x * kWaves + wave; p < P; p += waves) {
        float xv[NV][8], g[NV][8];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int j = lane + SSD_WAVE * v;
            const bool in = j < c8;
            unpack8(in ? x[p * c8 + j] : make_uint4(0, 0, 0, 0), xv[v]);
            unpack8(in ? dy[p * c8 + j] : make_uint4(0, 0, 0, 0), g[v]);
        }
        const float r = rnorm != nullptr ? rnorm[p] : pixel_rnorm<NV>(xv, eps);
        float d = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                xv[v][k] *= r;                                   // xh, rebuilt from x in fp32
                acc[v][k] = fmaf(g[v][k], xv[v][k], acc[v][k]);
                g[v][k] *= s[v][k];                              // t
                d = fmaf(g[v][k], xv[v][k], d);
            }
        d = wave_sum(d);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int j = lane + SSD_WAVE * v;
            if (j >= c8) continue;
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = r * (g[v][k] - xv[v][k] * d);
            if (accumulate) {
                float old[8];
                unpack8(dx[p * c8 + j], old);
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] += old[k];
            }
            dx[p * c8 + j] = pack8(o);
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int j = lane + SSD_WAVE * v;
        if (j < c8) {
#pragma unroll
            for (int k = 0; k < 8; ++k) red[wave][8 * j + k] = acc[v][k];
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += kThreads) {
        float t = red[0][c];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += red[w][c];
        partial[(long long)blockIdx.x * C + c] = t;
    }
}

// ds[c] = sum of the `rows` partial rows: thread (g, c) adds rows g, g + 32, ... in ascending order, then the 32 groups are
// added in group order.  One workgroup per 32 channels (128-byte row segments).
__global__ __launch_bounds__(32 * kRedGroups) void k_l2norm_dscale(const float* __restrict__ partial, int rows, int C,
                                                                    float* __restrict__ ds) {
    __shared__ float red[kRedGroups][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float t = 0.f;
    for (int r = g; r < rows; r += kRedGroups) t += partial[(long long)r * C + c];
    red[g][cl] = t;
    __syncthreads();
    if (g == 0) {
        float sum = red[0][cl];
        for (int k = 1; k < kRedGroups; ++k) sum += red[k][cl];
        ds[c] = sum;
    }
}

bool shape_ok(int C) { return C >= 128 && C <= kMaxC && C % 128 == 0; }

int bwd_blocks(long long P) {
    const long long b = (P + kWaves - 1) / kWaves;
    return (int)(b < kBwdBlocks ? b : kBwdBlocks);
}

}  // namespace

extern "C" size_t ssd_l2norm_ws_bytes(long long P, int C) {
    if (P < 1 || !shape_ok(C)) return 0;
    return (size_t)bwd_blocks(P) * (size_t)C * sizeof(float);
}

extern "C" int ssd_l2norm_fwd(const void* x, const float* scale, void* y, float* rnorm, long long P, int C, float eps,
                              void* stream) {
    if (x == nullptr || scale == nullptr || y == nullptr || x == y || P < 1 || !(eps >= 0.f)) return SSD_ERR_VALUE;
    if (!shape_ok(C)) return SSD_ERR_UNSUPPORTED;
    const long long b = (P + kWaves - 1) / kWaves;
    const int grid = (int)(b < kFwdBlocks ? b : kFwdBlocks);
    hipStream_t s = (hipStream_t)stream;
    if (C <= 512)
        k_l2norm_fwd<1><<<grid, kThreads, 0, s>>>((const uint4*)x, scale, (uint4*)y, rnorm, P, C, eps);
    else
        k_l2norm_fwd<2><<<grid, kThreads, 0, s>>>((const uint4*)x, scale, (uint4*)y, rnorm, P, C, eps);
    return ssd_launch_status();
}

extern "C" int ssd_l2norm_bwd(const void* dy, const void* x, const float* scale, const float* rnorm, void* dx, int accumulate,
                              float* dscale, void* ws, size_t ws_bytes, long long P, int C, float eps, void* stream) {
    if (dy == nullptr || x == nullptr || scale == nullptr || dx == nullptr || dscale == nullptr || dx == x || dx == dy || P < 1 ||
        !(eps >= 0.f))
        return SSD_ERR_VALUE;
    if (!shape_ok(C)) return SSD_ERR_UNSUPPORTED;
    if (ws == nullptr || ws_bytes < ssd_l2norm_ws_bytes(P, C)) return SSD_ERR_VALUE;
    const int grid = bwd_blocks(P);
    hipStream_t s = (hipStream_t)stream;
    if (C <= 512)
        k_l2norm_bwd<1><<<grid, kThreads, 0, s>>>((const uint4*)dy, (const uint4*)x, scale, rnorm, (uint4*)dx, accumulate ? 1 : 0,
                                                  (float*)ws, P, C, eps);
    else
        k_l2norm_bwd<2><<<grid, kThreads, 0, s>>>((const uint4*)dy, (const uint4*)x, scale, rnorm, (uint4*)dx, accumulate ? 1 : 0,
                                                  (float*)ws, P, C, eps);
    k_l2norm_dscale<<<C / 32, 32 * kRedGroups, 0, s>>>((const float*)ws, grid, C, dscale);
    return ssd_launch_status();
}
