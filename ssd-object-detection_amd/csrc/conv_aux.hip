// The kernels of the convolution stack that are not convolutions (NHWC bf16, gfx950): weight transposes for the data gradient,
// the f32 -> bf16 cast, image preparation, 2x2 / stride-2 max pooling forward / backward (models/ssd_model.py:77-84) and the
// packing of the head gradients into a level's padded NHWC map.  Each with its C entry point at the end of the file.
#include "common.h"
#include <hip/hip_bf16.h>

#include "conv_common.h"
namespace {

// ------------------------------------------------------------------------------------------------
// W[co][kh][kw][ci] (bf16) -> Wt[ci][KH-1-kh][KW-1-kw][co] for the data gradient
__global__ void k_weight_transpose(const bf16_raw* __restrict__ w, bf16_raw* __restrict__ wt, int Cout, int KH, int KW,
                                   int Cin, int Cout_pad) {
    // wt has row length KH*KW*Cout_pad (Cout padded to a multiple of 8 with zeros)
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)Cin * KH * KW * Cout_pad;
    if (i >= total) return;
    const int co = (int)(i % Cout_pad);
    long long r = i / Cout_pad;
    const int kw = (int)(r % KW); r /= KW;
    const int kh = (int)(r % KH); r /= KH;
    const int ci = (int)r;
    bf16_raw v = 0;
    if (co < Cout) v = w[(((long long)co * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)) * Cin + ci];
    wt[i] = v;
}

// All transposed copies of a network in ONE launch: blockIdx.y = tensor, descriptor rows {src, dst, Cout, K, Cin, Cout_pad}
// (device array of int64), blockIdx.x = 32x32 (co, ci) tile x tap; the tile goes through LDS so that both the read (ci
// contiguous) and the write (co contiguous) are 64-byte runs.  33 launches of the per-tensor kernel cost 0.26 ms per step.
__global__ __launch_bounds__(256) void k_weight_transpose_batched(const long long* __restrict__ desc) {
    __shared__ bf16_raw tile[32][33];
    const long long* d = desc + (long long)blockIdx.y * 6;
    const bf16_raw* w = reinterpret_cast<const bf16_raw*>(d[0]);
    bf16_raw* wt = reinterpret_cast<bf16_raw*>(d[1]);
    // K field: kernel size in the low byte; bit 8 set = tap-major layout for the sparse head data gradient (sparse.hip):
    // wt[kh][kw][ci][co] = w[co][kh][kw][ci], not flipped
    const int Cout = (int)d[2], K = (int)d[3] & 0xff, tapmajor = ((int)d[3] >> 8) & 1, Cin = (int)d[4], Cout_pad = (int)d[5];
    const int tco = (Cout_pad + 31) >> 5, tci = (Cin + 31) >> 5;
    int t = blockIdx.x;
    if (t >= tco * tci * K * K) return;
    const int tap = t % (K * K); t /= K * K;
    const int ci0 = (t % tci) * 32, co0 = (t / tci) * 32;
    const int kh = tap / K, kw = tap - kh * K;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;                 // 32 x 8
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int co = co0 + ty + 8 * j, ci = ci0 + tx;
        bf16_raw v = 0;
        const int skh = tapmajor ? kh : K - 1 - kh, skw = tapmajor ? kw : K - 1 - kw;
        if (co < Cout && ci < Cin) v = w[(((long long)co * K + skh) * K + skw) * Cin + ci];
        tile[ty + 8 * j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = ci0 + ty + 8 * j, co = co0 + tx;
        if (ci >= Cin || co >= Cout_pad) continue;
        if (tapmajor) wt[(((long long)kh * K + kw) * Cin + ci) * Cout_pad + co] = tile[tx][ty + 8 * j];
        else wt[(((long long)ci * K + kh) * K + kw) * Cout_pad + co] = tile[tx][ty + 8 * j];
    }
}

// f32 -> bf16 cast (weights after an optimizer step)
__global__ void k_cast_bf16(const float* __restrict__ src, bf16_raw* __restrict__ dst, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = f2bf(src[i]);
}

// image f32 [B,H,W,3] in [0,1] -> bf16 [B,H,W,8], (x-0.5)*2 (models/ssd_model.py:214), channels 3..7 zero
__global__ void k_image_prep(const float* __restrict__ img, bf16_raw* __restrict__ out, long long npix, int normalize) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    float r = img[3 * i], gch = img[3 * i + 1], b = img[3 * i + 2];
    if (normalize) { r = (r - 0.5f) * 2.f; gch = (gch - 0.5f) * 2.f; b = (b - 0.5f) * 2.f; }
    *reinterpret_cast<uint4*>(out + 8 * i) =
        make_uint4(pack_bf16x2(r, gch), (unsigned)f2bf(b), 0u, 0u);
}

// 2x2 stride-2 max pooling, NHWC bf16, 8 channels per thread.  pad_b/pad_r = 1 for TF "SAME" on odd sizes.
__global__ void k_maxpool_fwd(const bf16_raw* __restrict__ x, bf16_raw* __restrict__ y, int B, int H, int W, int C,
                              int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c8 = C >> 3;
    const long long total = (long long)B * Ho * Wo * c8;
    if (i >= total) return;
    const int c = (int)(i % c8);
    long long r = i / c8;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float best[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) best[k] = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int iy = 2 * oy + dy, ix = 2 * ox + dx;
            if (iy >= H || ix >= W) continue;
            const uint4 v = *reinterpret_cast<const uint4*>(x + ((((long long)b * H + iy) * W + ix) * C + c * 8));
            const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                best[2 * k] = fmaxf(best[2 * k], __uint_as_float(wds[k] << 16));
                best[2 * k + 1] = fmaxf(best[2 * k + 1], __uint_as_float(wds[k] & 0xffff0000u));
            }
        }
    unsigned o[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (__float_as_uint(best[2 * k]) >> 16) | (__float_as_uint(best[2 * k + 1]) & 0xffff0000u);
    *reinterpret_cast<uint4*>(y + ((((long long)b * Ho + oy) * Wo + ox) * C + c * 8)) = make_uint4(o[0], o[1], o[2], o[3]);
}

// Backward of the pooling + the ReLU in front of it: dx = dy at the first maximum of each window (TF
// MaxPoolGrad), zero elsewhere and wherever x <= 0 (x is a post-ReLU activation).
__global__ void k_maxpool_bwd(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ y, const bf16_raw* __restrict__ dy,
                              bf16_raw* __restrict__ dx, int B, int H, int W, int C, int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c8 = C >> 3;
    const long long total = (long long)B * Ho * Wo * c8;
    if (i >= total) return;
    const int c = (int)(i % c8);
    long long r = i / c8;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const long long oidx = (((long long)b * Ho + oy) * Wo + ox) * C + c * 8;
    const uint4 yv = *reinterpret_cast<const uint4*>(y + oidx);
    const uint4 gv = *reinterpret_cast<const uint4*>(dy + oidx);
    const bf16_raw* yy = reinterpret_cast<const bf16_raw*>(&yv);
    const bf16_raw* gg = reinterpret_cast<const bf16_raw*>(&gv);
    bool done[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) done[k] = false;
#pragma unroll
    for (int dyy = 0; dyy < 2; ++dyy)
#pragma unroll
        for (int dxx = 0; dxx < 2; ++dxx) {
            const int iy = 2 * oy + dyy, ix = 2 * ox + dxx;
            if (iy >= H || ix >= W) continue;
            const long long iidx = (((long long)b * H + iy) * W + ix) * C + c * 8;
            const uint4 xv = *reinterpret_cast<const uint4*>(x + iidx);
            const bf16_raw* xx = reinterpret_cast<const bf16_raw*>(&xv);
            bf16_raw o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool hit = !done[k] && xx[k] == yy[k];
                o[k] = (hit && bf2f(xx[k]) > 0.f) ? gg[k] : (bf16_raw)0;
                done[k] = done[k] || hit;
            }
            *reinterpret_cast<uint4*>(dx + iidx) = *reinterpret_cast<const uint4*>(o);
        }
}

// Pooling with a recorded winner: the forward pass also writes, per pooled element, a 4-bit code = position (2 dy + dx) of
// the first maximum of its window, or 4 if that maximum is <= 0 (post-ReLU input: no gradient flows).  The backward pass
// then needs only dy and the codes (1/4 byte per input element) instead of re-reading x and y: 0.97 GB instead of
// 1.84 GB for the first pool at batch 64.  Same routing rule as k_maxpool_bwd (TF MaxPoolGrad + ReLU mask).
__global__ void k_maxpool_fwd_argmax(const bf16_raw* __restrict__ x, bf16_raw* __restrict__ y, unsigned* __restrict__ code,
                                     int B, int H, int W, int C, int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c8 = C >> 3;
    if (i >= (long long)B * Ho * Wo * c8) return;
    const int c = (int)(i % c8);
    long long r = i / c8;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    float best[8];
    unsigned pos[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { best[k] = -INFINITY; pos[k] = 4u; }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int iy = 2 * oy + dy, ix = 2 * ox + dx;
            if (iy >= H || ix >= W) continue;
            const uint4 v = *reinterpret_cast<const uint4*>(x + ((((long long)b * H + iy) * W + ix) * C + c * 8));
            const unsigned wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float f = (k & 1) ? __uint_as_float(wds[k >> 1] & 0xffff0000u) : __uint_as_float(wds[k >> 1] << 16);
                if (f > best[k]) { best[k] = f; pos[k] = (unsigned)(2 * dy + dx); }   // strict: the first maximum wins
            }
        }
    unsigned o[4], cw = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (__float_as_uint(best[2 * k]) >> 16) | (__float_as_uint(best[2 * k + 1]) & 0xffff0000u);
#pragma unroll
    for (int k = 0; k < 8; ++k) cw |= (best[k] > 0.f ? pos[k] : 4u) << (4 * k);
    *reinterpret_cast<uint4*>(y + ((((long long)b * Ho + oy) * Wo + ox) * C + c * 8)) = make_uint4(o[0], o[1], o[2], o[3]);
    code[i] = cw;
}

__global__ void k_maxpool_bwd_argmax(const unsigned* __restrict__ code, const bf16_raw* __restrict__ dy, bf16_raw* __restrict__ dx,
                                     int B, int H, int W, int C, int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c8 = C >> 3;
    if (i >= (long long)B * Ho * Wo * c8) return;
    const int c = (int)(i % c8);
    long long r = i / c8;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const uint4 gv = *reinterpret_cast<const uint4*>(dy + ((((long long)b * Ho + oy) * Wo + ox) * C + c * 8));
    const unsigned g[4] = {gv.x, gv.y, gv.z, gv.w};
    const unsigned cw = code[i];
#pragma unroll
    for (int dyy = 0; dyy < 2; ++dyy)
#pragma unroll
        for (int dxx = 0; dxx < 2; ++dxx) {
            const int iy = 2 * oy + dyy, ix = 2 * ox + dxx;
            if (iy >= H || ix >= W) continue;
            const unsigned p = (unsigned)(2 * dyy + dxx);
            unsigned o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned lo = ((cw >> (8 * k)) & 15u) == p ? 0x0000ffffu : 0u;
                const unsigned hi = ((cw >> (8 * k + 4)) & 15u) == p ? 0xffff0000u : 0u;
                o[k] = g[k] & (lo | hi);
            }
            *reinterpret_cast<uint4*>(dx + ((((long long)b * H + iy) * W + ix) * C + c * 8)) = make_uint4(o[0], o[1], o[2], o[3]);
        }
}

// The same un-pooling added onto a dx that already holds a gradient (an activation that feeds a head as well as the
// pooling): dx[p] = bf16(float(dx[p]) + dy) at each window's winner, one fp32 addition and one rounding; every other
// element keeps its bits (code 4, the losers of a window, and the row / column a VALID pooling of an odd map leaves out,
// which no thread visits).  A window has one owner thread, so its four dx chunks are read and written by that thread
// alone: no memset, no atomics.  The four loads are issued before the first store.  Per dx element 2 B read + 2 B
// written + 1/4 of (2 B dy + 1/2 B code), against 2 B written + the same quarter for the overwrite form.
__global__ void k_maxpool_bwd_argmax_acc(const unsigned* __restrict__ code, const bf16_raw* __restrict__ dy, bf16_raw* __restrict__ dx,
                                         int B, int H, int W, int C, int Ho, int Wo) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int c8 = C >> 3;
    if (i >= (long long)B * Ho * Wo * c8) return;
    const int c = (int)(i % c8);
    long long r = i / c8;
    const int ox = (int)(r % Wo); r /= Wo;
    const int oy = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const uint4 gv = *reinterpret_cast<const uint4*>(dy + ((((long long)b * Ho + oy) * Wo + ox) * C + c * 8));
    const unsigned g[4] = {gv.x, gv.y, gv.z, gv.w};
    const unsigned cw = code[i];
    uint4 old[4];
    bool in[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int iy = 2 * oy + (p >> 1), ix = 2 * ox + (p & 1);
        in[p] = iy < H && ix < W;
        old[p] = make_uint4(0u, 0u, 0u, 0u);
        if (in[p]) old[p] = *reinterpret_cast<const uint4*>(dx + ((((long long)b * H + iy) * W + ix) * C + c * 8));
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        if (!in[p]) continue;
        const int iy = 2 * oy + (p >> 1), ix = 2 * ox + (p & 1);
        const unsigned d[4] = {old[p].x, old[p].y, old[p].z, old[p].w};
        unsigned o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned s = pack_bf16x2(__uint_as_float(d[k] << 16) + __uint_as_float(g[k] << 16),
                                           __uint_as_float(d[k] & 0xffff0000u) + __uint_as_float(g[k] & 0xffff0000u));
            const unsigned lo = ((cw >> (8 * k)) & 15u) == (unsigned)p ? 0x0000ffffu : 0u;
            const unsigned hi = ((cw >> (8 * k + 4)) & 15u) == (unsigned)p ? 0xffff0000u : 0u;
            o[k] = (s & (lo | hi)) | (d[k] & ~(lo | hi));
        }
        *reinterpret_cast<uint4*>(dx + ((((long long)b * H + iy) * W + ix) * C + c * 8)) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// dloc [B][A][4], dconf [B][A][classes] (bf16) -> one level's padded NHWC gradient [B][H*W][npad].  A pixel's row is the
// concatenation of its per_cell*4 loc values, its per_cell*classes conf values (both contiguous in the sources) and
// zero padding.  One thread per 16-byte chunk of the output (8 channels): the sources are only 2-byte aligned
// (classes = 81 is odd), so they are read element-wise (consecutive lanes -> consecutive addresses) and stored once.
__global__ void k_head_grad_pack(const bf16_raw* __restrict__ dloc, const bf16_raw* __restrict__ dconf,
                                 bf16_raw* __restrict__ out, int B, int hw, int per_cell, int classes, int npad,
                                 int anchors_total, int level_off) {
    const int cpr = npad >> 3;                                // chunks per row
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * hw * cpr) return;
    const int ch = (int)(i % cpr);
    const long long r = i / cpr;
    const int pix = (int)(r % hw);
    const int b = (int)(r / hw);
    const int n_loc = per_cell * 4, n_conf = per_cell * classes;
    const long long anchor0 = (long long)b * anchors_total + level_off + (long long)pix * per_cell;
    const bf16_raw* pl = dloc + anchor0 * 4;
    const bf16_raw* pc = dconf + anchor0 * classes - n_loc;
    if (!((per_cell | level_off | anchors_total) & 1)) {      // even anchor counts: every run 4-byte aligned, two channels per load
        unsigned w4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = ch * 8 + 2 * j;
            w4[j] = n < n_loc ? *reinterpret_cast<const unsigned*>(pl + n)
                              : (n < n_loc + n_conf ? *reinterpret_cast<const unsigned*>(pc + n) : 0u);
        }
        *reinterpret_cast<uint4*>(out + r * npad + ch * 8) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
        return;
    }
    bf16_raw v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int n = ch * 8 + j;
        v[j] = n < n_loc ? pl[n] : (n < n_loc + n_conf ? pc[n] : (bf16_raw)0);
    }
    *reinterpret_cast<uint4*>(out + r * npad + ch * 8) =
        make_uint4((unsigned)v[0] | ((unsigned)v[1] << 16), (unsigned)v[2] | ((unsigned)v[3] << 16),
                   (unsigned)v[4] | ((unsigned)v[5] << 16), (unsigned)v[6] | ((unsigned)v[7] << 16));
}

}  // namespace

extern "C" {

int ssd_weight_transpose(const void* w, void* w_t, int Cout, int ksize, int Cin, int Cout_pad, void* stream) {
    if (!w || !w_t || Cout <= 0 || ksize <= 0 || Cin <= 0 || Cout_pad < Cout || Cout_pad % 8) return SSD_ERR_VALUE;
    const long long total = (long long)Cin * ksize * ksize * Cout_pad;
    hipLaunchKernelGGL(k_weight_transpose, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const bf16_raw*>(w), static_cast<bf16_raw*>(w_t), Cout, ksize, ksize, Cin, Cout_pad);
    return ssd_launch_status();
}

int ssd_weight_transpose_batched(const long long* desc, int ntensors, int max_tiles, void* stream) {
    if (!desc || ntensors <= 0 || max_tiles <= 0) return SSD_ERR_VALUE;
    hipLaunchKernelGGL(k_weight_transpose_batched, dim3((unsigned)max_tiles, (unsigned)ntensors), dim3(256), 0, (hipStream_t)stream, desc);
    return ssd_launch_status();
}

int ssd_cast_bf16(const float* src, void* dst, long long n, void* stream) {
    if (n < 0 || (n > 0 && (!src || !dst))) return SSD_ERR_VALUE;
    if (n == 0) return SSD_OK;
    hipLaunchKernelGGL(k_cast_bf16, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                       static_cast<bf16_raw*>(dst), n);
    return ssd_launch_status();
}

int ssd_image_prep(const float* img, void* out, int B, int H, int W, int normalize, void* stream) {
    if (!img || !out || B <= 0 || H <= 0 || W <= 0) return SSD_ERR_VALUE;
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(k_image_prep, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img,
                       static_cast<bf16_raw*>(out), npix, normalize);
    return ssd_launch_status();
}

int ssd_maxpool2x2_fwd(const void* x, void* y, int B, int H, int W, int C, int Ho, int Wo, void* stream) {
    if (!x || !y || B <= 0 || C <= 0 || C % 8) return SSD_ERR_VALUE;
    if ((Ho != H / 2 && Ho != (H + 1) / 2) || (Wo != W / 2 && Wo != (W + 1) / 2) || Ho <= 0 || Wo <= 0) return SSD_ERR_VALUE;
    const long long total = (long long)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(k_maxpool_fwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const bf16_raw*>(x), static_cast<bf16_raw*>(y), B, H, W, C, Ho, Wo);
    return ssd_launch_status();
}

int ssd_maxpool2x2_fwd_argmax(const void* x, void* y, void* code, int B, int H, int W, int C, int Ho, int Wo, void* stream) {
    if (!x || !y || !code || B <= 0 || C <= 0 || C % 8) return SSD_ERR_VALUE;
    if ((Ho != H / 2 && Ho != (H + 1) / 2) || (Wo != W / 2 && Wo != (W + 1) / 2) || Ho <= 0 || Wo <= 0) return SSD_ERR_VALUE;
    const long long total = (long long)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(k_maxpool_fwd_argmax, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const bf16_raw*>(x), static_cast<bf16_raw*>(y), static_cast<unsigned*>(code), B, H, W, C, Ho, Wo);
    return ssd_launch_status();
}

int ssd_maxpool2x2_bwd_argmax(const void* code, const void* dy, void* dx, int B, int H, int W, int C, int Ho, int Wo,
                              void* stream) {
    if (!code || !dy || !dx || B <= 0 || C <= 0 || C % 8 || Ho <= 0 || Wo <= 0) return SSD_ERR_VALUE;
    if (2 * Ho < H || 2 * Wo < W) {
        // VALID pooling of an odd size leaves the last row/column without gradient: clear it first
        if (hipMemsetAsync(dx, 0, (size_t)B * H * W * C * 2, (hipStream_t)stream) != hipSuccess) return SSD_ERR_LAUNCH;
    }
    const long long total = (long long)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(k_maxpool_bwd_argmax, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned*>(code), static_cast<const bf16_raw*>(dy), static_cast<bf16_raw*>(dx), B, H, W, C,
                       Ho, Wo);
    return ssd_launch_status();
}

int ssd_maxpool2x2_bwd_argmax_accumulate(const void* code, const void* dy, void* dx, int B, int H, int W, int C, int Ho, int Wo,
                                         void* stream) {
    if (!code || !dy || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 || Ho <= 0 || Wo <= 0) return SSD_ERR_VALUE;
    const long long total = (long long)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(k_maxpool_bwd_argmax_acc, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const unsigned*>(code), static_cast<const bf16_raw*>(dy), static_cast<bf16_raw*>(dx), B, H, W, C,
                       Ho, Wo);
    return ssd_launch_status();
}

int ssd_maxpool2x2_bwd(const void* x, const void* y, const void* dy, void* dx, int B, int H, int W, int C, int Ho, int Wo,
                       void* stream) {
    if (!x || !y || !dy || !dx || B <= 0 || C % 8) return SSD_ERR_VALUE;
    if (2 * Ho < H || 2 * Wo < W) {
        // VALID pooling of an odd size leaves the last row/column without gradient: clear it first
        if (hipMemsetAsync(dx, 0, (size_t)B * H * W * C * 2, (hipStream_t)stream) != hipSuccess) return SSD_ERR_LAUNCH;
    }
    const long long total = (long long)B * Ho * Wo * (C / 8);
    hipLaunchKernelGGL(k_maxpool_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const bf16_raw*>(x), static_cast<const bf16_raw*>(y), static_cast<const bf16_raw*>(dy),
                       static_cast<bf16_raw*>(dx), B, H, W, C, Ho, Wo);
    return ssd_launch_status();
}

int ssd_head_grad_pack(const void* dloc, const void* dconf, void* out, int B, int hw, int per_cell, int classes, int npad,
                       int anchors_total, int level_off, void* stream) {
    if (!dloc || !dconf || !out || B <= 0 || hw <= 0 || npad < per_cell * (4 + classes) || npad % 8) return SSD_ERR_VALUE;
    const long long total = (long long)B * hw * (npad / 8);
    hipLaunchKernelGGL(k_head_grad_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const bf16_raw*>(dloc), static_cast<const bf16_raw*>(dconf), static_cast<bf16_raw*>(out),
                       B, hw, per_cell, classes, npad, anchors_total, level_off);
    return ssd_launch_status();
}

}  // extern "C"
