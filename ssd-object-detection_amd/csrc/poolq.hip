// Quantising max poolings of the VGG-16 SSD300's inference fp8 forward (engine.py, fp8_inference=True): pool4 (2x2 / stride 2)
// and pool5 (3x3 / stride 1) read a bf16 map and write the pooled map as an MX-fp8 pair, so the fp8 convolution behind them is
// fed without a bf16 round trip and a separate quantisation pass.  No reference counterpart (fp32 TensorFlow layers); defined
// bit for bit as ssd_quantize_mx_fp8 of the bf16 pooling's map:
//   k_maxpool_mxfp8<2>   ssd_maxpool2x2_fwd   (k_maxpool_fwd, conv_aux.hip: windows clipped at the bottom / right edge, fmaxf)
//   k_maxpool_mxfp8<3>   ssd_maxpool3x3s1_fwd (k_maxpool3x3s1_fwd, atrous.hip: pad 1, the first maximum in window order)
// The maximum is taken on the bf16 values (a pooled value is one of them: no rounding), then the rule of mxfp8.h on the pooled
// values -- a NaN input is dropped by either maximum as in the bf16 poolings, an infinity that wins makes its block non-finite.
// No winner codes: inference only.  One thread per output pixel and 8 channels, 16 bytes per load; a 32-channel block is four
// neighbouring lanes (C % 32 == 0 and 256 threads per block: a group is in or out of the loop together), its amax two xor
// shuffles, as k_add_relu_mxfp8.
#include "common.h"
#include <hip/hip_bf16.h>
#include "mxfp8.h"

namespace {

typedef unsigned short bf16_raw;

template <int KS>
__global__ __launch_bounds__(256) void k_maxpool_mxfp8(const bf16_raw* __restrict__ x, bf16_raw* __restrict__ y,
                                                       uint2* __restrict__ q, unsigned char* __restrict__ scale, int B, int H, int W,
                                                       int C, int Ho, int Wo) {
    const int c8 = C >> 3;
    const long long total = (long long)B * Ho * Wo * c8;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int cc = (int)(idx % c8);
        long long r = idx / c8;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int b = (int)(r / Ho);
        float best[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) best[k] = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < KS; ++dy)
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) {
                const int iy = KS == 2 ? 2 * oy + dy : oy - 1 + dy, ix = KS == 2 ? 2 * ox + dx : ox - 1 + dx;
                if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
                const uint4 v = *reinterpret_cast<const uint4*>(x + (((long long)b * H + iy) * W + ix) * C + cc * 8);
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float f = (k & 1) ? __uint_as_float(w[k >> 1] & 0xffff0000u) : __uint_as_float(w[k >> 1] << 16);
                    if constexpr (KS == 2) best[k] = fmaxf(best[k], f);
                    else if (f > best[k]) best[k] = f;
                }
            }
        if (y) {
            unsigned o4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o4[k] = (__float_as_uint(best[2 * k]) >> 16) | (__float_as_uint(best[2 * k + 1]) & 0xffff0000u);
            *reinterpret_cast<uint4*>(y + idx * 8) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
        }
        float amax = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) amax = mx_amax(amax, best[k]);
        amax = mx_amax(amax, __shfl_xor(amax, 1));
        amax = mx_amax(amax, __shfl_xor(amax, 2));
        const int e = mx_block_exp(amax);
        const bool bad = mx_nonfinite(amax);
        const float inv = ldexpf(1.f, -e);
        q[idx] = make_uint2(mx_pack4(best[0], best[1], best[2], best[3], inv, bad), mx_pack4(best[4], best[5], best[6], best[7], inv, bad));
        if ((idx & 3) == 0) scale[idx >> 2] = (unsigned char)(e + 127);
    }
}

inline unsigned grid_for(long long items) {
    const long long g = (items + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

inline bool overlaps(const void* a, long long abytes, const void* b, long long bbytes) {
    if (!a || !b) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

template <int KS>
int launch(const void* x, void* y, void* q, void* scale, int B, int H, int W, int C, int Ho, int Wo, void* stream) {
    if (!x || !q || !scale || B < 1 || H < 1 || W < 1 || C < 1 || Ho < 1 || Wo < 1) return SSD_ERR_VALUE;
    if (C % 32) return SSD_ERR_UNSUPPORTED;
    const long long nin = (long long)B * H * W * C, nout = (long long)B * Ho * Wo * C;
    if (nin >= (1ll << 31)) return SSD_ERR_UNSUPPORTED;
    if (overlaps(y, nout * 2, x, nin * 2) || overlaps(q, nout, x, nin * 2) || overlaps(scale, nout / 32, x, nin * 2) ||
        overlaps(q, nout, y, nout * 2) || overlaps(scale, nout / 32, y, nout * 2) || overlaps(scale, nout / 32, q, nout))
        return SSD_ERR_VALUE;
    hipLaunchKernelGGL(k_maxpool_mxfp8<KS>, dim3(grid_for(nout >> 3)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const bf16_raw*>(x), static_cast<bf16_raw*>(y), static_cast<uint2*>(q),
                       static_cast<unsigned char*>(scale), B, H, W, C, Ho, Wo);
    return ssd_launch_status();
}

}  // namespace

extern "C" {

int ssd_maxpool2x2_fwd_mxfp8(const void* x, void* y_bf16, void* q, void* scale, int B, int H, int W, int C, int Ho, int Wo,
                             void* stream) {
    if (H < 1 || W < 1 || (Ho != H / 2 && Ho != (H + 1) / 2) || (Wo != W / 2 && Wo != (W + 1) / 2)) return SSD_ERR_VALUE;
    return launch<2>(x, y_bf16, q, scale, B, H, W, C, Ho, Wo, stream);
}

int ssd_maxpool3x3s1_fwd_mxfp8(const void* x, void* y_bf16, void* q, void* scale, int B, int H, int W, int C, void* stream) {
    return launch<3>(x, y_bf16, q, scale, B, H, W, C, H, W, stream);
}

}  // extern "C"
