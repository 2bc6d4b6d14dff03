// The MX-fp8 quantisation rule of k_quant_mx_fp8 (fp8conv.hip), for the kernels that quantise their own output in the epilogue
// (k_conv_mxfp8, k_add_relu_mxfp8): a block of 32 values gets the E8M0 scale 2^e with e the smallest integer such that
// amax / 2^e <= 448 (e4m3's largest finite value), and its elements the round-to-nearest OCP e4m3 bytes of v / 2^e.  The same
// operations in the same order as k_quant_mx_fp8, so a fused quantisation equals the separate pass bit for bit.
#pragma once

namespace {

// exponent e of the block scale (the stored byte is e + 127)
__device__ __forceinline__ int mx_block_exp(float amax) {
    int e = 0;
    if (amax > 0.f) {
        int ex;
        const float m = frexpf(amax / 448.f, &ex);            // amax / 448 = m * 2^ex, m in [0.5, 1)
        e = (m == 0.5f) ? ex - 1 : ex;
        e = e < -127 ? -127 : (e > 127 ? 127 : e);
    }
    return e;
}

// four values (times inv = 2^-e) -> four e4m3 bytes in one word, element 0 in the lowest byte
__device__ __forceinline__ unsigned mx_pack4(float a, float b, float c, float d, float inv) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c * inv, d * inv, w, true);
    return (unsigned)w;
}

}  // namespace
