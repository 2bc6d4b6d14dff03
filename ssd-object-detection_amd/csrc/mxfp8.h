// The MX-fp8 quantisation rule of k_quant_mx_fp8 (fp8conv.hip), for the kernels that quantise their own output in the epilogue
// (k_conv_mxfp8, k_add_relu_mxfp8): a block of 32 values gets the E8M0 scale 2^e with e the smallest integer such that
// amax / 2^e <= 448 (e4m3's largest finite value), clamped to -127 .. 127 (e = 0 for an all-zero block), and its elements the
// round-to-nearest OCP e4m3 bytes of v / 2^e.  The same operations in the same order as k_quant_mx_fp8, so a fused quantisation
// equals the separate pass bit for bit.
//
// Non-finite input.  A block that holds a NaN or an infinity becomes 32 bytes 0x7F (e4m3's NaN) under the scale byte 127: it
// dequantises to NaN everywhere, and its scale byte is never 255 (E8M0's own NaN, which the matrix instruction would spread over
// the whole accumulator row without a trace of where it came from).  A diverged step so stays visible in whatever consumes the
// block, instead of turning into finite numbers.  The block maximum is therefore taken with mx_amax, IEEE 754-2019's maximum
// (v_maximum3_f32: a NaN operand gives NaN; fmaxf would drop it), so amax is finite exactly when every element is.
#pragma once

namespace {

// the running block maximum with one more element: max(amax, |v|), NaN if either is
__device__ __forceinline__ float mx_amax(float amax, float v) { return __builtin_elementwise_maximum(amax, fabsf(v)); }

// the block holds a NaN or an infinity
__device__ __forceinline__ bool mx_nonfinite(float amax) { return !(amax <= 3.4028234663852886e38f); }

// exponent e of the block scale (the stored byte is e + 127); 0 for an all-zero and for a non-finite block
__device__ __forceinline__ int mx_block_exp(float amax) {
    int e = 0;
    if (amax > 0.f && !mx_nonfinite(amax)) {
        int ex;
        const float m = frexpf(amax / 448.f, &ex);            // amax / 448 = m * 2^ex, m in [0.5, 1)
        e = (m == 0.5f) ? ex - 1 : ex;
        e = e < -127 ? -127 : (e > 127 ? 127 : e);
    }
    return e;
}

// four values (times inv = 2^-e) -> four e4m3 bytes in one word, element 0 in the lowest byte; NaN bytes for a non-finite block
__device__ __forceinline__ unsigned mx_pack4(float a, float b, float c, float d, float inv, bool nonfinite) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(a * inv, b * inv, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c * inv, d * inv, w, true);
    return nonfinite ? 0x7f7f7f7fu : (unsigned)w;
}

}  // namespace
