// 3x3 / stride 1 / pad 1 convolution FORWARD in block-scaled fp8 (OCP e4m3, one E8M0 scale per 32 channels: the MX format) on
// v_mfma_scale_f32_16x16x128_f8f6f4 -- BASELINE configs[4] ("SSD512 ... fp8 MFMA convs") for the layers with >= 256 input
// channels.  The reference has no counterpart (fp32 TensorFlow convolutions, models/ssd_model.py:86-93 for these layers): parity
// is against the fp32 restatement on the SAME dequantised operands (exact up to fp32 summation order) and, as the stated
// quantisation error, against the fp32 convolution of the bf16 operands (tests/test_fp8_gpu.py).
//
// Operand layout of the instruction, probed on the device (tools_dev/mfma_scale_layout_check.hip + the one-hot channel sweep of
// tools_dev/dbg_fp8.py): lane (gq = lane >> 4, li = lane & 15) holds row / column li; its bytes 0..15 are k = 16 gq + i, its bytes
// 16..31 are k = 64 + 16 gq + (i - 16) -- two 64-deep halves, as the bf16 instructions' k-steps -- and the scale byte of lane group s
// (selected by opsel from a 32-bit register) scales the MX block k = 32 s .. 32 s + 31, which is spread over the first halves
// of lane groups 2 (s & 1) .. +1 or their second halves.  So a lane reads 16-byte chunks gq and 4 + gq of its 128-byte row.
//
// Kernel = the 128 x 128 implicit GEMM of k_conv_igemm_dma (conv.hip) at one byte per element: a k-step is one tap x 128 channels
// (rows of 128 B, LDS-DMA with the same XOR-swizzled image, two LDS buffers, one barrier per step), the scale bytes of a step
// travel as 4-byte LDS-DMA pieces next to the tiles, one matrix instruction per 16 x 16 tile and step (bf16: two).
//
// k_conv_mxfp8 generalises that kernel to the ResNet-50 trunk's fp8 forward (resnet_engine.py, precision="mxfp8"): 1x1 and 3x3
// filters, stride 1 and 2 with TF-SAME pads, and an epilogue that writes the bf16 map, its MX-fp8 form (quantised in registers,
// bitwise ssd_quantize_mx_fp8 of that bf16 map) or both -- so the next fp8 layer is fed without a separate quantisation pass.
// Its data-gradient mode (DG) serves the trunk's stride-1 data gradients after a training-mode fp8 forward: the same main loop
// on dy and the transposed filters, an epilogue with ssd_conv2d_bwd_data's accumulate and ReLU mask.
// Its pooled mode (POOL) serves the SSD300 VGG trunk's fp8 forward (engine.py, precision="mxfp8"): block3_conv3 and the 2x2
// max pool behind it in one launch that stores the pooled map only -- the same main loop on tiles of 32 whole 2x2 windows.
// Its dilated mode (ATROUS) serves fc6 of the VGG-16 SSD300's fp8 forward (engine.py, fp8_inference=True): the same main loop
// with the tap offset times the dilation, over the taps that reach the map.
#include <algorithm>
#include "common.h"
#include <hip/hip_bf16.h>
#include "conv_common.h"
#include "mxfp8.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
__device__ __forceinline__ unsigned f8_ld4(const char* __restrict__ p, const char* __restrict__ other) { (void)other; return *reinterpret_cast<const unsigned*>(p); }

constexpr int F8_TILE = 128 * 128;           // operand tile of a k-step: 128 rows x 128 B
constexpr int F8_BUF = 2 * F8_TILE + 2 * 512;   // A | B | scales A [128][4] | scales B [128][4]
constexpr int F8_LDS = 2 * F8_BUF;           // 66 KB

// one 32-channel block per thread: scale = 2^ceil(log2(amax / 448)) as an E8M0 byte, elements = OCP e4m3 of x / scale
__global__ __launch_bounds__(256) void k_quant_mx_fp8(const bf16_raw* __restrict__ x, unsigned char* __restrict__ q,
                                                      unsigned char* __restrict__ scale, long long nblocks) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nblocks; i += (long long)gridDim.x * 256) {
        const uint4* src = reinterpret_cast<const uint4*>(x + i * 32);
        float v[32];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint4 w = src[j];
            const unsigned ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[j * 8 + 2 * k] = __uint_as_float(ws[k] << 16);
                v[j * 8 + 2 * k + 1] = __uint_as_float(ws[k] & 0xffff0000u);
            }
        }
        float amax = 0.f;                                     // the rule and its non-finite case: mxfp8.h
#pragma unroll
        for (int j = 0; j < 32; ++j) amax = mx_amax(amax, v[j]);
        const int e = mx_block_exp(amax);                     // smallest e with amax * 2^-e <= 448 (e4m3's largest finite value)
        const bool bad = mx_nonfinite(amax);
        const float inv = ldexpf(1.f, -e);
        unsigned out[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) out[j] = mx_pack4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3], inv, bad);
        uint4* dst = reinterpret_cast<uint4*>(q + i * 32);
        dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
        dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
        scale[i] = (unsigned char)(e + 127);
    }
}

__global__ __launch_bounds__(256) void k_conv3x3_mxfp8(const unsigned char* __restrict__ x, const unsigned char* __restrict__ xs,
                                                       const unsigned char* __restrict__ w, const unsigned char* __restrict__ wsc,
                                                       ConvGeom g, Epilogue ep) {
    // g: x [B,H,W,C] bytes, C % 128 == 0; w [N][9][C] bytes; xs [B*H*W][C/32], wsc [N][9][C/32] scale bytes
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave & 1, wave_n = wave >> 1;
    const int ntn = (g.N + 127) / 128;
    const int mt = blockIdx.x / ntn, n0 = (blockIdx.x % ntn) * 128, m0 = mt * 128;
    const int cb = g.C >> 5;                                  // scale bytes per pixel / per (filter, tap)
    const int csteps = g.C >> 7;                              // k-steps per tap

    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (unsigned)g.M * (unsigned)g.C, 0x00020000);
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (unsigned)g.N * 9u * (unsigned)g.C, 0x00020000);
    const __amdgpu_buffer_rsrc_t xsres = __builtin_amdgcn_make_buffer_rsrc((void*)xs, 0, (unsigned)g.M * (unsigned)cb, 0x00020000);
    const __amdgpu_buffer_rsrc_t wsres = __builtin_amdgcn_make_buffer_rsrc((void*)wsc, 0, (unsigned)g.N * 9u * (unsigned)cb, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;

    // tile pieces: instruction i (16 per operand, 4 per wave: i = wave + 4 j) covers tile rows 8i..8i+7; lane L -> row
    // 8i + 2 (L >> 4) + ((L >> 3) & 1), 16-byte chunk (L & 7) ^ ((4i + (L >> 4)) & 7)   [the image swz() reads]
    int py[4], px[4], pb[4];                                  // pixel of the staged activation row (py < 0: beyond M)
    unsigned wrow[4], cchunk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = wave + 4 * j;
        const int r = 8 * i + 2 * (lane >> 4) + ((lane >> 3) & 1);
        cchunk[j] = (unsigned)((lane & 7) ^ ((4 * i + (lane >> 4)) & 7)) * 16u;
        const int m = m0 + r;
        const bool mv = m < g.M;
        const int mm = mv ? m : 0;
        const int b = fdiv(mm, g.d_hw);
        const int rem = mm - b * g.d_hw.d;
        const int oy = fdiv(rem, g.d_w);
        py[j] = mv ? oy : -(1 << 20);
        px[j] = rem - oy * g.d_w.d;
        pb[j] = b * g.H * g.W;
        const int n = n0 + r;
        wrow[j] = n < g.N ? (unsigned)n * 9u * (unsigned)g.C : 0xffffffffu;
    }
    // scale pieces: 4 bytes per row and step; waves 0,1 bring the activation rows 64 wave + lane, waves 2,3 the filter rows
    const int srow = (wave & 1) * 64 + lane;
    int sy = 0, sx = 0, sb = 0;
    unsigned swrow = 0xffffffffu;
    if (wave < 2) {
        const int m = m0 + srow;
        const bool mv = m < g.M;
        const int mm = mv ? m : 0;
        const int b = fdiv(mm, g.d_hw);
        const int rem = mm - b * g.d_hw.d;
        const int oy = fdiv(rem, g.d_w);
        sy = mv ? oy : -(1 << 20); sx = rem - oy * g.d_w.d; sb = b * g.H * g.W;
    } else {
        const int n = n0 + srow;
        swrow = n < g.N ? (unsigned)n * 9u * (unsigned)cb : 0xffffffffu;
    }
    auto issue = [&](int step, int buf) {
        const int tap = step / csteps, cs = step - tap * csteps;
        const int kh = tap / 3 - 1, kw = tap % 3 - 1;
        char* base = smem + buf * F8_BUF;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = wave + 4 * j;
            const int iy = py[j] + kh, ix = px[j] + kw;
            const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            const unsigned off = (unsigned)(pb[j] + iy * g.W + ix) * (unsigned)g.C + (unsigned)cs * 128u + cchunk[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(base + i * 1024), 16, ok ? off : OOB, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = wave + 4 * j;
            const unsigned off = wrow[j] + (unsigned)tap * (unsigned)g.C + (unsigned)cs * 128u + cchunk[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wres, (lds_void*)(base + F8_TILE + i * 1024), 16, wrow[j] != 0xffffffffu ? off : OOB, 0, 0, 0);
        }
        if (wave < 2) {
            const int iy = sy + kh, ix = sx + kw;
            const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            const unsigned off = (unsigned)(sb + iy * g.W + ix) * (unsigned)cb + (unsigned)cs * 4u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xsres, (lds_void*)(base + 2 * F8_TILE + wave * 256), 4, ok ? off : OOB, 0, 0, 0);
        } else {
            const unsigned off = swrow + (unsigned)tap * (unsigned)cb + (unsigned)cs * 4u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wsres, (lds_void*)(base + 2 * F8_TILE + 512 + (wave - 2) * 256), 4, swrow != 0xffffffffu ? off : OOB, 0, 0, 0);
        }
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[c][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int nsteps = 9 * csteps;
    const int gq = lane >> 4, li = lane & 15;
    issue(0, 0);
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (st + 1 < nsteps) issue(st + 1, cur ^ 1);
        const char* base = smem + cur * F8_BUF;
        v8i fx[4], fw[4];
        int sxv[4], swv[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int row = wave_m * 64 + p * 16 + li;
            const uint4 lo = lds_ld16_scoped(base + swz(row, gq), smem), hi = lds_ld16_scoped(base + swz(row, 4 + gq), smem);
            fx[p] = v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            sxv[p] = (int)(f8_ld4(base + 2 * F8_TILE + row * 4, smem) >> (8 * gq));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int row = wave_n * 64 + c * 16 + li;
            const uint4 lo = lds_ld16_scoped(base + F8_TILE + swz(row, gq), smem), hi = lds_ld16_scoped(base + F8_TILE + swz(row, 4 + gq), smem);
            fw[c] = v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            swv[c] = (int)(f8_ld4(base + 2 * F8_TILE + 512 + row * 4, smem) >> (8 * gq));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                acc[c][p] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[c], fx[p], acc[c][p], 0, 0, 0, swv[c], 0, sxv[p]);
    }
    int mrow[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = m0 + wave_m * 64 + p * 16 + (lane & 15);
        mrow[p] = m < g.M ? m : -1;
    }
    conv_epilogue_rows<EPI_FWD, 4, 4>(acc, g, ep, mrow, n0 + wave_n * 64, lane);
}

// Outputs of k_conv_mxfp8: any non-empty subset of a bf16 map and its MX-fp8 form.
struct MxOut {
    const float* bias;                       // [N] or null
    int relu;
    bf16_raw* y;                             // [M][N] bf16 or null
    unsigned char* q;                        // [M][N] e4m3 or null (then qs is null too); N % 32 == 0
    unsigned char* qs;                       // [M][N/32] E8M0
    const bf16_raw* mask;                    // DG: zero where mask <= 0 ([M][N] bf16, the forward activation), or null
    int accumulate;                          // DG: y += result before the mask (y then holds the earlier gradient)
    int Mp;                                  // POOL: y / q / qs hold the 2x2 max-pooled map [B,Hp,Wp,N], Mp = B*Hp*Wp pixels
    FastDiv d_phw, d_pw;                     // POOL: divide by Hp*Wp and by Wp
    unsigned long long taps;                 // ATROUS: the live taps, four bits each (tap = 3 ty + tx), in tap order
    int ntaps, dil;                          // ATROUS: their count; the dilation (tap t reads row y + (t / 3) dil, pads = dil)
};

// The general MX-fp8 forward convolution: KS x KS filters (1 or 3), stride g.mul (1 or 2), TF-SAME pads g.pad_t / g.pad_l.  The
// main loop is k_conv3x3_mxfp8's (same staging, same k-step order tap-major, so the 3x3 / stride-1 result is bitwise the same).
// Epilogue: bias, ReLU, ONE bf16 rounding; then, for the fp8 output, the rule of k_quant_mx_fp8 on the rounded values.  A lane
// holds channels n + 4 gq .. +3 of one pixel per 16 x 16 tile, so a 32-channel block is tiles 2 cp and 2 cp + 1 of the lanes
// li, li + 16, li + 32, li + 48: the block amax is the lane's 8 values reduced over the four lane groups (two xor shuffles).
// DG = the stride-1 data gradient (ssd_conv2d_bwd_data_mxfp8): x = dy, w = the transposed filters, pads k - 1 - pad; no bias or
// ReLU, but y += result (accumulate) and then zero where mask <= 0, in ssd_conv2d_bwd_data's order, before the ONE rounding.
// POOL = the convolution followed by a 2x2 / stride-2 max pool (ssd_conv2d_fwd_pool_mxfp8): a tile is 32 whole pooling windows
// instead of 128 consecutive pixels, and the epilogue pools the bf16-rounded pixels of each window before its stores.  Every
// conv pixel still sees the same k-steps in the same order, so it is bitwise the pixel of the plain launch.
// ATROUS = the dilated 3x3 / stride-1 forward (ssd_conv2d_atrous_fwd_mxfp8): the same main loop with the tap offset times
// ep.dil and pads of ep.dil, over the live taps only -- a tap that lies outside the map for every pixel (dil >= H for a row
// of taps, dil >= W for a column) would stage zeros through the out-of-range offset and add +0 to every accumulator, so
// dropping it changes no bit.  At dil == 1 the steps are the plain launch's.
template <int KS, bool DG, bool POOL = false, bool ATROUS = false>
__global__ __launch_bounds__(256) void k_conv_mxfp8(const unsigned char* __restrict__ x, const unsigned char* __restrict__ xs,
                                                    const unsigned char* __restrict__ w, const unsigned char* __restrict__ wsc,
                                                    ConvGeom g, MxOut ep) {
    // g: x [B,H,W,C] bytes, C % 128 == 0; w [N][KS][KS][C] bytes; xs [B*H*W][C/32], wsc [N][KS][KS][C/32] scale bytes
    constexpr int KK = KS * KS;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave & 1, wave_n = wave >> 1;
    const int ntn = (g.N + 127) / 128;
    const int mt = blockIdx.x / ntn, n0 = (blockIdx.x % ntn) * 128, m0 = mt * 128;
    const int cb = g.C >> 5;
    const int csteps = g.C >> 7;
    const int stride = g.mul;
    const unsigned xbytes = (unsigned)g.B * (unsigned)g.H * (unsigned)g.W * (unsigned)g.C;     // < 2^31 (host check)

    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, xbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (unsigned)g.N * (unsigned)KK * (unsigned)g.C, 0x00020000);
    const __amdgpu_buffer_rsrc_t xsres = __builtin_amdgcn_make_buffer_rsrc((void*)xs, 0, xbytes >> 5, 0x00020000);
    const __amdgpu_buffer_rsrc_t wsres = __builtin_amdgcn_make_buffer_rsrc((void*)wsc, 0, (unsigned)g.N * (unsigned)KK * (unsigned)cb, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;

    // tile row r -> top-left input coordinate (y, x) of its output pixel's window (y < 0 far off: no pixel) and the image's
    // first pixel b0.  Plain: row r is output pixel m0 + r of the flattened [B,Ho,Wo] index.  POOL: the tile holds the pooled
    // pixels 32 mt .. 32 mt + 31 of the flattened [B,Hp,Wp] index, and row r = 64 wm + 16 p + li is member p (dy = p >> 1,
    // dx = p & 1) of window 16 wm + li -- the epilogue's lane then holds all four pixels of one window (pixel tiles p = 0..3)
    auto place = [&](int r, int& y, int& x, int& b0) {
        if constexpr (POOL) {
            const int q = mt * 32 + (r >> 6) * 16 + (r & 15), p = (r >> 4) & 3;
            const bool qv = q < ep.Mp;
            const int qq = qv ? q : 0;
            const int b = fdiv(qq, ep.d_phw);
            const int rem = qq - b * ep.d_phw.d;
            const int yp = fdiv(rem, ep.d_pw);
            const int oy = 2 * yp + (p >> 1), ox = 2 * (rem - yp * ep.d_pw.d) + (p & 1);
            y = (qv && oy < g.Ho && ox < g.Wo) ? oy * stride - g.pad_t : -(1 << 20);
            x = ox * stride - g.pad_l;
            b0 = b * g.H * g.W;
        } else {
            const int m = m0 + r;
            const bool mv = m < g.M;
            const int mm = mv ? m : 0;
            const int b = fdiv(mm, g.d_hw);
            const int rem = mm - b * g.d_hw.d;
            const int oy = fdiv(rem, g.d_w);
            y = mv ? oy * stride - g.pad_t : -(1 << 20);
            x = (rem - oy * g.d_w.d) * stride - g.pad_l;
            b0 = b * g.H * g.W;
        }
    };
    // rows as in k_conv3x3_mxfp8
    int py[4], px[4], pb[4];
    unsigned wrow[4], cchunk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = wave + 4 * j;
        const int r = 8 * i + 2 * (lane >> 4) + ((lane >> 3) & 1);
        cchunk[j] = (unsigned)((lane & 7) ^ ((4 * i + (lane >> 4)) & 7)) * 16u;
        place(r, py[j], px[j], pb[j]);
        const int n = n0 + r;
        wrow[j] = n < g.N ? (unsigned)n * (unsigned)KK * (unsigned)g.C : 0xffffffffu;
    }
    const int srow = (wave & 1) * 64 + lane;
    int sy = 0, sx = 0, sb = 0;
    unsigned swrow = 0xffffffffu;
    if (wave < 2) {
        place(srow, sy, sx, sb);
    } else {
        const int n = n0 + srow;
        swrow = n < g.N ? (unsigned)n * (unsigned)KK * (unsigned)cb : 0xffffffffu;
    }
    auto issue = [&](int step, int buf) {
        const int slot = step / csteps, cs = step - slot * csteps;
        const int tap = ATROUS ? (int)((ep.taps >> (4 * slot)) & 15ull) : slot;
        const int kh = (tap / KS) * (ATROUS ? ep.dil : 1), kw = (tap % KS) * (ATROUS ? ep.dil : 1);
        char* base = smem + buf * F8_BUF;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = wave + 4 * j;
            const int iy = py[j] + kh, ix = px[j] + kw;
            const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            const unsigned off = (unsigned)(pb[j] + iy * g.W + ix) * (unsigned)g.C + (unsigned)cs * 128u + cchunk[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(base + i * 1024), 16, ok ? off : OOB, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = wave + 4 * j;
            const unsigned off = wrow[j] + (unsigned)tap * (unsigned)g.C + (unsigned)cs * 128u + cchunk[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wres, (lds_void*)(base + F8_TILE + i * 1024), 16, wrow[j] != 0xffffffffu ? off : OOB, 0, 0, 0);
        }
        if (wave < 2) {
            const int iy = sy + kh, ix = sx + kw;
            const bool ok = (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            const unsigned off = (unsigned)(sb + iy * g.W + ix) * (unsigned)cb + (unsigned)cs * 4u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xsres, (lds_void*)(base + 2 * F8_TILE + wave * 256), 4, ok ? off : OOB, 0, 0, 0);
        } else {
            const unsigned off = swrow + (unsigned)tap * (unsigned)cb + (unsigned)cs * 4u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wsres, (lds_void*)(base + 2 * F8_TILE + 512 + (wave - 2) * 256), 4, swrow != 0xffffffffu ? off : OOB, 0, 0, 0);
        }
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[c][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int nsteps = (ATROUS ? ep.ntaps : KK) * csteps;
    const int gq = lane >> 4, li = lane & 15;
    issue(0, 0);
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (st + 1 < nsteps) issue(st + 1, cur ^ 1);
        const char* base = smem + cur * F8_BUF;
        v8i fx[4], fw[4];
        int sxv[4], swv[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int row = wave_m * 64 + p * 16 + li;
            const uint4 lo = lds_ld16_scoped(base + swz(row, gq), smem), hi = lds_ld16_scoped(base + swz(row, 4 + gq), smem);
            fx[p] = v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            sxv[p] = (int)(f8_ld4(base + 2 * F8_TILE + row * 4, smem) >> (8 * gq));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int row = wave_n * 64 + c * 16 + li;
            const uint4 lo = lds_ld16_scoped(base + F8_TILE + swz(row, gq), smem), hi = lds_ld16_scoped(base + F8_TILE + swz(row, 4 + gq), smem);
            fw[c] = v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            swv[c] = (int)(f8_ld4(base + 2 * F8_TILE + 512 + row * 4, smem) >> (8 * gq));
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                acc[c][p] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[c], fx[p], acc[c][p], 0, 0, 0, swv[c], 0, sxv[p]);
    }

    const int ldq = g.N >> 5;
    if constexpr (POOL) {
        // epilogue: bias, ReLU, ONE bf16 rounding per conv pixel; the max over the window's pixels inside the conv map, in
        // k_maxpool_fwd's order (dy, then dx: tiles p = 0..3); then the pooled pixel's stores and quantisation as below
        const int q = mt * 32 + wave_m * 16 + li;
        const bool qv = q < ep.Mp;
        bool in[4];
        {
            const int qq = qv ? q : 0;
            const int b = fdiv(qq, ep.d_phw);
            const int rem = qq - b * ep.d_phw.d;
            const int yp = fdiv(rem, ep.d_pw), xp = rem - yp * ep.d_pw.d;
#pragma unroll
            for (int p = 0; p < 4; ++p) in[p] = 2 * yp + (p >> 1) < g.Ho && 2 * xp + (p & 1) < g.Wo;
        }
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {
            const int nblk = n0 + wave_n * 64 + cp * 32;
            if (nblk >= g.N) continue;                        // wave-uniform (N % 32 == 0: the whole block lies inside N)
            float v[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = nblk + h * 16 + gq * 4;
                float b4[4] = {0.f, 0.f, 0.f, 0.f};
                if (ep.bias) {
                    const float4 bv = *reinterpret_cast<const float4*>(ep.bias + n);
                    b4[0] = bv.x; b4[1] = bv.y; b4[2] = bv.z; b4[3] = bv.w;
                }
                float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    float t[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        t[j] = acc[2 * cp + h][p][j] + b4[j];
                        if (ep.relu) t[j] = fmaxf(t[j], 0.f);
                    }
                    const unsigned lo = pack_bf16x2(t[0], t[1]), hi = pack_bf16x2(t[2], t[3]);
                    const float r[4] = {__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
                                        __uint_as_float(hi & 0xffff0000u)};
                    if (in[p]) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) best[j] = fmaxf(best[j], r[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) v[4 * h + j] = best[j];
                if (ep.y && qv)                               // bf16 values already: the packing is exact
                    *reinterpret_cast<uint2*>(ep.y + (long long)q * g.N + n) = make_uint2(pack_bf16x2(best[0], best[1]),
                                                                                           pack_bf16x2(best[2], best[3]));
            }
            if (ep.q) {
                float amax = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) amax = mx_amax(amax, v[j]);
                amax = mx_amax(amax, __shfl_xor(amax, 16));
                amax = mx_amax(amax, __shfl_xor(amax, 32));
                const int e = mx_block_exp(amax);
                const bool bad = mx_nonfinite(amax);
                const float inv = ldexpf(1.f, -e);
                if (qv) {
                    unsigned char* o = ep.q + (long long)q * g.N + nblk + gq * 4;
                    *reinterpret_cast<unsigned*>(o) = mx_pack4(v[0], v[1], v[2], v[3], inv, bad);
                    *reinterpret_cast<unsigned*>(o + 16) = mx_pack4(v[4], v[5], v[6], v[7], inv, bad);
                    if (gq == 0) ep.qs[(long long)q * ldq + (nblk >> 5)] = (unsigned char)(e + 127);
                }
            }
        }
        return;
    }
    // epilogue: per pixel tile p and channel block cp (tiles 2 cp, 2 cp + 1); the block test is wave-uniform, so every lane
    // of the wave takes part in the shuffles (lanes beyond M compute and discard)
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int m = m0 + wave_m * 64 + p * 16 + li;
        const bool mv = m < g.M;
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {
            const int nblk = n0 + wave_n * 64 + cp * 32;
            if (nblk >= g.N) continue;
            float v[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = nblk + h * 16 + gq * 4;
                float b4[4] = {0.f, 0.f, 0.f, 0.f};
                if (ep.bias) {
                    if (n + 3 < g.N) {
                        const float4 bv = *reinterpret_cast<const float4*>(ep.bias + n);
                        b4[0] = bv.x; b4[1] = bv.y; b4[2] = bv.z; b4[3] = bv.w;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) if (n + j < g.N) b4[j] = ep.bias[n + j];
                    }
                }
                float t[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    t[j] = acc[2 * cp + h][p][j] + b4[j];
                    if (ep.relu) t[j] = fmaxf(t[j], 0.f);
                }
                if constexpr (DG) {                           // N % 32 == 0: n + 3 < N
                    if (mv && ep.accumulate) {                // two gradients meet at this map
                        const uint2 old = *reinterpret_cast<const uint2*>(ep.y + (long long)m * g.N + n);
                        t[0] += __uint_as_float(old.x << 16); t[1] += __uint_as_float(old.x & 0xffff0000u);
                        t[2] += __uint_as_float(old.y << 16); t[3] += __uint_as_float(old.y & 0xffff0000u);
                    }
                    if (mv && ep.mask) {                      // ReLU backward: zero where the forward activation was <= 0
                        const uint2 mk = *reinterpret_cast<const uint2*>(ep.mask + (long long)m * g.N + n);
                        if (!(__uint_as_float(mk.x << 16) > 0.f)) t[0] = 0.f;
                        if (!(__uint_as_float(mk.x & 0xffff0000u) > 0.f)) t[1] = 0.f;
                        if (!(__uint_as_float(mk.y << 16) > 0.f)) t[2] = 0.f;
                        if (!(__uint_as_float(mk.y & 0xffff0000u) > 0.f)) t[3] = 0.f;
                    }
                }
                const unsigned lo = pack_bf16x2(t[0], t[1]), hi = pack_bf16x2(t[2], t[3]);
                v[4 * h] = __uint_as_float(lo << 16); v[4 * h + 1] = __uint_as_float(lo & 0xffff0000u);
                v[4 * h + 2] = __uint_as_float(hi << 16); v[4 * h + 3] = __uint_as_float(hi & 0xffff0000u);
                if (ep.y && mv && n < g.N) {
                    bf16_raw* o = ep.y + (long long)m * g.N + n;
                    if (n + 3 < g.N) {
                        *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);
                    } else {
                        const bf16_raw e4[4] = {(bf16_raw)(lo & 0xffffu), (bf16_raw)(lo >> 16), (bf16_raw)(hi & 0xffffu), (bf16_raw)(hi >> 16)};
#pragma unroll
                        for (int j = 0; j < 4; ++j) if (n + j < g.N) o[j] = e4[j];
                    }
                }
            }
            if (ep.q) {                                       // N % 32 == 0: the whole block lies inside N
                float amax = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) amax = mx_amax(amax, v[j]);
                amax = mx_amax(amax, __shfl_xor(amax, 16));
                amax = mx_amax(amax, __shfl_xor(amax, 32));
                const int e = mx_block_exp(amax);
                const bool bad = mx_nonfinite(amax);
                const float inv = ldexpf(1.f, -e);
                if (mv) {
                    unsigned char* o = ep.q + (long long)m * g.N + nblk + gq * 4;
                    *reinterpret_cast<unsigned*>(o) = mx_pack4(v[0], v[1], v[2], v[3], inv, bad);
                    *reinterpret_cast<unsigned*>(o + 16) = mx_pack4(v[4], v[5], v[6], v[7], inv, bad);
                    if (gq == 0) ep.qs[(long long)m * ldq + (nblk >> 5)] = (unsigned char)(e + 127);
                }
            }
        }
    }
}

OnceLds g_f8_once;
OnceLds g_f8g_once[2];
OnceLds g_f8d_once[2];
OnceLds g_f8p_once;
OnceLds g_f8a_once;

}  // namespace

extern "C" {

int ssd_quantize_mx_fp8(const void* x_bf16, void* q, void* scale, long long n, void* stream) {
    if (!x_bf16 || !q || !scale || n <= 0 || (n & 31)) return SSD_ERR_VALUE;
    const long long nb = n / 32;
    const long long gridl = (nb + 255) / 256;
    hipLaunchKernelGGL(k_quant_mx_fp8, dim3((unsigned)(gridl > 16384 ? 16384 : gridl)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const bf16_raw*>(x_bf16), static_cast<unsigned char*>(q), static_cast<unsigned char*>(scale), nb);
    return ssd_launch_status();
}

int ssd_conv3x3_fwd_mxfp8(const void* x8, const void* xscale, const void* w8, const void* wscale, const float* bias, void* y, int B,
                          int H, int W, int Cin, int Cout, int relu, void* stream) {
    if (!x8 || !xscale || !w8 || !wscale || !y || B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return SSD_ERR_VALUE;
    if (Cin % 128 || Cout % 8) return SSD_ERR_UNSUPPORTED;
    if ((long long)B * H * W * Cin >= (1ll << 31) || (long long)Cout * 9 * Cin >= (1ll << 31)) return SSD_ERR_UNSUPPORTED;
    const ConvGeom g = make_geom(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, 1, 1);
    Epilogue ep = {};
    ep.bias = bias; ep.relu = relu; ep.out = static_cast<bf16_raw*>(y); ep.ldo = Cout;
    if (ensure_lds(g_f8_once, reinterpret_cast<const void*>(k_conv3x3_mxfp8), F8_LDS) != 0) return SSD_ERR_LAUNCH;
    const unsigned grid = (unsigned)(((g.M + 127) / 128) * ((Cout + 127) / 128));
    hipLaunchKernelGGL(k_conv3x3_mxfp8, dim3(grid), dim3(256), F8_LDS, (hipStream_t)stream, static_cast<const unsigned char*>(x8),
                       static_cast<const unsigned char*>(xscale), static_cast<const unsigned char*>(w8),
                       static_cast<const unsigned char*>(wscale), g, ep);
    return ssd_launch_status();
}

int ssd_conv2d_fwd_mxfp8(const void* x8, const void* xscale, const void* w8, const void* wscale, const float* bias, void* y_bf16,
                         void* y8, void* yscale, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad_t, int pad_l,
                         int Ho, int Wo, int relu, void* stream) {
    if (!x8 || !xscale || !w8 || !wscale) return SSD_ERR_VALUE;
    if ((!y_bf16 && !y8) || (!y8 != !yscale)) return SSD_ERR_VALUE;             // no output, or q without its scales
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 || pad_t < 0 || pad_l < 0) return SSD_ERR_VALUE;
    if (Cin % 128 || (k != 1 && k != 3) || (stride != 1 && stride != 2) || Cout % 8 || (y8 && Cout % 32)) return SSD_ERR_UNSUPPORTED;
    if (pad_t >= k || pad_l >= k || (Ho - 1) * stride - pad_t >= H || (Wo - 1) * stride - pad_l >= W) return SSD_ERR_VALUE;
    if ((long long)B * H * W * Cin >= (1ll << 31) || (long long)Cout * k * k * Cin >= (1ll << 31) ||
        (long long)B * Ho * Wo * Cout * 2 >= (1ll << 31))
        return SSD_ERR_UNSUPPORTED;
    const ConvGeom g = make_geom(B, H, W, Cin, Ho, Wo, Cout, k, k, stride, 1, pad_t, pad_l);
    MxOut ep = {};
    ep.bias = bias; ep.relu = relu; ep.y = static_cast<bf16_raw*>(y_bf16);
    ep.q = static_cast<unsigned char*>(y8); ep.qs = static_cast<unsigned char*>(yscale);
    const void* fn = k == 1 ? reinterpret_cast<const void*>(k_conv_mxfp8<1, false>) : reinterpret_cast<const void*>(k_conv_mxfp8<3, false>);
    if (ensure_lds(g_f8g_once[k == 1 ? 0 : 1], fn, F8_LDS) != 0) return SSD_ERR_LAUNCH;
    const unsigned grid = (unsigned)(((g.M + 127) / 128) * ((Cout + 127) / 128));
    const auto* xp = static_cast<const unsigned char*>(x8);
    const auto* xsp = static_cast<const unsigned char*>(xscale);
    const auto* wp = static_cast<const unsigned char*>(w8);
    const auto* wsp = static_cast<const unsigned char*>(wscale);
    if (k == 1)
        hipLaunchKernelGGL((k_conv_mxfp8<1, false>), dim3(grid), dim3(256), F8_LDS, (hipStream_t)stream, xp, xsp, wp, wsp, g, ep);
    else
        hipLaunchKernelGGL((k_conv_mxfp8<3, false>), dim3(grid), dim3(256), F8_LDS, (hipStream_t)stream, xp, xsp, wp, wsp, g, ep);
    return ssd_launch_status();
}

int ssd_conv2d_fwd_pool_mxfp8(const void* x8, const void* xscale, const void* w8, const void* wscale, const float* bias,
                              void* y_pool_bf16, void* y_pool8, void* y_pool_scale, int B, int H, int W, int Cin, int Cout, int k,
                              int stride, int pad_t, int pad_l, int Ho, int Wo, int relu, int Hp, int Wp, void* stream) {
    if (!x8 || !xscale || !w8 || !wscale) return SSD_ERR_VALUE;
    if ((!y_pool_bf16 && !y_pool8) || (!y_pool8 != !y_pool_scale)) return SSD_ERR_VALUE;    // no output, or q without its scales
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 || pad_t < 0 || pad_l < 0) return SSD_ERR_VALUE;
    if ((Hp != Ho / 2 && Hp != (Ho + 1) / 2) || (Wp != Wo / 2 && Wp != (Wo + 1) / 2) || Hp <= 0 || Wp <= 0) return SSD_ERR_VALUE;
    if (Cin % 128 || k != 3 || stride != 1 || Cout % 32) return SSD_ERR_UNSUPPORTED;
    if (pad_t >= k || pad_l >= k || (Ho - 1) * stride - pad_t >= H || (Wo - 1) * stride - pad_l >= W) return SSD_ERR_VALUE;
    if ((long long)B * H * W * Cin >= (1ll << 31) || (long long)Cout * k * k * Cin >= (1ll << 31) ||
        (long long)B * Ho * Wo * Cout * 2 >= (1ll << 31))
        return SSD_ERR_UNSUPPORTED;
    const ConvGeom g = make_geom(B, H, W, Cin, Ho, Wo, Cout, k, k, stride, 1, pad_t, pad_l);
    MxOut ep = {};
    ep.bias = bias; ep.relu = relu; ep.y = static_cast<bf16_raw*>(y_pool_bf16);
    ep.q = static_cast<unsigned char*>(y_pool8); ep.qs = static_cast<unsigned char*>(y_pool_scale);
    ep.Mp = B * Hp * Wp;
    ep.d_phw = make_fastdiv(Hp * Wp);
    ep.d_pw = make_fastdiv(Wp);
    if (ensure_lds(g_f8p_once, reinterpret_cast<const void*>(k_conv_mxfp8<3, false, true>), F8_LDS) != 0) return SSD_ERR_LAUNCH;
    const unsigned grid = (unsigned)(((ep.Mp + 31) / 32) * ((Cout + 127) / 128));         // 32 pooling windows per tile
    hipLaunchKernelGGL((k_conv_mxfp8<3, false, true>), dim3(grid), dim3(256), F8_LDS, (hipStream_t)stream,
                       static_cast<const unsigned char*>(x8), static_cast<const unsigned char*>(xscale),
                       static_cast<const unsigned char*>(w8), static_cast<const unsigned char*>(wscale), g, ep);
    return ssd_launch_status();
}

int ssd_conv2d_atrous_fwd_mxfp8(const void* x8, const void* xscale, const void* w8, const void* wscale, const float* bias,
                                void* y_bf16, void* y8, void* yscale, int B, int H, int W, int Cin, int Cout, int dilation, int relu,
                                void* stream) {
    if (!x8 || !xscale || !w8 || !wscale) return SSD_ERR_VALUE;
    if ((!y_bf16 && !y8) || (!y8 != !yscale)) return SSD_ERR_VALUE;             // no output, or q without its scales
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || dilation < 1) return SSD_ERR_VALUE;
    if (Cin % 128 || Cout % 8 || (y8 && Cout % 32)) return SSD_ERR_UNSUPPORTED;
    if ((long long)B * H * W * Cin >= (1ll << 31) || (long long)Cout * 9 * Cin >= (1ll << 31) ||
        (long long)B * H * W * Cout * 2 >= (1ll << 31))
        return SSD_ERR_UNSUPPORTED;
    const int dil = std::min(dilation, std::max(H, W));      // beyond the map only the centre tap is live, whatever the dilation
    const ConvGeom g = make_geom(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, dil, dil);
    MxOut ep = {};
    ep.bias = bias; ep.relu = relu; ep.y = static_cast<bf16_raw*>(y_bf16);
    ep.q = static_cast<unsigned char*>(y8); ep.qs = static_cast<unsigned char*>(yscale);
    ep.dil = dil;
    for (int ty = 0; ty < 3; ++ty)                           // the live taps, as live_taps() of atrous.hip
        for (int tx = 0; tx < 3; ++tx) {
            if ((ty != 1 && dil >= H) || (tx != 1 && dil >= W)) continue;
            ep.taps |= (unsigned long long)(3 * ty + tx) << (4 * ep.ntaps);
            ++ep.ntaps;
        }
    if (ensure_lds(g_f8a_once, reinterpret_cast<const void*>(k_conv_mxfp8<3, false, false, true>), F8_LDS) != 0) return SSD_ERR_LAUNCH;
    const unsigned grid = (unsigned)(((g.M + 127) / 128) * ((Cout + 127) / 128));
    hipLaunchKernelGGL((k_conv_mxfp8<3, false, false, true>), dim3(grid), dim3(256), F8_LDS, (hipStream_t)stream,
                       static_cast<const unsigned char*>(x8), static_cast<const unsigned char*>(xscale),
                       static_cast<const unsigned char*>(w8), static_cast<const unsigned char*>(wscale), g, ep);
    return ssd_launch_status();
}

int ssd_conv2d_bwd_data_mxfp8(const void* dy8, const void* dyscale, const void* wt8, const void* wtscale, const void* relu_src,
                              void* dx_bf16, void* dx8, void* dxscale, int B, int H, int W, int Cin, int Cout, int k, int pad_t,
                              int pad_l, int Ho, int Wo, int accumulate, void* stream) {
    if (!dy8 || !dyscale || !wt8 || !wtscale) return SSD_ERR_VALUE;
    if ((!dx_bf16 && !dx8) || (!dx8 != !dxscale) || (accumulate && !dx_bf16)) return SSD_ERR_VALUE;
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 || pad_t < 0 || pad_l < 0) return SSD_ERR_VALUE;
    if (Cout % 128 || Cin % 32 || (k != 1 && k != 3)) return SSD_ERR_UNSUPPORTED;
    // the forward implicit GEMM on dy [B,Ho,Wo,Cout] with the transposed filters and the mirrored pads, output [B,H,W,Cin]
    const int qt = k - 1 - pad_t, ql = k - 1 - pad_l;
    if (qt < 0 || ql < 0 || H - 1 - qt >= Ho || W - 1 - ql >= Wo) return SSD_ERR_VALUE;
    if ((long long)B * Ho * Wo * Cout >= (1ll << 31) || (long long)Cin * k * k * Cout >= (1ll << 31) ||
        (long long)B * H * W * Cin * 2 >= (1ll << 31))
        return SSD_ERR_UNSUPPORTED;
    const ConvGeom g = make_geom(B, Ho, Wo, Cout, H, W, Cin, k, k, 1, 1, qt, ql);
    MxOut ep = {};
    ep.y = static_cast<bf16_raw*>(dx_bf16);
    ep.q = static_cast<unsigned char*>(dx8); ep.qs = static_cast<unsigned char*>(dxscale);
    ep.mask = static_cast<const bf16_raw*>(relu_src); ep.accumulate = accumulate;
    const void* fn = k == 1 ? reinterpret_cast<const void*>(k_conv_mxfp8<1, true>) : reinterpret_cast<const void*>(k_conv_mxfp8<3, true>);
    if (ensure_lds(g_f8d_once[k == 1 ? 0 : 1], fn, F8_LDS) != 0) return SSD_ERR_LAUNCH;
    const unsigned grid = (unsigned)(((g.M + 127) / 128) * ((Cin + 127) / 128));
    const auto* xp = static_cast<const unsigned char*>(dy8);
    const auto* xsp = static_cast<const unsigned char*>(dyscale);
    const auto* wp = static_cast<const unsigned char*>(wt8);
    const auto* wsp = static_cast<const unsigned char*>(wtscale);
    if (k == 1)
        hipLaunchKernelGGL((k_conv_mxfp8<1, true>), dim3(grid), dim3(256), F8_LDS, (hipStream_t)stream, xp, xsp, wp, wsp, g, ep);
    else
        hipLaunchKernelGGL((k_conv_mxfp8<3, true>), dim3(grid), dim3(256), F8_LDS, (hipStream_t)stream, xp, xsp, wp, wsp, g, ep);
    return ssd_launch_status();
}

}  // extern "C"
