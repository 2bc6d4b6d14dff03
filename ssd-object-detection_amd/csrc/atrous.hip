// Atrous (dilated) 3x3 convolution and 3x3 / stride-1 max pooling for gfx950 (MI355X): the two operators of the SSD paper's
// VGG-16 trunk that the reference does not have (it truncates VGG-16 at block3 and has no dilation) -- `pool5` (3x3, stride 1)
// and the dilated `fc6` (3x3, dilation 6, 512 -> 1024 on the 19x19 map).  Semantics: Keras Conv2D(3, dilation_rate=d,
// padding="same"), MaxPooling2D(3, strides=1, padding="same") and their tape.gradient.  No network launches them yet.
//
// Forward and data gradient are ONE implicit-GEMM kernel (k_atrous_igemm): rows are the B*H*W pixels, columns the output
// channels; a dilated 3x3 is nine 1x1 GEMMs on shifted rows that accumulate into one tile.  Per tap a row's source is
// `row + constant`; a row whose source lies outside its own image (a tile spans image boundaries whenever H*W does not divide
// 128) gets an offset beyond the buffer descriptor's range, for which the LDS-DMA writes zeros without a branch (the idiom of
// PW_OOB in pwgemm.hip).  Taps that are dead for the whole map (d >= H or d >= W) are dropped on the host: the reduction walks
// live taps x ceil(K / 64) chunks only.  With symmetric padding the data gradient is the same convolution of dy with the
// transposed, flipped filters of ssd_weight_transpose.
// Tile 128 px x 128 ch x 64 k, four waves (2 x 2, 64 x 64 each: 16 accumulator tiles), the LDS image, DMA ownership and the
// one-barrier double buffer of k_conv_igemm_dma (conv.hip); the store stage is conv_common.h's staged epilogue.
//
// The weight gradient (k_atrous_wgrad) is k_conv_wgrad's 128 x 128 GEMM over pixels with tap-shifted rows of x, over the LIVE
// (tap, ci) columns only; slabs over the pixel axis are summed in a fixed order by k_atrous_wgrad_reduce, which also writes the
// zeros of the dead taps.  dbias is the column sum of dy from the same pass (an MFMA against ones).  No atomics anywhere.
#include <algorithm>
#include <cstdint>
#include "common.h"
#include <hip/hip_bf16.h>
#include "conv_common.h"

namespace {

constexpr int AT_BM = 128, AT_BN = 128, AT_NT = 256;
constexpr int AT_BUF = (AT_BM + AT_BN) * 128;    // one k-step: 128 rows x 64 k bf16 of either operand (32 KB)
constexpr int AT_LDS = 2 * AT_BUF;               // 64 KB: two workgroups per CU
constexpr unsigned AT_OOB = 0x80000000u;         // beyond every descriptor (operands are below 2^31 bytes): zeros

// The live taps of a call, four bits each (tap = 3 ty + tx), in tap order.
struct AtrousTaps {
    unsigned long long packed;
    int n;
};

inline AtrousTaps live_taps(int H, int W, int d) {
    AtrousTaps t{0ull, 0};
    for (int ty = 0; ty < 3; ++ty)
        for (int tx = 0; tx < 3; ++tx) {
            if ((ty != 1 && d >= H) || (tx != 1 && d >= W)) continue;
            t.packed |= (unsigned long long)(3 * ty + tx) << (4 * t.n);
            ++t.n;
        }
    return t;
}

// g: source [B,H,W,C = K] and destination [B,H,W,N]; w rows of g.ldw = 9 K elements, tap-major.  dil: min(dilation, max(H, W)).
template <int EPI>
__global__ __launch_bounds__(AT_NT) void k_atrous_igemm(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ w, ConvGeom g,
                                                        Epilogue ep, AtrousTaps taps, int dil) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    auto s_x = [&](int buf) { return smem + buf * AT_BUF; };
    auto s_w = [&](int buf) { return smem + buf * AT_BUF + AT_BM * 128; };

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave & 1, wave_n = wave >> 1;
    // XCD-aware tile order, as k_conv_igemm_dma: the channel tiles of one pixel tile are consecutive on one XCD
    const int ntn = (g.N + AT_BN - 1) / AT_BN, ntm = (g.M + AT_BM - 1) / AT_BM;
    const int kx = blockIdx.x >> 3;
    const int mt = (kx / ntn) * 8 + (blockIdx.x & 7);
    if (mt >= ntm) return;
    const int m0 = mt * AT_BM, n0 = (kx % ntn) * AT_BN;
    const int K = g.C;
    const unsigned rowb = (unsigned)K * 2u;

    // DMA ownership: wave-instruction i = (wave & 1) + 2 * ((wave >> 1) + 2 j) covers tile rows 8i .. 8i+7;
    // lane L -> row 8i + 2 (L >> 4) + ((L >> 3) & 1), chunk (L & 7) ^ ((row >> 1) & 7)   [the image swz() reads]
    const int rl = 2 * (lane >> 4) + ((lane >> 3) & 1);
    const int slot = (lane & 7) ^ (4 * (wave & 1) + (lane >> 4));
    int mpix[4];                                // the row's output pixel
    unsigned vmask[4];                          // bit t: tap t of the row reads inside its own image
    unsigned wrow[4];                           // byte offset of the weight row, ~0u beyond N
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = (wave & 1) + 2 * ((wave >> 1) + 2 * j);
        const int m = m0 + 8 * i + rl;
        mpix[j] = m;
        vmask[j] = 0u;
        if (m < g.M) {
            const int b = fdiv(m, g.d_hw);
            const int rem = m - b * g.d_hw.d;
            const int oy = fdiv(rem, g.d_w), ox = rem - oy * g.d_w.d;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = oy + (t / 3 - 1) * dil, ix = ox + (t % 3 - 1) * dil;
                if ((unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W) vmask[j] |= 1u << t;
            }
        }
        const int n = n0 + 8 * i + rl;
        wrow[j] = n < g.N ? (unsigned)n * (unsigned)g.ldw * 2u : ~0u;
    }
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (unsigned)g.M * rowb, 0x00020000);
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (unsigned)g.N * (unsigned)g.ldw * 2u, 0x00020000);

    const int KT = (K + 63) >> 6;               // k-chunks per tap; the last one may be partial (K % 8 == 0)
    int ti = 0, kc = 0;                         // the step the next issue stages
    auto issue_dma = [&](int buf) {
        const int t = (int)((taps.packed >> (4 * ti)) & 15ull);
        const int ty = t / 3, tx = t - 3 * ty;
        const int delta = ((ty - 1) * g.W + (tx - 1)) * dil;            // source pixel = row pixel + delta (same image when valid)
        const int k = kc * 64 + slot * 8;
        const bool kvalid = k < K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = (wave & 1) + 2 * ((wave >> 1) + 2 * j);
            const bool ok = kvalid && ((vmask[j] >> t) & 1u);
            const unsigned off = (unsigned)(mpix[j] + delta) * rowb + (unsigned)k * 2u;
            dma16_buf(xres, s_x(buf) + i * 1024, ok ? off : AT_OOB);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = (wave & 1) + 2 * ((wave >> 1) + 2 * j);
            const bool ok = kvalid && wrow[j] != ~0u;
            dma16_buf(wres, s_w(buf) + i * 1024, ok ? wrow[j] + (unsigned)(t * K + k) * 2u : AT_OOB);
        }
        if (++kc == KT) { kc = 0; ++ti; }
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[c][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nks = taps.n * KT;
    issue_dma(0);
    const int frow = lane & 15, fk = lane >> 4;
    for (int ks = 0; ks < nks; ++ks) {
        const int cur = ks & 1;
        // step ks has landed everywhere and everybody is done reading step ks - 1, whose buffer the next issue refills
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (ks + 1 < nks) issue_dma(cur ^ 1);
#pragma unroll
        for (int ksub = 0; ksub < 2; ++ksub) {
            bf16x8_t fx[4], fw[4];
#pragma unroll
            for (int p = 0; p < 4; ++p)
                fx[p] = *reinterpret_cast<const bf16x8_t*>(s_x(cur) + swz(wave_m * 64 + p * 16 + frow, ksub * 4 + fk));
#pragma unroll
            for (int c = 0; c < 4; ++c)
                fw[c] = *reinterpret_cast<const bf16x8_t*>(s_w(cur) + swz(wave_n * 64 + c * 16 + frow, ksub * 4 + fk));
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[c], fx[p], acc[c][p], 0, 0, 0);
        }
    }
    // (no DMA is in flight: the last step issued none; the staged epilogue opens with a barrier)
    auto row_to_m = [&](int row) { return m0 + row < g.M ? m0 + row : -1; };
    staged_epilogue<EPI, AT_BM, AT_BN, 4, 4, AT_NT>(acc, smem, g, ep, n0, wave_m * 64, wave_n * 64, tid, row_to_m);
}

// ------------------------------------------------------------------------------------------------
// Weight gradient: k_conv_wgrad's block (conv_wgrad.hip) with tap-shifted rows.  grid (column tiles, co tiles, pixel splits);
// columns are the live taps' (tap, ci) pairs, ncols = taps.n * Cin; per step 64 pixels, staged through registers, read back
// with transposing LDS reads.  slab_w [split][Cout][ncols], slab_b [split][Cout] (null: no bias gradient).
constexpr int AW_LD = 288;                       // LDS row stride (bytes) of a [pixel][128 ch] tile: 256 + 32 pad
constexpr int AW_TILE = 64 * AW_LD;
constexpr int AW_LDS = 4 * AW_TILE;              // two buffers x (dy, x): 72 KB

__global__ __launch_bounds__(256) void k_atrous_wgrad(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ dy,
                                                      float* __restrict__ slab_w, float* __restrict__ slab_b, int M, int H, int W,
                                                      int Cin, int Cout, int ldy, FastDiv d_hw, FastDiv d_w, AtrousTaps taps, int dil,
                                                      int m_per_split) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    auto s_dy = [&](int buf) { return smem + buf * (2 * AW_TILE); };
    auto s_x = [&](int buf) { return smem + buf * (2 * AW_TILE) + AW_TILE; };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_m = wave & 1, wave_n = wave >> 1;       // m: co, n: (tap, ci) columns
    const int col0 = blockIdx.x * 128, co0 = blockIdx.y * 128;
    const int cpt = Cin >> 3;
    const int ncols = taps.n * Cin;
    const int m_begin = blockIdx.z * m_per_split;
    const int m_end = min(M, m_begin + m_per_split);

    const int cslot = tid & 15, prow = tid >> 4;           // 16-byte column chunk, pixel row (+16j)
    const int qx = (col0 >> 3) + cslot;                     // this thread's column chunk -> (live tap, channel)
    const bool xcol_ok = qx < taps.n * cpt;
    const int tapi = xcol_ok ? qx / cpt : 0;
    const int ccx = qx - tapi * cpt;
    const int tap = (int)((taps.packed >> (4 * tapi)) & 15ull);
    const int sy = (tap / 3 - 1) * dil, sx = (tap % 3 - 1) * dil;
    const int co_chunk = co0 + cslot * 8;
    const bool dycol_ok = co_chunk < Cout;

    uint4 rdy[4], rxx[4];
    auto load_tiles = [&](int mstep) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = mstep + prow + 16 * j;
            const bool mok = m < m_end;
            rdy[j] = make_uint4(0, 0, 0, 0);
            rxx[j] = make_uint4(0, 0, 0, 0);
            if (mok && dycol_ok) rdy[j] = *reinterpret_cast<const uint4*>(dy + ((long long)m * ldy + co_chunk));
            if (mok && xcol_ok) {
                const int b = fdiv(m, d_hw);
                const int rem = m - b * d_hw.d;
                const int oy = fdiv(rem, d_w);
                const int ox = rem - oy * d_w.d;
                const int iy = oy + sy, ix = ox + sx;
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                    rxx[j] = *reinterpret_cast<const uint4*>(x + ((((long long)b * H + iy) * W + ix) * Cin + ccx * 8));
            }
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<uint4*>(s_dy(buf) + (prow + 16 * j) * AW_LD + cslot * 16) = rdy[j];
            *reinterpret_cast<uint4*>(s_x(buf) + (prow + 16 * j) * AW_LD + cslot * 16) = rxx[j];
        }
    };

    f32x4_t acc[4][4];
    f32x4_t accb[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        accb[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = slab_b != nullptr && blockIdx.x == 0 && wave_n == 0;
    bf16x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;

    const int nsteps = (m_end - m_begin + 63) / 64;
    if (nsteps > 0) {
        load_tiles(m_begin);
        store_tiles(0);
    }
    __syncthreads();
    // transposing read: lane (16-group gq, index i) supplies the address of k-row (i >> 2), columns 4 (i & 3) .. +3
    const int gq = lane >> 4, li = lane & 15;
    const int tr_row = li >> 2, tr_col = (li & 3) * 4;
    for (int st = 0; st < nsteps; ++st) {
        const int cur = st & 1;
        const bool more = st + 1 < nsteps;
        if (more) load_tiles(m_begin + (st + 1) * 64);
#pragma unroll
        for (int ksub = 0; ksub < 2; ++ksub) {
            bf16x8_t fa[4], fb[4];
            const int krow = ksub * 32 + gq * 8 + tr_row;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const char* base = s_dy(cur) + krow * AW_LD + (wave_m * 64 + a * 16 + tr_col) * 2;
                union { s16x4_t h[2]; bf16x8_t v; } u;
                u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base));
                u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + 4 * AW_LD));
                fa[a] = u.v;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const char* base = s_x(cur) + krow * AW_LD + (wave_n * 64 + c * 16 + tr_col) * 2;
                union { s16x4_t h[2]; bf16x8_t v; } u;
                u.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base));
                u.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + 4 * AW_LD));
                fb[c] = u.v;
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb[c], acc[a][c], 0, 0, 0);
            if (do_bias) {
#pragma unroll
                for (int a = 0; a < 4; ++a) accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], ones, accb[a], 0, 0, 0);
            }
        }
        if (more) store_tiles(cur ^ 1);
        __syncthreads();
    }
    // partial tile -> slab[z][co][col]  (D[row = co (lane >> 4) * 4 + j][col = lane & 15])
    float* out = slab_w + (long long)blockIdx.z * Cout * ncols;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = col0 + wave_n * 64 + c * 16 + (lane & 15);
            if (col >= ncols) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + wave_m * 64 + a * 16 + (lane >> 4) * 4 + j;
                if (co < Cout) out[(long long)co * ncols + col] = acc[a][c][j];
            }
        }
    if (do_bias && (lane & 15) == 0) {
        float* ob = slab_b + (long long)blockIdx.z * Cout;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + wave_m * 64 + a * 16 + (lane >> 4) * 4 + j;
                if (co < Cout) ob[co] = accb[a][j];
            }
    }
}

// dw [Cout][9][Cin] = sum over the splits, in split order, of the live taps' slab columns; dead taps: zeros.  Blocks
// [0, nbw): four elements of dw per thread; the blocks behind them: dbias.
__global__ __launch_bounds__(256) void k_atrous_wgrad_reduce(const float* __restrict__ slab_w, const float* __restrict__ slab_b,
                                                             float* __restrict__ dw, float* __restrict__ db, int Cin, int Cout,
                                                             AtrousTaps taps, int ns, unsigned nbw) {
    const int ncols = taps.n * Cin;
    if (blockIdx.x < nbw) {
        const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
        if (i >= (long long)Cout * 9 * Cin) return;
        const int co = (int)(i / (9 * Cin));
        const int r = (int)(i - (long long)co * 9 * Cin);
        const int t = r / Cin, c = r - t * Cin;
        int li = -1;
        for (int k = 0; k < taps.n; ++k)
            if ((int)((taps.packed >> (4 * k)) & 15ull) == t) li = k;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (li >= 0) {
            const float* p = slab_w + (long long)co * ncols + li * Cin + c;
            for (int z = 0; z < ns; ++z) {
                const float4 v = *reinterpret_cast<const float4*>(p + (long long)z * Cout * ncols);
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
        }
        *reinterpret_cast<float4*>(dw + i) = s;
    } else {
        const int i = (int)(blockIdx.x - nbw) * 256 + threadIdx.x;
        if (i >= Cout) return;
        float s = 0.f;
        for (int z = 0; z < ns; ++z) s += slab_b[(long long)z * Cout + i];
        db[i] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 max pooling: k_maxpool3x3s2_fwd / _bwd (eltwise.hip) at stride 1, same code convention (one nibble per
// element = 3 dy + dx of the FIRST maximum in window order, 15 = the maximum is <= 0).  One thread per pixel and 8 channels.
__global__ __launch_bounds__(256) void k_maxpool3x3s1_fwd(const bf16_raw* __restrict__ x, bf16_raw* __restrict__ y,
                                                          unsigned* __restrict__ code, int B, int H, int W, int C) {
    const int c8 = C >> 3;
    const long long total = (long long)B * H * W * c8;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int cc = (int)(idx % c8);
        long long r = idx / c8;
        const int ox = (int)(r % W); r /= W;
        const int oy = (int)(r % H);
        const int b = (int)(r / H);
        float best[8];
        unsigned pos[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { best[k] = -INFINITY; pos[k] = 15u; }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iy = oy - 1 + dy, ix = ox - 1 + dx;
                if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
                const uint4 v = *reinterpret_cast<const uint4*>(x + (((long long)b * H + iy) * W + ix) * C + cc * 8);
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const float f = (k & 1) ? __uint_as_float(w[k >> 1] & 0xffff0000u) : __uint_as_float(w[k >> 1] << 16);
                    if (f > best[k]) { best[k] = f; pos[k] = (unsigned)(3 * dy + dx); }
                }
            }
        unsigned o4[4], cw = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) o4[k] = (__float_as_uint(best[2 * k]) >> 16) | (__float_as_uint(best[2 * k + 1]) & 0xffff0000u);
#pragma unroll
        for (int k = 0; k < 8; ++k) cw |= (best[k] > 0.f ? pos[k] : 15u) << (4 * k);
        *reinterpret_cast<uint4*>(y + idx * 8) = make_uint4(o4[0], o4[1], o4[2], o4[3]);
        code[idx] = cw;
    }
}

// Backward: every input pixel belongs to up to nine windows, so the gradient is GATHERED per input pixel -- dx[p] = sum of dy
// over the windows whose recorded winner is p, in window order, in fp32, rounded once: deterministic, no atomics.
__global__ __launch_bounds__(256) void k_maxpool3x3s1_bwd(const unsigned* __restrict__ code, const bf16_raw* __restrict__ dy,
                                                          bf16_raw* __restrict__ dx, int B, int H, int W, int C) {
    const int c8 = C >> 3;
    const long long total = (long long)B * H * W * c8;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
        const int cc = (int)(idx % c8);
        long long r = idx / c8;
        const int ix = (int)(r % W); r /= W;
        const int iy = (int)(r % H);
        const int b = (int)(r / H);
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int oy = max(iy - 1, 0); oy <= min(iy + 1, H - 1); ++oy)
            for (int ox = max(ix - 1, 0); ox <= min(ix + 1, W - 1); ++ox) {
                const unsigned me = (unsigned)(3 * (iy - oy + 1) + (ix - ox + 1));
                const long long o = (((long long)b * H + oy) * W + ox) * c8 + cc;
                const unsigned cw = code[o];
                const uint4 g = *reinterpret_cast<const uint4*>(dy + o * 8);
                const unsigned w[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (((cw >> (4 * k)) & 15u) != me) continue;
                    acc[k] += (k & 1) ? __uint_as_float(w[k >> 1] & 0xffff0000u) : __uint_as_float(w[k >> 1] << 16);
                }
            }
        *reinterpret_cast<uint4*>(dx + idx * 8) = make_uint4(pack_bf16x2(acc[0], acc[1]), pack_bf16x2(acc[2], acc[3]),
                                                             pack_bf16x2(acc[4], acc[5]), pack_bf16x2(acc[6], acc[7]));
    }
}

// ------------------------------------------------------------------------------------------------
// Host side
inline unsigned grid_for(long long items) {
    const long long g = (items + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

inline bool overlaps(const void* a, long long abytes, const void* b, long long bbytes) {
    if (!a || !b) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// SSD_OK, or why the GEMM form [M = B H W][K] x [N][9 K] is not served.  The DMA streams address either operand with 31-bit
// byte offsets (AT_OOB must lie beyond both descriptors, a tile's overhang included).
int igemm_serves(int B, int H, int W, int K, int N) {
    const long long M = (long long)B * H * W;
    if ((M + AT_BM) * K * 2 >= (1ll << 31) || ((long long)N + AT_BN) * 9 * K * 2 >= (1ll << 31) || M * N * 2 >= (1ll << 31))
        return SSD_ERR_UNSUPPORTED;
    return SSD_OK;
}

template <int EPI>
int launch_igemm(const void* x, const void* w, const Epilogue& ep, int B, int H, int W, int K, int N, int dilation, void* stream) {
    const int dil = std::min(dilation, std::max(H, W));                  // beyond the map only the centre tap is live, whatever d
    const ConvGeom g = make_geom(B, H, W, K, H, W, N, 3, 3, 1, 1, dil, dil);
    const AtrousTaps taps = live_taps(H, W, dil);
    const int ntm = (g.M + AT_BM - 1) / AT_BM, ntn = (N + AT_BN - 1) / AT_BN;
    const unsigned grid = (unsigned)((ntm + 7) / 8 * 8 * ntn);
    auto kern = k_atrous_igemm<EPI>;
    static OnceLds once;
    if (ensure_lds(once, reinterpret_cast<const void*>(kern), AT_LDS) != 0) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(AT_NT), AT_LDS, (hipStream_t)stream, static_cast<const bf16_raw*>(x),
                       static_cast<const bf16_raw*>(w), g, ep, taps, dil);
    return ssd_launch_status();
}

// Pixel splits of the weight gradient, by a cost model of the launch: two workgroups fit a CU (72 KB of LDS each), so
// tiles x splits workgroups run in rounds of 512; a 64-pixel step of a round was measured at ~1.5 us on fc6's shape, and a
// split's slab is written and read once at ~4 TB/s.  Splits of whole steps, at least 256 pixels each; the first minimum wins.
// A function of the shape alone: the workspace query and the call agree.
struct WgradSplit { int ns, per_split, ctiles, mtiles, ntaps; };
WgradSplit wgrad_split(int B, int H, int W, int Cin, int Cout, int dilation) {
    WgradSplit s;
    const long long M = (long long)B * H * W;
    s.ntaps = live_taps(H, W, std::min(dilation, std::max(H, W))).n;
    s.ctiles = (s.ntaps * Cin + 127) / 128;
    s.mtiles = (Cout + 127) / 128;
    const long long tiles = (long long)s.ctiles * s.mtiles;
    const long long slab_ns = ((long long)Cout * s.ntaps * Cin * 4 * 2) / 4000;      // one split's slab, written and read
    const long long most = std::min<long long>((M + 255) / 256, 64);
    long long best = -1;
    s.ns = 1;
    s.per_split = (int)((M + 63) / 64 * 64);
    for (long long want = 1; want <= most; ++want) {
        const long long per = ((M + want - 1) / want + 63) / 64 * 64;
        const long long ns = (M + per - 1) / per;
        const long long cost = (tiles * ns + 511) / 512 * (per / 64) * 1500 + ns * slab_ns;
        if (best < 0 || cost < best) { best = cost; s.ns = (int)ns; s.per_split = (int)per; }
    }
    return s;
}

int wgrad_serves(int B, int H, int W, int Cin, int Cout, int ldy) {
    if (Cin % 64 || Cout % 8 || ldy < Cout || ldy % 8) return SSD_ERR_UNSUPPORTED;
    const long long M = (long long)B * H * W;
    if (M * Cin * 2 >= (1ll << 31) || M * ldy * 2 >= (1ll << 31) || (long long)Cout * 9 * Cin >= (1ll << 31)) return SSD_ERR_UNSUPPORTED;
    return SSD_OK;
}

size_t wgrad_ws_bytes(const WgradSplit& s, int Cin, int Cout) {
    return (size_t)s.ns * ((size_t)Cout * s.ntaps * Cin + (size_t)Cout) * sizeof(float);
}

}  // namespace

extern "C" {

int ssd_conv2d_atrous_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                          int dilation, int relu, void* stream) {
    if (!x || !w || !y || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || dilation < 1) return SSD_ERR_VALUE;
    if (Cin % 64 || Cout % 8) return SSD_ERR_UNSUPPORTED;
    if (igemm_serves(B, H, W, Cin, Cout) != SSD_OK) return SSD_ERR_UNSUPPORTED;
    const long long M = (long long)B * H * W, ybytes = M * Cout * 2;
    if (overlaps(y, ybytes, x, M * Cin * 2) || overlaps(y, ybytes, w, (long long)Cout * 9 * Cin * 2) ||
        overlaps(y, ybytes, bias, (long long)Cout * 4))
        return SSD_ERR_VALUE;
    Epilogue ep = {};
    ep.bias = bias;
    ep.relu = relu;
    ep.out = static_cast<bf16_raw*>(y);
    ep.ldo = Cout;
    return launch_igemm<EPI_FWD>(x, w, ep, B, H, W, Cin, Cout, dilation, stream);
}

int ssd_conv2d_atrous_bwd_data(const void* dy, const void* w_t, const void* relu_src, void* dx, int B, int H, int W, int Cin,
                               int Cout_pad, int dilation, int accumulate, void* stream) {
    if (!dy || !w_t || !dx || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout_pad < 1 || dilation < 1) return SSD_ERR_VALUE;
    if (Cin % 64 || Cout_pad % 8) return SSD_ERR_UNSUPPORTED;
    if (igemm_serves(B, H, W, Cout_pad, Cin) != SSD_OK) return SSD_ERR_UNSUPPORTED;
    const long long M = (long long)B * H * W, dxbytes = M * Cin * 2;
    if (overlaps(dx, dxbytes, dy, M * Cout_pad * 2) || overlaps(dx, dxbytes, w_t, (long long)Cin * 9 * Cout_pad * 2)) return SSD_ERR_VALUE;
    Epilogue ep = {};
    ep.out = static_cast<bf16_raw*>(dx);
    ep.ldo = Cin;
    ep.mask_src = static_cast<const bf16_raw*>(relu_src);      // (may be dx itself: a chunk is read before it is stored)
    ep.accumulate = accumulate ? 1 : 0;
    return launch_igemm<EPI_DGRAD>(dy, w_t, ep, B, H, W, Cout_pad, Cin, dilation, stream);
}

size_t ssd_conv2d_atrous_bwd_weight_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ldy, int dilation) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || dilation < 1 || (long long)B * H * W >= (1ll << 31)) return 0;
    if (wgrad_serves(B, H, W, Cin, Cout, ldy) != SSD_OK) return 0;
    return wgrad_ws_bytes(wgrad_split(B, H, W, Cin, Cout, dilation), Cin, Cout);
}

int ssd_conv2d_atrous_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, int B, int H, int W, int Cin, int Cout,
                                 int ldy, int dilation, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !dy || !dw || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || dilation < 1 || (long long)B * H * W >= (1ll << 31))
        return SSD_ERR_VALUE;
    if (wgrad_serves(B, H, W, Cin, Cout, ldy) != SSD_OK) return SSD_ERR_UNSUPPORTED;
    const long long M = (long long)B * H * W, dwbytes = (long long)Cout * 9 * Cin * 4;
    if (overlaps(dw, dwbytes, x, M * Cin * 2) || overlaps(dw, dwbytes, dy, M * ldy * 2) || overlaps(dbias, (long long)Cout * 4, x, M * Cin * 2) ||
        overlaps(dbias, (long long)Cout * 4, dy, M * ldy * 2) || overlaps(dbias, (long long)Cout * 4, dw, dwbytes))
        return SSD_ERR_VALUE;
    const WgradSplit sp = wgrad_split(B, H, W, Cin, Cout, dilation);
    const size_t need = wgrad_ws_bytes(sp, Cin, Cout);
    if (!ws || ws_bytes < need) return SSD_ERR_WORKSPACE;
    const int dil = std::min(dilation, std::max(H, W));
    const AtrousTaps taps = live_taps(H, W, dil);
    float* slab_w = static_cast<float*>(ws);
    float* slab_b = slab_w + (size_t)sp.ns * Cout * taps.n * Cin;
    hipStream_t s = (hipStream_t)stream;
    static OnceLds once;
    if (ensure_lds(once, reinterpret_cast<const void*>(k_atrous_wgrad), AW_LDS) != 0) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_atrous_wgrad, dim3(sp.ctiles, sp.mtiles, sp.ns), dim3(256), AW_LDS, s, static_cast<const bf16_raw*>(x),
                       static_cast<const bf16_raw*>(dy), slab_w, dbias ? slab_b : nullptr, (int)M, H, W, Cin, Cout, ldy,
                       make_fastdiv(H * W), make_fastdiv(W), taps, dil, sp.per_split);
    if (hipGetLastError() != hipSuccess) return SSD_ERR_LAUNCH;
    const unsigned nbw = (unsigned)(((long long)Cout * 9 * Cin / 4 + 255) / 256), nbb = dbias ? (unsigned)((Cout + 255) / 256) : 0u;
    hipLaunchKernelGGL(k_atrous_wgrad_reduce, dim3(nbw + nbb), dim3(256), 0, s, slab_w, slab_b, dw, dbias, Cin, Cout, taps, sp.ns, nbw);
    return ssd_launch_status();
}

int ssd_maxpool3x3s1_fwd(const void* x, void* y, void* code, int B, int H, int W, int C, void* stream) {
    if (!x || !y || !code || B < 1 || H < 1 || W < 1 || C < 1) return SSD_ERR_VALUE;
    if (C % 8) return SSD_ERR_UNSUPPORTED;
    const long long n = (long long)B * H * W * C;
    if (n >= (1ll << 31)) return SSD_ERR_UNSUPPORTED;
    if (overlaps(y, n * 2, x, n * 2) || overlaps(code, n / 2, x, n * 2) || overlaps(y, n * 2, code, n / 2)) return SSD_ERR_VALUE;
    hipLaunchKernelGGL(k_maxpool3x3s1_fwd, dim3(grid_for(n >> 3)), dim3(256), 0, (hipStream_t)stream, static_cast<const bf16_raw*>(x),
                       static_cast<bf16_raw*>(y), static_cast<unsigned*>(code), B, H, W, C);
    return ssd_launch_status();
}

int ssd_maxpool3x3s1_bwd(const void* code, const void* dy, void* dx, int B, int H, int W, int C, void* stream) {
    if (!code || !dy || !dx || B < 1 || H < 1 || W < 1 || C < 1) return SSD_ERR_VALUE;
    if (C % 8) return SSD_ERR_UNSUPPORTED;
    const long long n = (long long)B * H * W * C;
    if (n >= (1ll << 31)) return SSD_ERR_UNSUPPORTED;
    if (overlaps(dx, n * 2, dy, n * 2) || overlaps(dx, n * 2, code, n / 2)) return SSD_ERR_VALUE;
    hipLaunchKernelGGL(k_maxpool3x3s1_bwd, dim3(grid_for(n >> 3)), dim3(256), 0, (hipStream_t)stream, static_cast<const unsigned*>(code),
                       static_cast<const bf16_raw*>(dy), static_cast<bf16_raw*>(dx), B, H, W, C);
    return ssd_launch_status();
}

}  // extern "C"
