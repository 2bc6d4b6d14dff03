// Convolution stack for gfx950 (MI355X): NHWC bf16 implicit-GEMM convolutions on MFMA, forward and data gradient.
//
// Replaces the TensorFlow kernels behind SSDObjectDetectionModel._build (models/ssd_model.py:74-171)
// and their autodiff (tape.gradient, :248): Conv2D 3x3/1x1 (+bias, +ReLU) forward and data gradient.  TF "SAME" padding is
// asymmetric for stride 2 (pad_before = pad_total/2, the remainder after) and is passed explicitly as (pad_t, pad_l).
//
// Kernels (DESIGN.md section 4 has the table): k_conv3x3_patch32 / k_conv3x3_p512 (3x3 with the halo patch in LDS),
// k_conv3x3_c64b (64 -> 64; its W0 form also produces the first layer's weight gradient), k_conv0_fwd (image layer),
// k_conv_igemm_8ph / k_conv_igemm_dma (implicit GEMM, split-K through k_igemm_finalize).  The dispatch (igemm_plan decides, launch_igemm launches)
// and the C entries are at the end of the file.  The weight gradient is conv_wgrad.hip; pooling, weight transposes, casts and the
// head-gradient packing are conv_aux.hip; the development knobs are knobs.hip.
#include <atomic>
#include <cstdint>
#include <type_traits>
#include "common.h"
#include <hip/hip_bf16.h>
#include <stdlib.h>

#include "conv_common.h"
namespace {

// split-K finalize: out = epilogue(sum over splits of slab[split][m][n..n+3] + bias)
template <int EPI>
__global__ void k_igemm_finalize(ConvGeom g, Epilogue ep) {
    const int n4 = (g.N + 3) >> 2;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)g.M * n4) return;
    const int m = (int)(idx / n4), n = (int)(idx - (long long)m * n4) * 4;
    const bool full = n + 3 < g.N;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (full && !(g.N & 3)) {                     // 16-byte aligned slab rows: one load per split (same order of additions)
        for (int z = 0; z < ep.ksplit; ++z) {
            const float4 t = *reinterpret_cast<const float4*>(ep.slab + ((long long)z * g.M + m) * g.N + n);
            v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w;
        }
    } else {
        for (int z = 0; z < ep.ksplit; ++z) {
            const float* sl = ep.slab + ((long long)z * g.M + m) * g.N + n;
#pragma unroll
            for (int j = 0; j < 4; ++j) if (n + j < g.N) v[j] += sl[j];
        }
    }
    if constexpr (EPI != EPI_DGRAD) {
        float b4[4];
        load_bias4(ep, n, g.N, false, b4);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += b4[j];
    }
    epi_store<EPI>(v, m, n, full, g, ep);
}

// ------------------------------------------------------------------------------------------------
// Implicit GEMM, LDS-DMA version: tiles go global -> LDS directly (global_load_lds_dwordx4: per-lane
// gather address, wave-uniform 1 KiB LDS destination, no VGPR staging, no ds_write).  The swizzled LDS
// image is produced by choosing which chunk each lane fetches: wave-instruction i fills bank rows
// 4i..4i+3 = tile rows 8i..8i+7; lane L owns slot L of that KiB.  Padding / out-of-range chunks are
// fetched from a 16-byte zero block (g_zero16, conv_common.h).  Schedule per k-step (two LDS buffers, ONE barrier):
//   wait vmcnt(0) + barrier  -> tile ks has landed everywhere and everybody is done reading tile ks-1
//   issue the DMA of tile ks+1 into the other buffer (in flight during this step's MFMAs)
//   read fragments of tile ks, 64 MFMAs.
template <int BM, int BN, int EPI, int PT>
__global__ __launch_bounds__((BM / (16 * PT)) * (BN >= 128 ? BN / 64 : 2) * 64) void k_conv_igemm_dma(
    const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ w, ConvGeom g, Epilogue ep) {
    constexpr int WAVES_M = BM / (16 * PT);     // wave tile: 16*PT pixels x 16*CT channels
    constexpr int WAVES_N = BN >= 128 ? BN / 64 : 2;
    constexpr int NW = WAVES_M * WAVES_N;       // waves per workgroup (4, 8 or 16)
    constexpr int CT = BN / (16 * WAVES_N);     // 16-wide channel tiles per wave (4, or 2 for BN = 64)
    constexpr int XI = BM / 8 / NW;             // activation DMA instructions per wave per k-step
    constexpr int WI = BN / 8 / NW;             // weight DMA instructions per wave per k-step
    static_assert(XI >= 1 && WI >= 1, "tile too small for the wave count");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    auto s_x = [&](int buf) { return smem + buf * ((BM + BN) * 128); };
    auto s_w = [&](int buf) { return smem + buf * ((BM + BN) * 128) + BM * 128; };

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave % WAVES_M, wave_n = wave / WAVES_M;
    // XCD-aware tile order: workgroup L runs on XCD L % 8 (round-robin dispatch); the N-tiles of one pixel tile are
    // consecutive on ONE XCD so that the gathered activation tile is fetched into that XCD's L2 once.
    const int ntn = (g.N + BN - 1) / BN;
    int ntm = (g.M + BM - 1) / BM;
    if (g.s2) ntm = (g.cls_n[0] + BM - 1) / BM + (g.cls_n[1] + BM - 1) / BM + (g.cls_n[2] + BM - 1) / BM + (g.cls_n[3] + BM - 1) / BM;
    const int kx = blockIdx.x >> 3;
    const int mt = (kx / ntn) * 8 + (blockIdx.x & 7);
    if (mt >= ntm) return;
    int m0 = mt * BM;
    const int n0 = (kx % ntn) * BN;
    // parity class of this tile (stride-2 data gradient only)
    int cls = 0, cls_count = g.M, cls_py = 0, cls_px = 0, cls_hw = 1, cls_wd = 1;
    if (g.s2) {
        int t0 = 0;
        for (cls = 0; cls < 3; ++cls) {
            const int ntc = (g.cls_n[cls] + BM - 1) / BM;
            if (mt < t0 + ntc) break;
            t0 += ntc;
        }
        m0 = (mt - t0) * BM;
        cls_count = g.cls_n[cls];
        cls_py = cls >> 1; cls_px = cls & 1;
        cls_wd = g.cls_w[cls_px];
        cls_hw = g.cls_h[cls_py] * cls_wd;
    }
    // destination pixel (b, oy, ox) of tile-local row index m (class-local when s2)
    auto decode = [&](int m, int& bb, int& oy, int& ox) {
        if (g.s2) {
            bb = m / cls_hw;
            const int rem = m - bb * cls_hw;
            const int a = rem / cls_wd;
            oy = 2 * a + cls_py;
            ox = 2 * (rem - a * cls_wd) + cls_px;
        } else {
            bb = fdiv(m, g.d_hw);
            const int rem = m - bb * g.d_hw.d;
            oy = fdiv(rem, g.d_w);
            ox = rem - oy * g.d_w.d;
        }
    };

    // DMA ownership: wave-instruction i = (wave&1) + 2*((wave>>1) + (NW/2)*j) covers tile rows 8i..8i+7 (i has the
    // wave's parity, so a lane fetches the same k-chunk for all of its rows);
    // lane L -> row 8i + 2*(L>>4) + ((L>>3)&1), chunk (L&7) ^ ((row>>1)&7) = (L&7) ^ (4*(wave&1) + (L>>4))
    const int rl = 2 * (lane >> 4) + ((lane >> 3) & 1);
    const int slot = (lane & 7) ^ (4 * (wave & 1) + (lane >> 4));
    // per staged row: (ybase, xbase) = source coordinate of tap (0,0) times div, rowpix = flat source pixel of it
    // (div == 1).  An invalid row gets ybase far outside so that every tap fails the range test.
    int ybase[XI], xbase[XI], ibase[XI];
#pragma unroll
    for (int j = 0; j < XI; ++j) {
        const int i = (wave & 1) + 2 * ((wave >> 1) + (NW / 2) * j);
        const int m = m0 + 8 * i + rl;
        const bool mv = m < cls_count;
        int b, oy, ox;
        decode(mv ? m : 0, b, oy, ox);
        ybase[j] = mv ? oy * g.mul - g.pad_t : -(1 << 20);
        xbase[j] = ox * g.mul - g.pad_l;
        ibase[j] = b * g.H * g.W;              // < 2^31 (checked on the host)
    }
    unsigned wrow[WI];                          // element offset of the weight row, ~0u if out of range (weights < 4G elements)
#pragma unroll
    for (int j = 0; j < WI; ++j) {
        const int i = (wave & 1) + 2 * ((wave >> 1) + (NW / 2) * j);
        const int n = n0 + 8 * i + rl;
        wrow[j] = n < g.N ? (unsigned)n * (unsigned)g.ldw : ~0u;
    }
    int tap = slot / g.cpt, cc = slot - tap * g.cpt;
    int kh = tap / g.KW, kw = tap - kh * g.KW;
    int q = slot;
    const int dmask = g.div - 1, dshift = g.div > 1 ? 1 : 0;   // div is 1 or 2

    // Tensors below 4 GB (every layer of the SSD networks): LDS-DMA through buffer descriptors -- 32-bit byte offsets, a lane
    // whose chunk is padding / out of range gets an offset beyond the buffer (the hardware writes zeros).  The 64-bit
    // per-lane address form below it (global_load_lds) moves the same bytes 4-5 % slower (measured on the weight-gradient patch
    // kernel, round 3) and remains for larger tensors.
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, g.dma32 ? (unsigned)g.B * g.H * g.W * g.C * 2u : 0u, 0x00020000);
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, g.dma32 ? (unsigned)g.N * (unsigned)g.ldw * 2u : 0u, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    auto issue_dma = [&](int buf) {
        const bool kvalid = q < g.nchunks;
#pragma unroll
        for (int j = 0; j < XI; ++j) {
            const int i = (wave & 1) + 2 * ((wave >> 1) + (NW / 2) * j);
            const int ny = ybase[j] + kh, nx = xbase[j] + kw;
            const int iy = ny >> dshift, ix = nx >> dshift;
            // unsigned compares fold the >= 0 tests; the element offset fits 32 bits (tensor < 4G elements, host check)
            const bool ok = kvalid && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W && (((ny | nx) & dmask) == 0);
            const unsigned off = (unsigned)(ibase[j] + iy * g.W + ix) * (unsigned)g.C + (unsigned)(cc * 8);
            if (g.dma32) {
                dma16_buf(xres, s_x(buf) + i * 1024, ok ? off * 2u : OOB);
            } else {
                const bf16_raw* src = ok ? x + off : reinterpret_cast<const bf16_raw*>(g_zero16);
                __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(s_x(buf) + i * 1024), 16, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < WI; ++j) {
            const int i = (wave & 1) + 2 * ((wave >> 1) + (NW / 2) * j);
            const bool wok = kvalid && wrow[j] != ~0u;
            if (g.dma32) {
                dma16_buf(wres, s_w(buf) + i * 1024, wok ? (wrow[j] + (unsigned)(q * 8)) * 2u : OOB);
            } else {
                const bf16_raw* src = wok ? w + (wrow[j] + (unsigned)(q * 8)) : reinterpret_cast<const bf16_raw*>(g_zero16);
                __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(s_w(buf) + i * 1024), 16, 0, 0);
            }
        }
        q += 8;
        cc += 8;
        while (cc >= g.cpt) {
            cc -= g.cpt;
            if (++kw == g.KW) { kw = 0; ++kh; }
        }
    };

    f32x4_t acc[CT][PT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int p = 0; p < PT; ++p) acc[c][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    int nks = (g.nchunks + 7) >> 3;
    // stride-2 data gradient: only the taps whose parity matches the tile's class contribute; steps are addressed
    // absolutely as (valid tap vt, sub-step) instead of incrementally.  The valid taps are rows th0, th0 + 2, .. by columns
    // tw0, tw0 + 2, .. in tap order; KH, KW <= 8 (make_geom), so at most 4 x 4 of them: 2 bits of row and of column each.
    unsigned vrow = 0, vcol = 0;
    int nvt = 0;
    const int th0 = (g.pad_t - cls_py) & 1, tw0 = (g.pad_l - cls_px) & 1;
    const int spt = g.cpt >> 3;                 // k-steps per tap (s2 only)
    if (g.s2) {
        for (int a = 0; th0 + 2 * a < g.KH; ++a)
            for (int b = 0; tw0 + 2 * b < g.KW; ++b) { vrow |= (unsigned)a << (2 * nvt); vcol |= (unsigned)b << (2 * nvt); ++nvt; }
        nks = nvt * spt;
    }
    auto set_step = [&](int step) {             // s2: position the k state on valid step `step`
        const int vt = step / spt, sub = step - vt * spt;
        kh = th0 + 2 * (int)((vrow >> (2 * vt)) & 3);
        kw = tw0 + 2 * (int)((vcol >> (2 * vt)) & 3);
        cc = sub * 8 + slot;
        q = (kh * g.KW + kw) * g.cpt + cc;
    };
    // split-K: this workgroup covers k-steps [ks0, ks1)
    int ks0 = 0, ks1 = nks;
    if (ep.slab) {
        const int per = (nks + ep.ksplit - 1) / ep.ksplit;
        ks0 = min(nks, (int)blockIdx.y * per);
        ks1 = min(nks, ks0 + per);
        if (!g.s2) {                              // position the incremental k state on step ks0
            q = ks0 * 8 + slot;
            tap = q / g.cpt; cc = q - tap * g.cpt;
            kh = tap / g.KW; kw = tap - kh * g.KW;
        }
    }
    if (g.s2 && ks0 < ks1) set_step(ks0);
    if (ks0 < ks1) issue_dma(0);
    const int frow = lane & 15, fk = lane >> 4;
    for (int ks = ks0; ks < ks1; ++ks) {
        const int cur = (ks - ks0) & 1;
        if (!(g.ablate & 2)) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
#pragma unroll
        for (int ksub = 0; ksub < 2; ++ksub) {
            // the next tile's DMA is issued between the two MFMA blocks: its address arithmetic and issue slots then
            // overlap with MFMAs already in flight instead of sitting in front of them
            if (ksub == SSD_DMA_SLOT && ks + 1 < ks1 && !(g.ablate & 1)) {
                if (g.s2) set_step(ks + 1);
                issue_dma(cur ^ 1);
            }
            bf16x8_t fx[PT], fw[CT];
#pragma unroll
            for (int p = 0; p < PT; ++p)
                fx[p] = *reinterpret_cast<const bf16x8_t*>(s_x(cur) + swz(wave_m * (16 * PT) + p * 16 + frow, ksub * 4 + fk));
#pragma unroll
            for (int c = 0; c < CT; ++c)
                fw[c] = *reinterpret_cast<const bf16x8_t*>(s_w(cur) + swz(wave_n * (16 * CT) + c * 16 + frow, ksub * 4 + fk));
            if (g.ablate & 4) {
#pragma unroll
                for (int p = 0; p < PT; ++p) asm volatile("" ::"v"(fx[p]));
#pragma unroll
                for (int c = 0; c < CT; ++c) asm volatile("" ::"v"(fw[c]));
            } else {
#pragma unroll
                for (int c = 0; c < CT; ++c)
#pragma unroll
                    for (int p = 0; p < PT; ++p)
                        acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[c], fx[p], acc[c][p], 0, 0, 0);
            }
        }
    }
    if (staged_ok<EPI>(g, ep) && !(g.ablate & 8)) {
        auto row_to_m = [&](int row) {
            const int m = m0 + row;
            if (m >= cls_count) return -1;
            if (!g.s2) return m;
            int b, oy, ox;
            decode(m, b, oy, ox);
            return (b * g.Ho + oy) * g.Wo + ox;
        };
        staged_epilogue<EPI, BM, BN, CT, PT, NW * 64>(acc, smem, g, ep, n0, wave_m * (16 * PT), wave_n * (16 * CT), tid, row_to_m);
        return;
    }
    int mrow[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        const int m = m0 + wave_m * (16 * PT) + p * 16 + (lane & 15);
        mrow[p] = m < cls_count ? m : -1;
        if (g.s2 && mrow[p] >= 0) {
            int b, oy, ox;
            decode(m, b, oy, ox);
            mrow[p] = (b * g.Ho + oy) * g.Wo + ox;
        }
    }
    conv_epilogue_rows<EPI, CT, PT>(acc, g, ep, mrow, n0 + wave_n * (16 * CT), lane);
}

// ------------------------------------------------------------------------------------------------
// Implicit GEMM, 256x256x64 tile, 8 waves, eight-phase ping-pong schedule (the wide stride-1/2 layers without
// parity classes or split-K).  Waves form two groups of four (one wave of each group per SIMD); the groups run
// half a phase apart, so that on every SIMD one wave is in its MFMA cluster while its partner issues LDS reads and
// the LDS-DMA of a later tile.  A k-tile is staged as four half-tiles of 16 KB (W0, X0, W1, X1: the 32 channels /
// 64 pixels of quadrant-row h of every wave); a phase stages ONE half-tile (2 DMA instructions per wave) and
// multiplies ONE quadrant (64 px x 32 ch x k64 = 16 MFMAs per wave).  Phase p issues half-tile p + 7 of the stream
// (W0 X0 W1 X1 per tile), i.e. three half-tiles of tile t+2 are still in flight across the barriers when tile t+1
// is first read: the only wait on the DMA counter is a counted vmcnt(6) in the last phase of a tile.
//   hazards: a half-tile is read one phase after the wait that retires it (RAW); it is re-staged two phases after
//   its last LDS read, or one phase after for W0 whose reads are retired (lgkmcnt) before the reading phase's
//   first barrier (WAR).  Both hold for either group under the half-phase stagger.
template <int HX, int HW>
__device__ __forceinline__ void mma_quadrant(f32x4_t (&acc)[4][8], const bf16x8_t (&fx)[4][2], const bf16x8_t (&fw)[2][2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                acc[HW * 2 + c][HX * 4 + p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[c][ks], fx[p][ks], acc[HW * 2 + c][HX * 4 + p], 0, 0, 0);
    // hipcc otherwise lets part of the cluster drift below the phase's closing barrier, in among the partner wave's
    // turn: tie the eight accumulators to this point (no instruction is emitted)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) asm volatile("" : "+v"(acc[HW * 2 + c][HX * 4 + p]));
}

__device__ __forceinline__ void keep_frags(const bf16x8_t (&fx)[4][2], const bf16x8_t (&fw)[2][2]) {   // dev ablation only
#pragma unroll
    for (int p = 0; p < 4; ++p) { asm volatile("" ::"v"(fx[p][0])); asm volatile("" ::"v"(fx[p][1])); }
#pragma unroll
    for (int c = 0; c < 2; ++c) { asm volatile("" ::"v"(fw[c][0])); asm volatile("" ::"v"(fw[c][1])); }
}

// ABL: compile-time development ablations (1 no DMA in the loop, 2 no barriers, 4 no MFMA, 16 no fragment reads); 0 in production
template <int EPI, int ABL>
__global__ __launch_bounds__(512) void k_conv_igemm_8ph(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ w,
                                                        ConvGeom g, Epilogue ep) {
    constexpr int BM = 256, BN = 256;
    constexpr int HALF = 128 * 128;             // one half-tile image: 128 rows x 64 k bf16
    constexpr int OFF_W0 = 0, OFF_X0 = HALF, OFF_W1 = 2 * HALF, OFF_X1 = 3 * HALF, BUF = 4 * HALF;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;    // wave tile: pixels wr*128.., channels wc*64..; group = wr
    const int ntn = (g.N + BN - 1) / BN;
    const int ntm = (g.M + BM - 1) / BM;
    const int kx = blockIdx.x >> 3;
    const int mt = (kx / ntn) * 8 + (blockIdx.x & 7);          // XCD-aware order, as k_conv_igemm_dma
    if (mt >= ntm) return;
    const int m0 = mt * BM, n0 = (kx % ntn) * BN;

    // DMA ownership inside a half-tile (16 one-KiB pieces = 8 rows each): wave-instruction i = (wave&1) + 2*((wave>>1) + 4j)
    const int rl = 2 * (lane >> 4) + ((lane >> 3) & 1);
    const int slot = (lane & 7) ^ (4 * (wave & 1) + (lane >> 4));
    int ybase[2][2], xbase[2][2], ibase[2][2];
    unsigned wrow[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 8 * ((wave & 1) + 2 * ((wave >> 1) + 4 * j)) + rl;       // row of the half-tile image
            const int m = m0 + (r >> 6) * 128 + h * 64 + (r & 63);
            const bool mv = m < g.M;
            const int mm = mv ? m : 0;
            const int b = fdiv(mm, g.d_hw);
            const int rem = mm - b * g.d_hw.d;
            const int oy = fdiv(rem, g.d_w);
            const int ox = rem - oy * g.d_w.d;
            ybase[h][j] = mv ? oy * g.mul - g.pad_t : -(1 << 20);
            xbase[h][j] = ox * g.mul - g.pad_l;
            ibase[h][j] = b * g.H * g.W;
            const int n = n0 + (r >> 5) * 64 + h * 32 + (r & 31);
            wrow[h][j] = n < g.N ? (unsigned)n * (unsigned)g.ldw : ~0u;
        }
    // k state of the activation stream (tap and channel chunk of this lane's slot) and of the weight stream
    int tap = slot / g.cpt, cc = slot - tap * g.cpt;
    int kh = tap / g.KW, kw = tap - kh * g.KW;
    int xq = slot, wq = slot;
    const int dmask = g.div - 1, dshift = g.div > 1 ? 1 : 0;

    // LDS-DMA through buffer descriptors: 32-bit byte offsets, and a lane whose chunk is padding / out of range gets
    // an offset beyond the buffer, for which the hardware writes zeros to the lane's LDS slot (no zero block, no branch)
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (unsigned)g.B * g.H * g.W * g.C * 2u, 0x00020000);
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (unsigned)g.N * (unsigned)g.ldw * 2u, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    auto issue_x = [&](int off, int h) {
        const bool kvalid = xq < g.nchunks;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = (wave & 1) + 2 * ((wave >> 1) + 4 * j);
            const int ny = ybase[h][j] + kh, nx = xbase[h][j] + kw;
            const int iy = ny >> dshift, ix = nx >> dshift;
            const bool ok = kvalid && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W && (((ny | nx) & dmask) == 0);
            const unsigned o = ((unsigned)(ibase[h][j] + iy * g.W + ix) * (unsigned)g.C + (unsigned)(cc * 8)) * 2u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(smem + off + i * 1024), 16, ok ? o : OOB, 0, 0, 0);
        }
    };
    auto advance_x = [&]() {                    // cpt >= 8 (host check): at most one tap boundary per k-tile
        xq += 8;
        cc += 8;
        const bool wrap = cc >= g.cpt;
        cc -= wrap ? g.cpt : 0;
        kw += wrap ? 1 : 0;
        const bool roll = kw == g.KW;
        kw = roll ? 0 : kw;
        kh += roll ? 1 : 0;
    };
    auto issue_w = [&](int off, int h) {
        const bool kvalid = wq < g.nchunks;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = (wave & 1) + 2 * ((wave >> 1) + 4 * j);
            const unsigned o = (wrow[h][j] + (unsigned)(wq * 8)) * 2u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wres, (lds_void*)(smem + off + i * 1024), 16,
                                                     (kvalid && wrow[h][j] != ~0u) ? o : OOB, 0, 0, 0);
        }
    };

    f32x4_t acc[4][8];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int p = 0; p < 8; ++p) acc[c][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nt = (g.nchunks + 7) >> 3;
    // prologue: tile 0 completely, W0 X0 W1 of tile 1.  Stages beyond the last tile are issued all the same: every
    // lane is then out of range, zeros land in a half-tile nobody reads any more, and the DMA count per phase stays 2.
    issue_w(OFF_W0, 0); issue_x(OFF_X0, 0); issue_w(OFF_W1, 1); issue_x(OFF_X1, 1);
    wq += 8;
    advance_x();
    issue_w(BUF + OFF_W0, 0); issue_x(BUF + OFF_X0, 0); issue_w(BUF + OFF_W1, 1);
    wq += 8;
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();          // group 1 runs half a phase behind group 0

    const int frow = lane & 15, fk = lane >> 4;
    const int xf0 = swz(wr * 64 + frow, fk), xf1 = swz(wr * 64 + frow, 4 + fk);     // + p * 2048
    const int wf0 = swz(wc * 32 + frow, fk), wf1 = swz(wc * 32 + frow, 4 + fk);     // + c * 2048
    auto ldf = [&](int off) {
        if constexpr (ABL & 16) return bf16x8_t{};
        else return *reinterpret_cast<const bf16x8_t*>(smem + off);
    };
    bf16x8_t fx[4][2] = {}, fw0[2][2] = {}, fw1[2][2] = {};

#define SSD_PHASE_MMA(HX_, HW_, FW_)                                                                                \
    if constexpr (!(ABL & 2)) __builtin_amdgcn_s_barrier();                                                              \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                                              \
    __builtin_amdgcn_s_setprio(1);                                                                                  \
    if constexpr (!(ABL & 4)) mma_quadrant<HX_, HW_>(acc, fx, FW_);                                                      \
    else keep_frags(fx, FW_);                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                              \
    __builtin_amdgcn_s_setprio(0);                                                                                  \
    if constexpr (!(ABL & 2)) __builtin_amdgcn_s_barrier();                                                              \
    __builtin_amdgcn_sched_barrier(0);

    for (int t = 0; t < nt; ++t) {
        const int cb = (t & 1) * BUF, nb = BUF - cb;
        // ---- phase 0: quadrant (X0, W0); stage X1 of tile t+1
#pragma unroll
        for (int c = 0; c < 2; ++c) { fw0[c][0] = ldf(cb + OFF_W0 + wf0 + c * 2048); fw0[c][1] = ldf(cb + OFF_W0 + wf1 + c * 2048); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < 4; ++p) { fx[p][0] = ldf(cb + OFF_X0 + xf0 + p * 2048); fx[p][1] = ldf(cb + OFF_X0 + xf1 + p * 2048); }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(8)" ::: "memory");      // the W0 reads are done: W0 may be re-staged next phase
        if constexpr (!(ABL & 1)) issue_x(nb + OFF_X1, 1);
        advance_x();
        SSD_PHASE_MMA(0, 0, fw0)
        // ---- phase 1: quadrant (X0, W1); stage W0 of tile t+2
#pragma unroll
        for (int c = 0; c < 2; ++c) { fw1[c][0] = ldf(cb + OFF_W1 + wf0 + c * 2048); fw1[c][1] = ldf(cb + OFF_W1 + wf1 + c * 2048); }
        if constexpr (!(ABL & 1)) issue_w(cb + OFF_W0, 0);
        SSD_PHASE_MMA(0, 1, fw1)
        // ---- phase 2: quadrant (X1, W1); stage X0 of tile t+2
#pragma unroll
        for (int p = 0; p < 4; ++p) { fx[p][0] = ldf(cb + OFF_X1 + xf0 + p * 2048); fx[p][1] = ldf(cb + OFF_X1 + xf1 + p * 2048); }
        if constexpr (!(ABL & 1)) issue_x(cb + OFF_X0, 0);
        SSD_PHASE_MMA(1, 1, fw1)
        // ---- phase 3: quadrant (X1, W0); stage W1 of tile t+2; all of tile t+1 has landed once only the last three
        // half-tiles (6 DMA instructions of this wave) are still in flight
        if constexpr (!(ABL & 1)) issue_w(cb + OFF_W1, 1);
        wq += 8;
        asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        SSD_PHASE_MMA(1, 0, fw0)
    }
#undef SSD_PHASE_MMA
    if (wr == 0) __builtin_amdgcn_s_barrier();          // balance the stagger

    // Epilogue through LDS (free now): with one workgroup per CU nothing would hide a scattered store tail
    if (staged_ok<EPI>(g, ep) && !(g.ablate & 8)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the (all-zero) stages issued past the last tile
        auto row_to_m = [&](int row) { const int m = m0 + row; return m < g.M ? m : -1; };
        staged_epilogue<EPI, 256, 256, 4, 8, 512>(acc, smem, g, ep, n0, wr * 128, wc * 64, tid, row_to_m);
        return;
    }
    int mrow[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int m = m0 + wr * 128 + p * 16 + (lane & 15);
        mrow[p] = m < g.M ? m : -1;
    }
    conv_epilogue_rows<EPI, 4, 8>(acc, g, ep, mrow, n0 + wc * 64, lane);
}

// ------------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolution with an LDS-resident input patch (forward, and data gradient with the transposed
// weights): the halo patch of a block is brought into LDS once per channel chunk and all nine taps read their MFMA
// fragments from it at shifted addresses; only the weight slice of a tap streams.  32-channel chunks, linear padded images, two workgroups per CU.
//   * patch image: one 96-byte row per halo pixel (64 B of channels + 32 B pad).  The pitch makes every shifted
//     ds_read_b128 conflict-free WITHOUT an address swizzle, so a fragment address is a per-lane base + immediate
//     (the swizzled 128-byte rows of the first form cost ~10 VALU per read and were 2-way conflicted for 3 of 4 shifts);
//   * weight slice of a tap: [BN][32 k] in 64-byte rows, chunk XORed with (-(row >> 2)) & 3 (conflict-free, fixed rows);
//   * all DMA through buffer descriptors: per-lane byte offsets are computed once, the (tap, chunk) part is a scalar
//     offset, invalid / padding lanes are out of range (zeros): no vector arithmetic per DMA in the loop;
//   * 80 KB of LDS (two patch buffers, two weight buffers) and <= 128 VGPRs: two workgroups per CU cover each other's
//     prologue, barriers and store tail; the next chunk's patch is prefetched at the first tap of the current one and
//     left in flight across the barrier (counted vmcnt).
constexpr int P32_PITCH = 96;
constexpr int P32_PATCH = 32 * 1024;                       // 324 px x 96 B = 31104 B, rounded to 32 DMA instructions
// Store stage of k_conv3x3_patch32 / k_conv3x3_p512: side tables in LDS (LdsSide, conv_common.h) unless the launch carries this
// bit in ConvGeom::ablate -- SSD_EPI_PREFETCH = 0, set by launch_patch: the stage then runs as it did without the tables
constexpr int EPI_NO_PREFETCH = 256;
constexpr int P32_OFF_MAP = 2 * P32_PATCH;                 // row map [256] int: over the weight buffers, once the last tap has been read

template <int BN, int EPI, bool FLAT>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_conv3x3_patch32(
    const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ w, ConvGeom g, Epilogue ep, int tiles_x, int tiles_y, int nblocks, int rowflat) {
    constexpr int CT = BN / 32;
    constexpr int PT = 4;
    constexpr int WBYTES = BN * 64;                          // weight slice of one tap
    constexpr int OFF_W = 2 * P32_PATCH;
    constexpr int OFF_DUMMY = OFF_W + 2 * WBYTES;            // BN = 64: waves 4-7 have no weight rows, their DMA lands here
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave & 3, wave_n = wave >> 2;
    // two block shapes.  flat == 0: a 16x16 block of one image, halo patch 18x18 (tap pitch Q = 18).
    // flat != 0 (narrow maps): the batch is one long strip of positions, image rows at pitch Q = W + 1 (ONE zero column
    // in front of every row: it is the right padding of the row before it as well, the way the ONE zero row between
    // images is the bottom padding of one and the top padding of the next); a block is 256 consecutive positions, its
    // patch those plus Q + 1 on either side, tap (kh,kw) is position + kh*Q + kw.  Pad positions are computed and
    // dropped: 5 % of the work at 38x38 and 10 % at 19x19, where 16x16 blocks would waste 37 % and 65 %.
    // XCD-aware order (workgroup L runs on XCD L % 8): the channel tiles of one pixel block are consecutive on ONE
    // XCD, so the block's patch is fetched into that L2 once
    const int ntn = (g.N + BN - 1) / BN;
    const int kx = blockIdx.x >> 3;
    const int pblock = (kx / ntn) * 8 + (blockIdx.x & 7);
    if (pblock >= nblocks) return;
    const int n0 = (kx % ntn) * BN;
    constexpr bool flat = FLAT;
    const int Q = FLAT ? g.W + 1 : PATCH_W;
    const int img = (g.H + 1) * Q;                          // flat positions per image
    int b = 0, y0 = 0, x0 = 0, f0 = 0;
    if constexpr (FLAT) {
        f0 = pblock * 256;
    } else {
        int t = pblock;
        const int tx = t % tiles_x; t /= tiles_x;
        x0 = tx * 16;
        if (rowflat) { y0 = t * 16; }                       // row of the strip of all images (below), not of one image
        else { const int ty = t % tiles_y; b = t / tiles_y; y0 = ty * 16; }
    }
    // rowflat (wide maps whose height is not a multiple of 16): the rows of all images form one strip, images separated
    // by ONE zero row, and a block is 16 consecutive strip rows x 16 columns -- it may straddle two images, the shared
    // zero row is the bottom padding of one and the top padding of the other.  75 rows per image cost 76 instead of 80.
    // The image pitch in strip rows is g.d_h1.d: H + 1, or the next EVEN number when the epilogue pools (H + 2 for an
    // even H, two zero rows), so that no 2x2 window straddles two images or two blocks (blocks start at even strip rows).
    // block row r (-1 .. 16 for the halo) -> row index into [B * H], -1 = padding / outside
    auto image_row = [&](int r) {
        if (!rowflat) { const int y = y0 + r; return (unsigned)y < (unsigned)g.H ? b * g.H + y : -1; }
        const int R = y0 + r;
        if (R < 0) return -1;
        const int bb = fdiv(R, g.d_h1), yy = R - bb * g.d_h1.d;
        return (bb < g.B && yy < g.H) ? bb * g.H + yy : -1;
    };
    // flat position -> source pixel (element offset / C) or -1
    auto flat_pixel = [&](int f) {
        if (f < 0) return -1;
        const int bb = f / img;
        const int r = f - bb * img;
        const int yy = r / Q, xx = r - yy * Q - 1;
        return (bb < g.B && yy < g.H && (unsigned)xx < (unsigned)g.W) ? (bb * g.H + yy) * g.W + xx : -1;
    };

    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (unsigned)g.B * g.H * g.W * g.C * 2u, 0x00020000);
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (unsigned)g.N * (unsigned)g.ldw * 2u, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    // patch DMA: instruction i = wave + 8j (j < 4) fills slots 64i .. 64i+63; slot q -> pixel q / 6, 16-byte piece q % 6
    unsigned pvo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = (wave + 8 * j) * 64 + lane;
        const int pp = q / 6, sl = q - pp * 6;
        int pix;
        if (flat) {
            pix = pp < 256 + 2 * (Q + 1) ? flat_pixel(f0 - (Q + 1) + pp) : -1;
        } else {
            const int py = pp / PATCH_W, px = pp - py * PATCH_W;
            const int ix = x0 - 1 + px;
            const int ir = pp < PATCH_PIX ? image_row(py - 1) : -1;
            pix = (ir >= 0 && (unsigned)ix < (unsigned)g.W) ? ir * g.W + ix : -1;
        }
        pvo[j] = (sl < 4 && pix >= 0) ? ((unsigned)pix * (unsigned)g.C + (unsigned)(sl * 8)) * 2u : OOB;
    }
    // weight DMA: instruction i = wave (< BN/16) fills rows 16i .. 16i+15; lane L -> row 16i + (L>>2), physical piece L & 3
    // BN = 64: the slices of TWO taps are staged per step (image rows 0..63 = the first tap, 64..127 = the second: the same
    // 128-row image and the same 80 KB of LDS as BN = 128), see the loop below
    unsigned wvo;
    {
        const int row = 16 * wave + (lane >> 2);
        const int piece = (lane & 3) ^ ((-(row >> 2)) & 3);
        const int n = n0 + (BN == 64 ? (row & 63) : row);
        wvo = (row < (BN == 64 ? 128 : BN) && n < g.N) ? ((unsigned)n * (unsigned)g.ldw + (unsigned)(piece * 8)) * 2u : OOB;
    }
    const int wdst = wave < BN / 16 ? wave * 1024 : -1;     // -1: dummy
    const int nchunk = g.C >> 5;

    // The kernel runs at the 128-register limit of four waves per SIMD, and the compiler kept three of the four patch offsets
    // in scratch, re-loading each one right in front of its DMA: "wait for the reload" is s_waitcnt vmcnt(0), which also waits
    // for the patch DMA issued just before to LAND -- the four requests of a chunk went out one memory round trip apart.
    // Here the three offsets are parked in scratch on purpose and fetched TOGETHER ahead of the first request of a chunk
    // (they are only needed once per chunk, when the fragment registers are free): one round trip, four requests back to back.
    unsigned pstash[3];
    pstash[0] = pvo[1]; pstash[1] = pvo[2]; pstash[2] = pvo[3];
    asm volatile("" ::"v"(&pstash[0]) : "memory");          // the address escapes: the array stays in (scratch) memory
    const unsigned pvo0 = pvo[0];
    auto dma_patch = [&](int chunk, int buf) {
        const unsigned o1 = pstash[0], o2 = pstash[1], o3 = pstash[2];
        char* dst = smem + buf * P32_PATCH + wave * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)dst, 16, pvo0, chunk * 64, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(dst + 8 * 1024), 16, o1, chunk * 64, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(dst + 16 * 1024), 16, o2, chunk * 64, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(dst + 24 * 1024), 16, o3, chunk * 64, 0, 0);
    };
    auto dma_w = [&](int chunk, int tap, int buf) {
        char* dst = wdst >= 0 ? smem + OFF_W + buf * WBYTES + wdst : smem + OFF_DUMMY;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wres, (lds_void*)dst, 16, wvo, (tap * g.C + chunk * 32) * 2, 0, 0);
    };

    f32x4_t acc[CT][PT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int p = 0; p < PT; ++p) acc[c][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fk = lane >> 4;
    const int xbase = (flat ? 4 * wave_m * 16 + frow : 4 * wave_m * PATCH_W + frow) * P32_PITCH + fk * 16;
    constexpr int prow = (FLAT ? 16 : PATCH_W) * P32_PITCH;  // bytes between the pixel tiles p, p+1 of a wave
    int wbase;
    {
        const int row = wave_n * (16 * CT) + frow;
        wbase = OFF_W + row * 64 + ((fk ^ ((-(row >> 2)) & 3)) << 4);
    }
    auto ldf = [&](int addr) { return *reinterpret_cast<const bf16x8_t*>(smem + addr); };

    if constexpr (BN == 64) {
        // 64 output channels: a wave has 8 MFMAs per tap, and with one barrier per tap the loop ran at 0.24 of the MFMA peak
        // (block2_conv1's data gradient).  Two taps per step: 16 MFMAs between barriers, five steps per chunk instead of
        // nine.  Waves 0-3 request the first tap's slice of a step, waves 4-7 the second's (out of range for the missing
        // tenth tap: zeros, never read), so every wave issues exactly one weight request per step and the counted waits of
        // the single-tap form carry over.
        constexpr int WB2 = 2 * WBYTES;
        auto dma_w2 = [&](int chunk, int step, int buf) {
            const int tap = 2 * step + (wave >> 2);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(wres, (lds_void*)(smem + OFF_W + buf * WB2 + wave * 1024), 16,
                                                     tap <= 8 ? wvo : OOB, ((tap <= 8 ? tap : 8) * g.C + chunk * 32) * 2, 0, 0);
        };
        dma_patch(0, 0);
        dma_w2(0, 0, 0);
        for (int chunk = 0; chunk < nchunk; ++chunk) {
            const int pb = (chunk & 1) * P32_PATCH;
            const bool next_chunk = chunk + 1 < nchunk;
#pragma unroll
            for (int st = 0; st < 5; ++st) {
                const int sidx = chunk * 5 + st;
                const int wb = (sidx & 1) * WB2;
                if (st == 1 && next_chunk) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (!(g.ablate & 16)) {
                    if (st < 4) dma_w2(chunk, st + 1, (sidx + 1) & 1);
                    else if (next_chunk) dma_w2(chunk + 1, 0, (sidx + 1) & 1);
                }
                if (st == 0 && next_chunk && !(g.ablate & 32)) dma_patch(chunk + 1, (chunk + 1) & 1);
                bf16x8_t fx[2][PT], fw[2][CT];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int tap = 2 * st + t;
                    if (tap > 8) continue;
                    const int tapoff = pb + xbase + ((tap / 3) * Q + tap % 3) * P32_PITCH;
#pragma unroll
                    for (int p = 0; p < PT; ++p) fx[t][p] = ldf(tapoff + p * prow);
#pragma unroll
                    for (int c = 0; c < CT; ++c) fw[t][c] = ldf(wb + wbase + t * WBYTES + c * 1024);
                }
                __builtin_amdgcn_s_setprio(0);               // (as in the 128-channel form below)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if (2 * st + t > 8) continue;
#pragma unroll
                    for (int c = 0; c < CT; ++c)
#pragma unroll
                        for (int p = 0; p < PT; ++p)
                            acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[t][c], fx[t][p], acc[c][p], 0, 0, 0);
                }
                __builtin_amdgcn_s_setprio(3);
            }
        }
    } else {
    dma_patch(0, 0);
    dma_w(0, 0, 0);
    for (int chunk = 0; chunk < nchunk; ++chunk) {
        const int pb = (chunk & 1) * P32_PATCH;
        const bool next_chunk = chunk + 1 < nchunk;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int wb = ((chunk + tap) & 1) * WBYTES;    // step s = 9 chunk + tap: s & 1 == (chunk + tap) & 1
            // this step's weight slice has landed (the patch prefetch issued after it at tap 0 may still be in flight)
            // ... and this wave's LDS reads of the previous step are retired (lgkmcnt) BEFORE the barrier: the weight
            // buffer they came from is re-staged right after it (a read merely issued before the barrier can still be
            // queued in the LDS when a fast L2-hit DMA of another wave lands)
            if (tap == 1 && next_chunk) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (!(g.ablate & 16)) {                          // dev: 16 = no weight DMA in the loop, 32 = no patch DMA in the loop
                if (tap < 8) dma_w(chunk, tap + 1, ((chunk + tap + 1) & 1));
                else if (next_chunk) dma_w(chunk + 1, 0, ((chunk + tap + 1) & 1));
            }
            if (tap == 0 && next_chunk && !(g.ablate & 32)) dma_patch(chunk + 1, (chunk + 1) & 1);
            bf16x8_t fx[PT], fw[CT];
            const int tapoff = pb + xbase + ((tap / 3) * Q + tap % 3) * P32_PITCH;
#pragma unroll
            for (int p = 0; p < PT; ++p) fx[p] = ldf(tapoff + p * prow);
#pragma unroll
            for (int c = 0; c < CT; ++c) fw[c] = ldf(wb + wbase + c * 1024);
            // the MFMA block runs at LOW priority, everything else of a step (wait, barrier, DMA issue, fragment reads) at high:
            // the short instructions of one workgroup's step slip in between the MFMAs of the other's (+3 % on every layer)
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int p = 0; p < PT; ++p)
                    acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[c], fx[p], acc[c][p], 0, 0, 0);
            __builtin_amdgcn_s_setprio(3);
        }
    }
    }
    if (staged_ok<EPI>(g, ep) && !(g.ablate & 8)) {          // tile image [256 block pixels][BN] in the (now idle) patch buffers
        auto row_to_m = [&](int row) {
            if (flat) return flat_pixel(f0 + row);
            const int ir = image_row(row >> 4), xx = x0 + (row & 15);
            return (ir >= 0 && xx < g.Wo) ? ir * g.Wo + xx : -1;
        };
        auto pool_index = [&](int py, int px) -> long long {
            if (flat) return -1;
            int bb = b, gy = (y0 >> 1) + py;
            const int gx = (x0 >> 1) + px;
            if (rowflat) {                                  // even image pitch: the window's two rows lie in ONE image's span
                const int R = y0 + 2 * py;
                bb = fdiv(R, g.d_h1);
                gy = (R - bb * g.d_h1.d) >> 1;
                if (bb >= g.B) return -1;
            }
            return (gy < ep.pool_h && gx < ep.pool_w) ? ((long long)bb * ep.pool_h + gy) * ep.pool_w + gx : -1;
        };
        if constexpr (FLAT && (BN == 128 || EPI == EPI_DGRAD)) {
            // strips: row_to_m is two runtime integer divisions, asked for once per chunk.  The row map goes where the weight
            // slices were: staged_epilogue writes it behind its first barrier, i.e. after every wave's last fragment read has
            // retired.  (Block form: row_to_m is a multiply-high; with the table two of its instantiations spilled 4 and 8
            // bytes more than without, so it keeps calling it.)
            LdsSide<P32_OFF_MAP, -1, -1> side;
            side.map = side.fill = !(g.ablate & EPI_NO_PREFETCH);
            side.signs = side.bias = false;
            staged_epilogue<EPI, 256, BN, CT, PT, 512>(acc, smem, g, ep, n0, wave_m * 64, wave_n * (16 * CT), tid, row_to_m, pool_index, side);
        } else {
            staged_epilogue<EPI, 256, BN, CT, PT, 512>(acc, smem, g, ep, n0, wave_m * 64, wave_n * (16 * CT), tid, row_to_m, pool_index);
        }
        return;
    }
    int mrow[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        if (flat) {
            mrow[p] = flat_pixel(f0 + (4 * wave_m + p) * 16 + (lane & 15));
        } else {
            const int ir = image_row(4 * wave_m + p), xx = x0 + (lane & 15);
            mrow[p] = (ir >= 0 && xx < g.Wo) ? ir * g.Wo + xx : -1;
        }
    }
    conv_epilogue_rows<EPI, CT, PT>(acc, g, ep, mrow, n0 + wave_n * (16 * CT), lane);
}

// ------------------------------------------------------------------------------------------------
// Third form of the LDS-patch kernel: 512 pixels x 128 channels per workgroup, ONE workgroup per CU (an alternative to
// k_conv3x3_patch32<128>, bit-identical results: same chunk / tap accumulation order).
// Twice the pixels per weight slice: 113 KB from L2 per 1152 MFMAs instead of 93 KB per 576, and a wave's tile is
// 128 px x 64 channels (12 fragment reads per 32 MFMAs instead of 8 per 16).  With a single workgroup on the CU nobody
// covers a stall, so latency is taken out of the loop instead:
//   * weight slices live in a ring of FOUR tap slots: the slice of step s + 3 is requested at step s and made visible
//     (vmcnt + barrier) at the top of step s + 2;
//   * the next chunk's halo patch is requested in the first four taps of the current chunk (two DMA instructions per wave
//     and tap) and is first read at the last tap;
//   * vmcnt is counted per tap (the tap loop is unrolled and the number of DMA instructions a wave issues per tap is fixed:
//     table N(T) below), so no wait includes a younger request;
//   * step s runs on fragments that were read from LDS during step s - 1 (second register set), so its MFMAs start right
//     after the barrier;
//   * the store stage fetches nothing and divides nothing per chunk: the tile's ReLU sign bytes (data gradient) or bias
//     (forward, heads) are requested in the prologue, ahead of the first patch piece, into LDS above everything the loop uses,
//     and the tile's row -> pixel map is computed once per row (P5_OFF_SIGNS / _MAP / _BIAS).
// Measured: within +-10 % of k_conv3x3_patch32 layer by layer (faster on the deep narrow maps,
// slower at 150x150) -- with either kernel the matrix pipes are busy ~60 % of the time and the waves are parked at the
// per-tap wait / barrier for most of the rest.
constexpr int P5_PIX = 34 * PATCH_W;                        // 612 halo pixels of a 32 x 16 block
constexpr int P5_NDMA = (P5_PIX * 6 + 63) / 64;             // 58 one-KiB DMA instructions
constexpr int P5_PATCH = P5_NDMA * 1024;                    // 59392 B per buffer
constexpr int P5_WSLOT = 128 * 64;                          // weight slice of one tap: [128 co][32 k]
constexpr int P5_OFF_W = 2 * P5_PATCH;
constexpr int P5_OFF_DUMMY = P5_OFF_W + 4 * P5_WSLOT;       // landing zone of the DMA instructions beyond the patch
constexpr int P5_LOOP_LDS = P5_OFF_DUMMY + 1024;           // 152576 B: what the main loop uses
// side tables of the store stage (LdsSide, conv_common.h), above everything the main loop touches: 163328 of the 163840 B a
// workgroup may have
constexpr int P5_OFF_SIGNS = P5_LOOP_LDS;                   // [512][16] ReLU sign bytes of the tile (data gradient)
constexpr int P5_OFF_MAP = P5_OFF_SIGNS + 512 * 16;         // [512] int: tile row -> output pixel
constexpr int P5_OFF_BIAS = P5_OFF_MAP + 512 * 4;           // [128] float (forward, heads)
constexpr int P5_LDS = P5_OFF_BIAS + 128 * 4;
static_assert(P5_LDS <= 160 * 1024, "k_conv3x3_p512: LDS of one workgroup");

template <int EPI, bool FLAT>
__global__ __launch_bounds__(512) void k_conv3x3_p512(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ w, ConvGeom g,
                                                      Epilogue ep, int tiles_x, int tiles_y, int nblocks, int rowflat) {
    constexpr int BN = 128, CT = 4, PT = 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave & 3, wave_n = wave >> 2;        // pixel rows 8 wave_m .. +7 of the block, channels 64 wave_n .. +63
    const int ntn = (g.N + BN - 1) / BN;
    const int kx = blockIdx.x >> 3;
    const int pblock = (kx / ntn) * 8 + (blockIdx.x & 7);   // channel tiles of one pixel block consecutive on ONE XCD
    if (pblock >= nblocks) return;
    const int n0 = (kx % ntn) * BN;
    const int Q = FLAT ? g.W + 1 : PATCH_W;
    const int img = (g.H + 1) * Q;
    int b = 0, y0 = 0, x0 = 0, f0 = 0;
    if constexpr (FLAT) {
        f0 = pblock * 512;
    } else {
        int t = pblock;
        const int tx = t % tiles_x; t /= tiles_x;
        x0 = tx * 16;
        if (rowflat) { y0 = t * 32; }
        else { const int ty = t % tiles_y; b = t / tiles_y; y0 = ty * 32; }
    }
    auto image_row = [&](int r) {                           // block row (-1 .. 32) -> row of [B * H] or -1, as in k_conv3x3_patch32
        if (!rowflat) { const int y = y0 + r; return (unsigned)y < (unsigned)g.H ? b * g.H + y : -1; }
        const int R = y0 + r;
        if (R < 0) return -1;
        const int bb = fdiv(R, g.d_h1), yy = R - bb * g.d_h1.d;
        return (bb < g.B && yy < g.H) ? bb * g.H + yy : -1;
    };
    auto flat_pixel = [&](int f) {
        if (f < 0) return -1;
        const int bb = f / img;
        const int r = f - bb * img;
        const int yy = r / Q, xx = r - yy * Q - 1;
        return (bb < g.B && yy < g.H && (unsigned)xx < (unsigned)g.W) ? (bb * g.H + yy) * g.W + xx : -1;
    };
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (unsigned)g.B * g.H * g.W * g.C * 2u, 0x00020000);
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (unsigned)g.N * (unsigned)g.ldw * 2u, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    // patch DMA: instruction i = wave + 8 j (j < 8; i >= 58 lands in the dummy zone) fills slots 64 i ..: slot q -> pixel q / 6,
    // 16-byte piece q % 6 (pieces 4, 5 are the row padding)
    unsigned pvo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int q = (wave + 8 * j) * 64 + lane;
        const int pp = q / 6, sl = q - pp * 6;
        int pix;
        if constexpr (FLAT) {
            pix = pp < 512 + 2 * (Q + 1) ? flat_pixel(f0 - (Q + 1) + pp) : -1;
        } else {
            const int py = pp / PATCH_W, px = pp - py * PATCH_W;
            const int ix = x0 - 1 + px;
            const int ir = pp < P5_PIX ? image_row(py - 1) : -1;
            pix = (ir >= 0 && (unsigned)ix < (unsigned)g.W) ? ir * g.W + ix : -1;
        }
        pvo[j] = (sl < 4 && pix >= 0 && wave + 8 * j < P5_NDMA) ? ((unsigned)pix * (unsigned)g.C + (unsigned)(sl * 8)) * 2u : OOB;
    }
    unsigned wvo;                                           // weight DMA: wave i fills rows 16 i .. 16 i + 15 of a slot
    {
        const int row = 16 * wave + (lane >> 2);
        const int piece = (lane & 3) ^ ((-(row >> 2)) & 3);
        const int n = n0 + row;
        wvo = n < g.N ? ((unsigned)n * (unsigned)g.ldw + (unsigned)(piece * 8)) * 2u : OOB;
        if (g.ablate & 16) wvo = OOB;                       // dev: weight requests fetch nothing (same instruction count)
    }
    const int nchunk = g.C >> 5;
    const int nstep = nchunk * 9;
    auto dma_piece = [&](int chunk, int buf, int j, bool live) {
        char* dst = wave + 8 * j < P5_NDMA ? smem + buf * P5_PATCH + (wave + 8 * j) * 1024 : smem + P5_OFF_DUMMY;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)dst, 16, live ? pvo[j] : OOB, chunk * 64, 0, 0);
    };
    auto dma_w = [&](int step) {                            // slice of step (chunk = step / 9, tap = step % 9) into ring slot step & 3
        const int st = step < nstep ? step : nstep - 1;     // past the end: a harmless refetch (the count per tap stays fixed)
        const int ch = st / 9, tp = st - ch * 9;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wres, (lds_void*)(smem + P5_OFF_W + (step & 3) * P5_WSLOT + wave * 1024), 16, wvo,
                                                 (tp * g.C + ch * 32) * 2, 0, 0);
    };
    f32x4_t acc[CT][PT];
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int p = 0; p < PT; ++p) acc[c][p] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fk = lane >> 4;
    const int xbase = (FLAT ? 8 * wave_m * 16 + frow : 8 * wave_m * PATCH_W + frow) * P32_PITCH + fk * 16;
    constexpr int prow = (FLAT ? 16 : PATCH_W) * P32_PITCH;
    int wbase;
    {
        const int row = wave_n * 64 + frow;
        wbase = P5_OFF_W + row * 64 + ((fk ^ ((-(row >> 2)) & 3)) << 4);
    }
    auto ldf = [&](int addr) { return lds_read_b128_scoped(smem + addr, smem); };
    auto load_x = [&](bf16x8_t (&fx)[PT], int pb, int tap) {
        const int tapoff = pb + xbase + ((tap / 3) * Q + tap % 3) * P32_PITCH;
#pragma unroll
        for (int p = 0; p < PT; ++p) fx[p] = ldf(tapoff + p * prow);
    };
    auto load_w = [&](bf16x8_t (&fw)[CT], int step) {
        const int wb = (step & 3) * P5_WSLOT;
#pragma unroll
        for (int c = 0; c < CT; ++c) fw[c] = ldf(wb + wbase + c * 1024);
    };
    auto row_to_m = [&](int row) {                          // tile row -> flat output pixel or -1
        if constexpr (FLAT) return flat_pixel(f0 + row);
        const int ir = image_row(row >> 4), xx = x0 + (row & 15);
        return (ir >= 0 && xx < g.Wo) ? ir * g.Wo + xx : -1;
    };
    // Side tables of the store stage, requested FIRST: they are the oldest requests in flight, so the prologue's counted wait
    // below covers them and no count of the tap loop sees them (every N(T) counts requests younger than a weight slice).
    LdsSide<P5_OFF_MAP, P5_OFF_SIGNS, P5_OFF_BIAS> side;
    side.map = side.fill = !(g.ablate & EPI_NO_PREFETCH) && staged_ok<EPI>(g, ep);
    side.signs = side.bias = false;
    if constexpr (EPI == EPI_DGRAD) {
        // ReLU sign bytes: one 16-byte piece per tile row, lane = row (wave i: rows 64 i .. 64 i + 63), rows outside the map
        // out of range = zeros.  Only where every row's piece is whole and 16-byte aligned -- N a multiple of 128, so that all
        // channel tiles are full and the row pitch N / 8 is a multiple of 16 -- and within the descriptor's 32-bit range;
        // otherwise, and under mask_src, the store stage reads its signs from global memory as before
        const long long sign_bytes = (long long)g.M * (g.N >> 3);
        side.signs = side.map && ep.mask_bits && !ep.mask_src && (g.N & 127) == 0 &&
                     (reinterpret_cast<unsigned long long>(ep.mask_bits) & 15ull) == 0 && sign_bytes < (1ll << 31) - 16;
        if (side.signs) {
            const int m = row_to_m(tid);
            lds_st4_scoped(smem + P5_OFF_MAP + tid * 4, smem, m);
            side.fill = false;
            const __amdgpu_buffer_rsrc_t sres = __builtin_amdgcn_make_buffer_rsrc((void*)ep.mask_bits, 0, (unsigned)sign_bytes, 0x00020000);
            dma16_buf(sres, smem + P5_OFF_SIGNS + wave * 1024, m >= 0 ? (unsigned)m * (unsigned)(g.N >> 3) + (unsigned)(n0 >> 3) : OOB);
        }
    } else {
        // bias of the tile: 128 floats, waves 0 and 1 (the others request nothing, into the dummy zone: one instruction per wave)
        side.bias = side.map;
        if (side.bias) {
            const __amdgpu_buffer_rsrc_t bres = __builtin_amdgcn_make_buffer_rsrc((void*)ep.bias, 0, ep.bias ? (unsigned)g.N * 4u : 0u, 0x00020000);
            const int n = n0 + wave * 64 + lane;
            char* dst = wave < 2 ? smem + P5_OFF_BIAS + wave * 256 : smem + P5_OFF_DUMMY;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(bres, (lds_void*)dst, 4, (wave < 2 && n < g.N) ? (unsigned)n * 4u : OOB, 0, 0, 0);
        }
    }
    // prologue: the whole first patch and the first three weight slices; fragments of step 0
#pragma unroll
    for (int j = 0; j < 8; ++j) dma_piece(0, 0, j, true);
    dma_w(0); dma_w(1); dma_w(2);
    bf16x8_t fxa[PT], fxb[PT], fwa[CT], fwb[CT];
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");         // patch 0 and slice 0 (slices 1, 2 are younger)
    __builtin_amdgcn_s_barrier();
    load_x(fxa, 0, 0);
    load_w(fwa, 0);
    // nine taps per chunk: the register set of a step follows the parity of the GLOBAL step, so chunks go in pairs (C % 64 == 0)
    auto run_chunk = [&](int chunk, auto par_tag) {
        constexpr int PAR = decltype(par_tag)::value;
        const int pb = (chunk & 1) * P5_PATCH;
        const bool next_chunk = chunk + 1 < nchunk && !(g.ablate & 32);   // dev 32: patch requests after the first fetch nothing
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            // Step s runs on fragments read during step s - 1; at its top it makes slice s + 1 (and, at tap 8, the next patch)
            // visible, requests slice s + 3 and two patch pieces (taps 0-3), and reads the fragments of step s + 1 under its
            // own MFMAs.  DMA instructions a wave has issued AFTER slice s + 1 (requested two steps ago, first of its step):
            //   T:    0  1  2  3  4  5  6  7  8
            //   N(T): 1  3  5  5  5  3  1  1  1       (first chunk: the prologue issued patch, slices 0, 1, 2 in that order: same)
            // All patch pieces of the NEXT chunk are requested by tap 3, i.e. older than everything tap 8 leaves in flight.
            constexpr int NT[9] = {1, 3, 5, 5, 5, 3, 1, 1, 1};
            if (NT[tap] == 1) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
            else if (NT[tap] == 3) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const int step = chunk * 9 + tap;
            dma_w(step + 3);
            if (tap < 4) {
                dma_piece(chunk + 1, (chunk + 1) & 1, 2 * tap, next_chunk);
                dma_piece(chunk + 1, (chunk + 1) & 1, 2 * tap + 1, next_chunk);
            }
            bf16x8_t (&fxc)[PT] = ((tap + PAR) & 1) ? fxb : fxa;
            bf16x8_t (&fxn)[PT] = ((tap + PAR) & 1) ? fxa : fxb;
            bf16x8_t (&fwc)[CT] = ((tap + PAR) & 1) ? fwb : fwa;
            bf16x8_t (&fwn)[CT] = ((tap + PAR) & 1) ? fwa : fwb;
            // fragments of the next step (tap 8: tap 0 of the next chunk, from the other patch buffer; the very last step
            // re-reads its own)
            if (tap < 8) load_x(fxn, pb, tap + 1);
            else load_x(fxn, next_chunk ? (P5_PATCH - pb) : pb, next_chunk ? 0 : 8);
            load_w(fwn, step + 1 < nstep ? step + 1 : step);
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int p = 0; p < PT; ++p)
                    acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fwc[c], fxc[p], acc[c][p], 0, 0, 0);
            // Issue order inside the step: one fragment read after every two MFMAs, the last eight MFMAs without.  Left alone the scheduler either
            // sinks the reads to just before their first use in the NEXT step (the MFMAs then start by waiting for LDS), or,
            // pinned in front of the MFMAs, all eight waves burst 96 KB of reads at the LDS right after the barrier and the
            // in-order MFMAs queue behind them: measured 0.59 MFMA-busy at 2.3 GHz with or without any memory traffic.
#define SSD_P5_GROUP(NM_) __builtin_amdgcn_sched_group_barrier(0x008, NM_, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0)
            SSD_P5_GROUP(2); SSD_P5_GROUP(2); SSD_P5_GROUP(2); SSD_P5_GROUP(2); SSD_P5_GROUP(2); SSD_P5_GROUP(2);
            SSD_P5_GROUP(2); SSD_P5_GROUP(2); SSD_P5_GROUP(2); SSD_P5_GROUP(2); SSD_P5_GROUP(2); SSD_P5_GROUP(2);
            __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);   // the last eight MFMAs cover the latency of the last reads
#undef SSD_P5_GROUP
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (int chunk = 0; chunk < nchunk; chunk += 2) {
        run_chunk(chunk, std::integral_constant<int, 0>{});
        run_chunk(chunk + 1, std::integral_constant<int, 1>{});
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // the refetches past the end have landed before LDS is reused
    if (staged_ok<EPI>(g, ep)) {                             // tile image [512 block pixels][128] over the patch buffers + ring
        auto pool_index = [&](int py, int px) -> long long {    // as in k_conv3x3_patch32
            if (FLAT) return -1;
            int bb = b, gy = (y0 >> 1) + py;
            const int gx = (x0 >> 1) + px;
            if (rowflat) {
                const int R = y0 + 2 * py;
                bb = fdiv(R, g.d_h1);
                gy = (R - bb * g.d_h1.d) >> 1;
                if (bb >= g.B) return -1;
            }
            return (gy < ep.pool_h && gx < ep.pool_w) ? ((long long)bb * ep.pool_h + gy) * ep.pool_w + gx : -1;
        };
        staged_epilogue<EPI, 512, BN, CT, PT, 512>(acc, smem, g, ep, n0, wave_m * 128, wave_n * 64, tid, row_to_m, pool_index, side);
        return;
    }
    int mrow[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        if constexpr (FLAT) {
            mrow[p] = flat_pixel(f0 + (8 * wave_m + p) * 16 + (lane & 15));
        } else {
            const int ir = image_row(8 * wave_m + p), xx = x0 + (lane & 15);
            mrow[p] = (ir >= 0 && xx < g.Wo) ? ir * g.Wo + xx : -1;
        }
    }
    conv_epilogue_rows<EPI, CT, PT>(acc, g, ep, mrow, n0 + wave_n * 64, lane);
}

// ------------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 with 64 input and 64 output channels (block1_conv2 forward and data gradient): 1.5-2.2 GB of
// traffic for 425 GFLOP, i.e. close to the HBM bound, and in the general patch kernel the [64][576] weight matrix
// (72 KB) was re-streamed for every 16x16 block: more than half of the CU's L2 ingest.  Here the weights live in
// REGISTERS for the whole kernel (a wave owns 32 output channels: 2 tiles x 9 taps x 2 k-halves = 36 A fragments,
// 144 VGPRs), workgroups are persistent, the only LDS traffic is the halo patch (64 channels, 160-byte rows: conflict-
// free and immediate-addressed) which is prefetched one block ahead, and the nine taps of a block run without a
// single barrier.  The result leaves through the shared staged epilogue.
constexpr int C64_PITCH = 160;

// ------------------------------------------------------------------------------------------------
// Timing the pieces of a first form of this kernel (16x16 blocks, one 8-wave workgroup per CU) on MI355X showed its
// fragment reads (72 ds_read_b128 per wave and block = 4.6k LDS cycles per block at 128 B/clk) to cost as much as its
// MFMAs (4.6k cycles) without overlapping them, and the epilogue (another 30 % of the time) to run with the matrix cores
// idle because the CU holds a single workgroup.  Here
//   * a fragment is read ONCE per patch row and reused by every tap that touches it: the wave walks the 6 patch rows of
//     its 4 output rows, and the fragment (row r, dx, k-half) feeds the MFMAs of (dy, p = r - dy) for all valid dy --
//     36 reads per wave and block instead of 72, issued two steps ahead of their use;
//   * workgroups are 4 waves on an 8 x 16 block and two of them share a CU (74 KB of LDS, 256 VGPRs per wave): they
//     drift apart, so one's epilogue (LDS turn-around, coalesced stores, fused pooling) runs under the other's MFMAs.
constexpr int C64B_ROWS = 8;                               // block = 8 rows x 16 columns
constexpr int C64B_PATCH_PIX = (C64B_ROWS + 2) * PATCH_W;  // 180 halo pixels
constexpr int C64B_NDMA = (C64B_PATCH_PIX * 10 + 63) / 64; // 29 wave-instructions of 64 x 16 B
constexpr int C64B_PATCH = C64B_NDMA * 1024;               // 29696 B per buffer
constexpr int C64B_STAGE = 2 * C64B_PATCH;                 // [128 px][64 ch] bf16 staging tile (16 KB)
constexpr int C64B_FRAG_DEPTH = 3;                          // fragment reads run two steps ahead (four and six: measured, no faster)
constexpr int C64B_BIAS = C64B_STAGE + 128 * 128;          // forward: the 64 biases (the accumulators start from them)
constexpr int C64B_LDS = C64B_BIAS + 256;

// W0 form (block1_conv2's data gradient + block1_conv1's weight gradient in one kernel).  The gradient this layer produces has
// exactly one consumer -- the weight gradient of the 3-channel first layer, dW0[co][tap][ci] = sum_px dX[px][co] * img[px +
// tap][ci] -- and that consumer was a pure HBM stream (k_conv0_wgrad: 737 MB read, 187 us at batch 64) behind a 737 MB
// write here.  The masked bf16 tile is already in LDS for the store stage: instead of storing it, the four waves multiply
// it with the 10 x 18 image halo patch (channels 0..3 of the 16-byte pixel, fetched by 4-byte LDS-DMA next to the 64-channel
// patch): wave w owns output channels 16 w .. +15, three column tiles of (4 taps x 4 channels) -- the pad channel of the
// centre tap carries ones, i.e. the bias gradient --, four k-steps of 32 pixels: 12 MFMAs and 32 transposing LDS reads per
// wave and block next to the 144 MFMAs of the convolution.  The running sums live in LDS (the kernel has no register to
// spare), one [64][72] + [64] fp32 slab per workgroup leaves at the end; nothing else is written.
struct C64W0 {
    const bf16_raw* img;                                    // [B][H][W][8] bf16 (ssd_image_prep), channels 3..7 zero
    float* slab_w;                                          // [gridDim.x][64][72]
    float* slab_b;                                          // [gridDim.x][64]
};
constexpr int C64B_IMG = 6 * 256;                           // 180 halo pixels x 8 bytes = six 4-byte DMA instructions
constexpr int C64B_W0_IMG = 2 * C64B_PATCH;                 // (the staging tile reuses the patch buffer just consumed)
constexpr int C64B_W0_SUMS = C64B_W0_IMG + 2 * C64B_IMG;
constexpr int C64B_W0_LDS = C64B_W0_SUMS + 4 * 3 * 64 * 16; // [wave][column tile][lane] f32x4

template <int EPI, bool W0 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_conv3x3_c64b(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ w, ConvGeom g, Epilogue ep, int tiles_x, int tiles_y,
                    C64W0 w0) {
    static_assert(!W0 || EPI == EPI_DGRAD, "the fused first-layer weight gradient belongs to the data gradient");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave & 1, wave_n = wave >> 1;        // output rows 4 wave_m + p, channels 32 wave_n + 16 c
    const int nblocks = g.B * tiles_x * tiles_y;
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (unsigned)g.B * g.H * g.W * 64u * 2u, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    constexpr int NJ = (C64B_NDMA + 3) / 4;                 // DMA instructions per wave: i = wave + 4 j
    const __amdgpu_buffer_rsrc_t ires = __builtin_amdgcn_make_buffer_rsrc((void*)(W0 ? w0.img : x), 0, (unsigned)g.B * g.H * g.W * 16u, 0x00020000);

    int pcode[NJ];                                          // py << 16 | px << 8 | byte offset of the piece, -1 = padding
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int q = (wave + 4 * j) * 64 + lane;
        const int pp = q / 10, sl = q - pp * 10;
        const int py = pp / PATCH_W, px = pp - py * PATCH_W;
        pcode[j] = (sl < 8 && pp < C64B_PATCH_PIX && wave + 4 * j < C64B_NDMA) ? ((py << 16) | (px << 8) | (sl * 16)) : -1;
    }
    auto issue_patch = [&](int t, int buf) {
        int r = t;
        const int tx = r % tiles_x; r /= tiles_x;
        const int ty = r % tiles_y;
        const int b = r / tiles_y;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (wave + 4 * j < C64B_NDMA) {
                const int iy = ty * C64B_ROWS - 1 + (pcode[j] >> 16), ix = tx * 16 - 1 + ((pcode[j] >> 8) & 255);
                const bool ok = pcode[j] >= 0 && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
                const unsigned off = (unsigned)((b * g.H + iy) * g.W + ix) * 128u + (unsigned)(pcode[j] & 255);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(smem + buf * C64B_PATCH + (wave + 4 * j) * 1024), 16,
                                                         ok ? off : OOB, 0, 0, 0);
            }
        }
        if constexpr (W0) {                                 // image halo: dword q = pixel q / 2, channels 2 (q & 1) .. +1
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (wave + 4 * j < 6) {
                    const int q = (wave + 4 * j) * 64 + lane, pp = q >> 1;
                    const int py = pp / PATCH_W, px = pp - py * PATCH_W;
                    const int iy = ty * C64B_ROWS - 1 + py, ix = tx * 16 - 1 + px;
                    const bool ok = pp < C64B_PATCH_PIX && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
                    const unsigned off = (unsigned)((b * g.H + iy) * g.W + ix) * 16u + (unsigned)(q & 1) * 4u;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(ires, (lds_void*)(smem + C64B_W0_IMG + buf * C64B_IMG + (wave + 4 * j) * 256), 4,
                                                             ok ? off : OOB, 0, 0, 0);
                }
            }
        }
    };
    // XCD-aware order: workgroup i runs on XCD i % 8; give every XCD one contiguous range of blocks and let its workgroups
    // walk it side by side, so that the halo rows/columns shared by neighbouring blocks meet in that XCD's L2
    const bool xcd_order = (gridDim.x & 7) == 0 && !(g.ablate & 64);
    const int per_xcd = (nblocks + 7) >> 3, slots = gridDim.x >> 3;
    auto block_of = [&](int i) {                            // the i-th block of this workgroup, -1 = done
        if (!xcd_order) { const int t = blockIdx.x + i * gridDim.x; return t < nblocks ? t : -1; }
        const int lin = i * slots + ((int)blockIdx.x >> 3);
        const int t = ((int)blockIdx.x & 7) * per_xcd + lin;
        return (lin < per_xcd && t < nblocks) ? t : -1;
    };
    if (block_of(0) >= 0) issue_patch(block_of(0), 0);

    const int frow = lane & 15, fk = lane >> 4;
    bf16x8_t fw[2][9][2];                                   // as in k_conv3x3_c64
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int n = wave_n * 32 + c * 16 + frow;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (n < g.N) v = *reinterpret_cast<const uint4*>(w + (unsigned)n * 576u + (unsigned)(tap * 64 + ks * 32 + fk * 8));
                fw[c][tap][ks] = *reinterpret_cast<const bf16x8_t*>(&v);
            }
    }
    const int xbase = (4 * wave_m * PATCH_W + frow) * C64_PITCH + fk * 16;
    // forward: the bias is the accumulators' initial value (from LDS, written once here; the first barrier of the block loop
    // publishes it) -- fetched in the epilogue it was a global round trip per block with the matrix cores idle
    if constexpr (EPI == EPI_FWD) {
        if (tid < 64) reinterpret_cast<float*>(smem + C64B_BIAS)[tid] = (ep.bias && tid < g.N) ? ep.bias[tid] : 0.f;
    }
    if constexpr (W0) {                                     // this wave's running sums (no other wave touches them)
        f32x4_t* sums = reinterpret_cast<f32x4_t*>(smem + C64B_W0_SUMS) + wave * 3 * 64 + lane;
#pragma unroll
        for (int nt = 0; nt < 3; ++nt) sums[nt * 64] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }

    // W0: mkn[p] = the four sign bytes of this wave's 32 channels at the lane's pixel of accumulator row p of block t (block row
    // 4 wave_m + p, column lane & 15); 0 outside the map
    unsigned mkn[4] = {0u, 0u, 0u, 0u};
    auto load_masks = [&](int t) {
        int r = t;
        const int tx = r % tiles_x; r /= tiles_x;
        const int ty = r % tiles_y;
        const int b = r / tiles_y;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int y = ty * C64B_ROWS + 4 * wave_m + p, xx = tx * 16 + (lane & 15);
            mkn[p] = 0u;
            if (y < g.Ho && xx < g.Wo)
                mkn[p] = *reinterpret_cast<const unsigned*>(ep.mask_bits + (long long)((b * g.Ho + y) * g.Wo + xx) * 8 + wave_n * 4);
        }
    };
    if constexpr (W0) { if (block_of(0) >= 0) load_masks(block_of(0)); }

    int it = 0, prev_st = 0;
    for (int t = block_of(0); t >= 0; t = block_of(++it)) {
        const int cur = it & 1;
        // this block's patch (issued one block ago) is older than the epilogue stores issued since: wait for all but those
        // (prev_st = wave-uniform lower bound of the store instructions the previous epilogue issued)
        if (g.ablate & 2) {}                                // (timing experiment, development builds: do not wait for the patch)
        else if (prev_st >= 6) asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");
        else if (prev_st == 5) asm volatile("s_waitcnt vmcnt(5) lgkmcnt(0)" ::: "memory");
        else if (prev_st == 4) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else if (prev_st == 3) asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
        else if (prev_st == 2) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        else if (prev_st == 1) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        __builtin_amdgcn_s_setprio(0);
        int r = t;
        const int tx = r % tiles_x; r /= tiles_x;
        const int ty = r % tiles_y;
        const int b = r / tiles_y;
        const int y0 = ty * C64B_ROWS, x0 = tx * 16;
        // data gradient: the ReLU mask (the forward activation at the output position) is fetched NOW, ahead of the next
        // patch, and is in registers long before the epilogue needs it -- fetched there, every block paid a full memory
        // round trip with the matrix cores idle (300 us of the 630 us this kernel took)
        // (only the sign-bit form of the mask is pre-fetched -- one register per chunk; a bf16 mask_src takes the shared staged
        //  epilogue, which reads it there: holding four 16-byte masks across the MFMA phase cost 12 more registers in a kernel
        //  that sits at the 256-register limit and spilled 20, each reload in the epilogue draining the store queue)
        //  The four chunks of a thread sit in ONE column of the block, two rows apart: their pixel indices are recomputed where
        //  they are used instead of being held across the MFMA phase.)
        unsigned mk[4];
        // chunk i of thread `t`: block row 2 i + (t >> 7), column (t >> 3) & 15, channels 8 (t & 7) .. +7; -1 = outside the map
        auto chunk_pixel = [&](int t, int i) {
            const int y = y0 + 2 * i + (t >> 7), xx = x0 + ((t >> 3) & 15);
            return (y < g.Ho && xx < g.Wo) ? (b * g.Ho + y) * g.Wo + xx : -1;
        };
        const bool premask = EPI == EPI_DGRAD && ep.mask_bits != nullptr && !(g.ablate & 128);
        if constexpr (W0) {
            // W0 form: the mask is applied to the accumulators themselves (the masked tile feeds the weight-gradient MFMAs from
            // LDS: no second pass over it) and travels one block ahead like the patch: the wait at the top of the loop has
            // covered it, the epilogue waits for no memory operation at all
#pragma unroll
            for (int p = 0; p < 4; ++p) mk[p] = mkn[p];
        } else if constexpr (EPI == EPI_DGRAD) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = chunk_pixel(tid, i);
                mk[i] = 0u;
                if (premask && m >= 0) mk[i] = ep.mask_bits[(long long)m * 8 + (tid & 7)];
            }
        }
        const int tnext = block_of(it + 1);
        if (tnext >= 0 && !(g.ablate & 1)) issue_patch(tnext, cur ^ 1);
        if constexpr (W0) { if (tnext >= 0) load_masks(tnext); }
        const int pb = cur * C64B_PATCH + xbase;
        f32x4_t acc[2][4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            f32x4_t a0 = f32x4_t{0.f, 0.f, 0.f, 0.f};
            if constexpr (EPI == EPI_FWD)
                a0 = *reinterpret_cast<const f32x4_t*>(smem + C64B_BIAS + (wave_n * 32 + c * 16 + (lane >> 4) * 4) * 4);
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[c][p] = a0;
        }
        // step s = (patch row rr = s / 6, dx = (s / 2) % 3, k-half = s & 1)
        auto frag = [&](int s2) {
            return *reinterpret_cast<const bf16x8_t*>(smem + pb + ((s2 / 6) * PATCH_W + (s2 / 2) % 3) * C64_PITCH + (s2 & 1) * 64);
        };
        // fragment ring: the read of step s2 + FD - 1 is issued at the start of step s2 (into the slot step s2 - 1 used)
        constexpr int FD = C64B_FRAG_DEPTH;
        bf16x8_t fr[FD];
#pragma unroll
        for (int i = 0; i < FD - 1; ++i) fr[i] = frag(i);
#pragma unroll
        for (int s2 = 0; s2 < 36; ++s2) {
            if (s2 + FD - 1 < 36) fr[(s2 + FD - 1) % FD] = frag(s2 + FD - 1);
            const int rr = s2 / 6, dx = (s2 / 2) % 3, ks = s2 & 1;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int p = rr - dy;
                if (p >= 0 && p < 4) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        acc[c][p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[c][dy * 3 + dx][ks], fr[s2 % FD], acc[c][p], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);              // keep the reads FD - 1 steps ahead, no further (144 VGPRs of weights)
        }
        // From here to the barrier at the top of the next block this wave runs at high priority: its epilogue (conversions, LDS
        // turn, stores / the fused weight gradient) is a few hundred short instructions that were being starved of issue slots
        // by the OTHER workgroup's stream of 144 MFMAs on the same SIMD -- the two workgroups of a CU did not overlap, they took
        // turns (section 4: "the second workgroup hides only half").  W0 form 480 -> 446 us, forward 410 -> 403 us.
        __builtin_amdgcn_s_setprio(3);
        if (g.ablate & 8) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int p = 0; p < 4; ++p) asm volatile("" :: "v"(acc[c][p]));
            prev_st = 0;
            continue;
        }
        auto row_to_m = [&](int row) {
            const int y = y0 + (row >> 4), xx = x0 + (row & 15);
            return (y < g.Ho && xx < g.Wo) ? (b * g.Ho + y) * g.Wo + xx : -1;
        };
        auto pool_index = [&](int py, int px) -> long long {
            const int gy = (y0 >> 1) + py, gx = (x0 >> 1) + px;
            return (gy < ep.pool_h && gx < ep.pool_w) ? ((long long)b * ep.pool_h + gy) * ep.pool_w + gx : -1;
        };
        if constexpr (W0) {
            // (the host only launches this form with sign bits: premask holds)
            char* st = smem + cur * C64B_PATCH;             // staging tile [128 px][64 ch] over the patch every wave is done with
            // (bare barriers: __syncthreads() would also wait for the next block's patch, the LDS-DMA in flight)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            int t2 = tid;
            asm volatile("" : "+v"(t2));                     // (opaque copy: indices are recomputed here, not held across the MFMA phase)
            {
                const int l3 = t2 & 63;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int col = wave_n * 32 + c * 16 + (l3 >> 4) * 4;
                    const int sh = 8 * (2 * c + (l3 >> 5)) + 4 * ((l3 >> 4) & 1);   // this lane's four sign bits within mk[p]
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int row = wave_m * 64 + p * 16 + (l3 & 15);
                        const unsigned bits = mk[p] >> sh;
                        const unsigned k0 = keep_mask2(bits, 0), k1 = keep_mask2(bits, 2);
                        lds_st8_scoped(st + row * 128 + ((((col >> 3) ^ row) & 7) << 4) + (col & 4) * 2, smem,
                            make_uint2((pack_bf16x2(acc[c][p][0], acc[c][p][1])) & k0,
                                       (pack_bf16x2(acc[c][p][2], acc[c][p][3])) & k1));
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            // dW0 tile of this wave: D[co = 16 wave + 4 (lane >> 4) + j][column = lane & 15] over the 128 pixels of the block.
            // MFMA k index 8 g + e of k-step s  <->  block pixel 32 s + 8 g + e (row 2 s + (g >> 1), column 8 (g & 1) + e); both
            // operands come through the transposing read: lane 4 q + p of a 16-lane group supplies the address of k row q (+ 4
            // for the second half), elements 4 p .. 4 p + 3 of the 16 columns.
            int l2 = t2 & 63;
            const int gq = l2 >> 4, q = (l2 >> 2) & 3, p4 = l2 & 3;
            int db[2], ib[3];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = 8 * gq + q + 4 * h;
                db[h] = r * 128 + ((((2 * wave + (p4 >> 1)) ^ r) & 7) << 4) + (p4 & 1) * 8;
            }
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) {                // column 4 p + ci of tile nt = tap 4 nt + p, image channel ci
                int tap = 4 * nt + p4;
                if (tap > 8) tap = 8;                       // (columns of taps 9..11 are never stored)
                ib[nt] = (((gq >> 1) + tap / 3) * PATCH_W + 8 * (gq & 1) + q + tap % 3) * 8;
            }
            const char* im = smem + C64B_W0_IMG + cur * C64B_IMG;
            f32x4_t* sums = reinterpret_cast<f32x4_t*>(smem + C64B_W0_SUMS) + wave * 3 * 64 + l2;
            f32x4_t aw[3];
#pragma unroll
            for (int nt = 0; nt < 3; ++nt) {
                const uint4 u = lds_ld16_scoped(reinterpret_cast<const char*>(sums + nt * 64), smem);
                aw[nt] = f32x4_t{__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)};
            }
            bf16x8_t ones;
#pragma unroll
            for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                bf16x8_t fd;
                reinterpret_cast<s16x4_t*>(&fd)[0] = lds_read_tr16_scoped(st + db[0] + s * 4096, smem);
                reinterpret_cast<s16x4_t*>(&fd)[1] = lds_read_tr16_scoped(st + db[1] + s * 4096, smem);
#pragma unroll
                for (int nt = 0; nt < 3; ++nt) {
                    bf16x8_t fp;
                    reinterpret_cast<s16x4_t*>(&fp)[0] = lds_read_tr16_scoped(im + ib[nt] + s * (2 * PATCH_W * 8), smem);
                    reinterpret_cast<s16x4_t*>(&fp)[1] = lds_read_tr16_scoped(im + ib[nt] + s * (2 * PATCH_W * 8) + 32, smem);
                    if (nt == 1) fp = (l2 & 15) == 3 ? ones : fp;   // centre tap, pad channel: the bias gradient
                    aw[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fd, fp, aw[nt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int nt = 0; nt < 3; ++nt)
                lds_st16_scoped(reinterpret_cast<char*>(sums + nt * 64), smem,
                                make_uint4(__float_as_uint(aw[nt][0]), __float_as_uint(aw[nt][1]), __float_as_uint(aw[nt][2]), __float_as_uint(aw[nt][3])));
            prev_st = 0;                                    // nothing was stored: only the DMA is in flight
            continue;
        }
        // The staging tile has its own LDS here and the barrier at the top of the block loop already separates one block's
        // reads of it from the next block's writes: ONE barrier per epilogue, and a bare one -- __syncthreads() also waits for
        // every LDS-DMA in flight (s_waitcnt vmcnt(0)), i.e. for the next block's patch, in the middle of the epilogue.
        if constexpr (EPI == EPI_FWD) {
            char* st = smem + C64B_STAGE;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int col = wave_n * 32 + c * 16 + (lane >> 4) * 4;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int row = wave_m * 64 + p * 16 + (lane & 15);
                    float v[4] = {acc[c][p][0], acc[c][p][1], acc[c][p][2], acc[c][p][3]};
                    if (ep.relu) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                    }
                    lds_st8_scoped(st + row * 128 + ((((col >> 3) ^ row) & 7) << 4) + (col & 4) * 2, smem,
                        make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])));
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            int t2 = tid;
            asm volatile("" : "+v"(t2));                     // (opaque copy: the store stage recomputes its indices instead of holding them across the MFMA phase)
            staged_store<EPI_FWD, 128, 64, 256, decltype(row_to_m), decltype(pool_index)>(st, g, ep, 0, t2, row_to_m, pool_index);
        } else if (premask) {
            if constexpr (EPI == EPI_DGRAD) {               // staged_epilogue's data-gradient path with the mask already here
                char* st = smem + C64B_STAGE;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int col = wave_n * 32 + c * 16 + (lane >> 4) * 4;
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int row = wave_m * 64 + p * 16 + (lane & 15);
                        lds_st8_scoped(st + row * 128 + ((((col >> 3) ^ row) & 7) << 4) + (col & 4) * 2, smem,
                            make_uint2(pack_bf16x2(acc[c][p][0], acc[c][p][1]),
                                       pack_bf16x2(acc[c][p][2], acc[c][p][3])));
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                int t2 = tid;
                asm volatile("" : "+v"(t2));                 // (opaque copy: keeps the compiler from carrying the indices over from above)
                // the masks are consumed HERE, in uniform control flow: left to the divergent chunks below, the wait for them was
                // re-issued at every join as s_waitcnt vmcnt(0) -- which also waits for the chunk store just issued
                asm volatile("" : "+v"(mk[0]), "+v"(mk[1]), "+v"(mk[2]), "+v"(mk[3]));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int idx = i * 256 + t2, row = idx >> 3, ch = idx & 7;
                    const int m = chunk_pixel(t2, i);
                    if (m < 0) continue;
                    uint4 v = lds_ld16_scoped(st + row * 128 + (((ch ^ row) & 7) << 4), smem);
                    v = gate_bits8(v, mk[i]);
                    *reinterpret_cast<uint4*>(ep.out + (long long)m * ep.ldo + ch * 8) = v;
                }
            }
        } else {
            staged_epilogue<EPI, 128, 64, 2, 4, 256, decltype(row_to_m), decltype(pool_index), false>(
                acc, smem + C64B_STAGE, g, ep, 0, wave_m * 64, wave_n * 32, tid, row_to_m, pool_index);
        }
        // store instructions of that epilogue with at least one active lane (its loop: iteration i, wave w covers the
        // 8 pixels x = 8 (w & 1) .. +7 of block row 2 i + (w >> 1)): a lower bound of what this wave issued after the DMA
        prev_st = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) prev_st += (y0 + 2 * i + (wave >> 1) < g.Ho && x0 + 8 * (wave & 1) < g.Wo) ? 1 : 0;
        if (EPI == EPI_FWD && !ep.out) prev_st = 0;          // pool-only: no full-resolution stores
        // fused pooling: wave w stores pooled row (y0 >> 1) + w, columns (x0 >> 1) .. + 7 (pooled map, then the codes)
        if (EPI == EPI_FWD && ep.pool_out && (y0 >> 1) + wave < ep.pool_h && (x0 >> 1) < ep.pool_w) prev_st += 2;
    }
    if constexpr (W0) {                                     // this workgroup's slab, in the layout of k_conv0_wgrad's
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();
        const float* sm = reinterpret_cast<const float*>(smem + C64B_W0_SUMS);
        auto tile_value = [&](int co, int tap, int ci) {    // D element (row co & 15, column 4 (tap & 3) + ci) of tile (co >> 4, tap >> 2)
            const int l = 16 * ((co & 15) >> 2) + 4 * (tap & 3) + ci;
            return sm[(((co >> 4) * 3 + (tap >> 2)) * 64 + l) * 4 + (co & 3)];
        };
        for (int idx = tid; idx < 64 * 72 + 64; idx += 256) {
            if (idx < 64 * 72) {
                const int co = idx / 72, col = idx - co * 72;
                w0.slab_w[(long long)blockIdx.x * (64 * 72) + idx] = (col & 7) < 3 ? tile_value(co, col >> 3, col & 7) : 0.f;
            } else if (w0.slab_b) {
                w0.slab_b[(long long)blockIdx.x * 64 + (idx - 64 * 72)] = tile_value(idx - 64 * 72, 4, 3);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// First layer, forward: 3x3 / stride 1 / pad 1, 8 input channels (3 image channels + padding), 64 output channels,
// bias + ReLU.  33 us of MFMA work against 830 MB of traffic: the kernel is organised around the stores.  A workgroup
// owns a 16x16 block: the 18x18 halo patch is 5 KB (one 16-byte pixel per DMA lane), the whole [64][72] weight matrix
// lives in registers as MFMA A fragments (k = 4 taps x 8 channels per MFMA, 3 MFMAs cover the 9 taps), every wave
// computes two 16-pixel rows and turns each [16 px][64 ch] result through its private 2 KB of LDS so that it leaves as
// two fully coalesced 1 KiB stores (16 consecutive NHWC pixels are contiguous).
__global__ __launch_bounds__(512) void k_conv0_fwd(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ w,
                                                   const float* __restrict__ bias, bf16_raw* __restrict__ out, ConvGeom g,
                                                   int relu, int tiles_x, int tiles_y, unsigned char* __restrict__ relu_bits) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 6 * 1024 + 8 * 2048];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nblocks = g.B * tiles_x * tiles_y;
    // persistent: blocks blockIdx.x, + gridDim.x, ...; the next block's patch is in flight while this one is computed
    auto issue_patch = [&](int t, int buf) {
        if (wave < 6) {                                     // one pixel per lane, row-major 18x18
            int r = t;
            const int tx = r % tiles_x; r /= tiles_x;
            const int ty = r % tiles_y;
            const int b = r / tiles_y;
            const int pp = wave * 64 + lane;
            const int py = pp / PATCH_W, px = pp - py * PATCH_W;
            const int iy = ty * 16 - 1 + py, ix = tx * 16 - 1 + px;
            const bool ok = pp < PATCH_PIX && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            const bf16_raw* src = ok ? x + (unsigned)((b * g.H + iy) * g.W + ix) * 8u : reinterpret_cast<const bf16_raw*>(g_zero16);
            __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(smem + buf * 6144 + wave * 1024), 16, 0, 0);
        }
    };
    if ((int)blockIdx.x < nblocks) issue_patch(blockIdx.x, 0);
    // weights as A fragments: lane (row = lane & 15, k chunk fk = lane >> 4) of tile c, k-step ks holds
    // w[c*16 + row][tap = 4 ks + fk][0..7]
    const int frow = lane & 15, fk = lane >> 4;
    bf16x8_t fw[4][3];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            const int tap = 4 * ks + fk, co = c * 16 + frow;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (tap < 9 && co < g.N) v = *reinterpret_cast<const uint4*>(w + (unsigned)co * 72u + (unsigned)tap * 8u);
            fw[c][ks] = *reinterpret_cast<const bf16x8_t*>(&v);
        }
    float b4[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int n = c * 16 + fk * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) b4[c][j] = (bias && n + j < g.N) ? bias[n + j] : 0.f;
    }
    // pixel fragment of k-step ks: lane (pixel = lane & 15, fk) reads the patch pixel shifted by tap 4 ks + fk
    int toff[3];
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) {
        int tap = 4 * ks + fk;
        if (tap > 8) tap = 8;                               // weights of the missing taps are zero
        toff[ks] = ((tap / 3) * PATCH_W + tap % 3 + frow) * 16;
    }
    char* stage = smem + 2 * 6144 + wave * 2048;
    int it = 0, prev_st = 0;
    for (int t = blockIdx.x; t < nblocks; t += gridDim.x, ++it) {
        const int cur = it & 1;
        // the patch DMA of this block is older than the stores this wave issued since: leave those in flight.  prev_st
        // counts only the store instructions that had at least one active lane (wave-uniform), i.e. a lower bound
        if (prev_st >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else if (prev_st == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        else if (prev_st == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else if (prev_st == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + (int)gridDim.x < nblocks) issue_patch(t + gridDim.x, cur ^ 1);
        int r = t;
        const int tx = r % tiles_x; r /= tiles_x;
        const int ty = r % tiles_y;
        const int b = r / tiles_y;
        const int y0 = ty * 16, x0 = tx * 16;
        const char* patch = smem + cur * 6144;
        prev_st = 0;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int h = 0; h < 2; ++h) prev_st += (y0 + 2 * wave + p < g.Ho && x0 + 8 * h < g.Wo) ? 1 : 0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int row = 2 * wave + p;                   // block row of this pixel tile
            bf16x8_t fx[3];
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) fx[ks] = *reinterpret_cast<const bf16x8_t*>(patch + row * (PATCH_W * 16) + toff[ks]);
            f32x4_t acc[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < 3; ++ks) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[c][ks], fx[ks], acc[c], 0, 0, 0);
            }
            // lane holds channels c*16 + fk*4 + {0..3} of pixel frow: bias, ReLU, pack, into the wave's staging tile
            // [16 px][128 B] with the 16-byte chunk index XORed by (px & 7)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float v[4] = {acc[c][0] + b4[c][0], acc[c][1] + b4[c][1], acc[c][2] + b4[c][2], acc[c][3] + b4[c][3]};
                if (relu) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
                }
                // (scoped: a plain LDS store here waits for the next block's patch DMA and, with it, for every store of the
                //  previous row -- s_waitcnt vmcnt(0) twice per block in a kernel that lives on its stores)
                lds_st8_scoped(stage + frow * 128 + (((c * 2 + (fk >> 1)) ^ (frow & 7)) << 4) + (fk & 1) * 8, smem,
                    make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])));
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // same wave wrote it: no barrier needed
            const int y = y0 + row;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int idx = h * 64 + lane;
                const int px = idx >> 3, ch = idx & 7;
                const uint4 v = lds_ld16_scoped(stage + px * 128 + ((ch ^ (px & 7)) << 4), smem);
                const int xx = x0 + px;
                if (y < g.Ho && xx < g.Wo) {        // N == 64 (host check): every chunk of the pixel is stored
                    *reinterpret_cast<uint4*>(out + ((unsigned)((b * g.Ho + y) * g.Wo + xx) * 64u + (unsigned)(ch * 8))) = v;
                    if (relu_bits) relu_bits[(unsigned)((b * g.Ho + y) * g.Wo + xx) * 8u + (unsigned)ch] = (unsigned char)relu_bits8(v);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging tile is reused by the second row
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Dispatch.  igemm_plan decides -- kernel, tiling, grid, refusal -- from values alone; launch_igemm launches what the plan says
// and the queries at the end of the file answer from the same plan.  A dispatch rule is changed in igemm_plan and nowhere else.
struct IgemmPlan {
    int id;                                  // SSD_PLAN_* kernel
    int flags;                               // SSD_PLAN_F_*
    unsigned grid;                           // workgroups launched (the implicit GEMMs: x, with y = ksplit); 0: k_pw_gemm sizes its own launch
    int wgs;                                 // ACTIVE workgroups (the grid minus those that return at once); -1: not known (k_pw_gemm)
    int lds;                                 // dynamic LDS bytes
    // pixel-block kernels (conv0, c64b, patch32, p512)
    int tiles_x, tiles_y;                    // blocks across a map (16 columns each) and down it (c64b: 8 rows, patch32 / conv0: 16, p512: 32)
    int nblocks;                             // pixel blocks of the launch (patch32 / p512: per channel tile)
    int rowflat;                             // patch32 / p512: one strip of rows over all images
    int pitch;                               // patch32 / p512: image pitch of that strip in rows, for ConvGeom::d_h1
    // implicit GEMMs (8-phase, LDS-DMA)
    int bm, bn, ksplit;
    unsigned ntm, ntn;
    int word() const { return id | flags; }  // what the ssd_conv2d_*_plan queries answer
};

// k_conv3x3_c64b: 8 x 16 pixel blocks walked by at most max_wgs persistent workgroups; returns the grid
unsigned c64b_tiling(int B, int H, int W, int max_wgs, int* tiles_x, int* tiles_y) {
    *tiles_x = (W + 15) / 16; *tiles_y = (H + C64B_ROWS - 1) / C64B_ROWS;
    const int nblocks = B * *tiles_x * *tiles_y;
    return (unsigned)(nblocks < max_wgs ? nblocks : max_wgs);
}

bool staged_ok_host(int epi, const ConvGeom& g, const EpiArgs& ep) {   // staged_ok (conv_common.h) of a launch without split-K
    return epi == EPI_HEAD || ((g.N & 7) == 0 && (ep.ldo & 7) == 0);
}

// SSD_OK and *p, or the status the call is refused with (nothing launched).  Reads no pointer.
//   epi, g, ep           EPI_* kind, geometry and epilogue facts of the call, after the entry's own argument checks (rule 1)
//   takes_pool           the caller can use a pooling epilogue (ssd_conv2d_fwd_pool)
//   plain_fwd            the call came in through ssd_conv2d_fwd / ssd_conv2d_fwd_relubits
//   has_ws, ws_bytes     the caller's workspace (split-K)
// The rules below are in the order that decides which of them wins and which status a refused call gets.
int igemm_plan(int epi, const ConvGeom& g, const EpiArgs& ep, bool takes_pool, bool plain_fwd, bool has_ws, size_t ws_bytes,
               IgemmPlan* p) {
    *p = IgemmPlan{};
    p->ksplit = 1;
    p->pitch = g.H + 1;
    const bool same3x3 = g.KH == 3 && g.KW == 3 && g.mul == 1 && g.div == 1 && g.pad_t == 1 && g.pad_l == 1 && g.H == g.Ho &&
                         g.W == g.Wo && g.H >= 16 && g.W >= 16;
    p->tiles_x = (g.Wo + 15) / 16; p->tiles_y = (g.Ho + 15) / 16;

    // ---- 2. the image layer: k_conv0_fwd, through the plain forward entry only ----
    if (plain_fwd && ssd_knob("SSD_CONV_FIRST", 1) && same3x3 && g.C == 8 && g.N == 64) {
        p->id = SSD_PLAN_CONV0_FWD;
        p->nblocks = g.B * p->tiles_x * p->tiles_y;
        p->wgs = p->nblocks < 768 ? p->nblocks : 768;
        p->grid = (unsigned)p->wgs;
        return SSD_OK;
    }

    // ---- 3. 64 -> 64: k_conv3x3_c64b, two workgroups per CU (not for the heads) ----
    if (epi != EPI_HEAD && ssd_knob("SSD_CONV_C64", 1) && same3x3 && g.C == 64 && g.N == 64 && g.ldw == 576 && !ep.accumulate &&
        !ep.up_out && (ep.ldo & 7) == 0 && (long long)g.B * g.H * g.W * 64 < (1ll << 31) - 16) {
        const bool pool = takes_pool && ep.pool_out;
        if (epi == EPI_FWD && !ep.out && !pool) return SSD_ERR_VALUE;
        p->id = SSD_PLAN_C64B;
        p->flags = pool ? SSD_PLAN_F_POOL_FUSED : 0;
        p->grid = c64b_tiling(g.B, g.Ho, g.Wo, ssd_knob("SSD_C64B_WGS", 512), &p->tiles_x, &p->tiles_y);
        p->nblocks = g.B * p->tiles_x * p->tiles_y;
        p->wgs = (int)p->grid;
        p->lds = C64B_LDS;
        return SSD_OK;
    }

    // ---- 4. LDS-patch family: 3x3 / stride 1 / pad 1 with N <= SSD_CONV_PATCH (default 256); beyond 128 channels only when
    // the 16x16 blocks waste little of the map (75x75 and larger: <= 14 %; 38x38 would waste 37 %) ----
    const int use_patch = ssd_knob("SSD_CONV_PATCH", 256);
    const bool patch_fits = g.N <= 128 || (long long)p->tiles_x * p->tiles_y * 256 * 4 <= (long long)g.Wo * g.Ho * 5;
    // narrow maps: strip blocks, any channel count.  The patch of 256 + 2 (W + 2) positions has to fit the 341 pixel rows of
    // a 32 KB buffer; the bound on W dates from the strip's first form (row pitch W + 2, 256 + 2 (W + 3) positions) and stays:
    // which layers take the strip form is part of the tested dispatch
    const int flat_knob = ssd_knob("SSD_CONV_PATCH_FLAT", 1);
    const bool flat = flat_knob && g.W <= 39 && g.W >= 16 && g.H >= 16 && (flat_knob >= 2 || !patch_fits || g.N > use_patch);
    if (same3x3 && g.C % 64 == 0 && ((g.N <= use_patch && patch_fits) || flat) &&
        (long long)g.B * g.H * g.W * g.C < (1ll << 31) - 16 && (long long)g.N * g.ldw < (1ll << 31) - 16) {   // 31-bit buffer offsets
        const bool can_pool = takes_pool && ep.pool_out && !flat && (g.N & 7) == 0 && (ep.ldo & 7) == 0 && !(g.ablate & 8);
        if (epi == EPI_FWD && !ep.out && !can_pool) return SSD_ERR_VALUE;
        if ((ep.up_out || ep.relu_bits || ep.mask_bits) && (!staged_ok_host(epi, g, ep) || (g.ablate & 8)))
            return SSD_ERR_UNSUPPORTED;                          // un-pooling and the sign bits live in the staged store
        // k_conv3x3_p512, 512 px x 128 channels, one workgroup per CU: from 256 input channels on (eight 32-channel chunks amortise
        // its longer prologue / epilogue; measured per layer in DESIGN.md section 9).  SSD_CONV_P512: 0 never, 1 (default) that rule,
        // 2 always
        // (the heads never take it.  Head 0, 38x38 x 512 channels: its element-wise scatter epilogue has nothing to hide
        //  behind with one workgroup per CU, 385 vs 334 us.  Head 1, 19x19 x 1024 channels, is 208 vs 222 us ALONE -- but it
        //  runs beside the extras' chain of small launches, and a 512-pixel workgroup holds 152 of the CU's 160 KB of LDS:
        //  not one of those launches (64 KB each) found a CU until it had drained, 190 us for a 15-GFLOP layer and the
        //  loss 130 us later.  With the 78 KB workgroups of the patch kernel the two overlap: -0.07 ms per step.)
        const int p512_knob = ssd_knob("SSD_CONV_P512", 1);
        const bool p512 = p512_knob && g.N > 64 && (p512_knob >= 2 || (epi != EPI_HEAD && g.C >= 256));
        const int rows = p512 ? 32 : 16;                         // block = rows x 16 pixels, or rows * 16 strip positions
        p->bn = p512 || g.N > 64 ? 128 : 64;
        p->id = p512 ? SSD_PLAN_P512 : (p->bn == 64 ? SSD_PLAN_P32_64 : SSD_PLAN_P32_128);
        p->lds = p512 ? P5_LDS : 2 * P32_PATCH + 2 * 128 * 64;   // patch32: BN = 64 stages two taps per step
        p->tiles_y = (g.Ho + rows - 1) / rows;
        // wide maps: one strip of rows over all images ("rowflat") when that needs fewer blocks.  Image pitch in strip rows:
        // H + 1 (one shared zero row); under fused pooling the next even number, so that a 2x2 window never straddles two
        // images -- nor two blocks, which start at multiples of 16 / 32 strip rows
        p->pitch = (epi == EPI_FWD && ep.pool_out && (g.H & 1) == 0) ? g.H + 2 : g.H + 1;
        const unsigned strips = (unsigned)(((long long)g.B * p->pitch + rows - 1) / rows);
        p->rowflat = (!flat && ssd_knob("SSD_CONV_PATCH_ROWFLAT", 1) && strips < (unsigned)(p->tiles_y * g.B)) ? 1 : 0;
        const unsigned nb = flat ? (unsigned)(((long long)g.B * (g.H + 1) * (g.W + 1) + rows * 16 - 1) / (rows * 16))
                                 : (p->rowflat ? strips * (unsigned)p->tiles_x : (unsigned)(p->tiles_x * p->tiles_y * g.B));
        p->nblocks = (int)nb;
        p->ntn = (unsigned)((g.N + p->bn - 1) / p->bn);
        p->flags = (flat ? SSD_PLAN_F_FLAT : 0) | (p->rowflat ? SSD_PLAN_F_ROWFLAT : 0) | (can_pool ? SSD_PLAN_F_POOL_FUSED : 0);
        p->wgs = (int)(nb * p->ntn);
        p->grid = 8 * p->ntn * ((nb + 7) / 8);
        return SSD_OK;
    }

    // ---- 5. outside the patch family nothing pools or un-pools in its epilogue ----
    if (epi == EPI_FWD && !ep.out) return SSD_ERR_VALUE;         // pool-only needs a pooling kernel
    if (ep.up_out) return SSD_ERR_UNSUPPORTED;

    // ---- 6. 1x1 / stride 1 on a large map: the persistent GEMM (pwgemm.hip) -- the DMA stream runs on across tile boundaries
    // (SSD_CONV_PW: bit 0 forward, bit 1 data gradient) ----
    if (epi != EPI_HEAD && (ssd_knob("SSD_CONV_PW", 3) & (epi == EPI_FWD ? 1 : 2)) && !(g.ablate & 8) && ssd_pw_gemm_serves(epi, &g, &ep)) {
        p->id = SSD_PLAN_PW;
        p->wgs = -1;
        return SSD_OK;
    }

    // ---- 7. implicit GEMM.  Tile choice: the CU ingests ~28 B/clk from L2, so MACs per staged byte decide the ceiling: prefer the
    // largest tile that still gives every CU work (>= ~2 workgroups per CU), SSD_CONV_TILE overrides (testing) ----
    const int force = ssd_knob("SSD_CONV_TILE", 0);
    const long long wg_256 = (long long)((g.M + 255) / 256);
    int bm = 128, bn = g.N <= 64 ? 64 : 128;
    const long long pad256 = (long long)((g.N + 255) / 256) * 256, pad128 = (long long)((g.N + 127) / 128) * 128;
    // (>= 352 rather than 384 workgroups: at 364 -- the 19x19 maps with 1024 channels -- the 8-phase kernel's deeper
    //  pipeline beats the 256x128 kernel's better fill by 12 %.  A third / fourth LDS stage in k_conv_igemm_dma itself was
    //  tried for the skinny layers and was neutral to 60 % slower: not the DMA latency bounds them)
    if (g.N > 128 && wg_256 * ((g.N + 255) / 256) >= 352 && pad256 * 4 <= pad128 * 5) { bm = 256; bn = 256; }
    else if (g.N > 64 && wg_256 * ((g.N + 127) / 128) >= 384) { bm = 256; bn = 128; }
    else if (g.N <= 64 && wg_256 >= 384) { bm = 256; bn = 64; }
    if (force == 1) { bm = 128; bn = g.N <= 64 ? 64 : 128; }
    if ((force == 2 || force == 4) && g.N > 128) { bm = 256; bn = 256; }   // (4: the LDS-DMA kernel instead of the 8-phase one)
    if (force == 3 && g.N > 64) { bm = 256; bn = 128; }
    // split-K for skinny problems (few tiles, long k loop): partial sums to the caller's workspace
    {
        const long long tiles = (long long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn);
        const int nks_all = g.s2 ? 0 : (g.nchunks + 7) / 8;
        if (ssd_knob("SSD_SPLITK", 1) && has_ws && tiles < 160 && nks_all >= 8) {
            long long want = (256 + tiles - 1) / tiles;
            if (want > nks_all / 2) want = nks_all / 2;
            if (want > 32) want = 32;
            while (want > 1 && (size_t)want * g.M * g.N * sizeof(float) > ws_bytes) --want;
            if (want > 1) p->ksplit = (int)want;
        }
    }
    // the sign bits are written / read by the staged store only (not by the split-K finalize or the scattered epilogue)
    if ((ep.relu_bits || ep.mask_bits) && (p->ksplit > 1 || !staged_ok_host(epi, g, ep) || (g.ablate & 8))) return SSD_ERR_UNSUPPORTED;
    p->bm = bm; p->bn = bn;
    p->ntm = (unsigned)((g.M + bm - 1) / bm);
    p->ntn = (unsigned)((g.N + bn - 1) / bn);
    if (bm == 256 && bn == 256 && force != 4 && !g.s2 && p->ksplit == 1 && g.cpt >= 8 &&
        (long long)g.B * g.H * g.W * g.C < (1ll << 31) - 16 && (long long)g.N * g.ldw < (1ll << 31) - 16) {
        p->id = SSD_PLAN_8PH;
        p->lds = 131072;
    } else {
        p->id = bm == 256 ? (bn == 256 ? SSD_PLAN_DMA_256_256 : (bn == 128 ? SSD_PLAN_DMA_256_128 : SSD_PLAN_DMA_256_64))
                          : (bn == 64 ? SSD_PLAN_DMA_128_64 : SSD_PLAN_DMA_128_128);
        p->flags = (p->ksplit > 1 ? SSD_PLAN_F_SPLITK : 0) | (g.s2 ? SSD_PLAN_F_S2 : 0);
        p->lds = 2 * (bm + bn) * 128;
        if (g.s2) { p->ntm = 0; for (int c = 0; c < 4; ++c) p->ntm += (unsigned)((g.cls_n[c] + bm - 1) / bm); }   // whole tiles per parity class
    }
    p->wgs = (int)(p->ntm * p->ntn * (unsigned)p->ksplit);
    p->grid = 8 * p->ntn * ((p->ntm + 7) / 8);
    return SSD_OK;
}

// ---- one launch helper per kernel family; launch_igemm's switch picks the template arguments.  SSD_ERR_LAUNCH when the
// kernel's LDS size cannot be registered, else SSD_OK (the launch itself is checked by the caller) ----
template <int EPI, bool W0>
int launch_c64b(unsigned grid, int lds, const bf16_raw* x, const bf16_raw* w, const ConvGeom& g, const Epilogue& ep, int tiles_x,
                int tiles_y, const C64W0& w0, hipStream_t s) {
    auto kern = k_conv3x3_c64b<EPI, W0>;
    static OnceLds set; if (ensure_lds(set, reinterpret_cast<const void*>(kern), lds) != 0) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, x, w, g, ep, tiles_x, tiles_y, w0);
    return SSD_OK;
}

template <auto KERN>                         // k_conv3x3_patch32<BN, EPI, FLAT> or k_conv3x3_p512<EPI, FLAT>
int launch_patch(const IgemmPlan& p, const bf16_raw* x, const bf16_raw* w, const ConvGeom& g, const Epilogue& ep, hipStream_t s) {
    ConvGeom gk = g;                         // what the kernel gets: g with the row strip's image pitch
    gk.d_h1 = make_fastdiv(p.pitch);
    if (!ssd_knob("SSD_EPI_PREFETCH", 1)) gk.ablate |= EPI_NO_PREFETCH;   // dev: the store stage without its LDS side tables
    auto kern = KERN;
    static OnceLds set; if (ensure_lds(set, reinterpret_cast<const void*>(kern), p.lds) != 0) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(512), p.lds, s, x, w, gk, ep, p.tiles_x, p.tiles_y, p.nblocks, p.rowflat);
    return SSD_OK;
}

template <int BM, int BN, int EPI>
int launch_dma(const IgemmPlan& p, const bf16_raw* x, const bf16_raw* w, const ConvGeom& g, const Epilogue& ep, hipStream_t s) {
    constexpr int PT = (BM == 256 && BN == 256) ? SSD_PT256 : 4;
    constexpr int NT = (BM / (16 * PT)) * (BN >= 128 ? BN / 64 : 2) * 64;
    auto kern = k_conv_igemm_dma<BM, BN, EPI, PT>;
    if (p.lds > 65536) {
        static OnceLds set; if (ensure_lds(set, reinterpret_cast<const void*>(kern), p.lds) != 0) return SSD_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(kern, dim3(p.grid, (unsigned)p.ksplit), dim3(NT), p.lds, s, x, w, g, ep);
    return SSD_OK;
}

template <int EPI, int ABL>
int launch_8ph(const IgemmPlan& p, const bf16_raw* x, const bf16_raw* w, const ConvGeom& g, const Epilogue& ep, hipStream_t s) {
    auto kern = k_conv_igemm_8ph<EPI, ABL>;
    static OnceLds set; if (ensure_lds(set, reinterpret_cast<const void*>(kern), p.lds) != 0) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(512), p.lds, s, x, w, g, ep);
    return SSD_OK;
}

// Plan the call, launch the plan.  *pooled (ssd_conv2d_fwd_pool): the launch pooled in its epilogue.
template <int EPI>
int launch_igemm(const void* x, const void* w, const ConvGeom& g, const Epilogue& ep_in, hipStream_t s, void* ws, size_t ws_bytes,
                 bool* pooled = nullptr, bool plain_fwd = false) {
    IgemmPlan p;
    int rc = igemm_plan(EPI, g, epi_args(ep_in), pooled != nullptr, plain_fwd, ws != nullptr, ws_bytes, &p);
    if (rc != SSD_OK) return rc;
    const bf16_raw* xp = static_cast<const bf16_raw*>(x);
    const bf16_raw* wp = static_cast<const bf16_raw*>(w);
    Epilogue ep = ep_in;
    ep.slab = p.ksplit > 1 ? static_cast<float*>(ws) : nullptr;
    ep.ksplit = p.ksplit;
    const bool flat = p.flags & SSD_PLAN_F_FLAT;
    switch (p.id) {
        case SSD_PLAN_CONV0_FWD:
            if constexpr (EPI == EPI_FWD)
                hipLaunchKernelGGL(k_conv0_fwd, dim3(p.grid), dim3(512), 0, s, xp, wp, ep.bias, ep.out, g, ep.relu, p.tiles_x, p.tiles_y,
                                   ep.relu_bits);
            break;
        case SSD_PLAN_C64B:
            if constexpr (EPI != EPI_HEAD) rc = launch_c64b<EPI, false>(p.grid, p.lds, xp, wp, g, ep, p.tiles_x, p.tiles_y, C64W0{}, s);
            break;
        case SSD_PLAN_P32_64:
            rc = flat ? launch_patch<k_conv3x3_patch32<64, EPI, true>>(p, xp, wp, g, ep, s)
                      : launch_patch<k_conv3x3_patch32<64, EPI, false>>(p, xp, wp, g, ep, s);
            break;
        case SSD_PLAN_P32_128:
            rc = flat ? launch_patch<k_conv3x3_patch32<128, EPI, true>>(p, xp, wp, g, ep, s)
                      : launch_patch<k_conv3x3_patch32<128, EPI, false>>(p, xp, wp, g, ep, s);
            break;
        case SSD_PLAN_P512:
            rc = flat ? launch_patch<k_conv3x3_p512<EPI, true>>(p, xp, wp, g, ep, s)
                      : launch_patch<k_conv3x3_p512<EPI, false>>(p, xp, wp, g, ep, s);
            break;
        case SSD_PLAN_PW: return ssd_pw_gemm_launch(EPI, x, w, &g, &ep, s);
        case SSD_PLAN_8PH:
#ifdef SSD_DEV_ABLATE
            if constexpr (EPI == EPI_FWD) {
                switch (g.ablate) {
                    case 1: rc = launch_8ph<EPI, 1>(p, xp, wp, g, ep, s); break;
                    case 4: rc = launch_8ph<EPI, 4>(p, xp, wp, g, ep, s); break;
                    case 5: rc = launch_8ph<EPI, 5>(p, xp, wp, g, ep, s); break;
                    case 20: rc = launch_8ph<EPI, 20>(p, xp, wp, g, ep, s); break;
                    case 21: rc = launch_8ph<EPI, 21>(p, xp, wp, g, ep, s); break;
                    case 23: rc = launch_8ph<EPI, 23>(p, xp, wp, g, ep, s); break;
                    default: rc = launch_8ph<EPI, 0>(p, xp, wp, g, ep, s); break;
                }
                break;
            }
#endif
            rc = launch_8ph<EPI, 0>(p, xp, wp, g, ep, s);
            break;
        case SSD_PLAN_DMA_256_256: rc = launch_dma<256, 256, EPI>(p, xp, wp, g, ep, s); break;
        case SSD_PLAN_DMA_256_128: rc = launch_dma<256, 128, EPI>(p, xp, wp, g, ep, s); break;
        case SSD_PLAN_DMA_256_64: rc = launch_dma<256, 64, EPI>(p, xp, wp, g, ep, s); break;
        case SSD_PLAN_DMA_128_64: rc = launch_dma<128, 64, EPI>(p, xp, wp, g, ep, s); break;
        default: rc = launch_dma<128, 128, EPI>(p, xp, wp, g, ep, s); break;   // SSD_PLAN_DMA_128_128
    }
    if (rc != SSD_OK) return rc;
    if (p.ksplit > 1) {
        if (hipGetLastError() != hipSuccess) return SSD_ERR_LAUNCH;
        const long long nthr = (long long)g.M * ((g.N + 3) / 4);
        hipLaunchKernelGGL(k_igemm_finalize<EPI>, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, g, ep);
    }
    if (p.flags & SSD_PLAN_F_POOL_FUSED) *pooled = true;
    return ssd_launch_status();
}

// ---- the geometry of a call, per entry, after the entry's checks of its sizes (SSD_ERR_VALUE): the entry and its query share it ----
int fwd_geom(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, ConvGeom* g) {
    if (!geom_ok(B, H, W, Cin, Ho, Wo, Cout, ksize) || stride <= 0) return SSD_ERR_VALUE;
    *g = make_geom(B, H, W, Cin, Ho, Wo, Cout, ksize, ksize, stride, 1, pad_t, pad_l);
    return SSD_OK;
}

int fwd_pool_geom(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int Hp, int Wp,
                  ConvGeom* g) {
    if (Cout % 8) return SSD_ERR_VALUE;
    if ((Hp != Ho / 2 && Hp != (Ho + 1) / 2) || (Wp != Wo / 2 && Wp != (Wo + 1) / 2) || Hp <= 0 || Wp <= 0) return SSD_ERR_VALUE;
    return fwd_geom(B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, g);
}

int head_geom(int B, int H, int W, int Cin, int per_cell, int classes, ConvGeom* g) {
    const int N = per_cell * (4 + classes);
    if (!geom_ok(B, H, W, Cin, H, W, N, 3) || per_cell <= 0 || classes <= 0) return SSD_ERR_VALUE;
    *g = make_geom(B, H, W, Cin, H, W, N, 3, 3, 1, 1, 1, 1);   // 3x3 SAME stride 1 (models/ssd_model.py:155-162)
    return SSD_OK;
}

// dy: [B,Ho,Wo,Cout_pad] is the source, dx: [B,H,W,Cin] the destination
int bwd_data_geom(int B, int H, int W, int Cin, int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, ConvGeom* g) {
    if (!geom_ok(B, Ho, Wo, Cout_pad, H, W, Cin, ksize) || stride <= 0) return SSD_ERR_VALUE;
    *g = make_geom(B, Ho, Wo, Cout_pad, H, W, Cin, ksize, ksize, 1, stride, ksize - 1 - pad_t, ksize - 1 - pad_l);
    return SSD_OK;
}

// ssd_conv2d_bwd_data_unpool: the pooled map [B,H,W,Cin] against the map before the pooling [B,Hf,Wf,Cin], then the geometry of
// the 3x3 / stride 1 / pad 1 data gradient in front of the un-pooling store
int unpool_geom(int B, int H, int W, int Cin, int Cout_pad, int Hf, int Wf, ConvGeom* g) {
    if (Cin % 8 || Hf <= 0 || Wf <= 0) return SSD_ERR_VALUE;
    if ((H != Hf / 2 && H != (Hf + 1) / 2) || (W != Wf / 2 && W != (Wf + 1) / 2)) return SSD_ERR_VALUE;
    if (2 * H < Hf || 2 * W < Wf) return SSD_ERR_UNSUPPORTED;     // VALID pooling of an odd size: the uncovered row / column is not written here
    if ((long long)B * Hf * Wf * Cin >= (1ll << 32)) return SSD_ERR_VALUE;
    return bwd_data_geom(B, H, W, Cin, Cout_pad, 3, 1, 1, 1, H, W, g);
}

// what a query answers from the plan: the plan word, or the ACTIVE workgroups of the (first) launch the call resolves to --
// SSD_ERR_UNSUPPORTED where the plan does not know them (the persistent pointwise GEMM)
int igemm_answer(int epi, const ConvGeom& g, const EpiArgs& ea, bool takes_pool, bool plain_fwd, size_t ws_bytes, int want) {
    IgemmPlan p;                             // want: 0 the plan word, 1 its active workgroups, 2 its dynamic LDS bytes
    const int rc = igemm_plan(epi, g, ea, takes_pool, plain_fwd, ws_bytes != 0, ws_bytes, &p);
    if (rc != SSD_OK) return rc;
    if (want == 0) return p.word();
    if (want == 2) return p.id == SSD_PLAN_PW ? SSD_ERR_UNSUPPORTED : p.lds;
    return p.wgs < 0 ? SSD_ERR_UNSUPPORTED : p.wgs;
}

}  // namespace

extern "C" {

static int conv2d_fwd_impl(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                           int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int relu, void* ws, size_t ws_bytes,
                           void* stream, void* relu_bits = nullptr) {
    ConvGeom g;
    if (!x || !w || !y || fwd_geom(B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, &g) != SSD_OK) return SSD_ERR_VALUE;
    Epilogue ep = {};
    ep.bias = bias; ep.relu = relu; ep.out = static_cast<bf16_raw*>(y); ep.ldo = Cout;
    ep.relu_bits = static_cast<unsigned char*>(relu_bits);
    return launch_igemm<EPI_FWD>(x, w, g, ep, (hipStream_t)stream, ws, ws_bytes, nullptr, true);
}

int ssd_conv2d_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                   int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int relu, void* ws, size_t ws_bytes,
                   void* stream) {
    return conv2d_fwd_impl(x, w, bias, y, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, relu, ws, ws_bytes, stream);
}

int ssd_conv2d_fwd_pool(const void* x, const void* w, const float* bias, void* y, void* y_pool, void* pool_code, int B, int H,
                        int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int relu, int Hp,
                        int Wp, void* ws, size_t ws_bytes, void* stream) {
    ConvGeom g;
    if (!x || !w || !y_pool || !pool_code ||
        fwd_pool_geom(B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, Hp, Wp, &g) != SSD_OK)
        return SSD_ERR_VALUE;
    // y == NULL: the caller has no use for the full-resolution map (nothing but the pooling reads it): served only by the
    // kernels that pool in their epilogue, SSD_ERR_VALUE (before anything is launched) for any other layer shape
    Epilogue ep = {};
    ep.bias = bias; ep.relu = relu; ep.out = static_cast<bf16_raw*>(y); ep.ldo = Cout;
    if (ssd_knob("SSD_CONV_POOL_FUSE", 1)) {
        ep.pool_out = static_cast<bf16_raw*>(y_pool); ep.pool_code = static_cast<unsigned*>(pool_code); ep.pool_h = Hp; ep.pool_w = Wp;
    }
    bool pooled = false;
    const int rc = launch_igemm<EPI_FWD>(x, w, g, ep, (hipStream_t)stream, ws, ws_bytes, &pooled);
    if (rc != SSD_OK || pooled) return rc;
    // this layer is not served by a 16x16-block kernel: pool in a second launch
    return ssd_maxpool2x2_fwd_argmax(y, y_pool, pool_code, B, Ho, Wo, Cout, Hp, Wp, stream);
}

int ssd_conv2d_head_fwd(const void* x, const void* w, const float* bias, void* loc, void* conf, int B, int H, int W,
                        int Cin, int per_cell, int classes, int anchors_total, int level_off, void* ws, size_t ws_bytes,
                        void* stream) {
    ConvGeom g;
    if (!x || !w || !loc || !conf || head_geom(B, H, W, Cin, per_cell, classes, &g) != SSD_OK) return SSD_ERR_VALUE;
    Epilogue ep = {};
    ep.bias = bias; ep.loc = static_cast<bf16_raw*>(loc); ep.conf = static_cast<bf16_raw*>(conf);
    ep.n_loc = per_cell * 4; ep.n_conf = per_cell * classes; ep.anchors_total = anchors_total;
    ep.level_off = level_off; ep.per_cell = per_cell; ep.classes = classes;
    return launch_igemm<EPI_HEAD>(x, w, g, ep, (hipStream_t)stream, ws, ws_bytes);
}

static int conv2d_bwd_data_impl(const void* dy, const void* w_t, const void* relu_src, void* dx, int B, int H, int W, int Cin,
                                int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int accumulate,
                                void* ws, size_t ws_bytes, void* stream, const void* up_code = nullptr,
                                void* up_dx = nullptr, int up_h = 0, int up_w = 0, const void* mask_bits = nullptr) {
    // dy: [B,Ho,Wo,Cout_pad]; w_t: [Cin][k][k][Cout_pad] (ssd_weight_transpose); dx, relu_src: [B,H,W,Cin]
    ConvGeom g;
    if (!dy || !w_t || (!dx && !up_dx) || bwd_data_geom(B, H, W, Cin, Cout_pad, ksize, stride, pad_t, pad_l, Ho, Wo, &g) != SSD_OK)
        return SSD_ERR_VALUE;
    Epilogue ep = {};
    ep.out = static_cast<bf16_raw*>(dx); ep.ldo = Cin; ep.mask_src = static_cast<const bf16_raw*>(relu_src);
    ep.accumulate = accumulate;
    ep.up_code = static_cast<const unsigned*>(up_code); ep.up_out = static_cast<bf16_raw*>(up_dx); ep.up_h = up_h; ep.up_w = up_w;
    ep.mask_bits = static_cast<const unsigned char*>(mask_bits);
    return launch_igemm<EPI_DGRAD>(dy, w_t, g, ep, (hipStream_t)stream, ws, ws_bytes);
}

int ssd_conv2d_fwd_relubits(const void* x, const void* w, const float* bias, void* y, void* relu_bits, int B, int H, int W, int Cin,
                            int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, void* ws, size_t ws_bytes,
                            void* stream) {
    // ssd_conv2d_fwd with ReLU that also writes the sign bits of its output: relu_bits [B*Ho*Wo][Cout/8] bytes
    if (!relu_bits || Cout % 8) return SSD_ERR_VALUE;
    return conv2d_fwd_impl(x, w, bias, y, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, 1, ws, ws_bytes, stream, relu_bits);
}

int ssd_conv2d_bwd_data_bits(const void* dy, const void* w_t, const void* relu_bits, void* dx, int B, int H, int W, int Cin,
                             int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int accumulate, void* ws,
                             size_t ws_bytes, void* stream) {
    // ssd_conv2d_bwd_data with the ReLU mask given as sign bits ([B*H*W][Cin/8] bytes of ssd_conv2d_fwd_relubits)
    if (!relu_bits || Cin % 8) return SSD_ERR_VALUE;
    return conv2d_bwd_data_impl(dy, w_t, nullptr, dx, B, H, W, Cin, Cout_pad, ksize, stride, pad_t, pad_l, Ho, Wo, accumulate, ws,
                                ws_bytes, stream, nullptr, nullptr, 0, 0, relu_bits);
}

int ssd_conv2d_bwd_data_unpool(const void* dy, const void* w_t, const void* relu_src, const void* pool_code, void* dx_pooled,
                               void* dx_full, int B, int H, int W, int Cin, int Cout_pad, int Hf, int Wf, void* ws, size_t ws_bytes,
                               void* stream) {
    // 3x3 / stride 1 / pad 1 data gradient w.r.t. a POOLED map [B,H,W,Cin], carried on through the 2x2 / stride-2 max pooling
    // that produced the map (pool_code [B,H,W,Cin/8] of ssd_maxpool2x2_fwd_argmax / ssd_conv2d_fwd_pool): dx_full [B,Hf,Wf,Cin]
    if (!pool_code || !dx_full) return SSD_ERR_VALUE;
    ConvGeom g;
    const int rc = unpool_geom(B, H, W, Cin, Cout_pad, Hf, Wf, &g);
    if (rc != SSD_OK) return rc;
    return conv2d_bwd_data_impl(dy, w_t, relu_src, dx_pooled, B, H, W, Cin, Cout_pad, 3, 1, 1, 1, H, W, 0, ws, ws_bytes, stream,
                                pool_code, dx_full, Hf, Wf);
}

int ssd_conv2d_bwd_data(const void* dy, const void* w_t, const void* relu_src, void* dx, int B, int H, int W, int Cin,
                        int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int accumulate,
                        void* ws, size_t ws_bytes, void* stream) {
    return conv2d_bwd_data_impl(dy, w_t, relu_src, dx, B, H, W, Cin, Cout_pad, ksize, stride, pad_t, pad_l, Ho, Wo, accumulate,
                                ws, ws_bytes, stream);
}

// Data gradient of the second layer (64 -> 64, 3x3 / stride 1 / pad 1) fused with the weight gradient of the first
// (8 padded image channels -> 64): k_conv3x3_c64b<EPI_DGRAD, true>.  The gradient w.r.t. the first layer's output never
// reaches memory.  dy [B,H,W,64]; w_t [64][3][3][64] (ssd_weight_transpose of the second layer); relu_bits [B*H*W][8] (sign
// bits of the first layer's output, ssd_conv2d_fwd_relubits); image [B,H,W,8]; dw0 f32 [64][3][3][8] (pad channels: zeros),
// dbias0 f32 [64] or null.  One fp32 slab per workgroup, summed in a fixed order by the reduction kernel.
size_t ssd_conv2d_bwd_data_wgrad_first_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)512 * (64 * 72 + 64) * sizeof(float);
}

int ssd_conv2d_bwd_data_wgrad_first(const void* dy, const void* w_t, const void* relu_bits, const void* image, float* dw0,
                                    float* dbias0, int B, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    if (!dy || !w_t || !relu_bits || !image || !dw0 || B <= 0 || H <= 0 || W <= 0) return SSD_ERR_VALUE;
    if (H < 16 || W < 16 || (long long)B * H * W * 64 >= (1ll << 31) - 16) return SSD_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < ssd_conv2d_bwd_data_wgrad_first_workspace_bytes(B, H, W)) return SSD_ERR_WORKSPACE;
    const ConvGeom g = make_geom(B, H, W, 64, H, W, 64, 3, 3, 1, 1, 1, 1);
    Epilogue ep = {};
    ep.ldo = 64;
    ep.mask_bits = static_cast<const unsigned char*>(relu_bits);
    int tiles_x, tiles_y;
    const unsigned grid = c64b_tiling(B, H, W, 512, &tiles_x, &tiles_y);   // (one workgroup per CU, to run beside the next weight gradient: slower)
    float* slab_w = static_cast<float*>(ws);
    float* slab_b = slab_w + (size_t)512 * 64 * 72;
    hipStream_t s = (hipStream_t)stream;
    const C64W0 w0 = {static_cast<const bf16_raw*>(image), slab_w, dbias0 ? slab_b : nullptr};
    if (launch_c64b<EPI_DGRAD, true>(grid, C64B_W0_LDS, static_cast<const bf16_raw*>(dy), static_cast<const bf16_raw*>(w_t), g, ep,
                                     tiles_x, tiles_y, w0, s) != SSD_OK || hipGetLastError() != hipSuccess)
        return SSD_ERR_LAUNCH;
    ssd_launch_wgrad_reduce(s, slab_w, 64ll * 72, 64ll * 72, dw0, slab_b, 64ll, 64, dbias0, (int)grid);
    return ssd_launch_status();
}

// ---- dispatch queries: the entry's geometry, the epilogue facts of the call the query stands for (bias and ReLU, every output
// the entry requires, no ReLU mask), and igemm_plan's answer.  Nothing is launched and no pointer exists ----
static int conv2d_fwd_query(int want, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho,
                            int Wo, int pool, size_t ws_bytes) {
    ConvGeom g;
    EpiArgs ea = {};
    ea.out = pool != 2;                                          // pool = 2: ssd_conv2d_fwd_pool without y
    ea.ldo = Cout;
    ea.pool_out = pool && ssd_knob("SSD_CONV_POOL_FUSE", 1);
    const int rc = pool ? fwd_pool_geom(B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, (Ho + 1) / 2, (Wo + 1) / 2, &g)
                        : fwd_geom(B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, &g);
    return rc != SSD_OK ? rc : igemm_answer(EPI_FWD, g, ea, pool != 0, pool == 0, ws_bytes, want);
}

static int conv2d_bwd_data_query(int want, int B, int H, int W, int Cin, int Cout_pad, int ksize, int stride, int pad_t, int pad_l,
                                 int Ho, int Wo, int accumulate, size_t ws_bytes) {
    ConvGeom g;
    EpiArgs ea = {};
    ea.out = true; ea.ldo = Cin; ea.accumulate = accumulate;
    const int rc = bwd_data_geom(B, H, W, Cin, Cout_pad, ksize, stride, pad_t, pad_l, Ho, Wo, &g);
    return rc != SSD_OK ? rc : igemm_answer(EPI_DGRAD, g, ea, false, false, ws_bytes, want);
}

int ssd_conv2d_fwd_plan(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo,
                        int pool, size_t ws_bytes) {
    return conv2d_fwd_query(0, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, pool, ws_bytes);
}

int ssd_conv2d_fwd_workgroups(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo,
                              int pool, size_t ws_bytes) {
    return conv2d_fwd_query(1, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, pool, ws_bytes);
}

int ssd_conv2d_head_fwd_plan(int B, int H, int W, int Cin, int per_cell, int classes, size_t ws_bytes) {
    ConvGeom g;
    const int rc = head_geom(B, H, W, Cin, per_cell, classes, &g);
    return rc != SSD_OK ? rc : igemm_answer(EPI_HEAD, g, EpiArgs{}, false, false, ws_bytes, false);
}

int ssd_conv2d_bwd_data_plan(int B, int H, int W, int Cin, int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho,
                             int Wo, int accumulate, size_t ws_bytes) {
    return conv2d_bwd_data_query(0, B, H, W, Cin, Cout_pad, ksize, stride, pad_t, pad_l, Ho, Wo, accumulate, ws_bytes);
}

int ssd_conv2d_bwd_data_unpool_plan(int B, int H, int W, int Cin, int Cout_pad, int Hf, int Wf, int has_relu_src, size_t ws_bytes) {
    ConvGeom g;
    EpiArgs ea = {};
    ea.up_out = true; ea.mask_src = has_relu_src != 0; ea.ldo = Cin;   // (dx_pooled is optional and decides nothing)
    const int rc = unpool_geom(B, H, W, Cin, Cout_pad, Hf, Wf, &g);
    return rc != SSD_OK ? rc : igemm_answer(EPI_DGRAD, g, ea, false, false, ws_bytes, 0);
}

int ssd_conv2d_bwd_data_workgroups(int B, int H, int W, int Cin, int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho,
                                   int Wo, int accumulate, size_t ws_bytes) {
    return conv2d_bwd_data_query(1, B, H, W, Cin, Cout_pad, ksize, stride, pad_t, pad_l, Ho, Wo, accumulate, ws_bytes);
}

int ssd_conv2d_fwd_lds_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo,
                             int pool, size_t ws_bytes) {
    return conv2d_fwd_query(2, B, H, W, Cin, Cout, ksize, stride, pad_t, pad_l, Ho, Wo, pool, ws_bytes);
}

int ssd_conv2d_bwd_data_lds_bytes(int B, int H, int W, int Cin, int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho,
                                  int Wo, int accumulate, size_t ws_bytes) {
    return conv2d_bwd_data_query(2, B, H, W, Cin, Cout_pad, ksize, stride, pad_t, pad_l, Ho, Wo, accumulate, ws_bytes);
}

const char* ssd_conv_plan_name(int plan) {
    switch (plan & SSD_PLAN_KERNEL_MASK) {
        case SSD_PLAN_C64B: return "k_conv3x3_c64b";
        case SSD_PLAN_P32_64: return "k_conv3x3_patch32<64>";
        case SSD_PLAN_P32_128: return "k_conv3x3_patch32<128>";
        case SSD_PLAN_P512: return "k_conv3x3_p512";
        case SSD_PLAN_8PH: return "k_conv_igemm_8ph";
        case SSD_PLAN_PW: return "k_pw_gemm";
        case SSD_PLAN_DMA_256_256: return "k_conv_igemm_dma<256,256>";
        case SSD_PLAN_DMA_256_128: return "k_conv_igemm_dma<256,128>";
        case SSD_PLAN_DMA_256_64: return "k_conv_igemm_dma<256,64>";
        case SSD_PLAN_DMA_128_64: return "k_conv_igemm_dma<128,64>";
        case SSD_PLAN_DMA_128_128: return "k_conv_igemm_dma<128,128>";
        case SSD_PLAN_CONV0_FWD: return "k_conv0_fwd";
        case SSD_PLAN_WG_FIRST: return "k_conv0_wgrad";
        case SSD_PLAN_WG_PATCH_16x16: return "k_conv3x3_wgrad_patch<16,2>";
        case SSD_PLAN_WG_PATCH_6x40: return "k_conv3x3_wgrad_patch<6,5>";
        case SSD_PLAN_WG_PATCH_10x24: return "k_conv3x3_wgrad_patch<10,3>";
        case SSD_PLAN_WG_TILE: return "k_conv_wgrad_tile";
        case SSD_PLAN_WG_GENERIC: return "k_conv_wgrad";
        default: return "?";
    }
}

}  // extern "C"
