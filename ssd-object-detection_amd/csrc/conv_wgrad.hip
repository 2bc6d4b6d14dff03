// Weight gradient of the convolution stack for gfx950 (MI355X): dW[co][kh][kw][ci] (and dbias) from x and dY, NHWC bf16 on MFMA.
//
// Every kernel writes fp32 partial sums ("slabs"), one per pixel split, and a reduction sums them in a fixed order: the result
// is deterministic.  Kernels (DESIGN.md section 4 has the table): k_conv3x3_wgrad_patch (3x3 / stride 1 / pad 1, operands
// resident in LDS, three block shapes), k_conv_wgrad_tile (256x256 GEMM over pixels), k_conv0_wgrad (the image layer),
// k_conv_wgrad (generic 128x128 GEMM; k_conv_wgrad_batched runs several small layers in one launch), k_wgrad_reduce2 (+ _batched)
// and k_wgrad_reduce_wide (the slab sums).  The host side -- one plan per layer, the launches, the C entries -- follows them.
// (The first layer's gradient fused into the second layer's data gradient is k_conv3x3_c64b<EPI_DGRAD, true>, conv.hip.)
#include <cstdint>
#include "common.h"
#include <hip/hip_bf16.h>

#include "conv_common.h"
namespace {

// ------------------------------------------------------------------------------------------------
// Weight gradient.  grid (col tiles, co tiles, splits).  Per step 64 pixels.
constexpr int WG_LD = 288;                   // LDS row stride (bytes) of a [pixel][128 ch] tile: 256 + 32 pad

__device__ __forceinline__ void conv_wgrad_block(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ dy,
                                                 float* __restrict__ slab_w, float* __restrict__ slab_b, const ConvGeom& g,
                                                 int m_per_split, char* smem, const int bidx, const int bidy, const int bidz) {
    // g: source = x dims (B,H,W,C), destination = dy dims (Ho,Wo,N); mul = stride, div = 1
    constexpr int TILE = 64 * WG_LD;
    auto s_dy = [&](int buf) { return smem + buf * (2 * TILE); };
    auto s_x = [&](int buf) { return smem + buf * (2 * TILE) + TILE; };

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_m = wave & 1, wave_n = wave >> 1;       // m: co, n: (tap,ci) columns
    const int col0 = bidx * 128, co0 = bidy * 128;
    const int ktot = g.ldw;                                 // KH*KW*C columns
    const int m_begin = bidz * m_per_split;
    const int m_end = min(g.M, m_begin + m_per_split);

    const int cslot = tid & 15, prow = tid >> 4;           // 16-byte column chunk, pixel row (+16j)
    // this thread's X column chunk -> (tap, channel)
    const int qx = (col0 >> 3) + cslot;
    const bool xcol_ok = qx < g.nchunks;
    const int tapx = xcol_ok ? qx / g.cpt : 0;
    const int ccx = qx - tapx * g.cpt;
    const int khx = tapx / g.KW, kwx = tapx - khx * g.KW;
    const int co_chunk = co0 + cslot * 8;
    const bool dycol_ok = co_chunk < g.N;

    uint4 rdy[4], rxx[4];
    auto load_tiles = [&](int mstep) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = mstep + prow + 16 * j;
            const bool mok = m < m_end;
            rdy[j] = make_uint4(0, 0, 0, 0);
            rxx[j] = make_uint4(0, 0, 0, 0);
            if (mok && dycol_ok) rdy[j] = *reinterpret_cast<const uint4*>(dy + ((long long)m * g.N + co_chunk));
            if (mok && xcol_ok) {
                const int b = fdiv(m, g.d_hw);
                const int rem = m - b * g.d_hw.d;
                const int oy = fdiv(rem, g.d_w);
                const int ox = rem - oy * g.d_w.d;
                const int iy = oy * g.mul - g.pad_t + khx, ix = ox * g.mul - g.pad_l + kwx;
                if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
                    rxx[j] = *reinterpret_cast<const uint4*>(x + ((((long long)b * g.H + iy) * g.W + ix) * g.C + ccx * 8));
            }
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<uint4*>(s_dy(buf) + (prow + 16 * j) * WG_LD + cslot * 16) = rdy[j];
            *reinterpret_cast<uint4*>(s_x(buf) + (prow + 16 * j) * WG_LD + cslot * 16) = rxx[j];
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
    const bool do_bias = slab_b != nullptr && bidx == 0 && wave_n == 0;
    bf16x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;

    const int nsteps = (m_end - m_begin + 63) / 64;
    if (nsteps > 0) {
        load_tiles(m_begin);
        store_tiles(0);
    }
    __syncthreads();
    // transposing read: lane (16-group gq, index i) supplies the address of k-row (i>>2), columns 4*(i&3)..+3
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
                const char* base = s_dy(cur) + krow * WG_LD + (wave_m * 64 + a * 16 + tr_col) * 2;
                const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base));
                const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base + 4 * WG_LD));
                union { s16x4_t h[2]; bf16x8_t v; } u;
                u.h[0] = lo; u.h[1] = hi;
                fa[a] = u.v;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const char* base = s_x(cur) + krow * WG_LD + (wave_n * 64 + c * 16 + tr_col) * 2;
                const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base));
                const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base + 4 * WG_LD));
                union { s16x4_t h[2]; bf16x8_t v; } u;
                u.h[0] = lo; u.h[1] = hi;
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
    // partial tile -> slab[z][co][col]  (D[row = co (lane>>4)*4+j][col = lane&15])
    float* out = slab_w + (long long)bidz * g.N * ktot;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = col0 + wave_n * 64 + c * 16 + (lane & 15);
            if (col >= ktot) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + wave_m * 64 + a * 16 + (lane >> 4) * 4 + j;
                if (co < g.N) out[(long long)co * ktot + col] = acc[a][c][j];
            }
        }
    if (do_bias && (lane & 15) == 0) {
        float* ob = slab_b + (long long)bidz * g.N;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + wave_m * 64 + a * 16 + (lane >> 4) * 4 + j;
                if (co < g.N) ob[co] = accb[a][j];
            }
    }
}

__global__ __launch_bounds__(WG) void k_conv_wgrad(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ dy,
                                                   float* __restrict__ slab_w, float* __restrict__ slab_b, ConvGeom g,
                                                   int m_per_split) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    conv_wgrad_block(x, dy, slab_w, slab_b, g, m_per_split, smem, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Several small layers' weight gradients in ONE launch (ssd_conv2d_bwd_weight_batched): block b belongs to the layer whose block
// range holds it and runs exactly the block of k_conv_wgrad it would have been there -- same slabs, same sums, bit for bit.
constexpr int WGB_MAX = 8;
struct WgradBatchItem {
    const bf16_raw* x;
    const bf16_raw* dy;
    float* slab_w;
    float* slab_b;
    ConvGeom g;
    int mps, ctiles, mtiles, blk0;
};
struct WgradBatchArgs {
    int count;
    WgradBatchItem it[WGB_MAX];
};
__global__ __launch_bounds__(WG) void k_conv_wgrad_batched(WgradBatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int l = 0;
#pragma unroll
    for (int k = 1; k < WGB_MAX; ++k) l += (k < a.count && (int)blockIdx.x >= a.it[k].blk0) ? 1 : 0;
    const WgradBatchItem& it = a.it[l];
    const int local = (int)blockIdx.x - it.blk0;
    const int per_split = it.ctiles * it.mtiles;
    const int bz = local / per_split, r = local - bz * per_split;
    const int by = r / it.ctiles, bx = r - by * it.ctiles;
    conv_wgrad_block(it.x, it.dy, it.slab_w, it.slab_b, it.g, it.mps, smem, bx, by, bz);
}

// ... and their slab sums in one launch: k_wgrad_reduce2's arithmetic per layer
struct ReduceBatchItem {
    const float* slab_w;
    const float* slab_b;
    float* dw;
    float* db;
    long long sw, nw, sb;
    int nb, ns, blk0;
    unsigned nbw;
};
struct ReduceBatchArgs {
    int count;
    ReduceBatchItem it[WGB_MAX];
};
__global__ __launch_bounds__(256) void k_wgrad_reduce2_batched(ReduceBatchArgs a) {
    int l = 0;
#pragma unroll
    for (int k = 1; k < WGB_MAX; ++k) l += (k < a.count && (int)blockIdx.x >= a.it[k].blk0) ? 1 : 0;
    const ReduceBatchItem& it = a.it[l];
    const unsigned local = blockIdx.x - (unsigned)it.blk0;
    if (local < it.nbw) {
        const long long i = ((long long)local * 256 + threadIdx.x) * 4;
        if (i >= it.nw) return;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int z = 0; z < it.ns; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(it.slab_w + (long long)z * it.sw + i);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4*>(it.dw + i) = s;
    } else {
        const int i = (int)(local - it.nbw) * 256 + threadIdx.x;
        if (i >= it.nb) return;
        float s = 0.f;
        for (int z = 0; z < it.ns; ++z) s += it.slab_b[(long long)z * it.sb + i];
        it.db[i] = s;
    }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient as a plain GEMM over pixels, 256 output channels x 256 (tap, ci) columns per workgroup, 64 pixels
// per step (the 1x1 and the strided layers with >= 256 channels; the 3x3 / stride-1 layers use the patch kernel below).
//   dW[co][col] += sum_m dY[m][co] * Xcol[m][col]
// Both tiles are [pixel][256 channels] images (512-byte rows) filled by buffer LDS-DMA (a lane whose pixel / column is
// padding gets an out-of-range offset = zeros) and read with transposing LDS reads.  The 32-byte column groups of a
// row are XORed with (row & 7): the eight consecutive rows of a half-wave read then hit eight bank groups, and since
// the key has period 8 every read address is a per-lane base + immediate.  Eight waves (2 x 4), each 128 co x 64 cols
// = 32 accumulator tiles, 64 MFMAs per step; two LDS buffers (128 KB), one barrier per step.
// (fragment reads: lds_read_tr16_scoped, conv_common.h)

constexpr int WT_TILE = 64 * 512;                          // one [64 px][256 ch] image
// Four 32-pixel stages (one MFMA k-sub-step each), three stages of DMA in flight behind a COUNTED vmcnt -- the step does not
// wait for the DMA it has just issued, and a stage's latency hides under three sub-steps of MFMAs.
__global__ __launch_bounds__(512) void k_conv_wgrad_tile(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ dy,
                                                         float* __restrict__ slab_w, float* __restrict__ slab_b, ConvGeom g,
                                                         int m_per_split, int nsplit, int cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave & 1, wave_n = wave >> 1;           // 128 channels x 64 columns per wave
    // XCD-aware order when the splits are a multiple of 8: all tiles of one pixel split run consecutively on ONE XCD
    // (workgroup L -> XCD L % 8) and share its rows through that L2; otherwise plain order, which keeps every XCD busy
    const int ktot = g.ldw;
    const int ctiles = (ktot + 255) >> 8, mtiles = (cout + 255) >> 8, tiles = ctiles * mtiles;
    int split, tile;
    if ((nsplit & 7) == 0) {
        const int kx = blockIdx.x >> 3;
        split = (kx / tiles) * 8 + (blockIdx.x & 7);
        tile = kx % tiles;
    } else {
        split = blockIdx.x / tiles;
        tile = blockIdx.x - split * tiles;
    }
    if (split >= nsplit) return;
    const int bx = tile % ctiles, by = tile / ctiles;
    const int col0 = bx * 256, co0 = by * 256;
    const int m_begin = split * m_per_split;
    const int m_end = min(g.M, m_begin + m_per_split);

    // DMA: instruction i (= wave + 8j, j < 4) fills tile rows 2i, 2i+1; lane L -> row 2i + (L>>5), physical chunk L & 31
    const __amdgpu_buffer_rsrc_t dyres = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, (unsigned)g.M * (unsigned)g.N * 2u, 0x00020000);
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (unsigned)g.B * g.H * g.W * g.C * 2u, 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    const int drow = lane >> 5;
    int rowj[4];
    unsigned dycol[4], xcol[4];                                // byte offset of the lane's chunk inside a pixel row, OOB if padding
    int xkh[4], xkw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int row = 2 * (wave + 8 * j) + drow;
        rowj[j] = row;
        const int pc = lane & 31;                              // physical 16-byte chunk
        const int lg = ((pc >> 1) & 8) | (((pc >> 1) ^ row) & 7);   // logical 32-byte group
        const int ch = (lg * 2 + (pc & 1)) * 8;                // channel / column of the tile
        dycol[j] = co0 + ch < g.N ? (unsigned)(co0 + ch) * 2u : OOB;
        const int q = (col0 + ch) >> 3;
        if (q < g.nchunks) {
            const int tap = q / g.cpt;
            xcol[j] = (unsigned)(q - tap * g.cpt) * 16u;
            xkh[j] = tap / g.KW;
            xkw[j] = tap - xkh[j] * g.KW;
        } else {
            xcol[j] = OOB; xkh[j] = 0; xkw[j] = 0;
        }
    }
    const bool pointwise = g.KH == 1 && g.KW == 1 && g.mul == 1 && g.pad_t == 0 && g.pad_l == 0;   // source pixel = output pixel
    constexpr int NJ = 2;                                        // DMA instructions per wave, operand and stage
    constexpr int XOFF = WT_TILE / 2;                            // the x image of a stage starts here
    auto issue_dma = [&](int mstep, int buf) {
        char* base = smem + buf * (2 * XOFF);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int m = mstep + rowj[j];
            const bool mok = m < m_end;
            const unsigned od = (unsigned)m * (unsigned)g.N * 2u + dycol[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dyres, (lds_void*)(base + (wave + 8 * j) * 1024), 16,
                                                     (mok && dycol[j] != OOB) ? od : OOB, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int m = mstep + rowj[j];
            bool ok = m < m_end && xcol[j] != OOB;
            unsigned pix;
            if (pointwise) {
                pix = (unsigned)m;
            } else {
                const int mm = ok ? m : 0;
                const int b = fdiv(mm, g.d_hw);
                const int rem = mm - b * g.d_hw.d;
                const int oy = fdiv(rem, g.d_w);
                const int ox = rem - oy * g.d_w.d;
                const int iy = oy * g.mul - g.pad_t + xkh[j], ix = ox * g.mul - g.pad_l + xkw[j];
                ok = ok && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
                pix = (unsigned)((b * g.H + iy) * g.W + ix);
            }
            const unsigned ox_ = pix * (unsigned)g.C * 2u + xcol[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(base + XOFF + (wave + 8 * j) * 1024), 16,
                                                     ok ? ox_ : OOB, 0, 0, 0);
        }
    };

    f32x4_t acc[8][4];
    f32x4_t accb[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        accb[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = slab_b != nullptr && bx == 0 && wave_n == 0;
    bf16x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;

    // MFMA k index <-> tile row: sub-step ksub, lane group gq, `half`: row = 32 ksub + 16 (gq>>1) + 8 half + 4 (gq&1) + (li>>2)
    const int gq = lane >> 4, li = lane & 15;
    const int kk0 = (gq >> 1) * 16 + (gq & 1) * 4 + (li >> 2);
    const int key = kk0 & 7;
    int abase[8], bbase[4];
#pragma unroll
    for (int a = 0; a < 8; ++a) abase[a] = kk0 * 512 + ((wave_m * 8 + (a ^ key)) << 5) + (li & 3) * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int gl = wave_n * 4 + c;
        bbase[c] = XOFF + kk0 * 512 + (((gl & 8) | ((gl & 7) ^ key)) << 5) + (li & 3) * 8;
    }
    auto rd = [&](int addr) { return lds_read_tr16_scoped(smem + addr, smem); };

    const int nsteps = (m_end - m_begin + 31) / 32;
#pragma unroll
    for (int p = 0; p < 3; ++p)
        if (p < nsteps) issue_dma(m_begin + p * 32, p);
    auto run = [&](auto bias_tag) {
        constexpr bool BIAS = decltype(bias_tag)::value;
        for (int st = 0; st < nsteps; ++st) {
            // stage st has landed when at most the two younger stages' 2 * NJ instructions each are still in flight
            const int younger = min(2, nsteps - 1 - st);
            if (younger == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();                    // ... for every wave; and stage st - 1's buffer is free (raw barrier:
            asm volatile("" ::: "memory");                   //  __syncthreads() would wait for vmcnt(0) first)
            if (st + 3 < nsteps) issue_dma(m_begin + (st + 3) * 32, (st + 3) & 3);
            const int boff = (st & 3) * (2 * XOFF);
            bf16x8_t fb[4], fa[8];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int half = 0; half < 2; ++half)
                    reinterpret_cast<s16x4_t*>(&fb[c])[half] = rd(bbase[c] + boff + half * 4096);
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int half = 0; half < 2; ++half)
                    reinterpret_cast<s16x4_t*>(&fa[a])[half] = rd(abase[a] + boff + half * 4096);
#pragma unroll
            for (int a = 0; a < 8; ++a) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb[c], acc[a][c], 0, 0, 0);
                if constexpr (BIAS) accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], ones, accb[a], 0, 0, 0);
            }
        }
    };
    if (do_bias) run(std::true_type{}); else run(std::false_type{});

    float* out = slab_w + (long long)split * g.N * ktot;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int col = col0 + wave_n * 64 + c * 16 + (lane & 15);
            if (col >= ktot) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + wave_m * 128 + a * 16 + (lane >> 4) * 4 + j;
                if (co < g.N) out[(long long)co * ktot + col] = acc[a][c][j];
            }
        }
    if (do_bias && (lane & 15) == 0) {
        float* ob = slab_b + (long long)split * g.N;
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + wave_m * 128 + a * 16 + (lane >> 4) * 4 + j;
                if (co < g.N) ob[co] = accb[a][j];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient of a 3x3 / stride 1 / pad 1 convolution with LDS-resident tiles ("patch" form).
// A workgroup owns 64 output channels x 64 input channels (one channel chunk) x all nine taps, and walks a range
// of 16x16 output-pixel blocks.  Per block it brings in the dY tile [256 px][64 co] and the 18x18 halo patch of X
// [324 px][64 ci] ONCE (LDS-DMA, double-buffered) and accumulates
//     dW[co][t][ci] += sum_px dY[px][co] * X[px + shift(t)][ci]          for the nine taps t
// with both operands fetched by transposing LDS reads (the patch at tap-shifted addresses).  The 144 accumulator
// tiles (4 co-tiles x 9 taps x 4 ci-tiles) are dealt to eight waves, 18 each (2 co-tiles x 9 taps x 1 ci-tile), so
// that all four SIMDs carry the same MFMA load (one wave per tap left one SIMD with 3 waves and the others with 2).
// ~128 MACs per byte brought into the CU, versus 32 for the generic 128x128 tile that re-stages X for every tap.
// Block geometry (template): BH output rows x 8*BW8 output columns.  The block's pixels are consumed as "pair groups"
// of 16 (two rows x eight columns); a k-step (32 pixels) takes two of them; an odd count is padded with an all-zero
// dY group.  Three shapes cover the SSD300 maps: 16x16 (300, 150, 75), 6x40 (38) and 10x24 (19).
template <int BH, int BW8>
struct WpGeom {
    static constexpr int BW = BW8 * 8;
    static constexpr int PW = BW + 2, PH = BH + 2;             // halo patch
    static constexpr int PPIX = PW * PH;
    static constexpr int P_INSTR = (PPIX * 8 + 63) / 64;       // one-KiB DMA instructions (8 pixels each)
    static constexpr int P_BYTES = P_INSTR * 1024;
    static constexpr int NPG = (BH / 2) * BW8;                 // pair groups
    static constexpr int KS = (NPG + 1) / 2;                   // k-steps per block
    static constexpr int DY_PIX = KS * 32;
    static constexpr int DY_BYTES = DY_PIX * 128;
    static constexpr int DY_INSTR = DY_PIX / 8;
    static constexpr int BUF = DY_BYTES + P_BYTES;             // one buffer: dY tile + X patch
    static_assert(BH % 2 == 0 && DY_INSTR % 8 == 0, "block shape");
};

// 32-byte column group permutation of a 128-byte pixel row.  A half-wave of a transposing read touches 8 CONSECUTIVE
// pixel rows (any alignment: taps shift them); (p & 1, (p >> 1) & 3) then takes all eight values, i.e. the eight
// 32-byte pieces fall into eight different bank groups.  The key has period 8 in p, which is what lets the reader
// keep eight per-lane base addresses and reach every (k-step, tap, half) with an immediate offset.
__device__ __forceinline__ int wp_key(int px) { return (px >> 1) & 3; }

template <int BH, int BW8>
__global__ __launch_bounds__(512) void k_conv3x3_wgrad_patch(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ dy,
                                                             float* __restrict__ slab_w, float* __restrict__ slab_b,
                                                             ConvGeom g, int tiles_x, int tiles_y, int tiles_per_split,
                                                             int nsplit, int cout, int single_buf, int xg) {
    // g: source = x (B,H,W,C), destination = dy (Ho=H, Wo=W, N = ldy)
    using G = WpGeom<BH, BW8>;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    // eight waves, two per SIMD (waves w and w + 4 share one), with UNEQUAL roles: the "loader" waves 0-3 issue all of
    // the next block's LDS-DMA (an LDS-DMA instruction holds its wave for 100-200 cycles, ~2700 cycles per block) and own
    // LTAPS = 4 taps x four co-tiles = 16 accumulator tiles of input-channel tile ct = w; their partners 4-7 issue no
    // DMA and own the other five taps = 20 tiles.  While a loader is stuck in its DMA issue the partner keeps the SIMD's MFMA
    // pipe busy; with equal shares and everybody issuing DMA both waves of a SIMD stalled together (measured: 459 us
    // with, 340 us without the DMA, same clock, the difference all in barrier waits).
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = wave & 3, role = wave >> 2;              // role 0: loader, first taps; role 1: the rest
    // work units (split, co tile, ci chunk), chunk fastest.  XCD-aware order (workgroup L runs on XCD L % 8): `xg`
    // consecutive units -- the channel groups that walk the SAME pixel blocks -- sit on one XCD, so that a dY tile /
    // X patch is fetched into that L2 once instead of once per group (xg from the host: a divisor of the unit count
    // per split, or a multiple of it, that still leaves every XCD with work)
    const int nchunk = g.C >> 6, cotiles = (cout + 63) >> 6;
    const int nunits = nchunk * cotiles * nsplit;
    const int j = blockIdx.x >> 3;
    int id = ((j / xg) * 8 + (blockIdx.x & 7)) * xg + j % xg;
    if (id >= nunits) return;
    const int chunk = id % nchunk; id /= nchunk;
    const int cot = id % cotiles;
    const int split = id / cotiles;
    const int co0 = cot * 64, ci0 = chunk * 64;
    const int ntiles = g.B * tiles_x * tiles_y;
    const int t_begin = split * tiles_per_split, t_end = min(ntiles, t_begin + tiles_per_split);

    // (buffer-descriptor DMA: 32-bit byte offsets, a lane outside the map / the tile gets an out-of-range offset and the
    //  hardware writes zeros -- no 64-bit address arithmetic and no zero block)
    const __amdgpu_buffer_rsrc_t xres = __builtin_amdgcn_make_buffer_rsrc((void*)x, 0, (unsigned)g.B * g.H * g.W * g.C * 2u, 0x00020000);
    const __amdgpu_buffer_rsrc_t dyres = __builtin_amdgcn_make_buffer_rsrc((void*)dy, 0, (unsigned)g.B * g.Ho * g.Wo * g.N * 2u, 0x00020000);
    constexpr unsigned WP_OOB = 0xfffffff0u;
    // DMA ownership: instruction i of the dY tile / of the patch goes to loader wave i % 4
    auto issue_dma = [&](int t, int buf) {
        int r = t;
        const int tx = r % tiles_x; r /= tiles_x;
        const int ty = r % tiles_y;
        const int b = r / tiles_y;
        const int y0 = ty * BH, x0 = tx * G::BW;
        char* base = smem + buf * G::BUF;
#pragma unroll
        for (int j = 0; j < G::DY_INSTR / 4; ++j) {
            const int i = ct + 4 * j;                       // 8 pixel slots x 128 B per instruction
            const int kk = 8 * i + (lane >> 3), sl = lane & 7;
            const int c16 = (((sl >> 1) ^ wp_key(kk)) << 1) | (sl & 1);
            const int pg = kk >> 4;                         // pair group -> (row pair, column group)
            const int rp = pg / BW8, xg = pg - rp * BW8;
            const int y = y0 + 2 * rp + ((kk >> 3) & 1), xx = x0 + xg * 8 + (kk & 7);
            const int co = co0 + c16 * 8;
            const bool ok = pg < G::NPG && y < g.Ho && xx < g.Wo && co < g.N;
            const unsigned off = ((unsigned)((b * g.Ho + y) * g.Wo + xx) * (unsigned)g.N + (unsigned)co) * 2u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(dyres, (lds_void*)(base + i * 1024), 16, ok ? off : WP_OOB, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < (G::P_INSTR + 3) / 4; ++j) {
            const int i = ct + 4 * j;
            if (i < G::P_INSTR) {
                const int pp = 8 * i + (lane >> 3), sl = lane & 7;
                const int c16 = (((sl >> 1) ^ wp_key(pp)) << 1) | (sl & 1);
                const int py = pp / G::PW, px = pp - py * G::PW;
                const int iy = y0 - 1 + py, ix = x0 - 1 + px;
                const bool ok = pp < G::PPIX && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
                const unsigned off = ((unsigned)((b * g.H + iy) * g.W + ix) * (unsigned)g.C + (unsigned)(ci0 + c16 * 8)) * 2u;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(xres, (lds_void*)(base + G::DY_BYTES + i * 1024), 16, ok ? off : WP_OOB, 0, 0, 0);
            }
        }
    };

    constexpr int LTAPS = 4;                                // taps of a loader wave; its partner takes the other 9 - LTAPS (3 | 6 measured the same)
    f32x4_t acc[4][9 - LTAPS];                              // [co tile][tap of this role]
    f32x4_t accb[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        accb[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t5 = 0; t5 < 9 - LTAPS; ++t5) acc[a][t5] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const bool do_bias = slab_b != nullptr && chunk == 0 && ct == 0 && role == 1;
    bf16x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;

    // two LDS buffers: the next block's DMA is in flight during this block's MFMAs
    if (t_begin < t_end && role == 0) issue_dma(t_begin, 0);
    // MFMA k index <-> block pixel: k-step ks, `half` select pair group pg = 2ks + half = (row pair rp, column group xg);
    // within it lane group gq and the lane select row 2rp + (gq>>1), column 8xg + 4*(gq&1) + (li>>2), so that the 8 rows
    // of a half-wave instruction are consecutive pixels.  All address arithmetic is hoisted: the dY row of a lane is
    // base + immediate, and a patch row is one of eight per-lane bases (pixel offset mod 8) + immediate.
    const int gq = lane >> 4, li = lane & 15;
    int abase[4];
    {
        const int kk0 = (gq >> 1) * 8 + (gq & 1) * 4 + (li >> 2);
#pragma unroll
        for (int a = 0; a < 4; ++a) abase[a] = kk0 * 128 + ((a ^ wp_key(kk0)) << 5) + (li & 3) * 8;
    }
    int gbase[8];
    {
        const int p0 = (gq >> 1) * G::PW + (gq & 1) * 4 + (li >> 2);
#pragma unroll
        for (int r = 0; r < 8; ++r) gbase[r] = G::DY_BYTES + (p0 + r) * 128 + ((ct ^ wp_key(p0 + r)) << 5) + (li & 3) * 8;
    }
    typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;
    // fragments of one k-step: 8 dY reads + 2 patch reads per tap (all with immediate offsets)
    struct Frag { bf16x8_t fa[4]; bf16x8_t fb[9 - LTAPS]; };
    // the block loop exists per role (and with / without the bias MFMAs) so that its body has no branch: the k-steps of
    // a block are one basic block, software-pipelined by hand (fragments of k-step ks+1 are read during the MFMAs of ks)
    auto run = [&](auto role_tag, auto bias_tag) {
        constexpr int ROLE = decltype(role_tag)::value;
        constexpr bool BIAS = decltype(bias_tag)::value;
        constexpr int TAP0 = ROLE == 0 ? 0 : LTAPS, NTAP = ROLE == 0 ? LTAPS : 9 - LTAPS;
        auto load_frag = [&](Frag& f, const int (&ab)[4], const int (&gb)[8], auto ks_tag) {
            constexpr int ks = decltype(ks_tag)::value;
#pragma unroll
            for (int half = 0; half < 2; ++half)
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    reinterpret_cast<s16x4_t*>(&f.fa[a])[half] =
                        lds_read_tr16_scoped(smem + ab[a] + (ks * 2 + half) * 2048, smem);
#pragma unroll
            for (int t5 = 0; t5 < NTAP; ++t5)
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int tap = TAP0 + t5;
                    const int pg = (ks * 2 + half) < G::NPG ? (ks * 2 + half) : 0;   // padding group: any finite data (dY is zero there)
                    const int rp = pg / BW8, xg = pg - rp * BW8;
                    const int ctap = (2 * rp + tap / 3) * G::PW + xg * 8 + (tap % 3);   // compile-time pixel offset
                    reinterpret_cast<s16x4_t*>(&f.fb[t5])[half] =
                        lds_read_tr16_scoped(smem + gb[ctap & 7] + (ctap >> 3) * 1024, smem);
                }
        };
        for (int t = t_begin; t < t_end; ++t) {
            const int cur = (t - t_begin) & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if constexpr (ROLE == 0) { if (t + 1 < t_end) issue_dma(t + 1, cur ^ 1); }
            const int boff = cur * G::BUF;
            int ab[4], gb[8];
#pragma unroll
            for (int a = 0; a < 4; ++a) ab[a] = abase[a] + boff;
#pragma unroll
            for (int r = 0; r < 8; ++r) gb[r] = gbase[r] + boff;
            Frag f0, f1;
            auto mma = [&](const Frag& f) {
#pragma unroll
                for (int t5 = 0; t5 < NTAP; ++t5)
#pragma unroll
                    for (int a = 0; a < 4; ++a)
                        acc[a][t5] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.fa[a], f.fb[t5], acc[a][t5], 0, 0, 0);
                if constexpr (BIAS) {
#pragma unroll
                    for (int a = 0; a < 4; ++a) accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.fa[a], ones, accb[a], 0, 0, 0);
                }
            };
            // interleave: one MFMA, then one LDS read of the next k-step
            auto weave = [&]() {
                constexpr int NR = 8 + 2 * NTAP, NM = 4 * NTAP;          // reads of the next k-step, MFMAs of this one
                constexpr int PAIRS = NR < NM ? NR : NM;
                if constexpr (NR > PAIRS) {                             // more reads than MFMAs: the surplus goes first
                    __builtin_amdgcn_sched_group_barrier(0x100, NR - PAIRS, 0);
                }
#pragma unroll
                for (int i = 0; i < PAIRS; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                constexpr int REST = NM - PAIRS + (BIAS ? 4 : 0);
                if constexpr (REST > 0) __builtin_amdgcn_sched_group_barrier(0x008, REST, 0);
            };
            static_assert(G::KS == 8, "the hand-unrolled pipeline below assumes eight k-steps per block");
            load_frag(f0, ab, gb, std::integral_constant<int, 0>{});
            // the woven fragment-read / MFMA stream of a block runs at LOW priority, the top of the block (wait, barrier, the
            // loaders' DMA issue, address set-up, first fragments) at high: the two waves of a SIMD are in different phases for
            // most of a block (loader / partner), and the one in its MFMAs no longer holds the other one up: +3-5 % per layer
            __builtin_amdgcn_s_setprio(0);
            load_frag(f1, ab, gb, std::integral_constant<int, 1>{}); mma(f0); weave();
            load_frag(f0, ab, gb, std::integral_constant<int, 2>{}); mma(f1); weave();
            load_frag(f1, ab, gb, std::integral_constant<int, 3>{}); mma(f0); weave();
            load_frag(f0, ab, gb, std::integral_constant<int, 4>{}); mma(f1); weave();
            load_frag(f1, ab, gb, std::integral_constant<int, 5>{}); mma(f0); weave();
            load_frag(f0, ab, gb, std::integral_constant<int, 6>{}); mma(f1); weave();
            load_frag(f1, ab, gb, std::integral_constant<int, 7>{}); mma(f0); weave();
            mma(f1);
            __builtin_amdgcn_s_setprio(3);
        }
    };
    if (role == 0) run(std::integral_constant<int, 0>{}, std::false_type{});
    else if (do_bias) run(std::integral_constant<int, 1>{}, std::true_type{});
    else run(std::integral_constant<int, 1>{}, std::false_type{});
    // slab[split][co][tap][ci]  (dW layout [Cout][kh][kw][Cin], rows = ldy channels)
    const int ktot = g.ldw;
    float* out = slab_w + (long long)split * g.N * ktot;
    const int tap0 = role == 0 ? 0 : LTAPS, ntap = role == 0 ? LTAPS : 9 - LTAPS;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int t5 = 0; t5 < 9 - LTAPS; ++t5) {
            if (t5 >= ntap) continue;
            const int col = (tap0 + t5) * g.C + ci0 + ct * 16 + (lane & 15);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + a * 16 + (lane >> 4) * 4 + j;
                if (co < g.N) out[(long long)co * ktot + col] = acc[a][t5][j];
            }
        }
    if (do_bias && (lane & 15) == 0) {
        float* ob = slab_b + (long long)split * g.N;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = co0 + a * 16 + (lane >> 4) * 4 + j;
                if (co < g.N) ob[co] = accb[a][j];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient of the first layer (3x3 / stride 1 / pad 1, 8 input channels = 3 image channels + padding, <= 64
// output channels): dW[co][tap][ch] = sum_px dY[px][co] * X[px + shift(tap)][ch], 72 columns.  The work is reading dY
// once (HBM-bound); a workgroup walks 16x16-pixel blocks (dY tile 32 KB + an 18x18 x 16-byte halo patch, LDS-DMA,
// double-buffered), wave w multiplies k-step w (32 pixels) of every block: 4 channel tiles x 5 column tiles (a column
// tile = two taps x 8 channels) = 20 MFMAs; the eight partial sums are added in wave order at the end.
constexpr int W0_DY = 256 * 128;                           // dY tile bytes
constexpr int W0_PATCH = 6 * 1024;                         // 324 px x 16 B = 5184 B -> 6 DMA instructions
constexpr int W0_BUF = W0_DY + W0_PATCH;

__global__ __launch_bounds__(512) void k_conv0_wgrad(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ dy,
                                                     float* __restrict__ slab_w, float* __restrict__ slab_b, ConvGeom g,
                                                     int tiles_x, int tiles_y, int tiles_per_split, int cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x;
    const int ntiles = g.B * tiles_x * tiles_y;
    const int t_begin = split * tiles_per_split, t_end = min(ntiles, t_begin + tiles_per_split);

    auto issue_dma = [&](int t, int buf) {
        int r = t;
        const int tx = r % tiles_x; r /= tiles_x;
        const int ty = r % tiles_y;
        const int b = r / tiles_y;
        const int y0 = ty * 16, x0 = tx * 16;
        char* base = smem + buf * W0_BUF;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                       // dY: slot layout of k_conv3x3_wgrad_patch<16, 2>
            const int i = wave + 8 * j;
            const int kk = 8 * i + (lane >> 3), sl = lane & 7;
            const int c16 = (((sl >> 1) ^ wp_key(kk)) << 1) | (sl & 1);
            const int pg = kk >> 4;
            const int y = y0 + 2 * (pg >> 1) + ((kk >> 3) & 1), xx = x0 + (pg & 1) * 8 + (kk & 7);
            const int co = c16 * 8;
            const bool ok = y < g.Ho && xx < g.Wo && co < g.N;
            const bf16_raw* src = ok ? dy + ((unsigned)((b * g.Ho + y) * g.Wo + xx) * (unsigned)g.N + (unsigned)co)
                                     : reinterpret_cast<const bf16_raw*>(g_zero16);
            __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(base + i * 1024), 16, 0, 0);
        }
        if (wave < 6) {                                     // patch: one 16-byte pixel per lane, row-major 18x18
            const int pp = wave * 64 + lane;
            const int py = pp / PATCH_W, px = pp - py * PATCH_W;
            const int iy = y0 - 1 + py, ix = x0 - 1 + px;
            const bool ok = pp < PATCH_PIX && (unsigned)iy < (unsigned)g.H && (unsigned)ix < (unsigned)g.W;
            const bf16_raw* src = ok ? x + (unsigned)((b * g.H + iy) * g.W + ix) * 8u : reinterpret_cast<const bf16_raw*>(g_zero16);
            __builtin_amdgcn_global_load_lds((gbl_void*)src, (lds_void*)(base + W0_DY + wave * 1024), 16, 0, 0);
        }
    };

    f32x4_t acc[4][5];
    f32x4_t accb[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        accb[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 5; ++c) acc[a][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    bf16x8_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (__bf16)1.0f;

    // this wave's k-step: block rows 2w, 2w+1.  MFMA k index <-> pixel as in k_conv3x3_wgrad_patch
    const int gq = lane >> 4, li = lane & 15;
    const int kk0 = (gq >> 1) * 8 + (gq & 1) * 4 + (li >> 2);
    int abase[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) abase[a] = wave * 4096 + kk0 * 128 + ((a ^ wp_key(kk0)) << 5) + (li & 3) * 8;
    // patch pixel of tap (0,0) for half 0: row 2w + (gq>>1), column 4 (gq&1) + (li>>2); column tile t: lanes with
    // (li & 2) == 0 read tap 2t, the others tap 2t+1 (tap 9 does not exist: its columns are never stored)
    const int p0 = (2 * wave + (gq >> 1)) * PATCH_W + (gq & 1) * 4 + (li >> 2);
    int bbase[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        int tap = 2 * t + ((li >> 1) & 1);
        if (tap > 8) tap = 8;
        bbase[t] = W0_DY + (p0 + (tap / 3) * PATCH_W + tap % 3) * 16 + (li & 1) * 8;
    }
    typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;
    auto rd = [&](int addr) { return lds_read_tr16_scoped(smem + addr, smem); };

    if (t_begin < t_end) issue_dma(t_begin, 0);
    for (int t = t_begin; t < t_end; ++t) {
        const int cur = (t - t_begin) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < t_end) issue_dma(t + 1, cur ^ 1);
        const int boff = cur * W0_BUF;
        bf16x8_t fa[4], fb[5];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int a = 0; a < 4; ++a) reinterpret_cast<s16x4_t*>(&fa[a])[half] = rd(boff + abase[a] + half * 2048);
#pragma unroll
            for (int c = 0; c < 5; ++c) reinterpret_cast<s16x4_t*>(&fb[c])[half] = rd(boff + bbase[c] + half * 8 * 16);
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int c = 0; c < 5; ++c) acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb[c], acc[a][c], 0, 0, 0);
            accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], ones, accb[a], 0, 0, 0);
        }
    }
    // sum the eight waves' partial tiles in wave order (fixed order: reproducible), through LDS
    __syncthreads();
    float* red = reinterpret_cast<float*>(smem);            // [24 tiles][64 lanes][4]
    for (int w = 0; w < 8; ++w) {
        if (wave == w) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    f32x4_t v;
                    if (c < 5) v = acc[a][c < 5 ? c : 0]; else v = accb[a];
                    f32x4_t* slot = reinterpret_cast<f32x4_t*>(red + ((a * 6 + c) * 64 + lane) * 4);
                    if (w > 0) { const f32x4_t o = *slot; v[0] += o[0]; v[1] += o[1]; v[2] += o[2]; v[3] += o[3]; }
                    *slot = v;
                }
            }
        }
        __syncthreads();
    }
    // slab[split][co][72]; tile (a, c): D row = co a*16 + (lane>>4)*4 + j, column c*16 + (lane&15)
    const int ktot = g.ldw;                                 // 72
    for (int idx = tid; idx < 24 * 64; idx += 512) {
        const int tile = idx >> 6, l = idx & 63;
        const int a = tile / 6, c = tile - a * 6;
        const f32x4_t v = *reinterpret_cast<const f32x4_t*>(red + idx * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = a * 16 + (l >> 4) * 4 + j;
            if (co >= g.N) continue;
            if (c < 5) {
                const int col = c * 16 + (l & 15);
                if (col < ktot) slab_w[((long long)split * g.N + co) * ktot + col] = v[j];
            } else if (slab_b != nullptr && (l & 15) == 0) {
                slab_b[(long long)split * g.N + co] = v[j];
            }
        }
    }
}

// weights and bias in one launch: blocks [0, nbw) reduce the first nw elements of the weight slab (stride sw per split)
// four at a time, the remaining blocks the nb bias elements (stride sb)
__global__ __launch_bounds__(256) void k_wgrad_reduce2(const float* __restrict__ slab_w, long long sw, long long nw,
                                                       float* __restrict__ dw, const float* __restrict__ slab_b, long long sb,
                                                       int nb, float* __restrict__ db, int nsplit, unsigned nbw) {
    if (blockIdx.x < nbw) {
        const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
        if (i >= nw) return;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int z = 0; z < nsplit; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(slab_w + (long long)z * sw + i);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4*>(dw + i) = s;
    } else {
        const int i = (int)(blockIdx.x - nbw) * 256 + threadIdx.x;
        if (i >= nb) return;
        float s = 0.f;
        for (int z = 0; z < nsplit; ++z) s += slab_b[(long long)z * sb + i];
        db[i] = s;
    }
}

// many splits, few outputs (first layer: 512 splits of 4.6 K values): 16 threads per float4 of the output, thread g adds
// splits g, g+16, ... in order, then the 16 partial sums are added in order: fixed summation order, 16x the parallelism
__global__ __launch_bounds__(256) void k_wgrad_reduce_wide(const float* __restrict__ slab_w, long long sw, long long nw,
                                                          float* __restrict__ dw, const float* __restrict__ slab_b, long long sb,
                                                          int nb, float* __restrict__ db, int nsplit, unsigned nbw) {
    __shared__ float4 part[256];
    const int o = threadIdx.x & 15, grp = threadIdx.x >> 4;
    float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x < nbw) {
        const long long i = ((long long)blockIdx.x * 16 + o) * 4;
        if (i < nw)
            for (int z = grp; z < nsplit; z += 16) {
                const float4 v = *reinterpret_cast<const float4*>(slab_w + (long long)z * sw + i);
                s4.x += v.x; s4.y += v.y; s4.z += v.z; s4.w += v.w;
            }
        part[threadIdx.x] = s4;
        __syncthreads();
        if (grp == 0 && i < nw) {
            float4 t = part[o];
            for (int k = 1; k < 16; ++k) { const float4 v = part[k * 16 + o]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
            *reinterpret_cast<float4*>(dw + i) = t;
        }
    } else {
        const int i = (int)(blockIdx.x - nbw) * 16 + o;
        float sacc = 0.f;
        if (i < nb)
            for (int z = grp; z < nsplit; z += 16) sacc += slab_b[(long long)z * sb + i];
        part[threadIdx.x].x = sacc;
        __syncthreads();
        if (grp == 0 && i < nb) {
            float t = part[o].x;
            for (int k = 1; k < 16; ++k) t += part[k * 16 + o].x;
            db[i] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Host side.  How a layer is split is decided ONCE, by wgrad_plan from the geometry alone; the single call, the batched call,
// the plan query and the workspace bound all read that decision or the helpers it is made of.

// ---- one predicate per kernel family.  Each is split into its channel condition -- all that the workspace bound can see --
// and the rest (knob, map side, tensor size), which only the plan knows ----
bool wgrad_same3x3(const ssd_wgrad_item& it) {            // 3x3 / stride 1 / pad 1: the output map is the input map
    return it.ksize == 3 && it.stride == 1 && it.pad_t == 1 && it.pad_l == 1 && it.H == it.Ho && it.W == it.Wo;
}

// first layer (8 padded image channels): dedicated kernel, 512 pixel-block splits at most
bool wgrad_first_channels(int Cin, int Cout, int ldy, int ksize) { return Cin == 8 && Cout <= 64 && ldy <= 64 && ksize == 3; }
bool wgrad_first_layer(const ssd_wgrad_item& it) {
    return ssd_knob("SSD_WGRAD_FIRST", 1) && wgrad_first_channels(it.Cin, it.Cout, it.ldy, it.ksize) && wgrad_same3x3(it) &&
           it.H >= 16 && it.W >= 16;
}

// patch kernel.  SSD_WGRAD_PATCH = smallest feature-map side it serves (0: off)
bool wgrad_use_patch(const ssd_wgrad_item& it) {
    const int mn = ssd_knob("SSD_WGRAD_PATCH", 16);
    return mn > 0 && wgrad_same3x3(it) && it.Cin % 64 == 0 && it.H >= mn && it.W >= mn;
}

// 256x256 GEMM weight-gradient kernel: used for wide layers the patch kernel does not serve
bool wgrad_tile_channels(int Cout, long long ktot) { return Cout > 128 && ktot >= 256; }
bool wgrad_use_tile(long long M, int Cout, int ldy, long long ktot, long long x_elems) {
    return ssd_knob("SSD_WGRAD_TILE", 1) && wgrad_tile_channels(Cout, ktot) && M >= 2048 && M * ldy < (1ll << 31) - 16 &&
           x_elems < (1ll << 31) - 16;
}

// ---- split rules ----
// block shape of the patch kernel for a map: the candidate with the least padded work (0: 16x16, 1: 6x40, 2: 10x24)
int wgrad_patch_shape(int Ho, int Wo, int* bh, int* bw) {
    static const int shapes[3][3] = {{16, 16, 16}, {6, 40, 15}, {10, 24, 15}};   // rows, columns, pair groups (of 16 slots)
    int best = 0;
    double best_cost = 0;
    for (int i = 0; i < 3; ++i) {
        // every block costs eight k-steps whatever its shape: fewest blocks wins
        const double cost = (double)((Ho + shapes[i][0] - 1) / shapes[i][0]) * ((Wo + shapes[i][1] - 1) / shapes[i][1]);
        if (i == 0 || cost < best_cost) { best = i; best_cost = cost; }
    }
    const int forced = ssd_knob("SSD_WGRAD_PATCH_SHAPE", -1);
    if (forced >= 0 && forced < 3) best = forced;
    *bh = shapes[best][0]; *bw = shapes[best][1];
    return best;
}

int wgrad_patch_plan(int B, int Ho, int Wo, int Cin, int Cout, int* tiles_x, int* tiles_y, int* tps, int* ns) {   // returns the shape
    int bh, bw;
    const int shape = wgrad_patch_shape(Ho, Wo, &bh, &bw);
    *tiles_x = (Wo + bw - 1) / bw; *tiles_y = (Ho + bh - 1) / bh;
    const int ntiles = B * *tiles_x * *tiles_y;
    const int groups = (Cin / 64) * ((Cout + 63) / 64);
    int want = 256 / groups;                                 // one workgroup per CU
    if (want < 1) want = 1;
    if (want > ntiles) want = ntiles;
    *tps = (ntiles + want - 1) / want;
    *ns = (ntiles + *tps - 1) / *tps;
    return shape;
}

constexpr int WG_BMO = 128, WG_BNC = 128;                    // k_conv_wgrad's tile: output channels x (tap, ci) columns

int wgrad_splits(long long M, int tiles) {
    long long want = 768 / tiles;                            // whole rounds: <= 3 workgroups per CU in total
    long long maxs = (M + 511) / 512;                        // at least 512 pixels per split
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    if (want > 512) want = 512;
    return (int)want;
}

// pixel splits for the 256x256 kernel (one workgroup per CU): estimated time = rounds x steps per split + slab traffic
int wgrad_tile_splits(long long M, int tiles, long long slab_elems) {
    int best = 1;
    double best_cost = 0;
    const long long maxs = M / 256 > 0 ? M / 256 : 1;
    for (int ns = 1; ns <= 64 && ns <= maxs; ++ns) {
        const long long rounds = ((long long)tiles * ns + 255) / 256;
        const long long steps = ((M + ns - 1) / ns + 63) / 64;
        const double cost = (double)rounds * steps * 2.2 + (double)ns * slab_elems * 8.0 / 4.0e6;   // microseconds
        if (ns == 1 || cost < best_cost) { best = ns; best_cost = cost; }
    }
    return best;
}

// ---- slab layout, every kernel: ns weight slabs [ldy][ktot] fp32, then ns bias slabs [ldy] ----
size_t slab_bytes(int ns, int ldy, long long ktot) { return (size_t)ns * ((size_t)ldy * ktot + ldy) * sizeof(float); }
float* slab_bias(float* slab_w, int ns, int ldy, long long ktot) { return slab_w + (size_t)ns * ldy * ktot; }

// ---- the plan ----
struct WgradPlan {
    int id;                                  // SSD_PLAN_WG_* (the patch shape included); SSD_PLAN_F_REDUCE_WIDE follows from ns
    int ns;                                  // slabs written == splits the reduction sums
    int per_split;                           // blocks per split (first layer, patch) or pixels per split, rounded up to 64 (tile, generic)
    int tx, ty;                              // pixel-block grid (first layer, patch)
    int ctiles, mtiles;                      // column / output-channel tiles (tile, generic)
    int xg;                                  // patch: units per XCD group
    unsigned grid;                           // workgroups of the slab kernel
    long long ktot;                          // (tap, ci) columns of dW
    int word() const { return id | (ns >= 32 ? SSD_PLAN_F_REDUCE_WIDE : 0); }   // what ssd_conv2d_bwd_weight_plan answers
};

// SSD_OK / SSD_ERR_VALUE; reads no pointer of `it`
int wgrad_plan(const ssd_wgrad_item& it, WgradPlan* p) {
    if (!geom_ok(it.B, it.H, it.W, it.Cin, it.Ho, it.Wo, it.Cout, it.ksize) || it.stride <= 0 || it.ldy < it.Cout || it.ldy % 8)
        return SSD_ERR_VALUE;
    *p = WgradPlan{};
    const long long M = (long long)it.B * it.Ho * it.Wo, x_elems = (long long)it.B * it.H * it.W * it.Cin;
    const long long ktot = p->ktot = (long long)it.ksize * it.ksize * it.Cin;
    if (wgrad_first_layer(it)) {
        p->id = SSD_PLAN_WG_FIRST;
        p->tx = (it.Wo + 15) / 16; p->ty = (it.Ho + 15) / 16;
        const int ntiles = it.B * p->tx * p->ty, want = ntiles < 512 ? ntiles : 512;
        p->per_split = (ntiles + want - 1) / want;
        p->ns = (ntiles + p->per_split - 1) / p->per_split;
        p->grid = (unsigned)p->ns;
    } else if (wgrad_use_patch(it) && x_elems * 2 < (1ll << 32) - 16 && M * it.ldy * 2 < (1ll << 32) - 16) {   // 32-bit DMA offsets
        const int shape = wgrad_patch_plan(it.B, it.Ho, it.Wo, it.Cin, it.Cout, &p->tx, &p->ty, &p->per_split, &p->ns);
        p->id = shape == 1 ? SSD_PLAN_WG_PATCH_6x40 : (shape == 2 ? SSD_PLAN_WG_PATCH_10x24 : SSD_PLAN_WG_PATCH_16x16);
        const int groups = (it.Cin / 64) * ((it.Cout + 63) / 64), nunits = groups * p->ns;
        // units per XCD group: the largest divisor of the channel-group count whose round-robin placement (group i on
        // XCD i % 8) keeps every XCD within ~7 % of its fair share of workgroups
        p->xg = 1;
        for (int d = groups; d >= 1; --d) {
            if (groups % d) continue;
            const int ngr = (nunits + d - 1) / d;
            const int load = ((ngr + 7) / 8) * d, fair = (nunits + 7) / 8;
            if (load * 100 <= fair * 107) { p->xg = d; break; }
        }
        if (!ssd_knob("SSD_WGRAD_PATCH_XCD", 1)) p->xg = 1;
        p->grid = (unsigned)(8 * p->xg * ((nunits + 8 * p->xg - 1) / (8 * p->xg)));
    } else {                                                 // a GEMM over pixels: the 256x256 tile or the generic 128x128 one
        const bool tile = wgrad_use_tile(M, it.Cout, it.ldy, ktot, x_elems);
        const int bmo = tile ? 256 : WG_BMO, bnc = tile ? 256 : WG_BNC;
        p->id = tile ? SSD_PLAN_WG_TILE : SSD_PLAN_WG_GENERIC;
        p->ctiles = (int)((ktot + bnc - 1) / bnc); p->mtiles = (it.Cout + bmo - 1) / bmo;
        p->ns = tile ? wgrad_tile_splits(M, p->ctiles * p->mtiles, (long long)it.ldy * ktot) : wgrad_splits(M, p->ctiles * p->mtiles);
        p->per_split = ((int)((M + p->ns - 1) / p->ns) + 63) / 64 * 64;
        p->grid = (unsigned)(p->ctiles * p->mtiles * p->ns);
    }
    return SSD_OK;
}

ConvGeom wgrad_geom(const ssd_wgrad_item& it) {             // source = x dims, destination = dy dims with N = ldy
    return make_geom(it.B, it.H, it.W, it.Cin, it.Ho, it.Wo, it.ldy, it.ksize, it.ksize, it.stride, 1, it.pad_t, it.pad_l);
}

}  // namespace

// dW / dbias = sum over splits of the slabs, fixed order
void ssd_launch_wgrad_reduce(hipStream_t s, const float* slab_w, long long sw, long long nw, float* dw, const float* slab_b,
                             long long sb, int nb, float* db, int ns) {
    if (ns >= 32) {
        const unsigned nbw = (unsigned)((nw / 4 + 15) / 16), nbb = db ? (unsigned)((nb + 15) / 16) : 0u;
        hipLaunchKernelGGL(k_wgrad_reduce_wide, dim3(nbw + nbb), dim3(256), 0, s, slab_w, sw, nw, dw, slab_b, sb, nb, db, ns, nbw);
    } else {
        const unsigned nbw = (unsigned)((nw / 4 + 255) / 256), nbb = db ? (unsigned)((nb + 255) / 256) : 0u;
        hipLaunchKernelGGL(k_wgrad_reduce2, dim3(nbw + nbb), dim3(256), 0, s, slab_w, sw, nw, dw, slab_b, sb, nb, db, ns, nbw);
    }
}

extern "C" {

static size_t wgrad_ws_bytes(const ssd_wgrad_item& it) {
    return ssd_conv2d_bwd_weight_workspace_bytes(it.B, it.Ho, it.Wo, it.Cin, it.Cout, it.ldy, it.ksize);
}

// An upper bound over the candidate kernels: the call has no stride, padding or input size, so each family is asked with
// its channel condition only -- deliberately the WIDER condition than wgrad_plan's (no knob, no map side, no tensor-size
// limit; the patch kernel as if the layer were 3x3 / stride 1 / pad 1 on this map).  Engine allocations follow from this number.
size_t ssd_conv2d_bwd_weight_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int ldy, int ksize) {
    if (B <= 0 || Ho <= 0 || Wo <= 0 || Cin <= 0 || Cout <= 0 || ldy < Cout || ksize <= 0) return 0;
    const long long ktot = (long long)ksize * ksize * Cin, M = (long long)B * Ho * Wo;
    const int tiles = (int)(((ktot + WG_BNC - 1) / WG_BNC) * ((Cout + WG_BMO - 1) / WG_BMO));
    int ns = wgrad_splits(M, tiles);                         // the generic kernel serves any layer
    if (wgrad_first_channels(Cin, Cout, ldy, ksize) && ns < 512) ns = 512;
    if (wgrad_tile_channels(Cout, ktot)) {
        const int ns2 = wgrad_tile_splits(M, (int)(((ktot + 255) / 256) * ((Cout + 255) / 256)), (long long)ldy * ktot);
        if (ns2 > ns) ns = ns2;
    }
    ssd_wgrad_item same = {};
    same.B = B; same.H = same.Ho = Ho; same.W = same.Wo = Wo; same.Cin = Cin; same.ksize = ksize;
    same.stride = same.pad_t = same.pad_l = 1;
    if (wgrad_use_patch(same)) {
        int tx, ty, tps, nsp;
        wgrad_patch_plan(B, Ho, Wo, Cin, Cout, &tx, &ty, &tps, &nsp);
        if (nsp > ns) ns = nsp;
    }
    return slab_bytes(ns, ldy, ktot);
}

static int conv2d_bwd_weight_impl(const ssd_wgrad_item& it, void* ws, size_t ws_bytes, void* stream) {
    // x: [B,H,W,Cin]; dy: [B,Ho,Wo,ldy] (first Cout channels used); dw: f32 [Cout][k][k][Cin]; dbias: f32 [Cout] or null
    WgradPlan p;
    if (!it.x || !it.dy || !it.dw || wgrad_plan(it, &p) != SSD_OK) return SSD_ERR_VALUE;
    if (!ws || ws_bytes < wgrad_ws_bytes(it)) return SSD_ERR_WORKSPACE;
    const ConvGeom g = wgrad_geom(it);
    const bf16_raw* x = static_cast<const bf16_raw*>(it.x);
    const bf16_raw* dy = static_cast<const bf16_raw*>(it.dy);
    float* slab_w = static_cast<float*>(ws);
    float* slab_b = slab_bias(slab_w, p.ns, it.ldy, p.ktot);
    float* sb = it.dbias ? slab_b : nullptr;
    hipStream_t s = (hipStream_t)stream;
#define SSD_LAUNCH_WP(BH_, BW8_)                                                                                    \
    do {                                                                                                            \
        using G_ = WpGeom<BH_, BW8_>;                                                                               \
        auto kern_ = k_conv3x3_wgrad_patch<BH_, BW8_>;                                                              \
        static OnceLds set_; if (ensure_lds(set_, reinterpret_cast<const void*>(kern_), (int)(2 * G_::BUF)) != 0) return SSD_ERR_LAUNCH; \
        hipLaunchKernelGGL(kern_, dim3(p.grid), dim3(512), (size_t)2 * G_::BUF, s, x, dy, slab_w, sb, g, p.tx, p.ty, p.per_split, \
                           p.ns, it.Cout, 0, p.xg);                                                                 \
    } while (0)
    switch (p.id) {
        case SSD_PLAN_WG_FIRST: {
            static OnceLds set; if (ensure_lds(set, reinterpret_cast<const void*>(k_conv0_wgrad), (int)(2 * W0_BUF)) != 0) return SSD_ERR_LAUNCH;
            hipLaunchKernelGGL(k_conv0_wgrad, dim3(p.grid), dim3(512), 2 * W0_BUF, s, x, dy, slab_w, sb, g, p.tx, p.ty, p.per_split, it.Cout);
            break;
        }
        case SSD_PLAN_WG_PATCH_16x16: SSD_LAUNCH_WP(16, 2); break;
        case SSD_PLAN_WG_PATCH_6x40: SSD_LAUNCH_WP(6, 5); break;
        case SSD_PLAN_WG_PATCH_10x24: SSD_LAUNCH_WP(10, 3); break;
        case SSD_PLAN_WG_TILE: {
            static OnceLds set; if (ensure_lds(set, reinterpret_cast<const void*>(k_conv_wgrad_tile), (int)(4 * WT_TILE)) != 0) return SSD_ERR_LAUNCH;
            hipLaunchKernelGGL(k_conv_wgrad_tile, dim3(p.grid), dim3(512), 4 * WT_TILE, s, x, dy, slab_w, sb, g, p.per_split, p.ns, it.Cout);
            break;
        }
        default: {                                           // SSD_PLAN_WG_GENERIC
            const size_t lds = 4 * 64 * WG_LD;
            static OnceLds set; if (ensure_lds(set, reinterpret_cast<const void*>(k_conv_wgrad), (int)lds) != 0) return SSD_ERR_LAUNCH;
            hipLaunchKernelGGL(k_conv_wgrad, dim3(p.ctiles, p.mtiles, p.ns), dim3(WG), lds, s, x, dy, slab_w, sb, g, p.per_split);
        }
    }
#undef SSD_LAUNCH_WP
    if (hipGetLastError() != hipSuccess) return SSD_ERR_LAUNCH;
    ssd_launch_wgrad_reduce(s, slab_w, (long long)it.ldy * p.ktot, (long long)it.Cout * p.ktot, it.dw, slab_b, (long long)it.ldy,
                            it.Cout, it.dbias, p.ns);
    return ssd_launch_status();
}

int ssd_conv2d_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, int B, int H, int W, int Cin, int Cout,
                          int ldy, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, void* ws, size_t ws_bytes,
                          void* stream) {
    const ssd_wgrad_item it = {x, dy, dw, dbias, B, H, W, Cin, Cout, ldy, ksize, stride, pad_t, pad_l, Ho, Wo};
    return conv2d_bwd_weight_impl(it, ws, ws_bytes, stream);
}

// dispatch query: the plan of the layer (wgrad_plan reads no pointer of the item)
int ssd_conv2d_bwd_weight_plan(int B, int H, int W, int Cin, int Cout, int ldy, int ksize, int stride, int pad_t, int pad_l,
                               int Ho, int Wo) {
    const ssd_wgrad_item it = {nullptr, nullptr, nullptr, nullptr, B, H, W, Cin, Cout, ldy, ksize, stride, pad_t, pad_l, Ho, Wo};
    WgradPlan p;
    const int rc = wgrad_plan(it, &p);
    return rc != SSD_OK ? rc : p.word();
}

// Several SMALL layers' weight gradients in two launches (slab kernel + slab sums) instead of two per layer: the extras on the
// 10x10 ... 1x1 maps (reference models/ssd_model.py:124-150) are six launches of 2-70 workgroups each, ~25 us apiece on the side
// stream beside the other streams' kernels.  Served: the layers whose plan is the generic kernel with fewer than 32 splits (the
// wide reduction's case); SSD_ERR_UNSUPPORTED otherwise, nothing launched.
// Every layer's blocks and sums are the ones its own call would have run: results are bit-identical to separate calls.
size_t ssd_conv2d_bwd_weight_batched_workspace_bytes(const ssd_wgrad_item* items, int count) {
    if (!items || count <= 0) return 0;
    size_t tot = 0;
    for (int i = 0; i < count; ++i) tot += ssd_align_up(wgrad_ws_bytes(items[i]), 256);
    return tot;
}

int ssd_conv2d_bwd_weight_batched(const ssd_wgrad_item* items, int count, void* ws, size_t ws_bytes, void* stream) {
    if (!items || count <= 0) return SSD_ERR_VALUE;
    if (count > WGB_MAX) return SSD_ERR_UNSUPPORTED;
    if (!ws || ws_bytes < ssd_conv2d_bwd_weight_batched_workspace_bytes(items, count)) return SSD_ERR_WORKSPACE;
    WgradBatchArgs wa;
    ReduceBatchArgs ra;
    wa.count = ra.count = count;
    char* ptr = static_cast<char*>(ws);
    int blk = 0, rblk = 0;
    for (int i = 0; i < count; ++i) {
        const ssd_wgrad_item& it = items[i];
        WgradPlan p;
        if (!it.x || !it.dy || !it.dw || wgrad_plan(it, &p) != SSD_OK) return SSD_ERR_VALUE;
        if (p.id != SSD_PLAN_WG_GENERIC || p.ns >= 32) return SSD_ERR_UNSUPPORTED;
        float* slab_w = reinterpret_cast<float*>(ptr);
        float* slab_b = slab_bias(slab_w, p.ns, it.ldy, p.ktot);
        ptr += ssd_align_up(wgrad_ws_bytes(it), 256);
        wa.it[i] = WgradBatchItem{static_cast<const bf16_raw*>(it.x), static_cast<const bf16_raw*>(it.dy), slab_w,
                                  it.dbias ? slab_b : nullptr, wgrad_geom(it), p.per_split, p.ctiles, p.mtiles, blk};
        blk += (int)p.grid;
        const long long nw = (long long)it.Cout * p.ktot;
        const unsigned nbw = (unsigned)((nw / 4 + 255) / 256), nbb = it.dbias ? (unsigned)((it.Cout + 255) / 256) : 0u;
        ra.it[i] = ReduceBatchItem{slab_w, slab_b, it.dw, it.dbias, (long long)it.ldy * p.ktot, nw, (long long)it.ldy, it.Cout, p.ns, rblk, nbw};
        rblk += (int)(nbw + nbb);
    }
    for (int i = count; i < WGB_MAX; ++i) { wa.it[i] = wa.it[0]; wa.it[i].blk0 = blk; ra.it[i] = ra.it[0]; ra.it[i].blk0 = rblk; }
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = 4 * 64 * WG_LD;
    static OnceLds attr_set; if (ensure_lds(attr_set, reinterpret_cast<const void*>(k_conv_wgrad_batched), (int)lds) != 0) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_conv_wgrad_batched, dim3(blk), dim3(WG), lds, s, wa);
    if (hipGetLastError() != hipSuccess) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_wgrad_reduce2_batched, dim3(rblk), dim3(256), 0, s, ra);
    return ssd_launch_status();
}

}  // extern "C"
