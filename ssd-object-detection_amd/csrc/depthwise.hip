// Depthwise 3x3 convolution for gfx950 (MI355X): forward, data gradient and weight gradient of Keras
// DepthwiseConv2D(3, strides = s, depth_multiplier = 1) + bias (+ ReLU) -- the operator a MobileNet-SSD / SSDLite trunk alternates
// with the 1x1 convolution (engine.MOBILENET_V1_SSD300_TRUNK's "dwconv" nodes).  x, y, dy, dx bf16 NHWC; w bf16 [3][3][C]; bias fp32 [C].
//
// Nothing mixes channels, so there is no GEMM: per element two bytes come in, two go out and nine FMAs happen in between.  These are
// streaming kernels.  A lane owns one channel group (8 channels: one 16-byte load or store) of one pixel COLUMN and walks a strip
// of DW_RH rows down it.  Consecutive lanes take consecutive channel groups of a pixel, then the next pixel of the row, then the
// next strip: a wave's access is one contiguous run of the row whatever C is (C = 32: 16 pixels x 4 lanes), and no lane idles
// short of the last wave of the grid.
//   Row reuse is in registers: every source row of the strip is loaded once and feeds the (up to three) output rows it belongs to
//   while their accumulators are live; the strip's walk is unrolled, so each accumulator receives its taps in tap order.
//   Column reuse is the wave's: the three loads of a row step (columns ix-1, ix, ix+1) are the same contiguous run shifted by one
//   pixel, so two of the three are hits in the CU's vector cache.  HBM sees each element once, plus the two halo rows between
//   strips (2 / DW_RH of the rows, served by L2 from the neighbouring strip's loads).
//   An LDS strip would remove the two cached loads per step at the price of a barrier per strip and of workgroup shapes that
//   depend on C and W; the cached loads are not what bounds these kernels.
//   The maps are addressed through buffer descriptors, out-of-map pixels by an offset beyond them (zeros, no branch), and a strip's
//   loads go out in groups of DW_GR rows, each group ahead of the arithmetic of the group before it.
// Grids cover the work (one thread per column strip and channel group); a thread past the end returns at once.
//
// Weight gradient: k_dwconv3x3_wgrad holds the 9 x 8 + 8 sums of its channel group in registers while it walks the column strips
// ("items") of its pixel slab, the workgroup sums its lanes' registers through LDS in lane order and writes one partial row
// [10][C] per slab; k_dwconv3x3_wgrad_reduce adds the slabs in slab order (sixteen fixed runs, then the sixteen run sums in
// order).  No atomics: the result is a function of the shape alone.
#include <algorithm>
#include <cstdint>
#include "common.h"
#include <hip/hip_bf16.h>
#include "conv_common.h"

namespace {

constexpr int DW_RH = 8;                         // rows of a lane's strip
constexpr int DW_NT = 256;
constexpr int DW_GR = 3;                         // source rows per load group (two groups of 3 x DW_GR loads are in registers)
constexpr int DW_WG_RH = 4;                      // weight gradient: rows of a strip (80 sums per lane leave room for fewer loads in flight)
constexpr int DW_WG_NT = 512;                    // weight gradient: at most this many threads, cgx channel groups x ity items
constexpr int DW_WG_ITY = 32;                    // ... and at most this many items side by side (the depth of the LDS sum)

// One thread per (image, strip, column, channel group), channel group fastest.  xbytes / ybytes: the [B,H,W,C] and [B,Ho,Wo,C]
// tensors' sizes, the ranges of their buffer descriptors.
struct DwGeom {
    int H, W, C, Ho, Wo, pad_t, pad_l;
    int c8, cols, nstrips, total;
    unsigned xbytes, ybytes;
    FastDiv d_c8, d_cols, d_strips;
};

// Every access to the maps goes through a buffer descriptor of the tensor's exact size: a lane whose pixel lies outside the map
// (or whose row the strip does not need) gets the offset DW_OOB, beyond every descriptor (tensors are below 2^31 bytes), for
// which a load returns zeros and a store is dropped -- no branch around any access, so a strip's walk is one basic block and its
// loads are issued ahead of the arithmetic that waits for them.
constexpr unsigned DW_OOB = 0x80000000u;
typedef unsigned dw_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t dw_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, 0x00020000);
}

__device__ __forceinline__ void dw_unpack(const dw_u32x4& v, float (&f)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = __uint_as_float(v[k] << 16);
        f[2 * k + 1] = __uint_as_float(v[k] & 0xffff0000u);
    }
}

__device__ __forceinline__ dw_u32x4 dw_pack(const float (&f)[8]) {
    return dw_u32x4{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
}

// bit k: element k of the packed group is > 0, read off the bf16 patterns that are stored, so the byte agrees with the stored map
// whatever the rounding did.  The group has been through max(., 0): no element is negative or a NaN, and -0 counts as zero.
__device__ __forceinline__ unsigned char dw_signs(const dw_u32x4& v) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m |= ((v[k] & 0x00007fffu) ? 1u : 0u) << (2 * k);
        m |= ((v[k] & 0x7fff0000u) ? 1u : 0u) << (2 * k + 1);
    }
    return (unsigned char)m;
}

// off, or an offset beyond the descriptor where !ok.  The empty asm hides that the mask is one of two constants: hipcc otherwise
// splits the strip's walk into branches on the row conditions, and a branch ends the run of loads in flight.
__device__ __forceinline__ unsigned dw_offset(unsigned off, bool ok) {
    unsigned mask = ok ? 0u : DW_OOB;
    asm("" : "+v"(mask));
    return off | mask;
}

__device__ __forceinline__ dw_u32x4 dw_load(__amdgpu_buffer_rsrc_t r, unsigned off, bool ok) {
    return __builtin_amdgcn_raw_buffer_load_b128(r, dw_offset(off, ok), 0, 0);
}

// The nine taps of a channel group are held packed and unpacked where they are used: as a float [9][8] array hipcc kept them in
// scratch in the stride-1 forward kernel.
__device__ __forceinline__ void dw_weights(const bf16_raw* __restrict__ w, int C, int cg, dw_u32x4 (&wq)[9]) {
#pragma unroll
    for (int t = 0; t < 9; ++t) wq[t] = *reinterpret_cast<const dw_u32x4*>(w + t * C + cg * 8);
}

// Output rows o0 .. o0 + DW_RH - 1 of column ox; source row r of the strip is iy = o0 S - pad_t + r and is tap row ky = r - S j
// of output row j.
// BITS: the lane also stores the sign byte of its 16-byte group (bit k: channel 8 cg + k > 0) at [pixel][cg] of `bits`, a sixteenth
// of the group's own byte offset, through a descriptor of that map's exact size: dropped where the 16-byte store is dropped.
template <int S, bool BITS>
__global__ __launch_bounds__(DW_NT) void k_dwconv3x3_fwd(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ w,
                                                         const float* __restrict__ bias, bf16_raw* __restrict__ y,
                                                         unsigned char* __restrict__ bits, DwGeom g, int relu) {
    const int idx = blockIdx.x * DW_NT + threadIdx.x;
    if (idx >= g.total) return;
    const int t0 = fdiv(idx, g.d_c8), cg = idx - t0 * g.c8;
    const int t1 = fdiv(t0, g.d_cols), ox = t0 - t1 * g.cols;
    const int b = fdiv(t1, g.d_strips), o0 = (t1 - b * g.nstrips) * DW_RH;
    const __amdgpu_buffer_rsrc_t xres = dw_rsrc(x, g.xbytes), yres = dw_rsrc(y, g.ybytes);
    const __amdgpu_buffer_rsrc_t bres = dw_rsrc(BITS ? (const void*)bits : (const void*)y, g.ybytes >> 4);
    dw_u32x4 wq[9];
    dw_weights(w, g.C, cg, wq);
    float acc[DW_RH][8];
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0;
    if (bias) {
        b0 = *reinterpret_cast<const float4*>(bias + cg * 8);
        b1 = *reinterpret_cast<const float4*>(bias + cg * 8 + 4);
    }
    const float bv[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    const float floor_ = relu ? 0.f : -INFINITY;
    const int nrows = min(DW_RH, g.Ho - o0);
    const int iy0 = o0 * S - g.pad_t, ix0 = ox * S - g.pad_l;
    const unsigned xoff = (unsigned)(b * g.H * g.W * g.C + cg * 8) * 2u;        // (element indices are below 2^30)
    const unsigned yoff = (unsigned)(((b * g.Ho + o0) * g.Wo + ox) * g.C + cg * 8) * 2u;
    bool colok[3];
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) colok[kx] = (unsigned)(ix0 + kx) < (unsigned)g.W;
    // source rows in groups of DW_GR: the next group's loads are issued before the current group's arithmetic and stores
    constexpr int R = S * (DW_RH - 1) + 3, G = (R + DW_GR - 1) / DW_GR;
    dw_u32x4 buf[2][DW_GR][3];
    auto load_group = [&](int grp) {
#pragma unroll
        for (int rr = 0; rr < DW_GR; ++rr) {
            const int r = grp * DW_GR + rr;
            if (r >= R) continue;
            const int iy = iy0 + r;
            const bool rowok = (unsigned)iy < (unsigned)g.H && r <= S * (nrows - 1) + 2;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
                buf[grp & 1][rr][kx] = dw_load(xres, xoff + (unsigned)((iy * g.W + ix0 + kx) * g.C) * 2u, rowok && colok[kx]);
        }
    };
    load_group(0);
#pragma unroll
    for (int grp = 0; grp < G; ++grp) {
        if (grp + 1 < G) load_group(grp + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rr = 0; rr < DW_GR; ++rr) {
            const int r = grp * DW_GR + rr;
            if (r >= R) continue;
            float xv[3][8];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) dw_unpack(buf[grp & 1][rr][kx], xv[kx]);
#pragma unroll
            for (int j = 0; j < DW_RH; ++j) {
                const int ky = r - S * j;
                if (ky < 0 || ky > 2) continue;
                if (ky == 0) {                                             // an output row starts from the bias at its first tap row
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[j][k] = bv[k];
                }
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    float wv[8];
                    dw_unpack(wq[3 * ky + kx], wv);
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[j][k] += xv[kx][k] * wv[k];
                }
                if (ky != 2) continue;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[j][k] = fmaxf(acc[j][k], floor_);
                const unsigned o = yoff + (unsigned)(j * g.Wo * g.C) * 2u;
                const dw_u32x4 q = dw_pack(acc[j]);
                __builtin_amdgcn_raw_buffer_store_b128(q, yres, dw_offset(o, j < nrows), 0, 0);
                if (BITS) __builtin_amdgcn_raw_buffer_store_b8(dw_signs(q), bres, dw_offset(o >> 4, j < nrows), 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Input rows of a strip in PADDED coordinates u = iy + pad_t: u0 .. u0 + DW_RH - 1 (u0 a multiple of DW_RH, so even) of column
// ix.  Tap row ky of input row j reads output row (u0 + j - ky) / S = u0 / S + m with m = (j - ky) / S where that is integral;
// the output rows are walked from the bottom up, so every input row receives ky = 0, 1, 2 in this order, and kx likewise.
// relu_src may be dx itself: a lane reads its element of either before it stores it, and no other lane touches that element.
// EXTRA: the call accumulates or masks (the plain form reads nothing of dx).
// BITS: the mask is the sign byte [pixel][cg] of relu_bits (relu_src is unused) and EXTRA says whether the call accumulates.  The
// byte of input row j is loaded with the row group in which that row receives its last tap row, so it is in a register a group
// ahead of its use; only the old dx of an accumulating call is still read at the point of use.
template <int S, bool EXTRA, bool BITS = false>
__global__ __launch_bounds__(DW_NT) void k_dwconv3x3_dgrad(const bf16_raw* __restrict__ dy, const bf16_raw* __restrict__ w,
                                                           const bf16_raw* relu_src, const unsigned char* __restrict__ relu_bits,
                                                           bf16_raw* dx, DwGeom g, int accumulate) {
    const int idx = blockIdx.x * DW_NT + threadIdx.x;
    if (idx >= g.total) return;
    const int t0 = fdiv(idx, g.d_c8), cg = idx - t0 * g.c8;
    const int t1 = fdiv(t0, g.d_cols), ix = t0 - t1 * g.cols;
    const int b = fdiv(t1, g.d_strips), u0 = (t1 - b * g.nstrips) * DW_RH;
    const __amdgpu_buffer_rsrc_t dyres = dw_rsrc(dy, g.ybytes), dxres = dw_rsrc(dx, g.xbytes);
    const __amdgpu_buffer_rsrc_t mres = BITS ? dw_rsrc(relu_bits, g.xbytes >> 4) : dw_rsrc(relu_src ? relu_src : dx, g.xbytes);
    const bool masked = BITS || relu_src != nullptr;
    dw_u32x4 wq[9];
    dw_weights(w, g.C, cg, wq);
    float acc[DW_RH][8];
    bool colok[3];
    unsigned coloff[3];
    const unsigned dyoff = (unsigned)(b * g.Ho * g.Wo * g.C + cg * 8) * 2u;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        const int t = ix + g.pad_l - kx, ox = t / S;                        // (t >= 0 wherever ox is used)
        colok[kx] = t >= 0 && (S == 1 || !(t & 1)) && ox < g.Wo;
        coloff[kx] = dyoff + (unsigned)(ox * g.C) * 2u;
    }
    const unsigned xoff = (unsigned)(((b * g.H + u0 - g.pad_t) * g.W + ix) * g.C + cg * 8) * 2u;    // row j: + j W C elements
    // output rows M_HI .. M_LO in groups of DW_GR, as the forward pass groups its source rows
    constexpr int M_LO = S == 1 ? -2 : -1, M_HI = (DW_RH - 1) / S, R = M_HI - M_LO + 1, G = (R + DW_GR - 1) / DW_GR;
    dw_u32x4 buf[2][DW_GR][3];
    unsigned char mbyte[DW_RH];
    auto load_group = [&](int grp) {
#pragma unroll
        for (int rr = 0; rr < DW_GR; ++rr) {
            const int m = M_HI - (grp * DW_GR + rr);
            if (m < M_LO) continue;
            const int oy = u0 / S + m;
            const bool rowok = (unsigned)oy < (unsigned)g.Ho;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) buf[grp & 1][rr][kx] = dw_load(dyres, coloff[kx] + (unsigned)(oy * g.Wo * g.C) * 2u, rowok && colok[kx]);
        }
        if (!BITS) return;
#pragma unroll
        for (int j = 0; j < DW_RH; ++j) {                                  // the input rows that this group completes
            const int kymax = S == 1 ? 2 : ((j & 1) ? 1 : 2);
            if ((M_HI - (j - kymax) / S) / DW_GR != grp) continue;
            const bool inside = (unsigned)(u0 + j - g.pad_t) < (unsigned)g.H;
            mbyte[j] = __builtin_amdgcn_raw_buffer_load_b8(mres, dw_offset((xoff + (unsigned)(j * g.W * g.C) * 2u) >> 4, inside), 0, 0);
        }
    };
    load_group(0);
#pragma unroll
    for (int grp = 0; grp < G; ++grp) {
        if (grp + 1 < G) load_group(grp + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rr = 0; rr < DW_GR; ++rr) {
            const int m = M_HI - (grp * DW_GR + rr);
            if (m < M_LO) continue;
            float gv[3][8];
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) dw_unpack(buf[grp & 1][rr][kx], gv[kx]);
#pragma unroll
            for (int j = 0; j < DW_RH; ++j) {
                const int ky = j - S * m;
                if (ky < 0 || ky > 2) continue;
                if (ky == (S == 1 ? 0 : (j & 1))) {                        // the first tap row input row j receives
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
                }
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    float wv[8];
                    dw_unpack(wq[3 * ky + kx], wv);
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[j][k] += gv[kx][k] * wv[k];
                }
                const int kymax = S == 1 ? 2 : ((j & 1) ? 1 : 2);         // the last tap row input row j receives
                if (ky != kymax) continue;
                const int iy = u0 + j - g.pad_t;
                const bool inside = (unsigned)iy < (unsigned)g.H;
                const unsigned o = xoff + (unsigned)(j * g.W * g.C) * 2u;
                if (BITS) {
                    float old[8];
                    if (EXTRA) dw_unpack(dw_load(dxres, o, inside && accumulate), old);
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[j][k] += EXTRA ? old[k] : 0.f;          // (+ 0: the sibling's sum, bit for bit)
                    dw_u32x4 q = dw_pack(acc[j]);
                    const unsigned mb = mbyte[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k)                                             // a masked element is +0, as the sibling's
                        q[k] &= (((mb >> (2 * k)) & 1u) ? 0x0000ffffu : 0u) | (((mb >> (2 * k + 1)) & 1u) ? 0xffff0000u : 0u);
                    __builtin_amdgcn_raw_buffer_store_b128(q, dxres, dw_offset(o, inside), 0, 0);
                    continue;
                } else if (EXTRA) {
                    float old[8], mk[8];
                    dw_unpack(dw_load(dxres, o, inside && accumulate), old);    // zeros where nothing is accumulated onto
                    dw_unpack(dw_load(mres, o, inside && masked), mk);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const float v = acc[j][k] + old[k];
                        acc[j][k] = (!masked || mk[k] > 0.f) ? v : 0.f;
                    }
                }
                __builtin_amdgcn_raw_buffer_store_b128(dw_pack(acc[j]), dxres, dw_offset(o, inside), 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient.  An item is one column strip (image, strip of DW_WG_RH output rows, output column), numbered column fastest; a
// slab is slab_items consecutive items; grid (slabs, channel tiles of cgx groups); thread = (tx: channel group, ty: item lane),
// cgx * ity threads.  slab [ns][10][C]: rows 0..8 the taps, row 9 the bias gradient.
struct DwWgradPlan {
    int c8, cgx, ity, ctiles, nstrips, n_items, slab_items, ns;
    FastDiv d_cols, d_strips;
};

template <int S>
__global__ __launch_bounds__(DW_WG_NT) void k_dwconv3x3_wgrad(const bf16_raw* __restrict__ x, const bf16_raw* __restrict__ dy,
                                                              float* __restrict__ slab, DwGeom g, DwWgradPlan p) {
    __shared__ float4 red[DW_WG_NT * 2];
    const int tid = threadIdx.x;
    const int ty = tid / p.cgx, tx = tid - ty * p.cgx;
    const int cg = blockIdx.y * p.cgx + tx;
    const bool live = cg < p.c8;
    const __amdgpu_buffer_rsrc_t xres = dw_rsrc(x, g.xbytes), dyres = dw_rsrc(dy, g.ybytes);
    float acc[10][8];
#pragma unroll
    for (int t = 0; t < 10; ++t)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[t][k] = 0.f;
    const int it_end = min(p.n_items, ((int)blockIdx.x + 1) * p.slab_items);
    if (live) {
        for (int it = blockIdx.x * p.slab_items + ty; it < it_end; it += p.ity) {
            const int t1 = fdiv(it, p.d_cols), ox = it - t1 * g.Wo;
            const int b = fdiv(t1, p.d_strips), o0 = (t1 - b * p.nstrips) * DW_WG_RH;
            const int nrows = min(DW_WG_RH, g.Ho - o0);
            const int iy0 = o0 * S - g.pad_t, ix0 = ox * S - g.pad_l;
            const unsigned xoff = (unsigned)(b * g.H * g.W * g.C + cg * 8) * 2u;
            const unsigned dyoff = (unsigned)(((b * g.Ho + o0) * g.Wo + ox) * g.C + cg * 8) * 2u;
            float gv[DW_WG_RH][8];
#pragma unroll
            for (int r = 0; r < S * (DW_WG_RH - 1) + 3; ++r) {
                const int iy = iy0 + r;
                const bool rowok = (unsigned)iy < (unsigned)g.H && r <= S * (nrows - 1) + 2;
                float xv[3][8];
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int ix = ix0 + kx;
                    dw_unpack(dw_load(xres, xoff + (unsigned)((iy * g.W + ix) * g.C) * 2u, rowok && (unsigned)ix < (unsigned)g.W), xv[kx]);
                }
#pragma unroll
                for (int j = 0; j < DW_WG_RH; ++j) {
                    const int ky = r - S * j;
                    if (ky < 0 || ky > 2) continue;
                    if (ky == 0) {
                        dw_unpack(dw_load(dyres, dyoff + (unsigned)(j * g.Wo * g.C) * 2u, j < nrows), gv[j]);
#pragma unroll
                        for (int k = 0; k < 8; ++k) acc[9][k] += gv[j][k];
                    }
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                        for (int k = 0; k < 8; ++k) acc[3 * ky + kx][k] += xv[kx][k] * gv[j][k];
                }
            }
        }
    }
    // the workgroup's sum, item lane by item lane in order: one tap row per pass through LDS
    const int ncols = p.cgx * 2;                                            // float4 columns of a tap row of this channel tile
    float* out = slab + (long long)blockIdx.x * 10 * g.C + (long long)blockIdx.y * p.cgx * 8;
#pragma unroll
    for (int t = 0; t < 10; ++t) {
        red[tid * 2] = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
        red[tid * 2 + 1] = make_float4(acc[t][4], acc[t][5], acc[t][6], acc[t][7]);
        __syncthreads();
        for (int q = tid; q < ncols; q += p.cgx * p.ity) {
            if (blockIdx.y * p.cgx + (q >> 1) >= p.c8) continue;
            float4 s = red[q];
            for (int l = 1; l < p.ity; ++l) {
                const float4 v = red[l * ncols + q];
                s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            }
            *reinterpret_cast<float4*>(out + t * g.C + q * 4) = s;
        }
        __syncthreads();
    }
}

// dw [9][C] and dbias [C] = the sum of the slabs in slab order: sixteen runs of `per` consecutive slabs each, then the sixteen
// run sums in order.  A block takes sixteen float4 columns of the [10][C] row.
__global__ __launch_bounds__(256) void k_dwconv3x3_wgrad_reduce(const float* __restrict__ slab, float* __restrict__ dw,
                                                                float* __restrict__ db, int C, int ns, int per) {
    __shared__ float4 part[16][16];
    const int col = threadIdx.x & 15, run = threadIdx.x >> 4;
    const int n4 = 10 * C / 4;
    const int q = blockIdx.x * 16 + col;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q < n4) {
        const int z1 = min(ns, (run + 1) * per);
        for (int z = run * per; z < z1; ++z) {
            const float4 v = *reinterpret_cast<const float4*>(slab + (long long)z * 10 * C + q * 4);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    part[run][col] = s;
    __syncthreads();
    if (run != 0 || q >= n4) return;
    for (int l = 1; l < 16; ++l) {
        const float4 v = part[l][col];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (q * 4 < 9 * C) *reinterpret_cast<float4*>(dw + q * 4) = s;
    else if (db) *reinterpret_cast<float4*>(db + (q * 4 - 9 * C)) = s;
}

// ------------------------------------------------------------------------------------------------
// Host side
inline bool overlaps(const void* a, long long abytes, const void* b, long long bbytes) {
    if (!a || !b) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

// the implied padding after the map: 0..2
inline bool pad_ok(int n, int no, int stride, int pad) {
    if (pad < 0 || pad > 1) return false;
    const long long after = ((long long)no - 1) * stride + 3 - n - pad;
    return after >= 0 && after <= 2;
}

// a bf16 [B,H,W,C] tensor of 2^31 bytes or more (every factor is below 2^31: no step overflows)
inline bool dw_big(int B, int H, int W, int C) {
    const long long lim = 1ll << 31;
    long long n = (long long)B * H;
    if (n >= lim) return true;
    n *= W;
    return n >= lim || n * C * 2 >= lim;
}

// SSD_OK, SSD_ERR_VALUE or SSD_ERR_UNSUPPORTED for the geometry shared by the three passes
int dw_geometry(int B, int H, int W, int C, int stride, int pad_t, int pad_l, int Ho, int Wo) {
    if (B < 1 || H < 1 || W < 1 || C < 1 || Ho < 1 || Wo < 1 || (stride != 1 && stride != 2)) return SSD_ERR_VALUE;
    if (!pad_ok(H, Ho, stride, pad_t) || !pad_ok(W, Wo, stride, pad_l)) return SSD_ERR_VALUE;
    if (C % 8 || dw_big(B, H, W, C) || dw_big(B, Ho, Wo, C) || 9ll * C * 4 >= (1ll << 31)) return SSD_ERR_UNSUPPORTED;
    return SSD_OK;
}

// cols x rows: the map the threads' columns and strips cover (the output map; the padded input map for the data gradient)
DwGeom dw_geom(int B, int H, int W, int C, int pad_t, int pad_l, int Ho, int Wo, int cols, int rows) {
    DwGeom g;
    g.H = H; g.W = W; g.C = C; g.Ho = Ho; g.Wo = Wo; g.pad_t = pad_t; g.pad_l = pad_l;
    g.c8 = C / 8;
    g.cols = cols;
    g.nstrips = (rows + DW_RH - 1) / DW_RH;
    g.xbytes = (unsigned)((long long)B * H * W * C * 2);
    g.ybytes = (unsigned)((long long)B * Ho * Wo * C * 2);
    g.total = B * g.nstrips * cols * g.c8;                                  // <= elements / 8 (+ one strip of padding): below 2^28
    g.d_c8 = make_fastdiv(g.c8);
    g.d_cols = make_fastdiv(cols);
    g.d_strips = make_fastdiv(g.nstrips);
    return g;
}

// A function of the shape alone: the workspace query and the call agree.  Items side by side: as many as fit DW_WG_NT threads,
// at most DW_WG_ITY; items in a row per lane: so that about 2048 workgroups remain where the shape has them, at most 16.
DwWgradPlan dw_wgrad_plan(int B, int C, int Ho, int Wo) {
    DwWgradPlan p;
    p.c8 = C / 8;
    p.cgx = std::min(p.c8, DW_WG_NT);
    p.ity = std::min(DW_WG_ITY, DW_WG_NT / p.cgx);
    p.ctiles = (p.c8 + p.cgx - 1) / p.cgx;
    p.nstrips = (Ho + DW_WG_RH - 1) / DW_WG_RH;
    p.n_items = B * p.nstrips * Wo;
    const long long per_lane = std::max<long long>(1, std::min<long long>(16, (long long)p.n_items * p.ctiles / ((long long)p.ity * 2048)));
    p.slab_items = p.ity * (int)per_lane;
    p.ns = (p.n_items + p.slab_items - 1) / p.slab_items;
    p.d_cols = make_fastdiv(Wo);
    p.d_strips = make_fastdiv(p.nstrips);
    return p;
}

}  // namespace

extern "C" {

// The forward pass with or without sign bytes (relu_bits u8 [B*Ho*Wo][C/8], an output like y).
static int dw_fwd(const void* x, const void* w, const float* bias, void* y, void* relu_bits, bool want_bits, int B, int H, int W, int C,
                  int stride, int pad_t, int pad_l, int Ho, int Wo, int relu, void* stream) {
    if (!x || !w || !y || (want_bits && !relu_bits)) return SSD_ERR_VALUE;
    const int rc = dw_geometry(B, H, W, C, stride, pad_t, pad_l, Ho, Wo);
    if (rc != SSD_OK) return rc;
    const long long xbytes = (long long)B * H * W * C * 2, ybytes = (long long)B * Ho * Wo * C * 2, bbytes = ybytes / 16;
    if (overlaps(y, ybytes, x, xbytes) || overlaps(y, ybytes, w, 9ll * C * 2) || overlaps(y, ybytes, bias, 4ll * C)) return SSD_ERR_VALUE;
    if (want_bits && (overlaps(relu_bits, bbytes, y, ybytes) || overlaps(relu_bits, bbytes, x, xbytes) ||
                      overlaps(relu_bits, bbytes, w, 9ll * C * 2) || overlaps(relu_bits, bbytes, bias, 4ll * C)))
        return SSD_ERR_VALUE;
    const DwGeom g = dw_geom(B, H, W, C, pad_t, pad_l, Ho, Wo, Wo, Ho);
    const dim3 grid((unsigned)((g.total + DW_NT - 1) / DW_NT));
    auto kern = stride == 1 ? (want_bits ? k_dwconv3x3_fwd<1, true> : k_dwconv3x3_fwd<1, false>)
                            : (want_bits ? k_dwconv3x3_fwd<2, true> : k_dwconv3x3_fwd<2, false>);
    hipLaunchKernelGGL(kern, grid, dim3(DW_NT), 0, (hipStream_t)stream, static_cast<const bf16_raw*>(x), static_cast<const bf16_raw*>(w),
                       bias, static_cast<bf16_raw*>(y), static_cast<unsigned char*>(relu_bits), g, relu ? 1 : 0);
    return ssd_launch_status();
}

int ssd_dwconv3x3_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int stride, int pad_t,
                      int pad_l, int Ho, int Wo, int relu, void* stream) {
    return dw_fwd(x, w, bias, y, nullptr, false, B, H, W, C, stride, pad_t, pad_l, Ho, Wo, relu, stream);
}

int ssd_dwconv3x3_fwd_relubits(const void* x, const void* w, const float* bias, void* y, void* relu_bits, int B, int H, int W, int C,
                               int stride, int pad_t, int pad_l, int Ho, int Wo, void* stream) {
    return dw_fwd(x, w, bias, y, relu_bits, true, B, H, W, C, stride, pad_t, pad_l, Ho, Wo, 1, stream);
}

// The data gradient masked by nothing, by relu_src (bf16, may be dx) or by relu_bits (u8 [B*H*W][C/8], never dx).
static int dw_bwd_data(const void* dy, const void* w, const void* relu_src, const void* relu_bits, bool want_bits, void* dx, int B, int H,
                       int W, int C, int stride, int pad_t, int pad_l, int Ho, int Wo, int accumulate, void* stream) {
    if (!dy || !w || !dx || (want_bits && !relu_bits)) return SSD_ERR_VALUE;
    const int rc = dw_geometry(B, H, W, C, stride, pad_t, pad_l, Ho, Wo);
    if (rc != SSD_OK) return rc;
    const long long dxbytes = (long long)B * H * W * C * 2;
    if (overlaps(dx, dxbytes, dy, (long long)B * Ho * Wo * C * 2) || overlaps(dx, dxbytes, w, 9ll * C * 2)) return SSD_ERR_VALUE;
    if (relu_src && relu_src != dx && overlaps(dx, dxbytes, relu_src, dxbytes)) return SSD_ERR_VALUE;
    if (want_bits && overlaps(dx, dxbytes, relu_bits, dxbytes / 16)) return SSD_ERR_VALUE;
    const DwGeom g = dw_geom(B, H, W, C, pad_t, pad_l, Ho, Wo, W, H + pad_t);
    const dim3 grid((unsigned)((g.total + DW_NT - 1) / DW_NT));
    const bool extra = accumulate || relu_src;
    auto kern = stride == 1 ? (extra ? k_dwconv3x3_dgrad<1, true> : k_dwconv3x3_dgrad<1, false>)
                            : (extra ? k_dwconv3x3_dgrad<2, true> : k_dwconv3x3_dgrad<2, false>);
    if (want_bits)
        kern = stride == 1 ? (accumulate ? k_dwconv3x3_dgrad<1, true, true> : k_dwconv3x3_dgrad<1, false, true>)
                           : (accumulate ? k_dwconv3x3_dgrad<2, true, true> : k_dwconv3x3_dgrad<2, false, true>);
    hipLaunchKernelGGL(kern, grid, dim3(DW_NT), 0, (hipStream_t)stream, static_cast<const bf16_raw*>(dy), static_cast<const bf16_raw*>(w),
                       static_cast<const bf16_raw*>(relu_src), static_cast<const unsigned char*>(relu_bits), static_cast<bf16_raw*>(dx), g,
                       accumulate ? 1 : 0);
    return ssd_launch_status();
}

int ssd_dwconv3x3_bwd_data(const void* dy, const void* w, const void* relu_src, void* dx, int B, int H, int W, int C, int stride,
                           int pad_t, int pad_l, int Ho, int Wo, int accumulate, void* stream) {
    return dw_bwd_data(dy, w, relu_src, nullptr, false, dx, B, H, W, C, stride, pad_t, pad_l, Ho, Wo, accumulate, stream);
}

int ssd_dwconv3x3_bwd_data_bits(const void* dy, const void* w, const void* relu_bits, void* dx, int B, int H, int W, int C, int stride,
                                int pad_t, int pad_l, int Ho, int Wo, int accumulate, void* stream) {
    return dw_bwd_data(dy, w, nullptr, relu_bits, true, dx, B, H, W, C, stride, pad_t, pad_l, Ho, Wo, accumulate, stream);
}

size_t ssd_dwconv3x3_bwd_weight_workspace_bytes(int B, int H, int W, int C, int stride, int Ho, int Wo) {
    if (B < 1 || H < 1 || W < 1 || C < 1 || Ho < 1 || Wo < 1 || (stride != 1 && stride != 2) || C % 8) return 0;
    if (dw_big(B, H, W, C) || dw_big(B, Ho, Wo, C) || 9ll * C * 4 >= (1ll << 31)) return 0;
    return (size_t)dw_wgrad_plan(B, C, Ho, Wo).ns * 10 * (size_t)C * sizeof(float);
}

int ssd_dwconv3x3_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, int B, int H, int W, int C, int stride,
                             int pad_t, int pad_l, int Ho, int Wo, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !dy || !dw) return SSD_ERR_VALUE;
    const int rc = dw_geometry(B, H, W, C, stride, pad_t, pad_l, Ho, Wo);
    if (rc != SSD_OK) return rc;
    const long long xbytes = (long long)B * H * W * C * 2, dybytes = (long long)B * Ho * Wo * C * 2, dwbytes = 9ll * C * 4;
    if (overlaps(dw, dwbytes, x, xbytes) || overlaps(dw, dwbytes, dy, dybytes) || overlaps(dbias, 4ll * C, x, xbytes) ||
        overlaps(dbias, 4ll * C, dy, dybytes) || overlaps(dbias, 4ll * C, dw, dwbytes))
        return SSD_ERR_VALUE;
    const DwWgradPlan p = dw_wgrad_plan(B, C, Ho, Wo);
    const size_t need = (size_t)p.ns * 10 * (size_t)C * sizeof(float);
    if (!ws || ws_bytes < need) return SSD_ERR_WORKSPACE;
    if (overlaps(ws, (long long)need, x, xbytes) || overlaps(ws, (long long)need, dy, dybytes) || overlaps(ws, (long long)need, dw, dwbytes) ||
        overlaps(ws, (long long)need, dbias, 4ll * C))
        return SSD_ERR_VALUE;
    const DwGeom g = dw_geom(B, H, W, C, pad_t, pad_l, Ho, Wo, Wo, Ho);
    hipStream_t s = (hipStream_t)stream;
    float* slab = static_cast<float*>(ws);
    auto kern = stride == 1 ? k_dwconv3x3_wgrad<1> : k_dwconv3x3_wgrad<2>;
    hipLaunchKernelGGL(kern, dim3(p.ns, p.ctiles), dim3(p.cgx * p.ity), 0, s, static_cast<const bf16_raw*>(x),
                       static_cast<const bf16_raw*>(dy), slab, g, p);
    if (hipGetLastError() != hipSuccess) return SSD_ERR_LAUNCH;
    const int n4 = 10 * C / 4;
    hipLaunchKernelGGL(k_dwconv3x3_wgrad_reduce, dim3((n4 + 15) / 16), dim3(256), 0, s, slab, dw, dbias, C, p.ns, (p.ns + 15) / 16);
    return ssd_launch_status();
}

}  // extern "C"
