// Softmax focal loss (Lin et al. 2017, "Focal Loss for Dense Object Detection", in its softmax form), forward + backward, for
// gfx950 (MI355X).  Opt-in, next to the reference's loss (loss.hip) and MultiBox (multibox.hip).  Every anchor stays in the
// classification term, weighted by (1 - p_t)^gamma; nothing is mined, so there is no select and no histogram:
//   t = gt_cls[a] if gt_mask[a] else C-1;  e_j = exp(z_j - max z);  Q = sum_{j != t} e_j;  S = Q + e_t;  q = Q / S (= 1 - p_t)
//   log p_t = log1p(-q) if q < 0.5 else (z_t - max z) - log S           (neither form cancels)
//   FL(a) = -alpha_t q^gamma log p_t;  L_pos = sum_pos FL / P;  L_neg = sum_{not pos} FL / P;  L_loc as MultiBox (boxterm.h:
//   smooth L1, or an IoU kind through the _box entries, in an instantiation of k_sf_rows of its own)
//   dconf[a, j] = grad_scale / P * alpha_t * (delta_tj - p_j) * (gamma p_t q^(gamma-1) log p_t - q^gamma)
// evaluated as -q^gamma (gamma p_t h + 1) with h = -log p_t / q (h = 1 at q == 0), which is finite at q == 0, and with
// delta_tt - p_t taken as q.
//
// Three launches, dense and rows form alike: k_sf_count (P from gt_mask: the pass below scales by 1 / P) -> k_sf_rows (conf read
// once through LDS with k_mb_rows' staging, the gradient computed in place there and written once; per-block f64 partial sums)
// -> k_sf_scalars (out8).  No atomics; every workspace word is written before it is read, so the workspace needs no initial
// contents.  All reductions are integer counts or fixed-order f64 sums: the results are bitwise reproducible.
#include "common.h"
#include <hip/hip_bf16.h>
#include <cmath>
#include "conv_common.h"
#include "rowblock.h"
#include "boxterm.h"

namespace {

static_assert(WG == 256, "two threads per anchor row (WG: conv_common.h)");
constexpr int ROWS = 128;                    // anchor rows per workgroup iteration (2 threads per row)
constexpr int CNT_CHUNK = 4096;              // mask bytes per workgroup of k_sf_count
constexpr int MAX_PERSIST = 768;             // 3 workgroups per CU
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr size_t rows_lds_bytes(int C) { return ((size_t)ROWS * C * sizeof(float) + 15) / 16 * 16; }
// k_sf_rows keeps [ROWS][C] f32 next to < 2 KB of reduction slots and row pointers
static_assert(rows_lds_bytes(SSD_LOSS_MAX_CLASSES) + 2048 <= LDS_LIMIT, "C bound of ssd_hip.h");

struct SfWs {                                // layout of the caller's workspace
    int* cnt;                                // [nc] positives per CNT_CHUNK mask bytes
    double* part_pos;                        // [nblk] per-block sum of the positives' FL
    double* part_neg;                        // [nblk] ... of the other anchors' FL
    double* part_sl1;                        // [nblk] ... of the positives' box term (smooth L1 or an IoU kind)
    int* bad;                                // [nblk] a logit of the block, or an offset of one of its positives, was not finite
};

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

inline size_t sf_ws_layout(size_t n, char* base, SfWs* w) {
    const size_t nblk = (n + ROWS - 1) / ROWS, nc = (n + CNT_CHUNK - 1) / CNT_CHUNK;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
    char* p_cnt = take(nc * sizeof(int));
    char* p_pp = take(nblk * sizeof(double));
    char* p_pn = take(nblk * sizeof(double));
    char* p_pl = take(nblk * sizeof(double));
    char* p_bad = take(nblk * sizeof(int));
    if (w) {
        w->cnt = (int*)p_cnt; w->part_pos = (double*)p_pp; w->part_neg = (double*)p_pn; w->part_sl1 = (double*)p_pl;
        w->bad = (int*)p_bad;
    }
    return off;
}

struct SfParams {
    size_t n, nblk;
    int nc, A, B, C;
    float gamma, alpha_fg, alpha_bg;         // alpha_t of a target class / of the background (both 1 with alpha == -1)
    float loc_weight, grad_scale;
};


struct SfLevels {                            // the rows form's geometry
    int levels;
    int hw[SSD_MAX_LEVELS], n[SSD_MAX_LEVELS], npad[SSD_MAX_LEVELS], off[SSD_MAX_LEVELS + 1];
    __hip_bfloat16* rows[SSD_MAX_LEVELS];
    int* rop[SSD_MAX_LEVELS];
    int* por[SSD_MAX_LEVELS];
    int* count;                              // [SSD_MAX_LEVELS]
};

// ------------------------------------------------------------------------------------------------
// Launch 1: positives per chunk of the mask (byte loads: a micro-batch's slice of the mask is not 16-byte aligned).
__global__ __launch_bounds__(WG) void k_sf_count(const uint8_t* __restrict__ mask, size_t n, int* __restrict__ cnt) {
    __shared__ int s_redi[4];
    const size_t i0 = (size_t)blockIdx.x * CNT_CHUNK;
    int c = 0;
#pragma unroll
    for (int i = 0; i < CNT_CHUNK / WG; ++i) {
        const size_t g = i0 + (size_t)i * WG + threadIdx.x;
        c += (g < n && mask[g] != 0) ? 1 : 0;
    }
    const int tot = block_sum_int<4>(c, s_redi);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

// P of the call, by every thread of a 256-thread workgroup
__device__ __forceinline__ int sf_total_pos(const int* __restrict__ cnt, int nc, int* s_redi) {
    int v = 0;
    for (int i = threadIdx.x; i < nc; i += WG) v += cnt[i];
    return block_sum_int<4>(v, s_redi);
}

// One anchor row in LDS, by its two threads (adjacent lanes): the logits z[0..C) are replaced by the row of dconf.  Returns
// FL(a); *bad is set where a logit is not finite.  Both threads compute the row scalars (the same operations in the same order).
template <int CC>
__device__ __forceinline__ float focal_row(float* z, int C_rt, int t, int half, const SfParams& p, float sc, bool* bad) {
    const int C = CC ? CC : C_rt;
    const int k0 = half ? (C + 1) / 2 : 0, k1 = half ? C : (C + 1) / 2;
    const float zt = z[t];
    float m = -INFINITY;
    bool nf = false;
    for (int k = k0; k < k1; ++k) {
        const float v = z[k];
        nf |= !(fabsf(v) < INFINITY);
        m = fmaxf(m, v);
    }
    m = fmaxf(m, __shfl_xor(m, 1));
    nf |= __shfl_xor((int)nf, 1) != 0;
    float qh = 0.f;
    for (int k = k0; k < k1; ++k) {
        const float e = expf(z[k] - m);
        z[k] = e;
        qh += k == t ? 0.f : e;
    }
    const float Q = qh + __shfl_xor(qh, 1);                   // (lane 0: Q0 + Q1, lane 1: Q1 + Q0 -- the same bits)
    const float et = expf(zt - m);
    const float S = Q + et;                                   // >= 1: the row's maximum contributes exp(0)
    const float inv = 1.f / S;
    const float q = Q / S, pt = et / S;
    const float logpt = q < 0.5f ? log1pf(-q) : (zt - m) - logf(S);
    const float qg = powf(q, p.gamma);                        // (pow(q, 0) == 1, q == 0 included)
    const float h = q > 0.f ? -logpt / q : 1.f;
    const float alpha_t = t != C - 1 ? p.alpha_fg : p.alpha_bg;
    const float coef = sc * alpha_t * -(qg * (p.gamma * pt * h + 1.f));
    for (int k = k0; k < k1; ++k) z[k] = coef * (k == t ? q : -(z[k] * inv));
    *bad = nf;
    return -alpha_t * qg * logpt;
}

// Launch 2.  Persistent grid over blocks of ROWS anchor rows, k_mb_rows' staging (the next block's logits are requested before
// the current block is computed on).  ROWSFORM: the gradient goes to the compact rows of `h` (every pixel is a row: the maps
// are the identity) instead of dconf / dloc.
template <typename T, int CC, bool ROWSFORM, bool IOU>
__global__ __launch_bounds__(WG) void k_sf_rows(const T* __restrict__ conf, const T* __restrict__ loc,
                                                const int* __restrict__ cls, const float* __restrict__ gloc,
                                                const uint8_t* __restrict__ mask, SfParams p, T* __restrict__ dconf,
                                                T* __restrict__ dloc, SfWs w, SfLevels h, BoxArgs bx) {
    extern __shared__ __attribute__((aligned(16))) float s_z[];   // [ROWS*C]: logits, then the gradient block
    __shared__ double s_red[4];
    __shared__ int s_redi[4];
    __shared__ T* s_dst[ROWSFORM ? ROWS : 1];                     // rows form: where a row's C gradient elements go
    const int C = CC ? CC : p.C;
    const size_t n = p.n, nblk = p.nblk;
    const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
    const int P = sf_total_pos(w.cnt, p.nc, s_redi);
    const float sc = P > 0 ? p.grad_scale / (float)P : 0.f;
    const float sl = box_scale(p.grad_scale, p.loc_weight, P);
    if (ROWSFORM && blockIdx.x == 0 && (int)threadIdx.x < h.levels) h.count[threadIdx.x] = P > 0 ? p.B * h.hw[threadIdx.x] : 0;
    constexpr int NV = CC ? (ROWS * CC * (int)sizeof(T) / 16 + WG - 1) / WG : 1;
    uint4 raw[NV];
    if constexpr (CC != 0) {
        if (blockIdx.x < nblk) {
            const size_t row0 = (size_t)blockIdx.x * ROWS;
            stage_load<T, NV>(conf + row0 * C, (size_t)min((size_t)ROWS, n - row0) * C, raw);
        }
    }
    for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const size_t row0 = blk * ROWS;
        const int nrow = (int)min((size_t)ROWS, n - row0);
        __syncthreads();                                   // the previous block's gradient has left LDS
        if constexpr (CC != 0) stage_store<T, NV>(conf + row0 * C, (size_t)nrow * C, raw, s_z);
        else stage_block<T>(conf + row0 * C, (size_t)nrow * C, s_z);
        __syncthreads();
        if constexpr (CC != 0) {
            const size_t nxt = blk + gridDim.x;
            if (nxt < nblk) {
                const size_t r1 = nxt * ROWS;
                stage_load<T, NV>(conf + r1 * C, (size_t)min((size_t)ROWS, n - r1) * C, raw);
            }
        }
        double acc_pos = 0.0, acc_neg = 0.0, acc_sl1 = 0.0;
        int my_bad = 0;
        if (r < nrow) {
            const size_t g = row0 + r;
            const bool pos = mask[g] != 0;
            const int t = pos ? min(max(cls[g], 0), C - 1) : C - 1;   // (a label outside [0, C) must not index past the row)
            bool nf;
            const float fl = focal_row<CC>(s_z + r * C, C, t, half, p, sc, &nf);
            if (half == 0) {
                my_bad = nf ? 1 : 0;
                if (pos) acc_pos = (double)fl; else acc_neg = (double)fl;
                float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
                if (pos) {
                    const float4 gl = reinterpret_cast<const float4*>(gloc)[g];
                    if constexpr (IOU) {
                        acc_sl1 = box_term<T>(bx, p.A, g, loc + 4 * g, gl, sl, &d);
                    } else {
                        acc_sl1 = box_loss<T>(loc + 4 * g, gl);
                        d = box_grad<T>(loc + 4 * g, gl, sl);
                    }
                }
                T* ol;
                if constexpr (ROWSFORM) {
                    const int b = (int)(g / (size_t)p.A);
                    const int a = (int)(g - (size_t)b * p.A);
                    int l = 0;
                    for (int k = 1; k < h.levels; ++k) l += a >= h.off[k] ? 1 : 0;
                    const int idx = a - h.off[l], nl = h.n[l];
                    const int pix = idx / nl, slot = idx - pix * nl;
                    const int row = b * h.hw[l] + pix;
                    T* dr = h.rows[l] + (size_t)row * h.npad[l];
                    s_dst[r] = dr + nl * 4 + slot * C;
                    ol = dr + slot * 4;
                    if (slot == 0) {                              // the pixel's first anchor: its maps and the row's zero padding
                        h.rop[l][row] = P > 0 ? row : -1;
                        h.por[l][row] = row;
                        for (int k = nl * (4 + C); k < h.npad[l]; ++k) dr[k] = from_f32<T>(0.f);
                    }
                } else {
                    ol = dloc + 4 * g;
                }
                ol[0] = from_f32<T>(d.x); ol[1] = from_f32<T>(d.y); ol[2] = from_f32<T>(d.z); ol[3] = from_f32<T>(d.w);
            }
        }
        // (the sums' barriers also publish the gradient block and s_dst)
        const double bp = block_sum<4>(acc_pos, s_red);
        const double bn = block_sum<4>(acc_neg, s_red);
        const double bl = block_sum<4>(acc_sl1, s_red);
        const int bb = block_sum_int<4>(my_bad, s_redi);
        if (threadIdx.x == 0) { w.part_pos[blk] = bp; w.part_neg[blk] = bn; w.part_sl1[blk] = bl; w.bad[blk] = bb; }
        if constexpr (ROWSFORM) {
            // consecutive lanes write consecutive elements of a row's conf channels
            const int count = nrow * C;
            for (int i = threadIdx.x; i < count; i += WG) {
                const int rr = i / C, k = i - rr * C;
                s_dst[rr][k] = from_f32<T>(s_z[i]);
            }
        } else {
            store_block<T>(dconf + row0 * C, s_z, (size_t)nrow * C);
        }
    }
}

// Launch 3: out8 = L_loc, L_pos, L_neg, total, P, N, 0, status, by one 256-thread workgroup.
__global__ __launch_bounds__(WG) void k_sf_scalars(SfWs w, SfParams p, float* __restrict__ out) {
    __shared__ double s_red[4];
    __shared__ int s_redi[4];
    const int P = sf_total_pos(w.cnt, p.nc, s_redi);
    double a = 0.0, b = 0.0, c = 0.0;
    int bad = 0;
    for (size_t i = threadIdx.x; i < p.nblk; i += WG) {
        a += w.part_pos[i]; b += w.part_neg[i]; c += w.part_sl1[i];
        bad |= w.bad[i];
    }
    a = block_sum<4>(a, s_red);
    b = block_sum<4>(b, s_red);
    c = block_sum<4>(c, s_red);
    bad = block_sum_int<4>(bad != 0 ? 1 : 0, s_redi);
    if (threadIdx.x == 0) {
        const bool ok = P > 0;
        const double dp = (double)P;
        const float l_pos = ok ? (float)(a / dp) : 0.f;
        const float l_neg = ok ? (float)(b / dp) : 0.f;
        const float l_loc = ok ? (float)((double)p.loc_weight * c / dp) : 0.f;
        out[0] = l_loc; out[1] = l_pos; out[2] = l_neg; out[3] = (l_loc + l_pos) + l_neg;
        out[4] = (float)P; out[5] = (float)((long long)p.n - P); out[6] = 0.f;
        const bool nf = bad != 0 || !(fabs(a) < (double)INFINITY) || !(fabs(b) < (double)INFINITY) || !(fabs(c) < (double)INFINITY);
        out[7] = nf ? 3.f : (ok ? 0.f : 1.f);
    }
}

template <typename T, int CC, bool ROWSFORM, bool IOU>
int launch_rows(const void* conf, const void* loc, const int32_t* cls, const float* gloc, const uint8_t* mask,
                const SfParams& p, const BoxArgs& bx, void* dconf, void* dloc, const SfWs& w, const SfLevels& h, hipStream_t s) {
    // more than 64 KB of dynamic LDS is registered once per device and kernel, for the largest block the bounds admit
    static OnceLds once;
    const size_t lds = rows_lds_bytes(p.C);
    if (lds > 64 * 1024 && ensure_lds(once, reinterpret_cast<const void*>(k_sf_rows<T, CC, ROWSFORM, IOU>),
                                      (int)rows_lds_bytes(SSD_LOSS_MAX_CLASSES)))
        return SSD_ERR_LAUNCH;
    const unsigned pgrid = (unsigned)min((size_t)MAX_PERSIST, p.nblk);
    hipLaunchKernelGGL((k_sf_rows<T, CC, ROWSFORM, IOU>), dim3(pgrid), dim3(WG), lds, s, (const T*)conf, (const T*)loc, cls, gloc,
                       mask, p, (T*)dconf, (T*)dloc, w, h, bx);
    return 0;
}

// the three launches of either form
template <typename T, bool ROWSFORM>
int launch_all(const void* conf, const void* loc, const int32_t* cls, const float* gloc, const uint8_t* mask,
               const SfParams& p, const BoxArgs& bx, float* out, void* dconf, void* dloc, const SfWs& w, const SfLevels& h,
               hipStream_t s) {
    hipLaunchKernelGGL(k_sf_count, dim3((unsigned)p.nc), dim3(WG), 0, s, mask, p.n, w.cnt);
    int rc;
    if (bx.kind != SSD_BOX_SMOOTH_L1)
        rc = p.C == 81 ? launch_rows<T, 81, ROWSFORM, true>(conf, loc, cls, gloc, mask, p, bx, dconf, dloc, w, h, s)
                       : launch_rows<T, 0, ROWSFORM, true>(conf, loc, cls, gloc, mask, p, bx, dconf, dloc, w, h, s);
    else
        rc = p.C == 81 ? launch_rows<T, 81, ROWSFORM, false>(conf, loc, cls, gloc, mask, p, bx, dconf, dloc, w, h, s)
                       : launch_rows<T, 0, ROWSFORM, false>(conf, loc, cls, gloc, mask, p, bx, dconf, dloc, w, h, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_sf_scalars, dim3(1), dim3(WG), 0, s, w, p, out);
    return ssd_launch_status();
}

// the refusals both entries share, before any launch
int sf_check(const void* conf, const void* loc, int dtype, const int32_t* cls, const float* gloc, const uint8_t* mask, int B,
             int A, int C, float gamma, float alpha, float loc_weight, float grad_scale, const float* out8, int box_kind,
             const double* priors, SfParams* p, BoxArgs* bx) {
    if (box_kind < SSD_BOX_SMOOTH_L1 || box_kind > SSD_BOX_CIOU || (box_kind != SSD_BOX_SMOOTH_L1 && !priors)) return SSD_ERR_VALUE;
    if (!std::isfinite(gamma) || gamma < 0.f || gamma > 8.f) return SSD_ERR_VALUE;
    if (!((alpha >= 0.f && alpha <= 1.f) || alpha == -1.f)) return SSD_ERR_VALUE;
    if (!std::isfinite(loc_weight) || loc_weight < 0.f || !std::isfinite(grad_scale)) return SSD_ERR_VALUE;
    if (dtype != SSD_F32 && dtype != SSD_BF16) return SSD_ERR_VALUE;
    if (B <= 0 || A <= 0 || C < 2) return SSD_ERR_VALUE;
    if (!conf || !loc || !cls || !gloc || !mask || !out8) return SSD_ERR_VALUE;
    if (C > SSD_LOSS_MAX_CLASSES) return SSD_ERR_UNSUPPORTED;
    p->n = (size_t)B * A; p->nblk = (p->n + ROWS - 1) / ROWS;
    if (p->nblk >= (1ull << 31)) return SSD_ERR_UNSUPPORTED;
    p->nc = (int)((p->n + CNT_CHUNK - 1) / CNT_CHUNK);
    p->A = A; p->B = B; p->C = C; p->gamma = gamma;
    p->alpha_fg = alpha == -1.f ? 1.f : alpha;
    p->alpha_bg = alpha == -1.f ? 1.f : 1.f - alpha;
    p->loc_weight = loc_weight; p->grad_scale = grad_scale;
    bx->kind = box_kind; bx->priors = priors;
    return 0;
}

}  // namespace

extern "C" {

size_t ssd_softmax_focal_loss_workspace_bytes(int B, int A, int C) {
    if (B <= 0 || A <= 0 || C <= 0) return 0;
    return sf_ws_layout((size_t)B * A, nullptr, nullptr);
}

size_t ssd_softmax_focal_loss_heads_workspace_bytes(int B, int A, int C) { return ssd_softmax_focal_loss_workspace_bytes(B, A, C); }

int ssd_softmax_focal_loss_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                   const uint8_t* gt_mask, int B, int A, int C, float gamma, float alpha, float loc_weight,
                                   float grad_scale, float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes,
                                   void* stream) {
    return ssd_softmax_focal_loss_box_fwd_bwd(conf, loc, dtype, gt_cls, gt_loc, gt_mask, B, A, C, gamma, alpha, loc_weight,
                                              grad_scale, out8, dconf, dloc, ws, ws_bytes, stream, SSD_BOX_SMOOTH_L1, nullptr);
}

int ssd_softmax_focal_loss_box_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                       const uint8_t* gt_mask, int B, int A, int C, float gamma, float alpha, float loc_weight,
                                       float grad_scale, float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes,
                                       void* stream, int box_kind, const double* priors) {
    SfParams p;
    BoxArgs bx;
    if (int rc = sf_check(conf, loc, dtype, gt_cls, gt_loc, gt_mask, B, A, C, gamma, alpha, loc_weight, grad_scale, out8, box_kind, priors, &p, &bx)) return rc;
    if (!dconf || !dloc) return SSD_ERR_VALUE;
    if (!ws || ws_bytes < sf_ws_layout(p.n, nullptr, nullptr)) return SSD_ERR_WORKSPACE;
    SfWs w;
    sf_ws_layout(p.n, static_cast<char*>(ws), &w);
    const SfLevels h = {};
    hipStream_t s = (hipStream_t)stream;
    if (dtype == SSD_F32) return launch_all<float, false>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, out8, dconf, dloc, w, h, s);
    return launch_all<__hip_bfloat16, false>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, out8, dconf, dloc, w, h, s);
}

int ssd_softmax_focal_loss_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                         const uint8_t* gt_mask, int B, int A, int C, float gamma, float alpha,
                                         float loc_weight, float grad_scale, float* out8, const ssd_head_grads* hg, void* ws,
                                         size_t ws_bytes, void* stream) {
    return ssd_softmax_focal_loss_box_fwd_bwd_heads(conf, loc, dtype, gt_cls, gt_loc, gt_mask, B, A, C, gamma, alpha, loc_weight,
                                                    grad_scale, out8, hg, ws, ws_bytes, stream, SSD_BOX_SMOOTH_L1, nullptr);
}

int ssd_softmax_focal_loss_box_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls,
                                             const float* gt_loc, const uint8_t* gt_mask, int B, int A, int C, float gamma,
                                             float alpha, float loc_weight, float grad_scale, float* out8,
                                             const ssd_head_grads* hg, void* ws, size_t ws_bytes, void* stream, int box_kind,
                                             const double* priors) {
    SfParams p;
    BoxArgs bx;
    if (int rc = sf_check(conf, loc, dtype, gt_cls, gt_loc, gt_mask, B, A, C, gamma, alpha, loc_weight, grad_scale, out8, box_kind, priors, &p, &bx)) return rc;
    if (dtype != SSD_BF16) return SSD_ERR_UNSUPPORTED;
    if (!hg || !hg->count || hg->levels <= 0 || hg->levels > SSD_MAX_LEVELS) return SSD_ERR_VALUE;
    SfLevels h = {};
    h.levels = hg->levels;
    long long off = 0;
    for (int l = 0; l < hg->levels; ++l) {
        if (hg->hw[l] <= 0 || hg->per_cell[l] <= 0 || hg->npad[l] < hg->per_cell[l] * (4 + C) || (hg->npad[l] & 7)) return SSD_ERR_VALUE;
        if (!hg->rows[l] || !hg->row_of_pixel[l] || !hg->pixel_of_row[l]) return SSD_ERR_VALUE;
        if ((long long)B * hg->hw[l] >= (1ll << 31)) return SSD_ERR_VALUE;
        h.hw[l] = hg->hw[l]; h.n[l] = hg->per_cell[l]; h.npad[l] = hg->npad[l];
        off += (long long)hg->hw[l] * hg->per_cell[l];
        if (off > A) return SSD_ERR_ASSERT;
        h.off[l + 1] = (int)off;
        h.rows[l] = (__hip_bfloat16*)hg->rows[l]; h.rop[l] = hg->row_of_pixel[l]; h.por[l] = hg->pixel_of_row[l];
    }
    for (int l = hg->levels; l < SSD_MAX_LEVELS; ++l) h.off[l + 1] = h.off[l];
    if (off != A) return SSD_ERR_ASSERT;                          // the levels tile the anchors, as for MultiBox
    h.count = hg->count;
    if (!ws || ws_bytes < sf_ws_layout(p.n, nullptr, nullptr)) return SSD_ERR_WORKSPACE;
    SfWs w;
    sf_ws_layout(p.n, static_cast<char*>(ws), &w);
    return launch_all<__hip_bfloat16, true>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, out8, nullptr, nullptr, w, h, (hipStream_t)stream);
}

}  // extern "C"
