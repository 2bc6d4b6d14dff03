// The SSD paper's MultiBox loss (Liu et al. 2016, eq. 1-3), forward + backward, for gfx950 (MI355X).  Opt-in: the reference's
// loss (loss.hip) stays the default.  It differs from that loss in three ways:
//   * hard negatives are mined PER IMAGE: image b keeps its k_b = min(ratio * P_b, A - P_b) non-positive anchors of largest
//     key(a) = CE(a, background) (ties at the k_b-th key kept), an image without positives mines nothing;
//   * the box term is smooth L1 (gradient: the difference clamped to [-1, 1]), or, by the box kind of the _box entries, the GIoU /
//     DIoU / CIoU loss of the decoded boxes (boxterm.h; the kernels that evaluate it are instantiations of their own, so the
//     smooth-L1 kernels are the code they were);
//   * all three terms are divided by the number of positives P of the call.
//   L_pos = sum_pos CE(a, gt_cls) / P;  L_neg = sum_neg key(a) / P;  L_loc = alpha * sum_pos sum_4 smoothL1(loc - gt_loc) / P
//   dconf = grad_scale / P * [pos * (softmax - onehot(gt_cls)) + neg * (softmax - onehot(C-1))]
//   dloc  = grad_scale * alpha / P * pos * clamp(loc - gt_loc, -1, 1)
//
// Launches: k_mb_rows (conf read once through LDS: lse, key, per-block f64 partial sums) -> k_mb_select (one workgroup per
// image: P_b, exact radix select of tau_b over the image's keys held in LDS, N_b, the f64 sum of the mined keys, a slice of the
// block partial sums, for the rows form the per-level pixel counts) -> dense: k_mb_grad | rows: k_mb_assign, k_mb_grad_rows.
// The scalars are written by workgroup 0 of the launch behind the select.  No global atomics, no histograms in global memory:
// every workspace word is written before it is read, so the workspace needs no initial contents.  All reductions are integer
// counts or fixed-order f64 sums.
#include "common.h"
#include <hip/hip_bf16.h>
#include <cmath>
#include "conv_common.h"
#include "rowblock.h"
#include "boxterm.h"

namespace {

static_assert(WG == 256, "two threads per anchor row (WG: conv_common.h)");
constexpr int ROWS = 128;                    // anchor rows per workgroup (2 threads per row)
constexpr int SWG = 1024;                    // threads of a select workgroup (16 waves)
constexpr int SWAVES = SWG / 64;
constexpr int HB = 2048;                     // bins of the widest radix digit: 11 + 11 + 10 bits
constexpr int MAX_PERSIST = 768;             // 3 workgroups per CU
constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr size_t rows_lds_bytes(int C) { return ((size_t)ROWS * C * sizeof(float) + 15) / 16 * 16; }
// k_mb_rows / k_mb_grad keep [ROWS][C] f32 next to 32 bytes of reduction slots: every C the reference loss admits fits
static_assert(rows_lds_bytes(SSD_LOSS_MAX_CLASSES) + 64 <= LDS_LIMIT, "C bound of ssd_hip.h");
// k_mb_select keeps the image's A keys (dynamic) next to the digit histogram and the reduction slots (static, < 12 KB)
constexpr size_t SELECT_STATIC_LDS = 12 * 1024;
constexpr size_t select_lds_bytes(int A) { return ((size_t)A * sizeof(unsigned) + 15) / 16 * 16; }
static_assert(select_lds_bytes(SSD_MULTIBOX_MAX_ANCHORS) + SELECT_STATIC_LDS <= LDS_LIMIT, "A bound of ssd_hip.h");
constexpr unsigned POS_KEY = 0xffffffffu;    // a positive's slot in the LDS key array (no candidate carries it: see k_mb_select)

struct MbWs {                                // layout of the caller's workspace
    float* key;                              // [n] background CE of every anchor
    float* lse;                              // [n] logsumexp per anchor
    double* part_pos;                        // [nblk] per-block sum of the positives' CE (NaN: a logit row was not finite)
    double* part_sl1;                        // [nblk] per-block sum of the positives' box term (smooth L1 or an IoU kind)
    unsigned* img_tau;                       // [B] bits of tau_b
    int* img_mined;                          // [B] k_b > 0
    int* img_P;                              // [B]
    int* img_N;                              // [B]
    double* img_sum;                         // [3][B]: mined keys | slice of part_pos | slice of part_sl1
    int* img_count;                          // [SSD_MAX_LEVELS][B] pixels with a selected anchor (rows form)
};

inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }

inline size_t mb_ws_layout(size_t B, size_t A, char* base, MbWs* w) {
    const size_t n = B * A, nblk = (n + ROWS - 1) / ROWS;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += al256(bytes); return p; };
    char* p_key = take(n * sizeof(float));
    char* p_lse = take(n * sizeof(float));
    char* p_pp = take(nblk * sizeof(double));
    char* p_pl = take(nblk * sizeof(double));
    char* p_tau = take(B * sizeof(unsigned));
    char* p_mined = take(B * sizeof(int));
    char* p_P = take(B * sizeof(int));
    char* p_N = take(B * sizeof(int));
    char* p_sum = take(3 * B * sizeof(double));
    char* p_cnt = take((size_t)SSD_MAX_LEVELS * B * sizeof(int));
    if (w) {
        w->key = (float*)p_key; w->lse = (float*)p_lse; w->part_pos = (double*)p_pp; w->part_sl1 = (double*)p_pl;
        w->img_tau = (unsigned*)p_tau; w->img_mined = (int*)p_mined; w->img_P = (int*)p_P; w->img_N = (int*)p_N;
        w->img_sum = (double*)p_sum; w->img_count = (int*)p_cnt;
    }
    return off;
}

struct MbParams {
    size_t n, nblk;
    int A, B, C, ratio;
    float alpha, grad_scale;
};


struct MbLevels {                            // the rows form's geometry (levels == 0: dense form)
    int levels;
    int hw[SSD_MAX_LEVELS], n[SSD_MAX_LEVELS], npad[SSD_MAX_LEVELS], off[SSD_MAX_LEVELS + 1];
    __hip_bfloat16* rows[SSD_MAX_LEVELS];
    int* rop[SSD_MAX_LEVELS];
    int* por[SSD_MAX_LEVELS];
    int* count;                              // [SSD_MAX_LEVELS]
};

// the one predicate every kernel uses for "anchor is a mined negative of its image" (the anchor is not a positive)
__device__ __forceinline__ bool mined_neg(float key, float tau, int mined) { return mined != 0 && key >= tau; }

// ------------------------------------------------------------------------------------------------
// Pass 1: one read of conf (k_loss_rows' staging: persistent grid, the next block's logits requested before the current block
// is reduced).  Per anchor: logsumexp and the background CE; per block: the positives' CE and box-term sums.  A block of 128
// rows may straddle two images: nothing here is per image.
template <typename T, int CC, bool IOU>
__global__ __launch_bounds__(WG) void k_mb_rows(const T* __restrict__ conf, const T* __restrict__ loc,
                                                const int* __restrict__ cls, const float* __restrict__ gloc,
                                                const uint8_t* __restrict__ mask, size_t n, int C_rt, MbWs w, int A,
                                                BoxArgs bx) {
    extern __shared__ __attribute__((aligned(16))) float s_z[];   // [ROWS*C]
    __shared__ double s_red[4];
    const int C = CC ? CC : C_rt;
    const size_t nblk = (n + ROWS - 1) / ROWS;
    const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
    const int k0 = half ? (C + 1) / 2 : 0, k1 = half ? C : (C + 1) / 2;
    constexpr int FIXED = (CC + 1) / 2;                       // trip count of the longer half row
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
        __syncthreads();                                   // previous block's LDS reads are done
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
        double acc_pos = 0.0, acc_sl1 = 0.0;
        if (r < nrow) {
            const float* z = s_z + r * C;
            float m = -INFINITY;
            float s = 0.f;
            if constexpr (CC != 0) {
                float zz[FIXED];
#pragma unroll
                for (int j = 0; j < FIXED; ++j) zz[j] = k0 + j < k1 ? z[k0 + j] : -INFINITY;
#pragma unroll
                for (int j = 0; j < FIXED; ++j) m = fmaxf(m, zz[j]);
                m = fmaxf(m, __shfl_xor(m, 1));
#pragma unroll
                for (int j = 0; j < FIXED; ++j) s += k0 + j < k1 ? __expf(zz[j] - m) : 0.f;
            } else {
                for (int k = k0; k < k1; ++k) m = fmaxf(m, z[k]);
                m = fmaxf(m, __shfl_xor(m, 1));
                for (int k = k0; k < k1; ++k) s += __expf(z[k] - m);
            }
            s += __shfl_xor(s, 1);
            if (half == 0) {
                const size_t g = row0 + r;
                const float logs = __logf(s);
                const float lse = m + logs;
                w.key[g] = (m - z[C - 1]) + logs;             // >= 0 by construction
                w.lse[g] = lse;
                // a row that is not finite poisons the block's sum: status 3 is read off the sums (k_mb_scalars)
                if (!(fabsf(lse) < INFINITY)) acc_pos = (double)NAN;
                if (mask[g] != 0) {
                    acc_pos += (double)((m - z[cls[g]]) + logs);
                    const float4 gl = reinterpret_cast<const float4*>(gloc)[g];
                    if constexpr (IOU) {
                        float4 unused;
                        acc_sl1 = box_term<T>(bx, A, g, loc + 4 * g, gl, 1.f, &unused);
                    } else {
                        acc_sl1 = box_loss<T>(loc + 4 * g, gl);
                    }
                }
            }
        }
        const double bp = block_sum<4>(acc_pos, s_red);
        const double bl = block_sum<4>(acc_sl1, s_red);
        if (threadIdx.x == 0) { w.part_pos[blk] = bp; w.part_sl1[blk] = bl; }
    }
}

// ------------------------------------------------------------------------------------------------
// Pass 2: one workgroup per image.
// In `hist` (nb <= 2 * SWG bins, in LDS) scanned from the top, the bin holding the k-th largest key (k >= 1; -1 if there are
// fewer than k keys); *k_in_bin = rank of the target inside that bin (1-based).  Thread t owns the `per` bins below
// nb - 1 - t * per; a workgroup prefix sum finds the owner of rank k.
__device__ __forceinline__ int find_bin(const int* hist, int nb, int k, int* k_in_bin, int* s_scan, int* s_res) {
    const int per = (nb + SWG - 1) / SWG;                      // 1 or 2
    const int hi = nb - 1 - (int)threadIdx.x * per;
    int h[2];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int b = hi - j;
        h[j] = (j < per && b >= 0) ? hist[b] : 0;
        mine += h[j];
    }
    int incl = mine;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
    }
    __syncthreads();                                         // previous users of s_scan / s_res are done
    if (lane == 63) s_scan[wave] = incl;
    if (threadIdx.x == 0) { s_res[0] = -1; s_res[1] = 0; }
    __syncthreads();
    int base = 0;
    for (int k2 = 0; k2 < wave; ++k2) base += s_scan[k2];
    const int before = base + incl - mine;                   // keys in bins above mine
    if (before < k && k <= before + mine) {                  // exactly one thread
        int run = before, b = hi;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (run + h[j] >= k) { b = hi - j; break; }
            run += h[j];
        }
        s_res[0] = b; s_res[1] = k - run;
    }
    __syncthreads();
    *k_in_bin = s_res[1];
    return s_res[0];
}

__global__ __launch_bounds__(SWG) void k_mb_select(const uint8_t* __restrict__ mask, MbWs w, MbParams p, MbLevels h) {
    extern __shared__ __attribute__((aligned(16))) unsigned s_key[];   // [A] key bits; POS_KEY at positives
    __shared__ int s_hist[HB];
    __shared__ int s_scan[SWAVES];
    __shared__ int s_res[2];
    __shared__ int s_redi[SWAVES];
    __shared__ double s_redd[SWAVES];
    const int b = blockIdx.x, A = p.A;
    const int lane = threadIdx.x & 63;
    const size_t g0 = (size_t)b * A;
    int my_pos = 0;
    for (int i = threadIdx.x; i < A; i += SWG) {
        const bool pos = mask[g0 + i] != 0;
        unsigned kb = __float_as_uint(w.key[g0 + i]);
        if (kb == POS_KEY) kb = 0x7fc00000u;                  // (a NaN either way: `key >= tau` is false for both)
        s_key[i] = pos ? POS_KEY : kb;
        my_pos += pos ? 1 : 0;
    }
    const int P = block_sum_int<SWAVES>(my_pos, s_redi);      // (its barriers publish s_key)
    const long long want = (long long)p.ratio * P;
    int k = (int)(want < (long long)(A - P) ? want : (long long)(A - P));
    const int mined = k > 0 ? 1 : 0;
    unsigned prefix = 0;
    if (mined) {                                              // uniform over the workgroup
        // exact radix select of the k-th largest candidate key: digits of 11, 11 and 10 bits from the top
        for (int lvl = 0; lvl < 3; ++lvl) {
            const int bits = lvl == 2 ? 10 : 11;
            const int shift = lvl == 0 ? 21 : (lvl == 1 ? 10 : 0);
            const int nb = 1 << bits;
            __syncthreads();                                  // find_bin's reads of the previous histogram are done
            for (int i = threadIdx.x; i < nb; i += SWG) s_hist[i] = 0;
            __syncthreads();
            for (int i0 = 0; i0 < A; i0 += SWG) {
                const int i = i0 + (int)threadIdx.x;
                const unsigned kb = i < A ? s_key[i] : POS_KEY;
                const bool act = kb != POS_KEY && (lvl == 0 || (kb >> (shift + bits)) == prefix);
                const int digit = (int)((kb >> shift) & (unsigned)(nb - 1));
                // the keys of an image crowd into a few bins of the top digit: the lanes that share the first active lane's bin
                // are counted by one LDS atomic (same-address LDS atomics of a wave serialise), the others add one by one
                const unsigned long long am = __ballot(act);
                if (am != 0ull) {
                    const int leader = __ffsll((long long)am) - 1;
                    const int ld = __shfl(digit, leader);
                    const bool same = act && digit == ld;
                    const unsigned long long sm = __ballot(same);
                    if (lane == leader) atomicAdd(&s_hist[ld], (int)__popcll(sm));
                    if (act && !same) atomicAdd(&s_hist[digit], 1);
                }
            }
            __syncthreads();
            int kin;
            int bin = find_bin(s_hist, nb, k, &kin, s_scan, s_res);
            if (bin < 0) { bin = 0; kin = 1; }                // (only with NaN keys, i.e. status 3: stay in bounds)
            prefix = (prefix << bits) | (unsigned)bin;
            k = kin;
        }
    }
    const float tau = __uint_as_float(prefix);
    int cnt = 0;
    double sum = 0.0;
    for (int i = threadIdx.x; i < A; i += SWG) {
        const unsigned kb = s_key[i];
        const float key = __uint_as_float(kb);
        if (kb != POS_KEY && mined_neg(key, tau, mined)) { ++cnt; sum += (double)key; }
    }
    const int N = block_sum_int<SWAVES>(cnt, s_redi);
    sum = block_sum<SWAVES>(sum, s_redd);
    // ... and a slice of k_mb_rows' per-block sums, so that the workgroup that writes the scalars adds B values per term
    const size_t per = (p.nblk + p.B - 1) / p.B, i0 = (size_t)b * per, i1 = min(p.nblk, i0 + per);
    double pp = 0.0, pl = 0.0;
    for (size_t i = i0 + threadIdx.x; i < i1; i += SWG) { pp += w.part_pos[i]; pl += w.part_sl1[i]; }
    pp = block_sum<SWAVES>(pp, s_redd);
    pl = block_sum<SWAVES>(pl, s_redd);
    if (threadIdx.x == 0) {
        w.img_tau[b] = prefix; w.img_mined[b] = mined; w.img_P[b] = P; w.img_N[b] = N;
        w.img_sum[b] = sum; w.img_sum[p.B + b] = pp; w.img_sum[2 * p.B + b] = pl;
    }
    // rows form: pixels of every level that carry a gradient
    for (int l = 0; l < h.levels; ++l) {
        int c = 0;
        const int nl = h.n[l];
        for (int pix = threadIdx.x; pix < h.hw[l]; pix += SWG) {
            const unsigned* kk = s_key + h.off[l] + pix * nl;
            bool f = false;
            for (int a = 0; a < nl; ++a) f |= kk[a] == POS_KEY || mined_neg(__uint_as_float(kk[a]), tau, mined);
            c += f ? 1 : 0;
        }
        const int tot = block_sum_int<SWAVES>(c, s_redi);
        if (threadIdx.x == 0) w.img_count[l * p.B + b] = tot;
    }
}

// The per-image results, summed in a fixed order by a 256-thread workgroup.
struct MbTotals {
    int P;
    long long N;
    double pos, sl1, neg;
    unsigned tau_min_bits;
    int any_mined;
};

__device__ __forceinline__ int mb_total_pos(const MbWs& w, int B, int* s_redi) {
    int v = 0;
    for (int i = threadIdx.x; i < B; i += WG) v += w.img_P[i];
    return block_sum_int<4>(v, s_redi);
}

// out8 = loc, pos, neg, total, P, N, tau_min, status (0 ok; 1: P == 0; 3: a logit row or a positive's offset was not finite,
// which takes precedence).  Called by every thread of one 256-thread workgroup.
__device__ __forceinline__ void mb_scalars(const MbWs& w, const MbParams& p, int P, float* __restrict__ out, int* s_redi,
                                           double* s_redd) {
    double a = 0.0, bb = 0.0, c = 0.0;
    int nn = 0;
    unsigned tmin = 0xffffffffu;
    for (int i = threadIdx.x; i < p.B; i += WG) {
        c += w.img_sum[i]; a += w.img_sum[p.B + i]; bb += w.img_sum[2 * p.B + i];
        nn += w.img_N[i];
        if (w.img_mined[i]) tmin = min(tmin, w.img_tau[i]);   // (keys are >= 0: their bits order as the floats do)
    }
    a = block_sum<4>(a, s_redd);
    bb = block_sum<4>(bb, s_redd);
    c = block_sum<4>(c, s_redd);
    const int N = block_sum_int<4>(nn, s_redi);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tmin = min(tmin, (unsigned)__shfl_xor((int)tmin, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_redi[threadIdx.x >> 6] = (int)tmin;
    __syncthreads();
    if (threadIdx.x == 0) {
        tmin = min(min((unsigned)s_redi[0], (unsigned)s_redi[1]), min((unsigned)s_redi[2], (unsigned)s_redi[3]));
        const bool ok = P > 0;
        const double dp = (double)P;
        const float l_pos = ok ? (float)(a / dp) : 0.f;
        const float l_loc = ok ? (float)((double)p.alpha * bb / dp) : 0.f;
        const float l_neg = ok ? (float)(c / dp) : 0.f;
        out[0] = l_loc; out[1] = l_pos; out[2] = l_neg; out[3] = (l_loc + l_pos) + l_neg;
        out[4] = (float)P; out[5] = (float)N; out[6] = tmin == 0xffffffffu ? 0.f : __uint_as_float(tmin);
        const bool bad = !(fabs(a) < (double)INFINITY) || !(fabs(bb) < (double)INFINITY) || !(fabs(c) < (double)INFINITY);
        out[7] = bad ? 3.f : (ok ? 0.f : 1.f);
    }
}

// Pass 3, dense form: gradients, written once and coalesced.  Only selected rows re-read their logits.
template <typename T, bool IOU>
__global__ __launch_bounds__(WG) void k_mb_grad(const T* __restrict__ conf, const T* __restrict__ loc,
                                                const int* __restrict__ cls, const float* __restrict__ gloc,
                                                const uint8_t* __restrict__ mask, MbParams p, T* __restrict__ dconf,
                                                T* __restrict__ dloc, MbWs w, float* __restrict__ out, BoxArgs bx) {
    extern __shared__ __attribute__((aligned(16))) float s_g[];   // [ROWS*C] gradient block
    __shared__ int s_redi[4];
    __shared__ double s_redd[4];
    const int C = p.C;
    const size_t row0 = (size_t)blockIdx.x * ROWS;
    const int nrow = (int)min((size_t)ROWS, p.n - row0);
    const int P = mb_total_pos(w, p.B, s_redi);
    const float sc = P > 0 ? p.grad_scale / (float)P : 0.f;
    const float sl = box_scale(p.grad_scale, p.alpha, P);

    for (int i = threadIdx.x; i < (ROWS * C + 3) / 4; i += WG)
        reinterpret_cast<float4*>(s_g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
    if (r < nrow) {
        const size_t g = row0 + r;
        const int b = (int)(g / (size_t)p.A);
        const bool pos = mask[g] != 0;
        const bool neg = !pos && mined_neg(w.key[g], __uint_as_float(w.img_tau[b]), w.img_mined[b]);
        if (pos || neg) {
            const float lse = w.lse[g];
            const int label = pos ? cls[g] : C - 1;
            const T* z = conf + g * C;
            float* o = s_g + r * C;
            const int k0 = half ? (C + 1) / 2 : 0, k1 = half ? C : (C + 1) / 2;
            for (int k = k0; k < k1; ++k) o[k] = (__expf(to_f32<T>(z[k]) - lse) - (k == label ? 1.f : 0.f)) * sc;
        }
        if (half == 0) {
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pos) {
                if constexpr (IOU) box_term<T>(bx, p.A, g, loc + 4 * g, reinterpret_cast<const float4*>(gloc)[g], sl, &d);
                else d = box_grad<T>(loc + 4 * g, reinterpret_cast<const float4*>(gloc)[g], sl);
            }
            T* o = dloc + 4 * g;
            o[0] = from_f32<T>(d.x); o[1] = from_f32<T>(d.y); o[2] = from_f32<T>(d.z); o[3] = from_f32<T>(d.w);
        }
    }
    __syncthreads();
    store_block<T>(dconf + row0 * C, s_g, (size_t)nrow * C);   // coalesced store of the gradient block
    if (blockIdx.x == 0) mb_scalars(w, p, P, out, s_redi, s_redd);
}

// ------------------------------------------------------------------------------------------------
// Rows form (ssd_multibox_loss_fwd_bwd_heads): the structure of loss.hip's k_hg_assign / k_loss_grad_rows with the per-image
// selection; k_mb_select has counted the pixels.
__device__ __forceinline__ bool mb_pixel_flag(const MbLevels& h, const uint8_t* __restrict__ mask, const MbWs& w, int A, int l,
                                              int b, int pix, float tau, int mined) {
    const size_t g0 = (size_t)b * A + h.off[l] + (size_t)pix * h.n[l];
    bool f = false;
    for (int a = 0; a < h.n[l]; ++a) f |= mask[g0 + a] != 0 || mined_neg(w.key[g0 + a], tau, mined);
    return f;
}

__global__ __launch_bounds__(WG) void k_mb_assign(const uint8_t* __restrict__ mask, MbWs w, MbParams p, MbLevels h,
                                                  float* __restrict__ out) {
    __shared__ int s_redi[4];
    __shared__ int s_wave[4];
    __shared__ double s_redd[4];
    const int b = blockIdx.x, l = blockIdx.y;
    const float tau = __uint_as_float(w.img_tau[b]);
    const int mined = w.img_mined[b];
    int before = 0;
    for (int i = threadIdx.x; i < b; i += WG) before += w.img_count[l * p.B + i];
    int base = block_sum_int<4>(before, s_redi);              // rows of this level in the images before this one
    const int hw = h.hw[l], npad = h.npad[l];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int p0 = 0; p0 < hw; p0 += WG) {
        const int pix = p0 + threadIdx.x;
        const bool f = pix < hw && mb_pixel_flag(h, mask, w, p.A, l, b, pix, tau, mined);
        const unsigned long long bal = __ballot(f);
        __syncthreads();                                     // previous chunk's s_wave reads are done
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int prefix = __popcll(bal & ((1ull << lane) - 1ull));
        for (int k = 0; k < wave; ++k) prefix += s_wave[k];
        const int chunk_total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        if (pix < hw) {
            const int flat = b * hw + pix;
            const int row = f ? base + prefix : -1;
            h.rop[l][flat] = row;
            if (f) {
                h.por[l][row] = flat;
                uint4* dst = reinterpret_cast<uint4*>(h.rows[l] + (size_t)row * npad);
                for (int k = 0; k < npad / 8; ++k) dst[k] = make_uint4(0, 0, 0, 0);
            }
        }
        base += chunk_total;
    }
    if (b == p.B - 1 && threadIdx.x == 0) h.count[l] = base;
    if (b == 0 && l == 0) {
        const int P = mb_total_pos(w, p.B, s_redi);
        mb_scalars(w, p, P, out, s_redi, s_redd);
    }
}

// Gradient of the selected anchors only, written into the compact rows (the arithmetic of k_mb_grad).
template <bool IOU>
__global__ __launch_bounds__(WG) void k_mb_grad_rows(const __hip_bfloat16* __restrict__ conf, const __hip_bfloat16* __restrict__ loc,
                                                     const int* __restrict__ cls, const float* __restrict__ gloc,
                                                     const uint8_t* __restrict__ mask, MbParams p, MbWs w, MbLevels h,
                                                     BoxArgs bx) {
    typedef __hip_bfloat16 T;
    __shared__ int s_redi[4];
    const int C = p.C;
    const size_t row0 = (size_t)blockIdx.x * ROWS;
    const int nrow = (int)min((size_t)ROWS, p.n - row0);
    const int P = mb_total_pos(w, p.B, s_redi);
    const float sc = P > 0 ? p.grad_scale / (float)P : 0.f;
    const float sl = box_scale(p.grad_scale, p.alpha, P);
    const int r = threadIdx.x >> 1, half = threadIdx.x & 1;
    if (r < nrow) {
        const size_t g = row0 + r;
        const int b = (int)(g / (size_t)p.A);
        const int a = (int)(g - (size_t)b * p.A);
        const bool pos = mask[g] != 0;
        const bool neg = !pos && mined_neg(w.key[g], __uint_as_float(w.img_tau[b]), w.img_mined[b]);
        if (pos || neg) {
            int l = 0;
            for (int k = 1; k < h.levels; ++k) l += a >= h.off[k] ? 1 : 0;
            const int idx = a - h.off[l];
            const int pix = idx / h.n[l], slot = idx - pix * h.n[l];
            const int row = h.rop[l][b * h.hw[l] + pix];
            if (row >= 0) {
                T* d = h.rows[l] + (size_t)row * h.npad[l];
                const float lse = w.lse[g];
                const int label = pos ? cls[g] : C - 1;
                const T* z = conf + g * C;
                T* o = d + h.n[l] * 4 + slot * C;
                const int k0 = half ? (C + 1) / 2 : 0, k1 = half ? C : (C + 1) / 2;
                for (int k = k0; k < k1; ++k) o[k] = from_f32<T>((__expf(to_f32<T>(z[k]) - lse) - (k == label ? 1.f : 0.f)) * sc);
                if (pos && half == 0) {
                    float4 dl;
                    if constexpr (IOU) box_term<T>(bx, p.A, g, loc + 4 * g, reinterpret_cast<const float4*>(gloc)[g], sl, &dl);
                    else dl = box_grad<T>(loc + 4 * g, reinterpret_cast<const float4*>(gloc)[g], sl);
                    T* ol = d + slot * 4;
                    ol[0] = from_f32<T>(dl.x); ol[1] = from_f32<T>(dl.y); ol[2] = from_f32<T>(dl.z); ol[3] = from_f32<T>(dl.w);
                }
            }
        }
    }
}

// More than 64 KB of dynamic LDS is registered once per device and kernel, for the largest block the bounds admit.
template <typename K>
int register_lds(OnceLds& once, K kern, size_t lds, size_t most) {
    return lds <= 64 * 1024 ? 0 : ensure_lds(once, reinterpret_cast<const void*>(kern), (int)most);
}

// the launches both forms share: conf read once, the per-image select
template <typename T, bool IOU>
int launch_rows_select(const void* conf, const void* loc, const int32_t* cls, const float* gloc, const uint8_t* mask,
                       const MbParams& p, const BoxArgs& bx, const MbLevels& h, MbWs w, hipStream_t s) {
    const size_t lds = rows_lds_bytes(p.C);
    const size_t most = (LDS_LIMIT - 64) / 16 * 16;
    const unsigned pgrid = (unsigned)min((size_t)MAX_PERSIST, p.nblk);
    static OnceLds once81, once0, once_sel;
    if (p.C == 81 ? register_lds(once81, k_mb_rows<T, 81, IOU>, lds, most) : register_lds(once0, k_mb_rows<T, 0, IOU>, lds, most)) return SSD_ERR_LAUNCH;
    const size_t slds = select_lds_bytes(p.A);
    if (register_lds(once_sel, k_mb_select, slds, select_lds_bytes(SSD_MULTIBOX_MAX_ANCHORS))) return SSD_ERR_LAUNCH;
    if (p.C == 81)
        hipLaunchKernelGGL((k_mb_rows<T, 81, IOU>), dim3(pgrid), dim3(WG), lds, s, (const T*)conf, (const T*)loc, cls, gloc, mask,
                           p.n, p.C, w, p.A, bx);
    else
        hipLaunchKernelGGL((k_mb_rows<T, 0, IOU>), dim3(pgrid), dim3(WG), lds, s, (const T*)conf, (const T*)loc, cls, gloc, mask,
                           p.n, p.C, w, p.A, bx);
    hipLaunchKernelGGL(k_mb_select, dim3(p.B), dim3(SWG), slds, s, mask, w, p, h);
    return 0;
}

template <typename T, bool IOU>
int launch_dense(const void* conf, const void* loc, const int32_t* cls, const float* gloc, const uint8_t* mask,
                 const MbParams& p, const BoxArgs& bx, float* out, void* dconf, void* dloc, MbWs w, hipStream_t s) {
    const size_t lds = rows_lds_bytes(p.C);
    static OnceLds once_grad;
    if (register_lds(once_grad, k_mb_grad<T, IOU>, lds, (LDS_LIMIT - 64) / 16 * 16)) return SSD_ERR_LAUNCH;
    MbLevels h = {};
    if (int rc = launch_rows_select<T, IOU>(conf, loc, cls, gloc, mask, p, bx, h, w, s)) return rc;
    hipLaunchKernelGGL((k_mb_grad<T, IOU>), dim3((unsigned)p.nblk), dim3(WG), lds, s, (const T*)conf, (const T*)loc, cls, gloc,
                       mask, p, (T*)dconf, (T*)dloc, w, out, bx);
    return ssd_launch_status();
}

// the refusals both entries share, before any launch
int mb_check(const void* conf, const void* loc, const int32_t* cls, const float* gloc, const uint8_t* mask, int B, int A,
             int C, int ratio, float alpha, float grad_scale, const float* out8, int box_kind, const double* priors, MbParams* p, BoxArgs* bx) {
    if (box_kind < SSD_BOX_SMOOTH_L1 || box_kind > SSD_BOX_CIOU || (box_kind != SSD_BOX_SMOOTH_L1 && !priors)) return SSD_ERR_VALUE;
    if (B <= 0 || A <= 0 || C < 2 || ratio < 1) return SSD_ERR_VALUE;
    if (!(alpha >= 0.f) || !(alpha < INFINITY) || !std::isfinite(grad_scale)) return SSD_ERR_VALUE;
    if (!conf || !loc || !cls || !gloc || !mask || !out8) return SSD_ERR_VALUE;
    if (C > SSD_LOSS_MAX_CLASSES || A > SSD_MULTIBOX_MAX_ANCHORS) return SSD_ERR_UNSUPPORTED;
    p->n = (size_t)B * A; p->nblk = (p->n + ROWS - 1) / ROWS;
    p->A = A; p->B = B; p->C = C; p->ratio = ratio; p->alpha = alpha; p->grad_scale = grad_scale;
    bx->kind = box_kind; bx->priors = priors;
    return 0;
}

}  // namespace

extern "C" {

int ssd_multibox_loss_max_anchors(void) { return SSD_MULTIBOX_MAX_ANCHORS; }

size_t ssd_multibox_loss_workspace_bytes(int B, int A, int C) {
    if (B <= 0 || A <= 0 || C <= 0) return 0;
    return mb_ws_layout((size_t)B, (size_t)A, nullptr, nullptr);
}

size_t ssd_multibox_loss_heads_workspace_bytes(int B, int A, int C) { return ssd_multibox_loss_workspace_bytes(B, A, C); }

int ssd_multibox_loss_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                              const uint8_t* gt_mask, int B, int A, int C, int neg_pos_ratio, float loc_weight,
                              float grad_scale, float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes,
                              void* stream) {
    return ssd_multibox_loss_box_fwd_bwd(conf, loc, dtype, gt_cls, gt_loc, gt_mask, B, A, C, neg_pos_ratio, loc_weight, grad_scale,
                                         out8, dconf, dloc, ws, ws_bytes, stream, SSD_BOX_SMOOTH_L1, nullptr);
}

int ssd_multibox_loss_box_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                  const uint8_t* gt_mask, int B, int A, int C, int neg_pos_ratio, float loc_weight,
                                  float grad_scale, float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes,
                                  void* stream, int box_kind, const double* priors) {
    MbParams p;
    BoxArgs bx;
    if (dtype != SSD_F32 && dtype != SSD_BF16) return SSD_ERR_VALUE;
    if (int rc = mb_check(conf, loc, gt_cls, gt_loc, gt_mask, B, A, C, neg_pos_ratio, loc_weight, grad_scale, out8, box_kind, priors, &p, &bx)) return rc;
    if (!dconf || !dloc) return SSD_ERR_VALUE;
    if (!ws || ws_bytes < mb_ws_layout((size_t)B, (size_t)A, nullptr, nullptr)) return SSD_ERR_WORKSPACE;
    MbWs w;
    mb_ws_layout((size_t)B, (size_t)A, static_cast<char*>(ws), &w);
    hipStream_t s = (hipStream_t)stream;
    const bool iou = box_kind != SSD_BOX_SMOOTH_L1;
    if (dtype == SSD_F32)
        return iou ? launch_dense<float, true>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, out8, dconf, dloc, w, s)
                   : launch_dense<float, false>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, out8, dconf, dloc, w, s);
    return iou ? launch_dense<__hip_bfloat16, true>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, out8, dconf, dloc, w, s)
               : launch_dense<__hip_bfloat16, false>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, out8, dconf, dloc, w, s);
}

int ssd_multibox_loss_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                    const uint8_t* gt_mask, int B, int A, int C, int neg_pos_ratio, float loc_weight,
                                    float grad_scale, float* out8, const ssd_head_grads* hg, void* ws, size_t ws_bytes,
                                    void* stream) {
    return ssd_multibox_loss_box_fwd_bwd_heads(conf, loc, dtype, gt_cls, gt_loc, gt_mask, B, A, C, neg_pos_ratio, loc_weight,
                                               grad_scale, out8, hg, ws, ws_bytes, stream, SSD_BOX_SMOOTH_L1, nullptr);
}

int ssd_multibox_loss_box_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                        const uint8_t* gt_mask, int B, int A, int C, int neg_pos_ratio, float loc_weight,
                                        float grad_scale, float* out8, const ssd_head_grads* hg, void* ws, size_t ws_bytes,
                                        void* stream, int box_kind, const double* priors) {
    MbParams p;
    BoxArgs bx;
    if (dtype != SSD_F32 && dtype != SSD_BF16) return SSD_ERR_VALUE;
    if (int rc = mb_check(conf, loc, gt_cls, gt_loc, gt_mask, B, A, C, neg_pos_ratio, loc_weight, grad_scale, out8, box_kind, priors, &p, &bx)) return rc;
    if (dtype != SSD_BF16) return SSD_ERR_UNSUPPORTED;
    if (!hg || !hg->count || hg->levels <= 0 || hg->levels > SSD_MAX_LEVELS) return SSD_ERR_VALUE;
    MbLevels h = {};
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
    if (off != A) return SSD_ERR_ASSERT;                          // the levels tile the anchors, as in ssd_loss_fwd_bwd_heads
    h.count = hg->count;
    if (!ws || ws_bytes < mb_ws_layout((size_t)B, (size_t)A, nullptr, nullptr)) return SSD_ERR_WORKSPACE;
    MbWs w;
    mb_ws_layout((size_t)B, (size_t)A, static_cast<char*>(ws), &w);
    hipStream_t s = (hipStream_t)stream;
    typedef __hip_bfloat16 T;
    const bool iou = box_kind != SSD_BOX_SMOOTH_L1;
    if (int rc = iou ? launch_rows_select<T, true>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, h, w, s)
                     : launch_rows_select<T, false>(conf, loc, gt_cls, gt_loc, gt_mask, p, bx, h, w, s)) return rc;
    hipLaunchKernelGGL(k_mb_assign, dim3(B, hg->levels), dim3(WG), 0, s, gt_mask, w, p, h, out8);
    if (iou)
        hipLaunchKernelGGL(k_mb_grad_rows<true>, dim3((unsigned)p.nblk), dim3(WG), 0, s, (const T*)conf, (const T*)loc, gt_cls,
                           gt_loc, gt_mask, p, w, h, bx);
    else
        hipLaunchKernelGGL(k_mb_grad_rows<false>, dim3((unsigned)p.nblk), dim3(WG), 0, s, (const T*)conf, (const T*)loc, gt_cls,
                           gt_loc, gt_mask, p, w, h, bx);
    return ssd_launch_status();
}

}  // extern "C"
