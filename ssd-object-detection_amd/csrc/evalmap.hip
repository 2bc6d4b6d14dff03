// Evaluation metric on the device for gfx950 (MI355X): the last stage behind k_score_decode + k_nms (detect.hip).
//
//   k_eval_match  per image: the kept anchors ordered by (score desc, anchor asc), cut to the first max_dets -- the order
//                 utils/metrics.coco_map gets from its stable sort of the anchor-ordered kept list -- then, per class and per
//                 IoU threshold, coco_map's greedy pass: detections in that order, each claims the still-unclaimed ground truth
//                 of its class with the highest IoU >= threshold, the LAST index winning among equal IoUs.  One workgroup per
//                 image: candidate list (LDS atomics), exact radix cut when more than CAP anchors are kept, rank sort of 64-bit
//                 keys (~score | anchor), rank sort by (class, rank) for the class segments, then one THREAD per (class
//                 segment, threshold) walks its segment.  With at most GL ground truths in the image (nearly always) every
//                 class-matched IoU is computed once, by all threads, into an LDS matrix and the claimed set is a register
//                 mask; with more, the walking thread computes IoUs as it goes and finds claimed boxes in the per-detection
//                 match list -- slower, no bound on the number of ground truths.
//   k_eval_ap     per class: 101-point AP at the ten thresholds from the flags sorted by (class, score desc, image, rank).
//                 The segment is scanned in chunks of one element per thread (ballot prefix counts of the ten flag bits, one
//                 load serves all thresholds).  Only true positives can raise the right-to-left precision envelope, so each
//                 contributes precision = ctp / (i + 1) to the LAST recall point <= its recall (LDS 64-bit max on the bits of a
//                 non-negative double); a suffix maximum over the 101 buckets is the sampled envelope.
//   (k_eval_match_coco / k_eval_ap_coco: COCO's twelve metrics; k_eval_match_voc / k_eval_ap_voc: PASCAL VOC's AP -- further down)
// IoU is utils/metrics.iou_matrix operation for operation in float64.  Compile with -ffp-contract=off.
#include "common.h"
#include <float.h>
#include <limits.h>

namespace {

constexpr int WG = 1024;                     // one key per thread in the rank sort
constexpr int CAP = 1024;                    // kept anchors that are sorted in LDS without the radix cut (k_nms keeps <= 1024)
constexpr int MAXD = 128;                    // ssd_eval_max_dets()
constexpr int GL = 48;                       // ground truths per image whose IoUs are cached in LDS
constexpr int NT = 10;                       // IoU thresholds
constexpr int NP = 101;                      // recall points

struct Thresholds { double v[NT]; };
struct RecallPoints { double v[NP]; };

// float bits -> unsigned, order preserving (-0 ordered as +0: numpy compares them equal)
__device__ __forceinline__ unsigned ordered_bits(float s) {
    const unsigned u = __float_as_uint(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix of a 0/1 flag over the workgroup (index order), and the total
__device__ __forceinline__ int wg_prefix(bool flag, int* s_wave, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) {
        if (w < wave) base += s_wave[w];
        total += s_wave[w];
    }
    return base + before;
}

// metrics.iou_matrix for one pair: detection (cx, cy, w, h) float32 widened exactly, ground truth float64
__device__ __forceinline__ double iou_f64(float4 d, double gx, double gy, double gw, double gh) {
    const double dx = (double)d.x, dy = (double)d.y, dw = (double)d.z, dh = (double)d.w;
    const double a0 = dx - dw / 2, a1 = dy - dh / 2, a2 = dx + dw / 2, a3 = dy + dh / 2;
    const double b0 = gx - gw / 2, b1 = gy - gh / 2, b2 = gx + gw / 2, b3 = gy + gh / 2;
    const double w = fmax(fmin(a2, b2) - fmax(a0, b0), 0.0);
    const double h = fmax(fmin(a3, b3) - fmax(a1, b1), 0.0);
    const double inter = w * h;
    const double area_a = (a2 - a0) * (a3 - a1);
    const double area_b = (b2 - b0) * (b3 - b1);
    const double uni = area_a + area_b - inter;
    return uni > 0.0 ? inter / fmax(uni, 1e-300) : 0.0;
}

// The selection stage of every matching kernel: the image's kept anchors ordered by (score desc, anchor asc), cut to the
// first max_dets.  Candidate list (LDS atomics), exact radix cut when more than CAP anchors are kept, rank sort of 64-bit keys
// (~score | anchor).  s_key [CAP] and s_idx [CAP] are scratch, dead on return; s_danchor[r] receives the anchor of rank r.
// Returns the number of detections; ends on a barrier.
__device__ __forceinline__ int select_ranked(const float* __restrict__ sc, const uint8_t* __restrict__ kp, int A, int max_dets,
                                             unsigned long long* s_key, int* s_idx, int* s_hist, int* s_wave, int* s_misc,
                                             int* s_danchor) {
    const int tid = threadIdx.x;
    if (tid < 4) s_misc[tid] = 0;
    __syncthreads();
    // the kept anchors, unordered (the sort orders them completely: the anchor index is part of the key)
    auto note = [&](int a) {
        const int slot = atomicAdd(&s_misc[0], 1);
        if (slot < CAP) s_idx[slot] = a;
    };
    if ((A & 3) == 0) {                          // rows of keep are 4-byte aligned: four anchors per load
        const unsigned* kp4 = reinterpret_cast<const unsigned*>(kp);
        const int nq = A >> 2;
        for (int q = tid; q < nq; q += WG) {
            const unsigned v = kp4[q];
            if (!v) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((v >> (8 * e)) & 0xffu) note(4 * q + e);
        }
    } else {
        for (int a = tid; a < A; a += WG)
            if (kp[a]) note(a);
    }
    __syncthreads();
    const int total = s_misc[0];
    int n_in;                                    // keys that enter the sort
    if (total <= CAP) {
        n_in = total;
        if (tid < total) {
            const int a = s_idx[tid];
            s_key[tid] = ((unsigned long long)(~ordered_bits(sc[a])) << 32) | (unsigned long long)(unsigned)a;
        }
    } else {
        // more kept anchors than sort slots (not what k_nms produces): exact cut to the max_dets best by radix select on the
        // ordered score bits, then their ordered compaction -- k_nms's cut
        unsigned prefix = 0;
        int k = max_dets;                        // rank (1-based, from the top) still to locate
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            for (int a = tid; a < A; a += WG)
                if (kp[a]) {
                    const unsigned key = ordered_bits(sc[a]);
                    if (shift == 24 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
                }
            __syncthreads();
            if (tid == 0) {
                int run = 0, d = 255;
                for (; d > 0; --d) {
                    if (run + s_hist[d] >= k) break;
                    run += s_hist[d];
                }
                s_misc[1] = d;
                s_misc[2] = k - run;
            }
            __syncthreads();
            prefix = (prefix << 8) | (unsigned)s_misc[1];
            k = s_misc[2];
            __syncthreads();
        }
        const unsigned cut_bits = prefix;        // take score > cut, and the first `k` (anchor order) with score == cut
        int filled = 0, eq_seen = 0;
        for (int a0 = 0; a0 < A; a0 += WG) {
            const int a = a0 + tid;
            bool is_c = a < A && kp[a];
            const unsigned key = is_c ? ordered_bits(sc[a]) : 0u;
            const bool is_eq = is_c && key == cut_bits;
            is_c = is_c && key >= cut_bits;
            int tot_eq = 0;
            const int eq_rank = wg_prefix(is_eq, s_wave, tot_eq);
            if (is_eq && eq_seen + eq_rank >= k) is_c = false;
            eq_seen += tot_eq;
            int tot = 0;
            const int pos = wg_prefix(is_c, s_wave, tot);
            if (is_c && filled + pos < CAP)
                s_key[filled + pos] = ((unsigned long long)(~key) << 32) | (unsigned long long)(unsigned)a;
            filled += tot;
        }
        n_in = min(filled, max_dets);            // == max_dets
    }
    __syncthreads();
    // sort by rank: keys are unique, every thread counts the keys below its own (broadcast LDS reads)
    const int nd = min(n_in, max_dets);
    {
        const unsigned long long mine = tid < n_in ? s_key[tid] : ~0ull;
        int rank = 0;
        for (int j = 0; j < n_in; ++j) rank += s_key[j] < mine ? 1 : 0;
        if (tid < n_in && rank < nd) s_danchor[rank] = (int)(unsigned)(mine & 0xffffffffull);
    }
    __syncthreads();                             // s_key / s_idx are dead from here on
    return nd;
}

__global__ __launch_bounds__(WG) void k_eval_match(const float* __restrict__ score, const int* __restrict__ cls,
                                                   const float4* __restrict__ box, const uint8_t* __restrict__ keep, int A,
                                                   const int* __restrict__ gt_cls, const double* __restrict__ gt_box,
                                                   const int* __restrict__ gt_off, Thresholds thr, int max_dets,
                                                   int* __restrict__ n_det, float* __restrict__ det_score,
                                                   int* __restrict__ det_cls, float4* __restrict__ det_box,
                                                   uint16_t* __restrict__ det_flags) {
    // s_big: the sort keys [CAP] u64 + the candidate list [CAP] int during the selection, the IoU matrix [MAXD][GL] afterwards
    __shared__ __attribute__((aligned(16))) double s_big[MAXD * GL];
    __shared__ float4 s_dbox[MAXD];
    __shared__ int s_dcls[MAXD];
    __shared__ int s_danchor[MAXD];
    __shared__ unsigned s_flags[MAXD];
    __shared__ int s_ord[MAXD];                  // detection ranks ordered by (class, rank)
    __shared__ int s_seg[MAXD];                  // first position in s_ord of every class segment (any order)
    __shared__ int s_match[NT][MAXD];            // uncached mode: ground truth claimed by the detection at a position, -1 none
    __shared__ double s_gbox[GL][4];
    __shared__ int s_gcls[GL];
    __shared__ int s_hist[256];
    __shared__ int s_wave[WG / 64];
    __shared__ int s_misc[4];
    static_assert(sizeof(double) * MAXD * GL >= CAP * (sizeof(unsigned long long) + sizeof(int)), "keys + list fit");
    unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_big);
    int* s_idx = reinterpret_cast<int*>(s_key + CAP);

    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t off = (size_t)b * A;
    const float* sc = score + off;
    const uint8_t* kp = keep + off;

    if (tid < MAXD) s_flags[tid] = 0u;
    const int nd = select_ranked(sc, kp, A, max_dets, s_key, s_idx, s_hist, s_wave, s_misc, s_danchor);
    // the detections: outputs fully written (slots at or beyond nd: score 0, class -1, box 0)
    if (tid < max_dets) {
        const size_t o = (size_t)b * max_dets + tid;
        float s = 0.f;
        int c = -1;
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < nd) {
            const int a = s_danchor[tid];
            s = sc[a];
            c = cls[off + a];
            bx = box[off + a];
            s_dcls[tid] = c;
            s_dbox[tid] = bx;
        }
        det_score[o] = s;
        det_cls[o] = c;
        det_box[o] = bx;
    }
    if (tid == 0) n_det[b] = nd;
    __syncthreads();
    // class segments: position of a detection among those ordered by (class, rank)
    if (tid < nd) {
        const int c = s_dcls[tid];
        int pos = 0;
        for (int r = 0; r < nd; ++r) {
            const int cr = s_dcls[r];
            pos += (cr < c || (cr == c && r < tid)) ? 1 : 0;
        }
        s_ord[pos] = tid;
    }
    __syncthreads();
    if (tid < nd) {
        const bool start = tid == 0 || s_dcls[s_ord[tid]] != s_dcls[s_ord[tid - 1]];
        if (start) s_seg[atomicAdd(&s_misc[3], 1)] = tid;
    }
    const int g0 = gt_off[b];
    const int G = max(gt_off[b + 1] - g0, 0);
    const bool cached = G <= GL;
    double* s_iou = s_big;
    if (cached) {
        if (tid < G) {
            s_gcls[tid] = gt_cls[g0 + tid];
#pragma unroll
            for (int e = 0; e < 4; ++e) s_gbox[tid][e] = gt_box[4 * (size_t)(g0 + tid) + e];
        }
        __syncthreads();
        // every class-matched IoU once
        for (int p = tid; p < nd * G; p += WG) {
            const int r = p / G, j = p - r * G;
            if (s_gcls[j] == s_dcls[r])
                s_iou[r * GL + j] = iou_f64(s_dbox[r], s_gbox[j][0], s_gbox[j][1], s_gbox[j][2], s_gbox[j][3]);
        }
    }
    __syncthreads();
    const int nseg = s_misc[3];
    // the greedy pass: one thread per (class segment, threshold)
    if (nd > 0 && G > 0) {
        for (int w = tid; w < nseg * NT; w += WG) {
            const int sg = w / NT, t = w - sg * NT;
            const int p0 = s_seg[sg];
            const int c = s_dcls[s_ord[p0]];
            const double th = thr.v[t];
            if (cached) {
                unsigned long long mine = 0ull;      // ground truths of this class
                for (int j = 0; j < G; ++j) mine |= (s_gcls[j] == c) ? (1ull << j) : 0ull;
                if (!mine) continue;
                unsigned long long taken = 0ull;
                for (int p = p0; p < nd; ++p) {
                    const int r = s_ord[p];
                    if (s_dcls[r] != c) break;
                    double best = th;
                    int bj = -1;
                    unsigned long long open = mine & ~taken;
                    while (open) {                   // ascending j, >=: the last index wins among equal IoUs
                        const int j = __ffsll((long long)open) - 1;
                        open &= open - 1ull;
                        const double v = s_iou[r * GL + j];
                        if (v >= best) { best = v; bj = j; }
                    }
                    if (bj >= 0) {
                        taken |= 1ull << bj;
                        atomicOr(&s_flags[r], 1u << t);
                    }
                }
            } else {
                for (int p = p0; p < nd; ++p) {
                    const int r = s_ord[p];
                    if (s_dcls[r] != c) break;
                    const float4 d = s_dbox[r];
                    double best = th;
                    int bj = -1;
                    for (int j = 0; j < G; ++j) {
                        if (gt_cls[g0 + j] != c) continue;
                        const double* g = gt_box + 4 * (size_t)(g0 + j);
                        const double v = iou_f64(d, g[0], g[1], g[2], g[3]);
                        if (!(v >= best)) continue;
                        bool taken = false;          // claimed by an earlier detection of the segment?
                        for (int q = p0; q < p && !taken; ++q) taken = s_match[t][q] == j;
                        if (!taken) { best = v; bj = j; }
                    }
                    s_match[t][p] = bj;
                    if (bj >= 0) atomicOr(&s_flags[r], 1u << t);
                }
            }
        }
    }
    __syncthreads();
    if (tid < max_dets) det_flags[(size_t)b * max_dets + tid] = tid < nd ? (uint16_t)s_flags[tid] : (uint16_t)0;
}

// AP of one class at the ten thresholds.  flags: every detection of the data set, sorted; seg_off[c] .. seg_off[c+1] the class's
// rows.  Any segment length: chunks of one element per thread, running counts carried in registers.
constexpr int AWG = 256;                    // four waves: ten running counts per thread and the wave totals stay in registers
__global__ __launch_bounds__(AWG) void k_eval_ap(const uint16_t* __restrict__ flags, const int* __restrict__ seg_off,
                                                const int* __restrict__ n_gt, RecallPoints pts, double* __restrict__ ap) {
    __shared__ unsigned long long s_best[NT][NP];    // bits of the best precision whose last recall point <= recall is k
    __shared__ double s_pts[NP];
    __shared__ int s_wtot[2][AWG / 64][NT];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ngt = n_gt[c];
    if (ngt <= 0) {                                  // not part of any mean (the caller excludes it)
        if (tid < NT) ap[(size_t)c * NT + tid] = 0.0;
        return;
    }
    for (int i = tid; i < NT * NP; i += AWG) (&s_best[0][0])[i] = 0ull;
    if (tid == 0) {                                  // constant indices: a lane-indexed read would copy the argument to scratch
#pragma unroll
        for (int k = 0; k < NP; ++k) s_pts[k] = pts.v[k];
    }
    const long long lo = seg_off[c], hi = seg_off[c + 1];
    const double dngt = (double)ngt;
    int carry[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) carry[t] = 0;
    __syncthreads();
    int par = 0;
    for (long long i0 = lo; i0 < hi; i0 += AWG, par ^= 1) {
        const long long i = i0 + tid;
        const unsigned f = i < hi ? (unsigned)flags[i] : 0u;
        int incl[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const unsigned long long m = __ballot((f >> t) & 1u);
            incl[t] = __popcll(m & ((2ull << lane) - 1ull));
            if (lane == 0) s_wtot[par][wave][t] = __popcll(m);
        }
        __syncthreads();                             // (double-buffered totals: one barrier per chunk)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int base = carry[t], tot = 0;
#pragma unroll
            for (int w = 0; w < AWG / 64; ++w) {
                const int v = s_wtot[par][w][t];
                if (w < wave) base += v;
                tot += v;
            }
            carry[t] += tot;
            if ((f >> t) & 1u) {
                const int ctp = base + incl[t];
                const double prec = (double)ctp / (double)(i - lo + 1);
                const double rec = (double)ctp / dngt;
                int a = 0, z = NP - 1;               // last k with pts[k] <= rec (pts[0] = 0 <= rec)
                while (a < z) {
                    const int mid = (a + z + 1) >> 1;
                    if (s_pts[mid] <= rec) a = mid; else z = mid - 1;
                }
                atomicMax(&s_best[t][a], (unsigned long long)__double_as_longlong(prec));
            }
        }
    }
    __syncthreads();
    if (tid < NT) {
        // sampled envelope = suffix maximum over the buckets; mean of the 101 samples summed in numpy's order (pairwise
        // summation of a block below 128 elements: eight running sums, combined as a tree, then the remainder in order)
        unsigned long long* row = s_best[tid];
        unsigned long long run = 0ull;
        for (int k = NP - 1; k >= 0; --k) {
            run = row[k] > run ? row[k] : run;
            row[k] = run;
        }
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = __longlong_as_double((long long)row[j]);
        int k = 8;
        for (; k + 8 <= NP; k += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += __longlong_as_double((long long)row[k + j]);
        }
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; k < NP; ++k) res += __longlong_as_double((long long)row[k]);
        ap[(size_t)c * NT + tid] = res / (double)NP;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The full COCO box protocol (utils/metrics.coco_summary): area ranges, crowd boxes, positions for AR.
//
//   k_eval_match_coco  k_eval_match's selection, rank sort and class segments, then one THREAD per (class segment, area range,
//                      threshold).  A ground truth is ignored in a range when it is crowd or its area lies outside it; the
//                      class's ground truths are two bit masks, valid and ignored, each walked in ascending index order: a
//                      detection looks at the unclaimed valid ones first and only without a match at the ignored ones, of which
//                      a crowd box may be claimed again.  The IoU against a crowd box (intersection / detection area) sits in
//                      the same LDS matrix.  An unmatched detection whose own area lies outside the range is ignored: that is
//                      the start value of its ignore word, which a match replaces bit by bit.
//   k_eval_ap_coco     k_eval_ap's scan per (class, area range) over the rows not ignored: the row index is the running count
//                      of non-ignored rows, the true-positive bits are masked by ~ig; beside it the true positives among the
//                      first 1 / 10 / max_dets detections of their (image, class) for the recall columns.
constexpr int NA = 4;                        // area ranges

struct AreaRanges { double lo[NA], hi[NA]; };

__device__ __forceinline__ bool outside(double area, double lo, double hi) { return area < lo || area > hi; }

// the pair's intersection over the detection's area (COCO's IoU against a crowd region); metrics.iou_matrix_crowd
__device__ __forceinline__ double ioa_f64(float4 d, double gx, double gy, double gw, double gh) {
    const double dx = (double)d.x, dy = (double)d.y, dw = (double)d.z, dh = (double)d.w;
    const double a0 = dx - dw / 2, a1 = dy - dh / 2, a2 = dx + dw / 2, a3 = dy + dh / 2;
    const double b0 = gx - gw / 2, b1 = gy - gh / 2, b2 = gx + gw / 2, b3 = gy + gh / 2;
    const double w = fmax(fmin(a2, b2) - fmax(a0, b0), 0.0);
    const double h = fmax(fmin(a3, b3) - fmax(a1, b1), 0.0);
    const double inter = w * h;
    const double area_a = (a2 - a0) * (a3 - a1);
    return area_a > 0.0 ? inter / fmax(area_a, 1e-300) : 0.0;
}

__global__ __launch_bounds__(WG) void k_eval_match_coco(
    const float* __restrict__ score, const int* __restrict__ cls, const float4* __restrict__ box,
    const uint8_t* __restrict__ keep, int A, const int* __restrict__ gt_cls, const double* __restrict__ gt_box,
    const int* __restrict__ gt_off, const uint8_t* __restrict__ gt_crowd, const double* __restrict__ area_scale, Thresholds thr,
    AreaRanges rng, int max_dets, int* __restrict__ n_det, float* __restrict__ det_score, int* __restrict__ det_cls,
    float4* __restrict__ det_box, uint16_t* __restrict__ det_flags, uint16_t* __restrict__ det_tp, uint16_t* __restrict__ det_ig,
    int* __restrict__ det_pos, uint8_t* __restrict__ gt_ignore) {
    // s_big: the sort keys [CAP] u64 + the candidate list [CAP] int during the selection; afterwards the IoU matrix [MAXD][GL]
    // or, uncached, s_match [NA][NT][MAXD]: the ground truth claimed by the detection at a position, -1 none
    __shared__ __attribute__((aligned(16))) double s_big[MAXD * GL];
    __shared__ float4 s_dbox[MAXD];
    __shared__ int s_dcls[MAXD];
    __shared__ int s_danchor[MAXD];
    __shared__ unsigned s_tp[NA][MAXD];
    __shared__ unsigned s_ig[NA][MAXD];
    __shared__ int s_ord[MAXD];                  // detection ranks ordered by (class, rank)
    __shared__ int s_seg[MAXD];                  // first position in s_ord of every class segment (any order)
    __shared__ double s_gbox[GL][4];
    __shared__ int s_gcls[GL];
    __shared__ unsigned s_gign[GL];              // bit a: ignored in range a; bit 8: crowd
    __shared__ int s_hist[256];
    __shared__ int s_wave[WG / 64];
    __shared__ int s_misc[4];
    static_assert(sizeof(double) * MAXD * GL >= sizeof(int) * NA * NT * MAXD, "the match list fits");
    unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_big);
    int* s_idx = reinterpret_cast<int*>(s_key + CAP);
    int (*s_match)[NT][MAXD] = reinterpret_cast<int (*)[NT][MAXD]>(s_big);

    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t off = (size_t)b * A;
    const float* sc = score + off;
    const uint8_t* kp = keep + off;
    const double scale = area_scale ? area_scale[b] : 1.0;

    const int nd = select_ranked(sc, kp, A, max_dets, s_key, s_idx, s_hist, s_wave, s_misc, s_danchor);
    // the detections: outputs fully written (slots at or beyond nd: score 0, class -1, box 0)
    if (tid < max_dets) {
        const size_t o = (size_t)b * max_dets + tid;
        float s = 0.f;
        int c = -1;
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < nd) {
            const int a = s_danchor[tid];
            s = sc[a];
            c = cls[off + a];
            bx = box[off + a];
            s_dcls[tid] = c;
            s_dbox[tid] = bx;
            const double area = (double)bx.z * (double)bx.w * scale;
#pragma unroll
            for (int a2 = 0; a2 < NA; ++a2) {    // unmatched: ignored where its own area lies outside the range
                s_tp[a2][tid] = 0u;
                s_ig[a2][tid] = outside(area, rng.lo[a2], rng.hi[a2]) ? 0x3ffu : 0u;
            }
        }
        det_score[o] = s;
        det_cls[o] = c;
        det_box[o] = bx;
    }
    if (tid == 0) n_det[b] = nd;
    __syncthreads();
    // class segments: position of a detection among those ordered by (class, rank); det_pos = its rank inside the class
    if (tid < max_dets) {
        int inside = 0;
        if (tid < nd) {
            const int c = s_dcls[tid];
            int pos = 0;
            for (int r = 0; r < nd; ++r) {
                const int cr = s_dcls[r];
                pos += (cr < c || (cr == c && r < tid)) ? 1 : 0;
                inside += (cr == c && r < tid) ? 1 : 0;
            }
            s_ord[pos] = tid;
        }
        det_pos[(size_t)b * max_dets + tid] = inside;
    }
    __syncthreads();
    if (tid < nd) {
        const bool start = tid == 0 || s_dcls[s_ord[tid]] != s_dcls[s_ord[tid - 1]];
        if (start) s_seg[atomicAdd(&s_misc[3], 1)] = tid;
    }
    const int g0 = gt_off[b];
    const int G = max(gt_off[b + 1] - g0, 0);
    const bool cached = G <= GL;
    double* s_iou = s_big;
    // the ground truths' ignore bits: crowd, or the area outside the range
    for (int j = tid; j < G; j += WG) {
        const double* g = gt_box + 4 * (size_t)(g0 + j);
        const double area = g[2] * g[3] * scale;
        const bool crowd = gt_crowd && gt_crowd[g0 + j];
        unsigned bits = 0u;
#pragma unroll
        for (int a = 0; a < NA; ++a) bits |= (crowd || outside(area, rng.lo[a], rng.hi[a])) ? (1u << a) : 0u;
        gt_ignore[g0 + j] = (uint8_t)bits;
        if (cached) {
            s_gign[j] = bits | (crowd ? 0x100u : 0u);
            s_gcls[j] = gt_cls[g0 + j];
#pragma unroll
            for (int e = 0; e < 4; ++e) s_gbox[j][e] = g[e];
        }
    }
    if (cached) {
        __syncthreads();
        // every class-matched IoU once (against a crowd box: intersection / detection area)
        for (int p = tid; p < nd * G; p += WG) {
            const int r = p / G, j = p - r * G;
            if (s_gcls[j] == s_dcls[r])
                s_iou[r * GL + j] = (s_gign[j] & 0x100u)
                                        ? ioa_f64(s_dbox[r], s_gbox[j][0], s_gbox[j][1], s_gbox[j][2], s_gbox[j][3])
                                        : iou_f64(s_dbox[r], s_gbox[j][0], s_gbox[j][1], s_gbox[j][2], s_gbox[j][3]);
        }
    }
    __syncthreads();
    const int nseg = s_misc[3];
    // the greedy pass: one thread per (class segment, area range, threshold)
    if (nd > 0 && G > 0) {
        for (int w = tid; w < nseg * NA * NT; w += WG) {
            const int sg = w / (NA * NT), a = (w / NT) % NA, t = w % NT;
            const int p0 = s_seg[sg];
            const int c = s_dcls[s_ord[p0]];
            const double th = thr.v[t];
            if (cached) {
                unsigned long long valid = 0ull, ign = 0ull, again = 0ull;      // this class's ground truths, by kind
                for (int j = 0; j < G; ++j) {
                    if (s_gcls[j] != c) continue;
                    const unsigned gi = s_gign[j];
                    if ((gi >> a) & 1u) ign |= 1ull << j; else valid |= 1ull << j;
                    if (gi & 0x100u) again |= 1ull << j;
                }
                if (!(valid | ign)) continue;
                unsigned long long taken = 0ull;
                for (int p = p0; p < nd; ++p) {
                    const int r = s_ord[p];
                    if (s_dcls[r] != c) break;
                    double best = th;
                    int bj = -1;
                    unsigned long long open = valid & ~taken;
                    while (open) {                   // ascending j, >=: the last index wins among equal IoUs
                        const int j = __ffsll((long long)open) - 1;
                        open &= open - 1ull;
                        const double v = s_iou[r * GL + j];
                        if (v >= best) { best = v; bj = j; }
                    }
                    if (bj < 0) {
                        open = ign & (~taken | again);
                        while (open) {
                            const int j = __ffsll((long long)open) - 1;
                            open &= open - 1ull;
                            const double v = s_iou[r * GL + j];
                            if (v >= best) { best = v; bj = j; }
                        }
                    }
                    if (bj >= 0) {
                        taken |= 1ull << bj;
                        atomicOr(&s_tp[a][r], 1u << t);
                        if ((ign >> bj) & 1ull) atomicOr(&s_ig[a][r], 1u << t); else atomicAnd(&s_ig[a][r], ~(1u << t));
                    }
                }
            } else {
                const double lo = rng.lo[a], hi = rng.hi[a];
                for (int p = p0; p < nd; ++p) {
                    const int r = s_ord[p];
                    if (s_dcls[r] != c) break;
                    const float4 d = s_dbox[r];
                    int bj = -1;
                    bool bign = false;
                    for (int pass = 0; pass < 2 && bj < 0; ++pass) {     // the valid ground truths, then the ignored ones
                        double best = th;
                        for (int j = 0; j < G; ++j) {
                            if (gt_cls[g0 + j] != c) continue;
                            const double* g = gt_box + 4 * (size_t)(g0 + j);
                            const bool crowd = gt_crowd && gt_crowd[g0 + j];
                            const bool gign = crowd || outside(g[2] * g[3] * scale, lo, hi);
                            if (gign != (pass == 1)) continue;
                            const double v = crowd ? ioa_f64(d, g[0], g[1], g[2], g[3]) : iou_f64(d, g[0], g[1], g[2], g[3]);
                            if (!(v >= best)) continue;
                            bool taken = false;      // claimed by an earlier detection of the segment?
                            if (!crowd)
                                for (int q = p0; q < p && !taken; ++q) taken = s_match[a][t][q] == j;
                            if (!taken) { best = v; bj = j; bign = gign; }
                        }
                    }
                    s_match[a][t][p] = bj;
                    if (bj >= 0) {
                        atomicOr(&s_tp[a][r], 1u << t);
                        if (bign) atomicOr(&s_ig[a][r], 1u << t); else atomicAnd(&s_ig[a][r], ~(1u << t));
                    }
                }
            }
        }
    }
    __syncthreads();
    if (tid < max_dets) {
        const size_t o = (size_t)b * max_dets + tid;
        const bool live = tid < nd;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            det_tp[o * NA + a] = live ? (uint16_t)s_tp[a][tid] : (uint16_t)0;
            det_ig[o * NA + a] = live ? (uint16_t)s_ig[a][tid] : (uint16_t)0;
        }
        det_flags[o] = live ? (uint16_t)(s_tp[0][tid] & ~s_ig[0][tid]) : (uint16_t)0;
    }
}

// AP of one (class, area range) at the ten thresholds over the rows that are not ignored, and the true positives among the
// first 1 / 10 / max_dets detections of their (image, class).  tp, ig: [N][NA] words of every detection of the data set, sorted.
__global__ __launch_bounds__(AWG) void k_eval_ap_coco(const uint16_t* __restrict__ tp, const uint16_t* __restrict__ ig,
                                                     const int* __restrict__ pos, const int* __restrict__ seg_off,
                                                     const int* __restrict__ n_gt, int C, int max_dets, RecallPoints pts,
                                                     double* __restrict__ ap, int* __restrict__ tp_count) {
    __shared__ unsigned long long s_best[NT][NP];    // bits of the best precision whose last recall point <= recall is k
    __shared__ double s_pts[NP];
    __shared__ int s_wtot[2][AWG / 64][2 * NT];
    __shared__ int s_cnt[3][NT];                     // true positives with pos < 1, pos < 10, pos < max_dets
    const int c = blockIdx.x, a = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t cell = (size_t)c * NA + a;
    const int ngt = n_gt[(size_t)a * C + c];
    if (ngt <= 0) {                                  // not part of any mean (the caller excludes it)
        if (tid < NT) ap[cell * NT + tid] = 0.0;
        if (tid < 3 * NT) tp_count[cell * 3 * NT + tid] = 0;
        return;
    }
    for (int i = tid; i < NT * NP; i += AWG) (&s_best[0][0])[i] = 0ull;
    if (tid < 3 * NT) (&s_cnt[0][0])[tid] = 0;
    if (tid == 0) {                                  // constant indices: a lane-indexed read would copy the argument to scratch
#pragma unroll
        for (int k = 0; k < NP; ++k) s_pts[k] = pts.v[k];
    }
    const long long lo = seg_off[c], hi = seg_off[c + 1];
    const double dngt = (double)ngt;
    int carry_tp[NT], carry_n[NT], first1[NT], first10[NT], firstm[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) carry_tp[t] = carry_n[t] = first1[t] = first10[t] = firstm[t] = 0;
    __syncthreads();
    int par = 0;
    for (long long i0 = lo; i0 < hi; i0 += AWG, par ^= 1) {
        const long long i = i0 + tid;
        const bool in = i < hi;
        const unsigned live = in ? (~(unsigned)ig[i * NA + a] & 0x3ffu) : 0u;    // bit t: the row counts at threshold t
        const unsigned f = in ? ((unsigned)tp[i * NA + a] & live) : 0u;
        const int ps = in ? pos[i] : INT_MAX;
        int incl_tp[NT], incl_n[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const unsigned long long m = __ballot((f >> t) & 1u);
            const unsigned long long n = __ballot((live >> t) & 1u);
            incl_tp[t] = __popcll(m & ((2ull << lane) - 1ull));
            incl_n[t] = __popcll(n & ((2ull << lane) - 1ull));
            if (lane == 0) {
                s_wtot[par][wave][t] = __popcll(m);
                s_wtot[par][wave][NT + t] = __popcll(n);
            }
        }
        __syncthreads();                             // (double-buffered totals: one barrier per chunk)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            int base = carry_tp[t], tot = 0, nbase = carry_n[t], ntot = 0;
#pragma unroll
            for (int w = 0; w < AWG / 64; ++w) {
                const int v = s_wtot[par][w][t], u = s_wtot[par][w][NT + t];
                if (w < wave) { base += v; nbase += u; }
                tot += v;
                ntot += u;
            }
            carry_tp[t] += tot;
            carry_n[t] += ntot;
            if ((f >> t) & 1u) {
                first1[t] += ps < 1 ? 1 : 0;
                first10[t] += ps < 10 ? 1 : 0;
                firstm[t] += ps < max_dets ? 1 : 0;
                const int ctp = base + incl_tp[t];
                const double prec = (double)ctp / (double)(nbase + incl_n[t]);
                const double rec = (double)ctp / dngt;
                int a2 = 0, z = NP - 1;              // last k with pts[k] <= rec (pts[0] = 0 <= rec)
                while (a2 < z) {
                    const int mid = (a2 + z + 1) >> 1;
                    if (s_pts[mid] <= rec) a2 = mid; else z = mid - 1;
                }
                atomicMax(&s_best[t][a2], (unsigned long long)__double_as_longlong(prec));
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (first1[t]) atomicAdd(&s_cnt[0][t], first1[t]);
        if (first10[t]) atomicAdd(&s_cnt[1][t], first10[t]);
        if (firstm[t]) atomicAdd(&s_cnt[2][t], firstm[t]);
    }
    __syncthreads();
    if (tid < NT) {
        // k_eval_ap's envelope and its mean in numpy's summation order
        unsigned long long* row = s_best[tid];
        unsigned long long run = 0ull;
        for (int k = NP - 1; k >= 0; --k) {
            run = row[k] > run ? row[k] : run;
            row[k] = run;
        }
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = __longlong_as_double((long long)row[j]);
        int k = 8;
        for (; k + 8 <= NP; k += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += __longlong_as_double((long long)row[k + j]);
        }
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; k < NP; ++k) res += __longlong_as_double((long long)row[k]);
        ap[cell * NT + tid] = res / (double)NP;
        tp_count[(cell * 3 + 0) * NT + tid] = s_cnt[0][tid];
        tp_count[(cell * 3 + 1) * NT + tid] = s_cnt[1][tid];
        tp_count[(cell * 3 + 2) * NT + tid] = s_cnt[2][tid];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// PASCAL VOC (utils/metrics.voc_map, VOCdevkit's VOCevaldet): one IoU threshold, no greedy pass.
//
//   k_eval_match_voc  select_ranked, then one THREAD per detection: (ovmax, jmax) over ALL boxes of its class in the image,
//                     claimed or not, difficult ones included, the FIRST index winning among equal IoUs.  A detection whose
//                     ovmax reaches the threshold is ignored when box jmax is difficult, a true positive when it is the
//                     lowest-ranked detection with that jmax, a false positive (duplicate) otherwise.  With at most GLV boxes
//                     in the image they sit in LDS and the lowest rank per box is an LDS minimum; with more, boxes are read from
//                     memory and a detection compares its rank with the earlier detections' jmax -- identical results.
//   k_eval_ap_voc     per class from the flags sorted by (class, score desc, image, rank): the 11-point mean (year 7) or the
//                     area under the monotone envelope (year 12).  Only true positives raise recall, and a row that is none
//                     never lies above the envelope of the true positive before it, so both reduce to the true-positive rows:
//                     year 7 is k_eval_ap's bucket maximum over 11 points; year 12 is the sum, in row order, of
//                     (ctp / n_pos - (ctp - 1) / n_pos) * (largest precision at or after the row).  That suffix maximum comes
//                     from a first pass that leaves the largest precision of every slot of rows in LDS; the second pass then
//                     forms the terms in parallel and one thread adds them in order.
constexpr int MAXDV = 256;                   // ssd_eval_voc_max_dets()
constexpr int GLV = 64;                      // ground truths per image held in LDS
constexpr int NPV = 11;                      // recall points of the VOC2007 metric
constexpr int NSLOT = 2048;                  // year 12: slots of rows whose largest precision is kept in LDS
constexpr int NSUB = 4096;                   // chunks per slot at most: NSLOT * NSUB * AWG rows >= 2^31

struct RecallPoints11 { double v[NPV]; };

__global__ __launch_bounds__(WG) void k_eval_match_voc(
    const float* __restrict__ score, const int* __restrict__ cls, const float4* __restrict__ box,
    const uint8_t* __restrict__ keep, int A, const int* __restrict__ gt_cls, const double* __restrict__ gt_box,
    const int* __restrict__ gt_off, const uint8_t* __restrict__ gt_difficult, double iou_thresh, int max_dets,
    int* __restrict__ n_det, float* __restrict__ det_score, int* __restrict__ det_cls, float4* __restrict__ det_box,
    uint8_t* __restrict__ det_flags, int* __restrict__ det_gt) {
    __shared__ unsigned long long s_key[CAP];
    __shared__ int s_idx[CAP];
    __shared__ float4 s_dbox[MAXDV];
    __shared__ int s_dcls[MAXDV];
    __shared__ int s_danchor[MAXDV];
    __shared__ int s_jmax[MAXDV];                // box a detection passes the threshold with, -1 none
    __shared__ double s_gbox[GLV][4];
    __shared__ int s_gcls[GLV];
    __shared__ int s_first[GLV];                 // lowest rank among the detections whose jmax is the box
    __shared__ int s_hist[256];
    __shared__ int s_wave[WG / 64];
    __shared__ int s_misc[4];

    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t off = (size_t)b * A;
    const float* sc = score + off;
    const uint8_t* kp = keep + off;

    const int nd = select_ranked(sc, kp, A, max_dets, s_key, s_idx, s_hist, s_wave, s_misc, s_danchor);
    const int g0 = gt_off[b];
    const int G = max(gt_off[b + 1] - g0, 0);
    const bool cached = G <= GLV;
    // the detections: outputs fully written (slots at or beyond nd: score 0, class -1, box 0)
    if (tid < max_dets) {
        const size_t o = (size_t)b * max_dets + tid;
        float s = 0.f;
        int c = -1;
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < nd) {
            const int a = s_danchor[tid];
            s = sc[a];
            c = cls[off + a];
            bx = box[off + a];
            s_dcls[tid] = c;
            s_dbox[tid] = bx;
        }
        det_score[o] = s;
        det_cls[o] = c;
        det_box[o] = bx;
    }
    if (tid == 0) n_det[b] = nd;
    if (cached && tid < G) {
        s_gcls[tid] = gt_cls[g0 + tid];
        s_first[tid] = INT_MAX;
#pragma unroll
        for (int e = 0; e < 4; ++e) s_gbox[tid][e] = gt_box[4 * (size_t)(g0 + tid) + e];
    }
    __syncthreads();
    // (ovmax, jmax): ascending j and >, so the first index wins among equal IoUs
    int jm = -1;
    if (tid < nd) {
        const int c = s_dcls[tid];
        const float4 d = s_dbox[tid];
        double best = -1.0;
        int bj = -1;
        if (cached) {
            for (int j = 0; j < G; ++j) {
                if (s_gcls[j] != c) continue;
                const double v = iou_f64(d, s_gbox[j][0], s_gbox[j][1], s_gbox[j][2], s_gbox[j][3]);
                if (v > best) { best = v; bj = j; }
            }
        } else {
            for (int j = 0; j < G; ++j) {
                if (gt_cls[g0 + j] != c) continue;
                const double* g = gt_box + 4 * (size_t)(g0 + j);
                const double v = iou_f64(d, g[0], g[1], g[2], g[3]);
                if (v > best) { best = v; bj = j; }
            }
        }
        jm = (bj >= 0 && best >= iou_thresh) ? bj : -1;
        s_jmax[tid] = jm;
        if (cached && jm >= 0) atomicMin(&s_first[jm], tid);
    }
    __syncthreads();
    if (tid < max_dets) {
        unsigned f = 0u;
        if (jm >= 0) {
            if (gt_difficult && gt_difficult[g0 + jm]) {
                f = 2u;
            } else if (cached) {
                f = s_first[jm] == tid ? 1u : 0u;
            } else {
                bool dup = false;                    // an earlier detection with the same box?
                for (int r = 0; r < tid && !dup; ++r) dup = s_jmax[r] == jm;
                f = dup ? 0u : 1u;
            }
        }
        const size_t o = (size_t)b * max_dets + tid;
        det_flags[o] = (uint8_t)f;
        det_gt[o] = jm;
    }
}

// AP of one class.  flags: every detection of the data set, sorted (bit 0 true positive, bit 1 ignored: neither count);
// seg_off[c] .. seg_off[c+1] the class's rows.  Any segment length.
__global__ __launch_bounds__(AWG) void k_eval_ap_voc(const uint8_t* __restrict__ flags, const int* __restrict__ seg_off,
                                                    const int* __restrict__ n_pos, int year, RecallPoints11 pts,
                                                    double* __restrict__ ap) {
    __shared__ unsigned long long s_slot[NSLOT];     // year 12: bits of the largest precision in a slot, then of the suffix
    __shared__ unsigned long long s_sub[NSUB];       // the same per chunk inside the current slot (slots of several chunks)
    __shared__ unsigned long long s_best[NPV];       // year 7: bits of the best precision whose last recall point <= recall is k
    __shared__ double s_pts[NPV];
    __shared__ double s_term[AWG];
    __shared__ double s_wmax[AWG / 64];
    __shared__ int s_wtot[AWG / 64][2];
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npos = n_pos[c];
    const long long lo = seg_off[c], hi = seg_off[c + 1];
    if (npos <= 0 || hi <= lo) {                     // not part of the mean (the caller excludes it), or no detection
        if (tid == 0) ap[c] = 0.0;
        return;
    }
    const double dnpos = (double)npos;
    const long long nchunk = (hi - lo + AWG - 1) / AWG;
    const long long cps = (nchunk + NSLOT - 1) / NSLOT;      // chunks per slot
    const int nslot = (int)((nchunk + cps - 1) / cps);
    if (year == 7) {
        if (tid < NPV) s_best[tid] = 0ull;
        if (tid == 0) {                              // constant indices: a lane-indexed read would copy the argument to scratch
#pragma unroll
            for (int k = 0; k < NPV; ++k) s_pts[k] = pts.v[k];
        }
    } else {
        for (int i = tid; i < nslot; i += AWG) s_slot[i] = 0ull;
    }
    __syncthreads();
    // one chunk: the row's kind and its inclusive counts of true and false positives; the carries move on
    int carry_tp = 0, carry_fp = 0;
    auto scan = [&](long long i0, bool& is_tp, int& ctp, int& cfp) {
        const long long i = i0 + tid;
        const unsigned f = i < hi ? (unsigned)flags[i] & 3u : 2u;
        is_tp = f == 1u;
        const unsigned long long mt = __ballot(is_tp), mf = __ballot(f == 0u);
        const unsigned long long upto = (2ull << lane) - 1ull;
        ctp = __popcll(mt & upto);
        cfp = __popcll(mf & upto);
        __syncthreads();
        if (lane == 0) { s_wtot[wave][0] = __popcll(mt); s_wtot[wave][1] = __popcll(mf); }
        __syncthreads();
        int tot_tp = 0, tot_fp = 0;
#pragma unroll
        for (int w = 0; w < AWG / 64; ++w) {
            const int vt = s_wtot[w][0], vf = s_wtot[w][1];
            if (w < wave) { ctp += vt; cfp += vf; }
            tot_tp += vt;
            tot_fp += vf;
        }
        ctp += carry_tp;
        cfp += carry_fp;
        carry_tp += tot_tp;
        carry_fp += tot_fp;
    };
    // first pass: year 7 the bucket maxima, year 12 the slot maxima
    for (long long ch = 0; ch < nchunk; ++ch) {
        bool is_tp;
        int ctp, cfp;
        scan(lo + ch * AWG, is_tp, ctp, cfp);
        if (!is_tp) continue;
        const double prec = (double)ctp / (double)(ctp + cfp);
        if (year == 7) {
            const double rec = (double)ctp / dnpos;
            int a = -1;                              // last k with pts[k] <= rec (none when pts[0] > rec)
            for (int k = 0; k < NPV; ++k) a = s_pts[k] <= rec ? k : a;
            if (a >= 0) atomicMax(&s_best[a], (unsigned long long)__double_as_longlong(prec));
        } else {
            atomicMax(&s_slot[ch / cps], (unsigned long long)__double_as_longlong(prec));
        }
    }
    __syncthreads();
    if (year == 7) {
        if (tid == 0) {                              // envelope = suffix maximum over the buckets; the points added in order
            unsigned long long run = 0ull;
            for (int k = NPV - 1; k >= 0; --k) {
                run = s_best[k] > run ? s_best[k] : run;
                s_best[k] = run;
            }
            double res = 0.0;
            for (int k = 0; k < NPV; ++k) res += __longlong_as_double((long long)s_best[k]);
            ap[c] = res / 11.0;
        }
        return;
    }
    if (tid == 0) {                                  // s_slot[s] = largest precision in slot s or any later one
        unsigned long long run = 0ull;
        for (int k = nslot - 1; k >= 0; --k) {
            run = s_slot[k] > run ? s_slot[k] : run;
            s_slot[k] = run;
        }
    }
    __syncthreads();
    carry_tp = carry_fp = 0;
    double acc = 0.0;                                // thread 0's
    for (int sl = 0; sl < nslot; ++sl) {
        const long long ch0 = (long long)sl * cps, ch1 = ch0 + cps < nchunk ? ch0 + cps : nchunk;
        const int nsub = (int)(ch1 - ch0);
        if (nsub > 1) {                              // the chunk maxima inside the slot, then their suffix
            const int keep_tp = carry_tp, keep_fp = carry_fp;
            for (int i = tid; i < nsub; i += AWG) s_sub[i] = 0ull;
            __syncthreads();
            for (long long ch = ch0; ch < ch1; ++ch) {
                bool is_tp;
                int ctp, cfp;
                scan(lo + ch * AWG, is_tp, ctp, cfp);
                if (is_tp)
                    atomicMax(&s_sub[ch - ch0], (unsigned long long)__double_as_longlong((double)ctp / (double)(ctp + cfp)));
            }
            __syncthreads();
            if (tid == 0) {
                unsigned long long run = 0ull;
                for (int k = nsub - 1; k >= 0; --k) {
                    run = s_sub[k] > run ? s_sub[k] : run;
                    s_sub[k] = run;
                }
            }
            __syncthreads();
            carry_tp = keep_tp;
            carry_fp = keep_fp;
        }
        const unsigned long long after_slot = sl + 1 < nslot ? s_slot[sl + 1] : 0ull;
        for (long long ch = ch0; ch < ch1; ++ch) {
            const int first_tp = carry_tp;
            bool is_tp;
            int ctp, cfp;
            scan(lo + ch * AWG, is_tp, ctp, cfp);
            // largest precision at or after the row: inside the wave, the later waves, the later chunks and slots
            double v = is_tp ? (double)ctp / (double)(ctp + cfp) : 0.0;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const double o = __shfl_down(v, d);
                if (lane + d < 64 && o > v) v = o;
            }
            if (lane == 0) s_wmax[wave] = v;
            __syncthreads();
#pragma unroll
            for (int w = 1; w < AWG / 64; ++w)
                if (w > wave && s_wmax[w] > v) v = s_wmax[w];
            unsigned long long later = after_slot;
            if (ch + 1 < ch1 && s_sub[ch + 1 - ch0] > later) later = s_sub[ch + 1 - ch0];
            const double tail = __longlong_as_double((long long)later);
            if (tail > v) v = tail;
            if (is_tp) s_term[ctp - first_tp - 1] = ((double)ctp / dnpos - (double)(ctp - 1) / dnpos) * v;
            __syncthreads();
            if (tid == 0) {
                const int n = carry_tp - first_tp;
                for (int k = 0; k < n; ++k) acc += s_term[k];
            }
            __syncthreads();
        }
    }
    if (tid == 0) ap[c] = acc;
}

}  // namespace

extern "C" {

int ssd_eval_max_dets(void) { return MAXD; }

int ssd_eval_match(const float* score, const int32_t* cls, const float* box, const uint8_t* keep, int B, int A,
                   const int32_t* gt_cls, const double* gt_box, const int32_t* gt_off, const double* iou_thresholds,
                   int max_dets, int32_t* n_det, float* det_score, int32_t* det_cls, float* det_box, uint16_t* det_flags,
                   void* stream) {
    if (B <= 0 || A <= 0 || max_dets <= 0 || max_dets > MAXD) return SSD_ERR_VALUE;
    if (!score || !cls || !box || !keep || !gt_off || !iou_thresholds) return SSD_ERR_VALUE;
    if (!n_det || !det_score || !det_cls || !det_box || !det_flags) return SSD_ERR_VALUE;
    Thresholds thr;
    for (int t = 0; t < NT; ++t) thr.v[t] = iou_thresholds[t];
    hipLaunchKernelGGL(k_eval_match, dim3(B), dim3(WG), 0, (hipStream_t)stream, score, cls, reinterpret_cast<const float4*>(box),
                       keep, A, gt_cls, gt_box, gt_off, thr, max_dets, n_det, det_score, det_cls,
                       reinterpret_cast<float4*>(det_box), det_flags);
    return ssd_launch_status();
}

int ssd_eval_ap(const uint16_t* flags_sorted, const int32_t* seg_off, const int32_t* n_gt, int C, const double* recall_points,
                double* ap, void* stream) {
    if (C <= 0 || !flags_sorted || !seg_off || !n_gt || !recall_points || !ap) return SSD_ERR_VALUE;
    RecallPoints pts;
    for (int k = 0; k < NP; ++k) pts.v[k] = recall_points[k];
    hipLaunchKernelGGL(k_eval_ap, dim3(C), dim3(AWG), 0, (hipStream_t)stream, flags_sorted, seg_off, n_gt, pts, ap);
    return ssd_launch_status();
}

int ssd_eval_match_coco(const float* score, const int32_t* cls, const float* box, const uint8_t* keep, int B, int A,
                        const int32_t* gt_cls, const double* gt_box, const int32_t* gt_off, const uint8_t* gt_crowd,
                        const double* area_scale, const double* area_ranges, const double* iou_thresholds, int max_dets,
                        int32_t* n_det, float* det_score, int32_t* det_cls, float* det_box, uint16_t* det_flags, uint16_t* det_tp,
                        uint16_t* det_ig, int32_t* det_pos, uint8_t* gt_ignore, void* stream) {
    if (B <= 0 || A <= 0 || max_dets <= 0 || max_dets > MAXD) return SSD_ERR_VALUE;
    if (!score || !cls || !box || !keep || !gt_off || !iou_thresholds || !area_ranges) return SSD_ERR_VALUE;
    if (!n_det || !det_score || !det_cls || !det_box || !det_flags || !det_tp || !det_ig || !det_pos) return SSD_ERR_VALUE;
    Thresholds thr;
    for (int t = 0; t < NT; ++t) thr.v[t] = iou_thresholds[t];
    AreaRanges rng;
    for (int a = 0; a < NA; ++a) {
        rng.lo[a] = area_ranges[2 * a];
        rng.hi[a] = area_ranges[2 * a + 1];
    }
    hipLaunchKernelGGL(k_eval_match_coco, dim3(B), dim3(WG), 0, (hipStream_t)stream, score, cls,
                       reinterpret_cast<const float4*>(box), keep, A, gt_cls, gt_box, gt_off, gt_crowd, area_scale, thr, rng,
                       max_dets, n_det, det_score, det_cls, reinterpret_cast<float4*>(det_box), det_flags, det_tp, det_ig, det_pos,
                       gt_ignore);
    return ssd_launch_status();
}

int ssd_eval_ap_coco(const uint16_t* tp_sorted, const uint16_t* ig_sorted, const int32_t* pos_sorted, const int32_t* seg_off,
                     const int32_t* n_gt, int C, int max_dets, const double* recall_points, double* ap, int32_t* tp_count,
                     void* stream) {
    if (C <= 0 || max_dets <= 0 || max_dets > MAXD) return SSD_ERR_VALUE;
    if (!tp_sorted || !ig_sorted || !pos_sorted || !seg_off || !n_gt || !recall_points || !ap || !tp_count) return SSD_ERR_VALUE;
    RecallPoints pts;
    for (int k = 0; k < NP; ++k) pts.v[k] = recall_points[k];
    hipLaunchKernelGGL(k_eval_ap_coco, dim3(C, NA), dim3(AWG), 0, (hipStream_t)stream, tp_sorted, ig_sorted, pos_sorted, seg_off,
                       n_gt, C, max_dets, pts, ap, tp_count);
    return ssd_launch_status();
}

int ssd_eval_voc_max_dets(void) { return MAXDV; }

int ssd_eval_match_voc(const float* score, const int32_t* cls, const float* box, const uint8_t* keep, int B, int A,
                       const int32_t* gt_cls, const double* gt_box, const int32_t* gt_off, const uint8_t* gt_difficult,
                       double iou_thresh, int max_dets, int32_t* n_det, float* det_score, int32_t* det_cls, float* det_box,
                       uint8_t* det_flags, int32_t* det_gt, void* stream) {
    if (B <= 0 || A <= 0 || max_dets <= 0 || max_dets > MAXDV) return SSD_ERR_VALUE;
    if (!(iou_thresh > 0.0) || !(iou_thresh <= DBL_MAX)) return SSD_ERR_VALUE;
    if (!score || !cls || !box || !keep || !gt_off) return SSD_ERR_VALUE;
    if (!n_det || !det_score || !det_cls || !det_box || !det_flags || !det_gt) return SSD_ERR_VALUE;
    hipLaunchKernelGGL(k_eval_match_voc, dim3(B), dim3(WG), 0, (hipStream_t)stream, score, cls,
                       reinterpret_cast<const float4*>(box), keep, A, gt_cls, gt_box, gt_off, gt_difficult, iou_thresh, max_dets,
                       n_det, det_score, det_cls, reinterpret_cast<float4*>(det_box), det_flags, det_gt);
    return ssd_launch_status();
}

int ssd_eval_ap_voc(const uint8_t* flags_sorted, const int32_t* seg_off, const int32_t* n_pos, int C, int year,
                    const double* recall_points, double* ap, void* stream) {
    if (C <= 0 || (year != 7 && year != 12)) return SSD_ERR_VALUE;
    if (!flags_sorted || !seg_off || !n_pos || !recall_points || !ap) return SSD_ERR_VALUE;
    RecallPoints11 pts;
    for (int k = 0; k < NPV; ++k) pts.v[k] = recall_points[k];
    hipLaunchKernelGGL(k_eval_ap_voc, dim3(C), dim3(AWG), 0, (hipStream_t)stream, flags_sorted, seg_off, n_pos, year, pts, ap);
    return ssd_launch_status();
}

}  // extern "C"
