/*
 * ssd_hip.h -- C ABI of the MI355X (gfx950) SSD hot-path library  (libssd_hip.so)
 *
 * Drop-in boundary for the data-parallel hot path of AcherStyx/SSD-Object-Detection.
 * The reference is pure Python (TensorFlow + numpy) and has no FFI; each entry point below
 * replaces one Python-level seam, cited as <file>:<line> relative to the reference tree.
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add at each seam.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - Unless a parameter says HOST, every pointer is a DEVICE pointer owned by the caller.
 *     The library allocates nothing, creates no streams, reads no environment variables and keeps no state that
 *     a result depends on: calls are re-entrant and thread-safe.  (Its only process-wide state: the idempotent
 *     once-per-device registration of kernels that need > 64 KB of LDS, and the development overrides of
 *     ssd_dev_knob at the end of this header, which the product never sets.)
 *     Scratch is passed as (ws, ws_bytes) sized by the matching *_workspace_bytes().
 *   - `stream` (last argument) is a hipStream_t passed as void*; all work is enqueued on it
 *     and nothing synchronises the host, so every call can be captured into a hipGraph.
 *   - Return value: SSD_OK (0) or a negative ssd_status.  Kernels never abort.  The Python
 *     wrapper maps SSD_ERR_ASSERT to AssertionError and SSD_ERR_VALUE to ValueError, the
 *     exception types the reference raises at the same seams.
 *   - Layouts: boxes are (cx, cy, w, h); activations NHWC; conv weights [Cout][kh][kw][Cin].
 *   - Alignment: every tensor pointer and every workspace 16-byte aligned (hipMalloc gives 256); the loc / conf outputs of
 *     ssd_conv2d_head_fwd 4-byte aligned.  Kernels use 16-byte vector accesses on them without checking.
 */
#ifndef SSD_HIP_H
#define SSD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SSD_OK = 0,
    SSD_ERR_ASSERT = -1,    /* a reference `assert` would have fired (utils/bbox.py:50-51,95; models/ssd_model.py:347-351,375) */
    SSD_ERR_VALUE = -2,     /* bad argument (reference: ValueError / TF InvalidArgument)                    */
    SSD_ERR_WORKSPACE = -3, /* ws_bytes smaller than *_workspace_bytes()                                    */
    SSD_ERR_LAUNCH = -4,    /* HIP launch failure (hipGetLastError != hipSuccess)                           */
    SSD_ERR_UNSUPPORTED = -5
} ssd_status;

typedef enum { SSD_F32 = 0, SSD_BF16 = 1 } ssd_dtype;

int ssd_hip_abi_version(void);
const char* ssd_status_string(int status);

/* ------------------------------------------------------------------------------------------
 * Default boxes -- replaces SSDObjectDetectionModel._build_prior_box (models/ssd_model.py:173-194)
 *   grid_hw    HOST int[2*levels]   (h, w) per level            (reference: loc-head output shapes, :164)
 *   s_ref      HOST double[levels+1]                            (:176)
 *   ratios     HOST int[ratio_off[levels]], ratio_off HOST int[levels+1]   (:177, CSR form)
 *   in_size    input side in pixels (300)                       (:184)
 *   out        DEVICE double[A*4], A = ssd_priors_count(...)    (cx,cy,w,h), unclipped, reference order
 * Bit-exact against the reference's float64 array.
 * ---------------------------------------------------------------------------------------- */
int ssd_priors_count(const int* grid_hw, int levels, const int* ratio_off);
int ssd_priors(const int* grid_hw, int levels, const double* s_ref, const int* ratios,
               const int* ratio_off, double in_size, double* out, void* stream);

/* Geometry of a prior set made by ssd_priors (levels <= SSD_MAX_LEVELS). */
#define SSD_MAX_LEVELS 8
#define SSD_GRID_VERIFIED 0x5D5D0001
typedef struct {
    int levels;
    int grid_h[SSD_MAX_LEVELS];
    int grid_w[SSD_MAX_LEVELS];
    int per_cell[SSD_MAX_LEVELS]; /* priors per cell = 2 + 2*len(ratios[level]) */
    int verified;                 /* SSD_GRID_VERIFIED once ssd_prior_grid_verify has checked it against a prior array; else 0 */
} ssd_prior_grid;

/* Check on the device that `grid` describes `priors` exactly: every prior at the cell centre ssd_priors computes, bit for
 * bit, in the reference's order, with one (w, h) per level and anchor type.  Sets grid->verified (HOST) accordingly and
 * returns SSD_OK either way; synchronises `stream` once -- call it when the prior set is built, not per step.
 *   scratch DEVICE int32[1].
 * ssd_match_encode takes its single-launch path only with a verified grid; a grid that was not verified (or does not fit)
 * is a pruning hint only and can never change a result. */
int ssd_prior_grid_verify(const double* priors, int A, ssd_prior_grid* grid, int32_t* scratch, void* stream);

/* Encoding of an all-zero (unmatched) target row against every prior: the value
 * apply_anchor_box (utils/bbox.py:94-101) produces for rows match_bbox left at 0, cast to f32 as
 * the TensorSpec at models/ssd_model.py:222 does.  Image-independent; computed once.
 *   priors DEVICE double[A*4] -> enc_zero DEVICE float[A*4] */
int ssd_encode_zero(const double* priors, int A, float* enc_zero, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batched target assignment -- replaces, for a whole batch, the per-image generator body
 *   match_bbox(cls, bbox, prior_box, thresh)   utils/bbox.py:44-91   (called models/ssd_model.py:212)
 *   apply_anchor_box(matched_loc, prior_box)   utils/bbox.py:94-101  (called models/ssd_model.py:213)
 *   + the float32 cast of the TensorSpec        models/ssd_model.py:222
 *
 *   gt_box   float[total_gt*4]  all images' boxes, concatenated (cx,cy,w,h in [0,1], w,h >= 0, finite)
 *   gt_cls   float[total_gt]    class ids stored as float (as the loaders emit them)
 *   gt_off   int32[B+1]         image b owns rows gt_off[b] .. gt_off[b+1]-1   (DEVICE)
 *   total_gt, max_nt            HOST-known sum / max of per-image counts (max_nt <= A else SSD_ERR_ASSERT, :50)
 *   priors   double[A*4]; enc_zero float[A*4] from ssd_encode_zero
 *   grid     HOST, may be NULL.  Optional: the geometry `priors` was generated with (ssd_priors).  Verified
 *            (ssd_prior_grid_verify) it selects the single-launch path, which enumerates the columns that can matter to
 *            a gt row from the geometry; unverified it only seeds a pruning bound.  Results are identical with,
 *            without or with a wrong hint.
 *   thresh   > 0 else SSD_ERR_ASSERT (:51)
 *   out_cls  int32[B*A]   (0 where unmatched -- not the background id, as in the reference)
 *   out_loc  float[B*A*4] encoded offsets (finite "zero-row" values where unmatched, as in the reference)
 *   out_mask uint8[B*A]   1 = positive
 *   out_owner int32[B*A] or NULL: the matched gt row of each anchor within its image (-1 = unmatched),
 *            i.e. index_list of utils/bbox.py:60-79 as a dense map.  The training path passes NULL.
 *   ws       scratch of >= ssd_match_encode_workspace_bytes(B, A, total_gt) bytes (used by the three-launch path only:
 *            no verified grid, or an image with more than 64 boxes); no state is kept in it.
 * Anchor indices / classes / masks are bit-exact with the reference; out_loc is bit-exact in
 * the division terms and <= 1 float32 ulp in the log terms (device log vs numpy log).
 * ---------------------------------------------------------------------------------------- */
size_t ssd_match_encode_workspace_bytes(int B, int A, int total_gt);
int ssd_match_encode(const float* gt_box, const float* gt_cls, const int32_t* gt_off, int B,
                     int total_gt, int max_nt, const double* priors, const float* enc_zero, int A,
                     const ssd_prior_grid* grid, double thresh, int32_t* out_cls, float* out_loc,
                     uint8_t* out_mask, int32_t* out_owner, void* ws, size_t ws_bytes, void* stream);

/* apply_anchor_box (utils/bbox.py:94-101) on n paired rows: float32 boxes against float64 priors,
 * float64 result [n*4] exactly as numpy returns it (division terms bit-exact, log terms <= 1 ulp).
 * The same shapes are required of both inputs by the reference's assert (:95); the wrapper checks. */
int ssd_apply_anchor_box(const float* box, const double* priors, int n, double* out, void* stream);

/* Pairwise IoU, the reference's iou_n (utils/bbox.py:28-41) for float32 box_1 rows against
 * float64 box_2 rows (the dtype mix match_bbox feeds it): out[i] = iou(b1[i], b2[i]), float64,
 * bit-exact.  Exposed for parity tests and for callers of iou_n. */
int ssd_iou_n(const float* b1, const double* b2, int n, double* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training loss, forward + backward -- replaces SSDObjectDetectionModel._ssd_loss
 * (models/ssd_model.py:341-396) and the part of tape.gradient (:248) that flows into the two
 * network outputs.
 *   conf      [B*A*C] class logits, background = class C-1 (:47,364-365); dtype SSD_F32 or SSD_BF16
 *   loc       [B*A*4] predicted offsets, same dtype
 *   gt_cls    int32[B*A], gt_loc float[B*A*4], gt_mask uint8[B*A]: the outputs of ssd_match_encode
 *   grad_scale multiplies both gradients (1.0 = d total_loss)
 *   out8      float[8]: loc loss, cls loss pos, cls loss neg (the reference's three scalars, :392-394),
 *             their sum, P, N (= number of mined negatives, ties included :372), tau, status
 *             (0 ok; 1 = P==0 or 3P > B*A, where TF would raise; 2 = tau==0, where the assert at :375 fires;
 *             3 = a logit row or a positive's offsets were NaN / Inf: a diverged run, reported first)
 *   dconf     [B*A*C], dloc [B*A*4]: gradients, same dtype as conf/loc; every element is written.  With status 1 both are
 *             exact zeros (and the compact form below has no rows: every count is 0, every row_of_pixel is -1)
 *   C         2 <= C <= SSD_LOSS_MAX_CLASSES: a block of 128 logit rows (512 * C bytes as f32) and the 8 KB level-1 histogram
 *             of the mining threshold share the 160 KB of LDS of a workgroup; SSD_ERR_UNSUPPORTED (nothing launched) beyond
 * Hard-negative mining is global over the B images handed in (one micro-batch), as in the reference.
 * fp32 losses agree with a float64 evaluation to <= 1e-4 relative.
 * ---------------------------------------------------------------------------------------- */
#define SSD_LOSS_MAX_CLASSES 303
size_t ssd_loss_workspace_bytes(int B, int A, int C);
int ssd_loss_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls,
                     const float* gt_loc, const uint8_t* gt_mask, int B, int A, int C, float grad_scale,
                     float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes, void* stream);

/* The same loss with the gradient handed over in the form the head convolutions' backward pass consumes, instead of the
 * dense dconf / dloc.  Only the anchors the loss selects carry a gradient -- the positives and the mined negatives, 4P of
 * B*A rows (:355-380; every other row of tape.gradient's result is exactly zero) -- so per feature level l the gradient is
 * a COMPACT list of pixel rows: row r of level l is the head output gradient of pixel pixel_of_row[l][r] (flat index
 * b*hw + y*W + x, ascending in r), channels in the head GEMM's order [per_cell*4 loc | per_cell*C conf | zero pad to npad];
 * row_of_pixel[l][b*hw + pix] is the inverse map (-1: the pixel carries no gradient); count[l] rows are valid.  Scattered
 * back, the rows are bit-identical to ssd_loss_fwd_bwd's dconf / dloc (tests/test_sparse_heads_gpu.py).
 *   hg        HOST struct, device pointers inside; rows / maps sized for B*hw rows (every pixel selected)
 *   dtype     SSD_BF16 only
 *   ws        >= ssd_loss_heads_workspace_bytes(B, A, C) bytes
 *   ws_clean  0: the call clears its histogram words first (a memset node).  1: the caller states they are zero already -- they
 *             are after a COMPLETED call of this function on the same ws with the same B and A (the last launch re-zeroes
 *             them), and no other use of ws in between; a wrong 1 gives a wrong mining threshold, not a fault
 * Consumers: ssd_heads_bwd_data_sparse, ssd_heads_bwd_weight_sparse. */
typedef struct {
    int levels;                               /* <= SSD_MAX_LEVELS; sum of hw*per_cell over the levels == A          */
    int hw[SSD_MAX_LEVELS];                   /* pixels of a level's feature map (H*W)                              */
    int per_cell[SSD_MAX_LEVELS];             /* default boxes per pixel (:153)                                     */
    int npad[SSD_MAX_LEVELS];                 /* row length, >= per_cell*(4+C), multiple of 8                       */
    void* rows[SSD_MAX_LEVELS];               /* DEVICE bf16 [B*hw][npad]                                           */
    int32_t* row_of_pixel[SSD_MAX_LEVELS];    /* DEVICE int32 [B*hw]                                                */
    int32_t* pixel_of_row[SSD_MAX_LEVELS];    /* DEVICE int32 [B*hw]                                                */
    int32_t* count;                           /* DEVICE int32 [SSD_MAX_LEVELS]                                      */
} ssd_head_grads;
size_t ssd_loss_heads_workspace_bytes(int B, int A, int C);
int ssd_loss_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                           const uint8_t* gt_mask, int B, int A, int C, float grad_scale, float* out8,
                           const ssd_head_grads* hg, void* ws, size_t ws_bytes, int ws_clean, void* stream);

/* ------------------------------------------------------------------------------------------
 * The SSD paper's MultiBox loss (Liu et al. 2016, eq. 1-3), forward + backward.  Opt-in, no reference counterpart: the
 * loss above stays the default.  Inputs as ssd_loss_fwd_bwd.  With CE(a, c) = logsumexp(conf[a]) - conf[a, c] and
 * key(a) = CE(a, C-1):
 *   per image b: P_b positives (gt_mask); the candidates are the other anchors; k_b = min(neg_pos_ratio * P_b, A - P_b);
 *             k_b == 0 mines nothing, else tau_b = the k_b-th largest candidate key and neg_b = {candidates with
 *             key >= tau_b} (ties at tau_b kept; positives are excluded explicitly, so tau_b == 0 is legal)
 *   P = sum P_b, N = sum |neg_b|, smoothL1(d) = 0.5 d^2 if |d| < 1 else |d| - 0.5
 *   L_pos = sum_pos CE(a, gt_cls) / P;  L_neg = sum_neg key(a) / P;  L_loc = loc_weight * sum_pos sum_4 smoothL1(loc - gt_loc) / P
 *   dconf = grad_scale / P * [pos * (softmax - onehot(gt_cls)) + neg * (softmax - onehot(C-1))]
 *   dloc  = grad_scale * loc_weight / P * pos * clamp(loc - gt_loc, -1, 1);  every element of both is written
 *   out8      float[8]: L_loc, L_pos, L_neg, (L_loc + L_pos) + L_neg, P, N, tau_min (the smallest tau_b of the images that
 *             mined, 0 if none did), status (0 ok; 1 = P == 0: scalars 0, gradients exact zeros, the rows form has every
 *             count 0 and every row_of_pixel -1; 3 = a logit row or a positive's offsets were NaN / Inf, reported first)
 *   neg_pos_ratio >= 1, loc_weight finite and >= 0, grad_scale finite: SSD_ERR_VALUE otherwise, as for a NULL pointer, a
 *             dtype that is neither SSD_F32 nor SSD_BF16, B <= 0, A <= 0 or C < 2
 *   C         <= SSD_LOSS_MAX_CLASSES; A <= SSD_MULTIBOX_MAX_ANCHORS (= ssd_multibox_loss_max_anchors()): the select keeps one
 *             image's A keys (4 bytes each) next to its 8 KB digit histogram in the 160 KB of LDS of a workgroup;
 *             SSD_ERR_UNSUPPORTED beyond either bound
 *   ws        >= ssd_multibox_loss_workspace_bytes(B, A, C) bytes (SSD_ERR_WORKSPACE otherwise); needs NO initial contents:
 *             every word is written before it is read, no global atomics
 * Every refusal happens on the host before anything is launched.  The normaliser P is per call (one micro-batch or one
 * rank's shard), as the counts of the loss above are.  Deterministic: integer counts and fixed-order f64 sums only.
 * The _heads form hands the gradient over as the compact rows of ssd_loss_fwd_bwd_heads (same struct, same layout, same
 * refusals for `hg`; SSD_ERR_ASSERT when the levels do not sum to A): dtype SSD_BF16 only (SSD_F32: SSD_ERR_UNSUPPORTED);
 * ws >= ssd_multibox_loss_heads_workspace_bytes(B, A, C) bytes, no ws_clean (nothing is carried from call to call);
 * scattered back, the rows are bit-identical to the dense form's dconf / dloc.
 * ---------------------------------------------------------------------------------------- */
#define SSD_MULTIBOX_MAX_ANCHORS 36864
int ssd_multibox_loss_max_anchors(void);
size_t ssd_multibox_loss_workspace_bytes(int B, int A, int C);
int ssd_multibox_loss_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                              const uint8_t* gt_mask, int B, int A, int C, int neg_pos_ratio, float loc_weight,
                              float grad_scale, float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes,
                              void* stream);
size_t ssd_multibox_loss_heads_workspace_bytes(int B, int A, int C);
int ssd_multibox_loss_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                    const uint8_t* gt_mask, int B, int A, int C, int neg_pos_ratio, float loc_weight,
                                    float grad_scale, float* out8, const ssd_head_grads* hg, void* ws, size_t ws_bytes,
                                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Softmax focal loss (Lin et al. 2017, "Focal Loss for Dense Object Detection", over the network's C softmax logits),
 * forward + backward.  Opt-in, no reference counterpart.  Inputs as ssd_multibox_loss_fwd_bwd; nothing is mined: every anchor
 * stays in the classification term, weighted by (1 - p_t)^gamma.  Per anchor a, with t = gt_cls[a] where gt_mask[a] and C-1
 * elsewhere (gt_cls is not read on unmasked anchors), m = max_j z_j, e_j = exp(z_j - m), S = sum_j e_j, p_j = e_j / S:
 *   q = (sum_{j != t} e_j) / S  (= 1 - p_t, never evaluated as that difference);
 *   log p_t = log1p(-q) where q < 0.5, (z_t - m) - log S elsewhere (neither cancels on a confident row)
 *   FL(a) = -alpha_t * q^gamma * log p_t;  alpha_t = alpha for t != C-1, 1 - alpha for the background; alpha == -1: alpha_t = 1
 *   P = number of positives;  L_pos = sum_pos FL / P;  L_neg = sum_{not pos} FL / P;
 *   L_loc = loc_weight * sum_pos sum_4 smoothL1(loc - gt_loc) / P
 *   dconf[a, j] = grad_scale / P * alpha_t * (delta_tj - p_j) * (gamma * p_t * q^(gamma-1) * log p_t - q^gamma), evaluated in
 *             a form that is finite at q == 0, where FL and the row are 0
 *   dloc      ssd_multibox_loss_fwd_bwd's, bit for bit on the same inputs (one device function);  every element of both
 *             gradients is written
 *   out8      float[8]: L_loc, L_pos, L_neg, (L_loc + L_pos) + L_neg, P, N = B*A - P, 0, status (0 ok; 1 = P == 0: scalars 0,
 *             gradients exact zeros, the rows form has every count 0 and every row_of_pixel -1; 3 = a logit or a positive's
 *             offsets were NaN / Inf, reported first)
 *   gamma     finite, in [0, 8]; alpha in [0, 1] or -1; loc_weight finite and >= 0, grad_scale finite: SSD_ERR_VALUE
 *             otherwise, as for a NULL pointer, a dtype that is neither SSD_F32 nor SSD_BF16, B <= 0, A <= 0 or C < 2
 *   C         <= SSD_LOSS_MAX_CLASSES (a block of 128 logit rows as f32 in LDS): SSD_ERR_UNSUPPORTED beyond.  No bound on A:
 *             there is no per-image select
 *   ws        >= ssd_softmax_focal_loss_workspace_bytes(B, A, C) bytes (SSD_ERR_WORKSPACE otherwise); needs NO initial
 *             contents, no atomics
 * Every refusal happens on the host before anything is launched.  Three launches: the count of positives, one streaming pass
 * that reads each logit row once and writes its gradient once, the scalars.  Deterministic: integer counts and fixed-order
 * f64 sums of per-block partials.  fp32 losses agree with a float64 evaluation to <= 1e-4 relative, f32 dconf elementwise to
 * 1e-4 relative.
 * The _heads form hands the gradient over as the rows of ssd_loss_fwd_bwd_heads (same struct, same channel order and zero
 * padding, same refusals for `hg`; SSD_ERR_ASSERT when the levels do not sum to A).  Every anchor carries a gradient, so every
 * pixel is a row: row r of level l is pixel r, both maps are the identity and count[l] = B * hw[l] (the sparse head kernels
 * serve full density as they are).  dtype SSD_BF16 only (SSD_F32: SSD_ERR_UNSUPPORTED); scattered back, the rows are
 * bit-identical to the dense form's dconf / dloc.
 * ---------------------------------------------------------------------------------------- */
size_t ssd_softmax_focal_loss_workspace_bytes(int B, int A, int C);
int ssd_softmax_focal_loss_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                   const uint8_t* gt_mask, int B, int A, int C, float gamma, float alpha, float loc_weight,
                                   float grad_scale, float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes,
                                   void* stream);
size_t ssd_softmax_focal_loss_heads_workspace_bytes(int B, int A, int C);
int ssd_softmax_focal_loss_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                         const uint8_t* gt_mask, int B, int A, int C, float gamma, float alpha,
                                         float loc_weight, float grad_scale, float* out8, const ssd_head_grads* hg, void* ws,
                                         size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The box term of the two losses above by kind: smooth L1 of the four offsets (kind 0: the entries above, which forward here),
 * or the GIoU (Rezatofighi et al. 2019), DIoU or CIoU (Zheng et al. 2020) loss of the decoded boxes.  Opt-in, no reference
 * counterpart.  Arguments, results, refusals, workspaces and launches as the entry of the same name without _box, plus
 *   box_kind  SSD_BOX_SMOOTH_L1 | SSD_BOX_GIOU | SSD_BOX_DIOU | SSD_BOX_CIOU; anything else: SSD_ERR_VALUE
 *   priors    DEVICE double[A*4] (cx, cy, w, h), the array the matcher and ssd_score_decode read; may be NULL with kind 0, which
 *             does not read it; NULL with an IoU kind: SSD_ERR_VALUE.  Both refusals happen on the host before any launch
 * Per positive anchor a, prior d = priors[a], t = loc[a], g = gt_loc[a], W = log(1000 / 16), f32 arithmetic:
 *   decode    relative to the prior's centre (every kind is translation invariant; a small width is not cancelled against an
 *             absolute position):  cx = t0 d_w, cy = t1 d_h, w = d_w exp(clamp(t2, -W, W)), h = d_h exp(clamp(t3, -W, W));
 *             (gx, gy, gw, gh) from g in the same way;  x1 = cx - w/2, x2 = cx + w/2, ..., X1 = gx - gw/2, ...
 *   iw = max(0, min(x2, X2) - max(x1, X1)), ih likewise;  I = iw ih;  U = w h + gw gh - I;  IoU = I / U
 *   cw = max(x2, X2) - min(x1, X1), ch likewise
 *   GIoU      L = 1 - IoU + (cw ch - U) / (cw ch)
 *   DIoU      L = 1 - IoU + rho^2 / c^2,  rho^2 = (cx - gx)^2 + (cy - gy)^2,  c^2 = cw^2 + ch^2
 *   CIoU      L = DIoU + alpha v,  v = (4 / pi^2) (atan(gw / gh) - atan(w / h))^2,  alpha = v / ((1 - IoU) + v) where v > 0,
 *             else 0; alpha is a constant in the gradient, dv/dw and dv/dh are the true derivatives (the 1 / (w^2 + h^2) kept)
 *   no epsilons: with positive prior sizes and the clamp every denominator is positive
 *   dL/dt0 = d_w dL/dcx, dL/dt1 = d_h dL/dcy, dL/dt2 = w dL/dw where |t2| < W, else 0; t3 likewise
 *   ties      max(p, q) / min(p, q) pass the gradient to the predicted coordinate under the strict comparison only, max(0, .)
 *             where its argument is > 0
 *   L_loc = loc_weight * sum_pos L / P;  dloc = grad_scale * loc_weight / P * pos * dL/dt: every element is written, exact zeros
 *             off the positives;  P, N, tau, the classification terms and dconf are those of kind 0, bit for bit
 *   status    3 also where a positive's box loss or gradient is not finite (a prior with a size that is not positive, say)
 * Both losses evaluate one device function: their dloc agree bit for bit on the same inputs, as for kind 0.  f32 losses agree
 * with a float64 evaluation to <= 1e-4 relative, f32 dloc per anchor to 1e-4 of the anchor's largest component.
 * ---------------------------------------------------------------------------------------- */
#define SSD_BOX_SMOOTH_L1 0
#define SSD_BOX_GIOU 1
#define SSD_BOX_DIOU 2
#define SSD_BOX_CIOU 3
int ssd_multibox_loss_box_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                  const uint8_t* gt_mask, int B, int A, int C, int neg_pos_ratio, float loc_weight,
                                  float grad_scale, float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes,
                                  void* stream, int box_kind, const double* priors);
int ssd_multibox_loss_box_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                        const uint8_t* gt_mask, int B, int A, int C, int neg_pos_ratio, float loc_weight,
                                        float grad_scale, float* out8, const ssd_head_grads* hg, void* ws, size_t ws_bytes,
                                        void* stream, int box_kind, const double* priors);
int ssd_softmax_focal_loss_box_fwd_bwd(const void* conf, const void* loc, int dtype, const int32_t* gt_cls, const float* gt_loc,
                                       const uint8_t* gt_mask, int B, int A, int C, float gamma, float alpha, float loc_weight,
                                       float grad_scale, float* out8, void* dconf, void* dloc, void* ws, size_t ws_bytes,
                                       void* stream, int box_kind, const double* priors);
int ssd_softmax_focal_loss_box_fwd_bwd_heads(const void* conf, const void* loc, int dtype, const int32_t* gt_cls,
                                             const float* gt_loc, const uint8_t* gt_mask, int B, int A, int C, float gamma,
                                             float alpha, float loc_weight, float grad_scale, float* out8,
                                             const ssd_head_grads* hg, void* ws, size_t ws_bytes, void* stream, int box_kind,
                                             const double* priors);

/* ------------------------------------------------------------------------------------------
 * Inference scoring + decode -- replaces the scoring half of SSDObjectDetectionModel.visualize
 * (models/ssd_model.py:479-488, mask=None branch) and the box decode of visualize_dataset (:466-467).
 *   conf [B*A*C], loc [B*A*4] (SSD_F32 / SSD_BF16), priors double[A*4]
 *   score  float[B*A]  best non-background softmax probability
 *   cls    int32[B*A]  its class (== argmax over all classes wherever cand is set)
 *   box    float[B*A*4] decoded (cx,cy,w,h) in pixels (in_size = 300) for candidates, 0 elsewhere
 *   cand   uint8[B*A]  score > score_thresh && !(p_background > score_thresh)
 * cls is written for every row (the first index among equal maxima), not only for candidates.  A block of 128 rows of C
 * floats is staged in dynamic LDS and must fit 150 KiB: C <= 300, SSD_ERR_UNSUPPORTED (nothing launched, nothing written)
 * beyond; ssd_class_scores and ssd_detect_pairs share the bound.  Launches above 64 KiB (C >= 129) are granted without a
 * hipFuncAttributeMaxDynamicSharedMemorySize registration (tests/test_detect_strict_gpu.py runs C = 129, 300 and 301).
 * ---------------------------------------------------------------------------------------- */
int ssd_score_decode(const void* conf, const void* loc, int dtype, const double* priors, int B, int A, int C,
                     float score_thresh, double in_size, float* score, int32_t* cls, float* box,
                     uint8_t* cand, void* stream);

/* Per-image, per-class greedy hard NMS.  The reference has NO suppression step; this
 * entry point is build-defined and its oracle is oracle/ssd_oracle.py:nms.  Candidates (cand != 0) are
 * ordered by (score desc, anchor asc); the first max_cand (<= ssd_nms_max_candidates()) take part; a
 * candidate is kept iff its IoU -- the reference's scalar iou (utils/bbox.py:6-25) evaluated in float32 --
 * with every already kept candidate of its class is <= iou_thresh.
 *   keep uint8[B*A] (fully written), keep_count int32[B] or NULL.  Bit-exact against the oracle. */
int ssd_nms_max_candidates(void);
int ssd_nms(const float* score, const int32_t* cls, const float* box, const uint8_t* cand, int B, int A,
            float iou_thresh, int max_cand, uint8_t* keep, int32_t* keep_count, void* stream);

/* Multi-label detection output (build-defined; the SSD detection-output protocol: every (anchor, class) pair is scored, an
 * anchor may be reported under several classes).  Per image, F = C-1 foreground classes, background = class C-1:
 *   1. p[a][c], c < F: float32 softmax probability (row maximum subtracted, __expf, fixed summation order).  One device
 *      function computes it for both entry points: the score bits ssd_detect_pairs reports equal what ssd_class_scores
 *      writes for the same pair.  (Not necessarily bit-equal to ssd_score_decode's score.)
 *   2. pair (a, c) is a candidate iff p[a][c] > score_thresh.  There is NO background test: the reference's
 *      `p_background <= thresh` rule belongs to the single-label path (ssd_score_decode) only.
 *   3. candidates are ordered by (score desc, anchor asc, class asc); only the first max_cand take part
 *      (1 <= max_cand <= ssd_detect_max_candidates()).  The cut is exact for every input, score ties included.
 *   4. a participating anchor is decoded as ssd_score_decode does it (float64, stored as float32 cx, cy, w, h).
 *   5. in that order a pair is kept iff its IoU (ssd_nms's float32 IoU) with every already kept pair OF ITS CLASS is
 *      <= iou_thresh.
 *   6. the kept pairs, in the same order, cut to the first keep_top_k (1 <= keep_top_k <= ssd_detect_max_keep()) = K rows.
 *   n_cand int32[B]  pairs above the threshold before the cut (exact); n_det int32[B] rows that hold a detection;
 *   det_score float[B*K], det_cls int32[B*K], det_anchor int32[B*K], det_box float[B*K*4], det_valid uint8[B*K]:
 *   rows at or beyond n_det hold score 0, class -1, anchor -1, box 0, valid 0 (ssd_eval_match's convention).  Every output
 *   element is written on every call.  ws: ssd_detect_pairs_workspace_bytes(B, A, C) bytes, no initial contents needed.
 * ssd_class_scores: step 1 alone, prob float[B*A*(C-1)] dense.
 * dtype SSD_F32 / SSD_BF16; 1 <= A <= 65536, 2 <= C <= 65536, A*(C-1) < 2^31.  Before any launch: SSD_ERR_VALUE for a NULL
 * pointer, B / A / C, max_cand or keep_top_k out of range; SSD_ERR_WORKSPACE for a short ws. */
int ssd_detect_max_candidates(void);
int ssd_detect_max_keep(void);
int ssd_class_scores(const void* conf, int dtype, int B, int A, int C, float* prob, void* stream);
size_t ssd_detect_pairs_workspace_bytes(int B, int A, int C);
int ssd_detect_pairs(const void* conf, const void* loc, int dtype, const double* priors, int B, int A, int C,
                     float score_thresh, double in_size, float iou_thresh, int max_cand, int keep_top_k, int32_t* n_cand,
                     int32_t* n_det, float* det_score, int32_t* det_cls, int32_t* det_anchor, float* det_box,
                     uint8_t* det_valid, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation metric on the device (no reference counterpart: the reference fetches its validation split at
 * models/ssd_model.py:291 and drops it).  Build-defined; the definition and oracle is utils/metrics.py:coco_map -- COCO
 * AP@[.50:.05:.95] for boxes without crowd regions or area ranges.
 *
 * ssd_eval_match: one launch per evaluated batch, consuming what ssd_score_decode + ssd_nms leave in memory.
 *   score float[B*A], cls int32[B*A], box float[B*A*4] (cx,cy,w,h pixels), keep uint8[B*A]
 *   gt_cls int32[total_gt], gt_box double[total_gt*4] (cx,cy,w,h pixels), gt_off int32[B+1] (CSR, as ssd_match_encode);
 *          gt_cls / gt_box may be NULL when gt_off[B] == 0.  Any number of boxes per image.
 *   iou_thresholds HOST double[10] (np.linspace(0.5, 0.95, 10): passed in, not recomputed)
 *   max_dets  1 .. ssd_eval_max_dets() (128)
 * Per image: the kept anchors ordered by (score desc, anchor asc), cut to the first max_dets; then per threshold and class
 * the detections in that order each claim, among the image's still-unclaimed boxes of their class, the one with the highest
 * IoU >= threshold, the LAST index winning among equal IoUs.  IoU is utils/metrics.py:iou_matrix in float64, operation for
 * operation, without fused multiply-adds: flags are bit-exact against the definition.
 *   n_det int32[B]; det_score float[B*max_dets], det_cls int32[B*max_dets], det_box float[B*max_dets*4],
 *   det_flags uint16[B*max_dets] (bit t: true positive at threshold t).  All fully written; slots at or beyond n_det hold
 *   score 0, class -1, box 0, flags 0.
 *
 * ssd_eval_ap: after the last batch, from all rows sorted by (class asc, score desc, image asc, rank asc).
 *   flags_sorted uint16[N] (not NULL, even for N = 0), seg_off int32[C+1] (class c owns rows seg_off[c] .. seg_off[c+1]-1),
 *   n_gt int32[C] ground truths per class, recall_points HOST double[101] (np.linspace(0, 1, 101))
 *   ap double[C*10]: 101-point interpolated AP per (class, threshold) -- cumulative TP / FP, recall = ctp / n_gt, precision
 *   = ctp / max(ctp + cfp, 1) made monotone from the right, sampled at the first index whose recall >= each point (0 where
 *   none), mean of the samples summed in numpy's pairwise order.  0 for classes with n_gt == 0 (the caller leaves them out
 *   of its means) and for classes without detections.  Segments of any length.
 * Both return SSD_ERR_VALUE before any launch for B <= 0, A <= 0, C <= 0, max_dets out of range or a NULL pointer.
 *
 * The full COCO box protocol -- area ranges, crowd boxes, average recall -- is a second pair of entry points beside those two;
 * its definition and oracle is utils/metrics.py:coco_summary (coco_match_image for the first stage, coco_tables_from_rows for
 * the second).  ssd_eval_match and ssd_eval_ap are unchanged by it.
 *
 * ssd_eval_match_coco: ssd_eval_match's inputs, and
 *   gt_crowd uint8[total_gt]  non-zero: a crowd region; NULL: none
 *   area_scale double[B]      per image (source width x source height) / (S x S); NULL: 1
 *   area_ranges HOST double[8]  (lo, hi) of the four ranges all / small / medium / large, bounds inclusive
 * The selection and order of the detections are ssd_eval_match's.  The area of a box, detection or ground truth, is
 * double(w) * double(h) * area_scale[image], left to right, without fused multiply-adds.  A ground truth is ignored in range a
 * when it is crowd or its area is < lo[a] or > hi[a].  IoU against a crowd box is intersection / area of the detection (the
 * corner-form area iou_matrix computes; 0 where it is not positive).  Per class, range and threshold the detections in order
 * each take the unclaimed non-ignored box of their class with the highest IoU >= threshold, the LAST index winning among equal
 * IoUs, and only when there is none an ignored one by the same rule, where a crowd box may be claimed again.  A matched
 * detection is a true positive and inherits the ignore flag of its match; an unmatched one is ignored when its own area is
 * outside the range.
 *   n_det, det_score, det_cls, det_box  as ssd_eval_match
 *   det_flags uint16[B*max_dets]    bit t: true positive at threshold t and not ignored, in range 0 -- ssd_eval_match's flags
 *                                   when no box is crowd and range 0 holds every area
 *   det_tp uint16[B*max_dets*4]     [image][slot][range], bit t: true positive at threshold t
 *   det_ig uint16[B*max_dets*4]     [image][slot][range], bit t: ignored at threshold t
 *   det_pos int32[B*max_dets]       rank of the detection among its image's detections of its class
 *   gt_ignore uint8[total_gt]       bit a: ignored in range a (NULL allowed when gt_off[B] == 0)
 * All fully written (gt_ignore: the boxes gt_off covers); slots at or beyond n_det hold zeros (class -1).  Images with more
 * than 48 ground truths take a path without the IoU cache, with identical results; any number of boxes per image.
 *
 * ssd_eval_ap_coco: after the last batch, a grid of (class, range), from rows sorted as for ssd_eval_ap.
 *   tp_sorted, ig_sorted uint16[N*4] ([row][range]; not NULL, even for N = 0), pos_sorted int32[N], seg_off int32[C+1],
 *   n_gt int32[4*C] ([range][class]: ground truths not ignored in the range), max_dets 1 .. ssd_eval_max_dets(),
 *   recall_points HOST double[101]
 *   ap double[C*4*10]  [class][range][threshold]: ssd_eval_ap's AP over the rows whose ignore bit is clear -- the row index is
 *                      the running count of such rows, a true positive counts when its ignore bit is clear
 *   tp_count int32[C*4*3*10]  [class][range][m][threshold]: true positives not ignored with pos < (1, 10, max_dets)[m]
 *   Both are 0 where n_gt == 0 (the caller leaves the class out of that range's means).
 * Both return SSD_ERR_VALUE before any launch on the conditions of ssd_eval_match / ssd_eval_ap.
 *
 * PASCAL VOC (VOCdevkit's VOCevaldet) is a third pair; its definition and oracle is utils/metrics.py:voc_map (voc_match_image
 * for the first stage, voc_ap_from_rows for the second).  It is not a special case of the pairs above: there is one IoU
 * threshold and no greedy pass.
 *
 * ssd_eval_match_voc: ssd_eval_match's inputs without the threshold table, and
 *   gt_difficult uint8[total_gt]  non-zero: a `difficult` box; NULL: none
 *   iou_thresh   one threshold, finite and > 0 (VOC: 0.5)
 *   max_dets     1 .. ssd_eval_voc_max_dets() (256: SSD's detection output keeps 200 per image)
 * The selection and order of the detections are ssd_eval_match's.  Per detection, over ALL boxes of its class in its image,
 * claimed or not, difficult ones included: ovmax = the highest IoU (iou_matrix in float64, continuous coordinates: VOCdevkit's
 * +1 pixel convention is not applied), jmax = the FIRST index attaining it.  When ovmax >= iou_thresh: the detection is ignored
 * if box jmax is difficult; else a true positive if no detection before it in the order has the same jmax with its own ovmax >=
 * iou_thresh; else a false positive (a duplicate, even where a second box would also pass).  Otherwise a false positive.
 *   n_det, det_score, det_cls, det_box  as ssd_eval_match
 *   det_flags uint8[B*max_dets]   bit 0: true positive, bit 1: ignored
 *   det_gt int32[B*max_dets]      jmax as an index into the image's boxes, -1 when ovmax < iou_thresh or there is no box
 * All fully written; slots at or beyond n_det hold score 0, class -1, box 0, flags 0, det_gt -1.  Images with more than 64
 * ground truths take a path without the per-box LDS arrays, with identical results; any number of boxes per image.
 *
 * ssd_eval_ap_voc: after the last batch, one workgroup per class, from rows sorted as for ssd_eval_ap.
 *   flags_sorted uint8[N] (not NULL, even for N = 0; a row whose bit 1 is set counts as neither true nor false positive),
 *   seg_off int32[C+1], n_pos int32[C] (non-difficult boxes per class), year 7 or 12,
 *   recall_points HOST double[11] (np.arange(11) / 10.0: passed in, not recomputed)
 *   ap double[C]: with ctp / cfp the cumulative counts, recall = ctp / n_pos, precision = ctp / max(ctp + cfp, 1):
 *     year 7:  (sum over k = 0..10, added in that order, of max{precision[i] : recall[i] >= recall_points[k]}, 0 where none) / 11.0
 *     year 12: mrec = [0, recall, 1], mpre = [0, precision, 0] made monotone from the right; the sum, in index order, of
 *              (mrec[i+1] - mrec[i]) * mpre[i+1] where mrec[i+1] != mrec[i]
 *   0 where n_pos <= 0 (the caller leaves the class out of its mean) or the class has no rows.  Segments of any length.
 * Both return SSD_ERR_VALUE before any launch on the conditions of ssd_eval_match / ssd_eval_ap, and for a year other than 7 or
 * 12 or an iou_thresh that is not finite or not > 0.
 * ---------------------------------------------------------------------------------------- */
int ssd_eval_max_dets(void);
int ssd_eval_match(const float* score, const int32_t* cls, const float* box, const uint8_t* keep, int B, int A,
                   const int32_t* gt_cls, const double* gt_box, const int32_t* gt_off, const double* iou_thresholds,
                   int max_dets, int32_t* n_det, float* det_score, int32_t* det_cls, float* det_box, uint16_t* det_flags,
                   void* stream);
int ssd_eval_ap(const uint16_t* flags_sorted, const int32_t* seg_off, const int32_t* n_gt, int C, const double* recall_points,
                double* ap, void* stream);
int ssd_eval_match_coco(const float* score, const int32_t* cls, const float* box, const uint8_t* keep, int B, int A,
                        const int32_t* gt_cls, const double* gt_box, const int32_t* gt_off, const uint8_t* gt_crowd,
                        const double* area_scale, const double* area_ranges, const double* iou_thresholds, int max_dets,
                        int32_t* n_det, float* det_score, int32_t* det_cls, float* det_box, uint16_t* det_flags, uint16_t* det_tp,
                        uint16_t* det_ig, int32_t* det_pos, uint8_t* gt_ignore, void* stream);
int ssd_eval_ap_coco(const uint16_t* tp_sorted, const uint16_t* ig_sorted, const int32_t* pos_sorted, const int32_t* seg_off,
                     const int32_t* n_gt, int C, int max_dets, const double* recall_points, double* ap, int32_t* tp_count,
                     void* stream);
int ssd_eval_voc_max_dets(void);
int ssd_eval_match_voc(const float* score, const int32_t* cls, const float* box, const uint8_t* keep, int B, int A,
                       const int32_t* gt_cls, const double* gt_box, const int32_t* gt_off, const uint8_t* gt_difficult,
                       double iou_thresh, int max_dets, int32_t* n_det, float* det_score, int32_t* det_cls, float* det_box,
                       uint8_t* det_flags, int32_t* det_gt, void* stream);
int ssd_eval_ap_voc(const uint8_t* flags_sorted, const int32_t* seg_off, const int32_t* n_pos, int C, int year,
                    const double* recall_points, double* ap, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution stack (NHWC bf16 activations, bf16 weights [Cout][k][k][Cin], fp32 accumulate on MFMA).
 * Replaces the TensorFlow kernels behind SSDObjectDetectionModel._build (models/ssd_model.py:74-171)
 * and behind tape.gradient (:248) for those layers.  TF "SAME" padding is passed explicitly:
 * pad_total = max((Ho-1)*stride + k - H, 0), pad_t = pad_total/2 (the remainder goes after).
 * Channel counts of activation tensors must be multiples of 8 (the 3-channel image is expanded to 8
 * zero-padded channels by ssd_image_prep).
 * (ws, ws_bytes) of the forward / data-gradient calls is OPTIONAL scratch (may be NULL/0): when given, skinny
 * problems (few output tiles, long reduction) are split over k with a fixed-order fp32 reduction; a few MB suffice
 * (ksplit * B*Ho*Wo * Cout * 4 bytes, only used when the layer has < 160 output tiles).
 * ---------------------------------------------------------------------------------------- */
/* y[B,Ho,Wo,Cout] = relu?(conv(x[B,H,W,Cin], w) + bias)          Conv2D, :86-151 and the VGG blocks :77-82 */
int ssd_conv2d_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin,
                   int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int relu, void* ws,
                   size_t ws_bytes, void* stream);
/* Conv2D + bias + ReLU followed by MaxPool2D 2x2 / stride 2 (models/ssd_model.py:77-84: block1_conv2 -> block1_pool etc.):
 * y as ssd_conv2d_fwd, y_pool [B,Hp,Wp,Cout] and pool_code as ssd_maxpool2x2_fwd_argmax of y.  Layers served by a
 * 16-wide block kernel pool the tile they already hold on chip; otherwise two launches.  Cout % 8 == 0.
 * y may be NULL when nothing but the pooling reads the full-resolution map (true for every pooled layer of the SSD300
 * trunk: the backward pass needs the pooled map and the winner codes only): the fused kernels then skip that store
 * (half of block1_conv2's traffic); a layer shape they do not serve returns SSD_ERR_VALUE before anything is launched. */
int ssd_conv2d_fwd_pool(const void* x, const void* w, const float* bias, void* y, void* y_pool, void* pool_code, int B, int H,
                        int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int relu, int Hp,
                        int Wp, void* ws, size_t ws_bytes, void* stream);
/* One pyramid level's loc+conf heads as ONE 3x3 SAME GEMM (N = per_cell*(4+classes); weight rows: loc filters
 * then conf filters), written straight into the concatenated outputs loc[B,A,4] / conf[B,A,classes]
 * (:155-167: the Reshape + Concatenate are the store addressing). */
int ssd_conv2d_head_fwd(const void* x, const void* w, const float* bias, void* loc, void* conf, int B, int H, int W,
                        int Cin, int per_cell, int classes, int anchors_total, int level_off, void* ws, size_t ws_bytes,
                        void* stream);
/* dx[B,H,W,Cin] (+)= conv_transpose(dy[B,Ho,Wo,Cout_pad], w_t), then zeroed where relu_src <= 0 (relu_src =
 * the forward activation stored in dx's place, or NULL).  w_t from ssd_weight_transpose. */
int ssd_conv2d_bwd_data(const void* dy, const void* w_t, const void* relu_src, void* dx, int B, int H, int W, int Cin,
                        int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int accumulate,
                        void* ws, size_t ws_bytes, void* stream);

/* ReLU sign bits.  ssd_conv2d_fwd_relubits = ssd_conv2d_fwd (relu = 1) that also writes one byte per pixel and 8 output
 * channels (bit k: channel 8c + k > 0), relu_bits [B*Ho*Wo][Cout/8]; ssd_conv2d_bwd_data_bits = ssd_conv2d_bwd_data with
 * its ReLU mask read from such bytes instead of the bf16 activation (relu_src): identical results, 16x fewer mask bytes --
 * re-reading whole activations for their sign cost the data gradients 13-130 us each.  Written / read in the staged store
 * of the kernels (and by the image-layer kernel): SSD_ERR_UNSUPPORTED, nothing launched, where a call resolves to a kernel
 * without it (split-K + finalize, scattered epilogues) -- use the plain functions there. */
int ssd_conv2d_fwd_relubits(const void* x, const void* w, const float* bias, void* y, void* relu_bits, int B, int H, int W, int Cin,
                            int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, void* ws, size_t ws_bytes,
                            void* stream);
int ssd_conv2d_bwd_data_bits(const void* dy, const void* w_t, const void* relu_bits, void* dx, int B, int H, int W, int Cin,
                             int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, int accumulate, void* ws,
                             size_t ws_bytes, void* stream);
/* Second layer's data gradient and first layer's weight gradient in ONE launch (block1_conv2 / block1_conv1 of the VGG-16
 * trunk, models/ssd_model.py:62-66): the gradient w.r.t. the first layer's output has a single consumer, the 3-channel first
 * layer's weight gradient, so it is multiplied with the image patch where it is produced and never stored -- equal to
 *   ssd_conv2d_bwd_data_bits(dy, w_t, relu_bits, dx, B,H,W, 64, 64, 3,1,1,1, H,W, 0, ...)  followed by
 *   ssd_conv2d_bwd_weight(image, dx, dw0, dbias0, B,H,W, 8, 64, 64, 3,1,1,1, H,W, ...)
 * up to fp32 summation order (dx is rounded to bf16 in both).  dy [B,H,W,64] bf16; w_t [64][3][3][64] (ssd_weight_transpose
 * of the second layer); relu_bits [B*H*W][8] (ssd_conv2d_fwd_relubits of the first layer); image [B,H,W,8] bf16
 * (ssd_image_prep); dw0 f32 [64][3][3][8] (columns of the five pad channels: zeros); dbias0 f32 [64] or NULL.  Fixed summation
 * order (one slab per workgroup in ws, reduced in order): bitwise reproducible.  H, W >= 16. */
size_t ssd_conv2d_bwd_data_wgrad_first_workspace_bytes(int B, int H, int W);
int ssd_conv2d_bwd_data_wgrad_first(const void* dy, const void* w_t, const void* relu_bits, const void* image, float* dw0,
                                    float* dbias0, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
/* The 3x3 / stride 1 / pad 1 data gradient w.r.t. a POOLED map [B,H,W,Cin], carried on through the 2x2 / stride-2 max
 * pooling that produced the map: dx_full[B,Hf,Wf,Cin] = ssd_maxpool2x2_bwd_argmax(pool_code, ssd_conv2d_bwd_data(...)) in
 * one launch, bit-identical (the un-pooling runs in the convolution's store stage: no pooled gradient in HBM, no second
 * kernel).  Served by the LDS-patch kernels only: SSD_ERR_UNSUPPORTED (nothing launched) for any other layer shape --
 * call the two functions then.  H = Hf/2 or (Hf+1)/2, W likewise (VALID / SAME pooling); VALID pooling of an odd Hf or Wf
 * (2 H < Hf or 2 W < Wf) is SSD_ERR_UNSUPPORTED as well: the row / column that no window covers would not be written.
 * dx_pooled (may be NULL): also receives the gradient w.r.t. the pooled map itself [B,H,W,Cin] -- the compressed form
 * ssd_conv2d_bwd_weight_unpooled reads. */
int ssd_conv2d_bwd_data_unpool(const void* dy, const void* w_t, const void* relu_src, const void* pool_code, void* dx_pooled,
                               void* dx_full, int B, int H, int W, int Cin, int Cout_pad, int Hf, int Wf, void* ws, size_t ws_bytes,
                               void* stream);
/* Weight gradient of a 3x3 / stride 1 / pad 1 convolution whose output is 2x2 / stride-2 max-pooled (block1_conv2, block2_conv2,
 * block3_conv3: models/ssd_model.py:77-84), from the gradient of the POOLED map dpool [B,Hp,Wp,Cout] and the pooling's winner codes
 * pool_code [B,Hp,Wp,Cout/8] (ssd_maxpool2x2_fwd_argmax / ssd_conv2d_fwd_pool):
 *   == ssd_conv2d_bwd_weight(x, ssd_maxpool2x2_bwd_argmax(pool_code, dpool), ...)   up to fp32 summation order,
 * without multiplying the three zeros of every pooling window: the window's four pixels are four consecutive k of a
 * structured-sparse MFMA (v_smfmac_f32_16x16x64_bf16), the pooled gradient is the compressed operand, the code its index.
 * Cin, Cout multiples of 64, H, W >= 16, Hp = H/2 or (H+1)/2 (VALID / SAME pooling); SSD_ERR_UNSUPPORTED otherwise (nothing
 * launched).  Deterministic (fixed-order split reduction). */
size_t ssd_conv2d_bwd_weight_unpooled_workspace_bytes(int B, int H, int W, int Cin, int Cout, int Hp, int Wp);
int ssd_conv2d_bwd_weight_unpooled(const void* x, const void* dpool, const void* pool_code, float* dw, float* dbias, int B, int H,
                                   int W, int Cin, int Cout, int Hp, int Wp, void* ws, size_t ws_bytes, void* stream);
/* dw f32 [Cout][k][k][Cin], dbias f32 [Cout] (or NULL) from x[B,H,W,Cin] and dy[B,Ho,Wo,ldy] (first Cout
 * channels).  Deterministic (fixed-order split reduction). */
size_t ssd_conv2d_bwd_weight_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int ldy, int ksize);
int ssd_conv2d_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, int B, int H, int W, int Cin,
                          int Cout, int ldy, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo, void* ws,
                          size_t ws_bytes, void* stream);
/* Several small layers' weight gradients in two launches instead of two per layer (the extras on the 10x10 ... 1x1 maps,
 * models/ssd_model.py:124-150): arguments per layer as ssd_conv2d_bwd_weight.  Served: layers that call would run on its
 * generic kernel with fewer than 32 pixel splits, at most 8 per call; SSD_ERR_UNSUPPORTED otherwise, nothing launched.
 * Bit-identical to the separate calls (same blocks, same slabs, same fixed-order sums). */
typedef struct {
    const void* x;
    const void* dy;
    float* dw;
    float* dbias;
    int B, H, W, Cin, Cout, ldy, ksize, stride, pad_t, pad_l, Ho, Wo;
} ssd_wgrad_item;
size_t ssd_conv2d_bwd_weight_batched_workspace_bytes(const ssd_wgrad_item* items, int count);
int ssd_conv2d_bwd_weight_batched(const ssd_wgrad_item* items, int count, void* ws, size_t ws_bytes, void* stream);
/* w bf16 [Cout][k][k][Cin] -> w_t bf16 [Cin][k][k][Cout_pad], spatially flipped (data-gradient operand) */
int ssd_weight_transpose(const void* w, void* w_t, int Cout, int ksize, int Cin, int Cout_pad, void* stream);
/* the same for `ntensors` weight tensors in one launch: desc = device array of int64 rows {w, w_t, Cout, ksize, Cin,
 * Cout_pad} (device addresses and sizes), max_tiles = max over tensors of ceil(Cout_pad/32)*ceil(Cin/32)*ksize^2 */
int ssd_weight_transpose_batched(const long long* desc, int ntensors, int max_tiles, void* stream);
int ssd_cast_bf16(const float* src, void* dst, long long n, void* stream);
/* image f32 [B,H,W,3] -> bf16 [B,H,W,8]; normalize != 0 applies (x-0.5)*2 (models/ssd_model.py:214) */
int ssd_image_prep(const float* img, void* out, int B, int H, int W, int normalize, void* stream);
/* Input pipeline on the device for a ragged batch of decoded uint8 RGB images: '/255'
 * (data_loaders/coco/make_dataset.py:117), cv2.resize(image, (S, S)) with its default INTER_LINEAR
 * (data_loaders/ssd/make_dataset.py:40) and, if normalize != 0, (x-0.5)*2 (models/ssd_model.py:214) -> bf16 [B,S,S,8].
 * src: the images back to back (H x W x 3 bytes each), src_off int64 [B] byte offset of each image, src_hw int32 [B][2]. */
int ssd_image_resize_prep(const void* src, const int64_t* src_off, const int32_t* src_hw, void* out, int B, int S,
                          int normalize, void* stream);
/* Ground-truth boxes of the same batch: COCO [x, y, w, h] in pixels (top-left) -> centre form (coco/make_dataset.py:132)
 * divided by the image size (ssd/make_dataset.py:43-44).  gt_off int32 [B+1] as in ssd_match_encode. */
int ssd_box_prep(const float* box_tlwh, const int32_t* gt_off, const int32_t* src_hw, float* box_out, int B, int total_gt,
                 void* stream);

/* ------------------------------------------------------------------------------------------
 * SSD data augmentation for training batches (no reference counterpart: the reference trains without augmentation; this
 * follows SSD, Liu et al. ECCV 2016 section 3.2, as Caffe-SSD / ssd.pytorch's SSDAugmentation without its channel swap).
 * Opt-in; tests/augment_oracle.py restates every operation below in numpy, in the same float32 order.
 *
 * Recipe, per image, in this order.  All float arithmetic is float32, one rounding per operation, no fused multiply-add;
 * clamp(x) = min(max(x, 0), 1).
 *  1. PHOTO, photometric distortion of the source pixels, as values in [0,1] (uint8 / 255 or the f32 source):
 *       brightness (photo bit 1):  x = clamp(x + delta)
 *       contrast   (bit 2), before the HSV step when bit 4 is set, after it otherwise:  x = clamp(x * alpha)
 *       HSV step, only when saturation (bit 8) or hue (bit 16) is on:
 *         v = max(r,g,b), m = min(r,g,b), d = v - m;  s = v > 0 ? d / v : 0
 *         h = d == 0 ? 0 : v == r ? 60 * ((g - b) / d) : v == g ? 120 + 60 * ((b - r) / d) : 240 + 60 * ((r - g) / d)
 *         (ties to r, then g);  h < 0 -> h + 360
 *         saturation: s = clamp(s * saturation);  hue: h = h + hue, then h >= 360 -> h - 360, h < 0 -> h + 360
 *         back: q6 = h / 60, i = floor(q6), f = q6 - i, i == 6 -> 0 (h may round to 360);
 *               p = v * (1 - s), q = v * (1 - s * f), t = v * (1 - s * (1 - f));
 *               sector 0..5 -> (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q); each channel clamped
 *  2. EXPAND (zoom out): canvas (canvas_w, canvas_h) = ((int)(ratio * W), (int)(ratio * H)), the image at integer offset
 *     (off_x, off_y) drawn uniformly in [0, canvas - size]; everything else is the SSD mean (123, 117, 104) / 255 (double
 *     division rounded to float32), not distorted.  Without expand the canvas is the image.
 *  3. CROP: mode drawn uniformly from 0..6 = whole image, minimum IoU 0.1 / 0.3 / 0.5 / 0.7 / 0.9, any patch.  For a mode
 *     other than 0 and an image with at least one box, trials t = 0..49: patch_w = clamp_int((int)(sw * canvas_w), 1,
 *     canvas_w) with sw = 0.3 + u * 0.7 (patch_h likewise, own draw), rejected unless 2 * patch_h >= patch_w and
 *     patch_h <= 2 * patch_w, origin drawn uniformly in [0, canvas - patch].  In canvas pixels a box is
 *         x1 = (cx - w * 0.5) * W + off_x,  x2 = (cx + w * 0.5) * W + off_x,  centre ccx = cx * W + off_x  (y likewise)
 *     and its IoU with the patch [px, px + pw) x [py, py + ph) is
 *         iw = max(min(x2, px + pw) - max(x1, px), 0), inter = iw * ih, iou = inter / (((x2 - x1) * (y2 - y1) + pw * ph) - inter)
 *     A trial is accepted when some box has iou >= the mode's minimum (mode 6: no such condition) and some box centre lies
 *     strictly inside the patch; the first accepted trial wins, none means no crop (patch = whole canvas).
 *     Boxes: with a crop, those whose centre lies strictly inside the patch are kept, in input order; without one, all.
 *     When EXPAND or CROP took effect every kept box is clipped to the patch and made relative to it:
 *         rx1 = (max(x1, px) - px) / pw,  rx2 = (min(x2, px + pw) - px) / pw,  cx = (rx1 + rx2) * 0.5,  w = rx2 - rx1
 *     otherwise it passes through unchanged.
 *  4. FLIP: the output grid is mirrored (output column x reads column S-1-x of the resized patch); cx = 1 - cx.
 *  5. Resize of the patch to S x S with the INTER_LINEAR rule of ssd_image_resize_prep (scale = patch size / S in double),
 *     taps clamped inside the patch, horizontal pass first; each tap is the fill or a distorted source pixel.  Then
 *     (x-0.5)*2 if normalize, bf16 [B,S,S,8] with channels 3..7 zero.
 * Stage mask bits: SSD_AUG_PHOTO 1, SSD_AUG_EXPAND 2, SSD_AUG_CROP 4, SSD_AUG_FLIP 8.  Mask 0 is the identity:
 * ssd_image_resize_prep + ssd_box_prep for uint8 sources, (x-0.5)*2 + ssd_image_prep for f32 sources of size S x S.
 *
 * Randomness: Philox-4x32-10 (Random123), key = (seed low word, seed high word), counter = (index low word, index high word,
 * slot, block) with index = first_index + b, the sample's position in the training stream.  u = word >> 8 scaled by 2^-24
 * is uniform in [0,1); U(lo, hi) = lo + u * (hi - lo); a coin is word >> 31 (1 = apply); an integer in [0, n) is
 * (word * n) >> 32 in 64 bits.  Slots:
 *     0  photometric  block 0: brightness coin, delta = (-32 + u * 64) / 255, contrast coin, alpha = 0.5 + u
 *                     block 1: contrast-first coin, saturation coin, saturation = 0.5 + u, hue coin
 *                     block 2: hue = -18 + u * 36 (degrees)
 *     1  expand       coin, ratio = 1 + u * 3, off_x, off_y
 *     2  mode, flip coin
 *     3 + t  crop trial t: sw, sh, px, py
 * A trial's numbers do not depend on earlier rejections: one lane per trial and the lowest accepted lane equal the
 * sequential loop.  The draws are made whatever the mask; the mask only decides what is applied.
 *
 * ssd_augment_plan: two launches of one wave per image (draws and crop search; then offsets and boxes), no host
 * synchronisation.
 *   box f32 [total_gt][4] relative (cx, cy, w, h) against src_hw int32 [B][2] (h, w); cls f32 [total_gt]; gt_off int32 [B+1]
 *   params   [B] ssd_augment_params, what was drawn and applied per image
 *   box_out / cls_out [total_gt]: the kept boxes compacted in image then input order, off_out int32 [B+1] their offsets;
 *            rows from off_out[B] up to total_gt are written as zeros.
 * Bounds contract with ssd_match_encode: it may be called on (box_out, cls_out, off_out) with the un-augmented total_gt and
 * max_nt, which bound the augmented counts from above: k_match_rows reads every row below total_gt (finite by the above),
 * the per-image kernels follow off_out, and max_nt only bounds the per-image count (and picks a kernel variant).
 * ssd_augment_image: one thread per output pixel.  src_kind 0: ragged uint8 as ssd_image_resize_prep (src_off int64 [B]
 * byte offsets); src_kind 1: f32 images in [0,1], src_off int64 [B] element offsets or NULL for a dense [B,H,W,3]
 * (image b at b*H*W*3, H and W from src_hw).
 * Both return SSD_ERR_VALUE before any launch for null pointers, B <= 0, S <= 0, total_gt < 0, unknown stage bits or an
 * unknown source kind.
 * ---------------------------------------------------------------------------------------- */
typedef enum { SSD_AUG_PHOTO = 1, SSD_AUG_EXPAND = 2, SSD_AUG_CROP = 4, SSD_AUG_FLIP = 8, SSD_AUG_ALL = 15 } ssd_augment_stage;
typedef struct {
    int32_t stages;            /* stage bits applied: PHOTO as requested; EXPAND, CROP, FLIP where drawn and taken */
    int32_t mode;              /* crop mode drawn, 0..6 (0 without CROP in the mask) */
    int32_t trial;             /* accepted crop trial, -1 = none */
    int32_t photo;             /* photometric bits applied: 1 brightness, 2 contrast, 4 contrast first, 8 saturation, 16 hue */
    int32_t canvas_w, canvas_h, off_x, off_y;
    int32_t patch_x, patch_y, patch_w, patch_h;     /* in canvas pixels */
    int32_t flip;
    int32_t n_boxes;           /* boxes kept */
    int32_t reserved[2];
    float delta, alpha, saturation, hue;            /* drawn values (recorded whether applied or not) */
} ssd_augment_params;
int ssd_augment_plan(const float* box, const float* cls, const int32_t* gt_off, const int32_t* src_hw, int B, int total_gt,
                     int stages, uint64_t seed, int64_t first_index, ssd_augment_params* params, float* box_out,
                     float* cls_out, int32_t* off_out, void* stream);
int ssd_augment_image(const void* src, int src_kind, const int64_t* src_off, const int32_t* src_hw,
                      const ssd_augment_params* params, void* out, int B, int S, int normalize, void* stream);
/* MaxPool2D 2x2 stride 2 (VGG block pools: VALID; models/ssd_model.py:84: SAME -> Ho = ceil(H/2)) */
int ssd_maxpool2x2_fwd(const void* x, void* y, int B, int H, int W, int C, int Ho, int Wo, void* stream);
/* pooling backward fused with the ReLU backward of the layer that produced x */
int ssd_maxpool2x2_bwd(const void* x, const void* y, const void* dy, void* dx, int B, int H, int W, int C, int Ho,
                       int Wo, void* stream);
/* The same pooling with a recorded winner (training): `code` u32 [B*Ho*Wo*C/8] receives one 4-bit code per pooled
 * element (window position 2*dy+dx of the first maximum, 4 = maximum <= 0: no gradient through the ReLU in front);
 * the backward pass then reads only dy and the codes.  Results are identical to ssd_maxpool2x2_fwd / _bwd. */
int ssd_maxpool2x2_fwd_argmax(const void* x, void* y, void* code, int B, int H, int W, int C, int Ho, int Wo, void* stream);
int ssd_maxpool2x2_bwd_argmax(const void* code, const void* dy, void* dx, int B, int H, int W, int C, int Ho, int Wo,
                              void* stream);
/* The un-pooling added onto a dx that already holds a gradient (an activation that feeds a head and a pooling: conv4_3 of
 * the VGG-16 SSD300): dx[p] = bf16(float(dx[p]) + g) where ssd_maxpool2x2_bwd_argmax would have written a winner's
 * gradient g at p (one fp32 addition, one rounding); every other element of dx keeps its bits: the losers of a window, code
 * 4, and the last row / column that a VALID pooling of an odd map does not cover.  No memset, no atomics; codes, packing
 * and shape rules as above (C % 8 == 0, SAME when 2*Ho > H).  SSD_ERR_VALUE before any launch otherwise. */
int ssd_maxpool2x2_bwd_argmax_accumulate(const void* code, const void* dy, void* dx, int B, int H, int W, int C, int Ho,
                                         int Wo, void* stream);
/* Block-scaled fp8 forward convolution (BASELINE configs[4]: "fp8 MFMA convs"; no reference counterpart -- the reference's
 * convolutions are fp32 TensorFlow ops, models/ssd_model.py:86-93 for the >= 256-channel 3x3 layers this serves).  MX format: OCP
 * e4m3 elements, one E8M0 scale byte (2^(s-127)) per 32 consecutive channels, multiplied on v_mfma_scale_f32_16x16x128_f8f6f4.
 *   ssd_quantize_mx_fp8     x bf16 [n] (n % 32 == 0) -> q u8 [n], scale u8 [n/32]: scale = smallest power of two with |x|/scale <= 448
 *                           (exponent clamped to -127 .. 127; an all-zero block: byte 127).  A block that holds a NaN or an infinity:
 *                           32 bytes 0x7F (e4m3 NaN) under the scale byte 127 -- it dequantises to NaN, no scale byte is ever 255.
 *                           The fused quantisers below follow the same rule (csrc/mxfp8.h).
 *   ssd_conv3x3_fwd_mxfp8   y bf16 [B,H,W,Cout] = relu?(conv3x3 SAME stride 1 of x with w + bias); x8 [B,H,W,Cin] / xscale [B,H,W,Cin/32],
 *                           w8 [Cout][3][3][Cin] / wscale [Cout][3][3][Cin/32] as ssd_quantize_mx_fp8 makes them; Cin % 128 == 0,
 *                           Cout % 8 == 0 (SSD_ERR_UNSUPPORTED otherwise); fp32 accumulation */
int ssd_quantize_mx_fp8(const void* x_bf16, void* q, void* scale, long long n, void* stream);
int ssd_conv3x3_fwd_mxfp8(const void* x8, const void* xscale, const void* w8, const void* wscale, const float* bias, void* y, int B,
                          int H, int W, int Cin, int Cout, int relu, void* stream);
/* The general MX-fp8 forward convolution of the ResNet-50 trunk's fp8 forward (BASELINE configs[4]; resnet_engine.py,
 * precision="mxfp8"): every trunk layer with Cin % 128 == 0 except the stem, fed directly by the layer before it.
 *   ssd_conv2d_fwd_mxfp8    relu?(conv of x with w + bias), k x k filters (k = 1 or 3), stride 1 or 2, explicit top / left pads
 *                           (TF-SAME: ssd_conv2d_fwd's), output [B,Ho,Wo,Cout].  x8 [B,H,W,Cin] / xscale [B,H,W,Cin/32],
 *                           w8 [Cout][k][k][Cin] / wscale [Cout][k][k][Cin/32] as ssd_quantize_mx_fp8 makes them; fp32 accumulation.
 *                           Outputs, any non-empty subset (null = not written): y_bf16 bf16 [B,Ho,Wo,Cout] (bias, ReLU, one
 *                           rounding); y8 u8 [B,Ho,Wo,Cout] + yscale u8 [B,Ho,Wo,Cout/32], given together: ssd_quantize_mx_fp8 of
 *                           that bf16 result, bit for bit, computed in the epilogue.  At k = 3, stride 1, pads 1 the bf16 output
 *                           equals ssd_conv3x3_fwd_mxfp8's.  SSD_ERR_VALUE: no output, y8 without yscale (or the reverse), bad
 *                           dimensions; SSD_ERR_UNSUPPORTED: Cin % 128, k not in {1, 3}, stride not in {1, 2}, Cout % 8, Cout % 32
 *                           with y8, an operand or output of 2^31 bytes or more.
 *   ssd_add_relu_fwd_mxfp8  out_bf16 = relu(a + b) (ssd_add_relu_fwd's result) and q u8 [n] / scale u8 [n/32] = its
 *                           ssd_quantize_mx_fp8, in one pass (a residual add feeding both bf16 and fp8 layers); n % 32 == 0,
 *                           blocks of 32 consecutive elements (= the per-pixel channel blocks when C % 32 == 0); SSD_ERR_VALUE
 *                           otherwise or for a null pointer */
int ssd_conv2d_fwd_mxfp8(const void* x8, const void* xscale, const void* w8, const void* wscale, const float* bias, void* y_bf16,
                         void* y8, void* yscale, int B, int H, int W, int Cin, int Cout, int k, int stride, int pad_t, int pad_l,
                         int Ho, int Wo, int relu, void* stream);
int ssd_add_relu_fwd_mxfp8(const void* a, const void* b, void* out_bf16, void* q, void* scale, long long n, void* stream);
/* The SSD300 VGG trunk's fp8 forward (engine.py, precision="mxfp8"; no reference counterpart: fp32 TensorFlow convolutions and
 * MaxPool2D, models/ssd_model.py:82-84): block3_conv3 and the SAME 2x2 max pool behind it in one launch, the full-resolution
 * map never stored -- the seam of ssd_conv2d_fwd_pool's pool_only mode (y == NULL) on block-scaled fp8 operands.
 *   ssd_conv2d_fwd_pool_mxfp8  ssd_maxpool2x2_fwd(ssd_conv2d_fwd_mxfp8's bf16 y) bit for bit: every conv pixel accumulated in the
 *                           same order (bias, ReLU, ONE bf16 rounding), then the max over each 2x2 / stride-2 window's pixels
 *                           inside the [Ho,Wo] map -- Hp = Ho / 2 (VALID) or (Ho + 1) / 2 (TF-SAME, windows clipped at the
 *                           edge), Wp likewise.  Outputs, any non-empty subset: y_pool_bf16 bf16 [B,Hp,Wp,Cout]; y_pool8 u8
 *                           [B,Hp,Wp,Cout] + y_pool_scale u8 [B,Hp,Wp,Cout/32], given together: ssd_quantize_mx_fp8 of that pooled
 *                           map, bit for bit.  Operands and pads as ssd_conv2d_fwd_mxfp8.  SSD_ERR_VALUE (nothing launched): a
 *                           missing operand, no output, y_pool8 without y_pool_scale (or the reverse), bad dimensions, pads or
 *                           pooled sizes; SSD_ERR_UNSUPPORTED (nothing launched): k != 3, stride != 1, Cin % 128, Cout % 32, an
 *                           operand or the unpooled output of 2^31 bytes or more.  Inference only: no winner codes. */
int ssd_conv2d_fwd_pool_mxfp8(const void* x8, const void* xscale, const void* w8, const void* wscale, const float* bias,
                              void* y_pool_bf16, void* y_pool8, void* y_pool_scale, int B, int H, int W, int Cin, int Cout, int k,
                              int stride, int pad_t, int pad_l, int Ho, int Wo, int relu, int Hp, int Wp, void* stream);
/* The VGG-16 SSD300's inference fp8 forward (engine.py, fp8_inference=True; no reference counterpart): the dilated fc6 on
 * block-scaled fp8 operands, and the two poolings no fp8 convolution can run inside its own launch -- pool4 behind conv4_3,
 * whose full-resolution map a head reads, and the 3x3 / stride-1 pool5 -- as poolings that quantise what they store.
 *   ssd_conv2d_atrous_fwd_mxfp8  relu?(Conv2D(3, dilation_rate = dilation, padding = "same") of x with w + bias): ssd_conv2d_atrous_fwd
 *                           on the operands of ssd_conv2d_fwd_mxfp8 (x8 / xscale, w8 [Cout][3][3][Cin] / wscale), fp32 accumulation,
 *                           ONE bf16 rounding; outputs as ssd_conv2d_fwd_mxfp8: any non-empty subset of y_bf16 [B,H,W,Cout] and the
 *                           pair y8 / yscale = ssd_quantize_mx_fp8 of that bf16 map, bit for bit.  Any dilation >= 1, stride 1.
 *                           ssd_conv2d_fwd_mxfp8's main loop with the tap offset times the dilation; taps that lie outside the
 *                           map for every pixel (dilation >= H: a row of taps, >= W: a column) are not issued, which changes no
 *                           bit.  At dilation 1 it equals ssd_conv2d_fwd_mxfp8(k = 3, stride 1, pads 1, 1) bit for bit.
 *                           SSD_ERR_VALUE: a missing operand, no output, y8 without yscale (or the reverse), bad dimensions,
 *                           dilation < 1; SSD_ERR_UNSUPPORTED: Cin % 128, Cout % 8, Cout % 32 with y8, an operand or output of
 *                           2^31 bytes or more.  Either before anything is launched.
 *   ssd_maxpool2x2_fwd_mxfp8    q u8 [B,Ho,Wo,C] + scale u8 [B,Ho,Wo,C/32] = ssd_quantize_mx_fp8(ssd_maxpool2x2_fwd(x)) bit for bit,
 *                           in one pass: the maximum over the bf16 values of each window, then the rule of csrc/mxfp8.h on the
 *                           pooled pixel's 32-channel blocks.  Ho = H / 2 (VALID) or (H + 1) / 2 (TF-SAME, windows clipped), Wo
 *                           likewise.  y_bf16 (bf16 [B,Ho,Wo,C], may be null): the pooled map itself as well.
 *   ssd_maxpool3x3s1_fwd_mxfp8  the same for ssd_maxpool3x3s1_fwd's y (3x3 / stride 1 / pad 1), outputs [B,H,W,C] / [B,H,W,C/32].
 *                           Both: x bf16 [B,H,W,C]; no winner codes (inference only).  SSD_ERR_VALUE: a NULL x, q or scale, a
 *                           dimension below 1, pooled sizes that are neither VALID nor SAME, overlapping tensors;
 *                           SSD_ERR_UNSUPPORTED: C % 32, a map of 2^31 elements or more.  Nothing is launched on either. */
int ssd_conv2d_atrous_fwd_mxfp8(const void* x8, const void* xscale, const void* w8, const void* wscale, const float* bias,
                                void* y_bf16, void* y8, void* yscale, int B, int H, int W, int Cin, int Cout, int dilation, int relu,
                                void* stream);
int ssd_maxpool2x2_fwd_mxfp8(const void* x, void* y_bf16, void* q, void* scale, int B, int H, int W, int C, int Ho, int Wo,
                             void* stream);
int ssd_maxpool3x3s1_fwd_mxfp8(const void* x, void* y_bf16, void* q, void* scale, int B, int H, int W, int C, void* stream);
/* The stride-1 data gradients of the ResNet-50 trunk after a training-mode fp8 forward (resnet_engine.py, mxfp8_bwd_plan):
 *   ssd_conv2d_bwd_data_mxfp8  dx[B,H,W,Cin] = ssd_conv2d_bwd_data's result at stride 1 on block-scaled fp8 operands -- dy8
 *                           [B,Ho,Wo,Cout] / dyscale [B,Ho,Wo,Cout/32] and wt8 [Cin][k][k][Cout] / wtscale [Cin][k][k][Cout/32],
 *                           ssd_quantize_mx_fp8 of dy and of ssd_weight_transpose's w_t; k = 1 or 3, pad_t / pad_l the FORWARD
 *                           pads (mirrored inside); fp32 accumulation.  Epilogue in ssd_conv2d_bwd_data's order: accumulate != 0:
 *                           + the bf16 dx already there; then zero where relu_src <= 0 (relu_src bf16 [B,H,W,Cin] or null); ONE
 *                           bf16 rounding.  Outputs, any non-empty subset: dx_bf16 bf16 [B,H,W,Cin]; dx8 u8 [B,H,W,Cin] + dxscale
 *                           u8 [B,H,W,Cin/32], given together: ssd_quantize_mx_fp8 of that bf16 result, bit for bit.
 *                           SSD_ERR_VALUE: a missing operand, no output, dx8 without dxscale (or the reverse), accumulate
 *                           without dx_bf16, bad dimensions or pads; SSD_ERR_UNSUPPORTED (nothing launched): Cout % 128,
 *                           Cin % 32, k not in {1, 3}, an operand or output of 2^31 bytes or more.  Stride-2 data gradients
 *                           have no fp8 form: ssd_conv2d_bwd_data. */
int ssd_conv2d_bwd_data_mxfp8(const void* dy8, const void* dyscale, const void* wt8, const void* wtscale, const void* relu_src,
                              void* dx_bf16, void* dx8, void* dxscale, int B, int H, int W, int Cin, int Cout, int k, int pad_t,
                              int pad_l, int Ho, int Wo, int accumulate, void* stream);
/* A chain of small convolutions in ONE launch, one workgroup per image, activations in LDS (chain.hip) -- the reference's
 * "extras" behind the 19x19 map (models/ssd_model.py:124-150: six layers on 10x10 ... 1x1 maps), forward or data gradient.
 * Layer l reads the output of layer l-1 (layer 0: in0 [B][Hi*Wi][Kc] bf16) and writes out [B][Ho*Wo][N] bf16:
 *   out[o][n] = epilogue( sum over taps t, channels k of  in[(o * mul + t - pad) / div][k] * w[n][t][k] )
 * with the source pixel taken only when divisible by div and inside the map -- the implicit-GEMM geometry of
 * ssd_conv2d_fwd (mul = stride, div = 1, w = filters [Cout][k][k][Cin]) and of ssd_conv2d_bwd_data (mul = 1, div = stride,
 * pad = ksize - 1 - pad, w = ssd_weight_transpose's [Cin][k][k][Cout_pad]).  Epilogue: + bias (if not null), ReLU (relu != 0),
 * sign bits written to relu_bits (if not null); accumulate != 0: out += result BEFORE the mask (two gradients meet at a
 * feature map); mask_bits / mask_src (at most one): zero where the bit is clear / the value is <= 0.
 * Needs Kc % 128 == 0, N % 16 == 0, Ho*Wo <= 112, div in {1, 2}, every layer's input + output image within 160 KB of LDS
 * (rows padded by 16 bytes): SSD_ERR_UNSUPPORTED otherwise, nothing launched.  fp32 accumulation in one pass over k. */
#define SSD_CHAIN_MAX_LAYERS 8
#define SSD_CHAIN_PACK_MAX 16
/* w of a chain layer is NOT the filter tensor itself but its fragment-packed copy (ssd_chain_pack_weights): for filters
 * [N][K] bf16 with k = (tap, channel) contiguous -- the forward filters [Cout][k*k*Cin] or ssd_weight_transpose's
 * [Cin][k*k*Cout_pad] -- packed[N/16][K/32][64][8] with element (lane, e) of fragment (nt, s) = w[16 nt + (lane & 15)]
 * [32 s + 8 (lane >> 4) + e]: a wave's MFMA operand is one contiguous KB.  N % 16 == 0, K % 32 == 0; up to
 * SSD_CHAIN_PACK_MAX tensors per launch.  Re-pack after every optimizer step. */
typedef struct {
    const void* src;
    void* dst;
    int N, K;
} ssd_chain_pack;
int ssd_chain_pack_weights(const ssd_chain_pack* items, int count, void* stream);
/* Optional: read the packed copies (items[i].dst, N, K; src unused) into every XCD's L2 from a second stream shortly before
 * the ssd_conv_chain launch that uses them -- the chain's workgroups stream the filters at one miss latency per 128 KB in
 * flight when they are cold.  Reads only; no effect on results. */
int ssd_chain_prefetch(const ssd_chain_pack* items, int count, void* stream);
typedef struct {
    const void* w;
    const float* bias;
    void* out;
    const void* mask_bits;
    const void* mask_src;
    void* relu_bits;
    int Hi, Wi, Kc, Ho, Wo, N, ksize, mul, div, pad_t, pad_l, relu, accumulate;
} ssd_chain_layer;
int ssd_conv_chain(const void* in0, const ssd_chain_layer* layers, int nlayers, int B, void* stream);
/* Pieces of a ResNet-50 trunk (BASELINE configs[4]; the reference hard-codes its VGG trunk, models/ssd_model.py:46,75-97, so these
 * have no reference counterpart: semantics are Keras / TensorFlow's Add + ReLU, MaxPooling2D(3, strides=2, padding="same") and
 * their tape.gradient).  bf16 NHWC, n = element count (a multiple of 8).
 *   ssd_add_relu_fwd      out = relu(a + b)                               (residual add of a bottleneck block)
 *   ssd_relu_mask_bwd     out (+)= g where act > 0                        (its gradient on the identity-skip branch)
 *   ssd_maxpool3x3s2_fwd  3x3 / stride-2 max pooling with explicit top / left padding; code u32 [B*Ho*Wo*C/8]: one nibble per
 *                         element = 3 dy + dx of the first maximum, 15 = maximum <= 0 (no gradient through the ReLU in front)
 *   ssd_maxpool3x3s2_bwd  dx = gather of dy over the (overlapping) windows whose winner is the pixel: deterministic */
int ssd_add_relu_fwd(const void* a, const void* b, void* out, long long n, void* stream);
int ssd_relu_mask_bwd(const void* g, const void* act, void* out, int accumulate, long long n, void* stream);
int ssd_maxpool3x3s2_fwd(const void* x, void* y, void* code, int B, int H, int W, int C, int Ho, int Wo, int pad_t, int pad_l,
                         void* stream);
int ssd_maxpool3x3s2_bwd(const void* code, const void* dy, void* dx, int B, int H, int W, int C, int Ho, int Wo, int pad_t, int pad_l,
                         void* stream);
/* ------------------------------------------------------------------------------------------
 * Pieces of the SSD paper's VGG-16 trunk (Liu et al. 2016, section 3.1: `pool5` 3x3 / stride 1 and the dilated `fc6`, 3x3,
 * dilation 6, 512 -> 1024 on the 19x19 map; no reference counterpart: the reference truncates VGG-16 at block3 and has no
 * dilation).  Semantics are Keras / TensorFlow's Conv2D(3, dilation_rate=d, padding="same"), MaxPooling2D(3, strides=1,
 * padding="same") and their tape.gradient.  Launched by SSDEngine on engine.VGG16_SSD300_TRUNK (nodes 17 and 18).
 *
 * Atrous convolution: kernel 3x3, stride 1, padding `dilation` on every side, output H x W.  Tap (ty, tx) of output pixel
 * (oy, ox) reads input pixel (oy + (ty-1) d, ox + (tx-1) d), or zero outside the map; a tap that is outside for every pixel
 * (d >= H for ty != 1, d >= W for tx != 1) is skipped, so any d >= max(H, W) leaves the centre tap alone.  Layouts are those of
 * ssd_conv2d_*: x, y, dy, dx bf16 NHWC; w bf16 [Cout][3][3][Cin]; w_t exactly what ssd_weight_transpose produces,
 * [Cin][3][3][Cout_pad], spatially flipped (with symmetric padding the data gradient is the same dilated convolution of dy with
 * w_t); bias fp32 [Cout] or NULL; dw fp32 [Cout][3][3][Cin], written, not accumulated (the dead taps: zeros); dbias fp32 [Cout]
 * or NULL; dy of the weight gradient [B,H,W,ldy], first Cout channels used.
 * Arithmetic: bf16 products accumulated in fp32 on the MFMA; y is rounded to bf16 once, after the bias and after max(., 0)
 * where relu; ssd_conv2d_atrous_bwd_data writes dx = bf16(conv_T), with accumulate dx = bf16(float(dx) + conv_T), either then
 * zeroed where relu_src <= 0 (relu_src: NULL, or the forward activation, which may be stored in dx's place as for
 * ssd_conv2d_bwd_data).  No floating-point atomics: dw and dbias are fixed-order sums of partial sums in ws, bitwise
 * reproducible; ws needs no initial contents and exactly ssd_conv2d_atrous_bwd_weight_workspace_bytes(...) bytes.
 * Supported: Cin % 64 == 0 (64 ... 1024 and beyond), Cout % 8 == 0 and Cout_pad % 8 == 0 (8 ... 1024 and beyond), ldy >= Cout
 * and ldy % 8 == 0, every operand and output below 2^31 bytes (32-bit offsets into buffer descriptors); any d >= 1.
 *
 * ssd_maxpool3x3s1_fwd / _bwd: windows clipped at the map's edge; code u32 [B*H*W*C/8], one nibble per element in the packing
 * of ssd_maxpool3x3s2_fwd = 3 dy + dx of the FIRST maximum in window order, 15 = the maximum is <= 0; the backward pass writes
 * dx[p] = the sum of dy over the (up to nine) windows whose code names p, gathered per input pixel in window order, in fp32,
 * rounded once: deterministic.  C % 8 == 0, B*H*W*C < 2^31.
 *
 * Refusals, decided on the host before anything is launched.  SSD_ERR_VALUE: a NULL required pointer (everything but bias,
 * relu_src and dbias); B, H, W, a channel count or dilation < 1; an output that overlaps an input (relu_src excepted).
 * SSD_ERR_WORKSPACE: ws NULL or smaller than the query (as ssd_conv2d_bwd_weight).  SSD_ERR_UNSUPPORTED (the size query
 * returns 0): a shape outside the supported range above.
 * ---------------------------------------------------------------------------------------- */
int ssd_conv2d_atrous_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int Cin, int Cout,
                          int dilation, int relu, void* stream);
int ssd_conv2d_atrous_bwd_data(const void* dy, const void* w_t, const void* relu_src, void* dx, int B, int H, int W, int Cin,
                               int Cout_pad, int dilation, int accumulate, void* stream);
size_t ssd_conv2d_atrous_bwd_weight_workspace_bytes(int B, int H, int W, int Cin, int Cout, int ldy, int dilation);
int ssd_conv2d_atrous_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, int B, int H, int W, int Cin, int Cout,
                                 int ldy, int dilation, void* ws, size_t ws_bytes, void* stream);
int ssd_maxpool3x3s1_fwd(const void* x, void* y, void* code, int B, int H, int W, int C, void* stream);
int ssd_maxpool3x3s1_bwd(const void* code, const void* dy, void* dx, int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depthwise 3x3 convolution: the operator a MobileNet-SSD / SSDLite trunk alternates with the 1x1 convolution (no reference
 * counterpart; the "dwconv" nodes of engine.MOBILENET_V1_SSD300_TRUNK launch it).  Semantics are Keras / TensorFlow's DepthwiseConv2D(3, strides = s,
 * depth_multiplier = 1) + bias (+ ReLU) and its tape.gradient: channel c of the output depends on channel c of the input
 * alone -- a nine-tap stencil bound by memory bandwidth, not a GEMM.
 *
 * Layouts: x [B,H,W,C], y and dy [B,Ho,Wo,C], dx [B,H,W,C], all bf16 NHWC; w bf16 [3][3][C] (Keras's (3,3,C,1) kernel,
 * channel-contiguous); bias fp32 [C] or NULL; dw fp32 [3][3][C] and dbias fp32 [C] or NULL, both written, not accumulated.
 * Geometry: stride 1 or 2; padding is passed explicitly as for ssd_conv2d_fwd: pad_t and pad_l are each 0 or 1, the bottom
 * and right padding is implied by the output size -- (Ho-1)*stride + 3 - H - pad_t must lie in 0..2, likewise for the width --
 * and what falls outside the map reads as zero.  TF SAME at stride 2 on an even map is pad_t = 0 with one row below; a
 * torch-style padding 1 with Ho = (H-1)/2 + 1 is served as well.
 * Arithmetic: the forward pass forms the nine products in fp32 and accumulates them in tap order (ky outer, kx inner) starting
 * from the bias, then max(., 0) where relu, then ONE rounding to bf16.  The data gradient is gathered per input pixel (no
 * scatter, no atomics): dx[b,iy,ix,c] = the fp32 sum, in tap order, of dy[b,oy,ox,c] * w[ky][kx][c] over the taps for which
 * oy = (iy + pad_t - ky) / stride is integral and inside the map, likewise ox; with accumulate the bf16 dx already there is
 * added; then zero where relu_src <= 0 (relu_src: NULL, or the forward activation, which may be stored in dx's place as for
 * ssd_conv2d_bwd_data); one rounding.  The weight gradient sums x * dy (dbias: dy) over all B*Ho*Wo output pixels as
 * fixed-order partial sums over pixel slabs in ws, reduced in slab order: bitwise reproducible, no floating-point atomics; ws
 * needs no initial contents and exactly ssd_dwconv3x3_bwd_weight_workspace_bytes(...) bytes.
 * Supported: C % 8 == 0, every tensor below 2^31 bytes.
 *
 * Refusals, decided on the host before anything is launched.  SSD_ERR_VALUE: a NULL required pointer (everything but bias,
 * relu_src and dbias); B, H, W, C, Ho or Wo < 1; a stride outside {1, 2}; pad_t or pad_l outside {0, 1}, or Ho / Wo that break
 * the rule above; an output that overlaps an input (relu_src aliasing dx is the one exception).  SSD_ERR_WORKSPACE: ws NULL or
 * smaller than the query.  SSD_ERR_UNSUPPORTED (the size query returns 0): C % 8 != 0, or a tensor of 2^31 bytes or more.
 * ---------------------------------------------------------------------------------------- */
int ssd_dwconv3x3_fwd(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int C, int stride, int pad_t,
                      int pad_l, int Ho, int Wo, int relu, void* stream);
int ssd_dwconv3x3_bwd_data(const void* dy, const void* w, const void* relu_src, void* dx, int B, int H, int W, int C, int stride,
                           int pad_t, int pad_l, int Ho, int Wo, int accumulate, void* stream);
/* ReLU sign bytes, in the layout of ssd_conv2d_fwd_relubits.  ssd_dwconv3x3_fwd_relubits = ssd_dwconv3x3_fwd (relu = 1), y bit
 * for bit, that also writes relu_bits u8 [B*Ho*Wo][C/8]: bit k of byte c is set where channel 8c + k of y is > 0.
 * ssd_dwconv3x3_bwd_data_bits = ssd_dwconv3x3_bwd_data, dx bit for bit, with the mask given as relu_bits u8 [B*H*W][C/8] instead
 * of relu_src: one byte per stored 16-byte group.  Both refuse what their siblings refuse, and with SSD_ERR_VALUE a NULL
 * relu_bits and relu_bits overlapping an output (or, where it is an output itself, an input). */
int ssd_dwconv3x3_fwd_relubits(const void* x, const void* w, const float* bias, void* y, void* relu_bits, int B, int H, int W, int C,
                               int stride, int pad_t, int pad_l, int Ho, int Wo, void* stream);
int ssd_dwconv3x3_bwd_data_bits(const void* dy, const void* w, const void* relu_bits, void* dx, int B, int H, int W, int C, int stride,
                                int pad_t, int pad_l, int Ho, int Wo, int accumulate, void* stream);
size_t ssd_dwconv3x3_bwd_weight_workspace_bytes(int B, int H, int W, int C, int stride, int Ho, int Wo);
int ssd_dwconv3x3_bwd_weight(const void* x, const void* dy, float* dw, float* dbias, int B, int H, int W, int C, int stride,
                             int pad_t, int pad_l, int Ho, int Wo, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward pass of ALL head convolutions (models/ssd_model.py:153-162; 3x3, stride 1, SAME, no activation) from the compact
 * gradient rows of ssd_loss_fwd_bwd_heads -- the part of tape.gradient (:248) behind the loc / conf outputs.  Work is
 * proportional to the rows that carry a gradient (4P of B*A anchors), not to the feature maps; results equal the dense
 * ssd_conv2d_bwd_data / ssd_conv2d_bwd_weight on the scattered rows up to fp32 summation order (dx rounds once to bf16).
 * One launch sequence serves every level; row counts are read on the device (no host synchronisation); deterministic.
 *   hl  HOST struct, per level: the feature map x bf16 [B,H,W,Cin] (Cin % 128 == 0 else SSD_ERR_UNSUPPORTED), cout =
 *       per_cell*(4+C) filters, w_tap = the head filters transposed tap-major bf16 [3][3][Cin][npad] (w_tap[kh][kw][ci][co]
 *       = w[co][kh][kw][ci], zero for co >= cout; ssd_weight_transpose_batched with bit 8 of the kernel-size field set),
 *       the ReLU mask of x as sign bits (relu_bits, uint8 [B,H,W,Cin/8]) or as the activation itself (relu_src) or neither,
 *       outputs dx bf16 [B,H,W,Cin] (overwritten: every pixel, zeros where no row reaches), dw f32 [cout][3][3][Cin], dbias
 *       f32 [cout] or NULL.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int levels;
    int H[SSD_MAX_LEVELS], W[SSD_MAX_LEVELS], Cin[SSD_MAX_LEVELS], cout[SSD_MAX_LEVELS];
    const void* x[SSD_MAX_LEVELS];
    const void* w_tap[SSD_MAX_LEVELS];
    const void* relu_bits[SSD_MAX_LEVELS];
    const void* relu_src[SSD_MAX_LEVELS];
    void* dx[SSD_MAX_LEVELS];
    float* dw[SSD_MAX_LEVELS];
    float* dbias[SSD_MAX_LEVELS];
} ssd_head_layers;
size_t ssd_heads_bwd_data_sparse_workspace_bytes(int B, const ssd_head_layers* hl);
int ssd_heads_bwd_data_sparse(const ssd_head_grads* hg, const ssd_head_layers* hl, int B, void* ws, size_t ws_bytes,
                              void* stream);
/* The same for a subset of the levels (bit l of level_mask): the small maps' gradients head the extras' data-gradient
 * chain, the 38x38 / 19x19 maps' are not read until that chain reaches them, so a caller may issue the two groups on two
 * streams.  Every level keeps its own slice of `ws`: calls with disjoint masks may share one workspace concurrently.
 * SSD_ERR_VALUE for an empty mask. */
int ssd_heads_bwd_data_sparse_levels(const ssd_head_grads* hg, const ssd_head_layers* hl, int B, unsigned level_mask,
                                     void* ws, size_t ws_bytes, void* stream);
size_t ssd_heads_bwd_weight_sparse_workspace_bytes(int B, const ssd_head_grads* hg, const ssd_head_layers* hl);
int ssd_heads_bwd_weight_sparse(const ssd_head_grads* hg, const ssd_head_layers* hl, int B, void* ws, size_t ws_bytes,
                                void* stream);

/* dloc[B,A,4], dconf[B,A,classes] (bf16) -> one level's padded NHWC head gradient [B, hw, npad] */
int ssd_head_grad_pack(const void* dloc, const void* dconf, void* out, int B, int hw, int per_cell, int classes,
                       int npad, int anchors_total, int level_off, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer step over one flat fp32 parameter buffer -- replaces the per-tensor Python loop of
 * _train_step: tf.clip_by_norm(g, 0.01) (models/ssd_model.py:249), the micro-batch mean (:251-256) and
 * optimizer.apply_gradients (:258-260; Adam/SGD and their hyper-parameters: tools/train.py:42-53).
 * Every tensor starts on a multiple of ssd_opt_block_elems() elements (pad with zeros);
 *   tensor_block_off int32[ntensors+1]: first block of each tensor;  block_tensor int32[n/block]: owner.
 * ---------------------------------------------------------------------------------------- */
int ssd_opt_block_elems(void);
/* scale[t] = clip / max(||grad_t||_2, clip) (clip <= 0: 1), norms[t] optional; partial: double[n/block] scratch */
int ssd_grad_clip_scales(const float* grad, long long n, const int32_t* tensor_block_off, int ntensors, float clip,
                         double* partial, float* scale, float* norms, void* stream);
/* grad *= scale[tensor]  in place (clipped gradients are what data-parallel ranks all-reduce) */
int ssd_grad_apply_scale(float* grad, long long n, const int32_t* block_tensor, const float* scale, void* stream);
/* acc = (first ? 0 : acc) + grad * scale[tensor]: the micro-batch accumulation of clipped gradients (:251-255) */
int ssd_grad_accumulate(float* acc, const float* grad, long long n, const int32_t* block_tensor, const float* scale,
                        int first, void* stream);
/* Keras Adam with lr_t = lr*sqrt(1-b2^t)/(1-b1^t) precomputed by the caller; the gradient is multiplied by
 * grad_scale (1/micro-batches or 1/world) and, if scale != NULL, by scale[tensor].  param_bf16 (may be NULL)
 * receives the bf16 copy the convolutions read. */
int ssd_adam_step(float* param, const float* grad, float* m, float* v, void* param_bf16, long long n,
                  const int32_t* block_tensor, const float* scale, float grad_scale, float lr_t, float beta1,
                  float beta2, float eps, void* stream);
int ssd_sgd_step(float* param, const float* grad, void* param_bf16, long long n, const int32_t* block_tensor,
                 const float* scale, float grad_scale, float lr, void* stream);
/* Momentum SGD with an optional per-tensor L2 term (no reference counterpart beyond tools/train.py:44-45's name == "sgd":
 * Keras SGD(momentum, nesterov), which is also Caffe SSD's solver form -- the learning rate is folded into the velocity).
 * Per element, in fp32, in this order, t = block_tensor[block]:
 *   sc = grad_scale * (scale ? scale[t] : 1)
 *   ge = g * sc;   if (decay) ge = ge + decay[t] * p          decay fp32[ntensors]: L2 coefficient per tensor, NULL = none
 *   v' = momentum * v - lr * ge
 *   p' = nesterov ? p + (momentum * v' - lr * ge) : p + v'
 * velocity is read and written; param_bf16 (may be NULL) receives the bf16 copy of p'.  One pass, no reductions; nothing
 * outside [0, n) is touched.  SSD_ERR_VALUE (nothing launched): param, grad or velocity NULL; n <= 0 or not a multiple of
 * ssd_opt_block_elems(); scale or decay without block_tensor; momentum outside [0, 1); nesterov not 0 or 1. */
int ssd_sgd_momentum_step(float* param, const float* grad, float* velocity, void* param_bf16, long long n,
                          const int32_t* block_tensor, const float* scale, const float* decay, float grad_scale, float lr,
                          float momentum, int nesterov, void* stream);
/* Exponential moving average of the parameters (no reference counterpart: TF's ExponentialMovingAverage / timm's ModelEma, the
 * weights a detector is validated and deployed with).  Per element, in fp32, om = one_minus_decay:
 *   e' = e + om * (p - e)
 * ema is read and written, param is only read.  One pass behind the optimizer launch that wrote param (a slice of the flat
 * buffer like that launch's, or all of it), 12 bytes per element, no reductions, no atomics, no workspace; nothing outside
 * [0, n) is touched.  The compiler may contract the multiply-add into one fma, so the result is promised bit for bit only
 * where the difference, the product and the sum are all exact.  Two factors are exact by construction: om == 1 stores param's
 * bits (-0.0, denormals and NaN payloads included) without reading ema -- the initialisation and "restart the average" --
 * and om == 0 leaves ema's bits as they are (nothing is launched).
 * SSD_ERR_VALUE (nothing launched): ema or param NULL; n <= 0 or not a multiple of ssd_opt_block_elems(); one_minus_decay NaN
 * or outside [0, 1]; the ranges [ema, ema + n) and [param, param + n) overlap. */
int ssd_ema_step(float* ema, const float* param, long long n, float one_minus_decay, void* stream);

/* ------------------------------------------------------------------------------------------
 * L2 normalisation over the channels with a learned per-channel scale (no reference counterpart: the SSD paper's layer on
 * the 38x38 map, section 3.1 / Caffe SSD's Normalize).  x, y, dy, dx: bf16 [P][C]; scale, dscale: fp32 [C]; rnorm: fp32 [P].
 * All arithmetic in fp32, per pixel p:
 *   r_p = 1 / sqrt(sum_k x_pk^2 + eps)      xh_pc = x_pc r_p      y_pc = bf16(scale_c xh_pc)
 *   t_pc = scale_c dy_pc      D_p = sum_k t_pk xh_pk      dx_pc = bf16(r_p (t_pc - xh_pc D_p) [+ dx_pc if accumulate])
 *   dscale_c = sum_p dy_pc xh_pc            (written, not accumulated; fixed summation order: bitwise reproducible)
 * ssd_l2norm_fwd writes r_p to rnorm where it is not NULL.  ssd_l2norm_bwd reads r_p from rnorm, or recomputes it from x
 * where rnorm is NULL (the same bits); xh is always rebuilt from x, never taken from y.  ws: ssd_l2norm_ws_bytes(P, C) bytes
 * of scratch without initial-content requirements.  y may not alias x; dx may alias neither x nor dy.
 * Shapes: C % 128 == 0, 128 <= C <= 1024, P >= 1; any other C: SSD_ERR_UNSUPPORTED (ssd_l2norm_ws_bytes: 0).  SSD_ERR_VALUE: a
 * NULL required pointer (everything but rnorm), an aliased output, P < 1, eps < 0 or a workspace that is too small.  Nothing is
 * launched on either error.
 * ---------------------------------------------------------------------------------------- */
size_t ssd_l2norm_ws_bytes(long long P, int C);
int ssd_l2norm_fwd(const void* x, const float* scale, void* y, float* rnorm, long long P, int C, float eps, void* stream);
int ssd_l2norm_bwd(const void* dy, const void* x, const float* scale, const float* rnorm, void* dx, int accumulate,
                   float* dscale, void* ws, size_t ws_bytes, long long P, int C, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Batch normalisation over the rows of an NHWC map (no reference counterpart: the ResNet-50 SSD512 trunk's opt-in training
 * mode).  x, y, dy, dx: bf16 [P][C], P = B H W rows, the channel fastest; gamma, beta, mean, rstd, running_mean, running_var,
 * dgamma, dbeta: fp32 [C].  All arithmetic in fp32, per channel c:
 *   training forward   mu = (1/P) sum_p x_pc      v = (1/P) sum_p (x_pc - mu)^2 (biased)      rstd = 1 / sqrt(v + eps)
 *                      y_pc = bf16(gamma_c (x_pc - mu) rstd + beta_c), through max(., 0) where relu;  mean <- mu, rstd <- rstd
 *                      running_mean <- (1 - m) running_mean + m mu     running_var <- (1 - m) running_var + m v P / (P - 1)
 *                      (PyTorch's convention; both running pointers NULL: no running update)
 *   inference forward  a = gamma / sqrt(running_var + eps)   b = beta - running_mean a   y = bf16(x a + b) [max(., 0)]
 *   backward           xh = (x - mu) rstd (rebuilt from x and the saved mean / rstd, never from y)
 *                      dbeta = sum_p dy     dgamma = sum_p dy xh     dx = bf16(gamma rstd (dy - dbeta / P - xh dgamma / P))
 *                      dy is expected masked by the node's own ReLU already; dgamma, dbeta are written, not accumulated.
 * The variance is never formed as E[x^2] - mu^2: per-thread shifted sums give (n, mean, M2) partials, merged by Chan's formula.
 * Per-channel sums come from fixed-order partial sums in ws (no atomics): bitwise reproducible.  ws: exactly ssd_bn_ws_bytes
 * bytes of scratch without initial-content requirements.  y may not alias x; dx may alias neither x nor dy.
 * Shapes: C % 64 == 0 and 64 <= C <= 2048, else SSD_ERR_UNSUPPORTED (ssd_bn_ws_bytes: 0); P >= 2 for training and backward,
 * P >= 1 for inference.  SSD_ERR_VALUE: a NULL required pointer, only one of the two running pointers, an aliased output,
 * eps <= 0, momentum outside (0, 1], P too small or a workspace that is too small.  Nothing is launched on either error.
 * ---------------------------------------------------------------------------------------- */
size_t ssd_bn_ws_bytes(long long P, int C);
int ssd_bn_fwd_train(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                     float* running_mean, float* running_var, float momentum, float eps, int relu, void* ws, size_t ws_bytes,
                     long long P, int C, void* stream);
int ssd_bn_fwd_infer(const void* x, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                     void* y, float eps, int relu, long long P, int C, void* stream);
int ssd_bn_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
               float* dbeta, void* ws, size_t ws_bytes, long long P, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dispatch queries (no reference counterpart; testing / reports): which kernel a convolution call with this shape
 * resolves to.  They run the library's own dispatch code with launching switched off, so the answer cannot drift from
 * what the call does.  Return: a plan word >= 0 (kernel id in SSD_PLAN_KERNEL_MASK, path flags above it) or a negative
 * ssd_status for a shape the call itself would reject.  pool: 0 = ssd_conv2d_fwd, 1 = ssd_conv2d_fwd_pool, 2 = the same
 * with y == NULL.  ws_bytes: the workspace the call would be given (0: none, no split-K).
 * ---------------------------------------------------------------------------------------- */
enum ssd_conv_plan {
    SSD_PLAN_KERNEL_MASK = 0xff,
    SSD_PLAN_C64B = 1, SSD_PLAN_P32_64, SSD_PLAN_P32_128, SSD_PLAN_8PH,
    SSD_PLAN_DMA_256_256, SSD_PLAN_DMA_256_128, SSD_PLAN_DMA_256_64, SSD_PLAN_DMA_128_64, SSD_PLAN_DMA_128_128,
    SSD_PLAN_CONV0_FWD, SSD_PLAN_P512, SSD_PLAN_PW,
    SSD_PLAN_WG_FIRST = 32, SSD_PLAN_WG_PATCH_16x16, SSD_PLAN_WG_PATCH_6x40, SSD_PLAN_WG_PATCH_10x24, SSD_PLAN_WG_TILE,
    SSD_PLAN_WG_GENERIC,
    SSD_PLAN_F_FLAT = 0x100,         /* strip blocks over a narrow map */
    SSD_PLAN_F_ROWFLAT = 0x200,      /* one strip of rows over all images */
    SSD_PLAN_F_SPLITK = 0x400,       /* split-K partial sums + k_igemm_finalize */
    SSD_PLAN_F_POOL_FUSED = 0x800,   /* 2x2 pooling computed in the convolution's epilogue */
    SSD_PLAN_F_S2 = 0x1000,          /* stride-2 data gradient by parity classes */
    SSD_PLAN_F_REDUCE_WIDE = 0x2000  /* >= 32 weight-gradient splits: k_wgrad_reduce_wide (else k_wgrad_reduce2) */
};
int ssd_conv2d_fwd_plan(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho, int Wo,
                        int pool, size_t ws_bytes);
int ssd_conv2d_head_fwd_plan(int B, int H, int W, int Cin, int per_cell, int classes, size_t ws_bytes);
int ssd_conv2d_bwd_data_plan(int B, int H, int W, int Cin, int Cout_pad, int ksize, int stride, int pad_t, int pad_l, int Ho,
                             int Wo, int accumulate, size_t ws_bytes);
/* ssd_conv2d_bwd_data_unpool (arguments as there; has_relu_src: relu_src != NULL): the data-gradient dispatch with the
 * un-pooling store, which ssd_conv2d_bwd_data_plan does not model (64 -> 64 never runs on k_conv3x3_c64b then).  Answers what
 * the call would return, its refusals included. */
int ssd_conv2d_bwd_data_unpool_plan(int B, int H, int W, int Cin, int Cout_pad, int Hf, int Wf, int has_relu_src,
                                    size_t ws_bytes);
int ssd_conv2d_bwd_weight_plan(int B, int H, int W, int Cin, int Cout, int ldy, int ksize, int stride, int pad_t, int pad_l,
                               int Ho, int Wo);
const char* ssd_conv_plan_name(int plan);
/* Launch size (the same dispatch code, launching switched off): the number of ACTIVE workgroups of the launch the call
 * resolves to -- the grid minus the workgroups that return at once (grids are rounded up to whole groups of 8, one per
 * XCD); for a split-K call the GEMM launch, not the finalize.  Set against the CU count (x workgroups per CU of the
 * kernel) it tells how full the launch's last round is.  Arguments as ssd_conv2d_fwd_plan / ssd_conv2d_bwd_data_plan.
 * Return: a count > 0, a negative ssd_status for a shape the call would reject, SSD_ERR_UNSUPPORTED where the launch site
 * reports none (the persistent pointwise GEMM). */
int ssd_conv2d_fwd_workgroups(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho,
                              int Wo, int pool, size_t ws_bytes);
int ssd_conv2d_bwd_data_workgroups(int B, int H, int W, int Cin, int Cout_pad, int ksize, int stride, int pad_t, int pad_l,
                                   int Ho, int Wo, int accumulate, size_t ws_bytes);
/* Dynamic LDS bytes of that launch (same dispatch code, same arguments): what the kernel is registered and launched with, to
 * be set against the 163840 bytes a workgroup may have.  Return: a byte count >= 0 (0: the kernel uses static LDS only), a
 * negative ssd_status for a shape the call would reject, SSD_ERR_UNSUPPORTED for the persistent pointwise GEMM. */
int ssd_conv2d_fwd_lds_bytes(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int pad_t, int pad_l, int Ho,
                             int Wo, int pool, size_t ws_bytes);
int ssd_conv2d_bwd_data_lds_bytes(int B, int H, int W, int Cin, int Cout_pad, int ksize, int stride, int pad_t, int pad_l,
                                  int Ho, int Wo, int accumulate, size_t ws_bytes);

/* Development only (no reference counterpart): override one of the library's kernel-selection defaults (names in DESIGN.md
 * section 4, e.g. "SSD_CONV_TILE") for A/B timing of kernel variants or to force a dispatch path in a test, inside one
 * process.  This is the ONE piece of mutable state the library has besides the once-per-device registration of large-LDS
 * kernels: relaxed atomics, never set by the product, never read from the environment, and results never depend on it (every
 * variant computes the same convolution).  SSD_ERR_VALUE for an unknown name. */
int ssd_dev_knob(const char* name, int value);

/* Measurement only (no reference counterpart, not on any product path): the inner loop of the convolution kernels without
 * their memory traffic -- 256 workgroups x 8 waves, each wave `iters` x 32 bf16 16x16x32 MFMAs fed by ds_read_b128 fragment
 * reads of random operands in LDS.  bench.py times it beside the train step: the rate this device sustains (devices of one
 * model differ by ~12 % on such a loop) and the in-kernel clock.
 *   stamps  DEVICE uint64[2 * ssd_dev_mfma_calibration_workgroups()]: per workgroup (delta s_memtime, delta s_memrealtime)
 *           around the loop -> clock = delta s_memtime / delta s_memrealtime x 100 MHz
 *   sink    DEVICE float[512 * workgroups], written and never read
 *   flop count of one call: ssd_dev_mfma_calibration_flops(iters) */
int ssd_dev_mfma_calibration_workgroups(void);
double ssd_dev_mfma_calibration_flops(int iters);
int ssd_dev_mfma_calibration(int iters, void* stamps, void* sink, void* stream);

/* ---- JPEG: entropy decode on the host, reconstruction on the device (csrc/jpeg_host.h, csrc/jpeg.hip) --------------------------
 * What the reference's reader does with skimage.io.imread (data_loaders/coco/make_dataset.py:112-117), split in two: the Huffman
 * stage stays on host threads, everything arithmetic runs on the device and lands in the uint8 arena that
 * ssd_image_resize_prep and ssd_augment_image (source kind 0) read.  The result equals libjpeg's default decode (integer
 * "islow" IDCT, "fancy" chroma upsampling, 16-bit fixed-point colour) bit for bit.
 *
 * Streams served: baseline sequential DCT (SOF0), 8-bit samples, Huffman; one component (any sampling factors: a single
 * component is never interleaved), or three YCbCr components with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1; 8-bit
 * quantisation tables; DHT / DQT anywhere before the scan; DRI and RSTn; one interleaved scan; fill bytes, FF 00 stuffing,
 * APPn and COM skipped.
 * SSD_ERR_UNSUPPORTED, nothing written: any other SOFn (extended, progressive, lossless, arithmetic) or DAC, sample precision
 *   other than 8, 2 or 4 components, other sampling factors, 16-bit quantisation tables, a scan that does not hold all
 *   components in frame order (multi-scan), three components marked RGB (Adobe transform 0, or ids 'R','G','B' without JFIF),
 *   more than 2^31 - 1 coefficients.
 * SSD_ERR_VALUE: no SOI; a segment length past the end or too short for its contents; zero width or height; a table id out of
 *   range, a missing table, an over-subscribed Huffman table; a Huffman code not in its table; a DC category above 15; a
 *   coefficient index past 63; entropy data that ends early; a missing or wrong restart marker; no EOI behind the scan.
 * SSD_ERR_WORKSPACE: capacity smaller than the coefficient count (ssd_jpeg_entropy_decode); nothing written.
 * Every read is checked against n, every write against capacity.
 *
 * The image record: SSD_JPEG_REC_WORDS int32 words, the same for the host header and for the device descriptor.  (Words, not
 * a struct: the record crosses host -> pinned -> device as one int32 array of B records.) */
#define SSD_JPEG_WIDTH 0
#define SSD_JPEG_HEIGHT 1
#define SSD_JPEG_NCOMP 2      /* 1 or 3 */
#define SSD_JPEG_KIND 3       /* SSD_JPEG_GREY / _444 / _422 / _420 */
#define SSD_JPEG_BLOCKS_W 4   /* [3] 8x8 blocks per row of each component's plane, padded to whole MCUs */
#define SSD_JPEG_BLOCKS_H 7   /* [3] ... per column */
#define SSD_JPEG_NCOEF 10     /* int16 coefficients of the image: 64 * sum over components of blocks_w * blocks_h */
#define SSD_JPEG_RESTART 11   /* restart interval in MCUs, 0 = none */
#define SSD_JPEG_COEF_OFF 12  /* [3] element offset of each component's plane; the host functions write them relative to the
                                 image's first coefficient, the caller of ssd_jpeg_reconstruct adds the image's base */
#define SSD_JPEG_QT 16        /* [3][64] the quantisation table of each component, natural (row-major) order */
#define SSD_JPEG_REC_WORDS 208
#define SSD_JPEG_GREY 0
#define SSD_JPEG_444 1
#define SSD_JPEG_422 2        /* luma 2x1 */
#define SSD_JPEG_420 3        /* luma 2x2 */
/* ssd_jpeg_info: HOST only (no HIP call).  Parses up to the scan header and fills rec.
 * ssd_jpeg_entropy_decode: HOST only, re-entrant (no globals: any number of threads at once).  Writes the image's ncoef
 *   QUANTISED coefficients: natural order, 64 per block, blocks row-major per component plane, planes at rec[COEF_OFF]; DC
 *   prediction undone; blocks that pad the planes to whole MCUs included as the stream codes them.  rec may be NULL. */
int ssd_jpeg_info(const void* data, size_t n, int32_t* rec);
int ssd_jpeg_entropy_decode(const void* data, size_t n, int16_t* coef, size_t capacity, int32_t* rec);
/* ssd_jpeg_reconstruct: coefficients -> RGB for a ragged batch, two launches (k_jpeg_idct, k_jpeg_rgb).
 *   coef        DEVICE int16 [total_coef], 16-byte aligned
 *   desc        DEVICE int32 [B, SSD_JPEG_REC_WORDS], COEF_OFF absolute (multiples of 64)
 *   dst         DEVICE uint8 [dst_bytes]; image b is written as H*W*3 bytes of interleaved RGB at dst_off[b] (DEVICE int64
 *               [B]), nothing else.  Grey streams write Y three times (the reference stacks grey images, :129-130)
 *   scratch     DEVICE, >= ssd_jpeg_reconstruct_workspace_bytes(total_coef) bytes (SSD_ERR_WORKSPACE otherwise), 16-byte
 *               aligned, no initial contents needed: the sample planes, one byte per coefficient at the coefficient's offset
 * A record whose planes do not lie inside total_coef, whose grids do not cover W x H for its kind, or whose destination does not
 * lie inside dst_bytes writes nothing (the kernels check; desc lives on the device).  SSD_ERR_VALUE before any launch: a NULL or
 * misaligned pointer, B <= 0, total_coef <= 0 or not a multiple of 64, dst_bytes <= 0.
 * Arithmetic, all integer, >> arithmetic, DS(x, n) = (x + (1 << (n-1))) >> n:
 *   d = coef * q (int32, wrapping).  IDCT: Loeffler-Ligtenberg-Moschytz with 13-bit constants, columns first with DS(., 11), then
 *   rows with DS(., 18), + 128, clamp to [0, 255].  One pass over d0..d7:
 *     z1=(d2+d6)*4433; t2=z1-d6*15137; t3=z1+d2*6270; t0=(d0+d4)<<13; t1=(d0-d4)<<13
 *     t10=t0+t3; t13=t0-t3; t11=t1+t2; t12=t1-t2;  o0=d7; o1=d5; o2=d3; o3=d1
 *     z1=o0+o3; z2=o1+o2; z3=o0+o2; z4=o1+o3; z5=(z3+z4)*9633
 *     o0*=2446; o1*=16819; o2*=25172; o3*=12299; z1*=-7373; z2*=-20995; z3=z3*-16069+z5; z4=z4*-3196+z5
 *     o0+=z1+z3; o1+=z2+z4; o2+=z2+z3; o3+=z1+z4
 *     out0..7 = DS of (t10+o3, t11+o2, t12+o1, t13+o0, t13-o0, t12-o1, t11-o2, t10-o3)
 *   Chroma of 2x1 / 2x2 streams: the plane cropped to cw = ceil(W/2) columns (2x2: and ceil(H/2) rows), edges replicated, then
 *     2x1: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2, first and last column p itself
 *     2x2: r[i] = 3 p[j][i] + p[j-1][i] for row 2j, 3 p[j][i] + p[j+1][i] for row 2j+1; out[2i] = (3 r[i] + r[i-1] + 8) >> 4,
 *          out[2i+1] = (3 r[i] + r[i+1] + 7) >> 4, first column (4 r[0] + 8) >> 4, last column (4 r[cw-1] + 7) >> 4
 *     cw <= 2: plain replication (libjpeg takes its triangle filter only for planes wider than two samples)
 *   Colour, cb and cr minus 128, F(x) = int(x * 65536 + 0.5):  R = Y + ((F(1.402) cr + 32768) >> 16),
 *     G = Y + ((-F(0.34414) cb - F(0.71414) cr + 32768) >> 16),  B = Y + ((F(1.772) cb + 32768) >> 16), each clamped. */
size_t ssd_jpeg_reconstruct_workspace_bytes(long long total_coef);
int ssd_jpeg_reconstruct(const int16_t* coef, const int32_t* desc, int B, uint8_t* dst, const int64_t* dst_off,
                         long long dst_bytes, void* scratch, size_t scratch_bytes, long long total_coef, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SSD_HIP_H */
