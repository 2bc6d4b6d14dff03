// SSD data augmentation on the device: photometric distortion, expand (zoom out), IoU-constrained patch crop and
// horizontal flip, fused with the INTER_LINEAR resize of prep.hip.  The recipe, the Philox slot layout and the bounds contract
// with ssd_match_encode are written out in include/ssd_hip.h; tests/augment_oracle.py restates every float32 operation in
// numpy, in the same order (compiled with -ffp-contract=off, as prep.hip).  Neither the canvas nor the patch is stored: each
// output pixel finds its four taps in canvas coordinates and each tap is either the fill or a distorted source pixel.
#include "common.h"

namespace {

typedef unsigned short bf16_raw;

enum { PH_BRIGHT = 1, PH_CONTRAST = 2, PH_CONTRAST_FIRST = 4, PH_SAT = 8, PH_HUE = 16 };
constexpr int TRIALS = 50;

struct U4 { unsigned x, y, z, w; };

// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; Random123's philox4x32 with R = 10)
__device__ __forceinline__ U4 philox(unsigned long long index, unsigned slot, unsigned block, unsigned long long seed) {
    unsigned c0 = (unsigned)index, c1 = (unsigned)(index >> 32), c2 = slot, c3 = block;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const unsigned lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    }
    return U4{c0, c1, c2, c3};
}

__device__ __forceinline__ float u01(unsigned w) { return (float)(w >> 8) * 0x1p-24f; }          // exact
__device__ __forceinline__ int below(unsigned w, int n) { return (int)(((unsigned long long)w * (unsigned)n) >> 32); }
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// a gt box in canvas pixels: corners and centre (ssd_hip.h step 3)
struct CBox { float x1, y1, x2, y2, cx, cy; };

__device__ __forceinline__ CBox canvas_box(float4 b, float W, float H, float left, float top) {
    CBox c;
    const float hw = b.z * 0.5f, hh = b.w * 0.5f;
    c.x1 = (b.x - hw) * W + left;
    c.x2 = (b.x + hw) * W + left;
    c.y1 = (b.y - hh) * H + top;
    c.y2 = (b.y + hh) * H + top;
    c.cx = b.x * W + left;
    c.cy = b.y * H + top;
    return c;
}

__device__ __forceinline__ bool centre_inside(const CBox& c, int px, int py, int pw, int ph) {
    return (float)px < c.cx && c.cx < (float)(px + pw) && (float)py < c.cy && c.cy < (float)(py + ph);
}

__device__ __forceinline__ float patch_iou(const CBox& c, int px, int py, int pw, int ph) {
    const float qx1 = (float)px, qx2 = (float)(px + pw), qy1 = (float)py, qy2 = (float)(py + ph);
    const float iw = fmaxf(fminf(c.x2, qx2) - fmaxf(c.x1, qx1), 0.f);
    const float ih = fmaxf(fminf(c.y2, qy2) - fmaxf(c.y1, qy1), 0.f);
    const float inter = iw * ih;
    const float ab = (c.x2 - c.x1) * (c.y2 - c.y1);
    const float ap = (float)pw * (float)ph;
    return inter / ((ab + ap) - inter);
}

// Everything of image b up to the crop decision; writes its params record (lane 0).
__device__ void plan_image(int b, int lane, const float4* __restrict__ box, const int* __restrict__ gt_off,
                          const int* __restrict__ src_hw, int stages, unsigned long long seed, long long first_index,
                          ssd_augment_params* __restrict__ params) {
    const unsigned long long idx = (unsigned long long)(first_index + b);
    const int H = src_hw[2 * b], W = src_hw[2 * b + 1];
    const int g0 = gt_off[b], n = gt_off[b + 1] - g0;
    ssd_augment_params p;
    p.stages = stages & SSD_AUG_PHOTO;
    p.reserved[0] = p.reserved[1] = 0;
    // 1. photometric values (slot 0)
    const U4 a = philox(idx, 0, 0, seed), c = philox(idx, 0, 1, seed), h = philox(idx, 0, 2, seed);
    p.delta = (-32.f + u01(a.y) * 64.f) / 255.f;
    p.alpha = 0.5f + u01(a.w);
    p.saturation = 0.5f + u01(c.z);
    p.hue = -18.f + u01(h.x) * 36.f;
    p.photo = (stages & SSD_AUG_PHOTO) ? (int)((a.x >> 31) * PH_BRIGHT | (a.z >> 31) * PH_CONTRAST | (c.x >> 31) * PH_CONTRAST_FIRST |
                                           (c.y >> 31) * PH_SAT | (c.w >> 31) * PH_HUE)
                                   : 0;
    if (!(p.photo & PH_CONTRAST)) p.photo &= ~PH_CONTRAST_FIRST;
    // 2. expand (slot 1)
    const U4 e = philox(idx, 1, 0, seed);
    int CW = W, CH = H, left = 0, top = 0;
    if ((stages & SSD_AUG_EXPAND) && (e.x >> 31)) {
        const float ratio = 1.f + u01(e.y) * 3.f;
        CW = (int)(ratio * (float)W);
        CH = (int)(ratio * (float)H);
        left = below(e.z, CW - W + 1);
        top = below(e.w, CH - H + 1);
        p.stages |= SSD_AUG_EXPAND;
    }
    p.canvas_w = CW; p.canvas_h = CH; p.off_x = left; p.off_y = top;
    // mode + flip (slot 2)
    const U4 m = philox(idx, 2, 0, seed);
    const int mode = (stages & SSD_AUG_CROP) ? below(m.x, 7) : 0;
    p.mode = mode;
    p.flip = (stages & SSD_AUG_FLIP) && (m.y >> 31) ? 1 : 0;
    if (p.flip) p.stages |= SSD_AUG_FLIP;
    // 3. crop search: lane t runs trial t (slot 3 + t)
    int px = 0, py = 0, pw = CW, ph = CH, trial = -1;
    if (mode != 0 && n > 0) {
        int tw = 0, th = 0, tx = 0, ty = 0;
        bool ok = false;
        if (lane < TRIALS) {
            const U4 r = philox(idx, 3 + lane, 0, seed);
            tw = min(max((int)((0.3f + u01(r.x) * 0.7f) * (float)CW), 1), CW);
            th = min(max((int)((0.3f + u01(r.y) * 0.7f) * (float)CH), 1), CH);
            tx = below(r.z, CW - tw + 1);
            ty = below(r.w, CH - th + 1);
            ok = 2 * th >= tw && th <= 2 * tw;
        }
        // every lane tests every box (lanes past the trials and rejected shapes are masked below): lane k loads box k of
        // each 64-box chunk once, the loop broadcasts it with readlane -- no dependent global load per box
        const float need = mode == 1 ? 0.1f : mode == 2 ? 0.3f : mode == 3 ? 0.5f : mode == 4 ? 0.7f : 0.9f;
        bool any_iou = mode == 6, any_ctr = false;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const float4 mine = k0 + lane < n ? box[g0 + k0 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            const int cnt = min(64, n - k0);
            for (int j = 0; j < cnt; ++j) {
                const float4 v = make_float4(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.x), j)),
                                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.y), j)),
                                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.z), j)),
                                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine.w), j)));
                const CBox cb = canvas_box(v, (float)W, (float)H, (float)left, (float)top);
                any_ctr = any_ctr || centre_inside(cb, tx, ty, tw, th);
                any_iou = any_iou || patch_iou(cb, tx, ty, tw, th) >= need;
            }
        }
        ok = ok && any_iou && any_ctr;
        const unsigned long long acc = __ballot(ok);
        if (acc) {
            trial = __ffsll((long long)acc) - 1;
            px = __shfl(tx, trial); py = __shfl(ty, trial); pw = __shfl(tw, trial); ph = __shfl(th, trial);
            p.stages |= SSD_AUG_CROP;
        }
    }
    p.trial = trial;
    p.patch_x = px; p.patch_y = py; p.patch_w = pw; p.patch_h = ph;
    // kept boxes: centre strictly inside the crop, all of them without one
    int kept = n;
    if (trial >= 0) {
        kept = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            bool keep = false;
            if (k < n) keep = centre_inside(canvas_box(box[g0 + k], (float)W, (float)H, (float)left, (float)top), px, py, pw, ph);
            kept += __popcll(__ballot(keep));
        }
    }
    p.n_boxes = kept;
    if (lane == 0) params[b] = p;
}

// Kept boxes of image b, compacted in input order at out_off (reads the record k_augment_plan wrote).
__device__ void write_boxes(int b, int lane, const float4* __restrict__ box, const float* __restrict__ cls,
                            const int* __restrict__ gt_off, const int* __restrict__ src_hw, const ssd_augment_params* params,
                            int out_off, float4* __restrict__ box_out, float* __restrict__ cls_out) {
    const ssd_augment_params& p = params[b];
    const int H = src_hw[2 * b], W = src_hw[2 * b + 1];
    const int g0 = gt_off[b], n = gt_off[b + 1] - g0;
    const bool crop = p.trial >= 0, geom = (p.stages & (SSD_AUG_EXPAND | SSD_AUG_CROP)) != 0, flip = p.flip != 0;
    const int px = p.patch_x, py = p.patch_y, pw = p.patch_w, ph = p.patch_h;
    const float fpx = (float)px, fpy = (float)py, fpx2 = (float)(px + pw), fpy2 = (float)(py + ph);
    const float fpw = (float)pw, fph = (float)ph;
    int base = out_off;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        bool keep = false;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < n) {
            v = box[g0 + k];
            const CBox cb = canvas_box(v, (float)W, (float)H, (float)p.off_x, (float)p.off_y);
            keep = !crop || centre_inside(cb, px, py, pw, ph);
            if (geom) {
                const float rx1 = (fmaxf(cb.x1, fpx) - fpx) / fpw, rx2 = (fminf(cb.x2, fpx2) - fpx) / fpw;
                const float ry1 = (fmaxf(cb.y1, fpy) - fpy) / fph, ry2 = (fminf(cb.y2, fpy2) - fpy) / fph;
                v = make_float4((rx1 + rx2) * 0.5f, (ry1 + ry2) * 0.5f, rx2 - rx1, ry2 - ry1);
            }
            if (flip) v.x = 1.f - v.x;
        }
        const unsigned long long bal = __ballot(keep);
        if (keep) {
            const int dst = base + __popcll(bal & ((1ull << lane) - 1ull));
            box_out[dst] = v;
            cls_out[dst] = cls[g0 + k];
        }
        base += __popcll(bal);
    }
}

__global__ __launch_bounds__(256) void k_augment_plan(const float4* __restrict__ box, const int* __restrict__ gt_off,
                                                      const int* __restrict__ src_hw, int B, int stages,
                                                      unsigned long long seed, long long first_index,
                                                      ssd_augment_params* __restrict__ params) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b < B) plan_image(b, threadIdx.x & 63, box, gt_off, src_hw, stages, seed, first_index, params);
}

// second launch, one wave per image: its output offset = sum of the kept counts of the images before it (each wave sums
// them itself -- no cross-wave scan), its boxes, off_out, and its share of the zero rows after the kept ones
__global__ __launch_bounds__(256) void k_augment_boxes(const float4* __restrict__ box, const float* __restrict__ cls,
                                                       const int* __restrict__ gt_off, const int* __restrict__ src_hw,
                                                       int B, int total_gt, const ssd_augment_params* __restrict__ params,
                                                       float4* __restrict__ box_out, float* __restrict__ cls_out,
                                                       int* __restrict__ off_out) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    int before = 0, all = 0;
    for (int j = lane; j < B; j += 64) {
        const int c = params[j].n_boxes;
        all += c;
        before += j < b ? c : 0;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        before += __shfl_xor(before, m);
        all += __shfl_xor(all, m);
    }
    if (lane == 0) {
        off_out[b] = before;
        if (b == B - 1) off_out[B] = all;
    }
    write_boxes(b, lane, box, cls, gt_off, src_hw, params, before, box_out, cls_out);
    for (int r = all + b * 64 + lane; r < total_gt; r += B * 64) {      // finite rows up to the old total
        box_out[r] = make_float4(0.f, 0.f, 0.f, 0.f);
        cls_out[r] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------------ image
__device__ __forceinline__ bf16_raw f2bf_rn(float f) {
    unsigned u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);                        // round to nearest even (inputs are finite)
    return (bf16_raw)(u >> 16);
}

// prep.hip's src_coord: cv2 INTER_LINEAR source taps of destination index d, clamped inside [0, n-1]
__device__ __forceinline__ void src_coord(int d, double scale, int n, int& s0, int& s1, float& f) {
    float fx = (float)__dadd_rn(__dmul_rn((double)d + 0.5, scale), -0.5);
    int s = (int)floorf(fx);
    fx -= (float)s;
    if (s < 0) { s = 0; fx = 0.f; }
    if (s >= n - 1) { s = n - 1; fx = 0.f; }
    s0 = s;
    s1 = s + 1 < n ? s + 1 : n - 1;
    f = fx;
}

__device__ __forceinline__ void contrast(float& r, float& g, float& b, float alpha) {
    r = clamp01(r * alpha); g = clamp01(g * alpha); b = clamp01(b * alpha);
}

// ssd_hip.h step 1 on one pixel
__device__ void distort(float& r, float& g, float& b, int photo, float delta, float alpha, float sat, float hue) {
    if (photo & PH_BRIGHT) { r = clamp01(r + delta); g = clamp01(g + delta); b = clamp01(b + delta); }
    if ((photo & PH_CONTRAST) && (photo & PH_CONTRAST_FIRST)) contrast(r, g, b, alpha);
    if (photo & (PH_SAT | PH_HUE)) {
        // branch-free: the selects pick the operands, each division runs once (the per-pixel branches diverged)
        const float v = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b), d = v - mn;
        float s = d / (v > 0.f ? v : 1.f);
        s = v > 0.f ? s : 0.f;
        const int sec = v == r ? 0 : v == g ? 1 : 2;
        const float num = sec == 0 ? g - b : sec == 1 ? b - r : r - g;
        const float hh = 60.f * (num / (d == 0.f ? 1.f : d));
        float h = sec == 0 ? hh : sec == 1 ? 120.f + hh : 240.f + hh;
        h = d == 0.f ? 0.f : h;
        h = h < 0.f ? h + 360.f : h;
        if (photo & PH_SAT) s = clamp01(s * sat);
        if (photo & PH_HUE) {
            h = h + hue;
            h = h >= 360.f ? h - 360.f : (h < 0.f ? h + 360.f : h);
        }
        const float q6 = h / 60.f;
        int i = (int)floorf(q6);
        const float f = q6 - (float)i;
        i = i >= 6 ? 0 : i;
        const float pp = v * (1.f - s), qq = v * (1.f - s * f), tt = v * (1.f - s * (1.f - f));
        // sectors 0..5: (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v) (v,p,q)
        r = (i == 0 || i == 5) ? v : i == 1 ? qq : i == 4 ? tt : pp;
        g = (i == 1 || i == 2) ? v : i == 0 ? tt : i == 3 ? qq : pp;
        b = (i == 3 || i == 4) ? v : i == 2 ? tt : i == 5 ? qq : pp;
        r = clamp01(r); g = clamp01(g); b = clamp01(b);
    }
    if ((photo & PH_CONTRAST) && !(photo & PH_CONTRAST_FIRST)) contrast(r, g, b, alpha);
}

__global__ void k_augment_image(const void* __restrict__ src, int kind, const long long* __restrict__ src_off,
                                const int* __restrict__ src_hw, const ssd_augment_params* __restrict__ params,
                                bf16_raw* __restrict__ out, int S, int normalize) {
    __shared__ float lut[256];                               // u8 / 255 as ssd_image_resize_prep
    lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
    __syncthreads();
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * S) return;
    const ssd_augment_params& p = params[b];
    const int H = src_hw[2 * b], W = src_hw[2 * b + 1];
    const int dy = i / S, dx0 = i - dy * S;
    const int dx = p.flip ? S - 1 - dx0 : dx0;
    int x0, x1, y0, y1;
    float fx, fy;
    src_coord(dx, (double)p.patch_w / (double)S, p.patch_w, x0, x1, fx);
    src_coord(dy, (double)p.patch_h / (double)S, p.patch_h, y0, y1, fy);
    const int sx[2] = {p.patch_x + x0 - p.off_x, p.patch_x + x1 - p.off_x};
    const int sy[2] = {p.patch_y + y0 - p.off_y, p.patch_y + y1 - p.off_y};
    const unsigned char* img8 = static_cast<const unsigned char*>(src) + (kind == 0 ? src_off[b] : 0);
    const float* img32 = static_cast<const float*>(src) + (kind == 1 ? (src_off ? src_off[b] : (long long)b * H * W * 3) : 0);
    const int photo = p.photo;
    float t[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int yy = sy[k >> 1], xx = sx[k & 1];
        if (xx < 0 || xx >= W || yy < 0 || yy >= H) {
            t[k][0] = (float)(123.0 / 255.0); t[k][1] = (float)(117.0 / 255.0); t[k][2] = (float)(104.0 / 255.0);
            continue;
        }
        const long long o = ((long long)yy * W + xx) * 3;
        if (kind == 0) {
            t[k][0] = lut[img8[o]]; t[k][1] = lut[img8[o + 1]]; t[k][2] = lut[img8[o + 2]];
        } else {
            t[k][0] = img32[o]; t[k][1] = img32[o + 1]; t[k][2] = img32[o + 2];
        }
        if (photo) distort(t[k][0], t[k][1], t[k][2], photo, p.delta, p.alpha, p.saturation, p.hue);
    }
    const float ax0 = 1.f - fx, ay0 = 1.f - fy;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float h0 = __fadd_rn(__fmul_rn(t[0][c], ax0), __fmul_rn(t[1][c], fx));
        const float h1 = __fadd_rn(__fmul_rn(t[2][c], ax0), __fmul_rn(t[3][c], fx));
        float r = __fadd_rn(__fmul_rn(h0, ay0), __fmul_rn(h1, fy));
        if (normalize) r = __fmul_rn(__fadd_rn(r, -0.5f), 2.f);
        v[c] = r;
    }
    *reinterpret_cast<uint4*>(out + ((long long)b * S * S + i) * 8) =
        make_uint4((unsigned)f2bf_rn(v[0]) | ((unsigned)f2bf_rn(v[1]) << 16), (unsigned)f2bf_rn(v[2]), 0u, 0u);
}

}  // namespace

extern "C" {

int ssd_augment_plan(const float* box, const float* cls, const int32_t* gt_off, const int32_t* src_hw, int B, int total_gt,
                     int stages, uint64_t seed, int64_t first_index, ssd_augment_params* params, float* box_out,
                     float* cls_out, int32_t* off_out, void* stream) {
    if (!gt_off || !src_hw || !params || !off_out || B <= 0 || total_gt < 0 || (stages & ~SSD_AUG_ALL)) return SSD_ERR_VALUE;
    if (total_gt > 0 && (!box || !cls || !box_out || !cls_out)) return SSD_ERR_VALUE;
    const dim3 grid((unsigned)((B + 3) / 4));
    hipLaunchKernelGGL(k_augment_plan, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(box), gt_off,
                       src_hw, B, stages, (unsigned long long)seed, (long long)first_index, params);
    if (hipGetLastError() != hipSuccess) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(k_augment_boxes, grid, dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(box), cls,
                       gt_off, src_hw, B, total_gt, params, reinterpret_cast<float4*>(box_out), cls_out, off_out);
    return ssd_launch_status();
}

int ssd_augment_image(const void* src, int src_kind, const int64_t* src_off, const int32_t* src_hw,
                      const ssd_augment_params* params, void* out, int B, int S, int normalize, void* stream) {
    if (!src || !src_hw || !params || !out || B <= 0 || S <= 0 || (src_kind != 0 && src_kind != 1)) return SSD_ERR_VALUE;
    if (src_kind == 0 && !src_off) return SSD_ERR_VALUE;
    hipLaunchKernelGGL(k_augment_image, dim3((unsigned)((S * S + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       src, src_kind, reinterpret_cast<const long long*>(src_off), src_hw, params, static_cast<bf16_raw*>(out),
                       S, normalize);
    return ssd_launch_status();
}

}  // extern "C"
