// The box term the losses normalised by the positives share (multibox.hip, softmax_focal.hip): smooth L1 of a positive's four
// offsets and its gradient, or one of the IoU losses (GIoU, DIoU, CIoU; include/ssd_hip.h) of the decoded boxes.  One definition,
// so that both losses' dloc agree bit for bit on the same inputs.
#pragma once
#include "rowblock.h"
#include "ssd_hip.h"

__device__ __forceinline__ float smooth_l1(float d) {
    const float a = fabsf(d);
    return a < 1.f ? 0.5f * d * d : a - 0.5f;
}

__device__ __forceinline__ float clamp1(float d) { return fminf(fmaxf(d, -1.f), 1.f); }

// grad_scale * loc_weight / P, the factor of every dloc element (0 without positives)
__device__ __forceinline__ float box_scale(float grad_scale, float loc_weight, int P) {
    return P > 0 ? grad_scale * loc_weight / (float)P : 0.f;
}

// sum_4 smoothL1(loc - gt_loc) of one positive
template <typename T>
__device__ __forceinline__ double box_loss(const T* __restrict__ pl, float4 gl) {
    return (double)smooth_l1(to_f32<T>(pl[0]) - gl.x) + (double)smooth_l1(to_f32<T>(pl[1]) - gl.y) +
           (double)smooth_l1(to_f32<T>(pl[2]) - gl.z) + (double)smooth_l1(to_f32<T>(pl[3]) - gl.w);
}

// scale * clamp(loc - gt_loc, -1, 1) of one positive
template <typename T>
__device__ __forceinline__ float4 box_grad(const T* __restrict__ pl, float4 gl, float scale) {
    return make_float4(scale * clamp1(to_f32<T>(pl[0]) - gl.x), scale * clamp1(to_f32<T>(pl[1]) - gl.y),
                       scale * clamp1(to_f32<T>(pl[2]) - gl.z), scale * clamp1(to_f32<T>(pl[3]) - gl.w));
}

// ------------------------------------------------------------------------------------------------
// The IoU kinds.  One positive: its loss (returned) and dL/dt of its four offsets (*grad, unscaled), in one pass, f32.  Both boxes
// are decoded relative to the prior's centre (the losses are translation invariant), so only the prior's size `pwh` is read.
// A max / min passes its gradient to the predicted coordinate under the strict comparison only, max(0, .) where its argument
// is > 0, the clamp of t2 / t3 where |t| < W.  NaN where an offset, the prior's size, the loss or a gradient component is not
// finite (status 3 is read off the sums).  Contraction is off inside: every kernel that inlines this computes the same bits.
constexpr float BOX_W_CLAMP = 4.135166556742356f;                 // log(1000 / 16), ssd_score_decode's bound

template <typename T>
__device__ __forceinline__ float box_iou(int kind, const T* __restrict__ pl, float4 gl, const double* __restrict__ pwh,
                                         float4* __restrict__ grad) {
#pragma clang fp contract(off)
    const float t0 = to_f32<T>(pl[0]), t1 = to_f32<T>(pl[1]), t2 = to_f32<T>(pl[2]), t3 = to_f32<T>(pl[3]);
    const float dw = (float)pwh[0], dh = (float)pwh[1];
    const float W = BOX_W_CLAMP;
    const float cx = t0 * dw, cy = t1 * dh;
    const float w = dw * expf(fminf(fmaxf(t2, -W), W)), h = dh * expf(fminf(fmaxf(t3, -W), W));
    const float gx = gl.x * dw, gy = gl.y * dh;
    const float gw = dw * expf(fminf(fmaxf(gl.z, -W), W)), gh = dh * expf(fminf(fmaxf(gl.w, -W), W));
    const float x1 = cx - 0.5f * w, x2 = cx + 0.5f * w, y1 = cy - 0.5f * h, y2 = cy + 0.5f * h;
    const float X1 = gx - 0.5f * gw, X2 = gx + 0.5f * gw, Y1 = gy - 0.5f * gh, Y2 = gy + 0.5f * gh;
    const float iwr = fminf(x2, X2) - fmaxf(x1, X1), ihr = fminf(y2, Y2) - fmaxf(y1, Y1);
    const float iw = fmaxf(0.f, iwr), ih = fmaxf(0.f, ihr);
    const float I = iw * ih, U = (w * h + gw * gh) - I, iou = I / U;
    const float cw = fmaxf(x2, X2) - fminf(x1, X1), ch = fmaxf(y2, Y2) - fminf(y1, Y1);
    // derivatives of iw, ih, cw, ch with respect to (centre, size) of their axis: corner indicators a (intersection), b (hull)
    const float ax2 = (iwr > 0.f && x2 < X2) ? 1.f : 0.f, ax1 = (iwr > 0.f && x1 > X1) ? 1.f : 0.f;
    const float ay2 = (ihr > 0.f && y2 < Y2) ? 1.f : 0.f, ay1 = (ihr > 0.f && y1 > Y1) ? 1.f : 0.f;
    const float bx2 = x2 > X2 ? 1.f : 0.f, bx1 = x1 < X1 ? 1.f : 0.f, by2 = y2 > Y2 ? 1.f : 0.f, by1 = y1 < Y1 ? 1.f : 0.f;
    // order of the four: cx, cy, w, h
    const float dI[4] = {ih * (ax2 - ax1), iw * (ay2 - ay1), 0.5f * ih * (ax2 + ax1), 0.5f * iw * (ay2 + ay1)};
    const float dA[4] = {0.f, 0.f, h, w};
    const float dcw[4] = {bx2 - bx1, 0.f, 0.5f * (bx2 + bx1), 0.f};
    const float dch[4] = {0.f, by2 - by1, 0.f, 0.5f * (by2 + by1)};
    float L = 1.f - iou;
    float dq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) dq[k] = -((dI[k] * U - I * (dA[k] - dI[k])) / (U * U));
    if (kind == SSD_BOX_GIOU) {
        const float Cc = cw * ch;
        L += (Cc - U) / Cc;
#pragma unroll
        for (int k = 0; k < 4; ++k) dq[k] += (U * (dcw[k] * ch + cw * dch[k]) - Cc * (dA[k] - dI[k])) / (Cc * Cc);
    } else {
        const float ex = cx - gx, ey = cy - gy;
        const float rho2 = ex * ex + ey * ey, c2 = cw * cw + ch * ch;
        L += rho2 / c2;
        const float dr[4] = {2.f * ex, 2.f * ey, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) dq[k] += (dr[k] * c2 - rho2 * (2.f * cw * dcw[k] + 2.f * ch * dch[k])) / (c2 * c2);
        if (kind == SSD_BOX_CIOU) {
            const float kpi = 0.4052847345693511f;                // 4 / pi^2
            const float da = atanf(gw / gh) - atanf(w / h);
            const float v = kpi * da * da;
            const float alpha = v > 0.f ? v / ((1.f - iou) + v) : 0.f;   // a constant in the gradient
            L += alpha * v;
            const float s = alpha * (2.f * kpi) * da / (w * w + h * h);  // dv/dw = -2 k da h / (w^2 + h^2), dv/dh = +2 k da w / (..)
            dq[2] -= s * h;
            dq[3] += s * w;
        }
    }
    const float g0 = dw * dq[0], g1 = dh * dq[1];
    const float g2 = fabsf(t2) < W ? w * dq[2] : 0.f, g3 = fabsf(t3) < W ? h * dq[3] : 0.f;
    *grad = make_float4(g0, g1, g2, g3);
    const float big = INFINITY;
    const bool ok = fabsf(t0) < big && fabsf(t1) < big && fabsf(t2) < big && fabsf(t3) < big && fabsf(gl.x) < big &&
                    fabsf(gl.y) < big && fabsf(gl.z) < big && fabsf(gl.w) < big && dw > 0.f && dh > 0.f && dw < big && dh < big &&
                    fabsf(L) < big && fabsf(g0) < big && fabsf(g1) < big && fabsf(g2) < big && fabsf(g3) < big;
    return ok ? L : NAN;
}

// The box kind and the priors of a call.  They travel behind every other kernel argument, so that the smooth-L1 instantiations
// keep the argument layout -- and with it the code -- they had before there were kinds.
struct BoxArgs {
    int kind;                                // SSD_BOX_*
    const double* priors;                    // [A*4], read by the IoU kinds only
};

// One positive at flat anchor index g under an IoU kind: its loss, and scale * dL/dt in *d.  Reads the size of prior g % A.
template <typename T>
__device__ __forceinline__ double box_term(const BoxArgs& bx, int A, size_t g, const T* __restrict__ pl, float4 gl, float scale,
                                           float4* __restrict__ d) {
    float4 u;
    const float L = box_iou<T>(bx.kind, pl, gl, bx.priors + 4 * (g % (size_t)A) + 2, &u);
    *d = make_float4(scale * u.x, scale * u.y, scale * u.z, scale * u.w);
    return (double)L;
}
