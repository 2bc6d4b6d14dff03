// The box term the losses normalised by the positives share (multibox.hip, softmax_focal.hip): smooth L1 of a positive's four
// offsets and its gradient.  One definition, so that both losses' dloc agree bit for bit on the same inputs.
#pragma once
#include "rowblock.h"

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
