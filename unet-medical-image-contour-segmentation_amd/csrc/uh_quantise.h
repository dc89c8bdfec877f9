// uh_quantise.h -- the 24-bit quantised probability that tta.hip and tiling.hip add as integers (DESIGN.md section 3 "Test-time
// augmentation", "Tiled prediction"): the fp32 softmax over the classes of a pixel's logits (one class: the sigmoid), then
// q = (uint32) rintf(p * 2^24).  Both merges call these functions, so a tile and a view of the same logits get the same q.
#pragma once
#include "uh_common.h"

constexpr float TTA_ONE = 16777216.0f;          // 2^24: the unit of a quantised probability

__device__ __forceinline__ unsigned tta_quantise(float p) { return (unsigned)rintf(p * TTA_ONE); }

// NC <= 4, everything in registers: q[c] of the NC logits at p
template <typename T, int NC>
__device__ __forceinline__ void tta_quantised_probs(const T* __restrict__ p, unsigned (&q)[NC]) {
    float l[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) l[c] = uh_to_f32(p[c]);
    if (NC == 1) {
        q[0] = tta_quantise(1.0f / (1.0f + expf(-l[0])));
    } else {
        float m = l[0];
#pragma unroll
        for (int c = 1; c < NC; ++c) m = fmaxf(m, l[c]);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) { l[c] = expf(l[c] - m); s += l[c]; }
#pragma unroll
        for (int c = 0; c < NC; ++c) q[c] = tta_quantise(l[c] / s);
    }
}

// any class count (> 1): the maximum and the denominator of the NC logits at p first, then class by class
template <typename T>
__device__ __forceinline__ void tta_softmax_stats(const T* __restrict__ p, int NC, float& mx, float& den) {
    float m = uh_to_f32(p[0]);
    for (int c = 1; c < NC; ++c) m = fmaxf(m, uh_to_f32(p[c]));
    float s = 0.f;
    for (int c = 0; c < NC; ++c) s += expf(uh_to_f32(p[c]) - m);
    mx = m;
    den = s;
}

template <typename T>
__device__ __forceinline__ unsigned tta_quantised_prob(T logit, float mx, float den) {
    return tta_quantise(expf(uh_to_f32(logit) - mx) / den);
}
