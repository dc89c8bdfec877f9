// uh_union_find.h -- batched union-find connected-component labelling over pixel indices, shared by post_process.hip
// (mask post-processing) and seg_pipeline.hip (external contours).  atomicMin links towards the smaller index, so each
// component's root is its minimum pixel index -- the raster-first pixel -- whatever the schedule.  Kernels live in an
// anonymous namespace: every source that includes this header gets its own copy.
#pragma once
#include "uh_common.h"

namespace {

__device__ __forceinline__ int pp_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int pp_find(const int* L, int x) {
    int p = pp_load(L + x);
    while (p != x) { x = p; p = pp_load(L + x); }
    return x;
}
__device__ __forceinline__ void pp_unite(int* L, int a, int b) {
    for (;;) {
        a = pp_find(L, a);
        b = pp_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }          // link the larger root under the smaller
        const int old = atomicMin(L + b, a);
        if (old == b) return;
        b = old;                                               // somebody re-linked b meanwhile: retry from there
    }
}

// sel[p] = 1 where the pixel belongs to the set being labelled
__global__ void pp_init_kernel(const unsigned char* __restrict__ sel, int* __restrict__ L, int* __restrict__ aux, long long n) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    L[p] = sel[p] ? (int)p : -1;
    aux[p] = 0;
}
// CONN8 = false: 4-connectivity (W, N); true: 8-connectivity (W, NW, N, NE)
template <bool CONN8>
__global__ void pp_union_kernel(const unsigned char* __restrict__ sel, int* __restrict__ L, int H, int W, long long n) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n || !sel[p]) return;
    const int x = (int)(p % W), y = (int)((p / W) % H);
    if (x > 0 && sel[p - 1]) pp_unite(L, (int)p, (int)p - 1);
    if (y > 0) {
        if (sel[p - W]) pp_unite(L, (int)p, (int)p - W);
        if (CONN8) {
            if (x > 0 && sel[p - W - 1]) pp_unite(L, (int)p, (int)p - W - 1);
            if (x + 1 < W && sel[p - W + 1]) pp_unite(L, (int)p, (int)p - W + 1);
        }
    }
}
// root[p] = representative; MODE 0: mark components that touch the image border, MODE 1: count pixels per component
template <int MODE>
__global__ void pp_flatten_kernel(const int* __restrict__ L, int* __restrict__ root, int* __restrict__ aux, int H, int W,
                                  long long n) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    int r = -1;
    if (L[p] >= 0) {
        r = pp_find(L, (int)p);
        if (MODE == 0) {
            const int x = (int)(p % W), y = (int)((p / W) % H);
            if (x == 0 || y == 0 || x == W - 1 || y == H - 1) aux[r] = 1;
        } else {
            atomicAdd(aux + r, 1);
        }
    }
    root[p] = r;
}

}  // namespace
