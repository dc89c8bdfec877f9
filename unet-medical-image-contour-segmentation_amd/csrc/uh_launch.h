// Host side of the pixel passes (bn.hip, bn_fused.hip, pool_up.hip, the 1x1 half of convt_1x1.hip, spatial_attn.hip): one launch
// plan -- vector form, hoisted coefficients, clamped flat grid -- and the dispatch over its forms.
#pragma once
#include <type_traits>
#include "uh_vec.h"

// Workgroups (of 256 threads) a flat grid-stride pass may ask for: 16 per CU for the BatchNorm, pool and upsample passes, 32 per CU
// for the 1x1 conv and the spatial-attention passes -- the values each pass was measured with; nothing in the kernels depends on them.
constexpr int UH_GRID_CAP = 256 * 16, UH_GRID_CAP_1X1 = 256 * 32;

static inline unsigned uh_flat_grid(int64_t total, int cap) {
    int64_t g = (total + 255) / 256;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// every (pointer, pixel stride) pair can be walked in 16-byte channel groups; a null (optional) pointer passes
template <typename T>
static inline bool uh_all_vec_ok(int) { return true; }
template <typename T, typename... Rest>
static inline bool uh_all_vec_ok(int C, const void* p, int ld, Rest... rest) {
    return (!p || uh_vec_ok<T>(p, ld, C)) && uh_all_vec_ok<T>(C, rest...);
}

// Thread = (item, channel group): an item is a pixel or a 2x2 window, a group is `vec` channels (16 bytes, or 1 channel in the
// scalar form).  hoist: the grid stride is a multiple of the group count, so a thread stays on the channel group it starts on
// and may keep that group's coefficients in registers.  Once the grid is capped a thread walks more than one element: a hoisting
// kernel launched without this condition computes with the wrong channels' coefficients.
struct PixelPass { int vec; bool hoist; unsigned grid; };

static inline PixelPass uh_pixel_pass(int64_t items, int C, int elem_size, bool all_vec_ok, int cap) {
    PixelPass p;
    p.vec = all_vec_ok ? 16 / elem_size : 1;
    const int G = C / p.vec;
    p.grid = uh_flat_grid(items * G, cap);
    p.hoist = all_vec_ok && ((int64_t)p.grid * 256) % G == 0;
    return p;
}

// f(V, HOIST) as integral constants for the plan's form: (VEC, true), (VEC, false) or (1, false) -- a scalar kernel never hoists.
// SCALAR = false: the entry point has refused the scalar form (UH_REQUIRE) and none is instantiated.  A kernel without a HOIST
// parameter ignores the second argument.
template <int VEC, bool SCALAR = true, typename F>
static inline void uh_pixel_launch(const PixelPass& p, F&& f) {
    if (p.vec == 1) {
        if constexpr (SCALAR) f(std::integral_constant<int, 1>{}, std::false_type{});
    } else if (p.hoist)
        f(std::integral_constant<int, VEC>{}, std::true_type{});
    else
        f(std::integral_constant<int, VEC>{}, std::false_type{});
}

// f(NC) with NC = ncls for ncls in 1 .. MAXC - 1, NC = MAXC for anything else (the entry points have checked the range)
template <int MAXC, int N = 1, typename F>
static inline void uh_class_dispatch(int ncls, F&& f) {
    if constexpr (N == MAXC)
        f(std::integral_constant<int, N>{});
    else if (ncls == N)
        f(std::integral_constant<int, N>{});
    else
        uh_class_dispatch<MAXC, N + 1>(ncls, f);
}

// ... and f(NC, LPP) for the head shape: C = LPP 16-byte groups, LPP = 8 or 16 lanes per pixel
template <int MAXC, typename F>
static inline void uh_head_dispatch(int ncls, int groups, F&& f) {
    uh_class_dispatch<MAXC>(ncls, [&](auto nc) {
        if (groups == 8) f(nc, std::integral_constant<int, 8>{});
        else f(nc, std::integral_constant<int, 16>{});
    });
}

// grid of the head-shape kernels: a workgroup trip covers four pixels per lane group
static inline unsigned uh_head_grid(int64_t npix, int LPP, int cap) {
    const int ppb4 = 4 * (256 / LPP);
    return uh_flat_grid((npix + ppb4 - 1) / ppb4 * 256, cap);
}

// bn.hip (internal): partials [nblk][2][C] -> dgamma, dbeta; the first step of every *_bwd_apply entry point that is given partial rows
int uh_bn_bwd_finalize_launch(const float* partials, int nblk, int C, float* dgamma, float* dbeta, hipStream_t st);

// 1 / n of the BatchNorm backward: n_total where the statistics span more than this call's pixels (SyncBN), else npix
static inline float uh_inv_n(int64_t n_total, int64_t npix) { return (float)(1.0 / (double)(n_total > 0 ? n_total : npix)); }

// log2 of a power of two below 2^24, -1 for anything else
static inline int uh_log2_exact(int G) {
    for (int k = 0; k < 24; ++k)
        if ((1 << k) == G) return k;
    return -1;
}
