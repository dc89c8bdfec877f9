// ensemble.hip -- checkpoint ensembles (DESIGN.md section 3 "Ensembles"): the members' quantised probabilities, or the integer
// sums the two merges (tta.hip, tiling.hip) export for a member, are added per pixel and class with an integer weight per member.
//   uh_ensemble_add     acc = (first ? 0 : acc) + weight s, s the member's q (logits), its uint32 view sums or its uint64 tile sums
//   uh_ensemble_finish  acc -> the first maximum, the quotient acc / T, the confidence floor(255 max / sum)
// The work is pixel-wise and has no geometry: every array is flat, [npix][NC].  Nothing here synchronises with the host,
// allocates or uses an atomic; no float enters a sum, so the result depends on no order of the members.
#include "uh_common.h"
#include "uh_launch.h"
#include "uh_quantise.h"

namespace {

typedef unsigned long long u64;

constexpr int ENS_GRID_CAP = UH_GRID_CAP;       // 16 workgroups per CU, as the other streaming pixel passes

// N values of U from / to p.  AL: p is 16-byte aligned and N sizeof(U) a multiple of 16 (the host has checked both), so the copy
// is N sizeof(U) / 16 16-byte accesses; otherwise element by element.
template <typename U, int N, bool AL>
__device__ __forceinline__ void ens_load(const U* __restrict__ p, U (&v)[N]) {
    if constexpr (AL) {
        static_assert((N * sizeof(U)) % 16 == 0, "a wide group is whole 16-byte units");
        __builtin_memcpy(v, __builtin_assume_aligned(p, 16), N * sizeof(U));
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = p[i];
    }
}
template <typename U, int N, bool AL>
__device__ __forceinline__ void ens_store(U* __restrict__ p, const U (&v)[N]) {
    if constexpr (AL) {
        static_assert((N * sizeof(U)) % 16 == 0, "a wide group is whole 16-byte units");
        __builtin_memcpy(__builtin_assume_aligned(p, 16), v, N * sizeof(U));
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = v[i];
    }
}

// pixels a thread takes at a time so that its logits are whole 16-byte units: the smallest P with P NC sizeof(T) % 16 == 0
__host__ __device__ constexpr int ens_group(int nc_bytes) {
    int p = 1;
    while ((p * nc_bytes) % 16) p *= 2;
    return p;
}

// ------------------------------------------------------------------------------------------------------------ add
// Logits, NC <= 4, everything in registers.  A thread takes P consecutive pixels: P NC logits in 16-byte loads, the quantiser
// of uh_quantise.h per pixel, P NC 64-bit sums in 16-byte loads and stores.  The npix % P pixels behind the last whole group
// go element by element (P = 1, AL = false: also the form of a base that is not 16-byte aligned).
template <typename T, int NC, int P, bool AL>
__device__ __forceinline__ void ens_add_group(const T* __restrict__ src, u64* __restrict__ acc, unsigned weight, bool first) {
    T l[P * NC];
    ens_load<T, P * NC, AL>(src, l);
    u64 a[P * NC];
    if (!first) ens_load<u64, P * NC, AL>(acc, a);
#pragma unroll
    for (int j = 0; j < P; ++j) {
        T lp[NC];
        unsigned q[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) lp[c] = l[j * NC + c];
        tta_quantised_probs<T, NC>(lp, q);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const u64 t = (u64)weight * q[c];
            a[j * NC + c] = first ? t : a[j * NC + c] + t;
        }
    }
    ens_store<u64, P * NC, AL>(acc, a);
}

template <typename T, int NC, int P>
__global__ __launch_bounds__(256) void ens_add_logits_kernel(const T* __restrict__ src, int64_t npix, unsigned weight, int first,
                                                              u64* __restrict__ acc) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t groups = npix / P;
    for (int64_t g = tid; g < groups; g += stride)
        ens_add_group<T, NC, P, (P > 1)>(src + g * (P * NC), acc + g * (P * NC), weight, first != 0);
    if (P > 1) {
        const int64_t pix = groups * P + tid;                        // the tail: fewer than P pixels
        if (pix < npix) ens_add_group<T, NC, 1, false>(src + pix * NC, acc + pix * NC, weight, first != 0);
    }
}

// logits, any class count: the maximum and the denominator of the pixel first, then class by class
template <typename T>
__global__ __launch_bounds__(256) void ens_add_logits_generic_kernel(const T* __restrict__ src, int64_t npix, int NC, unsigned weight,
                                                                      int first, u64* __restrict__ acc) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += stride) {
        const T* __restrict__ p = src + pix * NC;
        u64* __restrict__ a = acc + pix * NC;
        float mx, den;
        tta_softmax_stats<T>(p, NC, mx, den);
        for (int c = 0; c < NC; ++c) {
            const u64 t = (u64)weight * tta_quantised_prob<T>(p[c], mx, den);
            a[c] = first ? t : a[c] + t;
        }
    }
}

// Integer sums (uint32 of uh_tta_merge, uint64 of uh_tile_merge): no class depends on another, so the arrays are walked flat, four
// elements per thread -- 16 (uint32) or 32 (uint64) bytes of source, 32 bytes of sums in 16-byte accesses -- whatever NC is.
// VEC = 1: element by element (a base that is not 16-byte aligned); the n % 4 elements behind the last group likewise.
template <typename S, int VEC>
__global__ __launch_bounds__(256) void ens_add_sums_kernel(const S* __restrict__ src, int64_t n, unsigned weight, int first,
                                                            u64* __restrict__ acc) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t groups = n / VEC;
    for (int64_t g = tid; g < groups; g += stride) {
        S s[VEC];
        u64 a[VEC];
        ens_load<S, VEC, (VEC > 1)>(src + g * VEC, s);
        if (!first) ens_load<u64, VEC, (VEC > 1)>(acc + g * VEC, a);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const u64 t = (u64)weight * (u64)s[i];
            a[i] = first ? t : a[i] + t;
        }
        ens_store<u64, VEC, (VEC > 1)>(acc + g * VEC, a);
    }
    if (VEC > 1) {
        const int64_t i = groups * VEC + tid;
        if (i < n) {
            const u64 t = (u64)weight * (u64)src[i];
            acc[i] = first ? t : acc[i] + t;
        }
    }
}

template <typename T>
void ens_launch_add_logits(const T* src, int64_t npix, int NC, unsigned weight, int first, u64* acc, bool aligned, hipStream_t st) {
    if (NC > 4) {
        hipLaunchKernelGGL((ens_add_logits_generic_kernel<T>), dim3(uh_flat_grid(npix, ENS_GRID_CAP)), dim3(256), 0, st, src, npix,
                           NC, weight, first, acc);
        return;
    }
    uh_class_dispatch<4>(NC, [&](auto nc) {
        constexpr int C = decltype(nc)::value;
        constexpr int P = ens_group(C * (int)sizeof(T));
        if (aligned) {
            const unsigned grid = uh_flat_grid((npix + P - 1) / P, ENS_GRID_CAP);
            hipLaunchKernelGGL((ens_add_logits_kernel<T, C, P>), dim3(grid), dim3(256), 0, st, src, npix, weight, first, acc);
        } else {
            hipLaunchKernelGGL((ens_add_logits_kernel<T, C, 1>), dim3(uh_flat_grid(npix, ENS_GRID_CAP)), dim3(256), 0, st, src, npix,
                               weight, first, acc);
        }
    });
}

template <typename S>
void ens_launch_add_sums(const S* src, int64_t n, unsigned weight, int first, u64* acc, bool aligned, hipStream_t st) {
    if (aligned)
        hipLaunchKernelGGL((ens_add_sums_kernel<S, 4>), dim3(uh_flat_grid((n + 3) / 4, ENS_GRID_CAP)), dim3(256), 0, st, src, n, weight,
                           first, acc);
    else
        hipLaunchKernelGGL((ens_add_sums_kernel<S, 1>), dim3(uh_flat_grid(n, ENS_GRID_CAP)), dim3(256), 0, st, src, n, weight, first,
                           acc);
}

// ------------------------------------------------------------------------------------------------------------ finish
// floor(255 m / s) for m <= s < 2^63, s > 0, without forming 255 m (which leaves 64 bits from m >= 2^56): eight steps of the
// restoring division give D = floor(256 m / s) and r = 256 m - D s for m < s, and 255 m = D s + (r - m) with -s < r - m < s.
__device__ __forceinline__ unsigned ens_scale255(u64 m, u64 s) {
    if (m >= s) return 255u;
    u64 r = m;
    unsigned D = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r <<= 1;
        const bool bit = r >= s;
        D = (D << 1) | (bit ? 1u : 0u);
        if (bit) r -= s;
    }
    return r >= m ? D : D - 1u;
}

__device__ __forceinline__ u64 ens_unit(const unsigned* __restrict__ den, int64_t pix, u64 unit) {
    return (den ? (u64)den[pix] : 1ull) * unit;                      // T = den views 2^24 total_weight < 2^59
}

// the three outputs of a pixel once its maximum, its index and the sum over the classes are known (NC > 1)
__device__ __forceinline__ uint8_t ens_confidence(u64 best, u64 sum) { return sum ? (uint8_t)ens_scale255(best, sum) : (uint8_t)0; }

// the one-class head: the class is 2 acc > T, the confidence that of the pair (a, T - a) with a = min(acc, T)
__device__ __forceinline__ void ens_finish_binary(u64 acc, u64 T, int64_t pix, uint8_t* __restrict__ classes,
                                                  uint8_t* __restrict__ confidence) {
    if (classes) classes[pix] = (uint8_t)(2ull * acc > T ? 1 : 0);
    if (confidence) {
        const u64 a = acc < T ? acc : T;
        const u64 m = a > T - a ? a : T - a;
        confidence[pix] = (uint8_t)ens_scale255(m, T);
    }
}

// NC <= 4: a pixel per thread, its sums in registers (16-byte loads where NC 8 bytes are whole 16-byte units and acc is aligned)
template <int NC, bool AL>
__global__ __launch_bounds__(256) void ens_finish_kernel(const u64* __restrict__ acc, const unsigned* __restrict__ den, u64 unit,
                                                          int64_t npix, uint8_t* __restrict__ classes, float* __restrict__ probs,
                                                          uint8_t* __restrict__ confidence) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += stride) {
        u64 a[NC];
        ens_load<u64, NC, (AL && NC % 2 == 0)>(acc + pix * NC, a);
        const u64 T = ens_unit(den, pix, unit);
        if (probs) {
            const double dT = (double)T;
#pragma unroll
            for (int c = 0; c < NC; ++c) probs[pix * NC + c] = (float)((double)a[c] / dT);
        }
        if (NC == 1) {
            ens_finish_binary(a[0], T, pix, classes, confidence);
        } else {
            u64 best = a[0], sum = a[0];
            unsigned idx = 0u;
#pragma unroll
            for (int c = 1; c < NC; ++c) {
                sum += a[c];
                if (a[c] > best) { best = a[c]; idx = c; }           // first maximum
            }
            if (classes) classes[pix] = (uint8_t)idx;
            if (confidence) confidence[pix] = ens_confidence(best, sum);
        }
    }
}

// any class count (> 4): class by class
__global__ __launch_bounds__(256) void ens_finish_generic_kernel(const u64* __restrict__ acc, const unsigned* __restrict__ den, u64 unit,
                                                                  int64_t npix, int NC, uint8_t* __restrict__ classes,
                                                                  float* __restrict__ probs, uint8_t* __restrict__ confidence) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x; pix < npix; pix += stride) {
        const u64* __restrict__ a = acc + pix * NC;
        const double dT = (double)ens_unit(den, pix, unit);
        u64 best = 0ull, sum = 0ull;
        unsigned idx = 0u;
        for (int c = 0; c < NC; ++c) {
            const u64 v = a[c];
            sum += v;
            if (c == 0 || v > best) { best = v; idx = c; }
            if (probs) probs[pix * NC + c] = (float)((double)v / dT);
        }
        if (classes) classes[pix] = (uint8_t)idx;
        if (confidence) confidence[pix] = ens_confidence(best, sum);
    }
}

bool ens_sizes_ok(int64_t npix, int NC) { return npix >= 1 && NC >= 1 && NC <= 256 && npix < (1ll << 40); }

}  // namespace

extern "C" int uh_ensemble_add(const void* src, int kind, int64_t npix, int NC, unsigned weight, int first, unsigned long long* acc,
                               uh_stream stream) {
    UH_REQUIRE(src && acc, "uh_ensemble_add: null pointer");
    UH_REQUIRE(kind == UH_F32 || kind == UH_BF16 || kind == UH_TILE_SUMS_I32 || kind == UH_ENS_SUMS_U64,
               "uh_ensemble_add: bad kind %d", kind);
    UH_REQUIRE(ens_sizes_ok(npix, NC), "uh_ensemble_add: bad sizes npix=%lld NC=%d (1 <= NC <= 256)", (long long)npix, NC);
    UH_REQUIRE(weight >= 1u && weight <= 1024u, "uh_ensemble_add: bad weight %u (1 .. 1024)", weight);
    const uintptr_t smask = kind == UH_BF16 ? 1 : kind == UH_ENS_SUMS_U64 ? 7 : 3;
    UH_REQUIRE((((uintptr_t)src) & smask) == 0 && (((uintptr_t)acc) & 7) == 0, "uh_ensemble_add: misaligned buffer");
    const bool aligned = uh_aligned16(src) && uh_aligned16(acc);
    u64* a = (u64*)acc;
    hipStream_t st = (hipStream_t)stream;
    switch (kind) {
        case UH_F32: ens_launch_add_logits<float>((const float*)src, npix, NC, weight, first, a, aligned, st); break;
        case UH_BF16: ens_launch_add_logits<bf16_t>((const bf16_t*)src, npix, NC, weight, first, a, aligned, st); break;
        case UH_TILE_SUMS_I32: ens_launch_add_sums<unsigned>((const unsigned*)src, npix * NC, weight, first, a, aligned, st); break;
        default: ens_launch_add_sums<u64>((const u64*)src, npix * NC, weight, first, a, aligned, st);
    }
    UH_CHECK_LAUNCH("ens_add_kernel");
    return UH_OK;
}

extern "C" int uh_ensemble_finish(const unsigned long long* acc, const unsigned int* den, int views, unsigned total_weight, int64_t npix,
                                  int NC, uint8_t* classes, float* probs, uint8_t* confidence, uh_stream stream) {
    UH_REQUIRE(acc, "uh_ensemble_finish: null pointer");
    UH_REQUIRE(classes || probs || confidence, "uh_ensemble_finish: null pointer (no output)");
    UH_REQUIRE(views == 1 || views == 2 || views == 4 || views == 8, "uh_ensemble_finish: bad views %d (1, 2, 4 or 8)", views);
    UH_REQUIRE(total_weight >= 1u && total_weight <= 1024u, "uh_ensemble_finish: bad total_weight %u (1 .. 1024)", total_weight);
    UH_REQUIRE(ens_sizes_ok(npix, NC), "uh_ensemble_finish: bad sizes npix=%lld NC=%d (1 <= NC <= 256)", (long long)npix, NC);
    UH_REQUIRE((((uintptr_t)acc) & 7) == 0 && (((uintptr_t)den | (uintptr_t)probs) & 3) == 0, "uh_ensemble_finish: misaligned buffer");
    const u64 unit = ((u64)views * total_weight) << 24;
    const u64* a = (const u64*)acc;
    const unsigned grid = uh_flat_grid(npix, ENS_GRID_CAP);
    hipStream_t st = (hipStream_t)stream;
    if (NC > 4) {
        hipLaunchKernelGGL(ens_finish_generic_kernel, dim3(grid), dim3(256), 0, st, a, den, unit, npix, NC, classes, probs, confidence);
    } else {
        const bool aligned = uh_aligned16(acc);
        uh_class_dispatch<4>(NC, [&](auto nc) {
            constexpr int C = decltype(nc)::value;
            if (aligned) hipLaunchKernelGGL((ens_finish_kernel<C, true>), dim3(grid), dim3(256), 0, st, a, den, unit, npix, classes, probs, confidence);
            else hipLaunchKernelGGL((ens_finish_kernel<C, false>), dim3(grid), dim3(256), 0, st, a, den, unit, npix, classes, probs, confidence);
        });
    }
    UH_CHECK_LAUNCH("ens_finish_kernel");
    return UH_OK;
}
