// What the loss passes share (loss.hip, focal_loss.hip, distill_loss.hip, surface_loss.hip).  The reduction scheme: per-thread ->
// wave shuffle -> LDS -> one partial row per block -> one finishing block that sums the rows' columns in double.  No atomics: a
// shape gives the same bits every time.  The head convention: ncls = 1 is the one-channel head, the two-class form on the logits
// (0, z), laid out [npix]; ncls = 2..MAXC a softmax head, laid out [npix][ncls].
#pragma once
#include "uh_common.h"
#include "uh_launch.h"

constexpr int LOSS_MAXBLK = 1024;
constexpr int LOSS_ROW = 32;     // floats per partial row

static inline int loss_nblk(int64_t n) {
    int64_t b = (n + 2047) / 2048;
    if (b > LOSS_MAXBLK) b = LOSS_MAXBLK;
    if (b < 1) b = 1;
    return (int)b;
}

// block-reduce K values held per thread; thread 0 writes them to row[]
template <int K>
__device__ __forceinline__ void block_reduce_store(float (&v)[K], float* row) {
    __shared__ float red[4][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = uh_wave_sum(v[k]);
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < K) row[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// one block of 256 threads: column sums of partials[nblk][LOSS_ROW] in double (tree reduction)
__device__ __forceinline__ double column_sum_256(const float* __restrict__ partials, int nblk, int k, double* red) {
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += (double)partials[(int64_t)b * LOSS_ROW + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    double r = red[0];
    __syncthreads();
    return r;
}

// floor(m / mask_div) as the reference's `true_masks //= 2` leaves it for the class indices a mask holds (train.py:119).  A 64-bit
// integer division is ~100 instructions on this chip and these kernels are instruction-bound (2 M elements, a few bytes each):
// values in [0, 2^31) -- every real mask -- take a shift (divisor 2) or a 32-bit division; anything else the full division,
// floored as `//` floors it: -1 // 2 is -1, a label outside every head, where the truncating -1 / 2 is class 0.
// R: the type a kernel wants the quotient in.  The conversion stands inside each branch, not behind the function: the 32-bit branch
// then converts a 32-bit integer (one v_cvt_f32_i32 for R = float), where a conversion of the merged 64-bit result costs a dozen
// instructions per label in kernels that are instruction-bound.
template <typename R>
__device__ __forceinline__ R uh_label_quot_as(int64_t m, int mask_div) {
    if ((uint64_t)m < (1ull << 31)) {
        const int v = (int)m;
        return (R)(mask_div == 2 ? (v >> 1) : (mask_div == 1 ? v : v / mask_div));
    }
    int64_t q = m / mask_div;
    if (m < 0 && q * mask_div != m) --q;
    return (R)q;
}

__device__ __forceinline__ int64_t uh_label_quot(int64_t m, int mask_div) { return uh_label_quot_as<int64_t>(m, mask_div); }
__device__ __forceinline__ float uh_mask_quot(int64_t m, int mask_div) { return uh_label_quot_as<float>(m, mask_div); }

// one pixel's logits as NC classes.  ONE: the one-channel head, logits [npix], the two-class form on (0, z)
template <int NC, bool ONE>
__device__ __forceinline__ void uh_head_load(const float* __restrict__ logits, int64_t p, float (&z)[NC]) {
    if constexpr (ONE) {
        z[0] = 0.f;
        z[1] = logits[p];
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) z[c] = logits[p * NC + c];
    }
}

// f(NC, ONE): (2, true) for the one-channel head, (ncls, false) otherwise
template <int MAXC, typename F>
static inline void uh_loss_head_dispatch(int ncls, F&& f) {
    uh_class_dispatch<MAXC>(ncls, [&](auto nc) {
        if constexpr (decltype(nc)::value == 1) f(std::integral_constant<int, 2>{}, std::true_type{});
        else f(nc, std::false_type{});
    });
}

static inline bool uh_loss_head_ok(const char* who, int ncls, int maxc) {
    if (ncls < 1 || ncls > maxc) { uh_set_error("%s: heads of 1 (sigmoid) to %d (softmax) classes, got %d", who, maxc, ncls); return false; }
    return true;
}

// loss.hip (internal): the column sums of partials[nblk][LOSS_ROW] in double -> sums[K], one workgroup (loss_finish_kernel): the
// second launch of every *_sums entry point, and what a data-parallel run all-reduces
int uh_loss_colsum_launch(const float* partials, int nblk, int K, float* sums, hipStream_t st);
