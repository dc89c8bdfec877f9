// distill_loss.hip -- knowledge distillation: the KL term between a teacher's and the student's temperature-softened class
// probabilities (Hinton et al.; DESIGN.md section 3 "Distillation").  The reference has no such term; the definition is pinned in
// torch-float64 terms (tests/distill_ref.py).  Student logits z, teacher logits v, a head of C classes (the one-channel head is
// C = 2 on (0, z) and (0, v)), temperature T > 0, weight w > 0, n pixels of the global batch:
//   q = softmax(v / T),  p = softmax(z / T)
//   kd    = T^2 / n sum_x sum_c q_c (log q_c - log p_c)
//   agree = 1 / n sum_x [argmax z = argmax v]                 (first maximum; a diagnostic, no gradient)
//   1. kd_sums_kernel    one pass over both logit tensors: per-block rows { sum KL, sum agree }
//      loss_finish_kernel  the rows' column sums in double -> sums[2] (uh_loss_colsum_launch; what a data-parallel run all-reduces)
//   2. kd_finish_kernel  { w kd, kd, agree } from the sums and n, in double
//   3. kd_grad_kernel    one pass: d(w kd)/dz_k = w T / n (p_k - q_k); it WRITES dlogits (the largest class's component is
//                        minus the sum of the others: no cancellation where both sides are sure of a class)
// Per pixel the KL is formed from shifted, scaled logits, never from logs of probabilities: with a_c = (v_c - max v) / T and
// b_c = (z_c - max z) / T the exponential of the largest is exactly 1, log sum exp = log1p(sum of the others), and
//   KL = sum_c q_c (a_c - b_c) - (log1p(rest_v) - log1p(rest_z)).
// Both tensors go through the same function (kd_side), so z == v gives a == b and equal log1p terms bit for bit: kd is exactly 0
// and p - q is +0.0 in every element.  q_c = 0 (underflow) multiplies a finite difference: an exact 0, no 0 * inf.
// No floating-point atomics; grid sizes depend on the shape alone: a call gives the same bits every time, and a pixel's gradient
// depends on that pixel's two logit vectors, n, T, w and the scale factor only.
#include <math.h>
#include "uh_loss_reduce.h"

namespace {

constexpr int KD_MAXC = 8;

// KD_NO_FMA.  The exact zero of z == v rests on both sides' a_c and p_c being the same ROUNDED products.  Left to itself the
// compiler contracts p_c - q_c = x_c inv - x'_c inv' into fma(x_c, inv, -(x'_c inv')), which is the rounding error of the first
// product, not 0 (and likewise a_c - b_c when 1 / T is no power of two).  Contraction is off in kd_side and around its uses.

template <int NC>
struct KdSide { float a[NC]; float p[NC]; float l1p; int am; };

// a_c = (z_c - max z) * inv_t, p = softmax(z * inv_t), l1p = log(sum_c exp(a_c)) = log1p(sum of the non-maximal ones), am = the
// first maximum.  Run on the teacher's and on the student's logits alike.
template <int NC>
__device__ __forceinline__ void kd_side(const float (&z)[NC], float inv_t, KdSide<NC>& o) {
#pragma clang fp contract(off)          // every product below is rounded on its own (see KD_NO_FMA)
    float m = z[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < NC; ++c)
        if (z[c] > m) { m = z[c]; am = c; }
    float x[NC];
    float rest = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) o.a[c] = (z[c] - m) * inv_t;          // a[am] = +0.0
    if constexpr (NC == 2) {
        // two classes: one exponential (the other is exp(0)), of the shift that is not the maximum's
        const float e2 = expf(am == 0 ? o.a[1] : o.a[0]);
        x[0] = am == 0 ? 1.f : e2;
        x[1] = am == 1 ? 1.f : e2;
        rest = e2;
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            x[c] = expf(o.a[c]);                                        // x[am] = 1
            rest += (c == am) ? 0.f : x[c];
        }
    }
    const float inv = 1.f / (1.f + rest);
#pragma unroll
    for (int c = 0; c < NC; ++c) o.p[c] = x[c] * inv;
    o.l1p = log1pf(rest);
    o.am = am;
}

template <int NC, bool ONE>
__global__ __launch_bounds__(256) void kd_sums_kernel(const float* __restrict__ student, const float* __restrict__ teacher, float inv_t,
                                                      int64_t npix, float* __restrict__ partials) {
    float acc[2] = {0.f, 0.f};
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)          // KD_NO_FMA
        float z[NC], v[NC];
        uh_head_load<NC, ONE>(student, p, z);
        uh_head_load<NC, ONE>(teacher, p, v);
        KdSide<NC> s, t;
        kd_side<NC>(z, inv_t, s);
        kd_side<NC>(v, inv_t, t);
        float kl = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) kl += t.p[c] * (t.a[c] - s.a[c]);
        kl -= t.l1p - s.l1p;
        acc[0] += kl;
        acc[1] += (s.am == t.am) ? 1.f : 0.f;
    }
    block_reduce_store<2>(acc, partials + (int64_t)blockIdx.x * LOSS_ROW);
}

__global__ void kd_finish_kernel(const float* __restrict__ sums, double n_mean, double T, double w, float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const double kd = T * T / n_mean * (double)sums[0];
    out[0] = (float)(w * kd);
    out[1] = (float)kd;
    out[2] = (float)((double)sums[1] / n_mean);
}

// coef = w T / n_mean, rounded once on the host
template <int NC, bool ONE>
__global__ __launch_bounds__(256) void kd_grad_kernel(const float* __restrict__ student, const float* __restrict__ teacher, float inv_t,
                                                      float coef, int64_t npix, const float* __restrict__ gscale,
                                                      float* __restrict__ dl) {
    const float k = (gscale ? gscale[0] : 1.f) * coef;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
#pragma clang fp contract(off)          // KD_NO_FMA
        float z[NC], v[NC];
        uh_head_load<NC, ONE>(student, p, z);
        uh_head_load<NC, ONE>(teacher, p, v);
        KdSide<NC> s, t;
        kd_side<NC>(z, inv_t, s);
        kd_side<NC>(v, inv_t, t);
        // sum_c (p_c - q_c) = 0: the component of the student's largest class is minus the sum of the others.  Where both sides are
        // sure of one class, p and q of that class are 1 - (something small) and their difference would keep no digit of it;
        // the other classes' differences are formed from the small numbers themselves.  (0 - (+0) = +0: z == v stays +0.0.)
        float d[NC];
        float others = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            d[c] = s.p[c] - t.p[c];
            others += (c == s.am) ? 0.f : d[c];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) d[c] = (c == s.am) ? 0.f - others : d[c];
        if constexpr (ONE) {
            dl[p] = k * d[1];
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) dl[p * NC + c] = k * d[c];
        }
    }
}

inline bool kd_positive(double v) { return v > 0.0 && v <= 1.0e30; }      // finite and > 0 (a NaN fails both)

}  // namespace

extern "C" int uh_distill_nsums(void) { return 2; }

extern "C" int uh_distill_sums(const float* student, const float* teacher, int64_t npix, int ncls, double T, float* sums, void* ws,
                               size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(student && teacher && sums && ws && npix > 0, "uh_distill_sums: bad args");
    if (!uh_loss_head_ok("uh_distill_sums", ncls, KD_MAXC)) return UH_EINVAL;
    UH_REQUIRE(kd_positive(T), "uh_distill_sums: the temperature must be finite and > 0, got %g", T);
    UH_REQUIRE(ws_bytes >= uh_loss_ws_bytes(npix), "uh_distill_sums: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = loss_nblk(npix);
    const float inv_t = (float)(1.0 / T);
    uh_loss_head_dispatch<KD_MAXC>(ncls, [&](auto nc, auto one) {
        hipLaunchKernelGGL((kd_sums_kernel<decltype(nc)::value, decltype(one)::value>), dim3(nblk), dim3(256), 0, st, student, teacher,
                           inv_t, npix, (float*)ws);
    });
    UH_CHECK_LAUNCH("kd_sums_kernel");
    return uh_loss_colsum_launch((const float*)ws, nblk, uh_distill_nsums(), sums, st);
}

extern "C" int uh_distill_finish(const float* sums, double n_mean, double T, double w, float* out, uh_stream stream) {
    UH_REQUIRE(sums && out, "uh_distill_finish: null pointer");
    UH_REQUIRE(kd_positive(n_mean) && kd_positive(T) && kd_positive(w),
               "uh_distill_finish: n_mean, the temperature and the weight must be finite and > 0, got %g, %g, %g", n_mean, T, w);
    hipLaunchKernelGGL(kd_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, n_mean, T, w, out);
    UH_CHECK_LAUNCH("kd_finish_kernel");
    return UH_OK;
}

extern "C" int uh_distill_grad(const float* student, const float* teacher, int64_t npix, int ncls, double n_mean, double T, double w,
                               const float* gscale, float* dlogits, uh_stream stream) {
    UH_REQUIRE(student && teacher && dlogits && npix > 0, "uh_distill_grad: bad args");
    if (!uh_loss_head_ok("uh_distill_grad", ncls, KD_MAXC)) return UH_EINVAL;
    UH_REQUIRE(kd_positive(n_mean) && kd_positive(T) && kd_positive(w),
               "uh_distill_grad: n_mean, the temperature and the weight must be finite and > 0, got %g, %g, %g", n_mean, T, w);
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = uh_flat_grid(npix, UH_GRID_CAP);
    const float inv_t = (float)(1.0 / T), coef = (float)(w * T / n_mean);
    uh_loss_head_dispatch<KD_MAXC>(ncls, [&](auto nc, auto one) {
        hipLaunchKernelGGL((kd_grad_kernel<decltype(nc)::value, decltype(one)::value>), dim3(grid), dim3(256), 0, st, student, teacher,
                           inv_t, coef, npix, gscale, dlogits);
    });
    UH_CHECK_LAUNCH("kd_grad_kernel");
    return UH_OK;
}
