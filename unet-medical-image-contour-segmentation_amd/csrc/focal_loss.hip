// focal_loss.hip -- class-weighted focal + Tversky loss for imbalanced classes (DESIGN.md section 3 "Focal / Tversky loss").
// The reference has no such loss; the definitions are pinned in torch-float64 terms (tests/focal_tversky_ref.py).  For a head of
// C classes (softmax p of the NC logits of a pixel; the one-channel head is C = 2 with logits (0, z)), labels t, weights w_c,
// exponent gamma, prices alpha / beta, a class subset K and eps = 1e-6:
//   u        = sum_{c != t} p_c                       (1 - p_t without the cancellation)
//   focal    = sum_x w_t u^gamma (-log p_t) / sum_x w_t,   -log p_t = logsumexp(z) - z_t
//   TI_c     = (TP_c + eps) / ((1 - alpha - beta) TP_c + alpha P_c + beta T_c + eps),  TP = sum p_c [t = c], P = sum p_c, T = sum [t = c]
//   tversky  = 1 / |K| sum_{c in K} (1 - TI_c)
//   1. ft_sums_kernel    one pass over the logits: per-block rows { F, W, TP_c.., P_c.., T_c.. } (2 + 3 C floats <= one LOSS_ROW)
//      loss_finish_kernel  the rows' column sums in double -> sums (uh_loss_colsum_launch; what a data-parallel run all-reduces)
//   2. ft_finish_kernel  { total, focal, tversky } from the sums, in double
//   3. ft_grad_kernel    one pass: dL/dz_k = w_t / W s (tau_k - p_k) + p_k (g_k - sum_c p_c g_c); it WRITES dlogits
// The exponential of the largest logit is exactly 1, so logsumexp - max = log1p(sum of the others) and, where the label is the
// largest logit, u = rest / (1 + rest): both keep their relative accuracy when the pixel is easy (u -> 0).  u^gamma takes
// multiplications for gamma in {0, 1, 2} and exp2(gamma log2 u) otherwise, chosen per launch (a template parameter).
// No floating-point atomics; grid sizes depend on the shape alone: a call gives the same bits every time, and a pixel's gradient
// depends on that pixel's logits, its label, the sums and the scale factor only.
#include "uh_loss_reduce.h"

namespace {

constexpr int FT_MAXC = 8;

struct FtParams { float w[FT_MAXC]; float gamma; };      // by value: every index below is a compile-time constant after unrolling

enum { FT_POW0 = 0, FT_POW1 = 1, FT_POW2 = 2, FT_POWX = 3 };

template <int GM>
__device__ __forceinline__ float ft_pow(float u, float gamma) {
    if constexpr (GM == FT_POW0) return 1.f;                // also at u = 0
    else if constexpr (GM == FT_POW1) return u;
    else if constexpr (GM == FT_POW2) return u * u;
    else return exp2f(gamma * log2f(u));                    // gamma > 0: u = 0 -> exp2(-inf) = 0
}

template <int NC>
struct FtPixel { float p[NC]; float u, q, nlp, wt; };

// softmax of z, u = sum_{c != t} p_c, q = p_t, nlp = -log p_t = log1p(rest) - (z_t - max), wt = w_t.  A label outside the head
// matches no class: wt = 0 and every indicator is 0 (nothing is indexed with it).
template <int NC>
__device__ __forceinline__ void ft_pixel(const float (&z)[NC], int t, const FtParams& prm, FtPixel<NC>& o) {
    float m = z[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < NC; ++c)
        if (z[c] > m) { m = z[c]; am = c; }
    float x[NC];
    float rest = 0.f, su = 0.f, zt = m, wt = 0.f;
    // two classes: one exponential (the other is exp(0)); z[1 - am] - m is that difference exactly, so the bits are the general form's
    [[maybe_unused]] float e2 = 0.f;
    if constexpr (NC == 2) e2 = expf(-fabsf(z[1] - z[0]));
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if constexpr (NC == 2) x[c] = (c == am) ? 1.f : e2;
        else x[c] = expf(z[c] - m);                         // x[am] = 1
        rest += (c == am) ? 0.f : x[c];
        su += (c == t) ? 0.f : x[c];                        // (t == am: the same terms in the same order as rest)
        zt = (c == t) ? z[c] : zt;
        wt = (c == t) ? prm.w[c] : wt;
    }
    const float inv = 1.f / (1.f + rest);
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        o.p[c] = x[c] * inv;
        q = (c == t) ? o.p[c] : q;
    }
    o.u = su * inv;
    o.q = q;
    o.nlp = log1pf(rest) - (zt - m);
    o.wt = wt;
}

template <int NC, int GM, bool ONE>
__global__ __launch_bounds__(256) void ft_sums_kernel(const float* __restrict__ logits, const int64_t* __restrict__ mask, int mask_div,
                                                      FtParams prm, int64_t npix, float* __restrict__ partials) {
    float v[2 + 3 * NC];
#pragma unroll
    for (int k = 0; k < 2 + 3 * NC; ++k) v[k] = 0.f;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        float z[NC];
        uh_head_load<NC, ONE>(logits, p, z);
        const int t = (int)uh_mask_quot(mask[p], mask_div);
        FtPixel<NC> px;
        ft_pixel<NC>(z, t, prm, px);
        v[0] += px.wt * (ft_pow<GM>(px.u, prm.gamma) * px.nlp);
        v[1] += px.wt;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            v[2 + c] += (c == t) ? px.p[c] : 0.f;
            v[2 + NC + c] += px.p[c];
            v[2 + 2 * NC + c] += (c == t) ? 1.f : 0.f;
        }
    }
    block_reduce_store<2 + 3 * NC>(v, partials + (int64_t)blockIdx.x * LOSS_ROW);
}

// sel: bit c set when class c is in K; nsel = |K|
__global__ void ft_finish_kernel(const float* __restrict__ sums, int C, double alpha, double beta, unsigned sel, int nsel,
                                 float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    const double eps = 1e-6;
    const double F = (double)sums[0], W = (double)sums[1];
    const double focal = W > 0.0 ? F / W : 0.0;
    double tv = 0.0;
    for (int c = 0; c < C; ++c) {
        if (!((sel >> c) & 1u)) continue;
        const double TP = (double)sums[2 + c], P = (double)sums[2 + C + c], T = (double)sums[2 + 2 * C + c];
        tv += 1.0 - (TP + eps) / ((1.0 - alpha - beta) * TP + alpha * P + beta * T + eps);
    }
    tv /= (double)nsel;
    out[0] = (float)(focal + tv);
    out[1] = (float)focal;
    out[2] = (float)tv;
}

template <int NC, int GM, bool ONE>
__global__ __launch_bounds__(256) void ft_grad_kernel(const float* __restrict__ logits, const int64_t* __restrict__ mask, int mask_div,
                                                      FtParams prm, double alpha, double beta, unsigned sel, int nsel, int64_t npix,
                                                      const float* __restrict__ sums, const float* __restrict__ gscale,
                                                      float* __restrict__ dl) {
    // d tversky / d p_c = tau_c ? ga[c] : gb[c], and 1 / W: formed once per block, in double, by NC + 1 threads
    __shared__ float coef[2 * NC + 1];
    if (threadIdx.x < NC) {
        const int c = threadIdx.x;
        const double eps = 1e-6;
        const double TP = (double)sums[2 + c], P = (double)sums[2 + NC + c], T = (double)sums[2 + 2 * NC + c];
        const double N = TP + eps, D = (1.0 - alpha - beta) * TP + alpha * P + beta * T + eps;
        const double k = ((sel >> c) & 1u) ? 1.0 / (double)nsel : 0.0;
        coef[c] = (float)(-k * (D - N * (1.0 - beta)) / (D * D));
        coef[NC + c] = (float)(k * N * alpha / (D * D));
    } else if (threadIdx.x == NC) {
        const double W = (double)sums[1];
        coef[2 * NC] = (float)(W > 0.0 ? 1.0 / W : 0.0);
    }
    __syncthreads();
    float ga[NC], gb[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) { ga[c] = coef[c]; gb[c] = coef[NC + c]; }
    const float inv_w = coef[2 * NC];
    const float gs = gscale ? gscale[0] : 1.f;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (int64_t)gridDim.x * blockDim.x) {
        float z[NC];
        uh_head_load<NC, ONE>(logits, p, z);
        const int t = (int)uh_mask_quot(mask[p], mask_div);
        FtPixel<NC> px;
        ft_pixel<NC>(z, t, prm, px);
        // s = gamma u^gamma q r - u^gamma, r = log(q) / u -> -1 as u -> 0; q = 0 (u = 1): q r = 0 * (-nlp), nlp finite
        float s = -1.f;
        if constexpr (GM != FT_POW0) {
            const float r = px.u > 0.f ? -px.nlp / px.u : -1.f;
            s = ft_pow<GM>(px.u, prm.gamma) * (prm.gamma * px.q * r - 1.f);
        }
        const float fk = px.wt * inv_w * s;
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) dot += px.p[c] * ((c == t) ? ga[c] : gb[c]);
        float g[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float tmp = (c == t) ? px.u : -px.p[c];            // tau_c - p_c; 1 - p_t is u
            g[c] = gs * (fk * tmp + px.p[c] * (((c == t) ? ga[c] : gb[c]) - dot));
        }
        if constexpr (ONE) {
            dl[p] = g[1];
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) dl[p * NC + c] = g[c];
        }
    }
}

template <typename F>
inline void ft_pow_dispatch(float gamma, F&& f) {
    if (gamma == 0.f) f(std::integral_constant<int, FT_POW0>{});
    else if (gamma == 1.f) f(std::integral_constant<int, FT_POW1>{});
    else if (gamma == 2.f) f(std::integral_constant<int, FT_POW2>{});
    else f(std::integral_constant<int, FT_POWX>{});
}

inline int ft_classes_of(int ncls) { return ncls == 1 ? 2 : ncls; }

// head, weights (HOST, one per class; two for the one-channel head) and gamma
bool ft_focal_ok(const char* who, int ncls, const float* weights, float gamma, FtParams* prm) {
    if (!uh_loss_head_ok(who, ncls, FT_MAXC)) return false;
    if (!weights) { uh_set_error("%s: null class weights", who); return false; }
    const int C = ft_classes_of(ncls);
    for (int c = 0; c < FT_MAXC; ++c) prm->w[c] = 0.f;
    for (int c = 0; c < C; ++c) {
        if (!(weights[c] > 0.f) || !(weights[c] <= 3.0e38f)) { uh_set_error("%s: class weight %d must be finite and > 0, got %g", who, c, (double)weights[c]); return false; }
        prm->w[c] = weights[c];
    }
    if (!(gamma >= 0.f) || !(gamma <= 3.0e38f)) { uh_set_error("%s: gamma must be finite and >= 0, got %g", who, (double)gamma); return false; }
    prm->gamma = gamma;
    return true;
}

// alpha, beta and the class subset K (HOST ids, distinct, inside the head)
bool ft_tversky_ok(const char* who, int ncls, double alpha, double beta, const int* classes, int K, unsigned* sel) {
    if (!uh_loss_head_ok(who, ncls, FT_MAXC)) return false;
    if (!(alpha >= 0.0) || !(beta >= 0.0) || !(alpha + beta > 0.0) || !(alpha + beta <= 1.0e30)) {
        uh_set_error("%s: alpha and beta must be finite and >= 0 with alpha + beta > 0, got %g and %g", who, alpha, beta);
        return false;
    }
    const int C = ft_classes_of(ncls);
    if (!classes || K < 1 || K > C) { uh_set_error("%s: 1 to %d Tversky classes, got %d", who, C, K); return false; }
    *sel = 0;
    for (int k = 0; k < K; ++k) {
        if (classes[k] < 0 || classes[k] >= C) { uh_set_error("%s: class id %d is outside the head [0, %d)", who, classes[k], C); return false; }
        if ((*sel >> classes[k]) & 1u) { uh_set_error("%s: class id %d is selected twice", who, classes[k]); return false; }
        *sel |= 1u << classes[k];
    }
    return true;
}

}  // namespace

extern "C" int uh_focal_tversky_nsums(int ncls) { return (ncls < 1 || ncls > FT_MAXC) ? 0 : 2 + 3 * ft_classes_of(ncls); }

extern "C" int uh_focal_tversky_sums(const float* logits, const int64_t* mask, int mask_div, int64_t npix, int ncls, const float* weights,
                                     float gamma, float* sums, void* ws, size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(logits && mask && sums && ws && npix > 0, "uh_focal_tversky_sums: bad args");
    UH_REQUIRE(mask_div > 0, "uh_focal_tversky_sums: mask_div must be positive");
    FtParams prm;
    if (!ft_focal_ok("uh_focal_tversky_sums", ncls, weights, gamma, &prm)) return UH_EINVAL;
    UH_REQUIRE(ws_bytes >= uh_loss_ws_bytes(npix), "uh_focal_tversky_sums: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = loss_nblk(npix);
    ft_pow_dispatch(gamma, [&](auto gm) {
        uh_loss_head_dispatch<FT_MAXC>(ncls, [&](auto nc, auto one) {
            hipLaunchKernelGGL((ft_sums_kernel<decltype(nc)::value, decltype(gm)::value, decltype(one)::value>), dim3(nblk), dim3(256), 0,
                               st, logits, mask, mask_div, prm, npix, (float*)ws);
        });
    });
    UH_CHECK_LAUNCH("ft_sums_kernel");
    return uh_loss_colsum_launch((const float*)ws, nblk, uh_focal_tversky_nsums(ncls), sums, st);
}

extern "C" int uh_focal_tversky_finish(const float* sums, int ncls, double alpha, double beta, const int* classes, int K, float* out,
                                       uh_stream stream) {
    UH_REQUIRE(sums && out, "uh_focal_tversky_finish: null pointer");
    unsigned sel = 0;
    if (!ft_tversky_ok("uh_focal_tversky_finish", ncls, alpha, beta, classes, K, &sel)) return UH_EINVAL;
    hipLaunchKernelGGL(ft_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, ft_classes_of(ncls), alpha, beta, sel, K, out);
    UH_CHECK_LAUNCH("ft_finish_kernel");
    return UH_OK;
}

extern "C" int uh_focal_tversky_grad(const float* logits, const int64_t* mask, int mask_div, int64_t npix, int ncls, const float* weights,
                                     float gamma, double alpha, double beta, const int* classes, int K, const float* sums,
                                     const float* gscale, float* dlogits, uh_stream stream) {
    UH_REQUIRE(logits && mask && sums && dlogits && npix > 0, "uh_focal_tversky_grad: bad args");
    UH_REQUIRE(mask_div > 0, "uh_focal_tversky_grad: mask_div must be positive");
    FtParams prm;
    if (!ft_focal_ok("uh_focal_tversky_grad", ncls, weights, gamma, &prm)) return UH_EINVAL;
    unsigned sel = 0;
    if (!ft_tversky_ok("uh_focal_tversky_grad", ncls, alpha, beta, classes, K, &sel)) return UH_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = uh_flat_grid(npix, UH_GRID_CAP);
    ft_pow_dispatch(gamma, [&](auto gm) {
        uh_loss_head_dispatch<FT_MAXC>(ncls, [&](auto nc, auto one) {
            hipLaunchKernelGGL((ft_grad_kernel<decltype(nc)::value, decltype(gm)::value, decltype(one)::value>), dim3(grid), dim3(256), 0,
                               st, logits, mask, mask_div, prm, alpha, beta, sel, K, npix, sums, gscale, dlogits);
        });
    });
    UH_CHECK_LAUNCH("ft_grad_kernel");
    return UH_OK;
}
