// optim.hip -- torch.nn.utils.clip_grad_norm_ (train.py:157) and torch.optim.RMSprop with momentum
// (train.py:80-81,158) over ONE flat fp32 buffer holding every parameter: two HBM-bound passes
// (sum of squares, fused clip + update) instead of ~250 foreach launches.
#include "uh_common.h"

constexpr int OPT_MAXBLK = 2048;

extern "C" size_t uh_optim_ws_bytes(int64_t n) {
    (void)n;
    return (size_t)OPT_MAXBLK * sizeof(float) + 16;
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partials) {
    float acc = 0.f;
    const int64_t n4 = n >> 2;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 v = g4[i];
        acc += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        acc += g[i] * g[i];
    __shared__ float red[4];
    acc = uh_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void grad_norm_finish_kernel(const float* __restrict__ partials, int nblk, float* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) s += (double)partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)sqrt(red[0]);
}

extern "C" int uh_grad_sumsq(const float* g, int64_t n, float* norm_out, void* ws, size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(g && norm_out && ws && n > 0, "uh_grad_sumsq: bad args");
    UH_REQUIRE(ws_bytes >= uh_optim_ws_bytes(n), "uh_grad_sumsq: workspace too small");
    UH_REQUIRE(uh_aligned16(g), "uh_grad_sumsq: gradient buffer must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int64_t nb = (n / 4 + 255) / 256;
    if (nb > OPT_MAXBLK) nb = OPT_MAXBLK;
    if (nb < 1) nb = 1;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)nb), dim3(256), 0, st, g, n, (float*)ws);
    UH_CHECK_LAUNCH("grad_sumsq_kernel");
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, (int)nb, norm_out);
    UH_CHECK_LAUNCH("grad_norm_finish_kernel");
    return UH_OK;
}

// The per-element update, shared by rmsprop_kernel and rmsprop_ema_kernel: ONE statement sequence, so that the compiler
// contracts both kernels' arithmetic the same way and what they write to p / g / sq / buf is bit-identical.
__device__ __forceinline__ void rmsprop_update(float& p, float& g, float& s, float& b, float coef, float lr, float alpha,
                                               float eps, float wd, float mu) {
    float gc = g * coef;
    g = gc;                                      // clip_grad_norm_ scales .grad in place
    float ge = gc + wd * p;
    s = alpha * s + (1.f - alpha) * ge * ge;
    b = mu * b + ge / (sqrtf(s) + eps);
    p = p - lr * b;
}

// A NaN / infinite gradient norm means the loss was not finite (train.py:149-151 aborts before it gets here): the step
// kernels leave the parameters and the optimizer state untouched, so that a step replayed from a captured graph -- where
// the host can only look at the loss afterwards -- cannot poison them either.
__device__ __forceinline__ bool norm_not_finite(const float* total_norm) {
    return total_norm && !(fabsf(total_norm[0]) < __builtin_huge_valf());
}

__global__ __launch_bounds__(256) void rmsprop_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ sq,
                                                      float* __restrict__ buf, int64_t n, const float* __restrict__ total_norm,
                                                      float max_norm, float lr, float alpha, float eps, float wd, float mu) {
    float coef = 1.f;
    if (norm_not_finite(total_norm)) return;
    if (max_norm > 0.f && total_norm) coef = fminf(max_norm / (total_norm[0] + 1e-6f), 1.f);
    const int64_t n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    f32x4* g4 = reinterpret_cast<f32x4*>(g);
    f32x4* s4 = reinterpret_cast<f32x4*>(sq);
    f32x4* b4 = reinterpret_cast<f32x4*>(buf);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pv = p4[i], gv = g4[i], sv = s4[i], bv = b4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pe = pv[k], ge = gv[k], se = sv[k], be = bv[k];
            rmsprop_update(pe, ge, se, be, coef, lr, alpha, eps, wd, mu);
            pv[k] = pe; gv[k] = ge; sv[k] = se; bv[k] = be;
        }
        p4[i] = pv; g4[i] = gv; s4[i] = sv; b4[i] = bv;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pe = p[i], ge = g[i], se = sq[i], be = buf[i];
        rmsprop_update(pe, ge, se, be, coef, lr, alpha, eps, wd, mu);
        p[i] = pe; g[i] = ge; sq[i] = se; buf[i] = be;
    }
}

// The same pass with one more read-and-write stream: e <- e + c (p_new - e), the exponential moving average of the
// parameters, c = 1 - d_t.  t = updates[0] is read from device memory by every block (one scalar load): the whole step may
// be replayed from a captured graph, and a decay passed by value would freeze the warm-up d_t = min(decay, (1 + t) /
// (warmup + t)) inside the graph.
__global__ __launch_bounds__(256) void rmsprop_ema_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ sq,
                                                          float* __restrict__ buf, float* __restrict__ ema, int64_t n,
                                                          const float* __restrict__ total_norm, float max_norm, float lr,
                                                          float alpha, float eps, float wd, float mu, float decay, int warmup,
                                                          const int32_t* __restrict__ updates) {
    float coef = 1.f;
    if (norm_not_finite(total_norm)) return;
    if (max_norm > 0.f && total_norm) coef = fminf(max_norm / (total_norm[0] + 1e-6f), 1.f);
    float d = decay;
    if (warmup > 0) {
        const float t = (float)updates[0];
        d = fminf(decay, (1.f + t) / ((float)warmup + t));
    }
    const float c = 1.f - d;
    const int64_t n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    f32x4* g4 = reinterpret_cast<f32x4*>(g);
    f32x4* s4 = reinterpret_cast<f32x4*>(sq);
    f32x4* b4 = reinterpret_cast<f32x4*>(buf);
    f32x4* e4 = reinterpret_cast<f32x4*>(ema);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pv = p4[i], gv = g4[i], sv = s4[i], bv = b4[i], ev = e4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pe = pv[k], ge = gv[k], se = sv[k], be = bv[k];
            rmsprop_update(pe, ge, se, be, coef, lr, alpha, eps, wd, mu);
            pv[k] = pe; gv[k] = ge; sv[k] = se; bv[k] = be;
            ev[k] = ev[k] + c * (pe - ev[k]);
        }
        p4[i] = pv; g4[i] = gv; s4[i] = sv; b4[i] = bv; e4[i] = ev;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pe = p[i], ge = g[i], se = sq[i], be = buf[i], ee = ema[i];
        rmsprop_update(pe, ge, se, be, coef, lr, alpha, eps, wd, mu);
        p[i] = pe; g[i] = ge; sq[i] = se; buf[i] = be;
        ema[i] = ee + c * (pe - ee);
    }
}

static inline unsigned rmsprop_grid(int64_t n) {
    int64_t nb = (n / 4 + 255) / 256;
    if (nb > 256 * 16) nb = 256 * 16;
    if (nb < 1) nb = 1;
    return (unsigned)nb;
}

extern "C" int uh_rmsprop_step(float* p, float* g, float* square_avg, float* momentum_buf, int64_t n,
                               const float* total_norm, float max_norm, float lr, float alpha, float eps,
                               float weight_decay, float momentum, uh_stream stream) {
    UH_REQUIRE(p && g && square_avg && momentum_buf && n > 0, "uh_rmsprop_step: bad args");
    UH_REQUIRE(uh_aligned16(p) && uh_aligned16(g) && uh_aligned16(square_avg) && uh_aligned16(momentum_buf),
               "uh_rmsprop_step: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(rmsprop_kernel, dim3(rmsprop_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, square_avg, momentum_buf,
                       n, total_norm, max_norm, lr, alpha, eps, weight_decay, momentum);
    UH_CHECK_LAUNCH("rmsprop_kernel");
    return UH_OK;
}

extern "C" int uh_rmsprop_step_ema(float* p, float* g, float* square_avg, float* momentum_buf, float* ema, int64_t n,
                                   const float* total_norm, float max_norm, float lr, float alpha, float eps,
                                   float weight_decay, float momentum, float decay, int warmup, const int32_t* updates,
                                   uh_stream stream) {
    UH_REQUIRE(p && g && square_avg && momentum_buf && ema && updates && n > 0, "uh_rmsprop_step_ema: bad args");
    UH_REQUIRE(uh_aligned16(p) && uh_aligned16(g) && uh_aligned16(square_avg) && uh_aligned16(momentum_buf) && uh_aligned16(ema),
               "uh_rmsprop_step_ema: buffers must be 16-byte aligned");
    UH_REQUIRE(decay > 0.f && decay < 1.f && warmup >= 0, "uh_rmsprop_step_ema: decay must lie in (0, 1), warmup >= 0");
    hipLaunchKernelGGL(rmsprop_ema_kernel, dim3(rmsprop_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, square_avg,
                       momentum_buf, ema, n, total_norm, max_norm, lr, alpha, eps, weight_decay, momentum, decay, warmup, updates);
    UH_CHECK_LAUNCH("rmsprop_ema_kernel");
    return UH_OK;
}

// Launched once per optimizer step behind its uh_rmsprop_step_ema launches (a step whose stale slices split the update into
// several runs sees one t throughout); a skipped step (non-finite norm) does not count.
__global__ void ema_tick_kernel(int32_t* updates, const float* total_norm) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || norm_not_finite(total_norm)) return;
    updates[0] = updates[0] + 1;
}

extern "C" int uh_ema_tick(int32_t* updates, const float* total_norm, uh_stream stream) {
    UH_REQUIRE(updates, "uh_ema_tick: bad args");
    hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, updates, total_norm);
    UH_CHECK_LAUNCH("ema_tick_kernel");
    return UH_OK;
}

// Exchange two fp32 buffers in place (the averaged weights go under the model and come out again without a third buffer).
__global__ __launch_bounds__(256) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
    const int64_t n4 = n >> 2;
    f32x4* a4 = reinterpret_cast<f32x4*>(a);
    f32x4* b4 = reinterpret_cast<f32x4*>(b);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 av = a4[i], bv = b4[i];
        a4[i] = bv; b4[i] = av;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float av = a[i], bv = b[i];
        a[i] = bv; b[i] = av;
    }
}

extern "C" int uh_swap_f32(float* a, float* b, int64_t n, uh_stream stream) {
    UH_REQUIRE(a && b && n > 0, "uh_swap_f32: bad args");
    UH_REQUIRE(uh_aligned16(a) && uh_aligned16(b), "uh_swap_f32: buffers must be 16-byte aligned");
    UH_REQUIRE(a + n <= b || b + n <= a, "uh_swap_f32: the buffers overlap");
    hipLaunchKernelGGL(swap_f32_kernel, dim3(rmsprop_grid(n)), dim3(256), 0, (hipStream_t)stream, a, b, n);
    UH_CHECK_LAUNCH("swap_f32_kernel");
    return UH_OK;
}

// ---------------------------------------------------------------------------------------------- AdamW and SGD
// The two other rules of the fused pass (train.OptimConfig): the conventions of the RMSprop kernels above -- one grid-stride pass,
// 16-byte loads and stores with a scalar tail, the clip coefficient read from the device norm, g overwritten with the clipped
// gradient, nothing written under a non-finite norm -- and, per rule, ONE per-element function shared by the plain and the
// averaging instantiation (template <bool EMA>), so that both write the same bits to p, g and the state.
__device__ __forceinline__ float clip_coef(const float* total_norm, float max_norm) {
    return (max_norm > 0.f && total_norm) ? fminf(max_norm / (total_norm[0] + 1e-6f), 1.f) : 1.f;
}

// c = 1 - d_t of the moving average, as rmsprop_ema_kernel forms it.
__device__ __forceinline__ float ema_coef(float decay, int warmup, const int32_t* updates) {
    float d = decay;
    if (warmup > 0) {
        const float t = (float)updates[0];
        d = fminf(decay, (1.f + t) / ((float)warmup + t));
    }
    return 1.f - d;
}

// b^t for an integer t >= 1 by squaring, in double (at most 31 squarings and as many products: about 1e-15 relative, nothing
// beside the one float32 rounding that follows).  Every thread forms it once, before its loop.
__device__ __forceinline__ double pow_int(double b, int t) {
    double r = 1.0;
    while (t > 0) {
        if (t & 1) r *= b;
        b *= b;
        t >>= 1;
    }
    return r;
}

// torch.optim.AdamW(amsgrad=False, maximize=False).  step = lr / bc1 and rbc2 = 1 / sqrt(bc2) arrive as float32 scalars, each
// formed in double and rounded once (adamw_kernel); lrwd = lr * wd: the decoupled decay is p - lrwd * p, which keeps a decay of
// 1e-7 that the float32 1 - lr * wd would round to a multiple of 6e-8.
__device__ __forceinline__ void adamw_update(float& p, float& g, float& m, float& v, float coef, float beta1, float beta2,
                                             float eps, float lrwd, float step, float rbc2) {
    float gc = g * coef;
    g = gc;                                      // clip_grad_norm_ scales .grad in place
    m = beta1 * m + (1.f - beta1) * gc;
    v = beta2 * v + (1.f - beta2) * gc * gc;
    float den = sqrtf(v) * rbc2 + eps;
    float pd = p - lrwd * p;                     // the decay takes the OLD parameter
    p = pd - step * (m / den);
}

// torch.optim.SGD(dampening=0); mu = 0 is plain SGD, a zero buffer gives torch's first step (b' = ge).
__device__ __forceinline__ void sgd_update(float& p, float& g, float& b, float coef, float lr, float wd, float mu, bool nesterov) {
    float gc = g * coef;
    g = gc;
    float ge = gc + wd * p;
    b = mu * b + ge;
    float d = nesterov ? ge + mu * b : b;
    p = p - lr * d;
}

// steps[0] is the number of updates applied so far, on the device like `updates`: the whole step may be replayed from a captured
// graph, and a step number passed by value would freeze the bias corrections inside it.  uh_ema_tick advances it.
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m_,
                                                    float* __restrict__ v_, float* __restrict__ ema, int64_t n,
                                                    const float* __restrict__ total_norm, float max_norm, float lr, float beta1,
                                                    float beta2, float eps, float wd, const int32_t* __restrict__ steps,
                                                    float decay, int warmup, const int32_t* __restrict__ updates) {
    if (norm_not_finite(total_norm)) return;
    const float coef = clip_coef(total_norm, max_norm);
    const int t = steps[0] + 1;
    const double bc1 = 1.0 - pow_int((double)beta1, t), bc2 = 1.0 - pow_int((double)beta2, t);
    const float step = (float)((double)lr / bc1), rbc2 = (float)(1.0 / sqrt(bc2));
    const float lrwd = lr * wd;
    float c = 0.f;
    if (EMA) c = ema_coef(decay, warmup, updates);
    const int64_t n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    f32x4* g4 = reinterpret_cast<f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m_);
    f32x4* v4 = reinterpret_cast<f32x4*>(v_);
    f32x4* e4 = reinterpret_cast<f32x4*>(ema);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pv = p4[i], gv = g4[i], mv = m4[i], vv = v4[i], ev;
        if (EMA) ev = e4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pe = pv[k], ge = gv[k], me = mv[k], ve = vv[k];
            adamw_update(pe, ge, me, ve, coef, beta1, beta2, eps, lrwd, step, rbc2);
            pv[k] = pe; gv[k] = ge; mv[k] = me; vv[k] = ve;
            if (EMA) ev[k] = ev[k] + c * (pe - ev[k]);
        }
        p4[i] = pv; g4[i] = gv; m4[i] = mv; v4[i] = vv;
        if (EMA) e4[i] = ev;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pe = p[i], ge = g[i], me = m_[i], ve = v_[i];
        adamw_update(pe, ge, me, ve, coef, beta1, beta2, eps, lrwd, step, rbc2);
        p[i] = pe; g[i] = ge; m_[i] = me; v_[i] = ve;
        if (EMA) {
            float ee = ema[i];
            ema[i] = ee + c * (pe - ee);
        }
    }
}

template <bool EMA>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf,
                                                  float* __restrict__ ema, int64_t n, const float* __restrict__ total_norm,
                                                  float max_norm, float lr, float wd, float mu, int nesterov, float decay,
                                                  int warmup, const int32_t* __restrict__ updates) {
    if (norm_not_finite(total_norm)) return;
    const float coef = clip_coef(total_norm, max_norm);
    const bool nes = nesterov != 0;
    float c = 0.f;
    if (EMA) c = ema_coef(decay, warmup, updates);
    const int64_t n4 = n >> 2;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    f32x4* g4 = reinterpret_cast<f32x4*>(g);
    f32x4* b4 = reinterpret_cast<f32x4*>(buf);
    f32x4* e4 = reinterpret_cast<f32x4*>(ema);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f32x4 pv = p4[i], gv = g4[i], bv = b4[i], ev;
        if (EMA) ev = e4[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pe = pv[k], ge = gv[k], be = bv[k];
            sgd_update(pe, ge, be, coef, lr, wd, mu, nes);
            pv[k] = pe; gv[k] = ge; bv[k] = be;
            if (EMA) ev[k] = ev[k] + c * (pe - ev[k]);
        }
        p4[i] = pv; g4[i] = gv; b4[i] = bv;
        if (EMA) e4[i] = ev;
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pe = p[i], ge = g[i], be = buf[i];
        sgd_update(pe, ge, be, coef, lr, wd, mu, nes);
        p[i] = pe; g[i] = ge; buf[i] = be;
        if (EMA) {
            float ee = ema[i];
            ema[i] = ee + c * (pe - ee);
        }
    }
}

static inline bool adamw_hyper_ok(float lr, float beta1, float beta2, float eps, float wd) {
    return lr >= 0.f && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && wd >= 0.f;
}

static inline bool sgd_hyper_ok(float lr, float wd, float mu, int nesterov) {
    return lr >= 0.f && wd >= 0.f && mu >= 0.f && (nesterov == 0 || (nesterov == 1 && mu > 0.f));
}

extern "C" int uh_adamw_step(float* p, float* g, float* exp_avg, float* exp_avg_sq, int64_t n, const float* total_norm,
                             float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                             const int32_t* steps, uh_stream stream) {
    UH_REQUIRE(p && g && exp_avg && exp_avg_sq && steps && n > 0, "uh_adamw_step: bad args");
    UH_REQUIRE(uh_aligned16(p) && uh_aligned16(g) && uh_aligned16(exp_avg) && uh_aligned16(exp_avg_sq),
               "uh_adamw_step: buffers must be 16-byte aligned");
    UH_REQUIRE(adamw_hyper_ok(lr, beta1, beta2, eps, weight_decay),
               "uh_adamw_step: lr, eps, weight_decay must be >= 0 and the betas lie in [0, 1)");
    hipLaunchKernelGGL(adamw_kernel<false>, dim3(rmsprop_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, exp_avg, exp_avg_sq,
                       (float*)nullptr, n, total_norm, max_norm, lr, beta1, beta2, eps, weight_decay, steps, 0.f, 0,
                       (const int32_t*)nullptr);
    UH_CHECK_LAUNCH("adamw_kernel");
    return UH_OK;
}

extern "C" int uh_adamw_step_ema(float* p, float* g, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                 const float* total_norm, float max_norm, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, const int32_t* steps, float decay, int warmup, const int32_t* updates,
                                 uh_stream stream) {
    UH_REQUIRE(p && g && exp_avg && exp_avg_sq && ema && steps && updates && n > 0, "uh_adamw_step_ema: bad args");
    UH_REQUIRE(uh_aligned16(p) && uh_aligned16(g) && uh_aligned16(exp_avg) && uh_aligned16(exp_avg_sq) && uh_aligned16(ema),
               "uh_adamw_step_ema: buffers must be 16-byte aligned");
    UH_REQUIRE(adamw_hyper_ok(lr, beta1, beta2, eps, weight_decay),
               "uh_adamw_step_ema: lr, eps, weight_decay must be >= 0 and the betas lie in [0, 1)");
    UH_REQUIRE(decay > 0.f && decay < 1.f && warmup >= 0, "uh_adamw_step_ema: decay must lie in (0, 1), warmup >= 0");
    hipLaunchKernelGGL(adamw_kernel<true>, dim3(rmsprop_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, exp_avg, exp_avg_sq,
                       ema, n, total_norm, max_norm, lr, beta1, beta2, eps, weight_decay, steps, decay, warmup, updates);
    UH_CHECK_LAUNCH("adamw_ema_kernel");
    return UH_OK;
}

extern "C" int uh_sgd_step(float* p, float* g, float* momentum_buf, int64_t n, const float* total_norm, float max_norm, float lr,
                           float weight_decay, float momentum, int nesterov, uh_stream stream) {
    UH_REQUIRE(p && g && momentum_buf && n > 0, "uh_sgd_step: bad args");
    UH_REQUIRE(uh_aligned16(p) && uh_aligned16(g) && uh_aligned16(momentum_buf), "uh_sgd_step: buffers must be 16-byte aligned");
    UH_REQUIRE(sgd_hyper_ok(lr, weight_decay, momentum, nesterov),
               "uh_sgd_step: lr, weight_decay, momentum must be >= 0, nesterov 0 or 1 and only with momentum > 0");
    hipLaunchKernelGGL(sgd_kernel<false>, dim3(rmsprop_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, momentum_buf,
                       (float*)nullptr, n, total_norm, max_norm, lr, weight_decay, momentum, nesterov, 0.f, 0,
                       (const int32_t*)nullptr);
    UH_CHECK_LAUNCH("sgd_kernel");
    return UH_OK;
}

extern "C" int uh_sgd_step_ema(float* p, float* g, float* momentum_buf, float* ema, int64_t n, const float* total_norm,
                               float max_norm, float lr, float weight_decay, float momentum, int nesterov, float decay, int warmup,
                               const int32_t* updates, uh_stream stream) {
    UH_REQUIRE(p && g && momentum_buf && ema && updates && n > 0, "uh_sgd_step_ema: bad args");
    UH_REQUIRE(uh_aligned16(p) && uh_aligned16(g) && uh_aligned16(momentum_buf) && uh_aligned16(ema),
               "uh_sgd_step_ema: buffers must be 16-byte aligned");
    UH_REQUIRE(sgd_hyper_ok(lr, weight_decay, momentum, nesterov),
               "uh_sgd_step_ema: lr, weight_decay, momentum must be >= 0, nesterov 0 or 1 and only with momentum > 0");
    UH_REQUIRE(decay > 0.f && decay < 1.f && warmup >= 0, "uh_sgd_step_ema: decay must lie in (0, 1), warmup >= 0");
    hipLaunchKernelGGL(sgd_kernel<true>, dim3(rmsprop_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, momentum_buf, ema, n,
                       total_norm, max_norm, lr, weight_decay, momentum, nesterov, decay, warmup, updates);
    UH_CHECK_LAUNCH("sgd_ema_kernel");
    return UH_OK;
}
