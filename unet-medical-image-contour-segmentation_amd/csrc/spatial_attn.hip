// spatial_attn.hip -- SpatialAttention (unet_parts.py:39-60) and the skip gate of Up(use_attention=True)
// (unet_parts.py:91-92) for NHWC tensors:
//
//   pool[p] = (mean_c x[p,c], max_c x[p,c])                     fp32 [B,H,W,2], plus the FIRST maximal channel [B,H,W] int32
//   a[p]    = sigmoid(sum_{ch,r,s} w[ch][r][s] * pool[p + (r-P, s-P), ch])    (k x k, zero padding P = k/2)   fp32 [B,H,W]
//   y[p,c]  = x[p,c] * a[p]                                     (optional, rounded once to the tensor dtype)
//
// backward:  g_a = sum_c dy*x (or given), g_s = g_a*a*(1-a), g_pool = transposed correlation of g_s,
//            dx = dy*a + g_avg/C + [c == argmax]*g_max, dw[ch][r][s] = sum_p g_s[p] * pool[p + (r-P, s-P), ch].
//
// The channel reductions walk a pixel's channels with a group of G lanes (G a power of two <= 64, one 16-byte vector per
// lane and step) that meets by wave shuffles; the k x k correlations run on LDS tiles of the 2-channel maps; the per-channel
// passes (gate, dx) are flat 16-byte vector loops.  The filter gradient is reduced per workgroup and finished in a fixed
// order (no float atomics: two runs are bit-identical).  HBM-bound: DESIGN.md section 3 "Spatial attention".
#include "uh_launch.h"

#define SA_BLOCK 256
#define SA_DW_BLOCKS 1024          // upper bound of the filter-gradient partial rows (uh_spatial_attn_dw_nblk)
#define SA_TH 8                    // LDS tile of the k x k correlations: SA_TH x SA_TW output pixels, one per thread
#define SA_TW 32

static inline int sa_group(int C, int V) {
    int nv = (C + V - 1) / V, g = 1;
    while (g < nv && g < 64) g <<= 1;
    return g;
}

// The launch form of the channel reductions (sa_pool_kernel, sa_gs_kernel) and of the flat passes (gate, dx): V channels per
// lane and step (one 16-byte vector where every tensor of the call allows it, else 1), G lanes per pixel, and the steps a lane
// takes to cover C.  The launches and uh_spatial_attn_plan both ask here.
struct SaPlan { int V, G, steps; };

static inline SaPlan sa_plan(int C, int vec, bool vec_ok) {
    const int V = vec_ok && C % vec == 0 ? vec : 1;
    const int G = sa_group(C, V);
    const int nv = (C + V - 1) / V;
    return SaPlan{V, G, (nv + G - 1) / G};
}

static inline unsigned sa_grid(int64_t npix, int G) {
    return (unsigned)((npix * G + SA_BLOCK - 1) / SA_BLOCK);
}

static_assert(SA_BLOCK == 256, "uh_flat_grid counts workgroups of 256 threads");
static inline unsigned sa_flat_grid(int64_t total) { return uh_flat_grid(total, UH_GRID_CAP_1X1); }

// (m, i) beats (mo, io) as the channel maximum: larger, or NaN against a number, or equal with a lower channel index
__device__ __forceinline__ bool sa_better(float m, int i, float mo, int io) {
    if (i < 0) return false;
    if (io < 0) return true;
    const bool n = m != m, no = mo != mo;
    if (n != no) return n;
    if (!n && m != mo) return m > mo;
    return i < io;
}

__device__ __forceinline__ float sa_group_sum(float v, int G) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ------------------------------------------------------------------------------------ channel mean / max / argmax
template <typename T, int V>
__global__ __launch_bounds__(SA_BLOCK) void sa_pool_kernel(const T* __restrict__ x, int ldx, float* __restrict__ pool,
                                                           int* __restrict__ amax, int64_t npix, int C, int G) {
    const int64_t gid = (int64_t)blockIdx.x * SA_BLOCK + threadIdx.x;
    const int64_t p = gid / G;
    const int lane = (int)(gid & (G - 1));
    const bool live = p < npix;
    float s = 0.f, m = 0.f;
    int mi = -1;
    if (live) {
        const T* px = x + p * ldx;
        for (int c0 = lane * V; c0 < C; c0 += G * V) {
            float v[V];
            uh_load<T, V>(px + c0, v);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                s += v[i];
                if (sa_better(v[i], c0 + i, m, mi)) { m = v[i]; mi = c0 + i; }
            }
        }
    }
    for (int o = G >> 1; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        const float mo = __shfl_xor(m, o, 64);
        const int io = __shfl_xor(mi, o, 64);
        if (sa_better(mo, io, m, mi)) { m = mo; mi = io; }
    }
    if (live && lane == 0) {
        pool[2 * p] = s / (float)C;
        pool[2 * p + 1] = m;
        amax[p] = mi;
    }
}

// ------------------------------------------------------------------------------------ k x k correlations on LDS tiles
// One workgroup per SA_TH x SA_TW output tile of one image; the (SA_TH + k - 1) x (SA_TW + k - 1) input halo is staged in LDS
// (zero outside the image: the conv's zero padding), one output pixel per thread.

// a[p] = sigmoid(sum_{ch,r,s} w[ch][r][s] * pool[p + (r-P, s-P)][ch])
template <int K>
__global__ __launch_bounds__(SA_BLOCK) void sa_map_tile_kernel(const float* __restrict__ pool, const float* __restrict__ w,
                                                               float* __restrict__ a, int H, int W) {
    constexpr int P = K / 2, KK = K * K, HH = SA_TH + K - 1, WW = SA_TW + K - 1;
    __shared__ float2 tile[HH][WW];
    const int h0 = blockIdx.y * SA_TH, w0 = blockIdx.x * SA_TW;
    const int64_t img = (int64_t)blockIdx.z * H * W;
    for (int i = threadIdx.x; i < HH * WW; i += SA_BLOCK) {
        const int hh = h0 + i / WW - P, ww = w0 + i % WW - P;
        float2 v = make_float2(0.f, 0.f);
        if (hh >= 0 && hh < H && ww >= 0 && ww < W) v = *reinterpret_cast<const float2*>(pool + 2 * (img + (int64_t)hh * W + ww));
        tile[i / WW][i % WW] = v;
    }
    __syncthreads();
    const int ty = threadIdx.x / SA_TW, tx = threadIdx.x % SA_TW;
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const float2 v = tile[ty + r][tx + q];
            acc += w[r * K + q] * v.x + w[KK + r * K + q] * v.y;
        }
    const int h = h0 + ty, x = w0 + tx;
    if (h < H && x < W) a[img + (int64_t)h * W + x] = uh_sigmoid(acc);
}

// d pool[p][ch] = sum_{r,s} w[ch][r][s] * g_s[p - (r-P, s-P)]   (the transposed correlation), fp32 [npix][2]
template <int K>
__global__ __launch_bounds__(SA_BLOCK) void sa_gpool_tile_kernel(const float* __restrict__ gs, const float* __restrict__ w,
                                                                 float* __restrict__ gpool, int H, int W) {
    constexpr int P = K / 2, KK = K * K, HH = SA_TH + K - 1, WW = SA_TW + K - 1;
    __shared__ float tile[HH][WW];
    const int h0 = blockIdx.y * SA_TH, w0 = blockIdx.x * SA_TW;
    const int64_t img = (int64_t)blockIdx.z * H * W;
    for (int i = threadIdx.x; i < HH * WW; i += SA_BLOCK) {
        const int hh = h0 + i / WW - P, ww = w0 + i % WW - P;
        tile[i / WW][i % WW] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? gs[img + (int64_t)hh * W + ww] : 0.f;
    }
    __syncthreads();
    const int ty = threadIdx.x / SA_TW, tx = threadIdx.x % SA_TW;
    float gavg = 0.f, gmax = 0.f;
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) {
            const float g = tile[ty + 2 * P - r][tx + 2 * P - q];
            gavg += w[r * K + q] * g;
            gmax += w[KK + r * K + q] * g;
        }
    const int h = h0 + ty, x = w0 + tx;
    if (h < H && x < W) *reinterpret_cast<float2*>(gpool + 2 * (img + (int64_t)h * W + x)) = make_float2(gavg, gmax);
}

// ------------------------------------------------------------------------------------ gate: y = x * a
template <typename T, int V>
__global__ __launch_bounds__(SA_BLOCK) void sa_gate_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ a,
                                                           T* __restrict__ y, int ldy, int64_t npix, int C) {
    const int nv = C / V;
    const int64_t total = npix * nv;
    for (int64_t i = (int64_t)blockIdx.x * SA_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SA_BLOCK) {
        const int64_t p = i / nv;
        const int c0 = (int)(i - p * nv) * V;
        const float av = a[p];
        float v[V];
        uh_load<T, V>(x + p * ldx + c0, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] *= av;
        uh_store<T, V>(y + p * ldy + c0, v);
    }
}

// ------------------------------------------------------------------------------------ backward: g_s
template <typename T, int V>
__global__ __launch_bounds__(SA_BLOCK) void sa_gs_kernel(const T* __restrict__ dy, int lddy, const T* __restrict__ x, int ldx,
                                                         const float* __restrict__ ga, const float* __restrict__ a,
                                                         float* __restrict__ gs, int64_t npix, int C, int G) {
    const int64_t gid = (int64_t)blockIdx.x * SA_BLOCK + threadIdx.x;
    const int64_t p = gid / G;
    const int lane = (int)(gid & (G - 1));
    const bool live = p < npix;
    float d = 0.f;
    if (live) {
        if (ga) {
            d = lane == 0 ? ga[p] : 0.f;
        } else {
            const T* px = x + p * ldx;
            const T* pd = dy + p * lddy;
            for (int c0 = lane * V; c0 < C; c0 += G * V) {
                float v[V], g[V];
                uh_load<T, V>(px + c0, v);
                uh_load<T, V>(pd + c0, g);
#pragma unroll
                for (int i = 0; i < V; ++i) d += v[i] * g[i];
            }
        }
    }
    d = sa_group_sum(d, G);
    if (live && lane == 0) {
        const float av = a[p];
        gs[p] = d * av * (1.f - av);
    }
}

// ------------------------------------------------------------------------------------ backward: dx
// dx = dy*a + g_avg/C + [c == argmax]*g_max   (dy == NULL: the standalone map, no product term)
template <typename T, int V>
__global__ __launch_bounds__(SA_BLOCK) void sa_dx_kernel(const float* __restrict__ gpool, const float* __restrict__ a,
                                                         const int* __restrict__ amax, const T* __restrict__ dy, int lddy,
                                                         T* __restrict__ dx, int lddx, int64_t npix, int C) {
    const int nv = C / V;
    const int64_t total = npix * nv;
    for (int64_t i = (int64_t)blockIdx.x * SA_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * SA_BLOCK) {
        const int64_t p = i / nv;
        const int c0 = (int)(i - p * nv) * V;
        const float2 g = *reinterpret_cast<const float2*>(gpool + 2 * p);
        const float gavg = g.x / (float)C;
        const int am = amax[p];
        float o[V];
        if (dy) {
            const float av = a[p];
            uh_load<T, V>(dy + p * lddy + c0, o);
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = o[j] * av + gavg;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = gavg;
        }
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (c0 + j == am) o[j] += g.y;
        uh_store<T, V>(dx + p * lddx + c0, o);
    }
}

// ------------------------------------------------------------------------------------ backward: dw
// Tiles of SA_TH x SA_TW pixels are dealt to the nblk workgroups in a fixed order; thread j owns tap j % 128 (< 2k^2) over
// half j / 128 of each tile's rows; the halves meet in LDS: one row of partials per workgroup, then one finishing pass.
static inline int sa_dw_nblk(int B, int H, int W) {
    const int64_t n = (int64_t)B * ((H + SA_TH - 1) / SA_TH) * ((W + SA_TW - 1) / SA_TW);
    return (int)(n > SA_DW_BLOCKS ? SA_DW_BLOCKS : n);
}

template <int K>
__global__ __launch_bounds__(SA_BLOCK) void sa_dw_partials_kernel(const float* __restrict__ gs, const float* __restrict__ pool,
                                                                  float* __restrict__ part, int B, int H, int W) {
    constexpr int P = K / 2, KK = K * K, HH = SA_TH + K - 1, WW = SA_TW + K - 1;
    static_assert(2 * KK <= 128 && SA_BLOCK == 256 && SA_TH % 2 == 0 && SA_TH * SA_TW == SA_BLOCK, "tap / half split");
    __shared__ float2 tile[HH][WW];
    __shared__ float gt[SA_TH][SA_TW];
    __shared__ float red[SA_BLOCK];
    const int tx_tiles = (W + SA_TW - 1) / SA_TW, ty_tiles = (H + SA_TH - 1) / SA_TH;
    const int64_t per_img = (int64_t)ty_tiles * tx_tiles;
    const int64_t ntiles = (int64_t)B * per_img;
    const int t = threadIdx.x % 128, half = threadIdx.x / 128;
    const int ch = t / KK, r = (t % KK) / K, q = t % K;
    float acc = 0.f;
    for (int64_t ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
        const int b = (int)(ti / per_img);
        const int rem = (int)(ti % per_img);
        const int h0 = (rem / tx_tiles) * SA_TH, w0 = (rem % tx_tiles) * SA_TW;
        const int64_t img = (int64_t)b * H * W;
        __syncthreads();                       // the previous tile's reads are done
        for (int i = threadIdx.x; i < HH * WW; i += SA_BLOCK) {
            const int hh = h0 + i / WW - P, ww = w0 + i % WW - P;
            float2 v = make_float2(0.f, 0.f);
            if (hh >= 0 && hh < H && ww >= 0 && ww < W) v = *reinterpret_cast<const float2*>(pool + 2 * (img + (int64_t)hh * W + ww));
            tile[i / WW][i % WW] = v;
        }
        {
            const int ty = threadIdx.x / SA_TW, tx = threadIdx.x % SA_TW;
            const int h = h0 + ty, x = w0 + tx;
            gt[ty][tx] = (h < H && x < W) ? gs[img + (int64_t)h * W + x] : 0.f;
        }
        __syncthreads();
        if (t < 2 * KK) {
            for (int yy = half * (SA_TH / 2); yy < (half + 1) * (SA_TH / 2); ++yy)
#pragma unroll 8
                for (int xx = 0; xx < SA_TW; ++xx) {
                    const float2 v = tile[yy + r][xx + q];
                    acc += gt[yy][xx] * (ch == 0 ? v.x : v.y);
                }
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < 2 * KK) part[(int64_t)blockIdx.x * 2 * KK + threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + 128];
}

// dw[t] = sum of the nblk partial rows: one workgroup per tap, strided sums then a fixed tree (same order every run)
__global__ __launch_bounds__(SA_BLOCK) void sa_dw_finish_kernel(const float* __restrict__ part, int nblk, int n,
                                                                float* __restrict__ dw) {
    __shared__ float red[SA_BLOCK / UH_WAVE];
    const int t = blockIdx.x;
    float s = 0.f;
    for (int b = threadIdx.x; b < nblk; b += SA_BLOCK) s += part[(int64_t)b * n + t];
    s = uh_wave_sum(s);
    if (threadIdx.x % UH_WAVE == 0) red[threadIdx.x / UH_WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot = 0.f;
        for (int i = 0; i < SA_BLOCK / UH_WAVE; ++i) tot += red[i];
        dw[t] = tot;
    }
}

// ------------------------------------------------------------------------------------ C ABI
template <int K>
static void sa_launch_fwd(const void* x, int ldx, float* pool, int* amax, const float* w, float* a, void* y, int ldy,
                          int B, int H, int W, int C, int dt, hipStream_t st) {
    const int64_t npix = (int64_t)B * H * W;
    const dim3 tiles((W + SA_TW - 1) / SA_TW, (H + SA_TH - 1) / SA_TH, B);
    UH_DISPATCH_DT(dt, T, {
        const SaPlan p = sa_plan(C, VEC, uh_vec_ok<T>(x, ldx, C) && (!y || uh_vec_ok<T>(y, ldy, C)));
        const int G = p.G;
        if (p.V == VEC) {
            hipLaunchKernelGGL((sa_pool_kernel<T, VEC>), dim3(sa_grid(npix, G)), dim3(SA_BLOCK), 0, st, (const T*)x, ldx, pool,
                               amax, npix, C, G);
            hipLaunchKernelGGL((sa_map_tile_kernel<K>), tiles, dim3(SA_BLOCK), 0, st, pool, w, a, H, W);
            if (y)
                hipLaunchKernelGGL((sa_gate_kernel<T, VEC>), dim3(sa_flat_grid(npix * (C / VEC))), dim3(SA_BLOCK), 0, st,
                                   (const T*)x, ldx, a, (T*)y, ldy, npix, C);
        } else {
            hipLaunchKernelGGL((sa_pool_kernel<T, 1>), dim3(sa_grid(npix, G)), dim3(SA_BLOCK), 0, st, (const T*)x, ldx, pool,
                               amax, npix, C, G);
            hipLaunchKernelGGL((sa_map_tile_kernel<K>), tiles, dim3(SA_BLOCK), 0, st, pool, w, a, H, W);
            if (y)
                hipLaunchKernelGGL((sa_gate_kernel<T, 1>), dim3(sa_flat_grid(npix * C)), dim3(SA_BLOCK), 0, st, (const T*)x, ldx,
                                   a, (T*)y, ldy, npix, C);
        }
    });
}

template <int K>
static void sa_launch_bwd(const void* dy, int lddy, const float* ga, const void* x, int ldx, const float* pool,
                          const int* amax, const float* w, const float* a, float* ws, void* dx, int lddx, float* dw,
                          float* part, int B, int H, int W, int C, int dt, hipStream_t st) {
    const int64_t npix = (int64_t)B * H * W;
    float* gpool = ws;                  // [npix][2]
    float* gs = ws + 2 * npix;          // [npix]
    const dim3 tiles((W + SA_TW - 1) / SA_TW, (H + SA_TH - 1) / SA_TH, B);
    UH_DISPATCH_DT(dt, T, {
        const SaPlan p = sa_plan(C, VEC, uh_vec_ok<T>(dx, lddx, C) && (!dy || (uh_vec_ok<T>(dy, lddy, C) && uh_vec_ok<T>(x, ldx, C))));
        const bool vec = p.V == VEC;
        const int G = ga ? 1 : p.G;         // the map's gradient is given per pixel: nothing to reduce
        if (vec)
            hipLaunchKernelGGL((sa_gs_kernel<T, VEC>), dim3(sa_grid(npix, G)), dim3(SA_BLOCK), 0, st, (const T*)dy, lddy,
                               (const T*)x, ldx, ga, a, gs, npix, C, G);
        else
            hipLaunchKernelGGL((sa_gs_kernel<T, 1>), dim3(sa_grid(npix, G)), dim3(SA_BLOCK), 0, st, (const T*)dy, lddy,
                               (const T*)x, ldx, ga, a, gs, npix, C, G);
        hipLaunchKernelGGL((sa_gpool_tile_kernel<K>), tiles, dim3(SA_BLOCK), 0, st, gs, w, gpool, H, W);
        if (vec)
            hipLaunchKernelGGL((sa_dx_kernel<T, VEC>), dim3(sa_flat_grid(npix * (C / VEC))), dim3(SA_BLOCK), 0, st, gpool, a,
                               amax, (const T*)dy, lddy, (T*)dx, lddx, npix, C);
        else
            hipLaunchKernelGGL((sa_dx_kernel<T, 1>), dim3(sa_flat_grid(npix * C)), dim3(SA_BLOCK), 0, st, gpool, a, amax,
                               (const T*)dy, lddy, (T*)dx, lddx, npix, C);
    });
    const int nblk = sa_dw_nblk(B, H, W);
    hipLaunchKernelGGL((sa_dw_partials_kernel<K>), dim3(nblk), dim3(SA_BLOCK), 0, st, gs, pool, part, B, H, W);
    hipLaunchKernelGGL(sa_dw_finish_kernel, dim3(2 * K * K), dim3(SA_BLOCK), 0, st, part, nblk, 2 * K * K, dw);
}

static bool sa_shape_ok(int B, int H, int W, int C, int k) {
    return B > 0 && H > 0 && W > 0 && C > 0 && (k == 3 || k == 7) && B <= 65535 && (H + SA_TH - 1) / SA_TH <= 65535 && (int64_t)B * H * W * 64 < ((int64_t)1 << 62);
}

extern "C" int uh_spatial_attn_dw_nblk(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return sa_dw_nblk(B, H, W);
}

extern "C" int uh_spatial_attn_plan(int C, int dt, int aligned, int64_t* out) {
    UH_REQUIRE(C > 0 && out && (dt == UH_F32 || dt == UH_BF16), "uh_spatial_attn_plan: bad args");
    const SaPlan p = sa_plan(C, dt == UH_BF16 ? 8 : 4, aligned != 0);
    out[0] = p.V;
    out[1] = p.G;
    out[2] = p.steps;
    return UH_OK;
}

extern "C" int uh_spatial_attn_fwd(const void* x, int ldx, const float* w, int k, float* pool, int* amax, float* a, void* y,
                                   int ldy, int B, int H, int W, int C, int dt, uh_stream stream) {
    UH_REQUIRE(x && w && pool && amax && a, "uh_spatial_attn_fwd: NULL pointer");
    UH_REQUIRE(sa_shape_ok(B, H, W, C, k), "uh_spatial_attn_fwd: bad shape B=%d H=%d W=%d C=%d k=%d (k is 3 or 7)", B, H, W, C, k);
    UH_REQUIRE(ldx >= C && (!y || ldy >= C), "uh_spatial_attn_fwd: pixel stride below the channel count");
    UH_REQUIRE(dt == UH_F32 || dt == UH_BF16, "uh_spatial_attn_fwd: dt must be UH_F32 or UH_BF16");
    UH_REQUIRE((((uintptr_t)pool) & 7) == 0, "uh_spatial_attn_fwd: pool must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (k == 7) sa_launch_fwd<7>(x, ldx, pool, amax, w, a, y, ldy, B, H, W, C, dt, st);
    else sa_launch_fwd<3>(x, ldx, pool, amax, w, a, y, ldy, B, H, W, C, dt, st);
    UH_CHECK_LAUNCH("spatial_attn_fwd");
    return UH_OK;
}

extern "C" int uh_spatial_attn_bwd(const void* dy, int lddy, const float* ga, const void* x, int ldx, const float* w, int k,
                                   const float* pool, const int* amax, const float* a, float* ws, void* dx, int lddx,
                                   float* dw, float* dw_partials, int nblk, int B, int H, int W, int C, int dt,
                                   uh_stream stream) {
    UH_REQUIRE((dy != NULL) != (ga != NULL), "uh_spatial_attn_bwd: exactly one of dy (gate) and ga (map) is given");
    UH_REQUIRE(!dy || x, "uh_spatial_attn_bwd: the gate backward needs x");
    UH_REQUIRE(w && pool && amax && a && ws && dx && dw && dw_partials, "uh_spatial_attn_bwd: NULL pointer");
    UH_REQUIRE(sa_shape_ok(B, H, W, C, k), "uh_spatial_attn_bwd: bad shape B=%d H=%d W=%d C=%d k=%d (k is 3 or 7)", B, H, W, C, k);
    UH_REQUIRE(lddx >= C && (!dy || (lddy >= C && ldx >= C)), "uh_spatial_attn_bwd: pixel stride below the channel count");
    UH_REQUIRE(dt == UH_F32 || dt == UH_BF16, "uh_spatial_attn_bwd: dt must be UH_F32 or UH_BF16");
    UH_REQUIRE(nblk >= uh_spatial_attn_dw_nblk(B, H, W), "uh_spatial_attn_bwd: dw_partials holds %d rows, %d needed", nblk,
               uh_spatial_attn_dw_nblk(B, H, W));
    UH_REQUIRE((((uintptr_t)pool) & 7) == 0 && (((uintptr_t)ws) & 7) == 0, "uh_spatial_attn_bwd: pool / ws must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (k == 7) sa_launch_bwd<7>(dy, lddy, ga, x, ldx, pool, amax, w, a, ws, dx, lddx, dw, dw_partials, B, H, W, C, dt, st);
    else sa_launch_bwd<3>(dy, lddy, ga, x, ldx, pool, amax, w, a, ws, dx, lddx, dw, dw_partials, B, H, W, C, dt, st);
    UH_CHECK_LAUNCH("spatial_attn_bwd");
    return UH_OK;
}
