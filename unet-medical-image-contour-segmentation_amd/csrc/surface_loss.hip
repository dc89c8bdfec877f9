// surface_loss.hip -- the distance-weighted surface loss of Kervadec et al. on the device, its maps rebuilt from the step's own
// (augmented) labels (DESIGN.md section 3 "Surface loss").  The reference has no such loss; the definitions are pinned in
// scipy / torch-float64 terms (tests/surface_loss_ref.py).  Per image b and selected class c of H x W int64 labels:
//   T_c           (label / mask_div == c): mask_div = 1 for a multi-class head, 2 for the binary head (the target BCE uses)
//   S(T), D_T[x]  border and exact squared distance of the contour metrics (contour_metrics.hip: uh_edt_sq_u8, reused as it is)
//   phi_c[b,y,x]  s * (float)sqrt((double)D_T[x]), s = -1 inside T_c, +1 outside; a border pixel (D = 0, inside) is -0.0f;
//                 T_c empty in image b: phi_c[b] = +0.0f everywhere, and the image has no gradient for that class
//   surface       1 / (n_mean K) * sum_b sum_x sum_{c in C} p_c(x) phi_c(x), p = sigmoid (binary) or softmax (multi-class)
//   binary        dL/dz   = g w / n_mean * phi * sigma (1 - sigma), sigma = sigmoid(z)
//   multi-class   dL/dz_k = g w / (n_mean K) * p_k * (phi_k [k in C] - sum_{c in C} p_c phi_c)
//   1. sl_border_kernel   border masks of all K classes straight from the int64 labels (no uint8 copy of them)
//   2. uh_edt_sq_u8       D over the K * B border images, kept in the workspace between the value and the gradient
//   3. sl_map_kernel      phi as fp32 [K][B][H][W] (uh_surface_dist_map, the public helper), or
//      sl_sums_kernel     the value: phi formed in registers from D and the labels, products and sums in fp64, one partial per
//                         workgroup, then sl_finish_kernel (one workgroup, a fixed tree), or
//      sl_grad_kernel     the gradient, one thread per pixel, the softmax of ncls <= 8 held in registers; it WRITES dlogits
// A pixel's NC logits (and its NC gradients) move as 16-byte vectors (uh_vec.h) where NC is a multiple of 4 and the tensor is
// 16-byte aligned; other heads (NC = 3: 12-byte rows) move them as NC dwords, which a wave still spends on whole cache lines.
// No floating-point atomics; grid sizes depend on the shape alone: a call gives the same bits every time, and a pixel's
// gradient depends on that pixel's logits, its own image's labels and the scale factor only.
#include "uh_loss_reduce.h"     // LOSS_MAXBLK, loss_nblk, uh_label_quot, uh_loss_head_ok
#include "uh_vec.h"

namespace {

constexpr int SL_MAXC = 8;                     // classes of the head, and selected classes per call
constexpr int SL_MAX_DIM = 32768;              // uh_edt_sq_u8's limits (squared distances are kept in 31 bits)
constexpr unsigned SL_NO_FEATURE = 0xFFFFFFFFu;

struct SlClasses { int k; int id[SL_MAXC]; };  // by value: every index below is a compile-time constant after unrolling

__device__ __forceinline__ float sl_phi(unsigned d2, bool inside) {
    if (d2 == SL_NO_FEATURE) return 0.0f;                          // T_c is empty in this image
    const float r = (float)sqrt((double)d2);
    return inside ? -r : r;
}

__device__ __forceinline__ float sl_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

__device__ __forceinline__ bool sl_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// one pixel's NC values; vec (wave-uniform): the row is 16-byte aligned and NC a multiple of 4
template <int NC>
__device__ __forceinline__ void sl_load_row(const float* __restrict__ row, float (&p)[NC], bool vec) {
    if constexpr (NC % 4 == 0) {
        if (vec) {
#pragma unroll
            for (int c = 0; c < NC; c += 4) {
                float v[4];
                uh_load<float, 4>(row + c, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) p[c + j] = v[j];
            }
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] = row[c];
}

template <int NC>
__device__ __forceinline__ void sl_store_row(float* __restrict__ row, const float (&g)[NC], bool vec) {
    if constexpr (NC % 4 == 0) {
        if (vec) {
#pragma unroll
            for (int c = 0; c < NC; c += 4) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = g[c + j];
                uh_store<float, 4>(row + c, v);
            }
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) row[c] = g[c];
}

template <int NC>
__device__ __forceinline__ void sl_softmax(const float* __restrict__ row, float (&p)[NC], bool vec) {
    sl_load_row<NC>(row, p, vec);
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < NC; ++c) m = fmaxf(m, p[c]);
    float den = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) { p[c] = expf(p[c] - m); den += p[c]; }
    const float inv = 1.f / den;
#pragma unroll
    for (int c = 0; c < NC; ++c) p[c] *= inv;
}

// blockIdx.y = image; out[k][b][y][x] = 1 on the border of T_k.  Neighbours outside the image are never read.
__global__ __launch_bounds__(256) void sl_border_kernel(const int64_t* __restrict__ mask, int div, SlClasses cls,
                                                        unsigned char* __restrict__ out, int B, int H, int W) {
    const long long hw = (long long)H * W;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const int b = blockIdx.y;
    const int64_t* img = mask + (long long)b * hw;
    const int x = (int)(p % W), y = (int)(p / W);
    const long long q = uh_label_quot(img[p], div);
    const bool frame = x == 0 || y == 0 || x == W - 1 || y == H - 1;
    long long ql = q, qr = q, qu = q, qd = q;
    if (!frame) {
        ql = uh_label_quot(img[p - 1], div); qr = uh_label_quot(img[p + 1], div);
        qu = uh_label_quot(img[p - W], div); qd = uh_label_quot(img[p + W], div);
    }
#pragma unroll
    for (int k = 0; k < SL_MAXC; ++k)
        if (k < cls.k) {
            const long long c = cls.id[k];
            const bool bd = q == c && (frame || ql != c || qr != c || qu != c || qd != c);
            out[((long long)k * B + b) * hw + p] = bd;
        }
}

__device__ __forceinline__ int sl_class_of(const SlClasses& cls, int k) {
    int c = cls.id[0];
#pragma unroll
    for (int j = 1; j < SL_MAXC; ++j) c = j == k ? cls.id[j] : c;
    return c;
}

// blockIdx.y = k; n = B * H * W pixels of one class's maps
__global__ __launch_bounds__(256) void sl_map_kernel(const unsigned* __restrict__ d2, const int64_t* __restrict__ mask, int div,
                                                     SlClasses cls, float* __restrict__ phi, long long n) {
    const int k = blockIdx.y;
    const long long c = sl_class_of(cls, k);
    const long long base = (long long)k * n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        phi[base + i] = sl_phi(d2[base + i], uh_label_quot(mask[i], div) == c);
}

// sum over the selected classes of p_c phi_c at pixel i, phi formed here; NC = 1: the sigmoid head (one map)
template <int NC>
__device__ __forceinline__ double sl_pixel_term(const float* __restrict__ logits, const unsigned* __restrict__ d2, long long q,
                                                const SlClasses& cls, long long i, long long n, bool vec) {
    if constexpr (NC == 1) {
        return (double)sl_sigmoid(logits[i]) * (double)sl_phi(d2[i], q == cls.id[0]);
    } else {
        float p[NC];
        sl_softmax<NC>(logits + i * NC, p, vec);
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < SL_MAXC; ++k)
            if (k < cls.k) {
                const int c = cls.id[k];
                float pc = 0.f;
#pragma unroll
                for (int j = 0; j < NC; ++j) pc = j == c ? p[j] : pc;
                t = __dadd_rn(t, __dmul_rn((double)pc, (double)sl_phi(d2[(long long)k * n + i], q == c)));
            }
        return t;
    }
}

// thread: its pixels in grid-stride order; wave: xor butterfly; workgroup: the four waves in order -> partials[blockIdx.x]
template <int NC>
__global__ __launch_bounds__(256) void sl_sums_kernel(const float* __restrict__ logits, const int64_t* __restrict__ mask, int div,
                                                      SlClasses cls, const unsigned* __restrict__ d2, long long n,
                                                      double* __restrict__ partials) {
    __shared__ double red[4];
    double acc = 0.0;
    const bool vec = sl_aligned16(logits);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        acc = __dadd_rn(acc, sl_pixel_term<NC>(logits, d2, uh_label_quot(mask[i], div), cls, i, n, vec));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = __dadd_rn(acc, __shfl_xor(acc, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = __dadd_rn(__dadd_rn(red[0], red[1]), __dadd_rn(red[2], red[3]));
}

// out = { surface, w * surface }, surface = sum * inv
__global__ __launch_bounds__(256) void sl_finish_kernel(const double* __restrict__ partials, int nblk, double inv, float w,
                                                        float* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s = __dadd_rn(s, partials[b]);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] = __dadd_rn(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float v = (float)__dmul_rn(red[0], inv);
        out[0] = v;
        out[1] = w * v;
    }
}

template <int NC>
__global__ __launch_bounds__(256) void sl_grad_kernel(const float* __restrict__ logits, const int64_t* __restrict__ mask, int div,
                                                      SlClasses cls, const unsigned* __restrict__ d2, long long n, float scale,
                                                      const float* __restrict__ gscale, float* __restrict__ dl) {
    const float gs = (gscale ? gscale[0] : 1.f) * scale;
    const bool vec = sl_aligned16(logits) && sl_aligned16(dl);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long q = uh_label_quot(mask[i], div);
        if constexpr (NC == 1) {
            const float sg = sl_sigmoid(logits[i]);
            dl[i] = gs * (sl_phi(d2[i], q == cls.id[0]) * (sg * (1.f - sg)));
        } else {
            float p[NC], ph[NC];
            sl_softmax<NC>(logits + i * NC, p, vec);
#pragma unroll
            for (int j = 0; j < NC; ++j) ph[j] = 0.f;
#pragma unroll
            for (int k = 0; k < SL_MAXC; ++k)
                if (k < cls.k) {
                    const int c = cls.id[k];
                    const float f = sl_phi(d2[(long long)k * n + i], q == c);
#pragma unroll
                    for (int j = 0; j < NC; ++j) ph[j] = j == c ? f : ph[j];
                }
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < NC; ++j) dot += p[j] * ph[j];      // ph is 0 outside C
#pragma unroll
            for (int j = 0; j < NC; ++j) p[j] = gs * (p[j] * (ph[j] - dot));
            sl_store_row<NC>(dl + i * NC, p, vec);
        }
    }
}

size_t sl_align16(size_t v) { return (v + 15) & ~(size_t)15; }

bool sl_shape_ok(const char* who, int B, int H, int W, int K) {
    if (B <= 0 || H <= 0 || W <= 0) { uh_set_error("%s: B, H and W must be positive (got %d, %d, %d)", who, B, H, W); return false; }
    if (K < 1 || K > SL_MAXC) { uh_set_error("%s: 1 to %d selected classes per call, got %d", who, SL_MAXC, K); return false; }
    if (H > SL_MAX_DIM || W > SL_MAX_DIM) { uh_set_error("%s: H and W are limited to %d (squared distances are kept in 31 bits)", who, SL_MAX_DIM); return false; }
    if ((long long)H * W >= (1ll << 31) || (long long)K * B * H * W >= (1ll << 40)) { uh_set_error("%s: pixel count out of range", who); return false; }
    if ((long long)K * B > 65535) { uh_set_error("%s: at most 65535 distance maps (K * B) per call", who); return false; }
    return true;
}

// ids >= 0 and distinct; below ncls for a softmax head (ncls >= 2).  The sigmoid head (ncls = 1) has one map, and its id is a
// value of the target mask / mask_div, not a channel; ncls = 0: no head
bool sl_classes_ok(const char* who, const int* classes, int K, int ncls, SlClasses* out) {
    if (ncls == 1 && K != 1) { uh_set_error("%s: the sigmoid head has one map, got %d classes", who, K); return false; }
    if (ncls == 1) ncls = 0;
    out->k = K;
    for (int k = 0; k < SL_MAXC; ++k) out->id[k] = k < K ? classes[k] : -1;
    for (int k = 0; k < K; ++k) {
        if (classes[k] < 0 || (ncls > 0 && classes[k] >= ncls)) {
            uh_set_error("%s: class id %d is outside [0, %d)", who, classes[k], ncls > 0 ? ncls : 0x7fffffff);
            return false;
        }
        for (int j = 0; j < k; ++j)
            if (classes[j] == classes[k]) { uh_set_error("%s: class id %d is selected twice", who, classes[k]); return false; }
    }
    return true;
}

// workspace: [D K*B*H*W u32][border K*B*H*W u8][EDT workspace][partials LOSS_MAXBLK f64]
struct SlWs { unsigned* d2; unsigned char* border; void* edt; size_t edt_bytes; double* partials; };

SlWs sl_carve(void* ws, int B, int H, int W, int K) {
    const size_t n = (size_t)K * B * H * W;
    char* base = (char*)ws;
    SlWs s;
    s.d2 = (unsigned*)base;
    s.border = (unsigned char*)(base + sl_align16(n * sizeof(unsigned)));
    s.edt = s.border + sl_align16(n);
    s.edt_bytes = sl_align16(uh_edt_sq_ws_bytes(K * B, H, W));
    s.partials = (double*)((char*)s.edt + s.edt_bytes);
    return s;
}

// border of every selected class, then D over the K * B border images into the workspace
int sl_build_d2(const char* who, const int64_t* mask, int mask_div, const SlClasses& cls, int B, int H, int W, const SlWs& s,
                hipStream_t st) {
    const long long hw = (long long)H * W;
    hipLaunchKernelGGL(sl_border_kernel, dim3((unsigned)((hw + 255) / 256), B), dim3(256), 0, st, mask, mask_div, cls, s.border, B, H, W);
    UH_CHECK_LAUNCH(who);
    return uh_edt_sq_u8(s.border, s.d2, cls.k * B, H, W, s.edt, s.edt_bytes, (uh_stream)st);
}

}  // namespace

extern "C" size_t uh_surface_loss_ws_bytes(int B, int H, int W, int K) {
    if (B <= 0 || H <= 0 || W <= 0 || K < 1 || K > SL_MAXC || (long long)K * B > 65535) return 0;
    const size_t n = (size_t)K * B * H * W;
    return sl_align16(n * sizeof(unsigned)) + sl_align16(n) + sl_align16(uh_edt_sq_ws_bytes(K * B, H, W)) +
           (size_t)LOSS_MAXBLK * sizeof(double) + 256;
}

#define SL_COMMON_CHECKS(who, ncls)                                                                             \
    if (!sl_shape_ok(who, B, H, W, K)) return UH_EINVAL;                                                        \
    UH_REQUIRE(mask_div > 0, who ": mask_div must be positive");                                                \
    SlClasses cls;                                                                                              \
    if (!sl_classes_ok(who, classes, K, ncls, &cls)) return UH_EINVAL;                                          \
    UH_REQUIRE(uh_aligned16(ws), who ": the workspace must be 16-byte aligned");                                \
    {                                                                                                           \
        const size_t need = uh_surface_loss_ws_bytes(B, H, W, K);                                               \
        if (ws_bytes < need) {                                                                                  \
            uh_set_error(who ": workspace %zu < %zu bytes", ws_bytes, need);                                    \
            return UH_EWORKSPACE;                                                                               \
        }                                                                                                       \
    }                                                                                                           \
    const SlWs s = sl_carve(ws, B, H, W, K);                                                                    \
    hipStream_t st = (hipStream_t)stream;                                                                       \
    const long long n = (long long)B * H * W

extern "C" int uh_surface_border_i64(const int64_t* mask, int mask_div, const int* classes, int K, uint8_t* border_out, int B, int H,
                                     int W, uh_stream stream) {
    UH_REQUIRE(mask && classes && border_out, "uh_surface_border_i64: null pointer");
    if (!sl_shape_ok("uh_surface_border_i64", B, H, W, K)) return UH_EINVAL;
    UH_REQUIRE(mask_div > 0, "uh_surface_border_i64: mask_div must be positive");
    SlClasses cls;
    if (!sl_classes_ok("uh_surface_border_i64", classes, K, 0, &cls)) return UH_EINVAL;
    const long long hw = (long long)H * W;
    hipLaunchKernelGGL(sl_border_kernel, dim3((unsigned)((hw + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, mask, mask_div, cls,
                       border_out, B, H, W);
    UH_CHECK_LAUNCH("uh_surface_border_i64");
    return UH_OK;
}

extern "C" int uh_surface_dist_map(const int64_t* mask, int mask_div, const int* classes, int K, float* phi_out, int B, int H, int W,
                                   void* ws, size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(mask && classes && phi_out && ws, "uh_surface_dist_map: null pointer");
    SL_COMMON_CHECKS("uh_surface_dist_map", 0);
    const int rc = sl_build_d2("uh_surface_dist_map", mask, mask_div, cls, B, H, W, s, st);
    if (rc != UH_OK) return rc;
    hipLaunchKernelGGL(sl_map_kernel, dim3(uh_flat_grid(n, UH_GRID_CAP), K), dim3(256), 0, st, (const unsigned*)s.d2, mask, mask_div, cls,
                       phi_out, n);
    UH_CHECK_LAUNCH("uh_surface_dist_map");
    return UH_OK;
}

extern "C" int uh_surface_loss_sums(const float* logits, const int64_t* mask, int mask_div, const int* classes, int K, int ncls, int B,
                                    int H, int W, double n_mean, float w, float* out, void* ws, size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(logits && mask && classes && out && ws, "uh_surface_loss_sums: null pointer");
    if (!uh_loss_head_ok("uh_surface_loss_sums", ncls, SL_MAXC)) return UH_EINVAL;
    UH_REQUIRE(n_mean > 0, "uh_surface_loss_sums: n_mean must be positive");
    SL_COMMON_CHECKS("uh_surface_loss_sums", ncls);
    const int rc = sl_build_d2("uh_surface_loss_sums", mask, mask_div, cls, B, H, W, s, st);
    if (rc != UH_OK) return rc;
    const int nblk = loss_nblk(n);
    uh_class_dispatch<SL_MAXC>(ncls, [&](auto nc) {
        hipLaunchKernelGGL((sl_sums_kernel<decltype(nc)::value>), dim3(nblk), dim3(256), 0, st, logits, mask, mask_div, cls,
                           (const unsigned*)s.d2, n, s.partials);
    });
    UH_CHECK_LAUNCH("uh_surface_loss_sums");
    hipLaunchKernelGGL(sl_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)s.partials, nblk, 1.0 / (n_mean * (double)K), w, out);
    UH_CHECK_LAUNCH("uh_surface_loss_sums");
    return UH_OK;
}

extern "C" int uh_surface_loss_grad(const float* logits, const int64_t* mask, int mask_div, const int* classes, int K, int ncls, int B,
                                    int H, int W, double n_mean, float w, const float* gscale, float* dlogits, int rebuild,
                                    void* ws, size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(logits && mask && classes && dlogits && ws, "uh_surface_loss_grad: null pointer");
    if (!uh_loss_head_ok("uh_surface_loss_grad", ncls, SL_MAXC)) return UH_EINVAL;
    UH_REQUIRE(n_mean > 0, "uh_surface_loss_grad: n_mean must be positive");
    SL_COMMON_CHECKS("uh_surface_loss_grad", ncls);
    if (rebuild) {
        const int rc = sl_build_d2("uh_surface_loss_grad", mask, mask_div, cls, B, H, W, s, st);
        if (rc != UH_OK) return rc;
    }
    const float scale = (float)((double)w / (n_mean * (double)K));
    const unsigned grid = uh_flat_grid(n, UH_GRID_CAP);
    uh_class_dispatch<SL_MAXC>(ncls, [&](auto nc) {
        hipLaunchKernelGGL((sl_grad_kernel<decltype(nc)::value>), dim3(grid), dim3(256), 0, st, logits, mask, mask_div, cls,
                           (const unsigned*)s.d2, n, scale, gscale, dlogits);
    });
    UH_CHECK_LAUNCH("uh_surface_loss_grad");
    return UH_OK;
}
