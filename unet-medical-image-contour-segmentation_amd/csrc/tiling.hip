// tiling.hip -- sliding-window tiled prediction (DESIGN.md section 3 "Tiled prediction"): an image is cut into tiles of one
// fixed shape, the tiles go through the eval forward, and a weighted integer merge puts their predictions back on the image grid.
//   per axis of length L:  tile length t = min(size, L); L <= size: one tile at 0; otherwise stride S = size - overlap,
//   n = ceil((L - size) / S) + 1 tiles at o_k = min(k S, L - size).  Only the last origin is ever clamped.
//   weight of position i in a tile of length t:  w(i) = max(1, min(i + 1, t - i, overlap));  a tile's weight is wy * wx <= 2^18.
//   uh_tile_grid    the counts, the tile shape and the origins, on the host
//   uh_tile_gather  x [B][H][W][C] fp32 -> tiles [B ny nx][th][tw][C]: a pure copy
//   uh_tile_merge   the tiles' logits (or the integer sums of uh_tta_merge) -> per image pixel the 64-bit sum over the covering
//                   tiles of wy wx q, the sum of the weights, the first maximum, the quotient
// Nothing here synchronises with the host, allocates or uses an atomic; no float enters a sum.
#include "uh_common.h"
#include "uh_quantise.h"

namespace {

typedef unsigned long long u64;

struct TileGeom {
    int H, W, size, overlap, S, ny, nx, th, tw;
};

__host__ __device__ inline bool tile_cfg_ok(int size, int overlap) {
    return size >= 16 && size <= 1024 && (size & 15) == 0 && overlap >= 0 && overlap <= size / 2;
}
__host__ __device__ inline int tile_axis_count(int L, int size, int S) { return L <= size ? 1 : (L - size + S - 1) / S + 1; }
__host__ __device__ inline int tile_origin(int k, int L, int size, int S) {
    if (L <= size) return 0;
    const int o = k * S, last = L - size;
    return o < last ? o : last;
}
__host__ __device__ inline int tile_weight(int i, int t, int overlap) {
    int w = i + 1 < t - i ? i + 1 : t - i;
    w = w < overlap ? w : overlap;
    return w > 1 ? w : 1;
}
// the tiles k0 .. k1 of an axis that hold position p (k1 - k0 <= 2): the regular tiles k with k S <= p < k S + size, and
// the clamped last one when p >= L - size
__host__ __device__ inline void tile_cover(int p, int L, int size, int S, int n, int& k0, int& k1) {
    if (L <= size) {
        k0 = k1 = 0;
        return;
    }
    k0 = p < size ? 0 : (p - size) / S + 1;
    k0 = k0 < n - 1 ? k0 : n - 1;
    k1 = p >= L - size ? n - 1 : p / S;
}

TileGeom tile_geom(int H, int W, int size, int overlap) {
    TileGeom g;
    g.H = H, g.W = W, g.size = size, g.overlap = overlap, g.S = size - overlap;
    g.ny = tile_axis_count(H, size, g.S), g.nx = tile_axis_count(W, size, g.S);
    g.th = H < size ? H : size, g.tw = W < size ? W : size;
    return g;
}

// ------------------------------------------------------------------------------------------------------------ gather
// A workgroup copies a band of rows of one tile.  A tile row is tw C consecutive floats in the image and in the tile, so the
// lanes walk along it: blockDim.x (a power of two <= 64, chosen by the host from the row length) lanes per row, blockDim.y
// rows at a time.  VEC = 4: rows are whole 16-byte units and the tile rows are 16-byte aligned; the image row is read in
// 16-byte units where its address allows (the same for every lane of a row) and float by float otherwise.  VEC = 1: float
// by float (a tile row that is no multiple of 4 floats: an image narrower than the tile).  No tile reaches outside the
// image (there is no padding), so only the lanes past the end of a row and the rows past the end of the band are masked.
template <int VEC>
__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ x, float* __restrict__ tiles, TileGeom g, int C,
                                                           int band) {
    const int n = blockIdx.x;
    const int per = g.ny * g.nx;
    const int b = n / per, t = n - b * per;
    const int ky = t / g.nx, kx = t - ky * g.nx;
    const int oy = tile_origin(ky, g.H, g.size, g.S), ox = tile_origin(kx, g.W, g.size, g.S);
    const int rowlen = g.tw * C / VEC;
    const float* __restrict__ src = x + (((int64_t)b * g.H + oy) * g.W + ox) * C;
    float* __restrict__ dst = tiles + (int64_t)n * g.th * g.tw * C;
    const int r0 = blockIdx.y * band;
    const int r1 = r0 + band < g.th ? r0 + band : g.th;
    for (int r = r0 + threadIdx.y; r < r1; r += blockDim.y) {
        const float* __restrict__ s = src + (int64_t)r * g.W * C;
        float* __restrict__ d = dst + (int64_t)r * g.tw * C;
        if (VEC == 4) {
            if ((((uintptr_t)s) & 15) == 0) {
                for (int e = threadIdx.x; e < rowlen; e += blockDim.x) ((f32x4*)d)[e] = ((const f32x4*)s)[e];
            } else {
                for (int e = threadIdx.x; e < rowlen; e += blockDim.x) {
                    f32x4 v;
                    v[0] = s[4 * e], v[1] = s[4 * e + 1], v[2] = s[4 * e + 2], v[3] = s[4 * e + 3];
                    ((f32x4*)d)[e] = v;
                }
            }
        } else {
            for (int e = threadIdx.x; e < rowlen; e += blockDim.x) d[e] = s[e];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ merge
// NC values of U from / to p; AL: p is aligned to min(16, NC sizeof(U)) bytes (a power-of-two NC sizeof(U) and a 16-byte aligned
// base, checked by the host), so the copy is one or two wide accesses
template <typename U, int NC, bool AL>
__device__ __forceinline__ void tile_load(const U* __restrict__ p, U (&v)[NC]) {
    constexpr int BYTES = NC * (int)sizeof(U);
    constexpr bool WIDE = AL && (BYTES & (BYTES - 1)) == 0 && BYTES >= 4;
    if constexpr (WIDE) {
        __builtin_memcpy(v, __builtin_assume_aligned(p, BYTES < 16 ? BYTES : 16), BYTES);
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = p[c];
    }
}
template <typename U, int NC, bool AL>
__device__ __forceinline__ void tile_store(U* __restrict__ p, const U (&v)[NC]) {
    constexpr int BYTES = NC * (int)sizeof(U);
    constexpr bool WIDE = AL && (BYTES & (BYTES - 1)) == 0 && BYTES >= 4;
    if constexpr (WIDE) {
        __builtin_memcpy(__builtin_assume_aligned(p, BYTES < 16 ? BYTES : 16), v, BYTES);
    } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) p[c] = v[c];
    }
}

template <typename T> struct tile_is_int { static constexpr bool value = false; };
template <> struct tile_is_int<int> { static constexpr bool value = true; };

// q of one tile pixel: the quantised probabilities of its logits (uh_quantise.h, as uh_tta_merge), or the sums of
// uh_tta_merge as they are
template <typename T, int NC, bool AL>
__device__ __forceinline__ void tile_pixel_q(const T* __restrict__ p, unsigned (&q)[NC]) {
    T l[NC];
    tile_load<T, NC, AL>(p, l);
    if constexpr (tile_is_int<T>::value) {
#pragma unroll
        for (int c = 0; c < NC; ++c) q[c] = (unsigned)l[c];
    } else {
        tta_quantised_probs<T, NC>(l, q);
    }
}

__device__ __forceinline__ float tile_quotient(u64 sum, double unit) { return (float)((double)sum / unit); }

// A workgroup takes 4 rows of 64 image pixels, one wave per row, one pixel per thread: the lanes of a wave read every
// covering tile in one contiguous run of 64 NC values (two runs where the wave crosses a tile's edge) and write 64
// consecutive pixels of every output.  NC <= 4: everything in registers.
template <typename T, int NC, bool AL>
__global__ __launch_bounds__(256) void tile_merge_kernel(const T* __restrict__ src, TileGeom g, int views, u64* __restrict__ sums,
                                                          unsigned* __restrict__ den, uint8_t* __restrict__ classes,
                                                          float* __restrict__ probs) {
    const int xs = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (xs >= g.W || y >= g.H) return;
    const int b = blockIdx.z;
    int ky0, ky1, kx0, kx1;
    tile_cover(y, g.H, g.size, g.S, g.ny, ky0, ky1);
    tile_cover(xs, g.W, g.size, g.S, g.nx, kx0, kx1);
    u64 acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0ull;
    unsigned d = 0u;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int ky = ky0 + j;
        if (ky > ky1) continue;
        const int iy = y - tile_origin(ky, g.H, g.size, g.S);
        const int wy = tile_weight(iy, g.th, g.overlap);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int kx = kx0 + i;
            if (kx > kx1) continue;
            const int ix = xs - tile_origin(kx, g.W, g.size, g.S);
            const unsigned w = (unsigned)(wy * tile_weight(ix, g.tw, g.overlap));
            const int64_t n = ((int64_t)b * g.ny + ky) * g.nx + kx;
            unsigned q[NC];
            tile_pixel_q<T, NC, AL>(src + ((n * g.th + iy) * g.tw + ix) * NC, q);
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] += (u64)w * q[c];
            d += w;
        }
    }
    const int64_t pix = ((int64_t)b * g.H + y) * g.W + xs;
    if (sums) tile_store<u64, NC, AL>(sums + pix * NC, acc);
    if (den) den[pix] = d;
    if (probs) {
        const double unit = (double)d * (double)views * 16777216.0;         // exact: < 2^22 * 2^3 * 2^24
        float p[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) p[c] = tile_quotient(acc[c], unit);
        tile_store<float, NC, AL>(probs + pix * NC, p);
    }
    if (classes) {
        unsigned idx = 0;
        if (NC == 1) {
            idx = acc[0] > (((u64)d * (unsigned)views) << 23) ? 1u : 0u;      // 2 sum > den views 2^24
        } else {
            u64 best = acc[0];
#pragma unroll
            for (int c = 1; c < NC; ++c)
                if (acc[c] > best) { best = acc[c]; idx = c; }               // first maximum
        }
        classes[pix] = (uint8_t)idx;
    }
}

// any class count: the pointer, the weight and (logits) the maximum and the denominator of every covering tile first, nine
// slots in registers, then class by class
template <typename T>
__global__ __launch_bounds__(256) void tile_merge_generic_kernel(const T* __restrict__ src, TileGeom g, int NC, int views,
                                                                  u64* __restrict__ sums, unsigned* __restrict__ den,
                                                                  uint8_t* __restrict__ classes, float* __restrict__ probs) {
    const int xs = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (xs >= g.W || y >= g.H) return;
    const int b = blockIdx.z;
    int ky0, ky1, kx0, kx1;
    tile_cover(y, g.H, g.size, g.S, g.ny, ky0, ky1);
    tile_cover(xs, g.W, g.size, g.S, g.nx, kx0, kx1);
    const T* ptr[9];
    float mx[9], sd[9];
    unsigned wt[9];
    unsigned d = 0u;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int s = 3 * j + i;
            const int ky = ky0 + j, kx = kx0 + i;
            ptr[s] = nullptr;
            mx[s] = 0.f;
            sd[s] = 1.f;
            wt[s] = 0u;
            if (ky > ky1 || kx > kx1) continue;
            const int iy = y - tile_origin(ky, g.H, g.size, g.S), ix = xs - tile_origin(kx, g.W, g.size, g.S);
            const int64_t n = ((int64_t)b * g.ny + ky) * g.nx + kx;
            ptr[s] = src + ((n * g.th + iy) * g.tw + ix) * NC;
            wt[s] = (unsigned)(tile_weight(iy, g.th, g.overlap) * tile_weight(ix, g.tw, g.overlap));
            d += wt[s];
            if constexpr (!tile_is_int<T>::value) tta_softmax_stats<T>(ptr[s], NC, mx[s], sd[s]);
        }
    }
    const int64_t pix = ((int64_t)b * g.H + y) * g.W + xs;
    const double unit = (double)d * (double)views * 16777216.0;
    u64 best = 0ull;
    unsigned idx = 0u;
    for (int c = 0; c < NC; ++c) {
        u64 a = 0ull;
#pragma unroll
        for (int s = 0; s < 9; ++s) {
            if (!wt[s]) continue;
            unsigned q;
            if constexpr (tile_is_int<T>::value) q = (unsigned)ptr[s][c];
            else q = tta_quantised_prob<T>(ptr[s][c], mx[s], sd[s]);
            a += (u64)wt[s] * q;
        }
        if (sums) sums[pix * NC + c] = a;
        if (probs) probs[pix * NC + c] = tile_quotient(a, unit);
        if (c == 0 || a > best) { best = a; idx = c; }
    }
    if (den) den[pix] = d;
    if (classes) classes[pix] = (uint8_t)idx;
}

template <typename T, bool AL>
void tile_launch_merge_nc(const T* src, const TileGeom& g, int B, int NC, int views, u64* sums, unsigned* den, uint8_t* classes,
                          float* probs, hipStream_t st) {
    const dim3 grid((unsigned)((g.W + 63) / 64), (unsigned)((g.H + 3) / 4), (unsigned)B), block(64, 4);
    switch (NC) {
        case 1: hipLaunchKernelGGL((tile_merge_kernel<T, 1, AL>), grid, block, 0, st, src, g, views, sums, den, classes, probs); break;
        case 2: hipLaunchKernelGGL((tile_merge_kernel<T, 2, AL>), grid, block, 0, st, src, g, views, sums, den, classes, probs); break;
        case 3: hipLaunchKernelGGL((tile_merge_kernel<T, 3, AL>), grid, block, 0, st, src, g, views, sums, den, classes, probs); break;
        case 4: hipLaunchKernelGGL((tile_merge_kernel<T, 4, AL>), grid, block, 0, st, src, g, views, sums, den, classes, probs); break;
        default:
            hipLaunchKernelGGL((tile_merge_generic_kernel<T>), grid, block, 0, st, src, g, NC, views, sums, den, classes, probs);
    }
}

template <typename T>
void tile_launch_merge(const T* src, const TileGeom& g, int B, int NC, int views, bool aligned, u64* sums, unsigned* den,
                       uint8_t* classes, float* probs, hipStream_t st) {
    if (aligned) tile_launch_merge_nc<T, true>(src, g, B, NC, views, sums, den, classes, probs, st);
    else tile_launch_merge_nc<T, false>(src, g, B, NC, views, sums, den, classes, probs, st);
}

bool tile_sizes_ok(int B, int H, int W, const TileGeom& g) {
    // grid.z = B, grid.y = H / 4 (merge); grid.x = B ny nx (gather); every element index stays far inside int64
    return B > 0 && H > 0 && W > 0 && B <= 65535 && (H + 3) / 4 <= 65535 && (int64_t)B * H * W < (1ll << 40) &&
           (int64_t)B * g.ny * g.nx < (1ll << 31);
}

}  // namespace

extern "C" int uh_tile_grid(int H, int W, int size, int overlap, int* ny, int* nx, int* th, int* tw, int* oy, int* ox) {
    UH_REQUIRE(tile_cfg_ok(size, overlap), "uh_tile_grid: bad config size=%d overlap=%d (size a multiple of 16 in [16, 1024], "
               "0 <= overlap <= size / 2)", size, overlap);
    UH_REQUIRE(H > 0 && W > 0, "uh_tile_grid: bad sizes H=%d W=%d", H, W);
    const TileGeom g = tile_geom(H, W, size, overlap);
    if (ny) *ny = g.ny;
    if (nx) *nx = g.nx;
    if (th) *th = g.th;
    if (tw) *tw = g.tw;
    if (oy)
        for (int k = 0; k < g.ny; ++k) oy[k] = tile_origin(k, H, size, g.S);
    if (ox)
        for (int k = 0; k < g.nx; ++k) ox[k] = tile_origin(k, W, size, g.S);
    return UH_OK;
}

extern "C" int uh_tile_gather(const float* x, float* tiles, int B, int H, int W, int C, int size, int overlap, uh_stream stream) {
    UH_REQUIRE(tile_cfg_ok(size, overlap), "uh_tile_gather: bad config size=%d overlap=%d (size a multiple of 16 in [16, 1024], "
               "0 <= overlap <= size / 2)", size, overlap);
    UH_REQUIRE(x && tiles, "uh_tile_gather: null pointer");
    UH_REQUIRE(H > 0 && W > 0, "uh_tile_gather: bad sizes B=%d H=%d W=%d C=%d (C <= 8)", B, H, W, C);
    const TileGeom g = tile_geom(H, W, size, overlap);
    UH_REQUIRE(tile_sizes_ok(B, H, W, g) && C >= 1 && C <= 8, "uh_tile_gather: bad sizes B=%d H=%d W=%d C=%d (C <= 8)", B, H, W, C);
    UH_REQUIRE((((uintptr_t)x | (uintptr_t)tiles) & 3) == 0, "uh_tile_gather: misaligned buffer");
    const bool vec = (g.tw * C) % 4 == 0 && uh_aligned16(tiles);
    const int rowlen = vec ? g.tw * C / 4 : g.tw * C;
    int bx = 1;
    while (bx < 64 && bx < rowlen) bx *= 2;
    const int by = 256 / bx, band = 4 * by;
    const dim3 grid((unsigned)(B * g.ny * g.nx), (unsigned)((g.th + band - 1) / band)), block((unsigned)bx, (unsigned)by);
    if (vec) hipLaunchKernelGGL(tile_gather_kernel<4>, grid, block, 0, (hipStream_t)stream, x, tiles, g, C, band);
    else hipLaunchKernelGGL(tile_gather_kernel<1>, grid, block, 0, (hipStream_t)stream, x, tiles, g, C, band);
    UH_CHECK_LAUNCH("tile_gather_kernel");
    return UH_OK;
}

extern "C" int uh_tile_merge(const void* src, int kind, int views, int B, int H, int W, int NC, int size, int overlap,
                             unsigned long long* sums, unsigned int* den, uint8_t* classes, float* probs, uh_stream stream) {
    UH_REQUIRE(tile_cfg_ok(size, overlap), "uh_tile_merge: bad config size=%d overlap=%d (size a multiple of 16 in [16, 1024], "
               "0 <= overlap <= size / 2)", size, overlap);
    UH_REQUIRE(src, "uh_tile_merge: null pointer");
    UH_REQUIRE(sums || den || classes || probs, "uh_tile_merge: null pointer (no output)");
    UH_REQUIRE(kind == UH_F32 || kind == UH_BF16 || kind == UH_TILE_SUMS_I32, "uh_tile_merge: bad kind %d", kind);
    UH_REQUIRE(views == 1 || views == 2 || views == 4 || views == 8, "uh_tile_merge: bad views %d (1, 2, 4 or 8)", views);
    UH_REQUIRE(kind == UH_TILE_SUMS_I32 || views == 1, "uh_tile_merge: bad views %d (logits are one view)", views);
    UH_REQUIRE(H > 0 && W > 0, "uh_tile_merge: bad sizes B=%d H=%d W=%d NC=%d", B, H, W, NC);
    const TileGeom g = tile_geom(H, W, size, overlap);
    UH_REQUIRE(tile_sizes_ok(B, H, W, g) && NC >= 1 && NC <= 256, "uh_tile_merge: bad sizes B=%d H=%d W=%d NC=%d", B, H, W, NC);
    UH_REQUIRE((((uintptr_t)src) & (kind == UH_BF16 ? 1 : 3)) == 0 && (((uintptr_t)sums) & 7) == 0 &&
               ((((uintptr_t)den | (uintptr_t)probs)) & 3) == 0, "uh_tile_merge: misaligned buffer");
    const bool aligned = uh_aligned16(src) && uh_aligned16(sums) && uh_aligned16(probs);
    u64* s64 = (u64*)sums;
    hipStream_t st = (hipStream_t)stream;
    if (kind == UH_BF16) tile_launch_merge<bf16_t>((const bf16_t*)src, g, B, NC, views, aligned, s64, den, classes, probs, st);
    else if (kind == UH_F32) tile_launch_merge<float>((const float*)src, g, B, NC, views, aligned, s64, den, classes, probs, st);
    else tile_launch_merge<int>((const int*)src, g, B, NC, views, aligned, s64, den, classes, probs, st);
    UH_CHECK_LAUNCH("tile_merge_kernel");
    return UH_OK;
}
