// tta.hip -- test-time augmentation around the eval forward (DESIGN.md section 3 "Test-time augmentation"): the views of a batch
// of images under a subgroup of the eight poses of the square, and the merge of the views' logits back onto the source grid.
//   view v = 4 t + 2 fy + fx, "flip, then transpose":  a source pixel (y, x) of an H x W image lies in view v at
//   (yy, xx) for t = 0 and at (xx, yy) for t = 1 (a W x H view), yy = fy ? H-1-y : y, xx = fx ? W-1-x : x.
//   uh_tta_views   x [B][H][W][C] fp32 -> the t = 0 views [K0 B][H][W][C] and the t = 1 views [K1 B][W][H][C]: a pure copy
//   uh_tta_merge   the views' logits -> per pixel the integer sum over the views of rint(p * 2^24), its first maximum, its mean
// Nothing here synchronises with the host or allocates.
#include "uh_common.h"
#include "uh_quantise.h"

namespace {

constexpr int TTA_TILE = 32;                    // source pixels per tile side
constexpr int TTA_MAX_C = 8;                    // image channels a tile holds (32 x 33 C floats of LDS)

__host__ __device__ inline bool tta_mask_ok(int mask) { return mask == 0x03 || mask == 0x0F || mask == 0x69 || mask == 0xFF; }

// One workgroup copies one 32 x 32 pixel tile of image b to its place in every view.  The source rows are read once, lanes
// along the row; the t = 0 views are written straight from the registers (a flipped row is the same 128 C bytes, lanes in
// reverse order).  The t = 1 views go through LDS: the tile is stored row by row with a leading dimension of 33 C floats
// and read back along the source's columns, so that the lanes of a store again walk one output row.  With f = ty C + c
// the lanes of a column read touch the words 33 C ty + C px + c = f + const (mod 32): no two of 32 lanes on a bank.
__global__ __launch_bounds__(256) void tta_views_kernel(const float* __restrict__ x, float* __restrict__ views0,
                                                         float* __restrict__ views1, int B, int H, int W, int C, int mask) {
    extern __shared__ float tile[];             // [32][33 C]
    const int b = blockIdx.z;
    const int y0 = blockIdx.y * TTA_TILE, x0 = blockIdx.x * TTA_TILE;
    const int rowlen = TTA_TILE * C;            // floats of a tile row
    const int ld = (TTA_TILE + 1) * C;
    const int n = TTA_TILE * rowlen;
    const int64_t HW = (int64_t)H * W;
    for (int idx = threadIdx.x; idx < n; idx += 256) {
        const int ty = idx / rowlen, e = idx - ty * rowlen;
        const int px = e / C, c = e - px * C;
        const int y = y0 + ty, xs = x0 + px;
        if (y >= H || xs >= W) continue;        // tiles that hang over the right or bottom edge
        const float val = x[(((int64_t)b * H + y) * W + xs) * C + c];
        tile[ty * ld + e] = val;
        int k = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            if (!((mask >> v) & 1)) continue;
            const int yy = (v & 2) ? H - 1 - y : y, xx = (v & 1) ? W - 1 - xs : xs;
            views0[(((int64_t)k * B + b) * HW + (int64_t)yy * W + xx) * C + c] = val;
            ++k;
        }
    }
    if (!(mask >> 4)) return;                   // (uniform: no transposed view in this mode)
    __syncthreads();
    for (int idx = threadIdx.x; idx < n; idx += 256) {
        const int px = idx / rowlen, f = idx - px * rowlen;
        const int ty = f / C, c = f - ty * C;
        const int y = y0 + ty, xs = x0 + px;
        if (y >= H || xs >= W) continue;
        const float val = tile[ty * ld + px * C + c];
        int k = 0;
#pragma unroll
        for (int v = 4; v < 8; ++v) {
            if (!((mask >> v) & 1)) continue;
            const int yy = (v & 2) ? H - 1 - y : y, xx = (v & 1) ? W - 1 - xs : xs;
            views1[(((int64_t)k * B + b) * HW + (int64_t)xx * H + yy) * C + c] = val;       // a W x H view: row xx, column yy
            ++k;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ merge
// (the quantised probability, tta_quantise and its softmax: uh_quantise.h, shared with tiling.hip)
// the logits of source pixel (b, y, xs) in view v; k0 / k1 = how many t = 0 / t = 1 views of the mask precede v
template <typename T>
__device__ __forceinline__ const T* tta_at(const T* __restrict__ l0, const T* __restrict__ l1, int v, int k0, int k1, int B, int b,
                                           int H, int W, int y, int xs, int NC) {
    const int yy = (v & 2) ? H - 1 - y : y, xx = (v & 1) ? W - 1 - xs : xs;
    const int64_t HW = (int64_t)H * W;
    if (v & 4) return l1 + (((int64_t)k1 * B + b) * HW + (int64_t)xx * H + yy) * NC;
    return l0 + (((int64_t)k0 * B + b) * HW + (int64_t)yy * W + xx) * NC;
}

// A workgroup takes a 16 x 16 pixel tile, each wave an 8 x 8 quadrant of it, one pixel per thread: the lanes of a wave then
// read eight 8-pixel runs of a view's logits whether the view is transposed or not (rows of the source are columns of a
// t = 1 view), and the four waves of the workgroup complete each other's cache lines.
__device__ __forceinline__ bool tta_pixel(int H, int W, int& y, int& xs) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    xs = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    y = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    return y < H && xs < W;
}

// NC <= 4: everything in registers.  Softmax per view in fp32 (NC = 1: the sigmoid), quantised, summed as integers: the
// sum does not depend on the order of the views.
template <typename T, int NC>
__global__ __launch_bounds__(256) void tta_merge_kernel(const T* __restrict__ l0, const T* __restrict__ l1, int B, int H, int W,
                                                         int mask, unsigned* __restrict__ sums, uint8_t* __restrict__ classes,
                                                         float* __restrict__ probs) {
    int y, xs;
    if (!tta_pixel(H, W, y, xs)) return;
    const int b = blockIdx.z;
    unsigned acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0u;
    int k0 = 0, k1 = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        if (!((mask >> v) & 1)) continue;
        const T* p = tta_at<T>(l0, l1, v, k0, k1, B, b, H, W, y, xs, NC);
        if (v & 4) ++k1; else ++k0;
        unsigned q[NC];
        tta_quantised_probs<T, NC>(p, q);
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += q[c];
    }
    const int V = k0 + k1;
    const int64_t pix = ((int64_t)b * H + y) * W + xs;
    if (sums) {
#pragma unroll
        for (int c = 0; c < NC; ++c) sums[pix * NC + c] = acc[c];
    }
    if (probs) {
        const float inv = 1.0f / ((float)V * TTA_ONE);              // V is a power of two: exact
#pragma unroll
        for (int c = 0; c < NC; ++c) probs[pix * NC + c] = (float)acc[c] * inv;
    }
    if (classes) {
        unsigned idx = 0;
        if (NC == 1) {
            idx = acc[0] > ((unsigned)V << 23) ? 1u : 0u;            // the averaged sigmoid > 0.5
        } else {
            unsigned best = acc[0];
#pragma unroll
            for (int c = 1; c < NC; ++c)
                if (acc[c] > best) { best = acc[c]; idx = c; }       // first maximum
        }
        classes[pix] = (uint8_t)idx;
    }
}

// any class count: the maximum and the denominator of every view first (8 pairs of registers), then class by class
template <typename T>
__global__ __launch_bounds__(256) void tta_merge_generic_kernel(const T* __restrict__ l0, const T* __restrict__ l1, int B, int H,
                                                                 int W, int NC, int mask, unsigned* __restrict__ sums,
                                                                 uint8_t* __restrict__ classes, float* __restrict__ probs) {
    int y, xs;
    if (!tta_pixel(H, W, y, xs)) return;
    const int b = blockIdx.z;
    const T* ptr[8];
    float mx[8], den[8];
    int k0 = 0, k1 = 0;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        ptr[v] = nullptr;
        mx[v] = 0.f;
        den[v] = 1.f;
        if (!((mask >> v) & 1)) continue;
        const T* p = tta_at<T>(l0, l1, v, k0, k1, B, b, H, W, y, xs, NC);
        if (v & 4) ++k1; else ++k0;
        ptr[v] = p;
        tta_softmax_stats<T>(p, NC, mx[v], den[v]);
    }
    const int V = k0 + k1;
    const float inv = 1.0f / ((float)V * TTA_ONE);
    const int64_t pix = ((int64_t)b * H + y) * W + xs;
    unsigned best = 0u, idx = 0u;
    for (int c = 0; c < NC; ++c) {
        unsigned a = 0u;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            if (!((mask >> v) & 1)) continue;
            a += tta_quantised_prob<T>(ptr[v][c], mx[v], den[v]);
        }
        if (sums) sums[pix * NC + c] = a;
        if (probs) probs[pix * NC + c] = (float)a * inv;
        if (c == 0 || a > best) { best = a; idx = c; }
    }
    if (classes) classes[pix] = (uint8_t)idx;
}

template <typename T>
void tta_launch_merge(const T* l0, const T* l1, int B, int H, int W, int NC, int mask, unsigned* sums, uint8_t* classes,
                      float* probs, hipStream_t st) {
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), (unsigned)B), block(256);
    switch (NC) {
        case 1: hipLaunchKernelGGL((tta_merge_kernel<T, 1>), grid, block, 0, st, l0, l1, B, H, W, mask, sums, classes, probs); break;
        case 2: hipLaunchKernelGGL((tta_merge_kernel<T, 2>), grid, block, 0, st, l0, l1, B, H, W, mask, sums, classes, probs); break;
        case 3: hipLaunchKernelGGL((tta_merge_kernel<T, 3>), grid, block, 0, st, l0, l1, B, H, W, mask, sums, classes, probs); break;
        case 4: hipLaunchKernelGGL((tta_merge_kernel<T, 4>), grid, block, 0, st, l0, l1, B, H, W, mask, sums, classes, probs); break;
        default:
            hipLaunchKernelGGL((tta_merge_generic_kernel<T>), grid, block, 0, st, l0, l1, B, H, W, NC, mask, sums, classes, probs);
    }
}

bool tta_sizes_ok(int B, int H, int W) {
    // grid.z = B, grid.y = tiles of H; a view index stays far inside int64
    return B > 0 && H > 0 && W > 0 && B <= 65535 && (H + 15) / 16 <= 65535 && (int64_t)B * H * W < (1ll << 40);
}

}  // namespace

extern "C" int uh_tta_views(const float* x, float* views0, float* views1, int B, int H, int W, int C, int mask, uh_stream stream) {
    UH_REQUIRE(tta_mask_ok(mask), "uh_tta_views: bad mask 0x%x (hflip 0x03, flips 0x0f, rot4 0x69, d4 0xff)", mask);
    UH_REQUIRE(x && views0 && (views1 || !(mask >> 4)), "uh_tta_views: null pointer");
    UH_REQUIRE(tta_sizes_ok(B, H, W) && C >= 1 && C <= TTA_MAX_C, "uh_tta_views: bad sizes B=%d H=%d W=%d C=%d (C <= %d)", B, H, W, C,
               TTA_MAX_C);
    UH_REQUIRE((((uintptr_t)x | (uintptr_t)views0 | (uintptr_t)views1) & 3) == 0, "uh_tta_views: misaligned buffer");
    const dim3 grid((unsigned)((W + TTA_TILE - 1) / TTA_TILE), (unsigned)((H + TTA_TILE - 1) / TTA_TILE), (unsigned)B);
    const size_t lds = sizeof(float) * TTA_TILE * (TTA_TILE + 1) * C;
    hipLaunchKernelGGL(tta_views_kernel, grid, dim3(256), lds, (hipStream_t)stream, x, views0, views1, B, H, W, C, mask);
    UH_CHECK_LAUNCH("tta_views_kernel");
    return UH_OK;
}

extern "C" int uh_tta_merge(const void* logits0, const void* logits1, int dt, int B, int H, int W, int NC, int mask,
                            unsigned int* sums, uint8_t* classes, float* probs, uh_stream stream) {
    UH_REQUIRE(tta_mask_ok(mask), "uh_tta_merge: bad mask 0x%x (hflip 0x03, flips 0x0f, rot4 0x69, d4 0xff)", mask);
    UH_REQUIRE(logits0 && (logits1 || !(mask >> 4)), "uh_tta_merge: null pointer");
    UH_REQUIRE(sums || classes || probs, "uh_tta_merge: null pointer (no output)");
    UH_REQUIRE(dt == UH_F32 || dt == UH_BF16, "uh_tta_merge: bad dtype %d", dt);
    UH_REQUIRE(tta_sizes_ok(B, H, W) && NC >= 1 && NC <= 256, "uh_tta_merge: bad sizes B=%d H=%d W=%d NC=%d", B, H, W, NC);
    const uintptr_t la = (uintptr_t)logits0 | (uintptr_t)logits1;
    UH_REQUIRE((la & (dt == UH_BF16 ? 1 : 3)) == 0 && (((uintptr_t)sums | (uintptr_t)probs) & 3) == 0,
               "uh_tta_merge: misaligned buffer");
    hipStream_t st = (hipStream_t)stream;
    if (dt == UH_BF16)
        tta_launch_merge<bf16_t>((const bf16_t*)logits0, (const bf16_t*)logits1, B, H, W, NC, mask, sums, classes, probs, st);
    else
        tta_launch_merge<float>((const float*)logits0, (const float*)logits1, B, H, W, NC, mask, sums, classes, probs, st);
    UH_CHECK_LAUNCH("tta_merge_kernel");
    return UH_OK;
}
