// crop.hip -- patch training (DESIGN.md section 3 "Patch training"): one seeded, foreground-aware square crop per item.
//   per item (labels [H][W] int64, words r0..r3), with ny = H - size + 1, nx = W - size + 1, n = the number of pixels whose
//   label is a set bit of class_mask (labels outside 0..63 never count) and T = fg_threshold in [0, 2^32]:
//     foreground branch, iff n > 0 and r0 < T:  k = (r1 n) >> 32, (py, px) the k-th such pixel in raster order,
//         jy = (r2 size) >> 32, jx = (r3 size) >> 32, oy = clamp(py - jy, 0, ny - 1), ox = clamp(px - jx, 0, nx - 1)
//     uniform branch, otherwise:                oy = (r2 ny) >> 32, ox = (r3 nx) >> 32
//   uh_crop_select  the origins: pass 1 counts every item over CROP_CHUNKS contiguous pixel chunks (wave ballots and
//                   popcounts, one uint32 partial per chunk); pass 2, one workgroup per item, scans the partials to the chunk
//                   that holds k, walks it with ballot prefix counts to the pixel and writes the origin
//   uh_crop_gather  [oy, oy + size) x [ox, ox + size) of every item's image and labels into one batch: a pure copy
// The item table is host memory: every row is checked before any launch, and the rows travel by value in the kernel
// arguments, CROP_ROWS at a time.  Nothing here synchronises with the host, allocates or uses an atomic.
#include "uh_common.h"

namespace {

typedef unsigned long long u64;
typedef __attribute__((ext_vector_type(2))) unsigned long long u64x2;

constexpr int CROP_CHUNKS = 1024;      // partials per item
constexpr int CROP_ROWS = 32;          // table rows per launch
constexpr int CROP_MAX_SIDE = 16384;   // H, W: an item holds at most 2^28 pixels
constexpr int CROP_BAND = 4;           // rows of a crop per gather workgroup: one per wave

struct SelRow {
    const int64_t* labels;
    int H, W;
    unsigned r[4];
};
struct SelRows {
    SelRow row[CROP_ROWS];
};
struct GatRow {
    const void* image;
    const int64_t* labels;
    int H, W, ld, pad;
};
struct GatRows {
    GatRow row[CROP_ROWS];
};

// pixels per chunk of an item of `hw` pixels: ceil(hw / CROP_CHUNKS) rounded up to whole waves
__host__ __device__ inline int crop_chunk_len(int hw) { return (((hw + CROP_CHUNKS - 1) / CROP_CHUNKS) + 63) & ~63; }

__device__ __forceinline__ bool crop_hit(int64_t v, u64 mask) { return (u64)v < 64ull && ((mask >> (unsigned)v) & 1ull); }

__device__ __forceinline__ int crop_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------------------ select
// pass 1: workgroup (chunk, row) counts its chunk; a wave takes 64 consecutive pixels per ballot, four ballots in flight
__global__ __launch_bounds__(256) void crop_count_kernel(SelRows t, u64 mask, unsigned* __restrict__ partial) {
    __shared__ unsigned wsum[4];
    const SelRow& it = t.row[blockIdx.y];
    const int hw = it.H * it.W;
    const int len = crop_chunk_len(hw);
    const int c = blockIdx.x;
    const int p0 = c * len < hw ? c * len : hw;                       // c len <= 2^28 + 2^16
    const int p1 = p0 + len < hw ? p0 + len : hw;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t* __restrict__ lab = it.labels;
    unsigned cnt = 0;
    for (int base = p0 + w * 64; base < p1; base += 1024) {
        bool hit[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = base + j * 256 + lane;
            hit[j] = p < p1 && crop_hit(lab[p], mask);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cnt += (unsigned)__popcll(__ballot(hit[j]));
    }
    if (lane == 0) wsum[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * CROP_CHUNKS + c] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__device__ __forceinline__ void crop_write_origin(int32_t* __restrict__ o, bool fg, int py, int px, const SelRow& it, int size) {
    const int ny = it.H - size + 1, nx = it.W - size + 1;
    int oy, ox;
    if (fg) {
        const int jy = (int)(((u64)it.r[2] * (unsigned)size) >> 32), jx = (int)(((u64)it.r[3] * (unsigned)size) >> 32);
        oy = crop_clamp(py - jy, ny - 1);
        ox = crop_clamp(px - jx, nx - 1);
    } else {
        oy = (int)(((u64)it.r[2] * (unsigned)ny) >> 32);
        ox = (int)(((u64)it.r[3] * (unsigned)nx) >> 32);
    }
    o[0] = oy;
    o[1] = ox;
}

// pass 2: one workgroup per row.  Thread t owns partials 4t .. 4t + 3; an exclusive scan over the 256 threads finds the thread,
// then the chunk, that holds rank k.  The chunk is walked 1024 pixels at a time: a wave ballots four runs of 64 pixels, the
// four waves' counts meet in LDS (two buffers, so one barrier per step), and in the step that holds the rank the lane whose
// prefix count equals it writes the origin.
__global__ __launch_bounds__(256) void crop_pick_kernel(SelRows t, int row0, u64 mask, u64 threshold, int size,
                                                         const unsigned* __restrict__ partial, int32_t* __restrict__ origin,
                                                         unsigned* __restrict__ count) {
    __shared__ unsigned wtot[4];
    __shared__ unsigned found[2];                                     // chunk, rank inside it
    __shared__ unsigned wcnt[2][4];
    const SelRow& it = t.row[blockIdx.x];
    const int b = row0 + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned* __restrict__ part = partial + (size_t)b * CROP_CHUNKS;
    unsigned q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = part[4 * tid + j];
    const unsigned mine = q[0] + q[1] + q[2] + q[3];
    unsigned inc = mine;                                              // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wtot[w] = inc;
    if (tid == 0) found[0] = 0u, found[1] = ~0u;                      // a rank no chunk holds: the walk ends without a pixel
    __syncthreads();
    unsigned before = 0, n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < w) before += wtot[j];
        n += wtot[j];
    }
    if (tid == 0 && count) count[b] = n;
    int32_t* __restrict__ o = origin + 2 * (size_t)b;
    const bool fg = n > 0 && (u64)it.r[0] < threshold;
    if (!fg) {
        if (tid == 0) crop_write_origin(o, false, 0, 0, it, size);
        return;
    }
    const unsigned k = (unsigned)(((u64)it.r[1] * n) >> 32);          // < n
    const unsigned excl = before + inc - mine;
    if (k >= excl && k < excl + mine) {                               // exactly one thread: mine > 0
        unsigned rest = k - excl;
        int j = 0;
        while (j < 3 && rest >= q[j]) rest -= q[j], ++j;
        found[0] = (unsigned)(4 * tid + j);
        found[1] = rest;
    }
    __syncthreads();
    const int hw = it.H * it.W;
    const int len = crop_chunk_len(hw);
    const int c = (int)found[0];
    unsigned rest = found[1];
    const int p0 = c * len < hw ? c * len : hw;
    const int p1 = p0 + len < hw ? p0 + len : hw;
    const int64_t* __restrict__ lab = it.labels;
    int buf = 0;
    for (int base = p0; base < p1; base += 1024, buf ^= 1) {
        u64 bal[4];
        unsigned cw = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = base + w * 256 + j * 64 + lane;
            bal[j] = __ballot(p < p1 && crop_hit(lab[p], mask));
            cw += (unsigned)__popcll(bal[j]);
        }
        if (lane == 0) wcnt[buf][w] = cw;
        __syncthreads();
        unsigned pre = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned v = wcnt[buf][j];
            if (j < w) pre += v;
            tot += v;
        }
        if (rest >= tot) {                                            // the same for every thread of the workgroup
            rest -= tot;
            continue;
        }
        if (rest >= pre && rest < pre + cw) {                         // this wave holds the pixel
            unsigned local = rest - pre;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned cj = (unsigned)__popcll(bal[j]);
                if (local < cj) {
                    const u64 below = bal[j] & ((1ull << lane) - 1ull);
                    if (((bal[j] >> lane) & 1ull) && (unsigned)__popcll(below) == local) {
                        const int p = base + w * 256 + j * 64 + lane;
                        const int py = p / it.W;
                        crop_write_origin(o, true, py, p - py * it.W, it, size);
                    }
                    break;
                }
                local -= cj;
            }
        }
        return;
    }
    // the labels changed between the passes: the partials no longer describe them
    if (tid == 0) crop_write_origin(o, false, 0, 0, it, size);
}

// ------------------------------------------------------------------------------------------------------------ gather
// Workgroup (band, row): CROP_BAND rows of one crop, 64 lanes along a row, 4 rows at a time.  DENSE (ld == ld_out == C): a crop
// row is size C consecutive elements on both sides and a whole number of 16-byte units; the destination row is 16-byte
// aligned (checked by the host) and is written in such units, the source row is read in them where its address allows, in
// 4-byte units where that holds, element by element otherwise.  U: an unsigned integer as wide as the element -- a copy
// of bits.  Label rows: two 8-byte loads, one 16-byte store.
template <typename U, bool DENSE>
__global__ __launch_bounds__(256) void crop_gather_kernel(GatRows t, int row0, int C, int size, const int32_t* __restrict__ origin,
                                                           U* __restrict__ image_out, int ld_out, int64_t* __restrict__ labels_out,
                                                           int labels_wide) {
    constexpr int VEC = 16 / (int)sizeof(U);
    const GatRow& it = t.row[blockIdx.y];
    const int b = row0 + blockIdx.y;
    const int oy = crop_clamp(origin[2 * (size_t)b], it.H - size), ox = crop_clamp(origin[2 * (size_t)b + 1], it.W - size);
    const int r0 = blockIdx.x * CROP_BAND;
    const int r1 = r0 + CROP_BAND < size ? r0 + CROP_BAND : size;
    for (int r = r0 + threadIdx.y; r < r1; r += blockDim.y) {
        const size_t srow = (size_t)(oy + r) * it.W + ox, drow = ((size_t)b * size + r) * size;
        if (image_out) {
            const U* __restrict__ s = (const U*)it.image + srow * it.ld;
            U* __restrict__ d = image_out + drow * ld_out;
            if (DENSE) {
                const int units = size * C / VEC;
                const uintptr_t a = (uintptr_t)s;
                if ((a & 15) == 0) {
                    for (int e = threadIdx.x; e < units; e += 64) ((u32x4*)d)[e] = ((const u32x4*)s)[e];
                } else if (sizeof(U) == 4 || (a & 3) == 0) {
                    const unsigned* __restrict__ s4 = (const unsigned*)s;
                    for (int e = threadIdx.x; e < units; e += 64) {
                        u32x4 v;
                        v[0] = s4[4 * e], v[1] = s4[4 * e + 1], v[2] = s4[4 * e + 2], v[3] = s4[4 * e + 3];
                        ((u32x4*)d)[e] = v;
                    }
                } else if constexpr (sizeof(U) == 2) {                // 2-byte elements at an odd element offset
                    for (int e = threadIdx.x; e < units; e += 64) {
                        u32x4 v;
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            v[i] = (unsigned)s[8 * e + 2 * i] | ((unsigned)s[8 * e + 2 * i + 1] << 16);
                        ((u32x4*)d)[e] = v;
                    }
                }
            } else {
                for (int e = threadIdx.x; e < size * C; e += 64) {
                    const int x = e / C, ch = e - x * C;
                    d[(size_t)x * ld_out + ch] = s[(size_t)x * it.ld + ch];
                }
            }
        }
        if (labels_out) {
            const int64_t* __restrict__ s = it.labels + srow;
            int64_t* __restrict__ d = labels_out + drow;
            if (labels_wide) {
                for (int e = threadIdx.x; e < size / 2; e += 64) {
                    u64x2 v;
                    v[0] = (u64)s[2 * e], v[1] = (u64)s[2 * e + 1];
                    ((u64x2*)d)[e] = v;
                }
            } else {
                for (int e = threadIdx.x; e < size; e += 64) d[e] = s[e];
            }
        }
    }
}

bool crop_size_ok(int size) { return size >= 16 && size <= CROP_MAX_SIDE && (size & 15) == 0; }

}  // namespace

#define CROP_REQUIRE_ROWS(fn, need_labels)                                                                                      \
    for (int b = 0; b < B; ++b) {                                                                                               \
        const uh_crop_item& it = items[b];                                                                                      \
        UH_REQUIRE(it.H > 0 && it.W > 0 && it.H <= CROP_MAX_SIDE && it.W <= CROP_MAX_SIDE,                                      \
                   fn ": bad sizes in row %d: H=%d W=%d (1 <= H, W <= 16384)", b, it.H, it.W);                                  \
        UH_REQUIRE(it.H >= size && it.W >= size, fn ": row %d is smaller than the crop: H=%d W=%d size=%d", b, it.H, it.W,      \
                   size);                                                                                                       \
        UH_REQUIRE(!(need_labels) || it.labels, fn ": null pointer (labels of row %d)", b);                                     \
        UH_REQUIRE((((uintptr_t)it.labels) & 7) == 0, fn ": misaligned buffer (labels of row %d)", b);                          \
    }

extern "C" size_t uh_crop_select_ws_bytes(int B) { return B > 0 ? (size_t)B * CROP_CHUNKS * sizeof(unsigned) : 0; }

extern "C" int uh_crop_select(const uh_crop_item* items, int B, int size, uint64_t class_mask, uint64_t fg_threshold, int32_t* origin,
                              uint32_t* count, void* ws, size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(items && origin && ws, "uh_crop_select: null pointer");
    UH_REQUIRE(B > 0 && B <= (1 << 20), "uh_crop_select: bad batch B=%d", B);
    UH_REQUIRE(crop_size_ok(size), "uh_crop_select: bad size %d (a multiple of 16 in [16, 16384])", size);
    UH_REQUIRE(fg_threshold <= (1ull << 32), "uh_crop_select: bad fg_threshold %llu (at most 2^32)", (unsigned long long)fg_threshold);
    UH_REQUIRE((((uintptr_t)origin | (uintptr_t)count | (uintptr_t)ws) & 3) == 0, "uh_crop_select: misaligned buffer");
    UH_REQUIRE(ws_bytes >= uh_crop_select_ws_bytes(B), "uh_crop_select: workspace too small: %zu bytes, need %zu", ws_bytes,
               uh_crop_select_ws_bytes(B));
    CROP_REQUIRE_ROWS("uh_crop_select", true)
    hipStream_t st = (hipStream_t)stream;
    unsigned* partial = (unsigned*)ws;
    for (int row0 = 0; row0 < B; row0 += CROP_ROWS) {
        const int rows = B - row0 < CROP_ROWS ? B - row0 : CROP_ROWS;
        SelRows t = {};
        for (int i = 0; i < rows; ++i) {
            const uh_crop_item& it = items[row0 + i];
            t.row[i].labels = it.labels, t.row[i].H = it.H, t.row[i].W = it.W;
            for (int j = 0; j < 4; ++j) t.row[i].r[j] = it.r[j];
        }
        hipLaunchKernelGGL(crop_count_kernel, dim3(CROP_CHUNKS, (unsigned)rows), dim3(256), 0, st, t, (u64)class_mask,
                           partial + (size_t)row0 * CROP_CHUNKS);
        UH_CHECK_LAUNCH("crop_count_kernel");
        hipLaunchKernelGGL(crop_pick_kernel, dim3((unsigned)rows), dim3(256), 0, st, t, row0, (u64)class_mask, (u64)fg_threshold, size,
                           partial, origin, count);
        UH_CHECK_LAUNCH("crop_pick_kernel");
    }
    return UH_OK;
}

extern "C" int uh_crop_gather(const uh_crop_item* items, int B, int C, int dt, int size, const int32_t* origin, void* image_out,
                              int ld_out, int64_t* labels_out, uh_stream stream) {
    UH_REQUIRE(items && origin, "uh_crop_gather: null pointer");
    UH_REQUIRE(image_out || labels_out, "uh_crop_gather: null pointer (no output)");
    UH_REQUIRE(B > 0 && B <= (1 << 20), "uh_crop_gather: bad batch B=%d", B);
    UH_REQUIRE(crop_size_ok(size), "uh_crop_gather: bad size %d (a multiple of 16 in [16, 16384])", size);
    UH_REQUIRE(dt == UH_F32 || dt == UH_BF16, "uh_crop_gather: bad dtype %d", dt);
    UH_REQUIRE(C >= 1 && C <= 4, "uh_crop_gather: bad channels C=%d (1 .. 4)", C);
    UH_REQUIRE(!image_out || ld_out >= C, "uh_crop_gather: bad pixel stride ld_out=%d for C=%d", ld_out, C);
    const uintptr_t emask = dt == UH_BF16 ? 1 : 3;
    UH_REQUIRE((((uintptr_t)origin) & 3) == 0 && (((uintptr_t)image_out) & emask) == 0 && (((uintptr_t)labels_out) & 7) == 0,
               "uh_crop_gather: misaligned buffer");
    CROP_REQUIRE_ROWS("uh_crop_gather", labels_out != nullptr)
    bool dense = image_out && ld_out == C && uh_aligned16(image_out);
    if (image_out)
        for (int b = 0; b < B; ++b) {
            const uh_crop_item& it = items[b];
            UH_REQUIRE(it.image, "uh_crop_gather: null pointer (image of row %d)", b);
            UH_REQUIRE((((uintptr_t)it.image) & emask) == 0, "uh_crop_gather: misaligned buffer (image of row %d)", b);
            UH_REQUIRE(it.ld >= C, "uh_crop_gather: bad pixel stride ld=%d in row %d for C=%d", it.ld, b, C);
            dense = dense && it.ld == C;
        }
    hipStream_t st = (hipStream_t)stream;
    const int wide = uh_aligned16(labels_out) ? 1 : 0;
    for (int row0 = 0; row0 < B; row0 += CROP_ROWS) {
        const int rows = B - row0 < CROP_ROWS ? B - row0 : CROP_ROWS;
        GatRows t = {};
        for (int i = 0; i < rows; ++i) {
            const uh_crop_item& it = items[row0 + i];
            t.row[i].image = it.image, t.row[i].labels = it.labels, t.row[i].H = it.H, t.row[i].W = it.W, t.row[i].ld = it.ld;
        }
        const dim3 grid((unsigned)((size + CROP_BAND - 1) / CROP_BAND), (unsigned)rows), block(64, 4);
        if (dt == UH_BF16) {
            if (dense) hipLaunchKernelGGL((crop_gather_kernel<uint16_t, true>), grid, block, 0, st, t, row0, C, size, origin,
                                          (uint16_t*)image_out, ld_out, labels_out, wide);
            else hipLaunchKernelGGL((crop_gather_kernel<uint16_t, false>), grid, block, 0, st, t, row0, C, size, origin,
                                    (uint16_t*)image_out, ld_out, labels_out, wide);
        } else {
            if (dense) hipLaunchKernelGGL((crop_gather_kernel<uint32_t, true>), grid, block, 0, st, t, row0, C, size, origin,
                                          (uint32_t*)image_out, ld_out, labels_out, wide);
            else hipLaunchKernelGGL((crop_gather_kernel<uint32_t, false>), grid, block, 0, st, t, row0, C, size, origin,
                                    (uint32_t*)image_out, ld_out, labels_out, wide);
        }
        UH_CHECK_LAUNCH("crop_gather_kernel");
    }
    return UH_OK;
}
