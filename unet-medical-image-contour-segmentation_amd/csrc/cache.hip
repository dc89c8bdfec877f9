// cache.hip -- device-resident dataset cache (DESIGN.md section 3 "Dataset cache"): cut a batch from the cached entries.
//   uh_cache_gather_u8  image_out[b] = the image_bytes bytes at items[b].image, mask_out[b] = the mask_bytes bytes at
//                       items[b].mask, for b < B: a pure copy of uint8, rows may repeat
// A source starts 16-byte aligned and is readable up to its length rounded up to 16 (the cache pads its entries), so a source
// is always read in whole aligned 16-byte units.  Item b of an output starts at b * bytes:
//   bytes % 16 == 0  every destination is aligned: 16-byte loads, 16-byte stores
//   otherwise        the destination of item b is off by d = (b * bytes) & 15.  Its first h = (16 - d) & 15 bytes and its last
//                    (bytes - h) % 16 bytes are written one by one; the aligned units between them are written with 16-byte
//                    stores, each formed from the two aligned source units that hold its bytes, shifted by h bytes in
//                    registers.  The second of the two starts below `bytes`, so it lies inside the padded source.
// Workgroup (chunk, row): CACHE_CHUNK bytes of one item's image or mask, CACHE_UNITS 16-byte units per thread, every load issued
// before the first store.  The item table is host memory: every row is checked before any launch, and the rows travel by
// value in the kernel arguments, CACHE_ROWS at a time.  Nothing here synchronises with the host, allocates or uses an atomic.
#include "uh_common.h"

namespace {

constexpr int CACHE_ROWS = 32;                               // table rows per launch
constexpr int CACHE_UNITS = 4;                               // 16-byte units per thread
constexpr size_t CACHE_CHUNK = (size_t)256 * CACHE_UNITS * 16;   // bytes per workgroup
constexpr size_t CACHE_MAX_BYTES = (size_t)1 << 40;          // per item: chunk counts stay far inside a grid dimension

struct CacheRow {
    const uint8_t* image;
    const uint8_t* mask;
};
struct CacheRows {
    CacheRow row[CACHE_ROWS];
};

__host__ __device__ inline unsigned cache_chunks(size_t bytes) { return (unsigned)((bytes + CACHE_CHUNK - 1) / CACHE_CHUNK); }

// the low 16 bytes of (hi : lo) >> 8 h, 0 < h < 16: dword i of the result starts h bytes into the eight dwords of lo, hi
__device__ __forceinline__ u32x4 cache_shift(u32x4 lo, u32x4 hi, unsigned h) {
    const unsigned w[9] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3], 0u};
    const unsigned q = h >> 2, s = h & 3;
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned a = w[i], c = w[i + 1];
        if (q == 1) a = w[i + 1], c = w[i + 2];
        if (q == 2) a = w[i + 2], c = w[i + 3];
        if (q == 3) a = w[i + 3], c = w[i + 4];
        v[i] = __builtin_amdgcn_alignbyte(c, a, s);
    }
    return v;
}

// one chunk of one item: src 16-byte aligned and readable to bytes rounded up to 16, dst = the item's first byte
template <bool ALIGNED>
__device__ __forceinline__ void cache_copy_chunk(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, size_t bytes,
                                                 unsigned chunk) {
    const unsigned h = ALIGNED ? 0u : (unsigned)((16 - ((uintptr_t)dst & 15)) & 15);      // the same for the whole workgroup
    const size_t head = h < bytes ? h : bytes;
    const size_t units = (bytes - head) >> 4;                                              // aligned destination units
    const size_t u0 = (size_t)chunk * (CACHE_CHUNK / 16);
    const u32x4* __restrict__ s16 = (const u32x4*)src;
    u32x4* __restrict__ d16 = (u32x4*)(dst + head);
    if (ALIGNED || h == 0) {
        u32x4 v[CACHE_UNITS];
#pragma unroll
        for (int j = 0; j < CACHE_UNITS; ++j) {
            const size_t u = u0 + (size_t)j * 256 + threadIdx.x;
            if (u < units) v[j] = s16[u];
        }
#pragma unroll
        for (int j = 0; j < CACHE_UNITS; ++j) {
            const size_t u = u0 + (size_t)j * 256 + threadIdx.x;
            if (u < units) d16[u] = v[j];
        }
    } else {
        u32x4 lo[CACHE_UNITS], hi[CACHE_UNITS];
#pragma unroll
        for (int j = 0; j < CACHE_UNITS; ++j) {
            const size_t u = u0 + (size_t)j * 256 + threadIdx.x;
            if (u < units) lo[j] = s16[u], hi[j] = s16[u + 1];        // 16 (u + 1) < head + 16 (u + 1) <= bytes
        }
#pragma unroll
        for (int j = 0; j < CACHE_UNITS; ++j) {
            const size_t u = u0 + (size_t)j * 256 + threadIdx.x;
            if (u < units) d16[u] = cache_shift(lo[j], hi[j], h);
        }
    }
    if (!ALIGNED && chunk == 0) {                                     // fewer than 16 bytes at either end
        const size_t tail0 = head + (units << 4);
        if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
        const size_t t = tail0 + (threadIdx.x - 64);                  // the second wave takes the tail
        if (threadIdx.x >= 64 && t < bytes) dst[t] = src[t];
    }
}

// grid (image chunks + mask chunks, rows): the first image_chunks workgroups of a row copy its image, the others its mask
template <bool ALIGNED>
__global__ __launch_bounds__(256) void cache_gather_kernel(CacheRows t, int row0, size_t image_bytes, size_t mask_bytes,
                                                           unsigned image_chunks, uint8_t* __restrict__ image_out,
                                                           uint8_t* __restrict__ mask_out) {
    const CacheRow& it = t.row[blockIdx.y];
    const size_t b = (size_t)row0 + blockIdx.y;
    if (blockIdx.x < image_chunks) cache_copy_chunk<ALIGNED>(it.image, image_out + b * image_bytes, image_bytes, blockIdx.x);
    else cache_copy_chunk<ALIGNED>(it.mask, mask_out + b * mask_bytes, mask_bytes, blockIdx.x - image_chunks);
}

}  // namespace

extern "C" int uh_cache_gather_u8(const uh_cache_item* items, int B, size_t image_bytes, size_t mask_bytes, uint8_t* image_out,
                                  uint8_t* mask_out, uh_stream stream) {
    UH_REQUIRE(items, "uh_cache_gather_u8: null pointer (items)");
    UH_REQUIRE(image_out || mask_out, "uh_cache_gather_u8: null pointer (no output)");
    UH_REQUIRE(B > 0 && B <= (1 << 20), "uh_cache_gather_u8: bad batch B=%d", B);
    UH_REQUIRE(!image_out || (image_bytes >= 1 && image_bytes <= CACHE_MAX_BYTES),
               "uh_cache_gather_u8: bad image_bytes %zu (1 .. 2^40)", image_bytes);
    UH_REQUIRE(!mask_out || (mask_bytes >= 1 && mask_bytes <= CACHE_MAX_BYTES), "uh_cache_gather_u8: bad mask_bytes %zu (1 .. 2^40)",
               mask_bytes);
    UH_REQUIRE(uh_aligned16(image_out) && uh_aligned16(mask_out), "uh_cache_gather_u8: misaligned buffer (outputs: 16 bytes)");
    for (int b = 0; b < B; ++b) {
        UH_REQUIRE(!image_out || items[b].image, "uh_cache_gather_u8: null pointer (image of row %d)", b);
        UH_REQUIRE(!mask_out || items[b].mask, "uh_cache_gather_u8: null pointer (mask of row %d)", b);
        UH_REQUIRE((!image_out || uh_aligned16(items[b].image)) && (!mask_out || uh_aligned16(items[b].mask)),
                   "uh_cache_gather_u8: misaligned buffer (row %d: 16 bytes)", b);
    }
    const unsigned ic = image_out ? cache_chunks(image_bytes) : 0u, mc = mask_out ? cache_chunks(mask_bytes) : 0u;
    const bool aligned = (!image_out || (image_bytes & 15) == 0) && (!mask_out || (mask_bytes & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    for (int row0 = 0; row0 < B; row0 += CACHE_ROWS) {
        const int rows = B - row0 < CACHE_ROWS ? B - row0 : CACHE_ROWS;
        CacheRows t = {};
        for (int i = 0; i < rows; ++i) t.row[i].image = items[row0 + i].image, t.row[i].mask = items[row0 + i].mask;
        const dim3 grid(ic + mc, (unsigned)rows), block(256);
        if (aligned) hipLaunchKernelGGL(cache_gather_kernel<true>, grid, block, 0, st, t, row0, image_bytes, mask_bytes, ic, image_out,
                                        mask_out);
        else hipLaunchKernelGGL(cache_gather_kernel<false>, grid, block, 0, st, t, row0, image_bytes, mask_bytes, ic, image_out,
                                mask_out);
        UH_CHECK_LAUNCH("cache_gather_kernel");
    }
    return UH_OK;
}
