// data_rescale.hip -- the rotate + rescale of BasicDataset items at scale < 1 (/root/reference/utils/data_loading.py:100-121,
// 66-70), moved from Pillow on the host to the device, byte for byte:
//   image: _rescaled(_quarter_turn(img, t), s, BICUBIC)   Pillow's ImagingResample for 8-bit data: the horizontal pass over
//          the rows the vertical pass reads, rounded to uint8, then the vertical pass, both with 22-bit integer taps built
//          on the host (utils/png_normalize.resample_coeffs);
//   mask:  _rescaled(_quarter_turn(mask, t), s, NEAREST)  Pillow's ImagingScaleAffine: out[y][x] = in[yi[y]][xi[x]] with
//          the index maps of its running double sum, built on the host (utils/data_rescale.nearest_index).
// The quarter turn comes first (the two passes round in between, so resizing before rotating is not the same operation).
// Neither side materialises a rotated copy: each workgroup loads the source block its output tile needs with lanes running
// along the source row (whatever the turn), stores it into LDS in rotated coordinates and computes from there.
// The output is uint8 [B][Ho][Wo][C] / [B][Ho][Wo]: uh_batch_prepare (turns = none) then divides, remaps and converts.
#include "uh_common.h"

namespace {

constexpr int RB_TX = 64;            // output columns per horizontal workgroup (one per lane)
constexpr int RB_TILE = 64;          // mask output tile
constexpr int RB_LDS_MAX = 64 * 1024;

// source pixel of rotated pixel (r, c) after `t` quarter turns counter-clockwise of an Hin x Win image (as data_prep.hip)
__device__ __forceinline__ void rb_source(int t, int r, int c, int Hin, int Win, int& gy, int& gx) {
    switch (t & 3) {
        case 0: gy = r; gx = c; break;
        case 1: gy = c; gx = Win - 1 - r; break;
        case 2: gy = Hin - 1 - r; gx = Win - 1 - c; break;
        default: gy = Hin - 1 - c; gx = r; break;
    }
}

__device__ __forceinline__ uint8_t rb_clip8(int acc) {             // Resample.c clip8 at PRECISION_BITS = 22
    if (acc >= (255 << 22) + (1 << 22)) return 255;
    if (acc <= 0) return 0;
    return (uint8_t)(acc >> 22);
}

// ImagingResampleHorizontal_8bpc of the rotated image (Hr x Wr) over its rows [row0, row0 + nrows), one RB_TX x rows tile
// per workgroup.  LDS: the rows x span source window (rotated coordinates, C bytes per pixel, pitch span * C), then the
// kh x RB_TX tap table.
template <int C>
__global__ __launch_bounds__(256) void rescale_h_kernel(const uint8_t* __restrict__ src, const int* __restrict__ turns, int Hin,
                                                         int Win, int Wr, const int* __restrict__ bounds,
                                                         const int* __restrict__ coef, int kh, int out_w, int row0, int nrows,
                                                         int rows, int span, uint8_t* __restrict__ tmp) {
    extern __shared__ int rb_lds[];
    int* s_k = rb_lds;                                            // [kh][RB_TX]
    uint8_t* s_px = reinterpret_cast<uint8_t*>(rb_lds + kh * RB_TX);
    const int b = blockIdx.z;
    const int t = turns ? (turns[b] & 3) : 0;
    const int c0 = blockIdx.x * RB_TX;
    const int r0 = blockIdx.y * rows;
    const int nr = min(rows, nrows - r0);
    const int c_last = min(c0 + RB_TX, out_w) - 1;
    const int xlo = bounds[2 * c0];
    const int w = min(bounds[2 * c_last] + bounds[2 * c_last + 1] - xlo, span);   // pixels of the window actually used
    for (int i = threadIdx.x; i < kh * RB_TX; i += 256) {
        const int j = i / RB_TX, cc = i % RB_TX, col = c0 + cc;
        s_k[j * RB_TX + cc] = col < out_w ? coef[(int64_t)col * kh + j] : 0;
    }
    // the window: lanes follow the source row -- the rotated row for even turns, the rotated column for odd ones
    const uint8_t* sb = src + (int64_t)b * Hin * Win * C;
    const int pitch = span * C;
    const int n = nr * w;
    for (int i = threadIdx.x; i < n; i += 256) {
        int ry, rx;
        if (t & 1) { rx = i / nr; ry = i - rx * nr; } else { ry = i / w; rx = i - ry * w; }
        int gy, gx;
        rb_source(t, row0 + r0 + ry, xlo + rx, Hin, Win, gy, gx);
        const bool ok = (unsigned)gy < (unsigned)Hin && (unsigned)gx < (unsigned)Win;
        const uint8_t* p = sb + ((int64_t)gy * Win + gx) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) s_px[ry * pitch + rx * C + ch] = ok ? p[ch] : (uint8_t)0;
    }
    __syncthreads();
    const int c = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = c0 + c;
    if (col >= out_w) return;
    const int off = bounds[2 * col] - xlo;
    int xn = min(bounds[2 * col + 1], kh);
    if (off < 0 || off + xn > w || bounds[2 * col] + xn > Wr) xn = 0;       // malformed table: never read outside the window
    for (int r = wave; r < nr; r += 4) {
        const uint8_t* row = s_px + r * pitch + off * C;
        uint8_t* o = tmp + (((int64_t)b * nrows + r0 + r) * out_w + col) * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            int acc = 1 << 21;
            for (int j = 0; j < xn; ++j) acc += (int)row[j * C + ch] * s_k[j * RB_TX + c];
            o[ch] = rb_clip8(acc);
        }
    }
}

// ImagingResampleVertical_8bpc: one output row of Wo * C bytes per (blockIdx.x-slice, blockIdx.y); bounds relative to row0
__global__ __launch_bounds__(256) void rescale_v_kernel(const uint8_t* __restrict__ tmp, int nrows, int row_bytes, int out_h,
                                                         const int* __restrict__ bounds, const int* __restrict__ coef, int kv,
                                                         uint8_t* __restrict__ dst) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= row_bytes) return;
    const int ymin = bounds[2 * y];
    int yn = min(bounds[2 * y + 1], kv);
    if (ymin < 0 || ymin + yn > nrows) yn = 0;
    const int* k = coef + (int64_t)y * kv;
    const uint8_t* col = tmp + ((int64_t)b * nrows + ymin) * row_bytes + e;
    int acc = 1 << 21;
    for (int j = 0; j < yn; ++j) acc += (int)col[(int64_t)j * row_bytes] * k[j];
    dst[((int64_t)b * out_h + y) * row_bytes + e] = rb_clip8(acc);
}

// NEAREST: out[y][x] = rotated[yi[y]][xi[x]], one 64 x 64 output tile per workgroup, gathered with lanes along the source
// row into LDS and written back row by row
__global__ __launch_bounds__(256) void rescale_nearest_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ turns,
                                                               int Hin, int Win, const int* __restrict__ xi,
                                                               const int* __restrict__ yi, int out_h, int out_w, int tilesX,
                                                               uint8_t* __restrict__ out) {
    __shared__ uint8_t s_m[RB_TILE][RB_TILE + 4];
    const int b = blockIdx.y;
    const int t = turns ? (turns[b] & 3) : 0;
    const int Y0 = (blockIdx.x / tilesX) * RB_TILE, X0 = (blockIdx.x % tilesX) * RB_TILE;
    const uint8_t* mb = mask + (int64_t)b * Hin * Win;
    for (int i = threadIdx.x; i < RB_TILE * RB_TILE; i += 256) {
        int oy, ox;
        if (t & 1) { ox = i / RB_TILE; oy = i % RB_TILE; } else { oy = i / RB_TILE; ox = i % RB_TILE; }
        const int y = Y0 + oy, x = X0 + ox;
        uint8_t v = 0;
        if (y < out_h && x < out_w) {
            int gy, gx;
            rb_source(t, yi[y], xi[x], Hin, Win, gy, gx);
            if ((unsigned)gy < (unsigned)Hin && (unsigned)gx < (unsigned)Win) v = mb[(int64_t)gy * Win + gx];
        }
        s_m[oy][ox] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RB_TILE * RB_TILE; i += 256) {
        const int oy = i / RB_TILE, ox = i % RB_TILE;
        const int y = Y0 + oy, x = X0 + ox;
        if (y < out_h && x < out_w) out[((int64_t)b * out_h + y) * out_w + x] = s_m[oy][ox];
    }
}

// rows of the horizontal tile and its LDS bytes for a window of `span` pixels: 16 rows (4 per wave) where they fit, else 4
int rb_rows(int kh, int span, int C, size_t* lds) {
    for (int rows : {16, 4}) {
        const size_t need = (size_t)kh * RB_TX * sizeof(int) + (size_t)rows * span * C;
        if (need <= (size_t)RB_LDS_MAX) { *lds = need; return rows; }
    }
    return 0;
}

}  // namespace

extern "C" size_t uh_batch_rescale_ws_bytes(int B, int C, int nrows, int out_w) {
    return (size_t)(B > 0 ? B : 0) * (size_t)(C > 0 ? C : 0) * (size_t)(nrows > 0 ? nrows : 0) * (size_t)(out_w > 0 ? out_w : 0) + 256;
}

extern "C" int uh_batch_rescale_u8(const uint8_t* img_u8, int C, const uint8_t* mask_u8, const int* turns, int odd_turns, int B,
                                   int Hin, int Win, const int* h_bounds, const int* h_coef, int kh, int span, int out_w,
                                   const int* v_bounds, const int* v_coef, int kv, int out_h, int row0, int nrows,
                                   const int* x_index, const int* y_index, uint8_t* img_out, uint8_t* mask_out, void* ws,
                                   size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(img_u8 || mask_u8, "uh_batch_rescale_u8: neither an image nor a mask batch");
    UH_REQUIRE(B > 0 && Hin > 0 && Win > 0 && out_w > 0 && out_h > 0, "uh_batch_rescale_u8: bad sizes B=%d %dx%d -> %dx%d",
               B, Hin, Win, out_h, out_w);
    UH_REQUIRE(odd_turns == 0 || odd_turns == 1, "uh_batch_rescale_u8: odd_turns is 0 or 1");
    UH_REQUIRE(odd_turns == 0 || turns, "uh_batch_rescale_u8: odd_turns without a turn table");
    UH_REQUIRE((int64_t)B * Hin * Win * 4 < (1ll << 40), "uh_batch_rescale_u8: batch too large");
    UH_REQUIRE(out_h <= 65535, "uh_batch_rescale_u8: output height %d > 65535", out_h);
    // the rotated size every item shares: Hin x Win for even turn counts, Win x Hin for odd ones
    const int Hr = odd_turns ? Win : Hin, Wr = odd_turns ? Hin : Win;
    UH_REQUIRE(out_w <= Wr && out_h <= Hr, "uh_batch_rescale_u8: %dx%d -> %dx%d is not a downscale", Hr, Wr, out_h, out_w);
    hipStream_t st = (hipStream_t)stream;
    if (img_u8) {
        UH_REQUIRE(C == 1 || C == 3, "uh_batch_rescale_u8: %d channels (1 or 3)", C);
        UH_REQUIRE(img_out && h_bounds && h_coef && v_bounds && v_coef && ws, "uh_batch_rescale_u8: image path: null pointer");
        UH_REQUIRE(kh >= 1 && kv >= 1 && span >= 1 && span <= Wr, "uh_batch_rescale_u8: bad filter sizes kh=%d kv=%d span=%d", kh, kv, span);
        UH_REQUIRE(row0 >= 0 && nrows > 0 && row0 + nrows <= Hr, "uh_batch_rescale_u8: rows [%d,%d) outside %d", row0, row0 + nrows, Hr);
        size_t lds = 0;
        const int rows = rb_rows(kh, span, C, &lds);
        UH_REQUIRE(rows > 0, "uh_batch_rescale_u8: a %d-pixel window with %d taps does not fit in %d bytes of LDS (scale too small)",
                   span, kh, RB_LDS_MAX);
        UH_REQUIRE((nrows + rows - 1) / rows <= 65535, "uh_batch_rescale_u8: too many rows");
        const size_t need = uh_batch_rescale_ws_bytes(B, C, nrows, out_w);
        if (ws_bytes < need) {
            uh_set_error("uh_batch_rescale_u8: workspace %zu < %zu bytes", ws_bytes, need);
            return UH_EWORKSPACE;
        }
        uint8_t* tmp = (uint8_t*)ws;
        dim3 gh((out_w + RB_TX - 1) / RB_TX, (nrows + rows - 1) / rows, B);
        if (C == 1)
            hipLaunchKernelGGL((rescale_h_kernel<1>), gh, dim3(256), lds, st, img_u8, turns, Hin, Win, Wr, h_bounds, h_coef, kh,
                               out_w, row0, nrows, rows, span, tmp);
        else
            hipLaunchKernelGGL((rescale_h_kernel<3>), gh, dim3(256), lds, st, img_u8, turns, Hin, Win, Wr, h_bounds, h_coef, kh,
                               out_w, row0, nrows, rows, span, tmp);
        UH_CHECK_LAUNCH("rescale_h_kernel");
        const int row_bytes = out_w * C;
        hipLaunchKernelGGL(rescale_v_kernel, dim3((row_bytes + 255) / 256, out_h, B), dim3(256), 0, st, (const uint8_t*)tmp, nrows,
                           row_bytes, out_h, v_bounds, v_coef, kv, img_out);
        UH_CHECK_LAUNCH("rescale_v_kernel");
    }
    if (mask_u8) {
        UH_REQUIRE(mask_out && x_index && y_index, "uh_batch_rescale_u8: mask path: null pointer");
        const int tilesX = (out_w + RB_TILE - 1) / RB_TILE, tilesY = (out_h + RB_TILE - 1) / RB_TILE;
        UH_REQUIRE((int64_t)tilesX * tilesY < (1ll << 31) && B <= 65535, "uh_batch_rescale_u8: mask grid too large");
        hipLaunchKernelGGL(rescale_nearest_kernel, dim3(tilesX * tilesY, B), dim3(256), 0, st, mask_u8, turns, Hin, Win, x_index,
                           y_index, out_h, out_w, tilesX, mask_out);
        UH_CHECK_LAUNCH("rescale_nearest_kernel");
    }
    return UH_OK;
}
