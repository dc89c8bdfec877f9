// seg_pipeline.hip -- the non-inference stages of the reference's seg_main.py (RAW -> LabelMe polygons), batched over B
// images of one geometry:
//   utils/raw2png.py        window / level of a 16-bit RAW to uint8                           -> uh_window_u16
//   utils/png_normalize.py  PIL LANCZOS resize + paste on a zero 512 x 512 canvas              -> uh_resample_lanczos_u8
//   utils/png_denormalize.py crop of the letterbox + PIL LANCZOS back to the original size     -> uh_resample_lanczos_u8
//   utils/mask2polygon.py   cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) of grey > 127 -> uh_contours_count / _emit
//
// The resampler is Pillow's ImagingResample for 8-bit images, integer for integer: the host builds the bounds and the
// 22-bit fixed-point coefficient tables in float64 once per geometry (png_normalize.py); the kernels only multiply and add.
// The contour tracer restates OpenCV's icvFetchContour (legacy C API, method CHAIN_APPROX_SIMPLE) one wave per contour,
// on per-pixel 8-neighbour bytes held in an LDS window.  PARITY UNPINNED against OpenCV (not installed here); the tests
// compare with a literal Python restatement and with hand-derived answers.
#include "uh_common.h"
#include "uh_union_find.h"

typedef __attribute__((ext_vector_type(2))) int i32x2;

namespace {

// ------------------------------------------------------------------------------------------------ window / level
// raw2png.py:_apply_windowing, numpy 1.26 semantics: out = uint8(trunc(float64(clip(x, mn, mx) - mn) / float64(mx - mn)
// * 255.0)); IEEE division and product in double (no fast-math), so every one of the 65 536 codes matches.
__device__ __forceinline__ uint32_t sp_window1(uint32_t x, long long mn, long long mx, double span) {
    long long c = (long long)x;
    c = c < mn ? mn : (c > mx ? mx : c);
    const double v = __dmul_rn(__ddiv_rn((double)(c - mn), span), 255.0);
    return (uint32_t)v;                                            // v in [0, 255]: truncation == astype(uint8)
}

__global__ __launch_bounds__(256) void window_u16_kernel(const uint16_t* __restrict__ raw, int64_t n, long long mn,
                                                          long long mx, double span, uint8_t* __restrict__ out) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i + 8 <= n) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(raw + i);
        u32x2 o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            uint32_t w = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t word = v[2 * h + (k >> 1)];
                w |= sp_window1((k & 1) ? (word >> 16) : (word & 0xffffu), mn, mx, span) << (8 * k);
            }
            o[h] = w;
        }
        *reinterpret_cast<u32x2*>(out + i) = o;
    } else {
        for (int64_t k = i; k < n; ++k) out[k] = (uint8_t)sp_window1(raw[k], mn, mx, span);
    }
}

// ------------------------------------------------------------------------------------------------ LANCZOS resample
constexpr int RS_TX = 64;            // output columns per horizontal workgroup (one per lane)
constexpr int RS_ROWS = 16;          // source rows per horizontal workgroup (4 per wave)
constexpr int RS_KMAX = 128;         // widest horizontal filter held in LDS: 128 x 64 int32 = 32 KiB

__device__ __forceinline__ uint8_t sp_clip8(int acc) {             // Resample.c clip8 at PRECISION_BITS = 22
    if (acc >= (255 << 22) + (1 << 22)) return 255;
    if (acc <= 0) return 0;
    return (uint8_t)(acc >> 22);
}

// ImagingResampleHorizontal_8bpc over the nrows source rows the vertical pass needs (row0 = first of them, relative to
// the source box).  The source byte goes through lut[] first (identity for the letterbox, class -> grey for the inverse).
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, int box_x, int box_y,
                                                          int box_w, int box_h, const uint8_t* __restrict__ lut,
                                                          const int* __restrict__ bounds, const int* __restrict__ coef, int kh,
                                                          int out_w, int row0, int nrows, uint8_t* __restrict__ tmp) {
    __shared__ int s_k[RS_KMAX][RS_TX];
    __shared__ int s_xmin[RS_TX], s_xn[RS_TX];
    __shared__ uint8_t s_lut[256];
    const int b = blockIdx.z;
    const int c = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col0 = blockIdx.x * RS_TX;
    for (int i = threadIdx.x; i < kh * RS_TX; i += 256) {
        const int j = i / RS_TX, cc = i % RS_TX, col = col0 + cc;
        s_k[j][cc] = col < out_w ? coef[(int64_t)col * kh + j] : 0;
    }
    if (threadIdx.x < RS_TX) {
        const int col = col0 + threadIdx.x;
        s_xmin[threadIdx.x] = col < out_w ? bounds[2 * col] : 0;
        s_xn[threadIdx.x] = col < out_w ? bounds[2 * col + 1] : 0;
    }
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int col = col0 + c;
    if (col >= out_w) return;
    const int xmin = s_xmin[c];
    int xn = s_xn[c];
    if (xn > kh) xn = kh;
    if (xmin < 0 || xmin + xn > box_w) xn = 0;                   // malformed table: never read outside the box
    for (int r = blockIdx.y * RS_ROWS + wave; r < nrows && r < (blockIdx.y + 1) * RS_ROWS; r += 4) {
        const int sy = row0 + r;
        int acc = 1 << 21;
        if (sy >= 0 && sy < box_h) {
            const uint8_t* row = src + ((int64_t)b * Hs + box_y + sy) * Ws + box_x + xmin;
            for (int j = 0; j < xn; ++j) acc += (int)s_lut[row[j]] * s_k[j][c];
        }
        tmp[((int64_t)b * nrows + r) * out_w + col] = sp_clip8(acc);
    }
}

// ImagingResampleVertical_8bpc, written straight into the (Hd x Wd) destination: the resampled block sits at (px, py),
// every other pixel is 0 (the zero canvas of png_normalize.py:552-557).  One output row per workgroup: the filter row is
// uniform, the intermediate rows are read coalesced.
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ tmp, int nrows, int out_w, int out_h,
                                                          const int* __restrict__ bounds, const int* __restrict__ coef, int kv,
                                                          uint8_t* __restrict__ dst, int Hd, int Wd, int px, int py) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= Wd) return;
    const int yy = y - py, xx = x - px;
    uint8_t v = 0;
    if (yy >= 0 && yy < out_h && xx >= 0 && xx < out_w) {
        const int ymin = bounds[2 * yy];
        int yn = bounds[2 * yy + 1];
        if (yn > kv) yn = kv;
        if (ymin < 0 || ymin + yn > nrows) yn = 0;
        const int* k = coef + (int64_t)yy * kv;
        const uint8_t* col = tmp + ((int64_t)b * nrows + ymin) * out_w + xx;
        int acc = 1 << 21;
        for (int j = 0; j < yn; ++j) acc += (int)col[(int64_t)j * out_w] * k[j];
        v = sp_clip8(acc);
    }
    dst[((int64_t)b * Hd + y) * Wd + x] = v;
}

// ------------------------------------------------------------------------------------------------ external contours
// Chain codes of OpenCV: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE (image y grows downwards).
__constant__ int SP_DX[8] = {1, 1, 0, -1, -1, -1, 0, 1};
__constant__ int SP_DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

constexpr int CT_TILE = 1024;        // pixels per compaction workgroup (256 threads x 4)
constexpr int CT_WIN_H = 64, CT_WIN_W = 128;   // LDS window of neighbour bytes per tracing wave (8 KiB)
constexpr int CT_WAVES = 4;

// fg / bg selection (grey > 127, mask2polygon.py:325) and the 8-neighbour byte of every pixel: bit s set when the
// neighbour in chain direction s is foreground (outside the image = background: OpenCV pads with a zero frame).  The
// neighbour bytes use a row pitch P (multiple of 16, columns W..P-1 hold 0) so that the tracer's window loads are whole
// 16-byte chunks.
__global__ __launch_bounds__(256) void ct_select_kernel(const uint8_t* __restrict__ grey, uint8_t* __restrict__ fg,
                                                         uint8_t* __restrict__ bg, uint8_t* __restrict__ nb, int H, int W,
                                                         int P, int64_t np) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= np) return;
    const int x = (int)(q % P);
    const int64_t rowi = q / P;                                  // b * H + y
    const int y = (int)(rowi % H);
    const int64_t img = rowi - y;                                 // b * H
    uint8_t m = 0;
    if (x < W) {
        const int64_t p = rowi * W + x;
        const bool f = grey[p] > 127;
        fg[p] = f;
        bg[p] = !f;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int xx = x + SP_DX[s], yy = y + SP_DY[s];
            if (xx >= 0 && xx < W && yy >= 0 && yy < H && grey[(img + yy) * W + xx] > 127) m |= (uint8_t)(1u << s);
        }
    }
    nb[q] = m;
}

// a contour starts at the root (raster-first pixel) of every 8-connected foreground component whose West neighbour is
// background 4-connected to the frame (x == 0: the frame itself)
__device__ __forceinline__ bool ct_is_start(const int* __restrict__ Lf, const int* __restrict__ rootb, const int* __restrict__ aux,
                                            int64_t p, int x) {
    if (Lf[p] != (int)p) return false;
    if (x == 0) return true;
    const int r = rootb[p - 1];
    return r >= 0 && aux[r] != 0;
}

// per 1024-pixel tile of one image: number of starts (grid: tiles x B)
__global__ __launch_bounds__(256) void ct_tile_count_kernel(const int* __restrict__ Lf, const int* __restrict__ rootb,
                                                             const int* __restrict__ aux, int H, int W, int tiles,
                                                             int* __restrict__ tile_cnt) {
    __shared__ int s_w[4];
    const int b = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    int cnt = 0;
    for (int k = 0; k < 4; ++k) {
        const int64_t lp = (int64_t)blockIdx.x * CT_TILE + threadIdx.x * 4 + k;
        if (lp < HW) cnt += ct_is_start(Lf, rootb, aux, b * HW + lp, (int)(lp % W));
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[(int64_t)b * tiles + blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// exclusive scan of in[0..n) in index order by one workgroup (fixed order: bit-identical every run); n = *n_dev when given.
// total_out (optional) receives the sum.
__global__ __launch_bounds__(1024) void ct_scan_kernel(const int* __restrict__ in, int n_const, const int* __restrict__ n_dev,
                                                        int* __restrict__ out, int* __restrict__ total_out) {
    constexpr int PER = 16;
    __shared__ int s_sum[1024];
    const int n = n_dev ? *n_dev : n_const;
    int carry = 0;
    for (int base = 0; base < n; base += 1024 * PER) {
        const int i0 = base + threadIdx.x * PER;
        int v[PER];
        int run = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            v[k] = (i0 + k < n) ? in[i0 + k] : 0;
            run += v[k];
        }
        s_sum[threadIdx.x] = run;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {                        // Hillis-Steele inclusive scan of the thread sums
            const int t = threadIdx.x >= o ? s_sum[threadIdx.x - o] : 0;
            __syncthreads();
            s_sum[threadIdx.x] += t;
            __syncthreads();
        }
        int acc = carry + s_sum[threadIdx.x] - run;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (i0 + k < n) out[i0 + k] = acc;
            acc += v[k];
        }
        carry += s_sum[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0 && total_out) *total_out = carry;
}

// info = {total contours, total points, error flag, ncont[B], cbase[B + 1]}; cbase = first contour (discovery order) of
// each image, from the tile scan
__global__ void ct_image_base_kernel(const int* __restrict__ tile_off, int tiles, int B, int* __restrict__ info) {
    const int b = threadIdx.x;
    int* ncont = info + 3;
    int* cbase = ncont + B;
    if (b < B) cbase[b] = tile_off[(int64_t)b * tiles];
    __syncthreads();
    if (b < B) ncont[b] = (b + 1 < B ? cbase[b + 1] : info[0]) - cbase[b];
    if (b == 0) { cbase[B] = info[0]; info[1] = 0; info[2] = 0; }
}

// the starts of each tile, in raster order, at their place in the discovery order (image-major, raster within an image)
__global__ __launch_bounds__(256) void ct_compact_kernel(const int* __restrict__ Lf, const int* __restrict__ rootb,
                                                          const int* __restrict__ aux, int H, int W, int tiles,
                                                          const int* __restrict__ tile_off, int* __restrict__ starts) {
    __shared__ int s_w[4];
    const int b = blockIdx.y;
    const int64_t HW = (int64_t)H * W;
    bool f[4];
    int cnt = 0;
    for (int k = 0; k < 4; ++k) {
        const int64_t lp = (int64_t)blockIdx.x * CT_TILE + threadIdx.x * 4 + k;
        f[k] = lp < HW && ct_is_start(Lf, rootb, aux, b * HW + lp, (int)(lp % W));
        cnt += f[k];
    }
    // exclusive prefix of cnt over the workgroup, in thread order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = cnt;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int pos = tile_off[(int64_t)b * tiles + blockIdx.x] + incl - cnt;
    for (int w = 0; w < wave; ++w) pos += s_w[w];
    for (int k = 0; k < 4; ++k)
        if (f[k]) starts[pos++] = (int)(b * HW + (int64_t)blockIdx.x * CT_TILE + threadIdx.x * 4 + k);
}

// One wave per contour, every lane walking the same chain (the state is wave-uniform, the LDS reads broadcast); the
// lanes share the reloads of the window.  EMIT = false: count the points of each contour into npts[out index];
// EMIT = true: write them at poff[out index].  The output order within an image is the reverse of the discovery order
// (cvInsertNodeIntoTree prepends siblings).
template <bool EMIT>
__global__ __launch_bounds__(256) void ct_trace_kernel(const uint8_t* __restrict__ nb, const int* __restrict__ starts,
                                                        int* __restrict__ info, int B, int H, int W, int P,
                                                        int* __restrict__ npts, const int* __restrict__ poff,
                                                        i32x2* __restrict__ pts, int64_t max_pts) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[CT_WAVES][CT_WIN_H * CT_WIN_W];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* win = s_win[wave];
    const int total = info[0];
    const int* cbase = info + 3 + B;
    const int64_t HW = (int64_t)H * W;
    const int64_t max_steps = 4 * HW + 16;                           // a border visits a pixel at most 4 times
    const int nwaves = gridDim.x * CT_WAVES;
    for (int c = blockIdx.x * CT_WAVES + wave; c < total; c += nwaves) {
        const int p0 = starts[c];
        const int b = (int)(p0 / HW);
        const int lp = (int)(p0 - (int64_t)b * HW);
        const int x0 = lp % W, y0 = lp / W;
        const int o = cbase[b] + cbase[b + 1] - 1 - c;               // reverse discovery order within image b
        const uint8_t* nbi = nb + (int64_t)b * H * P;
        int wx0 = 0, wy0 = 0;
        bool loaded = false;
        auto fetch = [&](int x, int y) -> uint32_t {
            if (!loaded || x < wx0 || x >= wx0 + CT_WIN_W || y < wy0 || y >= wy0 + CT_WIN_H) {
                wx0 = ((x - CT_WIN_W / 2) >> 4) << 4;                 // 16-byte aligned column origin (may be < 0)
                wy0 = y - CT_WIN_H / 2;
                __builtin_amdgcn_wave_barrier();
                for (int k = lane; k < CT_WIN_H * (CT_WIN_W / 16); k += 64) {
                    const int r = k / (CT_WIN_W / 16), cx = (k % (CT_WIN_W / 16)) * 16;
                    const int gy = wy0 + r, gx = wx0 + cx;
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (gy >= 0 && gy < H && gx >= 0 && gx < P) v = *reinterpret_cast<const u32x4*>(nbi + (int64_t)gy * P + gx);
                    *reinterpret_cast<u32x4*>(win + r * CT_WIN_W + cx) = v;
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                loaded = true;
            }
            return win[(y - wy0) * CT_WIN_W + (x - wx0)];
        };
        int count = 0;
        int64_t base = 0;
        if (EMIT) base = poff[o];
        auto emit = [&](int x, int y) {
            if (EMIT && lane == 0 && base + count < max_pts) pts[base + count] = i32x2{x, y};
            ++count;
        };
        const uint32_t n0 = fetch(x0, y0);
        // search from code 4 downwards (3, 2, 1, 0, 7, 6, 5) for the first foreground neighbour i1
        int s = 4;
        do { s = (s - 1) & 7; } while (!((n0 >> s) & 1u) && s != 4);
        if (s == 4) {
            emit(x0, y0);                                             // single-pixel contour
        } else {
            const int x1 = x0 + SP_DX[s], y1 = y0 + SP_DY[s];
            int prev_s = s ^ 4;
            int cx = x0, cy = y0;
            int64_t steps = 0;
            for (;;) {
                const uint32_t m = fetch(cx, cy);
                // first foreground neighbour searching s+1, s+2, ... (mod 8)
                const uint32_t rot = ((m | (m << 8)) >> (s + 1)) & 0xffu;
                const int t = __builtin_ctz(rot | 0x100u);            // rot != 0: the previous pixel is a neighbour
                const int sn = (s + 1 + t) & 7;
                if (sn != prev_s) { emit(cx, cy); prev_s = sn; }
                const int nx = cx + SP_DX[sn], ny = cy + SP_DY[sn];
                if (nx == x0 && ny == y0 && cx == x1 && cy == y1) break;
                cx = nx; cy = ny;
                s = (sn + 4) & 7;
                if (++steps > max_steps || rot == 0u) {               // cannot happen for a well-formed neighbour map
                    if (lane == 0) atomicOr(info + 2, 1);
                    break;
                }
            }
        }
        if (!EMIT && lane == 0) npts[o] = count;
        if (EMIT && lane == 0 && count != npts[o]) atomicOr(info + 2, 2);
    }
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int uh_window_u16(const uint16_t* raw, int64_t n, int window_length, int window_width, uint8_t* out,
                             uh_stream stream) {
    UH_REQUIRE(raw && out && n >= 0, "uh_window_u16: bad args");
    UH_REQUIRE(window_width >= 2, "uh_window_u16: window width %d < 2 gives an empty window (0 / 0 in the reference)",
               window_width);
    UH_REQUIRE(uh_aligned16(raw) && (((uintptr_t)out) & 7) == 0, "uh_window_u16: raw must be 16-byte and out 8-byte aligned");
    if (n == 0) return UH_OK;
    const long long half = window_width / 2;
    const long long mn = (long long)window_length - half, mx = (long long)window_length + half;
    hipLaunchKernelGGL(window_u16_kernel, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, (hipStream_t)stream, raw, n, mn, mx,
                       (double)(mx - mn), out);
    UH_CHECK_LAUNCH("uh_window_u16");
    return UH_OK;
}

extern "C" size_t uh_resample_ws_bytes(int B, int nrows, int out_w) {
    return (size_t)(B > 0 ? B : 0) * (size_t)(nrows > 0 ? nrows : 0) * (size_t)(out_w > 0 ? out_w : 0) + 256;
}

extern "C" int uh_resample_lanczos_u8(const uint8_t* src, int B, int Hs, int Ws, int box_x, int box_y, int box_w, int box_h,
                                      const uint8_t* lut, const int* h_bounds, const int* h_coef, int kh, int out_w,
                                      const int* v_bounds, const int* v_coef, int kv, int out_h, int row0, int nrows,
                                      uint8_t* dst, int Hd, int Wd, int px, int py, void* ws, size_t ws_bytes,
                                      uh_stream stream) {
    UH_REQUIRE(src && lut && h_bounds && h_coef && v_bounds && v_coef && dst && ws, "uh_resample_lanczos_u8: null pointer");
    UH_REQUIRE(B > 0 && Hs > 0 && Ws > 0 && Hd > 0 && Wd > 0 && out_w > 0 && out_h > 0 && nrows > 0,
               "uh_resample_lanczos_u8: bad sizes");
    UH_REQUIRE(box_x >= 0 && box_y >= 0 && box_w > 0 && box_h > 0 && box_x + box_w <= Ws && box_y + box_h <= Hs,
               "uh_resample_lanczos_u8: source box (%d,%d,%d,%d) outside the %dx%d source", box_x, box_y, box_w, box_h, Ws, Hs);
    UH_REQUIRE(row0 >= 0 && row0 + nrows <= box_h, "uh_resample_lanczos_u8: rows [%d,%d) outside the box", row0, row0 + nrows);
    UH_REQUIRE(kh >= 1 && kh <= RS_KMAX, "uh_resample_lanczos_u8: horizontal filter of %d taps (1..%d supported)", kh, RS_KMAX);
    UH_REQUIRE(kv >= 1, "uh_resample_lanczos_u8: bad vertical filter size");
    UH_REQUIRE(px >= 0 && py >= 0 && px + out_w <= Wd && py + out_h <= Hd, "uh_resample_lanczos_u8: placement outside the canvas");
    UH_REQUIRE((int64_t)B * Hs * Ws < (1ll << 40) && (int64_t)B * Hd * Wd < (1ll << 40), "uh_resample_lanczos_u8: batch too large");
    UH_REQUIRE(Hd <= 65535, "uh_resample_lanczos_u8: destination height %d > 65535", Hd);
    const size_t need = uh_resample_ws_bytes(B, nrows, out_w);
    if (ws_bytes < need) {
        uh_set_error("uh_resample_lanczos_u8: workspace %zu < %zu bytes", ws_bytes, need);
        return UH_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = (uint8_t*)ws;
    hipLaunchKernelGGL(resample_h_kernel, dim3((out_w + RS_TX - 1) / RS_TX, (nrows + RS_ROWS - 1) / RS_ROWS, B), dim3(256), 0, st,
                       src, Hs, Ws, box_x, box_y, box_w, box_h, lut, h_bounds, h_coef, kh, out_w, row0, nrows, tmp);
    hipLaunchKernelGGL(resample_v_kernel, dim3((Wd + 255) / 256, Hd, B), dim3(256), 0, st, (const uint8_t*)tmp, nrows, out_w, out_h,
                       v_bounds, v_coef, kv, dst, Hd, Wd, px, py);
    UH_CHECK_LAUNCH("uh_resample_lanczos_u8");
    return UH_OK;
}

// ---- contours: workspace layout (every region 256-byte aligned)
namespace {
struct CtLayout {
    size_t Lf, Lb, rootb, aux, fg, bg, nb, tile_cnt, tile_off, starts, poff, total;
    int P, tiles;
    int64_t maxc;
};
inline size_t ct_al(size_t v) { return (v + 255) & ~(size_t)255; }
CtLayout ct_layout(int B, int H, int W) {
    CtLayout l;
    const size_t n = (size_t)B * H * W;
    l.P = (W + 15) & ~15;
    l.tiles = (int)(((int64_t)H * W + CT_TILE - 1) / CT_TILE);
    l.maxc = (int64_t)B * ((H + 1) / 2) * ((W + 1) / 2);
    size_t o = 0;
    l.Lf = o; o += ct_al(n * 4);
    l.Lb = o; o += ct_al(n * 4);
    l.rootb = o; o += ct_al(n * 4);
    l.aux = o; o += ct_al(n * 4);
    l.fg = o; o += ct_al(n);
    l.bg = o; o += ct_al(n);
    l.nb = o; o += ct_al((size_t)B * H * l.P);
    l.tile_cnt = o; o += ct_al((size_t)B * l.tiles * 4);
    l.tile_off = o; o += ct_al((size_t)B * l.tiles * 4);
    l.starts = o; o += ct_al((size_t)l.maxc * 4);
    l.poff = o; o += ct_al((size_t)l.maxc * 4);
    l.total = o;
    return l;
}
int ct_check(const char* who, int B, int H, int W, const void* ws, size_t ws_bytes) {
    UH_REQUIRE(ws && B > 0 && B <= 1024 && H > 0 && W > 0, "%s: bad args (B = 1..1024)", who);
    UH_REQUIRE((int64_t)B * H * ((W + 15) & ~15) < (1ll << 31), "%s: pixel count of %dx%dx%d overflows int32", who, B, H, W);
    UH_REQUIRE(uh_aligned16(ws), "%s: workspace must be 16-byte aligned", who);
    const size_t need = ct_layout(B, H, W).total;
    if (ws_bytes < need) {
        uh_set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, need);
        return UH_EWORKSPACE;
    }
    return UH_OK;
}
constexpr int CT_TRACE_BLOCKS = 1024;
}  // namespace

extern "C" size_t uh_contours_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return ct_layout(B, H, W).total;
}
extern "C" size_t uh_contours_max(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)ct_layout(B, H, W).maxc;
}

extern "C" int uh_contours_count(const uint8_t* grey, int B, int H, int W, void* ws, size_t ws_bytes, int* info, int* npts,
                                 uh_stream stream) {
    const int rc = ct_check("uh_contours_count", B, H, W, ws, ws_bytes);
    if (rc != UH_OK) return rc;
    UH_REQUIRE(grey && info && npts, "uh_contours_count: null pointer");
    const CtLayout l = ct_layout(B, H, W);
    char* w = (char*)ws;
    int* Lf = (int*)(w + l.Lf);
    int* Lb = (int*)(w + l.Lb);
    int* rootb = (int*)(w + l.rootb);
    int* aux = (int*)(w + l.aux);
    uint8_t* fg = (uint8_t*)(w + l.fg);
    uint8_t* bg = (uint8_t*)(w + l.bg);
    uint8_t* nb = (uint8_t*)(w + l.nb);
    int* tile_cnt = (int*)(w + l.tile_cnt);
    int* tile_off = (int*)(w + l.tile_off);
    int* starts = (int*)(w + l.starts);
    int* poff = (int*)(w + l.poff);
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)B * H * W;
    const int64_t np = (int64_t)B * H * l.P;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    hipLaunchKernelGGL(ct_select_kernel, dim3((unsigned)((np + 255) / 256)), blk, 0, st, grey, fg, bg, nb, H, W, l.P, np);
    // 8-connected foreground components (roots = raster-first pixels); aux is scratch here
    hipLaunchKernelGGL(pp_init_kernel, grid, blk, 0, st, (const unsigned char*)fg, Lf, aux, n);
    hipLaunchKernelGGL(pp_union_kernel<true>, grid, blk, 0, st, (const unsigned char*)fg, Lf, H, W, n);
    // 4-connected background components; aux[root] = 1 where one touches the image border (= the frame's background)
    hipLaunchKernelGGL(pp_init_kernel, grid, blk, 0, st, (const unsigned char*)bg, Lb, aux, n);
    hipLaunchKernelGGL(pp_union_kernel<false>, grid, blk, 0, st, (const unsigned char*)bg, Lb, H, W, n);
    hipLaunchKernelGGL(pp_flatten_kernel<0>, grid, blk, 0, st, (const int*)Lb, rootb, aux, H, W, n);
    // starts, compacted in a fixed order
    hipLaunchKernelGGL(ct_tile_count_kernel, dim3(l.tiles, B), blk, 0, st, (const int*)Lf, (const int*)rootb, (const int*)aux, H, W,
                       l.tiles, tile_cnt);
    hipLaunchKernelGGL(ct_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)tile_cnt, B * l.tiles, (const int*)nullptr, tile_off,
                       info);
    hipLaunchKernelGGL(ct_image_base_kernel, dim3(1), dim3(B < 64 ? 64 : ((B + 63) / 64) * 64), 0, st, (const int*)tile_off, l.tiles,
                       B, info);
    hipLaunchKernelGGL(ct_compact_kernel, dim3(l.tiles, B), blk, 0, st, (const int*)Lf, (const int*)rootb, (const int*)aux, H, W,
                       l.tiles, (const int*)tile_off, starts);
    // count pass, then the point offsets in output order
    hipLaunchKernelGGL(ct_trace_kernel<false>, dim3(CT_TRACE_BLOCKS), blk, 0, st, (const uint8_t*)nb, (const int*)starts, info, B, H,
                       W, l.P, npts, (const int*)nullptr, (i32x2*)nullptr, (int64_t)0);
    hipLaunchKernelGGL(ct_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)npts, 0, (const int*)info, poff, info + 1);
    UH_CHECK_LAUNCH("uh_contours_count");
    return UH_OK;
}

extern "C" int uh_contours_emit(void* ws, size_t ws_bytes, int B, int H, int W, int* info, const int* npts, int* points,
                                int64_t max_points, uh_stream stream) {
    const int rc = ct_check("uh_contours_emit", B, H, W, ws, ws_bytes);
    if (rc != UH_OK) return rc;
    UH_REQUIRE(info && npts && (points || max_points == 0) && max_points >= 0, "uh_contours_emit: bad args");
    UH_REQUIRE((((uintptr_t)points) & 7) == 0, "uh_contours_emit: points must be 8-byte aligned");
    const CtLayout l = ct_layout(B, H, W);
    char* w = (char*)ws;
    hipLaunchKernelGGL(ct_trace_kernel<true>, dim3(CT_TRACE_BLOCKS), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)(w + l.nb),
                       (const int*)(w + l.starts), info, B, H, W, l.P, (int*)npts, (const int*)(w + l.poff), (i32x2*)points,
                       max_points);
    UH_CHECK_LAUNCH("uh_contours_emit");
    return UH_OK;
}
