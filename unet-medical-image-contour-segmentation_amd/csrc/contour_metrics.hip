// contour_metrics.hip -- contour-distance metrics of two class maps on the device: Hausdorff distance (HD), its 95th
// percentile (HD95), average symmetric surface distance (ASSD) and IoU (DESIGN.md section 3 "Contour metrics").  The
// reference has no such metric; the definitions are pinned in scipy / numpy terms (tests/contour_metrics_ref.py):
//   border S(M)   pixels of M with one of their four edge neighbours outside M (outside the image counts as outside)
//   D_M[x]        min over q in S(M) of |x - q|^2, an exact integer; 0xFFFFFFFF everywhere when S(M) is empty
//   R             sqrt(D_T[p]) for p in S(P) together with sqrt(D_P[q]) for q in S(T)  (one multiset, medpy's convention)
//   HD = max R, HD95 = numpy.percentile(R, 95) (linear), ASSD = mean R, IoU = |P & T| / |P | T|
// Everything is integer up to the finish kernel; the only atomics are integer atomicAdd / atomicMax, whose result does not
// depend on their order, and the fp64 sums of the finish run in an order fixed by the image alone: a call gives the same
// bits every time, and image i of a batch gives the bits it gives alone.
//   1. cm_border_kernel       both masks in one pass: border masks + |P|, |T|, |P&T|, |P|T|, |S(P)|, |S(T)| per image
//   2. edt_columns_kernel     g2[y][x] = squared distance to the nearest feature of column x (down scan, up scan); thread = x
//   3. edt_rows_kernel        D[y][x] = min_j g2[y][j] + (x - j)^2, the row of g2 staged in LDS, bounded search outwards from
//                             x (|x - j|^2 < best so far); FULL writes the map, otherwise only the pixels of the other border
//                             are evaluated and counted into the per-image histogram over d^2
//   4. cm_finish_kernel       one workgroup per image walks the histogram in ascending d^2 and writes the record
#include "uh_common.h"

namespace {

constexpr unsigned EDT_INF = 0x80000000u;      // "no feature": real values are < 2^31 and INF + (W-1)^2 < 2^32 (H, W <= 32768)
constexpr int EDT_MAX_DIM = 32768;
constexpr int EDT_LDS_W = 4096;                // one row of g2 in LDS: 16 KB
constexpr int CNT_STRIDE = 8;                  // per-image counters: |P| |T| |P&T| |P|T| |S(P)| |S(T)| max d^2, n (gathered)

__device__ __forceinline__ unsigned cm_wave_sum_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ bool cm_is_border(const unsigned char* __restrict__ img, int cls, int x, int y, int H, int W) {
    const long long p = (long long)y * W + x;
    if (img[p] != cls) return false;
    if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return true;
    return img[p - 1] != cls || img[p + 1] != cls || img[p - W] != cls || img[p + W] != cls;
}

__global__ __launch_bounds__(256) void border_kernel(const unsigned char* __restrict__ mask, int cls, unsigned char* __restrict__ out,
                                                     int H, int W) {
    const long long hw = (long long)H * W;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const unsigned char* img = mask + (long long)blockIdx.y * hw;
    out[(long long)blockIdx.y * hw + p] = cm_is_border(img, cls, (int)(p % W), (int)(p / W), H, W);
}

__global__ __launch_bounds__(256) void cm_border_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ truth,
                                                        int cls_pred, int cls_true, unsigned char* __restrict__ bp,
                                                        unsigned char* __restrict__ bt, unsigned* __restrict__ counts, int H, int W) {
    __shared__ unsigned red[4][6];
    const long long hw = (long long)H * W;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long base = (long long)blockIdx.y * hw;
    unsigned c[6] = {0, 0, 0, 0, 0, 0};
    if (p < hw) {
        const int x = (int)(p % W), y = (int)(p / W);
        const bool mp = pred[base + p] == cls_pred, mt = truth[base + p] == cls_true;
        const bool sp = mp && cm_is_border(pred + base, cls_pred, x, y, H, W);
        const bool st = mt && cm_is_border(truth + base, cls_true, x, y, H, W);
        bp[base + p] = sp;
        bt[base + p] = st;
        c[0] = mp; c[1] = mt; c[2] = mp && mt; c[3] = mp || mt; c[4] = sp; c[5] = st;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned s = cm_wave_sum_u32(c[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const unsigned s = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (s) atomicAdd(counts + (long long)blockIdx.y * CNT_STRIDE + threadIdx.x, s);
    }
}

// pass 1: thread = column x of image blockIdx.y; every load and store of a step is one coalesced row segment
__global__ __launch_bounds__(64) void edt_columns_kernel(const unsigned char* __restrict__ feat, unsigned* __restrict__ g2, int H, int W) {
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= W) return;
    const long long base = (long long)blockIdx.y * H * W + x;
    unsigned d = EDT_INF;                                          // distance to the nearest feature above, EDT_INF = none yet
    for (int y = 0; y < H; ++y) {
        const long long p = base + (long long)y * W;
        d = feat[p] ? 0u : (d == EDT_INF ? EDT_INF : d + 1u);
        g2[p] = d;
    }
    d = EDT_INF;
    for (int y = H - 1; y >= 0; --y) {
        const long long p = base + (long long)y * W;
        const unsigned down = g2[p];
        d = down == 0u ? 0u : (d == EDT_INF ? EDT_INF : d + 1u);
        const unsigned m = d < down ? d : down;                    // EDT_INF is the largest value either side can hold
        g2[p] = m == EDT_INF ? EDT_INF : m * m;                    // m <= 32767: the square is below 2^30
    }
}

// min_j row[j] + (x - j)^2 by a search outwards from x: a column at distance r can only win while r^2 < best
template <typename Row>
__device__ __forceinline__ unsigned edt_row_min(const Row row, int x, int W) {
    unsigned best = row[x];
    for (int r = 1; r < W; ++r) {
        const unsigned r2 = (unsigned)r * (unsigned)r;
        if (r2 >= best) break;
        const int a = x - r, b = x + r;
        if (a < 0 && b >= W) break;
        if (a >= 0) { const unsigned v = row[a] + r2; best = v < best ? v : best; }
        if (b < W) { const unsigned v = row[b] + r2; best = v < best ? v : best; }
    }
    return best;
}

// pass 2: one workgroup per row (blockIdx.x = y, blockIdx.y = image).  FULL: out[p] = D (0xFFFFFFFF without a feature).
// Otherwise D is evaluated at the pixels of `sel` only and counted: hist[image][D] += 1, counts[image][6] = max D,
// counts[image][7] += 1.  LDS: the row of g2 is staged (W <= EDT_LDS_W); wider rows are searched in global memory.
// g2 and out may be the same buffer in the LDS form (the row is staged before it is overwritten): no __restrict__ on them.
template <bool FULL, bool LDS>
__global__ __launch_bounds__(256) void edt_rows_kernel(const unsigned* g2, unsigned* out,
                                                       const unsigned char* __restrict__ sel, unsigned* __restrict__ hist,
                                                       unsigned* __restrict__ counts, long long nbins, int H, int W) {
    __shared__ unsigned srow[LDS ? EDT_LDS_W : 1];
    const long long rowbase = ((long long)blockIdx.y * H + blockIdx.x) * W;
    const unsigned* grow = g2 + rowbase;
    if (!FULL) {
        int any = 0;
        for (int x = threadIdx.x; x < W; x += 256) any |= sel[rowbase + x];
        if (!__syncthreads_or(any)) return;                        // no border pixel of the other mask in this row
    }
    if (LDS) {
        for (int x = threadIdx.x; x < W; x += 256) srow[x] = grow[x];
        __syncthreads();
    }
    for (int x = threadIdx.x; x < W; x += 256) {
        if (!FULL && !sel[rowbase + x]) continue;
        const unsigned d = LDS ? edt_row_min((const unsigned*)srow, x, W) : edt_row_min(grow, x, W);
        if (FULL) {
            out[rowbase + x] = d >= EDT_INF ? 0xFFFFFFFFu : d;
        } else if (d < EDT_INF) {                                  // the other mask is empty: the image is undefined, nothing counted
            unsigned* c = counts + (long long)blockIdx.y * CNT_STRIDE;
            atomicAdd(hist + (long long)blockIdx.y * nbins + d, 1u);
            atomicMax(c + 6, d);
            atomicAdd(c + 7, 1u);
        }
    }
}

// One workgroup of 16 waves per image.  Bins 0..max d^2 are cut into 16 contiguous spans, one per wave, in tiles of 64 bins
// (lane = bin: coalesced).  The counts are integers; the fp64 sum of count * sqrt(d^2) is added per lane in ascending tile
// order, then over the lanes and the waves in a fixed tree: the order depends on max d^2, that is on the image, alone.
__global__ __launch_bounds__(1024) void cm_finish_kernel(const unsigned* __restrict__ hist, const unsigned* __restrict__ counts,
                                                         uh_contour_record* __restrict__ rec, long long nbins) {
    __shared__ unsigned wcount[16];
    __shared__ double wsum[16];
    __shared__ unsigned stat[2];
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned* c = counts + (long long)b * CNT_STRIDE;
    const unsigned* h = hist + (long long)b * nbins;
    const unsigned n_pred = c[0], n_true = c[1], maxd2 = c[6], n = c[7];
    const bool both_empty = n_pred == 0 && n_true == 0;
    const bool undefined = !both_empty && (n_pred == 0 || n_true == 0);
    const long long tiles = ((long long)maxd2 + 64) / 64;          // tiles of 64 bins that cover 0..maxd2
    const long long per_wave = (tiles + 15) / 16;
    const long long t0 = wave * per_wave, t1 = (t0 + per_wave < tiles) ? t0 + per_wave : tiles;
    unsigned cnt = 0;
    double sum = 0.0;
    if (!undefined && !both_empty)
        for (long long t = t0; t < t1; ++t) {
            const long long k = t * 64 + lane;
            const unsigned v = k <= (long long)maxd2 ? h[k] : 0u;
            cnt += v;
            if (v) sum = __dadd_rn(sum, __dmul_rn((double)v, sqrt((double)k)));
        }
    cnt = cm_wave_sum_u32(cnt);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum = __dadd_rn(sum, __shfl_xor(sum, o, 64));
    if (lane == 0) { wcount[wave] = cnt; wsum[wave] = sum; }
    if (threadIdx.x < 2) stat[threadIdx.x] = 0;
    __syncthreads();
    // numpy.percentile(R, 95), method "linear": virtual index (n - 1) * q, lower neighbour floor(), weight the rest
    const double q = 95.0 / 100.0;
    double vi = n ? __dmul_rn((double)(n - 1), q) : 0.0;
    unsigned lo = 0, hi = 0;
    double gamma = 0.0;
    if (n > 0) {
        if (vi >= (double)(n - 1)) { lo = hi = n - 1; }
        else { if (vi < 0.0) vi = 0.0; lo = (unsigned)floor(vi); hi = lo + 1; gamma = vi - (double)lo; }
    }
    if (!undefined && !both_empty && n > 0) {
        unsigned before = 0;                                       // values in the spans of the waves before this one
        for (int w = 0; w < wave; ++w) before += wcount[w];
        const unsigned mine = wcount[wave];
        if (mine && lo < before + mine && hi >= before) {          // one of the two order statistics lies in this span
            unsigned run = before;
            for (long long t = t0; t < t1; ++t) {
                const long long k = t * 64 + lane;
                const unsigned v = k <= (long long)maxd2 ? h[k] : 0u;
                unsigned inc = v;                                  // inclusive scan over the 64 bins of the tile
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned up = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += up;
                }
                const unsigned first = run + inc - v;              // rank of this bin's first value
                if (v && lo >= first && lo < first + v) stat[0] = (unsigned)k;
                if (v && hi >= first && hi < first + v) stat[1] = (unsigned)k;
                run += __shfl(inc, 63, 64);
                if (run > hi) break;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int w = 0; w < 16; ++w) total = __dadd_rn(total, wsum[w]);
    uh_contour_record r;
    r.n_pred = n_pred; r.n_true = n_true; r.n_inter = c[2]; r.n_union = c[3];
    r.n_border_pred = c[4]; r.n_border_true = c[5];
    r.n = n; r.max_d2 = maxd2; r.d2_lo = stat[0]; r.d2_hi = stat[1];
    r.undefined = undefined ? 1u : 0u; r.reserved = 0u;
    r.weight = gamma; r.sum_dist = total;
    if (undefined) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        r.hd = nan; r.hd95 = nan; r.assd = nan; r.iou = 0.0;
    } else if (both_empty) {
        r.hd = 0.0; r.hd95 = 0.0; r.assd = 0.0; r.iou = 1.0;
    } else {
        const double a = sqrt((double)stat[0]), bb = sqrt((double)stat[1]);
        const double diff = __dadd_rn(bb, -a);                     // numpy's _lerp: from the nearer end
        r.hd = sqrt((double)maxd2);
        r.hd95 = gamma >= 0.5 ? __dadd_rn(bb, -__dmul_rn(diff, __dadd_rn(1.0, -gamma))) : __dadd_rn(a, __dmul_rn(diff, gamma));
        r.assd = n ? total / (double)n : 0.0;
        r.iou = (double)c[2] / (double)c[3];
    }
    rec[b] = r;
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
size_t hist_bins(int H, int W) { return (size_t)(H - 1) * (H - 1) + (size_t)(W - 1) * (W - 1) + 1; }

bool shape_ok(const char* who, int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) { uh_set_error("%s: B, H and W must be positive (got %d, %d, %d)", who, B, H, W); return false; }
    if (H > EDT_MAX_DIM || W > EDT_MAX_DIM) { uh_set_error("%s: H and W are limited to %d (squared distances are kept in 31 bits)", who, EDT_MAX_DIM); return false; }
    if ((long long)H * W >= (1ll << 31) || (long long)B * H * W >= (1ll << 40)) { uh_set_error("%s: pixel count out of range", who); return false; }
    if (B > 65535) { uh_set_error("%s: at most 65535 images per call", who); return false; }
    return true;
}

void launch_columns(const uint8_t* feat, unsigned* g2, int B, int H, int W, hipStream_t st) {
    hipLaunchKernelGGL(edt_columns_kernel, dim3((W + 63) / 64, B), dim3(64), 0, st, feat, g2, H, W);
}

}  // namespace

static_assert(sizeof(uh_contour_record) == 96, "uh_contour_record is 12 x 4 + 6 x 8 bytes");

extern "C" int uh_mask_border_u8(const uint8_t* mask, int cls, uint8_t* out, int B, int H, int W, uh_stream stream) {
    UH_REQUIRE(mask && out, "uh_mask_border_u8: null pointer");
    if (!shape_ok("uh_mask_border_u8", B, H, W)) return UH_EINVAL;
    UH_REQUIRE(cls >= 0 && cls <= 255, "uh_mask_border_u8: the class value must fit a byte");
    const long long hw = (long long)H * W;
    hipLaunchKernelGGL(border_kernel, dim3((unsigned)((hw + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, mask, cls, out, H, W);
    UH_CHECK_LAUNCH("uh_mask_border_u8");
    return UH_OK;
}

// the column pass writes straight into the output map and the row pass reads its row into LDS before it overwrites it, so
// rows of up to EDT_LDS_W need no workspace; wider rows are searched in global memory and need the column pass kept apart
extern "C" size_t uh_edt_sq_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 256 + (W > EDT_LDS_W ? (size_t)B * H * W * sizeof(unsigned) : 0);
}

extern "C" int uh_edt_sq_u8(const uint8_t* feature_u8, uint32_t* out_u32, int B, int H, int W, void* ws, size_t ws_bytes,
                            uh_stream stream) {
    UH_REQUIRE(feature_u8 && out_u32 && ws, "uh_edt_sq_u8: null pointer");
    if (!shape_ok("uh_edt_sq_u8", B, H, W)) return UH_EINVAL;
    const size_t need = uh_edt_sq_ws_bytes(B, H, W);
    if (ws_bytes < need) {
        uh_set_error("uh_edt_sq_u8: workspace %zu < %zu bytes", ws_bytes, need);
        return UH_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const bool lds = W <= EDT_LDS_W;
    unsigned* g2 = lds ? out_u32 : (unsigned*)ws;
    launch_columns(feature_u8, g2, B, H, W, st);
    if (lds)
        hipLaunchKernelGGL((edt_rows_kernel<true, true>), dim3(H, B), dim3(256), 0, st, (const unsigned*)g2, out_u32,
                           (const unsigned char*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, 0ll, H, W);
    else
        hipLaunchKernelGGL((edt_rows_kernel<true, false>), dim3(H, B), dim3(256), 0, st, (const unsigned*)g2, out_u32,
                           (const unsigned char*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, 0ll, H, W);
    UH_CHECK_LAUNCH("uh_edt_sq_u8");
    return UH_OK;
}

// workspace: [counters B x 8 u32][histograms B x ((H-1)^2 + (W-1)^2 + 1) u32][g2 B*H*W u32][border P][border T]
extern "C" size_t uh_contour_metrics_ws_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t n = (size_t)B * H * W;
    return align16((size_t)B * CNT_STRIDE * sizeof(unsigned)) + align16((size_t)B * hist_bins(H, W) * sizeof(unsigned)) +
           align16(n * sizeof(unsigned)) + 2 * align16(n) + 256;
}

extern "C" int uh_contour_metrics(const uint8_t* pred_u8, const uint8_t* true_u8, int cls_pred, int cls_true,
                                  uh_contour_record* records_out, int B, int H, int W, void* ws, size_t ws_bytes, uh_stream stream) {
    UH_REQUIRE(pred_u8 && true_u8 && records_out && ws, "uh_contour_metrics: null pointer");
    if (!shape_ok("uh_contour_metrics", B, H, W)) return UH_EINVAL;
    UH_REQUIRE(cls_pred >= 0 && cls_pred <= 255 && cls_true >= 0 && cls_true <= 255, "uh_contour_metrics: the class values must fit a byte");
    UH_REQUIRE(uh_aligned16(ws), "uh_contour_metrics: the workspace must be 16-byte aligned");
    const size_t need = uh_contour_metrics_ws_bytes(B, H, W);
    if (ws_bytes < need) {
        uh_set_error("uh_contour_metrics: workspace %zu < %zu bytes", ws_bytes, need);
        return UH_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)B * H * W;
    const long long nbins = (long long)hist_bins(H, W);
    const size_t cnt_bytes = align16((size_t)B * CNT_STRIDE * sizeof(unsigned));
    const size_t hist_bytes = align16((size_t)B * nbins * sizeof(unsigned));
    char* base = (char*)ws;
    unsigned* counts = (unsigned*)base;
    unsigned* hist = (unsigned*)(base + cnt_bytes);
    unsigned* g2 = (unsigned*)(base + cnt_bytes + hist_bytes);
    unsigned char* bp = (unsigned char*)g2 + align16(n * sizeof(unsigned));
    unsigned char* bt = bp + align16(n);
    if (hipMemsetAsync(base, 0, cnt_bytes + hist_bytes, st) != hipSuccess) {
        uh_set_error("uh_contour_metrics: clearing the histograms failed");
        return UH_ELAUNCH;
    }
    const long long hw = (long long)H * W;
    hipLaunchKernelGGL(cm_border_kernel, dim3((unsigned)((hw + 255) / 256), B), dim3(256), 0, st, pred_u8, true_u8, cls_pred, cls_true,
                       bp, bt, counts, H, W);
    const bool lds = W <= EDT_LDS_W;
    for (int dir = 0; dir < 2; ++dir) {                            // D_T at S(P), then D_P at S(T): one multiset
        const unsigned char* feat = dir == 0 ? bt : bp;
        const unsigned char* sel = dir == 0 ? bp : bt;
        launch_columns(feat, g2, B, H, W, st);
        if (lds)
            hipLaunchKernelGGL((edt_rows_kernel<false, true>), dim3(H, B), dim3(256), 0, st, (const unsigned*)g2, (unsigned*)nullptr,
                               sel, hist, counts, nbins, H, W);
        else
            hipLaunchKernelGGL((edt_rows_kernel<false, false>), dim3(H, B), dim3(256), 0, st, (const unsigned*)g2, (unsigned*)nullptr,
                               sel, hist, counts, nbins, H, W);
    }
    hipLaunchKernelGGL(cm_finish_kernel, dim3(B), dim3(1024), 0, st, (const unsigned*)hist, (const unsigned*)counts, records_out, nbins);
    UH_CHECK_LAUNCH("uh_contour_metrics");
    return UH_OK;
}
