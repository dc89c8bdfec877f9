// augment.hip -- seeded training augmentation of a prepared batch (DESIGN.md section 3 "Training augmentation"): one launch
// takes the NHWC fp32 / bf16 image and the int64 labels that uh_batch_prepare wrote and produces a new pair, per item
//   geometry    an inverse affine map (flip, rotation, isotropic scale, translation about the image centre, composed on the host)
//               from an output pixel centre to a source position, evaluated in INTEGER arithmetic: six int64 Q32 numbers per
//               item, source coordinate rounded to Q16, bilinear image / nearest labels from that one coordinate;
//   photometry  gamma -> contrast about 0.5 -> brightness -> additive Gaussian noise -> clamp to [0, 1], image only, each stage
//               SKIPPED when its parameter is neutral (the identity configuration returns the input bits);
//   noise       Philox4x32-10 written out below, keyed per item, counter from the element index: no state, no launch order.
// uh_batch_augment_elastic is the same stage with a smooth displacement field added to the source position (a cubic
// B-spline over a coarse control grid, integer too: see batch_augment_elastic_kernel); both kernels share everything else.
// The reference has no such stage (its augmentation is the x4 quarter turns of data_loading.py:100-121, csrc/data_prep.hip).
//
// Coordinates.  Pixel (x, y) covers [x, x+1) x [y, y+1); its centre is (x + 0.5, y + 0.5).  With the row m = (m00 m01 m02 /
// m10 m11 m12) in Q32 (value * 2^32, rounded to nearest on the host)
//     S_x = m00 (2x + 1) + m01 (2y + 1) + 2 m02          (Q33: the source CENTRE coordinate, exact in int64)
//     q_x = (S_x + 2^16) >> 17                            (Q16, round half up, arithmetic shift)
//   labels:  column floor(q_x / 2^16) = q_x >> 16                                   (the pixel that contains the position)
//   image:   u = q_x - 2^15 (the position in index space), x0 = u >> 16, weight wx = (u & 0xFFFF) * 2^-16 (exact in fp32)
// and the same for y.  Every step is integer, so a numpy restatement (tests/augment_ref.py) produces the same bits.
//
// Interpolation, in fp32, in THIS order, no fused multiply-add (fp contraction is off for the whole file):
//     top = p00 + wx * (p01 - p00)        bot = p10 + wx * (p11 - p10)        v = top + wy * (bot - top)
// with a zero weight taking the pixel itself (wx == 0: top = p00, bot = p10; wy == 0: v = top), so integer maps (identity,
// flips) copy bits.  bf16 is widened, computed in fp32 and rounded to nearest-even once, at the store.
// Border.  UH_AUG_CLAMP: neighbour indices (image) and the label index are clamped to the image.  UH_AUG_FILL: a neighbour
// outside the image is `fill_image`, a label outside is `fill_label`.
//
// Traffic: 4C + 8 bytes read and written per pixel at fp32, a gather with the locality of a small rotation.  Reads go
// straight through L1 / L2 (a 64 x 16 output tile touches a source box a few rows taller); staging the box in LDS was not
// needed: DESIGN.md records the measured rate.
#include "uh_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_TW = 64, AUG_TH = 16;          // output tile of a 256-thread workgroup: 64 columns x 4 rows, 4 times

// ---- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
struct philox4 { uint32_t v[4]; };

__device__ __forceinline__ philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    philox4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}

// normal number `j` (0..3) of a Philox block: words (0, 1) and (2, 3) are two Box-Muller pairs, radius from
// u = (r + 0.5) 2^-32 in (0, 1], angle from v = r 2^-32; j even takes the cosine, j odd the sine
__device__ __forceinline__ float aug_normal(const philox4& p, int j) {
    const uint32_t ra = p.v[j & 2], rb = p.v[(j & 2) + 1];
    const float u = ((float)ra + 0.5f) * 2.3283064365386963e-10f;
    const float v = (float)rb * 2.3283064365386963e-10f;
    const float rad = sqrtf(-2.0f * logf(u));
    const float ang = 6.283185307179586f * v;
    return rad * ((j & 1) ? sinf(ang) : cosf(ang));
}

// Q16 source coordinate of one axis: (a (2x+1) + b (2y+1) + 2c + 2^16) >> 17, in wrapping 64-bit arithmetic
__device__ __forceinline__ int64_t aug_q16(int64_t a, int64_t row_term, int x) {
    const uint64_t s = (uint64_t)row_term + (uint64_t)a * (uint64_t)(int64_t)(2 * x + 1);
    return (int64_t)(s + 65536ull) >> 17;
}

__device__ __forceinline__ int aug_clampi(int64_t v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

// what a workgroup knows about its item: the parameter row, the item's planes and which photometric stages run
template <typename T>
struct aug_item {
    uh_augment_params P;
    const T* ib;
    const int64_t* lb;
    bool do_gamma, do_contrast, do_bright, do_noise, photometric;

    __device__ __forceinline__ aug_item(const uh_augment_params* params, const T* in, int ld_in, const int64_t* lab_in, int b, int H,
                                        int W)
        : P(params[b]),                                          // one row per workgroup: uniform loads
          ib(in ? in + (int64_t)b * H * W * ld_in : nullptr),
          lb(lab_in ? lab_in + (int64_t)b * H * W : nullptr) {
        do_gamma = P.gamma != 1.0f, do_contrast = P.contrast != 1.0f, do_bright = P.brightness != 0.0f;
        do_noise = P.noise_std != 0.0f;
        photometric = do_gamma || do_contrast || do_bright || do_noise;
    }

    // Q16 source position of the affine walk at output pixel (x, y)
    __device__ __forceinline__ void affine_q16(int x, int y, int64_t& qx, int64_t& qy) const {
        const uint64_t ty = (uint64_t)(int64_t)(2 * y + 1);
        const int64_t rowx = (int64_t)((uint64_t)P.m[1] * ty + 2ull * (uint64_t)P.m[2]);
        const int64_t rowy = (int64_t)((uint64_t)P.m[4] * ty + 2ull * (uint64_t)P.m[5]);
        qx = aug_q16(P.m[0], rowx, x), qy = aug_q16(P.m[3], rowy, x);
    }
};

// output pixel (x, y) of item b from the Q16 source position (qx, qy): nearest label, bilinear image, photometry, noise
template <typename T, int C>
__device__ __forceinline__ void aug_pixel(const aug_item<T>& it, int64_t qx, int64_t qy, int b, int x, int y, int ld_in,
                                          T* __restrict__ out, int ld_out, int64_t* __restrict__ lab_out, int H, int W,
                                          int fill_mode, float fill_image, int64_t fill_label) {
    const uh_augment_params& P = it.P;
    const int64_t opix = ((int64_t)b * H + y) * W + x;
    if (it.lb) {
        const int64_t lx = qx >> 16, ly = qy >> 16;
        const bool inside = lx >= 0 && lx < W && ly >= 0 && ly < H;
        const int cx = aug_clampi(lx, 0, W - 1), cy = aug_clampi(ly, 0, H - 1);
        const int64_t v = it.lb[(int64_t)cy * W + cx];             // the clamped index is always readable
        lab_out[opix] = (fill_mode && !inside) ? fill_label : v;
    }
    if (!it.ib) return;
    const int64_t ux = qx - 32768, uy = qy - 32768;
    const int64_t ix0 = ux >> 16, iy0 = uy >> 16;
    const int fx = (int)(ux & 0xFFFF), fy = (int)(uy & 0xFFFF);
    const float wx = (float)fx * 1.52587890625e-05f, wy = (float)fy * 1.52587890625e-05f;
    // neighbour indices, clamped so that every address is inside the image whatever the tables hold
    const int x0 = aug_clampi(ix0, 0, W - 1), x1 = aug_clampi(ix0 + 1, 0, W - 1);
    const int y0 = aug_clampi(iy0, 0, H - 1), y1 = aug_clampi(iy0 + 1, 0, H - 1);
    const bool vx0 = ix0 >= 0 && ix0 < W, vx1 = ix0 + 1 >= 0 && ix0 + 1 < W;
    const bool vy0 = iy0 >= 0 && iy0 < H, vy1 = iy0 + 1 >= 0 && iy0 + 1 < H;
    const T* r0 = it.ib + (int64_t)y0 * W * ld_in;
    const T* r1 = it.ib + (int64_t)y1 * W * ld_in;
    philox4 blk;
    uint32_t blk_id = 0xFFFFFFFFu;                                 // e >> 2 < 2^30 for every accepted size
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float p00 = uh_to_f32(r0[(int64_t)x0 * ld_in + c]), p01 = uh_to_f32(r0[(int64_t)x1 * ld_in + c]);
        float p10 = uh_to_f32(r1[(int64_t)x0 * ld_in + c]), p11 = uh_to_f32(r1[(int64_t)x1 * ld_in + c]);
        if (fill_mode) {
            p00 = (vx0 && vy0) ? p00 : fill_image;
            p01 = (vx1 && vy0) ? p01 : fill_image;
            p10 = (vx0 && vy1) ? p10 : fill_image;
            p11 = (vx1 && vy1) ? p11 : fill_image;
        }
        const float top = fx ? p00 + wx * (p01 - p00) : p00;
        const float bot = fx ? p10 + wx * (p11 - p10) : p10;
        float v = fy ? top + wy * (bot - top) : top;
        if (it.photometric) {
            if (it.do_gamma) v = powf(fminf(fmaxf(v, 0.0f), 1.0f), P.gamma);
            if (it.do_contrast) v = (v - 0.5f) * P.contrast + 0.5f;
            if (it.do_bright) v = v + P.brightness;
            if (it.do_noise) {
                const uint32_t e = (uint32_t)(((int64_t)y * W + x) * C + c);
                if ((e >> 2) != blk_id) {
                    blk_id = e >> 2;
                    blk = philox4x32_10(blk_id, 0u, 0u, 1u, P.key[0], P.key[1]);
                }
                v = v + P.noise_std * aug_normal(blk, (int)(e & 3u));
            }
            v = fminf(fmaxf(v, 0.0f), 1.0f);
        }
        out[opix * ld_out + c] = uh_from_f32<T>(v);
    }
}

template <typename T, int C>
__global__ __launch_bounds__(256) void batch_augment_kernel(const T* __restrict__ in, int ld_in, const int64_t* __restrict__ lab_in,
                                                             const uh_augment_params* __restrict__ params, T* __restrict__ out,
                                                             int ld_out, int64_t* __restrict__ lab_out, int H, int W, int tilesX,
                                                             int fill_mode, float fill_image, int64_t fill_label) {
    const int b = blockIdx.y;
    const aug_item<T> it(params, in, ld_in, lab_in, b, H, W);
    const int X0 = (blockIdx.x % tilesX) * AUG_TW, Y0 = (blockIdx.x / tilesX) * AUG_TH;
    const int x = X0 + (threadIdx.x & 63);
    if (x >= W) return;
#pragma unroll
    for (int k = 0; k < AUG_TH / 4; ++k) {
        const int y = Y0 + (threadIdx.x >> 6) + 4 * k;
        if (y >= H) break;
        int64_t qx, qy;
        it.affine_q16(x, y, qx, qy);
        aug_pixel<T, C>(it, qx, qy, b, x, y, ld_in, out, ld_out, lab_out, H, W, fill_mode, fill_image, fill_label);
    }
}

// ---- elastic deformation (DESIGN.md section 3 "Elastic deformation"): a cubic B-spline displacement field over a control
// grid of spacing `egrid` pixels, added to the affine walk's Q16 position at the OUTPUT pixel.  control [B][GH][GW][2] holds
// (dx, dy) in Q16 pixels, control point k of an axis at (k - 1) egrid; weights [egrid][4] holds the basis at (n + 0.5) / egrid
// in Q20, every row summing to 2^20.  With cx = x / egrid, nx = x % egrid (and cy, ny):
//     r_k  = (sum_j w[nx][j] d[cy + k][cx + j] + 2^19) >> 20          k = 0..3, per component, int64, arithmetic shift
//     disp = (sum_k w[ny][k] r_k + 2^19) >> 20
// egrid is a multiple of 16 = AUG_TH and tiles start at multiples of 16 rows, so cy is ONE value for the workgroup, and the
// 64 columns of the tile touch at most 64 / 16 + 3 = 7 control columns: the workgroup stages that 4 x 7 x 2 patch in LDS
// once (56 loads), clamped to |d| < 2^22.  r_k depends on the column only, and a lane keeps its column over its 4 rows: it
// forms its eight r_k once (32 multiply-adds, its weight row one 16-byte load) and spends 8 multiply-adds per pixel on
// the column pass, whose weight row w[ny] is the same for the whole wave.  Weights are clamped to [0, 2^20] on load, so
// |r_k| <= 2^24 fits an int and no sum passes 2^46 whatever the tables hold; the sampler clamps every index it forms.
constexpr int AUG_PATCH_W = AUG_TW / 16 + 3;
constexpr int AUG_DMAX = (1 << 22) - 1;

__device__ __forceinline__ int aug_clamp32(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename T, int C>
__global__ __launch_bounds__(256) void batch_augment_elastic_kernel(const T* __restrict__ in, int ld_in,
                                                                     const int64_t* __restrict__ lab_in,
                                                                     const uh_augment_params* __restrict__ params,
                                                                     const int32_t* __restrict__ control,
                                                                     const int32_t* __restrict__ weights, int egrid, int GH, int GW,
                                                                     T* __restrict__ out, int ld_out, int64_t* __restrict__ lab_out,
                                                                     int H, int W, int tilesX, int fill_mode, float fill_image,
                                                                     int64_t fill_label) {
    __shared__ int32_t patch[4][AUG_PATCH_W][2];
    const int b = blockIdx.y;
    const aug_item<T> it(params, in, ld_in, lab_in, b, H, W);
    const int X0 = (blockIdx.x % tilesX) * AUG_TW, Y0 = (blockIdx.x / tilesX) * AUG_TH;
    const int cx0 = X0 / egrid, cy = Y0 / egrid;
    if (threadIdx.x < 4 * AUG_PATCH_W * 2) {
        const int k = threadIdx.x / (AUG_PATCH_W * 2), j = (threadIdx.x % (AUG_PATCH_W * 2)) >> 1, c = threadIdx.x & 1;
        int v = 0;                                                 // past the table (columns right of the image): unused
        if (cy + k < GH && cx0 + j < GW) v = control[(((int64_t)b * GH + cy + k) * GW + cx0 + j) * 2 + c];
        patch[k][j][c] = aug_clamp32(v, -AUG_DMAX, AUG_DMAX);
    }
    __syncthreads();
    const int x = X0 + (threadIdx.x & 63);
    if (x >= W) return;
    const int cxl = x / egrid - cx0, nx = x - (x / egrid) * egrid;   // cxl <= 3: the tile is 64 wide, a cell at least 16
    int rx[4], ry[4];
    {
        const int4 wq = *reinterpret_cast<const int4*>(weights + 4 * nx);
        const int w[4] = {aug_clamp32(wq.x, 0, 1 << 20), aug_clamp32(wq.y, 0, 1 << 20), aug_clamp32(wq.z, 0, 1 << 20),
                          aug_clamp32(wq.w, 0, 1 << 20)};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int64_t sx = 1 << 19, sy = 1 << 19;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sx += (int64_t)w[j] * patch[k][cxl + j][0];
                sy += (int64_t)w[j] * patch[k][cxl + j][1];
            }
            rx[k] = (int)(sx >> 20), ry[k] = (int)(sy >> 20);
        }
    }
#pragma unroll
    for (int k = 0; k < AUG_TH / 4; ++k) {
        const int y = Y0 + (threadIdx.x >> 6) + 4 * k;
        if (y >= H) break;
        const int ny = __builtin_amdgcn_readfirstlane(y - cy * egrid);   // one row per wave: a uniform load of w[ny]
        int64_t dx = 1 << 19, dy = 1 << 19;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int w = aug_clamp32(weights[4 * ny + j], 0, 1 << 20);
            dx += (int64_t)w * rx[j];
            dy += (int64_t)w * ry[j];
        }
        int64_t qx, qy;
        it.affine_q16(x, y, qx, qy);
        aug_pixel<T, C>(it, qx + (dx >> 20), qy + (dy >> 20), b, x, y, ld_in, out, ld_out, lab_out, H, W, fill_mode, fill_image,
                        fill_label);
    }
}

// the launch of `kernel<T, C>` for the runtime channel count
#define AUG_LAUNCH(kernel, ...)                                                                                       \
    switch (C) {                                                                                                      \
        case 1: hipLaunchKernelGGL((kernel<T, 1>), grid, dim3(256), 0, st, __VA_ARGS__); break;                        \
        case 2: hipLaunchKernelGGL((kernel<T, 2>), grid, dim3(256), 0, st, __VA_ARGS__); break;                        \
        case 3: hipLaunchKernelGGL((kernel<T, 3>), grid, dim3(256), 0, st, __VA_ARGS__); break;                        \
        default: hipLaunchKernelGGL((kernel<T, 4>), grid, dim3(256), 0, st, __VA_ARGS__); break;                       \
    }

struct aug_elastic { const int32_t* control; const int32_t* weights; int egrid, GH, GW; };

template <typename T>
void launch_augment(int C, dim3 grid, hipStream_t st, const T* in, int ld_in, const int64_t* lab_in, const uh_augment_params* params,
                    const aug_elastic* el, T* out, int ld_out, int64_t* lab_out, int H, int W, int tilesX, int fill_mode,
                    float fill_image, int64_t fill_label) {
    if (el) {
        AUG_LAUNCH(batch_augment_elastic_kernel, in, ld_in, lab_in, params, el->control, el->weights, el->egrid, el->GH, el->GW, out,
                   ld_out, lab_out, H, W, tilesX, fill_mode, fill_image, fill_label)
    } else {
        AUG_LAUNCH(batch_augment_kernel, in, ld_in, lab_in, params, out, ld_out, lab_out, H, W, tilesX, fill_mode, fill_image,
                   fill_label)
    }
}

// the checks and the launch that both entry points share; `name` is the entry point, for the messages
int augment_entry(const char* name, const void* image_in, int ld_in, const int64_t* labels_in, const uh_augment_params* params,
                  const aug_elastic* el, void* image_out, int ld_out, int64_t* labels_out, int B, int H, int W, int C, int dt,
                  int border, float fill_image, int fill_label, uh_stream stream) {
    UH_REQUIRE(image_in || labels_in, "%s: neither an image nor a label batch", name);
    UH_REQUIRE(params, "%s: null parameter table", name);
    UH_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0 && H <= 16384 && W <= 16384, "%s: bad sizes B=%d H=%d W=%d", name, B, H, W);
    UH_REQUIRE(!image_in || (C >= 1 && C <= 4 && image_out && ld_in >= C && ld_out >= C && image_out != image_in),
               "%s: image batch needs 1..4 channels, strides >= C and an output that is not the input", name);
    UH_REQUIRE(!labels_in || (labels_out && labels_out != labels_in), "%s: label batch needs an output that is not the input", name);
    UH_REQUIRE(dt == UH_F32 || dt == UH_BF16, "%s: bad dtype %d", name, dt);
    UH_REQUIRE(border == UH_AUG_CLAMP || border == UH_AUG_FILL, "%s: bad border mode %d", name, border);
    UH_REQUIRE((int64_t)H * W * (image_in ? C : 1) < (1ll << 32), "%s: item too large for the noise counter", name);
    hipStream_t st = (hipStream_t)stream;
    const int tilesX = (W + AUG_TW - 1) / AUG_TW, tilesY = (H + AUG_TH - 1) / AUG_TH;
    dim3 grid(tilesX * tilesY, B);
    const int Ck = image_in ? C : 1;
    if (dt == UH_BF16)
        launch_augment<bf16_t>(Ck, grid, st, (const bf16_t*)image_in, ld_in, labels_in, params, el, (bf16_t*)image_out, ld_out,
                               labels_out, H, W, tilesX, border == UH_AUG_FILL, fill_image, (int64_t)fill_label);
    else
        launch_augment<float>(Ck, grid, st, (const float*)image_in, ld_in, labels_in, params, el, (float*)image_out, ld_out,
                              labels_out, H, W, tilesX, border == UH_AUG_FILL, fill_image, (int64_t)fill_label);
    UH_CHECK_LAUNCH(el ? "batch_augment_elastic_kernel" : "batch_augment_kernel");
    return UH_OK;
}

}  // namespace

extern "C" int uh_batch_augment(const void* image_in, int ld_in, const int64_t* labels_in, const uh_augment_params* params,
                                void* image_out, int ld_out, int64_t* labels_out, int B, int H, int W, int C, int dt, int border,
                                float fill_image, int fill_label, uh_stream stream) {
    return augment_entry("uh_batch_augment", image_in, ld_in, labels_in, params, nullptr, image_out, ld_out, labels_out, B, H, W, C,
                         dt, border, fill_image, fill_label, stream);
}

extern "C" int uh_batch_augment_elastic(const void* image_in, int ld_in, const int64_t* labels_in, const uh_augment_params* params,
                                        const int32_t* control, const int32_t* weights, int grid, void* image_out, int ld_out,
                                        int64_t* labels_out, int B, int H, int W, int C, int dt, int border, float fill_image,
                                        int fill_label, uh_stream stream) {
    UH_REQUIRE(control && weights && uh_aligned16(weights), "uh_batch_augment_elastic: null control table or weights not 16-byte aligned");
    UH_REQUIRE(grid >= 16 && grid <= 256 && grid % 16 == 0, "uh_batch_augment_elastic: grid %d is not a multiple of 16 in [16, 256]", grid);
    UH_REQUIRE(H > 0 && W > 0, "uh_batch_augment_elastic: bad sizes H=%d W=%d", H, W);
    const aug_elastic el = {control, weights, grid, (H + grid - 1) / grid + 3, (W + grid - 1) / grid + 3};
    return augment_entry("uh_batch_augment_elastic", image_in, ld_in, labels_in, params, &el, image_out, ld_out, labels_out, B, H, W,
                         C, dt, border, fill_image, fill_label, stream);
}
