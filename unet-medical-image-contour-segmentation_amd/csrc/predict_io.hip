// predict_io.hip -- the byte stages around the eval forward of predict.py and of evaluate.py's PNG dumps: a folder of decoded
// 8-bit grey images goes in, grey-coded class maps come out (/root/reference/predict.py, evaluate.py, utils/data_loading.py):
//   data_loading.py:86-87 + predict.py:19-20   `if (img > 1).any(): img = img / 255.0`, then .to(float32)  -> uh_predict_prepare_u8
//   predict.py:27 / evaluate.py:111            mask_pred.argmax(dim=1), kept as one byte per pixel         -> uh_logits_to_classes_u8
//   predict.py:52-58, evaluate.py:96-105,150-163  class index -> display grey through a 256-entry table    -> uh_classes_to_grey_u8
// Plain streaming kernels: a thread moves 16 bytes of the narrow side per access, the grid covers the data once, tails and
// unaligned pointers take a scalar path.  Nothing here synchronises with the host or allocates.
#include "uh_common.h"

namespace {

// flags[b] = 1 when image b holds a byte > 1.  The images of a batch lie back to back and H*W may be odd, so image b may
// start at any byte: a thread's 16-byte chunk is tested as four words when it is aligned and whole, byte by byte otherwise.
__global__ __launch_bounds__(256) void pio_any_gt1_kernel(const uint8_t* __restrict__ img, int64_t per_image,
                                                           int* __restrict__ flags) {
    const int b = blockIdx.y;
    const uint8_t* p = img + (int64_t)b * per_image;
    const int lead = (int)((16 - ((uintptr_t)p & 15)) & 15);          // bytes before the first aligned chunk of this image
    bool any = false;
    // chunk 0 = the unaligned head [0, lead), chunk c >= 1 = [lead + 16 (c - 1), lead + 16 c)
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;; c += (int64_t)gridDim.x * 256) {
        const int64_t lo = c == 0 ? 0 : lead + 16 * (c - 1);
        if (lo >= per_image) break;
        const int64_t hi = c == 0 ? (lead < per_image ? lead : per_image) : (lo + 16 < per_image ? lo + 16 : per_image);
        if (c != 0 && hi - lo == 16) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(p + lo);
            any |= ((v[0] | v[1] | v[2] | v[3]) & 0xFEFEFEFEu) != 0u;
        } else {
            for (int64_t k = lo; k < hi; ++k) any |= p[k] > 1;
        }
    }
    if (__any(any) && (threadIdx.x & 63) == 0) flags[b] = 1;          // every writer stores the same value
}

// uint8 [B][H][W] -> float32 [B][1][H][W] over the flat batch: 16 pixels per thread (one 16-byte load, four 16-byte stores).
// The 256 quotients are built once per workgroup with the correctly rounded division numpy performs.
__global__ __launch_bounds__(256) void pio_prepare_kernel(const uint8_t* __restrict__ img, const int* __restrict__ flags,
                                                           float* __restrict__ out, int64_t per_image, int64_t n, int vec) {
    __shared__ float s_div[256];
    s_div[threadIdx.x] = __fdiv_rn((float)threadIdx.x, 255.0f);
    __syncthreads();
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i >= n) return;
    const int64_t b0 = i / per_image;
    if (vec && i + 16 <= n && i + 16 <= (b0 + 1) * per_image) {        // the chunk lies inside one image
        const bool div = flags[b0] != 0;
        const u32x4 v = *reinterpret_cast<const u32x4*>(img + i);
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned u = (v[w] >> (8 * k)) & 0xFFu;
                o[k] = div ? s_div[u] : (float)u;
            }
            *reinterpret_cast<f32x4*>(out + i + 4 * w) = o;
        }
    } else {
        for (int64_t k = i; k < n && k < i + 16; ++k) {
            const unsigned u = img[k];
            out[k] = flags[k / per_image] != 0 ? s_div[u] : (float)u;
        }
    }
}

// index of the FIRST maximum, a NaN counting as the maximum (torch.argmax; the rule of argmax_classes_kernel in infer.hip)
template <int C> __device__ __forceinline__ unsigned pio_argmax(const float* l) {
    float best = l[0];
    unsigned idx = 0;
#pragma unroll
    for (int c = 1; c < C; ++c) {
        const float v = l[c];
        const bool take = (v > best) || (v != v && best == best);
        if (take) { best = v; idx = c; }
    }
    return idx;
}

// logits T [npix][C] -> uint8 [npix].  A thread takes PIX = 16 / sizeof(T) pixels: C 16-byte loads (its 16 C bytes are
// contiguous), one PIX-byte store.  The last, partial group is done pixel by pixel.
template <typename T, int C>
__global__ __launch_bounds__(256) void pio_classes_kernel(const T* __restrict__ logits, int64_t npix, uint8_t* __restrict__ out) {
    constexpr int PIX = uh_vec16<T>::N;
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PIX;
    if (p0 >= npix) return;
    if (p0 + PIX <= npix) {
        float l[PIX * C];
        const uh_vec16<T>* src = reinterpret_cast<const uh_vec16<T>*>(logits + p0 * C);
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const uh_vec16<T> v = src[j];
#pragma unroll
            for (int k = 0; k < PIX; ++k) l[j * PIX + k] = v.get(k);
        }
        unsigned w[PIX / 4];
#pragma unroll
        for (int q = 0; q < PIX / 4; ++q) {
            w[q] = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) w[q] |= pio_argmax<C>(l + (4 * q + k) * C) << (8 * k);
        }
        if (PIX == 4) {
            *reinterpret_cast<unsigned*>(out + p0) = w[0];
        } else {
            u32x2 o;
            o[0] = w[0];
            o[1] = w[PIX / 4 - 1];
            *reinterpret_cast<u32x2*>(out + p0) = o;
        }
    } else {
        for (int64_t p = p0; p < npix; ++p) {
            float l[C];
#pragma unroll
            for (int c = 0; c < C; ++c) l[c] = uh_to_f32(logits[p * C + c]);
            out[p] = (uint8_t)pio_argmax<C>(l);
        }
    }
}

// any class count, any alignment: one pixel per thread
template <typename T>
__global__ __launch_bounds__(256) void pio_classes_generic_kernel(const T* __restrict__ logits, int ncls, int64_t npix,
                                                                   uint8_t* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const T* l = logits + p * ncls;
    float best = uh_to_f32(l[0]);
    int idx = 0;
    for (int c = 1; c < ncls; ++c) {
        const float v = uh_to_f32(l[c]);
        const bool take = (v > best) || (v != v && best == best);
        if (take) { best = v; idx = c; }
    }
    out[p] = (uint8_t)idx;
}

template <typename T>
void pio_launch_classes(const T* logits, int64_t npix, int ncls, uint8_t* out, hipStream_t st) {
    constexpr int PIX = uh_vec16<T>::N;
    const bool vec = ncls >= 2 && ncls <= 4 && uh_aligned16(logits) && (((uintptr_t)out) & (PIX - 1)) == 0;
    if (!vec) {
        hipLaunchKernelGGL((pio_classes_generic_kernel<T>), dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, logits, ncls,
                           npix, out);
        return;
    }
    const dim3 grid((unsigned)((npix + 256 * PIX - 1) / (256 * PIX)));
    switch (ncls) {
        case 2: hipLaunchKernelGGL((pio_classes_kernel<T, 2>), grid, dim3(256), 0, st, logits, npix, out); break;
        case 3: hipLaunchKernelGGL((pio_classes_kernel<T, 3>), grid, dim3(256), 0, st, logits, npix, out); break;
        default: hipLaunchKernelGGL((pio_classes_kernel<T, 4>), grid, dim3(256), 0, st, logits, npix, out); break;
    }
}

// out[i] = lut[in[i]], 16 bytes per thread; in == out is allowed (a thread reads its chunk before it writes it)
__global__ __launch_bounds__(256) void pio_grey_kernel(const uint8_t* in, uint8_t* out, const uint8_t* __restrict__ lut,
                                                        int64_t n, int vec) {
    __shared__ uint8_t s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i >= n) return;
    if (vec && i + 16 <= n) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(in + i);
        u32x4 o;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned r = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) r |= (unsigned)s_lut[(v[w] >> (8 * k)) & 0xFFu] << (8 * k);
            o[w] = r;
        }
        *reinterpret_cast<u32x4*>(out + i) = o;
    } else {
        for (int64_t k = i; k < n && k < i + 16; ++k) out[k] = s_lut[in[k]];
    }
}

constexpr int64_t PIO_MAX = 1ll << 40;          // grids stay far below 2^31 workgroups

}  // namespace

extern "C" int uh_predict_prepare_u8(const uint8_t* img_u8, float* image_out, int* flags_ws, int B, int H, int W,
                                     uh_stream stream) {
    UH_REQUIRE(img_u8 && image_out && flags_ws, "uh_predict_prepare_u8: null pointer");
    UH_REQUIRE(B > 0 && H > 0 && W > 0, "uh_predict_prepare_u8: bad sizes B=%d H=%d W=%d", B, H, W);
    UH_REQUIRE((int64_t)B * H * W < PIO_MAX, "uh_predict_prepare_u8: batch too large");
    hipStream_t st = (hipStream_t)stream;
    const int64_t per = (int64_t)H * W, n = per * B;
    if (hipMemsetAsync(flags_ws, 0, sizeof(int) * B, st) != hipSuccess) {
        uh_set_error("uh_predict_prepare_u8: memset failed");
        return UH_ELAUNCH;
    }
    int gx = (int)((per / 16 + 2 + 255) / 256);                       // chunks: the head, the aligned ones, the tail
    if (gx > 256) gx = 256;
    hipLaunchKernelGGL(pio_any_gt1_kernel, dim3(gx, B), dim3(256), 0, st, img_u8, per, flags_ws);
    UH_CHECK_LAUNCH("pio_any_gt1_kernel");
    const int vec = uh_aligned16(img_u8) && uh_aligned16(image_out);
    hipLaunchKernelGGL(pio_prepare_kernel, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, st, img_u8, flags_ws, image_out, per,
                       n, vec);
    UH_CHECK_LAUNCH("pio_prepare_kernel");
    return UH_OK;
}

extern "C" int uh_logits_to_classes_u8(const void* logits, int64_t npix, int ncls, int dt, uint8_t* classes_out,
                                       uh_stream stream) {
    UH_REQUIRE(logits && classes_out, "uh_logits_to_classes_u8: null pointer");
    UH_REQUIRE(npix >= 0 && npix < PIO_MAX && ncls >= 1 && ncls <= 256, "uh_logits_to_classes_u8: bad sizes npix=%lld ncls=%d",
               (long long)npix, ncls);
    UH_REQUIRE(dt == UH_F32 || dt == UH_BF16, "uh_logits_to_classes_u8: bad dtype %d", dt);
    if (npix == 0) return UH_OK;
    if (dt == UH_BF16)
        pio_launch_classes<bf16_t>((const bf16_t*)logits, npix, ncls, classes_out, (hipStream_t)stream);
    else
        pio_launch_classes<float>((const float*)logits, npix, ncls, classes_out, (hipStream_t)stream);
    UH_CHECK_LAUNCH("pio_classes_kernel");
    return UH_OK;
}

extern "C" int uh_classes_to_grey_u8(const uint8_t* classes, uint8_t* grey_out, const uint8_t* lut, int64_t n, uh_stream stream) {
    UH_REQUIRE(classes && grey_out && lut, "uh_classes_to_grey_u8: null pointer");
    UH_REQUIRE(n >= 0 && n < PIO_MAX, "uh_classes_to_grey_u8: bad size n=%lld", (long long)n);
    if (n == 0) return UH_OK;
    const int vec = uh_aligned16(classes) && uh_aligned16(grey_out);
    hipLaunchKernelGGL(pio_grey_kernel, dim3((unsigned)((n + 4095) / 4096)), dim3(256), 0, (hipStream_t)stream, classes, grey_out,
                       lut, n, vec);
    UH_CHECK_LAUNCH("pio_grey_kernel");
    return UH_OK;
}
