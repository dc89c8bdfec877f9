/*
 * unet_hip.h -- C ABI of libunet_hip.so: the MI355X (gfx950) kernels behind the UNet
 * segmentation train-step path.
 *
 * The reference (Florescence/UNet-Medical-Image-Contour-Segmentation) has no FFI of its own:
 * its hot path is the torch.nn surface of unet/unet_parts.py, utils/dice_score.py,
 * utils/boundary_loss.py and train.py:113-159.  Each entry point below
 * names the reference statement(s) it replaces.  Conventions for every function:
 *
 *   - plain pointers and sizes only; device pointers unless a parameter says "host";
 *   - activations are NHWC ("channels_last", train.py:113,262): element (b,h,w,c) of a tensor
 *     with pixel stride `ld` (elements) lives at ((b*H + h)*W + w)*ld + c.  `ld` >= C lets a
 *     tensor be a channel slice of a wider buffer (zero-copy torch.cat of unet_parts.py:95);
 *   - `dt` is the activation dtype: UH_F32 or UH_BF16; statistics, reductions, weights' master
 *     copies and all gradients of parameters are fp32;
 *   - no allocation, no host sync, no global mutable state inside: workspaces are caller owned,
 *     kernels are enqueued on `stream` (a hipStream_t) and the call returns immediately;
 *   - returns 0 on success, a negative UH_E* code otherwise; uh_last_error() gives the text
 *     (thread-local).  The Python shim raises RuntimeError from it.
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* uh_stream;            /* hipStream_t */

enum { UH_F32 = 0, UH_BF16 = 1,
       /* fp32 tensors, 3x3 conv products on the bf16 matrix pipe ("bf16x3": w*x ~= wh*xh + wh*xl + wl*xh with bf16
        * halves, fp32 accumulate, ~1e-5 relative).  Accepted by uh_pack_w3x3 (writes [hi | lo] bf16 arrays of
        * Cout*9*Cin elements each into the same number of bytes as the fp32 pack), uh_conv3x3_fwd,
        * uh_conv3x3_fwd_affine_relu (MFMA-aligned shapes only: Cin % 16 == 0, Cout % 64 == 0) and uh_conv3x3_wgrad
        * (channel counts multiples of 64). */
       UH_F32X3 = 2,
       /* Flags OR-ed into the dtype argument of uh_pack_w3x3 and uh_conv3x3_fwd / uh_conv3x3_fwd_affine_relu: the packed
        * filter is FRAGMENT-MAJOR instead of KRSC -- 1 KiB blocks, one per (16 filter rows, tap, 64-byte K chunk), laid out
        * as the 64 lanes of an MFMA A-operand read them, so that the conv kernel's fragment load is 8 whole cache lines
        * instead of 16 half lines (the forward kernel was bound by its vector-memory path, not by the matrix pipe).  Only
        * for calls that uh_conv3x3_wfrag_ok() accepts (the LDS-DMA MFMA kernel); UH_WFRAG = forward copy / the `w` of a
        * conv call, UH_WFRAG_D = backward-data copy of uh_pack_w3x3 (it is the `w` of the backward-data conv call, which
        * then passes UH_WFRAG).  In uh_pack_w3x3_batched the flags are per layer (table column 9: bit 0 forward copy,
        * bit 1 backward-data copy). */
       UH_WFRAG = 0x100, UH_WFRAG_D = 0x200 };
enum { UH_OK = 0, UH_EINVAL = -1, UH_ELAUNCH = -2, UH_EWORKSPACE = -3 };

const char* uh_last_error(void);
int uh_version(void);

/* ---- parameter layout --------------------------------------------------------------------
 * nn.Conv2d weight [O,I,3,3] fp32 with arbitrary strides (contiguous or channels_last,
 * train.py:262) -> KRSC [O][3][3][I] in `dt` (w_fwd) and the flipped/transposed copy
 * [I][3][3][O] (w_dgrad, may be NULL) that turns conv3x3_fwd into the data-gradient conv. */
int uh_pack_w3x3(const float* w, int64_t sO, int64_t sI, int64_t sH, int64_t sW, int Cout, int Cin,
                 void* w_fwd, void* w_dgrad, int dt, uh_stream stream);
/* All layers at once: table = nlayers x 10 int64 on the DEVICE {w pointer, sO, sI, sH, sW, Cout, Cin, first element
 * of the layer in the flat outputs, first tile of the layer, flags}; a layer has ceil(Cout/32)*ceil(Cin/32)*9 tiles and
 * ntiles is their sum.  flags: bit 0 / bit 1 = forward / backward-data copy fragment-major (UH_WFRAG).  w_dgrad_flat may
 * be NULL. */
int uh_pack_w3x3_batched(const int64_t* table, int nlayers, int64_t ntiles, void* w_fwd_flat,
                         void* w_dgrad_flat, int dt, uh_stream stream);
/* KRSC fp32 weight gradient -> gradient tensor with the parameter's own strides. */
int uh_unpack_dw3x3(const float* dw_krsc, float* dw, int64_t sO, int64_t sI, int64_t sH, int64_t sW,
                    int Cout, int Cin, uh_stream stream);

/* ---- nn.Conv2d(k=3, padding=1, bias=False)  (unet_parts.py:15,18) --------------------------
 * y[b,h,w,o] = sum_{r,s,i} x[b,h+r-1,w+s-1,i] * w[o][r][s][i]; the input is the virtual channel
 * concat of (x0:C0) and (x1:C1) (x1 may be NULL with C1 = 0).
 * stat_partials (may be NULL): nslab = uh_conv3x3_stat_slabs(); fp32 [nslab][2][Cout] per-slab
 * (mean, M2 = sum (y - mean)^2) of the STORED y over the slab's pixels, then [nslab] pixel counts
 * (a kernel that needs fewer slabs writes 0 counts for the rest), then [nslab] scratch:
 * nslab*(2*Cout + 2) floats.  These are BatchNorm2d's batch
 * statistics (unet_parts.py:16,19) without a second pass over y.  With w = w_dgrad this is conv
 * backward-data. */
int uh_conv3x3_stat_slabs(int B, int H, int W, int Cin, int Cout, int dt);
/* 1 if uh_conv3x3_fwd will run this shape on the LDS-DMA MFMA kernel (16-byte aligned pointers assumed), i.e. if the
 * filter may be packed fragment-major (UH_WFRAG); dt = UH_F32 or UH_BF16. */
int uh_conv3x3_wfrag_ok(int B, int H, int W, int C0, int C1, int Cout, int ld0, int ld1, int ldy, int dt);
/* Which kernel uh_conv3x3_fwd (and, with the backward-data filter pack, backward-data) gives a call with dense pitches
 * (ld0 = C0, ld1 = C1, ldy = Cout) and 16-byte aligned pointers; host only, no device touched.  dt = UH_F32, UH_BF16 or
 * UH_F32X3.  0 = not an MFMA shape (stem or generic kernel), 1 = 128-channel slabs, 2 = register-resident filter, 3 = K split
 * inside the workgroup, 4 = streaming filter, 5 = a tensor past the 2 GiB buffer window (the older MFMA kernel).  The kernels
 * sum in different orders: a batch gives bit-identical per-image results only where every layer gets the same answer as for
 * one image (BatchPredictor.launch_lengths).  UH_EINVAL for a bad shape or dtype. */
int uh_conv3x3_fwd_kernel(int B, int H, int W, int C0, int C1, int Cout, int dt);
/* The same question for backward-weights: the launch plan uh_conv3x3_wgrad (narrow = 0) or uh_conv3x3_wgrad_narrow (narrow = 1)
 * gives a call with dense pitches (ld0 = C0, ld1 = C1, lddy = Cout) and 16-byte aligned pointers; host only.  out[0..7] (HOST
 * memory) = { kernel, nsplit, grid.x, grid.y, threads, slab format, reduce kernel, reduce blocks }.
 * kernel: 0 = conv3x3_wgrad_generic (no workspace, no reduction), 1 / 2 / 3 = conv3x3_wgrad_stem / _stem_v2 / _stem_v3 (at most 4
 * input channels in one source; v3: bf16 with 64 output channels), 4 = conv3x3_wgrad_mfma (fp32, bf16x3, or bf16 with a tensor
 * past the 2 GiB buffer window), 5 / 6 = the bf16 LDS-DMA kernel conv3x3_wgrad_mfma_v2 with 64- / 128-row output-channel tiles.
 * nsplit = the pixel ranges, one slab of Cout * 9 * (C0 + C1) partial sums each in the workspace (0 for kernel 0).
 * slab format: 0 = fp32, 1 = block-scaled fp16 pairs (kernels 5 and 6 unless UH_WGRAD_SLAB_F32=1).
 * reduce kernel: 0 = none, 1 = scalar (the result is no multiple of 4 floats; in a call, also where dw_krsc or ws is off 16
 * bytes), 2 = 16-byte pieces, 3 = many splits of a small result (uh_stem_bn_relu_bwd_wgrad only: never in this answer),
 * 4 = fp16 pairs; reduce blocks = its workgroups, the row's block count in uh_slab_reduce_batched's table.
 * A narrow or bf16x3 (UH_F32X3) call exists on the MFMA path only: for those the answer describes a call only where kernel >= 4,
 * any other shape is refused by the call itself.  UH_EINVAL for a bad shape or dtype or out == NULL. */
int uh_conv3x3_wgrad_plan(int B, int H, int W, int C0, int C1, int Cout, int dt, int narrow, int64_t* out);
/* The pinned plan (batch-invariant eval forward).  plan_B > 0: the kernel FORM is chosen as for a launch of plan_B images of this
 * H x W, while tiles, grid, byte extents and the 2 GiB test (code 5) stay with the real B; where the launch's own form sums in the
 * same order as the pinned one (uh_conv3x3_fwd_sum_class) the launch keeps its own.  plan_B = 0: the unpinned answers above.
 * uh_conv3x3_fwd_kernel_plan = the code uh_conv3x3_fwd_affine_relu_plan(.., B, plan_B, ..) runs; uh_conv3x3_wfrag_ok_plan = may its
 * filter be packed fragment-major (codes 1-4).  With plan_B = 1 every image of a batch is computed bit for bit as it is alone. */
int uh_conv3x3_fwd_kernel_plan(int B, int plan_B, int H, int W, int C0, int C1, int Cout, int dt);
int uh_conv3x3_wfrag_ok_plan(int B, int plan_B, int H, int W, int C0, int C1, int Cout, int ld0, int ld1, int ldy, int dt);
/* Summation class of a kernel code 0..5: codes of one class add a pixel's products in the same order and give the same bits
 * (1, 2 and 4 -> 1; 0, 3 and 5 stand alone).  UH_EINVAL for another code. */
int uh_conv3x3_fwd_sum_class(int kernel);
int uh_conv3x3_fwd(const void* x0, int C0, int ld0, const void* x1, int C1, int ld1,
                   const void* w, void* y, int ldy, int Cout, float* stat_partials,
                   int B, int H, int W, int dt, uh_stream stream);
/* Backward-data of the SECOND conv of a DoubleConv fused with the first pass of the BatchNorm backward of the layer in front of it
 * (unet_parts.py:15-20 differentiated).  The launch computes dx = conv(dy, w_dgrad) as uh_conv3x3_fwd
 * does -- dx is the gradient of z = ReLU(BatchNorm(q)), q [B,H,W,Cdx] the raw output of the first conv -- and, from its
 * accumulators (rounded to bf16 as stored) and one read of q, the per-workgroup partial sums
 *     partials[row][0][c] = sum_p g,   partials[row][1][c] = sum_p g * (q - mean[c]) * rstd[c],    g = dx where q*scale+shift > 0 else 0
 * in the [nblk][2][C] layout uh_bn_relu_bwd_apply / uh_bn_bwd_finalize take: uh_bn_relu_bwd_reduce (a read of dx and of q) is not
 * launched for that layer.  coef = [scale | shift | mean | rstd], Cdx floats each (what uh_bn_finalize produced in the forward).
 * bf16, MFMA-aligned single-source shapes below 2 GiB, ldq == lddx: uh_conv3x3_dgrad_bnsum_rows() returns the number of partial rows the
 * call writes (nblk), or 0 when the shape must take the two separate kernels.  dt may carry UH_WFRAG (pack of w_dgrad). */
int uh_conv3x3_dgrad_bnsum_rows(int B, int H, int W, int Cdy, int Cdx, int lddy, int lddx, int ldq, int dt);
int uh_conv3x3_dgrad_bnsum(const void* dy, int Cdy, int lddy, const void* w_dgrad, void* dx, int lddx, int Cdx,
                           const void* q, int ldq, const float* coef, float* partials,
                           int B, int H, int W, int dt, uh_stream stream);
/* The stem of the network with a RECOMPUTED output (inc.double_conv.0-2: Conv2d(1 -> 64) -> BatchNorm2d -> ReLU on a
 * single-channel image, unet_parts.py:15-17; unet_model.py:15): the conv output y costs 9 multiply-adds per element and is the
 * largest tensor of the model, so it is never stored -- every consumer rebuilds it from the image on the matrix pipe (a GEMM
 * with K = 9: csrc/stem_mfma.hip) with the roundings of the stored path (y to bf16 before BatchNorm, dy to bf16 before the
 * contraction).  The MFMA adds the nine products in its own order: against the serial-FMA stem kernel of uh_conv3x3_fwd, y
 * differs by one bf16 ulp on about one element in 10^4; all four entry points use the same arithmetic, so the backward pass
 * sees exactly the forward pass's ReLU mask and xhat.
 *   uh_stem_stats               per-workgroup BatchNorm statistics rows of y (layout / row count of uh_conv3x3_fwd: feed uh_bn_finalize)
 *   uh_stem_bn_relu_fwd         z = max(round_bf16(conv(x, w)) * scale + shift, 0)
 *   uh_stem_bn_relu_bwd_reduce  partials[uh_stem_nblk()][2][64] = {sum dz [z>0], sum dz [z>0] xhat}  (finish with uh_bn_bwd_finalize)
 *   uh_stem_bn_relu_bwd_wgrad   dw[64][3][3][1] = sum dy (x) x with dy = scale * (dz [z>0] - dbeta/n - xhat * dgamma/n) rounded
 *                               to bf16 as uh_bn_relu_bwd_apply would store it (n_total: pixel count of the statistics, 0 = B*H*W)
 * bf16, Cin = 1, w = KRSC pack [64][9][1] (uh_pack_w3x3); dz / z 16-byte aligned.  uh_stem_ok() says whether a layer qualifies. */
int uh_stem_ok(int Cin, int Cout, int dt);
int uh_stem_nblk(int B, int H, int W);
int uh_stem_stats(const void* x, int Cin, int ldx, const void* w, float* stat_partials, int B, int H, int W, int dt,
                  uh_stream stream);
int uh_stem_bn_relu_fwd(const void* x, int Cin, int ldx, const void* w, const float* scale, const float* shift, void* z, int ldz,
                        int B, int H, int W, int dt, uh_stream stream);
int uh_stem_bn_relu_bwd_reduce(const void* dz, int lddz, const void* x, int Cin, int ldx, const void* w, const float* scale,
                               const float* shift, const float* mean, const float* rstd, float* partials, int B, int H, int W,
                               int dt, uh_stream stream);
size_t uh_stem_bwd_wgrad_ws_bytes(int B, int H, int W, int Cin);
int uh_stem_bn_relu_bwd_wgrad(const void* dz, int lddz, const void* x, int Cin, int ldx, const void* w, const float* scale,
                              const float* shift, const float* mean, const float* rstd, const float* dgamma, const float* dbeta,
                              int64_t n_total, float* dw_krsc, void* ws, size_t ws_bytes, int B, int H, int W, int dt,
                              uh_stream stream);
/* Inference form of (Conv2d -> BatchNorm2d(eval) -> ReLU)  (unet_parts.py:15-20 under model.eval(),
 * evaluate.py:30 / predict.py:17): z = max(conv(x, w)*scale + shift, 0) with scale/shift from
 * uh_bn_eval_coeffs, applied to the accumulators -- the pre-BatchNorm tensor is never written. */
int uh_conv3x3_fwd_affine_relu(const void* x0, int C0, int ld0, const void* x1, int C1, int ld1,
                               const void* w, void* z, int ldz, int Cout, const float* scale,
                               const float* shift, int B, int H, int W, int dt, uh_stream stream);
/* The same call under the pinned plan (see uh_conv3x3_fwd_kernel_plan): plan_B = 0 is uh_conv3x3_fwd_affine_relu. */
int uh_conv3x3_fwd_affine_relu_plan(const void* x0, int C0, int ld0, const void* x1, int C1, int ld1,
                                    const void* w, void* z, int ldz, int Cout, const float* scale,
                                    const float* shift, int B, int plan_B, int H, int W, int dt, uh_stream stream);
/* conv backward-weights: dw[o][r][s][i] = sum_{b,h,w} dy[b,h,w,o] * x[b,h+r-1,w+s-1,i] (fp32 KRSC).
 * bf16 MFMA path: the per-split partial sums (fp32 accumulators) travel through `ws` as block-scaled fp16 -- 11 significant
 * bits, one power-of-two scale per workgroup block -- and are added in fp32 in a fixed order (deterministic); UH_WGRAD_SLAB_F32=1
 * in the environment keeps them fp32. */
size_t uh_conv3x3_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout, int dt);
int uh_conv3x3_wgrad(const void* dy, int lddy, const void* x0, int C0, int ld0,
                     const void* x1, int C1, int ld1, float* dw_krsc, int Cout,
                     void* ws, size_t ws_bytes, int B, int H, int W, int dt, uh_stream stream);
/* Backward-weights in two stages, the second deferred and batched.  uh_conv3x3_wgrad_partials = uh_conv3x3_wgrad without its
 * closing reduction over the pixel splits: the partial results stay in `ws` (which must stay alive and untouched until the
 * reduction has run) and desc[0..7] -- HOST memory -- receives { slabs, dw_krsc, n, nsplit, format, row, blocks, rows per scale block }; desc[3] == 0
 * means the shape took a path without slabs and dw_krsc is already final.  uh_slab_reduce_batched finishes any number of such
 * layers in ONE launch: `table` is DEVICE memory holding the rows (8 int64 each) with [6] replaced by the row's first block
 * (running sum of the block counts), total_blocks their sum.  Filter gradients only feed the optimizer (train.py:157-158), so
 * the eighteen small reduce launches of a backward pass can wait until then.  Results are bit-identical to uh_conv3x3_wgrad. */
int uh_conv3x3_wgrad_partials(const void* dy, int lddy, const void* x0, int C0, int ld0, const void* x1, int C1, int ld1,
                              float* dw_krsc, int Cout, void* ws, size_t ws_bytes, int B, int H, int W, int dt,
                              int64_t* desc, uh_stream stream);
int uh_slab_reduce_batched(const int64_t* table, int nrows, int64_t total_blocks, uh_stream stream);
/* Narrow-tensor forms for the small-width models (UNet_S / UNet_T, unet_model.py:52-126: 8..64-channel layers).  The
 * layer is COMPUTED as the next 64-aligned layer (filters zero-padded to C0 + C1 -> Cout, all multiples of 64, so the MFMA
 * kernels apply), but the tensors in HBM hold only their first C0v / C1v / Coutv channels per pixel (multiples of one
 * 16-byte piece: 8 bf16 / 4 fp32; ld* >= the valid count): channels beyond the valid count are read as zeros and never
 * written.  stat_partials / scale / shift are sized for the padded Cout.  fwd: scale == shift == NULL stores the raw conv
 * output (training, + optional statistics); otherwise the inference form z = max(conv*scale + shift, 0).
 * wgrad: dw_krsc is the padded [Cout][3][3][C0 + C1] gradient (rows / columns of padding come out 0); workspace from
 * uh_conv3x3_wgrad_ws_bytes of the padded shape.  Shapes outside the MFMA path return UH_EINVAL.
 * uh_pack_w3x3_padded: uh_pack_w3x3 of the reference-layout filter [Cout][C0 + C1][3][3] into the padded layer
 * [Coutp][Cp0 + Cp1] (source block 0 -> padded channels 0.., block 1 -> Cp0.., zeros elsewhere); the backward-data copy
 * [Cp0 + Cp1][3][3][Coutp] holds the per-source filters as its row blocks (UH_F32 / UH_BF16). */
int uh_pack_w3x3_padded(const float* w, int64_t sO, int64_t sI, int64_t sH, int64_t sW, int Cout, int C0, int C1,
                        int Coutp, int Cp0, int Cp1, void* w_fwd, void* w_dgrad, int dt, uh_stream stream);
int uh_conv3x3_fwd_narrow(const void* x0, int C0, int C0v, int ld0, const void* x1, int C1, int C1v, int ld1,
                          const void* w, void* y, int ldy, int Cout, int Coutv, float* stat_partials,
                          const float* scale, const float* shift, int B, int H, int W, int dt, uh_stream stream);
/* The same call under the pinned plan (see uh_conv3x3_fwd_kernel_plan): plan_B = 0 is uh_conv3x3_fwd_narrow. */
int uh_conv3x3_fwd_narrow_plan(const void* x0, int C0, int C0v, int ld0, const void* x1, int C1, int C1v, int ld1,
                               const void* w, void* y, int ldy, int Cout, int Coutv, float* stat_partials,
                               const float* scale, const float* shift, int B, int plan_B, int H, int W, int dt, uh_stream stream);
int uh_conv3x3_wgrad_narrow(const void* dy, int lddy, int Cout, int Coutv, const void* x0, int C0, int C0v, int ld0,
                            const void* x1, int C1, int C1v, int ld1, float* dw_krsc, void* ws, size_t ws_bytes,
                            int B, int H, int W, int dt, uh_stream stream);

/* ---- nn.BatchNorm2d + nn.ReLU(inplace)  (unet_parts.py:16-17,19-20) ------------------------
 * finalize: merge the conv's stat slabs (Chan's formula, double) -> mean, rstd = 1/sqrt(var_biased + eps),
 * scale = gamma*rstd, shift = beta - mean*scale; running stats (may be NULL) updated in place with
 * `momentum` and the UNBIASED variance (n = pixels per channel); *num_batches_tracked (int64 on the
 * device, may be NULL) += 1.  Slab rows whose pixel count is 0 are ignored; n == 0: use the sum of the rows' counts.
 * m2_out (may be NULL): the merged
 * M2 = sum (y - mean)^2 per channel -- with (mean, M2, n) per rank as rows, a second call merges ranks (SyncBN). */
int uh_bn_finalize(const float* stat_partials, int nslab, int C, int64_t n,
                   const float* gamma, const float* beta, float* running_mean, float* running_var,
                   int64_t* num_batches_tracked, float momentum, float eps,
                   float* scale, float* shift, float* mean, float* rstd, float* m2_out, uh_stream stream);
/* uh_bn_finalize over the first C channels of stat rows that are ldc >= C channels wide (small-width layers: the conv, and
 * so its statistics, are laid out for the 64-aligned channel count, uh_conv3x3_fwd_narrow); per-channel arrays: C entries. */
int uh_bn_finalize_ld(const float* stat_partials, int nslab, int ldc, int C, int64_t n,
                      const float* gamma, const float* beta, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, float momentum, float eps,
                      float* scale, float* shift, float* mean, float* rstd, float* m2_out, uh_stream stream);
/* eval mode: scale/shift from the running statistics. */
int uh_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, float eps, int C, float* scale, float* shift,
                      uh_stream stream);
/* The launch plan of the pixel passes (BatchNorm + ReLU apply / backward, the pool tail, max-pool, bilinear x2, the 1x1
 * backward-data): what a call over `items` pixels (or 2x2 windows) of C channels takes; host only, no device touched.
 * aligned != 0: every tensor of the call is 16-byte aligned with a pixel stride of whole 16-byte pieces.  cap: the most
 * workgroups of 256 threads the pass asks for (4096; 8192 for the 1x1 conv).  out[0..2] (HOST memory) = {vec, hoist, grid}:
 * vec = channels per thread (8 bf16 / 4 fp32 where aligned and C is a multiple of that, else 1), grid = workgroups =
 * min(cap, ceil(items * (C / vec) / 256)), hoist = 1 where vec > 1 and grid * 256 is a multiple of C / vec: every thread then stays on
 * one channel group and the kernels that can keep that group's coefficients in registers do.  UH_EINVAL for a bad
 * size or dtype or out == NULL. */
int uh_pixel_pass_plan(int64_t items, int C, int dt, int aligned, int cap, int64_t* out);
/* z = max(y*scale + shift, 0) */
int uh_bn_relu_apply(const void* y, int ldy, const float* scale, const float* shift,
                     void* z, int ldz, int64_t npix, int C, int dt, uh_stream stream);
/* backward, pass 1: per-channel sums of dz*[z>0] and dz*[z>0]*xhat -> partials [nblk][2][C];
 * returns the number of partial rows it will write through uh_bn_bwd_nblk(). */
int uh_bn_bwd_nblk(int64_t npix, int C);
int uh_bn_relu_bwd_reduce(const void* dz, int lddz, const void* y, int ldy,
                          const float* scale, const float* shift, const float* mean, const float* rstd,
                          float* partials, int64_t npix, int C, int dt, uh_stream stream);
/* backward, pass 2: dgamma = sum2, dbeta = sum1 (written fp32), and
 * dy = scale*(dz*[z>0] - sum1/n - xhat*sum2/n) with n = n_total (0: npix).  nblk == 0: dgamma / dbeta already hold
 * the sums (e.g. all-reduced over the ranks of a data-parallel job: SyncBN, with n_total the global pixel count)
 * and are only read.  uh_bn_bwd_finalize is the first half alone (partials -> dgamma, dbeta). */
int uh_bn_bwd_finalize(const float* partials, int nblk, int C, float* dgamma, float* dbeta, uh_stream stream);
int uh_bn_relu_bwd_apply(const void* dz, int lddz, const void* y, int ldy,
                         const float* scale, const float* shift, const float* mean, const float* rstd,
                         const float* partials, int nblk, float* dgamma, float* dbeta,
                         void* dy, int lddy, int64_t npix, int64_t n_total, int C, int dt, uh_stream stream);

/* ---- BatchNorm + ReLU fused with its consumer (csrc/bn_fused.hip) ---------------------------
 * "pool tail": the second conv of an encoder DoubleConv (unet_parts.py:18-20), whose activation is the skip connection
 * AND the input of nn.MaxPool2d(2) (unet_parts.py:32; unet_model.py:28-32).  uh_bn_relu_pool_ok: H, W even, C a multiple
 * of 16 bytes.  apply: z = relu(bn(y)) [B,H,W,C] and pooled [B,H/2,W/2,C] in one pass over y.  The backward passes
 * replace uh_maxpool2_bwd + uh_bn_relu_bwd_reduce / _apply: dz = dskip (may be NULL) + route(dpool) is rebuilt on the fly
 * (never stored), bit-identical to what the unfused kernels compute; partials / nblk / dgamma / dbeta / n_total as in
 * uh_bn_relu_bwd_reduce / uh_bn_relu_bwd_apply with npix = B*H*W. */
int uh_bn_relu_pool_ok(int B, int H, int W, int C, int dt);
int uh_bn_relu_pool_apply(const void* y, int ldy, const float* scale, const float* shift, void* z, int ldz,
                          void* pooled, int ldp, int B, int H, int W, int C, int dt, uh_stream stream);
int uh_bn_relu_pool_bwd_reduce(const void* dskip, int ldskip, const void* dpool, int lddp, const void* y, int ldy,
                               const float* scale, const float* shift, const float* mean, const float* rstd,
                               float* partials, int B, int H, int W, int C, int dt, uh_stream stream);
int uh_bn_relu_pool_bwd_apply(const void* dskip, int ldskip, const void* dpool, int lddp, const void* y, int ldy,
                              const float* scale, const float* shift, const float* mean, const float* rstd,
                              const float* partials, int nblk, float* dgamma, float* dbeta, void* dy, int lddy,
                              int B, int H, int W, int64_t n_total, int C, int dt, uh_stream stream);
/* "head tail": the last DoubleConv's second conv, whose activation only feeds the 1x1 OutConv (unet_parts.py:103;
 * unet_model.py:37).  uh_bn_relu_head_ok: C = 8 or 16 sixteen-byte channel groups (64 / 128 channels in bf16), n_classes
 * <= 4.  fwd: logits[p][k] = head_b[k] + sum_c relu(bn(y))[p][c] * head_w[k][c] (fp32; the activation is rounded to the
 * tensor dtype first, as if it had been stored) -- z is never written.  bwd_reduce: the BatchNorm partials of
 * dz = dlogits . head_w AND the OutConv gradients dhead_w [ncls][C], dhead_b [ncls] (fp32, written); ws: scratch of
 * uh_bn_relu_head_bwd_ws_bytes.  bwd_apply: as uh_bn_relu_bwd_apply with dz rebuilt from dlogits. */
int uh_bn_relu_head_ok(int C, int ncls, int dt);
int uh_bn_relu_head_fwd(const void* y, int ldy, const float* scale, const float* shift, const float* head_w,
                        const float* head_b, float* logits, int64_t npix, int C, int ncls, int dt, uh_stream stream);
size_t uh_bn_relu_head_bwd_ws_bytes(int64_t npix, int C, int ncls);
int uh_bn_relu_head_bwd_reduce(const float* dlogits, const float* head_w, const void* y, int ldy, const float* scale,
                               const float* shift, const float* mean, const float* rstd, float* partials,
                               float* dhead_w, float* dhead_b, void* ws, size_t ws_bytes, int64_t npix, int C,
                               int ncls, int dt, uh_stream stream);
int uh_bn_relu_head_bwd_apply(const float* dlogits, const float* head_w, const void* y, int ldy, const float* scale,
                              const float* shift, const float* mean, const float* rstd, const float* partials,
                              int nblk, float* dgamma, float* dbeta, void* dy, int lddy, int64_t npix,
                              int64_t n_total, int C, int ncls, int dt, uh_stream stream);

/* ---- nn.MaxPool2d(2)  (unet_parts.py:32) -------------------------------------------------- */
int uh_maxpool2_fwd(const void* x, int ldx, void* y, int ldy, int B, int H, int W, int C, int dt,
                    uh_stream stream);
/* dx = (dskip ? dskip : 0) + route(dy) to the FIRST maximum of each 2x2 window in row-major
 * order; rows/cols beyond 2*floor(H/2) get only dskip. */
int uh_maxpool2_bwd(const void* x, int ldx, const void* dy, int lddy, const void* dskip, int ldskip,
                    void* dx, int lddx, int B, int H, int W, int C, int dt, uh_stream stream);

/* ---- nn.Upsample(2, 'bilinear', align_corners=True) + F.pad  (unet_parts.py:70,85-88) ------
 * x [B,h,w,C] -> y [B,Ho,Wo,C]: the 2h x 2w upsampled image sits at (pad_top, pad_left), the rest
 * of y is zero filled. */
int uh_upsample2x_fwd(const void* x, int ldx, void* y, int ldy, int B, int h, int w, int C,
                      int Ho, int Wo, int pad_top, int pad_left, int dt, uh_stream stream);
/* The same with the BatchNorm + ReLU in front of it applied on the way in: x is the RAW output of the last conv below an Up block
 * (unet_model.py:34-37), the activation max(x*scale + shift, 0) -- read by nothing but nn.Upsample (unet_parts.py:70,80) -- is
 * rounded to the tensor dtype as uh_bn_relu_apply would store it and interpolated, never written.  Bit-identical to
 * uh_bn_relu_apply + uh_upsample2x_fwd.  uh_bn_relu_upsample2x_ok: 1 when the shape takes the fused kernel (C a multiple of a
 * 16-byte piece; pointers / strides 16-byte aligned are checked by the call). */
int uh_bn_relu_upsample2x_ok(int B, int h, int w, int C, int Ho, int Wo, int dt);
int uh_bn_relu_upsample2x_fwd(const void* x, int ldx, const float* scale, const float* shift, void* y, int ldy,
                              int B, int h, int w, int C, int Ho, int Wo, int pad_top, int pad_left, int dt, uh_stream stream);
int uh_upsample2x_bwd(const void* dy, int lddy, void* dx, int lddx, int B, int h, int w, int C,
                      int Ho, int Wo, int pad_top, int pad_left, int dt, uh_stream stream);

/* ---- SpatialAttention + the gated skip of Up(use_attention=True)  (unet_parts.py:39-60,91-92) ---------------------
 * x [B,H,W,C] in dt with pixel stride ldx; w = the conv1 weight [1][2][k][k] fp32 contiguous (k = 3 or 7, zero padding k/2).
 * Forward: pool = fp32 [B*H*W][2] (channel mean, channel max; 8-byte aligned), amax = int32 [B*H*W] (the FIRST maximal
 * channel, which receives the max's gradient as torch.max(dim=1) routes it), a = fp32 [B*H*W] the sigmoid map; y (may be
 * NULL: the standalone module) = x * a in dt, rounded once, pixel stride ldy.
 * Backward: exactly one of dy (the gate: gradient of y, pixel stride lddy; x is then needed) and ga (the standalone map:
 * fp32 [B*H*W] gradient of a) is given.  ws = fp32 workspace of 3*B*H*W floats, 8-byte aligned (the gradient of pool, then
 * g_a * a * (1 - a)); dx = dy*a + d(mean)/dx + d(max)/dx in dt (pixel stride lddx); dw = fp32 [2*k*k], summed over
 * per-workgroup rows dw_partials = fp32 [nblk][2*k*k] with nblk >= uh_spatial_attn_dw_nblk(B, H, W) in a fixed order
 * (bit-identical between runs).  B <= 65535.
 * uh_spatial_attn_plan: the launch form a call takes; host only, no device touched.  aligned != 0: every channel tensor of the
 * call (forward: x and y; backward: dx, and dy and x of the gate) is 16-byte aligned with a pixel stride of whole 16-byte
 * pieces.  out[0..2] (HOST memory) = {V, G, steps}: V = channels per lane and step (8 bf16 / 4 fp32 where aligned and C is a
 * multiple of that, else 1), G = the lanes that share a pixel in the channel reductions (the smallest power of two that holds
 * ceil(C / V), at most 64; the map's backward, whose gradient is given per pixel, reduces nothing and uses one lane),
 * steps = ceil(ceil(C / V) / G), the strides of G * V channels a lane takes.  UH_EINVAL for a bad size or dtype or out == NULL. */
int uh_spatial_attn_dw_nblk(int B, int H, int W);
int uh_spatial_attn_plan(int C, int dt, int aligned, int64_t* out);
int uh_spatial_attn_fwd(const void* x, int ldx, const float* w, int k, float* pool, int* amax, float* a, void* y,
                        int ldy, int B, int H, int W, int C, int dt, uh_stream stream);
int uh_spatial_attn_bwd(const void* dy, int lddy, const float* ga, const void* x, int ldx, const float* w, int k,
                        const float* pool, const int* amax, const float* a, float* ws, void* dx, int lddx,
                        float* dw, float* dw_partials, int nblk, int B, int H, int W, int C, int dt,
                        uh_stream stream);

/* ---- nn.ConvTranspose2d(Cin, Cout, 2, 2) + F.pad  (unet_parts.py:73,85-88) -----------------
 * w is the parameter itself: [Cin][Cout][2][2] fp32 contiguous; bias [Cout] fp32. */
int uh_convt2x2_fwd(const void* x, int ldx, const float* w, const float* bias, void* y, int ldy,
                    int B, int h, int w_, int Cin, int Cout, int Ho, int Wo, int pad_top, int pad_left,
                    int dt, uh_stream stream);
int uh_convt2x2_dgrad(const void* dy, int lddy, const float* w, void* dx, int lddx,
                      int B, int h, int w_, int Cin, int Cout, int Ho, int Wo, int pad_top, int pad_left,
                      int dt, uh_stream stream);
size_t uh_convt2x2_wgrad_ws_bytes(int B, int h, int w_, int Cin, int Cout);
int uh_convt2x2_wgrad(const void* dy, int lddy, const void* x, int ldx, float* dw, float* dbias,
                      void* ws, size_t ws_bytes, int B, int h, int w_, int Cin, int Cout,
                      int Ho, int Wo, int pad_top, int pad_left, int dt, uh_stream stream);

/* MFMA path of the same layer (csrc/convt_mfma.hip): all three directions as K-contiguous GEMMs over pixels.
 * uh_convt2x2_mfma_ok() tells whether a problem qualifies (channel counts multiples of a 64-byte chunk, tensors
 * below 2 GiB, pixel count a multiple of the chunk); otherwise use the functions above.
 * uh_convt2x2_pack: reference weight [Cin][Cout][2][2] fp32 -> w_fwd [(q,co)][ci] and w_dgrad [ci][(q,co)]
 * (Cin*Cout*4 elements each, activation dtype), q = 2*r + s. */
int uh_convt2x2_mfma_ok(int B, int h, int w_, int Cin, int Cout, int Ho, int Wo, int dt);
/* Pinned twin: 1 iff a launch of plan_B images qualifies (then every multiple does) AND the real B fits the 2 GiB windows;
 * plan_B = 0 is uh_convt2x2_mfma_ok(B, ..).  0 = run uh_convt2x2_fwd for the whole batch. */
int uh_convt2x2_mfma_ok_plan(int B, int plan_B, int h, int w_, int Cin, int Cout, int Ho, int Wo, int dt);
int uh_convt2x2_pack(const float* w, int Cin, int Cout, void* w_fwd, void* w_dgrad, int dt, uh_stream stream);
int uh_convt2x2_fwd_mfma(const void* x, int ldx, const void* w_fwd, const float* bias, void* y, int ldy,
                         int B, int h, int w_, int Cin, int Cout, int Ho, int Wo, int pad_top, int pad_left,
                         int dt, uh_stream stream);
int uh_convt2x2_dgrad_mfma(const void* dy, int lddy, const void* w_dgrad, void* dx, int lddx,
                           int B, int h, int w_, int Cin, int Cout, int Ho, int Wo, int pad_top, int pad_left,
                           int dt, uh_stream stream);
size_t uh_convt2x2_wgrad_mfma_ws_bytes(int B, int h, int w_, int Cin, int Cout, int dt);
int uh_convt2x2_wgrad_mfma(const void* dy, int lddy, const void* x, int ldx, float* dw, float* dbias,
                           void* ws, size_t ws_bytes, int B, int h, int w_, int Cin, int Cout,
                           int Ho, int Wo, int pad_top, int pad_left, int dt, uh_stream stream);

/* ---- OutConv: nn.Conv2d(Cin, ncls, 1) with bias  (unet_parts.py:103) -----------------------
 * w [ncls][Cin] fp32, bias [ncls] fp32; logits are fp32 [npix][ncls]. */
int uh_conv1x1_fwd(const void* x, int ldx, const float* w, const float* bias, float* logits,
                   int64_t npix, int Cin, int ncls, int dt, uh_stream stream);
int uh_conv1x1_dgrad(const float* dlogits, const float* w, void* dx, int lddx,
                     int64_t npix, int Cin, int ncls, int dt, uh_stream stream);
size_t uh_conv1x1_wgrad_ws_bytes(int64_t npix, int Cin, int ncls);
int uh_conv1x1_wgrad(const float* dlogits, const void* x, int ldx, float* dw, float* dbias,
                     void* ws, size_t ws_bytes, int64_t npix, int Cin, int ncls, int dt, uh_stream stream);

/* ---- losses ------------------------------------------------------------------------------
 * Binary path (train.py:118-134): t = (mask / mask_div) as float (train.py:119 uses // 2), or t
 * taken from `target_f` when mask is NULL.  sums[0..3] = { sum softplus-BCE, sum sigmoid*t,
 * sum sigmoid, sum t } (fp32, caller zeroes nothing: the kernel overwrites). */
size_t uh_loss_ws_bytes(int64_t n);
int uh_bce_dice_sums(const float* logits, const int64_t* mask, int mask_div, const float* target_f,
                     int64_t n, float* sums, void* ws, size_t ws_bytes, uh_stream stream);
/* dlogits = gscale[0] * ( w_bce*(sigmoid - t)/n + w_dice * d(1 - dice)/dlogit ) with the Dice
 * ratio formed from `sums` (global-batch sums; after a cross-rank all-reduce they give the
 * single-process reference's gradient).  dice_score.py:14-18 including the sets_sum==0 branch.
 * gscale is a device pointer (upstream gradient of the scalar loss); n_mean = element count of
 * the BCE mean (the GLOBAL batch when sharded). */
int uh_bce_dice_grad(const float* logits, const int64_t* mask, int mask_div, const float* target_f,
                     int64_t n, const float* sums, double n_mean, float w_bce, float w_dice,
                     const float* gscale, float* dlogits, uh_stream stream);
/* Multi-class path (train.py:136-142): logits [npix][ncls] fp32, mask int64 class ids.
 * sums = { sum CE, inter[c]..., psum[c]..., tsum[c]... } (1 + 3*ncls floats). */
int uh_ce_dice_sums(const float* logits, const int64_t* mask, int64_t npix, int ncls, float* sums,
                    void* ws, size_t ws_bytes, uh_stream stream);
int uh_ce_dice_grad(const float* logits, const int64_t* mask, int64_t npix, int ncls,
                    const float* sums, double n_mean, float w_ce, float w_dice, const float* gscale,
                    float* dlogits, uh_stream stream);
/* dice_coeff (dice_score.py:5-25) for arbitrary float inputs: per-group sums {sum x*t, sum x, sum t}
 * over `ngroups` contiguous groups of `group_len` elements -> sums [ngroups][3]. */
int uh_dice_sums(const float* x, const float* t, int64_t ngroups, int64_t group_len, float* sums,
                 void* ws, size_t ws_bytes, uh_stream stream);
/* boundary_loss (boundary_loss.py:5-118), value only.  pred [B][H][W] fp32 with element stride
 * `pstride` (4-D [B,C,H,W]-logical channel select = base pointer + stride), target fp32 [B][H][W];
 * out[0] = loss.  ws from uh_loss_ws_bytes(B*H*W). */
int uh_boundary_loss(const float* pred, int64_t pstride, int64_t bstride, const float* target, int B, int H, int W,
                     int edge_width, float edge_weight, float smooth, float* out,
                     void* ws, size_t ws_bytes, uh_stream stream);
/* The same with the target given as the int64 class-index mask and a divisor, target = mask / mask_div (train.py:119 `true_masks
 * //= 2` feeding train.py:134): no float copy of the mask is made. */
int uh_boundary_loss_mask(const float* pred, int64_t pstride, int64_t bstride, const int64_t* mask, int mask_div, int B, int H,
                          int W, int edge_width, float edge_weight, float smooth, float* out, void* ws, size_t ws_bytes,
                          uh_stream stream);

/* ---- clip_grad_norm_ + RMSprop  (train.py:80-81,157-158) -----------------------------------
 * Flat-buffer form: all parameters / gradients / optimizer states live in four equally laid out
 * fp32 buffers of n elements (the Python shim points every nn.Parameter at a view of them).
 * uh_grad_sumsq: norm_out[0] = sqrt(sum g^2)  (clip_grad_norm_'s total_norm).
 * uh_rmsprop_step: coef = min(1, max_norm/(norm+1e-6)); g *= coef (written back, as
 * clip_grad_norm_ does); g += wd*p; v = alpha*v + (1-alpha)*g^2; buf = mu*buf + g/(sqrt(v)+eps);
 * p -= lr*buf.  total_norm is a device pointer (no host sync); max_norm <= 0 disables clipping. */
size_t uh_optim_ws_bytes(int64_t n);
int uh_grad_sumsq(const float* g, int64_t n, float* norm_out, void* ws, size_t ws_bytes, uh_stream stream);
int uh_rmsprop_step(float* p, float* g, float* square_avg, float* momentum_buf, int64_t n,
                    const float* total_norm, float max_norm, float lr, float alpha, float eps,
                    float weight_decay, float momentum, uh_stream stream);
/* uh_rmsprop_step_ema: the same pass with one more stream, the exponential moving average of the parameters:
 * ema += c * (p_new - ema), c = 1 - d_t, d_t = warmup > 0 ? min(decay, (1 + t) / (warmup + t)) : decay, all in fp32,
 * t = updates[0] read on the device (the step may be replayed from a captured graph).  What it writes to p, g,
 * square_avg and momentum_buf is bit-identical to uh_rmsprop_step; a non-finite total_norm leaves ema untouched too.
 * uh_ema_tick: updates[0] += 1 unless total_norm[0] is not finite (total_norm may be NULL); once per optimizer step,
 * behind its uh_rmsprop_step_ema launches.
 * uh_swap_f32: exchanges two disjoint 16-byte aligned buffers of n floats (averaged weights in and out of the model). */
int uh_rmsprop_step_ema(float* p, float* g, float* square_avg, float* momentum_buf, float* ema, int64_t n,
                        const float* total_norm, float max_norm, float lr, float alpha, float eps,
                        float weight_decay, float momentum, float decay, int warmup, const int32_t* updates,
                        uh_stream stream);
int uh_ema_tick(int32_t* updates, const float* total_norm, uh_stream stream);
int uh_swap_f32(float* a, float* b, int64_t n, uh_stream stream);
/* The two other rules of the same pass (no counterpart in the reference; train.OptimConfig, --optimizer), with the conventions of
 * uh_rmsprop_step: coef = min(1, max_norm/(norm+1e-6)) from the device norm, g *= coef written back, nothing written when the
 * norm is not finite, 16-byte aligned buffers.  The _ema forms add the moving average of uh_rmsprop_step_ema and write the same
 * bits to p, g and the state as the plain forms.
 * uh_adamw_step: torch.optim.AdamW(amsgrad=False): m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g^2;
 * p = (p - lr*wd*p) - (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps), bc_i = 1 - b_i^t, t = steps[0] + 1.  steps is a DEVICE int32[1],
 * the number of updates applied so far (the step may be replayed from a captured graph); lr/bc1 and 1/sqrt(bc2) are formed in
 * double from the float32 betas and t and rounded to float32 once.  uh_ema_tick(steps, norm) advances it, once per optimizer
 * step, behind the step's launches.  lr, eps, weight_decay >= 0, betas in [0, 1).
 * uh_sgd_step: torch.optim.SGD(dampening=0): g += wd*p; buf = mu*buf + g; p -= lr * (nesterov ? g + mu*buf : buf).  A zero
 * buffer gives torch's first step.  lr, weight_decay, momentum >= 0; nesterov is 0 or 1 and needs momentum > 0. */
int uh_adamw_step(float* p, float* g, float* exp_avg, float* exp_avg_sq, int64_t n, const float* total_norm,
                  float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                  const int32_t* steps, uh_stream stream);
int uh_adamw_step_ema(float* p, float* g, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                      const float* total_norm, float max_norm, float lr, float beta1, float beta2, float eps,
                      float weight_decay, const int32_t* steps, float decay, int warmup, const int32_t* updates,
                      uh_stream stream);
int uh_sgd_step(float* p, float* g, float* momentum_buf, int64_t n, const float* total_norm, float max_norm, float lr,
                float weight_decay, float momentum, int nesterov, uh_stream stream);
int uh_sgd_step_ema(float* p, float* g, float* momentum_buf, float* ema, int64_t n, const float* total_norm,
                    float max_norm, float lr, float weight_decay, float momentum, int nesterov, float decay, int warmup,
                    const int32_t* updates, uh_stream stream);

/* ---- scalar assembly ------------------------------------------------------------------------
 * dice_coeff from per-group sums {sum x*t, sum x, sum t} (dice_score.py:14-25): out[0] = mean over
 * groups of (2I+eps)/(S+eps) with S := 2I where S == 0. */
int uh_dice_from_sums(const float* sums, int64_t ngroups, float eps, float* out, uh_stream stream);
/* train.py:121-134: out = { total, bce_mean, dice_loss, boundary } with
 * total = bce_mean + dice_loss + w_boundary*boundary[0]; sums from uh_bce_dice_sums. */
int uh_seg_loss_binary_finish(const float* sums, double n_mean, const float* boundary, float w_boundary,
                              float* out, uh_stream stream);
/* train.py:119-134 for one process in three launches instead of six (+ the torch glue between them): one pass over the
 * logits forms the BCE / Dice partial sums and the prediction's min / max (boundary_loss.py:28), the boundary counts follow,
 * one block finishes.  logits fp32 [B][H][W] dense, mask int64 class ids, target = mask / mask_div.
 * sums[0..3] as uh_bce_dice_sums writes them (uh_bce_dice_grad takes them); out[0..3] = { total, bce_mean, dice_loss,
 * boundary } as uh_seg_loss_binary_finish writes them, out[4] = 1.0 when total is NaN (train.py:149), else 0.0.
 * w_boundary == 0 skips the boundary term (out[3] = 0).  Bit-identical to the separate calls.  Data-parallel runs keep the
 * separate calls (the sums are all-reduced between them).  ws: uh_seg_loss_fused_ws_bytes(). */
size_t uh_seg_loss_fused_ws_bytes(void);
int uh_seg_loss_binary_fused(const float* logits, const int64_t* mask, int mask_div, int B, int H, int W, int edge_width,
                             float edge_weight, float smooth, float w_boundary, double n_mean, float* sums, float* out,
                             void* ws, size_t ws_bytes, uh_stream stream);
/* train.py:137-142: out = { total, ce_mean, dice_loss, boundary }, sums from uh_ce_dice_sums. */
int uh_seg_loss_multiclass_finish(const float* sums, int ncls, double n_mean, const float* boundary,
                                  float w_boundary, float* out, uh_stream stream);

/* ---- connected_component_loss, host part  (utils/connected_component_loss.py:20-59) -----------
 * masks: HOST uint8 [B][H][W], non-zero = (p > 0.5).  Restates cv2.findContours(RETR_EXTERNAL,
 * CHAIN_APPROX_SIMPLE) + cv2.contourArea + cv2.boundingRect (Suzuki-Abe outer borders, shoelace area).
 * out[0] = (sum of small-area and near-edge penalties) / B, out[1] = number of external contours.
 * PARITY UNPINNED (OpenCV is not available in this image). */
int uh_cc_loss_host(const uint8_t* masks, int B, int H, int W, int edge_distance, int min_area, double* out);
/* The same loss with the masks left on the device: hole filling + 8-connected components by union-find,
 * contourArea as the integer sum over 2x2 pixel blocks that the border polygon encloses (full squares + corner halves),
 * boundingRect by integer atomics; out = DEVICE double[2] {sum of penalties / B, number of external contours}. */
size_t uh_cc_loss_ws_bytes(int B, int H, int W);
int uh_cc_loss_device(const uint8_t* masks, int B, int H, int W, int edge_distance, int min_area, void* ws, size_t ws_bytes,
                      double* out, uh_stream stream);

/* ---- inference masks  (predict.py:27, evaluate.py:60-62,111) ------------------------------------
 * uh_argmax_classes: logits fp32 [npix][ncls] -> int64 index of the first maximum per pixel (torch.argmax(dim=1)).
 * uh_threshold_mask: binary head, out = (logit > 0) as 0.0/1.0  (== sigmoid(logit) > 0.5). */
int uh_argmax_classes(const float* logits, int64_t npix, int ncls, int64_t* out, uh_stream stream);
int uh_threshold_mask(const float* logits, int64_t n, float* out, uh_stream stream);

/* ---- mask post-processing on the device  (utils/post_process.py:51-88, used by evaluate.py:71-78) ----
 * mask / out: DEVICE uint8 [B][H][W] class indices {0,1,2}.  Hole filling of the class-2 foreground, k x k opening,
 * 8-connected components with fewer than min_area pixels removed; out is 2 for kept pixels and 0 elsewhere (the
 * reference zeroes the class-1 background too).  ws: uh_postprocess_ws_bytes() bytes.  PARITY UNPINNED (OpenCV). */
size_t uh_postprocess_ws_bytes(int B, int H, int W);
int uh_postprocess_masks(const uint8_t* mask, uint8_t* out, int B, int H, int W, int min_area,
                         int morph_kernel_size, void* ws, size_t ws_bytes, uh_stream stream);

/* ---- contour-distance metrics on the device  (no counterpart in the reference; DESIGN.md section 3 "Contour metrics") ----
 * For boolean H x W masks P (prediction) and T (truth):
 *   border S(M)  pixels of M with one of their four edge neighbours outside M; outside the image counts as outside M
 *   D_M[x]       min over q in S(M) of |x - q|^2, an exact integer in pixel units; 0xFFFFFFFF everywhere if S(M) is empty
 *   R            sqrt(D_T[p]) for every p in S(P) together with sqrt(D_P[q]) for every q in S(T), one multiset
 *   HD = max R, HD95 = numpy.percentile(R, 95) (linear interpolation), ASSD = mean R, IoU = |P & T| / |P | T|
 *   both masks empty: HD = HD95 = ASSD = 0, IoU = 1.  Exactly one empty: the distances are NaN, undefined = 1, IoU = 0.
 * Integer atomics only, fp64 sums in an order fixed by the image: the same bits on every call and in every batch.
 * H, W <= 32768 (squared distances are kept in 31 bits), H * W < 2^31; UH_EINVAL otherwise.
 * uh_mask_border_u8: out[b][y][x] = 1 on the border of (mask == cls), else 0.  DEVICE uint8 [B][H][W] both.
 * uh_edt_sq_u8: out_u32[b][y][x] = squared distance to the nearest NON-ZERO pixel of feature_u8 (DEVICE uint8 [B][H][W]),
 *   0xFFFFFFFF in an image without one.  Column scans, then a row pass over the row staged in LDS (W <= 4096; wider rows
 *   are searched in global memory and need the larger workspace that uh_edt_sq_ws_bytes reports).
 * uh_contour_metrics: P = (pred_u8 == cls_pred), T = (true_u8 == cls_true) per image of DEVICE uint8 [B][H][W] class maps;
 *   records_out: DEVICE uh_contour_record[B].  ws: uh_contour_metrics_ws_bytes() bytes, 16-byte aligned; it holds the
 *   per-image histogram over d^2 ((H-1)^2 + (W-1)^2 + 1 bins of uint32) and is cleared by the call. */
typedef struct uh_contour_record {
    uint32_t n_pred, n_true, n_inter, n_union;   /* |P|, |T|, |P & T|, |P | T| */
    uint32_t n_border_pred, n_border_true;       /* |S(P)|, |S(T)| */
    uint32_t n;                                  /* |R|: n_border_pred + n_border_true where defined, else 0 */
    uint32_t max_d2;                             /* max d^2 over R */
    uint32_t d2_lo, d2_hi;                       /* d^2 of the order statistics floor(v) and floor(v) + 1, v = 0.95 (n - 1) */
    uint32_t undefined;                          /* 1: exactly one of the masks is empty */
    uint32_t reserved;
    double weight;                               /* v - floor(v): HD95 interpolates sqrt(d2_lo) .. sqrt(d2_hi) by it */
    double sum_dist;                             /* sum over R of sqrt(d^2) */
    double hd, hd95, assd, iou;
} uh_contour_record;                             /* 96 bytes: 12 x uint32, then 6 x double */
int uh_mask_border_u8(const uint8_t* mask, int cls, uint8_t* out, int B, int H, int W, uh_stream stream);
size_t uh_edt_sq_ws_bytes(int B, int H, int W);
int uh_edt_sq_u8(const uint8_t* feature_u8, uint32_t* out_u32, int B, int H, int W, void* ws, size_t ws_bytes, uh_stream stream);
size_t uh_contour_metrics_ws_bytes(int B, int H, int W);
int uh_contour_metrics(const uint8_t* pred_u8, const uint8_t* true_u8, int cls_pred, int cls_true, uh_contour_record* records_out,
                       int B, int H, int W, void* ws, size_t ws_bytes, uh_stream stream);

/* ---- surface loss on the device  (no counterpart in the reference; DESIGN.md section 3 "Surface loss"; csrc/surface_loss.hip) ----
 * The distance-weighted surface loss of Kervadec et al., its maps built from the labels the step holds.  Per image b and
 * selected class c (classes: HOST int [K], distinct ids, 1 <= K <= 8) of DEVICE int64 labels mask [B][H][W]:
 *   T_c          (mask / mask_div == c), floor division: mask_div = 1 for a multi-class head, 2 for the binary head (BCE's target)
 *   S(T), D_T    border and exact squared distance as the contour metrics define them (uh_edt_sq_u8 runs over K * B images)
 *   phi_c[b,y,x] s * (float)sqrt((double)D_T[x]), s = -1 inside T_c, +1 outside; a border pixel is -0.0f; T_c empty in image b:
 *                phi_c[b] = +0.0f everywhere and the image has no gradient for that class
 *   surface      1 / (n_mean K) * sum_b sum_x sum_{c in C} p_c(x) phi_c(x), p = sigmoid(z) (ncls = 1) or softmax(z)_c (2 <= ncls <= 8)
 *   binary       dL/dz   = g w / n_mean * phi * sigma (1 - sigma), sigma = sigmoid(z)
 *   multi-class  dL/dz_k = g w / (n_mean K) * p_k * (phi_k [k in C] - sum_{c in C} p_c phi_c)
 * n_mean = pixel count of the mean (B H W of the GLOBAL batch when sharded); g = gscale[0], a device pointer (NULL = 1), as in
 * uh_bce_dice_grad.  Products and sums of the value in fp64, per-workgroup partials and a one-workgroup finish in a fixed order, no
 * floating-point atomics: the same bits on every call; a pixel's gradient depends on its own logits and its own image's labels only.
 * Limits: those of uh_edt_sq_u8 over K * B images (H, W <= 32768, H W < 2^31, K B <= 65535); UH_EINVAL otherwise, and for a null
 * pointer, K < 1, a class id outside [0, ncls) for a softmax head (any id >= 0 where there is no head; the sigmoid head takes
 * K = 1 and the id is a value of the target mask / mask_div, 1 for the foreground), ncls outside 1..8.
 * uh_surface_border_i64: border_out DEVICE uint8 [K][B][H][W] = 1 on S(T_k), all K classes in one launch, no uint8 copy of the labels.
 * uh_surface_dist_map:   phi_out DEVICE fp32 [K][B][H][W] (border, distance, map).
 * uh_surface_loss_sums:  logits fp32 [B][H][W] (ncls = 1) or [npix][ncls]; out[0] = surface, out[1] = w * surface (after a sum over
 *   data-parallel ranks they are the global batch's).  Leaves D in the workspace for uh_surface_loss_grad.
 * uh_surface_loss_grad:  WRITES dlogits (every element; autograd owns the sum over the loss nodes).  rebuild = 0: D is what
 *   uh_surface_loss_sums left in this workspace for the same labels and classes; rebuild != 0: border and distance are formed
 *   again first (another call used the workspace in between).  No fp32 map is written.
 * ws: uh_surface_loss_ws_bytes(B, H, W, K) bytes, 16-byte aligned: D, the border masks, the EDT's workspace and the partials. */
size_t uh_surface_loss_ws_bytes(int B, int H, int W, int K);
int uh_surface_border_i64(const int64_t* mask, int mask_div, const int* classes, int K, uint8_t* border_out, int B, int H, int W,
                          uh_stream stream);
int uh_surface_dist_map(const int64_t* mask, int mask_div, const int* classes, int K, float* phi_out, int B, int H, int W,
                        void* ws, size_t ws_bytes, uh_stream stream);
int uh_surface_loss_sums(const float* logits, const int64_t* mask, int mask_div, const int* classes, int K, int ncls, int B, int H,
                         int W, double n_mean, float w, float* out, void* ws, size_t ws_bytes, uh_stream stream);
int uh_surface_loss_grad(const float* logits, const int64_t* mask, int mask_div, const int* classes, int K, int ncls, int B, int H,
                         int W, double n_mean, float w, const float* gscale, float* dlogits, int rebuild, void* ws,
                         size_t ws_bytes, uh_stream stream);

/* ---- focal + Tversky loss  (no counterpart in the reference; DESIGN.md section 3 "Focal / Tversky loss"; csrc/focal_loss.hip) ----
 * The class-weighted replacement of the CE + Dice pair for imbalanced classes.  A head of C classes: ncls = 2..8 is a softmax
 * head (C = ncls, logits fp32 [npix][ncls], labels mask / mask_div); ncls = 1 is the one-channel head, the two-class form
 * (C = 2) on the logits (0, z): logits fp32 [npix], labels mask / mask_div (the binary loss's mask_div = 2).  With p = softmax:
 *   u        = sum_{c != t} p_c                                   (1 - p_t, formed without the cancellation)
 *   focal    = sum_x w_t u^gamma (-log p_t) / sum_x w_t           (-log p_t = logsumexp - z_t; gamma = 0: u^gamma = 1, also at u = 0)
 *   TI_c     = (TP_c + eps) / ((1 - alpha - beta) TP_c + alpha P_c + beta T_c + eps),  eps = 1e-6
 *   tversky  = 1 / K sum_{c in classes} (1 - TI_c);   total = focal + tversky
 * weights: HOST fp32 [C], each finite and > 0.  classes: HOST int [K], distinct ids in [0, C).  gamma >= 0; alpha, beta >= 0
 * with alpha + beta > 0.  UH_EINVAL for anything else, for ncls outside 1..8, a null pointer or a workspace that is too small.
 * uh_focal_tversky_nsums: the length of the sums vector, 2 + 3 C (0 for a bad ncls).
 * uh_focal_tversky_sums:  sums DEVICE fp32 [2 + 3 C] = { sum w_t u^gamma (-log p_t), sum w_t, TP_c.., P_c.., T_c.. }; after a sum
 *   over data-parallel ranks they are the global batch's, and value and gradient follow from them.  ws: uh_loss_ws_bytes(npix).
 * uh_focal_tversky_finish: out DEVICE fp32 [3] = { total, focal, tversky } from the sums, in double.
 * uh_focal_tversky_grad:   WRITES dlogits (every element) = gscale[0] * d total / d logits (gscale DEVICE or NULL = 1):
 *   w_t / W s (tau_k - p_k) + p_k (g_k - sum_c p_c g_c), s = gamma u^gamma q r - u^gamma, r = log(q) / u (-1 at u = 0).
 * No floating-point atomics: a call gives the same bits every time, and a pixel's gradient depends on its own logits and label,
 * the sums and gscale only.  u^gamma takes multiplications for gamma in {0, 1, 2}, exp2(gamma log2 u) otherwise. */
int uh_focal_tversky_nsums(int ncls);
int uh_focal_tversky_sums(const float* logits, const int64_t* mask, int mask_div, int64_t npix, int ncls, const float* weights,
                          float gamma, float* sums, void* ws, size_t ws_bytes, uh_stream stream);
int uh_focal_tversky_finish(const float* sums, int ncls, double alpha, double beta, const int* classes, int K, float* out,
                            uh_stream stream);
int uh_focal_tversky_grad(const float* logits, const int64_t* mask, int mask_div, int64_t npix, int ncls, const float* weights,
                          float gamma, double alpha, double beta, const int* classes, int K, const float* sums, const float* gscale,
                          float* dlogits, uh_stream stream);

/* ---- knowledge distillation  (no counterpart in the reference; DESIGN.md section 3 "Distillation"; csrc/distill_loss.hip) ----
 * The KL term between a teacher's and the student's temperature-softened class probabilities (Hinton et al.).  student, teacher:
 * DEVICE fp32 logits of the same head, [npix][ncls] for a softmax head (ncls = 2..8) or [npix] for the one-channel head
 * (ncls = 1), which is the two-class form on (0, z) and (0, v).  No labels.  With temperature T > 0, weight w > 0, n_mean the
 * pixel count of the mean (that of the GLOBAL batch when sharded), q = softmax(teacher / T) and p = softmax(student / T):
 *   kd       = T^2 / n_mean * sum_x sum_c q_c (log q_c - log p_c)
 *   agree    = 1 / n_mean * sum_x [argmax student = argmax teacher]   (first maximum; a diagnostic without gradient)
 * Per pixel the KL is formed from the shifted, scaled logits a_c = (v_c - max v) * (1 / T), b_c = (z_c - max z) * (1 / T) as
 * sum_c q_c (a_c - b_c) - (log1p(rest_v) - log1p(rest_z)), the same instructions on both tensors: q_c = 0 contributes an exact 0,
 * student == teacher gives kd = 0.0 and a gradient of +0.0 exactly, and nothing overflows at logits of magnitude 100.
 * UH_EINVAL before any launch for a null pointer, ncls outside 1..8, npix < 1, a non-finite or non-positive T, w or n_mean, or a
 * workspace that is too small.
 * uh_distill_nsums:  the length of the sums vector, 2.
 * uh_distill_sums:   sums DEVICE fp32 [2] = { sum_x KL, sum_x agree } of this call's pixels; after a sum over data-parallel ranks
 *   they are the global batch's.  ws: uh_loss_ws_bytes(npix).
 * uh_distill_finish: out DEVICE fp32 [3] = { w kd, kd, agree } from the sums and n_mean, in double.
 * uh_distill_grad:   WRITES dlogits (every element, the student's layout) = gscale[0] * w T / n_mean * (p - q) (gscale DEVICE or
 *   NULL = 1); the one-channel head gets the k = 1 component.  The component of the student's largest class is formed as
 *   minus the sum of the others (sum_c (p_c - q_c) = 0), which keeps its digits where both sides are sure of that class.
 * No floating-point atomics: a call gives the same bits every time, and a pixel's gradient depends on its own two logit vectors,
 * n_mean, T, w and gscale only. */
int uh_distill_nsums(void);
int uh_distill_sums(const float* student, const float* teacher, int64_t npix, int ncls, double T, float* sums, void* ws,
                    size_t ws_bytes, uh_stream stream);
int uh_distill_finish(const float* sums, double n_mean, double T, double w, float* out, uh_stream stream);
int uh_distill_grad(const float* student, const float* teacher, int64_t npix, int ncls, double n_mean, double T, double w,
                    const float* gscale, float* dlogits, uh_stream stream);

/* ---- input pipeline, device stage (utils/data_loading.py:65-132, train.py:113-114) ---------------------------
 * What BasicDataset.__getitem__ does to a DECODED image / mask pair, for a whole batch in one pass:
 *   img_u8   DEVICE uint8 [B][Hin][Win][C] (C = 1..4, what np.asarray(PIL image) holds), or NULL (masks only)
 *   mask_u8  DEVICE uint8 [B][Hin][Win] grey levels (255 contour / 128 background / 0 ghost), or NULL (images only)
 *   turns    DEVICE int [B]: quarter turns counter-clockwise of item b (index % 4 of the x4 augmentation,
 *            data_loading.py:100-121), or NULL = no rotation.  odd_turns = 1 when the items' turn counts are odd (every
 *            item of a batch must have the same output shape: Hin x Win for even counts, Win x Hin for odd ones; square
 *            images may mix them: pass odd_turns = 0)
 *   image_out  NHWC [B][Ho][Wo][ld_out >= C] in dt (UH_F32 / UH_BF16): u / 255 when the IMAGE holds a value above 1, else
 *              the raw 0 / 1 value (data_loading.py:86-87); channels C..ld_out-1 are not written
 *   labels_out int64 [B][Ho][Wo]: 255 -> 2, 128 -> 1, anything else -> 0 (data_loading.py:74-78)
 *   flags_ws   DEVICE int [B] workspace (per-image "holds a value above 1")
 * Decode stays on the host; the BICUBIC / NEAREST rescale of scale < 1 is uh_batch_rescale_u8, run before this call. */
int uh_batch_prepare(const uint8_t* img_u8, int C, const uint8_t* mask_u8, const int* turns, int odd_turns, void* image_out,
                     int ld_out, int64_t* labels_out, int* flags_ws, int B, int Hin, int Win, int dt, uh_stream stream);
/* uh_batch_rescale_u8: the dataset's rotate + rescale at scale < 1 (data_loading.py:66-70, 100-121), Pillow's bytes exactly:
 *   img_out  = _rescaled(_quarter_turn(img, t), s, BICUBIC)   DEVICE uint8 [B][out_h][out_w][C], C = 1 or 3
 *   mask_out = _rescaled(_quarter_turn(mask, t), s, NEAREST)  DEVICE uint8 [B][out_h][out_w]
 *   of img_u8 DEVICE uint8 [B][Hin][Win][C] / mask_u8 DEVICE uint8 [B][Hin][Win] (either may be null), turns / odd_turns as
 *   uh_batch_prepare.  The tables describe the ROTATED size Hr x Wr (Win x Hin when odd_turns) and are built on the host:
 *   h_bounds / h_coef [out_w][2] / [out_w][kh] and v_bounds / v_coef [out_h][2] / [out_h][kv] as uh_resample_lanczos_u8
 *   (bicubic filter; the horizontal pass covers rotated rows [row0, row0 + nrows), vertical bounds relative to row0);
 *   span >= the source pixels any 64 consecutive output columns read (xmin of the last + taps - xmin of the first);
 *   x_index [out_w] / y_index [out_h]: Pillow's NEAREST source column / row of every output pixel.
 *   ws: uh_batch_rescale_ws_bytes(B, C, nrows, out_w) bytes (the uint8 intermediate of the two passes). */
size_t uh_batch_rescale_ws_bytes(int B, int C, int nrows, int out_w);
int uh_batch_rescale_u8(const uint8_t* img_u8, int C, const uint8_t* mask_u8, const int* turns, int odd_turns, int B, int Hin,
                        int Win, const int* h_bounds, const int* h_coef, int kh, int span, int out_w, const int* v_bounds,
                        const int* v_coef, int kv, int out_h, int row0, int nrows, const int* x_index, const int* y_index,
                        uint8_t* img_out, uint8_t* mask_out, void* ws, size_t ws_bytes, uh_stream stream);

/* ---- training augmentation of a prepared batch  (no counterpart in the reference; DESIGN.md section 3 "Training
 * augmentation").  One launch maps what uh_batch_prepare wrote to a new batch of the same shape and dtype:
 *   image_in   DEVICE NHWC [B][H][W][ld_in >= C] in dt (UH_F32 / UH_BF16), C = 1..4, or NULL (labels only)
 *   labels_in  DEVICE int64 [B][H][W], or NULL (images only)
 *   params     DEVICE uh_augment_params [B], one row per item, built on the host (utils/augment.py):
 *     m[6]       the inverse affine map in Q32 (value * 2^32, rounded to nearest): the source CENTRE coordinate of output
 *                pixel (x, y) is  sx = m[0] (x + 0.5) + m[1] (y + 0.5) + m[2],  sy = m[3] (x + 0.5) + m[4] (y + 0.5) + m[5],
 *                evaluated exactly in int64 and rounded to Q16 (half up); pixel i covers [i, i + 1).  Labels take the pixel
 *                that contains (sx, sy); the image is bilinear at (sx - 0.5, sy - 0.5) with 16-bit weights, in fp32:
 *                top = p00 + wx (p01 - p00), bot = p10 + wx (p11 - p10), v = top + wy (bot - top), no fused multiply-add,
 *                a zero weight taking the pixel itself.  |m[i]| < 2^48 (addresses stay inside the image whatever the table holds).
 *     gamma, contrast, brightness, noise_std   image only, after the geometry, in this order: v = clamp(v, 0, 1)^gamma,
 *                v = (v - 0.5) contrast + 0.5, v = v + brightness, v = v + noise_std z, then clamp to [0, 1].  A stage whose
 *                parameter is neutral (1, 1, 0, 0) is skipped; with all four neutral there is no clamp either.
 *     key[2]     Philox4x32-10 key of the item's noise: element e = (y W + x) C + c takes normal number e & 3 of the block
 *                with counter (e >> 2, 0, 0, 1); words (0, 1) and (2, 3) are Box-Muller pairs, radius from
 *                u = (r + 0.5) 2^-32, angle 2 pi r 2^-32, cosine first.
 *   border     UH_AUG_CLAMP: source indices are clamped to the image (image and labels);
 *              UH_AUG_FILL: a source pixel outside the image is fill_image, a label outside is fill_label
 *   image_out / labels_out   same shapes (pixel stride ld_out >= C), not the inputs.  bf16 is computed in fp32 and rounded once.
 * H, W <= 16384 and H W C < 2^32. */
enum { UH_AUG_CLAMP = 0, UH_AUG_FILL = 1 };
typedef struct uh_augment_params {
    int64_t m[6];
    float gamma, contrast, brightness, noise_std;
    uint32_t key[2];
} uh_augment_params;                             /* 72 bytes: 6 x int64, 4 x float, 2 x uint32 */
int uh_batch_augment(const void* image_in, int ld_in, const int64_t* labels_in, const uh_augment_params* params, void* image_out,
                     int ld_out, int64_t* labels_out, int B, int H, int W, int C, int dt, int border, float fill_image,
                     int fill_label, uh_stream stream);
/* uh_batch_augment_elastic: uh_batch_augment with an elastic deformation (DESIGN.md section 3 "Elastic deformation"): a cubic
 * B-spline displacement field is added to the Q16 source position q of the affine walk, evaluated at the OUTPUT pixel; from
 * q' = q + displacement on everything is uh_batch_augment (labels, bilinear image, borders, photometry, noise).
 *   grid      control-point spacing in pixels, a multiple of 16 in [16, 256]; GW = ceil(W / grid) + 3, GH = ceil(H / grid) + 3
 *   control   DEVICE int32 [B][GH][GW][2]: (dx, dy) of every control point in Q16 pixels, control point k of an axis at
 *             position (k - 1) grid.  Values are clamped to |d| < 2^22 on load.
 *   weights   DEVICE int32 [grid][4], 16-byte aligned: row n the uniform cubic B-spline basis at t = (n + 0.5) / grid in Q20,
 *             every row summing to 2^20 (utils/augment.py: elastic_weights).  Values are clamped to [0, 2^20] on load.
 *   With cx = x / grid, nx = x % grid, cy = y / grid, ny = y % grid, per component, in int64 with arithmetic shifts:
 *     r_k = (sum_j weights[nx][j] control[cy + k][cx + j] + 2^19) >> 20   (k = 0..3),
 *     displacement = (sum_k weights[ny][k] r_k + 2^19) >> 20.
 *   Source addresses stay inside the image whatever the tables hold. */
int uh_batch_augment_elastic(const void* image_in, int ld_in, const int64_t* labels_in, const uh_augment_params* params,
                             const int32_t* control, const int32_t* weights, int grid, void* image_out, int ld_out,
                             int64_t* labels_out, int B, int H, int W, int C, int dt, int border, float fill_image, int fill_label,
                             uh_stream stream);

/* ---- RAW -> contour pipeline, non-inference stages  (seg_main.py; utils/raw2png.py, png_normalize.py, png_denormalize.py,
 * mask2polygon.py).  Batched over B images of one geometry.
 *
 * uh_window_u16: raw2png.py:_apply_windowing.  raw DEVICE uint16 [n] (16-byte aligned), out DEVICE uint8 [n] (8-byte aligned):
 *   mn = WL - WW/2, mx = WL + WW/2, out = trunc(double(clamp(x, mn, mx) - mn) / double(mx - mn) * 255.0), in IEEE double.
 *   WW < 2 is refused (the reference divides 0 by 0). */
int uh_window_u16(const uint16_t* raw, int64_t n, int window_length, int window_width, uint8_t* out, uh_stream stream);
/* uh_resample_lanczos_u8: Pillow's 8-bit two-pass resample (Image.resize(..., LANCZOS)) of the box (box_x, box_y, box_w,
 *   box_h) of src DEVICE uint8 [B][Hs][Ws], written at (px, py) into dst DEVICE uint8 [B][Hd][Wd], every other dst pixel 0.
 *   lut: DEVICE uint8 [256] applied to each source byte first (identity, or class index -> grey level).
 *   h_bounds / v_bounds: DEVICE int [out_w][2] / [out_h][2] {first tap, number of taps}; h_coef / v_coef: DEVICE int
 *   [out_w][kh] / [out_h][kv] 22-bit fixed-point weights (Resample.c precompute_coeffs + normalize_coeffs_8bpc, built on the
 *   host).  Horizontal bounds are relative to box_x; the horizontal pass runs over box rows [row0, row0 + nrows) into ws,
 *   and vertical bounds are relative to row0.  kh <= 128.  ws: uh_resample_ws_bytes(B, nrows, out_w) bytes. */
size_t uh_resample_ws_bytes(int B, int nrows, int out_w);
int uh_resample_lanczos_u8(const uint8_t* src, int B, int Hs, int Ws, int box_x, int box_y, int box_w, int box_h,
                           const uint8_t* lut, const int* h_bounds, const int* h_coef, int kh, int out_w,
                           const int* v_bounds, const int* v_coef, int kv, int out_h, int row0, int nrows,
                           uint8_t* dst, int Hd, int Wd, int px, int py, void* ws, size_t ws_bytes, uh_stream stream);
/* External contours of (grey > 127): cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) as OpenCV's icvFetchContour
 * traces them, PARITY UNPINNED (OpenCV is not available here).  grey: DEVICE uint8 [B][H][W]; B <= 1024 and B*H*roundup(W,16)
 * < 2^31.  ws: uh_contours_ws_bytes() bytes, 16-byte aligned, kept between the two calls.
 * uh_contours_count fills info: DEVICE int [3 + 2B + 1] = {total contours, total points, error flags, ncont[B], first
 *   contour of each image [B + 1]}, and npts: DEVICE int [uh_contours_max()] points per contour, contours ordered
 *   image-major and, within an image, in cv2's list order (reverse raster order of the start pixels).
 * uh_contours_emit writes the points, int32 {x, y} pairs (8-byte aligned), contour after contour in the same order;
 *   max_points = capacity in points (>= info[1]).  info[2] != 0 after either call = an inconsistent walk (a bug). */
size_t uh_contours_ws_bytes(int B, int H, int W);
size_t uh_contours_max(int B, int H, int W);
int uh_contours_count(const uint8_t* grey, int B, int H, int W, void* ws, size_t ws_bytes, int* info, int* npts,
                      uh_stream stream);
int uh_contours_emit(void* ws, size_t ws_bytes, int B, int H, int W, int* info, const int* npts, int* points,
                     int64_t max_points, uh_stream stream);

/* ---- predict.py / evaluate.py PNG dumps: the byte stages around the eval forward  (csrc/predict_io.hip) -------------
 * uh_predict_prepare_u8: the image branch of BasicDataset.preprocess at scale 1 for a batch of decoded grey images of one
 *   size (data_loading.py:86-87, predict.py:19-20): img_u8 DEVICE uint8 [B][H][W] -> image_out DEVICE float32 [B][1][H][W];
 *   an image that holds a byte > 1 becomes u / 255 (the correctly rounded fp32 quotient numpy computes), any other image keeps
 *   its raw 0.0 / 1.0.  The test is made per image on the device; flags_ws: DEVICE int [B] workspace.
 * uh_logits_to_classes_u8: argmax over the classes, straight to one byte per pixel: logits [npix][ncls] (the head's NHWC
 *   view) in dt (UH_F32 / UH_BF16) -> classes_out DEVICE uint8 [npix]; first maximum, a NaN counts as the maximum (the rule
 *   of uh_argmax_classes).  ncls <= 256.
 * uh_classes_to_grey_u8: grey_out[i] = lut[classes[i]] for n bytes, lut DEVICE uint8 [256]; grey_out may be classes
 *   (in place).  The reference's tables: predict.py:52-58 / evaluate.py:150-154 (0, 128, 255), evaluate.py:160-163
 *   (post-processed: 2 -> 255, everything else 0), evaluate.py:96-97,103-105 (binary head: 1 -> 255). */
int uh_predict_prepare_u8(const uint8_t* img_u8, float* image_out, int* flags_ws, int B, int H, int W, uh_stream stream);
int uh_logits_to_classes_u8(const void* logits, int64_t npix, int ncls, int dt, uint8_t* classes_out, uh_stream stream);
int uh_classes_to_grey_u8(const uint8_t* classes, uint8_t* grey_out, const uint8_t* lut, int64_t n, uh_stream stream);

/* ---- test-time augmentation around the eval forward  (csrc/tta.hip; the reference has none) ---------------------------
 * A view is v = 4 t + 2 fy + fx, "flip, then transpose": a source pixel (y, x) of an H x W image lies in view v at (yy, xx)
 * for t = 0 and at (xx, yy) of a W x H view for t = 1, with yy = fy ? H-1-y : y and xx = fx ? W-1-x : x.  mask: the views
 * of a mode as bits over v, one of 0x03 (hflip), 0x0f (flips), 0x69 (rot4: the quarter turns), 0xff (d4); K0 / K1 = its
 * number of t = 0 / t = 1 views, V = K0 + K1.
 * uh_tta_views: x DEVICE float32 [B][H][W][C] (C <= 8) -> views0 [K0 B][H][W][C], the t = 0 views in ascending v, view-major
 *   (entry k B + b), and views1 [K1 B][W][H][C], the t = 1 views likewise (may be null when K1 = 0).  A pure copy.
 * uh_tta_merge: logits0 [K0 B][H][W][NC] and logits1 [K1 B][W][H][NC] (null when K1 = 0), the logits of those views in dt
 *   (UH_F32 / UH_BF16).  Per source pixel and view: the fp32 softmax over the classes (NC = 1: the sigmoid) of the logits at
 *   the pixel's position in the view, quantised as q = (uint32) rintf(p * 2^24); the q of all views are added as integers, so
 *   the result does not depend on the order of the views.  Outputs, each nullable (one at least): sums uint32 [B][H][W][NC];
 *   classes uint8 [B][H][W], the first maximum of the sums (NC = 1: sum > V 2^23, the averaged sigmoid > 0.5); probs float32
 *   [B][H][W][NC] = sum / (V 2^24), exact.  1 <= NC <= 256; B <= 65535. */
int uh_tta_views(const float* x, float* views0, float* views1, int B, int H, int W, int C, int mask, uh_stream stream);
int uh_tta_merge(const void* logits0, const void* logits1, int dt, int B, int H, int W, int NC, int mask, unsigned int* sums,
                 uint8_t* classes, float* probs, uh_stream stream);

/* ---- sliding-window tiled prediction  (csrc/tiling.hip; the reference has none) ----------------------------------------
 * Config: size, the tile side, a multiple of 16 in [16, 1024]; overlap, 0 <= overlap <= size / 2.  Per axis of length L the
 * tile length is t = min(size, L) (no padding); L <= size: one tile at origin 0; otherwise the stride is S = size - overlap,
 * there are n = ceil((L - size) / S) + 1 tiles and tile k starts at o_k = min(k S, L - size), so a position lies in at most 3
 * tiles of an axis.  Position i of a tile has the weight w(i) = max(1, min(i + 1, t - i, overlap)); a tile's weight at a pixel
 * is wy wx <= 2^18.  ny, nx: the tile counts of an H x W image; th = min(size, H), tw = min(size, W): its tile shape.
 * uh_tile_grid: host only, no launch.  Fills *ny, *nx, *th, *tw and the origins oy[ny], ox[nx]; every output may be null
 *   (ask for the counts first).  UH_EINVAL for a bad config or H, W < 1.
 * uh_tile_gather: x DEVICE float32 [B][H][W][C] (C <= 8; the output of uh_predict_prepare_u8 for the WHOLE images) -> tiles
 *   [B ny nx][th][tw][C], image-major, then row-major over the grid.  A pure copy, one launch for the batch.
 * uh_tile_merge: src [B ny nx][th][tw][NC], the tiles' results: kind UH_F32 / UH_BF16 = logits, quantised per tile pixel as
 *   uh_tta_merge quantises a view (q = (uint32) rintf(p 2^24), p the fp32 softmax, NC = 1: the sigmoid; the same device
 *   function), views = 1; kind UH_TILE_SUMS_I32 = the int32 sums of uh_tta_merge over `views` (1, 2, 4 or 8) views, < 2^28.
 *   Per image pixel the covering tiles' wy wx q are added in 64-bit integers (< 9 2^18 2^27 < 2^49): no atomics, no float in a
 *   sum, the result is bit-reproducible.  Outputs, each nullable (one at least): sums uint64 [B][H][W][NC]; den uint32
 *   [B][H][W] = the sum of wy wx; classes uint8 [B][H][W], the first maximum of the sums (NC = 1: 2 sum > den views 2^24);
 *   probs float32 [B][H][W][NC] = (float)((double) sum / ((double) den views 2^24)).  1 <= NC <= 256; B <= 65535.
 * Null or misaligned pointers, a bad kind, views or config: UH_EINVAL before any launch. */
enum { UH_TILE_SUMS_I32 = 3 };
int uh_tile_grid(int H, int W, int size, int overlap, int* ny, int* nx, int* th, int* tw, int* oy, int* ox);
int uh_tile_gather(const float* x, float* tiles, int B, int H, int W, int C, int size, int overlap, uh_stream stream);
int uh_tile_merge(const void* src, int kind, int views, int B, int H, int W, int NC, int size, int overlap,
                  unsigned long long* sums, unsigned int* den, uint8_t* classes, float* probs, uh_stream stream);

/* ---- checkpoint ensembles  (csrc/ensemble.hip; the reference has none) -------------------------------------------------
 * The members' results are added per pixel and class as integers, each member with an integer weight; the work has no
 * geometry, so every array is flat: [npix][NC], logits through the head's NHWC view.
 * uh_ensemble_add: acc uint64 [npix][NC]; first != 0: acc[i] = weight s[i] (the accumulator needs no memset), first == 0:
 *   acc[i] += weight s[i].  kind says what src holds: UH_F32 / UH_BF16 = a member's logits, s = q = (uint32) rintf(p 2^24), p the
 *   fp32 softmax over the classes (NC = 1: the sigmoid) -- the device functions uh_tta_merge and uh_tile_merge quantise with,
 *   so the same logits give the same q in all three; UH_TILE_SUMS_I32 = the uint32 sums of uh_tta_merge; UH_ENS_SUMS_U64 = the
 *   uint64 sums of uh_tile_merge.  No atomics, no float after the quantisation: the result depends on no order of the members.
 *   1 <= NC <= 256, 1 <= weight <= 1024, npix < 2^40.
 * uh_ensemble_finish: per pixel T = den[pix] views 2^24 total_weight (den null: 1; views 1, 2, 4 or 8; 1 <= total_weight
 *   <= 1024).  Outputs, each nullable (one at least): classes uint8 [npix], the first maximum of acc over the classes (NC = 1:
 *   2 acc > T); probs float32 [npix][NC] = (float)((double) acc / (double) T); confidence uint8 [npix] = floor(255 max_c acc[c] /
 *   sum_c acc[c]), 0 where the sum is 0 (NC = 1: floor(255 max(a, T - a) / T) with a = min(acc, T)).
 * Bound: a member's tile sums stay below 2^49 with their views included (above), so acc < 2^49 total_weight <= 2^59 and
 *   T < 2^22 2^3 2^24 2^10 = 2^59: every sum and 2 acc fit in 64 bits.  255 acc fits only while den views total_weight < 2^32;
 *   the confidence is formed by a restoring division that never holds 255 acc, so it is exact over the whole range.
 * Null or misaligned pointers (acc 8 bytes; src, den, probs their element), a bad kind, views, weight, total_weight or NC:
 * UH_EINVAL before any launch. */
enum { UH_ENS_SUMS_U64 = 4 };
int uh_ensemble_add(const void* src, int kind, int64_t npix, int NC, unsigned weight, int first, unsigned long long* acc,
                    uh_stream stream);
int uh_ensemble_finish(const unsigned long long* acc, const unsigned int* den, int views, unsigned total_weight, int64_t npix,
                       int NC, uint8_t* classes, float* probs, uint8_t* confidence, uh_stream stream);

/* ---- patch training: seeded foreground-aware crops  (csrc/crop.hip; the reference has none) ---------------------------
 * One square crop of side `size` (a multiple of 16, >= 16) per item.  The item table is HOST memory, one row per item, and the
 * items may differ in size (1 <= H, W <= 16384, both >= size): every row is checked before any launch and the rows travel
 * by value in the kernel arguments, so no call copies, allocates or synchronises with the host.  r[0..3] are the item's four
 * random words.  With ny = H - size + 1, nx = W - size + 1 and n the number of pixels whose label v has bit v of class_mask
 * set (labels outside 0..63 never count):
 *   foreground branch, iff n > 0 and r[0] < fg_threshold (0 .. 2^32):  k = (r[1] n) >> 32, (py, px) the k-th such pixel in
 *     raster order, jy = (r[2] size) >> 32, jx = (r[3] size) >> 32, oy = clamp(py - jy, 0, ny - 1), ox = clamp(px - jx, 0, nx - 1);
 *   uniform branch, otherwise:  oy = (r[2] ny) >> 32, ox = (r[3] nx) >> 32.
 * uh_crop_select: origin DEVICE int32 [B][2] = (oy, ox); count DEVICE uint32 [B] = n, nullable; ws DEVICE, at least
 *   uh_crop_select_ws_bytes(B) bytes, 4-byte aligned.  Two launches per 32 rows, no atomics; `image` and `ld` are not read.
 * uh_crop_gather: image_out [B][size][size][ld_out] in dt (UH_F32 / UH_BF16) and labels_out int64 [B][size][size], each nullable
 *   (one at least; without image_out the rows' `image` may be null): the bits of [oy, oy + size) x [ox, ox + size) of every
 *   item, C channels (1 .. 4) of a pixel.  The origin is clamped into [0, H - size] x [0, W - size] as it is loaded, so no source
 *   address leaves its item whatever the table holds.  Sources need the alignment of their element only.
 * Null or misaligned pointers, a bad size, C, stride, dtype or threshold, a row smaller than `size` or a short workspace:
 * UH_EINVAL before any launch. */
typedef struct uh_crop_item {
    const void* image;                 /* DEVICE NHWC [H][W][ld] in dt, or NULL (labels only) */
    const int64_t* labels;             /* DEVICE int64 [H][W] */
    int H, W, ld, reserved;
    uint32_t r[4];
} uh_crop_item;
size_t uh_crop_select_ws_bytes(int B);
int uh_crop_select(const uh_crop_item* items, int B, int size, uint64_t class_mask, uint64_t fg_threshold, int32_t* origin,
                   uint32_t* count, void* ws, size_t ws_bytes, uh_stream stream);
int uh_crop_gather(const uh_crop_item* items, int B, int C, int dt, int size, const int32_t* origin, void* image_out, int ld_out,
                   int64_t* labels_out, uh_stream stream);

/* ---- device-resident dataset cache: cut a batch from cached entries  (csrc/cache.hip; the reference has none) ---------------
 * uh_cache_gather_u8: image_out DEVICE uint8 [B][image_bytes] and mask_out DEVICE uint8 [B][mask_bytes], both contiguous, each
 *   nullable (one at least): item b of an output is a copy of the image_bytes (mask_bytes) bytes at row b's pointer.  Rows may
 *   repeat and come in any order.  The item table is HOST memory, one row per batch item: every row is checked before any
 *   launch and the rows travel by value in the kernel arguments, 32 per launch, so no call copies to the device, allocates or
 *   synchronises with the host.  Without image_out (mask_out) the rows' `image` (`mask`) may be null and its length is not read.
 * Sources: every pointer is 16-byte aligned and READABLE UP TO ITS LENGTH ROUNDED UP TO 16: the kernel reads whole aligned
 *   16-byte units, so it may read up to 15 bytes of padding behind a source and nothing beyond them.  The cache pads every
 *   entry of its arena to a multiple of 16 bytes to guarantee this (utils/dataset_cache.py, plan_entries).
 * Destinations: the output bases are 16-byte aligned; item b starts at b * bytes, aligned or not.  Any length >= 1 (at most
 *   2^40) is copied exactly: no byte outside [out, out + B * bytes) is written.  Aligned 16-byte units of a destination are
 *   written with 16-byte stores, the fewer than 16 bytes in front of and behind them one by one.
 * Null or misaligned pointers, B < 1, both outputs null, or a zero length with a non-null output: UH_EINVAL before any launch. */
typedef struct uh_cache_item {
    const uint8_t* image;              /* DEVICE uint8 [image_bytes], 16-byte aligned, padded to a multiple of 16; or NULL */
    const uint8_t* mask;               /* DEVICE uint8 [mask_bytes], likewise */
} uh_cache_item;
int uh_cache_gather_u8(const uh_cache_item* items, int B, size_t image_bytes, size_t mask_bytes, uint8_t* image_out,
                       uint8_t* mask_out, uh_stream stream);

#ifdef __cplusplus
}
#endif
#endif
