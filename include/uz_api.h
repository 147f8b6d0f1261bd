/*
 * uz_api.h - C ABI of libuz_hip.so: the MI355X (gfx950) implementation of the
 * U-Net / PHiSeg / Probabilistic-U-Net forward+backward hot path of
 * gigantenbein/UNet-Zoo.
 *
 * The reference has NO native / FFI boundary of its own: the path
 * sits behind Python nn.Module classes that dispatch ATen ops.  Each entry point
 * below therefore replaces one ATen call site of the reference; the call site
 * it replaces is cited (file:line relative to the reference repository).
 *
 * Conventions
 *  - plain C, no torch types: device pointers + sizes.  Tensors are fp32 NCHW.
 *    A tensor argument is a *channel-slice view*: `ptr` points at channel 0 of
 *    the view, `C` is the number of channels of the view and `Ctot` the channel
 *    count of the underlying buffer (batch stride = Ctot*H*W floats).  Writing a
 *    producer's output at a channel offset of a wider buffer is how torch.cat
 *    (phiseg.py:71,315; unet.py:72) is eliminated.
 *  - every call is asynchronous on the given hipStream_t (passed as void*); no
 *    call synchronises the device or allocates device memory.
 *  - return 0 on success, <0 on error; uz_last_error() gives the message
 *    (thread local, valid until the next call on that thread).
 *  - `accumulate != 0` means dst += result (gradient fan-in), else dst = result.
 */
#ifndef UZ_API_H
#define UZ_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UZ_VERSION 100

int         uz_version(void);
const char* uz_last_error(void);
/* number of MI355X compute units / device name of the current device (diagnostics) */
int         uz_device_info(int* n_cu, char* name, int name_cap);

/* ---------------------------------------------------------------- convolution
 * nn.Conv2d(k=3, stride 1, pad 1) / nn.Conv2d(k=1): torchlayers.py:18, unet.py:25-29,
 * phiseg.py:95-96,281-284, probabilistic_unet.py:95,156-163.  w is the PyTorch
 * parameter itself, layout [Cout][Cin][ks][ks]; bias may be NULL.
 * fp32 in, fp32 out, fp32 accumulation everywhere.  Two implicit-GEMM kernel families:
 *  - fp32 MFMA (v_mfma_f32_32x32x2_f32) for every shape, including the 1..3-channel image /
 *    latent inputs (channel tiles are zero padded in LDS); 1x1 heads with <= 8 outputs run on
 *    streaming VALU kernels instead;
 *  - for the large 3x3 layers, the fp16 matrix pipe with split operands (each fp32 value, scaled by a power of two,
 *    = two fp16 pieces of 11 significand bits; three piece products, fp32 accumulate: split_f16.h, conv_split.hip,
 *    conv_wgrad_split.hip) - 22-bit operands (per layer within 2x the error of the fp32-MFMA kernels against fp64 (measured 0.5 - 0.8x on the heaviest layer); end to end at batch 32 the gradients' median error against fp64 is 1.6x the fp32 reference's own, logits within 1e-4, argmax bit-equal: tests/test_full_configs_gpu.py, tests/test_phiseg_gpu.py).  Environment switch, read once per process:
 *    UZ_CONV_MATH=f32 (fp32 MFMA only) | split (split path on every eligible 3x3 shape) | unset.
 *    The forward / data-gradient split path keeps its packed weight image in `workspace`.
 * Deep, low-resolution levels (2x2 .. 16x16) cannot fill 256 CUs with output tiles alone: with a
 * workspace of uz_conv_workspace() bytes the input-channel loop is split over workgroups and summed
 * in a fixed order (bitwise reproducible); workspace may be NULL (no split, slower, same result up
 * to summation order).                                                                          */
/* run-time override of UZ_CONV_MATH for tests / diagnostics: -1 = environment, 0 = f32, 1 = default policy (fp32-accurate fp16
 * split where it pays), 2 = split on every eligible shape, 3 = bf16: the layers of mode 1 with one bf16 piece per operand and one
 * MFMA product, fp32 accumulation (bf16 arithmetic, fp32 storage; BASELINE configs[4] is quoted in bf16).  Workspace sizes depend
 * on the mode: query them after switching.  Not thread safe.                                                            */
int uz_set_conv_math(int mode);
int uz_get_conv_math(void);
/* kernel family a call takes under the current mode: kind 0 fwd / 1 bwd_data / 2 bwd_weight -> 0 fp32 MFMA, 1 split-fp16 MFMA,
 * 2 streaming VALU (1x1 heads with 1, 2, 3, 4, 6 or 8 outputs and Cin <= 512: uz_heads_route).  Used by bench.py to price each op. */
int uz_conv_route(int kind, int Cin, int Cout, int N, int H, int W, int ks);
size_t uz_conv_workspace(int Cin, int Cout, int N, int H, int W, int ks);   /* covers fwd and bwd_data */
/* Magnitude bounds (`*_amax`, all nullable): device scalars holding an UPPER BOUND of max|tensor| (any bound within ~2^10 of
 * the true maximum keeps full accuracy).  The split-fp16 kernels scale their operands by a power of two derived from the bound
 * before splitting them into fp16 pieces; NULL makes the call measure the tensor itself (one extra pass - the stand-alone
 * path; the model plans pass bounds that the producing kernels maintain: y_amax / a_amax / dy_amax outputs below are
 * atomic-max accumulated into a slot the caller zeroes once per pass).  The fp32-MFMA kernels ignore the input bounds.   */
int uz_conv_fwd(const float* x, int Cin, int CinTot,
                const float* w, const float* bias,
                float* y, int Cout, int CoutTot,
                int N, int H, int W, int ks, int relu,
                const float* x_amax, const float* w_amax, float* y_amax,
                void* workspace, size_t workspace_bytes, void* stream);
/* Weight images of the split path packed ONCE per step for a whole tape (instead of inside every call): the caller keeps a
 * buffer of uz_conv_packed_bytes() per (layer, direction), describes them in a device table of 8 int64 per layer
 * {w address, image address, Mc, Kc, wCi, uz_conv_pack_cot(), flags, first row} with rows counted by uz_conv_pack_rows()
 * (Mc / Kc = output / contraction channels of the direction: forward Cout / Cin, data gradient Cin / Cout; wCi = Cin), runs
 * uz_conv_pack_weights once (w_amax = the bound every image is scaled with) and hands each image to the *_packed calls,
 * which are otherwise uz_conv_fwd / uz_conv_bwd_data (packed_w may be NULL: same behaviour as those).
 * flags: bit 0 = data gradient; bit 1 = w is a Conv3d parameter [Cout][C][3][3][3] read straight into the depth-window layout
 * (volumes section below) - the image uz_w3d_permute mode 0 / mode 1 and a row without the bit would give, byte for byte.
 * Such a row is sized for the 2-D call of the window: forward Mc = Cout, Kc = 3 C with contraction index k = kd C + ci;
 * data gradient Mc = C, Kc = 3 Cout with k = j Cout + co and kd = 2 - j, where the kernel takes Cout as Kc / 3.  wCi is the
 * parameter's own second dimension C in both directions - not the 2-D call's Cin = 3 C.                                     */
size_t uz_conv_packed_bytes(int Cin, int Cout, int W, int dgrad);
int uz_conv_pack_rows(int Cin, int Cout, int W, int dgrad);
int uz_conv_pack_cot(int Cin, int Cout, int W, int dgrad);
int uz_conv_pack_weights(const int64_t* table, int n_layers, int total_rows, const float* w_amax, void* stream);
int uz_conv_fwd_packed(const float* x, int Cin, int CinTot,
                       const float* w, const float* bias,
                       float* y, int Cout, int CoutTot,
                       int N, int H, int W, int ks, int relu,
                       const float* x_amax, const float* w_amax, float* y_amax,
                       void* workspace, size_t workspace_bytes, const void* packed_w, void* stream);
/* Forward convolution that also reduces the BatchNorm statistics of its output while the tile is in registers
 * (torchlayers.py:18-21: every Conv2d of a Conv2D unit feeds a BatchNorm2d): bn_partials (nullable) receives
 * uz_conv_bn_partials(...) x Cout x 4 floats for uz_bn_relu_fwd_pre.  uz_conv_bn_partials returns 0 for shapes whose kernel
 * cannot do this (off the split-fp16 path, split-K); relu must be 0 with bn_partials.                                     */
int uz_conv_bn_partials(int Cin, int Cout, int N, int H, int W, int ks);
int uz_conv_fwd_bnstats(const float* x, int Cin, int CinTot, const float* w, const float* bias,
                        float* y, int Cout, int CoutTot, int N, int H, int W, int ks, int relu,
                        const float* x_amax, const float* w_amax, float* y_amax,
                        void* workspace, size_t workspace_bytes, const void* packed_w, float* bn_partials, void* stream);
int uz_conv_bwd_data_packed(const float* dy, int Cout, int CoutTot,
                            const float* w,
                            float* dx, int Cin, int CinTot,
                            int N, int H, int W, int ks, int accumulate,
                            const float* dy_amax, const float* w_amax,
                            void* workspace, size_t workspace_bytes, const void* packed_w, void* stream);
/* autograd of the above w.r.t. its input (aten::convolution_backward, input part):
 * dx[b,ci] (+)= sum_co sum_tap dy[b,co,.] * w[co,ci,flip(tap)]                 */
int uz_conv_bwd_data(const float* dy, int Cout, int CoutTot,
                     const float* w,
                     float* dx, int Cin, int CinTot,
                     int N, int H, int W, int ks, int accumulate,
                     const float* dy_amax, const float* w_amax,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Data gradient with the ReLU backward of the unit that produced A folded in (vanilla U-Net blocks, unet.py:25-30: Conv -> ReLU ->
 * Conv): dx = (a > 0) ? conv_T(dy, w) (+ dx) : 0 - i.e. dx leaves as the gradient w.r.t. that unit's convolution output, no
 * separate uz_relu_bwd pass.  partials: uz_conv_bwd_relu_partials() x Cin x 4 floats whose .x components uz_chan_sum_partials adds
 * up to the unit's bias gradient; dx_amax: bound slot of dx.  uz_conv_bwd_relu_partials() == 0: shape not supported (off the
 * split path or split-K) - use uz_conv_bwd_data + uz_relu_bwd. */
int uz_conv_bwd_relu_partials(int Cin, int Cout, int N, int H, int W, int ks);
int uz_conv_bwd_data_relu(const float* dy, int Cout, int CoutTot, const float* w, float* dx, int Cin, int CinTot,
                          int N, int H, int W, int ks, int accumulate, const float* dy_amax, const float* w_amax,
                          void* workspace, size_t workspace_bytes, const void* packed_w,
                          const float* a, int aCtot, float* partials, float* dx_amax, void* stream);
int uz_chan_sum_partials(const float* partials, int n_rows, int C, float* out, void* stream);
/* The same fold for the OTHER last writers of a unit's dA: the backward of the pooling / interpolation that consumed A (the third
 * unit of every U-Net block).  partials: uz_resample_bwd_relu_rows(kind, C, N, H, W) x C doubles (kind 0 = avgpool2 with H x W the
 * high-resolution plane, 1 = bilinear2x with H x W the low-resolution plane), summed by uz_chan_sum_partials_d. */
int uz_resample_bwd_relu_rows(int kind, int C, int N, int H, int W);
int uz_avgpool2_bwd_relu(const float* dy, int C, int CtotDy, float* dx, int CtotDx, int N, int H, int W, int accumulate,
                         const float* a, int CtotA, double* partials, float* dx_amax, void* stream);
int uz_bilinear2x_bwd_relu(const float* dy, int C, int CtotDy, float* dx, int CtotDx, int N, int H, int W, int align_corners, int accumulate,
                           const float* a, int CtotA, double* partials, float* dx_amax, void* stream);
int uz_chan_sum_partials_d(const double* partials, int n_rows, int C, float* out, void* stream);
/* every bias gradient of a tape in one launch: table = n_entries rows of 5 int64 {partials pointer, out pointer, n_rows, C, partials are double} */
int uz_chan_sum_table(const int64_t* table, int n_entries, int max_channels, void* stream);
/* autograd w.r.t. the weight: dw[co,ci,tap] = sum_{b,y,x} dy * x_shifted.
 * Deterministic split-K: partial slabs in `workspace` (uz_conv_bwd_weight_workspace
 * bytes), then an ordered reduction.  db (nullable) = sum_{b,y,x} dy.
 * Depth window (Cin == 3 * CinTot, ks 3: a Conv3d run over D slices, see the volume section): dw is written in the Conv3d
 * parameter layout [Cout][CinTot][3][3][3] (contraction channel k = kd * CinTot + ci), no separate permutation needed.   */
size_t uz_conv_bwd_weight_workspace(int Cin, int Cout, int N, int H, int W, int ks);
int uz_conv_bwd_weight(const float* x, int Cin, int CinTot,
                       const float* dy, int Cout, int CoutTot,
                       float* dw, float* db,
                       int N, int H, int W, int ks,
                       const float* x_amax, const float* dy_amax,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- BatchNorm2d(eps, momentum) + ReLU
 * torchlayers.py:20-21 (nn.BatchNorm2d(eps=1e-3, momentum=0.01) -> nn.ReLU).
 * training != 0: batch statistics (biased var) normalise, running stats get the
 * momentum update with the unbiased var; save_mean_rstd[2*C] keeps (mean, rstd) for
 * backward.  training == 0: running stats normalise.  workspace >= uz_bn_workspace(). */
size_t uz_bn_workspace(int C, int N, int H, int W);
int uz_bn_relu_fwd(const float* y, int C, int CtotY,
                   const float* gamma, const float* beta,
                   float* running_mean, float* running_var,
                   float* save_mean_rstd,
                   float* a, int CtotA,
                   int N, int H, int W, float eps, float momentum, int training, int relu,
                   float* a_amax, void* workspace, void* stream);
/* The same with the batch statistics taken from the partials the producing convolution wrote in its epilogue
 * (uz_conv_fwd_bnstats): conv_partials = [n_partials][C][4] floats {sum, sum of squares, max, max of the negated}; NULL / 0 =
 * uz_bn_relu_fwd.  Training mode, N*H*W > 4096 only.                                                                     */
int uz_bn_relu_fwd_pre(const float* y, int C, int CtotY, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, float* save_mean_rstd,
                       float* a, int CtotA, int N, int H, int W, float eps, float momentum,
                       int training, int relu, float* a_amax, void* workspace,
                       const float* conv_partials, int n_partials, void* stream);
/* Small planes (N*H*W <= 4096: the 8x8 ... 2x2 levels), where a Conv2D unit (torchlayers.py:7-29) is a chain of short launches:
 * the convolution's split-K reduce folded into the BatchNorm.  uz_conv_splitk_parts() = number of partial-sum slabs the fp32 forward
 * kernel produces for a shape when given its workspace (1: unsplit or another kernel family - not foldable); uz_conv_fwd_slabs runs
 * that kernel only and leaves [parts][N][Cout][H*W] floats at the start of `workspace` (>= uz_conv_workspace()); uz_bn_relu_fwd_slabs
 * then forms y = conv_bias + slabs (slab order: bit-identical to uz_conv_fwd), WRITES y (the backward pass reads it) and does what
 * uz_bn_relu_fwd does.                                                                                                    */
int uz_conv_splitk_parts(int Cin, int Cout, int N, int H, int W, int ks);
int uz_conv_fwd_slabs(const float* x, int Cin, int CinTot, const float* w, int Cout, int N, int H, int W, int ks,
                      void* workspace, size_t workspace_bytes, void* stream);
int uz_conv_bwd_splitk_parts(int Cin, int Cout, int N, int H, int W, int ks);      /* the data gradient's split count (1: not split, or another kernel family) */
int uz_conv_bwd_data_slabs(const float* dy, int Cout, int CoutTot, const float* w, int Cin, int N, int H, int W, int ks,
                           float* slabs_out, void* stream);                        /* [parts][N][Cin][H*W] partial sums; summed by uz_bn_relu_bwd_ex(da_slabs) */
int uz_bn_relu_fwd_slabs(const float* slabs, int n_slabs, const float* conv_bias, float* y, int C, int CtotY,
                         const float* gamma, const float* beta, float* running_mean, float* running_var, float* save_mean_rstd,
                         float* a, int CtotA, int N, int H, int W, float eps, float momentum,
                         int training, int relu, float* a_amax, void* stream);
/* native_batch_norm_backward + threshold_backward: da -> dy, dgamma, dbeta, and the
 * conv-bias gradient dbias = sum dy (nullable).  dy may alias da.               */
int uz_bn_relu_bwd(const float* da, int CtotDa,
                   const float* y, int C, int CtotY,
                   const float* gamma, const float* beta, const float* save_mean_rstd,
                   float* dy, int CtotDy,
                   float* dgamma, float* dbeta, float* dbias,
                   int N, int H, int W, int relu,
                   float* dy_amax, void* workspace, void* stream);
/* ReLU-only units of the vanilla U-Net (unet.py:26,28,30): da * [a > 0] (threshold_backward)
 * fused with the conv-bias gradient.                                              */
int uz_relu_bwd(const float* da, int CtotDa, const float* a, int C, int CtotA,
                float* dy, int CtotDy, float* dbias,
                int N, int H, int W, float* dy_amax, void* workspace, void* stream);

/* ---------------------------------------------------------------- split storage + folded BatchNorm backward (round 4)
 * Conv2D unit = Conv2d -> BatchNorm2d -> ReLU (torchlayers.py:18-21), 106 of them per PHiSeg step.  Two things the producer of
 * a tensor can do for the matrix kernels that consume it:
 *
 * Split storage.  A tensor whose bound is known BEFORE its first element is written (BatchNorm forward: exact output range from
 * the statistics; BatchNorm backward: analytic bound; pooling / interpolation: the input's bound) may be stored as one 32-bit
 * word per element holding the two fp16 pieces of v * s (low half h1 = fp16(v s), high half h2 = fp16(v s - h1), s = the power of
 * two the split kernels derive from the bound slot) - the operand pieces the consuming convolution would otherwise form from the
 * fp32 value in its staging (scale, clamp, two conversions, subtract, convert per element).  Same bytes, same values
 * (h1 + h2 = v s to 2^-22); the `out_packed` producers below write it, the `*_packed` flags of the convolution calls read it.
 * A concat buffer with two producers carries two bounds: channels [0, seg_channels) were scaled from x_amax, the rest from
 * x_amax2 (seg_channels a multiple of 16; 0 = one bound).  uz_pack_split / uz_unpack_split convert whole tensors (tests, tools).
 *
 * Folded backward reduction.  The data gradient that writes dA of a unit LAST can apply the unit's ReLU mask (alpha y + beta' > 0)
 * and leave the unit's BatchNorm-backward sums {sum dz, sum dz x_hat, max |dz|, max |x_hat|} per (tile, channel) in its epilogue
 * (bn_y = the unit's pre-normalisation output, bn_save = the 4 C floats uz_bn_relu_fwd_ex saved); uz_bn_relu_bwd_ex then runs a
 * one-workgroup-per-channel finalise instead of the reduction pass over dA and y.  uz_conv_bwd_relu_partials() gives the number of
 * partial rows (0: shape not supported).                                                                                       */
int uz_pack_split(const float* x, float* packed, size_t n, const float* amax, void* stream);
int uz_unpack_split(const float* packed, float* x, size_t n, const float* amax, void* stream);
int uz_bn_relu_fwd_ex(const float* y, int C, int CtotY, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float* save_mean_rstd_ab,
                      float* a, int CtotA, int N, int H, int W, float eps, float momentum,
                      int training, int relu, float* a_amax, void* workspace,
                      const float* conv_partials, int n_partials, int out_packed, void* stream);
int uz_bn_relu_bwd_ex(const float* da, int CtotDa, const float* y, int C, int CtotY,
                      const float* gamma, const float* beta, const float* save_mean_rstd,
                      float* dy, int CtotDy, float* dgamma, float* dbeta, float* dbias,
                      int N, int H, int W, int relu, float* dy_amax, void* workspace,
                      const float* conv_partials, int n_partials, int out_packed, double* dbias_partials,
                      const float* da_slabs, int n_da_slabs, void* stream);   /* da_slabs: dA = the sum of these [n][N][C][H*W] slabs (small planes, uz_conv_bwd_data_slabs); da is then not read */
/* uz_bn_relu_fwd_ex as two calls (large planes, training, statistics from the convolution's partials): phase 1 = statistics only (table of 4 C floats,
 * running buffers, the activation's bound; y / a untouched and nullable), phase 2 = the apply pass alone from what phase 1 left.  A following
 * uz_conv_fwd_bn_ex depends on phase 1 only: the apply pass then runs beside that convolution instead of in front of it. */
int uz_bn_relu_fwd_phase(const float* y, int C, int CtotY, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float* save_mean_rstd_ab,
                         float* a, int CtotA, int N, int H, int W, float eps, float momentum,
                         int relu, float* a_amax, const float* conv_partials, int n_partials, int out_packed, int phase, void* stream);
int uz_bn_fwd_fused_limit(int H, int W);         /* N*H*W up to which the training-mode uz_bn_relu_fwd(_ex) WITHOUT conv_partials is one launch (statistics + apply from registers) */
int uz_bn_bwd_fused_limit(int H, int W);         /* N*H*W up to which uz_bn_relu_bwd(_ex) is one launch with the channel's batch on chip: no out_packed / dbias_partials there */
int uz_bn_bwd_dbias_rows(int N, int H, int W);   /* rows of dbias_partials ([rows][C] doubles, summed by uz_chan_sum_table); 0: small-plane path */
/* What a BatchNorm call launches, answered on the host by the very function the entry points dispatch on (the library loads without a
 * GPU).  direction: 0 = uz_bn_relu_fwd / _pre / _ex / _phase / _slabs / _b16, 1 = uz_bn_relu_bwd / _ex / _b16; N, C, H, W, training as the
 * call takes them; vec != 0: every view the call inspects (y and a; da, y and dy) is 16-byte aligned; flags: 1 conv_partials given,
 * 2 out_packed, 4 dbias_partials given, 8 slabs / da_slabs given, 16 a *_b16 (bf16 storage) entry point.  out6 receives
 *   [0] path: 0 small (one 256-thread workgroup per channel), 1 mid (one 512- / 1024-thread workgroup per channel), 2 large
 *       (statistics or reduction pass + apply pass), 3 large with bf16 storage;
 *   [1] instance: small - elements per thread 2 / 8 / 16; mid - threads per workgroup 512 / 1024; large - 0;
 *   [2] parts: chunks of 16 384 elements per plane;   [3] nb, [4] ngrp: images per reduction workgroup and the number of image
 *       groups of the large paths (0 elsewhere);   [5] 1 where the float4 instance runs.
 * Honours UZ_BN_MID, UZ_BN_MID_FWD and UZ_BN_MID_HALF as the dispatch does (each read once per process).  Returns 0, or -1 for
 * arguments no entry point accepts (empty tensor, unknown flag bits, bf16 storage outside N*H*W > 32 768 with H*W % 4 == 0).       */
int uz_bn_route(int direction, int N, int C, int H, int W, int training, int vec, int flags, int* out6);
int uz_avgpool2_fwd_ex(const float* x, int C, int CtotX, float* y, int CtotY, int N, int H, int W,
                       const float* x_amax, float* y_amax, int out_packed, void* stream);
int uz_bilinear2x_fwd_ex(const float* x, int C, int CtotX, float* y, int CtotY, int N, int H, int W, int align_corners,
                         const float* x_amax, float* y_amax, int out_packed, void* stream);
int uz_conv_fwd_ex(const float* x, int Cin, int CinTot, const float* w, const float* bias,
                   float* y, int Cout, int CoutTot, int N, int H, int W, int ks, int relu,
                   const float* x_amax, const float* w_amax, float* y_amax,
                   void* workspace, size_t workspace_bytes, const void* packed_w, float* bn_partials,
                   int x_packed, const float* x_amax2, int seg_channels, void* stream);
/* uz_conv_fwd_ex for a layer that follows a Conv -> BatchNorm -> ReLU unit (reference torchlayers.py:18-21) and reads that unit's
 * PRE-normalisation output y_prev with its statistics table bn_save ([4][Cin]: mean, rstd, alpha, beta' - uz_bn_relu_fwd_ex): the staging
 * applies a = max(alpha y_prev + beta', 0) (bn_relu) itself and splits with the scale of a_amax, the bound of the APPLIED activation.
 * Same values as reading the unit's stored activation; the unit's apply pass leaves the chain of dependent launches.  Split path only. */
int uz_conv_fwd_bn_ex(const float* y_prev, int Cin, int CinTot, const float* bn_save, int bn_relu,
                      const float* w, const float* bias, float* y, int Cout, int CoutTot, int N, int H, int W, int ks,
                      const float* a_amax, const float* w_amax, float* y_amax,
                      void* workspace, size_t workspace_bytes, const void* packed_w, float* bn_partials, void* stream);
int uz_conv_bwd_data_ex(const float* dy, int Cout, int CoutTot, const float* w, float* dx, int Cin, int CinTot,
                        int N, int H, int W, int ks, int accumulate, const float* dy_amax, const float* w_amax,
                        void* workspace, size_t workspace_bytes, const void* packed_w, int dy_packed,
                        const float* bn_y, int bn_yCtot, const float* bn_save, int bn_relu, float* bn_partials, void* stream);
int uz_conv_bwd_weight_ex(const float* x, int Cin, int CinTot, const float* dy, int Cout, int CoutTot,
                          float* dw, float* db, int N, int H, int W, int ks,
                          const float* x_amax, const float* dy_amax, void* workspace, size_t workspace_bytes,
                          int x_packed, const float* x_amax2, int seg_channels, int dy_packed, float* slabs_out, void* stream);
/* Weight-gradient slab reductions of many layers in ONE launch.  slabs_out (above, nullable): the call leaves its
 * uz_conv_bwd_weight_slabs() x ks*ks x Cout x Cin partial sums there instead of reducing them into dw; uz_wgrad_reduce_table adds
 * them later - table rows of 8 int64 {slabs, dw, S, Cout, Cin, ks*ks, first block, volC}, blocks counted by uz_wgrad_reduce_blocks();
 * volC = 0, or - the call was a depth window (Cin = 3 volC view channels over a volC-channel buffer) - the window's C: the sum
 * then leaves in the Conv3d parameter layout [Cout][volC][3][3][3] exactly as the call's own reduction writes it.
 * Same order of additions as the in-call reduction (bitwise the same dw).                                                        */
int uz_conv_bwd_weight_slabs(int Cin, int Cout, int N, int H, int W, int ks);
int uz_wgrad_reduce_blocks(int Cin, int Cout, int ks);
int uz_wgrad_reduce_table(const int64_t* table, int n_layers, int total_blocks, void* stream);

/* ---------------------------------------------------------------- resampling
 * nn.AvgPool2d(2, 2, padding=0, ceil_mode=True): phiseg.py:23, unet.py:22,
 * probabilistic_unet.py:56.  Ho = ceil(H/2); partial windows divide by the
 * in-bounds element count.                                                        */
int uz_avgpool2_fwd(const float* x, int C, int CtotX, float* y, int CtotY,
                    int N, int H, int W, const float* x_amax, float* y_amax, void* stream);   /* |y| <= bound of |x| is forwarded */
int uz_avgpool2_bwd(const float* dy, int C, int CtotDy, float* dx, int CtotDx,
                    int N, int H, int W, int accumulate, void* stream);
/* F.interpolate(mode='bilinear', scale_factor=2, align_corners=ac): phiseg.py:66,213-216,
 * 305-309 (ac=1), unet.py:67 (ac=0).  (H, W) are the INPUT sizes.                 */
int uz_bilinear2x_fwd(const float* x, int C, int CtotX, float* y, int CtotY,
                      int N, int H, int W, int align_corners, const float* x_amax, float* y_amax, void* stream);
int uz_bilinear2x_bwd(const float* dy, int C, int CtotDy, float* dx, int CtotDx,
                      int N, int H, int W, int align_corners, int accumulate, void* stream);
/* F.interpolate(size=[Ho,Wo], mode='nearest'), integer factor: phiseg.py:321        */
int uz_nearest_fwd(const float* x, int C, int CtotX, float* y, int CtotY,
                   int N, int H, int W, int factor, void* stream);
int uz_nearest_bwd(const float* dy, int C, int CtotDy, float* dx, int CtotDx,
                   int N, int H, int W, int factor, int accumulate, void* stream);
/* torch.mean over H then W (probabilistic_unet.py:114-115): (N,C,H,W) -> (N,C)       */
int uz_spatial_mean_fwd(const float* x, int C, int CtotX, float* y, int N, int H, int W, void* stream);
int uz_spatial_mean_bwd(const float* dy, int C, float* dx, int CtotDx, int N, int H, int W,
                        int accumulate, void* stream);

/* The kernel a streaming call takes, answered on the host from the very predicates the entry points dispatch through (the
 * library loads without a GPU).  op: 0 uz_avgpool2_fwd, 1 uz_avgpool2_bwd(_relu), 2 uz_bilinear2x_fwd, 3 uz_bilinear2x_bwd(_relu),
 * 4 uz_nearest_bwd, 5 uz_add_views.  C, N, H, W as the entry point takes them; arg = the factor of op 4 (unused elsewhere);
 * align_* = byte alignment (16, 8 or 4) of the views the dispatch inspects: src = x / dy / a, dst = y / dx, aux = the activation
 * of op 1's _relu form / b of op 5 (16 when absent).  Returns 0 generic / scalar kernel, 1 vector or band kernel (float4 / float2
 * pooling, forward band, backward pair band, float4 add), 2 float4 backward band, 3 one wave per element.  Honours
 * UZ_BILINEAR_BWD_PAIR as the dispatch does.  The band kernels' workgroups per plane: uz_resample_bwd_relu_rows(1, ...) / N. */
int uz_stream_route(int op, int C, int N, int H, int W, int arg, int align_src, int align_dst, int align_aux);

/* ---------------------------------------------------------------- latent heads / losses
 * mask (N,1,H,W) float {0,1,..} -> cat([patch, onehot(mask)-0.5], 1): utils.py:289-311,
 * phiseg.py:178-183, probabilistic_unet.py:103-109.  out has in_ch + nlabels channels. */
int uz_posterior_input(const float* patch, int in_ch, const float* mask, int nlabels,
                       float* out, int N, int H, int W, void* stream);
/* Reparameterised latent sample.  act = 0: SampleZBlock tail (phiseg.py:100-105), sigma =
 * softplus(pre_sigma) (beta 1, threshold 20); act = 1: AxisAlignedConvGaussian + rsample
 * (probabilistic_unet.py:124-129,350), sigma = exp(pre_sigma).  z = mu + sigma * eps (z nullable:
 * the prior's own draw is discarded in training, phiseg.py:200-202).  n = number of elements. */
int uz_latent_sample_fwd(const float* mu, const float* pre_sigma, const float* eps,
                         float* sigma, float* z, size_t n, int act, void* stream);
/* dmu_pre = dmu + dz ; dpre_sigma = (dsigma + dz*eps) * dsigma/dpre, with dsigma/dpre =
 * 1 - exp(-sigma) (softplus) or sigma (exp); dmu / dsigma / dz are nullable (treated as 0).  */
int uz_latent_sample_bwd(const float* dmu, const float* dsigma, const float* dz,
                         const float* eps, const float* sigma,
                         float* dmu_pre, float* dpre_sigma, size_t n, int act, void* stream);
/* The two heads of a SampleZBlock and its sampling tail as ONE launch (phiseg.py:95-105): mu = mu_conv(h), pre_sigma =
 * sigma_conv(h) (1x1 convolutions, L latent channels each, weights [L][Cin], biases nullable), sigma = softplus(pre_sigma)
 * (act = 0; act = 1: exp), z = mu + sigma * eps (z nullable).  h is a view of Cin channels in a buffer of CinTot; mu,
 * pre_sigma, sigma, z, eps are contiguous [N][L][H][W].  Bit-identical to uz_conv_fwd x 2 + uz_latent_sample_fwd; h is read
 * once.  1 <= L <= 4, Cin <= 512 (uz_latent_heads_ok). */
int uz_latent_heads_ok(int Cin, int L);
int uz_latent_heads_fwd(const float* h, int Cin, int CinTot, const float* w_mu, const float* b_mu,
                        const float* w_sigma, const float* b_sigma, const float* eps, float* mu, float* pre_sigma,
                        float* sigma, float* z, int L, int N, int H, int W, int act, void* stream);
/* Backward of the two heads: dh (+)= w_a^T dy_a + w_b^T dy_b in one pass (head a's rows are added first: pass the head whose
 * separate data gradient would have run first), and both heads' weight / bias gradients from one read of h (fp64 ordered
 * partial sums in `workspace`, uz_latent_heads_bwd_weight_workspace bytes; db_* nullable). */
int uz_latent_heads_bwd_data(const float* dy_a, const float* dy_b, int L, const float* w_a, const float* w_b,
                             float* dh, int Cin, int CinTot, int N, int H, int W, int accumulate, void* stream);
size_t uz_latent_heads_bwd_weight_workspace(int Cin, int L, int N, int H, int W);
int uz_latent_heads_bwd_weight(const float* h, int Cin, int CinTot, const float* dy_a, const float* dy_b, int L,
                               float* dw_a, float* db_a, float* dw_b, float* db_b, int N, int H, int W,
                               void* workspace, size_t workspace_bytes, void* stream);
/* What a 1x1 head (ks = 1, at most 8 outputs) or a latent-heads call launches, answered on the host from the very predicates the
 * entry points dispatch through (the library loads without a GPU).  op: 0 the 1x1 forward (uz_conv_fwd* with relu = 0,
 * uz_conv1x1_fwd_b16), 1 its data gradient, 2 its weight gradient, 3 uz_latent_heads_fwd, 4 uz_latent_heads_bwd_data,
 * 5 uz_latent_heads_bwd_weight.  Cout: the output channels of ops 0 - 2, L of ops 3 - 5; Cin, N, H, W as the call takes them;
 * aligned != 0: every view the call inspects is 16-byte aligned (x and y; dy and dx; x and dy; h, mu, pre_sigma, sigma and - when
 * given - z and eps; dy_a, dy_b and dh; h, dy_a and dy_b).  out5 receives
 *   [0] form: 0 scalar, 1 float4, 2 channel-parallel forward (op 3 only), 3 not covered by the streaming kernels (ops 0 - 2 with
 *       Cout outside {1, 2, 3, 4, 6, 8} or Cin > 512: the call runs the MFMA kernels, [1] .. [4] stay 0);
 *   [1] workgroups of 1 024 pixels per image (ops 0, 1, 3, 4), or QPB, the pixel quads per workgroup, of form 2;
 *   [2] channel groups (grid.z) and [3] channels per group of the data gradients (ops 1, 4), the last group may be ragged;
 *   [4] chunks of the weight gradients (ops 2, 5): ceil(N*H*W / 16 384), at most 64.
 * Honours UZ_HEADS_PAR as the dispatch does.  Returns 0, or -1 for arguments no entry point accepts (empty tensor, latent heads
 * outside 1 <= L <= 4, Cin <= 512).                                                                                              */
int uz_heads_route(int op, int Cin, int Cout, int N, int H, int W, int aligned, int* out5);
/* KL_two_gauss_with_diag_cov with the reference's sigma1*sigma0 quirk (phiseg.py:436-453),
 * times `weight` (4**level, phiseg.py:463).  Tensors are (N, per_sample) contiguous.
 * fwd writes loss_out[0] (single block, ordered); bwd writes the four gradients * scale. */
int uz_kl_fwd(const float* mu0, const float* s0, const float* mu1, const float* s1,
              int N, int per_sample, float weight, float* loss_out, void* stream);
/* uz_kl_fwd with a scratch of >= 512 bytes (nullable): tensors beyond 128 k elements (a volume's full-resolution latent level is ONE
 * sample of 2 M elements) are summed by up to 64 workgroups + an ordered final pass instead of one workgroup. */
int uz_kl_fwd_ws(const float* mu0, const float* s0, const float* mu1, const float* s1, int N, int per_sample, float weight,
                 float* loss_out, void* workspace, void* stream);
/* partial workgroups uz_kl_fwd_ws sums (N, per_sample) with, given a workspace: 1 = the single-workgroup kernel of uz_kl_fwd */
int uz_kl_fwd_parts(int N, int per_sample);
int uz_kl_bwd(const float* mu0, const float* s0, const float* mu1, const float* s1,
              int N, int per_sample, float weight, const float* loss_scale,
              float* dmu0, float* ds0, float* dmu1, float* ds1, void* stream);
/* residual_multinoulli_loss (phiseg.py:481-513), 2..8 classes, L levels of (N,K,H,W) logits
 * given as an array of L device pointers held in DEVICE memory (s_ptrs).  level l loss =
 * mean_b sum_pix CE(sum_{j>=l} s_j, mask).  loss_out[l], l=0..L-1.                      */
size_t uz_ce_workspace(int N, int H, int W, int L);
int uz_residual_ce_fwd(const float* const* s_ptrs, int L, int K, const float* mask,
                       int N, int H, int W, float* loss_out, void* workspace, void* stream);
int uz_residual_ce_bwd(const float* const* s_ptrs, float* const* ds_ptrs, int L, int K, const float* mask,
                       int N, int H, int W, const float* loss_scale, void* stream);
/* nn.CrossEntropyLoss() mean over all pixels (unet.py:159-165) = residual CE with L=1 scaled 1/(H*W) */
/* loss_terms[0..n-1] -> total[0] = sum (ordered)                                         */
int uz_sum_terms(const float* terms, int n, float* total, void* stream);
/* accumulate_output(use_softmax) + argmax (phiseg.py:428-434, train_model.py:186,195):
 * acc = sum_l s_l ; soft = softmax_c(acc) ; label = argmax_c.  soft / label nullable.     */
int uz_accumulate_softmax_argmax(const float* const* s_ptrs, int L, int K, int N, int H, int W,
                                 float* acc, float* soft, uint8_t* label, void* stream);

/* ---------------------------------------------------------------- mask-free inference (PHISeg.predict; csrc/predict.hip)
 * patch.repeat(S, 1, 1, 1) of a channel slice: y[s*B + b, c] = x[b, c] for s < S.  x / y are C-channel slices of buffers with
 * CtotX / CtotY channels (the convention of uz_nearest_fwd); x holds B images, y S*B.  Every source element is read once and
 * written S times; 16-byte accesses where H*W % 4 == 0 and both slices start 16-byte aligned, 4-byte ones otherwise.          */
int uz_batch_repeat_fwd(const float* x, int C, int CtotX, float* y, int CtotY,
                        int B, int S, int H, int W, void* stream);
/* S samples of B images in one pass over the L level logits (S*B,K,H,W), row s*B + b = sample s of image b (s_ptrs: L device
 * pointers held in DEVICE memory; the inputs are not written):  acc = sum_l s_l in fp32, in the level order of
 * uz_accumulate_softmax_argmax; soft = softmax_K(acc); labels = argmax_K(acc); mean_soft[b] = (sum_s soft[s*B + b]) / S, added
 * in the order s = 0 .. S-1 by the one thread that owns the pixel (bit-repeatable); mean_label = argmax_K(mean_soft);
 * entropy = -sum_k p_k ln p_k of p = mean_soft (a term with p_k = 0 is 0).  Softmax, mean and entropy are evaluated in fp64 and
 * rounded to fp32 once, when they are stored; mean_label is decided on the unrounded means.  Both argmax take the first maximum,
 * as np.argmax does.  1 <= K <= 8.  soft (S*B,K,H,W), labels (S*B,H,W), mean_label (B,H,W) and entropy (B,H,W) are nullable.   */
int uz_sample_stats(const float* const* s_ptrs, int L, int K, int B, int S, int H, int W,
                    float* soft, uint8_t* labels, float* mean_soft, uint8_t* mean_label, float* entropy, void* stream);
/* The same statistics for S samples of ONE volume that arrive one after another (PHISeg3D.predict; csrc/predict.hip), read from the
 * L level logits at their own resolution - the nearest resize to the full volume is never materialised.
 * uz_vol_sample_accum, one sample:
 *   s_ptrs, ctot, f, fz   HOST arrays of L entries: level l is a volume [D / fz[l]][ctot[l]][H / f[l]][W / f[l]] (Plan.vol layout; the
 *                         pointer addresses real slice 0, classes are its channels 0 .. K-1, ctot[l] >= K); voxel (od, oy, ox) reads
 *                         (od / fz, oy / f, ox / f), the index of uz_nearest3d_fwd.  The inputs are not written.
 *   labels  (D, H, W) uint8, soft (K, D, H, W) fp32 or null: this sample's argmax (first maximum) and softmax, dense
 *   acc     (K, D, H, W) fp64: the running sum of the samples' probabilities, ASSIGNED when first != 0, added to otherwise
 * The logits are summed in fp32 in the level order of uz_sample_stats, everything behind the sum is fp64.
 * uz_vol_sample_finish: p = acc / S -> mean_soft (K, D, H, W) fp32, mean_label (D, H, W) uint8 = first maximum of the unrounded p,
 * entropy (D, H, W) fp32 = -sum_k p_k ln p_k (a term with p_k = 0 is 0); mean_label and entropy are nullable.
 * Fed S samples in the order s = 0 .. S-1, the pair gives bit for bit what uz_sample_stats gives on the resized levels with B = 1 and
 * H W := D H W.  1 <= K <= 8, 1 <= L <= 8, D H W < 2^31; a null pointer, a factor below 1, a size that is not level size x factor and
 * ctot < K are errors.  One voxel per thread, any shape and alignment.                                                           */
int uz_vol_sample_accum(const float* const* s_ptrs, const int* ctot, const int* f, const int* fz, int L, int K, int D, int H, int W,
                        uint8_t* labels, float* soft, double* acc, int first, void* stream);
int uz_vol_sample_finish(const double* acc, int K, int S, int D, int H, int W,
                         float* mean_soft, uint8_t* mean_label, float* entropy, void* stream);
/* A whole volume (D, H, W) from overlapping windows (PHISeg3D.predict_volume; csrc/volwindow.hip).  A window has extent
 * (wd, wh, ww) and origin (oz, oy, ox) >= 0 in the volume and may hang over its far faces; window voxel (z, y, x) is volume voxel
 * (oz + z, oy + y, ox + x).
 * uz_vol_window_gather: src (C, D, H, W) fp32, dense -> dst, the C-channel slice of a plan volume [wd][Ctot][wh][ww] (Plan.vol
 *   layout; the pointer addresses channel 0 of the slice in real slice 0).  Every element of the slice is written once: the
 *   source voxel, or 0 where the window hangs over the volume.  src is not written.
 * uz_vol_window_accum, one sample of one window:
 *   s_ptrs, ctot, f, fz   HOST arrays of L entries, as uz_vol_sample_accum takes them, for a volume of the WINDOW's extent: level l
 *                         is [wd / fz[l]][ctot[l]][wh / f[l]][ww / f[l]] and window voxel (z, y, x) reads (z / fz, y / f, x / f).
 *                         The logits are summed in fp32 in the level order of uz_sample_stats; everything behind the sum is fp64
 *                         (max-shifted softmax p_k).  The inputs are not written.
 *   tz, ty, tx            DEVICE tables of wd, wh, ww fp64 blend weights; the voxel's weight is (tz[z] * ty[y]) * tx[x]
 *   acc  (K, D, H, W) fp64, THIS sample's accumulator: acc[k][voxel] += weight * p_k (a product and a sum, each rounded once)
 *   wsum (D, H, W) fp64: wsum[voxel] += weight when add_weight != 0 - the caller sets it for ONE sample of each window
 *   Only the window voxels inside the volume are touched.  The caller zeroes acc and wsum before the first window.
 * uz_vol_window_finish, once, for all S samples: acc (S, K, D, H, W), wsum (D, H, W) ->
 *   labels (S, D, H, W) uint8 = first maximum of acc_s;  p_s = acc_s / wsum;  soft (S, K, D, H, W) = fp32(p_s), nullable;
 *   mean = (sum_s p_s) / S, added in the order s = 0 .. S-1;  mean_soft (K, D, H, W) = fp32(mean);  mean_label (D, H, W) = first
 *   maximum of the unrounded mean, entropy (D, H, W) = -sum_k mean_k ln mean_k (a term with mean_k = 0 is 0); both nullable.
 * No atomics: launches on one stream serialise the adds to a voxel, so windows fed in a fixed order give the same bits every time.
 * One element per thread, one form for every shape and alignment.  1 <= K <= 8, 1 <= L <= 8, D H W < 2^31, wd wh ww < 2^31 (gather:
 * C D H W and wd C wh ww < 2^31).  Refused by the host part before any launch (-1, uz_last_error names the reason, nothing is
 * written): a null pointer (wsum too, whatever add_weight says), a factor below 1, a window that is not level size x factor,
 * ctot < K (gather: Ctot < C), an origin below 0, an extent or size below 1.  A voxel that no window reached (wsum == 0) is data the
 * host part cannot see: uz_vol_window_finish gives it label 0, probabilities 0 and entropy 0 - never NaN; covering the volume is
 * the caller's duty (models/phiseg3D.py window_grid does).
 * Mirrored passes (predict_volume(flips=...)): flip is a mask 0 .. 7, bit 0, 1, 2 = D, H, W as prm[30] of uz_augment_volume.  A pass
 * mirrors the WINDOW within itself: net-frame voxel (z, y, x) is window voxel (z', y', x'), z' = wd - 1 - z where bit 0 is set, else z
 * (likewise y', x'); grid, origins and coverage are those of the unmirrored pass.
 * uz_vol_window_gather_ex: dst voxel (z, y, x) = src voxel (oz + z', oy + y', ox + x'), 0 where that lies beyond the volume.
 * uz_vol_window_accum_ex: net-frame voxel (z, y, x) - levels read at (z / fz, y / f, x / f) as ever - adds to volume voxel
 *   (oz + z', oy + y', ox + x') with the weight (tz[z'] * ty[y']) * tx[x']: the tables are indexed in the window, not in the net frame,
 *   so they need not be symmetric.  add_weight acts on wsum at the same voxel; nothing is touched where it lies beyond the volume.
 * uz_vol_window_noise: field (C2, d, h, w) fp32, dense - one sample's row of one latent level's noise - -> dst, the C2-channel slice of
 *   a plan volume [cd][Ctot][ch][cw]: dst (z, c, y, x) = field (c, oz + z', oy + y', ox + x') with the mirror taken in the crop
 *   (cd, ch, cw), origin and extents at the LEVEL's resolution.  Every element of the slice is written once.
 * With flip == 0 the _ex calls give the bytes of the plain ones (which forward to them) and uz_vol_window_noise those of a slice copy.
 * Refused as above, and: a mask outside 0 .. 7, a crop that leaves its field, C2 d h w or cd C2 ch cw >= 2^31.                     */
int uz_vol_window_gather(const float* src, int C, int D, int H, int W, int oz, int oy, int ox,
                         float* dst, int Ctot, int wd, int wh, int ww, void* stream);
int uz_vol_window_accum(const float* const* s_ptrs, const int* ctot, const int* f, const int* fz, int L, int K,
                        int wd, int wh, int ww, int oz, int oy, int ox, int D, int H, int W,
                        const double* tz, const double* ty, const double* tx, double* acc, double* wsum, int add_weight, void* stream);
int uz_vol_window_finish(const double* acc, const double* wsum, int K, int S, int D, int H, int W,
                         uint8_t* labels, float* soft, float* mean_soft, uint8_t* mean_label, float* entropy, void* stream);
int uz_vol_window_gather_ex(const float* src, int C, int D, int H, int W, int oz, int oy, int ox,
                            float* dst, int Ctot, int wd, int wh, int ww, int flip, void* stream);
int uz_vol_window_accum_ex(const float* const* s_ptrs, const int* ctot, const int* f, const int* fz, int L, int K,
                           int wd, int wh, int ww, int oz, int oy, int ox, int D, int H, int W,
                           const double* tz, const double* ty, const double* tx, double* acc, double* wsum, int add_weight, int flip,
                           void* stream);
int uz_vol_window_noise(const float* field, int C2, int d, int h, int w, int oz, int oy, int ox, int cd, int ch, int cw, int flip,
                        float* dst, int Ctot, void* stream);
/* Fcomb (probabilistic_unet.py:185-199) in eval mode for S latent draws per image, features read once (ProbabilisticUnet.predict;
 * csrc/fcomb.hip).
 *   feat      (B, C of CtotF, H, W), C == 32
 *   mu, sigma (B, L); eps (S*B, L), row s*B + b
 *   z         out (S*B, L):  z = mu[b] + sigma[b] * eps[s*B + b]   (one fused multiply-add)
 *   params    table of pointers in DEVICE memory: per unit u < n_units {w, bias, gamma, beta, running_mean, running_var}, then
 *             {w_last, bias_last}; w of unit 0 is (32, 32 + L) - its columns 32 .. address z -, of the others (32, 32), w_last (K, 32).
 *             The tensors behind the table are read through the constant address space: nothing may write them while the kernel runs.
 *   logits    out (S*B, K, H, W), row s*B + b
 * Every unit is conv 1x1 -> (y - running_mean) * (1 / sqrtf(running_var + bn_eps)) * gamma + beta -> ReLU, the head a bare 1x1
 * convolution; fp32 multiply-adds in a fixed order in every UZ_CONV_MATH mode, no atomics.  C == 32, 1 <= L, K, n_units <= 8;
 * anything else is refused before a launch.                                                                                       */
int uz_fcomb_sample_fwd(const float* feat, int C, int CtotF, const float* mu, const float* sigma, const float* eps,
                        const float* const* params, int n_units, float bn_eps, int L, int K, int B, int S, int H, int W,
                        float* z, float* logits, void* stream);
/* What uz_fcomb_sample_fwd launches for these sizes, from the predicate it launches with (answered on the host).  out5 receives
 * [0] pixels per workgroup (256 or 512: one or two per thread), [1] samples per workgroup, [2] [3] [4] the grid: pixel blocks,
 * images, sample groups (the last group may be ragged).  Honours UZ_FCOMB_PX (1 | 2) as the launch does.  0, or -1 for sizes
 * uz_fcomb_sample_fwd refuses.                                                                                                    */
int uz_fcomb_sample_route(int L, int K, int n_units, int B, int S, int H, int W, int* out5);

/* ---------------------------------------------------------------- validation metrics (train_model.py:186-230)
 * out[i][j][0..2] = |a_i==label & b_j==label|, |a_i==label|, |b_j==label| over HW pixels (int32, exact): the integer core of
 * utils.generalised_energy_distance (utils.py:148-200; IoU = medpy.metric.jc, MedPy 0.4.0) and of the per-label Dice
 * (train_model.py:212-224; medpy.metric.dc).  a: (Na, HW) uint8 label maps, b: (Nb, HW).                               */
int uz_label_pair_counts(const uint8_t* a, int Na, const uint8_t* b, int Nb, int HW, int label, int32_t* out, void* stream);
/* utils.variance_ncc_dist (utils.py:202-247): pixel-wise cross-entropy maps E_ss (HW) and E_sy (M, HW) of N softmax samples
 * (N,K,HW) against M one-hot ground truths (M,K,HW); then ncc(E_ss, E_sy[j]) for every j (utils.py:130-145).              */
int uz_ncc_maps(const float* soft, const float* gt_onehot, int N, int M, int K, int HW, float* E_ss, float* E_sy, void* stream);
int uz_ncc(const float* a, const float* v, int M, int HW, float* out, void* stream);
/* GED, NCC and per-label Dice of S samples of B images against A annotators each, in five launches on `stream` with no host round
 * trip (csrc/score.hip).  P = pixels of a map (H W, or D H W of a volume with B = 1).
 *   labels (S, B, P) uint8: sample s of image b is row s*B + b (Prediction.labels); ann (B, A, P) uint8; mean_label (B, P) uint8;
 *   soft (S, B, K, P) fp32 (Prediction.soft) or null: no NCC, `ncc` and `ncc_pairs` are then not written.
 * Bit planes: for every map and every label k in 0 .. K-1 a plane of ceil(P / 64) 64-bit words in the workspace, bit q % 64 of word
 * q / 64 set when pixel q equals k (bits from P on are 0; a pixel value >= K sets no bit).  Pair counts: popcount(x & y) over the
 * planes.  counts (nullable) int32: for b = 0 .. B-1, within b for k = 0 .. K-1, three matrices [S][A][3] (samples x annotators),
 * [S][S][3] (samples x samples), [A][A][3] (annotators x annotators), each in the layout of uz_label_pair_counts: intersection,
 * |first|, |second|.  Integer, no atomics.
 *   ged (B) fp64: per pair and label l in 1 .. K-1, IoU = 1 if both maps are empty of l, 0 if exactly one is, else inter / union;
 *       d = 1 - (sum_l IoU_l) / (K - 1);  GED_b = 2/(S A) sum d_sy - 1/S^2 sum d_ss - 1/A^2 sum d_yy.  One 256-thread workgroup per
 *       image: thread t adds the pairs t, t + 256, ... of a matrix in row-major pair order, the 256 partial sums are then added by
 *       the xor-butterfly within each wave (offsets 32 .. 1) and the four waves in the order 0 .. 3.
 *   dice (B, A, K) fp64: mean_label[b] against EVERY annotator j, label k: 1 if both are empty of k, 0 if exactly one is, else
 *       2 inter / (|a| + |b|) (train_model.py:212-224).
 *   ncc_pairs (B, A) fp32: for image b what uz_ncc_maps + uz_ncc give on soft[:, b] and the one-hot of ann[b], bit for bit (the same
 *       device functions; the one-hot value is read from the uint8 label).  ncc (B) fp64 = (sum_j ncc_pairs[b][j], j = 0 .. A-1) / A.
 * Every output is written once by its owner, nothing is accumulated across launches: a repeated call is bit-equal.
 * 2 <= K <= 8; B, S, A, P >= 1; the element counts of every operand, of `counts` and of the planes must fit int32.  A refused call
 * writes nothing.  workspace: uz_score_workspace bytes (0 for sizes uz_score_samples refuses), 256-byte aligned.                    */
size_t uz_score_workspace(int B, int S, int A, int K, int P);
int uz_score_samples(const uint8_t* labels, const uint8_t* ann, const uint8_t* mean_label, const float* soft,
                     int B, int S, int A, int K, int P, void* workspace,
                     int32_t* counts, double* ged, float* ncc_pairs, double* ncc, double* dice, void* stream);

/* ---------------------------------------------------------------- optimiser / vector ops
 * torch.optim.Adam(lr, betas, eps, weight_decay as L2 added to the gradient): train_model.py:49,122.
 * One launch over a contiguous range of the flat parameter buffer.                        */
int uz_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                 int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                 float grad_scale, void* stream);
int uz_axpy(float* y, const float* x, float alpha, size_t n, void* stream);     /* y += alpha*x */
/* Additive coupling of revtorch's ReversibleBlock (torchlayers.py:55-82: y1 = x1 + F(x2), y2 = x2 + G(y1), and its inversion
 * x2 = y2 - G(y1), x1 = y1 - F(x2) in the recomputing backward pass): y = (accumulate ? y : 0) + a + alpha * b on
 * channel-slice views of C channels (b nullable: plain strided copy / gradient fan-in).                                    */
int uz_add_views(const float* a, int CtotA, const float* b, int CtotB, float* y, int CtotY, int C, int N, int H, int W,
                 float alpha, int accumulate, const float* a_amax, const float* b_amax, float* y_amax, void* stream);
/* slot[0] = max(slot[0], max_i |x_i|) (slot holds a non-negative float; zero it first for a plain maximum) */
int uz_absmax(const float* x, size_t n, float* slot, void* stream);
/* dst bound slot = max(dst, value of src bound slot): forwards a magnitude bound through ops that cannot raise it (pooling, interpolation) */
int uz_absmax_copy(const float* src_slot, float* dst_slot, void* stream);
/* Latent noise eps ~ N(0, 1) (phiseg.py:104 torch.randn_like, probabilistic_unet.py:276 rsample) on the device: Philox4x32-10 +
 * Box-Muller keyed by rng_state = {seed, offset} (two uint64 in DEVICE memory; offset counts 4-float blocks).  uz_step_counters
 * runs behind it: counters[idx[k]] += 1 for the BatchNorm batch counters (num_batches_tracked) of the pass and
 * rng_state.offset += advance - so a replayed launch never repeats a draw.  (uint64_t parameters are passed as pointers / int64.) */
int uz_randn_fill(float* dst, size_t n, const void* rng_state, void* stream);
int uz_step_counters(int64_t* counters, const int64_t* idx, int n_idx, void* rng_state, int64_t advance, void* stream);
/* Device flag word of the split-fp16 convolution path.  The kernels scale every operand by a power of two taken from an upper
 * bound of its tensor's magnitudes; a bound that is too small by more than 4x (a stale parameter bound, a wrong bound passed to a
 * stand-alone call) would overflow fp16.  Such values are CLAMPED to the largest finite fp16 (the result is wrong but never inf /
 * NaN) and a bit is raised here: 1 = activation, 2 = weight, 4 = output gradient.  Synchronises the stream; clear != 0 resets. */
int uz_device_flags(int* out, int clear, void* stream);
/* diagnostics: when buf is non-null the split-fp16 convolution kernels write 8 int64 per workgroup (first 4096 workgroups):
 * shader-clock stamps at start / first tile staged / sum of the staging phases / main loop end / kernel end, the
 * 100 MHz real-time counter at start and end, and the workgroup's tile count (tools/stamp_conv.py).  NULL switches it off. */
void uz_debug_stamps(void* buf);
int uz_scale(float* y, float alpha, size_t n, void* stream);                    /* y *= alpha   */
int uz_zero_f32(float* p, size_t n, void* stream);                              /* p[0..n) = 0  (kernel launch, graph-capturable) */
int uz_copy_f32(float* dst, const float* src, size_t n, void* stream);          /* dst = src    (kernel launch, graph-capturable) */
/* sqrt(sum x^2) terms of utils.l2_regularisation (utils.py:93-101): one norm per tensor of a
 * table of (offset, count) pairs over the flat parameter buffer; out[i] = ||p_i||_2.       */
int uz_l2_norms(const float* flat, const int64_t* offs_counts, int n_tensors, float* out, void* stream);
int uz_l2_norms_bwd(const float* flat, const int64_t* offs_counts, int n_tensors, const float* norms,
                    const float* scale, float* grad_flat, void* stream);          /* g += scale * p / ||p|| */

/* ---------------------------------------------------------------- op tape
 * A forward or backward pass is a static list of the calls above ("tape"), built once by
 * the host for a (model, N, H, W) and replayed with ONE FFI call per pass - or captured
 * into a hipGraph.  What each op's i[] / p[] / f[] slots mean - the tape encoding - is defined in
 * ONE place, the table uz_ops.def next to this header: csrc/tape.hip dispatches by its names,
 * the Python face builds its plans by them, and the op codes below are its entries in order.  */
enum {
  UZ_OP__NONE = 0,       /* no op: a zeroed uz_op is refused */
#define UZ_OP(name, lists) UZ_OP_##name,
#include "uz_ops.def"
#undef UZ_OP
  UZ_OP__COUNT
};
typedef struct uz_op {
  int32_t  code;
  int32_t  i[15];
  float    f[4];
  int64_t  n;          /* element / byte count for the vector ops */
  void*    p[12];
} uz_op;
int uz_run_tape(const uz_op* ops, int n_ops, void* stream);
/* What this binary is: writes a JSON object {variant, products_per_mac, exp_patch_dma, exp_pref_all, diag_skip_compiled, source_hash,
 * experiment} into out (cap bytes) and returns `experiment` (0 for a product build: three piece products per operand pair, no experiment or
 * diagnostic code compiled in).  bench.py prints it in config.build and refuses to report a line from an experiment build. */
int uz_build_info(char* out, int cap);
/* Capture the tape into a hipGraph on `stream` and return an opaque executable handle. */
int  uz_graph_create(const uz_op* ops, int n_ops, void* stream, void** graph_exec_out);
/* Lane capture: like uz_graph_create, but the captured graph carries the tape's dependency DAG
 * instead of one chain.  Ops are partitioned into lanes (each with its own scratch copy, resolved
 * by the host into the op's pointers); op k follows the previous op of its lane and the earlier
 * ops listed in wait[0..n_wait) (which must have signal != 0).  Independent chains of the tape
 * overlap on the device at replay; results are bit-identical to uz_run_tape.                   */
#define UZ_MAX_LANES 8
typedef struct uz_sched {
  int32_t lane;
  int32_t signal;
  int32_t n_wait;
  int32_t wait[UZ_MAX_LANES];
} uz_sched;
int  uz_graph_create_lanes(const uz_op* ops, const uz_sched* sched, int n_ops, int n_lanes,
                           void* stream, void** graph_exec_out);
/* Workgroups a split-path weight gradient (uz_conv_bwd_weight*, 3x3, >= 64 channels) is cut into: a process setting the host makes BEFORE it
 * sizes slab buffers with uz_conv_bwd_weight_slabs and keeps while it runs the calls sized with it (the Python face sets it per model in
 * front of every tape: PHISeg 128, ProbabilisticUnet 192, others 256 = one workgroup per CU).  No counterpart in the reference. */
void uz_set_wgrad_target(int workgroups);   /* a tape whose slab buffers were sized under another target refuses to run (UZ_OP_CONV_BWD_WEIGHT i[12]) */
int  uz_get_wgrad_target(void);
/* The same DAG replayed WITHOUT a hipGraph: lane 0 runs on `stream`, every other lane on a library-owned stream that forks from
 * and joins `stream`; every cross-lane edge is one event that names exactly the op it waits for.  Replaces the reference's
 * implicit stream order (it has none: PyTorch issues phiseg.py:326-537 op by op on one stream). */
int  uz_run_tape_lanes(const uz_op* ops, const uz_sched* sched, int n_ops, int n_lanes, void* stream);
/* diagnostics (tools/lane_trace.py): enable != 0 arms one timing event behind each of the first `capacity` ops of every following
 * uz_run_tape_lanes call; enable == 0 disarms and, with out != NULL, writes the end time (ms since the call began) of every op of the
 * last call and returns their count */
int  uz_lane_trace(int enable, int capacity, float* out, int n_out);
int  uz_graph_launch(void* graph_exec, void* stream);
void uz_graph_destroy(void* graph_exec);

/* ---------------------------------------------------------------- deep-level chain (round 6)
 * The 16 x 16 ... 2 x 2 levels of PHiSeg (phiseg.py:14-39 encoder levels 3 - 6, :42-73 UpConvolutionalBlock, :76-106 SampleZBlock,
 * :209-221 / :269-277 the likelihood's small planes) are ~340 launches of 5 - 40 us per step on the step's critical chains; beside the
 * device-filling convolutions of the other lanes each of them waits 80 - 180 us for a register slot.  uz_chain_run executes a whole
 * sub-DAG of such ops as PHASES of ONE persistent launch: n_workgroups resident workgroups (1024 threads = four waves per SIMD at
 * <= 128 VGPRs, one per CU at most) walk the phase table; the sub-ops of one phase are independent and are cut into tiles (ntiles,
 * counted by uz_chain_op_tiles: WAVE tiles for UZ_CH_CONV3, workgroup tiles otherwise) dealt round-robin to the workgroups starting
 * at workgroup tile0; phases are separated by a grid barrier among
 * the launch's own workgroups (bounded spin: a barrier that does not complete within ~2 s raises the status word and every
 * workgroup leaves - uz_chain_status).  Sub-ops mirror the per-op entry points above (same operands, same results to fp32 rounding;
 * the 3 x 3 convolutions run on the fp16 matrix pipe with two-piece split operands like uz_conv_fwd_ex's split path, staged straight
 * from global memory: no LDS).  Device tables: `ops` = n_ops uz_chain_op in phase order, `phases` = n_phases pairs {first op, op
 * count}; `state` = uz_chain_state_bytes() bytes (zeroed by the call).                                                              */
enum {
  UZ_CH_CONV3 = 1,      /* 3x3 pad 1, contraction channels % 16 == 0, output channels % 32 == 0 (forward and data gradient differ only in the packed image).
                           p = x, image (uz_chain_pack_weights), bias|NULL, y, slabs|NULL, x_amax, w_amax; i = Kc, KcTot, Mc, McTot, N, H, W, S, accumulate.
                           S == 1: y (+)= conv + bias; S > 1: slabs[S][N][Mc][HW] = partial sums (the consumer adds bias + slabs in order) */
  UZ_CH_CONV3_SMALL,    /* 3x3 pad 1 on the vector pipe, contraction channels <= 4 (the 2-channel latents), forward only.
                           p = x, w [Mc][Kc][3][3], bias|NULL, y; i = Kc, KcTot, Mc, McTot, N, H, W */
  UZ_CH_BN_FWD,         /* training-mode BatchNorm + ReLU of one Conv2D unit (torchlayers.py:18-21), N*H*W <= 8192.
                           p = y, gamma, beta, running_mean, running_var, save, a, slabs|NULL, a_amax|NULL, conv bias|NULL; i = C, CtotY, CtotA, N, HW, relu, S; f = eps, momentum */
  UZ_CH_AVGPOOL_FWD,    /* p = x, y, x_amax|NULL, y_amax|NULL; i = C, CtotX, CtotY, N, H, W (input plane) */
  UZ_CH_BILINEAR_FWD,   /* p = x, y, x_amax|NULL, y_amax|NULL; i = C, CtotX, CtotY, N, H, W (input plane), align_corners */
  UZ_CH_HEADS_FWD,      /* uz_latent_heads_fwd with L == 2: p = h, w_mu, b_mu, w_sigma, b_sigma, eps, mu, pre, sigma, z|NULL; i = Cin, CinTot, N, HW, act */
  UZ_CH_BN_BWD,         /* backward of UZ_CH_BN_FWD. p = dA, y, gamma, save, dy [N][C][HW], dgamma, dbeta, dbias|NULL, dy_amax|NULL, slabs|NULL (of dA), beta; i = C, CtotDa, CtotY, N, HW, relu, S */
  UZ_CH_AVGPOOL_BWD,    /* p = dy, dx; i = C, CtotDy, CtotDx, N, H, W (high-resolution plane), accumulate */
  UZ_CH_BILINEAR_BWD,   /* p = dy, dx; i = C, CtotDy, CtotDx, N, H, W (low-resolution plane), align_corners, accumulate */
  UZ_CH_LATENT_HEADS_BWD, /* uz_latent_sample_bwd + uz_latent_heads_bwd_data (L == 2): p = kl_dmu|NULL, kl_dsigma|NULL, dz|NULL, eps, sigma, g_mu (out), g_pre (out), w_sigma, w_mu, dh|NULL; i = Cin, CinTot, N, HW, act, accumulate */
  UZ_CH_CONV3_SMALL_BWD_DATA, /* data gradient of UZ_CH_CONV3_SMALL: p = dy, w [Mc][Kc][3][3], dx; i = Kc (<= 4, channels of dx), KcTot, Mc, McTot, N, H, W, accumulate */
  UZ_CH_SLAB_SUM,       /* dst (+)= sum_s slabs[s] in slab order: p = slabs [S][N][C][HW], dst; i = S, N, C, CtotDst, HW, accumulate */
  UZ_CH__COUNT
};
typedef struct uz_chain_op {
  int32_t code;        /* UZ_CH_* */
  int32_t tile0;       /* first workgroup tile of this sub-op inside its phase */
  int32_t ntiles;      /* uz_chain_op_tiles */
  int32_t rsv;
  int32_t i[16];
  float   f[4];
  void*   p[12];
} uz_chain_op;
int    uz_chain_op_tiles(const uz_chain_op* op);                 /* host: workgroup tiles of one sub-op, < 0 on a shape it does not cover */
int    uz_chain_conv_ksplit(int Kc, int Mc, int N, int H, int W, int n_workgroups);   /* S a UZ_CH_CONV3 of this shape should run with */
size_t uz_chain_packed_bytes(int Kc, int Mc);                     /* bytes of one packed image */
int    uz_chain_pack_blocks(int Kc, int Mc);                      /* 256-thread blocks uz_chain_pack_weights spends on one image */
/* table (device, int64): per layer {w, image, Mc, Kc, Cin of the parameter tensor, dgrad, first block}: image = the two fp16 pieces of
 * w * split_scale(*w_amax) in MFMA fragment order [tap][Kc / 16][Mc / 32][piece][lane][8]; dgrad: rows = input channels, taps flipped */
int    uz_chain_pack_weights(const int64_t* table, int n_layers, int total_blocks, const float* w_amax, void* stream);
size_t uz_chain_state_bytes(void);
int    uz_chain_run(const uz_chain_op* ops, const int32_t* phases, int n_phases, int n_ops, int n_workgroups, void* state, void* stream);
int    uz_chain_status(const void* state, int* out, void* stream);   /* synchronises; out = 0 ok, else 1 + the phase whose barrier timed out */

/* ---------------------------------------------------------------- data-parallel gradient exchange (RCCL over xGMI)
 * New component (the reference has no communication layer): one process per GPU, full replica, and
 * between loss.backward() and optimizer.step() (train_model.py:121-122) the flat fp32 gradient buffer is averaged over the
 * ranks.  librccl.so is bound at run time (uz_comm_load: path or NULL for the default search); the 128-byte unique id is
 * created on rank 0 (uz_comm_unique_id) and handed to the other ranks by the host (torch.distributed store / file / pipe);
 * uz_comm_init is collective.  Every call below is asynchronous on the given stream.                                       */
int  uz_comm_load(const char* librccl_path);
int  uz_comm_version(void);                                   /* RCCL version code, < 0 when RCCL cannot be loaded */
int  uz_comm_unique_id(void* out_128B);
int  uz_comm_init(int rank, int nranks, const void* unique_id_128B, void** comm_out);
void uz_comm_destroy(void* comm);
int  uz_comm_size(void* comm);
int  uz_allreduce_mean_f32(void* comm, float* flat, size_t count, void* stream);         /* in place, ncclAvg */
/* several slices {offset, count} (in floats, pairs in HOST memory) of one buffer in ONE RCCL group launch */
int  uz_allreduce_mean_f32_multi(void* comm, float* flat, const int64_t* offs_counts, int n_slices, void* stream);
int  uz_broadcast_f32(void* comm, float* flat, size_t count, int root, void* stream);
/* streams / events for overlapping the collective with the rest of the backward tape: a UZ_OP_EVENT_RECORD op inside the
 * backward tape (also when the tape is replayed as a hipGraph: external event-record node) marks a gradient bucket final;
 * the communication stream waits for it (uz_stream_wait_event) and runs the bucket's all-reduce beside the remaining
 * backward kernels; the compute stream finally waits for an event recorded behind the last all-reduce.                     */
int  uz_stream_create(void** stream_out, int high_priority);
void uz_stream_destroy(void* stream);
int  uz_stream_synchronize(void* stream);
int  uz_event_create(void** event_out, int timing);
void uz_event_destroy(void* event);
int  uz_event_record(void* event, void* stream);
int  uz_stream_wait_event(void* stream, void* event);
int  uz_event_elapsed_ms(void* start, void* stop, float* ms_out);

/* ---------------------------------------------------------------- input pipeline (data/batch_provider.py:43-67,140-271)
 * One training batch from a dataset resident in HBM: row gather (idx), random annotator (ann), rotation, random crop + resize
 * and flips per sample, images bilinear, labels as one-hot maps with an argmax after each resampling stage (OpenCV rules
 * restated, utils.py:16-36).  X (M,H,W) f32, Y (M,H,W,A) u8; params (B,8) f32 = {do_rot, cos, sin, do_scale, p_x, p_y, r, flips}
 * drawn by the host in the reference's order; outputs x (B,1,H,W) f32 and s (B,H,W) f32.                                    */
int uz_augment_batch(const float* X, const uint8_t* Y, int H, int W, int A, const int* idx, const int* ann,
                     const float* params, int B, int nlabels, float* x_out, float* s_out, void* stream);

/* ---------------------------------------------------------------- volume input pipeline (data/bratsDataset.py:34-96,
 * data/BratsProcessing/augmentation.py:12-104)
 * One BraTS volume, resident in HBM as the HDF5 file stores it, through augment3DImage + random crop + _toEvaluationOneHot + the
 * NCXYZ transpose.  img [X][Y][Z][C] f32 channels last; lbl [X][Y][Z] u8 with the raw values 0, 1, 2, 4, or NULL (hasMasks=False:
 * y_eval and y_raw must be NULL too).  Outputs: x_out (C, Xc, Yc, Zc) f32 planar - PHISeg3D's patch[0] with D = X, H = Y, W = Z;
 * y_eval (3, Xc, Yc, Zc) f32, nullable: l != 0, l != 0 && l != 2, l == 4; y_raw (Xc, Yc, Zc) u8, nullable: the augmented raw label.
 * prm is a HOST table of UZ_AUG3_NPRM doubles drawn by data/brats_dataset.py:draw_augmentation3d in the reference's order:
 *   [0] do_rot [1] cos [2] sin   [3] do_scale [4] sX [5] sY (the integer scaled size round(X scale), round(Y scale))
 *   [6] do_elastic [7..15] dx[9] [16..24] dy[9] (the 3 x 3 displacement matrices, row major)
 *   [25] do_shift [26..29] shift[4]   [30] flips (bit 0, 1, 2 = axis X, Y, Z)   [31] ox [32] oy [33] oz (crop origin)
 * Stages run in the reference's order, each on the result of the one before (two channels-last images in `workspace`, 16-byte
 * aligned, uz_augment_volume_workspace bytes); all in-plane geometry acts on the plane [X][Y] of one z, rows = X, columns = Y:
 *   rotate   source = rot_coords of csrc/augment.hip about (Y/2, X/2) in fp32, BORDER_REPLICATE; image bilinear with clamped taps,
 *            label the voxel at floor(s + 0.5) per axis, clamped;
 *   scale    resize to (sX, sY): image INTER_LINEAR ((o + 0.5) src/dst - 0.5, clamped taps), label INTER_NEAREST min(floor(o src/dst),
 *            src - 1) in fp64; a smaller plane is centred at (X - sX)/2 and the rest filled with voxel [0,0,0,:] of the volume AS IT
 *            ENTERS the stage (labels 0), a larger one centre-cropped at (sX - X)/2;
 *   elastic  dx, dy resized to X x Y with INTER_CUBIC (A = -0.75, taps clamped) in fp64 on the device, map = (float)(index + d);
 *            image: q = rint(32 map) half to even, taps q >> 5 and + 1 with weights (q & 31)/32, BORDER_REFLECT of any distance;
 *            label: the voxel at rint(map), BORDER_REFLECT;
 *   last     shift[c] added to channels 0..3, flips, out[x][y][z] = flipped[x + ox][y + oy][z + oz] - in the last stage's store.
 * 1 <= C <= 8, every element count within int32, shift only with C >= 4 (the reference hard-codes four channels and raises below).
 * A NULL where none is allowed, a crop that leaves the volume or a parameter that is not finite is refused before any launch (-1,
 * uz_last_error names the reason) and nothing is written.  No atomics: every output element is written once, a repeated call is
 * bit-equal.  One thread per voxel, z fastest; with C == 4 and a 16-byte aligned img a tap is one float4, else a scalar path.
 * uz_augment_volume_route (host only, like uz_vol_route; align_img = 16, 8 or 4) answers from the predicate the launch uses:
 * out2[0] = 0 scalar path, 1 float4 path; out2[1] = workgroups of the widest launch a call on this volume can make (a stage over
 * the whole volume, 256 voxels per workgroup).                                                                               */
#define UZ_AUG3_NPRM 34
size_t uz_augment_volume_workspace(int C, int X, int Y, int Z);
int    uz_augment_volume(const float* img, const uint8_t* lbl, int C, int X, int Y, int Z,
                         const double* prm, int Xc, int Yc, int Zc, void* workspace,
                         float* x_out, float* y_eval, uint8_t* y_raw, void* stream);
int    uz_augment_volume_route(int C, int X, int Y, int Z, int align_img, int* out2);

/* ---------------------------------------------------------------- volume scores (data/bratsUtils.py:6-24,57-84)
 * The numbers a BraTS validation reports, of label volumes that are already in HBM (PHISeg3D.predict's samples and mean label, the
 * y_raw of uz_augment_volume).  All volumes are (D, H, W) uint8, W fastest, unit voxel spacing (the reference passes none).
 *
 * uz_vol_edt_sq: d2[v] = min over the voxels u with seeds[u] != 0 of |v - u|^2, an EXACT integer, INT32_MAX everywhere when no voxel
 * is a seed.  Replaces scipy.ndimage.distance_transform_edt(~seeds) inside MedPy 0.4.0's __surface_distances (bratsUtils.py:78-79),
 * which getHd95 runs on the host twice per region and sample.  Three separable passes, W, H, D, all in unsigned integer arithmetic:
 * the W pass is two scans per row (one wave per row), the H and D passes evaluate out[i] = min_j (g[j] + (i - j)^2) directly from a
 * tile of 64 neighbouring columns x up to 128 axis positions in LDS (a longer axis is walked in chunks of 128 j).  The sentinel of "no
 * seed" between the passes is 2^30 and every pass clamps what it stores to it, so g[j] + (i - j)^2 < 2^31 as long as
 * D^2 + H^2 + W^2 <= 2^30: that is the limit (240 x 240 x 155: 139 225).  `workspace`: uz_vol_edt_sq_workspace bytes (one int32 volume),
 * 4-byte aligned like d2.  Refused (-1, nothing written): a null pointer, an empty axis, D*H*W >= 2^31, the limit above, misalignment.
 *
 * uz_vol_region_scores: N label volumes pred (N, D, H, W) against ONE label volume ref for R regions.  A region is a SET of label
 * values, a bit mask in HOST memory: the voxel with label v belongs to region r of pred when bit v of pred_sets[r] is 1 (ref_sets[r]
 * for ref); a value >= 32 belongs to no region.  Raw BraTS labels: WT = bits {1, 2, 4}, TC = {1, 4}, ET = {4} (getWTMask / getTCMask /
 * getETMask, bratsUtils.py:86-93).  Outputs, row n, region r:
 *   counts (N, R, 4) int64 = {tp, |pred|, |ref|, P = D*H*W}, exact (integer atomics);
 *   scores (N, R, 4) fp64  = {dice, sensitivity, specificity, hd95}, each from the integer counts with one fp64 division:
 *     dice        = 2 tp / (|pred| + |ref|), 1 when both are empty (bratsUtils.py:19-21 with the NaN fix of :15);
 *     sensitivity = tp / |ref|, 1 when |ref| = 0 (:57-65);
 *     specificity = (P - |pred| - |ref| + tp) / (P - |ref|) (:67-72); NaN when |ref| = P, as the reference's 0 / 0 is;
 *     hd95        = bratsUtils.py:74-84: -1 when |pred| = 0 or |ref| = 0; else numpy.percentile(., 95) (linear rule: h = 0.95 (n - 1),
 *                   lo = floor(h), v[lo] + (h - lo)(v[lo + 1] - v[lo]) in fp64) of the n surface distances of both directions together:
 *                   sqrt(d2) of the ref border's transform at the voxels of the pred border, and the reverse.  The border of a mask
 *                   is its voxels with one of the six face neighbours outside the mask or outside the volume (binary_erosion with
 *                   connectivity 1 and border_value 0).  The two order statistics are found exactly: an integer histogram over d2
 *                   (per-workgroup LDS part for d2 < 1024, integer atomics beyond it) and a prefix walk.
 *   Exactness: the reference sums 0 / 1 floats in fp32 and is therefore inexact above 2^24 voxels of a region; this call is exact
 *   there and equal to the reference below that size.  No float atomics anywhere: a repeated call is bit-equal.
 * The reference border's transform is built once per region and shared by the N rows: a call with want_hd95 runs R (N + 1)
 * transforms.  With want_hd95 == 0 no transform runs, the workspace shrinks to 16 bytes and the hd95 column is NaN.
 * `workspace`: uz_vol_region_scores_workspace bytes (three int32 volumes and the histogram), 16-byte aligned.
 * Refused (-1, uz_last_error names the reason, nothing written): a null pointer (scores, counts and workspace are all required),
 * N < 1 or N > UZ_VOL_MAX_ROWS, R < 1 or R > UZ_VOL_MAX_REGIONS, the size limits of uz_vol_edt_sq, with want_hd95
 * D^2 + H^2 + W^2 > UZ_VOL_HD95_MAX_SQ (the histogram has one bin per squared distance), a workspace off 16 bytes, counts or scores
 * off 8.  The *_workspace functions return 0 for such sizes.
 * uz_vol_region_scores_route (host only, like uz_vol_route) answers from the predicates the launches use: out4[0], out4[1] = form of
 * the H and the D pass of a transform of this volume (0 the whole axis in one LDS tile, 1 chunks of 128), out4[2] = workgroups of
 * the widest launch of the call (pointers taken as 4-byte aligned), out4[3] = transforms the call runs: R (N + 1), or 0 without hd95. */
#define UZ_VOL_MAX_REGIONS 8
#define UZ_VOL_MAX_ROWS 65536
#define UZ_VOL_HD95_MAX_SQ (1 << 22)
size_t uz_vol_edt_sq_workspace(int D, int H, int W);
int    uz_vol_edt_sq(const uint8_t* seeds, int D, int H, int W, int32_t* d2, void* workspace, void* stream);
size_t uz_vol_region_scores_workspace(int N, int R, int D, int H, int W, int want_hd95);
int    uz_vol_region_scores(const uint8_t* pred, int N, const uint32_t* pred_sets, const uint8_t* ref, const uint32_t* ref_sets, int R,
                            int D, int H, int W, int want_hd95, void* workspace, int64_t* counts, double* scores, void* stream);
int    uz_vol_region_scores_route(int N, int R, int D, int H, int W, int want_hd95, int* out4);

/* ---------------------------------------------------------------- volume components (data/BratsProcessing/utils.py:228-251)
 * keep_largest_connected_components of label volumes that are already in HBM: the step between drawing samples and scoring them.  The
 * reference runs skimage.measure.label(connectivity=1) per label 1, 2, 3 on the host, keeps the blob with the largest area
 * (np.argmax over regionprops, in label order) and zeroes everything else.  Here N volumes (N, D, H, W) uint8, dense, W fastest, go
 * through one call.  Everything is integer and exact; no float atomics, so a repeated call is bit-equal.
 *   Connectivity: face neighbours, 6 in 3-D and 4 when D == 1 (skimage connectivity=1, scipy's default structure), in the two calls
 *   below; the _ex calls further down take 18 and 26 neighbours as well.  Volumes never
 *   connect to each other, rows never across the row end, slices never across the slice end.
 *   A SET is a bit mask of label values 0 .. 31, as uz_vol_region_scores takes regions: a voxel is foreground of set m when bit `label`
 *   of m is 1; a value of 32 or more is in no set.
 * uz_vol_label_components, one set: labels (N, D, H, W) int32 = 0 on background, on foreground 1 + the smallest local linear index
 * (z*H + y)*W + x over the voxel's component (local to its own volume): a canonical labelling, independent of scan order and of the
 * order in which atomics arrive.  sizes (N, D, H, W) int32, nullable = the voxel count of the voxel's component, 0 on background.
 * uz_vol_keep_components, R sets and min_voxels[r] >= 0 in HOST memory; each set is labelled on its own (the sets may be nested or
 * overlap, WT / TC / ET).  A component of set r is KEPT when, with min_voxels[r] == 0, it is the largest component of set r in its
 * volume - among equally large ones the smallest canonical label wins, the component whose first voxel in C order comes first, which
 * is the reference's argmax -, and with min_voxels[r] = m >= 1 when its size is >= m.  A voxel with label l is LISTED when some set
 * contains l.  out (N, D, H, W) uint8 = l when the voxel is listed and for every set that contains l its component in that set is
 * kept; 0 when it is listed and some component fails; an unlisted voxel is 0, or l with keep_unlisted != 0.  A set that is empty in
 * a volume keeps and removes nothing.  Sets {1}, {2}, {3}, min_voxels 0, keep_unlisted 0: the reference function, for a 3-D mask and
 * for a 2-D one (D == 1).  out may not overlap vol: later sets must see the unfiltered input, so in-place is not offered.
 * A union-find with the minimum index as root (csrc/volcomp.hip): x-runs from a ballot per 64 voxels of a row, one union per overlap
 * of two runs in neighbouring rows and slices (agent-scope relaxed atomics only, fetch_min decides; every loop moves to a strictly
 * smaller index or stops and no thread waits for another), one integer add per run for the sizes, one 64-bit maximum per wave for
 * the largest.  All N volumes of one set go through each launch; the sets run one after the other through the same workspace.
 * `workspace`: uz_vol_components_workspace bytes (two int32 per voxel and 8 bytes per volume), 16-byte aligned.
 * Limits: N*D*H*W < 2^31, 1 <= N <= UZ_VOL_MAX_ROWS, 1 <= R <= UZ_VOL_MAX_REGIONS.  Refused before any launch (-1, uz_last_error names
 * the reason, nothing written): a null pointer (sizes excepted), an empty axis, the limits, a negative min_voxels, a workspace off
 * 16 bytes, labels or sizes off 4, out overlapping vol.  uz_vol_components_workspace returns 0 for sizes it refuses.
 * uz_vol_components_route (host only, like uz_vol_region_scores_route) answers from the predicates the launches use: out2[0] = the
 * form (always 0: there is one), out2[1] = workgroups of the widest launch of a call.
 *
 * The _ex calls and uz_vol_fill_holes: wider neighbourhoods, relabelling, hole filling.  Same volumes, sets, workspace bytes and limits.
 *   `connectivity` is 1, 2 or 3, as skimage's `connectivity` and scipy's generate_binary_structure(3, c) define it: two voxels of one
 *   volume are neighbours when every coordinate differs by at most 1 and at most `connectivity` coordinates differ - 6, 18 or 26
 *   neighbours, and with D == 1 there is no z neighbour, so 4, 8 and 8.  Volumes never join; a neighbour outside 0 <= z < D,
 *   0 <= y < H, 0 <= x < W does not exist and is never read.  The labelling stays canonical (1 + the smallest local index) and the
 *   union-find the same: at connectivity >= 2 the merge pass looks, from every foreground voxel, at the rows (z, y-1) and (z-1, y) at
 *   x-1, x, x+1 and at the rows (z-1, y-1) and (z-1, y+1) at x (connectivity 2) or at x-1, x, x+1 (connectivity 3); the first voxel of a
 *   run whose window touches a run of the other row unites the two, and a window that touches two runs unites both.
 * uz_vol_label_components_ex: uz_vol_label_components at `connectivity`; with connectivity 1 the same output.
 * uz_vol_keep_components_ex: uz_vol_keep_components at `connectivity`, with relabel[r] in HOST memory: -1, a voxel that set r removes
 * becomes 0, or a value v in 0 .. 255, it becomes v.  The sets run in order and every set sees the unfiltered input; a set that keeps
 * a voxel writes nothing, and the last set that removes a voxel decides its value; nothing is labelled a second time, so a value
 * written by relabelling is never itself filtered.  With connectivity 1 and relabel all -1 the output of uz_vol_keep_components.
 * uz_vol_fill_holes, R sets with fill_values[r] and max_voxels[r] >= 0 in HOST memory.  The COMPLEMENT of set r is every voxel whose
 * label is not in the set (a value of 32 or more is in it); it is labelled like a set, at `connectivity` - here the BACKGROUND's, as
 * the `structure` of scipy.ndimage.binary_fill_holes is, whose default is 1.  A component of the complement is a HOLE when none of its
 * voxels lies on the volume's border: the six faces for D > 1; for D == 1, an image, the rows y = 0 and y = H-1 and the columns x = 0
 * and x = W-1 only (else an image could have no hole).  out = vol everywhere except in the holes of set r with max_voxels[r] == 0 or
 * with at most max_voxels[r] voxels, which become fill_values[r], a member of set r.  Every set sees vol, not the earlier sets'
 * output, and a later set overwrites an earlier one: with the regions listed from outer to inner the inner region's value wins.
 * out may not overlap vol.  A root is marked as reaching the border by an integer OR into bit 31 of its size word (sizes stay below
 * 2^31): idempotent, so the result does not depend on the order of arrival.  No third volume: the workspace is the same.
 * Refused before any launch, nothing written, uz_last_error beginning with the function's name: what the calls above refuse, a
 * connectivity outside 1 .. 3, relabel[r] outside -1 .. 255, a fill value that is no member of its set, a negative max_voxels.
 * uz_vol_components_route_ex (host only): out2[0] = the merge instance the launches of a call at `connectivity` take (1, 2 or 3),
 * out2[1] = workgroups of the widest launch, as uz_vol_components_route.                                                        */
size_t uz_vol_components_workspace(int N, int D, int H, int W);
int    uz_vol_label_components(const uint8_t* vol, int N, int D, int H, int W, uint32_t set,
                               int32_t* labels, int32_t* sizes, void* workspace, void* stream);
int    uz_vol_keep_components(const uint8_t* vol, int N, int D, int H, int W, const uint32_t* sets, const int32_t* min_voxels, int R,
                              int keep_unlisted, uint8_t* out, void* workspace, void* stream);
int    uz_vol_components_route(int N, int D, int H, int W, int* out2);
int    uz_vol_label_components_ex(const uint8_t* vol, int N, int D, int H, int W, uint32_t set, int connectivity,
                                  int32_t* labels, int32_t* sizes, void* workspace, void* stream);
int    uz_vol_keep_components_ex(const uint8_t* vol, int N, int D, int H, int W, const uint32_t* sets, const int32_t* min_voxels,
                                 const int32_t* relabel, int R, int connectivity, int keep_unlisted, uint8_t* out, void* workspace, void* stream);
int    uz_vol_fill_holes(const uint8_t* vol, int N, int D, int H, int W, const uint32_t* sets, const int32_t* fill_values,
                         const int32_t* max_voxels, int R, int connectivity, uint8_t* out, void* workspace, void* stream);
int    uz_vol_components_route_ex(int N, int D, int H, int W, int connectivity, int* out2);

/* ---------------------------------------------------------------- volume morphology and lesion-wise scores (the BraTS rankings since 2023)
 * uz_vol_morph: binary dilation (erode = 0) or erosion (erode = 1) of the membership mask of N label volumes.  vol (N, D, H, W) uint8,
 * dense, W fastest; foreground is {label in set}, a SET as the components calls take it (a value of 32 or more is in no set).
 * out (N, D, H, W) uint8 = 0 / 1.  The call is scipy.ndimage.binary_dilation / binary_erosion with
 * structure = generate_binary_structure(3, connectivity), iterations = `iterations`, border_value = 0: `iterations` passes of the 7-,
 * 19- or 27-voxel stencil, a voxel outside the volume reading as 0 - an erosion eats inward from the faces, as scipy's does.  With
 * D == 1 there is no z neighbour and the stencil is the 2-D one (5, 9 or 9 voxels), the rule of the labelling calls: scipy on the
 * 2-D array.  Volumes never touch each other, rows never wrap into the next row; iterations == 0 copies the membership mask.
 * Bit planes (csrc/volmorph.hip): the mask is packed once, one 64-bit word per ballot of a wave, rows padded to whole words; every
 * pass works on words - an x step is w | w << 1 | w >> 1 with the carry bits of the neighbouring words of the same row, a y or z
 * step an OR (erosion: AND) with the words of the neighbouring rows, x-widened where one more coordinate may differ - and clears the
 * pad bits of every row's last word; the result is unpacked once.  One launch per pass.  Integer and exact, bit-equal on repetition.
 * `workspace`: uz_vol_morph_workspace bytes (two packed planes), 16-byte aligned; 0 for sizes the call refuses.
 * Refused before any launch (-1, uz_last_error names the reason, nothing written): a null pointer, an empty axis, N < 1 or
 * N > UZ_VOL_MAX_ROWS, N*D*H*W >= 2^31, a connectivity outside 1 .. 3, iterations < 0, erode outside 0 / 1, a workspace off 16 bytes,
 * out overlapping vol.
 * uz_vol_morph_route (host only): out2[0] = the 64-bit words of a packed row, out2[1] = workgroups of the widest launch of a call.
 *
 * uz_vol_lesion_scores: N label volumes pred (N, D, H, W) against ONE label volume ref (D, H, W) for R regions, the operands of
 * uz_vol_region_scores (pred_sets / ref_sets: R bit masks in HOST memory).  The definition below is this library's CONTRACT; it follows
 * the published description of the BraTS 2023 lesion-wise ranking, but parity with the challenge's own tool is not pinned (the tool
 * is not part of the test tier).  For region r and row n let G = the reference voxels in ref_sets[r], P = the row's voxels in
 * pred_sets[r], Dk = G dilated `dilation` times with the 18-neighbour structure (uz_vol_morph, connectivity 2).
 *   1. Reference lesions are the 26-connected components of Dk, numbered g = 0 .. n_ref-1 by ascending canonical label - the order of
 *      their first voxels in C order, scipy.ndimage.label's numbering.  gt_vol[g] = |G and Dk_g|.  Two reference blobs that the
 *      dilation joins are ONE lesion.  Computed once per region: it does not depend on the row.
 *   2. Predicted components are the 26-connected components of P, with their sizes.
 *   3. match(g) = the predicted components with at least one voxel in Dk_g; pred_vol[n][g] = the sum of their FULL sizes, each
 *      component once; inter[n][g] = |G and Dk_g and P|.  A component may match several lesions and counts in the pred_vol of each.
 *      (Dilating every lesion on its own gives the same Dk_g, and every predicted voxel inside Dk_g belongs to a matched component.)
 *   4. A lesion is KEPT when gt_vol[g] >= min_ref_voxels; one that is not kept is dropped from every sum, and a component that
 *      touches a dropped lesion's Dk_g is still no false positive.  A predicted component is a FALSE POSITIVE when it has no voxel
 *      in Dk at all and its size is >= min_pred_voxels.
 *   5. dice_g = 2 inter / (gt_vol + pred_vol), 0 for a missed lesion (pred_vol == 0).  n_tp / n_fn = kept lesions with / without a match.
 *      scores (N, R, 4) fp64 = {lesion_dice = (sum over kept g of dice_g) / (n_kept + n_fp), summed serially in ascending g in fp64;
 *      lesion sensitivity n_tp / n_kept; precision n_tp / (n_tp + n_fp); F1 = 2 n_tp / (2 n_tp + n_fn + n_fp)}; an empty denominator
 *      gives 1.0.  counts (N, R, 8) int64 = {n_ref, n_kept, n_tp, n_fn, n_fp, n_pred, lesions beyond max_lesions, roots with links
 *      beyond max_links}.  lesions (N, R, max_lesions, 3) int64, nullable = {gt_vol, inter, pred_vol} per lesion, 0 beyond n_ref.
 *   Overflow: the tables hold max_lesions lesions and a component is linked to at most max_links lesions.  A lesion beyond the table
 *   keeps its voxels in Dk (a component on it is no false positive) but enters no table and no sum; all such lesions together are one
 *   link.  counts[6] = n_ref - max_lesions when positive, counts[7] = the predicted components that touch more than max_links
 *   different lesions.  Either one non-zero makes the four scores of that (n, r) NaN; the call still returns 0: this is data the
 *   host part cannot see.
 *   6. Lesion-wise HD95 (uz_vol_lesion_scores_ex with want_hd95 != 0; like the rest of this section it follows the challenge's
 *      description, and parity with the challenge's own tool is not pinned).  For a table lesion g with pred_vol[n][g] > 0 let
 *      A_g = G and Dk_g, the lesion's undilated voxels, and B_ng = the union of the predicted components in match(g), each one whole,
 *      as pred_vol counts it (a component that reaches several lesions belongs to the B of each; the links beyond max_links are not
 *      in it).  The border of a mask is the rule of uz_vol_region_scores - a voxel of the mask with a face neighbour outside the mask
 *      or outside the volume -, taken of A_g and of B_ng as masks of their own.  (The kernels use border(A_g) = border(G) and Dk_g,
 *      border(B_ng) = border(P) and B_ng: two face neighbours of G share a lesion, two of P a component.)  S_ng = the multiset of
 *      the exact integer squared distances of both directions: min over u in border(A_g) of |q - u|^2 for every q in border(B_ng),
 *      and min over q in border(B_ng) of |u - q|^2 for every u in border(A_g).  With m = |S_ng| (>= 2), S_ng sorted,
 *      hq = 0.95 (m - 1), k0 = floor(hq), k1 = min(k0 + 1, m - 1): hd95_g = sqrt(s[k0]) + (hq - k0) (sqrt(s[k1]) - sqrt(s[k0])) in
 *      fp64, the percentile rule of uz_vol_region_scores.  hd95 (N, R) fp64 = (sum over kept g of t_g, serially in ascending g in
 *      fp64, + hd95_penalty * n_fp, one product added after the loop) / (n_kept + n_fp), t_g = hd95_g for a matched lesion and
 *      hd95_penalty for a missed one; a dropped lesion enters nothing; 0.0 with no kept lesion and no false positive.  *hd95_penalty
 *      is ONE fp64 in HOST memory, read before the call returns (as the sets are; the challenge's description gives 374 for a missed
 *      lesion or a false positive).  hd_lesions (N, R, max_lesions, 3) int64, nullable = {m, s[k0], s[k1]} for every table lesion
 *      with a match, kept or not, and 0 otherwise.  hd_counts (N, R, 2) int64 = {the border voxels of the table lesions beyond
 *      max_border, the (predicted border voxel, link to a table lesion) entries of the row beyond max_border}: max_border,
 *      1 .. D*H*W, bounds both lists per row.  Where a list overflowed, hd95 of that (n, r) is NaN and its hd_lesions are 0; the four
 *      scores are left alone.  hd95 is NaN too where counts[6] or counts[7] is non-zero.  The call still returns 0.
 * csrc/vollesion.hip: per region uz_vol_morph and two uz_vol_label_components_ex sweeps at connectivity 3 (the reference side on one
 * volume, the prediction side on all N), a two-level count that ranks the root voxels of Dk, and the (component, lesion) pairs
 * counted once each by max_links rounds of an integer fetch_min on one word per component root, the root's own thread adding the
 * component's size behind every round.  Integer atomics only, no float atomics: exact, independent of order, bit-equal on repetition.
 * `workspace`: uz_vol_lesion_scores_workspace bytes, 16-byte aligned: the labelling's workspace for N volumes, the morphology's for
 * one, a uint8 and two int32 volumes for the reference side, two int32 volumes per row, and the tables.
 * Refused before any launch (-1, nothing written): a null pointer (lesions excepted), an empty axis, N < 1 or N > UZ_VOL_MAX_ROWS,
 * R < 1 or R > UZ_VOL_MAX_REGIONS, N*D*H*W >= 2^31, dilation outside 0 .. UZ_VOL_MAX_DILATION, a negative min_ref_voxels or
 * min_pred_voxels, max_lesions outside 1 .. UZ_VOL_MAX_LESIONS, max_links outside 1 .. UZ_VOL_MAX_LINKS, a workspace off 16 bytes,
 * counts, lesions or scores off 8.  uz_vol_lesion_scores_workspace returns 0 for the sizes the call would refuse.
 * uz_vol_lesion_scores_route (host only): out2[0] = the merge instance both labelling sweeps take (3), out2[1] = workgroups of the
 * widest launch of a call.
 * uz_vol_lesion_scores_ex: uz_vol_lesion_scores (which is this call with want_hd95 = 0) and, with want_hd95 != 0, rule 6.  The border
 *   of G is compacted into one list of voxel indices grouped by lesion (count, scan, scatter); in every link round, between offer and
 *   settle, the border voxels of P whose component is about to settle a link are appended as (voxel, lesion) to their row's list, and
 *   after the rounds each row's list is sorted by lesion with a counting sort.  The pair kernel gives a workgroup out4[2] queries of
 *   one (row, lesion) and walks the lesion's border in LDS tiles of out4[3] seeds: a running minimum per query in a register, and with
 *   the roles swapped one integer fetch_min per (seed, workgroup) into the row's copy of the reference list.  One workgroup per
 *   (row, lesion) then selects s[k0] and s[k1] exactly with a radix select on the keys (an LDS histogram per pass), and one thread per
 *   row forms the mean.  Integer arithmetic up to the interpolation, integer atomics only, no host round trip: bit-equal on repetition.
 *   The pair kernel's work is the product of the two border sizes per (row, lesion).
 *   With want_hd95 == 0 the three hd_ pointers, hd95_penalty and max_border are not looked at and nothing of rule 6 is launched or
 *   written; uz_vol_lesion_scores_workspace_ex then equals uz_vol_lesion_scores_workspace.  With want_hd95 the call also refuses a
 *   null hd_counts, hd95 or hd95_penalty, D^2 + H^2 + W^2 > 2^30, max_border outside 1 .. D*H*W, a penalty that is negative or not
 *   finite, and hd_counts, hd_lesions or hd95 off 8 bytes; the workspace grows by lists of max_border entries per row.
 * uz_vol_lesion_scores_route_ex (host only): out4[0], out4[1] as uz_vol_lesion_scores_route; out4[2] = the queries one workgroup of
 *   the pair kernel takes, out4[3] = the seeds of one LDS tile (both 0 with want_hd95 == 0).                                    */
#define UZ_VOL_MAX_DILATION 16
#define UZ_VOL_MAX_LESIONS 4096
#define UZ_VOL_MAX_LINKS 16
size_t uz_vol_morph_workspace(int N, int D, int H, int W);
int    uz_vol_morph(const uint8_t* vol, int N, int D, int H, int W, uint32_t set, int connectivity, int iterations, int erode,
                    uint8_t* out, void* workspace, void* stream);
int    uz_vol_morph_route(int N, int D, int H, int W, int* out2);
size_t uz_vol_lesion_scores_workspace(int N, int R, int D, int H, int W, int max_lesions);
int    uz_vol_lesion_scores(const uint8_t* pred, int N, const uint32_t* pred_sets, const uint8_t* ref, const uint32_t* ref_sets, int R,
                            int D, int H, int W, int dilation, int min_ref_voxels, int min_pred_voxels, int max_lesions, int max_links,
                            void* workspace, int64_t* counts, int64_t* lesions, double* scores, void* stream);
int    uz_vol_lesion_scores_route(int N, int R, int D, int H, int W, int* out2);
size_t uz_vol_lesion_scores_workspace_ex(int N, int R, int D, int H, int W, int max_lesions, int want_hd95, int max_border);
int    uz_vol_lesion_scores_ex(const uint8_t* pred, int N, const uint32_t* pred_sets, const uint8_t* ref, const uint32_t* ref_sets, int R,
                               int D, int H, int W, int dilation, int min_ref_voxels, int min_pred_voxels, int max_lesions, int max_links,
                               int want_hd95, const double* hd95_penalty, int max_border,
                               void* workspace, int64_t* counts, int64_t* lesions, double* scores,
                               int64_t* hd_counts, int64_t* hd_lesions, double* hd95, void* stream);
int    uz_vol_lesion_scores_route_ex(int N, int R, int D, int H, int W, int want_hd95, int* out4);

/* ---------------------------------------------------------------- volume uncertainty (the BraTS uncertainty task; calibration)
 * Judges S sampled label volumes of ONE case as an uncertainty estimate against one reference, per region, from the votes of the
 * samples: with S samples a voxel's region probability takes only the S + 1 values c / S, so one integer table per region holds
 * everything.  Restates the BraTS uncertainty-task evaluation (filtered Dice, filtered true-positive and true-negative ratios over
 * uncertainty thresholds, their areas, score = (AUC_dice + (1 - AUC_ftp) + (1 - AUC_ftn)) / 3) with the levels 0 .. S in the place
 * of its thresholds 0 .. 100, and the usual reliability numbers (ECE, MCE, Brier) with one bin per vote count.  The reference
 * project evaluates no uncertainty; bratsUtils.py:6-24,86-93 gives the Dice convention and the regions.
 *   samples (S, D, H, W) uint8, dense, W fastest; decision and ref (D, H, W) uint8; pred_sets / ref_sets: R bit masks in HOST memory,
 *   exactly as uz_vol_region_scores takes them (a value of 32 or more is in no set).  Per region r and voxel v:
 *     c = number of samples s with samples[s][v] in pred_sets[r];   d = 1 when decision[v] is in pred_sets[r];
 *     t = 1 when ref[v] is in ref_sets[r];   a = d ? S - c : c, the samples that contradict the decision: the uncertainty is a / S.
 *   table (R, S+1, 2, 2) int64: table[r][c][d][t] = number of voxels; the entries of a region sum to P = D*H*W.
 *   levels (R, S+1, 4) int64 = {tp_j, fp_j, fn_j, tn_j} over the voxels kept at level j, those with a <= j:
 *     tp_j = sum_{c >= S-j} T[c][1][1], fp_j = sum_{c >= S-j} T[c][1][0], fn_j = sum_{c <= j} T[c][0][1], tn_j = sum_{c <= j} T[c][0][0];
 *     level S keeps every voxel.
 *   curves (R, S+1, 3) fp64, each ONE division of exact integers: dice_j = 2 tp_j / (2 tp_j + fp_j + fn_j), 1 when the denominator
 *     is 0 (the convention of uz_vol_region_scores); ftp_j = (tp_S - tp_j) / tp_S, 0 when tp_S = 0; ftn_j = (tn_S - tn_j) / tn_S,
 *     0 when tn_S = 0.
 *   auc (R, 4) fp64 = {auc_dice, auc_ftp, auc_ftn, score}: trapezoid sums over the uniform grid j / S,
 *     auc_x = (1/S) sum_{j<S} (x_j + x_{j+1}) / 2, summed in fp64 in the order of j (every term lies in [0, 1]: the error is below
 *     (S + 4) 2^-52); score = (auc_dice + (1 - auc_ftp) + (1 - auc_ftn)) / 3.
 *   calibration (R, 3) fp64 = {ece, mce, brier} with n_c = sum_{d,t} T[c][d][t] and pos_c = sum_d T[c][d][1], each ONE division of
 *     an exact integer numerator: ece = (sum_c |S pos_c - c n_c|) / (S P); mce = max over c with n_c > 0 of |S pos_c - c n_c| / (S n_c);
 *     brier = (sum_c pos_c (S-c)^2 + (n_c - pos_c) c^2) / (S^2 P).  Every numerator and denominator is below 2^53 for P < 2^31 and
 *     S <= 255 (the largest, S^2 P, is below 2^47), so each is exact in fp64 and each quotient is correctly rounded.
 *   votes (R, D, H, W) uint8, nullable = c, the per-region vote map (a BraTS uncertainty submission writes 100 a / S from it).
 * Two launches (csrc/voluncert.hip).  The table pass streams the S + 2 volumes once: a wide form (16 or 4 voxels per thread with
 * 16- or 4-byte loads, when EVERY row samples + s P, decision, ref and votes + r P is so aligned) and a scalar form (any address; it
 * also takes the tail of the wide form); membership by a 256-entry table in LDS, the region tables in LDS as uint32 with LDS
 * atomics, the bin (c, d, t) = (0, 0, 0) counted in registers and added once per wave, words of four background voxels skipped
 * without touching LDS.  No global atomics: every workgroup of a capped, grid-striding grid stores its whole table to its own slice
 * of the workspace, and the finish (one workgroup per region) sums the slices in int64 and forms everything else in integers up to
 * the final divisions.  Exact, independent of order, bit-equal on repetition; nothing depends on the workspace's previous content.
 * `workspace`: uz_vol_uncertainty_workspace bytes (at most 1024 slices of R (S+1) 4 uint32), 16-byte aligned.
 * Refused before any launch (-1, uz_last_error names the reason, nothing written): a null pointer (votes excepted), S < 1 or
 * S > UZ_VOL_UNC_MAX_SAMPLES, R < 1 or R > UZ_VOL_MAX_REGIONS, an empty axis, S*D*H*W >= 2^31, a workspace off 16 bytes, table,
 * levels, curves, auc or calibration off 8.  uz_vol_uncertainty_workspace returns 0 for the sizes the call would refuse.
 * uz_vol_uncertainty_route (host only, like uz_vol_components_route) answers from the predicates the launch uses, for a call WITH
 * votes whose pointers all have byte alignment `align` (1, 2, 4, 8 or 16): out3[0] = 0 the scalar form, 1 the wide form,
 * out3[1] = workgroups of the table pass, out3[2] = 1 when the pass grid-strides (P exceeds what the capped grid covers in one sweep). */
#define UZ_VOL_UNC_MAX_SAMPLES 255
size_t uz_vol_uncertainty_workspace(int S, int R, int D, int H, int W);
int    uz_vol_uncertainty(const uint8_t* samples, int S, const uint8_t* decision, const uint32_t* pred_sets,
                          const uint8_t* ref, const uint32_t* ref_sets, int R, int D, int H, int W,
                          void* workspace, int64_t* table, int64_t* levels, double* curves, double* auc,
                          double* calibration, uint8_t* votes, void* stream);
int    uz_vol_uncertainty_route(int S, int R, int D, int H, int W, int align, int* out3);

/* ---------------------------------------------------------------- volume preparation (data/BratsProcessing/brats18_data_loader.py:31-96,
 * brats18_validation_data_loader.py:27-74) and the way back into native space
 * uz_vol_prepare turns one raw case - the stacked modalities as they come from the challenge - into what the HDF5 file stores:
 * crop_volume_allDim, crop_or_pad_slice_to_size and normalise_image in seven launches on the caller's stream.  The box never visits
 * the host; no host round trip, no synchronisation.
 *   raw (X, Y, Z, C) fp32, channels last; mask (X, Y, Z) uint8, nullable; target extent (Xt, Yt, Zt); placement 0 = centre (the
 *   training loader), 1 = corner (the validation loader).  image (Xt, Yt, Zt, C) fp32; mask_out (Xt, Yt, Zt) uint8, null exactly
 *   when mask is; info int32[16]; stats (C, 3) fp64 = {count, mean, std}.
 *   BOX  per spatial axis the minimum and the maximum + 1 of the index over the voxels where ANY channel is > 0 (np.argwhere(image > 0),
 *   not != 0: a negative value does not open the box, neither does a NaN).
 *   PLACEMENT  per axis a descriptor {n, t, e}: target voxel t + i shows native voxel n + i for 0 <= i < e.  Box [b0, b1), s = b1 - b0,
 *   target T, d = abs(T - s) / 2 (integer division):
 *     centre, T <  s:  n = b0 + d, t = 0, e = T          centre, T >= s:  n = b0, t = d, e = s
 *     corner:          n = b0,     t = 0, e = min(s, T)
 *   The reference's corner placement truncates x only and raises when y or z does not fit; here every axis is truncated.
 *   Everything of the target outside the placed block is 0, in image and in mask_out.
 *   info[0..5] = {x0, y0, z0, x1, y1, z1} the box, [6..8] = n, [9..11] = t, [12..14] = e, [15] = flags: bit 0 = no voxel > 0, bit 1 =
 *   some axis lost voxels (T < s).  With bit 0 every output is 0: image, mask_out, stats and all fifteen descriptor entries.
 *   STATISTICS  per channel over the PLACED voxels with value != 0: a zero inside the box does not count, a negative value does, a
 *   voxel that was cropped away does not.  count = their number; mean = sum / count in fp64; std = sqrt(sum((x - mean)^2) / count) in
 *   fp64 with the unrounded fp64 mean - numpy's two-pass nanstd, ddof = 0, on fp64 input: the validation loader's route.  (The
 *   training loader hands fp32 to nanmean / nanstd; what it gets depends on numpy's fp32 pairwise order and is not restated.)  A
 *   channel without such a voxel has {0, 0, 0} (numpy: NaN and a warning) and its voxels are all 0.  A NaN counts and propagates.
 *   Summation order, fixed: a thread adds its voxels in index order (grid stride), the 64 lanes of a wave by a shuffle tree, the four
 *   waves of a workgroup in order, the workgroup stores to its own slice; the fold adds slices t, t + 256, ... per thread and then the
 *   same tree.  No float atomics: a repeated call is bit-equal.  Error: every fp64 sum of n terms obeys |err| <= (n - 1) 2^-53 sum|term|
 *   to first order whatever the order, so |mean - exact| <= (n - 1) 2^-53 sum|x| / n + 2^-53 |mean| (the division); a term (x - mean)^2
 *   carries three roundings (the difference, the product, or one less with a fused multiply-add), so with V the exact variance and dm
 *   the error of the mean |sum / n - V| <= (n + 3) 2^-53 (V + dm^2) + dm^2, and |std - exact| <= that / sqrt(V) + 2^-52 sqrt(V) (the
 *   division, the square root).  With integer-valued intensities below 2^53 / n the sums of x are exact.
 *   STORE  out = (x == 0) ? 0 : (x - f32(mean)) / f32(std) in fp32: one subtraction and one correctly rounded IEEE division, what
 *   np.divide(image - m, s) does with m, s cast to float32.  std == 0 (one voxel, or a constant channel) gives what IEEE gives: NaN
 *   on that channel's non-zero voxels.
 * Kernels (csrc/volprep.hip): a wide form - C == 4 and raw and image 16-byte aligned: a voxel is one 16-byte load and one 16-byte
 * store - and a scalar form for any C in 1 .. UZ_VOL_PREP_MAX_CHANNELS and any fp32 alignment.  Grids are capped (2048 workgroups of
 * 256 threads) and grid-striding.  Launches: bounds (one read of raw) | fold bounds + descriptor | sums | fold -> count, mean |
 * centred squares | fold -> std | store (with the mask).  The three passes behind the descriptor walk the target extent, whose
 * size the host knows, and touch memory only inside the placed block.
 * `workspace`: uz_vol_prepare_workspace bytes (a 32-byte box slice and a 128-byte sum slice per workgroup), 16-byte aligned; nothing
 * depends on its previous content, nor on that of the outputs.
 * Limits: X*Y*Z*C < 2^31, Xt*Yt*Zt*C < 2^31, 1 <= C <= 8.  Refused before any launch (-1, uz_last_error names the reason, nothing
 * written): a null pointer (mask and mask_out excepted, but only both or neither), an empty axis, the limits, a placement other than
 * 0 / 1, a workspace off 16 bytes, info off 4, stats off 8.  uz_vol_prepare_workspace returns 0 for sizes the call would refuse.
 * uz_vol_prepare_route (host only) answers from the predicates the launches use, for raw and image of byte alignment `align` (4, 8
 * or 16): out3[0] = 0 the scalar form, 1 the wide form; out3[1] = workgroups of the widest pass (bounds walks X*Y*Z voxels, the
 * others Xt*Yt*Zt); out3[2] = 1 when that pass grid-strides.
 *
 * uz_vol_restore puts N rows of target extent back into native volumes: label maps, vote maps (uint8) or entropy maps (fp32).
 *   rows (N, Xt, Yt, Zt) and out (N, X, Y, Z) of one element type, elem = 1 (uint8) or 4 (fp32); place int32[9] in DEVICE memory =
 *   info[6..14] of uz_vol_prepare = {n, t, e}.  Native voxel v takes target voxel t + (v - n) where 0 <= v - n < e on all three axes,
 *   and `fill` elsewhere; every output element is written exactly once.  fill: one element of that type in HOST memory.
 *   lut: 256 bytes in HOST memory, nullable, uint8 rows only: out = lut[row value] (class index -> raw label {0, 1, 2, 4}).  It maps
 *   the rows, never the fill.  It is copied into the launch arguments: the caller need not keep it alive.
 *   `place` is data the host cannot see: the kernel clips per voxel (the ranges are intersected in 64-bit arithmetic, any nine int32)
 *   and never reads outside rows.
 * One thread per element, or per W consecutive elements with one 4- / 16-byte store where out is so aligned: W = 16 (uint8, out on 16
 * bytes) or 4 (uint8, out on 4; fp32, out on 16).  The source is read element by element (Z is odd in real cases) and its row is
 * looked up once per (n, x, y); the tail of N*X*Y*Z % W elements goes one per thread.
 * Limits: N*X*Y*Z < 2^31, N*Xt*Yt*Zt < 2^31.  Refused before the launch: a null pointer (lut excepted), an empty axis, N < 1, the
 * limits, elem other than 1 / 4, a non-null lut with elem = 4, fp32 rows or out off 4 bytes, place off 4, out overlapping rows.
 * uz_vol_restore_route (host only), for an `out` of byte alignment `align`: out3[0] = W, the elements a thread writes (1, 4 or 16);
 * out3[1] = workgroups; out3[2] = 0 (one sweep, always). */
#define UZ_VOL_PREP_MAX_CHANNELS 8
size_t uz_vol_prepare_workspace(int C, int X, int Y, int Z, int Xt, int Yt, int Zt);
int    uz_vol_prepare(const float* raw, const uint8_t* mask, int C, int X, int Y, int Z, int Xt, int Yt, int Zt, int placement,
                      void* workspace, float* image, uint8_t* mask_out, int32_t* info, double* stats, void* stream);
int    uz_vol_prepare_route(int C, int X, int Y, int Z, int Xt, int Yt, int Zt, int align, int* out3);
int    uz_vol_restore(const void* rows, int elem, int N, int Xt, int Yt, int Zt, const int32_t* place, const uint8_t* lut,
                      const void* fill, void* out, int X, int Y, int Z, void* stream);
int    uz_vol_restore_route(int elem, int N, int X, int Y, int Z, int align, int* out3);

/* ---------------------------------------------------------------- volumes (models/phiseg3D.py), one sample
 * A volume is stored [D + 2][C][H][W] (zero slice before and after the D real ones) = a batch of D 2-D images.  Conv3d(3x3x3,
 * pad 1) (phiseg3D.py:24) then is uz_conv_fwd / uz_conv_bwd_* with the depth window as 3 C input channels (pointer = slice d-1,
 * Cin = 3 C, CinTot = C) and permuted weights: mode 0 forward [co][kd][ci][9], mode 1 data gradient [(j, co)][ci][9] (kd = 2 - j),
 * mode 2 weight gradient back to the parameter layout [co][ci][kd][9].  BatchNorm3d / ReLU / 1x1x1 heads run their 2-D entry
 * points over the D slices.  AvgPool3d(2, 2, ceil_mode) (phiseg3D.py:101); depth stage of F.interpolate(mode='trilinear',
 * scale_factor=2, align_corners=True) (phiseg3D.py:146,306,376 - the in-plane stage is uz_bilinear2x_*); nearest volume resize.
 * Pointers address slice 0 of the REAL slices; (D, H, W) are input sizes.                                                     */
int uz_w3d_permute(const float* src, float* dst, int Cout, int Cin, int mode, void* stream);
int uz_avgpool3d_fwd(const float* x, int C, int CtotX, float* y, int CtotY, int D, int H, int W, void* stream);
int uz_avgpool3d_bwd(const float* dy, int C, int CtotDy, float* dx, int CtotDx, int D, int H, int W, int accumulate, void* stream);
int uz_depth_lerp2x_fwd(const float* x, int C, int CtotX, float* y, int CtotY, int D, int H, int W, void* stream);
int uz_depth_lerp2x_bwd(const float* dy, int C, int CtotDy, float* dx, int CtotDx, int D, int H, int W, int accumulate, void* stream);
int uz_nearest3d_fwd(const float* x, int C, int CtotX, float* y, int CtotY, int D, int H, int W, int f, int fz, void* stream);
int uz_nearest3d_bwd(const float* dy, int C, int CtotDy, float* dx, int CtotDx, int D, int H, int W, int f, int fz, int accumulate, void* stream);
/* What a volume call launches, answered on the host from the very route functions the entry points dispatch through (the library
 * loads without a GPU).  op: 0 uz_avgpool3d_fwd, 1 uz_avgpool3d_bwd, 2 uz_depth_lerp2x_fwd, 3 uz_depth_lerp2x_bwd, 4 uz_nearest3d_fwd,
 * 5 uz_nearest3d_bwd, 6 - 9 the *_b16 forms of 0 - 3, 10 uz_w3d_permute (C = Cout, D = Cin), 11 uz_cvt_f32_to_b16 / uz_cvt_b16_to_f32
 * of C*D*H*W elements.  C, D, H, W as the entry point takes them; f, fz = the factors of ops 4 and 5 (unused elsewhere); align_* =
 * byte alignment (16, 8 or 4) of the views the dispatch inspects: src = x / dy, dst = y / dx.  out2 receives
 *   [0] kernel: 0 scalar, 1 float4, 2 bf16 storage (float4 wide), 3 one wave per element (nearest backward from 64 children on);
 *   [1] workgroups along grid.x: per plane for ops 0 - 9 (256 elements, float4s or float2 pairs per workgroup, capped at 64 - the
 *       grid-stride loop covers the rest; kernel 3: four elements per workgroup, uncapped), in all for ops 10 (cap 2 048) and 11
 *       (cap 65 535).
 * Returns 0, or -1 for arguments no entry point accepts (empty tensor, a *_b16 form off its float4 shape or alignment).            */
int uz_vol_route(int op, int C, int D, int H, int W, int f, int fz, int align_src, int align_dst, int* out2);

/* ---------------------------------------------------------------- bf16 storage (BASELINE config 5: PHiSeg3D "bf16"; phiseg3D.py:13-35)
 * A tensor in bf16 storage has the same N x C x H x W shape with 2-byte elements (round to nearest even when written, widened exactly
 * when read); every arithmetic stays what the fp32-storage entry points do in the single-piece bf16 mode (uz_set_conv_math(3)):
 * bf16 operands, fp32 accumulation, fp32 / fp64 BatchNorm statistics (of the STORED values), fp32 parameters and gradients.  Each
 * tensor operand of these entry points carries its own flag (0 = fp32, 1 = bf16), so a plan may keep any subset of its buffers in
 * bf16.  Scope: the large planes of a volume - 3x3 convolutions on the matrix-pipe path with an unsplit chunk loop (weight
 * gradient: rows a multiple of 32 wide), the large-plane BatchNorm path (N*H*W > 32 768, H*W % 4 == 0), AvgPool3d and the depth
 * stage of the trilinear interpolation.  Replaces, for such tensors: uz_conv_fwd_packed / uz_conv_bwd_data_packed /
 * uz_conv_bwd_weight_ex, uz_bn_relu_fwd_pre / uz_bn_relu_bwd, uz_avgpool3d_* / uz_depth_lerp2x_*.                               */
int uz_conv_fwd_b16(const void* x, int Cin, int CinTot, const float* w, const float* bias,
                    void* y, int Cout, int CoutTot, int N, int H, int W, int ks,
                    void* workspace, size_t workspace_bytes, const void* packed_w, float* bn_partials,
                    int x_b16, int y_b16, void* stream);
int uz_conv_bwd_data_b16(const void* dy, int Cout, int CoutTot, const float* w, void* dx, int Cin, int CinTot,
                         int N, int H, int W, int ks, int accumulate,
                         void* workspace, size_t workspace_bytes, const void* packed_w, int dy_b16, int dx_b16, void* stream);
int uz_conv_split_parts(int kind, int Cin, int Cout, int N, int H, int W);   /* chunk-loop split of the matrix-pipe kernel (kind 0 forward, 1 data gradient); the *_b16 convolutions need 1 */
int uz_conv_bwd_weight_b16(const void* x, int Cin, int CinTot, const void* dy, int Cout, int CoutTot,
                           float* dw, int N, int H, int W, int ks, void* workspace, size_t workspace_bytes,
                           int x_b16, int dy_b16, float* slabs_out, void* stream);
int uz_bn_relu_fwd_b16(const void* y, int C, int CtotY, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, float* save_mean_rstd,
                       void* a, int CtotA, int N, int H, int W, float eps, float momentum, int training, int relu,
                       void* workspace, const float* conv_partials, int n_partials, int y_b16, int a_b16, void* stream);
int uz_bn_relu_bwd_b16(const void* da, int CtotDa, const void* y, int C, int CtotY,
                       const float* gamma, const float* beta, const float* save_mean_rstd,
                       void* dy, int CtotDy, float* dgamma, float* dbeta, float* dbias,
                       int N, int H, int W, int relu, void* workspace, int da_b16, int y_b16, int dy_b16, void* stream);
int uz_avgpool3d_fwd_b16(const void* x, int C, int CtotX, void* y, int CtotY, int D, int H, int W, int x_b16, int y_b16, void* stream);
int uz_avgpool3d_bwd_b16(const void* dy, int C, int CtotDy, void* dx, int CtotDx, int D, int H, int W, int accumulate, int dy_b16, int dx_b16, void* stream);
int uz_depth_lerp2x_fwd_b16(const void* x, int C, int CtotX, void* y, int CtotY, int D, int H, int W, int x_b16, int y_b16, void* stream);
int uz_depth_lerp2x_bwd_b16(const void* dy, int C, int CtotDy, void* dx, int CtotDx, int D, int H, int W, int accumulate, int dy_b16, int dx_b16, void* stream);
/* in-plane stage of the trilinear interpolation: the HIGH-resolution side (y; dy) in bf16 storage, the low-resolution side fp32 */
int uz_bilinear2x_fwd_b16(const float* x, int C, int CtotX, void* y, int CtotY, int N, int H, int W, int align_corners, int y_b16, void* stream);
int uz_bilinear2x_bwd_b16(const void* dy, int C, int CtotDy, float* dx, int CtotDx, int N, int H, int W, int align_corners, int accumulate, int dy_b16, void* stream);
/* 1x1(x1) heads with 1 .. 8 outputs (mu_conv / sigma_conv phiseg3D.py:83-84, s_layer): the many-channel operand (x; dx of the data
 * gradient) in bf16 storage, the few-channel side (y, dy) fp32.  Replace uz_conv_fwd / uz_conv_bwd_data / uz_conv_bwd_weight (ks = 1). */
int uz_conv1x1_fwd_b16(const void* x, int Cin, int CinTot, const float* w, const float* bias, float* y, int Cout, int CoutTot,
                       int N, int H, int W, int x_b16, void* stream);
int uz_conv1x1_bwd_data_b16(const float* dy, int Cout, int CoutTot, const float* w, void* dx, int Cin, int CinTot,
                            int N, int H, int W, int accumulate, int dx_b16, void* stream);
int uz_conv1x1_bwd_weight_b16(const void* x, int Cin, int CinTot, const float* dy, int Cout, int CoutTot, float* dw, float* db,
                              int N, int H, int W, void* workspace, size_t workspace_bytes, int x_b16, void* stream);
/* element-wise conversions between the two storage formats (n elements, contiguous) */
int uz_cvt_f32_to_b16(const float* src, void* dst, size_t n, void* stream);
int uz_cvt_b16_to_f32(const void* src, float* dst, size_t n, void* stream);

/* Fcomb input (probabilistic_unet.py:172-197) */
/* z (N,L) tiled over HxW into channels of a (N,Ctot,H,W) buffer, and its backward (sum over pixels) */
int uz_bcast_channels_fwd(const float* z, int L, float* y, int CtotY, int N, int H, int W, void* stream);
int uz_bcast_channels_bwd(const float* dy, int CtotDy, int L, float* dz, int N, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UZ_API_H */
