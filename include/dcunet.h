/* dcunet.h -- C ABI of libdcunet.so: the UNet2DS hot path as gfx950 HIP kernels.
 *
 * The reference (alexklibisz/deep-calcium) has no FFI for this path: every op
 * below is a Keras-2.0.6/TF-1.2.1 layer instantiated by unet() at
 * /root/reference/deepcalcium/models/neurons/unet_2d_summary.py:123-224 and run
 * through model.fit_generator (:429) / model.predict (:87, :588, :592).  Each
 * entry point names the reference call site whose arithmetic it replaces; the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All pointers are DEVICE pointers (plain pointers, no torch types); the one
 *     exception, dc_crop_augment's `items_host`, says so in its name.
 *   - Activations NHWC fp32; conv kernels HWIO (3,3,Cin,Cout); transposed-conv
 *     kernels (2,2,Cout,Cin)  -- Keras `channels_last` layouts.
 *   - "ld" arguments are pixel strides in floats: a tensor argument `p, ld`
 *     addresses channel c of pixel i at p[i*ld + c] (lets producers write into
 *     channel slices of a concat buffer; pass ld == C for a dense tensor).
 *   - The library never allocates, frees or retains DEVICE memory; workspaces
 *     are caller-allocated (sizes from the *_ws_floats helpers).  There is no
 *     hipMalloc / hipFree / hipStreamSynchronize anywhere in the library.
 *   - Every launch is asynchronous on `stream` (a hipStream_t passed as void*;
 *     NULL = the legacy default stream).  The caller sets the device.
 *   - Return value: 0 OK, -1 invalid argument/shape/alignment, -2 HIP runtime
 *     error, -3 unsupported shape.  dc_last_error() returns a thread-local message.
 *   - Channel counts must be multiples of 4 (except the 1-channel network input
 *     and the 2-logit head) and powers of two where noted.
 */
#ifndef DCUNET_H
#define DCUNET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* dc_stream_t;

/* ABI revision: dc_version() of the loaded library must EQUAL the DC_ABI_VERSION of the header the caller was built /
 * bound against (argument lists change between revisions; the Python binding refuses a mismatch). */
#define DC_ABI_VERSION 132
int dc_version(void);
const char* dc_last_error(void);

/* The frames of ONE call: every device entry point that takes `int tc` refuses tc > DC_FRAMES_PER_CALL_MAX = 2^30 with
 * DC_EUNSUP (-3) before it launches anything (a longer recording arrives in chunks, as every reader of the package feeds it).
 * Below the limit the kernels' per-frame table indices 2 * f + 1 and their frame loops' f + gridDim.y (at most 65535) fit an
 * int; the contract no longer relies on the caller for that.  The limits on t0 + tc, T * H * W and H * W stay as they are. */
#define DC_FRAMES_PER_CALL_MAX 1073741824L

/* ---- weight re-layout for the implicit-GEMM kernels -------------------------
 * dst[tap][k/4][n][k%4] = src[(flip ? taps-1-tap : tap)*s_tap + k*s_k + n*s_n].
 *   conv3x3 fwd  : taps 9, K=Cin,  Ncols=Cout, s_tap=Cin*Cout, s_k=Cout, s_n=1,   flip 0
 *   conv3x3 dgrad: taps 9, K=Cout, Ncols=Cin,  s_tap=Cin*Cout, s_k=1,    s_n=Cout, flip 1
 *   convT   fwd  : taps 1, K=Cin,  Ncols=4*Cout, s_tap=0,      s_k=1,    s_n=Cin,  flip 0
 *   convT   dgrad: taps 4, K=Cout, Ncols=Cin,  s_tap=Cout*Cin, s_k=Cin,  s_n=1,    flip 0   */
int dc_pack_weights(const float* src, float* dst, int taps, int K, int Ncols,
                    long s_tap, long s_k, long s_n, int flip, dc_stream_t stream);

/* ---- Conv2D(nf,(3,3),'same')  unet_2d_summary.py:164-165 ---------------------
 * z = conv(x, w) + bias ; optional per-channel (sum, sumsq) partials of z for
 * BatchNorm (stats != NULL: double[tiles][Cout][2], tiles = dc_conv3x3_tiles(); formed per tile from shifted sums
 * and Chan merges, so the variance survives |mean| >> sigma -- csrc/common.h DcMoments);
 * optional fused inference epilogue y = relu?(z*scale + shift).
 * wp = dc_pack_weights(conv3x3 fwd form).  x: [N,H,W,Cin] dense, z: [N,H,W,Cout] with pixel stride z_ld. */
int dc_conv3x3_tiles(int N, int H, int W, int Cout);
int dc_conv3x3_fwd(const float* x, const float* wp, const float* bias, float* z, long z_ld, double* stats,
                   const float* scale, const float* shift, int relu,
                   int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
/* First layer (Cin == 1): x is the (N,H,W) image itself, w is the plain HWIO (3,3,1,Cout) kernel.
 * stats: double[dc_conv3x3_c1_tiles()][Cout][2].  out_absmax (nullable, float[Cout], zeroed by the caller): max |output|
 * per channel is folded in (atomic max) -- the range-guard bound of the next f16x3 layer in inference. */
int dc_conv3x3_c1_tiles(int N, int H, int W, int Cout);
int dc_conv3x3_c1_fwd(const float* x, const float* w, const float* bias, float* z, long z_ld, double* stats,
                      const float* scale, const float* shift, int relu, float* out_absmax, long out_absmax_ld,
                      int N, int H, int W, int Cout, dc_stream_t stream);
/* dx = conv3x3_transpose(dz): wp = dc_pack_weights(conv3x3 dgrad form). dz: [N,H,W,Cout], dx: [N,H,W,Cin]. */
int dc_conv3x3_dgrad(const float* dz, const float* wp, float* dx,
                     int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
/* dW (HWIO) = sum_p x[p+tap] (x) dz[p].  ws: float[dc_conv3x3_wgrad_ws_floats()] scratch (split-K slabs,
 * reduced in a fixed order => bit-reproducible). */
long dc_conv3x3_wgrad_ws_floats(int N, int H, int W, int Cin, int Cout);
int dc_conv3x3_wgrad(const float* x, const float* dz, float* dw, float* ws,
                     int N, int H, int W, int Cin, int Cout, dc_stream_t stream);

/* ---- split-fp16 ("f16x3") variants: same contraction on the fp16 matrix cores with fp32-grade accuracy ----
 * Every fp32 operand is split exactly into hi + lo fp16 (22-bit significand) and hi*hi + hi*lo + lo*hi is
 * accumulated in fp32: 3 fp16 MFMAs replace 8 fp32 ones.  wp16 = dc_pack_weights_f16x3 (same forms/strides as
 * dc_pack_weights; dc_pack_weights_f16x3_floats() floats of storage).
 * fp16's exponent range is covered by exact POWER-OF-TWO operand scales, undone in the epilogue:
 *   - weights: dc_pack_weights_f16x3 brings max|w| into [2^10, 2^11) and stores the scale in a 16-byte trailer of wp16;
 *   - gradient operands: in_scale / dz_scale, a nullable DEVICE scalar from dc_bn_bwd_apply_finalize;
 *   - activation operands: in_abound / x_abound, a nullable per-channel magnitude bound (float[Cin]) written by the
 *     layer that produced the tensor -- dc_bn_stats_finalize_affine / dc_bn_relu_drop_fwd in training
 *     (|gamma|*sqrt(count)+|beta|, valid for ANY data), the out_absmax of the producing kernel in inference; the
 *     consumer scales so that the largest bound lands in [2^14, 2^15): no activation can reach fp16 inf, tiny
 *     ones keep their low bits.  NULL = scale 1.
 *   Measured bounds (inference) live in DC_ABOUND_SLOTS = 8 replicas of the per-channel array, `*_ld` floats apart: a
 *   producer folds max |output| into replica (workgroup id mod 8) with an atomic max (out_absmax, out_absmax_ld; the
 *   caller zeroes all replicas first), the consumer takes the max over the replicas (in_abound_ld > 0).
 *   in_abound_ld == 0: a single array (the training-mode bound).
 *   out_absmax_ld == -1 (optimistic inference): nothing is measured; out_absmax[0] is set to 1 if any output exceeds
 *   32768 (or is NaN) -- the caller then repeats the forward pass with measured bounds.  A BatchNorm network's
 *   activations are O(1), so this path normally runs with no guard traffic at all.
 *   Narrow launches (images of at most 16 x 16 pixels whose grid would leave most of the chip idle: the 256- / 512-channel
 *   layers of a 128^2 / 96^2 training window) are split over K into 2-4 slabs and combined by a second launch in a fixed
 *   order (bit-reproducible; dc_conv3x3_tiles() rows unchanged).  The slabs live in the CALLER's `splitk_ws`
 *   (float[dc_conv3x3_splitk_ws_floats()] / float[dc_convT2x2_dgrad_splitk_ws_floats()]; 0 floats: this shape never
 *   splits); splitk_ws == NULL: the launch is not split (same result up to summation order).  One workspace serves the
 *   launches of ONE stream: launches on different streams that may run concurrently need their own. */
#define DC_ABOUND_SLOTS 8
long dc_pack_weights_f16x3_floats(int taps, int K, int Ncols);
int dc_pack_weights_f16x3(const float* src, void* dst, int taps, int K, int Ncols,
                          long s_tap, long s_k, long s_n, int flip, dc_stream_t stream);
/* every layer's dc_pack_weights_f16x3 in ONE launch.  jobs_dev: device array of (njobs + 1) x 10 longs,
 *   { src pointer, dst pointer, taps, K, Ncols, s_tap, s_k, s_n, flip, first block of the job };
 * the trailing sentinel entry only carries the grid size (= total_blocks) in its last field. */
int dc_pack_weights_f16x3_batch(const long* jobs_dev, int njobs, int total_blocks, dc_stream_t stream);
/* floats of split-K scratch a conv3x3 launch of this shape may use: forward incl. the _bnin variant (dgrad == 0) or plain
 * data gradient (dgrad != 0). */
long dc_conv3x3_splitk_ws_floats(int N, int H, int W, int Cin, int Cout, int dgrad);
long dc_convT2x2_dgrad_splitk_ws_floats(int N, int H, int W, int Cin, int Cout);
/* BatchNorm-partial rows of a split-fp16 conv3x3 forward.  stats_rows == 0 (or dc_conv3x3_tiles()): one row per pixel tile,
 * double[dc_conv3x3_tiles()][Cout][2].  stats_rows == dc_conv3x3_stats_rows(): where the persistent role-split kernel serves the
 * launch, every (workgroup, consumer set) Chan-merges the tiles it computes and writes ONE row -- at most 2 x #CUs rows instead
 * of up to 8 192, so the finalize launch that follows reads KBs instead of MBs (86 -> < 10 us at 512^2 x 16); the per-channel
 * statistics they finalize to are the same up to fp32 rounding of the merges.  For launches the role-split kernel does not
 * serve the query returns dc_conv3x3_tiles().  Needs the current device's CU count: call it on the GPU box. */
int dc_conv3x3_stats_rows(int N, int H, int W, int Cin, int Cout);
int dc_conv3x3_fwd_f16x3(const float* x, const void* wp16, const float* bias, float* z, long z_ld, double* stats, int stats_rows,
                         const float* scale, const float* shift, int relu, const float* in_abound, long in_abound_ld,
                         float* out_absmax, long out_absmax_ld, float* splitk_ws, int N, int H, int W, int Cin, int Cout,
                         dc_stream_t stream);
/* data gradients: the power-of-two scale of dz comes EITHER as a device scalar (dz_scale, from dc_pow2_scale_from_absmax /
 * dc_bn_bwd_apply_finalize; nullable = 1) OR as the per-block max |dz| array dc_bn_bwd_apply wrote (dz_absmax[dz_absmax_n]):
 * every workgroup then derives the same power of two itself (target 1024), and no finalize launch sits between the
 * BatchNorm-backward apply pass and the data gradient.  Pass at most one of the two. */
int dc_conv3x3_dgrad_f16x3(const float* dz, const void* wp16, float* dx, const float* dz_scale,
                           const float* dz_absmax, int dz_absmax_n, float* splitk_ws,
                           int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
int dc_convT2x2_fwd_f16x3(const float* x, const void* wp16, const float* bias, float* z, long z_ld, double* stats,
                          const float* scale, const float* shift, int relu, const float* in_abound, long in_abound_ld,
                          float* out_absmax, long out_absmax_ld, int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
int dc_convT2x2_dgrad_f16x3(const float* dz, const void* wp16, float* dx, const float* dz_scale,
                            const float* dz_absmax, int dz_absmax_n, float* splitk_ws,
                            int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
/* BatchNorm-partial rows (`tiles`) of the split-fp16 conv-transpose forward: it runs wider column blocks than the fp32 kernel
 * (256 / 128 columns per workgroup: each staged input tile feeds 4x / 2x the MFMAs) on correspondingly flatter pixel tiles,
 * so its stats buffer is double[dc_convT2x2_f16x3_tiles()][4*Cout][2] -- NOT dc_convT2x2_tiles(), which sizes dc_convT2x2_fwd's. */
int dc_convT2x2_f16x3_tiles(int N, int H, int W, int Cout);
/* weight gradients: same workspace (dc_*_wgrad_ws_floats) and fixed-order slab reduction as the fp32 entry points;
 * dz_scale = device scalar from dc_pow2_scale_from_absmax (nullable). */
int dc_conv3x3_wgrad_f16x3(const float* x, const float* dz, float* dw, float* ws, const float* dz_scale,
                           const float* x_abound, int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
int dc_convT2x2_wgrad_f16x3(const float* x, const float* dz, float* dw, float* ws, const float* dz_scale,
                            const float* x_abound, int N, int H, int W, int Cin, int Cout, dc_stream_t stream);

/* ---- BatchNorm + ReLU applied ON LOAD ("bnin"): the layer input is a NON-materialised activation -------------
 * Conv2D -> BatchNormalization -> Activation('relu') (unet_2d_summary.py:164-167) feeding the next Conv2D /
 * Conv2DTranspose / head with no Dropout or pooling in between never needs its activation in HBM: the consumer
 * takes the producer's pre-BN tensor z_in plus the per-channel training-mode affine
 *     in_scale[c] = gamma*invstd,  in_shift[c] = beta - mean*in_scale[c]      (dc_bn_stats_finalize_affine)
 * and forms relu(fmaf(z, in_scale, in_shift)) while staging the operand; zero padding stays zero.  Saves one HBM
 * write + one read of the activation per such layer (dc_bn_relu_drop_fwd is skipped).  Other arguments exactly as
 * in the entry point without _bnin. */
/* abound (nullable, float[C]): the activation's per-channel magnitude bound |gamma|*sqrt(count) + |beta| for the
 * consumers' fp16 range guard. */
int dc_bn_stats_finalize_affine(const double* partial, int parts, int groups, int C, double count, float eps,
                                float momentum, float* mean, float* invstd, float* moving_mean, float* moving_var,
                                const float* gamma, const float* beta, float* scale, float* shift, float* abound,
                                dc_stream_t stream);
int dc_conv3x3_fwd_bnin_f16x3(const float* z_in, const float* in_scale, const float* in_shift, const float* in_abound,
                              const void* wp16, const float* bias, float* z, long z_ld, double* stats, int stats_rows, const float* scale,
                              const float* shift, int relu, float* splitk_ws, int N, int H, int W, int Cin, int Cout,
                              dc_stream_t stream);
int dc_convT2x2_fwd_bnin_f16x3(const float* z_in, const float* in_scale, const float* in_shift, const float* in_abound,
                               const void* wp16, const float* bias, float* z, long z_ld, double* stats, const float* scale,
                               const float* shift, int relu, int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
int dc_conv3x3_wgrad_bnin_f16x3(const float* z_in, const float* in_scale, const float* in_shift, const float* in_abound,
                                const float* dz, float* dw, float* ws, const float* dz_scale, int N, int H, int W,
                                int Cin, int Cout, dc_stream_t stream);
int dc_convT2x2_wgrad_bnin_f16x3(const float* z_in, const float* in_scale, const float* in_shift, const float* in_abound,
                                 const float* dz, float* dw, float* ws, const float* dz_scale, int N, int H, int W,
                                 int Cin, int Cout, dc_stream_t stream);
int dc_head_fwd_bnin(const float* z_in, const float* in_scale, const float* in_shift, const float* kh, const float* bh,
                     const uint8_t* y, float* p, float* partial, long pixels, int C, dc_stream_t stream);
int dc_head_bwd_bnin(const float* z_in, const float* in_scale, const float* in_shift, const float* p, const uint8_t* y,
                     const float* kh, float* da, float* partial, int loss_kind, const double* sums, long pixels, int C,
                     dc_stream_t stream);


/* ---- Conv2DTranspose(nf, 2, strides=2)  unet_2d_summary.py:156-157 -----------
 * x: [N,H,W,Cin] -> z: [N,2H,2W,Cout].  wp = dc_pack_weights(convT fwd form).
 * stats: double[dc_convT2x2_tiles()][4*Cout][2] (finalize with groups = 4). */
int dc_convT2x2_tiles(int N, int H, int W, int Cout);
int dc_convT2x2_fwd(const float* x, const float* wp, const float* bias, float* z, long z_ld, double* stats,
                    const float* scale, const float* shift, int relu,
                    int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
int dc_convT2x2_dgrad(const float* dz, const float* wp, float* dx,
                      int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
long dc_convT2x2_wgrad_ws_floats(int N, int H, int W, int Cin, int Cout);
int dc_convT2x2_wgrad(const float* x, const float* dz, float* dw, float* ws,
                      int N, int H, int W, int Cin, int Cout, dc_stream_t stream);

/* ---- BatchNormalization + Activation('relu') + Dropout  :158-159,:166-167,:179 ---
 * finalize: partial (sum,sumsq)[parts][groups*C][2] -> mean[C], invstd[C] = 1/sqrt(var_biased+eps);
 * if momentum >= 0: moving <- moving*momentum + batch*(1-momentum) (biased variance, Keras 2.0.6). */
int dc_bn_stats_finalize(const double* partial, int parts, int groups, int C, double count, float eps,
                         float momentum, float* mean, float* invstd, float* moving_mean, float* moving_var,
                         dc_stream_t stream);
/* inference fold: scale = gamma/sqrt(mvar+eps); shift = beta + (bias - mmean)*scale */
int dc_bn_fold(const float* gamma, const float* beta, const float* mmean, const float* mvar, const float* bias,
               float eps, float* scale, float* shift, int C, dc_stream_t stream);
/* a = dropout(relu(gamma*(z-mean)*invstd + beta)).  z dense [pixels][C]; out strided (out_ld).
 * Dropout: keep >= 1 -> none; mask != NULL -> explicit uint8 {0,1} [pixels][C]; else counter-based RNG(seed).
 * abound (nullable, float[C]): also writes the activation's per-channel magnitude bound
 * (|gamma|*sqrt(count) + |beta|)/keep for the consumers' fp16 range guard; count = elements per channel the
 * statistics were taken over (pixels; world*pixels under 'sync' data parallelism). */
int dc_bn_relu_drop_fwd(const float* z, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, const uint8_t* mask, float keep, uint64_t seed,
                        float* out, long out_ld, long pixels, int C, double count, float* abound, dc_stream_t stream);
/* dc_bn_relu_drop_fwd of a block that feeds MaxPooling2D((2,2)) (unet_2d_summary.py:166-170) AND that pooling, in one
 * pass over z [N,H,W,C]: writes the activation (out, strided: it is also the skip connection), pooled [N,H/2,W/2,C] and
 * idx (nullable uint8, argmax 0..3 in row-major window order, first max on ties).  Bit-identical to the two separate
 * calls; one tensor read less. */
int dc_bn_relu_drop_pool_fwd(const float* z, const float* mean, const float* invstd, const float* gamma,
                             const float* beta, const uint8_t* mask, float keep, uint64_t seed, float* out, long out_ld,
                             float* pooled, uint8_t* idx, int N, int H, int W, int C, double count, float* abound,
                             dc_stream_t stream);
/* backward, pass 1: partial[blocks][C][2] = (sum dy, sum dy*xhat) with dy = da*relu'(.)*dropmask/keep.
 * blocks = dc_bn_bwd_blocks(pixels, C).  amax_partial (nullable) [blocks][C] = max |dy| per block and channel
 * (what dc_bn_bwd_finalize_dzin bounds |dz| with; every pass-1 producer below takes the same argument). */
int dc_bn_bwd_blocks(long pixels, int C);
int dc_bn_bwd_reduce(const float* da, long da_ld, const float* z, const float* mean, const float* invstd,
                     const float* gamma, const float* beta, const uint8_t* mask, float keep, uint64_t seed,
                     float* partial, float* amax_partial, long pixels, int C, dc_stream_t stream);
/* backward, pass 2: dz = gamma*invstd*(dy - dbeta/M - xhat*dgamma/M); dbias_partial[blocks][C] = sum dz;
 * absmax_partial (nullable) [blocks] = max |dz| per block, for dc_pow2_scale_from_absmax. */
int dc_bn_bwd_apply(const float* da, long da_ld, const float* z, const float* mean, const float* invstd,
                    const float* gamma, const float* beta, const uint8_t* mask, float keep, uint64_t seed,
                    const float* dgamma, const float* dbeta, float* dz, float* dbias_partial, float* absmax_partial,
                    long pixels, int C, dc_stream_t stream);
/* scale[0] = 2^floor(log2(target / max_i partial[i])) (1 for an all-zero tensor): the exact power-of-two input scale
 * of the f16x3 gradient contractions. */
int dc_pow2_scale_from_absmax(const float* partial, int n, float target, float* scale, dc_stream_t stream);
/* what follows dc_bn_bwd_apply, in ONE launch: dbias[c] = sum over blocks of dbias_partial[b][c] (fixed order) and,
 * when absmax_partial / scale are given, scale[0] as dc_pow2_scale_from_absmax(absmax_partial, blocks, target). */
int dc_bn_bwd_apply_finalize(const float* dbias_partial, const float* absmax_partial, int blocks, int C, float target,
                             float* dbias, float* scale, dc_stream_t stream);

/* ---- inference: Conv2D -> (folded BN) -> ReLU whose output also feeds MaxPooling2D((2,2)) ----------------------------
 * dc_conv3x3_fwd_f16x3 (optimistic range flag out_flag, nullable) that also writes pool [N,H/2,W/2,Cout] = what
 * dc_maxpool2x2_fwd gives on z.  dc_conv3x3_fwd_pool_blocks() == 0: shape not served, use the two kernels. */
int dc_conv3x3_fwd_pool_blocks(int N, int H, int W, int Cin, int Cout);
int dc_conv3x3_fwd_pool_f16x3(const float* x, const void* wp16, const float* bias, float* z, long z_ld,
                              const float* scale, const float* shift, int relu, float* out_flag, float* pool,
                              int N, int H, int W, int Cin, int Cout, dc_stream_t stream);

/* ---- BatchNorm-backward sums fused into the kernel that PRODUCES da ("bnred") -------------------------------
 * The kernel that writes da of a BatchNorm layer also emits that layer's pass-1 partial sums
 * bn_partial[blocks][C][2] = (sum dy, sum dy*xhat), dy = da * [relu gate] * dropout, so dc_bn_bwd_reduce (and its
 * re-read of da and z) is skipped; dc_bn_bwd_finalize(bn_partial, blocks, ...) follows as usual.
 *   dc_head_bwd_bnin_bnred : blocks = dc_head_blocks(pixels); BN layer = the head's (non-materialised) input layer
 *   dc_maxpool2x2_bwd_bnred: blocks = dc_maxpool2x2_bwd_blocks(); BN layer = the pooled layer (z dense [N,H,W,C]) */
/*   dc_conv3x3_dgrad_bnred_f16x3: dc_conv3x3_dgrad_f16x3 whose output dx IS the `da` of the BatchNorm layer in front
 *   (dense [N,H,W,Cin], no dropout, pre-BN tensor z of the same shape): rows = dc_conv3x3_dgrad_bnred_blocks(...) partial
 *   rows of bn_partial[rows][Cin][2]; rows == 0 -> shape not served, use dc_conv3x3_dgrad_f16x3 + dc_bn_bwd_reduce. */
/* Kernel routing query (no launch): > 0 (the pixel-tile count) when a conv3x3 launch of this shape -- forward
 * (dgrad == 0; with_stats != 0: BatchNorm partials requested) or data gradient (dgrad != 0) -- runs the persistent
 * role-split kernel `igemm_pp_kernel` (64-column instantiation <2,2,*> when the GEMM column count, Cout forward / Cin
 * data gradient, exceeds 32; <4,1,*> otherwise); 0: one of the 256-thread kernels.  Depends on shape and DC_IGEMM_PP only. */
int dc_conv3x3_pp_blocks(int N, int H, int W, int Cin, int Cout, int dgrad, int with_stats);
int dc_conv3x3_dgrad_bnred_blocks(int N, int H, int W, int Cin, int Cout);
int dc_conv3x3_dgrad_bnred_f16x3(const float* dz, const void* wp16, float* dx, const float* dz_scale,
                                 const float* dz_absmax, int dz_absmax_n, const float* z,
                                 const float* mean, const float* invstd, const float* gamma, const float* beta,
                                 float* bn_partial, float* amax_partial, int N, int H, int W, int Cin, int Cout,
                                 dc_stream_t stream);
int dc_head_bwd_bnin_bnred(const float* z_in, const float* in_scale, const float* in_shift, const float* p,
                           const uint8_t* y, const float* kh, float* da, float* partial, int loss_kind,
                           const double* sums, const float* bn_mean, const float* bn_invstd, float* bn_partial,
                           float* amax_partial, long pixels, int C, dc_stream_t stream);
/*   dc_convT2x2_dgrad_bnred_f16x3: dc_convT2x2_dgrad_f16x3 whose output dx IS the `da` of the block in front of the up-convolution
 *   (dense [N,H,W,Cin], no Dropout): rows = dc_convT2x2_dgrad_bnred_blocks(); 0 -> not served (W <= 16), two-pass path. */
int dc_convT2x2_dgrad_bnred_blocks(int N, int H, int W, int Cin, int Cout);
int dc_convT2x2_dgrad_bnred_f16x3(const float* dz, const void* wp16, float* dx, const float* dz_scale,
                                  const float* dz_absmax, int dz_absmax_n, const float* z,
                                  const float* mean, const float* invstd, const float* gamma, const float* beta,
                                  float* bn_partial, float* amax_partial, int N, int H, int W, int Cin, int Cout,
                                  dc_stream_t stream);
int dc_maxpool2x2_bwd_blocks(int N, int H, int W, int C);
int dc_maxpool2x2_bwd_bnred(const float* dy, const uint8_t* idx, const float* skip, long skip_ld, float* dx,
                            const float* z, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, const uint8_t* mask, float keep, uint64_t seed, float* bn_partial,
                            float* amax_partial, int N, int H, int W, int C, dc_stream_t stream);

/* ---- BatchNorm backward WITHOUT the apply pass: "dz on load" (unet_2d_summary.py:163-167, Dropout-free blocks) ------
 * dz = gamma*invstd*(dy - dbeta/M - xhat*dgamma/M) is a per-channel affine of (dy, z): the data- and weight-gradient
 * kernels of the block form it while they stage their operands, so dz is never written and dc_bn_bwd_apply (read da,
 * read z, write dz) disappears:  dy = [fmaf(z, sc, sh) > 0] * da ;  dz = fmaf(A, dy, fmaf(D, z - mu, E)).
 *   dc_bn_bwd_finalize_dzin = dc_bn_bwd_finalize (partial != NULL; partial == NULL: dgamma / dbeta are INPUTS, the
 *     all-reduced sums of 'sync' BatchNorm, count = global elements per channel) + the table
 *     dz_coef[DC_DZ_COEF_ROWS][C] = { sc, sh, mu, A, D, E, bound } with bound_c >= max |dz_c| for ANY data
 *     (= |A| (max|dy_c| + |dbeta|/M + sqrt(M) |dgamma|/M); amax_partial[P][C] = per-row max |dy_c| from the pass-1
 *     producer): the consumers' fp16 range guard brings the largest bound into [2^14, 2^15).
 *   dc_conv3x3_dgrad_dzin_f16x3: dx = conv3x3_transpose(dz) from (da, z, dz_coef) (all dense [N,H,W,Cout]); role-split
 *     kernel only: dc_conv3x3_dgrad_dzin_blocks() == 0 -> shape not served, use dc_bn_bwd_apply + dc_conv3x3_dgrad_f16x3.
 *     red_z != NULL: dx IS the `da` of the BatchNorm layer in front (as dc_conv3x3_dgrad_bnred_f16x3): also emits
 *     bn_partial[rows][Cin][2] and amax_partial[rows][Cin], rows = the returned block count.
 *     dz_out != NULL (round 5): the dz the producers form is also WRITTEN, once per pixel (dense [N,H,W,Cout], fp32, unscaled),
 *     for a plain weight gradient (dc_conv3x3_wgrad_f16x3 / _bnin, dz_scale = dc_pow2_scale_from_absmax over row 6 of dz_coef):
 *     the BatchNorm-backward apply pass of the block disappears (1 tensor write instead of 2 reads + 1 write) and only the data
 *     gradient pays for forming dz -- the dz-on-load weight gradient is the slower of the two dz-on-load kernels.
 *   dc_conv3x3_wgrad_dzin_f16x3: dW = sum_p x[p+tap] (x) dz[p]; x as dc_conv3x3_wgrad_f16x3 (in_scale / in_shift NULL)
 *     or the producer's pre-BN tensor with BN + ReLU on load (as dc_conv3x3_wgrad_bnin_f16x3).  Cin == 1 (first layer):
 *     x is the (N,H,W) image.
 * The conv bias in front of a BatchNorm has the exact gradient sum_p dz = 0: dc_bn_bwd_finalize_dzin writes that 0 to
 * dbias[C] (nullable; the apply pass summed rounding noise there). */
#define DC_DZ_COEF_ROWS 7
int dc_bn_bwd_finalize_dzin(const float* partial, const float* amax_partial, int P, int C, const float* mean,
                            const float* invstd, const float* gamma, const float* beta, double count,
                            float* dgamma, float* dbeta, float* dz_coef, float* dbias, dc_stream_t stream);
int dc_conv3x3_dgrad_dzin_blocks(int N, int H, int W, int Cin, int Cout);
int dc_conv3x3_dgrad_dzin_f16x3(const float* da, const float* z, const float* dz_coef, const void* wp16, float* dx, float* dz_out,
                                const float* red_z, const float* red_mean, const float* red_invstd,
                                const float* red_gamma, const float* red_beta, float* bn_partial, float* amax_partial,
                                int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
int dc_conv3x3_wgrad_dzin_f16x3(const float* x, const float* in_scale, const float* in_shift, const float* x_abound,
                                const float* da, const float* z, const float* dz_coef, float* dw, float* ws,
                                int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
/* The first layer's (unet_2d_summary.py:170-172, Cin == 1) dz-on-load weight gradient WITHOUT the read of z: the thread that
 * holds the 3 x 6 image window of its four pixels rebuilds z = conv3x3(x, w) + bias from it, bit for bit what
 * dc_conv3x3_c1_fwd(x, w, bias, z, ..., scale = shift = NULL, relu = 0) wrote (one definition of that arithmetic, explicit
 * fused multiply-adds), and forms dz from (da, that z, dz_coef): dw equals dc_conv3x3_wgrad_dzin_f16x3(Cin = 1)'s exactly,
 * one full-resolution tensor pass less.  w: the layer's (3,3,1,Cout) kernel, bias nullable; ws as
 * dc_conv3x3_wgrad_ws_floats(Cin = 1).  Serves the 4-pixel kernel only: W % 4 != 0 or an unaligned x -> DC_EUNSUP. */
int dc_conv3x3_c1_wgrad_dzin_zre(const float* x, const float* w, const float* bias, const float* da, const float* dz_coef,
                                 float* dw, float* ws, int N, int H, int W, int Cout, dc_stream_t stream);

/* Joint backward of a conv block with 32 output channels at a 512^2-class resolution (the HBM-bound blocks of the network:
 * e0b / d0b, 32 -> 32, and d0a, 64 -> 32): ONE kernel stages dz (formed on load, as above) and the block input x once per
 * tile and produces dx, dW and -- 32 -> 32 only, red_z != NULL -- the pass-1 sums / max |dy| of the layer in front: every
 * tensor of the block is read once (4 tensor passes instead of 7; when red_z is x itself, the usual case, its values reach the
 * sums through LDS).  Arguments as dc_conv3x3_dgrad_dzin_f16x3 + dc_conv3x3_wgrad_dzin_f16x3 (wp16 = the data-gradient form
 * of the kernel); the 64 -> 32 variant takes a materialised x (in_scale NULL) and no red_z.
 * dc_conv3x3_bwd_joint_blocks() = rows of bn_partial / amax_partial (0: shape not served -- needs Cout == 32, Cin 32 or 64,
 * W >= 32: use the two separate kernels); ws: float[dc_conv3x3_bwd_joint_ws_floats()] (one dW slab per workgroup, reduced
 * in a fixed order => bit-reproducible). */
int dc_conv3x3_bwd_joint_blocks(int N, int H, int W, int Cin, int Cout);
long dc_conv3x3_bwd_joint_ws_floats(int N, int H, int W, int Cin, int Cout);
int dc_conv3x3_bwd_joint_f16x3(const float* x, const float* in_scale, const float* in_shift, const float* x_abound,
                               const float* da, const float* z, const float* dz_coef, const void* wp16, float* dx,
                               const float* red_z, const float* red_mean, const float* red_invstd, const float* red_gamma,
                               const float* red_beta, float* bn_partial, float* amax_partial, float* dw, float* ws,
                               int N, int H, int W, int Cin, int Cout, dc_stream_t stream);
/* The 32 -> 32 block right under the head (d0b, unet_2d_summary.py:219-222): its `da` is the head's dlogits.Kh^T, a rank-one
 * tensor da[pix][c] = kd[c] * s[pix], kd[c] = kh[c][1] - kh[c][0], s = dL/dlogit1.  The head's "s mode" entry points
 * (dc_head_fwd_bwd_s, dc_head_bwd_bnin_bnred_s) write s[pixels] instead of da[pixels][C]; this entry point takes (s, kh) in
 * place of da and its producers form kd[c] * s (one rounding, as the head's store) on load: every output equals
 * dc_conv3x3_bwd_joint_f16x3's on the materialised da bit for bit, and the tensor is neither written nor read.
 * Cin = Cout = 32 only (DC_EUNSUP otherwise); the remaining arguments as dc_conv3x3_bwd_joint_f16x3. */
int dc_conv3x3_bwd_joint_r1_f16x3(const float* x, const float* in_scale, const float* in_shift, const float* x_abound,
                                  const float* s, const float* kh, const float* z, const float* dz_coef, const void* wp16,
                                  float* dx, const float* red_z, const float* red_mean, const float* red_invstd,
                                  const float* red_gamma, const float* red_beta, float* bn_partial, float* amax_partial,
                                  float* dw, float* ws, int N, int H, int W, int Cin, int Cout, dc_stream_t stream);

/* ---- synchronised BatchNorm for batch-sharded data parallelism ('sync' mode) ---------------------
 * The per-channel sums leave the device between two launches so the host can all-reduce them over the ranks:
 *   forward : dc_bn_stats_reduce (conv partials -> double sums[C][2]) | all-reduce(sum) | dc_bn_stats_finalize_sums with
 *             count = GLOBAL elements per channel (scale/shift nullable: the training affine of the _bnin consumers);
 *   backward: dc_bn_bwd_finalize | all-reduce(sum) of (dgamma, dbeta) | dc_bn_bwd_apply_count with the same count.
 * With one rank (or count == pixels) the results equal the local entry points'. */
int dc_bn_stats_reduce(const double* partial, int parts, int groups, int C, double* sums, dc_stream_t stream);
/* partial rows folded parts -> chunks (fixed order, whole rows read coalesced): out = double[chunks][groups * C][2], same layout
 * as `partial`; dc_bn_stats_finalize* / dc_bn_stats_reduce then take (out, chunks, groups).  For launches with thousands of tile
 * rows (the 512^2-class layers), where the finalize's strided 16-byte reads cost more than this extra launch. */
int dc_bn_stats_rows_fold(const double* partial, int parts, int groups, int C, int chunks, double* out, dc_stream_t stream);
int dc_bn_stats_finalize_sums(const double* sums, int C, double count, float eps, float momentum, float* mean,
                              float* invstd, float* moving_mean, float* moving_var, const float* gamma,
                              const float* beta, float* scale, float* shift, float* abound, dc_stream_t stream);
int dc_bn_bwd_apply_count(const float* da, long da_ld, const float* z, const float* mean, const float* invstd,
                          const float* gamma, const float* beta, const uint8_t* mask, float keep, uint64_t seed,
                          const float* dgamma, const float* dbeta, float* dz, float* dbias_partial,
                          float* absmax_partial, long pixels, double count, int C, dc_stream_t stream);

/* ---- MaxPooling2D(2, strides=2)  :176 ----------------------------------------
 * in strided [N,H,W,C] (in_ld), out dense [N,H/2,W/2,C], idx (nullable) uint8 in {0..3}: FIRST max in
 * row-major window order (bit-exact contract). */
int dc_maxpool2x2_fwd(const float* in, long in_ld, float* out, uint8_t* idx,
                      int N, int H, int W, int C, dc_stream_t stream);
/* dx[N,H,W,C] dense = route(dy, idx) + (skip ? skip (strided, skip_ld) : 0) */
int dc_maxpool2x2_bwd(const float* dy, const uint8_t* idx, const float* skip, long skip_ld, float* dx,
                      int N, int H, int W, int C, dc_stream_t stream);

/* ---- UpSampling2D() + Dropout  :160-161,:198 (the upsampling_or_transpose != 'transpose' branch) -------------
 * nearest 2x of in [N,H,W,C] (dense) into out [N,2H,2W,C] (pixel stride out_ld), dropout applied to the
 * up-sampled tensor (mask uint8 [N,2H,2W,C] or counter RNG(seed); keep >= 1: none).
 * abound_in / abound_out (nullable pair, float[C]): range-guard bound of the source / of the up-sampled tensor
 * (= abound_in / keep); abound_in_ld > 0: all DC_ABOUND_SLOTS replicas (inference), *_ld floats apart. */
int dc_upsample2x_drop_fwd(const float* in, float* out, long out_ld, const uint8_t* mask, float keep, uint64_t seed,
                           const float* abound_in, long abound_in_ld, float* abound_out, long abound_out_ld,
                           int N, int H, int W, int C, dc_stream_t stream);
/* din[N,H,W,C] (dense) = sum over each 2x2 block of dout (pixel stride dout_ld) * dropout factor */
int dc_upsample2x_drop_bwd(const float* dout, long dout_ld, const uint8_t* mask, float keep, uint64_t seed, float* din,
                           int N, int H, int W, int C, dc_stream_t stream);

/* ---- Conv2D(2,1,softmax) + Lambda(x[...,-1]) + loss + metrics  :221-222,:372-380,:398-399 ------------------
 * p = softmax(a.Kh + bh)[...,1].  y != NULL: also partial[blocks][DC_HEAD_SUMS = 12] =
 *   {bce_sum, sum round(p)*y, sum round(p), sum clip(y-round(p),0,1), sum y, sum y*p, sum p*p, sum y*y,
 *    sum p, weighted_bce_sum, 0, 0}
 * (Keras clip/logit BCE form; round half to even; weighted BCE of utils/neurons.py:13-29).
 * blocks = dc_head_blocks(pixels); reduce with dc_reduce_partials_f64(partial, blocks, 12, sums). */
int dc_head_blocks(long pixels);
int dc_head_fwd(const float* a, const float* kh, const float* bh, const uint8_t* y, float* p, float* partial,
                long pixels, int C, dc_stream_t stream);
/* da = dlogits.Kh^T; partial[blocks][C+4] = (sum a[c]*s ..., sum s, pad) with s = dL/dlogit1 = -dL/dlogit0.
 * loss_kind: 0 binary_crossentropy (mean), 1 weighted_binary_crossentropy (mean), 2 dice_loss, 3 dicesq_loss
 * (unet_2d_summary.py:372-377); kinds 2,3 read the forward's reduced sums (device double[12]). */
int dc_head_bwd(const float* a, const float* p, const uint8_t* y, const float* kh, float* da, float* partial,
                int loss_kind, const double* sums, long pixels, int C, dc_stream_t stream);
/* head gradient from partial: dkh[c][0] = -S_c, dkh[c][1] = S_c, dbh = (-S, S) */
/* Training with a per-pixel loss (loss_kind 0 binary_crossentropy / 1 weighted_binary_crossentropy): dc_head_fwd and
 * dc_head_bwd(_bnin)(_bnred) in ONE pass over the head's input -- p, the 12 metric partials, da, the head's
 * weight-gradient partials (grad_partial: [blocks][C+4], for dc_head_grad_finalize) and, when bn_partial is given, the
 * producing BatchNorm layer's backward sums ([blocks][C][2]; needs in_scale / in_shift / bn_mean / bn_invstd).
 * in_scale / in_shift NULL: `a` is a materialised activation.  The dice losses need the global sums before their
 * backward: DC_EUNSUP. */
int dc_head_fwd_bwd(const float* a, const float* in_scale, const float* in_shift, const float* kh, const float* bh,
                    const uint8_t* y, float* p, float* partial, float* da, float* grad_partial, int loss_kind,
                    const float* bn_mean, const float* bn_invstd, float* bn_partial, float* amax_partial, long pixels,
                    int C, dc_stream_t stream);
/* "s mode" of the two head backward kernels that feed a dz-on-load block (:221-222): da = dlogits.Kh^T has rank one, so only
 * its per-pixel factor s[pixels] = dL/dlogit1 is written (da[pix][c] = (kh[c][1] - kh[c][0]) * s[pix], formed on load by
 * dc_conv3x3_bwd_joint_r1_f16x3); p, the metric partials, the weight-gradient partials, bn_partial and amax_partial are those
 * of dc_head_fwd_bwd / dc_head_bwd_bnin_bnred bit for bit.  No da argument: nothing of that size is touched. */
int dc_head_fwd_bwd_s(const float* a, const float* in_scale, const float* in_shift, const float* kh, const float* bh,
                      const uint8_t* y, float* p, float* partial, float* s, float* grad_partial, int loss_kind,
                      const float* bn_mean, const float* bn_invstd, float* bn_partial, float* amax_partial, long pixels,
                      int C, dc_stream_t stream);
int dc_head_bwd_bnin_bnred_s(const float* z_in, const float* in_scale, const float* in_shift, const float* p,
                             const uint8_t* y, const float* kh, float* s, float* partial, int loss_kind,
                             const double* sums, const float* bn_mean, const float* bn_invstd, float* bn_partial,
                             float* amax_partial, long pixels, int C, dc_stream_t stream);
int dc_head_grad_finalize(const float* partial, int blocks, int C, float* dkh, float* dbh, dc_stream_t stream);

/* ---- generic deterministic reductions ------------------------------------------
 * out[l] = scale * sum_p in[p*L + l]  (double accumulation, fixed order). tmp: float[32*L] scratch. */
int dc_reduce_partials(const float* in, int P, long L, float scale, float* out, float* tmp, dc_stream_t stream);
int dc_reduce_partials_f64(const float* in, int P, int L, double* out, dc_stream_t stream);
/* out[c] = sum_p in[(p*C + c)*2 + j] -> dbeta (j=0), dgamma (j=1) */
int dc_bn_bwd_finalize(const float* partial, int P, int C, float* dgamma, float* dbeta, dc_stream_t stream);

/* ---- Adam(0.002), Keras 2.0.6 form  :335 ------------------------------------------
 * g' = g*gscale; m = b1*m+(1-b1)*g'; v = b2*v+(1-b2)*g'^2; p -= lr_t*m/(sqrt(v)+eps), flat over n floats. */
int dc_adam_step_flat(float* p, const float* g, float* m, float* v, long n, float lr_t, float b1, float b2,
                      float eps, float gscale, dc_stream_t stream);

/* ---- 8x test-time augmentation of predict()  unet_2d_summary.py:585-595, utils/neurons.py:112-137 ---------------
 * The augmentations are pixel permutations; maps / invmaps (int32 [K][H*W]) are made on the host by applying the table's
 * own functions to an index image.  dc_gather_maps: out[k][p] = in[maps[k][p]] (n = H*W elements per copy).
 * dc_tta_merge: m = sum_k preds[k][invmaps[k][p]] / K in double, table order (numpy's float64 accumulation), cropped to
 * hs x ws; mask (uint8 [hs][ws]) = m > threshold; mean_out (nullable float [hs][ws]) = m. */
int dc_gather_maps(const float* in, const int* maps, float* out, int K, long n, dc_stream_t stream);
int dc_tta_merge(const float* preds, const int* invmaps, int K, int H, int W, int hs, int ws, double threshold,
                 uint8_t* mask, float* mean_out, dc_stream_t stream);

/* ---- training-batch assembly on the device: UNet2DSummary._batch_gen  unet_2d_summary.py:434-530 -----------------
 * S (float32) / M (uint8): the normalised summary images / flattened masks of ALL datasets, concatenated into one device
 * buffer each (src_elems elements; same layout for both), uploaded once per fit().  The host draws the reference's random
 * stream (:479-527) and describes item b by four longs
 *   items_host[b] = { element offset of the crop origin (y0, x0) in S / M, row stride of that image, eh << 32 | ew, d4 }:
 * the eh x ew crop is zero-filled to the (hw, hw) window (:505-521) and permuted by the composition of the drawn flips /
 * rot90s (:524-527), one of 8 dihedral maps:  out[i][j] = win[r][c], (r, c) = (d4 & 1) ? (j, i) : (i, j),
 * r = (d4 & 2) ? hw-1-r : r, c = (d4 & 4) ? hw-1-c : c.  x: float32 [B][hw][hw], y: uint8 [B][hw][hw].
 * items_host is the ONE HOST pointer of this ABI: the items are validated against src_elems and travel in the kernel
 * argument block (chunks of DC_CROP_MAX_ITEMS) -- nothing is staged, copied asynchronously or retained. */
#define DC_CROP_MAX_ITEMS 64
int dc_crop_augment(const float* S, const uint8_t* M, long src_elems, const long* items_host, int B, int hw,
                    float* x, uint8_t* y, dc_stream_t stream);
/* out[n][r][c] = p[n][y0 + r][x0 + c] > 0.5 (uint8): numpy's `mp[y0:y1, x0:x1].round()` of _ValidationMetricsCB
 * (unet_2d_summary.py:90-91; half-to-even: 0.5 -> 0) on N probability maps of H x W. */
int dc_round_window_u8(const float* p, int N, int H, int W, int y0, int y1, int x0, int x1, uint8_t* out,
                       dc_stream_t stream);

/* ---- host-side Neurofinder scoring of the validation callback  unet_2d_summary.py:90-91 -> datasets/nf.py:153-174 -----
 * HOST pointers, no device work, no stream: the per-mask scoring _ValidationMetricsCB runs 6 x n times per epoch, as one native
 * call (the GIL is released around it, so scoring threads run beside the validation forwards).  truth / pred: uint8 [H][W]
 * (non-zero = foreground).  8-connected components numbered in raster order of their first pixel (skimage.measure.label's
 * default on 2-D input); neurofinder.centers with `threshold` (5 in the reference's nf_mask_metrics) and neurofinder.shapes
 * (threshold inf) restated as in deep_calcium_amd/nf_metrics.py, bit-identical to it (tests/test_nf_matching.py).
 * counts[4] = { regions in truth, regions in pred, centre hits, matched pairs np }; inc[k] / exc[k] (k < np <= cap) =
 * |A & B| / |A| and |A & B| / |B| of the k-th matched pair in the order of the truth's regions (the caller takes the means:
 * recall = hits / counts[0], precision = hits / counts[1]).
 * ws: dc_host_nf_ws_bytes(H, W) bytes of HOST scratch owned by the caller (one per scoring thread; nothing is allocated). */
long dc_host_nf_ws_bytes(int H, int W);
int dc_host_nf_pairs(const uint8_t* truth, const uint8_t* pred, int H, int W, double threshold, int* counts,
                     double* inc, double* exc, int cap, void* ws);
int dc_host_label8(const uint8_t* mask, int H, int W, int* labels, int* n, void* ws);

/* ---- series summaries: a recording (T,H,W) of 16-bit frames -> the (H,W) images the network segments ------------------------
 * What the reference computes on the host while it builds a dataset (datasets/nf.py:121-130: series/mean accumulated IN its
 * float16 storage, series/max in int16) and standardises in its default series_summary_func (_summarize_series,
 * unet_2d_summary.py:227-241), plus the summaries it leaves to the user's own series_summary_func: the true mean, the max
 * projection, the temporal standard deviation and the local correlation image.
 * frames: int16 (is_unsigned == 0) or uint16 (is_unsigned != 0), [tc][H][W] contiguous, 2-byte aligned -- W and H*W need no
 * padding.  A recording arrives in chunks: t0 = index of the chunk's first frame, n_total = frames of the whole recording.
 * All running state lives in the CALLER's buffers (H*W elements each); the chunk with t0 == 0 initialises it (previous
 * contents are ignored), every later chunk continues it.  Chunk boundaries never change a bit of any result.
 * DC_SERIES_MAX_FRAMES: the int64 sums hold T * 65535^2 < 2^63 for every T up to it; beyond: DC_EUNSUP (-3). */
#define DC_SERIES_MAX_FRAMES 2147483647L
/* datasets/nf.py:121-130, per pixel over the chunk's frames in order:
 *   mean16 (bits of a float16): m = float16(double(m) + double(x) / n_total) -- IEEE double divide and add, ONE rounding
 *     to nearest even per frame (never through float32), inf above 65504: bit-identical to `ds_mean[...] += img * 1. / n`;
 *   max16 (int16): min(max(m, x), 32767) starting from 0 (`np.maximum(ds_max, img)` through the saturating int16 store);
 *   sum, sumsq (int64), vmax (int32): exact sum x, sum x*x and the true maximum.
 * mean16 / max16: both given or both NULL (the float16 chain is the expensive part of the pass). */
int dc_series_accumulate(const void* frames, int is_unsigned, int tc, long t0, long n_total, uint16_t* mean16,
                         int16_t* max16, long* sum, long* sumsq, int* vmax, int H, int W, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
/* the exact cross sums of the local correlation image (no counterpart in datasets/nf.py:121-130 or
 * unet_2d_summary.py:227-241: a series_summary_func of the user's): xy = int64[4][H*W], xy[j][p] = sum_t x_p * x_q with q the
 * right (j = 0), down (1), down-right (2), down-left (3) neighbour of p; a neighbour outside the image contributes 0. */
int dc_series_accumulate_xy(const void* frames, int is_unsigned, int tc, long t0, long* xy, int H, int W,
                            dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
/* state -> float32 images (each output nullable; the user-side summaries next to datasets/nf.py:121-130 /
 * unet_2d_summary.py:227-241): mean = sum / T; std = sqrt(T sum x^2 - (sum x)^2) / T (population); corr (needs xy) = the
 * mean over the pixel's EXISTING 8 neighbours of the Pearson correlation, a pair with a zero-variance pixel counting 0,
 * a pixel without neighbours giving 0.  The numerators T sum xy - sum x sum y and T sum x^2 - (sum x)^2 are formed
 * exactly in 128-bit integers, converted to double with one rounding; then one divide (and one sqrt) in double and one
 * rounding to float32 per value -- mean and std within 1 float32 ulp of the exact value; corr sums up to 8 such quotients
 * in double (absolute error below 1e-14, i.e. within 1 float32 ulp unless the neighbours' correlations cancel to |corr| < 1e-6). */
int dc_series_finalize(const long* sum, const long* sumsq, const long* xy, float* mean, float* sdev, float* corr,
                       int H, int W, long T, dc_stream_t stream);
/* out = (in - mean(in)) / std(in) over one H x W float32 image: `(summ - np.mean(summ)) / np.std(summ)` of
 * _summarize_series, unet_2d_summary.py:227-241 (its input: the series/mean of datasets/nf.py:121-130).  Sums in double, fixed
 * order (two-pass variance); subtraction and division in double, one rounding to float32.
 * ws: float[dc_series_standardize_ws_floats()], 8-byte aligned.  in == out is allowed. */
long dc_series_standardize_ws_floats(int H, int W);
int dc_image_standardize(const float* in, float* out, float* ws, int H, int W, dc_stream_t stream);
/* temporal binning: the means of b consecutive frames, streamed (no counterpart in datasets/nf.py:121-130 or
 * unet_2d_summary.py:227-241; what is averaged before anything is correlated).  frames: [tc][H][W], int16 or uint16 by
 * is_unsigned, 2-byte aligned.  carry: int32[H*W], 4-byte aligned, the sum of the `phase` frames of the open bin that earlier calls
 * have seen, 0 <= phase < b.  The call consumes tc more frames, writes n_out = (phase + tc) / b frames of the same 16-bit type to
 * `out` and leaves in `carry` the sum of the (phase + tc) % b frames of the bin that is still open:
 *   out[j] = floor((2 s + b) / (2 b)), s the exact sum of the bin's b frames
 * -- the mean rounded half up, the floor holding for negative sums (the rule of dc_motion_bin); it lies between the bin's
 * smallest and largest value, and |s| <= 64 * 65535 < 2^22 fits int32.  carry is READ only when phase > 0 (never pre-cleared)
 * and WRITTEN only when (phase + tc) % b > 0; a call with phase + tc < b writes no frame and only extends carry.  b = 1 is a copy;
 * tc == 0 launches nothing.  Chunk boundaries never change a bit.
 * DC_EINVAL (-1): b < 1, phase outside [0, b), a negative or zero size, a null pointer that would be followed, a misaligned
 * buffer, out overlapping frames or carry (or carry overlapping frames).  DC_EUNSUP (-3): b > DC_SERIES_MAX_BIN_FRAMES, H * W > 2^30. */
#define DC_SERIES_MAX_BIN_FRAMES 64
int dc_series_bin_time(const void* frames, int is_unsigned, int tc, int H, int W, int b, int phase, int* carry, void* out,
                       dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */

/* ---- ROI traces: a recording (T,H,W) of 16-bit frames + a set of ROIs -> one fluorescence trace per ROI -------------------
 * What the reference's spikes model reads from its dataset files: `traces`, a (no. ROIs, no. frames) matrix
 * (unet_1d_segmentation.py:182-187), normalised per trace as (traces - mean) / std along time (unet_1d_segmentation.py:158-167).
 * The reference has no code that makes the matrix from a recording and a mask; this is that step.
 * frames: as for dc_series_accumulate (int16 / uint16 by is_unsigned, [tc][H][W] contiguous, 2-byte aligned), a chunk of the
 * recording starting at frame t0.
 * ROIs are CSR rows, all DEVICE memory, never read on the host: row_off int32[S + 1] (non-decreasing, row_off[0] = 0), row_pix
 * int32[row_off[S]] flat pixel indices y * W + x, row_roi int32[S] (nullable) the ROI (output row) CSR row s adds into; NULL
 * means CSR row s IS ROI s, and then S == R.  ROIs may overlap, an index listed twice counts twice, a row may be empty, an
 * index outside [0, H*W) contributes 0 and is never dereferenced, a row whose row_roi is outside [0, R) adds nowhere.  A
 * caller cuts long ROIs into rows of bounded length (row_roi names the owner), so that one whole-image ROI among hundreds of
 * small ones does not make the launch as long as one workgroup walking it.
 *   dc_roi_trace_accumulate: sums = int64[R][ld].  Columns [t0, t0 + tc) of ALL R rows are fully written (never pre-clear),
 *     no other column is touched: sums[r][t0 + t] = the exact integer sum of ROI r's pixels in frame t of the chunk --
 *     independent of the chunking of the recording and of how ROIs are cut into rows.
 *   dc_roi_trace_finalize: areas int32[R] = pixels per ROI; each output float[R][T] dense, nullable.
 *     mean[r][t] = double(sums) / double(area), ONE rounding to float32 (numpy's (sums / area).astype(float32), bit for bit).
 *     zscore[r][t] = (trace - mean_t) / std_t with the population standard deviation; the area cancels:
 *     (T S_t - sum S) / sqrt(T sum S^2 - (sum S)^2), both numerators exact in 128-bit integers, each rounded ONCE to double,
 *     then sqrt and divide in double and one rounding to float32: within 1 float32 ulp.  A trace that is constant in time
 *     (T == 1 included) gives exactly 0 where numpy gives NaN (0 / 0) and the reference's asserts (:165-166) fail; an ROI of
 *     area <= 0 gives 0 in both outputs.
 * DC_ROI_TRACE_MAX_VOLUME: T * H * W <= 2^46 keeps (T * 65535 * H * W)^2 < 2^124, so every intermediate of the z-score fits
 * (for ROIs that list at most H * W pixels); beyond: DC_EUNSUP (-3).  dc_roi_trace_accumulate checks (t0 + tc) * H * W,
 * dc_roi_trace_finalize, which is not told the image size, T alone. */
#define DC_ROI_TRACE_MAX_VOLUME 70368744177664L
int dc_roi_trace_accumulate(const void* frames, int is_unsigned, int tc, long t0, const int* row_off, const int* row_pix,
                            const int* row_roi, int S, int R, long* sums, long ld, int H, int W, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_roi_trace_finalize(const long* sums, long ld, const int* areas, int R, long T, float* mean, float* zscore,
                          dc_stream_t stream);

/* ---- Weighted ROI traces: every entry of an ROI carries a 16-bit weight --------------------------------------------------------
 * dc_roi_wtrace_accumulate is dc_roi_trace_accumulate, word for word, with one more array: row_wgt uint16[row_off[S]], DEVICE
 * memory, 2-byte aligned, row_wgt[e] the weight of entry e of row_pix.  sums[r][t0 + t] = the exact int64 sum of w_e * x_e over
 * ROI r's entries in frame t.  ANY uint16 weight is legal: |w x| <= 65535^2 < 2^32, and at most 2^30 entries per ROI keep
 * |S| < 2^62 (csrc/wtrace_math.h derives what 32 bits can hold of this: nothing, so the kernel sums in int64 from the first term).
 * Everything else is inherited: an index outside [0, H*W) contributes 0 and is never dereferenced; an index listed twice counts
 * once per listing, each with its own weight; an empty row, a row_roi outside [0, R) and row_roi == NULL with S == R behave as
 * above; columns [t0, t0 + tc) of ALL R rows are fully written and nothing else is touched; the same bits for every chunking,
 * every cut of ROIs into rows, every launch geometry and every run.  Error codes as above; a null or odd-address row_wgt:
 * DC_EINVAL.
 * The weight sum W_r = sum of w over ROI r stands where the area stood in dc_roi_trace_finalize, dc_trace_baseline* and
 * dc_trace_pair_*: mean = S / W is the weighted mean, the z-score is area-free, and |S| <= 65535 W holds term by term.  THE CALLER
 * PROMISES 1 <= W_r <= 2^31 - 1 and T * W_r <= 2^46 (the volume limit above, with W for H * W). */
int dc_roi_wtrace_accumulate(const void* frames, int is_unsigned, int tc, long t0, const int* row_off, const int* row_pix,
                             const unsigned short* row_wgt, const int* row_roi, int S, int R, long* sums, long ld, int H, int W,
                             dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */

/* ---- ROI footprint maps: the correlation of every pixel of an ROI's support with the ROI's own trace ---------------------------
 * The one decision of the chain that never looks at the recording is which pixels belong to a neuron (the ROIs are the regions
 * of a mask predicted from ONE summary image).  This is the check of an ROI against the movie it came from, the quantity
 * CaImAn's spatial r_values and suite2p's footprint weights are built on.  The reference has no counterpart; THESE DEFINITIONS
 * ARE THE SPECIFICATION.  Integers until the last step, independent of how the recording was chunked.
 * x_p(t): pixel p in frame t.  ROI r: pixels P_r, area A_r, trace S_r(t) = sum over P_r of x_p(t) (what
 * dc_roi_trace_accumulate writes).  The SUPPORT of ROI r is chosen by the caller (P_r plus a halo, sorted by flat index); each
 * of its ENTRIES (r, p) is `inside` (p in P_r) or not.  A pixel in the supports of two ROIs is two independent entries.
 *   per entry, over all T frames:   a = sum x,  b = sum x^2,  c = sum x S_r      (c: 128 bits, c_hi * 2^64 + c_lo)
 *   per ROI:                        u = sum S_r,  w = sum S_r^2                   (w: 128 bits)
 *   Cxx = T b - a^2,  Cxs = T c - a u,  Css = T w - u^2, exact in 128-bit integers;
 *   halo entry:    Cxl = Cxs,        Cll = Css;
 *   inside entry:  Cxl = Cxs - Cxx,  Cll = Css - 2 Cxs + Cxx: the pixel is taken out of the trace it is compared with
 *                  (L = S - x), otherwise every pixel of a small ROI correlates with itself;
 *   corr = (float)(f64(Cxl) / (sqrt(f64(Cxx)) * sqrt(f64(Cll)))), each numerator rounded ONCE to double, no fused multiply-add;
 *   exactly 0 where Cxx <= 0 or Cll <= 0 (a pixel or trace constant in time, T == 1, the pixel of a one-pixel ROI; numpy: NaN).
 * Limits: T * H * W <= DC_ROI_TRACE_MAX_VOLUME as above, and T <= DC_ROI_PIXEL_MAX_FRAMES = 2^31 - 1 so that b < 2^63; under
 * both every intermediate stays below 2^127 (csrc/footprint_math.h derives it).  Beyond: DC_EUNSUP (-3).
 * All pointers are DEVICE memory, there are no out-parameters and nothing is read on the host.
 *   dc_roi_pixel_accumulate: row_off / row_pix / row_roi: a CSR over the support ENTRIES, in the form of
 *     dc_roi_trace_accumulate (row_roi nullable, then S == R); entry e = position in row_pix, N = row_off[S] entries (an
 *     entry at or beyond N is never touched).  sums = int64[R][ld] whose columns [t0, t0 + tc) dc_roi_trace_accumulate has
 *     filled on the same stream.  mom = int64[4 * N], CALLER-OWNED AND CALLER-ZEROED before the first chunk: planes a, b, c_lo,
 *     c_hi of N entries each; the call ADDS the chunk's contribution.  Every entry is owned by one thread of one workgroup:
 *     no atomics, the same bits for every chunking and every run.  Exact for any 16-bit x and ANY int64 sums (|S| <= 2^46 is
 *     what the limits allow).  An index outside [0, H*W) contributes nothing and is never dereferenced; a row whose row_roi is
 *     outside [0, R) adds nothing.
 *   dc_roi_trace_moments: rmom = int64[3 * R]: u, w_lo, w_hi of every row of sums = int64[R][ld] over its first T columns.
 *   dc_roi_pixel_corr: inside int32[N] (non-zero: inside); corr float[N], one value per entry in entry order; the entries of a
 *     row whose row_roi is outside [0, R) get 0.
 * N == 0, S == 0, R == 0 (and tc == 0 for the accumulation): 0, nothing launched. */
#define DC_ROI_PIXEL_MAX_FRAMES 2147483647L
int dc_roi_pixel_accumulate(const void* frames, int is_unsigned, int tc, long t0, const int* row_off, const int* row_pix,
                            const int* row_roi, int S, int R, const long* sums, long ld, long* mom, int N, int H, int W,
                            dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_roi_trace_moments(const long* sums, long ld, int R, long T, long* rmom, dc_stream_t stream);
int dc_roi_pixel_corr(const long* mom, int N, const int* row_off, const int* row_roi, int S, int R, const int* inside,
                      const long* rmom, long T, float* corr, dc_stream_t stream);

/* ---- ROI pixel-pair correlation: the correlation of every pixel of an ROI with every other pixel of it ---------------------------
 * An ROI is an 8-connected region of a mask predicted from ONE summary image, so two cells that touch are one ROI with one
 * trace.  The footprint map above cannot separate them (both halves correlate with the summed trace); the correlation of the
 * pixels with EACH OTHER can.  That is a k x k Gram matrix per ROI, accumulated over the recording beside the traces.  The
 * reference has no counterpart; THESE DEFINITIONS ARE THE SPECIFICATION.  Integers until the last step, independent of how the
 * recording was chunked.
 * ROI r: k_r own pixels in flat-index order (no halo), x_i(t) the i-th of them in frame t.  Over all T frames:
 *   a_i  = sum_t x_i(t)                       int64, exact, |a_i| < 2^47
 *   g_ij = sum_t x_i(t) x_j(t), i <= j        int64, exact, |g_ij| <= 65535^2 T < 2^63
 *   Cij  = T g_ij - a_i a_j                   exact in 128-bit integers (|T g| < 2^94, |a a| < 2^94)
 *   corr_ij = dc_fp_corr of csrc/footprint_math.h on {Cii, Cij, Cjj}: (float)(f64(Cij) / (sqrt(f64(Cii)) * sqrt(f64(Cjj)))), each
 *             numerator rounded ONCE to double, no fused multiply-add: within 1 float32 ulp, bit-symmetric, in [-1, 1], the
 *             diagonal exactly 1 for a pixel that varies; row, column AND diagonal exactly 0 for a pixel that is constant in time
 *             (T == 1 included; numpy: NaN).
 * Limits: T <= DC_ROI_PIXEL_MAX_FRAMES and T * H * W <= DC_ROI_TRACE_MAX_VOLUME as above; k_r <= DC_ROI_PAIR_MAX_AREA;
 * G = sum k_r^2 <= DC_ROI_PAIR_MAX_STATE (1 GiB of int64).  Beyond: DC_EUNSUP (-3).
 * All pointers are DEVICE memory, there are no out-parameters and nothing is read on the host.
 *   state: a = int64[P], P = sum k_r, in the order of roi_pix; g = int64[G]: ROI r owns a full k_r x k_r row-major square at
 *     goff[r].  CALLER-OWNED AND CALLER-ZEROED before the first chunk; dc_roi_pair_accumulate ADDS the chunk's contribution to a
 *     and to the entries i <= j of g.  The lower triangle is never read or written by it.
 *   dc_roi_pair_accumulate: frames as for dc_roi_trace_accumulate, a chunk of tc frames.  roi_off int32[R + 1], roi_pix
 *     int32[P] flat indices y * W + x, goff int64[R].  tiles int32[ntiles][3] = (r, ti, tj), ti <= tj: one workgroup per tile of
 *     DC_ROI_PAIR_TILE x DC_ROI_PAIR_TILE pairs (rows ti * TILE.., columns tj * TILE.. of ROI r's square); the caller lists
 *     every tile with ti <= tj < ceil(k_r / TILE) of every ROI ONCE.  The tile ti == tj also owns a for its pixels.  Every state
 *     word is read, added to and written once per call by one thread of one workgroup: no atomics, the same bits for every
 *     chunking and every run.  The frames are staged DC_ROI_PAIR_BATCH at a time.  A tile that names an ROI outside [0, R), with
 *     tj < ti or outside the ROI, an ROI with k_r > DC_ROI_PAIR_MAX_AREA or whose square leaves [0, G) or whose pixels leave
 *     [0, P) is skipped whole; a pixel index outside [0, H*W) is never dereferenced and counts as 0.  What the host can see of
 *     the limits is refused: G > DC_ROI_PAIR_MAX_STATE, G > DC_ROI_PAIR_MAX_AREA * P, ntiles >= 2^31, or more tiles than R
 *     ROIs of the largest area have.
 *   dc_roi_pair_corr: corr float[G] in the layout of g: every (i, j) of every ROI's square is written, the lower triangle
 *     included (it reads g at [min(i,j)][max(i,j)]).  An ROI that dc_roi_pair_accumulate would skip is skipped.
 * R == 0, P == 0, G == 0, ntiles == 0 (and tc == 0 for the accumulation): 0, nothing launched. */
#define DC_ROI_PAIR_TILE 64
#define DC_ROI_PAIR_BATCH 32
#define DC_ROI_PAIR_MAX_AREA 1024
#define DC_ROI_PAIR_MAX_STATE 134217728L
int dc_roi_pair_accumulate(const void* frames, int is_unsigned, int tc, const int* roi_off, const int* roi_pix, const long* goff,
                           const int* tiles, long ntiles, int R, long* a, long* g, int P, long G, int H, int W, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_roi_pair_corr(const long* a, const long* g, const int* roi_off, const long* goff, int R, int P, long G, long T, float* corr,
                     dc_stream_t stream);

/* ---- Detrended correlations: centred moments pooled over segments of the recording ----------------------------------------------
 * A recording bleaches and drifts.  A decay common to all pixels is a signal every pixel shares: it pushes every whole-recording
 * correlation above (the series `corr` image, the footprint maps, the pixel-pair matrices) towards 1.  Correlating WITHIN segments
 * of L frames and pooling removes every trend that is constant inside a segment -- piecewise-constant detrending; a trend inside a
 * segment stays.  The reference has no counterpart; THESE DEFINITIONS ARE THE SPECIFICATION.  Integers until the last step, no
 * look-ahead, independent of how the recording was chunked.
 * The T frames are cut into n = max(1, T / L) segments: n - 1 of L frames and a last one of L_last = T - (n - 1) L frames
 * (L <= L_last < 2 L); T < 2 L: one segment of T frames.  M = L * L_last (M = T when n == 1), mult_s = M / L_s: L_last for a full
 * segment, L for the last, 1 when n == 1 -- so len * mult == M for every segment.  For any two series x, y a reader correlates,
 * with the exact sums a_s = sum x, a'_s = sum y, g_s = sum x y over segment s:
 *   N(x, y) = sum_s mult_s (L_s g_s - a_s a'_s)       exact in 128-bit integers: M times the pooled within-segment cross sum
 *   corr    = today's arithmetic on {N(x,x), N(x,y), N(y,y)}: dc_fp_corr for pairs and footprints (the footprint rule for an
 *             inside entry is linear, Cxl = Cxs - Cxx, Cll = Css - 2 Cxs + Cxx, and is applied to the pooled numerators),
 *             dc_series_finalize's neighbour mean for the series image.  With n == 1 the numerators are T g - a a': the same bits
 *             as the undetrended entry points give.
 *   std     = (float)sqrt(f64(N(x,x)) / f64(M * T)): population, within 1 float32 ulp of the exact value.
 * Limits: 2 <= L <= DC_DETREND_MAX_FRAMES; a segment beside others has len, mult <= 2 L - 1 <= 8191, one alone mult == 1 and
 * len <= 2^31 - 1; all limits of the undetrended entry points; and M * H * W <= 2^46, which keeps the largest numerator, the
 * footprint Css, below 2^124 (csrc/detrend_math.h derives the magnitudes).  Beyond: DC_EUNSUP (-3); len < 1 or mult < 1:
 * DC_EINVAL.  All pointers are DEVICE memory, there are no out-parameters and nothing is read on the host.
 * A POOLED WORD is one 16-byte {lo, hi} element (two's complement, value = hi * 2^64 + lo) of a 16-byte aligned int64 buffer;
 * the pooled state is CALLER-OWNED AND CALLER-ZEROED.  Every state word is owned by one thread of one workgroup: no atomics, the
 * same bits for every chunking and every run.  The caller accumulates a segment with the undetrended accumulate entry points
 * and calls the fold at the segment's last frame.
 *   dc_series_fold_segment: sum, sumsq, xy (nullable, then pooled_cov is null too), vmax: the state of dc_series_accumulate /
 *     dc_series_accumulate_xy over the len frames of the segment.  pooled_var: H * W words, += mult (len sumsq - sum^2);
 *     pooled_cov: 4 * H * W words in the layout of xy, += mult (len xy[j] - sum_p sum_q(j)), a neighbour outside the image adds
 *     nothing.  sum_total int64[H * W] += sum (zeroed by the caller), vmax_total int32[H * W] = max(vmax_total, vmax) (set to
 *     INT32_MIN by the caller): the whole recording's sum and maximum.  The segment state is NOT cleared: the next segment's first
 *     accumulate passes t0 == 0, which initialises it.
 *   dc_series_finalize_pooled: mean (nullable; needs sum_total) = (float)(double(sum_total) / double(T)), sdev (nullable), corr
 *     (nullable; needs pooled_cov): the neighbour rule and summation order of dc_series_finalize; a pair with a non-positive
 *     N(x,x) counts 0.
 *   dc_roi_pair_fold_segment: a, g, roi_off, goff, tiles as for dc_roi_pair_accumulate, one workgroup per tile.  pooled: G words in
 *     the layout of g; entry i <= j += mult (len g_ij - a_i a_j), the lower triangle is never touched.  LEAVES a AND g ZERO (the
 *     kernel clears the g word it owns, a is cleared by a stream-ordered memset behind it).
 *   dc_roi_pair_corr_pooled: corr float[G] as dc_roi_pair_corr writes it, the lower triangle mirrored: bit-symmetric, the diagonal
 *     exactly 1 for a pixel that varies within some segment; row, column and diagonal exactly 0 for one constant within every segment.
 *   dc_roi_pixel_fold_segment: mom and the CSR as for dc_roi_pixel_accumulate over the segment; rmom = int64[3 * R], what
 *     dc_roi_trace_moments gives for the segment's columns (sums + t_start, T = len).  pooled_xx, pooled_xs: N words each,
 *     += mult (len b - a^2) and mult (len c - a u); pooled_ss: R words, += mult (len w - u^2).  CLEARS the four planes of mom of
 *     every entry it folds.  A row whose row_roi is outside [0, R) is skipped.
 *   dc_roi_pixel_corr_pooled: corr float[N] by the inside / halo rule and dc_fp_corr; the entries of a row whose row_roi is outside
 *     [0, R) get 0. */
#define DC_DETREND_MAX_FRAMES 4096
int dc_series_fold_segment(const long* sum, const long* sumsq, const long* xy, const int* vmax, long len, long mult, long* pooled_var,
                           long* pooled_cov, long* sum_total, int* vmax_total, int H, int W, dc_stream_t stream);
int dc_series_finalize_pooled(const long* pooled_var, const long* pooled_cov, const long* sum_total, float* mean, float* sdev, float* corr,
                              int H, int W, long M, long T, dc_stream_t stream);
int dc_roi_pair_fold_segment(long* a, long* g, const int* roi_off, const long* goff, const int* tiles, long ntiles, int R, int P, long G,
                             long len, long mult, long* pooled, dc_stream_t stream);
int dc_roi_pair_corr_pooled(const long* pooled, const int* roi_off, const long* goff, int R, int P, long G, float* corr, dc_stream_t stream);
int dc_roi_pixel_fold_segment(long* mom, int N, const int* row_off, const int* row_roi, int S, int R, const long* rmom, long len, long mult,
                              long* pooled_xx, long* pooled_xs, long* pooled_ss, int H, int W, dc_stream_t stream);
int dc_roi_pixel_corr_pooled(const long* pooled_xx, const long* pooled_xs, const long* pooled_ss, int N, const int* row_off,
                             const int* row_roi, int S, int R, const int* inside, float* corr, dc_stream_t stream);

/* ---- ROI trace-pair correlation: the correlation over time of the traces of two ROIs ----------------------------------------------
 * The opposite mistake to the one the pixel-pair matrices catch: ONE cell that arrives as SEVERAL ROIs (a nucleus-excluded ring
 * broken into arcs, a cell cut by a one-pixel line of sub-threshold probability).  What decides a merge is the correlation of the
 * traces of two neighbouring ROIs, and its inputs already lie on the device after the streaming pass: the int64 sums of
 * dc_roi_trace_accumulate.  No further pass over the recording.  The reference has no counterpart; THESE DEFINITIONS ARE THE
 * SPECIFICATION.  Integers until the last step; the same bits every run and for every launch geometry.
 * sums = int64 rows of stride ld >= T (a column offset is the caller's pointer arithmetic: 8-byte alignment only), R rows.
 * pairs = int32[P][2] = (i, j): any order, i == j allowed, a pair may appear twice.  x = sums[i], y = sums[j].
 * seg_len = 0: one segment of T frames.  Otherwise L = seg_len in [2, DC_DETREND_MAX_FRAMES] and the T frames are cut as in the
 * section above: n = max(1, T / L) segments, the last absorbing the remainder, M = L * L_last (M = T when n == 1), mult_s = M / L_s.
 * L > T / 2 is one segment: the bits of seg_len = 0.
 *   dc_trace_pair_moments: num = int64[P][6] = {Nxx_lo, Nxx_hi, Nxy_lo, Nxy_hi, Nyy_lo, Nyy_hi} (two's complement, hi * 2^64 + lo),
 *     N(x, y) = sum_s mult_s (L_s g_s - a_s a'_s) with a_s = sum x, a'_s = sum y in int64 and g_s = sum x y in 128 bits; Nxx = N(x, x),
 *     Nxy = N(x, y), Nyy = N(y, y): every pair is self-contained.  Every word of every p < P is written, each by one thread; a pair
 *     that names a row outside [0, R) gets zeros; nothing at or beyond P is touched.  No atomics.
 *     RANGE: exact whenever |S| * max(M, T) <= 2^62 for every value read -- e.g. |S| <= 2^16 A (an ROI of A 16-bit pixels) with
 *     max(M, T) * A <= 2^46, the volume limits above; then |N| <= 2^124 (csrc/trace_pair_math.h derives it).  THE CALLER PROMISES
 *     this (not checked), as for dc_trace_baseline.  Neuropil-corrected numerators (|N| < 2^62) are outside it.
 *   dc_trace_pair_corr: corr float[P] = dc_fp_corr of csrc/footprint_math.h on {Nxx, Nxy, Nyy}: (float)(f64(Nxy) / (sqrt(f64(Nxx)) *
 *     sqrt(f64(Nyy)))), each numerator rounded ONCE to double, no fused multiply-add: within 1 float32 ulp, in [-1, 1], the same
 *     bits for (i, j) and (j, i); exactly 1 for i == j on a row that varies, exactly 0 where either row is constant within every
 *     segment (zero numerators, so also for a pair that names no row), exactly -1 for a row against its mirror image c - x.
 * Refused: a null pointer, a negative size, ld < T, a misaligned buffer, seg_len < 0 or == 1: DC_EINVAL (-1); T > 2^31 - 1,
 * seg_len > DC_DETREND_MAX_FRAMES, P > DC_TRACE_PAIR_MAX_PAIRS: DC_EUNSUP (-3).  P == 0, R == 0 or T == 0: 0, nothing launched.
 * All pointers are DEVICE memory, there are no out-parameters and nothing is read on the host. */
#define DC_TRACE_PAIR_MAX_PAIRS 16777216L
int dc_trace_pair_moments(const long* sums, long ld, int R, long T, int seg_len, const int* pairs, long P, long* num, dc_stream_t stream);
int dc_trace_pair_corr(const long* num, long P, float* corr, dc_stream_t stream);

/* ---- Frame quality: per-frame scores that find artefact frames, and the gather that leaves them out --------------------------------
 * A stimulation-light flash, a gated (dark) PMT frame, a z-jump: in such a frame ALL pixels move together, so three of them in a
 * thousand push every pixel-pair and trace-pair correlation towards 1, become the `max` image and inflate `std`.  What finds them
 * is a score per frame, computed where the frames already are; the rule on the scores is the host's (frames.flag_frames).  The
 * reference has no counterpart; THESE DEFINITIONS ARE THE SPECIFICATION.  Integers until the last step; the same bits every run
 * and for every launch geometry.
 * frames = tc dense H x W frames of 16 bits, int16 or uint16 (is_unsigned); tmpl = NULL or one H x W image of the SAME type (what
 * make_template returns).  The rectangle is rows [y0, y1), columns [x0, x1) of the frame, n = (y1 - y0) * (x1 - x0) pixels
 * (valid_rectangle's, or the whole frame); 2-byte alignment of frames and tmpl is all that is asked.
 *   dc_frame_moments: moments = int64[tc][3] = {a, b, c} per frame over the rectangle: a = sum x, b = sum x^2, c = sum x * tmpl
 *     (0 with tmpl == NULL).  n <= DC_FRAME_MAX_PIXELS = 2^28 keeps |a| < 2^44, b < 2^60, |c| < 2^60 (csrc/frame_math.h).  The
 *     rows are zeroed by the call itself (never pre-clear) and the workgroups' partial sums are added with 64-bit integer atomics:
 *     integer addition, so the order changes no bit.  Nothing at or beyond tc is touched.  The template's own sums ta = sum tmpl,
 *     tb = sum tmpl^2 are this function run on the template as a chunk of one frame.
 *   dc_frame_quality: mean[f] = (float)((double)a / (double)n); corr[f] (corr may be NULL) = dc_fp_corr of csrc/footprint_math.h on
 *     the 128-bit numerators {n b - a a, n c - a ta, n tb - ta ta}: (float)(f64(Nxt) / (sqrt(f64(Nxx)) * sqrt(f64(Ntt)))), each
 *     numerator rounded ONCE to double, no fused multiply-add: within 1 float32 ulp, in [-1, 1]; exactly 0 for a frame or a
 *     template that is constant over the rectangle (n == 1 included), exactly 1 for a frame equal to a template that varies,
 *     exactly -1 for frame = k - tmpl.  THE CALLER TIES THE ARGUMENTS TOGETHER (not checked, nothing here can): n must be the pixel
 *     count of the very rectangle that was passed to dc_frame_moments for these moments, and ta, tb the template's sums over that
 *     same rectangle; a mismatch gives wrong means and correlations without an error.
 *   dc_frame_gather: out[i] = frames[idx[i]] for i < k, a move of 16-bit values; idx = int32[k] in DEVICE memory; an entry outside
 *     [0, tc) gives an all-zero frame and is never followed.  out must not overlap frames.  k == 0 launches nothing.
 * Refused: a null pointer that would be followed, a negative or zero size, a rectangle that is empty or leaves the frame, n < 1, a
 * misaligned buffer (moments 8 bytes, mean / corr / idx 4, frames 2), out overlapping frames: DC_EINVAL (-1); n > 2^28 or
 * H * W > 2^30: DC_EUNSUP (-3).  tc == 0: 0, nothing launched.  All pointers are DEVICE memory, there are no out-parameters and
 * nothing is read on the host. */
#define DC_FRAME_MAX_PIXELS 268435456L
int dc_frame_moments(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int y0, int y1, int x0, int x1,
                     long* moments, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_frame_quality(const long* moments, int tc, long n, long ta, long tb, float* mean, float* corr, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_frame_gather(const void* frames, int tc, const int* idx, int k, int H, int W, void* out, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */

/* ---- dF/F traces: neuropil correction, rolling-percentile baseline, (F - F0) / F0 -----------------------------------------------
 * The step between ROI traces and spikes that the z-score above cannot replace: a recording bleaches and drifts, and every ROI
 * collects out-of-focus neuropil light.  The reference has no counterpart; THESE DEFINITIONS ARE THE SPECIFICATION.  Integers end
 * to end, one rounding at the end, no dependence on how the recording was chunked.
 * Inputs: S[r][t], the int64 ROI sums dc_roi_trace_accumulate writes, and A[r], the ROI areas.
 *   offset   o: an integer dark level added to every pixel, |o| <= 65535 (default 0).
 *   weight   w in [0, 1], taken in 256ths: a = floor(256 w + 0.5).
 *   numerator N[r][t] and denominator D[r] (int64; the corrected per-pixel fluorescence is N / D):
 *     without neuropil, or for an ROI whose ring is empty:   N = S + o A,                               D = A;
 *     with a ring of An > 0 pixels and sums Sn:              N = 256 An (S + o A) - a A (Sn + o An),    D = 256 An A.
 *     The HOST checks An * A < 2^36 before anything is launched: |S + o A| < 2^17 A for 16-bit pixels, so |N| < 2^62.
 *   window   half-width h in [0, DC_TRACE_BASELINE_MAX_HALF]: the window of frame t is [max(0, t - h), min(T - 1, t + h)], n frames
 *            -- clipped at the ends of the trace, never padded.
 *   rank     integer percentile q in [0, 100]: k = (q * (n - 1)) / 100 in INTEGER division.  Not numpy's float rule
 *            (floor(0.29 * 100) is 28, this gives 29; the two differ in 198 (q, n) pairs for n < 4096): the oracle is
 *            np.sort(window)[k], never np.percentile.
 *   baseline B[r][t] = the k-th smallest (0-based) of N[r] over the window, int64.  Ties are values: which of two equal samples is
 *            picked cannot matter.
 *   dF/F     dff[r][t] = (float)((double)(N - B) / (double)B) where B > 0, exactly 0.f where B <= 0.  N - B is formed in int64 (no
 *            overflow below 2^62); each int64 -> double conversion is one round-to-nearest, like numpy's: bit-equal to
 *            ((N - B).astype(float64) / B.astype(float64)).astype(float32).  D cancels.
 *   scaled   f = (float)((double)N / (double)D), baseline = (float)((double)B / (double)D).
 * All pointers are DEVICE memory, there are no out-parameters and nothing is read on the host.
 *   dc_trace_combine: num[r][t] = ca[r] * sums[r][t] - cb[r] * sums[np_row[r]][t] + cc[r] in int64, r < R.  sums = int64 rows of
 *     stride ld; np_row int32[R]: np_row[r] < 0 means no second term, otherwise ANY row of sums, rows >= R included (the rings
 *     of a streaming pass follow the ROIs); ca, cb, cc int64[R] come from the host (the formulas above); num int64[R][T] dense.
 *   dc_trace_baseline: num = int64 rows of stride ld; base int64[R][T] and dff float[R][T], each nullable and dense.  THE CALLER
 *     PROMISES |num| < 2^62 (not checked).  half > DC_TRACE_BASELINE_MAX_HALF: DC_EUNSUP (-3); q outside [0, 100], a negative
 *     count, ld < T or a misaligned buffer: -1.  R == 0 or T == 0: 0, nothing launched.
 *   dc_trace_scale: out[r][t] = (float)((double)x[r][t] / (double)den[r]), exactly 0 where den[r] <= 0; x = int64 rows of stride
 *     ld, den int64[R], out float[R][T] dense. */
#define DC_TRACE_BASELINE_MAX_HALF 2047
int dc_trace_combine(const long* sums, long ld, const int* np_row, const long* ca, const long* cb, const long* cc, int R, long T,
                     long* num, dc_stream_t stream);
int dc_trace_baseline(const long* num, long ld, int R, long T, int half, int q, long* base, float* dff, dc_stream_t stream);
int dc_trace_scale(const long* x, long ld, const long* den, int R, long T, float* out, dc_stream_t stream);

/* ---- Spikes by deconvolution: non-negative AR(1) deconvolution of a trace, without a trained model ---------------------------
 * The last stage of the chain for a user who has no UNet1D model file: calcium c[t] = g c[t-1] + s[t] with s >= 0 is fitted to
 * every trace by the pool-merging (OASIS-style) forward pass below.  The reference has no counterpart; THESE DEFINITIONS ARE THE
 * SPECIFICATION.  A trace is sequential, but it consists only of IEEE double adds, multiplies, one division per merge and
 * comparisons: with the operation order fixed (csrc/deconv_math.h, no fused multiply-add, no reassociation) and the powers of g
 * taken from one table, the result is defined bit for bit, on the device and on the host.
 * Inputs
 *   y[r][t]  float32 or float64 rows of stride ld >= T (is_f64 = 0 / 1); float32 is widened to double exactly.  THE CALLER
 *            PROMISES FINITE VALUES (not checked on the device; the Python layer checks host arrays).  Feed dF/F; a constant
 *            baseline per trace can be given or fitted ("A baseline in the deconvolution" below).
 *   G[0..T]  double, T + 1 entries: G[0] = 1, G[l] = G[l-1] * g, built ONCE ON THE HOST by that loop of multiplications, never by
 *            pow().  g = G[1], 0 < g < 1.
 *   lam[r] >= 0, smin[r] >= 0: doubles per trace, the L1 penalty on the spikes and the smallest spike allowed.
 * Forward pass, per trace: a stack of pools (v, w, t0, l).  For t = 0 .. T - 1:
 *   push (y[t] - mu, 1.0, t, 1), mu = lam * (1.0 - g) for t < T - 1 and mu = lam for t = T - 1;
 *   with p the pool below the top pool q: while the stack holds at least two pools and v_q < G[l_p] * v_p + smin, merge
 *     a = G[l_p];  num = w_p * v_p + (a * w_q) * v_q;  den = w_p + (a * a) * w_q;  v_p = num / den;  w_p = den;  l_p += l_q;  pop q.
 *   The parentheses are the evaluation order.
 * Outputs, float64 and dense, every element written (the caller need not clear them):
 *   calcium[r][t0_i + k] = b_i * G[k] for 0 <= k < l_i, b_i = v_i where v_i > 0.0 and +0.0 otherwise;
 *   spikes[r][t0_i] = calcium[t0_i] - g * calcium[t0_i - 1] for every pool i >= 1, exactly +0.0 at every other frame, frame 0
 *     included.  Not clamped: with smin = 0 it can be below zero by rounding only.  An event is spikes > 0.
 *   pools[r]: int32, the final number of pools.
 * Not built: AR(2); optimising g by the residual; a time-varying baseline; a wave-parallel segment merge (it would change the operation
 * order and so the bits); integer-exact arithmetic (the pool values are not closed under any fixed-point format).
 *   dc_trace_deconv_ws_bytes: the workspace of dc_trace_deconv_ar1, 24 * R * T bytes (0 for an empty or unsupported shape).
 *   dc_trace_deconv_ar1: forward pass (one lane per trace, 64 traces per workgroup), then the fill (one thread per sample).  All
 *     pointers are DEVICE memory.  g is passed by value and must equal G[1].  ws holds the pools below the top one as [depth][R]
 *     planes (v, w, (t0, l)); its contents afterwards are the final stacks.  lam and smin are not read on the host: THE CALLER
 *     PROMISES lam, smin >= 0.  T > 2^24 or R * T > 2^31: DC_EUNSUP (-3).  g outside (0, 1), a null pointer, a negative count,
 *     ld < T or a misaligned buffer (8 bytes; 4 for float32 y and for pools): -1.  R == 0 or T == 0: 0, nothing launched.
 *   dc_trace_deconv_ar1_host: the same arithmetic (the same header) compiled for the host, over HOST pointers, one trace after the
 *     other on the calling thread; it allocates T pools of host memory for the duration of the call.  g = G[1]; G[0] != 1, a
 *     negative or NaN lam[r] or smin[r]: -1; otherwise the codes above.  The speed baseline, and the bit-for-bit check of the
 *     library against the oracle on a machine without a GPU.
 * The noise-constrained search: one of the two parameters is not given but found, per trace, so that the residual equals the
 * noise (OASIS, CaImAn's constrained foopsi): the largest p tried with RSS(p) <= sigma^2 T.  csrc/deconv_search_math.h is the one
 * implementation.  which = DC_TRACE_DECONV_SEARCH_SMIN (0) or DC_TRACE_DECONV_SEARCH_LAM (1) names the searched parameter; the
 * other one stays at fixed_other[r] >= 0.  sigma[r]: finite, >= 0 and below 2^500.  rounds = N in [1, 64].
 *   RSS(p): the forward pass above with the searched parameter at p; c[t] = the calcium output; d_t = (double)y[t] - c[t];
 *     RSS = fold(t -> d_t * d_t, T), the fold of "Trace dynamics" below (256 lane sums, then the tree); the product is rounded
 *     once.
 *   target = (sigma * sigma) * (double)T.
 *   round 0: p = 0.0, r0 = RSS(0).  If !(r0 < target): p* = 0, status 1, rss = r0 (the residual reaches the noise unconstrained;
 *     sigma = 0 ends here).  Otherwise lo = 0, rss_lo = r0, hi = sigma, expanding.
 *   rounds 1 .. N: p = expanding ? hi : 0.5 * (lo + hi); r = RSS(p).  r <= target: lo = p, rss_lo = r, and hi = hi + hi while
 *     expanding.  Otherwise hi = p and the search stops expanding for good.
 *   end: p* = lo, rss = rss_lo, status = expanding ? 2 : 0.  Status 2: never bracketed, the constraint is still slack at p*.
 *   calcium, spikes, pools: the outputs above at p*, the bits dc_trace_deconv_ar1 gives for that parameter.
 *   Promised: RSS(p*) <= target for status 0 and 2; for status 0 also RSS(hi) > target, and after e expanding rounds (the one
 *     that failed included) and N - e bisections hi - lo = 2^max(e-2, 0) sigma / 2^(N-e), to the rounding of the midpoints.
 *     RSS is monotone in lam, so p* is the constrained optimum to that resolution; it is NOT monotone in smin, where only the
 *     invariant holds.
 *   dc_trace_deconv_search_state_bytes: the state of dc_trace_deconv_ar1_constrained, 40 * R bytes (0 for R <= 0): five planes of
 *     R 8-byte words, lo, hi, rss_lo, target (doubles) and the phase (an integer); afterwards plane 3 holds the targets.
 *   dc_trace_deconv_ar1_constrained: enqueues round 0, the N rounds and the final pass -- N + 2 forward passes, each but the last
 *     followed by one residual-and-step launch (one workgroup of 256 threads per trace, at most
 *     DC_TRACE_DECONV_SEARCH_MAX_GROUPS workgroups: beyond, a workgroup walks several traces), then the fill -- with no host
 *     synchronisation and nothing read back.  All pointers are DEVICE memory.  gs == NULL: one decay g (by value, = G[1]) and
 *     one table G for all traces, ldG is not used.  Otherwise trace r uses gs[r] and the row G + r * ldG, as in
 *     dc_trace_deconv_ar1_each below, and g is not used.  ws: dc_trace_deconv_ws_bytes.  param = double[R], rss = double[R],
 *     status = int32[R]; param is also the array the forward passes read the searched parameter from.  THE CALLER PROMISES
 *     sigma and fixed_other in the ranges above (not checked: nothing is read on the host) and, per trace, 0 < gs[r] < 1 =
 *     G[r][1].  which or rounds out of range, ldG < T + 1 with gs given: -1; otherwise the codes of dc_trace_deconv_ar1.
 *   dc_trace_deconv_search_step: one residual-and-step launch alone, what dc_trace_deconv_ar1_constrained enqueues after every
 *     forward pass but the final one: the residual of the stacks in ws (pools[r] of them per trace), then the step of every
 *     trace's search in `state`, which writes the next parameter to param (last = 1: p*, rss and status instead).  ldG = 0: one
 *     table for all traces; ldG >= T + 1: row r of G.  THE CALLER PROMISES that ws, pools, state and param are those of a
 *     dc_trace_deconv_ar1_constrained call on the same y, R and T.  It is here to be timed by itself.
 *   dc_trace_deconv_ar1_constrained_host: the same arithmetic (the same headers) compiled for the host, over HOST pointers, one
 *     decay for all traces (g = G[1]), one trace after the other on the calling thread; sigma and fixed_other are checked (-1).
 *     The speed baseline, and the bit-for-bit check against the oracle on a machine without a GPU.
 * Not built for the search: AR(2); both parameters at once; a warm start (every round is a full forward pass); the OASIS closed-
 * form update of lam (it would change the operation order); a joint search over g.
 * A baseline in the deconvolution: one constant b = base[r] per trace, given or fitted.  dF/F over a low rolling percentile sits
 * about one noise sigma above zero in its quiet stretches; the non-negative model has no term for a constant and pays for the
 * offset with spurious spikes.  csrc/deconv_base_math.h is the one implementation.  base = double[R], finite.
 *   forward pass: the pushed value is x = ((double)y[t] - b) - mu, in that order; z - 0.0 is z for every double, so b = 0 gives the
 *     bits of the entry points above.  calcium stays c, without the baseline: the fitted trace is c + b.
 *   for the stacks a forward pass at (p, b) left: d_t = ((double)y[t] - b) - calcium[t]; RSS = fold(d_t * d_t, T); S = fold(d_t, T);
 *     A = fold(a_t, T) with a_t = +0.0 except at the first frame of a pool with v > 0, where, l the pool's length and g = G[1],
 *     u = (1.0 - G[l]) / (1.0 - g), q = (1.0 - G[l] * G[l]) / (1.0 - g * g), a_t = (u * u) / q.  Within a pool v is the G-weighted
 *     least-squares value, so for the current partition d(sum c)/db = -A and T - A is -T dphi/db of the mean residual phi = S / T.
 *   baseline step: den = 1.0 - A / (double)T; if !(den > 0.25) den = 0.25; b' = b + (S / (double)T) / den.  A clamped Newton step on
 *     phi(b) = 0, the stationarity condition in b of both the lam and the smin problem (the penalty does not involve b).
 *   fit at fixed parameters, rounds = N in [1, DC_TRACE_DECONV_BASE_MAX_ROUNDS]: from b_0 = base on entry, N times a forward pass at
 *     b and the step; then the forward pass and the fill at b_N, which base holds afterwards.  With a threshold that is too high
 *     the missed events' fluorescence is absorbed into b: fit the baseline together with the noise-constrained search.
 *   joint search (which, sigma, fixed_other, rounds = N as above; the state gains b, carried, and b_lo):
 *     round 0: p = 0, b = b_0, r0 = RSS; no baseline step (at p = 0 the baseline is not identifiable).  !(r0 < target): status 1,
 *       p* = 0, b* = b_0.  Otherwise lo = 0, b_lo = b_0, rss_lo = r0, hi = sigma, expanding.
 *     rounds 1 .. N: p = expanding ? hi : 0.5 * (lo + hi).  Pass A at (p, b) gives S and A, hence b'.  Pass B at (p, b') gives
 *       r = RSS.  r <= target: lo = p, b_lo = b', rss_lo = r, and hi = hi + hi while expanding.  Otherwise hi = p and the expansion
 *       is over.  Either way b = b' is carried into the next round.
 *     end: p* = lo, b* = b_lo, rss = rss_lo, statuses as above; one last forward pass and the fill at (p*, b*).
 *     Promised: RSS(p*, b*) <= target for status 0 and 2, evaluated at exactly that pair (so it does not depend on b having
 *       converged); the outputs are the bits dc_trace_deconv_ar1_base gives at (p*, b*); the bracket-width formula above.  NOT
 *       promised: that b* is the exact minimiser, or (smin) that no larger threshold also satisfies the constraint.
 *   dc_trace_deconv_ar1_base: forward pass and fill with the baseline base[r].  gs == NULL: one decay g (by value, = G[1]) and one
 *     table; otherwise gs[r] and the row G + r * ldG, as in dc_trace_deconv_ar1_constrained.  THE CALLER PROMISES FINITE base.
 *   dc_trace_deconv_ar1_fit_base: the fit: N forward passes, each followed by one launch of the residual kernel (DC_TRACE_DECONV_BASE_FIT),
 *     then forward and fill; nothing is read back.  base is read (b_0) and written (b_N).
 *   dc_trace_deconv_base_state_bytes: the state of dc_trace_deconv_ar1_constrained_base, 56 * R bytes (0 for R <= 0): the five
 *     planes of the plain search, then b and b_lo; plane 3 holds the targets.
 *   dc_trace_deconv_ar1_constrained_base: the joint search: 2 N + 2 forward passes, each but the last followed by one launch of the
 *     residual kernel, then the fill; no host synchronisation, nothing read back.  base is read (b_0) and written (b*); param and
 *     base are also the arrays the forward passes read.  Promises and codes as for dc_trace_deconv_ar1_constrained.
 *   dc_trace_deconv_base_step: one launch of the residual kernel alone: RSS, S and A of the stacks in ws (pools[r] of them per
 *     trace) at base[r] in one sweep -- one workgroup of 256 threads per trace, at most DC_TRACE_DECONV_SEARCH_MAX_GROUPS workgroups --,
 *     then by mode: DC_TRACE_DECONV_BASE_FIT (0) base[r] = b' (state, param, rss and status may be NULL); _PASS_A (1) the same
 *     for every search that is not finished, b kept in the state; _PASS_B (2) the step of the search, the next parameter to
 *     param; _PASS_LAST (3) that step, then p*, b*, rss and status.  sums = NULL, or double[3][R]: the three folds.  ldG = 0: one
 *     table for all traces; ldG >= T + 1: row r of G; g = G[1] of that table.  THE CALLER PROMISES that ws, pools, state, param and
 *     base are those of one of the two calls above on the same y, R and T.  It is here to be timed by itself.
 *   dc_trace_deconv_ar1_fit_base_host, dc_trace_deconv_ar1_constrained_base_host: the same arithmetic (the same headers) compiled
 *     for the host, over HOST pointers, one trace after the other on the calling thread.  ldG = 0: one table for all traces,
 *     otherwise row r of G; g = G[1] of the table.  What is read is checked (-1), a baseline that is not finite included.  The fit
 *     also takes rounds = 0: the given baseline, the host twin of dc_trace_deconv_ar1_base.
 * Not built for the baseline: a time-varying baseline; a joint search over g; AR(2). */
#define DC_TRACE_DECONV_SEARCH_SMIN 0
#define DC_TRACE_DECONV_SEARCH_LAM 1
#define DC_TRACE_DECONV_SEARCH_MAX_ROUNDS 64
#define DC_TRACE_DECONV_SEARCH_MAX_GROUPS 8192
#define DC_TRACE_DECONV_MAX_FRAMES 16777216L
#define DC_TRACE_DECONV_MAX_SAMPLES 2147483648L
long dc_trace_deconv_ws_bytes(int R, long T);
int dc_trace_deconv_ar1(const void* y, int is_f64, long ld, int R, long T, double g, const double* G, const double* lam,
                        const double* smin, void* ws, double* calcium, double* spikes, int* pools, dc_stream_t stream);
int dc_trace_deconv_ar1_host(const void* y, int is_f64, long ld, int R, long T, const double* G, const double* lam, const double* smin,
                             double* calcium, double* spikes, int* pools);
long dc_trace_deconv_search_state_bytes(int R);
int dc_trace_deconv_ar1_constrained(const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                                    int which, const double* sigma, const double* fixed_other, int rounds, void* ws, void* state,
                                    double* calcium, double* spikes, int* pools, double* param, double* rss, int* status,
                                    dc_stream_t stream);
int dc_trace_deconv_search_step(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const void* ws,
                                const int* pools, int last, void* state, double* param, double* rss, int* status, dc_stream_t stream);
int dc_trace_deconv_ar1_constrained_host(const void* y, int is_f64, long ld, int R, long T, const double* G, int which, const double* sigma,
                                         const double* fixed_other, int rounds, double* calcium, double* spikes, int* pools, double* param,
                                         double* rss, int* status);
#define DC_TRACE_DECONV_BASE_MAX_ROUNDS 64
#define DC_TRACE_DECONV_BASE_FIT 0
#define DC_TRACE_DECONV_BASE_PASS_A 1
#define DC_TRACE_DECONV_BASE_PASS_B 2
#define DC_TRACE_DECONV_BASE_PASS_LAST 3
long dc_trace_deconv_base_state_bytes(int R);
int dc_trace_deconv_ar1_base(const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                             const double* lam, const double* smin, const double* base, void* ws, double* calcium, double* spikes, int* pools,
                             dc_stream_t stream);
int dc_trace_deconv_ar1_fit_base(const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                                 const double* lam, const double* smin, int rounds, void* ws, double* calcium, double* spikes, int* pools,
                                 double* base, dc_stream_t stream);
int dc_trace_deconv_ar1_constrained_base(const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G,
                                         long ldG, int which, const double* sigma, const double* fixed_other, int rounds, void* ws, void* state,
                                         double* calcium, double* spikes, int* pools, double* param, double* base, double* rss, int* status,
                                         dc_stream_t stream);
int dc_trace_deconv_base_step(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const void* ws, const int* pools,
                              int mode, void* state, double* param, double* base, double* rss, int* status, double* sums, dc_stream_t stream);
int dc_trace_deconv_ar1_fit_base_host(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const double* lam,
                                      const double* smin, int rounds, double* calcium, double* spikes, int* pools, double* base);
int dc_trace_deconv_ar1_constrained_base_host(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, int which,
                                              const double* sigma, const double* fixed_other, int rounds, double* calcium, double* spikes,
                                              int* pools, double* param, double* base, double* rss, int* status);

/* ---- A rise time in the deconvolution: AR(2) -----------------------------------------------------------------------------------
 * The AR(1) model above lets a spike raise the fluorescence within one frame; an indicator that takes several frames to peak is
 * then explained as a run of spikes.  Here c[t] = g1 c[t-1] + g2 c[t-2] + s[t], s >= 0, with two real roots 0 < r < d < 1 per
 * frame, d the decay and r the rise: g1 = d + r, g2 = -(d * r), one pair for all traces.  csrc/deconv_ar2_math.h is the one
 * implementation; the reference has no counterpart, THESE DEFINITIONS ARE THE SPECIFICATION.  IEEE doubles in the order written,
 * the parentheses included, no fused multiply-add, no reassociation: the result is defined bit for bit, on the device and on the host.
 * y, ld, is_f64, lam, smin, base as above.
 *   H  double, three rows of stride ldH >= T + 1, BUILT ONCE ON THE HOST (deep_calcium_amd.deconv.ar2_table), T + 1 entries each:
 *        h[0] = 1.0, h[1] = g1, h[k] = g1 * h[k-1] + g2 * h[k-2]: the response to one spike; H(k) = h[k], and +0.0 for k < 0;
 *        HH[0] = 0.0, HH[l+1] = HH[l] + h[l] * h[l];   HP[0] = 0.0, HP[l+1] = HP[l] + h[l] * h[l-1], the term of l = 0 being +0.0.
 *      The tail of h underflows through the subnormals and may change sign there; those values are part of the definition.
 *   A pool covers l frames from t0 and holds v, the fitted calcium at t0; u, the calcium at t0 - 1 (the last value of the pool
 *   below, +0.0 for the lowest pool); and two data moments, A = sum_k h[k] x[t0+k] and B = sum_k H(k-1) x[t0+k].
 *     calc(p, k) = b for k = 0 and h[k] * b + (g2 * h[k-1]) * u_p for k >= 1, b = v_p where v_p > 0.0 and +0.0 otherwise;
 *     fit(p) = (A_p - (g2 * u_p) * HP[l_p]) / HH[l_p]: the least-squares value given u.
 * Forward pass, frame t: x = ((double)y[t] - base) - mu_t, mu_t = lam * ((1.0 - g1) - g2) for t < T - 2, lam * (1.0 - g1) at
 * t = T - 2 and lam at t = T - 1.
 *   1. cur = (A = x, B = +0.0, t0 = t, l = 1).
 *   2. No pool below cur: u_cur = +0.0, v_cur = fit(cur); the frame is done.
 *   3. p the pool right below: last = calc(p, l_p - 1); sec = l_p >= 2 ? calc(p, l_p - 2) : u_p; u_cur = last; v_cur = fit(cur).
 *   4. If !(v_cur < (g1 * last + g2 * sec) + smin) the frame is done.
 *   5. Otherwise merge, m = l_p: A = (A_p + h[m] * A_cur) + (g2 * h[m-1]) * B_cur; B = (B_p + h[m-1] * A_cur) + (g2 * H(m-2)) * B_cur;
 *      t0 = t0_p, l = m + l_cur; p is gone, cur is the merged pool; go to 2.
 *   The shift identity h[m+k] = h[m] h[k] + g2 h[m-1] h[k-1] makes A and B of the merged pool the sums of its frames: a merge is a
 *   handful of operations however long the pools are.
 * Outputs, float64 and dense, every element written: calcium[r][t0 + k] = calc(p, k); spikes[r][t0] = (calcium[t0] - g1 * last) -
 *   g2 * sec for every pool but the lowest, last and sec of the pool below as in step 3, +0.0 at every other frame; pools[r].
 * Promised: the bits; feasibility up to rounding (calcium >= 0, spikes above -1e-9 max|y|).  NOT promised: optimality.  Unlike
 *   AR(1), the greedy pass fits a pool without regard to the pools it later supports (OASIS's own approximation for p = 2).
 * The noise-constrained search is the one above, unchanged: the state, the rounds, the statuses, target.  Only RSS(p) is new: the
 *   fold of ((double)y[t] - calcium[t])^2 over the AR(2) stacks.  It takes no baseline.
 *   dc_trace_deconv_ar2_ws_bytes: the workspace, 40 * R * T bytes (0 for an empty or unsupported shape): the pools as [depth][R]
 *     planes v, u, A, B, (t0, l).
 *   dc_trace_deconv_ar2: forward pass (one lane per trace, 64 traces per workgroup), then the fill.  All pointers are DEVICE
 *     memory; base = double[R] or NULL.  THE CALLER PROMISES lam, smin >= 0, a finite base and a table H of these g1, g2.  g2 >= 0,
 *     g1 <= 0, g1 + g2 >= 1, g1 * g1 + 4.0 * g2 <= 0, ldH < T + 1, a null or misaligned pointer: -1; the limits of the
 *     deconvolution above: -3.  R == 0 or T == 0: 0, nothing launched.
 *   dc_trace_deconv_ar2_constrained: N + 2 forward passes, each but the last followed by one residual-and-step launch, then the
 *     fill; arguments, promises and codes as for dc_trace_deconv_ar1_constrained (state: dc_trace_deconv_search_state_bytes).
 *   dc_trace_deconv_ar2_host, dc_trace_deconv_ar2_constrained_host: the same arithmetic (the same header) compiled for the host,
 *     over HOST pointers, one trace after the other on the calling thread.  What is read is checked (-1), the first entries of the
 *     table included.
 * (g1, g2) from the traces themselves: "Trace dynamics: AR(2) coefficients" below.
 * Not built: fitting the baseline under AR(2) (A of "A baseline in the deconvolution" has no AR(2) form yet); a pair of roots per
 * trace; complex or equal roots; OASIS's corrective passes towards the exact optimum. */
long dc_trace_deconv_ar2_ws_bytes(int R, long T);
int dc_trace_deconv_ar2(const void* y, int is_f64, long ld, int R, long T, double g1, double g2, const double* H, long ldH, const double* lam,
                        const double* smin, const double* base, void* ws, double* calcium, double* spikes, int* pools, dc_stream_t stream);
int dc_trace_deconv_ar2_host(const void* y, int is_f64, long ld, int R, long T, double g1, double g2, const double* H, long ldH,
                             const double* lam, const double* smin, const double* base, double* calcium, double* spikes, int* pools);
int dc_trace_deconv_ar2_constrained(const void* y, int is_f64, long ld, int R, long T, double g1, double g2, const double* H, long ldH, int which,
                                    const double* sigma, const double* fixed_other, int rounds, void* ws, void* state, double* calcium,
                                    double* spikes, int* pools, double* param, double* rss, int* status, dc_stream_t stream);
int dc_trace_deconv_ar2_constrained_host(const void* y, int is_f64, long ld, int R, long T, double g1, double g2, const double* H, long ldH,
                                         int which, const double* sigma, const double* fixed_other, int rounds, double* calcium, double* spikes,
                                         int* pools, double* param, double* rss, int* status);

/* ---- Trace dynamics: noise and AR(1) decay -----------------------------------------------------------------------------------
 * The one parameter of the deconvolution above that had no data-driven default: the decay g, which depends on indicator,
 * expression level, temperature and cell type.  Per trace, from the whole trace: the robust noise sigma of its first difference
 * (what sets smin), its autocovariance xc at lags 0 .. lags, and CaImAn's least-squares AR(1) coefficient with the noise removed
 * at lag 0 only.  The reference has no counterpart; THESE DEFINITIONS ARE THE SPECIFICATION (csrc/trace_dyn_math.h is their one
 * implementation: IEEE doubles, no fused multiply-add, no reassociation).  y, ld, is_f64 as above; float32 is widened exactly.
 *   noise, by VALUE (order-free): d[t] = y[t+1] - y[t], t in [0, T-1).  med(x) of n values: the (n-1)/2-th smallest for odd n,
 *     (x_(n/2-1) + x_(n/2)) / 2.0 for even n.  m = med(d), mad = med(|d - m|), sigma = (1.4826 * mad) / sqrt(2.0); sigma = 0.0 for
 *     T < 3.  Bit-equal to numpy's 1.4826 * median(|d - median(d)|) / sqrt(2) (deep_calcium_amd.deconv.trace_noise).
 *   fold(f, n), FIXED ORDER, W = DC_TRACE_DYN_LANES = 256: (1) for j in [0, W): P[j] = +0.0, then for t = j, j + W, ... < n
 *     ascending P[j] = P[j] + f(t); (2) for h = 128, 64, ..., 1 and every j < h: P[j] = P[j] + P[j+h]; (3) the result is P[0].
 *     n <= 0 gives +0.0.
 *   autocovariance: mean = fold(y, T) / (double)T; for l = 0 .. lags: q_l = fold(t -> (y[t] - mean) * (y[t+l] - mean), T - l),
 *     xc_l = q_l / (double)T.  lags in [1, DC_TRACE_DYN_MAX_LAGS].
 *   decay: A_0 = xc_0 - sn * sn, A_i = xc_i for 1 <= i < lags, b_i = xc_(i+1); num = the left fold from +0.0 of A_i * b_i over
 *     ascending i, den the same of A_i * A_i; g_raw = num / den.  g_raw = NaN (undefined) when T < lags + 2, when den == 0.0 or
 *     when the quotient is not finite.  sn is the sigma above unless the caller passes its own.  Adding a constant to the trace
 *     does not change the estimate.  g_raw is NOT clamped to (0, 1): that is the caller's (deep_calcium_amd.pick_gamma).
 * All pointers are DEVICE memory (except for the _host entry), there are no out-parameters and nothing is read on the host.
 * Columns >= T of a padded row are never read.  Every output word is written by one thread; no floating-point atomics.
 *   dc_trace_noise: sigma = double[R].  One 256-thread workgroup per trace (at most DC_TRACE_DYN_MAX_GROUPS workgroups: beyond,
 *     a workgroup walks several traces); the medians by a radix descent over a monotone 64-bit key of the double, no workspace.
 *   dc_trace_ar1_estimate: xc = double (R, lags + 1) dense, g_raw = double[R].  sn = double[R] or NULL: the noise that enters
 *     A_0.  sigma = double[R] or NULL: where given, the noise above is computed and written; with sn == NULL it is also what
 *     enters A_0, and sigma must then be given.  One launch, one workgroup per trace, capped as above.
 *   dc_ar1_tables: G[r][0] = 1.0, G[r][l] = G[r][l-1] * g[r] for l = 1 .. T; g = double[R], rows of stride ldG >= T + 1 (entries
 *     beyond T are not written).  Row r is bit-equal to the host's table of g[r].  T == 0 writes the one entry per row.
 *   dc_trace_deconv_ar1_each: dc_trace_deconv_ar1 with a decay and a table row per trace: g = double[R] in DEVICE memory, G the
 *     rows dc_ar1_tables writes.  Trace r gives the bits of dc_trace_deconv_ar1 run on that trace alone with g[r].  The same
 *     workspace (dc_trace_deconv_ws_bytes).  THE CALLER PROMISES 0 < g[r] < 1 and G[r][1] == g[r] (not checked: nothing is read
 *     on the host).  ldG < T + 1: -1; otherwise the codes of dc_trace_deconv_ar1.
 *   dc_trace_ar1_estimate_host: dc_trace_ar1_estimate compiled for the host (the same header), over HOST pointers, one trace
 *     after the other on the calling thread, the medians by std::nth_element; it allocates T - 1 doubles for the duration of the
 *     call.  The speed baseline, and the bit-for-bit check of the library against the oracle on a machine without a GPU.
 * Limits as for the deconvolution: T > 2^24 or R * T > 2^31: DC_EUNSUP (-3).  A null or misaligned pointer (8 bytes; 4 for
 * float32 y), ld < T, a negative count, lags outside [1, 16]: -1.  R == 0 or T == 0: 0, nothing launched (dc_ar1_tables: R == 0).
 * Not built: refining g by the deconvolution residual; noise from the power spectrum; per-segment estimates; weights on
 * the lags.  AR(2): the next section. */
#define DC_TRACE_DYN_LANES 256
#define DC_TRACE_DYN_MAX_LAGS 16
#define DC_TRACE_DYN_MAX_GROUPS 8192
int dc_trace_noise(const void* y, int is_f64, long ld, int R, long T, double* sigma, dc_stream_t stream);
int dc_trace_ar1_estimate(const void* y, int is_f64, long ld, int R, long T, int lags, const double* sn, double* sigma, double* xc,
                          double* g_raw, dc_stream_t stream);
int dc_ar1_tables(const double* g, int R, long T, double* G, long ldG, dc_stream_t stream);
int dc_trace_deconv_ar1_each(const void* y, int is_f64, long ld, int R, long T, const double* g, const double* G, long ldG,
                             const double* lam, const double* smin, void* ws, double* calcium, double* spikes, int* pools,
                             dc_stream_t stream);
int dc_trace_ar1_estimate_host(const void* y, int is_f64, long ld, int R, long T, int lags, const double* sn, double* sigma, double* xc,
                               double* g_raw);

/* ---- Trace dynamics: AR(2) coefficients ----------------------------------------------------------------------------------------
 * The two parameters of "A rise time in the deconvolution" from the traces themselves: CaImAn's estimate_time_constant(p = 2), a
 * least squares in two unknowns on the autocovariance, the noise removed on the diagonal.  The O(R T) work -- the two medians and
 * the lags + 1 folds -- is dc_trace_ar1_estimate above, unchanged; this is the per-trace epilogue on what it wrote.  THESE
 * DEFINITIONS ARE THE SPECIFICATION (csrc/trace_dyn_math.h, dc_dyn_ar2_solve: IEEE doubles, no fused multiply-add, this order).
 *   with c0 = xc_0 - sn * sn, rows i = 0 .. lags - 1:  a_i = (i == 0 ? c0 : xc_i),  b_i = (i == 0 ? xc_1 : i == 1 ? c0 : xc_(i-1)),
 *     y_i = xc_(i+1) -- toeplitz(xc[0 .. lags-1], xc[0 .. 1]) - sn^2 I, regressed on xc[1 .. lags];
 *   five left folds from +0.0 over ascending i: Saa += a_i * a_i, Sab += a_i * b_i, Sbb += b_i * b_i, Say += a_i * y_i,
 *     Sby += b_i * y_i;
 *   det = Saa * Sbb - Sab * Sab,  g1_raw = (Say * Sbb - Sby * Sab) / det,  g2_raw = (Saa * Sby - Sab * Say) / det.
 *   Both are NaN (undefined) when T < lags + 2, when !(det > 0.0) or when either quotient is not finite.  Nothing is clamped and
 *   no roots are taken: the roots d, r = (g1 +- sqrt(g1 * g1 + 4 g2)) / 2, which of them are usable and their pooling over the
 *   traces are the caller's (deep_calcium_amd.ar2_roots, pick_roots).
 *   dc_trace_ar2_solve: xc = double (R, lags + 1) dense, exactly as dc_trace_ar1_estimate writes it; sn = double[R], the sigma the
 *     same launch wrote or the caller's own; g12_raw = double (R, 2) dense.  All DEVICE memory; T is the length of the traces xc
 *     came from (it only decides whether the estimate is defined).  One lane per trace, 64 to a workgroup, at most
 *     DC_TRACE_DYN_MAX_GROUPS workgroups: beyond, a lane walks several traces.  Every output word is written by one thread.
 *   dc_trace_ar2_solve_host: the same function compiled for the host, over HOST pointers.
 * lags in [2, DC_TRACE_DYN_MAX_LAGS].  A null or misaligned pointer (8 bytes), lags outside [2, 16], a negative count: -1; the
 * limits of the deconvolution (T > 2^24, R * T > 2^31): -3.  R == 0: 0, nothing launched.
 * Not built: roots per trace in the deconvolution (one pooled pair serves all traces); complex or equal roots; per-segment
 * estimates; weights on the lags; fitting the baseline under AR(2). */
int dc_trace_ar2_solve(const double* xc, int R, long T, int lags, const double* sn, double* g12_raw, dc_stream_t stream);
int dc_trace_ar2_solve_host(const double* xc, int R, long T, int lags, const double* sn, double* g12_raw);

/* ---- rigid motion correction: register the frames of a recording to a template ------------------------------------------------
 * Every stage above assumes registered frames (Neurofinder's are; the recordings of the reference's other example,
 * examples/neurons/unet2ds_sj.py, were registered by an outside tool: it reads directories named ..._stabilized).  This is that
 * step: rigid, whole-pixel translation, found by exhaustive search within +-S, S <= DC_MOTION_MAX_SHIFT; the piecewise-rigid
 * mode built on it, the sub-pixel refinement of both and the two-level wide search (radii up to DC_MOTION_MAX_WIDE_SHIFT) follow
 * below.  FFT methods are out of scope.  Integer
 * arithmetic only: every result is exact, so the chunking
 * of a recording never changes a bit.
 * frames: as for dc_series_accumulate (int16 / uint16 by is_unsigned, [tc][H][W] contiguous, 2-byte aligned); tmpl: [H][W] of the
 * same type.  H > 2S and W > 2S (else DC_EINVAL); S > 16 or H * W > 2^30: DC_EUNSUP (-3).
 * SIGN CONVENTION: a shift (dy, dx) means out[y][x] = frame[y + dy][x + dx].  A frame cut from a scene at offset (+a, +b)
 * relative to the template is therefore found as (dy, dx) = (-a, -b).
 *   dc_motion_ssd: scores = int64[tc][2S+1][2S+1], dy the slow axis (index dy + S), fully written (never pre-clear):
 *     scores[t][dy+S][dx+S] = sum over the template's interior y in [S, H-S), x in [S, W-S) of (tmpl[y][x] - frame[y+dy][x+dx])^2
 *     -- every shift sums the same (H-2S)(W-2S) pixels and never reads outside the frame.  |d| <= 65535 and H * W <= 2^30, so a
 *     score is below 2^62.  S = 0 is legal (one score per frame).
 *   dc_motion_pick: shifts = int32[tc][2] (dy, dx), best = int64[tc] (nullable: the picked score).  The picked shift minimises
 *     the tuple (score, dy^2 + dx^2, dy, dx) lexicographically: a constant frame, or a pattern periodic within the window, gets the
 *     smallest displacement, and (0, 0) wins every tie it takes part in.
 *   dc_motion_apply: out[t][y][x] = frames[t][y + dy][x + dx] where that lies inside the frame, `fill` (a 16-bit value, given
 *     as an int in [-32768, 65535]) elsewhere; (dy, dx) = shifts[t] is read on the device.  A pure move of 16-bit values (the
 *     signedness does not matter).  Any int32 shift works (not only those within the search radius); |dy| >= H or |dx| >= W gives
 *     an all-fill frame.  out must not overlap frames (DC_EINVAL). */
#define DC_MOTION_MAX_SHIFT 16
int dc_motion_ssd(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, long* scores,
                  dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_pick(const long* scores, int tc, int S, int* shifts, long* best, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_apply(const void* frames, int tc, const int* shifts, int H, int W, int fill, void* out, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */

/* ---- piecewise-rigid motion correction: one whole-pixel shift per block of the frame, blended into a shift field ----------------
 * A two-photon frame is scanned line by line while the tissue moves, so its top is displaced differently from its bottom.  The
 * frame is cut into By x Bx blocks; every block gets the frame's rigid shift plus a residual within +-D, D <= DC_MOTION_MAX_DEV,
 * and the block shifts are blended bilinearly into one whole-pixel shift per pixel.  Integers only, the sign convention above.
 * M = S + D; By, Bx in [1, DC_MOTION_MAX_BLOCKS].
 * BLOCK GEOMETRY (a function of H, W, By, Bx alone, so an int32[tc][By][Bx][2] array of shifts is self-describing): block i covers
 *   rows [e(i), e(i+1)), e(i) = floor(i * H / By); columns likewise from W and Bx.  For scoring a block is clipped to the interior
 *   [M, H-M) x [M, W-M) and every clipped block must keep a pixel on both axes: H > 2M, e(1) > M and e(By-1) < H - M (else DC_EINVAL).
 *   dc_motion_block_ssd: bscores = int64[tc][By][Bx][2D+1][2D+1], fully written (never pre-clear):
 *     bscores[t][i][j][ey+D][ex+D] = sum over the clipped block (i, j) of (tmpl[y][x] - frame[y + dy + ey][x + dx + ex])^2,
 *     (dy, dx) = rigid[t] (int32[tc][2], e.g. what dc_motion_pick wrote) read on the device and CLAMPED there to [-S, S] per
 *     component: no value in that table makes the kernel read outside the frame.  Every candidate of a block sums the same
 *     pixels, and summed over the blocks a candidate's scores are the rigid-style score over the margin-M interior at
 *     (dy + ey, dx + ex).  D = 0 is legal (one score per block).
 *   dc_motion_block_pick: block_shifts = int32[tc][By][Bx][2], best = int64[tc][By][Bx] (nullable).  The residual minimises
 *     (bscore, ey^2 + ex^2, ey, ex) lexicographically -- the order of dc_motion_pick, so a featureless block follows the rigid
 *     shift --; block_shifts[t][i][j] = clamp(rigid[t]) + residual.
 *   dc_motion_warp: out[t][y][x] = frames[t][y + fy][x + fx] inside the frame, `fill` elsewhere, with the SHIFT FIELD (fy, fx) of
 *     (y, x) computed per axis in doubled coordinates.  Centres C2(i) = e(i) + e(i+1) - 1 (strictly increasing; By <= H and Bx <= W
 *     are required, else DC_EINVAL).  For row y, p = 2y: if By == 1 or p <= C2(0): i0 = i1 = 0, w = 0; if p >= C2(By-1): i0 = i1 =
 *     By-1, w = 0; otherwise i0 is the largest i with C2(i) <= p, i1 = i0 + 1, w = floor(256 (p - C2(i0)) / (C2(i1) - C2(i0))) in
 *     [0, 256).  Columns give j0, j1, v the same way.  Per component, s the block shifts of the frame, in 64-bit arithmetic:
 *       num = (256-w) ((256-v) s[i0][j0] + v s[i0][j1]) + w ((256-v) s[i1][j0] + v s[i1][j1]),  field = floor((num + 32768) / 65536).
 *     Equal block shifts give exactly that shift everywhere (then this is dc_motion_apply), and the field never leaves
 *     [min s, max s]; any int32 block shift is legal, |fy| >= H gives an all-fill row.  A pure move of 16-bit values: where the
 *     field changes by one pixel a source pixel is repeated or skipped -- the price of whole-pixel exactness.  The ABI takes the
 *     geometry, not weight tables: no index read from memory addresses block_shifts.  out must not overlap frames (DC_EINVAL).
 * D > 8, By or Bx > 32, S > 16 or H * W > 2^30: DC_EUNSUP (-3). */
#define DC_MOTION_MAX_DEV 8
#define DC_MOTION_MAX_BLOCKS 32
int dc_motion_block_ssd(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, int D, int By, int Bx,
                        const int* rigid, long* bscores, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_block_pick(const long* bscores, const int* rigid, int tc, int By, int Bx, int S, int D, int* block_shifts, long* best,
                         dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_warp(const void* frames, int tc, const int* block_shifts, int By, int Bx, int H, int W, int fill, void* out,
                   dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */

/* ---- sub-pixel motion correction: the picks refined to 1/16 pixel, the frames interpolated bilinearly ---------------------------
 * FINE SHIFTS are int32 in units of 1 / DC_MOTION_SUB of a pixel, with the sign convention above: a fine shift (sy, sx) =
 * (16 dy, 16 dx) means exactly the whole-pixel shift (dy, dx).  Integers only (csrc/motion_math.h): every result is exact and the
 * chunking of a recording never changes a bit.
 * REFINEMENT of a picked entry of a score table, per axis: s0 the picked score, sm and sp its neighbours at -1 and +1 on that axis
 *   with the other axis held at the pick.  A pick on the table's border on that axis: q = 0.  Otherwise N = sm - sp,
 *   D = sm - 2 s0 + sp (>= 0, and |N| <= D, because s0 is the minimum); D == 0: q = 0; otherwise
 *   m = floor((16 |N| + D - 1) / (2 D)), q = sign(N) m -- the vertex of the parabola through the three scores in sixteenths, a tie
 *   at a half going to the pick.  q lies in [-8, 8]; a symmetric neighbourhood gives 0; sm == s0 < sp gives exactly -8; the mirror
 *   image of a table gives the mirrored q.  Exact for scores up to 2^62 - 1 (16 |N| is never formed).  fine = 16 * picked + q.
 *   dc_motion_refine: fine = int32[tc][2] from the dc_motion_ssd tables `scores` and the dc_motion_pick rows `shifts`.  A row
 *     outside [-S, S] (no pick writes one) gives q = 0 and reads nothing outside the table.
 *   dc_motion_block_refine: fine = int32[tc][By][Bx][2] from the dc_motion_block_ssd tables, the rigid rows and the
 *     dc_motion_block_pick rows `block_shifts`: the picked residual is block_shifts - clamp(rigid, S), refined within its own
 *     [2D+1][2D+1] table; fine = 16 * block_shifts + q.  A residual outside [-D, D] gives q = 0 and reads nothing outside the table.
 * SPLIT of a fine shift: iy = floor(sy / 16), fy = sy - 16 iy in [0, 16) for either sign; ix, fx likewise.
 * INTERPOLATION: the values are read as int16 or uint16 numbers (is_unsigned as for dc_motion_ssd); a_ij = frame[y + iy + i][x + ix + j]:
 *     out = floor(((16-fy) ((16-fx) a00 + fx a01) + fy ((16-fx) a10 + fx a11) + 128) / 256).
 *   The result lies between the smallest and the largest tap, so it fits the dtype.  A tap whose weight is zero is not used: row
 *   i = 1 only when fy > 0, column j = 1 only when fx > 0.  If any USED tap lies outside the frame the output is `fill`.
 *   dc_motion_apply_sub: out[t][y][x] = the interpolation at (sy, sx) = fine[t] (int32[tc][2], read on the device; any int32 is
 *     legal).  With fine shifts that are multiples of 16 this is dc_motion_apply bit for bit.
 *   dc_motion_warp_sub: the same with a fine shift per pixel: the SHIFT FIELD of dc_motion_warp computed from the fine block shifts
 *     (int32[tc][By][Bx][2]; that arithmetic is exact for any int32), split and interpolated per pixel.  Equal fine block shifts
 *     make it dc_motion_apply_sub.  With fine block shifts that are multiples of 16, the output equals that of
 *     dc_motion_warp on the block shifts / 16 at every pixel where the fine field is itself a multiple of 16 -- everywhere when
 *     the frame's block shifts are equal; between block centres whose shifts differ the fine field passes through the fractions
 *     that the whole-pixel field rounds away, which is the point of it.
 * Sizes, limits, alignment and the overlap rule are those of the whole-pixel counterparts (DC_EINVAL / DC_EUNSUP alike). */
#define DC_MOTION_SUB 16
int dc_motion_refine(const long* scores, const int* shifts, int tc, int S, int* fine, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_block_refine(const long* bscores, const int* rigid, const int* block_shifts, int tc, int By, int Bx, int S, int D, int* fine,
                           dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_apply_sub(const void* frames, int is_unsigned, int tc, const int* fine, int H, int W, int fill, void* out,
                        dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_warp_sub(const void* frames, int is_unsigned, int tc, const int* fine_block_shifts, int By, int Bx, int H, int W, int fill,
                       void* out, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */

/* ---- wide search: shifts beyond DC_MOTION_MAX_SHIFT by a two-level, coarse-to-fine search -------------------------------------
 * The exhaustive search costs (2S+1)^2 passes over the interior, so its radius is capped at 16.  The wide search finds a coarse
 * shift on frames and template binned c x c (the unchanged dc_motion_ssd + dc_motion_pick at radius Sc = ceil(S / c) <= 16), then
 * scores the full-resolution shifts within +-D, D = c, of c times that pick.  Integers only, the sign convention above.  It is
 * NOT the exhaustive argmin of radius S: it is that argmin whenever it lies within +-D of the clamped centre (below).
 * c in {2, 4, 8}; S in [D, DC_MOTION_MAX_WIDE_SHIFT]; D <= DC_MOTION_MAX_DEV; H > 2S and W > 2S.
 *   dc_motion_bin: out = [tc][Hc][Wc] of the frames' 16-bit type, Hc = floor(H / c), Wc = floor(W / c) (trailing rows and columns
 *     are dropped): out[t][Y][X] = floor((sum over i, j in [0, c) of frame[cY+i][cX+j] + c^2/2) / c^2), the mean rounded half up,
 *     the floor holding for negative sums.  The result lies between the cell's smallest and largest value.  Template and frames
 *     are binned by this one function.  c not 2, 4 or 8: DC_EUNSUP; Hc or Wc == 0, or out overlapping frames: DC_EINVAL.
 *   dc_motion_ssd_around: wscores = int64[tc][2D+1][2D+1], ey the slow axis (index ey + D), fully written (never pre-clear):
 *     wscores[t][ey+D][ex+D] = sum over y in [S, H-S), x in [S, W-S) of (tmpl[y][x] - frame[y+cy+ey][x+cx+ex])^2 with the CENTRE
 *     (cy, cx) = clamp(mult * rows[t], -(S-D), S-D) per component -- rows = int32[tc][2] (e.g. the coarse dc_motion_pick rows,
 *     mult = c), read on the device, the product formed in 64 bits and clamped there: any int32 row and mult are legal and
 *     nothing outside the frame is read.  These are the entries (cy+ey, cx+ex) of the dc_motion_ssd table of radius S: the same
 *     pixels, the same bound (< 2^62).  D = 0 is legal (one score per frame).
 *   dc_motion_pick_around: shifts = int32[tc][2], the TOTAL shift (dy, dx) = centre + (ey, ex) that minimises (wscore,
 *     dy^2 + dx^2, dy, dx) lexicographically -- the order of dc_motion_pick over total shifts, not residuals, so the result equals
 *     the exhaustive pick of radius S whenever that pick lies in the window.  best = int64[tc] (nullable: the picked score).
 *     fine = int32[tc][2] (nullable): 16 * shift + q, q the REFINEMENT above of the picked residual within the window table --
 *     q = 0 on an axis where the residual lies on the window's border (such a pick is not refined) or where the denominator is 0.
 * S > 128, D > 8 or H * W > 2^30: DC_EUNSUP (-3); S < D or no interior: DC_EINVAL.  tc == 0 launches nothing. */
#define DC_MOTION_MAX_WIDE_SHIFT 128
int dc_motion_bin(const void* frames, int is_unsigned, int tc, int H, int W, int c, void* out, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_ssd_around(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int S, int D, const int* rows,
                         int mult, long* wscores, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_motion_pick_around(const long* wscores, const int* rows, int mult, int tc, int S, int D, int* shifts, long* best, int* fine,
                          dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */

/* ---- bidirectional scan-phase correction: the odd lines of a resonant-scanned recording moved against the even ones ------------
 * A resonant scanner draws even lines left to right and odd lines right to left; a phase error between the two sweeps displaces
 * all odd lines horizontally against the even ones by a constant few pixels.  This is the step in front of registration: one
 * whole-pixel offset per recording, found by exhaustive search within +-P, 0 <= P <= DC_BIDI_MAX_OFFSET, and applied as a pure
 * move of 16-bit values.  Integers only: every result is exact and the chunking of a recording never changes a bit.  A sub-pixel
 * or per-frame offset is not built.  frames: as for dc_motion_ssd (int16 / uint16 by is_unsigned, [tc][H][W] contiguous).
 * SIGN CONVENTION, in the motion section's words: an offset p means out[y][x] = frame[y][x + p] for ODD y and out[y][x] =
 * frame[y][x] for even y.  Odd lines recorded as frame[y][x] = scene[y][x + b] are found as p = -b.
 *   dc_bidi_scores: scores = int64[tc][2P+1], index p + P, fully written (never pre-clear):
 *     scores[t][p+P] = sum over odd y in [1, H-1) and x in [P, W-P) of (2 f[y][x+p] - f[y-1][x] - f[y+1][x])^2 -- every candidate
 *     sums the same pixels and never reads outside the frame; the two even neighbours cancel a vertical gradient to first order.
 *     |e| <= 131070, so e^2 < 2^34 (formed in 64 bits), and with H * W <= 2^28 a score is below 2^61.  P = 0 is legal (one score
 *     per frame).  H < 3 or W <= 2P: DC_EINVAL; P > 16 or H * W > 2^28: DC_EUNSUP (-3).  tc == 0 launches nothing.
 *   THE PICK is the host's (the scores of the frames used are summed per offset first, in integers of any size): the offset
 *     minimises (total, p^2, p) -- 0 wins every tie it is part of, then the smaller |p|, then the negative one: the order of
 *     dc_motion_pick in one dimension.
 *   dc_bidi_apply: the move above; `fill` (as for dc_motion_apply) goes where x + p leaves the row, even rows are copied.  p is
 *     passed by value and any int32 is legal; |p| >= W gives all-fill odd rows; p = 0 is a copy.  out must not overlap frames
 *     (DC_EINVAL); H * W > 2^30: DC_EUNSUP. */
#define DC_BIDI_MAX_OFFSET 16
int dc_bidi_scores(const void* frames, int is_unsigned, int tc, int H, int W, int P, long* scores, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */
int dc_bidi_apply(const void* frames, int tc, int p, int H, int W, int fill, void* out, dc_stream_t stream);   /* tc <= DC_FRAMES_PER_CALL_MAX */

/* ---- UNet1D spike inference: traces in, spike probabilities out ------------------------------------------------------------
 * The reference's second model family, UNet1DSegmentation: the network unet1d (unet_1d_segmentation.py:49-148) as its predict()
 * runs it (unet_1d_segmentation.py:422-459), inference mode only (Dropout is the identity; BatchNormalization uses its moving
 * statistics, folded by dc_bn_fold with eps 1e-3).  Input: the (N,T) matrix of z-scored traces dc_roi_trace_finalize writes.
 * Activations are channels-last fp32 [N][T][C]; a tensor argument `p, ld` addresses channel c of sample t of trace n at
 * p[(n*T + t)*ld + c] (ld: a multiple of 4), so a producer writes its channel slice of a concat buffer: the skip tensors
 * are produced straight into channels [2C, 3C) of the buffer the decoder's conv_layer reads (ld = 3C), the pooling reads them from
 * there, and dc_upsample1d_2x_fwd fills channels [0, 2C).  Every kernel works inside one trace: nothing is read across a trace
 * boundary and a sample's arithmetic does not depend on N, so a trace's outputs are the same bits however the traces are batched.
 *   dc_conv1d_k5_fwd: conv_layer, Conv1D(nbf, 5, strides=1, padding='same') + BatchNormalization + relu (:81-84):
 *     y[n][t][:] = relu?(fmaf(sum_{tap,c} x[n][t+tap-2][c] w[tap][c][:], scale, shift)); samples outside [0,T) of the SAME trace are 0.
 *     x dense [N][T][Cin]; wp = dc_pack_weights(taps 5, K=Cin, Ncols=Cout, s_tap=Cin*Cout, s_k=Cout, s_n=1, flip 0) of the Keras
 *     (5,Cin,Cout) kernel; (scale, shift) from dc_bn_fold (the conv bias is folded in).  Cin % 4 == 0, Cout % 4 == 0, any T, N >= 1.
 *     Implicit GEMM on the fp32 matrix cores, fp32 accumulation in a fixed order (channel chunk of 16, then tap, then channel).
 *   dc_conv1d_k5_c1_fwd: the first conv_layer (:86-89), Cin == 1: x is the (N,T) trace matrix itself, w the plain (5,1,Cout) kernel
 *     (16-byte aligned, like scale / shift); the taps are an fmaf chain in tap order.
 *   dc_maxpool1d_2_fwd: MaxPooling1D(2, strides=2) (:93).  out dense [N][T/2][C], T/2 rounded down (an odd last sample is dropped;
 *     T == 1: the output is empty, nothing is launched, DC_OK).  Bit-exact.
 *   dc_upsample1d_2x_fwd: UpSampling1D() (:79).  in dense [N][T][C]; out[n][2t][:] = out[n][2t+1][:] = in[n][t][:].  Bit-exact.
 *   dc_spike_head_fwd: Conv1D(2, 1) -> MaxPooling1D(margin + 1, strides=1, padding='same') -> softmax -> x[:, :, -1] (:139-145), pool =
 *     margin + 1 in 1..64.  a dense [N][T][C], kh [C][2], bh [2], p float32 [N][T]:
 *       l[n][t][j] = bh[j] + sum_c a[n][t][c] kh[c][j];   m[n][t][j] = max l[n][max(0, t-(pool-1)/2) .. min(T-1, t+pool/2)][j]
 *       p[n][t] = 1 / (1 + exp(m0 - m1))
 *     (TensorFlow 'SAME': the smaller pad is on the left, and padding never wins the max; T < pool is fine.) */
int dc_conv1d_k5_fwd(const float* x, const float* wp, const float* scale, const float* shift, int relu, float* y, long y_ld,
                     int N, int T, int Cin, int Cout, dc_stream_t stream);
int dc_conv1d_k5_c1_fwd(const float* x, const float* w, const float* scale, const float* shift, int relu, float* y, long y_ld,
                        int N, int T, int Cout, dc_stream_t stream);
int dc_maxpool1d_2_fwd(const float* in, long in_ld, float* out, int N, int T, int C, dc_stream_t stream);
int dc_upsample1d_2x_fwd(const float* in, float* out, long out_ld, int N, int T, int C, dc_stream_t stream);
int dc_spike_head_fwd(const float* a, const float* kh, const float* bh, int pool, float* p, int N, int T, int C,
                      dc_stream_t stream);

/* ---- UNet1D training: the 1-D hot path of a train step ---------------------------------------------------------------------
 * unet1d (unet_1d_segmentation.py:49-148) as fit() trains it (:217-380) with the loss and metrics of utils/spikes.py:11-57.
 * A 1-D activation [N][T][C] is a [pixels][C] tensor with pixels = N*T, so BatchNorm / ReLU / Dropout (dc_bn_stats_finalize,
 * dc_bn_relu_drop_fwd, dc_bn_bwd_reduce / _finalize / _apply), dc_adam_step_flat and dc_reduce_partials above serve this network
 * as they are.  Conventions of the inference section: channels-last fp32, `p, ld` strided tensors, nothing read across a trace
 * boundary; sums are fp32 (or double) in a FIXED order without atomics, so a repeated call gives the same bits.
 *   training-mode forward of conv_layer (:81-84): z = conv + bias is dc_conv1d_k5_fwd / _c1_fwd with scale = 1 (a vector of ones),
 *     shift = bias, relu = 0 (fmaf(acc, 1, b) is exact); then
 *   dc_conv1d_stats: partial[blocks][C][2] = (sum z, sum z^2) per channel in double, blocks = dc_conv1d_stats_blocks(pixels, C) --
 *     the layout dc_bn_stats_finalize reads with parts = blocks, groups = 1.  z [pixels][C] with sample stride z_ld; C % 4 == 0,
 *     C <= 1024.
 *   data gradient of conv_layer: dx[n][t][ci] = sum_{tap,co} dz[n][t-tap+2][co] w[tap][ci][co] is dc_conv1d_k5_fwd on dz with
 *     wp = dc_pack_weights(w, taps 5, K=Cout, Ncols=Cin, s_tap=Cin*Cout, s_k=1, s_n=Cout, flip 1), scale = 1, shift = 0, relu = 0
 *     (y_ld lets it write dx in place).  The first layer (Cin == 1) needs none.
 *   dc_conv1d_k5_wgrad: dw[tap][ci][co] = sum_{n,t} x[n][t+tap-2][ci] dz[n][t][co], x zero outside [0,T) of the SAME trace.
 *     x dense [N][T][Cin], dz dense [N][T][Cout], dw the Keras (5,Cin,Cout) kernel gradient; Cin % 4 == 0, Cout % 4 == 0, any T, N >= 1.
 *     fp32 matrix cores; the contraction over N*T is split over dc_conv1d_k5_wgrad_blocks() workgroups into slabs of
 *     ws (float[dc_conv1d_k5_wgrad_ws_floats()], caller-owned, contents irrelevant) that dc_reduce_partials adds in a fixed order.
 *     The bias gradient is the dbias_partial of dc_bn_bwd_apply.
 *   dc_conv1d_k5_c1_wgrad: the first layer; x is the (N,T) trace matrix, dw the (5,1,Cout) kernel gradient, Cout <= 1024.
 *   dc_maxpool1d_2_bwd: dx[n][2t+i][c] = (i == argmax ? dy[n][t][c] : 0) + (skip ? skip[n][2t+i][c] : 0).  dy dense [N][T/2][C];
 *     `in, in_ld` the stored forward INPUT of the pooling, from which the argmax is recomputed (the first of two equal values wins);
 *     `skip, skip_ld` (nullable) the gradient arriving over the skip connection, i.e. the [2C,3C) slice of the decoder conv's dx;
 *     dx [N][T][C] with sample stride dx_ld.  An odd last sample gets only its skip gradient.  Values are moved and added once: exact.
 *   dc_upsample1d_2x_drop_fwd / _bwd: UpSampling1D() + Dropout (:114-115).  out[n][2t+i][c] = in[n][t][c] * f[n][2t+i][c], and
 *     din[n][t][c] = dout[n][2t][c] f[n][2t][c] + dout[n][2t+1][c] f[n][2t+1][c], with f = mask / keep.  Dropout as in
 *     dc_bn_relu_drop_fwd: keep >= 1 -> none (the forward is then dc_upsample1d_2x_fwd bit for bit); mask != NULL -> explicit uint8
 *     {0,1} [N][2T][C] (4-byte aligned); else the counter RNG(seed) on the element index of the dense up-sampled tensor.
 *   dc_spike_head_train_fwd: dc_spike_head_fwd (the same p, bit for bit) plus, against labels y (uint8 [N][T]),
 *     partial[blocks][8] = {sum l, sum round(p) y, sum round(p), sum clip(y - round(p), 0, 1), sum y, 0, 0, 0},
 *     l = -(wpos y log(p + 1e-7) + wneg (1 - y) log(1 - p + 1e-7)), round half to even; blocks = dc_spike_head_train_fwd_blocks(N, T);
 *     reduce with dc_reduce_partials_f64(partial, blocks, 8, sums).  The reported loss is sums[0] / (N T).  1 - p is formed as
 *     1 / (1 + exp(m1 - m0)), so it keeps its digits where p rounds to 1.
 *   dc_spike_head_train_bwd: gradient of that mean loss.  dm1[t] = dl/dp p (1 - p) / (N T), dm0 = -dm1; dm_j[t] goes to the FIRST
 *     maximal logit of t's 'SAME' window (gathered in ascending t); da[n][s][c] = sum_j dl_j[s] kh[c][j] (dense [N][T][C]);
 *     grad_partial[blocks][2C+2] = the blocks' shares of (dkh[c][j] ..., dbh[0], dbh[1]), blocks = dc_spike_head_train_bwd_blocks(N, T):
 *     dc_reduce_partials(grad_partial, blocks, 2C+2, 1, out, tmp) yields the head's kernel and bias gradients back to back. */
int dc_conv1d_stats_blocks(long pixels, int C);
int dc_conv1d_stats(const float* z, long z_ld, double* partial, long pixels, int C, dc_stream_t stream);
long dc_conv1d_k5_wgrad_ws_floats(int N, int T, int Cin, int Cout);
int dc_conv1d_k5_wgrad_blocks(int N, int T, int Cin, int Cout);
int dc_conv1d_k5_wgrad(const float* x, const float* dz, float* dw, float* ws, int N, int T, int Cin, int Cout,
                       dc_stream_t stream);
long dc_conv1d_k5_c1_wgrad_ws_floats(int N, int T, int Cout);
int dc_conv1d_k5_c1_wgrad(const float* x, const float* dz, float* dw, float* ws, int N, int T, int Cout, dc_stream_t stream);
int dc_maxpool1d_2_bwd(const float* dy, const float* in, long in_ld, const float* skip, long skip_ld, float* dx, long dx_ld,
                       int N, int T, int C, dc_stream_t stream);
int dc_upsample1d_2x_drop_fwd(const float* in, float* out, long out_ld, const uint8_t* mask, float keep, uint64_t seed,
                              int N, int T, int C, dc_stream_t stream);
int dc_upsample1d_2x_drop_bwd(const float* dout, long dout_ld, const uint8_t* mask, float keep, uint64_t seed, float* din,
                              int N, int T, int C, dc_stream_t stream);
int dc_spike_head_train_fwd_blocks(int N, int T);
int dc_spike_head_train_bwd_blocks(int N, int T);
int dc_spike_head_train_fwd(const float* a, const float* kh, const float* bh, int pool, const uint8_t* y, float wpos, float wneg,
                            float* p, float* partial, int N, int T, int C, dc_stream_t stream);
int dc_spike_head_train_bwd(const float* a, const float* kh, const float* bh, int pool, const uint8_t* y, float wpos, float wneg,
                            float* da, float* grad_partial, int N, int T, int C, dc_stream_t stream);

/* misc */
int dc_fill(float* p, long n, float value, dc_stream_t stream);
/* p[i] *= s: the 1/G of the BatchNorm moving-statistics average over G data-parallel ranks (moving stats are
 * "averaged ... at checkpoint"; the sum itself is the RCCL all-reduce) */
int dc_scale_flat(float* p, long n, float s, dc_stream_t stream);
/* timing helper: run `fn`-independent HIP event timing is done by the caller via hipEvent* through ctypes:
 * these wrap hipEventCreate/Record/Synchronize/ElapsedTime on the given stream (so bench.py measures on the
 * stream the kernels are launched on). */
int dc_event_create(void** ev);
/* measurement hook (bench.py's per-kernel timer): the NEXT conv3x3 weight-gradient / joint-backward entry point called from THIS host
 * thread records ev_before right in front of its matrix kernel and ev_after right behind it, on the launch stream -- i.e. without
 * the slab-reduction launches that follow inside the same entry point (what rocprofv3 reports for that kernel symbol).  One shot. */
int dc_bracket_next_launch(void* ev_before, void* ev_after);
/* the kernel symbol (as rocprofv3 prints it, template arguments included) a conv3x3 weight-gradient launch of this shape runs:
 * dzin != 0 for dc_conv3x3_wgrad_dzin_f16x3, else dc_conv3x3_wgrad_f16x3 / _bnin.  Routing only, no launch. */
const char* dc_conv3x3_wgrad_kernel_name(int N, int H, int W, int Cin, int Cout, int dzin);
/* an event for stream ordering on ONE device only (hipEventDisableTiming | hipEventDisableSystemFence): what the engine's two-stream
 * backward hands between its streams.  Not for host synchronisation (no system-scope fence at the marker). */
int dc_event_create_sync(void** ev);
/* the same WITH the marker's system-scope fence (hipEventDisableTiming only): for the hand-offs whose consumer is not a queue of
 * this device -- the events in front of and behind a collective (a peer GPU reads / writes the buffer over xGMI). */
int dc_event_create_fenced(void** ev);
/* hipStreamWaitEvent(stream, ev): work queued on `stream` after this call waits for the work `ev` was last recorded behind */
int dc_stream_wait_event(dc_stream_t stream, void* ev);
int dc_event_record(void* ev, dc_stream_t stream);
int dc_event_elapsed_ms(void* start, void* stop, float* ms);
int dc_event_destroy(void* ev);

/* ---- collectives: the data-parallel gradient exchange (SURVEY 8b "call librccl.so ... directly via ctypes or a 3-function
 * dc_comm_* wrapper", 8e: one ncclAllReduce(sum, fp32) over the flat gradient buffer, optionally in buckets) ---------------
 * No reference counterpart: the reference trains on ONE device (README.md:23 pins CUDA_VISIBLE_DEVICES="0"; its step is the
 * model.fit_generator -> train_on_batch of unet_2d_summary.py:429-430); what is exchanged here is that step's flat gradient.
 * RCCL (librccl.so.1) is resolved with dlopen at the first dc_comm_* call -- the copy the process already holds (PyTorch-ROCm's)
 * when there is one; every other entry point works without it (DC_EUNSUP + message from these when it cannot be loaded).
 *   dc_comm_unique_id: HOST buffer of DC_COMM_ID_BYTES, filled by ONE rank and handed to the others out of band (the binding
 *     sends it through the torch.distributed store that rendezvoused the ranks);
 *   dc_comm_init_rank: collective over the nranks callers (one per GPU; binds the caller's current device), returns the handle;
 *   dc_comm_all_reduce_sum (fp32: the flat gradient) / _f64 (the step's loss / metric sums): buf[0..n) <- sum over ranks, in place,
 *     asynchronous on `stream` (a launch like any other: it can be recorded on a tape -- the backward of a data-parallel step
 *     replays as ONE tape, collectives included);
 *   dc_comm_group_start / _end: ncclGroupStart / ncclGroupEnd around several of them.
 * The caller orders the buffer's producers in front of the call with events made by dc_event_create_fenced. */
#define DC_COMM_ID_BYTES 128
int dc_comm_unique_id(void* id_host);
int dc_comm_init_rank(void** comm, const void* id_host, int nranks, int rank);
int dc_comm_all_reduce_sum(void* comm, float* buf, long n, dc_stream_t stream);
int dc_comm_all_reduce_sum_f64(void* comm, double* buf, long n, dc_stream_t stream);
int dc_comm_group_start(void);
int dc_comm_group_end(void);
int dc_comm_destroy(void* comm);

/* ---- launch tape: a step's enqueue sequence, recorded once, replayed from C --------------------------------------------
 * The reference's train loop calls train_on_batch once per step (model.fit_generator, unet_2d_summary.py:429-430); here a
 * step is ~230 asynchronous launches whose sequence is FIXED once the engine is warm -- same entry points, pointers and
 * shapes; only a few scalars (dropout seeds, Adam's lr_t, the batch pointers) change.  A tape holds such a sequence as
 * (entry point name, arguments) and replays it with ONE call: every operation goes through its entry point unchanged
 * (argument checks, status codes); `dc_tape_patch` marks the arguments that take a per-replay value.  HOST memory only; the
 * tape retains the recorded pointer VALUES (the caller keeps those buffers alive and in place, as for any launch).
 *   dc_tape_append: fn = the name of an int-returning launch entry point of this header (not: size / routing queries,
 *     dc_crop_augment and dc_host_* [host data read at call time], the event create / elapsed / destroy helpers);
 *     args8 = its arguments as 8-byte slots in declaration order: integers and pointers as longs, float / double
 *     arguments as the bit pattern of a double.
 *   dc_tape_patch(op, arg, slot): argument `arg` of operation `op` is values[slot] at replay (call in operation order).
 *   dc_tape_replay(first, count, values, nvalues): operations [first, first + count); stops at the first failing one. */
int dc_tape_create(void** tape);
int dc_tape_destroy(void* tape);
int dc_tape_append(void* tape, const char* fn, const long* args8, int nargs);
int dc_tape_patch(void* tape, int op, int arg, int slot);
int dc_tape_replay(void* tape, int first, int count, const long* values, int nvalues);
int dc_tape_len(void* tape);

#ifdef __cplusplus
}
#endif
#endif
