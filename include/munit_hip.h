/*
 * munit_hip.h -- C ABI of libmunit_hip.so: the gfx950 (MI355X / CDNA4) kernels behind the
 * MUNIT AdaINGen / AdaINGen_double + MsImageDis training step.
 *
 * The reference (cc-ai/MUNIT) is pure Python on PyTorch and has no FFI of its own
 * (SURVEY.md section 0.1); every entry point below therefore replaces a *stock torch op
 * call site* of the reference hot path, cited as scripts/<file>:<line>.  The Python side
 * (munit_amd/ops.py) binds these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - All tensor pointers are DEVICE pointers.  Parameters, their gradients, statistics and loss scalars are float32;
 *     activations are float32 or -- in the bf16-storage mode, see MUNIT_DTYPE_* -- bfloat16, and then travel as void*.
 *     Activations are NHWC ([B][H][W][C], C contiguous) -- the memory image of a torch channels_last tensor.
 *     Convolution weights are [Cout][KH][KW][Cin] -- the memory image of a torch OIHW
 *     tensor in channels_last format, so state_dict shapes stay (O, I, KH, KW).
 *   - Every call is asynchronous on `stream` (a hipStream_t passed as void*); the library
 *     never synchronises, allocates no device memory and keeps no state between calls
 *     (munit_stream_wait_stream caches one HIP event per host thread and device).
 *     The caller owns every buffer, including the workspace `ws` (size from the matching
 *     *_workspace_bytes query; must be 256-byte aligned).
 *   - Return value: 0 on success, negative on error; munit_last_error() returns a
 *     thread-local description of the last failure.
 */
#ifndef MUNIT_HIP_H
#define MUNIT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* munit_stream_t; /* hipStream_t */

enum { MUNIT_OK = 0, MUNIT_ERR_ARG = -1, MUNIT_ERR_WORKSPACE = -2, MUNIT_ERR_LAUNCH = -3 };
enum { MUNIT_ACT_NONE = 0, MUNIT_ACT_RELU = 1, MUNIT_ACT_LRELU = 2, MUNIT_ACT_TANH = 3 };
enum { MUNIT_PAD_ZERO = 0, MUNIT_PAD_REFLECT = 1 };
/* MUNIT_COMPUTE_F32: exact fp32 MFMA (the reference's arithmetic).  MUNIT_COMPUTE_BF16: operands rounded to
 * bf16 (nearest-even) as they are staged into LDS, v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- the
 * bf16 mode of BASELINE.json config #3, a build extension with no reference counterpart.  Layers whose
 * channel count is not a multiple of 32 (the 3-channel image layers) stay fp32 in both modes.
 * MUNIT_COMPUTE_F32X3: fp32 accuracy on the bf16 matrix pipe -- each fp32 operand is split exactly into three
 * bf16 values (a = a0 + a1 + a2) and the six products a_i*b_j with i + j <= 2 are accumulated in fp32; the
 * dropped terms are <= 2^-24 |a||b|, below the rounding of an fp32 FMA chain.  Opt-in. */
enum { MUNIT_COMPUTE_F32 = 0, MUNIT_COMPUTE_BF16 = 1, MUNIT_COMPUTE_F32X3 = 2 };
/* Element type of an ACTIVATION tensor in HBM (BASELINE.json config #3: bf16 storage).  Parameters, biases, AdaIN
 * parameters, norm statistics, accumulators, gradients of parameters and loss scalars are always fp32.  A bf16 tensor
 * needs a channel count that is a multiple of 64 in the convolutions (one 128-byte tile row) and of 4 elsewhere;
 * 3-channel images and 1x1-spatial vectors stay fp32.  Pointers of such tensors travel as void*. */
enum { MUNIT_DTYPE_F32 = 0, MUNIT_DTYPE_BF16 = 1 };

int munit_version(void);
const char* munit_last_error(void);

/* Data-parallel exchange for hosts without a communicator of their own (no reference counterpart:
 * scripts/train.py:171-225 is single-process).  A thin layer over RCCL, resolved with dlopen at the first call (no link-time
 * dependency; inside a PyTorch process the already-loaded librccl is used).  Rank 0 calls munit_comm_unique_id and hands the
 * 128 bytes to every rank by its own means; every rank then calls munit_comm_init (collective), on the device it will use.
 * munit_comm_allreduce sums `count` floats in place over all ranks, asynchronously on `stream` (the flat gradient buffer of
 * an update; the caller scales by 1/world).  The Python host of this repository uses torch.distributed instead (the launch
 * contract of bench.py); these entry points are exercised by tests/test_gpu_dp.py at world size 1.
 * munit_shutdown releases what the library keeps between calls (the RCCL handle); it is refused with MUNIT_ERR_ARG while a
 * communicator made by munit_comm_init is still alive.  The first call from several host threads is serialised. */
typedef void* munit_comm_t;
int munit_comm_unique_id(void* id_out, size_t bytes);
int munit_comm_init(munit_comm_t* comm, int rank, int world, const void* unique_id);
int munit_comm_allreduce(munit_comm_t comm, float* buf, size_t count, munit_stream_t stream);
int munit_comm_destroy(munit_comm_t comm);
int munit_shutdown(void);

/* Stream plumbing (no reference counterpart: torch's autograd engine orders everything on one stream).  `waiter` waits
 * for all work enqueued so far on `signaler`; both streams belong to the current device.  Used to fork backward-weight
 * onto a side stream without creating torch Event / Stream objects per layer. */
int munit_stream_wait_stream(munit_stream_t waiter, munit_stream_t signaler);

/* ------------------------------------------------------------------------------------
 * Convolution.  Replaces nn.ReflectionPad2d/ZeroPad2d + nn.Conv2d (+ bias + activation)
 * of Conv2dBlock.forward (scripts/networks.py:695-701, pads :642-649, conv :691-693),
 * the bare nn.Conv2d heads (networks.py:68, :472), nn.Linear of LinearBlock
 * (networks.py:712, as a 1x1 convolution on a [B][1][1][K] image) and, with
 * upsample = 1, the nn.Upsample(scale_factor=2) + 5x5 conv pair of the decoder
 * (networks.py:532-546) without materialising the upsampled tensor.
 *   x: [B][H][W][Cin]   w: [Cout][KH][KW][Cin]   bias: [Cout] or NULL
 *   y: [B][Ho][Wo][Cout],  Ho = ((H << upsample) + 2*pad - KH) / stride + 1
 * act is applied after the bias (MUNIT_ACT_*; slope = LeakyReLU negative slope).
 * Implicit-GEMM on v_mfma_f32_16x16x4_f32 (exact fp32), LDS-staged NHWC tiles.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  int B, H, W, Cin;
  int Cout, KH, KW;
  int stride, pad, pad_mode; /* MUNIT_PAD_* */
  int upsample;              /* 0 or 1: nearest x2 of x before padding */
  int act;                   /* MUNIT_ACT_* fused after bias (fwd only) */
  float slope;
  int compute;               /* MUNIT_COMPUTE_*: arithmetic of the contraction */
  int in_dtype, out_dtype;   /* MUNIT_DTYPE_* of x (and dx) / of y (and dy).  A bf16 x runs the bf16-storage kernels:
                              * direct-to-LDS tiles of 64 channels, v_mfma_f32_16x16x32_bf16, bf16 weight image */
} munit_conv_desc;

int munit_conv2d_out_hw(const munit_conv_desc* d, int* Ho, int* Wo);

size_t munit_conv2d_fwd_workspace_bytes(const munit_conv_desc* d); /* 0 for most layers */
int munit_conv2d_fwd(const munit_conv_desc* d, const void* x, const float* w, const float* bias,
                     void* y, void* ws, size_t ws_bytes, munit_stream_t stream);

/* backward-data (autograd of the sites above): dx[B][H][W][Cin] from dy[B][Ho][Wo][Cout]
 * (dy is the gradient w.r.t. the PRE-activation output; use munit_act_bwd first when an
 * activation was fused).  Handles the adjoint of reflect padding (border fold-add) and of
 * the nearest upsample (2x2 sum).  If add != NULL, dx = result + add (same shape).
 * Rounding of a bf16 dx (in_dtype = bf16).  The LDS-patch and the direct (1x1) forms round the fp32 sum once.  The
 * strided, up-sampling and 3-output-channel layers ("... + fold_kernel<bf16_t>" in munit_conv2d_kernel_name; a direct
 * form given `add` as well) round TWICE, by design, to halve the traffic of the padded-domain buffer: the gradient
 * w.r.t. the padded (and up-sampled) input is stored as bf16, the fold sums n of those values in fp32 (n = 1 at an
 * interior pixel of a strided layer, 4 under the nearest x2, up to 4 x 9 = 36 at a mirrored corner of an up-sampling
 * layer), adds `add`, and rounds once more.  Worst case: n / 2 ulps of the largest folded value plus half an ulp of
 * the result (|error| <= n * 2^-8 * max|g| + ulp(dx) / 2); with n = 1 the second rounding is the identity.  The folded
 * gathers take no `add` with a bf16 dx (refused).  tests/test_gpu_exact.py pins both behaviours bit for bit. */
size_t munit_conv2d_dgrad_workspace_bytes(const munit_conv_desc* d);
int munit_conv2d_dgrad(const munit_conv_desc* d, const void* dy, const float* w, const void* add,
                       void* dx, void* ws, size_t ws_bytes, munit_stream_t stream);

/* backward-weight: dw = beta*dw + sum_m dy[m][co] * im2col(x)[m][kh][kw][ci], layout of w;
 * db = beta*db + sum_m dy[m][co] when db != NULL.  Deterministic split-K (slabs in ws). */
size_t munit_conv2d_wgrad_workspace_bytes(const munit_conv_desc* d);
int munit_conv2d_wgrad(const munit_conv_desc* d, const void* x, const void* dy, float* dw,
                       float* db, float beta, void* ws, size_t ws_bytes, munit_stream_t stream);

/* Prepared weight images.  Two passes multiply by a re-laid-out image of the layer's weights: backward-data
 * (flipped / transposed, one slice per stride phase: the autograd transpose of nn.Conv2d, networks.py:691-693) and the
 * sub-pixel forward of the nearest-x2 + 5x5 decoder convs (networks.py:532-546; four merged 3x3 phase kernels).
 * The fp32 3x3 / stride 1 / pad 1 layers with wide channel counts (the residual blocks, networks.py:603-624) and those
 * phase kernels run as Winograd F(2x2, 3x3) on the fp32 matrix pipe: their images are U = G g G^T (16 frequencies per
 * channel pair, laid out for the kernel's direct-to-LDS loads; _WINOGRAD_DGRAD: of the filter rotated by 180 degrees with
 * the channel roles swapped; _SUBPIXEL_WINOGRAD: of the four merged phase filters; _WINOGRAD_S2: of the four 2x2 parity
 * filters of a 4x4 / stride 2 layer, F(3x3, 2x2)).  Same results as the direct form to
 * fp32 rounding (the algorithm cuDNN uses for the reference's own fp32 3x3 convolutions).
 * Weights change only at optimizer.step() (scripts/trainer.py:252-268), so the caller may keep these images: query
 * the size (0 = the pass uses w as it is), fill a munit_prep_item on the host with munit_conv2d_prep_item, build
 * the image with munit_conv2d_prepare_weights (one layer) or munit_conv2d_prepare_weights_batch (a table of items
 * in DEVICE memory, one launch for every layer of an optimizer) and hand it to the *_prepared entry points.  With
 * wp == NULL those behave exactly like munit_conv2d_fwd / _dgrad (image rebuilt into the workspace per call). */
enum { MUNIT_PASS_FWD = 0, MUNIT_PASS_DGRAD = 1, MUNIT_PASS_WGRAD = 2 };
enum { MUNIT_PREP_NONE = 0, MUNIT_PREP_DGRAD = 1, MUNIT_PREP_SUBPIXEL = 2, MUNIT_PREP_CAST = 3,
       MUNIT_PREP_WINOGRAD = 4, MUNIT_PREP_WINOGRAD_DGRAD = 5, MUNIT_PREP_SUBPIXEL_WINOGRAD = 6,
       MUNIT_PREP_WINOGRAD_S2 = 7, MUNIT_PREP_WINOGRAD_S2_DGRAD = 8,
       MUNIT_PREP_SUBPIXEL_WINOGRAD_DGRAD = 9 /* [the _DGRAD image][Winograd image of the four rotated phase filters] */ };
typedef struct {
  const float* w; /* [Cout][KH][KW][Cin] */
  float* wp;      /* image, munit_conv2d_prepared_weight_bytes() bytes (bf16 elements when bf16 != 0) */
  int Cout, KH, KW, Cin;
  int kind;       /* MUNIT_PREP_*; _CAST = the weights as they are, rounded to bf16 (forward of a bf16-input layer) */
  int ps;         /* stride phases per axis (MUNIT_PREP_DGRAD) */
  int bf16;       /* image in bf16: the pass runs the bf16-storage kernels */
} munit_prep_item;
size_t munit_conv2d_prepared_weight_bytes(const munit_conv_desc* d, int pass);
int munit_conv2d_prep_item(const munit_conv_desc* d, int pass, const float* w, float* wp, munit_prep_item* out);
int munit_conv2d_prepare_weights(const munit_prep_item* item, munit_stream_t stream);
int munit_conv2d_prepare_weights_batch(const munit_prep_item* items_dev, int n, munit_stream_t stream);
int munit_conv2d_fwd_prepared(const munit_conv_desc* d, const void* x, const float* w, const void* wp,
                              const float* bias, void* y, void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_conv2d_dgrad_prepared(const munit_conv_desc* d, const void* dy, const float* w, const void* wp,
                                const void* add, void* dx, void* ws, size_t ws_bytes, munit_stream_t stream);

/* nn.Linear of LinearBlock (scripts/networks.py:712, 743-749) under its own name: y[B][N] = act(x[B][K] w[N][K]^T + bias),
 * i.e. the 1x1 convolution on a [B][1][1][K] image (same kernels).  bwd: dx (or NULL), dw = beta*dw + dy^T x and
 * db likewise (or NULL); dy is the gradient at the PRE-activation output (apply munit_act_bwd first). */
size_t munit_linear_workspace_bytes(int B, int K, int N);
int munit_linear_fwd(const float* x, const float* w, const float* bias, float* y, int B, int K, int N, int act,
                     float slope, void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_linear_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int B, int K,
                     int N, float beta, void* ws, size_t ws_bytes, munit_stream_t stream);

/* FLOPs (2 x multiply-accumulates over valid GEMM rows) the kernels ISSUE for one call of the pass, next to the
 * algorithmic 2*B*Ho*Wo*Cout*KH*KW*Cin of the torch op it replaces (nn.Conv2d / its autograd, networks.py:691-693):
 * the sub-pixel form of the up-sampling convs and the box-sum backward-data execute fewer, strided backward-data over
 * the padded domain and the 4-channel re-layout of the 3-channel image layers slightly more.  Measurement only
 * (bench.py: roofline.step_executed_tflop). */
double munit_conv2d_executed_flops(const munit_conv_desc* d, int pass);
/* Name, as rocprofv3 shows it, of the kernel (or kernel group) that carries `pass` of this layer: the dispatch of the three
 * entry points stated as text.  Measurement only (bench.py picks the dominant kernel of the step by measured time and names
 * it with this).  The name depends on the whole descriptor, d->compute, d->in_dtype and d->out_dtype included: the bf16-storage
 * tiles, the bf16 backward-weight kernels and the CT = 1 / CT = 2 variants on fp32 tensors each have a name of their own, asked
 * of the same host predicates the launches act on.  A descriptor the entry point would refuse at launch is named
 * "refused: <reason>"; one that fails munit_conv2d_out_hw "invalid".  Static storage; never NULL. */
const char* munit_conv2d_kernel_name(const munit_conv_desc* d, int pass);

/* dx = dy * act'(y) for the fused activations (y = post-activation output). n elements. */
int munit_act_bwd(int act, float slope, const float* y, const float* dy, float* dx, size_t n,
                  munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Instance norm / AdaIN.  Replaces nn.InstanceNorm2d(affine=False)
 * (scripts/networks.py:657) and AdaptiveInstanceNorm2d.forward = F.batch_norm on the
 * (1, B*C, H, W) view (networks.py:823-845): per-(b,c) mean and BIASED variance over HW,
 *   y = act( (x - mean) * rsqrt(var + eps) * weight[b][c] + bias[b][c] ) + residual
 * adain == NULL -> weight 1 / bias 0.  Otherwise weight[b][c] = adain[b*ad_ld + w_off + c],
 * bias[b][c] = adain[b*ad_ld + b_off + c] (the slicing of assign_adain_params,
 * networks.py:230-239, done by address).  relu: the activation act() as MUNIT_ACT_* -- 0 none, 1 ReLU,
 * 2 LeakyReLU(0.2), 3 tanh (networks.py:668-681 pairs any norm with any activation).  residual may be NULL
 * (ResBlock's `out += residual`, networks.py:620-624).
 * stats: [B][C][2] (mean, rstd) written for the backward.  C % 4 == 0, C <= 1024.
 * ------------------------------------------------------------------------------------ */
size_t munit_instnorm_workspace_bytes(int B, int HW, int C);
int munit_instnorm_fwd(const float* x, float* y, float* stats, int B, int HW, int C,
                       const float* adain, int ad_ld, int w_off, int b_off, const float* residual,
                       int relu, float eps, void* ws, size_t ws_bytes, munit_stream_t stream);
/* dx from dy (gradient w.r.t. y before the residual add; the residual's gradient is dy
 * itself).  d_adain (same addressing as adain) receives dweight/dbias when not NULL. */
int munit_instnorm_bwd(const float* x, const float* dy, const float* stats, float* dx, int B, int HW,
                       int C, const float* adain, float* d_adain, int ad_ld, int w_off, int b_off,
                       int relu, void* ws, size_t ws_bytes, munit_stream_t stream);

/* The kernels a forward or backward at (B, HW, C) of MUNIT_DTYPE_* tensors runs, asked of the host predicates the launches
 * act on: 0 = flat (statistics, fold, apply), 1 = channel-sliced (statistics, apply), 2 = one-pass forward (one kernel that
 * keeps the plane of a (sample, 16-channel group) in registers: fp32, C % 64 == 0, at most 16 splits of at most 256 pixels;
 * the backward of such a shape runs the channel-sliced kernels).  -1 for dimensions the entry points refuse.  All routes give
 * the same bits and leave the same split partials in the workspace. */
int munit_instnorm_route(int B, int HW, int C, int dtype);

/* bf16-storage forms (x, y, dy, dx, residual are bf16 tensors; statistics, AdaIN parameters and their gradients fp32) */
int munit_instnorm_fwd_bf16(const void* x, void* y, float* stats, int B, int HW, int C,
                            const float* adain, int ad_ld, int w_off, int b_off, const void* residual,
                            int relu, float eps, void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_instnorm_bwd_bf16(const void* x, const void* dy, const float* stats, void* dx, int B, int HW,
                            int C, const float* adain, float* d_adain, int ad_ld, int w_off, int b_off,
                            int relu, void* ws, size_t ws_bytes, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * MUNIT's custom LayerNorm (scripts/networks.py:851-878): per-sample mean and UNBIASED
 * std over C*H*W, y = act( (x - mean) / (std + eps) * gamma[c] + beta[c] ), act = MUNIT_ACT_* in `relu`.
 * stats: [B][2] (mean, std).  C % 4 == 0, C <= 1024.
 * ------------------------------------------------------------------------------------ */
size_t munit_layernorm_workspace_bytes(int B, int HW, int C);
int munit_layernorm_fwd(const float* x, float* y, float* stats, int B, int HW, int C,
                        const float* gamma, const float* beta, int relu, float eps, void* ws,
                        size_t ws_bytes, munit_stream_t stream);
/* dgamma/dbeta: = acc*old + new (acc 0 or 1). */
int munit_layernorm_bwd(const float* x, const float* dy, const float* stats, float* dx, int B, int HW,
                        int C, const float* gamma, const float* beta, float* dgamma, float* dbeta,
                        float acc, int relu, float eps, void* ws, size_t ws_bytes,
                        munit_stream_t stream);

/* bf16-storage forms (x, y, dy, dx bf16; gamma, beta and their gradients fp32) */
int munit_layernorm_fwd_bf16(const void* x, void* y, float* stats, int B, int HW, int C,
                             const float* gamma, const float* beta, int relu, float eps, void* ws,
                             size_t ws_bytes, munit_stream_t stream);
int munit_layernorm_bwd_bf16(const void* x, const void* dy, const float* stats, void* dx, int B, int HW,
                             int C, const float* gamma, const float* beta, float* dgamma, float* dbeta,
                             float acc, int relu, float eps, void* ws, size_t ws_bytes,
                             munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Pooling.  nn.AvgPool2d(3, stride=2, padding=1, count_include_pad=False)
 * (scripts/networks.py:32-34) and nn.AdaptiveAvgPool2d(1) (networks.py:471).
 * ------------------------------------------------------------------------------------ */
int munit_avgpool3s2_fwd(const float* x, float* y, int B, int H, int W, int C, munit_stream_t stream);
int munit_avgpool3s2_bwd(const float* dy, float* dx, int B, int H, int W, int C, munit_stream_t stream);
int munit_gap_fwd(const float* x, float* y, int B, int HW, int C, munit_stream_t stream);
int munit_gap_bwd(const float* dy, float* dx, int B, int HW, int C, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Losses.  torch.mean(torch.abs(a - b)) (scripts/trainer.py:290), the masked form
 * torch.mean(torch.abs((a - b) * (1 - mask))) (trainer.py:305; mask is [B][H][W], one value
 * per pixel, broadcast over C) and LSGAN torch.mean((x - target)**2) (networks.py:91,109).
 * out: one device float (written, deterministic two-stage reduction, partials in ws).
 * Backward: gout is a DEVICE scalar (upstream gradient, already times the loss weight).
 * ------------------------------------------------------------------------------------ */
size_t munit_loss_workspace_bytes(size_t n);
int munit_l1_mean_fwd(const float* a, const float* b, const float* mask, size_t npix, int C, float* out,
                      void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_l1_mean_bwd(const float* a, const float* b, const float* mask, size_t npix, int C,
                      const float* gout, float* da, float* db, munit_stream_t stream);
/* recon_criterion on bf16 tensors (the content codes of the bf16-storage mode, trainer.py:470-471): a, b, da, db bf16 */
int munit_l1_mean_fwd_bf16(const void* a, const void* b, const float* mask, size_t npix, int C, float* out,
                           void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_l1_mean_bwd_bf16(const void* a, const void* b, const float* mask, size_t npix, int C,
                           const float* gout, void* da, void* db, munit_stream_t stream);
/* Synthetic-pair reconstruction loss (trainer.py:452-464): x_a, x_b, x_ab, x_ba NHWC fp32, npix pixels of C channels
 * (C in 1..4).  A pixel is aligned when sum_c |x_a - x_b| == 0 (formed on the fly; no mask tensor exists).
 * out = sum over aligned pixels of sum_c (|x_ab - x_b| + |x_ba - x_a|) / (npix * C): the sum of the reference's two
 * recon_criterion_mask(., ., 1 - mask_alignment) means.  ws: munit_loss_workspace_bytes.  bwd writes dx_ab and dx_ba (either
 * may be NULL) = gout[0] / (npix * C) * aligned * sign(.), sign(0) = 0; x_a and x_b get no gradient. */
int munit_pair_l1_fwd(const float* x_a, const float* x_b, const float* x_ab, const float* x_ba, size_t npix, int C,
                      float* out, void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_pair_l1_bwd(const float* x_a, const float* x_b, const float* x_ab, const float* x_ba, size_t npix, int C,
                      const float* gout, float* dx_ab, float* dx_ba, munit_stream_t stream);
int munit_mse_const_fwd(const float* x, float target, size_t n, float* out, void* ws, size_t ws_bytes,
                        munit_stream_t stream);
int munit_mse_const_bwd(const float* x, float target, size_t n, const float* gout, float* dx,
                        munit_stream_t stream);
/* Multi-scale LSGAN loss in one launch pair (networks.py:117-162): nseg segments (1..8) of n[s] > 0 floats at x[s], each
 * with its own target; x, n, target (and dx) are HOST arrays, handed to the kernels by value.  A segment may start at any
 * 4-byte boundary (the second half of a batched output).  out[0] = sum_s mean((x_s - target_s)^2), the mean scaled in
 * double and the segments added in index order; seg_out (nullable, nseg floats) gets each segment's mean.  No atomics:
 * two calls on the same data are bitwise equal.  ws: munit_lsgan_workspace_bytes(nseg).  bwd writes every dx[s] in full:
 * dx_s[i] = 2 * gout[0] / n_s * (x_s[i] - target_s).  Bad arguments return MUNIT_ERR_ARG before any launch. */
size_t munit_lsgan_workspace_bytes(int nseg);
int munit_lsgan_fwd(const float* const* x, const size_t* n, const float* target, int nseg, float* out, float* seg_out,
                    void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_lsgan_bwd(const float* const* x, const size_t* n, const float* target, int nseg, const float* gout,
                    float* const* dx, munit_stream_t stream);
/* Multi-scale non-saturating GAN loss (dis.gan_type nsgan, networks.py:79-139), the sibling of the LSGAN pair above with the
 * same arguments and the same contract (segments, host arrays by value, any 4-byte start, double-scaled means added in index
 * order, nullable seg_out, no atomics, bitwise repeatable, bwd writes every dx[s] in full).  target[s] must be exactly 0 or 1
 * (anything else: MUNIT_ERR_ARG before any launch).  With z = x for target 0 and z = -x for target 1,
 *   out[0] = sum_s mean(softplus(z_s)),  softplus(z) = max(z, 0) + log1p(exp(-|z|)),
 *   dx_s[i] = gout[0] / n_s * (1 - 2 target_s) * sigmoid(z),  sigmoid(z) = 1 / (1 + exp(-z)) for z >= 0, exp(z) / (1 + exp(z)) else
 * -- the quantity the reference's mean(binary_cross_entropy(sigmoid(x), target)) evaluates.  Where the reference's fp32
 * `sigmoid` saturates (logits beyond about 16.6), the reference returns 100 per element and a zero gradient; the build
 * returns the true value |z| and the true gradient.  Infinite logits give +inf / 0 loss elements and gout / n_s / 0 gradients,
 * a NaN logit a NaN loss and a NaN in that one dx element.  ws: munit_nsgan_workspace_bytes(nseg). */
size_t munit_nsgan_workspace_bytes(int nseg);
int munit_nsgan_fwd(const float* const* x, const size_t* n, const float* target, int nseg, float* out, float* seg_out,
                    void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_nsgan_bwd(const float* const* x, const size_t* n, const float* target, int nseg, const float* gout,
                    float* const* dx, munit_stream_t stream);
/* ------------------------------------------------------------------------------------
 * Spectral normalisation (dis.norm: sn; SpectralNorm, scripts/networks.py:885-942).  A normalised convolution runs as the
 * ordinary convolution with weight_bar (no bias, no activation) followed by the scale-bias-activation below:
 * conv(x, W / sigma) = conv(x, W) / sigma, so no weight image depends on sigma and sigma never reaches the host.
 *
 * Power iteration over ALL normalised layers of a module in one call (four launches, no grid synchronisation): items_dev is a
 * DEVICE array of n descriptors.  Per layer, with W = weight_bar viewed (O, I * KH * KW):
 *   v <- l2n(W^T u),  u <- l2n(W v),  sigma = u . (W v),   l2n(a) = a / (|a| + 1e-12);
 * sigma[2 * slot] = sigma and sigma[2 * slot + 1] = 1 / sigma.  w is read in place in its [O][KH][KW][I] memory order; v is
 * kept in the reference's column order (i, kh, kw), so state dicts interchange.  max_O / max_N: the largest O and I * KH * KW of
 * the table (they size the grid and the workspace; a layer beyond them is left untouched); max_N <= 8192.  fp32 with fp32
 * accumulation, every sum in a fixed order: two calls on the same state are bitwise equal. */
typedef struct munit_sn_item {
  const float* w; /* weight_bar */
  float* u;       /* O */
  float* v;       /* I * KH * KW */
  int O, KH, KW, I;
  int slot;
} munit_sn_item;
size_t munit_sn_power_iter_workspace_bytes(int n, int max_O, int max_N);
int munit_sn_power_iter(const munit_sn_item* items_dev, int n, int max_O, int max_N, float* sigma, void* ws, size_t ws_bytes,
                        munit_stream_t stream);
/* y = act(raw * *inv_sigma + bias[c]) over npix pixels of C channels (NHWC fp32); bias nullable.  inv_sigma: the layer's
 * device slot (sigma + 2 * slot + 1). */
int munit_sn_act_fwd(const float* raw, const float* inv_sigma, const float* bias, float* y, size_t npix, int C, int act,
                     float slope, munit_stream_t stream);
/* Backward of the above from dy and y: dz = dy * act'(y); draw = dz * *inv_sigma (what the convolution's backward receives,
 * so that its backward-weight yields G = wgrad(x, dZ / sigma)); db[c] = beta * db[c] + sum dz (beta 0 or 1; 0 never reads db);
 * coef[0] = sum dz * raw * inv_sigma^2 = <G, W> / sigma, the coefficient of the rank-1 correction below.  Two deterministic
 * stages through ws.  db and coef both NULL (the layer's parameters take no gradient): draw alone, one launch, raw and ws
 * unused. */
size_t munit_sn_act_bwd_workspace_bytes(size_t npix, int C);
int munit_sn_act_bwd(const float* dy, const float* y, const float* raw, const float* inv_sigma, float* draw, float* db,
                     float beta, float* coef, size_t npix, int C, int act, float slope, void* ws, size_t ws_bytes,
                     munit_stream_t stream);
/* dw = beta * dw - coef[0] * u (x) v in the weight's memory order ([O][KH][KW][I]; v in the reference's column order), beta 0
 * or 1: the sigma term of d weight_bar, taken with the u, v of the time of the call (the reference's `.data` swaps leave
 * autograd with the latest pair for every pass). */
int munit_sn_grad_fix(float* dw, const float* coef, const float* u, const float* v, int O, int KH, int KW, int I, float beta,
                      munit_stream_t stream);
/* out = sum_i w[i] * *(terms[i]); n <= 32; terms are device scalars, w host floats. */
int munit_weighted_sum(const float* const* terms, const float* w, int n, float* out,
                       munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Adam (torch.optim.Adam as configured at scripts/trainer.py:109-120: L2-coupled
 * weight_decay, amsgrad off) over one flat fp32 buffer of n elements.  step >= 1.
 * Hyper-parameters are doubles, as in torch: beta2 = 0.999 and 1 - beta2 = 0.001 are each rounded
 * to fp32 separately (computing 1 - (float)beta2 in fp32 is off by 1.3e-5 relative).
 * ------------------------------------------------------------------------------------ */
int munit_adam_step(float* p, const float* g, float* m, float* v, size_t n, double lr, double beta1,
                    double beta2, double eps, double weight_decay, int step, munit_stream_t stream);

/* ExtraAdam (scripts/extraadam.py:14-168; selected by `optimizer: extra...`, scripts/trainer.py:41-45,
 * stepped by the *_opt_step methods, trainer.py:252-268: extrapolation on even iterations, step on odd).
 * Every call advances the moments and forms u = -lr*sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps).
 * mode 0: p_saved = p, p += u (first extrapolation since the last step); mode 1: p += u;
 * mode 2: p = p_saved + u (the update step). */
int munit_extraadam_step(float* p, const float* g, float* m, float* v, float* p_saved, size_t n, double lr,
                         double beta1, double beta2, double eps, double weight_decay, int step, int mode,
                         munit_stream_t stream);

/* y[i] = alpha * x[i] (+ y[i] if accumulate); used for the 1/world gradient averaging. */
int munit_scale(const float* x, float* y, size_t n, float alpha, int accumulate, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Input pipeline.  Replaces the per-image torchvision/PIL chain of the
 * reference's loaders -- RandomHorizontalFlip -> Resize(new_size) -> RandomCrop -> ToTensor ->
 * Normalize(0.5, 0.5) (scripts/utils.py:229-249, 717-738; MyDataset.transform, utils.py:296-345) --
 * with one batched device pass over decoded uint8 images of different sizes.  The resize is Pillow's
 * BILINEAR resampler (anti-aliased, 22-bit fixed point, uint8 between the passes) restated bit-exactly.
 *   pool : device bytes holding the decoded images back to back (RGB, HWC interleaved; masks 1 byte/pixel)
 *   descs: device array of B descriptors (the random draws are made by the host loader)
 *   out  : images [B][out_h][out_w][3] fp32 in [-1, 1]; masks [B][out_h][out_w] fp32
 * ksize_max >= munit_image_ksize(src, rs) of every image axis in the batch (filter taps per output).
 * ------------------------------------------------------------------------------------ */
typedef struct {
  long long src_off;  /* byte offset of the image in pool */
  int src_h, src_w;   /* decoded size */
  int rs_h, rs_w;     /* size after Resize (= src size when no resize); unused by munit_mask_preprocess */
  int crop_i, crop_j; /* top-left corner of the crop window in the resized image */
  int flip;           /* 1: flipped left-right before the resize */
  int kind;           /* munit_label_preprocess only: 0 mask, 1 label map.  munit_image_preprocess and
                         munit_mask_preprocess ignore the field (it was `reserved`; the layout is unchanged) */
} munit_image_desc;

int munit_image_ksize(int src_size, int rs_size);
size_t munit_image_preprocess_workspace_bytes(int B, int out_h, int out_w, int ksize_max);
int munit_image_preprocess(const unsigned char* pool, const munit_image_desc* descs, int B, int out_h,
                           int out_w, int ksize_max, float* out, void* ws, size_t ws_bytes,
                           munit_stream_t stream);
/* Mask chain of MyDataset.transform (utils.py:318-330): flip, NEAREST resize of the whole mask to
 * (out_w, out_h), crop of that image at (crop_j, crop_i) with zero fill past its edge (what the reference
 * computes), ToTensor, and x255 for samples whose maximum is 1. */
size_t munit_mask_preprocess_workspace_bytes(int B, int out_h, int out_w);
int munit_mask_preprocess(const unsigned char* pool, const munit_image_desc* descs, int B, int out_h,
                          int out_w, float* out, void* ws, size_t ws_bytes, munit_stream_t stream);
/* Plane chain of MyDatasetSynthetic.transform (utils.py:495-543) for N single-band uint8 planes -- for a batch of B
 * synthetic samples N = 3B: the masks, the semantic_a maps, the semantic_b maps.  Unlike munit_mask_preprocess, each
 * plane is flipped, resized with Pillow's NEAREST to the descriptor's (rs_w, rs_h) -- the size of the resized image --
 * and cropped at (crop_i, crop_j); only the crop window is computed.  out: [N][out_h][out_w] fp32.
 *   kind 0 (mask): 1.0f where (vmax == 1 ? v == 1 : v >= 128), else 0.0f, vmax = the maximum of the plane's crop
 *     window: to_tensor (x255 when np.max of the cropped mask is 1) followed by > 0.5 -> 1, < 0.5 -> 0 (no byte gives
 *     exactly 0.5);
 *   kind 1 (label map): mapping() of utils.py:1356-1366 on the grey value -- 255 -> 8, 200 -> 7, 178 -> 6, 149 -> 5,
 *     133 -> 4, 76 -> 3, 55 -> 2, 29 -> 1, every other value unchanged -- as a float.
 * The descriptors are device memory and cannot be validated: a window position outside [0, rs) or a source index
 * outside [0, src) reads no pixel and counts as grey value 0; nothing is read outside a plane of the stated size.
 * The workspace holds the index tables and the per-plane maxima; there is no host synchronisation. */
size_t munit_label_preprocess_workspace_bytes(int N, int out_h, int out_w);
int munit_label_preprocess(const unsigned char* pool, const munit_image_desc* descs, int N, int out_h,
                           int out_w, float* out, void* ws, size_t ws_bytes, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Sample grids (scripts/utils.py:768-814, __write_images): torchvision's make_grid(nrow, padding=0, normalize=True)
 * followed by save_image's conversion to bytes, for a list of image batches, in two launches and without a host
 * synchronisation.  `src` is a HOST array of nsrc (1..16) descriptors, handed to the kernels by value; source s is n >= 1
 * fp32 images of H x W with 1 or 3 channels, planar or interleaved, starting at any 4-byte boundary.
 *   v   = (x + pre_add) * pre_mul                       (two fp32 roundings; 0, 1 is the identity)
 *   lo, hi = minimum, maximum of v over the sum-of-n images named (a one-channel image counts three times)
 *   d   = max(hi - lo, 1e-5), t = (v - lo) * (1 / d)    (hi - lo in double, rounded to fp32 once: python floats; the
 *                                                        reciprocal is what torch's device kernel for tensor / scalar takes)
 *   out = (uint8) clamp(t * 255 + 0.5, 0, 255), truncating; `* 255` and `+ 0.5` rounded separately
 * Tiling: nmaps = sum n images in list order, row-major, xmaps = min(nrow, nmaps) per row, ymaps = ceil(nmaps / xmaps)
 * rows; cells past nmaps are 0.  out: [ymaps * H][xmaps * W][3] bytes, every one written; at most 2^31 - 1 of them.
 * The workspace holds the per-block (min, max) partials of the range pass; the pack pass reduces them (no atomics: two
 * calls are bitwise equal).  A NaN input gives no defined picture; nothing outside the stated tensors is touched.
 * ------------------------------------------------------------------------------------ */
typedef struct {
  const float* data;  /* device pointer */
  int n;              /* images */
  int channels;       /* 1 or 3 */
  int layout;         /* 0 planar [n][C][H][W], 1 interleaved [n][H][W][C] */
} munit_grid_src;

size_t munit_image_grid_workspace_bytes(int nsrc, int H, int W, int nrow);
int munit_image_grid_u8(const munit_grid_src* src, int nsrc, int H, int W, int nrow, float pre_add, float pre_mul,
                        unsigned char* out, void* ws, size_t ws_bytes, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Semantic-consistency loss (scripts/trainer.py:706-771): the frozen Resnet34_8s segmentation network
 * (scripts/utils.py:933-983, scripts/resnet.py) and its head.  The convolutions run through munit_conv2d_* with
 * BatchNorm folded into their weights; the dilated 3x3 layers of layer3 / layer4 run undilated on the phase images
 * of munit_space_to_batch.  Images and activations are NHWC fp32.
 * ------------------------------------------------------------------------------------ */
/* seg_transform of (x + 1) / 2 (utils.py:159-174): y = ((x + 1) / 2 - mean_c) / std_c with the ImageNet statistics;
 * x, y: npix pixels of 3 channels.  bwd: dx = dy / std_c / 2. */
int munit_seg_input_fwd(const float* x, float* y, size_t npix, munit_stream_t stream);
int munit_seg_input_bwd(const float* dy, float* dx, size_t npix, munit_stream_t stream);
/* Space-to-batch by f (inverse 0): y[(n*f + py)*f + px][i][j][c] = x[n][i*f + py][j*f + px][c], x [N][H][W][C],
 * H % f == W % f == 0.  inverse 1: the way back -- x is then the phase-major [N*f*f][H/f][W/f][C] input and y the
 * [N][H][W][C] output (N, H, W always describe the plain layout).  A dilation-d 3x3 conv
 * with zero pad d is the undilated pad-1 conv on every phase image; applied twice with f = 2 it gives the d = 4 phases.
 * A permutation: each pass is the other's adjoint. */
int munit_space_to_batch(const float* x, float* y, int N, int H, int W, int C, int f, int inverse, munit_stream_t stream);
/* nn.MaxPool2d(3, stride=2, padding=1): y [B][Ho][Wo][C], Ho = (H - 1) / 2 + 1.  idx (one byte per output) receives the
 * window position kh*3 + kw of the winner: the FIRST maximal element in window order (kh-major), torch's tie rule.
 * bwd: dx[h][w] = sum of dy over the windows whose recorded winner is (h, w) (a gather; deterministic). */
int munit_maxpool3s2_fwd(const float* x, float* y, unsigned char* idx, int B, int H, int W, int C, munit_stream_t stream);
int munit_maxpool3s2_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int H, int W, int C,
                         munit_stream_t stream);
/* BasicBlock tail y = relu(a + r), n % 4 == 0 (backward: munit_act_bwd with MUNIT_ACT_RELU on y). */
int munit_add_relu_fwd(const float* a, const float* r, float* y, size_t n, munit_stream_t stream);
/* Head: logits [B][h][w][19] are up-sampled bilinearly (align_corners = False) to [B][h*S][w*S] on the fly.
 * labels [B][h*S][w*S] int32 in 0..18.  mask [B][h*S][w*S] (values 0 / 1) or NULL.  NULL: nn.CrossEntropyLoss over the
 * 19 classes.  Otherwise the masked form of trainer.py:746-769: logits (1 - m) * z with m appended as a 20th class,
 * target (1 - m) * label + 19 m.  out = (sum of the pixel losses) / norm (one device float; norm = pixels per mean, so
 * one call over a batch of two images per pair gives the sum of the two means).  bwd: dlogits [B][h][w][19] =
 * gout[0] / norm * adjoint of the up-sample of the pixel gradients (a gather; deterministic).  ws: _workspace_bytes. */
size_t munit_seg_ce_workspace_bytes(int B, int h, int w, int S);
int munit_seg_ce_fwd(const float* logits, const int* labels, const float* mask, int B, int h, int w, int S, float norm,
                     float* out, void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_seg_ce_bwd(const float* logits, const int* labels, const float* mask, int B, int h, int w, int S, float norm,
                     const float* gout, float* dlogits, void* ws, size_t ws_bytes, munit_stream_t stream);
/* The head against a ground-truth map of the simulator's 10 classes (trainer.py:732-737, merge_classes of
 * utils.py:1330-1353).  The 19 up-sampled logits are merged into 10: merged class 0 is the constant 0, 1 = {0, 1},
 * 2 = {2, 3, 4}, 3 = {5, 6, 7}, 4 = {8}, 5 = {9}, 6 = {10}, 7 = {11, 12}, 8 = {13, 17, 18}, 9 = {14, 15, 16} (sums of the
 * member logits).  gt [B][h*S][w*S] FLOAT32 as the loader delivers it, truncated toward zero like .type(torch.long);
 * valid values 0..9.  mask NULL: the 10-class cross-entropy; otherwise the masked form with new_class = 10 (logits
 * (1 - m) * merged, m appended as the 11th logit, target (1 - m) * gt + 10 m).  out, norm, ws and the refusals as
 * munit_seg_ce_*.  bwd: the pixel gradient of a merged class goes to each of its members (class 0's is dropped), then
 * through the same up-sample adjoint; deterministic.
 * A label outside 0..9, NaN or infinite is never used as an index: that pixel's loss is NaN (so `out` is NaN and the
 * step's loss_sem_seg shows it) and its gradient 0; both calls still return MUNIT_OK. */
int munit_seg_ce_gt_fwd(const float* logits, const float* gt, const float* mask, int B, int h, int w, int S, float norm,
                        float* out, void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_seg_ce_gt_bwd(const float* logits, const float* gt, const float* mask, int B, int h, int w, int S, float norm,
                        const float* gout, float* dlogits, void* ws, size_t ws_bytes, munit_stream_t stream);

/* The plain K-class head of the trainable segmentation head (adaptation.sem_seg_lambda, trainer.py:1303-1318): logits
 * [B][h][w][K], K in 2..32, up-sampled bilinearly by S in {1, 2, 4, 8} on the fly with the tap order of munit_seg_ce_*;
 * nn.CrossEntropyLoss over the K classes against gt [B][h*S][w*S] FLOAT32 truncated toward zero; no mask, no class merge.
 * out = (sum of the pixel losses) / norm.  bwd writes the pixel gradients to the workspace, then gathers them through
 * the up-sample's adjoint: dlogits [B][h][w][K]; deterministic.  A label outside 0..K-1, NaN or infinite is never used as
 * an index: that pixel's loss is NaN and its gradient 0; both calls still return MUNIT_OK.  Each pass refuses a
 * workspace short of its own need (fwd: one float per block, bwd: the gradient at the up-sampled resolution);
 * _workspace_bytes covers both. */
size_t munit_seg_ce_direct_workspace_bytes(int B, int h, int w, int S, int K);
int munit_seg_ce_direct_fwd(const float* logits, const float* gt, int B, int h, int w, int S, int K, float norm, float* out,
                            void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_seg_ce_direct_bwd(const float* logits, const float* gt, int B, int h, int w, int S, int K, float norm,
                            const float* gout, float* dlogits, void* ws, size_t ws_bytes, munit_stream_t stream);
/* nn.AvgPool2d(7, stride=1, padding=3) with the padding counted: y[b][i][j][c] = (sum of x over the 7x7 window clipped to
 * the map) / 49; x, y [B][H][W][C], C % 4 == 0, any H, W >= 1, x != y.  The operator is its own adjoint: bwd computes
 * dx from dy the same way.  Fixed summation order; deterministic. */
int munit_avgpool7_fwd(const float* x, float* y, int B, int H, int W, int C, munit_stream_t stream);
int munit_avgpool7_bwd(const float* dy, float* dx, int B, int H, int W, int C, munit_stream_t stream);
/* labels = argmax over the 19 up-sampled logits (first maximal class on ties: torch's max(1)[1]). */
int munit_seg_labels(const float* logits, int B, int h, int w, int S, int* labels, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Feature-level domain adaptation (adaptation.adv_lambda / dfeat_lambda): the kernels of domainClassifier
 * (scripts/utils.py:1277-1327, 1370-1392) that are not convolutions.  fp32, NHWC, C % 4 == 0.  Deterministic: reductions
 * run in a fixed order (per-block partials in ws, one finishing pass), no atomics.
 * ------------------------------------------------------------------------------------ */
/* nn.BatchNorm2d over x [R = B*H*W][C] (C <= 1024, C / 4 divides 256).  Training mode (eval 0; R >= 2):
 * y = act((x - mean) * rstd * gamma + beta) with the batch mean and the BIASED variance (two passes: the squares are taken
 * about the mean), rstd = 1 / sqrt(var + eps); mean [2][C] (the mean as a sum of two floats, high parts then low parts) and
 * rstd [C] are written for the backward; running_mean / running_var
 * move in place by `momentum`, running_var with the UNBIASED variance.  relu: 0 / 1.  eval 1: normalises with
 * running_mean / running_var and writes y alone (mean, rstd, ws may be NULL).  ws: munit_batchnorm_workspace_bytes(C). */
size_t munit_batchnorm_workspace_bytes(int C);
int munit_batchnorm_fwd(const float* x, float* y, float* mean, float* rstd, float* running_mean, float* running_var,
                        long long R, int C, const float* gamma, const float* beta, int relu, int eval, float eps,
                        float momentum, void* ws, size_t ws_bytes, munit_stream_t stream);
/* Backward of the training-mode forward.  y is read behind a ReLU only (relu 1; NULL otherwise).  dx is always written;
 * dgamma / dbeta = acc * old + new (acc 0 or 1) when not NULL, untouched when NULL. */
int munit_batchnorm_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* mean,
                        const float* rstd, float* dx, float* dgamma, float* dbeta, float acc, long long R, int C,
                        int relu, void* ws, size_t ws_bytes, munit_stream_t stream);
/* Batch norm whose statistics span W data-parallel ranks of R_local rows each (equal on all ranks; N = W * R_local >= 2,
 * refused by stats_local and the backward halves; W in 1..64): W ranks compute what one process computes on the joined batch.  Each pass has a
 * local half, which writes the rank's partial results into row `rank` of an exchange buffer xch of W rows and ZEROES the
 * other rows, and a finishing half, which expects xch summed over all ranks (one all-reduce(SUM) issued by the host between
 * the two; adding zeros is exact, so every rank then holds bitwise the same rows) and merges the rows in rank order, in
 * double.  xch_floats: the size of the buffer, at least W * 3 * C (forward) or W * 4 * C (backward).
 *   stats_local: row = the local mean as two floats [2][C] and M2 = sum (x - local mean)^2 [C].
 *   fwd_apply:   mean = sum mean_r / W, M2 = sum M2_r + R_local * sum (mean_r - mean)^2; writes mean [2][C], rstd [2][C] =
 *                1 / sqrt(M2 / N + eps) as two floats like the mean (high parts, then low parts), moves running_mean /
 *                running_var (unbiased M2 / (N - 1)) and writes y.
 *   bwd_local:   row = the local sum of g [C] and of g * xhat [C] (g = dy gated by y > 0 behind a ReLU), accumulated in
 *                double and written as two floats each: the high parts [2][C], then the low parts [2][C].  With few rows
 *                per channel (two ranks of batch 1 after the average pool) xhat^2 is close to 1 and dx below cancels to
 *                eps * rstd^2 of its terms, so a sum or an rstd rounded to fp32 would be wrong in dx's second digit.
 *   bwd_finish:  dx = gamma * rstd * (g - S_g / N - xhat * S_gx / N) in double with the totals over all ranks; dgamma / dbeta =
 *                acc * old + the LOCAL sums (row `rank`) when not NULL: the optimizer's gradient exchange averages them.
 * ws: munit_batchnorm_dp_workspace_bytes(C) for stats_local, bwd_local and bwd_finish. */
size_t munit_batchnorm_dp_workspace_bytes(int C);
int munit_batchnorm_dp_stats_local(const float* x, long long R_local, int C, int W, int rank, float* xch, size_t xch_floats,
                                   void* ws, size_t ws_bytes, munit_stream_t stream);
int munit_batchnorm_dp_fwd_apply(const float* x, float* y, float* mean, float* rstd, float* running_mean, float* running_var,
                                 long long R_local, int C, int W, const float* xch, size_t xch_floats, const float* gamma,
                                 const float* beta, int relu, float eps, float momentum, munit_stream_t stream);
int munit_batchnorm_dp_bwd_local(const float* x, const float* dy, const float* y, const float* mean, const float* rstd,
                                 long long R_local, int C, int relu, int W, int rank, float* xch, size_t xch_floats, void* ws,
                                 size_t ws_bytes, munit_stream_t stream);
int munit_batchnorm_dp_bwd_finish(const float* x, const float* dy, const float* y, const float* gamma, const float* mean,
                                  const float* rstd, float* dx, float* dgamma, float* dbeta, float acc, long long R_local,
                                  int C, int relu, int W, int rank, const float* xch, size_t xch_floats, void* ws,
                                  size_t ws_bytes, munit_stream_t stream);
/* nn.MaxPool2d(2): y [B][H/2][W/2][C] (floor: an odd trailing row / column is dropped; H, W >= 2).  idx (one byte per
 * output) receives the window position kh*2 + kw of the winner: the FIRST maximal element in window order, torch's tie
 * rule (a NaN counts as maximal).  bwd writes every dx element exactly once: dy at the winners, 0 at the losers and in the
 * dropped row / column. */
int munit_maxpool2_fwd(const float* x, float* y, unsigned char* idx, int B, int H, int W, int C, munit_stream_t stream);
int munit_maxpool2_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int H, int W, int C,
                       munit_stream_t stream);
/* nn.AvgPool2d((16, 16)) + squeeze on a map with 16 <= H, W <= 31: y [B][C] = mean of the top-left 16x16 window
 * (C / 4 divides 256).  bwd: dx = dy / 256 inside the window, 0 outside. */
int munit_avgpool16_fwd(const float* x, float* y, int B, int H, int W, int C, munit_stream_t stream);
int munit_avgpool16_bwd(const float* dy, float* dx, int B, int H, int W, int C, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * FID evaluation (scripts/inception_utils.py).  Everything is fp32, row-major and asynchronous
 * on `stream`; every argument check below returns MUNIT_ERR_ARG before any launch.
 *
 * Batched dense product on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32):
 *   C_p = alpha * op(A_p) * B_p + beta_eye * I   for the n <= MUNIT_GEMM_MAX problems of the host table `prob`,
 * all in ONE launch and of one shape: op(A) is [M][K] (A itself [M][K], or [K][M] with transA != 0), B [K][N], C [M][N],
 * any M, N, K >= 1, leading dimensions lda / ldb / ldc >= the row length (the padding is neither read nor written).  The
 * table is read during the call.  No C may overlap any A, B or other C of the launch.  Each output element is one k-ordered
 * fmaf chain from 0, then alpha * acc + (row == col ? beta_eye : 0): no split-K, no atomics, bitwise repeatable. */
enum { MUNIT_GEMM_MAX = 8 };
typedef struct munit_gemm_problem {
  const float* A;
  const float* B;
  float* C;
} munit_gemm_problem;
int munit_gemm_f32(const munit_gemm_problem* prob, int n, int M, int N, int K, int lda, int ldb, int ldc, int transA,
                   float alpha, float beta_eye, munit_stream_t stream);
/* torch_cov(pool, rowvar=False) with its mean (inception_utils.py:90-120, :285): mu[D] = column mean of pool[N][D], N >= 2,
 * sigma[D][D] = Xc^T Xc / (N - 1) with Xc = pool - mu held in ws (centred first, as the reference does).  Unlike the
 * reference, whose `m -= mean` writes through a view, pool is not modified. */
size_t munit_fid_moments_workspace_bytes(int N, int D);
int munit_fid_moments(const float* pool, int N, int D, float* mu, float* sigma, void* ws, size_t ws_bytes,
                      munit_stream_t stream);
/* sqrt_newton_schulz (inception_utils.py:125-140) on A[b][D][D] -> sA[b][D][D], iters >= 0, the recurrence unchanged:
 * normA = sqrt(sum(A o A)) per matrix, Y = A / normA, Z = I; iters times T = 1.5 I - 0.5 Z Y, Y <- Y T, Z <- T Z (the two
 * in one launch); sA = Y sqrt(normA).  No early exit, no clamp, no host synchronisation: the whole loop is enqueued by
 * this one call. */
size_t munit_sqrt_newton_schulz_workspace_bytes(int D, int b);
int munit_sqrt_newton_schulz(const float* A, int D, int iters, int b, float* sA, void* ws, size_t ws_bytes,
                             munit_stream_t stream);
/* torch_calculate_frechet_distance (inception_utils.py:205-241) with the iteration count as an argument:
 * out[0] = |mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr sqrt_newton_schulz(sigma1 sigma2, iters), a device scalar. */
size_t munit_frechet_distance_workspace_bytes(int D);
int munit_frechet_distance(const float* mu1, const float* sigma1, const float* mu2, const float* sigma2, int D, int iters,
                           float* out, void* ws, size_t ws_bytes, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Inception-v3 feature trunk of FID evaluation (scripts/inception_utils.py:27-85, WrapInception; DESIGN.md section 10.7;
 * csrc/inception.hip).  Inference only, fp32, NHWC, asynchronous on `stream`; every argument check returns MUNIT_ERR_ARG
 * before any launch: null pointers, x_ld / y_ld shorter than the slice, a stride other than 1 or 2, pads above
 * (K - 1) / 2, output extents below 1, y overlapping x.
 *
 * Rectangular convolution: y = relu?(conv(x, w) + bias), KH x KW filter (each 1..15), one pad per axis, zero padding.
 *   x: B x H x W pixels of Cin channels, pixel p at x + p * x_ld (x_ld >= Cin); y: B x Ho x Wo pixels of Cout channels,
 *   pixel p at y + p * y_ld (y_ld >= Cout), Ho = (H + 2 pad_h - KH) / stride + 1.  The per-pixel strides let a layer read a
 *   channel slice of a wider buffer and write into a channel slice of a concatenated output; the channels of a pixel
 *   outside the slices are neither read nor written.  x and y must lie in different buffers: the overlap check compares
 *   the whole byte spans from the first to the last word of each slice, so two disjoint channel slices interleaved in one
 *   buffer are refused as overlapping.
 *   wk: the weights as the k-major image [KH][KW][Cin][Cout] (row k = (kh * KW + kw) * Cin + ci holds the Cout values
 *   w[co][ci][kh][kw]), built once when the layer is loaded.  bias: Cout values.
 *   Arithmetic: implicit GEMM on v_mfma_f32_32x32x2_f32; every output is one k-ordered fmaf chain from 0, then + bias, then
 *   ReLU; no split-K, no atomics.  The chain depends neither on the tile shape nor on B: an image's output is bitwise the
 *   same in any batch.  tile: -1 lets the host choose (the answer of the tile query below: the 64 x 64 tile while 128 x 128
 *   tiles would number fewer than the current device's compute units (asked once per device; 256 where none answers), else the 128-row tile that pads Cout least), 0 the 128 x 128 tile,
 *   1 the 64 x 64 tile, 2 the 128 x 64 tile. */
typedef struct munit_rect_desc {
  int B, H, W, Cin, x_ld;
  int Cout, y_ld;
  int KH, KW, stride; /* stride 1 | 2 */
  int pad_h, pad_w;
  int relu;
} munit_rect_desc;
int munit_conv2d_rect_out_hw(const munit_rect_desc* d, int* Ho, int* Wo);
int munit_conv2d_rect_tile(const munit_rect_desc* d); /* 0 | 1 | 2, or MUNIT_ERR_ARG */
int munit_conv2d_rect_fwd(const munit_rect_desc* d, const float* x, const float* wk, const float* bias, float* y, int tile,
                          munit_stream_t stream);
/* The trunk's 3 x 3 pooling.  (Named `window`, not `pool`: the symbols matching munit_*pool* are the autograd pooling table of
 * munit_amd.ops, one forward and one backward each, and this forward-only kernel is not one of them.)
 * 3 x 3 window over B x H x W pixels of C channels with the same per-pixel strides (x and y in different buffers, as
 * above): MUNIT_WINDOW_MAX is F.max_pool2d(3, stride, pad) (padding never wins: negative inputs survive), MUNIT_WINDOW_AVG is
 * F.avg_pool2d(3, stride, pad) with count_include_pad = True: zero padding, the nine taps summed in window order (kh-major),
 * the divisor always 9.  stride 1 | 2, pad 0 | 1, C % 4 == 0, x_ld and y_ld multiples of 4, x and y 16-byte aligned. */
enum { MUNIT_WINDOW_MAX = 0, MUNIT_WINDOW_AVG = 1 };
int munit_window3_fwd(const float* x, float* y, int B, int H, int W, int C, int x_ld, int y_ld, int mode, int stride,
                      int pad, munit_stream_t stream);
/* WrapInception.forward's first lines in one launch: v = ((x + 1) / 2 - mean_c) / std_c with the ImageNet statistics, then
 * (unless H = W = 299) the bilinear resize with align_corners = True to 299 x 299.  x: B images of 3 x H x W, layout 0
 * planar [B][3][H][W] or 1 interleaved [B][H][W][3], dense; y: [B][299][299][3]. */
int munit_inception_input(const float* x, int layout, int B, int H, int W, float* y, munit_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Domain-invariant perceptual loss (vgg_w; scripts/trainer.py:618-636; csrc/vgg.hip).  fp32, NHWC,
 * asynchronous on `stream`; every argument check returns MUNIT_ERR_ARG before any launch.  The frozen VGG16 itself runs on
 * the convolution entry points and the 2x2 max-pool above.
 *
 * vgg_preprocess (utils.py:1051-1063): x, y are npix pixels of 3 channels in different buffers; y[p][c] =
 * (x[p][2 - c] + 1) * 255 * 0.5 - mean_c with mean = (103.939, 116.779, 123.680) for the B, G, R planes of y -- the
 * reference's operations in its order, hence torch's result bit for bit.  bwd: dx[p][c] = 127.5 * dy[p][2 - c]. */
int munit_vgg_input_fwd(const float* x, float* y, size_t npix, munit_stream_t stream);
int munit_vgg_input_bwd(const float* dy, float* dx, size_t npix, munit_stream_t stream);
/* out[0] = mean over all B * HW * C elements of (IN(f) - IN(t))^2, IN = instance norm without affine: per (b, c) over the HW
 * pixels, biased variance, eps 1e-5 inside the square root.  f, t: [B][HW][C], C % 4 == 0, B <= 65535; they may be the same
 * buffer.  stats [2][B][C][2] floats receives (mean, 1 / sqrt(var + eps)) of f, then of t, for the backward.  Statistics and the
 * sum are taken in fp64 and reduced in a fixed order in two stages (no atomics): two calls on the same data are bitwise equal,
 * and f == t gives exactly 0.  ws: munit_in_mse_workspace_bytes; a shorter one is refused with MUNIT_ERR_WORKSPACE before
 * anything is written.
 * bwd, to f only: with n_f, n_t the normalised maps, N = B * HW * C and g = 2 gout[0] (n_f - n_t) / N,
 *   df = (g - mean_hw(g) - n_f * mean_hw(g * n_f)) / sqrt(var_f + eps),
 * from the statistics the forward saved; df [B][HW][C] is written in full and must not alias f or t. */
size_t munit_in_mse_workspace_bytes(int B, int C);
int munit_in_mse_fwd(const float* f, const float* t, int B, int HW, int C, float* out, float* stats, void* ws, size_t ws_bytes,
                     munit_stream_t stream);
int munit_in_mse_bwd(const float* f, const float* t, const float* stats, int B, int HW, int C, const float* gout, float* df,
                     munit_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUNIT_HIP_H */
