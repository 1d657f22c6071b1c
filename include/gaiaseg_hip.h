/*
 * gaiaseg_hip.h — C-ABI of the MI355X (gfx950) kernels behind the GAIA-seg supernet hot path.
 *
 * The reference (GAIA-seg) has no FFI: every kernel it runs is reached through torch ops called
 * from Python nn.Modules.  This header therefore declares one entry point
 * per torch-op call site on the hot path; each comment cites the
 * reference call site the entry point replaces.  All functions
 *   - take raw device pointers, sizes, element strides and a hipStream_t passed as void*,
 *   - allocate nothing (workspaces are passed in; query sizes with the *_workspace_bytes calls),
 *   - are re-entrant, keep no global state, never synchronise the device,
 *   - return 0 on success, a negative GS_E_* code for argument errors and a positive hipError_t
 *     value when a launch failed.
 *
 * Tensor conventions (fp32 everywhere, like the reference: fp16_enabled=False,
 * gaiaseg/models/decode_heads/dynamic_fcn_head.py:81):
 *   activations : NHWC, element (n,h,w,c) at n*H*W*ld + (h*W + w)*ld + c, ld >= C ("pixel stride"),
 *                 ld and C multiples of 4 (the only exceptions are the 3-channel input image, read
 *                 through explicit strides, and num_classes, which the host pads to 4 with zeros);
 *   conv weight : physical [KH][KW][Ci_max][Co_ld] (HWIO) — the max-size supernet tensor; the
 *                 kernels read the leading slice [:, :, :Ci, :Co] in place (DynConv2d semantics,
 *                 SURVEY.md Appendix A1), so no per-step repacking of the sliced weight exists;
 *   labels      : int64 [N,H,W], ignore_index (255) allowed.
 */
#ifndef GAIASEG_HIP_H
#define GAIASEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_OK 0
#define GS_E_BADARG (-1)     /* inconsistent / unsupported descriptor */
#define GS_E_ALIGN (-2)      /* pointer or stride not aligned as documented */
#define GS_E_WORKSPACE (-3)  /* workspace too small */
#define GS_E_NULL (-4)       /* required pointer is NULL */

/* ABI version of this header; bumped on any signature change. */
int gs_abi_version(void);
/* Human-readable text for a return code of any function below. */
const char* gs_error_string(int code);
/* gfx target the library was compiled for ("gfx950"). */
const char* gs_target_arch(void);

/* ------------------------------------------------------------------------------------------ */
/* Dynamic (slimmable) convolution as implicit GEMM on fp32 MFMA — K1/K2/K3/K6/K10/K11/K12/K16 */
/* ------------------------------------------------------------------------------------------ */
/* Replaces F.conv2d(x, weight[:Co,:Ci], bias[:Co], stride, padding, dilation) of gaiavision
 * DynConv2d as called from DynamicBottleneck / DynamicConvModule / conv_seg
 * (gaiaseg/models/utils/dynamic_res_layer.py:84-125, gaiaseg/models/backbones/dynamic_resnet.py:255-302,
 *  gaiaseg/models/decode_heads/dynamic_fcn_head.py:76-126, dynamic_psp_head.py:53-59,123,140-147,
 *  dynamic_uper_head.py:40-79) and its autograd backward (dgrad / wgrad). */
typedef struct gs_conv_desc {
  int32_t N, H, W;        /* input batch and spatial size                                   */
  int32_t Ci, Co;         /* ACTIVE channels this step (Co padded to a multiple of 4)       */
  int32_t Ci_max, Co_ld;  /* weight physical dims: [KH][KW][Ci_max][Co_ld], Co_ld % 4 == 0   */
  int32_t KH, KW;
  int32_t stride, pad, dil;
  int32_t Ho, Wo;         /* floor((H + 2p - d(k-1) - 1)/s) + 1, checked by the library      */
  int64_t x_sn, x_sh, x_sw, x_sc; /* element strides of x (NHWC: x_sc = 1; image: NCHW)     */
  int32_t ldy;            /* pixel stride of y / dy (>= Co, % 4 == 0)                        */
  int32_t ld_add;         /* pixel stride of the optional addend (0 if unused)               */
  int32_t role;           /* GS_CONV_ROLE_*: profiling label only, results are identical     */
  int32_t reserved;       /* must be 0                                                       */
  /* Optional: x is the INPUT of a BatchNorm + ReLU whose output the convolution consumes
   * (bottleneck bn1 -> conv2, bn2 -> conv3).  in_affine = that BatchNorm's coefficient block
   * [scale | beta | mean | invstd][Ci] (as written by gs_conv_bn_forward / gs_bn_finalize) and the
   * forward and weight-gradient kernels evaluate relu((x - mean) * scale + beta) in their operand
   * loaders: the normalised activation is never written to or read from HBM, zero padding applies
   * to the activation.  gs_conv2d_dgrad ignores it (its result is the gradient w.r.t. the
   * activation).  Only where gs_conv2d_in_affine_supported(d) != 0; NULL = x is used as it is. */
  const float* in_affine;
} gs_conv_desc;
/* 1 if gs_conv2d_forward / gs_conv2d_wgrad / gs_conv_bn_* accept d->in_affine for this shape
 * (NHWC x, 1x1 or 3x3, Ci % 16 == 0, Ci <= 640: the fast kernels with 64-row tiles). */
int gs_conv2d_in_affine_supported(const gs_conv_desc* d);
/* role = GS_CONV_ROLE_BOTTLENECK3X3 marks conv2 of DynamicBottleneck (SURVEY.md K3,
 * gaiaseg/models/utils/dynamic_res_layer.py:96-106): the forward dispatches an identically compiled
 * but separately NAMED kernel instantiation (igemm_rows_fast_kernel<..., ROLE = 1, ...> and
 * splitk_reduce_kernel<false, 1>), so a rocprofv3 kernel trace reports the headline kernel of
 * bench.py's roofline on its own rows. */
#define GS_CONV_ROLE_GENERIC 0
#define GS_CONV_ROLE_BOTTLENECK3X3 1

/* bytes of split-K scratch the three calls below may use for this descriptor (max of the three) */
size_t gs_conv2d_workspace_bytes(const gs_conv_desc* d);

/* y[n,ho,wo,:Co] = conv(x, w[:, :, :Ci, :Co]) (+ bias[:Co]) (+ addend).  bias/addend may be NULL.
 * The network's stem -- 7x7, stride 2, pad 3, Ci = Ci_max = 3 on the NCHW image, Co in {32, 48, 64},
 * Wo % 128 == 0 (gaiaseg/models/backbones/dynamic_resnet.py:290-297) -- has its own forward and
 * weight-gradient kernels (csrc/stem.hip); gs_debug_last_conv_launch reports them as 128-row tiles. */
int gs_conv2d_forward(const gs_conv_desc* d, const float* x, const float* w, const float* bias,
                      const float* addend, float* y, void* workspace, size_t workspace_bytes,
                      void* stream);
/* dx[n,h,w,:Ci] (= or +=) sum_{taps,co} dy * w.   dx is NHWC with pixel stride x_sw (x_sc == 1).
 * accumulate != 0 adds to the existing dx (residual / multi-consumer gradients). */
int gs_conv2d_dgrad(const gs_conv_desc* d, const float* dy, const float* w, float* dx,
                    int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* dw[:, :, :Ci, :Co] = sum_pixels x (gathered) * dy, written into the max-size gradient tensor
 * (same physical layout as w); the rest of dw is left untouched (zero by the host's contract). */
int gs_conv2d_wgrad(const gs_conv_desc* d, const float* x, const float* dy, float* dw,
                    void* workspace, size_t workspace_bytes, void* stream);

/* out[c] = sum over rows of src[r*ld + c], c < C  (conv_seg bias gradient; also used by tests).
 * workspace >= gs_colsum_workspace_bytes(rows, C). */
size_t gs_colsum_workspace_bytes(int64_t rows, int32_t C);
int gs_colsum(const float* src, int64_t rows, int32_t C, int32_t ld, float* out, void* workspace,
              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Depthwise 3x3 / 7x7 convolution (DeepLabV3+ separable convolutions, ConvNeXt blocks)        */
/* ------------------------------------------------------------------------------------------ */
/* F.conv2d(x, w[:C], bias[:C], stride 1, padding, dilation, groups = C) of a depthwise DynConv2d
 * (mmcv DepthwiseSeparableConvModule.depthwise_conv as used by mmseg's DepthwiseSeparableASPPHead):
 *   y[n,h,w,c] = sum_{kh,kw} x[n, h + kh*dil - pad, w + kw*dil - pad, c] * w[kh,kw,0,c]  (+ bias[c])
 * with zero padding; Ho = H + 2*pad - (KH-1)*dil, Wo likewise.  x is NHWC with pixel stride ldx, y / dy NHWC
 * with pixel stride ldy (a channel slice of a concat buffer is a legal source or destination).  The
 * weight is the physical HWIO tensor with I = 1, [KH][KW][1][C_ld]: channel-contiguous, and only its
 * leading C channels are read (width-dynamic like gs_conv2d_*).  fp32 throughout, whatever
 * gs_set_forward_precision / gs_set_train_precision say.  The kernels are bandwidth-bound: one thread
 * per float4 channel quad over a strip of pixels; the 3x3 kernel keeps its nine weight quads in
 * registers, the 7x7 kernel (ConvNeXt's dwconv) walks the tap columns with seven at a time.
 * Supported: KH = KW = 3 or KH = KW = 7, stride = 1, dil >= 1, pad >= 0 with Ho, Wo >= 1 (GS_E_BADARG otherwise, also
 * for sizes <= 0 and pitches below C); C, C_ld, ldx, ldy multiples of 4 and 16-byte aligned pointers
 * (GS_E_ALIGN); GS_E_NULL for a missing descriptor or pointer.  The descriptor is checked first, on the
 * host, before any launch. */
typedef struct gs_dwconv_desc {
  int32_t N, H, W;        /* input batch and spatial size                                    */
  int32_t C, C_ld;        /* ACTIVE channels; channel pitch of the weight's taps (>= C)      */
  int32_t KH, KW;         /* 3, 3 or 7, 7                                                    */
  int32_t stride, pad, dil;
  int32_t ldx, ldy;       /* pixel strides of x / dx and of y / dy                           */
} gs_dwconv_desc;
/* bytes of scratch gs_dwconv2d_wgrad needs (0 for a descriptor it would refuse): one [KH*KW][C] partial
 * per run of 256 output pixels; non-decreasing in N * Ho * Wo. */
size_t gs_dwconv2d_workspace_bytes(const gs_dwconv_desc* d);
/* bias may be NULL. */
int gs_dwconv2d_forward(const gs_dwconv_desc* d, const float* x, const float* w, const float* bias,
                        float* y, void* stream);
/* dx[n,h,w,:C] (= or +=) the same stencil over dy with mirrored taps; accumulate != 0 adds to dx. */
int gs_dwconv2d_dgrad(const gs_dwconv_desc* d, const float* dy, const float* w, float* dx,
                      int accumulate, void* stream);
/* dw[kh,kw,0,:C] = sum_{n,h,w} x[n, h + kh*dil - pad, w + kw*dil - pad, :C] * dy[n,h,w,:C], written into
 * the max-size gradient tensor [KH][KW][1][C_ld]; channels C..C_ld-1 are never written.  Two launches:
 * per-run partials in the workspace, then their sum in a fixed order -- no float atomics, the result
 * is bit-identical from run to run.  GS_E_WORKSPACE when workspace_bytes is below the query. */
int gs_dwconv2d_wgrad(const gs_dwconv_desc* d, const float* x, const float* dy, float* dw,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* SegNeXt: multi-scale convolutional attention (MSCAN's strip convolutions) and its gate       */
/* ------------------------------------------------------------------------------------------ */
/* The depthwise chain of mmseg's MSCAAttention in one operator, on an NHWC map x [N,H,W,C]:
 *   a   = dwconv K0xK0 (x, w0) + b0                                     (K0 = 5, padding K0/2)
 *   r_i = dwconv 1xK_i (a, w_row[i]) + b_row[i],   i = 0..2             (K = 7, 11, 21, padding K_i/2)
 *   s   = a + sum_i ( dwconv K_ix1 (r_i, w_col[i]) + b_col[i] )
 * stride 1, no dilation, zero padding ("same"), so s has the shape of x.  x / dx have the pixel pitch
 * ldx and s / ds the pitch lds (channel slices of wider buffers are legal).  Every filter is the
 * physical HWIO tensor with I = 1 ([K0][K0][1][C_ld], [1][K][1][C_ld], [K][1][1][C_ld]: channel-contiguous
 * taps with pitch C_ld) and every bias a vector; only their leading C channels are read, and only the
 * leading C channels of the gradients are written.  fp32 in every precision mode.  The kernels are
 * bandwidth-bound: one thread per float4 channel quad over a strip of 8 positions along the filter's
 * axis, taps in the padding skipped.  No float atomics: every sum has a fixed order (per output the taps
 * in their order, the branches i in theirs; filter gradients per run of at most 256 pixels, then the runs
 * in order), so two runs are bit-identical.
 * Checked on the host before any launch: GS_E_NULL (descriptor, tensor, a filter struct or one of its
 * 14 pointers), GS_E_BADARG (a size <= 0, K0 even or outside 1..7, a K[i] even or outside 1..21, a pitch
 * or C_ld below C, more than 2^31 - 1 pixels), GS_E_ALIGN (C, C_ld or a pitch no multiple of 4, a pointer
 * not 16-byte aligned), GS_E_WORKSPACE. */
typedef struct gs_msca_desc {
  int32_t N, H, W;        /* batch and spatial size of x and s                               */
  int32_t C, C_ld;        /* ACTIVE channels; channel pitch of every filter's taps (>= C)    */
  int32_t K0;             /* size of the square filter (odd, <= 7)                           */
  int32_t K[3];           /* lengths of the three strip pairs (odd, <= 21)                   */
  int32_t ldx, lds;       /* pixel strides of x / dx and of s / ds                           */
} gs_msca_desc;
typedef struct gs_msca_filters {
  const float* w0;
  const float* b0;
  const float* w_row[3];  /* 1 x K[i] */
  const float* b_row[3];
  const float* w_col[3];  /* K[i] x 1 */
  const float* b_col[3];
} gs_msca_filters;
typedef struct gs_msca_filter_grads {
  float* w0;
  float* b0;
  float* w_row[3];
  float* b_row[3];
  float* w_col[3];
  float* b_col[3];
} gs_msca_filter_grads;
/* bytes the forward keeps for the backward (0 for a descriptor the calls would refuse): a and the three
 * row results r_i, packed [N*H*W][C] each -- four tensors of the map's size per call.  (Keeping a alone
 * and recomputing r_i would save three of them for one more pass of the row kernel in the backward.) */
size_t gs_msca_saved_bytes(const gs_msca_desc* d);
/* bytes of scratch gs_msca_backward needs (0 for a descriptor it would refuse): the gradients of a and
 * of the r_i (four tensors) and the per-run partials of the 14 parameter gradients.  A function of
 * N*H*W, C and the filter sizes alone, non-decreasing in N*H*W. */
size_t gs_msca_workspace_bytes(const gs_msca_desc* d);
/* s as above; `saved` (gs_msca_saved_bytes(d) bytes, 16-byte aligned) is filled for the backward.
 * Three launches, ten passes over a tensor of the map's size. */
int gs_msca_forward(const gs_msca_desc* d, const float* x, const gs_msca_filters* filters, float* s,
                    void* saved, void* stream);
/* dx[..., :C] (= or +=, accumulate != 0 adds: x usually has a second consumer, the gate) and all 14
 * parameter gradients, written into the max-size gradient tensors (channels C.. are never written).
 * Gradient pointers are never NULL: pass scratch for a frozen parameter.  Seven launches. */
int gs_msca_backward(const gs_msca_desc* d, const float* x, const float* ds, const gs_msca_filters* filters,
                     const void* saved, float* dx, int accumulate, const gs_msca_filter_grads* grads,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The gate on rows x C views with a pixel pitch per operand: y = g * u. */
int gs_gate_mul_forward(const float* g, const float* u, float* y, int64_t rows, int32_t C, int32_t ldg,
                        int32_t ldu, int32_t ldy, void* stream);
/* dg = dy * u (written) and du (= or +=, accumulate != 0 adds) dy * g.  dg may be dy's buffer.
 * GS_E_BADARG (rows or C <= 0, a pitch below C), GS_E_ALIGN (C or a pitch no multiple of 4, a pointer not
 * 16-byte aligned), GS_E_NULL, for the forward alike. */
int gs_gate_mul_backward(const float* dy, const float* g, const float* u, float* dg, float* du,
                         int64_t rows, int32_t C, int32_t lddy, int32_t ldg, int32_t ldu, int32_t lddg,
                         int32_t lddu, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* ConvNeXt block operators: LayerNorm over channels, GELU, layer scale + residual              */
/* ------------------------------------------------------------------------------------------ */
/* All on NHWC fp32 "rows x C" views: rows = N*H*W pixels, C ACTIVE channels, a pixel pitch ld >= C per
 * operand (a channel slice of a wider buffer is a legal operand), parameters sliced to their leading C
 * channels.  fp32 in every precision mode.  Arguments are checked on the host before any launch:
 * GS_E_NULL (descriptor or pointer), GS_E_BADARG (rows or C <= 0, a pitch below C, eps <= 0),
 * GS_E_ALIGN (C or a pitch no multiple of 4, a tensor pointer not 16-byte aligned), GS_E_WORKSPACE.
 * No float atomics: every reduction has a fixed order and is bit-identical from run to run.
 *
 * LayerNorm (nn.LayerNorm(C) on channels_last data == the ConvNeXt channels_first LayerNorm on NCHW):
 *   y[r,c] = (x[r,c] - mean[r]) * rstd[r] * weight[c] + bias[c],   rstd = 1 / sqrt(var + eps),
 * var the biased variance of the row.  mean and rstd are [rows] and are saved for the backward.  Any C
 * that is a multiple of 4 (a row is walked by up to one wave in as many steps as it needs). */
typedef struct gs_layernorm_desc {
  int64_t rows;           /* N*H*W                                                           */
  int32_t C;              /* ACTIVE channels                                                 */
  int32_t ldx, ldy;       /* pixel strides of x / dx and of y / dy                           */
  float eps;
} gs_layernorm_desc;
int gs_layernorm_forward(const gs_layernorm_desc* d, const float* x, const float* weight,
                         const float* bias, float* y, float* mean, float* rstd, void* stream);
/* bytes of scratch gs_layernorm_backward needs (0 for a descriptor it would refuse): one [2][C] partial
 * per run of 256 rows. */
size_t gs_layernorm_workspace_bytes(const gs_layernorm_desc* d);
/* dx[r,:C] (= or +=, accumulate != 0 adds) the LayerNorm data gradient; dweight[:C] = sum_r dy * xhat and
 * dbias[:C] = sum_r dy through per-run partials in the workspace and their ordered sum.  Channels C..
 * of dweight / dbias are never written.  dx may be dy's buffer when ldx == ldy. */
int gs_layernorm_backward(const gs_layernorm_desc* d, const float* x, const float* dy,
                          const float* weight, const float* mean, const float* rstd, float* dx,
                          float* dweight, float* dbias, int accumulate, void* workspace,
                          size_t workspace_bytes, void* stream);
/* nn.GELU() (exact erf form): y = x * 0.5 * (1 + erf(x / sqrt 2)). */
int gs_gelu_forward(const float* x, float* y, int64_t rows, int32_t C, int32_t ldx, int32_t ldy,
                    void* stream);
/* dx = dy * (Phi(x) + x * phi(x)), recomputed from the saved pre-activation x.  dx may be dy's buffer. */
int gs_gelu_backward(const float* x, const float* dy, float* dx, int64_t rows, int32_t C, int32_t ldx,
                     int32_t lddy, int32_t lddx, void* stream);
/* out[r,c] = identity[r,c] + gamma[c] * z[r,c]  (ConvNeXt: x = input + gamma * branch).  out may be
 * identity's buffer. */
int gs_layer_scale_add_forward(const float* identity, const float* z, const float* gamma, float* out,
                               int64_t rows, int32_t C, int32_t ldi, int32_t ldz, int32_t ldo,
                               void* stream);
/* one [C] partial per run of 256 rows (0 for arguments gs_layer_scale_backward would refuse). */
size_t gs_layer_scale_workspace_bytes(int64_t rows, int32_t C);
/* dz[r,:C] = gamma * dout and dgamma[:C] = sum_r dout * z (per-run partials, then their ordered sum);
 * channels C.. of dgamma are never written.  The identity's gradient is dout itself.  dz may be dout's
 * or z's buffer. */
int gs_layer_scale_backward(const float* dout, const float* z, const float* gamma, float* dz,
                            float* dgamma, int64_t rows, int32_t C, int32_t lddo, int32_t ldz,
                            int32_t lddz, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* ConvNeXt V2: GELU fused with Global Response Normalization (arXiv 2301.00808)                */
/* ------------------------------------------------------------------------------------------ */
/* On the [N, P, C] hidden tensor of a block (P = H*W pixels per sample, C ACTIVE channels, NHWC rows
 * with a pixel pitch per operand), with a = gelu(x) in the exact erf form of gs_gelu_*:
 *   G[n,c]  = sqrt(sum_p a[n,p,c]^2)
 *   Nx[n,c] = G[n,c] / (mean over the C active channels of G[n,:] + eps)
 *   y[n,p,c] = a[n,p,c] * (1 + weight[c] * Nx[n,c]) + bias[c]
 * a is never stored: the forward reads x twice and writes y, the backward reads dy and x twice and
 * writes dx.  weight / bias are the physical max-size vectors; only their leading C entries are read,
 * and only the leading C entries of dweight / dbias are written.  fp32 in every precision mode, no
 * atomics, every sum in a fixed order (sums over pixels in runs of 256 cut per sample, so the result
 * for a sample does not depend on the batch it sits in).  Checked on the host before any launch:
 * GS_E_NULL (descriptor or pointer), GS_E_BADARG (N, P or C <= 0, a pitch below C, eps <= 0,
 * N > 65535), GS_E_ALIGN (C or a pitch no multiple of 4, a pointer not 16-byte aligned), GS_E_WORKSPACE. */
typedef struct gs_gelu_grn_desc {
  int32_t N, P;           /* samples, pixels per sample (H*W)                                */
  int32_t C;              /* ACTIVE channels                                                 */
  int32_t ldx, ldy;       /* pixel strides of x and y                                        */
  int32_t lddy, lddx;     /* pixel strides of dy and dx                                      */
  float eps;
} gs_gelu_grn_desc;
/* bytes of scratch either direction needs (0 for a descriptor they would refuse): [2][C] partials per
 * run of 256 pixels of a sample, and [4][C] per sample for their sums and the backward's coefficients. */
size_t gs_gelu_grn_workspace_bytes(const gs_gelu_grn_desc* d);
/* y as above; G [N][C] is saved for the backward. */
int gs_gelu_grn_forward(const gs_gelu_grn_desc* d, const float* x, const float* weight, const float* bias,
                        float* y, float* G, void* workspace, size_t workspace_bytes, void* stream);
/* With S[n,c] = sum_p dy * a, T[n,c] = sum_p dy, D = weight * S and m = mean_c G[n,:] + eps:
 *   dbias[c] = sum_n T,  dweight[c] = sum_n Nx * S  (samples added in order),
 *   dG[n,c] = D / m - (1/C) sum_c' D[n,c'] G[n,c'] / m^2,
 *   dx = (dy * (1 + weight * Nx) + a * dG / G) * gelu'(x),  the term through G zero where G == 0.
 * a and gelu' are recomputed from the saved pre-activation x.  dx may be dy's buffer. */
int gs_gelu_grn_backward(const gs_gelu_grn_desc* d, const float* x, const float* dy, const float* weight,
                         const float* G, float* dx, float* dweight, float* dbias, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* ConvTranspose2d(kernel_size = 2, stride = 2), forward only (BEiT's fpn1 / fpn2)              */
/* ------------------------------------------------------------------------------------------ */
/* y[n, 2 h + dy, 2 w + dx, :Cout] = sum_ci x[n, h, w, ci] * w4[ci][(2 dy + dx) * Cout + co] (+ bias[co]):
 * kernel == stride, so the four taps are four independent 1x1 convolutions.  They run as ONE
 * gs_conv2d_forward GEMM Cin -> 4 Cout (the MFMA implicit-GEMM kernels, in the library's forward
 * precision) into scratch, and a depth-to-space kernel moves the rows to their output pixels and adds the
 * bias.  x: NHWC fp32 [N][H][W] with pixel pitch ldx >= Cin; w4: [Cin][4 Cout] packed, i.e. torch's
 * ConvTranspose2d weight [Cin][Cout][2][2] permuted to [Cin][2][2][Cout]; bias: [Cout] or NULL;
 * y: NHWC [N][2 H][2 W] with pixel pitch ldy >= Cout, columns Cout.. are not written.
 * GS_E_BADARG (a size <= 0, a pitch below its width, more than 2^31 - 1 output pixels), GS_E_ALIGN (Cin,
 * Cout or a pitch no multiple of 4, a pointer not 16-byte aligned), GS_E_NULL, GS_E_WORKSPACE (below
 * gs_deconv2x2_workspace_bytes, which is 0 for sizes the forward refuses). */
size_t gs_deconv2x2_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
int gs_deconv2x2_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t ldx,
                         const float* w4, int32_t Cout, const float* bias, float* y, int32_t ldy,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Multi-head softmax self-attention (head dimension 64) and the ViT token assembly             */
/* ------------------------------------------------------------------------------------------ */
/* ElasticMHA.forward with relative_position=False (gaiaseg/models/backbones/elastic_transformer.py):
 *   O[b,i,h,:] = sum_j softmax_j(scale * <Q[b,i,h,:], K[b,j,h,:]>) V[b,j,h,:],   no mask, no dropout.
 * Q, K, V, O and their gradients are fp32 "rows x C" views as above: rows = B*N tokens, head h in columns
 * [64 h, 64 h + 64), one pitch >= 64 * heads per operand; a column slice of a wider buffer is a legal
 * operand (Q, K, V as three slices of one buffer).  `heads` is the ACTIVE head count.  fp32-accurate in
 * every precision mode (exact fp32 MFMA); no N x N matrix is stored (online softmax over key tiles of 32
 * rows; a workgroup owns 128 query rows).  lse[b,h,i] = log sum_j exp(scale * <q_i, k_j>) is [B][heads][N]
 * and is saved for the backward.  No float atomics; bit-identical from run to run.
 * Checked on the host before any launch: GS_E_NULL (descriptor or pointer), GS_E_BADARG (B, N or heads
 * <= 0, B or heads > 65535, a pitch below 64 * heads, scale <= 0), GS_E_ALIGN (a pitch no multiple of 4, a
 * pointer not 16-byte aligned), GS_E_WORKSPACE.  Nothing outside the active columns of O / dQ / dK / dV
 * is written. */
typedef struct gs_attention_desc {
  int32_t B, N, heads;              /* batch, tokens per image, ACTIVE heads                     */
  int32_t ldq, ldk, ldv, ldo;       /* token pitches of Q, K, V, O                               */
  int32_t lddq, lddk, lddv, lddo;   /* token pitches of dQ, dK, dV, dO (all eight are checked)   */
  float scale;                      /* 64^-0.5 in ElasticMHA                                     */
} gs_attention_desc;
int gs_attention_forward(const gs_attention_desc* d, const float* q, const float* k, const float* v,
                         float* o, float* lse, void* stream);
/* BEiT's attention (forward only: the frozen teacher of DynamicDistiller): gs_attention_forward with an
 * additive per-head relative-position bias,
 *   O[b,i,h,:] = sum_j softmax_j(scale * <q_i, k_j> + table[idx(i,j)][h]) v_j,
 * for N = Wh * Ww + 1 tokens, token 0 the cls token and token t >= 1 at (ty, tx) = divmod(t - 1, Ww) of the
 * Wh x Ww patch window.  With R = (2 Wh - 1)(2 Ww - 1):
 *   idx(i, j) = (iy - jy + Wh - 1) * (2 Ww - 1) + (ix - jx + Ww - 1)   for i, j >= 1,
 *   idx(0, j >= 1) = R,   idx(i >= 1, 0) = R + 1,   idx(0, 0) = R + 2.
 * table is fp32 [R + 3][heads] with row pitch ld_table >= heads: a checkpoint's
 * relative_position_bias_table as it stands.  q, k, v, o, lse and d as for gs_attention_forward (same
 * kernel, same exact-fp32 products, online softmax, fixed summation order, no atomics); lse includes the
 * bias.  No N x N tensor exists anywhere: a workgroup stages its head's column of the table in LDS and
 * gathers from it, which caps the table at GS_ATTENTION_RELPOS_MAX_ROWS rows (32 KiB beside the 16.5 KiB
 * of key / value tiles; windows 32 x 64 and 40 x 40 fit).  A zero table gives the bits of
 * gs_attention_forward.
 * Checked before any launch: what gs_attention_forward checks, then GS_E_BADARG for Wh or Ww < 1,
 * N != Wh * Ww + 1, ld_table < heads or R + 3 > GS_ATTENTION_RELPOS_MAX_ROWS; GS_E_NULL (table too);
 * GS_E_ALIGN (table: 4-byte aligned). */
#define GS_ATTENTION_RELPOS_MAX_ROWS 8192
int gs_attention_relpos_forward(const gs_attention_desc* d, const float* q, const float* k, const float* v,
                                const float* table, int32_t ld_table, int32_t Wh, int32_t Ww, float* o,
                                float* lse, void* stream);
/* bytes of scratch gs_attention_backward needs (0 for a descriptor it would refuse): delta[B][heads][N]. */
size_t gs_attention_workspace_bytes(const gs_attention_desc* d);
/* dQ, dK, dV (each = or +=, accumulate != 0 adds) from Q, K, V, O, lse and dO.  P is recomputed from Q, K
 * and lse; delta = <dO, O> goes through the workspace.  Two kernels: one workgroup per 128 keys owns dK /
 * dV and sweeps the queries, one per 128 queries owns dQ and sweeps the keys. */
int gs_attention_backward(const gs_attention_desc* d, const float* q, const float* k, const float* v,
                          const float* o, const float* lse, const float* d_o, float* dq, float* dk,
                          float* dv, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* The opt-in fp16-operand twins of the four entries above (csrc/attention_f16.hip: the same kernel
 * templates of csrc/attention_common.h on another operand format): same descriptor, same
 * arguments, same host-side checks and error codes, same padding rules, fp32 in memory, no float atomics,
 * bit-identical from run to run -- but every product runs on v_mfma_f32_32x32x16_f16 with fp32
 * accumulation, so they are NOT fp32-accurate: Q, K, V and dO are rounded to fp16 once where they are
 * staged; the scores, the relative-position bias, the running maximum, the row sum, lse and delta stay
 * fp32; exp(S - m) is rounded to fp16 only as the operand of the P V product (the row sum adds the fp32
 * values); the backward recomputes S with the forward's instruction and k order and rounds exp(S - lse) and
 * dS = P (dP - delta) to fp16 as operands.  The backward is invariant to a power-of-two scale of dO (a
 * loss scale): its pre-pass records max|dO| per workgroup beside delta, every product runs on dO * 2^e with
 * 2^e max|dO| in [4, 8), and the results are multiplied by 2^-e at the store; dO == 0 gives exact zeros;
 * the conversion of dS saturates at the fp16 maximum.  lse of gs_attention_forward_f16 is what
 * gs_attention_backward_f16 expects (a pair: do not mix with the fp32 entries).  A zero table gives the
 * bits of gs_attention_forward_f16.  The workspace is delta[B][heads][N] followed by the
 * B * heads * ceil(N / 128) maxima.  Error bounds and the protocol that tests them: DESIGN.md section 32. */
int gs_attention_forward_f16(const gs_attention_desc* d, const float* q, const float* k, const float* v,
                             float* o, float* lse, void* stream);
int gs_attention_relpos_forward_f16(const gs_attention_desc* d, const float* q, const float* k, const float* v,
                                    const float* table, int32_t ld_table, int32_t Wh, int32_t Ww, float* o,
                                    float* lse, void* stream);
size_t gs_attention_workspace_bytes_f16(const gs_attention_desc* d);
int gs_attention_backward_f16(const gs_attention_desc* d, const float* q, const float* k, const float* v,
                              const float* o, const float* lse, const float* d_o, float* dq, float* dk,
                              float* dv, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* Attention with separate query and key lengths (the spatial-reduction attention of SegFormer's Mix
 * Transformer: all Nq tokens of a stage attend to the Nk tokens of a map reduced by sr_ratio):
 *   O[b,i,h,:] = sum_{j < Nk} softmax_j(scale * <Q[b,i,h,:], K[b,j,h,:]>) V[b,j,h,:],   i < Nq.
 * Q, O, dQ, dO are [B*Nq] rows, K, V, dK, dV are [B*Nk] rows, lse is [B][heads][Nq]; everything else is the
 * contract of gs_attention_* above, and these ARE those kernels (csrc/attention_common.h) with the owned and
 * the swept length taken from different fields: exact fp32 MFMA, online softmax (no Nq x Nk matrix), no float
 * atomics, a fixed summation order (bit-identical from run to run), nothing written outside the active
 * columns and rows, rows past Nq or Nk staged as zeros and never read, a key past Nk scores -inf.  Any
 * Nq >= 1 and Nk >= 1 is legal, Nk > Nq too.  With Nq == Nk and a forced split of 1 every output equals
 * gs_attention_* bit for bit.  The same host-side checks and codes, applied to both lengths.
 * Backward: dQ as in gs_attention_backward (a workgroup owns 128 queries and sweeps the keys).  dK / dV: a
 * workgroup owns 128 keys and sweeps one SLAB of the queries; the grid has a slab dimension S.  S == 1
 * stores dK / dV directly.  S > 1: every slab (whole 32-row tiles of queries; none is empty) writes its
 * [B*Nk][64 * heads] partials of dK and dV into the workspace and a second launch sums them in slab order
 * into dK / dV (= or +=).  S is a pure function of the descriptor and the device's CU count: the key tiles
 * x heads x B workgroups are multiplied until they fill one round of the CUs (the kernel runs one workgroup
 * per CU), with at least 4 query tiles per slab.  The workspace is delta[B][heads][Nq] (rounded up to 16 bytes) followed by
 * the partials [2][S][B*Nk][64 * heads] when S > 1.
 * gs_debug_set_attention_kv_split(S >= 1) forces the split (clipped to what gives whole, non-empty slabs) for
 * the workspace query and the backward alike; -1 restores the plan; anything else is GS_E_BADARG. */
typedef struct gs_attention_kv_desc {
  int32_t B, Nq, Nk, heads;         /* batch, queries and keys per image, ACTIVE heads           */
  int32_t ldq, ldk, ldv, ldo;       /* token pitches of Q, K, V, O                               */
  int32_t lddq, lddk, lddv, lddo;   /* token pitches of dQ, dK, dV, dO (all eight are checked)   */
  float scale;
} gs_attention_kv_desc;
int gs_attention_kv_forward(const gs_attention_kv_desc* d, const float* q, const float* k, const float* v,
                            float* o, float* lse, void* stream);
size_t gs_attention_kv_workspace_bytes(const gs_attention_kv_desc* d);
int gs_attention_kv_backward(const gs_attention_kv_desc* d, const float* q, const float* k, const float* v,
                             const float* o, const float* lse, const float* d_o, float* dq, float* dk,
                             float* dv, int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int gs_debug_set_attention_kv_split(int32_t S);
/* Swin's shifted-window attention, head dimension 32 (transformers' SwinLayer with always_partition):
 * attention local to ws x ws windows of an NHWC map [B][H][W] (the PADDED map: H % ws == W % ws == 0), on a
 * cyclically shifted frame with a region mask when shift > 0, with a learned per-head relative-position bias.
 * Row b*H*W + y*W + x of every operand is the token at (y, x); head h sits in columns [32 h, 32 h + 32); one
 * pitch per operand (Q, K, V may be three column slices of one buffer); `heads` is the ACTIVE head count.
 *   shifted frame  y' = (y - shift) mod H, x' = (x - shift) mod W;   window (y' / ws, x' / ws);
 *   in-window position (iy, ix) = (y' % ws, x' % ws);
 *   s(i, j) = scale * <q_i, k_j> + table[idx(i, j)][h] + mask(i, j)   for tokens i, j of one window,
 *   idx(i, j) = (iy - jy + ws - 1) * (2 ws - 1) + (ix - jx + ws - 1),
 *   mask = 0 if shift == 0 or region(i) == region(j), else -100.0 (finite, as in the original),
 *   region(y', x') = 3 r(y', H) + r(x', W),   r(t, L) = (t >= L - ws) + (t >= L - shift),
 *   O_i = sum_j softmax_j(s(i, j)) v_j.
 * table is fp32 [(2 ws - 1)^2][ld_table], ld_table >= heads (a checkpoint's relative_position_bias_table at
 * the supernet's maximum head count; the leading `heads` columns are read).  lse is [B][heads][H*W] at the
 * token's (y, x) and is saved for the backward.  The roll, the partition, the bias gather, the mask, the
 * reverse and the roll back are index arithmetic inside one kernel (csrc/window_attention.hip): a one-wave
 * workgroup per (window, head), the ws^2 tokens padded to 64 in LDS (a padded key scores -inf and contributes
 * nothing, a padded query is never stored), every product on the exact fp32 MFMA.
 * Backward: dQ, dK, dV (each = or +=) are complete inside a window.  dtable[r][h] = (or +=, the same flag) the
 * sum over batch, windows and pairs with idx == r of dS; only columns < heads are written.  It is formed
 * without atomics: the (batch, window) items are cut into S slabs of consecutive items, a workgroup per (slab,
 * head) walks its slab and sums every table entry's pairs in a fixed order, writes its [heads][(2 ws - 1)^2]
 * partial to the workspace (S * heads * (2 ws - 1)^2 floats, rounded up to 16 bytes), and a second launch
 * adds the partials in slab order.  S is a pure function of the descriptor and the CU count (3 * CUs / heads,
 * at most one item per slab); gs_debug_set_window_attention_split(S >= 1) forces it (clipped so that no slab
 * is empty) for the query and the backward alike, -1 restores the plan, anything else is GS_E_BADARG.
 * Bit-identical from run to run.  Nothing outside the active columns and rows is written.
 * Checked on the host before any launch, in this order: GS_E_NULL (descriptor); GS_E_BADARG (B, H, W or heads
 * <= 0, B or heads > 65535, scale <= 0, ws outside 2..8, H % ws or W % ws != 0, shift outside [0, ws), more
 * than 2^31 - 1 tokens); GS_E_ALIGN (a pitch no multiple of 4); GS_E_BADARG (a pitch below 32 * heads,
 * ld_table < heads); GS_E_NULL (any pointer, table and dtable included); GS_E_ALIGN (an operand pointer not
 * 16-byte aligned, table or dtable not 4-byte aligned); GS_E_WORKSPACE. */
typedef struct gs_window_attention_desc {
  int32_t B, H, W;                  /* batch and the (padded) map                                */
  int32_t ws, shift, heads;         /* window size 2..8, shift in [0, ws), ACTIVE heads          */
  int32_t ldq, ldk, ldv, ldo;       /* token pitches of Q, K, V, O                               */
  int32_t lddq, lddk, lddv, lddo;   /* token pitches of dQ, dK, dV, dO (all eight are checked)   */
  int32_t ld_table;                 /* row pitch of table and dtable                             */
  float scale;                      /* 32^-0.5 in Swin                                           */
} gs_window_attention_desc;
int gs_window_attention_forward(const gs_window_attention_desc* d, const float* q, const float* k,
                                const float* v, const float* table, float* o, float* lse, void* stream);
size_t gs_window_attention_workspace_bytes(const gs_window_attention_desc* d);
int gs_window_attention_backward(const gs_window_attention_desc* d, const float* q, const float* k,
                                 const float* v, const float* table, const float* o, const float* lse,
                                 const float* d_o, float* dq, float* dk, float* dv, float* dtable,
                                 int accumulate, void* workspace, size_t workspace_bytes, void* stream);
int gs_debug_set_window_attention_split(int32_t S);
/* Window padding as a materialised pad and crop; each is the other's backward.
 * gs_map_pad: dst[b, y, x, :C] (= or +=) src[b, y, x, :C] for y < H and x < W, else 0: src is [B][H][W] with
 * pixel pitch lds, dst [B][Hp][Wp] with pitch ldd, Hp >= H, Wp >= W.
 * gs_map_crop: dst[b, y, x, :C] (= or +=) src[b, y, x, :C]: src is [B][Hp][Wp] (pitch lds), dst [B][H][W]
 * (pitch ldd).  Columns C.. are never written.  GS_E_BADARG (a size <= 0, Hp < H, Wp < W, a pitch below C,
 * more than 2^31 - 1 pixels), GS_E_ALIGN (C or a pitch no multiple of 4, a pointer not 16-byte aligned),
 * GS_E_NULL. */
int gs_map_pad(const float* src, int32_t lds, float* dst, int32_t ldd, int32_t B, int32_t H, int32_t W,
               int32_t Hp, int32_t Wp, int32_t C, int accumulate, void* stream);
int gs_map_crop(const float* src, int32_t lds, float* dst, int32_t ldd, int32_t B, int32_t H, int32_t W,
                int32_t Hp, int32_t Wp, int32_t C, int accumulate, void* stream);
/* The LayerNorm of Swin's patch merging without the space-to-depth copy: statistics over the 4 C values of
 * each 2 x 2 cell of an NHWC map [B][H][W] (H, W even), the result written back as a map of the same shape
 * (a 2x2 stride-2 gs_conv2d then is the reduction).  Pixel (2 cy + r, 2 cx + q) of a cell is phase
 * g = 2 q + r (transformers' order of the four concatenated slices) and reads weight and bias at
 * g * Cmax + c: a subnet of C active channels under a maximum of Cmax takes the leading C channels of each of
 * the four groups of the [4 Cmax] parameters.
 *   y = (x - mean[cell]) * rstd[cell] * weight[g Cmax + c] + bias[g Cmax + c],  rstd = 1 / sqrt(var + eps).
 * mean and rstd are [B * H/2 * W/2] and are saved for the backward.  Backward: dx (= or +=, pitch ldx);
 * dweight and dbias (written, =) at g * Cmax + c for c < C only, through one [2][4 C] partial per run of 64
 * cells in the workspace and their sum in run order.  No atomics; bit-identical from run to run.
 * GS_E_NULL, GS_E_BADARG (a size <= 0, odd H or W, Cmax < C, a pitch below C, eps <= 0, more than 2^31 - 1
 * pixels), GS_E_ALIGN (C, Cmax or a pitch no multiple of 4, a tensor pointer not 16-byte aligned),
 * GS_E_WORKSPACE. */
typedef struct gs_cell_layernorm_desc {
  int32_t B, H, W;        /* the map (H and W even)                                          */
  int32_t C, Cmax;        /* ACTIVE channels, channel count of a parameter group             */
  int32_t ldx, ldy;       /* pixel pitches of x / dx and of y / dy                           */
  float eps;
} gs_cell_layernorm_desc;
int gs_cell_layernorm_forward(const gs_cell_layernorm_desc* d, const float* x, const float* weight,
                              const float* bias, float* y, float* mean, float* rstd, void* stream);
size_t gs_cell_layernorm_workspace_bytes(const gs_cell_layernorm_desc* d);
int gs_cell_layernorm_backward(const gs_cell_layernorm_desc* d, const float* x, const float* dy,
                               const float* weight, const float* mean, const float* rstd, float* dx,
                               float* dweight, float* dbias, int accumulate, void* workspace,
                               size_t workspace_bytes, void* stream);
/* ElasticTransformer's token assembly on the leading D columns: from patches [B*T][D] (pitch ldp),
 * cls_token[:D] and pos_embed[:T+1, :D] (pitch ldpos, the max-size embedding width),
 *   x[b,0,:] = cls_token + pos_embed[0],   x[b,1+t,:] = patches[b,t] + pos_embed[1+t]      (x: [B*(T+1)][D]).
 * GS_E_BADARG for B, T or D <= 0 or a pitch below D, GS_E_ALIGN for D or a pitch no multiple of 4 or a
 * pointer not 16-byte aligned, GS_E_NULL. */
int gs_vit_tokens_forward(const float* patches, int32_t ldp, const float* cls_token, const float* pos_embed,
                          int32_t ldpos, float* x, int32_t ldx, int32_t B, int32_t T, int32_t D, void* stream);
/* dpatches[b,t,:D] = dx[b,1+t]; dpos_embed[n,:D] = sum_b dx[b,n] and dcls_token[:D] = sum_b dx[b,0], summed
 * in the order of b.  Columns D.. and rows T+1.. are never written. */
int gs_vit_tokens_backward(const float* dx, int32_t lddx, float* dpatches, int32_t lddp, float* dcls_token,
                           float* dpos_embed, int32_t ldpos, int32_t B, int32_t T, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* ElasticConvformer: the coupling units between the conv branch and the token stream           */
/* ------------------------------------------------------------------------------------------ */
/* All on fp32 "rows x C" views as the ConvNeXt operators above: a pitch >= the width per operand,
 * parameters sliced to their leading columns, fp32 in every precision mode, arguments checked on the host
 * before any launch (GS_E_NULL, GS_E_BADARG for a size <= 0, a pitch below the width, eps <= 0 or an s that
 * does not divide H and W, GS_E_ALIGN for a width or pitch no multiple of 4 or a tensor pointer not
 * 16-byte aligned, GS_E_WORKSPACE).  No float atomics; every sum has a fixed order.
 *
 * Conv features to tokens (Elastic_conv2trans after its pooling and projection, and the `x_st + x_t` of
 * Elastic_ConvTrans_Block.forward, gaiaseg/models/backbones/elastic_convformer.py).  z is [B*T][D], the
 * token stream x_t and out are [B*(T+1)][D] with the cls row in front of every image:
 *   out[b,0,:]   = x_t[b,0,:] + x_t[b,0,:]
 *   out[b,1+t,:] = x_t[b,1+t,:] + gelu(LN(z[b,t,:]) * weight + bias)            (exact-erf GELU)
 * mean and rstd are [B*T] and are saved for the backward. */
typedef struct gs_fcu_down_desc {
  int32_t B, T, D;          /* images, tokens per image without the cls row, ACTIVE width        */
  int32_t ldz, ldxt, ldo;   /* pitches of z, of x_t and of out / dout                            */
  int32_t lddz, lddxt;      /* pitches of dz and of dx_t (all five are always checked)           */
  float eps;
} gs_fcu_down_desc;
int gs_fcu_down_forward(const gs_fcu_down_desc* d, const float* z, const float* x_t, const float* weight,
                        const float* bias, float* out, float* mean, float* rstd, void* stream);
/* bytes of scratch gs_fcu_down_backward needs (0 for a descriptor it would refuse): one [2][D] partial
 * per run of 256 rows of z. */
size_t gs_fcu_down_workspace_bytes(const gs_fcu_down_desc* d);
/* From dout [B*(T+1)][D]: dx_t (= or +=, accumulate_dx_t != 0 adds) dout on token rows and 2 dout on cls
 * rows; dz the gradient through the GELU and the LayerNorm, the GELU input recomputed from z, mean and
 * rstd; dweight[:D] / dbias[:D] through per-run partials and their ordered sum (columns D.. are never
 * written).  dx_t may be dout's buffer. */
int gs_fcu_down_backward(const gs_fcu_down_desc* d, const float* z, const float* dout, const float* weight,
                         const float* bias, const float* mean, const float* rstd, float* dz, float* dx_t,
                         float* dweight, float* dbias, int accumulate_dx_t, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Tokens to conv features (the F.interpolate of Elastic_trans2conv, nearest with an integer factor, and the
 * `x + x_t` in front of conv2 of Elastic_conv_Block):  out[b,y,x,:C] = x[b,y,x,:C] + r[b,y/s,x/s,:C] with
 * x, out [B][H][W] and r [B][H/s][W/s]; s >= 1 divides H and W.  out may be x's buffer. */
int gs_fcu_up_add_forward(const float* x, const float* r, float* out, int32_t B, int32_t H, int32_t W,
                          int32_t C, int32_t s, int32_t ldx, int32_t ldr, int32_t ldo, void* stream);
/* dr[b,i,j,:C] (= or +=) the sum of dout over the s x s block of (i, j), rows first, then columns (s == 1:
 * dout itself).  H, W are the sizes of dout.  The gradient of x is dout. */
int gs_fcu_up_add_backward(const float* dout, float* dr, int32_t B, int32_t H, int32_t W, int32_t C,
                           int32_t s, int32_t lddo, int32_t lddr, int accumulate, void* stream);
/* The token assembly without a position embedding:  x[b,0,:D] = cls_token[:D],  x[b,1+t,:D] = patches[b,t]
 * (x: [B*(T+1)][D]); dpatches[b,t] = dx[b,1+t], dcls_token[:D] = sum_b dx[b,0] in the order of b. */
int gs_fcu_tokens_forward(const float* patches, int32_t ldp, const float* cls_token, float* x, int32_t ldx,
                          int32_t B, int32_t T, int32_t D, void* stream);
int gs_fcu_tokens_backward(const float* dx, int32_t lddx, float* dpatches, int32_t lddp, float* dcls_token,
                           int32_t B, int32_t T, int32_t D, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* OCRNet: the soft-region gather and the pixel-to-region attention                             */
/* ------------------------------------------------------------------------------------------ */
/* Both on fp32 "rows x C" views as the operators above (a pitch >= the width per operand, float4
 * multiples, 16-byte aligned bases), fp32 in every precision mode.  No float atomics: every sum over
 * pixels goes through partials per run of rows and a fixed-order sum, so results are bit-identical from
 * run to run.  Pad columns are never read and nothing outside the active columns is written.  Workspaces
 * come from the caller (the queries need no device), so both are safe inside a captured step graph.
 * Checked on the host before any launch: GS_E_NULL (descriptor or pointer), GS_E_BADARG (a size <= 0,
 * K > GS_OCR_MAX_CLASSES, a width above its maximum, B > 65535, B * P >= 2^31, a pitch below its width, a
 * scale that is not finite), GS_E_ALIGN (a width or a pitch no multiple of 4, a tensor pointer not
 * 16-byte aligned), GS_E_WORKSPACE. */
#define GS_OCR_MAX_CLASSES 256
#define GS_OCR_GATHER_MAX_CHANNELS 2048
#define GS_OCR_ATTEND_MAX_CHANNELS 512
/* mmseg's SpatialGatherModule.  logits L [B][P][K] (pitch ldl >= K), features F [B][P][C]:
 *   w[b,k,p]   = softmax over the P pixels of scale * L[b,p,k]
 *   ctx[b,k,:] = sum_p w[b,k,p] * F[b,p,:]                                        (ctx: [B][K][C])
 * w is never stored; stats [B][K][2] receives (max, log sum) of every class map for the backward. */
typedef struct gs_ocr_gather_desc {
  int32_t B, P, K, C;         /* images, pixels per image, classes, ACTIVE feature width         */
  int32_t ldl, ldf, ldc;      /* pitches of the logits, of the features and of ctx               */
  int32_t lddl, lddf, lddc;   /* pitches of dlogits, dfeats and dctx (all six are always checked) */
  float scale;
} gs_ocr_gather_desc;
/* bytes of scratch either direction needs (0 for a descriptor they would refuse): the statistics'
 * partials per run of 64 rows, and one [K][C] partial per run of 128 rows. */
size_t gs_ocr_gather_workspace_bytes(const gs_ocr_gather_desc* d);
int gs_ocr_gather_forward(const gs_ocr_gather_desc* d, const float* logits, const float* feats, float* ctx,
                          float* stats, void* workspace, size_t workspace_bytes, void* stream);
/* With t[b,k] = <dctx[b,k,:], ctx[b,k,:]> (= sum_p w dw) and dw[b,k,p] = <dctx[b,k,:], F[b,p,:]>:
 *   dfeats[b,p,:] (= or +=, accumulate_dfeats != 0 adds) sum_k w[b,k,p] * dctx[b,k,:]
 *   dlogits[b,p,k] = scale * w[b,k,p] * (dw[b,k,p] - t[b,k])
 * and columns K .. round_up(K, 4) - 1 of dlogits are zeroed. */
int gs_ocr_gather_backward(const gs_ocr_gather_desc* d, const float* logits, const float* feats, const float* ctx,
                           const float* stats, const float* dctx, float* dlogits, float* dfeats,
                           int accumulate_dfeats, void* workspace, size_t workspace_bytes, void* stream);
/* The core of mmseg's SelfAttentionBlock as ObjectAttentionBlock uses it.  Queries Q [B][P][ch], keys Kr and
 * values V [B][K][ch]:
 *   a[b,p,k]   = softmax over the K regions of ch^-0.5 * <Q[b,p,:], Kr[b,k,:]>
 *   out[b,p,:] = sum_k a[b,p,k] * V[b,k,:]
 * The map a is not stored: lse [B][P] keeps the log-sum-exp of every pixel's scores, and the backward
 * recomputes a from Q and Kr.  Keys and values are staged in LDS in chunks of classes with a running
 * max / sum, so K is bounded by GS_OCR_MAX_CLASSES only. */
typedef struct gs_ocr_attend_desc {
  int32_t B, P, K, ch;               /* images, pixels per image, regions, ACTIVE width           */
  int32_t ldq, ldk, ldv, ldo;        /* pitches of Q, Kr, V and out                               */
  int32_t lddq, lddk, lddv, lddo;    /* pitches of dQ, dKr, dV and dout (all eight always checked) */
} gs_ocr_attend_desc;
int gs_ocr_attend_forward(const gs_ocr_attend_desc* d, const float* q, const float* k, const float* v, float* out,
                          float* lse, void* stream);
/* bytes of scratch the backward needs (0 for a descriptor it would refuse): a and ds of every pixel, and
 * one [K][ch] partial per run of 128 rows. */
size_t gs_ocr_attend_workspace_bytes(const gs_ocr_attend_desc* d);
/* With da[b,p,k] = <dout[b,p,:], V[b,k,:]> and ds = a * (da - <dout[b,p,:], out[b,p,:]>):
 *   dq[b,p,:] = ch^-0.5 * sum_k ds * Kr[b,k,:],   dk[b,k,:] = ch^-0.5 * sum_p ds * Q[b,p,:],
 *   dv[b,k,:] = sum_p a * dout[b,p,:].   All three are overwritten. */
int gs_ocr_attend_backward(const gs_ocr_attend_desc* d, const float* q, const float* k, const float* v,
                           const float* out, const float* lse, const float* dout, float* dq, float* dk, float* dv,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Dynamic BatchNorm (+ residual add, + ReLU) — K4, K8                                         */
/* ------------------------------------------------------------------------------------------ */
/* Replaces F.batch_norm on the leading C-slice of max-size parameters (gaiavision DynBN /
 * DynSyncBN; call sites dynamic_resnet.py:267-300,411,
 * dynamic_res_layer.py:92, DynamicBottleneck norm1-3, DynamicConvModule norm) fused with the
 * following nn.ReLU(inplace=True) and the bottleneck's `out += identity`.
 *
 * Training forward is three launches:
 *   gs_bn_stats     : per-channel shifted sums  S1 = sum(x - x[0,c]),  S2 = sum (x - x[0,c])^2
 *                     reduced in a fixed order (deterministic) into sums[2*C]
 *   (optional all-reduce of sums[] + count across ranks for SyncBN — done by the host)
 *   gs_bn_finalize  : mean/var -> coeffs {scale = gamma*invstd, beta, mean, invstd}; updates
 *                     running_mean/var (momentum, unbiased var)
 *   gs_bn_apply     : y = relu?((x - mean)*scale + beta (+ residual))
 */
size_t gs_bn_stats_workspace_bytes(int64_t rows, int32_t C);
/* sums: [3*C] floats = {S1[C], S2[C], shift[C]} (shift = x[0,c], the conditioning offset). */
int gs_bn_stats(const float* x, int64_t rows, int32_t C, int32_t ldx, float* sums,
                void* workspace, size_t workspace_bytes, void* stream);
/* count = number of samples per channel that produced sums (N*H*W, or the global count for SyncBN).
 * coeffs: [4*C] = {scale[C], beta[C], mean[C], invstd[C]}.  running_* may be NULL (no update).
 * gamma/beta may be NULL (treated as 1/0). */
int gs_bn_finalize(const float* sums, double count, int32_t C, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean,
                   float* running_var, float* coeffs, void* stream);
/* SyncBN exchange (torch.nn.SyncBatchNorm's all_gather of [mean, var, count]; heads
 * with norm_cfg SyncBN): gs_bn_sync_local turns the shifted sums of gs_bn_stats into this rank's
 * payload local[2C+1] = {mean[C], biased var[C], count} (double); after the host's all_gather into
 * gathered[world][2C+1], gs_bn_sync_merge produces the merged sums {0, gvar*total, gmean}[3C] that
 * gs_bn_finalize takes (count = total).  One launch each. */
int gs_bn_sync_local(const float* sums, double count, int32_t C, double* local, void* stream);
int gs_bn_sync_merge(const double* gathered, int32_t world, int32_t C, float* merged, void* stream);
/* gs_bn_stats + gs_bn_finalize in two launches instead of three, for rank-local statistics
 * (count = rows).  Bit-identical to the separate calls. */
int gs_bn_stats_finalize(const float* x, int64_t rows, int32_t C, int32_t ldx, const float* gamma,
                         const float* beta, float eps, float momentum, float* running_mean,
                         float* running_var, float* coeffs, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Eval-mode coefficients from running statistics (norm_eval / inference). coeffs as above. */
int gs_bn_eval_coeffs(const float* running_mean, const float* running_var, int32_t C,
                      const float* gamma, const float* beta, float eps, float* coeffs,
                      void* stream);
/* y = act((x - mean)*scale + beta + residual).  residual may be NULL; relu != 0 applies max(.,0).
 * x and y may alias (in-place).  */
int gs_bn_apply(const float* x, int64_t rows, int32_t C, int32_t ldx, const float* coeffs,
                const float* residual, int32_t ld_res, int32_t relu, float* y, int32_t ldy,
                void* stream);
/* gs_bn_apply with ReLU that also writes the mask bytes mask[rows][C/4] (bit e of byte q set <=>
 * y[r][4q+e] > 0), see gs_bn_args::relu_mask. */
int gs_bn_apply_mask(const float* x, int64_t rows, int32_t C, int32_t ldx, const float* coeffs,
                     const float* residual, int32_t ld_res, float* y, int32_t ldy, uint8_t* mask,
                     void* stream);

/* Backward.  mask_mode: 0 = none; 1 = ReLU directly after this BN (mask recomputed from
 * (x-mean)*scale+beta > 0); 2 = mask from a saved post-activation tensor `act` (> 0), used for the
 * bottleneck output relu(out + identity) where `act` is the block output.
 *   gs_bn_bwd_reduce : sums[2*C] = { sum g , sum g*xhat }, g = dy * mask.  If g_out != NULL the
 *                      masked gradient g is also written there (may alias dy): it is the gradient
 *                      of the identity branch.
 *   gs_bn_bwd_apply  : dx = scale * (g - sum_g/count - xhat * sum_gx/count)   (training stats)
 *                      or dx = scale * g when use_batch_stats == 0 (eval-mode BN in training).
 *                      Also writes dgamma[:C] = sum_gx, dbeta[:C] = sum_g when non-NULL. */
size_t gs_bn_bwd_workspace_bytes(int64_t rows, int32_t C);
int gs_bn_bwd_reduce(const float* dy, int32_t ld_dy, const float* x, int32_t ldx,
                     const float* act, int32_t ld_act, int64_t rows, int32_t C,
                     const float* coeffs, int32_t mask_mode, float* g_out, int32_t ld_g,
                     float* sums, void* workspace, size_t workspace_bytes, void* stream);
int gs_bn_bwd_apply(const float* dy, int32_t ld_dy, const float* x, int32_t ldx,
                    const float* act, int32_t ld_act, int64_t rows, int32_t C,
                    const float* coeffs, const float* sums, double count, int32_t mask_mode,
                    int32_t use_batch_stats, float* dx, int32_t ld_dx, float* dgamma,
                    float* dbeta, void* stream);

/* Per-subnet BatchNorm re-calibration (core/bn_calibration.py): one table-driven launch that
 * moves the leading `channels` running statistics of every listed BatchNorm between its buffers
 * and a flat fp32 bank, layer i at bank[offset_i .. offset_i + 2*channels_i) = [mean[c] | var[c]].
 *   GS_BN_CALIB_SAVE  : bank  = running            (snapshot; first batch of an accumulation)
 *   GS_BN_CALIB_ADD   : bank += running            (further batches; momentum-1 forwards leave
 *                                                   the batch's own statistics in the buffers)
 *   GS_BN_CALIB_WRITE : running = bank * scale     (scale 1/K commits the average of K batches,
 *                                                   scale 1 from a SAVE bank restores bit for bit)
 * `scale` is read by WRITE only, which multiplies (it never divides).  One fp32 operation per
 * element in a fixed order: results are bit-reproducible.  `layers` and `bank` are device memory;
 * channels beyond a layer's `channels` and bank floats outside the layers' ranges are never
 * touched.  GS_E_NULL (layers or bank) / GS_E_BADARG (n_layers <= 0, bank_floats <= 0, op outside
 * 0..2) before any launch.  An entry with channels < 0, offset < 0, offset + 2*channels >
 * bank_floats or a null buffer pointer is skipped by the kernel, not followed. */
typedef struct GsBnCalibLayer {
  float* running_mean; /* device pointers of one BatchNorm's buffers */
  float* running_var;
  int32_t channels;    /* active leading channels c */
  int32_t offset;      /* first float of this layer's [mean[c] | var[c]] in the bank */
} GsBnCalibLayer;
#define GS_BN_CALIB_SAVE 0
#define GS_BN_CALIB_ADD 1
#define GS_BN_CALIB_WRITE 2
int gs_bn_calib_fold(const GsBnCalibLayer* layers, int32_t n_layers, float* bank,
                     int64_t bank_floats, int32_t op, float scale, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* conv -> BatchNorm (+ residual) (+ ReLU) issued by ONE host call per direction               */
/* ------------------------------------------------------------------------------------------ */
/* Replaces the module chain conv -> norm -> activate of gaiavision DynamicConvModule and of each
 * conv/bn pair of DynamicBottleneck (gaiaseg/models/utils/dynamic_res_layer.py:84-125,
 * gaiaseg/models/backbones/dynamic_resnet.py:255-302, decode heads' ConvModules) for rank-local
 * BatchNorm.  Same kernels as gs_conv2d_*, gs_bn_* and gs_stream_fork; it exists because one host
 * call per module costs as much host time as the kernels cost GPU time on this path, and because
 * the batch statistics can then come from the conv itself: without split-K the conv epilogue writes
 * per-tile partial sums that are merged exactly (Chan et al., double, fixed order — equal to
 * gs_bn_stats up to rounding); with split-K one kernel sums the slabs, stores y and accumulates the
 * statistics (bit-identical to gs_conv2d_forward + gs_bn_stats_finalize).  Backward is a pure
 * composition.  workspace must be >= gs_conv_bn_workspace_bytes(d). */
typedef struct gs_bn_args {
  const float* gamma;        /* [>= C] or NULL (1)                                              */
  const float* beta;         /* [>= C] or NULL (0)                                              */
  float* running_mean;       /* [>= C] or NULL                                                  */
  float* running_var;        /* [>= C] or NULL                                                  */
  float eps, momentum;
  int32_t use_batch_stats;   /* 1: statistics of this batch (training); 0: running statistics   */
  int32_t update_running;    /* 1: update running_mean / running_var (training mode)            */
  int32_t relu;              /* ReLU after the BN (+ residual)                                  */
  int32_t reserved;          /* must be 0                                                       */
  uint8_t* relu_mask;        /* forward, relu != 0, z != NULL: if not NULL the apply pass also
                                writes the ReLU mask [rows][Co/4], one byte per channel quad
                                (bit e set <=> z[.., 4q+e] > 0) -- 1/16 of z, for the consumer's
                                fused BatchNorm-backward epilogue (gs_bn_bwd_fuse mode 3)          */
  const float* residual_coeffs; /* forward, residual != NULL: if not NULL, `residual` is the RAW
                                output of another conv (the projection shortcut of a stage's first
                                block, gaiaseg/models/utils/dynamic_res_layer.py:70-94) and these
                                are that conv's BatchNorm coefficients [scale | beta | mean | ..][C]
                                (layout of `coeffs`): the apply pass adds
                                (residual - mean) * scale + beta, so the shortcut's normalised
                                output is never written or read                                     */
} gs_bn_args;
/* max(gs_conv2d_workspace_bytes, gs_bn_stats_workspace_bytes) for this conv's output */
size_t gs_conv_bn_workspace_bytes(const gs_conv_desc* d);
/* y = conv(x, w) [N*Ho*Wo][ldy] (kept for backward); coeffs[4*Co] (kept for backward);
 * z = relu?(BN(y) (+ residual)) with pixel stride ldz.  The conv has no bias (norm follows).
 * z == NULL (residual must be NULL): only y and coeffs are produced; the consumer evaluates
 * relu(BN(y)) in its operand loader (gs_conv_desc::in_affine = coeffs).  d->in_affine of THIS conv is
 * honoured in forward and in the weight gradient of gs_conv_bn_backward. */
int gs_conv_bn_forward(const gs_conv_desc* d, const float* x, const float* w, const gs_bn_args* bn,
                       const float* residual, int32_t ld_res, float* y, float* coeffs, float* z,
                       int32_t ldz, void* workspace, size_t workspace_bytes, void* stream);
/* dz: gradient of z (in/out: overwritten with the masked gradient when write_g != 0 — that is the
 * gradient of the identity branch of a bottleneck); mask_mode as gs_bn_bwd_reduce (z is the saved
 * post-activation tensor for mode 2).  dy: scratch [N*Ho*Wo][ldy] receiving the gradient of the conv
 * output; bsums: scratch [2*Co].  dgamma/dbeta/dw/dx may be NULL (not needed).  side_stream != NULL
 * runs the weight gradient there (forked after dy is complete; the caller joins it later with
 * gs_stream_fork(side_stream, stream)) using side_workspace.
 *
 * Cross-layer fusion of the BatchNorm backward reduction (the bn_bwd_partial pass over dz and y):
 *   input_bn != NULL: x is the output of relu(bn_prev(y_prev) [+ residual]) and this call's data
 *     gradient is the LAST contribution to its gradient (accumulate_dx included).  Where the dgrad
 *     kernel allows it (stride 1, no split-K, fast path) its epilogue masks the gradient with that
 *     ReLU's mask, stores the masked gradient g into dx and reduces {sum g, sum g * xhat_prev} into
 *     input_bn->sums; *input_bn->fused is set to 1 (else 0 and dx holds the plain gradient).
 *   sums_ready != 0: THIS layer's dz already is the masked gradient and bsums already holds its
 *     sums (a consumer's call did the above): the reduction pass is skipped, mask_mode is ignored. */
typedef struct gs_bn_bwd_fuse {
  const float* y;        /* bn_prev's input [rows][ldy]                                         */
  const float* act;      /* mode 2: bn_prev's post-activation output [rows][ldact], else NULL   */
  const float* coeffs;   /* bn_prev's coefficient block [scale | beta | mean | invstd][Ci]      */
  float* sums;           /* out: [2*Ci] = {sum g, sum g * xhat}                                  */
  int32_t* fused;        /* out (host): 1 if the fused epilogue ran                             */
  int32_t ldy, ldact;
  int32_t mode;          /* 1: mask = bn_prev(y) > 0 ; 2: mask = act > 0 ; 3: mask bits (below)  */
  int32_t reserved;
  const uint8_t* mask;   /* mode 3: gs_bn_args::relu_mask of bn_prev's forward [rows][ldmask]:
                            the same mask as mode 2 without reading the activation again         */
  int32_t ldmask;        /* bytes per pixel row, >= Ci / 4                                       */
  int32_t reserved2;     /* must be 0                                                            */
} gs_bn_bwd_fuse;
int gs_conv_bn_backward(const gs_conv_desc* d, const float* x, const float* w, const float* y,
                        const float* z, int32_t ldz, const float* coeffs, const gs_bn_args* bn,
                        float* dz, int32_t ld_dz, int32_t mask_mode, int32_t write_g, float* dy,
                        float* bsums, float* dgamma, float* dbeta, float* dw, float* dx,
                        int32_t accumulate_dx, void* workspace, size_t workspace_bytes,
                        void* side_workspace, size_t side_workspace_bytes, void* stream,
                        void* side_stream, const gs_bn_bwd_fuse* input_bn, int32_t sums_ready);

/* Live timer of the forward launches with role GS_CONV_ROLE_BOTTLENECK3X3: bench.py's `roofline`.
 * One pair of HIP events per op on the launch stream.  Where the op is ONE kernel (unsplit, or split-K
 * combined inside the launch: the default) the pair is attached to that kernel's own dispatch
 * (hipExtLaunchKernelGGL start / stop events: the dispatch's begin / end timestamps, what a rocprofv3
 * kernel trace reports); where a reduce launch follows, or with GS_K3_TIMER_MARKERS set, the events are
 * markers recorded in front of the conv and behind the last launch (2-3 us more per op).
 * enable(1) resets and starts, enable(0) stops; read after a device synchronize. */
int gs_k3_timer_enable(int32_t on);
int gs_k3_timer_read(int64_t* launches, double* total_ms, double* total_flops);

/* ------------------------------------------------------------------------------------------ */
/* Pooling — K5, K7                                                                            */
/* ------------------------------------------------------------------------------------------ */
/* nn.AvgPool2d(kernel_size=s, stride=s, ceil_mode=True, count_include_pad=False): the shortcut
 * pooling of avg_down=True (gaiaseg/models/utils/dynamic_res_layer.py:75-82).  Output size
 * ceil(H/s) x ceil(W/s); border windows average their in-bounds pixels only.
 * backward: dx[n,h,w,:] (+)= dy[n,h/s,w/s,:] / count(window). */
int gs_avgpool_ceil_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldx,
                            int32_t s, float* y, int32_t ldy, void* stream);
int gs_avgpool_ceil_backward(const float* dy, int32_t ld_dy, int32_t N, int32_t H, int32_t W,
                             int32_t C, int32_t s, float* dx, int32_t ld_dx, int32_t accumulate,
                             void* stream);
/* nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (dynamic_resnet.py:302,413), generic k/s/p.
 * idx (uint8 tap index of the first maximum in (kh,kw) scan order, as ATen) is saved for bwd. */
int gs_maxpool_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldx,
                       int32_t k, int32_t s, int32_t p, int32_t Ho, int32_t Wo, float* y,
                       int32_t ldy, uint8_t* idx, void* stream);
/* dx (= or += when accumulate) gather of dy through idx.  */
int gs_maxpool_backward(const float* dy, int32_t ld_dy, const uint8_t* idx, int32_t N, int32_t H,
                        int32_t W, int32_t C, int32_t k, int32_t s, int32_t p, int32_t Ho,
                        int32_t Wo, float* dx, int32_t ld_dx, int32_t accumulate, void* stream);

/* nn.AdaptiveAvgPool2d(s) for all pool_scales of DynamicPPM in ONE read of x
 * (dynamic_psp_head.py:48-51).  scales[nscales] (e.g. {1,2,3,6}); y is the concatenation over
 * scales of [N][s][s][C] blocks (pixel stride C).  Bin edges floor(i*H/s), ceil((i+1)*H/s). */
size_t gs_adaptive_avgpool_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C,
                                           const int32_t* scales, int32_t nscales);
int gs_adaptive_avgpool_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t C,
                                int32_t ldx, const int32_t* scales, int32_t nscales, float* y,
                                void* workspace, size_t workspace_bytes, void* stream);
/* dx (= or +=) sum over scales of dy_bin / bin_area for every bin containing the pixel. */
int gs_adaptive_avgpool_backward(const float* dy, int32_t N, int32_t H, int32_t W, int32_t C,
                                 const int32_t* scales, int32_t nscales, float* dx, int32_t ld_dx,
                                 int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Bilinear resize (align_corners False/True) — K9, K15, K16, K17                              */
/* ------------------------------------------------------------------------------------------ */
/* mmseg.ops.resize == F.interpolate(mode='bilinear') (dynamic_psp_head.py:67-71,
 * dynamic_uper_head.py:108-112,123-127).  Writes into a channel slice of a wider buffer (ldy) so
 * that torch.cat never materialises (PPM / FPN concat fusion); accumulate != 0 gives the UPer
 * top-down `laterals[i-1] += resize(laterals[i])` in one pass. */
int gs_bilinear_forward(const float* x, int32_t N, int32_t Hi, int32_t Wi, int32_t C, int32_t ldx,
                        int32_t Ho, int32_t Wo, int32_t align_corners, float* y, int32_t ldy,
                        int32_t accumulate, void* stream);
/* Adjoint (deterministic gather form): dx (= or +=) sum_p w_p * dy_p.  Large footprints (small
 * source maps) are split over destination-row slices into the workspace and summed in order. */
size_t gs_bilinear_backward_workspace_bytes(int32_t N, int32_t Hi, int32_t Wi, int32_t C,
                                            int32_t Ho, int32_t Wo);
int gs_bilinear_backward(const float* dy, int32_t ld_dy, int32_t N, int32_t Hi, int32_t Wi,
                         int32_t C, int32_t Ho, int32_t Wo, int32_t align_corners, float* dx,
                         int32_t ld_dx, int32_t accumulate, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Elementwise helpers                                                                         */
/* ------------------------------------------------------------------------------------------ */
/* dst[r, :C] (= or +=) src[r, :C] * alpha for strided 2-D views (concat slices, grad accumulation). */
int gs_copy2d(const float* src, int32_t ld_src, float* dst, int32_t ld_dst, int64_t rows,
              int32_t C, float alpha, int32_t accumulate, void* stream);
/* nn.Dropout2d (fcn_head.py:248-253): y[n,p,c] = x[n,p,c] * mask[n*C + c]; mask already holds
 * keep/(1-p).  Same kernel is its own backward.  x, y may alias. */
int gs_scale_nc(const float* x, int32_t ldx, const float* mask, int32_t N, int64_t pixels_per_image,
                int32_t C, float* y, int32_t ldy, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Pixel-wise cross entropy with on-the-fly bilinear upsampling — K13, K14                     */
/* ------------------------------------------------------------------------------------------ */
/* Replaces resize(seg_logit -> label size) + F.cross_entropy(reduction='none', ignore_index) +
 * weight_reduce_loss(mean over ALL pixels) + accuracy(top-1)
 * (gaiaseg/models/decode_heads/dynamic_fcn_head.py:137-159; spec copies
 *  gaiaseg/models/losses/cross_entropy_loss.py:81-92, utils.py:26-55, accuracy.py:38-49).
 * logits: [N,h,w,Cls] through element strides (l_sn,l_sh,l_sw,l_sc); labels int64 [N,H,W].
 * pixel_weight: optional float [N,H,W] (OHEM sampler weights), class_weight optional [Cls].
 * out[0] = sum_i w_i * ce_i (host divides by N*H*W and multiplies loss_weight),
 * out[1] = number of pixels whose argmax == label.     (both accumulated in double, fixed order)
 * The full-resolution logits are never materialised. */
typedef struct gs_ce_desc {
  int32_t N, h, w, Cls;      /* logits                                                        */
  int32_t H, W;              /* label / loss resolution                                       */
  int64_t l_sn, l_sh, l_sw, l_sc;
  int32_t ignore_index;
  int32_t align_corners;
} gs_ce_desc;
size_t gs_ce_workspace_bytes(const gs_ce_desc* d);
/* lse: optional float [N,H,W]; when non-NULL the per-pixel log-sum-exp of the resized logits is
 * saved there for gs_ce_backward (which requires it). */
int gs_ce_forward(const gs_ce_desc* d, const float* logits, const int64_t* labels,
                  const float* pixel_weight, const float* class_weight, float* lse, double* out,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Same, with the host-side epilogue of `losses` folded in: out2[0] = float(out[0]) * loss_scale
 * (= loss_weight / (N*H*W)), out2[1] = float(out[1]) * acc_scale (= 100 / (N*H*W)), both fp32 —
 * dynamic_fcn_head.py:149-159 computes exactly these two scalars. */
int gs_ce_forward_scaled(const gs_ce_desc* d, const float* logits, const int64_t* labels,
                         const float* pixel_weight, const float* class_weight, float* lse,
                         float loss_scale, float acc_scale, float* out2, void* workspace,
                         size_t workspace_bytes, void* stream);
/* dlogits[n,y,x,c] = grad_scale * sum_p bilinear_w(p->(y,x)) * w_p * cw * (softmax_p[c] - [c==label_p])
 * written densely (pixel stride ld_d, columns Cls..ld_d-1 zeroed).  Deterministic gather form:
 * one workgroup per low-resolution logit pixel walks its bilinear footprint. */
int gs_ce_backward(const gs_ce_desc* d, const float* logits, const int64_t* labels,
                   const float* pixel_weight, const float* class_weight, const float* lse,
                   float grad_scale, float* dlogits, int32_t ld_d, void* stream);
/* Same result through the tile form when the up-scaling is a power-of-two integer factor with
 * align_corners = 0 (every mmseg head of this path: x8 / x16 / x32): one workgroup per tile of
 * full-resolution pixels between four low-resolution logit pixels evaluates each softmax term once
 * (the gather form of gs_ce_backward evaluates it once per neighbour, i.e. four times), then a
 * fixed-order gather adds the four corner sums per low-resolution pixel.  Any OTHER up-scaling of at
 * most 64 full-resolution pixels per tile on average (config 4's 193 -> 769, align_corners either way)
 * takes the row-tile form (r04): the same tiles, bounds found with the resize's own source-index
 * arithmetic, one 16-lane DPP row per tile.  Falls back to gs_ce_backward otherwise (larger
 * non-power-of-two ratios, down-scaling).  workspace >= gs_ce_backward_workspace_bytes(d, ld_d), which
 * is 0 exactly when the gather form will be used. */
size_t gs_ce_backward_workspace_bytes(const gs_ce_desc* d, int32_t ld_d);
int gs_ce_backward_ws(const gs_ce_desc* d, const float* logits, const int64_t* labels,
                      const float* pixel_weight, const float* class_weight, const float* lse,
                      float grad_scale, float* dlogits, int32_t ld_d, void* workspace,
                      size_t workspace_bytes, void* stream);
/* OHEMPixelSampler support: prob[n,Y,X] = softmax(resized logit)[label]
 * for valid pixels, 2.0 for ignored ones (so they sort last). */
int gs_ce_label_prob(const gs_ce_desc* d, const float* logits, const int64_t* labels, float* prob,
                     void* stream);

/* OHEMPixelSampler.sample (mmseg): from the label probabilities written by
 * gs_ce_label_prob, weight[i] = 1 for the hard valid pixels, else 0.
 *   use_thresh != 0 : threshold = max(thresh, sorted_valid_prob[min(batch_kept, n_valid-1)]),
 *                     keep prob < threshold          (OHEM with `thresh`)
 *   use_thresh == 0 : keep the batch_kept valid pixels of smallest probability (= largest loss)
 * The rank statistic is an exact 3-pass radix select (integer atomics only; reproducible). */
size_t gs_ohem_workspace_bytes(void);
int gs_ohem_weights(const float* prob, int64_t n, int64_t batch_kept, float thresh,
                    int32_t use_thresh, float* weight, void* workspace, size_t workspace_bytes,
                    void* stream);

/* ------------------------------------------------------------------------------------------ */
/* In-place distillation (sandwich rule) — the student members' loss                           */
/* ------------------------------------------------------------------------------------------ */
/* The distillation branch of the decode heads' forward_train (gaiaseg/models/decode_heads/
 * dynamic_psp_head.py:176-245, dynamic_fcn_head.py:161-231), fed by the MAX subnet's logits
 * (train_step of dynamic_encoder_decoder-distill-backup (1).py:52-64, tools/train_supernet.py:180-187):
 *   out[0] = scale * sum_{n,c,Y,X} -softmax(t/T)[c] * log softmax(s/T)[c]
 * with the host's scale = distillation_weight / (N * D) (D = 1000 for the PSP head, 2000 for the FCN
 * head): the reference's (-bmm(student_score.log(), teacher_score)).mean() / D, a sum over classes and
 * pixels and a mean over the batch; labels do not enter it.  log softmax is s/T - lse(s/T), finite
 * where the reference's log(softmax) is not.  Student and teacher share N, h, w, Cls and have their
 * own element strides.  interpolation = 1: both are bilinearly resized to (H, W) (align_corners as
 * given) on the fly; interpolation = 0: the loss is taken at logit resolution and (H, W) must equal
 * (h, w).  Per-pixel losses are summed in double in a fixed order (bit-reproducible). */
typedef struct gs_kd_desc {
  int32_t N, h, w, Cls;        /* logits, both tensors                                          */
  int32_t H, W;                /* evaluation grid: the label size, or (h, w) without interpolation */
  int64_t s_sn, s_sh, s_sw, s_sc;   /* student strides (elements)                               */
  int64_t t_sn, t_sh, t_sw, t_sc;   /* teacher strides                                          */
  float T;                     /* temperature (> 0)                                             */
  int32_t align_corners;
  int32_t interpolation;
  int32_t reserved;
} gs_kd_desc;
size_t gs_kd_workspace_bytes(const gs_kd_desc* d);
/* lse_s / lse_t: optional float [N,H,W]; when non-NULL the per-pixel log-sum-exp of s/T and t/T is
 * saved there for gs_kd_backward (which requires both).  out: one float. */
int gs_kd_forward(const gs_kd_desc* d, const float* student, const float* teacher, float* lse_s,
                  float* lse_t, float scale, float* out, void* workspace, size_t workspace_bytes,
                  void* stream);
/* ds[n,y,x,c] = adjoint of the resize of grad_scale / T * (softmax(s/T) - softmax(t/T)), written
 * densely (pixel stride ld_d, columns Cls..ld_d-1 zeroed); the teacher receives no gradient.  With
 * interpolation and workspace >= gs_kd_backward_workspace_bytes(d, ld_d) the tile form runs (every
 * term evaluated once, then a fixed-order gather of four corner sums per logit pixel); with a smaller
 * workspace the gather form (one workgroup per logit pixel).  The workspace size is 0 without
 * interpolation (pointwise). */
size_t gs_kd_backward_workspace_bytes(const gs_kd_desc* d, int32_t ld_d);
int gs_kd_backward(const gs_kd_desc* d, const float* student, const float* teacher,
                   const float* lse_s, const float* lse_t, float grad_scale, float* ds, int32_t ld_d,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Fixed-teacher distillation (DynamicDistiller) — the logit loss and the pairwise loss        */
/* ------------------------------------------------------------------------------------------ */
/* distill_loss of gaiaseg/models/segmentors/dynamic_distiller.py:341-356,397-403: both low-resolution
 * logit maps are bilinearly resized to the image size (H, W) with the STUDENT's align_corners, then
 *   out[0] = scale * sum_{n,c,Y,X} -softmax(t'/T)[c] * log softmax(s'/T)[c]
 * with the host's scale = distill_loss_weight / (N * H * W) (no T^2 factor).  gs_kd_desc with the
 * teacher at a resolution of its own: (hs, ws) and (ht, wt) are independent (an OS8 teacher over an
 * OS32 student, or the reverse).  Neither resized map is materialised.  The contract of every entry is
 * that of its gs_kd_* namesake (lse of both maps saved at [N,H,W]; double fixed-order sums; ds dense
 * at pixel stride ld_d with zeroed pad columns; tile form with a workspace of
 * gs_distill_backward_workspace_bytes, gather form with less); the device code is shared, and at
 * (ht, wt) == (hs, ws) the results equal gs_kd_forward / gs_kd_backward with interpolation = 1 bit
 * for bit. */
typedef struct gs_distill_desc {
  int32_t N, Cls;
  int32_t hs, ws;              /* student logits                                                 */
  int32_t ht, wt;              /* teacher logits                                                 */
  int32_t H, W;                /* evaluation grid: the image size                                */
  int64_t s_sn, s_sh, s_sw, s_sc;   /* student strides (elements)                               */
  int64_t t_sn, t_sh, t_sw, t_sc;   /* teacher strides                                          */
  float T;                     /* temperature (> 0)                                             */
  int32_t align_corners;
} gs_distill_desc;
size_t gs_distill_workspace_bytes(const gs_distill_desc* d);
int gs_distill_forward(const gs_distill_desc* d, const float* student, const float* teacher,
                       float* lse_s, float* lse_t, float scale, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t gs_distill_backward_workspace_bytes(const gs_distill_desc* d, int32_t ld_d);
int gs_distill_backward(const gs_distill_desc* d, const float* student, const float* teacher,
                        const float* lse_s, const float* lse_t, float grad_scale, float* ds,
                        int32_t ld_d, void* workspace, size_t workspace_bytes, void* stream);

/* pairwise_loss of dynamic_distiller.py:309-339 on a window of the last backbone feature maps.  The
 * window pixels rows y0..y1-1, columns x0..x1-1 are taken row-major, P = (y1 - y0) * (x1 - x0); the
 * host passes the reference's slice as written, one column (x1 = x0 + 1).  Each pixel's channel vector
 * is L2-normalised (denominator max(norm, 1e-12), F.normalize), G_s and G_t are the P x P Gram
 * matrices of the normalised student and teacher vectors, and
 *   out[0] = scale * -sum_{n,i,j} softmax(G_t/T, over i)[n,i,j] * log_softmax(G_s/T, over j)[n,i,j]
 * (the reference's dim=1 / dim=2) with the host's scale = pairwise_loss_weight / (N * step_h * step_w).
 * Student and teacher have their own channel counts, map sizes (the window must lie inside both) and
 * element strides.  P above GS_PAIRWISE_MAX_P returns GS_E_BADARG before any launch.
 * forward: 3 launches (raw Gram tiles of both maps; per-image normalise + softmaxes + loss; final
 * sum), backward: 3 launches (zero fill; gradient coefficients; coefficients x window).  None grows
 * with N, P or C; no host synchronisation; fp32 sums in a fixed order, the final sum in double, no
 * float atomics: bit-reproducible.  A channels-last map (c stride 1, other strides and the base
 * address multiples of 4 floats) is read as float4s with a scalar tail; any other layout by scalars.
 * `save`: gs_pairwise_save_bytes(d) bytes, 8-byte aligned, written by the forward and read (and used
 * as scratch) by the backward. */
#define GS_PAIRWISE_MAX_P 128
typedef struct gs_pairwise_desc {
  int32_t N, Cs, Ct;
  int32_t H, W;                /* student map                                                    */
  int32_t Ht, Wt;              /* teacher map                                                    */
  int32_t y0, y1, x0, x1;      /* window, in both maps                                           */
  int32_t reserved;
  int64_t s_sn, s_sc, s_sh, s_sw;   /* student strides (elements)                               */
  int64_t t_sn, t_sc, t_sh, t_sw;   /* teacher strides                                          */
  float T;                     /* temperature (> 0)                                             */
  int32_t reserved2;
} gs_pairwise_desc;
size_t gs_pairwise_save_bytes(const gs_pairwise_desc* d);
int gs_pairwise_forward(const gs_pairwise_desc* d, const float* student, const float* teacher,
                        float scale, float* out, void* save, size_t save_bytes, void* stream);
/* ds[n,y,x,c]: the gradient of out[0] * grad_scale / scale with respect to the student map, dense at
 * pixel stride ld_d (>= Cs, a multiple of 4; columns Cs..ld_d-1 zeroed), zero outside the window; the
 * chain log-softmax -> Gram -> normalise includes the eps clamp (a pixel whose norm is below 1e-12
 * gets g / 1e-12 as autograd does: finite).  The teacher receives no gradient. */
int gs_pairwise_backward(const gs_pairwise_desc* d, const float* student, void* save,
                         size_t save_bytes, float grad_scale, float* ds, int32_t ld_d, void* stream);

/* Channel-wise distillation (Shu et al., ICCV 2021; mmrazor's ChannelWiseDivergence) of two logit maps
 * of one shape [N, C, H, W], each with element strides of its own.  With phi(x)[n,c,:] the softmax of
 * x[n,c,:] / T over the P = H * W PIXELS of one class map,
 *   out[0] = scale * T^2 * sum_{n,c} sum_p phi(t) * (log phi(t) - log phi(s))
 * with the host's scale = weight / (N * C).  One pass: every logit is read once, no [N, C, H, W]
 * temporary is written.  A column (n, c) is five running numbers (the two maxima, Z_s, Z_t and
 * A = sum e_t (t - s) / T; KL = A / Z_t + (m_s - m_t) / T + log Z_s - log Z_t) whose partial states
 * combine associatively; a map is split over gs_cwd_debug_partials(d) workgroups by pixel range, a
 * second launch (one wave per class map) rescales the partials to the map's maxima and sums them in
 * double in a fixed order, and a third sums the N * C column losses in double in a fixed order:
 * bit-reproducible, no float atomics.  The split depends on the descriptor alone.  Channels-last maps
 * (c stride 1; the other strides and the base addresses multiples of 4 floats) are read as float4s,
 * the partial last quad by scalars: the pad columns C .. ld-1 are never read.  Any other layout is
 * read by scalars.
 * lse_s / lse_t: float [N, C], written by the forward: m / T + log Z of each class map.
 * workspace: gs_cwd_workspace_bytes(d) bytes, 8-byte aligned (GS_E_WORKSPACE when smaller).
 * GS_E_NULL / GS_E_BADARG (a size <= 0, N > 65535, T <= 0 or infinite) before any launch. */
typedef struct gs_cwd_desc {
  int32_t N, C, H, W;
  int64_t s_sn, s_sc, s_sh, s_sw;   /* student strides (elements)                               */
  int64_t t_sn, t_sc, t_sh, t_sw;   /* teacher strides                                          */
  float T;                     /* temperature (> 0)                                             */
  int32_t reserved;
} gs_cwd_desc;
size_t gs_cwd_workspace_bytes(const gs_cwd_desc* d);
int gs_cwd_forward(const gs_cwd_desc* d, const float* student, const float* teacher, float* lse_s,
                   float* lse_t, float scale, float* out, void* workspace, size_t workspace_bytes,
                   void* stream);
/* ds[n,y,x,c] = scale * T * (exp(s / T - lse_s[n,c]) - exp(t / T - lse_t[n,c])), elementwise, written
 * densely at pixel stride ld_d (>= C; columns C..ld_d-1 zeroed).  The teacher receives no gradient. */
int gs_cwd_backward(const gs_cwd_desc* d, const float* student, const float* teacher,
                    const float* lse_s, const float* lse_t, float scale, float* ds, int32_t ld_d,
                    void* stream);
/* The number of pixel ranges (workgroups) one class map is split into for d's sizes and strides
 * (>= 1; host arithmetic, no device needed), or a negative GS_E_* for a bad descriptor. */
int gs_cwd_debug_partials(const gs_cwd_desc* d);

/* ------------------------------------------------------------------------------------------ */
/* Inference epilogue — K17                                                                    */
/* ------------------------------------------------------------------------------------------ */
/* argmax over classes of bilinearly resized logits (softmax is monotone):
 * seg[n,Y,X] = argmax_c resize(logits)[n,c,Y,X]  (dynamic_distiller.py:461-521 whole_inference +
 * simple_test).  If probs != NULL also writes softmax probabilities [N,H,W,Cls] (aug_test). */
int gs_resize_argmax(const gs_ce_desc* d, const float* logits, int64_t* seg, float* probs,
                     void* stream);

/* Whole-image and sliding-window test mode as ONE gather kernel
 * (dynamic_distiller.py:416-459 slide_inference, :461-473 whole_inference, :475-508 inference,
 * :510-540 simple_test / aug_test).  The reference accumulates every window's up-sampled logits
 * into a [N,C,H,W] tensor (159 MB at 1024x2048), counts, divides, resizes to ori_shape, applies
 * softmax, flips and takes the argmax in separate passes.  Here the low-resolution logits of all
 * windows stay resident and each output pixel gathers them: nothing of size C*H*W exists unless
 * the caller asks for the probabilities.
 *   logits : [ny*nx][N][hl][wl][ld] fp32 (NHWC per window, window index row-major, ld % 4 == 0,
 *            ld >= C): the decode head's output for every window of hc x wc image pixels
 *   win_y / win_x : HOST arrays of the ny window-row / nx window-column origins (<= 64 each); the
 *            window list is their product.  Whole mode: ny = nx = 1, origin 0, hc = H, wc = W.
 *   pred(y,x) = sum over covering windows of bilinear(logits_win)(y - y0, x - x0) / cover count
 *   out = resize(pred, (Ho, Wo)) (identity when Ho == H and Wo == W: `rescale` to ori_shape)
 *   p = softmax_c(out), read at the mirrored position when flip = 1 (horizontal) / 2 (vertical)
 *   probs_out[N][C][Ho][Wo] = (probs_in ? probs_in : 0) + p     (either may be NULL; may alias)
 *   labels[N][Ho][Wo]       = argmax_c of that sum (of the logits when no probabilities are used)
 * Returns GS_E_BADARG if a window leaves the image or a pixel is not covered. */
typedef struct gs_slide_desc {
  int32_t N, C, ld;       /* images per window, classes, padded class stride of logits */
  int32_t hl, wl;         /* low-resolution logits size of one window */
  int32_t hc, wc;         /* window size in image pixels */
  int32_t H, W;           /* image size */
  int32_t Ho, Wo;         /* output size */
  int32_t ny, nx;         /* window rows / columns */
  int32_t align_corners;
  int32_t flip;           /* 0 none, 1 horizontal, 2 vertical */
  int32_t reserved;       /* must be 0 */
} gs_slide_desc;
int gs_slide_fuse(const gs_slide_desc* d, const int32_t* win_y, const int32_t* win_x,
                  const float* logits, const float* probs_in, float* probs_out, int64_t* labels,
                  void* stream);
/* Test / A-B hook: label-only, un-rescaled gs_slide_fuse calls walk strips of 4 output pixels that
 * share their low-resolution cell's corner vectors (mode 1, the default) or use the per-pixel kernel
 * (mode 0); -1 = back to the GS_SLIDE_STRIP environment value.  Both give bit-identical label maps. */
int gs_debug_set_slide_strip(int32_t mode);

/* mIoU evaluation support: conf[label*C + pred] += 1 over the pixels
 * whose label != ignore_index; conf is [C*C] uint64, accumulated (zero it before the first call).
 * Replaces mmseg's intersect_and_union histogramming behind
 * gaiaseg/core/evaluation/cross_arch_eval_hooks.py:85-92. */
int gs_confusion_matrix(const int64_t* pred, const int64_t* label, int64_t n, int32_t num_classes,
                        int32_t ignore_index, uint64_t* conf, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Optimiser — K18                                                                             */
/* ------------------------------------------------------------------------------------------ */
/* torch.optim.SGD(momentum, weight_decay, dampening=0, nesterov=False) over flat fp32 arenas
 * (cfg optimizer: configs/_dynamic_/models/pspnet_ar50to101v2_gsync.py:175).  One call updates
 * one contiguous element range [0,n) of the arenas; the host merges the parameters used this step
 * into a few ranges (parameters of depth-skipped blocks are not in any range: no update at all).
 * momentum_buf starts at zero, so the first use gives buf = g exactly as torch does.
 *   g = grad*grad_scale + weight_decay*p ; buf = momentum*buf + g ; p -= lr*buf
 * grad_scale is 1/world_size for the data-parallel mean. n % 4 == 0, pointers 16-byte aligned.
 * zero_grad != 0 clears grad after use (optimizer.zero_grad() of the NEXT iteration folded in:
 * OptimizerHook's zero_grad -> backward -> step order). */
int gs_sgd_step(float* param, float* grad, float* momentum_buf, int64_t n, float lr,
                float momentum, float weight_decay, float grad_scale, int32_t zero_grad, void* stream);
/* Same update with the hyper-parameters read from DEVICE memory when the kernel runs:
 * hyper = {lr, momentum, weight_decay, grad_scale} (16-byte aligned).  The launch carries no
 * step-dependent value, so a hipGraph captured around a whole training step (core/runner.py) can be
 * replayed under the poly learning-rate schedule (PolyLrUpdaterHook) by rewriting 16 bytes. */
/* Writes {lr, momentum, weight_decay, grad_scale} into that buffer in stream order (the values travel
 * as kernel arguments: unlike an asynchronous copy from a reused host buffer, a launch that is still
 * queued when the host moves on to the next step keeps its own values). */
int gs_sgd_set_hyper(float* hyper, float lr, float momentum, float weight_decay, float grad_scale,
                     void* stream);
int gs_sgd_step_hyper(float* param, float* grad, float* momentum_buf, int64_t n, const float* hyper,
                      int32_t zero_grad, void* stream);
/* Parameter groups (paramwise_cfg: per-group lr / weight decay, core/optimizer.py).  BatchNorm
 * parameters sit between the conv weights of the forward-order arena, so a grouping cuts a subnet's
 * few merged ranges into many fragments (84-294 for the anchors of the in-tree supernets when norm
 * parameters are a group of their own); ONE launch walks a table of chunks instead.
 *   chunk = {begin, length, group} in units of 4 floats, relative to the three arena bases; every
 *           chunk lies inside one fragment of one group (the host cuts fragments into chunks of at
 *           most a few thousand floats and uploads the table once per set of ranges).  16 bytes per
 *           entry, table 16-byte aligned; begin >= 0, length >= 0, 0 <= group < n_groups (an entry
 *           that breaks this is skipped, not followed).
 *   hyper = {momentum, grad_scale, n_groups, 0, lr_0, wd_0, lr_1, wd_1, ...}: 4 + 2 *
 *           GS_SGD_MAX_GROUPS floats of device memory, 16-byte aligned, written by
 *           gs_sgd_set_group_hyper in stream order (values travel as kernel arguments, as in
 *           gs_sgd_set_hyper).  gs_sgd_step_groups carries no step-dependent argument, so a captured
 *           step graph replays under a changing per-group schedule.
 * The per-element update is gs_sgd_step's own expression: a group whose lr / wd equal the by-value
 * arguments of gs_sgd_step gets bit-identical results.  Elements outside the table are never
 * touched in param, grad or momentum_buf.  GS_E_NULL / GS_E_BADARG (n_chunks <= 0, n_groups outside
 * [1, GS_SGD_MAX_GROUPS]) / GS_E_ALIGN before any launch. */
#define GS_SGD_MAX_GROUPS 16
typedef struct GsSgdGroups {
  float lr_wd[2 * GS_SGD_MAX_GROUPS]; /* {lr_0, wd_0, lr_1, wd_1, ...}; entries >= n_groups ignored */
} GsSgdGroups;
typedef struct GsSgdChunk {
  int32_t begin;    /* first float4 of the chunk */
  int32_t length;   /* float4s in the chunk */
  int32_t group;    /* index into the hyper table */
  int32_t reserved; /* 0 */
} GsSgdChunk;
int gs_sgd_set_group_hyper(float* hyper, float momentum, float grad_scale, int32_t n_groups,
                           GsSgdGroups lr_wd, void* stream);
int gs_sgd_step_groups(float* param, float* grad, float* momentum_buf, const GsSgdChunk* chunks,
                       int32_t n_chunks, const float* hyper, int32_t zero_grad, void* stream);
/* Fused AdamW (torch.optim.AdamW, single-tensor form, amsgrad=False, maximize=False) over a chunk
 * table, with a step counter PER PARAMETER in device memory (torch keeps state['step'] per parameter
 * and advances it only when the parameter has a gradient; a depth-skipped block of a supernet has
 * none).  For every element of every chunk, with t = steps[slot] + 1 of the chunk's parameter:
 *   g = grad * grad_scale
 *   p *= (float)(1 - lr*wd)
 *   m += (g - m) * (float)(1 - beta1)
 *   v  = v * (float)beta2 + g*g * (float)(1 - beta2)
 *   p -= (float)(lr / (1 - beta1^t)) * m / (sqrt(v) / (float)sqrt(1 - beta2^t) + (float)eps)
 *   grad = 0 when zero_grad != 0
 * Every scalar is formed in fp64 and rounded to fp32 once, as torch forms them in Python doubles;
 * 1 - beta^t is -expm1(t log beta), evaluated in fp64 once per chunk.
 *   chunks: GsSgdChunk entries whose `reserved` field is the SLOT of the chunk's parameter in
 *           `steps`.  A chunk never spans two parameters and one parameter's chunks are contiguous
 *           in the table.  An entry naming a group >= n_groups, a slot outside [0, n_slots), a
 *           negative begin or a length <= 0 is skipped, not followed.
 *   steps:  n_slots int32 counters of device memory.  The step kernel only reads them; a second
 *           small launch of the same call advances, in stream order and without atomics, the counter
 *           of every parameter the table stepped, by one.  No host read: a captured step graph
 *           replays both launches.
 *   hyper:  GS_ADAMW_HYPER_DOUBLES doubles of device memory, 16-byte aligned: {beta1, beta2, eps,
 *           grad_scale, n_groups, log beta1, log beta2, 0, lr_0, wd_0, lr_1, wd_1, ...}, written by
 *           gs_adamw_set_group_hyper in stream order (the values travel as kernel arguments).
 * Elements outside the table are never read or written in param, grad, exp_avg or exp_avg_sq.
 * GS_E_NULL / GS_E_BADARG (n_chunks <= 0, n_slots <= 0, n_groups outside [1, GS_SGD_MAX_GROUPS], a
 * beta outside [0, 1), eps <= 0) / GS_E_ALIGN before any launch. */
#define GS_ADAMW_HYPER_DOUBLES (8 + 2 * GS_SGD_MAX_GROUPS)
typedef struct GsAdamwGroups {
  double lr_wd[2 * GS_SGD_MAX_GROUPS]; /* {lr_0, wd_0, lr_1, wd_1, ...}; entries >= n_groups ignored */
} GsAdamwGroups;
int gs_adamw_set_group_hyper(double* hyper, double beta1, double beta2, double eps, double grad_scale,
                             int32_t n_groups, GsAdamwGroups lr_wd, void* stream);
int gs_adamw_step_groups(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int32_t* steps,
                         int32_t n_slots, const GsSgdChunk* chunks, int32_t n_chunks,
                         const double* hyper, int32_t zero_grad, void* stream);
/* Gradient accumulation of a sandwich iteration (one SGD step over several subnets, US-Nets): the
 * weight-gradient kernels overwrite their gradient, so each member's gradients are moved into an
 * accumulation arena:  dst[i] += src[i]; src[i] = 0  for i in [0, n).  One launch per range; float4
 * when both pointers are 16-byte aligned.  dst and src must not overlap. */
int gs_grad_accumulate(float* dst, float* src, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Training input pipeline                                             */
/* ------------------------------------------------------------------------------------------ */
/* One sample of the reference's train_pipeline (configs/_dynamic_/models/
 * pspnet_ar50to101v2_gsync.py:60-75: Resize(ratio_range) -> RandomCrop -> RandomFlip ->
 * PhotoMetricDistortion -> Normalize(to_rgb) -> Pad -> DefaultFormatBundle) as one gather kernel
 * from the ORIGINAL uint8 image [src_h][src_w][3] and label map [src_h][src_w] on the device to
 * out_img fp32 [3][out_h][out_w] and out_label int64 [out_h][out_w] (may be NULL).  The random
 * decisions are made by the caller and passed in the descriptor:
 *   res_h, res_w      size of the (virtual) resized image        (mmcv.imrescale)
 *   crop_y/x, crop_h/w the crop window inside it, crop <= out     (RandomCrop; the rest is padding)
 *   flip              horizontal flip of the crop                 (RandomFlip)
 *   pm_*              PhotoMetricDistortion: brightness delta, contrast alpha (first = mode 1),
 *                     saturation alpha, integer hue delta (uint8 HSV, H in [0,180))
 *   mean/std/to_rgb   Normalize; pad_val / seg_pad_val            (Pad)
 * Resize: image bilinear with half-pixel centres rounded to uint8, label nearest. */
typedef struct gs_augment_desc {
  int32_t src_h, src_w, src_is_rgb;
  int32_t res_h, res_w;
  int32_t crop_y, crop_x, crop_h, crop_w;
  int32_t out_h, out_w;
  int32_t flip;
  int32_t pm_enable, pm_brightness, pm_contrast, pm_contrast_first, pm_saturation, pm_hue;
  float pm_delta, pm_alpha, pm_sat_alpha;
  int32_t pm_hue_delta;
  int32_t to_rgb;
  float mean[3], std[3];
  float pad_val;
  int32_t seg_pad_val;
} gs_augment_desc;
int gs_seg_augment(const gs_augment_desc* d, const uint8_t* img, const uint8_t* label,
                   float* out_img, int64_t* out_label, void* stream);

/* Test-time augmentation views (mmseg's MultiScaleFlipAug test pipeline): ONE
 * launch writes every view of one decoded uint8 image [src_h][src_w][3] (BGR, or RGB with
 * src_is_rgb as in gs_augment_desc).  View k is the image resized to res_h x res_w (gs_seg_augment's
 * bilinear: half-pixel centres, edge-clamped, rounded to uint8), then flipped (0 none, 1 horizontal,
 * 2 vertical), then normalised ((x - mean) / std, RGB planes when to_rgb): fp32 [3][res_h][res_w] at
 * `out`, usually this image's slot of the view's [N][3][res_h][res_w] batch tensor.  The arithmetic is
 * gs_seg_augment's own (separately rounded fp32 operations), so an unflipped view equals what that
 * kernel writes for the same size bit for bit, and a flipped view is the exact mirror image of its
 * unflipped twin.  There is no label input or output; nothing outside the 3 * res_h * res_w floats
 * of each slot is written, and a slot needs 4-byte alignment only.  The descriptor travels by value.
 * GS_E_NULL (img or a view's out) / GS_E_BADARG (n_views outside [1, GS_TTA_MAX_VIEWS], a
 * non-positive size, flip outside {0, 1, 2}, std <= 0) before any launch. */
#define GS_TTA_MAX_VIEWS 16
typedef struct gs_tta_view {
  int32_t res_h, res_w;
  int32_t flip;        /* 0 none, 1 horizontal, 2 vertical */
  int32_t reserved;    /* 0 */
  float* out;
} gs_tta_view;
typedef struct gs_tta_desc {
  int32_t src_h, src_w, src_is_rgb;
  int32_t n_views;
  int32_t to_rgb;
  float mean[3], std[3];
  int32_t reserved;    /* 0 */
  gs_tta_view views[GS_TTA_MAX_VIEWS];   /* entries >= n_views ignored */
} gs_tta_desc;
int gs_tta_views(gs_tta_desc d, const uint8_t* img, void* stream);

/* mmseg's show_result blend on the device: labels int64 [H][W], img uint8 [H][W][3] in BGR, palette
 * uint8 [num_classes][3] in RGB -> out uint8 [H][W][3] in BGR,
 *   out = uint8(img * (1 - opacity) + colour_bgr * opacity)
 * evaluated in double and truncated (numpy's result for a Python float opacity, exactly).  A label
 * outside [0, num_classes) takes colour (0, 0, 0), as mmseg's zero-initialised color_seg does.  out
 * must not overlap img.  GS_E_NULL / GS_E_BADARG (a size or num_classes <= 0, opacity outside [0, 1]). */
int gs_seg_overlay(const int64_t* labels, const uint8_t* img, const uint8_t* palette,
                   int32_t num_classes, int32_t H, int32_t W, double opacity, uint8_t* out,
                   void* stream);

/* Elastic input resolution (data.input_shape): one launch resamples a
 * normalised batch on the device.
 *   img    fp32 NCHW [N][3][h][w] -> out_img [N][3][H][W]: bilinear, align_corners=False, ATen's fp32
 *          source indices and weights (F.interpolate's);
 *   label  int64 [N][1][h][w] -> out_label [N][1][H][W]: nearest, source index
 *          min(floor(dst * (float)in / out), in - 1) in fp32 (ATen's); every value, 255 included, is
 *          copied as it is.  label and out_label may both be NULL (evaluation rescales the image only).
 * All four tensors are contiguous; the sources and the destinations must not overlap.  No workspace,
 * no atomics, launched on `stream` (capturable).  The output is written in aligned 16-byte pieces
 * over the flat tensors, so out_img and out_label must be 16-byte aligned; img needs 4-byte and label
 * 8-byte alignment.  GS_E_NULL: img or out_img NULL, or only one of label / out_label given;
 * GS_E_BADARG: a size <= 0, a plane of more than 2^31 - 1 pixels, or a source or output image of
 * 2^63 elements and more; GS_E_ALIGN. */
int gs_batch_rescale(const float* img, const int64_t* label, int32_t N, int32_t h, int32_t w,
                     float* out_img, int64_t* out_label, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Forward precision of the convolutions (inference; tools/test_supernet.py with cfg.fp16).       */
/*   0 = fp32 (default): every launch as documented above.                                     */
/*   1 = fp16 operands: a forward launch of gs_conv2d_forward / gs_conv_bn_forward that takes   */
/*       the fast row kernel with a 64-row tile (columns narrowed to 64 / 48 where the planner  */
/*       chose 80 / 32) contracts on GS_KLOOP_F16: both operands -- the input AFTER its fp32     */
/*       in_affine BatchNorm + ReLU -- are rounded once to fp16 (round to nearest even) and     */
/*       multiplied on v_mfma_f32_16x16x32_f16 with fp32 accumulation.  The error of an output   */
/*       is that of an fp64 contraction of the rounded operands plus fp32 accumulation noise    */
/*       (~1e-6 of sum |a||b|).  Outputs, BatchNorm, residual, ReLU and split-K stay fp32.       */
/*       The stem, the 1x1 streaming kernel, the generic kernel and all data- and weight-       */
/*       gradient launches keep their fp32 paths.  Not for training: the gradients assume fp32. */
/* Process-global.  gs_set_forward_precision returns GS_E_BADARG for any other mode.            */
/* ------------------------------------------------------------------------------------------ */
int gs_set_forward_precision(int32_t mode);
int32_t gs_get_forward_precision(void);
/* ------------------------------------------------------------------------------------------ */
/* Training precision of the convolutions (fp16 mixed-precision training, separate from the    */
/* inference switch above, which it neither reads nor changes).                                */
/*   0 = fp32 (default): every launch as documented above.                                     */
/*   1 = fp16 operands: every forward launch that forward precision 1 puts on GS_KLOOP_F16      */
/*       (in_affine included) AND every data-gradient launch of gs_conv2d_dgrad /               */
/*       gs_conv_bn_backward that takes the fast row kernel with a 64-row tile -- stride 1 and    */
/*       the parity classes of a strided one; columns narrowed to 64 / 48 where the planner chose */
/*       80 / 32, split-K factor and workspace unchanged -- contract on GS_KLOOP_F16: dy and W    */
/*       rounded once to fp16 (round to nearest even), fp32 accumulation; the fused              */
/*       BatchNorm-backward epilogue and the split-K combine stay fp32.  The stem, the 1x1        */
/*       streaming kernel (forward and data gradient), the generic kernels and every weight-     */
/*       gradient launch keep their fp32 paths.                                                  */
/* Process-global.  gs_set_train_precision returns GS_E_BADARG for any other mode.              */
/* ------------------------------------------------------------------------------------------ */
int gs_set_train_precision(int32_t mode);
int32_t gs_get_train_precision(void);

/* ------------------------------------------------------------------------------------------ */
/* Tuning hook (tools/sweep_conv_plans.py): force tile rows (64|128), tile columns            */
/* (32|48|64|80|96|128) and split-K factor of the following gs_conv2d_* calls; bm = 0 restores */
/* the planner.  Process-global, not thread-safe, results stay exact (only the fixed summation */
/* order of split-K changes).                                                                  */
/* ------------------------------------------------------------------------------------------ */
int gs_debug_force_plan(int32_t bm, int32_t bn, int32_t splits);
/* The tile / split-K plan the library would choose for an M x N x K implicit GEMM (max_splits: 64 for
 * forward / dgrad, 512 for wgrad).  Host arithmetic only (no GPU needed). */
int gs_debug_query_plan(int32_t M, int32_t N, int32_t K, int32_t max_splits, int32_t* bm,
                        int32_t* bn, int32_t* splits, int32_t* ksteps_per_split);

/* Which kernel family and K loop an implicit-GEMM launch used.  The parity tests assert it, so that a
 * comparison against F.conv2d is known to have exercised the loop it claims to (the stride-1 data
 * gradient of every bottleneck conv, gaiaseg/models/utils/dynamic_res_layer.py:105-125, contracts on
 * GS_KLOOP_BF16X3 when its grid is large enough and on the fp32 loops otherwise). */
#define GS_OP_FORWARD 0
#define GS_OP_DGRAD 1
#define GS_OP_WGRAD 2
#define GS_KLOOP_GENERIC 0      /* igemm_rows_kernel / igemm_wgrad_kernel: any shape, sectioned loop  */
#define GS_KLOOP_FP32 1         /* fast kernels, v_mfma_f32_16x16x4_f32, one K step per barrier       */
#define GS_KLOOP_FP32_PAIRS 2   /* the same, two K steps per barrier                                  */
#define GS_KLOOP_BF16X3 3       /* six v_mfma_f32_16x16x32_bf16 over an exact 3-way bf16 split        */
#define GS_KLOOP_STREAM 4       /* 1x1 streaming kernel: weights resident in LDS, persistent over rows  */
#define GS_KLOOP_COUNT 5         /* entries per op of the count / FLOP tables below (GS_KLOOP_F16 has none) */
#define GS_KLOOP_F16 5           /* forward, fp16 mode only: one v_mfma_f32_16x16x32_f16 on operands
                                  * rounded to fp16; reported by gs_debug_last_conv_launch and
                                  * gs_debug_query_conv_launch, counted by gs_debug_f16_launches  */
typedef struct gs_debug_launch {
  int32_t op;                   /* GS_OP_*                                                            */
  int32_t kloop;                /* GS_KLOOP_*                                                         */
  int32_t bm, bn, splits, ksteps_per_split;
  int32_t in_affine;            /* 1: relu(bn(x)) evaluated in the operand loader                     */
  int32_t bn_bwd_mode;          /* dgrad: gs_bn_bwd_fuse mode folded into the tile epilogue (0 none)   */
} gs_debug_launch;
/* The most recent conv launch issued by the calling thread (a strided dgrad reports its last parity
 * class).  GS_E_BADARG if the thread has not launched any. */
int gs_debug_last_conv_launch(gs_debug_launch* out);
/* counts[(op * GS_KLOOP_COUNT + kloop) * 3 + bn_bwd_mode] = launches since the last reset
 * (process-wide, 45 entries); reset != 0 clears after reading.  counts may be NULL (reset only). */
int gs_debug_conv_launch_counts(int64_t* counts, int32_t reset);
/* flops[op * GS_KLOOP_COUNT + kloop] (15 entries) = algorithmic FLOPs (2 * M * N * K of the implicit GEMM, padding not counted)
 * launched since the last reset: bench.py states which share of a step's contraction work ran on
 * which MFMA path, so that its roofline fractions name the right bound.  The forward thread and the
 * autograd thread may both launch: the counters are updated atomically. */
int gs_debug_conv_launch_flops(double* flops, int32_t reset);
/* Forward convolutions on the bf16x3 K loop: 0 = never (fp32 MFMA loops), 1 = the shapes where it
 * measured ahead (3x3, not where the two-steps-per-barrier fp32 loop runs unsplit), 2 = every launch
 * the loop's gate admits (the operator tests), 3 = the split-K 3x3s only (the default: see
 * csrc/igemm_core.h x3_fwd_mode for the parity margins behind that choice), -1 = back to the
 * GS_X3_FWD environment value.  Process-global. */
int gs_debug_set_x3_fwd(int32_t mode);
/* Split-K launches of the forward / data-gradient row kernels: 1 = every output tile's partial slabs
 * are summed inside the launch by the tile's last-arriving workgroup, which then runs the unsplit
 * epilogue (default; csrc/igemm_core.h splitk_publish), 0 = a separate reduce launch sums them,
 * -1 = back to the GS_SPLITK_INKERNEL environment value.  Both sum in split order: the outputs are
 * bit-identical.  Process-global. */
int gs_debug_set_splitk_inkernel(int32_t mode);
/* Split-K row launches since the last reset that combined their slabs inside the launch (the parity
 * tests check that the shapes they compare really took that path); reset != 0 clears the count. */
int64_t gs_debug_splitk_combined(int32_t reset);
/* The per-tile partials a fused conv + BatchNorm call leaves (BatchNorm statistics of the forward,
 * BatchNorm-backward sums of a data gradient with gs_bn_bwd_fuse).  mode is a mask — 1: the forward
 * statistics, 2: the data gradient's sums, 3: both —; a set bit means launches with at most
 * GS_COL_FINALIZE_MAX (160) row tiles merge them inside the launch — the last workgroup of every
 * column tile writes the coefficients / sums (csrc/igemm_core.h column_finalize_*), 0 = a separate
 * launch merges them (the default: the in-launch form measured neutral on the training step, every
 * workgroup pays the arrival hand-off), -1 = back to the GS_COL_FINALIZE environment value.
 * Process-global.
 * gs_debug_col_finalized: launches since the last reset that merged their partials themselves. */
int gs_debug_set_col_finalize(int32_t mode);
int64_t gs_debug_col_finalized(int32_t reset);
/* Compute units the planners assume: hipDeviceProp::multiProcessorCount of the current device, read
 * once at first use (256 on an MI355X; 256 is also assumed when no device is present). */
int gs_debug_num_cu(void);
/* Dispatch of the streaming 1x1 kernel (csrc/igemm_stream.h): 0 = never, 1 = the shapes where it
 * measured ahead of the tile kernels (default), 2 = every shape whose weights fit in LDS (the operator
 * tests cover all of its code paths this way), -1 = back to the GS_STREAM environment value.
 * Process-global, not thread-safe. */
int gs_debug_set_stream_mode(int32_t mode);
/* The same for the forward launches with role GS_CONV_ROLE_BOTTLENECK3X3 only: flops[kloop], 5 entries
 * (which bound bench.py's headline `roofline` is priced against). */
int gs_debug_k3_flops(double* flops, int32_t reset);
/* Launches on GS_KLOOP_F16 since the last reset (*n) and their algorithmic FLOPs (*flops, 2 * M * N * K);
 * either pointer may be NULL, reset != 0 clears both after reading. */
int gs_debug_f16_launches(int64_t* n, double* flops, int32_t reset);
/* The same split by op: n[GS_OP_FORWARD], n[GS_OP_DGRAD] and flops[...] (2 entries each; either
 * pointer may be NULL), reset != 0 clears these two pairs after reading (not gs_debug_f16_launches'). */
int gs_debug_f16_launches_by_op(int64_t* n, double* flops, int32_t reset);
/* What gs_conv2d_forward / _dgrad / _wgrad (op = GS_OP_*) WOULD launch for this descriptor: host
 * arithmetic only, no GPU needed (honours gs_debug_force_plan, the GS_X3 switches,
 * gs_set_forward_precision and gs_set_train_precision).  For a strided
 * dgrad it describes the parity class (0, 0). */
int gs_debug_query_conv_launch(const gs_conv_desc* d, int32_t op, gs_debug_launch* out);

/* ------------------------------------------------------------------------------------------ */
/* Stream fork / join: work enqueued on `to` after this call waits for everything enqueued on  */
/* `from` before it (hipEventRecord + hipStreamWaitEvent on an internal event ring).  Used to   */
/* run the weight-gradient kernels on a side stream beside BN-backward / dgrad (the reference   */
/* runs all of backward on one stream: torch autograd, gaiaseg/apis/train.py:88-96).            */
/* ------------------------------------------------------------------------------------------ */
int gs_stream_fork(void* from_stream, void* to_stream);

#ifdef __cplusplus
}
#endif
#endif /* GAIASEG_HIP_H */
