// ConvTranspose2d(kernel_size = 2, stride = 2) forward on NHWC fp32 (include/gaiaseg_hip.h).
//
// Kernel == stride: output pixel (2 h + dy, 2 w + dx) depends on input pixel (h, w) alone, through tap
// (dy, dx).  The four taps are four 1x1 convolutions of the same input, so they run as ONE implicit-GEMM
// launch Cin -> 4 Cout on the tuned MFMA kernels (gs_conv2d_forward: BEiT-B's fpn1 is 2 x 768 x 3072 flops
// per token, far too much for anything but the GEMM), writing rows [pixel][tap][Cout] into scratch.  The
// depth-to-space kernel below moves every row's four Cout-wide pieces to their output pixels and adds
// the bias: one float4 read and one float4 write per element, bandwidth-bound.
#include "common.h"

namespace gs {
namespace {

// s: [N*H*W][4][C] packed; y[n][2 h + dy][2 w + dx][:C] = s[(n, h, w)][2 dy + dx][:C] + bias
__global__ __launch_bounds__(256) void depth_to_space2_kernel(const float* __restrict__ s,
                                                              const float* __restrict__ bias,
                                                              float* __restrict__ y, const int64_t items,
                                                              const int H, const int W, const int C4,
                                                              const int ldy) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % C4);
    const int64_t row = it / C4;          // (pixel, tap)
    const int tap = (int)(row & 3);
    const int64_t pix = row >> 2;
    const int w = (int)(pix % W);
    const int64_t nh = pix / W;
    const int h = (int)(nh % H);
    const int64_t n = nh / H;
    f32x4 v = *reinterpret_cast<const f32x4*>(s + it * 4);
    if (bias) v += *reinterpret_cast<const f32x4*>(bias + cq * 4);
    const int64_t opix = (n * (2 * H) + 2 * h + (tap >> 1)) * (2 * W) + 2 * w + (tap & 1);
    *reinterpret_cast<f32x4*>(y + opix * ldy + cq * 4) = v;
  }
}

int deconv_check(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return GS_E_BADARG;
  if (4 * (int64_t)N * H * W > INT32_MAX || 4 * (int64_t)Cout > INT32_MAX) return GS_E_BADARG;
  if (Cin % 4 || Cout % 4) return GS_E_ALIGN;
  return GS_OK;
}

gs_conv_desc gemm_desc(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t ldx) {
  gs_conv_desc d = {};
  d.N = N; d.H = H; d.W = W;
  d.Ci = d.Ci_max = Cin;
  d.Co = d.Co_ld = d.ldy = 4 * Cout;
  d.KH = d.KW = 1;
  d.stride = 1; d.pad = 0; d.dil = 1;
  d.Ho = H; d.Wo = W;
  d.x_sn = (int64_t)H * W * ldx; d.x_sh = (int64_t)W * ldx; d.x_sw = ldx; d.x_sc = 1;
  return d;
}

inline size_t scratch_bytes(int32_t N, int32_t H, int32_t W, int32_t Cout) {
  return (size_t)N * H * W * 4 * Cout * sizeof(float);   // a multiple of 16: Cout % 4 == 0
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_deconv2x2_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout) {
  if (deconv_check(N, H, W, Cin, Cout) != GS_OK) return 0;
  const gs_conv_desc d = gemm_desc(N, H, W, Cin, Cout, Cin);
  return scratch_bytes(N, H, W, Cout) + gs_conv2d_workspace_bytes(&d);
}

extern "C" int gs_deconv2x2_forward(const float* x, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t ldx,
                                    const float* w4, int32_t Cout, const float* bias, float* y, int32_t ldy,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = deconv_check(N, H, W, Cin, Cout);
  if (rc != GS_OK) return rc;
  if (ldx % 4 || ldy % 4) return GS_E_ALIGN;
  if (ldx < Cin || ldy < Cout) return GS_E_BADARG;
  if (!x || !w4 || !y) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(w4) || !aligned16(y) || (bias && !aligned16(bias)) ||
      (workspace && !aligned16(workspace)))
    return GS_E_ALIGN;
  if (!workspace || workspace_bytes < gs_deconv2x2_workspace_bytes(N, H, W, Cin, Cout)) return GS_E_WORKSPACE;
  const gs_conv_desc d = gemm_desc(N, H, W, Cin, Cout, ldx);
  const size_t sb = scratch_bytes(N, H, W, Cout);
  float* scratch = static_cast<float*>(workspace);
  const int grc = gs_conv2d_forward(&d, x, w4, nullptr, nullptr, scratch, static_cast<char*>(workspace) + sb,
                                    workspace_bytes - sb, stream);
  if (grc != GS_OK) return grc;
  const int64_t items = (int64_t)N * H * W * 4 * (Cout / 4);
  hipLaunchKernelGGL(depth_to_space2_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream),
                     scratch, bias, y, items, H, W, Cout / 4, ldy);
  return launch_status();
}
