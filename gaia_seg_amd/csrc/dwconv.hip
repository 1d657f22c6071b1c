// Depthwise 3x3 and 7x7 convolution (stride 1, any dilation and padding) on NHWC fp32: forward, data
// gradient and a two-stage weight gradient (gs_dwconv2d_* in include/gaiaseg_hip.h).  The text below
// describes the 3x3 kernels; the 7x7 ones (ConvNeXt) follow them further down with their own structure.
//
// A depthwise conv has no channel reduction: 9 multiply-adds per output element against 8 bytes moved,
// so all three kernels are bandwidth-bound and there is nothing for the matrix cores to do.  One thread
// owns one float4 channel quad; consecutive lanes own consecutive quads of the same pixel, so every
// load and store of a wave is a run of contiguous 16-byte pieces.  The nine weight quads of a thread
// live in registers.  Taps that fall into the zero padding are skipped, not loaded.
//
//   forward / dgrad : one stencil kernel.  A thread computes a strip of kStrip output pixels of one
//                     column, `dil` rows apart: the kStrip + 2 input rows they touch are the same
//                     residue class modulo dil, so each is loaded once per tap column and reused by
//                     the three vertical taps.  (The vertical direction is the one to reuse in
//                     registers: rows a dilation apart are megabytes apart, the horizontal taps are a
//                     few pixels apart and come from the caches.)  The data gradient is the same
//                     stencil on dy with the taps mirrored and the padding 2 * dil - pad.
//   wgrad           : stage 1 reduces runs of kWgPixels output pixels to per-run partials
//                     [run][tap][C] in the workspace (registers, then a fixed-order LDS sum over the
//                     16 pixel lanes of a workgroup); stage 2 sums the runs of every (tap, quad) in a
//                     fixed order.  No atomics: bit-identical from run to run.
#include "common.h"

namespace gs {
namespace {

constexpr int kStrip = 4;         // output pixels of one column per thread (forward / dgrad)
constexpr int kWgQuads = 16;      // channel quads per weight-gradient workgroup (256 contiguous bytes)
constexpr int kWgLanes = 16;      // pixel lanes per weight-gradient workgroup
constexpr int kWgPixels = 256;    // output pixels per stage-1 workgroup (16 per lane)

struct DwStencil {
  int32_t N, Hi, Wi, Ho, Wo, C4;
  int32_t ldi, ldo, ldw;     // pixel pitches of in / out and the tap pitch of w, in floats
  int32_t dil, off;          // input coordinate of tap k for output coordinate o: o + k * dil - off
  int32_t flip, accumulate, strips;
};

__global__ __launch_bounds__(256) void dw_stencil_kernel(const DwStencil a, const float* __restrict__ in,
                                                         const float* __restrict__ w,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ out, const int64_t items) {
  const int dil = a.dil;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    int64_t r = it / a.C4;
    const int wo = (int)(r % a.Wo);
    r /= a.Wo;
    const int s = (int)(r % a.strips);
    const int n = (int)(r / a.strips);
    // strip s: the output rows h0, h0 + dil, ... of one residue class modulo dil
    const int h0 = s % dil + (s / dil) * kStrip * dil;
    if (h0 >= a.Ho) continue;
    f32x4 wt[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] = ld4(w + (int64_t)(a.flip ? 8 - k : k) * a.ldw + cq * 4);
    f32x4 acc[kStrip];
    const f32x4 b = bias ? ld4(bias + cq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kStrip; ++j) acc[j] = b;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int wi = wo + kw * dil - a.off;
      if (wi < 0 || wi >= a.Wi) continue;
      const float* col = in + ((int64_t)n * a.Hi * a.Wi + wi) * a.ldi + cq * 4;
      f32x4 win[kStrip + 2];
#pragma unroll
      for (int j = 0; j < kStrip + 2; ++j) {
        const int hi = h0 + j * dil - a.off;
        // (rows that only feed outputs beyond Ho are not loaded either)
        const bool ok = hi >= 0 && hi < a.Hi && h0 + (j > 2 ? j - 2 : 0) * dil < a.Ho;
        win[j] = ok ? ld4(col + (int64_t)hi * a.Wi * a.ldi) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int j = 0; j < kStrip; ++j) acc[j] += win[j + kh] * wt[kh * 3 + kw];
    }
#pragma unroll
    for (int j = 0; j < kStrip; ++j) {
      const int ho = h0 + j * dil;
      if (ho >= a.Ho) break;
      float* p = out + (((int64_t)n * a.Ho + ho) * a.Wo + wo) * a.ldo + cq * 4;
      st4(p, a.accumulate ? ld4(p) + acc[j] : acc[j]);
    }
  }
}

struct DwWgrad {
  int32_t H, W, Ho, Wo, C4;
  int32_t ldx, ldy, ldw, C;
  int32_t dil, pad;
  int64_t pixels;            // N * Ho * Wo
  int32_t runs;              // ceil(pixels / kWgPixels)
  int32_t taps;              // KH * KW
};

// stage 1: grid (runs, quad groups).  part[(run * 9 + tap) * C + c]
__global__ __launch_bounds__(256) void dw_wgrad_partial_kernel(const DwWgrad a, const float* __restrict__ x,
                                                               const float* __restrict__ dy,
                                                               float* __restrict__ part) {
  __shared__ f32x4 sh[9][kWgLanes][kWgQuads];
  const int ql = threadIdx.x % kWgQuads, pl = threadIdx.x / kWgQuads;
  const int cq = blockIdx.y * kWgQuads + ql;
  const int64_t p0 = (int64_t)blockIdx.x * kWgPixels;
  f32x4 acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cq < a.C4) {
    for (int i = 0; i < kWgPixels / kWgLanes; ++i) {
      const int64_t pix = p0 + i * kWgLanes + pl;
      if (pix >= a.pixels) break;
      const int wo = (int)(pix % a.Wo);
      const int64_t t = pix / a.Wo;
      const int ho = (int)(t % a.Ho);
      const int64_t n = t / a.Ho;
      const f32x4 g = ld4(dy + pix * a.ldy + cq * 4);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        const int hi = ho + kh * a.dil - a.pad;
        if (hi < 0 || hi >= a.H) continue;
        const float* row = x + (n * a.H + hi) * a.W * a.ldx + cq * 4;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int wi = wo + kw * a.dil - a.pad;
          if (wi >= 0 && wi < a.W) acc[kh * 3 + kw] += ld4(row + (int64_t)wi * a.ldx) * g;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) sh[k][pl][ql] = acc[k];
  __syncthreads();
  if (threadIdx.x < 9 * kWgQuads) {
    const int k = threadIdx.x / kWgQuads;
    if (cq < a.C4) {
      f32x4 s = sh[k][0][ql];
#pragma unroll
      for (int l = 1; l < kWgLanes; ++l) s += sh[k][l][ql];
      st4(part + ((int64_t)blockIdx.x * 9 + k) * a.C + cq * 4, s);
    }
  }
}

// stage 2: grid (quad groups, taps).  Lane l sums runs l, l + 16, ... in order, then the 16 lane
// sums are added in order.
__global__ __launch_bounds__(256) void dw_wgrad_sum_kernel(const DwWgrad a, const float* __restrict__ part,
                                                           float* __restrict__ dw) {
  __shared__ f32x4 sh[kWgLanes][kWgQuads];
  const int ql = threadIdx.x % kWgQuads, pl = threadIdx.x / kWgQuads;
  const int cq = blockIdx.x * kWgQuads + ql;
  const int k = blockIdx.y;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cq < a.C4)
    for (int r = pl; r < a.runs; r += kWgLanes) s += ld4(part + ((int64_t)r * a.taps + k) * a.C + cq * 4);
  sh[pl][ql] = s;
  __syncthreads();
  if (pl == 0 && cq < a.C4) {
    f32x4 t = sh[0][ql];
#pragma unroll
    for (int l = 1; l < kWgLanes; ++l) t += sh[l][ql];
    st4(dw + (int64_t)k * a.ldw + cq * 4, t);
  }
}

// ---- 7x7 ----------------------------------------------------------------------------------------
// 49 weight quads do not fit in registers beside the accumulators, so the 7x7 stencil walks the tap
// COLUMNS: for one kw it holds the 7 weight quads of that column and the kStrip7 + 6 input rows the
// strip touches (one load each, reused by all 7 vertical taps), and adds 7 * kStrip7 products into the
// strip's accumulators.  Per output quad that is (kStrip7 + 6) * 7 / kStrip7 = 12.25 input loads and
// 6.1 weight loads, all but the first touch of a line from L1 / L2: the HBM traffic stays one read of
// x and one write of y.  Summation order per output: kw outermost, then kh, like the 3x3 kernel.
constexpr int kK7 = 7;
constexpr int kStrip7 = 8;

__global__ __launch_bounds__(256) void dw7_stencil_kernel(const DwStencil a, const float* __restrict__ in,
                                                          const float* __restrict__ w,
                                                          const float* __restrict__ bias,
                                                          float* __restrict__ out, const int64_t items) {
  const int dil = a.dil;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    int64_t r = it / a.C4;
    const int wo = (int)(r % a.Wo);
    r /= a.Wo;
    const int s = (int)(r % a.strips);
    const int n = (int)(r / a.strips);
    const int h0 = s % dil + (s / dil) * kStrip7 * dil;
    if (h0 >= a.Ho) continue;
    f32x4 acc[kStrip7];
    const f32x4 b = bias ? ld4(bias + cq * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kStrip7; ++j) acc[j] = b;
#pragma unroll 1
    for (int kw = 0; kw < kK7; ++kw) {
      const int wi = wo + kw * dil - a.off;
      if (wi < 0 || wi >= a.Wi) continue;
      f32x4 wt[kK7];
#pragma unroll
      for (int kh = 0; kh < kK7; ++kh) {
        const int k = kh * kK7 + kw;
        wt[kh] = ld4(w + (int64_t)(a.flip ? kK7 * kK7 - 1 - k : k) * a.ldw + cq * 4);
      }
      const float* col = in + ((int64_t)n * a.Hi * a.Wi + wi) * a.ldi + cq * 4;
      f32x4 win[kStrip7 + kK7 - 1];
#pragma unroll
      for (int j = 0; j < kStrip7 + kK7 - 1; ++j) {
        const int hi = h0 + j * dil - a.off;
        // row j feeds the outputs max(0, j - 6) .. j of the strip: skip it when all of them are beyond Ho
        const bool ok = hi >= 0 && hi < a.Hi && h0 + (j > kK7 - 1 ? j - (kK7 - 1) : 0) * dil < a.Ho;
        win[j] = ok ? ld4(col + (int64_t)hi * a.Wi * a.ldi) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int kh = 0; kh < kK7; ++kh)
#pragma unroll
        for (int j = 0; j < kStrip7; ++j) acc[j] += win[j + kh] * wt[kh];
    }
#pragma unroll
    for (int j = 0; j < kStrip7; ++j) {
      const int ho = h0 + j * dil;
      if (ho >= a.Ho) break;
      float* p = out + (((int64_t)n * a.Ho + ho) * a.Wo + wo) * a.ldo + cq * 4;
      st4(p, a.accumulate ? ld4(p) + acc[j] : acc[j]);
    }
  }
}

// 7x7 stage 1: grid (runs, quad groups, 7 tap rows).  A workgroup owns ONE tap row kh of a run, so a
// thread carries 7 accumulator quads (49 would leave two waves per SIMD); the seven workgroups of a run
// read the same dy and overlapping rows of x, which the caches serve.  part[(run * 49 + tap) * C + c]
__global__ __launch_bounds__(256) void dw7_wgrad_partial_kernel(const DwWgrad a, const float* __restrict__ x,
                                                                const float* __restrict__ dy,
                                                                float* __restrict__ part) {
  __shared__ f32x4 sh[kK7][kWgLanes][kWgQuads];
  const int ql = threadIdx.x % kWgQuads, pl = threadIdx.x / kWgQuads;
  const int cq = blockIdx.y * kWgQuads + ql;
  const int kh = blockIdx.z;
  const int64_t p0 = (int64_t)blockIdx.x * kWgPixels;
  f32x4 acc[kK7];
#pragma unroll
  for (int k = 0; k < kK7; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cq < a.C4) {
    for (int i = 0; i < kWgPixels / kWgLanes; ++i) {
      const int64_t pix = p0 + i * kWgLanes + pl;
      if (pix >= a.pixels) break;
      const int wo = (int)(pix % a.Wo);
      const int64_t t = pix / a.Wo;
      const int ho = (int)(t % a.Ho);
      const int64_t n = t / a.Ho;
      const int hi = ho + kh * a.dil - a.pad;
      if (hi < 0 || hi >= a.H) continue;
      const f32x4 g = ld4(dy + pix * a.ldy + cq * 4);
      const float* row = x + (n * a.H + hi) * a.W * a.ldx + cq * 4;
#pragma unroll
      for (int kw = 0; kw < kK7; ++kw) {
        const int wi = wo + kw * a.dil - a.pad;
        if (wi >= 0 && wi < a.W) acc[kw] += ld4(row + (int64_t)wi * a.ldx) * g;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kK7; ++k) sh[k][pl][ql] = acc[k];
  __syncthreads();
  if (threadIdx.x < kK7 * kWgQuads) {
    const int k = threadIdx.x / kWgQuads;
    if (cq < a.C4) {
      f32x4 s = sh[k][0][ql];
#pragma unroll
      for (int l = 1; l < kWgLanes; ++l) s += sh[k][l][ql];
      st4(part + ((int64_t)blockIdx.x * (kK7 * kK7) + kh * kK7 + k) * a.C + cq * 4, s);
    }
  }
}

// Everything a call can get wrong, checked on the host before any launch.
int dw_check(const gs_dwconv_desc* d) {
  if (!d) return GS_E_NULL;
  if ((d->KH != 3 && d->KH != 7) || d->KW != d->KH || d->stride != 1 || d->dil < 1 || d->pad < 0)
    return GS_E_BADARG;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return GS_E_BADARG;
  if (d->C % 4 || d->C_ld % 4 || d->ldx % 4 || d->ldy % 4) return GS_E_ALIGN;
  if (d->C > d->C_ld || d->C > d->ldx || d->C > d->ldy) return GS_E_BADARG;
  const int64_t ho = (int64_t)d->H + 2LL * d->pad - (d->KH - 1LL) * d->dil;
  const int64_t wo = (int64_t)d->W + 2LL * d->pad - (d->KH - 1LL) * d->dil;
  if (ho < 1 || wo < 1 || ho > INT32_MAX || wo > INT32_MAX) return GS_E_BADARG;
  // (K - 1) * dil - pad (the data gradient's padding) and every coordinate o + k * dil - off stay in int32
  if (d->dil > (1 << 24) || d->pad > (1 << 24)) return GS_E_BADARG;
  const int64_t runs = ceil_div((int64_t)d->N * ho * wo, kWgPixels);
  if (runs > INT32_MAX || ceil_div(d->C / 4, kWgQuads) > 65535) return GS_E_BADARG;
  return GS_OK;
}

// strips of kStrip output rows `dil` apart that cover Ho rows: per residue class ceil(Ho / dil) rows
inline int dw_strips(int ho, int dil, int strip) { return dil * (int)ceil_div(ceil_div(ho, dil), strip); }

inline int dw_out(const gs_dwconv_desc* d, int in) { return in + 2 * d->pad - (d->KH - 1) * d->dil; }

int launch_stencil(DwStencil a, int k, const float* in, const float* w, const float* bias, float* out,
                   void* stream) {
  a.strips = dw_strips(a.Ho, a.dil, k == kK7 ? kStrip7 : kStrip);
  const int64_t items = (int64_t)a.N * a.strips * a.Wo * a.C4;
  const dim3 grid(stream_grid(items, 256));
  if (k == kK7)
    hipLaunchKernelGGL(dw7_stencil_kernel, grid, dim3(256), 0, as_stream(stream), a, in, w, bias, out, items);
  else
    hipLaunchKernelGGL(dw_stencil_kernel, grid, dim3(256), 0, as_stream(stream), a, in, w, bias, out, items);
  return launch_status();
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_dwconv2d_workspace_bytes(const gs_dwconv_desc* d) {
  if (dw_check(d) != GS_OK) return 0;
  const int64_t runs = ceil_div((int64_t)d->N * dw_out(d, d->H) * dw_out(d, d->W), kWgPixels);
  return (size_t)runs * d->KH * d->KW * d->C * sizeof(float);
}

extern "C" int gs_dwconv2d_forward(const gs_dwconv_desc* d, const float* x, const float* w,
                                   const float* bias, float* y, void* stream) {
  const int rc = dw_check(d);
  if (rc != GS_OK) return rc;
  if (!x || !w || !y) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(w) || !aligned16(y) || !aligned16(bias)) return GS_E_ALIGN;
  DwStencil a;
  a.N = d->N; a.Hi = d->H; a.Wi = d->W; a.Ho = dw_out(d, d->H); a.Wo = dw_out(d, d->W);
  a.C4 = d->C / 4; a.ldi = d->ldx; a.ldo = d->ldy; a.ldw = d->C_ld;
  a.dil = d->dil; a.off = d->pad; a.flip = 0; a.accumulate = 0;
  return launch_stencil(a, d->KH, x, w, bias, y, stream);
}

extern "C" int gs_dwconv2d_dgrad(const gs_dwconv_desc* d, const float* dy, const float* w, float* dx,
                                 int accumulate, void* stream) {
  const int rc = dw_check(d);
  if (rc != GS_OK) return rc;
  if (!dy || !w || !dx) return GS_E_NULL;
  if (!aligned16(dy) || !aligned16(w) || !aligned16(dx)) return GS_E_ALIGN;
  // dx[h] = sum_k dy[h + pad - k * dil] w[k] = sum_k' dy[h + k' * dil - ((K-1) * dil - pad)] w[K-1 - k']
  DwStencil a;
  a.N = d->N; a.Hi = dw_out(d, d->H); a.Wi = dw_out(d, d->W); a.Ho = d->H; a.Wo = d->W;
  a.C4 = d->C / 4; a.ldi = d->ldy; a.ldo = d->ldx; a.ldw = d->C_ld;
  a.dil = d->dil; a.off = (d->KH - 1) * d->dil - d->pad; a.flip = 1; a.accumulate = accumulate ? 1 : 0;
  return launch_stencil(a, d->KH, dy, w, nullptr, dx, stream);
}

extern "C" int gs_dwconv2d_wgrad(const gs_dwconv_desc* d, const float* x, const float* dy, float* dw,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = dw_check(d);
  if (rc != GS_OK) return rc;
  if (!x || !dy || !dw || !workspace) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(dw) || !aligned16(workspace)) return GS_E_ALIGN;
  if (workspace_bytes < gs_dwconv2d_workspace_bytes(d)) return GS_E_WORKSPACE;
  DwWgrad a;
  a.H = d->H; a.W = d->W; a.Ho = dw_out(d, d->H); a.Wo = dw_out(d, d->W);
  a.C4 = d->C / 4; a.C = d->C; a.ldx = d->ldx; a.ldy = d->ldy; a.ldw = d->C_ld;
  a.dil = d->dil; a.pad = d->pad;
  a.pixels = (int64_t)d->N * a.Ho * a.Wo;
  a.runs = (int32_t)ceil_div(a.pixels, kWgPixels);
  a.taps = d->KH * d->KW;
  const unsigned groups = (unsigned)ceil_div(a.C4, kWgQuads);
  float* part = static_cast<float*>(workspace);
  if (d->KH == kK7)
    hipLaunchKernelGGL(dw7_wgrad_partial_kernel, dim3((unsigned)a.runs, groups, kK7), dim3(256), 0,
                       as_stream(stream), a, x, dy, part);
  else
    hipLaunchKernelGGL(dw_wgrad_partial_kernel, dim3((unsigned)a.runs, groups), dim3(256), 0,
                       as_stream(stream), a, x, dy, part);
  hipLaunchKernelGGL(dw_wgrad_sum_kernel, dim3(groups, (unsigned)a.taps), dim3(256), 0, as_stream(stream), a,
                     part, dw);
  return launch_status();
}
