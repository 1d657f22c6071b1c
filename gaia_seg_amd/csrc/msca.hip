// SegNeXt's multi-scale convolutional attention (MSCAN's spatial gating unit without its 1x1 conv) on
// NHWC fp32, forward and backward, and the elementwise gate that follows it (gs_msca_* and gs_gate_mul_*
// in include/gaiaseg_hip.h):
//
//   a   = dw K0xK0 (x) + b0                                         (K0 = 5)
//   r_i = dw 1xK_i (a) + b_row_i,  i = 0..2                         (K = 7, 11, 21)
//   s   = a + sum_i ( dw K_ix1 (r_i) + b_col_i )
//
// Nothing here reduces over channels, so every kernel is bandwidth-bound and follows dwconv.hip: one
// thread owns one float4 channel quad, consecutive lanes own consecutive quads of one pixel, reuse
// along the filter's axis happens in registers, taps in the zero padding are skipped, and every sum has
// a fixed order (no atomics).
//
// The strip filters are 1-D, so ONE device function does all twelve of them: conv1d computes kS
// consecutive outputs of a line from the kS + K - 1 inputs they touch (each loaded once), along H or W
// (the axis is a pitch), with the taps as stored or mirrored (the data gradient).  A filter of K taps
// runs in the smallest of the three instantiated widths (7, 11, 21) that holds it, centred, the other
// slots zero and the inputs only they would touch not loaded.
//
//   forward  (3 launches, 10 tensor passes):
//     stencil : x -> a                          1 read, 1 write     (the 7x7 kernel of dwconv.hip in K)
//     split   : a -> r_0, r_1, r_2              1 read, 3 writes
//     merge   : a, r_0..2 -> s                  4 reads, 1 write
//   a and the three r_i are the `saved` buffer of the backward (4 tensors, gs_msca_saved_bytes).
//   backward (7 launches; 21 tensor passes, 22 when dx is added to, counting every tensor a launch touches
//   once -- the filter-gradient launches re-read theirs from the caches, see below):
//     split^T  : ds -> dr_0..2 (columns, mirrored)              1 read, 3 writes
//     wgrad    : (ds, r_i) -> partials of d w_col_i, d b_col_i  4 reads
//     merge^T  : ds, dr_0..2 -> da (rows, mirrored)             4 reads, 1 write
//     wgrad    : (dr_i, a) -> partials of d w_row_i, d b_row_i  4 reads
//     wgrad0   : (da, x) -> partials of d w0, d b0              2 tensors: the K0 tap-row workgroups of a run
//                                                                each read da once and K0 taps of x per pixel
//                                                                (K0 and K0 * K0 loads per pixel, all but the
//                                                                first touch of a line from L1 / L2)
//     stencil^T: da -> dx (written or added to)                 1 read, 1 write (+1 read to accumulate)
//     sum      : partials -> the 14 gradients, runs added in a fixed order
//   dr_0..2, da and the partials live in the workspace.  The unfused chain of seven convolutions and
//   three adds moves 17 passes forward (7 x 2 + 3) and about 46 backward (per conv a data gradient,
//   2 passes, a filter gradient, 2, and a bias gradient, 1, plus the gradient adds).
#include "common.h"

namespace gs {
namespace {

constexpr int kS = 8;            // outputs of one line per thread (strip filters and the square stencil)
constexpr int kQuads = 16;       // channel quads per filter-gradient workgroup (256 contiguous bytes)
constexpr int kLanes = 16;       // pixel / strip lanes per filter-gradient workgroup
constexpr int kRunStrips = 32;   // strips per run of the strip filters' gradient (2 per lane, <= 256 pixels)
constexpr int kRunPixels = 256;  // pixels per run of the square filter's gradient (16 per lane)
constexpr int kChunk = 8;        // taps per round of the workgroup's LDS sum (32 KiB)
constexpr int kMaxK0 = 7, kMaxK = 21;
constexpr int kFilters = 14;

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// ---- 1-D building blocks ------------------------------------------------------------------------
// acc[o] += sum_k in[(pos0 + o + k - K/2) * pitch] * w[(flip ? K - 1 - k : k) * ldw], o = 0..kS-1; positions
// outside [0, L) are the zero padding.  Per output the products are added in the order of k.
template <int KM>
__device__ __forceinline__ void conv1d(f32x4 (&acc)[kS], const float* __restrict__ in, int pos0, int L,
                                       int64_t pitch, const float* __restrict__ w, int ldw, int K,
                                       int flip) {
  const int shift = (KM - K) / 2;   // the K taps sit in the middle of KM slots
  f32x4 wt[KM];
#pragma unroll
  for (int t = 0; t < KM; ++t) {
    const int k = t - shift;
    wt[t] = (k >= 0 && k < K) ? ld4(w + (int64_t)(flip ? K - 1 - k : k) * ldw) : zero4();
  }
#pragma unroll
  for (int j = 0; j < kS + KM - 1; ++j) {
    const int pos = pos0 + j - KM / 2;
    // (inputs that only empty slots would touch are not loaded)
    const bool ok = pos >= 0 && pos < L && j >= shift && j <= shift + K + kS - 2;
    const f32x4 v = ok ? ld4(in + (int64_t)pos * pitch) : zero4();
#pragma unroll
    for (int t = 0; t < KM; ++t) {
      const int o = j - t;
      if (o >= 0 && o < kS) acc[o] += v * wt[t];
    }
  }
}

// accw[t] += sum_o g[o] * in[(pos0 + o + t - KM/2) * pitch]: the filter gradient of the same strip (slot t
// is tap t - (KM - K) / 2; the slots beside the K taps collect products nobody reads).
template <int KM>
__device__ __forceinline__ void wgrad1d(f32x4 (&accw)[KM], const f32x4 (&g)[kS],
                                        const float* __restrict__ in, int pos0, int L, int64_t pitch,
                                        int K) {
  const int shift = (KM - K) / 2;
#pragma unroll
  for (int j = 0; j < kS + KM - 1; ++j) {
    const int pos = pos0 + j - KM / 2;
    const bool ok = pos >= 0 && pos < L && j >= shift && j <= shift + K + kS - 2;
    const f32x4 v = ok ? ld4(in + (int64_t)pos * pitch) : zero4();
#pragma unroll
    for (int t = 0; t < KM; ++t) {
      const int o = j - t;
      if (o >= 0 && o < kS) accw[t] += v * g[o];
    }
  }
}

__device__ __forceinline__ void conv_any(f32x4 (&acc)[kS], const float* in, int pos0, int L, int64_t pitch,
                                         const float* w, int ldw, int K, int flip) {
  if (K <= 7) conv1d<7>(acc, in, pos0, L, pitch, w, ldw, K, flip);
  else if (K <= 11) conv1d<11>(acc, in, pos0, L, pitch, w, ldw, K, flip);
  else conv1d<21>(acc, in, pos0, L, pitch, w, ldw, K, flip);
}

// One 1-D pass over a [N, H, W, C4] map in strips of kS positions of a line.
struct Strip {
  int32_t N, H, W, C4;
  int32_t axis;            // 0: the lines are columns (strips along H), 1: rows (along W)
  int32_t flip;            // mirrored taps (data gradient)
  int32_t ldw;             // tap pitch of the filters
  int32_t K[3];
  int32_t strips;          // strips per line
};

struct Ptr3 { const float* p[3]; };
struct Out3 { float* p[3]; };

// strip sid -> first position, line length, pixel index of the line's position 0, pixels per position
__device__ __forceinline__ void strip_decode(const Strip& a, int64_t sid, int& pos0, int& L, int64_t& pix0,
                                             int& step) {
  if (a.axis == 0) {
    const int w = (int)(sid % a.W);
    sid /= a.W;
    pos0 = (int)(sid % a.strips) * kS;
    pix0 = (sid / a.strips) * a.H * a.W + w;
    L = a.H;
    step = a.W;
  } else {
    pos0 = (int)(sid % a.strips) * kS;
    pix0 = (sid / a.strips) * a.W;   // sid / strips = n * H + h
    L = a.W;
    step = 1;
  }
}

// out_i = filter_i(in) + bias_i, i = 0..2
__global__ __launch_bounds__(256) void msca_split_kernel(const Strip a, const float* __restrict__ in,
                                                         const int ldi, const Ptr3 w, const Ptr3 bias,
                                                         const Out3 out, const int ldo, const int64_t items) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    int pos0, L, step;
    int64_t pix0;
    strip_decode(a, it / a.C4, pos0, L, pix0, step);
    const float* line = in + pix0 * ldi + cq * 4;
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
      const f32x4 b = bias.p[i] ? ld4(bias.p[i] + cq * 4) : zero4();
      f32x4 acc[kS];
#pragma unroll
      for (int j = 0; j < kS; ++j) acc[j] = b;
      conv_any(acc, line, pos0, L, (int64_t)step * ldi, w.p[i] + cq * 4, a.ldw, a.K[i], a.flip);
      float* o = out.p[i] + pix0 * ldo + cq * 4;
#pragma unroll
      for (int j = 0; j < kS; ++j) {
        if (pos0 + j >= L) break;
        st4(o + (int64_t)(pos0 + j) * step * ldo, acc[j]);
      }
    }
  }
}

// out = base + sum_i ( filter_i(in_i) + bias_i )
__global__ __launch_bounds__(256) void msca_merge_kernel(const Strip a, const float* __restrict__ base,
                                                         const int ldb, const Ptr3 in, const int ldi,
                                                         const Ptr3 w, const Ptr3 bias,
                                                         float* __restrict__ out, const int ldo,
                                                         const int64_t items) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    int pos0, L, step;
    int64_t pix0;
    strip_decode(a, it / a.C4, pos0, L, pix0, step);
    f32x4 b = zero4();
#pragma unroll
    for (int i = 0; i < 3; ++i)
      if (bias.p[i]) b += ld4(bias.p[i] + cq * 4);
    f32x4 acc[kS];
    const float* bl = base + pix0 * ldb + cq * 4;
#pragma unroll
    for (int j = 0; j < kS; ++j)
      acc[j] = pos0 + j < L ? ld4(bl + (int64_t)(pos0 + j) * step * ldb) + b : zero4();
#pragma unroll 1
    for (int i = 0; i < 3; ++i)
      conv_any(acc, in.p[i] + pix0 * ldi + cq * 4, pos0, L, (int64_t)step * ldi, w.p[i] + cq * 4, a.ldw,
               a.K[i], a.flip);
    float* o = out + pix0 * ldo + cq * 4;
#pragma unroll
    for (int j = 0; j < kS; ++j) {
      if (pos0 + j >= L) break;
      st4(o + (int64_t)(pos0 + j) * step * ldo, acc[j]);
    }
  }
}

// The workgroup's sum of acc[t] over its kLanes lanes, in lane order, kChunk slots per round; slot t is
// written to dst[(t - shift) * C] where that is one of the K taps.
template <int KM>
__device__ __forceinline__ void reduce_taps(f32x4 (&acc)[KM], int shift, int K,
                                            f32x4 (*sh)[kLanes][kQuads], float* dst, int C, int cq,
                                            bool okq) {
  const int ql = threadIdx.x % kQuads, pl = threadIdx.x / kQuads;
#pragma unroll
  for (int k0 = 0; k0 < KM; k0 += kChunk) {
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kChunk; ++kk)
      if (k0 + kk < KM) sh[kk][pl][ql] = acc[k0 + kk];
    __syncthreads();
    if (threadIdx.x < kChunk * kQuads) {
      const int kk = threadIdx.x / kQuads;
      const int k = k0 + kk - shift;
      if (k0 + kk < KM && k >= 0 && k < K && okq) {
        f32x4 s = sh[kk][0][ql];
#pragma unroll
        for (int l = 1; l < kLanes; ++l) s += sh[kk][l][ql];
        st4(dst + (int64_t)k * C + cq * 4, s);
      }
    }
  }
}

// Filter and bias gradient of strip filter i = blockIdx.z over one run of strips:
// part[(run * ptaps + off_i + k) * C + c], the bias at k = K_i; off_i = sum_{i' < i} (K_i' + 1).
template <int KM>
__device__ __forceinline__ void wgrad_strip_body(const Strip& a, const float* __restrict__ g, int ldg,
                                                 const float* __restrict__ in, int ldi, float* part, int C,
                                                 int64_t total, int K, f32x4 (*sh)[kLanes][kQuads]) {
  const int ql = threadIdx.x % kQuads, pl = threadIdx.x / kQuads;
  const int cq = blockIdx.y * kQuads + ql;
  const bool okq = cq < a.C4;
  f32x4 accw[KM];
  f32x4 accb[1] = {zero4()};
#pragma unroll
  for (int t = 0; t < KM; ++t) accw[t] = zero4();
  if (okq) {
    for (int r = 0; r < kRunStrips / kLanes; ++r) {
      const int64_t sid = (int64_t)blockIdx.x * kRunStrips + r * kLanes + pl;
      if (sid >= total) break;
      int pos0, L, step;
      int64_t pix0;
      strip_decode(a, sid, pos0, L, pix0, step);
      const float* gl = g + pix0 * ldg + cq * 4;
      f32x4 gv[kS];
#pragma unroll
      for (int j = 0; j < kS; ++j) {
        gv[j] = pos0 + j < L ? ld4(gl + (int64_t)(pos0 + j) * step * ldg) : zero4();
        accb[0] += gv[j];
      }
      wgrad1d<KM>(accw, gv, in + pix0 * ldi + cq * 4, pos0, L, (int64_t)step * ldi, K);
    }
  }
  reduce_taps<KM>(accw, (KM - K) / 2, K, sh, part, C, cq, okq);
  reduce_taps<1>(accb, 0, 1, sh, part + (int64_t)K * C, C, cq, okq);
}

__global__ __launch_bounds__(256) void msca_wgrad_strip_kernel(const Strip a, const Ptr3 g, const int ldg,
                                                               const Ptr3 in, const int ldi,
                                                               float* __restrict__ part, const int C,
                                                               const int64_t total, const int ptaps) {
  __shared__ f32x4 sh[kChunk][kLanes][kQuads];
  const int i = blockIdx.z;
  const int K = a.K[i];
  int off = 0;
  for (int q = 0; q < i; ++q) off += a.K[q] + 1;
  float* dst = part + ((int64_t)blockIdx.x * ptaps + off) * C;
  if (K <= 7) wgrad_strip_body<7>(a, g.p[i], ldg, in.p[i], ldi, dst, C, total, K, sh);
  else if (K <= 11) wgrad_strip_body<11>(a, g.p[i], ldg, in.p[i], ldi, dst, C, total, K, sh);
  else wgrad_strip_body<21>(a, g.p[i], ldg, in.p[i], ldi, dst, C, total, K, sh);
}

// ---- the square filter: dwconv.hip's 7x7 kernels with the size as a template parameter ------------
struct Square {
  int32_t N, H, W, C4, C;
  int32_t ldi, ldo, ldw;
  int32_t flip, accumulate, strips;
  int64_t pixels;
};

template <int K>
__global__ __launch_bounds__(256) void msca_stencil_kernel(const Square a, const float* __restrict__ in,
                                                           const float* __restrict__ w,
                                                           const float* __restrict__ bias,
                                                           float* __restrict__ out, const int64_t items) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    int64_t r = it / a.C4;
    const int wo = (int)(r % a.W);
    r /= a.W;
    const int h0 = (int)(r % a.strips) * kS;
    const int64_t n = r / a.strips;
    f32x4 acc[kS];
    const f32x4 b = bias ? ld4(bias + cq * 4) : zero4();
#pragma unroll
    for (int j = 0; j < kS; ++j) acc[j] = b;
#pragma unroll 1
    for (int kw = 0; kw < K; ++kw) {
      const int wi = wo + kw - K / 2;
      if (wi < 0 || wi >= a.W) continue;
      f32x4 wt[K];
#pragma unroll
      for (int kh = 0; kh < K; ++kh) {
        const int k = kh * K + kw;
        wt[kh] = ld4(w + (int64_t)(a.flip ? K * K - 1 - k : k) * a.ldw + cq * 4);
      }
      const float* col = in + (n * a.H * a.W + wi) * a.ldi + cq * 4;
      f32x4 win[kS + K - 1];
#pragma unroll
      for (int j = 0; j < kS + K - 1; ++j) {
        const int hi = h0 + j - K / 2;
        win[j] = (hi >= 0 && hi < a.H) ? ld4(col + (int64_t)hi * a.W * a.ldi) : zero4();
      }
#pragma unroll
      for (int kh = 0; kh < K; ++kh)
#pragma unroll
        for (int j = 0; j < kS; ++j) acc[j] += win[j + kh] * wt[kh];
    }
#pragma unroll
    for (int j = 0; j < kS; ++j) {
      const int ho = h0 + j;
      if (ho >= a.H) break;
      float* p = out + ((n * a.H + ho) * a.W + wo) * a.ldo + cq * 4;
      st4(p, a.accumulate ? ld4(p) + acc[j] : acc[j]);
    }
  }
}

// grid (runs, quad groups, K tap rows): part[(run * (K*K + 1) + tap) * C + c], the bias (summed by the
// workgroups of tap row 0) at tap K*K.  ldi is x's pitch, ldo the gradient's.
template <int K>
__global__ __launch_bounds__(256) void msca_wgrad0_kernel(const Square a, const float* __restrict__ x,
                                                          const float* __restrict__ dy,
                                                          float* __restrict__ part) {
  __shared__ f32x4 sh[kChunk][kLanes][kQuads];
  const int ql = threadIdx.x % kQuads, pl = threadIdx.x / kQuads;
  const int cq = blockIdx.y * kQuads + ql;
  const bool okq = cq < a.C4;
  const int kh = blockIdx.z;
  const int64_t p0 = (int64_t)blockIdx.x * kRunPixels;
  f32x4 acc[K];
  f32x4 accb[1] = {zero4()};
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = zero4();
  if (okq) {
    for (int i = 0; i < kRunPixels / kLanes; ++i) {
      const int64_t pix = p0 + i * kLanes + pl;
      if (pix >= a.pixels) break;
      const int wo = (int)(pix % a.W);
      const int64_t t = pix / a.W;
      const int ho = (int)(t % a.H);
      const int64_t n = t / a.H;
      const f32x4 g = ld4(dy + pix * a.ldo + cq * 4);
      accb[0] += g;
      const int hi = ho + kh - K / 2;
      if (hi < 0 || hi >= a.H) continue;
      const float* row = x + (n * a.H + hi) * a.W * a.ldi + cq * 4;
#pragma unroll
      for (int kw = 0; kw < K; ++kw) {
        const int wi = wo + kw - K / 2;
        if (wi >= 0 && wi < a.W) acc[kw] += ld4(row + (int64_t)wi * a.ldi) * g;
      }
    }
  }
  float* dst = part + (int64_t)blockIdx.x * (K * K + 1) * a.C;
  reduce_taps<K>(acc, 0, K, sh, dst + (int64_t)kh * K * a.C, a.C, cq, okq);
  if (kh == 0) reduce_taps<1>(accb, 0, 1, sh, dst + (int64_t)K * K * a.C, a.C, cq, okq);
}

// ---- the last launch: runs -> gradients -----------------------------------------------------------
struct SumPlan {
  struct Entry {
    float* dst;          // the filter's (or bias's) max-size gradient
    int64_t off;         // floats from the workspace's partials to [run 0][this filter's tap 0]
    int32_t taps, runs;
    int32_t stride;      // taps per run of the region
    int32_t ldd;         // tap pitch of dst
  } e[kFilters];
  int32_t C4, C;
};

// grid (quad groups, all taps).  Lane l sums runs l, l + 16, ... in order, then the lane sums in order.
__global__ __launch_bounds__(256) void msca_sum_kernel(const SumPlan p, const float* __restrict__ part) {
  __shared__ f32x4 sh[kLanes][kQuads];
  const int ql = threadIdx.x % kQuads, pl = threadIdx.x / kQuads;
  const int cq = blockIdx.x * kQuads + ql;
  int t = blockIdx.y, f = 0;
  while (f < kFilters - 1 && t >= p.e[f].taps) t -= p.e[f++].taps;
  const float* src = part + p.e[f].off + (int64_t)t * p.C;
  const int runs = p.e[f].runs;
  const int64_t stride = (int64_t)p.e[f].stride * p.C;
  f32x4 s = zero4();
  if (cq < p.C4)
    for (int r = pl; r < runs; r += kLanes) s += ld4(src + r * stride + cq * 4);
  sh[pl][ql] = s;
  __syncthreads();
  if (pl == 0 && cq < p.C4) {
    f32x4 v = sh[0][ql];
#pragma unroll
    for (int l = 1; l < kLanes; ++l) v += sh[l][ql];
    st4(p.e[f].dst + (int64_t)t * p.e[f].ldd + cq * 4, v);
  }
}

// ---- gate ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_mul_forward_kernel(const float* __restrict__ g,
                                                               const float* __restrict__ u,
                                                               float* __restrict__ y, const int64_t items,
                                                               const int C4, const int ldg, const int ldu,
                                                               const int ldy) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int64_t r = it / C4;
    const int c = (int)(it % C4) * 4;
    st4(y + r * ldy + c, ld4(g + r * ldg + c) * ld4(u + r * ldu + c));
  }
}

__global__ __launch_bounds__(256) void gate_mul_backward_kernel(
    const float* __restrict__ dy, const float* __restrict__ g, const float* __restrict__ u, float* dg, float* du,
    const int64_t items, const int C4, const int lddy, const int ldg, const int ldu, const int lddg,
    const int lddu, const int accumulate) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int64_t r = it / C4;
    const int c = (int)(it % C4) * 4;
    const f32x4 d = ld4(dy + r * lddy + c);
    const f32x4 gu = d * ld4(g + r * ldg + c);
    const f32x4 gg = d * ld4(u + r * ldu + c);
    float* pu = du + r * lddu + c;
    st4(pu, accumulate ? ld4(pu) + gu : gu);
    st4(dg + r * lddg + c, gg);
  }
}

// ---- host ---------------------------------------------------------------------------------------
// Everything a call can get wrong, checked on the host before any launch.
int msca_check(const gs_msca_desc* d) {
  if (!d) return GS_E_NULL;
  if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0) return GS_E_BADARG;
  if (d->K0 < 1 || d->K0 > kMaxK0 || d->K0 % 2 == 0) return GS_E_BADARG;
  for (int i = 0; i < 3; ++i)
    if (d->K[i] < 1 || d->K[i] > kMaxK || d->K[i] % 2 == 0) return GS_E_BADARG;
  if (d->C % 4 || d->C_ld % 4 || d->ldx % 4 || d->lds % 4) return GS_E_ALIGN;
  if (d->C > d->C_ld || d->C > d->ldx || d->C > d->lds) return GS_E_BADARG;
  // pixel counts, run counts (grid.x) and quad groups (grid.y) within the launch limits
  if ((int64_t)d->N * d->H * d->W > INT32_MAX || ceil_div(d->C / 4, kQuads) > 65535) return GS_E_BADARG;
  return GS_OK;
}

inline int64_t msca_pixels(const gs_msca_desc* d) { return (int64_t)d->N * d->H * d->W; }
inline int msca_strip_taps(const gs_msca_desc* d) { return d->K[0] + d->K[1] + d->K[2] + 3; }

// The workspace: dr_0..2 and da, packed [P][C], then the partials of the square filter, of the column
// filters and of the row filters.  The strip regions are sized for one strip per pixel, which no map
// exceeds, so that the size depends on the pixel count alone.
struct Layout {
  int64_t tensor, part0, partc, partr, total;   // in floats
  int64_t runs0, runs_bound;
};

Layout msca_layout(const gs_msca_desc* d) {
  Layout l;
  const int64_t P = msca_pixels(d);
  l.tensor = P * d->C;
  l.runs0 = ceil_div(P, kRunPixels);
  l.runs_bound = ceil_div(P, kRunStrips);
  l.part0 = 4 * l.tensor;
  l.partc = l.part0 + l.runs0 * (d->K0 * d->K0 + 1) * d->C;
  l.partr = l.partc + l.runs_bound * msca_strip_taps(d) * d->C;
  l.total = l.partr + l.runs_bound * msca_strip_taps(d) * d->C;
  return l;
}

Strip make_strip(const gs_msca_desc* d, int axis, int flip) {
  Strip a;
  a.N = d->N; a.H = d->H; a.W = d->W; a.C4 = d->C / 4;
  a.axis = axis; a.flip = flip; a.ldw = d->C_ld;
  for (int i = 0; i < 3; ++i) a.K[i] = d->K[i];
  a.strips = (int)ceil_div(axis == 0 ? d->H : d->W, kS);
  return a;
}

inline int64_t strip_count(const Strip& a) {
  return (int64_t)a.N * a.strips * (a.axis == 0 ? a.W : a.H);
}

Square make_square(const gs_msca_desc* d, int ldi, int ldo, int flip, int accumulate) {
  Square a;
  a.N = d->N; a.H = d->H; a.W = d->W; a.C4 = d->C / 4; a.C = d->C;
  a.ldi = ldi; a.ldo = ldo; a.ldw = d->C_ld;
  a.flip = flip; a.accumulate = accumulate;
  a.strips = (int)ceil_div(d->H, kS);
  a.pixels = msca_pixels(d);
  return a;
}

void launch_stencil(const Square& a, int k0, const float* in, const float* w, const float* bias, float* out,
                    void* stream) {
  const int64_t items = (int64_t)a.N * a.strips * a.W * a.C4;
  const dim3 grid(stream_grid(items, 256));
  hipStream_t st = as_stream(stream);
  switch (k0) {
    case 1: hipLaunchKernelGGL(msca_stencil_kernel<1>, grid, dim3(256), 0, st, a, in, w, bias, out, items); break;
    case 3: hipLaunchKernelGGL(msca_stencil_kernel<3>, grid, dim3(256), 0, st, a, in, w, bias, out, items); break;
    case 5: hipLaunchKernelGGL(msca_stencil_kernel<5>, grid, dim3(256), 0, st, a, in, w, bias, out, items); break;
    default: hipLaunchKernelGGL(msca_stencil_kernel<7>, grid, dim3(256), 0, st, a, in, w, bias, out, items); break;
  }
}

void launch_wgrad0(const Square& a, int k0, unsigned runs, unsigned groups, const float* x, const float* dy,
                   float* part, void* stream) {
  const dim3 grid(runs, groups, (unsigned)k0);
  hipStream_t st = as_stream(stream);
  switch (k0) {
    case 1: hipLaunchKernelGGL(msca_wgrad0_kernel<1>, grid, dim3(256), 0, st, a, x, dy, part); break;
    case 3: hipLaunchKernelGGL(msca_wgrad0_kernel<3>, grid, dim3(256), 0, st, a, x, dy, part); break;
    case 5: hipLaunchKernelGGL(msca_wgrad0_kernel<5>, grid, dim3(256), 0, st, a, x, dy, part); break;
    default: hipLaunchKernelGGL(msca_wgrad0_kernel<7>, grid, dim3(256), 0, st, a, x, dy, part); break;
  }
}

bool filters_null(const gs_msca_filters* f) {
  if (!f || !f->w0 || !f->b0) return true;
  for (int i = 0; i < 3; ++i)
    if (!f->w_row[i] || !f->b_row[i] || !f->w_col[i] || !f->b_col[i]) return true;
  return false;
}

bool filters_aligned(const gs_msca_filters* f) {
  if (!aligned16(f->w0) || !aligned16(f->b0)) return false;
  for (int i = 0; i < 3; ++i)
    if (!aligned16(f->w_row[i]) || !aligned16(f->b_row[i]) || !aligned16(f->w_col[i]) ||
        !aligned16(f->b_col[i]))
      return false;
  return true;
}

int rows_check(int64_t rows, int32_t C, std::initializer_list<int32_t> lds) {
  if (rows <= 0 || C <= 0) return GS_E_BADARG;
  if (C % 4) return GS_E_ALIGN;
  for (int32_t ld : lds)
    if (ld % 4) return GS_E_ALIGN;
  for (int32_t ld : lds)
    if (ld < C) return GS_E_BADARG;
  return GS_OK;
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_msca_saved_bytes(const gs_msca_desc* d) {
  if (msca_check(d) != GS_OK) return 0;
  return (size_t)(4 * msca_pixels(d) * d->C) * sizeof(float);
}

extern "C" size_t gs_msca_workspace_bytes(const gs_msca_desc* d) {
  if (msca_check(d) != GS_OK) return 0;
  return (size_t)msca_layout(d).total * sizeof(float);
}

extern "C" int gs_msca_forward(const gs_msca_desc* d, const float* x, const gs_msca_filters* filters, float* s,
                               void* saved, void* stream) {
  const int rc = msca_check(d);
  if (rc != GS_OK) return rc;
  if (!x || !s || !saved || filters_null(filters)) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(s) || !aligned16(saved) || !filters_aligned(filters)) return GS_E_ALIGN;
  const int C = d->C;
  const int64_t T = msca_pixels(d) * C;
  float* a = static_cast<float*>(saved);
  const Out3 r = {{a + T, a + 2 * T, a + 3 * T}};
  const Ptr3 rc3 = {{a + T, a + 2 * T, a + 3 * T}};
  const Ptr3 wrow = {{filters->w_row[0], filters->w_row[1], filters->w_row[2]}};
  const Ptr3 brow = {{filters->b_row[0], filters->b_row[1], filters->b_row[2]}};
  const Ptr3 wcol = {{filters->w_col[0], filters->w_col[1], filters->w_col[2]}};
  const Ptr3 bcol = {{filters->b_col[0], filters->b_col[1], filters->b_col[2]}};
  hipStream_t st = as_stream(stream);
  launch_stencil(make_square(d, d->ldx, C, 0, 0), d->K0, x, filters->w0, filters->b0, a, stream);
  const Strip rows = make_strip(d, 1, 0);
  int64_t items = strip_count(rows) * rows.C4;
  hipLaunchKernelGGL(msca_split_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, st, rows, (const float*)a,
                     C, wrow, brow, r, C, items);
  const Strip cols = make_strip(d, 0, 0);
  items = strip_count(cols) * cols.C4;
  hipLaunchKernelGGL(msca_merge_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, st, cols, (const float*)a,
                     C, rc3, C, wcol, bcol, s, d->lds, items);
  return launch_status();
}

extern "C" int gs_msca_backward(const gs_msca_desc* d, const float* x, const float* ds,
                                const gs_msca_filters* filters, const void* saved, float* dx, int accumulate,
                                const gs_msca_filter_grads* grads, void* workspace, size_t workspace_bytes,
                                void* stream) {
  const int rc = msca_check(d);
  if (rc != GS_OK) return rc;
  if (!x || !ds || !saved || !dx || !workspace || filters_null(filters)) return GS_E_NULL;
  if (!grads || !grads->w0 || !grads->b0) return GS_E_NULL;
  for (int i = 0; i < 3; ++i)
    if (!grads->w_row[i] || !grads->b_row[i] || !grads->w_col[i] || !grads->b_col[i]) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(ds) || !aligned16(saved) || !aligned16(dx) || !aligned16(workspace) ||
      !filters_aligned(filters))
    return GS_E_ALIGN;
  if (!aligned16(grads->w0) || !aligned16(grads->b0)) return GS_E_ALIGN;
  for (int i = 0; i < 3; ++i)
    if (!aligned16(grads->w_row[i]) || !aligned16(grads->b_row[i]) || !aligned16(grads->w_col[i]) ||
        !aligned16(grads->b_col[i]))
      return GS_E_ALIGN;
  if (workspace_bytes < gs_msca_workspace_bytes(d)) return GS_E_WORKSPACE;

  const int C = d->C;
  const Layout l = msca_layout(d);
  const int64_t T = l.tensor;
  const float* a = static_cast<const float*>(saved);
  float* ws = static_cast<float*>(workspace);
  float* da = ws + 3 * T;
  const Out3 dr = {{ws, ws + T, ws + 2 * T}};
  const Ptr3 drc = {{ws, ws + T, ws + 2 * T}};
  const Ptr3 r = {{a + T, a + 2 * T, a + 3 * T}};
  const Ptr3 a3 = {{a, a, a}};
  const Ptr3 ds3 = {{ds, ds, ds}};
  const Ptr3 none = {{nullptr, nullptr, nullptr}};
  const Ptr3 wrow = {{filters->w_row[0], filters->w_row[1], filters->w_row[2]}};
  const Ptr3 wcol = {{filters->w_col[0], filters->w_col[1], filters->w_col[2]}};
  const unsigned groups = (unsigned)ceil_div(C / 4, kQuads);
  const int ptaps = msca_strip_taps(d);
  hipStream_t st = as_stream(stream);

  // columns: dr_i = filter_i^T(ds); d w_col_i, d b_col_i from (ds, r_i)
  const Strip cols = make_strip(d, 0, 1);
  const int64_t ncols = strip_count(cols);
  int64_t items = ncols * cols.C4;
  hipLaunchKernelGGL(msca_split_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, st, cols, ds, d->lds, wcol,
                     none, dr, C, items);
  const unsigned runs_c = (unsigned)ceil_div(ncols, kRunStrips);
  hipLaunchKernelGGL(msca_wgrad_strip_kernel, dim3(runs_c, groups, 3), dim3(256), 0, st, cols, ds3, d->lds, r, C,
                     ws + l.partc, C, ncols, ptaps);
  // rows: da = ds + sum_i filter_i^T(dr_i); d w_row_i, d b_row_i from (dr_i, a)
  const Strip rows = make_strip(d, 1, 1);
  const int64_t nrows = strip_count(rows);
  items = nrows * rows.C4;
  hipLaunchKernelGGL(msca_merge_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, st, rows, ds, d->lds, drc, C,
                     wrow, none, da, C, items);
  const unsigned runs_r = (unsigned)ceil_div(nrows, kRunStrips);
  hipLaunchKernelGGL(msca_wgrad_strip_kernel, dim3(runs_r, groups, 3), dim3(256), 0, st, rows, drc, C, a3, C,
                     ws + l.partr, C, nrows, ptaps);
  // the square filter: d w0, d b0 from (da, x); dx (+)= filter^T(da)
  launch_wgrad0(make_square(d, d->ldx, C, 0, 0), d->K0, (unsigned)l.runs0, groups, x, da, ws + l.part0,
                stream);
  launch_stencil(make_square(d, C, d->ldx, 1, accumulate ? 1 : 0), d->K0, da, filters->w0, nullptr, dx,
                 stream);

  SumPlan p;
  p.C4 = C / 4; p.C = C;
  int n = 0, total_taps = 0;
  auto add = [&](float* dst, int64_t off, int taps, int64_t runs, int stride, int ldd) {
    p.e[n].dst = dst; p.e[n].off = off; p.e[n].taps = taps; p.e[n].runs = (int32_t)runs;
    p.e[n].stride = stride; p.e[n].ldd = ldd;
    ++n;
    total_taps += taps;
  };
  const int t0 = d->K0 * d->K0;
  add(grads->w0, l.part0, t0, l.runs0, t0 + 1, d->C_ld);
  add(grads->b0, l.part0 + (int64_t)t0 * C, 1, l.runs0, t0 + 1, 0);
  int off = 0;
  for (int i = 0; i < 3; ++i) {
    add(grads->w_col[i], l.partc + (int64_t)off * C, d->K[i], runs_c, ptaps, d->C_ld);
    add(grads->b_col[i], l.partc + (int64_t)(off + d->K[i]) * C, 1, runs_c, ptaps, 0);
    add(grads->w_row[i], l.partr + (int64_t)off * C, d->K[i], runs_r, ptaps, d->C_ld);
    add(grads->b_row[i], l.partr + (int64_t)(off + d->K[i]) * C, 1, runs_r, ptaps, 0);
    off += d->K[i] + 1;
  }
  hipLaunchKernelGGL(msca_sum_kernel, dim3(groups, (unsigned)total_taps), dim3(256), 0, st, p, (const float*)ws);
  return launch_status();
}

extern "C" int gs_gate_mul_forward(const float* g, const float* u, float* y, int64_t rows, int32_t C,
                                   int32_t ldg, int32_t ldu, int32_t ldy, void* stream) {
  const int rc = rows_check(rows, C, {ldg, ldu, ldy});
  if (rc != GS_OK) return rc;
  if (!g || !u || !y) return GS_E_NULL;
  if (!aligned16(g) || !aligned16(u) || !aligned16(y)) return GS_E_ALIGN;
  const int64_t items = rows * (C / 4);
  hipLaunchKernelGGL(gate_mul_forward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream), g,
                     u, y, items, C / 4, ldg, ldu, ldy);
  return launch_status();
}

extern "C" int gs_gate_mul_backward(const float* dy, const float* g, const float* u, float* dg, float* du,
                                    int64_t rows, int32_t C, int32_t lddy, int32_t ldg, int32_t ldu,
                                    int32_t lddg, int32_t lddu, int accumulate, void* stream) {
  const int rc = rows_check(rows, C, {lddy, ldg, ldu, lddg, lddu});
  if (rc != GS_OK) return rc;
  if (!dy || !g || !u || !dg || !du) return GS_E_NULL;
  if (!aligned16(dy) || !aligned16(g) || !aligned16(u) || !aligned16(dg) || !aligned16(du)) return GS_E_ALIGN;
  const int64_t items = rows * (C / 4);
  hipLaunchKernelGGL(gate_mul_backward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream),
                     dy, g, u, dg, du, items, C / 4, lddy, ldg, ldu, lddg, lddu, accumulate ? 1 : 0);
  return launch_status();
}
