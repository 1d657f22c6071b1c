// Shared pieces of the "rows x C" pointwise operators (csrc/convnext_ops.hip, csrc/fcu.hip): float4
// access, the sum inside a lane group, exact-erf GELU, the argument check of a pitched row matrix, and
// stage 2 of the parameter-gradient column sums.
//
//   parameter grads  : a column sum over all rows runs in two stages.  Stage 1 (one kernel per operator)
//                      reduces runs of kRunRows rows to partials [run][plane][C] in the workspace
//                      (registers, then a fixed-order LDS sum over the 16 row lanes of a workgroup),
//                      stage 2 (col_runs_sum_kernel) sums the runs of every column in a fixed order.
//                      No atomics.
//
// Everything sits in an unnamed namespace: each translation unit that includes this gets its own copy.
#pragma once
#include "common.h"

namespace gs {
namespace {

constexpr int kColQuads = 16;     // channel quads per column-reduction workgroup (256 contiguous bytes)
constexpr int kColLanes = 16;     // row lanes per column-reduction workgroup
constexpr int kRunRows = 256;     // rows per stage-1 workgroup (16 per lane)

__device__ __forceinline__ float hsum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }

// sum over the G lanes of a group (G a power of two <= 64, groups aligned to G): every lane gets it
__device__ __forceinline__ float group_sum(float v, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

struct ColArgs {
  int64_t rows;
  int32_t C4, C, runs, planes;
  int32_t lda, ldb, ldc;
};

// stage 2: grid (quad groups, planes).  Lane l sums runs l, l + 16, ... in order, then the 16 lane sums
// are added in order.  Plane 0 goes to out0, plane 1 to out1.
__global__ __launch_bounds__(256) void col_runs_sum_kernel(const ColArgs a, const float* __restrict__ part,
                                                           float* __restrict__ out0,
                                                           float* __restrict__ out1) {
  __shared__ f32x4 sh[kColLanes][kColQuads];
  const int ql = threadIdx.x % kColQuads, pl = threadIdx.x / kColQuads;
  const int cq = blockIdx.x * kColQuads + ql;
  const int k = blockIdx.y;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cq < a.C4)
    for (int r = pl; r < a.runs; r += kColLanes) s += ld4(part + ((int64_t)r * a.planes + k) * a.C + cq * 4);
  sh[pl][ql] = s;
  __syncthreads();
  if (pl == 0 && cq < a.C4) {
    f32x4 t = sh[0][ql];
#pragma unroll
    for (int l = 1; l < kColLanes; ++l) t += sh[l][ql];
    st4((k == 0 ? out0 : out1) + cq * 4, t);
  }
}

// 0.5 * (1 + erf(x / sqrt 2)) and the normal density
__device__ __forceinline__ float gelu_cdf(float v) { return 0.5f * (1.0f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_fwd(float v) { return v * gelu_cdf(v); }
__device__ __forceinline__ float gelu_grad(float v) {
  return gelu_cdf(v) + v * 0.39894228040143268f * expf(-0.5f * v * v);
}
__device__ __forceinline__ f32x4 gelu_fwd4(f32x4 v) {
  return f32x4{gelu_fwd(v.x), gelu_fwd(v.y), gelu_fwd(v.z), gelu_fwd(v.w)};
}
__device__ __forceinline__ f32x4 gelu_grad4(f32x4 v) {
  return f32x4{gelu_grad(v.x), gelu_grad(v.y), gelu_grad(v.z), gelu_grad(v.w)};
}

// rows x C with pitches: sizes, float4 multiples, pitch >= C, and a column-reduction grid that fits
inline int rows_check(int64_t rows, int32_t c, const int32_t* ld, int n_ld) {
  if (rows <= 0 || c <= 0) return GS_E_BADARG;
  if (c % 4) return GS_E_ALIGN;
  for (int i = 0; i < n_ld; ++i)
    if (ld[i] % 4) return GS_E_ALIGN;
  for (int i = 0; i < n_ld; ++i)
    if (ld[i] < c) return GS_E_BADARG;
  if (ceil_div(rows, kRunRows) > INT32_MAX || ceil_div(c / 4, kColQuads) > 65535) return GS_E_BADARG;
  return GS_OK;
}

inline size_t col_bytes(int64_t rows, int32_t c, int planes) {
  return (size_t)ceil_div(rows, kRunRows) * planes * c * sizeof(float);
}

// lanes that share one row of C4 quads: the smallest power of two >= C4, at most a wave
inline int32_t row_group(int32_t C4) {
  int32_t g = 1;
  while (g < C4 && g < kWave) g *= 2;
  return g;
}

}  // namespace
}  // namespace gs
