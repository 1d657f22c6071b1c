// ConvNeXt V2's Global Response Normalization fused with the GELU in front of it, on NHWC fp32
// (include/gaiaseg_hip.h): a = gelu(x) never exists in memory.
//
//   G[n,c]  = sqrt(sum_p a[n,p,c]^2),   Nx[n,c] = G[n,c] / (mean_c G[n,:] + eps),
//   y[n,p,c] = a[n,p,c] * (1 + weight[c] * Nx[n,c]) + bias[c]
//
// The operand is the widest tensor of the block ([N, P, 4C]) and every kernel here is bandwidth-bound.
// Forward, two passes over it: per-(sample, channel) partial sums of a^2 over runs of kRunRows pixels
// (the runs are cut per sample: run r of sample n covers pixels r * kRunRows .. of that sample only),
// their ordered sum to G, and the apply pass, whose prologue takes the mean of the sample's G.
// Backward, two passes: the partials of S = sum_p dy * a and T = sum_p dy, their ordered sum, one
// workgroup that turns S, T and G into the coefficients A = 1 + weight * Nx and B = dG / G of every
// (n, c) and into dweight / dbias (samples added in order), and dx = (dy * A + a * B) * gelu'(x).
// One thread owns float4 channel quads; the column reductions use the 16 quads x 16 row lanes
// workgroup of csrc/rowwise.h.  No atomics, every sum has a fixed order.
#include "rowwise.h"

namespace gs {
namespace {

struct GrnArgs {
  int64_t P, items;            // pixels per sample; items = P * C4 quads per sample
  int32_t N, C, C4, R;         // R = runs per sample
  int32_t ldx, ldy, lddy, lddx;
  float eps, inv_c;
};

// sum over the 256 threads of a workgroup, every thread gets it: butterflies inside the four waves,
// then the four wave sums in order
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = group_sum(v, kWave);
  __syncthreads();               // sh may still be read from an earlier call
  if (threadIdx.x % kWave == 0) sh[threadIdx.x / kWave] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ f32x4 sqrt4(f32x4 v) { return f32x4{sqrtf(v.x), sqrtf(v.y), sqrtf(v.z), sqrtf(v.w)}; }

// stage 1: grid (N * R, quad groups).  kBackward == 0: plane 0 = sum gelu(x)^2.
// kBackward == 1: plane 0 = sum dy * gelu(x), plane 1 = sum dy.  part is [N][R][planes][C].
template <int kBackward>
__global__ __launch_bounds__(256) void grn_partial_kernel(const GrnArgs a, const float* __restrict__ x,
                                                          const float* __restrict__ dy,
                                                          float* __restrict__ part) {
  constexpr int kPlanes = kBackward ? 2 : 1;
  __shared__ f32x4 sh[kPlanes][kColLanes][kColQuads];
  const int ql = threadIdx.x % kColQuads, pl = threadIdx.x / kColQuads;
  const int cq = blockIdx.y * kColQuads + ql;
  const int64_t n = blockIdx.x / a.R, p0 = (int64_t)(blockIdx.x % a.R) * kRunRows;
  f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
  if (cq < a.C4) {
    for (int i = 0; i < kRunRows / kColLanes; ++i) {
      const int64_t p = p0 + i * kColLanes + pl;
      if (p >= a.P) break;
      const int64_t row = n * a.P + p;
      const f32x4 v = gelu_fwd4(ld4(x + row * a.ldx + cq * 4));
      if (kBackward) {
        const f32x4 g = ld4(dy + row * a.lddy + cq * 4);
        s0 += g * v;
        s1 += g;
      } else {
        s0 += v * v;
      }
    }
  }
  sh[0][pl][ql] = s0;
  if (kBackward) sh[kPlanes - 1][pl][ql] = s1;
  __syncthreads();
  if (threadIdx.x < kPlanes * kColQuads && cq < a.C4) {
    const int k = threadIdx.x / kColQuads;
    f32x4 s = sh[k][0][ql];
#pragma unroll
    for (int l = 1; l < kColLanes; ++l) s += sh[k][l][ql];
    st4(part + ((int64_t)blockIdx.x * kPlanes + k) * a.C + cq * 4, s);
  }
}

// stage 2: grid (quad groups, planes, N).  Lane l sums runs l, l + 16, ... of its sample in order, then
// the 16 lane sums are added in order.  out is [N][planes][C]; kSqrt stores the root (G).
template <int kSqrt>
__global__ __launch_bounds__(256) void grn_runs_sum_kernel(const GrnArgs a, const int planes,
                                                           const float* __restrict__ part,
                                                           float* __restrict__ out) {
  __shared__ f32x4 sh[kColLanes][kColQuads];
  const int ql = threadIdx.x % kColQuads, pl = threadIdx.x / kColQuads;
  const int cq = blockIdx.x * kColQuads + ql;
  const int k = blockIdx.y;
  const int64_t n = blockIdx.z;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cq < a.C4)
    for (int r = pl; r < a.R; r += kColLanes) s += ld4(part + ((n * a.R + r) * planes + k) * a.C + cq * 4);
  sh[pl][ql] = s;
  __syncthreads();
  if (pl == 0 && cq < a.C4) {
    f32x4 t = sh[0][ql];
#pragma unroll
    for (int l = 1; l < kColLanes; ++l) t += sh[l][ql];
    st4(out + (n * planes + k) * a.C + cq * 4, kSqrt ? sqrt4(t) : t);
  }
}

// the apply pass: grid (workgroups per sample, N).  Every workgroup of a sample takes the same mean of G
// in the same order.
__global__ __launch_bounds__(256) void grn_apply_kernel(const GrnArgs a, const float* __restrict__ x,
                                                        const float* __restrict__ weight,
                                                        const float* __restrict__ bias,
                                                        const float* __restrict__ G, float* __restrict__ y) {
  __shared__ float sh[4];
  const int64_t n = blockIdx.y;
  const float* g = G + n * a.C;
  float s = 0.f;
  for (int q = threadIdx.x; q < a.C4; q += 256) s += hsum(ld4(g + q * 4));
  const float inv = 1.0f / (block_sum(s, sh) * a.inv_c + a.eps);
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < a.items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    const int64_t row = n * a.P + it / a.C4;
    const f32x4 v = gelu_fwd4(ld4(x + row * a.ldx + cq * 4));
    const f32x4 scale = 1.0f + ld4(weight + cq * 4) * (ld4(g + cq * 4) * inv);
    st4(y + row * a.ldy + cq * 4, v * scale + ld4(bias + cq * 4));
  }
}

// one workgroup: for every sample in order, m = mean_c G + eps and k2 = sum_c D * G / (C m^2) with
// D = weight * S; then coef[n][0][c] = A = 1 + weight * G / m, coef[n][1][c] = B = (D / m - k2) / G (0 where
// G == 0, torch's convention for the 2-norm), dweight += (G / m) * S, dbias += T.  st is [N][2][C] (S, T).
__global__ __launch_bounds__(256) void grn_coef_kernel(const GrnArgs a, const float* __restrict__ weight,
                                                       const float* __restrict__ G,
                                                       const float* __restrict__ st, float* __restrict__ coef,
                                                       float* dweight, float* dbias) {
  __shared__ float sh[4];
  for (int64_t n = 0; n < a.N; ++n) {
    const float* g = G + n * a.C;
    const float* S = st + n * 2 * a.C;
    const float* T = S + a.C;
    float sg = 0.f, sd = 0.f;
    for (int q = threadIdx.x; q < a.C4; q += 256) {
      const f32x4 gq = ld4(g + q * 4);
      sg += hsum(gq);
      sd += hsum(ld4(weight + q * 4) * ld4(S + q * 4) * gq);
    }
    const float m = block_sum(sg, sh) * a.inv_c + a.eps;
    const float inv = 1.0f / m;
    const float k2 = block_sum(sd, sh) * a.inv_c * inv * inv;
    for (int q = threadIdx.x; q < a.C4; q += 256) {
      const f32x4 gq = ld4(g + q * 4), w = ld4(weight + q * 4), s = ld4(S + q * 4);
      const f32x4 nx = gq * inv;
      const f32x4 dg = w * s * inv - k2;
      const f32x4 b = f32x4{gq.x > 0.f ? dg.x / gq.x : 0.f, gq.y > 0.f ? dg.y / gq.y : 0.f,
                            gq.z > 0.f ? dg.z / gq.z : 0.f, gq.w > 0.f ? dg.w / gq.w : 0.f};
      st4(coef + n * 2 * a.C + q * 4, 1.0f + w * nx);
      st4(coef + (n * 2 + 1) * a.C + q * 4, b);
      const f32x4 dw = nx * s, db = ld4(T + q * 4);
      // the same thread owns quad q for every sample: its read-add-write sequence is ordered
      st4(dweight + q * 4, n ? ld4(dweight + q * 4) + dw : dw);
      st4(dbias + q * 4, n ? ld4(dbias + q * 4) + db : db);
    }
  }
}

// dx = (dy * A + gelu(x) * B) * gelu'(x).  dx may be dy's buffer: an element is read and written by the
// same thread.
__global__ __launch_bounds__(256) void grn_dx_kernel(const GrnArgs a, const float* __restrict__ x,
                                                     const float* dy, const float* __restrict__ coef,
                                                     float* dx) {
  const int64_t total = a.items * a.N;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    const int64_t row = it / a.C4, n = row / a.P;
    const f32x4 v = ld4(x + row * a.ldx + cq * 4);
    const f32x4 g = ld4(dy + row * a.lddy + cq * 4);
    const f32x4 A = ld4(coef + n * 2 * a.C + cq * 4), B = ld4(coef + (n * 2 + 1) * a.C + cq * 4);
    st4(dx + row * a.lddx + cq * 4, (g * A + gelu_fwd4(v) * B) * gelu_grad4(v));
  }
}

int grn_check(const gs_gelu_grn_desc* d) {
  if (!d) return GS_E_NULL;
  if (d->N <= 0 || d->P <= 0) return GS_E_BADARG;
  const int32_t ld[4] = {d->ldx, d->ldy, d->lddy, d->lddx};
  const int rc = rows_check((int64_t)d->N * d->P, d->C, ld, 4);
  if (rc != GS_OK) return rc;
  if (!(d->eps > 0.f)) return GS_E_BADARG;
  // grid limits: N * runs in x, N in z
  if ((int64_t)d->N * ceil_div(d->P, kRunRows) > INT32_MAX || d->N > 65535) return GS_E_BADARG;
  return GS_OK;
}

GrnArgs grn_args(const gs_gelu_grn_desc* d) {
  GrnArgs a;
  a.N = d->N; a.P = d->P; a.C = d->C; a.C4 = d->C / 4;
  a.items = a.P * a.C4;
  a.R = (int32_t)ceil_div(d->P, kRunRows);
  a.ldx = d->ldx; a.ldy = d->ldy; a.lddy = d->lddy; a.lddx = d->lddx;
  a.eps = d->eps; a.inv_c = 1.0f / (float)d->C;
  return a;
}

// floats: partials [N][R][2][C], then their sums [N][2][C], then the coefficients [N][2][C]
size_t grn_bytes(const gs_gelu_grn_desc* d) {
  return (size_t)d->N * d->C * (2 * (size_t)ceil_div(d->P, kRunRows) + 4) * sizeof(float);
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_gelu_grn_workspace_bytes(const gs_gelu_grn_desc* d) {
  return grn_check(d) == GS_OK ? grn_bytes(d) : 0;
}

extern "C" int gs_gelu_grn_forward(const gs_gelu_grn_desc* d, const float* x, const float* weight,
                                   const float* bias, float* y, float* G, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const int rc = grn_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({x, weight, bias, y, G, workspace})) return GS_E_NULL;
  if (!all_aligned16({x, weight, bias, y, G, workspace})) return GS_E_ALIGN;
  if (workspace_bytes < grn_bytes(d)) return GS_E_WORKSPACE;
  const GrnArgs a = grn_args(d);
  const unsigned groups = (unsigned)ceil_div(a.C4, kColQuads);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(grn_partial_kernel<0>, dim3((unsigned)(a.N * a.R), groups), dim3(256), 0,
                     as_stream(stream), a, x, static_cast<const float*>(nullptr), part);
  hipLaunchKernelGGL(grn_runs_sum_kernel<1>, dim3(groups, 1, (unsigned)a.N), dim3(256), 0, as_stream(stream),
                     a, 1, part, G);
  const int per_sample = (stream_grid(a.items * a.N, 256) + a.N - 1) / a.N;
  hipLaunchKernelGGL(grn_apply_kernel, dim3((unsigned)per_sample, (unsigned)a.N), dim3(256), 0,
                     as_stream(stream), a, x, weight, bias, G, y);
  return launch_status();
}

extern "C" int gs_gelu_grn_backward(const gs_gelu_grn_desc* d, const float* x, const float* dy,
                                    const float* weight, const float* G, float* dx, float* dweight,
                                    float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = grn_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({x, dy, weight, G, dx, dweight, dbias, workspace})) return GS_E_NULL;
  if (!all_aligned16({x, dy, weight, G, dx, dweight, dbias, workspace})) return GS_E_ALIGN;
  if (workspace_bytes < grn_bytes(d)) return GS_E_WORKSPACE;
  const GrnArgs a = grn_args(d);
  const unsigned groups = (unsigned)ceil_div(a.C4, kColQuads);
  float* part = static_cast<float*>(workspace);
  float* st = part + (size_t)a.N * a.R * 2 * a.C;
  float* coef = st + (size_t)a.N * 2 * a.C;
  // S and T read dy before dx (which may be dy's buffer) is written
  hipLaunchKernelGGL(grn_partial_kernel<1>, dim3((unsigned)(a.N * a.R), groups), dim3(256), 0,
                     as_stream(stream), a, x, dy, part);
  hipLaunchKernelGGL(grn_runs_sum_kernel<0>, dim3(groups, 2, (unsigned)a.N), dim3(256), 0, as_stream(stream),
                     a, 2, part, st);
  hipLaunchKernelGGL(grn_coef_kernel, dim3(1), dim3(256), 0, as_stream(stream), a, weight, G, st, coef,
                     dweight, dbias);
  hipLaunchKernelGGL(grn_dx_kernel, dim3(stream_grid(a.items * a.N, 256)), dim3(256), 0, as_stream(stream),
                     a, x, dy, coef, dx);
  return launch_status();
}
