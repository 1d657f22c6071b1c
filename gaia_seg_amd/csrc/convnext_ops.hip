// The ConvNeXt block's pointwise operators on NHWC fp32 (include/gaiaseg_hip.h): LayerNorm over the
// channels of a pixel, exact-erf GELU, and the per-channel layer scale fused with the residual add.
//
// All of them move a few bytes per flop and are bandwidth-bound; one thread owns float4 channel quads
// and consecutive lanes own consecutive quads of a pixel, so a wave's loads and stores are runs of
// contiguous 16-byte pieces.  Rows are pixels (N*H*W of them) with a pitch ld >= C.
//
//   LayerNorm        : a GROUP of G lanes owns one row, G the smallest power of two >= C/4, at most a
//                      wave (64).  A lane walks the quads lane, lane + G, ... of its row, so C is not
//                      bounded by the group; rows narrower than a wave share it (C = 96: two rows per
//                      wave).  Statistics are taken on x - x[row][0]: a common offset of the row cancels
//                      before anything is squared or summed, and a constant row gives exactly
//                      (0, 1/sqrt(eps)).  The variance is the mean of the squared CENTRED values (a second
//                      sweep over the row, served by L1), never E[x^2] - mean^2.  Sums inside a group
//                      are xor butterflies: a fixed order, and every lane gets the total.
//   parameter grads  : dweight / dbias of LayerNorm and dgamma of the layer scale are column sums over
//                      all rows, in the two stages of csrc/rowwise.h.  No atomics.
//   GELU, layer scale: grid-stride element-wise kernels.
#include "rowwise.h"

namespace gs {
namespace {

struct LnArgs {
  int64_t rows, row_blocks;   // row_blocks = ceil(rows / (256 / G))
  int32_t C4, ldx, ldy, G;
  float eps, inv_c;
  int32_t accumulate;
};

__global__ __launch_bounds__(256) void ln_forward_kernel(const LnArgs a, const float* __restrict__ x,
                                                         const float* __restrict__ weight,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ y, float* __restrict__ mean,
                                                         float* __restrict__ rstd) {
  const int G = a.G, gl = threadIdx.x % G, per_block = 256 / G;
  for (int64_t rb = blockIdx.x; rb < a.row_blocks; rb += gridDim.x) {
    const int64_t row = rb * per_block + threadIdx.x / G;
    const int c4 = row < a.rows ? a.C4 : 0;          // lanes of a row beyond the end only join the sums
    const float* xr = x + (row < a.rows ? row : 0) * a.ldx;
    const float x0 = xr[0];
    float s = 0.f;
    for (int q = gl; q < c4; q += G) s += hsum(ld4(xr + q * 4) - x0);
    const float m = group_sum(s, G) * a.inv_c;       // mean - x0
    float ss = 0.f;
    for (int q = gl; q < c4; q += G) {
      const f32x4 d = (ld4(xr + q * 4) - x0) - m;
      ss += hsum(d * d);
    }
    const float rs = 1.0f / sqrtf(group_sum(ss, G) * a.inv_c + a.eps);
    float* yr = y + row * a.ldy;
    for (int q = gl; q < c4; q += G) {
      const f32x4 d = (ld4(xr + q * 4) - x0) - m;
      st4(yr + q * 4, d * rs * ld4(weight + q * 4) + ld4(bias + q * 4));
    }
    if (gl == 0 && c4) {
      mean[row] = x0 + m;
      rstd[row] = rs;
    }
  }
}

// dx = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)),  g = dy * weight,  xhat = (x - mean) * rstd
__global__ __launch_bounds__(256) void ln_backward_dx_kernel(const LnArgs a, const float* __restrict__ x,
                                                             const float* dy,
                                                             const float* __restrict__ weight,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, float* dx) {
  const int G = a.G, gl = threadIdx.x % G, per_block = 256 / G;
  for (int64_t rb = blockIdx.x; rb < a.row_blocks; rb += gridDim.x) {
    const int64_t row = rb * per_block + threadIdx.x / G;
    const int c4 = row < a.rows ? a.C4 : 0;
    const int64_t r = row < a.rows ? row : 0;
    const float* xr = x + r * a.ldx;
    const float* gr = dy + r * a.ldy;
    const float mu = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
    for (int q = gl; q < c4; q += G) {
      const f32x4 g = ld4(gr + q * 4) * ld4(weight + q * 4);
      s1 += hsum(g);
      s2 += hsum(g * ((ld4(xr + q * 4) - mu) * rs));
    }
    const float m1 = group_sum(s1, G) * a.inv_c, m2 = group_sum(s2, G) * a.inv_c;
    float* dr = dx + r * a.ldx;
    for (int q = gl; q < c4; q += G) {
      const f32x4 g = ld4(gr + q * 4) * ld4(weight + q * 4);
      const f32x4 v = ((g - m1) - (ld4(xr + q * 4) - mu) * rs * m2) * rs;
      st4(dr + q * 4, a.accumulate ? ld4(dr + q * 4) + v : v);
    }
  }
}

// LayerNorm stage 1: grid (runs, quad groups).  plane 0 = sum dy * xhat (dweight), plane 1 = sum dy (dbias)
__global__ __launch_bounds__(256) void ln_param_partial_kernel(const ColArgs a, const float* __restrict__ x,
                                                               const float* __restrict__ dy,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ rstd,
                                                               float* __restrict__ part) {
  __shared__ f32x4 sh[2][kColLanes][kColQuads];
  const int ql = threadIdx.x % kColQuads, pl = threadIdx.x / kColQuads;
  const int cq = blockIdx.y * kColQuads + ql;
  const int64_t r0 = (int64_t)blockIdx.x * kRunRows;
  f32x4 aw = f32x4{0.f, 0.f, 0.f, 0.f}, ab = aw;
  if (cq < a.C4) {
    for (int i = 0; i < kRunRows / kColLanes; ++i) {
      const int64_t row = r0 + i * kColLanes + pl;
      if (row >= a.rows) break;
      const f32x4 g = ld4(dy + row * a.ldb + cq * 4);
      aw += g * ((ld4(x + row * a.lda + cq * 4) - mean[row]) * rstd[row]);
      ab += g;
    }
  }
  sh[0][pl][ql] = aw;
  sh[1][pl][ql] = ab;
  __syncthreads();
  if (threadIdx.x < 2 * kColQuads && cq < a.C4) {
    const int k = threadIdx.x / kColQuads;
    f32x4 s = sh[k][0][ql];
#pragma unroll
    for (int l = 1; l < kColLanes; ++l) s += sh[k][l][ql];
    st4(part + ((int64_t)blockIdx.x * 2 + k) * a.C + cq * 4, s);
  }
}

// Layer scale backward, stage 1 fused with dz: grid (runs, quad groups).  dz = gamma * dout for the
// rows of the run, and the run's partial of sum dout * z.  dz may be dout's or z's own buffer: an
// element is read and written by the same thread.
__global__ __launch_bounds__(256) void ls_backward_partial_kernel(const ColArgs a, const float* dout,
                                                                  const float* z,
                                                                  const float* __restrict__ gamma, float* dz,
                                                                  float* __restrict__ part) {
  __shared__ f32x4 sh[kColLanes][kColQuads];
  const int ql = threadIdx.x % kColQuads, pl = threadIdx.x / kColQuads;
  const int cq = blockIdx.y * kColQuads + ql;
  const int64_t r0 = (int64_t)blockIdx.x * kRunRows;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cq < a.C4) {
    const f32x4 gm = ld4(gamma + cq * 4);
    for (int i = 0; i < kRunRows / kColLanes; ++i) {
      const int64_t row = r0 + i * kColLanes + pl;
      if (row >= a.rows) break;
      const f32x4 g = ld4(dout + row * a.lda + cq * 4);
      acc += g * ld4(z + row * a.ldb + cq * 4);
      st4(dz + row * a.ldc + cq * 4, g * gm);
    }
  }
  sh[pl][ql] = acc;
  __syncthreads();
  if (pl == 0 && cq < a.C4) {
    f32x4 s = sh[0][ql];
#pragma unroll
    for (int l = 1; l < kColLanes; ++l) s += sh[l][ql];
    st4(part + (int64_t)blockIdx.x * a.C + cq * 4, s);
  }
}

__global__ __launch_bounds__(256) void gelu_forward_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           const int64_t items, const int C4, const int ldx,
                                                           const int ldy) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % C4);
    const int64_t row = it / C4;
    const f32x4 v = ld4(x + row * ldx + cq * 4);
    st4(y + row * ldy + cq * 4, f32x4{gelu_fwd(v.x), gelu_fwd(v.y), gelu_fwd(v.z), gelu_fwd(v.w)});
  }
}

// dx may be dy's own buffer
__global__ __launch_bounds__(256) void gelu_backward_kernel(const float* __restrict__ x, const float* dy,
                                                            float* dx, const int64_t items, const int C4,
                                                            const int ldx, const int lddy, const int lddx) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % C4);
    const int64_t row = it / C4;
    const f32x4 v = ld4(x + row * ldx + cq * 4);
    const f32x4 g = ld4(dy + row * lddy + cq * 4);
    st4(dx + row * lddx + cq * 4,
        g * f32x4{gelu_grad(v.x), gelu_grad(v.y), gelu_grad(v.z), gelu_grad(v.w)});
  }
}

// out may be identity's own buffer
__global__ __launch_bounds__(256) void ls_forward_kernel(const float* identity, const float* __restrict__ z,
                                                         const float* __restrict__ gamma, float* out,
                                                         const int64_t items, const int C4, const int ldi,
                                                         const int ldz, const int ldo) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % C4);
    const int64_t row = it / C4;
    st4(out + row * ldo + cq * 4,
        ld4(identity + row * ldi + cq * 4) + ld4(gamma + cq * 4) * ld4(z + row * ldz + cq * 4));
  }
}

int ln_check(const gs_layernorm_desc* d) {
  if (!d) return GS_E_NULL;
  const int32_t ld[2] = {d->ldx, d->ldy};
  const int rc = rows_check(d->rows, d->C, ld, 2);
  if (rc != GS_OK) return rc;
  if (!(d->eps > 0.f)) return GS_E_BADARG;
  return GS_OK;
}

LnArgs ln_args(const gs_layernorm_desc* d, int accumulate) {
  LnArgs a;
  a.rows = d->rows; a.C4 = d->C / 4; a.ldx = d->ldx; a.ldy = d->ldy;
  a.G = row_group(a.C4);
  a.row_blocks = ceil_div(d->rows, 256 / a.G);
  a.eps = d->eps; a.inv_c = 1.0f / (float)d->C;
  a.accumulate = accumulate ? 1 : 0;
  return a;
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_layernorm_workspace_bytes(const gs_layernorm_desc* d) {
  return ln_check(d) == GS_OK ? col_bytes(d->rows, d->C, 2) : 0;
}

extern "C" int gs_layernorm_forward(const gs_layernorm_desc* d, const float* x, const float* weight,
                                    const float* bias, float* y, float* mean, float* rstd, void* stream) {
  const int rc = ln_check(d);
  if (rc != GS_OK) return rc;
  if (!x || !weight || !bias || !y || !mean || !rstd) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(weight) || !aligned16(bias) || !aligned16(y)) return GS_E_ALIGN;
  const LnArgs a = ln_args(d, 0);
  const dim3 grid(stream_grid(a.row_blocks * 256, 256));
  hipLaunchKernelGGL(ln_forward_kernel, grid, dim3(256), 0, as_stream(stream), a, x, weight, bias, y, mean,
                     rstd);
  return launch_status();
}

extern "C" int gs_layernorm_backward(const gs_layernorm_desc* d, const float* x, const float* dy,
                                     const float* weight, const float* mean, const float* rstd, float* dx,
                                     float* dweight, float* dbias, int accumulate, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  const int rc = ln_check(d);
  if (rc != GS_OK) return rc;
  if (!x || !dy || !weight || !mean || !rstd || !dx || !dweight || !dbias || !workspace) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(weight) || !aligned16(dx) || !aligned16(dweight) ||
      !aligned16(dbias) || !aligned16(workspace))
    return GS_E_ALIGN;
  if (workspace_bytes < col_bytes(d->rows, d->C, 2)) return GS_E_WORKSPACE;
  ColArgs c;
  c.rows = d->rows; c.C4 = d->C / 4; c.C = d->C; c.planes = 2;
  c.runs = (int32_t)ceil_div(d->rows, kRunRows);
  c.lda = d->ldx; c.ldb = d->ldy; c.ldc = 0;
  const unsigned groups = (unsigned)ceil_div(c.C4, kColQuads);
  float* part = static_cast<float*>(workspace);
  // the parameter gradients read x and dy before dx (which may be dy's buffer) is written
  hipLaunchKernelGGL(ln_param_partial_kernel, dim3((unsigned)c.runs, groups), dim3(256), 0, as_stream(stream),
                     c, x, dy, mean, rstd, part);
  hipLaunchKernelGGL(col_runs_sum_kernel, dim3(groups, 2), dim3(256), 0, as_stream(stream), c, part, dweight,
                     dbias);
  const LnArgs a = ln_args(d, accumulate);
  const dim3 grid(stream_grid(a.row_blocks * 256, 256));
  hipLaunchKernelGGL(ln_backward_dx_kernel, grid, dim3(256), 0, as_stream(stream), a, x, dy, weight, mean,
                     rstd, dx);
  return launch_status();
}

extern "C" int gs_gelu_forward(const float* x, float* y, int64_t rows, int32_t C, int32_t ldx, int32_t ldy,
                               void* stream) {
  const int32_t ld[2] = {ldx, ldy};
  const int rc = rows_check(rows, C, ld, 2);
  if (rc != GS_OK) return rc;
  if (!x || !y) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(y)) return GS_E_ALIGN;
  const int64_t items = rows * (C / 4);
  hipLaunchKernelGGL(gelu_forward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream), x,
                     y, items, C / 4, ldx, ldy);
  return launch_status();
}

extern "C" int gs_gelu_backward(const float* x, const float* dy, float* dx, int64_t rows, int32_t C,
                                int32_t ldx, int32_t lddy, int32_t lddx, void* stream) {
  const int32_t ld[3] = {ldx, lddy, lddx};
  const int rc = rows_check(rows, C, ld, 3);
  if (rc != GS_OK) return rc;
  if (!x || !dy || !dx) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(dy) || !aligned16(dx)) return GS_E_ALIGN;
  const int64_t items = rows * (C / 4);
  hipLaunchKernelGGL(gelu_backward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream), x,
                     dy, dx, items, C / 4, ldx, lddy, lddx);
  return launch_status();
}

extern "C" int gs_layer_scale_add_forward(const float* identity, const float* z, const float* gamma,
                                          float* out, int64_t rows, int32_t C, int32_t ldi, int32_t ldz,
                                          int32_t ldo, void* stream) {
  const int32_t ld[3] = {ldi, ldz, ldo};
  const int rc = rows_check(rows, C, ld, 3);
  if (rc != GS_OK) return rc;
  if (!identity || !z || !gamma || !out) return GS_E_NULL;
  if (!aligned16(identity) || !aligned16(z) || !aligned16(gamma) || !aligned16(out)) return GS_E_ALIGN;
  const int64_t items = rows * (C / 4);
  hipLaunchKernelGGL(ls_forward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream),
                     identity, z, gamma, out, items, C / 4, ldi, ldz, ldo);
  return launch_status();
}

extern "C" size_t gs_layer_scale_workspace_bytes(int64_t rows, int32_t C) {
  const int32_t ld[1] = {C};
  return rows_check(rows, C, ld, 1) == GS_OK ? col_bytes(rows, C, 1) : 0;
}

extern "C" int gs_layer_scale_backward(const float* dout, const float* z, const float* gamma, float* dz,
                                       float* dgamma, int64_t rows, int32_t C, int32_t lddo, int32_t ldz,
                                       int32_t lddz, void* workspace, size_t workspace_bytes, void* stream) {
  const int32_t ld[3] = {lddo, ldz, lddz};
  const int rc = rows_check(rows, C, ld, 3);
  if (rc != GS_OK) return rc;
  if (!dout || !z || !gamma || !dz || !dgamma || !workspace) return GS_E_NULL;
  if (!aligned16(dout) || !aligned16(z) || !aligned16(gamma) || !aligned16(dz) || !aligned16(dgamma) ||
      !aligned16(workspace))
    return GS_E_ALIGN;
  if (workspace_bytes < col_bytes(rows, C, 1)) return GS_E_WORKSPACE;
  ColArgs c;
  c.rows = rows; c.C4 = C / 4; c.C = C; c.planes = 1;
  c.runs = (int32_t)ceil_div(rows, kRunRows);
  c.lda = lddo; c.ldb = ldz; c.ldc = lddz;
  const unsigned groups = (unsigned)ceil_div(c.C4, kColQuads);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(ls_backward_partial_kernel, dim3((unsigned)c.runs, groups), dim3(256), 0,
                     as_stream(stream), c, dout, z, gamma, dz, part);
  hipLaunchKernelGGL(col_runs_sum_kernel, dim3(groups, 1), dim3(256), 0, as_stream(stream), c, part, dgamma,
                     dgamma);
  return launch_status();
}
