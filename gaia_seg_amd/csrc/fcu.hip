// ElasticConvformer's coupling units between the conv branch and the token stream (include/gaiaseg_hip.h),
// on fp32 "rows x C" views with a pitch per operand, float4 lanes, no float atomics.
//
//   fcu_down   : tokens out of conv features.  z [B*T][D] is the pooled, projected conv map; the token
//                stream x_t and the result are [B*(T+1)][D] with the cls row in front of every image:
//                  out[b,0]   = x_t[b,0] + x_t[b,0]
//                  out[b,1+t] = x_t[b,1+t] + gelu(LN(z[b,t]))
//                One kernel walks the OUTPUT rows: a group of G lanes (csrc/convnext_ops.hip) owns a row,
//                takes the LayerNorm statistics of its z row exactly as ln_forward_kernel does and stores
//                the sum; the lanes of a cls row join the group sums with nothing and store 2 x.  The
//                backward recomputes the GELU input from z, mean and rstd; dweight / dbias go through
//                the per-run partials of csrc/rowwise.h; one more kernel over the output rows writes dz
//                and dx_t (dout on token rows, 2 dout on cls rows).
//   fcu_up_add : out[b,y,x] = x[b,y,x] + r[b,y/s,x/s] (nearest upsample by s, added), and
//                dr[b,i,j] = the sum of the s x s block of dout, rows first, then columns: a fixed order.
//   fcu_tokens : x[b,0] = cls, x[b,1+t] = patches[b,t]: the token assembly without a position embedding.
#include "rowwise.h"

namespace gs {
namespace {

struct DownArgs {
  int64_t out_rows, row_blocks;   // B * (T + 1); ceil(out_rows / (256 / G))
  int32_t T, C4, G;
  int32_t ldz, ldxt, ldo, lddz, lddxt;
  float eps, inv_c;
  int32_t accumulate;
};

__global__ __launch_bounds__(256) void fcu_down_forward_kernel(const DownArgs a, const float* __restrict__ z,
                                                               const float* __restrict__ xt,
                                                               const float* __restrict__ weight,
                                                               const float* __restrict__ bias,
                                                               float* __restrict__ out,
                                                               float* __restrict__ mean,
                                                               float* __restrict__ rstd) {
  const int G = a.G, gl = threadIdx.x % G, per_block = 256 / G;
  for (int64_t rb = blockIdx.x; rb < a.row_blocks; rb += gridDim.x) {
    const int64_t orow = rb * per_block + threadIdx.x / G;
    const bool live = orow < a.out_rows;
    const int64_t b = live ? orow / (a.T + 1) : 0;
    const int n = live ? (int)(orow % (a.T + 1)) : 0;
    const bool tok = live && n > 0;
    const int64_t zrow = tok ? b * a.T + (n - 1) : 0;
    const int c4 = tok ? a.C4 : 0;                    // other lanes only join the sums
    const float* zr = z + zrow * a.ldz;
    const float z0 = zr[0];
    float s = 0.f;
    for (int q = gl; q < c4; q += G) s += hsum(ld4(zr + q * 4) - z0);
    const float m = group_sum(s, G) * a.inv_c;        // mean - z0
    float ss = 0.f;
    for (int q = gl; q < c4; q += G) {
      const f32x4 d = (ld4(zr + q * 4) - z0) - m;
      ss += hsum(d * d);
    }
    const float rs = 1.0f / sqrtf(group_sum(ss, G) * a.inv_c + a.eps);
    if (!live) continue;
    const float* xr = xt + orow * a.ldxt;
    float* yr = out + orow * a.ldo;
    if (tok) {
      for (int q = gl; q < c4; q += G) {
        const f32x4 d = (ld4(zr + q * 4) - z0) - m;
        st4(yr + q * 4, ld4(xr + q * 4) + gelu_fwd4(d * rs * ld4(weight + q * 4) + ld4(bias + q * 4)));
      }
      if (gl == 0) {
        mean[zrow] = z0 + m;
        rstd[zrow] = rs;
      }
    } else {
      for (int q = gl; q < a.C4; q += G) {
        const f32x4 v = ld4(xr + q * 4);
        st4(yr + q * 4, v + v);
      }
    }
  }
}

// stage 1 of dweight / dbias: grid (runs of z rows, quad groups).  With u = xhat * weight + bias and
// gy = dout * gelu'(u):  plane 0 = sum gy * xhat, plane 1 = sum gy.  lda = ldz, ldb = lddo.
__global__ __launch_bounds__(256) void fcu_down_param_partial_kernel(const ColArgs a, const int T,
                                                                     const float* __restrict__ z,
                                                                     const float* __restrict__ dout,
                                                                     const float* __restrict__ weight,
                                                                     const float* __restrict__ bias,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ rstd,
                                                                     float* __restrict__ part) {
  __shared__ f32x4 sh[2][kColLanes][kColQuads];
  const int ql = threadIdx.x % kColQuads, pl = threadIdx.x / kColQuads;
  const int cq = blockIdx.y * kColQuads + ql;
  const int64_t r0 = (int64_t)blockIdx.x * kRunRows;
  f32x4 aw = f32x4{0.f, 0.f, 0.f, 0.f}, ab = aw;
  if (cq < a.C4) {
    const f32x4 w = ld4(weight + cq * 4), bi = ld4(bias + cq * 4);
    for (int i = 0; i < kRunRows / kColLanes; ++i) {
      const int64_t row = r0 + i * kColLanes + pl;
      if (row >= a.rows) break;
      const int64_t orow = row + row / T + 1;          // b * (T + 1) + 1 + t
      const f32x4 xh = (ld4(z + row * a.lda + cq * 4) - mean[row]) * rstd[row];
      const f32x4 gy = ld4(dout + orow * a.ldb + cq * 4) * gelu_grad4(xh * w + bi);
      aw += gy * xh;
      ab += gy;
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

// token rows: dz = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)), g = dout * gelu'(u) * weight, and
// dx_t (= or +=) dout; cls rows: dx_t (= or +=) 2 dout.  dx_t may be dout's buffer (an element is read and
// written by the same thread, after its last read).
__global__ __launch_bounds__(256) void fcu_down_backward_kernel(const DownArgs a, const float* __restrict__ z,
                                                                const float* dout,
                                                                const float* __restrict__ weight,
                                                                const float* __restrict__ bias,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ rstd,
                                                                float* __restrict__ dz, float* dxt) {
  const int G = a.G, gl = threadIdx.x % G, per_block = 256 / G;
  for (int64_t rb = blockIdx.x; rb < a.row_blocks; rb += gridDim.x) {
    const int64_t orow = rb * per_block + threadIdx.x / G;
    const bool live = orow < a.out_rows;
    const int64_t b = live ? orow / (a.T + 1) : 0;
    const int n = live ? (int)(orow % (a.T + 1)) : 0;
    const bool tok = live && n > 0;
    const int64_t zrow = tok ? b * a.T + (n - 1) : 0;
    const int c4 = tok ? a.C4 : 0;
    const float* zr = z + zrow * a.ldz;
    const float* gr = dout + (live ? orow : 0) * a.ldo;
    const float mu = mean[zrow], rs = rstd[zrow];
    float s1 = 0.f, s2 = 0.f;
    for (int q = gl; q < c4; q += G) {
      const f32x4 w = ld4(weight + q * 4), xh = (ld4(zr + q * 4) - mu) * rs;
      const f32x4 g = ld4(gr + q * 4) * gelu_grad4(xh * w + ld4(bias + q * 4)) * w;
      s1 += hsum(g);
      s2 += hsum(g * xh);
    }
    const float m1 = group_sum(s1, G) * a.inv_c, m2 = group_sum(s2, G) * a.inv_c;
    if (!live) continue;
    float* dzr = dz + zrow * a.lddz;
    float* dxr = dxt + orow * a.lddxt;
    const float k = tok ? 1.0f : 2.0f;
    for (int q = gl; q < a.C4; q += G) {
      const f32x4 go = ld4(gr + q * 4);
      if (tok) {
        const f32x4 w = ld4(weight + q * 4), xh = (ld4(zr + q * 4) - mu) * rs;
        const f32x4 g = go * gelu_grad4(xh * w + ld4(bias + q * 4)) * w;
        st4(dzr + q * 4, ((g - m1) - xh * m2) * rs);
      }
      const f32x4 v = go * k;
      st4(dxr + q * 4, a.accumulate ? ld4(dxr + q * 4) + v : v);
    }
  }
}

struct UpArgs {
  int64_t items;
  int32_t H, W, C4, s;     // H, W: the fine map for the forward, the coarse one for the backward
  int32_t lda, ldb, ldc;
  int32_t accumulate;
};

// lda = ldx, ldb = ldr, ldc = ldo.  out may be x's buffer.
__global__ __launch_bounds__(256) void fcu_up_add_forward_kernel(const UpArgs a, const float* x,
                                                                 const float* __restrict__ r, float* out) {
  const int Wc = a.W / a.s, Hc = a.H / a.s;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < a.items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    const int64_t pix = it / a.C4;
    const int xx = (int)(pix % a.W);
    const int yy = (int)((pix / a.W) % a.H);
    const int64_t b = pix / ((int64_t)a.W * a.H);
    const int64_t src = (b * Hc + yy / a.s) * Wc + xx / a.s;
    st4(out + pix * a.ldc + cq * 4, ld4(x + pix * a.lda + cq * 4) + ld4(r + src * a.ldb + cq * 4));
  }
}

// lda = lddo, ldb = lddr; H, W the coarse sizes.  One thread owns a quad of one coarse cell.
__global__ __launch_bounds__(256) void fcu_up_add_backward_kernel(const UpArgs a, const float* __restrict__ dout,
                                                                  float* __restrict__ dr) {
  const int Wf = a.W * a.s;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < a.items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % a.C4);
    const int64_t cell = it / a.C4;
    const int j = (int)(cell % a.W);
    const int64_t bi = cell / a.W;                                  // b * Hc + i
    const float* g0 = dout + (bi * a.s * Wf + (int64_t)j * a.s) * a.lda + cq * 4;
    f32x4 sum = ld4(g0);
    for (int dy = 0; dy < a.s; ++dy)
      for (int dx = (dy == 0 ? 1 : 0); dx < a.s; ++dx) sum += ld4(g0 + ((int64_t)dy * Wf + dx) * a.lda);
    float* d = dr + cell * a.ldb + cq * 4;
    st4(d, a.accumulate ? ld4(d) + sum : sum);
  }
}

__global__ __launch_bounds__(256) void fcu_tokens_forward_kernel(const float* __restrict__ patches,
                                                                 const float* __restrict__ cls,
                                                                 float* __restrict__ x, const int64_t items,
                                                                 const int T, const int D4, const int ldp,
                                                                 const int ldx) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % D4);
    const int64_t tok = it / D4;
    const int n = (int)(tok % (T + 1));
    const int64_t b = tok / (T + 1);
    st4(x + tok * ldx + cq * 4, n == 0 ? ld4(cls + cq * 4) : ld4(patches + (b * T + n - 1) * ldp + cq * 4));
  }
}

// dpatch[b,t] = dx[b,1+t];  dcls = sum_b dx[b,0] in the order of b.  One thread owns a quad of one token index.
__global__ __launch_bounds__(256) void fcu_tokens_backward_kernel(const float* __restrict__ dx,
                                                                  float* __restrict__ dpatch,
                                                                  float* __restrict__ dcls, const int64_t items,
                                                                  const int B, const int T, const int D4,
                                                                  const int lddx, const int lddp) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % D4);
    const int n = (int)(it / D4);
    if (n == 0) {
      f32x4 s = ld4(dx + cq * 4);
      for (int b = 1; b < B; ++b) s += ld4(dx + (int64_t)b * (T + 1) * lddx + cq * 4);
      st4(dcls + cq * 4, s);
    } else {
      for (int b = 0; b < B; ++b)
        st4(dpatch + ((int64_t)b * T + n - 1) * lddp + cq * 4,
            ld4(dx + ((int64_t)b * (T + 1) + n) * lddx + cq * 4));
    }
  }
}

int down_check(const gs_fcu_down_desc* d) {
  if (!d) return GS_E_NULL;
  if (d->B <= 0 || d->T <= 0) return GS_E_BADARG;
  const int32_t ld[5] = {d->ldz, d->ldxt, d->ldo, d->lddz, d->lddxt};
  const int rc = rows_check((int64_t)d->B * (d->T + 1), d->D, ld, 5);
  if (rc != GS_OK) return rc;
  if (!(d->eps > 0.f)) return GS_E_BADARG;
  return GS_OK;
}

DownArgs down_args(const gs_fcu_down_desc* d, int accumulate) {
  DownArgs a;
  a.out_rows = (int64_t)d->B * (d->T + 1);
  a.T = d->T; a.C4 = d->D / 4; a.G = row_group(a.C4);
  a.row_blocks = ceil_div(a.out_rows, 256 / a.G);
  a.ldz = d->ldz; a.ldxt = d->ldxt; a.ldo = d->ldo; a.lddz = d->lddz; a.lddxt = d->lddxt;
  a.eps = d->eps; a.inv_c = 1.0f / (float)d->D;
  a.accumulate = accumulate ? 1 : 0;
  return a;
}

// B maps of H x W pixels (the fine size) and their s-fold coarse maps
int up_check(int32_t B, int32_t H, int32_t W, int32_t C, int32_t s, const int32_t* ld, int n_ld) {
  if (B <= 0 || H <= 0 || W <= 0 || s <= 0) return GS_E_BADARG;
  if (H % s || W % s) return GS_E_BADARG;
  return rows_check((int64_t)B * H * W, C, ld, n_ld);
}

int tokens_check(int32_t B, int32_t T, int32_t D, const int32_t* ld, int n_ld) {
  if (B <= 0 || T <= 0) return GS_E_BADARG;
  return rows_check((int64_t)B * (T + 1), D, ld, n_ld);
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_fcu_down_workspace_bytes(const gs_fcu_down_desc* d) {
  return down_check(d) == GS_OK ? col_bytes((int64_t)d->B * d->T, d->D, 2) : 0;
}

extern "C" int gs_fcu_down_forward(const gs_fcu_down_desc* d, const float* z, const float* x_t,
                                   const float* weight, const float* bias, float* out, float* mean, float* rstd,
                                   void* stream) {
  const int rc = down_check(d);
  if (rc != GS_OK) return rc;
  if (!z || !x_t || !weight || !bias || !out || !mean || !rstd) return GS_E_NULL;
  if (!aligned16(z) || !aligned16(x_t) || !aligned16(weight) || !aligned16(bias) || !aligned16(out))
    return GS_E_ALIGN;
  const DownArgs a = down_args(d, 0);
  hipLaunchKernelGGL(fcu_down_forward_kernel, dim3(stream_grid(a.row_blocks * 256, 256)), dim3(256), 0,
                     as_stream(stream), a, z, x_t, weight, bias, out, mean, rstd);
  return launch_status();
}

extern "C" int gs_fcu_down_backward(const gs_fcu_down_desc* d, const float* z, const float* dout,
                                    const float* weight, const float* bias, const float* mean,
                                    const float* rstd, float* dz, float* dx_t, float* dweight, float* dbias,
                                    int accumulate_dx_t, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = down_check(d);
  if (rc != GS_OK) return rc;
  if (!z || !dout || !weight || !bias || !mean || !rstd || !dz || !dx_t || !dweight || !dbias || !workspace)
    return GS_E_NULL;
  if (!aligned16(z) || !aligned16(dout) || !aligned16(weight) || !aligned16(bias) || !aligned16(dz) ||
      !aligned16(dx_t) || !aligned16(dweight) || !aligned16(dbias) || !aligned16(workspace))
    return GS_E_ALIGN;
  const int64_t zrows = (int64_t)d->B * d->T;
  if (workspace_bytes < col_bytes(zrows, d->D, 2)) return GS_E_WORKSPACE;
  ColArgs c;
  c.rows = zrows; c.C4 = d->D / 4; c.C = d->D; c.planes = 2;
  c.runs = (int32_t)ceil_div(zrows, kRunRows);
  c.lda = d->ldz; c.ldb = d->ldo; c.ldc = 0;
  const unsigned groups = (unsigned)ceil_div(c.C4, kColQuads);
  float* part = static_cast<float*>(workspace);
  // the parameter gradients read dout before dx_t (which may be dout's buffer) is written
  hipLaunchKernelGGL(fcu_down_param_partial_kernel, dim3((unsigned)c.runs, groups), dim3(256), 0,
                     as_stream(stream), c, d->T, z, dout, weight, bias, mean, rstd, part);
  hipLaunchKernelGGL(col_runs_sum_kernel, dim3(groups, 2), dim3(256), 0, as_stream(stream), c, part, dweight,
                     dbias);
  const DownArgs a = down_args(d, accumulate_dx_t);
  hipLaunchKernelGGL(fcu_down_backward_kernel, dim3(stream_grid(a.row_blocks * 256, 256)), dim3(256), 0,
                     as_stream(stream), a, z, dout, weight, bias, mean, rstd, dz, dx_t);
  return launch_status();
}

extern "C" int gs_fcu_up_add_forward(const float* x, const float* r, float* out, int32_t B, int32_t H,
                                     int32_t W, int32_t C, int32_t s, int32_t ldx, int32_t ldr, int32_t ldo,
                                     void* stream) {
  const int32_t ld[3] = {ldx, ldr, ldo};
  const int rc = up_check(B, H, W, C, s, ld, 3);
  if (rc != GS_OK) return rc;
  if (!x || !r || !out) return GS_E_NULL;
  if (!aligned16(x) || !aligned16(r) || !aligned16(out)) return GS_E_ALIGN;
  UpArgs a;
  a.items = (int64_t)B * H * W * (C / 4);
  a.H = H; a.W = W; a.C4 = C / 4; a.s = s; a.lda = ldx; a.ldb = ldr; a.ldc = ldo; a.accumulate = 0;
  hipLaunchKernelGGL(fcu_up_add_forward_kernel, dim3(stream_grid(a.items, 256)), dim3(256), 0,
                     as_stream(stream), a, x, r, out);
  return launch_status();
}

extern "C" int gs_fcu_up_add_backward(const float* dout, float* dr, int32_t B, int32_t H, int32_t W, int32_t C,
                                      int32_t s, int32_t lddo, int32_t lddr, int accumulate, void* stream) {
  const int32_t ld[2] = {lddo, lddr};
  const int rc = up_check(B, H, W, C, s, ld, 2);
  if (rc != GS_OK) return rc;
  if (!dout || !dr) return GS_E_NULL;
  if (!aligned16(dout) || !aligned16(dr)) return GS_E_ALIGN;
  UpArgs a;
  a.H = H / s; a.W = W / s; a.C4 = C / 4; a.s = s; a.lda = lddo; a.ldb = lddr; a.ldc = 0;
  a.items = (int64_t)B * a.H * a.W * a.C4;
  a.accumulate = accumulate ? 1 : 0;
  hipLaunchKernelGGL(fcu_up_add_backward_kernel, dim3(stream_grid(a.items, 256)), dim3(256), 0,
                     as_stream(stream), a, dout, dr);
  return launch_status();
}

extern "C" int gs_fcu_tokens_forward(const float* patches, int32_t ldp, const float* cls_token, float* x,
                                     int32_t ldx, int32_t B, int32_t T, int32_t D, void* stream) {
  const int32_t ld[2] = {ldp, ldx};
  const int rc = tokens_check(B, T, D, ld, 2);
  if (rc != GS_OK) return rc;
  if (!patches || !cls_token || !x) return GS_E_NULL;
  if (!aligned16(patches) || !aligned16(cls_token) || !aligned16(x)) return GS_E_ALIGN;
  const int64_t items = (int64_t)B * (T + 1) * (D / 4);
  hipLaunchKernelGGL(fcu_tokens_forward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream),
                     patches, cls_token, x, items, T, D / 4, ldp, ldx);
  return launch_status();
}

extern "C" int gs_fcu_tokens_backward(const float* dx, int32_t lddx, float* dpatches, int32_t lddp,
                                      float* dcls_token, int32_t B, int32_t T, int32_t D, void* stream) {
  const int32_t ld[2] = {lddx, lddp};
  const int rc = tokens_check(B, T, D, ld, 2);
  if (rc != GS_OK) return rc;
  if (!dx || !dpatches || !dcls_token) return GS_E_NULL;
  if (!aligned16(dx) || !aligned16(dpatches) || !aligned16(dcls_token)) return GS_E_ALIGN;
  const int64_t items = (int64_t)(T + 1) * (D / 4);
  hipLaunchKernelGGL(fcu_tokens_backward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream),
                     dx, dpatches, dcls_token, items, B, T, D / 4, lddx, lddp);
  return launch_status();
}
