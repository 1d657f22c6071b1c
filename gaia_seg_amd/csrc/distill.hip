// In-place distillation loss (sandwich-rule training) with on-the-fly bilinear upsampling — gfx950.
//
// Replaces, for the student members of a sandwich iteration, the chain of
//   resize(seg_logits), resize(teacher_logits)        (when `interpolation`)   dynamic_psp_head.py:206-216
//   softmax(teacher / T), softmax(student / T)                                 dynamic_psp_head.py:220-221
//   (-bmm(student_score.log(), teacher_score)).mean() / D * distillation_weight  :226,241
// i.e.  loss = scale * sum_{n,c,Y,X} -q[c] * log p[c],  p = softmax(s / T), q = softmax(t / T),
// with the host's scale = distillation_weight / (N * D).  log p is taken as s / T - lse(s / T), not
// as log(softmax): finite where the reference's softmax underflows to 0.
// As in loss.hip no [N, Cls, H, W] tensor is written: a full-resolution pixel interpolates its
// logits from the four neighbouring low-resolution pixels; per-pixel losses are summed in double in
// a fixed order (bit-reproducible, no float atomics).  Backward:
//   ds = scale / T * (p - q)   at the evaluation grid, then the adjoint of the resize;
// the tile form (one group of lanes per tile of full-resolution pixels between four low-resolution
// pixels, every term evaluated once, then a fixed-order gather of the four corner sums) or, without a
// workspace, the gather form of loss.hip's ce_bwd_kernel.
#include <algorithm>
#include "common.h"
#include "resize.h"

namespace gs {

struct KdArgs {
  gs_kd_desc d;
  float sh, sw;
};

// ATen's association order (loss.hip tap_value): ly0 * (lx0 * p00 + lx1 * p01) + ly1 * (lx0 * p10 + lx1 * p11)
__device__ __forceinline__ float kd_tap(const float* b, long o00, long o01, long o10, long o11,
                                        float lx0, float lx1, float ly0, float ly1, long coff) {
  return ly0 * (lx0 * b[o00 + coff] + lx1 * b[o01 + coff]) +
         ly1 * (lx0 * b[o10 + coff] + lx1 * b[o11 + coff]);
}

// Offsets and weights of one evaluation-grid pixel in both tensors.
struct KdPx {
  long s00, s01, s10, s11, t00, t01, t10, t11;
  float lx0, lx1, ly0, ly1;
};
template <bool INTERP>
__device__ __forceinline__ KdPx kd_px(const KdArgs& a, int n, int Y, int X) {
  const gs_kd_desc& d = a.d;
  KdPx p;
  int y0 = Y, y1 = Y, x0 = X, x1 = X;
  p.lx0 = 1.f; p.lx1 = 0.f; p.ly0 = 1.f; p.ly1 = 0.f;
  if (INTERP) {
    const Lerp ly = lerp_coord(Y, a.sh, d.h, d.align_corners);
    const Lerp lx = lerp_coord(X, a.sw, d.w, d.align_corners);
    y0 = ly.i0; y1 = ly.i1; x0 = lx.i0; x1 = lx.i1;
    p.lx0 = lx.l0; p.lx1 = lx.l1; p.ly0 = ly.l0; p.ly1 = ly.l1;
  }
  const long sb = (long)n * d.s_sn, tb = (long)n * d.t_sn;
  p.s00 = sb + y0 * d.s_sh + x0 * d.s_sw; p.s01 = sb + y0 * d.s_sh + x1 * d.s_sw;
  p.s10 = sb + y1 * d.s_sh + x0 * d.s_sw; p.s11 = sb + y1 * d.s_sh + x1 * d.s_sw;
  p.t00 = tb + y0 * d.t_sh + x0 * d.t_sw; p.t01 = tb + y0 * d.t_sh + x1 * d.t_sw;
  p.t10 = tb + y1 * d.t_sh + x0 * d.t_sw; p.t11 = tb + y1 * d.t_sh + x1 * d.t_sw;
  return p;
}
template <bool INTERP>
__device__ __forceinline__ float kd_val(const float* b, long o00, long o01, long o10, long o11,
                                        const KdPx& p, long coff) {
  if (!INTERP) return b[o00 + coff];
  return kd_tap(b, o00, o01, o10, o11, p.lx0, p.lx1, p.ly0, p.ly1, coff);
}

// One thread per evaluation-grid pixel (grid-stride): two class passes — the online log-sum-exp of
// s / T and t / T, then sum_c q_c * (lse_s - s_c / T) — and a fixed-order block sum into part[block].
template <bool INTERP>
__global__ __launch_bounds__(256) void kd_fwd_kernel(const KdArgs a, const float* __restrict__ s,
                                                     const float* __restrict__ t,
                                                     float* __restrict__ lse_s,
                                                     float* __restrict__ lse_t,
                                                     double* __restrict__ part) {
  const gs_kd_desc& d = a.d;
  const long total = (long)d.N * d.H * d.W;
  const float T = d.T;
  double acc = 0.0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int X = (int)(i % d.W);
    const long r = i / d.W;
    const int Y = (int)(r % d.H);
    const int n = (int)(r / d.H);
    const KdPx p = kd_px<INTERP>(a, n, Y, X);
    float ms = -__builtin_huge_valf(), ss = 0.f, mt = -__builtin_huge_valf(), st = 0.f;
    for (int c = 0; c < d.Cls; ++c) {
      const float zs = kd_val<INTERP>(s, p.s00, p.s01, p.s10, p.s11, p, (long)c * d.s_sc) / T;
      const float zt = kd_val<INTERP>(t, p.t00, p.t01, p.t10, p.t11, p, (long)c * d.t_sc) / T;
      if (zs > ms) { ss = ss * expf(ms - zs) + 1.f; ms = zs; } else { ss += expf(zs - ms); }
      if (zt > mt) { st = st * expf(mt - zt) + 1.f; mt = zt; } else { st += expf(zt - mt); }
    }
    const float ls = ms + logf(ss), lt = mt + logf(st);
    float l = 0.f;
    for (int c = 0; c < d.Cls; ++c) {
      const float zs = kd_val<INTERP>(s, p.s00, p.s01, p.s10, p.s11, p, (long)c * d.s_sc) / T;
      const float zt = kd_val<INTERP>(t, p.t00, p.t01, p.t10, p.t11, p, (long)c * d.t_sc) / T;
      l += expf(zt - lt) * (ls - zs);
    }
    if (lse_s) lse_s[i] = ls;
    if (lse_t) lse_t[i] = lt;
    acc += (double)l;
  }
  __shared__ double sh[4];
  acc = wave_sum_d(acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// one block: out[0] = float(scale * sum of the partials), fixed order
__global__ __launch_bounds__(256) void kd_final_kernel(const double* __restrict__ part, int nparts,
                                                       double scale, float* __restrict__ out) {
  __shared__ double sh[4];
  double l = 0.0;
  for (int p = threadIdx.x; p < nparts; p += 256) l += part[p];
  l = wave_sum_d(l);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = l;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)((sh[0] + sh[1] + sh[2] + sh[3]) * scale);
}

// ---- backward without interpolation: one element (pixel, column) per thread, pad columns zeroed ----
__global__ __launch_bounds__(256) void kd_bwd_point_kernel(const KdArgs a, const float* __restrict__ s,
                                                           const float* __restrict__ t,
                                                           const float* __restrict__ lse_s,
                                                           const float* __restrict__ lse_t,
                                                           float coef, float* __restrict__ ds,
                                                           int ld) {
  const gs_kd_desc& d = a.d;
  const long total = (long)d.N * d.h * d.w * ld;
  const float T = d.T;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % ld);
    const long px = i / ld;
    float v = 0.f;
    if (c < d.Cls) {
      const int x = (int)(px % d.w);
      const long r = px / d.w;
      const int y = (int)(r % d.h), n = (int)(r / d.h);
      const float zs = s[n * d.s_sn + y * d.s_sh + x * d.s_sw + c * d.s_sc] / T;
      const float zt = t[n * d.t_sn + y * d.t_sh + x * d.t_sw + c * d.t_sc] / T;
      v = coef * (expf(zs - lse_s[px]) - expf(zt - lse_t[px]));
    }
    ds[i] = v;
  }
}

// ---- backward with interpolation, tile form ----
// Tile (ty, tx), ty in 0..h, tx in 0..w: the full-resolution pixels whose first source row is ty - 1
// and first source column tx - 1 (loss.hip ce_bwd_rowtile_kernel: bounds from lerp_coord itself, so
// membership is exact for every scale and align_corners).  LANES lanes own one tile: 16 (one DPP
// row; ~16-pixel tiles of config 4's 193 -> 769), 64 (one wave; x8) or 256 (x16, x32).  Classes in
// passes of KD_KCH; each pass stages the tile's four corner logits of both tensors in LDS, every
// lane accumulates the four corner sums of its pixels, the group reduces them in a fixed order and
// writes part[tile][slot][class]; kd_bwd_gather_kernel adds the four corner sums of the four tiles
// around each low-resolution pixel.
constexpr int KD_KCH = 8;

__device__ __forceinline__ float kd_row16_sum(float v) {   // lane 15 of each 16-lane row: the row's sum
  auto shr = [](float x, auto ctrl) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x),
                                                                 decltype(ctrl)::value, 0xf, 0xf, true));
  };
  using std::integral_constant;
  v += shr(v, integral_constant<int, 0x111>{});   // row_shr:1
  v += shr(v, integral_constant<int, 0x112>{});   // row_shr:2
  v += shr(v, integral_constant<int, 0x114>{});   // row_shr:4
  v += shr(v, integral_constant<int, 0x118>{});   // row_shr:8
  return v;
}

__device__ __forceinline__ int kd_first_dst(int k, float scale, int in, int out, int align) {
  if (k <= 0) return 0;
  if (k > in - 1) return out;
  float est = align ? (scale > 0.f ? (float)k / scale : (float)out) : ((float)k + 0.5f) / scale - 0.5f;
  int y = (int)floorf(est) - 1;
  y = y < 0 ? 0 : (y > out ? out : y);
  while (y < out && lerp_coord(y, scale, in, align).i0 < k) ++y;
  while (y > 0 && lerp_coord(y - 1, scale, in, align).i0 >= k) --y;
  return y;
}

template <int LANES>
__global__ __launch_bounds__(256) void kd_bwd_tile_kernel(const KdArgs a, const float* __restrict__ s,
                                                          const float* __restrict__ t,
                                                          const float* __restrict__ lse_s,
                                                          const float* __restrict__ lse_t,
                                                          float coef, long ntiles,
                                                          float* __restrict__ part, int cp) {
  constexpr int TPB = 256 / LANES;
  __shared__ float4 cs[TPB][KD_KCH], ct[TPB][KD_KCH];
  __shared__ float red[4][4 * KD_KCH];
  const gs_kd_desc& d = a.d;
  const float T = d.T;
  const int al = d.align_corners;
  const int grp = threadIdx.x / LANES, lane = threadIdx.x % LANES;
  const long tile = (long)blockIdx.x * TPB + grp;
  const bool live = tile < ntiles;
  const int tw = d.w + 1, th = d.h + 1;
  const int tx = live ? (int)(tile % tw) : 0;
  const long r = live ? tile / tw : 0;
  const int ty = (int)(r % th);
  const int n = (int)(r / th);
  int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  if (live && ty > 0 && tx > 0) {
    y0 = kd_first_dst(ty - 1, a.sh, d.h, d.H, al);
    y1 = kd_first_dst(ty, a.sh, d.h, d.H, al);
    x0 = kd_first_dst(tx - 1, a.sw, d.w, d.W, al);
    x1 = kd_first_dst(tx, a.sw, d.w, d.W, al);
  }
  const int nx = x1 - x0, npx = (y1 - y0) * nx;
  const int r0 = max(ty - 1, 0), r1 = min(ty, d.h - 1), c0i = max(tx - 1, 0), c1i = min(tx, d.w - 1);
  const float* sb = s + (long)n * d.s_sn;
  const float* tb = t + (long)n * d.t_sn;
  const long so00 = r0 * d.s_sh + c0i * d.s_sw, so01 = r0 * d.s_sh + c1i * d.s_sw,
             so10 = r1 * d.s_sh + c0i * d.s_sw, so11 = r1 * d.s_sh + c1i * d.s_sw;
  const long to00 = r0 * d.t_sh + c0i * d.t_sw, to01 = r0 * d.t_sh + c1i * d.t_sw,
             to10 = r1 * d.t_sh + c0i * d.t_sw, to11 = r1 * d.t_sh + c1i * d.t_sw;
  float* prow = part + (live ? tile : 0) * 4 * cp;
  for (int c0 = 0; c0 < d.Cls; c0 += KD_KCH) {
    const int nc = min(KD_KCH, d.Cls - c0);
    __syncthreads();   // the previous pass has finished reading the staged corners
    for (int c = lane; c < KD_KCH; c += LANES) {   // classes past nc repeat the last one; not written
      const long cc = c0 + min(c, nc - 1);
      const long os = cc * d.s_sc, ot = cc * d.t_sc;
      cs[grp][c] = npx > 0 ? make_float4(sb[so00 + os], sb[so01 + os], sb[so10 + os], sb[so11 + os])
                           : make_float4(0.f, 0.f, 0.f, 0.f);
      ct[grp][c] = npx > 0 ? make_float4(tb[to00 + ot], tb[to01 + ot], tb[to10 + ot], tb[to11 + ot])
                           : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    float a00[KD_KCH], a01[KD_KCH], a10[KD_KCH], a11[KD_KCH];
#pragma unroll
    for (int c = 0; c < KD_KCH; ++c) { a00[c] = 0.f; a01[c] = 0.f; a10[c] = 0.f; a11[c] = 0.f; }
    for (int q = lane; q < npx; q += LANES) {
      const int Y = y0 + q / nx, X = x0 + q % nx;
      const long pi = ((long)n * d.H + Y) * d.W + X;
      const Lerp ly = lerp_coord(Y, a.sh, d.h, al);
      const Lerp lx = lerp_coord(X, a.sw, d.w, al);
      // slot 1 = low-resolution index ty (tx), slot 0 = the one before it (both weights at the far
      // border, where i1 == i0 == ty - 1)
      const float wy1 = (ly.i0 == ty ? ly.l0 : 0.f) + (ly.i1 == ty ? ly.l1 : 0.f);
      const float wy0 = (ly.i0 != ty ? ly.l0 : 0.f) + (ly.i1 != ty ? ly.l1 : 0.f);
      const float wx1 = (lx.i0 == tx ? lx.l0 : 0.f) + (lx.i1 == tx ? lx.l1 : 0.f);
      const float wx0 = (lx.i0 != tx ? lx.l0 : 0.f) + (lx.i1 != tx ? lx.l1 : 0.f);
      const float w00 = wy0 * wx0 * coef, w01 = wy0 * wx1 * coef, w10 = wy1 * wx0 * coef,
                  w11 = wy1 * wx1 * coef;
      const float ls = lse_s[pi], lt = lse_t[pi];
#pragma unroll
      for (int c = 0; c < KD_KCH; ++c) {
        const float4 S = cs[grp][c], U = ct[grp][c];
        // the forward's association order, so that exp(z - lse) sums to one as there
        const float zs = (ly.l0 * (lx.l0 * S.x + lx.l1 * S.y) + ly.l1 * (lx.l0 * S.z + lx.l1 * S.w)) / T;
        const float zt = (ly.l0 * (lx.l0 * U.x + lx.l1 * U.y) + ly.l1 * (lx.l0 * U.z + lx.l1 * U.w)) / T;
        const float g = expf(zs - ls) - expf(zt - lt);
        a00[c] += w00 * g; a01[c] += w01 * g; a10[c] += w10 * g; a11[c] += w11 * g;
      }
    }
    if (LANES == 16) {
#pragma unroll
      for (int c = 0; c < KD_KCH; ++c) {
        const float v0 = kd_row16_sum(a00[c]), v1 = kd_row16_sum(a01[c]), v2 = kd_row16_sum(a10[c]),
                    v3 = kd_row16_sum(a11[c]);
        if (live && lane == 15 && c < nc) {
          prow[0 * cp + c0 + c] = v0; prow[1 * cp + c0 + c] = v1;
          prow[2 * cp + c0 + c] = v2; prow[3 * cp + c0 + c] = v3;
        }
      }
    } else if (LANES == 64) {
#pragma unroll
      for (int c = 0; c < KD_KCH; ++c) {
        const float v0 = wave_sum(a00[c]), v1 = wave_sum(a01[c]), v2 = wave_sum(a10[c]),
                    v3 = wave_sum(a11[c]);
        if (live && lane == 0 && c < nc) {
          prow[0 * cp + c0 + c] = v0; prow[1 * cp + c0 + c] = v1;
          prow[2 * cp + c0 + c] = v2; prow[3 * cp + c0 + c] = v3;
        }
      }
    } else {
      const int wl = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
      for (int c = 0; c < KD_KCH; ++c) {
        const float v0 = wave_sum(a00[c]), v1 = wave_sum(a01[c]), v2 = wave_sum(a10[c]),
                    v3 = wave_sum(a11[c]);
        if (wl == 0) {
          red[wave][c] = v0; red[wave][KD_KCH + c] = v1; red[wave][2 * KD_KCH + c] = v2;
          red[wave][3 * KD_KCH + c] = v3;
        }
      }
      __syncthreads();
      if (threadIdx.x < 4 * KD_KCH) {
        const int slot = threadIdx.x / KD_KCH, c = threadIdx.x % KD_KCH;
        if (live && c < nc)
          prow[slot * cp + c0 + c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) +
                                     red[3][threadIdx.x];
      }
    }
  }
}

// ds[n, y, x, c] = corner sums of the four tiles around low-resolution pixel (y, x); pad columns 0
__global__ __launch_bounds__(256) void kd_bwd_gather_kernel(const float* __restrict__ part, int N,
                                                            int h, int w, int Cls, int cp,
                                                            float* __restrict__ ds, int ld) {
  const long total = (long)N * h * w * ld;
  const int tw = w + 1, th = h + 1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % ld);
    const long px = i / ld;
    float v = 0.f;
    if (c < Cls) {
      const int x = (int)(px % w);
      const long r = px / w;
      const int y = (int)(r % h), n = (int)(r / h);
      const long t11 = ((long)n * th + y) * tw + x;   // tile (y, x): this pixel is its slot (1, 1)
      v = part[((t11 + tw + 1) * 4 + 0) * cp + c];    // tile (y+1, x+1), slot (0, 0)
      v += part[((t11 + tw) * 4 + 1) * cp + c];       // tile (y+1, x  ), slot (0, 1)
      v += part[((t11 + 1) * 4 + 2) * cp + c];        // tile (y,   x+1), slot (1, 0)
      v += part[(t11 * 4 + 3) * cp + c];              // tile (y,   x  ), slot (1, 1)
    }
    ds[i] = v;
  }
}

// ---- backward with interpolation, gather form (no workspace): one workgroup per low-resolution
// pixel walks its bilinear footprint (loss.hip ce_bwd_kernel); every term is evaluated four times ----
constexpr int KD_GCH = 16;
__global__ __launch_bounds__(256) void kd_bwd_gather_form_kernel(const KdArgs a, const float* __restrict__ s,
                                                                 const float* __restrict__ t,
                                                                 const float* __restrict__ lse_s,
                                                                 const float* __restrict__ lse_t,
                                                                 float coef, float* __restrict__ ds,
                                                                 int ld) {
  __shared__ float sh[4][KD_GCH];
  const gs_kd_desc& d = a.d;
  const float T = d.T;
  const int al = d.align_corners;
  const int x = blockIdx.x % d.w;
  const int r = blockIdx.x / d.w;
  const int y = r % d.h;
  const int n = r / d.h;
  int ylo, yhi, xlo, xhi;
  dst_range(y, a.sh, d.H, ylo, yhi);
  dst_range(x, a.sw, d.W, xlo, xhi);
  const int nx = xhi - xlo + 1, npx = (yhi - ylo + 1) * nx;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nthr = blockDim.x, nwave = nthr >> 6;
  float* orow = ds + ((long)(n * d.h + y) * d.w + x) * ld;
  for (int c0 = 0; c0 < d.Cls; c0 += KD_GCH) {
    const int nc = min(KD_GCH, d.Cls - c0);
    float acc[KD_GCH];
#pragma unroll
    for (int c = 0; c < KD_GCH; ++c) acc[c] = 0.f;
    for (int q = threadIdx.x; q < npx; q += nthr) {
      const int Y = ylo + q / nx, X = xlo + q % nx;
      const Lerp ly = lerp_coord(Y, a.sh, d.h, al);
      const Lerp lx = lerp_coord(X, a.sw, d.w, al);
      const float wgt = adj_weight(ly, y) * adj_weight(lx, x);
      if (wgt == 0.f) continue;
      const long pi = ((long)n * d.H + Y) * d.W + X;
      const KdPx p = kd_px<true>(a, n, Y, X);
      const float ls = lse_s[pi], lt = lse_t[pi], w = wgt * coef;
#pragma unroll
      for (int c = 0; c < KD_GCH; ++c) {
        if (c < nc) {
          const float zs = kd_val<true>(s, p.s00, p.s01, p.s10, p.s11, p, (long)(c0 + c) * d.s_sc) / T;
          const float zt = kd_val<true>(t, p.t00, p.t01, p.t10, p.t11, p, (long)(c0 + c) * d.t_sc) / T;
          acc[c] += w * (expf(zs - ls) - expf(zt - lt));
        }
      }
    }
#pragma unroll
    for (int c = 0; c < KD_GCH; ++c) {
      if (c < nc) {
        const float v = wave_sum(acc[c]);
        if (lane == 0) sh[wave][c] = v;
      }
    }
    __syncthreads();
    if (threadIdx.x < nc) {
      float v = sh[0][threadIdx.x];
      for (int wv = 1; wv < nwave; ++wv) v += sh[wv][threadIdx.x];
      orow[c0 + threadIdx.x] = v;
    }
    __syncthreads();
  }
  for (int c = d.Cls + threadIdx.x; c < ld; c += nthr) orow[c] = 0.f;
}

// ---- gradient accumulation over arena ranges: dst += src; src = 0 ----
__global__ __launch_bounds__(256) void accumulate_clear_kernel(float* __restrict__ dst,
                                                               float* __restrict__ src, long n,
                                                               int vec) {
  const long stride = (long)gridDim.x * blockDim.x;
  const long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long done = 0;
  if (vec) {
    const long n4 = n >> 2;
    float4* d4 = reinterpret_cast<float4*>(dst);
    float4* s4 = reinterpret_cast<float4*>(src);
    for (long i = i0; i < n4; i += stride) {
      float4 a = d4[i];
      const float4 b = s4[i];
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      d4[i] = a;
      s4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    done = n4 << 2;
  }
  for (long i = done + i0; i < n; i += stride) {
    dst[i] += src[i];
    src[i] = 0.f;
  }
}

static int check_kd(const gs_kd_desc* d, KdArgs& a) {
  if (!d) return GS_E_NULL;
  if (d->N <= 0 || d->h <= 0 || d->w <= 0 || d->Cls <= 0 || d->H <= 0 || d->W <= 0)
    return GS_E_BADARG;
  if (!(d->T > 0.f) || d->T == __builtin_huge_valf()) return GS_E_BADARG;
  if (d->interpolation != 0 && d->interpolation != 1) return GS_E_BADARG;
  if (!d->interpolation && (d->H != d->h || d->W != d->w)) return GS_E_BADARG;
  a.d = *d;
  a.sh = resize_scale(d->h, d->H, d->align_corners);
  a.sw = resize_scale(d->w, d->W, d->align_corners);
  return GS_OK;
}
static int kd_grid(const gs_kd_desc* d) { return stream_grid((long)d->N * d->H * d->W, 256); }

// lanes per tile from the mean tile size (full-resolution pixels per low-resolution pixel)
static int kd_tile_lanes(const gs_kd_desc* d) {
  const double px = (double)d->H * d->W / ((double)d->h * d->w);
  return px <= 24.0 ? 16 : px <= 96.0 ? 64 : 256;
}

}  // namespace gs

using namespace gs;

extern "C" size_t gs_kd_workspace_bytes(const gs_kd_desc* d) {
  KdArgs a;
  if (check_kd(d, a)) return 0;
  return (size_t)kd_grid(d) * sizeof(double);
}

extern "C" int gs_kd_forward(const gs_kd_desc* d, const float* student, const float* teacher,
                             float* lse_s, float* lse_t, float scale, float* out, void* workspace,
                             size_t workspace_bytes, void* stream) {
  KdArgs a;
  int rc = check_kd(d, a);
  if (rc) return rc;
  if (!student || !teacher || !out || !workspace) return GS_E_NULL;
  const int grid = kd_grid(d);
  if ((size_t)grid * sizeof(double) > workspace_bytes) return GS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return GS_E_ALIGN;
  hipStream_t st = as_stream(stream);
  double* part = static_cast<double*>(workspace);
  if (d->interpolation)
    hipLaunchKernelGGL(kd_fwd_kernel<true>, dim3(grid), dim3(256), 0, st, a, student, teacher, lse_s,
                       lse_t, part);
  else
    hipLaunchKernelGGL(kd_fwd_kernel<false>, dim3(grid), dim3(256), 0, st, a, student, teacher, lse_s,
                       lse_t, part);
  hipLaunchKernelGGL(kd_final_kernel, dim3(1), dim3(256), 0, st, part, grid, (double)scale, out);
  return launch_status();
}

extern "C" size_t gs_kd_backward_workspace_bytes(const gs_kd_desc* d, int32_t ld_d) {
  KdArgs a;
  if (check_kd(d, a) || !d->interpolation || ld_d < d->Cls) return 0;
  return (size_t)d->N * (d->h + 1) * (d->w + 1) * 4 * ld_d * sizeof(float);
}

extern "C" int gs_kd_backward(const gs_kd_desc* d, const float* student, const float* teacher,
                              const float* lse_s, const float* lse_t, float grad_scale, float* ds,
                              int32_t ld_d, void* workspace, size_t workspace_bytes, void* stream) {
  KdArgs a;
  int rc = check_kd(d, a);
  if (rc) return rc;
  if (!student || !teacher || !lse_s || !lse_t || !ds) return GS_E_NULL;
  if (ld_d < d->Cls) return GS_E_BADARG;
  hipStream_t st = as_stream(stream);
  const float coef = grad_scale / d->T;
  if (!d->interpolation) {
    const long total = (long)d->N * d->h * d->w * ld_d;
    hipLaunchKernelGGL(kd_bwd_point_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, st, a,
                       student, teacher, lse_s, lse_t, coef, ds, ld_d);
    return launch_status();
  }
  const size_t need = gs_kd_backward_workspace_bytes(d, ld_d);
  if (!workspace || workspace_bytes < need) {
    const long sup = (2L * d->H / d->h + 1) * (2L * d->W / d->w + 1);
    const int threads = sup > 128 ? 256 : sup > 64 ? 128 : 64;
    hipLaunchKernelGGL(kd_bwd_gather_form_kernel, dim3(d->N * d->h * d->w), dim3(threads), 0, st, a,
                       student, teacher, lse_s, lse_t, coef, ds, ld_d);
    return launch_status();
  }
  float* part = static_cast<float*>(workspace);
  const long ntiles = (long)d->N * (d->h + 1) * (d->w + 1);
  const int lanes = kd_tile_lanes(d);
  const dim3 grid((unsigned)ceil_div(ntiles, 256 / lanes));
  if (lanes == 16)
    hipLaunchKernelGGL(kd_bwd_tile_kernel<16>, grid, dim3(256), 0, st, a, student, teacher, lse_s,
                       lse_t, coef, ntiles, part, ld_d);
  else if (lanes == 64)
    hipLaunchKernelGGL(kd_bwd_tile_kernel<64>, grid, dim3(256), 0, st, a, student, teacher, lse_s,
                       lse_t, coef, ntiles, part, ld_d);
  else
    hipLaunchKernelGGL(kd_bwd_tile_kernel<256>, grid, dim3(256), 0, st, a, student, teacher, lse_s,
                       lse_t, coef, ntiles, part, ld_d);
  const long total = (long)d->N * d->h * d->w * ld_d;
  hipLaunchKernelGGL(kd_bwd_gather_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, st, part,
                     d->N, d->h, d->w, d->Cls, ld_d, ds, ld_d);
  return launch_status();
}

extern "C" int gs_grad_accumulate(float* dst, float* src, int64_t n, void* stream) {
  if (!dst || !src) return GS_E_NULL;
  if (n < 0 || dst == src) return GS_E_BADARG;
  if (n == 0) return GS_OK;
  const bool vec = aligned16(dst) && aligned16(src);
  const long work = vec ? (n >> 2) + (n & 3) : n;
  hipLaunchKernelGGL(accumulate_clear_kernel, dim3(stream_grid(work, 256)), dim3(256), 0,
                     as_stream(stream), dst, src, (long)n, vec ? 1 : 0);
  return launch_status();
}
