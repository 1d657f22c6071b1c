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

// d.h, d.w are the student's logit size.  The teacher's (ht, wt) equals it for gs_kd_* (tsame) and is
// free for gs_distill_* (the fixed teacher of DynamicDistiller may have another output stride).
struct KdArgs {
  gs_kd_desc d;
  float sh, sw;
  int ht, wt;
  float sht, swt;
  int tsame;
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
  float lx0, lx1, ly0, ly1;       // the student's weights
  float tx0, tx1, ty0, ty1;       // the teacher's (the same numbers when a.tsame)
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
  p.tx0 = p.lx0; p.tx1 = p.lx1; p.ty0 = p.ly0; p.ty1 = p.ly1;
  if (INTERP && !a.tsame) {
    const Lerp ly = lerp_coord(Y, a.sht, a.ht, d.align_corners);
    const Lerp lx = lerp_coord(X, a.swt, a.wt, d.align_corners);
    y0 = ly.i0; y1 = ly.i1; x0 = lx.i0; x1 = lx.i1;
    p.tx0 = lx.l0; p.tx1 = lx.l1; p.ty0 = ly.l0; p.ty1 = ly.l1;
  }
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
template <bool INTERP>
__device__ __forceinline__ float kd_tval(const float* b, const KdPx& p, long coff) {
  if (!INTERP) return b[p.t00 + coff];
  return kd_tap(b, p.t00, p.t01, p.t10, p.t11, p.tx0, p.tx1, p.ty0, p.ty1, coff);
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
      const float zt = kd_tval<INTERP>(t, p, (long)c * d.t_sc) / T;
      if (zs > ms) { ss = ss * expf(ms - zs) + 1.f; ms = zs; } else { ss += expf(zs - ms); }
      if (zt > mt) { st = st * expf(mt - zt) + 1.f; mt = zt; } else { st += expf(zt - mt); }
    }
    const float ls = ms + logf(ss), lt = mt + logf(st);
    float l = 0.f;
    for (int c = 0; c < d.Cls; ++c) {
      const float zs = kd_val<INTERP>(s, p.s00, p.s01, p.s10, p.s11, p, (long)c * d.s_sc) / T;
      const float zt = kd_tval<INTERP>(t, p, (long)c * d.t_sc) / T;
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

// TSAME: the teacher shares the student's grid and its four corners are staged with the student's;
// otherwise (gs_distill_*) every pixel gathers the teacher's logits through the teacher's own taps.
template <int LANES, bool TSAME>
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
      ct[grp][c] = npx > 0 && TSAME
                       ? make_float4(tb[to00 + ot], tb[to01 + ot], tb[to10 + ot], tb[to11 + ot])
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
      KdPx tp;
      if (!TSAME) tp = kd_px<true>(a, n, Y, X);
#pragma unroll
      for (int c = 0; c < KD_KCH; ++c) {
        const float4 S = cs[grp][c], U = ct[grp][c];
        // the forward's association order, so that exp(z - lse) sums to one as there
        const float zs = (ly.l0 * (lx.l0 * S.x + lx.l1 * S.y) + ly.l1 * (lx.l0 * S.z + lx.l1 * S.w)) / T;
        float zt;
        if (TSAME)
          zt = (ly.l0 * (lx.l0 * U.x + lx.l1 * U.y) + ly.l1 * (lx.l0 * U.z + lx.l1 * U.w)) / T;
        else   // (classes past nc repeat the last one, as the staged corners do; not written)
          zt = kd_tval<true>(t, tp, (long)(c0 + min(c, nc - 1)) * d.t_sc) / T;
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
          const float zt = kd_tval<true>(t, p, (long)(c0 + c) * d.t_sc) / T;
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
  a.ht = d->h; a.wt = d->w; a.sht = a.sh; a.swt = a.sw; a.tsame = 1;
  return GS_OK;
}
// gs_distill_desc -> the gs_kd_desc of the student (interpolation on) + the teacher's grid
static int check_distill(const gs_distill_desc* q, gs_kd_desc& d, KdArgs& a) {
  if (!q) return GS_E_NULL;
  if (q->ht <= 0 || q->wt <= 0) return GS_E_BADARG;
  d.N = q->N; d.h = q->hs; d.w = q->ws; d.Cls = q->Cls; d.H = q->H; d.W = q->W;
  d.s_sn = q->s_sn; d.s_sh = q->s_sh; d.s_sw = q->s_sw; d.s_sc = q->s_sc;
  d.t_sn = q->t_sn; d.t_sh = q->t_sh; d.t_sw = q->t_sw; d.t_sc = q->t_sc;
  d.T = q->T; d.align_corners = q->align_corners; d.interpolation = 1; d.reserved = 0;
  const int rc = check_kd(&d, a);
  if (rc) return rc;
  a.ht = q->ht; a.wt = q->wt;
  a.sht = resize_scale(q->ht, q->H, q->align_corners);
  a.swt = resize_scale(q->wt, q->W, q->align_corners);
  a.tsame = (q->ht == q->hs && q->wt == q->ws) ? 1 : 0;
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

static int kd_forward_launch(const gs_kd_desc* d, const KdArgs& a, const float* student,
                             const float* teacher, float* lse_s, float* lse_t, float scale,
                             float* out, void* workspace, size_t workspace_bytes, void* stream) {
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

extern "C" int gs_kd_forward(const gs_kd_desc* d, const float* student, const float* teacher,
                             float* lse_s, float* lse_t, float scale, float* out, void* workspace,
                             size_t workspace_bytes, void* stream) {
  KdArgs a;
  int rc = check_kd(d, a);
  if (rc) return rc;
  return kd_forward_launch(d, a, student, teacher, lse_s, lse_t, scale, out, workspace,
                           workspace_bytes, stream);
}

extern "C" size_t gs_kd_backward_workspace_bytes(const gs_kd_desc* d, int32_t ld_d) {
  KdArgs a;
  if (check_kd(d, a) || !d->interpolation || ld_d < d->Cls) return 0;
  return (size_t)d->N * (d->h + 1) * (d->w + 1) * 4 * ld_d * sizeof(float);
}

template <int LANES>
static void kd_tile_launch(const KdArgs& a, dim3 grid, hipStream_t st, const float* student,
                           const float* teacher, const float* lse_s, const float* lse_t, float coef,
                           long ntiles, float* part, int cp) {
  if (a.tsame)
    hipLaunchKernelGGL((kd_bwd_tile_kernel<LANES, true>), grid, dim3(256), 0, st, a, student, teacher,
                       lse_s, lse_t, coef, ntiles, part, cp);
  else
    hipLaunchKernelGGL((kd_bwd_tile_kernel<LANES, false>), grid, dim3(256), 0, st, a, student, teacher,
                       lse_s, lse_t, coef, ntiles, part, cp);
}

static int kd_backward_launch(const gs_kd_desc* d, const KdArgs& a, const float* student,
                              const float* teacher, const float* lse_s, const float* lse_t,
                              float grad_scale, float* ds, int32_t ld_d, void* workspace,
                              size_t workspace_bytes, void* stream) {
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
    kd_tile_launch<16>(a, grid, st, student, teacher, lse_s, lse_t, coef, ntiles, part, ld_d);
  else if (lanes == 64)
    kd_tile_launch<64>(a, grid, st, student, teacher, lse_s, lse_t, coef, ntiles, part, ld_d);
  else
    kd_tile_launch<256>(a, grid, st, student, teacher, lse_s, lse_t, coef, ntiles, part, ld_d);
  const long total = (long)d->N * d->h * d->w * ld_d;
  hipLaunchKernelGGL(kd_bwd_gather_kernel, dim3(stream_grid(total, 256)), dim3(256), 0, st, part,
                     d->N, d->h, d->w, d->Cls, ld_d, ds, ld_d);
  return launch_status();
}

extern "C" int gs_kd_backward(const gs_kd_desc* d, const float* student, const float* teacher,
                              const float* lse_s, const float* lse_t, float grad_scale, float* ds,
                              int32_t ld_d, void* workspace, size_t workspace_bytes, void* stream) {
  KdArgs a;
  int rc = check_kd(d, a);
  if (rc) return rc;
  return kd_backward_launch(d, a, student, teacher, lse_s, lse_t, grad_scale, ds, ld_d, workspace,
                            workspace_bytes, stream);
}

// ---- fixed-teacher distillation: the same launches with the teacher on a grid of its own ----
extern "C" size_t gs_distill_workspace_bytes(const gs_distill_desc* q) {
  gs_kd_desc d;
  KdArgs a;
  if (check_distill(q, d, a)) return 0;
  return gs_kd_workspace_bytes(&d);
}

extern "C" int gs_distill_forward(const gs_distill_desc* q, const float* student,
                                  const float* teacher, float* lse_s, float* lse_t, float scale,
                                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
  gs_kd_desc d;
  KdArgs a;
  int rc = check_distill(q, d, a);
  if (rc) return rc;
  return kd_forward_launch(&d, a, student, teacher, lse_s, lse_t, scale, out, workspace,
                           workspace_bytes, stream);
}

extern "C" size_t gs_distill_backward_workspace_bytes(const gs_distill_desc* q, int32_t ld_d) {
  gs_kd_desc d;
  KdArgs a;
  if (check_distill(q, d, a)) return 0;
  return gs_kd_backward_workspace_bytes(&d, ld_d);
}

extern "C" int gs_distill_backward(const gs_distill_desc* q, const float* student,
                                   const float* teacher, const float* lse_s, const float* lse_t,
                                   float grad_scale, float* ds, int32_t ld_d, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  gs_kd_desc d;
  KdArgs a;
  int rc = check_distill(q, d, a);
  if (rc) return rc;
  return kd_backward_launch(&d, a, student, teacher, lse_s, lse_t, grad_scale, ds, ld_d, workspace,
                            workspace_bytes, stream);
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

// ------------------------------------------------------------------------------------------------
// Pairwise affinity loss of the fixed-teacher distiller (dynamic_distiller.py:309-339).
//   x_i: the channel vector of window pixel i;  d_i = max(|x_i|, eps);  G_ij = x_i . x_j / (d_i d_j)
//   A_ij = softmax over i of Gt_ij / T,  L_ij = log softmax over j of Gs_ij / T,  loss = -sum A_ij L_ij
// Backward, with p_ij = exp(L_ij), r_i = sum_j A_ij and coef = grad_scale / T:
//   D_ij = dloss / dGs_ij = coef * (r_i p_ij - A_ij),   E_kj = D_kj + D_jk,
//   g_k  = dloss / d(x_k / d_k) = sum_j E_kj x_j / d_j,
//   dx_k = (g_k - m_k (x_k / d_k) sum_j E_kj Gs_kj) / d_k,   m_k = 1 where |x_k| >= eps, else 0
// (below eps the clamp holds the denominator constant: autograd's g_k / eps), i.e. dx = Wc X with the
// P x P coefficients Wc_kj = E_kj / (d_k d_j) - [j == k] m_k sum_j' E_kj' Gs_kj' / d_k^2.
// save (floats, per image n): Gs[P*P] | Gt[P*P] | Wc[P*P] | d_s[P] | m_s[P] | lse_s[P] | lse_t[P] | r[P],
// behind N doubles of per-image loss partials.
// ------------------------------------------------------------------------------------------------
namespace gs {

constexpr int PW_TILE = 16;    // Gram tile: 16 x 16 outputs per workgroup
constexpr int PW_CCH = 64;     // channels per staged chunk
constexpr int PW_LDS = PW_CCH + 4;   // padded row: consecutive rows start 4 banks apart
constexpr float PW_EPS = 1e-12f;

struct PwMap {
  const float* base;
  long sn, sc, sh, sw;
  int C, vec;
};
struct PwArgs {
  gs_pairwise_desc d;
  int P, nx;
};
__host__ __device__ __forceinline__ long pw_per_image(int P) { return 3L * P * P + 5L * P; }

// channels [c0, c0 + PW_CCH) of window pixel p of image n into dst (zeros past C)
__device__ __forceinline__ void pw_stage_row(const PwMap& m, const PwArgs& a, int n, int p, int c0,
                                             float* dst, int lane, int lanes) {
  const int y = a.d.y0 + p / a.nx, x = a.d.x0 + p % a.nx;
  const float* row = m.base + (long)n * m.sn + (long)y * m.sh + (long)x * m.sw;
  if (m.vec) {
    for (int q = lane; q < PW_CCH / 4; q += lanes) {
      const int c = c0 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c + 3 < m.C) {
        v = *reinterpret_cast<const float4*>(row + c);
      } else {   // the scalar tail
        if (c < m.C) v.x = row[c];
        if (c + 1 < m.C) v.y = row[c + 1];
        if (c + 2 < m.C) v.z = row[c + 2];
      }
      *reinterpret_cast<float4*>(dst + 4 * q) = v;
    }
  } else {
    for (int q = lane; q < PW_CCH; q += lanes) {
      const int c = c0 + q;
      dst[q] = c < m.C ? row[(long)c * m.sc] : 0.f;
    }
  }
}

// grid (tiles_j, tiles_i, 2 N): raw Gram tile R_ij = sum_c x_i[c] x_j[c] of one map of one image.
// Every output is one thread's fixed-order sum (four interleaved partial sums over the channels),
// and R_ij == R_ji bit for bit.
__global__ __launch_bounds__(256) void pw_gram_kernel(const PwArgs a, const PwMap ms, const PwMap mt,
                                                      float* __restrict__ save) {
  __shared__ __attribute__((aligned(16))) float ra[PW_TILE][PW_LDS], rb[PW_TILE][PW_LDS];
  const int P = a.P;
  const int n = blockIdx.z >> 1, which = blockIdx.z & 1;
  const PwMap& m = which ? mt : ms;
  const int i0 = blockIdx.y * PW_TILE, j0 = blockIdx.x * PW_TILE;
  const int ti = threadIdx.x / PW_TILE, tj = threadIdx.x % PW_TILE;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = 0; c0 < m.C; c0 += PW_CCH) {
    __syncthreads();
    // 32 rows, 8 threads each
    const int r = threadIdx.x / 8, l = threadIdx.x % 8;
    const int p = (r < PW_TILE ? i0 + r : j0 + r - PW_TILE);
    float* dst = r < PW_TILE ? ra[r] : rb[r - PW_TILE];
    if (p < P) {
      pw_stage_row(m, a, n, p, c0, dst, l, 8);
    } else {
      for (int q = l; q < PW_CCH; q += 8) dst[q] = 0.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < PW_CCH; c += 4) {
      const float4 u = *reinterpret_cast<const float4*>(&ra[ti][c]);
      const float4 v = *reinterpret_cast<const float4*>(&rb[tj][c]);
      acc.x = fmaf(u.x, v.x, acc.x); acc.y = fmaf(u.y, v.y, acc.y);
      acc.z = fmaf(u.z, v.z, acc.z); acc.w = fmaf(u.w, v.w, acc.w);
    }
  }
  const int i = i0 + ti, j = j0 + tj;
  if (i < P && j < P) {
    float* G = save + (long)n * pw_per_image(P) + (long)which * P * P;
    G[(long)i * P + j] = (acc.x + acc.y) + (acc.z + acc.w);
  }
}

// one workgroup per image: normalise both Gram matrices in place, the teacher's column softmax, the
// student's row log-softmax, the loss of the image in double.  Thread k owns row k (and column k).
__global__ __launch_bounds__(GS_PAIRWISE_MAX_P) void pw_loss_kernel(const PwArgs a,
                                                                    float* __restrict__ save,
                                                                    double* __restrict__ part) {
  __shared__ float ds_[GS_PAIRWISE_MAX_P], dt_[GS_PAIRWISE_MAX_P], lt_[GS_PAIRWISE_MAX_P];
  __shared__ double red[GS_PAIRWISE_MAX_P / 64];
  const int P = a.P, n = blockIdx.x, k = threadIdx.x;
  const float T = a.d.T;
  float* Gs = save + (long)n * pw_per_image(P);
  float* Gt = Gs + (long)P * P;
  float* vec = Gs + 3L * P * P;
  float* d_s = vec; float* m_s = vec + P; float* lse_s = vec + 2 * P; float* lse_t = vec + 3 * P;
  float* rsum = vec + 4 * P;
  if (k < P) {
    const float ns = sqrtf(Gs[(long)k * P + k]), nt = sqrtf(Gt[(long)k * P + k]);
    ds_[k] = fmaxf(ns, PW_EPS);
    dt_[k] = fmaxf(nt, PW_EPS);
    d_s[k] = ds_[k];
    m_s[k] = ns >= PW_EPS ? 1.f : 0.f;
  }
  __syncthreads();
  float ls = 0.f;
  if (k < P) {
    float mx = -__builtin_huge_valf();
    for (int j = 0; j < P; ++j) {
      const float gs_ = Gs[(long)k * P + j] / (ds_[k] * ds_[j]);
      Gs[(long)k * P + j] = gs_;
      Gt[(long)k * P + j] = Gt[(long)k * P + j] / (dt_[k] * dt_[j]);
      mx = fmaxf(mx, gs_ / T);
    }
    float se = 0.f;
    for (int j = 0; j < P; ++j) se += expf(Gs[(long)k * P + j] / T - mx);
    ls = mx + logf(se);
    lse_s[k] = ls;
  }
  __syncthreads();   // every row of Gt is normalised (global writes of this workgroup are visible)
  if (k < P) {       // column k of Gt: the softmax over i
    float mx = -__builtin_huge_valf();
    for (int i = 0; i < P; ++i) mx = fmaxf(mx, Gt[(long)i * P + k] / T);
    float se = 0.f;
    for (int i = 0; i < P; ++i) se += expf(Gt[(long)i * P + k] / T - mx);
    lt_[k] = mx + logf(se);
    lse_t[k] = lt_[k];
  }
  __syncthreads();
  float l = 0.f;
  if (k < P) {
    float r = 0.f;
    for (int j = 0; j < P; ++j) {
      const float A = expf(Gt[(long)k * P + j] / T - lt_[j]);
      r += A;
      l += A * (ls - Gs[(long)k * P + j] / T);
    }
    rsum[k] = r;
  }
  double acc = wave_sum_d((double)l);
  if ((k & 63) == 0) red[k >> 6] = acc;
  __syncthreads();
  if (k == 0) {
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    part[n] = t;
  }
}

// one workgroup per image, thread k owns row k: Wc (see the head of this section)
__global__ __launch_bounds__(GS_PAIRWISE_MAX_P) void pw_coef_kernel(const PwArgs a,
                                                                    float* __restrict__ save,
                                                                    float coef) {
  const int P = a.P, n = blockIdx.x, k = threadIdx.x;
  if (k >= P) return;
  const float T = a.d.T;
  const float* Gs = save + (long)n * pw_per_image(P);
  const float* Gt = Gs + (long)P * P;
  float* Wc = save + (long)n * pw_per_image(P) + 2L * P * P;
  const float* vec = Gs + 3L * P * P;
  const float* d_s = vec; const float* m_s = vec + P; const float* lse_s = vec + 2 * P;
  const float* lse_t = vec + 3 * P; const float* rsum = vec + 4 * P;
  const float dk = d_s[k], lsk = lse_s[k], ltk = lse_t[k], rk = rsum[k];
  float sg = 0.f;
  for (int j = 0; j < P; ++j) {
    const float gkj = Gs[(long)k * P + j], gjk = Gs[(long)j * P + k];
    const float Dkj = coef * (rk * expf(gkj / T - lsk) - expf(Gt[(long)k * P + j] / T - lse_t[j]));
    const float Djk = coef * (rsum[j] * expf(gjk / T - lse_s[j]) - expf(Gt[(long)j * P + k] / T - ltk));
    const float E = Dkj + Djk;
    sg += E * gkj;
    Wc[(long)k * P + j] = E / (dk * d_s[j]);
  }
  Wc[(long)k * P + k] -= m_s[k] * sg / (dk * dk);
}

__global__ __launch_bounds__(256) void pw_zero_kernel(float4* __restrict__ p, long n4) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
    p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// grid (channel chunks, N): dx[k, c] = sum_j Wc[k, j] x_j[c] for the chunk's PW_CCH channels; the
// window's chunk is staged once, thread (rg, c4) owns rows rg, rg + 16, ... and four channels.
__global__ __launch_bounds__(256) void pw_apply_kernel(const PwArgs a, const PwMap ms,
                                                       const float* __restrict__ save,
                                                       float* __restrict__ ds, int ld) {
  __shared__ __attribute__((aligned(16))) float xs[GS_PAIRWISE_MAX_P][PW_CCH];
  const int P = a.P, n = blockIdx.y, c0 = blockIdx.x * PW_CCH;
  const float* Wc = save + (long)n * pw_per_image(P) + 2L * P * P;
  for (int p = threadIdx.x / 16; p < P; p += 16) pw_stage_row(ms, a, n, p, c0, xs[p], threadIdx.x % 16, 16);
  __syncthreads();
  const int c4 = (threadIdx.x % 16) * 4, rg = threadIdx.x / 16;
  if (c0 + c4 >= ms.C) return;
  for (int k = rg; k < P; k += 16) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* wrow = Wc + (long)k * P;
    for (int j = 0; j < P; ++j) {
      const float w = wrow[j];
      const float4 v = *reinterpret_cast<const float4*>(&xs[j][c4]);
      acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y);
      acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
    }
    const int y = a.d.y0 + k / a.nx, x = a.d.x0 + k % a.nx;
    float* o = ds + (((long)n * a.d.H + y) * a.d.W + x) * ld + c0 + c4;
    // (ld is a multiple of 4 and >= Cs: a whole float4 stays inside the pixel; channels past Cs were
    // staged as zeros, so the pad columns receive zeros)
    *reinterpret_cast<float4*>(o) = acc;
  }
}

static PwMap pw_map(const float* base, long sn, long sc, long sh, long sw, int C) {
  PwMap m;
  m.base = base; m.sn = sn; m.sc = sc; m.sh = sh; m.sw = sw; m.C = C;
  m.vec = (sc == 1 && sn % 4 == 0 && sh % 4 == 0 && sw % 4 == 0 && aligned16(base)) ? 1 : 0;
  return m;
}

static int check_pw(const gs_pairwise_desc* d, PwArgs& a) {
  if (!d) return GS_E_NULL;
  if (d->N <= 0 || d->Cs <= 0 || d->Ct <= 0 || d->H <= 0 || d->W <= 0 || d->Ht <= 0 || d->Wt <= 0)
    return GS_E_BADARG;
  if (d->y0 < 0 || d->y1 <= d->y0 || d->x0 < 0 || d->x1 <= d->x0) return GS_E_BADARG;
  if (d->y1 > d->H || d->x1 > d->W || d->y1 > d->Ht || d->x1 > d->Wt) return GS_E_BADARG;
  if (!(d->T > 0.f) || d->T == __builtin_huge_valf()) return GS_E_BADARG;
  const long P = (long)(d->y1 - d->y0) * (d->x1 - d->x0);
  if (P > GS_PAIRWISE_MAX_P) return GS_E_BADARG;
  a.d = *d;
  a.P = (int)P;
  a.nx = d->x1 - d->x0;
  return GS_OK;
}

}  // namespace gs

extern "C" size_t gs_pairwise_save_bytes(const gs_pairwise_desc* d) {
  PwArgs a;
  if (check_pw(d, a)) return 0;
  return (size_t)d->N * sizeof(double) + (size_t)d->N * pw_per_image(a.P) * sizeof(float);
}

extern "C" int gs_pairwise_forward(const gs_pairwise_desc* d, const float* student,
                                   const float* teacher, float scale, float* out, void* save,
                                   size_t save_bytes, void* stream) {
  PwArgs a;
  int rc = check_pw(d, a);
  if (rc) return rc;
  if (!student || !teacher || !out || !save) return GS_E_NULL;
  if (save_bytes < gs_pairwise_save_bytes(d)) return GS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(save) & 7) return GS_E_ALIGN;
  hipStream_t st = as_stream(stream);
  double* part = static_cast<double*>(save);
  float* fsave = reinterpret_cast<float*>(part + d->N);
  const PwMap ms = pw_map(student, d->s_sn, d->s_sc, d->s_sh, d->s_sw, d->Cs);
  const PwMap mt = pw_map(teacher, d->t_sn, d->t_sc, d->t_sh, d->t_sw, d->Ct);
  const unsigned tiles = (unsigned)ceil_div(a.P, PW_TILE);
  hipLaunchKernelGGL(pw_gram_kernel, dim3(tiles, tiles, 2u * d->N), dim3(256), 0, st, a, ms, mt, fsave);
  hipLaunchKernelGGL(pw_loss_kernel, dim3(d->N), dim3(GS_PAIRWISE_MAX_P), 0, st, a, fsave, part);
  hipLaunchKernelGGL(kd_final_kernel, dim3(1), dim3(256), 0, st, part, d->N, (double)scale, out);
  return launch_status();
}

extern "C" int gs_pairwise_backward(const gs_pairwise_desc* d, const float* student, void* save,
                                    size_t save_bytes, float grad_scale, float* ds, int32_t ld_d,
                                    void* stream) {
  PwArgs a;
  int rc = check_pw(d, a);
  if (rc) return rc;
  if (!student || !save || !ds) return GS_E_NULL;
  if (ld_d < d->Cs || ld_d % 4 != 0) return GS_E_BADARG;
  if (save_bytes < gs_pairwise_save_bytes(d)) return GS_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(save) & 7) || !aligned16(ds)) return GS_E_ALIGN;
  hipStream_t st = as_stream(stream);
  float* fsave = reinterpret_cast<float*>(static_cast<double*>(save) + d->N);
  const PwMap ms = pw_map(student, d->s_sn, d->s_sc, d->s_sh, d->s_sw, d->Cs);
  const long n4 = (long)d->N * d->H * d->W * ld_d / 4;
  hipLaunchKernelGGL(pw_zero_kernel, dim3(stream_grid(n4, 256)), dim3(256), 0, st,
                     reinterpret_cast<float4*>(ds), n4);
  hipLaunchKernelGGL(pw_coef_kernel, dim3(d->N), dim3(GS_PAIRWISE_MAX_P), 0, st, a, fsave,
                     grad_scale / d->T);
  hipLaunchKernelGGL(pw_apply_kernel, dim3((unsigned)ceil_div(d->Cs, PW_CCH), d->N), dim3(256), 0, st,
                     a, ms, fsave, ds, ld_d);
  return launch_status();
}
