// OCRNet's two region operators (include/gaiaseg_hip.h), on fp32 "rows x C" views with a pitch per operand,
// float4 lanes, no float atomics: every sum over pixels goes through per-run partials and a fixed-order sum.
//
//   gather : w[b,k,p] = softmax over the P pixels of s * L[b,p,k];  ctx[b,k,:] = sum_p w[b,k,p] F[b,p,:]
//            (mmseg's SpatialGatherModule).  w is never stored: the statistics pass (the pattern of
//            csrc/cwd.hip: online max / sum per run of rows, then the runs joined by one wave) leaves max and
//            log-sum per (b, k); the product pass recomputes exp(s L - max) while it stages a run's
//            weights in LDS, and the ordered sum over the runs divides by the sum.
//   attend : a[b,p,k] = softmax over the K regions of ch^-0.5 <Q[b,p], Kr[b,k]>;  out[b,p,:] = sum_k a V[b,k,:]
//            (the core of mmseg's SelfAttentionBlock as ObjectAttentionBlock uses it).  Keys and values
//            are walked in class chunks that fit the LDS, with a running max / sum per pixel; K <= chunk
//            is the one-chunk instance of the same loop.
//
// Three kernels walk pixel rows (attend forward, attend backward, gather backward): a group of G lanes
// (csrc/convnext_ops.hip) owns a row, holds its quads in registers, and every class costs one dot product
// over the group (row_sum) and one scaled add of the class vector read from LDS.  The two
// products over pixels (ctx; dKr and dV) share one kernel pair: ocr_prod_partial_kernel sums a run of
// kProdRun rows for kProdKC classes at a time (one wave per 32 rows, 64 column quads per wave, the run's
// weights in LDS), ocr_prod_sum_kernel adds the runs of every column in a fixed order.
#include <float.h>
#include "rowwise.h"

namespace gs {
namespace {

constexpr int kStatRun = 64;      // pixel rows per workgroup of the statistics pass
constexpr int kProdRun = 128;     // pixel rows per product workgroup (32 per wave)
constexpr int kProdKC = 20;       // classes per sweep of the product kernel (Cityscapes' 19 in one)
constexpr int kRowsPerGroup = 4;  // pixel rows a lane group of the attend kernels carries in registers
constexpr int kGatherBwdRows = 32;   // pixel rows per workgroup of the gather backward
constexpr int kChunkFloats = 12288;  // class vectors staged in LDS at a time (48 KiB)

// sum over the G lanes that own a row, every lane gets it.  A whole wave sums on the DPP lanes (no LDS
// traffic, common.h); smaller groups take the xor butterfly.  G is the same in every lane of a launch and
// every lane of the wave is active where this is called.
__device__ __forceinline__ float row_sum(float v, int G) { return G == kWave ? wave_sum_dpp(v) : group_sum(v, G); }

// one online-softmax step: (m, z) absorb x
__device__ __forceinline__ void online_step(float& m, float& z, float x) {
  if (x > m) {
    z = z * expf(m - x) + 1.0f;
    m = x;
  } else {
    z += expf(x - m);
  }
}

// ---- gather: softmax statistics over the pixels of every class map ---------------------------------
struct StatArgs {
  int32_t P, K, ldl, runs, KL;   // runs of kStatRun rows per image; KL lanes across classes (power of two >= K)
  float s;
};

// grid (runs, B).  Lane (pl, kl) walks rows pl, pl + 256 / KL, ... of the run for class kl; the row lanes
// are then joined in order.  part: [B][runs][K][2] = (max, sum of exp(x - max)).
__global__ __launch_bounds__(256) void ocr_stats_partial_kernel(const StatArgs a, const float* __restrict__ logits,
                                                                float* __restrict__ part) {
  __shared__ float shm[256], shz[256];
  const int kl = threadIdx.x % a.KL, pl = threadIdx.x / a.KL, PL = 256 / a.KL;
  const int64_t b = blockIdx.y;
  const int r0 = blockIdx.x * kStatRun;
  float m = -FLT_MAX, z = 0.f;
  if (kl < a.K) {
    const float* col = logits + (b * a.P) * a.ldl + kl;
    for (int r = pl; r < kStatRun; r += PL) {
      const int row = r0 + r;
      if (row >= a.P) break;
      online_step(m, z, a.s * col[(int64_t)row * a.ldl]);
    }
  }
  shm[threadIdx.x] = m;
  shz[threadIdx.x] = z;
  __syncthreads();
  if (pl == 0 && kl < a.K) {
    float M = shm[kl];
    for (int l = 1; l < PL; ++l) M = fmaxf(M, shm[l * a.KL + kl]);
    float Z = 0.f;
    for (int l = 0; l < PL; ++l) Z += shz[l * a.KL + kl] * expf(shm[l * a.KL + kl] - M);
    float* o = part + ((b * a.runs + blockIdx.x) * a.K + kl) * 2;
    o[0] = M;
    o[1] = Z;
  }
}

// grid (K, B), one wave per (b, k): lane l joins runs l, l + 64, ... in order, then the lanes are joined (the
// max is exact in any order, the sum goes through wave_sum's fixed tree).  stats: [B][K][2] = (max, log sum);
// zsum: [B][K] = sum.
__global__ __launch_bounds__(64) void ocr_stats_final_kernel(const StatArgs a, const float* __restrict__ part,
                                                             float* __restrict__ stats, float* __restrict__ zsum) {
  const int64_t b = blockIdx.y;
  const int64_t i = b * a.K + blockIdx.x;
  const float* p = part + ((b * a.runs) * a.K + blockIdx.x) * 2;
  const int64_t step = (int64_t)a.K * 2;
  float M = -FLT_MAX;
  for (int r = threadIdx.x; r < a.runs; r += kWave) M = fmaxf(M, p[r * step]);
  for (int off = kWave / 2; off > 0; off >>= 1) M = fmaxf(M, __shfl_xor(M, off, kWave));
  float Z = 0.f;
  for (int r = threadIdx.x; r < a.runs; r += kWave) Z += p[r * step + 1] * expf(p[r * step] - M);
  Z = wave_sum(Z);
  if (threadIdx.x == 0) {
    stats[2 * i] = M;
    stats[2 * i + 1] = logf(Z);
    zsum[i] = Z;
  }
}

// ---- the product over pixels: out[b,k,:] = sum_p w[b,p,k] X[b,p,:] ---------------------------------
struct ProdArgs {
  int32_t P, K, C4, C, runs;   // runs of kProdRun rows per image
  int32_t ldx, ldw;            // pitch of X; of the weight rows (LOGITS: of the logits)
  float s;                     // LOGITS: the scale in front of the logits
};

// grid (runs, ceil(C4 / 64), B).  LOGITS: w = exp(s * wsrc[b,p,k] - stats[b,k].max), the unnormalised
// softmax weight; else w = wsrc[b,p,k].  part: [B][runs][K][C].
template <bool LOGITS>
__global__ __launch_bounds__(256) void ocr_prod_partial_kernel(const ProdArgs a, const float* __restrict__ wsrc,
                                                               const float* __restrict__ stats,
                                                               const float* __restrict__ X,
                                                               float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float w_lds[kProdRun][kProdKC];
  __shared__ f32x4 red[3][4][kWave];
  const int lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
  const int cq = blockIdx.y * kWave + lane;
  const bool col = cq < a.C4;
  const int64_t b = blockIdx.z;
  const int r0 = blockIdx.x * kProdRun, rw = wv * (kProdRun / 4);
  const float* Xb = X + (b * a.P) * a.ldx + (col ? cq * 4 : 0);
  const float* Wb = wsrc + (b * a.P) * a.ldw;
  float* pb = part + ((b * a.runs + blockIdx.x) * a.K) * a.C + cq * 4;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.K; k0 += kProdKC) {
    __syncthreads();   // the previous sweep has read w_lds and red
    for (int i = threadIdx.x; i < kProdRun * kProdKC; i += 256) {
      const int r = i / kProdKC, kk = i % kProdKC;
      const int row = r0 + r, k = k0 + kk;
      float w = 0.f;
      if (row < a.P && k < a.K) {
        const float x = Wb[(int64_t)row * a.ldw + k];
        w = LOGITS ? expf(a.s * x - stats[(b * a.K + k) * 2]) : x;
      }
      w_lds[r][kk] = w;
    }
    __syncthreads();
    f32x4 acc[kProdKC];
#pragma unroll
    for (int kk = 0; kk < kProdKC; ++kk) acc[kk] = zero;
#pragma unroll 2
    for (int i = 0; i < kProdRun / 4; ++i) {
      const int row = r0 + rw + i;
      if (row >= a.P) break;
      const f32x4 f = col ? ld4(Xb + (int64_t)row * a.ldx) : zero;
#pragma unroll
      for (int g = 0; g < kProdKC / 4; ++g) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(&w_lds[rw + i][4 * g]);
        acc[4 * g + 0] += f * w4.x;
        acc[4 * g + 1] += f * w4.y;
        acc[4 * g + 2] += f * w4.z;
        acc[4 * g + 3] += f * w4.w;
      }
    }
    // the four waves' sums, four classes at a time: wave 0 adds waves 1, 2, 3 in order
#pragma unroll
    for (int g = 0; g < kProdKC / 4; ++g) {
      if (g) __syncthreads();
      if (wv) {
#pragma unroll
        for (int j = 0; j < 4; ++j) red[wv - 1][j][lane] = acc[4 * g + j];
      }
      __syncthreads();
      if (wv == 0 && col) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + 4 * g + j;
          if (k < a.K) st4(pb + (int64_t)k * a.C, ((acc[4 * g + j] + red[0][j][lane]) + red[1][j][lane]) + red[2][j][lane]);
        }
      }
    }
  }
}

struct ProdSumArgs {
  int32_t K, C4, C, runs, ldo;
  float scale;                 // without zsum: out = scale * sum
};

// grid (ceil(C4 / 16), K, B): col_runs_sum_kernel's order (lane l sums runs l, l + 16, ..., then the 16 lane
// sums in order).  zsum given: out = sum / zsum[b,k] (the softmax normalisation of the gather).
__global__ __launch_bounds__(256) void ocr_prod_sum_kernel(const ProdSumArgs a, const float* __restrict__ part,
                                                           const float* __restrict__ zsum, float* __restrict__ out) {
  __shared__ f32x4 sh[kColLanes][kColQuads];
  const int ql = threadIdx.x % kColQuads, pl = threadIdx.x / kColQuads;
  const int cq = blockIdx.x * kColQuads + ql;
  const int k = blockIdx.y;
  const int64_t b = blockIdx.z;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (cq < a.C4)
    for (int r = pl; r < a.runs; r += kColLanes) s += ld4(part + ((b * a.runs + r) * a.K + k) * a.C + cq * 4);
  sh[pl][ql] = s;
  __syncthreads();
  if (pl == 0 && cq < a.C4) {
    f32x4 t = sh[0][ql];
#pragma unroll
    for (int l = 1; l < kColLanes; ++l) t += sh[l][ql];
    t = zsum ? t / zsum[b * a.K + k] : t * a.scale;
    st4(out + (b * a.K + k) * a.ldo + cq * 4, t);
  }
}

// ---- gather backward ------------------------------------------------------------------------------
// t[b,k] = <dctx[b,k,:], ctx[b,k,:]>.  grid (K, B), one wave.
__global__ __launch_bounds__(64) void ocr_gather_t_kernel(const float* __restrict__ dctx,
                                                          const float* __restrict__ ctx, float* __restrict__ t,
                                                          const int K, const int C4, const int lddc,
                                                          const int ldc) {
  const int64_t i = (int64_t)blockIdx.y * K + blockIdx.x;
  float s = 0.f;
  for (int q = threadIdx.x; q < C4; q += kWave) s += hsum(ld4(dctx + i * lddc + q * 4) * ld4(ctx + i * ldc + q * 4));
  s = wave_sum(s);
  if (threadIdx.x == 0) t[i] = s;
}

struct GatherBwdArgs {
  int32_t P, K, C4, C, G, KC;
  int32_t ldl, ldf, lddc, lddl, lddf;
  float s;
  int32_t accumulate;
};

// grid (ceil(P / kGatherBwdRows), B).  dctx is walked in chunks of KC classes staged in LDS; a group of G
// lanes owns a pixel row with its NQ quads per lane in registers:
//   dw = <dctx[k], F[p]>,  w = exp(s L - max - lse),  dL[p,k] = s w (dw - t[k]),  dF[p] (+)= sum_k w dctx[k]
// dF is written after the first chunk and added to after the others (by the thread that wrote it).
template <int NQ>
__global__ __launch_bounds__(256) void ocr_gather_bwd_kernel(const GatherBwdArgs a, const float* __restrict__ logits,
                                                             const float* __restrict__ feats,
                                                             const float* __restrict__ stats,
                                                             const float* __restrict__ tdot,
                                                             const float* __restrict__ dctx,
                                                             float* __restrict__ dlogits, float* dfeats) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* dc = smem;                               // [KC][C]
  float* st = smem + (size_t)a.KC * a.C;          // [KC][3]: max, lse, t
  const int G = a.G, gl = threadIdx.x % G, grp = threadIdx.x / G, ngrp = 256 / G;
  const int64_t b = blockIdx.y;
  const int r0 = blockIdx.x * kGatherBwdRows;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  int chunk = 0;
  for (int k0 = 0; k0 < a.K; k0 += a.KC, ++chunk) {
    const int kn = min(a.KC, a.K - k0);
    __syncthreads();
    for (int i = threadIdx.x; i < kn * a.C4; i += 256) {
      const int kk = i / a.C4, q = i % a.C4;
      st4(dc + kk * a.C + q * 4, ld4(dctx + (b * a.K + k0 + kk) * a.lddc + q * 4));
    }
    for (int i = threadIdx.x; i < kn; i += 256) {
      st[3 * i] = stats[(b * a.K + k0 + i) * 2];
      st[3 * i + 1] = stats[(b * a.K + k0 + i) * 2 + 1];
      st[3 * i + 2] = tdot[b * a.K + k0 + i];
    }
    __syncthreads();
    for (int r = grp; r < kGatherBwdRows; r += ngrp) {
      const int row = r0 + r;
      const bool live = row < a.P;
      const int64_t pix = b * a.P + (live ? row : a.P - 1);
      f32x4 f[NQ], acc[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int q = gl + j * G;
        f[j] = q < a.C4 ? ld4(feats + pix * a.ldf + q * 4) : zero;
        acc[j] = zero;
      }
      const float* lrow = logits + pix * a.ldl + k0;
      float* dlrow = dlogits + pix * a.lddl + k0;
      for (int kk = 0; kk < kn; ++kk) {
        f32x4 d[NQ];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const int q = gl + j * G;
          d[j] = q < a.C4 ? ld4(dc + kk * a.C + q * 4) : zero;
          dot += hsum(f[j] * d[j]);
        }
        const float dw = row_sum(dot, G);
        const float w = expf((a.s * lrow[kk] - st[3 * kk]) - st[3 * kk + 1]);
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[j] += d[j] * w;
        if (live && gl == kk % G) dlrow[kk] = a.s * w * (dw - st[3 * kk + 2]);
      }
      if (live) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          const int q = gl + j * G;
          if (q < a.C4) {
            float* p = dfeats + pix * a.lddf + q * 4;
            st4(p, (a.accumulate || chunk) ? ld4(p) + acc[j] : acc[j]);
          }
        }
      }
    }
  }
  // the pad columns of the logits' float4 pitch
  const int pad = (a.K + 3) / 4 * 4 - a.K;
  for (int i = threadIdx.x; i < kGatherBwdRows * pad; i += 256) {
    const int row = r0 + i / pad;
    if (row < a.P) dlogits[(b * a.P + row) * a.lddl + a.K + i % pad] = 0.f;
  }
}

// ---- attend ---------------------------------------------------------------------------------------
struct AttendArgs {
  int32_t P, K, C4, C, G, KC, ldw;   // ldw: pitch of the backward's a / ds rows in the workspace
  int32_t ldq, ldk, ldv, ldo, lddq, lddo;
  float scale;
};

// stage classes k0 .. k0 + kn - 1 of keys and values (active columns only) into ks / vs [KC][C]
__device__ __forceinline__ void stage_kv(const AttendArgs& a, int64_t b, int k0, int kn, const float* kr,
                                         const float* v, float* ks, float* vs) {
  for (int i = threadIdx.x; i < kn * a.C4; i += 256) {
    const int kk = i / a.C4, q = i % a.C4;
    st4(ks + kk * a.C + q * 4, ld4(kr + (b * a.K + k0 + kk) * a.ldk + q * 4));
    st4(vs + kk * a.C + q * 4, ld4(v + (b * a.K + k0 + kk) * a.ldv + q * 4));
  }
}

// grid (ceil(P / (kRowsPerGroup * 256 / G)), B).  A group of G lanes owns kRowsPerGroup pixel rows.
template <int NQ>
__global__ __launch_bounds__(256) void ocr_attend_fwd_kernel(const AttendArgs a, const float* __restrict__ q,
                                                             const float* __restrict__ kr,
                                                             const float* __restrict__ v, float* __restrict__ out,
                                                             float* __restrict__ lse) {
  constexpr int R = kRowsPerGroup;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ks = smem;
  float* vs = smem + (size_t)a.KC * a.C;
  const int G = a.G, gl = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t b = blockIdx.y;
  const int row0 = (blockIdx.x * (256 / G) + grp) * R;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 qr[R][NQ], acc[R][NQ];
  float m[R], z[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int64_t pix = b * a.P + min(row0 + i, a.P - 1);
    m[i] = -FLT_MAX;
    z[i] = 0.f;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int c = gl + j * G;
      qr[i][j] = c < a.C4 ? ld4(q + pix * a.ldq + c * 4) : zero;
      acc[i][j] = zero;
    }
  }
  for (int k0 = 0; k0 < a.K; k0 += a.KC) {
    const int kn = min(a.KC, a.K - k0);
    __syncthreads();
    stage_kv(a, b, k0, kn, kr, v, ks, vs);
    __syncthreads();
    for (int kk = 0; kk < kn; ++kk) {
      f32x4 kq[NQ], vq[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int c = gl + j * G;
        kq[j] = c < a.C4 ? ld4(ks + kk * a.C + c * 4) : zero;
        vq[j] = c < a.C4 ? ld4(vs + kk * a.C + c * 4) : zero;
      }
#pragma unroll
      for (int i = 0; i < R; ++i) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NQ; ++j) dot += hsum(qr[i][j] * kq[j]);
        const float s = row_sum(dot, G) * a.scale;
        const float mn = fmaxf(m[i], s);
        const float alpha = expf(m[i] - mn), p = expf(s - mn);
        z[i] = z[i] * alpha + p;
        m[i] = mn;
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[i][j] = acc[i][j] * alpha + vq[j] * p;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int row = row0 + i;
    if (row >= a.P) continue;
    const int64_t pix = b * a.P + row;
    const float inv = 1.0f / z[i];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int c = gl + j * G;
      if (c < a.C4) st4(out + pix * a.ldo + c * 4, acc[i][j] * inv);
    }
    if (gl == 0) lse[pix] = m[i] + logf(z[i]);
  }
}

// the same walk for the backward: with D = <dout[p], out[p]> (= sum_k a da),
//   a = exp(scale <q, k> - lse),  da = <dout, v>,  ds = a (da - D),  dq += scale ds k
// and a, ds go to the workspace rows wa / wd [B*P][ldw] for the two products over pixels (dV, dKr).
template <int NQ>
__global__ __launch_bounds__(256) void ocr_attend_bwd_kernel(const AttendArgs a, const float* __restrict__ q,
                                                             const float* __restrict__ kr,
                                                             const float* __restrict__ v,
                                                             const float* __restrict__ out,
                                                             const float* __restrict__ lse,
                                                             const float* __restrict__ dout, float* __restrict__ dq,
                                                             float* __restrict__ wa, float* __restrict__ wd) {
  constexpr int R = kRowsPerGroup;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ks = smem;
  float* vs = smem + (size_t)a.KC * a.C;
  const int G = a.G, gl = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t b = blockIdx.y;
  const int row0 = (blockIdx.x * (256 / G) + grp) * R;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 qr[R][NQ], go[R][NQ], acc[R][NQ];
  float ls[R], D[R];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int64_t pix = b * a.P + min(row0 + i, a.P - 1);
    ls[i] = lse[pix];
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int c = gl + j * G;
      qr[i][j] = c < a.C4 ? ld4(q + pix * a.ldq + c * 4) : zero;
      go[i][j] = c < a.C4 ? ld4(dout + pix * a.lddo + c * 4) : zero;
      acc[i][j] = zero;
      if (c < a.C4) dot += hsum(go[i][j] * ld4(out + pix * a.ldo + c * 4));
    }
    D[i] = row_sum(dot, G);
  }
  for (int k0 = 0; k0 < a.K; k0 += a.KC) {
    const int kn = min(a.KC, a.K - k0);
    __syncthreads();
    stage_kv(a, b, k0, kn, kr, v, ks, vs);
    __syncthreads();
    for (int kk = 0; kk < kn; ++kk) {
      f32x4 kq[NQ], vq[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const int c = gl + j * G;
        kq[j] = c < a.C4 ? ld4(ks + kk * a.C + c * 4) : zero;
        vq[j] = c < a.C4 ? ld4(vs + kk * a.C + c * 4) : zero;
      }
#pragma unroll
      for (int i = 0; i < R; ++i) {
        float sd = 0.f, dd = 0.f;
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
          sd += hsum(qr[i][j] * kq[j]);
          dd += hsum(go[i][j] * vq[j]);
        }
        const float s = row_sum(sd, G) * a.scale, da = row_sum(dd, G);
        const float p = expf(s - ls[i]);
        const float ds = p * (da - D[i]);
        const float g = ds * a.scale;
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[i][j] += kq[j] * g;
        const int row = row0 + i;
        if (row < a.P && gl == kk % G) {
          const int64_t o = (b * a.P + row) * a.ldw + k0 + kk;
          wa[o] = p;
          wd[o] = ds;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int row = row0 + i;
    if (row >= a.P) continue;
    const int64_t pix = b * a.P + row;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int c = gl + j * G;
      if (c < a.C4) st4(dq + pix * a.lddq + c * 4, acc[i][j]);
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------
constexpr int kMaxClasses = GS_OCR_MAX_CLASSES;

int sizes_check(int32_t B, int32_t P, int32_t K, int32_t C, int32_t c_max) {
  if (B <= 0 || P <= 0 || K <= 0 || C <= 0) return GS_E_BADARG;
  if (K > kMaxClasses || C > c_max || B > 65535) return GS_E_BADARG;
  if (C % 4) return GS_E_ALIGN;
  if ((int64_t)B * P > INT32_MAX) return GS_E_BADARG;
  return GS_OK;
}

int pitch_check(const int32_t* ld, const int32_t* width, int n) {
  for (int i = 0; i < n; ++i)
    if (ld[i] % 4) return GS_E_ALIGN;
  for (int i = 0; i < n; ++i)
    if (ld[i] < width[i]) return GS_E_BADARG;
  return GS_OK;
}

int gather_check(const gs_ocr_gather_desc* d) {
  if (!d) return GS_E_NULL;
  int rc = sizes_check(d->B, d->P, d->K, d->C, GS_OCR_GATHER_MAX_CHANNELS);
  if (rc != GS_OK) return rc;
  const int32_t ld[6] = {d->ldl, d->ldf, d->ldc, d->lddl, d->lddf, d->lddc};
  const int32_t w[6] = {d->K, d->C, d->C, d->K, d->C, d->C};
  rc = pitch_check(ld, w, 6);
  if (rc != GS_OK) return rc;
  if (!(d->scale == d->scale) || d->scale > FLT_MAX || d->scale < -FLT_MAX) return GS_E_BADARG;
  return GS_OK;
}

int attend_check(const gs_ocr_attend_desc* d) {
  if (!d) return GS_E_NULL;
  int rc = sizes_check(d->B, d->P, d->K, d->ch, GS_OCR_ATTEND_MAX_CHANNELS);
  if (rc != GS_OK) return rc;
  const int32_t ld[8] = {d->ldq, d->ldk, d->ldv, d->ldo, d->lddq, d->lddk, d->lddv, d->lddo};
  const int32_t w[8] = {d->ch, d->ch, d->ch, d->ch, d->ch, d->ch, d->ch, d->ch};
  return pitch_check(ld, w, 8);
}

inline size_t up4(size_t n) { return (n + 3) / 4 * 4; }

// floats of the product kernels' partials for one [K][C] result per image
inline size_t prod_floats(int32_t B, int32_t P, int32_t K, int32_t C) {
  return (size_t)B * ceil_div(P, kProdRun) * K * C;
}

// gather workspace: [stat partials | zsum | t | product partials], each a float4 multiple
struct GatherWs {
  size_t stat, zsum, t, prod;   // offsets in floats
  size_t floats;
};
GatherWs gather_ws(const gs_ocr_gather_desc* d) {
  GatherWs w;
  w.stat = 0;
  w.zsum = up4((size_t)d->B * ceil_div(d->P, kStatRun) * d->K * 2);
  w.t = w.zsum + up4((size_t)d->B * d->K);
  w.prod = w.t + up4((size_t)d->B * d->K);
  w.floats = w.prod + prod_floats(d->B, d->P, d->K, d->C);
  return w;
}

// attend workspace: [a rows | ds rows | product partials]
struct AttendWs {
  size_t ldw, a, ds, prod, floats;
};
AttendWs attend_ws(const gs_ocr_attend_desc* d) {
  AttendWs w;
  w.ldw = up4(d->K);
  w.a = 0;
  w.ds = (size_t)d->B * d->P * w.ldw;
  w.prod = 2 * w.ds;
  w.floats = w.prod + prod_floats(d->B, d->P, d->K, d->ch);
  return w;
}

void launch_product(bool from_logits, int32_t B, int32_t P, int32_t K, int32_t C, const float* wsrc, int32_t ldw,
                    float s, const float* stats, const float* X, int32_t ldx, float* part, const float* zsum,
                    float scale, float* out, int32_t ldo, hipStream_t st) {
  ProdArgs a;
  a.P = P; a.K = K; a.C4 = C / 4; a.C = C; a.runs = (int32_t)ceil_div(P, kProdRun);
  a.ldx = ldx; a.ldw = ldw; a.s = s;
  const dim3 grid((unsigned)a.runs, (unsigned)ceil_div(a.C4, kWave), (unsigned)B);
  if (from_logits)
    hipLaunchKernelGGL(ocr_prod_partial_kernel<true>, grid, dim3(256), 0, st, a, wsrc, stats, X, part);
  else
    hipLaunchKernelGGL(ocr_prod_partial_kernel<false>, grid, dim3(256), 0, st, a, wsrc, stats, X, part);
  ProdSumArgs s2;
  s2.K = K; s2.C4 = C / 4; s2.C = C; s2.runs = a.runs; s2.ldo = ldo; s2.scale = scale;
  hipLaunchKernelGGL(ocr_prod_sum_kernel, dim3((unsigned)ceil_div(s2.C4, kColQuads), (unsigned)K, (unsigned)B),
                     dim3(256), 0, st, s2, part, zsum, out);
}

// classes per LDS chunk for `vectors` staged matrices of width C
inline int32_t chunk_classes(int32_t K, int32_t C, int vectors) {
  const int32_t kc = kChunkFloats / (vectors * C);
  return K < kc ? K : kc;
}

AttendArgs attend_args(const gs_ocr_attend_desc* d) {
  AttendArgs a;
  a.P = d->P; a.K = d->K; a.C4 = d->ch / 4; a.C = d->ch; a.G = row_group(a.C4);
  a.KC = chunk_classes(d->K, d->ch, 2);
  a.ldw = (int32_t)up4(d->K);
  a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv; a.ldo = d->ldo; a.lddq = d->lddq; a.lddo = d->lddo;
  a.scale = 1.0f / sqrtf((float)d->ch);
  return a;
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_ocr_gather_workspace_bytes(const gs_ocr_gather_desc* d) {
  return gather_check(d) == GS_OK ? gather_ws(d).floats * sizeof(float) : 0;
}

extern "C" int gs_ocr_gather_forward(const gs_ocr_gather_desc* d, const float* logits, const float* feats,
                                     float* ctx, float* stats, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  const int rc = gather_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({logits, feats, ctx, stats, workspace})) return GS_E_NULL;
  if (!all_aligned16({logits, feats, ctx, workspace})) return GS_E_ALIGN;
  const GatherWs w = gather_ws(d);
  if (workspace_bytes < w.floats * sizeof(float)) return GS_E_WORKSPACE;
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  StatArgs a;
  a.P = d->P; a.K = d->K; a.ldl = d->ldl; a.runs = (int32_t)ceil_div(d->P, kStatRun); a.s = d->scale;
  a.KL = 1;
  while (a.KL < d->K) a.KL *= 2;
  hipLaunchKernelGGL(ocr_stats_partial_kernel, dim3((unsigned)a.runs, (unsigned)d->B), dim3(256), 0, st, a, logits,
                     ws + w.stat);
  hipLaunchKernelGGL(ocr_stats_final_kernel, dim3((unsigned)d->K, (unsigned)d->B), dim3(64), 0, st, a, ws + w.stat,
                     stats, ws + w.zsum);
  launch_product(true, d->B, d->P, d->K, d->C, logits, d->ldl, d->scale, stats, feats, d->ldf, ws + w.prod,
                 ws + w.zsum, 1.0f, ctx, d->ldc, st);
  return launch_status();
}

extern "C" int gs_ocr_gather_backward(const gs_ocr_gather_desc* d, const float* logits, const float* feats,
                                      const float* ctx, const float* stats, const float* dctx, float* dlogits,
                                      float* dfeats, int accumulate_dfeats, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const int rc = gather_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({logits, feats, ctx, stats, dctx, dlogits, dfeats, workspace})) return GS_E_NULL;
  if (!all_aligned16({logits, feats, ctx, dctx, dlogits, dfeats, workspace})) return GS_E_ALIGN;
  const GatherWs w = gather_ws(d);
  if (workspace_bytes < w.floats * sizeof(float)) return GS_E_WORKSPACE;
  float* tdot = static_cast<float*>(workspace) + w.t;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ocr_gather_t_kernel, dim3((unsigned)d->K, (unsigned)d->B), dim3(64), 0, st, dctx, ctx, tdot,
                     d->K, d->C / 4, d->lddc, d->ldc);
  GatherBwdArgs a;
  a.P = d->P; a.K = d->K; a.C4 = d->C / 4; a.C = d->C; a.G = row_group(a.C4);
  a.KC = chunk_classes(d->K, d->C, 1);
  a.ldl = d->ldl; a.ldf = d->ldf; a.lddc = d->lddc; a.lddl = d->lddl; a.lddf = d->lddf;
  a.s = d->scale; a.accumulate = accumulate_dfeats ? 1 : 0;
  const dim3 grid((unsigned)ceil_div(d->P, kGatherBwdRows), (unsigned)d->B);
  const size_t lds = ((size_t)a.KC * a.C + (size_t)a.KC * 3) * sizeof(float);
  const int nq = (int)ceil_div(a.C4, a.G);
#define GS_GATHER_BWD(NQ)                                                                                     \
  hipLaunchKernelGGL(ocr_gather_bwd_kernel<NQ>, grid, dim3(256), lds, st, a, logits, feats, stats, tdot, dctx, \
                     dlogits, dfeats)
  if (nq <= 1) GS_GATHER_BWD(1);
  else if (nq <= 2) GS_GATHER_BWD(2);
  else if (nq <= 4) GS_GATHER_BWD(4);
  else GS_GATHER_BWD(8);
#undef GS_GATHER_BWD
  return launch_status();
}

extern "C" size_t gs_ocr_attend_workspace_bytes(const gs_ocr_attend_desc* d) {
  return attend_check(d) == GS_OK ? attend_ws(d).floats * sizeof(float) : 0;
}

extern "C" int gs_ocr_attend_forward(const gs_ocr_attend_desc* d, const float* q, const float* k, const float* v,
                                     float* out, float* lse, void* stream) {
  const int rc = attend_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({q, k, v, out, lse})) return GS_E_NULL;
  if (!all_aligned16({q, k, v, out})) return GS_E_ALIGN;
  const AttendArgs a = attend_args(d);
  const dim3 grid((unsigned)ceil_div(d->P, kRowsPerGroup * (256 / a.G)), (unsigned)d->B);
  const size_t lds = (size_t)2 * a.KC * a.C * sizeof(float);
  if (ceil_div(a.C4, a.G) <= 1)
    hipLaunchKernelGGL(ocr_attend_fwd_kernel<1>, grid, dim3(256), lds, as_stream(stream), a, q, k, v, out, lse);
  else
    hipLaunchKernelGGL(ocr_attend_fwd_kernel<2>, grid, dim3(256), lds, as_stream(stream), a, q, k, v, out, lse);
  return launch_status();
}

extern "C" int gs_ocr_attend_backward(const gs_ocr_attend_desc* d, const float* q, const float* k, const float* v,
                                      const float* out, const float* lse, const float* dout, float* dq, float* dk,
                                      float* dv, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = attend_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({q, k, v, out, lse, dout, dq, dk, dv, workspace})) return GS_E_NULL;
  if (!all_aligned16({q, k, v, out, dout, dq, dk, dv, workspace})) return GS_E_ALIGN;
  const AttendWs w = attend_ws(d);
  if (workspace_bytes < w.floats * sizeof(float)) return GS_E_WORKSPACE;
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = as_stream(stream);
  const AttendArgs a = attend_args(d);
  const dim3 grid((unsigned)ceil_div(d->P, kRowsPerGroup * (256 / a.G)), (unsigned)d->B);
  const size_t lds = (size_t)2 * a.KC * a.C * sizeof(float);
  if (ceil_div(a.C4, a.G) <= 1)
    hipLaunchKernelGGL(ocr_attend_bwd_kernel<1>, grid, dim3(256), lds, st, a, q, k, v, out, lse, dout, dq, ws + w.a,
                       ws + w.ds);
  else
    hipLaunchKernelGGL(ocr_attend_bwd_kernel<2>, grid, dim3(256), lds, st, a, q, k, v, out, lse, dout, dq, ws + w.a,
                       ws + w.ds);
  // dV = sum_p a dout;  dKr = ch^-0.5 sum_p ds Q: the partials' storage serves one after the other
  launch_product(false, d->B, d->P, d->K, d->ch, ws + w.a, a.ldw, 0.f, nullptr, dout, d->lddo, ws + w.prod, nullptr,
                 1.0f, dv, d->lddv, st);
  launch_product(false, d->B, d->P, d->K, d->ch, ws + w.ds, a.ldw, 0.f, nullptr, q, d->ldq, ws + w.prod, nullptr,
                 a.scale, dk, d->lddk, st);
  return launch_status();
}
