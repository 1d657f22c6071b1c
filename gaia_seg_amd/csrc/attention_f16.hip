// Multi-head softmax self-attention (head dimension 64) with fp16 MFMA operands: the opt-in twin of
// attention.hip (gs_attention_*_f16 in include/gaiaseg_hip.h).  Same structure -- a workgroup is 4 waves and
// owns 128 rows of one (batch, head), tiles of 32 rows are swept through LDS, the first product is oriented
// so that the next one sums over its row index, the backward is the dK/dV-owner + dQ-owner pair, no float
// atomics, fixed summation order -- with every product on v_mfma_f32_32x32x16_f16 (fp32 accumulation).
// HBM holds fp32 throughout; the softmax state (running maximum, sum, lse, delta) is fp32.
//
// Operand maps of the 32x32x16 MFMA (lane l, i = l & 31, h = l >> 5, fragment element j = 0..7):
// A[i][k = 8 h + j], B[k = 8 h + j][i]; the result has its column on the lane and row acc_row(r, h) in
// register r, as for the fp32 instruction.  A result tile X is the next product's B operand without lane
// movement: registers 8 s .. 8 s + 7, converted to fp16, are the fragment of k-step s (s = 0, 1), which
// puts row 16 s + 8 (j >> 2) + 4 h + (j & 3) of X in element j.  The A operand of that product follows the
// same k order: it is read from a TRANSPOSED LDS image [d][row of the tile], where the eight elements are
// two runs of four (8 bytes each) at rows 16 s + 4 h and 16 s + 8 + 4 h.
//
// Rounding points:
//   * Q, K, V and dO are rounded to fp16 (round to nearest even) once, where they are staged into LDS or
//     into operand registers.
//   * S = scale * Q K^T accumulates in fp32; the relative-position bias is added to S in fp32.  The
//     backward recomputes S with the same instruction and the same k order (the natural one, d = 16 s +
//     8 h + j), so exp(S - lse) agrees with the saved lse to fp32 rounding.
//   * exp(S - m) is rounded to fp16 only as the operand of the P V product; the row sum adds the fp32
//     values.  exp(S - lse) and dS = P (dP - delta) are rounded to fp16 as operands of the dV and dK / dQ
//     products.
//   * Gradient range: plain fp16 rounding of dS loses small gradients (dS goes subnormal although every
//     fp32 input is normal).  The delta pre-pass therefore also writes max|dO| of each of its workgroups;
//     every main workgroup reduces those (at most B * heads * ceil(N / 128) values; a maximum does not
//     depend on the order) and picks the power of two 2^e that brings max|dO| into [4, 8).  All products
//     run on dO * 2^e and delta * 2^e (exact), and the accumulators are multiplied by 2^-e at the store
//     (exact): gradients of dO and of dO * 2^k are the same bits up to the factor.  max|dO| == 0 (or not
//     finite) gives e = 0.  Why [4, 8): |dP| <= 64 max|dO 2^e| max|V| < 512 max|V| and |delta 2^e| obeys
//     the same bound (it is a convex combination of the row of dP), so |dS| < 1024 max|V|: below the
//     fp16 maximum 65504 for max|V| < 64, far above what a LayerNorm-ed activation times a trained weight
//     gives; past that the conversion of dS saturates at +-65504 instead of producing inf (NaN stays NaN).
//     A larger target would saturate earlier, a smaller one gives away exponent range at the small end,
//     where dS = P (dP - delta) with P ~ 1 / N is what underflows.
//
// LDS images of a 32 x 64 tile, fp16: "rows" [row][d] at a pitch of 72 halves (144 B: the 16-byte
// fragment reads of 8 consecutive lanes fall in disjoint banks) for the first products, "cols" [d][row] at
// a pitch of 36 halves (72 B: the 8-byte reads of 32 lanes cover the 64 banks once) for the second ones.
// A tile that both kinds of product read (Q and dO in the dK/dV kernel, K in the dQ kernel) is staged in
// both images from one global load.  The global loads of tile t + 1 are in flight while tile t is
// multiplied (TileRegs below).
//
// Padding as in attention.hip: a key past N gets the score -inf and p == 0 exactly, rows past N are staged
// as zeros and never read from memory, rows past N are not stored.
#include <math.h>

#include "attention_common.h"

namespace gs {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int kPitchR = 72;   // halves per row of the "rows" image
constexpr int kPitchC = 36;   // halves per row of the "cols" image
constexpr int kRowsHalves = kTK * kPitchR;
constexpr int kColsHalves = kD * kPitchC;
constexpr float kF16Max = 65504.f;

__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// A thread's share of a 32 x 64 tile on its way from memory to LDS: thread (kg, c2) holds rows 4 kg .. 4 kg + 3,
// columns 2 c2 and 2 c2 + 1.  The loads of the NEXT tile are issued before the products of the current one
// and land in LDS after them, so their latency is hidden behind the MFMAs (a register prefetch).
struct TileRegs {
  float2 v[4];
};

// rows [row0, row0 + 32) of one (batch, head) block `src` (pitch ld); rows >= N are 0 and are not read
__device__ __forceinline__ void load_tile(TileRegs& t, const float* src, int row0, int N, int ld) {
  const int c2 = threadIdx.x & 31, kg = threadIdx.x >> 5;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = row0 + 4 * kg + i;
    t.v[i] = float2{0.f, 0.f};
    if (row < N) t.v[i] = *reinterpret_cast<const float2*>(src + (int64_t)row * ld + 2 * c2);
  }
}

// the tile times mul, rounded to fp16, into the LDS images the template asks for
template <bool kRows, bool kCols>
__device__ __forceinline__ void store_tile(_Float16* rows, _Float16* cols, const TileRegs& t, float mul) {
  const int c2 = threadIdx.x & 31, kg = threadIdx.x >> 5;
  _Float16 x[4], y[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[i] = (_Float16)(t.v[i].x * mul);
    y[i] = (_Float16)(t.v[i].y * mul);
  }
  if constexpr (kRows) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<f16x2*>(rows + (4 * kg + i) * kPitchR + 2 * c2) = f16x2{x[i], y[i]};
  }
  if constexpr (kCols) {
    *reinterpret_cast<f16x4*>(cols + (2 * c2) * kPitchC + 4 * kg) = f16x4{x[0], x[1], x[2], x[3]};
    *reinterpret_cast<f16x4*>(cols + (2 * c2 + 1) * kPitchC + 4 * kg) = f16x4{y[0], y[1], y[2], y[3]};
  }
}

// k-step s (0..3) of the "rows" image: this lane's A fragment of tile row `row`, d = 16 s + 8 h + j
__device__ __forceinline__ f16x8 rows_frag(const _Float16* rows, int row, int s, int h) {
  return *reinterpret_cast<const f16x8*>(rows + row * kPitchR + 16 * s + 8 * h);
}

// k-step s (0, 1) of the "cols" image: this lane's A fragment of column d, in the k order of an
// accumulator fragment (tile rows 16 s + 8 (j >> 2) + 4 h + (j & 3))
__device__ __forceinline__ f16x8 cols_frag(const _Float16* cols, int d, int s, int h) {
  const _Float16* p = cols + d * kPitchC + 16 * s + 4 * h;
  const f16x4 lo = *reinterpret_cast<const f16x4*>(p), hi = *reinterpret_cast<const f16x4*>(p + 8);
  return f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// registers 8 s .. 8 s + 7 of an accumulator as the B fragment of k-step s
__device__ __forceinline__ f16x8 acc_frag(const f32x16& x, int s) {
  f16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = (_Float16)x[8 * s + j];
  return f;
}

// the same with the conversion saturating at the fp16 maximum (NaN stays NaN)
__device__ __forceinline__ f16x8 acc_frag_sat(const f32x16& x, int s) {
  f16x8 f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float v = x[8 * s + j];
    f[j] = (_Float16)(v > kF16Max ? kF16Max : (v < -kF16Max ? -kF16Max : v));
  }
  return f;
}

// this lane's B fragments of a row it owns, times mul: reg[s][j] = row[16 s + 8 h + j]; zeros past the end
__device__ __forceinline__ void load_row_frags(f16x8 (&reg)[4], const float* row, bool ok, int h, float mul) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    f32x4 v0 = f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
    if (ok) {
      v0 = ld4(row + 16 * s + 8 * h) * mul;
      v1 = ld4(row + 16 * s + 8 * h + 4) * mul;
    }
    reg[s] = f16x8{(_Float16)v0.x, (_Float16)v0.y, (_Float16)v0.z, (_Float16)v0.w,
                   (_Float16)v1.x, (_Float16)v1.y, (_Float16)v1.z, (_Float16)v1.w};
  }
}

// grid (ceil(N / 128), heads, B); kBias as in attention.hip's forward kernel
template <bool kBias>
__global__ __launch_bounds__(256) void attn_forward_f16_kernel(const AttnArgs a, const float* __restrict__ Q,
                                                               const float* __restrict__ K,
                                                               const float* __restrict__ V,
                                                               float* __restrict__ O, float* __restrict__ lse,
                                                               const AttnBias rb) {
  __shared__ __attribute__((aligned(16))) _Float16 sK[kRowsHalves];
  __shared__ __attribute__((aligned(16))) _Float16 sV[kColsHalves];
  __shared__ int sKoff[kBias ? kTK : 1];
  extern __shared__ float sTab[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ql = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * kTQ + wave * 32 + ql;
  const bool qok = q < a.N;
  const int64_t tok0 = (int64_t)b * a.N;
  f16x8 qf[4];
  load_row_frags(qf, Q + (tok0 + (qok ? q : 0)) * a.ldq + hd * kD, qok, h, 1.f);
  const float* Kb = K + tok0 * a.ldk + hd * kD;
  const float* Vb = V + tok0 * a.ldv + hd * kD;
  f32x16 o0 = zero16(), o1 = zero16();
  float m = -INFINITY, l = 0.f;   // l: the sum over this lane half's keys
  // the cls query (and a lane past N, whose result is dropped) reads row R whatever the key
  int qterm = rb.R, qand = 0, key0 = rb.R + 2;
  if constexpr (kBias) {
    for (int t = threadIdx.x; t < rb.R + 3; t += 256) sTab[t] = rb.table[(int64_t)t * rb.ld + hd];
    if (qok && q > 0) {
      const int iy = (q - 1) / rb.Ww, ix = (q - 1) - iy * rb.Ww;
      qterm = iy * (2 * rb.Ww - 1) + ix;
      qand = -1;
      key0 = rb.R + 1;
    }
  }
  TileRegs tk, tv;
  load_tile(tk, Kb, 0, a.N, a.ldk);
  load_tile(tv, Vb, 0, a.N, a.ldv);
  for (int k0 = 0; k0 < a.N; k0 += kTK) {
    __syncthreads();
    store_tile<true, false>(sK, nullptr, tk, 1.f);
    store_tile<false, true>(nullptr, sV, tv, 1.f);
    load_tile(tk, Kb, k0 + kTK, a.N, a.ldk);   // the next tile (nothing is read past N)
    load_tile(tv, Vb, k0 + kTK, a.N, a.ldv);
    if constexpr (kBias) {
      if (threadIdx.x < kTK) {   // key j = 1 + jy Ww + jx: (Wh - 1 - jy)(2 Ww - 1) + (Ww - 1 - jx)
        const int j = k0 + threadIdx.x;
        int off = 0;             // the cls key (replaced by key0 below) and keys past N (score -inf)
        if (j >= 1 && j < a.N) {
          const int jy = (j - 1) / rb.Ww, jx = (j - 1) - jy * rb.Ww;
          off = (rb.Wh - 1 - jy) * (2 * rb.Ww - 1) + (rb.Ww - 1 - jx);
        }
        sKoff[threadIdx.x] = off;
      }
    }
    __syncthreads();
    f32x16 s = zero16();   // S^T[key][query]
#pragma unroll
    for (int st = 0; st < 4; ++st) s = mfma16(rows_frag(sK, ql, st, h), qf[st], s);
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float sc = __fmul_rn(s[r], a.scale);
      if constexpr (kBias) {
        const int kr = acc_row(r, h);
        sc += sTab[k0 + kr == 0 ? key0 : qterm + (sKoff[kr] & qand)];
      }
      s[r] = (k0 + acc_row(r, h) < a.N) ? sc : -INFINITY;
      tmax = fmaxf(tmax, s[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m, tmax);   // finite: key k0 of every tile exists
    const float alpha = expf(m - m_new);  // 0 at the first tile
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = expf(s[r] - m_new);          // exactly 0 for a key past N
      ps += s[r];                         // the fp32 value, not the operand's rounding of it
    }
    l = l * alpha + ps;
    o0 *= alpha;
    o1 *= alpha;
#pragma unroll
    for (int st = 0; st < 2; ++st) {      // O^T[d][query] += V^T[d][key] P^T[key][query]
      const f16x8 p = acc_frag(s, st);
      o0 = mfma16(cols_frag(sV, ql, st, h), p, o0);
      o1 = mfma16(cols_frag(sV, 32 + ql, st, h), p, o1);
    }
    m = m_new;
  }
  l += __shfl_xor(l, 32, 64);
  if (qok) {
    store_row(O + (tok0 + q) * a.ldo + hd * kD, o0, o1, h, 1.0f / l, 0);
    if (h == 0) lse[((int64_t)b * a.heads + hd) * a.N + q] = m + logf(l);
  }
}

// grid (ceil(N / 128), heads, B): delta[b,h,i] = <dO, O> of the workgroup's 128 tokens (two threads per
// token, 32 columns each, summed in a fixed order) and gmax[workgroup] = max|dO| over them
__global__ __launch_bounds__(256) void attn_delta_f16_kernel(const AttnArgs a, const float* __restrict__ dO,
                                                             const float* __restrict__ O,
                                                             float* __restrict__ delta, float* __restrict__ gmax) {
  __shared__ float sMax[4];
  const int hd = blockIdx.y, b = blockIdx.z;
  const int tok = blockIdx.x * kTQ + (threadIdx.x >> 1), half = threadIdx.x & 1;
  float acc = 0.f, amax = 0.f;
  if (tok < a.N) {
    const float* g = dO + ((int64_t)b * a.N + tok) * a.lddo + hd * kD + 32 * half;
    const float* o = O + ((int64_t)b * a.N + tok) * a.ldo + hd * kD + 32 * half;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const f32x4 x = ld4(g + c * 4), y = ld4(o + c * 4);
      acc = fmaf(x.x, y.x, acc);
      acc = fmaf(x.y, y.y, acc);
      acc = fmaf(x.z, y.z, acc);
      acc = fmaf(x.w, y.w, acc);
      amax = fmaxf(amax, fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w))));
    }
  }
  const float other = __shfl_xor(acc, 1, 64);
  if (tok < a.N && half == 0) delta[((int64_t)b * a.heads + hd) * a.N + tok] = acc + other;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  if ((threadIdx.x & 63) == 0) sMax[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0)
    gmax[((int64_t)b * a.heads + hd) * gridDim.x + blockIdx.x] =
        fmaxf(fmaxf(sMax[0], sMax[1]), fmaxf(sMax[2], sMax[3]));
}

// The exponent e of the gradient scale from the pre-pass's n maxima (the same value in every thread of
// every workgroup: a maximum does not depend on the order).  2^e brings max|dO| into [4, 8); 0 for a
// maximum that is 0 or not finite; |e| <= 126 so that 2^e and 2^-e are normal floats.
__device__ __forceinline__ int grad_scale_exponent(const float* __restrict__ gmax, int64_t n, float* sMax) {
  float m = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += 256) m = fmaxf(m, gmax[i]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) sMax[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sMax[0], sMax[1]), fmaxf(sMax[2], sMax[3]));
  const int biased = (int)((__float_as_uint(m) >> 23) & 0xffu);
  if (m == 0.f || biased == 255) return 0;
  const int e = 129 - biased;
  return e > 126 ? 126 : (e < -126 ? -126 : e);
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

// grid (ceil(N / 128), heads, B): the workgroup owns dK and dV of its 128 keys
__global__ __launch_bounds__(256) void attn_backward_dkv_f16_kernel(
    const AttnArgs a, const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    const float* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ gmax, const int64_t n_gmax, float* dK, float* dV) {
  __shared__ __attribute__((aligned(16))) _Float16 sQ[kRowsHalves];
  __shared__ __attribute__((aligned(16))) _Float16 sG[kRowsHalves];
  __shared__ __attribute__((aligned(16))) _Float16 sQc[kColsHalves];
  __shared__ __attribute__((aligned(16))) _Float16 sGc[kColsHalves];
  __shared__ float sL[kTK];
  __shared__ float sD[kTK];
  __shared__ float sMax[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kl = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int key = blockIdx.x * kTQ + wave * 32 + kl;
  const bool kok = key < a.N;
  const int64_t tok0 = (int64_t)b * a.N;
  const int e = grad_scale_exponent(gmax, n_gmax, sMax);
  const float gs = pow2f(e);
  f16x8 kf[4], vf[4];
  load_row_frags(kf, K + (tok0 + (kok ? key : 0)) * a.ldk + hd * kD, kok, h, 1.f);
  load_row_frags(vf, V + (tok0 + (kok ? key : 0)) * a.ldv + hd * kD, kok, h, 1.f);
  const float* Qb = Q + tok0 * a.ldq + hd * kD;
  const float* Gb = dO + tok0 * a.lddo + hd * kD;
  const float* Lb = lse + ((int64_t)b * a.heads + hd) * a.N;
  const float* Db = delta + ((int64_t)b * a.heads + hd) * a.N;
  f32x16 dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
  TileRegs tq, tg;
  load_tile(tq, Qb, 0, a.N, a.ldq);
  load_tile(tg, Gb, 0, a.N, a.lddo);
  for (int q0 = 0; q0 < a.N; q0 += kTK) {
    __syncthreads();
    store_tile<true, true>(sQ, sQc, tq, 1.f);
    store_tile<true, true>(sG, sGc, tg, gs);
    load_tile(tq, Qb, q0 + kTK, a.N, a.ldq);   // the next tile (nothing is read past N)
    load_tile(tg, Gb, q0 + kTK, a.N, a.lddo);
    if (threadIdx.x < kTK) {
      const bool ok = q0 + (int)threadIdx.x < a.N;
      sL[threadIdx.x] = ok ? Lb[q0 + threadIdx.x] : 0.f;
      sD[threadIdx.x] = ok ? Db[q0 + threadIdx.x] * gs : 0.f;
    }
    __syncthreads();
    f32x16 s = zero16(), dp = zero16();   // S[query][key], dP[query][key]
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      s = mfma16(rows_frag(sQ, kl, st, h), kf[st], s);
      dp = mfma16(rows_frag(sG, kl, st, h), vf[st], dp);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qq = acc_row(r, h);
      const float p = (q0 + qq < a.N) ? expf(__fmul_rn(s[r], a.scale) - sL[qq]) : 0.f;
      s[r] = p;
      dp[r] = p * (dp[r] - sD[qq]);
    }
#pragma unroll
    for (int st = 0; st < 2; ++st) {      // dV^T[d][key] += dO^T[d][q] P[q][key];  dK^T += Q^T dS
      const f16x8 p = acc_frag(s, st), ds = acc_frag_sat(dp, st);
      dv0 = mfma16(cols_frag(sGc, kl, st, h), p, dv0);
      dv1 = mfma16(cols_frag(sGc, 32 + kl, st, h), p, dv1);
      dk0 = mfma16(cols_frag(sQc, kl, st, h), ds, dk0);
      dk1 = mfma16(cols_frag(sQc, 32 + kl, st, h), ds, dk1);
    }
  }
  if (kok) {
    const float inv = pow2f(-e);
    store_row(dK + (tok0 + key) * a.lddk + hd * kD, dk0, dk1, h, a.scale * inv, a.accumulate);
    store_row(dV + (tok0 + key) * a.lddv + hd * kD, dv0, dv1, h, inv, a.accumulate);
  }
}

// grid (ceil(N / 128), heads, B): the workgroup owns dQ of its 128 queries
__global__ __launch_bounds__(256) void attn_backward_dq_f16_kernel(
    const AttnArgs a, const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    const float* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ delta,
    const float* __restrict__ gmax, const int64_t n_gmax, float* dQ) {
  __shared__ __attribute__((aligned(16))) _Float16 sK[kRowsHalves];
  __shared__ __attribute__((aligned(16))) _Float16 sV[kRowsHalves];
  __shared__ __attribute__((aligned(16))) _Float16 sKc[kColsHalves];
  __shared__ float sMax[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ql = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * kTQ + wave * 32 + ql;
  const bool qok = q < a.N;
  const int64_t tok0 = (int64_t)b * a.N;
  const int e = grad_scale_exponent(gmax, n_gmax, sMax);
  const float gs = pow2f(e);
  f16x8 qf[4], gf[4];
  load_row_frags(qf, Q + (tok0 + (qok ? q : 0)) * a.ldq + hd * kD, qok, h, 1.f);
  load_row_frags(gf, dO + (tok0 + (qok ? q : 0)) * a.lddo + hd * kD, qok, h, gs);
  const int64_t stat = ((int64_t)b * a.heads + hd) * a.N + (qok ? q : 0);
  const float lse_q = qok ? lse[stat] : 0.f, delta_q = qok ? delta[stat] * gs : 0.f;
  const float* Kb = K + tok0 * a.ldk + hd * kD;
  const float* Vb = V + tok0 * a.ldv + hd * kD;
  f32x16 dq0 = zero16(), dq1 = zero16();
  TileRegs tk, tv;
  load_tile(tk, Kb, 0, a.N, a.ldk);
  load_tile(tv, Vb, 0, a.N, a.ldv);
  for (int k0 = 0; k0 < a.N; k0 += kTK) {
    __syncthreads();
    store_tile<true, true>(sK, sKc, tk, 1.f);
    store_tile<true, false>(sV, nullptr, tv, 1.f);
    load_tile(tk, Kb, k0 + kTK, a.N, a.ldk);   // the next tile (nothing is read past N)
    load_tile(tv, Vb, k0 + kTK, a.N, a.ldv);
    __syncthreads();
    f32x16 s = zero16(), dp = zero16();   // S^T[key][query], dP^T[key][query]
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      s = mfma16(rows_frag(sK, ql, st, h), qf[st], s);
      dp = mfma16(rows_frag(sV, ql, st, h), gf[st], dp);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = (k0 + acc_row(r, h) < a.N) ? expf(__fmul_rn(s[r], a.scale) - lse_q) : 0.f;
      dp[r] = p * (dp[r] - delta_q);
    }
#pragma unroll
    for (int st = 0; st < 2; ++st) {      // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
      const f16x8 ds = acc_frag_sat(dp, st);
      dq0 = mfma16(cols_frag(sKc, ql, st, h), ds, dq0);
      dq1 = mfma16(cols_frag(sKc, 32 + ql, st, h), ds, dq1);
    }
  }
  if (qok) store_row(dQ + (tok0 + q) * a.lddq + hd * kD, dq0, dq1, h, a.scale * pow2f(-e), a.accumulate);
}

inline int64_t attn_tiles(const gs_attention_desc* d) { return ceil_div(d->N, kTQ); }

// delta[B][heads][N], then max|dO| of each of the pre-pass's B * heads * ceil(N / 128) workgroups
inline size_t attn_ws_bytes_f16(const gs_attention_desc* d) {
  const int64_t floats = (int64_t)d->B * d->heads * (d->N + attn_tiles(d));
  return (size_t)ceil_div(floats * (int64_t)sizeof(float), 16) * 16;
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_attention_workspace_bytes_f16(const gs_attention_desc* d) {
  return attn_check(d) == GS_OK ? attn_ws_bytes_f16(d) : 0;
}

extern "C" int gs_attention_forward_f16(const gs_attention_desc* d, const float* q, const float* k,
                                        const float* v, float* o, float* lse, void* stream) {
  const int rc = attn_check(d);
  if (rc != GS_OK) return rc;
  if (!q || !k || !v || !o || !lse) return GS_E_NULL;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse)) return GS_E_ALIGN;
  const AttnArgs a = attn_args(d, 0);
  const dim3 grid((unsigned)attn_tiles(d), (unsigned)d->heads, (unsigned)d->B);
  hipLaunchKernelGGL(attn_forward_f16_kernel<false>, grid, dim3(256), 0, as_stream(stream), a, q, k, v, o, lse,
                     AttnBias{nullptr, 0, 0, 0, 0});
  return launch_status();
}

extern "C" int gs_attention_relpos_forward_f16(const gs_attention_desc* d, const float* q, const float* k,
                                               const float* v, const float* table, int32_t ld_table,
                                               int32_t Wh, int32_t Ww, float* o, float* lse, void* stream) {
  int rc = attn_check(d);
  if (rc == GS_OK) rc = attn_relpos_check(d, ld_table, Wh, Ww);
  if (rc != GS_OK) return rc;
  if (!q || !k || !v || !table || !o || !lse) return GS_E_NULL;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse) ||
      (reinterpret_cast<uintptr_t>(table) & 3u))
    return GS_E_ALIGN;
  const int64_t R = (2 * (int64_t)Wh - 1) * (2 * (int64_t)Ww - 1);
  const AttnArgs a = attn_args(d, 0);
  const AttnBias rb = {table, ld_table, Wh, Ww, (int32_t)R};
  const dim3 grid((unsigned)attn_tiles(d), (unsigned)d->heads, (unsigned)d->B);
  const size_t lds = (size_t)ceil_div((R + 3) * (int64_t)sizeof(float), 16) * 16;
  hipLaunchKernelGGL(attn_forward_f16_kernel<true>, grid, dim3(256), lds, as_stream(stream), a, q, k, v, o, lse,
                     rb);
  return launch_status();
}

extern "C" int gs_attention_backward_f16(const gs_attention_desc* d, const float* q, const float* k,
                                         const float* v, const float* o, const float* lse, const float* d_o,
                                         float* dq, float* dk, float* dv, int accumulate, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  const int rc = attn_check(d);
  if (rc != GS_OK) return rc;
  if (!q || !k || !v || !o || !lse || !d_o || !dq || !dk || !dv || !workspace) return GS_E_NULL;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse) ||
      !aligned16(d_o) || !aligned16(dq) || !aligned16(dk) || !aligned16(dv) || !aligned16(workspace))
    return GS_E_ALIGN;
  if (workspace_bytes < attn_ws_bytes_f16(d)) return GS_E_WORKSPACE;
  const AttnArgs a = attn_args(d, accumulate);
  float* delta = static_cast<float*>(workspace);
  float* gmax = delta + (int64_t)d->B * d->heads * d->N;
  const int64_t n_gmax = (int64_t)d->B * d->heads * attn_tiles(d);
  const dim3 grid((unsigned)attn_tiles(d), (unsigned)d->heads, (unsigned)d->B);
  hipLaunchKernelGGL(attn_delta_f16_kernel, grid, dim3(256), 0, as_stream(stream), a, d_o, o, delta, gmax);
  hipLaunchKernelGGL(attn_backward_dkv_f16_kernel, grid, dim3(256), 0, as_stream(stream), a, q, k, v, d_o, lse,
                     delta, gmax, n_gmax, dk, dv);
  hipLaunchKernelGGL(attn_backward_dq_f16_kernel, grid, dim3(256), 0, as_stream(stream), a, q, k, v, d_o, lse,
                     delta, gmax, n_gmax, dq);
  return launch_status();
}
