// Multi-head softmax self-attention (head dimension 64) on fp32 "rows x C" token views, forward and
// backward (gs_attention_* and gs_attention_*_f16 in include/gaiaseg_hip.h).  The three main kernels --
// forward (with or without BEiT's relative-position bias), dK / dV and dQ -- and the host side of every
// entry are written once here, as templates over an OPERAND POLICY that says how a matrix product is fed:
//
//   F32Ops (attention.hip)     : every product on the exact fp32 MFMA v_mfma_f32_32x32x2_f32 (a k-ordered
//                                fp32 fma chain), so the operator is fp32-accurate in every precision mode.
//   F16Ops (attention_f16.hip) : the opt-in fp16-operand form: every product on v_mfma_f32_32x32x16_f16
//                                (fp32 accumulation).  HBM holds fp32 throughout; the softmax state (running
//                                maximum, sum, lse, delta) is fp32.
//
// Each of the two files defines its policy, its delta pre-pass (the two sum in different orders and stay two
// kernels) and its extern "C" entries, which are one-line calls of the host templates at the end of this
// file.  No N x N matrix is stored, no float atomics are used and every sum has a fixed order: results are
// bit-identical from run to run.
//
// Structure, common to both policies.  A workgroup is 4 waves and owns kTQ = 128 rows of one (batch, head),
// 32 per wave, in operand registers; tiles of kTK = 32 rows of the other operand are swept through LDS.
// Both MFMAs (lane l, i = l & 31, h = l >> 5) give a 32x32 result with its COLUMN on the lane and row
// (r & 3) + 8 (r >> 2) + 4 h in register r (acc_row below).  Each product is oriented so that the index the
// NEXT product sums over is the result's row index: a result register is then (part of) the next MFMA's B
// operand as it stands, and everything that belongs to the column (a query's running maximum, sum, lse and
// delta; a key's dK / dV) lives on the lane.
//
//   forward  : Q in registers, key tiles of K and V through LDS.  S^T = K Q^T puts the query on the lane:
//              the row maximum and sum are 16 register steps and one exchange between the lane halves.
//              O^T += V^T P^T keeps the query on the lane, so the online rescale is per lane.  A key past N
//              gets the score -inf, hence p = exp(-inf) = 0 exactly.
//   relpos   : the same kernel with BEiT's relative-position bias added to the scaled score (template
//              parameter kBias; the bias-free instantiation contains none of it).  The N x N bias is never
//              formed: the head's column of the table (at most 8192 floats) is staged in LDS once per
//              workgroup and gathered per score.  Lanes of a half wave hold consecutive queries, so their
//              table rows are consecutive except where the window row wraps: few bank conflicts, and no
//              gather traffic beside the K / V stream in L2.  Forward only.
//   backward : delta[b,h,i] = <dO, O> by a pre-pass.  Then two kernels:
//              dK / dV : a workgroup owns 128 keys (K and V in registers) and sweeps query tiles of 32 (Q,
//                        dO, lse, delta in LDS): S = Q K^T and dP = dO V^T have the key on the lane,
//                        dV^T += dO^T P and dK^T += Q^T dS take them as B operands.
//              dQ      : a workgroup owns 128 queries (Q, dO in registers) and sweeps key tiles of 32:
//                        S^T and dP^T as in the forward, dQ^T += K^T dS^T.
//              Seven products instead of five, and no sum across workgroups.
//   padding  : rows past N are staged as zeros and never read from memory, rows past N are not stored.
//   lengths  : the kernels take the number of queries Nq and of keys Nk separately (AttnArgs): the forward and
//              dQ own queries and sweep keys, dK / dV owns keys and sweeps queries.  The self-attention
//              entries run them at Nq = Nk = N; gs_attention_kv_* (the Mix Transformer's attention to a
//              reduced map, fp32 operands only) at any two lengths.
//   slabs    : with few keys and many queries the dK / dV grid of one workgroup per 128 keys leaves the chip
//              idle, so its grid has a slab dimension: S slabs of whole query tiles, each workgroup sweeping
//              one slab.  S == 1 (always, for the self-attention entries) stores dK / dV directly; S > 1
//              stores every slab's partial in the workspace and attn_slab_combine_kernel adds the slabs in
//              slab order: still no atomics and a fixed order.  attn_split_plan chooses S.
//
// What a policy supplies (and nothing else differs between the two precisions):
//   Row                  the operand registers of a row the lane owns, and load_row (with a multiplier);
//   Tile<kRows, kCols>   the LDS image(s) of a 32 x 64 tile: "rows" feeds the first products (a tile row
//                        times an owned row, 64 deep, kSteps1 MFMAs: mma1), "cols" the second ones (tile
//                        columns times an accumulator, 32 deep, kSteps2 MFMAs: frag / frag_sat and mma2);
//   TileLoad, load_tile, store_tile
//                        a tile's way from memory to LDS.  Every sweep is: barrier, store_tile of the
//                        current tile, load_tile of the next one, barrier, products;
//   GradMax, grad_exponent
//                        the exponent e of the gradient scale 2^e (below; always 0 for fp32, where every
//                        multiplication by 2^0 folds away at compile time);
//   ws_bytes, launch_delta
//                        the backward's workspace and its pre-pass.
//
// fp32 operands.  MFMA operand map: A[i][k = h], B[k = h][j = i].  Row: reg[s] = row[2 s + h].  One LDS
// image serves both kinds of product: 32 rows x 64 floats at a pitch of 66 floats, read by rows ([lane row]
// [2 s + h], conflict free at that pitch) for the first products and by columns ([acc_row][lane column])
// for the second ones.  A tile goes from global memory straight into LDS between the two barriers
// (load_tile only records what to load): there is no register prefetch.  The delta pre-pass is one thread
// per (token, head) and forms the same d-ordered fma chain as the MFMA (a single token gives dP == delta
// bit for bit, so dQ = dK = 0 exactly).
//
// fp16 operands.  MFMA operand map (fragment element j = 0..7): A[i][k = 8 h + j], B[k = 8 h + j][i].  A
// result tile X is the next product's B operand without lane movement: registers 8 s .. 8 s + 7, converted
// to fp16, are the fragment of k-step s (s = 0, 1), which puts row 16 s + 8 (j >> 2) + 4 h + (j & 3) of X in
// element j.  The A operand of that product follows the same k order: it is read from a TRANSPOSED LDS
// image [d][row of the tile], where the eight elements are two runs of four (8 bytes each) at rows 16 s +
// 4 h and 16 s + 8 + 4 h.
//   LDS images of a 32 x 64 tile, fp16: "rows" [row][d] at a pitch of 72 halves (144 B: the 16-byte
//   fragment reads of 8 consecutive lanes fall in disjoint banks) for the first products, "cols" [d][row] at
//   a pitch of 36 halves (72 B: the 8-byte reads of 32 lanes cover the 64 banks once) for the second ones.
//   A tile that both kinds of product read (Q and dO in the dK/dV kernel, K in the dQ kernel) is staged in
//   both images from one global load.  The global loads of tile t + 1 are in flight while tile t is
//   multiplied (TileLoad holds them in registers).
//   Rounding points:
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
#pragma once
#include <math.h>

#include <algorithm>

#include "common.h"

namespace gs {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kD = 64;        // head dimension
constexpr int kTK = 32;       // rows of a tile that is swept through LDS
constexpr int kTQ = 128;      // rows a workgroup owns (32 per wave)

__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}
__device__ __forceinline__ float pow2f(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

// Nq queries attend to Nk keys per image (the self-attention entries pass Nq = Nk = N).  slab_rows: the
// queries one workgroup of the dK / dV kernel sweeps (a multiple of kTK; >= Nq when there is one slab).
struct AttnArgs {
  int32_t B, Nq, Nk, heads;
  int32_t ldq, ldk, ldv, ldo, lddq, lddk, lddv, lddo;
  float scale;
  int32_t accumulate;
  int32_t slab_rows;
};

// BEiT's relative-position bias: one fp32 table [(2 Wh - 1)(2 Ww - 1) + 3][heads] (row pitch ld)
struct AttnBias {
  const float* table;
  int32_t ld, Wh, Ww, R;   // R = (2 Wh - 1)(2 Ww - 1): rows R, R + 1, R + 2 are the three cls entries
};

// The row this lane owns in a grid (ceil(n_owned / 128) [x slabs], heads, B): lane column l32 of wave's
// 32 x 32 results, lane half h, row `row` (tile `tile` of the n_owned queries or keys) of (batch b, head hd);
// ok: the row exists (row0 is a row that may be addressed).
struct Owner {
  int l32, h, hd, b, row, row0;
  bool ok;
  int64_t qtok0, ktok0, stat0;   // the batch's first query / key token; the (batch, head)'s first lse / delta
};
__device__ __forceinline__ Owner owner(const AttnArgs& a, int n_owned, int tile) {
  Owner w;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  w.l32 = lane & 31;
  w.h = lane >> 5;
  w.hd = blockIdx.y;
  w.b = blockIdx.z;
  w.row = tile * kTQ + wave * 32 + w.l32;
  w.ok = w.row < n_owned;
  w.row0 = w.ok ? w.row : 0;
  w.qtok0 = (int64_t)w.b * a.Nq;
  w.ktok0 = (int64_t)w.b * a.Nk;
  w.stat0 = ((int64_t)w.b * a.heads + w.hd) * a.Nq;
  return w;
}

// an accumulator pair (columns d 0..31 and 32..63 of a row this lane owns, transposed) to memory
__device__ __forceinline__ void store_row(float* row, const f32x16& a0, const f32x16& a1, int h, float mul,
                                          int accumulate) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 v0 = f32x4{a0[4 * g], a0[4 * g + 1], a0[4 * g + 2], a0[4 * g + 3]} * mul;
    f32x4 v1 = f32x4{a1[4 * g], a1[4 * g + 1], a1[4 * g + 2], a1[4 * g + 3]} * mul;
    float* p0 = row + 8 * g + 4 * h;
    float* p1 = p0 + 32;
    if (accumulate) {
      v0 += ld4(p0);
      v1 += ld4(p1);
    }
    st4(p0, v0);
    st4(p1, v1);
  }
}

// ---- the relative-position bias -------------------------------------------------------------------------
// The score of (query i, key j) gets table[idx(i, j)][head] added before the softmax.  The head's column of
// the table is staged once in (dynamic) LDS; idx(i, j) for i, j >= 1 is qterm(i) + koff(j), qterm on the lane
// and koff computed once per key tile by 32 threads.
struct BiasLane {
  int qterm, qand, key0;
};

__device__ __forceinline__ BiasLane bias_stage(const AttnBias& rb, float* sTab, const Owner& w) {
  for (int t = threadIdx.x; t < rb.R + 3; t += 256) sTab[t] = rb.table[(int64_t)t * rb.ld + w.hd];
  // the cls query (and a lane past N, whose result is dropped) reads row R whatever the key
  BiasLane bl = {rb.R, 0, rb.R + 2};
  if (w.ok && w.row > 0) {
    const int iy = (w.row - 1) / rb.Ww, ix = (w.row - 1) - iy * rb.Ww;
    bl.qterm = iy * (2 * rb.Ww - 1) + ix;
    bl.qand = -1;
    bl.key0 = rb.R + 1;
  }
  return bl;
}

// koff of the keys of tile k0; key j = 1 + jy Ww + jx: (Wh - 1 - jy)(2 Ww - 1) + (Ww - 1 - jx)
__device__ __forceinline__ void bias_key_offsets(const AttnBias& rb, int* sKoff, int k0, int N) {
  if (threadIdx.x < kTK) {
    const int j = k0 + threadIdx.x;
    int off = 0;             // the cls key (replaced by key0 in scores) and keys past N (score -inf)
    if (j >= 1 && j < N) {
      const int jy = (j - 1) / rb.Ww, jx = (j - 1) - jy * rb.Ww;
      off = (rb.Wh - 1 - jy) * (2 * rb.Ww - 1) + (rb.Ww - 1 - jx);
    }
    sKoff[threadIdx.x] = off;
  }
}

// ---- the softmax ----------------------------------------------------------------------------------------
// s = S^T[key][query] of tile k0 as the MFMA left it -> scale * s (+ bias), -inf for a key past N; returns
// the maximum over the tile's 32 keys
template <bool kBias>
__device__ __forceinline__ float scores(f32x16& s, float scale, int k0, int N, int h, const float* sTab,
                                        const int* sKoff, const BiasLane& bl) {
  float tmax = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float sc = __fmul_rn(s[r], scale);
    if constexpr (kBias) {
      const int kr = acc_row(r, h);
      sc += sTab[k0 + kr == 0 ? bl.key0 : bl.qterm + (sKoff[kr] & bl.qand)];
    }
    s[r] = (k0 + acc_row(r, h) < N) ? sc : -INFINITY;
    tmax = fmaxf(tmax, s[r]);
  }
  return fmaxf(tmax, __shfl_xor(tmax, 32, 64));
}

// the online-softmax step: s -> P^T = exp(s - new maximum) in fp32; the running maximum m, this lane half's
// sum l and the accumulators are rescaled to the new maximum
__device__ __forceinline__ void softmax_step(f32x16& s, float tmax, float& m, float& l, f32x16& o0, f32x16& o1) {
  const float m_new = fmaxf(m, tmax);   // finite: key k0 of every tile exists
  const float alpha = expf(m - m_new);  // 0 at the first tile
  float ps = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    s[r] = expf(s[r] - m_new);          // exactly 0 for a key past N
    ps += s[r];                         // the fp32 value, whatever the next product rounds its operand to
  }
  l = l * alpha + ps;
  o0 *= alpha;
  o1 *= alpha;
  m = m_new;
}

__device__ __forceinline__ void forward_store(const AttnArgs& a, const Owner& w, float* O, float* lse,
                                              const f32x16& o0, const f32x16& o1, float m, float l) {
  l += __shfl_xor(l, 32, 64);
  if (w.ok) {
    store_row(O + (w.qtok0 + w.row) * a.ldo + w.hd * kD, o0, o1, w.h, 1.0f / l, 0);
    if (w.h == 0) lse[w.stat0 + w.row] = m + logf(l);
  }
}

// ---- the kernels: grid (ceil(N / 128), heads, B), 256 threads -------------------------------------------
template <class P, bool kBias>
__global__ __launch_bounds__(256) void attn_forward_kernel(const AttnArgs a, const float* __restrict__ Q,
                                                           const float* __restrict__ K,
                                                           const float* __restrict__ V, float* __restrict__ O,
                                                           float* __restrict__ lse, const AttnBias rb) {
  __shared__ typename P::template Tile<true, false> sK;
  __shared__ typename P::template Tile<false, true> sV;
  __shared__ int sKoff[kBias ? kTK : 1];
  extern __shared__ float sTab[];
  const Owner w = owner(a, a.Nq, blockIdx.x);
  typename P::Row qreg;
  P::load_row(qreg, Q + (w.qtok0 + w.row0) * a.ldq + w.hd * kD, w.ok, w.h, 1.f);
  const float* Kb = K + w.ktok0 * a.ldk + w.hd * kD;
  const float* Vb = V + w.ktok0 * a.ldv + w.hd * kD;
  f32x16 o0 = zero16(), o1 = zero16();
  float m = -INFINITY, l = 0.f;   // l: the sum over this lane half's keys
  BiasLane bl = {};
  if constexpr (kBias) bl = bias_stage(rb, sTab, w);
  typename P::TileLoad tk, tv;
  P::load_tile(tk, Kb, 0, a.Nk, a.ldk);
  P::load_tile(tv, Vb, 0, a.Nk, a.ldv);
  for (int k0 = 0; k0 < a.Nk; k0 += kTK) {
    __syncthreads();
    P::store_tile(sK, tk, 1.f);
    P::store_tile(sV, tv, 1.f);
    P::load_tile(tk, Kb, k0 + kTK, a.Nk, a.ldk);   // the next tile (nothing is read past Nk)
    P::load_tile(tv, Vb, k0 + kTK, a.Nk, a.ldv);
    if constexpr (kBias) bias_key_offsets(rb, sKoff, k0, a.Nk);
    __syncthreads();
    f32x16 s = zero16();   // S^T[key][query]
#pragma unroll
    for (int st = 0; st < P::kSteps1; ++st) s = P::mma1(sK, w.l32, st, qreg, s, w.h);
    const float tmax = scores<kBias>(s, a.scale, k0, a.Nk, w.h, sTab, sKoff, bl);
    softmax_step(s, tmax, m, l, o0, o1);
#pragma unroll
    for (int st = 0; st < P::kSteps2; ++st) {   // O^T[d][query] += V^T[d][key] P^T[key][query]
      const typename P::Frag p = P::frag(s, st);
      o0 = P::mma2(sV, w.l32, st, p, o0, w.h);
      o1 = P::mma2(sV, 32 + w.l32, st, p, o1, w.h);
    }
  }
  forward_store(a, w, O, lse, o0, o1, m, l);
}

// The workgroup owns dK and dV of its 128 keys over one slab of the queries: grid.x = key tiles x slabs
// (blockIdx.x = slab * key tiles + key tile), slab s = queries [s * slab_rows, min(Nq, (s + 1) * slab_rows)).
// One slab: dK / dV are stored (= or +=) as they stand.  Several: slab s stores (=) its partial of the
// image's [Nk][64 * heads] block at dK + s * slab_stride, dV + s * slab_stride (pitches lddk, lddv: the
// caller points them into the workspace), and attn_slab_combine_kernel sums the slabs in slab order.
template <class P>
__global__ __launch_bounds__(256) void attn_backward_dkv_kernel(
    const AttnArgs a, const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    const float* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ delta,
    const typename P::GradMax gm, float* dK, float* dV, const int ktiles, const int64_t slab_stride) {
  __shared__ typename P::template Tile<true, true> sQ;
  __shared__ typename P::template Tile<true, true> sG;
  __shared__ float sL[kTK];
  __shared__ float sD[kTK];
  const int slab = blockIdx.x / ktiles;
  const Owner w = owner(a, a.Nk, blockIdx.x - slab * ktiles);
  const int q_begin = slab * a.slab_rows;
  const int q_end = (int64_t)q_begin + a.slab_rows < a.Nq ? q_begin + a.slab_rows : a.Nq;   // a ragged tile: Nq
  const int e = P::grad_exponent(gm);
  const float gs = pow2f(e);
  typename P::Row kreg, vreg;
  P::load_row(kreg, K + (w.ktok0 + w.row0) * a.ldk + w.hd * kD, w.ok, w.h, 1.f);
  P::load_row(vreg, V + (w.ktok0 + w.row0) * a.ldv + w.hd * kD, w.ok, w.h, 1.f);
  const float* Qb = Q + w.qtok0 * a.ldq + w.hd * kD;
  const float* Gb = dO + w.qtok0 * a.lddo + w.hd * kD;
  const float* Lb = lse + w.stat0;
  const float* Db = delta + w.stat0;
  f32x16 dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
  typename P::TileLoad tq, tg;
  P::load_tile(tq, Qb, q_begin, q_end, a.ldq);
  P::load_tile(tg, Gb, q_begin, q_end, a.lddo);
  for (int q0 = q_begin; q0 < q_end; q0 += kTK) {
    __syncthreads();
    P::store_tile(sQ, tq, 1.f);
    P::store_tile(sG, tg, gs);
    P::load_tile(tq, Qb, q0 + kTK, q_end, a.ldq);   // the next tile (nothing is read past the slab)
    P::load_tile(tg, Gb, q0 + kTK, q_end, a.lddo);
    if (threadIdx.x < kTK) {
      const bool ok = q0 + (int)threadIdx.x < q_end;
      sL[threadIdx.x] = ok ? Lb[q0 + threadIdx.x] : 0.f;
      sD[threadIdx.x] = ok ? Db[q0 + threadIdx.x] * gs : 0.f;
    }
    __syncthreads();
    f32x16 s = zero16(), dp = zero16();   // S[query][key], dP[query][key]
#pragma unroll
    for (int st = 0; st < P::kSteps1; ++st) {
      s = P::mma1(sQ, w.l32, st, kreg, s, w.h);
      dp = P::mma1(sG, w.l32, st, vreg, dp, w.h);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qq = acc_row(r, w.h);
      const float p = (q0 + qq < q_end) ? expf(__fmul_rn(s[r], a.scale) - sL[qq]) : 0.f;
      s[r] = p;
      dp[r] = p * (dp[r] - sD[qq]);
    }
#pragma unroll
    for (int st = 0; st < P::kSteps2; ++st) {   // dV^T[d][key] += dO^T[d][q] P[q][key];  dK^T += Q^T dS
      const typename P::Frag p = P::frag(s, st), ds = P::frag_sat(dp, st);
      dv0 = P::mma2(sG, w.l32, st, p, dv0, w.h);
      dv1 = P::mma2(sG, 32 + w.l32, st, p, dv1, w.h);
      dk0 = P::mma2(sQ, w.l32, st, ds, dk0, w.h);
      dk1 = P::mma2(sQ, 32 + w.l32, st, ds, dk1, w.h);
    }
  }
  if (w.ok) {
    const float inv = pow2f(-e);
    const int64_t at = slab * slab_stride + w.ktok0 + w.row;
    store_row(dK + at * a.lddk + w.hd * kD, dk0, dk1, w.h, a.scale * inv, a.accumulate);
    store_row(dV + at * a.lddv + w.hd * kD, dv0, dv1, w.h, inv, a.accumulate);
  }
}

// the workgroup owns dQ of its 128 queries
template <class P>
__global__ __launch_bounds__(256) void attn_backward_dq_kernel(
    const AttnArgs a, const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    const float* __restrict__ dO, const float* __restrict__ lse, const float* __restrict__ delta,
    const typename P::GradMax gm, float* dQ) {
  __shared__ typename P::template Tile<true, true> sK;
  __shared__ typename P::template Tile<true, false> sV;
  const Owner w = owner(a, a.Nq, blockIdx.x);
  const int e = P::grad_exponent(gm);
  const float gs = pow2f(e);
  typename P::Row qreg, greg;
  P::load_row(qreg, Q + (w.qtok0 + w.row0) * a.ldq + w.hd * kD, w.ok, w.h, 1.f);
  P::load_row(greg, dO + (w.qtok0 + w.row0) * a.lddo + w.hd * kD, w.ok, w.h, gs);
  const float lse_q = w.ok ? lse[w.stat0 + w.row0] : 0.f;
  const float delta_q = w.ok ? delta[w.stat0 + w.row0] * gs : 0.f;
  const float* Kb = K + w.ktok0 * a.ldk + w.hd * kD;
  const float* Vb = V + w.ktok0 * a.ldv + w.hd * kD;
  f32x16 dq0 = zero16(), dq1 = zero16();
  typename P::TileLoad tk, tv;
  P::load_tile(tk, Kb, 0, a.Nk, a.ldk);
  P::load_tile(tv, Vb, 0, a.Nk, a.ldv);
  for (int k0 = 0; k0 < a.Nk; k0 += kTK) {
    __syncthreads();
    P::store_tile(sK, tk, 1.f);
    P::store_tile(sV, tv, 1.f);
    P::load_tile(tk, Kb, k0 + kTK, a.Nk, a.ldk);   // the next tile (nothing is read past Nk)
    P::load_tile(tv, Vb, k0 + kTK, a.Nk, a.ldv);
    __syncthreads();
    f32x16 s = zero16(), dp = zero16();   // S^T[key][query], dP^T[key][query]
#pragma unroll
    for (int st = 0; st < P::kSteps1; ++st) {
      s = P::mma1(sK, w.l32, st, qreg, s, w.h);
      dp = P::mma1(sV, w.l32, st, greg, dp, w.h);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = (k0 + acc_row(r, w.h) < a.Nk) ? expf(__fmul_rn(s[r], a.scale) - lse_q) : 0.f;
      dp[r] = p * (dp[r] - delta_q);
    }
#pragma unroll
    for (int st = 0; st < P::kSteps2; ++st) {   // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
      const typename P::Frag ds = P::frag_sat(dp, st);
      dq0 = P::mma2(sK, w.l32, st, ds, dq0, w.h);
      dq1 = P::mma2(sK, 32 + w.l32, st, ds, dq1, w.h);
    }
  }
  if (w.ok)
    store_row(dQ + (w.qtok0 + w.row) * a.lddq + w.hd * kD, dq0, dq1, w.h, a.scale * pow2f(-e), a.accumulate);
}


// dK / dV = (or +=) the sum over the slabs, in slab order, of the partials the dK / dV kernel left in the
// workspace: part = dK partials [slabs][rows][4 c4] then dV partials in the same shape.  One thread per four
// columns of a key row of dK or dV: a fixed order, no atomics.
__global__ __launch_bounds__(256) void attn_slab_combine_kernel(const float* __restrict__ part, float* dK,
                                                                float* dV, const int64_t rows, const int c4,
                                                                const int slabs, const int lddk, const int lddv,
                                                                const int accumulate) {
  const int64_t per = rows * c4, items = 2 * per;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const bool is_v = it >= per;
    const int64_t at = is_v ? it - per : it;
    const int64_t row = at / c4;
    const int cq = (int)(at - row * c4);
    const float* src = part + (is_v ? (int64_t)slabs * per * 4 : 0) + at * 4;
    f32x4 sum = ld4(src);
    for (int sl = 1; sl < slabs; ++sl) sum += ld4(src + (int64_t)sl * per * 4);
    float* dst = is_v ? dV + row * lddv + cq * 4 : dK + row * lddk + cq * 4;
    if (accumulate) sum += ld4(dst);
    st4(dst, sum);
  }
}

// ---- host side ------------------------------------------------------------------------------------------
// Every entry runs on a gs_attention_kv_desc; the self-attention entries pass theirs through SelfDesc.
struct SelfDesc {
  gs_attention_kv_desc kv;
  const gs_attention_kv_desc* p;
  explicit SelfDesc(const gs_attention_desc* d) : kv(), p(nullptr) {
    if (!d) return;
    kv.B = d->B; kv.Nq = d->N; kv.Nk = d->N; kv.heads = d->heads;
    kv.ldq = d->ldq; kv.ldk = d->ldk; kv.ldv = d->ldv; kv.ldo = d->ldo;
    kv.lddq = d->lddq; kv.lddk = d->lddk; kv.lddv = d->lddv; kv.lddo = d->lddo;
    kv.scale = d->scale;
    p = &kv;
  }
};

int attn_check(const gs_attention_kv_desc* d) {
  if (!d) return GS_E_NULL;
  if (d->B <= 0 || d->Nq <= 0 || d->Nk <= 0 || d->heads <= 0 || !(d->scale > 0.f)) return GS_E_BADARG;
  if (d->B > 65535 || d->heads > 65535 || d->heads > INT32_MAX / kD) return GS_E_BADARG;
  const int32_t ld[8] = {d->ldq, d->ldk, d->ldv, d->ldo, d->lddq, d->lddk, d->lddv, d->lddo};
  for (int i = 0; i < 8; ++i)
    if (ld[i] % 4) return GS_E_ALIGN;
  for (int i = 0; i < 8; ++i)
    if (ld[i] < kD * d->heads) return GS_E_BADARG;
  return GS_OK;
}

// what gs_attention_relpos_forward checks beyond attn_check, before the pointers
int attn_relpos_check(const gs_attention_kv_desc* d, int32_t ld_table, int32_t Wh, int32_t Ww) {
  if (d->Nq != d->Nk) return GS_E_BADARG;
  if (Wh < 1 || Ww < 1 || (int64_t)Wh * Ww + 1 != d->Nq || ld_table < d->heads) return GS_E_BADARG;
  const int64_t R = (2 * (int64_t)Wh - 1) * (2 * (int64_t)Ww - 1);
  return R + 3 > GS_ATTENTION_RELPOS_MAX_ROWS ? GS_E_BADARG : GS_OK;
}

// How the dK / dV kernel splits the queries: `slabs` slabs of slab_rows queries each (a multiple of kTK; the
// last one may be shorter; no slab is empty).
struct AttnSplit {
  int32_t slabs, slab_rows;
};
// the split nearest to `want` slabs that has whole tiles per slab
inline AttnSplit attn_split(const gs_attention_kv_desc* d, int64_t want) {
  const int64_t qtiles = ceil_div(d->Nq, kTK), ktiles = ceil_div(d->Nk, kTQ);
  want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, qtiles), INT32_MAX / ktiles));
  const int64_t per = ceil_div(qtiles, want);
  const int64_t slabs = ceil_div(qtiles, per);
  return AttnSplit{(int32_t)slabs, slabs == 1 ? d->Nq : (int32_t)(per * kTK)};
}
// The planned split of gs_attention_kv_backward, a pure function of the descriptor and the CU count.  The
// dK / dV kernel's 210 VGPRs and 64 AGPRs (two owned rows, four accumulators, two score tiles) leave one wave
// per SIMD, so a CU holds ONE workgroup: the key tiles x heads x B workgroups are multiplied by query slabs
// until they fill one round of those CU places, and not past it -- measured (profiles/r23_segformer.md), the
// whole backward is fastest there at three of the recipe's four stage shapes (40 workgroups of stage 3: S = 4 /
// 6 / 8 / 16 take 224 / 197 / 233 / 212 us) and within the spread between runs of twice as many slabs at
// the fourth, where it halves the workspace.  No slab gets fewer than kMinSlabTiles query tiles: a slab's partial pair of [128][64] dK /
// dV blocks, stored and read again by the combine, is as many bytes as four query tiles of Q and dO.
constexpr int kMinSlabTiles = 4;
inline AttnSplit attn_split_plan(const gs_attention_kv_desc* d) {
  const int64_t wgs = ceil_div(d->Nk, kTQ) * d->heads * d->B;
  const int64_t by_places = (int64_t)num_cu() / wgs;
  const int64_t by_work = ceil_div(d->Nq, kTK) / kMinSlabTiles;
  return attn_split(d, std::min(by_places, by_work));
}

AttnArgs attn_args(const gs_attention_kv_desc* d, int accumulate) {
  AttnArgs a;
  a.B = d->B; a.Nq = d->Nq; a.Nk = d->Nk; a.heads = d->heads;
  a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv; a.ldo = d->ldo;
  a.lddq = d->lddq; a.lddk = d->lddk; a.lddv = d->lddv; a.lddo = d->lddo;
  a.scale = d->scale;
  a.accumulate = accumulate ? 1 : 0;
  a.slab_rows = d->Nq;
  return a;
}

// workgroups that own 128 queries each: the forward, dQ and the fp16 delta pre-pass
inline int64_t attn_tiles(const gs_attention_kv_desc* d) { return ceil_div(d->Nq, kTQ); }
inline dim3 attn_grid(const gs_attention_kv_desc* d) {
  return dim3((unsigned)attn_tiles(d), (unsigned)d->heads, (unsigned)d->B);
}

// the backward's workspace: what the policy's pre-pass leaves (delta first), then the slabs' partials
// [2][slabs][B * Nk][64 * heads] when there is more than one slab
template <class P>
size_t attn_ws_bytes(const gs_attention_kv_desc* d, const AttnSplit& sp) {
  const size_t part = (size_t)2 * sp.slabs * d->B * d->Nk * kD * d->heads * sizeof(float);
  return P::ws_bytes(d) + (sp.slabs > 1 ? part : 0);
}

// Errors are reported in this order: descriptor, relpos arguments, NULL, alignment, workspace.
template <class P>
size_t attn_workspace_bytes(const gs_attention_kv_desc* d, int64_t want_slabs) {
  if (attn_check(d) != GS_OK) return 0;
  return attn_ws_bytes<P>(d, want_slabs > 0 ? attn_split(d, want_slabs) : attn_split_plan(d));
}

template <class P>
int attn_forward(const gs_attention_kv_desc* d, const float* q, const float* k, const float* v, float* o,
                 float* lse, void* stream) {
  const int rc = attn_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({q, k, v, o, lse})) return GS_E_NULL;
  if (!all_aligned16({q, k, v, o, lse})) return GS_E_ALIGN;
  hipLaunchKernelGGL((attn_forward_kernel<P, false>), attn_grid(d), dim3(256), 0, as_stream(stream),
                     attn_args(d, 0), q, k, v, o, lse, AttnBias{nullptr, 0, 0, 0, 0});
  return launch_status();
}

template <class P>
int attn_relpos_forward(const gs_attention_kv_desc* d, const float* q, const float* k, const float* v,
                        const float* table, int32_t ld_table, int32_t Wh, int32_t Ww, float* o, float* lse,
                        void* stream) {
  int rc = attn_check(d);
  if (rc == GS_OK) rc = attn_relpos_check(d, ld_table, Wh, Ww);
  if (rc != GS_OK) return rc;
  if (any_null({q, k, v, table, o, lse})) return GS_E_NULL;
  if (!all_aligned16({q, k, v, o, lse}) || (reinterpret_cast<uintptr_t>(table) & 3u)) return GS_E_ALIGN;
  const int64_t R = (2 * (int64_t)Wh - 1) * (2 * (int64_t)Ww - 1);
  const AttnBias rb = {table, ld_table, Wh, Ww, (int32_t)R};
  const size_t lds = (size_t)ceil_div((R + 3) * (int64_t)sizeof(float), 16) * 16;
  hipLaunchKernelGGL((attn_forward_kernel<P, true>), attn_grid(d), dim3(256), lds, as_stream(stream),
                     attn_args(d, 0), q, k, v, o, lse, rb);
  return launch_status();
}

// want_slabs: the query split of the dK / dV kernel -- 1 for the self-attention entries (one slab, stored
// directly), <= 0 for the plan
template <class P>
int attn_backward(const gs_attention_kv_desc* d, const float* q, const float* k, const float* v, const float* o,
                  const float* lse, const float* d_o, float* dq, float* dk, float* dv, int accumulate,
                  void* workspace, size_t workspace_bytes, int64_t want_slabs, void* stream) {
  const int rc = attn_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({q, k, v, o, lse, d_o, dq, dk, dv, workspace})) return GS_E_NULL;
  if (!all_aligned16({q, k, v, o, lse, d_o, dq, dk, dv, workspace})) return GS_E_ALIGN;
  const AttnSplit sp = want_slabs > 0 ? attn_split(d, want_slabs) : attn_split_plan(d);
  if (workspace_bytes < attn_ws_bytes<P>(d, sp)) return GS_E_WORKSPACE;
  const AttnArgs a = attn_args(d, accumulate);
  float* delta = static_cast<float*>(workspace);
  const typename P::GradMax gm = P::launch_delta(d, a, d_o, o, delta, as_stream(stream));
  const int ktiles = (int)ceil_div(d->Nk, kTQ);
  const dim3 kgrid((unsigned)(ktiles * sp.slabs), (unsigned)d->heads, (unsigned)d->B);
  if (sp.slabs == 1) {
    hipLaunchKernelGGL(attn_backward_dkv_kernel<P>, kgrid, dim3(256), 0, as_stream(stream), a, q, k, v, d_o, lse,
                       delta, gm, dk, dv, ktiles, (int64_t)0);
  } else {
    AttnArgs ap = a;   // the partials: packed rows, plain stores
    ap.slab_rows = sp.slab_rows;
    ap.lddk = ap.lddv = kD * d->heads;
    ap.accumulate = 0;
    const int64_t rows = (int64_t)d->B * d->Nk;
    float* part = reinterpret_cast<float*>(static_cast<char*>(workspace) + P::ws_bytes(d));
    hipLaunchKernelGGL(attn_backward_dkv_kernel<P>, kgrid, dim3(256), 0, as_stream(stream), ap, q, k, v, d_o,
                       lse, delta, gm, part, part + (int64_t)sp.slabs * rows * ap.lddk, ktiles, rows);
    hipLaunchKernelGGL(attn_slab_combine_kernel, dim3(stream_grid(2 * rows * (ap.lddk / 4), 256)), dim3(256), 0,
                       as_stream(stream), part, dk, dv, rows, ap.lddk / 4, (int)sp.slabs, (int)d->lddk,
                       (int)d->lddv, a.accumulate);
  }
  hipLaunchKernelGGL(attn_backward_dq_kernel<P>, attn_grid(d), dim3(256), 0, as_stream(stream), a, q, k, v,
                     d_o, lse, delta, gm, dq);
  return launch_status();
}

}  // namespace
}  // namespace gs
