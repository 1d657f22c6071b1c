// Multi-head softmax self-attention (head dimension 64) on fp32 "rows x C" token views, forward and
// backward, and the ViT token assembly (include/gaiaseg_hip.h).
//
// Every matrix product runs on the exact fp32 MFMA v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain),
// so the operator is fp32-accurate in every precision mode.  No N x N matrix is stored, no float atomics
// are used and every sum has a fixed order: results are bit-identical from run to run.
//
// MFMA operand maps (lane l, i = l & 31, h = l >> 5): A[i][k = h], B[k = h][j = i]; the 32x32 result has
// its COLUMN on the lane and row (r & 3) + 8 (r >> 2) + 4 h in register r (acc_row below).  Each product
// is oriented so that the index the NEXT product sums over is the result's row index: a result register
// is then the next MFMA's B operand as it stands, and everything that belongs to the column (a query's
// running maximum, sum, lse and delta; a key's dK / dV) lives on the lane.
//
//   forward  : a workgroup = 4 waves = kTQ = 128 queries of one (batch, head), 32 per wave, Q in registers.
//              Key tiles of kTK = 32 rows of K and V go through LDS.  S^T = K Q^T puts the query on the
//              lane: the row maximum and sum are 16 register steps and one exchange between the lane
//              halves.  O^T += V^T P^T keeps the query on the lane, so the online rescale is per lane.
//              A key past N gets the score -inf, hence p = exp(-inf) = 0 exactly.
//   relpos   : the same kernel with BEiT's relative-position bias added to the scaled score (template
//              parameter; the bias-free instantiation is the code above, unchanged).  The N x N bias is
//              never formed: the head's column of the table (at most 8192 floats) is staged in LDS once
//              per workgroup and gathered per score.  Lanes of a half wave hold consecutive queries, so
//              their table rows are consecutive except where the window row wraps: few bank conflicts,
//              and no gather traffic beside the K / V stream in L2.  Forward only.
//   backward : delta[b,h,i] = <dO, O> by a pre-pass, as the same d-ordered fma chain the MFMA forms (a
//              single token gives dP == delta bit for bit, so dQ = dK = 0 exactly).  Then two kernels:
//              dK / dV : a workgroup owns 128 keys (32 per wave, K and V in registers) and sweeps query
//                        tiles of 32 (Q, dO, lse, delta in LDS): S = Q K^T and dP = dO V^T have the key
//                        on the lane, dV^T += dO^T P and dK^T += Q^T dS take them as B operands.
//              dQ      : a workgroup owns 128 queries (Q, dO in registers) and sweeps key tiles of 32:
//                        S^T and dP^T as in the forward, dQ^T += K^T dS^T.
//              Seven products instead of five, and no sum across workgroups.
//   LDS image: a tile is 32 rows x 64 floats at a pitch of 66 floats; it is read by rows ([lane row][2 s
//              + h], conflict free at that pitch) for the first products and by columns ([acc_row][lane
//              column]) for the second ones.
#include <math.h>

#include "attention_common.h"

namespace gs {
namespace {

constexpr int kPitch = 66;    // floats per LDS tile row

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// rows [row0, row0 + 32) of one (batch, head) block `src` (pitch ld) into an LDS tile; rows >= N are 0
__device__ __forceinline__ void stage_tile(float* tile, const float* src, int row0, int N, int ld) {
  for (int idx = threadIdx.x; idx < kTK * (kD / 4); idx += 256) {
    const int row = idx >> 4, c4 = idx & 15;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row0 + row < N) v = ld4(src + (int64_t)(row0 + row) * ld + c4 * 4);
    float* d = tile + row * kPitch + c4 * 4;   // 8-byte aligned at an even pitch
    *reinterpret_cast<float2*>(d) = float2{v.x, v.y};
    *reinterpret_cast<float2*>(d + 2) = float2{v.z, v.w};
  }
}

// this lane's operand registers of a row it owns: reg[s] = row[2 s + h]; zeros for a row past the end
__device__ __forceinline__ void load_row_regs(float (&reg)[32], const float* row, bool ok, int h) {
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ok) v = ld4(row + c * 4);
    reg[2 * c] = h ? v.y : v.x;
    reg[2 * c + 1] = h ? v.w : v.z;
  }
}

// grid (ceil(N / 128), heads, B).  kBias: the score of (query i, key j) gets table[idx(i, j)][head] added
// before the softmax.  The head's column of the table is staged once in (dynamic) LDS; idx(i, j) for
// i, j >= 1 is qterm(i) + koff(j), qterm on the lane and koff computed once per key tile by 32 threads.
template <bool kBias>
__global__ __launch_bounds__(256) void attn_forward_kernel(const AttnArgs a, const float* __restrict__ Q,
                                                           const float* __restrict__ K,
                                                           const float* __restrict__ V, float* __restrict__ O,
                                                           float* __restrict__ lse, const AttnBias rb) {
  __shared__ float sK[kTK * kPitch];
  __shared__ float sV[kTK * kPitch];
  __shared__ int sKoff[kBias ? kTK : 1];
  extern __shared__ float sTab[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ql = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * kTQ + wave * 32 + ql;
  const bool qok = q < a.N;
  const int64_t tok0 = (int64_t)b * a.N;
  float qreg[32];
  load_row_regs(qreg, Q + (tok0 + (qok ? q : 0)) * a.ldq + hd * kD, qok, h);
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
  for (int k0 = 0; k0 < a.N; k0 += kTK) {
    __syncthreads();
    stage_tile(sK, Kb, k0, a.N, a.ldk);
    stage_tile(sV, Vb, k0, a.N, a.ldv);
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
    for (int st = 0; st < 32; ++st) s = mfma(sK[ql * kPitch + 2 * st + h], qreg[st], s);
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
      ps += s[r];
    }
    l = l * alpha + ps;
    o0 *= alpha;
    o1 *= alpha;
#pragma unroll
    for (int r = 0; r < 16; ++r) {        // O^T[d][query] += V^T[d][key] P^T[key][query]
      const float* vr = sV + acc_row(r, h) * kPitch + ql;
      o0 = mfma(vr[0], s[r], o0);
      o1 = mfma(vr[32], s[r], o1);
    }
    m = m_new;
  }
  l += __shfl_xor(l, 32, 64);
  if (qok) {
    store_row(O + (tok0 + q) * a.ldo + hd * kD, o0, o1, h, 1.0f / l, 0);
    if (h == 0) lse[((int64_t)b * a.heads + hd) * a.N + q] = m + logf(l);
  }
}

// delta[b,h,i] = sum_d dO * O as the d-ordered fma chain: one thread per (token, head)
__global__ __launch_bounds__(256) void attn_delta_kernel(const AttnArgs a, const float* __restrict__ dO,
                                                         const float* __restrict__ O,
                                                         float* __restrict__ delta) {
  const int64_t items = (int64_t)a.B * a.N * a.heads;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int hd = (int)(it % a.heads);
    const int64_t tok = it / a.heads;
    const float* g = dO + tok * a.lddo + hd * kD;
    const float* o = O + tok * a.ldo + hd * kD;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      const f32x4 x = ld4(g + c * 4), y = ld4(o + c * 4);
      acc = fmaf(x.x, y.x, acc);
      acc = fmaf(x.y, y.y, acc);
      acc = fmaf(x.z, y.z, acc);
      acc = fmaf(x.w, y.w, acc);
    }
    delta[((tok / a.N) * a.heads + hd) * a.N + tok % a.N] = acc;
  }
}

// grid (ceil(N / 128), heads, B): the workgroup owns dK and dV of its 128 keys
__global__ __launch_bounds__(256) void attn_backward_dkv_kernel(const AttnArgs a, const float* __restrict__ Q,
                                                                const float* __restrict__ K,
                                                                const float* __restrict__ V,
                                                                const float* __restrict__ dO,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ delta, float* dK,
                                                                float* dV) {
  __shared__ float sQ[kTK * kPitch];
  __shared__ float sG[kTK * kPitch];
  __shared__ float sL[kTK];
  __shared__ float sD[kTK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kl = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int key = blockIdx.x * kTQ + wave * 32 + kl;
  const bool kok = key < a.N;
  const int64_t tok0 = (int64_t)b * a.N;
  float kreg[32], vreg[32];
  load_row_regs(kreg, K + (tok0 + (kok ? key : 0)) * a.ldk + hd * kD, kok, h);
  load_row_regs(vreg, V + (tok0 + (kok ? key : 0)) * a.ldv + hd * kD, kok, h);
  const float* Qb = Q + tok0 * a.ldq + hd * kD;
  const float* Gb = dO + tok0 * a.lddo + hd * kD;
  const float* Lb = lse + ((int64_t)b * a.heads + hd) * a.N;
  const float* Db = delta + ((int64_t)b * a.heads + hd) * a.N;
  f32x16 dk0 = zero16(), dk1 = zero16(), dv0 = zero16(), dv1 = zero16();
  for (int q0 = 0; q0 < a.N; q0 += kTK) {
    __syncthreads();
    stage_tile(sQ, Qb, q0, a.N, a.ldq);
    stage_tile(sG, Gb, q0, a.N, a.lddo);
    if (threadIdx.x < kTK) {
      const bool ok = q0 + (int)threadIdx.x < a.N;
      sL[threadIdx.x] = ok ? Lb[q0 + threadIdx.x] : 0.f;
      sD[threadIdx.x] = ok ? Db[q0 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    f32x16 s = zero16(), dp = zero16();   // S[query][key], dP[query][key]
#pragma unroll
    for (int st = 0; st < 32; ++st) {
      s = mfma(sQ[kl * kPitch + 2 * st + h], kreg[st], s);
      dp = mfma(sG[kl * kPitch + 2 * st + h], vreg[st], dp);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qq = acc_row(r, h);
      const float p = (q0 + qq < a.N) ? expf(__fmul_rn(s[r], a.scale) - sL[qq]) : 0.f;
      s[r] = p;
      dp[r] = p * (dp[r] - sD[qq]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {        // dV^T[d][key] += dO^T[d][q] P[q][key];  dK^T += Q^T dS
      const int qq = acc_row(r, h);
      const float* gr = sG + qq * kPitch + kl;
      const float* qr = sQ + qq * kPitch + kl;
      dv0 = mfma(gr[0], s[r], dv0);
      dv1 = mfma(gr[32], s[r], dv1);
      dk0 = mfma(qr[0], dp[r], dk0);
      dk1 = mfma(qr[32], dp[r], dk1);
    }
  }
  if (kok) {
    store_row(dK + (tok0 + key) * a.lddk + hd * kD, dk0, dk1, h, a.scale, a.accumulate);
    store_row(dV + (tok0 + key) * a.lddv + hd * kD, dv0, dv1, h, 1.0f, a.accumulate);
  }
}

// grid (ceil(N / 128), heads, B): the workgroup owns dQ of its 128 queries
__global__ __launch_bounds__(256) void attn_backward_dq_kernel(const AttnArgs a, const float* __restrict__ Q,
                                                               const float* __restrict__ K,
                                                               const float* __restrict__ V,
                                                               const float* __restrict__ dO,
                                                               const float* __restrict__ lse,
                                                               const float* __restrict__ delta, float* dQ) {
  __shared__ float sK[kTK * kPitch];
  __shared__ float sV[kTK * kPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ql = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y, b = blockIdx.z;
  const int q = blockIdx.x * kTQ + wave * 32 + ql;
  const bool qok = q < a.N;
  const int64_t tok0 = (int64_t)b * a.N;
  float qreg[32], greg[32];
  load_row_regs(qreg, Q + (tok0 + (qok ? q : 0)) * a.ldq + hd * kD, qok, h);
  load_row_regs(greg, dO + (tok0 + (qok ? q : 0)) * a.lddo + hd * kD, qok, h);
  const int64_t stat = ((int64_t)b * a.heads + hd) * a.N + (qok ? q : 0);
  const float lse_q = qok ? lse[stat] : 0.f, delta_q = qok ? delta[stat] : 0.f;
  const float* Kb = K + tok0 * a.ldk + hd * kD;
  const float* Vb = V + tok0 * a.ldv + hd * kD;
  f32x16 dq0 = zero16(), dq1 = zero16();
  for (int k0 = 0; k0 < a.N; k0 += kTK) {
    __syncthreads();
    stage_tile(sK, Kb, k0, a.N, a.ldk);
    stage_tile(sV, Vb, k0, a.N, a.ldv);
    __syncthreads();
    f32x16 s = zero16(), dp = zero16();   // S^T[key][query], dP^T[key][query]
#pragma unroll
    for (int st = 0; st < 32; ++st) {
      s = mfma(sK[ql * kPitch + 2 * st + h], qreg[st], s);
      dp = mfma(sV[ql * kPitch + 2 * st + h], greg[st], dp);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = (k0 + acc_row(r, h) < a.N) ? expf(__fmul_rn(s[r], a.scale) - lse_q) : 0.f;
      dp[r] = p * (dp[r] - delta_q);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {        // dQ^T[d][query] += K^T[d][key] dS^T[key][query]
      const float* kr = sK + acc_row(r, h) * kPitch + ql;
      dq0 = mfma(kr[0], dp[r], dq0);
      dq1 = mfma(kr[32], dp[r], dq1);
    }
  }
  if (qok) store_row(dQ + (tok0 + q) * a.lddq + hd * kD, dq0, dq1, h, a.scale, a.accumulate);
}

// x[b,0,:D] = cls + pos[0];  x[b,1+t,:D] = patch[b,t] + pos[1+t]
__global__ __launch_bounds__(256) void vit_tokens_forward_kernel(const float* __restrict__ patches,
                                                                 const float* __restrict__ cls,
                                                                 const float* __restrict__ pos,
                                                                 float* __restrict__ x, const int64_t items,
                                                                 const int T, const int D4, const int ldp,
                                                                 const int ldpos, const int ldx) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % D4);
    const int64_t tok = it / D4;
    const int n = (int)(tok % (T + 1));
    const int64_t b = tok / (T + 1);
    const f32x4 v = n == 0 ? ld4(cls + cq * 4) : ld4(patches + (b * T + n - 1) * ldp + cq * 4);
    st4(x + tok * ldx + cq * 4, v + ld4(pos + (int64_t)n * ldpos + cq * 4));
  }
}

// dpatch[b,t] = dx[b,1+t];  dpos[n] = sum_b dx[b,n] in the order of b;  dcls = the same sum of row 0
__global__ __launch_bounds__(256) void vit_tokens_backward_kernel(const float* __restrict__ dx,
                                                                  float* __restrict__ dpatch,
                                                                  float* __restrict__ dcls,
                                                                  float* __restrict__ dpos, const int64_t items,
                                                                  const int B, const int T, const int D4,
                                                                  const int lddx, const int lddp,
                                                                  const int ldpos) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % D4);
    const int n = (int)(it / D4);
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int b = 0; b < B; ++b) {
      const f32x4 g = ld4(dx + ((int64_t)b * (T + 1) + n) * lddx + cq * 4);
      if (n > 0) st4(dpatch + ((int64_t)b * T + n - 1) * lddp + cq * 4, g);
      s += g;
    }
    st4(dpos + (int64_t)n * ldpos + cq * 4, s);
    if (n == 0) st4(dcls + cq * 4, s);
  }
}

inline size_t attn_ws_bytes(const gs_attention_desc* d) {
  return (size_t)ceil_div((int64_t)d->B * d->heads * d->N * (int64_t)sizeof(float), 16) * 16;
}

int tokens_check(int32_t B, int32_t T, int32_t D, const int32_t* ld, int n_ld) {
  if (B <= 0 || T <= 0 || D <= 0) return GS_E_BADARG;
  if (D % 4) return GS_E_ALIGN;
  for (int i = 0; i < n_ld; ++i)
    if (ld[i] % 4) return GS_E_ALIGN;
  for (int i = 0; i < n_ld; ++i)
    if (ld[i] < D) return GS_E_BADARG;
  return GS_OK;
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_attention_workspace_bytes(const gs_attention_desc* d) {
  return attn_check(d) == GS_OK ? attn_ws_bytes(d) : 0;
}

extern "C" int gs_attention_forward(const gs_attention_desc* d, const float* q, const float* k, const float* v,
                                    float* o, float* lse, void* stream) {
  const int rc = attn_check(d);
  if (rc != GS_OK) return rc;
  if (!q || !k || !v || !o || !lse) return GS_E_NULL;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse)) return GS_E_ALIGN;
  const AttnArgs a = attn_args(d, 0);
  const dim3 grid((unsigned)ceil_div(d->N, kTQ), (unsigned)d->heads, (unsigned)d->B);
  hipLaunchKernelGGL(attn_forward_kernel<false>, grid, dim3(256), 0, as_stream(stream), a, q, k, v, o, lse,
                     AttnBias{nullptr, 0, 0, 0, 0});
  return launch_status();
}

extern "C" int gs_attention_relpos_forward(const gs_attention_desc* d, const float* q, const float* k,
                                           const float* v, const float* table, int32_t ld_table, int32_t Wh,
                                           int32_t Ww, float* o, float* lse, void* stream) {
  const int rc = attn_check(d);
  if (rc != GS_OK) return rc;
  const int rb_rc = attn_relpos_check(d, ld_table, Wh, Ww);
  if (rb_rc != GS_OK) return rb_rc;
  const int64_t R = (2 * (int64_t)Wh - 1) * (2 * (int64_t)Ww - 1);
  if (!q || !k || !v || !table || !o || !lse) return GS_E_NULL;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse) ||
      (reinterpret_cast<uintptr_t>(table) & 3u))
    return GS_E_ALIGN;
  const AttnArgs a = attn_args(d, 0);
  const AttnBias rb = {table, ld_table, Wh, Ww, (int32_t)R};
  const dim3 grid((unsigned)ceil_div(d->N, kTQ), (unsigned)d->heads, (unsigned)d->B);
  const size_t lds = (size_t)ceil_div((R + 3) * (int64_t)sizeof(float), 16) * 16;
  hipLaunchKernelGGL(attn_forward_kernel<true>, grid, dim3(256), lds, as_stream(stream), a, q, k, v, o, lse, rb);
  return launch_status();
}

extern "C" int gs_attention_backward(const gs_attention_desc* d, const float* q, const float* k,
                                     const float* v, const float* o, const float* lse, const float* d_o,
                                     float* dq, float* dk, float* dv, int accumulate, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  const int rc = attn_check(d);
  if (rc != GS_OK) return rc;
  if (!q || !k || !v || !o || !lse || !d_o || !dq || !dk || !dv || !workspace) return GS_E_NULL;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(o) || !aligned16(lse) ||
      !aligned16(d_o) || !aligned16(dq) || !aligned16(dk) || !aligned16(dv) || !aligned16(workspace))
    return GS_E_ALIGN;
  if (workspace_bytes < attn_ws_bytes(d)) return GS_E_WORKSPACE;
  const AttnArgs a = attn_args(d, accumulate);
  float* delta = static_cast<float*>(workspace);
  const dim3 grid((unsigned)ceil_div(d->N, kTQ), (unsigned)d->heads, (unsigned)d->B);
  hipLaunchKernelGGL(attn_delta_kernel, dim3(stream_grid((int64_t)d->B * d->N * d->heads, 256)), dim3(256), 0,
                     as_stream(stream), a, d_o, o, delta);
  hipLaunchKernelGGL(attn_backward_dkv_kernel, grid, dim3(256), 0, as_stream(stream), a, q, k, v, d_o, lse,
                     delta, dk, dv);
  hipLaunchKernelGGL(attn_backward_dq_kernel, grid, dim3(256), 0, as_stream(stream), a, q, k, v, d_o, lse,
                     delta, dq);
  return launch_status();
}

extern "C" int gs_vit_tokens_forward(const float* patches, int32_t ldp, const float* cls_token,
                                     const float* pos_embed, int32_t ldpos, float* x, int32_t ldx, int32_t B,
                                     int32_t T, int32_t D, void* stream) {
  const int32_t ld[3] = {ldp, ldpos, ldx};
  const int rc = tokens_check(B, T, D, ld, 3);
  if (rc != GS_OK) return rc;
  if (!patches || !cls_token || !pos_embed || !x) return GS_E_NULL;
  if (!aligned16(patches) || !aligned16(cls_token) || !aligned16(pos_embed) || !aligned16(x)) return GS_E_ALIGN;
  const int64_t items = (int64_t)B * (T + 1) * (D / 4);
  hipLaunchKernelGGL(vit_tokens_forward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream),
                     patches, cls_token, pos_embed, x, items, T, D / 4, ldp, ldpos, ldx);
  return launch_status();
}

extern "C" int gs_vit_tokens_backward(const float* dx, int32_t lddx, float* dpatches, int32_t lddp,
                                      float* dcls_token, float* dpos_embed, int32_t ldpos, int32_t B, int32_t T,
                                      int32_t D, void* stream) {
  const int32_t ld[3] = {lddx, lddp, ldpos};
  const int rc = tokens_check(B, T, D, ld, 3);
  if (rc != GS_OK) return rc;
  if (!dx || !dpatches || !dcls_token || !dpos_embed) return GS_E_NULL;
  if (!aligned16(dx) || !aligned16(dpatches) || !aligned16(dcls_token) || !aligned16(dpos_embed))
    return GS_E_ALIGN;
  const int64_t items = (int64_t)(T + 1) * (D / 4);
  hipLaunchKernelGGL(vit_tokens_backward_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream),
                     dx, dpatches, dcls_token, dpos_embed, items, B, T, D / 4, lddx, lddp, ldpos);
  return launch_status();
}
