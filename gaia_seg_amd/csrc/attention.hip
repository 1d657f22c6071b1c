// The fp32-operand attention entries (gs_attention_* in include/gaiaseg_hip.h): the operand policy of the
// exact fp32 MFMA for the kernels of attention_common.h -- which describes the kernels, the operand maps and
// the LDS image -- and the fp32 delta pre-pass.  Also the ViT token assembly (gs_vit_tokens_*).
#include "attention_common.h"

namespace gs {
namespace {

// delta[b,h,i] = sum_d dO * O as the d-ordered fma chain: one thread per (token, head)
__global__ __launch_bounds__(256) void attn_delta_kernel(const AttnArgs a, const float* __restrict__ dO,
                                                         const float* __restrict__ O,
                                                         float* __restrict__ delta) {
  const int64_t items = (int64_t)a.B * a.Nq * a.heads;
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
    delta[((tok / a.Nq) * a.heads + hd) * a.Nq + tok % a.Nq] = acc;
  }
}

struct F32Ops {
  static constexpr int kPitch = 66;    // floats per LDS tile row
  static constexpr int kSteps1 = 32;   // MFMAs (k = 2) of a 64-deep first product
  static constexpr int kSteps2 = 16;   // MFMAs of a 32-deep second product (two lane halves)

  static __device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
  }

  // reg[s] = row[2 s + h]
  struct Row {
    float reg[32];
  };
  // this lane's operand registers of a row it owns, times mul; zeros for a row past the end
  static __device__ __forceinline__ void load_row(Row& r, const float* row, bool ok, int h, float mul) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok) v = ld4(row + c * 4) * mul;
      r.reg[2 * c] = h ? v.y : v.x;
      r.reg[2 * c + 1] = h ? v.w : v.z;
    }
  }

  // one image, read by rows and by columns
  template <bool kRows, bool kCols>
  struct Tile {
    float v[kTK * kPitch];
  };
  // what store_tile copies: rows [row0, row0 + 32) of one (batch, head) block `src` (pitch ld)
  struct TileLoad {
    const float* src;
    int row0, N, ld;
  };
  static __device__ __forceinline__ void load_tile(TileLoad& t, const float* src, int row0, int N, int ld) {
    t = TileLoad{src, row0, N, ld};
  }
  // the tile times mul from memory into the image; rows >= N are 0 and are not read
  template <bool kRows, bool kCols>
  static __device__ __forceinline__ void store_tile(Tile<kRows, kCols>& tile, const TileLoad& t, float mul) {
    for (int idx = threadIdx.x; idx < kTK * (kD / 4); idx += 256) {
      const int row = idx >> 4, c4 = idx & 15;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t.row0 + row < t.N) v = ld4(t.src + (int64_t)(t.row0 + row) * t.ld + c4 * 4) * mul;
      float* d = tile.v + row * kPitch + c4 * 4;   // 8-byte aligned at an even pitch
      *reinterpret_cast<float2*>(d) = float2{v.x, v.y};
      *reinterpret_cast<float2*>(d + 2) = float2{v.z, v.w};
    }
  }

  // k-step st of (tile row `row`) x (owned row)
  template <bool kCols>
  static __device__ __forceinline__ f32x16 mma1(const Tile<true, kCols>& t, int row, int st, const Row& r,
                                                f32x16 acc, int h) {
    return mfma(t.v[row * kPitch + 2 * st + h], r.reg[st], acc);
  }
  // k-step st of (tile column d) x (accumulator): the accumulator's register st is the B operand as it is
  typedef float Frag;
  static __device__ __forceinline__ Frag frag(const f32x16& x, int st) { return x[st]; }
  static __device__ __forceinline__ Frag frag_sat(const f32x16& x, int st) { return x[st]; }
  template <bool kRows>
  static __device__ __forceinline__ f32x16 mma2(const Tile<kRows, true>& t, int d, int st, Frag b, f32x16 acc,
                                                int h) {
    return mfma(t.v[acc_row(st, h) * kPitch + d], b, acc);
  }

  // no gradient scale: 2^0
  struct GradMax {};
  static __device__ __forceinline__ int grad_exponent(const GradMax&) { return 0; }

  // delta[B][heads][N]
  static size_t ws_bytes(const gs_attention_kv_desc* d) {
    return (size_t)ceil_div((int64_t)d->B * d->heads * d->Nq * (int64_t)sizeof(float), 16) * 16;
  }
  static GradMax launch_delta(const gs_attention_kv_desc* d, const AttnArgs& a, const float* d_o, const float* o,
                              float* delta, hipStream_t stream) {
    hipLaunchKernelGGL(attn_delta_kernel, dim3(stream_grid((int64_t)d->B * d->Nq * d->heads, 256)), dim3(256), 0,
                       stream, a, d_o, o, delta);
    return GradMax{};
  }
};

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
  return attn_workspace_bytes<F32Ops>(SelfDesc(d).p, 1);
}

extern "C" int gs_attention_forward(const gs_attention_desc* d, const float* q, const float* k, const float* v,
                                    float* o, float* lse, void* stream) {
  return attn_forward<F32Ops>(SelfDesc(d).p, q, k, v, o, lse, stream);
}

extern "C" int gs_attention_relpos_forward(const gs_attention_desc* d, const float* q, const float* k,
                                           const float* v, const float* table, int32_t ld_table, int32_t Wh,
                                           int32_t Ww, float* o, float* lse, void* stream) {
  return attn_relpos_forward<F32Ops>(SelfDesc(d).p, q, k, v, table, ld_table, Wh, Ww, o, lse, stream);
}

extern "C" int gs_attention_backward(const gs_attention_desc* d, const float* q, const float* k,
                                     const float* v, const float* o, const float* lse, const float* d_o,
                                     float* dq, float* dk, float* dv, int accumulate, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return attn_backward<F32Ops>(SelfDesc(d).p, q, k, v, o, lse, d_o, dq, dk, dv, accumulate, workspace,
                               workspace_bytes, 1, stream);
}

// gs_debug_set_attention_kv_split: >= 1 forces that query split on gs_attention_kv_*, -1 is the plan
static int g_kv_split = -1;

extern "C" int gs_debug_set_attention_kv_split(int32_t S) {
  if (S != -1 && S < 1) return GS_E_BADARG;
  g_kv_split = S;
  return GS_OK;
}

extern "C" size_t gs_attention_kv_workspace_bytes(const gs_attention_kv_desc* d) {
  return attn_workspace_bytes<F32Ops>(d, g_kv_split);
}

extern "C" int gs_attention_kv_forward(const gs_attention_kv_desc* d, const float* q, const float* k,
                                       const float* v, float* o, float* lse, void* stream) {
  return attn_forward<F32Ops>(d, q, k, v, o, lse, stream);
}

extern "C" int gs_attention_kv_backward(const gs_attention_kv_desc* d, const float* q, const float* k,
                                        const float* v, const float* o, const float* lse, const float* d_o,
                                        float* dq, float* dk, float* dv, int accumulate, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return attn_backward<F32Ops>(d, q, k, v, o, lse, d_o, dq, dk, dv, accumulate, workspace, workspace_bytes,
                               g_kv_split, stream);
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
