// The opt-in fp16-operand attention entries (gs_attention_*_f16 in include/gaiaseg_hip.h): the operand
// policy of v_mfma_f32_32x32x16_f16 for the kernels of attention_common.h -- which describes the kernels,
// the operand maps, the two LDS images, the rounding points and the gradient scale -- and the delta pre-pass
// that also finds max|dO|.
#include "attention_common.h"

namespace gs {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// grid (ceil(N / 128), heads, B): delta[b,h,i] = <dO, O> of the workgroup's 128 tokens (two threads per
// token, 32 columns each, summed in a fixed order) and gmax[workgroup] = max|dO| over them
__global__ __launch_bounds__(256) void attn_delta_f16_kernel(const AttnArgs a, const float* __restrict__ dO,
                                                             const float* __restrict__ O,
                                                             float* __restrict__ delta, float* __restrict__ gmax) {
  __shared__ float sMax[4];
  const int hd = blockIdx.y, b = blockIdx.z;
  const int tok = blockIdx.x * kTQ + (threadIdx.x >> 1), half = threadIdx.x & 1;
  float acc = 0.f, amax = 0.f;
  if (tok < a.Nq) {
    const float* g = dO + ((int64_t)b * a.Nq + tok) * a.lddo + hd * kD + 32 * half;
    const float* o = O + ((int64_t)b * a.Nq + tok) * a.ldo + hd * kD + 32 * half;
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
  if (tok < a.Nq && half == 0) delta[((int64_t)b * a.heads + hd) * a.Nq + tok] = acc + other;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  if ((threadIdx.x & 63) == 0) sMax[threadIdx.x >> 6] = amax;
  __syncthreads();
  if (threadIdx.x == 0)
    gmax[((int64_t)b * a.heads + hd) * gridDim.x + blockIdx.x] =
        fmaxf(fmaxf(sMax[0], sMax[1]), fmaxf(sMax[2], sMax[3]));
}

struct F16Ops {
  static constexpr int kPitchR = 72;   // halves per row of the "rows" image
  static constexpr int kPitchC = 36;   // halves per row of the "cols" image
  static constexpr float kF16Max = 65504.f;
  static constexpr int kSteps1 = 4;    // MFMAs (k = 16) of a 64-deep first product
  static constexpr int kSteps2 = 2;    // MFMAs of a 32-deep second product

  static __device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }

  // B fragments: reg[s][j] = row[16 s + 8 h + j]
  struct Row {
    f16x8 reg[4];
  };
  // this lane's B fragments of a row it owns, times mul, rounded to fp16; zeros for a row past the end
  static __device__ __forceinline__ void load_row(Row& r, const float* row, bool ok, int h, float mul) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      f32x4 v0 = f32x4{0.f, 0.f, 0.f, 0.f}, v1 = v0;
      if (ok) {
        v0 = ld4(row + 16 * s + 8 * h) * mul;
        v1 = ld4(row + 16 * s + 8 * h + 4) * mul;
      }
      r.reg[s] = f16x8{(_Float16)v0.x, (_Float16)v0.y, (_Float16)v0.z, (_Float16)v0.w,
                       (_Float16)v1.x, (_Float16)v1.y, (_Float16)v1.z, (_Float16)v1.w};
    }
  }

  // the images a kernel asks for: rows [row][d], cols [d][row]
  template <bool kRows, bool kCols>
  struct Tile;
  // A thread's share of a 32 x 64 tile on its way from memory to LDS: thread (kg, c2) holds rows 4 kg ..
  // 4 kg + 3, columns 2 c2 and 2 c2 + 1.  The loads of the NEXT tile are issued before the products of the
  // current one and land in LDS after them, so their latency is hidden behind the MFMAs (a register prefetch).
  struct TileLoad {
    float2 v[4];
  };
  // rows [row0, row0 + 32) of one (batch, head) block `src` (pitch ld); rows >= N are 0 and are not read
  static __device__ __forceinline__ void load_tile(TileLoad& t, const float* src, int row0, int N, int ld) {
    const int c2 = threadIdx.x & 31, kg = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + 4 * kg + i;
      t.v[i] = float2{0.f, 0.f};
      if (row < N) t.v[i] = *reinterpret_cast<const float2*>(src + (int64_t)row * ld + 2 * c2);
    }
  }
  // the tile times mul, rounded to fp16, into the images the tile has
  template <bool kRows, bool kCols>
  static __device__ __forceinline__ void store_tile(Tile<kRows, kCols>& tile, const TileLoad& t, float mul) {
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
        *reinterpret_cast<f16x2*>(tile.rows + (4 * kg + i) * kPitchR + 2 * c2) = f16x2{x[i], y[i]};
    }
    if constexpr (kCols) {
      *reinterpret_cast<f16x4*>(tile.cols + (2 * c2) * kPitchC + 4 * kg) = f16x4{x[0], x[1], x[2], x[3]};
      *reinterpret_cast<f16x4*>(tile.cols + (2 * c2 + 1) * kPitchC + 4 * kg) = f16x4{y[0], y[1], y[2], y[3]};
    }
  }

  // k-step st (0..3) of (tile row `row`) x (owned row): the A fragment is d = 16 st + 8 h + j of the row
  template <bool kCols>
  static __device__ __forceinline__ f32x16 mma1(const Tile<true, kCols>& t, int row, int st, const Row& r,
                                                f32x16 acc, int h) {
    return mfma16(*reinterpret_cast<const f16x8*>(t.rows + row * kPitchR + 16 * st + 8 * h), r.reg[st], acc);
  }
  // registers 8 st .. 8 st + 7 of an accumulator as the B fragment of k-step st (0, 1)
  typedef f16x8 Frag;
  static __device__ __forceinline__ Frag frag(const f32x16& x, int st) {
    f16x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (_Float16)x[8 * st + j];
    return f;
  }
  // the same with the conversion saturating at the fp16 maximum (NaN stays NaN)
  static __device__ __forceinline__ Frag frag_sat(const f32x16& x, int st) {
    f16x8 f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = x[8 * st + j];
      f[j] = (_Float16)(v > kF16Max ? kF16Max : (v < -kF16Max ? -kF16Max : v));
    }
    return f;
  }
  // k-step st of (tile column d) x (accumulator fragment): the A fragment is column d in the k order of an
  // accumulator fragment (tile rows 16 st + 8 (j >> 2) + 4 h + (j & 3))
  template <bool kRows>
  static __device__ __forceinline__ f32x16 mma2(const Tile<kRows, true>& t, int d, int st, Frag b, f32x16 acc,
                                                int h) {
    const _Float16* p = t.cols + d * kPitchC + 16 * st + 4 * h;
    const f16x4 lo = *reinterpret_cast<const f16x4*>(p), hi = *reinterpret_cast<const f16x4*>(p + 8);
    return mfma16(f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}, b, acc);
  }

  // the pre-pass's n maxima of |dO|
  struct GradMax {
    const float* gmax;
    int64_t n;
  };
  // The exponent e of the gradient scale (the same value in every thread of every workgroup: a maximum does
  // not depend on the order).  2^e brings max|dO| into [4, 8); 0 for a maximum that is 0 or not finite;
  // |e| <= 126 so that 2^e and 2^-e are normal floats.  Contains a barrier: called by the whole workgroup.
  static __device__ __forceinline__ int grad_exponent(const GradMax& gm) {
    __shared__ float sMax[4];
    float m = 0.f;
    for (int64_t i = threadIdx.x; i < gm.n; i += 256) m = fmaxf(m, gm.gmax[i]);
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

  // delta[B][heads][N], then max|dO| of each of the pre-pass's B * heads * ceil(N / 128) workgroups
  static size_t ws_bytes(const gs_attention_kv_desc* d) {
    const int64_t floats = (int64_t)d->B * d->heads * (d->Nq + attn_tiles(d));
    return (size_t)ceil_div(floats * (int64_t)sizeof(float), 16) * 16;
  }
  static GradMax launch_delta(const gs_attention_kv_desc* d, const AttnArgs& a, const float* d_o, const float* o,
                              float* delta, hipStream_t stream) {
    float* gmax = delta + (int64_t)d->B * d->heads * d->Nq;
    hipLaunchKernelGGL(attn_delta_f16_kernel, attn_grid(d), dim3(256), 0, stream, a, d_o, o, delta, gmax);
    return GradMax{gmax, (int64_t)d->B * d->heads * attn_tiles(d)};
  }
};

template <>
struct F16Ops::Tile<true, false> {
  __attribute__((aligned(16))) _Float16 rows[kTK * kPitchR];
};
template <>
struct F16Ops::Tile<false, true> {
  __attribute__((aligned(16))) _Float16 cols[kD * kPitchC];
};
template <>
struct F16Ops::Tile<true, true> {
  __attribute__((aligned(16))) _Float16 rows[kTK * kPitchR];
  __attribute__((aligned(16))) _Float16 cols[kD * kPitchC];
};

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" size_t gs_attention_workspace_bytes_f16(const gs_attention_desc* d) {
  return attn_workspace_bytes<F16Ops>(SelfDesc(d).p, 1);
}

extern "C" int gs_attention_forward_f16(const gs_attention_desc* d, const float* q, const float* k,
                                        const float* v, float* o, float* lse, void* stream) {
  return attn_forward<F16Ops>(SelfDesc(d).p, q, k, v, o, lse, stream);
}

extern "C" int gs_attention_relpos_forward_f16(const gs_attention_desc* d, const float* q, const float* k,
                                               const float* v, const float* table, int32_t ld_table,
                                               int32_t Wh, int32_t Ww, float* o, float* lse, void* stream) {
  return attn_relpos_forward<F16Ops>(SelfDesc(d).p, q, k, v, table, ld_table, Wh, Ww, o, lse, stream);
}

extern "C" int gs_attention_backward_f16(const gs_attention_desc* d, const float* q, const float* k,
                                         const float* v, const float* o, const float* lse, const float* d_o,
                                         float* dq, float* dk, float* dv, int accumulate, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return attn_backward<F16Ops>(SelfDesc(d).p, q, k, v, o, lse, d_o, dq, dk, dv, accumulate, workspace,
                               workspace_bytes, 1, stream);
}
