// What the fp32 attention kernels (attention.hip) and the fp16-operand ones (attention_f16.hip) share: the
// tile sizes, the 32x32 accumulator's register map, the row store and the host-side descriptor checks.
#pragma once
#include "common.h"

namespace gs {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kD = 64;        // head dimension
constexpr int kTK = 32;       // rows of a tile that is swept through LDS
constexpr int kTQ = 128;      // rows a workgroup owns (32 per wave)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}

struct AttnArgs {
  int32_t B, N, heads;
  int32_t ldq, ldk, ldv, ldo, lddq, lddk, lddv, lddo;
  float scale;
  int32_t accumulate;
};

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

// BEiT's relative-position bias: one fp32 table [(2 Wh - 1)(2 Ww - 1) + 3][heads] (row pitch ld)
struct AttnBias {
  const float* table;
  int32_t ld, Wh, Ww, R;   // R = (2 Wh - 1)(2 Ww - 1): rows R, R + 1, R + 2 are the three cls entries
};

int attn_check(const gs_attention_desc* d) {
  if (!d) return GS_E_NULL;
  if (d->B <= 0 || d->N <= 0 || d->heads <= 0 || !(d->scale > 0.f)) return GS_E_BADARG;
  if (d->B > 65535 || d->heads > 65535 || d->heads > INT32_MAX / kD) return GS_E_BADARG;
  const int32_t ld[8] = {d->ldq, d->ldk, d->ldv, d->ldo, d->lddq, d->lddk, d->lddv, d->lddo};
  for (int i = 0; i < 8; ++i)
    if (ld[i] % 4) return GS_E_ALIGN;
  for (int i = 0; i < 8; ++i)
    if (ld[i] < kD * d->heads) return GS_E_BADARG;
  return GS_OK;
}

// what gs_attention_relpos_forward checks beyond attn_check, before the pointers
int attn_relpos_check(const gs_attention_desc* d, int32_t ld_table, int32_t Wh, int32_t Ww) {
  if (Wh < 1 || Ww < 1 || (int64_t)Wh * Ww + 1 != d->N || ld_table < d->heads) return GS_E_BADARG;
  const int64_t R = (2 * (int64_t)Wh - 1) * (2 * (int64_t)Ww - 1);
  return R + 3 > GS_ATTENTION_RELPOS_MAX_ROWS ? GS_E_BADARG : GS_OK;
}

AttnArgs attn_args(const gs_attention_desc* d, int accumulate) {
  AttnArgs a;
  a.B = d->B; a.N = d->N; a.heads = d->heads;
  a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv; a.ldo = d->ldo;
  a.lddq = d->lddq; a.lddk = d->lddk; a.lddv = d->lddv; a.lddo = d->lddo;
  a.scale = d->scale;
  a.accumulate = accumulate ? 1 : 0;
  return a;
}

}  // namespace
}  // namespace gs
