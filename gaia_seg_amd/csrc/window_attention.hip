// Swin's operators (gs_window_attention_*, gs_map_pad / gs_map_crop, gs_cell_layernorm_* in
// include/gaiaseg_hip.h).
//
// Shifted-window attention, head dimension 32, on fp32 NHWC maps.  The roll, the window partition, the
// relative-position bias, the region mask, the reverse and the roll back are index arithmetic: token t of
// window (wy, wx) sits at (y', x') = (wy ws + t / ws, wx ws + t % ws) of the shifted frame, i.e. at
// ((y' + shift) mod H, (x' + shift) mod W) of the map.  No [windows, heads, ws^2, ws^2] tensor exists.
//
// Structure.  A workgroup is ONE wave and handles one (window, head) at a time; the ws^2 <= 64 tokens are
// padded to 64, so a window is a 64 x 64 score matrix of four 32 x 32 tiles of the exact fp32 MFMA
// v_mfma_f32_32x32x2_f32 (lane l: i = l & 31, h = l >> 5; A[i][k = h], B[k = h][j = i]; the result has its
// column on the lane and row (r & 3) + 8 (r >> 2) + 4 h in register r).  As in attention_common.h every
// product is oriented so that the next one sums over the result's row index and takes the registers as its
// B operand as they stand.  A [64][32] operand is an LDS image at a pitch of 33 floats: read by rows
// ([lane row][2 s + h]) and by columns ([acc_row][lane]) without bank conflicts.
//
//   forward  : grid (windows, heads, B).  Q, K, V staged (lane t loads token t's 32 floats).  For each half
//              of the queries: S^T = K Q^T (query on the lane; all 64 keys at once, so the softmax is one
//              pass: no running maximum), + bias + mask, O^T = V^T P^T.  LDS 26768 B (26.1 KiB).
//   backward : grid (slabs, heads); a workgroup walks the (batch, window) items of its slab.  Per item: Q, K,
//              dO staged, V staged through the dS image into registers, delta = <dO, O> on lane t.  For each
//              half of the keys: S = Q K^T and dP = dO V^T (key on the lane), P, dS = P (dP - delta) written to
//              the [64][65] dS image, dV^T = dO^T P, dK^T = Q^T dS, stored.  Then dQ = dS K (rows of the dS
//              image times columns of the K image) and the table: lane e owns table entries e, e + 64, ...
//              and walks the (ws - |dy|)(ws - |dx|) pairs of each in a fixed order out of the dS image,
//              adding into a register that lives across the slab's windows.  The slab's [heads][R] partial
//              goes to the workspace; win_table_combine_kernel adds the slabs in slab order.  dQ, dK, dV
//              are complete inside a window.  No float atomics; bit-identical from run to run.  LDS 44688 B (43.6 KiB).
//   padding  : a token past ws^2 is staged as zeros and never read from memory; as a key it scores -inf
//              (p = 0 exactly), as a query it is never stored and its p is forced to 0 in the backward.
#include <math.h>

#include <algorithm>

#include "common.h"

namespace gs {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWD = 32;      // head dimension
constexpr int kWT = 64;      // tokens of a padded window
constexpr int kWP = 33;      // pitch of a [64][32] image
constexpr int kSP = 65;      // pitch of the [64][64] dS image
constexpr int kMaxR = 225;   // (2 * 8 - 1)^2 table rows

__device__ __forceinline__ int wacc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ f32x16 wzero16() {
  f32x16 z;
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.f;
  return z;
}
__device__ __forceinline__ f32x16 wmfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

struct WinArgs {
  int32_t B, H, W, ws, shift, heads;
  int32_t ldq, ldk, ldv, ldo, lddq, lddk, lddv, lddo, ld_table;
  float scale;
  int32_t accumulate;
  int32_t nwx, nw, R;   // windows along W, windows per image, table rows
};

// token t of window (wy, wx) of image b
struct Tok {
  bool ok;          // t < ws^2
  int64_t row;      // its row in the "rows x C" views (0 for a padded token)
  int64_t pix;      // y * W + x
  int qterm, koff;  // idx(i, j) = qterm(i) + koff(j)
  int region;       // 0 without a shift
};
__device__ __forceinline__ int win_r(int t, int L, int ws, int shift) { return (t >= L - ws) + (t >= L - shift); }
__device__ __forceinline__ Tok win_tok(const WinArgs& a, int b, int wy, int wx, int t) {
  Tok k;
  k.ok = t < a.ws * a.ws;
  const int iy = t / a.ws, ix = t - iy * a.ws;
  const int yp = wy * a.ws + iy, xp = wx * a.ws + ix;
  int y = yp + a.shift, x = xp + a.shift;
  y -= y >= a.H ? a.H : 0;
  x -= x >= a.W ? a.W : 0;
  k.pix = k.ok ? (int64_t)y * a.W + x : 0;
  k.row = k.ok ? (int64_t)b * a.H * a.W + k.pix : 0;
  k.qterm = k.ok ? iy * (2 * a.ws - 1) + ix : 0;
  k.koff = k.ok ? (a.ws - 1 - iy) * (2 * a.ws - 1) + (a.ws - 1 - ix) : 0;
  k.region = (k.ok && a.shift > 0) ? 3 * win_r(yp, a.H, a.ws, a.shift) + win_r(xp, a.W, a.ws, a.shift) : 0;
  return k;
}

// the 32 floats of a token's head (zeros for a padded token) into row `t` of a [64][32] image
__device__ __forceinline__ void stage_row(float* img, int t, const float* src, bool ok) {
#pragma unroll
  for (int c = 0; c < kWD / 4; ++c) {
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ok) v = ld4(src + 4 * c);
    float* d = img + t * kWP + 4 * c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
}

// an accumulator (columns d of a row this lane owns, transposed: register r is d = 8 (r >> 2) + 4 h + (r & 3))
__device__ __forceinline__ void wstore_row(float* row, const f32x16& acc, int h, float mul, int accumulate) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 v = f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]} * mul;
    float* p = row + 8 * g + 4 * h;
    if (accumulate) v += ld4(p);
    st4(p, v);
  }
}

// scale * s + table[idx] (+ the -100 of two regions)
__device__ __forceinline__ float win_score(float s, float scale, const float* sTab, int idx, bool other_region) {
  float sc = __fmul_rn(s, scale) + sTab[idx];
  if (other_region) sc += -100.0f;
  return sc;
}

__global__ __launch_bounds__(64) void win_forward_kernel(const WinArgs a, const float* __restrict__ Q,
                                                         const float* __restrict__ K,
                                                         const float* __restrict__ V,
                                                         const float* __restrict__ table, float* __restrict__ O,
                                                         float* __restrict__ lse) {
  __shared__ float sQ[kWT * kWP];
  __shared__ float sK[kWT * kWP];
  __shared__ float sV[kWT * kWP];
  __shared__ float sTab[kMaxR + 3];
  __shared__ int sKoff[kWT];
  __shared__ int sReg[kWT];
  const int lane = threadIdx.x, l32 = lane & 31, h = lane >> 5;
  const int win = blockIdx.x, hd = blockIdx.y, b = blockIdx.z;
  const int wy = win / a.nwx, wx = win - wy * a.nwx;
  const int N = a.ws * a.ws;
  {
    const Tok t = win_tok(a, b, wy, wx, lane);
    stage_row(sQ, lane, Q + t.row * a.ldq + hd * kWD, t.ok);
    stage_row(sK, lane, K + t.row * a.ldk + hd * kWD, t.ok);
    stage_row(sV, lane, V + t.row * a.ldv + hd * kWD, t.ok);
    sKoff[lane] = t.koff;
    sReg[lane] = t.region;
    for (int e = lane; e < a.R; e += kWT) sTab[e] = table[(int64_t)e * a.ld_table + hd];
  }
  __syncthreads();
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const Tok ti = win_tok(a, b, wy, wx, qb * 32 + l32);   // the query on this lane
    float qreg[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) qreg[s] = sQ[(qb * 32 + l32) * kWP + 2 * s + h];
    f32x16 s0 = wzero16(), s1 = wzero16();   // S^T[key][query], keys 0..31 and 32..63
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      s0 = wmfma(sK[l32 * kWP + 2 * st + h], qreg[st], s0);
      s1 = wmfma(sK[(32 + l32) * kWP + 2 * st + h], qreg[st], s1);
    }
    float m = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j0 = wacc_row(r, h), j1 = 32 + j0;
      s0[r] = j0 < N ? win_score(s0[r], a.scale, sTab, ti.qterm + sKoff[j0], sReg[j0] != ti.region) : -INFINITY;
      s1[r] = j1 < N ? win_score(s1[r], a.scale, sTab, ti.qterm + sKoff[j1], sReg[j1] != ti.region) : -INFINITY;
      m = fmaxf(m, fmaxf(s0[r], s1[r]));
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));   // finite: key 0 exists
    float l = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s0[r] = expf(s0[r] - m);   // exactly 0 for a padded key
      s1[r] = expf(s1[r] - m);
      l += s0[r] + s1[r];
    }
    l += __shfl_xor(l, 32, 64);
    f32x16 o = wzero16();   // O^T[d][query] = V^T[d][key] P^T[key][query]
#pragma unroll
    for (int st = 0; st < 16; ++st) o = wmfma(sV[wacc_row(st, h) * kWP + l32], s0[st], o);
#pragma unroll
    for (int st = 0; st < 16; ++st) o = wmfma(sV[(32 + wacc_row(st, h)) * kWP + l32], s1[st], o);
    if (ti.ok) {
      wstore_row(O + ti.row * a.ldo + hd * kWD, o, h, 1.0f / l, 0);
      if (h == 0) lse[((int64_t)b * a.heads + hd) * a.H * a.W + ti.pix] = m + logf(l);
    }
  }
}

// grid (slabs, heads): slab s walks items [s * per, min(items, (s + 1) * per)) of the B * nw (batch, window)
// pairs and leaves its table partial at part[(s * heads + head) * R ..]
__global__ __launch_bounds__(64) void win_backward_kernel(
    const WinArgs a, const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V,
    const float* __restrict__ table, const float* __restrict__ O, const float* __restrict__ lse,
    const float* __restrict__ dO, float* dQ, float* dK, float* dV, float* __restrict__ part, const int64_t per,
    const int64_t items) {
  __shared__ float sQ[kWT * kWP];
  __shared__ float sK[kWT * kWP];
  __shared__ float sG[kWT * kWP];
  __shared__ float sDS[kWT * kSP];   // V at pitch kWP first, then dS[query][key]
  __shared__ float sTab[kMaxR + 3];
  __shared__ float sL[kWT];
  __shared__ float sD[kWT];
  __shared__ int sKoff[kWT];
  __shared__ int sQt[kWT];
  __shared__ int sReg[kWT];
  __shared__ int64_t sRow[kWT];
  const int lane = threadIdx.x, l32 = lane & 31, h = lane >> 5;
  const int hd = blockIdx.y;
  const int N = a.ws * a.ws, T = 2 * a.ws - 1;
  for (int e = lane; e < a.R; e += kWT) sTab[e] = table[(int64_t)e * a.ld_table + hd];
  float tacc[4] = {0.f, 0.f, 0.f, 0.f};   // table entries lane, lane + 64, lane + 128, lane + 192
  const int64_t begin = (int64_t)blockIdx.x * per;
  const int64_t end = begin + per < items ? begin + per : items;
  for (int64_t it = begin; it < end; ++it) {
    const int b = (int)(it / a.nw), win = (int)(it - (int64_t)b * a.nw);
    const int wy = win / a.nwx, wx = win - wy * a.nwx;
    __syncthreads();   // the previous window's reads of the images
    {
      const Tok t = win_tok(a, b, wy, wx, lane);
      const float* g = dO + t.row * a.lddo + hd * kWD;
      const float* o = O + t.row * a.ldo + hd * kWD;
      stage_row(sQ, lane, Q + t.row * a.ldq + hd * kWD, t.ok);
      stage_row(sK, lane, K + t.row * a.ldk + hd * kWD, t.ok);
      stage_row(sDS, lane, V + t.row * a.ldv + hd * kWD, t.ok);
      stage_row(sG, lane, g, t.ok);
      float acc = 0.f;   // delta = <dO, O> as the d-ordered fma chain
      if (t.ok) {
#pragma unroll
        for (int c = 0; c < kWD / 4; ++c) {
          const f32x4 x = ld4(g + c * 4), y = ld4(o + c * 4);
          acc = fmaf(x.x, y.x, acc);
          acc = fmaf(x.y, y.y, acc);
          acc = fmaf(x.z, y.z, acc);
          acc = fmaf(x.w, y.w, acc);
        }
      }
      sD[lane] = acc;
      sL[lane] = t.ok ? lse[((int64_t)b * a.heads + hd) * a.H * a.W + t.pix] : 0.f;
      sKoff[lane] = t.koff;
      sQt[lane] = t.qterm;
      sReg[lane] = t.region;
      sRow[lane] = t.ok ? t.row : -1;
    }
    __syncthreads();
    float vreg[2][16];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int s = 0; s < 16; ++s) vreg[kb][s] = sDS[(kb * 32 + l32) * kWP + 2 * s + h];
    __syncthreads();   // V is in registers: the image becomes dS
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int j = kb * 32 + l32;   // the key on this lane
      const bool jok = j < N;
      const int koff = sKoff[j], jreg = sReg[j];
      float kreg[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) kreg[s] = sK[j * kWP + 2 * s + h];
      f32x16 s0 = wzero16(), s1 = wzero16(), dp0 = wzero16(), dp1 = wzero16();   // [query][key]
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        s0 = wmfma(sQ[l32 * kWP + 2 * st + h], kreg[st], s0);
        s1 = wmfma(sQ[(32 + l32) * kWP + 2 * st + h], kreg[st], s1);
        dp0 = wmfma(sG[l32 * kWP + 2 * st + h], vreg[kb][st], dp0);
        dp1 = wmfma(sG[(32 + l32) * kWP + 2 * st + h], vreg[kb][st], dp1);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int q0 = wacc_row(r, h), q1 = 32 + q0;
        float p0 = 0.f, p1 = 0.f;
        if (jok && q0 < N)
          p0 = expf(win_score(s0[r], a.scale, sTab, sQt[q0] + koff, sReg[q0] != jreg) - sL[q0]);
        if (jok && q1 < N)
          p1 = expf(win_score(s1[r], a.scale, sTab, sQt[q1] + koff, sReg[q1] != jreg) - sL[q1]);
        s0[r] = p0;
        s1[r] = p1;
        dp0[r] = p0 * (dp0[r] - sD[q0]);
        dp1[r] = p1 * (dp1[r] - sD[q1]);
        sDS[q0 * kSP + j] = dp0[r];
        sDS[q1 * kSP + j] = dp1[r];
      }
      f32x16 dv = wzero16(), dk = wzero16();   // dV^T[d][key] = dO^T[d][q] P[q][key];  dK^T = Q^T dS
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        dv = wmfma(sG[wacc_row(st, h) * kWP + l32], s0[st], dv);
        dk = wmfma(sQ[wacc_row(st, h) * kWP + l32], dp0[st], dk);
      }
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        dv = wmfma(sG[(32 + wacc_row(st, h)) * kWP + l32], s1[st], dv);
        dk = wmfma(sQ[(32 + wacc_row(st, h)) * kWP + l32], dp1[st], dk);
      }
      const int64_t row = sRow[j];
      if (row >= 0) {
        wstore_row(dK + row * a.lddk + hd * kWD, dk, h, a.scale, a.accumulate);
        wstore_row(dV + row * a.lddv + hd * kWD, dv, h, 1.f, a.accumulate);
      }
    }
    __syncthreads();   // dS is complete
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {   // dQ[query][d] = dS[query][key] K[key][d]: d on the lane
      f32x16 dq = wzero16();
#pragma unroll
      for (int st = 0; st < 32; ++st)
        dq = wmfma(sDS[(qb * 32 + l32) * kSP + 2 * st + h], sK[(2 * st + h) * kWP + l32], dq);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = sRow[qb * 32 + wacc_row(r, h)];
        if (row >= 0) {
          float* p = dQ + row * a.lddq + hd * kWD + l32;
          float v = dq[r] * a.scale;
          if (a.accumulate) v += *p;
          *p = v;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {   // the table: entry e = (dy + ws - 1) T + (dx + ws - 1), dy = iy - jy
      const int e = lane + 64 * u;
      if (e < a.R) {
        const int ey = e / T, dy = ey - (a.ws - 1), dx = e - ey * T - (a.ws - 1);
        const int jy0 = dy < 0 ? -dy : 0, jy1 = dy > 0 ? a.ws - dy : a.ws;
        const int jx0 = dx < 0 ? -dx : 0, jx1 = dx > 0 ? a.ws - dx : a.ws;
        float sum = 0.f;
        for (int jy = jy0; jy < jy1; ++jy)
          for (int jx = jx0; jx < jx1; ++jx)
            sum += sDS[((jy + dy) * a.ws + jx + dx) * kSP + jy * a.ws + jx];
        tacc[u] += sum;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = lane + 64 * u;
    if (e < a.R) part[((int64_t)blockIdx.x * a.heads + hd) * a.R + e] = tacc[u];
  }
}

// dtable[r][h] = (or +=) the sum over the slabs, in slab order, of part[s][h][r]
__global__ __launch_bounds__(256) void win_table_combine_kernel(const float* __restrict__ part, float* dtable,
                                                                const int slabs, const int heads, const int R,
                                                                const int ld_table, const int accumulate) {
  const int it = blockIdx.x * 256 + threadIdx.x;
  if (it >= heads * R) return;
  const int hd = it / R, r = it - hd * R;
  float sum = part[it];
  for (int s = 1; s < slabs; ++s) sum += part[(int64_t)s * heads * R + it];
  float* dst = dtable + (int64_t)r * ld_table + hd;
  if (accumulate) sum += *dst;
  *dst = sum;
}

int win_check(const gs_window_attention_desc* d) {
  if (!d) return GS_E_NULL;
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->heads <= 0 || !(d->scale > 0.f)) return GS_E_BADARG;
  if (d->B > 65535 || d->heads > 65535) return GS_E_BADARG;
  if (d->ws < 2 || d->ws > 8 || d->H % d->ws || d->W % d->ws) return GS_E_BADARG;
  if (d->shift < 0 || d->shift >= d->ws) return GS_E_BADARG;
  if ((int64_t)d->B * d->H * d->W > INT32_MAX) return GS_E_BADARG;
  const int32_t ld[8] = {d->ldq, d->ldk, d->ldv, d->ldo, d->lddq, d->lddk, d->lddv, d->lddo};
  for (int i = 0; i < 8; ++i)
    if (ld[i] % 4) return GS_E_ALIGN;
  for (int i = 0; i < 8; ++i)
    if (ld[i] < kWD * d->heads) return GS_E_BADARG;
  if (d->ld_table < d->heads) return GS_E_BADARG;
  return GS_OK;
}

WinArgs win_args(const gs_window_attention_desc* d, int accumulate) {
  WinArgs a;
  a.B = d->B; a.H = d->H; a.W = d->W; a.ws = d->ws; a.shift = d->shift; a.heads = d->heads;
  a.ldq = d->ldq; a.ldk = d->ldk; a.ldv = d->ldv; a.ldo = d->ldo;
  a.lddq = d->lddq; a.lddk = d->lddk; a.lddv = d->lddv; a.lddo = d->lddo;
  a.ld_table = d->ld_table;
  a.scale = d->scale;
  a.accumulate = accumulate ? 1 : 0;
  a.nwx = d->W / d->ws;
  a.nw = a.nwx * (d->H / d->ws);
  a.R = (2 * d->ws - 1) * (2 * d->ws - 1);
  return a;
}

// The slabs of the backward: `slabs` runs of `per` consecutive (batch, window) items, none empty.  The plan
// is a pure function of the descriptor and the CU count: the backward's 44688 B (43.6 KiB) of LDS let three
// workgroups share a CU, so slabs x heads fills one round of those places and no more.  Measured at the four
// stage maps of a 1024x512 crop (profiles/r24_swin.md): the plan is the fastest of S = plan / 4 .. 4 x plan at
// every shape; twice as many slabs cost 14 .. 28 % (a second, partly filled round), half as many 64 .. 107 %.
constexpr int kWinPlacesPerCU = 3;
struct WinSplit {
  int64_t slabs, per;
};
inline WinSplit win_split(const gs_window_attention_desc* d, int64_t want) {
  const int64_t items = (int64_t)d->B * (d->H / d->ws) * (d->W / d->ws);
  if (want <= 0) want = (int64_t)kWinPlacesPerCU * num_cu() / d->heads;
  want = std::max<int64_t>(1, std::min<int64_t>(want, items));
  const int64_t per = ceil_div(items, want);
  return WinSplit{ceil_div(items, per), per};
}
inline size_t win_ws_bytes(const gs_window_attention_desc* d, const WinSplit& sp) {
  const int64_t R = (2 * d->ws - 1) * (2 * d->ws - 1);
  return (size_t)ceil_div(sp.slabs * d->heads * R * (int64_t)sizeof(float), 16) * 16;
}

int g_win_split = -1;

// ---- gs_map_pad / gs_map_crop -----------------------------------------------------------------------------
// one thread per four channels of a pixel of the LARGER map [B][Hp][Wp]
__global__ __launch_bounds__(256) void map_pad_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                      const int64_t items, const int H, const int W,
                                                      const int Hp, const int Wp, const int c4, const int lds,
                                                      const int ldd, const int accumulate) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % c4);
    const int64_t pix = it / c4;
    const int x = (int)(pix % Wp);
    const int y = (int)((pix / Wp) % Hp);
    const int64_t b = pix / ((int64_t)Wp * Hp);
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (y < H && x < W) v = ld4(src + ((b * H + y) * W + x) * lds + cq * 4);
    float* p = dst + pix * ldd + cq * 4;
    if (accumulate) v += ld4(p);
    st4(p, v);
  }
}
// one thread per four channels of a pixel of the SMALLER map [B][H][W]
__global__ __launch_bounds__(256) void map_crop_kernel(const float* __restrict__ src, float* dst,
                                                       const int64_t items, const int H, const int W,
                                                       const int Hp, const int Wp, const int c4, const int lds,
                                                       const int ldd, const int accumulate) {
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int cq = (int)(it % c4);
    const int64_t pix = it / c4;
    const int x = (int)(pix % W);
    const int y = (int)((pix / W) % H);
    const int64_t b = pix / ((int64_t)W * H);
    f32x4 v = ld4(src + ((b * Hp + y) * Wp + x) * lds + cq * 4);
    float* p = dst + pix * ldd + cq * 4;
    if (accumulate) v += ld4(p);
    st4(p, v);
  }
}

// small map [B][H][W] with pitch ld_small, padded map [B][Hp][Wp] with pitch ld_big
int map_check(int32_t B, int32_t H, int32_t W, int32_t Hp, int32_t Wp, int32_t C, int32_t ld_small,
              int32_t ld_big) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Hp < H || Wp < W) return GS_E_BADARG;
  if ((int64_t)B * Hp * Wp > INT32_MAX) return GS_E_BADARG;
  if (C % 4 || ld_small % 4 || ld_big % 4) return GS_E_ALIGN;
  if (ld_small < C || ld_big < C) return GS_E_BADARG;
  return GS_OK;
}

// ---- gs_cell_layernorm_* ----------------------------------------------------------------------------------
// A LayerNorm over the 4 C values of a 2 x 2 cell of the map, written back as a map: the statistics of Swin's
// patch merging without the space-to-depth copy.  Pixel (2 cy + r, 2 cx + q) of a cell is phase g = 2 q + r
// and reads the parameters at g * Cmax + c.
struct CellArgs {
  int64_t cells;
  int32_t H, W, C, Cmax, ldx, ldy;
  float eps;
};
__device__ __forceinline__ float wave_allsum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
// the first pixel of cell `cell`
__device__ __forceinline__ int64_t cell_pixel(const CellArgs& a, int64_t cell) {
  const int cw = a.W / 2, ch = a.H / 2;
  const int cx = (int)(cell % cw);
  const int cy = (int)((cell / cw) % ch);
  const int64_t b = cell / ((int64_t)cw * ch);
  return (b * a.H + 2 * cy) * a.W + 2 * cx;
}
// item i of a cell's 4 * (C / 4) float4s: phase g (r = g & 1, q = g >> 1) and channel quad
__device__ __forceinline__ int64_t cell_item(const CellArgs& a, int i, int c4, int& g, int& cq) {
  g = i / c4;
  cq = i - g * c4;
  return (int64_t)(g & 1) * a.W + (g >> 1);   // pixel offset inside the cell
}

// one wave per cell, 4 cells per workgroup
__global__ __launch_bounds__(256) void cell_ln_forward_kernel(const CellArgs a, const float* __restrict__ x,
                                                              const float* __restrict__ weight,
                                                              const float* __restrict__ bias,
                                                              float* __restrict__ y, float* __restrict__ mean,
                                                              float* __restrict__ rstd) {
  const int lane = threadIdx.x & 63;
  const int c4 = a.C / 4, n4 = 4 * c4;
  const float inv = 1.0f / (float)(4 * a.C);
  for (int64_t cell = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); cell < a.cells; cell += (int64_t)gridDim.x * 4) {
    const int64_t p0 = cell_pixel(a, cell);
    float s = 0.f;
    for (int i = lane; i < n4; i += 64) {
      int g, cq;
      const int64_t po = cell_item(a, i, c4, g, cq);
      const f32x4 v = ld4(x + (p0 + po) * a.ldx + cq * 4);
      s += (v.x + v.y) + (v.z + v.w);
    }
    const float mu = wave_allsum(s) * inv;
    float s2 = 0.f;
    for (int i = lane; i < n4; i += 64) {
      int g, cq;
      const int64_t po = cell_item(a, i, c4, g, cq);
      const f32x4 v = ld4(x + (p0 + po) * a.ldx + cq * 4) - mu;
      s2 += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    const float rs = 1.0f / sqrtf(wave_allsum(s2) * inv + a.eps);
    for (int i = lane; i < n4; i += 64) {
      int g, cq;
      const int64_t po = cell_item(a, i, c4, g, cq);
      const f32x4 v = (ld4(x + (p0 + po) * a.ldx + cq * 4) - mu) * rs;
      const int pc = g * a.Cmax + cq * 4;
      st4(y + (p0 + po) * a.ldy + cq * 4, v * ld4(weight + pc) + ld4(bias + pc));
    }
    if (lane == 0) {
      mean[cell] = mu;
      rstd[cell] = rs;
    }
  }
}

// dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy * weight, the means over the cell's 4 C values
__global__ __launch_bounds__(256) void cell_ln_backward_dx_kernel(const CellArgs a, const float* __restrict__ x,
                                                                  const float* dy,
                                                                  const float* __restrict__ weight,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ rstd, float* dx,
                                                                  const int accumulate) {
  const int lane = threadIdx.x & 63;
  const int c4 = a.C / 4, n4 = 4 * c4;
  const float inv = 1.0f / (float)(4 * a.C);
  for (int64_t cell = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); cell < a.cells; cell += (int64_t)gridDim.x * 4) {
    const int64_t p0 = cell_pixel(a, cell);
    const float mu = mean[cell], rs = rstd[cell];
    float sg = 0.f, sgx = 0.f;
    for (int i = lane; i < n4; i += 64) {
      int g, cq;
      const int64_t po = cell_item(a, i, c4, g, cq);
      const f32x4 xh = (ld4(x + (p0 + po) * a.ldx + cq * 4) - mu) * rs;
      const f32x4 gv = ld4(dy + (p0 + po) * a.ldy + cq * 4) * ld4(weight + g * a.Cmax + cq * 4);
      sg += (gv.x + gv.y) + (gv.z + gv.w);
      sgx += (gv.x * xh.x + gv.y * xh.y) + (gv.z * xh.z + gv.w * xh.w);
    }
    const float mg = wave_allsum(sg) * inv, mgx = wave_allsum(sgx) * inv;
    for (int i = lane; i < n4; i += 64) {
      int g, cq;
      const int64_t po = cell_item(a, i, c4, g, cq);
      const f32x4 xh = (ld4(x + (p0 + po) * a.ldx + cq * 4) - mu) * rs;
      const f32x4 gv = ld4(dy + (p0 + po) * a.ldy + cq * 4) * ld4(weight + g * a.Cmax + cq * 4);
      f32x4 v = (gv - mg - xh * mgx) * rs;
      float* p = dx + (p0 + po) * a.ldx + cq * 4;
      if (accumulate) v += ld4(p);
      st4(p, v);
    }
  }
}

constexpr int kCellRun = 64;   // cells per run of the parameter-gradient partials
// one thread per (run, phase, channel): part[run][0][g * C + c] = sum dy * xhat, part[run][1][..] = sum dy,
// over the run's cells in cell order
__global__ __launch_bounds__(256) void cell_ln_param_partial_kernel(const CellArgs a, const float* __restrict__ x,
                                                                    const float* __restrict__ dy,
                                                                    const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd,
                                                                    float* __restrict__ part, const int64_t items) {
  const int n = 4 * a.C;
  for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (int64_t)gridDim.x * 256) {
    const int gc = (int)(it % n);
    const int64_t run = it / n;
    const int g = gc / a.C, c = gc - g * a.C;
    const int64_t po = (int64_t)(g & 1) * a.W + (g >> 1);
    const int64_t c0 = run * kCellRun, c1 = c0 + kCellRun < a.cells ? c0 + kCellRun : a.cells;
    float sw = 0.f, sb = 0.f;
    for (int64_t cell = c0; cell < c1; ++cell) {
      const int64_t p = cell_pixel(a, cell) + po;
      const float d = dy[p * a.ldy + c];
      sw = fmaf(d, (x[p * a.ldx + c] - mean[cell]) * rstd[cell], sw);
      sb += d;
    }
    part[run * 2 * n + gc] = sw;
    part[run * 2 * n + n + gc] = sb;
  }
}
// dweight[g * Cmax + c], dbias[g * Cmax + c] = the runs' partials in run order
__global__ __launch_bounds__(256) void cell_ln_param_sum_kernel(const float* __restrict__ part,
                                                                float* __restrict__ dweight,
                                                                float* __restrict__ dbias, const int64_t runs,
                                                                const int C, const int Cmax) {
  const int n = 4 * C;
  const int gc = blockIdx.x * 256 + threadIdx.x;
  if (gc >= n) return;
  float sw = 0.f, sb = 0.f;
  for (int64_t r = 0; r < runs; ++r) {
    sw += part[r * 2 * n + gc];
    sb += part[r * 2 * n + n + gc];
  }
  const int g = gc / C, c = gc - g * C;
  dweight[g * Cmax + c] = sw;
  dbias[g * Cmax + c] = sb;
}

int cell_check(const gs_cell_layernorm_desc* d) {
  if (!d) return GS_E_NULL;
  if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->C <= 0 || d->Cmax < d->C || !(d->eps > 0.f)) return GS_E_BADARG;
  if (d->H % 2 || d->W % 2 || (int64_t)d->B * d->H * d->W > INT32_MAX) return GS_E_BADARG;
  if (d->C % 4 || d->Cmax % 4 || d->ldx % 4 || d->ldy % 4) return GS_E_ALIGN;
  if (d->ldx < d->C || d->ldy < d->C) return GS_E_BADARG;
  return GS_OK;
}
CellArgs cell_args(const gs_cell_layernorm_desc* d) {
  CellArgs a;
  a.cells = (int64_t)d->B * (d->H / 2) * (d->W / 2);
  a.H = d->H; a.W = d->W; a.C = d->C; a.Cmax = d->Cmax; a.ldx = d->ldx; a.ldy = d->ldy;
  a.eps = d->eps;
  return a;
}
inline int64_t cell_runs(const gs_cell_layernorm_desc* d) {
  return ceil_div((int64_t)d->B * (d->H / 2) * (d->W / 2), kCellRun);
}

}  // namespace
}  // namespace gs

using namespace gs;

extern "C" int gs_debug_set_window_attention_split(int32_t S) {
  if (S != -1 && S < 1) return GS_E_BADARG;
  g_win_split = S;
  return GS_OK;
}

extern "C" size_t gs_window_attention_workspace_bytes(const gs_window_attention_desc* d) {
  if (win_check(d) != GS_OK) return 0;
  return win_ws_bytes(d, win_split(d, g_win_split));
}

extern "C" int gs_window_attention_forward(const gs_window_attention_desc* d, const float* q, const float* k,
                                           const float* v, const float* table, float* o, float* lse,
                                           void* stream) {
  const int rc = win_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({q, k, v, table, o, lse})) return GS_E_NULL;
  if (!all_aligned16({q, k, v, o, lse}) || (reinterpret_cast<uintptr_t>(table) & 3u)) return GS_E_ALIGN;
  const WinArgs a = win_args(d, 0);
  hipLaunchKernelGGL(win_forward_kernel, dim3((unsigned)a.nw, (unsigned)d->heads, (unsigned)d->B), dim3(64), 0,
                     as_stream(stream), a, q, k, v, table, o, lse);
  return launch_status();
}

extern "C" int gs_window_attention_backward(const gs_window_attention_desc* d, const float* q, const float* k,
                                            const float* v, const float* table, const float* o, const float* lse,
                                            const float* d_o, float* dq, float* dk, float* dv, float* dtable,
                                            int accumulate, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  const int rc = win_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({q, k, v, table, o, lse, d_o, dq, dk, dv, dtable, workspace})) return GS_E_NULL;
  if (!all_aligned16({q, k, v, o, lse, d_o, dq, dk, dv, workspace}) ||
      (reinterpret_cast<uintptr_t>(table) & 3u) || (reinterpret_cast<uintptr_t>(dtable) & 3u))
    return GS_E_ALIGN;
  const WinSplit sp = win_split(d, g_win_split);
  if (workspace_bytes < win_ws_bytes(d, sp)) return GS_E_WORKSPACE;
  const WinArgs a = win_args(d, accumulate);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(win_backward_kernel, dim3((unsigned)sp.slabs, (unsigned)d->heads), dim3(64), 0,
                     as_stream(stream), a, q, k, v, table, o, lse, d_o, dq, dk, dv, part, sp.per,
                     (int64_t)d->B * a.nw);
  hipLaunchKernelGGL(win_table_combine_kernel, dim3((unsigned)ceil_div((int64_t)d->heads * a.R, 256)), dim3(256),
                     0, as_stream(stream), part, dtable, (int)sp.slabs, (int)d->heads, (int)a.R,
                     (int)d->ld_table, a.accumulate);
  return launch_status();
}

extern "C" int gs_map_pad(const float* src, int32_t lds, float* dst, int32_t ldd, int32_t B, int32_t H,
                          int32_t W, int32_t Hp, int32_t Wp, int32_t C, int accumulate, void* stream) {
  const int rc = map_check(B, H, W, Hp, Wp, C, lds, ldd);
  if (rc != GS_OK) return rc;
  if (!src || !dst) return GS_E_NULL;
  if (!aligned16(src) || !aligned16(dst)) return GS_E_ALIGN;
  const int64_t items = (int64_t)B * Hp * Wp * (C / 4);
  hipLaunchKernelGGL(map_pad_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream), src, dst,
                     items, H, W, Hp, Wp, C / 4, lds, ldd, accumulate ? 1 : 0);
  return launch_status();
}

extern "C" int gs_map_crop(const float* src, int32_t lds, float* dst, int32_t ldd, int32_t B, int32_t H,
                           int32_t W, int32_t Hp, int32_t Wp, int32_t C, int accumulate, void* stream) {
  const int rc = map_check(B, H, W, Hp, Wp, C, ldd, lds);
  if (rc != GS_OK) return rc;
  if (!src || !dst) return GS_E_NULL;
  if (!aligned16(src) || !aligned16(dst)) return GS_E_ALIGN;
  const int64_t items = (int64_t)B * H * W * (C / 4);
  hipLaunchKernelGGL(map_crop_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream), src, dst,
                     items, H, W, Hp, Wp, C / 4, lds, ldd, accumulate ? 1 : 0);
  return launch_status();
}

extern "C" int gs_cell_layernorm_forward(const gs_cell_layernorm_desc* d, const float* x, const float* weight,
                                         const float* bias, float* y, float* mean, float* rstd, void* stream) {
  const int rc = cell_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({x, weight, bias, y, mean, rstd})) return GS_E_NULL;
  if (!all_aligned16({x, weight, bias, y})) return GS_E_ALIGN;
  const CellArgs a = cell_args(d);
  hipLaunchKernelGGL(cell_ln_forward_kernel, dim3(stream_grid(a.cells * 64, 256)), dim3(256), 0,
                     as_stream(stream), a, x, weight, bias, y, mean, rstd);
  return launch_status();
}

extern "C" size_t gs_cell_layernorm_workspace_bytes(const gs_cell_layernorm_desc* d) {
  if (cell_check(d) != GS_OK) return 0;
  return (size_t)cell_runs(d) * 2 * 4 * d->C * sizeof(float);
}

extern "C" int gs_cell_layernorm_backward(const gs_cell_layernorm_desc* d, const float* x, const float* dy,
                                          const float* weight, const float* mean, const float* rstd, float* dx,
                                          float* dweight, float* dbias, int accumulate, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  const int rc = cell_check(d);
  if (rc != GS_OK) return rc;
  if (any_null({x, dy, weight, mean, rstd, dx, dweight, dbias, workspace})) return GS_E_NULL;
  if (!all_aligned16({x, dy, weight, dx, dweight, dbias, workspace})) return GS_E_ALIGN;
  if (workspace_bytes < gs_cell_layernorm_workspace_bytes(d)) return GS_E_WORKSPACE;
  const CellArgs a = cell_args(d);
  const int64_t runs = cell_runs(d), items = runs * 4 * d->C;
  float* part = static_cast<float*>(workspace);
  // the partials read x and dy before the dx kernel may overwrite dy's buffer
  hipLaunchKernelGGL(cell_ln_param_partial_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, as_stream(stream),
                     a, x, dy, mean, rstd, part, items);
  hipLaunchKernelGGL(cell_ln_param_sum_kernel, dim3((unsigned)ceil_div(4 * (int64_t)d->C, 256)), dim3(256), 0,
                     as_stream(stream), part, dweight, dbias, runs, (int)d->C, (int)d->Cmax);
  hipLaunchKernelGGL(cell_ln_backward_dx_kernel, dim3(stream_grid(a.cells * 64, 256)), dim3(256), 0,
                     as_stream(stream), a, x, dy, weight, mean, rstd, dx, accumulate ? 1 : 0);
  return launch_status();
}
