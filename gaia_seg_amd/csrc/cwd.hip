// Channel-wise distillation loss (Shu et al., ICCV 2021; mmrazor's ChannelWiseDivergence) — gfx950.
//
// Student logits s and teacher logits t, both [N, C, H, W], P = H * W pixels per class map:
//   phi(x)[n,c,p] = softmax over the PIXELS p of x[n,c,:] / T
//   out[0]        = scale * T^2 * sum_{n,c} KL(phi(t)[n,c] || phi(s)[n,c])
//   ds            = scale * T   * (phi(s) - phi(t))                 (the teacher gets no gradient)
// with the host's scale = weight / (N * C).
//
// Forward, one pass: a column (n, c) is described by five running numbers,
//   m_s, Z_s = sum exp((s - m_s) / T),   m_t, Z_t = sum e_t, e_t = exp((t - m_t) / T),
//   A = sum e_t * (t - s) / T,           KL = A / Z_t + (m_s - m_t) / T + log Z_s - log Z_t,
// and two partial states of one column combine associatively: the larger maxima, Z_s rescaled by
// exp((m_s_old - m_s_new) / T), Z_t and A by exp((m_t_old - m_t_new) / T).  Every logit is read once,
// no [N, C, H, W] temporary exists.  A map is split over several workgroups by pixel range; each
// writes its partial states; a second launch (one wave per column) rescales a column's partials to the
// column's maxima and sums them in double in a fixed order, and stores lse = m / T + log Z of both maps
// for the backward; a third, one workgroup, sums the N * C column losses in double in a fixed order:
// bit-reproducible, no float atomics.
//
// Fast path (channel stride 1; the other strides, the base addresses multiples of 4 floats): a thread
// owns one channel quad of a strided set of pixels and loads float4s, consecutive lanes covering
// consecutive bytes of a pixel; the last, partial quad is loaded by scalars so that the pad columns
// C .. ld-1 are never read.  Any other layout: the same kernel with one channel per thread.
#include <algorithm>
#include "common.h"

namespace gs {

constexpr int CWD_THREADS = 256;
// (both overridable at compile time; GS_HIP_LIB selects another build of the library: tuning only)
#ifndef GS_CWD_MIN_PX
#define GS_CWD_MIN_PX 8
#endif
#ifndef GS_CWD_TARGET_WGS
#define GS_CWD_TARGET_WGS 512
#endif
constexpr int CWD_MIN_PX = GS_CWD_MIN_PX;            // a split leaves every thread at least this many pixels
constexpr int CWD_TARGET_WGS = GS_CWD_TARGET_WGS;    // 256 CUs x 2: splitting stops once the grid is this large
constexpr int CWD_UNROLL = 4;          // pixels whose loads are in flight per thread

struct CwdPlan {
  int vec;        // channels per thread: 4 (fast path) or 1
  int qb;         // channel units (quads or channels) side by side in a workgroup: a power of two <= 64
  int qg;         // unit groups (grid.y)
  int slots;      // pixel slots of a workgroup = CWD_THREADS / qb
  int nparts;     // pixel ranges per column (grid.x)
  long span;      // pixels per range
  int cpad;       // qg * qb * vec: channel pitch of the partial states
};

struct CwdArgs {
  gs_cwd_desc d;
  CwdPlan p;
  long P;
  float invT;
  int s_flat, t_flat;   // rows are contiguous in pixels: offset = p * sw
};

struct CwdState {
  float ms, zs, mt, zt, a;
};

__device__ __forceinline__ CwdState cwd_empty() {
  CwdState z;
  z.ms = -__builtin_huge_valf(); z.zs = 0.f; z.mt = -__builtin_huge_valf(); z.zt = 0.f; z.a = 0.f;
  return z;
}

// one online-softmax step of (m, Z) and of a sum `acc` that carries the same factor; `add` enters acc
// with weight exp((x - m_new) / T).  One exp per step; m = -inf gives e = 0 and Z = 1.
__device__ __forceinline__ void cwd_step(float x, float invT, float& m, float& z, float& acc, float add) {
  const float dlt = (x - m) * invT;
  const float e = expf(-fabsf(dlt));
  if (dlt > 0.f) {
    z = z * e + 1.f;
    acc = acc * e + add;
    m = x;
  } else {
    z += e;
    acc += e * add;
  }
}

__device__ __forceinline__ void cwd_update(CwdState& st, float s, float t, float invT) {
  float unused = 0.f;
  cwd_step(s, invT, st.ms, st.zs, unused, 0.f);
  // (t - s) / T rounded as the final stage rounds (m_s - m_t) / T: a one-pixel map cancels exactly
  cwd_step(t, invT, st.mt, st.zt, st.a, __fmul_rn(__fsub_rn(t, s), invT));
}

// x <- combine(x, y); equal maxima (both -inf included) rescale by exactly 1
__device__ __forceinline__ void cwd_combine(CwdState& x, const CwdState& y, float invT) {
  const float ms = fmaxf(x.ms, y.ms), mt = fmaxf(x.mt, y.mt);
  const float rxs = x.ms == ms ? 1.f : expf((x.ms - ms) * invT);
  const float rys = y.ms == ms ? 1.f : expf((y.ms - ms) * invT);
  const float rxt = x.mt == mt ? 1.f : expf((x.mt - mt) * invT);
  const float ryt = y.mt == mt ? 1.f : expf((y.mt - mt) * invT);
  x.zs = x.zs * rxs + y.zs * rys;
  x.zt = x.zt * rxt + y.zt * ryt;
  x.a = x.a * rxt + y.a * ryt;
  x.ms = ms; x.mt = mt;
}

__device__ __forceinline__ long cwd_px_off(long p, int W, long sh, long sw, int flat) {
  return flat ? p * sw : (p / W) * sh + (p % W) * sw;
}

// V channels of one pixel; channels at and past `nc` (the partial last quad) read as 0
template <int V>
__device__ __forceinline__ void cwd_load(const float* row, int nc, float (&v)[V]) {
  if (V == 4) {
    if (nc >= 4) {
      const float4 q = *reinterpret_cast<const float4*>(row);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) v[j] = j < nc ? row[j] : 0.f;
    }
  } else {
    v[0] = row[0];
  }
}

// grid (nparts, qg, N).  Thread (slot, u): unit u of the group's qb units (V channels each), pixels
// p0 + slot, p0 + slot + slots, ... of the range.  part[n][k][j][cpad]: state component j of range k.
template <int V>
__global__ __launch_bounds__(CWD_THREADS) void cwd_fwd_kernel(const CwdArgs a, const float* __restrict__ s,
                                                              const float* __restrict__ t,
                                                              float* __restrict__ part) {
  __shared__ float red[3][5][V][64];   // waves 1..3, lanes < qb
  const gs_cwd_desc& d = a.d;
  const CwdPlan& pl = a.p;
  const int qb = pl.qb, slots = pl.slots;
  const int u = threadIdx.x % qb, slot = threadIdx.x / qb;
  const int n = blockIdx.z, k = blockIdx.x;
  const int c0 = (blockIdx.y * qb + u) * V;
  const int nc = min(V, d.C - c0);           // <= 0: a unit past the last channel
  const float invT = a.invT;
  const long p0 = (long)k * pl.span, p1 = min(a.P, p0 + pl.span);
  CwdState st[V];
#pragma unroll
  for (int j = 0; j < V; ++j) st[j] = cwd_empty();
  if (nc > 0) {
    const float* sb = s + (long)n * d.s_sn + (long)c0 * d.s_sc;
    const float* tb = t + (long)n * d.t_sn + (long)c0 * d.t_sc;
    for (long p = p0 + slot; p < p1; p += (long)CWD_UNROLL * slots) {
      float vs[CWD_UNROLL][V], vt[CWD_UNROLL][V];
#pragma unroll
      for (int r = 0; r < CWD_UNROLL; ++r) {
        const long q = p + (long)r * slots;
        if (q < p1) {
          cwd_load<V>(sb + cwd_px_off(q, d.W, d.s_sh, d.s_sw, a.s_flat), nc, vs[r]);
          cwd_load<V>(tb + cwd_px_off(q, d.W, d.t_sh, d.t_sw, a.t_flat), nc, vt[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < CWD_UNROLL; ++r) {
        if (p + (long)r * slots < p1) {
#pragma unroll
          for (int j = 0; j < V; ++j) cwd_update(st[j], vs[r][j], vt[r][j], invT);
        }
      }
    }
  }
  // lanes of one wave that share a unit: lane l takes lane l + off, so lanes < qb end with the wave's state
  for (int off = 32; off >= qb; off >>= 1) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      CwdState o;
      o.ms = __shfl_down(st[j].ms, off, 64); o.zs = __shfl_down(st[j].zs, off, 64);
      o.mt = __shfl_down(st[j].mt, off, 64); o.zt = __shfl_down(st[j].zt, off, 64);
      o.a = __shfl_down(st[j].a, off, 64);
      cwd_combine(st[j], o, invT);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave > 0 && lane < qb) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      red[wave - 1][0][j][lane] = st[j].ms; red[wave - 1][1][j][lane] = st[j].zs;
      red[wave - 1][2][j][lane] = st[j].mt; red[wave - 1][3][j][lane] = st[j].zt;
      red[wave - 1][4][j][lane] = st[j].a;
    }
  }
  __syncthreads();
  if (wave == 0 && lane < qb && nc > 0) {
    float* prow = part + ((long)n * pl.nparts + k) * 5 * pl.cpad + c0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      CwdState acc = st[j];
      for (int w = 0; w < 3; ++w) {   // waves in index order
        CwdState o;
        o.ms = red[w][0][j][lane]; o.zs = red[w][1][j][lane]; o.mt = red[w][2][j][lane];
        o.zt = red[w][3][j][lane]; o.a = red[w][4][j][lane];
        cwd_combine(acc, o, invT);
      }
      if (j < nc) {
        prow[0 * pl.cpad + j] = acc.ms; prow[1 * pl.cpad + j] = acc.zs; prow[2 * pl.cpad + j] = acc.mt;
        prow[3 * pl.cpad + j] = acc.zt; prow[4 * pl.cpad + j] = acc.a;
      }
    }
  }
}

// One wave per column (n, c): lane l owns partials l, l + 64, ...  The column's maxima first (exact in
// any order), then every partial rescaled to them and summed in double, lane-local in index order and
// across lanes in wave_sum_d's fixed order; lane 0 stores lse of both maps and the column's loss.
__global__ __launch_bounds__(256) void cwd_cols_kernel(const CwdArgs a, const float* __restrict__ part,
                                                       float* __restrict__ lse_s,
                                                       float* __restrict__ lse_t,
                                                       double* __restrict__ col_loss) {
  const gs_cwd_desc& d = a.d;
  const CwdPlan& pl = a.p;
  const long cols = (long)d.N * d.C;
  const int lane = threadIdx.x & 63;
  const long col = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (col >= cols) return;   // (a whole wave; no barrier follows)
  const int n = (int)(col / d.C), c = (int)(col % d.C);
  const float* pr = part + (long)n * pl.nparts * 5 * pl.cpad + c;
  float ms = -__builtin_huge_valf(), mt = -__builtin_huge_valf();
  for (int k = lane; k < pl.nparts; k += 64) {
    const float* q = pr + (long)k * 5 * pl.cpad;
    ms = fmaxf(ms, q[0]);
    mt = fmaxf(mt, q[2 * pl.cpad]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ms = fmaxf(ms, __shfl_xor(ms, off, 64));
    mt = fmaxf(mt, __shfl_xor(mt, off, 64));
  }
  double zs = 0.0, zt = 0.0, av = 0.0;
  for (int k = lane; k < pl.nparts; k += 64) {
    const float* q = pr + (long)k * 5 * pl.cpad;
    const float mk = q[0], nk = q[2 * pl.cpad];
    const double rs = mk == ms ? 1.0 : (double)expf((mk - ms) * a.invT);
    const double rt = nk == mt ? 1.0 : (double)expf((nk - mt) * a.invT);
    zs += (double)q[pl.cpad] * rs;
    zt += (double)q[3 * pl.cpad] * rt;
    av += (double)q[4 * pl.cpad] * rt;
  }
  zs = wave_sum_d(zs); zt = wave_sum_d(zt); av = wave_sum_d(av);
  if (lane == 0) {
    const double lzs = log(zs), lzt = log(zt);
    // (m_s - m_t) / T rounded exactly as cwd_update rounds (t - s) / T
    const float dm = __fmul_rn(__fsub_rn(ms, mt), a.invT);
    col_loss[col] = av / zt + (double)dm + lzs - lzt;
    lse_s[col] = __fmul_rn(ms, a.invT) + (float)lzs;
    lse_t[col] = __fmul_rn(mt, a.invT) + (float)lzt;
  }
}

// one workgroup: out[0] = float(scale * sum of the column losses), fixed order
__global__ __launch_bounds__(256) void cwd_sum_kernel(const double* __restrict__ col_loss, long cols,
                                                      double scale, float* __restrict__ out) {
  __shared__ double sh[4];
  double l = 0.0;
  for (long i = threadIdx.x; i < cols; i += 256) l += col_loss[i];
  l = wave_sum_d(l);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = l;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)((((sh[0] + sh[1]) + sh[2]) + sh[3]) * scale);
}

// ds[n, y, x, c] = coef * (exp(s / T - lse_s[n, c]) - exp(t / T - lse_t[n, c])), pad columns zeroed.
// V == 4: one channel quad per thread (float4 loads of full quads, one float4 store).
template <int V>
__global__ __launch_bounds__(256) void cwd_bwd_kernel(const CwdArgs a, const float* __restrict__ s,
                                                      const float* __restrict__ t,
                                                      const float* __restrict__ lse_s,
                                                      const float* __restrict__ lse_t, float coef,
                                                      float* __restrict__ ds, int ld) {
  const gs_cwd_desc& d = a.d;
  const int units = ld / V;
  const long total = (long)d.N * a.P * units;
  const float invT = a.invT;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(i % units) * V;
    const long px = i / units;
    const long p = px % a.P;
    const int n = (int)(px / a.P);
    const int nc = min(V, d.C - c0);
    float g[V];
#pragma unroll
    for (int j = 0; j < V; ++j) g[j] = 0.f;
    if (nc > 0) {
      float vs[V], vt[V];
      cwd_load<V>(s + (long)n * d.s_sn + (long)c0 * d.s_sc + cwd_px_off(p, d.W, d.s_sh, d.s_sw, a.s_flat),
                  nc, vs);
      cwd_load<V>(t + (long)n * d.t_sn + (long)c0 * d.t_sc + cwd_px_off(p, d.W, d.t_sh, d.t_sw, a.t_flat),
                  nc, vt);
      const float* ls = lse_s + (long)n * d.C + c0;
      const float* lt = lse_t + (long)n * d.C + c0;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (j < nc) {
          // products and differences rounded one by one: equal inputs and equal lse cancel exactly
          const float es = expf(__fsub_rn(__fmul_rn(vs[j], invT), ls[j]));
          const float et = expf(__fsub_rn(__fmul_rn(vt[j], invT), lt[j]));
          g[j] = coef * (es - et);
        }
      }
    }
    if (V == 4) {
      *reinterpret_cast<float4*>(ds + px * ld + c0) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
      ds[px * ld + c0] = g[0];
    }
  }
}

static bool cwd_vec_ok(const float* base, long sn, long sc, long sh, long sw) {
  return sc == 1 && sn % 4 == 0 && sh % 4 == 0 && sw % 4 == 0 && aligned16(base);
}

// The split depends on the descriptor alone (not on the device): results are the same everywhere.
static void cwd_plan(const gs_cwd_desc* d, bool vec, CwdPlan& p) {
  p.vec = vec ? 4 : 1;
  const int units = (int)ceil_div(d->C, p.vec);
  // the width with the fewest idle lanes, the wider one on a tie (longer contiguous runs per pixel)
  int best = 1;
  if (units >= 4) {
    long best_pad = -1;
    for (int qb = 4; qb <= 64; qb *= 2) {
      const long pad = ceil_div(units, qb) * qb;
      if (best_pad < 0 || pad <= best_pad) { best_pad = pad; best = qb; }
    }
  } else {
    while (best < units) best *= 2;
  }
  p.qb = best;
  p.qg = (int)ceil_div(units, p.qb);
  p.slots = CWD_THREADS / p.qb;
  p.cpad = p.qg * p.qb * p.vec;
  const long P = (long)d->H * d->W;
  const long by_work = ceil_div(P, (long)p.slots * CWD_MIN_PX);
  const long by_grid = ceil_div(CWD_TARGET_WGS, (long)d->N * p.qg);
  long parts = by_work < by_grid ? by_work : by_grid;
  if (parts < 1) parts = 1;
  p.span = ceil_div(P, parts);
  p.nparts = (int)ceil_div(P, p.span);
}

static int check_cwd(const gs_cwd_desc* d, CwdArgs& a) {
  if (!d) return GS_E_NULL;
  if (d->N <= 0 || d->C <= 0 || d->H <= 0 || d->W <= 0) return GS_E_BADARG;
  if (d->N > 65535) return GS_E_BADARG;   // grid.z
  if (!(d->T > 0.f) || d->T == __builtin_huge_valf()) return GS_E_BADARG;
  a.d = *d;
  a.P = (long)d->H * d->W;
  a.invT = 1.f / d->T;
  a.s_flat = d->s_sh == (int64_t)d->W * d->s_sw ? 1 : 0;
  a.t_flat = d->t_sh == (int64_t)d->W * d->t_sw ? 1 : 0;
  return GS_OK;
}

// partial states (floats), then one double per column
static size_t cwd_part_bytes(const gs_cwd_desc* d, const CwdPlan& p) {
  return ((size_t)d->N * p.nparts * 5 * p.cpad * sizeof(float) + 7) & ~(size_t)7;
}
static size_t cwd_ws_bytes(const gs_cwd_desc* d, const CwdPlan& p) {
  return cwd_part_bytes(d, p) + (size_t)d->N * d->C * sizeof(double);
}

}  // namespace gs

using namespace gs;

// The workspace is sized for the scalar layout's plan when it is the larger one, so that one query
// serves whatever the alignment of the pointers turns out to be.
extern "C" size_t gs_cwd_workspace_bytes(const gs_cwd_desc* d) {
  CwdArgs a;
  if (check_cwd(d, a)) return 0;
  CwdPlan pv, ps;
  cwd_plan(d, true, pv);
  cwd_plan(d, false, ps);
  return std::max(cwd_ws_bytes(d, pv), cwd_ws_bytes(d, ps));
}

// Pixel ranges per column for this descriptor's strides (base addresses taken as 16-byte aligned).
extern "C" int gs_cwd_debug_partials(const gs_cwd_desc* d) {
  CwdArgs a;
  const int rc = check_cwd(d, a);
  if (rc) return rc;
  const bool vec = cwd_vec_ok(nullptr, d->s_sn, d->s_sc, d->s_sh, d->s_sw) &&
                   cwd_vec_ok(nullptr, d->t_sn, d->t_sc, d->t_sh, d->t_sw);
  cwd_plan(d, vec, a.p);
  return a.p.nparts;
}

extern "C" int gs_cwd_forward(const gs_cwd_desc* d, const float* student, const float* teacher,
                              float* lse_s, float* lse_t, float scale, float* out, void* workspace,
                              size_t workspace_bytes, void* stream) {
  CwdArgs a;
  const int rc = check_cwd(d, a);
  if (rc) return rc;
  if (!student || !teacher || !lse_s || !lse_t || !out || !workspace) return GS_E_NULL;
  const bool vec = cwd_vec_ok(student, d->s_sn, d->s_sc, d->s_sh, d->s_sw) &&
                   cwd_vec_ok(teacher, d->t_sn, d->t_sc, d->t_sh, d->t_sw);
  cwd_plan(d, vec, a.p);
  if (cwd_ws_bytes(d, a.p) > workspace_bytes) return GS_E_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return GS_E_ALIGN;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  double* col_loss = reinterpret_cast<double*>(static_cast<char*>(workspace) + cwd_part_bytes(d, a.p));
  const long cols = (long)d->N * d->C;
  const dim3 grid((unsigned)a.p.nparts, (unsigned)a.p.qg, (unsigned)d->N);
  if (vec)
    hipLaunchKernelGGL(cwd_fwd_kernel<4>, grid, dim3(CWD_THREADS), 0, st, a, student, teacher, part);
  else
    hipLaunchKernelGGL(cwd_fwd_kernel<1>, grid, dim3(CWD_THREADS), 0, st, a, student, teacher, part);
  hipLaunchKernelGGL(cwd_cols_kernel, dim3((unsigned)ceil_div(cols, 4)), dim3(256), 0, st, a, part, lse_s,
                     lse_t, col_loss);
  hipLaunchKernelGGL(cwd_sum_kernel, dim3(1), dim3(256), 0, st, col_loss, cols,
                     (double)scale * (double)d->T * (double)d->T, out);
  return launch_status();
}

extern "C" int gs_cwd_backward(const gs_cwd_desc* d, const float* student, const float* teacher,
                               const float* lse_s, const float* lse_t, float scale, float* ds,
                               int32_t ld_d, void* stream) {
  CwdArgs a;
  const int rc = check_cwd(d, a);
  if (rc) return rc;
  if (!student || !teacher || !lse_s || !lse_t || !ds) return GS_E_NULL;
  if (ld_d < d->C) return GS_E_BADARG;
  const bool vec = ld_d % 4 == 0 && aligned16(ds) &&
                   cwd_vec_ok(student, d->s_sn, d->s_sc, d->s_sh, d->s_sw) &&
                   cwd_vec_ok(teacher, d->t_sn, d->t_sc, d->t_sh, d->t_sw);
  a.p = CwdPlan();
  hipStream_t st = as_stream(stream);
  const float coef = scale * d->T;
  const long total = (long)d->N * a.P * (vec ? ld_d / 4 : ld_d);
  const dim3 grid(stream_grid(total, 256));
  if (vec)
    hipLaunchKernelGGL(cwd_bwd_kernel<4>, grid, dim3(256), 0, st, a, student, teacher, lse_s, lse_t, coef,
                       ds, ld_d);
  else
    hipLaunchKernelGGL(cwd_bwd_kernel<1>, grid, dim3(256), 0, st, a, student, teacher, lse_s, lse_t, coef,
                       ds, ld_d);
  return launch_status();
}
