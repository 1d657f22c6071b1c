// Routing of the dynamic convolution: which kernel family, tile plan and K loop a descriptor takes.
// Host only.  Included by the conv translation units (igemm_fwd.hip, igemm_dgrad.hip, igemm_wgrad.hip);
// it needs the streaming kernel's planner (igemm_stream.h) and the stem's gate (fused_internal.h) on top
// of igemm_core.h.
#pragma once
#include "igemm_core.h"
#include "igemm_stream.h"
#include "fused_internal.h"

namespace gs {

// K loop of a fast row launch (GS_KLOOP_*).  bf16x3 contraction (see PackBf16x3): stride-1 dgrad,
// 64-row tiles, BN 64 / 48.  r02 sweep over the supernet's data-gradient shapes
// (profiles/r02_bf16x3_probe.md): +7.5 % in sum against the fp32 loop, ahead everywhere except short
// split-K ranges (a split's 16 K steps are 8 bf16 steps: the fill does not amortise) and
// one-workgroup-per-CU launches (its single LDS stage wants co-resident workgroups to hide the two
// barriers per step: s3 1x1 256->1024, 30.5 vs 25.6 us), which keep the fp32 loop.  GS_X3=0 switches
// it off, GS_X3=n (n > 1) raises the minimum K steps per workgroup (3 K steps = 2 bf16 steps, a
// quarter wasted: -10 %).  The forward runs on it only behind GS_X3_FWD=<min K steps> (the [k][n]
// weights are staged with eight dword loads per thread and step: level with the fp32 loop).
// Long K ranges otherwise run two K steps per barrier (pipelined_k_loop_pairs) when the launch has at
// most three workgroups per CU anyway (its four LDS stages allow no more); big grids and short K
// ranges keep the two-stage loop, whose smaller footprint lets five workgroups per CU overlap their
// fill / drain (r01 A/B: s2..s4 3x3 and the head convs +3..7 %, s1 3x3 -3 % if paired).
// forward on the bf16x3 loop: 0 = never, 1 = every 3x3 where it measured ahead of the fp32 loops, 2 =
// wherever the loop's gate admits it (tests, sweeps), 3 = the split-K 3x3s only (DEFAULT); GS_X3_FWD
// sets the initial value, gs_debug_set_x3_fwd changes it at run time.
// Why not everywhere it is faster (K3 +9 % at stage 1): the bf16x3 contraction is ~1.3-1.5x noisier
// than the exact fmaf chain of the fp32 MFMA (the bf16 MFMA's internal accumulation: see PackBf16x3) and
// forward noise is amplified by every layer behind it.  With mode 1 the median error ratio of the
// ill-conditioned parameter gradients against the fp32 oracle rose from 1.15 to 1.53 on config 4
// (bound 1.5, tests/parity.py) and three parameters of config 3 left the 3x bound.  Mode 3 keeps the
// early layers on the fp32 MFMA and takes the loop only where a 3x3 is split along K -- stages 3-4 at
// bs 2 and the heads' big-K convs, +3..5 % per launch: the margins of the full-size tests do not move
// (config 4 median 1.13 vs 1.15, config 3 p90 1.72 vs 1.70, largest ratio 2.06 both), K3 on the
// sampled mix 0.541 -> 0.551 of the fp32 peak, the step +0.65 % (A/B/A/B on one box).
extern int g_x3_fwd;   // capi_misc.hip (-1 = not yet read from the environment)
static inline int x3_fwd_mode() {
  if (g_x3_fwd < 0) g_x3_fwd = env_int("GS_X3_FWD", 3);
  return g_x3_fwd;
}
static inline bool pair_loop_ok(const Plan& pl) {
  return pl.nk_per_split >= pair_min_ksteps() &&
         (long)pl.tiles_m * pl.tiles_n * pl.splits <= 3L * num_cu();
}
static inline bool x3_grid_ok(const Plan& pl, int min_ksteps_) {
  // (r03 A/B: 32 instead of 48 puts the MIN anchor's split-K launches on the loop as well -- MIN +1 %,
  // sampled mix +-0; kept at 48)
  static const int split_min = env_int("GS_X3_SPLIT_MIN", 48);
  return min_ksteps_ > 0 && pl.bm == 64 && pl.nk_per_split >= min_ksteps_ &&
         (pl.splits == 1 || pl.nk_per_split >= split_min) &&
         (long)pl.tiles_m * pl.tiles_n * pl.splits >= 2L * num_cu();
}
// Forward precision (gs_set_forward_precision, inference): 0 = fp32 (default), 1 = fp16 operands.
// Training precision (gs_set_train_precision): 1 = the forward launches of the fp16 inference mode
// AND the fast data-gradient launches contract fp16 operands; weight gradients stay fp32.
extern int g_fwd_precision;     // capi_misc.hip
extern int g_train_precision;   // capi_misc.hip
static inline bool f16_train_on() { return g_train_precision == 1; }
static inline bool f16_fwd_on() { return g_fwd_precision == 1 || f16_train_on(); }
// The f16 loop's tiles: 64 rows, BN 64 or 48 (f16_narrow turns the planner's 80 / 32 into them).
static inline bool f16_plan_ok(const Plan& pl) { return pl.bm == 64 && (pl.bn == 64 || pl.bn == 48); }
// A fast data-gradient launch of this plan runs on the f16 loop in training fp16 mode: the tiles the
// bf16x3 data-gradient gate admits, without its grid-size condition (as the f16 forward).
// (profiles/r05_fp16_training.md: per shape class against the fp32 loops, kernels alone)
static inline bool f16_dgrad_ok(const Plan& pl) { return f16_train_on() && f16_plan_ok(pl); }
template <bool BTRANS>
static inline int rows_fast_kloop(const Plan& pl, bool in_affine, int ks = 3) {
  // fp16 mode: every fast forward launch on a 64-row tile, in_affine included;
  // training fp16 mode: the fast data gradients as well (section 17)
  if (!BTRANS && f16_fwd_on() && f16_plan_ok(pl)) return GS_KLOOP_F16;
  if (BTRANS && f16_dgrad_ok(pl)) return GS_KLOOP_F16;
  if constexpr (BTRANS) {
    static const int x3_min = env_int("GS_X3", 4);
    if (x3_grid_ok(pl, x3_min) && (pl.bn == 64 || pl.bn == 48)) return GS_KLOOP_BF16X3;
  } else {
    // Forward (r03: the [k][n] weights staged one k row per thread and step, packed_k_loop<BFWD>).
    // Per shape against the fp32 loops, kernels alone (profiles/r03_fwd_x3_per_shape.md): 3x3 at
    // stage 1 +9 % (one K step per barrier there), the split-K 3x3s of stages 3-4 +3..5 %, the
    // unsplit 3x3 of stage 2 -4 % (the two-steps-per-barrier fp32 loop wins), 1x1s -10..+8 %
    // without a pattern.  Production: 3x3 only, and not where the paired fp32 loop runs unsplit.
    const int mode = x3_fwd_mode();
    if (mode > 0 && !in_affine && x3_grid_ok(pl, 4) && (pl.bn == 64 || pl.bn == 48)) {
      if (mode == 2) return GS_KLOOP_BF16X3;
      if (mode == 3) {   // only the split-K 3x3s (stages 3-4: late layers, the least amplification)
        if (ks == 3 && pl.splits > 1) return GS_KLOOP_BF16X3;
      } else if (ks == 3 && !(pair_loop_ok(pl) && pl.splits == 1)) {
        return GS_KLOOP_BF16X3;
      }
    }
  }
  return pair_loop_ok(pl) ? GS_KLOOP_FP32_PAIRS : GS_KLOOP_FP32;
}

// ------------------------------------------------------------------------------------------
// Routes: which kernel family, plan and K loop a checked descriptor takes, per op.  The entry points
// (gs_conv2d_forward / _dgrad / _wgrad and the fused layers), the workspace queries,
// gs_conv2d_in_affine_supported and gs_debug_query_conv_launch all read the SAME route; the entry
// points keep only what is theirs (IgemmArgs, tickets, epilogue wiring, the reduce launch).
// ------------------------------------------------------------------------------------------
enum ConvPath {
  PATH_STEM,             // stem.hip: the 7x7 stride-2 conv of the NCHW image (forward, weight gradient)
  PATH_STREAM,           // igemm_stream.h: short-K 1x1 over many rows (forward, data gradient)
  PATH_FAST_ROWS,        // igemm_rows_fast_kernel (forward, stride-1 data gradient)
  PATH_GENERIC_ROWS,     // igemm_rows_kernel
  PATH_STRIDED_CLASSES,  // strided data gradient: one fast row launch per input-pixel parity class
  PATH_FAST_WGRAD,       // igemm_wgrad_fast_kernel
  PATH_GENERIC_WGRAD     // igemm_wgrad_kernel
};

// the few call-time facts outside the descriptor that change a route
struct RouteHints {
  bool bias_or_addend = false;   // forward: the stem and streaming kernels take neither
  long bnbwd_ld = 0;             // dgrad: widest leading dimension of a fused BatchNorm-backward
                                 // request (stream_plan's 32-bit offset test), 0 = none
};

struct ConvRoute {
  int path;                 // ConvPath
  Plan plan;                // tile plan of the op's GEMM (PATH_STRIDED_CLASSES: of class (0, 0))
  Plan shown;               // what gs_debug_launch reports: `plan`, or the stem / stream tiling
  int kloop;                // GS_KLOOP_*
  int ks;                   // kernel-size tag: 1, 3, or 0 (anything else)
  bool vec;                 // x is an NHWC source readable as float4
  bool fast;                // the operands meet the fast kernels' conditions (also on PATH_STREAM)
  bool aff;                 // in_affine is evaluated in the loaders
  size_t src_bytes, dense_bytes;   // extents of the gathered / dense operand
  size_t need;              // split-K slab bytes of `plan` (classes: the largest class)
  size_t reserve;           // what gs_conv2d_workspace_bytes reserves for this op
  bool combine;             // split-K slabs may be combined inside the launch (splitk_publish)
  StreamPlan stream;        // PATH_STREAM
};

static inline int ksize_tag(const gs_conv_desc* d) {
  if (d->KH == 1 && d->KW == 1) return 1;
  if (d->KH == 3 && d->KW == 3) return 3;
  return 0;
}
static bool x_is_vector(const gs_conv_desc* d) {
  return d->x_sc == 1 && (d->Ci & 3) == 0 && (d->x_sw & 3) == 0 && (d->x_sh & 3) == 0 &&
         (d->x_sn & 3) == 0;
}
static inline size_t x_bytes(const gs_conv_desc* d) { return (size_t)d->N * d->x_sn * sizeof(float); }
static inline size_t dy_bytes(const gs_conv_desc* d) {
  return (size_t)d->N * d->Ho * d->Wo * d->ldy * sizeof(float);
}
static inline size_t w_bytes(const gs_conv_desc* d) {
  return (size_t)d->KH * d->KW * d->Ci_max * d->Co_ld * sizeof(float);
}
// GS_NO_FAST (set before the process starts) keeps every conv on the generic kernels
static inline bool no_fast() { static const bool v = getenv("GS_NO_FAST") != nullptr; return v; }
// the fast row kernel needs: channels per tap % BK == 0, 1x1 or 3x3, operands within the 31-bit
// offsets of its buffer loads (and, forward, an NHWC vector source: the caller's test)
static inline bool fast_rows_ok(int cs, int ks, size_t src_bytes, size_t dense_bytes) {
  return !no_fast() && (ks == 1 || ks == 3) && (cs % BK) == 0 && src_bytes < (1ull << 31) &&
         dense_bytes < (1ull << 31);
}
// The in-launch combine addresses the slabs with 32-bit byte offsets.  The planner never exceeds
// kMaxSlabBytes; a forced plan (gs_debug_force_plan) may, and then keeps the separate reduce launch.
static_assert(kMaxSlabBytes < (1ull << 32), "planned slabs fit the combine's 32-bit offsets");
static inline bool combine_ok(const Plan& pl, size_t need) {
  return splitk_combine_ok(pl) && need < (1ull << 32);
}
// the f16 loop's tiles for a fast launch whose planner tile is 64 x 80 / 64 x 32: 64 / 48 columns, the
// split-K factor (hence the workspace) unchanged
static inline Plan f16_narrow(Plan pl, int Nn) {
  if (pl.bm == 64 && (pl.bn == 80 || pl.bn == 32) && g_force_plan[0] == 0) {
    pl.bn = pl.bn == 80 ? 64 : 48;
    pl.tiles_n = (int)ceil_div(Nn, pl.bn);
  }
  return pl;
}

static inline ConvRoute route_forward(const gs_conv_desc* d, const RouteHints& h = RouteHints{}) {
  ConvRoute r{};
  const long M = (long)d->N * d->Ho * d->Wo;
  r.ks = ksize_tag(d);
  r.vec = x_is_vector(d);
  r.aff = d->in_affine != nullptr;
  r.src_bytes = x_bytes(d);
  r.dense_bytes = w_bytes(d);
  r.fast = r.vec && fast_rows_ok(d->Ci, r.ks, r.src_bytes, r.dense_bytes);
  r.plan = make_plan((int)M, d->Co, d->KH * d->KW * d->Ci, true);
  if (r.fast && f16_fwd_on()) r.plan = f16_narrow(r.plan, d->Co);
  r.shown = r.plan;
  r.need = r.reserve = slab_bytes(r.plan, M, d->Co);
  r.kloop = GS_KLOOP_GENERIC;
  r.path = PATH_GENERIC_ROWS;
  if (!r.vec && !h.bias_or_addend && stem_conv_ok(d)) {   // 128-row tiles, its own loop
    r.path = PATH_STEM;
    r.aff = false;
    r.shown = Plan{128, d->Co, 1, 37, 37, d->N * d->Ho * (d->Wo / 128), 1};
    return r;
  }
  if (!r.fast) return r;
  r.path = PATH_FAST_ROWS;
  r.kloop = rows_fast_kloop<false>(r.plan, r.aff, r.ks);
  r.combine = combine_ok(r.plan, r.need);
  // the streaming 1x1 kernel: 1x1, stride 1, no padding, contiguous pixel rows, no bias / addend, and
  // stream_plan() finds a column-block width whose weights fit in LDS
  if (!h.bias_or_addend && r.ks == 1 && d->stride == 1 && d->pad == 0 &&
      d->x_sh == (int64_t)d->W * d->x_sw && d->x_sn == (int64_t)d->H * d->x_sh &&
      !(d->in_affine && d->Ci > 256))
    r.stream = stream_plan(M, d->Co, d->Ci, false, d->ldy);
  if (r.stream.ok) {
    r.path = PATH_STREAM;
    r.kloop = GS_KLOOP_STREAM;
    r.combine = false;
    const int nk = (int)ceil_div(d->Ci, BK);
    r.shown = Plan{kStreamBM, r.stream.bnw, 1, nk, nk, r.stream.row_groups, r.stream.ncb};
  }
  return r;
}

// ---- strided dgrad as s*s stride-1 sub-problems (one per input-pixel parity class) ----
// For input row h = hq*s + ph the taps kh with (ph + pad - kh*dil) % s == 0 contribute, reading
// dy row hq + (ph + pad - kh*dil)/s.  Those taps form an arithmetic progression, so each class is
// an ordinary gather-GEMM over a sub-sampled tap grid: no MFMA work is spent on structural zeros
// (the single-launch form wastes 1 - 1/s^2 of it).
struct TapAxis {
  int n;      // number of valid taps
  int k0;     // first valid tap
  int dk;     // tap step
  int off0;   // source offset of the first valid tap
  int step;   // source offset step per valid tap
};
static inline TapAxis tap_axis(int ph, int pad, int dil, int s, int K) {
  TapAxis a{0, 0, 1, 0, 0};
  int first = -1, second = -1;
  for (int k = 0; k < K; ++k) {
    const int num = ph + pad - k * dil;
    if (((num % s) + s) % s == 0) {
      if (first < 0) first = k;
      else if (second < 0) second = k;
      ++a.n;
    }
  }
  if (a.n == 0) return a;
  a.k0 = first;
  a.dk = second > 0 ? second - first : 1;
  a.off0 = (ph + pad - first * dil) / s;          // exact division
  a.step = -(a.dk * dil) / s;
  return a;
}
static inline int class_len(int L, int s, int ph) { return L > ph ? (L - ph + s - 1) / s : 0; }

// one parity class of a strided data gradient as a fast row launch
struct DgradClass {
  int ph, pw, Hq, Wq;
  TapAxis th, tw;
  long M;             // N * Hq * Wq rows
  int ktot;           // taps of the class * Co
  Plan plan;
  int kloop;
  size_t need;
  bool combine;
};
static inline DgradClass dgrad_class(const gs_conv_desc* d, int ph, int pw, int min_taps = 0) {
  DgradClass c{};
  const int s = d->stride;
  c.ph = ph; c.pw = pw;
  c.th = tap_axis(ph, d->pad, d->dil, s, d->KH);
  c.tw = tap_axis(pw, d->pad, d->dil, s, d->KW);
  c.Hq = class_len(d->H, s, ph);
  c.Wq = class_len(d->W, s, pw);
  c.M = (long)d->N * c.Hq * c.Wq;
  c.ktot = std::max(min_taps, c.th.n * c.tw.n) * d->Co;
  if (c.M == 0 || c.ktot == 0) return c;
  c.plan = make_plan((int)c.M, d->Ci, c.ktot, true);
  if (f16_train_on()) c.plan = f16_narrow(c.plan, d->Ci);
  c.kloop = rows_fast_kloop<true>(c.plan, false);
  c.need = slab_bytes(c.plan, c.M, d->Ci);
  c.combine = combine_ok(c.plan, c.need);
  return c;
}
// f(class) for every class that has taps and pixels
template <class F>
static inline void for_each_dgrad_class(const gs_conv_desc* d, F&& f) {
  for (int ph = 0; ph < d->stride; ++ph)
    for (int pw = 0; pw < d->stride; ++pw) {
      const DgradClass c = dgrad_class(d, ph, pw);
      if (c.M != 0 && c.ktot != 0) f(c);
    }
}
// some class has no tap at all (e.g. 3 of the 4 classes of a 1x1 stride-2 conv): its pixels stay zero
static inline bool dgrad_has_tapless_class(const gs_conv_desc* d) {
  for (int p = 0; p < d->stride; ++p)
    if (!tap_axis(p, d->pad, d->dil, d->stride, d->KH).n || !tap_axis(p, d->pad, d->dil, d->stride, d->KW).n)
      return true;
  return false;
}

static inline ConvRoute route_dgrad(const gs_conv_desc* d, const RouteHints& h = RouteHints{}) {
  ConvRoute r{};
  const long M = (long)d->N * d->H * d->W;
  r.ks = ksize_tag(d);
  r.vec = x_is_vector(d);
  r.src_bytes = dy_bytes(d);
  r.dense_bytes = w_bytes(d);
  r.fast = fast_rows_ok(d->Co, r.ks, r.src_bytes, r.dense_bytes);
  r.plan = make_plan((int)M, d->Ci, d->KH * d->KW * d->Co, true);
  if (r.fast && d->stride == 1 && f16_train_on()) r.plan = f16_narrow(r.plan, d->Ci);
  r.shown = r.plan;
  r.need = r.reserve = slab_bytes(r.plan, M, d->Ci);
  r.kloop = GS_KLOOP_GENERIC;
  r.path = PATH_GENERIC_ROWS;
  if (d->stride > 1) {
    // (the workspace query covers both forms of a strided data gradient, whichever runs)
    size_t classes = 0;
    for_each_dgrad_class(d, [&](const DgradClass& c) { classes = std::max(classes, c.need); });
    r.reserve = std::max(r.reserve, classes);
    if (r.fast && M * d->x_sw < (1L << 31)) {
      const DgradClass c0 = dgrad_class(d, 0, 0, 1);
      r.path = PATH_STRIDED_CLASSES;
      r.plan = r.shown = c0.plan;
      r.kloop = c0.kloop;
      r.need = classes;
    }
    return r;
  }
  if (!r.fast) return r;
  r.path = PATH_FAST_ROWS;
  r.kloop = rows_fast_kloop<true>(r.plan, false);
  r.combine = combine_ok(r.plan, r.need);
  // short-K 1x1 data gradients over many rows: the streaming kernel.  (A padded 1x1 has Ho = H + 2 pad:
  // the streaming kernel maps dy row m to dx row m, so it takes only the unpadded form; the tile
  // kernels handle padding through base_h / base_w.)
  if (r.ks == 1 && d->pad == 0 && d->H == d->Ho && d->W == d->Wo && d->x_sc == 1)
    r.stream = stream_plan(M, d->Ci, d->Co, true, std::max<long>(d->x_sw, h.bnbwd_ld));
  if (r.stream.ok) {
    r.path = PATH_STREAM;
    r.kloop = GS_KLOOP_STREAM;
    r.combine = false;
    const int nk = (int)ceil_div(d->Co, BK);
    r.shown = Plan{kStreamBM, r.stream.bnw, 1, nk, nk, r.stream.row_groups, r.stream.ncb};
  }
  return r;
}

static inline ConvRoute route_wgrad(const gs_conv_desc* d, const RouteHints& = RouteHints{}) {
  ConvRoute r{};
  const long M = (long)d->KH * d->KW * d->Ci;
  r.ks = ksize_tag(d);
  r.vec = x_is_vector(d);
  r.aff = d->in_affine != nullptr;
  r.src_bytes = x_bytes(d);
  r.dense_bytes = dy_bytes(d);
  r.fast = r.vec && !no_fast() && r.src_bytes < (1ull << 31) && r.dense_bytes < (1ull << 31);
  // K runs over pixels (up to 131072 at stage 1) while M x N is tiny: allow deep split-K
  static const int old_plan = env_int("GS_WGRAD_OLD_PLAN", 0);
  r.plan = old_plan ? make_plan((int)M, d->Co, d->N * d->Ho * d->Wo, true, 512, false)
                    : make_plan((int)M, d->Co, d->N * d->Ho * d->Wo, true, 512, true, 4.0);
  r.shown = r.plan;
  r.need = slab_bytes(r.plan, M, d->Co);
  r.reserve = std::max(r.need, stem_wgrad_slab_bytes(d));
  r.kloop = GS_KLOOP_GENERIC;
  r.path = PATH_GENERIC_WGRAD;
  if (!r.vec && stem_wgrad_on() && stem_conv_ok(d)) {   // persistent groups of 128-row tiles
    r.path = PATH_STEM;
    r.aff = false;
    const int tiles = d->N * d->Ho * (d->Wo / 128);
    const int groups = (int)(stem_wgrad_slab_bytes(d) / ((size_t)147 * d->Co * sizeof(float)));
    r.shown = Plan{128, d->Co, groups, tiles, (int)ceil_div(tiles, groups), 1, 1};
    return r;
  }
  if (r.fast) {
    r.path = PATH_FAST_WGRAD;
    r.kloop = pair_loop_ok(r.plan) ? GS_KLOOP_FP32_PAIRS : GS_KLOOP_FP32;
  }
  return r;
}

// gs_conv_desc::in_affine (relu(bn(x)) in the operand loaders) needs the fast forward and wgrad
// kernels with 64-row tiles and the coefficient image in LDS
static inline bool conv_in_affine_ok(const gs_conv_desc* d) {
  if (d->Ci > kAffMaxC) return false;
  const ConvRoute f = route_forward(d);
  return f.fast && f.plan.bm == 64 && route_wgrad(d).plan.bm == 64;
}

}  // namespace gs
