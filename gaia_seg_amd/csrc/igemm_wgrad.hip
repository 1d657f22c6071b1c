// DynConv2d weight gradient (implicit GEMM over pixels, split-K) — see igemm_core.h
#include "igemm_route.h"

using namespace gs;

extern "C" int gs_conv2d_wgrad(const gs_conv_desc* d, const float* x, const float* dy, float* dw,
                               void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_desc(d);
  if (rc != GS_OK) return rc;
  if (!x || !dy || !dw) return GS_E_NULL;
  if (!aligned16(dy) || !aligned16(dw)) return GS_E_ALIGN;
  const ConvRoute r = route_wgrad(d);
  const bool vec = r.vec, fast = r.fast;
  if (vec && !aligned16(x)) return GS_E_ALIGN;
  if (r.path == PATH_STEM)   // the stem: stem.hip
    return stem_wgrad(d, x, dy, dw, workspace, workspace_bytes, as_stream(stream));
  const Plan& pl = r.plan;
  const long M = (long)d->KH * d->KW * d->Ci;
  const size_t need = r.need;
  if (need > workspace_bytes || (need && !workspace)) return GS_E_WORKSPACE;

  IgemmArgs a{};
  a.src = x; a.dense = dy; a.out = dw; a.slab = need ? static_cast<float*>(workspace) : nullptr;
  a.s_n = d->x_sn; a.s_h = d->x_sh; a.s_w = d->x_sw; a.s_c = d->x_sc;
  a.Hs = d->H; a.Ws = d->W; a.Cs = d->Ci;
  a.Hp = d->Ho; a.Wp = d->Wo; a.npix = d->N * d->Ho * d->Wo;
  a.KW = d->KW; a.taps = d->KH * d->KW;
  a.mul_h = a.mul_w = d->stride; a.base_h = a.base_w = -d->pad;
  a.step_h = a.step_w = d->dil; a.div_h = a.div_w = 1;
  a.d_tap = 0; a.d_row = d->ldy; a.n_lim = d->Co;
  a.M = (int)M; a.Nn = d->Co; a.Ktot = a.npix;
  a.o_tap = (long)d->Ci_max * d->Co_ld; a.o_row = d->Co_ld;
  a.nk_total = pl.nk_total; a.nk_per_split = pl.nk_per_split;
  a.tiles_m = pl.tiles_m; a.tiles_n = pl.tiles_n;
  hipStream_t st = as_stream(stream);
  const int ks = r.ks;
  a.src_bytes = (unsigned)r.src_bytes;
  a.dense_bytes = (unsigned)r.dense_bytes;
  if (d->in_affine) {
    if (!conv_in_affine_ok(d) || !fast || pl.bm != 64 || (ks != 1 && ks != 3)) return GS_E_BADARG;
    if (!aligned16(d->in_affine)) return GS_E_ALIGN;
    a.a_coeffs = d->in_affine;
  }
  if (fast && ks == 1) launch_wgrad_fast<1>(pl, r.kloop, a, st);
  else if (fast && ks == 3) launch_wgrad_fast<3>(pl, r.kloop, a, st);
  else if (fast) launch_wgrad_fast<0>(pl, r.kloop, a, st);
  else if (!vec) launch_wgrad<true, 0>(pl, a, st);
  else if (ks == 1) launch_wgrad<false, 1>(pl, a, st);
  else if (ks == 3) launch_wgrad<false, 3>(pl, a, st);
  else launch_wgrad<false, 0>(pl, a, st);
  rc = launch_status();
  if (rc != GS_OK) return rc;
  if (pl.splits > 1) {
    launch_reduce(a, pl.splits, 1, st);
    rc = launch_status();
  }
  return rc;
}
