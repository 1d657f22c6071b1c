// gfx950: fused AdamW (decoupled weight decay) over a chunk table of the flat parameter arena, with
// per-parameter step counters in device memory.
#include <algorithm>
#include "common.h"

namespace gs {

// torch.optim.AdamW's single-tensor update (amsgrad=False, maximize=False) over a TABLE of chunks.
// chunk = {begin, length, group, slot} in float4 units relative to the arena bases (GsSgdChunk with
// `reserved` = the index of the parameter's counter in `steps`); a chunk never spans two parameters.
// One workgroup per chunk (grid-stride over the table): the entry, and with it every scalar of the
// update, is uniform over the workgroup.
// hyper (doubles) = {beta1, beta2, eps, gscale, n_groups, log(beta1), log(beta2), 0, lr_0, wd_0, ...}.
// The scalars are formed in fp64, as torch forms them in Python doubles, and rounded to fp32 only
// where they meet the tensors: (float)(1 - lr*wd), (float)(1 - beta1), (float)beta2,
// (float)(1 - beta2), (float)(lr / bc1), (float)sqrt(bc2), (float)eps.  The bias corrections
// 1 - beta^t are -expm1(t * log(beta)): no cancellation at small t (fp32 1 - powf(beta, t) loses
// ~6e-5 relative at t = 1 for beta2 = 0.999).  They cost two fp64 expm1 per CHUNK, not per element;
// the per-element work is fp32 mul / add, one sqrtf and two divisions, all correctly rounded.
// The kernel only READS steps; adamw_bump_kernel advances them afterwards in stream order.
// Elements outside the table are never read or written; an entry naming a group the hyper table does
// not have, or a slot outside steps, is skipped.
__device__ __forceinline__ bool adamw_chunk_ok(const GsSgdChunk& ch, int n_groups, int n_slots) {
  return (unsigned)ch.group < (unsigned)n_groups && (unsigned)ch.reserved < (unsigned)n_slots &&
         ch.begin >= 0 && ch.length > 0;
}

template <bool ZERO>
__global__ __launch_bounds__(256) void adamw_groups_kernel(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
    const int32_t* __restrict__ steps, int n_slots, const GsSgdChunk* __restrict__ chunks,
    int n_chunks, const double* __restrict__ hyper) {
  const double beta1 = hyper[0], beta2 = hyper[1], eps = hyper[2];
  const float gscale = (float)hyper[3];
  const int n_groups = (int)hyper[4];
  const double log_b1 = hyper[5], log_b2 = hyper[6];
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  const float epsf = (float)eps;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const GsSgdChunk ch = chunks[c];
    if (!adamw_chunk_ok(ch, n_groups, n_slots)) continue;
    const double lr = hyper[8 + 2 * ch.group], wd = hyper[9 + 2 * ch.group];
    const double t = (double)steps[ch.reserved] + 1.0;
    const double bc1 = -expm1(t * log_b1), bc2 = -expm1(t * log_b2);
    const float decay = (float)(1.0 - lr * wd);
    const float neg_step = (float)(-(lr / bc1));
    const float bc2_sqrt = (float)sqrt(bc2);
    const long end = (long)ch.begin + ch.length;
    for (long i = (long)ch.begin + threadIdx.x; i < end; i += blockDim.x) {
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i] * gscale;
      f32x4 pv = reinterpret_cast<f32x4*>(p)[i] * decay;
      f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
      f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
      mv = mv + (gv - mv) * w1;
      vv = vv * b2 + (gv * w2) * gv;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float denom = sqrtf(vv[k]) / bc2_sqrt + epsf;
        pv[k] = pv[k] + (neg_step * mv[k]) / denom;
      }
      reinterpret_cast<f32x4*>(m)[i] = mv;
      reinterpret_cast<f32x4*>(v)[i] = vv;
      reinterpret_cast<f32x4*>(p)[i] = pv;
      if (ZERO) reinterpret_cast<f32x4*>(g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// steps[slot] += 1 for every parameter the table steps: one thread per chunk, and the thread of a
// parameter's FIRST chunk (its predecessor in the table names another slot, or is skipped) writes.
// One parameter's chunks are contiguous in the table, so exactly one thread writes a counter: no
// atomics.  Launched behind the step kernel on the same stream.
__global__ __launch_bounds__(256) void adamw_bump_kernel(int32_t* __restrict__ steps, int n_slots,
                                                         const GsSgdChunk* __restrict__ chunks,
                                                         int n_chunks,
                                                         const double* __restrict__ hyper) {
  const int n_groups = (int)hyper[4];
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n_chunks; c += gridDim.x * blockDim.x) {
    const GsSgdChunk ch = chunks[c];
    if (!adamw_chunk_ok(ch, n_groups, n_slots)) continue;
    if (c > 0) {
      const GsSgdChunk prev = chunks[c - 1];
      if (prev.reserved == ch.reserved && adamw_chunk_ok(prev, n_groups, n_slots)) continue;
    }
    steps[ch.reserved] += 1;
  }
}

__global__ void adamw_set_group_hyper_kernel(double* hyper, double beta1, double beta2, double eps,
                                             double gscale, int n_groups, GsAdamwGroups v) {
  const int t = threadIdx.x;
  if (t == 0) {
    hyper[0] = beta1; hyper[1] = beta2; hyper[2] = eps; hyper[3] = gscale;
    hyper[4] = (double)n_groups; hyper[5] = log(beta1); hyper[6] = log(beta2); hyper[7] = 0.0;
  }
  if (t < 2 * GS_SGD_MAX_GROUPS) hyper[8 + t] = t < 2 * n_groups ? v.lr_wd[t] : 0.0;
}

}  // namespace gs

using namespace gs;

extern "C" int gs_adamw_set_group_hyper(double* hyper, double beta1, double beta2, double eps,
                                        double grad_scale, int32_t n_groups, GsAdamwGroups lr_wd,
                                        void* stream) {
  if (!hyper) return GS_E_NULL;
  if (n_groups < 1 || n_groups > GS_SGD_MAX_GROUPS) return GS_E_BADARG;
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps > 0.0))
    return GS_E_BADARG;
  if (!aligned16(hyper)) return GS_E_ALIGN;
  hipLaunchKernelGGL(adamw_set_group_hyper_kernel, dim3(1), dim3(64), 0, as_stream(stream), hyper,
                     beta1, beta2, eps, grad_scale, (int)n_groups, lr_wd);
  return launch_status();
}

extern "C" int gs_adamw_step_groups(float* param, float* grad, float* exp_avg, float* exp_avg_sq,
                                    int32_t* steps, int32_t n_slots, const GsSgdChunk* chunks,
                                    int32_t n_chunks, const double* hyper, int32_t zero_grad,
                                    void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !steps || !chunks || !hyper) return GS_E_NULL;
  if (n_chunks <= 0 || n_slots <= 0) return GS_E_BADARG;
  if (!aligned16(param) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
      !aligned16(chunks) || !aligned16(hyper) || (reinterpret_cast<uintptr_t>(steps) & 3u))
    return GS_E_ALIGN;
  // a fixed number of workgroups (8 per CU), fewer only when the table is shorter
  const int grid = (int)std::min<int64_t>(n_chunks, (int64_t)num_cu() * 8);
  if (zero_grad)
    hipLaunchKernelGGL((adamw_groups_kernel<true>), dim3(grid), dim3(256), 0, as_stream(stream),
                       param, grad, exp_avg, exp_avg_sq, (const int32_t*)steps, (int)n_slots, chunks,
                       (int)n_chunks, hyper);
  else
    hipLaunchKernelGGL((adamw_groups_kernel<false>), dim3(grid), dim3(256), 0, as_stream(stream),
                       param, grad, exp_avg, exp_avg_sq, (const int32_t*)steps, (int)n_slots, chunks,
                       (int)n_chunks, hyper);
  int rc = launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(adamw_bump_kernel, dim3(stream_grid(n_chunks, 256)), dim3(256), 0,
                     as_stream(stream), steps, (int)n_slots, chunks, (int)n_chunks, hyper);
  return launch_status();
}
