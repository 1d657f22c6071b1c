// Elastic input resolution (data.input_shape): ONE launch resamples a
// normalised training / evaluation batch on the device.
//
//   image   fp32 NCHW [N][3][h][w] -> [N][3][H][W]   bilinear, align_corners=False; the source indices
//           and weights are resize.h's (ATen's area_pixel_compute_source_index in fp32), so the weights
//           equal F.interpolate's bit for bit, as everywhere else in the project
//   labels  int64 [N][1][h][w] -> [N][1][H][W]       nearest, src = min(floor(dst * (float)in / out),
//           in - 1) in fp32 (ATen's nearest_neighbor_compute_source_index); 255 is a value like any other
//
// The kernel is a pure gather: every output element is written exactly once, from 4 (image) or 1
// (label) source elements.  No workspace, no atomics, the caller's stream.  It is bound by the output
// stores, so the OUTPUT is walked as one flat array in 16-byte pieces (4 floats of the image, 2 int64
// of the labels): both output tensors are contiguous and their bases 16-byte aligned, hence every
// piece is an aligned 16-byte store whatever W is -- a piece may run over the end of a row (or of a
// plane) into the next, each of its elements decodes its own (plane, Y, X).  Only the last
// (total mod 4 floats, total mod 2 labels) elements of a tensor are stored one by one.
#include "common.h"
#include "resize.h"

namespace gs {

struct RescaleArgs {
  const float* img;
  const int64_t* label;     // may be null (then out_label is null as well)
  float* out_img;
  int64_t* out_label;
  int h, w, H, W;
  long img_total;           // N * 3 * H * W
  long lab_total;           // N * H * W, 0 without labels
  long img_pieces;          // ceil(img_total / 4)
  long lab_pieces;          // ceil(lab_total / 2)
  float sh, sw;             // resize_scale(h, H, 0), resize_scale(w, W, 0)
};

__global__ __launch_bounds__(256) void batch_rescale_kernel(const RescaleArgs a) {
  const long hw = (long)a.h * a.w;
  const long pieces = a.img_pieces + a.lab_pieces;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < pieces;
       q += (long)gridDim.x * blockDim.x) {
    if (q < a.img_pieces) {
      const long base = q * 4;
      const int cnt = (int)(a.img_total - base < 4 ? a.img_total - base : 4);
      int X = (int)(base % a.W);
      long r = base / a.W;
      int Y = (int)(r % a.H);
      long p = r / a.H;                       // plane n * 3 + c
      float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < cnt) {
          const Lerp ly = lerp_coord(Y, a.sh, a.h, 0), lx = lerp_coord(X, a.sw, a.w, 0);
          const float* s = a.img + p * hw;
          const float* r0 = s + (long)ly.i0 * a.w;
          const float* r1 = s + (long)ly.i1 * a.w;
          v[k] = ly.l0 * (lx.l0 * r0[lx.i0] + lx.l1 * r0[lx.i1]) +
                 ly.l1 * (lx.l0 * r1[lx.i0] + lx.l1 * r1[lx.i1]);
          if (++X == a.W) { X = 0; if (++Y == a.H) { Y = 0; ++p; } }
        }
      }
      if (cnt == 4) {
        f32x4 o = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(a.out_img + base) = o;
      } else {
        for (int k = 0; k < cnt; ++k) a.out_img[base + k] = v[k];
      }
    } else {
      const long base = (q - a.img_pieces) * 2;
      const int cnt = (int)(a.lab_total - base < 2 ? a.lab_total - base : 2);
      int X = (int)(base % a.W);
      long r = base / a.W;
      int Y = (int)(r % a.H);
      long p = r / a.H;                       // sample n
      long v[2] = {0, 0};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (k < cnt) {
          const int sy = min((int)floorf((float)Y * a.sh), a.h - 1);
          const int sx = min((int)floorf((float)X * a.sw), a.w - 1);
          v[k] = a.label[p * hw + (long)sy * a.w + sx];
          if (++X == a.W) { X = 0; if (++Y == a.H) { Y = 0; ++p; } }
        }
      }
      if (cnt == 2) {
        u32x4 o = {(unsigned)v[0], (unsigned)((unsigned long)v[0] >> 32), (unsigned)v[1],
                   (unsigned)((unsigned long)v[1] >> 32)};
        *reinterpret_cast<u32x4*>(a.out_label + base) = o;
      } else {
        a.out_label[base] = v[0];
      }
    }
  }
}

}  // namespace gs

using namespace gs;

extern "C" int gs_batch_rescale(const float* img, const int64_t* label, int32_t N, int32_t h,
                                int32_t w, float* out_img, int64_t* out_label, int32_t H, int32_t W,
                                void* stream) {
  if (!img || !out_img) return GS_E_NULL;
  if ((label == nullptr) != (out_label == nullptr)) return GS_E_NULL;
  if (N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return GS_E_BADARG;
  // a plane's pixel count must fit the int arithmetic of the coordinates, the element counts of the
  // source and of the output image a signed 64-bit index
  if ((int64_t)h * w > INT32_MAX || (int64_t)H * W > INT32_MAX) return GS_E_BADARG;
  if ((int64_t)H * W > INT64_MAX / 3 / N || (int64_t)h * w > INT64_MAX / 3 / N) return GS_E_BADARG;
  if (!aligned16(out_img) || (out_label && !aligned16(out_label))) return GS_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(img) & 3u) || (reinterpret_cast<uintptr_t>(label) & 7u))
    return GS_E_ALIGN;
  RescaleArgs a;
  a.img = img; a.label = label; a.out_img = out_img; a.out_label = out_label;
  a.h = h; a.w = w; a.H = H; a.W = W;
  a.img_total = (long)N * 3 * H * W;
  a.lab_total = label ? (long)N * H * W : 0;
  a.img_pieces = ceil_div(a.img_total, 4);
  a.lab_pieces = ceil_div(a.lab_total, 2);
  a.sh = resize_scale(h, H, 0);
  a.sw = resize_scale(w, W, 0);
  hipLaunchKernelGGL(batch_rescale_kernel, dim3(stream_grid(a.img_pieces + a.lab_pieces, 256)),
                     dim3(256), 0, as_stream(stream), a);
  return launch_status();
}
