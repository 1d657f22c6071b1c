// Test-time augmentation views and the result overlay.
//
// gs_tta_views: every view of mmseg's MultiScaleFlipAug test pipeline (Resize(keep_ratio) to each
// scale -> RandomFlip -> Normalize -> ImageToTensor) for ONE decoded uint8 image in ONE launch.  A
// view is the image's pixels at one size, possibly mirrored; like gs_seg_augment every output pixel
// gathers its source from the ORIGINAL image, so no resized uint8 image ever exists.  Used as a
// test-time resize gs_seg_augment also reads a label map and writes an int64 label plane nobody
// reads (20 B written per output pixel); here 12 B are written and nothing but the image is read.
//
// Arithmetic: the contract at the top of augment.hip, through the same inlined device functions
// (augment_fetch.h).  The flip is applied after the resize: pixel (y, x) of a flipped view is pixel
// (y, W-1-x) or (H-1-y, x) of the unflipped view, evaluated by the same expression on the same
// integers, so a view and its mirror image are bit-identical.
//
// gs_seg_overlay: mmseg's show_result blend, out = uint8(img * (1 - opacity) + colour * opacity),
// evaluated in double and truncated as numpy does with a Python float opacity.
#include "augment_fetch.h"   // (switches fp contraction off for this file)

namespace gs {

// grid: x strides over the pixels of a view, y = view.  One pixel per lane: a wave writes 256
// contiguous bytes to each of the three channel planes.  A slot is only 4-byte aligned when
// 3 * res_h * res_w is odd, so the stores are single floats.
__global__ __launch_bounds__(256) void tta_views_kernel(const gs_tta_desc d,
                                                        const uint8_t* __restrict__ img) {
  const gs_tta_view v = d.views[blockIdx.y];
  const long plane = (long)v.res_h * v.res_w;
  const float sy = (float)d.src_h / (float)v.res_h, sx = (float)d.src_w / (float)v.res_w;
  float* __restrict__ out = v.out;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < plane;
       i += (long)gridDim.x * blockDim.x) {
    const int ox = (int)(i % v.res_w), oy = (int)(i / v.res_w);
    const int rx = v.flip == 1 ? v.res_w - 1 - ox : ox;    // position in the unflipped view
    const int ry = v.flip == 2 ? v.res_h - 1 - oy : oy;
    float c[3];
    fetch_bilinear_u8(img, d.src_h, d.src_w, sy, sx, ry, rx, c);
    const float b = d.src_is_rgb ? c[2] : c[0], g = c[1], r = d.src_is_rgb ? c[0] : c[2];
    store_normalized(out, plane, i, b, g, r, d.to_rgb, d.mean, d.std);
  }
}

// Four pixels (12 bytes, three 32-bit words) per lane; `packed` = img and out are 4-byte aligned, so
// whole words move.  The last group of an image whose pixel count is no multiple of 4, and unaligned
// buffers, go byte by byte.
__global__ __launch_bounds__(256) void seg_overlay_kernel(const int64_t* __restrict__ labels,
                                                          const uint8_t* __restrict__ img,
                                                          const uint8_t* __restrict__ palette,
                                                          int num_classes, long pixels, double opacity,
                                                          int packed, uint8_t* __restrict__ out) {
  const double keep = 1.0 - opacity;
  const long groups = (pixels + 3) / 4;
  for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups;
       gi += (long)gridDim.x * blockDim.x) {
    const long p0 = gi * 4;
    const int n = (int)(pixels - p0 < 4 ? pixels - p0 : 4);
    const bool words = packed && n == 4;
    uint32_t w[3] = {0u, 0u, 0u};
    if (words) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(img + p0 * 3);
      w[0] = src[0]; w[1] = src[1]; w[2] = src[2];
    } else {
      for (int k = 0; k < 3 * n; ++k) w[k >> 2] |= (uint32_t)img[p0 * 3 + k] << (8 * (k & 3));
    }
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= n) break;
      const int64_t l = labels[p0 + j];
      const bool known = l >= 0 && l < num_classes;      // anything else: colour (0, 0, 0)
#pragma unroll
      for (int k = 0; k < 3; ++k) {                        // k: B, G, R of the image; palette is RGB
        const int byte = 3 * j + k;
        const double px = (double)((w[byte >> 2] >> (8 * (byte & 3))) & 0xffu);
        const double col = known ? (double)palette[l * 3 + (2 - k)] : 0.0;
        const double val = px * keep + col * opacity;
        o[byte >> 2] |= ((uint32_t)(int)val & 0xffu) << (8 * (byte & 3));
      }
    }
    if (words) {
      uint32_t* dst = reinterpret_cast<uint32_t*>(out + p0 * 3);
      dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    } else {
      for (int k = 0; k < 3 * n; ++k) out[p0 * 3 + k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
  }
}

}  // namespace gs

using namespace gs;

extern "C" int gs_tta_views(gs_tta_desc d, const uint8_t* img, void* stream) {
  if (!img) return GS_E_NULL;
  if (d.n_views < 1 || d.n_views > GS_TTA_MAX_VIEWS) return GS_E_BADARG;
  if (d.src_h <= 0 || d.src_w <= 0) return GS_E_BADARG;
  long widest = 0;
  for (int k = 0; k < d.n_views; ++k) {
    const gs_tta_view& v = d.views[k];
    if (!v.out) return GS_E_NULL;
    if (v.res_h <= 0 || v.res_w <= 0 || v.flip < 0 || v.flip > 2) return GS_E_BADARG;
    const long plane = (long)v.res_h * v.res_w;
    if (plane > widest) widest = plane;
  }
  for (int k = 0; k < 3; ++k)
    if (!(d.std[k] > 0.f)) return GS_E_BADARG;
  hipLaunchKernelGGL(tta_views_kernel, dim3(stream_grid(widest, 256), d.n_views), dim3(256), 0,
                     as_stream(stream), d, img);
  return launch_status();
}

extern "C" int gs_seg_overlay(const int64_t* labels, const uint8_t* img, const uint8_t* palette,
                              int32_t num_classes, int32_t H, int32_t W, double opacity, uint8_t* out,
                              void* stream) {
  if (!labels || !img || !palette || !out) return GS_E_NULL;
  if (H <= 0 || W <= 0 || num_classes <= 0) return GS_E_BADARG;
  if (!(opacity >= 0.0 && opacity <= 1.0)) return GS_E_BADARG;   // (keeps the blend inside [0, 255])
  const long pixels = (long)H * W;
  const int packed = (reinterpret_cast<uintptr_t>(img) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
  hipLaunchKernelGGL(seg_overlay_kernel, dim3(stream_grid((pixels + 3) / 4, 256)), dim3(256), 0,
                     as_stream(stream), labels, img, palette, (int)num_classes, pixels, opacity,
                     packed, out);
  return launch_status();
}
