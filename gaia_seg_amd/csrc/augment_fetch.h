// The two steps every image kernel of the input pipeline shares (augment.hip, tta.hip): the bilinear
// uint8 fetch from the ORIGINAL image and the normalising store.  The arithmetic contract is stated
// at the top of augment.hip; both kernels inline exactly these expressions, so a pixel of the
// virtual resized image has one value whichever kernel produces it.
#pragma once
#include "common.h"

// separately rounded fp32 operations (see augment.hip); holds for every function defined below
// this line in the including file
#pragma clang fp contract(off)

namespace gs {

// Pixel (ry, rx) of the image resized with scales sy = src_h / res_h, sx = src_w / res_w: half-pixel
// centres, edge-clamped, bilinear in float, rounded to the nearest integer.  c[] is in the channel
// order of the source.
__device__ __forceinline__ void fetch_bilinear_u8(const uint8_t* __restrict__ img, int src_h,
                                                  int src_w, float sy, float sx, int ry, int rx,
                                                  float c[3]) {
  float fy = ((float)ry + 0.5f) * sy - 0.5f, fx = ((float)rx + 0.5f) * sx - 0.5f;
  int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
  float wy = fy - (float)y0, wx = fx - (float)x0;
  if (y0 < 0) { y0 = 0; wy = 0.f; }
  if (x0 < 0) { x0 = 0; wx = 0.f; }
  int y1 = y0 + 1, x1 = x0 + 1;
  if (y1 > src_h - 1) { y1 = src_h - 1; if (y0 > src_h - 1) { y0 = src_h - 1; } }
  if (x1 > src_w - 1) { x1 = src_w - 1; if (x0 > src_w - 1) { x0 = src_w - 1; } }
  const uint8_t* p00 = img + ((long)y0 * src_w + x0) * 3;
  const uint8_t* p01 = img + ((long)y0 * src_w + x1) * 3;
  const uint8_t* p10 = img + ((long)y1 * src_w + x0) * 3;
  const uint8_t* p11 = img + ((long)y1 * src_w + x1) * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float top = (float)p00[k] + ((float)p01[k] - (float)p00[k]) * wx;
    const float bot = (float)p10[k] + ((float)p11[k] - (float)p10[k]) * wx;
    c[k] = rintf(top + (bot - top) * wy);
  }
}

// Normalize (to_rgb -> planes R, G, B) + DefaultFormatBundle (CHW float): pixel i of three planes.
__device__ __forceinline__ void store_normalized(float* __restrict__ out, long plane, long i, float b,
                                                 float g, float r, int to_rgb, const float mean[3],
                                                 const float std[3]) {
  const float ch0 = to_rgb ? r : b, ch2 = to_rgb ? b : r;
  out[i] = (ch0 - mean[0]) / std[0];
  out[plane + i] = (g - mean[1]) / std[1];
  out[2 * plane + i] = (ch2 - mean[2]) / std[2];
}

}  // namespace gs
