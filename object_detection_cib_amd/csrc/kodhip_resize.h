// OpenCV's fixed-point INTER_LINEAR coefficients (resize.cpp, 8-bit images), shared by the letterbox kernels of val_prep.hip
// (images in the pool) and video.hip (frames where they lie): both must produce the same bits.
#pragma once
#include "kodhip_common.h"

__device__ __forceinline__ int sat16(float v) {
  int r = __float2int_rn(v);
  return r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
}

// left source index + 11-bit weights of destination index d (resize.cpp, INTER_LINEAR)
__device__ __forceinline__ void lin_coeff(int d, double scale, int n_src, bool clamp_edges, int& s, int& w0, int& w1) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f -= (float)s;
  if (clamp_edges) {        // horizontal: x < 0 and x >= width-1 collapse to one tap; vertical clamps the two rows instead
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= n_src - 1) { s = n_src - 1; f = 0.f; }
  }
  w0 = sat16((1.f - f) * 2048.f);
  w1 = sat16(f * 2048.f);
}
