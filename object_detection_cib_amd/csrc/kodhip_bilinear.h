// The singly rounded fp32 bilinear arithmetic of F.interpolate(mode="bilinear", align_corners=False), shared by
// kodhip_tta_view (tta.hip) and kodhip_multiscale_batch (multiscale.hip): both must produce the same bits.
// All fp32, every operation rounded on its own (no FMA):
//   per axis   scale = fp32(n_in) / fp32(n_out)
//              src   = max(fp32(fp32(dst + 0.5f) * scale) - 0.5f, 0)
//              i0 = (int)src, i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1
//   out = hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c + wx1 * d)      a, b on row y0, c, d on row y1; products rounded, then
//                                                                    the sum; then the outer products, then the outer sum
#pragma once
#include "kodhip_common.h"

// source index pair and weights of destination index `dst` along an axis of n_in source samples
__device__ __forceinline__ void bilin_axis(int dst, float scale, int n_in, int& i0, int& i1, float& l0, float& l1) {
  const float src = fmaxf(__fsub_rn(__fmul_rn(__fadd_rn((float)dst, 0.5f), scale), 0.5f), 0.f);
  i0 = (int)src;
  l1 = __fsub_rn(src, (float)i0);
  l0 = __fsub_rn(1.f, l1);
  i0 = min(i0, n_in - 1);          // (src <= n_in - 1/2 for every dst < n_out: i0 = n_in - 1 is reached when up-scaling; keeps the reads in bounds)
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
}

// a, b: the taps x0, x1 of row y0; c, d: of row y1
__device__ __forceinline__ float bilin_mix(float wx0, float wx1, float hy0, float hy1, float a, float b, float c, float d) {
  const float top = __fadd_rn(__fmul_rn(wx0, a), __fmul_rn(wx1, b));
  const float bot = __fadd_rn(__fmul_rn(wx0, c), __fmul_rn(wx1, d));
  return __fadd_rn(__fmul_rn(hy0, top), __fmul_rn(hy1, bot));
}
