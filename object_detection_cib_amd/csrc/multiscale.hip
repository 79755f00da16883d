// Multi-scale training (YOLOv5 train.py --multi-scale: F.interpolate(imgs, size=ns, mode="bilinear", align_corners=False) on
// every batch): one launch resizes a base-size batch that is already on the device to the h x w canvas of the step - up or
// down, each axis on its own - and writes it straight into the network's input layout (bf16 pixel pairs [B][h][w/2][8], what
// kodhip_nchw_to_nhwc4 produces), and scales the batch's target boxes (fp64 xyxy pixels) with it in the same launch.
//
// The image arithmetic is kodhip_tta_view's (kodhip_bilinear.h), all fp32, every operation rounded on its own.  h = H, w = W
// gives l1 = 0 on both axes and reproduces the pixels: there is no copy special case.  The source is the fp32 NCHW batch or
// the bf16 pixel-pair batch a device pipeline composites (bf16 -> fp32 is exact).
// Boxes: x' = x * (fp64(w) / fp64(W)), y' = y * (fp64(h) / fp64(H)), one rounded fp64 multiply each; zero padding rows stay zero.
#include "kodhip_bilinear.h"

namespace {

struct MultiScaleArgs {
  const float* x;          // [B][3][H][W] or null
  const bf16_t* xp;        // [B][H][W/2][8] or null
  bf16_t* pairs;           // [B][h][w/2][8]
  float* f32;              // [B][3][h][w] or null
  int B, H, W, h, w;
  float scale_y, scale_x;
  const double* boxes_in;  // [n][4] xyxy
  double* boxes_out;
  long n4;                 // 4 * n coordinates
  double sx, sy;
  int pixel_blocks;
};

// pixel blocks: one thread per output pixel pair (2 x 3 channels, one 16-byte store); behind them the box blocks: one
// thread per coordinate
template <bool PAIRS> __global__ __launch_bounds__(256) void multiscale_batch_kernel(MultiScaleArgs a) {
  if ((int)blockIdx.x >= a.pixel_blocks) {
    const long j = (long)(blockIdx.x - a.pixel_blocks) * blockDim.x + threadIdx.x;
    if (j < a.n4) a.boxes_out[j] = __dmul_rn(a.boxes_in[j], (j & 1) ? a.sy : a.sx);
    return;
  }
  const unsigned wq = (unsigned)a.w >> 1;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)a.B * a.h * wq) return;
  // B * h * w < 2^33 (checked by the launcher), so a pixel-pair index fits 32 bits: 32-bit divisions
  const unsigned iu = (unsigned)i;
  const int q = (int)(iu % wq);
  const unsigned t = iu / wq;
  const int y = (int)(t % (unsigned)a.h), b = (int)(t / (unsigned)a.h);
  int y0, y1;
  float hy0, hy1;
  bilin_axis(y, a.scale_y, a.H, y0, y1, hy0, hy1);
  float v[2][3];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    int x0, x1;
    float wx0, wx1;
    bilin_axis(2 * q + k, a.scale_x, a.W, x0, x1, wx0, wx1);
    if (PAIRS) {
      // a source pixel is 4 bf16 (8 bytes); an even x0 has x1 = x0 + 1 in the same 16-byte pair (W is even)
      const bf16_t* r0 = a.xp + ((size_t)b * a.H + y0) * a.W * 4;
      const bf16_t* r1 = a.xp + ((size_t)b * a.H + y1) * a.W * 4;
      bf16x4 p00, p01, p10, p11;
      if ((x0 & 1) == 0) {
        const bf16x8 u0 = *reinterpret_cast<const bf16x8*>(r0 + (size_t)x0 * 4);
        const bf16x8 u1 = *reinterpret_cast<const bf16x8*>(r1 + (size_t)x0 * 4);
        p00 = __builtin_shufflevector(u0, u0, 0, 1, 2, 3);
        p01 = __builtin_shufflevector(u0, u0, 4, 5, 6, 7);
        p10 = __builtin_shufflevector(u1, u1, 0, 1, 2, 3);
        p11 = __builtin_shufflevector(u1, u1, 4, 5, 6, 7);
      } else {
        p00 = *reinterpret_cast<const bf16x4*>(r0 + (size_t)x0 * 4);
        p01 = *reinterpret_cast<const bf16x4*>(r0 + (size_t)x1 * 4);
        p10 = *reinterpret_cast<const bf16x4*>(r1 + (size_t)x0 * 4);
        p11 = *reinterpret_cast<const bf16x4*>(r1 + (size_t)x1 * 4);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
        v[k][c] = bilin_mix(wx0, wx1, hy0, hy1, bf2f(p00[c]), bf2f(p01[c]), bf2f(p10[c]), bf2f(p11[c]));
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* pl = a.x + (size_t)(b * 3 + c) * a.H * a.W;
        const float* r0 = pl + (size_t)y0 * a.W;
        const float* r1 = pl + (size_t)y1 * a.W;
        v[k][c] = bilin_mix(wx0, wx1, hy0, hy1, r0[x0], r0[x1], r1[x0], r1[x1]);
      }
    }
  }
  kod_store_input_pair(a.f32, a.pairs, b, y, q, a.h, a.w, v);      // (a.pairs is never null: the launcher checks)
}

bool ranges_overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}

}  // namespace

extern "C" {

int kodhip_multiscale_batch(const float* x_f32, const void* x_pairs, void* out_pairs, float* out_f32, int B, int H, int W, int h,
                            int w, const double* boxes_in, double* boxes_out, int n, hipStream_t stream) {
  KOD_CHECK_ARG((x_f32 != nullptr) != (x_pairs != nullptr), "multiscale_batch: exactly one source (x_f32 or x_pairs)");
  KOD_CHECK_ARG(out_pairs, "multiscale_batch: null out_pairs");
  KOD_CHECK_ARG(B > 0 && H > 0 && W > 0 && h > 0 && w > 0, "multiscale_batch: bad sizes");
  KOD_CHECK_ARG(W % 2 == 0 && w % 2 == 0, "multiscale_batch: W and w must be even (pixel pairs)");
  KOD_CHECK_ARG((long)B * h * w < (1l << 33) && (long)B * H * W < (1l << 33), "multiscale_batch: batch too large");
  KOD_CHECK_ARG(n >= 0, "multiscale_batch: negative box count");
  KOD_CHECK_ARG(((uintptr_t)out_pairs & 15) == 0 && ((uintptr_t)x_pairs & 15) == 0 && ((uintptr_t)out_f32 & 7) == 0 &&
                    ((uintptr_t)x_f32 & 3) == 0,
                "multiscale_batch: misaligned buffer (pairs 16 bytes, out_f32 8 bytes)");
  const bool boxes = n > 0 && boxes_in != nullptr;
  KOD_CHECK_ARG(!boxes || boxes_out, "multiscale_batch: boxes_in without boxes_out");
  const void* src = x_f32 ? (const void*)x_f32 : x_pairs;
  const size_t src_bytes = (size_t)B * H * W * (x_f32 ? 12 : 8);
  KOD_CHECK_ARG(!ranges_overlap(src, src_bytes, out_pairs, (size_t)B * h * w * 8) &&
                    !(out_f32 && ranges_overlap(src, src_bytes, out_f32, (size_t)B * h * w * 12)),
                "multiscale_batch: an output overlaps the source");
  KOD_CHECK_ARG(!boxes || boxes_out == boxes_in || !ranges_overlap(boxes_in, (size_t)n * 32, boxes_out, (size_t)n * 32),
                "multiscale_batch: boxes_out must be boxes_in or disjoint from it");
  MultiScaleArgs a = {};
  a.x = x_f32; a.xp = (const bf16_t*)x_pairs; a.pairs = (bf16_t*)out_pairs; a.f32 = out_f32;
  a.B = B; a.H = H; a.W = W; a.h = h; a.w = w;
  a.scale_y = (float)H / (float)h;
  a.scale_x = (float)W / (float)w;
  a.boxes_in = boxes_in; a.boxes_out = boxes_out;
  a.n4 = boxes ? 4l * n : 0;
  a.sx = (double)w / (double)W;
  a.sy = (double)h / (double)H;
  a.pixel_blocks = cdiv((long)B * h * (w / 2), 256);
  const dim3 grid(a.pixel_blocks + cdiv(a.n4, 256));
  if (x_pairs) hipLaunchKernelGGL(multiscale_batch_kernel<true>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(multiscale_batch_kernel<false>, grid, dim3(256), 0, stream, a);
  KOD_LAUNCH_CHECK("multiscale_batch");
  return KOD_OK;
}

}  // extern "C"
