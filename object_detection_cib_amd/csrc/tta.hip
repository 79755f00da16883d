// Test-time augmentation (YOLOv5 models/yolo.py::_forward_augment, utils/torch_utils.py::scale_img): one view of a batch
// that is already on the device - optional left-right flip, bilinear down-scaling to h x w, placed top-left in an Hp x Wp
// canvas filled with `pad` - written straight into the network's input layout (bf16 pixel pairs [B][Hp][Wp/2][8], what
// kodhip_nchw_to_nhwc4 produces), so the view goes into forward(..., image_ready=True) with no fp32 intermediate.
//
// The resize is F.interpolate(mode="bilinear", align_corners=False, size=(h, w)) with the arithmetic fixed as follows, all
// fp32, every operation rounded on its own (no FMA):
//   per axis   scale = fp32(n_in) / fp32(n_out)
//              src   = max(fp32(fp32(dst + 0.5f) * scale) - 0.5f, 0)
//              i0 = (int)src, i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1
//   out = hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c + wx1 * d)      a, b on row y0, c, d on row y1; products rounded, then
//                                                                    the sum; then the outer products, then the outer sum
// The flip comes first (the view is the resize of x[..., ::-1]); it is folded into the column index of the reads.
// h = H, w = W gives l1 = 0 on both axes and reproduces the (flipped) pixels.
#include "kodhip_bilinear.h"

namespace {

struct TtaViewArgs {
  const float* x;        // [B][3][H][W]
  bf16_t* pairs;         // [B][Hp][Wp/2][8]
  float* f32;            // [B][3][Hp][Wp] or null
  int B, H, W, h, w, Hp, Wp, flip;
  float pad, scale_y, scale_x;
};

// one thread per output pixel pair: 2 x 3 channels, one 16-byte store
__global__ __launch_bounds__(256) void tta_view_kernel(TtaViewArgs a) {
  const int Wq = a.Wp >> 1;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)a.B * a.Hp * Wq) return;
  const int q = (int)(i % Wq);
  const long t = i / Wq;
  const int y = (int)(t % a.Hp), b = (int)(t / a.Hp);
  float v[2][3];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[k][c] = a.pad;
  if (y < a.h) {
    int y0, y1;
    float hy0, hy1;
    bilin_axis(y, a.scale_y, a.H, y0, y1, hy0, hy1);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int x = 2 * q + k;
      if (x >= a.w) continue;
      int x0, x1;
      float wx0, wx1;
      bilin_axis(x, a.scale_x, a.W, x0, x1, wx0, wx1);
      if (a.flip) { x0 = a.W - 1 - x0; x1 = a.W - 1 - x1; }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* pl = a.x + (size_t)(b * 3 + c) * a.H * a.W;
        const float* r0 = pl + (size_t)y0 * a.W;
        const float* r1 = pl + (size_t)y1 * a.W;
        v[k][c] = bilin_mix(wx0, wx1, hy0, hy1, r0[x0], r0[x1], r1[x0], r1[x1]);
      }
    }
  }
  kod_store_input_pair(a.f32, a.pairs, b, y, q, a.Hp, a.Wp, v);    // (a.pairs is never null: the launcher checks)
}

}  // namespace

extern "C" {

// x [B][3][H][W] fp32 -> out_pairs bf16 [B][Hp][Wp/2][8] (and out_f32 [B][3][Hp][Wp] when not null: the same fp32 values
// before their rounding to bf16).  Down-scaling only: h <= H, w <= W; h <= Hp, w <= Wp, Wp even.
int kodhip_tta_view(const float* x, void* out_pairs, float* out_f32, int B, int H, int W, int h, int w, int Hp, int Wp,
                    int flip_lr, float pad, hipStream_t stream) {
  KOD_CHECK_ARG(x && out_pairs, "tta_view: null pointer");
  KOD_CHECK_ARG(B > 0 && H > 0 && W > 0 && h > 0 && w > 0, "tta_view: bad sizes");
  KOD_CHECK_ARG(h <= H && w <= W, "tta_view: down-scaling only (h <= H, w <= W)");
  KOD_CHECK_ARG(Hp >= h && Wp >= w, "tta_view: the canvas must hold the view (Hp >= h, Wp >= w)");
  KOD_CHECK_ARG(Wp % 2 == 0, "tta_view: Wp must be even (pixel pairs)");
  KOD_CHECK_ARG(flip_lr == 0 || flip_lr == 1, "tta_view: flip_lr must be 0 or 1");
  KOD_CHECK_ARG((long)B * Hp * Wp < (1l << 33), "tta_view: batch too large");
  TtaViewArgs a = {};
  a.x = x; a.pairs = (bf16_t*)out_pairs; a.f32 = out_f32;
  a.B = B; a.H = H; a.W = W; a.h = h; a.w = w; a.Hp = Hp; a.Wp = Wp; a.flip = flip_lr;
  a.pad = pad;
  a.scale_y = (float)H / (float)h;
  a.scale_x = (float)W / (float)w;
  hipLaunchKernelGGL(tta_view_kernel, dim3(cdiv((long)B * Hp * (Wp / 2), 256)), dim3(256), 0, stream, a);
  KOD_LAUNCH_CHECK("tta_view");
  return KOD_OK;
}

}  // extern "C"
