// Video frames as network input: the validation letterbox (val_prep.hip letterbox_kernel: OpenCV's fixed-point INTER_LINEAR,
// padding 114, / 255.f, the copy path when nothing is resized) reading each frame WHERE IT LIES - packed RGB / BGR with a row
// pitch, NV12 (a decoder surface: Y plane + interleaved UV plane) or I420 (three planes) - addressed by pointer instead of by
// pool offset.  There is no intermediate RGB image: every bilinear tap is converted to saturated u8 RGB on the fly, so the
// output is, bit for bit, kodhip_letterbox_batch's for the RGB image the colour conversion of the whole frame would give.
//
// YUV -> RGB is OpenCV's 4:2:0 conversion (cvtColor COLOR_YUV2RGB_NV12 / _I420, color_yuv.simd.hpp): 20-bit fixed point in
// int32, chroma not interpolated (pixel (r, c) takes the sample (r >> 1, c >> 1)); the six coefficients travel in the record,
// so the host picks the matrix per frame (data/frames.py matrix_coeffs).  The largest accumulator over all (Y, U, V) and all
// four matrices is 5.74e8 (tests/test_frames_reference.py).
#include "kodhip_resize.h"

namespace {

enum { FMT_RGB24 = 0, FMT_BGR24 = 1, FMT_NV12 = 2, FMT_I420 = 3 };

struct KodFrameDesc {
  const unsigned char* plane[3];  // device addresses: RGB/BGR: [0]; NV12: Y, UV; I420: Y, U, V
  int pitch0, pitch12;            // bytes between rows of plane 0 / of planes 1 and 2 (>= the row's bytes, otherwise free)
  int format;                     // FMT_*
  int h, w;                       // frame size (4:2:0 formats: both even)
  int nh, nw;                     // size after the resize
  int top, left;                  // position on the canvas
  double scale_x, scale_y;        // source / destination, as ValDesc
  int yoff, cy, cvr, cvg, cug, cub;
};

__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// One pixel of the frame as u8 r | g << 8 | b << 16.  r in [0, h), c in [0, w): the callers clamp.
//
// Loads: only bytes of the pixel itself are touched - three byte loads for a packed pixel, one byte of Y, the two bytes of
// the UV pair (a 2-byte copy the compiler may split).  letterbox_kernel's single 4-byte load per tap reads one byte past the
// pixel, which ImagePool's slack makes legal; a foreign surface has no slack and may end on the last byte of an allocation, and
// a 4-byte load "everywhere except a row's last pixel" would put a per-tap branch on the lane that holds it while still
// depending on nothing about alignment.  The bytes of a tap share one 64-byte line, so the narrower loads cost issue slots,
// not memory traffic; what that costs against the 4-byte tap is measured (tools/bench_frames.py, LOG.md).
template <int FMT> __device__ __forceinline__ unsigned frame_px(const KodFrameDesc& d, int r, int c) {
  if (FMT == FMT_RGB24 || FMT == FMT_BGR24) {
    const unsigned char* p = d.plane[0] + (long)r * d.pitch0 + (long)c * 3;
    const unsigned a = p[0], g = p[1], b = p[2];
    return FMT == FMT_RGB24 ? (a | (g << 8) | (b << 16)) : (b | (g << 8) | (a << 16));
  } else {
    const int Y = d.plane[0][(long)r * d.pitch0 + c];
    int U, V;
    if (FMT == FMT_NV12) {
      unsigned short uv;
      __builtin_memcpy(&uv, d.plane[1] + (long)(r >> 1) * d.pitch12 + (c >> 1) * 2, 2);
      U = uv & 255; V = uv >> 8;
    } else {
      const long o = (long)(r >> 1) * d.pitch12 + (c >> 1);
      U = d.plane[1][o]; V = d.plane[2][o];
    }
    const int uu = U - 128, vv = V - 128;
    const int y = max(0, Y - d.yoff) * d.cy + (1 << 19);
    const int R = sat8((y + d.cvr * vv) >> 20);                    // (>> on a negative sum is arithmetic: floor, as OpenCV)
    const int G = sat8((y + d.cvg * vv + d.cug * uu) >> 20);
    const int B = sat8((y + d.cub * uu) >> 20);
    return (unsigned)R | ((unsigned)G << 8) | ((unsigned)B << 16);
  }
}

// the two pixels of output pair (y, xp) of a frame in format FMT; px: 114 where the frame does not reach
template <int FMT> __device__ __forceinline__ void frame_pair(const KodFrameDesc& d, int dy, int xp, int px[2][3]) {
  const bool copy = d.nh == d.h && d.nw == d.w;
  int r0 = dy, r1 = dy, b0 = 0, b1 = 0;
  if (!copy) {
    int sy;
    lin_coeff(dy, d.scale_y, d.h, false, sy, b0, b1);
    r0 = min(max(sy, 0), d.h - 1);
    r1 = min(max(sy + 1, 0), d.h - 1);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {             // (`left` may be odd: each pixel of the pair decides for itself)
    const int dx = 2 * xp + k - d.left;
    if (dx < 0 || dx >= d.nw) continue;
    if (copy) {
      const unsigned p = frame_px<FMT>(d, r0, dx);
#pragma unroll
      for (int c = 0; c < 3; ++c) px[k][c] = (p >> (8 * c)) & 255;
    } else {
      int sx, a0, a1;
      lin_coeff(dx, d.scale_x, d.w, true, sx, a0, a1);
      const int sx1 = min(sx + 1, d.w - 1);
      const unsigned p00 = frame_px<FMT>(d, r0, sx), p01 = frame_px<FMT>(d, r0, sx1);
      const unsigned p10 = frame_px<FMT>(d, r1, sx), p11 = frame_px<FMT>(d, r1, sx1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int S0 = (int)((p00 >> (8 * c)) & 255) * a0 + (int)((p01 >> (8 * c)) & 255) * a1;
        const int S1 = (int)((p10 >> (8 * c)) & 255) * a0 + (int)((p11 >> (8 * c)) & 255) * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        px[k][c] = min(max(v, 0), 255);
      }
    }
  }
}

// One thread per pixel PAIR of a canvas row, as letterbox_kernel: one 16-byte store into the pair layout, one 8-byte store per
// fp32 plane.  The record (and with it the format) is uniform over a block, so the format switch does not diverge.
// grid: (ceil(H * W/2 / 256), B)
__global__ __launch_bounds__(256) void letterbox_frames_kernel(const KodFrameDesc* __restrict__ descs, float* __restrict__ out_f32,
                                                               bf16_t* __restrict__ out_pairs, int H, int W) {
  const int b = blockIdx.y;
  const int Wp = W >> 1;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= H * Wp) return;
  const int y = q / Wp, xp = q - y * Wp;
  const KodFrameDesc d = descs[b];
  int px[2][3] = {{114, 114, 114}, {114, 114, 114}};
  const int dy = y - d.top;
  if (dy >= 0 && dy < d.nh) {
    switch (d.format) {
      case FMT_RGB24: frame_pair<FMT_RGB24>(d, dy, xp, px); break;
      case FMT_BGR24: frame_pair<FMT_BGR24>(d, dy, xp, px); break;
      case FMT_NV12: frame_pair<FMT_NV12>(d, dy, xp, px); break;
      case FMT_I420: frame_pair<FMT_I420>(d, dy, xp, px); break;
      default: break;                       // (an unknown format reads nothing: the frame stays grey)
    }
  }
  float v[2][3];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[k][c] = (float)px[k][c] / 255.f;
  if (out_f32) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      *reinterpret_cast<float2*>(out_f32 + ((size_t)(b * 3 + c) * H + y) * W + 2 * xp) = make_float2(v[0][c], v[1][c]);
  }
  if (out_pairs) {   // network input layout [B][H][W/2][8] = pixel pairs x 4 channels
    bf16x8 o = {(bf16_t)v[0][0], (bf16_t)v[0][1], (bf16_t)v[0][2], (bf16_t)0.f,
                (bf16_t)v[1][0], (bf16_t)v[1][1], (bf16_t)v[1][2], (bf16_t)0.f};
    *reinterpret_cast<bf16x8*>(out_pairs + (((size_t)b * H + y) * Wp + xp) * 8) = o;
  }
}

}  // namespace

extern "C" {

int kodhip_frame_desc_bytes(void) { return (int)sizeof(KodFrameDesc); }

// descs: device [B] KodFrameDesc; out_f32 [B,3,H,W] and/or out_pairs (bf16 [B,H,W/2,8]).
int kodhip_letterbox_frames(const void* descs, float* out_f32, void* out_pairs, int B, int H, int W, hipStream_t stream) {
  KOD_CHECK_ARG(descs && (out_f32 || out_pairs) && B > 0 && B <= 65535 && H > 0 && W > 0 && W % 2 == 0 &&
                    (long)H * W <= (1L << 30),
                "letterbox_frames: bad args (W must be even)");
  KOD_CHECK_ARG(((uintptr_t)out_f32 % 8) == 0 && ((uintptr_t)out_pairs % 16) == 0,
                "letterbox_frames: out_f32 must be 8-byte aligned, out_pairs 16-byte aligned");
  hipLaunchKernelGGL(letterbox_frames_kernel, dim3(cdiv((long)H * (W / 2), 256), B), dim3(256), 0, stream,
                     (const KodFrameDesc*)descs, out_f32, (bf16_t*)out_pairs, H, W);
  KOD_LAUNCH_CHECK("letterbox_frames");
  return KOD_OK;
}

}  // extern "C"
