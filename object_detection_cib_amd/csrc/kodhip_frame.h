// A video frame where it lies, for the kernels that read one (video.hip: the letterbox; crops.hip: the cutouts): the record, the
// per-format pixel fetch and the frame as a source of kodhip_resize.h's body.
//
// YUV -> RGB is OpenCV's 4:2:0 conversion (cvtColor COLOR_YUV2RGB_NV12 / _I420, color_yuv.simd.hpp): 20-bit fixed point in
// int32, chroma not interpolated (pixel (r, c) takes the sample (r >> 1, c >> 1)); the six coefficients travel in the record,
// so the host picks the matrix per frame (data/frames.py matrix_coeffs).  The largest accumulator over all (Y, U, V) and all
// four matrices is 5.74e8 (tests/test_frames_reference.py).
#pragma once
#include "kodhip_resize.h"

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
// the UV pair (a 2-byte copy the compiler may split).  The pool source's single 4-byte load per tap reads one byte past the
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

// a frame in format FMT as letterbox source (kodhip_resize.h)
template <int FMT> struct FrameSource {
  const KodFrameDesc& d;
  int r[2];
  __device__ __forceinline__ void rows(int r0, int r1) { r[0] = r0; r[1] = r1; }
  __device__ __forceinline__ unsigned px(int i, int c) const { return frame_px<FMT>(d, r[i], c); }
};
