// Second-stage crops: the pixels inside detection boxes, cut out of the frames where they lie (kodhip_frame.h) and resized to one
// fixed size, for a classifier / attribute / re-identification model behind the detector (YOLOv5 apply_classifier, save_one_box).
//
// Two launches, no host synchronisation between them:
//   crop_plan_kernel   one thread per detection row: the rectangle in YOLOv5's fp32 arithmetic, every operation rounded once
//                      (-ffp-contract=off), then the resize geometry in double, as letterbox_table forms it
//   crop_batch_kernel  one thread per output pixel: kodhip_resize.h's body (OpenCV's fixed-point INTER_LINEAR, the copy path,
//                      padding 114) applied to the cutout ALONE - lin_coeff runs with the cutout's size and the taps are clamped
//                      to the cutout's edges, as cv2.resize of a slice sees nothing of its neighbours; the cutout's origin is
//                      added only where a pixel is fetched, so a 4:2:0 cutout at an odd origin takes chroma sample
//                      (r >> 1, c >> 1) of the absolute position, and equals the cutout of the converted RGB frame bit for bit
#include <math.h>

#include "kodhip_frame.h"

namespace {

struct KodCropDesc {
  int frame;                      // index of the frame record the cutout is taken from
  int valid;                      // 0: empty (nothing is read, every pixel is the pad)
  int x0, y0, w, h;               // the cutout in the frame's pixels (empty: all four 0)
  int nh, nw;                     // size after the resize
  int top, left;                  // position in the out_h x out_w output
  double scale_x, scale_y;        // source / destination, as ValDesc
};

struct CropNorm { float mean[3], std[3]; int on; };

// a cutout of a frame as letterbox source (kodhip_resize.h): rows and columns are counted from the cutout's corner
template <int FMT> struct CropSource {
  const KodFrameDesc& f;
  int x0, y0;
  int r[2];
  __device__ __forceinline__ void rows(int r0, int r1) { r[0] = y0 + r0; r[1] = y0 + r1; }
  __device__ __forceinline__ unsigned px(int i, int c) const { return frame_px<FMT>(f, r[i], x0 + c); }
};

template <int FMT>
__device__ __forceinline__ void crop_px(const KodFrameDesc& f, const KodCropDesc& c, int dy, int dx, int px[3]) {
  const bool copy = c.nh == c.h && c.nw == c.w;
  int r0, r1, b0, b1;
  letterbox_rows(c, copy, dy, r0, r1, b0, b1);
  CropSource<FMT> src{f, c.x0, c.y0, {0, 0}};
  src.rows(r0, r1);
  letterbox_px(c, copy, dx, b0, b1, src, px);
}

// grid: ceil(N / 256)
__global__ __launch_bounds__(256) void crop_plan_kernel(const KodFrameDesc* __restrict__ frames, int B, const float* __restrict__ rows,
                                                        int row_stride, const int* __restrict__ row_index,
                                                        const int* __restrict__ frame_index, int N, int out_h, int out_w, int mode,
                                                        int square, float gain, float pad, KodCropDesc* __restrict__ crops,
                                                        int* __restrict__ rects) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  KodCropDesc c;
  c.frame = frame_index[n];
  c.valid = 0;
  c.x0 = c.y0 = c.w = c.h = 0;
  c.nh = c.nw = 1;
  c.top = c.left = 0;
  c.scale_x = c.scale_y = 1.0;
  const int ri = row_index[n];
  if (c.frame >= 0 && c.frame < B && ri >= 0) {
    const float* row = rows + (size_t)ri * row_stride;
    const float x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
    if (isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)) {
      const float W = (float)frames[c.frame].w, H = (float)frames[c.frame].h;
      // xyxy2xywh, the square, gain and pad, xywh2xyxy, clip_boxes: one fp32 rounding per operation
      const float cx = (x1 + x2) / 2.f, cy = (y1 + y2) / 2.f;
      float w = x2 - x1, h = y2 - y1;
      if (square) w = h = fmaxf(w, h);
      w = w * gain + pad;
      h = h * gain + pad;
      float ax = cx - w / 2.f, bx = cx + w / 2.f, ay = cy - h / 2.f, by = cy + h / 2.f;
      if (!(isnan(ax) || isnan(bx) || isnan(ay) || isnan(by))) {       // (inf - inf of an overflowed box: empty)
        ax = fminf(fmaxf(ax, 0.f), W); bx = fminf(fmaxf(bx, 0.f), W);
        ay = fminf(fmaxf(ay, 0.f), H); by = fminf(fmaxf(by, 0.f), H);
        const int x0 = (int)ax, y0 = (int)ay;                          // int(): toward zero
        const int cw = (int)bx - x0, ch = (int)by - y0;
        if (cw >= 1 && ch >= 1) {
          c.valid = 1;
          c.x0 = x0; c.y0 = y0; c.w = cw; c.h = ch;
          c.nh = out_h; c.nw = out_w;
          if (mode == 1) {
            const double r = fmin(out_h / (double)ch, out_w / (double)cw);
            c.nh = (int)fmin(fmax(rint(ch * r), 1.0), (double)out_h);  // rint: half to even, Python's round
            c.nw = (int)fmin(fmax(rint(cw * r), 1.0), (double)out_w);
            c.top = (out_h - c.nh) / 2;
            c.left = (out_w - c.nw) / 2;
          }
          c.scale_y = 1.0 / (c.nh / (double)ch);
          c.scale_x = 1.0 / (c.nw / (double)cw);
        }
      }
    }
  }
  crops[n] = c;
  if (rects) {
    int* q = rects + (size_t)n * 4;
    q[0] = c.x0; q[1] = c.y0; q[2] = c.w; q[3] = c.h;
  }
}

// grid: (ceil(out_h * out_w / 256), N); the crop record (and with it the frame and its format) is uniform over a block
__global__ __launch_bounds__(256) void crop_batch_kernel(const KodFrameDesc* __restrict__ frames, int B, const KodCropDesc* __restrict__ crops,
                                                         float* __restrict__ out_f32, unsigned char* __restrict__ out_u8, int out_h,
                                                         int out_w, int bgr, CropNorm norm) {
  const int n = blockIdx.y;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= out_h * out_w) return;
  const int y = q / out_w, x = q - y * out_w;
  const KodCropDesc c = crops[n];
  int px[3] = {114, 114, 114};
  const int dy = y - c.top, dx = x - c.left;
  if (c.valid && c.frame >= 0 && c.frame < B && dy >= 0 && dy < c.nh && dx >= 0 && dx < c.nw) {
    const KodFrameDesc f = frames[c.frame];
    switch (f.format) {
      case FMT_RGB24: crop_px<FMT_RGB24>(f, c, dy, dx, px); break;
      case FMT_BGR24: crop_px<FMT_BGR24>(f, c, dy, dx, px); break;
      case FMT_NV12: crop_px<FMT_NV12>(f, c, dy, dx, px); break;
      case FMT_I420: crop_px<FMT_I420>(f, c, dy, dx, px); break;
      default: break;                       // (an unknown format reads nothing: the crop stays grey)
    }
  }
  if (bgr) { const int t = px[0]; px[0] = px[2]; px[2] = t; }
  if (out_f32) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v = (float)px[k] / 255.f;
      if (norm.on) v = (v - norm.mean[k]) / norm.std[k];
      out_f32[(((size_t)n * 3 + k) * out_h + y) * out_w + x] = v;
    }
  }
  if (out_u8) {
    unsigned char* o = out_u8 + (((size_t)n * out_h + y) * out_w + x) * 3;
    o[0] = (unsigned char)px[0]; o[1] = (unsigned char)px[1]; o[2] = (unsigned char)px[2];
  }
}

// the size checks both launchers share
#define CROP_CHECK_SIZES(name)                                                                                          \
  do {                                                                                                                  \
    KOD_CHECK_ARG(B >= 1 && B <= 65535, name ": B %d: expected 1..65535 frames", B);                                    \
    KOD_CHECK_ARG(N >= 1 && N <= 65535, name ": N %d: expected 1..65535 crops per launch", N);                          \
    KOD_CHECK_ARG(out_h >= 1 && out_h <= 1024 && out_w >= 1 && out_w <= 1024, name ": out_h %d, out_w %d: expected 1..1024", \
                  out_h, out_w);                                                                                        \
  } while (0)

}  // namespace

extern "C" {

int kodhip_crop_desc_bytes(void) { return (int)sizeof(KodCropDesc); }

int kodhip_crop_plan(const void* frames, int B, const float* rows, int row_stride, const int* row_index, const int* frame_index, int N,
                     int out_h, int out_w, int mode, int square, float gain, float pad, void* crops, int* rects, hipStream_t stream) {
  KOD_CHECK_ARG(frames && rows && row_index && frame_index && crops, "crop_plan: null frames, rows, row_index, frame_index or crops");
  CROP_CHECK_SIZES("crop_plan");
  KOD_CHECK_ARG(row_stride >= 4, "crop_plan: row_stride %d below 4 (x1, y1, x2, y2 come first)", row_stride);
  KOD_CHECK_ARG(mode == 0 || mode == 1, "crop_plan: mode %d: expected 0 (stretch) or 1 (letterbox)", mode);
  KOD_CHECK_ARG(isfinite(gain) && gain > 0.f, "crop_plan: gain must be finite and > 0");
  KOD_CHECK_ARG(isfinite(pad) && pad >= 0.f, "crop_plan: pad must be finite and >= 0");
  hipLaunchKernelGGL(crop_plan_kernel, dim3(cdiv(N, 256)), dim3(256), 0, stream, (const KodFrameDesc*)frames, B, rows, row_stride,
                     row_index, frame_index, N, out_h, out_w, mode, square ? 1 : 0, gain, pad, (KodCropDesc*)crops, rects);
  KOD_LAUNCH_CHECK("crop_plan");
  return KOD_OK;
}

int kodhip_crop_batch(const void* frames, int B, const void* crops, int N, float* out_f32, unsigned char* out_u8, int out_h, int out_w,
                      int bgr, const float* mean_std, hipStream_t stream) {
  KOD_CHECK_ARG(frames && crops, "crop_batch: null frames or crops");
  KOD_CHECK_ARG(out_f32 || out_u8, "crop_batch: at least one output (out_f32, out_u8)");
  CROP_CHECK_SIZES("crop_batch");
  CropNorm norm = {{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, 0};
  if (mean_std) {
    for (int k = 0; k < 3; ++k) {
      KOD_CHECK_ARG(isfinite(mean_std[k]), "crop_batch: mean[%d] must be finite", k);
      KOD_CHECK_ARG(isfinite(mean_std[3 + k]) && mean_std[3 + k] != 0.f, "crop_batch: std[%d] must be finite and non-zero", k);
      norm.mean[k] = mean_std[k];
      norm.std[k] = mean_std[3 + k];
    }
    norm.on = 1;
  }
  hipLaunchKernelGGL(crop_batch_kernel, dim3(cdiv((long)out_h * out_w, 256), N), dim3(256), 0, stream, (const KodFrameDesc*)frames, B,
                     (const KodCropDesc*)crops, out_f32, out_u8, out_h, out_w, bgr ? 1 : 0, norm);
  KOD_LAUNCH_CHECK("crop_batch");
  return KOD_OK;
}

}  // extern "C"
