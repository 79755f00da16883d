// Video frames as network input: the validation letterbox (kodhip_resize.h, the body val_prep.hip's letterbox_kernel runs:
// OpenCV's fixed-point INTER_LINEAR, padding 114, / 255.f, the copy path when nothing is resized) reading each frame WHERE IT LIES - packed RGB / BGR with a row
// pitch, NV12 (a decoder surface: Y plane + interleaved UV plane) or I420 (three planes) - addressed by pointer instead of by
// pool offset.  There is no intermediate RGB image: every bilinear tap is converted to saturated u8 RGB on the fly, so the
// output is, bit for bit, kodhip_letterbox_batch's for the RGB image the colour conversion of the whole frame would give.
// (the record, the colour conversion and the pixel fetch: kodhip_frame.h)
#include "kodhip_frame.h"

namespace {

// kodhip_resize.h's letterbox body over the frames.  The record (and with it the format) is uniform over a block, so the format
// switch does not diverge.
// grid: (ceil(H * W/2 / 256), B)
__global__ __launch_bounds__(256) void letterbox_frames_kernel(const KodFrameDesc* __restrict__ descs, float* __restrict__ out_f32,
                                                               bf16_t* __restrict__ out_pairs, int H, int W) {
  letterbox_thread(descs, out_f32, out_pairs, H, W, [](const KodFrameDesc& d, int dy, int xp, int px[2][3]) {
    switch (d.format) {
      case FMT_RGB24: letterbox_pair(d, dy, xp, FrameSource<FMT_RGB24>{d, {0, 0}}, px); break;
      case FMT_BGR24: letterbox_pair(d, dy, xp, FrameSource<FMT_BGR24>{d, {0, 0}}, px); break;
      case FMT_NV12: letterbox_pair(d, dy, xp, FrameSource<FMT_NV12>{d, {0, 0}}, px); break;
      case FMT_I420: letterbox_pair(d, dy, xp, FrameSource<FMT_I420>{d, {0, 0}}, px); break;
      default: break;                       // (an unknown format reads nothing: the frame stays grey)
    }
  });
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
