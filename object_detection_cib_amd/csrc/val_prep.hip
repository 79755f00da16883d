// Validation pre-processing on the device: resize to the longest side + letter-box pad + /255 + HWC -> CHW, one launch
// per batch, reading u8 source images from the pool in HBM, onto the image_size square or any H x W canvas (rectangular
// inference / validation).  The kernel body is kodhip_resize.h's, shared with video.hip; this file supplies the pool source.
//
// Reference (per sample, DataLoader workers): SampleReader.__call__(letter_box=True)
//   kod/data/sample_reader.py:16-40   A.LongestMaxSize(S, cv2.INTER_LINEAR) + A.PadIfNeeded(S, S, BORDER_CONSTANT, 114)
//   kod/data/sample_reader.py:102-136 the call
//   kod/data/augmentations/albu.py:91-119  ValidationSampleAugmentor: A.ToFloat(255) + ToTensorV2 (HWC -> CHW)
// cv2.resize(INTER_LINEAR) on 8-bit images is OpenCV's fixed-point path (resize.cpp): 11-bit horizontal and vertical
// weights, intermediate rows in int32, dst = ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2.  The geometry (new
// size, pads, the two double-precision scales) is computed on the host exactly as the libraries do
// (data/device_pipeline.py) and passed per sample.
#include "kodhip_resize.h"      // lin_coeff, letterbox_pair, letterbox_thread (shared with video.hip)

namespace {

struct ValDesc {
  long off;                 // byte offset of the source image in the pool (HWC u8)
  int h, w;                 // source size
  int nh, nw;               // size after LongestMaxSize
  int top, left;            // PadIfNeeded offsets
  double scale_x, scale_y;  // source / destination (1 / inv_scale as OpenCV computes it)
};

// The pool as letterbox source: a pixel's three channel bytes as ONE unaligned 4-byte load (the byte behind them is the next
// pixel, the next image or the pool's slack: kodhip_letterbox_batch's contract)
struct PoolSource {
  const unsigned char* img;   // the image's first byte
  int pitch;                  // bytes per row
  const unsigned char* row[2];
  __device__ __forceinline__ void rows(int r0, int r1) {
    row[0] = img + (long)r0 * pitch;
    row[1] = img + (long)r1 * pitch;
  }
  __device__ __forceinline__ unsigned px(int i, int c) const {
    unsigned q;
    __builtin_memcpy(&q, row[i] + c * 3, 4);
    return q;
  }
};

// The letterbox on an H x W canvas (validation, Detector, rectangular or square): kodhip_resize.h's body over the pool.
// grid: (ceil(H * W/2 / 256), B)
__global__ __launch_bounds__(256) void letterbox_kernel(const unsigned char* __restrict__ pool, const ValDesc* __restrict__ descs,
                                                        float* __restrict__ out_f32, bf16_t* __restrict__ out_pairs, int H, int W) {
  letterbox_thread(descs, out_f32, out_pairs, H, W, [&](const ValDesc& d, int dy, int xp, int px[2][3]) {
    letterbox_pair(d, dy, xp, PoolSource{pool + d.off, d.w * 3, {nullptr, nullptr}}, px);
  });
}

// the argument checks and the launch of both entry points; `name` is the entry's, for the error text
int letterbox_launch(const char* name, const void* pool, const void* descs, float* out_f32, void* out_pairs, int B, int H, int W,
                     hipStream_t stream) {
  KOD_CHECK_ARG(pool && descs && (out_f32 || out_pairs) && B > 0 && B <= 65535 && H > 0 && W > 0 && W % 2 == 0 &&
                    (long)H * W <= (1L << 30),
                "%s: bad args (W must be even)", name);
  KOD_CHECK_ARG(((uintptr_t)out_f32 % 8) == 0 && ((uintptr_t)out_pairs % 16) == 0,
                "%s: out_f32 must be 8-byte aligned, out_pairs 16-byte aligned", name);
  hipLaunchKernelGGL(letterbox_kernel, dim3(cdiv((long)H * (W / 2), 256), B), dim3(256), 0, stream, (const unsigned char*)pool,
                     (const ValDesc*)descs, out_f32, (bf16_t*)out_pairs, H, W);
  KOD_LAUNCH_CHECK(name);
  return KOD_OK;
}

}  // namespace

extern "C" {

int kodhip_val_prep_desc_bytes(void) { return (int)sizeof(ValDesc); }

// pool: u8 source images (HWC), followed by at least 1 readable byte behind the last image (ImagePool leaves 8); descs: device
// [B] ValDesc, top / left relative to the canvas; out_f32 [B,3,H,W] (8-byte aligned) and/or out_pairs (bf16 [B,H,W/2,8], 16-byte
// aligned); B <= 65535.
int kodhip_letterbox_batch(const void* pool, const void* descs, float* out_f32, void* out_pairs, int B, int H, int W,
                           hipStream_t stream) {
  return letterbox_launch("letterbox_batch", pool, descs, out_f32, out_pairs, B, H, W, stream);
}

// The S x S square: kodhip_letterbox_batch with H = W = S, under the same contract.
int kodhip_val_prep_batch(const void* pool, const void* descs, float* out_f32, void* out_pairs, int B, int S,
                          hipStream_t stream) {
  return letterbox_launch("val_prep_batch", pool, descs, out_f32, out_pairs, B, S, S, stream);
}

}  // extern "C"
