// Validation pre-processing on the device: resize to the longest side + letter-box pad + /255 + HWC -> CHW, one launch
// per batch, reading u8 source images from the pool in HBM.
//
// Reference (per sample, DataLoader workers): SampleReader.__call__(letter_box=True)
//   kod/data/sample_reader.py:16-40   A.LongestMaxSize(S, cv2.INTER_LINEAR) + A.PadIfNeeded(S, S, BORDER_CONSTANT, 114)
//   kod/data/sample_reader.py:102-136 the call
//   kod/data/augmentations/albu.py:91-119  ValidationSampleAugmentor: A.ToFloat(255) + ToTensorV2 (HWC -> CHW)
// cv2.resize(INTER_LINEAR) on 8-bit images is OpenCV's fixed-point path (resize.cpp): 11-bit horizontal and vertical
// weights, intermediate rows in int32, dst = ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2.  The geometry (new
// size, pads, the two double-precision scales) is computed on the host exactly as the libraries do
// (data/device_pipeline.py) and passed per sample.
#include "kodhip_resize.h"      // sat16, lin_coeff (shared with video.hip)

namespace {

struct ValDesc {
  long off;                 // byte offset of the source image in the pool (HWC u8)
  int h, w;                 // source size
  int nh, nw;               // size after LongestMaxSize
  int top, left;            // PadIfNeeded offsets
  double scale_x, scale_y;  // source / destination (1 / inv_scale as OpenCV computes it)
};

// grid: (ceil(S*S/256), B)
__global__ __launch_bounds__(256) void val_prep_kernel(const unsigned char* pool, const ValDesc* descs, float* out_f32,
                                                       bf16_t* out_pairs, int S) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= S * S) return;
  const int y = p / S, x = p - y * S;
  const ValDesc d = descs[b];
  int px[3] = {114, 114, 114};
  const int dy = y - d.top, dx = x - d.left;
  if (dy >= 0 && dy < d.nh && dx >= 0 && dx < d.nw) {
    const unsigned char* src = pool + d.off;
    if (d.nh == d.h && d.nw == d.w) {
#pragma unroll
      for (int c = 0; c < 3; ++c) px[c] = src[((long)dy * d.w + dx) * 3 + c];
    } else {
      int sx, a0, a1, sy, b0, b1;
      lin_coeff(dx, d.scale_x, d.w, true, sx, a0, a1);
      lin_coeff(dy, d.scale_y, d.h, false, sy, b0, b1);
      const int sx1 = min(sx + 1, d.w - 1);
      const int r0 = min(max(sy, 0), d.h - 1), r1 = min(max(sy + 1, 0), d.h - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int S0 = src[((long)r0 * d.w + sx) * 3 + c] * a0 + src[((long)r0 * d.w + sx1) * 3 + c] * a1;
        const int S1 = src[((long)r1 * d.w + sx) * 3 + c] * a0 + src[((long)r1 * d.w + sx1) * 3 + c] * a1;
        const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
        px[c] = min(max(v, 0), 255);
      }
    }
  }
  float v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = (float)px[c] / 255.f;
  if (out_f32) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out_f32[((size_t)(b * 3 + c) * S + y) * S + x] = v[c];
  }
  if (out_pairs) {   // network input layout [B][S][S/2][8] = pixel pairs x 4 channels
    bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)0.f};
    *reinterpret_cast<bf16x4*>(out_pairs + ((size_t)(b * S + y) * S + x) * 4) = o;
  }
}

// a pixel's three channel bytes as ONE unaligned 4-byte load (the byte behind them is the next pixel, the next image or the
// pool's slack: kodhip_letterbox_batch's contract)
__device__ __forceinline__ unsigned load_px(const unsigned char* p) {
  unsigned q;
  __builtin_memcpy(&q, p, 4);
  return q;
}

// The letterbox on an H x W canvas (rectangular inference / validation): val_prep_kernel's arithmetic, one thread per pixel
// PAIR of a row.  The vertical coefficients and the two source rows are found once per thread, each tap is one 4-byte load,
// the pair leaves as one 16-byte store into the pair layout and one 8-byte store per fp32 plane (a wave writes 1 KiB / 512
// contiguous bytes per row segment).  The index is flat over H * W/2, so a 64-wide canvas still fills its blocks.
// grid: (ceil(H * W/2 / 256), B)
__global__ __launch_bounds__(256) void letterbox_kernel(const unsigned char* __restrict__ pool, const ValDesc* __restrict__ descs,
                                                        float* __restrict__ out_f32, bf16_t* __restrict__ out_pairs, int H, int W) {
  const int b = blockIdx.y;
  const int Wp = W >> 1;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= H * Wp) return;
  const int y = q / Wp, xp = q - y * Wp;
  const ValDesc d = descs[b];
  int px[2][3] = {{114, 114, 114}, {114, 114, 114}};
  const int dy = y - d.top;
  if (dy >= 0 && dy < d.nh) {
    const unsigned char* src = pool + d.off;
    const bool copy = d.nh == d.h && d.nw == d.w;
    const unsigned char *row0, *row1;
    int b0 = 0, b1 = 0;
    if (copy) {
      row0 = row1 = src + (long)dy * d.w * 3;
    } else {
      int sy;
      lin_coeff(dy, d.scale_y, d.h, false, sy, b0, b1);
      row0 = src + (long)min(max(sy, 0), d.h - 1) * d.w * 3;
      row1 = src + (long)min(max(sy + 1, 0), d.h - 1) * d.w * 3;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {           // (`left` may be odd: each pixel of the pair decides for itself)
      const int dx = 2 * xp + k - d.left;
      if (dx < 0 || dx >= d.nw) continue;
      if (copy) {
        const unsigned p = load_px(row0 + dx * 3);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[k][c] = (p >> (8 * c)) & 255;
      } else {
        int sx, a0, a1;
        lin_coeff(dx, d.scale_x, d.w, true, sx, a0, a1);
        const int sx1 = min(sx + 1, d.w - 1);
        const unsigned p00 = load_px(row0 + sx * 3), p01 = load_px(row0 + sx1 * 3);
        const unsigned p10 = load_px(row1 + sx * 3), p11 = load_px(row1 + sx1 * 3);
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
    *reinterpret_cast<bf16x8*>(out_pairs + ((size_t)(b * H + y) * Wp + xp) * 8) = o;
  }
}

}  // namespace

extern "C" {

int kodhip_val_prep_desc_bytes(void) { return (int)sizeof(ValDesc); }

// pool: u8 source images (HWC); descs: device [B] ValDesc; out_f32 [B,3,S,S] and/or out_pairs (bf16 [B,S,S/2,8]).
int kodhip_val_prep_batch(const void* pool, const void* descs, float* out_f32, void* out_pairs, int B, int S,
                          hipStream_t stream) {
  KOD_CHECK_ARG(pool && descs && (out_f32 || out_pairs) && B > 0 && S > 0 && S % 2 == 0, "val_prep_batch: bad args");
  hipLaunchKernelGGL(val_prep_kernel, dim3(cdiv((long)S * S, 256), B), dim3(256), 0, stream, (const unsigned char*)pool,
                     (const ValDesc*)descs, out_f32, (bf16_t*)out_pairs, S);
  KOD_LAUNCH_CHECK("val_prep_batch");
  return KOD_OK;
}

// The same records on an H x W canvas (top / left relative to it): out_f32 [B,3,H,W] and/or out_pairs (bf16 [B,H,W/2,8]).
// pool: followed by at least 1 readable byte behind the last image (ImagePool leaves 8).
int kodhip_letterbox_batch(const void* pool, const void* descs, float* out_f32, void* out_pairs, int B, int H, int W,
                           hipStream_t stream) {
  KOD_CHECK_ARG(pool && descs && (out_f32 || out_pairs) && B > 0 && B <= 65535 && H > 0 && W > 0 && W % 2 == 0 &&
                    (long)H * W <= (1L << 30),
                "letterbox_batch: bad args (W must be even)");
  KOD_CHECK_ARG(((uintptr_t)out_f32 % 8) == 0 && ((uintptr_t)out_pairs % 16) == 0,
                "letterbox_batch: out_f32 must be 8-byte aligned, out_pairs 16-byte aligned");
  hipLaunchKernelGGL(letterbox_kernel, dim3(cdiv((long)H * (W / 2), 256), B), dim3(256), 0, stream, (const unsigned char*)pool,
                     (const ValDesc*)descs, out_f32, (bf16_t*)out_pairs, H, W);
  KOD_LAUNCH_CHECK("letterbox_batch");
  return KOD_OK;
}

}  // extern "C"
