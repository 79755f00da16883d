// The validation letterbox (OpenCV's fixed-point INTER_LINEAR on 8-bit images, padding 114, / 255.f, a copy path when nothing
// is resized) as ONE kernel body for the letterbox kernels of val_prep.hip (images in the pool) and video.hip (frames where
// they lie): a kernel supplies its record type and how a source pixel is fetched, everything else is here.
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

// The body in two steps, for a record Desc with h, w, nh, nw, scale_x, scale_y (ValDesc, KodFrameDesc, crops.hip's view of a
// cutout) and a source Src - src.rows(r0, r1) names the two source rows of this thread (both in [0, h)), then src.px(i, c) is
// pixel (row i = 0 | 1, column c in [0, w)) as u8 r | g << 8 | b << 16 (higher bits are ignored).
//
// letterbox_rows: row dy of the resized image -> its source rows and their 11-bit weights (the copy path: the row itself).
template <typename Desc>
__device__ __forceinline__ void letterbox_rows(const Desc& d, bool copy, int dy, int& r0, int& r1, int& b0, int& b1) {
  r0 = dy; r1 = dy; b0 = 0; b1 = 0;
  if (!copy) {
    int sy;
    lin_coeff(dy, d.scale_y, d.h, false, sy, b0, b1);
    r0 = min(max(sy, 0), d.h - 1);
    r1 = min(max(sy + 1, 0), d.h - 1);
  }
}

// letterbox_px: column dx in [0, nw) of that row -> the pixel's three channels
template <typename Desc, typename Src>
__device__ __forceinline__ void letterbox_px(const Desc& d, bool copy, int dx, int b0, int b1, const Src& src, int px[3]) {
  if (copy) {
    const unsigned p = src.px(0, dx);
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (p >> (8 * c)) & 255;
  } else {
    int sx, a0, a1;
    lin_coeff(dx, d.scale_x, d.w, true, sx, a0, a1);
    const int sx1 = min(sx + 1, d.w - 1);
    const unsigned p00 = src.px(0, sx), p01 = src.px(0, sx1);
    const unsigned p10 = src.px(1, sx), p11 = src.px(1, sx1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int S0 = (int)((p00 >> (8 * c)) & 255) * a0 + (int)((p01 >> (8 * c)) & 255) * a1;
      const int S1 = (int)((p10 >> (8 * c)) & 255) * a0 + (int)((p11 >> (8 * c)) & 255) * a1;
      const int v = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
      px[c] = min(max(v, 0), 255);
    }
  }
}

// The two pixels of output pair xp of row dy of the resized image (d.nh x d.nw, `left` columns into the canvas); px keeps
// what it holds (the pad) where the image does not reach.
template <typename Desc, typename Src>
__device__ __forceinline__ void letterbox_pair(const Desc& d, int dy, int xp, Src src, int px[2][3]) {
  const bool copy = d.nh == d.h && d.nw == d.w;
  int r0, r1, b0, b1;
  letterbox_rows(d, copy, dy, r0, r1, b0, b1);
  src.rows(r0, r1);
#pragma unroll
  for (int k = 0; k < 2; ++k) {             // (`left` may be odd: each pixel of the pair decides for itself)
    const int dx = 2 * xp + k - d.left;
    if (dx < 0 || dx >= d.nw) continue;
    letterbox_px(d, copy, dx, b0, b1, src, px[k]);
  }
}

// One thread of a letterbox launch, grid (ceil(H * W/2 / 256), B): one pixel PAIR of a canvas row.  The index is flat over
// H * W/2, so a 64-wide canvas still fills its blocks; the record is uniform over a block.  fill(d, dy, xp, px) is called for
// the rows the image reaches and hands `letterbox_pair` its source; the pair leaves as u8 / 255.f through
// kod_store_input_pair (one 16-byte store into the pair layout, one 8-byte store per fp32 plane).
template <typename Desc, typename Fill>
__device__ __forceinline__ void letterbox_thread(const Desc* __restrict__ descs, float* __restrict__ out_f32,
                                                 bf16_t* __restrict__ out_pairs, int H, int W, Fill&& fill) {
  const int b = blockIdx.y;
  const int Wp = W >> 1;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= H * Wp) return;
  const int y = q / Wp, xp = q - y * Wp;
  const Desc d = descs[b];
  int px[2][3] = {{114, 114, 114}, {114, 114, 114}};
  const int dy = y - d.top;
  if (dy >= 0 && dy < d.nh) fill(d, dy, xp, px);
  float v[2][3];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[k][c] = (float)px[k][c] / 255.f;
  kod_store_input_pair(out_f32, out_pairs, b, y, xp, H, W, v);
}
