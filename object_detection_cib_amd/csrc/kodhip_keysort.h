// The 64-bit key sort shared by the NMS (postproc.hip) and the cross-tile merge (tiles.hip): keys are
// sortable_desc(score) << 32 | candidate index, so that an ascending sort lists the best score first and equal scores by
// candidate index.  Everything here has internal linkage: each translation unit that includes the header gets its own
// kernels, and postproc.hip's launches are what they were when the code lived there.
#pragma once
#include "kodhip_common.h"

namespace {

struct NmsArgs {
  const float* det;      // [B][rows][5+nc]
  unsigned long long* keys;   // [B][kcap]  (power of two capacity)
  int* ncand;            // [B]
  float* out;            // [B][max_det][6]
  int* nout;             // [B]
  int B, rows, nc, kcap, max_det, max_nms;
  float conf, iou_thr, max_wh;
};

__device__ __forceinline__ unsigned int sortable_desc(float s) {
  // positive floats: bit pattern is monotonic; invert for descending order under an ascending sort
  return 0xFFFFFFFFu - __float_as_uint(s);
}

// ---- sort of the candidate keys (ascending = best score first, ties by candidate index) ------------------------
// Bitonic network over npad_b = next power of two >= ncand[b] keys per image, spread over the whole chip instead of
// one block per image: the passes with partner distance < SORT_CHUNK run inside LDS (one block per 4096-key chunk),
// the few passes with a longer distance are one launch each.  An image whose candidate count is small leaves every
// block beyond its padded length (and every pass beyond its size) immediately, so a trained network (hundreds of
// candidates) costs one LDS sort per image, while the random-init worst case (252 000 candidates) uses all CUs.
// The kernels read a.keys, a.kcap and a.ncand only.
constexpr int SORT_CHUNK = 4096;          // keys per block (32 KB of LDS), 512 threads x 8 keys

__device__ __forceinline__ int npad_of(int n) {
  int npad = 64;
  while (npad < n) npad <<= 1;
  return npad;
}

// pad [n, npad) with +inf keys, then sort every SORT_CHUNK-sized chunk completely (k = 2 .. SORT_CHUNK), directions
// taken from the GLOBAL element index so that the chunks form the bitonic sequences the later merge passes expect
__global__ __launch_bounds__(512) void nms_sort_local_kernel(NmsArgs a) {
  __shared__ unsigned long long sk[SORT_CHUNK];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int n = a.ncand[b];
  const int npad = npad_of(n);
  const int base = chunk * SORT_CHUNK;
  if (base >= npad) return;
  unsigned long long* K = a.keys + (size_t)b * a.kcap;
  const int len = npad - base < SORT_CHUNK ? npad - base : SORT_CHUNK;      // power of two
  for (int i = tid; i < len; i += 512) sk[i] = (base + i < n) ? K[base + i] : ~0ull;
  __syncthreads();
  for (int k = 2; k <= len; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (len >> 1); t += 512) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // lower index of pair t
        const int p = i | j;
        unsigned long long x = sk[i], y = sk[p];
        const bool up = ((base + i) & k) == 0;
        if ((x > y) == up) { sk[i] = y; sk[p] = x; }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < len; i += 512) K[base + i] = sk[i];
}

// one pass (k, j) with j >= SORT_CHUNK: partner pairs straight in global memory (L2-resident), one pair per thread
__global__ __launch_bounds__(256) void nms_sort_global_kernel(NmsArgs a, int k, int j) {
  const int b = blockIdx.y;
  const int npad = npad_of(a.ncand[b]);
  if (k > npad) return;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= (npad >> 1)) return;
  unsigned long long* K = a.keys + (size_t)b * a.kcap;
  const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
  const int p = i | j;
  unsigned long long x = K[i], y = K[p];
  const bool up = (i & k) == 0;
  if ((x > y) == up) { K[i] = y; K[p] = x; }
}

// the passes j = SORT_CHUNK/2 .. 1 of merge size k (k > SORT_CHUNK) inside LDS
__global__ __launch_bounds__(512) void nms_sort_merge_kernel(NmsArgs a, int k) {
  __shared__ unsigned long long sk[SORT_CHUNK];
  const int b = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;
  const int npad = npad_of(a.ncand[b]);
  const int base = chunk * SORT_CHUNK;
  if (k > npad || base >= npad) return;
  unsigned long long* K = a.keys + (size_t)b * a.kcap;
  for (int i = tid; i < SORT_CHUNK; i += 512) sk[i] = K[base + i];
  __syncthreads();
  const bool up = (base & k) == 0;                 // k > SORT_CHUNK: one direction per chunk
  for (int j = SORT_CHUNK >> 1; j > 0; j >>= 1) {
    for (int t = tid; t < (SORT_CHUNK >> 1); t += 512) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
      const int p = i | j;
      unsigned long long x = sk[i], y = sk[p];
      if ((x > y) == up) { sk[i] = y; sk[p] = x; }
    }
    __syncthreads();
  }
  for (int i = tid; i < SORT_CHUNK; i += 512) K[base + i] = sk[i];
}

// the launches that sort a.keys[b][0 .. a.ncand[b]) for b < B (a.kcap keys of workspace per image)
inline void key_sort_launch(const NmsArgs& a, int B, hipStream_t stream) {
  const int key_cap = a.kcap;
  const int chunks = key_cap > SORT_CHUNK ? key_cap / SORT_CHUNK : 1;
  hipLaunchKernelGGL(nms_sort_local_kernel, dim3(chunks, B), dim3(512), 0, stream, a);
  for (int k = 2 * SORT_CHUNK; k <= key_cap; k <<= 1) {
    for (int j = k >> 1; j >= SORT_CHUNK; j >>= 1)
      hipLaunchKernelGGL(nms_sort_global_kernel, dim3(cdiv(key_cap / 2, 256), B), dim3(256), 0, stream, a, k, j);
    hipLaunchKernelGGL(nms_sort_merge_kernel, dim3(chunks, B), dim3(512), 0, stream, a, k);
  }
}

}  // namespace
