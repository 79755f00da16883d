// Tiled (sliced) inference for images larger than the network's input: the image stays at its native resolution, overlapping
// S x S tiles go through the network, and the boxes found in all tiles (and in one letterboxed view of the whole image)
// are merged in full-image coordinates.
//
//   tile_batch       : slot t = the S x S window of a u8 HWC pool image with its corner at (x0, y0), as fp32 [T][3][S][S]
//                      and / or as the network's bf16 pixel pairs [T][S][S/2][8].  A pixel inside the image is (float)u8 / 255.f,
//                      a pixel outside it 114 / 255.f - the values of the letterbox (kodhip_resize.h), so a tile is
//                      bit-identical to a letterbox at scale 1.
//   merge_detections : one greedy pass per image over the rows kodhip_nms_ex kept in each of its views (already in image
//                      pixels).  Classes are compared directly - there is no class offset, which in fp32 costs ulps that
//                      grow with the class index and collides classes once coordinates pass max_wh = 4096 px.  Two
//                      metrics: IoU, and intersection over the smaller area (IoS), which is 1 for the part of an object
//                      that a tile border cut off inside the whole box from the neighbouring tile.  Two modes: NMS (the
//                      absorbed row is dropped) and non-maximum merging (NMM: the keeper's box grows to the hull of what
//                      it absorbs).
//
// The merge in the order the definition gives it - sorted candidates; a candidate not yet absorbed is kept and absorbs
// every later candidate, not yet absorbed, that matches its ORIGINAL box - is computed candidate by candidate: a
// candidate is absorbed by the FIRST keeper (in keep order) that matches it, and is kept when none does and fewer than
// max_det rows are kept.  Both say the same: keeper k meets candidate c exactly when no keeper before k absorbed c.
// Candidates are taken in batches of one per thread and tested against the keepers in LDS; then the batch is resolved wave
// by wave (a wave keeps its live candidates in order, the waves behind it meet the new keepers after one barrier).  Hulls
// are min / max of fp32 values - exact, and independent of the order they are taken in - formed with integer LDS atomics
// on an order-preserving image of the bits (no floating-point atomics).
#include "kodhip_common.h"
#include "kodhip_keysort.h"

#define KOD_MERGE_MAX_ROWS 65536          // candidates per image (the key workspace and the 32-bit slot index allow more;
                                          // the limit keeps the sort to sixteen 4096-key chunks per image)

namespace {

// ------------------------------------------------------------------------------------------------------ tile_batch
struct TileDesc {
  long off;                 // byte offset of the source image in the pool (HWC u8)
  int h, w;                 // source size
  int x0, y0;               // the window's corner in the source image
};

// PX pixels of one row per thread (PX = 4: 16-byte fp32 stores; PX = 2 for S % 4 == 2: 8-byte).  grid: (ceil(S * S/PX / 256), T)
template <int PX>
__global__ __launch_bounds__(256) void tile_batch_kernel(const unsigned char* __restrict__ pool, const TileDesc* __restrict__ descs,
                                                         float* __restrict__ out_f32, bf16_t* __restrict__ out_pairs, int S) {
  const int t = blockIdx.y;
  const int Sq = S / PX;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S * Sq) return;
  const int y = i / Sq, x = (i - y * Sq) * PX;
  const TileDesc d = descs[t];
  const int sy = d.y0 + y, sx = d.x0 + x;
  int px[PX * 3];
#pragma unroll
  for (int k = 0; k < PX * 3; ++k) px[k] = 114;
  if (sy >= 0 && sy < d.h) {
    const unsigned char* img = pool + d.off;
    const unsigned char* src = img + ((long)sy * d.w + sx) * 3;
    // the PX * 3 bytes as aligned 4-byte words when they all lie in the row and the words stay inside the image
    const unsigned char* lo = src - ((uintptr_t)src & 3);
    const int sh = (int)((uintptr_t)src & 3) * 8;
    constexpr int WORDS = (PX * 3 + 3 + 3) / 4;          // PX * 3 bytes starting at byte 0 .. 3 of the first word
    if (sx >= 0 && sx + PX <= d.w && lo >= img && lo + 4 * WORDS <= img + (long)d.h * d.w * 3) {
      unsigned int wd[WORDS];
#pragma unroll
      for (int k = 0; k < WORDS; ++k) wd[k] = reinterpret_cast<const unsigned int*>(lo)[k];
#pragma unroll
      for (int k = 0; k < PX * 3; ++k) {
        // byte sh / 8 + k lies in word k / 4 or the next one: a 64-bit shift over the two keeps the word index constant
        const unsigned long long two = (unsigned long long)wd[k / 4] | ((unsigned long long)wd[k / 4 + 1] << 32);
        px[k] = (int)((two >> (sh + 8 * (k % 4))) & 0xFF);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        if (sx + p >= 0 && sx + p < d.w) {
#pragma unroll
          for (int c = 0; c < 3; ++c) px[p * 3 + c] = src[p * 3 + c];
        }
      }
    }
  }
  float v[PX][3];
#pragma unroll
  for (int p = 0; p < PX; ++p)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[p][c] = (float)px[p * 3 + c] / 255.f;
  if (out_f32) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = out_f32 + ((size_t)(t * 3 + c) * S + y) * S + x;
      if (PX == 4) *reinterpret_cast<float4*>(o) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
      else *reinterpret_cast<float2*>(o) = make_float2(v[0][c], v[1][c]);
    }
  }
  if (out_pairs) {   // network input layout [T][S][S/2][8] = pixel pairs x 4 channels
#pragma unroll
    for (int q = 0; q < PX / 2; ++q) {
      bf16x8 o;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[4 * k + c] = (bf16_t)v[2 * q + k][c];
        o[4 * k + 3] = (bf16_t)0.f;
      }
      *reinterpret_cast<bf16x8*>(out_pairs + ((size_t)(t * S + y) * S + x + 2 * q) * 4) = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------ merge_detections
struct MergeArgs {
  const float* rows;          // [V][max_rows][6]
  const int* counts;          // [V]
  const int* view_start;      // [n_images + 1]
  unsigned long long* keys;   // [n_images][kcap]
  float* out;                 // [n_images][max_det][6]
  int* nout;                  // [n_images]: the candidate count between the launches, the kept count at the end
  int kcap, max_rows, max_det, metric, mode, agnostic;
  float thr;
};

constexpr int MERGE_THREADS = 1024;
constexpr int MERGE_MAX_DET = 300;

__device__ __forceinline__ int merge_count(const MergeArgs& a, int v) { return min(max(a.counts[v], 0), a.max_rows); }

// keys of image b's candidates, in (view, rank) order: the low word is the candidate's slot (view - first view) * max_rows +
// rank, which orders like its position among the valid rows and leads back to the row without a search.  Rows at or
// beyond a view's count are not read.
__global__ __launch_bounds__(MERGE_THREADS) void merge_candidates_kernel(MergeArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int v0 = a.view_start[b], v1 = a.view_start[b + 1];
  unsigned long long* K = a.keys + (size_t)b * a.kcap;
  int base = 0;
  for (int v = v0; v < v1; ++v) {
    const long slot0 = (long)(v - v0) * a.max_rows;
    if (slot0 >= a.kcap) break;                                   // (key_cap below views * max_rows: the views that fit)
    const int c = min(merge_count(a, v), (int)(a.kcap - slot0));  // base <= slot0: base + r stays below key_cap
    for (int r = tid; r < c; r += MERGE_THREADS)
      K[base + r] = ((unsigned long long)sortable_desc(a.rows[((size_t)v * a.max_rows + r) * 6 + 4]) << 32) | (unsigned int)(slot0 + r);
    base += c;
  }
  if (tid == 0) a.nout[b] = base;
}

// does keeper (box A, area aa) absorb candidate (box B, area ab)?  inter as in the NMS's iou_gt; a 0 / 0 is NaN: no match.
// An empty intersection never matches (0 / x is 0, -0 or NaN, none above thr >= 0), so it skips the division.
__device__ __forceinline__ bool merge_match(const float4 A, float aa, const float* Bx, float ab, int metric, float thr) {
  float xx1 = fmaxf(A.x, Bx[0]), yy1 = fmaxf(A.y, Bx[1]);
  float xx2 = fminf(A.z, Bx[2]), yy2 = fminf(A.w, Bx[3]);
  float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  float inter = w * h;
  if (!(inter > 0.f)) return false;
  float m = metric ? inter / fminf(aa, ab) : inter / (aa + ab - inter);
  return m > thr;
}

// fp32 <-> unsigned with the same order (for finite values and infinities), so that a hull's min / max can be taken with
// integer LDS atomics: exact, and the same whatever order the absorbed boxes arrive in
__device__ __forceinline__ unsigned int ordered_u32(float f) {
  const unsigned int u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ordered_f32(unsigned int e) {
  return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e);
}

// one block per image.  Per batch of MERGE_THREADS sorted candidates (one per thread, wave w holds the w-th 64 of them):
//   1. every candidate meets the keepers of the earlier batches, first match wins;
//   2. wave after wave: wave w keeps, in order, its candidates that are still alive (each new keeper meets the wave's
//      later candidates at once, by shuffles), publishes the new keepers, and after one barrier the waves behind it let
//      their live candidates meet them.
__global__ __launch_bounds__(MERGE_THREADS) void merge_greedy_kernel(MergeArgs a) {
  __shared__ float4 kb[MERGE_MAX_DET];               // the keepers' original boxes
  __shared__ float2 kac[MERGE_MAX_DET];              // area, class
  __shared__ float ks[MERGE_MAX_DET];
  __shared__ unsigned int hull[MERGE_MAX_DET][4];    // NMM: min x1, min y1, max x2, max y2 as ordered_u32
  __shared__ int nk_s[2];
  constexpr int WAVES = MERGE_THREADS / 64;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v0 = a.view_start[b];
  const unsigned long long* K = a.keys + (size_t)b * a.kcap;
  const int n = a.nout[b];                     // (written by merge_candidates_kernel; every thread reads it before the end)
  const bool nmm = a.mode == 1, agn = a.agnostic != 0;
  int nk = 0;
  for (int base = 0; base < n; base += MERGE_THREADS) {
    if (!nmm && nk >= a.max_det) break;                 // NMS: nothing left to decide.  NMM: the keepers still absorb
    const int i = base + tid;
    bool alive = i < n;
    float box[4] = {0, 0, 0, 0}, area = 0.f, score = 0.f, cls = 0.f;
    int by = -1;
    if (alive) {
      const unsigned int slot = (unsigned int)K[i];
      const int v = slot / a.max_rows, r = slot - v * a.max_rows;
      const float* row = a.rows + ((size_t)(v0 + v) * a.max_rows + r) * 6;
#pragma unroll
      for (int k = 0; k < 4; ++k) box[k] = row[k];
      score = row[4]; cls = row[5];
      area = (box[2] - box[0]) * (box[3] - box[1]);
      for (int k0 = 0; k0 < nk && by < 0; k0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + u;
          if (k < nk && by < 0) {
            const float4 kk = kb[k];
            const float2 ac = kac[k];
            if ((agn || ac.y == cls) && merge_match(kk, ac.x, box, area, a.metric, a.thr)) by = k;
          }
        }
      }
      alive = by < 0;
    }
    for (int w = 0; w < WAVES && base + w * 64 < n; ++w) {
      const int nk0 = nk;
      if (nk0 >= a.max_det) break;                      // (block-uniform) the candidates still alive are dropped
      if (wave == w) {
        int mk = nk0;
        unsigned long long mask = __ballot(alive);
        while (mask && mk < a.max_det) {
          const int j = __ffsll((long long)mask) - 1;   // the wave's earliest candidate still alive: kept
          float4 jb;
          jb.x = __shfl(box[0], j, 64); jb.y = __shfl(box[1], j, 64); jb.z = __shfl(box[2], j, 64); jb.w = __shfl(box[3], j, 64);
          const float jarea = __shfl(area, j, 64), jcls = __shfl(cls, j, 64);
          if (lane == j) {
            kb[mk] = jb; kac[mk] = make_float2(area, cls); ks[mk] = score;
#pragma unroll
            for (int k = 0; k < 4; ++k) hull[mk][k] = ordered_u32(box[k]);
            alive = false;
          }
          if (alive && lane > j && (agn || jcls == cls) && merge_match(jb, jarea, box, area, a.metric, a.thr)) { by = mk; alive = false; }
          ++mk;
          mask = __ballot(alive);
        }
        alive = false;                                  // (max_det reached inside the wave)
        if (lane == 0) nk_s[w & 1] = mk;
      }
      __syncthreads();
      nk = nk_s[w & 1];
      if (alive && wave > w) {
        for (int k = nk0; k < nk; ++k) {
          const float2 ac = kac[k];
          if ((agn || ac.y == cls) && merge_match(kb[k], ac.x, box, area, a.metric, a.thr)) { by = k; alive = false; break; }
        }
      }
    }
    if (nmm && by >= 0) {                               // (the keeper's own values were stored before the barrier that showed it)
      atomicMin(&hull[by][0], ordered_u32(box[0])); atomicMin(&hull[by][1], ordered_u32(box[1]));
      atomicMax(&hull[by][2], ordered_u32(box[2])); atomicMax(&hull[by][3], ordered_u32(box[3]));
    }
    __syncthreads();
  }
  __syncthreads();
  float* O = a.out + (size_t)b * a.max_det * 6;
  for (int k = tid; k < nk; k += MERGE_THREADS) {
    const float4 kk = kb[k];
    O[k * 6 + 0] = nmm ? ordered_f32(hull[k][0]) : kk.x;
    O[k * 6 + 1] = nmm ? ordered_f32(hull[k][1]) : kk.y;
    O[k * 6 + 2] = nmm ? ordered_f32(hull[k][2]) : kk.z;
    O[k * 6 + 3] = nmm ? ordered_f32(hull[k][3]) : kk.w;
    O[k * 6 + 4] = ks[k];
    O[k * 6 + 5] = kac[k].y;
  }
  if (tid == 0) a.nout[b] = nk;
}

}  // namespace

extern "C" {

int kodhip_tile_desc_bytes(void) { return (int)sizeof(TileDesc); }

// pool: u8 source images (HWC); descs: device [T] { long off; int h, w, x0, y0; }; out_f32 [T,3,S,S] and/or out_pairs
// (bf16 [T,S,S/2,8]), both 16-byte aligned.
int kodhip_tile_batch(const void* pool, const void* descs, float* out_f32, void* out_pairs, int T, int S, hipStream_t stream) {
  KOD_CHECK_ARG(pool && descs, "tile_batch: null pool or descs");
  KOD_CHECK_ARG(out_f32 || out_pairs, "tile_batch: both outputs are null");
  KOD_CHECK_ARG(T >= 1 && S >= 2 && S % 2 == 0, "tile_batch: T must be >= 1 and S even and >= 2");
  KOD_CHECK_ARG((((uintptr_t)out_f32 | (uintptr_t)out_pairs) & 15) == 0, "tile_batch: outputs must be 16-byte aligned");
  KOD_CHECK_ARG((long)T * S * S < (1l << 29) && T <= 65535, "tile_batch: batch too large");
  if (S % 4 == 0)
    hipLaunchKernelGGL(tile_batch_kernel<4>, dim3(cdiv((long)S * (S / 4), 256), T), dim3(256), 0, stream, (const unsigned char*)pool,
                       (const TileDesc*)descs, out_f32, (bf16_t*)out_pairs, S);
  else
    hipLaunchKernelGGL(tile_batch_kernel<2>, dim3(cdiv((long)S * (S / 2), 256), T), dim3(256), 0, stream, (const unsigned char*)pool,
                       (const TileDesc*)descs, out_f32, (bf16_t*)out_pairs, S);
  KOD_LAUNCH_CHECK("tile_batch");
  return KOD_OK;
}

int kodhip_merge_max_rows(void) { return KOD_MERGE_MAX_ROWS; }

// rows [V][max_rows][6] (x1, y1, x2, y2, score, class; kodhip_nms_ex's `out`, in image pixels), counts [V], the views of
// image i are view_start[i] .. view_start[i + 1]; keys: n_images * key_cap u64 workspace; out [n_images][max_det][6], nout [n_images].
int kodhip_merge_detections(const float* rows, const int* counts, const int* view_start, void* keys, int key_cap, float* out,
                            int* nout, int n_images, int max_rows, int max_det, int metric, float thr, int mode, int agnostic,
                            hipStream_t stream) {
  KOD_CHECK_ARG(rows && counts && view_start && keys && out && nout, "merge_detections: null pointer");
  KOD_CHECK_ARG(n_images >= 1 && n_images <= 65535 && max_rows >= 1, "merge_detections: n_images must be in 1..65535, max_rows >= 1");
  KOD_CHECK_ARG(max_det >= 1 && max_det <= MERGE_MAX_DET, "merge_detections: max_det must be in 1..300");
  KOD_CHECK_ARG(metric == 0 || metric == 1, "merge_detections: metric must be 0 (IoU) or 1 (IoS)");
  KOD_CHECK_ARG(mode == 0 || mode == 1, "merge_detections: mode must be 0 (NMS) or 1 (NMM)");
  KOD_CHECK_ARG(agnostic == 0 || agnostic == 1, "merge_detections: agnostic must be 0 or 1");
  KOD_CHECK_ARG(thr >= 0.f && thr <= 1.f, "merge_detections: thr must be in [0, 1]");
  KOD_CHECK_ARG(key_cap >= 64 && (key_cap & (key_cap - 1)) == 0 && key_cap <= KOD_MERGE_MAX_ROWS,
                "merge_detections: key_cap must be a power of two in 64..%d", KOD_MERGE_MAX_ROWS);
  MergeArgs a = {};
  a.rows = rows; a.counts = counts; a.view_start = view_start; a.keys = (unsigned long long*)keys; a.out = out; a.nout = nout;
  a.kcap = key_cap; a.max_rows = max_rows; a.max_det = max_det; a.metric = metric; a.mode = mode; a.agnostic = agnostic;
  a.thr = thr;
  hipLaunchKernelGGL(merge_candidates_kernel, dim3(n_images), dim3(MERGE_THREADS), 0, stream, a);
  KOD_LAUNCH_CHECK("merge_candidates");
  NmsArgs s = {};
  s.keys = a.keys; s.ncand = nout; s.kcap = key_cap;
  key_sort_launch(s, n_images, stream);
  KOD_LAUNCH_CHECK("merge_sort");
  hipLaunchKernelGGL(merge_greedy_kernel, dim3(n_images), dim3(MERGE_THREADS), 0, stream, a);
  KOD_LAUNCH_CHECK("merge_greedy");
  return KOD_OK;
}

}  // extern "C"
