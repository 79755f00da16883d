// Weighted boxes fusion (WBF; Solovyev, Wang, Gabruseva 2021) for model ensembles: the views of an image are the members
// of an ensemble, which all see the same object, so their boxes are averaged and agreement raises a box's rank - unlike
// merge_detections (tiles.hip), whose views see different parts of an image.
//
//   candidates : a row of view v with score s is a candidate iff t = s * w[v] > 0 (drops zero, negative and NaN scores);
//                key = sortable_desc(t) << 32 | slot, slot = (view - first view) * max_rows + rank as in the cross-tile merge;
//                a row that is no candidate gets the high word 0xFFFFFFFF, which sorts behind every t > 0.
//   sort       : the bitonic key sort of kodhip_keysort.h (key_cap <= 4096: one LDS pass per image).
//   greedy pass: one block per image, candidate after candidate (each one meets fused boxes that the one before it may
//                have moved, so the pass is serial by definition).  The parallelism is across clusters: thread t scans
//                clusters t, t + 256, ..., the block reduces on (largest IoU, lowest cluster) - inside a wave by data-parallel
//                primitives, across the four waves through LDS - and the thread that OWNS the
//                chosen cluster (cluster % 256) updates it - the only thread that will read it in the next scan, so one
//                barrier per candidate suffices (the reduction slots alternate between two sets).  A candidate without a
//                match opens cluster nc, written by the thread that owns it.
//   ranking    : final score = (st / n) * (min(n, W) / W); the clusters' keys sortable_desc(score) << 32 | cluster are
//                sorted inside the block (bitonic, in the LDS the accumulators occupied) and the first max_det emitted.
//
// LDS per cluster: fused box 16 B + class 4 B (scanned by the owner), weighted coordinate sums 16 B (touched at a join);
// the sums of t and the member counts stay in the owner's registers (16 clusters per thread at most).  4096 clusters:
// 144 KiB + 6 KiB of staged candidates, of the 160 KiB a gfx950 workgroup may use; the launch asks for what key_cap needs.
// Every operation is fp32 and rounded on its own (the library is built with -ffp-contract=off).
#include "kodhip_common.h"
#include "kodhip_keysort.h"

#define KOD_FUSE_MAX_ROWS 4096            // candidates per image (13 models x 300 rows), = clusters an image can open

namespace {

struct FuseArgs {
  const float* rows;          // [V][max_rows][6]
  const int* counts;          // [V]
  const int* view_start;      // [n_images + 1]
  const float* weight;        // [V]
  unsigned long long* keys;   // [n_images][kcap]
  float* out;                 // [n_images][max_det][6]
  int* nout;                  // [n_images]: the slot count between the launches, the emitted count at the end
  int kcap, max_rows, max_det, agnostic;
  float thr;
};

constexpr int FUSE_THREADS = 256;
constexpr int FUSE_WAVES = FUSE_THREADS / 64;
constexpr int FUSE_SLICES = KOD_FUSE_MAX_ROWS / FUSE_THREADS;     // clusters a thread owns at most
constexpr int FUSE_MAX_DET = 300;
constexpr unsigned int FUSE_NO_CANDIDATE = 0xFFFFFFFFu;           // = sortable_desc(+0.f): behind every t > 0

// bytes of dynamic LDS for `cap` clusters: fused boxes, coordinate sums (later the ranking keys), classes, one batch of
// staged candidates (box, t, class), the two sets of reduction slots and W
constexpr size_t fuse_lds_bytes(int cap) {
  return (size_t)cap * (16 + 16 + 4) + FUSE_THREADS * (16 + 4 + 4) + 2 * FUSE_WAVES * 8 + 16;
}

// keys of image b's rows, in (view, rank) order (merge_candidates_kernel's slot scheme); rows at or beyond a view's count
// are not read
__global__ __launch_bounds__(FUSE_THREADS) void fuse_candidates_kernel(FuseArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int v0 = a.view_start[b], v1 = a.view_start[b + 1];
  unsigned long long* K = a.keys + (size_t)b * a.kcap;
  int base = 0;
  for (int v = v0; v < v1; ++v) {
    const long slot0 = (long)(v - v0) * a.max_rows;
    if (slot0 >= a.kcap) break;                                   // (key_cap below views * max_rows: the views that fit)
    const int c = min(min(max(a.counts[v], 0), a.max_rows), (int)(a.kcap - slot0));   // base <= slot0: base + r stays below key_cap
    const float w = a.weight[v];
    for (int r = tid; r < c; r += FUSE_THREADS) {
      const float t = a.rows[((size_t)v * a.max_rows + r) * 6 + 4] * w;
      const unsigned int hi = t > 0.f ? sortable_desc(t) : FUSE_NO_CANDIDATE;
      K[base + r] = ((unsigned long long)hi << 32) | (unsigned int)(slot0 + r);
    }
    base += c;
  }
  if (tid == 0) a.nout[b] = base;
}

// A match as one word that orders like (larger IoU first, equal IoUs to the cluster created first): the bits of the IoU
// (positive: monotonic) above the inverted cluster index.  "No match" is 0: every match has iou > thr >= 0.
__device__ __forceinline__ unsigned long long fuse_match_key(float iou, int idx) {
  return ((unsigned long long)__float_as_uint(iou) << 32) | (0xFFFFFFFFu - (unsigned int)idx);
}

// max of v and the value the DPP pattern CTRL brings from another lane (rows outside ROW_MASK keep their own)
template <int CTRL, int ROW_MASK> __device__ __forceinline__ unsigned long long fuse_dpp_max(unsigned long long v) {
  const int lo = (int)(unsigned int)v, hi = (int)(unsigned int)(v >> 32);
  const unsigned int olo = (unsigned int)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false);
  const unsigned int ohi = (unsigned int)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
  const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
  return o > v ? o : v;
}

// the wave's largest key, uniform: a reduction by data-parallel primitives (no LDS round trips, unlike six shuffles on the
// path every candidate waits for) - within quads, half rows and rows of 16 lanes, then row 0 -> 1 and 2 -> 3, then rows
// 0..1 -> 2..3; lane 63 holds the result
__device__ __forceinline__ unsigned long long fuse_wave_max(unsigned long long v) {
  v = fuse_dpp_max<0xB1, 0xF>(v);            // quad_perm [1, 0, 3, 2]
  v = fuse_dpp_max<0x4E, 0xF>(v);            // quad_perm [2, 3, 0, 1]
  v = fuse_dpp_max<0x141, 0xF>(v);           // row_half_mirror
  v = fuse_dpp_max<0x140, 0xF>(v);           // row_mirror
  v = fuse_dpp_max<0x142, 0xA>(v);           // row_bcast:15 into rows 1 and 3
  v = fuse_dpp_max<0x143, 0xC>(v);           // row_bcast:31 into rows 2 and 3
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, 63);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), 63);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(FUSE_THREADS) void fuse_greedy_kernel(FuseArgs a) {
  extern __shared__ float4 fuse_lds[];
  const int cap = a.kcap;
  float4* F = fuse_lds;                                   // [cap] the clusters' fused boxes
  float4* acc = F + cap;                                  // [cap] sums of t * coordinate
  unsigned long long* sk = reinterpret_cast<unsigned long long*>(acc);   // [cap] ranking keys, once the pass is over
  float4* cb = acc + cap;                                 // [FUSE_THREADS] staged candidates: box
  float* kcls = reinterpret_cast<float*>(cb + FUSE_THREADS);   // [cap] the clusters' classes
  float* ct = kcls + cap;                                 // [FUSE_THREADS] t (0: no candidate, the pass ends)
  float* cc = ct + FUSE_THREADS;                          // [FUSE_THREADS] class
  unsigned long long* red = reinterpret_cast<unsigned long long*>(cc + FUSE_THREADS);   // [2][FUSE_WAVES] the waves' best matches
  float* Wsh = reinterpret_cast<float*>(red + 2 * FUSE_WAVES);

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v0 = a.view_start[b], v1 = a.view_start[b + 1];
  const unsigned long long* K = a.keys + (size_t)b * a.kcap;
  const int n = a.nout[b];                     // (written by fuse_candidates_kernel; every thread reads it before the end)
  const bool agn = a.agnostic != 0;
  const float thr = a.thr;
  if (tid == 0) {
    float W = 0.f;
    for (int v = v0; v < v1; ++v) W = W + a.weight[v];
    *Wsh = W;
  }
  float st_r[FUSE_SLICES];                     // sum of t and member count of clusters tid, tid + 256, ...
  int n_r[FUSE_SLICES];
#pragma unroll
  for (int s = 0; s < FUSE_SLICES; ++s) { st_r[s] = 0.f; n_r[s] = 0; }
  int nc = 0, step = 0;
  bool done = false;
  for (int base = 0; base < n && !done; base += FUSE_THREADS) {
    __syncthreads();                           // the batch before this one has been read
    {
      const int i = base + tid;
      float t = 0.f;
      if (i < n) {
        const unsigned long long key = K[i];
        const unsigned int hi = (unsigned int)(key >> 32);
        if (hi != FUSE_NO_CANDIDATE) {
          const unsigned int slot = (unsigned int)key;
          const int v = slot / a.max_rows, r = slot - v * a.max_rows;
          const float* row = a.rows + ((size_t)(v0 + v) * a.max_rows + r) * 6;
          cb[tid] = make_float4(row[0], row[1], row[2], row[3]);
          cc[tid] = row[5];
          t = __uint_as_float(0xFFFFFFFFu - hi);             // the t the key was made from, bit for bit
        }
      }
      ct[tid] = t;
    }
    __syncthreads();
    const int m = min(FUSE_THREADS, n - base);
    float nt = ct[0], ncls = cc[0];            // the next candidate, read ahead of the barrier it would otherwise wait behind
    float4 nB = cb[0];
    for (int j = 0; j < m; ++j) {
      const float t = nt;
      if (!(t > 0.f)) { done = true; break; }  // (block-uniform) sorted: no candidate follows
      const float4 B = nB;
      const float cls = ncls;
      if (j + 1 < m) { nt = ct[j + 1]; nB = cb[j + 1]; ncls = cc[j + 1]; }
      const float ab = (B.z - B.x) * (B.w - B.y);
      float best = thr;
      int bi = -1;
      for (int k = tid; k < nc; k += FUSE_THREADS) {
        if (!agn && kcls[k] != cls) continue;
        const float4 A = F[k];
        const float w = fmaxf(0.f, fminf(A.z, B.z) - fmaxf(A.x, B.x));
        const float h = fmaxf(0.f, fminf(A.w, B.w) - fmaxf(A.y, B.y));
        const float inter = w * h;
        if (!(inter > 0.f)) continue;          // an empty intersection never matches
        const float aa = (A.z - A.x) * (A.w - A.y);
        const float iou = inter / ((aa + ab) - inter);
        if (iou > best) { best = iou; bi = k; }              // (k ascends: an equal IoU stays with the earlier cluster)
      }
      unsigned long long key = fuse_wave_max(bi >= 0 ? fuse_match_key(best, bi) : 0ull);
      const int set = (step & 1) * FUSE_WAVES;
      if (lane == 0) red[set + wave] = key;
      __syncthreads();
#pragma unroll
      for (int w = 0; w < FUSE_WAVES; ++w) {
        const unsigned long long o = red[set + w];
        key = o > key ? o : key;
      }
      bi = key ? (int)(0xFFFFFFFFu - (unsigned int)key) : 0x7FFFFFFF;
      ++step;
      if (bi != 0x7FFFFFFF) {
        if ((bi & (FUSE_THREADS - 1)) == tid) {              // the owner: the only thread that scans cluster bi
          const int sl = bi / FUSE_THREADS;
          float st = 0.f;
#pragma unroll
          for (int s = 0; s < FUSE_SLICES; ++s)
            if (s == sl) { st_r[s] = st_r[s] + t; n_r[s] += 1; st = st_r[s]; }
          float4 s4 = acc[bi];
          s4.x = s4.x + t * B.x; s4.y = s4.y + t * B.y; s4.z = s4.z + t * B.z; s4.w = s4.w + t * B.w;
          acc[bi] = s4;
          F[bi] = make_float4(s4.x / st, s4.y / st, s4.z / st, s4.w / st);
        }
      } else {
        if ((nc & (FUSE_THREADS - 1)) == tid) {
          const int sl = nc / FUSE_THREADS;
#pragma unroll
          for (int s = 0; s < FUSE_SLICES; ++s)
            if (s == sl) { st_r[s] = t; n_r[s] = 1; }
          F[nc] = B;
          kcls[nc] = cls;
          acc[nc] = make_float4(t * B.x, t * B.y, t * B.z, t * B.w);
        }
        ++nc;                                  // (nc <= candidates taken <= key_cap: inside the LDS arrays)
      }
    }
  }
  __syncthreads();                             // the pass is over: acc is free, F and kcls are read by every thread
  // ---- ranking by the final score, equal scores by creation order
  const float W = *Wsh;
#pragma unroll
  for (int s = 0; s < FUSE_SLICES; ++s) {
    const int k = tid + s * FUSE_THREADS;
    if (k < nc) {
      const float cnt = (float)n_r[s];
      const float score = (st_r[s] / cnt) * (fminf(cnt, W) / W);
      sk[k] = ((unsigned long long)sortable_desc(score) << 32) | (unsigned int)k;
    }
  }
  const int npad = npad_of(nc);                // <= cap: nc <= cap, both cap and npad powers of two >= 64
  for (int k = nc + tid; k < npad; k += FUSE_THREADS) sk[k] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (npad >> 1); t += FUSE_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int p = i | j;
        const unsigned long long x = sk[i], y = sk[p];
        const bool up = (i & k) == 0;
        if ((x > y) == up) { sk[i] = y; sk[p] = x; }
      }
      __syncthreads();
    }
  }
  const int m = min(nc, a.max_det);
  float* O = a.out + (size_t)b * a.max_det * 6;
  for (int i = tid; i < m; i += FUSE_THREADS) {
    const unsigned long long key = sk[i];
    const int k = (int)(unsigned int)key;
    const float4 f = F[k];
    O[i * 6 + 0] = f.x; O[i * 6 + 1] = f.y; O[i * 6 + 2] = f.z; O[i * 6 + 3] = f.w;
    O[i * 6 + 4] = __uint_as_float(0xFFFFFFFFu - (unsigned int)(key >> 32));
    O[i * 6 + 5] = kcls[k];
  }
  if (tid == 0) a.nout[b] = m;
}

}  // namespace

extern "C" {

int kodhip_fuse_max_rows(void) { return KOD_FUSE_MAX_ROWS; }

// rows [V][max_rows][6] (x1, y1, x2, y2, score, class; kodhip_nms_ex's `out`, in image pixels), counts [V], the views of
// image i are view_start[i] .. view_start[i + 1], view_weight [V]; keys: n_images * key_cap u64 workspace;
// out [n_images][max_det][6], nout [n_images].
int kodhip_fuse_detections(const float* rows, const int* counts, const int* view_start, const float* view_weight, void* keys,
                           int key_cap, float* out, int* nout, int n_images, int max_rows, int max_det, float thr, int agnostic,
                           hipStream_t stream) {
  KOD_CHECK_ARG(rows && counts && view_start && view_weight && keys && out && nout, "fuse_detections: null pointer");
  KOD_CHECK_ARG(n_images >= 1 && n_images <= 65535 && max_rows >= 1, "fuse_detections: n_images must be in 1..65535, max_rows >= 1");
  KOD_CHECK_ARG(max_det >= 1 && max_det <= FUSE_MAX_DET, "fuse_detections: max_det must be in 1..300");
  KOD_CHECK_ARG(agnostic == 0 || agnostic == 1, "fuse_detections: agnostic must be 0 or 1");
  KOD_CHECK_ARG(thr >= 0.f && thr <= 1.f, "fuse_detections: thr must be in [0, 1]");
  KOD_CHECK_ARG(key_cap >= 64 && (key_cap & (key_cap - 1)) == 0 && key_cap <= KOD_FUSE_MAX_ROWS,
                "fuse_detections: key_cap must be a power of two in 64..%d", KOD_FUSE_MAX_ROWS);
  FuseArgs a = {};
  a.rows = rows; a.counts = counts; a.view_start = view_start; a.weight = view_weight; a.keys = (unsigned long long*)keys;
  a.out = out; a.nout = nout; a.kcap = key_cap; a.max_rows = max_rows; a.max_det = max_det; a.agnostic = agnostic; a.thr = thr;
  const size_t lds = fuse_lds_bytes(key_cap);
  if (lds > 64 * 1024) {                       // beyond the default limit of dynamic LDS: ask for it (no launch, no stream work)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fuse_greedy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      kodhip_set_error("fuse_detections: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
      return (int)e;
    }
  }
  hipLaunchKernelGGL(fuse_candidates_kernel, dim3(n_images), dim3(FUSE_THREADS), 0, stream, a);
  KOD_LAUNCH_CHECK("fuse_candidates");
  NmsArgs s = {};
  s.keys = a.keys; s.ncand = nout; s.kcap = key_cap;
  key_sort_launch(s, n_images, stream);
  KOD_LAUNCH_CHECK("fuse_sort");
  hipLaunchKernelGGL(fuse_greedy_kernel, dim3(n_images), dim3(FUSE_THREADS), lds, stream, a);
  KOD_LAUNCH_CHECK("fuse_greedy");
  return KOD_OK;
}

}  // extern "C"
