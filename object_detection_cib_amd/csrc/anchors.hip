// Auto-anchor on the device: YOLOv5's anchor metric, its genetic anchor evolution and the Lloyd step of the k-means that
// seeds it (utils/autoanchor.py: check_anchors / kmean_anchors), made deterministic.  Inputs are box sizes wh [N][2] fp32.
//
// Shape shared by the three families:
//   * grid = min(ceil(N / 256), 2048) blocks of 256 threads, grid-strided beyond that: a function of N alone, so the order
//     of every sum is too (the CU count of the device plays no part);
//   * a block's partial results go wave shuffle -> LDS -> ONE slot per block of a workspace slab; a small second launch
//     sums a row of slots (lane l takes slots l, l + 64, ... in order, then the same shuffle) - no floating-point atomics,
//     no inter-block waits: the launch boundary on the stream is the only ordering between the phases;
//   * candidate anchors / centroids are staged in LDS (hence the limits n <= 32, P <= 64, R <= 64).
// Floating-point sums are fp64, counts are exact integers.  Per-box arithmetic is fp32 with IEEE divisions (the library is
// built with -fno-fast-math -ffp-contract=off), so numpy float32 reproduces every per-box value bit for bit.  Box sizes
// and anchors are expected positive and finite.
#include "kodhip_common.h"

#define KOD_ANCHOR_THREADS 256
#define KOD_ANCHOR_WAVES (KOD_ANCHOR_THREADS / 64)
#define KOD_ANCHOR_GRID_CAP 2048
#define KOD_ANCHOR_MAX_N 32
#define KOD_ANCHOR_MAX_P 64
#define KOD_ANCHOR_MAX_R 64
#define KOD_ANCHOR_PAIRS_PER_THREAD (KOD_ANCHOR_MAX_R * KOD_ANCHOR_MAX_N / KOD_ANCHOR_THREADS)   // 8
#define KOD_ANCHOR_SELECT_THREADS 1024
#define KOD_ANCHOR_NO_LABEL 255

namespace {

struct AnchorTrace { int winner, accepted; double fitness; };      // kodhip_anchor_trace_bytes() = 16

inline int anchor_grid(long N) { return (int)(N >= (long)KOD_ANCHOR_GRID_CAP * KOD_ANCHOR_THREADS ? KOD_ANCHOR_GRID_CAP : cdiv(N, KOD_ANCHOR_THREADS)); }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

__device__ __forceinline__ unsigned int wave_sum_u32(unsigned int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// One wave sums a row of G block slots: lane l adds slots l, l + 64, ... in that order, then the butterfly.
__device__ __forceinline__ double wave_sum_slots_d(const double* row, int G, int lane) {
  double s = 0.0;
  for (int b = lane; b < G; b += 64) s += row[b];
  return wave_sum_d(s);
}
__device__ __forceinline__ unsigned long long wave_sum_slots_u64(const unsigned long long* row, int G, int lane) {
  unsigned long long s = 0;
  for (int b = lane; b < G; b += 64) s += row[b];
  return wave_sum_u64(s);
}

// Slab of the fitness pass: three arrays [P][G] (fp64 fitness, u64 recalled boxes, u64 box-anchor pairs above threshold).
struct FitSlab { double* f; unsigned long long* r; unsigned long long* c; };
__host__ __device__ inline FitSlab fit_slab(void* ws, int P, int G) {
  FitSlab s;
  s.f = (double*)ws;
  s.r = (unsigned long long*)(s.f + (size_t)P * G);
  s.c = s.r + (size_t)P * G;
  return s;
}

// Fitness of P anchor sets over all boxes.  MUTATE: set p is max(k * v[p], 2) of the current anchors k (one fp32 multiply,
// then a max); otherwise the sets are read as they are.
template <bool MUTATE>
__global__ __launch_bounds__(KOD_ANCHOR_THREADS) void anchor_fitness_kernel(const float2* __restrict__ wh, long N,
                                                                           const float* __restrict__ k,
                                                                           const float* __restrict__ v, int P, int n, float t,
                                                                           void* ws) {
  __shared__ float s_k[KOD_ANCHOR_MAX_P * KOD_ANCHOR_MAX_N * 2];
  __shared__ double s_f[KOD_ANCHOR_MAX_P][KOD_ANCHOR_WAVES];
  __shared__ unsigned int s_r[KOD_ANCHOR_MAX_P][KOD_ANCHOR_WAVES];
  __shared__ unsigned int s_c[KOD_ANCHOR_MAX_P][KOD_ANCHOR_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n2 = n * 2;
  for (int i = tid; i < P * n2; i += KOD_ANCHOR_THREADS) {
    if (MUTATE) {
      const float m = k[i % n2] * v[i];
      s_k[i] = m > 2.0f ? m : 2.0f;
    } else {
      s_k[i] = k[i];
    }
  }
  __syncthreads();

  const long stride = (long)gridDim.x * KOD_ANCHOR_THREADS;
  const long first = (long)blockIdx.x * KOD_ANCHOR_THREADS + tid;
  for (int p = 0; p < P; ++p) {
    const float* kp = s_k + p * n2;
    double fs = 0.0;
    unsigned int nr = 0, np = 0;
    for (long i = first; i < N; i += stride) {
      const float2 b = wh[i];
      float best = 0.0f;
      unsigned int above = 0;
      for (int j = 0; j < n; ++j) {
        const float rw = b.x / kp[2 * j], rh = b.y / kp[2 * j + 1];
        const float iw = 1.0f / rw, ih = 1.0f / rh;
        const float mw = rw < iw ? rw : iw, mh = rh < ih ? rh : ih;
        const float x = mw < mh ? mw : mh;
        above += x > t ? 1u : 0u;
        best = (j == 0 || x > best) ? x : best;
      }
      if (best > t) { fs += (double)best; nr += 1u; }
      np += above;
    }
    fs = wave_sum_d(fs);
    nr = wave_sum_u32(nr);
    np = wave_sum_u32(np);
    if (lane == 0) { s_f[p][wave] = fs; s_r[p][wave] = nr; s_c[p][wave] = np; }
  }
  __syncthreads();
  if (tid < P) {
    double fs = 0.0;
    unsigned long long nr = 0, np = 0;
#pragma unroll
    for (int w = 0; w < KOD_ANCHOR_WAVES; ++w) { fs += s_f[tid][w]; nr += s_r[tid][w]; np += s_c[tid][w]; }
    const int G = gridDim.x;
    const FitSlab s = fit_slab(ws, P, G);
    const size_t o = (size_t)tid * G + blockIdx.x;
    s.f[o] = fs; s.r[o] = nr; s.c[o] = np;
  }
}

// One wave per anchor set: the sums over the G block slots.
__global__ __launch_bounds__(KOD_ANCHOR_THREADS) void anchor_metric_finish_kernel(const void* ws, int P, int G, double* fitness_sum,
                                                                                 long long* n_recalled, long long* n_pairs) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * KOD_ANCHOR_WAVES + (threadIdx.x >> 6);
  if (p >= P) return;
  const FitSlab s = fit_slab(const_cast<void*>(ws), P, G);
  const double f = wave_sum_slots_d(s.f + (size_t)p * G, G, lane);
  const unsigned long long r = wave_sum_slots_u64(s.r + (size_t)p * G, G, lane);
  const unsigned long long c = wave_sum_slots_u64(s.c + (size_t)p * G, G, lane);
  if (lane == 0) { fitness_sum[p] = f; n_recalled[p] = (long long)r; n_pairs[p] = (long long)c; }
}

// One block: the P fitness sums (the order of anchor_metric_finish_kernel), the winner (largest sum, equal sums -> lower
// index), acceptance (strictly better than the current fitness) and the trace entry of this generation.
__global__ __launch_bounds__(KOD_ANCHOR_SELECT_THREADS) void anchor_select_kernel(const void* ws, int P, int G, int n, float* k,
                                                                                  const float* __restrict__ v, double* fitness,
                                                                                  AnchorTrace* trace) {
  __shared__ double s_fit[KOD_ANCHOR_MAX_P];
  __shared__ int s_win, s_acc;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FitSlab s = fit_slab(const_cast<void*>(ws), P, G);
  for (int p = wave; p < P; p += KOD_ANCHOR_SELECT_THREADS / 64) {
    const double f = wave_sum_slots_d(s.f + (size_t)p * G, G, lane);
    if (lane == 0) s_fit[p] = f;
  }
  __syncthreads();
  if (tid == 0) {
    int win = 0;
    double best = s_fit[0];
    for (int p = 1; p < P; ++p) {
      if (s_fit[p] > best) { best = s_fit[p]; win = p; }
    }
    const int acc = best > *fitness ? 1 : 0;
    if (acc) *fitness = best;
    trace->winner = win; trace->accepted = acc; trace->fitness = best;
    s_win = win; s_acc = acc;
  }
  __syncthreads();
  if (s_acc && tid < 2 * n) {
    const float m = k[tid] * v[(size_t)s_win * 2 * n + tid];
    k[tid] = m > 2.0f ? m : 2.0f;
  }
}

// ---- k-means ----------------------------------------------------------------------------------------------------------
// Slab of the Lloyd step: rows q = r * (n + 1) + j of G block slots; j < n: fp64 sums of the members' x and y and their
// count, j == n: the restart's distortion (in sx).
struct KmSlab { double* sx; double* sy; unsigned long long* cnt; };
__host__ __device__ inline KmSlab km_slab(void* ws, int R, int n, int G) {
  const size_t rows = (size_t)R * (n + 1);
  KmSlab s;
  s.sx = (double*)ws;
  s.sy = s.sx + rows * G;
  s.cnt = (unsigned long long*)(s.sy + rows * G);
  return s;
}

// Assignment + per-block member sums.  A tile is 256 points: every thread labels its point for each restart (LDS), then
// thread q = r * n + j walks the tile's points IN ORDER and adds the members of centroid j of restart r (registers).
__global__ __launch_bounds__(KOD_ANCHOR_THREADS) void anchor_kmeans_assign_kernel(const float2* __restrict__ pts, long N,
                                                                                 const float* __restrict__ cent, int R, int n,
                                                                                 int* __restrict__ labels, void* ws) {
  __shared__ float s_c[KOD_ANCHOR_MAX_R * KOD_ANCHOR_MAX_N * 2];
  __shared__ unsigned char s_label[KOD_ANCHOR_MAX_R][KOD_ANCHOR_THREADS];
  __shared__ float2 s_pt[KOD_ANCHOR_THREADS];
  __shared__ double s_dist[KOD_ANCHOR_MAX_R][KOD_ANCHOR_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int RN = R * n;
  for (int i = tid; i < RN * 2; i += KOD_ANCHOR_THREADS) s_c[i] = cent[i];
  for (int i = tid; i < R * KOD_ANCHOR_WAVES; i += KOD_ANCHOR_THREADS) s_dist[i / KOD_ANCHOR_WAVES][i % KOD_ANCHOR_WAVES] = 0.0;

  double ax[KOD_ANCHOR_PAIRS_PER_THREAD], ay[KOD_ANCHOR_PAIRS_PER_THREAD];
  unsigned int ac[KOD_ANCHOR_PAIRS_PER_THREAD];
#pragma unroll
  for (int u = 0; u < KOD_ANCHOR_PAIRS_PER_THREAD; ++u) { ax[u] = 0.0; ay[u] = 0.0; ac[u] = 0u; }
  __syncthreads();

  const long stride = (long)gridDim.x * KOD_ANCHOR_THREADS;
  for (long base = (long)blockIdx.x * KOD_ANCHOR_THREADS; base < N; base += stride) {      // block-uniform trip count
    const long i = base + tid;
    const bool live = i < N;
    const float2 pt = live ? pts[i] : make_float2(0.f, 0.f);
    s_pt[tid] = pt;
    for (int r = 0; r < R; ++r) {
      const float* c = s_c + r * n * 2;
      float bd = 0.f;
      int bj = 0;
      for (int j = 0; j < n; ++j) {
        const float dx = pt.x - c[2 * j], dy = pt.y - c[2 * j + 1];
        const float d = dx * dx + dy * dy;
        if (j == 0 || d < bd) { bd = d; bj = j; }            // strict: equal distances keep the lower index
      }
      s_label[r][tid] = live ? (unsigned char)bj : (unsigned char)KOD_ANCHOR_NO_LABEL;
      if (labels && live) labels[(size_t)r * N + i] = bj;
      const double ds = wave_sum_d(live ? (double)bd : 0.0);
      if (lane == 0) s_dist[r][wave] += ds;                  // one owner per cell, tile after tile
    }
    __syncthreads();
    const int cnt = (int)((N - base) < KOD_ANCHOR_THREADS ? (N - base) : KOD_ANCHOR_THREADS);
#pragma unroll
    for (int u = 0; u < KOD_ANCHOR_PAIRS_PER_THREAD; ++u) {
      const int q = tid + u * KOD_ANCHOR_THREADS;
      if (q < RN) {
        const int r = q / n, j = q - r * n;
        for (int m = 0; m < cnt; ++m) {
          if (s_label[r][m] == j) { ax[u] += (double)s_pt[m].x; ay[u] += (double)s_pt[m].y; ac[u] += 1u; }
        }
      }
    }
    __syncthreads();
  }

  const int G = gridDim.x;
  const KmSlab s = km_slab(ws, R, n, G);
#pragma unroll
  for (int u = 0; u < KOD_ANCHOR_PAIRS_PER_THREAD; ++u) {
    const int q = tid + u * KOD_ANCHOR_THREADS;
    if (q < RN) {
      const int r = q / n, j = q - r * n;
      const size_t o = ((size_t)r * (n + 1) + j) * G + blockIdx.x;
      s.sx[o] = ax[u]; s.sy[o] = ay[u]; s.cnt[o] = ac[u];
    }
  }
  if (tid < R) {
    double d = 0.0;
#pragma unroll
    for (int w = 0; w < KOD_ANCHOR_WAVES; ++w) d += s_dist[tid][w];
    s.sx[((size_t)tid * (n + 1) + n) * G + blockIdx.x] = d;
  }
}

// One wave per slab row: new centroid = float32(sum / count) (an empty cluster keeps its centroid), counts, distortion.
__global__ __launch_bounds__(KOD_ANCHOR_THREADS) void anchor_kmeans_update_kernel(const void* ws, int R, int n, int G, float* cent,
                                                                                 double* distortion, long long* counts) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * KOD_ANCHOR_WAVES + (threadIdx.x >> 6);
  if (q >= R * (n + 1)) return;
  const int r = q / (n + 1), j = q - r * (n + 1);
  const KmSlab s = km_slab(const_cast<void*>(ws), R, n, G);
  const double sx = wave_sum_slots_d(s.sx + (size_t)q * G, G, lane);
  if (j == n) {
    if (lane == 0) distortion[r] = sx;
    return;
  }
  const double sy = wave_sum_slots_d(s.sy + (size_t)q * G, G, lane);
  const unsigned long long c = wave_sum_slots_u64(s.cnt + (size_t)q * G, G, lane);
  if (lane == 0) {
    counts[r * n + j] = (long long)c;
    if (c) {
      cent[(r * n + j) * 2] = (float)(sx / (double)c);
      cent[(r * n + j) * 2 + 1] = (float)(sy / (double)c);
    }
  }
}

inline bool finite_f(float x) { return x == x && x - x == 0.0f; }
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace

extern "C" {

int kodhip_anchor_max_anchors(void) { return KOD_ANCHOR_MAX_N; }
int kodhip_anchor_max_population(void) { return KOD_ANCHOR_MAX_P; }
int kodhip_anchor_max_restarts(void) { return KOD_ANCHOR_MAX_R; }
int kodhip_anchor_trace_bytes(void) { return (int)sizeof(AnchorTrace); }
int kodhip_anchor_block_size(void) { return KOD_ANCHOR_THREADS; }
int kodhip_anchor_grid_cap(void) { return KOD_ANCHOR_GRID_CAP; }

// the larger of the two slabs: rows x blocks x (fp64, fp64, u64); the fitness pass uses P rows, a Lloyd step R * (n + 1)
long kodhip_anchor_workspace_bytes(long N, int sets) {
  if (N < 1 || sets < 1) return 0;
  return (long)align256((size_t)sets * (KOD_ANCHOR_MAX_N + 1) * anchor_grid(N) * 24);
}

int kodhip_anchor_metric(const float* wh, long N, const float* anchors, int P, int n, float t, void* workspace,
                         double* fitness_sum, long long* n_recalled, long long* n_pairs, hipStream_t stream) {
  KOD_CHECK_ARG(wh && anchors && workspace && fitness_sum && n_recalled && n_pairs, "anchor_metric: null pointer");
  KOD_CHECK_ARG(aligned8(wh) && aligned8(workspace), "anchor_metric: wh and workspace must be 8-byte aligned");
  KOD_CHECK_ARG(N >= 1 && N <= 0x7fffffffL, "anchor_metric: N %ld outside 1..2^31-1", N);
  KOD_CHECK_ARG(n >= 1 && n <= KOD_ANCHOR_MAX_N, "anchor_metric: n %d outside 1..%d anchors", n, KOD_ANCHOR_MAX_N);
  KOD_CHECK_ARG(P >= 1 && P <= KOD_ANCHOR_MAX_P, "anchor_metric: P %d outside 1..%d anchor sets", P, KOD_ANCHOR_MAX_P);
  KOD_CHECK_ARG(finite_f(t), "anchor_metric: threshold is not finite");
  const int G = anchor_grid(N);
  hipLaunchKernelGGL(anchor_fitness_kernel<false>, dim3(G), dim3(KOD_ANCHOR_THREADS), 0, stream, (const float2*)wh, N, anchors,
                     (const float*)nullptr, P, n, t, workspace);
  KOD_LAUNCH_CHECK("anchor_metric");
  hipLaunchKernelGGL(anchor_metric_finish_kernel, dim3(cdiv(P, KOD_ANCHOR_WAVES)), dim3(KOD_ANCHOR_THREADS), 0, stream,
                     (const void*)workspace, P, G, fitness_sum, n_recalled, n_pairs);
  KOD_LAUNCH_CHECK("anchor_metric");
  return KOD_OK;
}

int kodhip_anchor_evolve(const float* wh, long N, float* anchors, double* fitness, const float* mutations, int gen, int P, int n,
                         float t, void* trace, void* workspace, hipStream_t stream) {
  KOD_CHECK_ARG(wh && anchors && fitness && workspace, "anchor_evolve: null pointer");
  KOD_CHECK_ARG(gen >= 0, "anchor_evolve: gen %d is negative", gen);
  KOD_CHECK_ARG(gen == 0 || (mutations && trace), "anchor_evolve: null pointer (mutations, trace)");
  KOD_CHECK_ARG(aligned8(wh) && aligned8(workspace) && aligned8(trace) && aligned8(fitness),
                "anchor_evolve: wh, fitness, trace and workspace must be 8-byte aligned");
  KOD_CHECK_ARG(N >= 1 && N <= 0x7fffffffL, "anchor_evolve: N %ld outside 1..2^31-1", N);
  KOD_CHECK_ARG(n >= 1 && n <= KOD_ANCHOR_MAX_N, "anchor_evolve: n %d outside 1..%d anchors", n, KOD_ANCHOR_MAX_N);
  KOD_CHECK_ARG(P >= 1 && P <= KOD_ANCHOR_MAX_P, "anchor_evolve: P %d outside 1..%d candidates", P, KOD_ANCHOR_MAX_P);
  KOD_CHECK_ARG(finite_f(t), "anchor_evolve: threshold is not finite");
  if (gen == 0) return KOD_OK;
  const int G = anchor_grid(N);
  const size_t per_gen = (size_t)P * n * 2;
  for (int g = 0; g < gen; ++g) {
    const float* v = mutations + (size_t)g * per_gen;
    hipLaunchKernelGGL(anchor_fitness_kernel<true>, dim3(G), dim3(KOD_ANCHOR_THREADS), 0, stream, (const float2*)wh, N,
                       (const float*)anchors, v, P, n, t, workspace);
    hipLaunchKernelGGL(anchor_select_kernel, dim3(1), dim3(KOD_ANCHOR_SELECT_THREADS), 0, stream, (const void*)workspace, P, G, n,
                       anchors, v, fitness, (AnchorTrace*)trace + g);
  }
  KOD_LAUNCH_CHECK("anchor_evolve");
  return KOD_OK;
}

int kodhip_anchor_kmeans_step(const float* points, long N, float* centroids, int R, int n, void* workspace, double* distortion,
                              long long* counts, int* labels, hipStream_t stream) {
  KOD_CHECK_ARG(points && centroids && workspace && distortion && counts, "anchor_kmeans_step: null pointer");
  KOD_CHECK_ARG(aligned8(points) && aligned8(workspace), "anchor_kmeans_step: points and workspace must be 8-byte aligned");
  KOD_CHECK_ARG(N >= 1 && N <= 0x7fffffffL, "anchor_kmeans_step: N %ld outside 1..2^31-1", N);
  KOD_CHECK_ARG(n >= 1 && n <= KOD_ANCHOR_MAX_N, "anchor_kmeans_step: n %d outside 1..%d centroids", n, KOD_ANCHOR_MAX_N);
  KOD_CHECK_ARG(R >= 1 && R <= KOD_ANCHOR_MAX_R, "anchor_kmeans_step: R %d outside 1..%d restarts", R, KOD_ANCHOR_MAX_R);
  const int G = anchor_grid(N);
  hipLaunchKernelGGL(anchor_kmeans_assign_kernel, dim3(G), dim3(KOD_ANCHOR_THREADS), 0, stream, (const float2*)points, N,
                     (const float*)centroids, R, n, labels, workspace);
  KOD_LAUNCH_CHECK("anchor_kmeans_step");
  hipLaunchKernelGGL(anchor_kmeans_update_kernel, dim3(cdiv((long)R * (n + 1), KOD_ANCHOR_WAVES)), dim3(KOD_ANCHOR_THREADS), 0, stream,
                     (const void*)workspace, R, n, G, centroids, distortion, counts);
  KOD_LAUNCH_CHECK("anchor_kmeans_step");
  return KOD_OK;
}

}  // extern "C"
