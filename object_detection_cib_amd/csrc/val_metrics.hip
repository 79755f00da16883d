// YOLOv5's validation metrics on the device: val.py's process_batch (per batch: kodhip_val_match) and utils/metrics.py's
// ap_per_class (once per epoch: kodhip_val_curves), accumulated over the whole validation set in a device-resident record
// store and read back once.
//
// MATCHING RULE - process_batch made deterministic.  Within one image, fp64 IoU = inter / (area_d + area_g - inter) as in
// map_match.hip (no epsilon, no +1; a pair whose union is zero or NaN, or whose IoU is NaN, is never a candidate):
//   1  a lane per detection d (index = NMS order, best score first): d PICKS the ground truth of its own class with the
//      largest IoU, equal IoUs -> the lower ground-truth index;
//   2  a lane per ground truth: it walks the detections that picked it in index order and hands each one run_d, the largest
//      IoU among the LOWER-index detections that picked the same ground truth (-1 if none);
//   3  a lane per detection: d is correct at threshold t iff run_d < t <= IoU_d, i.e. IoU_d reaches t and no earlier picker
//      of its ground truth does.  The result is a BITMASK over the thresholds, not a prefix count: an earlier picker with a
//      smaller IoU takes the low thresholds away and leaves the high ones (a hole at the bottom).
// A detection that loses its ground truth is not offered its second best.  This is neither confusion.hip's rule (class-
// agnostic, ONE IoU threshold, the picker with the HIGHEST IoU wins the ground truth) nor map_match.hip's (COCO: greedy in
// score order per threshold, a detection whose best ground truth is taken moves on to its next best, at most 256 ground
// truths).  Classes outside [0, nc) take no part.  No cap on ground truths per image.
//
// RECORD STORE.  Every detection with a class in [0, nc) appends one 8-byte record {score bits : 32, class : 16 | mask : 16}
// at offsets[b] + its rank among the image's participating detections: image order within the batch, detection order within
// the image.  offsets come from one small launch (participating detections per image, their exclusive prefix on top of the
// device-side running count, which it advances) - no per-image atomics, the order never depends on scheduling.  nt[label]
// is counted with 64-bit integer atomics (sums of integers: order-free).  Nothing is written at or beyond `capacity`.
//
// CURVES.  Order contract: class ascending, score descending, arrival index ascending.  One key sort (kodhip_keysort.h:
// sortable_desc(score) << 32 | arrival index, the NMS's network) over all records, then one block per class collects its
// records from the sorted sequence in order.  A block per (class, threshold) then does the cumulative counts, the precision
// envelope (running maximum from the right) and numpy's interp at the 101 recall points; threshold 0's block also
// interpolates precision and recall at the 1000 confidence points.  All of it fp64 in ap_per_class's operation order (the
// library is built with -fno-fast-math -ffp-contract=off); the two grids are the host's arrays, never recomputed here.
// Scores are expected non-negative (sortable_desc); every hand-off between blocks is a launch boundary.
#include "kodhip_keysort.h"

#define KOD_VM_MAX_DET 1024          // per-detection state in LDS: 8 (IoU) + 8 (run) + 4 (pick) + 4 (class) bytes each = 24 KiB
#define KOD_VM_MAX_T 16              // the mask's 16 bits
#define KOD_VM_MAX_NC 65536          // the class's 16 bits
#define KOD_VM_MAX_X 1024            // recall points per AP (LDS)
#define KOD_VM_THREADS 256
#define KOD_VM_MAX_RECORDS (1ll << 30)   // the sort's key capacity is an int and a power of two

namespace {

struct VmRecord { unsigned int score, cm; };      // cm = class | mask << 16

// rank of this thread among the block's threads with `flag` set (thread order); total = how many.  Two barriers.
__device__ __forceinline__ int block_rank(bool flag, int* s_w, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < KOD_VM_THREADS / 64; ++i) {
    const int v = s_w[i];
    if (i < w) pre += v;
    tot += v;
  }
  __syncthreads();
  total = tot;
  return pre + __popcll(m & ((1ull << lane) - 1ull));
}

// inclusive scan over the block in thread order (op associative, `identity` its neutral element); total = all 256.
template <typename V, typename Op>
__device__ __forceinline__ V block_scan(V v, V identity, Op op, V* s_w, V& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V u = __shfl_up(v, o, 64);
    if (lane >= o) v = op(u, v);
  }
  if (lane == 63) s_w[w] = v;
  __syncthreads();
  V pre = identity, tot = identity;
#pragma unroll
  for (int i = 0; i < KOD_VM_THREADS / 64; ++i) {
    const V x = s_w[i];
    if (i < w) pre = op(pre, x);
    tot = op(tot, x);
  }
  __syncthreads();
  total = tot;
  return op(pre, v);
}

__device__ __forceinline__ bool class_in_range(float fc, int nc) { return fc > -1.0f && fc < (float)nc; }   // NaN fails both

// ---- per batch -------------------------------------------------------------------------------------------------

struct VmMatchArgs {
  const float* det;       // [B][max_det][6]
  const int* ndet;        // [B]
  const double* gt;       // [n][4] xyxy
  const long* gt_label;   // [n]
  const int* gt_start;    // [B+1]
  VmRecord* rec;          // [capacity]
  int* count;             // [1] running record count
  int* offsets;           // [B] scratch: first record slot of each image
  unsigned long long* nt; // [nc]
  long long capacity;
  int B, max_det, nc, T;
  double thr[KOD_VM_MAX_T];
};

__device__ __forceinline__ int vm_ndet(const VmMatchArgs& a, int b) {
  return max(min(min(a.ndet[b], a.max_det), KOD_VM_MAX_DET), 0);
}

// one block: participating detections per image (a wave per image), then their exclusive prefix on top of the running count
__global__ __launch_bounds__(KOD_VM_THREADS) void val_offsets_kernel(VmMatchArgs a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = w; b < a.B; b += KOD_VM_THREADS / 64) {
    const int nd = vm_ndet(a, b);
    const float* D = a.det + (size_t)b * a.max_det * 6;
    int cnt = 0;
    for (int base = 0; base < nd; base += 64) {
      const int d = base + lane;
      const bool in = d < nd && class_in_range(D[(size_t)d * 6 + 5], a.nc);
      cnt += __popcll(__ballot(in));
    }
    if (lane == 0) a.offsets[b] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = *a.count;
    for (int b = 0; b < a.B; ++b) {
      const int c = a.offsets[b];
      a.offsets[b] = run;
      run += c;
    }
    *a.count = run;
  }
}

__global__ __launch_bounds__(KOD_VM_THREADS) void val_match_kernel(VmMatchArgs a) {
  __shared__ double s_iou[KOD_VM_MAX_DET];
  __shared__ double s_run[KOD_VM_MAX_DET];
  __shared__ int s_pick[KOD_VM_MAX_DET];       // in-image ground-truth index, -1: none
  __shared__ int s_cls[KOD_VM_MAX_DET];        // -1: takes no part
  __shared__ double s_thr[KOD_VM_MAX_T];
  __shared__ int s_w[KOD_VM_THREADS / 64];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int nc = a.nc;
  const int nd = vm_ndet(a, b);
  const int g0 = a.gt_start[b];
  const int ng = (a.gt && a.gt_label) ? max(a.gt_start[b + 1] - g0, 0) : 0;
  const float* D = a.det + (size_t)b * a.max_det * 6;
  const double* G = a.gt + (size_t)g0 * 4;
  const long* L = a.gt_label + g0;
  if (tid < KOD_VM_MAX_T) s_thr[tid] = tid < a.T ? a.thr[tid] : 0.0;

  // phase 1: every detection picks a ground truth of its class
  for (int d = tid; d < nd; d += KOD_VM_THREADS) {
    const float* r = D + (size_t)d * 6;
    const float fc = r[5];
    const bool in_range = class_in_range(fc, nc);
    const int cls = in_range ? (int)fc : -1;             // (int) truncates toward zero
    int pick = -1;
    double best = -1.0;
    if (in_range) {
      const double x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
      const double ad = (x2 - x1) * (y2 - y1);
      for (int g = 0; g < ng; ++g) {
        if (L[g] != (long)cls) continue;
        const double gx1 = G[(size_t)g * 4], gy1 = G[(size_t)g * 4 + 1], gx2 = G[(size_t)g * 4 + 2], gy2 = G[(size_t)g * 4 + 3];
        double w = fmin(x2, gx2) - fmax(x1, gx1);
        double h = fmin(y2, gy2) - fmax(y1, gy1);
        w = w > 0 ? w : 0; h = h > 0 ? h : 0;
        const double inter = w * h;
        const double uni = ad + (gx2 - gx1) * (gy2 - gy1) - inter;
        if (!(uni > 0.0 || uni < 0.0)) continue;            // zero or NaN union
        const double iou = inter / uni;
        if (!(iou == iou)) continue;
        if (pick < 0 || iou > best) { best = iou; pick = g; }   // strict: equal IoUs keep the lower index
      }
    }
    s_pick[d] = pick;
    s_iou[d] = best;
    s_run[d] = -1.0;
    s_cls[d] = cls;
  }
  __syncthreads();

  // phase 2: every ground truth walks its pickers in index order
  for (int g = tid; g < ng; g += KOD_VM_THREADS) {
    const long lab = L[g];
    if (lab < 0 || lab >= nc) continue;
    atomicAdd(&a.nt[lab], 1ull);
    double run = -1.0;
    for (int d = 0; d < nd; ++d) {
      if (s_pick[d] != g) continue;
      s_run[d] = run;                        // d picked this lane's ground truth only: no other lane writes it
      const double iou = s_iou[d];
      if (iou > run) run = iou;
    }
  }
  __syncthreads();

  // phase 3: masks, and the records in detection order
  const long long first = a.offsets[b];
  int done = 0;
  for (int base = 0; base < nd; base += KOD_VM_THREADS) {
    const int d = base + tid;
    const bool part = d < nd && s_cls[d] >= 0;
    int total;
    const int rank = block_rank(part, s_w, total);
    if (part) {
      unsigned int mask = 0;
      if (s_pick[d] >= 0) {
        const double iou = s_iou[d], run = s_run[d];
        for (int t = 0; t < a.T; ++t) {
          const double thr = s_thr[t];
          if (run < thr && thr <= iou) mask |= 1u << t;
        }
      }
      const long long slot = first + done + rank;
      if (slot >= 0 && slot < a.capacity) {
        VmRecord rec;
        rec.score = __float_as_uint(D[(size_t)d * 6 + 4]);
        rec.cm = (unsigned int)s_cls[d] | (mask << 16);
        a.rec[slot] = rec;
      }
    }
    done += total;
  }
}

// ---- append one store to another (merge, gather, tests) -------------------------------------------------------------

__global__ __launch_bounds__(KOD_VM_THREADS) void val_append_kernel(VmRecord* dst, const int* dst_count, long long dst_capacity,
                                                                   const VmRecord* src, const int* src_count, long long src_bound) {
  const long long n = min((long long)max(*src_count, 0), src_bound);
  const long long i = (long long)blockIdx.x * KOD_VM_THREADS + threadIdx.x;
  const long long slot = (long long)max(*dst_count, 0) + i;
  if (i < n && slot < dst_capacity) dst[slot] = src[i];
}

__global__ void val_append_count_kernel(int* dst_count, const int* src_count, long long src_bound) {
  if (threadIdx.x == 0 && blockIdx.x == 0)
    *dst_count = max(*dst_count, 0) + (int)min((long long)max(*src_count, 0), src_bound);
}

// ---- curves ----------------------------------------------------------------------------------------------------------

struct VmCurveArgs {
  const VmRecord* rec;        // [capacity] arrival order
  const int* count;           // [1]
  const long long* nt;        // [nc]
  const double* px;           // [npx] device copy of the host's confidence grid
  const double* xr;           // [nx] device copy of the host's recall grid
  long long capacity;
  int nc, T, npx, nx;
  // workspace
  int* n;                     // [1] min(count, capacity)
  unsigned long long* keys;   // [kcap]
  VmRecord* srec;             // [capacity] records in (score descending, arrival) order
  VmRecord* crec;             // [capacity] the same, class-major
  long long* start;           // [nc+1]
  int* tpc;                   // [T][capacity] cumulative true positives
  double* env;                // [T][capacity + 2 nc] precision envelopes (two sentinels per class)
  // outputs
  double* p;                  // [nc][npx]
  double* r;                  // [nc][npx]
  double* ap;                 // [nc][T]
  unsigned long long* n_p;    // [nc]
};

__global__ void val_begin_kernel(VmCurveArgs a) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *a.n = (int)min((long long)max(*a.count, 0), a.capacity);
}

__global__ __launch_bounds__(KOD_VM_THREADS) void val_keys_kernel(VmCurveArgs a) {
  const long long i = (long long)blockIdx.x * KOD_VM_THREADS + threadIdx.x;
  if (i >= *a.n) return;
  const VmRecord rec = a.rec[i];
  a.keys[i] = ((unsigned long long)sortable_desc(__uint_as_float(rec.score)) << 32) | (unsigned long long)(unsigned int)i;
  const int c = (int)(rec.cm & 0xFFFFu);
  if (c < a.nc) atomicAdd(&a.n_p[c], 1ull);
}

__global__ void val_starts_kernel(VmCurveArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long run = 0;
  for (int c = 0; c < a.nc; ++c) {
    a.start[c] = run;
    run += (long long)a.n_p[c];
  }
  a.start[a.nc] = run;
}

__global__ __launch_bounds__(KOD_VM_THREADS) void val_gather_kernel(VmCurveArgs a) {
  const long long i = (long long)blockIdx.x * KOD_VM_THREADS + threadIdx.x;
  const int n = *a.n;
  if (i >= n) return;
  const unsigned int idx = (unsigned int)(a.keys[i] & 0xFFFFFFFFull);
  if (idx < (unsigned int)n) a.srec[i] = a.rec[idx];
}

// a block per class: its records out of the sorted sequence, order kept
__global__ __launch_bounds__(KOD_VM_THREADS) void val_bucket_kernel(VmCurveArgs a) {
  __shared__ int s_w[KOD_VM_THREADS / 64];
  const int c = blockIdx.x, tid = threadIdx.x;
  const long long s = a.start[c];
  const long long nrec = a.start[c + 1] - s;
  if (nrec <= 0) return;
  const int n = *a.n;
  long long done = 0;
  for (int base = 0; base < n && done < nrec; base += KOD_VM_THREADS) {
    const int i = base + tid;
    VmRecord rec = {0u, 0u};
    bool mine = false;
    if (i < n) {
      rec = a.srec[i];
      mine = (int)(rec.cm & 0xFFFFu) == c;
    }
    int total;
    const int rank = block_rank(mine, s_w, total);
    const long long slot = s + done + rank;
    if (mine && slot < a.capacity) a.crec[slot] = rec;
    done += total;
  }
}

// numpy.interp's index: the last i in [0, m) with xp(i) <= x, -1 when x < xp(0); xp non-decreasing
template <typename XP> __device__ __forceinline__ long long interp_index(long long m, double x, XP xp) {
  long long lo = -1, hi = m;
  while (hi - lo > 1) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (xp(mid) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// numpy.interp at one point, right = fp(m - 1)
template <typename XP, typename FP> __device__ __forceinline__ double interp_at(long long m, double x, XP xp, FP fp, double left) {
  const long long j = interp_index(m, x, xp);
  if (j < 0) return left;
  if (j == m - 1) return fp(j);
  const double xj = xp(j), fj = fp(j);
  if (xj == x) return fj;
  const double slope = (fp(j + 1) - fj) / (xp(j + 1) - xj);
  return slope * (x - xj) + fj;
}

// a block per (class, threshold)
__global__ __launch_bounds__(KOD_VM_THREADS) void val_curves_kernel(VmCurveArgs a) {
  __shared__ double s_q[KOD_VM_MAX_X];
  __shared__ double s_wd[KOD_VM_THREADS / 64];
  __shared__ int s_wi[KOD_VM_THREADS / 64];
  const int c = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  const long long s = a.start[c];
  const long long n = a.start[c + 1] - s;
  const long long nl = a.nt[c];
  double* P = a.p + (size_t)c * a.npx;
  double* R = a.r + (size_t)c * a.npx;
  if (n <= 0 || nl <= 0) {                               // no records or no ground truth: zero rows
    if (tid == 0) a.ap[(size_t)c * a.T + j] = 0.0;
    if (j == 0)
      for (int i = tid; i < a.npx; i += KOD_VM_THREADS) { P[i] = 0.0; R[i] = 0.0; }
    return;
  }
  const VmRecord* rec = a.crec + s;
  int* tpc = a.tpc + (size_t)j * a.capacity + s;
  double* env = a.env + (size_t)j * (a.capacity + 2 * (long long)a.nc) + s + 2 * (long long)c;

  // cumulative true positives at this threshold (false positives: k + 1 - tpc[k])
  int carry = 0;
  for (long long base = 0; base < n; base += KOD_VM_THREADS) {
    const long long k = base + tid;
    const int v = k < n ? (int)((rec[k].cm >> (16 + j)) & 1u) : 0;
    int total;
    const int incl = block_scan(v, 0, [](int x, int y) { return x + y; }, s_wi, total);
    if (k < n) tpc[k] = carry + incl;
    carry += total;
  }
  __syncthreads();

  const double den = (double)nl + 1e-16;
  auto recall = [&](long long k) { return (double)tpc[k] / den; };
  auto precision = [&](long long k) {
    const double tp = (double)tpc[k], fp = (double)(k + 1 - (long long)tpc[k]);
    return tp / (tp + fp);
  };
  const long long m = n + 2;
  auto mrec = [&](long long i) { return i == 0 ? 0.0 : (i == m - 1 ? 1.0 : recall(i - 1)); };
  auto mpre = [&](long long i) { return i == 0 ? 1.0 : (i == m - 1 ? 0.0 : precision(i - 1)); };

  // precision envelope: running maximum from the right
  double top = 0.0;                                      // every mpre is >= 0, the rightmost is 0
  for (long long base = 0; base < m; base += KOD_VM_THREADS) {
    const long long i = m - 1 - (base + tid);
    const double v = i >= 0 ? mpre(i) : 0.0;
    double total;
    const double incl = block_scan(v, 0.0, [](double x, double y) { return x > y ? x : y; }, s_wd, total);
    if (i >= 0) env[i] = incl > top ? incl : top;
    top = total > top ? total : top;
  }
  __syncthreads();

  // AP: interp(xr, mrec, envelope), trapezoids
  auto envf = [&](long long i) { return env[i]; };
  for (int t = tid; t < a.nx; t += KOD_VM_THREADS) s_q[t] = interp_at(m, a.xr[t], mrec, envf, env[0]);
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int k = 0; k + 1 < a.nx; ++k) sum += (s_q[k] + s_q[k + 1]) / 2.0 * (a.xr[k + 1] - a.xr[k]);
    a.ap[(size_t)c * a.T + j] = sum;
  }

  // threshold 0: recall and precision over confidence, interp(-px, -conf, ., left = 0 / 1)
  if (j == 0) {
    auto nconf = [&](long long k) { return -(double)__uint_as_float(rec[k].score); };
    for (int i = tid; i < a.npx; i += KOD_VM_THREADS) {
      const double x = -a.px[i];
      R[i] = interp_at(n, x, nconf, recall, 0.0);
      P[i] = interp_at(n, x, nconf, precision, 1.0);
    }
  }
}

inline long long vm_key_cap(long long capacity) {
  long long k = 64;
  while (k < capacity) k <<= 1;
  return k;
}
inline long long vm_align(long long bytes) { return (bytes + 15) & ~15ll; }

// carve the workspace; -> bytes used
inline long long vm_carve(VmCurveArgs& a, char* base) {
  long long off = 0;
  auto take = [&](long long bytes) { char* p = base ? base + off : nullptr; off += vm_align(bytes); return p; };
  a.n = (int*)take(16);
  a.keys = (unsigned long long*)take(vm_key_cap(a.capacity) * 8);
  a.srec = (VmRecord*)take(a.capacity * 8);
  a.crec = (VmRecord*)take(a.capacity * 8);
  a.start = (long long*)take(((long long)a.nc + 1) * 8);
  a.tpc = (int*)take((long long)a.T * a.capacity * 4);
  a.env = (double*)take((long long)a.T * (a.capacity + 2 * (long long)a.nc) * 8);
  return off;
}

}  // namespace

extern "C" {

int kodhip_val_max_det(void) { return KOD_VM_MAX_DET; }
int kodhip_val_max_thresholds(void) { return KOD_VM_MAX_T; }
int kodhip_val_record_bytes(void) { return (int)sizeof(VmRecord); }

int kodhip_val_match(const float* det, const int* ndet, const double* gt_boxes, const long* gt_labels, const int* gt_start,
                     const double* iou_thresholds /* host */, int T, void* records, int* count, long long capacity,
                     long long* nt, int* offsets, int B, int max_det, int nc, hipStream_t stream) {
  KOD_CHECK_ARG(det && ndet && gt_start && iou_thresholds && records && count && nt && offsets && B > 0 && max_det > 0 && nc > 0,
                "val_match: bad args");
  KOD_CHECK_ARG(max_det <= KOD_VM_MAX_DET, "val_match: max_det %d beyond the %d detections per image the kernel holds", max_det,
                KOD_VM_MAX_DET);
  KOD_CHECK_ARG(T > 0 && T <= KOD_VM_MAX_T, "val_match: 1 to %d IoU thresholds", KOD_VM_MAX_T);
  KOD_CHECK_ARG(nc <= KOD_VM_MAX_NC, "val_match: at most %d classes", KOD_VM_MAX_NC);
  KOD_CHECK_ARG(capacity > 0 && capacity <= KOD_VM_MAX_RECORDS, "val_match: record capacity outside 1 .. 2^30");
  VmMatchArgs a = {};
  a.det = det; a.ndet = ndet; a.gt = gt_boxes; a.gt_label = gt_labels; a.gt_start = gt_start;
  a.rec = (VmRecord*)records; a.count = count; a.offsets = offsets; a.nt = (unsigned long long*)nt;
  a.capacity = capacity; a.B = B; a.max_det = max_det; a.nc = nc; a.T = T;
  for (int i = 0; i < T; ++i) a.thr[i] = iou_thresholds[i];
  hipLaunchKernelGGL(val_offsets_kernel, dim3(1), dim3(KOD_VM_THREADS), 0, stream, a);
  hipLaunchKernelGGL(val_match_kernel, dim3(B), dim3(KOD_VM_THREADS), 0, stream, a);
  KOD_LAUNCH_CHECK("val_match");
  return KOD_OK;
}

int kodhip_val_append(void* dst, int* dst_count, long long dst_capacity, const void* src, const int* src_count,
                      long long src_bound, hipStream_t stream) {
  KOD_CHECK_ARG(dst && dst_count && src && src_count && dst != src, "val_append: bad args");
  KOD_CHECK_ARG(dst_capacity > 0 && dst_capacity <= KOD_VM_MAX_RECORDS && src_bound > 0 && src_bound <= KOD_VM_MAX_RECORDS,
                "val_append: capacity / bound outside 1 .. 2^30");
  hipLaunchKernelGGL(val_append_kernel, dim3(cdiv(src_bound, KOD_VM_THREADS)), dim3(KOD_VM_THREADS), 0, stream, (VmRecord*)dst,
                     (const int*)dst_count, dst_capacity, (const VmRecord*)src, src_count, src_bound);
  hipLaunchKernelGGL(val_append_count_kernel, dim3(1), dim3(64), 0, stream, dst_count, src_count, src_bound);
  KOD_LAUNCH_CHECK("val_append");
  return KOD_OK;
}

long long kodhip_val_curves_workspace_bytes(long long capacity, int nc, int T) {
  if (capacity <= 0 || capacity > KOD_VM_MAX_RECORDS || nc <= 0 || nc > KOD_VM_MAX_NC || T <= 0 || T > KOD_VM_MAX_T) return -1;
  VmCurveArgs a = {};
  a.capacity = capacity; a.nc = nc; a.T = T;
  return vm_carve(a, nullptr);
}

int kodhip_val_curves(const void* records, const int* count, long long capacity, const long long* nt, const double* px, int npx,
                      const double* xr, int nx, int nc, int T, void* workspace, double* p, double* r, double* ap,
                      long long* n_p, hipStream_t stream) {
  KOD_CHECK_ARG(records && count && nt && px && xr && workspace && p && r && ap && n_p, "val_curves: bad args");
  KOD_CHECK_ARG(capacity > 0 && capacity <= KOD_VM_MAX_RECORDS, "val_curves: record capacity outside 1 .. 2^30");
  KOD_CHECK_ARG(nc > 0 && nc <= KOD_VM_MAX_NC && T > 0 && T <= KOD_VM_MAX_T, "val_curves: bad nc / T");
  KOD_CHECK_ARG(npx > 0 && nx > 1 && nx <= KOD_VM_MAX_X, "val_curves: bad grid sizes (at most %d recall points)", KOD_VM_MAX_X);
  KOD_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "val_curves: workspace not 16-byte aligned");
  VmCurveArgs a = {};
  a.rec = (const VmRecord*)records; a.count = count; a.nt = nt; a.px = px; a.xr = xr;
  a.capacity = capacity; a.nc = nc; a.T = T; a.npx = npx; a.nx = nx;
  a.p = p; a.r = r; a.ap = ap; a.n_p = (unsigned long long*)n_p;
  vm_carve(a, (char*)workspace);
  const int blocks = cdiv(capacity, KOD_VM_THREADS);
  hipError_t e = hipMemsetAsync(n_p, 0, (size_t)nc * 8, stream);
  if (e != hipSuccess) { kodhip_set_error("val_curves: %s", hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(val_begin_kernel, dim3(1), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(val_keys_kernel, dim3(blocks), dim3(KOD_VM_THREADS), 0, stream, a);
  NmsArgs s = {};
  s.keys = a.keys; s.kcap = (int)vm_key_cap(capacity); s.ncand = a.n;
  key_sort_launch(s, 1, stream);
  hipLaunchKernelGGL(val_starts_kernel, dim3(1), dim3(64), 0, stream, a);
  hipLaunchKernelGGL(val_gather_kernel, dim3(blocks), dim3(KOD_VM_THREADS), 0, stream, a);
  hipLaunchKernelGGL(val_bucket_kernel, dim3(nc), dim3(KOD_VM_THREADS), 0, stream, a);
  hipLaunchKernelGGL(val_curves_kernel, dim3(nc, T), dim3(KOD_VM_THREADS), 0, stream, a);
  KOD_LAUNCH_CHECK("val_curves");
  return KOD_OK;
}

}  // extern "C"
