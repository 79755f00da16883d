// Detection confusion matrix on the device: YOLOv5's ConfusionMatrix.process_batch (val.py / utils/metrics.py), made
// deterministic.  Class-AGNOSTIC matching, unlike the COCO matcher of map_match.hip: a detection may take a ground truth
// of another class, which is what fills the off-diagonal cells.
//
// One block per image, three phases over LDS-resident per-detection state:
//   1  a lane per detection: keep it when score > conf_thres (fp32, strict) and pick the ground truth with the largest
//      IoU > iou_thres (fp64, strict; equal IoUs -> lower ground-truth index; NaN never a candidate);
//   2  a lane per ground truth: among the detections that picked it take the one with the largest IoU (equal IoUs ->
//      lower detection index = higher score), count matrix[class][label], or matrix[nc][label] when nobody picked it.
//      A detection that loses here is NOT offered its second-best ground truth (YOLOv5's rule, not greedy matching);
//   3  a lane per detection: kept and not taken -> matrix[class][nc].
// Detections / ground truths with a class outside [0, nc) take no part.  No cap on ground truths per image.
//
// Counts: with nc <= KOD_CONFUSION_LDS_NC the image's (nc+1)^2 matrix is summed in LDS and only its non-zero cells are
// flushed with one 64-bit integer atomic each; beyond that the matrix no longer fits next to the per-detection state
// and every event is one global atomic.  Integer sums: the result does not depend on the order.
#include "kodhip_common.h"

#define KOD_CONFUSION_MAX_DET 1024     // per-detection state in LDS: 8 (IoU) + 4 (pick) + 4 (class) + 4 (taken) bytes each
#define KOD_CONFUSION_LDS_NC 80        // (80 + 1)^2 x 4 B = 26 244 B of LDS matrix; 20 KiB of detection state beside it
#define KOD_CONFUSION_THREADS 256

namespace {

struct ConfArgs {
  const float* det;       // [B][max_det][6]
  const int* ndet;        // [B]
  const double* gt;       // [n][4] xyxy
  const long* gt_label;   // [n]
  const int* gt_start;    // [B+1]
  unsigned long long* matrix;   // [(nc+1)^2] row = predicted, column = true
  int B, max_det, nc;
  float conf;
  double iou;
};

enum { PICK_NONE = -1, PICK_DROPPED = -2 };

template <bool LDS_MATRIX>
__global__ __launch_bounds__(KOD_CONFUSION_THREADS) void confusion_match_kernel(ConfArgs a) {
  __shared__ double s_iou[KOD_CONFUSION_MAX_DET];
  __shared__ int s_pick[KOD_CONFUSION_MAX_DET];      // in-image ground-truth index, or a PICK_* code
  __shared__ int s_cls[KOD_CONFUSION_MAX_DET];
  __shared__ int s_taken[KOD_CONFUSION_MAX_DET];
  __shared__ unsigned int s_mat[LDS_MATRIX ? (KOD_CONFUSION_LDS_NC + 1) * (KOD_CONFUSION_LDS_NC + 1) : 1];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int nc = a.nc, side = nc + 1;
  const int nd = max(min(min(a.ndet[b], a.max_det), KOD_CONFUSION_MAX_DET), 0);
  const int g0 = a.gt_start[b];
  const int ng = (a.gt && a.gt_label) ? max(a.gt_start[b + 1] - g0, 0) : 0;
  const float* D = a.det + (size_t)b * a.max_det * 6;
  const double* G = a.gt + (size_t)g0 * 4;
  const long* L = a.gt_label + g0;

  auto count = [&](int row, int col) {
    if (LDS_MATRIX) atomicAdd(&s_mat[row * side + col], 1u);
    else atomicAdd(&a.matrix[(size_t)row * side + col], 1ull);
  };

  if (LDS_MATRIX) {
    for (int i = tid; i < side * side; i += KOD_CONFUSION_THREADS) s_mat[i] = 0u;
  }

  // phase 1: every detection chooses a ground truth
  for (int d = tid; d < nd; d += KOD_CONFUSION_THREADS) {
    const float* r = D + (size_t)d * 6;
    const float fx1 = r[0], fy1 = r[1], fx2 = r[2], fy2 = r[3], score = r[4], fc = r[5];
    const bool in_range = fc > -1.0f && fc < (float)nc;          // (int) truncates toward zero; NaN fails both
    int pick = PICK_DROPPED;
    double best = a.iou;
    if (score > a.conf && in_range) {
      pick = PICK_NONE;
      const double x1 = fx1, y1 = fy1, x2 = fx2, y2 = fy2;
      const double ad = (x2 - x1) * (y2 - y1);
      for (int g = 0; g < ng; ++g) {
        const long lab = L[g];
        if (lab < 0 || lab >= nc) continue;
        const double gx1 = G[g * 4], gy1 = G[g * 4 + 1], gx2 = G[g * 4 + 2], gy2 = G[g * 4 + 3];
        double w = fmin(x2, gx2) - fmax(x1, gx1);
        double h = fmin(y2, gy2) - fmax(y1, gy1);
        w = w > 0 ? w : 0; h = h > 0 ? h : 0;
        const double inter = w * h;
        const double iou = inter / (ad + (gx2 - gx1) * (gy2 - gy1) - inter);
        if (iou > best) { best = iou; pick = g; }                 // strict: equal IoUs keep the lower index, NaN never wins
      }
    }
    s_pick[d] = pick;
    s_iou[d] = best;
    s_cls[d] = in_range ? (int)fc : 0;
    s_taken[d] = 0;
  }
  __syncthreads();

  // phase 2: every ground truth chooses among the detections that picked it
  for (int g = tid; g < ng; g += KOD_CONFUSION_THREADS) {
    const long lab = L[g];
    if (lab < 0 || lab >= nc) continue;
    int win = -1;
    double best = 0.0;
    for (int d = 0; d < nd; ++d) {
      if (s_pick[d] != g) continue;
      const double iou = s_iou[d];
      if (win < 0 || iou > best) { best = iou; win = d; }         // strict: equal IoUs keep the lower detection index
    }
    if (win >= 0) {
      count(s_cls[win], (int)lab);
      s_taken[win] = 1;                  // `win` picked this lane's ground truth only: no other lane writes it
    } else {
      count(nc, (int)lab);
    }
  }
  __syncthreads();

  // phase 3: kept detections nobody took are background false positives
  for (int d = tid; d < nd; d += KOD_CONFUSION_THREADS) {
    if (s_pick[d] != PICK_DROPPED && !s_taken[d]) count(s_cls[d], nc);
  }

  if (LDS_MATRIX) {
    __syncthreads();
    for (int i = tid; i < side * side; i += KOD_CONFUSION_THREADS) {
      const unsigned int v = s_mat[i];
      if (v) atomicAdd(&a.matrix[i], (unsigned long long)v);
    }
  }
}

}  // namespace

extern "C" {

int kodhip_confusion_max_det(void) { return KOD_CONFUSION_MAX_DET; }
int kodhip_confusion_lds_classes(void) { return KOD_CONFUSION_LDS_NC; }

int kodhip_confusion_match(const float* det, const int* ndet, const double* gt_boxes, const long* gt_labels,
                           const int* gt_start, long long* matrix, int B, int max_det, int nc, float conf_thres,
                           double iou_thres, hipStream_t stream) {
  KOD_CHECK_ARG(det && ndet && gt_start && matrix && B > 0 && max_det > 0 && nc > 0, "confusion_match: bad args");
  KOD_CHECK_ARG(max_det <= KOD_CONFUSION_MAX_DET, "confusion_match: max_det %d beyond the %d detections per image the kernel holds",
                max_det, KOD_CONFUSION_MAX_DET);
  KOD_CHECK_ARG(nc < 46340, "confusion_match: (nc + 1)^2 overflows an int");
  ConfArgs a = {};
  a.det = det; a.ndet = ndet; a.gt = gt_boxes; a.gt_label = gt_labels; a.gt_start = gt_start;
  a.matrix = (unsigned long long*)matrix;
  a.B = B; a.max_det = max_det; a.nc = nc; a.conf = conf_thres; a.iou = iou_thres;
  if (nc <= KOD_CONFUSION_LDS_NC)
    hipLaunchKernelGGL(confusion_match_kernel<true>, dim3(B), dim3(KOD_CONFUSION_THREADS), 0, stream, a);
  else
    hipLaunchKernelGGL(confusion_match_kernel<false>, dim3(B), dim3(KOD_CONFUSION_THREADS), 0, stream, a);
  KOD_LAUNCH_CHECK("confusion_match");
  return KOD_OK;
}

}  // extern "C"
