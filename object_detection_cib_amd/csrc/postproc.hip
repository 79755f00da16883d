// Evaluation post-process on the device: prediction decode + YOLOv5-style batched NMS.
//
//   decode : kod/lightning/experiments/yv5_baseline/layers.py:55-63,74-76,87-89,143-153 (get_detections,
//            exp.py:70-102): xy = (sigmoid*2 + grid - .5)*stride, wh = (sigmoid*2)^2*anchor_px, cxcywh->xyxy,
//            sigmoid(obj), sigmoid(cls), rows ordered (level, anchor, y, x)
//   nms    : kod/core/nms.py:9-75 + torchvision.ops.nms: obj > conf, cls *= obj, multi-label candidates in
//            nonzero (row, class) order, top-30000 by score, boxes offset by class*4096 (in fp32, as the
//            reference does - the offset rounding is part of the result), greedy IoU > thr, first 300.
//
// Candidate compaction by ballot prefix sums (one block per image), a chip-wide bitonic sort of (score desc,
// candidate index asc) 64-bit keys, then a wave-batched greedy pass that keeps the <=300 survivors in LDS.  Everything is integer / comparison logic on fp32 values => results are bit-identical to the reference.
//
//   nms_ex : the deployment form (YOLOv5 detect.py): best-class candidates (multi_label=False: one candidate per row, the
//            argmax of cls * obj, lowest class index among equal maxima), a class filter applied to the candidate's class,
//            and the kept rows mapped from the letterboxed frame back to the source image (subtract the pad, multiply by
//            the inverse scale, clip - each operation rounded on its own).  Same keys, same sort, same greedy pass: the
//            best-class form needs `rows` keys per image where the multi-label one needs `rows * nc`.
//   decode_view : kodhip_decode for one view of test-time augmentation (YOLOv5 models/yolo.py::_forward_augment): the same
//            per-row arithmetic (one __device__ function, decode_row), then cx, cy, w, h divided by the view's scale, cx
//            mirrored about the full width for a flipped view, written to the view's own rows of the merged tensor.
#include "kodhip_common.h"
#include "kodhip_keysort.h"

struct KodLetterbox { float left, top, scale_x, scale_y, width, height; };      // include/kodhip.h
static_assert(sizeof(KodLetterbox) == 24, "KodLetterbox is six floats");

namespace {

struct DecodeLevel { const float* raw; int h, w, stride, row0; float aw[3], ah[3]; };
struct DecodeArgs { DecodeLevel lv[3]; float* det; int B, A, nc, rows; };

// What kodhip_decode_view adds to a row (test-time augmentation: the row belongs to one view of a merged tensor): the box
// back in the full-size frame - cx, cy, w, h each divided by `scale` (IEEE fp32 division, YOLOv5's `p[..., :4] /= scale`),
// then cx = full_w - cx for a left-right flipped view.
struct DecodeView { float scale, full_w; int flip, row_offset, rows_total; };

// One decoded row, shared by kodhip_decode and kodhip_decode_view: `row` counts the rows of the levels in `a` (level,
// anchor, y, x), `o` is where its 5 + nc values go.  VIEW = false never looks at `v`.
template <bool VIEW>
__device__ __forceinline__ void decode_row(const DecodeArgs& a, int b, int row, float* o, const DecodeView& v) {
  const int P = 5 + a.nc;
  int l = row >= a.lv[2].row0 ? 2 : (row >= a.lv[1].row0 ? 1 : 0);
  const DecodeLevel& L = a.lv[l];
  int r = row - L.row0;
  int hw = L.h * L.w;
  int an = r / hw, cell = r - an * hw;
  int gy = cell / L.w, gx = cell - gy * L.w;
  const float* p = L.raw + ((size_t)(b * a.A + an) * hw + cell) * P;
  float sx = 1.f / (1.f + expf(-p[0])), sy = 1.f / (1.f + expf(-p[1]));
  float sw = 1.f / (1.f + expf(-p[2])), sh = 1.f / (1.f + expf(-p[3]));
  float cx = (sx * 2.f + (float)gx - 0.5f) * (float)L.stride;
  float cy = (sy * 2.f + (float)gy - 0.5f) * (float)L.stride;
  float w = (sw * 2.f) * (sw * 2.f) * L.aw[an], h = (sh * 2.f) * (sh * 2.f) * L.ah[an];
  if (VIEW) {
    cx = __fdiv_rn(cx, v.scale); cy = __fdiv_rn(cy, v.scale); w = __fdiv_rn(w, v.scale); h = __fdiv_rn(h, v.scale);
    if (v.flip) cx = v.full_w - cx;
  }
  o[0] = cx - 0.5f * w; o[1] = cy - 0.5f * h; o[2] = cx + 0.5f * w; o[3] = cy + 0.5f * h;
  for (int k = 4; k < P; ++k) o[k] = 1.f / (1.f + expf(-p[k]));
}

__global__ void decode_kernel(DecodeArgs a) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (b, row)
  if (i >= (long)a.B * a.rows) return;
  int b = (int)(i / a.rows), row = (int)(i - (long)b * a.rows);
  decode_row<false>(a, b, row, a.det + (size_t)i * (5 + a.nc), DecodeView{});
}

// the rows of one view: a.lv holds the view's levels, a masked-out level with no rows (its row0 is the next level's, so
// no row selects it); a.rows = the view's own rows, written at [row_offset, row_offset + a.rows) of each image's
// rows_total rows.  Nothing else is written.
__global__ void decode_view_kernel(DecodeArgs a, DecodeView v) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // one thread per (b, own row)
  if (i >= (long)a.B * a.rows) return;
  int b = (int)(i / a.rows), row = (int)(i - (long)b * a.rows);
  decode_row<true>(a, b, row, a.det + ((size_t)b * v.rows_total + v.row_offset + row) * (5 + a.nc), v);
}

// ------------------------------------------------------------------------------------------------ NMS
// NmsArgs, sortable_desc and the key sort: kodhip_keysort.h (shared with tiles.hip)

__global__ __launch_bounds__(1024) void nms_candidates_kernel(NmsArgs a) {
  __shared__ int wtot[16];
  __shared__ int base_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = 5 + a.nc;
  const float* D = a.det + (size_t)b * a.rows * P;
  unsigned long long* K = a.keys + (size_t)b * a.kcap;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int r0 = 0; r0 < a.rows; r0 += 1024) {
    int row = r0 + tid;
    int cnt = 0;
    float obj = 0.f;
    if (row < a.rows) {
      obj = D[(size_t)row * P + 4];
      if (obj > a.conf) {
        if (a.nc > 1) {
          for (int c = 0; c < a.nc; ++c) cnt += (D[(size_t)row * P + 5 + c] * obj > a.conf) ? 1 : 0;
        } else {
          cnt = (D[(size_t)row * P + 5] * obj > a.conf) ? 1 : 0;      // best-class path, one class
        }
      }
    }
    // exclusive scan of cnt over the block (wave scan + wave totals)
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wtot[w];
    int total = 0;
    for (int w = 0; w < 16; ++w) total += wtot[w];
    int pos = base_s + before + incl - cnt;
    if (cnt) {
      for (int c = 0; c < a.nc; ++c) {
        float s = D[(size_t)row * P + 5 + c] * obj;
        if (s > a.conf) {
          if (pos < a.kcap)
            K[pos] = ((unsigned long long)sortable_desc(s) << 32) | (unsigned int)(row * a.nc + c);
          ++pos;
        }
      }
    }
    __syncthreads();
    if (tid == 0) base_s += total;
    __syncthreads();
  }
  if (tid == 0) a.ncand[b] = base_s < a.kcap ? base_s : a.kcap;
}

// kodhip_nms_ex's compaction: the ballot / prefix-scan shape of nms_candidates_kernel with an optional class filter
// (`keep` [nc], null = every class) and, with BEST, an argmax over the classes in place of the class loop - at most one
// candidate per row, so `rows` keys hold every candidate.  The filter looks at the candidate's class AFTER the argmax
// (YOLOv5 general.py: `x = x[(x[:, 5:6] == classes).any(1)]` follows `conf, j = x[:, 5:].max(1)`).
template <bool BEST>
__global__ __launch_bounds__(1024) void nms_candidates_ex_kernel(NmsArgs a, const unsigned char* __restrict__ keep) {
  __shared__ int wtot[16];
  __shared__ int base_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = 5 + a.nc;
  const float* D = a.det + (size_t)b * a.rows * P;
  unsigned long long* K = a.keys + (size_t)b * a.kcap;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int r0 = 0; r0 < a.rows; r0 += 1024) {
    const int row = r0 + tid;
    int cnt = 0, bc = 0;
    float obj = 0.f, best = 0.f;
    if (row < a.rows) {
      const float* r = D + (size_t)row * P;
      obj = r[4];
      if (obj > a.conf) {
        if (BEST) {
          best = r[5] * obj;
          for (int c = 1; c < a.nc; ++c) {
            const float s = r[5 + c] * obj;
            if (s > best) { best = s; bc = c; }          // equal maxima: the lowest class index stays
          }
          cnt = (best > a.conf && (!keep || keep[bc])) ? 1 : 0;
        } else {
          for (int c = 0; c < a.nc; ++c) cnt += (r[5 + c] * obj > a.conf && (!keep || keep[c])) ? 1 : 0;
        }
      }
    }
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wtot[w];
    int total = 0;
    for (int w = 0; w < 16; ++w) total += wtot[w];
    int pos = base_s + before + incl - cnt;
    if (cnt) {
      if (BEST) {
        if (pos < a.kcap) K[pos] = ((unsigned long long)sortable_desc(best) << 32) | (unsigned int)(row * a.nc + bc);
      } else {
        const float* r = D + (size_t)row * P;
        for (int c = 0; c < a.nc; ++c) {
          const float s = r[5 + c] * obj;
          if (s > a.conf && (!keep || keep[c])) {
            if (pos < a.kcap) K[pos] = ((unsigned long long)sortable_desc(s) << 32) | (unsigned int)(row * a.nc + c);
            ++pos;
          }
        }
      }
    }
    __syncthreads();
    if (tid == 0) base_s += total;
    __syncthreads();
  }
  if (tid == 0) a.ncand[b] = base_s < a.kcap ? base_s : a.kcap;
}

__device__ __forceinline__ bool iou_gt(const float* A, float aa, const float* Bx, float ab, float thr) {
  float xx1 = fmaxf(A[0], Bx[0]), yy1 = fmaxf(A[1], Bx[1]);
  float xx2 = fminf(A[2], Bx[2]), yy2 = fminf(A[3], Bx[3]);
  float w = fmaxf(0.f, xx2 - xx1), h = fmaxf(0.f, yy2 - yy1);
  float inter = w * h;
  return inter / (aa + ab - inter) > thr;
}

// one wave per image
__global__ __launch_bounds__(64) void nms_greedy_kernel(NmsArgs a) {
  __shared__ float kb[304][4];
  __shared__ float ka[304];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int P = 5 + a.nc;
  const float* D = a.det + (size_t)b * a.rows * P;
  const unsigned long long* K = a.keys + (size_t)b * a.kcap;
  int n = a.ncand[b];
  if (n > a.max_nms) n = a.max_nms;
  float* O = a.out + (size_t)b * a.max_det * 6;
  int nk = 0;
  for (int base = 0; base < n && nk < a.max_det; base += 64) {
    int i = base + lane;
    bool alive = i < n;
    float box[4] = {0, 0, 0, 0}, raw[4] = {0, 0, 0, 0}, area = 0.f, score = 0.f;
    int cls = 0;
    if (alive) {
      unsigned long long key = K[i];
      unsigned int id = (unsigned int)key;
      int row = id / a.nc;
      cls = id - row * a.nc;
      const float* r = D + (size_t)row * P;
      score = r[5 + cls] * r[4];
      float off = (float)cls * a.max_wh;
#pragma unroll
      for (int k = 0; k < 4; ++k) { raw[k] = r[k]; box[k] = r[k] + off; }
      area = (box[2] - box[0]) * (box[3] - box[1]);
      for (int k = 0; k < nk && alive; ++k)
        if (iou_gt(kb[k], ka[k], box, area, a.iou_thr)) alive = false;
    }
    unsigned long long mask = __ballot(alive);
    while (mask && nk < a.max_det) {
      int j = __ffsll((long long)mask) - 1;          // earliest surviving candidate of the batch: kept
      float jb[4], jarea;
#pragma unroll
      for (int k = 0; k < 4; ++k) jb[k] = __shfl(box[k], j, 64);
      jarea = __shfl(area, j, 64);
      if (lane == j) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { kb[nk][k] = box[k]; O[nk * 6 + k] = raw[k]; }
        ka[nk] = area;
        O[nk * 6 + 4] = score;
        O[nk * 6 + 5] = (float)cls;
        alive = false;
      }
      if (alive && lane > j && iou_gt(jb, jarea, box, area, a.iou_thr)) alive = false;
      ++nk;
      mask = __ballot(alive);
      __syncthreads();
    }
    __syncthreads();
  }
  if (lane == 0) a.nout[b] = nk;
}

// the kept rows back into the source image, one thread per (image, output slot): x' = min(max((x - left) * scale_x, 0), width)
// and the same for y; runs behind the greedy pass, which stays as it is.  Rows beyond nout[b] are not touched.
__global__ __launch_bounds__(256) void nms_unletterbox_kernel(float* out, const int* nout, const KodLetterbox* lb, int B, int max_det) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * max_det) return;
  const int b = i / max_det;
  if (i - b * max_det >= nout[b]) return;
  const KodLetterbox L = lb[b];
  float* o = out + (size_t)i * 6;
  o[0] = fminf(fmaxf((o[0] - L.left) * L.scale_x, 0.f), L.width);
  o[1] = fminf(fmaxf((o[1] - L.top) * L.scale_y, 0.f), L.height);
  o[2] = fminf(fmaxf((o[2] - L.left) * L.scale_x, 0.f), L.width);
  o[3] = fminf(fmaxf((o[3] - L.top) * L.scale_y, 0.f), L.height);
}

// the launches of kodhip_nms / kodhip_nms_ex (arguments already checked).  best_class = 0 and keep = null: the candidate
// kernel of kodhip_nms; lb = null: nothing behind the greedy pass.
int nms_launch(const NmsArgs& a, int best_class, const unsigned char* keep, const KodLetterbox* lb, hipStream_t stream) {
  const int B = a.B;
  if (best_class)
    hipLaunchKernelGGL(nms_candidates_ex_kernel<true>, dim3(B), dim3(1024), 0, stream, a, keep);
  else if (keep)
    hipLaunchKernelGGL(nms_candidates_ex_kernel<false>, dim3(B), dim3(1024), 0, stream, a, keep);
  else
    hipLaunchKernelGGL(nms_candidates_kernel, dim3(B), dim3(1024), 0, stream, a);
  KOD_LAUNCH_CHECK("nms_candidates");
  key_sort_launch(a, B, stream);
  KOD_LAUNCH_CHECK("nms_sort");
  hipLaunchKernelGGL(nms_greedy_kernel, dim3(B), dim3(64), 0, stream, a);
  KOD_LAUNCH_CHECK("nms_greedy");
  if (lb) {
    hipLaunchKernelGGL(nms_unletterbox_kernel, dim3(cdiv((long)B * a.max_det, 256)), dim3(256), 0, stream, a.out, a.nout, lb, B, a.max_det);
    KOD_LAUNCH_CHECK("nms_unletterbox");
  }
  return KOD_OK;
}

}  // namespace

extern "C" {

struct KodDecodeLevel { const float* raw; int h, w, stride; float anchor_w[3], anchor_h[3]; };

// det [B][sum A*h*w][5+nc] fp32 from the three head tensors [B][A][h][w][5+nc] (anchors in pixels)
int kodhip_decode(const KodDecodeLevel* levels /* host[3] */, float* det, int B, int A, int nc, hipStream_t stream) {
  KOD_CHECK_ARG(levels && det && B > 0 && A == 3 && nc > 0, "decode: bad args (3 anchors per cell)");
  DecodeArgs a = {};
  int row0 = 0;
  for (int l = 0; l < 3; ++l) {
    KOD_CHECK_ARG(levels[l].raw, "decode: null level");
    a.lv[l].raw = levels[l].raw; a.lv[l].h = levels[l].h; a.lv[l].w = levels[l].w; a.lv[l].stride = levels[l].stride;
    a.lv[l].row0 = row0;
    for (int k = 0; k < 3; ++k) { a.lv[l].aw[k] = levels[l].anchor_w[k]; a.lv[l].ah[k] = levels[l].anchor_h[k]; }
    row0 += A * levels[l].h * levels[l].w;
  }
  a.det = det; a.B = B; a.A = A; a.nc = nc; a.rows = row0;
  hipLaunchKernelGGL(decode_kernel, dim3(cdiv((long)B * row0, 256)), dim3(256), 0, stream, a);
  KOD_LAUNCH_CHECK("decode");
  return KOD_OK;
}

// kodhip_decode for one view of a merged [B][rows_total][5+nc] tensor (test-time augmentation).  `levels` are the view's
// own three head tensors (h, w, stride of the VIEW's shape); level l takes part when bit l of level_mask is set (a
// masked-out level may have a null `raw`).  The view's rows - the unmasked levels in level order - go to
// [row_offset, row_offset + own rows) of every image; the box is brought back into the full-size frame first:
// cx, cy, w, h each divided by `scale`, then cx = full_width - cx when flip_lr, then the corners as in kodhip_decode.
// scale = 1, flip_lr = 0, level_mask = 7, row_offset = 0, rows_total = own rows: kodhip_decode bit for bit.
int kodhip_decode_view(const KodDecodeLevel* levels /* host[3] */, float* det, int B, int A, int nc, float scale, int flip_lr,
                       float full_width, int level_mask, int row_offset, int rows_total, hipStream_t stream) {
  KOD_CHECK_ARG(levels && det && B > 0 && A == 3 && nc > 0, "decode_view: bad args (3 anchors per cell)");
  KOD_CHECK_ARG(level_mask > 0 && level_mask < 8, "decode_view: level_mask must select at least one of the three levels");
  KOD_CHECK_ARG(scale > 0.f && (flip_lr == 0 || flip_lr == 1), "decode_view: scale must be positive, flip_lr 0 or 1");
  DecodeArgs a = {};
  int row0 = 0;
  for (int l = 0; l < 3; ++l) {
    const bool on = (level_mask >> l) & 1;
    KOD_CHECK_ARG(!on || (levels[l].raw && levels[l].h > 0 && levels[l].w > 0), "decode_view: null or empty level");
    a.lv[l].raw = levels[l].raw; a.lv[l].h = levels[l].h; a.lv[l].w = levels[l].w; a.lv[l].stride = levels[l].stride;
    a.lv[l].row0 = row0;
    for (int k = 0; k < 3; ++k) { a.lv[l].aw[k] = levels[l].anchor_w[k]; a.lv[l].ah[k] = levels[l].anchor_h[k]; }
    if (on) row0 += A * levels[l].h * levels[l].w;
  }
  KOD_CHECK_ARG(row_offset >= 0 && (long)row_offset + row0 <= rows_total, "decode_view: the view's rows do not fit in rows_total");
  a.det = det; a.B = B; a.A = A; a.nc = nc; a.rows = row0;
  DecodeView v = {scale, full_width, flip_lr, row_offset, rows_total};
  hipLaunchKernelGGL(decode_view_kernel, dim3(cdiv((long)B * row0, 256)), dim3(256), 0, stream, a, v);
  KOD_LAUNCH_CHECK("decode_view");
  return KOD_OK;
}

// keys: B * key_cap u64 workspace (key_cap = power of two >= rows*nc, or smaller to cap candidates);
// out [B][max_det][6] (x1,y1,x2,y2,score,cls), nout [B], ncand [B].
int kodhip_nms(const float* det, void* keys, int key_cap, int* ncand, float* out, int* nout,
               int B, int rows, int nc, float conf_thres, float nms_thres, int max_det, int max_nms, float max_wh,
               hipStream_t stream) {
  KOD_CHECK_ARG(det && keys && ncand && out && nout && B > 0 && rows > 0 && nc > 0, "nms: bad args");
  KOD_CHECK_ARG(key_cap >= 64 && (key_cap & (key_cap - 1)) == 0, "nms: key_cap must be a power of two >= 64");
  KOD_CHECK_ARG(max_det > 0 && max_det <= 300 && max_nms > 0, "nms: max_det must be in 1..300");
  KOD_CHECK_ARG((long)rows * nc < (1l << 31), "nms: too many candidates");
  NmsArgs a = {};
  a.det = det; a.keys = (unsigned long long*)keys; a.ncand = ncand; a.out = out; a.nout = nout;
  a.B = B; a.rows = rows; a.nc = nc; a.kcap = key_cap; a.max_det = max_det; a.max_nms = max_nms;
  a.conf = conf_thres; a.iou_thr = nms_thres; a.max_wh = max_wh;
  return nms_launch(a, 0, nullptr, nullptr, stream);
}


int kodhip_letterbox_bytes(void) { return (int)sizeof(KodLetterbox); }

// kodhip_nms with the deployment options.  best_class: one candidate per row (key_cap >= rows holds them all);
// class_keep [nc] u8: candidates of a class with 0 are dropped (best_class: after the argmax); letterbox [B]: the rows
// written to `out` are mapped back and clipped.  best_class = 0 with both pointers null is kodhip_nms launch for launch.
// Class-agnostic suppression is max_wh = 0.
int kodhip_nms_ex(const float* det, void* keys, int key_cap, int* ncand, float* out, int* nout,
                  int B, int rows, int nc, float conf_thres, float nms_thres, int max_det, int max_nms, float max_wh,
                  int best_class, const unsigned char* class_keep, const KodLetterbox* letterbox, hipStream_t stream) {
  KOD_CHECK_ARG(det && keys && ncand && out && nout && B > 0 && rows > 0 && nc > 0, "nms_ex: bad args");
  KOD_CHECK_ARG(key_cap >= 64 && (key_cap & (key_cap - 1)) == 0, "nms_ex: key_cap must be a power of two >= 64");
  KOD_CHECK_ARG(max_det > 0 && max_det <= 300 && max_nms > 0, "nms_ex: max_det must be in 1..300");
  KOD_CHECK_ARG(best_class == 0 || best_class == 1, "nms_ex: best_class must be 0 or 1");
  KOD_CHECK_ARG((long)rows * nc < (1l << 31), "nms_ex: too many candidates");
  NmsArgs a = {};
  a.det = det; a.keys = (unsigned long long*)keys; a.ncand = ncand; a.out = out; a.nout = nout;
  a.B = B; a.rows = rows; a.nc = nc; a.kcap = key_cap; a.max_det = max_det; a.max_nms = max_nms;
  a.conf = conf_thres; a.iou_thr = nms_thres; a.max_wh = max_wh;
  return nms_launch(a, best_class, class_keep, letterbox, stream);
}

}  // extern "C"
