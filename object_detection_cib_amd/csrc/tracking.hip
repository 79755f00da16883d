// Multi-object tracking in ByteTrack's form (Zhang et al., ECCV 2022): boxes and scores in, identities out.  One block per
// stream, serial in time (a stream's F frames run one after the other inside one launch), parallel over tracks, detections
// and pairs.  All state lives in the caller's device buffer; nothing is read back, allocated or waited for, and every loop
// is bounded by cap and max_rows, so a launch can be captured in a hipGraph.
//
//   state      : per stream a 16-byte header {frame, next_id, dropped, pad} and cap records KodTrack (include/kodhip.h).
//                Record t belongs to thread t % 256: only that thread reads or writes it, so the records stay in global
//                memory (L2) and no ordering between threads is needed for them.  What other threads must see of a track -
//                its box, class, state and match - is mirrored in LDS.
//   filter     : ByteTrack's 8-state constant-velocity Kalman filter.  With F = [[I, I], [0, I]], H = [I 0] and diagonal
//                noise its covariance never leaves four independent 2 x 2 blocks, so a coordinate is five floats (p, v,
//                Ppp, Ppv, Pvv) and predict / update are a dozen scalar operations in registers: no 8 x 8 matrix, no inverse.
//   association: greedy and fully ordered - the admissible pairs by similarity descending, equal similarities by lower
//                slot, then lower row; a pair is accepted iff neither side is taken.  Computed as rounds of mutual best
//                choices: every open track picks its best open detection (ties to the lower row), every open detection its
//                best open track (ties to the lower slot), and the pairs that picked each other are accepted.  The first
//                pair of the order among the open ones is always mutual, and a mutual pair has no earlier pair on either
//                side, so the rounds reach the sorted pass's result; at most min(tracks, detections) rounds, usually two or
//                three.  The similarities are recomputed per round from the boxes in LDS (1024 x 300 of them would not fit);
//                the open tracks and rows are bit masks (ballots), so a round walks only what is still open, and a pair
//                without an intersection is dropped before the division.
//   compaction : free slots, detections that start a track and the emitted tracks are ranked by wave 0 with ballots.
//
// LDS at cap 1024: track mirror 36 KiB + detections 11 KiB.  Every operation is fp32 and rounded on its own (the library
// is built with -ffp-contract=off; fp32 division is correctly rounded).
#include "kodhip_common.h"

#define KOD_TRACK_MAX_ROWS 300
#define KOD_TRACK_MIN_CAP 64
#define KOD_TRACK_MAX_CAP 1024

namespace {

struct KodTrackHeader { int frame, next_id, dropped, pad; };
struct KodTrack {
  int state, id, last_frame, start_frame;
  float score, cls;
  float kf[4][5];               // per coordinate (cx, cy, a, h): p, v, Ppp, Ppv, Pvv
  int pad[2];
};
static_assert(sizeof(KodTrackHeader) == 16 && sizeof(KodTrack) == 112 && sizeof(KodTrack) % 16 == 0, "published layout");

enum { TRK_FREE = 0, TRK_NEW = 1, TRK_TRACKED = 2, TRK_LOST = 3 };
enum { DET_NONE = 0, DET_HIGH = 1, DET_LOW = 2 };

constexpr int TRK_THREADS = 256;
constexpr float TRK_WP = 0.05f, TRK_WV = 0.00625f;

struct TrackArgs {
  unsigned char* state;
  const float* rows;            // [S][F][max_rows][6]
  const int* counts;            // [S][F]
  float* out;                   // [S][F][cap][6]
  int* out_ids;                 // [S][F][cap][2]
  int* nout;                    // [S][F]
  int F, max_rows, cap, fuse_score, agnostic, max_lost;
  float high, low, newt, sim1, sim2, sim3;
};

constexpr size_t track_state_bytes(int cap) { return sizeof(KodTrackHeader) + (size_t)cap * sizeof(KodTrack); }
// track mirror: box 16 B, class, state, match, free list, choice / rank = 36 B per slot; detections: box 16 B, score, class,
// kind, taken-by, choice / starting rows = 36 B per row; three counts and the masks of the open tracks and rows
constexpr int TRK_ROW_WORDS = (KOD_TRACK_MAX_ROWS + 63) / 64;
constexpr size_t track_lds_bytes(int cap) { return (size_t)cap * 36 + KOD_TRACK_MAX_ROWS * 36 + 16 + (KOD_TRACK_MAX_CAP / 64 + TRK_ROW_WORDS) * 8; }

__device__ __forceinline__ float4 track_box(const float (*kf)[5]) {
  const float w = kf[2][0] * kf[3][0];
  const float x1 = kf[0][0] - w / 2.f, y1 = kf[1][0] - kf[3][0] / 2.f;
  return make_float4(x1, y1, x1 + w, y1 + kf[3][0]);
}

__device__ __forceinline__ void track_predict(float (*kf)[5]) {
  const float hh = kf[3][0];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float sp = c == 2 ? 1e-2f : TRK_WP * hh, sv = c == 2 ? 1e-5f : TRK_WV * hh;
    const float p = kf[c][0], v = kf[c][1], ppp = kf[c][2], ppv = kf[c][3], pvv = kf[c][4];
    kf[c][0] = p + v;
    kf[c][2] = ((ppp + 2.f * ppv) + pvv) + sp * sp;
    kf[c][3] = ppv + pvv;
    kf[c][4] = pvv + sv * sv;
  }
}

__device__ __forceinline__ void track_update(float (*kf)[5], const float* z) {
  const float hh = kf[3][0];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float sr = c == 2 ? 1e-1f : TRK_WP * hh;
    const float p = kf[c][0], v = kf[c][1], ppp = kf[c][2], ppv = kf[c][3], pvv = kf[c][4];
    const float S = ppp + sr * sr;
    const float kp = ppp / S, kv = ppv / S, y = z[c] - p;
    kf[c][0] = p + kp * y;
    kf[c][1] = v + kv * y;
    kf[c][2] = ppp - (kp * kp) * S;
    kf[c][3] = ppv - (kp * kv) * S;
    kf[c][4] = pvv - (kv * kv) * S;
  }
}

__device__ __forceinline__ void track_initiate(float (*kf)[5], const float* z) {
  const float h = z[3];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const float sp = c == 2 ? 1e-2f : 0.1f * h, sv = c == 2 ? 1e-5f : 0.0625f * h;
    kf[c][0] = z[c]; kf[c][1] = 0.f; kf[c][2] = sp * sp; kf[c][3] = 0.f; kf[c][4] = sv * sv;
  }
}

// a detection's box as the filter's measurement (cx, cy, a, h)
__device__ __forceinline__ void track_measure(const float4 b, float* z) {
  const float w = b.z - b.x, h = b.w - b.y;
  z[0] = b.x + w / 2.f; z[1] = b.y + h / 2.f; z[2] = w / h; z[3] = h;
}

// kodhip_fuse_detections' IoU, track A against detection B, times the detection's score where asked for
__device__ __forceinline__ float track_sim(const float4 A, const float4 B, float score, bool fuse) {
  const float w = fmaxf(0.f, fminf(A.z, B.z) - fmaxf(A.x, B.x));
  const float h = fmaxf(0.f, fminf(A.w, B.w) - fmaxf(A.y, B.y));
  const float inter = w * h;
  if (!(inter > 0.f)) return 0.f;                         // iou would be 0 or NaN: never above a threshold >= 0
  const float aa = (A.z - A.x) * (A.w - A.y), ab = (B.z - B.x) * (B.w - B.y);
  const float iou = inter / ((aa + ab) - inter);
  return fuse ? iou * score : iou;
}

__global__ __launch_bounds__(TRK_THREADS) void track_reset_kernel(unsigned char* state, int cap) {
  unsigned int* S = reinterpret_cast<unsigned int*>(state + (size_t)blockIdx.x * track_state_bytes(cap));
  const int words = (int)(track_state_bytes(cap) / 4);
  for (int i = threadIdx.x; i < words; i += TRK_THREADS) S[i] = i == 1 ? 1u : 0u;       // header {0, next_id = 1, 0, 0}
}

__global__ __launch_bounds__(TRK_THREADS) void track_update_kernel(TrackArgs a) {
  extern __shared__ float4 trk_lds[];
  const int cap = a.cap, R = KOD_TRACK_MAX_ROWS;
  float4* tb = trk_lds;                                   // [cap] box of the (predicted) filter
  float4* db = tb + cap;                                  // [R]   detection box
  float* tc = reinterpret_cast<float*>(db + R);           // [cap] class
  int* tst = reinterpret_cast<int*>(tc + cap);            // [cap] state
  int* tm = tst + cap;                                    // [cap] matched detection row, -1: none
  int* flist = tm + cap;                                  // [cap] the free slots, ascending
  int* tch = flist + cap;                                 // [cap] the round's choice; later creation rank, output rank
  float* dsc = reinterpret_cast<float*>(tch + cap);       // [R] score
  float* dcl = dsc + R;                                   // [R] class
  int* dkind = reinterpret_cast<int*>(dcl + R);           // [R] DET_*
  int* dtk = dkind + R;                                   // [R] taken by slot, -1: free
  int* dch = dtk + R;                                     // [R] the round's choice; later the rows that start a track
  int* cnt = dch + R;                                     // [0] free slots, [1] starting rows (16 bytes)
  unsigned long long* tmask = reinterpret_cast<unsigned long long*>(cnt + 4);   // [cap / 64] tracks open in the current association
  unsigned long long* dmask = tmask + KOD_TRACK_MAX_CAP / 64;                   // [ceil(n / 64)] rows open in it

  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave64 = tid & ~63;
  unsigned char* base = a.state + (size_t)s * track_state_bytes(cap);
  KodTrackHeader* hdr = reinterpret_cast<KodTrackHeader*>(base);
  KodTrack* rec = reinterpret_cast<KodTrack*>(base + sizeof(KodTrackHeader));
  const bool agn = a.agnostic != 0;
  int frame = hdr->frame, next_id = hdr->next_id, dropped = hdr->dropped;      // (uniform; written back by thread 0 at the end)

  for (int f = 0; f < a.F; ++f) {
    frame += 1;
    const size_t sf = (size_t)s * a.F + f;
    const float* rows = a.rows + sf * a.max_rows * 6;
    const int n = min(max(a.counts[sf], 0), a.max_rows);
    __syncthreads();                                      // the frame before this one has been read
    // ---- detections: box, score, class, kind
    for (int d = tid; d < n; d += TRK_THREADS) {
      const float* r = rows + (size_t)d * 6;
      const float4 b = make_float4(r[0], r[1], r[2], r[3]);
      const float sc = r[4];
      const float w = b.z - b.x, h = b.w - b.y;
      int kind = DET_NONE;
      if (w > 0.f && h > 0.f && sc == sc) kind = sc > a.high ? DET_HIGH : (sc > a.low ? DET_LOW : DET_NONE);
      db[d] = b; dsc[d] = sc; dcl[d] = r[5]; dkind[d] = kind; dtk[d] = -1;
    }
    // ---- 1. predict (tracked and lost; a lost track's height stops changing), the boxes the associations compare
    for (int t = tid; t < cap; t += TRK_THREADS) {
      KodTrack* k = rec + t;
      const int st = k->state;
      tst[t] = st; tm[t] = -1;
      if (st != TRK_FREE) {
        float kf[4][5];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 5; ++j) kf[c][j] = k->kf[c][j];
        if (st != TRK_NEW) {
          if (st == TRK_LOST) kf[3][1] = 0.f;
          track_predict(kf);
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int j = 0; j < 5; ++j) k->kf[c][j] = kf[c][j];
        }
        tb[t] = track_box(kf);
        tc[t] = k->cls;
      }
    }
    // ---- 3., 4., 6. the three associations
    for (int phase = 0; phase < 3; ++phase) {
      const float thr = phase == 0 ? a.sim1 : (phase == 1 ? a.sim2 : a.sim3);
      const bool fuse = phase != 1 && a.fuse_score != 0;
      const int want = phase == 1 ? DET_LOW : DET_HIGH;
      __syncthreads();                                    // tst / tm / dkind / dtk as the steps before left them
      for (int t0 = wave64; t0 < cap; t0 += TRK_THREADS) {          // (wave-uniform bounds: a wave's ballot is one word)
        const int t = t0 + lane, st = tst[t];
        const bool in = phase == 0 ? (st == TRK_TRACKED || st == TRK_LOST) : (phase == 1 ? st == TRK_TRACKED : st == TRK_NEW);
        const unsigned long long m = __ballot(in && tm[t] < 0);
        if (lane == 0) tmask[t0 >> 6] = m;
      }
      for (int d0 = wave64; d0 < n; d0 += TRK_THREADS) {
        const int d = d0 + lane;
        const unsigned long long m = __ballot(d < n && dkind[d] == want && dtk[d] < 0);
        if (lane == 0) dmask[d0 >> 6] = m;
      }
      __syncthreads();
      const int twords = cap >> 6, dwords = (n + 63) >> 6;
      const int rounds = min(cap, n) + 1;                 // every round but the last accepts a pair
      for (int round = 0; round < rounds; ++round) {
        for (int t = tid; t < cap; t += TRK_THREADS) {    // a track's best open detection, equal similarities: the lower row
          int pick = -1;
          if ((tmask[t >> 6] >> (t & 63)) & 1ull) {
            const float4 A = tb[t];
            const float cls = tc[t];
            float best = thr;
            for (int w = 0; w < dwords; ++w) {
              for (unsigned long long m = dmask[w]; m; m &= m - 1) {
                const int d = (w << 6) + __builtin_ctzll(m);
                if (!agn && cls != dcl[d]) continue;
                const float sim = track_sim(A, db[d], dsc[d], fuse);
                if (sim > best) { best = sim; pick = d; }
              }
            }
          }
          tch[t] = pick;
        }
        for (int d = tid; d < n; d += TRK_THREADS) {      // a detection's best open track, equal similarities: the lower slot
          int pick = -1;
          if ((dmask[d >> 6] >> (d & 63)) & 1ull) {
            const float4 B = db[d];
            const float cls = dcl[d], sc = dsc[d];
            float best = thr;
            for (int w = 0; w < twords; ++w) {
              for (unsigned long long m = tmask[w]; m; m &= m - 1) {
                const int t = (w << 6) + __builtin_ctzll(m);
                if (!agn && tc[t] != cls) continue;
                const float sim = track_sim(tb[t], B, sc, fuse);
                if (sim > best) { best = sim; pick = t; }
              }
            }
          }
          dch[d] = pick;
        }
        __syncthreads();
        int any = 0;
        for (int t = tid; t < cap; t += TRK_THREADS) {
          const int d = tch[t];
          if (d >= 0 && dch[d] == t) {
            tm[t] = d; dtk[d] = t; any = 1;
            atomicAnd(&tmask[t >> 6], ~(1ull << (t & 63)));
            atomicAnd(&dmask[d >> 6], ~(1ull << (d & 63)));
          }
        }
        if (!__syncthreads_or(any)) break;                // (block-uniform)
      }
    }
    // ---- matched tracks are updated; 5. unmatched tracked -> lost; unmatched new -> free
    for (int t = tid; t < cap; t += TRK_THREADS) {
      const int st = tst[t], d = tm[t];
      tch[t] = -1;
      if (st == TRK_FREE) continue;
      KodTrack* k = rec + t;
      if (d >= 0) {
        float kf[4][5], z[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 5; ++j) kf[c][j] = k->kf[c][j];
        track_measure(db[d], z);
        track_update(kf, z);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 5; ++j) k->kf[c][j] = kf[c][j];
        k->state = TRK_TRACKED; k->score = dsc[d]; k->cls = dcl[d]; k->last_frame = frame;
        tst[t] = TRK_TRACKED;
      } else if (st == TRK_TRACKED) {
        k->state = TRK_LOST; tst[t] = TRK_LOST;
      } else if (st == TRK_NEW) {
        k->state = TRK_FREE; tst[t] = TRK_FREE;
      }
    }
    __syncthreads();
    // ---- 7. the free slots ascending and the rows that start a track, in row order (wave 0)
    if (tid < 64) {
      int nf = 0;
      for (int t0 = 0; t0 < cap; t0 += 64) {
        const bool fr = tst[t0 + lane] == TRK_FREE;
        const unsigned long long m = __ballot(fr);
        if (fr) flist[nf + __popcll(m & ((1ull << lane) - 1ull))] = t0 + lane;
        nf += __popcll(m);
      }
      int ncr = 0;
      for (int d0 = 0; d0 < n; d0 += 64) {
        const int d = d0 + lane;
        const bool cr = d < n && dkind[d] == DET_HIGH && dtk[d] < 0 && dsc[d] >= a.newt;
        const unsigned long long m = __ballot(cr);
        if (cr) dch[ncr + __popcll(m & ((1ull << lane) - 1ull))] = d;
        ncr += __popcll(m);
      }
      if (lane == 0) { cnt[0] = nf; cnt[1] = ncr; }
    }
    __syncthreads();
    const int nf = cnt[0], ncr = cnt[1], made = min(nf, ncr);
    for (int r = tid; r < made; r += TRK_THREADS) tch[flist[r]] = r;            // slot -> creation rank
    __syncthreads();
    // ---- creation by the slot's owner; 8. lost for too long -> free
    for (int t = tid; t < cap; t += TRK_THREADS) {
      KodTrack* k = rec + t;
      const int r = tch[t];
      if (r >= 0) {
        const int d = dch[r];
        float kf[4][5], z[4];
        track_measure(db[d], z);
        track_initiate(kf, z);
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int j = 0; j < 5; ++j) k->kf[c][j] = kf[c][j];
        const int st = frame == 1 ? TRK_TRACKED : TRK_NEW;
        k->state = st; k->id = next_id + r; k->last_frame = frame; k->start_frame = frame;
        k->score = dsc[d]; k->cls = dcl[d];
        tst[t] = st; tm[t] = d;
      } else if (tst[t] == TRK_LOST && frame - k->last_frame > a.max_lost) {
        k->state = TRK_FREE; tst[t] = TRK_FREE;
      }
    }
    next_id += made;
    dropped += ncr - made;
    __syncthreads();
    // ---- 9. the tracked ones by slot ascending
    if (tid < 64) {
      int no = 0;
      for (int t0 = 0; t0 < cap; t0 += 64) {
        const bool o = tst[t0 + lane] == TRK_TRACKED;
        const unsigned long long m = __ballot(o);
        tch[t0 + lane] = o ? no + __popcll(m & ((1ull << lane) - 1ull)) : -1;
        no += __popcll(m);
      }
      if (lane == 0) a.nout[sf] = no;
    }
    __syncthreads();
    float* O = a.out + sf * cap * 6;
    int* I = a.out_ids + sf * cap * 2;
    for (int t = tid; t < cap; t += TRK_THREADS) {
      const int r = tch[t];
      if (r < 0) continue;
      const KodTrack* k = rec + t;                        // (this thread's own writes)
      float kf[4][5];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int j = 0; j < 5; ++j) kf[c][j] = k->kf[c][j];
      const float4 b = track_box(kf);
      O[r * 6 + 0] = b.x; O[r * 6 + 1] = b.y; O[r * 6 + 2] = b.z; O[r * 6 + 3] = b.w;
      O[r * 6 + 4] = k->score; O[r * 6 + 5] = k->cls;
      I[r * 2 + 0] = k->id; I[r * 2 + 1] = tm[t];
    }
  }
  if (tid == 0) { hdr->frame = frame; hdr->next_id = next_id; hdr->dropped = dropped; }
}

bool track_cap_ok(int cap) { return cap >= KOD_TRACK_MIN_CAP && cap <= KOD_TRACK_MAX_CAP && (cap & (cap - 1)) == 0; }

}  // namespace

extern "C" {

int kodhip_track_header_bytes(void) { return (int)sizeof(KodTrackHeader); }
int kodhip_track_bytes(void) { return (int)sizeof(KodTrack); }
long long kodhip_track_workspace_bytes(int S, int cap, int max_rows) { (void)S; (void)cap; (void)max_rows; return 0; }

int kodhip_track_reset(void* state, int S, int cap, hipStream_t stream) {
  KOD_CHECK_ARG(state, "track_reset: null pointer");
  KOD_CHECK_ARG(S >= 1 && S <= 65535, "track_reset: S must be in 1..65535");
  KOD_CHECK_ARG(track_cap_ok(cap), "track_reset: cap must be a power of two in %d..%d", KOD_TRACK_MIN_CAP, KOD_TRACK_MAX_CAP);
  hipLaunchKernelGGL(track_reset_kernel, dim3(S), dim3(TRK_THREADS), 0, stream, (unsigned char*)state, cap);
  KOD_LAUNCH_CHECK("track_reset");
  return KOD_OK;
}

int kodhip_track_update(void* state, const float* rows, const int* counts, int S, int F, int max_rows, int cap, float high_thres,
                        float low_thres, float new_thres, float sim1, float sim2, float sim3, int fuse_score, int agnostic,
                        int max_lost, float* out, int* out_ids, int* nout, void* workspace, hipStream_t stream) {
  (void)workspace;                                        // kodhip_track_workspace_bytes() is 0: never read, may be null
  KOD_CHECK_ARG(state && rows && counts && out && out_ids && nout, "track_update: null pointer");
  KOD_CHECK_ARG(S >= 1 && S <= 65535 && F >= 1, "track_update: S must be in 1..65535, F >= 1");
  KOD_CHECK_ARG(max_rows >= 1 && max_rows <= KOD_TRACK_MAX_ROWS, "track_update: max_rows must be in 1..%d", KOD_TRACK_MAX_ROWS);
  KOD_CHECK_ARG(track_cap_ok(cap), "track_update: cap must be a power of two in %d..%d", KOD_TRACK_MIN_CAP, KOD_TRACK_MAX_CAP);
  const float th[6] = {high_thres, low_thres, new_thres, sim1, sim2, sim3};
  for (int i = 0; i < 6; ++i) KOD_CHECK_ARG(th[i] >= 0.f && th[i] <= 1.f, "track_update: thresholds must be in [0, 1]");
  KOD_CHECK_ARG(low_thres <= high_thres, "track_update: low_thres above high_thres");
  KOD_CHECK_ARG((fuse_score == 0 || fuse_score == 1) && (agnostic == 0 || agnostic == 1), "track_update: fuse_score and agnostic must be 0 or 1");
  KOD_CHECK_ARG(max_lost >= 0, "track_update: max_lost must be >= 0");
  TrackArgs a = {};
  a.state = (unsigned char*)state; a.rows = rows; a.counts = counts; a.out = out; a.out_ids = out_ids; a.nout = nout;
  a.F = F; a.max_rows = max_rows; a.cap = cap; a.fuse_score = fuse_score; a.agnostic = agnostic; a.max_lost = max_lost;
  a.high = high_thres; a.low = low_thres; a.newt = new_thres; a.sim1 = sim1; a.sim2 = sim2; a.sim3 = sim3;
  hipLaunchKernelGGL(track_update_kernel, dim3(S), dim3(TRK_THREADS), track_lds_bytes(cap), stream, a);   // (<= 48 KiB of LDS)
  KOD_LAUNCH_CHECK("track_update");
  return KOD_OK;
}

}  // extern "C"
