// Weight EMA (YOLOv5 utils/torch_utils.py ModelEMA.update: `v *= d; v += (1 - d) * msd[k]` over every floating-point entry of
// the state dict) and the exchange that puts the averaged weights into the network for validation, each as ONE launch over up
// to four flat segments - the engine's parameter arena and its two BatchNorm statistic arenas (engine/ema.py).
//
// Update, per element, all fp32 and every operation rounded on its own (the library is built with -ffp-contract=off and the
// operations are spelled __fmul_rn / __fadd_rn besides):  e = fl( fl(e * d) + fl(omd * m) ).  d and omd arrive as two fp32
// values: the host forms 1 - d in double before it rounds, which is what torch does with a Python double; the kernel never
// forms 1 - d.  Swap is a copy of 32-bit words, so NaN payloads survive.
//
// The segment table travels by value in the kernel arguments (no device table, no upload).  A block owns EMA_CHUNK consecutive
// elements of one segment and finds its segment through the prefix of the per-segment block counts.  A segment whose two bases
// are 16-byte aligned goes through 16-byte loads and stores (four independent ones per lane and side), the numel % 4 elements
// behind them one lane each; any other 4-byte aligned pair of bases takes the one-element-per-lane path.  Nothing at or
// beyond numel is read or written.
#include "kodhip_common.h"

namespace {

constexpr int EMA_MAX_SEG = 4;
constexpr int EMA_THREADS = 256;
constexpr int EMA_UNROLL = 4;                                    // 16-byte accesses per lane and side
constexpr long EMA_CHUNK = (long)EMA_THREADS * 4 * EMA_UNROLL;   // elements per block: 4096 (16 KiB per side)

struct EmaArgs {
  const float* m[EMA_MAX_SEG];   // update: the model side (read only); swap: side a
  float* e[EMA_MAX_SEG];         // update: the shadow (read, written); swap: side b
  long n[EMA_MAX_SEG];
  int start[EMA_MAX_SEG];        // first block of the segment
  int vec[EMA_MAX_SEG];          // both bases 16-byte aligned
  int nseg;
  float d, omd;
};

__device__ __forceinline__ float ema_mix(float e, float m, float d, float omd) { return __fadd_rn(__fmul_rn(e, d), __fmul_rn(omd, m)); }

template <bool SWAP> __global__ __launch_bounds__(EMA_THREADS) void ema_kernel(EmaArgs a) {
  // the block's segment: the last one that starts at or before it (block-uniform; static indices into the by-value table)
  const float* mp = a.m[0];
  float* ep = a.e[0];
  long n = a.n[0];
  int first = 0, vec = a.vec[0];
#pragma unroll
  for (int k = 1; k < EMA_MAX_SEG; ++k) {
    if (k < a.nseg && (int)blockIdx.x >= a.start[k]) {
      mp = a.m[k]; ep = a.e[k]; n = a.n[k]; first = a.start[k]; vec = a.vec[k];
    }
  }
  const int b = (int)blockIdx.x - first;
  const long base = (long)b * EMA_CHUNK;
  const int tid = (int)threadIdx.x;
  float* mw = const_cast<float*>(mp);            // (written by the swap only)
  if (vec) {
    const long n4 = n & ~3l;
    long i[EMA_UNROLL];
    u32x4 mv[EMA_UNROLL], ev[EMA_UNROLL];
#pragma unroll
    for (int u = 0; u < EMA_UNROLL; ++u) {
      i[u] = base + ((long)u * EMA_THREADS + tid) * 4;
      if (i[u] < n4) {                           // (both multiples of 4: the whole quad lies below n4)
        mv[u] = *reinterpret_cast<const u32x4*>(mp + i[u]);
        ev[u] = *reinterpret_cast<const u32x4*>(ep + i[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < EMA_UNROLL; ++u) {
      if (i[u] < n4) {
        if (SWAP) {
          *reinterpret_cast<u32x4*>(mw + i[u]) = ev[u];
          *reinterpret_cast<u32x4*>(ep + i[u]) = mv[u];
        } else {
          u32x4 o;
#pragma unroll
          for (int c = 0; c < 4; ++c) o[c] = __float_as_uint(ema_mix(__uint_as_float(ev[u][c]), __uint_as_float(mv[u][c]), a.d, a.omd));
          *reinterpret_cast<u32x4*>(ep + i[u]) = o;
        }
      }
    }
    // the numel % 4 elements behind the last quad: one lane each, in the block whose chunk holds them
    if (n4 < n && n4 / EMA_CHUNK == b && tid < (int)(n - n4)) {
      const long j = n4 + tid;
      unsigned int* eu = reinterpret_cast<unsigned int*>(ep);
      unsigned int* mu = reinterpret_cast<unsigned int*>(mw);
      const unsigned int x = mu[j], y = eu[j];
      if (SWAP) { mu[j] = y; eu[j] = x; }
      else eu[j] = __float_as_uint(ema_mix(__uint_as_float(y), __uint_as_float(x), a.d, a.omd));
    }
    return;
  }
  unsigned int* eu = reinterpret_cast<unsigned int*>(ep);
  unsigned int* mu = reinterpret_cast<unsigned int*>(mw);
  const long end = base + EMA_CHUNK < n ? base + EMA_CHUNK : n;
  for (long j = base + tid; j < end; j += EMA_THREADS) {
    const unsigned int x = mu[j], y = eu[j];
    if (SWAP) { mu[j] = y; eu[j] = x; }
    else eu[j] = __float_as_uint(ema_mix(__uint_as_float(y), __uint_as_float(x), a.d, a.omd));
  }
}

bool ema_overlap(const void* p, long np, const void* q, long nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + (uintptr_t)nq * 4 && b < a + (uintptr_t)np * 4;
}

// Validates the host tables and builds the by-value kernel arguments over the segments with numel > 0.  Returns KOD_OK with
// *blocks = 0 when there is nothing to do.  both_written: the first side is written too (swap), so its segments must not
// overlap each other either.
int ema_args(const char* fn, const void* const* m, void* const* e, const long* numels, int nseg, bool both_written, EmaArgs& a,
             int* blocks) {
  KOD_CHECK_ARG(nseg >= 1 && nseg <= EMA_MAX_SEG, "%s: nseg %d: expected 1 .. %d", fn, nseg, EMA_MAX_SEG);
  KOD_CHECK_ARG(m && e && numels, "%s: null segment table", fn);
  for (int k = 0; k < nseg; ++k) {
    KOD_CHECK_ARG(numels[k] >= 0, "%s: segment %d: negative numel", fn, k);
    KOD_CHECK_ARG(numels[k] == 0 || (m[k] && e[k]), "%s: segment %d: null pointer", fn, k);
    KOD_CHECK_ARG(numels[k] == 0 || ((((uintptr_t)m[k] | (uintptr_t)e[k]) & 3) == 0), "%s: segment %d: base not 4-byte aligned", fn, k);
  }
  for (int j = 0; j < nseg; ++j) {
    for (int k = 0; k < nseg; ++k) {
      if (numels[j] == 0 || numels[k] == 0) continue;
      KOD_CHECK_ARG(!ema_overlap(m[j], numels[j], e[k], numels[k]), "%s: segments %d and %d of the two sides alias", fn, j, k);
      if (j < k) {
        KOD_CHECK_ARG(!ema_overlap(e[j], numels[j], e[k], numels[k]), "%s: written segments %d and %d overlap", fn, j, k);
        KOD_CHECK_ARG(!both_written || !ema_overlap(m[j], numels[j], m[k], numels[k]), "%s: written segments %d and %d overlap", fn, j, k);
      }
    }
  }
  a = EmaArgs{};
  long total = 0;
  int s = 0;
  for (int k = 0; k < nseg; ++k) {
    if (numels[k] == 0) continue;
    a.m[s] = (const float*)m[k];
    a.e[s] = (float*)e[k];
    a.n[s] = numels[k];
    a.start[s] = (int)total;
    a.vec[s] = ((((uintptr_t)m[k] | (uintptr_t)e[k]) & 15) == 0) ? 1 : 0;
    total += (numels[k] + EMA_CHUNK - 1) / EMA_CHUNK;
    KOD_CHECK_ARG(total < (1l << 31), "%s: too many elements for one launch", fn);
    ++s;
  }
  a.nseg = s;
  *blocks = (int)total;
  return KOD_OK;
}

}  // namespace

extern "C" {

int kodhip_ema_update(const float* const* model_ptrs, float* const* shadow_ptrs, const long* numels, int nseg, float d, float omd,
                      hipStream_t stream) {
  EmaArgs a;
  int blocks = 0;
  const int rc = ema_args("ema_update", (const void* const*)model_ptrs, (void* const*)shadow_ptrs, numels, nseg, false, a, &blocks);
  if (rc != KOD_OK) return rc;
  if (blocks == 0) return KOD_OK;
  a.d = d;
  a.omd = omd;
  hipLaunchKernelGGL(ema_kernel<false>, dim3(blocks), dim3(EMA_THREADS), 0, stream, a);
  KOD_LAUNCH_CHECK("ema_update");
  return KOD_OK;
}

int kodhip_ema_swap(void* const* a_ptrs, void* const* b_ptrs, const long* numels, int nseg, hipStream_t stream) {
  EmaArgs a;
  int blocks = 0;
  const int rc = ema_args("ema_swap", (const void* const*)a_ptrs, b_ptrs, numels, nseg, true, a, &blocks);
  if (rc != KOD_OK) return rc;
  if (blocks == 0) return KOD_OK;
  hipLaunchKernelGGL(ema_kernel<true>, dim3(blocks), dim3(EMA_THREADS), 0, stream, a);
  KOD_LAUNCH_CHECK("ema_swap");
  return KOD_OK;
}

}  // extern "C"
