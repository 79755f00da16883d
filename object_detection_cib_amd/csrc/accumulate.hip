// Gradient accumulation (Lightning's Trainer(accumulate_grad_batches), YOLOv5 train.py's `accumulate`): what autograd's
// `.grad += g` does across backward() calls, as ONE launch over the flat gradient arena (engine/accumulate.py, engine/arenas.py).
//
// Per element, fp32:  acc = grad, a copy of the 32-bit word (the first micro-batch of a window: -0.0 stays -0.0 and a NaN keeps
// its payload; it is not an add to zero), or  acc = fl(acc + grad), one rounding (__fadd_rn; the library is built with
// -ffp-contract=off besides).  Which of the two is the launch's mode - or, in mode 2, a flag in device memory that the caller
// writes outside a captured graph, like the optimizer's `hyper`: one captured launch then serves every position of a window.
// The flag is read by every lane from the same address (uniform across the wave) and is only read.
//
// A block owns ACC_CHUNK consecutive elements.  Two bases that are 16-byte aligned go through 16-byte loads and stores (four
// independent ones per lane and side), the n % 4 elements behind them one lane each; any other 4-byte aligned pair of bases
// takes the one-element-per-lane path.  Nothing at or beyond n is read or written; the copy form never reads acc.
#include "kodhip_common.h"

namespace {

constexpr int ACC_THREADS = 256;
constexpr int ACC_UNROLL = 4;                                    // 16-byte accesses per lane and side
constexpr long ACC_CHUNK = (long)ACC_THREADS * 4 * ACC_UNROLL;   // elements per block: 4096 (16 KiB per side)

__device__ __forceinline__ unsigned int acc_add(unsigned int a, unsigned int g) {
  return __float_as_uint(__fadd_rn(__uint_as_float(a), __uint_as_float(g)));
}

template <int MODE, bool VEC> __global__ __launch_bounds__(ACC_THREADS) void grad_accumulate_kernel(
    float* __restrict__ acc, const float* __restrict__ grad, long n, const float* __restrict__ ctl) {
  const bool copy = MODE == 1 || (MODE == 2 && ctl[0] != 0.0f);
  const int b = (int)blockIdx.x;
  const long base = (long)b * ACC_CHUNK;
  const int tid = (int)threadIdx.x;
  unsigned int* au = reinterpret_cast<unsigned int*>(acc);
  const unsigned int* gu = reinterpret_cast<const unsigned int*>(grad);
  if (VEC) {
    const long n4 = n & ~3l;
    long i[ACC_UNROLL];
    u32x4 gv[ACC_UNROLL], av[ACC_UNROLL];
#pragma unroll
    for (int u = 0; u < ACC_UNROLL; ++u) {
      i[u] = base + ((long)u * ACC_THREADS + tid) * 4;
      if (i[u] < n4) {                           // (both multiples of 4: the whole quad lies below n4)
        gv[u] = *reinterpret_cast<const u32x4*>(gu + i[u]);
        if (!copy) av[u] = *reinterpret_cast<const u32x4*>(au + i[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < ACC_UNROLL; ++u) {
      if (i[u] < n4) {
        u32x4 o = gv[u];
        if (!copy) {
#pragma unroll
          for (int c = 0; c < 4; ++c) o[c] = acc_add(av[u][c], gv[u][c]);
        }
        *reinterpret_cast<u32x4*>(au + i[u]) = o;
      }
    }
    // the n % 4 elements behind the last quad: one lane each, in the block whose chunk holds them
    if (n4 < n && n4 / ACC_CHUNK == b && tid < (int)(n - n4)) {
      const long j = n4 + tid;
      const unsigned int g = gu[j];
      au[j] = copy ? g : acc_add(au[j], g);
    }
    return;
  }
  const long end = base + ACC_CHUNK < n ? base + ACC_CHUNK : n;
  for (long j = base + tid; j < end; j += ACC_THREADS) {
    const unsigned int g = gu[j];
    au[j] = copy ? g : acc_add(au[j], g);
  }
}

template <int MODE> void acc_launch(bool vec, int blocks, hipStream_t stream, float* acc, const float* grad, long n,
                                    const float* ctl) {
  if (vec)
    hipLaunchKernelGGL((grad_accumulate_kernel<MODE, true>), dim3(blocks), dim3(ACC_THREADS), 0, stream, acc, grad, n, ctl);
  else
    hipLaunchKernelGGL((grad_accumulate_kernel<MODE, false>), dim3(blocks), dim3(ACC_THREADS), 0, stream, acc, grad, n, ctl);
}

}  // namespace

extern "C" {

int kodhip_grad_accumulate(float* acc, const float* grad, long n, int mode, const float* ctl, hipStream_t stream) {
  KOD_CHECK_ARG(n >= 0, "grad_accumulate: negative n");
  KOD_CHECK_ARG(mode >= 0 && mode <= 2, "grad_accumulate: mode %d: expected 0 (add), 1 (copy) or 2 (ctl[0] selects)", mode);
  KOD_CHECK_ARG(mode != 2 || ctl, "grad_accumulate: mode 2 needs ctl");
  KOD_CHECK_ARG(mode != 2 || ((uintptr_t)ctl & 3) == 0, "grad_accumulate: ctl not 4-byte aligned");
  KOD_CHECK_ARG(n == 0 || (acc && grad), "grad_accumulate: null pointer");
  if (n == 0) return KOD_OK;
  const uintptr_t a = (uintptr_t)acc, g = (uintptr_t)grad;
  KOD_CHECK_ARG(((a | g) & 3) == 0, "grad_accumulate: base not 4-byte aligned");
  KOD_CHECK_ARG(n <= (long)(~(uintptr_t)0 >> 3), "grad_accumulate: n too large");
  KOD_CHECK_ARG(!(a < g + (uintptr_t)n * 4 && g < a + (uintptr_t)n * 4), "grad_accumulate: acc overlaps grad");
  if (mode == 2) {
    const uintptr_t c = (uintptr_t)ctl;
    KOD_CHECK_ARG(!(a < c + 16 && c < a + (uintptr_t)n * 4), "grad_accumulate: acc overlaps ctl");
  }
  const long blocks = (n + ACC_CHUNK - 1) / ACC_CHUNK;
  KOD_CHECK_ARG(blocks < (1l << 31), "grad_accumulate: too many elements for one launch");
  const bool vec = ((a | g) & 15) == 0;
  if (mode == 0) acc_launch<0>(vec, (int)blocks, stream, acc, grad, n, ctl);
  else if (mode == 1) acc_launch<1>(vec, (int)blocks, stream, acc, grad, n, ctl);
  else acc_launch<2>(vec, (int)blocks, stream, acc, grad, n, ctl);
  KOD_LAUNCH_CHECK("grad_accumulate");
  return KOD_OK;
}

}  // extern "C"
