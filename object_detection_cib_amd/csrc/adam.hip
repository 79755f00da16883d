// Fused multi-tensor Adam / AdamW (torch.optim.Adam and AdamW, single-tensor non-capturable arithmetic) as ONE launch over the
// engine's flat arenas, in the shape of sgd_nesterov_kernel (csrc/misc_ops.hip): four elements per lane with 16-byte accesses,
// the optimizer group per 64-element granule (0 bias, 1 decay, 2 norm, above 2: padding, skipped), an optional per-element
// keep mask (0 = element of a frozen tensor: no decay, no moments, no update) and an optional clip block consumed between the
// gradient scale and the update exactly as the SGD kernel consumes it.  Reads p, g, exp_avg, exp_avg_sq and writes p, exp_avg,
// exp_avg_sq: 7 x 4 bytes per element.
//
// hyper (device memory, so a replayed hipGraph sees per-step schedules AND per-step bias corrections; KOD_ADAM_HYPER_FLOATS
// floats, kodhip_adam_hyper_floats()):
//   [0..2] nss   = fp32(-(lr / (1 - beta1 ** step)))      [3..5]   beta2                 [6..8]   omb1 = fp32(1 - beta1)
//   [9]    grad_scale (the slot kodhip_grad_norm reads)   [10]     flags: 1 maximize + 2 decoupled weight decay (AdamW)
//   [11]   spare                                          [12..14] omb2 = fp32(1 - beta2)
//   [15..17] bc2s = fp32((1 - beta2 ** step) ** 0.5)      [18..20] eps                   [21..23] wd
//   [24..26] c_decay = fp32(1 - lr * wd)                  [27..31] spare
// every per-group constant formed on the host in doubles as torch forms it, then rounded to fp32; the kernel forms none.
//
// Per element, all fp32, every operation rounded once (the library is built with -ffp-contract=off and the operations are
// spelled out besides, so the order is the source's):
//   gg = g * grad_scale;  [norm: gg = gg * coef | value: clamp with clamp_'s NaN];  maximize: gg = -gg
//   Adam  (wd != 0): gg = fma(p, wd, gg)                 AdamW (wd != 0): p = p * c_decay
//   m = fma(gg - m, omb1, m)                             (torch's lerp_ for a weight < 0.5, i.e. beta1 >= 0.5)
//   v = fma(omb2 * gg, gg, v * beta2)
//   den = sqrt(v) / bc2s + eps
//   p = p + (nss * m) / den
// The square root is sqrtf, the correctly rounded one (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; the division
// `/` behind __fdiv_rn is covered by the same default): HIP's __fsqrt_rn is the hardware's approximate v_sqrt_f32 unless
// OCML_BASIC_ROUNDED_OPERATIONS is defined, and is off by one ulp in about one element of a hundred.
#include "kodhip_common.h"

#define KOD_ADAM_HYPER_FLOATS 32

namespace {

enum { ADAM_CLIP_NONE = -1, ADAM_CLIP_NORM = 0, ADAM_CLIP_VALUE = 1 };      // (0 / 1: the `mode` of kodhip.h, as for SGD)

template <bool MASKED, int CLIP>
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, const unsigned char* gid,
                                                   const unsigned char* keep, long n, const float* hyper, const float* clip) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  const unsigned char grp = gid[i >> 6];
  if (grp > 2) return;
  unsigned char kk[4] = {1, 1, 1, 1};
  if constexpr (MASKED) {
    const uchar4 kv = *reinterpret_cast<const uchar4*>(keep + i);
    kk[0] = kv.x; kk[1] = kv.y; kk[2] = kv.z; kk[3] = kv.w;
    if ((kk[0] | kk[1] | kk[2] | kk[3]) == 0) return;
  }
  const float nss = hyper[grp], beta2 = hyper[3 + grp], omb1 = hyper[6 + grp], gscale = hyper[9];
  const float omb2 = hyper[12 + grp], bc2s = hyper[15 + grp], eps = hyper[18 + grp], wd = hyper[21 + grp];
  const float c_decay = hyper[24 + grp];
  const int flags = (int)hyper[10];
  const bool maximize = (flags & 1) != 0, decoupled = (flags & 2) != 0;
  float coef = 1.f, cv = 0.f;
  if constexpr (CLIP != ADAM_CLIP_NONE) { coef = clip[4]; cv = clip[8]; }
  f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
  f32x4 gv = kod_load_once<f32x4>(g + i);
  f32x4 mv = *reinterpret_cast<const f32x4*>(m + i);
  f32x4 vv = *reinterpret_cast<const f32x4*>(v + i);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (MASKED && !kk[e]) continue;
    float gg = __fmul_rn(gv[e], gscale);
    if constexpr (CLIP == ADAM_CLIP_NORM) gg = __fmul_rn(gg, coef);
    if constexpr (CLIP == ADAM_CLIP_VALUE) gg = gg < -cv ? -cv : (gg > cv ? cv : gg);
    if (maximize) gg = -gg;
    float pe = pv[e];
    if (wd != 0.f) {
      if (decoupled) pe = __fmul_rn(pe, c_decay);
      else gg = __fmaf_rn(pe, wd, gg);
    }
    const float me = __fmaf_rn(__fsub_rn(gg, mv[e]), omb1, mv[e]);
    const float ve = __fmaf_rn(__fmul_rn(omb2, gg), gg, __fmul_rn(vv[e], beta2));
    const float den = __fadd_rn(__fdiv_rn(sqrtf(ve), bc2s), eps);      // (sqrtf, not __fsqrt_rn: see the head of the file)
    mv[e] = me;
    vv[e] = ve;
    pv[e] = __fadd_rn(pe, __fdiv_rn(__fmul_rn(nss, me), den));
  }
  *reinterpret_cast<f32x4*>(p + i) = pv;
  *reinterpret_cast<f32x4*>(m + i) = mv;
  *reinterpret_cast<f32x4*>(v + i) = vv;
}

}  // namespace

extern "C" {

int kodhip_adam_hyper_floats(void) { return KOD_ADAM_HYPER_FLOATS; }

// hyper: DEVICE pointer to the block above; keep_mask (may be NULL: everything trainable): u8 per element; clip (NULL: no
// clipping, clip_mode must then be -1): the clip block of kodhip_grad_norm with clip_mode 0 norm (reads clip[4]) or 1 value
// (clip[8]).  n: a multiple of 64 (whole granules), so no lane's four elements straddle the end.
int kodhip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const void* group_ids,
                     const void* keep_mask, long n, const float* hyper, const float* clip, int clip_mode, hipStream_t stream) {
  KOD_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && group_ids && hyper, "adam_step: null pointer");
  KOD_CHECK_ARG(n > 0 && n % 64 == 0, "adam_step: n %ld is not a positive multiple of 64", n);
  KOD_CHECK_ARG(clip_mode == ADAM_CLIP_NONE || clip_mode == ADAM_CLIP_NORM || clip_mode == ADAM_CLIP_VALUE,
                "adam_step: unknown clip mode %d", clip_mode);
  KOD_CHECK_ARG(clip_mode == ADAM_CLIP_NONE || clip, "adam_step: clip mode %d without a clip block", clip_mode);
  KOD_CHECK_ARG(clip_mode != ADAM_CLIP_NONE || !clip, "adam_step: a clip block without a clip mode");
  KOD_CHECK_ARG(n / 4 / 256 < (1l << 31) - 1, "adam_step: too many elements for one launch");
#define KOD_ADAM(M, CL)                                                                                                     \
  hipLaunchKernelGGL((adam_kernel<M, CL>), dim3(cdiv(n / 4, 256)), dim3(256), 0, stream, params, grads, exp_avg, exp_avg_sq, \
                     (const unsigned char*)group_ids, (const unsigned char*)keep_mask, n, hyper, clip)
#define KOD_ADAM_CLIP(M)                                                                        \
  do {                                                                                          \
    if (clip_mode == ADAM_CLIP_NONE) KOD_ADAM(M, ADAM_CLIP_NONE);                               \
    else if (clip_mode == ADAM_CLIP_NORM) KOD_ADAM(M, ADAM_CLIP_NORM);                          \
    else KOD_ADAM(M, ADAM_CLIP_VALUE);                                                          \
  } while (0)
  if (keep_mask) KOD_ADAM_CLIP(true); else KOD_ADAM_CLIP(false);
#undef KOD_ADAM_CLIP
#undef KOD_ADAM
  KOD_LAUNCH_CHECK("adam_step");
  return KOD_OK;
}

}  // extern "C"
