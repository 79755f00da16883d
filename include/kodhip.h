/* libkodhip - C ABI of the MI355X-native YOLOv5 training hot path for `kod`
 * (craston/object_detection_cib).
 *
 * The reference has no FFI: its seam is Hydra `_target_` instantiation of Python classes
 * (kod/configs/nn/networks/yv5.yaml:1, kod/configs/nn/losses/yv5.yaml:4, kod/configs/assigners/yv5.yaml:6)
 * whose arithmetic is reached through aten / torchvision ops.  Each entry point below replaces the aten
 * op(s) a reference call site asks for; INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer owned by the caller unless marked "host";
 *   - the library never allocates, frees or retains device memory and never synchronises: work is
 *     enqueued on `stream` (pass torch.cuda.current_stream().cuda_stream);
 *   - return 0 = OK, <0 = argument error (nothing launched), >0 = hipError_t; kodhip_last_error() gives
 *     the message (thread local);
 *   - activations are channels-last bf16 [B][H][W][ld]; a tensor may be a channel slice (ld, coff) of a
 *     wider concat buffer - that is how torch.cat (csp.py:109, sppf.py:76, yolov5_pafpn.py:186,199)
 *     disappears; all channel counts / offsets are multiples of 8 (16-byte accesses);
 *   - packed MFMA weight operands (kodhip_pack_weights) have a tap-major K axis with every tap padded to a
 *     multiple of 32 channels: w_packed [N][Kp], k = tap * round_up(Cin, 32) + ci, Kp = KH*KW*round_up(Cin, 32);
 *     w_dgrad [Cin][Kdp], k = tap * round_up(N, 32) + n.  (kodhip_conv_wgrad's Kp is the K extent of its fp32
 *     gradient slabs, k = tap * Cin + ci, Kp = round_up(KH*KW*Cin, 32).)
 */
#ifndef KODHIP_H
#define KODHIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* kodStream_t;

const char* kodhip_last_error(void);
int kodhip_version(void);
int kodhip_device_count(void);

/* ---- layout / packing ------------------------------------------------------------------------- */
/* Lightning batch_to_device + first conv input: NCHW fp32 image -> [B][H][W][4] bf16 (C<=4, zero pad). */
int kodhip_nchw_to_nhwc4(const float* x, void* y, int B, int C, int H, int W, kodStream_t stream);
/* fp32 master weights (state_dict layout [Cout][Cin][KH][KW]) -> bf16 MFMA packs; descs = device array of
 * int64[13] rows {w_off,f_off,d_off,N,Cin,KH,KW,Kp,Kdp,Ntot,n_off,stem,blk_begin}. */
int kodhip_pack_weights(const float* master, void* fpack, void* dpack, const void* descs, int nlayers,
                        long total_blocks, kodStream_t stream);
int kodhip_pack_desc_bytes(void);

/* ---- convolution (aten::convolution / convolution_backward; call sites kod/nn/layers/csp.py:30-46,
 *      kod/nn/layers/sppf.py:29-36,61-67, kod/nn/backbones/yolov5.py:44-52,102-110,
 *      kod/nn/necks/yolov5_pafpn.py:61-73,110-122,152-166) ------------------------------------------ */
int kodhip_conv_stats_slots(long M, int N);
int kodhip_conv_fwd_raw(const void* x, const void* w_packed, void* y, float* stats,
                        int B, int H, int W, int ldx, int xcoff, int Cin,
                        int N, int KH, int KW, int SH, int SW, int PH, int PW, int Kp,
                        int ldy, int ycoff, kodStream_t stream);
/* Eval-mode conv+BN+act unit as ONE launch: out = act(conv(x, w) * scale + shift) (+ residual), scale = gamma *
 * rsqrt(running_var + eps), shift = beta - running_mean * scale given by the caller ([N] floats each, 16-byte aligned).
 * The constants meet the fp32 accumulator (z = fma(S, scale, shift)), act(z) is rounded to bf16 once; with a residual
 * ([B*Ho*Wo][ldr] bf16, channels rcoff .. rcoff + N) the sum of that bf16 value and the residual is rounded again - the
 * same two roundings as kodhip_bn_act_apply.  No pre-BN tensor is written and no statistics are summed.  Geometry, tiles
 * and launch plan are those of kodhip_conv_fwd_raw (kodhip_conv_plan_query op 0).  act / slope as kodhip_bn_act_apply
 * (0 SiLU, 1 ReLU, 2 LeakyReLU(slope), 3 Hardswish, 4 Identity).  `out` ([B*Ho*Wo][ldo], channels ocoff .. ocoff + N)
 * must not overlap `x` or `residual`: a tile is stored while other tiles still read their inputs.  Errors name
 * conv_fwd_fused. */
int kodhip_conv_fwd_fused(const void* x, const void* w_packed, const float* scale, const float* shift,
                          const void* residual /* or NULL */, int ldr, int rcoff, void* out,
                          int B, int H, int W, int ldx, int xcoff, int Cin,
                          int N, int KH, int KW, int SH, int SW, int PH, int PW, int Kp,
                          int ldo, int ocoff, int act, float slope, kodStream_t stream);
/* three biased 1x1 head convs of one level fused (kod/nn/heads/yolov5.py:12-136), out [B][A][H*W][5+nc] fp32.
 * Class-count limit.  This entry point, kodhip_yolo_loss and kodhip_yolo_loss_iou take 5 + nc <= 128 (nc <= 123, the
 * range of their element -> (cell, slot) division) and refuse more with an error status ("at most 123 classes").  The
 * backward pass of the heads, kodhip_head_bwd_prep, additionally needs A * (5 + nc) padded to 8 to be <= 256 (one row
 * of its LDS tile).  The limit of a network that is to be TRAINED is therefore the smaller one:
 *     nc <= min(256 / A, 128) - 5, i.e. 80 classes with the 3 anchors per cell of every shipped configuration
 * (3 * 85 = 255 -> 256 sits exactly on it).  The Python engine refuses a larger class count when it is built
 * (engine/graph.py check_head_limits), before any launch. */
int kodhip_conv_fwd_head(const void* x, const void* w_packed, const float* bias, float* out,
                         int B, int H, int W, int ldx, int xcoff, int Cin, int A, int nc, int Kp,
                         kodStream_t stream);
/* Data gradients (aten::convolution_backward dX).  `accumulate`: bit 0 = add to the bf16 partial already in dx (read-
 * modify-write: rounds the partial and the sum); bits 8.. = fp32 accumulation of an activation gradient with several
 * producers (autograd sums those in fp32 before anything is rounded): 1<<8 first producer - also store the fp32 values
 * to dx_f32, the fp32 shadow of dx (same indexing, row stride ldx floats); 2<<8 later producer - add the shadow's sum
 * in the MFMA accumulators before the single bf16 rounding, store the sum back; 3<<8 last producer - the same without
 * the store; 4<<8 - the partial is dx's own bf16 content left by exact producers (a residual pass-through), added in
 * fp32 before the rounding.  dx_f32 may be NULL for modes 0 and 4. */
int kodhip_conv_dgrad(const void* dy, const void* w_dgrad, void* dx,
                      int B, int H, int W, int ldx, int xcoff, int Cin,
                      int N, int KH, int KW, int SH, int SW, int PH, int PW, int Kp,
                      int ldy, int ycoff, int accumulate, void* dx_f32, kodStream_t stream);
/* dX of a 3x3/s2/p1 conv by output-pixel parity classes (9 instead of 36 taps of MFMA work) */
int kodhip_conv_dgrad_s2(const void* dy, const void* w_dgrad_s2, void* dx,
                         int B, int H, int W, int ldx, int xcoff, int Cin, int N,
                         int ldy, int ycoff, int accumulate, void* dx_f32, kodStream_t stream);
/* Data gradient that also produces the BatchNorm-backward reduction of the conv units whose output gradient it
 * completes (it must be the LAST writer of those channel ranges of dx): fuses aten::convolution_backward (dX) with
 * the reduction half of native_batch_norm_backward + silu_backward of the producing Conv2dNormActivation
 * (kod/nn/layers/csp.py:30-46).  Per segment: partials[2][ch_count][slots] = per-block sums of dz and dz*y. */
typedef struct KodBnRedSeg {
  int ch_begin, ch_count;       /* channel range of dx (relative to xcoff) owned by one producing unit */
  const void* raw; int ldr;     /* that unit's pre-BN output y, bf16 [pixels of dx][ldr] */
  const float* aff;             /* scale[ch_count] | shift[ch_count] */
  float* partials;
} KodBnRedSeg;
int kodhip_conv_dgrad_bnred_slots(int B, int H, int W, int Cin, int N, int KH, int KW, int SH, int SW, int PH, int PW,
                                  int ldy, int stride2 /* 1: the kodhip_conv_dgrad_s2 form */);  /* 0: cannot be fused */
int kodhip_conv_dgrad_bnred(const void* dy, const void* w_dgrad, void* dx,
                            int B, int H, int W, int ldx, int xcoff, int Cin,
                            int N, int KH, int KW, int SH, int SW, int PH, int PW, int Kp,
                            int ldy, int ycoff, int accumulate, void* dx_f32, const void* segments /* host KodBnRedSeg[nseg] */,
                            int nseg, int slots, kodStream_t stream);
int kodhip_conv_dgrad_s2_bnred(const void* dy, const void* w_dgrad_s2, void* dx,
                               int B, int H, int W, int ldx, int xcoff, int Cin, int N,
                               int ldy, int ycoff, int accumulate, void* dx_f32, const void* segments, int nseg, int slots,
                               kodStream_t stream);
/* The same data gradient "folded": one stride-1 gather over the 2x2 dY neighbourhood of each 2x2 output-pixel block,
 * 4 parity classes x Cin output columns, depth-to-space epilogue (16 tap-class products instead of 9, but dY is staged
 * once and both x parities of a pixel pair are stored together: faster for the shallow, staging-bound layers).
 * w_fold: [4*Cin][4*round_up(N,32)] (pack mode 3).  kodhip_conv_dgrad_s2_folded: which form to pack / call (1 = folded). */
int kodhip_conv_dgrad_s2_folded(int Cin, int N);
int kodhip_conv_dgrad_s2f(const void* dy, const void* w_fold, void* dx,
                          int B, int H, int W, int ldx, int xcoff, int Cin, int N,
                          int ldy, int ycoff, int accumulate, void* dx_f32, kodStream_t stream);
int kodhip_conv_dgrad_s2f_bnred_slots(int B, int H, int W, int Cin, int N, int ldy);
int kodhip_conv_dgrad_s2f_bnred(const void* dy, const void* w_fold, void* dx,
                                int B, int H, int W, int ldx, int xcoff, int Cin, int N,
                                int ldy, int ycoff, int accumulate, void* dx_f32, const void* segments, int nseg, int slots,
                                kodStream_t stream);
/* dX of TWO pointwise (1x1/s1/p0) convs that read the same tensor - a CSP layer's main_conv and short_conv
 * (kod/nn/layers/csp.py:96-111) - as one launch over the concatenated reduction: dx is written once instead of written
 * and then accumulated into by a second launch.  dy1 / dy2: [B*H*W][ldy] (+ycoff, N channels each), w1 / w2: their
 * dgrad packs [Cin][Kp], Kp = round_up(N, 32). */
int kodhip_conv_dgrad_dual(const void* dy1, const void* w1, const void* dy2, const void* w2, void* dx,
                           int B, int H, int W, int ldx, int xcoff, int Cin, int N, int Kp, int ldy, int ycoff,
                           int accumulate, void* dx_f32, kodStream_t stream);
int kodhip_conv_dgrad_dual_bnred_slots(int B, int H, int W, int Cin, int N, int ldy);
int kodhip_conv_dgrad_dual_bnred(const void* dy1, const void* w1, const void* dy2, const void* w2, void* dx,
                                 int B, int H, int W, int ldx, int xcoff, int Cin, int N, int Kp, int ldy, int ycoff,
                                 int accumulate, void* dx_f32, const void* segments, int nseg, int slots, kodStream_t stream);
/* Read-only launch plan of a convolution (nothing is launched, no pointer is read): which tile shape and kernel form a
 * geometry reaches.  The geometry is given as the entry point named by `op` takes it: 0 kodhip_conv_fwd_raw, 1 kodhip_conv_dgrad,
 * 2 kodhip_conv_dgrad_s2, 3 kodhip_conv_dgrad_s2f, 4 kodhip_conv_dgrad_dual (ops 2..4 ignore KH .. PW; ops 2, 3 ignore Kp).
 * out (host, 8 ints) = {bm, bn (pixels x channels of a block's tile), row3 (1: the 3x3 / stride-1 row form), fast (1: LDS-DMA
 * path), tiles_m, tiles_n, groups_m (persistent blocks per channel tile: a block loops over tiles_m / groups_m pixel tiles),
 * bm of the merged four-class launch of op 2, 0 when the launch is not merged}. */
int kodhip_conv_plan_query(int op, int B, int H, int W, int ldx, int xcoff, int Cin,
                           int N, int KH, int KW, int SH, int SW, int PH, int PW, int Kp,
                           int ldy, int ycoff, int* out);
/* Slab count of the kernel kodhip_conv_wgrad picks for this geometry (3x3 / stride 1 / pad 1 layers with whole
 * 32-channel chunks take a form that stages dY once per block and every input row once per kernel row): size the slab
 * region with this one.  H, W: input dims; ldx / ldy: row strides of x / dy in elements. */
int kodhip_conv_wgrad_splits_geo(int B, int H, int W, int ldx, int Cin, int N, int KH, int KW, int SH, int SW, int PH, int PW,
                                 int Kp, int ldy);
/* grad: fp32 [n_valid][Cin][KH][KW] = scale * dW of the first n_valid output channels (the state_dict layout; stem = 1:
 * [n_valid][3][6][6] from the pixel-pair K axis).  n_valid < N (dy padded with columns that are no weights, e.g. the heads'
 * Npad): exactly n_valid * Cin * KH * KW floats are written, nothing behind them; the partial slabs always hold all N rows. */
int kodhip_conv_wgrad(const void* x, const void* dy, float* partials, float* grad,
                      int B, int H, int W, int ldx, int xcoff, int Cin,
                      int N, int KH, int KW, int SH, int SW, int PH, int PW, int Kp,
                      int ldy, int ycoff, int n_valid, int stem, float scale, kodStream_t stream);
/* Read-only launch plan of kodhip_conv_wgrad (dual = 0) / kodhip_conv_wgrad_dual (dual = 1; KH .. PW ignored).
 * out (host, 8 ints) = {tn, tk (output rows x K columns of a block's tile; ROW3 form: 32 wn rn rows x 32 wc channels of all nine
 * taps), row3, wn, rn, wc (the ROW3 form's wave layout, 0 otherwise), splits, dma (1: LDS-DMA kernel, 0: register-staged)}. */
int kodhip_conv_wgrad_plan_query(int B, int H, int W, int ldx, int Cin, int N, int KH, int KW, int SH, int SW, int PH, int PW,
                                 int Kp, int ldy, int dual, int* out);
/* Weight gradients of TWO pointwise layers with the same input (a CSP layer's main_conv and short_conv,
 * kod/nn/layers/csp.py:85-99) in one launch + one reduction: the shared input is streamed from HBM once.  dy1 / dy2:
 * [B*H*W][ldy] (+ycoff, N channels each); partials: kodhip_conv_wgrad_dual_splits(...) * 2N * Kp floats; grad1 / grad2: fp32
 * [N][Cin].  kodhip_conv_wgrad_dual_splits returns 0 where the form does not apply (then: two kodhip_conv_wgrad launches). */
int kodhip_conv_wgrad_dual_splits(int B, int H, int W, int ldx, int Cin, int N, int Kp, int ldy);
int kodhip_conv_wgrad_dual(const void* x, const void* dy1, const void* dy2, float* partials, float* grad1, float* grad2,
                           int B, int H, int W, int ldx, int xcoff, int Cin, int N, int Kp, int ldy, int ycoff,
                           float scale, kodStream_t stream);
/* The stem's whole backward in one kernel + the slab reduction: dY = k1 * dA * silu'(y * scale + shift) + k2 * y + k3 is
 * formed on the fly and multiplied into dW; dY is never written (the stem - kod/nn/backbones/yolov5.py:44-52, 6x6 / stride 2
 * / pad 2 on the image - has no data gradient, so the weight gradient is dY's only reader).  Replaces
 * kodhip_bn_silu_bwd_apply + kodhip_conv_wgrad(stem = 1) for that unit.  x: pixel pairs [B][H][Wp][8] bf16 (Wp = width / 2);
 * dA: [B * H/2 * Wp][lda] (+dacoff), y: [..][ldy] pre-BatchNorm output (left untouched); coef = k1[N] | k2[N] | k3[N] from
 * kodhip_bn_bwd_coeffs*; partials: kodhip_stem_bwd_fused_blocks(B, H, Wp, N) * (N <= 32 ? 32 : 64) * 160 floats; grad: fp32
 * [N][3][6][6].  N <= 64 (two 32-channel tiles per block above 32). */
int kodhip_stem_bwd_fused_blocks(int B, int H, int Wp, int N);
int kodhip_stem_bwd_fused(const void* x, const void* dA, int lda, int dacoff, const void* y, int ldy,
                          const float* scale, const float* shift, const float* coef, float* partials, float* grad,
                          int B, int H, int Wp, int N, float gscale, kodStream_t stream);

/* ---- BatchNorm2d(eps 1e-3, momentum .03) + SiLU (kod/nn/networks/yolov5.py:24,
 *      kod/nn/layers/activations.py:7; aten::native_batch_norm(+backward), silu(+backward)) ---------- */
int kodhip_bn_reduce_partials(const float* partials, double* sums, int C, int T, kodStream_t stream);
int kodhip_bn_finalize(const double* sums, double count, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, float momentum, float eps,
                       float* scale, float* shift, float* mean, float* rstd, int C, int update_running,
                       kodStream_t stream);
/* single-GPU forms: partial slabs -> constants in one launch (no cross-rank all-reduce in between) */
int kodhip_bn_finalize_partials(const float* partials, int T, double count, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, float momentum, float eps,
                                float* scale, float* shift, float* mean, float* rstd, int C, int update_running,
                                kodStream_t stream);
/* SyncBN forms of the two single launches: the rank's sums are exchanged through the peer buffers (kodhip_peer_*, below)
 * inside the kernel.  count = pixels of ALL ranks; view = host KodPeerView (copied into the launch); slot = first granule
 * of this exchange (it uses 4 * C).  Parameter gradients (dgamma, dbeta) keep the rank's own sums. */
int kodhip_bn_finalize_partials_peer(const float* partials, int T, double count, const float* gamma, const float* beta,
                                     float* running_mean, float* running_var, float momentum, float eps,
                                     float* scale, float* shift, float* mean, float* rstd, int C, int update_running,
                                     const void* view, unsigned int slot, kodStream_t stream);
int kodhip_bn_bwd_coeffs_partials_peer(const float* partials, int T, double count, const float* gamma, const float* mean,
                                       const float* rstd, float* dgamma, float* dbeta, float* coef, int C,
                                       int raw_moment, const void* view, unsigned int slot, kodStream_t stream);
/* kodhip_bn_bwd_coeffs_partials for two units in one launch (a CSP layer's short_conv + main_conv) */
int kodhip_bn_bwd_coeffs_partials2(const float* partials0, int T0, double count0, const float* gamma0, const float* mean0,
                                   const float* rstd0, float* dgamma0, float* dbeta0, float* coef0, int C0, int raw_moment0,
                                   const float* partials1, int T1, double count1, const float* gamma1, const float* mean1,
                                   const float* rstd1, float* dgamma1, float* dbeta1, float* coef1, int C1, int raw_moment1,
                                   kodStream_t stream);
int kodhip_bn_bwd_coeffs_partials(const float* partials, int T, double count, const float* gamma, const float* mean,
                                  const float* rstd, float* dgamma, float* dbeta, float* coef, int C,
                                  int raw_moment /* 1: partials[1] = sum dz*y (kodhip_conv_dgrad_bnred) */,
                                  kodStream_t stream);
/* eval-mode BatchNorm inside a training network (the module's training flag is off): mean / rstd hold the running
 * statistics' constants (kodhip_bn_eval_constants); dgamma / dbeta are reduced as above, coef = (gamma*rstd, 0, 0) - the
 * plain eval-mode data gradient; no cross-rank exchange.  The two-unit form takes a mode per job (eval_k = 0: the
 * train-mode coefficients of kodhip_bn_bwd_coeffs_partials2, count_k is then required). */
int kodhip_bn_bwd_coeffs_eval_partials(const float* partials, int T, const float* gamma, const float* mean,
                                       const float* rstd, float* dgamma, float* dbeta, float* coef, int C,
                                       int raw_moment, kodStream_t stream);
int kodhip_bn_bwd_coeffs_eval_partials2(const float* partials0, int T0, double count0, const float* gamma0,
                                        const float* mean0, const float* rstd0, float* dgamma0, float* dbeta0,
                                        float* coef0, int C0, int raw_moment0, int eval0,
                                        const float* partials1, int T1, double count1, const float* gamma1,
                                        const float* mean1, const float* rstd1, float* dgamma1, float* dbeta1,
                                        float* coef1, int C1, int raw_moment1, int eval1, kodStream_t stream);
/* eval-mode constants of n_units units in one launch.  desc: DEVICE table of n_units descriptors of
 * kodhip_bn_eval_desc_bytes() bytes each: {gamma, beta, running_mean, running_var, aff, coef (or null), C, 0} as 64-bit
 * words.  Writes aff = scale | shift | mean | rstd (C floats each) from the running statistics, and with coef the
 * eval-mode backward coefficients (gamma*rstd, 0, 0); no running statistic is written. */
int kodhip_bn_eval_constants(const void* desc, int n_units, float eps, kodStream_t stream);
int kodhip_bn_eval_desc_bytes(void);
int kodhip_bn_silu_apply(const void* y, int ldy /* row stride of y (>= C: y may be a channel slice) */, const float* scale, const float* shift,
                         const void* residual, int ldr, int rcoff,
                         void* out, int ldo, int ocoff, long M, int C, kodStream_t stream);
int kodhip_bn_bwd_slots(long M, int C);
int kodhip_bn_silu_bwd_reduce(const void* dA, int lda, int dacoff, const void* y, int ldy, const float* scale,
                              const float* shift, const float* mean, const float* rstd, float* partials,
                              long M, int C, kodStream_t stream);
int kodhip_bn_bwd_coeffs(const double* sums_local, const double* sums_global, double count, const float* gamma,
                         const float* mean, const float* rstd, float* dgamma, float* dbeta, float* coef, int C,
                         int raw_moment, kodStream_t stream);
int kodhip_bn_silu_bwd_apply(const void* dA, int lda, int dacoff, void* y_inout, int ldy, const float* scale,
                             const float* shift, const float* coef, void* dI, int ldi, int dicoff, int di_accum,
                             long M, int C, kodStream_t stream);

/* The same three elementwise passes for the other activations the reference's layer signatures admit
 * (kod/nn/layers/csp.py:16-46: `activation_layer: Callable[..., nn.Module]`; its configs use SiLUInplace only):
 * act = 0 SiLU (the entries above are this with act = 0), 1 ReLU, 2 LeakyReLU(slope), 3 Hardswish, 4 identity (activation_layer=None);
 * torch's conventions at the kinks.  One set of kernels, the activation a template parameter; a network built with a
 * non-SiLU one runs the BatchNorm-backward reduction as its own pass. */
int kodhip_bn_act_apply(const void* y, int ldy, const float* scale, const float* shift, const void* residual, int ldr, int rcoff,
                        void* out, int ldo, int ocoff, long M, int C, int act, float slope, kodStream_t stream);
int kodhip_bn_act_bwd_apply(const void* dA, int lda, int dacoff, void* y_inout, int ldy, const float* scale, const float* shift,
                            const float* coef, void* dI, int ldi, int dicoff, int di_accum, long M, int C, int act, float slope,
                            kodStream_t stream);
int kodhip_bn_act_bwd_reduce(const void* dA, int lda, int dacoff, const void* y, int ldy, const float* scale, const float* shift,
                             const float* mean, const float* rstd, float* partials, long M, int C, int act, float slope,
                             kodStream_t stream);

/* ---- SPPF max-pool, nearest upsample (kod/nn/layers/sppf.py:46-50,73-76,
 *      kod/nn/necks/yolov5_pafpn.py:144-146,182-184) ------------------------------------------------- */
/* idx: [B][H][W][C] bytes, the winning tap of every output (an opaque code: written by _fwd, read by _bwd of the same
 * library); argmax as torch's scan: first maximum in row-major window order, a NaN beats every number */
int kodhip_maxpool5_fwd(const void* x, int ldx, int xcoff, void* y, int ldy, int ycoff, void* idx,
                        int B, int H, int W, int C, kodStream_t stream);
/* dx_f32 (NULL = none): fp32 shadow of dx holding the earlier producers' partial sum (see kodhip_conv_dgrad) */
int kodhip_maxpool5_bwd(const void* dy, int ldy, int ycoff, const void* idx, void* dx, int ldx, int xcoff,
                        int B, int H, int W, int C, const float* dx_f32, kodStream_t stream);
/* any odd window K <= 15 (SPPFBottleneck's kernel_sizes, sppf.py:27-67): K = 5 dispatches to the kernels above */
int kodhip_maxpool_fwd(const void* x, int ldx, int xcoff, void* y, int ldy, int ycoff, void* idx,
                       int B, int H, int W, int C, int K, kodStream_t stream);
int kodhip_maxpool_bwd(const void* dy, int ldy, int ycoff, const void* idx, void* dx, int ldx, int xcoff,
                       int B, int H, int W, int C, int K, const float* dx_f32, kodStream_t stream);
int kodhip_upsample2x_fwd(const void* x, int ldx, int xcoff, void* y, int ldy, int ycoff,
                          int B, int H, int W, int C, kodStream_t stream);
int kodhip_upsample2x_bwd(const void* dy, int ldy, int ycoff, void* dx, int ldx, int xcoff, int accumulate,
                          int B, int H, int W, int C, const float* dx_f32, kodStream_t stream);
/* workspace: 2048 * Npad floats (per-block bias partials).  Npad = A * (5 + nc) padded to 8, at most 256 (see the
 * class-count limit at kodhip_conv_fwd_head); anything else is refused with "head_bwd_prep: bad Npad" */
int kodhip_head_bwd_prep(const float* g, void* dy, float* workspace, float* db_box, float* db_obj, float* db_cls,
                         int B, int HW, int A, int nc, int Npad, kodStream_t stream);

/* ---- optimizer (torch.optim.SGD as grouped by kod/nn/optim/smart.py:36-58) ---------------------- */
int kodhip_sgd_nesterov(float* params, const float* grads, float* momentum_buf, const void* group_ids,
                        long n, const float* hyper /* device, 12 floats: lr[3] momentum[3] wd[3] grad_scale,
                                                      flags = nesterov (smart_sgd.yaml: 1) + 2 maximize + 4 first step
                                                      (only read when dampening != 0), dampening */,
                        kodStream_t stream);
/* kodhip_sgd_nesterov over the elements whose keep_mask byte (device, n bytes) is non-zero; the others (frozen tensors,
   engine/freeze.py) are not touched: no weight decay, no momentum, no update */
int kodhip_sgd_nesterov_masked(float* params, const float* grads, float* momentum_buf, const void* group_ids,
                               const void* keep_mask, long n, const float* hyper, kodStream_t stream);
/* ---- gradient norm and clipping over the gradient arena (torch.nn.utils.clip_grad_norm_ / clip_grad_value_, Lightning's
 * Trainer(gradient_clip_val, gradient_clip_algorithm)) ----
 * clip block: device memory, kodhip_clip_block_bytes() = 16 fp32:
 *   [0] total 2-norm of grad_scale * g over the counted elements   [1] bias group  [2] decay group  [3] norm group
 *   [4] clip coefficient min(1, max_norm / (total + 1e-6)), formed in fp32 as torch forms it
 *   [5] 1.0 when the total norm is NaN or Inf, else 0.0            [6] steps skipped so far (skip_nonfinite)   [7] spare
 *   [8] INPUT: max_norm (mode 0, norm) or the clamp value (mode 1, value); written by the caller, may change between
 *       replays of a captured step like `hyper`                    [9..15] spare
 * [0..6] are written by kodhip_grad_norm only.  Sums of squares are formed in fp64 and reduced in a fixed order (one partial
 * per block and group, no atomics): the same bits on every run and replay, whatever the device. */
int kodhip_clip_block_bytes(void);
int kodhip_grad_norm_workspace_bytes(void);
/* count_mask (device, n bytes, may be NULL = every element of groups 0..2 counts): 0 leaves the element out (arena
   padding, frozen tensors).  workspace: kodhip_grad_norm_workspace_bytes(), 8-byte aligned.  skip_nonfinite: a NaN / Inf
   total bumps clip[6].  nontemporal: gradient loads that do not allocate in the caches.  Two launches. */
int kodhip_grad_norm(const float* grads, const void* group_ids, const void* count_mask, long n, const float* hyper,
                     float* clip, void* workspace, int skip_nonfinite, int nontemporal, kodStream_t stream);
/* kodhip_sgd_nesterov (keep_mask NULL) / kodhip_sgd_nesterov_masked with the gradient clipped after the scale:
   mode 0: (g * grad_scale) * clip[4]; mode 1: clamp(g * grad_scale, -clip[8], +clip[8]) (a NaN stays a NaN).  clip[4] == 1
   gives the bits of the unclipped entries.  skip_nonfinite and clip[5] != 0: nothing is written. */
int kodhip_sgd_nesterov_clipped(float* params, const float* grads, float* momentum_buf, const void* group_ids,
                                const void* keep_mask, long n, const float* hyper, const float* clip, int mode,
                                int skip_nonfinite, kodStream_t stream);
/* the gradients themselves, in place, over the counted elements: mode 0 g *= clip[4], mode 1 g = clamp(g, -clip[8], +clip[8]) */
int kodhip_grad_clip_inplace(float* grads, const void* group_ids, const void* count_mask, long n, const float* clip,
                             int mode, kodStream_t stream);
/* ---- Adam / AdamW (torch.optim.Adam, torch.optim.AdamW; single-tensor, non-capturable arithmetic) as one launch over the
 * arenas, csrc/adam.hip.  hyper: device, kodhip_adam_hyper_floats() = 32 fp32, every per-group constant (3 groups: bias,
 * decay, norm) formed by the caller in double as torch forms it and then rounded to fp32:
 *   [0..2] nss = -(lr / (1 - beta1 ** step))   [3..5] beta2   [6..8] omb1 = 1 - beta1   [9] grad_scale (where
 *   kodhip_grad_norm reads it)   [10] flags = 1 maximize + 2 decoupled weight decay (AdamW)   [11] spare
 *   [12..14] omb2 = 1 - beta2   [15..17] bc2s = (1 - beta2 ** step) ** 0.5   [18..20] eps   [21..23] wd
 *   [24..26] c_decay = 1 - lr * wd   [27..31] spare
 * `step` is the caller's count: the block is rewritten before every step, also before every replay of a captured one.
 * Per element, fp32, each operation rounded once:  gg = g * grad_scale; [clip]; maximize: gg = -gg;
 *   Adam, wd != 0: gg = fma(p, wd, gg);  AdamW, wd != 0: p = p * c_decay;  m = fma(gg - m, omb1, m)  (torch's lerp_ for
 *   beta1 >= 0.5);  v = fma(omb2 * gg, gg, v * beta2);  p = p + (nss * m) / (sqrt(v) / bc2s + eps).
 * keep_mask (device, n bytes, may be NULL): 0 = element of a frozen tensor, untouched.  clip (may be NULL) with clip_mode
 * 0: (g * grad_scale) * clip[4]; 1: clamp(g * grad_scale, -clip[8], +clip[8]) (a NaN stays a NaN); clip NULL needs
 * clip_mode -1.  Refused before any launch (< 0, the text names adam_step): a NULL pointer, n <= 0 or n % 64 != 0, a clip
 * mode without a clip block or the reverse, an unknown clip mode. */
int kodhip_adam_hyper_floats(void);
int kodhip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const void* group_ids,
                     const void* keep_mask, long n, const float* hyper, const float* clip, int clip_mode, kodStream_t stream);
/* ---- weight EMA (YOLOv5 ModelEMA: `v *= d; v += (1 - d) * msd[k]`), beside the step, never inside it ----------------
 * Up to 4 segments per launch; model_ptrs / shadow_ptrs / numels are HOST arrays of nseg entries (device pointers, element
 * counts) that travel by value in the kernel arguments.  Per element, fp32, every operation rounded on its own:
 *   shadow = fl( fl(shadow * d) + fl(omd * model) )
 * with omd = float32(1.0 - d) formed in double by the caller (float32(1 - d) != 1 - float32(d)).  NaN, Inf and subnormals
 * as IEEE fp32.  Bases 16-byte aligned: 16-byte accesses; any 4-byte aligned base and any numel >= 0 are correct; nothing
 * at or beyond numel is touched; a segment with numel 0 is skipped (its pointers may be NULL).  Refused (< 0, nothing
 * launched): nseg outside 1..4, a NULL table, a negative numel, a NULL or misaligned pointer with numel > 0, a model segment
 * that overlaps a shadow segment, two written segments that overlap. */
int kodhip_ema_update(const float* const* model_ptrs, float* const* shadow_ptrs, const long* numels, int nseg, float d, float omd,
                      kodStream_t stream);
/* exchanges the contents of the paired segments (numels in 32-bit words: a pure copy, NaN payloads included, so an int64
 * buffer goes as two words per value); the same tables, rules and refusals as kodhip_ema_update */
int kodhip_ema_swap(void* const* a_ptrs, void* const* b_ptrs, const long* numels, int nseg, kodStream_t stream);
/* ---- gradient accumulation (Lightning's accumulate_grad_batches; autograd's `.grad += g`), csrc/accumulate.hip ----
 * acc <- grad (mode 1: a copy of 32-bit words) or acc <- fl(acc + grad) (mode 0, __fadd_rn, one rounding);
 * mode 2: ctl[0] != 0 selects the copy, else the add - the form a captured graph holds, ctl written by the caller
 * outside the graph like `hyper`.  ctl: device, 4 fp32 (16 bytes), only read in mode 2.  NaN, Inf and subnormals as IEEE
 * fp32.  Bases 16-byte aligned: 16-byte accesses; any 4-byte aligned bases and any n >= 0 are correct; nothing at or beyond
 * n is touched; n == 0 launches nothing.  Refused (< 0, nothing launched, the text names grad_accumulate): a NULL pointer
 * with n > 0, negative n, a base that is not 4-byte aligned, an unknown mode, mode 2 with NULL ctl, acc overlapping grad
 * (or ctl). */
int kodhip_grad_accumulate(float* acc, const float* grad, long n, int mode, const float* ctl, kodStream_t stream);
int kodhip_fill_u32(void* p, uint32_t value, long n, kodStream_t stream);
/* dst (device) <- src (PINNED host memory), bytes % 16 == 0, both 16-byte aligned: a kernel pulling the bytes through the
 * host memory's device mapping - the small per-step tables of the data path (kod/data/detection.py's per-sample results)
 * without an async-copy hand-over on the step's stream; hipMemcpyAsync when the memory has no device mapping */
int kodhip_pull_from_host(void* dst, const void* src_pinned, long bytes, kodStream_t stream);
/* debug: *dst = the device's constant-rate wall clock (100 MHz), stream-ordered - time stamps inside a replayed hipGraph */
int kodhip_debug_stamp(unsigned long long* dst, kodStream_t stream);

/* ---- target assignment + loss (kod/core/label_assignment/yv5.py:45-319,
 *      kod/lightning/experiments/yv5_baseline/loss.py:65-248, kod/core/bbox/iou.py:200-246) ---------- */
typedef struct KodAssignLevel {
  int* idx; int* label; float* gt; float* anc; int* count;
  float anchor_w[3], anchor_h[3];
  int stride;
} KodAssignLevel;
int kodhip_assign_targets(const double* boxes, const long* labels, const int* samples, int n, int cap,
                          int img_w, int img_h, float threshold, const KodAssignLevel* levels /* host[3] */,
                          kodStream_t stream);
typedef struct KodLossLevel {
  const float* logits; float* grad;
  const int* idx; const int* label; const float* gt; const float* anc; const int* count;
  int* cellmaps; int* rowprev; float* rowgrad; float* tobj;
  int fh, fw;
  float balance;
} KodLossLevel;
/* out: 16 floats - [0..2] localization / objectness / classification, [3..11] per-level raw means, [12] (with upstream)
 * upstream[0] * ((loc + cls) + obj): the training-step scalar of exp.py:104-121 when the three upstreams are one scale */
int kodhip_yolo_loss(const KodLossLevel* levels /* host[3] */, int B, int A, int nc, int cap,
                     float lam_box, float lam_obj, float lam_cls, const float* pos_weight,
                     const float* upstream, float* partials, int nslots, float* out, int compute_grad,
                     kodStream_t stream);

/* the same with the loss's IoUCalculator (loss.py:46-63,96): iou_kind 0 iou | 1 giou | 2 diou | 3 ciou (iou.py:9-14) and its eps;
 * (3, 1e-7f) is what kodhip_yolo_loss runs */
int kodhip_yolo_loss_iou(const KodLossLevel* levels /* host[3] */, int B, int A, int nc, int cap,
                         float lam_box, float lam_obj, float lam_cls, const float* pos_weight,
                         const float* upstream, float* partials, int nslots, float* out, int compute_grad,
                         int iou_kind, float iou_eps, kodStream_t stream);

/* the same with YOLOv5's loss hyper-parameters (hyp.*.yaml fl_gamma / obj_pw, train.py --label-smoothing; cls_pw is pos_weight):
 * FocalLoss(gamma, alpha) around both BCE terms (fl_gamma 0 = off, else >= 1), class targets cls_pos at the row's label and
 * cls_neg elsewhere (smooth_BCE: 1 - eps / 2, eps / 2), a pos_weight on the objectness BCE.  The objectness target stays
 * clamp(iou, 0), not detached: under focal its gradient depends on the cell's surviving (last row's) target.
 * opt is a host pointer; NULL or neutral (0, any alpha, 1, 0, 1) runs exactly kodhip_yolo_loss_iou - the same kernels, the same bits.
 * Refused with a status and a message, nothing launched: fl_gamma < 0 or in (0, 1) or not finite, fl_alpha outside (0, 1),
 * cls_pos outside (0.5, 1], cls_neg outside [0, 0.5), obj_pos_weight <= 0 or not finite.  Same launches as the default path. */
typedef struct KodLossOptions { float fl_gamma, fl_alpha, cls_pos, cls_neg, obj_pos_weight; } KodLossOptions;
int kodhip_yolo_loss_ex(const KodLossLevel* levels /* host[3] */, int B, int A, int nc, int cap,
                        float lam_box, float lam_obj, float lam_cls, const float* pos_weight,
                        const float* upstream, float* partials, int nslots, float* out, int compute_grad,
                        int iou_kind, float iou_eps, const KodLossOptions* opt /* host, or NULL */, kodStream_t stream);

/* Aligned IoU family behind kod.core.bbox.iou.IoUCalculator.__call__ (kod/core/bbox/iou.py:77-95,142-268):
 * boxes [m][4] xyxy fp32 -> out [m]; kind 0 iou | 1 giou | 2 diou | 3 ciou (IoUType order, iou.py:9-14).
 * The backward follows autograd's conventions (max/min ties split evenly, clamp(0) passes at 0, CIoU alpha constant). */
int kodhip_iou_fwd(const float* boxes1, const float* boxes2, float* out, long m, int kind, float eps,
                   kodStream_t stream);
int kodhip_iou_bwd(const float* boxes1, const float* boxes2, const float* grad_out, float* grad_boxes1 /* or NULL */,
                   float* grad_boxes2 /* or NULL */, long m, int kind, float eps, kodStream_t stream);

/* ---- device data path: mosaic + warpAffine + HSV + flip + /255 (+ mixup) in one gather kernel
 *      (kod/data/mosaic.py:58-132, kod/data/augmentations/default.py:279-320,354-408,433-438) ------- */
int kodhip_compose_desc_bytes(void);
int kodhip_compose_batch(const void* pool, const void* descs, const float* mix, const void* bilinear_tab,
                         float* out_f32, void* out_pairs, int B, int S, kodStream_t stream);
/* image_color_transforms (kod/data/augmentations/default.py:420-432,460-461; the reference's shipped default,
 * kod/configs/data/augmentations/aug_params.yaml:15): the albumentations stage between warp and HSV for ONE sample whose
 * gate fired - descriptor `entry` (2 * sample + slot of descs [B][2]) is warped into out_u8 [S][S][3] and the fired
 * transforms run on it in Compose order: ops bit 0 Blur(blur_k in 3/5/7), 1 MedianBlur(median_k), 2 ToGray, 3 CLAHE(clahe_clip
 * in [1, 4], 8 x 8 tiles, on the L channel of an 8-bit Lab image).  tmp_u8: S*S*3 bytes, luts_u8: 64*256 bytes, color_tab: the
 * Lab tables (data/device_pipeline.color_table()).  The descriptor's `pre` field must hold out_u8 when descs is uploaded:
 * kodhip_compose_batch (same stream, afterwards) then takes that sample's warped pixels from there. */
int kodhip_compose_color(const void* pool, const void* descs, const void* bilinear_tab, const void* color_tab, int entry,
                         int ops, int blur_k, int median_k, double clahe_clip, void* out_u8, void* tmp_u8, void* luts_u8,
                         int S, kodStream_t stream);

/* ---- validation pre-processing: SampleReader (LongestMaxSize + PadIfNeeded(114), kod/data/sample_reader.py:16-40,
 *      102-136) + ValidationSampleAugmentor (ToFloat(255) + CHW, kod/data/augmentations/albu.py:91-119) ------------ */
int kodhip_val_prep_desc_bytes(void);
/* kodhip_letterbox_batch: B records of kodhip_val_prep_desc_bytes() bytes (data/device_pipeline.py VAL_DESC) letterboxed onto an
 * H x W canvas - OpenCV's fixed-point INTER_LINEAR, padding 114, / 255.f, a copy path when nothing is resized.  A record's top /
 * left are PadIfNeeded's centre position on that canvas (engine/tiles.py letterbox_geometry; nh <= H and nw <= W are the
 * caller's to hold).  out_f32 [B,3,H,W] (8-byte aligned) and / or out_pairs bf16 [B,H,W/2,8] (16-byte aligned), W even,
 * B <= 65535; the network takes multiples of 32.  One thread per pixel pair; every tap is one 4-byte load, so the pool must
 * stay readable 1 byte behind its last image (ImagePool leaves 8).
 * kodhip_val_prep_batch is kodhip_letterbox_batch with H = W = S: the same kernel under the same contract (since version 114:
 * the readable byte behind the pool, the two alignments, B <= 65535, checked before the launch with errors that name
 * val_prep_batch; before, it ran a kernel of its own that needed none of them). */
int kodhip_val_prep_batch(const void* pool, const void* descs /* device [B] */, float* out_f32 /* or NULL */,
                          void* out_pairs /* or NULL */, int B, int S, kodStream_t stream);
int kodhip_letterbox_batch(const void* pool, const void* descs /* device [B] */, float* out_f32 /* or NULL */,
                           void* out_pairs /* or NULL */, int B, int H, int W, kodStream_t stream);
/* kodhip_letterbox_frames: kodhip_letterbox_batch for video frames that are read WHERE THEY LIE (csrc/video.hip): no pool, no
 * intermediate RGB image.  descs: device [B] records of kodhip_frame_desc_bytes() bytes (data/frames.py FRAME_DESC): three
 * plane addresses (64-bit device addresses), pitch of plane 0 and of planes 1 / 2 in bytes (any value >= the row's bytes),
 * format (0 RGB24, 1 BGR24: packed, 3 B / pixel; 2 NV12: Y plane + interleaved UV plane; 3 I420: Y, U, V planes; 4:2:0 frames
 * have even h and w), then h, w, nh, nw, top, left, scale_x, scale_y as in kodhip_letterbox_batch's records, then six ints
 * yoff, CY, CVR, CVG, CUG, CUB: OpenCV's 20-bit fixed-point 4:2:0 conversion, y = max(0, Y - yoff) * CY + 2^19,
 * R = sat8((y + CVR (V-128)) >> 20), G = sat8((y + CVG (V-128) + CUG (U-128)) >> 20), B = sat8((y + CUB (U-128)) >> 20), chroma
 * sample (r >> 1, c >> 1) for pixel (r, c).  Every bilinear tap is converted to u8 RGB first, so both outputs equal, bit for
 * bit, kodhip_letterbox_batch's on the RGB image the conversion of the whole frame gives.  Only bytes inside a frame's rows are
 * read (byte / 2-byte loads; nothing depends on the alignment of an address or a pitch).  B <= 65535, W even, H * W <= 2^30,
 * out_f32 8-byte and out_pairs 16-byte aligned; the arguments are checked before the launch. */
int kodhip_frame_desc_bytes(void);
int kodhip_letterbox_frames(const void* descs /* device [B] */, float* out_f32 /* [B,3,H,W] or NULL */,
                            void* out_pairs /* bf16 [B,H,W/2,8] or NULL */, int B, int H, int W, kodStream_t stream);

/* ---- second-stage crops (csrc/crops.hip; YOLOv5 utils/general.py apply_classifier, utils/plots.py save_one_box): the pixels
 *      inside N detection boxes, cut out of frames that are read where they lie and resized to out_h x out_w.  Two launches, no
 *      host synchronisation between them; both check their arguments before launching (B and N 1..65535, out_h and out_w
 *      1..1024) and take `frames`: device [B] records of kodhip_frame_desc_bytes() bytes, of which only the planes, pitches,
 *      format, h, w and the six colour integers are read.
 *
 * kodhip_crop_plan, one thread per crop: crop n takes row rows + row_index[n] * row_stride (row_stride >= 4 floats; x1, y1, x2, y2
 * come first - a [B, max_det, 6] buffer with gaps and a dense [N, 6] one both work) of frame frame_index[n].  The rectangle in
 * fp32, every operation rounded once: cx = (x1 + x2) / 2, w = x2 - x1 (likewise y); square: w = h = max(w, h); w = w * gain + pad;
 * x1' = cx - w / 2, x2' = cx + w / 2; clamped to [0, W] and [0, H] of the frame; x0 = int(x1'), cw = int(x2') - x0 (toward zero).
 * cw < 1 or ch < 1, a non-finite coordinate (or a NaN edge of an overflowed box), a negative row index or a frame index
 * outside [0, B) make the crop EMPTY: valid = 0, the rectangle (0, 0, 0, 0), nothing is read for it.  Geometry in double: mode 0
 * (stretch, cv2.resize(cutout, (out_w, out_h))): nh = out_h, nw = out_w, top = left = 0; mode 1 (letterbox):
 * r = min(out_h / ch, out_w / cw), nh = clamp(rint(ch * r), 1, out_h) (half to even), likewise nw, top = (out_h - nh) / 2,
 * left = (out_w - nw) / 2; scale_y = 1.0 / (nh / (double)ch), scale_x likewise.  gain finite and > 0, pad finite and >= 0.
 * crops: device [N] records of kodhip_crop_desc_bytes() bytes (core/crops.py CROP_DESC: int frame, valid, x0, y0, w, h, nh, nw,
 * top, left; double scale_x, scale_y); rects: int32 [N, 4] (x0, y0, cw, ch) in the frame's pixels, or NULL.
 *
 * kodhip_crop_batch, grid (ceil(out_h * out_w / 256), N), one thread per output pixel: OpenCV's fixed-point INTER_LINEAR of
 * kodhip_letterbox_batch applied to the cutout ALONE (coefficients from cw / ch, taps clamped to the cutout's edges; the origin
 * is added only where a pixel is fetched, so a 4:2:0 cutout at an odd origin takes chroma sample (r >> 1, c >> 1) of the
 * absolute position), the copy path when nh == ch and nw == cw, 114 for letterbox borders and for every pixel of an empty
 * crop.  out_f32 [N, 3, out_h, out_w]: (float)p / 255.f, then with mean_std (HOST float[6]: mean r g b, std r g b in the
 * output's channel order; std finite and non-zero) (v - mean[c]) / std[c], a true division; out_u8 [N, out_h, out_w, 3];
 * at least one of the two.  bgr != 0 swaps the channel order of both.  Only bytes inside a frame's rows are read, with byte
 * loads; nothing depends on alignment. */
int kodhip_crop_desc_bytes(void);
int kodhip_crop_plan(const void* frames /* device [B] */, int B, const float* rows, int row_stride, const int* row_index /* [N] */,
                     const int* frame_index /* [N] */, int N, int out_h, int out_w, int mode, int square, float gain, float pad,
                     void* crops /* device [N] */, int* rects /* [N, 4] or NULL */, kodStream_t stream);
int kodhip_crop_batch(const void* frames /* device [B] */, int B, const void* crops /* device [N] */, int N,
                      float* out_f32 /* or NULL */, unsigned char* out_u8 /* or NULL */, int out_h, int out_w, int bgr,
                      const float* mean_std /* host [6] or NULL */, kodStream_t stream);

/* ---- evaluation post-process (kod/lightning/experiments/yv5_baseline/layers.py:55-155, exp.py:70-102;
 *      kod/core/nms.py:9-75 + torchvision.ops.nms) -------------------------------------------------- */
typedef struct KodDecodeLevel { const float* raw; int h, w, stride; float anchor_w[3], anchor_h[3]; } KodDecodeLevel;
int kodhip_decode(const KodDecodeLevel* levels /* host[3] */, float* det, int B, int A, int nc, kodStream_t stream);
int kodhip_nms(const float* det, void* keys, int key_cap, int* ncand, float* out, int* nout,
               int B, int rows, int nc, float conf_thres, float nms_thres, int max_det, int max_nms, float max_wh,
               kodStream_t stream);

/* ---- test-time augmentation (YOLOv5 models/yolo.py::_forward_augment, utils/torch_utils.py::scale_img): the batch also
 *      goes through the network flipped left-right at 0.83 of its size and unflipped at 0.67; the three sets of
 *      predictions are brought back into the full-size frame, trimmed (_clip_augmented) and concatenated for ONE NMS.
 *
 * kodhip_tta_view: one view of a batch that is already on the device.  x [B][3][H][W] fp32 is flipped left-right first
 * (flip_lr), resized to h x w (bilinear, align_corners = False; down-scaling only) and placed top-left in an Hp x Wp
 * canvas filled with `pad` (YOLOv5: 0.447).  out_pairs: bf16 [B][Hp][Wp/2][8], the network's input layout (what
 * kodhip_nchw_to_nhwc4 produces, the same fp32 -> bf16 rounding); out_f32 [B][3][Hp][Wp] or NULL: the same fp32 values.
 * The arithmetic, fp32, every operation rounded on its own (no FMA), per axis with n_in source and n_out view samples:
 *     scale = fp32(n_in) / fp32(n_out)
 *     src   = max(fp32(fp32(dst + 0.5f) * scale) - 0.5f, 0)
 *     i0 = (int)src, i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1
 *     out   = hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c + wx1 * d)       a, b on row y0; c, d on row y1
 * (products rounded, then the inner sums, then the outer products, then the outer sum).  h = H and w = W give l1 = 0
 * everywhere: the (flipped) pixels themselves.  Refused before any launch: a null x or out_pairs, h > H, w > W, Hp < h,
 * Wp < w, odd Wp.
 *
 * kodhip_decode_view: kodhip_decode for one view of the merged [B][rows_total][5+nc] tensor.  `levels` describe the
 * view's own head tensors; bit l of level_mask says whether level l takes part (the first view drops its last level, the
 * last view its first).  The view's rows go to [row_offset, row_offset + own rows) of every image, nothing else is
 * written.  Per row: cx, cy, w, h as in kodhip_decode at the view's strides, each divided by `scale` (IEEE fp32
 * division), cx = full_width - cx when flip_lr, then the corners cx -+ 0.5f * w, cy -+ 0.5f * h; objectness and class
 * scores untouched.  scale = 1, flip_lr = 0, level_mask = 7, row_offset = 0, rows_total = own rows is kodhip_decode bit
 * for bit. */
int kodhip_tta_view(const float* x, void* out_pairs, float* out_f32 /* or NULL */, int B, int H, int W, int h, int w,
                    int Hp, int Wp, int flip_lr, float pad, kodStream_t stream);
int kodhip_decode_view(const KodDecodeLevel* levels /* host[3] */, float* det, int B, int A, int nc, float scale,
                       int flip_lr, float full_width, int level_mask, int row_offset, int rows_total, kodStream_t stream);

/* ---- multi-scale training (YOLOv5 train.py --multi-scale: F.interpolate(imgs, size, mode="bilinear", align_corners=False)
 *      on every batch, to a random multiple of 32 between 0.5 and 1.5 of the training size).
 *
 * kodhip_multiscale_batch: one launch resizes a base-size batch that is already on the device to h x w - up or down, each
 * axis on its own - and scales the batch's boxes with it.  Exactly one source is given: x_f32 [B][3][H][W] fp32, or x_pairs
 * bf16 [B][H][W/2][8] (the network's input layout; read as bf16 -> fp32, which is exact).  out_pairs: bf16 [B][h][w/2][8]
 * (channels 3 and 7 are 0, the fp32 -> bf16 rounding of kodhip_nchw_to_nhwc4); out_f32 [B][3][h][w] or NULL: the same fp32
 * values before that rounding.  The image arithmetic is kodhip_tta_view's, fp32, every operation rounded on its own (no
 * FMA), per axis with n_in source and n_out destination samples:
 *     scale = fp32(n_in) / fp32(n_out)
 *     src   = max(fp32(fp32(dst + 0.5f) * scale) - 0.5f, 0)
 *     i0 = (int)src (at most n_in - 1), i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1
 *     out   = hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c + wx1 * d)       a, b on row y0; c, d on row y1
 * h = H and w = W give l1 = 0 everywhere: the pixels themselves (rounded to bf16 in out_pairs).
 * Boxes: boxes_in [n][4] fp64 xyxy pixels of the base size -> boxes_out, x' = x * (fp64(w) / fp64(W)), y' = y * (fp64(h) /
 * fp64(H)), one rounded fp64 multiply each; rows of zeros stay zeros; boxes_out == boxes_in is allowed; n == 0 or NULL
 * boxes_in: pixels only.  One thread per output pixel pair, the boxes in extra blocks of the same launch.
 * Refused before any launch: both or neither source, a null out_pairs, odd W or w, non-positive sizes, B * h * w or B * H * W
 * of 2^33 and more, n < 0, misaligned buffers (pairs 16 bytes, out_f32 8), an output that overlaps the source, boxes_out
 * partly overlapping boxes_in. */
int kodhip_multiscale_batch(const float* x_f32 /* or NULL */, const void* x_pairs /* or NULL */, void* out_pairs,
                            float* out_f32 /* or NULL */, int B, int H, int W, int h, int w,
                            const double* boxes_in /* or NULL */, double* boxes_out, int n, kodStream_t stream);

/* kodhip_nms with the deployment options of YOLOv5's detect.py.  With best_class = 0, class_keep = NULL and
 * letterbox = NULL it is kodhip_nms: the same launches, the same bits.
 *   best_class = 1  (multi_label=False) one candidate per row: score = max over c of fp32(cls_c * obj), the LOWEST class
 *                   index among equal maxima; kept if obj > conf and score > conf.  Keys, sort and greedy pass are those
 *                   of kodhip_nms, candidates are listed in row order, and key_cap >= rows holds every candidate (the
 *                   multi-label form needs rows * nc).
 *   class_keep      u8 [nc]: a candidate whose class has 0 is dropped - in best-class mode AFTER the argmax (a row whose
 *                   best class is not listed is gone even if a listed class passes conf); in multi-label mode this is
 *                   the same as zeroing the class columns.
 *   letterbox       [B]: NMS runs in the letterboxed frame; the rows written to `out` become
 *                   x' = min(max(fp32(fp32(x - left) * scale_x), 0), width), y' likewise with top, scale_y, height
 *                   (one small launch behind the greedy pass).  Boxes that clipping makes degenerate stay.
 * Class-agnostic suppression needs no option: max_wh = 0.  max_det in 1..300, key_cap a power of two >= 64,
 * best_class 0 or 1 - checked before any launch. */
typedef struct KodLetterbox { float left, top, scale_x, scale_y, width, height; } KodLetterbox;   /* 24 bytes */
int kodhip_letterbox_bytes(void);
int kodhip_nms_ex(const float* det, void* keys, int key_cap, int* ncand, float* out, int* nout,
                  int B, int rows, int nc, float conf_thres, float nms_thres, int max_det, int max_nms, float max_wh,
                  int best_class, const unsigned char* class_keep /* [nc] or NULL */,
                  const KodLetterbox* letterbox /* [B] or NULL */, kodStream_t stream);

/* ---- tiled (sliced) inference: an image larger than the network's input is cut into overlapping S x S tiles at its
 *      native resolution, the tiles (and one letterboxed view of the whole image) go through the network and
 *      kodhip_nms_ex, whose KodLetterbox rows (tile at (x0, y0): left = -x0, top = -y0, scale 1, the image's width and
 *      height) put the kept rows into image pixels, and ONE merge per image joins what the views found.
 *
 * kodhip_tile_batch: descs is a device array [T] of { long off; int h, w, x0, y0; } (kodhip_tile_desc_bytes() = 24);
 * slot t is the S x S window of the u8 HWC image at pool + off with its corner at (x0, y0).  A pixel inside the image is
 * (float)u8 / 255.f, a pixel outside it (an image smaller than the tile) 114 / 255.f: the values of kodhip_val_prep_batch,
 * so a tile is bit-identical to a letterbox at scale 1.  out_f32 [T][3][S][S] and / or out_pairs bf16 [T][S][S/2][8] (the
 * network's input layout, the same fp32 -> bf16 rounding, a zero fourth channel); both 16-byte aligned.  Refused before
 * any launch: a null pool or descs, both outputs null, T < 1, S < 2, odd S, a misaligned output.
 *
 * kodhip_merge_detections: rows [V][max_rows][6] (x1, y1, x2, y2, score, class: kodhip_nms_ex's `out`, in image pixels)
 * and counts [V]; rows at or beyond a view's count are never read.  The views of image i are view_start[i] ..
 * view_start[i + 1] (view_start: device int [n_images + 1]).  An image's candidates are its views' valid rows in (view,
 * rank) order; they are sorted by score, best first, equal scores in that order (key = sortable score << 32 | slot, slot =
 * (view - first view) * max_rows + rank; the bitonic network of kodhip_nms).  Then, candidate by candidate: one that an
 * earlier keeper has absorbed is skipped; otherwise it is kept as output row nk and absorbs every later candidate, not
 * yet absorbed, of the same class (any class when agnostic) whose metric against the keeper's ORIGINAL box exceeds thr.
 * mode 0 (NMS): the absorbed candidate is dropped.  mode 1 (NMM): the keeper's output box also becomes the hull (fminf of
 * the x1 / y1, fmaxf of the x2 / y2; exact); score and class stay the keeper's.  No further row is kept once max_det are.
 * All fp32, every operation rounded on its own: area = (x2 - x1) * (y2 - y1); inter = max(0, min(x2) - max(x1)) *
 * max(0, min(y2) - max(y1)); metric 0 (IoU) = inter / (aa + ab - inter), metric 1 (IoS) = inter / fminf(aa, ab); 0 / 0 is
 * NaN and matches nothing.  Classes are compared directly: there is no class offset.
 * keys: n_images * key_cap u64 workspace, key_cap a power of two in 64 .. kodhip_merge_max_rows() (65536) and at least an
 * image's views * max_rows.  out [n_images][max_det][6], best score first; nout [n_images] (used as scratch between the
 * launches).  Refused before any launch: null pointers, n_images < 1, max_rows < 1, max_det outside 1..300, metric / mode /
 * agnostic other than 0 or 1, thr outside [0, 1], a bad key_cap. */
int kodhip_tile_desc_bytes(void);
int kodhip_tile_batch(const void* pool, const void* descs, float* out_f32 /* or NULL */, void* out_pairs /* or NULL */,
                      int T, int S, kodStream_t stream);
int kodhip_merge_max_rows(void);
int kodhip_merge_detections(const float* rows, const int* counts, const int* view_start, void* keys, int key_cap,
                            float* out, int* nout, int n_images, int max_rows, int max_det, int metric, float thr,
                            int mode, int agnostic, kodStream_t stream);

/* ---- model ensembles: weighted boxes fusion (WBF; Solovyev, Wang, Gabruseva 2021), csrc/fusion.hip.  The views of an
 *      image are the members of an ensemble (model 0 .. M-1); rows, counts and view_start are kodhip_merge_detections'.
 *
 * kodhip_fuse_detections, per image, all fp32 with every operation rounded on its own: W = the sum of its views' weights
 * in view order.  A row of view v with score s is a candidate iff t = s * view_weight[v] > 0 (zero, negative and NaN
 * scores are dropped); candidates are taken by t descending, equal t by view, then rank (key = sortable t << 32 | slot,
 * the bitonic network of kodhip_nms).  Each candidate (box b, class c) meets every cluster of class c (every cluster
 * when agnostic) through the cluster's CURRENT fused box F: area = (x2 - x1) * (y2 - y1), inter = max(0, min(x2) -
 * max(x1)) * max(0, min(y2) - max(y1)), an empty intersection never matches, iou = inter / ((area_F + area_b) - inter).
 * It joins the cluster of largest iou > thr (strict, NaN never matches; equal IoUs: the cluster created first): per
 * coordinate acc += t * x, then st += t, n += 1, F = acc / st.  Without a match it opens a cluster: F = its own four
 * floats bit for bit, acc = t * x, st = t, n = 1, class c (an agnostic cluster keeps its first member's class).  Final
 * score of a cluster = (st / n) * (min(n, W) / W), n as a float.  out: the clusters by final score descending, equal
 * scores by creation order, the first max_det of them as x1, y1, x2, y2, score, class.  Nothing is cut before that ranking.
 * view_weight: device fp32 [V], finite and > 0.  keys: n_images * key_cap u64 workspace, key_cap a power of two in 64 ..
 * kodhip_fuse_max_rows() (4096 = 13 models x 300 rows) and at least an image's views * max_rows (views that do not fit
 * are left out; nothing is written beyond key_cap).  out [n_images][max_det][6]; nout [n_images] (used as scratch between
 * the launches).  Refused before any launch: null pointers, n_images < 1, max_rows < 1, max_det outside 1..300, agnostic
 * other than 0 or 1, thr outside [0, 1], a bad key_cap. */
int kodhip_fuse_max_rows(void);
int kodhip_fuse_detections(const float* rows, const int* counts, const int* view_start, const float* view_weight,
                           void* keys, int key_cap, float* out, int* nout, int n_images, int max_rows, int max_det,
                           float thr, int agnostic, kodStream_t stream);

/* ---- multi-object tracking in ByteTrack's form (Zhang et al., ECCV 2022), csrc/tracking.hip: which of this frame's boxes is
 *      the object seen in the frame before.  All state lives in the caller's device buffer; a call is one launch, one block
 *      per stream, and can be captured in a hipGraph (no synchronisation, no allocation, every loop bounded by cap and max_rows).
 *
 * state: per stream kodhip_track_header_bytes() (16: KodTrackHeader) + cap * kodhip_track_bytes() (112: KodTrack), 16-byte
 * aligned; cap a power of two in 64..1024.  kodhip_track_reset frees all slots of S streams: every byte 0, next_id = 1.
 * kf holds, per coordinate c of (cx, cy, a = w / h, h), p, v, Ppp, Ppv, Pvv: ByteTrack's 8-state constant-velocity Kalman
 * filter, whose covariance never leaves four independent 2 x 2 blocks.  All arithmetic is fp32, every operation rounded on
 * its own, in the order written here; wp = 0.05f, wv = 0.00625f:
 *   measurement of a row: w = x2 - x1, h = y2 - y1, cx = x1 + w / 2, cy = y1 + h / 2, a = w / h; a row with !(w > 0 && h > 0)
 *              or a NaN score takes part in nothing;
 *   track box: w = a * h, x1 = cx - w / 2, y1 = cy - h / 2, x2 = x1 + w, y2 = y1 + h (from the p values);
 *   initiate : p = z, v = 0, Ppv = 0, Ppp = s * s with s = 0.1f * h (a: 1e-2f), Pvv = s * s with s = 0.0625f * h (a: 1e-5f);
 *   predict  : hh = h's p before; sp = wp * hh (a: 1e-2f), sv = wv * hh (a: 1e-5f); from the old values p = p + v,
 *              Ppp = ((Ppp + 2 * Ppv) + Pvv) + sp * sp, Ppv = Ppv + Pvv, Pvv = Pvv + sv * sv;
 *   update(z): hh = h's p before; sr = wp * hh (a: 1e-1f); S = Ppp + sr * sr, kp = Ppp / S, kv = Ppv / S, y = z - p;
 *              p = p + kp * y, v = v + kv * y, Ppp = Ppp - (kp * kp) * S, Ppv = Ppv - (kp * kv) * S, Pvv = Pvv - (kv * kv) * S.
 * Similarity of a track box A and a row B: kodhip_fuse_detections' IoU (area = (x2 - x1) * (y2 - y1), inter = max(0, min(x2)
 * - max(x1)) * max(0, min(y2) - max(y1)), iou = inter / ((aa + ab) - inter)), times the row's score where fuse_score applies;
 * NaN matches nothing; with agnostic 0 a pair of different classes is not admissible.
 * Association is greedy and fully ordered (NOT ByteTrack's optimal linear assignment, whose ties are undetermined): the
 * admissible pairs (slot t, row d) with sim > thr (strict) by sim descending, equal sims by lower t, then lower d; a pair is
 * accepted iff neither side is taken yet.
 * One frame (frame += 1 first): 1. every tracked or lost track is predicted, a lost one with v of h set to 0 first; new
 * tracks are not.  2. a row is "high" iff score > high_thres, "low" iff low_thres < score <= high_thres.  3. tracked and
 * lost tracks against the high rows, fuse_score as given, thr = sim1; a match updates the filter, sets state = tracked and
 * score, cls, last_frame from the row (a lost track keeps its id).  4. tracks still unmatched whose state is tracked
 * against the low rows, plain IoU, thr = sim2.  5. tracked tracks still unmatched become lost (last_frame stays).  6. new
 * tracks against the high rows left over, fuse_score as given, thr = sim3; an unmatched new track becomes free.  7. high
 * rows still unmatched with score >= new_thres start tracks, in row order into the lowest free slots (those of step 6
 * included): id = next_id++, the filter initiated, state = tracked if frame == 1 else new, start_frame = last_frame = frame;
 * without a free slot the row is dropped and dropped += 1.  8. lost tracks with frame - last_frame > max_lost become free
 * (only `state` changes; the slot is usable from the next frame).  9. every track in state tracked, by slot ascending:
 * out row = track box of the updated filter, score, class; out_ids row = id, the matched row (a frame-1 creation: its own).
 *
 * kodhip_track_update: rows [S][F][max_rows][6] (kodhip_nms_ex's `out`), counts [S][F] (rows at or beyond a count are never
 * read); a stream's F frames run one after the other inside the launch (a clip: a batch of consecutive frames through the
 * network, then one call).  out [S][F][cap][6], out_ids [S][F][cap][2], nout [S][F]; nothing is written behind the emitted
 * rows.  workspace: kodhip_track_workspace_bytes() bytes - 0 today, the pointer is not read and may be null.  Refused before
 * any launch: null pointers, S < 1, F < 1, max_rows outside 1..300, a bad cap, a threshold outside [0, 1], low_thres >
 * high_thres, fuse_score / agnostic other than 0 or 1, max_lost < 0. */
typedef struct KodTrackHeader { int frame, next_id, dropped, pad; } KodTrackHeader;               /* 16 bytes */
typedef struct KodTrack {                                                                         /* 112 bytes */
  int state;                    /* 0 free, 1 new, 2 tracked, 3 lost */
  int id, last_frame, start_frame;
  float score, cls;
  float kf[4][5];
  int pad[2];
} KodTrack;
int kodhip_track_header_bytes(void);
int kodhip_track_bytes(void);
long long kodhip_track_workspace_bytes(int S, int cap, int max_rows);
int kodhip_track_reset(void* state, int S, int cap, kodStream_t stream);
int kodhip_track_update(void* state, const float* rows, const int* counts, int S, int F, int max_rows, int cap,
                        float high_thres, float low_thres, float new_thres, float sim1, float sim2, float sim3,
                        int fuse_score, int agnostic, int max_lost, float* out, int* out_ids, int* nout, void* workspace,
                        kodStream_t stream);

/* detection <-> ground-truth matching of COCO-style mAP (kod/lightning/callbacks/pycoco_map_eval.py:50-125 ->
 * vision_evaluation -> pycocotools COCOeval.evaluateImg); tp [B][max_det][T] u8, counted [B][max_det] u8.
 * At most 256 ground truths per image take part in the matching (later ones are never matched). */
int kodhip_map_match(const float* det, const int* ndet, const double* gt_boxes, const long* gt_labels,
                     const int* gt_start, void* tp, void* counted, int B, int max_det, int nc,
                     const double* iou_thresholds /* host */, int T, int max_per_class, kodStream_t stream);

/* detection confusion matrix (YOLOv5 val.py ConfusionMatrix.process_batch, deterministic): the arrays of kodhip_map_match;
 * matrix is device int64 [(nc+1)*(nc+1)], row = predicted class, column = true class, index nc = background, and is ADDED
 * to.  Per image, class-agnostic, fp64 IoU without +1: a detection with score > conf_thres (fp32, strict) picks the
 * ground truth of largest IoU > iou_thres (strict; ties -> lower ground-truth index); a ground truth takes, among the
 * detections that picked it, the one of largest IoU (ties -> lower detection index); losers are not re-matched.  Matched
 * pair -> [class][label], ground truth nobody took -> [nc][label], kept detection not taken -> [class][nc].  Classes
 * outside [0, nc) take no part.  No cap on ground truths per image; max_det <= kodhip_confusion_max_det().
 * kodhip_confusion_lds_classes(): the largest nc whose per-image matrix is summed on chip before the atomic flush. */
int kodhip_confusion_max_det(void);
int kodhip_confusion_lds_classes(void);
int kodhip_confusion_match(const float* det, const int* ndet, const double* gt_boxes, const long* gt_labels,
                           const int* gt_start, long long* matrix, int B, int max_det, int nc, float conf_thres,
                           double iou_thres, kodStream_t stream);

/* ---- YOLOv5 validation metrics (val.py process_batch + utils/metrics.py ap_per_class), csrc/val_metrics.hip.
 * A record is kodhip_val_record_bytes() = 8 bytes: {score fp32 bits : 32, class : 16 | mask over the IoU thresholds : 16}.
 * records / count / nt are device memory owned by the caller: records [capacity] (8-byte aligned), count int32 [1] (the
 * running record count), nt int64 [nc] (ground truths per class, ADDED to).  capacity <= 2^30; nothing is ever written at
 * or beyond it, so a caller that keeps capacity >= the sum of B * max_det over its batches never loses a record.
 *
 * kodhip_val_match: the arrays of kodhip_confusion_match plus T <= kodhip_val_max_thresholds() host fp64 IoU thresholds
 * (used as given).  Per image, fp64 IoU without +1 or epsilon (a zero or NaN union is never a candidate): a detection
 * picks the ground truth of its own class with the largest IoU (ties -> lower ground-truth index) and is correct at
 * threshold t iff run < t <= IoU, run = the largest IoU among LOWER-index detections that picked the same ground truth
 * (-1 if none); a detection that loses its ground truth is not re-matched.  Every detection with a class in [0, nc) appends
 * one record, in image order then detection order; offsets is device scratch int32 [B].  max_det <= kodhip_val_max_det().
 *
 * kodhip_val_append: appends the first min(*src_count, src_bound) records of src behind dst's and advances *dst_count.
 *
 * kodhip_val_curves: sorts the records by (class ascending, score descending, arrival ascending) and evaluates, per class
 * with nt > 0 and at least one record (zero rows otherwise), ap_per_class in fp64 and its operation order:
 * r [nc][npx] = interp(-px, -conf, recall, left = 0) and p [nc][npx] = interp(-px, -conf, precision, left = 1) at
 * threshold 0, ap [nc][T] = trapezoid sum over xr of interp(xr, [0, recall, 1], envelope of [1, precision, 0]); n_p [nc]
 * int64 = records per class.  px [npx] and xr [nx <= 1024] are DEVICE copies of the host's fp64 grids (np.linspace(0, 1,
 * 1000) and np.linspace(0, 1, 101)): the kernels never recompute a grid value.  workspace: device memory of at least
 * kodhip_val_curves_workspace_bytes(capacity, nc, T) bytes (-1 for bad arguments), 16-byte aligned.  Scores >= 0.
 * All three only enqueue (no allocation, copy to the host or synchronisation). */
int kodhip_val_max_det(void);
int kodhip_val_max_thresholds(void);
int kodhip_val_record_bytes(void);
int kodhip_val_match(const float* det, const int* ndet, const double* gt_boxes, const long* gt_labels, const int* gt_start,
                     const double* iou_thresholds /* host */, int T, void* records, int* count, long long capacity,
                     long long* nt, int* offsets, int B, int max_det, int nc, kodStream_t stream);
int kodhip_val_append(void* dst, int* dst_count, long long dst_capacity, const void* src, const int* src_count,
                      long long src_bound, kodStream_t stream);
long long kodhip_val_curves_workspace_bytes(long long capacity, int nc, int T);
int kodhip_val_curves(const void* records, const int* count, long long capacity, const long long* nt, const double* px, int npx,
                      const double* xr, int nx, int nc, int T, void* workspace, double* p, double* r, double* ap,
                      long long* n_p, kodStream_t stream);

/* ---- auto-anchor (YOLOv5 utils/autoanchor.py: check_anchors / kmean_anchors), csrc/anchors.hip.  Box sizes wh are device
 * fp32 [N][2], positive and finite, 8-byte aligned.  Every launch uses min(ceil(N / kodhip_anchor_block_size()),
 * kodhip_anchor_grid_cap()) blocks, grid-strided beyond: sums are ordered by N alone and repeat bit for bit.  The functions
 * only enqueue kernels (no allocation, copy or synchronisation: capturable); `workspace` is device memory of at least
 * kodhip_anchor_workspace_bytes(N, sets) bytes, sets = P (metric, evolve) or R (k-means step), 8-byte aligned.
 * Limits: n <= kodhip_anchor_max_anchors(), P <= kodhip_anchor_max_population(), R <= kodhip_anchor_max_restarts(). */
int kodhip_anchor_max_anchors(void);
int kodhip_anchor_max_population(void);
int kodhip_anchor_max_restarts(void);
int kodhip_anchor_block_size(void);
int kodhip_anchor_grid_cap(void);
int kodhip_anchor_trace_bytes(void);                 /* one trace entry: { int winner; int accepted; double fitness_sum; } */
long kodhip_anchor_workspace_bytes(long N, int sets);
/* P anchor sets [P][n][2] in one launch pair.  Per box and anchor, fp32: r = wh / k, x = min(min(r_w, 1 / r_w), min(r_h, 1 / r_h)),
 * best = max over the anchors.  fitness_sum[p] = sum of best where best > t (fp64), n_recalled[p] = boxes with best > t,
 * n_pairs[p] = (box, anchor) pairs with x > t; t = float32(1 / thr), comparisons strict.  Outputs are device arrays [P]. */
int kodhip_anchor_metric(const float* wh, long N, const float* anchors, int P, int n, float t, void* workspace,
                         double* fitness_sum, long long* n_recalled, long long* n_pairs, kodStream_t stream);
/* The whole genetic search, 2 * gen launches: in generation g candidate p is max(anchors * mutations[g][p], 2.0f) (fp32
 * multiply, then max); the candidate with the largest fitness sum (equal sums: lower index) replaces `anchors` [n][2] and
 * `*fitness` (device fp64, in/out) when it is strictly better; trace[g] (device) records winner, accepted, winner's sum.
 * mutations: device fp32 [gen][P][n][2].  gen = 0 launches nothing. */
int kodhip_anchor_evolve(const float* wh, long N, float* anchors, double* fitness, const float* mutations, int gen, int P, int n,
                         float t, void* trace, void* workspace, kodStream_t stream);
/* One Lloyd step of R independent restarts: points [N][2], centroids [R][n][2] in/out.  A point joins the centroid of least
 * (x-cx)*(x-cx) + (y-cy)*(y-cy) (fp32, equal distances: lower index); new centroid = float32(fp64 sum / count), an empty
 * cluster keeps its centroid.  distortion [R] fp64 = sum of the winning squared distances (to the OLD centroids),
 * counts [R][n] int64, labels [R][N] int32 or NULL - all device. */
int kodhip_anchor_kmeans_step(const float* points, long N, float* centroids, int R, int n, void* workspace, double* distortion,
                              long long* counts, int* labels, kodStream_t stream);

/* ---- data-parallel collectives (Lightning strategy=ddp + sync_batchnorm=True, kod/configs/trainer/ddp.yaml:4-9:
 *      torch DistributedDataParallel's bucketed gradient all-reduce, SyncBatchNorm's statistic exchange and the
 *      initial parameter/buffer broadcast).  RCCL enqueued on the caller's stream; hipGraph-capturable. ------ */
int kodhip_comm_load(const char* rccl_path /* NULL: the copy already loaded in the process */);
int kodhip_comm_unique_id(void* id128 /* host, 128 bytes out */);
int kodhip_comm_init(void** comm, const void* id128, int rank, int world);
int kodhip_comm_destroy(void* comm);
int kodhip_comm_allreduce_sum(void* comm, void* buf, long count, int elem_bytes /* 4: fp32, 8: fp64 */, kodStream_t stream);
int kodhip_comm_allreduce_sum_to(void* comm, const void* send, void* recv, long count, int elem_bytes, kodStream_t stream);
int kodhip_comm_broadcast(void* comm, void* buf, long bytes, int root, kodStream_t stream);
/* collectives enqueued between the two calls are launched as one fused operation (ncclGroupStart / ncclGroupEnd) */
int kodhip_comm_group_start(void);
int kodhip_comm_group_end(void);

/* ---- SyncBN statistic exchange over peer buffers (sync_batchnorm: True, kod/configs/trainer/ddp.yaml:9; replaces the
 *      114 small all-reduces torch SyncBatchNorm issues per step).  Every rank of the node owns one small exchange
 *      buffer - the ONE device allocation this library makes (fine-grained memory), freed by kodhip_peer_destroy - and
 *      maps the others' through HIP IPC; the BatchNorm finalize / coefficient kernels publish their two fp64 sums per
 *      channel there and read the other ranks' directly over xGMI: no collective launch, no communicator order. ----- */
#define KODHIP_PEER_MAX 8
typedef struct KodPeerView {                       /* passed BY VALUE to the *_peer kernels */
  unsigned long long* peers[KODHIP_PEER_MAX];
  int world, rank;
  const unsigned int* seq;
  int* timeout_flag;                               /* device: 1 = a poll gave up, 2 = the ranks' step counters diverged */
  int* host_flag;                                  /* the same verdict mirrored into pinned host memory */
  long max_spins;                                  /* polls before a wait gives up and raises the flag */
} KodPeerView;
/* fails (no coarse-grained fallback) when fine-grained device memory cannot be had: the caller keeps the RCCL exchanges */
int kodhip_peer_create(void** peer, int rank, int world, long granules /* 8-byte granules: 4 per channel per exchange site */);
int kodhip_peer_export(void* peer, void* handle64 /* host, 64 bytes out: hipIpcMemHandle_t */);
int kodhip_peer_connect(void* peer, const void* handles /* host, world x 64 bytes in rank order */);
/* the same for ranks living in ONE process (no IPC): peers = the world's kodhip_peer_create handles in rank order */
int kodhip_peer_connect_local(void* peer, void* const* peers);
int kodhip_peer_view_bytes(void);
int kodhip_peer_view(void* peer, void* view_out /* host KodPeerView */);
int kodhip_peer_step_begin(void* peer, kodStream_t stream);      /* once per step, before its first exchange */
int kodhip_peer_allreduce_f64(void* peer, const double* in, double* out, int n, unsigned int slot, kodStream_t stream);
/* all ranks of a one-process group (kodhip_peer_connect_local) in ONE dispatch (the ranks' blocks wait for each other, so they
 * must be co-resident: separate launches on separate streams may share a hardware queue); ins / outs in rank order */
int kodhip_peer_allreduce_f64_multi(void* const* peers, int world, const double* const* ins, double* const* outs, int n,
                                    unsigned int slot, kodStream_t stream);
int kodhip_peer_timed_out(void* peer, int* flag /* host out; synchronises, resets the flag */);
/* the verdict without a device synchronisation (pinned host mirror): 0 ok, 1 a poll gave up, 2 step counters diverged.
 * A failed exchange never folds a stale payload into the statistics: its sums become NaN. */
int kodhip_peer_status(void* peer, int* flag /* host out */);
int kodhip_peer_destroy(void* peer);

#ifdef __cplusplus
}
#endif
#endif /* KODHIP_H */
