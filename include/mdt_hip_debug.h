/*
 * mdt_hip_debug.h -- process-global test and measurement hooks of libmdt_hip.so.
 *
 * NOT part of the product boundary (mdt_hip.h and the operator headers): every setter here flips a launch choice for EVERY handle
 * of the process, none is needed to run the model, and a host that binds the library should leave them alone.  The parity tests
 * use them to pin one kernel form against another, bench.py and tools/ to measure one.  All of them write one table inside the
 * library (csrc/mdt_internal.h: mdt_switches); a negative argument restores the default unless a hook says otherwise.  No other
 * header includes this one.
 */
#ifndef MDT_HIP_DEBUG_H
#define MDT_HIP_DEBUG_H

#include <stdint.h>
#include "mdt_hip.h"
#include "mdt_hip_ops.h"
#include "mdt_hip_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The split forms of the model's fused MLP launch and of the wide LayerNorm-prologue products (mdt_gemm_args.Wp_split / Wp_pair): 0 = the fp32 launches
 * everywhere, 1 = on, negative = default (MDT_HIP_MLP_SPLIT from the environment; unset = 1). */
void mdt_op_set_mlp_split(int32_t on);
/* The model-level entry points run the MLP sublayer through mdt_op_mlp from `rows` rows (B * horizon) on; 0 = never (the two-GEMM
 * sequence), -1 = default (1401; 768 where the split form applies).  The split form always needs 768 rows: below them a setting
 * runs the fp32 form. */
void mdt_op_set_mlp_fuse_min(int32_t rows);
/* Rollout-sized model-level calls queue the products that do not depend on their neighbours in the launch chain (the sigma-MLP /
 * adaLN table of mdt_sample_ddim, the MDTV token embedding) and let each ride as extra workgroups in the next split-K small-M
 * launch.  0 = every product its own launch, 1 = on, -1 = default (on).  Same tiles, same order inside each product: results are
 * bit-identical either way.
 * mdt_op_side_jobs_paired: how many launches of this process have taken such a product along so far. */
void mdt_op_set_side_jobs(int32_t on);
int64_t mdt_op_side_jobs_paired(void);
/* 1 = the K = 384 products that take the weight-stationary body (from 8192 rows on: the training step at B = 1024) run its
 * THREE-WAY bf16 SPLIT form -- every fp32 operand as three bf16 parts, six v_mfma_f32_16x16x32_bf16 products per k32 step with fp32
 * accumulation: fp32's product accuracy (not its bits) at 2.7x the fp32 matrix rate; 0 = the fp32 MFMA form; negative = default
 * (MDT_HIP_WS_SPLIT from the environment; unset = 1). */
void mdt_op_set_ws_split(int32_t on);
/* 1 = from 8192 rows on the weight-gradient product dW = dY^T X (mdt_op_linear_bwd) runs as three-way bf16 splits of both operands;
 * 0 = the fp32 MFMA kernel everywhere; negative = default (MDT_HIP_TN_SPLIT from the environment; unset = 1). */
void mdt_op_set_tn_split(int32_t on);

/* Wave schedule inside mdt_op_mlp's kernel.  Low byte = number of k-steps the second wave of every SIMD starts behind the first
 * (0 = lockstep with a workgroup barrier between the two products), | 256 = MFMA loops at raised issue priority; -1 = default
 * (18 | 256).  Every setting produces the same bits (the K order of both products does not depend on it). */
void mdt_op_set_mlp_skew(int32_t v);

/* Force the workgroup geometry of every following GEMM launch in this process.
 * 0 = heuristic (default): up to 15 rows the split-K small-M kernel -- one workgroup per 16 columns, K divided between its
 * 8 waves --; up to 512 rows the same kernel for the products whose half-height tiling would have fewer than 60 (LayerNorm
 * prologue) / 100 (plain, <= 192 rows) / 160 (plain, <= 512 rows) tiles; up to 1400 rows the half-height tiled geometry 6;
 * beyond, the widest row-tile geometry that still fills the chip;
 * 1 = 4 waves 32x64; 2 = 8 waves 32x128; 3 = 8 waves 32x384; 4 = 8 waves 32x512; 5 = 4 waves 32x128; 6 = 4 waves 16x64;
 * 7 = 4 waves 64x128; 8 = 4 waves 32x256; 9 = 4 waves 32x192;
 * 10 / 12 / 16 = the TALL body (128-row tiles, both operands staged in LDS by LDS-DMA; plain prologue, K % 32 == 0;
 * anything else falls back to the heuristic): 4 waves 128x128 / 128x64 / 128x96; 23 = 128x64 with a loader wave, 3 stages;
 * -1 = the split-K small-M kernel wherever it applies.
 * 30 = the weight-stationary body wherever it is supported, whatever the row count.
 * Row-tile, tall and (fp32 form, mdt_op_set_ws_split(0)) weight-stationary geometries compute bit-identical results (same k order
 * per output element); the small-M kernel and the weight-stationary body's bf16 split form (the default) agree to fp32 rounding. */
void mdt_op_set_gemm_geometry(int32_t geometry);

/* The model-level entry points compute the self-attention of a LARGE batch in the prologue of its output projection
 * (mdt_op_attn_proj's contract on 32-row tiles, k_attn_proj_wide) from `rows` rows on: 0 = never (attention launch + projection
 * GEMM; also switches off the one-workgroup-per-sample form, mdt_op_attn_xattn), -1 = default 1401. */
void mdt_op_set_attn_wide_min(int32_t rows);

/* mdt_op_attention (mdt_hip_ops.h) as a sampler call with candidates launches it: the args->B query samples are chunks of which
 * ctx_div consecutive ones share a context, so sample b reads the k / v rows of context b / ctx_div (k / v hold B / ctx_div * Tk
 * rows; B a multiple of ctx_div).  ctx_div = 1 is mdt_op_attention. */
mdt_status mdt_op_attention_shared(const mdt_attn_args *args, int32_t ctx_div, void *stream);
/* The three attention ops as the decoder's cross-attention launches them at contexts above 16 tokens: a causal launch (top-left
 * aligned mask) with Tk > 16 stages and multiplies its first kv_rows keys only, min(Tq, Tk) <= kv_rows < Tk -- the keys some query
 * sees.  Tk stays the k / v sample stride (sample b's rows start at row b * Tk) and the row length of the dropout index
 * ((b H + h) Tq + i) Tk + j; k / v rows kv_rows .. Tk-1 are never read, and the backward writes rows kv_rows .. Tk-1 of dk / dv as
 * zeros (accumulate_kv: leaves them as they are).  Results equal the full-key launch's.  kv_rows = 0 or Tk is that launch:
 * mdt_op_attention_shared, mdt_op_attn_fwd_train, mdt_op_attn_bwd.  Anything else: MDT_ERR_INVALID_ARG. */
mdt_status mdt_op_attention_prefix(const mdt_attn_args *args, int32_t ctx_div, int32_t kv_rows, void *stream);
mdt_status mdt_op_attn_fwd_train_prefix(const mdt_attn_train_args *args, int32_t kv_rows, void *stream);
mdt_status mdt_op_attn_bwd_prefix(const mdt_attn_bwd_args *args, int32_t kv_rows, void *stream);
/* Bytes of dynamic LDS one workgroup of the attention kernels for Tq or Tk above 16 takes (one workgroup per (sample, head); the
 * launch is refused above 160 KiB).  With T16 = T rounded up to a multiple of 16 and Tv = the keys the launch stages (kv_rows; Tk
 * without a prefix):
 *   forward   4 [(Tq16 + Tv16)(hd + 4) + hd (Tv16 + 4)]
 *   backward  4 [(2 Tq16 + 2 Tv16)(hd + 4) + 2 Tq16 (Tv16 + 4)]  */
int64_t mdt_op_attn_chunk_lds(int32_t hd, int32_t Tq, int32_t kv_rows, int32_t bwd);

/* The two attention launches of the MAP pooling block (mdt_map_pool.h) on the caller's buffers, either kernel family:
 * family 0 = one workgroup per sample (what the block runs at N <= 16; 1..16 tokens, refused above its 64 KiB LDS rule),
 * family 1 = one workgroup per (sample, head group) (what the block runs at N 17..64; here reachable at N 1..64, so that the two
 * can be compared at equal shapes).  q (Q, D): the seed queries, shared by the samples; kv (batch, N, 2 D): K | V rows;
 * out (batch, Q, D); probs (batch, Q, H, N) or NULL in the forward.  The backward reads probs and d_out (batch, Q, D) and writes
 * every element of dq_part (batch, Q, D) and d_kv (batch, N, 2 D) once (no accumulation, nothing to zero).  Q 1..16, D a multiple
 * of 16 up to 512, H even and a divisor of D, 16-byte aligned pointers. */
mdt_status mdt_op_map_attn_fwd(int32_t family, const float *q, const float *kv, float *out, float *probs, int64_t batch, int32_t Q,
                               int32_t N, int32_t D, int32_t H, void *stream);
mdt_status mdt_op_map_attn_bwd(int32_t family, const float *q, const float *kv, const float *probs, const float *d_out,
                               float *dq_part, float *d_kv, int64_t batch, int32_t Q, int32_t N, int32_t D, int32_t H, void *stream);
/* Bytes of dynamic LDS one workgroup of family 1 takes (the rule of mdt_map_pool.h); -1 for a shape that is none. */
int64_t mdt_op_map_attn_lds(int32_t Q, int32_t N, int32_t D, int32_t H, int32_t bwd);

/* The narrow (A = 1..64 wide) linears around the action tokens, each as the training step launches it (A <= 16: one form; 17..64:
 * 16-column tiles of A).  Dense fp32 rows unless a stride is named; every output element is written once, nothing accumulates.
 *   mdt_op_narrow_dw : partial[y] = sum over the rows [M y / n_slices, M (y + 1) / n_slices) of G[m][a] Y[m][d] for y = 0 ..
 *                      n_slices - 1 (a slice without rows: zeros); G (M, A), Y (M, D) with row stride ldy >= D, partial
 *                      (n_slices, A, D), or (n_slices, D, A) when transposed.  The step runs 512 slices and sums them with
 *                      mdt_op_colsum.
 *   mdt_op_narrow_out: out (M, A) = G WT^T; G (M, D) with row stride ldg >= D, WT (A, D).
 *   mdt_op_narrow_dx : out (M, D) = G W; G (M, A), W (A, D).
 * A null pointer, M < 1, A outside 1..64, D < 1, n_slices outside 1..65535 or a stride below D: MDT_ERR_INVALID_ARG, nothing launched. */
mdt_status mdt_op_narrow_dw(const float *G, const float *Y, int64_t ldy, float *partial, int32_t n_slices, int32_t M, int32_t A,
                            int32_t D, int32_t transposed, void *stream);
mdt_status mdt_op_narrow_out(const float *G, int64_t ldg, const float *WT, float *out, int32_t M, int32_t A, int32_t D, void *stream);
mdt_status mdt_op_narrow_dx(const float *G, const float *W, float *out, int32_t M, int32_t A, int32_t D, void *stream);

/* The four element-wise kernels of the steered samplers (mdt_sample_ddim_steer, mdt_sample_steer), each through the launch its
 * entry point makes, on the caller's buffers.  Each is a grid-stride loop over N + R indices -- the N action elements, then the R
 * per-row sigma entries -- of at most 1024 workgroups of 256 threads (mdt_op_steer_seed: the N elements only).  Dense fp32.
 *   mdt_op_steer_seed : D = c_skip x + c_out F;  e = weight (known - D);  dF = c_out e  (the EDM scalings of sigma, sd).
 *   mdt_op_steer_step : g = c_in small + c_skip e;  D' = D + scale g;  x_out = ratio x_in + coef D', clamped to [lo, hi] per
 *                       column i % A where bounds are given;  sig_rows = sigma_next.  x_out may be x_in.  N = 0: the sigma rows
 *                       only, every element pointer unused.
 *   mdt_op_steer_first: X = x_T;  Y = x_T + cn n0 (n0 null or cn == 0: x_T's bits);  hist (4, N) = 0;  sig_rows = sigma0.
 *   mdt_op_steer_plan : D' as above at ev->sigma, then one evaluation of a sampler plan (mdt_hip.h: mdt_sampler_eval) on the
 *                       registers X, Y, D', d = (Y - D') / sigma, H0..H3, N0, N1: x_out = sum cx R, clamped where bounds are
 *                       given and ev->ends_step;  y_out (or null) = cy[NREG] x_out + sum cy R;  rec (2, N) (or null) = Y, D'
 *                       where ev->begins_step;  the history shift of ev->push;  sig_rows = ev->sigma_next.  noise (n_noise, N) or
 *                       null: a row of ev->noise outside [0, n_noise), or any row of a null noise, reads as 0.  x_out may be X,
 *                       y_out may be Y.
 * Refused with MDT_ERR_INVALID_ARG and a text that names the hook and the field, nothing launched: a null required pointer
 * (element operands where N > 0, sig_rows where R > 0); N < 0, R < 0 or N + R < 1 (seed: N < 1); A < 1, or bounds with N no
 * multiple of A; lo without hi or hi without lo; n_noise < 0; sigma, sigma0 or sd not finite and > 0. */
mdt_status mdt_op_steer_seed(const float *F, const float *x, const float *known, const float *weight, float sigma, float sd,
                             int64_t N, float *D, float *e, float *dF, void *stream);
mdt_status mdt_op_steer_step(const float *small, const float *e, const float *D, const float *x_in, float sigma, float sd, float scale,
                             float ratio, float coef, const float *lo, const float *hi, int32_t A, float sigma_next, int64_t N,
                             int64_t R, float *x_out, float *sig_rows, void *stream);
mdt_status mdt_op_steer_first(const float *x_T, const float *n0, float cn, float sigma0, int64_t N, int64_t R, float *X, float *Y,
                              float *hist, float *sig_rows, void *stream);
mdt_status mdt_op_steer_plan(const mdt_sampler_eval *ev, const float *small, const float *e, const float *D, const float *Y,
                             const float *X, float *x_out, float *y_out, float *hist, const float *noise, const float *lo,
                             const float *hi, float *rec, float *sig_rows, int64_t N, int64_t R, float sd, float scale,
                             int32_t n_noise, int32_t A, void *stream);

/* The three kernels of mdt_denoising_score (mdt_hip.h; csrc/mdt_score.hip), each through the launch the call makes, on the caller's
 * buffers.  Dense fp32, 256 threads a workgroup.  B observations, K chunks each, S levels, M noise rows per level; decoder sample
 * j = ((b S + s) K + k) M + m is chunk r = b K + k at level s with noise row i = s M + m.  sigmas (and weights) are HOST arrays of S
 * floats and ride in the kernel arguments.  With den2 = sigma^2 + sd^2, c_in = 1 / sqrt(den2):
 *   mdt_op_score_prep  : over the B S K M Ta decoder rows (sample j, step t), a grid-stride loop over rows * D / 4 threads of at most
 *                        4096 workgroups.  x0 (B K, Ta, A), noise (S M, Ta, A), WaT (A, D), ba (D) are read;
 *                        noised (rows, A) = x0[r, t] + sigma_s noise[i, t] (the product rounded, then the sum);
 *                        y (rows, D) = ba + sum_c (noised[c] c_in(sigma_s)) WaT[c] -- mdt_op_action_embed's arithmetic on `noised`
 *                        with the rows' sigma: c_in by its expression, the fma chain over c = 0 .. A-1 from the bias --;
 *                        sig_rows (B S K M) = sigma_s per sample;  ctx_sig (B S) = sigma_s per (b, s), or NULL: not written.
 *   mdt_op_score_repeat: row i of (B S) <- row i / S of the B rows, for three operands at once: tok -> tok_o (width w1), tok2 ->
 *                        tok2_o (w2; w2 == 0: neither pointer is used), goal -> goal_o (wg); bits, a grid-stride loop over
 *                        B S (w1 + w2 + wg) of at most 4096 workgroups.
 *   mdt_op_score_reduce: score (B K), one workgroup per chunk r, F (B S K M, E) the network's raw output per decoder sample, x0
 *                        (B K, E), noise (S M, E):
 *                            q = sigma / den2 x0[r] - sd^2 / den2 noise[i] - sd / sqrt(den2) F[j],
 *                            score[r] = - sum_s (weights[s] / M) sum_m sum_e q^2.
 *                        Wave w of four takes the samples i with i % 4 == w in order, lane l the elements e = l, l + 64, ..: a
 *                        sample's lane sum enters the lane's total by one fma with weights[s] / M; then the xor butterfly over the
 *                        64 lanes (offsets 32 .. 1) and (p0 + p1) + (p2 + p3) over the waves.  One writer per element, no atomics: a
 *                        call repeats bit for bit, and a chunk reads no other chunk's rows.
 * Every output element is written once; inputs are only read.  Refused with MDT_ERR_INVALID_ARG and a text that names the hook and
 * the field, nothing launched: a null required pointer (all but ctx_sig, and tok2 / tok2_o where w2 == 0); B, K, Ta, A, E, w1 or wg
 * below 1; S or M outside [1, 64]; D below 4 or no multiple of 4; w2 < 0; sd or a level not finite and > 0; a weight not finite and
 * >= 0; B * K above 2^31 - 1 (reduce: one workgroup per chunk). */
mdt_status mdt_op_score_prep(const float *x0, const float *noise, const float *sigmas, int32_t S, int32_t K, int32_t M, int64_t B,
                             int32_t Ta, int32_t A, int32_t D, float sd, const float *WaT, const float *ba, float *y, float *noised,
                             float *sig_rows, float *ctx_sig, void *stream);
mdt_status mdt_op_score_repeat(const float *tok, const float *tok2, const float *goal, int64_t B, int32_t S, int32_t w1, int32_t w2,
                               int32_t wg, float *tok_o, float *tok2_o, float *goal_o, void *stream);
mdt_status mdt_op_score_reduce(const float *F, const float *x0, const float *noise, const float *sigmas, const float *weights,
                               int64_t B, int32_t S, int32_t K, int32_t M, int32_t E, float sd, float *score, void *stream);

/* The selection kernel of mdt_sample*_select (mdt_hip.h; csrc/mdt_score.hip), through the launch the call makes, on the caller's
 * buffers: scores (B K) and chunks (B K, E) are read; index (B) int32 and best (B, E) are written, each element once.  One workgroup
 * of 256 threads per observation: index[b] is the k that gc_sampling.best_candidates(chunks, scores, K) gives -- with the key of a
 * score being the score, NaN read as -Inf, +Inf as the largest finite float and -Inf as the lowest (torch.nan_to_num(nan=-inf)), the
 * largest key wins and ties go to the lowest k; K NaN scores select 0 -- and best[b] = chunks[b K + index[b]], bits.  Lane t scans
 * k = t, t + 256, ..; the wave's 64 lanes and then the four waves reduce (key, k) in a fixed order; no atomics: a call repeats bit
 * for bit.  Refused with MDT_ERR_INVALID_ARG, "mdt_op_score_select: ..." naming the field, nothing launched: a null pointer; B, K
 * or E below 1; B above 2^31 - 1. */
mdt_status mdt_op_score_select(const float *scores, const float *chunks, int64_t B, int32_t K, int32_t E, float *best, int32_t *index,
                               void *stream);

/* Measurement hook: bracket every fused-MLP launch of the model-level calls that follow (mdt_sample_ddim, mdt_forward, ...)
 * with a pair of HIP events on its stream; mdt_op_trace_mlp_read waits for them, writes up to `cap` durations in
 * MICROSECONDS (launch order) to `us`, releases the events and returns how many it wrote.  The duration of the dominant
 * kernel inside its launch chain, as a kernel trace reports it (bench.py's roofline.dominant_kernel).  Process-wide; not
 * for use under stream capture. */
void mdt_op_trace_mlp(int32_t enable);
int32_t mdt_op_trace_mlp_read(float *us, int32_t cap);
/* Behind every traced launch the hook also brackets NOTHING with a second pair of events: mdt_op_trace_mlp_read_empty returns
 * those empty brackets (microseconds; same order and count as the last mdt_op_trace_mlp_read) -- what the bracket itself costs
 * on the stream.  Launch bracket minus empty bracket = the kernel as a kernel trace's row reports it. */
int32_t mdt_op_trace_mlp_read_empty(float *us, int32_t cap);
/* Measurement hook: in stream order, one wave per XCD writes {shader-clock counter (s_memtime), constant 100 MHz counter
 * (s_memrealtime)} to out16[2 x + 0 .. 1] (device memory, 16 values, zero them first; x = the XCD the wave ran on: the shader-clock
 * counters of the eight XCDs are not synchronised).  Two stamps around a span of launches give, XCD by XCD, the average shader clock
 * the chip sustained over it: (d memtime / d memrealtime) x 100 MHz -- what bench.py reports as roofline.sustained_mhz beside the
 * 2.4 GHz the peak is quoted at. */
mdt_status mdt_op_clock_stamp(uint64_t *out16, void *stream);

/* Only a library built with -DMDT_DEBUG_TIMING (the phase-timing variant that the phase tools under tools/ build beside the product library)
 * also exports
 *     int mdt_debug_set_timing_buffer(unsigned long long *stamps);
 * which points the kernels' phase stamps at a device buffer (NULL: off).  The product library does not have the symbol, so it is
 * named here and declared by the tools that load that variant. */

#ifdef __cplusplus
}
#endif
#endif
