/*
 * mdt_hip_ops.h -- kernel-level entry points of libmdt_hip.so.
 *
 * These launch ONE hand-written gfx950 kernel each on caller-provided device buffers.  The model-level
 * ABI (mdt_hip.h) is built from exactly these launches; they are exported so that the parity tests can
 * pin every kernel against a PyTorch fp32 reference of the same op, and so that bench.py can time the
 * dominant kernel in isolation.  fp32 everywhere, row-major, device pointers 16-byte aligned.
 *
 * Reference ops replaced (all in mdt/models/networks/transformers/transformer_blocks.py unless noted):
 *   mdt_op_gemm       nn.Linear (+ F.layer_norm :38 / nn.LayerNorm :205 prologue, modulate :262,
 *                     nn.GELU :171 / nn.Mish / nn.SiLU :251 epilogue, gated residual :296-307)
 *   mdt_op_attention  F.scaled_dot_product_attention :142 (+ RotaryEmbedding position_embeddings.py:138)
 *   mdt_op_layernorm  LayerNorm.forward :37-38
 *   mdt_op_head       decoder.ln + action_pred (mdtv_transformer.py:233-235) + GCDenoiser.forward
 *                     combine (score_wrappers.py:79-80) + sample_ddim update (gc_sampling.py:948-950)
 *                     + next step's action_emb (mdtv_transformer.py:226)
 */
#ifndef MDT_HIP_OPS_H
#define MDT_HIP_OPS_H

#include <stdint.h>
#include "mdt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MDT_ACT_NONE = 0, MDT_ACT_GELU = 1, MDT_ACT_MISH = 2, MDT_ACT_SILU = 3,
       MDT_ACT_SWIGLU = 4 /* only as mdt_linear_bwd_args.dx_act: the layer below is a SwishGLU, dX has 2K columns */ };
enum { MDT_HEAD_DENOISED = 0, MDT_HEAD_DDIM = 1, MDT_HEAD_RAW = 2,
       MDT_HEAD_PLAN = 3 /* a sampler plan's update (mdt_sample; internal: needs the plan operands, not mdt_op_head) */ };

/* Number of floats of the fragment-packed image of an (N, K) Linear weight (N, K multiples of 16). */
int64_t mdt_op_packed_numel(int64_t N, int64_t K);

/* Pack rows [0, n_rows) of a row-major (n_rows, K) weight into rows [n_off, n_off+n_rows) of a packed
 * (N_total, K) image: for every 16(n) x 16(k) block, lane l = n%16 + 16*((k%16)/4) holds the 4
 * consecutive-k values W[n][k0 + 4*(l>>4) .. +3] -- the operand order of v_mfma_f32_16x16x4_f32. */
mdt_status mdt_op_pack_weight(const float *w, int64_t n_rows, int64_t K, float *packed, int64_t n_off,
                              int64_t N_total, void *stream);
/* The packed image of a SwishGLU project weight (2H, K) for mdt_gemm_args.aux_mode 3: 16-row tile 2t holds projected rows
 * [16t, 16t+16), tile 2t+1 the gate rows [H + 16t, H + 16t + 16) (voltron SwishGLU / transformer_blocks.py:54-62:
 * projected, gate = project(x).tensor_split(2, dim=-1)).  H % 16 == 0, K % 16 == 0. */
mdt_status mdt_op_pack_weight_glu(const float *w, int64_t H2, int64_t K, float *packed, void *stream);

typedef struct {
    const float *A;        /* (M, K) activations, row stride lda (multiple of 4)                      */
    int64_t lda;
    const float *Wp;       /* packed (N, K) weight                                                    */
    const float *bias;     /* (N) or NULL                                                             */
    float *out;            /* output rows, row stride ldo                                             */
    int64_t ldo;
    int32_t M, N, K;
    /* prologue: LayerNorm over K (needs K <= 512) and optional modulate shift + x*scale              */
    int32_t ln;            /* 0 = plain A, 1 = layer_norm(A) * ln_w (+ ln_b)                          */
    const float *ln_w, *ln_b;
    const float *mod;      /* NULL, or modulation table: row (m / rows_per_sample) * mod_stride       */
    int64_t mod_stride;    /* 0 broadcasts one row to the whole batch; like shift_off, scale_off and  */
    int32_t shift_off, scale_off;   /* gate_off a multiple of 4 floats (the rows are read 16 bytes at a time) */
    int32_t rows_per_sample;
    /* epilogue                                                                                        */
    int32_t act;           /* MDT_ACT_*  applied after bias                                           */
    int32_t residual;      /* 1: out = out + gate * value (gate = 1 when gate_off < 0)                */
    int32_t gate_off;      /* offset of the gate vector inside the mod row, or -1                     */
    int32_t gin, gout, goff;   /* output row = (m / gin) * gout + m % gin + goff  (1,1,0 = identity)  */
    const float *rowvec;   /* NULL or (N) vector added to every row after bias (positional embedding) */
    /* batched launch: `batch` independent products in one launch, member z reading A + z*bs_a, Wp + z*bs_w and
     * writing out + z*bs_out (floats); 0 or 1 = a single product.  Used for the split-K partial products of the
     * training path's weight gradients.                                                              */
    int32_t batch;
    int64_t bs_a, bs_w, bs_out;
    /* training: a second (M, N) operand laid out like `out` (row stride ldo, same row remap), plain prologue, no residual:
     *   aux_mode 1: aux = the value BEFORE `act` (after bias): one launch leaves both u and act(u);
     *   aux_mode 2: out = value * act'(aux)  -- `act` names the activation whose derivative is taken, the value itself is
     *               not activated (dX of the Linear that follows an activation: d_u = (dY W) * act'(u)).
     *   aux_mode 3: SwishGLU forward on the producing Linear (N = 2H columns [projected | gate]; Wp packed by
     *               mdt_op_pack_weight_glu, which interleaves the two halves tile by tile so that one wave holds a projected
     *               column and its gate): aux (M, 2H, row stride 2 * ldo) = u in its natural column order, out (M, H, row
     *               stride ldo) = projected * silu(gate).  N % 32 == 0.
     *   aux_mode 4: SwishGLU backward on the input-gradient product of the Linear that FOLLOWS it (N = H columns of
     *               d_out): aux = u (M, 2H, row stride ldo), out (M, 2H, row stride ldo) = [value * silu(gate) |
     *               value * projected * silu'(gate)].                                                              */
    const float *aux;
    int32_t aux_mode;
    /* merge-on-read (consumer side of mdt_op_mlp): a_parts >= 2 means the activation rows are the SUM of a_parts arrays
     * A, A + a_part_stride, ... (floats; same lda), added in that fixed order -- the partial slabs a fused MLP launch left;
     * needs the LayerNorm prologue (whole rows per wave) and the wide tiles (N >= 1024, M > 1400 rows).  a_merged (optional,
     * may not alias any part): the summed rows are also written there (row stride lda) by the column-0 tiles, so that
     * the next residual GEMM finds the residual stream in one place.  0 / 1 = plain A.                              */
    int32_t a_parts;
    int64_t a_part_stride;
    float *a_merged;
    /* optional (round 6): the three-way bf16 split image of the same weight (mdt_op_pack_weight_split; rows in the order of Wp's).
     * Where it is given, the LayerNorm-prologue products on the wide tiles (K = 384 or 512, N a multiple of 384, from 768 rows on,
     * plain output rows) multiply in the split form -- six bf16 MFMA products per 32-deep step, fp32
     * accumulation: fp32's product accuracy, not the fp32 form's bits -- unless mdt_op_set_mlp_split(0).  NULL: the fp32 form. */
    const void *Wp_split;
    /* optional: the fp16 pair image of the same weight (mdt_op_pack_weight_pair).  Takes the same products as Wp_split (which wins
     * where both are given) through the two-way fp16 pair split described at mdt_op_pack_weight_pair. */
    const void *Wp_pair;
} mdt_gemm_args;

mdt_status mdt_op_gemm(const mdt_gemm_args *args, void *stream);

/* The whole MLP sublayer of a (Conditioned)Block as ONE launch (transformer_blocks.py:160-181, 296-309):
 *     x + gate * ( act( prologue(x) @ W1^T + b1 ) @ W2^T + b2 )
 * `fc` describes the first Linear as for mdt_op_gemm (A = x rows with lda, M, K = D, N = 4D, LayerNorm (+ modulate)
 * prologue, act; `out` ignored), `proj` the second (Wp, bias, N = D, K = 4D, mod / mod_stride / gate_off /
 * rows_per_sample for the gate; A / out ignored).  A workgroup owns 32 rows and ONE 512-wide slice of the hidden layer:
 * it keeps its (32 x 512) slice of act(.) in LDS and multiplies it by the matching K-slice of W2, so the hidden layer never
 * reaches memory and the S = 4D / 512 slices of a row tile produce S partial slabs
 *     parts[0] = x + gate * (h_0 W2_0^T + b2),   parts[s] = gate * (h_s W2_s^T)        (slab s at parts + s * part_stride)
 * whose sum IN THE ORDER 0, 1, .., S-1 is the sublayer's output (deterministic: no atomics).  The consumer adds them on
 * read (mdt_gemm_args.a_parts, mdt_head_args.y_parts).  *n_parts returns S.  Needs D a multiple of 128, D <= 512, and
 * parts (S * part_stride floats, part_stride >= M * D) not aliasing x -- except S == 1, where parts may be x itself. */
mdt_status mdt_op_mlp(const mdt_gemm_args *fc, const mdt_gemm_args *proj, float *parts, int64_t part_stride,
                      int32_t *n_parts, void *stream);
/* The same launch with every contraction as a THREE-WAY bf16 SPLIT (round 6): each fp32 operand as three bf16 parts, six
 * v_mfma_f32_16x16x32_bf16 products per 32-deep step, fp32 accumulation -- fp32's product accuracy (not the bits of mdt_op_mlp) at a
 * third of its matrix-pipe time.  fc_split / proj_split: images of the two weights made by mdt_op_pack_weight_split ((4 D, D) and
 * (D, 4 D) row-major sources; 6 bytes per weight); fc->Wp / proj->Wp are not read.  The model-level entry points use it
 * from the row count of mdt_op_set_mlp_fuse_min on unless mdt_op_set_mlp_split(0) / MDT_HIP_MLP_SPLIT=0 (negative: default). */
mdt_status mdt_op_pack_weight_split(const float *w, int64_t n_rows, int64_t K, void *image, void *stream);
/* ... rows [n_off, n_off + n_rows) of a taller image (stacked weights: query | key | value); n_off a multiple of 16 */
mdt_status mdt_op_pack_weight_split_rows(const float *w, int64_t n_rows, int64_t K, void *image, int64_t n_off, void *stream);
mdt_status mdt_op_mlp_split(const mdt_gemm_args *fc, const mdt_gemm_args *proj, const void *fc_split, const void *proj_split,
                            float *parts, int64_t part_stride, int32_t *n_parts, void *stream);

/* The same launches in the two-way fp16 PAIR split -- the form the model's own launches take from 768 rows on (the three-way bf16
 * entries above keep their behaviour bit for bit).
 * Numerics.  An operand element x of a scale group is stored as h1 + h2 = x s:  h1 = fp16(x s), h2 = fp16(x s - h1), both rounded to
 * nearest (the subtraction is exact in fp32) -- 22 significand bits.  s is a power of two that brings the group's largest |x| into
 * [2^14, 2^15) (exponent clamped to +-126; a zero group gets 2^126), below fp16's 65504 with room for rounding, so no finite fp32
 * operand -- a hidden activation above 65504, an all-zero row or tile, a tile of fp32 subnormals -- turns into Inf or NaN.  Groups: one
 * scale per activation ROW (computed in the launch: the LayerNorm prologue's rows, the GELU epilogue's 512-wide hidden slices) and
 * one per 16-row TILE of the (N, K) weight (= one MFMA column tile; made by the pack kernel, no global reduction).  A k32 step is
 * three v_mfma_f32_16x16x32_f16 products, x2 w1, x1 w2, x1 w1, fp32 accumulation; the epilogue multiplies each accumulator by the
 * exact reciprocal of (row scale x tile scale) (one v_ldexp_f32) before bias, activation and gate.  Elements more than 2^-14 below
 * their group's maximum lose low bits of h2 to fp16's subnormal range -- below 2^-28 of the maximum, whether or not the MFMA keeps
 * fp16 subnormals.  A row or tile that holds Inf or NaN gets a NaN scale: the outputs that depend on it are NaN, no others.
 * Against float64 the error stays within 1.5x the fp32 launches' (tests/test_gpu_f16_pair.py); not their bits.
 * Image of an (N, K) weight, N % 16 == 0, K % 32 == 0: column tile nt at nt * (K / 32 * 2048 + 16) bytes = K / 32 steps x 2 parts x
 * 1 KiB fragments (step kk, part p at (2 kk + p) * 1024; lane l's 16 bytes = the part's eight fp16 of
 * W[16 nt + l % 16][32 kk + 16 h + 4 (l / 16) + e] at slot 4 h + e), then a 16-byte trailer {fp32 s, 0, 0, 0}.
 * mdt_op_pair_image_bytes = 4 N K + N bytes (-1: bad shape).
 * mdt_op_pack_weight_pair: rows [0, n_rows) of w (n_rows, K) -> column tiles n_off / 16 .. of the image (n_rows, n_off multiples of
 * 16: stacked weights are packed row range by row range).  mdt_op_pair_from_packed: the same image, bit for bit, from the fp32
 * fragment image of the whole weight (mdt_op_pack_weight).
 * mdt_op_mlp_pair: mdt_op_mlp_split on pair images.  mdt_op_gemm_ln_pair: the wide LayerNorm-prologue product on args->Wp_pair
 * (K = 384 or 512, N a multiple of 384, plain output rows, a_parts <= 4; Wp is not read) at ANY row count and whatever the
 * switches say; mdt_op_gemm takes the same launch from 768 rows on where Wp_pair is given and Wp_split is not. */
int64_t mdt_op_pair_image_bytes(int64_t n_rows, int64_t K);
mdt_status mdt_op_pack_weight_pair(const float *w, int64_t n_rows, int64_t K, void *image, int64_t n_off, void *stream);
mdt_status mdt_op_pair_from_packed(const float *packed, int64_t N, int64_t K, void *image, void *stream);
mdt_status mdt_op_mlp_pair(const mdt_gemm_args *fc, const mdt_gemm_args *proj, const void *fc_pair, const void *proj_pair,
                           float *parts, int64_t part_stride, int32_t *n_parts, void *stream);
mdt_status mdt_op_gemm_ln_pair(const mdt_gemm_args *args, void *stream);

/* From 8192 rows on, mdt_op_gemm's K = 384 products that take the weight-stationary body run the same three-way bf16 split form
 * (fp32's product accuracy, not its bits, at 2.7x the fp32 matrix rate) unless MDT_HIP_WS_SPLIT=0.
 * The process-global hooks that switch these launches between their forms -- mdt_op_set_mlp_split, mdt_op_set_mlp_fuse_min,
 * mdt_op_set_side_jobs, mdt_op_set_ws_split, mdt_op_set_mlp_skew, mdt_op_set_gemm_geometry -- and the measurement hooks
 * mdt_op_trace_mlp* / mdt_op_clock_stamp are test and measurement tools, not part of this boundary: mdt_hip_debug.h. */

typedef struct {
    const float *q; int64_t ldq;       /* (B*Tq, >= H*hd) query rows                                  */
    const float *k; const float *v;    /* (B*Tk, ...) key / value rows                                */
    int64_t ldkv;
    float *out; int64_t ldo;           /* (B*Tq, H*hd)                                                */
    int32_t B, H, hd, Tq, Tk;          /* hd in {16,32,48,64}; Tq, Tk <= 16, or <= 64 at hd >= 32     */
    int32_t causal;                    /* 1: key j visible to query i iff j <= i (top-left aligned)   */
    int32_t rope;                      /* 1: rotate q by its position 0..Tq-1 and k by 0..Tk-1        */
} mdt_attn_args;

mdt_status mdt_op_attention(const mdt_attn_args *args, void *stream);

/* One sample's self-attention fused into its output projection (the rollout batch B = 1, where every launch is
 * latency): out (+)= gate * (softmax(q k^T / sqrt(hd)) v @ W^T + bias) for the T <= 16 rows of qkv (T, 3*K), q | k | v
 * column blocks of K = 8 * hd each.  `proj` describes the projection as for mdt_op_gemm (A is ignored, M = T; bias /
 * residual / gate as there; no LayerNorm prologue, activation or row remap).  8 heads, hd in {16,32,48,64}, no RoPE.
 * Replaces Attention.forward's SDPA + c_proj (transformer_blocks.py:142-157) for one sample.
 * Summation order: since round 5 both attention products run on the MFMA pipe inside this launch (wave = head, k order of the
 * matrix instruction), so its results differ from mdt_op_attention + mdt_op_gemm on the same operands in the last bits: within
 * 2e-5 absolute + 1e-4 relative on values of order one (tests/test_gpu_ops.py::test_fused_attention_projection_against_the_two_
 * launches_at_rollout_batches, B = 1 .. 8); the model-level entry points use it up to 32 samples. */
mdt_status mdt_op_attn_proj(const mdt_gemm_args *proj, const float *qkv, int64_t ldq, int32_t hd, int32_t T, int32_t causal,
                            void *stream);
/* (More than 64 samples: the same contract for a LARGE batch, M = samples * T rows, causal, residual, hd in {16, 32, 48} --
 * the attention of each 32-row tile is computed in the prologue of the tiled projection GEMM, k_attn_proj_wide; the
 * model-level entry points use it from 1401 rows on -- mdt_op_set_attn_wide_min, mdt_hip_debug.h.) */

mdt_status mdt_op_layernorm(const float *in, const float *w, const float *b, float *out, int64_t M, int32_t D,
                            void *stream);

typedef struct {
    const float *y;            /* (M, D) decoder residual stream                                      */
    const float *ln_w;         /* decoder.ln.weight (D), ln_b optional                                */
    const float *ln_b;
    const float *Wp, *bp;      /* action_pred.weight (A, D) row-major UNPACKED, bias (A); A <= 64     */
    const float *x;            /* (M, A) current noisy actions                                        */
    const float *sigma;        /* sigma of sample b at sigma[b * sigma_stride]                        */
    int64_t sigma_stride;
    float *out;                /* (M, A)                                                              */
    int32_t M, D, A, rows_per_sample;
    int32_t mode;              /* MDT_HEAD_*                                                          */
    const float *step;         /* DDIM: device {ratio, coef, sigma_next}                              */
    float sigma_data;
    /* optional fused embedding of the NEXT step's input: y_next = (out * c_in(sigma_next)) Wa^T + ba */
    float *y_next;             /* NULL or (M, D) (may alias y)                                        */
    const float *Wa, *ba;      /* action_emb.weight TRANSPOSED to (A, D) row-major, bias (D)          */
    int32_t no_ln;             /* 1: y is used as it is (the MLP head's hidden layer), ln_w / ln_b only have to be
                                * readable for D floats                                                */
    int32_t y_parts;           /* >= 2 (A <= 8 only): the rows are the sum of y_parts arrays y, y + y_part_stride, ... (the slabs */
    int64_t y_part_stride;     /* mdt_op_mlp left), added in that order; 0 / 1 = plain y                             */
} mdt_head_args;

/* A <= 16: one wave per row (A <= 8 and A > 8 instantiations).  17 <= A <= 64: one workgroup per 16 rows, both products as
 * 16 x 16 tiles of v_mfma_f32_16x16x4_f32 (the same modes and operands; dynamic LDS 4 (16 (ceil16(D) + 4) + 16 (ceil16(A) + 4))
 * bytes).  D % 4 == 0, D <= 512. */
mdt_status mdt_op_head(const mdt_head_args *args, void *stream);

/* Collapsed cross-attention (see mdt_kernels.hip): fold the sigma-independent context K|V into the query and
 * output projections once per sampler call ... */
typedef struct {
    const float *kv; int64_t ldkv; /* (B*Te, ...) rows holding K at column 0 and V at column D of this block   */
    const float *WqT_p;            /* fragment image of cross_att.query.weight TRANSPOSED: mdt_op_pack_weight_t(Wq, D, D, D, .., 0, D / 16) */
    const float *bq;               /* cross_att.query.bias (D)                                                 */
    const float *Wo_p;             /* fragment image of cross_att.c_proj.weight: mdt_op_pack_weight(Wo, D, D, .., 0)               */
    float *U, *Wf;                 /* out: B images of 4 H * D floats each, opaque: MFMA weight-fragment order, every head */
                                   /* padded to 4 context tokens (row p = 4 h + j; mdt_kernels.hip "Collapsed ...")        */
    float *c;                      /* out: (B, 4 H)                                                                        */
    int32_t B, H, hd, D, Te;       /* H in {4, 8}, hd in {16, 32, 48, 64}, D = H * hd a multiple of 128, 1 <= Te <= 4      */
} mdt_xfold_args;
mdt_status mdt_op_xattn_fold(const mdt_xfold_args *args, void *stream);

/* ... and apply the whole sublayer  y += c_proj(softmax_causal(q K^T / sqrt(hd)) V) + bo  per denoising step. */
typedef struct {
    float *y;                      /* (B*Ta, D) residual stream, updated in place                              */
    const float *ln_w, *ln_b;      /* ln3 weight / bias (D)                                                    */
    const float *U, *Wf, *c;       /* from mdt_op_xattn_fold                                                   */
    const float *bo;               /* cross_att.c_proj.bias (D) or NULL                                        */
    int32_t B, H, D, Te, Ta;       /* D a multiple of 128, Ta <= 16                                             */
    float *y_out;                  /* NULL: y is updated in place; else the new rows go here and y stays as it is */
} mdt_xapply_args;
mdt_status mdt_op_xattn_apply(const mdt_xapply_args *args, void *stream);

/* Rollout batches: mdt_op_xattn_apply and the LayerNorm(+ modulate)-prologue Linear that follows it on the same rows (mlp.c_fc,
 * transformer_blocks.py:301-307) in ONE launch (k_xattn_gemm_smallm): every 16-column workgroup of the Linear repeats the
 * sample's cross-attention on the MFMA pipe and multiplies its output rows straight out of LDS; the workgroup of column 0
 * writes the new rows to x->y_out, which must be given and differ from x->y (the other workgroups may still be reading x->y).
 * `g` as for mdt_op_gemm with g->A == x->y, lda = K = x->D, M = x->B * x->Ta, rows_per_sample = x->Ta, no residual / row remap /
 * split input.  Results equal the two launches bit for bit.  The model-level entry points use it up
 * to 2 samples (B = 4 measured slower: 1.67 vs 1.58 ms per call). */
mdt_status mdt_op_xattn_gemm(const mdt_xapply_args *x, const mdt_gemm_args *g, void *stream);

/* The middle of a ConditionedBlock for a batch of at most one sample per compute unit, ONE launch, one workgroup per sample
 * (k_attn_xattn): mdt_op_attn_proj's contract (causal self-attention of the sample's T rows -> c_proj + gate + residual,
 * transformer_blocks.py:296-300) followed by mdt_op_xattn_apply's on the same rows (:301-305); the rows between the two
 * sublayers stay in the workgroup's LDS and x->y == proj->out is written once.  8 heads of 48 (K = N = ldo = 384, ldq = 3 K),
 * T = x->Ta <= 16, proj->M = x->B * T; results equal the two launches up to the summation order of the self-attention
 * (this form runs q k^T and P v on the MFMA pipe, one wave per head).  The model-level entry points use it
 * from 200 rows up to 512 samples (mdt_op_set_attn_wide_min(0) switches it off together with the tiled form). */
mdt_status mdt_op_attn_xattn(const mdt_gemm_args *proj, const float *qkv, int64_t ldq, const mdt_xapply_args *x, int32_t hd,
                             int32_t T, void *stream);

/* The same launch with the output projection on fp16 pair splits: proj->Wp_pair (required; proj->Wp is ignored) is the image
 * mdt_op_pack_weight_pair makes of c_proj.weight (mdt_op_pair_image_bytes(384, 384) bytes, 16-byte aligned).  The attention output
 * gets one power-of-two scale per row and is multiplied as two fp16 parts, three v_mfma_f32_16x16x32_f16 per 32 columns of K
 * instead of eight v_mfma_f32_16x16x4_f32; everything behind the projection is mdt_op_attn_xattn's.  fp32-grade results, not
 * its bits.  An Inf / NaN in a sample's attention output reaches that sample's rows only.  The model-level entry points use it
 * from 768 rows on (mdt_op_set_mlp_split(0) restores the fp32 launch). */
mdt_status mdt_op_attn_xattn_pair(const mdt_gemm_args *proj, const float *qkv, int64_t ldq, const mdt_xapply_args *x, int32_t hd,
                                  int32_t T, void *stream);

/* y = (x * c_in(sigma)) Wa^T + ba   (c_in omitted when sigma == NULL); WaT = action_emb.weight transposed to (A, D) */
mdt_status mdt_op_action_embed(const float *x, const float *sigma, int64_t sigma_stride, float sigma_data,
                               const float *WaT, const float *ba, float *y, int64_t M, int32_t A, int32_t D,
                               int32_t rows_per_sample, void *stream);

#ifdef __cplusplus
}
#endif
#endif
