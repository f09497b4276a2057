/*
 * mdt_map_pool.h -- C ABI of the attention-pooling head the contrastive (CLA) auxiliary loss hangs on the denoiser's
 * context tokens: MAPBlock, the `latent_proj` of ClipStyleProjection('map').
 * Same library (libmdt_hip.so), same conventions as mdt_hip.h: fp32, row-major, 16-byte aligned device pointers,
 * work enqueued on the caller's HIP stream, mdt_status + mdt_last_error().
 *
 * Reference interface replaced (paths relative to the reference checkout):
 *   mdt/models/networks/transformers/transformer_blocks.py:746-791  MAPBlock.__init__/forward
 *   mdt/models/networks/transformers/transformer_blocks.py:716-743  MAPAttention
 *   mdt/models/networks/transformers/transformer_blocks.py:42-62    RMSNorm, SwishGLU
 *   call sites: transformer_blocks.py:833-870 (ClipStyleProjection), mdt/models/mdtv_agent.py:133-138 (construction,
 *   clip_style='map'), :440-484 (compute_contrastive_loss: clip_proj on latent_encoder_emb of both modalities)
 */
#ifndef MDT_MAP_POOL_H
#define MDT_MAP_POOL_H

#include <stdint.h>

#include "mdt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdt_map_pool mdt_map_pool; /* opaque */

/* Constructor arguments of MAPBlock (transformer_blocks.py:747-756) with do_rms_norm = do_swish_glu = True (the
 * defaults, the only form the reference constructs).  The reference's MAPBlock runs its attention with
 * 2 * n_heads heads (:759); n_heads below is the CONSTRUCTOR argument (8 in ClipStyleProjection). */
typedef struct {
    int32_t n_latents;   /* learnt seed vectors = output rows per sample; 1 (ClipStyleProjection) .. 16 */
    int32_t embed_dim;   /* width of the pooled tokens (input of `projection`); multiple of 16            */
    int32_t output_dim;  /* width of everything after `projection`; multiple of 16, <= 512               */
    int32_t n_heads;     /* constructor argument; the attention uses 2 * n_heads heads                   */
    int32_t mlp_hidden;  /* int(mlp_ratio * output_dim); multiple of 16                                  */
} mdt_map_pool_config;

/* Parameters by their MAPBlock state_dict names: "latents", "projection.weight|bias", "attn_norm.g",
 * "attn.q.weight", "attn.kv.weight", "attn.proj.weight|bias", "mlp_norm.g", "mlp.0.project.weight|bias",
 * "mlp.1.weight|bias" (registration order of the reference module). */
mdt_status mdt_map_pool_create(const mdt_map_pool_config *cfg, mdt_map_pool **out);
mdt_status mdt_map_pool_destroy(mdt_map_pool *p);
int64_t mdt_map_pool_param_count(const mdt_map_pool *p);
const char *mdt_map_pool_param_name(const mdt_map_pool *p, int64_t i);
int64_t mdt_map_pool_param_numel(const mdt_map_pool *p, int64_t i);
mdt_status mdt_map_pool_load_param(mdt_map_pool *p, const char *name, const float *src, int64_t numel, void *stream);

/* MAPBlock.forward(x) (transformer_blocks.py:787-791):
 *   x   : (B, N, embed_dim) tokens to pool, 1 <= N <= 64 (the denoiser's own context limit); N < 1 or N > 64 returns
 *         MDT_ERR_UNSUPPORTED ("1..64 tokens per sample") before anything is enqueued
 *   out : (B, n_latents, output_dim)   (the reference squeezes dim 1 when n_latents == 1: same memory)
 *
 * The attention is one of two kernel pairs, chosen by the token count alone.  With Q = n_latents, D = output_dim,
 * H = 2 * n_heads, hd = D / H:
 *
 * N <= 16: one workgroup per sample with the sample's queries, keys, values and scores in LDS, within a 64 KiB budget.  Bytes:
 *   inference (mdt_map_pool_forward)       : 4 * (Q*D + 2*N*D + Q*H*N)        q, k|v, scores
 *   training  (mdt_map_pool_forward_train) : 4 * (2*Q*D + 2*N*D + 2*Q*H*N)    + dO and dS for the backward
 * A call whose budget exceeds 65536 bytes returns MDT_ERR_UNSUPPORTED ("LDS budget") before anything is enqueued.  The training
 * budget is the larger one, so at N <= 16 a shape can be ACCEPTED FOR INFERENCE AND REFUSED FOR TRAINING.  Example: n_latents 16,
 * output_dim 256, n_heads 8, N = 16 needs exactly 65536 bytes for inference (accepted) and 98304 for training
 * (refused); n_latents 16, output_dim 512, N = 16 is refused for both.  ClipStyleProjection's shape (one latent, 384
 * channels, n_heads 8) fits with 16 tokens in both: 51712 and 54272 bytes.
 *
 * N 17..64: one workgroup per (sample, group of hg heads), which holds only the W = hg * hd channels of its heads and stages
 * the K slice and the V slice of the sample one after the other in the same LDS rows:
 *   hg = the largest divisor of H with hg <= 8 and hg * hd <= 128 (1 when there is none: hd > 64)
 *   W  = hg * hd,   Wp = W | 1 (the staged rows have an odd stride)
 *   inference : 4 * (Q*W + N*Wp + Q*hg*N)        q, K then V, scores
 *   training  : 4 * (2*Q*W + N*Wp + 2*Q*hg*N)    + dO and dS for the backward
 * The largest workgroups any accepted handle can ask for, at Q 16 and N 64: the widest single head, hd 256 (512 channels,
 * n_heads 1), takes 86272 and 106752 bytes; eight heads of 16 (W = 128) take 73984 and 114944, the maximum of the rule.  All
 * are inside the 160 KiB of a CU, so NOTHING IS REFUSED for LDS above 16 tokens, for inference or for training; the
 * shipped head at 34 tokens takes 14120 / 15048 bytes.  The rule above 16 tokens is therefore the laxer one: 16 latents x 512
 * channels is refused at 16 tokens and accepted at 17.  (Retiring the <= 16-token pair would lift that; its bits and its
 * refusals are pinned by tests.)  mdt_op_map_attn_lds (mdt_hip_debug.h) returns the second rule's bytes. */
mdt_status mdt_map_pool_forward(mdt_map_pool *p, const float *x, int64_t batch, int32_t n_tokens, float *out,
                                void *stream);

/* ---- training ----
 * mdt_map_pool_train_prepare allocates the transposed weight images; parameters must be uploaded again after it.
 * Gradients come back in one flat buffer: parameter i at [mdt_map_pool_grad_offset(i), + numel), reference layout.
 * Several tapes may be alive (the agent pools the language and the vision context before one backward);
 * mdt_map_pool_backward ACCUMULATES into `grads` and optionally returns d(x). */
mdt_status mdt_map_pool_train_prepare(mdt_map_pool *p);
int64_t mdt_map_pool_grad_numel(const mdt_map_pool *p);
int64_t mdt_map_pool_grad_offset(const mdt_map_pool *p, int64_t i);
mdt_status mdt_map_pool_forward_train(mdt_map_pool *p, const float *x, int64_t batch, int32_t n_tokens, float *out,
                                      int32_t *tape, void *stream);
mdt_status mdt_map_pool_backward(mdt_map_pool *p, int32_t tape, const float *g_out, float *grads, float *d_x,
                                 void *stream);
mdt_status mdt_map_pool_tape_release(mdt_map_pool *p, int32_t tape);

/* ---- loss: InfoNCE between the pooled embeddings ----
 * MDTVAgent.clip_auxiliary_loss(image_features, lang_features, mode) (mdt/models/mdtv_agent.py:774-799): both sets
 * L2-normalised, S = exp(logit_scale) * img @ lang^T, cross entropy against the diagonal over the rows
 * (img_to_text), the columns (text_to_img) or the mean of both (symmetric).  Value and -- when the three gradient
 * pointers are given -- dL/d(image_features), dL/d(lang_features), dL/d(logit_scale) in the same enqueue. */
enum { MDT_INFONCE_SYMMETRIC = 0, MDT_INFONCE_IMG_TO_TEXT = 1, MDT_INFONCE_TEXT_TO_IMG = 2 };
typedef struct {
    const float *image_features;  /* (batch, dim)                                                   */
    const float *lang_features;   /* (batch, dim)                                                   */
    const float *logit_scale;     /* device scalar: the log temperature parameter (mdtv_agent.py:140) */
    int32_t batch, dim;           /* dim: multiple of 16, at most 65536; batch 1..32768 (the GLOBAL batch after the gather);
                                   * ceil16(batch) * dim < 2^30.  Anything else: MDT_ERR_UNSUPPORTED / MDT_ERR_INVALID_ARG
                                   * before anything is enqueued */
    int32_t mode;                 /* MDT_INFONCE_*                                                    */
    float *loss;                  /* device scalar out                                                */
    float *d_image, *d_lang;      /* (batch, dim) out, or all three NULL                              */
    float *d_logit_scale;         /* device scalar out                                                */
    float *scratch;               /* mdt_op_infonce_scratch(batch, dim) floats                        */
} mdt_infonce_args;
int64_t mdt_op_infonce_scratch(int64_t batch, int64_t dim);
mdt_status mdt_op_infonce(const mdt_infonce_args *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MDT_MAP_POOL_H */
