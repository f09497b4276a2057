/*
 * mdt_hip.h -- C ABI of libmdt_hip.so: the MI355X (gfx950) implementation of MDT's diffusion-transformer
 * action-denoising hot path (EDM-preconditioned score network + multi-step sampler loop).
 *
 * The reference (intuitive-robots/mdt_policy) is pure Python and has NO FFI boundary for this path; the
 * operator API the path sits behind is Python.  Each entry point below therefore cites
 * the reference Python call it stands under; the Python facade in mdt_policy_amd/models/ presents the
 * reference's own class / function signatures on top of this ABI (binding shown in INTEGRATION.md).
 *
 * Conventions
 *   - C linkage, POD arguments only: raw pointers, int64 sizes, an opaque handle, a hipStream_t passed
 *     as void*.  No exceptions cross the boundary: every call returns an mdt_status; the message of the
 *     last failure on the calling thread is available from mdt_last_error().
 *   - All tensors are fp32, row-major, contiguous, batch-major (B, T, C); data pointers are DEVICE
 *     pointers on the handle's device and must be 16-byte aligned, except where marked "host".
 *   - All work is enqueued on the caller's stream (e.g. torch.cuda.current_stream().cuda_stream on
 *     PyTorch-ROCm); nothing synchronises the device except mdt_reserve()/first-use workspace growth,
 *     which may call hipMalloc.  Inputs are caller-owned and never written; outputs are caller-owned.
 *   - A handle is bound to one device and is not thread-safe (one handle per GPU / per process rank).
 */
#ifndef MDT_HIP_H
#define MDT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mdt_model mdt_model; /* opaque */

typedef enum {
    MDT_OK = 0,
    MDT_ERR_INVALID_ARG = 1,   /* bad pointer / size / alignment / unknown parameter name            */
    MDT_ERR_UNSUPPORTED = 2,   /* configuration outside what the HIP path implements (stated in msg) */
    MDT_ERR_NOT_LOADED = 3,    /* a parameter needed by the call was never loaded                    */
    MDT_ERR_HIP = 4,           /* a HIP runtime call failed (message carries hipGetErrorString)      */
    MDT_ERR_STATE = 5,         /* call sequence error, e.g. mdt_denoise_cached() without mdt_encode()  */
    MDT_ERR_NUMERIC = 6        /* an adaptive sampler stopped: NaN error or step size, or a step that no longer moves */
} mdt_status;

enum { MDT_ARCH_MDTV = 0, MDT_ARCH_MDT = 1 };
enum { MDT_MODALITY_VIS = 0, MDT_MODALITY_LANG = 1 };

/*
 * Constructor fields of the score network.  Mirrors the Hydra kwargs of
 *   mdt.models.networks.mdtv_transformer.MDTVTransformer.__init__  (reference mdtv_transformer.py:38-68,
 *   conf/model/model/mdtv_transformer.yaml:6-35) and
 *   mdt.models.networks.mdt_transformer.MDTTransformer.__init__    (reference mdt_transformer.py:39-68),
 * plus GCDenoiser's sigma_data (reference score_wrappers.py:26-29).  Dropout probabilities are not part
 * of the ABI: this path is the eval-mode forward.
 */
typedef struct {
    int32_t arch;                 /* MDT_ARCH_MDTV | MDT_ARCH_MDT                                   */
    int32_t embed_dim;            /* d; multiple of 16, <= 512                                      */
    int32_t n_heads;              /* head dim d/n_heads in {16,32,48,64}                            */
    int32_t n_enc_layers;
    int32_t n_dec_layers;
    int32_t action_dim;           /* 1..64 (17..64: the tiled action head and narrow gradients)     */
    int32_t obs_dim;              /* multiple of 16                                                 */
    int32_t goal_dim;             /* multiple of 16                                                 */
    int32_t n_obs_token;          /* MDT-V: state tokens per sample (3); MDT: ignored (static+gripper).  The context is
                                   * [sigma token] + goal_seq_len + n_obs_token + [proprio token]: 1..16 tokens, 17..64 at
                                   * head dim 32 / 48 / 64 */
    int32_t goal_seq_len;         /* G >= 1: goal tokens per sample.  Every `goal` argument is (B, G, goal_dim); the G rows
                                   * are embedded row by row and enter the context in order, bounded by the context rule
                                   * above.  MDT with use_abs_pos_emb: goal token j adds pos_emb[:, j], the state rows
                                   * pos_emb[:, G] */
    int32_t action_seq_len;       /* Ta <= 16; 17..64 at head dim 32 / 48 / 64                      */
    int32_t use_mlp_goal;         /* goal_emb / lang_emb are Linear-GELU-Linear                     */
    int32_t use_modality_encoder; /* separate lang_emb                                              */
    int32_t use_abs_pos_emb;      /* MDT only: pos_emb added to the encoder tokens                  */
    int32_t use_rot_embed;        /* RoPE on q/k (rot dim 32, theta 1e4), position_embeddings.py:83 */
    int32_t use_ada_conditioning; /* 1: sigma conditions the decoder blocks (adaLN-Zero, shipped configs);
                                     0: sigma embedding is the first ENCODER token, plain Block decoder
                                        (mdtv_transformer.py:296-297, transformer_blocks.py:460-506)  */
    int32_t use_noise_encoder;    /* with use_ada_conditioning: NoiseBlock (ln(x)+c) instead of
                                     ConditionedBlock (transformer_blocks.py:312-341, :533-544)      */
    int32_t linear_output;        /* 1: action_pred = Linear(d, A); 0: Linear(d, h) -> GELU -> Linear(h, A), h = 100
                                   * (MDTV, mdtv_transformer.py:178-185) / h = d (MDT, mdt_transformer.py:170-177) */
    int32_t bias;                 /* reference 'bias' flag: biases on c_proj / MLP / LayerNorms     */
    float   sigma_data;           /* GCDenoiser.sigma_data                                          */
    int32_t no_goal_conditioning; /* 1: constructor kwarg goal_conditioned=False.  MDTV: the goal rows FOLLOW the
                                     state tokens (mdtv_transformer.py:284-299); MDT: no goal rows at all, which
                                     the reference can only run with use_ada_conditioning=0 (mdt_transformer.py:326-334) */
    int32_t proprio_dim;          /* MDT-V: width of state['state_obs'] (1..16; conf/model/model/mdtv_transformer.yaml:11) */
    int32_t use_proprio;          /* MDT-V: 1 = every call carries state['state_obs'] (B, 1, proprio_dim), passed as
                                     `tokens2`: proprio_emb (Linear(p, 2d), Mish, Linear(2d, d)) embeds it into one
                                     more context token BEHIND the state tokens, and a goal_conditioned=False model
                                     then has no goal token at all (mdtv_transformer.py:260-266, 284-299).  The
                                     reference decides per call ('state_obs' in states); a handle is built for one
                                     of the two context layouts, the facade keeps one handle per layout.          */
} mdt_config;

/* Human-readable message of the last failing call on this thread ("" if none). */
const char *mdt_last_error(void);

/* Library version string and the offload architecture it was compiled for ("gfx950"). */
const char *mdt_version(void);

/* hydra.utils.instantiate(cfg.model) -> GCDenoiser.__init__ -> MDTVTransformer.__init__
 * (reference score_wrappers.py:26-29, mdtv_transformer.py:38-195).  Allocates the packed weight arena on
 * the current HIP device.  Parameters start unloaded. */
mdt_status mdt_create(const mdt_config *cfg, mdt_model **out);
mdt_status mdt_destroy(mdt_model *m);

/* Enumeration of the parameters the forward path READS, in the reference's state_dict order (the
 * checkpoint / positional-EMA contract, reference mdt/evaluation/utils.py:92-103).  Names are GCDenoiser
 * state_dict keys ("inner_model.…").  Parameters the reference carries but never reads on this path
 * (pos_emb in MDT-V, proprio_emb.* unless use_proprio, *.rotary_pos_emb.freqs; reference mdtv_transformer.py:105,160-164,
 * 260-266) are not enumerated; mdt_load_param() accepts and ignores them. */
int64_t     mdt_param_count(const mdt_model *m);
const char *mdt_param_name(const mdt_model *m, int64_t index);
int64_t     mdt_param_numel(const mdt_model *m, int64_t index);

/* load_state_dict / optimizer step: copy one fp32 parameter (reference layout, e.g. Linear weight
 * (out,in) row-major) from `src` (host OR device pointer) into the library's MFMA-fragment-packed
 * arena.  Stream-ordered on `stream`; a host `src` must stay valid until the stream has passed. */
mdt_status mdt_load_param(mdt_model *m, const char *name, const float *src, int64_t numel, void *stream);

/* The same for n parameters at once -- a whole load_state_dict, or the re-upload of every parameter an optimizer step
 * changed -- as ONE kernel launch for all device-resident sources (host sources take the mdt_load_param path).  A
 * training loop calls this once per step. */
mdt_status mdt_load_params(mdt_model *m, int32_t n, const char *const *names, const float *const *srcs,
                           const int64_t *numels, void *stream);

/* Pre-size the workspace for batches up to max_batch (avoids hipMalloc later, e.g. before graph capture).  A sampler call needs
 * its decoder samples: batch, 2 * batch when guided; a *_multi call (below) batch * candidates chunks, 2 * batch * candidates when
 * guided -- reserve that before capturing one. */
mdt_status mdt_reserve(mdt_model *m, int64_t max_batch);

/* Number of times the workspace was (re)allocated.  A captured HIP graph of a sampler call holds workspace addresses: it
 * stays valid while this number does not change (mdt_reserve the largest batch first, capture afterwards).  It also moves when a
 * parameter load during training leaves the bf16 split weight images of the large-batch launches stale (round 6): a graph captured
 * before that would replay those launches without the refresh they need. */
int64_t mdt_ws_generation(const mdt_model *m);

/* inner_model.forward_enc_only(state, action, goal, sigma)
 * (reference mdtv_transformer.py:213-222; mdt_transformer.py:211-229 / :257-281): goal/state token
 * embedding, n_enc_layers Blocks, final LayerNorm.  Also projects the per-decoder-block cross-attention
 * K/V once and keeps ctx + K/V cached in the handle for mdt_denoise_cached()/samplers.
 *   sigma  : (B,) device.  Read only when use_ada_conditioning == 0 (the sigma embedding is then the first
 *            context token, so the cached context is only valid for that sigma); may be NULL otherwise.
 *   tokens : MDT-V state['state_images'] (B, n_obs_token, obs_dim); MDT state['static'] (B,1,obs_dim)
 *   tokens2: MDT state['gripper'] (B,1,obs_dim); MDT-V: state['state_obs'] (B,1,proprio_dim) when the handle was
 *            created with use_proprio, else NULL
 *   goal   : (B, goal_seq_len, goal_dim) -- here and in every entry point below that takes a goal
 *   honour_modality: 1 = pick lang_emb when modality==LANG (MDT-V always; MDT forward_enc_only),
 *                    0 = always goal_emb (MDT.forward -> enc_only_forward, mdt_transformer.py:215)
 *   ctx_out: (B, Te, d) or NULL -- the value the reference caches as inner_model.latent_encoder_emb
 * Te = [sigma token] + goal_seq_len goal rows + state tokens + [proprio token] <= 64 (above 16: head dim 32 / 48 / 64).  The decoder's
 * cross-attention is causal on its Ta x Te score matrix, top-left aligned: query row t sees context rows j <= t, so rows
 * j >= Ta reach the decoder only through the encoder's self-attention (as in the reference), and above 16 tokens the
 * cross-attention launches stage the first min(Ta, Te) K / V rows of a sample only. */
mdt_status mdt_encode(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                      int32_t modality, int32_t honour_modality, const float *sigma, int64_t batch,
                      float *ctx_out, void *stream);

/* GCDenoiser.forward(state, action, goal, sigma) given the cached context of the last mdt_encode()
 * (reference score_wrappers.py:65-80 -> mdtv_transformer.py:224-236): EDM preconditioning, sigma
 * embedding, adaLN decoder, action head.   x:(B,Ta,A)  sigma:(B,) device  out:(B,Ta,A).
 * flags: MDT_RAW_OUTPUT returns the network output F instead of F*c_out + x*c_skip (GCDenoiser.loss);
 *        MDT_RAW_INPUT feeds x to action_emb without the c_in scaling (inner_model.forward_dec_only);
 *        MDT_SIGMA_SCALAR: `sigma` points to ONE float shared by the whole batch (what every sampler passes:
 *        sigmas[i] * s_in) -- one sigma-embedding / adaLN row instead of B, broadcast by the kernels. */
enum { MDT_RAW_OUTPUT = 1, MDT_RAW_INPUT = 2, MDT_SIGMA_SCALAR = 4 };
mdt_status mdt_denoise_cached(mdt_model *m, const float *x, const float *sigma, int64_t batch,
                              int32_t flags, float *out, void *stream);

/* model(state, action, goal, sigma) exactly as the samplers call it (reference gc_sampling.py:945):
 * mdt_encode + mdt_denoise_cached in one call ("as written": the encoder is re-run). */
mdt_status mdt_forward(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                       int32_t modality, const float *x, const float *sigma, int64_t batch,
                       float *out, float *ctx_out, void *stream);

/* sample_ddim(model, state, action, goal, sigmas) (reference gc_sampling.py:922-951) as ONE enqueue:
 * encoder + cross K/V once, sigma-embedding/adaLN vectors for all steps once, then n_steps decoder
 * evaluations with the update x <- (s_{i+1}/s_i) x - expm1(-h_i) den fused into the action-head kernel.
 * (use_ada_conditioning == 0: the encoder depends on sigma and runs inside the step loop, as in the reference;
 * ctx_out then receives the LAST step's context, which is what the reference leaves in latent_encoder_emb.)
 *   x_T    : (B, Ta, A) initial noisy actions (already multiplied by sigma_max, mdtv_agent.py:546)
 *   sigmas : HOST array of n_steps+1 floats (get_sigmas_* output, last entry normally 0)
 *   out    : (B, Ta, A) sampled actions;  ctx_out: optional (B,Te,d) latent_encoder_emb
 * Arguments are checked before anything is enqueued (an invalid-argument return leaves no device work behind).
 * Under stream capture: the HOST schedule travels by value in the first kernel's arguments, so a captured call bakes the
 * schedule of capture time into the graph (a replay does not re-read `sigmas`); capture mdt_sample_ddim_dev, whose schedule is
 * read from device memory at every replay, when the schedule may change between replays. */
mdt_status mdt_sample_ddim(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                           int32_t modality, const float *x_T, const float *sigmas_host, int32_t n_steps,
                           int64_t batch, float *out, float *ctx_out, void *stream);

/* The same call with the noise schedule in DEVICE memory, as MDTVAgent.get_noise_schedule builds it (mdtv_agent.py:660-667):
 * the per-step scalars t = -ln(sigma), h, sigma ratio and -expm1(-h) (gc_sampling.py:946-950) are computed by a device kernel,
 * nothing is copied to the host and the call never synchronises.  sigmas_dev: n_steps + 1 floats on the model's device. */
mdt_status mdt_sample_ddim_dev(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                               int32_t modality, const float *x_T, const float *sigmas_dev, int32_t n_steps,
                               int64_t batch, float *out, float *ctx_out, void *stream);

/* The other samplers of the reference's dispatch table (mdtv_agent.py:593-658) as ONE enqueue each, like mdt_sample_ddim:
 * a plan kernel derives the sampler's denoiser evaluations and a table of per-evaluation coefficients from the schedule,
 * then every evaluation is one decoder pass whose action-head kernel applies the sampler update and embeds the next input.
 * Schedule: n_steps + 1 levels, except for MDT_SAMPLER_DPM_FAST (below).  Schedule assumption (what every get_sigmas_*
 * guarantees): all n_steps + 1 levels are > 0 except the final one, which is
 * 0.  The Python loops branch on sigmas[i + 1] == 0 (and on sigma_down == 0 for the ancestral samplers); the native
 * call takes the branch at the last step and only there, so its launch sequence depends on the kind and n_steps alone. */
typedef enum {
    MDT_SAMPLER_EULER = 0,              /* sample_euler              (s_churn, s_tmin, s_tmax, s_noise) */
    MDT_SAMPLER_EULER_ANCESTRAL = 1,    /* sample_euler_ancestral    (eta)                              */
    MDT_SAMPLER_HEUN = 2,               /* sample_heun               (s_churn, s_tmin, s_tmax, s_noise) */
    MDT_SAMPLER_DPM_2 = 3,              /* sample_dpm_2              (s_churn, s_tmin, s_tmax, s_noise) */
    MDT_SAMPLER_DPM_2_ANCESTRAL = 4,    /* sample_dpm_2_ancestral    (eta)                              */
    MDT_SAMPLER_LMS = 5,                /* sample_lms                (order 1..4)                       */
    MDT_SAMPLER_DPMPP_2S = 6,           /* sample_dpmpp_2s                                              */
    MDT_SAMPLER_DPMPP_2S_ANCESTRAL = 7, /* sample_dpmpp_2s_ancestral (eta, s_noise)                     */
    MDT_SAMPLER_DPMPP_2M = 8,           /* sample_dpmpp_2m / sample_dpmpp_2_with_lms                    */
    MDT_SAMPLER_DPMPP_SDE = 9,          /* sample_dpmpp_sde          (eta, s_noise, r)                  */
    MDT_SAMPLER_DPM_FAST = 10,          /* sample_dpm_fast           (eta, s_noise)                     */
    MDT_SAMPLER_COUNT = 11
} mdt_sampler_kind;
/* MDT_SAMPLER_DPM_FAST: the schedule is the two levels {sigma_max, sigma_min}, both > 0, and n_steps is the evaluation count
 * n (1..MDT_SAMPLER_MAX_EVALS): n // 3 + 1 solver steps uniform in t = -ln(sigma).  eta != 0 needs sigma_min < sigma_max
 * (as the Python function: no ancestral noise when sampling in reverse).  Violations give MDT_ERR_INVALID_ARG on a host
 * schedule; a device schedule is read at replay time and not checked. */

/* The samplers' scalar parameters; a field a kind does not take is ignored.  Python's defaults: eta 1, s_churn 0,
 * s_tmin 0, s_tmax +inf, s_noise 1, r 0.5, order 4. */
typedef struct mdt_sampler_params {
    float eta, s_churn, s_tmin, s_tmax, s_noise, r;
    int32_t order;
} mdt_sampler_params;

enum { MDT_SAMPLER_MAX_STEPS = 64, MDT_SAMPLER_MAX_EVALS = 2 * MDT_SAMPLER_MAX_STEPS, MDT_SAMPLER_NREG = 10 };
/* Registers of the per-element update, in coefficient order: X the state, Y this evaluation's input, D its denoised output,
 * d = (Y - D) / sigma, H0..H3 the history slots (H0 the newest), N0 / N1 this evaluation's noise rows. */
enum { MDT_R_X = 0, MDT_R_Y = 1, MDT_R_D = 2, MDT_R_DD = 3, MDT_R_H0 = 4, MDT_R_N0 = 8, MDT_R_N1 = 9 };
enum { MDT_PUSH_NONE = 0, MDT_PUSH_D = 1, MDT_PUSH_DD = 2 };

/* One denoiser evaluation of a plan (32 words).  The head of this evaluation computes, per element,
 *     X' = sum_k cx[k] R[k]                      (the new state; the sampler's output after the last evaluation)
 *     Y' = cy[NREG] X' + sum_k cy[k] R[k]        (the next evaluation's input, embedded with c_in(sigma_next))
 * and then pushes D or d into H0 (older slots move down one; the oldest is dropped) when `push` says so. */
typedef struct mdt_sampler_eval {
    float sigma;                     /* the denoiser's sigma (c_in / c_skip / c_out and the conditioning row)          */
    float sigma_next;                /* the next evaluation's sigma; 0 after the last                                 */
    float cx[MDT_SAMPLER_NREG];
    float cy[MDT_SAMPLER_NREG + 1];
    int32_t push;                    /* MDT_PUSH_*                                                                    */
    int32_t noise[2];                /* rows of the noise buffer read as N0 / N1, -1 = none                           */
    int32_t draws;                   /* noise rows the Python loop draws from this evaluation up to the next one      */
    int32_t step;                    /* the sampler step this evaluation belongs to                                   */
    float t;                         /* DPM-Solver kinds: t = -ln(sigma) of this evaluation as the Python loop has it   */
    int32_t ends_step;               /* 1 on the last evaluation of its sampler step: X' is the step's result (where a loop
                                        that clips runs scaler.clip_output); a step's pass evaluation is its last          */
    int32_t begins_step;             /* 1 on the first evaluation of its step: its input and denoised output are what the
                                        Python loop hands to `callback`                                                   */
    int32_t pad[1];
} mdt_sampler_eval;

typedef struct mdt_sampler_plan_t {
    int32_t n_evals, n_noise;        /* evaluations; noise rows the Python loop draws (the rows the call reads)        */
    int32_t y0_noise;                /* the first input is Y_0 = x_T + y0_cn * N[y0_noise] (-1: Y_0 = x_T)             */
    float y0_cn;
    int32_t y0_draws;                /* noise rows the Python loop draws before the first evaluation                   */
    int32_t pad[3];
    mdt_sampler_eval e[MDT_SAMPLER_MAX_EVALS];
} mdt_sampler_plan_t;

/* Host helper (no GPU work): the plan mdt_sample would build for this kind, parameter set and HOST schedule (n_steps + 1
 * levels, or the two of MDT_SAMPLER_DPM_FAST; the device runs the same routine; libm and the device's math functions may
 * differ in the last place). */
mdt_status mdt_sampler_plan(int32_t kind, const mdt_sampler_params *params, const float *sigmas_host, int32_t n_steps,
                            mdt_sampler_plan_t *plan);

/* sample_<kind>(model, state, action, goal, sigmas, ...) as ONE enqueue (see mdt_sampler_kind).
 *   params : host struct (NULL: Python's defaults)
 *   noise  : NULL or (n_noise, B, Ta, A) device noise in the Python loop's draw order (plan.n_noise rows: randn_like draws
 *            times nothing -- s_noise is applied by the call); required when the noise can matter: s_churn > 0 for euler /
 *            heun / dpm_2, eta != 0 for the ancestral kinds and dpmpp_sde.  n_noise: rows available, at least plan.n_noise
 *            (mdt_sample) or the structural maximum (mdt_sample_dev: n for euler / heun / dpm_2 / dpmpp_2s_ancestral, n - 1
 *            for euler_ancestral / dpm_2_ancestral, 2 (n - 1) for dpmpp_sde with eta != 0, n // 3 + 1 for dpm_fast with
 *            eta != 0; rows beyond the plan's are unread).  dpm_fast: eta != 0 and s_noise != 0 need the noise buffer.
 *   ctx_out: optional (B, Te, d): what the Python loop leaves in latent_encoder_emb.
 * Arguments are checked before anything is enqueued.  Capture-safe; mdt_sample_dev reads its schedule at replay time. */
mdt_status mdt_sample(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                      const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_host,
                      int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, float *out, float *ctx_out,
                      void *stream);
mdt_status mdt_sample_dev(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                          const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_dev,
                          int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, float *out, float *ctx_out,
                          void *stream);

/* The full form of the plan-sampler call; every other fixed-schedule entry of this family is it with named defaults:
 *   mdt_sample / mdt_sample_dev: opts = NULL;  mdt_sample_guided / _dev_guided: opts = {cond_lambda};
 *   mdt_sample_sde_tree*: kind = MDT_SAMPLER_DPMPP_SDE, noise = NULL, opts = {cond_lambda (1.0f unless _guided), tree}.
 * Still ONE enqueue, with the launches of the call it extends.
 *   lo, hi : the bounds of scaler.clip_output, x <- min(max(x, lo), hi) per action dimension as torch.clamp computes it (NaN
 *            stays NaN; lo > hi gives hi), applied in the head of every evaluation that ends a step of a loop that clips there:
 *            after every step of euler, euler_ancestral, heun, dpm_2, dpm_2_ancestral, lms, dpmpp_2s, dpmpp_2s_ancestral; after
 *            every step but the final one of dpmpp_sde; never in dpmpp_2m and dpm_fast (the reference's loops take a scaler
 *            there and do not read it).  +-inf bounds leave every bit as it is.
 *   record : one row pair per sampler step i -- n_steps of them, n_steps // 3 + 1 (the solver steps) for MDT_SAMPLER_DPM_FAST --
 *            [i][0] the input of the step's first evaluation in action units (after the sigma_hat churn: the loop's 'x'),
 *            [i][1] its denoised output (the guided call: the combined D_lambda).
 *   tree   : the noise of mdt_sample_sde_tree (kind must be MDT_SAMPLER_DPMPP_SDE; `noise` is then not read).
 *   pin_known, pin_keep : pinned actions (chunk inpainting: receding-horizon replanning with overlap, way-points, "first action =
 *            current pose").  Both (B, Ta, A), keep in [0, 1].  The pin is an argument of the denoiser:
 *                D'(x; sigma) = keep * known + (1 - keep) * D(x; sigma)
 *            per element in fp32 as D + keep (known - D), with selects at both ends: keep == 0 gives the bits of D, keep == 1 the
 *            bits of known.  With guidance D is the combined D_lambda (guide first, then pin).  The head applies it right after
 *            the EDM combine, so every sampler uses D' wherever it used D: its update, its derivative d = (x - D') / sigma, its
 *            history slots and the `denoised` of the record.  Bounds clamp x where they did; x_T stays the caller's.  Under every
 *            kind whose schedule ends at sigma = 0 the elements with keep == 1 arrive at `known` to rounding; MDT_SAMPLER_DPM_FAST
 *            stops at sigma_min and arrives within O(sigma_min); 0 < keep < 1 blends the prediction toward `known` at every step.
 *            Values outside [0, 1] are not checked here (the Python facade's ActionPin refuses them).
 * opts == NULL is {sizeof(mdt_sample_opts), 1.0f, NULL, NULL, NULL, NULL}; a call without a pin launches what it did before pins.
 * `size` is sizeof(mdt_sample_opts), or the struct's size before pin_known / pin_keep were appended (40 on LP64): the two fields
 * then read as NULL, so a client compiled against the earlier header keeps working.
 * Checked before anything is enqueued (MDT_ERR_INVALID_ARG, the message names the field): any other size, exactly one of lo / hi,
 * exactly one of pin_known / pin_keep, a non-finite cond_lambda, tree with another kind.  lo, hi, record, pin_known and pin_keep
 * need no more than a float's alignment (the head reads and writes them element by element): a slice of a larger tensor will do.
 * mdt_sample_dpm_adaptive takes no options and no pin: a pinned adaptive run is the Python host loop (sample_dpm_adaptive with
 * extra_args = {"pin": ...}), which applies the pin in GCDenoiser.forward. */
typedef struct mdt_sample_opts {
    int32_t size;                    /* sizeof(mdt_sample_opts): lets the struct grow                                   */
    float cond_lambda;               /* 1.0f: the unguided call; anything else: the doubled-batch guided call           */
    const float *lo, *hi;            /* (A,) device; both NULL: no bounds                                               */
    float *record;                   /* NULL or (steps, 2, B, Ta, A) device: [i][0] = x, [i][1] = denoised               */
    const struct mdt_brownian_source *tree; /* NULL, or dpmpp_sde's tree noise as in mdt_sample_sde_tree (below)         */
    const float *pin_known, *pin_keep; /* both NULL, or both (B, Ta, A) device: D' = keep known + (1 - keep) D             */
} mdt_sample_opts;
mdt_status mdt_sample_opt(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                          const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_host,
                          int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, float *out, float *ctx_out,
                          const mdt_sample_opts *opts, void *stream);
mdt_status mdt_sample_dev_opt(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                              const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_dev,
                              int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, float *out, float *ctx_out,
                              const mdt_sample_opts *opts, void *stream);

/* The full form of the DDIM call: mdt_sample_ddim / _dev are it with opts = NULL, mdt_sample_ddim_guided / _dev_guided with
 * opts = {cond_lambda}.  It reads cond_lambda and pin_known / pin_keep (above); lo and hi are accepted and not read -- the
 * reference's DDIM takes a scaler and never clips; record and tree are MDT_ERR_INVALID_ARG (the message names the field). */
mdt_status mdt_sample_ddim_opt(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                               const float *x_T, const float *sigmas_host, int32_t n_steps, int64_t batch, float *out,
                               float *ctx_out, const mdt_sample_opts *opts, void *stream);
mdt_status mdt_sample_ddim_dev_opt(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                   const float *x_T, const float *sigmas_dev, int32_t n_steps, int64_t batch, float *out,
                                   float *ctx_out, const mdt_sample_opts *opts, void *stream);

/* Several action chunks per observation from one shared context: the *_opt call of each family with `candidates` = K >= 1 chunks
 * for each of the `batch` = B observations (best-of-N with a critic, the chunk most coherent with a pinned one, the spread over
 * chunks as an uncertainty signal).  Still ONE enqueue.  What does not depend on the noisy actions -- the guide staging, the
 * encoder, the stacked cross K|V product, the fold of the collapsed cross-attention -- runs on the B observations (2B when
 * guided); the decoder blocks and every head run on the B * K chunks (2 B K decoder samples when guided).
 * Layout, observation-major: chunk k of observation b is sample b * K + k.
 *   per chunk       : x_T and out (B * K, Ta, A); the noise rows (n_noise, B * K, Ta, A); opts.pin_known / pin_keep (B * K, Ta, A);
 *                     opts.record (steps, 2, B * K, Ta, A); opts.tree's seeds (n_seeds = 1 or B * K)
 *   per observation : tokens, tokens2, goal; ctx_out (B, Te, d)
 * Guided, the decoder runs [B K conditional | B K unconditional] samples over the contexts [B conditional | B unconditional]:
 * decoder sample s reads context s / K in either half.  Every option means what it means in the *_opt call, per chunk.
 * candidates == 1 enqueues exactly the launches of the *_opt entry and gives its bits.  Before anything is enqueued,
 * MDT_ERR_INVALID_ARG with the entry and the field in the message: candidates < 1; a batch * candidates (doubled when guided)
 * beyond what the decoder's row counts hold.  The workspace grows for the decoder samples: a caller who captures the call
 * reserves B * K first, 2 * B * K when guided (mdt_reserve).  The per-context buffers are carved at that size too and the call
 * uses their first B (2B) entries.
 * mdt_sample_dpm_adaptive has no such form (the Python facade's host loop expands the observations instead). */
mdt_status mdt_sample_multi(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                            const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_host,
                            int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, int32_t candidates, float *out,
                            float *ctx_out, const mdt_sample_opts *opts, void *stream);
mdt_status mdt_sample_dev_multi(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_dev,
                                int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, int32_t candidates,
                                float *out, float *ctx_out, const mdt_sample_opts *opts, void *stream);
mdt_status mdt_sample_ddim_multi(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                 const float *x_T, const float *sigmas_host, int32_t n_steps, int64_t batch, int32_t candidates,
                                 float *out, float *ctx_out, const mdt_sample_opts *opts, void *stream);
mdt_status mdt_sample_ddim_dev_multi(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                     const float *x_T, const float *sigmas_dev, int32_t n_steps, int64_t batch,
                                     int32_t candidates, float *out, float *ctx_out, const mdt_sample_opts *opts, void *stream);

/* Score action chunks by their denoising error: the step between mdt_sample*_multi and the selection, forwards only.  ONE enqueue
 * on the inference path -- no mdt_train_prepare, no tape, no synchronisation, nothing read back -- and safe to capture into a
 * graph once the workspace holds the call's rows (mdt_reserve(batch * candidates * n_levels * draws), or one eager call, first).
 *     score[r] = - sum_s w_s (1 / M) sum_m sum_e q[r, s, m, e]^2,   q = (x0[r] - D(x0[r] + sigma_s n[s, m]; sigma_s, context(r / K))) / sigma_s
 * for the R = B * K chunks x0 (R, Ta, A), chunk k of observation b at row b * K + k; S = n_levels levels sigmas_host (S,) and
 * weights weights_host (S,), both in host memory and read before the call returns; M = draws noise rows per level, noise
 * (S, M, Ta, A) on the device, the same rows for every chunk of every observation (antithetic pairs n, -n side by side cancel the
 * part of the estimate that is odd in n).  By the pointwise I-MMSE relation this is log p(x0) up to a constant of the call for a
 * denoiser that is the posterior mean, truncated to the range of the levels: higher is better, and score goes to a per-observation
 * argmax as it is.  It ranks chunks; it is no calibrated likelihood.  weights_host == NULL: the trapezoid rule in ln sigma over the
 * levels in the order given (w = 1 for a single level); the levels must then be strictly monotone.
 * q is formed from the raw network output F without forming x0 - D: q = sigma / (sigma^2 + sd^2) x0 - c_skip n - sd / sqrt(sigma^2 + sd^2) F.
 * The encoder, the stacked cross K|V product and the fold run once on the B observations (tokens, tokens2, goal as in
 * mdt_sample_ddim_multi), the decoder blocks and the head once on B * S * K * M samples, each with its own sigma; with
 * use_ada_conditioning = 0 sigma is a context token and the encoder runs on the B * S contexts.  ctx_out: NULL or (B, Te, d), the
 * observations' context (sigma as a context token: at the last level).  A chunk's score does not depend on the other chunks of
 * the call, and the sums have one fixed order: the same call gives the same bits.
 * MDT_ERR_INVALID_ARG, "mdt_denoising_score: ..." naming the field, before anything is enqueued: a null handle or required
 * pointer; batch or candidates < 1; n_levels or draws outside [1, 64]; a level that is not finite and > 0; a weight that is not
 * finite and >= 0; weights_host == NULL with levels that are not strictly monotone; MDT, or a use_proprio handle, without tokens2;
 * more rows batch * candidates * n_levels * draws than the decoder's 2^24 / max(Te, Ta) samples. */
mdt_status mdt_denoising_score(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                               const float *x0, const float *sigmas_host, const float *weights_host, int32_t n_levels,
                               const float *noise, int32_t draws, int64_t batch, int32_t candidates, float *score, float *ctx_out,
                               void *stream);

/* Sample, score and select in ONE enqueue: the mdt_sample*_multi call of each family, mdt_denoising_score on its chunks and the
 * per-observation selection, with nothing read back -- the replan-and-select loop of a controller as one call, capturable like its
 * parts.  Each entry is its *_multi entry with `out` replaced by `best` (B, Ta, A), the winning chunk of every observation, and a
 * `select` argument in front of `stream`:
 *   sigmas_host, weights_host, n_levels, noise, draws : the score's levels, weights (NULL: the trapezoid rule in ln sigma), and
 *            noise rows (n_levels, draws, Ta, A), as mdt_denoising_score takes them
 *   chunks : (B * K, Ta, A), all the sampled chunks -- what the *_multi entry writes to `out`, bit for bit
 *   scores : (B * K), what mdt_denoising_score gives on those chunks
 *   index  : (B) int32, per observation the k of the largest score: ties go to the lowest k; a NaN score loses to every other,
 *            -Inf included; an observation whose scores are all NaN selects 0.  (Exactly gc_sampling.best_candidates' index, whose
 *            torch.nan_to_num reads +Inf as the largest finite float: +Inf ties with FLT_MAX.)  best[b] = chunks[b * K + index[b]].
 * `opts` means what it means in the *_multi entry -- guidance, bounds, pin, record, tree -- and shapes the SAMPLING only: the score
 * is that of the unguided, unpinned, unclamped conditional model on the final chunks, as mdt_denoising_score's is.  ctx_out is the
 * sampler's.  candidates == 1 is legal: best is the chunk, index 0.
 * Where the context does not depend on sigma (use_ada_conditioning = 1, the NoiseBlock decoder) the score phase runs no encoder: it
 * reads the context, the cross K|V rows and the folded operands the sampler's prefix left for the B observations (a guided call's
 * conditional half).  The unguided call's scores then have mdt_denoising_score's bits; a guided call's encoder ran 2B contexts
 * where the stand-alone scorer runs B, which may route its products differently.  With sigma as a context token the score phase
 * stages and encodes its B * n_levels contexts as mdt_denoising_score does.
 * The workspace: max(the sampler's decoder samples, B * K * n_levels * draws), reserved once before the first launch; a caller who
 * captures the call makes one eager call, or mdt_reserve of that maximum, first.
 * MDT_ERR_INVALID_ARG before anything is enqueued, the message naming the entry and the field: a NULL select or a select.size that is
 * not sizeof(mdt_select_spec); a NULL best, chunks, scores, index, sigmas_host or noise; whatever mdt_denoising_score refuses of
 * n_levels, draws, the levels, the weights and batch * candidates * n_levels * draws; whatever the *_multi entry refuses.
 * mdt_sample_dpm_adaptive and the steered calls have no such form. */
typedef struct mdt_select_spec {
    int32_t size;                             /* sizeof(mdt_select_spec): lets the struct grow                                  */
    const float *sigmas_host, *weights_host;  /* (S,) host; weights NULL: trapezoid rule in ln sigma, as mdt_denoising_score    */
    int32_t n_levels;
    const float *noise; int32_t draws;        /* (S, M, Ta, A) device                                                           */
    float *chunks;                            /* (B*K, Ta, A) device, required: all sampled chunks                              */
    float *scores;                            /* (B*K) device, required                                                         */
    int32_t *index;                           /* (B) device, required                                                           */
} mdt_select_spec;
mdt_status mdt_sample_select(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                             const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_host,
                             int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, int32_t candidates, float *best,
                             float *ctx_out, const mdt_sample_opts *opts, const mdt_select_spec *select, void *stream);
mdt_status mdt_sample_dev_select(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                 const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_dev,
                                 int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, int32_t candidates,
                                 float *best, float *ctx_out, const mdt_sample_opts *opts, const mdt_select_spec *select,
                                 void *stream);
mdt_status mdt_sample_ddim_select(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                  const float *x_T, const float *sigmas_host, int32_t n_steps, int64_t batch, int32_t candidates,
                                  float *best, float *ctx_out, const mdt_sample_opts *opts, const mdt_select_spec *select,
                                  void *stream);
mdt_status mdt_sample_ddim_dev_select(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                      const float *x_T, const float *sigmas_dev, int32_t n_steps, int64_t batch,
                                      int32_t candidates, float *best, float *ctx_out, const mdt_sample_opts *opts,
                                      const mdt_select_spec *select, void *stream);

/* sample_dpm_adaptive (eta = 0): DPM-Solver-12 / -23 with the PID step-size control of _StepControl, as ONE blocking call.
 * Every attempted step runs its 2 or 3 denoiser evaluations; the head of the last one writes both the order-k ("high") and the
 * order-(k-1) ("low") result, one small kernel writes per-workgroup partial sums of the scaled error, and the host reads them
 * back (one synchronisation per attempt), sums them in double in a fixed order and updates the controller.  A rejected step
 * leaves the state as it was.  Returns MDT_ERR_STATE on a capturing stream (nothing enqueued) and MDT_ERR_NUMERIC where the
 * Python loop would spin forever (NaN error or step size, or s + h == s in fp32). */
typedef struct mdt_dpm_adaptive_params {
    int32_t order;                   /* 2 or 3                                                                          */
    double rtol, atol, h_init, pcoeff, icoeff, dcoeff, accept_safety;  /* Python's defaults: 0.05 0.0078 0.05 0 1 0 0.81   */
} mdt_dpm_adaptive_params;
typedef struct mdt_dpm_adaptive_info {
    int32_t steps, nfe, n_accept, n_reject;  /* the Python loop's info dict                                             */
} mdt_dpm_adaptive_info;
/* _StepControl's state (gc_sampling.py): step size h, filter weights, log inverse error history */
typedef struct mdt_dpm_control {
    double h, w[3], safety, eps, hist[3];
    int32_t started, pad;
} mdt_dpm_control;
enum { MDT_DPM_REJECT = 0, MDT_DPM_ACCEPT = 1, MDT_DPM_STOP = 2 };

/* Host helpers (no GPU work).  mdt_dpm_control_init / _update: the controller the call runs (update returns MDT_DPM_* in
 * *decision; STOP where the error or the new h is NaN).  mdt_dpm_adaptive_plan: the evaluations of one attempted step from
 * s to t (t = -ln sigma) at `order`; the last evaluation's cx is the order-k combine, its cy the order-(k-1) one. */
mdt_status mdt_dpm_control_init(mdt_dpm_control *c, double h, double pcoeff, double icoeff, double dcoeff, double order,
                                double accept_safety);
mdt_status mdt_dpm_control_update(mdt_dpm_control *c, float error, int32_t *decision);
mdt_status mdt_dpm_adaptive_plan(int32_t order, float s, float t, mdt_sampler_plan_t *plan);

/* params: NULL = Python's defaults (order 3).  out (B, Ta, A), ctx_out optional (B, Te, d), info optional (host). */
mdt_status mdt_sample_dpm_adaptive(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                                   int32_t modality, const float *x_T, float sigma_min, float sigma_max,
                                   const mdt_dpm_adaptive_params *params, int64_t batch, float *out, float *ctx_out,
                                   mdt_dpm_adaptive_info *info, void *stream);

/* Classifier-free guidance.  With D(x; sigma, g) the GCDenoiser output and D(x; sigma, 0) the same call with uncond=True (the
 * goal zeroed before its embedding, reference mdtv_transformer.py:246-258), the guided denoiser is
 *     D_lambda(x; sigma) = D(x; sigma, 0) + lambda (D(x; sigma, g) - D(x; sigma, 0))
 * lambda = 1: the conditional model; 0: the unconditional one; > 1: a stronger pull towards the goal.  Any finite lambda is
 * accepted; NaN / +-Inf give MDT_ERR_INVALID_ARG before anything is enqueued.  c_skip x is the same in both branches, so the
 * calls combine the network outputs instead, F = F_0 + lambda (F_g - F_0) in fp32 per element before the output scaling.
 *
 * Each call is its family's full form with opts = {cond_lambda} (mdt_sample_dpm_adaptive_guided: its unguided twin plus
 * `cond_lambda`). At lambda == 1, and on a model without a goal token (goal_conditioned=False with MDT, or with MDT-V and
 * use_proprio: there `uncond` changes nothing), it runs the unguided call and gives its bits. Otherwise ONE call runs the
 * sampler loop over 2B samples: [0, B) conditional, [B, 2B) the same state tokens with every one of the goal_seq_len goal rows zero (and the same `modality`
 * embedder). The 2B encoder inputs are staged inside the stream (handle-owned buffers, no host synchronisation: capture-safe
 * like the unguided calls); the encoder, the cross-attention K/V and every decoder pass run at 2B; each action head reads rows
 * r and r + B Ta, combines them and updates the B samples of state. The noise rows are those of the unguided call at B (the
 * host loop's draws). ctx_out receives the conditional context (B, Te, d). The workspace grows for 2B samples: mdt_reserve(m,
 * 2 B) before capturing a guided call. */
mdt_status mdt_sample_ddim_guided(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                                  int32_t modality, const float *x_T, const float *sigmas_host, int32_t n_steps,
                                  int64_t batch, float *out, float *ctx_out, float cond_lambda, void *stream);
mdt_status mdt_sample_ddim_dev_guided(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                                      int32_t modality, const float *x_T, const float *sigmas_dev, int32_t n_steps,
                                      int64_t batch, float *out, float *ctx_out, float cond_lambda, void *stream);
mdt_status mdt_sample_guided(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                             const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_host,
                             int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, float *out, float *ctx_out,
                             float cond_lambda, void *stream);
mdt_status mdt_sample_dev_guided(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                 const float *x_T, int32_t kind, const mdt_sampler_params *params, const float *sigmas_dev,
                                 int32_t n_steps, const float *noise, int32_t n_noise, int64_t batch, float *out,
                                 float *ctx_out, float cond_lambda, void *stream);
mdt_status mdt_sample_dpm_adaptive_guided(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                                          int32_t modality, const float *x_T, float sigma_min, float sigma_max,
                                          const mdt_dpm_adaptive_params *params, int64_t batch, float *out, float *ctx_out,
                                          float cond_lambda, mdt_dpm_adaptive_info *info, void *stream);

/* Brownian-tree noise: the default noise sampler of sample_dpmpp_sde (the reference's BrownianTreeNoiseSampler) without
 * torchsde.  A virtual Brownian tree (Levy midpoint construction, csrc/mdt_brownian.h) on [lo, hi] (lo < hi; W(lo) = 0) whose
 * value at any point is a pure function of (seed, element, point), walked in double until the interval is <= tol (at most 62
 * levels; a tol that needs more is MDT_ERR_INVALID_ARG; the reference's 1e-6 takes 27 levels on [0.001, 80]).  The normals are
 * Box-Muller on the library's Philox4x32-10 keyed by the seed.  The noise value of a query (from, to) is
 *     (W(to) - W(from)) / sqrt(|to - from|)          (double, rounded once to fp32; points clamped to [lo, hi])
 * Seeds: n_seeds == 1: one tree per element of the whole (batch, per_row) tensor (element = its flat index); n_seeds == batch:
 * sample b uses seeds[b] and the element index inside its row, so a sample's noise does not depend on the rest of the batch.
 * Bit parity with torchsde is not a goal (another algorithm); the law is the same. */
enum { MDT_BROWNIAN_MAX_PAIRS = 64 };
/* mdt_brownian_noise: out (n_q, batch, per_row) on the device for n_q <= MDT_BROWNIAN_MAX_PAIRS HOST pairs
 * (pairs[2 q], pairs[2 q + 1]) = (from, to); seeds: n_seeds device keys.  One launch, capture-safe, never synchronises (the
 * pairs ride in the kernel's arguments).  mdt_brownian_noise_host: the same values from the same routine on host memory (seeds
 * and out on the host, any n_q, no GPU work). */
mdt_status mdt_brownian_noise(const uint64_t *seeds, int32_t n_seeds, double lo, double hi, double tol, const double *pairs,
                              int32_t n_q, int64_t batch, int64_t per_row, float *out, void *stream);
mdt_status mdt_brownian_noise_host(const uint64_t *seeds, int32_t n_seeds, double lo, double hi, double tol, const double *pairs,
                                   int32_t n_q, int64_t batch, int64_t per_row, float *out);

/* The tree of a dpmpp_sde call that draws its noise inside the call (mdt_sample_sde_tree*).  lo < hi: the tree's interval (a
 * noise sampler built with its own sigma_min / sigma_max); lo == hi == 0: the schedule's smallest positive and largest level,
 * the reference's default, taken on the device for a device schedule. */
typedef struct mdt_brownian_source {
    const uint64_t *seeds;           /* device: n_seeds keys                                                           */
    int32_t n_seeds;                 /* 1 or batch (see mdt_brownian_noise)                                            */
    int32_t pad;
    double lo, hi;                   /* the tree's interval, or 0, 0: the schedule's                                   */
    double tol;                      /* the walk's resolution (reference default 1e-6)                                 */
} mdt_brownian_source;

/* sample_dpmpp_sde (MDT_SAMPLER_DPMPP_SDE) with the noise of the reference's default noise sampler -- the Brownian tree of
 * `tree` -- drawn inside the call instead of read from a noise buffer (mdt_sample_opt / mdt_sample_dev_opt with opts.tree; a
 * NULL `tree` is MDT_ERR_INVALID_ARG). The plan kernel records the (from, to) points of every noise row -- (sigma(t),
 * sigma(s)) then (sigma(t), sigma(t_next)), each where sigma_up != 0, t = -ln(sigma) as the Python loop forms them -- and one
 * more launch before the first evaluation writes every row into a handle-owned buffer from the tree; the evaluations then read
 * it as they read a caller's noise (the same bits as passing those rows to mdt_sample). A device schedule is read in place
 * (interval and points included): capture-safe, no synchronisation. The first call at a larger batch or step count grows the
 * buffer (synchronising, and a new mdt_ws_generation): make one eager call before capturing. With eta == 0 or s_noise == 0 the
 * tree is not read. */
mdt_status mdt_sample_sde_tree(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                               const float *x_T, const mdt_sampler_params *params, const float *sigmas_host, int32_t n_steps,
                               const mdt_brownian_source *tree, int64_t batch, float *out, float *ctx_out, void *stream);
mdt_status mdt_sample_sde_tree_dev(mdt_model *m, const float *tokens, const float *tokens2, const float *goal, int32_t modality,
                                   const float *x_T, const mdt_sampler_params *params, const float *sigmas_dev, int32_t n_steps,
                                   const mdt_brownian_source *tree, int64_t batch, float *out, float *ctx_out, void *stream);
mdt_status mdt_sample_sde_tree_guided(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                                      int32_t modality, const float *x_T, const mdt_sampler_params *params,
                                      const float *sigmas_host, int32_t n_steps, const mdt_brownian_source *tree, int64_t batch,
                                      float *out, float *ctx_out, float cond_lambda, void *stream);
mdt_status mdt_sample_sde_tree_dev_guided(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                                          int32_t modality, const float *x_T, const mdt_sampler_params *params,
                                          const float *sigmas_dev, int32_t n_steps, const mdt_brownian_source *tree,
                                          int64_t batch, float *out, float *ctx_out, float cond_lambda, void *stream);

/* GCDenoiser.loss(state, action, goal, noise, sigma) forward value, eval mode (reference
 * score_wrappers.py:45-63): noised = a + n*sigma; F = inner(noised*c_in); target = (a - c_skip*noised)/c_out;
 * loss = mean((F - target)^2) over all B*Ta*A elements.  loss_out: 1 float (device); model_output: (B,Ta,A). */
mdt_status mdt_loss_fwd(mdt_model *m, const float *tokens, const float *tokens2, const float *goal,
                        int32_t modality, const float *action, const float *noise, const float *sigma,
                        int64_t batch, float *loss_out, float *model_output, float *ctx_out, void *stream);

/* Algorithmic FLOPs of one sampler call per action chunk (SURVEY.md 8(d) accounting: 2MNK per Linear,
 * full score matrices, encoder + cross K/V once, n_steps decoder evaluations). */
double mdt_flops_per_chunk(const mdt_model *m, int32_t n_steps);

/* Host helper (no GPU work): pyhash.fnv1_32 as the reference's harness uses it to derive deterministic
 * validation window sizes and environment seeds (mdt/datasets/base_dataset.py:20,37; mdt/evaluation/utils.py:17,305).
 * FNV-1, 32 bit: for each byte  h = h * 0x01000193; h ^= byte  (pyhash-0.9.3/src/fnv/hash_32.c:91-113), started from
 * `seed` -- pyhash passes its seed (default 0) as the initial value (src/FNV1.h:36-39, src/Hash.h:113,167), NOT the
 * standard offset basis 0x811c9dc5.  Chaining: pass the previous result as `seed`. */
uint32_t mdt_fnv1_32(const void *buf, uint64_t len, uint32_t seed);

/* Where the library's LARGE, batch-sized buffers come from: workspaces, training tapes and backward scratch (the weight
 * arenas and small tables stay hipMalloc'ed).  By default they are raw hipMalloc's; a host framework with its own caching
 * allocator (PyTorch) would then see "out of memory" while its own pool sits on gigabytes of cached-but-free blocks -- or the
 * other way round.  With an allocator installed the buffers live in the host's pool: `alloc(bytes, user)` returns a device
 * pointer (256-byte aligned, on the current device) or NULL when it cannot; `free_(ptr, user)` releases one -- the library
 * calls it only after hipDeviceSynchronize() (growing a buffer) or from the destroy functions.  NULL, NULL restores
 * hipMalloc / hipFree; buffers are released through whatever allocated them.  The switch is PROCESS-WIDE and takes effect for
 * every later allocation of every component (denoiser handles, Perceiver resampler, contrastive head, training tapes), whenever
 * it is made: buffers that already exist stay with the allocator they came from.  (The Python facade installs
 * torch.cuda.caching_allocator_alloc / _delete on every engine construction -- idempotent.) */
typedef void *(*mdt_alloc_fn)(size_t bytes, void *user);
typedef void (*mdt_free_fn)(void *ptr, void *user);
mdt_status mdt_set_allocator(mdt_alloc_fn alloc, mdt_free_fn free_, void *user);

/* Host shutdown: restore hipMalloc / hipFree AND forget the release callbacks of the buffers the installed allocator handed
 * out so far -- a later destroy call then DROPS such a buffer instead of calling `free_` (the host's pool is going away with
 * the process; its callbacks may already be gone).  The Python facade calls it from an atexit hook, so that a handle whose
 * finaliser runs during interpreter teardown never calls into a freed ctypes closure. */
mdt_status mdt_allocator_detach(void);

#ifdef __cplusplus
}
#endif
#endif /* MDT_HIP_H */
