// mdt_internal.h -- launcher prototypes shared by the kernel sources and the host logic of every module (denoiser,
// Perceiver resampler, MAP pool, masked-image decoder ops, InfoNCE), plus the host helpers they all use: error plumbing,
// Lin, the Bump carver, gemm_args and the batch-buffer allocator.  The bookkeeping of the three stateful handles (parameter
// slots, tapes, growing device blocks) is in mdt_handle.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "mdt_hip.h"
#include "mdt_hip_ops.h"
#include "mdt_resampler.h"
#include "mdt_hip_train.h"
#include "mdt_mae.h"
#include "mdt_route.h"   // which kernel a launch runs on: the shape rules, thresholds and *_supported predicates (host only)
#include "mdt_route_train.h"   // ... and the training path's: the Linear backward's plan, training attention, the row-wise kernels

// ---- error plumbing: the message behind mdt_last_error() (thread local, defined in mdt_model.hip) ----
mdt_status mdt_fail(mdt_status st, const char* fmt, ...);

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) return mdt_fail(MDT_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e));  \
    } while (0)

#define MDT_TRY(expr)                      \
    do {                                   \
        mdt_status _s = (expr);            \
        if (_s != MDT_OK) return _s;       \
    } while (0)

#define LAUNCH(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return mdt_fail(MDT_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));       \
    } while (0)

// ---- a Linear whose weight lives fragment-packed in a handle's arena ----
struct Lin {
    float* wp = nullptr;    // fragment-packed (N, K)
    float* bias = nullptr;  // (N) or nullptr
    int N = 0, K = 0;
    float* wt = nullptr;    // training only: fragment-packed image of W^T (N' = K, K' = N), for dX = dY W
    void* ws = nullptr;     // the MLP's two Linears, the stacked q|k|v and the decoder's attention c_proj: fp16 pair fragment image (4 N K + N bytes; mdt_mlp_split.h)
};

// bump allocator over one hipMalloc'ed block (count pass with base == nullptr, then the real pass)
struct Bump {
    float* base = nullptr;
    size_t off = 0;
    float* take(size_t n) {
        float* p = base ? base + off : nullptr;
        off += (n + 63) & ~(size_t)63;  // 256-byte granules keep every buffer 16-byte aligned
        return p;
    }
};

static inline mdt_gemm_args gemm_args(const float* A, int64_t lda, const Lin& w, float* out, int64_t ldo, int M) {
    mdt_gemm_args g;
    memset(&g, 0, sizeof g);
    g.A = A; g.lda = lda; g.Wp = w.wp; g.Wp_pair = w.ws; g.bias = w.bias; g.out = out; g.ldo = ldo;
    g.M = M; g.N = w.N; g.K = w.K;
    g.shift_off = -1; g.scale_off = -1; g.gate_off = -1; g.rows_per_sample = 1;
    g.gin = 1; g.gout = 1; g.goff = 0;
    return g;
}

// ---- the process-global test and measurement switches (setters: include/mdt_hip_debug.h, each a one-line write) ----
// One table, defined in mdt_kernels.hip and hidden from the library's dynamic symbols.  -1 = "the default" in every field but gemm_geometry, whose setter documents 0 as the
// heuristic and -1 as a geometry of its own.  Atomics: host threads may drive different handles side by side.
struct mdt_switches {
    std::atomic<int> attn_wide_min{-1};  // mdt_op_set_attn_wide_min: rows; 0 = never (and no k_attn_xattn either)
    std::atomic<int> mlp_fuse_min{-1};   // mdt_op_set_mlp_fuse_min: rows; 0 = never
    std::atomic<int> mlp_skew{-1};       // mdt_op_set_mlp_skew
    std::atomic<int> gemm_geometry{0};   // mdt_op_set_gemm_geometry
    std::atomic<int> trace_mlp{-1};      // mdt_op_trace_mlp: 1 = on
    std::atomic<int> side_jobs{-1};      // mdt_op_set_side_jobs: 0 = off
    // ... and the ones an environment variable fills the first time they are read (mdt_switch_env)
    std::atomic<int> ws_split{-1};       // MDT_HIP_WS_SPLIT / mdt_op_set_ws_split
    std::atomic<int> mlp_split{-1};      // MDT_HIP_MLP_SPLIT / mdt_op_set_mlp_split
    std::atomic<int> tn_split{-1};       // MDT_HIP_TN_SPLIT / mdt_op_set_tn_split
    std::atomic<int> dw_stream{-1};      // MDT_HIP_DW_STREAM (mdt_train.hip)
    std::atomic<int> xfold{-1};          // MDT_HIP_XFOLD (mdt_create)
};
extern mdt_switches g_mdt_sw __attribute__((visibility("hidden")));
// a field with an environment variable: its value if set (>= 0), else the variable's integer (unset: dflt), which `latch` keeps in
// the field.  xfold is read without latch: mdt_create looks at the environment every time, and a test flips it between two handles.
__attribute__((visibility("hidden"))) int mdt_switch_env(std::atomic<int>& field, const char* var, int dflt, bool latch = true);

// batch-sized buffers (workspace, tapes, backward scratch): through the installed allocator (mdt_set_allocator) or hipMalloc
hipError_t mdt_dev_malloc(void** p, size_t bytes);
hipError_t mdt_dev_free(void* p);

// the current device's buffer of zeros (stands in for absent bias / LayerNorm-bias vectors); nullptr on failure
const float* mdt_zeros();
// the process switches a route (mdt_route.h) depends on, read once per launch; and whether a side job is queued on this host thread
mdt_route_switches mdt_route_snapshot();
hipError_t mdt_launch_gemm(const mdt_gemm_args& a, hipStream_t s);
// the MLP sublayer as one launch (k_mlp): S = mdt_mlp_slices(D) partial slabs at parts + s * part_stride
hipError_t mdt_launch_mlp(const mdt_gemm_args& fc, const mdt_gemm_args& proj, float* parts, int64_t part_stride, hipStream_t s);
// the same launch in the three-way bf16 split form (mdt_mlp_split.h): w1s / w2s = split images of fc / proj (mdt_launch_pack_weight_split)
hipError_t mdt_launch_mlp_split(const mdt_gemm_args& fc, const mdt_gemm_args& proj, const void* w1s, const void* w2s, float* parts,
                                int64_t part_stride, hipStream_t s);
// ... and on fp16 pair images (the form the model's launches take)
hipError_t mdt_launch_mlp_pair(const mdt_gemm_args& fc, const mdt_gemm_args& proj, const void* w1p, const void* w2p, float* parts,
                               int64_t part_stride, hipStream_t s);
// (n_rows, K) row-major fp32 -> column tiles n_off / 16 .. of the fp16 pair image (n_rows, n_off % 16 == 0, K % 32 == 0); the same
// image from the fp32 fragment image of the whole (N, K) weight.  mdt_pair_image_bytes (mdt_mlp_split.h) = 4 N K + N
// the wide LayerNorm-prologue product (K = 384 / 512, N a multiple of 384, plain output rows) in the pair form on a.Wp_pair
bool mdt_gemm_ln_pair_supported(const mdt_gemm_args& a);
hipError_t mdt_launch_gemm_ln_pair(const mdt_gemm_args& a, hipStream_t s);
constexpr int64_t mdt_pair_image_bytes(int64_t N, int64_t K) { return (N / 16) * ((K / 32) * 2048 + 16); }
hipError_t mdt_launch_pack_weight_pair(const float* w, int n_rows, int K, void* image, hipStream_t s, int n_off = 0);
hipError_t mdt_launch_pair_from_packed(const float* wp, int N, int K, void* image, hipStream_t s);
// (n_rows, K) row-major fp32 -> split image of 6 n_rows K bytes (n_rows % 16 == 0, K % 32 == 0)
hipError_t mdt_launch_pack_weight_split(const float* w, int n_rows, int K, void* image, hipStream_t s, int n_off = 0);
// the same image from the fp32 fragment image of the weight (mdt_launch_pack_weight's output for the whole (N, K) matrix)
hipError_t mdt_launch_split_from_packed(const float* wp, int N, int K, void* image, hipStream_t s);
// ctx_div (here and in the three cross-attention launchers below; 1 = the plain launch): the launch's a.B samples are decoder
// samples of which ctx_div consecutive ones share a context -- the candidates of a sampler call -- so sample b reads the k / v
// rows (the folded operands U, Wf, c) of context b / ctx_div.  The public argument structs keep their layout.
// kv_rows (here and in mdt_launch_attn_fwd_train / mdt_launch_attn_bwd; 0 or a.Tk = every key): a causal launch with Tk > 16 stages
// and multiplies its first kv_rows >= min(Tq, Tk) keys only -- the keys some query sees under the top-left aligned mask; a.Tk stays
// the K / V sample stride and the row length of the dropout index, and the backward leaves dk / dv rows kv_rows .. Tk-1 zero.
hipError_t mdt_launch_attention(const mdt_attn_args& a, const float* rope_cos, const float* rope_sin, hipStream_t s, int ctx_div = 1,
                                int kv_rows = 0);
// chunks of 17 .. 64 rows (mdt_attn_chunk.hip): where mdt_launch_attention, mdt_launch_attn_fwd_train and mdt_launch_attn_bwd go
// once max(Tq, Tk) > 16 -- head dim 32 / 48 / 64, Tq, Tk <= 64; rotary tables of max(Tq, Tk) positions x 16 frequencies
// (mdt_prefix_rows_ok -- the kv_rows the launchers and the *_prefix hooks of mdt_hip_debug.h accept --, mdt_attn_chunk_supported and
// mdt_attn_chunk_lds -- bytes of dynamic LDS of one workgroup; Tv = the keys it stages --: mdt_route_train.h)
constexpr int MDT_ROPE_POSITIONS = 64;   // rows of a handle's rotary tables
hipError_t mdt_launch_attn_chunk(const mdt_attn_args& a, const float* rope_cos, const float* rope_sin, hipStream_t s, int ctx_div, int kv_rows = 0);
hipError_t mdt_launch_attn_chunk_fwd_train(const mdt_attn_train_args& a, const mdt_attn_train_route& r, hipStream_t s);   // r: family CHUNK
hipError_t mdt_launch_attn_chunk_bwd(const mdt_attn_bwd_args& a, const mdt_attn_train_route& r, hipStream_t s);
// one sample's self-attention fused into its output projection p (rollout batch 1); see mdt_kernels.hip
hipError_t mdt_launch_attn_proj(const mdt_gemm_args& p, const float* qkv, int64_t ldq, int H, int hd, int T, int causal,
                                hipStream_t s);
// the same for a LARGE batch: the causal attention of a 32-row tile computed in the projection's prologue (k_attn_proj_wide)
hipError_t mdt_launch_attn_proj_wide(const mdt_gemm_args& p, const float* qkv, int64_t ldq, int H, int hd, int T, hipStream_t s);
// one workgroup per sample: self-attention -> projection -> collapsed cross-attention (k_attn_xattn); x.y == p.out
hipError_t mdt_launch_attn_xattn(const mdt_gemm_args& p, const float* qkv, int64_t ldq, const mdt_xapply_args& x, int H, int hd,
                                 int T, hipStream_t s, int ctx_div = 1, bool pair = false);   // pair: the projection on p.Wp_pair (fp16 pairs)
// side jobs (mdt_kernels.hip): small-M products that ride in the launches of the small-M products that follow them
hipError_t mdt_gemm_side_push(const mdt_gemm_args& a, hipStream_t s);
hipError_t mdt_gemm_side_push_front(const mdt_gemm_args& a, hipStream_t s);
hipError_t mdt_gemm_side_flush(hipStream_t s);
void mdt_gemm_side_drop();
size_t mdt_gemm_side_pending();                       // jobs still queued on this host thread
hipError_t mdt_gemm_side_launch_front(hipStream_t s);  // the head of the queue as a launch of its own
hipError_t mdt_launch_layernorm(const float* in, const float* w, const float* b, float* out, int M, int D,
                                hipStream_t s, float* out2 = nullptr);
hipError_t mdt_launch_sigma_emb(const float* sigma, int64_t sstride, const float* freqs, float* out, int R, int D,
                                hipStream_t s);
// the DDIM sampler's once-per-call scalar work in one launch: per-step scalars, the sigma embeddings of all steps, the first
// action embedding (mdt_kernels.hip: k_sample_prep); the schedule from device memory or, by value, from the host
constexpr int MDT_SCHED_MAX = 64;
struct mdt_sched_arg { float s[MDT_SCHED_MAX + 1]; };
hipError_t mdt_launch_sample_prep(const float* sigmas_dev, const float* sigmas_host, int n_steps, float* steps, const float* freqs,
                                  float* sig_e, int D, const float* x, float sd, const float* Wa, const float* ba, float* y, int M,
                                  int A, hipStream_t s, int Mx = 0);
// (Mx: rows of x; 0 = M.  The guided sampler passes M = 2 Mx: the embedding goes to both halves of y)
// the other samplers' once-per-call work (mdt_kernels.hip: k_sampler_plan + k_sampler_first): the plan of mdt_sampler_plan.h
// built on the device, the sigma embeddings of every evaluation (sig_e == nullptr: none), the first input Y_0 -> y0 (M, A), the
// four history slots hist (4, M, A) zeroed, and Y_0's action embedding -> y.  tq: nullptr, or (dpmpp_sde with tree noise) where
// the plan records its noise rows' points and the schedule's interval (mdt_sampler_plan.h)
struct mdt_tree_q;
// the tree of a tree-noise sampler call, checked before anything is enqueued (mdt_brownian.hip)
mdt_status mdt_check_brownian_source(const char* who, const mdt_brownian_source* src, int64_t batch, int64_t per_row);
hipError_t mdt_launch_sampler_prep(const float* sigmas_dev, const float* sigmas_host, int n_steps, int kind,
                                   const mdt_sampler_params& prm, mdt_sampler_plan_t* plan, const float* freqs, float* sig_e,
                                   int D, const float* x, const float* noise, int n_noise, float* y0, float* hist, float sd, const float* Wa,
                                   const float* ba, float* y, int M, int A, hipStream_t s, int Mx = 0, mdt_tree_q* tq = nullptr);
// the tree-noise rows of a dpmpp_sde call (mdt_brownian.hip: k_brownian_fill): rows (max_rows, nel) of the points the plan kernel
// recorded in tq (rows beyond tq->n are not written), from the trees of src (lo >= hi: tq's interval)
hipError_t mdt_launch_brownian_fill(const mdt_tree_q* tq, const mdt_brownian_source& src, int max_rows, int64_t nel, int64_t per_row,
                                    float* out, hipStream_t s);
// k_sampler_first alone (the adaptive DPM-Solver's per-attempt first input, from a plan uploaded by the host)
hipError_t mdt_launch_sampler_first(const mdt_sampler_plan_t* plan, const float* x, const float* noise, int n_noise, float* y0,
                                    float* hist, float sd, const float* Wa, const float* ba, float* y, int M, int A, int D,
                                    hipStream_t s, int Mx = 0);
// the adaptive DPM-Solver's scaled-error partial sums (mdt_kernels.hip: k_dpm_error): mdt_dpm_error_parts(nel) floats -> part
constexpr int MDT_DPM_PARTS = 256;
int mdt_dpm_error_parts(int64_t nel);
hipError_t mdt_launch_dpm_error(const float* lo, const float* hi, const float* prev, int64_t nel, float rtol, float atol,
                                float* part, hipStream_t s);
// operands of the head's plan epilogue (MDT_HEAD_PLAN): mdt_head_args.x is the evaluation's input Y, .out receives X'
struct mdt_head_plan {
    const mdt_sampler_eval* e;  // this evaluation's row of the plan (device)
    const float* xs;            // (M, A) the state X
    float* hist;                // (4, M, A) history slots H0..H3
    const float* noise;         // (n_noise, M, A) or nullptr (every noise operand reads as 0)
    float* y_out;               // (M, A) receives Y' (nullptr after the last evaluation; may alias mdt_head_args.x)
    int64_t nel;                // M * A
    int32_t n_noise;            // rows of `noise`: a plan row at or beyond it reads as 0 (the device plan is never trusted
                                // to stay inside the caller's buffer)
    // mdt_sample_opts (both pairs null: the epilogue as it was)
    const float *lo = nullptr, *hi = nullptr;      // (A,) bounds, both or neither: X' is clamped where e->ends_step
    float *rec_x = nullptr, *rec_d = nullptr;      // (M, A) both or neither: receive Y and D where e->begins_step
};
// classifier-free guidance of a sampler call (mdt_sample_*_guided): `on` = the call runs the doubled batch, conditional samples
// [0, B) and unconditional ones [B, 2B), and its heads combine the two halves with `lam`
struct mdt_guide {
    bool on = false;
    float lam = 1.f;
};
// pinned actions of a sampler call (mdt_sample_opts.pin_known / pin_keep): both (M, A) device rows, both or neither.  The head
// turns its denoised value D into keep == 0 ? D : keep == 1 ? known : D + keep (known - D) before anything else reads it
struct mdt_head_pin {
    const float *known = nullptr, *keep = nullptr;
};
// the action head on a.M rows: pl == nullptr the DDIM / denoiser head, else the plan head.  gd.on: the decoder rows of the a.M
// state rows are a.y's [0, M) (conditional) and [M, 2M) (unconditional); F = F_u + lam (F_g - F_u); y_next (if any) receives 2M rows
// pn: the call's pinned actions (the default: none)
hipError_t mdt_launch_head(const mdt_head_args& a, const mdt_head_plan* pl, mdt_guide gd, hipStream_t s, mdt_head_pin pn = {});
inline hipError_t mdt_launch_head(const mdt_head_args& a, hipStream_t s) { return mdt_launch_head(a, nullptr, mdt_guide(), s); }
// action vectors of 17 .. 64 elements (mdt_head_wide.hip): where mdt_launch_head goes once a.A > 16 -- the same launch in every
// mode, on 16-row MFMA tiles; D % 4 == 0, D <= 512, no slab input (y_parts <= 1).  mdt_head_wide_lds: bytes of dynamic LDS of one
// workgroup, checked against the 160 KiB of a workgroup before the launch (hipErrorInvalidValue, nothing enqueued)
constexpr int MDT_ACTION_DIM_MAX = 64;
size_t mdt_head_wide_lds(int D, int A, bool guided);
hipError_t mdt_launch_head_wide(const mdt_head_args& a, const mdt_head_plan* pl, mdt_guide gd, hipStream_t s, mdt_head_pin pn = {});
// the guided sampler's 2B encoder inputs (tokens and tokens2 twice, the goal then zeros) in one launch
hipError_t mdt_launch_guide_stage(const float* tok, const float* tok2, const float* goal, float* tok_o, float* tok2_o, float* goal_o,
                                  int B, int w1, int w2, int G, hipStream_t s);
hipError_t mdt_launch_action_embed(const float* x, const float* sigma, int64_t sstride, float sd, const float* Wa,
                                   const float* ba, float* y, int M, int A, int D, int rps, hipStream_t s);
// mdt_denoising_score (mdt_score.hip): the S levels and weights of a call by value; decoder sample ((b S + s) K + k) M + m is
// chunk k of observation b at level s with noise row m.  prep: the embedded input y (rows, D), the noised rows (rows, A), the
// samples' sigma (B S K M) and, where asked for, the contexts' (B S).  repeat: the encoder inputs of observation b at contexts
// b S .. b S + S - 1 (w2 == 0: no tokens2).  reduce: score (B K) from the raw network output F of those samples.
constexpr int MDT_SCORE_MAX = 64;
struct mdt_score_levels { float sigma[MDT_SCORE_MAX], weight[MDT_SCORE_MAX]; };
hipError_t mdt_launch_score_prep(const float* x0, const float* noise, const mdt_score_levels& lv, int64_t B, int S, int K, int M, int Ta,
                                 int A, int D, float sd, const float* Wa, const float* ba, float* y, float* noised, float* sig_rows,
                                 float* ctx_sig, hipStream_t s);
hipError_t mdt_launch_score_repeat(const float* tok, const float* tok2, const float* goal, float* tok_o, float* tok2_o, float* goal_o,
                                   int64_t B, int S, int w1, int w2, int wg, hipStream_t s);
hipError_t mdt_launch_score_reduce(const float* F, const float* x0, const float* noise, const mdt_score_levels& lv, int64_t B, int S,
                                   int K, int M, int E, float sd, float* score, hipStream_t s);
// mdt_sample*_select: per observation the index best_candidates gives on score (B K) and that chunk of chunks (B K, E) -> best (B, E)
hipError_t mdt_launch_score_select(const float* score, const float* chunks, int64_t B, int K, int E, float* best, int32_t* index,
                                   hipStream_t s);
hipError_t mdt_launch_noise_input(const float* act, const float* noise, const float* sigma, float* noised, int64_t n,
                                  int per_sample, hipStream_t s);
constexpr int MDT_LOSS_PARTS = 1024;   // floats of scratch mdt_launch_loss_reduce wants (`part`)
hipError_t mdt_launch_loss_reduce(const float* F, const float* act, const float* noised, const float* sigma, float sd,
                                  int64_t n, int per_sample, float* loss, float* part, hipStream_t s);
hipError_t mdt_launch_pack_weight(const float* w, int n_rows, int K, float* packed, int n_off, hipStream_t s);
hipError_t mdt_launch_pack_weight_glu(const float* w, int H, int K, float* packed, hipStream_t s);
// one move of a batched parameter upload (k_multi_load): src is (rows, K) row-major on the device
enum { MDT_LOAD_RAW = 0, MDT_LOAD_PACK = 1, MDT_LOAD_PACK_T = 2, MDT_LOAD_TRANSPOSE = 3, MDT_LOAD_PAD_COLS = 4,
       MDT_LOAD_PACK_SPLIT = 5,    // PACK_SPLIT: the three-way bf16 split fragment image (mdt_mlp_split.h); dst is a byte image of 6 rows K bytes
       MDT_LOAD_PACK_PAIR = 6 };   // PACK_PAIR: the fp16 pair image; ONE block per 16 source rows (its chunk index = the tile), p0 = n_off
struct mdt_load_entry {
    const float* src;
    float* dst;
    int32_t kind, rows, K;
    int32_t p0;  // PACK: first packed row (n_off);  PACK_T: k offset in the W^T image (n_off);  PAD_COLS: row pitch
    int32_t p1;  // PACK_T: 16-blocks along the image's k (= Lin.N / 16)
    int32_t pad_;
};
hipError_t mdt_launch_multi_load(const mdt_load_entry* tab, const int2* blocks, int n_blocks, hipStream_t s);
hipError_t mdt_launch_transpose(const float* src, float* dst, int R, int Cc, hipStream_t s);
hipError_t mdt_launch_xattn_fold(const mdt_xfold_args& a, hipStream_t s);
hipError_t mdt_launch_xattn_fold_n(const mdt_xfold_args* sets, int n, hipStream_t s);  // equal shapes; one launch per 8 sets
hipError_t mdt_launch_xattn_apply(const mdt_xapply_args& a, hipStream_t s, int ctx_div = 1);
// the collapsed cross-attention + the LayerNorm-prologue Linear on its output rows in one launch (k_xattn_gemm_smallm)
hipError_t mdt_launch_xattn_gemm(const mdt_xapply_args& x, const mdt_gemm_args& g, hipStream_t s, int ctx_div = 1);
size_t mdt_xattn_lds_floats(int D, int H);  // LDS floats of the collapsed cross-attention body (xattn_tile)
// x[(b * gout + goff + j)][:] += tab[j][:], j < gin, b < B: a (gin, D) table added to gin consecutive rows of every group of gout
hipError_t mdt_launch_add_group_rows(float* x, const float* tab, int64_t B, int gin, int gout, int goff, int D, hipStream_t s);
// ---- Perceiver resampler kernels ----
// media (B, T, n, D) + time_pos_emb[t] * mask[b][t] -> out (same shape); mask may be nullptr
hipError_t mdt_launch_add_time_emb(const float* media, const float* tpe, const uint8_t* mask, float* out, int64_t B,
                                   int T, int n, int D, hipStream_t s);
// out[b*R + r][:] = src[r][:]
hipError_t mdt_launch_bcast_rows(const float* src, float* out, int64_t B, int R, int D, hipStream_t s);
// softmax(q k^T * scale) v for few queries over many keys: q (B*Tq, H*64) ld ldq; k / v rows (B*Tk) ld ldkv
hipError_t mdt_launch_attention_long(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv,
                                     float* out, int64_t ldo, int B, int H, int hd, int Tq, int Tk, float scale,
                                     hipStream_t s);
bool mdt_attention_long_supported(int hd, int Tq, int Tk);
// ---- training-path kernels (mdt_train_kernels.hip) ----
hipError_t mdt_launch_pack_weight_t(const float* src, int rows, int cols, int64_t ld, float* packed, int k_off, int K16,
                                    hipStream_t s, int slice_len = 0);
hipError_t mdt_launch_transpose_ld(const float* src, int64_t lds_, float* dst, int64_t ldd, int R, int Cc, float* part,
                                   hipStream_t s, int slice_len = 0);
// floats of scratch mdt_linear_bwd needs for an (M, N, K) layer
int64_t mdt_linear_bwd_scratch(int64_t M, int64_t N, int64_t K);
// dW[n][k] = sum_m dY[m][n] X[m][k] from the row-major operands (mdt_train_kernels.hip: k_gemm_tn), S row slices of L rows; the tile
// is the route's (mdt_route_train.h: mdt_route_gemm_tn / mdt_route_gemm_tn_split)
hipError_t mdt_launch_gemm_tn(const float* dY, int64_t ldy, const float* X, int64_t ldx, float* out, int64_t slice_stride, int M, int N,
                              int K, int S, int L, int accumulate, float* bpart, hipStream_t s);
// the same product as three-way bf16 splits of both operands (k_gemm_tn_split: 128 x 128 / 128 x 192 tiles, 8 waves, 123 / 154 KB of LDS)
hipError_t mdt_launch_gemm_tn_split(const float* dY, int64_t ldy, const float* X, int64_t ldx, float* out, int64_t slice_stride, int M, int N,
                                    int K, int S, int L, int accumulate, float* bpart, hipStream_t s);
hipError_t mdt_launch_colsum2(const float* X0, const float* X1, int64_t ldx, int M, int N, float* out0, float* out1,
                              int accumulate, hipStream_t s);
hipError_t mdt_launch_ln_fwd_train(const mdt_ln_train_args& a, hipStream_t s);
hipError_t mdt_launch_ln_bwd(const mdt_ln_bwd_args& a, hipStream_t s);
// fused pairs of the training path (round 6): LayerNorm backward + the merge backward behind it; merge + the LayerNorm of its result
hipError_t mdt_launch_ln_bwd_merge(const mdt_ln_bwd_args& a, const mdt_merge_args& g, hipStream_t s);
hipError_t mdt_launch_merge_ln_fwd(const mdt_merge_args& g, const mdt_ln_train_args& l, hipStream_t s);
hipError_t mdt_launch_act_fwd(const float* u, float* out, int64_t n, int act, hipStream_t s);
hipError_t mdt_launch_act_bwd(const float* u, const float* dy, float* du, int64_t n, int act, hipStream_t s);
hipError_t mdt_launch_merge_fwd(const mdt_merge_args& a, hipStream_t s);
hipError_t mdt_launch_merge_bwd(const mdt_merge_args& a, hipStream_t s);
hipError_t mdt_launch_attn_fwd_train(const mdt_attn_train_args& a, hipStream_t s, int kv_rows = 0);
hipError_t mdt_launch_colsum(const float* X, int64_t ldx, int M, int N, float* out, int accumulate, hipStream_t s);
// a table of independent column sums run as one launch: dst[n] (+)= sum_m src[m * ld + n], m < M, n < N
struct mdt_colsum_entry {
    const float* src;
    float* dst;
    int64_t ld;
    int32_t M, N, accumulate;
};
enum { MDT_COLSUM_TABLE = 80 };  // entries per launch (passed by value: 80 x 40 B of kernel arguments)
struct mdt_colsum_table { mdt_colsum_entry e[MDT_COLSUM_TABLE]; };
hipError_t mdt_launch_colsum_batched(const mdt_colsum_entry* entries, int n, hipStream_t s);
hipError_t mdt_launch_attn_bwd(const mdt_attn_bwd_args& a, hipStream_t s, int kv_rows = 0);
hipError_t mdt_launch_loss_grad(const float* F, const float* act, const float* noised, const float* sigma, float sd,
                                int64_t n, int per_sample, const float* gscale, float* dF, hipStream_t s);
hipError_t mdt_launch_narrow_dx(const float* G, const float* W, float* out, int M, int A, int D, hipStream_t s);
// D = c_skip x + c_out F (den; may be nullptr) and the backward's seed dF = c_out g (g / dF; may be nullptr); its end
// out = c_in dxin + c_skip g; and d_sigma per sample (k_denoise_dsigma; d_e == nullptr: no sigma-embedding path)
hipError_t mdt_launch_denoise_seed(const float* F, const float* x, const float* sigma, const float* g, float sd, int64_t n,
                                   int per_sample, float* den, float* dF, hipStream_t s);
hipError_t mdt_launch_denoise_finish(const float* dxin, const float* sigma, const float* g, float sd, int64_t n, int per_sample,
                                     float* out, hipStream_t s);
hipError_t mdt_launch_denoise_dsigma(const float* g, const float* x, const float* F, const float* xin, const float* dxin,
                                     const float* e, const float* d_e, const float* freqs, const float* sigma, float sd, int B,
                                     int per_sample, int D, float* out, hipStream_t s);
// out[m][n] = act(b[n] + sum_a X[m][a] WT[a][n]), A <= 16; pre (optional): the pre-activation rows
hipError_t mdt_launch_narrow_linear(const float* X, const float* WT, const float* b, float* pre, float* out, int M, int A,
                                    int N, int act, hipStream_t s);
// out[m][a] = sum_d G[m][d] WT[a][d], A <= 16   (input gradient of the narrow-input Linear; WT is (A, D))
hipError_t mdt_launch_narrow_out(const float* G, int64_t ldg, const float* WT, float* out, int M, int A, int D, hipStream_t s);
hipError_t mdt_launch_narrow_dw(const float* G, const float* Y, int64_t ldy, float* partial, int n_slices, int M, int A,
                                int D, int transposed, hipStream_t s);
hipError_t mdt_launch_scaled_input(const float* x, const float* sigma, float sd, int64_t n, int per_sample, float* out,
                                   hipStream_t s);
hipError_t mdt_launch_gather_rows(const float* src, float* dst, int M, int D, int gin, int gout, int goff, hipStream_t s);
hipError_t mdt_launch_dropout_rows(float* x, int64_t rows, int D, int rows_per_sample, int row_lo, float p, uint32_t site,
                                   uint64_t seed, hipStream_t s);
hipError_t mdt_launch_add_inplace(const float* x, float* y, int64_t n, hipStream_t s);
// dst[r][c] += src[r][c] for r < rows, c < cols (leading dimensions lds_ / ldd)
hipError_t mdt_launch_add_2d(const float* src, int64_t lds_, float* dst, int64_t ldd, int rows, int cols, hipStream_t s);
// backward of a Linear through the forward GEMM kernel (mdt_train.hip); see mdt_linear_bwd_args
// defer_bias (optional, with bias_space of at least 256 * N floats that stay valid until the caller runs the entry): the
// per-slice bias partials are left in bias_space and *defer_bias describes their final column sum instead of launching it
// (defer_bias->src == nullptr on return: the bias gradient was produced another way, nothing to run).
mdt_status mdt_linear_bwd(const mdt_linear_bwd_args& a, hipStream_t s, mdt_colsum_entry* defer_bias = nullptr,
                          float* bias_space = nullptr);
hipError_t mdt_launch_attention_long_bwd(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldkv,
                                         const float* d_out, int64_t ld_do, float* dq, int64_t ld_dq, float* dk, float* dv,
                                         int64_t ld_dkv, int B, int H, int hd, int Tq, int Tk, float scale, hipStream_t s,
                                         float* dkl = nullptr, int F = 0);  // F > 0: keys < F -> dk / dv (B*F rows), the rest -> dkl
bool mdt_attention_long_bwd_supported(int hd, int Tq, int Tk);
hipError_t mdt_launch_time_emb_grad(const float* dxf, const uint8_t* mask, float* out, float* partial, int64_t B, int T, int n,
                                    int D, int accumulate, hipStream_t s);  // partial: B*T*D floats of scratch
hipError_t mdt_launch_multi_adamw(const mdt_opt_tensor* tab, const int2* blocks, int n_blocks, float lr, float beta1,
                                  float beta2, float eps, float wd, float bc1, float bc2_sqrt, hipStream_t s);
hipError_t mdt_launch_multi_axpby(const mdt_opt_tensor* tab, const int2* blocks, int n_blocks, float a, float b,
                                  hipStream_t s);
// partial: 2 * n_blocks floats; out[0] = sum of squares of the g (which = 0) or p (1) members, out[1] = non-finite count
hipError_t mdt_launch_multi_sumsq(const mdt_opt_tensor* tab, const int2* blocks, int n_blocks, int which, float* partial,
                                  float* out, hipStream_t s);
// k_opt_ctl writes ctl (4 floats, 16-byte aligned) from the device scalars, k_multi_adamw_dev reads it
hipError_t mdt_launch_multi_adamw_dev(const mdt_opt_tensor* tab, const int2* blocks, int n_blocks, float lr, float beta1,
                                      float beta2, float eps, float wd, float* step, const float* grad_scale,
                                      const float* found_inf, const float* grad_sumsq, float max_norm, float* ctl,
                                      float* grad_norm, hipStream_t s);
// RMSNorm / SwishGLU row kernels (mdt_map_pool.hip), shared with the masked-image decoder's ops (mdt_mae.hip)
hipError_t mdt_launch_rms_fwd(const float* x, const float* g, float* out, int64_t M, int D, float eps, hipStream_t s);
hipError_t mdt_launch_rms_bwd(const float* x, const float* g, const float* dy, float* dx, int accumulate, float* pg, int64_t M,
                              int D, float eps, hipStream_t s, const float* res = nullptr);
hipError_t mdt_launch_swiglu_fwd(const float* u, float* out, int64_t M, int Hm, hipStream_t s);
hipError_t mdt_launch_swiglu_bwd(const float* u, const float* d_out, float* du, int64_t M, int Hm, hipStream_t s);
struct mdt_model;
void mdt_train_free(mdt_model* m);  // releases what mdt_train_prepare() and the tapes allocated (mdt_train.hip)
