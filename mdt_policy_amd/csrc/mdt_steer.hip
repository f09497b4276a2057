// mdt_steer.hip -- mdt_sample_ddim_steer and mdt_sample_steer (include/mdt_hip_train.h): DDIM, and every sampler of a plan
// (mdt_sampler_plan.h), steered toward known actions through the denoiser's Jacobian, as one enqueue.
//
// A steer is (known, weight, beta).  Wherever the sampler used D(x; sigma) it uses
//     D'(x; sigma) = D + s(sigma) J^T (weight . (known - D)),   J = dD/dx,   s(sigma) = min(beta, 1 + sigma^2 / sigma_data^2)
// (pseudo-inverse guidance as real-time chunking clips it; e = weight . (known - D) is a constant of the step).  The denoiser and
// its vector-Jacobian product are the training path's, shared with mdt_log_likelihood (mdt_loglik.h): the encoder and the cross
// K|V once per call on the B observations (once per step where sigma is a context token), per step one tape-keeping decoder
// forward on the R = B * K chunks and one input-gradient-only backward over that tape.  This file holds the kernels that stand
// where mdt_ll_vjp's seed and finish launches stand -- the seed forms D and e on the way, the finish the steered update -- and one
// host loop, `evaluations`, that both entries run: per evaluation the context where sigma is a token, the forward, the backward
// between the seed and the entry's finish.  An entry brings its first launch (the rows' sigma), a setter for what changes per
// evaluation, and its finish: DDIM k_steer_step, with the coefficients formed on the host; mdt_sample_steer, per evaluation of a
// sampler plan on the evaluation's input Y at its own sigma, k_steer_plan -- D' and then the plan's per-element update
// (head_plan_elem, the one the unsteered plan heads call) on X, Y, D', d = (Y - D') / sigma, H0..H3, N0, N1.  Both entries stand
// in mdt_loglik.h's frame: head checks, their own, tail checks, then mdt_ll_scoped around the loop.
// No kernel here uses atomics, LDS or scratch; every element is written by one thread.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mdt_hip_debug.h"
#include "mdt_hip_train.h"
#include "mdt_internal.h"
#include "mdt_launch.h"
#include "mdt_device.h"
#include "mdt_edm.h"
#include "mdt_loglik.h"
#include "mdt_sampler_plan.h"
#include "mdt_tiles.h"

#define fail mdt_fail

namespace {

// Every kernel: 256 threads (four wave64), grid-stride over the N = R * Ta * A elements.  Ta * A = 70 is no multiple of 64 and N
// rarely one of 256: the bound is per element, and no lane cooperates with another, so a partly filled wave just idles its tail.
constexpr int STEER_THREADS = 256;
constexpr int STEER_MAX_BLOCKS = 1024;
constexpr const char* NOT_CAPTURE_SAFE = "the tape path is not capture-safe and the call";  // ... cannot be captured

unsigned steer_grid(int64_t n) {
    const int64_t g = (n + STEER_THREADS - 1) / STEER_THREADS;
    return (unsigned)(g < 1 ? 1 : (g > STEER_MAX_BLOCKS ? STEER_MAX_BLOCKS : g));
}

// The seed of the backward and the constraint error in one pass over the tape's F and x (k_denoise_seed's arithmetic, sigma
// shared by all rows): D = c_skip x + c_out F;  e = weight (known - D);  dF = c_out e.
__global__ __launch_bounds__(STEER_THREADS) void k_steer_seed(const float* __restrict__ F, const float* __restrict__ x,
                                                              const float* __restrict__ known, const float* __restrict__ weight,
                                                              float sg, float sd, int64_t N, float* __restrict__ D,
                                                              float* __restrict__ e, float* __restrict__ dF) {
    const float den2 = edm_den2_round_sd(sg, sd);
    const float c_skip = edm_c_skip(sd, den2), c_out = edm_c_out(sg, sd, den2);
    for (int64_t i = (int64_t)blockIdx.x * STEER_THREADS + threadIdx.x; i < N; i += (int64_t)gridDim.x * STEER_THREADS) {
        const float d = edm_denoised(F[i], x[i], c_out, c_skip);
        const float ev = weight[i] * (known[i] - d);
        D[i] = d;
        e[i] = ev;
        dF[i] = c_out * ev;
    }
}

// The end of the backward and the steered DDIM step over the N elements, the R per-row sigma entries behind them
// (k_denoise_finish's arithmetic): g = c_in small + c_skip e;  D' = D + scale g;  x_out = ratio x_in + coef D', clamped to
// [lo, hi] per action dimension as torch.clamp does (NaN stays, lo > hi gives hi) where bounds are given;  sig_rows = the next
// forward's sigma.  x_in and x_out may be the same buffer (each element is read and written by its own thread), so neither is
// __restrict__; x_in is only read.  N == 0: only the sigma rows (the first forward's).
__global__ __launch_bounds__(STEER_THREADS) void k_steer_step(const float* __restrict__ small, const float* __restrict__ e,
                                                              const float* __restrict__ D, const float* x_in, float sg, float sd,
                                                              float scale, float ratio, float coef, const float* __restrict__ lo,
                                                              const float* __restrict__ hi, int A, float sigma_next, int64_t N,
                                                              int64_t R, float* x_out, float* __restrict__ sig_rows) {
    const float den2 = edm_den2_round_sd(sg, sd);
    const float c_in = edm_c_in(den2), c_skip = edm_c_skip(sd, den2);
    for (int64_t i = (int64_t)blockIdx.x * STEER_THREADS + threadIdx.x; i < N + R; i += (int64_t)gridDim.x * STEER_THREADS) {
        if (i < N) {
            const float g = fmaf(small[i], c_in, e[i] * c_skip);
            const float dp = D[i] + scale * g;
            float v = ratio * x_in[i] + coef * dp;
            if (lo) {
                const int a = (int)(i % A);
                const float l = lo[a], h = hi[a];
                v = v < l ? l : v;
                v = v > h ? h : v;
            }
            x_out[i] = v;
        } else {
            sig_rows[i - N] = sigma_next;
        }
    }
}


// The first launch of a plan call over the N elements, the R sigma entries behind them (k_sampler_first's arithmetic without the
// embedding): Y_0 = x_T + y0_cn N[y0_noise] (n0: that noise row or null), X = x_T, the four history slots zero -- a zero
// coefficient does not neutralise what an earlier call left there -- and the rows' sigma for the first forward.  x_T is only read.
__global__ __launch_bounds__(STEER_THREADS) void k_steer_first(const float* __restrict__ x_T, const float* __restrict__ n0, float cn,
                                                               float sigma0, int64_t N, int64_t R, float* __restrict__ X,
                                                               float* __restrict__ Y, float* __restrict__ hist,
                                                               float* __restrict__ sig_rows) {
    for (int64_t i = (int64_t)blockIdx.x * STEER_THREADS + threadIdx.x; i < N + R; i += (int64_t)gridDim.x * STEER_THREADS) {
        if (i < N) {
            float v = x_T[i];
            if (n0 != nullptr && cn != 0.f) v = v + n0[i] * cn;
            X[i] = x_T[i];
            Y[i] = v;
#pragma unroll
            for (int h = 0; h < 4; ++h) hist[h * N + i] = 0.f;
        } else {
            sig_rows[i - N] = sigma0;
        }
    }
}

// what one evaluation of a steered plan call hands its finish launch: the evaluation's row of the plan by value (cx, cy, push,
// the noise rows, the step marks, sigma_next), and the call's buffers
struct SteerPlanArgs {
    mdt_sampler_eval ev;
    const float *small, *e, *D;  // the backward's result at the network's input, the seed's e and D
    const float* Y;              // (N) this evaluation's input; y_out may be the same buffer
    const float* X;              // (N) the state; x_out may be the same buffer
    float *x_out, *y_out;        // X' (the call's `out` after the last evaluation);  Y' or null after the last evaluation
    float* hist;                 // (4, N)
    const float* noise;          // (n_noise, N) or null: every noise operand reads as 0
    const float *lo, *hi;        // (A,) or null: where this evaluation's step is clipped at all (mdt_plan_loop_clips)
    float* rec;                  // (2, N) this step's record rows or null
    float* sig_rows;             // (R)
    int64_t N, R;
    float sd, scale;
    int32_t n_noise, A;
};

// The end of the backward and one evaluation of a sampler plan over the N elements, the R per-row sigma entries behind them:
// g = c_in small + c_skip e;  D' = D + scale g;  then head_plan_elem with D' as the denoised value -- X' = sum cx R clamped to
// [lo, hi] where the evaluation ends a step, Y' = cy[NREG] X' + sum cy R, the record rows (Y, D') where it begins one, the history
// shift -- and sig_rows = sigma_next.  X / x_out, Y / y_out and the history slots are read and written in place: each element by
// its own thread, every read before the write, so none of them is __restrict__.
__global__ __launch_bounds__(STEER_THREADS) void k_steer_plan(SteerPlanArgs a) {
    const float sg = a.ev.sigma, den2 = edm_den2_round_sd(sg, a.sd);
    const float c_in = edm_c_in(den2), c_skip = edm_c_skip(a.sd, den2);
    float cx[MDT_SAMPLER_NREG], cy[MDT_SAMPLER_NREG + 1];
#pragma unroll
    for (int k = 0; k < MDT_SAMPLER_NREG; ++k) { cx[k] = a.ev.cx[k]; cy[k] = a.ev.cy[k]; }
    cy[MDT_SAMPLER_NREG] = a.ev.cy[MDT_SAMPLER_NREG];
    const int push = a.ev.push;
    const bool clip = a.lo != nullptr && a.ev.ends_step != 0;
    const bool rec = a.rec != nullptr && a.ev.begins_step != 0;
    const int nn = a.noise != nullptr ? a.n_noise : 0;  // rows outside [0, n_noise) read as 0
    const float* n0 = (a.ev.noise[0] >= 0 && a.ev.noise[0] < nn) ? a.noise + a.ev.noise[0] * a.N : nullptr;
    const float* n1 = (a.ev.noise[1] >= 0 && a.ev.noise[1] < nn) ? a.noise + a.ev.noise[1] * a.N : nullptr;
    const mdt_head_plan pl = {nullptr, a.X, a.hist, a.noise, a.y_out, a.N, nn, a.lo, a.hi, a.rec, a.rec ? a.rec + a.N : nullptr};
    for (int64_t i = (int64_t)blockIdx.x * STEER_THREADS + threadIdx.x; i < a.N + a.R; i += (int64_t)gridDim.x * STEER_THREADS) {
        if (i < a.N) {
            const float g = fmaf(a.small[i], c_in, a.e[i] * c_skip);
            const float dp = a.D[i] + a.scale * g;
            float l = 0.f, h = 0.f;
            if (clip) {
                const int c = (int)(i % a.A);
                l = a.lo[c]; h = a.hi[c];
            }
            float xn, yn;
            head_plan_elem(&pl, cx, cy, push, clip, rec, a.N, n0, n1, i, a.Y[i], dp, sg, l, h, true, xn, yn);
            a.x_out[i] = xn;
        } else {
            a.sig_rows[i - a.N] = a.ev.sigma_next;
        }
    }
}

// the call's buffers over one device block (y and hist: the plan call's)
struct SteerBufs {
    float *x, *D, *e, *sig, *y, *hist;
};

void carve(Bump& b, int64_t rows, int per, SteerBufs* o) {
    SteerBufs t;
    t.x = b.take(rows * per); t.D = b.take(rows * per); t.e = b.take(rows * per); t.sig = b.take(rows);
    t.y = b.take(rows * per); t.hist = b.take(4 * rows * per);
    if (o) *o = t;
}

struct Call {
    mdt_model* m;
    mdt_ll_run run;
    hipStream_t s;
    const float *tokens, *tokens2, *goal, *known, *weight, *lo, *hi;
    int modality;
    int64_t R, N;
    SteerBufs b;
    // the step under way
    float sg, scale, ratio, coef, sigma_next;
    const float* x_in;
    float* x_out;
    // the plan call: the evaluation under way
    SteerPlanArgs pa;
};

hipError_t steer_seed(const mdt_ll_io& io, void* arg, hipStream_t s) {
    const Call& c = *(const Call*)arg;
    return mdt_launch_lds<k_steer_seed>(dim3(steer_grid(c.N)), dim3(STEER_THREADS), 0, s, io.F, io.x, c.known, c.weight, c.sg, io.sd,
                                        c.N, c.b.D, c.b.e, io.dF);
}

hipError_t steer_step(const mdt_ll_io& io, void* arg, hipStream_t s) {
    const Call& c = *(const Call*)arg;
    return mdt_launch_lds<k_steer_step>(dim3(steer_grid(c.N + c.R)), dim3(STEER_THREADS), 0, s, (const float*)io.small,
                                        (const float*)c.b.e, (const float*)c.b.D, c.x_in, c.sg, io.sd, c.scale, c.ratio, c.coef,
                                        c.lo, c.hi, c.m->A, c.sigma_next, c.N, c.R, c.x_out, c.b.sig);
}

hipError_t steer_plan(const mdt_ll_io& io, void* arg, hipStream_t s) {
    const Call& c = *(const Call*)arg;
    SteerPlanArgs a = c.pa;
    a.small = io.small;
    return mdt_launch_lds<k_steer_plan>(dim3(steer_grid(c.N + c.R)), dim3(STEER_THREADS), 0, s, a);
}

// the rows' sigma for the first forward (k_steer_step over no elements)
mdt_status fill_sigma(Call& c, float sigma) {
    LAUNCH(mdt_launch_lds<k_steer_step>(dim3(steer_grid(c.R)), dim3(STEER_THREADS), 0, c.s, (const float*)nullptr,
                                        (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 1.f, 1.f, 0.f, 0.f, 0.f,
                                        (const float*)nullptr, (const float*)nullptr, 1, sigma, (int64_t)0, c.R, (float*)nullptr,
                                        c.b.sig));
    return MDT_OK;
}

// The evaluations of a steered call, after its first launch has filled the rows' sigma.  `set(i)` fills what evaluation i's seed
// and finish launches read from `c` and returns the forward's input; the context is hoisted unless sigma is one of its tokens.
template <class Set>
mdt_status evaluations(Call& c, int n, Set set, mdt_ll_launch finish, float* ctx_out) {
    mdt_model* m = c.m;
    if (m->cond != COND_TOKEN) MDT_TRY(mdt_ll_context(m, c.run, c.tokens, c.tokens2, c.goal, c.modality, nullptr, c.s));
    for (int i = 0; i < n; ++i) {
        const float* x = set(i);
        if (m->cond == COND_TOKEN)  // sigma is a context token: the context is this evaluation's, still on the B observations
            MDT_TRY(mdt_ll_context(m, c.run, c.tokens, c.tokens2, c.goal, c.modality, c.b.sig, c.s));
        MDT_TRY(mdt_ll_forward(m, c.run, x, c.b.sig, c.s));
        MDT_TRY(mdt_ll_backward(m, c.run, steer_seed, finish, &c, c.s));
    }
    if (ctx_out)
        HIP_TRY(hipMemcpyAsync(ctx_out, mdt_ll_ctx(m, c.run), (size_t)c.run.B * m->Te * m->D * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    return MDT_OK;
}

// DDIM's steps: forward on x, backward between k_steer_seed and k_steer_step
mdt_status run(Call& c, const float* x_T, const float* sig, int n, float beta, float* out, float* ctx_out) {
    const float sd = c.m->cfg.sigma_data;
    MDT_TRY(fill_sigma(c, sig[0]));
    return evaluations(c, n, [&](int i) {
        // the DDIM coefficients as the native sampler forms them (k_sample_prep): t = -ln sigma, exp(-t') / exp(-t), -expm1(-(t' - t))
        const float t = -logf(sig[i]), tn = -logf(sig[i + 1]);
        c.sg = sig[i];
        c.ratio = expf(-tn) / expf(-t);
        c.coef = -expm1f(-(tn - t));
        c.scale = fminf(beta, 1.f + (sig[i] * sig[i]) / (sd * sd));
        c.sigma_next = sig[i + 1];
        c.x_in = i == 0 ? x_T : c.b.x;       // x_T is only read
        c.x_out = i == n - 1 ? out : c.b.x;
        return c.x_in;
    }, steer_step, ctx_out);
}

// the plan's evaluations: forward on Y, backward between k_steer_seed and k_steer_plan
mdt_status run_plan(Call& c, int kind, int n_steps, const mdt_sampler_plan_t& P, const float* x_T, const float* noise, int n_noise,
                    float beta, float* record, float* out, float* ctx_out) {
    const float sd = c.m->cfg.sigma_data;
    const int E = P.n_evals;
    const float* y0n = (noise && P.y0_noise >= 0 && P.y0_noise < n_noise) ? noise + (int64_t)P.y0_noise * c.N : nullptr;
    LAUNCH(mdt_launch_lds<k_steer_first>(dim3(steer_grid(c.N + c.R)), dim3(STEER_THREADS), 0, c.s, x_T, y0n, P.y0_cn, P.e[0].sigma,
                                         c.N, c.R, c.b.x, c.b.y, c.b.hist, c.b.sig));
    SteerPlanArgs& a = c.pa;  // the call's buffers and sizes once, the evaluation's own fields in the setter
    a.small = nullptr; a.e = c.b.e; a.D = c.b.D;
    a.Y = c.b.y; a.X = c.b.x;
    a.hist = c.b.hist;
    a.noise = noise;
    a.sig_rows = c.b.sig;
    a.N = c.N; a.R = c.R;
    a.sd = sd;
    a.n_noise = noise ? n_noise : 0;
    a.A = c.m->A;
    return evaluations(c, E, [&](int e) {
        const bool last = e == E - 1, clips = c.lo && mdt_plan_loop_clips(kind, last);
        const float sg = P.e[e].sigma;
        c.sg = sg;
        a.ev = P.e[e];
        a.x_out = last ? out : c.b.x;
        a.y_out = last ? nullptr : c.b.y;
        a.lo = clips ? c.lo : nullptr; a.hi = clips ? c.hi : nullptr;
        a.rec = record ? record + (int64_t)mdt_plan_step_of(kind, n_steps, e) * 2 * c.N : nullptr;
        a.scale = fminf(beta, 1.f + (sg * sg) / (sd * sd));
        return (const float*)c.b.y;
    }, steer_plan, ctx_out);
}

// the call's arguments and, over the handle's steer block grown to R rows, its buffers
mdt_status steer_call(Call& c, mdt_model* m, hipStream_t s, const float* tokens, const float* tokens2, const float* goal, int modality,
                      int64_t R, const float* known, const float* weight, const float* lo, const float* hi) {
    c.m = m; c.s = s; c.tokens = tokens; c.tokens2 = tokens2; c.goal = goal; c.known = known; c.weight = weight; c.lo = lo; c.hi = hi;
    c.modality = modality; c.R = R; c.N = R * m->Ta * m->A;
    const int per = m->Ta * m->A;
    return mdt_grow_carve(m->st_ws, m->st_rows, R, [&](Bump& b, int64_t rows) { carve(b, rows, per, b.base ? &c.b : nullptr); });
}

}  // namespace

extern "C" mdt_status mdt_sample_ddim_steer(mdt_model* m, const float* tokens, const float* tokens2, const float* goal,
                                            int32_t modality, const float* x_T, const float* sigmas, int32_t n_steps,
                                            int64_t batch, int32_t candidates, const float* known, const float* weight, float beta,
                                            const float* lo, const float* hi, float* out, float* ctx_out, void* stream) {
    const char* fn = "mdt_sample_ddim_steer";
    MDT_TRY(mdt_ll_check_head(fn, m, tokens, goal, {{x_T, "x_T"}, {sigmas, "sigmas"}, {known, "known"}, {weight, "weight"}, {out, "out"}},
                              batch, candidates));
    if (n_steps < 1 || n_steps > MDT_SAMPLER_MAX_STEPS)
        return fail(MDT_ERR_INVALID_ARG, "%s: n_steps is %d, must be in [1, %d]", fn, n_steps, (int)MDT_SAMPLER_MAX_STEPS);
    if (!std::isfinite(beta) || !(beta > 0.f)) return fail(MDT_ERR_INVALID_ARG, "%s: beta is %g, must be finite and > 0", fn, beta);
    for (int i = 0; i < n_steps; ++i)
        if (!std::isfinite(sigmas[i]) || !(sigmas[i] > 0.f))
            return fail(MDT_ERR_INVALID_ARG, "%s: sigmas[%d] is %g: the schedule must be finite and > 0, then end in 0", fn, i, sigmas[i]);
    if (sigmas[n_steps] != 0.f)
        return fail(MDT_ERR_INVALID_ARG, "%s: sigmas[%d] is %g: the schedule must be finite and > 0, then end in 0", fn, n_steps,
                    sigmas[n_steps]);
    if ((!lo) != (!hi)) return fail(MDT_ERR_INVALID_ARG, "%s: null %s: the bounds lo and hi come together", fn, lo ? "hi" : "lo");
    hipStream_t s = (hipStream_t)stream;
    MDT_TRY(mdt_ll_check_tail(m, fn, tokens2, batch, candidates, s, NOT_CAPTURE_SAFE));

    Call c;
    MDT_TRY(steer_call(c, m, s, tokens, tokens2, goal, modality, batch * candidates, known, weight, lo, hi));
    return mdt_ll_scoped(m, batch, candidates, s, &c.run, [&] { return run(c, x_T, sigmas, n_steps, beta, out, ctx_out); });
}

extern "C" mdt_status mdt_sample_steer(mdt_model* m, const float* tokens, const float* tokens2, const float* goal, int32_t modality,
                                       const float* x_T, int32_t kind, const mdt_sampler_params* params, const float* sigmas_host,
                                       int32_t n_steps, const float* noise, int32_t n_noise, int64_t batch, int32_t candidates,
                                       const float* known, const float* weight, float beta, const float* lo, const float* hi,
                                       float* record, float* out, float* ctx_out, void* stream) {
    const char* fn = "mdt_sample_steer";
    MDT_TRY(mdt_ll_check_head(fn, m, tokens, goal,
                              {{x_T, "x_T"}, {sigmas_host, "sigmas_host"}, {known, "known"}, {weight, "weight"}, {out, "out"}}, batch,
                              candidates));
    if (!std::isfinite(beta) || !(beta > 0.f)) return fail(MDT_ERR_INVALID_ARG, "%s: beta is %g, must be finite and > 0", fn, beta);
    const mdt_sampler_params p = params ? *params : mdt_sampler_defaults();
    int E = 0, rows = 0;
    switch (mdt_plan_shape(kind, p, n_steps, &E, &rows)) {
        case MDT_PLAN_OK: break;
        case MDT_PLAN_BAD_KIND:
            return fail(MDT_ERR_INVALID_ARG, "%s: kind is %d, must be an mdt_sampler_kind in [0, %d)", fn, kind, (int)MDT_SAMPLER_COUNT);
        case MDT_PLAN_BAD_STEPS:
            return fail(MDT_ERR_INVALID_ARG, "%s: n_steps is %d, must be in [1, %d]%s", fn, n_steps, mdt_plan_max_n(kind),
                        kind == MDT_SAMPLER_DPM_FAST ? " (dpm_fast's evaluations)" : "");
        default:
            return fail(MDT_ERR_INVALID_ARG, "%s: params.order is %d, lms takes 1..4", fn, p.order);
    }
    const int levels = mdt_plan_levels(kind, n_steps);
    const char* rule = kind == MDT_SAMPLER_DPM_FAST ? "dpm_fast takes the two levels {sigma_max, sigma_min}, finite and > 0"
                                                    : "the schedule must be finite and > 0, then end in 0";
    for (int i = 0; i < levels; ++i) {
        const bool zero = kind != MDT_SAMPLER_DPM_FAST && i == levels - 1;
        const float v = sigmas_host[i];
        if (zero ? v != 0.f : (!std::isfinite(v) || !(v > 0.f)))
            return fail(MDT_ERR_INVALID_ARG, "%s: sigmas_host[%d] is %g: %s", fn, i, v, rule);
    }
    if (mdt_plan_check_levels(kind, p, sigmas_host) != MDT_PLAN_OK)
        return fail(MDT_ERR_INVALID_ARG, "%s: params.eta is %g: dpm_fast with eta != 0 needs sigma_min < sigma_max (sigmas_host is {%g, %g})",
                    fn, p.eta, sigmas_host[0], sigmas_host[1]);
    if ((!lo) != (!hi)) return fail(MDT_ERR_INVALID_ARG, "%s: null %s: the bounds lo and hi come together", fn, lo ? "hi" : "lo");
    static thread_local mdt_sampler_plan_t P;
    MDT_TRY(mdt_sampler_plan(kind, &p, sigmas_host, n_steps, &P));
    if (!noise && mdt_plan_needs_noise(kind, p))
        return fail(MDT_ERR_INVALID_ARG, "%s: null noise: this sampler and parameter set read %d noise rows", fn, P.n_noise);
    if (noise && n_noise < P.n_noise)
        return fail(MDT_ERR_INVALID_ARG, "%s: n_noise is %d, the sampler reads %d noise rows", fn, n_noise, P.n_noise);
    for (int e = 0; record && e < P.n_evals; ++e)  // the record's rows are placed by the structure: it must be the plan's
        if (P.e[e].step != mdt_plan_step_of(kind, n_steps, e))
            return fail(MDT_ERR_STATE, "%s: evaluation %d is in step %d of the plan, %d by its structure", fn, e, P.e[e].step,
                        mdt_plan_step_of(kind, n_steps, e));
    hipStream_t s = (hipStream_t)stream;
    MDT_TRY(mdt_ll_check_tail(m, fn, tokens2, batch, candidates, s, NOT_CAPTURE_SAFE));

    Call c;
    MDT_TRY(steer_call(c, m, s, tokens, tokens2, goal, modality, batch * candidates, known, weight, lo, hi));
    return mdt_ll_scoped(m, batch, candidates, s, &c.run,
                         [&] { return run_plan(c, kind, n_steps, P, x_T, noise, n_noise, beta, record, out, ctx_out); });
}

// ------------------------------------------------------------------------------------------------
// test hooks (mdt_hip_debug.h): the four kernels above on the caller's buffers, each through the launch its entry point makes --
// steer_grid of what the entry passes, STEER_THREADS, mdt_launch_lds.  What a model call guarantees by construction is checked here.
// ------------------------------------------------------------------------------------------------
namespace {

struct Named {
    const void* p;
    const char* name;
};

mdt_status hook_nulls(const char* fn, std::initializer_list<Named> ps) {
    for (const Named& n : ps)
        if (!n.p) return fail(MDT_ERR_INVALID_ARG, "%s: null %s", fn, n.name);
    return MDT_OK;
}

mdt_status hook_sizes(const char* fn, int64_t N, int64_t R) {
    if (N < 0) return fail(MDT_ERR_INVALID_ARG, "%s: N is %lld, must be >= 0", fn, (long long)N);
    if (R < 0) return fail(MDT_ERR_INVALID_ARG, "%s: R is %lld, must be >= 0", fn, (long long)R);
    if (N + R < 1) return fail(MDT_ERR_INVALID_ARG, "%s: N + R is 0: nothing to launch over", fn);
    return MDT_OK;
}

mdt_status hook_positive(const char* fn, const char* name, float v) {
    if (!std::isfinite(v) || !(v > 0.f)) return fail(MDT_ERR_INVALID_ARG, "%s: %s is %g, must be finite and > 0", fn, name, v);
    return MDT_OK;
}

mdt_status hook_bounds(const char* fn, const float* lo, const float* hi, int32_t A, int64_t N) {
    if (A < 1) return fail(MDT_ERR_INVALID_ARG, "%s: A is %d, must be >= 1", fn, A);
    if ((!lo) != (!hi)) return fail(MDT_ERR_INVALID_ARG, "%s: null %s: the bounds lo and hi come together", fn, lo ? "hi" : "lo");
    if (lo && N % A != 0)
        return fail(MDT_ERR_INVALID_ARG, "%s: N is %lld, no multiple of A = %d: the bounds are per column of rows of A", fn,
                    (long long)N, A);
    return MDT_OK;
}

}  // namespace

extern "C" mdt_status mdt_op_steer_seed(const float* F, const float* x, const float* known, const float* weight, float sigma, float sd,
                                        int64_t N, float* D, float* e, float* dF, void* stream) {
    const char* fn = "mdt_op_steer_seed";
    MDT_TRY(hook_nulls(fn, {{F, "F"}, {x, "x"}, {known, "known"}, {weight, "weight"}, {D, "D"}, {e, "e"}, {dF, "dF"}}));
    if (N < 1) return fail(MDT_ERR_INVALID_ARG, "%s: N is %lld, must be >= 1", fn, (long long)N);
    MDT_TRY(hook_positive(fn, "sigma", sigma));
    MDT_TRY(hook_positive(fn, "sd", sd));
    LAUNCH(mdt_launch_lds<k_steer_seed>(dim3(steer_grid(N)), dim3(STEER_THREADS), 0, (hipStream_t)stream, F, x, known, weight, sigma, sd,
                                        N, D, e, dF));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_steer_step(const float* small, const float* e, const float* D, const float* x_in, float sigma, float sd,
                                        float scale, float ratio, float coef, const float* lo, const float* hi, int32_t A,
                                        float sigma_next, int64_t N, int64_t R, float* x_out, float* sig_rows, void* stream) {
    const char* fn = "mdt_op_steer_step";
    MDT_TRY(hook_sizes(fn, N, R));
    if (N > 0) MDT_TRY(hook_nulls(fn, {{small, "small"}, {e, "e"}, {D, "D"}, {x_in, "x_in"}, {x_out, "x_out"}}));
    if (R > 0) MDT_TRY(hook_nulls(fn, {{sig_rows, "sig_rows"}}));
    MDT_TRY(hook_bounds(fn, lo, hi, A, N));
    MDT_TRY(hook_positive(fn, "sigma", sigma));
    MDT_TRY(hook_positive(fn, "sd", sd));
    LAUNCH(mdt_launch_lds<k_steer_step>(dim3(steer_grid(N + R)), dim3(STEER_THREADS), 0, (hipStream_t)stream, small, e, D, x_in, sigma,
                                        sd, scale, ratio, coef, lo, hi, (int)A, sigma_next, N, R, x_out, sig_rows));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_steer_first(const float* x_T, const float* n0, float cn, float sigma0, int64_t N, int64_t R, float* X,
                                         float* Y, float* hist, float* sig_rows, void* stream) {
    const char* fn = "mdt_op_steer_first";
    MDT_TRY(hook_sizes(fn, N, R));
    if (N > 0) MDT_TRY(hook_nulls(fn, {{x_T, "x_T"}, {X, "X"}, {Y, "Y"}, {hist, "hist"}}));
    if (R > 0) MDT_TRY(hook_nulls(fn, {{sig_rows, "sig_rows"}}));
    MDT_TRY(hook_positive(fn, "sigma0", sigma0));
    LAUNCH(mdt_launch_lds<k_steer_first>(dim3(steer_grid(N + R)), dim3(STEER_THREADS), 0, (hipStream_t)stream, x_T, n0, cn, sigma0, N, R,
                                         X, Y, hist, sig_rows));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_steer_plan(const mdt_sampler_eval* ev, const float* small, const float* e, const float* D, const float* Y,
                                        const float* X, float* x_out, float* y_out, float* hist, const float* noise, const float* lo,
                                        const float* hi, float* rec, float* sig_rows, int64_t N, int64_t R, float sd, float scale,
                                        int32_t n_noise, int32_t A, void* stream) {
    const char* fn = "mdt_op_steer_plan";
    MDT_TRY(hook_nulls(fn, {{ev, "ev"}}));
    MDT_TRY(hook_sizes(fn, N, R));
    if (N > 0) MDT_TRY(hook_nulls(fn, {{small, "small"}, {e, "e"}, {D, "D"}, {Y, "Y"}, {X, "X"}, {x_out, "x_out"}, {hist, "hist"}}));
    if (R > 0) MDT_TRY(hook_nulls(fn, {{sig_rows, "sig_rows"}}));
    MDT_TRY(hook_bounds(fn, lo, hi, A, N));
    if (n_noise < 0) return fail(MDT_ERR_INVALID_ARG, "%s: n_noise is %d, must be >= 0", fn, n_noise);
    MDT_TRY(hook_positive(fn, "ev->sigma", ev->sigma));
    MDT_TRY(hook_positive(fn, "sd", sd));
    SteerPlanArgs a;
    a.ev = *ev;
    a.small = small; a.e = e; a.D = D;
    a.Y = Y; a.X = X;
    a.x_out = x_out; a.y_out = y_out;
    a.hist = hist;
    a.noise = noise;
    a.lo = lo; a.hi = hi;
    a.rec = rec;
    a.sig_rows = sig_rows;
    a.N = N; a.R = R;
    a.sd = sd; a.scale = scale;
    a.n_noise = n_noise; a.A = A;
    LAUNCH(mdt_launch_lds<k_steer_plan>(dim3(steer_grid(N + R)), dim3(STEER_THREADS), 0, (hipStream_t)stream, a));
    return MDT_OK;
}
