// mdt_score.hip -- the kernels of mdt_denoising_score (include/mdt_hip.h; the call itself stands beside the sampler entries in
// mdt_model.hip): action chunks scored by their likelihood-weighted denoising error,
//     score[r] = - sum_s w_s (1 / M) sum_m sum_e q[r, s, m, e]^2,   q = (x0 - D(x0 + sigma_s n[s, m]; sigma_s)) / sigma_s,
// from ONE decoder pass over B * S * K * M decoder samples.  Decoder sample j = ((b S + s) K + k) M + m is chunk k of observation
// b at level s with noise row m: consecutive samples share a context (S K M of them the observation's; where sigma is a context
// token K M of them the context of (b, s)), and the M draws of a chunk at one level lie side by side.
//   k_score_prep    the decoder's input: x = x0 + sigma_s n[s, m] per element, the rows' sigma, and the action embedding of
//                   x c_in(sigma_s), by the functions k_action_embed calls (mdt_edm.h)
//   k_score_repeat  where sigma is a context token: each observation's encoder inputs S times (context b S + s)
//   k_score_reduce  the score from the network's raw output F, in the residual form
//                       q = sigma / (sigma^2 + sd^2) x0 - c_skip n - sd / sqrt(sigma^2 + sd^2) F
//                   which never forms x0 - D, so nothing cancels at small sigma
//   k_score_select  the selection behind the scores: per observation the index gc_sampling.best_candidates gives, and that chunk
// The levels and the weights are host values and ride in the kernel arguments (mdt_score_levels): no copy, nothing to capture
// beside the launches.  No atomics anywhere: every output element has one writer and the sums have one fixed order.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <initializer_list>

#include "mdt_device.h"
#include "mdt_edm.h"
#include "mdt_hip_debug.h"
#include "mdt_internal.h"
#include "mdt_launch.h"

namespace {

constexpr int SCORE_THREADS = 256;  // four wave64
constexpr int SCORE_MAX_BLOCKS = 4096;

// (b, s, k, m) of decoder sample j
struct ScoreIndex { int64_t b; int s, k, m; };
__device__ __forceinline__ ScoreIndex score_index(int64_t j, int S, int K, int M) {
    ScoreIndex i;
    i.m = (int)(j % M); j /= M;
    i.k = (int)(j % K); j /= K;
    i.s = (int)(j % S);
    i.b = j / S;
    return i;
}

// One thread per four embedding columns of a decoder row, grid-stride over rows * D / 4.  The thread of a row's first columns
// also stores the row's A noised actions (the head's `x`), and the one of a sample's first row the sample's sigma (and the
// context's, where sigma is a context token: ctx_sig (B * S), written by the (k, m) = (0, 0) sample).  x0 and noise are only read.
__global__ __launch_bounds__(SCORE_THREADS) void k_score_prep(const float* __restrict__ x0, const float* __restrict__ noise,
                                                              mdt_score_levels lv, int S, int K, int M, int Ta, int A, int D, float sd,
                                                              const float* __restrict__ WaT, const float* __restrict__ ba,
                                                              int64_t rows, float* __restrict__ y, float* __restrict__ noised,
                                                              float* __restrict__ sig_rows, float* __restrict__ ctx_sig) {
    const int n4 = D >> 2;
    const int64_t total = rows * n4;
    for (int64_t idx = (int64_t)blockIdx.x * SCORE_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * SCORE_THREADS) {
        const int64_t row = idx / n4;
        const int n = (int)(idx - row * n4) * 4;
        const int64_t j = row / Ta;
        const int t = (int)(row - j * Ta);
        const ScoreIndex i = score_index(j, S, K, M);
        const float sg = lv.sigma[i.s];
        const float cin = edm_c_in(edm_den2_round_both(sg, sd));
        const float* xr = x0 + ((i.b * K + i.k) * Ta + t) * A;
        const float* nr = noise + (((int64_t)i.s * M + i.m) * Ta + t) * A;
        f32x4 acc = *(const f32x4*)(ba + n);
        for (int c = 0; c < A; ++c) {
            float xin;  // two roundings, as x0 + sigma * n is written everywhere else: __fmul_rn is a plain product to the compiler,
            {           // which contracts it into the sum unless told otherwise
#pragma clang fp contract(off)
                const float p = sg * nr[c];
                xin = xr[c] + p;
            }
            if (n == 0) noised[row * A + c] = xin;
            acc = action_embed_step(acc, xin, cin, WaT + (int64_t)c * D + n);
        }
        *(f32x4*)(y + row * D + n) = acc;
        if (n == 0 && t == 0) {
            sig_rows[j] = sg;
            if (ctx_sig != nullptr && i.k == 0 && i.m == 0) ctx_sig[i.b * S + i.s] = sg;
        }
    }
}

// dst row i of (B * S) <- src row i / S, for the three encoder inputs at once (widths w1, w2, wg floats; w2 == 0: no tokens2)
__global__ __launch_bounds__(SCORE_THREADS) void k_score_repeat(const float* __restrict__ tok, const float* __restrict__ tok2,
                                                                const float* __restrict__ goal, float* __restrict__ tok_o,
                                                                float* __restrict__ tok2_o, float* __restrict__ goal_o, int64_t BS,
                                                                int S, int w1, int w2, int wg) {
    const int w = w1 + w2 + wg;
    const int64_t total = BS * w;
    for (int64_t idx = (int64_t)blockIdx.x * SCORE_THREADS + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * SCORE_THREADS) {
        const int64_t i = idx / w, b = i / S;
        const int c = (int)(idx - i * w);
        if (c < w1) tok_o[i * w1 + c] = tok[b * w1 + c];
        else if (c < w1 + w2) tok2_o[i * w2 + (c - w1)] = tok2[b * w2 + (c - w1)];
        else goal_o[i * wg + (c - w1 - w2)] = goal[b * wg + (c - w1 - w2)];
    }
}

// One workgroup per chunk r = b K + k.  The S threads of the first waves form the level's constants once; wave w then takes the
// chunk's decoder samples i = s M + m with i % 4 == w in index order, its lanes striding over the E = Ta * A elements (70 is no
// multiple of 64: the tail lanes add nothing), a sample's sum entering the lane's total as w_s / M times it; then the xor
// butterfly over the 64 lanes and a two-level tree over the four waves in LDS.  Every order is fixed: a call repeats bit for bit.
__global__ __launch_bounds__(SCORE_THREADS) void k_score_reduce(const float* __restrict__ F, const float* __restrict__ x0,
                                                                const float* __restrict__ noise, mdt_score_levels lv, int S, int K,
                                                                int M, int E, float sd, float* __restrict__ score) {
    __shared__ float c_x[MDT_SCORE_MAX], c_n[MDT_SCORE_MAX], c_f[MDT_SCORE_MAX], c_w[MDT_SCORE_MAX], part[SCORE_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t r = blockIdx.x, b = r / K;
    const int k = (int)(r - b * K);
    if (tid < S) {
        const float sg = lv.sigma[tid], den2 = edm_den2_round_both(sg, sd);
        c_x[tid] = sg / den2;
        c_n[tid] = edm_c_skip(sd, den2);
        c_f[tid] = sd / sqrtf(den2);
        c_w[tid] = lv.weight[tid] / (float)M;
    }
    __syncthreads();
    const float* xr = x0 + r * E;
    float acc = 0.f;
    for (int i = wave; i < S * M; i += SCORE_THREADS / 64) {
        const int s = i / M, m = i - s * M;
        const float* Fr = F + (((b * S + s) * K + k) * M + m) * E;
        const float* nr = noise + (int64_t)i * E;
        const float cx = c_x[s], cn = c_n[s], cf = c_f[s];
        float sum = 0.f;
        for (int e = lane; e < E; e += 64) {
            const float q = cx * xr[e] - cn * nr[e] - cf * Fr[e];
            sum = fmaf(q, q, sum);
        }
        acc = fmaf(c_w[s], sum, acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (tid == 0) score[r] = -((part[0] + part[1]) + (part[2] + part[3]));
}

// A score as the selection orders it: best_candidates' torch.nan_to_num(scores, nan=-inf) -- NaN below everything, and, by that
// function's defaults, +Inf the largest finite float and -Inf the lowest (so +Inf ties with FLT_MAX, and -Inf beats NaN).
__device__ __forceinline__ float select_key(float v) {
    if (v != v) return -INFINITY;
    return fminf(fmaxf(v, -3.402823466e+38f), 3.402823466e+38f);
}
// whether (v, k) goes before (bv, bk): the larger key, then the lower index -- a total order, the k being distinct
__device__ __forceinline__ bool select_beats(float v, int k, float bv, int bk) { return v > bv || (v == bv && k < bk); }

// One workgroup per observation b.  Lane t scans the keys of k = t, t + 256, .. and keeps its first largest; a lane without a k holds
// (-Inf, INT_MAX), which loses every tie, so K all-NaN scores select k = 0.  Then the xor butterfly over the 64 lanes carrying
// (key, k) -- the order is total, so every lane ends with the wave's winner -- and the four waves' winners from LDS in wave order,
// by every thread alike.  The workgroup then copies the winner's E elements; thread 0 stores the index.  scores and chunks are only read.
__global__ __launch_bounds__(SCORE_THREADS) void k_score_select(const float* __restrict__ score, const float* __restrict__ chunks, int K,
                                                                 int E, float* __restrict__ best, int32_t* __restrict__ index) {
    __shared__ float pv[SCORE_THREADS / 64];
    __shared__ int pk[SCORE_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t b = blockIdx.x;
    const float* sr = score + b * K;
    float bv = -INFINITY;
    int bk = 0x7fffffff;
    for (int k = tid; k < K; k += SCORE_THREADS) {
        const float v = select_key(sr[k]);
        if (select_beats(v, k, bv, bk)) { bv = v; bk = k; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int ok = __shfl_xor(bk, off, 64);
        if (select_beats(ov, ok, bv, bk)) { bv = ov; bk = ok; }
    }
    if (lane == 0) { pv[wave] = bv; pk[wave] = bk; }
    __syncthreads();
    bv = pv[0]; bk = pk[0];
#pragma unroll
    for (int w = 1; w < SCORE_THREADS / 64; ++w)
        if (select_beats(pv[w], pk[w], bv, bk)) { bv = pv[w]; bk = pk[w]; }
    const float* src = chunks + (b * K + bk) * E;
    float* dst = best + b * E;
    for (int e = tid; e < E; e += SCORE_THREADS) dst[e] = src[e];
    if (tid == 0) index[b] = bk;
}

unsigned score_grid(int64_t n) {
    const int64_t g = (n + SCORE_THREADS - 1) / SCORE_THREADS;
    return (unsigned)(g < 1 ? 1 : (g > SCORE_MAX_BLOCKS ? SCORE_MAX_BLOCKS : g));
}

bool score_shape_ok(int64_t B, int S, int K, int M) {
    return B >= 1 && K >= 1 && S >= 1 && S <= MDT_SCORE_MAX && M >= 1 && M <= MDT_SCORE_MAX;
}

}  // namespace

hipError_t mdt_launch_score_prep(const float* x0, const float* noise, const mdt_score_levels& lv, int64_t B, int S, int K, int M, int Ta,
                                 int A, int D, float sd, const float* Wa, const float* ba, float* y, float* noised, float* sig_rows,
                                 float* ctx_sig, hipStream_t s) {
    if (!score_shape_ok(B, S, K, M) || Ta < 1 || A < 1 || D < 4 || (D & 3)) return hipErrorInvalidValue;
    const int64_t rows = B * S * K * M * Ta;
    return mdt_launch_lds<k_score_prep>(dim3(score_grid(rows * (D >> 2))), dim3(SCORE_THREADS), 0, s, x0, noise, lv, S, K, M, Ta, A, D, sd,
                                        Wa, ba, rows, y, noised, sig_rows, ctx_sig);
}

hipError_t mdt_launch_score_repeat(const float* tok, const float* tok2, const float* goal, float* tok_o, float* tok2_o, float* goal_o,
                                   int64_t B, int S, int w1, int w2, int wg, hipStream_t s) {
    if (B < 1 || S < 1 || w1 < 1 || w2 < 0 || wg < 1 || (w2 > 0 && (!tok2 || !tok2_o))) return hipErrorInvalidValue;
    return mdt_launch_lds<k_score_repeat>(dim3(score_grid(B * S * (w1 + w2 + wg))), dim3(SCORE_THREADS), 0, s, tok, tok2, goal, tok_o,
                                          tok2_o, goal_o, B * S, S, w1, w2, wg);
}

hipError_t mdt_launch_score_reduce(const float* F, const float* x0, const float* noise, const mdt_score_levels& lv, int64_t B, int S,
                                   int K, int M, int E, float sd, float* score, hipStream_t s) {
    if (!score_shape_ok(B, S, K, M) || E < 1 || B * K > 0x7fffffff) return hipErrorInvalidValue;
    return mdt_launch_lds<k_score_reduce>(dim3((unsigned)(B * K)), dim3(SCORE_THREADS), 0, s, F, x0, noise, lv, S, K, M, E, sd, score);
}

hipError_t mdt_launch_score_select(const float* score, const float* chunks, int64_t B, int K, int E, float* best, int32_t* index,
                                   hipStream_t s) {
    if (B < 1 || B > 0x7fffffff || K < 1 || E < 1) return hipErrorInvalidValue;
    return mdt_launch_lds<k_score_select>(dim3((unsigned)B), dim3(SCORE_THREADS), 0, s, score, chunks, K, E, best, index);
}

// ------------------------------------------------------------------------------------------------
// test hooks (mdt_hip_debug.h): the kernels above on the caller's buffers, each through the launch mdt_denoising_score makes
// or mdt_sample*_select makes (mdt_launch_score_*).  What the call guarantees by construction is checked here, before anything is launched.
// ------------------------------------------------------------------------------------------------
namespace {

struct Named {
    const void* p;
    const char* name;
};

mdt_status hook_nulls(const char* fn, std::initializer_list<Named> ps) {
    for (const Named& n : ps)
        if (!n.p) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: null %s", fn, n.name);
    return MDT_OK;
}

mdt_status hook_at_least_1(const char* fn, const char* name, int64_t v) {
    if (v < 1) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: %s is %lld, must be >= 1", fn, name, (long long)v);
    return MDT_OK;
}

mdt_status hook_up_to_max(const char* fn, const char* name, int32_t v) {
    if (v < 1 || v > MDT_SCORE_MAX)
        return mdt_fail(MDT_ERR_INVALID_ARG, "%s: %s is %d, must be in [1, %d]", fn, name, (int)v, MDT_SCORE_MAX);
    return MDT_OK;
}

mdt_status hook_sd(const char* fn, float sd) {
    if (!std::isfinite(sd) || !(sd > 0.f)) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: sd is %g, must be finite and > 0", fn, (double)sd);
    return MDT_OK;
}

// the S levels (and weights, or null: zeros) into the kernel argument; S is in [1, MDT_SCORE_MAX] here
mdt_status hook_levels(const char* fn, const float* sigmas, const float* weights, int32_t S, mdt_score_levels* lv) {
    memset(lv, 0, sizeof *lv);
    for (int i = 0; i < S; ++i) {
        if (!std::isfinite(sigmas[i]) || !(sigmas[i] > 0.f))
            return mdt_fail(MDT_ERR_INVALID_ARG, "%s: sigmas[%d] is %g, must be finite and > 0", fn, i, (double)sigmas[i]);
        lv->sigma[i] = sigmas[i];
    }
    for (int i = 0; weights && i < S; ++i) {
        if (!std::isfinite(weights[i]) || !(weights[i] >= 0.f))
            return mdt_fail(MDT_ERR_INVALID_ARG, "%s: weights[%d] is %g, must be finite and >= 0", fn, i, (double)weights[i]);
        lv->weight[i] = weights[i];
    }
    return MDT_OK;
}

}  // namespace

extern "C" mdt_status mdt_op_score_prep(const float* x0, const float* noise, const float* sigmas, int32_t S, int32_t K, int32_t M,
                                        int64_t B, int32_t Ta, int32_t A, int32_t D, float sd, const float* WaT, const float* ba,
                                        float* y, float* noised, float* sig_rows, float* ctx_sig, void* stream) {
    const char* fn = "mdt_op_score_prep";
    MDT_TRY(hook_nulls(fn, {{x0, "x0"}, {noise, "noise"}, {sigmas, "sigmas"}, {WaT, "WaT"}, {ba, "ba"}, {y, "y"}, {noised, "noised"},
                            {sig_rows, "sig_rows"}}));
    MDT_TRY(hook_at_least_1(fn, "B", B));
    MDT_TRY(hook_at_least_1(fn, "K", K));
    MDT_TRY(hook_up_to_max(fn, "S", S));
    MDT_TRY(hook_up_to_max(fn, "M", M));
    MDT_TRY(hook_at_least_1(fn, "Ta", Ta));
    MDT_TRY(hook_at_least_1(fn, "A", A));
    if (D < 4 || (D & 3)) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: D is %d, must be a multiple of 4 and >= 4", fn, (int)D);
    MDT_TRY(hook_sd(fn, sd));
    mdt_score_levels lv;
    MDT_TRY(hook_levels(fn, sigmas, nullptr, S, &lv));
    LAUNCH(mdt_launch_score_prep(x0, noise, lv, B, S, K, M, Ta, A, D, sd, WaT, ba, y, noised, sig_rows, ctx_sig, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_score_repeat(const float* tok, const float* tok2, const float* goal, int64_t B, int32_t S, int32_t w1,
                                          int32_t w2, int32_t wg, float* tok_o, float* tok2_o, float* goal_o, void* stream) {
    const char* fn = "mdt_op_score_repeat";
    MDT_TRY(hook_nulls(fn, {{tok, "tok"}, {goal, "goal"}, {tok_o, "tok_o"}, {goal_o, "goal_o"}}));
    MDT_TRY(hook_at_least_1(fn, "B", B));
    MDT_TRY(hook_up_to_max(fn, "S", S));
    MDT_TRY(hook_at_least_1(fn, "w1", w1));
    if (w2 < 0) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: w2 is %d, must be >= 0", fn, (int)w2);
    MDT_TRY(hook_at_least_1(fn, "wg", wg));
    if (w2 > 0) MDT_TRY(hook_nulls(fn, {{tok2, "tok2"}, {tok2_o, "tok2_o"}}));
    LAUNCH(mdt_launch_score_repeat(tok, tok2, goal, tok_o, tok2_o, goal_o, B, S, w1, w2, wg, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_score_reduce(const float* F, const float* x0, const float* noise, const float* sigmas,
                                          const float* weights, int64_t B, int32_t S, int32_t K, int32_t M, int32_t E, float sd,
                                          float* score, void* stream) {
    const char* fn = "mdt_op_score_reduce";
    MDT_TRY(hook_nulls(fn, {{F, "F"}, {x0, "x0"}, {noise, "noise"}, {sigmas, "sigmas"}, {weights, "weights"}, {score, "score"}}));
    MDT_TRY(hook_at_least_1(fn, "B", B));
    MDT_TRY(hook_up_to_max(fn, "S", S));
    MDT_TRY(hook_at_least_1(fn, "K", K));
    MDT_TRY(hook_up_to_max(fn, "M", M));
    MDT_TRY(hook_at_least_1(fn, "E", E));
    if (B > (int64_t)0x7fffffff / K)
        return mdt_fail(MDT_ERR_INVALID_ARG, "%s: B * K is %lld * %d, more than 2147483647 chunks (one workgroup each)", fn, (long long)B,
                        (int)K);
    MDT_TRY(hook_sd(fn, sd));
    mdt_score_levels lv;
    MDT_TRY(hook_levels(fn, sigmas, weights, S, &lv));
    LAUNCH(mdt_launch_score_reduce(F, x0, noise, lv, B, S, K, M, E, sd, score, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_score_select(const float* scores, const float* chunks, int64_t B, int32_t K, int32_t E, float* best,
                                          int32_t* index, void* stream) {
    const char* fn = "mdt_op_score_select";
    MDT_TRY(hook_nulls(fn, {{scores, "scores"}, {chunks, "chunks"}, {best, "best"}, {index, "index"}}));
    MDT_TRY(hook_at_least_1(fn, "B", B));
    MDT_TRY(hook_at_least_1(fn, "K", K));
    MDT_TRY(hook_at_least_1(fn, "E", E));
    if (B > (int64_t)0x7fffffff)
        return mdt_fail(MDT_ERR_INVALID_ARG, "%s: B is %lld, more than 2147483647 observations (one workgroup each)", fn, (long long)B);
    LAUNCH(mdt_launch_score_select(scores, chunks, B, K, E, best, index, (hipStream_t)stream));
    return MDT_OK;
}
