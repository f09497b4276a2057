// mdt_loglik.hip -- mdt_log_likelihood (include/mdt_hip_train.h): gc_sampling.log_likelihood + _dopri5 as one blocking call.
//
// Reference: gc_sampling.py:468-490 (the probability-flow ODE with Hutchinson's divergence estimate, integrated by
// torchdiffeq's dopri5, whose role _dopri5 plays in the Python facade).  The denoiser and its vector-Jacobian product are the
// training path's (mdt_loglik.h: the encoder and the cross K|V once, a tape-keeping decoder forward and P input-gradient-only
// backwards per evaluation); this file holds the integrator: the Dormand-Prince stage sums, the right-hand side, the scaled
// error and the final reduction as wave64 kernels, and the host loop that reads one set of partial sums back per attempted step.
// No kernel here uses atomics and every reduction runs in a fixed order (lanes stride, xor shuffles, an LDS tree, then the host's
// double sum in index order), so the step sequence -- and with it every bit of the result -- repeats from call to call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "mdt_launch.h"
#include "mdt_loglik.h"

#define fail mdt_fail

namespace {

// Dormand-Prince 5(4): node positions, stage weights (row i feeds stage i + 1; the last row is the 5th-order solution:
// first-same-as-last) and the difference to the embedded 4th-order weights (gc_sampling.py: _DP_C, _DP_A, _DP_E)
const double DP_C[7] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0, 1.0};
const double DP_A[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84},
};
const double DP_E[7] = {35.0 / 384 - 5179.0 / 57600, 0.0, 500.0 / 1113 - 7571.0 / 16695, 125.0 / 192 - 393.0 / 640,
                        -2187.0 / 6784 + 92097.0 / 339200, 11.0 / 84 - 187.0 / 2100, -1.0 / 40};

constexpr int LL_PARTS = 256;  // most workgroups of a norm launch (256 elements each per trip): partial sums read back per step
constexpr int LL_TERMS = 7;

// sum_j c[j] * k[j] over the stage derivatives of one state part, by value: n terms (zero weights left out, as the loop does)
struct Terms {
    const float* k[LL_TERMS];
    float c[LL_TERMS];
    int n;
};

__device__ __forceinline__ float terms_at(const Terms& t, int64_t i) {
    float acc = 0.f;
    for (int j = 0; j < t.n; ++j) acc += t.c[j] * t.k[j][i];
    return acc;
}

// A stage's input: x_out = x + h sum_j a_j kx_j over the N = R * per action elements; the R entries behind them fill the per-row
// sigma the decoder reads and, where d_out is given (the step's last stage: y_new), d_out = d + h sum_j a_j kd_j.
__global__ __launch_bounds__(256) void k_ll_stage(const float* __restrict__ x, const float* __restrict__ d, Terms kx, Terms kd,
                                                  float h, float sigma, int64_t N, int64_t R, float* __restrict__ x_out,
                                                  float* __restrict__ d_out, float* __restrict__ sig_rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        x_out[i] = x[i] + h * terms_at(kx, i);
    } else if (i < N + R) {
        const int64_t r = i - N;
        sig_rows[r] = sigma;
        if (d_out) d_out[r] = d[r] + h * terms_at(kd, r);
    }
}

__device__ __forceinline__ float wave_sum(float a) {
    for (int w = 32; w > 0; w >>= 1) a += __shfl_xor(a, w, 64);
    return a;  // every lane holds the same sum: the butterfly adds the same pairs in the same order on each
}

// The right-hand side at (x, sigma), one wave per row: kx = (x - D) / sigma per element, kd = mean_p sum_e v_p (v_p - J^T v_p)
// / sigma per row.  per = Ta * A is no multiple of 64: lanes stride over the row and the tail lanes add zeros.
__global__ __launch_bounds__(256) void k_ll_rhs(const float* __restrict__ x, const float* __restrict__ den,
                                                const float* __restrict__ v, const float* __restrict__ jtv, int P, float sigma,
                                                int per, int64_t R, float* __restrict__ kx, float* __restrict__ kd) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int64_t base = row * per, N = R * per;
    for (int e = lane; e < per; e += 64) kx[base + e] = (x[base + e] - den[base + e]) / sigma;
    float total = 0.f;
    for (int p = 0; p < P; ++p) {
        float a = 0.f;
        for (int e = lane; e < per; e += 64) {
            const float vv = v[p * N + base + e];
            a += vv * (vv - jtv[p * N + base + e]);
        }
        total += wave_sum(a);
    }
    if (lane == 0) kd[row] = total / (float)P / sigma;
}

// element i of the whole state (x part, then the delta part)
__device__ __forceinline__ float both(const float* __restrict__ a, const float* __restrict__ b, int64_t i, int64_t N) {
    return i < N ? a[i] : b[i - N];
}

// a workgroup's sum of `acc` in a fixed order -> part[blockIdx.x]
__device__ __forceinline__ void block_part(float acc, float* red, float* __restrict__ part) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
    __syncthreads();
}

// The scaled error of an attempted step over all N + R entries of both state parts: err = h sum_j e_j k_j,
// scale = atol + rtol max(|y|, |y_new|); per-workgroup partial sums of (err / scale)^2 (grid-stride, then an LDS tree).
__global__ __launch_bounds__(256) void k_ll_error(const float* __restrict__ x, const float* __restrict__ xn,
                                                  const float* __restrict__ d, const float* __restrict__ dn, Terms ex, Terms ed,
                                                  float h, float rtol, float atol, int64_t N, int64_t R, float* __restrict__ part) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N + R; i += (int64_t)gridDim.x * 256) {
        const float err = h * (i < N ? terms_at(ex, i) : terms_at(ed, i - N));
        const float sc = atol + rtol * fmaxf(fabsf(both(x, d, i, N)), fabsf(both(xn, dn, i, N)));
        const float q = err / sc;
        acc += q * q;
    }
    block_part(acc, red, part);
}

// The starting step's norms with scale = atol + rtol |y|: part[0 .. parts) of (y / scale)^2 and part[LL_PARTS ..) of
// ((ka - kb) / scale)^2 -- kb == nullptr: of (ka / scale)^2.
__global__ __launch_bounds__(256) void k_ll_start(const float* __restrict__ x, const float* __restrict__ d,
                                                  const float* __restrict__ kax, const float* __restrict__ kad,
                                                  const float* __restrict__ kbx, const float* __restrict__ kbd, float rtol,
                                                  float atol, int64_t N, int64_t R, float* __restrict__ part) {
    __shared__ float red[256];
    float a0 = 0.f, a1 = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N + R; i += (int64_t)gridDim.x * 256) {
        const float y = both(x, d, i, N);
        const float sc = atol + rtol * fabsf(y);
        float k = both(kax, kad, i, N);
        if (kbx) k -= both(kbx, kbd, i, N);
        const float q0 = y / sc, q1 = k / sc;
        a0 += q0 * q0;
        a1 += q1 * q1;
    }
    block_part(a0, red, part);
    block_part(a1, red, part + LL_PARTS);
}

// ll = sum_e log N(latent_e; 0, sigma_max^2) + delta, one wave per row (torch.distributions.Normal.log_prob per element, then
// the row's sum), and the optional copies of the final state.
__global__ __launch_bounds__(256) void k_ll_finish(const float* __restrict__ x, const float* __restrict__ d, float sigma_max,
                                                   int per, int64_t R, float* __restrict__ ll, float* __restrict__ latent,
                                                   float* __restrict__ delta) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const float var2 = 2.f * sigma_max * sigma_max, lsc = logf(sigma_max), half_l2pi = 0.918938533204672741780f;
    float a = 0.f;
    for (int e = lane; e < per; e += 64) {
        const float xv = x[row * per + e];
        a += -(xv * xv) / var2 - lsc - half_l2pi;
        if (latent) latent[row * per + e] = xv;
    }
    a = wave_sum(a);
    if (lane == 0) {
        ll[row] = a + d[row];
        if (delta) delta[row] = d[row];
    }
}

// each observation's K|V rows K times: dst row b*K + k = src row b, 16 bytes per thread
__global__ __launch_bounds__(256) void k_ll_repeat_rows(const float4* __restrict__ src, float4* __restrict__ dst, int64_t rows,
                                                        int K, int64_t w4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * w4) return;
    const int64_t r = i / w4;
    dst[i] = src[(r / K) * w4 + (i - r * w4)];
}

int norm_parts(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, LL_PARTS); }

// the pinned host block the partial sums come back into
struct LLHost {
    float part[2 * LL_PARTS];
};

// the integrator's buffers over one device block
struct LLBufs {
    float *x, *xn, *xs, *d, *dn, *kx[7], *kd[7], *den, *jtv, *sig, *part;
};

void carve(Bump& b, int64_t rows, int64_t probes, int per, LLBufs* o) {
    LLBufs t;
    const int64_t N = rows * per;
    t.x = b.take(N); t.xn = b.take(N); t.xs = b.take(N);
    t.d = b.take(rows); t.dn = b.take(rows);
    for (int j = 0; j < 7; ++j) { t.kx[j] = b.take(N); t.kd[j] = b.take(rows); }
    t.den = b.take(N); t.jtv = b.take(probes * N); t.sig = b.take(rows); t.part = b.take(2 * LL_PARTS);
    if (o) *o = t;
}

Terms terms(float* const* k, const double* c, int n) {
    Terms t;
    t.n = 0;
    for (int j = 0; j < n; ++j)
        if (c[j] != 0.0) { t.k[t.n] = k[j]; t.c[t.n] = (float)c[j]; ++t.n; }
    for (int j = t.n; j < LL_TERMS; ++j) { t.k[j] = nullptr; t.c[j] = 0.f; }
    return t;
}

struct Call {
    mdt_model* m;
    mdt_ll_run run;
    hipStream_t s;
    const float *tokens, *tokens2, *goal, *v;
    int modality, P, per;
    int64_t R, N;
    LLBufs b;
    LLHost* host;
};

// f(sigma, x_in) -> (kx, kd); c.b.sig holds sigma on every row (k_ll_stage filled it)
mdt_status evaluate(Call& c, const float* x_in, double sigma, float* kx, float* kd) {
    mdt_model* m = c.m;
    if (m->cond == COND_TOKEN)  // sigma is a context token: the context is this evaluation's, still on the B observations
        MDT_TRY(mdt_ll_context(m, c.run, c.tokens, c.tokens2, c.goal, c.modality, c.b.sig, c.s));
    MDT_TRY(mdt_ll_forward(m, c.run, x_in, c.b.sig, c.s));
    for (int p = 0; p < c.P; ++p)
        MDT_TRY(mdt_ll_vjp(m, c.run, c.v + p * c.N, p == 0 ? c.b.den : nullptr, c.b.jtv + p * c.N, c.s));
    LAUNCH(mdt_launch_lds<k_ll_rhs>(dim3((unsigned)((c.R + 3) / 4)), dim3(256), 0, c.s, x_in, (const float*)c.b.den, c.v,
                                    (const float*)c.b.jtv, c.P, (float)sigma, c.per, c.R, kx, kd));
    return MDT_OK;
}

// x_out (and d_out) = y + h sum_j a[j] k_j over the first n stage derivatives, and the rows' sigma
mdt_status stage(Call& c, const double* a, int n, double h, double sigma, float* x_out, float* d_out) {
    LAUNCH(mdt_launch_lds<k_ll_stage>(dim3((unsigned)((c.N + c.R + 255) / 256)), dim3(256), 0, c.s, (const float*)c.b.x,
                                      (const float*)c.b.d, terms(c.b.kx, a, n), terms(c.b.kd, a, n), (float)h, (float)sigma, c.N,
                                      c.R, x_out, d_out, c.b.sig));
    return MDT_OK;
}

// `sets` x parts floats of c.b.part -> the host, one synchronisation; out[k] = sqrt(sum / n) in double, index order
mdt_status read_norms(Call& c, int sets, double* out) {
    const int parts = norm_parts(c.N + c.R);
    HIP_TRY(hipMemcpyAsync(c.host->part, c.b.part, (size_t)((sets - 1) * LL_PARTS + parts) * sizeof(float), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    for (int k = 0; k < sets; ++k) {
        double sum = 0.0;
        for (int i = 0; i < parts; ++i) sum += c.host->part[k * LL_PARTS + i];
        out[k] = sqrt(sum / (double)(c.N + c.R));
    }
    return MDT_OK;
}

mdt_status integrate(Call& c, const float* x0, double t0, double t1, const mdt_loglik_params& p, mdt_loglik_info* inf) {
    LLBufs& b = c.b;
    const unsigned grid = (unsigned)norm_parts(c.N + c.R);
    const float rtol = (float)p.rtol, atol = (float)p.atol;
    HIP_TRY(hipMemcpyAsync(b.x, x0, (size_t)c.N * sizeof(float), hipMemcpyDeviceToDevice, c.s));
    HIP_TRY(hipMemsetAsync(b.d, 0, (size_t)c.R * sizeof(float), c.s));
    if (c.m->cond != COND_TOKEN) MDT_TRY(mdt_ll_context(c.m, c.run, c.tokens, c.tokens2, c.goal, c.modality, nullptr, c.s));
    // ---- Hairer's starting step: k1 = f(t0, y0), d0 = |y0|, d1 = |k1|; a probe evaluation one guessed step away gives d2
    double t = t0, nrm[2];
    MDT_TRY(stage(c, nullptr, 0, 0.0, t, b.xs, nullptr));  // (no terms: xs = x, and the rows' sigma)
    MDT_TRY(evaluate(c, b.xs, t, b.kx[0], b.kd[0]));
    LAUNCH(mdt_launch_lds<k_ll_start>(dim3(grid), dim3(256), 0, c.s, (const float*)b.x, (const float*)b.d, (const float*)b.kx[0],
                                      (const float*)b.kd[0], (const float*)nullptr, (const float*)nullptr, rtol, atol, c.N, c.R, b.part));
    MDT_TRY(read_norms(c, 2, nrm));
    const double d1 = nrm[1];
    double h = mdt_dopri5_h0(nrm[0], d1);
    if (std::isnan(h)) return fail(MDT_ERR_NUMERIC, "mdt_log_likelihood: the starting step is NaN (|y0| = %g, |f0| = %g)", nrm[0], d1);
    const double one = 1.0;
    MDT_TRY(stage(c, &one, 1, h, t + h, b.xs, nullptr));  // y0 + h k1
    MDT_TRY(evaluate(c, b.xs, t + h, b.kx[1], b.kd[1]));
    LAUNCH(mdt_launch_lds<k_ll_start>(dim3(grid), dim3(256), 0, c.s, (const float*)b.x, (const float*)b.d, (const float*)b.kx[1],
                                      (const float*)b.kd[1], (const float*)b.kx[0], (const float*)b.kd[0], rtol, atol, c.N, c.R, b.part));
    MDT_TRY(read_norms(c, 2, nrm));
    h = mdt_dopri5_h1(h, d1, nrm[1]);
    inf->fevals = 2;
    if (std::isnan(h)) return fail(MDT_ERR_NUMERIC, "mdt_log_likelihood: the starting step is NaN (|f0| = %g, |f1 - f0| = %g)", d1, nrm[1]);
    // ---- the steps
    for (int n = 0; n < p.max_steps; ++n) {
        if (t1 - t <= 0) return MDT_OK;
        h = std::min(h, fabs(t1 - t));
        if (t + h == t)
            return fail(MDT_ERR_NUMERIC, "mdt_log_likelihood: the step no longer moves (sigma = %g, h = %g) after %d steps", t, h, inf->steps);
        for (int i = 1; i < 7; ++i) {
            const double ti = t + DP_C[i] * h;
            float* xi = i == 6 ? b.xn : b.xs;
            MDT_TRY(stage(c, DP_A[i], i, h, ti, xi, i == 6 ? b.dn : nullptr));
            MDT_TRY(evaluate(c, xi, ti, b.kx[i], b.kd[i]));
        }
        LAUNCH(mdt_launch_lds<k_ll_error>(dim3(grid), dim3(256), 0, c.s, (const float*)b.x, (const float*)b.xn, (const float*)b.d,
                                          (const float*)b.dn, terms(b.kx, DP_E, 7), terms(b.kd, DP_E, 7), (float)h, rtol, atol, c.N,
                                          c.R, b.part));
        MDT_TRY(read_norms(c, 1, nrm));
        const double ratio = nrm[0];
        inf->steps += 1;
        inf->fevals += 6;
        if (std::isnan(ratio))
            return fail(MDT_ERR_NUMERIC, "mdt_log_likelihood: the scaled error is NaN (sigma = %g, h = %g) after %d steps", t, h, inf->steps);
        int32_t accept = 0;
        const double h_next = mdt_dopri5_next(h, ratio, &accept);
        if (accept) {  // y <- y_new, k1 <- k7: pointers change hands
            t = h >= fabs(t1 - t) ? t1 : t + h;
            std::swap(b.x, b.xn);
            std::swap(b.d, b.dn);
            std::swap(b.kx[0], b.kx[6]);
            std::swap(b.kd[0], b.kd[6]);
            inf->n_accept += 1;
        } else {
            inf->n_reject += 1;
        }
        h = h_next;
        if (std::isnan(h)) return fail(MDT_ERR_NUMERIC, "mdt_log_likelihood: the step size is NaN after %d steps", inf->steps);
    }
    return fail(MDT_ERR_NUMERIC, "mdt_log_likelihood: step budget exhausted before reaching sigma_max (max_steps = %d, sigma = %g)",
                p.max_steps, t);
}

}  // namespace

hipError_t mdt_launch_ll_repeat_rows(const float* src, float* dst, int64_t B, int K, int64_t w, hipStream_t s) {
    const int64_t n4 = B * K * (w / 4);
    return mdt_launch_lds<k_ll_repeat_rows>(dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const float4*)src, (float4*)dst,
                                            B * K, K, w / 4);
}

extern "C" double mdt_dopri5_h0(double d0, double d1) { return (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1; }

extern "C" double mdt_dopri5_h1(double h0, double d1, double d2) {
    const double mx = std::max(d1, d2 / h0);
    const double h1 = mx <= 1e-15 ? std::max(1e-6, 1e-3 * h0) : pow(0.01 / mx, 0.2);
    return std::min(100.0 * h0, h1);
}

extern "C" double mdt_dopri5_next(double h, double ratio, int32_t* accept) {
    if (accept) *accept = ratio <= 1.0 ? 1 : 0;
    if (ratio == 0.0) return h * 10.0;
    return h * std::min(10.0, std::max(0.2, 0.9 * pow(ratio, -0.2)));
}

extern "C" mdt_status mdt_log_likelihood(mdt_model* m, const float* tokens, const float* tokens2, const float* goal,
                                         int32_t modality, const float* x, const float* v, float sigma_min, float sigma_max,
                                         int64_t batch, int32_t candidates, const mdt_loglik_params* params, float* ll,
                                         float* latent, float* delta, mdt_loglik_info* info, void* stream) {
    const char* fn = "mdt_log_likelihood";
    MDT_TRY(mdt_ll_check_head(fn, m, tokens, goal, {{x, "x"}, {v, "v"}, {ll, "ll"}}, batch, candidates));
    mdt_loglik_params p = {(int32_t)sizeof(mdt_loglik_params), 1, 1e-4, 1e-4, 10000, 0};
    if (params) {
        if (params->size != (int32_t)sizeof(mdt_loglik_params))
            return fail(MDT_ERR_INVALID_ARG, "%s: params.size is %d, sizeof(mdt_loglik_params) is %d", fn, params->size,
                        (int)sizeof(mdt_loglik_params));
        p = *params;
    }
    if (p.probes < 1) return fail(MDT_ERR_INVALID_ARG, "%s: params.probes is %d, must be >= 1", fn, p.probes);
    if (!std::isfinite(sigma_min) || !(sigma_min > 0.f))
        return fail(MDT_ERR_INVALID_ARG, "%s: sigma_min is %g, must be finite and > 0", fn, sigma_min);
    if (!(sigma_max > sigma_min) || !std::isfinite(sigma_max))
        return fail(MDT_ERR_INVALID_ARG, "%s: sigma_max is %g, must be finite and > sigma_min (%g)", fn, sigma_max, sigma_min);
    if (!std::isfinite(p.rtol) || !(p.rtol > 0)) return fail(MDT_ERR_INVALID_ARG, "%s: params.rtol is %g, must be finite and > 0", fn, p.rtol);
    if (!std::isfinite(p.atol) || !(p.atol > 0)) return fail(MDT_ERR_INVALID_ARG, "%s: params.atol is %g, must be finite and > 0", fn, p.atol);
    if (p.max_steps < 1) return fail(MDT_ERR_INVALID_ARG, "%s: params.max_steps is %d, must be >= 1", fn, p.max_steps);
    hipStream_t s = (hipStream_t)stream;
    MDT_TRY(mdt_ll_check_tail(m, fn, tokens2, batch, candidates, s, "the call synchronises every step and"));

    Call c;
    const int64_t R = batch * candidates;
    c.m = m; c.s = s; c.tokens = tokens; c.tokens2 = tokens2; c.goal = goal; c.v = v; c.modality = modality;
    c.P = p.probes; c.per = m->Ta * m->A; c.R = R; c.N = R * c.per;
    MDT_TRY(mdt_grow_carve(m->ll_ws, m->ll_rows, m->ll_probes, R, (int64_t)p.probes,
                           [&](Bump& b, int64_t rows, int64_t probes) { carve(b, rows, probes, c.per, b.base ? &c.b : nullptr); }));
    if (!m->ll_host) HIP_TRY(hipHostMalloc(&m->ll_host, sizeof(LLHost), hipHostMallocDefault));
    c.host = (LLHost*)m->ll_host;
    mdt_loglik_info inf = {0, 0, 0, 0};
    const mdt_status st = mdt_ll_scoped(m, batch, candidates, s, &c.run, [&]() -> mdt_status {
        MDT_TRY(integrate(c, x, (double)sigma_min, (double)sigma_max, p, &inf));
        hipError_t e = mdt_launch_lds<k_ll_finish>(dim3((unsigned)((R + 3) / 4)), dim3(256), 0, s, (const float*)c.b.x,
                                                   (const float*)c.b.d, sigma_max, c.per, R, ll, latent, delta);
        return e == hipSuccess ? MDT_OK : fail(MDT_ERR_HIP, "%s: finish launch failed: %s", fn, hipGetErrorString(e));
    });
    if (st == MDT_OK && info) *info = inf;
    return st;
}
