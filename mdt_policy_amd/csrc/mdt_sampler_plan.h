// The sampler plans behind mdt_sample (include/mdt_hip.h): for one sampler kind, parameter set and schedule, the list of
// denoiser evaluations and the per-evaluation coefficients the action-head kernel applies (MDT_HEAD_PLAN).  One routine for
// the host (mdt_sampler_plan) and the device (k_sampler_plan, which reads a device schedule at replay time).
//
// Every scalar is the Python loop's expression (gc_sampling.py) in fp32, as the reference's 0-dim tensors compute it:
// get_ancestral_step, t = -ln(sigma), expm1, the log-space midpoints, sigma_hat with s_churn.  The LMS coefficients are the
// exact integrals of the Lagrange basis (3-point Gauss-Legendre in double: exact for the cubic and lower bases of orders
// 1..4; the Python loop's adaptive quadrature agrees up to its rounding).
//
// Schedule assumption: sig[0..n-1] > 0 and sig[n] == 0.  The loops' branches on sig[i + 1] == 0 are then taken at the last
// step and only there, so the evaluation count depends on the kind and n alone.  The ancestral branches on sigma_down == 0
// (fp32 can round sigma_down to 0 on a steep step) and dpmpp_sde's on sigma_up != 0 are followed as the loops follow them:
// a second evaluation the loop skips still runs, with coefficients that leave the state as it is, and the noise rows are
// numbered in the loop's draw order -- n_noise is the loop's draw count, at most mdt_plan_shape's.
//
// dpm_fast takes the two levels {sigma_max, sigma_min} and n evaluations instead (_dpm_fast_run): its steps are the uniform
// t grid of torch.linspace, every stage's eps is d = (Y - D) / sigma of its evaluation (each evaluation's input is the stage
// point), and the combines are linear in X, d and the pushed eps_0 / eps_1.
#pragma once

#include <math.h>
#include <string.h>

#include "mdt_hip.h"

#ifndef MDT_HD
#define MDT_HD __host__ __device__
#endif

// Python's defaults of the sampler functions (gc_sampling.py)
MDT_HD inline mdt_sampler_params mdt_sampler_defaults() {
    mdt_sampler_params p;
    p.eta = 1.f; p.s_churn = 0.f; p.s_tmin = 0.f; p.s_tmax = INFINITY; p.s_noise = 1.f; p.r = 0.5f; p.order = 4;
    return p;
}

enum { MDT_PLAN_OK = 0, MDT_PLAN_BAD_KIND = 1, MDT_PLAN_BAD_STEPS = 2, MDT_PLAN_BAD_ORDER = 3, MDT_PLAN_BAD_SIGMA = 4 };

// levels of the schedule of a kind and n: n + 1, or dpm_fast's two {sigma_max, sigma_min}
MDT_HD inline int mdt_plan_levels(int kind, int n) { return kind == MDT_SAMPLER_DPM_FAST ? 2 : n + 1; }

// largest n of a kind: steps, or dpm_fast's evaluations
MDT_HD inline int mdt_plan_max_n(int kind) {
    return kind == MDT_SAMPLER_DPM_FAST ? MDT_SAMPLER_MAX_EVALS : MDT_SAMPLER_MAX_STEPS;
}

// evaluations and noise rows of a plan, from the structure alone (the checks of mdt_sample run this before enqueuing)
MDT_HD inline int mdt_plan_shape(int kind, const mdt_sampler_params& p, int n, int* n_evals, int* n_noise) {
    if (kind < 0 || kind >= MDT_SAMPLER_COUNT) return MDT_PLAN_BAD_KIND;
    if (n < 1 || n > mdt_plan_max_n(kind)) return MDT_PLAN_BAD_STEPS;
    if (kind == MDT_SAMPLER_LMS && (p.order < 1 || p.order > 4)) return MDT_PLAN_BAD_ORDER;
    if (kind == MDT_SAMPLER_DPM_FAST) {  // n evaluations; one noise row per step with s_up != 0 (at most)
        *n_evals = n;
        *n_noise = p.eta != 0.f ? n / 3 + 1 : 0;
        return MDT_PLAN_OK;
    }
    const bool two = kind == MDT_SAMPLER_HEUN || kind == MDT_SAMPLER_DPM_2 || kind == MDT_SAMPLER_DPM_2_ANCESTRAL ||
                     kind == MDT_SAMPLER_DPMPP_2S || kind == MDT_SAMPLER_DPMPP_2S_ANCESTRAL || kind == MDT_SAMPLER_DPMPP_SDE;
    *n_evals = two ? 2 * n - 1 : n;
    switch (kind) {
        case MDT_SAMPLER_EULER: case MDT_SAMPLER_HEUN: case MDT_SAMPLER_DPM_2: case MDT_SAMPLER_DPMPP_2S_ANCESTRAL:
            *n_noise = n; break;  // eps every step (euler family: even at s_churn = 0), noise_sampler every step (2s_a)
        case MDT_SAMPLER_EULER_ANCESTRAL: case MDT_SAMPLER_DPM_2_ANCESTRAL:
            *n_noise = n - 1; break;  // while sigma_down > 0 (at most)
        case MDT_SAMPLER_DPMPP_SDE:
            *n_noise = p.eta != 0.f ? 2 * (n - 1) : 0; break;  // both sub-steps while sigma_up != 0 (at most)
        default:
            *n_noise = 0;
    }
    return MDT_PLAN_OK;
}

// whether the noise can change the result (else a call may pass no noise buffer)
MDT_HD inline bool mdt_plan_needs_noise(int kind, const mdt_sampler_params& p) {
    switch (kind) {
        case MDT_SAMPLER_EULER: case MDT_SAMPLER_HEUN: case MDT_SAMPLER_DPM_2:
            return p.s_churn > 0.f && p.s_noise != 0.f;
        case MDT_SAMPLER_EULER_ANCESTRAL: case MDT_SAMPLER_DPM_2_ANCESTRAL:
            return p.eta != 0.f;
        case MDT_SAMPLER_DPMPP_2S_ANCESTRAL: case MDT_SAMPLER_DPMPP_SDE: case MDT_SAMPLER_DPM_FAST:
            return p.eta != 0.f && p.s_noise != 0.f;
        default:
            return false;
    }
}

// The sampler step evaluation e belongs to, from the structure alone (mdt_sampler_eval::step of any plan of this kind and n): the
// host places a call's per-step record rows with it without reading a device plan.
MDT_HD inline int mdt_plan_step_of(int kind, int n, int e) {
    if (kind == MDT_SAMPLER_DPM_FAST) {  // orders 3 .. 3 then 2, 1 (3 | n) or n % 3: one evaluation per order
        const int m = n / 3 + 1;
        for (int i = 0, k = 0; i < m; ++i) {
            k += n % 3 == 0 ? (i < m - 2 ? 3 : i == m - 2 ? 2 : 1) : (i < m - 1 ? 3 : n % 3);
            if (e < k) return i;
        }
        return m - 1;
    }
    int evals = 0, rows = 0;
    mdt_plan_shape(kind, mdt_sampler_defaults(), n, &evals, &rows);
    return evals == n ? e : e / 2;  // two evaluations per step but the last
}

// Whether the reference's loop of this kind runs scaler.clip_output on the result of the step that evaluation e ends (`last`:
// e is the plan's final evaluation).  sample_dpmpp_2m and sample_dpm_fast take a scaler and never read it, and
// sample_dpmpp_sde leaves its final Euler step through `continue`, in front of the clip (reference gc_sampling.py:699-734,
// 673-697, 770-792); every other loop clips after every step.
MDT_HD inline bool mdt_plan_loop_clips(int kind, bool last) {
    if (kind == MDT_SAMPLER_DPMPP_2M || kind == MDT_SAMPLER_DPM_FAST) return false;
    return !(kind == MDT_SAMPLER_DPMPP_SDE && last);
}

namespace mdt_plan_detail {

// begins_step / ends_step of every evaluation, from its neighbours' `step`
MDT_HD inline void mark_steps(mdt_sampler_plan_t* P) {
    for (int k = 0; k < P->n_evals; ++k) {
        P->e[k].begins_step = k == 0 || P->e[k - 1].step != P->e[k].step;
        P->e[k].ends_step = k + 1 == P->n_evals || P->e[k + 1].step != P->e[k].step;
    }
}

struct Anc { float down, up; };
// get_ancestral_step (gc_sampling.py:97-103)
MDT_HD inline Anc ancestral(float from, float to, float eta) {
    if (eta == 0.f) return {to, 0.f};
    const float up = fminf(to, eta * sqrtf(to * to * (from * from - to * to) / (from * from)));
    return {sqrtf(to * to - up * up), up};
}
MDT_HD inline float t_of(float s) { return -logf(s); }
MDT_HD inline float s_of(float t) { return expf(-t); }
// torch.lerp(log a, log b, 0.5).exp(): the log-space midpoint of dpm_2 / dpm_2_ancestral
MDT_HD inline float log_mid(float a, float b) {
    const float la = logf(a), lb = logf(b);
    return expf(lb - (lb - la) * 0.5f);
}
// integral over [t[i], t[i+1]] of the j-th Lagrange basis polynomial through t[i], t[i-1], .., t[i-order+1]
// (linear_multistep_coeff, gc_sampling.py:406-419)
MDT_HD inline float lms_coeff(int order, const float* t, int i, int j) {
    const double a = t[i], b = t[i + 1], m = 0.5 * (a + b), h = 0.5 * (b - a);
    const double u = 0.7745966692414834, xs[3] = {m - h * u, m, m + h * u}, ws[3] = {5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0};
    double acc = 0.0;
    for (int q = 0; q < 3; ++q) {
        double prod = 1.0;
        for (int k = 0; k < order; ++k)
            if (k != j) prod *= (xs[q] - (double)t[i - k]) / ((double)t[i - j] - (double)t[i - k]);
        acc += ws[q] * prod;
    }
    return (float)(acc * h);
}

struct Builder {
    mdt_sampler_plan_t* P;
    int rows = 0;  // noise rows drawn so far (the loop's order)
    float* q = nullptr;  // dpmpp_sde with tree noise: the (from, to) points of every row (mdt_tree_q::q), or null
    MDT_HD mdt_sampler_eval& add(float sigma, int step) {
        mdt_sampler_eval& e = P->e[P->n_evals++];
        memset(&e, 0, sizeof e);
        e.sigma = sigma;
        e.noise[0] = e.noise[1] = -1;
        e.step = step;
        e.cy[MDT_SAMPLER_NREG] = 1.f;  // by default the next input is the new state
        return e;
    }
    // the noise slot of evaluation e that reads `row` (a free one if no slot reads it yet)
    MDT_HD static int slot(mdt_sampler_eval& e, int row) {
        if (e.noise[0] == row || e.noise[0] < 0) { e.noise[0] = row; return MDT_R_N0; }
        e.noise[1] = row;
        return MDT_R_N1;
    }
    // the next evaluation's input gets c * N[row] on top (sigma_hat churn): in the head of the evaluation before it, or in Y_0
    MDT_HD void churn(int row, float c) {
        if (P->n_evals == 0) { P->y0_noise = row; P->y0_cn = c; return; }
        mdt_sampler_eval& e = P->e[P->n_evals - 1];
        e.cy[slot(e, row)] += c;
    }
    // one more noise row drawn; returns its index
    MDT_HD int draw() {
        if (P->n_evals == 0) P->y0_draws += 1;
        else P->e[P->n_evals - 1].draws += 1;
        return rows++;
    }
    // an evaluation the loop skips (a sigma_down == 0 step before the last): the state passes through unchanged
    MDT_HD void pass(float sigma, int step) {
        mdt_sampler_eval& c = add(sigma, step);
        c.cx[MDT_R_X] = 1.f;
    }
};

// the points of dpmpp_sde's noise_sampler calls at step i as the host loop forms them from 0-dim fp32 tensors: sigma(t),
// sigma(t + h r), sigma(t_next), t = -ln(sigma), with ln / exp rounded once from double (dpm_t / dpm_s below: the correctly
// rounded fp32 results but in rare last-place cases, on the host and the device alike)
MDT_HD inline float dpm_t(float s);
MDT_HD inline float dpm_s(float t);
MDT_HD inline void sde_points(float s, float sn, float r, float* from, float* mid, float* next) {
#pragma clang fp contract(off)
    const float t = dpm_t(s), tn = dpm_t(sn), h = tn - t, sm = t + h * r;
    *from = dpm_s(t); *mid = dpm_s(sm); *next = dpm_s(tn);
}

// torch.linspace(t0, t1, m + 1)[i] in fp32 as torch's CPU kernel computes it: from the nearer end
MDT_HD inline float dpm_grid(float t0, float t1, int m, int i) {
    const float step = (t1 - t0) / (float)m;
    return i < (m + 1) / 2 ? fmaf(step, (float)i, t0) : fmaf(-step, (float)(m - i), t1);
}

// the DPM-Solver kinds' transcendental functions in double, rounded once to fp32: the same value on the host and the device,
// and the loop's (torch's fp32 log / exp / expm1 on the host) but in rare last-place cases.  dpm_fast's step size multiplies
// e^h ~ sigma_max / sigma_min: one ulp of t = -ln(sigma_max) (4.8e-7 at 80) moves a one-step result by ~1e-4.
MDT_HD inline float dpm_t(float s) { return -(float)log((double)s); }
MDT_HD inline float dpm_s(float t) { return (float)exp(-(double)t); }
MDT_HD inline float dpm_expm1(float x) { return (float)expm1((double)x); }

// one DPM-Solver step of order 1..3 from t to td (_dpm_stages + _dpm_combine, gc_sampling.py): eps_0 at t on the state, eps_k
// at the interior node k on the estimate the lower stages give there.  Every eps is d = (Y - D) / sigma of its evaluation;
// eps_0 and eps_1 are pushed (H0 the newest).  Returns the step's last evaluation.  No contraction: the products are the
// loop's 0-dim fp32 tensor products.
MDT_HD inline mdt_sampler_eval& dpm_step(Builder& b, float t, float td, int order, int step) {
#pragma clang fp contract(off)
    const float h = td - t, sn = dpm_s(td), em = dpm_expm1(h);
    const float c0 = sn * em;  // x - c0 eps_0: the order-1 update
    mdt_sampler_eval& a = b.add(dpm_s(t), step);
    a.t = t;
    a.cx[MDT_R_X] = 1.f;
    if (order == 1) { a.cx[MDT_R_DD] = -c0; return a; }
    const float r1 = order == 2 ? 0.5f : 1.f / 3.f, rh1 = r1 * h, s1 = t + rh1;
    a.push = MDT_PUSH_DD;
    a.cy[MDT_SAMPLER_NREG] = 0.f; a.cy[MDT_R_X] = 1.f; a.cy[MDT_R_DD] = -(dpm_s(s1) * dpm_expm1(rh1));
    mdt_sampler_eval& c = b.add(dpm_s(s1), step);
    c.t = s1;
    c.cx[MDT_R_X] = 1.f;
    if (order == 2) {  // x - c0 eps_0 - sn / (2 r_1) expm1(h) (eps_1 - eps_0), 2 r_1 = 1
        const float c1 = sn / 1.f * em;
        c.cx[MDT_R_H0] = c1 - c0; c.cx[MDT_R_DD] = -c1;
        return c;
    }
    // the second node's input: x - a2 eps_0 - b2 (eps_1 - eps_0), b2 = sigma(s2) (r2 / r1) (expm1(r2 h) / (r2 h) - 1)
    const float r2 = 2.f / 3.f, rh2 = r2 * h, s2 = t + rh2, e2 = dpm_expm1(rh2);
    const float a2 = dpm_s(s2) * e2, b2 = (dpm_s(s2) * 2.f) * (e2 / rh2 - 1.f);
    c.push = MDT_PUSH_DD;
    c.cy[MDT_SAMPLER_NREG] = 0.f; c.cy[MDT_R_X] = 1.f; c.cy[MDT_R_H0] = b2 - a2; c.cy[MDT_R_DD] = -b2;
    mdt_sampler_eval& d = b.add(dpm_s(s2), step);
    d.t = s2;
    // x - c0 eps_0 - sn / r2 (expm1(h) / h - 1) (eps_2 - eps_0); H0 = eps_1, H1 = eps_0
    const float c2 = sn / r2 * (em / h - 1.f);
    d.cx[MDT_R_X] = 1.f; d.cx[MDT_R_H0 + 1] = c2 - c0; d.cx[MDT_R_DD] = -c2;
    return d;
}

// _dpm_fast_run (gc_sampling.py): m = n // 3 + 1 steps on linspace(t_start, t_end, m + 1), orders 3 .. 3 then 2, 1 (3 | n)
// or n % 3; with eta != 0 each step ends at _ancestral_split's t_det and adds s_up s_noise times one noise row
MDT_HD inline void dpm_fast(Builder& b, const mdt_sampler_params& p, const float* sig, int n) {
#pragma clang fp contract(off)
    const float t0 = dpm_t(sig[0]), t1 = dpm_t(sig[1]);
    const int m = n / 3 + 1;
    for (int i = 0; i < m; ++i) {
        const int order = n % 3 == 0 ? (i < m - 2 ? 3 : i == m - 2 ? 2 : 1) : (i < m - 1 ? 3 : n % 3);
        const float t = dpm_grid(t0, t1, m, i), tn = dpm_grid(t0, t1, m, i + 1);
        float td = tn, up = 0.f;
        if (p.eta != 0.f) {
            const Anc an = ancestral(dpm_s(t), dpm_s(tn), p.eta);
            td = fminf(t1, dpm_t(an.down));
            const float sa = dpm_s(tn), sd = dpm_s(td);
            up = sqrtf(sa * sa - sd * sd);
        }
        mdt_sampler_eval& z = dpm_step(b, t, td, order, i);
        if (up != 0.f) z.cx[Builder::slot(z, b.draw())] = (float)((double)up * (double)p.s_noise);
    }
}

}  // namespace mdt_plan_detail

// one attempted step of _dpm_adaptive_run (gc_sampling.py) from s to t at order 2 or 3: the stages of dpm_step.  The last
// evaluation's cx is the order-k combine ("high", the head's X'), its cy the order-(k-1) combine on the same stages ("low",
// the head's Y', written to the low buffer; nothing is embedded after it): order 2 -> x - c0 eps_0; order 3 -> the order-2
// combine with r_1 = 1/3, x - c0 eps_0 - sn / (2 r_1) expm1(h) (eps_1 - eps_0).
MDT_HD inline void mdt_dpm_adaptive_step_plan(int order, float s, float t, mdt_sampler_plan_t* P) {
#pragma clang fp contract(off)
    using namespace mdt_plan_detail;
    P->n_evals = 0; P->n_noise = 0; P->y0_noise = -1; P->y0_cn = 0.f; P->y0_draws = 0;
    P->pad[0] = P->pad[1] = P->pad[2] = 0;
    Builder b{P};
    mdt_sampler_eval& z = dpm_step(b, s, t, order, 0);
    for (int k = 0; k < P->n_evals; ++k) P->e[k].sigma_next = k + 1 < P->n_evals ? P->e[k + 1].sigma : 0.f;
    mark_steps(P);
    const float h = t - s, sn = dpm_s(t), em = dpm_expm1(h), c0 = sn * em;
    for (int k = 0; k <= MDT_SAMPLER_NREG; ++k) z.cy[k] = 0.f;
    z.cy[MDT_R_X] = 1.f;
    if (order == 2) {  // H0 = eps_0
        z.cy[MDT_R_H0] = -c0;
    } else {  // H0 = eps_1, H1 = eps_0
        const float c1 = sn / (2.f / 3.f) * em;
        z.cy[MDT_R_H0 + 1] = c1 - c0; z.cy[MDT_R_H0] = -c1;
    }
}

// _StepControl (gc_sampling.py) in the same double arithmetic: log domain, arctan limiter, history shift on accept
inline void mdt_dpm_control_start(mdt_dpm_control* c, double h, double kp, double ki, double kd, double order, double safety) {
    memset(c, 0, sizeof *c);
    c->h = h;
    c->w[0] = (kp + ki + kd) / order; c->w[1] = -(kp + 2 * kd) / order; c->w[2] = kd / order;
    c->safety = safety;
    c->eps = 1e-8;
}
// MDT_DPM_ACCEPT / _REJECT, or _STOP where the error or the new h is NaN (the Python loop never ends there)
inline int mdt_dpm_control_step(mdt_dpm_control* c, float error) {
    const double cur = -log((double)error + c->eps);
    if (!c->started) { c->hist[0] = c->hist[1] = c->hist[2] = cur; c->started = 1; }
    else c->hist[0] = cur;
    double acc = 0.0;
    for (int i = 0; i < 3; ++i) acc += c->w[i] * c->hist[i];
    const double factor = 1.0 + atan(exp(acc) - 1.0);
    const bool ok = factor >= c->safety;
    if (ok) { c->hist[2] = c->hist[1]; c->hist[1] = cur; }
    c->h *= factor;
    if (error != error || c->h != c->h) return MDT_DPM_STOP;
    return ok ? MDT_DPM_ACCEPT : MDT_DPM_REJECT;
}

// the schedule checks of the host entry points (a device schedule is not read back): dpm_fast's two levels must be > 0, and
// eta != 0 needs t_end > t_start (sample_dpm_fast's ValueErrors)
inline int mdt_plan_check_levels(int kind, const mdt_sampler_params& p, const float* sig) {
    if (kind != MDT_SAMPLER_DPM_FAST) return MDT_PLAN_OK;
    if (!(sig[0] > 0.f) || !(sig[1] > 0.f)) return MDT_PLAN_BAD_SIGMA;
    if (p.eta != 0.f && !(mdt_plan_detail::dpm_t(sig[1]) > mdt_plan_detail::dpm_t(sig[0]))) return MDT_PLAN_BAD_SIGMA;
    return MDT_PLAN_OK;
}

// the LMS coefficients of step i (cur = min(i + 1, order) of them) -> c[0..cur-1]; independent across steps, so the device
// computes them one step per thread before the serial build (k_sampler_plan)
MDT_HD inline void mdt_lms_step_coeffs(int order, const float* sig, int i, float* c) {
    const int cur = i + 1 < order ? i + 1 : order;
    for (int j = 0; j < cur; ++j) c[j] = mdt_plan_detail::lms_coeff(cur, sig, i, j);
}

// sig: mdt_plan_levels(kind, n) levels.  lms: nullptr, or the n x 4 table of mdt_lms_step_coeffs (the same values, computed beforehand).
// queries: nullptr, or (dpmpp_sde) 2 floats per noise row that receive the row's (from, to) points (sde_points).
// Returns MDT_PLAN_*.
MDT_HD inline int mdt_build_sampler_plan(int kind, const mdt_sampler_params& p, const float* sig, int n, mdt_sampler_plan_t* P,
                                         const float* lms = nullptr, float* queries = nullptr) {
    using namespace mdt_plan_detail;
    int n_evals = 0, n_noise = 0;
    const int st = mdt_plan_shape(kind, p, n, &n_evals, &n_noise);
    if (st != MDT_PLAN_OK) return st;
    P->n_evals = 0;
    P->n_noise = 0;
    P->y0_noise = -1;
    P->y0_cn = 0.f;
    P->y0_draws = 0;
    P->pad[0] = P->pad[1] = P->pad[2] = 0;
    Builder b{P};
    b.q = queries;
    if (kind == MDT_SAMPLER_DPM_FAST) dpm_fast(b, p, sig, n);
    for (int i = 0; i < n && kind != MDT_SAMPLER_DPM_FAST; ++i) {
        const float s = sig[i], sn = sig[i + 1];
        const bool last = i == n - 1;
        switch (kind) {
            case MDT_SAMPLER_EULER: case MDT_SAMPLER_HEUN: case MDT_SAMPLER_DPM_2: {
                // gamma, sigma_hat and the churn of Algorithm 2 (gc_sampling.py:231-235): eps = randn * s_noise every step
                const double gamma = (p.s_tmin <= s && s <= p.s_tmax) ? fmin((double)p.s_churn / n, 1.4142135623730951 - 1.0) : 0.0;
                const float sh = s * (float)(gamma + 1.0);
                const int row = b.draw();
                if (gamma > 0.0) b.churn(row, p.s_noise * sqrtf(sh * sh - s * s));
                const float dt = sn - sh;
                mdt_sampler_eval& a = b.add(sh, i);
                if (kind == MDT_SAMPLER_EULER || last) {  // Euler step (heun / dpm_2 on the step to sigma = 0)
                    a.cx[MDT_R_Y] = 1.f; a.cx[MDT_R_DD] = dt;
                } else if (kind == MDT_SAMPLER_HEUN) {  // x_2 = x + d dt; x + (d + d_2) / 2 dt
                    a.cx[MDT_R_Y] = 1.f; a.push = MDT_PUSH_DD;
                    a.cy[MDT_SAMPLER_NREG] = 0.f; a.cy[MDT_R_Y] = 1.f; a.cy[MDT_R_DD] = dt;
                    mdt_sampler_eval& c = b.add(sn, i);
                    c.cx[MDT_R_X] = 1.f; c.cx[MDT_R_H0] = 0.5f * dt; c.cx[MDT_R_DD] = 0.5f * dt;
                } else {  // dpm_2: x_2 = x + d (sigma_mid - sigma_hat); x + d_2 dt
                    const float sm = log_mid(sh, sn);
                    a.cx[MDT_R_Y] = 1.f;
                    a.cy[MDT_SAMPLER_NREG] = 0.f; a.cy[MDT_R_Y] = 1.f; a.cy[MDT_R_DD] = sm - sh;
                    mdt_sampler_eval& c = b.add(sm, i);
                    c.cx[MDT_R_X] = 1.f; c.cx[MDT_R_DD] = dt;
                }
                break;
            }
            case MDT_SAMPLER_EULER_ANCESTRAL: {
                const Anc an = ancestral(s, sn, p.eta);
                mdt_sampler_eval& a = b.add(s, i);
                a.cx[MDT_R_Y] = 1.f; a.cx[MDT_R_DD] = an.down - s;
                if (an.down > 0.f) a.cx[Builder::slot(a, b.draw())] = an.up;
                break;
            }
            case MDT_SAMPLER_DPM_2_ANCESTRAL: {
                const Anc an = ancestral(s, sn, p.eta);
                mdt_sampler_eval& a = b.add(s, i);
                if (an.down == 0.f) {
                    a.cx[MDT_R_Y] = 1.f; a.cx[MDT_R_DD] = an.down - s;
                    if (!last) b.pass(sn, i);
                    break;
                }
                const float sm = log_mid(s, an.down);
                a.cx[MDT_R_Y] = 1.f;
                a.cy[MDT_SAMPLER_NREG] = 0.f; a.cy[MDT_R_Y] = 1.f; a.cy[MDT_R_DD] = sm - s;
                mdt_sampler_eval& c = b.add(sm, i);
                c.cx[MDT_R_X] = 1.f; c.cx[MDT_R_DD] = an.down - s;
                c.cx[Builder::slot(c, b.draw())] = an.up;
                break;
            }
            case MDT_SAMPLER_LMS: {
                mdt_sampler_eval& a = b.add(s, i);
                const int cur = i + 1 < p.order ? i + 1 : p.order;
                a.cx[MDT_R_Y] = 1.f;
                float c[4];
                if (lms) for (int j = 0; j < cur; ++j) c[j] = lms[4 * i + j];
                else mdt_lms_step_coeffs(p.order, sig, i, c);
                for (int j = 0; j < cur; ++j) a.cx[j == 0 ? MDT_R_DD : MDT_R_H0 + j - 1] = c[j];
                a.push = MDT_PUSH_DD;
                break;
            }
            case MDT_SAMPLER_DPMPP_2M: {
                mdt_sampler_eval& a = b.add(s, i);
                const float t = t_of(s), tn = t_of(sn), h = tn - t;
                const float ratio = s_of(tn) / s_of(t), em1 = expm1f(-h);
                a.cx[MDT_R_Y] = ratio;
                if (i == 0 || last) {
                    a.cx[MDT_R_D] = -em1;
                } else {
                    const float r = (t - t_of(sig[i - 1])) / h;
                    a.cx[MDT_R_D] = -em1 * (1.f + 1.f / (2.f * r));
                    a.cx[MDT_R_H0] = em1 * (1.f / (2.f * r));
                }
                a.push = MDT_PUSH_D;
                break;
            }
            case MDT_SAMPLER_DPMPP_2S: case MDT_SAMPLER_DPMPP_2S_ANCESTRAL: {
                const Anc an = kind == MDT_SAMPLER_DPMPP_2S ? Anc{sn, 0.f} : ancestral(s, sn, p.eta);
                mdt_sampler_eval& a = b.add(s, i);
                mdt_sampler_eval* fin = &a;
                if (an.down == 0.f) {  // Euler to sigma_down = 0
                    a.cx[MDT_R_Y] = 1.f; a.cx[MDT_R_DD] = an.down - s;
                } else {
                    const float t = t_of(s), tn = t_of(an.down), h = tn - t, sm = t + 0.5f * h;
                    a.cx[MDT_R_Y] = 1.f;
                    a.cy[MDT_SAMPLER_NREG] = 0.f; a.cy[MDT_R_Y] = s_of(sm) / s_of(t); a.cy[MDT_R_D] = -expm1f(-h * 0.5f);
                    mdt_sampler_eval& c = b.add(s_of(sm), i);
                    c.cx[MDT_R_X] = s_of(tn) / s_of(t); c.cx[MDT_R_D] = -expm1f(-h);
                    fin = &c;
                }
                if (kind == MDT_SAMPLER_DPMPP_2S_ANCESTRAL) fin->cx[Builder::slot(*fin, b.draw())] = p.s_noise * an.up;
                if (an.down == 0.f && !last) b.pass(sn, i);
                break;
            }
            case MDT_SAMPLER_DPMPP_SDE: {
                mdt_sampler_eval& a = b.add(s, i);
                if (last) { a.cx[MDT_R_Y] = 1.f; a.cx[MDT_R_DD] = sn - s; break; }
                const float t = t_of(s), tn = t_of(sn), h = tn - t, sm = t + h * p.r, fac = 1.f / (2.f * p.r);
                const Anc a1 = ancestral(s_of(t), s_of(sm), p.eta);
                const float s1 = t_of(a1.down);
                a.cx[MDT_R_Y] = 1.f; a.push = MDT_PUSH_D;
                a.cy[MDT_SAMPLER_NREG] = 0.f; a.cy[MDT_R_Y] = s_of(s1) / s_of(t); a.cy[MDT_R_D] = -expm1f(t - s1);
                float qf = 0.f, qm = 0.f, qn = 0.f;
                if (b.q) sde_points(s, sn, p.r, &qf, &qm, &qn);
                if (a1.up != 0.f) {
                    const int row = b.draw();
                    a.cy[Builder::slot(a, row)] = p.s_noise * a1.up;
                    if (b.q) { b.q[2 * row] = qf; b.q[2 * row + 1] = qm; }
                }
                mdt_sampler_eval& c = b.add(s_of(sm), i);
                const Anc a2 = ancestral(s_of(t), s_of(tn), p.eta);
                const float t2 = t_of(a2.down), em = expm1f(t - t2);
                c.cx[MDT_R_X] = s_of(t2) / s_of(t);
                c.cx[MDT_R_H0] = -em * (1.f - fac);
                c.cx[MDT_R_D] = -em * fac;
                if (a2.up != 0.f) {
                    const int row = b.draw();
                    c.cx[Builder::slot(c, row)] = p.s_noise * a2.up;
                    if (b.q) { b.q[2 * row] = qf; b.q[2 * row + 1] = qn; }
                }
                break;
            }
        }
    }
    P->n_noise = b.rows;
    for (int k = 0; k < P->n_evals; ++k) P->e[k].sigma_next = k + 1 < P->n_evals ? P->e[k + 1].sigma : 0.f;
    mark_steps(P);
    mdt_sampler_eval& z = P->e[P->n_evals - 1];
    for (int k = 0; k <= MDT_SAMPLER_NREG; ++k) z.cy[k] = 0.f;  // nothing follows the last evaluation
    return MDT_PLAN_OK;
}

// The tree-noise rows of a dpmpp_sde call (mdt_sample_sde_tree*): the plan records the (from, to) points of every noise row,
// and the schedule's interval, beside the plan in device memory; k_brownian_fill (mdt_brownian.hip) reads them.
struct mdt_tree_q {
    double lo, hi;                        // the schedule's smallest positive and largest level
    int32_t n, pad;                       // noise rows of the plan
    float q[2 * MDT_SAMPLER_MAX_EVALS];   // (from, to) of row r at q[2 r], q[2 r + 1]
};

// lo / hi of a schedule of `levels` levels (the reference's sigma_min = smallest positive level, sigma_max = largest)
MDT_HD inline void mdt_tree_interval(const float* sig, int levels, double* lo, double* hi) {
    float l = INFINITY, h = -INFINITY;
    for (int i = 0; i < levels; ++i) {
        if (sig[i] > 0.f && sig[i] < l) l = sig[i];
        if (sig[i] > h) h = sig[i];
    }
    *lo = l; *hi = h;
}
