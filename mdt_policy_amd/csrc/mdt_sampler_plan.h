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

enum { MDT_PLAN_OK = 0, MDT_PLAN_BAD_KIND = 1, MDT_PLAN_BAD_STEPS = 2, MDT_PLAN_BAD_ORDER = 3 };

// evaluations and noise rows of a plan, from the structure alone (the checks of mdt_sample run this before enqueuing)
MDT_HD inline int mdt_plan_shape(int kind, const mdt_sampler_params& p, int n, int* n_evals, int* n_noise) {
    if (kind < 0 || kind >= MDT_SAMPLER_COUNT) return MDT_PLAN_BAD_KIND;
    if (n < 1 || n > MDT_SAMPLER_MAX_STEPS) return MDT_PLAN_BAD_STEPS;
    if (kind == MDT_SAMPLER_LMS && (p.order < 1 || p.order > 4)) return MDT_PLAN_BAD_ORDER;
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
        case MDT_SAMPLER_DPMPP_2S_ANCESTRAL: case MDT_SAMPLER_DPMPP_SDE:
            return p.eta != 0.f && p.s_noise != 0.f;
        default:
            return false;
    }
}

namespace mdt_plan_detail {

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

}  // namespace mdt_plan_detail

// the LMS coefficients of step i (cur = min(i + 1, order) of them) -> c[0..cur-1]; independent across steps, so the device
// computes them one step per thread before the serial build (k_sampler_plan)
MDT_HD inline void mdt_lms_step_coeffs(int order, const float* sig, int i, float* c) {
    const int cur = i + 1 < order ? i + 1 : order;
    for (int j = 0; j < cur; ++j) c[j] = mdt_plan_detail::lms_coeff(cur, sig, i, j);
}

// sig: n + 1 levels.  lms: nullptr, or the n x 4 table of mdt_lms_step_coeffs (the same values, computed beforehand).
// Returns MDT_PLAN_*.
MDT_HD inline int mdt_build_sampler_plan(int kind, const mdt_sampler_params& p, const float* sig, int n, mdt_sampler_plan_t* P,
                                         const float* lms = nullptr) {
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
    for (int i = 0; i < n; ++i) {
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
                if (a1.up != 0.f) a.cy[Builder::slot(a, b.draw())] = p.s_noise * a1.up;
                mdt_sampler_eval& c = b.add(s_of(sm), i);
                const Anc a2 = ancestral(s_of(t), s_of(tn), p.eta);
                const float t2 = t_of(a2.down), em = expm1f(t - t2);
                c.cx[MDT_R_X] = s_of(t2) / s_of(t);
                c.cx[MDT_R_H0] = -em * (1.f - fac);
                c.cx[MDT_R_D] = -em * fac;
                if (a2.up != 0.f) c.cx[Builder::slot(c, b.draw())] = p.s_noise * a2.up;
                break;
            }
        }
    }
    P->n_noise = b.rows;
    for (int k = 0; k < P->n_evals; ++k) P->e[k].sigma_next = k + 1 < P->n_evals ? P->e[k + 1].sigma : 0.f;
    mdt_sampler_eval& z = P->e[P->n_evals - 1];
    for (int k = 0; k <= MDT_SAMPLER_NREG; ++k) z.cy[k] = 0.f;  // nothing follows the last evaluation
    return MDT_PLAN_OK;
}
