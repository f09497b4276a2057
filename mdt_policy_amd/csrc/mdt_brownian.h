// The virtual Brownian tree behind mdt_brownian_noise and the tree-noise dpmpp_sde calls (include/mdt_hip.h): one routine
// for the host (mdt_brownian_noise_host) and the device (k_brownian_fill, mdt_brownian.hip).  The value of the path at any
// point is a pure function of (seed, element, point): the Levy midpoint construction on [lo, hi] (Li et al. 2020, the idea
// behind torchsde's BrownianTree), so values at different points are jointly a Brownian path whatever is asked, in any order.
//
//   W(lo) = 0, W(hi) = sqrt(hi - lo) z(0, e)
//   walk to t (clamped to [lo, hi]) from a = lo, b = hi, node = 1 while b - a > tol (at most MDT_BT_MAX_DEPTH levels):
//     m = a + (b - a) / 2,  W(m) = (W(a) + W(b)) / 2 + 0.5 sqrt(b - a) z(node, e)
//     t < m: [a, m], node = 2 node;  else: [m, b], node = 2 node + 1
//   W(t) = W(a) + (t - a) / (b - a) (W(b) - W(a))
//   z(node, e): Box-Muller on the words of philox4(seed, site = e, ctr = node) (mdt_device.h), u1 = (k1 + 1) 2^-53 and
//   u2 = k2 2^-53 with k1 = (w0 >> 5) 2^26 + (w1 >> 6), k2 the same of w2, w3; z = sqrt(-2 ln u1) cos(2 pi u2)
//   noise value of (from, to): (W(to) - W(from)) / sqrt(|to - from|), in double, rounded once to fp32
//
// Everything is double and uncontracted, so the host and the device agree up to their libm's last double place.
#pragma once

#include <math.h>
#include <stdint.h>

#include "mdt_device.h"

#define MDT_BT_MAX_DEPTH 62  // node < 2^63

// the standard normal z(node, e) of the tree keyed by seed
__host__ __device__ inline double mdt_bt_normal(uint64_t seed, uint32_t e, uint64_t node) {
#pragma clang fp contract(off)
    const philox4_t r = philox4(seed, e, node);
    const uint64_t k1 = ((uint64_t)(r.w[0] >> 5) << 26) + (r.w[1] >> 6);
    const uint64_t k2 = ((uint64_t)(r.w[2] >> 5) << 26) + (r.w[3] >> 6);
    const double u1 = (double)(k1 + 1) * 0x1p-53, u2 = (double)k2 * 0x1p-53;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// one node of a walk: the interval [a, b], the path at its ends, the node number and its depth
struct mdt_bt_node {
    double a, b, wa, wb;
    uint64_t node;
    int depth;
};

__host__ __device__ inline mdt_bt_node mdt_bt_root(uint64_t seed, uint32_t e, double lo, double hi) {
#pragma clang fp contract(off)
    return {lo, hi, 0.0, sqrt(hi - lo) * mdt_bt_normal(seed, e, 0), 1, 0};
}

// the midpoint of n's interval and the path there
__host__ __device__ inline void mdt_bt_mid(uint64_t seed, uint32_t e, const mdt_bt_node& n, double* m, double* wm) {
#pragma clang fp contract(off)
    *m = n.a + (n.b - n.a) / 2;
    *wm = (n.wa + n.wb) / 2 + 0.5 * sqrt(n.b - n.a) * mdt_bt_normal(seed, e, n.node);
}

__host__ __device__ inline bool mdt_bt_open(const mdt_bt_node& n, double tol) {
    return n.depth < MDT_BT_MAX_DEPTH && n.b - n.a > tol;
}

__host__ __device__ inline void mdt_bt_step(mdt_bt_node& n, bool left, double m, double wm) {
    if (left) { n.b = m; n.wb = wm; n.node = 2 * n.node; }
    else { n.a = m; n.wa = wm; n.node = 2 * n.node + 1; }
    ++n.depth;
}

// W(t) from node n down (t inside n's interval)
__host__ __device__ inline double mdt_bt_finish(uint64_t seed, uint32_t e, mdt_bt_node n, double tol, double t) {
#pragma clang fp contract(off)
    while (mdt_bt_open(n, tol)) {
        double m, wm;
        mdt_bt_mid(seed, e, n, &m, &wm);
        mdt_bt_step(n, t < m, m, wm);
    }
    return n.wa + (t - n.a) / (n.b - n.a) * (n.wb - n.wa);
}

__host__ __device__ inline double mdt_bt_clamp(double t, double lo, double hi) { return t < lo ? lo : (t > hi ? hi : t); }

// W(t) of the tree (seed, e) on [lo, hi]
__host__ __device__ inline double mdt_bt_value(uint64_t seed, uint32_t e, double lo, double hi, double tol, double t) {
    return mdt_bt_finish(seed, e, mdt_bt_root(seed, e, lo, hi), tol, mdt_bt_clamp(t, lo, hi));
}

// the noise value of (from, to): both walks share their path from the root down to the level where they part (the same
// nodes, so the same values as two separate walks)
__host__ __device__ inline float mdt_bt_increment(uint64_t seed, uint32_t e, double lo, double hi, double tol, double from,
                                                  double to) {
#pragma clang fp contract(off)
    const double f = mdt_bt_clamp(from, lo, hi), t = mdt_bt_clamp(to, lo, hi);
    mdt_bt_node n = mdt_bt_root(seed, e, lo, hi);
    while (mdt_bt_open(n, tol)) {
        double m, wm;
        mdt_bt_mid(seed, e, n, &m, &wm);
        if ((f < m) != (t < m)) break;
        mdt_bt_step(n, f < m, m, wm);
    }
    const double wf = mdt_bt_finish(seed, e, n, tol, f), wt = mdt_bt_finish(seed, e, n, tol, t);
    return (float)((wt - wf) / sqrt(fabs(to - from)));
}

// levels a walk on [lo, hi] takes at most before the interval is <= tol; > MDT_BT_MAX_DEPTH: the tolerance is too fine
inline int mdt_bt_depth(double lo, double hi, double tol) {
    int d = 0;
    for (double w = hi - lo; w > tol && d <= MDT_BT_MAX_DEPTH; w /= 2) ++d;
    return d;
}
