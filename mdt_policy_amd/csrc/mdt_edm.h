// mdt_edm.h -- the EDM preconditioning (score_wrappers.py:59-80) and one step of the action embedding, stated once for the
// kernels that need them:
//     den2 = sigma^2 + sd^2,   c_in = 1 / sqrt(den2),   c_skip = sd^2 / den2,   c_out = sigma sd / sqrt(den2),
//     D(x; sigma) = c_out F + c_skip x,   y[n..n+3] = ba[n..n+3] + sum_c (x_c c_in) WaT[c][n..n+3].
// Plain device functions, no state.  Every rounding is written out -- an explicit fmaf, or products and a sum with contraction
// off -- so a kernel's bits follow from the functions it calls, not from what the compiler fuses in its context: two kernels that
// call the same functions on the same values agree bit for bit, and two that call different ones are known not to.
//
// den2 exists in three roundings and the combine D in two (DESIGN.md 4.3l lists every site, and which kernels therefore agree).
// The forms differ by at most one ulp of their result and none is more right than another, but a c_in is the same number only
// where the form is the same.  A new kernel takes the form of the kernel whose values it has to reproduce.
#pragma once
#include "mdt_device.h"

// both squares rounded, then their sum: rn(rn(sigma^2) + rn(sd^2)).  The form of the decoder's own embedding (k_action_embed),
// and so of whatever hands the decoder the rows it would have made itself (k_score_prep).
__device__ __forceinline__ float edm_den2_round_both(float sigma, float sd) {
#pragma clang fp contract(off)
    return sigma * sigma + sd * sd;
}
// sd^2 rounded, sigma^2 exact inside the fma: rn(sigma^2 + rn(sd^2)).  The form wherever c_skip's sd^2 stands beside it.
__device__ __forceinline__ float edm_den2_round_sd(float sigma, float sd) { return fmaf(sigma, sigma, sd * sd); }
// sigma^2 rounded, sd^2 exact inside the fma: rn(rn(sigma^2) + sd^2).  The samplers' first embedding.
__device__ __forceinline__ float edm_den2_round_sigma(float sigma, float sd) { return fmaf(sd, sd, sigma * sigma); }

__device__ __forceinline__ float edm_c_in(float den2) { return 1.0f / sqrtf(den2); }
__device__ __forceinline__ float edm_c_skip(float sd, float den2) { return sd * sd / den2; }
__device__ __forceinline__ float edm_c_out(float sigma, float sd, float den2) { return sigma * sd / sqrtf(den2); }

// D = c_out F + c_skip x.  The training and steer paths: the skip term rounded, the network's term exact inside the fma ...
__device__ __forceinline__ float edm_denoised(float F, float x, float c_out, float c_skip) { return fmaf(F, c_out, x * c_skip); }
// ... and the wide sampler head: both products rounded, then their sum
__device__ __forceinline__ float edm_denoised_round_both(float F, float x, float c_out, float c_skip) {
#pragma clang fp contract(off)
    return F * c_out + x * c_skip;
}

// One input of a row's action embedding, columns n..n+3: acc += (xin c_in) wrow[0..3], the product rounded, each column one fma.
// The embedding is this step over the A inputs in order c = 0 .. A - 1, from acc = ba[n..n+3], with wrow = WaT + c D + n (the
// weight stored transposed, (A, D)).  xin is the row's c-th network input before the c_in scaling.  The loop stays with the
// caller: some kernels form, and store, xin inside it.
__device__ __forceinline__ f32x4 action_embed_step(f32x4 acc, float xin, float c_in, const float* wrow) {
    const float xv = xin * c_in;
    const f32x4 w = *(const f32x4*)wrow;
    acc.x = fmaf(xv, w.x, acc.x); acc.y = fmaf(xv, w.y, acc.y);
    acc.z = fmaf(xv, w.z, acc.z); acc.w = fmaf(xv, w.w, acc.w);
    return acc;
}
