// mdt_loglik.h -- what mdt_log_likelihood (mdt_loglik.hip: the integrator's kernels and host loop) takes from the training path
// (mdt_train.hip: tapes, the eval-mode encoder, the tape-keeping decoder forward, the input-gradient-only backward), and the one
// launcher the training path takes from it.
#pragma once
#include "mdt_model_types.h"

// one run: the B observations' tape (encoder activations, context, K|V of B*Te rows) and the decoder's tape at R = B*K rows
struct mdt_ll_run {
    mdt_tape_id enc = -1, dec = -1;
    int64_t B = 0;
    int K = 1;
};

// the handle is prepared and loaded and no staged loss backward is under way on it (MDT_ERR_STATE); nothing is enqueued
mdt_status mdt_ll_check(mdt_model* m, const char* fn);
// both tapes acquired on `s`, the backward's scratch reserved at R rows and entered
mdt_status mdt_ll_open(mdt_model* m, int64_t B, int K, hipStream_t s, mdt_ll_run* r);
// eval-mode encoder on the B observations (sigma: (B,), read only when it is a context token), the stacked cross K|V product on
// B*Te rows, each observation's K|V rows K times into the decoder tape (K == 1: the product writes there directly)
mdt_status mdt_ll_context(mdt_model* m, const mdt_ll_run& r, const float* tokens, const float* tokens2, const float* goal,
                          int modality, const float* sigma, hipStream_t s);
// the decoder forward on the R rows against the staged K|V, kept on the tape; x (R, Ta, A), sigma (R,)
mdt_status mdt_ll_forward(mdt_model* m, const mdt_ll_run& r, const float* x, const float* sigma, hipStream_t s);
// over that tape: denoised = D(x; sigma) (optional) and vjp = (dD/dx)^T v; the tape is only read
mdt_status mdt_ll_vjp(mdt_model* m, const mdt_ll_run& r, const float* v, float* denoised, float* vjp, hipStream_t s);
// mdt_ll_vjp's backward between a seed and a finish launch of the caller's (mdt_steer.hip swaps both for its own): over the
// R * Ta * A = n elements, the seed reads the tape (F the raw network output, x the forward's input, sigma per row) and leaves the
// upstream gradient of F in dF; the finish reads small = d y0 . Wa, the gradient at the network's input c_in x
struct mdt_ll_io {
    const float *F, *x, *sigma;
    float *dF, *small;
    int64_t n;
    int per;  // Ta * A
    float sd;
};
typedef hipError_t (*mdt_ll_launch)(const mdt_ll_io& io, void* arg, hipStream_t s);
mdt_status mdt_ll_backward(mdt_model* m, const mdt_ll_run& r, mdt_ll_launch seed, mdt_ll_launch finish, void* arg, hipStream_t s);
// the B observations' context (B, Te, D) on the encoder tape, as mdt_ll_context left it
const float* mdt_ll_ctx(mdt_model* m, const mdt_ll_run& r);
// tapes released, scratch handed back; safe after a failed open (ids < 0 are skipped)
mdt_status mdt_ll_close(mdt_model* m, const mdt_ll_run& r, hipStream_t s);

// dst (B*K, w) <- row b of src (B, w) at rows b*K .. b*K + K - 1; w % 4 == 0, both 16-byte aligned
hipError_t mdt_launch_ll_repeat_rows(const float* src, float* dst, int64_t B, int K, int64_t w, hipStream_t s);
