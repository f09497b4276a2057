// mdt_loglik.h -- the tape path of mdt_log_likelihood (mdt_loglik.hip), mdt_sample_ddim_steer and mdt_sample_steer (mdt_steer.hip):
// what they take from the training path (mdt_train.hip: tapes, the eval-mode encoder, the tape-keeping decoder forward, the
// input-gradient-only backward), the frame all three entries stand in, and the launcher mdt_train.hip takes from mdt_loglik.hip.
#pragma once
#include <algorithm>
#include <initializer_list>

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

// ---- the frame of an entry: mdt_ll_check_head, the entry's own checks, mdt_ll_check_tail, then mdt_ll_scoped around its body.
// No check enqueues; every refusal is "<fn>: ..." through mdt_fail.
struct mdt_ll_ptr {
    const void* p;
    const char* name;
};
// null handle, tokens, goal, the entry's own required pointers in the order given, batch < 1, candidates < 1
inline mdt_status mdt_ll_check_head(const char* fn, const mdt_model* m, const float* tokens, const float* goal,
                                    std::initializer_list<mdt_ll_ptr> own, int64_t batch, int candidates) {
    if (!m) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: null handle", fn);
    if (!tokens) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: null tokens", fn);
    if (!goal) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: null goal", fn);
    for (const mdt_ll_ptr& o : own)
        if (!o.p) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: null %s", fn, o.name);
    if (batch < 1) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: batch is %lld, must be >= 1", fn, (long long)batch);
    if (candidates < 1) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: candidates is %d, must be >= 1", fn, candidates);
    return MDT_OK;
}
// MDT_ERR_STATE "<fn>: <reason> cannot be captured" while `s` is capturing (mdt_sample_dpm_adaptive's refusal too)
inline mdt_status mdt_refuse_capture(hipStream_t s, const char* fn, const char* reason) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing(s, &cs));
    return cs == hipStreamCaptureStatusNone ? MDT_OK : mdt_fail(MDT_ERR_STATE, "%s: %s cannot be captured", fn, reason);
}
// the handle's side: tokens2 where MDT or use_proprio needs it, mdt_ll_check between the two, the decoder's rows, the capture
inline mdt_status mdt_ll_check_tail(mdt_model* m, const char* fn, const float* tokens2, int64_t batch, int candidates, hipStream_t s,
                                    const char* reason) {
    if (m->cfg.arch == MDT_ARCH_MDT && !tokens2)
        return mdt_fail(MDT_ERR_INVALID_ARG, "%s: null tokens2: MDT needs the gripper tokens", fn);
    MDT_TRY(mdt_ll_check(m, fn));
    if (m->p_row >= 0 && !tokens2)
        return mdt_fail(MDT_ERR_INVALID_ARG, "%s: null tokens2: this handle was created with use_proprio and needs state_obs", fn);
    const int64_t limit = ((int64_t)1 << 24) / std::max(m->Te, m->Ta);  // the decoder's row counts (int)
    if (batch > limit / candidates)
        return mdt_fail(MDT_ERR_INVALID_ARG, "%s: batch * candidates = %lld * %d is more than the decoder's %lld samples", fn,
                        (long long)batch, candidates, (long long)limit);
    return mdt_refuse_capture(s, fn, reason);
}
// mdt_ll_open, `body` only if that succeeded, mdt_ll_close on every path; the first failure is the result, with its own message
template <class Body>
mdt_status mdt_ll_scoped(mdt_model* m, int64_t B, int K, hipStream_t s, mdt_ll_run* r, Body body) {
    mdt_status st = mdt_ll_open(m, B, K, s, r);
    if (st == MDT_OK) st = body();
    const mdt_status closed = mdt_ll_close(m, *r, s);
    return st != MDT_OK ? st : closed;
}

// dst (B*K, w) <- row b of src (B, w) at rows b*K .. b*K + K - 1; w % 4 == 0, both 16-byte aligned
hipError_t mdt_launch_ll_repeat_rows(const float* src, float* dst, int64_t B, int K, int64_t w, hipStream_t s);
