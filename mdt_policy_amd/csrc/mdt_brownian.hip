// mdt_brownian.hip -- Brownian-tree noise (include/mdt_hip.h: mdt_brownian_noise, mdt_brownian_noise_host, and the rows of the
// tree-noise dpmpp_sde calls, mdt_model.hip: sample_plan_impl).  The tree itself is mdt_brownian.h.
//
// One thread per (row, element): a row's two points share their walk from the root down to the level where they part
// (mdt_bt_increment), so a thread takes about one walk's worth of normals for close points and two for distant ones.  Per element
// the rows of a dpmpp_sde call ask for 2 n - 1 distinct points; walking each once per element (one thread per element) would
// halve the normals but leave 1/18 of the threads -- the walk is a chain of dependent double transcendentals and needs the
// threads to hide its latency.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "mdt_internal.h"
#include "mdt_brownian.h"
#include "mdt_sampler_plan.h"

namespace {

struct BtArgs {
    const uint64_t* seeds;
    int32_t n_seeds, n_q;        // n_q: the rows (pairs below), or the rows launched for (tq: rows beyond tq->n exit)
    double lo, hi, tol;          // lo >= hi: tq's interval
    const mdt_tree_q* tq;        // the plan's points, or null: pairs
    int64_t nel, per_row;
    float* out;                  // (n_q, nel)
    double pairs[2 * MDT_BROWNIAN_MAX_PAIRS];
};

// the value of row r, element k (host and device)
__host__ __device__ inline float bt_row_value(const BtArgs& a, double lo, double hi, double from, double to, int64_t k) {
    const int64_t b = k / a.per_row;
    const uint64_t seed = a.n_seeds == 1 ? a.seeds[0] : a.seeds[b];
    const uint32_t e = (uint32_t)(a.n_seeds == 1 ? k : k - b * a.per_row);
    return mdt_bt_increment(seed, e, lo, hi, a.tol, from, to);
}

__global__ __launch_bounds__(256) void k_brownian_fill(BtArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = idx / a.nel, k = idx - r * a.nel;
    if (r >= a.n_q) return;
    double from, to, lo = a.lo, hi = a.hi;
    if (a.tq) {
        if (r >= a.tq->n) return;
        from = a.tq->q[2 * r];
        to = a.tq->q[2 * r + 1];
        if (!(lo < hi)) { lo = a.tq->lo; hi = a.tq->hi; }
    } else {
        from = a.pairs[2 * r];
        to = a.pairs[2 * r + 1];
    }
    a.out[idx] = bt_row_value(a, lo, hi, from, to, k);
}

hipError_t launch_fill(const BtArgs& a, hipStream_t s) {
    const int64_t n = (int64_t)a.n_q * a.nel;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_brownian_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// the checks both entry points share
mdt_status check_tree(const char* who, const void* seeds, int32_t n_seeds, double lo, double hi, double tol, int64_t batch,
                      int64_t per_row) {
    // (sample_plan_impl, mdt_model.hip, gives a tree entry without its tree this text too: change both together)
    if (!seeds || batch < 1 || per_row < 1 || (n_seeds != 1 && n_seeds != batch))
        return mdt_fail(MDT_ERR_INVALID_ARG, "%s: bad argument (seeds, n_seeds = 1 or batch, batch, per_row)", who);
    if (batch * per_row > (int64_t)UINT32_MAX) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: more than 2^32 - 1 elements", who);
    if (!(tol > 0.0) || !isfinite(tol)) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: tol must be finite and > 0", who);
    if (lo == 0.0 && hi == 0.0) return MDT_OK;  // the schedule's interval (mdt_brownian_source)
    if (!(lo < hi) || !isfinite(lo) || !isfinite(hi)) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: the tree needs lo < hi", who);
    if (mdt_bt_depth(lo, hi, tol) > MDT_BT_MAX_DEPTH)
        return mdt_fail(MDT_ERR_INVALID_ARG, "%s: tol %g needs more than %d levels on [%g, %g]", who, tol, MDT_BT_MAX_DEPTH, lo, hi);
    return MDT_OK;
}

mdt_status noise_args(const char* who, const uint64_t* seeds, int32_t n_seeds, double lo, double hi, double tol, const double* pairs,
                      int32_t n_q, int64_t batch, int64_t per_row, float* out, BtArgs* a) {
    MDT_TRY(check_tree(who, seeds, n_seeds, lo, hi, tol, batch, per_row));
    if (lo == 0.0 && hi == 0.0) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: the tree needs lo < hi", who);
    if (n_q < 0 || (n_q > 0 && (!pairs || !out))) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: bad argument (pairs, n_q, out)", who);
    a->seeds = seeds; a->n_seeds = n_seeds; a->n_q = n_q;
    a->lo = lo; a->hi = hi; a->tol = tol;
    a->tq = nullptr;
    a->nel = batch * per_row; a->per_row = per_row;
    a->out = out;
    return MDT_OK;
}

}  // namespace

mdt_status mdt_check_brownian_source(const char* who, const mdt_brownian_source* src, int64_t batch, int64_t per_row) {
    if (!src) return mdt_fail(MDT_ERR_INVALID_ARG, "%s: null tree", who);
    return check_tree(who, src->seeds, src->n_seeds, src->lo, src->hi, src->tol, batch, per_row);
}

hipError_t mdt_launch_brownian_fill(const mdt_tree_q* tq, const mdt_brownian_source& src, int max_rows, int64_t nel, int64_t per_row,
                                    float* out, hipStream_t s) {
    BtArgs a;
    memset(&a, 0, sizeof a);
    a.seeds = src.seeds; a.n_seeds = src.n_seeds; a.n_q = max_rows;
    a.lo = src.lo; a.hi = src.hi; a.tol = src.tol;
    a.tq = tq;
    a.nel = nel; a.per_row = per_row;
    a.out = out;
    return launch_fill(a, s);
}

extern "C" mdt_status mdt_brownian_noise(const uint64_t* seeds, int32_t n_seeds, double lo, double hi, double tol, const double* pairs,
                                         int32_t n_q, int64_t batch, int64_t per_row, float* out, void* stream) {
    BtArgs a;
    memset(&a, 0, sizeof a);
    MDT_TRY(noise_args("mdt_brownian_noise", seeds, n_seeds, lo, hi, tol, pairs, n_q, batch, per_row, out, &a));
    if (n_q > MDT_BROWNIAN_MAX_PAIRS)
        return mdt_fail(MDT_ERR_INVALID_ARG, "mdt_brownian_noise: at most %d pairs per call", (int)MDT_BROWNIAN_MAX_PAIRS);
    for (int i = 0; i < 2 * n_q; ++i) a.pairs[i] = pairs[i];
    LAUNCH(launch_fill(a, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_brownian_noise_host(const uint64_t* seeds, int32_t n_seeds, double lo, double hi, double tol,
                                              const double* pairs, int32_t n_q, int64_t batch, int64_t per_row, float* out) {
    BtArgs a;
    memset(&a, 0, sizeof a);
    MDT_TRY(noise_args("mdt_brownian_noise_host", seeds, n_seeds, lo, hi, tol, pairs, n_q, batch, per_row, out, &a));
    for (int32_t r = 0; r < n_q; ++r)
        for (int64_t k = 0; k < a.nel; ++k) out[r * a.nel + k] = bt_row_value(a, lo, hi, pairs[2 * r], pairs[2 * r + 1], k);
    return MDT_OK;
}
