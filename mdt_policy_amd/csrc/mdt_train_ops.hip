// mdt_train_ops.hip -- the Linear backward built from the forward fp32-MFMA GEMM, and the kernel-level C ABI of
// the training path (include/mdt_hip_train.h, "kernel level").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <mutex>
#include <vector>

#include "mdt_internal.h"

#define fail mdt_fail

// out = X W^T (+ b):
//   dW[n][k] = sum_m dY[m][n] X[m][k]  -> GEMM with row operand dY^T (N x Mp, materialised by a transpose) and the
//              "weight" X^T packed as an (N' = K, K' = Mp) image: out'(N x K) = dY^T . (X^T)^T
//   dX[m][k] = sum_n dY[m][n] W[n][k]  -> GEMM with row operand dY and the packed image of W^T (N' = K, K' = N)
// Mp = M rounded up to 16; the pad columns / k-slices are zero, so they add nothing.
// The slicing of the row reduction, the kernel and the scratch layout of a call are ONE plan (mdt_route_train.h:
// mdt_route_linear_bwd): mdt_linear_bwd executes it, and the two scratch sizes are read off the same function.
int64_t mdt_linear_bwd_scratch(int64_t M, int64_t N, int64_t K) { return mdt_route_linear_bwd_scratch(M, N, K); }

mdt_status mdt_linear_bwd(const mdt_linear_bwd_args& a, hipStream_t s, mdt_colsum_entry* defer_bias, float* bias_space) {
    if (a.M < 1 || a.N < 1 || a.K < 1 || (a.K % 16)) return fail(MDT_ERR_INVALID_ARG, "linear_bwd: bad shape");
    // every refusal comes before the first launch: a refused call has enqueued nothing, so a caller may correct its arguments
    // and call again without counting a gradient twice
    if (a.dW && (a.N % 16)) return fail(MDT_ERR_INVALID_ARG, "linear_bwd: N must be a multiple of 16 for dW");
    if (a.dX) {
        if (!a.Wt || (a.N % 16)) return fail(MDT_ERR_INVALID_ARG, "linear_bwd: dX needs the packed W^T and N % 16 == 0");
        if (a.dx_act_u) {
            if (a.accumulate_dx || a.N > 512) return fail(MDT_ERR_INVALID_ARG, "linear_bwd: dx_act_u needs accumulate_dx = 0 and N <= 512");
            if (a.dx_act == MDT_ACT_SWIGLU && a.ldxo < 2 * (int64_t)a.K)
                return fail(MDT_ERR_INVALID_ARG, "linear_bwd: SwishGLU backward writes 2 K columns (ldxo >= 2 K)");
        }
    }
    if (defer_bias) defer_bias->src = nullptr;
    // the plan: which dW path, how many slices, where each region of `scratch` lies (mdt_route_train.h)
    const mdt_linear_bwd_plan p = mdt_route_linear_bwd(a.M, a.N, a.K, !(a.ldy % 4) && !(a.ldx % 4), a.dW != nullptr, a.dbias != nullptr,
                                                       mdt_route_snapshot());
    const int S = p.S, L = p.L;
    const bool bias_from_partials = p.bias_from_partials;   // the dW path also leaves the bias gradient's partial column sums
    if (a.dbias && !bias_from_partials) LAUNCH(mdt_launch_colsum(a.dY, a.ldy, a.M, a.N, a.dbias, a.accumulate_dw, s));
    float* parts = a.scratch + p.parts;                          // [S][N][K] partial products (S > 1)
    if (p.path == MDT_DW_TN || p.path == MDT_DW_TN_SPLIT) {
        // dW straight from dY and X: one batched launch, then partial products and the bias gradient's per-slice column sums
        // added up in a fixed order
        const bool defer = a.dbias && defer_bias && bias_space && S <= 256;
        float* bpart = defer ? bias_space : a.scratch + p.bpart;   // [S][N]
        if (p.path == MDT_DW_TN_SPLIT)
            LAUNCH(mdt_launch_gemm_tn_split(a.dY, a.ldy, a.X, a.ldx, S > 1 ? parts : a.dW, (int64_t)a.N * a.K, a.M, a.N, a.K, S, L,
                                            S > 1 ? 0 : a.accumulate_dw, a.dbias ? bpart : nullptr, s));
        else
            LAUNCH(mdt_launch_gemm_tn(a.dY, a.ldy, a.X, a.ldx, S > 1 ? parts : a.dW, (int64_t)a.N * a.K, a.M, a.N, a.K, S, L,
                                      S > 1 ? 0 : a.accumulate_dw, a.dbias ? bpart : nullptr, s));
        if (S > 1) LAUNCH(mdt_launch_colsum(parts, (int64_t)a.N * a.K, S, a.N * a.K, a.dW, a.accumulate_dw, s));
        if (defer) *defer_bias = mdt_colsum_entry{bpart, a.dbias, (int64_t)a.N, S, a.N, a.accumulate_dw};
        else if (a.dbias) LAUNCH(mdt_launch_colsum(bpart, a.N, S, a.N, a.dbias, a.accumulate_dw, s));
    } else if (p.path == MDT_DW_COPY) {
        float* dYt = a.scratch + p.dYt;                          // [S][N][L]
        float* Xt = a.scratch + p.Xt;                            // [S] packed (N' = K, K' = L)
        float* bpart = a.scratch + p.bpart;                      // (ceil(M/32), N) column partials of dY
        if ((int64_t)S * L != a.M) {  // zero pad rows of the last slice
            HIP_TRY(hipMemsetAsync(dYt + (int64_t)(S - 1) * a.N * L, 0, (size_t)a.N * L * sizeof(float), s));
            HIP_TRY(hipMemsetAsync(Xt + (int64_t)(S - 1) * a.K * L, 0, (size_t)a.K * L * sizeof(float), s));
        }
        LAUNCH(mdt_launch_transpose_ld(a.dY, a.ldy, dYt, L, a.M, a.N, bias_from_partials ? bpart : nullptr, s, L));
        if (bias_from_partials) LAUNCH(mdt_launch_colsum(bpart, a.N, (a.M + 31) / 32, a.N, a.dbias, a.accumulate_dw, s));
        LAUNCH(mdt_launch_pack_weight_t(a.X, a.M, a.K, a.ldx, Xt, 0, L / 16, s, L));
        Lin w;
        w.wp = Xt; w.bias = nullptr; w.N = a.K; w.K = L;
        mdt_gemm_args g = gemm_args(dYt, L, w, S > 1 ? parts : a.dW, a.K, a.N);
        if (S > 1) {
            g.batch = S; g.bs_a = (int64_t)a.N * L; g.bs_w = (int64_t)a.K * L; g.bs_out = (int64_t)a.N * a.K;
        } else {
            g.residual = a.accumulate_dw;
        }
        LAUNCH(mdt_launch_gemm(g, s));
        if (S > 1) LAUNCH(mdt_launch_colsum(parts, (int64_t)a.N * a.K, S, a.N * a.K, a.dW, a.accumulate_dw, s));
    }
    if (a.dX) {
        Lin w;
        w.wp = const_cast<float*>(a.Wt); w.bias = nullptr; w.N = a.K; w.K = a.N;
        mdt_gemm_args g = gemm_args(a.dY, a.ldy, w, a.dX, a.ldxo, a.M);
        g.residual = a.accumulate_dx;
        if (a.dx_act_u) {  // dX = (dY W) * act'(u): the activation's backward rides on this product's epilogue
            g.aux = a.dx_act_u; g.aux_mode = 2; g.act = a.dx_act;
            if (a.dx_act == MDT_ACT_SWIGLU) {  // dX (M, 2K; ldxo) from d = dY W (M, K) and u (M, 2K; ldxo)
                g.aux_mode = 4; g.act = MDT_ACT_NONE;
            }
        }
        LAUNCH(mdt_launch_gemm(g, s));
    }
    return MDT_OK;
}

extern "C" int64_t mdt_op_linear_bwd_scratch(int64_t M, int64_t N, int64_t K) { return mdt_linear_bwd_scratch(M, N, K); }
extern "C" int64_t mdt_op_linear_bwd_scratch_exact(int64_t M, int64_t N, int64_t K) { return mdt_route_linear_bwd_scratch_exact(M, N, K); }

extern "C" mdt_status mdt_op_linear_bwd(const mdt_linear_bwd_args* a, void* stream) {
    if (!a || !a->X || !a->dY || !a->scratch) return fail(MDT_ERR_INVALID_ARG, "mdt_op_linear_bwd: null argument");
    return mdt_linear_bwd(*a, (hipStream_t)stream);
}

extern "C" mdt_status mdt_op_pack_weight_t(const float* src, int64_t rows, int64_t cols, int64_t ld, float* packed,
                                           int64_t k_off, int64_t k_total, void* stream) {
    if (!src || !packed || rows < 0 || cols < 1 || (cols % 16) || (k_total % 16) || k_off < 0 || k_off + rows > k_total)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_pack_weight_t: bad argument");
    LAUNCH(mdt_launch_pack_weight_t(src, (int)rows, (int)cols, ld, packed, (int)k_off, (int)(k_total / 16),
                                    (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_ln_fwd_train(const mdt_ln_train_args* a, void* stream) {
    if (!a || !a->x || !a->w || !a->out || a->M < 1) return fail(MDT_ERR_INVALID_ARG, "mdt_op_ln_fwd_train: bad argument");
    LAUNCH(mdt_launch_ln_fwd_train(*a, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_ln_bwd(const mdt_ln_bwd_args* a, void* stream) {
    if (!a || !a->x || !a->stats || !a->w || !a->dh || !a->dx || !a->pw || a->B < 1)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_ln_bwd: bad argument");
    LAUNCH(mdt_launch_ln_bwd(*a, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_attn_bwd(const mdt_attn_bwd_args* a, void* stream) {
    if (!a || !a->q || !a->k || !a->v || !a->d_out || !a->dq || !a->dk || !a->dv)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_attn_bwd: null argument");
    LAUNCH(mdt_launch_attn_bwd(*a, (hipStream_t)stream));
    return MDT_OK;
}
// test hook (mdt_hip_debug.h): the backward of the decoder's cross-attention at a context above 16 tokens
extern "C" mdt_status mdt_op_attn_bwd_prefix(const mdt_attn_bwd_args* a, int32_t kv_rows, void* stream) {
    if (!a || !a->q || !a->k || !a->v || !a->d_out || !a->dq || !a->dk || !a->dv)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_attn_bwd_prefix: null argument");
    if (!mdt_prefix_rows_ok(a->Tq, a->Tk, a->causal, kv_rows))
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_attn_bwd_prefix: kv_rows %d: 0, Tk, or min(Tq, Tk) .. Tk - 1 of a causal launch with Tk > 16", kv_rows);
    LAUNCH(mdt_launch_attn_bwd(*a, (hipStream_t)stream, kv_rows));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_act_fwd(const float* u, float* out, int64_t n, int32_t act, void* stream) {
    if (!u || !out || n < 1) return fail(MDT_ERR_INVALID_ARG, "mdt_op_act_fwd: bad argument");
    LAUNCH(mdt_launch_act_fwd(u, out, n, act, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_act_bwd(const float* u, const float* dy, float* du, int64_t n, int32_t act, void* stream) {
    if (!u || !dy || !du || n < 1) return fail(MDT_ERR_INVALID_ARG, "mdt_op_act_bwd: bad argument");
    LAUNCH(mdt_launch_act_bwd(u, dy, du, n, act, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_merge_fwd(const mdt_merge_args* a, void* stream) {
    if (!a || !a->x || !a->a || !a->out || a->B < 1 || a->rows_per_sample < 1)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_merge_fwd: bad argument");
    LAUNCH(mdt_launch_merge_fwd(*a, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_merge_bwd(const mdt_merge_args* a, void* stream) {
    if (!a || !a->x || !a->a || !a->out || a->B < 1 || a->rows_per_sample < 1)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_merge_bwd: bad argument");
    LAUNCH(mdt_launch_merge_bwd(*a, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_merge_ln_fwd(const mdt_merge_args* g, const mdt_ln_train_args* l, void* stream) {
    if (!g || !l || !g->x || !g->a || !g->out || !l->w || !l->out || g->B < 1 || g->rows_per_sample < 1 ||
        (int64_t)g->B * g->rows_per_sample != l->M || g->D != l->D)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_merge_ln_fwd: bad argument");
    LAUNCH(mdt_launch_merge_ln_fwd(*g, *l, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_ln_bwd_merge(const mdt_ln_bwd_args* a, const mdt_merge_args* g, void* stream) {
    if (!a || !g || !a->x || !a->stats || !a->w || !a->dh || !a->dx || !a->pw || a->B < 1 || !g->a || !g->out ||
        g->B != a->B || g->rows_per_sample != a->rows_per_sample || g->D != a->D)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_ln_bwd_merge: bad argument");
    LAUNCH(mdt_launch_ln_bwd_merge(*a, *g, (hipStream_t)stream));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_attn_fwd_train(const mdt_attn_train_args* a, void* stream) {
    if (!a || !a->q || !a->k || !a->v || !a->out) return fail(MDT_ERR_INVALID_ARG, "mdt_op_attn_fwd_train: null argument");
    LAUNCH(mdt_launch_attn_fwd_train(*a, (hipStream_t)stream));
    return MDT_OK;
}
// test hook (mdt_hip_debug.h): the training forward of the decoder's cross-attention at a context above 16 tokens
extern "C" mdt_status mdt_op_attn_fwd_train_prefix(const mdt_attn_train_args* a, int32_t kv_rows, void* stream) {
    if (!a || !a->q || !a->k || !a->v || !a->out) return fail(MDT_ERR_INVALID_ARG, "mdt_op_attn_fwd_train_prefix: null argument");
    if (!mdt_prefix_rows_ok(a->Tq, a->Tk, a->causal, kv_rows))
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_attn_fwd_train_prefix: kv_rows %d: 0, Tk, or min(Tq, Tk) .. Tk - 1 of a causal launch with Tk > 16", kv_rows);
    LAUNCH(mdt_launch_attn_fwd_train(*a, (hipStream_t)stream, kv_rows));
    return MDT_OK;
}

extern "C" mdt_status mdt_op_colsum(const float* X, int64_t ldx, int64_t M, int64_t N, float* out, int32_t accumulate,
                                    void* stream) {
    if (!X || !out || M < 1 || N < 1) return fail(MDT_ERR_INVALID_ARG, "mdt_op_colsum: bad argument");
    LAUNCH(mdt_launch_colsum(X, ldx, (int)M, (int)N, out, accumulate, (hipStream_t)stream));
    return MDT_OK;
}

// test hooks (mdt_hip_debug.h): the narrow linears around the action tokens, each through the launcher the step calls
extern "C" mdt_status mdt_op_narrow_dw(const float* G, const float* Y, int64_t ldy, float* partial, int32_t n_slices, int32_t M,
                                       int32_t A, int32_t D, int32_t transposed, void* stream) {
    if (!G || !Y || !partial) return fail(MDT_ERR_INVALID_ARG, "mdt_op_narrow_dw: null argument");
    if (M < 1 || A < 1 || A > MDT_ACTION_DIM_MAX || D < 1 || n_slices < 1 || n_slices > 65535 || ldy < D)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_narrow_dw: M %d, A %d (1..%d), D %d, n_slices %d (1..65535), ldy %lld (>= D)", M, A,
                    MDT_ACTION_DIM_MAX, D, n_slices, (long long)ldy);
    LAUNCH(mdt_launch_narrow_dw(G, Y, ldy, partial, n_slices, M, A, D, transposed != 0, (hipStream_t)stream));
    return MDT_OK;
}
extern "C" mdt_status mdt_op_narrow_out(const float* G, int64_t ldg, const float* WT, float* out, int32_t M, int32_t A, int32_t D,
                                        void* stream) {
    if (!G || !WT || !out) return fail(MDT_ERR_INVALID_ARG, "mdt_op_narrow_out: null argument");
    if (M < 1 || A < 1 || A > MDT_ACTION_DIM_MAX || D < 1 || ldg < D)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_narrow_out: M %d, A %d (1..%d), D %d, ldg %lld (>= D)", M, A, MDT_ACTION_DIM_MAX, D,
                    (long long)ldg);
    LAUNCH(mdt_launch_narrow_out(G, ldg, WT, out, M, A, D, (hipStream_t)stream));
    return MDT_OK;
}
extern "C" mdt_status mdt_op_narrow_dx(const float* G, const float* W, float* out, int32_t M, int32_t A, int32_t D, void* stream) {
    if (!G || !W || !out) return fail(MDT_ERR_INVALID_ARG, "mdt_op_narrow_dx: null argument");
    if (M < 1 || A < 1 || A > MDT_ACTION_DIM_MAX || D < 1)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_narrow_dx: M %d, A %d (1..%d), D %d", M, A, MDT_ACTION_DIM_MAX, D);
    LAUNCH(mdt_launch_narrow_dx(G, W, out, M, A, D, (hipStream_t)stream));
    return MDT_OK;
}

// ------------------------------------------------------------------------------------------------
// multi-tensor optimizer updates: the (tensor, chunk) table of a call lives in device memory.  A training loop passes the
// same pointers step after step, so the tables are cached by content (16 slots per device, least recently used replaced -- the reference's
// configure_optimizers builds 6-7 parameter groups plus the EMA list --, pinned staging): a repeated
// table costs nothing, a new one is one asynchronous copy -- the call never waits for the stream (a stream
// synchronisation here cost 1.5 ms per B = 1024 step: the host lost its run-ahead over the backward's launches).
// ------------------------------------------------------------------------------------------------
namespace {
struct OptSlot {
    void* dev = nullptr;
    void* host = nullptr;  // pinned
    size_t cap = 0;
    hipEvent_t ev = nullptr;  // recorded behind the kernel that last read `dev`
    hipStream_t stream = nullptr;  // ... and the stream it was recorded on (the upload was enqueued there as well)
    bool busy = false;
    std::vector<char> key;    // the caller's table bytes this slot holds
    size_t tab_bytes = 0;
    size_t ctl_off = 0;       // 16 bytes behind table and block list: the control block of mdt_op_multi_adamw_dev
    int n_blocks = 0;
    uint64_t last_use = 0;
};
struct OptTable {  // one per device: the tables live in that device's memory
    std::mutex mu;
    OptSlot slots[16];
    uint64_t clock = 0;
    // the per-chunk partials of mdt_op_multi_sumsq for callers that bring none: grown on demand, never shrunk
    float* partial = nullptr;
    size_t partial_cap = 0;   // floats
    hipEvent_t partial_ev = nullptr;  // behind the last k_sumsq_finish that read it, on partial_stream
    hipStream_t partial_stream = nullptr;
    bool partial_busy = false;
};
OptTable g_opt_dev[32];
}  // namespace

static mdt_status upload_opt_table(OptTable& g_opt, const mdt_opt_tensor* tensors, int n, const mdt_opt_tensor** d_tab,
                                   const int2** d_blocks, int* n_blocks, OptSlot** used, hipStream_t s) {
    const int CH = 4096;  // OPT_CHUNK of the kernels
    const size_t key_bytes = (size_t)n * sizeof(mdt_opt_tensor);
    for (OptSlot& sl : g_opt.slots)
        if (sl.dev && sl.key.size() == key_bytes && memcmp(sl.key.data(), tensors, key_bytes) == 0) {
            *d_tab = (const mdt_opt_tensor*)sl.dev;
            *d_blocks = (const int2*)((const char*)sl.dev + sl.tab_bytes);
            *n_blocks = sl.n_blocks;
            *used = &sl;
            sl.last_use = ++g_opt.clock;
            // a hit from ANOTHER stream: the table's copy (and its last reader) were enqueued elsewhere -- order behind them
            if (sl.busy && sl.stream != s) HIP_TRY(hipStreamWaitEvent(s, sl.ev, 0));
            return MDT_OK;
        }
    std::vector<int2> blocks;
    for (int i = 0; i < n; ++i) {
        if (tensors[i].numel < 0 || tensors[i].numel > ((int64_t)1 << 31) - CH)
            return fail(MDT_ERR_INVALID_ARG, "multi-tensor update: tensor %d has an unsupported size", i);
        for (int64_t off = 0; off < tensors[i].numel; off += CH) blocks.push_back(make_int2(i, (int)off));
    }
    const size_t tab_bytes = (key_bytes + 255) & ~(size_t)255;
    const size_t data_bytes = tab_bytes + blocks.size() * sizeof(int2);
    const size_t total = ((data_bytes + 15) & ~(size_t)15) + 16;  // + the control block (device only, never copied)
    OptSlot* lru = &g_opt.slots[0];
    for (OptSlot& c : g_opt.slots)
        if (c.last_use < lru->last_use) lru = &c;
    OptSlot& sl = *lru;
    sl.last_use = ++g_opt.clock;
    if (!sl.ev) HIP_TRY(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (sl.busy) HIP_TRY(hipEventSynchronize(sl.ev));  // the last kernel that read this slot (long done in practice)
    if (total > sl.cap) {
        if (sl.dev) HIP_TRY(hipFree(sl.dev));
        if (sl.host) HIP_TRY(hipHostFree(sl.host));
        sl.dev = sl.host = nullptr; sl.cap = 0;
        HIP_TRY(hipMalloc(&sl.dev, total * 2));
        HIP_TRY(hipHostMalloc(&sl.host, total * 2, hipHostMallocDefault));
        sl.cap = total * 2;
    }
    memcpy(sl.host, tensors, key_bytes);
    memcpy((char*)sl.host + tab_bytes, blocks.data(), blocks.size() * sizeof(int2));
    HIP_TRY(hipMemcpyAsync(sl.dev, sl.host, data_bytes, hipMemcpyHostToDevice, s));
    sl.key.assign((const char*)tensors, (const char*)tensors + key_bytes);
    sl.tab_bytes = tab_bytes;
    sl.ctl_off = total - 16;
    sl.n_blocks = (int)blocks.size();
    *d_tab = (const mdt_opt_tensor*)sl.dev;
    *d_blocks = (const int2*)((const char*)sl.dev + tab_bytes);
    *n_blocks = sl.n_blocks;
    *used = &sl;
    return MDT_OK;
}

// a byte blob (move table + block list of k_multi_load) through the same content-keyed slots
static mdt_status upload_blob(OptTable& g_opt, const std::vector<char>& bytes, const void** dev, OptSlot** used, hipStream_t s) {
    for (OptSlot& sl : g_opt.slots)
        if (sl.dev && sl.key.size() == bytes.size() && memcmp(sl.key.data(), bytes.data(), bytes.size()) == 0) {
            *dev = sl.dev; *used = &sl;
            sl.last_use = ++g_opt.clock;
            if (sl.busy && sl.stream != s) HIP_TRY(hipStreamWaitEvent(s, sl.ev, 0));  // see upload_opt_table
            return MDT_OK;
        }
    OptSlot* lru = &g_opt.slots[0];
    for (OptSlot& c : g_opt.slots)
        if (c.last_use < lru->last_use) lru = &c;
    OptSlot& sl = *lru;
    sl.last_use = ++g_opt.clock;
    if (!sl.ev) HIP_TRY(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (sl.busy) HIP_TRY(hipEventSynchronize(sl.ev));
    if (bytes.size() > sl.cap) {
        if (sl.dev) HIP_TRY(hipFree(sl.dev));
        if (sl.host) HIP_TRY(hipHostFree(sl.host));
        sl.dev = sl.host = nullptr; sl.cap = 0;
        HIP_TRY(hipMalloc(&sl.dev, bytes.size() * 2));
        HIP_TRY(hipHostMalloc(&sl.host, bytes.size() * 2, hipHostMallocDefault));
        sl.cap = bytes.size() * 2;
    }
    memcpy(sl.host, bytes.data(), bytes.size());
    HIP_TRY(hipMemcpyAsync(sl.dev, sl.host, bytes.size(), hipMemcpyHostToDevice, s));
    sl.key = bytes;
    sl.tab_bytes = 0; sl.n_blocks = 0;
    *dev = sl.dev; *used = &sl;
    return MDT_OK;
}

// Fragment-packed images of n Linear weights (N_i, K_i) -- the forward operand into wp[i] and, where wt[i] is given, the image
// of W^T for dX = dY W -- in ONE launch (a training step re-packs every weight of a module after its optimizer step).
extern "C" mdt_status mdt_op_pack_many(int32_t n, const float* const* srcs, const int32_t* N, const int32_t* K, float* const* wp,
                                       float* const* wt, void* stream) {
    if (n < 0 || (n > 0 && (!srcs || !N || !K || !wp))) return fail(MDT_ERR_INVALID_ARG, "mdt_op_pack_many: bad argument");
    if (n == 0) return MDT_OK;
    std::vector<mdt_load_entry> tab;
    std::vector<int2> blocks;
    auto add = [&](const float* src, float* dst, int kind, int rows, int Kc, int p1) {
        mdt_load_entry e;
        memset(&e, 0, sizeof e);
        e.src = src; e.dst = dst; e.kind = kind; e.rows = rows; e.K = Kc; e.p0 = 0; e.p1 = p1;
        const int64_t work = kind == MDT_LOAD_PACK_T ? (int64_t)((rows + 3) / 4) * Kc : (int64_t)rows * (Kc / 4);
        for (int64_t c = 0; c * 1024 < work; ++c) blocks.push_back(make_int2((int)tab.size(), (int)c));
        tab.push_back(e);
    };
    for (int i = 0; i < n; ++i) {
        if (!srcs[i] || !wp[i] || N[i] < 16 || K[i] < 16 || (N[i] % 16) || (K[i] % 16) || ((uintptr_t)srcs[i] & 15) || ((uintptr_t)wp[i] & 15))
            return fail(MDT_ERR_INVALID_ARG, "mdt_op_pack_many: entry %d (N, K multiples of 16; 16-byte aligned pointers)", i);
        add(srcs[i], wp[i], MDT_LOAD_PACK, N[i], K[i], 0);
        if (wt && wt[i]) add(srcs[i], wt[i], MDT_LOAD_PACK_T, N[i], K[i], N[i] / 16);
    }
    const size_t tab_bytes = (tab.size() * sizeof(mdt_load_entry) + 255) & ~(size_t)255;
    std::vector<char> bytes(tab_bytes + blocks.size() * sizeof(int2), 0);
    memcpy(bytes.data(), tab.data(), tab.size() * sizeof(mdt_load_entry));
    memcpy(bytes.data() + tab_bytes, blocks.data(), blocks.size() * sizeof(int2));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 32) return fail(MDT_ERR_INVALID_ARG, "device index %d out of range", dev);
    OptTable& g_opt = g_opt_dev[dev];
    std::lock_guard<std::mutex> lock(g_opt.mu);
    hipStream_t s = (hipStream_t)stream;
    const void* d = nullptr;
    OptSlot* slot = nullptr;
    MDT_TRY(upload_blob(g_opt, bytes, &d, &slot, s));
    LAUNCH(mdt_launch_multi_load((const mdt_load_entry*)d, (const int2*)((const char*)d + tab_bytes), (int)blocks.size(), s));
    HIP_TRY(hipEventRecord(slot->ev, s));
    slot->busy = true;
    slot->stream = s;
    return MDT_OK;
}

extern "C" mdt_status mdt_op_multi_adamw(const mdt_opt_tensor* tensors, int32_t n, float lr, float beta1, float beta2,
                                         float eps, float weight_decay, int64_t step, void* stream) {
    if (!tensors || n < 0 || step < 1) return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_adamw: bad argument");
    for (int i = 0; i < n; ++i)
        if (!tensors[i].p || !tensors[i].g || !tensors[i].m || !tensors[i].v)
            return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_adamw: tensor %d lacks p / g / m / v", i);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 32) return fail(MDT_ERR_INVALID_ARG, "device index %d out of range", dev);
    OptTable& g_opt = g_opt_dev[dev];
    std::lock_guard<std::mutex> lock(g_opt.mu);
    hipStream_t s = (hipStream_t)stream;
    const mdt_opt_tensor* tab; const int2* blocks; int nb;
    OptSlot* slot = nullptr;
    MDT_TRY(upload_opt_table(g_opt, tensors, n, &tab, &blocks, &nb, &slot, s));
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    LAUNCH(mdt_launch_multi_adamw(tab, blocks, nb, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)std::sqrt(bc2), s));
    HIP_TRY(hipEventRecord(slot->ev, s));
    slot->busy = true;
    slot->stream = s;
    return MDT_OK;
}

extern "C" mdt_status mdt_op_multi_ema(const mdt_opt_tensor* tensors, int32_t n, float decay, void* stream) {
    if (!tensors || n < 0 || !(decay >= 0.f && decay <= 1.f)) return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_ema: bad argument");
    for (int i = 0; i < n; ++i)
        if (!tensors[i].p || !tensors[i].ema) return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_ema: tensor %d lacks p / ema", i);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 32) return fail(MDT_ERR_INVALID_ARG, "device index %d out of range", dev);
    OptTable& g_opt = g_opt_dev[dev];
    std::lock_guard<std::mutex> lock(g_opt.mu);
    hipStream_t s = (hipStream_t)stream;
    const mdt_opt_tensor* tab; const int2* blocks; int nb;
    OptSlot* slot = nullptr;
    MDT_TRY(upload_opt_table(g_opt, tensors, n, &tab, &blocks, &nb, &slot, s));
    LAUNCH(mdt_launch_multi_axpby(tab, blocks, nb, decay, 1.0f - decay, s));
    HIP_TRY(hipEventRecord(slot->ev, s));
    slot->busy = true;
    slot->stream = s;
    return MDT_OK;
}

extern "C" int64_t mdt_op_multi_sumsq_scratch(const mdt_opt_tensor* tensors, int32_t n) {
    if (!tensors || n < 0) return 0;
    int64_t nb = 0;
    for (int i = 0; i < n; ++i)
        if (tensors[i].numel > 0) nb += (tensors[i].numel + 4095) / 4096;  // OPT_CHUNK of the kernels
    return 2 * nb;
}

extern "C" mdt_status mdt_op_multi_sumsq(const mdt_opt_tensor* tensors, int32_t n, int32_t which, float* out, float* partials,
                                         int64_t partials_numel, void* stream) {
    if (!tensors || n < 0 || !out || (which != 0 && which != 1) || partials_numel < 0)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_sumsq: bad argument");
    for (int i = 0; i < n; ++i)
        if (tensors[i].numel != 0 && !(which ? (const float*)tensors[i].p : tensors[i].g))  // an empty tensor has no storage
            return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_sumsq: tensor %d lacks %s", i, which ? "p" : "g");
    const int64_t need = mdt_op_multi_sumsq_scratch(tensors, n);
    if (partials && partials_numel < need)
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_sumsq: %lld floats of partials given, %lld needed", (long long)partials_numel,
                    (long long)need);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 32) return fail(MDT_ERR_INVALID_ARG, "device index %d out of range", dev);
    OptTable& g_opt = g_opt_dev[dev];
    std::lock_guard<std::mutex> lock(g_opt.mu);
    hipStream_t s = (hipStream_t)stream;
    const mdt_opt_tensor* tab; const int2* blocks; int nb;
    OptSlot* slot = nullptr;
    MDT_TRY(upload_opt_table(g_opt, tensors, n, &tab, &blocks, &nb, &slot, s));
    const bool own = partials == nullptr && need > 0;
    if (own) {
        if (!g_opt.partial_ev) HIP_TRY(hipEventCreateWithFlags(&g_opt.partial_ev, hipEventDisableTiming));
        if ((size_t)need > g_opt.partial_cap) {
            if (g_opt.partial_busy) HIP_TRY(hipEventSynchronize(g_opt.partial_ev));  // its last reader (long done in practice)
            if (g_opt.partial) HIP_TRY(mdt_dev_free(g_opt.partial));
            g_opt.partial = nullptr; g_opt.partial_cap = 0; g_opt.partial_busy = false;
            HIP_TRY(mdt_dev_malloc((void**)&g_opt.partial, (size_t)need * 2 * sizeof(float)));
            g_opt.partial_cap = (size_t)need * 2;
        }
        if (g_opt.partial_busy && g_opt.partial_stream != s) HIP_TRY(hipStreamWaitEvent(s, g_opt.partial_ev, 0));
        partials = g_opt.partial;
    }
    LAUNCH(mdt_launch_multi_sumsq(tab, blocks, nb, which, partials, out, s));
    HIP_TRY(hipEventRecord(slot->ev, s));
    slot->busy = true;
    slot->stream = s;
    if (own) {
        HIP_TRY(hipEventRecord(g_opt.partial_ev, s));
        g_opt.partial_busy = true;
        g_opt.partial_stream = s;
    }
    return MDT_OK;
}

extern "C" mdt_status mdt_op_multi_adamw_dev(const mdt_opt_tensor* tensors, int32_t n, float lr, float beta1, float beta2,
                                             float eps, float weight_decay, float* step, const float* grad_scale,
                                             const float* found_inf, const float* grad_sumsq, float max_norm, float* grad_norm,
                                             void* stream) {
    if (!tensors || n < 0 || !step || max_norm != max_norm || (max_norm > 0.f && !grad_sumsq))
        return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_adamw_dev: bad argument");
    for (int i = 0; i < n; ++i)
        if (!tensors[i].p || !tensors[i].g || !tensors[i].m || !tensors[i].v)
            return fail(MDT_ERR_INVALID_ARG, "mdt_op_multi_adamw_dev: tensor %d lacks p / g / m / v", i);
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 32) return fail(MDT_ERR_INVALID_ARG, "device index %d out of range", dev);
    OptTable& g_opt = g_opt_dev[dev];
    std::lock_guard<std::mutex> lock(g_opt.mu);
    hipStream_t s = (hipStream_t)stream;
    const mdt_opt_tensor* tab; const int2* blocks; int nb;
    OptSlot* slot = nullptr;
    MDT_TRY(upload_opt_table(g_opt, tensors, n, &tab, &blocks, &nb, &slot, s));
    float* ctl = (float*)((char*)slot->dev + slot->ctl_off);
    LAUNCH(mdt_launch_multi_adamw_dev(tab, blocks, nb, lr, beta1, beta2, eps, weight_decay, step, grad_scale, found_inf, grad_sumsq,
                                      max_norm, ctl, grad_norm, s));
    HIP_TRY(hipEventRecord(slot->ev, s));
    slot->busy = true;
    slot->stream = s;
    return MDT_OK;
}
