// mdt_route_train.h -- the training path's sibling of mdt_route.h: how a weight gradient is sliced and what scratch that takes,
// which attention kernel a training launch runs on, and the forms of the row-wise kernels, as pure functions of shapes, flags and
// the switch snapshot.  The same rules: plain C++17, host only, no HIP type, no allocation -- a host compiler builds it alone
// (tests/c_client/route_table.cpp prints the table tests/test_route_table.py pins and sweeps the plan's invariants).  The launchers
// (mdt_train_ops.hip, mdt_train_kernels.hip, mdt_attn_chunk.hip) ask the route and execute it; the scratch sizes are read off the
// same plan the launch runs, so the two cannot drift apart.
#pragma once
#include "mdt_route.h"
#include "mdt_hip_train.h"

// ================================================================================================
// 1. the Linear backward:  dW (N, K) = dY^T X,  dbias = colsum(dY)
// ================================================================================================
// Split of the row reduction of dW = dY^T X into S parallel slices of L rows (multiples of 32), so that the product fills the chip
// however small N x K is: slice s multiplies its own rows in ONE batched launch (grid.z = S), and the S partial (N, K) products are
// summed in a fixed order by a column sum -- deterministic, unlike atomics.
static constexpr int64_t TN_SPLIT_MIN_ROWS = 8192;   // rows from which the wide n-tiles and the bf16 split kernel are used
static constexpr int64_t TN_SLICE_MIN_ROWS = 128;    // least slice depth of k_gemm_tn: small batches (B = 128: 1280 rows) need the split even more than large ones
// workgroups (in units of 64-column tiles) aimed for.  Measured at B = 1024: round 2, everything in one stream: 768 -> 11.27 ms step /
// 42.1 ms head, 1536 -> 11.18 / 41.4, 2304 -> 11.22 / 41.4; round 6, the weight gradients beside the chain on a side stream:
// 1536 -> 9.34, 768 -> 9.25, 512 -> 9.23 (fewer, deeper slices: less partial-sum traffic beside the chain)
static constexpr int64_t TN_TARGET = 512;
static constexpr int64_t TN_SLICE_CAP = 128;   // measured: masked-image head 37.7 ms (64) -> 37.2 (128) = (192, 256); denoiser step unchanged
static constexpr int64_t TN_ROUND = 256;       // one round of one-per-CU workgroups (the 192-wide fp32 tile, the bf16 split kernel)
// whole rounds of resident workgroups are taken where that is within this factor of the target's slice count
static constexpr int64_t TN_ROUNDS_NUM = 3, TN_ROUNDS_DEN = 2;

enum mdt_dw_path {
    MDT_DW_NONE = 0,   // no weight gradient asked for
    MDT_DW_TN,         // k_gemm_tn<KT, WN>: straight from the row-major operands, fp32 MFMA
    MDT_DW_TN_SPLIT,   // k_gemm_tn_split<KTW, TNW>: the same as three-way bf16 splits of both operands
    MDT_DW_COPY,       // a row stride that is no multiple of 4 floats: transposed copies, a packed image, the batched forward GEMM
};
struct mdt_linear_bwd_plan {
    int path = MDT_DW_NONE;
    int S = 0, L = 0;            // slices of the row reduction and their length (a multiple of 32; S L >= M)
    int tn = 0, tk = 0;          // the (n, k) tile of the k_gemm_tn kernels
    int t0 = 0, t1 = 0;          // their template integers: <KT, WN> / <KTW, TNW>
    unsigned gx = 0, gz = 1;     // grid (gx, 1, gz = S)
    int threads = 0;
    size_t lds = 0;              // dynamic LDS bytes
    bool bias_from_partials = false;   // the dW path leaves the bias gradient's partial column sums too (else: a column sum of dY)
    // offsets, in floats, of the regions carved from `scratch`, and the floats needed in all
    int64_t dYt = 0, Xt = 0;     // COPY: [S][N][L] transposed dY; [S] packed (N' = K, K' = L) images of X^T
    int64_t parts = 0;           // [S][N][K] partial products (written when S > 1)
    int64_t bpart = 0;           // TN paths: [S][N] per-slice column sums of dY; COPY: (ceil(M / 32), N) column partials
    int64_t total = 0;
};

namespace mdt_route_detail {
inline int64_t slice_len(int64_t M, int64_t s) { return ((M + s - 1) / s + 31) / 32 * 32; }   // equal slices: at most 31 pad rows each
inline void slices(mdt_linear_bwd_plan& p, int64_t M, int64_t s) {
    const int64_t l = slice_len(M, s);
    p.S = (int)((M + l - 1) / l);
    p.L = (int)l;
}
}  // namespace mdt_route_detail

// k-tile width for a K-column product: the one that pads K less (128 on a tie)
inline int mdt_tn_ktile(int K) { return (K + 191) / 192 * 192 < (K + 127) / 128 * 128 ? 192 : 128; }

// k_gemm_tn's (n, k) tile for an M-deep product.  n-tile: 192 wide (12 waves, needs N and K multiples of 192: every Linear of this
// model) from 8192 reduction rows on for matrices of at least 576 x 192, else 128 wide where N is a multiple of 128, else 64;
// k-tile: 192 with the 192-wide n-tile, else the one that pads K less.
inline void mdt_route_tn_tile(int64_t M, int N, int K, int* tn, int* tk) {
    const bool ok192 = N % 192 == 0 && K % 192 == 0, ok128 = N % 128 == 0;
    // measured, product + sum of its slices (tools/dw_bench.py, us at 64 / 128 / 192): M = 104448: 1536 x 192 712 / 689 / 628,
    // 192 x 768 357 / - / 307, 576 x 192 288 / - / 285, 192 x 192 115 / - / 139;  M = 10240: 1536 x 384 137 / 130 / 130,
    // 384 x 1536 134 / 128 / 128, 1152 x 384 108 / 98 / 108, 384 x 384 51 / 48 / 63;  M = 4096: 64 wide or a tie
    // (192 wide with ONE round of workgroups, below: 1536 x 192 597, 192 x 768 280, 576 x 192 263)
    // M = 10240 with that slicing: 1536 x 384 119, 384 x 1536 118, 1152 x 384 97, 384 x 384 45 -- 192 wide everywhere it fits
    const int w = ok192 && M >= TN_SPLIT_MIN_ROWS && (int64_t)N * K >= 576 * 192 ? 192 : (ok128 && M >= TN_SPLIT_MIN_ROWS ? 128 : 64);
    *tn = w;
    *tk = w == 192 ? 192 : mdt_tn_ktile(K);
}
// k_gemm_tn_split's tile (128 x 128 / 128 x 192 / 192 x 128; 8 / 8 / 6 waves, 123 / 154 / 154 KB of LDS): (n, k) = 192 x 128 where
// 128-wide n-tiles would pad N by more than an eighth and 192-wide ones do not (N = 192, 576 ...), else 128 x (192 where that pads
// K less, else 128)
inline void mdt_route_tn_split_tile(int N, int K, int* tn, int* tk) {
    const bool n192 = 8 * ((N + 127) / 128 * 128) > 9 * N && 8 * ((N + 191) / 192 * 192) <= 9 * N;
    *tn = n192 ? 192 : 128;
    *tk = n192 ? 128 : mdt_tn_ktile(K);
}

// the slices of k_gemm_tn (64 x 128 tiles and wider, no transposed / packed copies to amortise): ~6 workgroups per CU queued (3 resident)
inline int64_t mdt_route_tn_slices(int64_t M, int64_t N, int64_t K, int tn, int tk) {
    // in units of 64-column tiles whatever the n-tile: a 128- / 192-wide workgroup counts two / three times (it has as many waves)
    const int64_t tiles = ((N + 63) / 64) * ((K + tk - 1) / tk);
    int64_t s = std::max<int64_t>(1, std::min<int64_t>((TN_TARGET + tiles - 1) / tiles, M / TN_SLICE_MIN_ROWS));
    if (tn == 192) {
        // twelve-wave workgroups, one per CU: ONE round of them (tools/dw_bench.py at M = 104448, us at 32 / 64 / 128 slices:
        // 1536 x 192 (8 tiles) 597 / 624 / 616, 192 x 768 (4) 495 / 280 / 302, 576 x 192 (3) 483 / 263 / 281)
        const int64_t tiles192 = (N / 192) * (K / 192);
        s = std::max<int64_t>(1, std::min<int64_t>((TN_ROUND + tiles192 / 2) / tiles192, M / TN_SLICE_MIN_ROWS));
    }
    s = std::min<int64_t>(s, TN_SLICE_CAP);
    if (tn != 192) {
        // whole rounds of workgroups here too where that is within a factor 1.5 of the above (192 x 192 at M = 104448, three
        // 64 x 192 tiles: 128 slices = 384 workgroups 118 us, 170 = 510 of the 512 that are resident at once 99 us, 256 108 us)
        const int64_t tiles_wg = ((N + tn - 1) / tn) * ((K + tk - 1) / tk);
        const int64_t slots = TN_ROUND * (tn == 64 ? (tk == 192 ? 2 : 3) : (tk == 192 ? 1 : 2));   // resident workgroups: LDS 51 / 68 / 68 / 84 KB
        const int64_t rounds = std::max<int64_t>(1, (tiles_wg * s + slots / 2) / slots);
        const int64_t s2 = std::min<int64_t>((rounds * slots) / tiles_wg, M / TN_SLICE_MIN_ROWS);
        if (s2 >= 1 && TN_ROUNDS_DEN * s2 <= TN_ROUNDS_NUM * s && TN_ROUNDS_NUM * s2 >= TN_ROUNDS_DEN * s) s = s2;
    }
    return s;
}
// the slices of the transposed-copy path (32 x 128 tiles of the forward GEMM): only worth it for deep reductions
inline int64_t mdt_route_copy_slices(int64_t M, int64_t N, int64_t K) {
    const int64_t tiles = ((N + 31) / 32) * ((K + 127) / 128);   // 32 x 128 tiles of one product
    constexpr int64_t target = 1000, min_depth = 512;  // workgroups aimed for, least slice depth
    // measured (B = 1024 step): aiming for ~1000 workgroups of >= 512-deep slices instead of 400
    // of >= 1024 is 11 % faster per step (several 4-wave workgroups share a CU); reductions under 4096 rows (B = 128:
    // 1280 rows) were 2.6 % slower when cut in two, so they keep the 1024-row floor
    const int64_t depth = M >= 4096 ? min_depth : std::max<int64_t>(min_depth, 1024);
    int64_t s = std::max<int64_t>(1, std::min<int64_t>((target + tiles - 1) / tiles, M / depth));
    s = std::min<int64_t>(s, 32);
    while (mdt_route_detail::slice_len(M, s) > 16384) ++s;   // keeps the GEMM's K' well inside its limit
    return s;
}

// the launch of k_gemm_tn<KT, WN> / k_gemm_tn_split<KTW, TNW> on S slices: tile, template integers, grid, threads, LDS
inline void mdt_route_gemm_tn(mdt_linear_bwd_plan& p, int64_t M, int N, int K, int S) {
    mdt_route_tn_tile(M, N, K, &p.tn, &p.tk);
    p.path = MDT_DW_TN; p.t0 = p.tk / 64; p.t1 = p.tn / 64;
    p.gx = (unsigned)(((N + p.tn - 1) / p.tn) * ((K + p.tk - 1) / p.tk)); p.gz = (unsigned)S;
    p.threads = 256 * p.t1;
    p.lds = (size_t)2 * 32 * ((p.tn + 4) + (p.tk + 4)) * sizeof(float);
}
inline void mdt_route_gemm_tn_split(mdt_linear_bwd_plan& p, int N, int K, int S) {
    mdt_route_tn_split_tile(N, K, &p.tn, &p.tk);
    const int tnw = p.tn / 64, nwv = tnw == 2 ? 8 : 6;
    p.path = MDT_DW_TN_SPLIT; p.t0 = p.tk / (16 * (nwv / tnw)); p.t1 = tnw;
    p.gx = (unsigned)(((N + p.tn - 1) / p.tn) * ((K + p.tk - 1) / p.tk)); p.gz = (unsigned)S;
    p.threads = 64 * nwv;
    p.lds = (size_t)2 * 3 * (p.tn + p.tk) * 80;
}

// The plan of one Linear backward's weight / bias gradient.  strides_aligned: ldx and ldy are multiples of 4 floats.  The caller
// has checked the shape (M, N, K >= 1, K % 16 == 0, N % 16 == 0 with a weight gradient).
inline mdt_linear_bwd_plan mdt_route_linear_bwd(int64_t M, int64_t N, int64_t K, bool strides_aligned, bool want_dW, bool want_dbias,
                                                const mdt_route_switches& sw) {
    using namespace mdt_route_detail;
    mdt_linear_bwd_plan p;
    if (!want_dW) return p;
    // the bias gradient rides on the dW path: per-slice column sums of dY from k_gemm_tn, per-32-row partials from the transpose
    p.bias_from_partials = want_dbias;
    if (strides_aligned) {
        // dW straight from dY and X: S slices of the row reduction as one batched launch, partial products and the bias
        // gradient's per-slice column sums added up in a fixed order afterwards
        int tn, tk;
        mdt_route_tn_tile(M, (int)N, (int)K, &tn, &tk);
        int64_t s = mdt_route_tn_slices(M, N, K, tn, tk);
        slices(p, M, s);
        // from 8192 rows on: the bf16 split kernel, ONE round of its one-per-CU workgroups (never more slices than the fp32 tiling
        // takes: the scratch bound is that tiling's)
        // ... where its n-tiles pad N by at most an eighth (tools/dw_bench.py, us fp32 / split: 12288 x 1536 x 384 127 / 101,
        // x 384 x 1536 128 / 100, x 1152 x 384 105 / 80, x 384 x 384 47 / 36; 104448 x 1536 x 192 598 / 510, x 576 x 192 217 / 185;
        // N = 192 on 128-wide n-tiles -- a quarter of its second tile empty -- loses: x 192 x 768 286 / 311, x 192 x 1536 507 / 590;
        // mdt_route_tn_split_tile gives such an N the 192 x 128 tile, which pads nothing, so the test below passes for it)
        int stn, stk;
        mdt_route_tn_split_tile((int)N, (int)K, &stn, &stk);
        if (M >= TN_SPLIT_MIN_ROWS && sw.tn_split != 0 && 8 * ((N + stn - 1) / stn * stn) <= 9 * N) {
            const int64_t tiles = ((N + stn - 1) / stn) * ((K + stk - 1) / stk);
            s = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(TN_ROUND / tiles, p.S), M / 256));   // never a second round
            slices(p, M, s);
            mdt_route_gemm_tn_split(p, (int)N, (int)K, p.S);
        } else {
            mdt_route_gemm_tn(p, M, (int)N, (int)K, p.S);
        }
        p.parts = 0;
        p.bpart = (int64_t)p.S * N * K;
        p.total = p.bpart + (int64_t)p.S * N + 64;
        return p;
    }
    p.path = MDT_DW_COPY;
    slices(p, M, mdt_route_copy_slices(M, N, K));
    const int64_t Mp = (int64_t)p.S * p.L;
    p.dYt = 0;
    p.Xt = N * Mp;
    p.parts = p.Xt + K * Mp;
    p.bpart = p.parts + (int64_t)p.S * N * K;
    p.total = p.bpart + N * (Mp / 32 + 2);
    return p;
}

// Floats of scratch ONE product of exactly M rows needs: the larger of the two plans' totals, aligned strides (the fp32 tiling,
// which never has fewer slices than the split form -- so the figure does not move with the switch) and not.
inline int64_t mdt_route_linear_bwd_scratch_exact(int64_t M, int64_t N, int64_t K) {
    mdt_route_switches fp32;
    fp32.tn_split = 0;
    return std::max(mdt_route_linear_bwd(M, N, K, false, true, true, fp32).total, mdt_route_linear_bwd(M, N, K, true, true, true, fp32).total);
}

// Floats of scratch that serve EVERY row count up to M.  The callers size their scratch once, for the largest batch seen, and
// reuse it for every smaller one -- and the slice count is not monotone in M (the n-tile changes at 8192 rows, the 192-wide tile
// wants one round of workgroups, the narrower ones whole rounds of the resident workgroups: a smaller batch can be cut into MORE
// slices than the capacity batch), so the exact figure at M is not enough.  Closed-form bounds of both paths:
//   k_gemm_tn: S <= M / 128 always; S <= 3/2 x min(ceil(target / tiles), cap) for the 64- / 128-wide tiles (`tiles` counted with
//              the k-tile that gives fewer of them), S <= (256 + t / 2) / t one-round slices for the 192-wide one;
//   transposed-copy path (odd shapes): its slice count s only grows with M and Mp = S L <= M + 32 s.
// tests/test_cpu_abi.py sweeps the exact need of every row count below a capacity against this bound, and so does route_table.cpp.
inline int64_t mdt_route_linear_bwd_scratch(int64_t M, int64_t N, int64_t K) {
    if (M < 1) M = 1;
    // k_gemm_tn.  The target is deliberately looser than the plan's TN_TARGET (512): it is the largest the plan has ever aimed
    // for, and the allocations it sizes must not shrink
    constexpr int64_t target = 1536;
    const int64_t tiles_min = ((N + 63) / 64) * ((K + 191) / 192);
    int64_t s_tn = (TN_ROUNDS_NUM * std::min<int64_t>((target + tiles_min - 1) / tiles_min, TN_SLICE_CAP) + 1) / TN_ROUNDS_DEN;
    if (N % 192 == 0 && K % 192 == 0) {
        const int64_t t192 = (N / 192) * (K / 192);
        s_tn = std::max<int64_t>(s_tn, (TN_ROUND + t192 / 2) / t192);
    }
    s_tn = std::max<int64_t>(1, std::min<int64_t>(s_tn, M / TN_SLICE_MIN_ROWS));
    const int64_t need_tn = s_tn * N * K + s_tn * N + 64;
    // transposed-copy path: its slice count before it is rounded to whole slices -- non-decreasing in M
    mdt_route_switches fp32;
    fp32.tn_split = 0;
    const int S = mdt_route_linear_bwd(M, N, K, false, true, true, fp32).S;
    int64_t s_old = std::max<int64_t>(S, std::min<int64_t>(32, std::max<int64_t>(1, M / 512)));
    while ((M + s_old - 1) / s_old > 16384) ++s_old;
    const int64_t Mp = M + 32 * s_old;
    const int64_t need_old = (N + K) * Mp + s_old * N * K + N * (Mp / 32 + 2);
    return std::max(std::max(need_tn, need_old), mdt_route_linear_bwd_scratch_exact(M, N, K));
}

// ================================================================================================
// 2. training attention (forward with dropout, backward)
// ================================================================================================
static constexpr int MDT_ATTN_CHUNK_T = 64;   // largest Tq / Tk of the chunk kernels (mdt_attn_chunk.hip)
static constexpr size_t MDT_LDS_MAX = 160 * 1024;   // bytes of LDS a workgroup can have on gfx950

// kv_rows a launch may stage: every key (0 or Tk), or a causal launch's prefix that holds every key some query sees -- key j is
// seen by the queries i >= j only, so j < min(Tq, Tk) -- at Tk > 16 (the 16-row kernels have no such form)
inline bool mdt_prefix_rows_ok(int Tq, int Tk, int causal, int kv_rows) {
    return kv_rows == 0 || kv_rows == Tk || (causal && Tk > 16 && kv_rows >= (Tq < Tk ? Tq : Tk) && kv_rows < Tk);
}
inline bool mdt_attn_chunk_supported(int hd, int Tq, int Tk) {
    return (hd == 32 || hd == 48 || hd == 64) && Tq >= 1 && Tk >= 1 && Tq <= MDT_ATTN_CHUNK_T && Tk <= MDT_ATTN_CHUNK_T;
}
// bytes of dynamic LDS of the chunk forward (q, k, V^T) or backward (q, k, v, dO and the two Tq16 x Tv16 matrices); Tv: the keys
// the launch stages -- Tk, or the visible prefix
inline size_t mdt_attn_chunk_lds(int hd, int Tq, int Tv, bool bwd) {
    const size_t Tq16 = (size_t)((Tq + 15) & ~15), Tv16 = (size_t)((Tv + 15) & ~15), st = (size_t)hd + 4;
    if (bwd) return ((2 * Tq16 + 2 * Tv16) * st + 2 * Tq16 * (Tv16 + 4)) * sizeof(float);
    return ((Tq16 + Tv16) * st + (size_t)hd * (Tv16 + 4)) * sizeof(float);
}
// which (hd, H) the MFMA kernels take, as the heads one workgroup runs (0: the one-wave-per-head kernels)
inline int mdt_attn_train_mfma_group(int hd, int H, int rope) {
    if (rope || (hd != 16 && hd != 32 && hd != 48 && hd != 64)) return 0;
    return H % 4 == 0 ? 4 : (H % 2 == 0 ? 2 : 1);
}

enum mdt_attn_train_family {
    MDT_ATTN_TRAIN_REFUSED = 0,
    MDT_ATTN_TRAIN_CHUNK,   // k_attn_chunk_fwd / _bwd<HD, DROP>: 17 .. 64 rows
    MDT_ATTN_TRAIN_MFMA,    // k_attn_fwd_train_mfma / k_attn_bwd_mfma<HD, HG>: HG heads per workgroup
    MDT_ATTN_TRAIN_WAVE,    // k_attn_fwd_train / k_attn_bwd<HD>: one wave per (sample, head) -- RoPE
};
struct mdt_attn_train_route {
    int family = MDT_ATTN_TRAIN_REFUSED;
    bool bwd = false;
    int hd = 0;         // template <HD, ...>
    int hg = 0;         // MFMA: heads per workgroup
    bool drop = false;  // CHUNK: the dropout instantiation
    int Tv = 0;         // CHUNK: keys staged
    unsigned gy = 0;    // grid (B, gy)
    int threads = 0;
    size_t lds = 0;     // dynamic LDS bytes
};
inline mdt_attn_train_route mdt_route_attn_train(int hd, int H, int Tq, int Tk, int causal, int rope, int kv_rows, bool dropout_on, bool bwd) {
    mdt_attn_train_route r;
    r.bwd = bwd; r.hd = hd;
    if (Tq > 16 || Tk > 16) {   // 17 .. 64 rows: mdt_attn_chunk.hip
        const int Tv = kv_rows > 0 ? kv_rows : Tk;   // keys staged: kv_rows = 0 means every key
        if (!mdt_attn_chunk_supported(hd, Tq, Tk) || H < 1 || H > 65535 || !mdt_prefix_rows_ok(Tq, Tk, causal, Tv)) return r;
        r.lds = mdt_attn_chunk_lds(hd, Tq, Tv, bwd);
        if (r.lds > MDT_LDS_MAX) return r;
        r.family = MDT_ATTN_TRAIN_CHUNK; r.drop = dropout_on; r.Tv = Tv; r.gy = (unsigned)H; r.threads = 256;
        return r;
    }
    if (kv_rows != 0 && kv_rows != Tk) return r;   // the visible prefix is a form of the chunk kernels
    if (Tq < 1 || Tk < 1) return r;
    if (rope && hd < 32) return r;
    if (const int hg = mdt_attn_train_mfma_group(hd, H, rope)) {
        const size_t rs = (size_t)hg * hd + 16;   // AttnMfma<HD, HG>::RS
        r.family = MDT_ATTN_TRAIN_MFMA; r.hg = hg; r.gy = (unsigned)(H / hg); r.threads = 64 * hg;
        r.lds = bwd ? ((size_t)(2 * Tq + 2 * Tk) * rs + (size_t)hg * (16 * 17 + 2 * 16 * 20)) * sizeof(float)
                    : ((size_t)(Tq + 2 * Tk) * rs + (size_t)hg * 16 * 17) * sizeof(float);
        return r;
    }
    if (hd != 16 && hd != 32 && hd != 48 && hd != 64) return r;
    r.family = MDT_ATTN_TRAIN_WAVE; r.gy = (unsigned)H; r.threads = 64;
    return r;
}
// the operand checks of the two launchers, whatever the family: 16-byte loads / stores of the head slices, RoPE with its tables
inline bool mdt_attn_train_operands_ok(const mdt_attn_train_args& a) {
    return !((a.ldq | a.ldkv | a.ldo) & 3) && !(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out) & 15) &&
           (!a.rope || (a.rope_cos && a.rope_sin));
}
inline bool mdt_attn_train_operands_ok(const mdt_attn_bwd_args& a) {
    return !((a.ldq | a.ld_do | a.ldkv | a.ld_dq | a.ld_dkv) & 3) &&
           !(((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.d_out | (uintptr_t)a.dq | (uintptr_t)a.dk | (uintptr_t)a.dv) & 15) &&
           (!a.rope || (a.rope_cos && a.rope_sin));
}
// the model's attention forward in a training step: the training kernel when dropout is live or its MFMA form applies, else the
// inference kernel (mdt_launch_attention)
inline bool mdt_route_attn_fwd_is_train(int hd, int H, int rope, bool dropout_on) {
    return dropout_on || mdt_attn_train_mfma_group(hd, H, rope) != 0;
}

// ================================================================================================
// 3. the row-wise kernels
// ================================================================================================
static constexpr int MDT_LN_MAX_D = 512;   // a LayerNorm row is held in registers: 64 lanes x 8 (LN_MAXC)
namespace mdt_route_detail {
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
}
// 16-byte accesses: the *4 kernels
inline bool mdt_ln_fwd_vec_ok(const mdt_ln_train_args& a) {
    using mdt_route_detail::al16;
    return a.D % 4 == 0 && al16(a.x) && al16(a.w) && al16(a.b) && al16(a.out) &&
           (!a.mod || (al16(a.mod) && a.mod_stride % 4 == 0 && (a.shift_off < 0 || a.shift_off % 4 == 0) &&
                       (a.scale_off < 0 || a.scale_off % 4 == 0)));
}
inline bool mdt_ln_bwd_vec_ok(const mdt_ln_bwd_args& a) {
    using mdt_route_detail::al16;
    return a.D % 4 == 0 && a.ld_dh % 4 == 0 && al16(a.x) && al16(a.dh) && al16(a.dx) && al16(a.w) && al16(a.b) &&
           (!a.mod || (al16(a.mod) && a.mod_stride % 4 == 0 && (a.scale_off < 0 || a.scale_off % 4 == 0)));
}
inline bool mdt_merge_vec_ok(const mdt_merge_args& a, bool bwd) {
    using mdt_route_detail::al16;
    return a.D % 4 == 0 && a.D >= 4 && a.D <= 1024 && al16(a.x) && al16(a.a) && al16(a.out) &&
           (!a.gate || (al16(a.gate) && a.gate_stride % 4 == 0)) && (!bwd || !a.dgate || (al16(a.dgate) && a.dgate_stride % 4 == 0));
}
enum mdt_rowwise_form {
    MDT_ROW_REFUSED = 0,
    MDT_ROW_SCALAR,        // the 4-byte kernel
    MDT_ROW_VEC4,          // the 16-byte kernel
    MDT_ROW_FUSED,         // merge + LayerNorm forward / LayerNorm + merge backward in one launch (both 16-byte)
    MDT_ROW_TWO_LAUNCHES,  // ... as the two kernels one after the other
};
inline int mdt_route_ln_fwd(const mdt_ln_train_args& a) {
    if (a.D > MDT_LN_MAX_D || a.D < 1) return MDT_ROW_REFUSED;
    return mdt_ln_fwd_vec_ok(a) ? MDT_ROW_VEC4 : MDT_ROW_SCALAR;
}
// the merge g, then the LayerNorm l of its result (l.x == g.out): one launch where both take 16-byte accesses
inline int mdt_route_merge_ln_fwd(const mdt_merge_args& g, const mdt_ln_train_args& l) {
    if (l.D > MDT_LN_MAX_D || l.D < 1) return MDT_ROW_REFUSED;
    return mdt_ln_fwd_vec_ok(l) && mdt_merge_vec_ok(g, false) && g.D == l.D && (int64_t)g.B * g.rows_per_sample == l.M && g.out != g.a
               ? MDT_ROW_FUSED : MDT_ROW_TWO_LAUNCHES;
}
struct mdt_ln_bwd_route {
    int form = MDT_ROW_REFUSED;
    int chunks = 1;   // workgroups per sample: grid (B, chunks), 256 threads
    int rb = 0;       // VEC4 / FUSED: rows a wave keeps in flight -- all of them, up to 3 (k_ln_bwd4<MG, RB>)
    size_t lds = 0;   // dynamic LDS bytes
};
// LayerNorm backward; g: the merge backward on the gradient it leaves (g.x == a.dx), or nullptr.  One launch for both where both
// take 16-byte accesses and a sample is one workgroup.
inline mdt_ln_bwd_route mdt_route_ln_bwd(const mdt_ln_bwd_args& a, const mdt_merge_args* g) {
    mdt_ln_bwd_route r;
    if (a.D > MDT_LN_MAX_D || a.D < 1 || a.rows_per_sample < 1) return r;
    r.chunks = a.row_chunks > 1 ? a.row_chunks : 1;
    const bool fused = g && r.chunks == 1 && mdt_ln_bwd_vec_ok(a) && mdt_merge_vec_ok(*g, true) && g->B == a.B &&
                       g->rows_per_sample == a.rows_per_sample && g->D == a.D;
    if (g && !fused) { r.form = MDT_ROW_TWO_LAUNCHES; return r; }
    if (r.chunks > 1 && (a.d_mod || r.chunks > a.rows_per_sample)) { r.form = MDT_ROW_REFUSED; return r; }
    if (!mdt_ln_bwd_vec_ok(a)) { r.form = MDT_ROW_SCALAR; r.lds = (size_t)16 * a.D * sizeof(float); return r; }
    const int per = (a.rows_per_sample + r.chunks - 1) / r.chunks;
    r.form = fused ? MDT_ROW_FUSED : MDT_ROW_VEC4;
    r.rb = per <= 4 ? 1 : (per <= 8 ? 2 : 3);
    r.lds = (size_t)4 * (fused ? 5 : 4) * a.D * sizeof(float);
    return r;
}

// column sums out[n] (+)= sum_m X[m][n]
static constexpr int MDT_COLSUM_SLICES = 64, MDT_COLSUM_MAXN = 4096;   // the sliced form's scratch: 64 row slices x 4096 columns per stream
static constexpr int MDT_COLSUM_DEEP_ROWS = 512;   // rows from which a sum is cut into slices (63 -> 2 x 9 us at M = 1024, N = 384)
enum mdt_colsum_form {
    MDT_COLSUM_PLAIN,    // k_colsum: one stage on N / 64 workgroups
    MDT_COLSUM_SLICED,   // k_colsum twice: 64 row slices in parallel, then their sum
    MDT_COLSUM_WIDE4,    // k_colsum_wide4: very many columns (the S slices of a weight gradient), 16-byte column groups
};
// aligned16: X and out are 16-byte aligned
inline int mdt_route_colsum(int64_t ldx, int M, int N, bool aligned16) {
    if (N >= 16384 && N % 4 == 0 && ldx % 4 == 0 && aligned16) return MDT_COLSUM_WIDE4;
    return M >= MDT_COLSUM_DEEP_ROWS && N <= MDT_COLSUM_MAXN ? MDT_COLSUM_SLICED : MDT_COLSUM_PLAIN;
}
// the narrow linears around the action tokens (k_narrow_out, k_narrow_dw): 16-column tiles of the wide form (17 <= A <= 64), 0 = the A <= 16 form
inline int mdt_route_narrow_tiles(int A) { return A > 16 ? (A + 15) / 16 : 0; }

// ================================================================================================
// the routes as text (tests and tools; launch paths do not call these)
// ================================================================================================
inline int mdt_route_text(const mdt_linear_bwd_plan& p, char* buf, size_t cap) {
    const char* path = p.path == MDT_DW_TN ? "tn" : p.path == MDT_DW_TN_SPLIT ? "tn_split" : p.path == MDT_DW_COPY ? "copy" : "none";
    if (p.path == MDT_DW_NONE) return snprintf(buf, cap, "none");
    if (p.path == MDT_DW_COPY)
        return snprintf(buf, cap, "copy S=%d L=%d scratch=%lld (dYt=%lld Xt=%lld parts=%lld bpart=%lld)", p.S, p.L, (long long)p.total,
                        (long long)p.dYt, (long long)p.Xt, (long long)p.parts, (long long)p.bpart);
    return snprintf(buf, cap, "%s %s<%d, %d> grid=(%u,1,%u) threads=%d lds=%zu S=%d L=%d scratch=%lld", path,
                    p.path == MDT_DW_TN ? "k_gemm_tn" : "k_gemm_tn_split", p.t0, p.t1, p.gx, p.gz, p.threads, p.lds, p.S, p.L, (long long)p.total);
}
inline int mdt_route_text(const mdt_attn_train_route& r, char* buf, size_t cap) {
    switch (r.family) {
        case MDT_ATTN_TRAIN_CHUNK:
            return snprintf(buf, cap, "%s<%d, %s> grid=(B,%u) threads=%d lds=%zu Tv=%d", r.bwd ? "k_attn_chunk_bwd" : "k_attn_chunk_fwd", r.hd,
                            r.drop ? "true" : "false", r.gy, r.threads, r.lds, r.Tv);
        case MDT_ATTN_TRAIN_MFMA:
            return snprintf(buf, cap, "%s<%d, %d> grid=(B,%u) threads=%d lds=%zu", r.bwd ? "k_attn_bwd_mfma" : "k_attn_fwd_train_mfma", r.hd, r.hg,
                            r.gy, r.threads, r.lds);
        case MDT_ATTN_TRAIN_WAVE:
            return snprintf(buf, cap, "%s<%d> grid=(B,%u) threads=%d lds=%zu", r.bwd ? "k_attn_bwd" : "k_attn_fwd_train", r.hd, r.gy, r.threads, r.lds);
        default: return snprintf(buf, cap, "REFUSED");
    }
}
inline const char* mdt_rowwise_form_name(int form) {
    switch (form) {
        case MDT_ROW_SCALAR: return "SCALAR";
        case MDT_ROW_VEC4: return "VEC4";
        case MDT_ROW_FUSED: return "FUSED";
        case MDT_ROW_TWO_LAUNCHES: return "TWO_LAUNCHES";
        default: return "REFUSED";
    }
}
inline const char* mdt_colsum_form_name(int form) {
    return form == MDT_COLSUM_WIDE4 ? "k_colsum_wide4" : form == MDT_COLSUM_SLICED ? "k_colsum x2 (64 slices)" : "k_colsum";
}
