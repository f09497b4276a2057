// mdt_route.h -- which kernel a launch runs on, as pure functions of shapes, flags and a snapshot of the process switches.
// Plain C++17, host only: no HIP type, no atomics, no allocation -- a host compiler builds it alone (tests/c_client/route_table.cpp
// prints the table tests/test_route_table.py pins).  The launchers (mdt_kernels.hip, mdt_model.hip) fill the snapshot once per
// launch, ask the route, and hold one switch from the route to the instantiation; every threshold and shape rule of the forward
// products lives here once, with the comment that carries its measurement.  Its sibling mdt_route_train.h holds the training path's:
// the Linear backward's plan (slices, kernel, scratch layout), the training attention kernels and the row-wise kernels' forms.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "mdt_hip_ops.h"

// ---- the switch snapshot: the process switches (mdt_internal.h: g_mdt_sw) a route depends on, read once per launch ----
struct mdt_route_switches {
    int gemm_geometry = 0;   // mdt_op_set_gemm_geometry: 0 = the rules below, -1 = the split-K kernel wherever it applies, > 0 forced
    int attn_wide_min = -1;  // mdt_op_set_attn_wide_min: rows; 0 = never (and no k_attn_xattn either); < 0 = the default
    int mlp_fuse_min = -1;   // mdt_op_set_mlp_fuse_min: rows; 0 = never; < 0 = the default
    int mlp_split = 1;       // MDT_HIP_MLP_SPLIT / mdt_op_set_mlp_split, resolved: 0 = the fp32 launches everywhere
    int ws_split = 1;        // MDT_HIP_WS_SPLIT / mdt_op_set_ws_split, resolved
    int tn_split = 1;        // MDT_HIP_TN_SPLIT / mdt_op_set_tn_split, resolved (mdt_route_train.h: the weight gradients)
    int side_pending = 0;    // a side job (mdt_gemm_side_push) is queued on this host thread
};

// ---- constants of the rules ----
// the buffer of zeros that stands in for absent bias / rowvec / LayerNorm-bias vectors: 256 KiB, so N, K <= 65536
static constexpr int ZEROS_FLOATS = 65536;
// rows up to which k_gemm_smallm is used: one row tile; beyond it the tile-count rule in mdt_route_gemm decides, up to
// GEMM_SMALLM_ROWS rows (round 1 had 192 rows here, before the half-height tiles)
static constexpr int GEMM_SMALLM_MAX = 15, GEMM_SMALLM_ROWS = 512;
static constexpr int GEMM_MID_MAX = 1400;  // rows up to which the 16 x 64 tiled geometry is used
#define MDT_TALL_BK 32   // the tall body's (mdt_tall.h) k step: K % 32 == 0
// rows from which the split forms of the sampler's launches are used (768: B = 80 2.97 -> 2.89 ms per call, 96 3.08 -> 2.93,
// 120 3.54 -> 2.96, 128 3.42 -> 2.96; B = 64 loses, 2.44 -> 2.90)
inline int mdt_split_min_rows() { return 768; }
// "this launch reads the fp16 pair images": split forms enabled and enough rows.  Below the row count the images may be stale (a
// training state's optimizer steps refresh them only for the launches that read them: split_ready in mdt_model.hip), so every
// reader -- the image refresh, the fused MLP, k_attn_xattn's projection, the LayerNorm-prologue split product -- asks HERE.
inline bool mdt_route_reads_pair(const mdt_route_switches& sw, int64_t rows) { return sw.mlp_split != 0 && rows >= mdt_split_min_rows(); }

// prologue kinds and split schemes as the kernels' template arguments number them (mdt_tiles.h: PRO_*, mdt_device.h: MDT_SPLIT_*;
// mdt_kernels.hip asserts the values agree)
enum { MDT_ROUTE_PRO_PLAIN = 0, MDT_ROUTE_PRO_LN = 1, MDT_ROUTE_PRO_LN_MOD_BCAST = 2, MDT_ROUTE_PRO_LN_MOD_ROWS = 3 };
enum { MDT_ROUTE_SCH_BF16X3 = 1, MDT_ROUTE_SCH_F16X2 = 2 };
// the prologue kind a product's arguments ask for
inline int mdt_route_pro(const mdt_gemm_args& a) {
    return !a.ln ? MDT_ROUTE_PRO_PLAIN
                 : (a.mod != nullptr && a.shift_off >= 0) ? (a.mod_stride == 0 ? MDT_ROUTE_PRO_LN_MOD_BCAST : MDT_ROUTE_PRO_LN_MOD_ROWS)
                                                          : MDT_ROUTE_PRO_LN;
}

// activation chunk length: whole K when it fits (always for the LayerNorm prologue), else the largest divisor of K
// that is a multiple of 16 and <= cap (cap 768 = 97 KiB of LDS for the one-workgroup-per-CU wide tiles, else 384)
inline int mdt_gemm_kchunk(int K, int ln, int cap) {
    if (ln || K <= 512) return K;
    for (int c = cap; c >= 16; c -= 16)
        if (K % c == 0) return c;
    return 16;
}

// ---- pure predicates ----
// WStream (mdt_tiles.h) addresses a weight image with 32-bit byte offsets from its base: every launcher that feeds one checks
// the image size (mdt_route_gemm does for the GEMMs; the fused MLP and attn_xattn tiles bound N and K by their shape rules)
inline bool w_image_ok(int64_t N, int64_t K) { return N * K < ((int64_t)1 << 30); }

// what mdt_gemm_side_push accepts as a side job: M <= 16 rows, the small-M kernel's own shape rules
inline bool smallm_shape_ok(const mdt_gemm_args& a) {
    return a.M >= 1 && a.M <= 15 && (!a.ln || a.K <= 512) && a.batch <= 1 && a.K <= 4096 && !a.aux_mode && a.a_parts <= 1 &&
           a.N <= ZEROS_FLOATS && a.K <= ZEROS_FLOATS && !(a.N & 15) && (int64_t)a.N * a.K < ((int64_t)1 << 30);
}

inline bool mdt_gemm_tall_supported(const mdt_gemm_args& a) {
    // (32-bit byte offsets from the operand bases: the activation block and the weight image each below 4 GiB)
    if ((int64_t)a.M * a.lda >= ((int64_t)1 << 30) || (int64_t)a.N * a.K >= ((int64_t)1 << 30)) return false;
    return !a.ln && a.a_parts <= 1 && a.batch <= 1 && a.K % MDT_TALL_BK == 0 && (a.N & 15) == 0 && a.M >= 1 && (a.lda & 3) == 0 &&
           (a.aux_mode == 0 || ((a.aux_mode == 1 || a.aux_mode == 2) && !a.residual));
}

// The weight-stationary body's fp32 form.  Workgroup = 8 waves x 2 column tiles (256-column panels), one per CU.  Measured and
// dropped (profiles/r05_ws_ab.txt): 4 waves x 2 tiles as two independent workgroups per CU (27.6 vs 27.5 ms per head step), 4 waves
// x 3 tiles for the N = 576 / 192 products (272 VGPRs: qkv 225 -> 215 us against the tall body, c_proj 81.6 -> 81.0 against the row
// tiles: not worth a shape).  Returns the wave count, 0 = no shape.
inline int ws_shape(const mdt_gemm_args& a) {
    if (a.K == 384) {
        // one column tile per wave: 128- (8 waves) or 192-column (12 waves) panels.  One round of one workgroup per CU either way;
        // what differs is how evenly the row tiles divide: cost ~ tiles per workgroup x waves (a SIMD's waves share its matrix pipe).
        // M = 10240: N = 384 -> 8 waves (3 panels x 80 chunks x 4 tiles), N = 1152 / 1536 -> 12 waves (6 x 40 x 8 / 8 x 32 x 10)
        const int ntiles = (a.M + 31) / 32;
        int best = 0, best_cost = 0;
        for (int nw : {12, 8}) {
            if (a.N % (nw * 16)) continue;
            const int panels = a.N / (nw * 16), groups = std::max(1, std::min(256 / (8 * panels), (ntiles + 7) / 8));
            if (8 * panels > 256) continue;
            const int tiles = (ntiles + 8 * groups - 1) / (8 * groups), cost = tiles * nw;
            if (!best || cost < best_cost) { best = nw; best_cost = cost; }
        }
        return best;
    }
    // 384-column panels, three waves per SIMD, 4 / 2 panels x 64 / 128 row chunks = 256 workgroups: the per-tile epilogue + barrier is
    // amortised over 18.4 k instead of 12.3 k clocks of MFMA issue and all 256 CUs work (SwishGLU forward 601 -> 544 us, plain 272 -> 248).
    // Not for the SwishGLU backward epilogue: at 168 VGPRs its u operands cannot be requested a tile ahead (348 -> 448 us)
    if (a.N % 384 == 0 && a.aux_mode != 4) return 12;
    return a.N % 256 == 0 ? 8 : 0;
}
// split form only: plain K = 192 products whose N is a multiple of 192 but not of 256 (the masked-image head's qkv and output
// projections, N = 576 / 192) -- twelve waves (three per SIMD) x one column tile.  (Their fp32 form was measured and dropped, above: no gain over the
// tall body; the split form is 1.4x.)
inline bool ws_split_192(const mdt_gemm_args& a, bool ws_split) {
    return ws_split && a.K == 192 && a.N % 192 == 0 && a.N % 256 != 0 && a.N / 192 <= 32 && a.aux_mode == 0 && a.act == MDT_ACT_NONE;
}
// ws_split: the three-way bf16 split of the weight-stationary body (mdt_ws.h) is on (mdt_route_switches.ws_split)
inline bool mdt_gemm_ws_supported(const mdt_gemm_args& a, bool ws_split) {
    const bool common = !a.ln && a.a_parts <= 1 && a.batch <= 1 && a.M >= 32 && (a.lda & 3) == 0 && (a.ldo & 3) == 0 && !a.residual &&
                        a.gin == 1 && a.gout == 1 && a.goff == 0 && a.rowvec == nullptr && (int64_t)a.N * a.K < ((int64_t)1 << 30);
    if (a.K == 384)   // plain rows, or an activation / the training hooks on the epilogue (GLU = 1 instantiation)
        return common && (a.aux_mode == 0 || ((a.aux_mode == 1 || a.aux_mode == 2) && a.aux != nullptr)) && ws_shape(a) != 0;
    const bool mode_ok = a.aux_mode == 0 || ((a.aux_mode == 3 || a.aux_mode == 4) && a.aux != nullptr);
    return common && a.K == 192 && (ws_shape(a) != 0 || ws_split_192(a, ws_split)) && a.act == MDT_ACT_NONE && mode_ok;
}

// ---- fused MLP sublayer (k_mlp) ----
inline bool mdt_mlp_supported(const mdt_gemm_args& f, const mdt_gemm_args& p) {
    const int D = f.K;
    return D >= 128 && D <= 512 && D % 128 == 0 && f.N == 4 * D && p.N == D && p.K == 4 * D && f.ln && f.batch <= 1 &&
           f.gin == 1 && f.gout == 1 && f.goff == 0 && f.rowvec == nullptr && !f.aux_mode && f.a_parts <= 1 && f.M >= 1 &&
           f.rows_per_sample >= 1 && p.rows_per_sample >= 1;
}
inline bool mdt_mlp_split_supported(const mdt_gemm_args& f, const mdt_gemm_args& p) { return mdt_mlp_supported(f, p); }
inline int mdt_mlp_slices(int D) { return 4 * D / 512; }

// which products take the LayerNorm-prologue split form: LayerNorm prologue over whole rows of K = 384 / 512, column count a
// multiple of the 384-wide panels, plain output rows
inline bool gemm_ln_split_shape(const mdt_gemm_args& a) {
    return a.ln && (a.K == 384 || a.K == 512) && a.N % 384 == 0 && a.M >= 1 &&
           a.batch <= 1 && !a.residual && a.gin == 1 && a.gout == 1 && a.goff == 0 && a.rowvec == nullptr && !a.aux_mode &&
           a.a_parts <= 4 && (a.lda & 3) == 0 && (a.ldo & 3) == 0;
}
// LDS bytes of gemm_ln_split_tile at model width D (mdt_mlp_split.h: gemm_ln_split_lds_bytes; mdt_kernels.hip asserts they agree)
constexpr size_t mdt_route_ln_split_lds(int D, int sch) {
    return (size_t)(sch == MDT_ROUTE_SCH_F16X2 ? 2 : 3) * 32 * (2 * D + 32) + (sch == MDT_ROUTE_SCH_F16X2 ? 128 : 0);
}

// ---- attention fused into its projection ----
// Self-attention of ONE sample fused into its output projection (k_attn_proj_smallm).  `p` is the projection's GEMM
// (A ignored: the attention output never reaches memory; M = the sample's T rows); q / k / v are the three column
// blocks of the (T, 3 K) qkv rows.  Supported: 8 heads of 16 / 32 / 48 / 64, T <= 16, no RoPE, plain output rows.
inline bool mdt_attn_proj_supported(const mdt_gemm_args& p, int H, int hd, int T, int rope) {
    return w_image_ok(p.N, p.K) && H == 8 && (hd == 16 || hd == 32 || hd == 48 || hd == 64) && p.K == H * hd && T >= 1 && T <= 16 && p.M >= T &&
           p.M % T == 0 && p.M / T <= 64 && (p.rows_per_sample == T || p.M == T) && !rope &&
           !(p.N & 15) && p.gin == 1 && p.gout == 1 && p.goff == 0 && !p.ln && p.act == MDT_ACT_NONE && p.rowvec == nullptr &&
           p.batch <= 1;
}
inline bool mdt_attn_proj_wide_supported(const mdt_gemm_args& p, int H, int hd, int T, int causal, int rope) {
    return w_image_ok(p.N, p.K) && H == 8 && (hd == 16 || hd == 32 || hd == 48) && p.K == H * hd && T >= 1 && T <= 16 && causal && !rope && p.residual &&
           p.M >= T && p.M % T == 0 && p.rows_per_sample == T && !(p.N & 15) && p.gin == 1 && p.gout == 1 && p.goff == 0 && !p.ln &&
           p.act == MDT_ACT_NONE && p.rowvec == nullptr && p.batch <= 1 && !p.aux_mode;
}
// which configurations the collapsed cross-attention covers (others keep the q GEMM + attention + c_proj GEMM sequence)
inline bool mdt_xattn_apply_supported(int D, int H, int Te, int Ta) {
    return D >= 128 && D <= 512 && D % 128 == 0 && (H == 4 || H == 8) && Te >= 1 && Te <= 4 && Ta >= 1 && Ta <= 16;
}
// Self-attention + projection + collapsed cross-attention of one sample per workgroup: `p` = the projection's arguments
// (as for mdt_launch_attn_proj_wide), `x` = the cross-attention's (x.y == p.out).  Head dimension 48 (d = 384).
inline bool mdt_attn_xattn_supported(const mdt_gemm_args& p, const mdt_xapply_args& x, int H, int hd, int T, int causal, int rope) {
    return mdt_attn_proj_wide_supported(p, H, hd, T, causal, rope) && hd == 48 && p.N == p.K && p.ldo == p.N && x.y == p.out &&
           x.D == p.N && x.H == H && H == 8 && x.Ta == T && (int64_t)x.B * T == p.M &&
           mdt_xattn_apply_supported(x.D, x.H, x.Te, x.Ta);
}
// Cross-attention + the Linear behind it in one launch (rollout batches): `x` as for mdt_launch_xattn_apply with a SEPARATE
// output array (x.y_out != x.y: the workgroups that repeat a sample's cross-attention read x.y while one of them writes), `g` =
// the Linear on the same rows (g.A == x.y, LayerNorm prologue, K = x.D, M = x.B * x.Ta, no residual, plain row mapping).
inline bool mdt_xattn_gemm_supported(const mdt_xapply_args& x, const mdt_gemm_args& g) {
    return w_image_ok(g.N, g.K) && mdt_xattn_apply_supported(x.D, x.H, x.Te, x.Ta) && x.y_out != nullptr && x.y_out != x.y && g.ln && g.K == x.D && g.A == x.y &&
           g.lda == x.D &&
           g.M == x.B * x.Ta && !(g.N & 15) && !g.residual && g.batch <= 1 && !g.aux_mode && g.a_parts <= 1 && g.gin == 1 &&
           g.gout == 1 && g.goff == 0 && g.rows_per_sample == x.Ta;
}

// ---- the GEMM route ----
enum mdt_gemm_body {
    MDT_GEMM_REFUSED = 0,
    MDT_GEMM_SMALLM,            // k_gemm_smallm: split-K, one workgroup per 16 columns and 16 rows
    MDT_GEMM_SMALLM_WITH_SIDE,  // k_gemm_smallm2: the same with a queued side job riding along
    MDT_GEMM_TILE,              // k_gemm<MTILES, NTW, NWAVES, PRO, RES>
    MDT_GEMM_PIPE,              // k_gemm_pipe<MTILES, NTW, NWAVES, LW, RES>: deep K, loader waves
    MDT_GEMM_GLU,               // k_gemm_glu<MTILES, NTW, NWAVES, GLU>: SwishGLU on the epilogue
    MDT_GEMM_MERGE,             // k_gemm_merge<NTW, PRO, XP>: rows = the sum of XP slabs
    MDT_GEMM_LN_SPLIT,          // k_gemm_ln_split<ND, NTW, PRO, XP, SCH>: the wide LayerNorm-prologue product in a split form
    MDT_GEMM_WS,                // k_gemm_ws<K16, NTW, NWAVES, GLU>: weight-stationary
    MDT_GEMM_WS_SPLIT,          // k_gemm_ws_split<K16, NTW, NWAVES, GLU>: the same as three-way bf16 splits
    MDT_GEMM_TALL,              // k_gemm_tall<2, 2, 2, 3, RES, 1>: 128 x 64 tiles, 4 + 1 waves, 3 stages (72 KiB: two per CU)
};
struct mdt_gemm_route {
    int body = MDT_GEMM_REFUSED;
    // the template integers that pick the instantiation (those the body's kernel has; the others stay 0)
    int mtiles = 0;   // 16-row tiles per workgroup (LN_SPLIT: ND = K / 128; WS / WS_SPLIT: K16 = K / 16)
    int ntw = 0;      // column tiles per wave
    int nwaves = 0;   // compute waves
    int lw = 0;       // loader waves
    int glu = 0;      // epilogue mode of the GLU / WS bodies
    int sch = 0;      // split scheme (MDT_ROUTE_SCH_*)
    int xp = 0;       // slabs summed on read
    int pro = 0;      // prologue kind (MDT_ROUTE_PRO_*), a function of the arguments alone
    bool res = false; // residual epilogue, a function of the arguments alone
    int kchunk = 0;   // activation chunk length
    int grid_n = 0;   // column tiles of the launch (WS bodies: panels)
    int tiles = 0;    // WS bodies: row tiles per workgroup
    unsigned gx = 0, gy = 1, gz = 1;   // SMALLM_WITH_SIDE: the product's own blocks; the launcher adds the rider's
    int threads = 0;
    size_t lds = 0;   // dynamic LDS bytes
};

namespace mdt_route_detail {
inline void tiled(mdt_gemm_route& r, const mdt_gemm_args& a, int body, int mtiles, int ntw, int nwaves, int lw, int kchunk) {
    const int MT = mtiles * 16, NTC = nwaves * ntw * 16;
    const int gn = (a.N + NTC - 1) / NTC, gm = (a.M + MT - 1) / MT;
    r.body = body; r.mtiles = mtiles; r.ntw = ntw; r.nwaves = nwaves; r.lw = lw; r.kchunk = kchunk; r.grid_n = gn;
    r.gx = (unsigned)(gn * gm);
    r.gz = body == MDT_GEMM_GLU ? 1u : (unsigned)(a.batch > 1 ? a.batch : 1);
    r.threads = 64 * (nwaves + lw);
    // (PIPE: double-buffered activation chunk)
    r.lds = (size_t)(body == MDT_GEMM_PIPE ? 2 : 1) * MT * (kchunk + 4) * sizeof(float);
}
// the LayerNorm-prologue split product in scheme sch: the caller has asked gemm_ln_split_shape
inline void ln_split(mdt_gemm_route& r, const mdt_gemm_args& a, int sch) {
    r.body = MDT_GEMM_LN_SPLIT; r.mtiles = a.K == 512 ? 4 : 3; r.ntw = 3; r.nwaves = 8; r.sch = sch;
    r.xp = a.a_parts >= 2 && a.a_parts <= 4 ? a.a_parts : 1;   // one array, or the sum of 2..4 slabs
    r.kchunk = a.K; r.grid_n = a.N / (8 * 3 * 16);
    r.gx = (unsigned)(r.grid_n * ((a.M + 31) / 32)); r.threads = 512; r.lds = mdt_route_ln_split_lds(128 * r.mtiles, sch);
}
// the weight-stationary bodies: the caller has asked mdt_gemm_ws_supported
inline void ws(mdt_gemm_route& r, const mdt_gemm_args& a, bool ws_split) {
    const int ntiles = (a.M + 31) / 32;
    auto split = [&](int k16, int ntw, int glu, int nw) {
        const int panels = a.N / (nw * ntw * 16);
        const int chunks = std::max(1, std::min(256 / panels, ntiles));
        r.body = MDT_GEMM_WS_SPLIT; r.mtiles = k16; r.ntw = ntw; r.nwaves = nw; r.glu = glu; r.sch = MDT_ROUTE_SCH_BF16X3;
        r.grid_n = panels; r.tiles = (ntiles + chunks - 1) / chunks;
        r.gx = 256; r.threads = 64 * nw; r.lds = (size_t)2 * 3 * 32 * (2 * k16 * 16 + 32);
    };
    auto fp32 = [&](int k16, int glu, int nw, int ntw) {
        const int panels = a.N / (nw * ntw * 16);
        // one round of one workgroup per CU: 8 x panels x groups blocks
        const int groups = std::max(1, std::min(256 / (8 * panels), (ntiles + 7) / 8));
        const int chunks = 8 * groups;
        r.body = MDT_GEMM_WS; r.mtiles = k16; r.ntw = ntw; r.nwaves = nw; r.glu = glu;
        r.grid_n = panels; r.tiles = (ntiles + chunks - 1) / chunks;
        r.gx = (unsigned)(chunks * panels); r.threads = 64 * nw; r.lds = (size_t)2 * 32 * (k16 * 16 + 4) * sizeof(float);
    };
    const int hooks = (a.aux_mode != 0 || a.act != MDT_ACT_NONE) ? 1 : 0;
    // the three-way bf16 split: K = 384, 128-column panels (8 waves, one column tile each); K = 192, 256-column panels
    if (ws_split && a.K == 384 && a.N % 128 == 0 && a.N / 128 <= 32) return split(24, 1, hooks, 8);
    if (ws_split && a.K == 192 && a.N % 256 == 0 && a.N / 256 <= 32 && a.act == MDT_ACT_NONE &&
        (a.aux_mode == 0 || a.aux_mode == 3 || a.aux_mode == 4))
        return split(12, 2, a.aux_mode, 8);
    if (ws_split_192(a, ws_split)) return split(12, 1, 0, 12);   // N = 192 / 576 ...: 192-column panels, twelve waves x one column tile
    const int nw = ws_shape(a) == 12 ? 12 : 8;
    if (a.K == 384) return fp32(24, hooks, nw, 1);
    return fp32(12, a.aux_mode, nw, 2);   // (K = 192: aux_mode 0, or a SwishGLU epilogue; the backward one never at twelve waves: ws_shape)
}
}  // namespace mdt_route_detail

inline mdt_gemm_route mdt_route_gemm(const mdt_gemm_args& a, const mdt_route_switches& sw) {
    using namespace mdt_route_detail;
    mdt_gemm_route r;
    r.pro = mdt_route_pro(a);
    r.res = a.residual != 0;
    const int force = sw.gemm_geometry;   // mdt_op_set_gemm_geometry
    const bool ws_split = sw.ws_split != 0;
    if (a.N > ZEROS_FLOATS || a.K > ZEROS_FLOATS) return r;
    // the weight stream is addressed with 32-bit byte offsets from the image's base (buffer loads, mdt_tiles.h: WStream)
    if (!w_image_ok(a.N, a.K)) return r;
    // the training hooks of the epilogue (aux) exist in the plain-prologue, non-residual tiled kernels only
    if (a.aux_mode && (!a.aux || a.ln || a.residual || a.batch > 1 || a.K > 512)) return r;
    // the weight-stationary body (mdt_ws.h), asked once: it takes what it supports from 8192 rows on (of the K = 192 products that
    // is aux_mode 0 / 3 / 4 only, so the SwishGLU epilogues reach it and the other training hooks do not) unless a geometry is forced
    const bool ws_ok = mdt_gemm_ws_supported(a, ws_split), ws_rows = a.M >= 8192 && force <= 0;
    if (a.aux_mode == 3 || a.aux_mode == 4) {  // SwishGLU on the epilogue: own kernels (4 waves; forward: pairs of column tiles per wave)
        if ((a.N & (a.aux_mode == 3 ? 31 : 15)) || a.gin != 1 || a.gout != 1 || a.goff != 0 || a.act != MDT_ACT_NONE) return r;
        // from 8192 rows on, K = 192: the weight-stationary body (mdt_ws.h) with the same epilogues -- round 5.  The masked-image
        // head's two SwishGLU products at B = 1024 (104448 rows).
        if (ws_ok && ws_rows) { ws(r, a, ws_split); return r; }
        const int kc = mdt_gemm_kchunk(a.K, 0, 384);
        if (a.aux_mode == 3) tiled(r, a, MDT_GEMM_GLU, 2, a.N % 256 == 0 ? 4 : 2, 4, 0, kc);
        else tiled(r, a, MDT_GEMM_GLU, 2, a.N % 192 == 0 ? 3 : 2, 4, 0, kc);
        r.glu = a.aux_mode;
        return r;
    }
    // the wide LayerNorm-prologue products in a split form (Wp_split: bf16 x 3, Wp_pair: fp16 x 2): the split image is there, the
    // shape fits, and enough rows that the wide tiles are the choice anyway (the fused MLP's threshold)
    if ((a.Wp_split != nullptr || a.Wp_pair != nullptr) && mdt_route_reads_pair(sw, a.M) && gemm_ln_split_shape(a) && force == 0) {
        // (the tile is written for any D <= 512 and 256-wide panels too; instantiated for the two shipped widths: MDT-V d = 384, MDT d = 512)
        // (Wp_split, where given, keeps its three-way bf16 form; the fp16 pair image otherwise)
        ln_split(r, a, a.Wp_split != nullptr ? MDT_ROUTE_SCH_BF16X3 : MDT_ROUTE_SCH_F16X2);
        return r;
    }
    if (a.a_parts > 1) {
        // a LayerNorm-prologue GEMM whose rows are the sum of a.a_parts slabs (2..4): wide tiles only
        if (!a.ln || a.K > 512 || a.residual || a.batch > 1 || a.aux_mode || a.a_parts > 4 || (a.N & 15)) return r;
        // 32 x 384 tiles when they divide N (qkv of d = 384: 1152), else 32 x 512
        tiled(r, a, MDT_GEMM_MERGE, 2, a.N % 384 == 0 ? 3 : 4, 8, 0, a.K);
        r.gz = 1; r.xp = a.a_parts;
        return r;
    }
    // (not for the batched split-K products of the weight gradients: few output rows there come with a DEEP reduction --
    // N = 192 layers of the masked-image decoder: 595 us as 16-column split-K tiles vs ~300 us tiled)
    // ... and beyond one row tile, the products whose half-height (16 x 64) tiling would leave most of the chip empty keep the
    // split-K kernel, which has 4x the workgroups: fewer than 60 tiles behind a LayerNorm prologue (every 16-column workgroup
    // repeats the row statistics), fewer than 100 / 160 (up to 192 / 512 rows) behind a plain one -- the two N = 384 residual
    // projections of a block at B = 12 ... 32.  Measured per sampler call (tools/latency.py, profiles/r04_lowbatch.txt):
    // B = 8 1.79 -> 1.69 ms, 10 2.06 -> 1.72, 16 2.43 -> 1.74, 19 2.93 -> 2.07, 24 2.36 -> 2.17, 32 2.39 -> 2.19.
    const int64_t tiles6 = (int64_t)((a.M + 15) / 16) * ((a.N + 63) / 64);
    const bool few_tiles = a.M <= GEMM_SMALLM_ROWS && tiles6 < (a.ln ? 60 : (a.M <= 192 ? 100 : 160));
    // (geometry hook -1: the split-K kernel wherever it applies -- tests that pin it against its fused variants)
    if ((a.M <= GEMM_SMALLM_MAX || few_tiles || force < 0) && force <= 0 && (!a.ln || a.K <= 512) && a.batch <= 1 && a.K <= 4096 && !a.aux_mode) {
        // a queued side job rides in this launch
        r.body = sw.side_pending && a.M <= 16 * 64 ? MDT_GEMM_SMALLM_WITH_SIDE : MDT_GEMM_SMALLM;
        r.kchunk = a.K; r.grid_n = a.N >> 4; r.threads = 512;
        if (r.body == MDT_GEMM_SMALLM) { r.gx = (unsigned)(a.N >> 4); r.gy = (unsigned)((a.M + 15) >> 4); }
        else r.gx = (unsigned)((a.N >> 4) * ((a.M + 15) >> 4));
        return r;
    }
    // Geometry selection (rows are in tiles of 32).  The decoder at B = 256 has 80 row tiles for 256 CUs:
    //   wide  (8 waves, 32 x 512 / 32 x 384): N >= 1024 -> 240 workgroups, each activation tile re-read 3x
    //   mid   (8 waves, 32 x 128)           : N  < 1024 -> 240 workgroups for N = 384
    //   small (4 waves, 32 x 64)            : few row tiles (small batches): more, smaller workgroups
    const int gm = (a.M + 31) / 32;
    // Pick the geometry with the best (wave fill) x (tile efficiency): workgroups run in waves of ~256 (one per CU), so
    // a count just above a multiple of 256 wastes most of its last wave (M = 10240, N = 384 on 32x384 tiles: 320
    // workgroups = 1.25 waves); wide tiles amortise the per-workgroup prologue / epilogue better than narrow ones.
    const int tile_n[5] = {0, 64, 128, 384, 512};
    const float eff[5] = {0.f, 0.85f, 0.92f, 1.0f, 1.0f};
    int geo = 1;
    float best = -1.f;
    for (int g = 4; g >= 1; --g) {
        const int cols = (a.N + tile_n[g] - 1) / tile_n[g];
        const int cnt = gm * cols;
        const float fill = (float)cnt / (float)(((cnt + 255) / 256) * 256);
        const float used = (float)a.N / (float)(cols * tile_n[g]);   // columns of the last tile that are real work
        const float score = fill * eff[g] * used;
        if (score > best) { best = score; geo = g; }
    }
    // deep K in several LDS chunks (mlp.c_proj and its kin, K = 4d) at large row counts: co-resident 4-wave 32 x 128
    // workgroups beat the 8-wave loader-wave kernel (tools/gemm_micro.py, N = 384, K = 1536: M = 10240 116 vs 131 us,
    // M = 5120 60 vs 66 us; at M = 2560 the loader-wave kernel still wins, 37.7 vs 42.5 us)
    if (geo == 2 && !a.ln && a.K > 512 && a.M >= 4096) geo = 5;
    // mid-size row counts (batches of ~20..140 chunks, and the training path's 384..1536-row dW products): half-height
    // tiles double the workgroup count; measured 4-17 % faster per sampler call up to M ~ 1400, slower beyond 2000
    // ... unless the output is so wide that they would be thousands (the stacked adaLN projection of a training batch:
    // 1024 x 9216 -> 9216 workgroups that each re-read their weight tile): then the scored choice stands
    if (a.M <= GEMM_MID_MAX && tiles6 <= 4096) {
        geo = 6;
        // ... except where 4-wave 32 x 192 tiles come out as (nearly) whole rounds of one workgroup per CU: the encoder's
        // and the B ~ 120..140 decoder's wide products (tools/gemm_shapes.py: 1024 x 1536 22.0 -> 18.3 us, 1024 x 3072 33.7 ->
        // 28.0, 1280 x 1152 21.6 -> 17.8; 1280 x 1536 -- 320 tiles -- 27.8 vs 28.5: stays; 1024 x 1152 -- 192 tiles -- wins
        // alone, 18.9 -> 17.5, and loses inside the encoder, 18.1 -> 19.5: stays)
        if (a.N % 192 == 0 && a.N >= 1152 && a.K <= 512 && a.batch <= 1) {
            const int cnt9 = gm * (a.N / 192);
            if ((float)cnt9 / (float)(((cnt9 + 255) / 256) * 256) >= 0.9f) geo = 9;
        }
    }
    // training-sized row counts without a LayerNorm prologue (forward / input-gradient products of a B = 1024 step, the
    // masked-image head's 104 k rows): 4 waves x 32 x 192 tiles -- two or three co-resident per CU, each weight fragment reused by
    // one wave only -- beat every 8-wave geometry whenever N is a multiple of 192 (tools/gemm_train_shapes.py: 10240 x 1536 x 384
    // 126 -> 107 us, 104448 x 192 x 768 372 -> 282 us, 104448 x 576 x 192 332 -> 233 us); N = 384 keeps the choices above
    // (36.5 vs 38.4 us at K = 384, the co-resident 32 x 128 tiles at K = 1536)
    if (!a.ln && a.M >= 4096 && a.N % 192 == 0 && a.N != 384 && a.batch <= 1) geo = 9;
    // ... and from 8192 rows on the TALL body (mdt_tall.h: 128-row tiles, both operands staged in LDS by LDS-DMA, each staged
    // element used by 2-4 waves) where the column count is a multiple of its 64-wide tiles: the forward / input-gradient
    // products of a B = 1024 training step and the masked-image head's 104 k rows (tools/gemm_train_shapes.py,
    // profiles/r04_gemm_train_shapes.txt: 104448 x 576 x 192 249 -> 213-231 us, 104448 x 192 x 768 290 -> 263-270,
    // 10240 x 384 x 1536 124 -> 105-112, 10240 x 1152 x 384 94 -> 88-92; 10240 x 384 x 384 unchanged, 4096 rows lose)
    // ... and the K = 192 products among them whose column count is a multiple of 256 on the weight-stationary body (mdt_ws.h)
    if (a.M >= 8192 && a.N % 64 == 0 && (a.N > 384 || a.K > 384) && a.batch <= 1 && mdt_gemm_tall_supported(a)) geo = 23;
    if (a.batch > 1) geo = 5;  // split-K partial products (deep reductions): geometry chosen for those
    if (force > 0) geo = force;
    // ... the weight-stationary body first, by the row rule or forced (geometry 30: tests pin it against the other bodies)
    if (ws_ok && (ws_rows || geo == 30)) { ws(r, a, ws_split); return r; }
    if (geo >= 10 && (geo != 23 || !mdt_gemm_tall_supported(a))) geo = 0;  // (forced geometry on a product the tall body does not take)
    switch (geo) {
        // the tall body (mdt_tall.h): 128-row tiles, operands by LDS-DMA, ONE loader wave issuing every DMA request of the workgroup.
        // (Round 4 also carried 128 x 128 / 128 x 64 / 128 x 96 tiles without the loader wave -- geometries 10 / 12 / 16 -- which no
        //  dispatcher rule reached after tools/gemm_train_shapes.py had measured them: pruned in round 5.)
        case 23: {  // 4 + 1 waves 128 x 64, 3 stages (72 KiB: two per CU)
            constexpr int WM = 2, WN = 2, NT = 2, NS = 3, LW = 1, BM = WM * 64, BN = WN * NT * 16;
            r.body = MDT_GEMM_TALL; r.mtiles = WM; r.ntw = NT; r.nwaves = WM * WN; r.lw = LW; r.kchunk = MDT_TALL_BK;
            r.grid_n = (a.N + BN - 1) / BN;
            r.gx = (unsigned)(r.grid_n * ((a.M + BM - 1) / BM)); r.threads = 64 * (WM * WN + LW);
            r.lds = (size_t)NS * (BM + BN) * MDT_TALL_BK * sizeof(float);
            return r;
        }
        case 1: tiled(r, a, MDT_GEMM_TILE, 2, 1, 4, 0, mdt_gemm_kchunk(a.K, a.ln, 384)); return r;
        case 2:
            // multi-chunk K: loader waves double-buffer the activation chunk
            if (!a.ln && a.K > 512) tiled(r, a, MDT_GEMM_PIPE, 2, 1, 8, 4, mdt_gemm_kchunk(a.K, 0, 384));
            else tiled(r, a, MDT_GEMM_TILE, 2, 1, 8, 0, mdt_gemm_kchunk(a.K, a.ln, 768));
            return r;
        case 3: tiled(r, a, MDT_GEMM_TILE, 2, 3, 8, 0, mdt_gemm_kchunk(a.K, a.ln, 768)); return r;
        case 4: tiled(r, a, MDT_GEMM_TILE, 2, 4, 8, 0, mdt_gemm_kchunk(a.K, a.ln, 768)); return r;
        case 6:
            // 4 waves 16 x 64.  Deep K (the encoder's / a mid batch's c_proj, K = 4d in four LDS chunks): with two LOADER waves that
            // double-buffer the activation chunk -- as a single-buffer loop each chunk was a memory round trip of its own in front of
            // its 24 k-steps, and half-height tiles have few workgroups per CU to hide it
            // (up to one workgroup per CU: beyond that the co-resident workgroups hide each other's round trips -- the encoder's
            //  1024-row c_proj, 384 workgroups, measured +0.1 % with the loader waves)
            if (!a.ln && a.K > 512 && !a.aux_mode && tiles6 <= 256) tiled(r, a, MDT_GEMM_PIPE, 1, 1, 4, 2, mdt_gemm_kchunk(a.K, 0, 384));
            else tiled(r, a, MDT_GEMM_TILE, 1, 1, 4, 0, mdt_gemm_kchunk(a.K, a.ln, 384));
            return r;
        case 7: tiled(r, a, MDT_GEMM_TILE, 4, 2, 4, 0, mdt_gemm_kchunk(a.K, a.ln, 384)); return r;  // 4 waves 64 x 128 (deep-K products)
        case 8: tiled(r, a, MDT_GEMM_TILE, 2, 4, 4, 0, mdt_gemm_kchunk(a.K, a.ln, 384)); return r;  // 4 waves 32 x 256: two workgroups per CU
        case 9: tiled(r, a, MDT_GEMM_TILE, 2, 3, 4, 0, mdt_gemm_kchunk(a.K, a.ln, 384)); return r;  // 4 waves 32 x 192
        default: tiled(r, a, MDT_GEMM_TILE, 2, 2, 4, 0, mdt_gemm_kchunk(a.K, a.ln, 384)); return r;  // 4 waves 32 x 128
    }
}

// ---- the blocks' routes (mdt_model.hip: run_self_attn, run_mlp, run_decoder_blocks, run_eval) ----
// largest batch whose self-attention runs fused into the projection (measured crossover)
// (round 2, B = 2 / 4 / 8: 1.87 -> 1.71, 2.02 -> 1.85, 2.24 -> 2.07 ms; B = 16 lost then, 2.76 -> 2.83.  Round 5, with the fused
//  kernel's attention on the MFMA pipe, its rows requested in one batch and its LDS cut to the T real rows -- two workgroups
//  per CU: B = 12 / 16 / 20 / 24 / 32 1.653 / 1.649 / 1.918 / 2.006 / 2.017 -> 1.49 / 1.50 / 1.74 / 1.93 / 1.95 ms; B = 48 loses,
//  2.30 -> 2.42)
static constexpr int64_t ATTN_PROJ_MAX_BATCH = 32;
// row count from which the self-attention runs in the prologue of its output projection
inline int mdt_attn_wide_min_rows(const mdt_route_switches& sw) {
    const int v = sw.attn_wide_min;
    return v >= 0 ? (v == 0 ? 1 << 30 : v) : 1401;
}
// row count from which (and batch up to which: two rounds of one workgroup per CU) one workgroup per sample runs self-attention,
// projection AND the collapsed cross-attention (k_attn_xattn); mdt_op_set_attn_wide_min(0) switches it off too
inline int mdt_attn_xattn_min_rows(const mdt_route_switches& sw) {
    // (round 3 started it where the fused MLP launch starts, 1401 rows; measured down the batch sizes in round 4 -- tools/latency.py,
    //  profiles/r04_lowbatch.txt -- it beats k_attn + projection + k_xattn_apply from 200 rows on: B = 20 2.03 -> 1.99 ms, 32 2.13 -> 2.09,
    //  40 2.48 -> 2.35, 80 3.12 -> 3.03, 100 3.26 -> 3.17, 128 3.62 -> 3.52, 140 4.33 -> 4.14; at 160 rows it loses, 1.71 -> 1.75)
    return sw.attn_wide_min == 0 ? 1 << 30 : 200;
}
static constexpr int64_t ATTN_XATTN_MAX_BATCH = 512;

enum mdt_attn_form {
    MDT_ATTN_PROJ_SMALL,  // k_attn_proj_smallm: rollout batch, attention and projection in one launch
    MDT_ATTN_XATTN,       // k_attn_xattn: one workgroup per sample through attention, projection and the collapsed cross-attention
    MDT_ATTN_PROJ_WIDE,   // k_attn_proj_wide: the causal attention of each 32-row tile in the projection's prologue
    MDT_ATTN_PLAIN,       // k_attn, then the projection as a GEMM of its own
};
struct mdt_attn_route {
    int form = MDT_ATTN_PLAIN;
    bool pair = false;   // ATTN_XATTN: the projection on its fp16 pair image
};
// `p`: the projection's arguments (M = B * T rows); fx: the collapsed cross-attention that follows on the same rows, or nullptr;
// has_pair: the projection's fp16 pair image exists
inline mdt_attn_route mdt_route_self_attn(const mdt_gemm_args& p, int64_t B, int T, int H, int hd, int causal, int rope,
                                          const mdt_xapply_args* fx, bool has_pair, const mdt_route_switches& sw) {
    mdt_attn_route r;
    const int M = p.M, D = p.N;
    if (B <= ATTN_PROJ_MAX_BATCH && mdt_attn_proj_supported(p, H, hd, T, rope)) { r.form = MDT_ATTN_PROJ_SMALL; return r; }
    if (fx && M >= mdt_attn_xattn_min_rows(sw) && B <= ATTN_XATTN_MAX_BATCH && mdt_attn_xattn_supported(p, *fx, H, hd, T, causal, rope)) {
        r.form = MDT_ATTN_XATTN;
        r.pair = has_pair && mdt_route_reads_pair(sw, M);
        return r;
    }
    // (up to one workgroup per CU: its 156 KB of LDS allow no second one, so beyond 256 tiles -- B > 272 -- the workgroups
    //  queue up behind each other while the plain projection keeps three per CU in flight: B = 512 10.35 vs 10.13 ms)
    const int64_t wide_tiles = (int64_t)((M + 31) / 32) * ((D + 127) / 128);
    if (M >= mdt_attn_wide_min_rows(sw) && (wide_tiles <= 256 || sw.attn_wide_min > 0) && mdt_attn_proj_wide_supported(p, H, hd, T, causal, rope))
        r.form = MDT_ATTN_PROJ_WIDE;
    return r;
}

// row count from which the MLP sublayer runs as ONE launch (k_mlp) that leaves partial slabs instead of the residual
// stream: below it the wide tiles do not fill the chip
// (`pair`: the launch would run in its split form (fp16 pairs, mdt_mlp_split.h), which pays from fewer rows -- mdt_split_min_rows(), B = 128: 1280 rows
// per call 3.42 -> 2.96 ms with the qkv products split too; a setting made with the hook is taken as it is)
inline int mdt_mlp_fuse_min_rows(const mdt_route_switches& sw, bool pair) {
    const int v = sw.mlp_fuse_min;
    if (v >= 0) return v == 0 ? 1 << 30 : v;
    return pair ? mdt_split_min_rows() : 1401;
}
enum mdt_mlp_form {
    MDT_MLP_FUSED_PAIR,   // k_mlp_split on the fp16 pair images: one launch, slabs out
    MDT_MLP_FUSED_F32,    // k_mlp: one launch, slabs out
    MDT_MLP_XATTN_IN_FC,  // k_xattn_gemm_smallm (the collapsed cross-attention inside c_fc), then c_proj
    MDT_MLP_TWO_GEMMS,    // c_fc and c_proj as two GEMMs
};
// f / p: c_fc's and c_proj's arguments; slabs_ok: the caller can hand slabs to the next reader; x_in_fc: the cross-attention is
// still to run on these rows (mdt_route_x_in_fc said so -- never fused then: the caller skipped its own cross-attention launch
// because the c_fc launch was to run it); has_pair: both pair images exist
inline int mdt_route_mlp(const mdt_gemm_args& f, const mdt_gemm_args& p, bool slabs_ok, bool x_in_fc, bool has_pair,
                         const mdt_route_switches& sw) {
    // the fp16 pair split form of the launch (mdt_mlp_split.h) wherever its images exist and it is not switched off; it pays
    // from fewer rows than the fp32 launch
    const bool pair = has_pair && mdt_route_reads_pair(sw, f.M) && mdt_mlp_split_supported(f, p);
    if (slabs_ok && !x_in_fc && f.M >= mdt_mlp_fuse_min_rows(sw, pair) && mdt_mlp_slices(f.K) >= 2 && mdt_mlp_supported(f, p))
        return pair ? MDT_MLP_FUSED_PAIR : MDT_MLP_FUSED_F32;
    return x_in_fc ? MDT_MLP_XATTN_IN_FC : MDT_MLP_TWO_GEMMS;
}

// batch up to which the cross-attention of a decoder block runs inside the c_fc launch that follows it (rollout batches;
// B = 4: 1.67 vs 1.58 ms per call) -- if that launch is the small-M kernel, and over an even number of blocks (the residual stream
// trades places with the attention buffer once per block)
static constexpr int64_t XATTN_FC_MAX_BATCH = 2;
inline bool mdt_route_x_in_fc(int64_t B, int blocks, const mdt_xapply_args& x, const mdt_gemm_args& fc) {
    return B <= XATTN_FC_MAX_BATCH && fc.M <= 192 && blocks % 2 == 0 && mdt_xattn_gemm_supported(x, fc);
}
// the one-launch head (linear output, HP = 0 hidden units; action vectors of at most 8) adds the last MLP's slabs itself
inline bool mdt_route_head_sums(int HP, int A) { return HP == 0 && A <= 8; }
// hand-offs to the kernels of the long shapes: action vectors of 17 .. 64 elements (mdt_head_wide.hip), chunks / contexts of
// 17 .. 64 rows (mdt_attn_chunk.hip)
inline bool mdt_route_head_wide(int A) { return A > 16; }
inline bool mdt_route_attn_chunk(int Tq, int Tk) { return std::max(Tq, Tk) > 16; }

// ---- a route as text: the kernel's name with its template integers as a kernel trace prints them, then grid, threads and LDS
// bytes.  For tests and tools; launch paths do not call it.  Returns what snprintf returns.
inline int mdt_route_text(const mdt_gemm_route& r, char* buf, size_t cap) {
    char k[96];
    const char* res = r.res ? "true" : "false";
    switch (r.body) {
        case MDT_GEMM_SMALLM: snprintf(k, sizeof k, "k_gemm_smallm"); break;
        case MDT_GEMM_SMALLM_WITH_SIDE: snprintf(k, sizeof k, "k_gemm_smallm2"); break;
        case MDT_GEMM_TILE: snprintf(k, sizeof k, "k_gemm<%d, %d, %d, %d, %s>", r.mtiles, r.ntw, r.nwaves, r.pro, res); break;
        case MDT_GEMM_PIPE: snprintf(k, sizeof k, "k_gemm_pipe<%d, %d, %d, %d, %s>", r.mtiles, r.ntw, r.nwaves, r.lw, res); break;
        case MDT_GEMM_GLU: snprintf(k, sizeof k, "k_gemm_glu<%d, %d, %d, %d>", r.mtiles, r.ntw, r.nwaves, r.glu); break;
        case MDT_GEMM_MERGE: snprintf(k, sizeof k, "k_gemm_merge<%d, %d, %d>", r.ntw, r.pro, r.xp); break;
        case MDT_GEMM_LN_SPLIT: snprintf(k, sizeof k, "k_gemm_ln_split<%d, %d, %d, %d, %d>", r.mtiles, r.ntw, r.pro, r.xp, r.sch); break;
        case MDT_GEMM_WS: snprintf(k, sizeof k, "k_gemm_ws<%d, %d, %d, %d>", r.mtiles, r.ntw, r.nwaves, r.glu); break;
        case MDT_GEMM_WS_SPLIT: snprintf(k, sizeof k, "k_gemm_ws_split<%d, %d, %d, %d>", r.mtiles, r.ntw, r.nwaves, r.glu); break;
        case MDT_GEMM_TALL: snprintf(k, sizeof k, "k_gemm_tall<2, 2, %d, 3, %s, %d>", r.ntw, res, r.lw); break;
        default: return snprintf(buf, cap, "REFUSED");
    }
    return snprintf(buf, cap, "%s grid=(%u,%u,%u) threads=%d lds=%zu", k, r.gx, r.gy, r.gz, r.threads, r.lds);
}
inline const char* mdt_attn_form_name(int form) {
    switch (form) {
        case MDT_ATTN_PROJ_SMALL: return "ATTN_PROJ_SMALL";
        case MDT_ATTN_XATTN: return "ATTN_XATTN";
        case MDT_ATTN_PROJ_WIDE: return "ATTN_PROJ_WIDE";
        default: return "ATTN_PLAIN";
    }
}
inline const char* mdt_mlp_form_name(int form) {
    switch (form) {
        case MDT_MLP_FUSED_PAIR: return "MLP_FUSED_PAIR";
        case MDT_MLP_FUSED_F32: return "MLP_FUSED_F32";
        case MDT_MLP_XATTN_IN_FC: return "MLP_XATTN_IN_FC";
        default: return "MLP_TWO_GEMMS";
    }
}
