// route_table.cpp -- which kernel a shape takes, one line per case, from the host-only route functions of
// mdt_policy_amd/csrc/mdt_route.h and mdt_route_train.h.  Stand-alone: no GPU, no library; tests/test_route_table.py builds it with
// the sanitizers and compares its lines with route_table.expected beside it.
//   route_table           the table:       <key>: <route>, then one `invariants: OK` line (or the first violation) of a sweep of
//                         the Linear backward's plan
//   route_table --cases   the cases as numbers, for a driver that issues them on a GPU and compares a kernel trace:
//                         <key> M N K ln residual aux_mode a_parts batch image geometry mlp_split ws_split side
//                         (image: 0 none, 1 Wp_pair, 2 Wp_split)
//                         lin_bwd/<key> M N K aligned tn_split
//                         attn_train/<key> hd H Tq Tk causal rope kv_rows dropout bwd
// Each pair of GEMM cases straddles one rule of mdt_route_gemm.  N x K = 384 x 384 unless the key says otherwise.
// The deep/ lines (table only) are whole training steps at the batches of tests/deep_row_configs.py.
#include <stdio.h>
#include <string.h>

#include "mdt_route_train.h"

static bool g_cases = false;
static const float* const SOME = (const float*)16;   // a non-null operand: routes look at pointers only to see whether they are there

struct GemmCase {
    const char* key;
    int M, N = 384, K = 384, ln = 0, residual = 0, aux_mode = 0, a_parts = 0, batch = 0, image = 0;
    mdt_route_switches sw;
};
static GemmCase gc(const char* key, int M, int N = 384, int K = 384) {
    GemmCase c;
    c.key = key; c.M = M; c.N = N; c.K = K;
    return c;
}
static GemmCase with_ln(GemmCase c) { c.ln = 1; return c; }
static GemmCase with_res(GemmCase c) { c.residual = 1; return c; }
static GemmCase with_aux(GemmCase c, int mode) { c.aux_mode = mode; return c; }
static GemmCase with_parts(GemmCase c, int n) { c.ln = 1; c.a_parts = n; return c; }
static GemmCase with_pair(GemmCase c) { c.ln = 1; c.image = 1; return c; }
static GemmCase with_geo(GemmCase c, int g) { c.sw.gemm_geometry = g; return c; }
static GemmCase no_mlp_split(GemmCase c) { c.sw.mlp_split = 0; return c; }
static GemmCase no_ws_split(GemmCase c) { c.sw.ws_split = 0; return c; }

static mdt_gemm_args args_of(const GemmCase& c) {
    mdt_gemm_args a;
    memset(&a, 0, sizeof a);
    a.A = SOME; a.Wp = SOME; a.out = (float*)SOME;
    a.M = c.M; a.N = c.N; a.K = c.K; a.lda = c.K;
    a.ldo = c.aux_mode == 4 ? 2 * c.N : c.N;
    a.shift_off = a.scale_off = a.gate_off = -1;
    a.rows_per_sample = 1; a.gin = a.gout = 1;
    a.ln = c.ln; a.ln_w = c.ln ? SOME : nullptr;
    a.residual = c.residual;
    a.aux_mode = c.aux_mode; a.aux = c.aux_mode ? SOME : nullptr;
    a.a_parts = c.a_parts; a.a_part_stride = (int64_t)c.M * c.K;
    a.batch = c.batch;
    if (c.image == 1) a.Wp_pair = SOME;
    if (c.image == 2) a.Wp_split = SOME;
    return a;
}
static void gemm(const GemmCase& c) {
    if (g_cases) {
        printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d\n", c.key, c.M, c.N, c.K, c.ln, c.residual, c.aux_mode, c.a_parts, c.batch, c.image,
               c.sw.gemm_geometry, c.sw.mlp_split, c.sw.ws_split, c.sw.side_pending);
        return;
    }
    char text[160];
    mdt_route_text(mdt_route_gemm(args_of(c), c.sw), text, sizeof text);
    printf("gemm/%s: %s\n", c.key, text);
}

// A block of the model: d = H * hd, Ta action rows, Te context rows, the collapsed cross-attention, an even decoder depth
struct BlockCase {
    const char* tag = "";
    int B = 1, H = 8, hd = 48, Ta = 10, Te = 4, rope = 0, A = 7, depth = 4;
    bool fold = true;   // the cross-attention is the collapsed one (mdt_xapply_args); false: q GEMM + attention + c_proj GEMM
    mdt_route_switches sw;
};
static void block(const BlockCase& c) {
    if (g_cases) return;
    const int D = c.H * c.hd;
    float y[1], att[1];   // two distinct residual-stream addresses
    auto proj = [&](int T) {
        mdt_gemm_args p;
        memset(&p, 0, sizeof p);
        p.A = att; p.Wp = SOME; p.out = y; p.lda = p.ldo = D; p.M = c.B * T; p.N = p.K = D;
        p.shift_off = p.scale_off = p.gate_off = -1; p.gin = p.gout = 1;
        p.residual = 1; p.rows_per_sample = T;
        return p;
    };
    mdt_xapply_args x;
    memset(&x, 0, sizeof x);
    x.y = y; x.B = c.B; x.H = c.H; x.D = D; x.Te = c.Te; x.Ta = c.Ta; x.y_out = att;
    mdt_gemm_args fc;
    memset(&fc, 0, sizeof fc);
    fc.A = y; fc.Wp = SOME; fc.lda = D; fc.ldo = 4 * D; fc.M = c.B * c.Ta; fc.N = 4 * D; fc.K = D; fc.ln = 1;
    fc.shift_off = fc.scale_off = fc.gate_off = -1; fc.gin = fc.gout = 1; fc.rows_per_sample = c.Ta; fc.act = MDT_ACT_GELU;
    mdt_gemm_args pj = proj(c.Ta);
    pj.N = D; pj.K = 4 * D; pj.lda = 4 * D;
    const bool x_in_fc = c.fold && mdt_route_x_in_fc(c.B, c.depth, x, fc);
    x.y_out = nullptr;   // (as the decoder leaves it for the attention route)
    const mdt_attn_route dec = mdt_route_self_attn(proj(c.Ta), c.B, c.Ta, c.H, c.hd, 1, c.rope, c.fold ? &x : nullptr, true, c.sw);
    const mdt_attn_route enc = mdt_route_self_attn(proj(c.Te), c.B, c.Te, c.H, c.hd, 0, c.rope, nullptr, false, c.sw);
    printf("block/B%d%s: dec_attn=%s%s enc_attn=%s mlp=%s mlp_no_out=%s x_in_fc=%d head_sums=%d head_wide=%d attn_chunk=%d\n", c.B, c.tag,
           mdt_attn_form_name(dec.form), dec.pair ? "+pair" : "", mdt_attn_form_name(enc.form),
           mdt_mlp_form_name(mdt_route_mlp(fc, pj, true, x_in_fc, true, c.sw)), mdt_mlp_form_name(mdt_route_mlp(fc, pj, false, x_in_fc, true, c.sw)),
           (int)x_in_fc, (int)mdt_route_head_sums(0, c.A), (int)mdt_route_head_wide(c.A), (int)mdt_route_attn_chunk(c.Ta, c.Te));
}

// ---- the training path (mdt_route_train.h) ----
// One Linear backward with dW and dbias.  aligned = 0: a row stride that is no multiple of 4 floats (the transposed-copy path, whose
// product is the batched forward GEMM: its route is printed behind the plan).
static void lin_bwd(int M, int N, int K, bool aligned = true, bool tn_split = true) {
    char key[64];
    snprintf(key, sizeof key, "lin_bwd/%dx%dx%d%s%s", M, N, K, aligned ? "" : "_unaligned", tn_split ? "" : "_tn_split0");
    if (g_cases) {
        printf("%s %d %d %d %d %d\n", key, M, N, K, (int)aligned, (int)tn_split);
        return;
    }
    mdt_route_switches sw;
    sw.tn_split = tn_split;
    const mdt_linear_bwd_plan p = mdt_route_linear_bwd(M, N, K, aligned, true, true, sw);
    char text[256], gtext[160] = "";
    mdt_route_text(p, text, sizeof text);
    if (p.path == MDT_DW_COPY) {   // out'(N x K) = dY^T . (X^T)^T: S slices of L rows as one batched product
        GemmCase c = gc("", N, K, p.L);
        c.batch = p.S > 1 ? p.S : 0;
        mdt_route_text(mdt_route_gemm(args_of(c), sw), gtext, sizeof gtext);
    }
    printf("%s: %s%s%s\n", key, text, gtext[0] ? " gemm: " : "", gtext);
}
static void attn_train(const char* key, int hd, int H, int Tq, int Tk, int causal = 0, int rope = 0, int kv_rows = 0, bool drop = false) {
    for (int bwd = 0; bwd < 2; ++bwd) {
        if (g_cases) {
            printf("attn_train/%s_%s %d %d %d %d %d %d %d %d %d\n", key, bwd ? "bwd" : "fwd", hd, H, Tq, Tk, causal, rope, kv_rows, (int)drop, bwd);
            continue;
        }
        char text[160];
        mdt_route_text(mdt_route_attn_train(hd, H, Tq, Tk, causal, rope, kv_rows, drop, bwd != 0), text, sizeof text);
        printf("attn_train/%s_%s: %s\n", key, bwd ? "bwd" : "fwd", text);
    }
}
// LayerNorm forward / backward of B samples of rps rows, and the merge fused with each; off: bytes the activation pointers are off
// a 16-byte boundary
static void ln(const char* key, int D, int rps, int off = 0, int row_chunks = 0, bool out_is_a = false) {
    if (g_cases) return;
    float* const X = (float*)(uintptr_t)(4096 + off);
    float* const Y = (float*)(uintptr_t)(8192 + off);
    float* const Z = (float*)(uintptr_t)(12288 + off);
    mdt_ln_train_args f;
    memset(&f, 0, sizeof f);
    f.x = X; f.w = SOME; f.b = SOME; f.out = Y; f.M = 8 * rps; f.D = D; f.rows_per_sample = rps; f.shift_off = f.scale_off = -1;
    mdt_merge_args g;
    memset(&g, 0, sizeof g);
    g.x = Z; g.a = Y; g.out = out_is_a ? Y : X; g.B = 8; g.rows_per_sample = rps; g.D = D;
    mdt_ln_train_args fl = f;
    fl.x = g.out;
    mdt_ln_bwd_args b;
    memset(&b, 0, sizeof b);
    b.x = X; b.stats = SOME; b.w = SOME; b.b = SOME; b.dh = Y; b.ld_dh = D; b.dx = Z; b.pw = (float*)SOME; b.B = 8; b.rows_per_sample = rps;
    b.D = D; b.row_chunks = row_chunks; b.shift_off = b.scale_off = -1;
    mdt_merge_args gb = g;
    gb.x = b.dx; gb.out = Y;
    const mdt_ln_bwd_route r = mdt_route_ln_bwd(b, nullptr), rm = mdt_route_ln_bwd(b, &gb);
    printf("ln/%s: fwd=%s merge_ln_fwd=%s bwd=%s rb=%d chunks=%d lds=%zu ln_bwd_merge=%s rb=%d lds=%zu\n", key, mdt_rowwise_form_name(mdt_route_ln_fwd(f)),
           mdt_rowwise_form_name(mdt_route_merge_ln_fwd(g, fl)), mdt_rowwise_form_name(r.form), r.rb, r.chunks, r.lds, mdt_rowwise_form_name(rm.form),
           rm.rb, rm.lds);
}
static void colsum(int M, int N, bool aligned = true) {
    if (g_cases) return;
    printf("colsum/%dx%d%s: %s colsum2=%s\n", M, N, aligned ? "" : "_off4", mdt_colsum_form_name(mdt_route_colsum(N, M, N, aligned)),
           M >= MDT_COLSUM_DEEP_ROWS ? "two colsums" : "k_colsum2");
}

// ---- whole training steps at deep row counts (tests/deep_row_configs.py, tests/test_gpu_deep_row_training.py) ----
// One line per product of a step of the model at batch B: <layer>.fwd the forward product (M, N, K), <layer>.bwd the plan of its
// weight / bias gradient, <layer>.dx its input-gradient product (M, K, N).  enc.* run on the B Te encoder rows, dec.* on the B Ta
// decoder rows, the rest on B rows (the token embedding: B n_tok).  A training step's products have no LayerNorm prologue (the
// LayerNorm is a launch of its own); c_fc leaves its pre-activation (aux_mode 1), c_proj's input gradient applies the activation's
// backward (aux_mode 2).
struct StepCase {
    const char* tag;
    int B, Ta = 10, Te = 4, D = 384, H = 8, A = 7, Ld = 4, n_tok = 3, G = 512, O = 384, HP = 0;
    bool proprio = false, mdt = false;
    mdt_route_switches sw;
};
static void step_product(const StepCase& c, const char* layer, int M, int N, int K, int fwd_aux = 0, int dx_aux = 0) {
    if (g_cases) return;
    char text[256];
    GemmCase f = gc("", M, N, K);
    if (fwd_aux) f = with_aux(f, fwd_aux);
    mdt_route_text(mdt_route_gemm(args_of(f), c.sw), text, sizeof text);
    printf("deep/%s/%s.fwd: %dx%dx%d %s\n", c.tag, layer, M, N, K, text);
    mdt_route_text(mdt_route_linear_bwd(M, N, K, true, true, true, c.sw), text, sizeof text);
    printf("deep/%s/%s.bwd: %dx%dx%d %s\n", c.tag, layer, M, N, K, text);
    GemmCase x = gc("", M, K, N);
    if (dx_aux) x = with_aux(x, dx_aux);
    mdt_route_text(mdt_route_gemm(args_of(x), c.sw), text, sizeof text);
    printf("deep/%s/%s.dx: %dx%dx%d %s\n", c.tag, layer, M, K, N, text);
}
static void step(const StepCase& c) {
    const int D = c.D, Me = c.B * c.Te, Md = c.B * c.Ta;
    for (int dec = 0; dec < 2; ++dec) {
        const int M = dec ? Md : Me;
        char layer[32];
        auto name = [&](const char* l) { snprintf(layer, sizeof layer, "%s.%s", dec ? "dec" : "enc", l); return layer; };
        step_product(c, name("qkv"), M, 3 * D, D);
        step_product(c, name("proj"), M, D, D);   // attn.c_proj; the decoder's cross_att.query and cross_att.c_proj have its shape
        step_product(c, name("c_fc"), M, 4 * D, D, 1);
        step_product(c, name("c_proj"), M, D, 4 * D, 0, 2);
    }
    step_product(c, "enc.kv_all", Me, c.Ld * 2 * D, D);   // every decoder block's cross-attention K | V from the context, stacked
    if (c.HP) step_product(c, "dec.head0", Md, c.HP, D);
    step_product(c, "mod_all", c.B, c.Ld * 6 * D, D);     // every decoder block's adaLN modulation, stacked
    step_product(c, "sigma_emb.1", c.B, 2 * D, D);
    step_product(c, "sigma_emb.3", c.B, D, 2 * D);
    step_product(c, "goal_emb.0", c.B, 2 * D, c.G);
    step_product(c, "goal_emb.2", c.B, D, 2 * D);
    step_product(c, "tok_emb", c.mdt ? c.B : c.B * c.n_tok, D, c.O);   // MDT: the static and the gripper camera's, one row per sample each
    if (c.proprio) step_product(c, "proprio_emb.2", c.B, D, 2 * D);
    if (g_cases) return;
    // the attention launches: encoder and decoder self-attention, the cross-attention (causal, top-left aligned: at a context above
    // 16 tokens it stages the visible prefix)
    const int H = c.H, hd = c.D / H;
    const int kv = c.Te > 16 ? (c.Te < c.Ta ? c.Te : c.Ta) : 0;   // mdt_visible_keys
    for (int bwd = 0; bwd < 2; ++bwd) {
        char e[160], d[160], x[160];
        mdt_route_text(mdt_route_attn_train(hd, H, c.Te, c.Te, 0, 0, 0, false, bwd != 0), e, sizeof e);
        mdt_route_text(mdt_route_attn_train(hd, H, c.Ta, c.Ta, 1, 0, 0, false, bwd != 0), d, sizeof d);
        mdt_route_text(mdt_route_attn_train(hd, H, c.Ta, c.Te, 1, 0, kv, false, bwd != 0), x, sizeof x);
        printf("deep/%s/attn.%s: enc %dx%d %s | dec %dx%d %s | cross %dx%d kv_rows=%d %s\n", c.tag, bwd ? "bwd" : "fwd", c.Te, c.Te, e, c.Ta, c.Ta, d,
               c.Ta, c.Te, kv, x);
    }
    printf("deep/%s/narrow: A=%d rows=%d slice_rows=%d..%d tiles=%d\n", c.tag, c.A, Md, Md / 512, (Md + 511) / 512, mdt_route_narrow_tiles(c.A));
}

// The plan's invariants over N, K in DIMS and every M up to 2048 plus the row counts where a rule changes: S L >= M, L % 32 == 0,
// regions disjoint and inside the total, the split plan never more slices than the fp32 plan, and the total of every path inside
// the bound mdt_route_linear_bwd_scratch gives for every capacity >= M of the sweep.
static bool plan_ok(const mdt_linear_bwd_plan& p, int64_t M, int64_t N, int64_t K, const char* what) {
    const int64_t Mp = (int64_t)p.S * p.L;
    bool ok = p.S >= 1 && Mp >= M && p.L % 32 == 0;
    if (p.path == MDT_DW_COPY)   // dYt [S][N][L], Xt [S][K][L], parts [S][N][K], bpart (ceil(M / 32), N)
        ok = ok && p.dYt == 0 && p.dYt + N * Mp <= p.Xt && p.Xt + K * Mp <= p.parts && p.parts + (int64_t)p.S * N * K <= p.bpart &&
             p.bpart + (M + 31) / 32 * N <= p.total;
    else   // parts [S][N][K], bpart [S][N]
        ok = ok && p.parts == 0 && p.parts + (int64_t)p.S * N * K <= p.bpart && p.bpart + (int64_t)p.S * N <= p.total &&
             p.gz == (unsigned)p.S && (int)p.gx == ((N + p.tn - 1) / p.tn) * ((K + p.tk - 1) / p.tk) && p.lds <= MDT_LDS_MAX;
    if (!ok) printf("invariants: VIOLATED by the %s plan at M=%lld N=%lld K=%lld (S=%d L=%d total=%lld)\n", what, (long long)M, (long long)N, (long long)K, p.S, p.L, (long long)p.total);
    return ok;
}
static void invariants() {
    if (g_cases) return;
    const int DIMS[] = {16, 64, 80, 192, 208, 384, 576, 1152, 1536};
    static int64_t rows[2048 + 6];
    int n_rows = 0;
    for (int m = 1; m <= 2048; ++m) rows[n_rows++] = m;
    for (int64_t m : {8191, 8192, 8193, 10240, 50176, 104448}) rows[n_rows++] = m;
    mdt_route_switches on, off;
    off.tn_split = 0;
    long points = 0;
    for (int N : DIMS)
        for (int K : DIMS) {
            int64_t worst = 0;   // the largest total of any row count so far: every capacity from here on must cover it
            for (int i = 0; i < n_rows; ++i) {
                const int64_t M = rows[i];
                const mdt_linear_bwd_plan split = mdt_route_linear_bwd(M, N, K, true, true, true, on), fp32 = mdt_route_linear_bwd(M, N, K, true, true, true, off),
                                          copy = mdt_route_linear_bwd(M, N, K, false, true, true, on);
                if (!plan_ok(split, M, N, K, "split") || !plan_ok(fp32, M, N, K, "fp32") || !plan_ok(copy, M, N, K, "copy")) return;
                if (split.S > fp32.S || fp32.path != MDT_DW_TN || copy.path != MDT_DW_COPY) {
                    printf("invariants: VIOLATED at M=%lld N=%d K=%d: %d split slices, %d fp32 slices\n", (long long)M, N, K, split.S, fp32.S);
                    return;
                }
                worst = std::max(worst, std::max(std::max(split.total, fp32.total), copy.total));
                if (std::max(fp32.total, copy.total) != mdt_route_linear_bwd_scratch_exact(M, N, K) || worst > mdt_route_linear_bwd_scratch(M, N, K)) {
                    printf("invariants: VIOLATED at M=%lld N=%d K=%d: a row count up to here needs %lld floats, the bound is %lld\n", (long long)M, N, K,
                           (long long)worst, (long long)mdt_route_linear_bwd_scratch(M, N, K));
                    return;
                }
                ++points;
            }
        }
    printf("invariants: OK (%ld points)\n", points);
}

int main(int argc, char** argv) {
    g_cases = argc > 1 && !strcmp(argv[1], "--cases");
    // small-M row limit
    gemm(with_ln(gc("ln_15", 15)));
    gemm(with_ln(gc("ln_16", 16)));
    // few tiles behind a LayerNorm prologue: 54 vs 60 half-height tiles
    gemm(with_ln(gc("ln_144", 144)));
    gemm(with_ln(gc("ln_160", 160)));
    // few tiles, plain, up to 192 rows: 96 vs 108 tiles
    gemm(gc("192x512", 192, 512));
    gemm(gc("192x576", 192, 576));
    // few tiles, plain, up to 512 rows: 140 vs 160 tiles
    gemm(gc("320x448", 320, 448));
    gemm(gc("320x512", 320, 512));
    // GEMM_SMALLM_ROWS
    gemm(gc("512x64", 512, 64));
    gemm(gc("513x64", 513, 64));
    // GEMM_MID_MAX
    gemm(gc("1400", 1400));
    gemm(gc("1401", 1401));
    // the 32 x 192 rule behind a LayerNorm prologue: fills 1.0, 0.625, 0.75, 0.9375
    gemm(with_ln(gc("ln_1024x1536", 1024, 1536)));
    gemm(with_ln(gc("ln_1280x1536", 1280, 1536)));
    gemm(with_ln(gc("ln_1024x1152", 1024, 1152)));
    gemm(with_ln(gc("ln_1280x1152", 1280, 1152)));
    // deep K, plain, residual
    gemm(with_res(gc("res_2560x384x1536", 2560, 384, 1536)));
    gemm(with_res(gc("res_5120x384x1536", 5120, 384, 1536)));
    // 4096 rows, plain
    gemm(gc("4096x1536", 4096, 1536));
    gemm(gc("4096x384", 4096, 384));
    // the 8192-row boundary
    gemm(gc("8191", 8191));
    gemm(gc("8192", 8192));
    // weight-stationary, split and fp32
    gemm(gc("10240x1536", 10240, 1536));
    gemm(no_ws_split(gc("10240x1536_ws_split0", 10240, 1536)));
    gemm(gc("10240x384", 10240, 384));
    gemm(no_ws_split(gc("10240x384_ws_split0", 10240, 384)));
    gemm(no_ws_split(gc("10240x1152_ws_split0", 10240, 1152)));
    // the tall body
    gemm(with_res(gc("res_10240x384x1536", 10240, 384, 1536)));
    // ws_split_192
    gemm(gc("104448x576x192", 104448, 576, 192));
    gemm(no_ws_split(gc("104448x576x192_ws_split0", 104448, 576, 192)));
    // SwishGLU epilogues: the weight-stationary body from 8192 rows on, the tiled kernels below
    gemm(with_aux(gc("glu3_104448x768x192", 104448, 768, 192), 3));
    gemm(with_aux(gc("glu4_104448x768x192", 104448, 768, 192), 4));
    gemm(no_ws_split(with_aux(gc("glu3_104448x768x192_ws_split0", 104448, 768, 192), 3)));
    gemm(no_ws_split(with_aux(gc("glu4_104448x768x192_ws_split0", 104448, 768, 192), 4)));
    gemm(with_aux(gc("glu3_1024x768x192", 1024, 768, 192), 3));
    gemm(with_aux(gc("glu3_1024x576x192", 1024, 576, 192), 3));
    gemm(with_aux(gc("glu4_1024x768x192", 1024, 768, 192), 4));
    gemm(with_aux(gc("glu4_1024x256x192", 1024, 256, 192), 4));
    // slab merge
    gemm(with_parts(gc("parts4_2560x1152", 2560, 1152), 4));
    gemm(with_parts(gc("parts4_2560x1536", 2560, 1536), 4));
    // the LayerNorm-prologue split product, with the pair image set
    gemm(with_pair(gc("pair_767x1152", 767, 1152)));
    gemm(with_pair(gc("pair_768x1152", 768, 1152)));
    gemm(with_pair(gc("pair_768x1536x512", 768, 1536, 512)));
    gemm(with_parts(with_pair(gc("pair_parts4_2560x1152", 2560, 1152)), 4));
    gemm(no_mlp_split(with_pair(gc("pair_768x1152_mlp_split0", 768, 1152))));
    gemm(with_geo(with_pair(gc("pair_768x1152_geo3", 768, 1152)), 3));
    // batched
    {
        GemmCase c = gc("batch4_1024", 1024);
        c.batch = 4;
        gemm(c);
    }
    // a pending side job
    {
        GemmCase c = gc("side_10", 10);
        c.sw.side_pending = 1;
        gemm(c);
        gemm(gc("10", 10));
    }
    // forced geometries
    gemm(with_geo(gc("geo-1_2560", 2560), -1));
    {
        static char keys[9][16];
        for (int g = 1; g <= 9; ++g) {
            snprintf(keys[g - 1], sizeof keys[0], "geo%d_2560", g);
            gemm(with_geo(gc(keys[g - 1], 2560), g));
        }
    }
    gemm(with_geo(gc("geo2_2560x384x1536", 2560, 384, 1536), 2));
    gemm(with_geo(gc("geo6_160x384x1536", 160, 384, 1536), 6));
    gemm(with_geo(gc("geo23_10240x1152", 10240, 1152), 23));
    gemm(with_geo(with_ln(gc("ln_geo23_2560", 2560)), 23));
    gemm(with_geo(gc("geo30_2560", 2560), 30));
    gemm(with_geo(with_ln(gc("ln_geo30_2560", 2560)), 30));
    // refusals
    gemm(gc("refused_32768x32768", 64, 32768, 32768));
    gemm(gc("refused_N65552", 64, 65552, 16));
    gemm(with_aux(with_ln(gc("refused_aux_ln", 64)), 1));

    // the blocks of the model: d = 384, 8 heads of 48, 10 action rows, 4 context rows
    for (int B : {1, 2, 3, 32, 33, 76, 77, 140, 141, 272, 273, 512, 513}) {
        BlockCase c;
        c.B = B;
        block(c);
    }
    for (int B : {77, 141}) {
        BlockCase c;
        c.B = B; c.tag = "_mlp_split0"; c.sw.mlp_split = 0;
        block(c);
    }
    for (int B : {33, 141}) {
        BlockCase c;
        c.B = B; c.tag = "_attn_wide_min0"; c.sw.attn_wide_min = 0;
        block(c);
    }
    for (int B : {141, 272, 273}) {   // RoPE (heads of 64): no fused attention form takes it
        BlockCase c;
        c.B = B; c.tag = "_rope_hd64"; c.rope = 1; c.hd = 64;
        block(c);
    }
    for (int B : {140, 141, 272, 273}) {   // no collapsed cross-attention: the tiled form from 1401 rows up to 256 tiles (B = 272)
        BlockCase c;
        c.B = B; c.tag = "_no_fold"; c.fold = false;
        block(c);
    }
    {
        BlockCase c;
        c.B = 4; c.tag = "_A9"; c.A = 9;
        block(c);
        c.tag = "_A17"; c.A = 17;
        block(c);
        c.tag = "_Ta17"; c.A = 7; c.Ta = 17;
        block(c);
    }

    // ---- the Linear backward (dW and dbias): the small shapes of tests/linear_bwd_shapes.py, whose hand-worked slice counts
    // tests/test_route_table.py asserts against these lines ----
    for (int M : {1, 31, 32, 33, 127, 128, 129, 130}) lin_bwd(M, 64, 128);
    for (int N : {16, 48, 80, 240}) lin_bwd(300, N, 128);
    for (int K : {16, 80, 208, 192, 576}) lin_bwd(300, 64, K);
    lin_bwd(1024, 16, 16);
    lin_bwd(1000, 80, 208);
    lin_bwd(300, 48, 80);
    lin_bwd(257, 64, 128);
    // 8192 rows: n-tile 64 -> 128, split off -> on
    lin_bwd(8191, 384, 384);
    lin_bwd(8192, 384, 384);
    lin_bwd(8192, 1152, 384);
    lin_bwd(8192, 192, 768);    // N = 192: the split kernel's 192 x 128 tile; its fp32 form: the 192-wide tile
    lin_bwd(8192, 192, 768, true, false);
    lin_bwd(8192, 192, 192);    // ... and the fp32 form below 576 x 192: 64 wide
    lin_bwd(8192, 192, 192, true, false);
    lin_bwd(10240, 640, 128);
    for (int split = 1; split >= 0; --split) {
        lin_bwd(12288, 1536, 384, true, split != 0);
        lin_bwd(12288, 384, 1536, true, split != 0);
    }
    lin_bwd(33000, 768, 208);
    lin_bwd(8223, 240, 80);
    // the masked-image head's 104 k rows: the fp32 form runs one round of 192-wide workgroups
    for (int split = 1; split >= 0; --split) {
        lin_bwd(104448, 1536, 192, true, split != 0);
        lin_bwd(104448, 576, 192, true, split != 0);
    }
    lin_bwd(104448, 192, 192);   // whole rounds of resident workgroups
    // a row stride that is no multiple of 4 floats: transposed copies, S = 1 and S > 1
    lin_bwd(300, 64, 128, false);
    lin_bwd(5000, 384, 384, false);
    invariants();

    // ---- training attention, forward and backward ----
    attn_train("hd64_H8", 64, 8, 10, 10);   // head groups 4 / 2 / 1
    attn_train("hd64_H6", 64, 6, 10, 10);
    attn_train("hd64_H7", 64, 7, 10, 10);
    attn_train("hd16_H8", 16, 8, 10, 10);
    attn_train("hd48_H8", 48, 8, 10, 10);
    attn_train("hd64_H8_rope", 64, 8, 10, 10, 0, 1);   // one wave per head
    attn_train("hd24_H8", 24, 8, 10, 10);              // refused
    attn_train("hd48_16x16", 48, 8, 16, 16, 1);
    attn_train("hd48_17x16", 48, 8, 17, 16, 1);        // the chunk kernels
    attn_train("hd48_10x17", 48, 8, 10, 17, 1);
    attn_train("hd48_64x64", 48, 8, 64, 64, 1);
    attn_train("hd48_65x64", 48, 8, 65, 64, 1);        // refused
    attn_train("hd16_17x17", 16, 8, 17, 17);           // refused: the chunk kernels take heads of 32 / 48 / 64
    attn_train("hd48_10x20_kv10", 48, 8, 10, 20, 1, 0, 10);   // a causal prefix that holds every visible key
    attn_train("hd48_10x20_kv9", 48, 8, 10, 20, 1, 0, 9);     // ... and one that does not
    attn_train("hd48_10x10_kv5", 48, 8, 10, 10, 1, 0, 5);     // the 16-row kernels have no prefix form
    attn_train("hd48_17x16_drop", 48, 8, 17, 16, 1, 0, 0, true);
    attn_train("hd48_10x10_drop", 48, 8, 10, 10, 1, 0, 0, true);

    // ---- the row-wise kernels ----
    ln("D384", 384, 10);
    ln("D384_off4", 384, 10, 4);
    ln("D382", 382, 10);
    ln("D384_rps4", 384, 4);     // rows a wave keeps in flight: 1 / 2 / 2 / 3
    ln("D384_rps5", 384, 5);
    ln("D384_rps8", 384, 8);
    ln("D384_rps9", 384, 9);
    ln("D384_chunks2", 384, 10, 0, 2);          // two workgroups per sample: the merge backward is a launch of its own
    ln("D384_out_is_a", 384, 10, 0, 0, true);   // the merge writes over its branch input: not fused with the LayerNorm behind it
    ln("D516", 516, 10);                        // wider than a row held in registers: refused
    colsum(64, 16380);
    colsum(64, 16384);
    colsum(64, 16384, false);
    colsum(511, 384);
    colsum(512, 384);
    colsum(1024, 4096);
    colsum(1024, 4100);
    for (int A : {16, 17}) {
        if (g_cases) break;
        printf("narrow/A%d: %s tiles=%d\n", A, mdt_route_narrow_tiles(A) ? "k_narrow_out<true> k_narrow_dw<true>" : "k_narrow_out<false> k_narrow_dw<false>",
               mdt_route_narrow_tiles(A));
    }

    // ---- the whole steps of tests/deep_row_configs.py, batch by batch ----
    // 4096 rows: geometry 9; 5120: geometry 5 at d = 384; 8128: the last batch below the 8192-row routes; 8192: on them
    for (int B : {64, 80, 127, 128}) {
        static char tags[4][24];
        char* tag = tags[B == 64 ? 0 : (B == 80 ? 1 : B - 125)];
        snprintf(tag, sizeof tags[0], "ta64_a64_B%d", B);
        StepCase c;
        c.tag = tag; c.B = B; c.Ta = 64; c.A = 64;
        step(c);
    }
    {
        StepCase c;
        c.tag = "ta64_a64_B128_split0"; c.B = 128; c.Ta = 64; c.A = 64; c.sw.ws_split = 0; c.sw.tn_split = 0;
        step(c);
        c.tag = "ta64_a64_B105"; c.B = 105; c.sw = mdt_route_switches();   // the scratch-reuse test's smaller batch
        step(c);
        c.tag = "ta64_a64_d192_B128"; c.B = 128; c.D = c.O = 192; c.H = 4;
        step(c);
        c.tag = "ta64_a64_d256_B64"; c.B = 64; c.D = c.O = 256; c.H = 8; c.G = 384;   // geometries 5 and 9 at 4096 rows
        step(c);
    }
    {
        StepCase c;
        c.tag = "ctx64_B128"; c.B = 128; c.Te = 64; c.n_tok = 63;
        step(c);
        c = StepCase();
        c.tag = "a64_rows2600_B260"; c.B = 260; c.A = 64;
        step(c);
        c = StepCase();
        c.tag = "a17_mlp_proprio_rows2600_B260"; c.B = 260; c.A = 17; c.HP = 112; c.Te = 5; c.proprio = true;
        step(c);
        c = StepCase();
        c.tag = "mdt_ta40_B205"; c.B = 205; c.Ta = 40; c.Te = 3; c.D = c.O = 512; c.Ld = 6; c.mdt = true;
        step(c);
    }
    if (!g_cases) {
        // scratch reuse: S of the 384 x 384 weight gradients (attn.c_proj and its kin) at the smaller batch and at the capacity batch
        mdt_route_switches sw;
        const mdt_linear_bwd_plan small = mdt_route_linear_bwd(105 * 64, 384, 384, true, true, true, sw), cap = mdt_route_linear_bwd(128 * 64, 384, 384, true, true, true, sw);
        printf("deep/scratch_reuse: B=105 rows=%d S=%d total=%lld | B=128 rows=%d S=%d total=%lld | bound_at_8192=%lld\n", 105 * 64, small.S, (long long)small.total,
               128 * 64, cap.S, (long long)cap.total, (long long)mdt_route_linear_bwd_scratch(128 * 64, 384, 384));
    }
    return 0;
}
