// route_table.cpp -- which kernel a shape takes, one line per case, from the host-only route functions of
// mdt_policy_amd/csrc/mdt_route.h.  Stand-alone: no GPU, no library; tests/test_route_table.py builds it with the sanitizers and
// compares its lines with route_table.expected beside it.
//   route_table           the table:       <key>: <route>
//   route_table --cases   the GEMM cases as numbers, for a driver that issues them on a GPU and compares a kernel trace:
//                         <key> M N K ln residual aux_mode a_parts batch image geometry mlp_split ws_split side
//                         (image: 0 none, 1 Wp_pair, 2 Wp_split)
// Each pair of GEMM cases straddles one rule of mdt_route_gemm.  N x K = 384 x 384 unless the key says otherwise.
#include <stdio.h>
#include <string.h>

#include "mdt_route.h"

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
    return 0;
}
