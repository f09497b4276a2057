/*
 * A plain-C host program that samples and selects through the C ABI alone, forwards only: K candidate chunks for each observation
 * from one encoded context (mdt_sample_ddim_multi), each scored by its likelihood-weighted denoising error in one native call
 * (mdt_denoising_score with the caller's levels and noise rows and the library's own trapezoid weights, the context again shared
 * per observation), then the best-scoring candidate per observation.  No Python, no torch, no mdt_train_prepare in the process.
 *
 *   score_client <blob> <out>
 * blob (little endian): int32 n_cfg_fields(19) | 19 x int32 mdt_config fields | float sigma_data |
 *   int32 n_params | per parameter: int32 name_len, name bytes, int64 numel, numel x float |
 *   int32 B, int32 K, int32 S, int32 M, int32 n_steps, (n_steps+1) x float sigmas, S x float levels (strictly monotone) |
 *   tokens (B) | goal (B) | x_T (B*K) | noise (S*M chunks)
 * out: B*K*Ta*A floats, the candidates (chunk k of observation b at row b*K + k), B*K floats, their scores, then B int32, the
 * candidate chosen per observation.  Before the scoring call the program checks that candidates = 0, draws = 0 and n_levels = 65
 * are refused with MDT_ERR_INVALID_ARG, the entry and the field in the message, and leave the handle usable.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mdt_hip.h"

#define CHECK(st)                                                                        \
    do {                                                                                 \
        if ((st) != MDT_OK) { fprintf(stderr, "mdt error: %s\n", mdt_last_error()); return 2; } \
    } while (0)
#define HIPCHECK(e)                                                                      \
    do {                                                                                 \
        if ((e) != hipSuccess) { fprintf(stderr, "hip error %d at line %d\n", (int)(e), __LINE__); return 3; } \
    } while (0)

static int rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n ? 0 : -1; }

static float* to_device(FILE* f, size_t n) {
    float* h = (float*)malloc(n * sizeof(float));
    float* d = NULL;
    if (!h || rd(f, h, n * sizeof(float)) || hipMalloc((void**)&d, n * sizeof(float)) != hipSuccess ||
        hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { free(h); return NULL; }
    free(h);
    return d;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: score_client <blob> <out>\n"); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("blob"); return 1; }
    int32_t nf = 0, fields[32];
    mdt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    if (rd(f, &nf, 4) || nf != 19 || rd(f, fields, 4 * nf) || rd(f, &cfg.sigma_data, 4)) return 1;
    memcpy(&cfg, fields, 4 * nf); /* the 19 int32 fields lead the struct in declaration order */
    mdt_model* m = NULL;
    CHECK(mdt_create(&cfg, &m));
    hipStream_t s;
    HIPCHECK(hipStreamCreate(&s));
    int32_t np = 0;
    if (rd(f, &np, 4)) return 1;
    for (int i = 0; i < np; ++i) {
        int32_t nl = 0;
        char name[512];
        int64_t numel = 0;
        if (rd(f, &nl, 4) || nl <= 0 || nl >= (int)sizeof name || rd(f, name, nl) || rd(f, &numel, 8)) return 1;
        name[nl] = 0;
        float* h = (float*)malloc((size_t)numel * sizeof(float));
        if (!h || rd(f, h, (size_t)numel * sizeof(float))) return 1;
        CHECK(mdt_load_param(m, name, h, numel, s));
        HIPCHECK(hipStreamSynchronize(s));
        free(h);
    }
    int32_t B = 0, K = 0, S = 0, M = 0, n_steps = 0;
    float sigmas[MDT_SAMPLER_MAX_STEPS + 1], levels[64];
    if (rd(f, &B, 4) || rd(f, &K, 4) || rd(f, &S, 4) || rd(f, &M, 4) || B < 1 || K < 1 || S < 1 || S > 64 || M < 1 || M > 64 ||
        rd(f, &n_steps, 4) || n_steps < 1 || n_steps > MDT_SAMPLER_MAX_STEPS || rd(f, sigmas, 4 * (n_steps + 1)) ||
        rd(f, levels, 4 * S)) return 1;
    const int n_tok = cfg.arch == MDT_ARCH_MDTV ? cfg.n_obs_token : 1;
    const size_t ntok = (size_t)B * n_tok * cfg.obs_dim, ngoal = (size_t)B * cfg.goal_dim;
    const size_t per = (size_t)cfg.action_seq_len * cfg.action_dim, nact = (size_t)B * K * per; /* per chunk: B * K of them */
    float* tok = to_device(f, ntok);
    float* tok2 = cfg.arch == MDT_ARCH_MDT ? to_device(f, ntok) : NULL;
    float* goal = to_device(f, ngoal);
    float* xT = to_device(f, nact);
    float* noise = to_device(f, (size_t)S * M * per); /* the same rows for every chunk */
    if (!tok || !goal || !xT || !noise) return 1;
    fclose(f);
    float *out = NULL, *score = NULL;
    HIPCHECK(hipMalloc((void**)&out, nact * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&score, (size_t)B * K * sizeof(float)));
    /* K candidates per observation from one context ... */
    CHECK(mdt_sample_ddim_multi(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, sigmas, n_steps, B, K, out, NULL, NULL, s));
    /* ... what the scoring call refuses, by name ... */
    const struct { int32_t k, n, d; const char* field; } bad[3] = {{0, S, M, "candidates"}, {K, S, 0, "draws"}, {K, 65, M, "n_levels"}};
    for (int i = 0; i < 3; ++i)
        if (mdt_denoising_score(m, tok, tok2, goal, MDT_MODALITY_LANG, out, levels, NULL, bad[i].n, noise, bad[i].d, B, bad[i].k, score,
                                NULL, s) != MDT_ERR_INVALID_ARG ||
            !strstr(mdt_last_error(), "mdt_denoising_score") || !strstr(mdt_last_error(), bad[i].field)) {
            fprintf(stderr, "a bad %s was not refused by name: %s\n", bad[i].field, mdt_last_error());
            return 4;
        }
    /* ... and their scores: one enqueue, nothing read back until the stream is idle */
    CHECK(mdt_denoising_score(m, tok, tok2, goal, MDT_MODALITY_LANG, out, levels, NULL, S, noise, M, B, K, score, NULL, s));
    HIPCHECK(hipStreamSynchronize(s));
    float* h = (float*)malloc(nact * sizeof(float));
    float* hs = (float*)malloc((size_t)B * K * sizeof(float));
    int32_t* pick = (int32_t*)malloc((size_t)B * sizeof(int32_t));
    if (!h || !hs || !pick) return 1;
    HIPCHECK(hipMemcpy(h, out, nact * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hs, score, (size_t)B * K * sizeof(float), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) { /* the best score; ties go to the lowest index */
        pick[b] = 0;
        for (int k = 1; k < K; ++k)
            if (hs[(size_t)b * K + k] > hs[(size_t)b * K + pick[b]]) pick[b] = k;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(h, sizeof(float), nact, o) != nact || fwrite(hs, sizeof(float), (size_t)B * K, o) != (size_t)B * K ||
        fwrite(pick, sizeof(int32_t), (size_t)B, o) != (size_t)B) return 1;
    fclose(o);
    printf("scored ddim: %d observations, %d candidates each, %d levels, %d draws, %s\n", B, K, S, M, mdt_version());
    CHECK(mdt_destroy(m));
    return 0;
}
