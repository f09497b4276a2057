/*
 * A plain-C host program that runs the replan-and-select loop of a controller as ONE call through the C ABI: K candidate chunks for
 * each observation sampled from one encoded context, scored by their likelihood-weighted denoising error against that same context
 * and the best chunk of every observation selected on the device (mdt_sample_ddim_select).  One enqueue, nothing read back until
 * the stream is idle.  No Python, no torch in the process.
 *
 *   select_client <blob> <out>
 * blob (little endian): int32 n_cfg_fields(19) | 19 x int32 mdt_config fields | float sigma_data |
 *   int32 n_params | per parameter: int32 name_len, name bytes, int64 numel, numel x float |
 *   int32 B, int32 K, int32 S, int32 M, int32 n_steps, (n_steps+1) x float sigmas, S x float levels (strictly monotone) |
 *   tokens (B) | goal (B) | x_T (B*K) | noise (S*M chunks)
 * out: B int32, the candidate chosen per observation, B*Ta*A floats, the chosen chunks, B*K floats, the scores, then B*K*Ta*A floats,
 * all the candidates.  Before the call the program checks that a NULL select, a select.size of 8, a NULL select.index and
 * n_levels = 65 are refused with MDT_ERR_INVALID_ARG, the entry and the field in the message, and leave the handle usable.  It
 * prints the index and the first elements of the chosen chunk of every observation.
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
    if (argc != 3) { fprintf(stderr, "usage: select_client <blob> <out>\n"); return 1; }
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
    float *chunks = NULL, *score = NULL, *best = NULL;
    int32_t* index = NULL;
    HIPCHECK(hipMalloc((void**)&chunks, nact * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&score, (size_t)B * K * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&best, (size_t)B * per * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&index, (size_t)B * sizeof(int32_t)));
    mdt_select_spec sel;
    memset(&sel, 0, sizeof sel);
    sel.size = (int32_t)sizeof sel;
    sel.sigmas_host = levels; /* weights_host stays NULL: the trapezoid rule in ln sigma */
    sel.n_levels = S;
    sel.noise = noise;
    sel.draws = M;
    sel.chunks = chunks;
    sel.scores = score;
    sel.index = index;
    /* what the call refuses, by name ... */
    mdt_select_spec bad[3] = {sel, sel, sel};
    const char* field[4] = {"select.size", "select.index", "n_levels", "select"};
    bad[0].size = 8;
    bad[1].index = NULL;
    bad[2].n_levels = 65;
    for (int i = 0; i < 4; ++i)
        if (mdt_sample_ddim_select(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, sigmas, n_steps, B, K, best, NULL, NULL,
                                   i < 3 ? &bad[i] : NULL, s) != MDT_ERR_INVALID_ARG ||
            !strstr(mdt_last_error(), "mdt_sample_ddim_select") || !strstr(mdt_last_error(), field[i])) {
            fprintf(stderr, "a bad %s was not refused by name: %s\n", field[i], mdt_last_error());
            return 4;
        }
    /* ... and the call: sample, score, select */
    CHECK(mdt_sample_ddim_select(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, sigmas, n_steps, B, K, best, NULL, NULL, &sel, s));
    HIPCHECK(hipStreamSynchronize(s));
    float* h = (float*)malloc(nact * sizeof(float));
    float* hs = (float*)malloc((size_t)B * K * sizeof(float));
    float* hb = (float*)malloc((size_t)B * per * sizeof(float));
    int32_t* pick = (int32_t*)malloc((size_t)B * sizeof(int32_t));
    if (!h || !hs || !hb || !pick) return 1;
    HIPCHECK(hipMemcpy(h, chunks, nact * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hs, score, (size_t)B * K * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(hb, best, (size_t)B * per * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(pick, index, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(pick, sizeof(int32_t), (size_t)B, o) != (size_t)B || fwrite(hb, sizeof(float), (size_t)B * per, o) != (size_t)B * per ||
        fwrite(hs, sizeof(float), (size_t)B * K, o) != (size_t)B * K || fwrite(h, sizeof(float), nact, o) != nact) return 1;
    fclose(o);
    for (int b = 0; b < B; ++b)
        printf("observation %d: candidate %d, score %.9g, chunk %.9g %.9g %.9g ...\n", b, (int)pick[b], (double)hs[(size_t)b * K + pick[b]],
               (double)hb[(size_t)b * per], (double)hb[(size_t)b * per + 1], (double)hb[(size_t)b * per + 2]);
    printf("selected ddim: %d observations, %d candidates each, %d levels, %d draws, %s\n", B, K, S, M, mdt_version());
    CHECK(mdt_destroy(m));
    return 0;
}
