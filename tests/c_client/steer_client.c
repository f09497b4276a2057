/*
 * A plain-C host program that replans with a steer through the C ABI alone: K candidate chunks for each observation from one
 * encoded context, sampled with Heun's second-order sampler and steered toward the known part of the previous chunk through
 * the denoiser's Jacobian (mdt_sample_steer: D' = D + min(beta, 1 + sigma^2 / sigma_data^2) J^T (weight (known - D)) at every
 * evaluation of the sampler's plan).  No Python, no torch in the process.
 *
 *   steer_client <blob> <out>
 * blob (little endian): int32 n_cfg_fields(19) | 19 x int32 mdt_config fields | float sigma_data |
 *   int32 n_params | per parameter: int32 name_len, name bytes, int64 numel, numel x float |
 *   int32 B, int32 K, int32 n_steps, (n_steps+1) x float sigmas, float beta | tokens (B) | goal (B) | x_T (B*K) | known (B*K) |
 *   weight (B*K)
 * out: B*K*Ta*A floats, the steered candidates (chunk k of observation b at row b*K + k).  Before the call the program checks
 * that beta = 0 and an unknown sampler kind are refused with MDT_ERR_INVALID_ARG, the entry and the field in the message, and
 * leave the handle usable.
 */
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mdt_hip.h"
#include "mdt_hip_train.h"

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
    if (argc != 3) { fprintf(stderr, "usage: steer_client <blob> <out>\n"); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("blob"); return 1; }
    int32_t nf = 0, fields[32];
    mdt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    if (rd(f, &nf, 4) || nf != 19 || rd(f, fields, 4 * nf) || rd(f, &cfg.sigma_data, 4)) return 1;
    memcpy(&cfg, fields, 4 * nf); /* the 19 int32 fields lead the struct in declaration order */
    mdt_model* m = NULL;
    CHECK(mdt_create(&cfg, &m));
    CHECK(mdt_train_prepare(m)); /* the steer differentiates the denoiser: before the parameters go up */
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
    int32_t B = 0, K = 0, n_steps = 0;
    float sigmas[MDT_SAMPLER_MAX_STEPS + 1], beta = 0.f;
    if (rd(f, &B, 4) || rd(f, &K, 4) || B < 1 || K < 1 || rd(f, &n_steps, 4) || n_steps < 1 || n_steps > MDT_SAMPLER_MAX_STEPS ||
        rd(f, sigmas, 4 * (n_steps + 1)) || rd(f, &beta, 4)) return 1;
    const int n_tok = cfg.arch == MDT_ARCH_MDTV ? cfg.n_obs_token : 1;
    const size_t ntok = (size_t)B * n_tok * cfg.obs_dim, ngoal = (size_t)B * cfg.goal_dim;
    const size_t per = (size_t)cfg.action_seq_len * cfg.action_dim, nact = (size_t)B * K * per; /* per chunk: B * K of them */
    float* tok = to_device(f, ntok);
    float* tok2 = cfg.arch == MDT_ARCH_MDT ? to_device(f, ntok) : NULL;
    float* goal = to_device(f, ngoal);
    float* xT = to_device(f, nact);
    float* known = to_device(f, nact);
    float* weight = to_device(f, nact);
    if (!tok || !goal || !xT || !known || !weight) return 1;
    fclose(f);
    float* out = NULL;
    HIPCHECK(hipMalloc((void**)&out, nact * sizeof(float)));
    /* what the call refuses, by name ... */
    if (mdt_sample_steer(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, MDT_SAMPLER_HEUN, NULL, sigmas, n_steps, NULL, 0, B, K, known,
                         weight, 0.f, NULL, NULL, NULL, out, NULL, s) != MDT_ERR_INVALID_ARG ||
        !strstr(mdt_last_error(), "mdt_sample_steer") || !strstr(mdt_last_error(), "beta")) {
        fprintf(stderr, "beta = 0 was not refused by name: %s\n", mdt_last_error());
        return 4;
    }
    if (mdt_sample_steer(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, MDT_SAMPLER_COUNT, NULL, sigmas, n_steps, NULL, 0, B, K, known,
                         weight, beta, NULL, NULL, NULL, out, NULL, s) != MDT_ERR_INVALID_ARG ||
        !strstr(mdt_last_error(), "mdt_sample_steer") || !strstr(mdt_last_error(), "kind")) {
        fprintf(stderr, "an unknown kind was not refused by name: %s\n", mdt_last_error());
        return 4;
    }
    /* ... and the steered Heun call: Python's default parameters (no churn: no noise rows), no bounds, no record */
    CHECK(mdt_sample_steer(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, MDT_SAMPLER_HEUN, NULL, sigmas, n_steps, NULL, 0, B, K, known,
                           weight, beta, NULL, NULL, NULL, out, NULL, s));
    HIPCHECK(hipStreamSynchronize(s));
    float* h = (float*)malloc(nact * sizeof(float));
    if (!h) return 1;
    HIPCHECK(hipMemcpy(h, out, nact * sizeof(float), hipMemcpyDeviceToHost));
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(h, sizeof(float), nact, o) != nact) return 1;
    fclose(o);
    printf("steered heun: %d observations, %d candidates each, %d steps, beta %g, %s\n", B, K, n_steps, beta, mdt_version());
    CHECK(mdt_destroy(m));
    return 0;
}
