/*
 * A plain-C host program that runs the other samplers through the C ABI alone (mdt_sample / mdt_sample_dev): what a C / C++
 * robot controller would do to sample with heun, euler_ancestral, ... -- no Python, no torch in the process.
 *
 *   sampler_client <blob> <out>
 * blob (little endian): int32 n_cfg_fields(19) | 19 x int32 mdt_config fields | float sigma_data |
 *   int32 n_params | per parameter: int32 name_len, name bytes, int64 numel, numel x float |
 *   int32 B, int32 n_steps, (n_steps+1) x float sigmas | tokens | goal | x_T |
 *   int32 kind | int32 has_params, then (has_params) 6 x float {eta, s_churn, s_tmin, s_tmax, s_noise, r} + int32 order |
 *   int32 n_noise | n_noise * B*Ta*A floats (the noise rows, in the Python loop's draw order)
 * out: B*Ta*A floats from mdt_sample (host schedule), then B*Ta*A floats from mdt_sample_dev (the schedule in device memory).
 * has_params == 0 passes params = NULL (the Python defaults).  The noise buffer is hipMalloc'ed here.
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
    if (argc != 3) { fprintf(stderr, "usage: sampler_client <blob> <out>\n"); return 1; }
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
    int32_t B = 0, n_steps = 0;
    float sigmas[MDT_SAMPLER_MAX_STEPS + 1];
    if (rd(f, &B, 4) || rd(f, &n_steps, 4) || n_steps < 1 || n_steps > MDT_SAMPLER_MAX_STEPS ||
        rd(f, sigmas, 4 * (n_steps + 1))) return 1;
    const int n_tok = cfg.arch == MDT_ARCH_MDTV ? cfg.n_obs_token : 1;
    const size_t ntok = (size_t)B * n_tok * cfg.obs_dim, ngoal = (size_t)B * cfg.goal_dim;
    const size_t nact = (size_t)B * cfg.action_seq_len * cfg.action_dim;
    float* tok = to_device(f, ntok);
    float* tok2 = cfg.arch == MDT_ARCH_MDT ? to_device(f, ntok) : NULL;
    float* goal = to_device(f, ngoal);
    float* xT = to_device(f, nact);
    int32_t kind = 0, has_params = 0, n_noise = 0;
    mdt_sampler_params prm;
    memset(&prm, 0, sizeof prm);
    if (!tok || !goal || !xT || rd(f, &kind, 4) || rd(f, &has_params, 4)) return 1;
    if (has_params && (rd(f, &prm.eta, 4) || rd(f, &prm.s_churn, 4) || rd(f, &prm.s_tmin, 4) || rd(f, &prm.s_tmax, 4) ||
                       rd(f, &prm.s_noise, 4) || rd(f, &prm.r, 4) || rd(f, &prm.order, 4))) return 1;
    if (rd(f, &n_noise, 4) || n_noise < 0) return 1;
    float* noise = n_noise ? to_device(f, (size_t)n_noise * nact) : NULL;
    fclose(f);
    if (n_noise && !noise) return 1;
    /* the plan on the host first (no GPU work): how many rows this call reads */
    mdt_sampler_plan_t* plan = (mdt_sampler_plan_t*)malloc(sizeof(mdt_sampler_plan_t));
    if (!plan) return 1;
    CHECK(mdt_sampler_plan(kind, has_params ? &prm : NULL, sigmas, n_steps, plan));
    float *out = NULL, *out_dev = NULL, *sig_dev = NULL;  /* two allocations: every data pointer must be 16-byte aligned */
    HIPCHECK(hipMalloc((void**)&out, nact * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&out_dev, nact * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&sig_dev, (n_steps + 1) * sizeof(float)));
    HIPCHECK(hipMemcpy(sig_dev, sigmas, (n_steps + 1) * sizeof(float), hipMemcpyHostToDevice));
    CHECK(mdt_sample(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, kind, has_params ? &prm : NULL, sigmas, n_steps, noise, n_noise,
                     B, out, NULL, s));
    CHECK(mdt_sample_dev(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, kind, has_params ? &prm : NULL, sig_dev, n_steps, noise,
                         n_noise, B, out_dev, NULL, s));
    HIPCHECK(hipStreamSynchronize(s));
    float* h = (float*)malloc(2 * nact * sizeof(float));
    if (!h) return 1;
    HIPCHECK(hipMemcpy(h, out, nact * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(h + nact, out_dev, nact * sizeof(float), hipMemcpyDeviceToHost));
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(h, sizeof(float), 2 * nact, o) != 2 * nact) return 1;
    fclose(o);
    printf("sampler kind %d: %d chunks, %d steps, %d evaluations, %d noise rows, %s\n", kind, B, n_steps, plan->n_evals,
           plan->n_noise, mdt_version());
    CHECK(mdt_destroy(m));
    return 0;
}
