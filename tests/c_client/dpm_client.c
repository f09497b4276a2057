/*
 * A plain-C host program that runs DPM-Solver-fast (mdt_sample / mdt_sample_dev with MDT_SAMPLER_DPM_FAST) and the adaptive
 * DPM-Solver (mdt_sample_dpm_adaptive) through the C ABI alone: the schedule is the two levels {sigma_max, sigma_min}, n_steps the evaluation count.
 *
 *   dpm_client <blob> <out>
 * blob (little endian): int32 n_cfg_fields(19) | 19 x int32 mdt_config fields | float sigma_data |
 *   int32 n_params | per parameter: int32 name_len, name bytes, int64 numel, numel x float |
 *   int32 B, int32 n_evals, float sigma_max, float sigma_min | tokens | goal | x_T | float eta, float s_noise |
 *   int32 n_noise | n_noise * B*Ta*A floats (the noise_sampler values, in the Python loop's order) |
 *   int32 order, 7 x double {rtol, atol, h_init, pcoeff, icoeff, dcoeff, accept_safety} (mdt_sample_dpm_adaptive, eta = 0)
 * out: B*Ta*A floats from mdt_sample (host levels), then B*Ta*A floats from mdt_sample_dev (the levels in device memory), then
 *   B*Ta*A floats from mdt_sample_dpm_adaptive over the same levels and its 4 x int32 info {steps, nfe, n_accept, n_reject}.
 */
#include <hip/hip_runtime_api.h>
#include <math.h>
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
    if (argc != 3) { fprintf(stderr, "usage: dpm_client <blob> <out>\n"); return 1; }
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
    float sigmas[2];
    if (rd(f, &B, 4) || rd(f, &n_steps, 4) || n_steps < 1 || n_steps > MDT_SAMPLER_MAX_EVALS || rd(f, sigmas, 8)) return 1;
    const int n_tok = cfg.arch == MDT_ARCH_MDTV ? cfg.n_obs_token : 1;
    const size_t ntok = (size_t)B * n_tok * cfg.obs_dim, ngoal = (size_t)B * cfg.goal_dim;
    const size_t nact = (size_t)B * cfg.action_seq_len * cfg.action_dim;
    float* tok = to_device(f, ntok);
    float* tok2 = cfg.arch == MDT_ARCH_MDT ? to_device(f, ntok) : NULL;
    float* goal = to_device(f, ngoal);
    float* xT = to_device(f, nact);
    int32_t n_noise = 0;
    const int32_t kind = MDT_SAMPLER_DPM_FAST;
    mdt_sampler_params prm;
    memset(&prm, 0, sizeof prm);
    prm.s_tmax = INFINITY; prm.r = 0.5f; prm.order = 4;  /* not read by dpm_fast */
    if (!tok || !goal || !xT || rd(f, &prm.eta, 4) || rd(f, &prm.s_noise, 4)) return 1;
    if (rd(f, &n_noise, 4) || n_noise < 0) return 1;
    float* noise = n_noise ? to_device(f, (size_t)n_noise * nact) : NULL;
    if (n_noise && !noise) return 1;
    mdt_dpm_adaptive_params ap;
    memset(&ap, 0, sizeof ap);
    if (rd(f, &ap.order, 4) || rd(f, &ap.rtol, 8) || rd(f, &ap.atol, 8) || rd(f, &ap.h_init, 8) || rd(f, &ap.pcoeff, 8) ||
        rd(f, &ap.icoeff, 8) || rd(f, &ap.dcoeff, 8) || rd(f, &ap.accept_safety, 8)) return 1;
    fclose(f);
    /* the plan on the host first (no GPU work): how many rows this call reads */
    mdt_sampler_plan_t* plan = (mdt_sampler_plan_t*)malloc(sizeof(mdt_sampler_plan_t));
    if (!plan) return 1;
    CHECK(mdt_sampler_plan(kind, &prm, sigmas, n_steps, plan));
    float *out = NULL, *out_dev = NULL, *sig_dev = NULL;  /* two allocations: every data pointer must be 16-byte aligned */
    HIPCHECK(hipMalloc((void**)&out, nact * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&out_dev, nact * sizeof(float)));
    HIPCHECK(hipMalloc((void**)&sig_dev, 2 * sizeof(float)));
    HIPCHECK(hipMemcpy(sig_dev, sigmas, 2 * sizeof(float), hipMemcpyHostToDevice));
    CHECK(mdt_sample(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, kind, &prm, sigmas, n_steps, noise, n_noise,
                     B, out, NULL, s));
    CHECK(mdt_sample_dev(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, kind, &prm, sig_dev, n_steps, noise,
                         n_noise, B, out_dev, NULL, s));
    float* out_ad = NULL;
    HIPCHECK(hipMalloc((void**)&out_ad, nact * sizeof(float)));
    mdt_dpm_adaptive_info info;
    CHECK(mdt_sample_dpm_adaptive(m, tok, tok2, goal, MDT_MODALITY_LANG, xT, sigmas[1], sigmas[0], &ap, B, out_ad, NULL, &info, s));
    HIPCHECK(hipStreamSynchronize(s));
    float* h = (float*)malloc(3 * nact * sizeof(float));
    if (!h) return 1;
    HIPCHECK(hipMemcpy(h, out, nact * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(h + nact, out_dev, nact * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(h + 2 * nact, out_ad, nact * sizeof(float), hipMemcpyDeviceToHost));
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(h, sizeof(float), 3 * nact, o) != 3 * nact || fwrite(&info, sizeof info, 1, o) != 1) return 1;
    fclose(o);
    printf("dpm_adaptive: %d steps, %d evaluations, %d accepted, %d rejected\n", info.steps, info.nfe, info.n_accept,
           info.n_reject);
    printf("dpm_fast: %d chunks, %d evaluations, %d noise rows, %s\n", B, plan->n_evals, plan->n_noise, mdt_version());
    CHECK(mdt_destroy(m));
    return 0;
}
