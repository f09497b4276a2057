// mdt_head_wide.hip -- the action head for action vectors of 17 .. 64 elements: the kernels behind mdt_launch_head once
// a.A > 16 (at most 16 elements keep head_rows of mdt_tiles.h, bit for bit).
//
// One launch does what the narrow head does: decoder LayerNorm (optional bias; none at all for the MLP head's hidden layer,
// a.no_ln) -> action_pred -> EDM combine -> pin -> DDIM step or a sampler plan's update -> the next input's action_emb embedding.
// head_rows keeps a row's action_pred / action_emb fragments of every column in registers of one wave; at 64 columns that is
// over a thousand VGPRs, so here a workgroup of four waves owns a 16-ROW tile and both products are 16 x 16 tiles of
// v_mfma_f32_16x16x4_f32:
//   1  wave w normalises rows 4 w .. 4 w + 3 of the tile (the guided head: of both halves, 8 rows) with head_rows' arithmetic and
//      leaves them in LDS, row stride D16 + 4 floats, columns D .. D16 - 1 zero (D16 = D rounded up to 16: the MLP head's hidden
//      width 100 is no multiple of 16);
//   2  wave w < NT = ceil(A / 16) forms column tile w of action_pred over K = D16: lane l holds, per 16-deep k block, the FOUR
//      consecutive k values 4 (l / 16) .. + 3 of weight row l % 16 (one 16-byte load from the row-major (A, D) image) and of
//      LDS row l % 16 -- the k order inside a block is the same permutation on both operands, so no fragment image of the
//      weights is needed; the fragments are requested eight k blocks at a time, the first group before the LayerNorm, each
//      later one while the group before it is multiplied.  Weight rows past A - 1 and k past D - 4 are clamped addresses: the
//      first give columns that are never stored and are zeroed before the second product, the second meet zeros in LDS;
//   3  the epilogue runs on the accumulator layout (lane l: rows 4 (l / 16) + r, column 16 w + l % 16), every (M, A) operand
//      loaded per element from a clamped address; the plan update is head_plan_elem, the one head_rows calls;
//   4  X' c_in(sigma_next) (the plan head: Y') goes through LDS (16 x (16 NT + 4), columns past A zero) into operand layout and
//      y_next = . Wa^T + ba is the second product, K = 16 NT, the D16 / 16 column tiles dealt to the four waves.
// Rows past a.M are clamped on load (they repeat row M - 1) and never formed as a store address.  y_next may alias y: a
// workgroup reads its own rows only, and has them in LDS before it writes.  No atomics: every output element has one owner.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mdt_internal.h"
#include "mdt_launch.h"
#include "mdt_device.h"
#include "mdt_sampler_plan.h"
#include "mdt_tiles.h"

namespace {

constexpr int HW_THREADS = 256;
constexpr size_t HW_LDS_MAX = 160 * 1024;  // gfx950: 160 KiB of LDS per workgroup

__host__ __device__ constexpr int hw_ceil16(int v) { return (v + 15) & ~15; }

template <int NT, bool PLAN, bool GUIDE>
__global__ __launch_bounds__(HW_THREADS) void k_head_wide(mdt_head_args a, mdt_head_plan pl, mdt_head_pin pn, float lam,
                                                          const float* __restrict__ zeros) {
    extern __shared__ __align__(16) float hw_lds[];
    constexpr int NR = GUIDE ? 32 : 16;   // decoder rows of the tile: the guided head normalises both halves
    constexpr int RPW = NR / 4;           // rows a wave normalises
    constexpr int XS = 16 * NT + 4;       // row stride of the updated tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, j = lane & 15;
    const int D = a.D, A = a.A, M = a.M;
    const int D16 = hw_ceil16(D), xst = D16 + 4, n4 = D >> 2;
    const int base = blockIdx.x * 16;     // < M: the grid is ceil(M / 16)
    float* xn = hw_lds;                   // [NR][xst] normalised rows
    float* xu = xn + NR * xst;            // [16][XS] next input, scaled
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};

    // action_pred fragments of this wave's column tile, requested KC k blocks at a time: the first group travels with the rows
    // of the LayerNorm, each later one while the group before it is multiplied.  Column and k are clamped addresses (a wave
    // beyond the last tile, wave >= NT, reads column A - 1 and multiplies nothing)
    constexpr int KC = 8, KGROUPS = 512 / 16 / KC;
    const int K16 = D16 >> 4;
    const int colv = wave * 16 + j, col = min(colv, A - 1);
    const float* wrow = a.Wp + (int64_t)col * D;
    f32x4 wb[2][KC];
#pragma unroll
    for (int u = 0; u < KC; ++u) wb[0][u] = ldg4(wrow + min(16 * u + 4 * g, D - 4));

    // ---- 1: LayerNorm of the tile's rows (head_rows' arithmetic), every row requested before the first is consumed ----
    {
        int cc[2];
        bool cv[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            cv[p] = lane + 64 * p < n4;
            cc[p] = 4 * min(lane + 64 * p, n4 - 1);
        }
        const float* lnb = a.ln_b != nullptr ? a.ln_b : zeros;
        f32x4 v[RPW][2], w[2], bb[2];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const int lr = wave * RPW + i;  // tile row; lr >= 16: the unconditional half
            const int64_t yrow = (int64_t)min(base + (lr & 15), M - 1) + (int64_t)(lr >> 4) * M;
#pragma unroll
            for (int p = 0; p < 2; ++p) v[i][p] = ldg4(a.y + yrow * D + cc[p]);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            w[p] = ldg4(a.ln_w + cc[p]);
            bb[p] = ldg4(lnb + cc[p]);
        }
        const float inv_d = 1.0f / (float)D;
        float red[RPW];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            red[i] = 0.f;
#pragma unroll
            for (int p = 0; p < 2; ++p) { v[i][p] = sel4(cv[p], v[i][p], zero4); red[i] += hsum4(v[i][p]); }
        }
        wave_sum_n<RPW>(red);
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const float mean = a.no_ln ? 0.f : red[i] * inv_d;
            red[i] = 0.f;
#pragma unroll
            for (int p = 0; p < 2; ++p) { v[i][p] = sel4(cv[p], v[i][p] - mean, zero4); red[i] += hsq4(v[i][p]); }
        }
        wave_sum_n<RPW>(red);
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            const float rstd = 1.0f / sqrtf(red[i] * inv_d + 1e-5f);
            float* dst = xn + (wave * RPW + i) * xst;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                v[i][p] = sel4(cv[p] && !a.no_ln, v[i][p] * rstd * w[p] + bb[p], v[i][p]);
                if (cv[p]) *(f32x4*)(dst + cc[p]) = v[i][p];
            }
            if (lane < (D16 >> 2) - n4) *(f32x4*)(dst + 4 * (n4 + lane)) = zero4;  // reduction padding D .. D16 - 1
        }
    }
    __syncthreads();

    // ---- 2, 3: wave w < NT owns column tile w ----
    float sig_next = 1.f, ratio = 0.f, coef = 0.f;
    if (a.mode == MDT_HEAD_DDIM) {
        ratio = a.step[0];
        coef = a.step[1];
        sig_next = a.step[2];
    }
    if constexpr (PLAN) sig_next = pl.e->sigma_next;
    if (wave < NT) {
        // the element operands travel with the product
        int64_t kel[4];
        bool own[4];
        float xin[4], sigma[4], pkn[4], pkp[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int srow = base + 4 * g + r, rowc = min(srow, M - 1);
            kel[r] = (int64_t)rowc * A + col;
            own[r] = srow < M && colv < A;
            xin[r] = a.x[kel[r]];
            sigma[r] = a.sigma[(int64_t)(rowc / a.rows_per_sample) * a.sigma_stride];
            pkn[r] = 0.f;
            pkp[r] = 0.f;
        }
        if (pn.known != nullptr) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { pkn[r] = pn.known[kel[r]]; pkp[r] = pn.keep[kel[r]]; }
        }
        const float bpv = a.bp[col];
        float blo = 0.f, bhi = 0.f;
        if constexpr (PLAN) {
            if (pl.lo != nullptr) { blo = pl.lo[col]; bhi = pl.hi[col]; }
        }
        const float* arow = xn + j * xst + 4 * g;
        f32x4 acc = zero4, accu = zero4;
#pragma unroll
        for (int c = 0; c < KGROUPS; ++c) {
            if (c * KC < K16) {  // wave-uniform
                if ((c + 1) * KC < K16) {
#pragma unroll
                    for (int u = 0; u < KC; ++u) wb[(c + 1) & 1][u] = ldg4(wrow + min(16 * ((c + 1) * KC + u) + 4 * g, D - 4));
                }
#pragma unroll
                for (int u = 0; u < KC; ++u) {
                    const int kk = c * KC + u;
                    if (kk < K16) {
                        const f32x4 b = wb[c & 1][u];
                        const f32x4 x0 = *(const f32x4*)(arow + 16 * kk);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.x, b.x, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.y, b.y, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.z, b.z, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.w, b.w, acc, 0, 0, 0);
                        if constexpr (GUIDE) {
                            const f32x4 x1 = *(const f32x4*)(arow + 16 * xst + 16 * kk);
                            accu = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.x, b.x, accu, 0, 0, 0);
                            accu = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.y, b.y, accu, 0, 0, 0);
                            accu = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.z, b.z, accu, 0, 0, 0);
                            accu = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.w, b.w, accu, 0, 0, 0);
                        }
                    }
                }
            }
        }
        const float sd = a.sigma_data;
        const float cin_next = edm_c_in(edm_den2_round_sd(sig_next, sd));
        float cx[MDT_SAMPLER_NREG], cy[MDT_SAMPLER_NREG + 1];
        int push = MDT_PUSH_NONE;
        bool clip = false, rec = false;
        int64_t nel = 0;
        const float *n0 = nullptr, *n1 = nullptr;
        if constexpr (PLAN) {
            const mdt_sampler_eval& e = *pl.e;
#pragma unroll
            for (int k = 0; k < MDT_SAMPLER_NREG; ++k) { cx[k] = e.cx[k]; cy[k] = e.cy[k]; }
            cy[MDT_SAMPLER_NREG] = e.cy[MDT_SAMPLER_NREG];
            push = e.push;
            clip = pl.lo != nullptr && e.ends_step != 0;
            rec = pl.rec_x != nullptr && e.begins_step != 0;
            nel = pl.nel;
            const int nn = pl.noise != nullptr ? pl.n_noise : 0;  // rows outside [0, n_noise) read as 0
            n0 = (e.noise[0] >= 0 && e.noise[0] < nn) ? pl.noise + e.noise[0] * nel : nullptr;
            n1 = (e.noise[1] >= 0 && e.noise[1] < nn) ? pl.noise + e.noise[1] * nel : nullptr;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float F;
            if constexpr (GUIDE) {
                const float fg = acc[r] + bpv, fu = accu[r] + bpv;
                F = fu + lam * (fg - fu);  // the network output of the guided denoiser, bias included
            } else {
                F = acc[r] + bpv;
            }
            float o = F;
            if (a.mode != MDT_HEAD_RAW) {
                const float den2 = edm_den2_round_sd(sigma[r], sd);
                const float c_skip = edm_c_skip(sd, den2), c_out = edm_c_out(sigma[r], sd, den2);
                float den = edm_denoised_round_both(F, xin[r], c_out, c_skip);
                if (pn.known != nullptr)  // selects at both ends: no 0 * inf, no sign-of-zero change
                    den = pkp[r] == 0.f ? den : (pkp[r] == 1.f ? pkn[r] : den + pkp[r] * (pkn[r] - den));
                o = a.mode == MDT_HEAD_DDIM ? ratio * xin[r] + coef * den : den;
            }
            float nxt = o;
            if constexpr (PLAN) head_plan_elem(&pl, cx, cy, push, clip, rec, nel, n0, n1, kel[r], xin[r], o, sigma[r], blo, bhi, own[r], o, nxt);
            if (own[r]) a.out[kel[r]] = o;
            xu[(4 * g + r) * XS + colv] = colv < A ? nxt * cin_next : 0.f;
        }
    }
    if (a.y_next == nullptr) return;  // workgroup-uniform
    __syncthreads();

    // ---- 4: the next input's embedding, column tiles nt = wave, wave + 4, .. of D16 / 16 ----
    const float* urow = xu + j * XS + 4 * g;
    for (int nt = wave; nt < (D16 >> 4); nt += 4) {
        const int n = nt * 16 + j, nc = min(n, D - 1);
        const float bias = a.ba[nc];
        f32x4 acc = (f32x4){bias, bias, bias, bias};
        f32x4 b[NT];
#pragma unroll
        for (int kb = 0; kb < NT; ++kb) {
            const int k0 = 16 * kb + 4 * g;
            b[kb].x = a.Wa[(int64_t)min(k0, A - 1) * D + nc];
            b[kb].y = a.Wa[(int64_t)min(k0 + 1, A - 1) * D + nc];
            b[kb].z = a.Wa[(int64_t)min(k0 + 2, A - 1) * D + nc];
            b[kb].w = a.Wa[(int64_t)min(k0 + 3, A - 1) * D + nc];
        }
#pragma unroll
        for (int kb = 0; kb < NT; ++kb) {
            const f32x4 x0 = *(const f32x4*)(urow + 16 * kb);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.x, b[kb].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.y, b[kb].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.z, b[kb].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.w, b[kb].w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int srow = base + 4 * g + r;
            if (srow < M && n < D) {
                a.y_next[(int64_t)srow * D + n] = acc[r];
                if constexpr (GUIDE) a.y_next[((int64_t)srow + M) * D + n] = acc[r];  // the one embedding goes to both halves
            }
        }
    }
}

template <int NT>
hipError_t launch_wide(const mdt_head_args& a, const mdt_head_plan* pl, mdt_guide gd, mdt_head_pin pn, size_t lds, hipStream_t s) {
    const dim3 grid((unsigned)((a.M + 15) / 16)), block(HW_THREADS);
    const float* zeros = mdt_zeros();
    if (zeros == nullptr) return hipErrorOutOfMemory;
    const mdt_head_plan none = {};
    if (gd.on && pl) return mdt_launch_lds<k_head_wide<NT, true, true>>(grid, block, lds, s, a, *pl, pn, gd.lam, zeros);
    if (gd.on) return mdt_launch_lds<k_head_wide<NT, false, true>>(grid, block, lds, s, a, none, pn, gd.lam, zeros);
    if (pl) return mdt_launch_lds<k_head_wide<NT, true, false>>(grid, block, lds, s, a, *pl, pn, 1.f, zeros);
    return mdt_launch_lds<k_head_wide<NT, false, false>>(grid, block, lds, s, a, none, pn, 1.f, zeros);
}

}  // namespace

// bytes of dynamic LDS of one workgroup: the normalised rows (16, the guided head 32) and the updated 16 x A16 tile
size_t mdt_head_wide_lds(int D, int A, bool guided) {
    return sizeof(float) * ((size_t)(guided ? 32 : 16) * (hw_ceil16(D) + 4) + (size_t)16 * (hw_ceil16(A) + 4));
}

// the one place the head's shape and LDS size are checked: a refusal enqueues nothing
hipError_t mdt_launch_head_wide(const mdt_head_args& a, const mdt_head_plan* pl, mdt_guide gd, hipStream_t s, mdt_head_pin pn) {
    if (a.A <= 16 || a.A > 64 || a.M < 1 || a.D < 4 || a.D % 4 || a.D > 512 || a.y_parts > 1 || a.x == nullptr) return hipErrorInvalidValue;
    const size_t lds = mdt_head_wide_lds(a.D, a.A, gd.on);
    if (lds > HW_LDS_MAX) return hipErrorInvalidValue;
    return mdt_with_const<2, 4>((a.A + 15) / 16, [&](auto c) { return launch_wide<decltype(c)::value>(a, pl, gd, pn, lds, s); });
}
