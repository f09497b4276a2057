// mdt_mlp_split.h -- the fused MLP launch (mdt_tiles.h mlp_tile) and the LayerNorm-prologue product in their SPLIT forms.  Template
// parameter SCH (mdt_split_ring.h split_scheme): the THREE-WAY bf16 split, or the TWO-WAY fp16 PAIR split
// of scaled operands that the model's launches take (5a (i)).
//
// Same work per workgroup as mlp_tile -- row tile `by` (32 rows) x hidden slice `s` (512 of the 4 D hidden columns):
//   x + gate * (act(prologue(x) W1^T + b1) W2^T + b2),  partial slab s of the second product to parts + s * part_stride --
// with every contraction as P (P + 1) / 2 products of operand parts per k32 step (x = x1 + .. + xP, w = w1 + .. + wP; order and
// schedule: split_phase, mdt_split_ring.h; fp32 accumulation) instead of eight v_mfma_f32_16x16x4_f32: six
// v_mfma_f32_16x16x32_bf16 (fp32's product accuracy, mdt_ws.h) = 96 matrix-pipe clocks per k32 step and accumulator instead of 256,
// or three v_mfma_f32_16x16x32_f16 (22 significand bits after the row / tile scales) = 48.
//
// Where the operands come from:
//   weights     PRE-SPLIT images (k_pack_weight_split / k_pack_weight_pair: made wherever the fp32 fragment image is made --
//               mdt_load_param(s), i.e. also after every optimizer step): fragment (column tile nt, k32 step kk, part p) = 1 KiB at
//               nt * tile_stride + (kk P + p) 1024, lane l's 16 bytes = the part's eight values of
//               W[16 nt + l % 16][32 kk + 16 h + 4 (l / 16) + e], slot 4 h + e; pair images end each column tile with its scale
//               (mdt_split_ring.h).  A wave streams its fragments L2 -> registers as mlp_tile does (SplitRing, two k32 steps):
//               bf16 x 3 is 1.5x the bytes of the fp32 image in a third of the matrix-pipe time -- 49 B per clock and CU of the
//               vector memory path's 64 at full rate (fp32: 14); tools/micro/mlp_split_probe.hip measured the two phases with this
//               traffic at 31 us against k_mlp's 52-58.  The pair form streams the fp32 image's bytes.
//   activations the LayerNorm (+ modulate) prologue of mlp_tile (gemm_stage_tile) stores its rows as their split, in the MFMA slot
//               order of mdt_ws.h (one ds_read_b128 per part, row tile and k32 step); pair form: one power-of-two scale per row;
//   hidden      the activation epilogue of the first product splits its values on the way into LDS, same slot order (pair form:
//               scaled by the row's maximum over the 512-wide slice, gathered in LDS in front of the barrier).
// LDS: split x tile P x 32 x (2 D + 32) B, overlaid after the first product by the split hidden slice P x 32 x 1056 B: 101 KB for
// three parts, 67.6 KB + 256 B of row scales and maxima for two (D <= 512 either way).
// No wave skew here (mlp_tile's flags): the hidden slice overlays the x tile, so the two products are separated by barriers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdt_device.h"
#include "mdt_internal.h"
#include "mdt_tiles.h"
#include "mdt_ws.h"

// (the split schemes, the weight-fragment ring SplitRing and the product loop split_phase: mdt_split_ring.h, which mdt_tiles.h includes)

// LDS bytes of mlp_split_tile at model width D (pair form: two parts -- 67.6 KB for D <= 512 -- + the rows' 32 scale exponents of
// the first product and the 32 maxima of the hidden rows)
__host__ __device__ constexpr int mlp_split_lds_bytes(int D, int sch = MDT_SPLIT_BF16X3) {
    const int P = split_parts(sch);
    const int xs = P * 32 * (2 * D + 32), hs = P * 32 * (2 * 512 + 32);
    return (xs > hs ? xs : hs) + (sch == MDT_SPLIT_F16X2 ? 256 : 0);
}

template <int NTW2, int PRO, int SCH = MDT_SPLIT_BF16X3>
__device__ __forceinline__ void mlp_split_tile(const mdt_gemm_args& f, const mdt_gemm_args& p, const char* __restrict__ w1s,
                                               const char* __restrict__ w2s, float* __restrict__ parts, int64_t part_stride, int by,
                                               int s, char* lds, const float* __restrict__ zeros, int tid) {
    constexpr int MTILES = 2, NWAVES = 8, MT = 32, HS = 512, NTW1 = 4, R = 2;
    constexpr int D = 128 * NTW2, K32a = D / 32, K32b = HS / 32;
    constexpr int ROWB1 = 2 * D + 32, PART1 = MT * ROWB1, ROWB2 = 2 * HS + 32, PART2 = MT * ROWB2;
    static_assert(NTW2 >= 1 && NTW2 <= 4, "D <= 512");
    using SS = split_scheme<SCH>;
    constexpr bool PAIR = SCH == MDT_SPLIT_F16X2;
    constexpr int FRAG = SS::FRAG;
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int lane = tid & 63, wave = tid >> 6;
    const int m0 = by * MT;
    const int nq = 4 * (lane >> 4);
    char* xs = lds;                                   // split x tile: P parts x [32][ROWB1]
    char* hs = lds;                                   // split hidden slice: P parts x [32][ROWB2] (after the first product)
    // pair form, behind both tiles: ordered bits of the hidden rows' largest |value|, scale exponents of the x rows
    unsigned* hmax = (unsigned*)(lds + mlp_split_lds_bytes(D, SCH) - 256);
    int* xexp = (int*)(hmax + 32);
    if constexpr (PAIR) {
        if (tid < 32) hmax[tid] = 0u;                 // (the barrier behind the prologue orders this before the first maximum)
    }

    // ---- first product's operands: the ring's first step and the bias travel under the prologue ----
    const int nt1 = (s * NWAVES + wave) * NTW1;       // hidden column tiles of this wave (global)
    SplitRing<NTW1, R, SCH> ring1;
    ring1.open(w1s, nt1 * SS::tile_stride(K32a), SS::tile_stride(K32a), lane);
#pragma unroll
    for (int u = 0; u < R - 1; ++u) ring1.request(u, u);
    f32x4 b1[NTW1];
    {
        const float* bp = f.bias != nullptr ? f.bias : zeros;
#pragma unroll
        for (int j = 0; j < NTW1; ++j) b1[j] = ldg4(bp + (nt1 + j) * 16 + nq);
    }
    // LayerNorm (+ modulate) of the tile's rows, stored as their split in MFMA slot order
    gemm_stage_tile<MTILES, NWAVES, PRO, false, 1, 2, SCH>(f, (float*)xs, ROWB1, m0, 0, D, zeros, tid, lane, wave, nullptr, xexp);
    __syncthreads();
    f32x4 acc1[MTILES][NTW1];
#pragma unroll
    for (int i = 0; i < MTILES; ++i)
#pragma unroll
        for (int j = 0; j < NTW1; ++j) acc1[i][j] = zero4;
    split_phase<NTW1, K32a, R, SCH>(ring1, xs, ROWB1, PART1, lane, acc1);

    // ---- second product's operands, requested before the activation epilogue so that they travel while it runs: the first
    //      fragments of W2's K slice [512 s, 512 s + 512), then bias / gate / residual rows of the output tile ----
    const int K32p = p.K >> 5;                        // k32 steps of the whole second product (4 D / 32)
    SplitRing<NTW2, R, SCH> ring2;
    ring2.open(w2s, (wave * NTW2) * SS::tile_stride(K32p) + (int64_t)s * K32b * FRAG, SS::tile_stride(K32p), lane);
#pragma unroll
    for (int u = 0; u < R - 1; ++u) ring2.request(u, u);
    // (d = 512, four column tiles per wave: gate and residual rows are requested behind the second product instead -- 64 registers
    //  the product's ring and accumulators need, 116 bytes of scratch otherwise)
    constexpr bool EARLY = NTW2 <= 3;
    f32x4 acc2[MTILES][NTW2], b2[NTW2], gate_v[MTILES][NTW2], res_v[MTILES][NTW2];
    int ncol[NTW2];
#pragma unroll
    for (int j = 0; j < NTW2; ++j) ncol[j] = (wave * NTW2 + j) * 16 + nq;
    const bool gated = p.mod != nullptr && p.gate_off >= 0;
    auto load_gate_res = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < MTILES; ++i) {
            const int64_t m = min(m0 + i * 16 + (lane & 15), f.M - 1);
            const float* gp = gated ? p.mod + p.gate_off + (p.mod_stride == 0 ? 0 : (m / p.rows_per_sample) * p.mod_stride)
                                    : zeros;
            const float* rp = s == 0 ? f.A + m * f.lda : zeros;  // slab 0 carries the residual stream
#pragma unroll
            for (int j = 0; j < NTW2; ++j) {
                gate_v[i][j] = ldg4(gp + ncol[j]);
                res_v[i][j] = ldg4(rp + ncol[j]);
            }
        }
    };
    {
        const float* bp = (s == 0 && p.bias != nullptr) ? p.bias : zeros;
#pragma unroll
        for (int j = 0; j < NTW2; ++j) b2[j] = ldg4(bp + ncol[j]);
#pragma unroll
        for (int i = 0; i < MTILES; ++i)
#pragma unroll
            for (int j = 0; j < NTW2; ++j) acc2[i][j] = zero4;
        if constexpr (EARLY) load_gate_res();
    }
    int he[MTILES] = {0, 0};                          // (pair) scale exponents of the lane's two hidden rows
    if constexpr (PAIR) {
        // activation in place, each hidden row's largest |value| over the 512-wide slice into LDS BEFORE the barrier
        int et1[NTW1];
#pragma unroll
        for (int j = 0; j < NTW1; ++j) et1[j] = pair_tile_exp(w1s, SS::tile_stride(K32a), nt1 + j);
#pragma unroll
        for (int i = 0; i < MTILES; ++i) {
            const int xe = xexp[i * 16 + (lane & 15)];
            unsigned mx = 0u;
#pragma unroll
            for (int j = 0; j < NTW1; ++j) {
                acc1[i][j] = apply_act(pair_unscale(acc1[i][j], xe + et1[j]) + b1[j], f.act);
                mx = max(mx, pair_absbits4(acc1[i][j]));
            }
            atomicMax(&hmax[i * 16 + (lane & 15)], mx);
        }
    }
    __syncthreads();                                  // everybody has read the x tile: the hidden slice overwrites it
    // ---- activation epilogue of the first product -> split hidden slice (lane holds hidden[16 i + lane % 16][tile * 16 + nq .. + 3]) ----
#pragma unroll
    for (int i = 0; i < MTILES; ++i)
#pragma unroll
        for (int j = 0; j < NTW1; ++j) {
            char* q = hs + split_slot(i * 16 + (lane & 15), (wave * NTW1 + j) * 16 + nq, ROWB2);
            if constexpr (PAIR) {
                const unsigned mx = hmax[i * 16 + (lane & 15)];
                he[i] = pair_scale_exp(mx);
                store_split<SCH>(q, PART2, acc1[i][j], pair_scale(mx));
            } else {
                store_split<SCH>(q, PART2, apply_act(acc1[i][j] + b1[j], f.act));
            }
        }
    __syncthreads();
    split_phase<NTW2, K32b, R, SCH>(ring2, hs, ROWB2, PART2, lane, acc2);

    if constexpr (!EARLY) load_gate_res();
    float* out = parts + (int64_t)s * part_stride;
#pragma unroll
    for (int i = 0; i < MTILES; ++i) {
        const int m = m0 + i * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < NTW2; ++j) {
            f32x4 v = acc2[i][j];
            if constexpr (PAIR) v = pair_unscale(v, he[i] + pair_tile_exp(w2s, SS::tile_stride(K32p), wave * NTW2 + j));
            v = v + b2[j];
            v = res_v[i][j] + (gated ? gate_v[i][j] * v : v);
            if (m < f.M) st4(out + (int64_t)m * p.ldo + ncol[j], v);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The LayerNorm-prologue product on the wide tiles (gemm_tile<2, NTW, 8, PRO, ...>: 32 rows x 8 waves x NTW column tiles, whole K
// staged once) in the split form -- the decoder's qkv products (K = d = 384 -> N = 1152: 25 us a launch, 40 launches a sampler call),
// whose rows are the sum of the fused MLP's slabs (XP > 1: gemm_stage_tile adds them on read, the column-0 tile also leaves the sum
// in a.a_merged).  The first half of mlp_split_tile with a plain epilogue: out = act(product + bias), plain output rows.
// LDS: the split x tile (76.8 KB at D = 384).
// ------------------------------------------------------------------------------------------------
// Pair form (SCH = MDT_SPLIT_F16X2): the image is a.Wp_pair, LDS = the two-part x tile (51.2 KB at D = 384) + the rows' 32 scale exponents.
__host__ __device__ constexpr int gemm_ln_split_lds_bytes(int D, int sch = MDT_SPLIT_BF16X3) {
    return split_parts(sch) * 32 * (2 * D + 32) + (sch == MDT_SPLIT_F16X2 ? 128 : 0);
}
template <int ND, int NTW, int PRO, int XP, int SCH = MDT_SPLIT_BF16X3>
__device__ __forceinline__ void gemm_ln_split_tile(const mdt_gemm_args& a, int by, int bx, char* lds, const float* __restrict__ zeros, int tid) {
    using SS = split_scheme<SCH>;
    constexpr bool PAIR = SCH == MDT_SPLIT_F16X2;
    constexpr int MTILES = 2, NWAVES = 8, MT = 32, R = 2;
    constexpr int D = 128 * ND, K32 = D / 32, ROWB = 2 * D + 32, PART = MT * ROWB;
    static_assert(ND >= 1 && ND <= 4, "D <= 512");
    const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int lane = tid & 63, wave = tid >> 6;
    const int m0 = by * MT, nq = 4 * (lane >> 4);
    char* xs = lds;
    const int nt0 = (bx * NWAVES + wave) * NTW;       // N is a multiple of the panel width: every wave has NTW real column tiles
    SplitRing<NTW, R, SCH> ring;
    const char* image = (const char*)(PAIR ? a.Wp_pair : a.Wp_split);
    int* xexp = (int*)(lds + SS::P * PART);           // (pair) scale exponents of the tile's rows
    ring.open(image, nt0 * SS::tile_stride(K32), SS::tile_stride(K32), lane);
#pragma unroll
    for (int u = 0; u < R - 1; ++u) ring.request(u, u);
    f32x4 bias_v[NTW];
    {
        const float* bp = a.bias != nullptr ? a.bias : zeros;
#pragma unroll
        for (int j = 0; j < NTW; ++j) bias_v[j] = ldg4(bp + (nt0 + j) * 16 + nq);
    }
    gemm_stage_tile<MTILES, NWAVES, PRO, false, XP, (NTW <= 3 && XP <= 3) ? 1 : 2, SCH>(a, (float*)xs, ROWB, m0, 0, D, zeros, tid, lane, wave,
                                                                                        bx == 0 ? a.a_merged : nullptr, xexp);
    __syncthreads();
    f32x4 acc[MTILES][NTW];
#pragma unroll
    for (int i = 0; i < MTILES; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[i][j] = zero4;
    split_phase<NTW, K32, R, SCH>(ring, xs, ROWB, PART, lane, acc);
#pragma unroll
    for (int i = 0; i < MTILES; ++i) {
        const int m = m0 + i * 16 + (lane & 15);
        const int xe = PAIR ? xexp[i * 16 + (lane & 15)] : 0;
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
            f32x4 v = acc[i][j];
            if constexpr (PAIR) v = pair_unscale(v, xe + pair_tile_exp(image, SS::tile_stride(K32), nt0 + j));
            if (m < a.M) st4(a.out + (int64_t)m * a.ldo + (nt0 + j) * 16 + nq, apply_act(v + bias_v[j], a.act));
        }
    }
}
