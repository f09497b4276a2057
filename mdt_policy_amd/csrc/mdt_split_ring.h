// mdt_split_ring.h -- the split SCHEMES, the ORDER RULE of their products, the weight-fragment ring of the split launches and the
// product loop on it (mdt_mlp_split.h: the fused MLP and the LayerNorm-prologue products; mdt_tiles.h: the output projection inside
// attn_xattn_tile).  DESIGN.md section 5a.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdt_device.h"   // mdt_bf16x8 / mdt_f16x8, MDT_SPLIT_*

#include <type_traits>

// ---- the split SCHEME of every split body (template parameter SCH) ----
//   MDT_SPLIT_BF16X3  three bf16 parts per operand, six products per k32 step, 6 bytes per weight (mdt_mlp_split.h's header);
//   MDT_SPLIT_F16X2   the PAIR form: two fp16 parts of the SCALED operand (mdt_device.h split2_f16: 22 significand bits), THREE
//                     v_mfma_f32_16x16x32_f16 products per k32 step (x2 w1, x1 w2, x1 w1), 4 bytes per weight -- half the matrix-pipe
//                     clocks and two thirds of the weight stream, the two co-limits of these launches.  One power-of-two scale per
//                     activation row (LayerNorm prologue: a wave reduction; hidden slice: an LDS maximum written before the barrier
//                     that separates the products anyway) and one per 16-column weight tile (made by the pack kernel); the epilogue
//                     undoes both with one v_ldexp_f32 per value before bias, activation and gate.
// Pair image of an (N, K) weight: column tile nt = K / 32 steps x 2 parts x 1 KiB fragments (lane / slot order as above) followed by
// a 16-byte trailer {fp32 scale, 0, 0, 0}: tile stride K / 32 * 2048 + 16 bytes, image size 4 N K + N bytes.
// parts per operand.  (A function of the scheme for the LDS-size helpers of mdt_mlp_split.h: their values have to reach the kernels as
// calls that the optimizer folds -- as constants of the front end they move mlp_split_tile's LDS addresses and its schedule.)
__host__ __device__ constexpr int split_parts(int sch) { return sch == MDT_SPLIT_F16X2 ? 2 : 3; }
template <int SCH> struct split_scheme {
    static constexpr int P = split_parts(SCH);
    static constexpr int FRAG = P * 1024;                                    // bytes of one (column tile, k32 step)
    static constexpr int TRAILER = SCH == MDT_SPLIT_F16X2 ? 16 : 0;          // bytes behind a column tile's fragments
    using frag_t = std::conditional_t<SCH == MDT_SPLIT_F16X2, mdt_f16x8, mdt_bf16x8>;
    __host__ __device__ static constexpr int64_t tile_stride(int K32) { return (int64_t)K32 * FRAG + TRAILER; }
};
// exponent of column tile nt's scale (pair images)
__device__ __forceinline__ int pair_tile_exp(const char* image, int64_t tile_stride, int nt) {
    const unsigned b = __float_as_uint(*(const float*)(image + (nt + 1) * tile_stride - 16));
    return (int)((b >> 23) & 255u) - 127;
}

// ring of R k32 steps x NT column tiles x P parts of weight fragments.  Fragment (j, kk, p) of the wave sits at byte
// base + j * tile_stride + (kk * P + p) * 1024 of the image, lane l's 16 bytes at l * 16.  BUFFER loads (resource = the image, one
// 32-bit per-lane offset per column tile, the step / part offset in the scalar operand): a global_load sends 64 x 8 bytes of address
// through the SIMD's register read path, 33 clocks of matrix-pipe time against 17.7 (mdt_tiles.h WStream) -- and the bf16 form
// requests 1.5x the fragments of the fp32 one per step.
template <int NT, int R, int SCH = MDT_SPLIT_BF16X3>
struct SplitRing {
    static constexpr int P = split_scheme<SCH>::P;
    using frag_t = typename split_scheme<SCH>::frag_t;
    frag_t w[R][NT][P];
    __amdgpu_buffer_rsrc_t rs;
    unsigned voff[NT];
    __device__ __forceinline__ void open(const void* image, int64_t first_byte, int64_t tile_stride, int lane) {
        rs = __builtin_amdgcn_make_buffer_rsrc((void*)image, 0, 0xffffffffu, 0x00020000);
#pragma unroll
        for (int j = 0; j < NT; ++j) voff[j] = (unsigned)(first_byte + j * tile_stride) + 16u * (unsigned)lane;
    }
    __device__ __forceinline__ void request(int slot, int kk) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int p = 0; p < P; ++p)
                w[slot][j][p] = __builtin_bit_cast(frag_t, __builtin_amdgcn_raw_buffer_load_b128(rs, voff[j], (kk * P + p) * 1024, 0));
    }
};

// ---- the products of a k32 step: the ORDER RULE of every split body, written here once ----
// An operand is the sum of its P parts, part 0 the largest.  The products of a k32 step run SMALLEST FIRST: for activation part
// q = P - 1 .. 0, weight parts wp = P - 1 - q .. 0 are multiplied against it (q + wp < P: six products of three bf16 parts, three
// of two fp16 parts), column tiles outside row tiles, so that a dependent MFMA sits at least two issue slots behind its producer.
// Part q of the NEXT step is then read into the same registers, right behind its last use -- no second operand set is ever live --
// with a sched_barrier(0x6) on each side of the reload: left alone, hipcc sinks the LDS reads to the end of the step (mdt_tiles.h
// MDT_SCHED_PIN; spelled as the builtin here, this header comes first).
// split_phase below is the rule as a loop, for every body that streams its weights through a SplitRing.  Two bodies keep it written
// out by hand, instruction schedule and all: gemm_ws_split_tile (mdt_ws.h: weights in register arrays, its own loads behind the
// reloads) and k_gemm_tn_split (mdt_train_kernels.hip: both operands whole in registers, no reloads) -- as loops they compile to
// other schedules (profiles/split_step_isa.txt).
template <int SCH>
__device__ __forceinline__ f32x4 split_mfma(const typename split_scheme<SCH>::frag_t& a, const typename split_scheme<SCH>::frag_t& b,
                                            const f32x4& acc) {
    if constexpr (SCH == MDT_SPLIT_F16X2) return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
// one product phase: acc[i][j] += sum over K32 k32 steps on MT 16-row tiles x NT column tiles.  Ring slots 0 .. R - 2 hold steps
// 0 .. R - 2 on entry (requested by the caller, early); activations from the split tile at `xa` (row stride rowb, part stride part,
// bytes; MFMA slot order, mdt_device.h split_slot)
template <int NT, int K32, int R, int SCH, int MT>
__device__ __forceinline__ void split_phase(SplitRing<NT, R, SCH>& ring, const char* xa, int rowb, int part, int lane, f32x4 (&acc)[MT][NT]) {
    constexpr int P = split_scheme<SCH>::P;
    using frag_t = typename split_scheme<SCH>::frag_t;
    const int aoff = (lane & 15) * rowb + (lane >> 4) * 16;
    frag_t x[P][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int q = 0; q < P; ++q) x[q][i] = *(const frag_t*)(xa + aoff + i * 16 * rowb + q * part);
#pragma unroll
    for (int kk = 0; kk < K32; ++kk) {
        const int u = kk % R;
        if (kk + R - 1 < K32) ring.request((kk + R - 1) % R, kk + R - 1);
        const char* pn = xa + aoff + (kk + 1) * 64;
        __builtin_amdgcn_sched_barrier(0x6);
#pragma unroll
        for (int q = P - 1; q >= 0; --q) {
#pragma unroll
            for (int wp = P - 1 - q; wp >= 0; --wp)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int i = 0; i < MT; ++i) acc[i][j] = split_mfma<SCH>(ring.w[u][j][wp], x[q][i], acc[i][j]);
            __builtin_amdgcn_sched_barrier(0x6);
            if (kk + 1 < K32) {
#pragma unroll
                for (int i = 0; i < MT; ++i) x[q][i] = *(const frag_t*)(pn + i * 16 * rowb + q * part);
            }
            __builtin_amdgcn_sched_barrier(0x6);
        }
    }
}
