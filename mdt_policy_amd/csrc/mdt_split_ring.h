// mdt_split_ring.h -- the split SCHEMES and the weight-fragment ring of the split launches (mdt_mlp_split.h: the fused MLP and the
// LayerNorm-prologue products; mdt_tiles.h: the output projection inside attn_xattn_tile).  DESIGN.md section 5a.
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
template <int SCH> struct split_scheme {
    static constexpr int P = SCH == MDT_SPLIT_F16X2 ? 2 : 3;                 // parts per operand
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

// ring of R k32 steps x NT column tiles x 3 parts of weight fragments.  Fragment (j, kk, p) of the wave sits at byte
// base + j * tile_stride + (kk * 3 + p) * 1024 of the image, lane l's 16 bytes at l * 16.  BUFFER loads (resource = the image, one
// 32-bit per-lane offset per column tile, the step / part offset in the scalar operand): a global_load sends 64 x 8 bytes of address
// through the SIMD's register read path, 33 clocks of matrix-pipe time against 17.7 (mdt_tiles.h WStream) -- and this form requests
// 1.5x the fragments of the fp32 one per step.
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

// one product phase on ONE 16-row tile (pair form; attn_xattn_tile's output projection): acc[j] += sum over K32 k32 steps.  Ring
// slots 0 .. R - 2 hold steps 0 .. R - 2 on entry; activations from the two-part tile at `xa` (row stride rowb, part stride part;
// MFMA slot order, mdt_device.h split_slot).  The three products of a step smallest first, pinned as in split_phase (mdt_mlp_split.h).
template <int NT, int K32, int R>
__device__ __forceinline__ void split_phase_one(SplitRing<NT, R, MDT_SPLIT_F16X2>& ring, const char* xa, int rowb, int part, int lane,
                                                f32x4 (&acc)[NT]) {
    const char* q = xa + (lane & 15) * rowb + (lane >> 4) * 16;
    mdt_f16x8 x1 = *(const mdt_f16x8*)q, x2 = *(const mdt_f16x8*)(q + part);
#pragma unroll
    for (int kk = 0; kk < K32; ++kk) {
        const int u = kk % R, un = (kk + R - 1) % R;
        const bool nx = kk + 1 < K32;
        if (kk + R - 1 < K32) ring.request(un, kk + R - 1);
        const char* p0 = q + (kk + 1) * 64;
        __builtin_amdgcn_sched_barrier(0x6);
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring.w[u][j][0], x2, acc[j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0x6);
        if (nx) x2 = *(const mdt_f16x8*)(p0 + part);
        __builtin_amdgcn_sched_barrier(0x6);
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring.w[u][j][1], x1, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring.w[u][j][0], x1, acc[j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0x6);
        if (nx) x1 = *(const mdt_f16x8*)p0;
        __builtin_amdgcn_sched_barrier(0x6);
    }
}
