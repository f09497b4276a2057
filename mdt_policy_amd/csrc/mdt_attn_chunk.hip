// mdt_attn_chunk.hip -- softmax attention of action chunks of 17 .. 64 rows: the three kernels behind mdt_launch_attention,
// mdt_launch_attn_fwd_train and mdt_launch_attn_bwd once max(Tq, Tk) > 16 (at most 16 rows keep their own kernels, bit for bit).
//
// Shapes: Tq, Tk <= 64, head dim 32 / 48 / 64 -- the decoder's causal self-attention (Tq = Tk = Ta), the encoder's
// non-causal one (Tq = Tk = Te) and the decoder's explicit cross-attention (Tq = Ta, Tk = Te; the causal mask is top-left
// aligned, so a query row i >= Tk sees every key and no query sees a key j >= Tq).
// The visible prefix (Tv): a causal launch whose keys j >= Tv = min(Tq, Tk) no query sees stages, sizes its LDS by and multiplies
// the first Tv keys only.  Tk stays the K / V sample stride (b * Tk rows) and the row length of the dropout index
// ((b H + h) Tq + i) Tk + j; the backward writes dk / dv rows Tv .. Tk-1 as zeros (accumulate_kv: leaves them as they are).
// One workgroup of four waves per (sample, head); wave w owns the 16-row QUERY tile w.  Everything is 16 x 16 tiles of
// v_mfma_f32_16x16x4_f32 on fp32 operands staged in LDS, modelled on k_attn_mid_fwd2 / k_attn_mid_bwd (mdt_mae.hip):
//   forward   scores TRANSPOSED (keys as the row operand, queries as the column operand), so that the accumulator of key tile tj,
//             acc[tj][r] = S[query 16 ti + m][key 16 tj + 4 g + r], is lane for lane the A fragment of P V: the softmax (and the
//             dropout multipliers) stay in registers.  Causal: key tiles above the diagonal are skipped (wave uniform), the
//             diagonal tile is masked per element.  V sits transposed in LDS.
//   backward  P is recomputed the same way, dP = dO V^T beside it; (m P) and dS = P (m dP - delta) scale go through two
//             Tq16 x Tv16 LDS matrices once, then dQ = dS K, dV = (m P)^T dO and dK = dS^T Q are row tiles dealt to the waves.
//             RoPE is rotated back on the accumulators (a pair's two columns sit in neighbouring lanes).
// Rows / keys past Tq / Tv inside the last tile are zero in LDS and masked in the softmax; their addresses are never formed.
// No atomics: every output element has one owner, results repeat bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mdt_internal.h"
#include "mdt_launch.h"
#include "mdt_device.h"

namespace {

constexpr int CHUNK_T = 64;          // largest Tq / Tk
constexpr int CHUNK_TILES = CHUNK_T / 16;
constexpr int CHUNK_NT = 256;        // four waves: one per query tile
constexpr int CHUNK_ROT = 32;        // rotary dims (position_embeddings.py / transformer_blocks.py:108)
constexpr float LOG2E = 1.44269504088896341f;

__device__ __forceinline__ f32x4 rope4(f32x4 v, const float* __restrict__ rc, const float* __restrict__ rs, int t, int c4, float sign) {
    // columns 4 c4 .. + 3 of a head's row at position t: rotary pairs 2 c4 and 2 c4 + 1 (tables: 16 frequencies per position)
    const float c0 = rc[t * 16 + 2 * c4], s0 = sign * rs[t * 16 + 2 * c4];
    const float c1 = rc[t * 16 + 2 * c4 + 1], s1 = sign * rs[t * 16 + 2 * c4 + 1];
    return (f32x4){v.x * c0 - v.y * s0, v.y * c0 + v.x * s0, v.z * c1 - v.w * s1, v.w * c1 + v.z * s1};
}

// T rows of one head's HD columns (row r at src + r * ld) -> LDS rows of HD + 4 floats, or (TRANS) columns of a [HD][vs] matrix;
// rows T .. T16-1 are zero (reduction padding of the MFMA products; never an address).  rc != nullptr: rotated by the row's position.
// Four loads per thread are requested from clamped rows before the first is consumed.
// Item i -> (row t, float4 column c): row major for the row layout (a wave reads whole rows); for TRANS 16 consecutive lanes take
// 16 consecutive rows of one column and the next 16 lanes the next column, so that a wave's four-byte stores of one feature go to
// 64 different banks (the column pitch 4 vs is 16 banks for every vs = Tv16 + 4) while a row still gives 64 contiguous bytes.
template <int H4, bool TRANS>
__device__ __forceinline__ void stage_item(int i, int& t, int& c) {
    if (TRANS) {
        const int j = i >> 4, th = j / H4;
        c = j - th * H4;
        t = 16 * th + (i & 15);
    } else {
        t = i / H4;
        c = i - t * H4;
    }
}
template <int HD, bool TRANS>
__device__ __forceinline__ void stage_rows(const float* __restrict__ src, int64_t ld, int T, int T16, float* dst, int vs,
                                           const float* __restrict__ rc, const float* __restrict__ rs, int tid) {
    constexpr int H4 = HD / 4, ST = HD + 4, U = 4;
    const int n = T16 * H4;
    for (int i0 = tid; i0 < n; i0 += CHUNK_NT * U) {
        f32x4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int t, c;
            stage_item<H4, TRANS>(min(i0 + u * CHUNK_NT, n - 1), t, c);
            v[u] = ldg4(src + (int64_t)min(t, T - 1) * ld + 4 * c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + u * CHUNK_NT;
            int t, c;
            stage_item<H4, TRANS>(min(i, n - 1), t, c);
            if (i < n) {
                f32x4 x = v[u];
                if (rc && 4 * c < CHUNK_ROT) x = rope4(x, rc, rs, min(t, T - 1), c, 1.f);
                if (t >= T) x = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (TRANS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) dst[(4 * c + e) * vs + t] = x[e];
                } else {
                    *(f32x4*)(dst + t * ST + 4 * c) = x;
                }
            }
        }
    }
}

// acc[r] = sum over the head's HD features of A[row 4 g + r][f] * B[row m][f]: a_rows / b_rows are the 16-row tiles in LDS (stride
// HD + 4); the lane reads its own row m of BOTH (the MFMA's row operand is a_rows, its column operand b_rows)
template <int HD>
__device__ __forceinline__ f32x4 tile_dot(const float* a_rows, const f32x4 (&bv)[HD / 16], int m, int g) {
    constexpr int ST = HD + 4, C16 = HD / 16;
    const float* ap = a_rows + m * ST + 4 * g;
    f32x4 av[C16];
#pragma unroll
    for (int c = 0; c < C16; ++c) av[c] = *(const f32x4*)(ap + 16 * c);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < C16; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c][e], bv[c][e], acc, 0, 0, 0);
    return acc;
}

// dropout multipliers of elements idx0 .. idx0 + 3 of a site (any alignment): word idx & 3 of Philox block idx >> 2, the mapping of
// attn_dropout_table (mdt_train_kernels.hip) -- one block when idx0 is a multiple of 4, else two
__device__ __forceinline__ f32x4 dropout_run4(uint64_t seed, uint32_t site, uint64_t idx0, float p) {
    const philox4_t r0 = philox4(seed, site, idx0 >> 2);
    const unsigned sh = (unsigned)idx0 & 3u;
    philox4_t r1 = r0;
    if (sh) r1 = philox4(seed, site, (idx0 >> 2) + 1);
    f32x4 out;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned w = sh + r;   // 0 .. 6
        const uint32_t word = w == 0 ? r0.w[0] : w == 1 ? r0.w[1] : w == 2 ? r0.w[2] : w == 3 ? r0.w[3] : w == 4 ? r1.w[0] : w == 5 ? r1.w[1] : r1.w[2];
        out[r] = dropout_keep(word, p);
    }
    return out;
}

// The probabilities of query tile ti in registers: pr[tj][r] = P[query 16 ti + m][key 16 tj + 4 g + r], NORMALISED iff NORM
// (else the caller scales its output rows by *inv).  qv: the lane's query row fragments.  Key tiles tj >= nkv are not computed
// (pr = 0).  sl2 = log2 e / sqrt(hd): the softmax runs in base 2.
template <int HD, bool NORM>
__device__ __forceinline__ void chunk_probs(const f32x4 (&qv)[HD / 16], const float* ks, int nkv, int qi, int Tk, bool causal, float sl2,
                                            int m, int g, f32x4 (&pr)[CHUNK_TILES], float* inv) {
    constexpr int ST = HD + 4;
    float mx = -INFINITY;
#pragma unroll
    for (int tj = 0; tj < CHUNK_TILES; ++tj) {
        pr[tj] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (tj < nkv) {
            pr[tj] = tile_dot<HD>(ks + 16 * tj * ST, qv, m, g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * tj + 4 * g + r;
                const bool vis = j < Tk && (!causal || j <= qi);
                pr[tj][r] = vis ? pr[tj][r] * sl2 : -INFINITY;
                mx = fmaxf(mx, pr[tj][r]);
            }
        }
    }
    mx = xrow_max(mx);   // key 0 is visible to every query: finite
    float sum = 0.f;
#pragma unroll
    for (int tj = 0; tj < CHUNK_TILES; ++tj) {
        if (tj < nkv) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pr[tj][r] = __builtin_amdgcn_exp2f(pr[tj][r] - mx);   // 2^(-inf) = 0 for masked keys
                sum += pr[tj][r];
            }
        }
    }
    const float iv = 1.0f / xrow_sum(sum);
    if (NORM) {
#pragma unroll
        for (int tj = 0; tj < CHUNK_TILES; ++tj) pr[tj] = pr[tj] * iv;
    }
    *inv = iv;
}

struct chunk_fwd_args {
    const float* q; int64_t ldq;
    const float* k; const float* v; int64_t ldkv;
    float* out; int64_t ldo;
    int32_t H, Tq, Tk, causal, ctx_div;
    int32_t Tv;                         // keys staged and multiplied (<= Tk; keys Tv .. Tk-1 are ones no query sees)
    const float *rc, *rs;               // rotary tables or nullptr
    float p; uint32_t site; uint64_t seed;
};

// forward (inference and training): out = (mask / (1 - p) * softmax(q k^T / sqrt(hd))) v
template <int HD, bool DROP>
__global__ __launch_bounds__(CHUNK_NT) void k_attn_chunk_fwd(chunk_fwd_args a, float sl2) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ST = HD + 4, C16 = HD / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, g = lane >> 4;
    const int b = blockIdx.x, h = blockIdx.y, bkv = a.ctx_div > 1 ? b / a.ctx_div : b;
    const int Tq = a.Tq, Tk = a.Tk, Tv = a.Tv, Tq16 = (Tq + 15) & ~15, Tv16 = (Tv + 15) & ~15, nq = Tq16 >> 4, nk = Tv16 >> 4, VS = Tv16 + 4;
    float* qs = lds;                 // [Tq16][ST]
    float* ks = qs + Tq16 * ST;      // [Tv16][ST]
    float* vt = ks + Tv16 * ST;      // [HD][VS]: V transposed
    stage_rows<HD, false>(a.q + (int64_t)b * Tq * a.ldq + h * HD, a.ldq, Tq, Tq16, qs, 0, a.rc, a.rs, tid);
    stage_rows<HD, false>(a.k + (int64_t)bkv * Tk * a.ldkv + h * HD, a.ldkv, Tv, Tv16, ks, 0, a.rc, a.rs, tid);
    stage_rows<HD, true>(a.v + (int64_t)bkv * Tk * a.ldkv + h * HD, a.ldkv, Tv, Tv16, vt, VS, nullptr, nullptr, tid);
    __syncthreads();
    const int ti = wave;
    if (ti >= nq) return;   // (no barrier below)
    const int qi = 16 * ti + m;                              // the lane's query; rows >= Tq are zero and never stored
    const int nkv = a.causal ? min(nk, ti + 1) : nk;         // key tiles this query tile sees
    f32x4 qv[C16];
#pragma unroll
    for (int c = 0; c < C16; ++c) qv[c] = *(const f32x4*)(qs + qi * ST + 16 * c + 4 * g);
    f32x4 pr[CHUNK_TILES];
    float inv;
    chunk_probs<HD, false>(qv, ks, nkv, qi, Tv, a.causal != 0, sl2, m, g, pr, &inv);
    if (DROP) {
        const uint64_t base = (((uint64_t)b * a.H + h) * Tq + min(qi, Tq - 1)) * Tk;
#pragma unroll
        for (int tj = 0; tj < CHUNK_TILES; ++tj)
            if (tj < nkv) pr[tj] = pr[tj] * dropout_run4(a.seed, a.site, base + 16 * tj + 4 * g, a.p);
    }
    // O[query 4 g + r][d = 16 c + m] = sum_key P[query][key] V[key][d]: the probabilities ARE the A fragments
    f32x4 o[C16];
#pragma unroll
    for (int c = 0; c < C16; ++c) o[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tj = 0; tj < CHUNK_TILES; ++tj) {
        if (tj < nkv) {
#pragma unroll
            for (int c = 0; c < C16; ++c) {
                const f32x4 vv = *(const f32x4*)(vt + (16 * c + m) * VS + 16 * tj + 4 * g);   // lane = (d, keys 4 g .. + 3)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[tj][e], vv[e], o[c], 0, 0, 0);
            }
        }
    }
    float* op = a.out + (int64_t)b * Tq * a.ldo + h * HD + m;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float ir = __shfl(inv, 4 * g + r, 64);   // the normaliser of output row 4 g + r lives in column 4 g + r
        const int row = 16 * ti + 4 * g + r;
        if (row < Tq) {
#pragma unroll
            for (int c = 0; c < C16; ++c) op[(int64_t)row * a.ldo + 16 * c] = o[c][r] * ir;
        }
    }
}

// One 16-row tile of C[i][d] = sum_k W(i, k) x[k][d] over n reduction tiles of 16: W(i, k) = S[i][k] (TRANS = false) or S[k][i]
// (true), S in LDS with row stride ss, x rows in LDS with stride HD + 4; acc[q][r] = C[16 ti + 4 g + r][16 q + m]
template <int HD, bool TRANS>
__device__ __forceinline__ void rows_tile(const float* S, int ss, const float* x, int n, int ti, int m, int g, f32x4 (&acc)[HD / 16]) {
    constexpr int ST = HD + 4, NC = HD / 16;
#pragma unroll
    for (int q = 0; q < NC; ++q) acc[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const float* sp = TRANS ? S + (4 * g) * ss + 16 * ti + m : S + (16 * ti + m) * ss + 4 * g;
    const float* xp = x + (4 * g) * ST + m;
    for (int c = 0; c < n; ++c) {
        f32x4 w;
        if (TRANS) { const float* t = sp + 16 * c * ss; w = (f32x4){t[0], t[ss], t[2 * ss], t[3 * ss]}; }
        else w = *(const f32x4*)(sp + 16 * c);
        f32x4 xv[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const float* r = xp + 16 * c * ST + 16 * q;
            xv[q] = (f32x4){r[0], r[ST], r[2 * ST], r[3 * ST]};
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < NC; ++q) acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[e], xv[q][e], acc[q], 0, 0, 0);
    }
}

// rows 16 ti + 4 g + r (< T) of such a tile -> dst (row stride ld): rc != nullptr rotates the gradient of a ROTATED row back (the
// transpose of the forward's rotation; a pair's columns 2 i, 2 i + 1 sit in lanes m, m ^ 1), acc: dst +=
template <int HD>
__device__ __forceinline__ void store_tile(f32x4 (&v)[HD / 16], float* dst, int64_t ld, int T, int ti, int m, int g,
                                           const float* __restrict__ rc, const float* __restrict__ rs, bool acc) {
    constexpr int NC = HD / 16;
    if (rc) {
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            if (16 * q < CHUNK_ROT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = min(16 * ti + 4 * g + r, T - 1), pi = (16 * q + m) >> 1;
                    const float other = __shfl_xor(v[q][r], 1, 64);
                    const float c = rc[t * 16 + pi], s = rs[t * 16 + pi];
                    v[q][r] = (m & 1) ? v[q][r] * c - other * s : v[q][r] * c + other * s;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * ti + 4 * g + r;
        if (row < T) {
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                float* p = dst + (int64_t)row * ld + 16 * q + m;
                *p = acc ? *p + v[q][r] : v[q][r];
            }
        }
    }
}

// backward: P is recomputed from q, k (nothing but the forward's inputs is read); dQ, dK, dV each written by one owner
template <int HD, bool DROP>
__global__ __launch_bounds__(CHUNK_NT) void k_attn_chunk_bwd(mdt_attn_bwd_args a, float scale, int Tv) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ST = HD + 4, C16 = HD / 16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, g = lane >> 4;
    const int b = blockIdx.x, h = blockIdx.y;
    const int Tq = a.Tq, Tk = a.Tk, Tq16 = (Tq + 15) & ~15, Tv16 = (Tv + 15) & ~15, nq = Tq16 >> 4, nk = Tv16 >> 4, SS = Tv16 + 4;
    float* qs = lds;                  // [Tq16][ST] (rotated)
    float* ks = qs + Tq16 * ST;       // [Tv16][ST] (rotated)
    float* vs = ks + Tv16 * ST;       // [Tv16][ST]
    float* os = vs + Tv16 * ST;       // [Tq16][ST]: dO
    float* Pm = os + Tq16 * ST;       // [Tq16][SS]: what multiplied V in the forward
    float* dS = Pm + Tq16 * SS;       // [Tq16][SS]
    const float* rc = a.rope ? a.rope_cos : nullptr;
    const float* rs = a.rope ? a.rope_sin : nullptr;
    stage_rows<HD, false>(a.q + (int64_t)b * Tq * a.ldq + h * HD, a.ldq, Tq, Tq16, qs, 0, rc, rs, tid);
    stage_rows<HD, false>(a.k + (int64_t)b * Tk * a.ldkv + h * HD, a.ldkv, Tv, Tv16, ks, 0, rc, rs, tid);
    stage_rows<HD, false>(a.v + (int64_t)b * Tk * a.ldkv + h * HD, a.ldkv, Tv, Tv16, vs, 0, nullptr, nullptr, tid);
    stage_rows<HD, false>(a.d_out + (int64_t)b * Tq * a.ld_do + h * HD, a.ld_do, Tq, Tq16, os, 0, nullptr, nullptr, tid);
    __syncthreads();
    if (wave < nq) {
        const int ti = wave, qi = 16 * ti + m;
        const int nkv = a.causal ? min(nk, ti + 1) : nk;
        f32x4 qv[C16], dv[C16];
#pragma unroll
        for (int c = 0; c < C16; ++c) {
            qv[c] = *(const f32x4*)(qs + qi * ST + 16 * c + 4 * g);
            dv[c] = *(const f32x4*)(os + qi * ST + 16 * c + 4 * g);
        }
        f32x4 pr[CHUNK_TILES], dp[CHUNK_TILES], mk[CHUNK_TILES];
        float inv;
        chunk_probs<HD, true>(qv, ks, nkv, qi, Tv, a.causal != 0, scale * LOG2E, m, g, pr, &inv);
        const uint64_t base = (((uint64_t)b * a.H + h) * Tq + min(qi, Tq - 1)) * Tk;
        float part = 0.f;
#pragma unroll
        for (int tj = 0; tj < CHUNK_TILES; ++tj) {
            dp[tj] = (f32x4){0.f, 0.f, 0.f, 0.f};
            mk[tj] = (f32x4){1.f, 1.f, 1.f, 1.f};
            if (tj < nkv) {
                dp[tj] = tile_dot<HD>(vs + 16 * tj * ST, dv, m, g);   // dP[query m][keys 4 g + r] = dO[m] . V[key]
                if (DROP) mk[tj] = dropout_run4(a.seed, a.site, base + 16 * tj + 4 * g, a.p);
                dp[tj] = dp[tj] * mk[tj];                             // out = (m P) V  =>  dP = m (dO V^T)
#pragma unroll
                for (int r = 0; r < 4; ++r) part = fmaf(pr[tj][r], dp[tj][r], part);
            }
        }
        const float delta = xrow_sum(part);
        const bool live = qi < Tq;
#pragma unroll
        for (int tj = 0; tj < CHUNK_TILES; ++tj) {
            if (tj < nk) {   // skipped key tiles: zeros (they are reduction padding below)
                f32x4 pm = {0.f, 0.f, 0.f, 0.f}, ds = {0.f, 0.f, 0.f, 0.f};
                if (tj < nkv && live) {
                    pm = pr[tj] * mk[tj];
#pragma unroll
                    for (int r = 0; r < 4; ++r) ds[r] = pr[tj][r] * (dp[tj][r] - delta) * scale;
                }
                *(f32x4*)(Pm + qi * SS + 16 * tj + 4 * g) = pm;
                *(f32x4*)(dS + qi * SS + 16 * tj + 4 * g) = ds;
            }
        }
    }
    __syncthreads();
    // the keys no query sees (rows Tv .. Tk-1 of dk and dv): zeros, each float4 written by one thread
    if (Tv < Tk && !a.accumulate_kv) {
        constexpr int H4 = HD / 4;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < (Tk - Tv) * H4; i += CHUNK_NT) {
            const int64_t off = ((int64_t)b * Tk + Tv + i / H4) * a.ld_dkv + h * HD + 4 * (i % H4);
            *(f32x4*)(a.dk + off) = z;
            *(f32x4*)(a.dv + off) = z;
        }
    }
    // row tiles dealt to the waves: dQ = dS K (nq tiles), dV = (m P)^T dO and dK = dS^T Q (nk tiles each)
    for (int it = wave; it < nq + 2 * nk; it += CHUNK_NT / 64) {
        f32x4 acc[C16];
        if (it < nq) {
            rows_tile<HD, false>(dS, SS, ks, nk, it, m, g, acc);
            store_tile<HD>(acc, a.dq + (int64_t)b * Tq * a.ld_dq + h * HD, a.ld_dq, Tq, it, m, g, rc, rs, false);
        } else if (it < nq + nk) {
            rows_tile<HD, true>(Pm, SS, os, nq, it - nq, m, g, acc);
            store_tile<HD>(acc, a.dv + (int64_t)b * Tk * a.ld_dkv + h * HD, a.ld_dkv, Tv, it - nq, m, g, nullptr, nullptr, a.accumulate_kv != 0);
        } else {
            rows_tile<HD, true>(dS, SS, qs, nq, it - nq - nk, m, g, acc);
            store_tile<HD>(acc, a.dk + (int64_t)b * Tk * a.ld_dkv + h * HD, a.ld_dkv, Tv, it - nq - nk, m, g, rc, rs, a.accumulate_kv != 0);
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int prefix_of(int Tk, int kv_rows) { return kv_rows > 0 ? kv_rows : Tk; }   // keys staged: kv_rows = 0 means every key

template <int HD>
hipError_t launch_fwd(const chunk_fwd_args& a, int B, hipStream_t s) {
    const size_t lds = mdt_attn_chunk_lds(HD, a.Tq, a.Tv, false);
    const float sl2 = LOG2E / sqrtf((float)HD);
    if (a.p > 0.f && a.seed != 0) return mdt_launch_lds<k_attn_chunk_fwd<HD, true>>(dim3(B, a.H), dim3(CHUNK_NT), lds, s, a, sl2);
    return mdt_launch_lds<k_attn_chunk_fwd<HD, false>>(dim3(B, a.H), dim3(CHUNK_NT), lds, s, a, sl2);
}

hipError_t chunk_fwd(const chunk_fwd_args& a, int B, int hd, hipStream_t s) {
    if (!mdt_attn_chunk_supported(hd, a.Tq, a.Tk) || B < 1 || a.H < 1 || a.H > 65535 || a.ctx_div < 1) return hipErrorInvalidValue;
    if (!mdt_prefix_rows_ok(a.Tq, a.Tk, a.causal, a.Tv)) return hipErrorInvalidValue;
    if (((a.ldq | a.ldkv | a.ldo) & 3) || !aligned16(a.q) || !aligned16(a.k) || !aligned16(a.v) || !aligned16(a.out)) return hipErrorInvalidValue;
    if (mdt_attn_chunk_lds(hd, a.Tq, a.Tv, false) > 160 * 1024) return hipErrorInvalidValue;
    switch (hd) {
        case 32: return launch_fwd<32>(a, B, s);
        case 48: return launch_fwd<48>(a, B, s);
        default: return launch_fwd<64>(a, B, s);
    }
}

template <int HD>
hipError_t launch_bwd(const mdt_attn_bwd_args& a, const mdt_attn_train_route& r, hipStream_t s) {
    const float scale = 1.0f / sqrtf((float)HD);
    if (r.drop) return mdt_launch_lds<k_attn_chunk_bwd<HD, true>>(dim3(a.B, r.gy), dim3(r.threads), r.lds, s, a, scale, r.Tv);
    return mdt_launch_lds<k_attn_chunk_bwd<HD, false>>(dim3(a.B, r.gy), dim3(r.threads), r.lds, s, a, scale, r.Tv);
}

}  // namespace

static_assert(CHUNK_T == MDT_ATTN_CHUNK_T && CHUNK_NT == 256, "mdt_route_train.h: the chunk kernels' row limit and workgroup size");

// test hook (mdt_hip_debug.h)
extern "C" int64_t mdt_op_attn_chunk_lds(int32_t hd, int32_t Tq, int32_t kv_rows, int32_t bwd) {
    return (int64_t)mdt_attn_chunk_lds(hd, Tq, kv_rows, bwd != 0);
}

hipError_t mdt_launch_attn_chunk(const mdt_attn_args& a, const float* rope_cos, const float* rope_sin, hipStream_t s, int ctx_div, int kv_rows) {
    if (a.rope && (!rope_cos || !rope_sin)) return hipErrorInvalidValue;
    chunk_fwd_args f;
    memset(&f, 0, sizeof f);
    f.q = a.q; f.ldq = a.ldq; f.k = a.k; f.v = a.v; f.ldkv = a.ldkv; f.out = a.out; f.ldo = a.ldo;
    f.H = a.H; f.Tq = a.Tq; f.Tk = a.Tk; f.causal = a.causal; f.ctx_div = ctx_div; f.Tv = prefix_of(a.Tk, kv_rows);
    f.rc = a.rope ? rope_cos : nullptr; f.rs = a.rope ? rope_sin : nullptr;
    return chunk_fwd(f, a.B, a.hd, s);
}

// the training launches: mdt_launch_attn_fwd_train / mdt_launch_attn_bwd (mdt_train_kernels.hip) have checked the operands and
// hand over their route (mdt_route_train.h: family CHUNK -- shape, prefix and LDS bytes accepted)
hipError_t mdt_launch_attn_chunk_fwd_train(const mdt_attn_train_args& a, const mdt_attn_train_route& r, hipStream_t s) {
    if (a.B < 1) return hipErrorInvalidValue;
    chunk_fwd_args f;
    memset(&f, 0, sizeof f);
    f.q = a.q; f.ldq = a.ldq; f.k = a.k; f.v = a.v; f.ldkv = a.ldkv; f.out = a.out; f.ldo = a.ldo;
    f.H = a.H; f.Tq = a.Tq; f.Tk = a.Tk; f.causal = a.causal; f.ctx_div = 1; f.Tv = r.Tv;
    f.rc = a.rope ? a.rope_cos : nullptr; f.rs = a.rope ? a.rope_sin : nullptr;
    f.p = a.p; f.site = a.site; f.seed = a.seed;
    switch (r.hd) {
        case 32: return launch_fwd<32>(f, a.B, s);
        case 48: return launch_fwd<48>(f, a.B, s);
        default: return launch_fwd<64>(f, a.B, s);
    }
}

hipError_t mdt_launch_attn_chunk_bwd(const mdt_attn_bwd_args& a, const mdt_attn_train_route& r, hipStream_t s) {
    if (a.B < 1) return hipErrorInvalidValue;
    switch (r.hd) {
        case 32: return launch_bwd<32>(a, r, s);
        case 48: return launch_bwd<48>(a, r, s);
        default: return launch_bwd<64>(a, r, s);
    }
}
