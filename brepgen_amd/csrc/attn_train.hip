// Attention core for TRAINING: forward that keeps the row log-sum-exp, dropout on the probabilities, and the backward
// (dQ, dK, dV) -- the differentiable form of attn.hip's bg_attn_fwd (same packed qkv layout, same key-padding mask), with an explicit
// score scale because a trainable module holds nn.MultiheadAttention's raw in_proj_weight.
//
//   forward   S = scale q k^T (+ -inf on padded keys), P = softmax(S), lse = max + log(sum) (before dropout),
//             O = (P o M / (1 - p)) V                       M = keep mask, see keep_nibble below
//   backward  P = exp(S - lse) recomputed in fp32,  delta_i = sum_j P~_ij dP_ij (= sum_d dO_id O_id, summed the way torch's softmax
//             backward sums it: exact cancellation in dS when a row has one key, and independent of the rounding of O),
//             dV = (P o M / (1-p))^T dO,  dP = (dO V^T) o M / (1-p),  dS = P o (dP - delta),  dQ = scale dS K,  dK = scale dS^T Q
//
// 16-bit kernels (bf16 / fp16 operands into v_mfma_f32_32x32x16, fp32 accumulation), all on the tile convention, the staging and the
// fragment reads of attn_tile.h; the short backward also on its element step, hi + lo split and store, of which the forward and the
// general backward keep their own text where a helper changed their instruction stream (listed in attn_tile.h):
//   * scores are computed with the WALKED index on the accumulator registers and the OWNED index on the lane
//     (forward and dQ: a wave owns 32 queries and walks the keys, S^T = K Q^T; dK/dV: a wave owns 32 keys and walks the queries,
//     S = Q K^T), so whatever belongs to the owned row -- running max and sum, lse, delta, the key's padding flag -- is lane-local;
//   * the 32 x 32 fp32 tile (P^T, dS^T, P, dS) is fed straight back as the B operand of the next product, which sums over the
//     walked index; the A operand is the transposed LDS image of the walked tile, read in the k order the registers already have.
//   Backward, general path (any N), is two launches: dQ (workgroup = 128 queries of one (sample, head), walks the key tiles twice: delta first -- left in
//   the workspace for the second launch -- then dS and dQ) and dK/dV (workgroup = 128 keys of one (sample, head), walks the query
//   tiles).  S and dP are computed three times, and dS and P~ enter dQ, dK and dV as hi + lo 16-bit pairs (one 16-bit rounding of them
//   costs as much accuracy as the result's own rounding): twelve MFMA products instead of five, and in exchange the error stays at
//   torch's fp32-math level and no sum ever crosses a workgroup -- no atomics, no [N, N] tensor, every output element
//   has ONE writer and a fixed summation order, so results repeat bit for bit and a sample's gradients depend on its rows alone.
//   Backward, N <= 64 (the face trainers): one launch, one workgroup per (sample, head), nothing recomputed (at_bwd16_short_kernel);
//   measured faster than the general path at N = 30, 50 and 64 (profiles/r13/attn_bwd_bench.json), so BG_ATTN_BWD_AUTO takes it.
// fp32 kernels: VALU restatement (one wave per owned row, fp64 accumulation), the parity mode of the 16-bit path -- not a performance path.
#include "attn_tile.h"
#include "philox.h"

namespace bg {

constexpr uint32_t AT_TAG = 0xAD700000u;       // Philox domain tag of the dropout mask (philox.h lists the tags in use)
constexpr int AT_SHORT_AUTO_N = 64;            // BG_ATTN_BWD_AUTO: 16-bit sequences up to this length take the one-launch kernel
constexpr int AT_MAX_N_DROP = 65536;           // the counter holds the query in 16 bits and the 4-key block in 16 bits

// ---- the dropout mask: a pure function of (seed, draw_id, GLOBAL sample, head, query, key) ----
// One Philox4x32-10 block = the four words of keys 4 kb .. 4 kb + 3 of one query:
//   counter = (query << 16 | kb, low 32 bits of g, draw_id, 0xAD70 << 16 | head << 12 | bits 32..43 of g),   key = seed,
// g = first_sample + b.  Key 4 kb + e is KEPT iff word e >= thr, thr = floor(p 2^32): P(keep) = 1 - thr / 2^32.
struct DropKey {
    uint32_t seed_lo, seed_hi, draw, thr;
    unsigned long long first;
    float rp;                                   // 1 / (1 - p)
};
// bit e of the result: key 4 kb + e of (g, head, q) is kept
__device__ __forceinline__ unsigned keep_nibble(const DropKey& dk, unsigned long long g, int head, int q, int kb) {
    uint32_t c[4] = {((uint32_t)q << 16) | (uint32_t)kb, (uint32_t)g, dk.draw, drop_word3(drop_tag_sub(AT_TAG, (uint32_t)head), g)};
    philox4x32_10(c, dk.seed_lo, dk.seed_hi);
    return (c[0] >= dk.thr ? 1u : 0u) | (c[1] >= dk.thr ? 2u : 0u) | (c[2] >= dk.thr ? 4u : 0u) | (c[3] >= dk.thr ? 8u : 0u);
}

__global__ __launch_bounds__(256) void at_mask_kernel(uint8_t* __restrict__ mask, int B, int N, DropKey dk) {
    const int nkb = (N + 3) >> 2;
    const long long total = (long long)B * BG_N_HEAD * N * nkb;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int kb = (int)(i % nkb);
    const long long row = i / nkb;                       // (b * 12 + head) * N + q
    const int q = (int)(row % N);
    const int head = (int)((row / N) % BG_N_HEAD);
    const long long b = row / N / BG_N_HEAD;
    const unsigned nib = keep_nibble(dk, dk.first + (unsigned long long)b, head, q, kb);
    uint8_t* p = mask + (size_t)row * N + 4 * kb;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (4 * kb + e < N) p[e] = (uint8_t)((nib >> e) & 1u);
}

// ------------------------------------------------------------------------------------------------
// Training forward, 16-bit.  grid (ceil(N / 128), 12, B); a wave owns 32 queries of (b, head) and walks the key tiles of 64.
// ------------------------------------------------------------------------------------------------
template <bool F16, bool DROP>
__global__ __launch_bounds__(256, 2) void at_fwd16_kernel(const void* __restrict__ qkv_, const uint8_t* __restrict__ key_pad,
                                                          void* __restrict__ out_, float* __restrict__ lse, int N, float scale, DropKey dk) {
    using E = Elem<F16>;
    using T = typename E::T;
    using V8 = typename E::V8;
    __shared__ __attribute__((aligned(16))) unsigned char lds[AT_RM + AT_TR + 256];
    unsigned char* kimg = lds;
    T* vtr = reinterpret_cast<T*>(lds + AT_RM);
    float* mb = reinterpret_cast<float*>(lds + AT_RM + AT_TR);       // additive mask bias of the tile's 64 keys
    const T* __restrict__ qkv = reinterpret_cast<const T*>(qkv_);
    T* __restrict__ out = reinterpret_cast<T*>(out_);

    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.z, head = blockIdx.y;
    const int q0 = blockIdx.x * 128 + wave * 32;
    const size_t row_base = (size_t)b * N;
    const T* base = qkv + row_base * QKV_LD + head * 64;
    const int q = q0 + l31;
    const unsigned long long g = dk.first + (unsigned long long)b;

    V8 qf[4];
    at_row_frags<F16>(base + (size_t)(q < N ? q : N - 1) * QKV_LD, h, qf);
    f32x16 o[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    const int nkt = (N + 63) / 64;
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();                                   // previous tile fully consumed
        at_stage<F16, 256, true, false>(base + BG_D_MODEL, QKV_LD, kt * 64, N, kimg, nullptr, tid);
        at_stage<F16, 256, false, true>(base + 2 * BG_D_MODEL, QKV_LD, kt * 64, N, nullptr, vtr, tid);
        if (tid < 64) {
            const int key = kt * 64 + tid;
            const bool dead = key >= N || (key_pad != nullptr && key_pad[row_base + key] != 0);
            mb[tid] = dead ? -INFINITY : 0.f;
        }
        __syncthreads();
        if (q0 >= N) continue;                             // wave-uniform; such a wave only helps to stage
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            if (kt * 64 + sub * 32 >= N) break;            // uniform: sub-tile entirely past the last key
            f32x16 s;
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s = E::mfma(at_frag_rm<F16>(kimg, sub * 32 + l31, ks * 2 + h), qf[ks], s);
            // online-softmax sub-tile, P V accumulate and the store are this kernel's own text (as in attn16_kernel: attn_tile.h)
            float mloc = -INFINITY;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float4 mbv = *reinterpret_cast<const float4*>(&mb[sub * 32 + 8 * g4 + 4 * h]);
                s[4 * g4 + 0] = s[4 * g4 + 0] * scale + mbv.x; s[4 * g4 + 1] = s[4 * g4 + 1] * scale + mbv.y;
                s[4 * g4 + 2] = s[4 * g4 + 2] * scale + mbv.z; s[4 * g4 + 3] = s[4 * g4 + 3] * scale + mbv.w;
                mloc = fmaxf(mloc, fmaxf(fmaxf(s[4 * g4 + 0], s[4 * g4 + 1]), fmaxf(s[4 * g4 + 2], s[4 * g4 + 3])));
            }
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float m_new = fmaxf(m_run, mloc);
            const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
            const float alpha = __expf(m_run - m_use);
            float psum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                s[r] = __expf(s[r] - m_use);
                psum += s[r];
            }
            l_run = l_run * alpha + psum;                  // the normaliser does not see the dropout
            m_run = m_new;
            if (DROP) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const unsigned nib = keep_nibble(dk, g, head, q, (kt * 64 + sub * 32 + at_walked(4 * g4, h)) >> 2);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[4 * g4 + e] = ((nib >> e) & 1u) ? s[4 * g4 + e] : 0.f;
                }
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                V8 pb;
#pragma unroll
                for (int e = 0; e < 8; ++e) pb[e] = (T)s[8 * sl + e];
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    o[dt] = E::mfma(at_frag_tr<F16>(vtr, dt * 32 + l31, sub * 32 + 16 * sl + 4 * h), pb, o[dt]);
            }
        }
    }

    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = l_tot > 0.f ? (DROP ? dk.rp : 1.0f) / l_tot : 0.f;
    if (q < N) {
        if (h == 0) lse[((size_t)b * BG_N_HEAD + head) * N + q] = l_tot > 0.f ? m_run + logf(l_tot) : 0.f;
        T* op = out + (row_base + q) * BG_D_MODEL + head * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *reinterpret_cast<typename E::V4*>(op + dt * 32 + 8 * g4 + 4 * h) =
                    E::pack4(o[dt][4 * g4 + 0] * inv, o[dt][4 * g4 + 1] * inv, o[dt][4 * g4 + 2] * inv, o[dt][4 * g4 + 3] * inv);
    }
}

// ------------------------------------------------------------------------------------------------
// Backward, 16-bit.  grid (ceil(N / 128), 12, B); a wave OWNS 32 rows (lane & 31) and WALKS the other side in tiles of 64.
//   DKV = false (dQ):    owned = queries (X = Q, Y = dO in registers), walked = keys    (A1 = K, A2 = V tiles in LDS)
//                        S^T = A1 X^T, dP^T = A2 Y^T, dQ^T += A1^T dS^T -- in TWO walks: the first one sums delta = rowsum(P~ o dP)
//                        (written to the workspace for the dK/dV kernel), the second one forms dS and dQ
//   DKV = true  (dK/dV): owned = keys    (X = K, Y = V in registers), walked = queries (A1 = Q, A2 = dO tiles in LDS)
//                        S = A1 X^T, dP = A2 Y^T, dV^T += A2^T P~, dK^T += A1^T dS
// ------------------------------------------------------------------------------------------------
template <bool F16, bool DROP, bool DKV>
__global__ __launch_bounds__(256, 2) void at_bwd16_kernel(const void* __restrict__ qkv_, const uint8_t* __restrict__ key_pad,
                                                          const float* __restrict__ lse, float* __restrict__ delta,
                                                          const void* __restrict__ dout_, void* __restrict__ dqkv_, int N, float scale,
                                                          DropKey dk) {
    using E = Elem<F16>;
    using T = typename E::T;
    using V8 = typename E::V8;
    constexpr int LDS_BYTES = 2 * AT_RM + (DKV ? 2 : 1) * AT_TR + 512;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    unsigned char* img1 = lds;
    unsigned char* img2 = lds + AT_RM;
    T* tr1 = reinterpret_cast<T*>(lds + 2 * AT_RM);
    T* tr2 = reinterpret_cast<T*>(lds + 2 * AT_RM + AT_TR);          // DKV only
    float* aux0 = reinterpret_cast<float*>(lds + LDS_BYTES - 512);   // dQ: 1 = dead key;  dK/dV: lse of the walked queries
    float* aux1 = aux0 + 64;                                         //                     dK/dV: delta of the walked queries
    const T* __restrict__ qkv = reinterpret_cast<const T*>(qkv_);
    const T* __restrict__ dout = reinterpret_cast<const T*>(dout_);
    T* __restrict__ dqkv = reinterpret_cast<T*>(dqkv_);

    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.z, head = blockIdx.y;
    const int own0 = blockIdx.x * 128 + wave * 32;
    const int own = own0 + l31, ownc = own < N ? own : N - 1;
    const size_t row_base = (size_t)b * N;
    const T* qb = qkv + row_base * QKV_LD + head * 64;               // Q; K at + 768, V at + 1536
    const T* dob = dout + row_base * BG_D_MODEL + head * 64;
    const float* lse_b = lse + ((size_t)b * BG_N_HEAD + head) * N;
    float* del_b = delta + ((size_t)b * BG_N_HEAD + head) * N;       // written by the dQ kernel, read by the dK/dV kernel
    const unsigned long long g = dk.first + (unsigned long long)b;

    const T* a1 = DKV ? qb : qb + BG_D_MODEL;
    const T* a2 = DKV ? dob : qb + 2 * BG_D_MODEL;
    const int ld2 = DKV ? BG_D_MODEL : QKV_LD;
    // the x / y row fragments (loads interleaved), the element step, the hi + lo split and the store are this kernel's own text: behind
    // attn_tile.h's helpers its instruction stream changed and the dropout instantiations measured slower
    V8 xf[4], yf[4];
    {
        const T* xp = (DKV ? qb + BG_D_MODEL : qb) + (size_t)ownc * QKV_LD;
        const T* yp = DKV ? qb + 2 * BG_D_MODEL + (size_t)ownc * QKV_LD : dob + (size_t)ownc * BG_D_MODEL;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            xf[ks] = *reinterpret_cast<const V8*>(xp + (ks * 2 + h) * 8);
            yf[ks] = *reinterpret_cast<const V8*>(yp + (ks * 2 + h) * 8);
        }
    }
    // what belongs to the owned row
    float lse_o = 0.f, del_o = 0.f;
    bool dead_o = false;
    if (DKV) dead_o = own >= N || (key_pad != nullptr && key_pad[row_base + ownc] != 0);
    else lse_o = lse_b[ownc];
    float dsum = 0.f;                                               // dQ, first walk: the lane's share of delta

    f32x16 acc1[2], acc2[2];                                        // dQ^T | dK^T (d tiles of 32), dV^T
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc1[dt][r] = 0.f; acc2[dt][r] = 0.f; }

    const int nwt = (N + 63) / 64;
    for (int pass = DKV ? 1 : 0; pass < 2; ++pass) {
        const bool sum_delta = !DKV && pass == 0;
        for (int t = 0; t < nwt; ++t) {
            __syncthreads();                                   // previous tile fully consumed
            if (sum_delta) at_stage<F16, 256, true, false>(a1, QKV_LD, t * 64, N, img1, tr1, tid);
            else at_stage<F16, 256, true, true>(a1, QKV_LD, t * 64, N, img1, tr1, tid);
            at_stage<F16, 256, true, DKV>(a2, ld2, t * 64, N, img2, tr2, tid);
            if (tid < 64) {
                const int w = t * 64 + tid;
                if (DKV) {
                    const int wc = w < N ? w : N - 1;
                    aux0[tid] = lse_b[wc];
                    aux1[tid] = del_b[wc];
                } else {
                    aux0[tid] = (w >= N || (key_pad != nullptr && key_pad[row_base + w] != 0)) ? 1.f : 0.f;
                }
            }
            __syncthreads();
            if (own0 >= N) continue;                           // wave-uniform; such a wave only helps to stage
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const int w0 = t * 64 + sub * 32;
                if (w0 >= N) break;                            // uniform: sub-tile entirely past the last row
                f32x16 s, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    s = E::mfma(at_frag_rm<F16>(img1, sub * 32 + l31, ks * 2 + h), xf[ks], s);
                    dp = E::mfma(at_frag_rm<F16>(img2, sub * 32 + l31, ks * 2 + h), yf[ks], dp);
                }
                unsigned keep[4] = {0xFFFFu, 0xFFFFu, 0xFFFFu, 0xFFFFu};   // DKV: keep[e] bit 4 g4 + (lane & 3); dQ: keep[g4] bit e
                if (DROP) {
                    if (DKV) {
                        // a block holds 4 consecutive KEYS of one query: lane j of each quad (4 consecutive keys, one block) draws the
                        // blocks of the quad's queries at_walked(4 g4, h) + j, and the quad exchanges the nibbles
                        unsigned nb = 0;
#pragma unroll
                        for (int g4 = 0; g4 < 4; ++g4)
                            nb |= keep_nibble(dk, g, head, w0 + at_walked(4 * g4, h) + (lane & 3), own >> 2) << (4 * g4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) keep[e] = (unsigned)__shfl((int)nb, (lane & ~3) + e, 64) >> (lane & 3);
                    } else {
#pragma unroll
                        for (int g4 = 0; g4 < 4; ++g4) keep[g4] = keep_nibble(dk, g, head, own, (w0 + at_walked(4 * g4, h)) >> 2);
                    }
                }
                f32x16 pt;                                     // P~ (dK/dV only)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const float4 x0 = *reinterpret_cast<const float4*>(&aux0[sub * 32 + at_walked(4 * g4, h)]);
                    const float4 x1 = *reinterpret_cast<const float4*>(&aux1[sub * 32 + at_walked(4 * g4, h)]);
                    const float v0[4] = {x0.x, x0.y, x0.z, x0.w}, v1[4] = {x1.x, x1.y, x1.z, x1.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int r = 4 * g4 + e;
                        const bool dead = DKV ? (dead_o || w0 + at_walked(r, h) >= N) : (v0[e] != 0.f);
                        const float lse_r = DKV ? v0[e] : lse_o, del_r = DKV ? v1[e] : del_o;
                        const float p = dead ? 0.f : __expf(s[r] * scale - lse_r);
                        float dpv = dp[r], pv = p;
                        if (DROP) {
                            const bool kept = DKV ? ((keep[e] >> (4 * g4)) & 1u) : ((keep[g4] >> e) & 1u);
                            dpv = kept ? dpv * dk.rp : 0.f;
                            pv = kept ? p * dk.rp : 0.f;
                        }
                        pt[r] = pv;
                        if (sum_delta) dsum += dead ? 0.f : p * dpv;
                        s[r] = dead ? 0.f : p * (dpv - del_r);          // dS
                    }
                }
                if (sum_delta) continue;
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    V8 dsb, dsl, ptb, ptl;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        dsb[e] = (T)s[8 * sl + e];
                        dsl[e] = (T)(s[8 * sl + e] - (float)dsb[e]);
                        ptb[e] = (T)pt[8 * sl + e];
                        ptl[e] = (T)(pt[8 * sl + e] - (float)ptb[e]);
                    }
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        at_mfma_hilo<F16>(acc1[dt], at_frag_tr<F16>(tr1, dt * 32 + l31, sub * 32 + 16 * sl + 4 * h), dsb, dsl);
                        if (DKV) at_mfma_hilo<F16>(acc2[dt], at_frag_tr<F16>(tr2, dt * 32 + l31, sub * 32 + 16 * sl + 4 * h), ptb, ptl);
                    }
                }
            }
        }
        if (sum_delta) {                                       // the query's keys are split over lane and lane ^ 32
            del_o = dsum + __shfl_xor(dsum, 32, 64);
            if (own < N && h == 0) del_b[own] = del_o;
        }
    }

    if (own < N) {
        T* op = dqkv + (row_base + own) * QKV_LD + head * 64 + (DKV ? BG_D_MODEL : 0);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d = dt * 32 + 8 * g4 + 4 * h;
                *reinterpret_cast<typename E::V4*>(op + d) = E::pack4(acc1[dt][4 * g4 + 0] * scale, acc1[dt][4 * g4 + 1] * scale,
                                                                      acc1[dt][4 * g4 + 2] * scale, acc1[dt][4 * g4 + 3] * scale);
                if (DKV)
                    *reinterpret_cast<typename E::V4*>(op + BG_D_MODEL + d) =
                        E::pack4(acc2[dt][4 * g4 + 0], acc2[dt][4 * g4 + 1], acc2[dt][4 * g4 + 2], acc2[dt][4 * g4 + 3]);
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Backward, 16-bit, N <= 64 in ONE launch with nothing recomputed: one workgroup = 2 waves = one (sample, head).
//   1. K, V (row-major), K^T, Q^T, dO^T (transposed) of the head are staged once.
//   2. Wave w owns queries 32 w .. 32 w + 31 exactly as the dQ kernel does (S^T = K Q^T, dP^T = V dO^T, both 32-key sub-tiles in
//      registers), so delta is a sum over the lane's own registers -- no second walk, no workspace -- and dQ^T = K^T dS^T follows.
//      The same arithmetic in the same order as the general path (attn_tile.h's helpers restate its text): dQ is that path's, bit
//      for bit (asserted).
//   3. dV and dK sum over the QUERY, which sits on the lane: P~ and then dS cross the LDS once, as hi + lo 16-bit images [key][query]
//      laid over the K / V / K^T images (dead by then), and wave w, now owning KEYS 32 w .. 32 w + 31, reads them back as the B
//      operand of dV^T = dO^T P~ and dK^T = Q^T dS (A operand: the transposed dO / Q image, queries in natural order).
// ------------------------------------------------------------------------------------------------
constexpr int AT_PS = 72;                      // row stride of an exchange image (16-bit elements): 144 B rows, 16-byte aligned

template <bool F16, bool DROP>
__global__ __launch_bounds__(128) void at_bwd16_short_kernel(const void* __restrict__ qkv_, const uint8_t* __restrict__ key_pad,
                                                             const float* __restrict__ lse, const void* __restrict__ dout_,
                                                             void* __restrict__ dqkv_, int N, float scale, DropKey dk) {
    using E = Elem<F16>;
    using T = typename E::T;
    using V8 = typename E::V8;
    static_assert(2 * 64 * AT_PS * 2 <= 2 * AT_RM + AT_TR, "the exchange images fit over K | V | K^T");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * AT_RM + 3 * AT_TR + 256];
    unsigned char* krm = lds;
    unsigned char* vrm = lds + AT_RM;
    T* ktr = reinterpret_cast<T*>(lds + 2 * AT_RM);
    T* qtr = reinterpret_cast<T*>(lds + 2 * AT_RM + AT_TR);
    T* dotr = reinterpret_cast<T*>(lds + 2 * AT_RM + 2 * AT_TR);
    float* deadf = reinterpret_cast<float*>(lds + 2 * AT_RM + 3 * AT_TR);      // 1 = padded key or key >= N
    T* img_hi = reinterpret_cast<T*>(lds);                                     // step 3 only
    T* img_lo = img_hi + 64 * AT_PS;
    const T* __restrict__ qkv = reinterpret_cast<const T*>(qkv_);
    const T* __restrict__ dout = reinterpret_cast<const T*>(dout_);
    T* __restrict__ dqkv = reinterpret_cast<T*>(dqkv_);

    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.z, head = blockIdx.y;
    const int own0 = wave * 32, own = own0 + l31, ownc = own < N ? own : N - 1;
    const size_t row_base = (size_t)b * N;
    const T* qb = qkv + row_base * QKV_LD + head * 64;
    const T* dob = dout + row_base * BG_D_MODEL + head * 64;
    const unsigned long long g = dk.first + (unsigned long long)b;

    // ---- 1. stage ----
    at_stage<F16, 128, true, true>(qb + BG_D_MODEL, QKV_LD, 0, N, krm, ktr, tid);
    at_stage<F16, 128, true, false>(qb + 2 * BG_D_MODEL, QKV_LD, 0, N, vrm, nullptr, tid);
    at_stage<F16, 128, false, true>(qb, QKV_LD, 0, N, nullptr, qtr, tid);
    at_stage<F16, 128, false, true>(dob, BG_D_MODEL, 0, N, nullptr, dotr, tid);
    if (tid < 64) deadf[tid] = (tid >= N || (key_pad != nullptr && key_pad[row_base + tid] != 0)) ? 1.f : 0.f;
    __syncthreads();

    // ---- 2. the wave's 32 queries against all keys: P~, dS (kept in registers), dQ ----
    f32x16 pt[2], ds[2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) { pt[sub][r] = 0.f; ds[sub][r] = 0.f; }
    if (own0 < N) {                                        // wave-uniform
        V8 xf[4], yf[4];
        at_row_frags<F16>(qb + (size_t)ownc * QKV_LD, h, xf);
        at_row_frags<F16>(dob + (size_t)ownc * BG_D_MODEL, h, yf);
        const float lse_o = lse[((size_t)b * BG_N_HEAD + head) * N + ownc];
        f32x16 dpm[2];                                     // masked dP
        float dsum = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            f32x16 s, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                s = E::mfma(at_frag_rm<F16>(krm, sub * 32 + l31, ks * 2 + h), xf[ks], s);
                dp = E::mfma(at_frag_rm<F16>(vrm, sub * 32 + l31, ks * 2 + h), yf[ks], dp);
            }
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                unsigned nib = 0xFu;
                if (DROP) nib = keep_nibble(dk, g, head, own, (sub * 32 + at_walked(4 * g4, h)) >> 2);
                const float4 x0 = *reinterpret_cast<const float4*>(&deadf[sub * 32 + at_walked(4 * g4, h)]);
                const float v0[4] = {x0.x, x0.y, x0.z, x0.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g4 + e;
                    const bool dead = v0[e] != 0.f || own >= N;
                    float dpv = dp[r], pv;
                    const float p = at_bwd_elem<DROP>(s[r], scale, lse_o, dead, (nib >> e) & 1u, dk.rp, dpv, pv);
                    dsum += dead ? 0.f : p * dpv;
                    pt[sub][r] = pv;
                    ds[sub][r] = p;                        // P for now
                    dpm[sub][r] = dead ? 0.f : dpv;
                }
            }
        }
        const float del_o = dsum + __shfl_xor(dsum, 32, 64);    // the query's keys are split over lane and lane ^ 32
        f32x16 acc[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int r = 0; r < 16; ++r) ds[sub][r] = ds[sub][r] == 0.f ? 0.f : ds[sub][r] * (dpm[sub][r] - del_o);
#pragma unroll
            for (int sl = 0; sl < 2; ++sl) {
                V8 dsb, dsl;
                at_split8<F16>(ds[sub], sl, dsb, dsl);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    at_mfma_hilo<F16>(acc[dt], at_frag_tr<F16>(ktr, dt * 32 + l31, sub * 32 + 16 * sl + 4 * h), dsb, dsl);
            }
        }
        if (own < N) at_store_acc<F16>(dqkv + (row_base + own) * QKV_LD + head * 64, acc, scale, h);
    }

    // ---- 3. P~ (round 0: dV) and dS (round 1: dK) across the LDS; the wave now owns keys 32 w .. 32 w + 31 ----
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        __syncthreads();                                   // K / V / K^T (round 0) or the previous images (round 1) fully consumed
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = sub * 32 + at_walked(r, h);
                T hi, lo;
                at_hilo(round == 0 ? pt[sub][r] : ds[sub][r], hi, lo);
                img_hi[key * AT_PS + own] = hi;
                img_lo[key * AT_PS + own] = lo;
            }
        __syncthreads();
        if (own0 >= N) continue;                           // wave-uniform: no key of this wave exists
        const T* tr = round == 0 ? dotr : qtr;
        f32x16 acc[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if (16 * ks >= N) break;                       // uniform: queries 16 ks .. do not exist (their P~ and dS are 0 anyway)
            const V8 bh = *reinterpret_cast<const V8*>(img_hi + own * AT_PS + 16 * ks + 8 * h);
            const V8 bl = *reinterpret_cast<const V8*>(img_lo + own * AT_PS + 16 * ks + 8 * h);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) at_mfma_hilo<F16>(acc[dt], at_frag_tr<F16, 4>(tr, dt * 32 + l31, 16 * ks + 8 * h), bh, bl);
        }
        if (own < N)
            at_store_acc<F16>(dqkv + (row_base + own) * QKV_LD + head * 64 + (round == 0 ? 2 * BG_D_MODEL : BG_D_MODEL), acc,
                              round == 0 ? 1.0f : scale, h);
    }
}

// ------------------------------------------------------------------------------------------------
// fp32: one wave per owned row of (b, head); lane = walked index for the scores, lane = d for the products.  fp32 operands and
// results, every dot product and sum accumulated in fp64 (v_fma_f64, a fixed order) and rounded once: the parity mode's error is the
// rounding of P, dS and the results themselves, not the length of a chain.
// ------------------------------------------------------------------------------------------------
template <bool DROP>
__global__ __launch_bounds__(256) void at_fwd32_kernel(const float* __restrict__ qkv, const uint8_t* __restrict__ key_pad,
                                                       float* __restrict__ out, float* __restrict__ lse, int N, float scale, DropKey dk) {
    extern __shared__ float at_dyn[];                  // 4 waves x N
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wave;
    const int head = blockIdx.y, b = blockIdx.z;
    float* p = at_dyn + (size_t)wave * N;
    const size_t row_base = (size_t)b * N;
    if (q >= N) return;                                // no block-level barriers below
    const float* base = qkv + row_base * QKV_LD + head * 64;
    const float* qp = base + (size_t)q * QKV_LD;
    const unsigned long long g = dk.first + (unsigned long long)b;
    float qv[64];
#pragma unroll
    for (int d = 0; d < 64; ++d) qv[d] = qp[d];
    float mloc = -INFINITY;
    for (int j = lane; j < N; j += 64) {
        float sc = -INFINITY;
        if (!(key_pad != nullptr && key_pad[row_base + j] != 0)) {
            const float* kp = base + (size_t)j * QKV_LD + BG_D_MODEL;
            double acc = 0.0;
#pragma unroll
            for (int d = 0; d < 64; ++d) acc = fma((double)qv[d], (double)kp[d], acc);
            sc = (float)(acc * (double)scale);
        }
        p[j] = sc;
        mloc = fmaxf(mloc, sc);
    }
    const float m = wave_max(mloc);
    const float m_use = (m == -INFINITY) ? 0.f : m;
    double lsum = 0.0;
    for (int j = lane; j < N; j += 64) {
        const float e = expf(p[j] - m_use);
        lsum += (double)e;
        bool kept = true;
        if (DROP) kept = (keep_nibble(dk, g, head, q, j >> 2) >> (j & 3)) & 1u;
        p[j] = kept ? e : 0.f;
    }
    const float l = wave_sum((float)lsum);
    at_wave_lds_sync();
    double a[4] = {0.0, 0.0, 0.0, 0.0};                // lane = d
    const float* vb = base + 2 * BG_D_MODEL + lane;
    int j = 0;
    for (; j + 4 <= N; j += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = fma((double)p[j + u], (double)vb[(size_t)(j + u) * QKV_LD], a[u]);
    }
    for (int u = 0; j + u < N; ++u) a[u] = fma((double)p[j + u], (double)vb[(size_t)(j + u) * QKV_LD], a[u]);
    const float acc = (float)((a[0] + a[1]) + (a[2] + a[3]));
    out[(row_base + q) * BG_D_MODEL + head * 64 + lane] = l > 0.f ? (DROP ? acc * dk.rp : acc) / l : 0.f;
    if (lane == 0) lse[((size_t)b * BG_N_HEAD + head) * N + q] = l > 0.f ? m_use + logf(l) : 0.f;
}

// DKV = false: owned = query (X = Q row, Y = dO row), writes dQ;  DKV = true: owned = key (X = K row, Y = V row), writes dK and dV
template <bool DROP, bool DKV>
__global__ __launch_bounds__(256) void at_bwd32_kernel(const float* __restrict__ qkv, const uint8_t* __restrict__ key_pad,
                                                       float* __restrict__ delta,
                                                       const float* __restrict__ dout, float* __restrict__ dqkv, int N, float scale,
                                                       DropKey dk) {
    extern __shared__ float at_dyn[];                  // 4 waves x 2 N: dS | P~ over the walked index
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int own = blockIdx.x * 4 + wave;
    const int head = blockIdx.y, b = blockIdx.z;
    float* ds = at_dyn + (size_t)wave * 2 * N;
    float* pt = ds + N;
    const size_t row_base = (size_t)b * N;
    if (own >= N) return;                              // no block-level barriers below
    const float* qb = qkv + row_base * QKV_LD + head * 64;
    const float* dob = dout + row_base * BG_D_MODEL + head * 64;
    // workspace: delta | row maximum | row sum, [B, 12, N] each, written by the dQ kernel and read by the dK/dV kernel.  The fp32
    // kernels normalise as torch does, P = exp(S - max) / sum: lse rounded to fp32 (|lse| up to ~8) would put an error of several
    // ulp into every P of its row.
    const size_t plane = (size_t)gridDim.z * BG_N_HEAD * N;
    float* del_b = delta + ((size_t)b * BG_N_HEAD + head) * N;
    float* max_b = del_b + plane;
    float* sum_b = del_b + 2 * plane;
    const unsigned long long g = dk.first + (unsigned long long)b;
    float* op = dqkv + (row_base + own) * QKV_LD + head * 64 + lane;
    if (DKV && key_pad != nullptr && key_pad[row_base + own] != 0) {      // wave-uniform: a padded key has P = 0 in every row
        op[BG_D_MODEL] = 0.f;
        op[2 * BG_D_MODEL] = 0.f;
        return;
    }
    const float* xp = (DKV ? qb + BG_D_MODEL : qb) + (size_t)own * QKV_LD;
    const float* yp = DKV ? qb + 2 * BG_D_MODEL + (size_t)own * QKV_LD : dob + (size_t)own * BG_D_MODEL;
    float xv[64], yv[64];
#pragma unroll
    for (int d = 0; d < 64; ++d) { xv[d] = xp[d]; yv[d] = yp[d]; }
    float mloc = -INFINITY;
    for (int w = lane; w < N; w += 64) {
        const int qi = DKV ? w : own, kj = DKV ? own : w;
        float dsv = 0.f, ptv = DKV ? 0.f : -INFINITY;  // dQ: pt carries the score first (-inf = padded key)
        if (!(!DKV && key_pad != nullptr && key_pad[row_base + w] != 0)) {
            const float* a1 = (DKV ? qb : qb + BG_D_MODEL) + (size_t)w * QKV_LD;
            const float* a2 = DKV ? dob + (size_t)w * BG_D_MODEL : qb + 2 * BG_D_MODEL + (size_t)w * QKV_LD;
            double sacc = 0.0, dacc = 0.0;
#pragma unroll
            for (int d = 0; d < 64; ++d) sacc = fma((double)xv[d], (double)a1[d], sacc);
#pragma unroll
            for (int d = 0; d < 64; ++d) dacc = fma((double)yv[d], (double)a2[d], dacc);
            const float sc = (float)(sacc * (double)scale);
            float dpv = (float)dacc;
            bool kept = true;
            if (DROP) {
                kept = (keep_nibble(dk, g, head, qi, kj >> 2) >> (kj & 3)) & 1u;
                dpv = kept ? dpv * dk.rp : 0.f;
            }
            if (DKV) {
                const float l = sum_b[w];
                const float pr = l > 0.f ? expf(sc - max_b[w]) / l : 0.f;
                ptv = DROP ? (kept ? pr * dk.rp : 0.f) : pr;
                dsv = pr * (dpv - del_b[w]);
            } else {                                   // the row's maximum, sum and delta are not known yet: keep S and the masked dP
                ptv = sc;
                dsv = dpv;
                mloc = fmaxf(mloc, sc);
            }
        }
        ds[w] = dsv;
        pt[w] = ptv;
    }
    if (!DKV) {
        const float m = wave_max(mloc);
        const float m_use = (m == -INFINITY) ? 0.f : m;
        double lsum = 0.0, dpart = 0.0;
        for (int w = lane; w < N; w += 64) {
            const float e = expf(pt[w] - m_use);
            pt[w] = e;
            lsum += (double)e;
        }
        const float l = wave_sum((float)lsum);
        for (int w = lane; w < N; w += 64) {
            const float pr = l > 0.f ? pt[w] / l : 0.f;
            pt[w] = pr;
            dpart += (double)pr * (double)ds[w];       // delta = rowsum(P o masked dP)
        }
        const float del_o = wave_sum((float)dpart);
        for (int w = lane; w < N; w += 64) ds[w] = pt[w] * (ds[w] - del_o);
        if (lane == 0) { del_b[own] = del_o; max_b[own] = m_use; sum_b[own] = l; }
    }
    at_wave_lds_sync();
    // lane = d
    const float* m1 = (DKV ? qb : qb + BG_D_MODEL) + lane;           // dQ: K rows;  dK: Q rows
    const float* m2 = dob + lane;                                    // dV: dO rows
    double a[4] = {0.0, 0.0, 0.0, 0.0}, c[4] = {0.0, 0.0, 0.0, 0.0};
    int w = 0;
    for (; w + 4 <= N; w += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = fma((double)ds[w + u], (double)m1[(size_t)(w + u) * QKV_LD], a[u]);
            if (DKV) c[u] = fma((double)pt[w + u], (double)m2[(size_t)(w + u) * BG_D_MODEL], c[u]);
        }
    }
    for (int u = 0; w + u < N; ++u) {
        a[u] = fma((double)ds[w + u], (double)m1[(size_t)(w + u) * QKV_LD], a[u]);
        if (DKV) c[u] = fma((double)pt[w + u], (double)m2[(size_t)(w + u) * BG_D_MODEL], c[u]);
    }
    const float r1 = (float)(((a[0] + a[1]) + (a[2] + a[3])) * (double)scale);
    if (DKV) {
        op[BG_D_MODEL] = r1;
        op[2 * BG_D_MODEL] = (float)((c[0] + c[1]) + (c[2] + c[3]));
    } else {
        op[0] = r1;
    }
}

// ---- host side ----
static int at_drop_key(const char* who, int B, int N, double p, unsigned long long seed, unsigned draw_id, long long first_sample, DropKey& dk) {
    const int bad = drop_key_common(B, p, seed, draw_id, first_sample, dk.seed_lo, dk.seed_hi, dk.draw, dk.first, dk.rp);
    BG_REQUIRE(bad != DROP_BAD_P, BG_E_ARG, "%s: dropout_p = %g outside [0, 1)", who, p);      // (NaN fails too)
    BG_REQUIRE(bad != DROP_NEGATIVE_FIRST, BG_E_ARG, "%s: negative first_sample", who);
    BG_REQUIRE(bad != DROP_FIRST_PAST_2_44, BG_E_ARG,
               "%s: first_sample + B = %lld + %d, the dropout counter holds global sample indices below 2^44", who, first_sample, B);
    BG_REQUIRE(p == 0.0 || N <= AT_MAX_N_DROP, BG_E_SHAPE, "%s: N = %d, the dropout counter holds sequences up to %d", who, N, AT_MAX_N_DROP);
    dk.thr = (uint32_t)floor(p * 4294967296.0);
    return 0;
}

static int at_fp32_lds(const char* who, const void* kernel, size_t shm, int N) {
    if (shm > 160 * 1024) {
        set_error("%s: N=%d too long for the fp32 parity kernel", who, N);
        return BG_E_SHAPE;
    }
    if (shm > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) {
            set_error("%s: %zu bytes of LDS for N=%d refused: %s", who, shm, N, hipGetErrorString(e));
            return (int)e;
        }
    }
    return 0;
}

}  // namespace bg

using namespace bg;

#define AT_CHECK_COMMON(who)                                                                                                \
    BG_REQUIRE(B >= 0 && B <= 65535, BG_E_ARG, who ": B = %d outside [0, 65535]", B);                                        \
    BG_REQUIRE(N >= 1, BG_E_ARG, who ": N = %d, at least one token", N);                                                    \
    BG_REQUIRE(dtype == BG_BF16 || dtype == BG_F16 || dtype == BG_F32, BG_E_DTYPE, who ": unsupported dtype %d", dtype);    \
    BG_REQUIRE(isfinite(scale), BG_E_ARG, who ": scale is not finite")

extern "C" int bg_attn_train_fwd(const void* qkv, const uint8_t* key_pad, void* out, float* lse, int B, int N, int dtype, float scale,
                                 double dropout_p, unsigned long long seed, unsigned draw_id, long long first_sample,
                                 bg_stream_t stream) {
    AT_CHECK_COMMON("bg_attn_train_fwd");
    BG_REQUIRE(qkv && out && lse, BG_E_ARG, "bg_attn_train_fwd: null pointer (qkv, out, lse)");
    BG_REQUIRE(aligned(qkv, 16) && aligned(out, 16) && aligned(lse, 4), BG_E_ALIGN,
               "bg_attn_train_fwd: 16-byte alignment of qkv / out, 4-byte of lse");
    DropKey dk;
    if (const int rc = at_drop_key("bg_attn_train_fwd", B, N, dropout_p, seed, draw_id, first_sample, dk)) return rc;
    if (B == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const bool drop = dk.thr != 0;
    if (dtype == BG_F32) {
        const size_t shm = (size_t)4 * N * sizeof(float);
        const void* k = drop ? reinterpret_cast<const void*>(at_fwd32_kernel<true>) : reinterpret_cast<const void*>(at_fwd32_kernel<false>);
        if (const int rc = at_fp32_lds("bg_attn_train_fwd", k, shm, N)) return rc;
        const dim3 grid((N + 3) / 4, BG_N_HEAD, B);
        if (drop) hipLaunchKernelGGL(at_fwd32_kernel<true>, grid, dim3(256), shm, s, (const float*)qkv, key_pad, (float*)out, lse, N, scale, dk);
        else hipLaunchKernelGGL(at_fwd32_kernel<false>, grid, dim3(256), shm, s, (const float*)qkv, key_pad, (float*)out, lse, N, scale, dk);
        return launch_status("attn_train_fwd_f32");
    }
    const dim3 grid((N + 127) / 128, BG_N_HEAD, B);
    with_bools(dtype == BG_F16, drop, [&](auto F16, auto DROP) {
        hipLaunchKernelGGL((at_fwd16_kernel<F16(), DROP()>), grid, dim3(256), 0, s, qkv, key_pad, out, lse, N, scale, dk);
    });
    return launch_status("attn_train_fwd16");
}

extern "C" size_t bg_attn_bwd_workspace_bytes(int B, int N, int dtype) {
    if (B <= 0 || N < 1 || !(dtype == BG_BF16 || dtype == BG_F16 || dtype == BG_F32)) return 0;
    // delta [B, 12, N]; BG_F32: + row maximum and row sum
    return (((size_t)B * BG_N_HEAD * N * sizeof(float) * (dtype == BG_F32 ? 3 : 1)) + 255) & ~(size_t)255;
}

template <bool DROP>
static int at_launch_bwd32(hipStream_t s, const void* qkv, const uint8_t* key_pad, float* delta, const void* dout,
                           void* dqkv, int B, int N, float scale, const DropKey& dk) {
    const size_t shm = (size_t)8 * N * sizeof(float);
    if (const int rc = at_fp32_lds("bg_attn_bwd", reinterpret_cast<const void*>(at_bwd32_kernel<DROP, false>), shm, N)) return rc;
    if (const int rc = at_fp32_lds("bg_attn_bwd", reinterpret_cast<const void*>(at_bwd32_kernel<DROP, true>), shm, N)) return rc;
    const dim3 grid((N + 3) / 4, BG_N_HEAD, B);
    hipLaunchKernelGGL((at_bwd32_kernel<DROP, false>), grid, dim3(256), shm, s, (const float*)qkv, key_pad, delta, (const float*)dout,
                       (float*)dqkv, N, scale, dk);
    hipLaunchKernelGGL((at_bwd32_kernel<DROP, true>), grid, dim3(256), shm, s, (const float*)qkv, key_pad, delta, (const float*)dout,
                       (float*)dqkv, N, scale, dk);
    return 0;
}

extern "C" int bg_attn_bwd(const void* qkv, const uint8_t* key_pad, const float* lse, const void* dout, void* dqkv, int B,
                           int N, int dtype, float scale, double dropout_p, unsigned long long seed, unsigned draw_id,
                           long long first_sample, int variant, void* workspace, size_t workspace_bytes, bg_stream_t stream) {
    AT_CHECK_COMMON("bg_attn_bwd");
    BG_REQUIRE(variant >= BG_ATTN_BWD_AUTO && variant <= BG_ATTN_BWD_SHORT, BG_E_ARG, "bg_attn_bwd: variant %d (0 auto, 1 general, 2 short)", variant);
    BG_REQUIRE(variant != BG_ATTN_BWD_SHORT || (N <= 64 && dtype != BG_F32), BG_E_SHAPE,
               "bg_attn_bwd: the short-sequence kernel takes N <= 64 and 16-bit operands (N = %d, dtype %d)", N, dtype);
    BG_REQUIRE(qkv && lse && dout && dqkv, BG_E_ARG, "bg_attn_bwd: null pointer (qkv, lse, dout, dqkv)");
    BG_REQUIRE(aligned(qkv, 16) && aligned(dout, 16) && aligned(dqkv, 16) && aligned(lse, 4) && aligned(workspace, 4), BG_E_ALIGN,
               "bg_attn_bwd: 16-byte alignment of qkv / dout / dqkv, 4-byte of lse / workspace");
    DropKey dk;
    if (const int rc = at_drop_key("bg_attn_bwd", B, N, dropout_p, seed, draw_id, first_sample, dk)) return rc;
    if (B == 0) return 0;
    const size_t need = bg_attn_bwd_workspace_bytes(B, N, dtype);
    BG_REQUIRE(workspace != nullptr && workspace_bytes >= need, BG_E_WORKSPACE, "bg_attn_bwd: workspace of %zu bytes, %zu needed",
               workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t s = (hipStream_t)stream;
    const bool drop = dk.thr != 0;
    float* delta = reinterpret_cast<float*>(workspace);
    if (dtype == BG_F32) {
        const int rc = drop ? at_launch_bwd32<true>(s, qkv, key_pad, delta, dout, dqkv, B, N, scale, dk)
                            : at_launch_bwd32<false>(s, qkv, key_pad, delta, dout, dqkv, B, N, scale, dk);
        if (rc) return rc;
        return launch_status("attn_bwd_f32");
    }
    if (variant == BG_ATTN_BWD_SHORT || (variant == BG_ATTN_BWD_AUTO && N <= AT_SHORT_AUTO_N)) {
        const dim3 sgrid(1, BG_N_HEAD, B);
        with_bools(dtype == BG_F16, drop, [&](auto F16, auto DROP) {
            hipLaunchKernelGGL((at_bwd16_short_kernel<F16(), DROP()>), sgrid, dim3(128), 0, s, qkv, key_pad, lse, dout, dqkv, N, scale, dk);
        });
        return launch_status("attn_bwd16_short");
    }
    const dim3 grid((N + 127) / 128, BG_N_HEAD, B);
    with_bools(dtype == BG_F16, drop, [&](auto F16, auto DROP) {
        hipLaunchKernelGGL((at_bwd16_kernel<F16(), DROP(), false>), grid, dim3(256), 0, s, qkv, key_pad, lse, delta, dout, dqkv, N, scale, dk);
        hipLaunchKernelGGL((at_bwd16_kernel<F16(), DROP(), true>), grid, dim3(256), 0, s, qkv, key_pad, lse, delta, dout, dqkv, N, scale, dk);
    });
    return launch_status("attn_bwd16");
}

extern "C" int bg_attn_dropout_mask(uint8_t* mask, int B, int N, double dropout_p, unsigned long long seed, unsigned draw_id,
                                    long long first_sample, bg_stream_t stream) {
    BG_REQUIRE(B >= 0, BG_E_ARG, "bg_attn_dropout_mask: negative B");
    BG_REQUIRE(N >= 1, BG_E_ARG, "bg_attn_dropout_mask: N = %d, at least one token", N);
    BG_REQUIRE(mask != nullptr, BG_E_ARG, "bg_attn_dropout_mask: null pointer (mask)");
    DropKey dk;
    if (const int rc = at_drop_key("bg_attn_dropout_mask", B, N, dropout_p, seed, draw_id, first_sample, dk)) return rc;
    BG_REQUIRE(N <= AT_MAX_N_DROP, BG_E_SHAPE, "bg_attn_dropout_mask: N = %d, the dropout counter holds sequences up to %d", N, AT_MAX_N_DROP);
    if (B == 0) return 0;
    const long long total = (long long)B * BG_N_HEAD * N * ((N + 3) / 4);
    BG_REQUIRE((total + 255) / 256 <= 0x7FFFFFFFLL, BG_E_SHAPE, "bg_attn_dropout_mask: B * 12 * N * N / 4 = %lld blocks is too many for one launch", total);
    hipLaunchKernelGGL(at_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mask, B, N, dk);
    return launch_status("attn_dropout_mask");
}
