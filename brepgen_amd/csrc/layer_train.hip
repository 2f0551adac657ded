// The glue of an encoder layer in TRAINING (nn.TransformerEncoderLayer(768, 12, 1024, dropout, norm_first=True), network.py:1076-1078):
// LayerNorm forward that keeps (mean, rstd), LayerNorm backward with the residual merge and the gamma / beta gradients, and the
// elementwise dropout ops (dropout + residual add, ReLU + dropout) with their backward.  Row-wise, memory-bound passes over
// [tokens, 768] / [tokens, 1024]; include/brepgen_hip.h states every entry.  Nothing is allocated, no atomics: one writer per output
// element and a fixed summation order.
//
// Layout of the LayerNorm kernels: a HALF-wave (32 lanes) owns one row of 768 = 32 x 3 x 8 columns; lane l holds the three 8-column
// chunks l, l + 32, l + 64 (16 bytes of 16-bit data, 32 bytes of fp32 each), a 256-thread workgroup works on 8 rows at a time.  Row
// sums: the 8 values of a chunk pairwise, the lane's three chunks in order, then a butterfly over the 32 lanes.
#include "bg_common.h"
#include "philox.h"

namespace bg {

constexpr int LT_C = 768;                 // LayerNorm width
constexpr int LT_CH = 3;                  // 8-column chunks per lane
constexpr int LT_SLOTS = 8;               // rows in flight per workgroup (one per half-wave)
constexpr int LT_MAX_WGS = 2048;          // grid cap: 8 resident workgroups of 256 threads per CU; the rest is strided over
constexpr int LT_CHAIN_MIN = 4, LT_CHAIN_MAX = 64, LT_CHAIN_TARGET = LT_SLOTS * 1024;

// rows per fp32 column-sum chain of bg_ln_bwd, a pure function of M (brepgen_hip.h): about 1024 workgroups where the rows allow it
static inline int lt_chain_rows(int M) {
    const int r = (M + LT_CHAIN_TARGET - 1) / LT_CHAIN_TARGET;
    return r < LT_CHAIN_MIN ? LT_CHAIN_MIN : (r > LT_CHAIN_MAX ? LT_CHAIN_MAX : r);
}
static inline int lt_bwd_chunks(int M) { const int rows = LT_SLOTS * lt_chain_rows(M); return (M + rows - 1) / rows; }
static inline int lt_bwd_wgs(int M) { const int c = lt_bwd_chunks(M); return c < LT_MAX_WGS ? c : LT_MAX_WGS; }

// ---- 8 consecutive elements of dtype DT (BG_F32 | BG_F16 | BG_BF16) <-> floats; `at` = element index, a multiple of 8 ----
template <int DT> __device__ __forceinline__ void lt_load8(const void* p, size_t at, float (&f)[8]) {
    if (DT == BG_F32) {
        const float4* q = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(p) + at);
        const float4 a = q[0], b = q[1];
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
        const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(p) + at);
        float lo[4], hi[4];
        unpack4_16<DT == BG_F16>(make_uint2(u.x, u.y), lo);
        unpack4_16<DT == BG_F16>(make_uint2(u.z, u.w), hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) { f[e] = lo[e]; f[4 + e] = hi[e]; }
    }
}
template <int DT> __device__ __forceinline__ void lt_store8(void* p, size_t at, const float (&f)[8]) {
    if (DT == BG_F32) {
        float4* q = reinterpret_cast<float4*>(reinterpret_cast<float*>(p) + at);
        q[0] = make_float4(f[0], f[1], f[2], f[3]);
        q[1] = make_float4(f[4], f[5], f[6], f[7]);
    } else {
        const uint2 a = pack4_16(f[0], f[1], f[2], f[3], DT), b = pack4_16(f[4], f[5], f[6], f[7], DT);       // one rounding, RNE
        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(p) + at) = make_uint4(a.x, a.y, b.x, b.y);
    }
}
// the 8 values of a chunk, pairwise
__device__ __forceinline__ float lt_sum8(const float (&a)[8]) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }
// butterfly over the 32 lanes that share a row (the partner of a lane is always in its own half-wave)
__device__ __forceinline__ float lt_half_sum(float t) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
    return t;
}

// ---- bg_ln_train_fwd ----
template <int XD, int YD>
__global__ __launch_bounds__(256) void lt_ln_fwd_kernel(const void* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        void* __restrict__ y, float* __restrict__ stats, int M, float eps) {
    const int l32 = threadIdx.x & 31, slot = threadIdx.x >> 5;
    float g[LT_CH][8], b[LT_CH][8];
#pragma unroll
    for (int j = 0; j < LT_CH; ++j) {
        lt_load8<BG_F32>(gamma, (size_t)(l32 + 32 * j) * 8, g[j]);
        lt_load8<BG_F32>(beta, (size_t)(l32 + 32 * j) * 8, b[j]);
    }
    for (long long row = (long long)blockIdx.x * LT_SLOTS + slot; row < M; row += (long long)gridDim.x * LT_SLOTS) {
        const size_t base = (size_t)row * LT_C;
        float d[LT_CH][8];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < LT_CH; ++j) {
            lt_load8<XD>(x, base + (size_t)(l32 + 32 * j) * 8, d[j]);
            s += lt_sum8(d[j]);
        }
        const float mean = lt_half_sum(s) * (1.0f / LT_C);
        float q = 0.f;                     // second pass over the row in registers: the CENTRED sum of squares
#pragma unroll
        for (int j = 0; j < LT_CH; ++j) {
            float sq[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { d[j][e] -= mean; sq[e] = d[j][e] * d[j][e]; }
            q += lt_sum8(sq);
        }
        const float rstd = 1.0f / sqrtf(lt_half_sum(q) * (1.0f / LT_C) + eps);
#pragma unroll
        for (int j = 0; j < LT_CH; ++j) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = d[j][e] * rstd * g[j][e] + b[j][e];
            lt_store8<YD>(y, base + (size_t)(l32 + 32 * j) * 8, o);
        }
        if (l32 == 0) *reinterpret_cast<float2*>(stats + 2 * (size_t)row) = make_float2(mean, rstd);
    }
}

// ---- bg_ln_bwd ----
// WG: also the column sums dgamma / dbeta.  A workgroup takes chunks of 8 * chain rows (row = chunk * 8 * chain + i * 8 + slot: the
// eight half-waves read eight consecutive rows); a lane adds the <= chain rows of its slot into 2 x 24 fp32 column accumulators, the
// eight slots' chains of a column meet in LDS and are added IN SLOT ORDER in fp64 into the workgroup's running fp64 sums (thread t
// owns quantities t, t + 256, ...; quantity = column for dgamma, 768 + column for dbeta), and the workgroup's 1536 doubles go to
// ws[blockIdx.x][1536] for lt_ln_reduce_kernel.
template <int XD, int YD, bool WG>
__global__ __launch_bounds__(256) void lt_ln_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ x, const float* __restrict__ stats,
                                                        const float* __restrict__ gamma, const void* __restrict__ dskip, void* __restrict__ dx,
                                                        double* __restrict__ ws, int M, int chain, int nchunks) {
    __shared__ __attribute__((aligned(16))) float red[WG ? LT_SLOTS * 2 * LT_C : 4];
    const int l32 = threadIdx.x & 31, slot = threadIdx.x >> 5;
    float g[LT_CH][8];
#pragma unroll
    for (int j = 0; j < LT_CH; ++j) lt_load8<BG_F32>(gamma, (size_t)(l32 + 32 * j) * 8, g[j]);
    double tot[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        float ag[LT_CH][8], ab[LT_CH][8];
        if (WG) {
#pragma unroll
            for (int j = 0; j < LT_CH; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) ag[j][e] = ab[j][e] = 0.f;
        }
        const long long row0 = (long long)chunk * (LT_SLOTS * chain) + slot;
        for (int i = 0; i < chain; ++i) {
            const long long row = row0 + (long long)i * LT_SLOTS;
            if (row >= M) break;
            const size_t base = (size_t)row * LT_C;
            const float2 st = *reinterpret_cast<const float2*>(stats + 2 * (size_t)row);      // (mean, rstd)
            float xh[LT_CH][8], gd[LT_CH][8];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < LT_CH; ++j) {
                float dv[8], pr[8];
                lt_load8<XD>(x, base + (size_t)(l32 + 32 * j) * 8, xh[j]);
                lt_load8<YD>(dy, base + (size_t)(l32 + 32 * j) * 8, dv);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    xh[j][e] = (xh[j][e] - st.x) * st.y;
                    gd[j][e] = g[j][e] * dv[e];
                    pr[e] = gd[j][e] * xh[j][e];
                    if (WG) { ag[j][e] += dv[e] * xh[j][e]; ab[j][e] += dv[e]; }
                }
                s1 += lt_sum8(gd[j]);
                s2 += lt_sum8(pr);
            }
            const float c1 = lt_half_sum(s1) * (1.0f / LT_C), c2 = lt_half_sum(s2) * (1.0f / LT_C);
#pragma unroll
            for (int j = 0; j < LT_CH; ++j) {
                float sk[8], o[8];
                if (dskip) lt_load8<XD>(dskip, base + (size_t)(l32 + 32 * j) * 8, sk);
                else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) sk[e] = 0.f;
                }
                // + sk in both forms: t + 0.0f is t for every t but -0, so a zero dskip and no dskip give the same bits
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = st.y * ((gd[j][e] - c1) - xh[j][e] * c2) + sk[e];
                lt_store8<XD>(dx, base + (size_t)(l32 + 32 * j) * 8, o);
            }
        }
        if (WG) {
#pragma unroll
            for (int j = 0; j < LT_CH; ++j) {
                float* at = red + slot * (2 * LT_C) + (l32 + 32 * j) * 8;
                *reinterpret_cast<float4*>(at) = make_float4(ag[j][0], ag[j][1], ag[j][2], ag[j][3]);
                *reinterpret_cast<float4*>(at + 4) = make_float4(ag[j][4], ag[j][5], ag[j][6], ag[j][7]);
                *reinterpret_cast<float4*>(at + LT_C) = make_float4(ab[j][0], ab[j][1], ab[j][2], ab[j][3]);
                *reinterpret_cast<float4*>(at + LT_C + 4) = make_float4(ab[j][4], ab[j][5], ab[j][6], ab[j][7]);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int sl = 0; sl < LT_SLOTS; ++sl) tot[k] += (double)red[sl * (2 * LT_C) + threadIdx.x + 256 * k];
            __syncthreads();
        }
    }
    if (WG) {
#pragma unroll
        for (int k = 0; k < 6; ++k) ws[(size_t)blockIdx.x * (2 * LT_C) + threadIdx.x + 256 * k] = tot[k];
    }
}

// ws [G][1536] fp64 -> dgamma | dbeta fp32: a workgroup owns 8 quantities; thread (group, c) adds the workgroups
// [group * per, (group + 1) * per), per = ceil(G / 32), of its quantity in index order, the 32 group sums are added in group order.
// (The loads of a thread do not depend on its additions: unrolled, eight are in flight -- with one at a time this launch took as long
// as the pass over the rows.)
constexpr int LT_RED_GROUPS = 32, LT_RED_COLS = 8;
__global__ __launch_bounds__(256) void lt_ln_reduce_kernel(const double* __restrict__ ws, int G, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    __shared__ double part[LT_RED_GROUPS][LT_RED_COLS];
    const int c = threadIdx.x & (LT_RED_COLS - 1), grp = threadIdx.x / LT_RED_COLS;
    const int q = blockIdx.x * LT_RED_COLS + c;              // < 1536: the grid is 192 workgroups
    const int per = (G + LT_RED_GROUPS - 1) / LT_RED_GROUPS;
    const int w1 = (grp + 1) * per < G ? (grp + 1) * per : G;
    double a = 0.0;
#pragma unroll 8
    for (int w = grp * per; w < w1; ++w) a += ws[(size_t)w * (2 * LT_C) + q];
    part[grp][c] = a;
    __syncthreads();
    if (grp == 0) {
        double t = part[0][c];
#pragma unroll
        for (int k = 1; k < LT_RED_GROUPS; ++k) t += part[k][c];
        if (q < LT_C) dgamma[q] = (float)t;
        else dbeta[q - LT_C] = (float)t;
    }
}

// ---- elementwise dropout: one thread per 8 consecutive columns = one Philox block (brepgen_hip.h) ----
struct LtDrop {
    uint32_t k0, k1, draw, tag;          // key = seed; tag = 0xD4090000 | site << 12
    uint32_t thr, CB, B;                 // keep iff half-word >= thr; CB = C / 8 column blocks per row
    float rp;                            // float(1 / (1 - p))
    unsigned long long first;            // first_sample
    unsigned long long nchunks;          // M * CB (< 2^32)
};
// keep bits of chunk q (bit j = element j kept)
__device__ __forceinline__ uint32_t lt_keep8(const LtDrop& k, uint32_t q) {
    const uint32_t r = q / k.CB, cb = q - r * k.CB;          // row, column block
    const uint32_t n = r / k.B, b = r - n * k.B;             // rows are sequence-first: token n of sample b
    const unsigned long long gs = k.first + b;
    uint32_t c[4] = {n * k.CB + cb, (uint32_t)gs, k.draw, drop_word3(k.tag, gs)};
    philox4x32_10(c, k.k0, k.k1);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t hw = (c[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
        m |= (hw >= k.thr ? 1u : 0u) << j;
    }
    return m;
}
#define LT_CHUNK_LOOP(k) \
    for (unsigned long long q_ = (unsigned long long)blockIdx.x * 256 + threadIdx.x; q_ < (k).nchunks; q_ += (unsigned long long)gridDim.x * 256)

// out = skip + keep * rp * branch  (SD: dtype of skip / out, BD: dtype of branch)
template <int SD, int BD, bool DROP>
__global__ __launch_bounds__(256) void lt_dropout_add_kernel(const void* __restrict__ branch, const void* __restrict__ skip, void* __restrict__ out, LtDrop k) {
    LT_CHUNK_LOOP(k) {
        const uint32_t q = (uint32_t)q_;
        const uint32_t m = DROP ? lt_keep8(k, q) : 0xFFu;
        float br[8], sk[8], o[8];
        lt_load8<BD>(branch, (size_t)q * 8, br);
        lt_load8<SD>(skip, (size_t)q * 8, sk);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (m >> e & 1u) ? sk[e] + br[e] * k.rp : sk[e];
        lt_store8<SD>(out, (size_t)q * 8, o);
    }
}
// dbranch = keep * rp * dout
template <int SD, int BD, bool DROP>
__global__ __launch_bounds__(256) void lt_dropout_bwd_kernel(const void* __restrict__ dout, void* __restrict__ dbranch, LtDrop k) {
    LT_CHUNK_LOOP(k) {
        const uint32_t q = (uint32_t)q_;
        const uint32_t m = DROP ? lt_keep8(k, q) : 0xFFu;
        float d[8], o[8];
        lt_load8<SD>(dout, (size_t)q * 8, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (m >> e & 1u) ? d[e] * k.rp : 0.f;
        lt_store8<BD>(dbranch, (size_t)q * 8, o);
    }
}
// h = (keep && x > 0) ? x * rp : 0; a kept NaN propagates (!(x <= 0) holds for it), a dropped element is 0 whatever x is
template <int DT, bool DROP>
__global__ __launch_bounds__(256) void lt_relu_dropout_kernel(const void* __restrict__ x, void* __restrict__ h, LtDrop k) {
    LT_CHUNK_LOOP(k) {
        const uint32_t q = (uint32_t)q_;
        const uint32_t m = DROP ? lt_keep8(k, q) : 0xFFu;
        float v[8], o[8];
        lt_load8<DT>(x, (size_t)q * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = ((m >> e & 1u) && !(v[e] <= 0.f)) ? v[e] * k.rp : 0.f;
        lt_store8<DT>(h, (size_t)q * 8, o);
    }
}
// dx = (h > 0) ? dh * rp : 0
template <int DT>
__global__ __launch_bounds__(256) void lt_relu_dropout_bwd_kernel(const void* __restrict__ h, const void* __restrict__ dh, void* __restrict__ dx, LtDrop k) {
    LT_CHUNK_LOOP(k) {
        const uint32_t q = (uint32_t)q_;
        float hv[8], d[8], o[8];
        lt_load8<DT>(h, (size_t)q * 8, hv);
        lt_load8<DT>(dh, (size_t)q * 8, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = hv[e] > 0.f ? d[e] * k.rp : 0.f;
        lt_store8<DT>(dx, (size_t)q * 8, o);
    }
}
__global__ __launch_bounds__(256) void lt_mask_kernel(uint8_t* __restrict__ mask, LtDrop k) {
    LT_CHUNK_LOOP(k) {
        const uint32_t q = (uint32_t)q_;
        const uint32_t m = lt_keep8(k, q);
        uint2 o;
        o.x = (m & 1u) | (m >> 1 & 1u) << 8 | (m >> 2 & 1u) << 16 | (m >> 3 & 1u) << 24;
        o.y = (m >> 4 & 1u) | (m >> 5 & 1u) << 8 | (m >> 6 & 1u) << 16 | (m >> 7 & 1u) << 24;
        *reinterpret_cast<uint2*>(mask + (size_t)q * 8) = o;
    }
}

// ---- host side ----
static inline bool lt_is_dtype(int d) { return d == BG_F32 || d == BG_F16 || d == BG_BF16; }
static inline bool lt_is_16(int d) { return d == BG_F16 || d == BG_BF16; }
// (dtype of x, dtype of y) the LayerNorm kernels are built for
static inline bool lt_ln_pair_ok(int xd, int yd) { return lt_is_dtype(xd) && lt_is_dtype(yd) && (xd == BG_F32 || yd == BG_F32 || yd == xd); }
template <int A, int B> struct LtPair { static constexpr int a = A, b = B; };
template <typename F> static void lt_ln_dispatch(int xd, int yd, F&& f) {
    if (xd == BG_F32 && yd == BG_F32) f(LtPair<BG_F32, BG_F32>{});
    else if (xd == BG_F32 && yd == BG_F16) f(LtPair<BG_F32, BG_F16>{});
    else if (xd == BG_F32 && yd == BG_BF16) f(LtPair<BG_F32, BG_BF16>{});
    else if (xd == BG_F16 && yd == BG_F16) f(LtPair<BG_F16, BG_F16>{});
    else if (xd == BG_F16 && yd == BG_F32) f(LtPair<BG_F16, BG_F32>{});
    else if (xd == BG_BF16 && yd == BG_BF16) f(LtPair<BG_BF16, BG_BF16>{});
    else f(LtPair<BG_BF16, BG_F32>{});
}

// shape and key checks shared by the dropout entries; fills `k`.  keyed: the entry takes (B, p, seed, draw_id, site, first_sample)
static int lt_drop_args(const char* who, int M, int C, int B, double p, unsigned long long seed, unsigned draw_id, int site,
                        long long first_sample, LtDrop& k) {
    BG_REQUIRE(M >= 0 && C >= 8 && C % 8 == 0, BG_E_SHAPE, "%s: M = %d must be >= 0 and C = %d a positive multiple of 8", who, M, C);
    BG_REQUIRE(B >= 1 && M % B == 0, BG_E_SHAPE, "%s: rows are sequence-first, M = %d must be a multiple of B = %d >= 1", who, M, B);
    BG_REQUIRE((unsigned long long)M * (unsigned)(C / 8) < (1ull << 32), BG_E_SHAPE, "%s: M * C / 8 = %llu does not fit 32 bits", who,
               (unsigned long long)M * (unsigned)(C / 8));
    const int bad = drop_key_common(B, p, seed, draw_id, first_sample, k.k0, k.k1, k.draw, k.first, k.rp);
    BG_REQUIRE(bad != DROP_BAD_P, BG_E_ARG, "%s: p = %g outside [0, 1)", who, p);
    BG_REQUIRE(site >= 0 && site <= 3, BG_E_ARG, "%s: site = %d outside 0 .. 3", who, site);
    BG_REQUIRE(bad == DROP_OK, BG_E_ARG, "%s: first_sample = %lld: first_sample + B must stay within 2^44", who, first_sample);
    k.tag = drop_tag_sub(0xD4090000u, (uint32_t)site);
    k.thr = (uint32_t)(p * 65536.0);                       // floor: p >= 0
    k.CB = (uint32_t)(C / 8); k.B = (uint32_t)B;
    k.nchunks = (unsigned long long)M * (unsigned)(C / 8);
    return 0;
}
static inline unsigned lt_chunk_grid(const LtDrop& k) {
    const unsigned long long b = (k.nchunks + 255) / 256;
    return (unsigned)(b < (unsigned long long)LT_MAX_WGS ? b : LT_MAX_WGS);
}

}  // namespace bg

using namespace bg;

extern "C" int bg_ln_train_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype, float* stats, int M,
                               float eps, bg_stream_t stream) {
    BG_REQUIRE(lt_ln_pair_ok(x_dtype, y_dtype), BG_E_DTYPE,
               "bg_ln_train_fwd: dtype pair x %d -> y %d (x fp32: any y; x 16-bit: y of the same dtype or fp32)", x_dtype, y_dtype);
    BG_REQUIRE(M >= 0, BG_E_SHAPE, "bg_ln_train_fwd: M = %d is negative", M);
    BG_REQUIRE(eps >= 0.f, BG_E_ARG, "bg_ln_train_fwd: eps = %g is negative", (double)eps);
    BG_REQUIRE(M == 0 || (x && gamma && beta && y && stats), BG_E_ARG, "bg_ln_train_fwd: null pointer (x, gamma, beta, y, stats)");
    BG_REQUIRE(aligned(x, 16) && aligned(gamma, 16) && aligned(beta, 16) && aligned(y, 16) && aligned(stats, 8), BG_E_ALIGN,
               "bg_ln_train_fwd: 16-byte alignment of x / gamma / beta / y, 8-byte alignment of stats");
    if (M == 0) return 0;
    const int rows8 = (M + LT_SLOTS - 1) / LT_SLOTS;
    const dim3 grid((unsigned)(rows8 < LT_MAX_WGS ? rows8 : LT_MAX_WGS));
    hipStream_t s = (hipStream_t)stream;
    lt_ln_dispatch(x_dtype, y_dtype, [&](auto pr) {
        hipLaunchKernelGGL((lt_ln_fwd_kernel<decltype(pr)::a, decltype(pr)::b>), grid, dim3(256), 0, s, x, gamma, beta, y, stats, M, eps);
    });
    return launch_status("ln_train_fwd");
}

extern "C" size_t bg_ln_bwd_workspace_bytes(int M) {
    if (M <= 0) return 0;
    return (size_t)lt_bwd_wgs(M) * (2 * LT_C) * sizeof(double);
}

extern "C" int bg_ln_bwd(const void* dy, int y_dtype, const void* x, int x_dtype, const float* stats, const float* gamma, const void* dskip,
                         void* dx, float* dgamma, float* dbeta, int M, void* workspace, size_t workspace_bytes, bg_stream_t stream) {
    BG_REQUIRE(lt_ln_pair_ok(x_dtype, y_dtype), BG_E_DTYPE,
               "bg_ln_bwd: dtype pair x %d -> y %d (x fp32: any y; x 16-bit: y of the same dtype or fp32)", x_dtype, y_dtype);
    BG_REQUIRE(M >= 0, BG_E_SHAPE, "bg_ln_bwd: M = %d is negative", M);
    BG_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), BG_E_ARG, "bg_ln_bwd: dgamma and dbeta must be given together or both be null");
    BG_REQUIRE(M == 0 || (dy && x && stats && gamma && dx), BG_E_ARG, "bg_ln_bwd: null pointer (dy, x, stats, gamma, dx)");
    BG_REQUIRE(aligned(dy, 16) && aligned(x, 16) && aligned(gamma, 16) && aligned(dskip, 16) && aligned(dx, 16) && aligned(dgamma, 16) &&
                   aligned(dbeta, 16) && aligned(workspace, 16) && aligned(stats, 8),
               BG_E_ALIGN, "bg_ln_bwd: 16-byte alignment of dy / x / gamma / dskip / dx / dgamma / dbeta / workspace, 8-byte alignment of stats");
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        if (dgamma) {
            hipError_t e = hipMemsetAsync(dgamma, 0, LT_C * sizeof(float), s);
            if (e == hipSuccess) e = hipMemsetAsync(dbeta, 0, LT_C * sizeof(float), s);
            BG_REQUIRE(e == hipSuccess, (int)e, "bg_ln_bwd: hipMemsetAsync: %s", hipGetErrorString(e));
        }
        return 0;
    }
    const size_t need = dgamma ? bg_ln_bwd_workspace_bytes(M) : 0;
    BG_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need), BG_E_ARG, "bg_ln_bwd: workspace of %zu bytes, %zu needed for M = %d",
               workspace ? workspace_bytes : (size_t)0, need, M);
    const int chain = lt_chain_rows(M), nchunks = lt_bwd_chunks(M), G = lt_bwd_wgs(M);
    double* ws = reinterpret_cast<double*>(workspace);
    lt_ln_dispatch(x_dtype, y_dtype, [&](auto pr) {
        if (dgamma)
            hipLaunchKernelGGL((lt_ln_bwd_kernel<decltype(pr)::a, decltype(pr)::b, true>), dim3((unsigned)G), dim3(256), 0, s, dy, x, stats, gamma, dskip,
                               dx, ws, M, chain, nchunks);
        else
            hipLaunchKernelGGL((lt_ln_bwd_kernel<decltype(pr)::a, decltype(pr)::b, false>), dim3((unsigned)G), dim3(256), 0, s, dy, x, stats, gamma, dskip,
                               dx, ws, M, chain, nchunks);
    });
    if (dgamma) hipLaunchKernelGGL(lt_ln_reduce_kernel, dim3(2 * LT_C / LT_RED_COLS), dim3(256), 0, s, (const double*)ws, G, dgamma, dbeta);
    return launch_status("ln_bwd");
}

extern "C" int bg_dropout_add_fwd(const void* branch, int branch_dtype, const void* skip, void* out, int stream_dtype, int M, int C, int B,
                                  double p, unsigned long long seed, unsigned draw_id, int site, long long first_sample, bg_stream_t stream) {
    BG_REQUIRE(lt_is_16(branch_dtype), BG_E_DTYPE, "bg_dropout_add_fwd: branch dtype %d (BG_BF16 or BG_F16)", branch_dtype);
    BG_REQUIRE(stream_dtype == BG_F32 || stream_dtype == branch_dtype, BG_E_DTYPE,
               "bg_dropout_add_fwd: stream dtype %d is neither BG_F32 nor the branch dtype %d", stream_dtype, branch_dtype);
    LtDrop k;
    if (int rc = lt_drop_args("bg_dropout_add_fwd", M, C, B, p, seed, draw_id, site, first_sample, k)) return rc;
    BG_REQUIRE(M == 0 || (branch && skip && out), BG_E_ARG, "bg_dropout_add_fwd: null pointer (branch, skip, out)");
    BG_REQUIRE(aligned(branch, 16) && aligned(skip, 16) && aligned(out, 16), BG_E_ALIGN, "bg_dropout_add_fwd: 16-byte alignment of branch / skip / out");
    if (M == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(lt_chunk_grid(k));
    with_bools(branch_dtype == BG_F16, k.thr != 0, [&](auto F16, auto DROP) {      // the stream: fp32 or the branch's own dtype
        constexpr int BD = F16() ? BG_F16 : BG_BF16;
        if (stream_dtype == BG_F32) hipLaunchKernelGGL((lt_dropout_add_kernel<BG_F32, BD, DROP()>), grid, dim3(256), 0, s, branch, skip, out, k);
        else hipLaunchKernelGGL((lt_dropout_add_kernel<BD, BD, DROP()>), grid, dim3(256), 0, s, branch, skip, out, k);
    });
    return launch_status("dropout_add_fwd");
}

extern "C" int bg_dropout_bwd(const void* dout, int stream_dtype, void* dbranch, int branch_dtype, int M, int C, int B, double p,
                              unsigned long long seed, unsigned draw_id, int site, long long first_sample, bg_stream_t stream) {
    BG_REQUIRE(lt_is_16(branch_dtype), BG_E_DTYPE, "bg_dropout_bwd: branch dtype %d (BG_BF16 or BG_F16)", branch_dtype);
    BG_REQUIRE(stream_dtype == BG_F32 || stream_dtype == branch_dtype, BG_E_DTYPE,
               "bg_dropout_bwd: stream dtype %d is neither BG_F32 nor the branch dtype %d", stream_dtype, branch_dtype);
    LtDrop k;
    if (int rc = lt_drop_args("bg_dropout_bwd", M, C, B, p, seed, draw_id, site, first_sample, k)) return rc;
    BG_REQUIRE(M == 0 || (dout && dbranch), BG_E_ARG, "bg_dropout_bwd: null pointer (dout, dbranch)");
    BG_REQUIRE(aligned(dout, 16) && aligned(dbranch, 16), BG_E_ALIGN, "bg_dropout_bwd: 16-byte alignment of dout / dbranch");
    if (M == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(lt_chunk_grid(k));
    with_bools(branch_dtype == BG_F16, k.thr != 0, [&](auto F16, auto DROP) {
        constexpr int BD = F16() ? BG_F16 : BG_BF16;
        if (stream_dtype == BG_F32) hipLaunchKernelGGL((lt_dropout_bwd_kernel<BG_F32, BD, DROP()>), grid, dim3(256), 0, s, dout, dbranch, k);
        else hipLaunchKernelGGL((lt_dropout_bwd_kernel<BD, BD, DROP()>), grid, dim3(256), 0, s, dout, dbranch, k);
    });
    return launch_status("dropout_bwd");
}

extern "C" int bg_relu_dropout_fwd(const void* x, void* h, int dtype, int M, int C, int B, double p, unsigned long long seed, unsigned draw_id,
                                   int site, long long first_sample, bg_stream_t stream) {
    BG_REQUIRE(lt_is_16(dtype), BG_E_DTYPE, "bg_relu_dropout_fwd: dtype %d (BG_BF16 or BG_F16)", dtype);
    LtDrop k;
    if (int rc = lt_drop_args("bg_relu_dropout_fwd", M, C, B, p, seed, draw_id, site, first_sample, k)) return rc;
    BG_REQUIRE(M == 0 || (x && h), BG_E_ARG, "bg_relu_dropout_fwd: null pointer (x, h)");
    BG_REQUIRE(aligned(x, 16) && aligned(h, 16), BG_E_ALIGN, "bg_relu_dropout_fwd: 16-byte alignment of x / h");
    if (M == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(lt_chunk_grid(k));
    with_bools(dtype == BG_F16, k.thr != 0, [&](auto F16, auto DROP) {
        hipLaunchKernelGGL((lt_relu_dropout_kernel<F16() ? BG_F16 : BG_BF16, DROP()>), grid, dim3(256), 0, s, x, h, k);
    });
    return launch_status("relu_dropout_fwd");
}

extern "C" int bg_relu_dropout_bwd(const void* h, const void* dh, void* dx, int dtype, int M, int C, double p, bg_stream_t stream) {
    BG_REQUIRE(lt_is_16(dtype), BG_E_DTYPE, "bg_relu_dropout_bwd: dtype %d (BG_BF16 or BG_F16)", dtype);
    LtDrop k;
    if (int rc = lt_drop_args("bg_relu_dropout_bwd", M, C, 1, p, 0, 0, 0, 0, k)) return rc;
    BG_REQUIRE(M == 0 || (h && dh && dx), BG_E_ARG, "bg_relu_dropout_bwd: null pointer (h, dh, dx)");
    BG_REQUIRE(aligned(h, 16) && aligned(dh, 16) && aligned(dx, 16), BG_E_ALIGN, "bg_relu_dropout_bwd: 16-byte alignment of h / dh / dx");
    if (M == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(lt_chunk_grid(k));
    if (dtype == BG_F16) hipLaunchKernelGGL((lt_relu_dropout_bwd_kernel<BG_F16>), grid, dim3(256), 0, s, h, dh, dx, k);
    else hipLaunchKernelGGL((lt_relu_dropout_bwd_kernel<BG_BF16>), grid, dim3(256), 0, s, h, dh, dx, k);
    return launch_status("relu_dropout_bwd");
}

extern "C" int bg_dropout_mask(uint8_t* mask, int M, int C, int B, double p, unsigned long long seed, unsigned draw_id, int site,
                               long long first_sample, bg_stream_t stream) {
    LtDrop k;
    if (int rc = lt_drop_args("bg_dropout_mask", M, C, B, p, seed, draw_id, site, first_sample, k)) return rc;
    BG_REQUIRE(M == 0 || mask, BG_E_ARG, "bg_dropout_mask: null pointer (mask)");
    BG_REQUIRE(aligned(mask, 8), BG_E_ALIGN, "bg_dropout_mask: 8-byte alignment of mask");
    if (M == 0) return 0;
    hipLaunchKernelGGL(lt_mask_kernel, dim3(lt_chunk_grid(k)), dim3(256), 0, (hipStream_t)stream, mask, k);
    return launch_status("dropout_mask");
}
