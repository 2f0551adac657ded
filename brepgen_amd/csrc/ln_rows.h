// The row kernels of the training LayerNorm over 768 columns, ONE definition for bg_ln_train_fwd / bg_ln_bwd (layer_train.hip, SILU = false)
// and bg_ln_silu_train_fwd / bg_ln_silu_bwd (mlp_train.hip, SILU = true: h = SiLU(LayerNorm(x)), the middle of the denoisers' MLPs).  The
// row statistics, the chain plan of the column sums (lt_chain_rows) and the fp64 merge (lt_ln_reduce, layer_train.hip) are shared; SILU
// only adds the activation to the forward's last step and its derivative to the backward's first.
//
// Layout: a HALF-wave (32 lanes) owns one row of 768 = 32 x 3 x 8 columns; lane l holds the three 8-column chunks l, l + 32, l + 64
// (16 bytes of 16-bit data, 32 bytes of fp32 each), a 256-thread workgroup works on 8 rows at a time.  Row sums: the 8 values of a chunk
// pairwise, the lane's three chunks in order, then a butterfly over the 32 lanes.
#pragma once
#include "bg_common.h"

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
static inline size_t lt_bwd_workspace_bytes(int M) { return M <= 0 ? 0 : (size_t)lt_bwd_wgs(M) * (2 * LT_C) * sizeof(double); }

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
// SiLU and its derivative in fp32: expf and IEEE divisions, as torch's fp32 SiLU (the results may stay fp32)
__device__ __forceinline__ float lt_silu(float u) { return u / (1.0f + expf(-u)); }
__device__ __forceinline__ float lt_silu_grad(float u) {
    const float sg = 1.0f / (1.0f + expf(-u));
    return sg + u * sg * (1.0f - sg);
}

// ---- forward: y = LN(x) (SILU: SiLU(LN(x))) and the rows' (mean, rstd) ----
template <int XD, int YD, bool SILU>
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
            for (int e = 0; e < 8; ++e) {
                o[e] = d[j][e] * rstd * g[j][e] + b[j][e];
                if (SILU) o[e] = lt_silu(o[e]);
            }
            lt_store8<YD>(y, base + (size_t)(l32 + 32 * j) * 8, o);
        }
        if (l32 == 0) *reinterpret_cast<float2*>(stats + 2 * (size_t)row) = make_float2(mean, rstd);
    }
}

// ---- backward ----
// WG: also the column sums dgamma / dbeta.  A workgroup takes chunks of 8 * chain rows (row = chunk * 8 * chain + i * 8 + slot: the
// eight half-waves read eight consecutive rows); a lane adds the <= chain rows of its slot into 2 x 24 fp32 column accumulators, the
// eight slots' chains of a column meet in LDS and are added IN SLOT ORDER in fp64 into the workgroup's running fp64 sums (thread t
// owns quantities t, t + 256, ...; quantity = column for dgamma, 768 + column for dbeta), and the workgroup's 1536 doubles go to
// ws[blockIdx.x][1536] for lt_ln_reduce.  SILU: dy is the gradient of h = SiLU(u), u = xhat * gamma + beta recomputed as the forward
// formed it; the LayerNorm backward runs on du = dy * SiLU'(u).
template <int XD, int YD, bool WG, bool SILU>
__global__ __launch_bounds__(256) void lt_ln_bwd_kernel(const void* __restrict__ dy, const void* __restrict__ x, const float* __restrict__ stats,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        const void* __restrict__ dskip, void* __restrict__ dx, double* __restrict__ ws, int M,
                                                        int chain, int nchunks) {
    __shared__ __attribute__((aligned(16))) float red[WG ? LT_SLOTS * 2 * LT_C : 4];
    const int l32 = threadIdx.x & 31, slot = threadIdx.x >> 5;
    float g[LT_CH][8], b[SILU ? LT_CH : 1][8];
#pragma unroll
    for (int j = 0; j < LT_CH; ++j) {
        lt_load8<BG_F32>(gamma, (size_t)(l32 + 32 * j) * 8, g[j]);
        if (SILU) lt_load8<BG_F32>(beta, (size_t)(l32 + 32 * j) * 8, b[SILU ? j : 0]);
    }
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
                    if (SILU) {
                        const float u = (xh[j][e] - st.x) * st.y * g[j][e] + b[SILU ? j : 0][e];
                        dv[e] = dv[e] * lt_silu_grad(u);
                    }
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

// ws [G][1536] fp64 -> dgamma | dbeta fp32, in the fixed order brepgen_hip.h states for bg_ln_bwd (layer_train.hip)
void lt_ln_reduce(const double* ws, int G, float* dgamma, float* dbeta, hipStream_t s);

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

// the checks and the launch of the forward entry `who` (bg_ln_train_fwd | bg_ln_silu_train_fwd)
template <bool SILU>
static int lt_ln_fwd_entry(const char* who, const void* x, int x_dtype, const float* gamma, const float* beta, void* y, int y_dtype, float* stats,
                           int M, float eps, bg_stream_t stream) {
    BG_REQUIRE(lt_ln_pair_ok(x_dtype, y_dtype), BG_E_DTYPE, "%s: dtype pair x %d -> y %d (x fp32: any y; x 16-bit: y of the same dtype or fp32)", who,
               x_dtype, y_dtype);
    BG_REQUIRE(M >= 0, BG_E_SHAPE, "%s: M = %d is negative", who, M);
    BG_REQUIRE(eps >= 0.f, BG_E_ARG, "%s: eps = %g is negative", who, (double)eps);
    BG_REQUIRE(M == 0 || (x && gamma && beta && y && stats), BG_E_ARG, "%s: null pointer (x, gamma, beta, y, stats)", who);
    BG_REQUIRE(aligned(x, 16) && aligned(gamma, 16) && aligned(beta, 16) && aligned(y, 16) && aligned(stats, 8), BG_E_ALIGN,
               "%s: 16-byte alignment of x / gamma / beta / y, 8-byte alignment of stats", who);
    if (M == 0) return 0;
    const int rows8 = (M + LT_SLOTS - 1) / LT_SLOTS;
    const dim3 grid((unsigned)(rows8 < LT_MAX_WGS ? rows8 : LT_MAX_WGS));
    hipStream_t s = (hipStream_t)stream;
    lt_ln_dispatch(x_dtype, y_dtype, [&](auto pr) {
        hipLaunchKernelGGL((lt_ln_fwd_kernel<decltype(pr)::a, decltype(pr)::b, SILU>), grid, dim3(256), 0, s, x, gamma, beta, y, stats, M, eps);
    });
    return launch_status(who + 3);          // the entry's name without "bg_"
}

// the checks and the launches of the backward entry `who` (bg_ln_bwd: beta and SILU unused | bg_ln_silu_bwd: dskip NULL)
template <bool SILU>
static int lt_ln_bwd_entry(const char* who, const void* dy, int y_dtype, const void* x, int x_dtype, const float* stats, const float* gamma,
                           const float* beta, const void* dskip, void* dx, float* dgamma, float* dbeta, int M, void* workspace,
                           size_t workspace_bytes, bg_stream_t stream) {
    BG_REQUIRE(lt_ln_pair_ok(x_dtype, y_dtype), BG_E_DTYPE, "%s: dtype pair x %d -> y %d (x fp32: any y; x 16-bit: y of the same dtype or fp32)", who,
               x_dtype, y_dtype);
    BG_REQUIRE(M >= 0, BG_E_SHAPE, "%s: M = %d is negative", who, M);
    BG_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), BG_E_ARG, "%s: dgamma and dbeta must be given together or both be null", who);
    BG_REQUIRE(M == 0 || (dy && x && stats && gamma && dx && (!SILU || beta)), BG_E_ARG, "%s: null pointer (dy, x, stats, gamma, %sdx)", who,
               SILU ? "beta, " : "");
    BG_REQUIRE(aligned(dy, 16) && aligned(x, 16) && aligned(gamma, 16) && aligned(beta, 16) && aligned(dskip, 16) && aligned(dx, 16) &&
                   aligned(dgamma, 16) && aligned(dbeta, 16) && aligned(workspace, 16) && aligned(stats, 8),
               BG_E_ALIGN, "%s: 16-byte alignment of dy / x / gamma / %sdskip / dx / dgamma / dbeta / workspace, 8-byte alignment of stats", who,
               SILU ? "beta / " : "");
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        if (dgamma) {
            hipError_t e = hipMemsetAsync(dgamma, 0, LT_C * sizeof(float), s);
            if (e == hipSuccess) e = hipMemsetAsync(dbeta, 0, LT_C * sizeof(float), s);
            BG_REQUIRE(e == hipSuccess, (int)e, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
        }
        return 0;
    }
    const size_t need = dgamma ? lt_bwd_workspace_bytes(M) : 0;
    BG_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need), BG_E_ARG, "%s: workspace of %zu bytes, %zu needed for M = %d", who,
               workspace ? workspace_bytes : (size_t)0, need, M);
    const int chain = lt_chain_rows(M), nchunks = lt_bwd_chunks(M), G = lt_bwd_wgs(M);
    double* ws = reinterpret_cast<double*>(workspace);
    lt_ln_dispatch(x_dtype, y_dtype, [&](auto pr) {
        if (dgamma)
            hipLaunchKernelGGL((lt_ln_bwd_kernel<decltype(pr)::a, decltype(pr)::b, true, SILU>), dim3((unsigned)G), dim3(256), 0, s, dy, x, stats, gamma,
                               beta, dskip, dx, ws, M, chain, nchunks);
        else
            hipLaunchKernelGGL((lt_ln_bwd_kernel<decltype(pr)::a, decltype(pr)::b, false, SILU>), dim3((unsigned)G), dim3(256), 0, s, dy, x, stats, gamma,
                               beta, dskip, dx, ws, M, chain, nchunks);
    });
    if (dgamma) lt_ln_reduce((const double*)ws, G, dgamma, dbeta, s);
    return launch_status(who + 3);
}

}  // namespace bg
