// The denoisers' MLPs and loss in TRAINING: nn.Sequential(Linear(k, 768), LayerNorm, SiLU, Linear(768, n)) with a "thin" side
// k or n <= 48 (the data embeds k = 6 / 12 / 48, fc_out n = 6 / 18 / 48; network.py:1076-1099), and the gradient of the masked MSE.
// include/brepgen_hip.h states every entry.  Nothing is allocated, no atomics: one writer per output element and a fixed order of
// every sum, so two calls give the same bits.
//
//   bg_thin_expand     Y [M, 768] = X [M, s] W + b         a workgroup: 64 rows x 256 columns, W's slab and the X tile in LDS
//   bg_thin_contract   Y [M, n]   = A [M, 768] W^T + b     a half-wave per row (ln_rows.h's layout), W [n, 768] fp32 in LDS
//   bg_thin_wgrad      G [s, 768] = T^T U                  fp32 chains of <= 64 rows per (row slot, k, column), fp64 across
//   bg_ln_silu_*       ln_rows.h's row kernels with SILU = true
//   bg_masked_mse_bwd  elementwise
//
// At s, n = 48 the three products are bound by the fp32 FMA rate (768 * 48 FMAs per row against 1.5 KB of 16-bit row), below that by
// the [M, 768] stream; an MFMA core would lift the first bound and is not attempted.
#include "ln_rows.h"

namespace bg {

constexpr int TH_MAX = 48;                // the thin dimension: 1 .. 48

// one element of a strided fp32 / 16-bit operand (the thin operands are read element-wise: any row stride, element alignment)
__device__ __forceinline__ float th_elem(const void* p, int dt, size_t i) {
    if (dt == BG_F32) return reinterpret_cast<const float*>(p)[i];
    if (dt == BG_F16) return (float)reinterpret_cast<const _Float16*>(p)[i];
    return __uint_as_float((uint32_t)reinterpret_cast<const unsigned short*>(p)[i] << 16);
}

// ---- bg_thin_expand ----
constexpr int TE_ROWS = 64, TE_SLAB = 256, TE_MAX_WGS = 256;       // rows of a tile = 8 slots x 8; columns of a workgroup
template <int YD>
__global__ __launch_bounds__(256) void th_expand_kernel(const void* __restrict__ x, int xdt, int ldx, const float* __restrict__ w, int k_major,
                                                        const float* __restrict__ b, void* __restrict__ y, int M, int s, int ntiles) {
    __shared__ __attribute__((aligned(16))) float wl[TH_MAX * TE_SLAB];        // [k][256 columns of the slab]
    __shared__ float xs[TE_ROWS * TH_MAX];                                      // [row of the tile][k], row stride 48
    const int tid = threadIdx.x, l32 = tid & 31, slot = tid >> 5, c0 = blockIdx.y * TE_SLAB;
    for (int i = tid; i < s * TE_SLAB; i += 256) {
        if (k_major) wl[i] = w[(size_t)(i / TE_SLAB) * LT_C + c0 + (i % TE_SLAB)];
        else wl[(i % s) * TE_SLAB + i / s] = w[(size_t)c0 * s + i];
    }
    float bias[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = b ? b[c0 + l32 * 8 + e] : 0.f;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long r0 = (long long)tile * TE_ROWS;
        __syncthreads();                                   // the previous tile's reads of xs (and, first, the staging of wl)
        for (int i = tid; i < TE_ROWS * s; i += 256) {
            const int r = i / s, k = i - r * s;
            xs[r * TH_MAX + k] = r0 + r < M ? th_elem(x, xdt, (size_t)(r0 + r) * ldx + k) : 0.f;
        }
        __syncthreads();
        float acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[i][e] = bias[e];
        for (int k = 0; k < s; ++k) {
            const float4 w0 = *reinterpret_cast<const float4*>(wl + k * TE_SLAB + l32 * 8), w1 = *reinterpret_cast<const float4*>(wl + k * TE_SLAB + l32 * 8 + 4);
            const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float xv = xs[(i * 8 + slot) * TH_MAX + k];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[i][e] = __builtin_fmaf(xv, wv[e], acc[i][e]);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long long row = r0 + i * 8 + slot;
            if (row < M) lt_store8<YD>(y, (size_t)row * LT_C + c0 + l32 * 8, acc[i]);
        }
    }
}

// ---- bg_thin_contract ----
constexpr int TC_THREADS = 1024, TC_R = 2, TC_ROWS = TC_THREADS / 32 * TC_R, TC_MAX_WGS = 256;      // 32 half-waves x 2 rows
template <int AD>
__global__ __launch_bounds__(TC_THREADS) void th_contract_kernel(const void* __restrict__ a, const float* __restrict__ w, const float* __restrict__ b,
                                                                 float* __restrict__ y, int M, int n, int ntiles) {
    __shared__ __attribute__((aligned(16))) float wl[TH_MAX * LT_C];            // W [n, 768] as it lies
    const int tid = threadIdx.x, l32 = tid & 31, slot = tid >> 5;
    for (int i = tid; i < n * (LT_C / 4); i += TC_THREADS) reinterpret_cast<float4*>(wl)[i] = reinterpret_cast<const float4*>(w)[i];
    __syncthreads();
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long r0 = (long long)tile * TC_ROWS + slot * TC_R;
        float av[TC_R][LT_CH][8];
#pragma unroll
        for (int r = 0; r < TC_R; ++r)
#pragma unroll
            for (int c = 0; c < LT_CH; ++c) {
                if (r0 + r < M) lt_load8<AD>(a, (size_t)(r0 + r) * LT_C + (size_t)(l32 + 32 * c) * 8, av[r][c]);
                else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) av[r][c][e] = 0.f;
                }
            }
        float keep[TC_R][2];
#pragma unroll
        for (int r = 0; r < TC_R; ++r) keep[r][0] = keep[r][1] = 0.f;
        for (int j = 0; j < n; ++j) {
            float p[TC_R];
#pragma unroll
            for (int r = 0; r < TC_R; ++r) p[r] = 0.f;
#pragma unroll
            for (int c = 0; c < LT_CH; ++c) {
                const float* at = wl + j * LT_C + (l32 + 32 * c) * 8;
                const float4 w0 = *reinterpret_cast<const float4*>(at), w1 = *reinterpret_cast<const float4*>(at + 4);
                const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e)
#pragma unroll
                    for (int r = 0; r < TC_R; ++r) p[r] = __builtin_fmaf(av[r][c][e], wv[e], p[r]);
            }
            const float bj = b ? b[j] : 0.f;
#pragma unroll
            for (int r = 0; r < TC_R; ++r) {
                const float v = lt_half_sum(p[r]) + bj;
                if (l32 == (j & 31)) {                               // j < 64: two values per lane and row
                    if (j < 32) keep[r][0] = v;
                    else keep[r][1] = v;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < TC_R; ++r) {
            if (r0 + r < M) {
                if (l32 < n) y[(size_t)(r0 + r) * n + l32] = keep[r][0];
                if (32 + l32 < n) y[(size_t)(r0 + r) * n + 32 + l32] = keep[r][1];
            }
        }
    }
}

// ---- bg_thin_wgrad ----
constexpr int TW_KG = 8, TW_SLAB = 256, TW_WGS = 256;                           // k's and columns of a workgroup; workgroups in all, about
constexpr int TW_Q = TW_KG * TW_SLAB;                                           // a slot's fp32 chains of the product, met in LDS
constexpr int TW_QC = TW_SLAB + TW_KG;                                          // a slot's fp64 column sums (of U | of T): the same LDS, after
constexpr int TW_FOLD = 8;                                                      // rows per fp32 chain of a column sum
struct TwPlan { int kgroups, s8, chain, nchunks, G; };
static inline TwPlan tw_plan(int M, int s) {
    TwPlan p;
    p.kgroups = (s + TW_KG - 1) / TW_KG;
    p.s8 = p.kgroups * TW_KG;
    const int cap = TW_WGS / p.kgroups;                                         // row workgroups: 256, 128, 85, 64, 51, 42
    const int r = (int)(((long long)M + 8ll * cap - 1) / (8ll * cap));
    p.chain = r < LT_CHAIN_MIN ? LT_CHAIN_MIN : (r > LT_CHAIN_MAX ? LT_CHAIN_MAX : r);
    p.nchunks = (int)(((long long)M + 8 * p.chain - 1) / (8 * p.chain));
    p.G = p.nchunks < cap ? p.nchunks : cap;
    return p;
}
static inline size_t tw_workspace_bytes(int M, int s) {
    if (M <= 0 || s < 1 || s > TH_MAX) return 0;
    const TwPlan p = tw_plan(M, s);
    return (size_t)p.G * ((size_t)p.s8 * LT_C + LT_C + p.s8) * sizeof(double);
}
// colsum_of: 0 none, 1 U's columns (workgroups of k group 0), 2 T's columns (workgroups of slab 0).  A column sum has full-mantissa
// addends and no product to hide behind: its fp32 chains are 8 rows, folded into the lane's fp64 sum (64-row chains measured 2.2 x
// the error of torch's tree reduction at 43 597 rows).
template <int UD>
__global__ __launch_bounds__(256) void th_wgrad_kernel(const void* __restrict__ t, int tdt, int ldt, const void* __restrict__ u, double* __restrict__ ws_g,
                                                       double* __restrict__ ws_u, double* __restrict__ ws_t, int M, int s, int s8, int chain, int nchunks,
                                                       int colsum_of) {
    __shared__ __attribute__((aligned(16))) float red[LT_SLOTS][TW_Q];
    const int tid = threadIdx.x, l32 = tid & 31, slot = tid >> 5, slab = blockIdx.y, k0 = blockIdx.z * TW_KG;
    const int kc = s - k0 < TW_KG ? s - k0 : TW_KG;
    const bool sum_u = colsum_of == 1 && blockIdx.z == 0, sum_t = colsum_of == 2 && slab == 0;
    double tot[TW_KG], totu = 0.0, tott = 0.0;
#pragma unroll
    for (int k = 0; k < TW_KG; ++k) tot[k] = 0.0;
    for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        float acc[TW_KG][8], au[8], at[TW_KG];
        double dau[8], dat[TW_KG];
#pragma unroll
        for (int k = 0; k < TW_KG; ++k) {
            at[k] = 0.f, dat[k] = 0.0;
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) au[e] = 0.f, dau[e] = 0.0;
        const long long row0 = (long long)chunk * (LT_SLOTS * chain) + slot;
        for (int i = 0; i < chain; ++i) {
            const long long row = row0 + (long long)i * LT_SLOTS;
            if (row >= M) break;
            float uv[8], tv[TW_KG];
            lt_load8<UD>(u, (size_t)row * LT_C + slab * TW_SLAB + l32 * 8, uv);
#pragma unroll
            for (int k = 0; k < TW_KG; ++k) tv[k] = k < kc ? th_elem(t, tdt, (size_t)row * ldt + k0 + k) : 0.f;
#pragma unroll
            for (int k = 0; k < TW_KG; ++k) {
                if (k < kc) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[k][e] = __builtin_fmaf(tv[k], uv[e], acc[k][e]);
                }
            }
            if (sum_u) {
#pragma unroll
                for (int e = 0; e < 8; ++e) au[e] += uv[e];
            }
            if (sum_t) {
#pragma unroll
                for (int k = 0; k < TW_KG; ++k) at[k] += tv[k];
            }
            if ((sum_u || sum_t) && (i & (TW_FOLD - 1)) == TW_FOLD - 1) {
#pragma unroll
                for (int e = 0; e < 8; ++e) dau[e] += (double)au[e], au[e] = 0.f;
#pragma unroll
                for (int k = 0; k < TW_KG; ++k) dat[k] += (double)at[k], at[k] = 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) dau[e] += (double)au[e];                       // the chain the loop left open
#pragma unroll
        for (int k = 0; k < TW_KG; ++k) dat[k] += (double)at[k];
#pragma unroll
        for (int k = 0; k < TW_KG; ++k) {
            float* to = &red[slot][k * TW_SLAB + l32 * 8];
            *reinterpret_cast<float4*>(to) = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
            *reinterpret_cast<float4*>(to + 4) = make_float4(acc[k][4], acc[k][5], acc[k][6], acc[k][7]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < TW_KG; ++k)
#pragma unroll
            for (int sl = 0; sl < LT_SLOTS; ++sl) tot[k] += (double)red[sl][k * TW_SLAB + tid];
        __syncthreads();
        if (sum_u || sum_t) {                                                      // uniform over the workgroup
            double* rc = reinterpret_cast<double*>(&red[0][0]);                    // [slot][TW_QC] doubles: 17 KB of the 64
#pragma unroll
            for (int e = 0; e < 8; ++e) rc[slot * TW_QC + l32 * 8 + e] = dau[e];
            if (l32 == 0) {
#pragma unroll
                for (int k = 0; k < TW_KG; ++k) rc[slot * TW_QC + TW_SLAB + k] = dat[k];
            }
            __syncthreads();
#pragma unroll
            for (int sl = 0; sl < LT_SLOTS; ++sl) {
                totu += rc[sl * TW_QC + tid];
                if (tid < TW_KG) tott += rc[sl * TW_QC + TW_SLAB + tid];
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < TW_KG; ++k) ws_g[((size_t)blockIdx.x * s8 + k0 + k) * LT_C + slab * TW_SLAB + tid] = tot[k];
    if (sum_u) ws_u[(size_t)blockIdx.x * LT_C + slab * TW_SLAB + tid] = totu;
    if (sum_t && tid < TW_KG) ws_t[(size_t)blockIdx.x * s8 + k0 + tid] = tott;
}
// one thread per output: the G workgroup partials of a quantity in index order, in fp64, rounded once
__global__ __launch_bounds__(256) void th_wgrad_reduce_kernel(const double* __restrict__ ws_g, const double* __restrict__ ws_u, const double* __restrict__ ws_t,
                                                              int G, int s, int s8, float* __restrict__ g, int g_transposed, float* __restrict__ colsum,
                                                              int colsum_of) {
    const int q = blockIdx.x * 256 + threadIdx.x, nq = s * LT_C;
    const int extra = colsum_of == 1 ? LT_C : (colsum_of == 2 ? s : 0);
    if (q >= nq + extra) return;
    const double* from;
    size_t stride;
    float* to;
    if (q < nq) {
        const int k = q / LT_C, c = q - k * LT_C;
        from = ws_g + (size_t)k * LT_C + c, stride = (size_t)s8 * LT_C;
        to = g_transposed ? g + (size_t)c * s + k : g + q;
    } else if (colsum_of == 1) {
        from = ws_u + (q - nq), stride = LT_C, to = colsum + (q - nq);
    } else {
        from = ws_t + (q - nq), stride = (size_t)s8, to = colsum + (q - nq);
    }
    double a = 0.0;
#pragma unroll 8
    for (int w = 0; w < G; ++w) a += from[(size_t)w * stride];
    *to = (float)a;
}

// ---- bg_masked_mse_bwd ----
__global__ __launch_bounds__(256) void mse_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const uint8_t* __restrict__ mask,
                                                      long long rows, int ld, int col0, int ncols, const float* __restrict__ out3,
                                                      const float* __restrict__ g, float* __restrict__ dpred) {
    const float valid = out3[2];
    const bool any = valid > 0.f;
    const float coef = any ? (2.0f * g[0]) / (valid * (float)ncols) : 0.f;
    const long long total = rows * ld;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / ld;
        const int c = (int)(i - r * ld);
        const bool in = any && c >= col0 && c < col0 + ncols && !(mask != nullptr && mask[r]);
        dpred[i] = in ? (pred[i] - target[i]) * coef : 0.f;            // a select: NaN / Inf outside the compared elements is never read
    }
}

static inline int th_dtype16(int d) { return d == BG_F16 || d == BG_BF16; }

}  // namespace bg

using namespace bg;

extern "C" int bg_thin_expand(const void* x, int x_dtype, int ldx, const float* w, int w_k_major, const float* b, void* y, int y_dtype, int M,
                              int s, bg_stream_t stream) {
    BG_REQUIRE(lt_is_dtype(x_dtype) && lt_is_dtype(y_dtype), BG_E_DTYPE, "bg_thin_expand: dtype x %d / y %d (BG_F32, BG_F16 or BG_BF16)", x_dtype,
               y_dtype);
    BG_REQUIRE(s >= 1 && s <= TH_MAX, BG_E_SHAPE, "bg_thin_expand: s = %d outside 1 .. %d", s, TH_MAX);
    BG_REQUIRE(M >= 0, BG_E_SHAPE, "bg_thin_expand: M = %d is negative", M);
    BG_REQUIRE(ldx >= s, BG_E_SHAPE, "bg_thin_expand: ldx = %d is below s = %d", ldx, s);
    BG_REQUIRE(M == 0 || (x && w && y), BG_E_ARG, "bg_thin_expand: null pointer (x, w, y)");
    BG_REQUIRE(aligned(y, 16) && aligned(w, 4) && aligned(b, 4) && aligned(x, x_dtype == BG_F32 ? 4 : 2), BG_E_ALIGN,
               "bg_thin_expand: 16-byte alignment of y, element alignment of x / w / b");
    if (M == 0) return 0;
    const int ntiles = (M + TE_ROWS - 1) / TE_ROWS;
    const dim3 grid((unsigned)(ntiles < TE_MAX_WGS ? ntiles : TE_MAX_WGS), LT_C / TE_SLAB);
    hipStream_t st = (hipStream_t)stream;
    if (y_dtype == BG_F32) hipLaunchKernelGGL((th_expand_kernel<BG_F32>), grid, dim3(256), 0, st, x, x_dtype, ldx, w, w_k_major, b, y, M, s, ntiles);
    else if (y_dtype == BG_F16) hipLaunchKernelGGL((th_expand_kernel<BG_F16>), grid, dim3(256), 0, st, x, x_dtype, ldx, w, w_k_major, b, y, M, s, ntiles);
    else hipLaunchKernelGGL((th_expand_kernel<BG_BF16>), grid, dim3(256), 0, st, x, x_dtype, ldx, w, w_k_major, b, y, M, s, ntiles);
    return launch_status("thin_expand");
}

extern "C" int bg_thin_contract(const void* a, int a_dtype, const float* w, const float* b, float* y, int M, int n, bg_stream_t stream) {
    BG_REQUIRE(th_dtype16(a_dtype), BG_E_DTYPE, "bg_thin_contract: a dtype %d (BG_BF16 or BG_F16)", a_dtype);
    BG_REQUIRE(n >= 1 && n <= TH_MAX, BG_E_SHAPE, "bg_thin_contract: n = %d outside 1 .. %d", n, TH_MAX);
    BG_REQUIRE(M >= 0, BG_E_SHAPE, "bg_thin_contract: M = %d is negative", M);
    BG_REQUIRE(M == 0 || (a && w && y), BG_E_ARG, "bg_thin_contract: null pointer (a, w, y)");
    BG_REQUIRE(aligned(a, 16) && aligned(w, 16) && aligned(b, 4) && aligned(y, 4), BG_E_ALIGN,
               "bg_thin_contract: 16-byte alignment of a / w, element alignment of b / y");
    if (M == 0) return 0;
    const int ntiles = (M + TC_ROWS - 1) / TC_ROWS;
    const dim3 grid((unsigned)(ntiles < TC_MAX_WGS ? ntiles : TC_MAX_WGS));
    hipStream_t st = (hipStream_t)stream;
    if (a_dtype == BG_F16) hipLaunchKernelGGL((th_contract_kernel<BG_F16>), grid, dim3(TC_THREADS), 0, st, a, w, b, y, M, n, ntiles);
    else hipLaunchKernelGGL((th_contract_kernel<BG_BF16>), grid, dim3(TC_THREADS), 0, st, a, w, b, y, M, n, ntiles);
    return launch_status("thin_contract");
}

extern "C" size_t bg_thin_wgrad_workspace_bytes(int M, int s) { return tw_workspace_bytes(M, s); }

extern "C" int bg_thin_wgrad(const void* t, int t_dtype, int ldt, const void* u, int u_dtype, float* g, int g_transposed, float* colsum,
                             int colsum_of, int M, int s, void* workspace, size_t workspace_bytes, bg_stream_t stream) {
    BG_REQUIRE(lt_is_dtype(t_dtype), BG_E_DTYPE, "bg_thin_wgrad: t dtype %d (BG_F32, BG_F16 or BG_BF16)", t_dtype);
    BG_REQUIRE(th_dtype16(u_dtype), BG_E_DTYPE, "bg_thin_wgrad: u dtype %d (BG_BF16 or BG_F16)", u_dtype);
    BG_REQUIRE(s >= 1 && s <= TH_MAX, BG_E_SHAPE, "bg_thin_wgrad: s = %d outside 1 .. %d", s, TH_MAX);
    BG_REQUIRE(M >= 0, BG_E_SHAPE, "bg_thin_wgrad: M = %d is negative", M);
    BG_REQUIRE(ldt >= s, BG_E_SHAPE, "bg_thin_wgrad: ldt = %d is below s = %d", ldt, s);
    BG_REQUIRE(colsum_of >= 0 && colsum_of <= 2 && (colsum_of == 0) == (colsum == nullptr), BG_E_ARG,
               "bg_thin_wgrad: colsum_of = %d (0 none, 1 of u, 2 of t) must go with a colsum pointer exactly when it is not 0", colsum_of);
    BG_REQUIRE(g && (M == 0 || (t && u)), BG_E_ARG, "bg_thin_wgrad: null pointer (t, u, g)");
    BG_REQUIRE(aligned(u, 16) && aligned(g, 4) && aligned(colsum, 4) && aligned(workspace, 16) && aligned(t, t_dtype == BG_F32 ? 4 : 2), BG_E_ALIGN,
               "bg_thin_wgrad: 16-byte alignment of u / workspace, element alignment of t / g / colsum");
    hipStream_t st = (hipStream_t)stream;
    if (M == 0) {
        hipError_t e = hipMemsetAsync(g, 0, (size_t)s * LT_C * sizeof(float), st);
        if (e == hipSuccess && colsum) e = hipMemsetAsync(colsum, 0, (size_t)(colsum_of == 1 ? LT_C : s) * sizeof(float), st);
        BG_REQUIRE(e == hipSuccess, (int)e, "bg_thin_wgrad: hipMemsetAsync: %s", hipGetErrorString(e));
        return 0;
    }
    const size_t need = tw_workspace_bytes(M, s);
    BG_REQUIRE(workspace != nullptr && workspace_bytes >= need, BG_E_ARG, "bg_thin_wgrad: workspace of %zu bytes, %zu needed for M = %d, s = %d",
               workspace ? workspace_bytes : (size_t)0, need, M, s);
    const TwPlan p = tw_plan(M, s);
    double* ws_g = reinterpret_cast<double*>(workspace);
    double* ws_u = ws_g + (size_t)p.G * p.s8 * LT_C;
    double* ws_t = ws_u + (size_t)p.G * LT_C;
    const dim3 grid((unsigned)p.G, LT_C / TW_SLAB, (unsigned)p.kgroups);
    if (u_dtype == BG_F16)
        hipLaunchKernelGGL((th_wgrad_kernel<BG_F16>), grid, dim3(256), 0, st, t, t_dtype, ldt, u, ws_g, ws_u, ws_t, M, s, p.s8, p.chain, p.nchunks, colsum_of);
    else
        hipLaunchKernelGGL((th_wgrad_kernel<BG_BF16>), grid, dim3(256), 0, st, t, t_dtype, ldt, u, ws_g, ws_u, ws_t, M, s, p.s8, p.chain, p.nchunks, colsum_of);
    const int nq = s * LT_C + (colsum_of == 1 ? LT_C : (colsum_of == 2 ? s : 0));
    hipLaunchKernelGGL(th_wgrad_reduce_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, (const double*)ws_g, (const double*)ws_u,
                       (const double*)ws_t, p.G, s, p.s8, g, g_transposed, colsum, colsum_of);
    return launch_status("thin_wgrad");
}

extern "C" int bg_ln_silu_train_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* h, int h_dtype, float* stats, int M,
                                    float eps, bg_stream_t stream) {
    return lt_ln_fwd_entry<true>("bg_ln_silu_train_fwd", x, x_dtype, gamma, beta, h, h_dtype, stats, M, eps, stream);
}

extern "C" size_t bg_ln_silu_bwd_workspace_bytes(int M) { return lt_bwd_workspace_bytes(M); }

extern "C" int bg_ln_silu_bwd(const void* dh, int h_dtype, const void* x, int x_dtype, const float* stats, const float* gamma, const float* beta,
                              void* dx, float* dgamma, float* dbeta, int M, void* workspace, size_t workspace_bytes, bg_stream_t stream) {
    return lt_ln_bwd_entry<true>("bg_ln_silu_bwd", dh, h_dtype, x, x_dtype, stats, gamma, beta, nullptr, dx, dgamma, dbeta, M, workspace,
                                 workspace_bytes, stream);
}

extern "C" int bg_masked_mse_bwd(const float* pred, const float* target, const uint8_t* row_mask, long long rows, int ld, int col0, int ncols,
                                 const float* out3, const float* g, float* dpred, bg_stream_t stream) {
    BG_REQUIRE(pred && target && out3 && g && dpred, BG_E_ARG, "bg_masked_mse_bwd: null pointer (pred, target, out3, g, dpred)");
    BG_REQUIRE(rows >= 0 && ncols > 0 && col0 >= 0 && col0 + ncols <= ld, BG_E_SHAPE, "bg_masked_mse_bwd: bad shape rows=%lld ld=%d col0=%d ncols=%d",
               rows, ld, col0, ncols);
    if (rows == 0) return 0;
    const long long blocks = (rows * ld + 255) / 256;
    hipLaunchKernelGGL(mse_bwd_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, pred, target, row_mask, rows,
                       ld, col0, ncols, out3, g, dpred);
    return launch_status("masked_mse_bwd");
}
