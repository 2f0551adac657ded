// What the two weight-gradient kernels share (linear_bwd.hip: lb_wgrad_kernel, conv_train.hip: cw_wgrad_kernel): the row-major
// LDS image of a 32 x 128 operand piece and its transpose-read fragments, the staged-dY bias sum, the host-side slice plan, and the
// checked body of their two entries (lb_wgrad_entry).
// Both kernels reduce over the ROW index of both operands in steps of LB_RS rows; they differ in where a row of the second
// operand comes from (a row of X; the pixel a tap shifts to, or zeros).  See linear_bwd.hip for the organisation.  The tile-body
// helpers below (lb_frag_offsets .. lb_store_db) are lb_wgrad_kernel's body, statement for statement; that kernel keeps its inline
// copy because compiling it through the helpers changes its register allocation and schedule.
#pragma once
#include "gemm16.h"

namespace bg {

typedef __attribute__((ext_vector_type(4))) short lb_v4s;

constexpr int LB_RS = 32;                  // rows of M per step
constexpr int LB_IMG = LB_RS * 256;        // one operand image: 32 rows x 128 16-bit columns
constexpr int LB_MAX_SPLIT = 64;
// AUTO split ("The Linear layers' backward"): aim for LB_TARGET_WGS tile x slice workgroups (two per CU), with at least
// LB_MIN_STEPS row steps per slice
constexpr int LB_TARGET_WGS = 512;
constexpr int LB_MIN_STEPS = 8;

// byte offset of 16-byte chunk ch (0..15) of image row `row`: the guide's dual-use image with plain 256-byte rows.  The sixteen
// 16-byte slots a 32-lane half of a transpose read touches (4 rows x 4 chunks) fall on sixteen distinct slots of the 256-byte bank row
__device__ __forceinline__ unsigned lb_off(int row, int ch) { return 256u * row + 16u * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

// eight consecutive rows of one column, as an MFMA fragment: rows r .. r + 3 from `p`, r + 4 .. r + 7 from `p4`
template <bool F16> __device__ __forceinline__ typename Elem<F16>::V8 lb_frag(const unsigned char* p, const unsigned char* p4) {
    union { lb_v4s s4[2]; typename Elem<F16>::V8 v; } u;
    u.s4[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lb_v4s*)p);
    u.s4[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) lb_v4s*)p4);
    return u.v;
}

template <bool F16> __device__ __forceinline__ void lb_add8(float (&acc)[8], uint4 v) {
    float f[4];
    unpack4_16<F16>(make_uint2(v.x, v.y), f);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += f[e];
    unpack4_16<F16>(make_uint2(v.z, v.w), f);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[4 + e] += f[e];
}

// ---- fragment addresses.  16-lane group gg = lane >> 4 reads the block of rows 8 h + {0..3} (second read: + 4) and columns
// 16 (gg & 1) .. + 15 of a 32-column MFMA tile; lane 4 q + p of the group supplies row q, columns 4 p .. 4 p + 3 and receives
// the four rows of column (lane & 15): column (lane & 31) of the tile, reduction slots 8 h .. 8 h + 7 = the MFMA's operand map ----
__device__ __forceinline__ void lb_frag_offsets(int lane, int wn, int wk, unsigned (&a_off)[2][2], unsigned (&b_off)[2][2]) {
    const int gi = lane & 15, gg = lane >> 4, h = gg >> 1;
    const int fq = gi >> 2, fp = gi & 3;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int row = 8 * h + 4 * s + fq;
            a_off[t][s] = lb_off(row, 8 * wn + 4 * t + 2 * (gg & 1) + (fp >> 1)) + 8u * (fp & 1);
            b_off[t][s] = lb_off(row, 8 * wk + 4 * t + 2 * (gg & 1) + (fp >> 1)) + 8u * (fp & 1) + LB_IMG;
        }
}

__device__ __forceinline__ void lb_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int ki = 0; ki < 2; ++ki)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ni][ki][r] = 0.f;
}

// the products of one staged step: img = [dY image | second-operand image] of LB_RS rows
template <bool F16>
__device__ __forceinline__ void lb_step(const unsigned char* img, const unsigned (&a_off)[2][2], const unsigned (&b_off)[2][2], f32x16 (&acc)[2][2]) {
    using E = Elem<F16>;
    using V8 = typename E::V8;
#pragma unroll
    for (int ks = 0; ks < LB_RS / 16; ++ks) {
        V8 a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t] = lb_frag<F16>(img + a_off[t][0] + ks * 16 * 256, img + a_off[t][1] + ks * 16 * 256);
            b[t] = lb_frag<F16>(img + b_off[t][0] + ks * 16 * 256, img + b_off[t][1] + ks * 16 * 256);
        }
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int ki = 0; ki < 2; ++ki) acc[ni][ki] = E::mfma(a[ni], b[ki], acc[ni][ki]);
    }
}

// a wave's 64 x 64 quarter of the tile: first row n_w, first column k_w of an output with row stride K at `out_base`.
// OUT: 0 / 1 = fp32, 2 = the operand dtype
template <bool F16, int OUT>
__device__ __forceinline__ void lb_store_tile(const f32x16 (&acc)[2][2], void* dw_, size_t out_base, int K, int n_w, int k_w, int lane) {
    using T = typename Elem<F16>::T;
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int ki = 0; ki < 2; ++ki)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n_w + 32 * ni + (r & 3) + 8 * (r >> 2) + 4 * h;
                const size_t at = out_base + (size_t)n * K + (k_w + 32 * ki + l31);
                if (OUT == 2) reinterpret_cast<T*>(dw_)[at] = cvt16<T>(acc[ni][ki][r]);
                else reinterpret_cast<float*>(dw_)[at] = acc[ni][ki][r];
            }
}

// the bias gradient of a tile's 128 columns from the staging threads' sums (thread = 8 columns sc = tid & 15, row group tid >> 4):
// the sixteen row groups in index order, written at db_[at0 ..]
template <bool F16, int OUT>
__device__ __forceinline__ void lb_store_db(const float (&dbacc)[8], unsigned char* lds, void* db_, size_t at0, int tid) {
    using T = typename Elem<F16>::T;
    const int sc = tid & 15, sr = tid >> 4;
    __syncthreads();                                  // the images are dead
    float* red = reinterpret_cast<float*>(lds);       // [16 row groups][128 columns]
#pragma unroll
    for (int e = 0; e < 8; ++e) red[sr * 128 + sc * 8 + e] = dbacc[e];
    __syncthreads();
    if (tid < 128) {
        float v = red[tid];
#pragma unroll
        for (int g = 1; g < 16; ++g) v += red[g * 128 + tid];
        const size_t at = at0 + tid;
        if (OUT == 2) reinterpret_cast<T*>(db_)[at] = cvt16<T>(v);
        else reinterpret_cast<float*>(db_)[at] = v;
    }
}

// ---- host-side plan ----
static inline int lb_steps(int M) { return (M + LB_RS - 1) / LB_RS; }
// rows per slice: whole row steps, the same for every slice but the last
static inline int lb_slice_rows(int M, int S) { return ((lb_steps(M) + S - 1) / S) * LB_RS; }
static inline bool lb_no_empty_slice(int M, int S) { return (long long)(S - 1) * lb_slice_rows(M, S) < (long long)M; }

static inline int lb_auto_split(int M, int N, int K) {
    const int steps = lb_steps(M);
    const long long tiles = (long long)(N / 128) * (K / 128);
    long long S = LB_TARGET_WGS / tiles;
    if (S > steps / LB_MIN_STEPS) S = steps / LB_MIN_STEPS;
    if (S > LB_MAX_SPLIT) S = LB_MAX_SPLIT;
    if (S < 1) S = 1;
    while (S > 1 && !lb_no_empty_slice(M, (int)S)) --S;
    return (int)S;
}

static inline size_t lb_workspace(int N, int K, int S) {
    if (S <= 1) return 0;
    return ((size_t)S * N * ((size_t)K + 1) * sizeof(float) + 255) & ~(size_t)255;
}

// dW [N, K] / db [N] (db may be null) = the S fp32 partials of `ws` ([S][N][K], then [S][N]) added in index order, written in fp32 or
// (out16) the 16-bit dtype: lb_reduce_kernel (linear_bwd.hip)
void lb_reduce(hipStream_t s, bool f16, bool out16, const float* ws, void* dw, void* db, int S, int N, int K);

// ---- the checked body of the two entries (bg_linear_wgrad | bg_conv_wgrad).  An entry calls lb_wgrad_dtypes, makes its own shape
// checks, and hands over M x N times M x K with the words of its messages: `op` names the second operand (x | a), `red` its width
// (K | C, the least ld_op: min_ld_op), `stride` the strides (row | pixel).  empty_ok: trailing slices may be empty (the conv kernel
// zero-fills them; bg_linear_wgrad rejects such a split).  launch(F16 constant, OUT constant, grid, dw, db, slice_rows) enqueues the
// entry's tile kernel: OUT 0 writes fp32 partials to the workspace, which lb_reduce then adds up; 1 / 2 write dW / db themselves ----
static int lb_wgrad_dtypes(const char* who, int dtype, int out_dtype) {
    BG_REQUIRE(dtype == BG_BF16 || dtype == BG_F16, BG_E_DTYPE, "%s: operand dtype %d (BG_BF16 or BG_F16)", who, dtype);
    BG_REQUIRE(out_dtype == BG_F32 || out_dtype == dtype, BG_E_DTYPE, "%s: out_dtype %d is neither BG_F32 nor the operand dtype %d", who,
               out_dtype, dtype);
    return 0;
}

template <typename Launch>
static int lb_wgrad_entry(const char* who, const char* op, const char* red, const char* stride, const void* dy, int ld_dy, const void* b, int ld_op,
                          int min_ld_op, void* dw, void* db, int M, int N, int K, int dtype, int out_dtype, int split, bool empty_ok,
                          void* workspace, size_t workspace_bytes, bg_stream_t stream, Launch&& launch) {
    BG_REQUIRE(split >= 0 && split <= LB_MAX_SPLIT, BG_E_ARG, "%s: split = %d outside [0, %d] (0 = auto)", who, split, LB_MAX_SPLIT);
    BG_REQUIRE(dw != nullptr, BG_E_ARG, "%s: null pointer (dw)", who);
    BG_REQUIRE(M == 0 || (dy != nullptr && b != nullptr), BG_E_ARG, "%s: null pointer (dy, %s)", who, op);
    BG_REQUIRE(ld_dy >= N && ld_op >= min_ld_op && ld_dy % 8 == 0 && ld_op % 8 == 0, BG_E_ALIGN,
               "%s: %s strides ld_dy = %d (>= N), ld_%s = %d (>= %s) must be multiples of 8 elements", who, stride, ld_dy, op, ld_op, red);
    BG_REQUIRE(aligned(dy, 16) && aligned(b, 16) && aligned(dw, 16) && aligned(db, 16) && aligned(workspace, 16), BG_E_ALIGN,
               "%s: 16-byte alignment of dy / %s / dw / db / workspace", who, op);
    hipStream_t s = (hipStream_t)stream;
    const bool out16 = out_dtype != BG_F32;
    if (M == 0) {
        const size_t esz = out16 ? 2 : 4;
        hipError_t e = hipMemsetAsync(dw, 0, (size_t)N * K * esz, s);
        if (e == hipSuccess && db) e = hipMemsetAsync(db, 0, (size_t)N * esz, s);
        BG_REQUIRE(e == hipSuccess, (int)e, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
        return 0;
    }
    const int S = split == 0 ? lb_auto_split(M, N, K) : split;
    BG_REQUIRE(empty_ok || lb_no_empty_slice(M, S), BG_E_ARG, "%s: split = %d leaves an empty slice for M = %d (slices are whole steps of %d rows)",
               who, S, M, LB_RS);
    const size_t need = lb_workspace(N, K, S);
    BG_REQUIRE(need == 0 || (workspace != nullptr && workspace_bytes >= need), BG_E_ARG, "%s: workspace of %zu bytes, %zu needed for split = %d", who,
               workspace ? workspace_bytes : (size_t)0, need, S);
    const dim3 grid((unsigned)((K / 128) * (N / 128) * S));      // one workgroup per (K tile, N tile, slice)
    const int slice_rows = lb_slice_rows(M, S);
    float* ws = (float*)workspace;
    auto tile = [&](auto F) {
        if (S > 1) launch(F, std::integral_constant<int, 0>{}, grid, (void*)ws, (void*)(ws + (size_t)S * N * K), slice_rows);
        else if (out16) launch(F, std::integral_constant<int, 2>{}, grid, dw, db, slice_rows);
        else launch(F, std::integral_constant<int, 1>{}, grid, dw, db, slice_rows);
    };
    if (dtype == BG_F16) tile(std::true_type{});
    else tile(std::false_type{});
    if (S > 1) lb_reduce(s, dtype == BG_F16, out16, ws, dw, db, S, N, K);
    return launch_status(who + 3);          // the entry's name without "bg_"
}

}  // namespace bg
