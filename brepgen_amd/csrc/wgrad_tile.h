// What the two weight-gradient kernels share (linear_bwd.hip: lb_wgrad_kernel, conv_train.hip: cw_wgrad_kernel): the row-major
// LDS image of a 32 x 128 operand piece and its transpose-read fragments, the staged-dY bias sum, and the host-side slice plan.
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

}  // namespace bg
