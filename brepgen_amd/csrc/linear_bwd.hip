// The Linear layers' backward: the weight gradient with the bias gradient folded in (bg_linear_wgrad), and the one-launch weight
// cast / transpose that feeds the forward and the data-gradient GEMMs (bg_weight_cast).  y = x W^T + b and dX = dY W both run on
// bg_gemm_ex_fwd as it stands (dX: a = dY, w = the transposed 16-bit copy bg_weight_cast writes); what the library lacked is
//       dW[n, k] = sum_m dY[m, n] X[m, k],      db[n] = sum_m dY[m, n],
// a product that reduces over the ROW index of both operands (M = tokens, 15 360 - 96 000 at the trainers' shapes) into a small
// output (36 - 108 tiles of 128 x 128).
//
// Organisation (lb_wgrad_kernel).  A workgroup of four waves owns one 128 x 128 tile of dW and one contiguous slice of the M rows
// (one workgroup per K tile x N tile x slice, handed to the XCDs in contiguous runs: see the kernel), and walks the slice in steps of LB_RS = 32 rows.  Per step the 32 x 128 pieces of dY and of X
// go through registers into two ROW-MAJOR LDS images (256-byte rows, 16-byte chunks XOR-swizzled: lb_off); rows at and beyond the
// slice's end are zero-filled in registers and never read from memory.  The reduction index of the 32x32x16 MFMA is the image ROW for
// both operands, so both fragments come from ds_read_b64_tr_b16, the hardware transpose read (a lane supplies the address of four
// consecutive columns of one row and receives four consecutive ROWS of one column); no transposed copy of either operand exists
// anywhere.  Wave (wn, wk) accumulates the 64 x 64 quarter of the tile in four accumulators; accumulator register r of (ni, ki) is
//       dW[n0 + 64 wn + 32 ni + (r & 3) + 8 (r >> 2) + 4 h][k0 + 64 wk + 32 ki + (lane & 31)],      h = lane >> 5.
// The next step's rows are fetched into registers before the current step's products and written to the other image pair after
// them: one barrier per step.
//
// Bias gradient.  The workgroups of the first K-tile column add up the dY values they stage anyway: a staging
// thread owns 8 columns and every 16th row, sums them in fp32 in row order, and the sixteen row groups are added in index order at the
// end.  No extra pass over dY, no extra MFMA.
//
// Determinism.  No atomics, one writer per output element, fixed summation order.  With S > 1 slices each writes its fp32 partial
// tile to the workspace ([S][N][K], then [S][N] for db) and lb_reduce_kernel adds the S partials in index order and writes dW / db in
// the output dtype; with S = 1 the tile kernel writes dW / db itself.
#include "wgrad_tile.h"
#include <stdlib.h>

namespace bg {

// OUT: 0 = fp32 partial tile to the workspace (split > 1), 1 = dW / db in fp32, 2 = dW / db in the operand dtype
template <bool F16, int OUT>
__global__ __launch_bounds__(256, 2) void lb_wgrad_kernel(const void* __restrict__ dy_, int ld_dy, const void* __restrict__ x_, int ld_x,
                                                          void* __restrict__ dw_, void* __restrict__ db_, int M, int N, int K,
                                                          int slice_rows, int plain_walk) {
    using E = Elem<F16>;
    using T = typename E::T;
    using V8 = typename E::V8;
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * LB_IMG];      // [stage][dY image | X image]
    const T* __restrict__ dy = reinterpret_cast<const T*>(dy_);
    const T* __restrict__ x = reinterpret_cast<const T*>(x_);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 1, wk = wave & 1;
    // XCD-aware walk (block b runs on XCD b % 8, each with a private L2): logical ids go K tile fastest, then N tile, then slice, and
    // an XCD gets a contiguous run of them -- the K / 128 workgroups that share a dY piece and the N tiles that share a slice of X
    // meet in one L2 instead of eight (environment BG_LINEAR_WGRAD_WALK=plain: the plain order, for the in-process A/B)
    const int lid = plain_walk ? (int)blockIdx.x : xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int kt_n = K >> 7, nt_n = N >> 7;
    const int kt = lid % kt_n, nt = (lid / kt_n) % nt_n, slice = lid / (kt_n * nt_n);
    const int k0 = kt * 128, n0 = nt * 128;
    const int m_begin = slice * slice_rows;
    const int m_end = min(M, m_begin + slice_rows);
    const int nsteps = m_end > m_begin ? (m_end - m_begin + LB_RS - 1) / LB_RS : 0;
    const bool with_db = db_ != nullptr && kt == 0;

    // ---- staging: thread = (16-byte chunk sc, rows sr and sr + 16) of both 32 x 128 pieces ----
    const int sc = tid & 15, sr = tid >> 4;
    const T* dyp = dy + n0 + sc * 8;
    const T* xp = x + k0 + sc * 8;
    const unsigned st_off = lb_off(sr, sc);            // row sr + 16 has the same swizzle term: + 16 * 256 bytes
    uint4 rdy[2], rx[2];
    float dbacc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) dbacc[e] = 0.f;
    auto fetch = [&](int it) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m_begin + it * LB_RS + sr + 16 * j;
            rdy[j] = make_uint4(0u, 0u, 0u, 0u);
            rx[j] = make_uint4(0u, 0u, 0u, 0u);
            if (m < m_end) {
                rdy[j] = *reinterpret_cast<const uint4*>(dyp + (size_t)m * ld_dy);
                rx[j] = *reinterpret_cast<const uint4*>(xp + (size_t)m * ld_x);
            }
        }
    };
    auto stash = [&](int st) {
        unsigned char* img = lds + st * 2 * LB_IMG + st_off;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<uint4*>(img + j * 16 * 256) = rdy[j];
            *reinterpret_cast<uint4*>(img + LB_IMG + j * 16 * 256) = rx[j];
        }
        if (with_db) {
            lb_add8<F16>(dbacc, rdy[0]);
            lb_add8<F16>(dbacc, rdy[1]);
        }
    };

    // ---- fragment addresses.  16-lane group gg = lane >> 4 reads the block of rows 8 h + {0..3} (second read: + 4) and columns
    // 16 (gg & 1) .. + 15 of a 32-column MFMA tile; lane 4 q + p of the group supplies row q, columns 4 p .. 4 p + 3 and receives
    // the four rows of column (lane & 15): column (lane & 31) of the tile, reduction slots 8 h .. 8 h + 7 = the MFMA's operand map ----
    const int gi = lane & 15, gg = lane >> 4, h = gg >> 1;
    const int fq = gi >> 2, fp = gi & 3;
    unsigned a_off[2][2], b_off[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int row = 8 * h + 4 * s + fq;
            a_off[t][s] = lb_off(row, 8 * wn + 4 * t + 2 * (gg & 1) + (fp >> 1)) + 8u * (fp & 1);
            b_off[t][s] = lb_off(row, 8 * wk + 4 * t + 2 * (gg & 1) + (fp >> 1)) + 8u * (fp & 1) + LB_IMG;
        }

    f32x16 acc[2][2];
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int ki = 0; ki < 2; ++ki)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ni][ki][r] = 0.f;

    if (nsteps > 0) {
        fetch(0);
        stash(0);
    }
    for (int it = 0; it < nsteps; ++it) {
        const int st = it & 1;
        const bool more = it + 1 < nsteps;
        if (more) fetch(it + 1);
        __syncthreads();                                  // stage st is written; everybody is done reading stage st ^ 1
        const unsigned char* img = lds + st * 2 * LB_IMG;
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
        if (more) stash(st ^ 1);
    }

    // ---- the tile ----
    const int l31 = lane & 31;
    const size_t out_base = OUT == 0 ? (size_t)slice * N * K : 0;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int ki = 0; ki < 2; ++ki)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + 64 * wn + 32 * ni + (r & 3) + 8 * (r >> 2) + 4 * h;
                const size_t at = out_base + (size_t)n * K + (k0 + 64 * wk + 32 * ki + l31);
                if (OUT == 2) reinterpret_cast<T*>(dw_)[at] = cvt16<T>(acc[ni][ki][r]);
                else reinterpret_cast<float*>(dw_)[at] = acc[ni][ki][r];
            }

    // ---- bias gradient: the sixteen row groups in index order ----
    if (with_db) {
        __syncthreads();                                  // the images are dead
        float* red = reinterpret_cast<float*>(lds);       // [16 row groups][128 columns]
#pragma unroll
        for (int e = 0; e < 8; ++e) red[sr * 128 + sc * 8 + e] = dbacc[e];
        __syncthreads();
        if (tid < 128) {
            float v = red[tid];
#pragma unroll
            for (int g = 1; g < 16; ++g) v += red[g * 128 + tid];
            const size_t at = (OUT == 0 ? (size_t)slice * N : 0) + n0 + tid;
            if (OUT == 2) reinterpret_cast<T*>(db_)[at] = cvt16<T>(v);
            else reinterpret_cast<float*>(db_)[at] = v;
        }
    }
}

// dW / db = the S partials added in index order.  One thread per four consecutive elements: items [0, nk / 4) are dW, the next
// N / 4 are db (partials at part + S * nk).
template <bool F16, bool OUT16>
__global__ __launch_bounds__(256) void lb_reduce_kernel(const float* __restrict__ part, void* __restrict__ dw_, void* __restrict__ db_,
                                                        int S, size_t nk, int N) {
    using T = typename Elem<F16>::T;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t nk4 = nk >> 2;
    const float* src;
    size_t stride, at;
    void* out;
    if (idx < nk4) {
        src = part + 4 * idx; stride = nk; at = 4 * idx; out = dw_;
    } else {
        const size_t j = idx - nk4;
        if (j >= (size_t)(N >> 2) || db_ == nullptr) return;
        src = part + (size_t)S * nk + 4 * j; stride = (size_t)N; at = 4 * j; out = db_;
    }
    float4 v = *reinterpret_cast<const float4*>(src);
    for (int s = 1; s < S; ++s) {
        const float4 p = *reinterpret_cast<const float4*>(src + (size_t)s * stride);
        v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    if (OUT16) *reinterpret_cast<typename Elem<F16>::V4*>(reinterpret_cast<T*>(out) + at) = Elem<F16>::pack4(v.x, v.y, v.z, v.w);
    else *reinterpret_cast<float4*>(reinterpret_cast<float*>(out) + at) = v;
}

// ---- bg_weight_cast: a 64 x 64 tile per workgroup through LDS; 16-byte global accesses on both sides ----
// MODE: 0 = 16-bit source (bits copied), 1 = fp32 -> bf16, 2 = fp32 -> fp16
template <int MODE>
__global__ __launch_bounds__(256) void lb_cast_kernel(const void* __restrict__ src_, void* __restrict__ dst_, void* __restrict__ dst_t_,
                                                      int R, int C) {
    constexpr int LD = 72;                                // tile row stride (16-bit elements): rows stay 16-byte aligned
    __shared__ __attribute__((aligned(16))) unsigned short tile[64 * LD];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    if (MODE == 0) {
        const unsigned short* src = reinterpret_cast<const unsigned short*>(src_);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int idx = j * 256 + tid, row = idx >> 3, c8 = idx & 7;
            *reinterpret_cast<uint4*>(tile + row * LD + 8 * c8) = *reinterpret_cast<const uint4*>(src + (size_t)(r0 + row) * C + c0 + 8 * c8);
        }
    } else {
        const float* src = reinterpret_cast<const float*>(src_);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = j * 256 + tid, row = idx >> 4, c4 = idx & 15;
            const float4 v = *reinterpret_cast<const float4*>(src + (size_t)(r0 + row) * C + c0 + 4 * c4);
            *reinterpret_cast<uint2*>(tile + row * LD + 4 * c4) = pack4_16(v.x, v.y, v.z, v.w, MODE == 2 ? BG_F16 : BG_BF16);
        }
    }
    __syncthreads();
    if (dst_) {
        unsigned short* dst = reinterpret_cast<unsigned short*>(dst_);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int idx = j * 256 + tid, row = idx >> 3, c8 = idx & 7;
            *reinterpret_cast<uint4*>(dst + (size_t)(r0 + row) * C + c0 + 8 * c8) = *reinterpret_cast<const uint4*>(tile + row * LD + 8 * c8);
        }
    }
    if (dst_t_) {
        unsigned short* dst_t = reinterpret_cast<unsigned short*>(dst_t_);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int idx = j * 256 + tid, col = idx >> 3, r8 = idx & 7;      // output row = source column
            unsigned short e[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) e[i] = tile[(8 * r8 + i) * LD + col];
            uint4 v;
            v.x = e[0] | ((unsigned)e[1] << 16); v.y = e[2] | ((unsigned)e[3] << 16);
            v.z = e[4] | ((unsigned)e[5] << 16); v.w = e[6] | ((unsigned)e[7] << 16);
            *reinterpret_cast<uint4*>(dst_t + (size_t)(c0 + col) * R + r0 + 8 * r8) = v;
        }
    }
}

// ---- host-side plan: wgrad_tile.h ----
static inline bool lb_shape_ok(int M, int N, int K) { return M >= 0 && N >= 128 && K >= 128 && N % 128 == 0 && K % 128 == 0; }

void lb_reduce(hipStream_t s, bool f16, bool out16, const float* ws, void* dw, void* db, int S, int N, int K) {
    const size_t nk = (size_t)N * K;
    const unsigned blocks = (unsigned)((nk / 4 + N / 4 + 255) / 256);
    with_bools(f16, out16, [&](auto F, auto O) {
        hipLaunchKernelGGL((lb_reduce_kernel<decltype(F)::value, decltype(O)::value>), dim3(blocks), dim3(256), 0, s, ws, dw, db, S, nk, N);
    });
}

}  // namespace bg

using namespace bg;

extern "C" int bg_linear_wgrad_split(int M, int N, int K) {
    if (!lb_shape_ok(M, N, K) || M == 0) return 1;
    return lb_auto_split(M, N, K);
}

extern "C" size_t bg_linear_wgrad_workspace_bytes(int M, int N, int K, int split) {
    if (!lb_shape_ok(M, N, K) || M == 0 || split < 0 || split > LB_MAX_SPLIT) return 0;
    return lb_workspace(N, K, split == 0 ? lb_auto_split(M, N, K) : split);
}

extern "C" int bg_linear_wgrad(const void* dy, int ld_dy, const void* x, int ld_x, void* dw, void* db, int M, int N, int K, int dtype,
                               int out_dtype, int split, void* workspace, size_t workspace_bytes, bg_stream_t stream) {
    if (int e = lb_wgrad_dtypes("bg_linear_wgrad", dtype, out_dtype)) return e;
    BG_REQUIRE(M >= 0, BG_E_SHAPE, "bg_linear_wgrad: M = %d is negative", M);
    BG_REQUIRE(N >= 128 && K >= 128 && N % 128 == 0 && K % 128 == 0 && N / 128 <= 65535, BG_E_SHAPE,
               "bg_linear_wgrad: N = %d and K = %d must be multiples of 128", N, K);
    const char* walk = getenv("BG_LINEAR_WGRAD_WALK");      // "plain": block order as launched, for the in-process A/B and its bit test
    const int plain = walk != nullptr && walk[0] == 'p';
    return lb_wgrad_entry("bg_linear_wgrad", "x", "K", "row", dy, ld_dy, x, ld_x, K, dw, db, M, N, K, dtype, out_dtype, split, false, workspace,
                          workspace_bytes, stream, [&](auto F, auto OUT, dim3 grid, void* dw_, void* db_, int slice_rows) {
                              hipLaunchKernelGGL((lb_wgrad_kernel<decltype(F)::value, decltype(OUT)::value>), grid, dim3(256), 0,
                                                 (hipStream_t)stream, dy, ld_dy, x, ld_x, dw_, db_, M, N, K, slice_rows, plain);
                          });
}

extern "C" int bg_weight_cast(const void* src, int src_dtype, int R, int C, void* dst, void* dst_t, int dtype, bg_stream_t stream) {
    BG_REQUIRE(dtype == BG_BF16 || dtype == BG_F16, BG_E_DTYPE, "bg_weight_cast: target dtype %d (BG_BF16 or BG_F16)", dtype);
    BG_REQUIRE(src_dtype == BG_F32 || src_dtype == dtype, BG_E_DTYPE, "bg_weight_cast: source dtype %d is neither BG_F32 nor the target dtype %d",
               src_dtype, dtype);
    BG_REQUIRE(R >= 64 && C >= 64 && R % 64 == 0 && C % 64 == 0 && R / 64 <= 65535, BG_E_SHAPE,
               "bg_weight_cast: R = %d and C = %d must be multiples of 64", R, C);
    BG_REQUIRE(src != nullptr, BG_E_ARG, "bg_weight_cast: null pointer (src)");
    BG_REQUIRE(dst != nullptr || dst_t != nullptr, BG_E_ARG, "bg_weight_cast: null pointer (dst and dst_t: at least one output)");
    BG_REQUIRE(aligned(src, 16) && aligned(dst, 16) && aligned(dst_t, 16), BG_E_ALIGN, "bg_weight_cast: 16-byte alignment of src / dst / dst_t");
    const dim3 grid(C / 64, R / 64);
    hipStream_t s = (hipStream_t)stream;
    if (src_dtype != BG_F32) hipLaunchKernelGGL(lb_cast_kernel<0>, grid, dim3(256), 0, s, src, dst, dst_t, R, C);
    else if (dtype == BG_BF16) hipLaunchKernelGGL(lb_cast_kernel<1>, grid, dim3(256), 0, s, src, dst, dst_t, R, C);
    else hipLaunchKernelGGL(lb_cast_kernel<2>, grid, dim3(256), 0, s, src, dst, dst_t, R, C);
    return launch_status("weight_cast");
}
