// Exact-fp32 GEMM on the f32-input matrix core (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, bitwise the
// same numerics as a VALU fp32 GEMM, at the 157 TFLOP/s vector rate).  Used for
//   * every nn.Linear of the fp32 parity mode (BASELINE configs[0], tolerance 1e-5), and
//   * the tiny-K first Linear of each embed MLP (K = 6 / 12 / 48, network.py:1080-1085) in every mode, so the
//     raw fp32 inputs (x_t, bboxes, latents) are never rounded to bf16.
// Any M, N, K; nn.Linear layout w[N,K]; tile 64x64x16, 4 waves (2x2), each wave one 32x32 accumulator.
#include "bg_common.h"

namespace bg {

constexpr int F_BM = 64, F_BN = 64, F_BK = 16, F_LD = F_BK + 1;   // +1 float pad: conflict-free ds_read_b32

__global__ __launch_bounds__(256) void gemm_f32_kernel(GemmArgs g) {
    __shared__ float As[F_BM * F_LD];
    __shared__ float Bs[F_BN * F_LD];
    const float* __restrict__ A = reinterpret_cast<const float*>(g.a);
    const float* __restrict__ W = reinterpret_cast<const float*>(g.w);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int nt_n = (g.N + F_BN - 1) / F_BN;
    const int m0 = (blockIdx.x / nt_n) * F_BM, n0 = (blockIdx.x % nt_n) * F_BN;
    const int Mv = g.m_dev ? *g.m_dev : g.M;                      // rows present (compacted batch: device-side count)
    if (m0 >= Mv) return;

    // global -> LDS assignment: thread t loads 4 consecutive k of one row of A and one row of W
    const int lrow = tid >> 2, lk = (tid & 3) * 4;
    const int arow = m0 + lrow, wrow = n0 + lrow;
    const bool a_ok = arow < Mv, w_ok = wrow < g.N_pad;
    const float* ap = A + (size_t)(a_ok ? arow : 0) * g.lda;
    const float* wp = W + (size_t)(w_ok ? wrow : 0) * g.K;

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    for (int k0 = 0; k0 < g.K; k0 += F_BK) {
        float av[4], wv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + lk + j;
            av[j] = (a_ok && k < g.K) ? ap[k] : 0.f;
            wv[j] = (w_ok && k < g.K) ? wp[k] : 0.f;
        }
        __syncthreads();   // previous tile fully consumed
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[lrow * F_LD + lk + j] = av[j];
            Bs[lrow * F_LD + lk + j] = wv[j];
        }
        __syncthreads();
        // lane l supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31] of each k=2 slice
        const float* as = &As[(wm * 32 + (lane & 31)) * F_LD + (lane >> 5)];
        const float* bs = &Bs[(wn * 32 + (lane & 31)) * F_LD + (lane >> 5)];
#pragma unroll
        for (int kk = 0; kk < F_BK / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[kk * 2], bs[kk * 2], acc, 0, 0, 0);
    }

    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const int col = n0 + wn * 32 + (lane & 31);
    if (col >= g.N) return;
    const float bias = g.bias ? g.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= Mv) continue;
        const int prow = g.row_map ? g.row_map[row] : row;        // this row's index in the padded token layout
        const int orow = g.map_out ? prow : row;
        float v = acc[r] + bias;
        if (g.act == BG_ACT_RELU) v = fmaxf(v, 0.f);
        if (g.add) v += g.add[(size_t)((g.map_add ? prow : row) / g.add_div) * g.ld_add + col];
        if (g.add2) v += g.add2[(size_t)((g.map_add2 ? prow : row) / g.add2_div) * g.ld_add2 + col];
        if (g.out_dtype == BG_BF16) reinterpret_cast<__bf16*>(g.out)[(size_t)orow * g.ldc + col] = (__bf16)v;
        else if (g.out_dtype == BG_F16) reinterpret_cast<_Float16*>(g.out)[(size_t)orow * g.ldc + col] = (_Float16)v;
        else reinterpret_cast<float*>(g.out)[(size_t)orow * g.ldc + col] = v;
    }
}

// M == 1 (the time-embedding MLP of a sampling step: ONE timestep shared by the batch): a 64x64-tile GEMM would run 12 blocks
// through a 48-step latency chain.  Here one wave owns one output column: lanes stride over K (coalesced 256-byte
// reads of the weight row), fma-accumulate, butterfly-reduce.
__global__ __launch_bounds__(256) void gemv_f32_kernel(GemmArgs g) {
    const float* __restrict__ A = reinterpret_cast<const float*>(g.a);
    const float* __restrict__ W = reinterpret_cast<const float*>(g.w);
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= g.N) return;
    const float* wr = W + (size_t)n * g.K;
    const float bias = g.bias ? g.bias[n] : 0.f;
    for (int m = 0; m < g.M; ++m) {
        const float* ar = A + (size_t)m * g.lda;
        float s = 0.f;
        for (int k = lane; k < g.K; k += 64) s = __builtin_fmaf(ar[k], wr[k], s);
        s = wave_sum(s);
        if (lane == 0) {
            float v = s + bias;
            if (g.act == BG_ACT_RELU) v = fmaxf(v, 0.f);
            if (g.add) v += g.add[(size_t)(m / g.add_div) * g.ld_add + n];
            if (g.add2) v += g.add2[(size_t)(m / g.add2_div) * g.ld_add2 + n];
            if (g.out_dtype == BG_BF16) reinterpret_cast<__bf16*>(g.out)[(size_t)m * g.ldc + n] = (__bf16)v;
            else if (g.out_dtype == BG_F16) reinterpret_cast<_Float16*>(g.out)[(size_t)m * g.ldc + n] = (_Float16)v;
            else reinterpret_cast<float*>(g.out)[(size_t)m * g.ldc + n] = v;
        }
    }
}

int gemm_f32(const GemmArgs& g, hipStream_t s) {
    if (g.M <= 0 || g.N <= 0) return 0;
    if (g.out_lo || g.res_hi || g.stats_out || g.stats_in) {
        set_error("gemm_f32: split residual / LayerNorm fold exist for 16-bit operands only");
        return BG_E_DTYPE;
    }
    // Dispatch rule: the GEMV rounds differently from the MFMA's k-ordered chain, so it may only be chosen by something
    // that does not depend on the batch composition.  M == 1 <=> one shared timestep (n_timesteps == 1) for ANY batch size;
    // per-sample timesteps (M == B) always take the MFMA kernel, so a sample gives the same bits in every batch.
    if (g.gemv_ok && g.M == 1 && g.K >= 64) {
        ProfScope prof(PK_GEMM_F32, 2.0 * g.M * g.N * (double)g.K, 4.0 * g.N * (double)g.K, s);
        hipLaunchKernelGGL(gemv_f32_kernel, dim3((g.N + 3) / 4), dim3(256), 0, s, g);
        return launch_status("gemv_f32");
    }
    const int nblk = ((g.M + F_BM - 1) / F_BM) * ((g.N + F_BN - 1) / F_BN);
    const double osz = g.out_dtype == BG_F32 ? 4.0 : 2.0;
    const double rows = g.rows_hint > 0 ? g.rows_hint : g.M;
    ProfScope prof(PK_GEMM_F32, 2.0 * rows * g.N * (double)g.K,
                   4.0 * rows * g.K + 4.0 * g.N * (double)g.K + osz * rows * g.N + (g.add ? 4.0 * (rows / g.add_div) * g.N : 0.0), s);
    hipLaunchKernelGGL(gemm_f32_kernel, dim3(nblk), dim3(256), 0, s, g);
    return launch_status("gemm_f32");
}

int gemm(const GemmArgs& g, int ab_dtype, hipStream_t s) {
    if (ab_dtype == BG_F32) return gemm_f32(g, s);
    if (ab_dtype == BG_BF16 || ab_dtype == BG_F16) return gemm_16bit(g, ab_dtype, s);
    set_error("gemm: unsupported operand dtype %d", ab_dtype);
    return BG_E_DTYPE;
}

}  // namespace bg

extern "C" int bg_gemm_ex_fwd(const bg_gemm_desc* d, bg_stream_t stream) {
    BG_REQUIRE(d && d->a && d->w && d->out, BG_E_ARG, "bg_gemm_ex_fwd: null pointer");
    BG_REQUIRE(d->M >= 0 && d->N > 0 && d->K > 0 && d->N_pad >= d->N && d->lda >= d->K && d->ldc >= d->N, BG_E_SHAPE,
               "bg_gemm_ex_fwd: bad shape M=%d N=%d N_pad=%d K=%d lda=%d ldc=%d", d->M, d->N, d->N_pad, d->K, d->lda, d->ldc);
    BG_REQUIRE(d->out_dtype == BG_F32 || d->out_dtype == BG_BF16 || d->out_dtype == BG_F16, BG_E_DTYPE, "bg_gemm_ex_fwd: out dtype %d", d->out_dtype);
    BG_REQUIRE((d->add == nullptr || d->add_div >= 1) && (d->add2 == nullptr || d->add2_div >= 1), BG_E_ARG,
               "bg_gemm_ex_fwd: addend divisors must be >= 1");
    bg::GemmArgs g = bg::linear(d->a, d->lda, d->w, d->bias, d->out, d->ldc, d->M, d->N, d->N_pad, d->K, d->out_dtype, d->act);
    bg::add_rows(g, d->add, d->ld_add, d->add_div);
    bg::add2_rows(g, d->add2, d->ld_add2, d->add2_div);
    bg::split_out(g, d->out_lo, d->stats_out);
    bg::split_residual_in(g, d->res_hi, d->res_lo, d->ld_res);
    bg::ln_fold_in(g, d->stats_in, d->colsum);
    g.ln_eps = d->ln_eps;
    return bg::gemm(g, d->ab_dtype, (hipStream_t)stream);
}

static inline int ilog2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}

extern "C" int bg_conv_gemm_fwd(const bg_conv_desc* d, bg_stream_t stream) {
    BG_REQUIRE(d && d->x && d->w && d->out && d->zero_page, BG_E_ARG, "bg_conv_gemm_fwd: null pointer");
    BG_REQUIRE(d->dtype == BG_BF16 || d->dtype == BG_F16, BG_E_DTYPE, "bg_conv_gemm_fwd: 16-bit operands only");
    BG_REQUIRE(d->S > 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->N > 0, BG_E_SHAPE, "bg_conv_gemm_fwd: empty shape");
    const int Ho = d->H << d->up, Wo = d->W << d->up;
    const int lw = ilog2_exact(Wo), lh = ilog2_exact(Ho), ls = (d->C % 64 == 0) ? ilog2_exact(d->C / 64) : -1;
    const bool narrow = d->N < 128;                                // w / bias zero-padded to 128 rows by the caller, no residual
    BG_REQUIRE(lw >= 0 && lh >= 0 && ls >= 0 && (d->kh & 1) && (d->kw & 1) && d->up >= 0 && d->up <= 1 &&
                   (d->N % 128 == 0 || (narrow && d->add == nullptr && d->bias != nullptr)), BG_E_SHAPE,
               "bg_conv_gemm_fwd: needs power-of-two output grid, C / 64 a power of two, odd window, N %% 128 == 0 -- or N < 128 with "
               "w and bias padded to 128 rows and no residual (H=%d W=%d up=%d C=%d k=%dx%d N=%d)", d->H, d->W, d->up, d->C, d->kh, d->kw, d->N);
    BG_REQUIRE(((uintptr_t)d->x & 15) == 0 && ((uintptr_t)d->zero_page & 127) == 0, BG_E_ALIGN, "bg_conv_gemm_fwd: alignment");
    const long long rows = (long long)d->S * Ho * Wo;
    BG_REQUIRE(rows < (1ll << 31), BG_E_SHAPE, "bg_conv_gemm_fwd: too many output pixels for one call (%lld)", rows);
    bg::GemmArgs g = bg::linear(d->x, d->C, d->w, d->bias, d->out, d->ldc, (int)rows, d->N, narrow ? 128 : d->N, d->kh * d->kw * d->C, BG_F32);
    bg::add_rows(g, d->add, d->ld_add, 1);
    g.cv_C = d->C; g.cv_H = d->H; g.cv_W = d->W; g.cv_kh = d->kh; g.cv_kw = d->kw; g.cv_up = d->up;
    g.cv_wo_log2 = lw; g.cv_ho_log2 = lh; g.cv_spt_log2 = ls; g.cv_zero = d->zero_page;
    return bg::gemm(g, d->dtype, (hipStream_t)stream);
}

extern "C" int bg_gemm_bias_act_fwd(const void* a, int lda, const void* w, const float* bias, void* out, int ldc,
                                    int M, int N, int N_pad, int K, int ab_dtype, int out_dtype, int act,
                                    const float* add, int ld_add, int add_div, bg_stream_t stream) {
    BG_REQUIRE(a && w && out, BG_E_ARG, "bg_gemm_bias_act_fwd: null pointer");
    BG_REQUIRE(M >= 0 && N > 0 && K > 0 && N_pad >= N && lda >= K && ldc >= N, BG_E_SHAPE,
               "bg_gemm_bias_act_fwd: bad shape M=%d N=%d N_pad=%d K=%d lda=%d ldc=%d", M, N, N_pad, K, lda, ldc);
    BG_REQUIRE(out_dtype == BG_F32 || out_dtype == BG_BF16 || out_dtype == BG_F16, BG_E_DTYPE, "bg_gemm_bias_act_fwd: out dtype %d", out_dtype);
    BG_REQUIRE(add == nullptr || add_div >= 1, BG_E_ARG, "bg_gemm_bias_act_fwd: add_div must be >= 1");
    bg::GemmArgs g = bg::linear(a, lda, w, bias, out, ldc, M, N, N_pad, K, out_dtype, act);
    bg::add_rows(g, add, ld_add, add_div);
    return bg::gemm(g, ab_dtype, (hipStream_t)stream);
}
