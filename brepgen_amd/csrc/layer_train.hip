// The glue of an encoder layer in TRAINING (nn.TransformerEncoderLayer(768, 12, 1024, dropout, norm_first=True), network.py:1076-1078):
// LayerNorm forward that keeps (mean, rstd), LayerNorm backward with the residual merge and the gamma / beta gradients, and the
// elementwise dropout ops (dropout + residual add, ReLU + dropout) with their backward.  Row-wise, memory-bound passes over
// [tokens, 768] / [tokens, 1024]; include/brepgen_hip.h states every entry.  Nothing is allocated, no atomics: one writer per output
// element and a fixed summation order.
//
// The LayerNorm row kernels, their layout and the 8-element load / store are ln_rows.h's (shared with mlp_train.hip, which instantiates
// them with the SiLU of the denoisers' MLPs); this file instantiates the plain LayerNorm and holds the fp64 merge of the column sums.
#include "ln_rows.h"
#include "philox.h"

namespace bg {

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
void lt_ln_reduce(const double* ws, int G, float* dgamma, float* dbeta, hipStream_t s) {
    hipLaunchKernelGGL(lt_ln_reduce_kernel, dim3(2 * LT_C / LT_RED_COLS), dim3(256), 0, s, ws, G, dgamma, dbeta);
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
    return lt_ln_fwd_entry<false>("bg_ln_train_fwd", x, x_dtype, gamma, beta, y, y_dtype, stats, M, eps, stream);
}

extern "C" size_t bg_ln_bwd_workspace_bytes(int M) { return lt_bwd_workspace_bytes(M); }

extern "C" int bg_ln_bwd(const void* dy, int y_dtype, const void* x, int x_dtype, const float* stats, const float* gamma, const void* dskip,
                         void* dx, float* dgamma, float* dbeta, int M, void* workspace, size_t workspace_bytes, bg_stream_t stream) {
    return lt_ln_bwd_entry<false>("bg_ln_bwd", dy, y_dtype, x, x_dtype, stats, gamma, nullptr, dskip, dx, dgamma, dbeta, M, workspace,
                                  workspace_bytes, stream);
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
