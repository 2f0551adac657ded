// The update half of a trainer iteration (trainer.py: clip_grad_norm_ + GradScaler.step / update + torch.optim.AdamW) as three launches
// with no host synchronisation; brepgen_amd/optim.py is the caller, tests/optim_restate.py the arithmetic in numpy.
//
//   bg_mt_grad_stats    per workgroup: fp64 sum of g^2 (every product of two fp32 values is exact in fp64), the largest finite |g| and
//                       a non-finite flag over the chunks it owns -> ONE partial.  No atomics; which thread adds which element in which
//                       order is a function of the chunk list alone, so the norm is the same bits on every run and every device.
//   bg_mt_adamw_step    every workgroup reduces the partials the same way (same norm, same found_inf everywhere), then either returns
//                       (found_inf: no byte of any p, m, v changes) or updates its chunks: clip, unscale, decoupled decay, Adam.
//   bg_optim_finish     one wave: the same reduction once more, then GradScaler.update's state machine, step += 1 and the fp64 beta
//                       powers.  A launch of its own, so that no workgroup of the step reads state another one rewrites.
//   bg_mt_scale_grads   g = g * c in place, for the stand-alone clip_grad_norm_.
//
// All tensors are fp32 and contiguous.  A chunk is OPT_CHUNK consecutive elements of one tensor; thread t owns the four elements
// 4 (t + 256 j) .. + 3 of it for j = 0 .. 3 -- as one 16-byte access where the chunk's pointers are 16-byte aligned, as four 4-byte
// accesses where they are not (the element -> thread map, and with it the summation order, is the same either way).
// Plain C++ and vector stores only; the build keeps -ffp-contract=off, so every line below rounds once per operation.
#include "bg_common.h"

namespace bg {

constexpr int OPT_THREADS = 256;
constexpr int OPT_CHUNK = BG_OPTIM_CHUNK;               // 4096 = 256 threads x 4 x 16 bytes
constexpr int OPT_MAX_BLOCKS = BG_OPTIM_MAX_BLOCKS;     // 2048: the memory-bound grid cap (256 CUs x 8 workgroups)
static_assert(OPT_CHUNK == OPT_THREADS * 16, "a chunk is four 16-byte accesses per thread");

struct OptPartial { double sumsq; uint32_t maxabs_bits; uint32_t nonfinite; };      // 16 bytes, one per workgroup of bg_mt_grad_stats
static_assert(sizeof(OptPartial) == 16, "partials are read as one 16-byte load");
static_assert(sizeof(bg_mt_row) == 56 && sizeof(bg_mt_chunk) == 16 && sizeof(bg_optim_state) == 32 && sizeof(bg_scaler_state) == 8, "ABI");

__device__ __forceinline__ double wave_sum_f64(double v) {      // butterfly, fixed association; every lane ends with the total
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}
__device__ __forceinline__ bool finite_bits(uint32_t b) { return (b & 0x7f800000u) != 0x7f800000u; }

// elements e .. e + 3 of a chunk of n: one 16-byte access where `vec` allows and all four exist, else one 4-byte access per element
// that exists (a load fills the rest with +0.0)
__device__ __forceinline__ float4 load4(const float* a, int e, int n, bool vec) {
    if (vec && e + 3 < n) return *reinterpret_cast<const float4*>(a + e);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < n) q.x = a[e];
    if (e + 1 < n) q.y = a[e + 1];
    if (e + 2 < n) q.z = a[e + 2];
    if (e + 3 < n) q.w = a[e + 3];
    return q;
}
__device__ __forceinline__ void store4(float* a, int e, int n, bool vec, const float4& q) {
    if (vec && e + 3 < n) { *reinterpret_cast<float4*>(a + e) = q; return; }
    if (e < n) a[e] = q.x;
    if (e + 1 < n) a[e + 1] = q.y;
    if (e + 2 < n) a[e + 2] = q.z;
    if (e + 3 < n) a[e + 3] = q.w;
}

struct OptChunk { const bg_mt_row* row; long long first; int n; };
__device__ __forceinline__ OptChunk open_chunk(const bg_mt_row* table, const bg_mt_chunk* chunks, int k) {
    const bg_mt_chunk c = chunks[k];
    const bg_mt_row* row = table + c.tensor;
    const long long left = row->numel - c.first;
    return OptChunk{row, c.first, (int)(left < OPT_CHUNK ? left : OPT_CHUNK)};
}

// ---- launch 1 ----------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(OPT_THREADS) void mt_grad_stats_kernel(const bg_mt_row* __restrict__ table, const bg_mt_chunk* __restrict__ chunks,
                                                                    int n_chunks, OptPartial* __restrict__ partials) {
    __shared__ double w_sum[OPT_THREADS / WAVE];
    __shared__ uint32_t w_max[OPT_THREADS / WAVE], w_bad[OPT_THREADS / WAVE];
    const int t = threadIdx.x;
    double acc = 0.0;
    uint32_t mx = 0u, bad = 0u;
    auto eat = [&](float g) {
        const uint32_t b = __float_as_uint(g) & 0x7fffffffu;
        if (finite_bits(b)) mx = max(mx, b);      // |g| of finite values orders like its bits
        else bad = 1u;
        acc += (double)g * (double)g;
    };
    for (int k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const OptChunk c = open_chunk(table, chunks, k);
        const float* g = c.row->g + c.first;
        const bool vec = ((uintptr_t)g & 15) == 0;
        float4 q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = load4(g, 4 * (t + OPT_THREADS * j), c.n, vec);      // + 0.0 changes neither sum, maximum nor flag
#pragma unroll
        for (int j = 0; j < 4; ++j) { eat(q[j].x); eat(q[j].y); eat(q[j].z); eat(q[j].w); }
    }
    acc = wave_sum_f64(acc);
    mx = wave_max_u32(mx);
    bad = wave_max_u32(bad);
    if ((t & (WAVE - 1)) == 0) { w_sum[t / WAVE] = acc; w_max[t / WAVE] = mx; w_bad[t / WAVE] = bad; }
    __syncthreads();
    if (t == 0) {
        OptPartial p;
        p.sumsq = ((w_sum[0] + w_sum[1]) + w_sum[2]) + w_sum[3];
        p.maxabs_bits = max(max(w_max[0], w_max[1]), max(w_max[2], w_max[3]));
        p.nonfinite = w_bad[0] | w_bad[1] | w_bad[2] | w_bad[3];
        partials[blockIdx.x] = p;
    }
}

// ---- what every later launch derives from the partials ------------------------------------------------------------------------------

struct OptVerdict { float norm, c, r; int found_inf; };

// One wave: lane l adds partials l, l + 64, .. in order, then the butterfly.  Called by wave 0 of a workgroup (all 64 lanes).
__device__ __forceinline__ OptVerdict judge(const OptPartial* partials, int n_partials, float max_norm, const bg_scaler_state* scaler, int lane) {
    double s = 0.0;
    uint32_t mx = 0u, bad = 0u;
    for (int i = lane; i < n_partials; i += WAVE) {
        const OptPartial q = partials[i];
        s += q.sumsq;
        mx = max(mx, q.maxabs_bits);
        bad |= q.nonfinite;
    }
    s = wave_sum_f64(s);
    mx = wave_max_u32(mx);
    bad = wave_max_u32(bad);
    OptVerdict v;
    v.norm = (float)sqrt(s);
    v.c = 1.0f;
    if (max_norm >= 0.f) {                         // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1)
        const float q = max_norm / (v.norm + 1e-6f);
        v.c = q < 1.0f ? q : 1.0f;
    }
    v.r = scaler ? (float)(1.0 / (double)scaler->scale) : 1.0f;
    // rounding is monotonic: if the largest finite |g| survives both multiplications, every smaller one does
    float big = __uint_as_float(mx) * v.c;
    big = big * v.r;
    v.found_inf = (bad != 0u || !finite_bits(__float_as_uint(big))) ? 1 : 0;
    return v;
}

struct OptHyper { float one_minus_b1, b2, one_minus_b2, eps; };

// ---- launch 2 ----------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float c, float r, float f, bool decay, const OptHyper& h,
                                           float bc2_sqrt, float step_size) {
    float gg = g * c;
    gg = gg * r;
    if (decay) p = p * f;
    const float d = gg - m;
    m = m + d * h.one_minus_b1;
    const float sq = gg * gg;
    v = v * h.b2 + h.one_minus_b2 * sq;
    const float denom = sqrtf(v) / bc2_sqrt + h.eps;
    p = p - step_size * (m / denom);
}

__global__ __launch_bounds__(OPT_THREADS) void mt_adamw_step_kernel(const bg_mt_row* __restrict__ table, const bg_mt_chunk* __restrict__ chunks,
                                                                    int n_chunks, const OptPartial* __restrict__ partials, int n_partials,
                                                                    const bg_optim_state* __restrict__ state, const bg_scaler_state* __restrict__ scaler,
                                                                    float max_norm, double beta1, double beta2, OptHyper h) {
    __shared__ float sh_c, sh_r;
    __shared__ int sh_inf;
    const int t = threadIdx.x;
    if (t < WAVE) {
        const OptVerdict v = judge(partials, n_partials, max_norm, scaler, t);
        if (t == 0) { sh_c = v.c; sh_r = v.r; sh_inf = v.found_inf; }
    }
    __syncthreads();
    if (sh_inf) return;
    const float c = sh_c, r = sh_r;
    // bias corrections of step + 1 from the fp64 powers the finish launch keeps (beta^step; one multiplication more here)
    const double bc1 = 1.0 - state->beta1_pow * beta1, bc2 = 1.0 - state->beta2_pow * beta2;
    const float bc2_sqrt = (float)sqrt(bc2);
    for (int k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const OptChunk ck = open_chunk(table, chunks, k);
        const bg_mt_row* row = ck.row;
        float* p = row->p + ck.first;
        const float* g = row->g + ck.first;
        float* m = row->m + ck.first;
        float* v = row->v + ck.first;
        const float f = row->decay;
        const bool decay = row->has_decay != 0;
        const float step_size = (float)(row->lr / bc1);
        const bool vec = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
        float4 P[4], G[4], M[4], V[4];      // every load of the chunk is in flight before the first result is stored
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * (t + OPT_THREADS * j);
            P[j] = load4(p, e, ck.n, vec);
            G[j] = load4(g, e, ck.n, vec);
            M[j] = load4(m, e, ck.n, vec);
            V[j] = load4(v, e, ck.n, vec);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * (t + OPT_THREADS * j);
            adamw_elem(P[j].x, G[j].x, M[j].x, V[j].x, c, r, f, decay, h, bc2_sqrt, step_size);
            adamw_elem(P[j].y, G[j].y, M[j].y, V[j].y, c, r, f, decay, h, bc2_sqrt, step_size);
            adamw_elem(P[j].z, G[j].z, M[j].z, V[j].z, c, r, f, decay, h, bc2_sqrt, step_size);
            adamw_elem(P[j].w, G[j].w, M[j].w, V[j].w, c, r, f, decay, h, bc2_sqrt, step_size);
            store4(p, e, ck.n, vec, P[j]);
            store4(m, e, ck.n, vec, M[j]);
            store4(v, e, ck.n, vec, V[j]);
        }
    }
}

// ---- launch 3 ----------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(WAVE) void optim_finish_kernel(const OptPartial* __restrict__ partials, int n_partials, bg_optim_state* __restrict__ state,
                                                            bg_scaler_state* __restrict__ scaler, float max_norm, double beta1, double beta2,
                                                            double growth, double backoff, int growth_interval) {
    const OptVerdict v = judge(partials, n_partials, max_norm, scaler, threadIdx.x);
    if (threadIdx.x != 0) return;
    state->total_norm = v.norm;
    state->found_inf = v.found_inf;
    if (v.found_inf) {
        if (scaler) { scaler->scale = (float)((double)scaler->scale * backoff); scaler->growth_tracker = 0; }      // _amp_update_scale_: the factors are doubles
        return;
    }
    if (n_partials > 0) {                          // no chunk, no update: the counter stays
        state->step = state->step + 1;
        state->beta1_pow = state->beta1_pow * beta1;
        state->beta2_pow = state->beta2_pow * beta2;
    }
    if (scaler) {
        const int tr = scaler->growth_tracker + 1;
        if (tr == growth_interval) {
            const float grown = (float)((double)scaler->scale * growth);
            if (finite_bits(__float_as_uint(grown))) scaler->scale = grown;
            scaler->growth_tracker = 0;
        } else scaler->growth_tracker = tr;
    }
}

// ---- stand-alone clipping ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(OPT_THREADS) void mt_scale_grads_kernel(const bg_mt_row* __restrict__ table, const bg_mt_chunk* __restrict__ chunks,
                                                                     int n_chunks, const OptPartial* __restrict__ partials, int n_partials,
                                                                     float max_norm, float* __restrict__ norm_out) {
    __shared__ float sh_c;
    const int t = threadIdx.x;
    if (t < WAVE) {
        const OptVerdict v = judge(partials, n_partials, max_norm, nullptr, t);
        if (t == 0) {
            sh_c = v.c;
            if (blockIdx.x == 0 && norm_out) *norm_out = v.norm;
        }
    }
    __syncthreads();
    const float c = sh_c;
    for (int k = blockIdx.x; k < n_chunks; k += gridDim.x) {
        const OptChunk ck = open_chunk(table, chunks, k);
        float* g = const_cast<float*>(ck.row->g) + ck.first;
        const bool vec = ((uintptr_t)g & 15) == 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = 4 * (t + OPT_THREADS * j);
            float4 q = load4(g, e, ck.n, vec);
            q.x = q.x * c; q.y = q.y * c; q.z = q.z * c; q.w = q.w * c;
            store4(g, e, ck.n, vec, q);
        }
    }
}

static int check_lists(const char* what, const bg_mt_row* table, const bg_mt_chunk* chunks, int n_chunks, const void* partials) {
    BG_REQUIRE(n_chunks >= 0, BG_E_SHAPE, "%s: n_chunks = %d", what, n_chunks);
    if (n_chunks == 0) return 0;
    BG_REQUIRE(table && chunks && partials, BG_E_ARG, "%s: null table, chunk list or partials", what);
    BG_REQUIRE((uintptr_t)table % 8 == 0 && (uintptr_t)chunks % 16 == 0 && (uintptr_t)partials % 16 == 0, BG_E_ALIGN,
               "%s: table must be 8-byte, chunk list and partials 16-byte aligned", what);
    return 0;
}
static int grid_of(int n_chunks) { return n_chunks < OPT_MAX_BLOCKS ? n_chunks : OPT_MAX_BLOCKS; }

}  // namespace bg

extern "C" int bg_mt_grad_stats(const bg_mt_row* table, const bg_mt_chunk* chunks, int n_chunks, void* partials, bg_stream_t stream) {
    if (int rc = bg::check_lists("bg_mt_grad_stats", table, chunks, n_chunks, partials)) return rc;
    if (n_chunks == 0) return 0;
    bg::ProfScope prof(bg::PK_MISC, 0.0, 4.0 * bg::OPT_CHUNK * (double)n_chunks, (hipStream_t)stream);
    hipLaunchKernelGGL(bg::mt_grad_stats_kernel, dim3(bg::grid_of(n_chunks)), dim3(bg::OPT_THREADS), 0, (hipStream_t)stream, table, chunks, n_chunks,
                       (bg::OptPartial*)partials);
    return bg::launch_status("bg_mt_grad_stats");
}

extern "C" int bg_mt_adamw_step(const bg_mt_row* table, const bg_mt_chunk* chunks, int n_chunks, const void* partials,
                                const bg_optim_state* state, const bg_scaler_state* scaler, float max_norm, double beta1, double beta2,
                                double eps, bg_stream_t stream) {
    if (int rc = bg::check_lists("bg_mt_adamw_step", table, chunks, n_chunks, partials)) return rc;
    BG_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.0, BG_E_ARG,
               "bg_mt_adamw_step: need 0 <= beta < 1 and eps >= 0 (beta1=%g beta2=%g eps=%g)", beta1, beta2, eps);
    if (n_chunks == 0) return 0;
    BG_REQUIRE(state, BG_E_ARG, "bg_mt_adamw_step: null state");
    BG_REQUIRE((uintptr_t)state % 8 == 0 && (uintptr_t)scaler % 4 == 0, BG_E_ALIGN, "bg_mt_adamw_step: state must be 8-byte, scaler 4-byte aligned");
    const bg::OptHyper h{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
    bg::ProfScope prof(bg::PK_MISC, 0.0, 28.0 * bg::OPT_CHUNK * (double)n_chunks, (hipStream_t)stream);
    hipLaunchKernelGGL(bg::mt_adamw_step_kernel, dim3(bg::grid_of(n_chunks)), dim3(bg::OPT_THREADS), 0, (hipStream_t)stream, table, chunks, n_chunks,
                       (const bg::OptPartial*)partials, bg::grid_of(n_chunks), state, scaler, max_norm, beta1, beta2, h);
    return bg::launch_status("bg_mt_adamw_step");
}

extern "C" int bg_optim_finish(const void* partials, int n_chunks, bg_optim_state* state, bg_scaler_state* scaler, float max_norm, double beta1,
                               double beta2, double growth_factor, double backoff_factor, int growth_interval, bg_stream_t stream) {
    BG_REQUIRE(n_chunks >= 0, BG_E_SHAPE, "bg_optim_finish: n_chunks = %d", n_chunks);
    BG_REQUIRE(state && (partials || n_chunks == 0), BG_E_ARG, "bg_optim_finish: null state or partials");
    BG_REQUIRE((uintptr_t)state % 8 == 0 && (uintptr_t)scaler % 4 == 0 && (uintptr_t)partials % 16 == 0, BG_E_ALIGN,
               "bg_optim_finish: state must be 8-byte, scaler 4-byte, partials 16-byte aligned");
    BG_REQUIRE(!scaler || growth_interval >= 1, BG_E_ARG, "bg_optim_finish: growth_interval = %d", growth_interval);
    hipLaunchKernelGGL(bg::optim_finish_kernel, dim3(1), dim3(bg::WAVE), 0, (hipStream_t)stream, (const bg::OptPartial*)partials,
                       bg::grid_of(n_chunks), state, scaler, max_norm, beta1, beta2, growth_factor, backoff_factor, growth_interval);
    return bg::launch_status("bg_optim_finish");
}

extern "C" int bg_mt_scale_grads(const bg_mt_row* table, const bg_mt_chunk* chunks, int n_chunks, const void* partials, float max_norm,
                                 float* norm_out, bg_stream_t stream) {
    if (int rc = bg::check_lists("bg_mt_scale_grads", table, chunks, n_chunks, partials)) return rc;
    BG_REQUIRE(max_norm >= 0.f, BG_E_ARG, "bg_mt_scale_grads: max_norm = %g", (double)max_norm);
    BG_REQUIRE((uintptr_t)norm_out % 4 == 0, BG_E_ALIGN, "bg_mt_scale_grads: norm_out must be 4-byte aligned");
    if (n_chunks == 0) {
        if (norm_out) {
            const hipError_t e = hipMemsetAsync(norm_out, 0, sizeof(float), (hipStream_t)stream);
            BG_REQUIRE(e == hipSuccess, (int)e, "bg_mt_scale_grads: clearing the norm failed: %s", hipGetErrorString(e));
        }
        return 0;
    }
    bg::ProfScope prof(bg::PK_MISC, 0.0, 8.0 * bg::OPT_CHUNK * (double)n_chunks, (hipStream_t)stream);
    hipLaunchKernelGGL(bg::mt_scale_grads_kernel, dim3(bg::grid_of(n_chunks)), dim3(bg::OPT_THREADS), 0, (hipStream_t)stream, table, chunks, n_chunks,
                       (const bg::OptPartial*)partials, bg::grid_of(n_chunks), max_norm, norm_out);
    return bg::launch_status("bg_mt_scale_grads");
}
