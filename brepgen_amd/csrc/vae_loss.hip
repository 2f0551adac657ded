// Posterior of the two VAE trainers (trainer.py:79-84, 118-119, 206-214, 248-249): diffusers' DiagonalGaussianDistribution on the
// moments the encoder programs write -- clamp the log-variance, draw z = mean + std * eps, and the per-sample KL to N(0, I) -- in ONE
// launch between the encode and the decode program.
//
// Mapping.  The kernel is memory-trivial (<= 40 B per latent element, a sample is 12 or 48 elements), so what matters is that no
// lane repeats work and that the per-sample sum needs neither LDS nor atomics:
//   - the unit of work is one Philox block = 4 consecutive elements of a sample in the noise order (c, p): a lane draws (or loads)
//     its four eps once, nothing is drawn twice;
//   - a sample's blocks go to G ADJACENT lanes of one wave, G = the power of two >= the block count, at most 64 (12 elements: 4
//     lanes, 16 samples per wave; 48 elements: 16 lanes, 4 samples per wave; longer samples: one wave each, looping), so the
//     sample's few hundred bytes are touched by one wave instruction and its KL is a butterfly over G lanes;
//   - the KL terms are formed and summed in fp64 (mean^2 + (expm1(lv) - lv): in fp32 var - 1 - lv cancels to nothing near lv = 0,
//     where a trained posterior lives), in an order fixed by (P * L) alone: the lane's blocks ascending, then the butterfly.  The
//     result is rounded to fp32 once.  No atomics: a sample's value does not depend on the batch, the grid or the call.
#include "bg_common.h"
#include "philox.h"

namespace bg {

__global__ __launch_bounds__(256) void vae_posterior_kernel(const float* __restrict__ moments, const float* __restrict__ noise,
                                                            long long n, int P, int L, int G, uint32_t seed_lo, uint32_t seed_hi,
                                                            uint32_t draw, long long sample0, float* __restrict__ z,
                                                            float* __restrict__ lv_out, float* __restrict__ kl) {
    const int E = P * L, blocks_per = E / 4 + ((E & 3) != 0);
    const int lig = threadIdx.x & (G - 1);                          // lane in its sample's group
    const long long spb = 256 / G;                                  // samples per workgroup and round
    const long long rounds = (n + spb * gridDim.x - 1) / (spb * gridDim.x);
    for (long long r = 0; r < rounds; ++r) {                        // the same trip count in every lane: the shuffles below are convergent
        const long long b = (r * gridDim.x + blockIdx.x) * spb + threadIdx.x / G;
        const bool valid = b < n;
        double acc = 0.0;
        if (valid) {
            const float* mo = moments + b * 2 * E;
            for (int k = lig; k < blocks_per; k += G) {
                const int e0 = 4 * k, left = E - e0;
                float eps[4];
                if (noise != nullptr) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) eps[j] = j < left ? noise[b * E + e0 + j] : 0.f;
                } else {
                    philox_randn4<false>(eps, (uint32_t)k, (unsigned long long)(sample0 + b), draw, seed_lo, seed_hi);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j >= left) break;
                    const int e = e0 + j, c = e / P, p = e - c * P;  // noise order (c, p) -> channels-last (p, c)
                    const float mean = mo[(long long)p * 2 * L + c], raw = mo[(long long)p * 2 * L + L + c];
                    const float lv = raw < -30.f ? -30.f : (raw > 20.f ? 20.f : raw);      // torch.clamp: a NaN stays a NaN
                    const float sd = expf(0.5f * lv);
                    const float t = sd * eps[j];                     // two roundings (-ffp-contract=off), like mean + std * eps in torch
                    const long long o = b * E + (long long)p * L + c;
                    z[o] = mean + t;
                    if (lv_out != nullptr) lv_out[o] = lv;
                    if (kl != nullptr) {
                        const double dm = (double)mean, dl = (double)lv;
                        acc += dm * dm + (expm1(dl) - dl);
                    }
                }
            }
        }
        if (kl != nullptr) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
                if (o < G) acc += __shfl_xor(acc, o, 64);
            if (valid && lig == 0) kl[b] = (float)(0.5 * acc);
        }
    }
}

}  // namespace bg

extern "C" int bg_vae_posterior(const float* moments, const float* noise, long long n, int P, int L, unsigned long long seed,
                                unsigned draw_id, long long first_sample, float* z_out, float* logvar_out, float* kl_out,
                                bg_stream_t stream) {
    using namespace bg;
    BG_REQUIRE(moments != nullptr && z_out != nullptr, BG_E_ARG, "bg_vae_posterior: null moments or z_out");
    BG_REQUIRE(n >= 0 && P > 0 && L > 0 && first_sample >= 0, BG_E_SHAPE, "bg_vae_posterior: bad shape n=%lld P=%d L=%d first_sample=%lld",
               n, P, L, first_sample);
    // element e of a sample is word (e % 4) of Philox block e / 4, and bg_philox_randn counts a sample's elements in an int
    BG_REQUIRE((long long)P * L <= 0x7FFFFFFFll, BG_E_SHAPE, "bg_vae_posterior: P * L = %lld elements per sample exceed the Philox block counter",
               (long long)P * L);
    if (n == 0) return 0;
    const int blocks_per = P * L / 4 + ((P * L & 3) != 0);
    int G = 1;
    while (G < blocks_per && G < 64) G <<= 1;
    const long long spb = 256 / G, wgs = (n + spb - 1) / spb;
    const int grid = (int)(wgs < 4096 ? wgs : 4096);
    ProfScope prof(PK_MISC, 0.0, (double)n * P * L * (noise ? 24.0 : 20.0), (hipStream_t)stream);
    hipLaunchKernelGGL(vae_posterior_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, moments, noise, n, P, L, G, (uint32_t)seed,
                       (uint32_t)(seed >> 32), draw_id, first_sample, z_out, logvar_out, kl_out);
    return launch_status("vae_posterior");
}
