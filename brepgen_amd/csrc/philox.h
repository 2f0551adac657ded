// Philox4x32-10 and the 32-bit word -> uniform map, defined once for the kernels that draw on the device (rng.hip: bg_philox_randn,
// mesh_sample.hip: bg_mesh_sample, vae_loss.hip: bg_vae_posterior).  Every user keys the generator with the run's seed and builds its counter from GLOBAL indices plus a
// 16-bit domain tag in the top half-word of word 3, so no two users ever share a counter.  oracle/philox.py restates it in numpy.
// Tags in use: 0xB9E5 bg_philox_randn / bg_vae_posterior, 0x5A3D bg_mesh_sample, 0xDA7A bg_batch_plan, 0xDA7B bg_points_rotate_normalize,
// 0xAD70 the attention dropout mask (attn_train.hip: bg_attn_train_fwd / bg_attn_bwd / bg_attn_dropout_mask), 0xD409 the elementwise
// dropout masks of an encoder layer (layer_train.hip: bg_dropout_add_fwd / bg_dropout_bwd / bg_relu_dropout_fwd / bg_dropout_mask).
#pragma once
#include "bg_common.h"

namespace bg {

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// u32 -> uniform in (0, 1): the top 23 bits, centred.  k + 0.5 with k < 2^23 is exactly representable in fp32 (24
// significant bits), so the 2^23 grid points are equally spaced, none is 0 and none is 1.
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f); }

// Element block `blk` (elements 4 blk .. 4 blk + 3) of GLOBAL sample `gs` of draw `draw` of bg_philox_randn's stream (domain tag
// 0xB9E5): one Philox block -> 2 Box-Muller pairs -> 4 N(0,1) values (RAW: the four words themselves, bit pattern in the float slots).
// The one definition of that stream: bg_philox_randn writes it out, bg_vae_posterior consumes it in place -- same bits.
template <bool RAW>
__device__ __forceinline__ void philox_randn4(float (&v)[4], uint32_t blk, unsigned long long gs, uint32_t draw, uint32_t seed_lo,
                                              uint32_t seed_hi) {
    uint32_t c[4] = {blk, (uint32_t)gs, draw, 0xB9E50000u | (uint32_t)((gs >> 32) & 0xFFFFu)};
    philox4x32_10(c, seed_lo, seed_hi);
    if (RAW) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __uint_as_float(c[j]);
    } else {
        const float r0 = sqrtf(-2.0f * logf(u01(c[0]))), r1 = sqrtf(-2.0f * logf(u01(c[2])));
        const float a0 = 6.28318530717958647692f * u01(c[1]), a1 = 6.28318530717958647692f * u01(c[3]);
        v[0] = r0 * cosf(a0); v[1] = r0 * sinf(a0); v[2] = r1 * cosf(a1); v[3] = r1 * sinf(a1);
    }
}

// ---- what the two dropout-mask families (0xAD70: attn_train.hip, 0xD409: layer_train.hip) share ----
// word 3 of the counter = tag_sub | bits 32..43 of the GLOBAL sample index gs; tag_sub = domain tag | 4-bit sub-stream (head / site) << 12
__host__ __device__ inline uint32_t drop_tag_sub(uint32_t tag, uint32_t sub) { return tag | (sub << 12); }
__device__ __forceinline__ uint32_t drop_word3(uint32_t tag_sub, unsigned long long gs) { return tag_sub | (uint32_t)((gs >> 32) & 0xFFFu); }
// host: checks p in [0, 1) (NaN fails) and 0 <= first_sample, first_sample + B <= 2^44, and fills the seed halves, draw, first and
// rp = float(1 / (1 - p)).  Returns which check failed first, in that order; the entry words its own message (and its threshold).
enum { DROP_OK = 0, DROP_BAD_P, DROP_NEGATIVE_FIRST, DROP_FIRST_PAST_2_44 };
inline int drop_key_common(int B, double p, unsigned long long seed, unsigned draw_id, long long first_sample, uint32_t& seed_lo,
                           uint32_t& seed_hi, uint32_t& draw, unsigned long long& first, float& rp) {
    if (!(p >= 0.0 && p < 1.0)) return DROP_BAD_P;
    if (first_sample < 0) return DROP_NEGATIVE_FIRST;
    if ((unsigned long long)first_sample + (unsigned long long)(B > 0 ? B : 0) > (1ull << 44)) return DROP_FIRST_PAST_2_44;
    seed_lo = (uint32_t)seed; seed_hi = (uint32_t)(seed >> 32); draw = draw_id;
    first = (unsigned long long)first_sample;
    rp = (float)(1.0 / (1.0 - p));
    return DROP_OK;
}

}  // namespace bg
