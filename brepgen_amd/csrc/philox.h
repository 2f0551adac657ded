// Philox4x32-10 and the 32-bit word -> uniform map, defined once for the kernels that draw on the device (rng.hip: bg_philox_randn,
// mesh_sample.hip: bg_mesh_sample).  Every user keys the generator with the run's seed and builds its counter from GLOBAL indices plus a
// 16-bit domain tag in the top half-word of word 3, so no two users ever share a counter.  oracle/philox.py restates it in numpy.
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

}  // namespace bg
