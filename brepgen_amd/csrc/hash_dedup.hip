// Training-set de-duplication of the reference's data_process/ (deduplicate_cad.py, deduplicate_surfedge.py) on the device: the SHA-256
// of every quantised point grid, the order-free key of a CAD's faces, and "first occurrence wins" over millions of 32-byte keys.
// (dedup.hip is something else: the bounding-box de-duplication between the stages of the sampling cascade.)
//
//   bg_points_sha256       real2bit + sha256(int64 bytes) fused, ONE LANE PER ITEM (SHA-256 is sequential per message; the parallelism
//                          is across items).  The int64 message never exists: after the clip the high half of every value is zero, so
//                          of the 16 words of a block the 8 odd ones are the constant 0 and the 8 even ones are the byte-swapped
//                          quantised values -- one block eats 8 floats.  A lane reading its own 12 KiB item would be uncoalesced, so
//                          the wave fetches the next 32 floats (4 blocks) of its 64 items cooperatively -- 128 contiguous bytes per
//                          item, 16-byte loads where the items are 16-byte aligned -- into registers while it hashes the current slab,
//                          and hands them over through LDS (row stride 33 words: lane = item reads hit 64 different banks).
//   bg_digest_group_keys   one workgroup (one wave) per CAD: rank every digest by counting the smaller ones (ties by position: a CAD may
//                          hold the same face twice), stage them sorted in LDS, hash the concatenation.
//   bg_first_occurrence    an open-addressing table of item indices in device memory: claim with atomicCAS, lower with atomicMin, then
//                          look the key up again.  The probe order varies from run to run, the minimum index per key does not.
//
// Everything is integer work on plain VGPRs; device memory is written with vector stores and int32 atomics only.
#include "bg_common.h"

namespace bg {

constexpr int HD_P_MAX = 1024, HD_BITS_MAX = 16, HD_GROUP_MAX = 4096;
constexpr int HD_SLAB = 32;                 // floats of an item per slab = 4 SHA-256 blocks
constexpr int HD_STRIDE = HD_SLAB + 1;      // LDS row stride in words (odd: conflict-free for lane = row)
constexpr int HD_THREADS = 256;             // first-occurrence kernels

__device__ __constant__ static const uint32_t SHA_K[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
    0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
    0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
    0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
    0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
    0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }      // v_alignbit_b32
__device__ __forceinline__ void sha_init(uint32_t (&st)[8]) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}
// One compression.  w is the block on entry and the rolling 16-word schedule afterwards (every index is a compile-time constant once
// the 64 rounds are unrolled: state and schedule live in 24 registers).  Words that the caller set to a literal 0 fold away.
__device__ __forceinline__ void sha_block(uint32_t (&st)[8], uint32_t (&w)[16]) {
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
            w[i & 15] += (rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3)) + w[(i - 7) & 15] + (rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10));
        }
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) | (~e & g)) + SHA_K[i] + w[i & 15];
        const uint32_t ab = a ^ b;
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((ab & c) | (~ab & b));      // Maj(a, b, c) as one bit-select
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}
__device__ __forceinline__ void sha_store(const uint32_t (&st)[8], uint8_t* out) {      // big-endian digest bytes, out 16-byte aligned
    uint4* o = reinterpret_cast<uint4*>(out);
    o[0] = make_uint4(__builtin_bswap32(st[0]), __builtin_bswap32(st[1]), __builtin_bswap32(st[2]), __builtin_bswap32(st[3]));
    o[1] = make_uint4(__builtin_bswap32(st[4]), __builtin_bswap32(st[5]), __builtin_bswap32(st[6]), __builtin_bswap32(st[7]));
}

// convert_utils.real2bit in its own order -- (x + 1) * (2^n - 1) / 2, one fp32 rounding each (the build forbids the fma; halving is
// exact), clip, truncate -- as the big-endian message word of the int64's low half.  A NaN quantises to 0.
__device__ __forceinline__ uint32_t quant_word(float x, float range) {
    float t = x + 1.0f;
    t = t * range;
    t = t * 0.5f;
    t = t > 0.f ? t : 0.f;
    t = t < range ? t : range;
    return __builtin_bswap32((uint32_t)t);
}

// ---- quantise + SHA-256, one lane per item -----------------------------------------------------------------------------------------------

template <bool VEC> __global__ __launch_bounds__(WAVE) void points_sha256_kernel(const float* __restrict__ x, long long M, int P, float range,
                                                                                 uint8_t* __restrict__ digest) {
    __shared__ float slab[WAVE * HD_STRIDE];
    const int lane = threadIdx.x;
    const long long item0 = (long long)blockIdx.x * WAVE;
    const int n = 3 * P, full = n >> 3, r = n & 7, n_slabs = (n + HD_SLAB - 1) / HD_SLAB;
    float pre[HD_SLAB];                       // the wave's next slab: 64 items x 32 floats over 64 lanes

    auto fetch = [&](int s) {
        if (VEC) {
#pragma unroll
            for (int k = 0; k < HD_SLAB / 4; ++k) {
                const int u = k * WAVE + lane, it = u >> 3, fl = s * HD_SLAB + (u & 7) * 4;      // 8 lanes x 16 bytes = one item's 128 bytes
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (item0 + it < M && fl < n) v = *reinterpret_cast<const float4*>(x + (size_t)(item0 + it) * n + fl);      // n % 4 == 0 here
                pre[4 * k] = v.x; pre[4 * k + 1] = v.y; pre[4 * k + 2] = v.z; pre[4 * k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < HD_SLAB; ++k) {
                const int u = k * WAVE + lane, it = u >> 5, fl = s * HD_SLAB + (u & 31);
                pre[k] = (item0 + it < M && fl < n) ? x[(size_t)(item0 + it) * n + fl] : 0.f;
            }
        }
    };
    auto stash = [&]() {
        if (VEC) {
#pragma unroll
            for (int k = 0; k < HD_SLAB / 4; ++k) {
                const int u = k * WAVE + lane, at = (u >> 3) * HD_STRIDE + (u & 7) * 4;
#pragma unroll
                for (int c = 0; c < 4; ++c) slab[at + c] = pre[4 * k + c];
            }
        } else {
#pragma unroll
            for (int k = 0; k < HD_SLAB; ++k) {
                const int u = k * WAVE + lane;
                slab[(u >> 5) * HD_STRIDE + (u & 31)] = pre[k];
            }
        }
    };

    uint32_t st[8], w[16];
    sha_init(st);
    const float* mine = slab + lane * HD_STRIDE;
    fetch(0);
    for (int s = 0; s < n_slabs; ++s) {
        __syncthreads();                      // the previous slab has been read
        stash();
        __syncthreads();
        if (s + 1 < n_slabs) fetch(s + 1);    // in flight under the four compressions below
        const int here = min(HD_SLAB / 8, full - s * (HD_SLAB / 8));
#pragma unroll 1
        for (int b = 0; b < here; ++b) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                w[2 * k] = quant_word(mine[b * 8 + k], range);
                w[2 * k + 1] = 0u;
            }
            sha_block(st, w);
        }
    }
    // the last r values (they sit in the slab still in LDS), the 0x80 byte and the bit length: one block, or two where the length
    // field does not fit behind 56 bytes of data (r == 7)
    const int tb = r ? full * 8 - (n_slabs - 1) * HD_SLAB : 0;
    const uint32_t bits = 192u * (uint32_t)P;
#pragma unroll 1
    for (int t = 0; t < (r == 7 ? 2 : 1); ++t) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t q = quant_word(mine[tb + k], range);
            w[2 * k] = t ? 0u : (k < r ? q : (k == r ? 0x80000000u : 0u));
            w[2 * k + 1] = 0u;
        }
        if (t || r < 7) w[15] = bits;
        sha_block(st, w);
    }
    if (item0 + lane < M) sha_store(st, digest + (size_t)(item0 + lane) * 32);
}

// ---- the key of a group: SHA-256 of its digests in byte order ------------------------------------------------------------------------------

__global__ __launch_bounds__(WAVE) void group_keys_kernel(const uint8_t* __restrict__ digest, const int* __restrict__ off, int max_group,
                                                          uint8_t* __restrict__ key) {
    extern __shared__ uint32_t sorted[];      // [max_group][8]: the digests as big-endian words (word order = byte order), sorted
    const int n = blockIdx.x, lane = threadIdx.x;
    const int o0 = off[n];
    int g = off[n + 1] - o0;
    g = (o0 < 0 || g < 0) ? 0 : min(g, max_group);          // the caller owns the offsets; the kernel only stays inside its LDS
    const uint4* d = reinterpret_cast<const uint4*>(digest) + 2 * (size_t)o0;
    for (int i = lane; i < g; i += WAVE) {
        const uint4 lo = d[2 * i], hi = d[2 * i + 1];
        const uint32_t m[8] = {__builtin_bswap32(lo.x), __builtin_bswap32(lo.y), __builtin_bswap32(lo.z), __builtin_bswap32(lo.w),
                               __builtin_bswap32(hi.x), __builtin_bswap32(hi.y), __builtin_bswap32(hi.z), __builtin_bswap32(hi.w)};
        int rank = 0;
        for (int j = 0; j < g; ++j) {
            const uint4 a = d[2 * j];
            const uint32_t a0 = __builtin_bswap32(a.x), a1 = __builtin_bswap32(a.y);
            bool less;
            if (a0 != m[0]) less = a0 < m[0];
            else if (a1 != m[1]) less = a1 < m[1];
            else {                                            // 64 equal bits: almost always the same face again
                const uint4 b = d[2 * j + 1];
                const uint32_t o[6] = {__builtin_bswap32(a.z), __builtin_bswap32(a.w), __builtin_bswap32(b.x), __builtin_bswap32(b.y),
                                       __builtin_bswap32(b.z), __builtin_bswap32(b.w)};
                less = j < i;                                 // ties: by position
                bool decided = false;
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    if (!decided && o[k] != m[2 + k]) { less = o[k] < m[2 + k]; decided = true; }
            }
            rank += less ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) sorted[rank * 8 + k] = m[k];
    }
    __syncthreads();
    uint32_t st[8], w[16];                    // every lane hashes the same message (LDS broadcasts); lane 0 stores
    sha_init(st);
#pragma unroll 1
    for (int b = 0; b < (g >> 1); ++b) {
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = sorted[b * 16 + k];
        sha_block(st, w);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = 0u;
    if (g & 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = sorted[(g - 1) * 8 + k];
        w[8] = 0x80000000u;
    } else w[0] = 0x80000000u;
    w[15] = 256u * (uint32_t)g;
    sha_block(st, w);
    if (lane == 0) sha_store(st, key + (size_t)n * 32);
}

// ---- first occurrence --------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool same_key(const uint4* key, long long i, const uint4& lo, const uint4& hi) {
    const uint4 a = key[2 * i], b = key[2 * i + 1];
    return a.x == lo.x && a.y == lo.y && a.z == lo.z && a.w == lo.w && b.x == hi.x && b.y == hi.y && b.z == hi.z && b.w == hi.w;
}
__device__ __forceinline__ unsigned long long home_slot(const uint4& lo, unsigned long long mask) {
    return (((unsigned long long)lo.y << 32) | lo.x) & mask;          // the first 8 bytes, little-endian
}

// claim an empty slot, or lower the index in the slot that this key owns.  Every index ever stored in a slot belongs to ONE key (a slot
// leaves -1 once, by the CAS of an item of that key, and afterwards only items of that key write to it), so comparing with whichever
// owner is read is valid; and a key owns one slot only: the first of its probe sequence that was not taken by another key.
__global__ __launch_bounds__(HD_THREADS) void first_claim_kernel(const uint4* __restrict__ key, long long N, int* __restrict__ table,
                                                                 unsigned long long mask) {
    const long long i = (long long)blockIdx.x * HD_THREADS + threadIdx.x;
    if (i >= N) return;
    const uint4 lo = key[2 * i], hi = key[2 * i + 1];
    unsigned long long s = home_slot(lo, mask);
    for (unsigned long long tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
        const int cur = atomicCAS(table + s, -1, (int)i);
        if (cur == -1) return;
        if (cur < 0 || cur >= N) return;                      // not a table this entry filled
        if (same_key(key, cur, lo, hi)) {
            atomicMin(table + s, (int)i);
            return;
        }
    }
}
__global__ __launch_bounds__(HD_THREADS) void first_keep_kernel(const uint4* __restrict__ key, long long N, const int* __restrict__ table,
                                                                unsigned long long mask, uint8_t* __restrict__ keep) {
    const long long i = (long long)blockIdx.x * HD_THREADS + threadIdx.x;
    if (i >= N) return;
    const uint4 lo = key[2 * i], hi = key[2 * i + 1];
    unsigned long long s = home_slot(lo, mask);
    uint8_t first = 0;
    for (unsigned long long tries = 0; tries <= mask; ++tries, s = (s + 1) & mask) {
        const int cur = table[s];
        if (cur < 0 || cur >= N) break;
        if (same_key(key, cur, lo, hi)) {
            first = cur == i ? 1 : 0;
            break;
        }
    }
    keep[i] = first;
}

}  // namespace bg

extern "C" int bg_points_sha256(const float* x, long long M, int P, int n_bits, uint8_t* digest, bg_stream_t stream) {
    BG_REQUIRE(M >= 0 && P >= 1 && P <= bg::HD_P_MAX && n_bits >= 1 && n_bits <= bg::HD_BITS_MAX, BG_E_SHAPE,
               "bg_points_sha256: need M >= 0, 1 <= P <= %d, 1 <= n_bits <= %d (M=%lld P=%d n_bits=%d)", bg::HD_P_MAX, bg::HD_BITS_MAX, M, P,
               n_bits);
    if (M == 0) return 0;
    BG_REQUIRE(x && digest, BG_E_ARG, "bg_points_sha256: null x or digest");
    BG_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)digest % 16 == 0, BG_E_ALIGN, "bg_points_sha256: x must be 4-byte, digest 16-byte aligned");
    const long long blocks = (M + bg::WAVE - 1) / bg::WAVE;
    BG_REQUIRE(blocks <= 0x7fffffffLL, BG_E_SHAPE, "bg_points_sha256: M = %lld is too large for one call", M);
    const float range = (float)((1 << n_bits) - 1);
    const bool vec = P % 4 == 0 && (uintptr_t)x % 16 == 0;
    bg::ProfScope prof(bg::PK_MISC, 0.0, (double)M * (12.0 * P + 32.0), (hipStream_t)stream);
    if (vec) hipLaunchKernelGGL(bg::points_sha256_kernel<true>, dim3((unsigned)blocks), dim3(bg::WAVE), 0, (hipStream_t)stream, x, M, P, range, digest);
    else hipLaunchKernelGGL(bg::points_sha256_kernel<false>, dim3((unsigned)blocks), dim3(bg::WAVE), 0, (hipStream_t)stream, x, M, P, range, digest);
    return bg::launch_status("bg_points_sha256");
}

extern "C" int bg_digest_group_keys(const uint8_t* digest, const int* off, int N, int max_group, uint8_t* key, bg_stream_t stream) {
    BG_REQUIRE(N >= 0 && max_group >= 0 && max_group <= bg::HD_GROUP_MAX, BG_E_SHAPE,
               "bg_digest_group_keys: need N >= 0, 0 <= max_group <= %d (N=%d max_group=%d)", bg::HD_GROUP_MAX, N, max_group);
    if (N == 0) return 0;
    BG_REQUIRE(off && key && (digest || max_group == 0), BG_E_ARG, "bg_digest_group_keys: null digest, off or key");
    BG_REQUIRE((uintptr_t)digest % 16 == 0 && (uintptr_t)key % 16 == 0 && (uintptr_t)off % 4 == 0, BG_E_ALIGN,
               "bg_digest_group_keys: digest and key must be 16-byte aligned");
    const size_t lds = 32 * (size_t)(max_group > 0 ? max_group : 1);
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(bg::group_keys_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)(32 * (size_t)bg::HD_GROUP_MAX));
        BG_REQUIRE(e == hipSuccess, (int)e, "bg_digest_group_keys: %d bytes of LDS refused: %s", (int)lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(bg::group_keys_kernel, dim3(N), dim3(bg::WAVE), lds, (hipStream_t)stream, digest, off, max_group, key);
    return bg::launch_status("bg_digest_group_keys");
}

extern "C" int bg_first_occurrence(const uint8_t* key, long long N, int* table, long long T, uint8_t* keep, bg_stream_t stream) {
    BG_REQUIRE(N >= 0 && N <= 0x3fffffffLL, BG_E_SHAPE, "bg_first_occurrence: need 0 <= N <= 2^30 - 1 (N=%lld)", N);
    BG_REQUIRE(T >= 2 && (T & (T - 1)) == 0 && T >= 2 * N && T <= (1LL << 31), BG_E_SHAPE,
               "bg_first_occurrence: the table size must be a power of two, T >= 2 N and T >= 2 (N=%lld T=%lld)", N, T);
    if (N == 0) return 0;
    BG_REQUIRE(key && table && keep, BG_E_ARG, "bg_first_occurrence: null key, table or keep");
    BG_REQUIRE((uintptr_t)key % 16 == 0 && (uintptr_t)table % 4 == 0, BG_E_ALIGN, "bg_first_occurrence: key must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(table, 0xFF, (size_t)T * sizeof(int), s);          // every slot -1
    BG_REQUIRE(e == hipSuccess, (int)e, "bg_first_occurrence: clearing the table failed: %s", hipGetErrorString(e));
    const unsigned blocks = (unsigned)((N + bg::HD_THREADS - 1) / bg::HD_THREADS);
    const uint4* k = reinterpret_cast<const uint4*>(key);
    hipLaunchKernelGGL(bg::first_claim_kernel, dim3(blocks), dim3(bg::HD_THREADS), 0, s, k, N, table, (unsigned long long)(T - 1));
    hipLaunchKernelGGL(bg::first_keep_kernel, dim3(blocks), dim3(bg::HD_THREADS), 0, s, k, N, (const int*)table, (unsigned long long)(T - 1), keep);
    return bg::launch_status("bg_first_occurrence");
}
