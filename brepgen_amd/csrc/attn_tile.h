// The tile convention and the tile steps of the 16-bit attention kernels -- attn_train.hip (training forward, dQ, dK/dV, the one-launch
// short backward) and attn.hip -- each defined ONCE here, as gemm16.h does for the GEMMs: what makes two of these kernels give the
// same bits for the same work is that they run the same text.  Helpers take lane values (l31 = lane & 31, h = lane >> 5, tid) as
// parameters and never read threadIdx.  Included by attn.hip and attn_train.hip only.  (Which kernel keeps its own text of which
// step, and why, is listed below, before the backward helpers; qkv_attn_kernel and attn16_long_kernel are hand-scheduled and keep
// all of theirs.)
//
// THE TILE CONVENTION.  A score tile is one v_mfma_f32_32x32x16 accumulator: A = 32 rows of the WALKED side (fragments read from an
// LDS image), B = 32 rows of the OWNED side (fragments held in registers, one row per lane & 31).  Lane (l31, h) then holds, in
// accumulator register r of sub-tile `sub`, the element
//       owned row l31   x   walked row 32 sub + at_walked(r, h),      at_walked(r, h) = (r & 3) + 8 (r >> 2) + 4 h,
// i.e. registers 4 g .. 4 g + 3 are four CONSECUTIVE walked rows starting at at_walked(4 g, h) = 8 g + 4 h, and a row's 32 walked
// elements are split over lane and lane ^ 32.  Whatever belongs to the owned row (running max and sum, lse, delta) is lane-local.
// The fp32 tile is fed straight back as the B operand of the next product, which sums over the walked index: registers 8 sl .. 8 sl + 7
// are its k-slots, and the A operand is read from a transposed image in that same order (at_frag_tr).  The same map places an
// accumulator of a [d][owned row] product: register r of d tile dt <-> d = 32 dt + at_walked(r, h) (at_store_acc).
#pragma once
#include "gemm16.h"
#include <math.h>

namespace bg {

constexpr int QKV_LD = 3 * BG_D_MODEL;     // row stride of the packed qkv tensor: 2304
constexpr int TR_LD = 68;                  // row stride of a transposed tile image (16-bit elements): the 32 d-rows a half-wave reads
                                           // with ds_read_b64 fall on 32 distinct bank pairs
constexpr int AT_RM = 64 * 128;            // row-major tile image: 64 rows x 128 B, 16-byte chunks XOR-swizzled (gemm16.h)
constexpr int AT_TR = 64 * TR_LD * 2;      // transposed tile image [64 d][TR_LD]

__device__ __forceinline__ int at_walked(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ---- operands ----
// the four 16-wide d slices of a lane's own row (B operand of a score product): k-chunk h of each slice
template <bool F16> __device__ __forceinline__ void at_row_frags(const typename Elem<F16>::T* rowp, int h, typename Elem<F16>::V8 (&f)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) f[ks] = *reinterpret_cast<const typename Elem<F16>::V8*>(rowp + (ks * 2 + h) * 8);
}
// A fragment of a row-major image: tile row `row`, 16-byte chunk `chunk`
template <bool F16> __device__ __forceinline__ typename Elem<F16>::V8 at_frag_rm(const unsigned char* img, int row, int chunk) {
    return *reinterpret_cast<const typename Elem<F16>::V8*>(img + row * 128 + ((chunk ^ swz_term(row)) << 4));
}
// A fragment of a transposed image: column d, tile rows w0 .. w0 + 3 and w0 + GAP .. w0 + GAP + 3.  GAP = 8, w0 = 32 sub + 16 sl + 4 h:
// the order in which registers 8 sl .. 8 sl + 7 hold the walked index;  GAP = 4, w0 = 16 ks + 8 h: eight rows in natural order
template <bool F16, int GAP = 8> __device__ __forceinline__ typename Elem<F16>::V8 at_frag_tr(const typename Elem<F16>::T* tr, int d, int w0) {
    using V4 = typename Elem<F16>::V4;
    const typename Elem<F16>::T* p = tr + d * TR_LD + w0;
    const V4 lo = *reinterpret_cast<const V4*>(p);
    const V4 hi = *reinterpret_cast<const V4*>(p + GAP);
    typename Elem<F16>::V8 a;
    a[0] = lo[0]; a[1] = lo[1]; a[2] = lo[2]; a[3] = lo[3];
    a[4] = hi[0]; a[5] = hi[1]; a[6] = hi[2]; a[7] = hi[3];
    return a;
}

// ---- tile staging through registers ----
// 64 rows (tile row r = row min(r0 + r, N - 1) of the sample) x 64 elements of `src` by a workgroup of NT threads.
// RM: row-major image, chunk c of row r at chunk c ^ swz_term(r);  TR: transposed image tr[d][r]
template <bool F16, int NT, bool RM, bool TR>
__device__ __forceinline__ void at_stage(const typename Elem<F16>::T* __restrict__ src, int ld, int r0, int N, unsigned char* img,
                                         typename Elem<F16>::T* tr, int tid) {
    using V8 = typename Elem<F16>::V8;
#pragma unroll
    for (int j = 0; j < 512 / NT; ++j) {
        const int idx = j * NT + tid;
        const int row = idx >> 3, c = idx & 7;
        int g = r0 + row;
        g = g < N ? g : N - 1;
        const V8 v = *reinterpret_cast<const V8*>(src + (size_t)g * ld + c * 8);
        if (RM) *reinterpret_cast<V8*>(img + row * 128 + ((c ^ swz_term(row)) << 4)) = v;
        if (TR) {                                      // the transposing LDS write
#pragma unroll
            for (int e = 0; e < 8; ++e) tr[(c * 8 + e) * TR_LD + row] = v[e];
        }
    }
}

// ---- the steps that stay in the kernels ----
// Each of the following came out of hipcc as another instruction stream behind a helper (commuted operands, moved zero-fills, a
// re-associated prologue) in kernels that must not change, or that measured slower with it, so these kernels keep their own text:
//   online-softmax sub-tile, P V accumulate, store    attn16_kernel (attn.hip: also its K-fragment read and transposing write),
//                                                      at_fwd16_kernel
//   row fragments (x and y loads interleaved), backward element step, hi + lo split, store    at_bwd16_kernel
// The helpers below serve at_bwd16_short_kernel and, where it was neutral, the kernels above.

// ---- backward ----
// one element: P recomputed from lse, the keep bit applied to P (-> pv = P~) and to dP (dpv, in place);  returns P
template <bool DROP>
__device__ __forceinline__ float at_bwd_elem(float s, float scale, float lse, bool dead, bool kept, float rp, float& dpv, float& pv) {
    const float p = dead ? 0.f : __expf(s * scale - lse);
    pv = p;
    if (DROP) {
        dpv = kept ? dpv * rp : 0.f;
        pv = kept ? p * rp : 0.f;
    }
    return p;
}
// dS and P~ enter their products as hi + lo 16-bit pairs (two MFMAs on one A fragment): rounded once to 16 bits they carry an error
// of the size of the RESULT's own rounding -- measured 1.5 x torch's mean and up to 3.3 x its max error
template <typename T> __device__ __forceinline__ void at_hilo(float v, T& hi, T& lo) {
    hi = (T)v;
    lo = (T)(v - (float)hi);
}
template <bool F16>      // registers 8 sl .. 8 sl + 7 of a tile
__device__ __forceinline__ void at_split8(const f32x16& v, int sl, typename Elem<F16>::V8& hi, typename Elem<F16>::V8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        typename Elem<F16>::T a, b;
        at_hilo(v[8 * sl + e], a, b);
        hi[e] = a; lo[e] = b;
    }
}
template <bool F16>
__device__ __forceinline__ void at_mfma_hilo(f32x16& acc, typename Elem<F16>::V8 a, typename Elem<F16>::V8 hi, typename Elem<F16>::V8 lo) {
    acc = Elem<F16>::mfma(a, hi, acc);
    acc = Elem<F16>::mfma(a, lo, acc);
}

// ---- accumulator store: acc[dt] register r (x factor) -> rowp[32 dt + at_walked(r, h)], the lane's own row ----
template <bool F16> __device__ __forceinline__ void at_store_acc(typename Elem<F16>::T* rowp, const f32x16 (&acc)[2], float factor, int h) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
            *reinterpret_cast<typename Elem<F16>::V4*>(rowp + dt * 32 + at_walked(4 * g4, h)) =
                Elem<F16>::pack4(acc[dt][4 * g4 + 0] * factor, acc[dt][4 * g4 + 1] * factor, acc[dt][4 * g4 + 2] * factor,
                                 acc[dt][4 * g4 + 3] * factor);
}

// ---- fp32 kernels: a wave's LDS writes become visible to its own lanes (no block-level barrier: waves leave early) ----
__device__ __forceinline__ void at_wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

}  // namespace bg
