// Pieces shared by the 16-bit MFMA kernels -- gemm_16bit.hip (128 x 128 persistent + generic tiles), gemm_p256.hip (256 x 256
// persistent, 8-phase K loop), gemm_split.hip (pipelined split-residual epilogue), qkv_attn.hip (fused QKV + attention),
// ffn_fused.hip (FFN1 + FFN2 in one launch); attn.hip / attn_train.hip take the types and the swizzle through attn_tile.h.  These kernels produce the same bits for the same
// work (the tests assert it kernel against kernel), and what makes them do so is defined ONCE, in this file: the element types, the
// LDS-DMA instruction, the 16-byte XOR swizzle, the split-residual octet, the LayerNorm-fold row coefficients, the 128 x 128 tile
// walk and the accumulator-to-patch write.  Every helper is forceinline and takes lane / row values as parameters: several kernels
// derive them from an opaque thread id on purpose (register pressure), so none reads threadIdx itself.
#pragma once
#include "bg_common.h"
#include <type_traits>

namespace bg {

constexpr int SMALL_LAUNCH_TILES = 160;   // launches of fewer 128 x 128 tiles run on 64 x 64 tiles (gemm_16bit.hip launch16)
constexpr int G_BK = 64;            // 16-bit elements per K-step = 128 bytes per tile row

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

template <bool F16> struct Elem;
template <> struct Elem<false> {
    using T = __bf16; using V8 = bf16x8; using V4 = bf16x4;
    static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ V4 pack4(float a, float b, float c, float d) { return to_bf16x4(a, b, c, d); }
};
template <> struct Elem<true> {
    using T = _Float16; using V8 = f16x8; using V4 = f16x4;
    static __device__ __forceinline__ f32x16 mfma(V8 a, V8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ V4 pack4(float a, float b, float c, float d) {
        // the fp32 values are made opaque first: where they come straight out of an fma, hipcc would otherwise fuse fma + conversion
        // into v_fma_mixlo_f16 (ONE rounding) in some kernels and not in others, and the GEMM kernels would differ by an ulp in ~10 ppm
        // of the fp16 values (seen between the 256 x 256 and the 128 x 128 kernel once the build flags changed in round 6)
        asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
        V4 r; r[0] = (_Float16)a; r[1] = (_Float16)b; r[2] = (_Float16)c; r[3] = (_Float16)d; return r;
    }
};

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// epilogue selection of the persistent kernels (one instantiation each, so that none carries the registers of another):
//   P_PLAIN16  16-bit output, bias (+ReLU)                              -- QKV / FFN1 without the LayerNorm fold, VAE convs
//   P_FOLD16   same with the LayerNorm fold (stats_in / colsum)         -- QKV / FFN1 of the denoisers
//   P_GENERAL  fp32 or 16-bit output with fp32 addends (add / add2)     -- fp32 residual stream, embeds, VAE residuals
//   P_SPLIT    split (hi, lo) output, addend = split residual or fp32 broadcast rows, optional row statistics
//                                                                       -- token embeds of the denoisers (row maps, broadcast addends)
//                                                                          and the tests' baseline for out-proj / FFN2, which the
//                                                                          product path runs on gemm_split.hip / gemm_p256.hip
enum { P_PLAIN16 = 0, P_FOLD16 = 1, P_GENERAL = 2, P_SPLIT = 3 };
constexpr int FOLD_PARTS = 12;      // the persistent kernels' LayerNorm fold is compiled for K = 768 (LN width of the denoisers)

// ---- LDS-DMA: global -> LDS without passing through registers, 16 bytes per lane = 1 KiB per wave instruction ----
// builtin form: lane l's 16 bytes at `gsrc` (a per-lane address) land at lds_wave_base (wave-uniform) + 16 l
__device__ __forceinline__ void lds_dma16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}
// inline-asm form, hidden from hipcc's wait insertion (the kernels that use it count vmcnt by hand): source = wave-uniform base
// `src` (SGPR pair) + per-lane byte offset `voff`, destination = LDS byte address `dst_lds` (wave-uniform) + 16 l.  m0 carries the
// destination and is restored, so the compiler's own uses of m0 around the call stay valid.
// (attn.hip: dma16_asm is the same instruction with a per-lane 64-bit address and no base -- kept there, it has one user.)
__device__ __forceinline__ void lds_dma_piece(unsigned dst_lds, const unsigned char* src, unsigned voff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(src), "s"(dst_lds) : "memory");
}

// ---- the 16-byte XOR swizzle of an LDS operand image (rows of 128 B = eight 16-byte chunks) ----
// Chunk c of tile row r lives at chunk c ^ swz_term(r): every 16-lane service group of a ds_read_b128 fragment read then touches 16
// distinct 16-byte slots of the 256-byte bank row (measured: SQ_LDS_BANK_CONFLICT = 0).  The LDS-DMA writes lane-linear, so the
// permutation is applied to the per-lane SOURCE address (dma_src_chunk) and once more by the fragment reads (frag_chunk_offsets):
// the same involution on both sides, the image a kernel reads is the operand itself.
__device__ __forceinline__ int swz_term(int row) { return (row >> 1) & 7; }
// DMA source side: lane (8 rows x 8 chunks per piece, chunk = lane & 7) fetches this 16-byte chunk of tile row `row`
__device__ __forceinline__ int dma_src_chunk(int lane, int row) { return (lane & 7) ^ swz_term(row); }
// fragment-read side: byte offsets inside the row of the lane's chunk (2 ks + hq) of the four 16-wide k-slices; l31 = lane & 31 is
// the fragment row inside its 32-row MFMA tile (tiles start at multiples of 32 rows: the term depends on l31 only), hq = lane >> 5.
// (gemm_p256.hip and qkv_attn.hip write this loop out themselves, on swz_term: DESIGN.md section 4, "where the compiler refused".)
__device__ __forceinline__ void frag_chunk_offsets(int l31, int hq, unsigned (&xk)[4]) {
    const int sw = swz_term(l31);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) xk[ks] = (unsigned)(((ks * 2 + hq) ^ sw) << 4);
}

// ---- split-residual octet: 8 consecutive columns of one output row, v = acc + bias already in `v` ----
// v += hi + lo of the residual planes (16 bytes each: the octet's 8 x 16 bit)
template <bool F16> __device__ __forceinline__ void octet_add_residual(float (&v)[8], uint4 hi, uint4 lo) {
    float fh[4], fl[4];
    unpack4_16<F16>(make_uint2(hi.x, hi.y), fh);
    unpack4_16<F16>(make_uint2(lo.x, lo.y), fl);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += fh[e] + fl[e];
    unpack4_16<F16>(make_uint2(hi.z, hi.w), fh);
    unpack4_16<F16>(make_uint2(lo.z, lo.w), fl);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 + e] += fh[e] + fl[e];
}
// (sum, sum of squares) of the octet.  THE association order of the row statistics: 4-column chunk partials, pairs first, then the
// two chunks -- and from there a butterfly over the lanes that share the row (group8_sum here; the generic kernel, gemm16_kernel,
// holds one 4-column chunk per lane and continues with group16_sum, whose first three steps are group8_sum's).
__device__ __forceinline__ float2 octet_stats(const float (&v)[8]) {
    const float s8 = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    const float q8 = ((v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])) + ((v[4] * v[4] + v[5] * v[5]) + (v[6] * v[6] + v[7] * v[7]));
    return make_float2(s8, q8);
}
// v -> the octet's 16 bytes of the hi plane and of the lo plane
template <bool F16> __device__ __forceinline__ void octet_split(const float (&v)[8], uint4& hi, uint4& lo) {
    const float va[4] = {v[0], v[1], v[2], v[3]}, vb[4] = {v[4], v[5], v[6], v[7]};
    uint2 ha, la, hb, lb;
    split4_16<F16>(va, ha, la);
    split4_16<F16>(vb, hb, lb);
    hi = make_uint4(ha.x, ha.y, hb.x, hb.y);
    lo = make_uint4(la.x, la.y, lb.x, lb.y);
}

// ---- LayerNorm fold: a row's coefficients from the FOLD_PARTS (sum, sum of squares) partials its producer left behind ----
// pair_at(part) -> float2 fetches one partial from wherever the kernel keeps them (registers, LDS, global memory); the sixteen
// zero-padded pairs are summed in tree16's order (bg_common.h), the order of the generic kernel's 16-lane butterfly.
template <typename PairAt> __device__ __forceinline__ float2 fold_row_sums(PairAt&& pair_at) {
    float ps[16], pq[16];
#pragma unroll
    for (int pp = 0; pp < 16; ++pp) {
        const float2 v = pp < FOLD_PARTS ? pair_at(pp) : make_float2(0.f, 0.f);
        ps[pp] = v.x; pq[pp] = v.y;
    }
    return make_float2(tree16(ps), tree16(pq));
}
// (rstd, -mean * rstd) of the row over its K columns.  (K and eps by reference: a kernel argument passed here is then read where
// ln_fold_coeffs uses it, behind the partials, as in the kernels' own code before this helper existed -- the register allocation of
// the kernels at the 256-VGPR limit depends on that order.)
template <typename PairAt> __device__ __forceinline__ float2 fold_row_coeffs(PairAt&& pair_at, const int& K, const float& eps) {
    const float2 s = fold_row_sums(pair_at);
    return ln_fold_coeffs(s.x, s.y, K, eps);
}

// ---- tile walk of the persistent 128 x 128 kernels (gemm_16bit.hip, gemm_split.hip) ----
// XCD-aware (block b runs on XCD b % 8; each XCD has a private 4 MiB L2): XCD x owns the row panels x, x + 8, ...; its G / 8
// workgroups walk that sub-grid column-fastest, so the ~64 concurrently running tiles of an XCD share a few A row panels and keep W
// resident.  (Column groups per XCD, a row-major walk and adjacent-column pairing of the two workgroups of a CU were measured in
// rounds 1-2 and are flat or slower: DESIGN.md section 4.)  Hybrid launches: the 256 x 256 kernel owns the row panels below p0
// (bg_common.h p256_rows; both kernels read the same answer).  The workgroup's tiles are t = w_local, w_local + cnt, ...
struct PanelWalk128 {
    int p0, m_panels, nt_n, xcd, w_local, cnt;
    // m_panels: row panels present, nt_n: column tiles; G = grid size, a multiple of 8 (launcher)
    __device__ __forceinline__ PanelWalk128(const GemmArgs& g, int m_panels_, int nt_n_, unsigned block, int G)
        : p0(g.hybrid ? (g.rows256_dev ? *g.rows256_dev : g.rows256_host) >> 7 : 0), m_panels(m_panels_), nt_n(nt_n_),
          xcd(block & 7), w_local(block >> 3), cnt(G >> 3) {}
    // origin of the workgroup's tile t; false: past the end
    __device__ __forceinline__ bool tile_at(int t, int& tm0, int& tn0) const {
        const int panel = p0 + xcd + (t / nt_n) * 8;
        tm0 = panel << 7;
        tn0 = (t % nt_n) << 7;
        return panel < m_panels;
    }
};

// ---- transposed product (weights as the MFMA's A operand: a lane owns one output row, four consecutive columns per accumulator
// quad): 16 rows x 64 fp32 columns of one row tile -> the wave's patch.  Patch rows of 256 B, 16-byte chunk XOR-swizzled by the
// row (ds_write_b128 here and the octets' ds_read_b128 on the way back are conflict-free).  The lanes with (l31 >> 4) == half
// own the 16 rows. ----
__device__ __forceinline__ void slab_to_patch(unsigned char* patch, int l31, int hq, int half, const f32x16 (&p)[2]) {
    if ((l31 >> 4) == half) {
        const int prow = l31 & 15;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c16 = j * 8 + 2 * q + hq;
                *reinterpret_cast<float4*>(patch + prow * 256 + ((c16 ^ prow) << 4)) =
                    make_float4(p[j][4 * q], p[j][4 * q + 1], p[j][4 * q + 2], p[j][4 * q + 3]);
            }
    }
}

// 256 x 256 persistent kernel (gemm_p256.hip).  p256_eligible: shape / argument checks only -- the caller decides whether the
// tile count makes it the faster choice.
bool p256_eligible(const GemmArgs& g);
template <bool F16> int launch_p256(const GemmArgs& g, hipStream_t s);

// software-pipelined split-residual kernel (gemm_split.hip): out-proj / FFN2 of the encoder layers
bool split_pipe_eligible(const GemmArgs& g);
template <bool F16> int launch_split_pipe(const GemmArgs& g, hipStream_t s);

}  // namespace bg
