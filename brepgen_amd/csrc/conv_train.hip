// The backward of a VAE ResnetBlock2D's convolution layer, y = conv(act(GroupNorm(x))) + b (stride 1, 'same' zero padding, odd window):
//   bg_conv_wgrad        dw[n, tap, c] = sum_{s,y,x} dy[s,y,x,n] a[s, y + ky - kh/2, x + kx - kw/2, c]  and  db[n] = sum dy[., n]
//   bg_conv_weight_pack  the nn.Conv weight [N, C, kh, kw] -> the forward pack [N, kh*kw*C] and / or the data-gradient pack
//                        [C, kh*kw*N] with the taps reversed, 16-bit, one launch
//   bg_gn_act_bwd        the backward of a = act(GroupNorm(x)): dx (+ dskip), dgamma, dbeta
// The data gradient needs no kernel of its own: a 'same' forward convolution of dy with the reversed-tap pack is it, so it runs on
// bg_conv_gemm_fwd / bg_im2col + bg_gemm_bias_act_fwd as the forward does.
// And of the two resampling convolutions between the blocks (Downsample2D: pad after + stride 2; Upsample2D: nearest x2 + 'same'):
//   bg_conv_wgrad_geom        bg_conv_wgrad with the geometry of the loader as a template parameter of the same kernel
//   bg_conv_weight_pack_down  the forward pack and / or the class-ordered pack of the stride-2 data gradient
//   bg_conv_down_dgrad        dx of the stride-2 convolution by the parity of the input pixel: gather, four GEMMs, interleave
//   bg_pool2x2_sum            the 2 x 2 sum that turns the stride-1 data gradient on the 2H x 2W grid into Upsample2D's dx
//
// Weight gradient (cw_wgrad_kernel).  This is lb_wgrad_kernel's organisation (linear_bwd.hip): a workgroup of four waves owns one
// 128 x 128 tile of dw [N, K = kh*kw*C] and one contiguous slice of the M = S*H*W output pixels, walked in steps of 32 rows through
// two row-major LDS images read by the hardware transpose read, one barrier per step, the bias gradient from the staged dY values,
// slices combined through an fp32 workspace by lb_reduce_kernel.  The one difference is the second operand's loader.  With
// C % 128 == 0 a 128-column K tile lies inside ONE tap (ky, kx), so the row the loader stages for output pixel m = (s, y, x) is the
// activation pixel (s, y + ky - kh/2, x + kx - kw/2): row m + (ky - kh/2) W + (kx - kw/2) of `a`, or zeros -- filled in registers,
// never read -- when the shifted pixel leaves the H x W grid of sample s.  A shifted row therefore never comes from a neighbouring
// sample, and the kh*kw-fold im2col matrix is never written.  lb_wgrad_kernel keeps its own copy of the tile body: hoisting it into
// the helpers of wgrad_tile.h changed that kernel's register allocation and schedule, and its instruction stream is what round 14
// measured.
//
// GroupNorm + activation backward.  With xh = (x - mean) rstd, v = gamma xh + beta, dv = da act'(v):
//     dgamma[c] = sum_{s,p} dv xh,   dbeta[c] = sum_{s,p} dv,
//     dx = rstd (dv gamma - m1 - xh m2) [+ dskip],   m1 = mean_group(dv gamma),  m2 = mean_group(dv gamma xh)
// (the means over the P positions x C/G channels of the element's (sample, group)); xh is formed with the statistics' mean corrected
// by its fp64-measured error (gb_finish_kernel).  Pass 1 (gb_sums_kernel) writes the per-(sample,
// channel) sums of dv and dv xh over chunks of 64 positions, in fp64.
// gb_finish_kernel adds the chunks in fp64 in index order and forms m1 / m2 per (sample, group); gb_param_kernel adds the samples
// in fp64 into dgamma / dbeta; pass 2 (gb_dx_kernel) recomputes dv and writes dx.  16-byte accesses throughout.
#include "wgrad_tile.h"
#include <math.h>

namespace bg {

// ---------------------------------------------------------------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------------------------------------------------------------
// OUT: 0 = fp32 partial tile to the workspace (split > 1), 1 = dw / db in fp32, 2 = dw / db in the operand dtype
// GEOM (bg_conv_geom): which pixel of `a` the tap of this K tile reads for output pixel m = (s, y, x) of dy's 2^lh x 2^lw grid.
//   0  'same', stride 1: (y + ky - kh/2, x + kx - kw/2) on dy's own grid -- the body round 18 wrote, untouched
//   1  DOWN2: (2y + ky, 2x + kx) on the 2^(lh+1) x 2^(lw+1) grid of `a` (padding AFTER the grid only)
//   2  UP2:   (uy >> 1, ux >> 1) on the 2^(lh-1) x 2^(lw-1) grid of `a`, uy = y + ky - 1, ux = x + kx - 1, tested against dy's grid
//             BEFORE the shift (-1 >> 1 is -1)
// In every geometry a row that leaves the sample's grid stays the zeros it was initialised with: nothing is read for it.
template <bool F16, int OUT, int GEOM = 0>
__global__ __launch_bounds__(256, 2) void cw_wgrad_kernel(const void* __restrict__ dy_, int ld_dy, const void* __restrict__ a_, int ld_a,
                                                          void* __restrict__ dw_, void* __restrict__ db_, int M, int N, int C, int kh,
                                                          int kw, int lh, int lw, int slice_rows) {
    using T = typename Elem<F16>::T;
    __shared__ __attribute__((aligned(16))) unsigned char lds[4 * LB_IMG];      // [stage][dY image | activation image]
    const T* __restrict__ dy = reinterpret_cast<const T*>(dy_);
    const T* __restrict__ a = reinterpret_cast<const T*>(a_);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave >> 1, wk = wave & 1;
    // lb_wgrad_kernel's XCD-aware walk: K tile fastest, then N tile, then slice; the K tiles of a tap share a dY piece AND (shifted by
    // less than a grid row or two) the activation rows, so the whole run of an XCD works out of one L2
    const int lid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int K = kh * kw * C;
    const int kt_n = K >> 7, nt_n = N >> 7;
    const int kt = lid % kt_n, nt = (lid / kt_n) % nt_n, slice = lid / (kt_n * nt_n);
    const int k0 = kt * 128, n0 = nt * 128;
    const int m_begin = slice * slice_rows;              // (a forced split beyond the row steps: trailing slices are empty, zero partials)
    const int m_end = min(M, m_begin + slice_rows);
    const int nsteps = m_end > m_begin ? (m_end - m_begin + LB_RS - 1) / LB_RS : 0;
    const bool with_db = db_ != nullptr && kt == 0;

    // the tap of this K tile (C % 128 == 0: one tap per tile) and its shift on the H x W grid
    const int tap = k0 / C, c0 = k0 - tap * C;
    const int oy = tap / kw - (kh >> 1), ox = tap % kw - (kw >> 1);
    const int H = 1 << lh, W = 1 << lw;
    const int shift = oy * W + ox;                      // rows of `a` between an output pixel and the pixel the tap reads

    // ---- staging: thread = (16-byte chunk sc, rows sr and sr + 16) of both 32 x 128 pieces ----
    const int sc = tid & 15, sr = tid >> 4;
    const T* dyp = dy + n0 + sc * 8;
    const T* ap = a + c0 + sc * 8;
    const unsigned st_off = lb_off(sr, sc);            // row sr + 16 has the same swizzle term: + 16 * 256 bytes
    uint4 rdy[2], ra[2];
    float dbacc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) dbacc[e] = 0.f;
    auto fetch = [&](int it) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m_begin + it * LB_RS + sr + 16 * j;
            rdy[j] = make_uint4(0u, 0u, 0u, 0u);
            ra[j] = make_uint4(0u, 0u, 0u, 0u);
            if (m < m_end) {
                rdy[j] = *reinterpret_cast<const uint4*>(dyp + (size_t)m * ld_dy);
                const int x = m & (W - 1), y = (m >> lw) & (H - 1);
                if (GEOM == 0) {
                    // inside the sample's own grid: row m + shift is then a pixel of the same sample, 0 <= m + shift < M
                    if ((unsigned)(y + oy) < (unsigned)H && (unsigned)(x + ox) < (unsigned)W)
                        ra[j] = *reinterpret_cast<const uint4*>(ap + (size_t)(m + shift) * ld_a);
                } else if (GEOM == 1) {
                    // ky = oy + 1, kx = ox + 1; m >> lw = s * H + y, so 2 (m >> lw) + ky is the row of a's [S * 2H, 2W] pixel grid
                    const int ay = 2 * y + oy + 1, ax = 2 * x + ox + 1;
                    if (ay < 2 * H && ax < 2 * W)
                        ra[j] = *reinterpret_cast<const uint4*>(ap + ((size_t)(2 * (m >> lw) + oy + 1) * (2 * W) + ax) * ld_a);
                } else {
                    const int uy = y + oy, ux = x + ox;
                    if ((unsigned)uy < (unsigned)H && (unsigned)ux < (unsigned)W)
                        ra[j] = *reinterpret_cast<const uint4*>(ap + ((size_t)((m >> (lw + lh)) * (H >> 1) + (uy >> 1)) * (W >> 1) + (ux >> 1)) * ld_a);
                }
            }
        }
    };
    auto stash = [&](int st) {
        unsigned char* img = lds + st * 2 * LB_IMG + st_off;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            *reinterpret_cast<uint4*>(img + j * 16 * 256) = rdy[j];
            *reinterpret_cast<uint4*>(img + LB_IMG + j * 16 * 256) = ra[j];
        }
        if (with_db) {
            lb_add8<F16>(dbacc, rdy[0]);
            lb_add8<F16>(dbacc, rdy[1]);
        }
    };

    unsigned a_off[2][2], b_off[2][2];
    lb_frag_offsets(lane, wn, wk, a_off, b_off);
    f32x16 acc[2][2];
    lb_zero(acc);

    if (nsteps > 0) {
        fetch(0);
        stash(0);
    }
    for (int it = 0; it < nsteps; ++it) {
        const int st = it & 1;
        const bool more = it + 1 < nsteps;
        if (more) fetch(it + 1);
        __syncthreads();                                  // stage st is written; everybody is done reading stage st ^ 1
        lb_step<F16>(lds + st * 2 * LB_IMG, a_off, b_off, acc);
        if (more) stash(st ^ 1);
    }

    lb_store_tile<F16, OUT>(acc, dw_, OUT == 0 ? (size_t)slice * N * K : 0, K, n0 + 64 * wn, k0 + 64 * wk, lane);
    if (with_db) lb_store_db<F16, OUT>(dbacc, lds, db_, (OUT == 0 ? (size_t)slice * N : 0) + n0, tid);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight pack: a workgroup takes a 32 (n) x 32 (c) x kh*kw block of the weight through LDS.  The source block is 32 runs of
// 32 * kh*kw consecutive elements; both outputs leave in 16-byte pieces (64-byte runs).
// MODE: 0 = 16-bit source (bits copied), 1 = fp32 -> bf16, 2 = fp32 -> fp16
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int CP_MAX_TAPS = 25;
template <int MODE>
__global__ __launch_bounds__(256) void cw_pack_kernel(const void* __restrict__ src_, void* __restrict__ fwd_, void* __restrict__ dgrad_,
                                                      int N, int C, int T) {
    __shared__ __attribute__((aligned(16))) unsigned short tile[32 * 32 * CP_MAX_TAPS];      // [n][c][t], as in the source
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int run = 32 * T;                               // consecutive source elements per n
    for (int i = tid; i < 32 * run; i += 256) {
        const int n = i / run, r = i - n * run;
        const size_t at = ((size_t)(n0 + n) * C + c0) * T + r;
        unsigned short v;
        if (MODE == 0) v = reinterpret_cast<const unsigned short*>(src_)[at];
        else if (MODE == 1) { union { __bf16 b; unsigned short u; } c; c.b = (__bf16)reinterpret_cast<const float*>(src_)[at]; v = c.u; }
        else { union { _Float16 h; unsigned short u; } c; c.h = cvt16<_Float16>(reinterpret_cast<const float*>(src_)[at]); v = c.u; }
        tile[i] = v;
    }
    __syncthreads();
    // item = (row of the 32 x T output block, 8-element piece q of its 32 columns)
    for (int i = tid; i < 32 * T * 4; i += 256) {
        const int q = i & 3, t = (i >> 2) % T, r = (i >> 2) / T;
        if (fwd_) {                                        // fwd[n0 + r][t][c0 + 8 q ..]
            unsigned short e[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) e[k] = tile[(r * 32 + 8 * q + k) * T + t];
            uint4 v;
            v.x = e[0] | ((unsigned)e[1] << 16); v.y = e[2] | ((unsigned)e[3] << 16);
            v.z = e[4] | ((unsigned)e[5] << 16); v.w = e[6] | ((unsigned)e[7] << 16);
            *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(fwd_) + ((size_t)(n0 + r) * T + t) * C + c0 + 8 * q) = v;
        }
        if (dgrad_) {                                      // dgrad[c0 + r][T - 1 - t][n0 + 8 q ..]
            unsigned short e[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) e[k] = tile[((8 * q + k) * 32 + r) * T + t];
            uint4 v;
            v.x = e[0] | ((unsigned)e[1] << 16); v.y = e[2] | ((unsigned)e[3] << 16);
            v.z = e[4] | ((unsigned)e[5] << 16); v.w = e[6] | ((unsigned)e[7] << 16);
            *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(dgrad_) + ((size_t)(c0 + r) * T + (T - 1 - t)) * N + n0 + 8 * q) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Downsample2D's data gradient and Upsample2D's pooling (see the header for the formulas)
//
// dx of the stride-2 convolution splits by the parity of the input pixel (iy, ix) = (2j + py, 2i + px) into four classes that take
// 1, 2, 2 and 4 of the nine taps: odd coordinates meet tap 1 at dy pixel j, even ones tap 0 at j and tap 2 at j - 1.  Each class is
// a plain GEMM of M = S*Ho*Wo rows: its operand row holds dy[j, i] and the one or three neighbours at j - 1 / i - 1 (zeros at the
// sample's first row / column, by an index test), its weight is the class's block of the class-ordered pack.  9 tap-products per four
// input pixels: the forward's work.  cd_gather_kernel writes the three multi-tap operands (class 0's is dy itself), four launches of
// bg_gemm_bias_act_fwd fill a class-major fp32 buffer [4][M][C], cd_interleave_kernel moves it to channels-last dx: every element
// of dx is written once, by that pass.
// ---------------------------------------------------------------------------------------------------------------------------------
// slot -> tap (ky * 3 + kx) of the class-ordered pack: (1,1) | (1,0) (1,2) | (0,1) (2,1) | (0,0) (0,2) (2,0) (2,2)
__device__ __constant__ int CD_SLOT_TAP[9] = {4, 3, 5, 1, 7, 0, 2, 6, 8};

// cw_pack_kernel's 32 x 32 x 9 block through LDS; outputs: the forward pack and / or the four class blocks [C, T_k * N] laid one after
// the other (T_k = 1, 2, 2, 4; block k starts at element C * N * {0, 1, 3, 5})
template <int MODE>
__global__ __launch_bounds__(256) void cd_pack_kernel(const void* __restrict__ src_, void* __restrict__ fwd_, void* __restrict__ down_, int N,
                                                      int C) {
    constexpr int T = 9;
    __shared__ __attribute__((aligned(16))) unsigned short tile[32 * 32 * T];      // [n][c][t], as in the source
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    constexpr int run = 32 * T;
    for (int i = tid; i < 32 * run; i += 256) {
        const int n = i / run, r = i - n * run;
        const size_t at = ((size_t)(n0 + n) * C + c0) * T + r;
        unsigned short v;
        if (MODE == 0) v = reinterpret_cast<const unsigned short*>(src_)[at];
        else if (MODE == 1) { union { __bf16 b; unsigned short u; } c; c.b = (__bf16)reinterpret_cast<const float*>(src_)[at]; v = c.u; }
        else { union { _Float16 h; unsigned short u; } c; c.h = cvt16<_Float16>(reinterpret_cast<const float*>(src_)[at]); v = c.u; }
        tile[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < 32 * T * 4; i += 256) {
        const int q = i & 3, t = (i >> 2) % T, r = (i >> 2) / T;
        if (fwd_) {                                        // fwd[n0 + r][t][c0 + 8 q ..]
            unsigned short e[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) e[k] = tile[(r * 32 + 8 * q + k) * T + t];
            uint4 v;
            v.x = e[0] | ((unsigned)e[1] << 16); v.y = e[2] | ((unsigned)e[3] << 16);
            v.z = e[4] | ((unsigned)e[5] << 16); v.w = e[6] | ((unsigned)e[7] << 16);
            *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(fwd_) + ((size_t)(n0 + r) * T + t) * C + c0 + 8 * q) = v;
        }
        if (down_) {                                       // t is the SLOT here: block k, tap slot - first slot of k
            const int tap = CD_SLOT_TAP[t];
            const int first = t == 0 ? 0 : t < 3 ? 1 : t < 5 ? 3 : 5, tk = t == 0 ? 1 : t < 5 ? 2 : 4;
            unsigned short e[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) e[k] = tile[((8 * q + k) * 32 + r) * T + tap];
            uint4 v;
            v.x = e[0] | ((unsigned)e[1] << 16); v.y = e[2] | ((unsigned)e[3] << 16);
            v.z = e[4] | ((unsigned)e[5] << 16); v.w = e[6] | ((unsigned)e[7] << 16);
            *reinterpret_cast<uint4*>(reinterpret_cast<unsigned short*>(down_) + (size_t)first * C * N +
                                      ((size_t)(c0 + r) * tk + (t - first)) * N + n0 + 8 * q) = v;
        }
    }
}

// item = (dy pixel m, 16-byte piece q of its N channels): a1[m] = [d(j,i) | d(j,i-1)], a2[m] = [d(j,i) | d(j-1,i)],
// a3[m] = [d(j,i) | d(j,i-1) | d(j-1,i) | d(j-1,i-1)], a neighbour outside the sample's Ho x Wo grid being zeros
__global__ __launch_bounds__(256) void cd_gather_kernel(const unsigned short* __restrict__ dy, int ld_dy, unsigned short* __restrict__ a1,
                                                        unsigned short* __restrict__ a2, unsigned short* __restrict__ a3, size_t items,
                                                        int N, int lho, int lwo) {
    const int n8 = N >> 3, Wo = 1 << lwo, Ho = 1 << lho;
    for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
        const size_t m = it / n8;
        const int q = (int)(it - m * n8);
        const int i = (int)(m & (Wo - 1)), j = (int)((m >> lwo) & (Ho - 1));
        const unsigned short* p = dy + m * ld_dy + 8 * q;
        const uint4 d00 = *reinterpret_cast<const uint4*>(p);
        uint4 d01 = make_uint4(0u, 0u, 0u, 0u), d10 = d01, d11 = d01;
        if (i >= 1) d01 = *reinterpret_cast<const uint4*>(p - (size_t)ld_dy);
        if (j >= 1) d10 = *reinterpret_cast<const uint4*>(p - (size_t)Wo * ld_dy);
        if (i >= 1 && j >= 1) d11 = *reinterpret_cast<const uint4*>(p - (size_t)(Wo + 1) * ld_dy);
        uint4* o1 = reinterpret_cast<uint4*>(a1 + m * 2 * N + 8 * q);
        uint4* o2 = reinterpret_cast<uint4*>(a2 + m * 2 * N + 8 * q);
        uint4* o3 = reinterpret_cast<uint4*>(a3 + m * 4 * N + 8 * q);
        o1[0] = d00; o1[n8] = d01;
        o2[0] = d00; o2[n8] = d10;
        o3[0] = d00; o3[n8] = d01; o3[2 * n8] = d10; o3[3 * n8] = d11;
    }
}

// item = 4 channels of dx pixel (s, iy, ix): class 0 (odd, odd), 1 (odd iy, even ix), 2 (even iy, odd ix), 3 (even, even); row
// (s, iy >> 1, ix >> 1) of that class's [M, C] block
__global__ __launch_bounds__(256) void cd_interleave_kernel(const float4* __restrict__ cls, float4* __restrict__ dx, size_t items, size_t M,
                                                            int C, int lh, int lw) {
    const int c4n = C >> 2, W = 1 << lw, H = 1 << lh;
    for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
        const size_t pix = it / c4n;
        const int c4 = (int)(it - pix * c4n);
        const int ix = (int)(pix & (W - 1)), iy = (int)((pix >> lw) & (H - 1));
        const size_t s = pix >> (lw + lh);
        const int k = (iy & 1) ? ((ix & 1) ? 0 : 1) : ((ix & 1) ? 2 : 3);
        const size_t m = (((s << (lh - 1)) + (iy >> 1)) << (lw - 1)) + (ix >> 1);
        dx[it] = cls[(k * M + m) * c4n + c4];
    }
}

// item = 4 channels of y pixel (s, Y, X): (u[2Y, 2X] + u[2Y, 2X+1]) + (u[2Y+1, 2X] + u[2Y+1, 2X+1]) (+ add), u [S, 2H, 2W, C]
__global__ __launch_bounds__(256) void pool2x2_sum_kernel(const float4* __restrict__ u, const float4* __restrict__ add, float4* __restrict__ y,
                                                          size_t items, int H, int W, int C) {
    const int c4n = C >> 2;
    for (size_t it = (size_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (size_t)gridDim.x * 256) {
        const size_t pix = it / c4n;
        const int c4 = (int)(it - pix * c4n);
        const size_t X = pix % W, sy = pix / W;               // sy = s * H + Y: row 2 sy of u's [S * 2H, 2W] pixel grid
        const float4* p = u + ((2 * sy) * (2 * (size_t)W) + 2 * X) * c4n + c4;
        const float4 a = p[0], b = p[c4n], c = p[2 * (size_t)W * c4n], d = p[(2 * (size_t)W + 1) * c4n];
        float4 o;
        o.x = (a.x + b.x) + (c.x + d.x); o.y = (a.y + b.y) + (c.y + d.y);
        o.z = (a.z + b.z) + (c.z + d.z); o.w = (a.w + b.w) + (c.w + d.w);
        if (add) {
            const float4 r = add[it];
            o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        y[it] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// GroupNorm + activation backward
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int GB_CHUNK = 64;             // positions per chunk (one workgroup)

// act'(v): the derivative of what bg_im2col's act_apply computes (vae.hip)
template <int ACT> __device__ __forceinline__ float gb_dact(float v) {
    if (ACT == 1) {
        const float sg = 1.0f / (1.0f + __expf(-v));
        return sg * (1.0f + v * (1.0f - sg));
    }
    if (ACT == 2) return 0.5f * (1.0f + erff(v * 0.70710678118654752f)) + v * (0.39894228040143268f * __expf(-0.5f * v * v));
    return 1.0f;
}

// (mean, rstd) of the four channels 4 j .. 4 j + 3 of sample s
__device__ __forceinline__ void gb_stats4(const float* __restrict__ stats, int s, int G, int cpg, int j, float (&mean)[4], float (&rstd)[4]) {
    if ((cpg & 3) == 0) {
        const float2 st = *reinterpret_cast<const float2*>(stats + ((size_t)s * G + (4 * j) / cpg) * 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) { mean[e] = st.x; rstd[e] = st.y; }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float2 st = *reinterpret_cast<const float2*>(stats + ((size_t)s * G + (4 * j + e) / cpg) * 2);
            mean[e] = st.x; rstd[e] = st.y;
        }
    }
}

// xc = x - mean, xh = (xc - delta) * rstd and dv of four channels of one position.  delta: the statistics' mean error (below); 0 in pass 1
template <int ACT>
__device__ __forceinline__ void gb_elem4(float4 x, float4 da, const float (&mean)[4], const float (&rstd)[4], const float (&delta)[4], float4 ga,
                                         float4 be, float (&xc)[4], float (&xh)[4], float (&dv)[4]) {
    const float xs[4] = {x.x, x.y, x.z, x.w}, ds[4] = {da.x, da.y, da.z, da.w};
    const float gs[4] = {ga.x, ga.y, ga.z, ga.w}, bs[4] = {be.x, be.y, be.z, be.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        xc[e] = xs[e] - mean[e];
        xh[e] = (xc[e] - delta[e]) * rstd[e];
        dv[e] = ds[e] * gb_dact<ACT>(xh[e] * gs[e] + bs[e]);
    }
}

// pass 1: part[s][chunk][0][c] = sum_p dv, [1][c] = sum_p dv xh, [2][c] = sum_p (x - mean) over the chunk's positions.  grid (chunks, S).
// Thread (r, j) of R = max(1, 256 / (C / 4)) position rows x C / 4 column quads adds positions p0 + r, p0 + r + R, ... of the chunk, then
// the R chains of a column are added in order of r.  Sums and products are fp64 from the first term (dv and xh are fp32 values): with
// fp32 chains of 32 positions the dgamma of [2, 64, 512] missed the tests' 2 x torch yardstick (7.3e-6 against 2 x 3.4e-6), and the pass
// stays bound by its two fp32 streams.
template <int ACT>
__global__ __launch_bounds__(256) void gb_sums_kernel(const float* __restrict__ da, const float* __restrict__ x, const float* __restrict__ stats,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, double* __restrict__ part,
                                                      int P, int C, int G) {
    __shared__ double red[256 * 12];
    const int tid = threadIdx.x, chunk = blockIdx.x, s = blockIdx.y, nchunk = gridDim.x;
    const int c4n = C >> 2, cpg = C / G;
    const int R = c4n >= 256 ? 1 : 256 / c4n;
    const int r = c4n >= 256 ? 0 : tid / c4n;
    const int p0 = chunk * GB_CHUNK, p1 = min(P, p0 + GB_CHUNK);
    const size_t base = (size_t)s * P * C;
    double* out = part + ((size_t)s * nchunk + chunk) * 3 * C;
    const bool active = r < R;
    for (int j = c4n >= 256 ? tid : tid - r * c4n; active && j < c4n; j += 256) {
        float mean[4], rstd[4];
        gb_stats4(stats, s, G, cpg, j, mean, rstd);
        const float4 ga = *reinterpret_cast<const float4*>(gamma + 4 * j);
        const float4 be = *reinterpret_cast<const float4*>(beta + 4 * j);
        const float zero[4] = {0.f, 0.f, 0.f, 0.f};
        double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0}, s3[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p = p0 + r; p < p1; p += R) {
            const size_t at = base + (size_t)p * C + 4 * j;
            float xc[4], xh[4], dv[4];
            gb_elem4<ACT>(*reinterpret_cast<const float4*>(x + at), *reinterpret_cast<const float4*>(da + at), mean, rstd, zero, ga, be, xc, xh, dv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)dv[e];
                s1[e] += d;
                s2[e] = fma(d, (double)xh[e], s2[e]);     // the product of two fp32 values is exact in fp64
                s3[e] += (double)xc[e];
            }
        }
        if (R == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                out[4 * j + e] = s1[e];
                out[C + 4 * j + e] = s2[e];
                out[2 * C + 4 * j + e] = s3[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                red[tid * 12 + e] = s1[e];
                red[tid * 12 + 4 + e] = s2[e];
                red[tid * 12 + 8 + e] = s3[e];
            }
        }
    }
    if (R > 1) {                                          // (uniform over the workgroup)
        __syncthreads();
        if (tid < c4n) {
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                double v = red[tid * 12 + e];
                for (int q = 1; q < R; ++q) v += red[(q * c4n + tid) * 12 + e];
                out[(e >> 2) * C + 4 * tid + (e & 3)] = v;
            }
        }
    }
}

// sums[s][0 | 1 | 2][c] = the chunks of part in index order (fp64); means[s][g] = (m1, m2, delta, 0).  One workgroup per sample.
// delta = mean_group(x - mean): what the fp32 statistics' mean is off by (a few ulp of |mean|: with |mean| = 50 std that is 1e-5 std, more
// than everything else in this backward together).  Pass 1 ran without it, so its second sum is corrected here to first order,
// sum dv xh_true = sum dv xh - delta rstd sum dv; pass 2 subtracts delta itself.
__global__ __launch_bounds__(256) void gb_finish_kernel(const double* __restrict__ part, const float* __restrict__ stats,
                                                        const float* __restrict__ gamma, double* __restrict__ sums, float* __restrict__ means,
                                                        int nchunk, int P, int C, int G) {
    const int tid = threadIdx.x, s = blockIdx.x;
    const double* in = part + (size_t)s * nchunk * 3 * C;
    double* out = sums + (size_t)s * 3 * C;
    for (int i = tid; i < 3 * C; i += 256) {
        double v = in[i];
        for (int ch = 1; ch < nchunk; ++ch) v += in[(size_t)ch * 3 * C + i];
        out[i] = v;
    }
    __threadfence_block();
    __syncthreads();
    const int cpg = C / G;
    const double inv = 1.0 / ((double)P * cpg);
    for (int g = tid; g < G; g += 256) {
        double sx = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) sx += out[2 * C + c];
        const float delta = (float)(sx * inv);
        const double dr = (double)delta * (double)stats[((size_t)s * G + g) * 2 + 1];
        double m1 = 0.0, m2 = 0.0;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            const double ga = (double)gamma[c];
            const double s2 = out[C + c] - dr * out[c];
            out[C + c] = s2;
            m1 += ga * out[c];
            m2 += ga * s2;
        }
        *reinterpret_cast<float4*>(means + ((size_t)s * G + g) * 4) = make_float4((float)(m1 * inv), (float)(m2 * inv), delta, 0.f);
    }
}

// dbeta[c] = sum_s sums[s][0][c], dgamma[c] = sum_s sums[s][1][c]: a workgroup takes 64 channels; thread (q, c) adds the samples of
// quarter q in index order in fp64, the four quarters are added in order.
__global__ __launch_bounds__(256) void gb_param_kernel(const double* __restrict__ sums, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                       int S, int C) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x, cl = tid & 63, q = tid >> 6;
    const int c = blockIdx.x * 64 + cl;
    const int per = (S + 3) / 4, s0 = q * per, s1 = min(S, s0 + per);
    double vb = 0.0, vg = 0.0;
    if (c < C)
        for (int s = s0; s < s1; ++s) {
            vb += sums[(size_t)s * 3 * C + c];
            vg += sums[(size_t)s * 3 * C + C + c];
        }
    red[0][tid] = vb;
    red[1][tid] = vg;
    __syncthreads();
    if (q == 0 && c < C) {
        dbeta[c] = (float)(((red[0][cl] + red[0][64 + cl]) + red[0][128 + cl]) + red[0][192 + cl]);
        dgamma[c] = (float)(((red[1][cl] + red[1][64 + cl]) + red[1][128 + cl]) + red[1][192 + cl]);
    }
}

// pass 2: dx = rstd * fma(-xh, m2, fma(dv, gamma, -m1)) [+ dskip].  One thread per four channels of one position, grid-strided.
template <int ACT>
__global__ __launch_bounds__(256) void gb_dx_kernel(const float* __restrict__ da, const float* __restrict__ x, const float* __restrict__ stats,
                                                    const float* __restrict__ means, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, const float* __restrict__ dskip, float* __restrict__ dx,
                                                    size_t total4, unsigned n4s, int C, int G) {
    const int c4n = C >> 2, cpg = C / G;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
        const int s = (int)(i / n4s);
        const int j = (int)(i % (unsigned)c4n);
        float mean[4], rstd[4], delta[4], m1[4], m2[4], xc[4], xh[4], dv[4];
        gb_stats4(stats, s, G, cpg, j, mean, rstd);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float4 m = *reinterpret_cast<const float4*>(means + ((size_t)s * G + (4 * j + e) / cpg) * 4);
            m1[e] = m.x; m2[e] = m.y; delta[e] = m.z;
        }
        const float4 ga = *reinterpret_cast<const float4*>(gamma + 4 * j);
        const float4 be = *reinterpret_cast<const float4*>(beta + 4 * j);
        gb_elem4<ACT>(reinterpret_cast<const float4*>(x)[i], reinterpret_cast<const float4*>(da)[i], mean, rstd, delta, ga, be, xc, xh, dv);
        const float gs[4] = {ga.x, ga.y, ga.z, ga.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = rstd[e] * fmaf(-xh[e], m2[e], fmaf(dv[e], gs[e], -m1[e]));
        if (dskip) {
            const float4 d = reinterpret_cast<const float4*>(dskip)[i];
            o[0] += d.x; o[1] += d.y; o[2] += d.z; o[3] += d.w;
        }
        reinterpret_cast<float4*>(dx)[i] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline int gb_chunks(int P) { return (P + GB_CHUNK - 1) / GB_CHUNK; }
static inline bool gb_shape_ok(int S, int P, int C, int G) {
    return S >= 1 && S <= 65535 && P >= 1 && C >= 4 && C % 4 == 0 && G >= 1 && C % G == 0 && (long long)S * P * C < (1ll << 40) &&
           (long long)P * (C / 4) < (1ll << 32);
}

static inline int cw_log2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return (v > 0 && (1 << l) == v) ? l : -1;
}
static inline bool cw_shape_ok(int S, int H, int W, int N, int C, int kh, int kw) {
    return S >= 0 && cw_log2(H) >= 0 && cw_log2(W) >= 0 && N >= 128 && C >= 128 && N % 128 == 0 && C % 128 == 0 && kh >= 1 && kw >= 1 &&
           kh <= 5 && kw <= 5 && (kh & 1) && (kw & 1) && (long long)S * H * W < (1ll << 31) - 4096 && (long long)N * kh * kw * C < (1ll << 31);
}

}  // namespace bg

using namespace bg;

extern "C" int bg_conv_wgrad_split(int S, int H, int W, int N, int C, int kh, int kw) {
    if (!cw_shape_ok(S, H, W, N, C, kh, kw) || S == 0) return 1;
    return lb_auto_split(S * H * W, N, kh * kw * C);
}

extern "C" size_t bg_conv_wgrad_workspace_bytes(int S, int H, int W, int N, int C, int kh, int kw, int split) {
    if (!cw_shape_ok(S, H, W, N, C, kh, kw) || S == 0 || split < 0 || split > LB_MAX_SPLIT) return 0;
    const int K = kh * kw * C;
    return lb_workspace(N, K, split == 0 ? lb_auto_split(S * H * W, N, K) : split);
}

extern "C" int bg_conv_wgrad(const void* dy, int ld_dy, const void* a, int ld_a, void* dw, void* db, int S, int H, int W, int N, int C,
                             int kh, int kw, int dtype, int out_dtype, int split, void* workspace, size_t workspace_bytes,
                             bg_stream_t stream) {
    if (int e = lb_wgrad_dtypes("bg_conv_wgrad", dtype, out_dtype)) return e;
    BG_REQUIRE(S >= 0 && cw_log2(H) >= 0 && cw_log2(W) >= 0 && (long long)S * H * W < (1ll << 31) - 4096, BG_E_SHAPE,
               "bg_conv_wgrad: S = %d samples of an H = %d x W = %d grid (powers of two, fewer than 2^31 pixels)", S, H, W);
    BG_REQUIRE(kh >= 1 && kw >= 1 && kh <= 5 && kw <= 5 && (kh & 1) && (kw & 1), BG_E_SHAPE,
               "bg_conv_wgrad: window %d x %d (odd, each at most 5)", kh, kw);
    BG_REQUIRE(N >= 128 && C >= 128 && N % 128 == 0 && C % 128 == 0 && (long long)N * kh * kw * C < (1ll << 31), BG_E_SHAPE,
               "bg_conv_wgrad: N = %d and C = %d must be multiples of 128", N, C);
    const int M = S * H * W, lh = cw_log2(H), lw = cw_log2(W);
    return lb_wgrad_entry("bg_conv_wgrad", "a", "C", "pixel", dy, ld_dy, a, ld_a, C, dw, db, M, N, kh * kw * C, dtype, out_dtype, split, true,
                          workspace, workspace_bytes, stream, [&](auto F, auto OUT, dim3 grid, void* dw_, void* db_, int slice_rows) {
                              hipLaunchKernelGGL((cw_wgrad_kernel<decltype(F)::value, decltype(OUT)::value>), grid, dim3(256), 0,
                                                 (hipStream_t)stream, dy, ld_dy, a, ld_a, dw_, db_, M, N, C, kh, kw, lh, lw, slice_rows);
                          });
}

extern "C" int bg_conv_weight_pack(const void* src, int src_dtype, int N, int C, int kh, int kw, void* fwd, void* dgrad, int dtype,
                                   bg_stream_t stream) {
    BG_REQUIRE(dtype == BG_BF16 || dtype == BG_F16, BG_E_DTYPE, "bg_conv_weight_pack: target dtype %d (BG_BF16 or BG_F16)", dtype);
    BG_REQUIRE(src_dtype == BG_F32 || src_dtype == dtype, BG_E_DTYPE,
               "bg_conv_weight_pack: source dtype %d is neither BG_F32 nor the target dtype %d", src_dtype, dtype);
    BG_REQUIRE(N >= 32 && C >= 32 && N % 32 == 0 && C % 32 == 0 && N / 32 <= 65535, BG_E_SHAPE,
               "bg_conv_weight_pack: N = %d and C = %d must be multiples of 32", N, C);
    BG_REQUIRE(kh >= 1 && kw >= 1 && kh <= 5 && kw <= 5 && (kh & 1) && (kw & 1) && (long long)N * C * kh * kw < (1ll << 31), BG_E_SHAPE,
               "bg_conv_weight_pack: window %d x %d (odd, each at most 5)", kh, kw);
    BG_REQUIRE(src != nullptr, BG_E_ARG, "bg_conv_weight_pack: null pointer (src)");
    BG_REQUIRE(fwd != nullptr || dgrad != nullptr, BG_E_ARG, "bg_conv_weight_pack: null pointer (fwd and dgrad: at least one output)");
    BG_REQUIRE(aligned(src, 16) && aligned(fwd, 16) && aligned(dgrad, 16), BG_E_ALIGN, "bg_conv_weight_pack: 16-byte alignment of src / fwd / dgrad");
    const dim3 grid(C / 32, N / 32);
    hipStream_t s = (hipStream_t)stream;
    const int T = kh * kw;
    if (src_dtype != BG_F32) hipLaunchKernelGGL(cw_pack_kernel<0>, grid, dim3(256), 0, s, src, fwd, dgrad, N, C, T);
    else if (dtype == BG_BF16) hipLaunchKernelGGL(cw_pack_kernel<1>, grid, dim3(256), 0, s, src, fwd, dgrad, N, C, T);
    else hipLaunchKernelGGL(cw_pack_kernel<2>, grid, dim3(256), 0, s, src, fwd, dgrad, N, C, T);
    return launch_status("conv_weight_pack");
}

extern "C" size_t bg_gn_act_bwd_workspace_bytes(int S, int P, int C, int G) {
    if (!gb_shape_ok(S, P, C, G)) return 0;
    return al256((size_t)S * gb_chunks(P) * 3 * C * sizeof(double)) + al256((size_t)S * 3 * C * sizeof(double)) + al256((size_t)S * G * 4 * sizeof(float));
}

extern "C" int bg_gn_act_bwd(const float* da, const float* x, const float* stats, const float* gamma, const float* beta, const float* dskip,
                             float* dx, float* dgamma, float* dbeta, int S, int P, int C, int G, int act, void* workspace,
                             size_t workspace_bytes, bg_stream_t stream) {
    BG_REQUIRE(S >= 1 && S <= 65535 && P >= 1 && (long long)S * P * C < (1ll << 40) && (long long)P * (C / 4) < (1ll << 32), BG_E_SHAPE,
               "bg_gn_act_bwd: S = %d samples (1 .. 65535) of P = %d positions (>= 1)", S, P);
    BG_REQUIRE(C >= 4 && C % 4 == 0 && G >= 1 && C % G == 0, BG_E_SHAPE, "bg_gn_act_bwd: C = %d must be a multiple of 4 and of G = %d", C, G);
    BG_REQUIRE(act >= BG_VACT_NONE && act <= BG_VACT_GELU, BG_E_ARG, "bg_gn_act_bwd: act = %d (bg_vae_act)", act);
    BG_REQUIRE(da && x && stats && gamma && beta && dx, BG_E_ARG, "bg_gn_act_bwd: null pointer (da, x, stats, gamma, beta, dx)");
    BG_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), BG_E_ARG, "bg_gn_act_bwd: dgamma and dbeta: both or neither");
    BG_REQUIRE(aligned(da, 16) && aligned(x, 16) && aligned(dskip, 16) && aligned(dx, 16) && aligned(gamma, 16) && aligned(beta, 16) &&
                   aligned(stats, 8) && aligned(dgamma, 4) && aligned(dbeta, 4) && aligned(workspace, 16),
               BG_E_ALIGN, "bg_gn_act_bwd: 16-byte alignment of da / x / dskip / dx / gamma / beta / workspace (stats: 8)");
    const size_t need = bg_gn_act_bwd_workspace_bytes(S, P, C, G);
    BG_REQUIRE(workspace != nullptr && workspace_bytes >= need, BG_E_ARG, "bg_gn_act_bwd: workspace of %zu bytes, %zu needed",
               workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t s = (hipStream_t)stream;
    const int nchunk = gb_chunks(P);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    double* part = reinterpret_cast<double*>(ws);
    double* sums = reinterpret_cast<double*>(ws + al256((size_t)S * nchunk * 3 * C * sizeof(double)));
    float* means = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(sums) + al256((size_t)S * 3 * C * sizeof(double)));
    const size_t total4 = (size_t)S * P * (C / 4);
    const unsigned n4s = (unsigned)((size_t)P * (C / 4));
    const unsigned blocks = (unsigned)((total4 + 255) / 256 < 65536 ? (total4 + 255) / 256 : 65536);
    auto run = [&](auto A) {
        constexpr int ACT = decltype(A)::value;
        hipLaunchKernelGGL(gb_sums_kernel<ACT>, dim3(nchunk, S), dim3(256), 0, s, da, x, stats, gamma, beta, part, P, C, G);
        hipLaunchKernelGGL(gb_finish_kernel, dim3(S), dim3(256), 0, s, (const double*)part, stats, gamma, sums, means, nchunk, P, C, G);
        if (dgamma) hipLaunchKernelGGL(gb_param_kernel, dim3((C + 63) / 64), dim3(256), 0, s, (const double*)sums, dgamma, dbeta, S, C);
        hipLaunchKernelGGL(gb_dx_kernel<ACT>, dim3(blocks), dim3(256), 0, s, da, x, stats, (const float*)means, gamma, beta, dskip, dx, total4,
                           n4s, C, G);
    };
    if (act == BG_VACT_SILU) run(std::integral_constant<int, 1>{});
    else if (act == BG_VACT_GELU) run(std::integral_constant<int, 2>{});
    else run(std::integral_constant<int, 0>{});
    return launch_status("gn_act_bwd");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Downsample2D / Upsample2D convolutions: the weight gradient in three geometries, the stride-2 data gradient, the 2 x 2 sum
// ---------------------------------------------------------------------------------------------------------------------------------
namespace bg {

// the grid of dy for an H x W grid of `a`; false where the geometry does not take the grid
static inline bool cw_geom_grid(int H, int W, int geom, int& Ho, int& Wo) {
    if (cw_log2(H) < 0 || cw_log2(W) < 0 || geom < BG_CONV_SAME || geom > BG_CONV_UP2) return false;
    if (geom == BG_CONV_DOWN2 && (H < 2 || W < 2)) return false;
    if (H > (1 << 14) || W > (1 << 14)) return false;
    Ho = geom == BG_CONV_DOWN2 ? H / 2 : geom == BG_CONV_UP2 ? 2 * H : H;
    Wo = geom == BG_CONV_DOWN2 ? W / 2 : geom == BG_CONV_UP2 ? 2 * W : W;
    return true;
}
static inline bool cw_geom_ok(int S, int H, int W, int N, int C, int kh, int kw, int geom) {
    int Ho, Wo;
    if (!cw_geom_grid(H, W, geom, Ho, Wo)) return false;
    if (geom == BG_CONV_SAME) return cw_shape_ok(S, H, W, N, C, kh, kw);
    return kh == 3 && kw == 3 && cw_shape_ok(S, H, W, N, C, kh, kw) && cw_shape_ok(S, Ho, Wo, N, C, kh, kw);
}
static inline unsigned cd_blocks(size_t items) { return (unsigned)((items + 255) / 256 < 65536 ? (items + 255) / 256 : 65536); }

}  // namespace bg

extern "C" int bg_conv_wgrad_geom_split(int S, int H, int W, int N, int C, int kh, int kw, int geom) {
    int Ho, Wo;
    if (!cw_geom_ok(S, H, W, N, C, kh, kw, geom) || S == 0 || !cw_geom_grid(H, W, geom, Ho, Wo)) return 1;
    return lb_auto_split(S * Ho * Wo, N, kh * kw * C);
}

extern "C" size_t bg_conv_wgrad_geom_workspace_bytes(int S, int H, int W, int N, int C, int kh, int kw, int geom, int split) {
    int Ho, Wo;
    if (!cw_geom_ok(S, H, W, N, C, kh, kw, geom) || S == 0 || split < 0 || split > LB_MAX_SPLIT || !cw_geom_grid(H, W, geom, Ho, Wo)) return 0;
    const int K = kh * kw * C;
    return lb_workspace(N, K, split == 0 ? lb_auto_split(S * Ho * Wo, N, K) : split);
}

extern "C" int bg_conv_wgrad_geom(const void* dy, int ld_dy, const void* a, int ld_a, void* dw, void* db, int S, int H, int W, int N, int C,
                                  int kh, int kw, int geom, int dtype, int out_dtype, int split, void* workspace, size_t workspace_bytes,
                                  bg_stream_t stream) {
    BG_REQUIRE(geom >= BG_CONV_SAME && geom <= BG_CONV_UP2, BG_E_ARG,
               "bg_conv_wgrad_geom: geom = %d (bg_conv_geom: BG_CONV_SAME = 0, BG_CONV_DOWN2 = 1, BG_CONV_UP2 = 2)", geom);
    if (geom == BG_CONV_SAME)
        return bg_conv_wgrad(dy, ld_dy, a, ld_a, dw, db, S, H, W, N, C, kh, kw, dtype, out_dtype, split, workspace, workspace_bytes, stream);
    if (int e = lb_wgrad_dtypes("bg_conv_wgrad_geom", dtype, out_dtype)) return e;
    int Ho = 0, Wo = 0;
    BG_REQUIRE(S >= 0 && cw_log2(H) >= 0 && cw_log2(W) >= 0 && H <= (1 << 14) && W <= (1 << 14), BG_E_SHAPE,
               "bg_conv_wgrad_geom: S = %d samples of an H = %d x W = %d grid of a (powers of two, at most 16384)", S, H, W);
    BG_REQUIRE(cw_geom_grid(H, W, geom, Ho, Wo), BG_E_SHAPE, "bg_conv_wgrad_geom: BG_CONV_DOWN2 halves the grid: H = %d and W = %d must be at least 2",
               H, W);
    BG_REQUIRE((long long)S * H * W < (1ll << 31) - 4096 && (long long)S * Ho * Wo < (1ll << 31) - 4096, BG_E_SHAPE,
               "bg_conv_wgrad_geom: S = %d samples of %d x %d and %d x %d pixels (fewer than 2^31 pixels)", S, H, W, Ho, Wo);
    BG_REQUIRE(kh == 3 && kw == 3, BG_E_SHAPE, "bg_conv_wgrad_geom: window %d x %d (3 x 3 only for BG_CONV_DOWN2 / BG_CONV_UP2)", kh, kw);
    BG_REQUIRE(N >= 128 && C >= 128 && N % 128 == 0 && C % 128 == 0 && (long long)N * 9 * C < (1ll << 31), BG_E_SHAPE,
               "bg_conv_wgrad_geom: N = %d and C = %d must be multiples of 128", N, C);
    const int M = S * Ho * Wo, lh = cw_log2(Ho), lw = cw_log2(Wo);
    const bool down = geom == BG_CONV_DOWN2;
    return lb_wgrad_entry("bg_conv_wgrad_geom", "a", "C", "pixel", dy, ld_dy, a, ld_a, C, dw, db, M, N, 9 * C, dtype, out_dtype, split, true,
                          workspace, workspace_bytes, stream, [&](auto F, auto OUT, dim3 grid, void* dw_, void* db_, int slice_rows) {
                              if (down)
                                  hipLaunchKernelGGL((cw_wgrad_kernel<decltype(F)::value, decltype(OUT)::value, 1>), grid, dim3(256), 0,
                                                     (hipStream_t)stream, dy, ld_dy, a, ld_a, dw_, db_, M, N, C, 3, 3, lh, lw, slice_rows);
                              else
                                  hipLaunchKernelGGL((cw_wgrad_kernel<decltype(F)::value, decltype(OUT)::value, 2>), grid, dim3(256), 0,
                                                     (hipStream_t)stream, dy, ld_dy, a, ld_a, dw_, db_, M, N, C, 3, 3, lh, lw, slice_rows);
                          });
}

extern "C" int bg_conv_weight_pack_down(const void* src, int src_dtype, int N, int C, void* fwd, void* down, int dtype, bg_stream_t stream) {
    BG_REQUIRE(dtype == BG_BF16 || dtype == BG_F16, BG_E_DTYPE, "bg_conv_weight_pack_down: target dtype %d (BG_BF16 or BG_F16)", dtype);
    BG_REQUIRE(src_dtype == BG_F32 || src_dtype == dtype, BG_E_DTYPE,
               "bg_conv_weight_pack_down: source dtype %d is neither BG_F32 nor the target dtype %d", src_dtype, dtype);
    BG_REQUIRE(N >= 32 && C >= 32 && N % 32 == 0 && C % 32 == 0 && N / 32 <= 65535 && (long long)N * C * 9 < (1ll << 31), BG_E_SHAPE,
               "bg_conv_weight_pack_down: N = %d and C = %d must be multiples of 32", N, C);
    BG_REQUIRE(src != nullptr, BG_E_ARG, "bg_conv_weight_pack_down: null pointer (src)");
    BG_REQUIRE(fwd != nullptr || down != nullptr, BG_E_ARG, "bg_conv_weight_pack_down: null pointer (fwd and down: at least one output)");
    BG_REQUIRE(aligned(src, 16) && aligned(fwd, 16) && aligned(down, 16), BG_E_ALIGN, "bg_conv_weight_pack_down: 16-byte alignment of src / fwd / down");
    const dim3 grid(C / 32, N / 32);
    hipStream_t s = (hipStream_t)stream;
    if (src_dtype != BG_F32) hipLaunchKernelGGL(cd_pack_kernel<0>, grid, dim3(256), 0, s, src, fwd, down, N, C);
    else if (dtype == BG_BF16) hipLaunchKernelGGL(cd_pack_kernel<1>, grid, dim3(256), 0, s, src, fwd, down, N, C);
    else hipLaunchKernelGGL(cd_pack_kernel<2>, grid, dim3(256), 0, s, src, fwd, down, N, C);
    return launch_status("conv_weight_pack_down");
}

static inline bool cd_shape_ok(int S, int H, int W, int N, int C) {
    return S >= 1 && cw_log2(H) >= 1 && cw_log2(W) >= 1 && H <= (1 << 14) && W <= (1 << 14) && (long long)S * H * W < (1ll << 31) - 4096 &&
           N >= 128 && C >= 128 && N % 128 == 0 && C % 128 == 0 && (long long)N * 9 * C < (1ll << 31);
}

extern "C" size_t bg_conv_down_dgrad_workspace_bytes(int S, int H, int W, int N, int C) {
    if (!cd_shape_ok(S, H, W, N, C)) return 0;
    const size_t M = (size_t)S * (H / 2) * (W / 2);
    return 2 * al256(M * 2 * N * 2) + al256(M * 4 * N * 2) + al256(4 * M * C * sizeof(float));
}

extern "C" int bg_conv_down_dgrad(const void* dy, int ld_dy, const void* pack, float* dx, int S, int H, int W, int N, int C, int dtype,
                                  void* workspace, size_t workspace_bytes, bg_stream_t stream) {
    BG_REQUIRE(dtype == BG_BF16 || dtype == BG_F16, BG_E_DTYPE, "bg_conv_down_dgrad: operand dtype %d (BG_BF16 or BG_F16)", dtype);
    BG_REQUIRE(S >= 1 && cw_log2(H) >= 1 && cw_log2(W) >= 1 && H <= (1 << 14) && W <= (1 << 14) && (long long)S * H * W < (1ll << 31) - 4096,
               BG_E_SHAPE, "bg_conv_down_dgrad: S = %d samples (>= 1) of an H = %d x W = %d grid of dx (powers of two, at least 2, fewer than 2^31 pixels)",
               S, H, W);
    BG_REQUIRE(N >= 128 && C >= 128 && N % 128 == 0 && C % 128 == 0 && (long long)N * 9 * C < (1ll << 31), BG_E_SHAPE,
               "bg_conv_down_dgrad: N = %d and C = %d must be multiples of 128", N, C);
    BG_REQUIRE(dy != nullptr && pack != nullptr && dx != nullptr, BG_E_ARG, "bg_conv_down_dgrad: null pointer (dy, pack, dx)");
    BG_REQUIRE(ld_dy >= N && ld_dy % 8 == 0, BG_E_ALIGN, "bg_conv_down_dgrad: pixel stride ld_dy = %d (>= N) must be a multiple of 8 elements", ld_dy);
    BG_REQUIRE(aligned(dy, 16) && aligned(pack, 16) && aligned(dx, 16) && aligned(workspace, 16), BG_E_ALIGN,
               "bg_conv_down_dgrad: 16-byte alignment of dy / pack / dx / workspace");
    const size_t need = bg_conv_down_dgrad_workspace_bytes(S, H, W, N, C);
    BG_REQUIRE(workspace != nullptr && workspace_bytes >= need, BG_E_ARG, "bg_conv_down_dgrad: workspace of %zu bytes, %zu needed",
               workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t s = (hipStream_t)stream;
    const int Ho = H / 2, Wo = W / 2, Mi = S * Ho * Wo;
    const size_t M = (size_t)Mi;
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    unsigned short* a1 = reinterpret_cast<unsigned short*>(ws);
    unsigned short* a2 = reinterpret_cast<unsigned short*>(ws + al256(M * 2 * N * 2));
    unsigned short* a3 = reinterpret_cast<unsigned short*>(ws + 2 * al256(M * 2 * N * 2));
    float* cls = reinterpret_cast<float*>(ws + 2 * al256(M * 2 * N * 2) + al256(M * 4 * N * 2));
    const size_t g_items = M * (N / 8);
    hipLaunchKernelGGL(cd_gather_kernel, dim3(cd_blocks(g_items)), dim3(256), 0, s, reinterpret_cast<const unsigned short*>(dy), ld_dy, a1, a2,
                       a3, g_items, N, cw_log2(Ho), cw_log2(Wo));
    if (int e = launch_status("conv_down_dgrad")) return e;
    // class k: operand [M, T_k * N] times block k of the pack [C, T_k * N] -> cls[k] [M, C]
    const unsigned short* w = reinterpret_cast<const unsigned short*>(pack);
    const void* ops[4] = {dy, a1, a2, a3};
    const int lda[4] = {ld_dy, 2 * N, 2 * N, 4 * N}, taps[4] = {1, 2, 2, 4}, first[4] = {0, 1, 3, 5};
    for (int k = 0; k < 4; ++k) {
        if (int e = bg_gemm_bias_act_fwd(ops[k], lda[k], w + (size_t)first[k] * C * N, nullptr, cls + (size_t)k * M * C, C, Mi, C, C, taps[k] * N,
                                         dtype, BG_F32, BG_ACT_NONE, nullptr, 0, 1, stream))
            return e;
    }
    const size_t i_items = (size_t)S * H * W * (C / 4);
    hipLaunchKernelGGL(cd_interleave_kernel, dim3(cd_blocks(i_items)), dim3(256), 0, s, reinterpret_cast<const float4*>(cls),
                       reinterpret_cast<float4*>(dx), i_items, M, C, cw_log2(H), cw_log2(W));
    return launch_status("conv_down_dgrad");
}

extern "C" int bg_pool2x2_sum(const float* u, const float* add, float* y, int S, int H, int W, int C, bg_stream_t stream) {
    BG_REQUIRE(S >= 1 && H >= 1 && W >= 1 && (long long)S * H * W < (1ll << 31), BG_E_SHAPE,
               "bg_pool2x2_sum: S = %d samples of an H = %d x W = %d output grid (each >= 1, fewer than 2^31 pixels)", S, H, W);
    BG_REQUIRE(C >= 4 && C % 4 == 0, BG_E_SHAPE, "bg_pool2x2_sum: C = %d must be a multiple of 4", C);
    BG_REQUIRE(u != nullptr && y != nullptr, BG_E_ARG, "bg_pool2x2_sum: null pointer (u, y)");
    BG_REQUIRE(aligned(u, 16) && aligned(add, 16) && aligned(y, 16), BG_E_ALIGN, "bg_pool2x2_sum: 16-byte alignment of u / add / y");
    const size_t items = (size_t)S * H * W * (C / 4);
    hipLaunchKernelGGL(pool2x2_sum_kernel, dim3(cd_blocks(items)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(u),
                       reinterpret_cast<const float4*>(add), reinterpret_cast<float4*>(y), items, H, W, C);
    return launch_status("pool2x2_sum");
}
