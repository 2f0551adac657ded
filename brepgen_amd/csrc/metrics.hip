// Evaluation metrics of the reference's pc_metric.py on the device: the pairwise Chamfer matrix behind
// COV / MMD (`_pairwise_CD`, pc_metric.py:45-80 -- there the `chamfer_distance` CUDA extension) and the occupancy-grid counts behind
// JSD (`entropy_of_occupancy_grid`, pc_metric.py:110-149 -- there an sklearn KD-tree on the CPU).
//
// bg_chamfer_pairwise -- DIRECT form, one workgroup per cloud pair (i, j), one pass for both directions:
//   * the 256 threads keep up to 2048 points of a_i in REGISTERS (8 per thread), b_j sits in LDS as SoA (24 KB for 2000 points) and is
//     read with wave-uniform ds_read_b128 (a broadcast: no bank conflicts); every point pair costs 3 sub + 1 mul + 2 fma and its share
//     of two v_min3: the row minimum (over q, per register point) and the column partial (over the thread's 8 points, per q);
//   * column minima: the thread's partials for 4 consecutive q are reduced over the 16 lanes of its DPP row (across the four banks for all
//     four q, then -- bank k keeping q + k -- over the bank's four lanes), lane 0 of every bank then ds_min_u32 its row's minimum into
//     cmin[q + k] (distances are >= +0, so their bit patterns order like unsigned integers: an INTEGER atomic, exact and order-free).
//     A minimum does not depend on the order it is taken in, so nothing here touches the bits;
//   * the two sums (rows, columns) run in a fixed order: per thread serially by index, then one 256-leaf tree in LDS.
//   out[i, j] therefore depends on a_i, b_j, Pa and Pb alone.  No floating-point atomics.
//   FINITE INPUTS ONLY: the unsigned ordering of the column side holds for finite distances; a NaN or Inf coordinate gives a NaN bit pattern
//   that orders above +Inf in ds_min_u32 while v_min3_f32 drops it on the row side, so the two directions would treat it differently.
//   Pa > 2048 (a_i does not fit the registers of one workgroup, so a column minimum would need state across register tiles): the same
//   pass runs twice with the roles swapped and rows only -- twice the arithmetic, any size.
//
// bg_occupancy_counts -- one workgroup per cloud, the per-axis nearest node by a lower-bound search on the fp32 axis and ONE comparison
// of the two neighbours' distances in double (exact: a difference of two floats is a double), an LDS bitmap for "this cloud touched the
// cell"; integer atomics only.
#include "bg_common.h"

namespace bg {

constexpr int MT_THREADS = 256;
constexpr int MT_T = 8;                           // register points per thread
constexpr int MT_TA = MT_THREADS * MT_T;          // points of the register-side cloud per tile
constexpr int MT_TB = 2048;                       // points of the LDS-side cloud per tile
constexpr unsigned MT_INF = 0x7f800000u;
constexpr unsigned MT_PAIRS_PER_LAUNCH = 1u << 22;   // cloud pairs (= workgroups) per launch of bg_chamfer_pairwise

// Column partials travel as the bit patterns of their distances (>= +0: unsigned order == float order; no canonicalisation needed).
template <int CTRL>
__device__ __forceinline__ unsigned dpp_umin(unsigned v) {
    return min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true));
}
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;

// One direction (+ the other one if COLS) of one cloud pair: A [Pa,3] on the register side, B [Pb,3] on the LDS side.
//   rs: this thread's share of sum_p min_q |A_p - B_q|^2;  cs (COLS, needs Pa <= MT_TA): its share of sum_q min_p.
template <bool COLS>
__device__ __forceinline__ void chamfer_pass(const float* __restrict__ A, int Pa, const float* __restrict__ B, int Pb, float* sx,
                                             float* sy, float* sz, unsigned* cmin, float& rs, float& cs) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int bank = (lane >> 2) & 3;                 // of the lane's DPP row
    unsigned keep[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) keep[k] = bank == k ? ~0u : 0u;
    rs = 0.f;
    cs = 0.f;
    for (int a0 = 0; a0 < Pa; a0 += MT_TA) {
        float ax[MT_T], ay[MT_T], az[MT_T], rmin[MT_T];
#pragma unroll
        for (int t = 0; t < MT_T; ++t) {
            const int p = a0 + t * MT_THREADS + tid;
            const size_t pp = p < Pa ? p : 0;         // a slot past the end repeats point 0: it cannot lower a column minimum
            ax[t] = A[3 * pp]; ay[t] = A[3 * pp + 1]; az[t] = A[3 * pp + 2];
            rmin[t] = __uint_as_float(MT_INF);
        }
        for (int b0 = 0; b0 < Pb; b0 += MT_TB) {
            const int nb = min(MT_TB, Pb - b0), nb4 = (nb + 3) & ~3;
            __syncthreads();                          // the previous tile has been read (points and cmin)
            for (int q = tid; q < nb4; q += MT_THREADS) {
                const size_t qq = q < nb ? b0 + q : 0;   // likewise: a repeat of point 0 cannot lower a row minimum
                sx[q] = B[3 * qq]; sy[q] = B[3 * qq + 1]; sz[q] = B[3 * qq + 2];
                if (COLS) cmin[q] = MT_INF;
            }
            __syncthreads();
            for (int q = 0; q < nb4; q += 4) {
                const f32x4 bx = *reinterpret_cast<const f32x4*>(sx + q), by = *reinterpret_cast<const f32x4*>(sy + q),
                            bz = *reinterpret_cast<const f32x4*>(sz + q);
                float c[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) c[k] = __uint_as_float(MT_INF);
#pragma unroll
                for (int t = 0; t < MT_T; ++t) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float dx = ax[t] - bx[k], dy = ay[t] - by[k], dz = az[t] - bz[k];
                        const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                        rmin[t] = __builtin_fminf(rmin[t], d);
                        if (COLS) c[k] = __builtin_fminf(c[k], d);
                    }
                }
                if (COLS) {
                    // minimum over the 16 lanes of every DPP row: first across its four banks (lane l with 15 - l, then with 7 - l) for all
                    // four q, then -- bank k keeping q + k -- over the bank's four lanes; lane 0 of every bank hands the result in
                    unsigned u[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) u[k] = dpp_umin<DPP_ROW_HALF_MIRROR>(dpp_umin<DPP_ROW_MIRROR>(__float_as_uint(c[k])));
                    unsigned v = (u[0] & keep[0]) | (u[1] & keep[1]) | (u[2] & keep[2]) | (u[3] & keep[3]);   // a select without branches
                    v = dpp_umin<DPP_QUAD_2301>(dpp_umin<DPP_QUAD_1032>(v));
                    if ((lane & 3) == 0) atomicMin(cmin + q + bank, v);
                }
            }
            if (COLS) {
                __syncthreads();
                for (int q = tid; q < nb; q += MT_THREADS) cs += __uint_as_float(cmin[q]);
            }
        }
#pragma unroll
        for (int t = 0; t < MT_T; ++t)
            if (a0 + t * MT_THREADS + tid < Pa) rs += rmin[t];
    }
}

// fixed-order sum of one value per thread; the result is returned to every thread
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int o = MT_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(MT_THREADS) void chamfer_pairwise_kernel(const float* __restrict__ a, int Pa, const float* __restrict__ b,
                                                                      int R, int Pb, float* __restrict__ out, unsigned pair0) {
    __shared__ __attribute__((aligned(16))) float sx[MT_TB], sy[MT_TB], sz[MT_TB];
    __shared__ unsigned cmin[MT_TB];
    __shared__ float red[MT_THREADS];
    const unsigned pair = pair0 + blockIdx.x;
    const unsigned i = pair / (unsigned)R, j = pair - i * (unsigned)R;
    const float* A = a + (size_t)i * Pa * 3;
    const float* B = b + (size_t)j * Pb * 3;
    float rs, cs, unused;
    if (Pa <= MT_TA) {
        chamfer_pass<true>(A, Pa, B, Pb, sx, sy, sz, cmin, rs, cs);
    } else {
        chamfer_pass<false>(A, Pa, B, Pb, sx, sy, sz, cmin, rs, unused);
        chamfer_pass<false>(B, Pb, A, Pa, sx, sy, sz, cmin, cs, unused);
    }
    rs = block_sum(rs, red);
    cs = block_sum(cs, red);
    if (threadIdx.x == 0) out[pair] = rs / (float)Pa + cs / (float)Pb;
}

constexpr int OC_MAXRES = 64;

__device__ __forceinline__ int nearest_node(const float* axis, int res, float x) {
    int lo = 0, hi = res;                              // first node >= x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (axis[mid] < x) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) return 0;
    if (lo == res) return res - 1;
    const double below = (double)x - (double)axis[lo - 1], above = (double)axis[lo] - (double)x;
    return above < below ? lo : lo - 1;                // an exact tie goes to the lower node
}

__global__ __launch_bounds__(256) void occupancy_counts_kernel(const float* __restrict__ pts, int P, const float* __restrict__ axis,
                                                               int res, unsigned* __restrict__ point_counts,
                                                               unsigned* __restrict__ cloud_counts) {
    __shared__ unsigned seen[OC_MAXRES * OC_MAXRES * OC_MAXRES / 32];
    __shared__ float ax[OC_MAXRES];
    const int tid = threadIdx.x, words = (res * res * res + 31) / 32;
    for (int w = tid; w < words; w += 256) seen[w] = 0u;
    if (tid < res) ax[tid] = axis[tid];
    __syncthreads();
    const float* p = pts + (size_t)blockIdx.x * P * 3;
    for (int n = tid; n < P; n += 256) {
        const int ix = nearest_node(ax, res, p[3 * (size_t)n]), iy = nearest_node(ax, res, p[3 * (size_t)n + 1]),
                  iz = nearest_node(ax, res, p[3 * (size_t)n + 2]);
        const unsigned cell = (unsigned)((ix * res + iy) * res + iz), bit = 1u << (cell & 31);
        atomicAdd(point_counts + cell, 1u);
        if (!(atomicOr(seen + (cell >> 5), bit) & bit)) atomicAdd(cloud_counts + cell, 1u);   // first point of this cloud in the cell
    }
}

}  // namespace bg

extern "C" int bg_chamfer_pairwise(const float* a, int S, int Pa, const float* b, int R, int Pb, float* out, bg_stream_t stream) {
    BG_REQUIRE(a && b && out, BG_E_ARG, "bg_chamfer_pairwise: null pointer");
    BG_REQUIRE(S > 0 && R > 0 && Pa > 0 && Pb > 0, BG_E_SHAPE, "bg_chamfer_pairwise: need S, R, Pa, Pb >= 1 (S=%d R=%d Pa=%d Pb=%d)", S, R,
               Pa, Pb);
    BG_REQUIRE((long long)S * R <= 0x7fffffffLL, BG_E_SHAPE, "bg_chamfer_pairwise: S * R = %lld exceeds one grid (2^31 - 1 pairs)",
               (long long)S * R);
    BG_REQUIRE(Pa <= 0x7fffffff / 3 && Pb <= 0x7fffffff / 3, BG_E_SHAPE, "bg_chamfer_pairwise: cloud too large (Pa=%d Pb=%d)", Pa, Pb);
    // one workgroup per pair; a launch carries at most 2^22 of them (2^30 threads, well inside what one grid may hold), the kernel takes
    // the first pair of its slice: the slicing changes nothing an entry depends on
    const unsigned total = (unsigned)S * (unsigned)R;
    for (unsigned pair0 = 0; pair0 < total; pair0 += bg::MT_PAIRS_PER_LAUNCH) {
        const unsigned n = total - pair0 < bg::MT_PAIRS_PER_LAUNCH ? total - pair0 : bg::MT_PAIRS_PER_LAUNCH;
        hipLaunchKernelGGL(bg::chamfer_pairwise_kernel, dim3(n), dim3(bg::MT_THREADS), 0, (hipStream_t)stream, a, Pa, b, R, Pb, out, pair0);
    }
    return bg::launch_status("bg_chamfer_pairwise");
}

extern "C" int bg_occupancy_counts(const float* pts, int n_clouds, int P, const float* axis, int res, unsigned* point_counts,
                                   unsigned* cloud_counts, bg_stream_t stream) {
    BG_REQUIRE(pts && axis && point_counts && cloud_counts, BG_E_ARG, "bg_occupancy_counts: null pointer");
    BG_REQUIRE(n_clouds > 0 && P > 0, BG_E_SHAPE, "bg_occupancy_counts: need n_clouds, P >= 1 (n_clouds=%d P=%d)", n_clouds, P);
    BG_REQUIRE(res >= 1 && res <= bg::OC_MAXRES, BG_E_SHAPE, "bg_occupancy_counts: need 1 <= res <= 64 (res=%d)", res);
    BG_REQUIRE(P <= 0x7fffffff / 3, BG_E_SHAPE, "bg_occupancy_counts: cloud too large (P=%d)", P);
    hipLaunchKernelGGL(bg::occupancy_counts_kernel, dim3(n_clouds), dim3(256), 0, (hipStream_t)stream, pts, P, axis, res, point_counts,
                       cloud_counts);
    return bg::launch_status("bg_occupancy_counts");
}
