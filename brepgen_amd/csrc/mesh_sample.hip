// Surface sampling of the reference's sample_points.py (`trimesh.sample.sample_surface`, 2000 points per
// generated STL, one CPU process per core there): pick a triangle with probability proportional to its area, place a point in it
// uniformly.  One launch for all meshes of a batch, one workgroup per mesh.
//
// Phase 1 -- the inclusive running sum of the fp64 triangle areas (fp32 vertices widened first), in chunks of 256 x 8 triangles:
//   * areas are computed one triangle per thread and lane (all of a thread's loads in flight together) and parked in the table; thread t
//     then owns 8 CONSECUTIVE entries and sums them in order;
//   * the 256 thread totals are chained IN ORDER on top of the previous chunk's last value (thread 0; 256 dependent additions per chunk);
//   * entry k = fl(base of its thread + its local sum).
//   Every level is "value of the previous group's LAST entry + local running sum", so the table is non-decreasing in floating point and a
//   zero-area triangle repeats its predecessor's value EXACTLY -- which is what lets the search below never pick one.  (A tree scan
//   associates neighbours differently and may step down by an ulp, or up at a zero-area triangle.)
//   The table lives in LDS up to MS_CAP triangles and in the caller's workspace above that; the same code serves both.
// Phase 2 -- per point: x = u0 * area in fp64, the smallest k with cdf_k > x by bisection, four points of a thread side by side (if
//   rounding leaves none: the last entry that raised the sum), then trimesh's reflected barycentric placement in fp32, op for op as include/brepgen_hip.h states it (the build has
//   -ffp-contract=off, so a numpy restatement is bit-identical).
// Uniforms are either the caller's or one Philox block per point, counter (p, GLOBAL mesh index, draw id, tag): a cloud depends on the
// seed, the draw id, the global mesh index and the mesh alone, not on the batch or the rank it was sampled in (as the noise of rng.hip).
#include "bg_common.h"
#include "philox.h"

namespace bg {

constexpr int MS_THREADS = 256;
constexpr int MS_E = 8;                            // consecutive table entries per thread
constexpr int MS_CHUNK = MS_THREADS * MS_E;
constexpr int MS_CAP = 6144;                       // triangles whose table stays in LDS (48 KiB of fp64: three workgroups per CU)
constexpr uint32_t MS_TAG = 0x5A3D0000u;           // Philox domain tag (bg_philox_randn: 0xB9E5)

// smallest k in [0, n] with cdf[k] > x (STRICT) or cdf[k] >= x; n if there is none (also for a NaN x: every comparison is false)
template <bool STRICT>
__device__ __forceinline__ int first_above(const double* cdf, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const double c = cdf[mid];
        if (STRICT ? c > x : c >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// one mesh: tri [T, 3, 3], cdf [T] (LDS or global).  Returns the total area to every thread.
__device__ __forceinline__ double area_table(const float* __restrict__ tri, int T, double* cdf, double* base) {
    const int tid = threadIdx.x;
    double carry = 0.0;
    for (int c0 = 0; c0 < T; c0 += MS_CHUNK) {
        const int n = min(MS_CHUNK, T - c0);
        // all 9 x MS_E loads of a thread are issued before the first area is formed: one memory round trip per chunk, not MS_E
        float v[MS_E][9];
#pragma unroll
        for (int j = 0; j < MS_E; ++j) {
            const float* q = tri + (size_t)(c0 + min(j * MS_THREADS + tid, n - 1)) * 9;      // a slot past the end repeats the last triangle
#pragma unroll
            for (int i = 0; i < 9; ++i) v[j][i] = q[i];
        }
#pragma unroll
        for (int j = 0; j < MS_E; ++j) {
            const int k = j * MS_THREADS + tid;
            const double ax = v[j][0], ay = v[j][1], az = v[j][2];
            const double ux = (double)v[j][3] - ax, uy = (double)v[j][4] - ay, uz = (double)v[j][5] - az;
            const double wx = (double)v[j][6] - ax, wy = (double)v[j][7] - ay, wz = (double)v[j][8] - az;
            const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
            if (k < n) cdf[c0 + k] = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
        }
        __syncthreads();
        double local[MS_E];
        double run = 0.0;
#pragma unroll
        for (int j = 0; j < MS_E; ++j) {
            const int k = tid * MS_E + j;
            if (k < n) run += cdf[c0 + k];
            local[j] = run;
        }
        base[tid] = run;
        __syncthreads();
        if (tid == 0) {
            // eight totals per LDS round trip (idle threads left 0, which changes nothing): the additions stay one dependent chain
            const int owners = (n + MS_E - 1) / MS_E;
            double b = carry;
            for (int t0 = 0; t0 < owners; t0 += 8) {
                double tot[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) tot[j] = base[t0 + j];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    base[t0 + j] = b;
                    b += tot[j];                    // == the table entry of thread t0 + j's last triangle, bit for bit
                }
            }
            base[MS_THREADS] = b;
        }
        __syncthreads();
        const double b = base[tid];
#pragma unroll
        for (int j = 0; j < MS_E; ++j) {
            const int k = tid * MS_E + j;
            if (k < n) cdf[c0 + k] = b + local[j];
        }
        carry = base[MS_THREADS];
        __syncthreads();                            // base is rewritten by the next chunk; the table is read by phase 2
    }
    return carry;
}

constexpr int MS_G = 4;                            // points a thread carries through the search together (independent LDS round trips)

__device__ __forceinline__ void place_points(const float* __restrict__ tri, int T, const double* cdf, double area, int P, uint32_t seed_lo,
                                             uint32_t seed_hi, uint32_t draw, unsigned long long g, const double* __restrict__ uni,
                                             float* __restrict__ pts, int* __restrict__ face) {
    const int top = 1 << (31 - __builtin_clz(T));     // the largest power of two <= T (T >= 1 here)
    for (int p0 = threadIdx.x; p0 < P; p0 += MS_THREADS * MS_G) {
        double x[MS_G];
        float r1[MS_G], r2[MS_G];
        int k[MS_G];
#pragma unroll
        for (int i = 0; i < MS_G; ++i) {
            const int p = min(p0 + i * MS_THREADS, P - 1);      // a slot past the end repeats the last point and is not stored
            double u0;
            if (uni) {
                u0 = uni[3 * (size_t)p];
                r1[i] = (float)uni[3 * (size_t)p + 1];
                r2[i] = (float)uni[3 * (size_t)p + 2];
            } else {
                uint32_t c[4] = {(uint32_t)p, (uint32_t)g, draw, MS_TAG | (uint32_t)((g >> 32) & 0xFFFFu)};
                philox4x32_10(c, seed_lo, seed_hi);
                const uint64_t top52 = (((uint64_t)c[0] << 32) | c[1]) >> 12;
                u0 = ((double)top52 + 0.5) * 0x1p-52;       // exact: 2 * top52 + 1 < 2^53
                r1[i] = u01(c[2]);
                r2[i] = u01(c[3]);
            }
            x[i] = u0 * area;
            k[i] = 0;
        }
        // k = the number of entries <= x = the smallest k with cdf_k > x (the table never decreases); T if there is none, also for a NaN x.
        // A fixed number of steps for every lane and point, so the MS_G searches of a thread overlap their LDS (or L2) round trips
        for (int step = top; step > 0; step >>= 1) {
#pragma unroll
            for (int i = 0; i < MS_G; ++i) {
                const int j = k[i] + step;
                const double c = cdf[min(j, T) - 1];
                if (j <= T && !(c > x[i])) k[i] = j;
            }
        }
#pragma unroll
        for (int i = 0; i < MS_G; ++i)
            if (k[i] == T) k[i] = first_above<false>(cdf, T, area);   // rounding left none: the last entry that raised the sum (cdf[T - 1] == area)
        float v[MS_G][9];                                             // the MS_G triangles are gathered together as well
#pragma unroll
        for (int i = 0; i < MS_G; ++i) {
            const float* q = tri + (size_t)k[i] * 9;
#pragma unroll
            for (int c = 0; c < 9; ++c) v[i][c] = q[c];
        }
#pragma unroll
        for (int i = 0; i < MS_G; ++i) {
            const int p = p0 + i * MS_THREADS;
            if (p < P) {
                float s1 = r1[i], s2 = r2[i];
                if (s1 + s2 > 1.0f) {
                    s1 = 1.0f - s1;
                    s2 = 1.0f - s2;
                }
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const float a = v[i][d], e1 = v[i][3 + d] - a, e2 = v[i][6 + d] - a;
                    const float t1 = s1 * e1, t2 = s2 * e2;
                    pts[3 * (size_t)p + d] = (a + t1) + t2;
                }
                face[p] = k[i];
            }
        }
    }
}

__global__ __launch_bounds__(MS_THREADS) void mesh_sample_kernel(const float* __restrict__ tri, const int* __restrict__ tri_off, int P,
                                                                 uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, long long first_mesh,
                                                                 const double* __restrict__ uniforms, double* __restrict__ cdf_ws,
                                                                 float* __restrict__ points, int* __restrict__ face,
                                                                 double* __restrict__ area_out) {
    __shared__ double tab[MS_CAP];
    __shared__ double base[MS_THREADS + 1];
    const int m = blockIdx.x;
    const int t0 = tri_off[m];
    const int T = max(tri_off[m + 1] - t0, 0);
    const float* mesh = tri + (size_t)t0 * 9;
    const double* uni = uniforms ? uniforms + (size_t)m * P * 3 : nullptr;
    float* pts = points + (size_t)m * P * 3;
    int* fc = face + (size_t)m * P;
    const unsigned long long g = (unsigned long long)(first_mesh + m);
    const bool in_lds = T <= MS_CAP;
    const double area = in_lds ? area_table(mesh, T, tab, base) : area_table(mesh, T, cdf_ws + t0, base);
    if (threadIdx.x == 0) area_out[m] = area;
    if (!(area > 0.0 && area <= 1.79769313486231570815e308)) {      // no triangles, zero area, Inf or NaN: nothing to pick from
        for (int p = threadIdx.x; p < P; p += MS_THREADS) {
            fc[p] = -1;
#pragma unroll
            for (int d = 0; d < 3; ++d) pts[3 * (size_t)p + d] = __uint_as_float(0x7fc00000u);
        }
        return;
    }
    if (in_lds) place_points(mesh, T, tab, area, P, seed_lo, seed_hi, draw, g, uni, pts, fc);
    else place_points(mesh, T, cdf_ws + t0, area, P, seed_lo, seed_hi, draw, g, uni, pts, fc);
}

}  // namespace bg

extern "C" int bg_mesh_sample(const float* tri, const int* tri_off, int M, int P, unsigned long long seed, unsigned draw_id,
                              long long first_mesh, const double* uniforms, double* cdf_ws, float* points, int* face, double* area,
                              bg_stream_t stream) {
    BG_REQUIRE(M >= 0 && P > 0 && first_mesh >= 0, BG_E_SHAPE, "bg_mesh_sample: need M >= 0, P >= 1, first_mesh >= 0 (M=%d P=%d first_mesh=%lld)",
               M, P, first_mesh);
    if (M == 0) return 0;
    BG_REQUIRE(tri && tri_off && cdf_ws, BG_E_ARG, "bg_mesh_sample: null input (tri, tri_off or cdf_ws)");
    BG_REQUIRE(points && face && area, BG_E_ARG, "bg_mesh_sample: null output (points, face or area)");
    BG_REQUIRE(P <= 0x7fffffff / 3, BG_E_SHAPE, "bg_mesh_sample: too many points per mesh (P=%d)", P);
    bg::ProfScope prof(bg::PK_MISC, 0.0, 28.0 * (double)M * P, (hipStream_t)stream);
    hipLaunchKernelGGL(bg::mesh_sample_kernel, dim3(M), dim3(bg::MS_THREADS), 0, (hipStream_t)stream, tri, tri_off, P, (uint32_t)seed,
                       (uint32_t)(seed >> 32), draw_id, first_mesh, uniforms, cdf_ws, points, face, area);
    return bg::launch_status("bg_mesh_sample");
}
