// Training batches of the reference's dataset.py on the device: what its DataLoader workers build one CAD at a
// time in numpy -- rotation augmentation of grids and boxes, recomputed boxes, "mating duplication" of edges through faceEdge_adj, the
// per-face and per-CAD shuffles, pad_repeat / pad_zero, masks, sorted edge corners -- and the admission filter of load_data.
//
//   bg_cad_filter               one workgroup per record: the all-pairs "same box" test of filter_data (order-free, see brepgen_hip.h)
//   bg_batch_plan               one workgroup per CAD of the batch: draws -> permutations -> the SOURCE ROW of every output slot
//                               (face_src / edge_src, -1 = zero padding), the rotation code and the three max-abs scales.  Stable
//                               argsort of at most a few dozen keys = counting the smaller ones; everything stays in LDS.
//   bg_batch_gather             one launch, three block ranges: (A) one workgroup per 12 288-byte face grid, (B) 32 edge grids of 384
//                               bytes per workgroup, 8 lanes each, (C) one thread per box / corner pair / mask entry.  A lane moves
//                               48 bytes = 4 points as three 16-byte accesses, so the augmented path (a signed permutation of the
//                               coordinates, in registers) and the plain copy are the same memory pattern.  Every output element is
//                               written: padding is +0.0, masks are 0 / 1.
//   bg_points_rotate_normalize  the VAE datasets' rotate_point_cloud, one wave per item, the points in registers, fp64 throughout.
//
// Device draws are Philox blocks keyed by the run's seed whose counters hold the record's GLOBAL number, the face, the element and the
// draw id (domain tags 0xDA7A / 0xDA7B) -- never the position in the batch.
#include "bg_common.h"
#include "philox.h"

namespace bg {

constexpr int BT_THREADS = 256;
constexpr uint32_t BT_TAG = 0xDA7A0000u;           // Philox domain tag of bg_batch_plan (low half-word: 0 = faces / CAD, f + 1 = edges of face f)
constexpr uint32_t PT_TAG = 0xDA7B0000u;           // ... of bg_points_rotate_normalize (low half-word: bits 32..47 of the item number)
constexpr uint32_t BT_CAD_ELEM = 0xFFFFFFFFu;      // element word of the per-CAD block (augment decision + quarter turns)
constexpr int BT_MAX_FACE = 512, BT_MAX_SLOTS = 4096;      // LDS of the plan: (5 S + 3 S E) * 4 bytes <= 59 392
constexpr int FACE_FLOATS = 32 * 32 * 3, EDGE_FLOATS = 32 * 3;
constexpr int UNIT = 12;                            // floats a lane moves: 4 points = 3 x 16 bytes
constexpr int EDGE_LANES = EDGE_FLOATS / UNIT;      // 8 lanes per edge grid
constexpr int EDGE_ROWS_PER_WG = BT_THREADS / EDGE_LANES;
static_assert(FACE_FLOATS == UNIT * BT_THREADS, "one workgroup moves one face grid");

// rotation by q quarter turns in the plane (a, b):  a' = cos a - sin b,  b' = sin a + cos b  with (cos, sin) in {(0,1), (-1,0), (0,-1)}
template <typename T> __device__ __forceinline__ void quarter(T& a, T& b, int q) {
    const T a0 = a, b0 = b;
    if (q == 1) { a = -b0; b = a0; }
    else if (q == 2) { a = -a0; b = -b0; }
    else if (q == 3) { a = b0; b = -a0; }
}
// the composed rotation about x, then y, then z (utils.py rotate_axis / rotate_point_cloud matrices at 90 / 180 / 270 degrees) as the
// signed permutation it is; `+ 0` turns a negated zero into +0.0, which is what the reference's sum of products gives
template <typename T> __device__ __forceinline__ void rot3(T& x, T& y, T& z, int code) {
    quarter(y, z, code & 3);
    quarter(z, x, (code >> 2) & 3);
    quarter(x, y, (code >> 4) & 3);
    x = x + (T)0; y = y + (T)0; z = z + (T)0;
}
__device__ __forceinline__ int turn_of(uint32_t w) { return 1 + (int)(((uint64_t)w * 3u) >> 32); }      // uniform over {1, 2, 3}
__device__ __forceinline__ int clamp_turn(int t) { return t < 1 ? 1 : (t > 3 ? 3 : t); }

// utils.py pad_repeat(n -> L): the source of slot i
__device__ __forceinline__ int pad_repeat_src(int i, int n, int L) {
    const int r = L / n, sep = L - r * n, cut = sep * (r + 1);
    return i < cut ? i / (r + 1) : sep + (i - cut) / r;
}
// position of element i in the stable argsort of key[0 .. n)
__device__ __forceinline__ int stable_rank(const uint32_t* key, int n, int i) {
    const uint32_t k = key[i];
    int r = 0;
    for (int j = 0; j < n; ++j) r += (key[j] < k || (key[j] == k && j < i)) ? 1 : 0;
    return r;
}

struct Span { int f0, F, e0, Ne; };       // a record's faces and edges, clamped to the store
__device__ __forceinline__ Span record_span(const bg_cad_store& st, int rec) {
    Span s = {0, 0, 0, 0};
    if (rec < 0 || rec >= st.n_records) return s;
    const int f0 = st.face_off[rec], f1 = st.face_off[rec + 1], e0 = st.edge_off[rec], e1 = st.edge_off[rec + 1];
    if (f0 >= 0 && f1 >= f0 && f1 <= st.n_faces) { s.f0 = f0; s.F = f1 - f0; }
    if (e0 >= 0 && e1 >= e0 && e1 <= st.n_edges) { s.e0 = e0; s.Ne = e1 - e0; }
    return s;
}
// adjacency list of GLOBAL face g: start and length, (0, 0) if it leaves the store
__device__ __forceinline__ int2 adj_span(const bg_cad_store& st, int g) {
    const int a0 = st.adj_off[g], a1 = st.adj_off[g + 1];
    return (a0 >= 0 && a1 >= a0 && a1 <= st.n_adj) ? make_int2(a0, a1 - a0) : make_int2(0, 0);
}

// ---- admission filter ------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool same_box(const float* a, const float* b, float sc, float thr) {
    bool same = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) same = same && (fabsf(a[k] * sc - b[k] * sc) < thr);      // a NaN is never "the same", as in numpy
    return same;
}

__global__ __launch_bounds__(BT_THREADS) void cad_filter_kernel(bg_cad_store st, int S, int E, float sc, float thr, uint8_t* __restrict__ keep) {
    const int rec = blockIdx.x, tid = threadIdx.x;
    const Span sp = record_span(st, rec);
    int bad = (tid == 0 && sp.F > S) ? 1 : 0;
    if (sp.F <= S)
        for (int f = tid; f < sp.F; f += BT_THREADS) {
            const int d = st.adj_off[sp.f0 + f + 1] - st.adj_off[sp.f0 + f];
            if (d > E || d <= 0 || adj_span(st, sp.f0 + f).y != d) bad = 1;
        }
    if (__syncthreads_or(bad)) {
        if (tid == 0) keep[rec] = 0;
        return;
    }
    const int F = sp.F;                       // <= S, every degree in 1 .. E from here on
    for (int p = tid; p < F * F; p += BT_THREADS) {
        const int i = p / F, j = p - i * F;
        if (i < j && same_box(st.surf_pos + (size_t)(sp.f0 + i) * 6, st.surf_pos + (size_t)(sp.f0 + j) * 6, sc, thr)) bad = 1;
    }
    const int EE = E * E;
    for (int p = tid; p < F * EE; p += BT_THREADS) {
        const int f = p / EE, q = p - f * EE, i = q / E, j = q - i * E;
        const int2 ad = adj_span(st, sp.f0 + f);
        if (i < j && j < ad.y) {
            const int ei = st.adj_idx[ad.x + i], ej = st.adj_idx[ad.x + j];
            if (ei < 0 || ei >= sp.Ne || ej < 0 || ej >= sp.Ne) bad = 1;                 // an edge id outside the record: not admitted
            else if (same_box(st.edge_pos + (size_t)(sp.e0 + ei) * 6, st.edge_pos + (size_t)(sp.e0 + ej) * 6, sc, thr)) bad = 1;
        }
    }
    const int any = __syncthreads_or(bad);
    if (tid == 0) keep[rec] = any ? 0 : 1;
}

// ---- plan ------------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(BT_THREADS) void batch_plan_kernel(bg_cad_store st, const int* __restrict__ idx, int kind, int S, int E, int aug,
                                                                uint32_t seed_lo, uint32_t seed_hi, uint32_t draw, bg_batch_draws dr, int have_draws,
                                                                int* __restrict__ face_src, int* __restrict__ edge_src, int* __restrict__ rot,
                                                                double* __restrict__ scale) {
    extern __shared__ uint32_t lds[];
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x, SE = S * E;
    uint32_t* fkey1 = lds;                     // [S] first face keys
    uint32_t* fkey2 = lds + S;                 // [S] second face keys (SurfPos)
    int* ford = (int*)(lds + 2 * S);           // [S] local face of shuffled position i
    int* ffin = (int*)(lds + 3 * S);           // [S] SurfPos: local face of final slot i
    int* fdeg = (int*)(lds + 4 * S);           // [S] degree of LOCAL face f, clamped to E
    uint32_t* ekey1 = lds + 5 * S;             // [S, E] keys by (local face, position in its adjacency list); reused as efin
    uint32_t* ekey2 = ekey1 + SE;
    int* eord = (int*)(ekey2 + SE);            // [S, E] adjacency position of shuffled position j
    int* efin = (int*)ekey1;                   // [S, E] EdgePos: adjacency position of final slot j

    const int rec = idx[b];
    const Span sp = record_span(st, rec);
    const int F = min(sp.F, S);                // a record too large for the batch is the caller's error (dataset.py raises); stay in bounds

    // the three scales: fp32 max-abs (exact), widened
    float m0 = 0.f, m1 = 0.f, m2 = 0.f;
    for (int i = tid; i < sp.F * 6; i += BT_THREADS) m0 = fmaxf(m0, fabsf(st.surf_pos[(size_t)sp.f0 * 6 + i]));
    for (int i = tid; i < sp.Ne * 6; i += BT_THREADS) {
        m1 = fmaxf(m1, fabsf(st.edge_pos[(size_t)sp.e0 * 6 + i]));
        m2 = fmaxf(m2, fabsf(st.corner_wcs[(size_t)sp.e0 * 6 + i]));
    }
    m0 = block_max(m0, red);
    m1 = block_max(m1, red);
    m2 = block_max(m2, red);
    if (tid == 0) {
        scale[3 * (size_t)b] = (double)m0;
        scale[3 * (size_t)b + 1] = (double)m1;
        scale[3 * (size_t)b + 2] = (double)m2;
        double u;
        int q[3];
        if (have_draws) {
            u = dr.u ? dr.u[b] : 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = dr.turns ? clamp_turn(dr.turns[3 * (size_t)b + k]) : 1;
        } else {
            uint32_t c[4] = {BT_CAD_ELEM, (uint32_t)rec, draw, BT_TAG};
            philox4x32_10(c, seed_lo, seed_hi);
            u = (double)u01(c[0]);
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = turn_of(c[1 + k]);
        }
        rot[b] = (aug && u > 0.5) ? (q[0] | (q[1] << 2) | (q[2] << 4)) : 0;
    }

    // face keys and degrees
    for (int i = tid; i < S; i += BT_THREADS) {
        uint32_t k1, k2;
        if (have_draws) {
            k1 = (dr.face_key1 && i < F) ? dr.face_key1[(size_t)b * S + i] : 0u;
            k2 = (dr.face_key2 && kind == BG_SURFPOS) ? dr.face_key2[(size_t)b * S + i] : 0u;
        } else {
            uint32_t c[4] = {(uint32_t)i, (uint32_t)rec, draw, BT_TAG};
            philox4x32_10(c, seed_lo, seed_hi);
            k1 = c[0]; k2 = c[1];
        }
        fkey1[i] = k1; fkey2[i] = k2;
        fdeg[i] = (i < F && kind >= BG_EDGEPOS) ? min(adj_span(st, sp.f0 + i).y, E) : 0;
    }
    __syncthreads();
    for (int i = tid; i < F; i += BT_THREADS) ford[stable_rank(fkey1, F, i)] = i;
    __syncthreads();
    if (kind == BG_SURFPOS) {
        if (F > 0)
            for (int i = tid; i < S; i += BT_THREADS) ffin[stable_rank(fkey2, S, i)] = ford[pad_repeat_src(i, F, S)];
        __syncthreads();
        for (int i = tid; i < S; i += BT_THREADS) face_src[(size_t)b * S + i] = F > 0 ? sp.f0 + ffin[i] : -1;
        return;
    }
    for (int i = tid; i < S; i += BT_THREADS) face_src[(size_t)b * S + i] = i < F ? sp.f0 + ford[i] : -1;
    if (kind == BG_SURFZ) return;

    // edge keys, by (local face f, position j in its adjacency list)
    for (int t = tid; t < F * E; t += BT_THREADS) {
        const int f = t / E, j = t - f * E;
        uint32_t k1, k2;
        if (have_draws) {
            k1 = (dr.edge_key1 && j < fdeg[f]) ? dr.edge_key1[((size_t)b * S + f) * E + j] : 0u;
            k2 = (dr.edge_key2 && kind == BG_EDGEPOS) ? dr.edge_key2[((size_t)b * S + f) * E + j] : 0u;
        } else {
            uint32_t c[4] = {(uint32_t)j, (uint32_t)rec, draw, BT_TAG | (uint32_t)(f + 1)};
            philox4x32_10(c, seed_lo, seed_hi);
            k1 = c[0]; k2 = c[1];
        }
        ekey1[t] = k1; ekey2[t] = k2;
    }
    __syncthreads();
    for (int t = tid; t < F * E; t += BT_THREADS) {
        const int f = t / E, j = t - f * E;
        if (j < fdeg[f]) eord[f * E + stable_rank(ekey1 + f * E, fdeg[f], j)] = j;
    }
    __syncthreads();                           // ekey1 is dead from here: efin takes its place
    if (kind == BG_EDGEPOS) {
        int r2[(BT_MAX_SLOTS + BT_THREADS - 1) / BT_THREADS], src[(BT_MAX_SLOTS + BT_THREADS - 1) / BT_THREADS];
#pragma unroll
        for (int it = 0; it < (BT_MAX_SLOTS + BT_THREADS - 1) / BT_THREADS; ++it) {
            const int t = it * BT_THREADS + tid;
            r2[it] = -1;
            if (t < F * E) {
                const int f = t / E, j = t - f * E, d = fdeg[f];
                if (d > 0) {
                    r2[it] = f * E + stable_rank(ekey2 + f * E, E, j);
                    src[it] = eord[f * E + pad_repeat_src(j, d, E)];
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < (BT_MAX_SLOTS + BT_THREADS - 1) / BT_THREADS; ++it)
            if (r2[it] >= 0) efin[r2[it]] = src[it];
        __syncthreads();
    }
    for (int t = tid; t < SE; t += BT_THREADS) {
        const int i = t / E, j = t - i * E;
        int out = -1;
        if (i < F) {
            const int f = ford[i], d = fdeg[f];
            const int pos = kind == BG_EDGEPOS ? (d > 0 ? efin[f * E + j] : -1) : (j < d ? eord[f * E + j] : -1);
            if (pos >= 0) {
                const int loc = st.adj_idx[adj_span(st, sp.f0 + f).x + pos];
                if (loc >= 0 && loc < sp.Ne) out = sp.e0 + loc;
            }
        }
        edge_src[(size_t)b * SE + t] = out;
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------------

struct GatherArgs {
    bg_cad_store st;
    bg_batch_out out;
    const int* face_src; const int* edge_src; const int* rot; const double* scale;
    int kind, B, S, E;
    float bs;
    int blocks_face, blocks_edge;              // block ranges (A) and (B); the rest is (C)
};

// 12 floats = 4 points of a grid row: src < 0 writes +0.0, code != 0 rotates
__device__ __forceinline__ void move_unit(const float* __restrict__ src_row, float* __restrict__ dst_row, int unit, bool live, int code) {
    float4 v[3];
    if (live) {
        const float4* s = reinterpret_cast<const float4*>(src_row) + unit * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = s[k];
        if (code) {
            float* p = reinterpret_cast<float*>(v);
#pragma unroll
            for (int k = 0; k < 4; ++k) rot3(p[3 * k], p[3 * k + 1], p[3 * k + 2], code);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4* d = reinterpret_cast<float4*>(dst_row) + unit * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = v[k];
}

// a box [lo, hi]: plain x * bs in fp32, or rotated, normalised, re-boxed and scaled in fp64 and rounded once
__device__ __forceinline__ void box_out(const float* __restrict__ in, float* __restrict__ out, int code, double scale, float bs) {
    if (!code) {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = in[k] * bs;
        return;
    }
    double a[3] = {(double)in[0], (double)in[1], (double)in[2]}, c[3] = {(double)in[3], (double)in[4], (double)in[5]};
    rot3(a[0], a[1], a[2], code);
    rot3(c[0], c[1], c[2], code);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double p = a[k] / scale, q = c[k] / scale;
        out[k] = (float)(fmin(p, q) * (double)bs);
        out[3 + k] = (float)(fmax(p, q) * (double)bs);
    }
}
// an edge's corner pair, ordered lexicographically by (x, y, z) on the scaled values (np.lexsort; a tie keeps the order)
template <typename T> __device__ __forceinline__ bool second_first(const T* p) {
    if (p[3] != p[0]) return p[3] < p[0];
    if (p[4] != p[1]) return p[4] < p[1];
    return p[5] < p[2];
}
__device__ __forceinline__ void corners_out(const float* __restrict__ in, float* __restrict__ out, int code, double scale, float bs) {
    if (!code) {
        float p[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) p[k] = in[k] * bs;
        const int o = second_first(p) ? 3 : 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { out[k] = p[o + k]; out[3 + k] = p[3 - o + k]; }
        return;
    }
    double p[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = (double)in[k];
    rot3(p[0], p[1], p[2], code);
    rot3(p[3], p[4], p[5], code);
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = p[k] / scale * (double)bs;
    const int o = second_first(p) ? 3 : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) { out[k] = (float)p[o + k]; out[3 + k] = (float)p[3 - o + k]; }
}

__global__ __launch_bounds__(BT_THREADS) void batch_gather_kernel(GatherArgs g) {
    const int tid = threadIdx.x, S = g.S, E = g.E;
    int blk = blockIdx.x;
    if (blk < g.blocks_face) {                                        // (A) face grid `blk` of [B, S]
        const int src = g.face_src[blk], code = g.rot[blk / S];
        const bool live = src >= 0 && src < g.st.n_faces;
        move_unit(g.st.surf_ncs + (size_t)(live ? src : 0) * FACE_FLOATS, g.out.surf_ncs + (size_t)blk * FACE_FLOATS, tid, live, code);
        return;
    }
    blk -= g.blocks_face;
    if (blk < g.blocks_edge) {                                        // (B) 32 edge grids of [B, S, E]
        const long long row = (long long)blk * EDGE_ROWS_PER_WG + tid / EDGE_LANES;
        if (row >= (long long)g.B * S * E) return;
        const int src = g.edge_src[row], code = g.rot[row / ((long long)S * E)];
        const bool live = src >= 0 && src < g.st.n_edges;
        move_unit(g.st.edge_ncs + (size_t)(live ? src : 0) * EDGE_FLOATS, g.out.edge_ncs + (size_t)row * EDGE_FLOATS, tid % EDGE_LANES, live, code);
        return;
    }
    blk -= g.blocks_edge;                                             // (C) boxes, corner pairs, masks
    const long long n_face = (long long)g.B * S, n_edge = g.kind >= BG_EDGEPOS ? n_face * E : 0;
    long long t = (long long)blk * BT_THREADS + tid;
    if (t < n_face) {
        const int src = g.face_src[t], b = (int)(t / S);
        const bool live = src >= 0 && src < g.st.n_faces;
        float* o = g.out.surf_pos + (size_t)t * 6;
        if (live) box_out(g.st.surf_pos + (size_t)src * 6, o, g.rot[b], g.scale[3 * (size_t)b], g.bs);
        else
#pragma unroll
            for (int k = 0; k < 6; ++k) o[k] = 0.f;
        if (g.kind == BG_SURFZ || g.kind == BG_EDGEPOS) g.out.surf_mask[t] = live ? 0 : 1;
        return;
    }
    t -= n_face;
    if (t >= n_edge) return;
    const int src = g.edge_src[t], b = (int)(t / ((long long)S * E));
    const bool live = src >= 0 && src < g.st.n_edges;
    const int code = g.rot[b];
    float* o = g.out.edge_pos + (size_t)t * 6;
    if (live) box_out(g.st.edge_pos + (size_t)src * 6, o, code, g.scale[3 * (size_t)b + 1], g.bs);
    else
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = 0.f;
    if (g.kind == BG_EDGEZ) {
        float* v = g.out.vertex_pos + (size_t)t * 6;
        if (live) corners_out(g.st.corner_wcs + (size_t)src * 6, v, code, g.scale[3 * (size_t)b + 2], g.bs);
        else
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = 0.f;
        g.out.edge_mask[t] = live ? 0 : 1;
    }
}

// ---- point augmentation ----------------------------------------------------------------------------------------------------------------

constexpr int PT_MAX = 1024, PT_PER_LANE = PT_MAX / WAVE;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(BT_THREADS) void points_kernel(const float* __restrict__ x, long long M, int P, int aug, uint32_t seed_lo,
                                                            uint32_t seed_hi, uint32_t draw, long long first_item, const double* __restrict__ u_in,
                                                            const int* __restrict__ turns, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * (BT_THREADS / WAVE) + (threadIdx.x >> 6);
    if (item >= M) return;                     // whole waves leave; no workgroup barrier below
    double u;
    int q[3];
    if (u_in) {
        u = u_in[item];
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = turns ? clamp_turn(turns[3 * item + k]) : 1;
    } else {
        const unsigned long long gi = (unsigned long long)(first_item + item);
        uint32_t c[4] = {0u, (uint32_t)gi, draw, PT_TAG | (uint32_t)((gi >> 32) & 0xFFFFu)};
        philox4x32_10(c, seed_lo, seed_hi);
        u = (double)u01(c[0]);
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = turn_of(c[1 + k]);
    }
    const float* src = x + (size_t)item * P * 3;
    float* dst = out + (size_t)item * P * 3;
    if (!(aug && u > 0.5)) {
        for (int i = lane; i < P * 3; i += WAVE) dst[i] = src[i];
        return;
    }
    double p[PT_PER_LANE][3];
#pragma unroll
    for (int k = 0; k < PT_PER_LANE; ++k) {
        const int i = lane + k * WAVE;
#pragma unroll
        for (int d = 0; d < 3; ++d) p[k][d] = i < P ? (double)src[3 * (size_t)i + d] : 0.0;
    }
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < PT_PER_LANE; ++k)
            if (lane + k * WAVE < P) { s[0] += p[k][0]; s[1] += p[k][1]; s[2] += p[k][2]; }
        double mean[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) mean[d] = wave_sum_d(s[d]) / (double)P;
        double mx = 0.0;
#pragma unroll
        for (int k = 0; k < PT_PER_LANE; ++k) {
            double c[3] = {p[k][0] - mean[0], p[k][1] - mean[1], p[k][2] - mean[2]};
            if (axis == 0) quarter(c[1], c[2], q[0]);
            else if (axis == 1) quarter(c[2], c[0], q[1]);
            else quarter(c[0], c[1], q[2]);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                p[k][d] = c[d] + mean[d];
                if (lane + k * WAVE < P) mx = fmax(mx, fabs(p[k][d]));
            }
        }
        mx = wave_max_d(mx);
#pragma unroll
        for (int k = 0; k < PT_PER_LANE; ++k)
#pragma unroll
            for (int d = 0; d < 3; ++d) p[k][d] = p[k][d] / mx;
    }
#pragma unroll
    for (int k = 0; k < PT_PER_LANE; ++k) {
        const int i = lane + k * WAVE;
        if (i < P)
#pragma unroll
            for (int d = 0; d < 3; ++d) dst[3 * (size_t)i + d] = (float)p[k][d];
    }
}

static int check_store(const bg_cad_store* st, const char* who) {
    BG_REQUIRE(st, BG_E_ARG, "%s: null store", who);
    BG_REQUIRE(st->n_records >= 0 && st->n_faces >= 0 && st->n_edges >= 0 && st->n_adj >= 0, BG_E_SHAPE,
               "%s: negative store size (records %d, faces %d, edges %d, adjacency %d)", who, st->n_records, st->n_faces, st->n_edges, st->n_adj);
    BG_REQUIRE(st->surf_ncs && st->surf_pos && st->edge_ncs && st->edge_pos && st->corner_wcs && st->face_off && st->edge_off &&
                   st->adj_off && st->adj_idx, BG_E_ARG, "%s: null array in the store", who);
    BG_REQUIRE(((uintptr_t)st->surf_ncs | (uintptr_t)st->edge_ncs) % 16 == 0, BG_E_ALIGN, "%s: surf_ncs / edge_ncs must be 16-byte aligned", who);
    return 0;
}
static int check_shape(int kind, int B, int S, int E, const char* who) {
    BG_REQUIRE(kind >= BG_SURFPOS && kind <= BG_EDGEZ, BG_E_ARG, "%s: kind %d is none of SurfPos, SurfZ, EdgePos, EdgeZ", who, kind);
    BG_REQUIRE(B >= 0 && S >= 1 && E >= 1 && S <= BT_MAX_FACE && (long long)S * E <= BT_MAX_SLOTS, BG_E_SHAPE,
               "%s: need B >= 0, 1 <= max_face <= %d, max_edge >= 1, max_face * max_edge <= %d (B=%d max_face=%d max_edge=%d)", who,
               BT_MAX_FACE, BT_MAX_SLOTS, B, S, E);
    BG_REQUIRE((long long)B * S * E <= 0x7fffffffLL / 8, BG_E_SHAPE, "%s: B * max_face * max_edge = %lld is too large for one call", who,
               (long long)B * S * E);
    return 0;
}

}  // namespace bg

extern "C" int bg_cad_filter(const bg_cad_store* store, int max_face, int max_edge, float scale, double threshold, uint8_t* keep,
                             bg_stream_t stream) {
    if (int rc = bg::check_store(store, "bg_cad_filter")) return rc;
    BG_REQUIRE(max_face >= 1 && max_edge >= 1 && max_edge <= 1024, BG_E_SHAPE, "bg_cad_filter: need max_face >= 1, 1 <= max_edge <= 1024 (max_face=%d max_edge=%d)",
               max_face, max_edge);
    if (store->n_records == 0) return 0;
    BG_REQUIRE(keep, BG_E_ARG, "bg_cad_filter: null output (keep)");
    hipLaunchKernelGGL(bg::cad_filter_kernel, dim3(store->n_records), dim3(bg::BT_THREADS), 0, (hipStream_t)stream, *store, max_face, max_edge,
                       scale, (float)threshold, keep);
    return bg::launch_status("bg_cad_filter");
}

extern "C" int bg_batch_plan(const bg_cad_store* store, const int* idx, int B, int kind, int max_face, int max_edge, int aug,
                             unsigned long long seed, unsigned draw_id, const bg_batch_draws* draws, int* face_src, int* edge_src, int* rot,
                             double* scale, bg_stream_t stream) {
    if (int rc = bg::check_store(store, "bg_batch_plan")) return rc;
    if (int rc = bg::check_shape(kind, B, max_face, max_edge, "bg_batch_plan")) return rc;
    if (B == 0) return 0;
    BG_REQUIRE(idx && face_src && rot && scale, BG_E_ARG, "bg_batch_plan: null idx, face_src, rot or scale");
    BG_REQUIRE(kind < BG_EDGEPOS || edge_src, BG_E_ARG, "bg_batch_plan: null edge_src for an edge batch");
    bg_batch_draws dr = {};
    if (draws) dr = *draws;
    const size_t lds = sizeof(uint32_t) * (5 * (size_t)max_face + (kind >= BG_EDGEPOS ? 3 * (size_t)max_face * max_edge : 0));
    hipLaunchKernelGGL(bg::batch_plan_kernel, dim3(B), dim3(bg::BT_THREADS), lds, (hipStream_t)stream, *store, idx, kind, max_face, max_edge,
                       aug ? 1 : 0, (uint32_t)seed, (uint32_t)(seed >> 32), draw_id, dr, draws ? 1 : 0, face_src, edge_src, rot, scale);
    return bg::launch_status("bg_batch_plan");
}

extern "C" int bg_batch_gather(const bg_cad_store* store, int kind, int B, int max_face, int max_edge, float bbox_scaled, const int* face_src,
                               const int* edge_src, const int* rot, const double* scale, const bg_batch_out* out, bg_stream_t stream) {
    if (int rc = bg::check_store(store, "bg_batch_gather")) return rc;
    if (int rc = bg::check_shape(kind, B, max_face, max_edge, "bg_batch_gather")) return rc;
    if (B == 0) return 0;
    BG_REQUIRE(face_src && rot && scale && out, BG_E_ARG, "bg_batch_gather: null face_src, rot, scale or out");
    BG_REQUIRE(kind < BG_EDGEPOS || edge_src, BG_E_ARG, "bg_batch_gather: null edge_src for an edge batch");
    const bool need_ncs = kind != BG_SURFPOS, need_smask = kind == BG_SURFZ || kind == BG_EDGEPOS, need_epos = kind >= BG_EDGEPOS,
               need_edgez = kind == BG_EDGEZ;
    BG_REQUIRE(out->surf_pos && (!need_ncs || out->surf_ncs) && (!need_smask || out->surf_mask) && (!need_epos || out->edge_pos) &&
                   (!need_edgez || (out->edge_ncs && out->edge_mask && out->vertex_pos)), BG_E_ARG,
               "bg_batch_gather: null output tensor of kind %d", kind);
    BG_REQUIRE((!need_ncs || (uintptr_t)out->surf_ncs % 16 == 0) && (!need_edgez || (uintptr_t)out->edge_ncs % 16 == 0), BG_E_ALIGN,
               "bg_batch_gather: surf_ncs / edge_ncs outputs must be 16-byte aligned");
    bg::GatherArgs g;
    g.st = *store; g.out = *out;
    g.face_src = face_src; g.edge_src = edge_src; g.rot = rot; g.scale = scale;
    g.kind = kind; g.B = B; g.S = max_face; g.E = max_edge; g.bs = bbox_scaled;
    const long long n_face = (long long)B * max_face, n_edge = n_face * max_edge;
    g.blocks_face = need_ncs ? (int)n_face : 0;
    g.blocks_edge = need_edgez ? (int)((n_edge + bg::EDGE_ROWS_PER_WG - 1) / bg::EDGE_ROWS_PER_WG) : 0;
    const long long small = n_face + (need_epos ? n_edge : 0);
    const long long blocks = (long long)g.blocks_face + g.blocks_edge + (small + bg::BT_THREADS - 1) / bg::BT_THREADS;
    BG_REQUIRE(blocks <= 0x7fffffffLL, BG_E_SHAPE, "bg_batch_gather: %lld workgroups exceed one launch", blocks);
    const double bytes = 2.0 * 4.0 * ((need_ncs ? (double)n_face * bg::FACE_FLOATS : 0.0) + (need_edgez ? (double)n_edge * bg::EDGE_FLOATS : 0.0)) +
                         52.0 * (double)small;
    bg::ProfScope prof(bg::PK_MISC, 0.0, bytes, (hipStream_t)stream);
    hipLaunchKernelGGL(bg::batch_gather_kernel, dim3((unsigned)blocks), dim3(bg::BT_THREADS), 0, (hipStream_t)stream, g);
    return bg::launch_status("bg_batch_gather");
}

extern "C" int bg_points_rotate_normalize(const float* x, long long M, int P, int aug, unsigned long long seed, unsigned draw_id,
                                          long long first_item, const double* u, const int* turns, float* out, bg_stream_t stream) {
    BG_REQUIRE(M >= 0 && P >= 1 && P <= bg::PT_MAX && first_item >= 0, BG_E_SHAPE,
               "bg_points_rotate_normalize: need M >= 0, 1 <= P <= %d, first_item >= 0 (M=%lld P=%d first_item=%lld)", bg::PT_MAX, M, P, first_item);
    if (M == 0) return 0;
    BG_REQUIRE(x && out, BG_E_ARG, "bg_points_rotate_normalize: null x or out");
    BG_REQUIRE(!turns || u, BG_E_ARG, "bg_points_rotate_normalize: turns without u (supply both or neither)");
    const long long blocks = (M + bg::BT_THREADS / bg::WAVE - 1) / (bg::BT_THREADS / bg::WAVE);
    BG_REQUIRE(blocks <= 0x7fffffffLL, BG_E_SHAPE, "bg_points_rotate_normalize: M = %lld is too large for one call", M);
    hipLaunchKernelGGL(bg::points_kernel, dim3((unsigned)blocks), dim3(bg::BT_THREADS), 0, (hipStream_t)stream, x, M, P, aug ? 1 : 0, (uint32_t)seed,
                       (uint32_t)(seed >> 32), draw_id, first_item, u, turns, out);
    return bg::launch_status("bg_points_rotate_normalize");
}
