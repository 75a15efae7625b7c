// The marching-tetrahedra tables of the two triangle kernels - tsdf_mesh_triangles_kernel of tsdf_fusion.hip (the dense volume) and
// tsdf_sparse_mesh_triangles_kernel of tsdf_sparse.hip (the block-sparse one) -, stated once.  include/monorec_hip.h has the rules.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tsdf_common.h"

namespace {

// Triangles of an even tetrahedron per case (bit i: corner c_i inside): bits 0-3 the count, then a nibble per vertex naming the
// tetrahedron's edge 0 E01, 1 E12, 2 E23, 3 E02, 4 E13, 5 E03 - the table of include/monorec_hip.h.  An odd tetrahedron swaps the
// last two vertices of every triangle.
constexpr unsigned TET_CASES[16] = {0x00000000u, 0x00005301u, 0x00001401u, 0x04515312u, 0x00002131u, 0x05202102u, 0x03202402u, 0x00002451u,
                                     0x00004251u, 0x04202302u, 0x01202502u, 0x00001231u, 0x03515412u, 0x00004101u, 0x00003501u, 0x00000000u};
// the six permutations (a, b, c), the even ones first, two bits per axis
constexpr unsigned TET_PERMS[6] = {0u | 1u << 2 | 2u << 4, 1u | 2u << 2 | 0u << 4, 2u | 0u << 2 | 1u << 4,
                                    0u | 2u << 2 | 1u << 4, 2u | 1u << 2 | 0u << 4, 1u | 0u << 2 | 2u << 4};

// the cases of the six tetrahedra of the cube at `at` of a block of codes with row stride sx and slice stride sxy, four bits each; 0
// where a corner is unseen
__device__ __forceinline__ unsigned cube_cases(const uint8_t* code, int at, int sx, int sxy) {
    const int unit[3] = {1, sx, sxy};
    const unsigned c0 = code[at], c3 = code[at + 1 + sx + sxy];
    if (!(c0 & c3 & SEEN)) return 0u;
    unsigned cases = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const unsigned perm = TET_PERMS[t];
        const int a1 = at + unit[perm & 3u];
        const unsigned c1 = code[a1], c2 = code[a1 + unit[(perm >> 2) & 3u]];
        if (!(c1 & c2 & SEEN)) continue;
        cases |= (((c0 & NEG) >> 1) | (c1 & NEG) | ((c2 & NEG) << 1) | ((c3 & NEG) << 2)) << (4 * t);
    }
    return cases;
}

// ---- vertex normals and the clustered level of detail, of both volumes (include/monorec_hip.h has the rules) ------------------------

constexpr unsigned EDGE_ALONG[7] = {1u, 2u, 4u, 3u, 5u, 6u, 7u};             // bit k: the edge of that type advances along axis k

// The record x y z red green blue of the vertex on edge e of the voxel at p, between tsdf tv and tn and the packed colours cv and cn of
// its two ends: the vertex kernels' arithmetic.  Returns s.
__device__ __forceinline__ float edge_record(float tv, float tn, const float p[3], int e, float voxel, unsigned cv, unsigned cn, float* r) {
    const float s = tv / (tv - tn);
    const float step = s * voxel;
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = (EDGE_ALONG[e] >> k) & 1u ? p[k] + step : p[k];
    write_colour(r, cv, cn, s);
    return s;
}

// g_i = tsdf(v + e_i) - tsdf(v - e_i) of the seen voxel v = (x, y, z) with tsdf tv; a neighbour that is not seen counts as v itself.
// sample(x, y, z, t): is that voxel inside the volume, stored and seen?  Then t is its tsdf.  The coordinates are the kernel's own.
template <class Sample>
__device__ __forceinline__ void voxel_gradient(const Sample& sample, int x, int y, int z, float tv, float g[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int dx = i == 0, dy = i == 1, dz = i == 2;
        float hi = tv, lo = tv, t;
        if (sample(x + dx, y + dy, z + dz, t)) hi = t;
        if (sample(x - dx, y - dy, z - dz, t)) lo = t;
        g[i] = hi - lo;
    }
}

// the unit normal (or 0 0 0) of the vertex at parameter s on edge e of voxel (x, y, z): tv and tn are the tsdf of the edge's two ends
template <class Sample>
__device__ __forceinline__ void vertex_normal(const Sample& sample, int x, int y, int z, float tv, int e, float tn, float s, float n[3]) {
    float ga[3], gb[3];
    const unsigned along = EDGE_ALONG[e];
    voxel_gradient(sample, x, y, z, tv, ga);
    voxel_gradient(sample, x + (int)(along & 1u), y + (int)((along >> 1) & 1u), z + (int)(along >> 2), tn, gb);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = ga[i] + s * (gb[i] - ga[i]);
    const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) n[i] = len > 0.0f ? n[i] / len : 0.0f;
}

// A cluster of c^3 voxels, c = 1 << sh, is summed in RUNS of 8 voxels: voxel i of the cluster in the order z outermost, then y, x
// fastest - (dx, dy, dz) = (i % c, (i / c) % c, i / c^2) - belongs to run i / 8, so a cluster of 2^3 is one run, one of 4^3 eight runs
// of two rows, one of 8^3 sixty-four runs of one row.  One lane sums one run, one lane adds a cluster's run sums in the order of the
// runs: a tree of a fixed shape.
constexpr int RUN = 8;

// the place of voxel i of the cluster whose first voxel is staged at at0 (row stride sx, slice stride sxy)
__device__ __forceinline__ int cluster_voxel_at(int at0, int sx, int sxy, int sh, int i) {
    const int c1 = (1 << sh) - 1;
    return at0 + (i >> (2 * sh)) * sxy + ((i >> sh) & c1) * sx + (i & c1);
}

// does a voxel of run `run` of that cluster own a vertex?
__device__ __forceinline__ int run_owns(const uint8_t* s_mask, int at0, int sx, int sxy, int sh, int run) {
    unsigned any = 0;
#pragma unroll
    for (int j = 0; j < RUN; ++j) any |= s_mask[cluster_voxel_at(at0, sx, sxy, sh, run * RUN + j)];
    return any != 0;
}

// The sums of one run, by ONE lane: the records (and with NORMALS the unit normals) of the vertices its voxels own, summed from 0.0f in
// fp32 in the order of the voxels, within a voxel the edges 0 .. 6, into sum[0 .. 6) (and [6 .. 9)); returns their count.
// vertex(dx, dy, dz, at, e, r): the record r[0 .. 6) and the normal r[6 .. 9) of the vertex on edge e of the cluster's voxel
// (dx, dy, dz), staged at `at`.
template <bool NORMALS, class Vertex>
__device__ __forceinline__ int run_sum(const uint8_t* s_mask, int at0, int sx, int sxy, int sh, int run, float* sum, const Vertex& vertex) {
    constexpr int N = NORMALS ? 9 : 6;
#pragma unroll
    for (int k = 0; k < N; ++k) sum[k] = 0.0f;
    int count = 0;
    const int c1 = (1 << sh) - 1;
    for (int j = 0; j < RUN; ++j) {
        const int i = run * RUN + j;
        const int at = cluster_voxel_at(at0, sx, sxy, sh, i);
        const unsigned mask = s_mask[at];
        if (!mask) continue;
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            if (!(mask & (1u << e))) continue;
            float r[9];
            vertex(i & c1, (i >> sh) & c1, i >> (2 * sh), at, e, r);
#pragma unroll
            for (int k = 0; k < N; ++k) sum[k] += r[k];
            ++count;
        }
    }
    return count;
}

// The vertex of a cluster from the sums of its `runs` runs, by ONE lane: part[k * stride + r] is sum k of run r, k = N the run's count
// as a float.  total_k starts at 0.0f and takes the runs in order; position and colour are total_k / count, the normal is its total
// divided by its length (or 0 0 0).  The cluster owns at least one vertex.  (A run without a vertex adds 0.0f, which changes nothing.)
template <bool NORMALS>
__device__ __forceinline__ void cluster_combine(const float* part, int stride, int runs, float* out) {
    constexpr int N = NORMALS ? 9 : 6;
    float total[N + 1];
#pragma unroll
    for (int k = 0; k <= N; ++k) total[k] = 0.0f;
    for (int r = 0; r < runs; ++r) {
#pragma unroll
        for (int k = 0; k <= N; ++k) total[k] += part[k * stride + r];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = total[k] / total[N];
    if constexpr (NORMALS) {
        const float len = sqrtf((total[6] * total[6] + total[7] * total[7]) + total[8] * total[8]);
#pragma unroll
        for (int k = 6; k < 9; ++k) out[k] = len > 0.0f ? total[k] / len : 0.0f;
    }
}

// The triangles of one cube after clustering.  cid(dx, dy, dz): the cluster (its index in cluster_base) of the cube's corner at that
// step from its base; every triangle of the cube's tetrahedra whose three owner voxels lie in three different clusters goes to
// emit(a, b, c), those three clusters in the triangle's winding.  The owners are the corners c0, c1, c2 of the tetrahedron.
template <class Cid, class Emit>
__device__ __forceinline__ void cluster_cube_triangles(unsigned cases, const Cid& cid, const Emit& emit) {
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        unsigned word = TET_CASES[(cases >> (4 * t)) & 15u];
        const int count = (int)(word & 15u);
        if (!count) continue;
        const unsigned perm = TET_PERMS[t];
        const int pa = perm & 3u, pb = (perm >> 2) & 3u;
        const int x1 = pa == 0, y1 = pa == 1, z1 = pa == 2;
        const int id0 = cid(0, 0, 0), id1 = cid(x1, y1, z1), id2 = cid(x1 + (pb == 0), y1 + (pb == 1), z1 + (pb == 2));
        word >>= 4;
        for (int n = 0; n < count; ++n, word >>= 12) {
            int v[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const unsigned own = (0x124u >> (2u * ((word >> (4 * k)) & 15u))) & 3u;      // E01 E12 E23 E02 E13 E03: c0 c1 c2 c0 c1 c0
                v[k] = own == 0 ? id0 : own == 1 ? id1 : id2;
            }
            if (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]) continue;
            const bool odd = t >= 3;
            emit(v[0], odd ? v[2] : v[1], odd ? v[1] : v[2]);
        }
    }
}

// cell = 2, 4 or 8 as a shift, or -1
inline int cluster_shift(int cell) { return cell == 2 ? 1 : cell == 4 ? 2 : cell == 8 ? 3 : -1; }

}  // namespace
