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

}  // namespace
