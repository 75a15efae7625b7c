// The block-sparse TSDF volume seen from a camera (monorec_amd/tsdf_fusion.py, SparseTSDFVolume.render): mr_tsdf_render_f32's march on
// the table and the pool of tsdf_sparse.hip, without a dense copy.  The ray, the cell of a sample, the clip, the interpolant and what a
// pixel writes are the dense kernel's (tsdf_render.h; compiled with -ffp-contract=off); the rule is in include/monorec_hip.h,
// tests/tsdf_sparse_render_ref.py restates it in numpy and the GPU tests compare bit for bit.
// B, BV, MAX_VOXELS, pool_index and the checks of table and pool (bad_sparse) are tsdf_common.h's, shared with tsdf_sparse.hip.
//
//   tsdf_sparse_render_kernel   a thread per pixel, a wave a compact 8 x 8 pixel tile, a workgroup 16 x 16 pixels of one view
//                               (blockIdx.z), as in the dense kernel: neighbouring rays walk neighbouring cells and blocks.  A sample
//                               costs one table load for the block of its cell base.  No slot there (and min_weight >= 0): the base
//                               corner is unseen, the sample is not valid, nothing else is read.  A cell whose base is not on a high
//                               face of its block (343 of 512) takes its 16 gathers from that one slot; the others look up the block of
//                               each corner.  (A jump from a sample in a block without a slot to the last sample still in it was
//                               measured and is not here: DESIGN.md section 7.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monorec_hip.h"
#include "tsdf_common.h"                     // the blocks, as tsdf_sparse.hip has them: B, BV, MAX_VOXELS, pool_index, bad_sparse
#include "tsdf_render.h"

namespace {

constexpr int MAX_BLOCKS_PER_AXIS = 1 << 27;     // 8 nb_a voxels fit an int

struct SparseRenderArgs {
    const int* table;
    const float* tsdf;
    const float* weight;
    const unsigned* colour;                      // r g b 0 per voxel or null
    int nbx, nby;
    int num_slots;                               // at most nbx * nby * nbz < 2^31
    float lim[3];                                // the largest float <= 8 nb_a - 2: the last cell base along each axis
    float inv, min_weight, t_min, step;
    int last;                                    // index of the last sample with t_k <= t_max
    int h, w, tiles_x;
    RayView v[MR_TSDF_MAX_FRAMES];
};

// the slot of block (bx, by, bz) of the table, or -1
__device__ __forceinline__ int slot_of(const SparseRenderArgs& a, int bx, int by, int bz) {
    const int s = a.table[((long long)bz * a.nby + by) * a.nbx + bx];
    return (unsigned)s < (unsigned)a.num_slots ? s : -1;
}

// The pool indices of the 8 corners of the cell at i into P, -1 for a corner in a block without a slot; s0: the slot of i's own block.
__device__ __forceinline__ void corner_indices(const SparseRenderArgs& a, const int i[3], int s0, long long P[8]) {
    if ((i[0] & 7) < 7 && (i[1] & 7) < 7 && (i[2] & 7) < 7) {                // one block holds all 8
        const long long p = s0 >= 0 ? pool_index(s0, i[0], i[1], i[2]) : -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) P[j] = s0 >= 0 ? p + (j & 1) + ((j >> 1) & 1) * B + (j >> 2) * (B * B) : -1;
        return;
    }
    const int b0[3] = {i[0] >> 3, i[1] >> 3, i[2] >> 3};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int x = i[0] + (j & 1), y = i[1] + ((j >> 1) & 1), z = i[2] + (j >> 2);
        const int bx = x >> 3, by = y >> 3, bz = z >> 3;                      // inside: x <= 8 nbx - 1, so the block is in the table
        const int s = (bx == b0[0] && by == b0[1] && bz == b0[2]) ? s0 : slot_of(a, bx, by, bz);
        P[j] = s >= 0 ? pool_index(s, x, y, z) : -1;
    }
}

// the 8 corner tsdf of an inside cell into T; false when a corner's weight is not above min_weight.  A corner without a slot: 0 and 1.
__device__ __forceinline__ bool corners_of(const SparseRenderArgs& a, const Cell& c, int s0, float T[8]) {
    long long P[8];
    corner_indices(a, c.i, s0, P);
    float W[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        W[j] = P[j] >= 0 ? a.weight[P[j]] : 0.0f;
        T[j] = P[j] >= 0 ? a.tsdf[P[j]] : 1.0f;
    }
    bool seen = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) seen = seen && (W[j] > a.min_weight);
    return seen;
}

__global__ __launch_bounds__(256) void tsdf_sparse_render_kernel(const SparseRenderArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = (blockIdx.x % a.tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
    const int v = (blockIdx.x / a.tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (u >= a.w || v >= a.h) return;
    const RayView& view = a.v[blockIdx.z];
    float o[3], e[3];
    ray_of_pixel(a, view, u, v, o, e);
    int k_lo, k_hi;
    clip_to_box(a, o, e, k_lo, k_hi);

    // With min_weight >= 0 a corner without a slot (weight 0) makes its sample not valid; below 0 it counts as seen, with tsdf 1.
    const bool unseen_is_invalid = a.min_weight >= 0.0f;
    bool prev_valid = false;
    int hit_k = -1, hit_i[3] = {0, 0, 0}, hit_slot = -1;
    float F_prev = 0.0f, F_hit = 0.0f, T[8], f[3] = {0.0f, 0.0f, 0.0f};
    for (int k = k_lo; k <= k_hi; ++k) {
        const Cell c = cell_of(a, o, e, k);
        if (!c.inside) { prev_valid = false; continue; }
        const int s0 = slot_of(a, c.i[0] >> 3, c.i[1] >> 3, c.i[2] >> 3);
        if (s0 < 0 && unseen_is_invalid) {                                  // corner i itself is unseen
            prev_valid = false;
            continue;
        }
        if (!corners_of(a, c, s0, T)) { prev_valid = false; continue; }
        const float F = trilinear(T, c.f[0], c.f[1], c.f[2]);
        if (prev_valid) {
            if (!(F_prev < 0.0f) && F < 0.0f) {
                hit_k = k; F_hit = F; f[0] = c.f[0]; f[1] = c.f[1]; f[2] = c.f[2];
                hit_i[0] = c.i[0]; hit_i[1] = c.i[1]; hit_i[2] = c.i[2]; hit_slot = s0;
                break;
            }
            if (F_prev < 0.0f && !(F < 0.0f)) break;
        }
        prev_valid = true;
        F_prev = F;
    }

    write_pixel(a, view, u, v, hit_k, F_prev, F_hit, T, f, a.colour != nullptr, [&](unsigned C[8]) {
        long long P[8];
        corner_indices(a, hit_i, hit_slot, P);
#pragma unroll
        for (int j = 0; j < 8; ++j) C[j] = P[j] >= 0 ? a.colour[P[j]] : 0u;
    });
}

}  // namespace

extern "C" int mr_tsdf_sparse_render_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                                         const uint8_t* colour, int64_t num_slots, const float* origin, float voxel_size, float min_weight,
                                         const mr_tsdf_ray_view* views, int32_t num_views, int32_t height, int32_t width, float t_min,
                                         float t_max, float step, void* stream) {
    long long blocks;
    if (bad_sparse(table, nbx, nby, nbz, tsdf, weight, colour, blocks)) return MR_ERR_BAD_ARGUMENT;
    if (nbx > MAX_BLOCKS_PER_AXIS || nby > MAX_BLOCKS_PER_AXIS || nbz > MAX_BLOCKS_PER_AXIS) return MR_ERR_BAD_ARGUMENT;
    if (num_slots < 0 || num_slots >= MAX_VOXELS / BV || num_slots > blocks) return MR_ERR_BAD_ARGUMENT;
    if (!origin || !(voxel_size > 0.0f) || min_weight != min_weight) return MR_ERR_BAD_ARGUMENT;
    if (bad_ray_views(views, num_views, height, width, t_min, t_max, step)) return MR_ERR_BAD_ARGUMENT;
    const long long last = last_sample(t_min, t_max, step);
    if (last < 0) return MR_ERR_BAD_ARGUMENT;
    SparseRenderArgs a;
    a.table = table; a.tsdf = tsdf; a.weight = weight; a.colour = reinterpret_cast<const unsigned*>(colour);
    a.nbx = nbx; a.nby = nby; a.num_slots = (int)num_slots;
    const int dims[3] = {nbx * B, nby * B, nbz * B};
    // no slot in use: no voxel is negative, so no sample is a hit - the rays are not marched, every output is written as 0
    const unsigned tiles = prepare_march(a, dims, origin, voxel_size, min_weight, t_min, step, num_slots ? last : -1, height, width, views,
                                         num_views);
    if (!tiles) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(tsdf_sparse_render_kernel, dim3(tiles, 1, (unsigned)num_views), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
