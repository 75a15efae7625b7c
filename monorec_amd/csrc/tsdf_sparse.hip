// A block-sparse TSDF volume (monorec_amd/tsdf_fusion.py, SparseTSDFVolume): storage only for the blocks of MR_TSDF_BLOCK^3 = 8^3 voxels
// that some keyframe puts within the truncation band of a surface.  No hashing: a direct-indexed table of one int32 per block (-1: no
// storage, else a slot) and a pool of slots of 512 voxels, handed out by one fetch-add on a cursor.  The arithmetic is the dense volume's
// (tsdf_common.h; compiled with -ffp-contract=off), the rules are in include/monorec_hip.h, tests/tsdf_sparse_ref.py restates them in
// numpy and the GPU tests compare bit for bit.
//
//   tsdf_sparse_integrate_kernel   a workgroup of 128 threads owns one block, a thread four voxels along x: the block's 2 KB of tsdf and
//                                  of weight are 128 contiguous 16-byte accesses.  Frames are culled per block with the dense kernel's
//                                  five planes; a block no frame reaches leaves before it has touched memory, the table included.  A
//                                  block without a slot is computed in registers from the empty state; whether it gets one is a
//                                  workgroup-wide OR of "some voxel in band" and then one atomic on the cursor.
//   tsdf_sparse_extract_kernel     a workgroup of 256 threads per slot: its 8^3 voxels plus one beyond the high faces (9^3: tsdf, a code
//                                  byte and the colour, 6.5 KB) staged from up to eight blocks through the table, then the dense vertex
//                                  kernel's masks, prefix sum and records: <3> over the three axis edges (the points), <7> over all
//                                  seven a voxel owns (the mesh's vertices), which also writes vertex_base per POOL voxel
//   tsdf_sparse_mesh_triangles_kernel   a workgroup per slot again: the code byte of its block plus TWO voxels beyond the high faces
//                                  (10^3, still only the seven + neighbours) and the 9^3 owner masks that follow from them (1.7 KB), then
//                                  the dense triangle kernel's cases, count and fill; an owner's vertex_base is read in the owner's slot
//   tsdf_sparse_vertex_normals_kernel, tsdf_sparse_cluster_vertices_kernel, tsdf_sparse_cluster_triangles_kernel   the mesh with a unit
//                                  normal per vertex, and at a level of detail (one vertex per cluster of 2^3, 4^3 or 8^3 voxels): the
//                                  dense kernels' rules through tsdf_mesh.h, a workgroup per slot
//   tsdf_sparse_gather_kernel      a box of voxels into dense arrays, 1 / 0 / 0 where a block has no slot
// B, BV, pool_index (of the gather) and bad_sparse are in tsdf_common.h, with what the dense volume's kernels run too.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monorec_hip.h"
#include "tsdf_common.h"
#include "tsdf_mesh.h"

namespace {

constexpr int S = B + 1, SN = S * S * S;         // staged block of the vertex kernel, and the owner masks of the triangle kernel
constexpr int C = B + 2, CN = C * C * C;         // staged codes of the triangle kernel

struct Pool {
    float* tsdf;
    float* weight;
    unsigned* colour;                            // r g b 0 per voxel or null
};

struct SparseIntegrateArgs {
    int* table;
    Pool pool;
    int* block_of_slot;
    unsigned long long* cursor;
    long long capacity;
    int nbx, nby;
    int x0, y0, z0, cx, cy;                      // the launch's box of blocks: its first block and its extent along x and y
    FrameArgs fr;                                // the frames, their planes, the cull radius of a block
};

__global__ __launch_bounds__(128) void tsdf_sparse_integrate_kernel(const SparseIntegrateArgs a) {
    __shared__ unsigned long long s_drawn;
    const int box = blockIdx.x;
    const int bx = a.x0 + box % a.cx, by = a.y0 + (box / a.cx) % a.cy, bz = a.z0 + box / (a.cx * a.cy);
    const long long vx = (long long)bx * B, vy = (long long)by * B, vz = (long long)bz * B;         // (a block count may reach 2^31 - 1)
    const float ccx = a.fr.ox + ((float)vx + 0.5f * (B - 1)) * a.fr.voxel;
    const float ccy = a.fr.oy + ((float)vy + 0.5f * (B - 1)) * a.fr.voxel;
    const float ccz = a.fr.oz + ((float)vz + 0.5f * (B - 1)) * a.fr.voxel;
    const unsigned live = live_frames(a.fr, ccx, ccy, ccz);
    if (live == 0) return;

    const int tid = threadIdx.x;
    const int bi = (bz * a.nby + by) * a.nbx + bx;                           // below 2^31 (checked by the entry)
    const int slot = a.table[bi];                                            // uniform over the workgroup
    float t[4] = {1.0f, 1.0f, 1.0f, 1.0f}, wgt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    unsigned col[4] = {0u, 0u, 0u, 0u};
    if (slot >= 0) {
        const long long at = (long long)slot * BV + tid * 4;
        const float4 tv = *reinterpret_cast<const float4*>(a.pool.tsdf + at);
        const float4 wv = *reinterpret_cast<const float4*>(a.pool.weight + at);
        t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
        wgt[0] = wv.x; wgt[1] = wv.y; wgt[2] = wv.z; wgt[3] = wv.w;
        if (a.pool.colour) {
            const uint4 cv = *reinterpret_cast<const uint4*>(a.pool.colour + at);
            col[0] = cv.x; col[1] = cv.y; col[2] = cv.z; col[3] = cv.w;
        }
    }

    const FrameArgs& fr = a.fr;
    const long long x = vx + (tid & 1) * 4, y = vy + ((tid >> 1) & 7), z = vz + (tid >> 4);
    const float py = fr.oy + (float)y * fr.voxel, pz = fr.oz + (float)z * fr.voxel;
    const float wf = (float)fr.w, hf = (float)fr.h;
    unsigned touched = 0;
    bool band = false;
    for (int fi = 0; fi < fr.num_frames; ++fi) {
        if (!(live & (1u << fi))) continue;
        const mr_tsdf_view& f = fr.f[fi];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float px = fr.ox + (float)(x + j) * fr.voxel;
            tsdf_update_voxel(f, px, py, pz, fr.w, wf, hf, fr.trunc, fr.max_depth, a.pool.colour != nullptr, t[j], wgt[j], col[j], touched, 1u << j, band);
        }
    }

    long long at;
    if (slot >= 0) {
        if (!touched) return;
        at = (long long)slot * BV + tid * 4;
    } else {
        if (!__syncthreads_or((int)band)) return;                            // free space, or never seen: no storage
        if (tid == 0) {
            const unsigned long long drawn = atomicAdd(a.cursor, 1ull);      // one per new block
            if (drawn < (unsigned long long)a.capacity) {
                a.table[bi] = (int)drawn;
                a.block_of_slot[drawn] = bi;
            }
            s_drawn = drawn;
        }
        __syncthreads();
        if (s_drawn >= (unsigned long long)a.capacity) return;               // the pool is full: the cursor tells
        at = (long long)s_drawn * BV + tid * 4;                              // the whole block, untouched voxels as 1 / 0 / 0
    }
    *reinterpret_cast<float4*>(a.pool.tsdf + at) = make_float4(t[0], t[1], t[2], t[3]);
    *reinterpret_cast<float4*>(a.pool.weight + at) = make_float4(wgt[0], wgt[1], wgt[2], wgt[3]);
    if (a.pool.colour) *reinterpret_cast<uint4*>(a.pool.colour + at) = make_uint4(col[0], col[1], col[2], col[3]);
}

struct SparseExtractArgs {
    const int* table;
    Pool pool;
    const int* block_of_slot;
    int nbx, nby, nbz;
    long long blocks;                            // nbx * nby * nbz
    long long num_slots;
    float ox, oy, oz, voxel, min_weight;
    float* records;                              // null: count only
    int* vertex_base;                            // per pool voxel: written by the 7-edge vertex kernel, read by the triangle kernel
    int* triangles;                              // null: count only
    long long capacity;
    unsigned long long* cursor;
};

// the slots of the workgroup's block (its own: blockIdx.x) and of its seven + neighbours, -1 where there is none; tid < 8
__device__ __forceinline__ void stage_slots(const SparseExtractArgs& a, int* s_slot, int tid, int bx, int by, int bz) {
    const int nx = bx + (tid & 1), ny = by + ((tid >> 1) & 1), nz = bz + (tid >> 2);
    int s = -1;
    if (nx < a.nbx && ny < a.nby && nz < a.nbz) s = tid == 0 ? (int)blockIdx.x : a.table[((long long)nz * a.nby + ny) * a.nbx + nx];
    s_slot[tid] = s < a.num_slots ? s : -1;
}

// Is voxel (x, y, z) - counted from the first voxel of block (bx, by, bz), from -1 to 9 - inside the volume, in a block with a slot, and
// seen?  Then t is its tsdf: what the normals ask of the volume (voxel_gradient, tsdf_mesh.h).  Through the table, not the staged slots:
// it reaches the - neighbours too.
struct BlockSample {
    const SparseExtractArgs& a;
    int bx, by, bz;
    __device__ __forceinline__ bool operator()(int x, int y, int z, float& t) const {
        const int nx = bx + (x >> 3), ny = by + (y >> 3), nz = bz + (z >> 3);        // (>> of -1 is -1)
        if ((unsigned)nx >= (unsigned)a.nbx || (unsigned)ny >= (unsigned)a.nby || (unsigned)nz >= (unsigned)a.nbz) return false;
        const int s = a.table[((long long)nz * a.nby + ny) * a.nbx + nx];
        if (s < 0 || s >= a.num_slots) return false;
        const long long p = pool_index(s, x, y, z);
        if (!(a.pool.weight[p] > a.min_weight)) return false;
        t = a.pool.tsdf[p];
        return true;
    }
};

// EDGES = 3: the axis edges alone, the points of mr_tsdf_sparse_extract_f32.  EDGES = 7: the vertices of the mesh, and vertex_base.
// NORMALS (the variant tsdf_sparse_vertex_normals_kernel alone): the unit normal of every vertex into normals[3 * index].
template <int EDGES, bool NORMALS>
__device__ __forceinline__ void sparse_extract_tile(const SparseExtractArgs& a, float* normals) {
    static_assert(EDGES == 3 || EDGES == 7, "the axis edges, or all a voxel owns");
    __shared__ float s_t[SN];
    __shared__ unsigned s_col[SN];
    __shared__ uint8_t s_code[SN];
    __shared__ int s_slot[8];
    __shared__ int wave_tot[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const int bi = a.block_of_slot[blockIdx.x];
    if (bi < 0 || bi >= a.blocks) return;                                    // (a slot the caller counts but no launch filled)
    const int bx = bi % a.nbx, by = (bi / a.nbx) % a.nby, bz = bi / (a.nbx * a.nby);
    if (tid < 8) stage_slots(a, s_slot, tid, bx, by, bz);
    __syncthreads();
    int any_neg = 0;
    for (int i = tid; i < SN; i += 256) {
        const int sx = i % S, sy = (i / S) % S, sz = i / (S * S);
        const int s = s_slot[(sx >> 3) | ((sy >> 3) << 1) | ((sz >> 3) << 2)];
        float t = 1.0f;
        unsigned c = 0u, rgb = 0u;
        if (s >= 0) {
            const long long p = (long long)s * BV + (((sz & 7) * B + (sy & 7)) * B + (sx & 7));
            if (a.pool.weight[p] > a.min_weight) {
                t = a.pool.tsdf[p];
                c = t < 0.0f ? (SEEN | NEG) : SEEN;
                if (a.pool.colour) rgb = a.pool.colour[p];
            }
        }
        s_t[i] = t;
        s_col[i] = rgb;
        s_code[i] = (uint8_t)c;
        any_neg |= (int)(c & NEG);
    }
    if (!__syncthreads_or(any_neg)) return;

    const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;              // the thread's two voxels: z = lz and lz + 4
    unsigned masks = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) masks |= edge_mask<EDGES>(s_code, ((lz + 4 * j) * S + ly) * S + lx, S, S * S) << (8 * j);
    const int mine = __popc(masks);
    int total;
    const int before = workgroup_prefix(mine, wave_tot, total);
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(a.cursor, (unsigned long long)total);   // one per workgroup
    if (!a.records) return;
    __syncthreads();
    if (!masks) return;
    long long rec = (long long)s_base + before;
    const float px = a.ox + (float)((long long)bx * B + lx) * a.voxel, py = a.oy + (float)((long long)by * B + ly) * a.voxel;
    const int s_far[7] = {1, S, S * S, 1 + S, 1 + S * S, S + S * S, 1 + S + S * S};
    constexpr unsigned along[7] = {1u, 2u, 4u, 3u, 5u, 6u, 7u};              // bit k: the edge advances along axis k
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned mask = (masks >> (8 * j)) & 0xffu;
        if (!mask) continue;
        const int at = ((lz + 4 * j) * S + ly) * S + lx;
        if constexpr (EDGES == 7) a.vertex_base[(long long)blockIdx.x * BV + (((lz + 4 * j) * B + ly) * B + lx)] = (int)rec;
        const float p[3] = {px, py, a.oz + (float)((long long)bz * B + lz + 4 * j) * a.voxel};
        const float tv = s_t[at];
        const unsigned cv = s_col[at];
#pragma unroll
        for (int e = 0; e < EDGES; ++e) {
            if (!(mask & (1u << e))) continue;
            if (rec < a.capacity) {
                const float s = tv / (tv - s_t[at + s_far[e]]);
                const float step = s * a.voxel;
                float* r = a.records + rec * 6;
#pragma unroll
                for (int k = 0; k < 3; ++k) r[k] = (along[e] >> k) & 1u ? p[k] + step : p[k];
                write_colour(r, cv, s_col[at + s_far[e]], s);
                if constexpr (NORMALS)
                    vertex_normal(BlockSample{a, bx, by, bz}, lx, ly, lz + 4 * j, tv, e, s_t[at + s_far[e]], s, normals + rec * 3);
            }
            ++rec;
        }
    }
}

template <int EDGES>
__global__ __launch_bounds__(256) void tsdf_sparse_extract_kernel(const SparseExtractArgs a) { sparse_extract_tile<EDGES, false>(a, nullptr); }

__global__ __launch_bounds__(256) void tsdf_sparse_vertex_normals_kernel(const SparseExtractArgs a, float* normals) {
    sparse_extract_tile<7, true>(a, normals);
}

// ---- the clustered level of detail (the dense kernels' rules and code: tsdf_mesh.h): a workgroup per slot, whose block is 64, 8 or 1
// whole clusters
struct ClusterArgs {
    float* normals;                              // vertices only; null: none
    int* cluster_base;                           // (8 / cell)^3 per slot: written by the vertex kernel, read by the triangle kernel
    int shift;                                   // cell = 1 << shift
};

// the vertex kernel's staging (tsdf, colour and code of the block plus one voxel) and masks, then the dense kernel's runs: a lane sums
// one of the block's 64 runs in the fixed order, the first lane of each cluster - 64, 8 or 1 of them - adds its 1, 8 or 64 runs in order
constexpr int UNITS = BV / RUN;
static_assert(SN >= 10 * UNITS, "the run sums (9 floats and a count per run) take the place of the staged tsdf");
template <bool NORMALS>
__global__ __launch_bounds__(256) void tsdf_sparse_cluster_vertices_kernel(const SparseExtractArgs a, const ClusterArgs k) {
    __shared__ float s_t[SN];
    __shared__ unsigned s_col[SN];
    __shared__ uint8_t s_code[SN];
    __shared__ uint8_t s_mask[SN];
    __shared__ uint8_t s_owns[UNITS];
    __shared__ int s_slot[8];
    __shared__ int wave_tot[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const int bi = a.block_of_slot[blockIdx.x];
    if (bi < 0 || bi >= a.blocks) return;                                    // (a slot the caller counts but no launch filled)
    const int bx = bi % a.nbx, by = (bi / a.nbx) % a.nby, bz = bi / (a.nbx * a.nby);
    if (tid < 8) stage_slots(a, s_slot, tid, bx, by, bz);
    __syncthreads();
    int any_neg = 0;
    for (int i = tid; i < SN; i += 256) {
        const int sx = i % S, sy = (i / S) % S, sz = i / (S * S);
        const int s = s_slot[(sx >> 3) | ((sy >> 3) << 1) | ((sz >> 3) << 2)];
        float t = 1.0f;
        unsigned c = 0u, rgb = 0u;
        if (s >= 0) {
            const long long p = (long long)s * BV + (((sz & 7) * B + (sy & 7)) * B + (sx & 7));
            if (a.pool.weight[p] > a.min_weight) {
                t = a.pool.tsdf[p];
                c = t < 0.0f ? (SEEN | NEG) : SEEN;
                if (a.pool.colour) rgb = a.pool.colour[p];
            }
        }
        s_t[i] = t;
        s_col[i] = rgb;
        s_code[i] = (uint8_t)c;
        any_neg |= (int)(c & NEG);
    }
    if (!__syncthreads_or(any_neg)) return;
    for (int i = tid; i < BV; i += 256) {
        const int at = ((i >> 6) * S + ((i >> 3) & 7)) * S + (i & 7);
        s_mask[at] = (uint8_t)edge_mask<7>(s_code, at, S, S * S);
    }
    __syncthreads();

    // the block is 64 runs of 8 voxels for every cell (tsdf_mesh.h): run `run` of cluster q of the block's is unit q * runs + run, on
    // thread 4 * unit - sixteen of them in every wave
    const int sh = k.shift, qn = B >> sh, runs = (1 << (3 * sh)) / RUN;
    const int unit = tid >> 2, q = unit / runs, run = unit % runs;
    const bool mine = (tid & 3) == 0;
    const int lx = (q % qn) << sh, ly = ((q / qn) % qn) << sh, lz = (q / (qn * qn)) << sh;           // the cluster's first voxel in the block
    const int at0 = (lz * S + ly) * S + lx;
    const int owns = mine ? run_owns(s_mask, at0, S, S * S, sh, run) : 0;
    if (mine) s_owns[unit] = (uint8_t)owns;
    __syncthreads();
    int has = 0;                                 // of the lane of the cluster's first run: does the cluster own a vertex?
    if (mine && run == 0)
        for (int r = 0; r < runs; ++r) has |= s_owns[unit + r];
    int total;
    const int before = workgroup_prefix(has, wave_tot, total);
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(a.cursor, (unsigned long long)total);   // one per workgroup
    if (!a.records) return;
    constexpr int N = NORMALS ? 9 : 6;
    float sum[N];
    int count = 0;
    if (owns) {
        const auto vertex = [&](int dx, int dy, int dz, int at, int e, float* r) {
            const int x = lx + dx, y = ly + dy, z = lz + dz;
            const int far = (int)(EDGE_ALONG[e] & 1u) + (int)((EDGE_ALONG[e] >> 1) & 1u) * S + (int)(EDGE_ALONG[e] >> 2) * (S * S);
            const float p[3] = {a.ox + (float)((long long)bx * B + x) * a.voxel, a.oy + (float)((long long)by * B + y) * a.voxel,
                                a.oz + (float)((long long)bz * B + z) * a.voxel};
            const float tv = s_t[at], tn = s_t[at + far];
            const float s = edge_record(tv, tn, p, e, a.voxel, s_col[at], s_col[at + far], r);
            if constexpr (NORMALS) vertex_normal(BlockSample{a, bx, by, bz}, x, y, z, tv, e, tn, s, r + 6);
        };
        count = run_sum<NORMALS>(s_mask, at0, S, S * S, sh, run, sum, vertex);
    }
    // the sums of the runs and, last, their counts go through LDS as [sum][run], in the place of the staged tsdf, which every lane has
    // finished reading
    __syncthreads();
    float* s_part = s_t;
    if (mine) {
#pragma unroll
        for (int c = 0; c < N; ++c) s_part[c * UNITS + unit] = owns ? sum[c] : 0.0f;
        s_part[N * UNITS + unit] = (float)count;
    }
    __syncthreads();                             // (also: s_base is there)
    if (!has) return;
    const long long rec = (long long)s_base + before;
    k.cluster_base[(long long)blockIdx.x * (qn * qn * qn) + q] = (int)rec;
    if (rec >= a.capacity) return;
    float out[9];
    cluster_combine<NORMALS>(s_part + unit, UNITS, runs, out);
#pragma unroll
    for (int c = 0; c < 6; ++c) a.records[rec * 6 + c] = out[c];
    if constexpr (NORMALS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) k.normals[rec * 3 + c] = out[6 + c];
    }
}

// the triangle kernel's cubes, two per thread, over the codes of the block plus ONE voxel (no masks: a vertex is its owner's cluster)
__global__ __launch_bounds__(256) void tsdf_sparse_cluster_triangles_kernel(const SparseExtractArgs a, const ClusterArgs k) {
    __shared__ uint8_t s_code[SN];
    __shared__ int s_slot[8];
    __shared__ int wave_tot[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const int bi = a.block_of_slot[blockIdx.x];
    if (bi < 0 || bi >= a.blocks) return;                                    // (a slot the caller counts but no launch filled)
    const int bx = bi % a.nbx, by = (bi / a.nbx) % a.nby, bz = bi / (a.nbx * a.nby);
    if (tid < 8) stage_slots(a, s_slot, tid, bx, by, bz);
    __syncthreads();
    int any_neg = 0;
    for (int i = tid; i < SN; i += 256) {
        const int sx = i % S, sy = (i / S) % S, sz = i / (S * S);            // 8 lies in the + neighbour
        const int s = s_slot[(sx >> 3) | ((sy >> 3) << 1) | ((sz >> 3) << 2)];
        unsigned c = 0u;
        if (s >= 0) {
            const long long p = (long long)s * BV + (((sz & 7) * B + (sy & 7)) * B + (sx & 7));
            if (a.pool.weight[p] > a.min_weight) c = a.pool.tsdf[p] < 0.0f ? (SEEN | NEG) : SEEN;
        }
        s_code[i] = (uint8_t)c;
        any_neg |= (int)(c & NEG);
    }
    if (!__syncthreads_or(any_neg)) return;

    const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6, sh = k.shift, qn = B >> sh;
    // the cluster of voxel (x, y, z) of the staged block, 0 .. 8, in its own slot's part of cluster_base: below 2^31 (checked by the
    // entry).  A corner of a cube with a case is seen, so its block has a slot.
    const auto cluster_at = [&](int x, int y, int z) {
        const int s = s_slot[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
        return (s * qn + ((z & 7) >> sh)) * qn * qn + ((y & 7) >> sh) * qn + ((x & 7) >> sh);
    };
    unsigned cases[2];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        cases[j] = cube_cases(s_code, ((lz + 4 * j) * S + ly) * S + lx, S, S * S);
        if (!cases[j]) continue;
        const auto cid = [&](int dx, int dy, int dz) { return cluster_at(lx + dx, ly + dy, lz + 4 * j + dz); };
        cluster_cube_triangles(cases[j], cid, [&](int, int, int) { ++mine; });
    }
    int total;
    const int before = workgroup_prefix(mine, wave_tot, total);
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(a.cursor, (unsigned long long)total);   // one per workgroup
    if (!a.triangles) return;
    __syncthreads();
    if (!mine) return;
    long long tri = (long long)s_base + before;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!cases[j]) continue;
        const auto cid = [&](int dx, int dy, int dz) { return cluster_at(lx + dx, ly + dy, lz + 4 * j + dz); };
        cluster_cube_triangles(cases[j], cid, [&](int va, int vb, int vc) {
            if (tri < a.capacity) {
                int* r = a.triangles + tri * 3;
                r[0] = k.cluster_base[va]; r[1] = k.cluster_base[vb]; r[2] = k.cluster_base[vc];
            }
            ++tri;
        });
    }
}

// The triangles of the cubes whose base voxel lies in the workgroup's block, two cubes per thread (z = lz and lz + 4): the dense triangle
// kernel's cases, count and fill.  An owner across a block face has its vertex_base in the slot of that + neighbour; it has one, because
// a cube emits only where all its corners are seen, and a voxel of a block without a slot is not.
__global__ __launch_bounds__(256) void tsdf_sparse_mesh_triangles_kernel(const SparseExtractArgs a) {
    __shared__ uint8_t s_code[CN];
    __shared__ uint8_t s_mask[SN];
    __shared__ int s_slot[8];
    __shared__ int wave_tot[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const int bi = a.block_of_slot[blockIdx.x];
    if (bi < 0 || bi >= a.blocks) return;                                    // (a slot the caller counts but no launch filled)
    const int bx = bi % a.nbx, by = (bi / a.nbx) % a.nby, bz = bi / (a.nbx * a.nby);
    if (tid < 8) stage_slots(a, s_slot, tid, bx, by, bz);
    __syncthreads();
    int any_neg = 0;
    for (int i = tid; i < CN; i += 256) {
        const int sx = i % C, sy = (i / C) % C, sz = i / (C * C);            // 8 and 9 lie in the + neighbour
        const int s = s_slot[(sx >> 3) | ((sy >> 3) << 1) | ((sz >> 3) << 2)];
        unsigned c = 0u;
        if (s >= 0) {
            const long long p = (long long)s * BV + (((sz & 7) * B + (sy & 7)) * B + (sx & 7));
            if (a.pool.weight[p] > a.min_weight) c = a.pool.tsdf[p] < 0.0f ? (SEEN | NEG) : SEEN;
        }
        s_code[i] = (uint8_t)c;
        if (sx < S && sy < S && sz < S) any_neg |= (int)(c & NEG);           // the corners of the block's cubes
    }
    if (!__syncthreads_or(any_neg)) return;

    const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
    unsigned cases[2];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        cases[j] = cube_cases(s_code, ((lz + 4 * j) * C + ly) * C + lx, C, C * C);
#pragma unroll
        for (int t = 0; t < 6; ++t) mine += (int)(TET_CASES[(cases[j] >> (4 * t)) & 15u] & 15u);
    }
    int total;
    const int before = workgroup_prefix(mine, wave_tot, total);
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(a.cursor, (unsigned long long)total);   // one per workgroup
    if (!a.triangles) return;
    for (int i = tid; i < SN; i += 256) {
        const int sx = i % S, sy = (i / S) % S, sz = i / (S * S);
        s_mask[i] = (uint8_t)edge_mask<7>(s_code, (sz * C + sy) * C + sx, C, C * C);
    }
    __syncthreads();
    if (!mine) return;
    long long tri = (long long)s_base + before;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (!cases[j]) continue;
#pragma unroll 1
        for (int t = 0; t < 6; ++t) {
            unsigned word = TET_CASES[(cases[j] >> (4 * t)) & 15u];
            const int count = (int)(word & 15u);
            if (!count) continue;
            const unsigned perm = TET_PERMS[t];
            const int pa = perm & 3u, pb = (perm >> 2) & 3u, pc = (perm >> 4) & 3u;
            // the owners c0, c1, c2 of the tetrahedron's six edges, as voxels 0 .. 8 of the staged block, and the edges' types
            const int x0 = lx, y0 = ly, z0 = lz + 4 * j;
            const int x1 = x0 + (pa == 0), y1 = y0 + (pa == 1), z1 = z0 + (pa == 2);
            const int x2 = x1 + (pb == 0), y2 = y1 + (pb == 1), z2 = z1 + (pb == 2);
            const auto m_at = [](int x, int y, int z) { return (z * S + y) * S + x; };
            const auto g_at = [&](int x, int y, int z) {                      // the voxel's place in the pool: its own slot's
                const int s = s_slot[(x >> 3) | ((y >> 3) << 1) | ((z >> 3) << 2)];
                return (long long)s * BV + (((z & 7) * B + (y & 7)) * B + (x & 7));
            };
            const int m_own[3] = {m_at(x0, y0, z0), m_at(x1, y1, z1), m_at(x2, y2, z2)};
            const long long g_own[3] = {g_at(x0, y0, z0), g_at(x1, y1, z1), g_at(x2, y2, z2)};
            const int owner[6] = {0, 1, 2, 0, 1, 0};
            const int type[6] = {pa, pb, pc, 2 + pa + pb, 2 + pb + pc, 6};
            word >>= 4;
            for (int n = 0; n < count; ++n, ++tri, word >>= 12) {
                if (tri >= a.capacity) continue;
                int v[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int edge = (int)((word >> (4 * k)) & 15u);
                    int own = 0, ty = 0;
#pragma unroll
                    for (int q = 0; q < 6; ++q) if (edge == q) { own = owner[q]; ty = type[q]; }
                    int mo = m_own[0];
                    long long go = g_own[0];
                    if (own == 1) { mo = m_own[1]; go = g_own[1]; }
                    if (own == 2) { mo = m_own[2]; go = g_own[2]; }
                    v[k] = a.vertex_base[go] + __popc((unsigned)s_mask[mo] & ((1u << ty) - 1u));
                }
                int* r = a.triangles + tri * 3;
                const bool odd = t >= 3;
                r[0] = v[0]; r[1] = odd ? v[2] : v[1]; r[2] = odd ? v[1] : v[2];
            }
        }
    }
}

struct SparseGatherArgs {
    const int* table;
    Pool pool;
    int nbx, nby;
    int x0, y0, z0, dx, dy;
    long long voxels;                            // dx * dy * dz
    float* tsdf;
    float* weight;
    unsigned* colour;                            // null: not asked for
};

__global__ __launch_bounds__(256) void tsdf_sparse_gather_kernel(const SparseGatherArgs a) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.voxels; i += stride) {
        const long long row = i / a.dx;
        const int x = a.x0 + (int)(i - row * a.dx), y = a.y0 + (int)(row % a.dy), z = a.z0 + (int)(row / a.dy);
        const int s = a.table[((long long)(z >> 3) * a.nby + (y >> 3)) * a.nbx + (x >> 3)];
        float t = 1.0f, w = 0.0f;
        unsigned c = 0u;
        if (s >= 0) {
            const long long p = pool_index(s, x, y, z);
            t = a.pool.tsdf[p];
            w = a.pool.weight[p];
            if (a.colour) c = a.pool.colour[p];
        }
        a.tsdf[i] = t;
        a.weight[i] = w;
        if (a.colour) a.colour[i] = c;
    }
}

// The box of blocks one frame can update, in double: a voxel is updated only if its camera-space point c = A p + t has 0 < c_2, projects
// within `slack` pixels of the image (view_planes) and has c_2 < d + trunc <= depth, so c lies in the pyramid between the camera centre
// and the four image-corner rays at `depth`, and p in the box of the five points A^-1 (c - t).  `push`: what the fp32 evaluation can move
// c by; it reaches p through A^-1.  False: anything doubtful (view_planes' cases, A nearly singular, non-finite numbers) - the whole table.
bool frame_box(const mr_tsdf_view& f, int h, int w, double depth, double push, double lo[3], double hi[3]) {
    if (!(f.fx > 0.0f) || !(f.fy > 0.0f)) return false;
    double A[3][3], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) A[r][k] = (double)f.m[4 * r + k];
        t[r] = (double)f.m[4 * r + 3];
        const double len = sqrt(A[r][0] * A[r][0] + A[r][1] * A[r][1] + A[r][2] * A[r][2]);
        if (!(len > 0.5 && len < 2.0)) return false;
    }
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    if (!(fabs(det) > 0.05)) return false;
    double inv[3][3], norm = 0.0;
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            inv[k][r] = (A[r1][k1] * A[r2][k2] - A[r1][k2] * A[r2][k1]) / det;                   // the cofactor, transposed
        }
    for (int r = 0; r < 3; ++r) norm = fmax(norm, fabs(inv[r][0]) + fabs(inv[r][1]) + fabs(inv[r][2]));
    const double slack_u = view_slack(f.cx, w, f.fx), slack_v = view_slack(f.cy, h, f.fy);
    const double su[2] = {(-0.5 - slack_u - (double)f.cx) / f.fx, ((double)w - 0.5 + slack_u - (double)f.cx) / f.fx};
    const double sv[2] = {(-0.5 - slack_v - (double)f.cy) / f.fy, ((double)h - 0.5 + slack_v - (double)f.cy) / f.fy};
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    for (int corner = 0; corner < 5; ++corner) {
        const double c[3] = {corner < 4 ? su[corner & 1] * depth : 0.0, corner < 4 ? sv[corner >> 1] * depth : 0.0, corner < 4 ? depth : 0.0};
        for (int k = 0; k < 3; ++k) {
            const double p = inv[k][0] * (c[0] - t[0]) + inv[k][1] * (c[1] - t[1]) + inv[k][2] * (c[2] - t[2]);
            if (!isfinite(p)) return false;
            lo[k] = fmin(lo[k], p - push * norm);
            hi[k] = fmax(hi[k], p + push * norm);
        }
    }
    return true;
}

// What the three surface entries share: the checks of table, pool, slots, output and cursor, and the kernels' arguments with no output
// set.  The triangle entry has no colour and no positions (NO_ORIGIN, a voxel of 1).  True: a bad argument.
bool surface_args(SparseExtractArgs& a, const int32_t* table, int nbx, int nby, int nbz, const float* tsdf, const float* weight,
                  const uint8_t* colour, const int32_t* block_of_slot, long long num_slots, const float* origin, float voxel_size,
                  float min_weight, const void* out, long long capacity, int64_t* cursor) {
    long long blocks;
    if (bad_sparse(table, nbx, nby, nbz, tsdf, weight, colour, blocks) || !block_of_slot || !origin) return true;
    if (((uintptr_t)block_of_slot & 3) || bad_output(out, capacity, cursor)) return true;
    if (num_slots < 0 || num_slots >= MAX_VOXELS / BV || num_slots > blocks) return true;
    if (!(voxel_size > 0.0f) || min_weight != min_weight) return true;
    a.table = table;
    a.pool = {const_cast<float*>(tsdf), const_cast<float*>(weight), reinterpret_cast<unsigned*>(const_cast<uint8_t*>(colour))};
    a.block_of_slot = block_of_slot;
    a.nbx = nbx; a.nby = nby; a.nbz = nbz; a.blocks = blocks; a.num_slots = num_slots;
    a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2]; a.voxel = voxel_size; a.min_weight = min_weight;
    a.records = nullptr; a.vertex_base = nullptr; a.triangles = nullptr;
    a.capacity = out ? capacity : 0;
    a.cursor = reinterpret_cast<unsigned long long*>(cursor);
    return false;
}

}  // namespace

extern "C" int mr_tsdf_sparse_integrate_f32(int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, float* tsdf, float* weight, uint8_t* colour,
                                            int32_t* block_of_slot, int64_t capacity, int64_t* cursor, const float* origin, float voxel_size,
                                            float trunc, float max_depth_m, const mr_tsdf_view* frames, int32_t num_frames, int32_t height,
                                            int32_t width, void* stream) {
    long long blocks;
    if (bad_sparse(table, nbx, nby, nbz, tsdf, weight, colour, blocks) || !block_of_slot || !cursor || !origin) return MR_ERR_BAD_ARGUMENT;
    if (((uintptr_t)block_of_slot & 3) || ((uintptr_t)cursor & 7)) return MR_ERR_BAD_ARGUMENT;
    if (capacity < 1 || capacity >= MAX_VOXELS / BV) return MR_ERR_BAD_ARGUMENT;
    if (!(voxel_size > 0.0f)) return MR_ERR_BAD_ARGUMENT;
    SparseIntegrateArgs a;
    // the dense entry's margins, for the sphere round the voxel centres of a block
    const double v = (double)voxel_size;
    const int nb[3] = {nbx, nby, nbz};
    const double voxels[3] = {(double)nbx * B, (double)nby * B, (double)nbz * B};
    const double margin = frame_args(a.fr, origin, voxel_size, trunc, max_depth_m, frames, num_frames, height, width, colour != nullptr, voxels, B,
                                     0.5 * v * sqrt(3.0 * (B - 1) * (B - 1)));
    if (margin < 0.0) return MR_ERR_BAD_ARGUMENT;
    a.table = table;
    a.pool = {tsdf, weight, reinterpret_cast<unsigned*>(colour)};
    a.block_of_slot = block_of_slot;
    a.cursor = reinterpret_cast<unsigned long long*>(cursor);
    a.capacity = capacity;
    a.nbx = nbx; a.nby = nby;
    // The launch's box of blocks: no frame can update a voxel outside it, so leaving the rest of the table out changes no result.  Depths
    // come from int16 centimetres (at most 327.67 m) and count up to max_depth_m; a voxel trunc behind one is still updated.
    const double depth = (fmax(0.0, fmin((double)max_depth_m, 327.67)) + (double)trunc) * (1.0 + 1e-6) + margin;
    int first[3] = {nbx, nby, nbz}, last[3] = {-1, -1, -1};
    for (int i = 0; i < num_frames; ++i) {
        double lo[3], hi[3];
        const bool known = isfinite(depth) && frame_box(frames[i], height, width, depth, margin, lo, hi);
        bool empty = false;
        int f_first[3], f_last[3];
        for (int k = 0; k < 3; ++k) {
            f_first[k] = 0; f_last[k] = nb[k] - 1;
            if (!known) continue;
            // voxel indices one further out than the box, then their blocks, clipped to the table while still double
            const double b_lo = floor((floor((lo[k] - (double)origin[k]) / v) - 1.0) / B), b_hi = floor((ceil((hi[k] - (double)origin[k]) / v) + 1.0) / B);
            if (!isfinite(b_lo) || !isfinite(b_hi)) continue;
            if (b_hi < 0.0 || b_lo > (double)(nb[k] - 1)) { empty = true; break; }
            f_first[k] = (int)fmax(b_lo, 0.0); f_last[k] = (int)fmin(b_hi, (double)(nb[k] - 1));
        }
        if (empty) continue;
        for (int k = 0; k < 3; ++k) { first[k] = f_first[k] < first[k] ? f_first[k] : first[k]; last[k] = f_last[k] > last[k] ? f_last[k] : last[k]; }
    }
    if (last[0] < first[0]) return 0;                                                    // no frame looks at the table: nothing to do
    a.x0 = first[0]; a.y0 = first[1]; a.z0 = first[2];
    a.cx = last[0] - first[0] + 1; a.cy = last[1] - first[1] + 1;
    const long long grid = (long long)a.cx * a.cy * (last[2] - first[2] + 1);           // at most the table: below 2^31
    hipLaunchKernelGGL(tsdf_sparse_integrate_kernel, dim3((unsigned)grid), dim3(128), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_sparse_extract_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                                          const uint8_t* colour, const int32_t* block_of_slot, int64_t num_slots, const float* origin,
                                          float voxel_size, float min_weight, float* records, int64_t capacity_records, int64_t* cursor,
                                          void* stream) {
    SparseExtractArgs a;
    if (surface_args(a, table, nbx, nby, nbz, tsdf, weight, colour, block_of_slot, num_slots, origin, voxel_size, min_weight, records,
                     capacity_records, cursor))
        return MR_ERR_BAD_ARGUMENT;
    if (num_slots == 0) return 0;
    a.records = records;
    hipLaunchKernelGGL(tsdf_sparse_extract_kernel<3>, dim3((unsigned)num_slots), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_sparse_mesh_vertices_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                                                const uint8_t* colour, const int32_t* block_of_slot, int64_t num_slots, const float* origin,
                                                float voxel_size, float min_weight, float* vertices, int64_t capacity_vertices,
                                                int32_t* vertex_base, int64_t* cursor, void* stream) {
    SparseExtractArgs a;
    if (surface_args(a, table, nbx, nby, nbz, tsdf, weight, colour, block_of_slot, num_slots, origin, voxel_size, min_weight, vertices,
                     capacity_vertices, cursor) ||
        ((uintptr_t)vertex_base & 3) || (vertices && !vertex_base))
        return MR_ERR_BAD_ARGUMENT;
    if (num_slots == 0) return 0;
    a.records = vertices; a.vertex_base = vertex_base;
    hipLaunchKernelGGL(tsdf_sparse_extract_kernel<7>, dim3((unsigned)num_slots), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_sparse_mesh_triangles_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf,
                                                 const float* weight, const int32_t* block_of_slot, int64_t num_slots, float min_weight,
                                                 const int32_t* vertex_base, int32_t* triangles, int64_t capacity_triangles, int64_t* cursor,
                                                 void* stream) {
    SparseExtractArgs a;
    if (surface_args(a, table, nbx, nby, nbz, tsdf, weight, nullptr, block_of_slot, num_slots, NO_ORIGIN, 1.0f, min_weight, triangles,
                     capacity_triangles, cursor) ||
        ((uintptr_t)vertex_base & 3) || (triangles && !vertex_base))
        return MR_ERR_BAD_ARGUMENT;
    if (num_slots == 0) return 0;
    a.triangles = triangles; a.vertex_base = const_cast<int*>(vertex_base);
    hipLaunchKernelGGL(tsdf_sparse_mesh_triangles_kernel, dim3((unsigned)num_slots), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_sparse_mesh_vertices_normals_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf,
                                                        const float* weight, const uint8_t* colour, const int32_t* block_of_slot,
                                                        int64_t num_slots, const float* origin, float voxel_size, float min_weight,
                                                        float* vertices, int64_t capacity_vertices, float* normals, int32_t* vertex_base,
                                                        int64_t* cursor, void* stream) {
    SparseExtractArgs a;
    if (surface_args(a, table, nbx, nby, nbz, tsdf, weight, colour, block_of_slot, num_slots, origin, voxel_size, min_weight, vertices,
                     capacity_vertices, cursor) ||
        ((uintptr_t)vertex_base & 3) || (vertices && !vertex_base) || ((uintptr_t)normals & 3) || (!vertices != !normals))
        return MR_ERR_BAD_ARGUMENT;
    if (num_slots == 0) return 0;
    a.records = vertices; a.vertex_base = vertex_base;
    hipLaunchKernelGGL(tsdf_sparse_vertex_normals_kernel, dim3((unsigned)num_slots), dim3(256), 0, (hipStream_t)stream, a, normals);
    return (int)hipGetLastError();
}

namespace {

// beyond surface_args, of the two cluster entries: the cell, cluster_base and its int32 indices.  True: a bad argument.
bool cluster_args(ClusterArgs& k, int cell, long long num_slots, const int* cluster_base, const void* out) {
    k.shift = cluster_shift(cell);
    if (k.shift < 0 || ((uintptr_t)cluster_base & 3) || (out && !cluster_base)) return true;
    const int qn = B >> k.shift;
    if (num_slots * (qn * qn * qn) >= (1ll << 31)) return true;
    k.normals = nullptr; k.cluster_base = const_cast<int*>(cluster_base);
    return false;
}

}  // namespace

extern "C" int mr_tsdf_sparse_mesh_cluster_vertices_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf,
                                                        const float* weight, const uint8_t* colour, const int32_t* block_of_slot,
                                                        int64_t num_slots, const float* origin, float voxel_size, float min_weight,
                                                        int32_t cell, float* vertices, int64_t capacity_vertices, float* normals,
                                                        int32_t* cluster_base, int64_t* cursor, void* stream) {
    SparseExtractArgs a;
    ClusterArgs k;
    if (surface_args(a, table, nbx, nby, nbz, tsdf, weight, colour, block_of_slot, num_slots, origin, voxel_size, min_weight, vertices,
                     capacity_vertices, cursor) ||
        cluster_args(k, cell, num_slots, cluster_base, vertices) || ((uintptr_t)normals & 3) || (normals && !vertices))
        return MR_ERR_BAD_ARGUMENT;
    if (num_slots == 0) return 0;
    a.records = vertices;
    k.normals = vertices ? normals : nullptr;
    if (k.normals) hipLaunchKernelGGL(tsdf_sparse_cluster_vertices_kernel<true>, dim3((unsigned)num_slots), dim3(256), 0, (hipStream_t)stream, a, k);
    else hipLaunchKernelGGL(tsdf_sparse_cluster_vertices_kernel<false>, dim3((unsigned)num_slots), dim3(256), 0, (hipStream_t)stream, a, k);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_sparse_mesh_cluster_triangles_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf,
                                                         const float* weight, const int32_t* block_of_slot, int64_t num_slots,
                                                         float min_weight, int32_t cell, const int32_t* cluster_base, int32_t* triangles,
                                                         int64_t capacity_triangles, int64_t* cursor, void* stream) {
    SparseExtractArgs a;
    ClusterArgs k;
    if (surface_args(a, table, nbx, nby, nbz, tsdf, weight, nullptr, block_of_slot, num_slots, NO_ORIGIN, 1.0f, min_weight, triangles,
                     capacity_triangles, cursor) ||
        cluster_args(k, cell, num_slots, cluster_base, triangles))
        return MR_ERR_BAD_ARGUMENT;
    if (num_slots == 0) return 0;
    a.triangles = triangles;
    hipLaunchKernelGGL(tsdf_sparse_cluster_triangles_kernel, dim3((unsigned)num_slots), dim3(256), 0, (hipStream_t)stream, a, k);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_sparse_gather_f32(const int32_t* table, int32_t nbx, int32_t nby, int32_t nbz, const float* tsdf, const float* weight,
                                         const uint8_t* colour, int32_t x0, int32_t y0, int32_t z0, int32_t dx, int32_t dy, int32_t dz,
                                         float* out_tsdf, float* out_weight, uint8_t* out_colour, void* stream) {
    long long blocks;
    if (bad_sparse(table, nbx, nby, nbz, tsdf, weight, colour, blocks) || !out_tsdf || !out_weight || (out_colour && !colour)) return MR_ERR_BAD_ARGUMENT;
    if (((uintptr_t)out_tsdf | (uintptr_t)out_weight | (uintptr_t)out_colour) & 3) return MR_ERR_BAD_ARGUMENT;
    if (x0 < 0 || y0 < 0 || z0 < 0 || dx < 1 || dy < 1 || dz < 1) return MR_ERR_BAD_ARGUMENT;
    if ((long long)x0 + dx > (long long)nbx * B || (long long)y0 + dy > (long long)nby * B || (long long)z0 + dz > (long long)nbz * B) return MR_ERR_BAD_ARGUMENT;
    const long long xy = (long long)dx * dy;
    if (xy >= MAX_VOXELS || dz > MAX_VOXELS / xy || xy * dz >= MAX_VOXELS) return MR_ERR_BAD_ARGUMENT;
    SparseGatherArgs a;
    a.table = table;
    a.pool = {const_cast<float*>(tsdf), const_cast<float*>(weight), reinterpret_cast<unsigned*>(const_cast<uint8_t*>(colour))};
    a.nbx = nbx; a.nby = nby;
    a.x0 = x0; a.y0 = y0; a.z0 = z0; a.dx = dx; a.dy = dy;
    a.voxels = xy * dz;
    a.tsdf = out_tsdf; a.weight = out_weight; a.colour = reinterpret_cast<unsigned*>(out_colour);
    long long grid = (a.voxels + 255) / 256;
    if (grid > 65536) grid = 65536;                                                      // grid-stride beyond that
    hipLaunchKernelGGL(tsdf_sparse_gather_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
