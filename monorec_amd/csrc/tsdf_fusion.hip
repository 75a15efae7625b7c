// TSDF fusion on the device (monorec_amd/tsdf_fusion.py): a dense voxel volume, the packed keyframes of mr_tsdf_frame_f32 integrated
// into it by running average, the zero-crossing surface out as points or as a welded triangle mesh.  The arithmetic is the one include/monorec_hip.h spells out -
// all fp32, every operation rounded on its own (compiled with -ffp-contract=off; `/` is the correctly rounded division) - and
// tests/tsdf_fusion_ref.py restates it in numpy; the GPU tests compare bit for bit.
//
//   tsdf_reset_kernel       tsdf = 1, weight = 0, colour = 0
//   tsdf_integrate_kernel   up to MR_TSDF_MAX_FRAMES keyframes per launch: a voxel is loaded once, updated by the frames in order in
//                           registers and stored once, and only by a thread one of whose voxels a frame updated
//   tsdf_mesh_vertices_kernel<3>   edge crossings on the three axis edges of a voxel as x y z r g b records (mr_tsdf_extract_f32); with
//                           no output it only counts
//   tsdf_mesh_vertices_kernel<7>, tsdf_mesh_triangles_kernel   the same surface as an indexed mesh (marching tetrahedra; further down):
//                           the same kernel over all seven edges a voxel owns, which also writes vertex_base, and the triangles
//   tsdf_mesh_vertex_normals_kernel   the <7> vertex tile code with the unit normal of every vertex beside its record
//   tsdf_mesh_cluster_vertices_kernel, tsdf_mesh_cluster_triangles_kernel   the mesh at a level of detail: one vertex per cluster of
//                           2^3, 4^3 or 8^3 voxels, the triangles between three different clusters (below the mesh kernels)
//   tsdf_skip_grid_kernel, tsdf_render_kernel   the volume seen from a camera (at the end)
// All but reset and render sweep the volume in one tile (tile_of_block); integrate and skip grid load a thread's four voxels with load_four.
//
// The integration sweeps the volume: 8 bytes (12 with colour) in and out per voxel and frame BATCH, the depth and colour images are
// gathered through the caches (a keyframe is a few hundred KB).  Measured kernel time (DESIGN.md section 7, 512 x 512 x 128 voxels,
// every voxel updated): 61 % of the achievable HBM rate at one frame per launch with colour, 70 % without; each further frame of a
// launch adds about 0.6 of the one-frame time and no volume traffic.  Shape of the sweep:
//   * a workgroup of 256 threads owns a tile of 32 x 8 x 4 voxels (MR_TSDF_TILE_X / _Y / _Z), a thread four voxels along x.  The 8
//     threads of a row move 128 contiguous bytes of tsdf and of weight - one whole cache line each where the row is aligned - and a
//     wave one z slice of 8 rows.  32 along x is the shortest row that fills a line; y and z are kept small so that the tile's
//     bounding sphere (radius 16 voxels, nearly all of it the x extent) stays tight for the culling, and so that volumes of a few
//     dozen voxels per side still spread over many workgroups.
//   * where a thread's four voxels are all inside the row and start on a 16-byte boundary they are one 16-byte load and store per
//     array; otherwise (odd nx, the tail of a row, a view that starts off the boundary) scalar accesses.  nx is arbitrary.
//   * culling: per frame five planes in world space (near and four sides, prepared by the host entry in double and pushed outwards),
//     tested against the tile's bounding sphere from blockIdx alone, so the test is uniform over the workgroup.  A tile all frames
//     skip returns before it has touched memory.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monorec_hip.h"
#include "tsdf_common.h"                     // the block-sparse volume's too: FrameArgs / frame_args, voxel update, edge masks, MAX_VOXELS, NO_ORIGIN, bad_output
#include "tsdf_mesh.h"                       // what its mesh runs too: the tetrahedron tables and the cases of a cube
#include "tsdf_render.h"                     // what its ray-cast (tsdf_sparse_render.hip) runs too: the ray, the cell, the clip, the pixel's outputs

namespace {

constexpr int TX = MR_TSDF_TILE_X, TY = MR_TSDF_TILE_Y, TZ = MR_TSDF_TILE_Z;
static_assert(TX == 32 && TY == 8 && TZ == 4, "256 threads, four voxels along x each");

struct IntegrateArgs {
    float* tsdf;
    float* weight;
    uint8_t* colour;                             // 4 bytes per voxel or null
    int nx, ny, nz;
    int tiles_x, tiles_y;
    FrameArgs fr;                                // the frames, their planes, the cull radius of a tile
};

__global__ __launch_bounds__(256) void tsdf_reset_kernel(float* __restrict__ tsdf, float* __restrict__ weight, unsigned* __restrict__ colour,
                                                         long long voxels) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < voxels; i += stride) {
        tsdf[i] = 1.0f;
        weight[i] = 0.0f;
        if (colour) colour[i] = 0u;
    }
}

// The workgroup's tile from blockIdx.  <TX, TY, TZ>: its first voxel; <1, 1, 1>: its index in tiles per axis, for the kernels that
// multiply at each use (they did before the decode was shared, and keep their instruction order that way).
struct Tile { int x, y, z; };

template <int UX, int UY, int UZ>
__device__ __forceinline__ Tile tile_of_block(int tiles_x, int tiles_y) {
    const int tile = blockIdx.x;
    return {(tile % tiles_x) * UX, ((tile / tiles_x) % tiles_y) * UY, (tile / (tiles_x * tiles_y)) * UZ};
}

// tsdf and weight of a thread's four voxels along x, of which the first n are in the row (1 and 0 for the rest): one 16-byte load per
// array where vec, else scalar loads.  Of the integrate and the skip-grid sweep.
__device__ __forceinline__ void load_four(const float* tp, const float* wp, int n, bool vec, float t[4], float wgt[4]) {
    if (vec) {
        const float4 tv = *reinterpret_cast<const float4*>(tp);
        const float4 wv = *reinterpret_cast<const float4*>(wp);
        t[0] = tv.x; t[1] = tv.y; t[2] = tv.z; t[3] = tv.w;
        wgt[0] = wv.x; wgt[1] = wv.y; wgt[2] = wv.z; wgt[3] = wv.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            t[j] = j < n ? tp[j] : 1.0f;
            wgt[j] = j < n ? wp[j] : 0.0f;
        }
    }
}

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const IntegrateArgs a) {
    const Tile b = tile_of_block<1, 1, 1>(a.tiles_x, a.tiles_y);
    // which frames can reach this tile: the centre of the (full) tile against the five planes of each frame
    const float ccx = a.fr.ox + ((float)(b.x * TX) + 0.5f * (TX - 1)) * a.fr.voxel;
    const float ccy = a.fr.oy + ((float)(b.y * TY) + 0.5f * (TY - 1)) * a.fr.voxel;
    const float ccz = a.fr.oz + ((float)(b.z * TZ) + 0.5f * (TZ - 1)) * a.fr.voxel;
    const unsigned live = live_frames(a.fr, ccx, ccy, ccz);
    if (live == 0) return;

    const int tid = threadIdx.x;
    const int x = b.x * TX + (tid & 7) * 4, y = b.y * TY + ((tid >> 3) & 7), z = b.z * TZ + (tid >> 6);
    if (x >= a.nx || y >= a.ny || z >= a.nz) return;
    const int n = a.nx - x < 4 ? a.nx - x : 4;
    const long long idx = ((long long)z * a.ny + y) * a.nx + x;
    float* tp = a.tsdf + idx;
    float* wp = a.weight + idx;
    unsigned* cp = a.colour ? reinterpret_cast<unsigned*>(a.colour) + idx : nullptr;
    const bool vec = n == 4 && (((uintptr_t)tp | (uintptr_t)wp) & 15) == 0;
    const bool cvec = n == 4 && ((uintptr_t)cp & 15) == 0;

    float t[4], wgt[4];
    unsigned col[4] = {0u, 0u, 0u, 0u};
    load_four(tp, wp, n, vec, t, wgt);
    if (cp) {
        if (cvec) {
            const uint4 cv = *reinterpret_cast<const uint4*>(cp);
            col[0] = cv.x; col[1] = cv.y; col[2] = cv.z; col[3] = cv.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (j < n) col[j] = cp[j];
        }
    }

    const FrameArgs& fr = a.fr;
    const float py = fr.oy + (float)y * fr.voxel, pz = fr.oz + (float)z * fr.voxel;
    const float wf = (float)fr.w, hf = (float)fr.h;
    unsigned touched = 0;
    bool band = false;                           // (the block-sparse volume's question; nobody asks here)
    for (int fi = 0; fi < fr.num_frames; ++fi) {
        if (!(live & (1u << fi))) continue;
        const mr_tsdf_view& f = fr.f[fi];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n) continue;
            const float px = fr.ox + (float)(x + j) * fr.voxel;
            tsdf_update_voxel(f, px, py, pz, fr.w, wf, hf, fr.trunc, fr.max_depth, cp != nullptr, t[j], wgt[j], col[j], touched, 1u << j, band);
        }
    }
    if (!touched) return;
    if (vec) {
        *reinterpret_cast<float4*>(tp) = make_float4(t[0], t[1], t[2], t[3]);
        *reinterpret_cast<float4*>(wp) = make_float4(wgt[0], wgt[1], wgt[2], wgt[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (touched & (1u << j)) { tp[j] = t[j]; wp[j] = wgt[j]; }
    }
    if (cp) {
        if (cvec) {
            *reinterpret_cast<uint4*>(cp) = make_uint4(col[0], col[1], col[2], col[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (touched & (1u << j)) cp[j] = col[j];
        }
    }
}

// ---- the surface: points on the grid's axis edges, or a welded triangle mesh by marching tetrahedra over the Kuhn split -------------
// (include/monorec_hip.h has the rules)
//
// The kernels give a workgroup of 256 threads the integrate kernel's tile of 32 x 8 x 4 voxels, a thread the four voxels (cubes) of
// one (x, y) column of it, and stage what the tile needs in LDS so that every value is read from memory once per workgroup, not once
// per edge or tetrahedron that touches it:
//   tsdf_mesh_vertices_kernel   tsdf (fp32) and a code byte (bit 0 seen, bit 1 seen and negative) of the tile plus one voxel beyond its
//                               high faces, 33 x 9 x 5 (7.4 KB): the far ends of the edges a voxel owns - all seven for the mesh, the
//                               three along the axes for the points, whose records are the mesh's vertices on those edges bit for bit
//   tsdf_mesh_triangles_kernel  the code byte alone for the tile plus TWO voxels, 34 x 10 x 6 (2 KB): a cube's tetrahedra use edges owned
//                               by its corners, and the rank of an edge among its owner's vertices needs the owner's whole mask, which
//                               reaches one voxel beyond the cube.  The masks of the 33 x 9 x 5 owners follow from the codes (1.5 KB).
// A tile whose staged block holds no seen negative voxel - nearly all of a fused volume: in front of every surface or never seen -
// leaves at the barrier that ends the staging (__syncthreads_or) and has touched neither its output, nor vertex_base, nor the cursor.
constexpr int VSX = TX + 1, VSY = TY + 1, VSZ = TZ + 1, VSN = VSX * VSY * VSZ;           // staged block of the vertex kernel
constexpr int CSX = TX + 2, CSY = TY + 2, CSZ = TZ + 2, CSN = CSX * CSY * CSZ;           // staged codes of the triangle kernel

struct MeshArgs {
    const float* tsdf;
    const float* weight;
    const unsigned* colour;                      // vertices only; r g b 0 per voxel or null
    int nx, ny, nz;
    int tiles_x, tiles_y;
    float ox, oy, oz, voxel, min_weight;
    float* vertices;                             // null: count only
    int* vertex_base;                            // written by the 7-edge vertex kernel, read by the triangle kernel
    int* triangles;                              // null: count only
    long long capacity;
    unsigned long long* cursor;
};

// is voxel (x, y, z) inside the volume and seen?  Then t is its tsdf: what the normals ask of the volume (voxel_gradient, tsdf_mesh.h)
struct VolumeSample {
    const MeshArgs& a;
    __device__ __forceinline__ bool operator()(int x, int y, int z, float& t) const {
        if ((unsigned)x >= (unsigned)a.nx || (unsigned)y >= (unsigned)a.ny || (unsigned)z >= (unsigned)a.nz) return false;
        const long long g = ((long long)z * a.ny + y) * a.nx + x;
        if (!(a.weight[g] > a.min_weight)) return false;
        t = a.tsdf[g];
        return true;
    }
};

// EDGES = 7: the vertices of the mesh, and vertex_base.  EDGES = 3: the axis edges alone, the points of mr_tsdf_extract_f32; nothing
// of it indexes with int32, so it serves volumes past 2^31 voxels.
// NORMALS (the variant tsdf_mesh_vertex_normals_kernel alone): the unit normal of every vertex into normals[3 * index], its gradients
// read from the volume, not from the staged block - they reach a voxel further on every side.
template <int EDGES, bool NORMALS>
__device__ __forceinline__ void mesh_vertices_tile(const MeshArgs& a, float* normals) {
    static_assert(EDGES == 3 || EDGES == 7, "the axis edges, or all a voxel owns");
    __shared__ float s_t[VSN];
    __shared__ uint8_t s_code[VSN];
    __shared__ int wave_tot[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const Tile o = tile_of_block<TX, TY, TZ>(a.tiles_x, a.tiles_y);
    const int x0 = o.x, y0 = o.y, z0 = o.z;
    const long long plane = (long long)a.nx * a.ny;
    int any_neg = 0;
    for (int i = tid; i < VSN; i += 256) {
        const int sx = i % VSX, sy = (i / VSX) % VSY, sz = i / (VSX * VSY);
        const int gx = x0 + sx, gy = y0 + sy, gz = z0 + sz;
        float t = 1.0f;
        unsigned c = 0u;
        if (gx < a.nx && gy < a.ny && gz < a.nz) {
            const long long g = (long long)gz * plane + (long long)gy * a.nx + gx;
            if (a.weight[g] > a.min_weight) {
                t = a.tsdf[g];
                c = t < 0.0f ? (SEEN | NEG) : SEEN;
            }
        }
        s_t[i] = t;
        s_code[i] = (uint8_t)c;
        any_neg |= (int)(c & NEG);
    }
    if (!__syncthreads_or(any_neg)) return;

    const int lx = tid & 31, ly = tid >> 5;
    unsigned masks = 0;                          // the masks of the thread's four voxels, a byte each
#pragma unroll
    for (int j = 0; j < TZ; ++j) masks |= edge_mask<EDGES>(s_code, (j * VSY + ly) * VSX + lx, VSX, VSX * VSY) << (8 * j);
    const int mine = __popc(masks);
    int total;
    const int before = workgroup_prefix(mine, wave_tot, total);
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(a.cursor, (unsigned long long)total);       // one per workgroup
    if (!a.vertices) return;
    __syncthreads();
    if (!masks) return;
    long long rec = (long long)s_base + before;
    const int gx = x0 + lx, gy = y0 + ly;        // inside the volume: a voxel outside it has no code, hence no mask
    const float px = a.ox + (float)gx * a.voxel, py = a.oy + (float)gy * a.voxel;
    const int s_far[7] = {1, VSX, VSX * VSY, 1 + VSX, 1 + VSX * VSY, VSX + VSX * VSY, 1 + VSX + VSX * VSY};
    const long long g_far[7] = {1, a.nx, plane, 1 + a.nx, 1 + plane, a.nx + plane, 1 + a.nx + plane};
    constexpr unsigned along[7] = {1u, 2u, 4u, 3u, 5u, 6u, 7u};                   // bit k: the edge advances along axis k
#pragma unroll
    for (int j = 0; j < TZ; ++j) {
        const unsigned mask = (masks >> (8 * j)) & 0xffu;
        if (!mask) continue;
        const int gz = z0 + j, at = (j * VSY + ly) * VSX + lx;
        const long long g = (long long)gz * plane + (long long)gy * a.nx + gx;
        if constexpr (EDGES == 7) a.vertex_base[g] = (int)rec;
        const float p[3] = {px, py, a.oz + (float)gz * a.voxel};
        const float tv = s_t[at];
        const unsigned cv = a.colour ? a.colour[g] : 0u;
#pragma unroll
        for (int e = 0; e < EDGES; ++e) {
            if (!(mask & (1u << e))) continue;
            if (rec < a.capacity) {
                const float s = tv / (tv - s_t[at + s_far[e]]);
                const float step = s * a.voxel;
                float* r = a.vertices + rec * 6;
#pragma unroll
                for (int k = 0; k < 3; ++k) r[k] = (along[e] >> k) & 1u ? p[k] + step : p[k];
                write_colour(r, cv, a.colour ? a.colour[g + g_far[e]] : 0u, s);
                if constexpr (NORMALS) vertex_normal(VolumeSample{a}, gx, gy, gz, tv, e, s_t[at + s_far[e]], s, normals + rec * 3);
            }
            ++rec;
        }
    }
}

template <int EDGES>
__global__ __launch_bounds__(256) void tsdf_mesh_vertices_kernel(const MeshArgs a) { mesh_vertices_tile<EDGES, false>(a, nullptr); }

__global__ __launch_bounds__(256) void tsdf_mesh_vertex_normals_kernel(const MeshArgs a, float* normals) { mesh_vertices_tile<7, true>(a, normals); }

__global__ __launch_bounds__(256) void tsdf_mesh_triangles_kernel(const MeshArgs a) {
    __shared__ uint8_t s_code[CSN];
    __shared__ uint8_t s_mask[VSN];
    __shared__ int wave_tot[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const Tile o = tile_of_block<TX, TY, TZ>(a.tiles_x, a.tiles_y);
    const int x0 = o.x, y0 = o.y, z0 = o.z;
    const long long plane = (long long)a.nx * a.ny;
    int any_neg = 0;
    for (int i = tid; i < CSN; i += 256) {
        const int sx = i % CSX, sy = (i / CSX) % CSY, sz = i / (CSX * CSY);
        const int gx = x0 + sx, gy = y0 + sy, gz = z0 + sz;
        unsigned c = 0u;
        if (gx < a.nx && gy < a.ny && gz < a.nz) {
            const long long g = (long long)gz * plane + (long long)gy * a.nx + gx;
            if (a.weight[g] > a.min_weight) c = a.tsdf[g] < 0.0f ? (SEEN | NEG) : SEEN;
        }
        s_code[i] = (uint8_t)c;
        if (sx < VSX && sy < VSY && sz < VSZ) any_neg |= (int)(c & NEG);          // the corners of the tile's cubes
    }
    if (!__syncthreads_or(any_neg)) return;

    const int lx = tid & 31, ly = tid >> 5;
    unsigned cases[TZ];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < TZ; ++j) {
        cases[j] = cube_cases(s_code, (j * CSY + ly) * CSX + lx, CSX, CSX * CSY);
#pragma unroll
        for (int t = 0; t < 6; ++t) mine += (int)(TET_CASES[(cases[j] >> (4 * t)) & 15u] & 15u);
    }
    int total;
    const int before = workgroup_prefix(mine, wave_tot, total);
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(a.cursor, (unsigned long long)total);       // one per workgroup
    if (!a.triangles) return;
    for (int i = tid; i < VSN; i += 256) {
        const int sx = i % VSX, sy = (i / VSX) % VSY, sz = i / (VSX * VSY);
        s_mask[i] = (uint8_t)edge_mask<7>(s_code, (sz * CSY + sy) * CSX + sx, CSX, CSX * CSY);
    }
    __syncthreads();
    if (!mine) return;
    long long tri = (long long)s_base + before;
    const auto m_unit = [](int k) { return k == 0 ? 1 : k == 1 ? VSX : VSX * VSY; };
    const auto g_unit = [&](int k) { return k == 0 ? 1ll : k == 1 ? (long long)a.nx : plane; };
#pragma unroll
    for (int j = 0; j < TZ; ++j) {
        if (!cases[j]) continue;
        const int m0 = (j * VSY + ly) * VSX + lx;
        const long long g0 = (long long)(z0 + j) * plane + (long long)(y0 + ly) * a.nx + (x0 + lx);
#pragma unroll 1
        for (int t = 0; t < 6; ++t) {
            unsigned word = TET_CASES[(cases[j] >> (4 * t)) & 15u];
            const int count = (int)(word & 15u);
            if (!count) continue;
            const unsigned perm = TET_PERMS[t];
            const int pa = perm & 3u, pb = (perm >> 2) & 3u, pc = (perm >> 4) & 3u;
            // owner (as a step from c0 in the mask block and in the volume) and edge type of the tetrahedron's six edges
            const int m_own[3] = {m0, m0 + m_unit(pa), m0 + m_unit(pa) + m_unit(pb)};
            const long long g_own[3] = {g0, g0 + g_unit(pa), g0 + g_unit(pa) + g_unit(pb)};
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

// ---- the clustered level of detail: one vertex per cluster of cell^3 voxels that owns a vertex of the full mesh, the full mesh's
// triangles between three different clusters (include/monorec_hip.h has the rules, tsdf_mesh.h the code the sparse volume runs too)
//   tsdf_mesh_cluster_vertices_kernel   a workgroup owns MR_TSDF_CLUSTER_TILE_X x _Y x _Z = 32 x 8 x 8 voxels - whole clusters for every
//                               cell - and stages tsdf and codes of the tile plus one voxel beyond its high faces (33 x 9 x 9, 13 KB) as
//                               the vertex kernel does, then the masks of its voxels.  The tile is 256 runs of 8 voxels for every cell
//                               (tsdf_mesh.h): a lane sums the vertices of one run in the fixed order, the run sums go through LDS
//                               (in the place of the staged tsdf) and the first lane of each cluster - 256, 32 or 4 of them - adds its 1, 8 or 64 runs in
//                               order; no atomics but the one on the cursor per workgroup.  It writes cluster_base.
//   tsdf_mesh_cluster_triangles_kernel  the triangle kernel's tile, cases and walk over the codes of the tile plus ONE voxel (no masks:
//                               a vertex is its owner's cluster), the count over the triangles that survive
constexpr int KX = MR_TSDF_CLUSTER_TILE_X, KY = MR_TSDF_CLUSTER_TILE_Y, KZ = MR_TSDF_CLUSTER_TILE_Z;
constexpr int KSX = KX + 1, KSY = KY + 1, KSZ = KZ + 1, KSN = KSX * KSY * KSZ;
static_assert(KX == 32 && KY == 8 && KZ == 8 && KX % B == 0 && KY % B == 0 && KZ % B == 0, "2048 voxels: 256, 32 or 4 whole clusters");
static_assert(KSN >= 10 * 256, "the run sums (9 floats and a count per run) take the place of the staged tsdf");

struct ClusterArgs {
    float* normals;                              // vertices only; null: none
    int* cluster_base;                           // written by the vertex kernel, read by the triangle kernel
    int shift;                                   // cell = 1 << shift
    int cx, cy;                                  // clusters of the volume along x and y
};

template <bool NORMALS>
__global__ __launch_bounds__(256) void tsdf_mesh_cluster_vertices_kernel(const MeshArgs a, const ClusterArgs k) {
    __shared__ float s_t[KSN];
    __shared__ uint8_t s_code[KSN];
    __shared__ uint8_t s_mask[KSN];
    __shared__ uint8_t s_owns[256];
    __shared__ int wave_tot[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const Tile o = tile_of_block<KX, KY, KZ>(a.tiles_x, a.tiles_y);
    const int x0 = o.x, y0 = o.y, z0 = o.z;
    const long long plane = (long long)a.nx * a.ny;
    int any_neg = 0;
    for (int i = tid; i < KSN; i += 256) {
        const int sx = i % KSX, sy = (i / KSX) % KSY, sz = i / (KSX * KSY);
        const int gx = x0 + sx, gy = y0 + sy, gz = z0 + sz;
        float t = 1.0f;
        unsigned c = 0u;
        if (gx < a.nx && gy < a.ny && gz < a.nz) {
            const long long g = (long long)gz * plane + (long long)gy * a.nx + gx;
            if (a.weight[g] > a.min_weight) {
                t = a.tsdf[g];
                c = t < 0.0f ? (SEEN | NEG) : SEEN;
            }
        }
        s_t[i] = t;
        s_code[i] = (uint8_t)c;
        any_neg |= (int)(c & NEG);
    }
    if (!__syncthreads_or(any_neg)) return;
    for (int i = tid; i < KX * KY * KZ; i += 256) {
        const int at = ((i / (KX * KY)) * KSY + (i / KX) % KY) * KSX + i % KX;
        s_mask[at] = (uint8_t)edge_mask<7>(s_code, at, KSX, KSX * KSY);
    }
    __syncthreads();

    // the thread's run: the tile has 256 runs of 8 voxels for every cell; run `run` of cluster q of the tile's is on thread q * runs + run
    const int sh = k.shift;
    const int qnx = KX >> sh, qny = KY >> sh, runs = (1 << (3 * sh)) / RUN;
    const int q = tid / runs, run = tid % runs;
    const int lx = (q % qnx) << sh, ly = ((q / qnx) % qny) << sh, lz = (q / (qnx * qny)) << sh;      // the cluster's first voxel in the tile
    const int at0 = (lz * KSY + ly) * KSX + lx;
    const int owns = run_owns(s_mask, at0, KSX, KSX * KSY, sh, run);
    s_owns[tid] = (uint8_t)owns;
    __syncthreads();
    int has = 0;                                 // of the lane of the cluster's first run: does the cluster own a vertex?
    if (run == 0)
        for (int r = 0; r < runs; ++r) has |= s_owns[tid + r];
    int total;
    const int before = workgroup_prefix(has, wave_tot, total);
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(a.cursor, (unsigned long long)total);       // one per workgroup
    if (!a.vertices) return;
    constexpr int N = NORMALS ? 9 : 6;
    float sum[N];
    int count = 0;
    if (owns) {
        const auto vertex = [&](int dx, int dy, int dz, int at, int e, float* r) {
            const int gx = x0 + lx + dx, gy = y0 + ly + dy, gz = z0 + lz + dz;
            const long long g = (long long)gz * plane + (long long)gy * a.nx + gx;
            const int far = (int)(EDGE_ALONG[e] & 1u) + (int)((EDGE_ALONG[e] >> 1) & 1u) * KSX + (int)(EDGE_ALONG[e] >> 2) * (KSX * KSY);
            const long long g_far = (long long)(EDGE_ALONG[e] & 1u) + (long long)((EDGE_ALONG[e] >> 1) & 1u) * a.nx + (long long)(EDGE_ALONG[e] >> 2) * plane;
            const float p[3] = {a.ox + (float)gx * a.voxel, a.oy + (float)gy * a.voxel, a.oz + (float)gz * a.voxel};
            const float tv = s_t[at], tn = s_t[at + far];
            const float s = edge_record(tv, tn, p, e, a.voxel, a.colour ? a.colour[g] : 0u, a.colour ? a.colour[g + g_far] : 0u, r);
            if constexpr (NORMALS) vertex_normal(VolumeSample{a}, gx, gy, gz, tv, e, tn, s, r + 6);
        };
        count = run_sum<NORMALS>(s_mask, at0, KSX, KSX * KSY, sh, run, sum, vertex);
    }
    // the sums of the runs and, last, their counts go through LDS as [sum][run], in the place of the staged tsdf, which every lane has
    // finished reading
    __syncthreads();
    float* s_part = s_t;
#pragma unroll
    for (int c = 0; c < N; ++c) s_part[c * 256 + tid] = owns ? sum[c] : 0.0f;
    s_part[N * 256 + tid] = (float)count;
    __syncthreads();                             // (also: s_base is there)
    if (!has) return;
    const long long rec = (long long)s_base + before;
    // (a cluster that owns a vertex holds a voxel of the volume: its place in cluster_base exists)
    k.cluster_base[((long long)((z0 + lz) >> sh) * k.cy + ((y0 + ly) >> sh)) * k.cx + ((x0 + lx) >> sh)] = (int)rec;
    if (rec >= a.capacity) return;
    float out[9];
    cluster_combine<NORMALS>(s_part + tid, 256, runs, out);
#pragma unroll
    for (int c = 0; c < 6; ++c) a.vertices[rec * 6 + c] = out[c];
    if constexpr (NORMALS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) k.normals[rec * 3 + c] = out[6 + c];
    }
}

__global__ __launch_bounds__(256) void tsdf_mesh_cluster_triangles_kernel(const MeshArgs a, const ClusterArgs k) {
    __shared__ uint8_t s_code[VSN];
    __shared__ int wave_tot[4];
    __shared__ unsigned long long s_base;
    const int tid = threadIdx.x;
    const Tile o = tile_of_block<TX, TY, TZ>(a.tiles_x, a.tiles_y);
    const int x0 = o.x, y0 = o.y, z0 = o.z;
    const long long plane = (long long)a.nx * a.ny;
    int any_neg = 0;
    for (int i = tid; i < VSN; i += 256) {
        const int sx = i % VSX, sy = (i / VSX) % VSY, sz = i / (VSX * VSY);
        const int gx = x0 + sx, gy = y0 + sy, gz = z0 + sz;
        unsigned c = 0u;
        if (gx < a.nx && gy < a.ny && gz < a.nz) {
            const long long g = (long long)gz * plane + (long long)gy * a.nx + gx;
            if (a.weight[g] > a.min_weight) c = a.tsdf[g] < 0.0f ? (SEEN | NEG) : SEEN;
        }
        s_code[i] = (uint8_t)c;
        any_neg |= (int)(c & NEG);
    }
    if (!__syncthreads_or(any_neg)) return;

    const int lx = tid & 31, ly = tid >> 5, sh = k.shift;
    unsigned cases[TZ];
    int mine = 0;
#pragma unroll
    for (int j = 0; j < TZ; ++j) {
        cases[j] = cube_cases(s_code, (j * VSY + ly) * VSX + lx, VSX, VSX * VSY);
        if (!cases[j]) continue;
        const auto cid = [&](int dx, int dy, int dz) {           // below the voxel count: below 2^31
            return (int)(((long long)((z0 + j + dz) >> sh) * k.cy + ((y0 + ly + dy) >> sh)) * k.cx + ((x0 + lx + dx) >> sh));
        };
        cluster_cube_triangles(cases[j], cid, [&](int, int, int) { ++mine; });
    }
    int total;
    const int before = workgroup_prefix(mine, wave_tot, total);
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(a.cursor, (unsigned long long)total);       // one per workgroup
    if (!a.triangles) return;
    __syncthreads();
    if (!mine) return;
    long long tri = (long long)s_base + before;
#pragma unroll
    for (int j = 0; j < TZ; ++j) {
        if (!cases[j]) continue;
        const auto cid = [&](int dx, int dy, int dz) {
            return (int)(((long long)((z0 + j + dz) >> sh) * k.cy + ((y0 + ly + dy) >> sh)) * k.cx + ((x0 + lx + dx) >> sh));
        };
        cluster_cube_triangles(cases[j], cid, [&](int va, int vb, int vc) {
            if (tri < a.capacity) {
                int* r = a.triangles + tri * 3;
                r[0] = k.cluster_base[va]; r[1] = k.cluster_base[vb]; r[2] = k.cluster_base[vc];
            }
            ++tri;
        });
    }
}

long long voxel_count(int nx, int ny, int nz) {                // MAX_VOXELS for anything at or beyond the bound, without overflow
    const long long xy = (long long)nx * ny;                     // < 2^62
    if (xy >= MAX_VOXELS || nz > MAX_VOXELS / xy) return MAX_VOXELS;
    return xy * nz;
}

// The checks the entries share: the volume, and - where an entry takes them; the defaults pass - origin, voxel_size and min_weight.
bool bad_volume(const void* tsdf, const void* weight, const void* colour, int nx, int ny, int nz, const float* origin = NO_ORIGIN,
                float voxel_size = 1.0f, float min_weight = 0.0f) {
    if (!tsdf || !weight || nx < 1 || ny < 1 || nz < 1 || !origin) return true;
    if (((uintptr_t)tsdf | (uintptr_t)weight | (uintptr_t)colour) & 3) return true;
    if (!(voxel_size > 0.0f) || min_weight != min_weight) return true;
    return voxel_count(nx, ny, nz) >= MAX_VOXELS;
}

// The tiles per axis of a sweep and the launch's grid; 0 when that does not fit 2^31 - 1.  For a checked volume (under 2^40 voxels).
unsigned tile_grid(int nx, int ny, int nz, int& tiles_x, int& tiles_y) {
    tiles_x = (nx - 1) / TX + 1; tiles_y = (ny - 1) / TY + 1;
    const long long tiles = (long long)tiles_x * tiles_y * ((nz - 1) / TZ + 1);
    return tiles > 0x7fffffffLL ? 0u : (unsigned)tiles;
}

}  // namespace

extern "C" int mr_tsdf_volume_reset_f32(float* tsdf, float* weight, uint8_t* colour, int32_t nx, int32_t ny, int32_t nz, void* stream) {
    if (bad_volume(tsdf, weight, colour, nx, ny, nz)) return MR_ERR_BAD_ARGUMENT;
    const long long voxels = voxel_count(nx, ny, nz);
    long long blocks = (voxels + 255) / 256;
    if (blocks > 65536) blocks = 65536;                          // grid-stride beyond that
    hipLaunchKernelGGL(tsdf_reset_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tsdf, weight,
                       reinterpret_cast<unsigned*>(colour), voxels);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_integrate_f32(float* tsdf, float* weight, uint8_t* colour, int32_t nx, int32_t ny, int32_t nz, const float* origin,
                                     float voxel_size, float trunc, float max_depth_m, const mr_tsdf_view* frames, int32_t num_frames,
                                     int32_t height, int32_t width, void* stream) {
    if (bad_volume(tsdf, weight, colour, nx, ny, nz, origin, voxel_size)) return MR_ERR_BAD_ARGUMENT;
    IntegrateArgs a;
    // the sphere round the voxel CENTRES of a full tile; the tiles reach up to TX voxels beyond the volume
    const double voxels[3] = {(double)nx, (double)ny, (double)nz};
    const double radius = 0.5 * (double)voxel_size * sqrt((double)((TX - 1) * (TX - 1) + (TY - 1) * (TY - 1) + (TZ - 1) * (TZ - 1)));
    if (frame_args(a.fr, origin, voxel_size, trunc, max_depth_m, frames, num_frames, height, width, colour != nullptr, voxels, TX, radius) < 0.0)
        return MR_ERR_BAD_ARGUMENT;
    a.tsdf = tsdf; a.weight = weight; a.colour = colour;
    a.nx = nx; a.ny = ny; a.nz = nz;
    const unsigned tiles = tile_grid(nx, ny, nz, a.tiles_x, a.tiles_y);
    if (!tiles) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

namespace {

// What the three surface entries share: the checks of volume, output and cursor, the kernels' arguments and, in `tiles`, the grid.
// The triangle entry has no colour and no positions (NO_ORIGIN, a voxel of 1).  True: a bad argument.
bool surface_args(MeshArgs& a, unsigned& tiles, const float* tsdf, const float* weight, const uint8_t* colour, int nx, int ny, int nz,
                  const float* origin, float voxel_size, float min_weight, const void* out, long long capacity, int64_t* cursor) {
    if (bad_volume(tsdf, weight, colour, nx, ny, nz, origin, voxel_size, min_weight)) return true;
    if (bad_output(out, capacity, cursor)) return true;
    if (nx > 0x7fffffff - CSX || ny > 0x7fffffff - CSY || nz > 0x7fffffff - CSZ) return true;   // x0 + sx of a staged block stays an int
    a.tsdf = tsdf; a.weight = weight; a.colour = reinterpret_cast<const unsigned*>(colour);
    a.nx = nx; a.ny = ny; a.nz = nz;
    a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2]; a.voxel = voxel_size; a.min_weight = min_weight;
    a.vertices = nullptr; a.triangles = nullptr; a.vertex_base = nullptr;
    a.capacity = out ? capacity : 0;
    a.cursor = reinterpret_cast<unsigned long long*>(cursor);
    tiles = tile_grid(nx, ny, nz, a.tiles_x, a.tiles_y);
    return tiles == 0;
}

// beyond those, of the two mesh entries (a checked volume): vertex indices are int32, and an output needs vertex_base
bool bad_mesh(int nx, int ny, int nz, const void* vertex_base, const void* out) {
    return voxel_count(nx, ny, nz) >= (1ll << 31) || ((uintptr_t)vertex_base & 3) || (out && !vertex_base);
}

}  // namespace

extern "C" int mr_tsdf_extract_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny, int32_t nz,
                                   const float* origin, float voxel_size, float min_weight, float* records, int64_t capacity_records,
                                   int64_t* cursor, void* stream) {
    MeshArgs a;
    unsigned tiles;
    if (surface_args(a, tiles, tsdf, weight, colour, nx, ny, nz, origin, voxel_size, min_weight, records, capacity_records, cursor))
        return MR_ERR_BAD_ARGUMENT;
    a.vertices = records;
    hipLaunchKernelGGL(tsdf_mesh_vertices_kernel<3>, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_mesh_vertices_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny, int32_t nz,
                                         const float* origin, float voxel_size, float min_weight, float* vertices, int64_t capacity_vertices,
                                         int32_t* vertex_base, int64_t* cursor, void* stream) {
    MeshArgs a;
    unsigned tiles;
    if (surface_args(a, tiles, tsdf, weight, colour, nx, ny, nz, origin, voxel_size, min_weight, vertices, capacity_vertices, cursor) ||
        bad_mesh(nx, ny, nz, vertex_base, vertices))
        return MR_ERR_BAD_ARGUMENT;
    a.vertices = vertices; a.vertex_base = vertex_base;
    hipLaunchKernelGGL(tsdf_mesh_vertices_kernel<7>, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_mesh_triangles_f32(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float min_weight,
                                          const int32_t* vertex_base, int32_t* triangles, int64_t capacity_triangles, int64_t* cursor,
                                          void* stream) {
    MeshArgs a;
    unsigned tiles;
    if (surface_args(a, tiles, tsdf, weight, nullptr, nx, ny, nz, NO_ORIGIN, 1.0f, min_weight, triangles, capacity_triangles, cursor) ||
        bad_mesh(nx, ny, nz, vertex_base, triangles))
        return MR_ERR_BAD_ARGUMENT;
    a.triangles = triangles; a.vertex_base = const_cast<int*>(vertex_base);
    hipLaunchKernelGGL(tsdf_mesh_triangles_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_mesh_vertices_normals_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny,
                                                 int32_t nz, const float* origin, float voxel_size, float min_weight, float* vertices,
                                                 int64_t capacity_vertices, float* normals, int32_t* vertex_base, int64_t* cursor,
                                                 void* stream) {
    MeshArgs a;
    unsigned tiles;
    if (surface_args(a, tiles, tsdf, weight, colour, nx, ny, nz, origin, voxel_size, min_weight, vertices, capacity_vertices, cursor) ||
        bad_mesh(nx, ny, nz, vertex_base, vertices) || ((uintptr_t)normals & 3) || (!vertices != !normals))
        return MR_ERR_BAD_ARGUMENT;
    a.vertices = vertices; a.vertex_base = vertex_base;
    hipLaunchKernelGGL(tsdf_mesh_vertex_normals_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a, normals);
    return (int)hipGetLastError();
}

namespace {

// beyond surface_args and bad_mesh, of the two cluster entries: the cell and the clusters per axis.  True: a bad argument.
bool cluster_args(ClusterArgs& k, int cell, int nx, int ny, int* cluster_base) {
    k.shift = cluster_shift(cell);
    if (k.shift < 0) return true;
    k.normals = nullptr; k.cluster_base = cluster_base;
    k.cx = (nx - 1) / cell + 1; k.cy = (ny - 1) / cell + 1;
    return false;
}

}  // namespace

extern "C" int mr_tsdf_mesh_cluster_vertices_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny,
                                                 int32_t nz, const float* origin, float voxel_size, float min_weight, int32_t cell,
                                                 float* vertices, int64_t capacity_vertices, float* normals, int32_t* cluster_base,
                                                 int64_t* cursor, void* stream) {
    MeshArgs a;
    ClusterArgs k;
    unsigned tiles;
    if (surface_args(a, tiles, tsdf, weight, colour, nx, ny, nz, origin, voxel_size, min_weight, vertices, capacity_vertices, cursor) ||
        bad_mesh(nx, ny, nz, cluster_base, vertices) || cluster_args(k, cell, nx, ny, cluster_base) || ((uintptr_t)normals & 3) ||
        (normals && !vertices) || nz > 0x7fffffff - KSZ)
        return MR_ERR_BAD_ARGUMENT;
    a.vertices = vertices;
    k.normals = vertices ? normals : nullptr;
    a.tiles_x = (nx - 1) / KX + 1; a.tiles_y = (ny - 1) / KY + 1;                        // no more tiles than surface_args counted
    tiles = (unsigned)((long long)a.tiles_x * a.tiles_y * ((nz - 1) / KZ + 1));
    if (k.normals) hipLaunchKernelGGL(tsdf_mesh_cluster_vertices_kernel<true>, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a, k);
    else hipLaunchKernelGGL(tsdf_mesh_cluster_vertices_kernel<false>, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a, k);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_mesh_cluster_triangles_f32(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz,
                                                  float min_weight, int32_t cell, const int32_t* cluster_base, int32_t* triangles,
                                                  int64_t capacity_triangles, int64_t* cursor, void* stream) {
    MeshArgs a;
    ClusterArgs k;
    unsigned tiles;
    if (surface_args(a, tiles, tsdf, weight, nullptr, nx, ny, nz, NO_ORIGIN, 1.0f, min_weight, triangles, capacity_triangles, cursor) ||
        bad_mesh(nx, ny, nz, cluster_base, triangles) || cluster_args(k, cell, nx, ny, const_cast<int*>(cluster_base)))
        return MR_ERR_BAD_ARGUMENT;
    a.triangles = triangles;
    hipLaunchKernelGGL(tsdf_mesh_cluster_triangles_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a, k);
    return (int)hipGetLastError();
}

// ---- the volume seen from a camera: ray-cast depth, normal and colour (include/monorec_hip.h has the arithmetic) --------------------
//
// tsdf_skip_grid_kernel   one byte per brick of MR_TSDF_BRICK^3 voxels (plus a voxel of halo on the + side): does it hold a seen negative
//                         voxel?  The integrate kernel's tile and 16-byte loads; a thread that finds one stores 1 into the (up to
//                         eight) bricks whose inclusive range holds it.  The bytes are cleared by a memset ahead of the launch; every
//                         store writes the same value, so their order does not matter.
// tsdf_render_kernel      a thread per pixel, a wave a compact 8 x 8 pixel tile, a workgroup 16 x 16 pixels of one view (blockIdx.z):
//                         neighbouring rays walk neighbouring cells, so the 16 gathers of a sample (8 corner weights, 8 corner tsdf)
//                         of a wave fall into few cache lines.  A ray is clipped to the volume's box, then marched; with the bricks a
//                         sample in an empty brick costs one byte load (the grid of a 512 x 512 x 128 volume is 512 KB: it stays in
//                         cache).
namespace {

constexpr int BRICK = MR_TSDF_BRICK;
static_assert(BRICK % 4 == 0 && BRICK >= 4, "the four voxels of a thread of the skip-grid sweep share a brick");

struct SkipArgs {
    const float* tsdf;
    const float* weight;
    int nx, ny, nz;
    int tiles_x, tiles_y;
    int bricks_x, bricks_y;
    float min_weight;
    uint8_t* bricks;
};

__global__ __launch_bounds__(256) void tsdf_skip_grid_kernel(const SkipArgs a) {
    const int tid = threadIdx.x;
    const Tile b = tile_of_block<1, 1, 1>(a.tiles_x, a.tiles_y);
    const int x = b.x * TX + (tid & 7) * 4, y = b.y * TY + ((tid >> 3) & 7), z = b.z * TZ + (tid >> 6);
    if (x >= a.nx || y >= a.ny || z >= a.nz) return;
    const int n = a.nx - x < 4 ? a.nx - x : 4;
    const long long idx = ((long long)z * a.ny + y) * a.nx + x;
    const float* tp = a.tsdf + idx;
    const float* wp = a.weight + idx;
    float t[4], wgt[4];
    load_four(tp, wp, n, n == 4 && (((uintptr_t)tp | (uintptr_t)wp) & 15) == 0, t, wgt);
    bool any = false, first = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool neg = wgt[j] > a.min_weight && t[j] < 0.0f;
        any = any || neg;
        if (j == 0) first = neg;
    }
    if (!any) return;
    // x .. x + 3 lie in brick x / BRICK; voxel B b also closes the inclusive range of brick b - 1
    const int bx = x / BRICK, by = y / BRICK, bz = z / BRICK;
    const int lx = (first && x % BRICK == 0 && bx > 0) ? 1 : 0, ly = (y % BRICK == 0 && by > 0) ? 1 : 0, lz = (z % BRICK == 0 && bz > 0) ? 1 : 0;
    for (int dz = 0; dz <= lz; ++dz)
        for (int dy = 0; dy <= ly; ++dy)
            for (int dx = 0; dx <= lx; ++dx)
                a.bricks[((long long)(bz - dz) * a.bricks_y + (by - dy)) * a.bricks_x + (bx - dx)] = 1;
}

struct RenderArgs {
    const float* tsdf;
    const float* weight;
    const unsigned* colour;                      // r g b 0 per voxel or null
    const uint8_t* bricks;                       // null: every sample is evaluated
    int nx, ny, nz;
    int bricks_x, bricks_y;
    float lim[3];                                // the largest float <= n_a - 2: the last cell base along each axis
    float inv, min_weight, t_min, step;
    int last;                                    // index of the last sample with t_k <= t_max
    int h, w, tiles_x;
    RayView v[MR_TSDF_MAX_FRAMES];
};

// the 8 corner tsdf of an inside cell into T; false when a corner's weight is not above min_weight
__device__ __forceinline__ bool corners_of(const RenderArgs& a, const Cell& c, float T[8], long long& base) {
    const long long plane = (long long)a.nx * a.ny;
    base = (long long)c.i[2] * plane + (long long)c.i[1] * a.nx + c.i[0];
    float W[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long long at = base + (j & 1) + ((j >> 1) & 1) * (long long)a.nx + (j >> 2) * plane;
        W[j] = a.weight[at];
        T[j] = a.tsdf[at];
    }
    bool seen = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) seen = seen && (W[j] > a.min_weight);
    return seen;
}

__global__ __launch_bounds__(256) void tsdf_render_kernel(const RenderArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = (blockIdx.x % a.tiles_x) * 16 + (wave & 1) * 8 + (lane & 7);
    const int v = (blockIdx.x / a.tiles_x) * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (u >= a.w || v >= a.h) return;
    const RayView& view = a.v[blockIdx.z];
    float o[3], e[3];
    ray_of_pixel(a, view, u, v, o, e);
    int k_lo, k_hi;
    clip_to_box(a, o, e, k_lo, k_hi);

    // prev: 0 not valid, 1 valid with F_prev, 2 skipped (in a brick of byte 0: not valid, or valid and not negative - evaluated in full
    // before the next sample that is)
    int prev = 0, hit_k = -1;
    float F_prev = 0.0f, F_hit = 0.0f, T[8], f[3] = {0.0f, 0.0f, 0.0f};
    long long base = 0;
    for (int k = k_lo; k <= k_hi; ++k) {
        const Cell c = cell_of(a, o, e, k);
        if (!c.inside) { prev = 0; continue; }
        if (a.bricks && !(prev == 1 && F_prev < 0.0f)) {                   // never skip behind a negative sample: the back-face stop
            const long long b = ((long long)(c.i[2] / BRICK) * a.bricks_y + c.i[1] / BRICK) * a.bricks_x + c.i[0] / BRICK;
            if (!a.bricks[b]) { prev = 2; continue; }
        }
        if (prev == 2) {                                                    // k - 1 was skipped: it is inside, and cannot end the ray
            const Cell p = cell_of(a, o, e, k - 1);
            float P[8];
            long long unused;
            prev = corners_of(a, p, P, unused) ? 1 : 0;
            F_prev = trilinear(P, p.f[0], p.f[1], p.f[2]);
        }
        if (!corners_of(a, c, T, base)) { prev = 0; continue; }
        const float F = trilinear(T, c.f[0], c.f[1], c.f[2]);
        if (prev == 1) {
            if (!(F_prev < 0.0f) && F < 0.0f) { hit_k = k; F_hit = F; f[0] = c.f[0]; f[1] = c.f[1]; f[2] = c.f[2]; break; }
            if (F_prev < 0.0f && !(F < 0.0f)) break;
        }
        prev = 1;
        F_prev = F;
    }

    write_pixel(a, view, u, v, hit_k, F_prev, F_hit, T, f, a.colour != nullptr, [&](unsigned C[8]) {
        const long long plane = (long long)a.nx * a.ny;
#pragma unroll
        for (int j = 0; j < 8; ++j) C[j] = a.colour[base + (j & 1) + ((j >> 1) & 1) * (long long)a.nx + (j >> 2) * plane];
    });
}

}  // namespace

extern "C" int mr_tsdf_skip_grid_u8(const float* tsdf, const float* weight, int32_t nx, int32_t ny, int32_t nz, float min_weight,
                                    uint8_t* bricks, void* stream) {
    if (bad_volume(tsdf, weight, nullptr, nx, ny, nz, NO_ORIGIN, 1.0f, min_weight) || !bricks) return MR_ERR_BAD_ARGUMENT;
    SkipArgs a;
    a.tsdf = tsdf; a.weight = weight; a.nx = nx; a.ny = ny; a.nz = nz; a.min_weight = min_weight; a.bricks = bricks;
    const unsigned tiles = tile_grid(nx, ny, nz, a.tiles_x, a.tiles_y);
    if (!tiles) return MR_ERR_BAD_ARGUMENT;
    a.bricks_x = (nx + BRICK - 1) / BRICK; a.bricks_y = (ny + BRICK - 1) / BRICK;
    const long long count = (long long)a.bricks_x * a.bricks_y * ((nz + BRICK - 1) / BRICK);
    const hipError_t cleared = hipMemsetAsync(bricks, 0, (size_t)count, (hipStream_t)stream);
    if (cleared != hipSuccess) return (int)cleared;
    hipLaunchKernelGGL(tsdf_skip_grid_kernel, dim3(tiles), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int mr_tsdf_render_f32(const float* tsdf, const float* weight, const uint8_t* colour, int32_t nx, int32_t ny, int32_t nz,
                                  const float* origin, float voxel_size, float min_weight, const uint8_t* bricks,
                                  const mr_tsdf_ray_view* views, int32_t num_views, int32_t height, int32_t width, float t_min, float t_max,
                                  float step, void* stream) {
    if (bad_volume(tsdf, weight, colour, nx, ny, nz, origin, voxel_size, min_weight)) return MR_ERR_BAD_ARGUMENT;
    if (bad_ray_views(views, num_views, height, width, t_min, t_max, step)) return MR_ERR_BAD_ARGUMENT;
    const long long last = last_sample(t_min, t_max, step);
    if (last < 0) return MR_ERR_BAD_ARGUMENT;
    RenderArgs a;
    a.tsdf = tsdf; a.weight = weight; a.colour = reinterpret_cast<const unsigned*>(colour); a.bricks = bricks;
    a.nx = nx; a.ny = ny; a.nz = nz;
    a.bricks_x = (nx + BRICK - 1) / BRICK; a.bricks_y = (ny + BRICK - 1) / BRICK;
    const int dims[3] = {nx, ny, nz};
    const unsigned tiles = prepare_march(a, dims, origin, voxel_size, min_weight, t_min, step, last, height, width, views, num_views);
    if (!tiles) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(tsdf_render_kernel, dim3(tiles, 1, (unsigned)num_views), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
