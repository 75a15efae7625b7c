// What tsdf_fusion.hip (the dense volume), tsdf_sparse.hip (the block-sparse one) and, for its last section, tsdf_sparse_render.hip share,
// so that they run the same code and not copies of it (include/monorec_hip.h has the rules; compiled with -ffp-contract=off): the update
// of one voxel by one frame, FrameArgs and the host's frame_args and planes, live_frames, edge masks, record colours, the workgroup
// prefix sum, the checks of the surface entries, and the blocks' B, BV, pool_index and bad_sparse.  The frame loop round
// the voxel update stays in the two kernels: as a shared inline function it cost the dense one five VGPRs.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monorec_hip.h"

namespace {

__device__ __forceinline__ unsigned blend_byte(unsigned old, unsigned pix, float w_old, float w_new) {
    const float c = fminf(255.0f, floorf(((float)old * w_old + (float)pix) / w_new + 0.5f));
    return (unsigned)c;
}

// One frame into the voxel at (px, py, pz), mr_tsdf_integrate_f32's arithmetic operation for operation: t, wgt and (with has_colour) the
// packed r g b 0 in col are updated in place.  An update sets `bit` in touched, and one with diff / trunc < 1 (in the band) sets band;
// a skip leaves everything as it was.
__device__ __forceinline__ void tsdf_update_voxel(const mr_tsdf_view& f, float px, float py, float pz, int w, float wf, float hf, float trunc,
                                                  float max_depth, bool has_colour, float& t, float& wgt, unsigned& col, unsigned& touched,
                                                  unsigned bit, bool& band) {
    const float c0 = ((f.m[0] * px + f.m[1] * py) + f.m[2] * pz) + f.m[3];
    const float c1 = ((f.m[4] * px + f.m[5] * py) + f.m[6] * pz) + f.m[7];
    const float c2 = ((f.m[8] * px + f.m[9] * py) + f.m[10] * pz) + f.m[11];
    if (!(c2 > 0.0f)) return;
    const float uf = roundf(f.fx * (c0 / c2) + f.cx);
    const float vf = roundf(f.fy * (c1 / c2) + f.cy);
    if (!(uf >= 0.0f && uf < wf && vf >= 0.0f && vf < hf)) return;
    const long long pix = (long long)(int)vf * w + (int)uf;
    const float d = (float)f.depth_cm[pix] / 100.0f;
    if (d <= 0.0f || d > max_depth) return;
    const float diff = d - c2;
    if (diff <= -trunc) return;
    const float ratio = diff / trunc;
    const float dist = fminf(1.0f, ratio);
    const float w_old = wgt, w_new = w_old + 1.0f;
    t = (t * w_old + dist) / w_new;
    if (has_colour) {
        const uint8_t* s = f.colour + pix * 3;
        const unsigned r = blend_byte(col & 0xffu, s[0], w_old, w_new);
        const unsigned g = blend_byte((col >> 8) & 0xffu, s[1], w_old, w_new);
        const unsigned b = blend_byte((col >> 16) & 0xffu, s[2], w_old, w_new);
        col = r | (g << 8) | (b << 16);
    }
    wgt = w_new;
    touched |= bit;
    band = band || ratio < 1.0f;
}

// What both integrate kernels read of a launch's frames; the host's frame_args (below) fills it.
struct FrameArgs {
    float ox, oy, oz, voxel, trunc, max_depth;
    int num_frames, h, w;
    float cull_radius;                           // bounding sphere of a workgroup's voxels plus the margin for the fp32 evaluation
    mr_tsdf_view f[MR_TSDF_MAX_FRAMES];
    float plane[MR_TSDF_MAX_FRAMES][5][4];       // (n, d) in world space, |n| = 1 or 0 (0: never culls); inside is n . p + d >= 0
};

// Which frames can reach a workgroup's voxels: their bounding sphere (centre, cull_radius) against the five planes of each frame.
// Uniform over the workgroup.
__device__ __forceinline__ unsigned live_frames(const FrameArgs& a, float ccx, float ccy, float ccz) {
    unsigned live = 0;
    const int num_frames = a.num_frames;
    const float cull_radius = a.cull_radius;
    for (int fi = 0; fi < num_frames; ++fi) {
        bool out = false;
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            const float* q = a.plane[fi][p];
            const float dist = ((q[0] * ccx + q[1] * ccy) + q[2] * ccz) + q[3];
            out = out || (dist < -cull_radius);                      // NaN: not culled
        }
        if (!out) live |= 1u << fi;
    }
    return live;
}

// exclusive prefix of `mine` over a workgroup of 256 threads and its total: shuffles within the wave, wave totals through LDS
__device__ __forceinline__ int workgroup_prefix(int mine, int* wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int before = incl - mine;
    total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int v = wave_tot[w]; if (w < wave) before += v; total += v; }
    return before;
}

constexpr unsigned SEEN = 1u, NEG = 2u;          // the code byte of a staged voxel: bit 0 seen, bit 1 seen and negative

// red green blue of a record, between the packed colours cv and cn of the edge's two voxels
__device__ __forceinline__ void write_colour(float* o, unsigned cv, unsigned cn, float s) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float fv = (float)((cv >> (8 * c)) & 0xffu), fn = (float)((cn >> (8 * c)) & 0xffu);
        o[3 + c] = floorf(fv + s * (fn - fv) + 0.5f);
    }
}

// the active-edge mask, over the first EDGES of the seven, of the voxel at `at` of a block of codes with row stride sx and slice stride sxy
template <int EDGES>
__device__ __forceinline__ unsigned edge_mask(const uint8_t* code, int at, int sx, int sxy) {
    const unsigned c = code[at];
    if (!(c & SEEN)) return 0u;
    const int far[7] = {1, sx, sxy, 1 + sx, 1 + sxy, sx + sxy, 1 + sx + sxy};
    unsigned mask = 0;
#pragma unroll
    for (int e = 0; e < EDGES; ++e) {
        const unsigned n = code[at + far[e]];
        if ((n & SEEN) && ((n ^ c) & NEG)) mask |= 1u << e;
    }
    return mask;
}

// pixels by which a view's planes are widened beyond the half pixel of roundf, along u (extent w) or v (extent h)
inline double view_slack(double centre, double extent, double focal) { return 1.0 + 1e-6 * (fabs(centre) + extent + focal); }

// The near and four side planes of one view in world space, in double.  A voxel can pass the kernel's cam_2 > 0 and image-bounds
// tests only if its camera-space point c = A p + t has c_2 > 0 and -0.5 <= fx c_0 / c_2 + cx < w - 0.5 (likewise v): the intersection
// of five half spaces n_c . c >= 0 through the camera centre.  They are widened by `slack` pixels beyond the half pixel of roundf, and
// the kernel culls a tile only when its sphere is `margin` further out than that (see mr_tsdf_integrate_f32): more than the fp32
// evaluation of c, of u and v and of the plane test itself can move a point.  Anything doubtful (non-positive focal lengths, A far
// from a rotation, non-finite numbers) leaves the plane at zero, which never culls.
inline void view_planes(const mr_tsdf_view& f, int h, int w, float out[5][4]) {
    for (int p = 0; p < 5; ++p) for (int k = 0; k < 4; ++k) out[p][k] = 0.0f;
    if (!(f.fx > 0.0f) || !(f.fy > 0.0f)) return;
    double rows[3];
    for (int r = 0; r < 3; ++r) {
        rows[r] = sqrt((double)f.m[4 * r] * f.m[4 * r] + (double)f.m[4 * r + 1] * f.m[4 * r + 1] + (double)f.m[4 * r + 2] * f.m[4 * r + 2]);
        if (!(rows[r] > 0.5 && rows[r] < 2.0)) return;
    }
    const double slack_u = view_slack(f.cx, w, f.fx), slack_v = view_slack(f.cy, h, f.fy);
    const double nc[5][3] = {
        {0.0, 0.0, 1.0},                                                          // c_2 >= 0
        {(double)f.fx, 0.0, (double)f.cx + 0.5 + slack_u},                        // u >= -0.5 - slack
        {-(double)f.fx, 0.0, (double)w - 0.5 + slack_u - (double)f.cx},           // u <= w - 0.5 + slack
        {0.0, (double)f.fy, (double)f.cy + 0.5 + slack_v},
        {0.0, -(double)f.fy, (double)h - 0.5 + slack_v - (double)f.cy},
    };
    for (int p = 0; p < 5; ++p) {
        double nw[3], d = 0.0;
        for (int k = 0; k < 3; ++k) nw[k] = nc[p][0] * f.m[k] + nc[p][1] * f.m[4 + k] + nc[p][2] * f.m[8 + k];
        for (int r = 0; r < 3; ++r) d += nc[p][r] * f.m[4 * r + 3];
        const double len = sqrt(nw[0] * nw[0] + nw[1] * nw[1] + nw[2] * nw[2]);
        const double lc = sqrt(nc[p][0] * nc[p][0] + nc[p][1] * nc[p][1] + nc[p][2] * nc[p][2]);
        if (!(len > 0.25 * lc) || !isfinite(len) || !isfinite(d)) continue;      // (A within [0.5, 2] per row, yet nearly singular along n_c)
        out[p][0] = (float)(nw[0] / len); out[p][1] = (float)(nw[1] / len); out[p][2] = (float)(nw[2] / len); out[p][3] = (float)(d / len);
    }
}

// The largest number the fp32 evaluation of a launch handles, for a volume whose voxels reach `corner` metres from the world's origin:
// the far corner of the volume plus a camera's translation.  The workgroup's centre, a voxel's camera-space point and the plane test are
// each a handful of roundings of numbers no larger than it, so 64 ulp of it (4e-6) is several times their sum; a thousandth of a voxel
// covers volumes at the origin: the callers' margin is 1e-3 * voxel + FP32_SLACK * reach.
constexpr double FP32_SLACK = 64.0 * 5.97e-8;
inline double frames_reach(double corner, const mr_tsdf_view* frames, int num_frames) {
    double reach = 0.0;
    for (int i = 0; i < num_frames; ++i) {
        const float* m = frames[i].m;
        reach = fmax(reach, 2.0 * corner + sqrt((double)m[3] * m[3] + (double)m[7] * m[7] + (double)m[11] * m[11]));
    }
    return reach;
}

// The frame half of an integrate launch, for both entries: the checks of the frames, the image and the limits, then `a` - the frames,
// their planes (those of the unused frames never cull) and the cull radius round a workgroup's sphere of `radius` metres.  The volume
// has voxels[k] voxels along axis k and its workgroups reach `pad` further; origin and voxel_size are checked by the caller.  Returns the
// margin 1e-3 * voxel + FP32_SLACK * reach that widens the cull radius (not negative; it may be infinite or NaN), or -1: a bad argument.
inline double frame_args(FrameArgs& a, const float* origin, float voxel_size, float trunc, float max_depth_m,
                       const mr_tsdf_view* frames, int num_frames, int height, int width, bool has_colour, const double voxels[3], int pad,
                       double radius) {
    if (!frames || num_frames < 1 || num_frames > MR_TSDF_MAX_FRAMES || height < 1 || width < 1) return -1.0;
    if (!(trunc > 0.0f) || max_depth_m != max_depth_m) return -1.0;
    if ((long long)height * width * 3 >= (1ll << 40)) return -1.0;
    for (int i = 0; i < num_frames; ++i)
        if (!frames[i].depth_cm || (has_colour && !frames[i].colour)) return -1.0;
    a.ox = origin[0]; a.oy = origin[1]; a.oz = origin[2];
    a.voxel = voxel_size; a.trunc = trunc; a.max_depth = max_depth_m;
    a.num_frames = num_frames; a.h = height; a.w = width;
    const double v = (double)voxel_size;
    double corner = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double far_k = fmax(fabs((double)origin[k]), fabs((double)origin[k] + (voxels[k] + pad) * v));
        corner += far_k * far_k;
    }
    corner = sqrt(corner);
    for (int i = 0; i < MR_TSDF_MAX_FRAMES; ++i) {
        a.f[i] = frames[i < num_frames ? i : 0];
        if (i < num_frames) view_planes(frames[i], height, width, a.plane[i]);
        else for (int p = 0; p < 5; ++p) for (int k = 0; k < 4; ++k) a.plane[i][p][k] = 0.0f;
    }
    const double margin = 1e-3 * v + FP32_SLACK * frames_reach(corner, frames, num_frames);
    const double cull = radius + margin;
    a.cull_radius = isfinite(cull) ? nextafterf((float)cull, INFINITY) : INFINITY;       // infinite: `dist < -inf` never holds
    return margin;
}

// ---- what the surface entries of both volumes check alike
constexpr long long MAX_VOXELS = 1ll << 40;      // of a volume, a pool or a gathered box: idx * 4 bytes and the block counts stay far from overflow
constexpr float NO_ORIGIN[3] = {0.0f, 0.0f, 0.0f};               // of an entry that takes no positions (with a voxel of 1)

// an output of 4-byte elements that may be null (count only) and the cursor beside it.  True: a bad argument.
inline bool bad_output(const void* out, long long capacity, const int64_t* cursor) {
    return !cursor || ((uintptr_t)cursor & 7) || ((uintptr_t)out & 3) || (out && capacity < 0);
}

// ---- the block-sparse volume: a table of one slot (or -1) per block of B^3 voxels, and a pool of BV voxels per slot
constexpr int B = MR_TSDF_BLOCK, BV = B * B * B;
static_assert(B == 8, "128 threads of four voxels along x; rows of 32 bytes; >> 3 and & 7 below");

// the pool index of voxel (x, y, z) of slot s; the coordinates may be the volume's or, up to B + 1, those of a block with its + halo
__device__ __forceinline__ long long pool_index(int s, int x, int y, int z) {
    return (long long)s * BV + (((z & 7) * B + (y & 7)) * B + (x & 7));
}

// The checks the sparse entries share: the table and the pool.  True: a bad argument.  `blocks` returns nbx * nby * nbz.
inline bool bad_sparse(const void* table, int nbx, int nby, int nbz, const void* tsdf, const void* weight, const void* colour, long long& blocks) {
    if (!table || !tsdf || !weight || nbx < 1 || nby < 1 || nbz < 1) return true;
    if (((uintptr_t)table & 3) || (((uintptr_t)tsdf | (uintptr_t)weight | (uintptr_t)colour) & 15)) return true;
    const long long xy = (long long)nbx * nby;                               // < 2^62
    if (xy >= (1ll << 31)) return true;
    blocks = xy * nbz;                                                       // < 2^62
    return blocks >= (1ll << 31);
}

}  // namespace
