// Cross-view consistency filter of a keyframe's inverse depth (include/monorec_hip.h, mr_depth_consistency_f32): every valid pixel of the
// reference keyframe is lifted to 3-D, projected into up to MR_CONSISTENCY_MAX_VIEWS neighbouring keyframes, compared with the depth the
// neighbour predicted there (nearest pixel) and brought back; a neighbour that agrees in depth and lands within max_reproj_px of the
// start is a hit.  Pixels with fewer than min_views hits are zeroed.  No reference lines stand behind it: the header is the definition.
//
// All fp32, every operation rounded on its own (compiled with -ffp-contract=off; the divisions are the correctly rounded ones), in the
// order of the header; tests/depth_consistency_ref.py restates it in numpy bit for bit.
//
// One pixel per thread.  A workgroup of 256 threads covers a tile of 32 x 8 pixels, a wave 32 x 2: the reference keyframe is read, and
// `out` / `hits` are written, as whole 128-byte (32-byte) row pieces, and since neighbouring pixels project onto neighbouring pixels the
// 64 gathers of a wave into one neighbour fall into a few cache lines of two or three rows - they are left to L2.  The neighbour loop is
// uniform across the wave (the views sit in the kernel arguments and are read with scalar loads); a lane that has dropped out of a
// neighbour carries a false predicate to the end of that iteration, and out-of-image lanes of ragged tiles run along as invalid pixels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monorec_hip.h"

namespace {

constexpr int TILE_W = 32, TILE_H = 8;

struct ConsistencyArgs {
    const float* inv_depth;                        // H x W
    float fx, fy, cx, cy;
    mr_consistency_view views[MR_CONSISTENCY_MAX_VIEWS];
    int num_views;
    float rel_tol, max_reproj_sq;                  // max_reproj_sq: max_reproj_px * max_reproj_px in fp32
    int check_reproj;                              // 0: max_reproj_px is +INFINITY
    int min_views, average;
    int H, W, tiles_x;                             // tiles_x: tiles per row of tiles; the grid is one-dimensional (grid.y holds 65535 at most)
    float* out;                                    // H x W or NULL
    uint8_t* hits;                                 // H x W or NULL
};

// valid iff inv > 0 and 1 / inv is finite and > 0 (NaN, 0, negatives, +inf and reciprocals that overflow are not)
__device__ __forceinline__ bool valid_depth(float inv, float& d) {
    d = 1.0f / inv;
    return inv > 0.0f && d > 0.0f && d < INFINITY;
}

__device__ __forceinline__ float row(const float* m, int r, float x, float y, float z) {
    return ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

__global__ __launch_bounds__(256) void depth_consistency_kernel(const ConsistencyArgs a) {
    const unsigned tile_y = blockIdx.x / (unsigned)a.tiles_x, tile_x = blockIdx.x - tile_y * (unsigned)a.tiles_x;
    const unsigned x = tile_x * TILE_W + (threadIdx.x & (TILE_W - 1));         // unsigned: below W + 32 and H + 8, which an int may not hold
    const unsigned y = tile_y * TILE_H + (threadIdx.x / TILE_W);
    const bool inside = x < (unsigned)a.W && y < (unsigned)a.H;
    const int idx = inside ? (int)(y * (unsigned)a.W + x) : 0;                 // H * W < 2^31
    const float inv = a.inv_depth[idx];
    float d;
    const bool valid = valid_depth(inv, d) && inside;
    const float xf = (float)x, yf = (float)y;
    const float X = ((xf - a.cx) / a.fx) * d, Y = ((yf - a.cy) / a.fy) * d, Z = d;
    float sum = d;
    int n = 0;
    for (int j = 0; j < a.num_views; ++j) {
        const mr_consistency_view& vw = a.views[j];
        const float q0 = row(vw.m, 0, X, Y, Z), q1 = row(vw.m, 1, X, Y, Z), q2 = row(vw.m, 2, X, Y, Z);
        bool ok = valid && q2 > 0.0f;                                          // 1. behind
        const float u = roundf(vw.fx * (q0 / q2) + vw.cx), v = roundf(vw.fy * (q1 / q2) + vw.cy);
        ok = ok && u >= 0.0f && u < (float)a.W && v >= 0.0f && v < (float)a.H; // 2. outside (NaN fails)
        const int ui = ok ? (int)u : 0, vi = ok ? (int)v : 0;
        const float invn = vw.inv_depth[vi * a.W + ui];                        // nearest neighbour; lanes that are out read pixel 0
        float dn;
        ok = valid_depth(invn, dn) && ok;                                      // 3. no depth
        ok = ok && fabsf(dn - q2) <= a.rel_tol * q2;                           // 4. depth
        const float Xn = ((u - vw.cx) / vw.fx) * dn, Yn = ((v - vw.cy) / vw.fy) * dn;
        const float p0 = row(vw.back, 0, Xn, Yn, dn), p1 = row(vw.back, 1, Xn, Yn, dn), p2 = row(vw.back, 2, Xn, Yn, dn);
        ok = ok && p2 > 0.0f;                                                  // 5. reprojection
        if (a.check_reproj) {
            const float ex = (a.fx * (p0 / p2) + a.cx) - xf, ey = (a.fy * (p1 / p2) + a.cy) - yf;
            ok = ok && (ex * ex + ey * ey <= a.max_reproj_sq);
        }
        if (ok) {                                                              // 6. hit
            n += 1;
            sum = sum + p2;
        }
    }
    if (!inside) return;
    if (a.hits) a.hits[idx] = (uint8_t)n;
    if (a.out) {
        float o = 0.0f;
        if (valid && n >= a.min_views) o = a.average ? 1.0f / (sum / (float)(1 + n)) : inv;
        a.out[idx] = o;
    }
}

}  // namespace

extern "C" int mr_depth_consistency_f32(const float* inv_depth, float fx, float fy, float cx, float cy, const mr_consistency_view* views,
                                        int32_t num_views, float rel_tol, float max_reproj_px, int32_t min_views, int32_t average,
                                        int32_t height, int32_t width, float* out, uint8_t* hits, void* stream) {
    if (!inv_depth || !views || (!out && !hits)) return MR_ERR_BAD_ARGUMENT;
    if (num_views < 1 || num_views > MR_CONSISTENCY_MAX_VIEWS || height < 1 || width < 1 || min_views < 0) return MR_ERR_BAD_ARGUMENT;
    if ((long long)height * width >= (1LL << 31)) return MR_ERR_BAD_ARGUMENT;
    if (!(rel_tol >= 0.0f) || !(max_reproj_px >= 0.0f)) return MR_ERR_BAD_ARGUMENT;                  // NaN or negative
    ConsistencyArgs a;
    a.inv_depth = inv_depth; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
    for (int j = 0; j < MR_CONSISTENCY_MAX_VIEWS; ++j) {
        a.views[j] = views[j < num_views ? j : 0];
        if (!a.views[j].inv_depth) return MR_ERR_BAD_ARGUMENT;
    }
    a.num_views = num_views;
    a.rel_tol = rel_tol;
    a.check_reproj = max_reproj_px < INFINITY ? 1 : 0;
    a.max_reproj_sq = max_reproj_px * max_reproj_px;
    a.min_views = min_views; a.average = average ? 1 : 0;
    a.H = height; a.W = width;
    a.out = out; a.hits = hits;
    const long long bx = ((long long)width + TILE_W - 1) / TILE_W, by = ((long long)height + TILE_H - 1) / TILE_H;
    a.tiles_x = (int)bx;
    if (bx * by > 0x7fffffffLL) return MR_ERR_BAD_ARGUMENT;                    // (cannot happen below 2^31 pixels: bx * by <= H * W)
    hipLaunchKernelGGL(depth_consistency_kernel, dim3((unsigned)(bx * by)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
