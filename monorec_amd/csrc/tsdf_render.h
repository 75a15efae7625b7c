// What the two ray-cast kernels share - tsdf_render_kernel of tsdf_fusion.hip (the dense volume) and tsdf_sparse_render_kernel of
// tsdf_sparse_render.hip (the block-sparse one) -, so that both march the same samples with the same arithmetic and not two copies of
// it: a pixel's ray, the cell of a sample, the clip to the volume's box, the trilinear interpolant, what a pixel writes, and the host's
// checks and preparation of a launch.  The kernels differ in how they fetch the eight corners of a cell and in how they pass empty space.
// include/monorec_hip.h has the rules; both sources are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monorec_hip.h"

namespace {

constexpr int MAX_SAMPLES = 1 << 20;

struct RayView {
    float r[9];                                  // camera -> world rotation, row-major
    float o[3];                                  // the camera centre in voxel units: (c - origin) * inv
    float fx, fy, cx, cy;
    float* depth;
    float* normal;
    uint8_t* colour;
};

// The launch arguments of both kernels have these members (`Args` below):
//   float lim[3]                 the largest float <= n_a - 2: the last cell base along each axis
//   float inv, min_weight, t_min, step
//   int last                     index of the last sample with t_k <= t_max
//   int h, w, tiles_x
//   RayView v[MR_TSDF_MAX_FRAMES]

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }

__device__ __forceinline__ float trilinear(const float c[8], float fx, float fy, float fz) {   // c[x + 2 y + 4 z]
    const float y0 = lerp(lerp(c[0], c[1], fx), lerp(c[2], c[3], fx), fy);
    const float y1 = lerp(lerp(c[4], c[5], fx), lerp(c[6], c[7], fx), fy);
    return lerp(y0, y1, fz);
}

struct Cell {
    float f[3];
    int i[3];
    bool inside;                                 // all 8 corners are voxels of the volume
};

template <class Args>
__device__ __forceinline__ Cell cell_of(const Args& a, const float o[3], const float e[3], int k) {
    const float t = a.t_min + (float)k * a.step;
    Cell c;
    c.inside = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float g = o[q] + t * e[q];
        const float fl = floorf(g);
        c.f[q] = g - fl;
        const bool in = fl >= 0.0f && fl <= a.lim[q];                      // NaN: outside
        c.inside = c.inside && in;
        c.i[q] = in ? (int)fl : 0;
    }
    return c;
}

// the ray of pixel (u, v) in voxel units: g = o + t * e at camera-z depth t
template <class Args>
__device__ __forceinline__ void ray_of_pixel(const Args& a, const RayView& view, int u, int v, float o[3], float e[3]) {
    const float rx = ((float)u - view.cx) / view.fx, ry = ((float)v - view.cy) / view.fy;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        o[q] = view.o[q];
        e[q] = ((view.r[3 * q] * rx + view.r[3 * q + 1] * ry) + view.r[3 * q + 2]) * a.inv;
    }
}

// Clip to the box 0 <= g_a <= n_a in t, then in k.  Only an optimisation, so it only has to be conservative: no sample outside
// [k_lo, k_hi] may be valid.  The crossing times t_a = (bound - o_a) / e_a are a few ulp of max(|t_a|) off, and so is the t at which
// the fp32 g_a = o_a + t_k * e_a crosses the bound (|o_a| / |e_a| is one of the two |t_a|); the range is widened by 1e-5 of the
// larger |t_a| (more than 80 ulp) and by one step, and the k range by one more sample for the roundings of (t - t_min) / step and of
// (float)k * step (k < 2^20: 0.07 of a sample each).  fmaxf / fminf drop a NaN, which leaves the range as it was.
template <class Args>
__device__ __forceinline__ void clip_to_box(const Args& a, const float o[3], const float e[3], int& k_lo, int& k_hi) {
    float t_lo = a.t_min, t_hi = a.t_min + (float)a.last * a.step;
    bool empty = false;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float top = a.lim[q] + 2.0f;                                  // n_a (or just below): beyond the last valid g_a
        if (e[q] == 0.0f) {
            empty = empty || !(o[q] >= 0.0f && o[q] <= top);                // g_a = o_a all along the ray
            continue;
        }
        const float ta = (0.0f - o[q]) / e[q], tb = (top - o[q]) / e[q];
        const float slack = 1e-5f * fmaxf(fabsf(ta), fabsf(tb)) + a.step;
        t_lo = fmaxf(t_lo, fminf(ta, tb) - slack);
        t_hi = fminf(t_hi, fmaxf(ta, tb) + slack);
    }
    k_lo = (int)fminf(fmaxf(floorf((t_lo - a.t_min) / a.step) - 1.0f, 0.0f), (float)a.last + 1.0f);
    k_hi = (int)fminf(fmaxf(ceilf((t_hi - a.t_min) / a.step) + 1.0f, -1.0f), (float)a.last);
    if (empty) k_hi = -1;
}

// What pixel (u, v) writes: a hit at sample hit_k (>= 0) with F_hit behind F_prev, in the cell of corner tsdf T at the fractions f, or
// nothing.  colour_of(C) fetches the packed r g b 0 of the hit cell's eight corners; it is called only with has_colour.
template <class Args, class ColourOf>
__device__ __forceinline__ void write_pixel(const Args& a, const RayView& view, int u, int v, int hit_k, float F_prev, float F_hit,
                                            const float T[8], const float f[3], bool has_colour, ColourOf colour_of) {
    const long long pix = (long long)v * a.w + u;
    float depth = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
    unsigned rgb[3] = {0u, 0u, 0u};
    if (hit_k >= 0) {
        const float s = F_prev / (F_prev - F_hit);
        depth = (a.t_min + (float)(hit_k - 1) * a.step) + s * a.step;
        if (view.normal) {
            const float gx = lerp(lerp(T[1] - T[0], T[3] - T[2], f[1]), lerp(T[5] - T[4], T[7] - T[6], f[1]), f[2]);
            const float gy = lerp(lerp(T[2] - T[0], T[3] - T[1], f[0]), lerp(T[6] - T[4], T[7] - T[5], f[0]), f[2]);
            const float gz = lerp(lerp(T[4] - T[0], T[5] - T[1], f[0]), lerp(T[6] - T[2], T[7] - T[3], f[0]), f[1]);
            const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
            if (len > 0.0f) { n[0] = gx / len; n[1] = gy / len; n[2] = gz / len; }
        }
        if (view.colour && has_colour) {
            unsigned C[8];
            colour_of(C);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float B[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) B[j] = (float)((C[j] >> (8 * ch)) & 0xffu);
                rgb[ch] = (unsigned)fminf(255.0f, floorf(trilinear(B, f[0], f[1], f[2]) + 0.5f));
            }
        }
    }
    view.depth[pix] = depth;
    if (view.normal) { float* o3 = view.normal + pix * 3; o3[0] = n[0]; o3[1] = n[1]; o3[2] = n[2]; }
    if (view.colour) { uint8_t* c3 = view.colour + pix * 3; c3[0] = (uint8_t)rgb[0]; c3[1] = (uint8_t)rgb[1]; c3[2] = (uint8_t)rgb[2]; }
}

// ---- the host's half of a launch

inline float t_of(float t_min, float step, long long k) { return t_min + (float)k * step; }

// The checks of the views, the image size and the range that both entries make.  True: a bad argument.
inline bool bad_ray_views(const mr_tsdf_ray_view* views, int num_views, int height, int width, float t_min, float t_max, float step) {
    if (!views || num_views < 1 || num_views > MR_TSDF_MAX_FRAMES || height < 1 || width < 1) return true;
    if (!(step > 0.0f) || !(t_min >= 0.0f) || !(t_max >= t_min) || !isfinite(t_min) || !isfinite(t_max)) return true;
    for (int i = 0; i < num_views; ++i) {
        const mr_tsdf_ray_view& s = views[i];
        if (!s.depth || (((uintptr_t)s.depth | (uintptr_t)s.normal) & 3)) return true;
        if (s.fx == 0.0f || s.fy == 0.0f || s.fx != s.fx || s.fy != s.fy) return true;
    }
    return false;
}

// the last k with t_k <= t_max, t_k as the kernel rounds it (non-decreasing in k): an estimate in double, then stepped into place.
// -1: more than MAX_SAMPLES samples.
inline long long last_sample(float t_min, float t_max, float step) {
    const double estimate = floor(((double)t_max - (double)t_min) / (double)step);
    if (!(estimate < (double)MAX_SAMPLES + 2.0)) return -1;
    long long last = (long long)estimate;
    while (last > 0 && t_of(t_min, step, last) > t_max) --last;
    while (last + 1 <= MAX_SAMPLES && t_of(t_min, step, last + 1) <= t_max) ++last;
    return last + 1 > MAX_SAMPLES ? -1 : last;
}

// The members the kernels share, for a volume of dims voxels.  Returns the pixel tiles of one view, or 0 when they do not fit a grid.
template <class Args>
inline unsigned prepare_march(Args& a, const int dims[3], const float* origin, float voxel_size, float min_weight, float t_min, float step,
                              long long last, int height, int width, const mr_tsdf_ray_view* views, int num_views) {
    for (int q = 0; q < 3; ++q) {
        float lim = (float)(dims[q] - 2);                                   // -1 for a single layer of voxels: no cell, no valid sample
        if ((double)lim > (double)(dims[q] - 2)) lim = nextafterf(lim, 0.0f);
        a.lim[q] = lim;
    }
    a.inv = 1.0f / voxel_size; a.min_weight = min_weight; a.t_min = t_min; a.step = step; a.last = (int)last;
    a.h = height; a.w = width; a.tiles_x = (width + 15) / 16;
    const long long tiles = (long long)a.tiles_x * ((height + 15) / 16);
    if (tiles > 0x7fffffffLL) return 0;
    for (int i = 0; i < MR_TSDF_MAX_FRAMES; ++i) {
        const mr_tsdf_ray_view& s = views[i < num_views ? i : 0];
        RayView& d = a.v[i];
        for (int q = 0; q < 3; ++q) {
            for (int j = 0; j < 3; ++j) d.r[3 * q + j] = s.m[4 * q + j];
            d.o[q] = (s.m[4 * q + 3] - origin[q]) * a.inv;
        }
        d.fx = s.fx; d.fy = s.fy; d.cx = s.cx; d.cy = s.cy;
        d.depth = s.depth; d.normal = s.normal; d.colour = s.colour;
    }
    return (unsigned)tiles;
}

}  // namespace
