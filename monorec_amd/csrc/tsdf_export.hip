// TSDF-fusion export (utils/util.py:78-92, save_frame_for_tsdf): everything the reference does to one keyframe before it hands two
// arrays to Pillow, for a batch of keyframes in one launch.
//
//   depth  = (1 / inv_depth * 100).to(int16); depth[depth < 0] = 0; depth[depth < min * 100] = 0; depth[depth > max * 100] = 0     (:83-88)
//   colour = ((keyframe + .5) * 255).to(uint8).permute(1, 2, 0)                                                                    (:82)
//   both cropped to [y0:y1, x0:x1] first                                                                                           (:79-81)
// optionally preceded by the static-mask vote and `depth *= mask` of create_pointcloud.py:90-92 (same convention as
// pointcloud_append_kernel in pointcloud.hip).
//
// Arithmetic is the x86 torch CPU's, operation by operation (compiled with -ffp-contract=off: the add and the multiply of the colour
// stay separate; the division is the correctly rounded one, never v_rcp alone).  The float -> int16 conversion of torch on x86 is a
// truncating 32-bit conversion whose low half is kept: 327.68 m and beyond wraps negative and is zeroed by `depth < 0`; values the
// 32-bit conversion cannot hold (|v| >= 2^31, NaN) come out as INT_MIN there, low half 0.  Both are spelled out below instead of
// being left to what an out-of-range conversion happens to do on the device.
//
// The outputs are walked as a flat run of cropped pixels, four per thread: 8 bytes of depth and 12 bytes of colour per thread, both at
// offsets that are multiples of their size whatever the crop width, so every store but the last thread's tail is a packed vector
// store.  Where image width, crop origin and crop width are all multiples of four the four pixels are one 16-byte load per plane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/monorec_hip.h"

namespace {

struct TsdfArgs {
    const float* inv_depth;                    // B x H x W
    const float* image;                        // B x 3 x H x W
    const float* masks[MR_MAX_VOTE_MASKS];     // B x H x W each
    int num_masks;
    float vote_above;                          // keep where sum(masks) > vote_above
    int y0, x0, ch, cw;                        // crop origin and size
    int H, W;
    float min_cm, max_cm;                      // -inf / +inf: no threshold
    long long pixels;                          // B * ch * cw
    int vec;                                   // every group of four is one aligned 16-byte run of one source row
    int16_t* depth;                            // B x ch x cw
    uint8_t* colour;                           // B x ch x cw x 3
};

__device__ __forceinline__ unsigned depth_cm(float d, float min_cm, float max_cm) {
    const float v = (1.0f / d) * 100.0f;                                   // :83, two roundings
    int i = 0;
    if (v > -2147483648.0f && v < 2147483648.0f) i = (int)v;               // else (NaN too): INT_MIN on x86, low half 0
    int s = (int)(short)(i & 0xffff);                                      // .to(torch.int16): low half, signed
    if (s < 0) s = 0;                                                      // :84
    const float f = (float)s;                                              // int16 against a Python float: compared in fp32
    if (f < min_cm) s = 0;                                                 // :85-86
    if (f > max_cm) s = 0;                                                 // :87-88
    return (unsigned)s;
}

__device__ __forceinline__ unsigned colour_byte(float k) {
    const float c = (k + 0.5f) * 255.0f;                                   // :82, add and multiply stay separate
    int i = 0;
    if (c > -2147483648.0f && c < 2147483648.0f) i = (int)c;
    return (unsigned)i & 0xffu;                                            // .to(torch.uint8) of a value in [0, 255]: the truncation
}

__global__ __launch_bounds__(256) void tsdf_frame_kernel(const TsdfArgs a) {
    const long long group = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long q0 = group * 4;
    if (q0 >= a.pixels) return;
    const long long plane = (long long)a.H * a.W;
    const long long per_image = (long long)a.ch * a.cw;
    float d[4], k[3][4];
    int n = 4;
    if (a.vec) {                                                           // (then pixels % 4 == 0 as well)
        const long long b = q0 / per_image, r = q0 - b * per_image;
        const int y = (int)(r / a.cw), x = (int)(r - (long long)y * a.cw);
        const long long src = b * plane + (long long)(a.y0 + y) * a.W + (a.x0 + x);
        const float4 dv = *reinterpret_cast<const float4*>(a.inv_depth + src);
        d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
        if (a.num_masks > 0) {                                             // torch.sum(torch.stack(mask_buffer), dim=0) > n - min_hits
            float4 s = *reinterpret_cast<const float4*>(a.masks[0] + src);
            for (int m = 1; m < a.num_masks; ++m) {
                const float4 t = *reinterpret_cast<const float4*>(a.masks[m] + src);
                s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
            }
            d[0] *= (s.x > a.vote_above) ? 1.f : 0.f;                      // depth *= mask
            d[1] *= (s.y > a.vote_above) ? 1.f : 0.f;
            d[2] *= (s.z > a.vote_above) ? 1.f : 0.f;
            d[3] *= (s.w > a.vote_above) ? 1.f : 0.f;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float4 kv = *reinterpret_cast<const float4*>(a.image + 2 * b * plane + c * plane + src);
            k[c][0] = kv.x; k[c][1] = kv.y; k[c][2] = kv.z; k[c][3] = kv.w;
        }
    } else {
        n = (int)((a.pixels - q0) < 4 ? (a.pixels - q0) : 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[j] = 0.f; k[0][j] = k[1][j] = k[2][j] = 0.f;
            if (j >= n) continue;
            const long long q = q0 + j;
            const long long b = q / per_image, r = q - b * per_image;
            const int y = (int)(r / a.cw), x = (int)(r - (long long)y * a.cw);
            const long long src = b * plane + (long long)(a.y0 + y) * a.W + (a.x0 + x);
            float dj = a.inv_depth[src];
            if (a.num_masks > 0) {
                float s = a.masks[0][src];
                for (int m = 1; m < a.num_masks; ++m) s += a.masks[m][src];
                dj *= (s > a.vote_above) ? 1.f : 0.f;
            }
            d[j] = dj;
#pragma unroll
            for (int c = 0; c < 3; ++c) k[c][j] = a.image[2 * b * plane + c * plane + src];
        }
    }
    unsigned z[4], px[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        z[j] = depth_cm(d[j], a.min_cm, a.max_cm);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[j][c] = colour_byte(k[c][j]);
    }
    if (n == 4) {
        // 4 x int16 -> 2 dwords; 4 x (r, g, b) -> 3 dwords: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 (little endian)
        *reinterpret_cast<uint2*>(a.depth + q0) = make_uint2(z[0] | (z[1] << 16), z[2] | (z[3] << 16));
        unsigned* o = reinterpret_cast<unsigned*>(a.colour + q0 * 3);
        o[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
        o[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
        o[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
    } else {                                                               // the last one to three pixels of the run
        for (int j = 0; j < n; ++j) {
            a.depth[q0 + j] = (int16_t)z[j];
            for (int c = 0; c < 3; ++c) a.colour[(q0 + j) * 3 + c] = (uint8_t)px[j][c];
        }
    }
}

}  // namespace

extern "C" int mr_tsdf_frame_f32(const float* inv_depth, const float* keyframe, const float* const* static_masks, int32_t num_masks,
                                 float vote_above, const int32_t* crop, float min_cm, float max_cm, int32_t batch, int32_t height,
                                 int32_t width, int16_t* depth, uint8_t* colour, void* stream) {
    if (!inv_depth || !keyframe || !depth || !colour || batch < 1 || height < 1 || width < 1) return MR_ERR_BAD_ARGUMENT;
    if (num_masks < 0 || num_masks > MR_MAX_VOTE_MASKS || (num_masks > 0 && !static_masks)) return MR_ERR_BAD_ARGUMENT;
    if (min_cm != min_cm || max_cm != max_cm) return MR_ERR_BAD_ARGUMENT;
    TsdfArgs a;
    a.inv_depth = inv_depth; a.image = keyframe;
    for (int k = 0; k < MR_MAX_VOTE_MASKS; ++k) a.masks[k] = k < num_masks ? static_masks[k] : nullptr;
    for (int k = 0; k < num_masks; ++k) if (!a.masks[k]) return MR_ERR_BAD_ARGUMENT;
    a.num_masks = num_masks; a.vote_above = vote_above;
    int y0 = 0, y1 = height, x0 = 0, x1 = width;
    if (crop) { y0 = crop[0]; y1 = crop[1]; x0 = crop[2]; x1 = crop[3]; }
    if (y0 < 0 || x0 < 0 || y1 > height || x1 > width || y1 <= y0 || x1 <= x0) return MR_ERR_BAD_ARGUMENT;
    a.y0 = y0; a.x0 = x0; a.ch = y1 - y0; a.cw = x1 - x0;
    a.H = height; a.W = width;
    a.min_cm = min_cm; a.max_cm = max_cm;
    a.pixels = (long long)batch * a.ch * a.cw;
    bool aligned = ((uintptr_t)inv_depth % 16 == 0) && ((uintptr_t)keyframe % 16 == 0);
    for (int k = 0; k < num_masks; ++k) aligned = aligned && ((uintptr_t)a.masks[k] % 16 == 0);
    a.vec = (aligned && width % 4 == 0 && x0 % 4 == 0 && a.cw % 4 == 0) ? 1 : 0;
    if (((uintptr_t)depth % 8) != 0 || ((uintptr_t)colour % 4) != 0) return MR_ERR_BAD_ARGUMENT;       // the packed stores
    a.depth = depth; a.colour = colour;
    const long long groups = (a.pixels + 3) / 4;
    const long long blocks = (groups + 255) / 256;
    if (blocks > 0x7fffffffLL) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(tsdf_frame_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
