// Host side shared by the direct kernels (conv_mfma.hip, conv_b8.hip) and, through wino_host.h, the reduced-multiply ones: the "LDS ceiling
// once per device, then launch" helper, the bf16 rounding of the packers, and the walk and size of the direct kernels' packed weight streams.
// Argument checks stay with the entry points: they differ between them, and so does the order they are made in.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <atomic>

#include "conv_layout.h"

// Raises the dynamic-LDS ceiling of `Kernel` to `ceiling_bytes` once per device (the attribute lives in the device's code object: a process
// that drives several GPUs - nn.DataParallel replicas - must set it on each; the mask is per instantiation, i.e. per kernel), then launches it.
template <auto Kernel, class KArgs>
int launch_lds_ceiling(int ceiling_bytes, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const KArgs& k) {
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (int)hipGetLastError();
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_acquire) & bit)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, ceiling_bytes);
        if (e != hipSuccess) return (int)e;
        attr_set.fetch_or(bit, std::memory_order_release);
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, k);
    return (int)hipGetLastError();
}

// fp32 -> bf16, round to nearest even
static inline uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x007fffffu)) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// ---- packed weight streams of the direct kernels ------------------------------------------------------------------------------------
// Every stream is the same walk, [cout group of mb 16-channel blocks][source][chunk of <= ck channels][tap][k-step][cout block][64 lanes],
// over sources padded to PAD channels (a power of two) and k-steps of KSTEP channels; lane l = (cout l & 15 of the block, lane group l >> 4).
// The streams differ in PAD, KSTEP and in what a lane holds: fp32 4 / 4 / 1 float, bf16 16 / 16 / 4 bf16, bf16x3 16 / 16 / 4 hi + 4 lo bf16,
// B8 32 / 32 / 8 bf16 (and ck = 32: a chunk is one k-step).
template <int PAD>
static inline int conv_pad_channels(int c) { return (c + PAD - 1) & ~(PAD - 1); }

static inline int conv_cout_groups(int out_channels, int mb) { return mr_ceil_div(mr_ceil_div(out_channels, 16), mb); }

// 64-lane fragments of a stream; the caller multiplies by the size of its fragment
template <int PAD, int KSTEP>
size_t conv_packed_fragments(int out_channels, const int32_t* src_channels, int num_src, int kh, int kw, int mb) {
    int cpad_total = 0;
    for (int s = 0; s < num_src; ++s) cpad_total += conv_pad_channels<PAD>(src_channels[s]);
    return (size_t)conv_cout_groups(out_channels, mb) * kh * kw * (cpad_total / KSTEP) * mb;
}

// Calls emit(lane group, w) once per lane in stream order; w(c) is the weight of the lane's output channel at channel c (0 .. KSTEP - 1) of
// the k-step, zero for padded channels and padded output channels.  weight: (out_channels, sum(src_channels), kh, kw) fp32, nn.Conv2d layout.
template <int PAD, int KSTEP, class Emit>
void conv_pack_walk(const float* weight, int out_channels, const int32_t* src_channels, int num_src, int kh, int kw, int mb, int ck, Emit emit) {
    const int groups = conv_cout_groups(out_channels, mb);
    const int taps = kh * kw;
    int cin_total = 0;
    for (int s = 0; s < num_src; ++s) cin_total += src_channels[s];
    for (int g = 0; g < groups; ++g) {
        int cin_off = 0;
        for (int s = 0; s < num_src; ++s) {
            const int cpad = conv_pad_channels<PAD>(src_channels[s]);
            for (int c0 = 0; c0 < cpad; c0 += ck) {
                const int ckq = cpad - c0 < ck ? cpad - c0 : ck;
                for (int tap = 0; tap < taps; ++tap)
                    for (int ks = 0; ks < ckq / KSTEP; ++ks)
                        for (int m = 0; m < mb; ++m)
                            for (int lane = 0; lane < 64; ++lane) {
                                const int cout = (g * mb + m) * 16 + (lane & 15);
                                emit(lane >> 4, [&](int c) {
                                    const int cl = c0 + ks * KSTEP + c;
                                    return cout < out_channels && cl < src_channels[s] ? weight[((size_t)cout * cin_total + (cin_off + cl)) * taps + tap] : 0.f;
                                });
                            }
            }
            cin_off += src_channels[s];
        }
    }
}
