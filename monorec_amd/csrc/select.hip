// Median scaling (reference utils/util.py:135-142, evaluater/evaluater.py:36-43) and the dense-target metrics
// (model/metric_functions/sparse_metrics.py:6-78) on the MI355X (gfx950).
//
//   masked_select_kernel      exact lower median of target[target > 0] and the prediction's sorted[(n-1)/2], sorted[n/2]
//                             over the same mask, per sample: radix select over order-preserving keys of the fp32 bit
//                             patterns, digits counted in LDS histograms with integer atomics (exact and deterministic,
//                             whatever order the compaction wrote the keys in).  One workgroup per (sample, tensor).
//   stage_scales_kernel       the ratios of k median_scaling calls in a row, from those statistics (one wave).
//   metric_stage_sums_kernel  one pass: per stage the prediction is multiplied by that stage's ratio (fp32, compounding
//                             like the reference) and one metric sum is accumulated (fp64, fixed reduction order).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/monorec_hip.h"
#include "metric_math.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 2048;     // digits of 11, 11 and 10 bits, most significant first

// order-preserving key: negatives get all bits flipped, the rest only the sign bit (NaNs land beyond +-inf; only counted)
__device__ inline uint32_t key_of(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline float float_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// bin of the histogram holding `rank` (0-based, counted from the smallest key); bin and rank within it -> LDS. Wave 0 only.
__device__ inline void find_bin(const uint32_t* hist, int bins, uint32_t rank, uint32_t* out_bin, uint32_t* out_rank) {
    const int lane = threadIdx.x & 63, per = bins / 64;
    uint32_t s = 0;
    for (int j = 0; j < per; ++j) s += hist[lane * per + j];
    uint32_t incl = s;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
    }
    uint32_t c = incl - s;
    if (c <= rank && rank < incl) {                     // exactly one lane
        for (int j = 0; j < per; ++j) {
            const uint32_t h = hist[lane * per + j];
            if (rank < c + h) {
                *out_bin = (uint32_t)(lane * per + j);
                *out_rank = rank - c;
                break;
            }
            c += h;
        }
    }
}

__global__ __launch_bounds__(kThreads) void masked_select_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                  int n, uint32_t* __restrict__ work, mr_median_stats* stats) {
    __shared__ uint32_t hist[kBins];
    __shared__ uint32_t s_count, s_nan, s_zero, s_inf, s_bin, s_rank, s_le, s_above;
    const int b = blockIdx.x, which = blockIdx.y;        // which: 0 = target, 1 = prediction
    const int tid = threadIdx.x, lane = tid & 63;
    const float* g = gt + (long long)b * n;
    const float* p = pred + (long long)b * n;
    uint32_t* keys = work + ((long long)b * 2 + which) * n;
    for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
    if (tid == 0) { s_count = 0; s_nan = 0; s_zero = 0; s_inf = 0; s_le = 0; s_above = 0xffffffffu; }
    __syncthreads();

    // pass 1: compact the selected values into `keys` (one LDS atomic per wave and step), histogram of the top digit, flags
    uint32_t nan = 0, zero = 0, inf = 0;
    for (int base = 0; base < n; base += 4 * kThreads) {
        float t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * kThreads + tid;
            t[u] = i < n ? g[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * kThreads + tid;
            const bool sel = t[u] > 0.f;                  // NaN targets are never selected
            const unsigned long long m = __ballot(sel);
            if (!m) continue;                             // wave-uniform
            uint32_t wbase = 0;
            if (lane == 0) wbase = atomicAdd(&s_count, (uint32_t)__popcll(m));
            wbase = __shfl(wbase, 0, 64);
            if (sel) {
                const float v = which ? p[i] : t[u];
                const uint32_t k = key_of(v);
                keys[wbase + __popcll(m & ((1ull << lane) - 1ull))] = k;
                atomicAdd(&hist[k >> 21], 1u);
                nan += v != v;
                zero += v == 0.f;
                inf += isinf(v);
            }
        }
    }
    if (which) {
        if (nan) atomicAdd(&s_nan, nan);
        if (zero) atomicAdd(&s_zero, zero);
        if (inf) atomicAdd(&s_inf, inf);
    }
    __syncthreads();
    const uint32_t m = s_count;
    if (m == 0) {
        if (tid == 0) {
            if (which == 0) { stats[b].count = 0; stats[b].target_median = __uint_as_float(0x7fc00000u); stats[b].reserved = 0; }
            else { stats[b].lo = stats[b].hi = __uint_as_float(0x7fc00000u); stats[b].nans = 0; stats[b].zeros = 0; stats[b].infs = 0; }
        }
        return;
    }

    // passes 2, 3: the next digits, counting only the keys that share the digits found so far
    const uint32_t lo_rank = (m - 1) / 2;
    uint32_t prefix = 0, rank = lo_rank;
    for (int d = 0; d < 3; ++d) {
        const int shift = d == 0 ? 21 : (d == 1 ? 10 : 0);
        const int bins = d == 2 ? 1024 : 2048;
        if (d > 0) {
            const int top = shift + (d == 2 ? 10 : 11);
            for (uint32_t i = tid; i < m; i += kThreads) {
                const uint32_t k = keys[i];
                if ((k >> top) == (prefix >> top)) atomicAdd(&hist[(k >> shift) & (bins - 1)], 1u);
            }
            __syncthreads();
        }
        if (tid < 64) find_bin(hist, bins, rank, &s_bin, &s_rank);
        __syncthreads();
        prefix |= s_bin << shift;
        rank = s_rank;
        __syncthreads();                                  // everybody has read s_bin / s_rank
        if (d < 2) {
            for (int i = tid; i < kBins; i += kThreads) hist[i] = 0;
            __syncthreads();
        }
    }
    if (which == 0) {
        if (tid == 0) { stats[b].count = (int32_t)m; stats[b].target_median = float_of(prefix); stats[b].reserved = 0; }
        return;
    }
    // sorted[m/2]: the same key when more than lo_rank + 1 keys are <= it (or m is odd), else the smallest key above it
    uint32_t le = 0, above = 0xffffffffu;
    for (uint32_t i = tid; i < m; i += kThreads) {
        const uint32_t k = keys[i];
        if (k <= prefix) ++le;
        else above = k < above ? k : above;
    }
    if (le) atomicAdd(&s_le, le);
    atomicMin(&s_above, above);
    __syncthreads();
    if (tid == 0) {
        const bool same = (m & 1u) || s_le > lo_rank + 1;
        stats[b].lo = float_of(prefix);
        stats[b].hi = float_of(same ? prefix : s_above);
        stats[b].nans = (int32_t)s_nan;
        stats[b].zeros = (int32_t)s_zero;
        stats[b].infs = (int32_t)s_inf;
    }
}

// torch.median(target[mask]) / torch.median(prediction[mask]) of each of `stages` median_scaling calls in a row.  After a
// finite non-zero ratio r the selection is p*r: sorted order kept (r > 0) or reversed (r < 0), so its new lower median is
// lo*r resp. hi*r; NaN stays NaN, 0 stays 0, inf stays inf.  A ratio of 0 turns inf into NaN and everything else into 0; an
// infinite ratio turns 0 into NaN and everything else into inf; a NaN ratio makes everything NaN.
__global__ __launch_bounds__(64) void stage_scales_kernel(const mr_median_stats* stats, int batch, int stages, float* scales,
                                                          mr_median_stats* out) {
    const float qnan = __uint_as_float(0x7fc00000u);
    for (int b = threadIdx.x; b < batch; b += 64) {
        mr_median_stats s = stats[b];
        for (int j = 0; j < stages; ++j) {
            const float r = (s.count == 0 || s.nans) ? qnan : s.target_median / s.lo;
            scales[(long long)b * stages + j] = r;
            if (r != r || (r == 0.f && s.infs) || (isinf(r) && s.zeros)) {
                s.nans = 1;
                s.lo = s.hi = qnan;
                continue;
            }
            const float a = s.lo * r, c = s.hi * r;
            s.lo = signbit(r) ? c : a;
            s.hi = signbit(r) ? a : c;
            if (r == 0.f) { s.zeros = s.count; s.infs = 0; }
            else if (isinf(r)) { s.infs = s.count; s.zeros = 0; }
        }
        if (out) out[b] = s;
    }
}

struct StageArgs {
    int num;
    int col[MR_MAX_METRIC_STAGES];
};

// One 1024-thread workgroup per sample, fp32 per element, fp64 accumulation, fixed reduction order.
__global__ __launch_bounds__(kThreads) void metric_stage_sums_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                      int H, int W, int y0, int y1, int x0, int x1,
                                                                      float inv_max_dist, const float* __restrict__ scales,
                                                                      const StageArgs st, double* __restrict__ out) {
    __shared__ double red[MR_MAX_METRIC_STAGES + 1][kWaves];
    const int b = blockIdx.x;
    const float* p = pred + (long long)b * H * W;
    const float* g = gt + (long long)b * H * W;
    const int rw = x1 - x0, n = (y1 - y0) * rw;
    float sc[MR_MAX_METRIC_STAGES];
#pragma unroll
    for (int j = 0; j < MR_MAX_METRIC_STAGES; ++j) sc[j] = (scales && j < st.num) ? scales[(long long)b * st.num + j] : 1.f;
    double acc[MR_MAX_METRIC_STAGES + 1];
#pragma unroll
    for (int j = 0; j <= MR_MAX_METRIC_STAGES; ++j) acc[j] = 0.0;
    const float t1 = 1.25f, t2 = (float)(1.25 * 1.25), t3 = (float)(1.25 * 1.25 * 1.25);
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int y = y0 + i / rw, x = x0 + i % rw;
        const float gi = g[y * W + x];
        float v = p[y * W + x];
        const bool masked = gi == 0.f || (inv_max_dist > 0.f && gi < inv_max_dist);     // get_mask
        acc[0] += masked ? 0.0 : 1.0;
        float gg = relu_keep_nan(gi);                                                    // get_positive_depth
        if (inv_max_dist > 0.f) gg = clamp_keep_nan(gg, inv_max_dist);                   // get_absolute_depth
        const float dg = 1.0f / gg;
#pragma unroll
        for (int j = 0; j < MR_MAX_METRIC_STAGES; ++j) {          // fully unrolled: sc[] and acc[] stay in registers
            if (j < st.num) {
                if (scales) v = v * sc[j];                                                // median_scaling, compounding
                const int col = st.col[j];
                if ((col & MR_METRIC_DENSE) || !masked) {
                    float pp = relu_keep_nan(v);
                    if (inv_max_dist > 0.f) pp = clamp_keep_nan(pp, inv_max_dist);
                    const float dp = 1.0f / pp;
                    const float d = dp - dg;
                    float q;
                    switch (col & 0xff) {
                        case 1: q = fabsf(d) / dg; break;
                        case 2: q = (d * d) / dg; break;
                        case 3: q = d * d; break;
                        case 4: { const float lg = logf(dp) - logf(dg); q = lg * lg; break; }
                        default: {
                            const float a = dg / dp, c = dp / dg;
                            const float th = max_keep_nan(a, c);                       // torch.max keeps NaN
                            const float t = (col & 0xff) == 5 ? t1 : ((col & 0xff) == 6 ? t2 : t3);
                            q = th < t ? 1.f : 0.f;
                        }
                    }
                    acc[1 + j] += (double)q;
                }
            }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k <= MR_MAX_METRIC_STAGES; ++k) {
        if (k <= st.num) {
            double v = acc[k];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if (lane == 0) red[k][wave] = v;
        }
    }
    __syncthreads();
    const int cols = 2 + st.num;
    if (threadIdx.x <= st.num) {
        double v = 0;
        for (int w = 0; w < kWaves; ++w) v += red[threadIdx.x][w];
        out[(long long)b * cols + (threadIdx.x == 0 ? 0 : 1 + threadIdx.x)] = v;
    } else if (threadIdx.x == st.num + 1) {
        out[(long long)b * cols + 1] = (double)n;
    }
}

}  // namespace

extern "C" int64_t mr_median_select_workspace_bytes(int32_t batch, int32_t height, int32_t width) {
    if (batch < 1 || height < 1 || width < 1) return -1;
    return (int64_t)2 * batch * height * width * (int64_t)sizeof(uint32_t);
}

extern "C" int mr_median_select_f32(const float* prediction, const float* target, int32_t batch, int32_t height, int32_t width,
                                    void* workspace, mr_median_stats* stats, void* stream) {
    if (!prediction || !target || !workspace || !stats || batch < 1 || height < 1 || width < 1) return MR_ERR_BAD_ARGUMENT;
    const long long n = (long long)height * width;
    if (n > 0x7fffffffll - 4 * kThreads) return MR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(masked_select_kernel, dim3((unsigned)batch, 2), dim3(kThreads), 0, (hipStream_t)stream, prediction, target,
                       (int)n, (uint32_t*)workspace, stats);
    return (int)hipGetLastError();
}

extern "C" int mr_median_stage_scales_f32(const mr_median_stats* stats, int32_t batch, int32_t num_stages, float* scales,
                                          mr_median_stats* stats_out, void* stream) {
    if (!stats || !scales || batch < 1 || num_stages < 1) return MR_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(stage_scales_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, batch, num_stages, scales, stats_out);
    return (int)hipGetLastError();
}

extern "C" int mr_metric_stage_sums_f32(const float* prediction, const float* target, int32_t batch, int32_t height, int32_t width,
                                        const int32_t* roi, float max_distance, const float* scales, int32_t num_stages,
                                        const int32_t* stage_columns, double* sums, void* stream) {
    if (!prediction || !target || !sums || !stage_columns || batch < 1 || height < 1 || width < 1 || num_stages < 1 ||
        num_stages > MR_MAX_METRIC_STAGES)
        return MR_ERR_BAD_ARGUMENT;
    int y0 = 0, y1 = height, x0 = 0, x1 = width;
    if (roi) { y0 = roi[0]; y1 = roi[1]; x0 = roi[2]; x1 = roi[3]; }
    if (y0 < 0 || x0 < 0 || y1 > height || x1 > width || y1 <= y0 || x1 <= x0) return MR_ERR_BAD_ARGUMENT;
    StageArgs st;
    st.num = num_stages;
    for (int j = 0; j < MR_MAX_METRIC_STAGES; ++j) {
        const int c = j < num_stages ? stage_columns[j] : 1;
        if ((c & 0xff) < 1 || (c & 0xff) > 7 || (c & ~(0xff | MR_METRIC_DENSE))) return MR_ERR_BAD_ARGUMENT;
        st.col[j] = c;
    }
    const float inv = max_distance > 0.f ? 1.0f / max_distance : 0.f;
    hipLaunchKernelGGL(metric_stage_sums_kernel, dim3((unsigned)batch), dim3(kThreads), 0, (hipStream_t)stream, prediction, target,
                       height, width, y0, y1, x0, x1, inv, scales, st, sums);
    return (int)hipGetLastError();
}
