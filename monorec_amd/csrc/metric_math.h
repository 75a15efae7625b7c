// Per-element helpers shared by the two metric reductions (sparse_metric_sums_kernel in eltwise.hip, metric_stage_sums_kernel in
// select.hip): torch.relu, torch.clamp_min and torch.max as torch computes them - a NaN operand passes through, where fmaxf (maxnum)
// would drop it and score a NaN prediction as a finite depth.  For operands without NaN they are fmaxf, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

__device__ inline float relu_keep_nan(float x) { return x != x ? x : fmaxf(x, 0.f); }
__device__ inline float clamp_keep_nan(float x, float lo) { return x != x ? x : fmaxf(x, lo); }
__device__ inline float max_keep_nan(float a, float c) { return (a != a || c != c) ? __uint_as_float(0x7fc00000u) : fmaxf(a, c); }
