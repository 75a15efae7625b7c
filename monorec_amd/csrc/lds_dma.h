// LDS-DMA, buffer descriptor, LDS pair read and the branch-free activation shared by the direct kernels (conv_mfma.hip, conv_b8.hip) and
// the reduced-multiply ones (conv_wino.hip, convt_wino.hip, conv1d_wino.hip, conv_wino44{,s,w}.hip).  Device code only; everything is
// force-inlined, so a translation unit pays for what it calls and nothing else.
// (conv_mfma.hip, conv_b8.hip and splitk_epilogue4_kernel keep the activation written out where they store, keep / slope hoisted ahead of
// the store loops: with act_max in its place hipcc clones those loops.)
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/monorec_hip.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- LDS-DMA, issued through inline asm ------------------------------------------------------------------------------------------
// hipcc treats an LDS-DMA builtin as a store that may alias every later ds_read and drains it (vmcnt(0)) before the MFMA sweep of the
// *other* pipeline buffer, which serialises load and compute.  Inline asm is invisible to that pass; the kernel waits itself
// (dma_wait_all / dma_wait_upto) right before the barrier that publishes the buffer.  M0 (LDS base of the DMA) is saved / restored
// inside the statement; `s_nop 4` covers the SALU/VALU-write -> VMEM-SGPR-read hazard the compiler does not pad for asm operands.
// The *_raw forms pass the scalar operands as they are (conv_mfma.hip, whose sweeps were tuned on that code).  The others send them
// through readfirstlane first: values derived from the wave index are uniform, but the compiler may hold them in VGPRs, which the "s"
// constraints of the asm do not fix up.
#define MR_LDS_DMA(INSN) "s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\t" INSN "\n\ts_mov_b32 m0, %0"
__device__ __forceinline__ void dma_buffer_dword_raw(unsigned lds_byte_addr, int voff, i32x4 srd, int soff) {
    unsigned keep;
    asm volatile(MR_LDS_DMA("buffer_load_dword %2, %3, %4 offen lds") : "=&s"(keep) : "s"(lds_byte_addr), "v"(voff), "s"(srd), "s"(soff) : "memory");
}
__device__ __forceinline__ void dma_buffer_x4_raw(unsigned lds_byte_addr, int voff, i32x4 srd, int soff) {
    unsigned keep;
    asm volatile(MR_LDS_DMA("buffer_load_dwordx4 %2, %3, %4 offen lds") : "=&s"(keep) : "s"(lds_byte_addr), "v"(voff), "s"(srd), "s"(soff) : "memory");
}
__device__ __forceinline__ void dma_global_x4_raw(unsigned lds_byte_addr, const void* g) {
    unsigned keep;
    asm volatile(MR_LDS_DMA("global_load_lds_dwordx4 %2, off") : "=&s"(keep) : "s"(lds_byte_addr), "v"(g) : "memory");
}
__device__ __forceinline__ void dma_global_x1_raw(unsigned lds_byte_addr, const void* g) {
    unsigned keep;
    asm volatile(MR_LDS_DMA("global_load_lds_dword %2, off") : "=&s"(keep) : "s"(lds_byte_addr), "v"(g) : "memory");
}
#undef MR_LDS_DMA
__device__ __forceinline__ void dma_buffer_x4(unsigned lds_byte_addr, int voff, i32x4 srd, int soff) {
    dma_buffer_x4_raw(__builtin_amdgcn_readfirstlane(lds_byte_addr), voff, srd, __builtin_amdgcn_readfirstlane(soff));
}
__device__ __forceinline__ void dma_global_x4(unsigned lds_byte_addr, const void* g) { dma_global_x4_raw(__builtin_amdgcn_readfirstlane(lds_byte_addr), g); }
__device__ __forceinline__ void dma_global_x1(unsigned lds_byte_addr, const void* g) { dma_global_x1_raw(__builtin_amdgcn_readfirstlane(lds_byte_addr), g); }
__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// s_waitcnt vmcnt(N) takes an immediate: wait until at most `n` (wave-uniform) of this wave's VMEM instructions are outstanding (rounding down is safe)
#define MR_VMCNT_CASE(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
__device__ __forceinline__ void dma_wait_upto(int n) {
    switch (n < 32 ? n : (n < 48 ? 32 : 48)) {
        MR_VMCNT_CASE(0) MR_VMCNT_CASE(1) MR_VMCNT_CASE(2) MR_VMCNT_CASE(3) MR_VMCNT_CASE(4) MR_VMCNT_CASE(5) MR_VMCNT_CASE(6) MR_VMCNT_CASE(7)
        MR_VMCNT_CASE(8) MR_VMCNT_CASE(9) MR_VMCNT_CASE(10) MR_VMCNT_CASE(11) MR_VMCNT_CASE(12) MR_VMCNT_CASE(13) MR_VMCNT_CASE(14) MR_VMCNT_CASE(15)
        MR_VMCNT_CASE(16) MR_VMCNT_CASE(17) MR_VMCNT_CASE(18) MR_VMCNT_CASE(19) MR_VMCNT_CASE(20) MR_VMCNT_CASE(21) MR_VMCNT_CASE(22) MR_VMCNT_CASE(23)
        MR_VMCNT_CASE(24) MR_VMCNT_CASE(25) MR_VMCNT_CASE(26) MR_VMCNT_CASE(27) MR_VMCNT_CASE(28) MR_VMCNT_CASE(29) MR_VMCNT_CASE(30) MR_VMCNT_CASE(31)
        MR_VMCNT_CASE(32) MR_VMCNT_CASE(48)
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
}

// buffer descriptor over `bytes` bytes from `base`: reads beyond them (and voff = -1, the padding) return zero
__device__ __forceinline__ i32x4 make_srd(const void* base, int bytes) {
    const unsigned long long p = (unsigned long long)base;
    i32x4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(unsigned)p);
    r.y = __builtin_amdgcn_readfirstlane((int)((unsigned)(p >> 32) & 0xffffu));
    r.z = __builtin_amdgcn_readfirstlane(bytes);
    r.w = 0x00020000;
    return r;
}

// One aligned 8-byte LDS read that stays one: left to itself hipcc drops the halves a caller does not use and re-pairs the rest into ds_read2_b32 -
// two dword accesses with the 32-bank rule (volatile keeps the access whole; the explicit LDS address space keeps it a ds_ instruction)
__device__ __forceinline__ f32x2 lds_pair(const float* p) {
    return *(const volatile __attribute__((address_space(3))) f32x2*)(__attribute__((address_space(3))) const float*)p;
}

// none / ReLU / LeakyReLU as ONE branch-free form, max(x, lo) with lo = x (none), 0 (ReLU: -inf -> 0 and no -0.0, like torch.relu),
// x * p0 (LeakyReLU, 0 <= p0 <= 1 - the host side rejects other slopes); lo's selector is wave-uniform: as a
// switch the compiler emitted scalar branches around every stored element of the epilogue (round 4: 200-450 branches per workgroup)
__device__ __forceinline__ float act_max(float v, int act, float p0) {
    const unsigned keep = act == MR_ACT_RELU ? 0u : ~0u;          // (an AND, not a select: a uniform select made hipcc clone the store loops)
    const float lo = __uint_as_float(__float_as_uint(v * (act == MR_ACT_LEAKY_RELU ? p0 : 1.f)) & keep);
    return fmaxf(v, lo);
}
