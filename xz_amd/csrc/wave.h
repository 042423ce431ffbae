// wave.h -- wavefront helpers and the launch-grid helper shared by the HIP units of the encoder and the decoder.
#ifndef XZAMD_WAVE_H
#define XZAMD_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// Make LDS stores of some lanes visible to later LDS loads of other lanes of the same wavefront:
// LDS hand-off between lanes of the wave.  DS instructions of one wave execute in issue order, so a
// ds_write is visible to any later ds_read of the same wave without waiting; what has to be
// prevented is the COMPILER moving accesses across the hand-off.  A compiler-only barrier: a fence
// builtin would also drain vmcnt, i.e. wait for every prefetch in flight at each hand-off.
__device__ __forceinline__ void wave_sync()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
// Sum over the 64 lanes on the DPP network (no LDS traffic): row-wise shifts, then the two row broadcasts; lane 63 has it.
__device__ __forceinline__ uint32_t wave_sum_dpp(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);     // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);     // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);     // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);     // row_shr:8   -> lane 15 of a row = row sum
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, true);     // row_bcast:15 into rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, true);     // row_bcast:31 into rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// A wave-uniform value the compiler must keep in a scalar register from here on (no instruction is emitted when it is
// there already): without the pin a loop-carried uniform chain can end up on the vector ALU as a whole.
__device__ __forceinline__ void pin_s(uint32_t& v) { asm volatile("" : "+s"(v)); }
__device__ __forceinline__ void pin_s(uint64_t& v) { asm volatile("" : "+s"(v)); }
__device__ __forceinline__ uint32_t lane_of(uint32_t v, uint32_t l) { return __builtin_amdgcn_readlane(v, uni(l)); }

inline uint32_t grid_for(uint64_t n, uint32_t threads, uint32_t cap)
{
    uint64_t g = (n + threads - 1) / threads;
    if (g > cap) g = cap;
    if (g == 0) g = 1;
    return (uint32_t)g;
}

} // namespace

#endif
