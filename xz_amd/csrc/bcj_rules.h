// bcj_rules.h -- the tests the x86 and RISC-V BCJ filters apply alike in both directions: the encoder's k_x86_bcj /
// k_riscv_bcj (lzma_filters.hip) and the decoder's unf_x86 / unf_riscv (lzma_decode.hip).
#ifndef XZAMD_BCJ_RULES_H
#define XZAMD_BCJ_RULES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// x86: an E8 / E9 opcode byte; a most significant operand byte that gets converted
__device__ __forceinline__ bool x86_is_op(uint32_t b) { return (b & 0xFEu) == 0xE8u; }
__device__ __forceinline__ bool x86_ms(uint32_t b) { return b == 0u || b == 0xFFu; }

// RISC-V: rv_step = how far the walk jumps from an examined position, rv_sync = the chunk rule (see k_riscv_bcj)
__device__ __forceinline__ uint32_t rv_rd32(const uint8_t* p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// not a pair: rd of the AUIPC != rs1 of the second instruction, or its two lowest opcode bits are not 11
__device__ __forceinline__ bool rv_not_pair(uint32_t auipc, uint32_t inst2) { return (((auipc << 8) ^ inst2) & 0xF8003u) != 3u; }
// the special form the encoder itself produces: rd = x2, bits 13:12 = 11, and a "rs1" that is neither x0 nor x2
__device__ __forceinline__ bool rv_special(uint32_t auipc) { return (auipc & 0x3FFFu) == 0x3117u && ((auipc >> 27) & 0x1Du) != 0; }
__device__ __forceinline__ uint32_t rv_step(const uint8_t* b, uint32_t i, uint32_t limit)
{
    if (i > limit) return 2;
    const uint32_t b0 = b[i];
    if (b0 == 0xEFu) return (b[i + 1] & 0x0Du) ? 2u : 4u;
    if ((b0 & 0x7Fu) != 0x17u) return 2;
    const uint32_t inst = rv_rd32(b + i);
    if (inst & 0xE80u) return rv_not_pair(inst, rv_rd32(b + i + 4)) ? 6u : 8u;
    return rv_special(inst) ? 8u : 4u;
}
__device__ __forceinline__ bool rv_sync(const uint8_t* b, uint32_t i, uint32_t limit)
{
    return (i < 2 || rv_step(b, i - 2, limit) <= 2) && (i < 4 || rv_step(b, i - 4, limit) <= 4) && (i < 6 || rv_step(b, i - 6, limit) <= 6);
}

} // namespace

#endif
