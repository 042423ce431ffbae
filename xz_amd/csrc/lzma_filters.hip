// lzma_filters.hip -- the filters in front of the LZMA2 coder and the integrity checks (stage table: lzma_kernels.hip).
// The inverse filters live in lzma_decode.hip; the tests both directions share are in bcj_rules.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_api.h"
#include "wave.h"
#include "bcj_rules.h"
#include "delta_rule.h"
#include "auto_bcj_rule.h"
#include "lclp_rule.h"

namespace {

// ------------------------------------------------------------------------------------------
// x86 BCJ encoder (simple/x86.c:26-118), one Block = one fresh filter (x86.c:121-136), start offset 0.
// The filter is a sequential state machine, but (1) every decision reads ORIGINAL bytes only -- a
// converted CALL/JMP skips its own four operand bytes, nothing re-reads a patched byte -- and (2) its
// state (prev_mask, prev_pos) is void at any position preceded by five bytes without an E8/E9: the
// next opcode then sees offset > 5 and clears prev_mask whatever came before, and no conversion can
// straddle such a position.  So a chunk owner starts at the first such synchronisation point of its
// chunk and runs to the first one at or after the chunk end (= where the next owner starts): exact,
// chunk-parallel, and sequential only on input without synchronisation points.
// `out` already holds a copy of `in`; only converted operands are written.  With `kind` (the automatic per-Block BCJ
// filter) only the Blocks whose kind[blk] is this filter's id are filtered; the others stay the copy.
// ------------------------------------------------------------------------------------------
constexpr uint32_t BCJ_CHUNK = 2048;

__global__ __launch_bounds__(256) void k_x86_bcj(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n,
        uint32_t block_size, uint32_t chunks_per_block, uint32_t nchunks, const uint32_t* __restrict__ kind)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const uint32_t blk = t / chunks_per_block, k = t - blk * chunks_per_block;
    const uint32_t bs = blk * block_size;
    if (bs >= n) return;
    if (kind && kind[blk] != 4u) return;
    const uint32_t size = min(n - bs, block_size);
    if (size < 5) return;
    const uint32_t limit = size - 5;                 // last position the filter examines
    const uint32_t s = k * BCJ_CHUNK;
    if (s > limit) return;
    const uint32_t e = s + BCJ_CHUNK;                // may exceed size; only compared
    const uint8_t* __restrict__ b = in + bs;
    uint8_t* __restrict__ o = out + bs;
    uint32_t pos = 0, run = 0;                       // run = non-opcode bytes immediately before pos
    if (k != 0) {
        bool found = false;
        for (uint32_t q = s - 5; q <= limit && q < e; ++q) {
            if (q >= s && run >= 5) { pos = q; found = true; break; }
            run = x86_is_op(b[q]) ? 0u : run + 1;
        }
        if (!found) return;                           // the previous owner runs through this chunk
    }
    uint32_t prev_mask = 0, prev_pos = pos - 6;       // "long ago" (x86.c:133: -5 at the Block start acts the same)
    while (pos <= limit) {
        if (pos >= e && run >= 5) break;              // next owner's start
        const uint32_t c = b[pos];
        if (!x86_is_op(c)) { ++pos; ++run; continue; }
        const uint32_t offset = pos - prev_pos;
        prev_pos = pos;
        if (offset > 5) prev_mask = 0;
        else for (uint32_t i = 0; i < offset; ++i) prev_mask = (prev_mask & 0x77u) << 1;
        uint32_t b4 = b[pos + 4];
        if (x86_ms(b4) && (prev_mask >> 1) <= 4 && (prev_mask >> 1) != 3) {
            const uint32_t b1 = b[pos + 1], b2 = b[pos + 2], b3 = b[pos + 3];
            uint32_t src = (b4 << 24) | (b3 << 16) | (b2 << 8) | b1;
            uint32_t dest;
            for (;;) {
                dest = src + (pos + 5);
                if (prev_mask == 0) break;
                const uint32_t pm = prev_mask >> 1;
                const uint32_t i = pm == 0 ? 0u : pm == 1 ? 1u : pm <= 3 ? 2u : 3u;    // MASK_TO_BIT_NUMBER
                const uint32_t bb = (dest >> (24 - i * 8)) & 0xFFu;
                if (!x86_ms(bb)) break;
                src = dest ^ ((1u << (32 - i * 8)) - 1);
            }
            o[pos + 4] = (uint8_t)(~(((dest >> 24) & 1) - 1));
            o[pos + 3] = (uint8_t)(dest >> 16);
            o[pos + 2] = (uint8_t)(dest >> 8);
            o[pos + 1] = (uint8_t)dest;
            run = x86_is_op(b1) ? 0u : 1u;
            run = x86_is_op(b2) ? 0u : run + 1;
            run = x86_is_op(b3) ? 0u : run + 1;
            run = x86_is_op(b4) ? 0u : run + 1;
            pos += 5;
            prev_mask = 0;
        } else {
            ++pos;
            run = 0;
            prev_mask |= 1;
            if (x86_ms(b4)) prev_mask |= 0x10;
        }
    }
}

// ------------------------------------------------------------------------------------------
// ARM64 BCJ encoder (simple/arm64.c:20-105) and delta encoder (delta/delta_encoder.c:20-45), one fresh
// filter per Block, start offset 0.  Both are stateless given the ORIGINAL bytes (ARM64: every aligned
// 4-byte instruction on its own, pc = offset inside the Block; delta: byte minus the byte `dist` before it
// in the Block, zero history), so they are plain data-parallel maps -- one thread per instruction / byte.
// k_arm64_bcj with `kind`: only the Blocks whose kind[b] is 0x0A, as in k_x86_bcj.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_arm64_bcj(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n,
        uint32_t block_size, uint32_t nblocks, const uint32_t* __restrict__ kind)
{
    const uint32_t spb = block_size / 4;                      // instruction slots per full Block
    if (spb == 0) return;
    const uint64_t total = (uint64_t)spb * nblocks;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint32_t b = (uint32_t)(t / spb), k = (uint32_t)(t - (uint64_t)b * spb);
        const uint32_t bs = b * block_size;
        if (bs >= n) continue;
        if (kind && kind[b] != 0x0Au) continue;
        const uint32_t len = min(n - bs, block_size) & ~3u;   // arm64.c:26: the tail (size & 3) stays as it is
        const uint32_t pc = k * 4;
        if (pc + 4 > len) continue;
        const uint32_t g = bs + pc;
        uint32_t instr;
        __builtin_memcpy(&instr, in + g, 4);
        if ((instr >> 26) == 0x25) {
            instr = 0x94000000u | ((instr + (pc >> 2)) & 0x03FFFFFFu);
            __builtin_memcpy(out + g, &instr, 4);
        } else if ((instr & 0x9F000000u) == 0x90000000u) {
            const uint32_t src = ((instr >> 29) & 3) | ((instr >> 3) & 0x001FFFFCu);
            if ((src + 0x00020000u) & 0x001C0000u) continue;
            instr &= 0x9000001Fu;
            const uint32_t dest = src + (pc >> 12);
            instr |= (dest & 3) << 29;
            instr |= (dest & 0x0003FFFCu) << 3;
            instr |= (0u - (dest & 0x00020000u)) & 0x00E00000u;
            __builtin_memcpy(out + g, &instr, 4);
        }
    }
}

// ARM / PowerPC / SPARC (simple/arm.c, powerpc.c, sparc.c: one 4-byte instruction per slot), ARM-Thumb
// (simple/armthumb.c: 2-byte slots, a BL pair is 4 bytes) and IA-64 (simple/ia64.c: 16-byte bundles of three
// 41-bit slots).  pc = offset inside the Block (start offset 0); the tail the reference leaves unfiltered
// (size & 3, size & 15, the last < 4 bytes) stays as it is.  Every slot converts on its own: in ARM-Thumb the
// reference skips the halfword behind a converted pair, but that halfword can never start a pair itself (its
// second byte would have to be 0xF0..0xF7 and 0xF8..0xFF at once), so the slots are independent there too.
__global__ __launch_bounds__(256) void k_bcj_simple(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n,
        uint32_t block_size, uint32_t nblocks, uint32_t kind)
{
    const uint32_t unit = kind == 8 ? 2u : kind == 6 ? 16u : 4u;
    const uint32_t spb = block_size / unit;                   // slots per full Block
    if (spb == 0) return;
    const uint64_t total = (uint64_t)spb * nblocks;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint32_t b = (uint32_t)(t / spb), k = (uint32_t)(t - (uint64_t)b * spb);
        const uint32_t bs = b * block_size;
        if (bs >= n) continue;
        const uint32_t blen = min(n - bs, block_size);
        const uint32_t pc = k * unit;
        const uint8_t* p = in + bs + pc;
        uint8_t* q = out + bs + pc;
        if (kind == 8) {                                      // ARM-Thumb BL pair
            if (blen < 4 || pc > blen - 4) continue;
            if ((p[1] & 0xF8u) != 0xF0u || (p[3] & 0xF8u) != 0xF8u) continue;
            uint32_t src = ((uint32_t)(p[1] & 7u) << 19) | ((uint32_t)p[0] << 11) | ((uint32_t)(p[3] & 7u) << 8) | p[2];
            src <<= 1;
            const uint32_t dest = (pc + 4 + src) >> 1;
            q[1] = (uint8_t)(0xF0u | ((dest >> 19) & 7u));
            q[0] = (uint8_t)(dest >> 11);
            q[3] = (uint8_t)(0xF8u | ((dest >> 8) & 7u));
            q[2] = (uint8_t)dest;
        } else if (kind == 6) {                               // IA-64 bundle
            if (pc + 16 > (blen & ~15u)) continue;
            uint8_t bun[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) bun[i] = p[i];
            const uint32_t tmpl = bun[0] & 0x1Fu;
            // branch slots by template (ia64.c BRANCH_TABLE): 16,17: 4  18,19: 6  22,23: 7  24,25,28,29: 4
            const uint32_t mask = (tmpl == 16 || tmpl == 17 || tmpl == 24 || tmpl == 25 || tmpl == 28 || tmpl == 29) ? 4u
                    : (tmpl == 18 || tmpl == 19) ? 6u : (tmpl == 22 || tmpl == 23) ? 7u : 0u;
            bool changed = false;
            uint32_t bit_pos = 5;
            for (uint32_t slot = 0; slot < 3; ++slot, bit_pos += 41) {
                if (((mask >> slot) & 1u) == 0) continue;
                const uint32_t byte_pos = bit_pos >> 3, bit_res = bit_pos & 7u;
                uint64_t instruction = 0;
                for (uint32_t j = 0; j < 6; ++j) instruction += (uint64_t)bun[j + byte_pos] << (8 * j);
                uint64_t norm = instruction >> bit_res;
                if (((norm >> 37) & 0xFu) != 0x5u || ((norm >> 9) & 0x7u) != 0) continue;
                uint32_t src = (uint32_t)((norm >> 13) & 0xFFFFFu);
                src |= (uint32_t)((norm >> 36) & 1u) << 20;
                src <<= 4;
                const uint32_t dest = (pc + src) >> 4;
                norm &= ~((uint64_t)0x8FFFFF << 13);
                norm |= (uint64_t)(dest & 0xFFFFFu) << 13;
                norm |= (uint64_t)(dest & 0x100000u) << (36 - 20);
                instruction &= (1u << bit_res) - 1;
                instruction |= norm << bit_res;
                for (uint32_t j = 0; j < 6; ++j) bun[j + byte_pos] = (uint8_t)(instruction >> (8 * j));
                changed = true;
            }
            if (changed) {
#pragma unroll
                for (int i = 0; i < 16; ++i) q[i] = bun[i];
            }
        } else {
            if (pc + 4 > (blen & ~3u)) continue;
            if (kind == 7) {                                  // ARM BL (little endian, condition "always")
                if (p[3] != 0xEBu) continue;
                uint32_t src = ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
                src <<= 2;
                const uint32_t dest = (pc + 8 + src) >> 2;
                q[2] = (uint8_t)(dest >> 16); q[1] = (uint8_t)(dest >> 8); q[0] = (uint8_t)dest;
            } else if (kind == 5) {                           // PowerPC b/bl with AA = 0, LK = 1 (big endian)
                if ((p[0] >> 2) != 0x12u || (p[3] & 3u) != 1u) continue;
                const uint32_t src = ((uint32_t)(p[0] & 3u) << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (p[3] & ~3u);
                const uint32_t dest = pc + src;
                q[0] = (uint8_t)(0x48u | ((dest >> 24) & 3u));
                q[1] = (uint8_t)(dest >> 16);
                q[2] = (uint8_t)(dest >> 8);
                q[3] = (uint8_t)((p[3] & 3u) | (dest & 0xFFu));
            } else {                                          // SPARC call (big endian)
                if (!((p[0] == 0x40u && (p[1] & 0xC0u) == 0x00u) || (p[0] == 0x7Fu && (p[1] & 0xC0u) == 0xC0u))) continue;
                uint32_t src = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
                src <<= 2;
                uint32_t dest = (pc + src) >> 2;
                dest = (((0u - ((dest >> 22) & 1u)) << 22) & 0x3FFFFFFFu) | (dest & 0x3FFFFFu) | 0x40000000u;
                q[0] = (uint8_t)(dest >> 24); q[1] = (uint8_t)(dest >> 16); q[2] = (uint8_t)(dest >> 8); q[3] = (uint8_t)dest;
            }
        }
    }
}

// RISC-V (simple/riscv.c:352-609, encoder).  The reference walks the Block in 2-byte steps; what it finds at an
// examined position decides how far it jumps: 2 (nothing), 4 (a converted JAL, or an AUIPC with rd x0/x2 that is
// not the special form), 6 (an AUIPC that has no partner), 8 (a converted AUIPC pair in either direction).  All
// of that is read from bytes no earlier conversion has touched, so step(i) is a function of the input, and a
// position is examined unless an examined position 2, 4 or 6 bytes before it jumps over it.  Hence the
// synchronisation rule used to cut the walk into chunks (the x86 kernel above does the same with its own
// rule): a position whose three predecessors cannot reach over it whatever their state -- step(i-2) <= 2,
// step(i-4) <= 4, step(i-6) <= 6 -- is examined by every walk.  Each chunk's owner starts at the first such
// position inside its chunk and stops at the first one behind its chunk.
__global__ __launch_bounds__(256) void k_riscv_bcj(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n,
        uint32_t block_size, uint32_t chunks_per_block, uint32_t nchunks)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nchunks) return;
    const uint32_t blk = t / chunks_per_block, k = t - blk * chunks_per_block;
    const uint32_t bs = blk * block_size;
    if (bs >= n) return;
    const uint32_t size = min(n - bs, block_size);
    if (size < 8) return;
    const uint32_t limit = size - 8;                 // last position the filter examines (riscv.c:364-372)
    const uint32_t s = k * BCJ_CHUNK;                // BCJ_CHUNK is even
    if (s > limit) return;
    const uint32_t e = s + BCJ_CHUNK;
    const uint8_t* __restrict__ b = in + bs;
    uint8_t* __restrict__ o = out + bs;
    uint32_t pos = 0;
    if (k != 0) {
        bool found = false;
        for (uint32_t q = s; q <= limit && q < e; q += 2)
            if (rv_sync(b, q, limit)) { pos = q; found = true; break; }
        if (!found) return;                          // the previous owner walks through this chunk
    }
    while (pos <= limit) {
        if (pos >= e && rv_sync(b, pos, limit)) break;      // the next owner's start
        const uint32_t b0 = b[pos];
        if (b0 == 0xEFu) {
            // JAL with rd = x1 / x5: pc-relative 20-bit immediate -> absolute, stored big endian (riscv.c:379-438)
            const uint32_t b1 = b[pos + 1];
            if (b1 & 0x0Du) { pos += 2; continue; }
            const uint32_t b2 = b[pos + 2], b3 = b[pos + 3];
            uint32_t addr = ((b1 & 0xF0u) << 8) | ((b2 & 0x0Fu) << 16) | ((b2 & 0x10u) << 7) | ((b2 & 0xE0u) >> 4)
                    | ((b3 & 0x7Fu) << 4) | ((b3 & 0x80u) << 13);
            addr += pos;
            o[pos + 1] = (uint8_t)((b1 & 0x0Fu) | ((addr >> 13) & 0xF0u));
            o[pos + 2] = (uint8_t)(addr >> 9);
            o[pos + 3] = (uint8_t)(addr >> 1);
            pos += 4;
        } else if ((b0 & 0x7Fu) == 0x17u) {
            uint32_t inst = rv_rd32(b + pos);
            if (inst & 0xE80u) {
                // AUIPC with rd other than x0 / x2 (riscv.c:440-551)
                const uint32_t inst2 = rv_rd32(b + pos + 4);
                if (rv_not_pair(inst, inst2)) { pos += 6; continue; }
                uint32_t addr = inst & 0xFFFFF000u;
                addr += (inst2 >> 20) - ((inst2 >> 19) & 0x1000u);
                addr += pos;
                inst = 0x17u | (2u << 7) | (inst2 << 12);
                o[pos] = (uint8_t)inst; o[pos + 1] = (uint8_t)(inst >> 8); o[pos + 2] = (uint8_t)(inst >> 16); o[pos + 3] = (uint8_t)(inst >> 24);
                o[pos + 4] = (uint8_t)(addr >> 24); o[pos + 5] = (uint8_t)(addr >> 16); o[pos + 6] = (uint8_t)(addr >> 8); o[pos + 7] = (uint8_t)addr;
            } else {
                // AUIPC with rd x0 / x2: only the special form is (un)converted (riscv.c:552-602)
                if (!rv_special(inst)) { pos += 4; continue; }
                const uint32_t fake_rs1 = inst >> 27;
                const uint32_t fake_addr = rv_rd32(b + pos + 4);
                const uint32_t fake_inst2 = (inst >> 12) | (fake_addr << 20);
                inst = 0x17u | (fake_rs1 << 7) | (fake_addr & 0xFFFFF000u);
                o[pos] = (uint8_t)inst; o[pos + 1] = (uint8_t)(inst >> 8); o[pos + 2] = (uint8_t)(inst >> 16); o[pos + 3] = (uint8_t)(inst >> 24);
                o[pos + 4] = (uint8_t)fake_inst2; o[pos + 5] = (uint8_t)(fake_inst2 >> 8); o[pos + 6] = (uint8_t)(fake_inst2 >> 16);
                o[pos + 7] = (uint8_t)(fake_inst2 >> 24);
            }
            pos += 8;
        } else {
            pos += 2;
        }
    }
}

__global__ __launch_bounds__(256) void k_delta(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n,
        uint32_t block_size, uint32_t dist)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint32_t bs = (g / block_size) * block_size;
        const uint8_t prev = g - bs >= dist ? in[g - dist] : (uint8_t)0;
        out[g] = (uint8_t)(in[g] - prev);
    }
}

// ------------------------------------------------------------------------------------------
// Automatic per-Block delta filter (delta_rule.h, DESIGN.md 3.5 "Automatic delta"): byte histograms of the Block
// under every candidate distance over a sample of the Block, an integer entropy cost per candidate, the choice, and the
// delta encoder with the distance read per Block.
// ------------------------------------------------------------------------------------------
constexpr uint32_t AD_RUN = 8;            // sample windows per workgroup of k_delta_stats
__device__ const uint8_t AD_LOG[256] = XZAMD_AD_LOG_TABLE;

// One workgroup = AD_RUN consecutive sample windows of one Block; a thread = 16 bytes of a window and the 32 bytes in
// front of them (three 16-byte loads where they lie inside the Block, single bytes at its two ends).  The 11 histograms
// live in LDS and are added to the Block's in global memory once per workgroup.  hist must be zero on entry.
__global__ __launch_bounds__(256) void k_delta_stats(const uint8_t* __restrict__ in, uint32_t n, uint32_t block_size,
        uint32_t runs_per_block, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[XZAMD_AD_HIST_WORDS];
    const uint32_t blk = blockIdx.x / runs_per_block, run = blockIdx.x - blk * runs_per_block;
    const uint64_t bs = (uint64_t)blk * block_size;
    if (bs >= n) return;
    const uint32_t blen = (uint32_t)min((uint64_t)block_size, (uint64_t)n - bs);
    const uint8_t* __restrict__ b = in + bs;
    for (uint32_t i = threadIdx.x; i < XZAMD_AD_HIST_WORDS; i += 256) h[i] = 0;
    __syncthreads();
    for (uint32_t w = run * AD_RUN; w < (run + 1) * AD_RUN; ++w) {
        const uint64_t o64 = (uint64_t)w * XZAMD_AD_PERIOD + threadIdx.x * 16u;     // of this thread's 16 bytes in the Block
        if (o64 >= blen) break;
        const uint32_t o = (uint32_t)o64;
        uint32_t x[12];                                   // bytes o - 32 .. o + 15 of the Block, zero outside of it
        if (o >= 32 && o + 16 <= blen) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                uint4 v;
                __builtin_memcpy(&v, b + o - 32 + 16 * q, 16);
                x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t p = (int64_t)o - 32 + 4 * q + k;
                    if (p >= 0 && p < (int64_t)blen) v |= (uint32_t)b[p] << (8 * k);
                }
                x[q] = v;
            }
        }
        const uint32_t cnt = min(16u, blen - o);          // sampled bytes of this thread
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((uint32_t)j < cnt) {
                const uint32_t cur = (x[8 + j / 4] >> (8 * (j & 3))) & 255u;
#pragma unroll
                for (uint32_t k = 0; k < XZAMD_AD_NCAND; ++k) {
                    const int p = 32 + j - (int)xzamd_ad_dist(k);      // k == 0: the byte itself, minus nothing
                    const uint32_t prev = k == 0 ? 0u : (x[p / 4] >> (8 * (p & 3))) & 255u;
                    atomicAdd(&h[k * 256 + ((cur - prev) & 255u)], 1u);
                }
            }
        }
    }
    __syncthreads();
    uint32_t* __restrict__ g = hist + (uint64_t)blk * XZAMD_AD_HIST_WORDS;
    for (uint32_t i = threadIdx.x; i < XZAMD_AD_HIST_WORDS; i += 256)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

// One wavefront per Block: S(k) = Ns * L(Ns) - sum_v hist[k][v] * L(hist[k][v]) for the 11 candidates, the rule,
// dist[b] = the chosen distance (0: no filter).
__global__ __launch_bounds__(64) void k_delta_choose(const uint32_t* __restrict__ hist, uint32_t nblocks,
        uint32_t* __restrict__ dist)
{
    const uint32_t blk = blockIdx.x, lane = threadIdx.x;
    if (blk >= nblocks) return;
    const uint32_t* __restrict__ g = hist + (uint64_t)blk * XZAMD_AD_HIST_WORDS;
    uint64_t S[XZAMD_AD_NCAND];
    uint64_t Ns = 0;
    for (uint32_t k = 0; k < XZAMD_AD_NCAND; ++k) {
        uint64_t sum = 0, cnt = 0;
        for (uint32_t v = lane; v < 256; v += 64) {
            const uint32_t c = g[k * 256 + v];
            sum += (uint64_t)c * xzamd_ad_log(c, AD_LOG);
            cnt += c;
        }
        for (int s = 32; s > 0; s >>= 1) {
            sum += __shfl_xor((unsigned long long)sum, s);
            cnt += __shfl_xor((unsigned long long)cnt, s);
        }
        if (k == 0) Ns = cnt;
        S[k] = Ns * xzamd_ad_log((uint32_t)Ns, AD_LOG) - sum;
    }
    if (lane == 0) dist[blk] = xzamd_ad_dist(xzamd_ad_rule(S, Ns));
}

// k_delta with the distance read per Block; a Block with distance 0 is copied, so that LZMA2 reads one buffer for the
// whole batch.  A thread = 16 bytes of the batch: one 16-byte load of them and one of the bytes `dist` in front when
// all of that lies inside one Block, single bytes at Block boundaries and at the end of the batch.
__global__ __launch_bounds__(256) void k_delta_blocks(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t n,
        uint32_t block_size, const uint32_t* __restrict__ dist)
{
    const uint64_t nvec = ((uint64_t)n + 15) / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nvec; t += stride) {
        const uint32_t g = (uint32_t)(t * 16);
        const uint32_t blk = g / block_size, off = g - blk * block_size;
        if (g + 16 <= n && off + 16 <= block_size) {
            const uint32_t d = dist[blk];
            uint4 c;
            __builtin_memcpy(&c, in + g, 16);
            if (d != 0 && off >= d) {
                uint4 p;
                __builtin_memcpy(&p, in + g - d, 16);
                // bytewise c - p: the borrow of every byte is kept out of its neighbour
                const uint32_t cw[4] = { c.x, c.y, c.z, c.w }, pw[4] = { p.x, p.y, p.z, p.w };
                uint32_t r[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    r[q] = ((cw[q] | 0x80808080u) - (pw[q] & 0x7F7F7F7Fu)) ^ ((cw[q] ^ ~pw[q]) & 0x80808080u);
                c = make_uint4(r[0], r[1], r[2], r[3]);
                __builtin_memcpy(out + g, &c, 16);
            } else if (d != 0) {
                for (uint32_t j = 0; j < 16; ++j)
                    out[g + j] = (uint8_t)(in[g + j] - (off + j >= d ? in[g + j - d] : (uint8_t)0));
            } else {
                __builtin_memcpy(out + g, &c, 16);
            }
        } else {
            const uint32_t e = min(n, g + 16);
            for (uint32_t q = g; q < e; ++q) {
                const uint32_t bq = q / block_size, oq = q - bq * block_size, d = dist[bq];
                out[q] = (uint8_t)(in[q] - (d != 0 && oq >= d ? in[q - d] : (uint8_t)0));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// Automatic per-Block BCJ filter (auto_bcj_rule.h, DESIGN.md 3.5 "Automatic BCJ"): per Block and candidate the hashed
// histograms of the call-site operands as they are stored and as the filter would store them, over the WHOLE Block, an
// integer entropy cost for each, and the choice.  The chosen Blocks are then filtered by the fixed-chain kernels above,
// which read kind[] (xzk_bcj_blocks).
// ------------------------------------------------------------------------------------------
constexpr uint32_t AB_TILE = 4096;        // bytes a workgroup of k_bcj_stats takes per step: 256 threads x 16
constexpr uint32_t AB_RUN = 16;           // steps per workgroup: 64 KiB of the Block for one clearing and one flush of 32 KiB of LDS

// One workgroup = AB_RUN consecutive tiles of one Block under one candidate (uniform per workgroup: no divergence on
// it); a thread = 16 bytes of a tile and the 4 bytes behind them, which the operand of an x86 site in its last bytes needs
// (one 16-byte and one 4-byte load where all 20 lie inside the Block, single bytes at the Block's end; nothing in front is
// needed, so the Block's start takes the fast path).  The two histograms live in LDS -- 32 KiB and not a byte more, so that five
// workgroups share a CU's 160 KiB -- and are added to the Block's in global memory once per workgroup; the site count goes
// there once per wavefront.  hist and nsites must be zero on entry.
__global__ __launch_bounds__(256) void k_bcj_stats(const uint8_t* __restrict__ in, uint32_t n, uint32_t block_size,
        uint32_t runs_per_block, uint32_t* __restrict__ hist, uint32_t* __restrict__ nsites)
{
    __shared__ uint32_t h[2 * XZAMD_AB_BUCKETS];
    const uint32_t per_block = runs_per_block * XZAMD_AB_NCAND;
    const uint32_t blk = blockIdx.x / per_block, r = blockIdx.x - blk * per_block;
    const uint32_t cand = r / runs_per_block, run = r - cand * runs_per_block;
    const uint64_t bs = (uint64_t)blk * block_size;
    if (bs >= n) return;
    const uint32_t blen = (uint32_t)min((uint64_t)block_size, (uint64_t)n - bs);
    if ((uint64_t)run * AB_RUN * AB_TILE >= blen) return;
    const uint8_t* __restrict__ b = in + bs;
    for (uint32_t i = threadIdx.x; i < 2 * XZAMD_AB_BUCKETS; i += 256) h[i] = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t t = run * AB_RUN; t < (run + 1) * AB_RUN; ++t) {
        const uint64_t o64 = (uint64_t)t * AB_TILE + threadIdx.x * 16u;      // of this thread's 16 bytes in the Block
        if (o64 >= blen) break;
        const uint32_t o = (uint32_t)o64;
        uint32_t x[5];                                    // bytes o .. o + 19 of the Block, zero behind its end
        if (o + 20 <= blen) {
            uint4 v;
            __builtin_memcpy(&v, b + o, 16);
            x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            __builtin_memcpy(&x[4], b + o + 16, 4);
        } else {
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t p = o + 4 * q + k;
                    if (p < blen) v |= (uint32_t)b[p] << (8 * k);
                }
                x[q] = v;
            }
        }
        if (cand == XZAMD_AB_X86) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t c = (x[j / 4] >> (8 * (j & 3))) & 255u;
                const uint32_t top = (x[(j + 4) / 4] >> (8 * (j & 3))) & 255u;
                if ((c & 0xFEu) == 0xE8u && (top == 0x00u || top == 0xFFu) && o + j + 4 < blen) {
                    const int p = j + 1;
                    const uint32_t rel = (p & 3) == 0 ? x[p / 4]
                            : (uint32_t)((((uint64_t)x[(p + 3) / 4] << 32) | x[p / 4]) >> (8 * (p & 3)));
                    atomicAdd(&h[xzamd_ab_hash(rel)], 1u);
                    atomicAdd(&h[XZAMD_AB_BUCKETS + xzamd_ab_hash(rel + o + j + 5u)], 1u);
                    ++mine;
                }
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t w = x[q], i = o + 4 * q;       // o is a multiple of 16: i mod 4 == 0 inside the Block
                if ((w >> 26) == 0x25u && i + 3 < blen) {
                    const uint32_t rel = w & 0x03FFFFFFu;
                    atomicAdd(&h[xzamd_ab_hash(rel)], 1u);
                    atomicAdd(&h[XZAMD_AB_BUCKETS + xzamd_ab_hash((rel + (i >> 2)) & 0x03FFFFFFu)], 1u);
                    ++mine;
                }
            }
        }
    }
    const uint32_t wave_sites = wave_sum_dpp(mine);      // (every lane is here: the loop above is left by break only)
    if ((threadIdx.x & 63u) == 0 && wave_sites) atomicAdd(&nsites[blk * XZAMD_AB_NCAND + cand], wave_sites);
    __syncthreads();
    uint32_t* __restrict__ g = hist + ((uint64_t)blk * XZAMD_AB_NCAND + cand) * (2 * XZAMD_AB_BUCKETS);
    for (uint32_t i = threadIdx.x; i < 2 * XZAMD_AB_BUCKETS; i += 256)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

// One wavefront per Block: the four costs S = N * L(N) - sum_v hist[v] * L(hist[v]), the rule, kind[b] = the chosen filter
// id (0: no filter).  With `dist` (the automatic delta runs too) a Block that gets a BCJ filter loses its delta distance.
__global__ __launch_bounds__(64) void k_bcj_choose(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ nsites,
        uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t* __restrict__ kind, uint32_t* __restrict__ dist)
{
    const uint32_t blk = blockIdx.x, lane = threadIdx.x;
    if (blk >= nblocks) return;
    const uint64_t bs = (uint64_t)blk * block_size;
    const uint32_t blen = bs >= n ? 0u : (uint32_t)min((uint64_t)block_size, (uint64_t)n - bs);
    uint64_t S[XZAMD_AB_NCAND][2], N[XZAMD_AB_NCAND];
    for (uint32_t k = 0; k < XZAMD_AB_NCAND; ++k) {
        N[k] = nsites[blk * XZAMD_AB_NCAND + k];
        for (uint32_t w = 0; w < 2; ++w) {
            const uint32_t* __restrict__ g = hist + (((uint64_t)blk * XZAMD_AB_NCAND + k) * 2 + w) * XZAMD_AB_BUCKETS;
            uint64_t sum = 0;
            for (uint32_t v = lane; v < XZAMD_AB_BUCKETS; v += 64) {
                const uint32_t c = g[v];
                sum += (uint64_t)c * xzamd_ad_log(c, AD_LOG);
            }
            for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor((unsigned long long)sum, s);
            S[k][w] = xzamd_ab_cost(N[k], sum, AD_LOG);
        }
    }
    if (lane == 0) {
        const uint64_t S_rel[XZAMD_AB_NCAND] = { S[0][0], S[1][0] }, S_abs[XZAMD_AB_NCAND] = { S[0][1], S[1][1] };
        const uint32_t kd = xzamd_ab_rule(S_rel, S_abs, N, blen);
        kind[blk] = kd;
        if (dist && kd) dist[blk] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// Automatic per-Block literal context (lclp_rule.h, DESIGN.md 3.5 "Automatic literal context"): the joint histogram
// H[pos & 7][prev >> 5][byte] of every Block's sample set, and per Block the costs of the candidate (lc, lp) pairs and
// the choice.
// ------------------------------------------------------------------------------------------
constexpr uint32_t LL_RUN = 8;            // sample windows per workgroup of k_lclp_stats: two per wavefront

// One workgroup = LL_RUN consecutive sample windows of one Block, one WAVEFRONT = one window at a time (a lane = 16 bytes
// in each of four passes, one 16-byte load where they lie inside the Block; the byte in front is one more load of the same
// line).  The whole joint table is privatised in LDS as 16-bit counters, two to a word: a workgroup counts at most
// LL_RUN * 4096 = 32,768 bytes, so no counter can carry into its neighbour, and 32 KiB of LDS leave room for five
// workgroups per CU.  The table is added to the Block's in global memory once per workgroup.  hist must be zero on entry.
static_assert(LL_RUN * XZAMD_AD_WINDOW < 65536u, "k_lclp_stats: 16-bit LDS counters");
__global__ __launch_bounds__(256) void k_lclp_stats(const uint8_t* __restrict__ in, uint32_t n, uint32_t block_size,
        uint32_t runs_per_block, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[XZAMD_LL_HIST_WORDS / 2];
    const uint32_t blk = blockIdx.x / runs_per_block, run = blockIdx.x - blk * runs_per_block;
    const uint64_t bs = (uint64_t)blk * block_size;
    if (bs >= n) return;
    const uint32_t blen = (uint32_t)min((uint64_t)block_size, (uint64_t)n - bs);
    const uint8_t* __restrict__ b = in + bs;
    for (uint32_t i = threadIdx.x; i < XZAMD_LL_HIST_WORDS / 2; i += 256) h[i] = 0;
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t w = run * LL_RUN + wave; w < (run + 1) * LL_RUN; w += 4) {
        const uint64_t w0 = (uint64_t)w * XZAMD_AD_PERIOD;
        if (w0 >= blen) break;
#pragma unroll
        for (uint32_t q = 0; q < XZAMD_AD_WINDOW / 1024u; ++q) {
            const uint64_t o64 = w0 + q * 1024u + lane * 16u;      // of this lane's 16 bytes in the Block
            if (o64 >= blen) continue;
            const uint32_t o = (uint32_t)o64;
            const uint32_t cnt = min(16u, blen - o);          // sampled bytes of this lane
            uint32_t x[4] = { 0, 0, 0, 0 };
            if (cnt == 16) {
                uint4 v;
                __builtin_memcpy(&v, b + o, 16);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else {
                for (uint32_t j = 0; j < cnt; ++j) x[j / 4] |= (uint32_t)b[o + j] << (8 * (j & 3));
            }
            uint32_t prev = o != 0 ? (uint32_t)b[o - 1] : 0u;
#pragma unroll
            for (uint32_t j = 0; j < 16; ++j) {
                if (j < cnt) {
                    const uint32_t cur = (x[j / 4] >> (8 * (j & 3))) & 255u;
                    const uint32_t idx = ((((o + j) & 7u) * 8u + (prev >> 5)) << 8) + cur;
                    atomicAdd(&h[idx >> 1], 1u << (16 * (idx & 1u)));
                    prev = cur;
                }
            }
        }
    }
    __syncthreads();
    uint32_t* __restrict__ g = hist + (uint64_t)blk * XZAMD_LL_HIST_WORDS;
    for (uint32_t i = threadIdx.x; i < XZAMD_LL_HIST_WORDS / 2; i += 256) {
        const uint32_t v = h[i];
        if (v & 0xFFFFu) atomicAdd(&g[2 * i], v & 0xFFFFu);
        if (v >> 16) atomicAdd(&g[2 * i + 1], v >> 16);
    }
}

// One workgroup per Block, a thread = one byte value: the sampled bytes of every (pos, prev) cell, then per candidate the
// thread's part of sum c * L(c) and of the used cells (xzamd_ll_byte over its column of the table), summed over the
// workgroup; thread 0 prices the candidates and applies the rule.  props[b] = lc | lp << 8.
__global__ __launch_bounds__(256) void k_lclp_choose(const uint32_t* __restrict__ hist, uint32_t nblocks, uint32_t lc, uint32_t lp,
        uint32_t* __restrict__ props)
{
    __shared__ uint32_t cells[XZAMD_LL_CELLS];
    __shared__ unsigned long long part_cl[4];
    __shared__ uint32_t part_used[4];
    __shared__ unsigned long long S[XZAMD_LL_MAXCAND];
    const uint32_t blk = blockIdx.x, t = threadIdx.x;
    if (blk >= nblocks) return;
    uint32_t cand[XZAMD_LL_MAXCAND];
    const uint32_t ncand = xzamd_ll_cands(lc, lp, cand);
    if (ncand == 1) {
        if (t == 0) props[blk] = cand[0];
        return;
    }
    const uint32_t* __restrict__ g = hist + (uint64_t)blk * XZAMD_LL_HIST_WORDS;
    {   // four threads per cell, 64 byte values each
        const uint32_t* __restrict__ row = g + (t >> 2) * 256u + (t & 3u) * 64u;
        uint32_t s = 0;
        for (uint32_t v = 0; v < 64; ++v) s += row[v];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if ((t & 3u) == 0) cells[t >> 2] = s;
    }
    __syncthreads();
    for (uint32_t k = 0; k < ncand; ++k) {
        uint64_t cl = 0;
        uint32_t used = 0;
        xzamd_ll_byte(g + t, 256, cand[k] & 255u, cand[k] >> 8, AD_LOG, &cl, &used);
        for (int s = 32; s > 0; s >>= 1) {
            cl += __shfl_xor((unsigned long long)cl, s);
            used += __shfl_xor(used, s);
        }
        if ((t & 63u) == 0) { part_cl[t >> 6] = cl; part_used[t >> 6] = used; }
        __syncthreads();
        if (t == 0)
            S[k] = xzamd_ll_cost(xzamd_ll_ctx(cells, cand[k] & 255u, cand[k] >> 8, AD_LOG),
                    part_cl[0] + part_cl[1] + part_cl[2] + part_cl[3], part_used[0] + part_used[1] + part_used[2] + part_used[3]);
        __syncthreads();
    }
    if (t == 0) {
        uint64_t Ns = 0, Sk[XZAMD_LL_MAXCAND];
        for (uint32_t i = 0; i < XZAMD_LL_CELLS; ++i) Ns += cells[i];
        for (uint32_t k = 0; k < ncand; ++k) Sk[k] = S[k];
        props[blk] = cand[xzamd_ll_rule(Sk, cand, ncand, Ns)];
    }
}

// ------------------------------------------------------------------------------------------
// SHA-256 Block check (check/sha256.c:120-189, FIPS 180-4): a serial hash per Block, so one THREAD per
// Block (Blocks are the parallelism; the default Check, CRC64, stays the fast path).  32 bytes per Block.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rotr32(uint32_t x, uint32_t r) { return (x >> r) | (x << (32 - r)); }

__global__ __launch_bounds__(64) void k_sha256_blocks(const uint8_t* __restrict__ in, uint32_t n, uint32_t block_size,
        uint32_t nblocks, uint8_t* __restrict__ out)
{
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
        0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
        0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
        0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
        0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2 };
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    const uint32_t bs = b * block_size;
    const uint32_t len = min(n, bs + block_size) - bs;
    uint32_t h[8] = { 0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19 };
    const uint32_t nchunks = (len + 9 + 63) / 64;               // message + 0x80 + 64-bit length
    const uint32_t nfull = len / 64;                            // chunks that are message bytes only
    // A SHA-256 is one serial chain of 64-byte compressions, so the parallelism is the Blocks: one LANE per Block (a
    // wavefront hashes 64 Blocks in lockstep).  Message words come in 16-byte loads, the schedule lives in a 16-word
    // ring in registers, the 64 rounds are unrolled.
    for (uint32_t c = 0; c < nchunks; ++c) {
        uint32_t w[16];
        if (c < nfull) {
            const uint8_t* p = in + bs + (uint64_t)c * 64;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint4 v;
                __builtin_memcpy(&v, p + 16 * q, 16);
                w[4 * q + 0] = __builtin_bswap32(v.x); w[4 * q + 1] = __builtin_bswap32(v.y);
                w[4 * q + 2] = __builtin_bswap32(v.z); w[4 * q + 3] = __builtin_bswap32(v.w);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                uint32_t v = 0;
                for (int k = 0; k < 4; ++k) {
                    const uint32_t o = c * 64 + i * 4 + k;
                    uint32_t byte = 0;
                    if (o < len) byte = in[bs + o];
                    else if (o == len) byte = 0x80;
                    else if (c + 1 == nchunks && i >= 14) {
                        const uint64_t bits = (uint64_t)len * 8;
                        byte = (uint32_t)(bits >> (8 * (7 - ((i - 14) * 4 + k)))) & 0xFF;
                    }
                    v = (v << 8) | byte;
                }
                w[i] = v;
            }
        }
        uint32_t a = h[0], bb = h[1], cc = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            if (i >= 16) {
                const uint32_t w15 = w[(i - 15) & 15], w2 = w[(i - 2) & 15];
                const uint32_t s0 = rotr32(w15, 7) ^ rotr32(w15, 18) ^ (w15 >> 3);
                const uint32_t s1 = rotr32(w2, 17) ^ rotr32(w2, 19) ^ (w2 >> 10);
                w[i & 15] = w[i & 15] + s0 + w[(i - 7) & 15] + s1;
            }
            const uint32_t S1 = rotr32(e, 6) ^ rotr32(e, 11) ^ rotr32(e, 25);
            const uint32_t ch = (e & f) ^ (~e & g);
            const uint32_t t1 = hh + S1 + ch + K[i] + w[i & 15];
            const uint32_t S0 = rotr32(a, 2) ^ rotr32(a, 13) ^ rotr32(a, 22);
            const uint32_t mj = (a & bb) ^ (a & cc) ^ (bb & cc);
            const uint32_t t2 = S0 + mj;
            hh = g; g = f; f = e; e = d + t1; d = cc; cc = bb; bb = a; a = t1 + t2;
        }
        h[0] += a; h[1] += bb; h[2] += cc; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    for (int i = 0; i < 8; ++i) {
        out[b * 32 + i * 4 + 0] = (uint8_t)(h[i] >> 24);
        out[b * 32 + i * 4 + 1] = (uint8_t)(h[i] >> 16);
        out[b * 32 + i * 4 + 2] = (uint8_t)(h[i] >> 8);
        out[b * 32 + i * 4 + 3] = (uint8_t)h[i];
    }
}

// ------------------------------------------------------------------------------------------
// CRC64 (check/crc64_fast.c; ECMA-182 reflected, poly 0xC96C5795D7870F42)
// ------------------------------------------------------------------------------------------
// Both Block checks of the device path share the code: T = uint64_t is CRC64 (ECMA-182 reflected,
// check/crc64_fast.c), T = uint32_t is CRC32 (IEEE reflected, check/crc32_fast.c).
template <typename T> struct CrcP;
template <> struct CrcP<uint64_t> { static constexpr uint64_t POLY = 0xC96C5795D7870F42ull; static constexpr uint64_t TOP = 1ull << 63; };
template <> struct CrcP<uint32_t> { static constexpr uint32_t POLY = 0xEDB88320u; static constexpr uint32_t TOP = 1u << 31; };

// product of two residues in the reflected representation (MSB = x^0)
template <typename T>
__device__ __forceinline__ T gf_mul(T a, T b)
{
    T r = 0;
    for (int i = 0; i < (int)(8 * sizeof(T)); ++i) {
        if (a & CrcP<T>::TOP) r ^= b;
        a <<= 1;
        b = (T)((b >> 1) ^ ((b & 1) ? CrcP<T>::POLY : (T)0));
    }
    return r;
}

template <typename T>
__device__ __forceinline__ T gf_xpow8(uint64_t nbytes)
{
    T base = (T)(CrcP<T>::TOP >> 8);     // x^8
    T acc = CrcP<T>::TOP;                // 1
    while (nbytes) {
        if (nbytes & 1) acc = gf_mul<T>(acc, base);
        base = gf_mul<T>(base, base);
        nbytes >>= 1;
    }
    return acc;
}

// Standard CRC (init ~0, final ~) of each strip of `strip` bytes; strips never straddle Blocks.
template <typename T>
__global__ __launch_bounds__(256) void k_crc_strips(const uint8_t* __restrict__ in, uint32_t n,
        uint32_t block_size, uint32_t strip, uint32_t strips_per_block, uint32_t nstrips,
        T* __restrict__ out)
{
    __shared__ T tab[256];
    {
        T r = (T)threadIdx.x;
        for (int k = 0; k < 8; ++k) r = (T)((r >> 1) ^ ((r & 1) ? CrcP<T>::POLY : (T)0));
        tab[threadIdx.x] = r;
    }
    __syncthreads();
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstrips) return;
    const uint32_t b = s / strips_per_block;
    const uint32_t bstart = b * block_size;
    const uint32_t bend = min(n, bstart + block_size);
    const uint32_t beg = bstart + (s - b * strips_per_block) * strip;
    T crc = (T)~(T)0;
    if (beg < bend) {
        const uint32_t end = min(bend, beg + strip);
        for (uint32_t i = beg; i < end; ++i)
            crc = (T)(tab[(crc ^ in[i]) & 0xFF] ^ (crc >> 8));
    }
    out[s] = (T)~crc;
}

// One wave per Block: fold the strip CRCs left to right: crc(A||B) = crc(A)*x^(8|B|) ^ crc(B).
// The Block's check is written as a uint64_t (CRC32 zero-extended).
template <typename T>
__global__ __launch_bounds__(64) void k_crc_fold(const T* __restrict__ strips, uint32_t n,
        uint32_t block_size, uint32_t strip, uint32_t strips_per_block, uint64_t* __restrict__ block_crc)
{
    const uint32_t b = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t bstart = b * block_size;
    const uint32_t bend = min(n, bstart + block_size);
    const uint32_t blen = bend - bstart;
    const uint32_t ns = (blen + strip - 1) / strip;          // strips actually used
    const uint32_t per = (ns + 63) / 64;
    const uint32_t s0 = min(ns, lane * per), s1 = min(ns, s0 + per);
    const T xs = gf_xpow8<T>(strip);
    // lane-local fold over its contiguous strips
    T acc = 0;              // crc of the empty string is 0 and is the identity of the fold
    uint64_t bytes = 0;
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t len = min(strip, blen - s * strip);
        const T c = strips[(uint64_t)b * strips_per_block + s];
        acc = (T)(gf_mul<T>(acc, len == strip ? xs : gf_xpow8<T>(len)) ^ c);
        bytes += len;
    }
    // sequential combine across lanes (64 steps, once per Block)
    T total = 0;
    for (uint32_t l = 0; l < 64; ++l) {
        const T cl = (T)__shfl((unsigned long long)acc, l);
        const uint64_t bl = __shfl((unsigned long long)bytes, l);
        if (bl) total = (T)(gf_mul<T>(total, gf_xpow8<T>(bl)) ^ cl);
    }
    if (lane == 0) block_crc[b] = (uint64_t)total;
}

} // namespace

extern "C" {

int xzk_x86_bcj(const uint8_t* d_in, uint8_t* d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    int e = (int)hipMemcpyAsync(d_out, d_in, n, hipMemcpyDeviceToDevice, st);
    if (e) return e;
    const uint32_t cpb = (block_size + BCJ_CHUNK - 1) / BCJ_CHUNK;
    const uint64_t nch = (uint64_t)cpb * nblocks;
    if (nch == 0 || nch > 0xFFFFFFFFull) return nch ? (int)hipErrorInvalidValue : 0;
    hipLaunchKernelGGL(k_x86_bcj, dim3((uint32_t)((nch + 255) / 256)), dim3(256), 0, st, d_in, d_out, n, block_size, cpb,
            (uint32_t)nch, (const uint32_t*)nullptr);
    return (int)hipGetLastError();
}

// prefilter kind: 0x0A = ARM64 BCJ, 0x0B = RISC-V BCJ, 5 / 6 / 7 / 8 / 9 = PowerPC / IA-64 / ARM / ARM-Thumb / SPARC BCJ, 3 = delta (dist 1..256):
// d_out = filtered copy of d_in
int xzk_prefilter(const uint8_t* d_in, uint8_t* d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t kind, uint32_t dist,
        void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (n == 0) return 0;
    if (kind == 0x0A) {
        int e = (int)hipMemcpyAsync(d_out, d_in, n, hipMemcpyDeviceToDevice, st);
        if (e) return e;
        hipLaunchKernelGGL(k_arm64_bcj, dim3(grid_for((uint64_t)n / 4 + 1, 256, 65536)), dim3(256), 0, st, d_in, d_out, n, block_size, nblocks,
                (const uint32_t*)nullptr);
    } else if (kind == 0x0B) {
        int e = (int)hipMemcpyAsync(d_out, d_in, n, hipMemcpyDeviceToDevice, st);
        if (e) return e;
        const uint32_t cpb = (block_size + BCJ_CHUNK - 1) / BCJ_CHUNK;
        const uint64_t nch = (uint64_t)cpb * nblocks;
        if (nch > 0xFFFFFFFFull) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(k_riscv_bcj, dim3((uint32_t)((nch + 255) / 256)), dim3(256), 0, st, d_in, d_out, n, block_size, cpb,
                (uint32_t)nch);
    } else if (kind >= 5 && kind <= 9) {
        int e = (int)hipMemcpyAsync(d_out, d_in, n, hipMemcpyDeviceToDevice, st);
        if (e) return e;
        hipLaunchKernelGGL(k_bcj_simple, dim3(grid_for((uint64_t)n / 2 + 1, 256, 65536)), dim3(256), 0, st, d_in, d_out, n, block_size,
                nblocks, kind);
    } else if (kind == 3) {
        hipLaunchKernelGGL(k_delta, dim3(grid_for(n, 256, 65536)), dim3(256), 0, st, d_in, d_out, n, block_size, dist);
    } else {
        return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

int xzk_delta_stats(const uint8_t* d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t* d_hist, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (nblocks == 0 || n == 0) return 0;
    if (block_size == 0 || (uint64_t)nblocks * block_size < n) return (int)hipErrorInvalidValue;
    int e = (int)hipMemsetAsync(d_hist, 0, (uint64_t)nblocks * XZAMD_AD_HIST_WORDS * 4, st);
    if (e) return e;
    const uint32_t wpb = (block_size + XZAMD_AD_PERIOD - 1) / XZAMD_AD_PERIOD;     // sample windows per full Block
    const uint32_t rpb = (wpb + AD_RUN - 1) / AD_RUN;
    const uint64_t grid = (uint64_t)rpb * nblocks;
    if (grid > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_delta_stats, dim3((uint32_t)grid), dim3(256), 0, st, d_in, n, block_size, rpb, d_hist);
    return (int)hipGetLastError();
}

int xzk_delta_choose(const uint32_t* d_hist, uint32_t nblocks, uint32_t* d_dist, void* stream_)
{
    if (nblocks == 0) return 0;
    hipLaunchKernelGGL(k_delta_choose, dim3(nblocks), dim3(64), 0, (hipStream_t)stream_, d_hist, nblocks, d_dist);
    return (int)hipGetLastError();
}

int xzk_delta_blocks(const uint8_t* d_in, uint8_t* d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, const uint32_t* d_dist,
        void* stream_)
{
    if (n == 0) return 0;
    if (block_size == 0 || (uint64_t)nblocks * block_size < n || n > 0xFFFFFFE0u) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_delta_blocks, dim3(grid_for(((uint64_t)n + 15) / 16, 256, 65536)), dim3(256), 0, (hipStream_t)stream_, d_in, d_out,
            n, block_size, d_dist);
    return (int)hipGetLastError();
}

int xzk_bcj_stats(const uint8_t* d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t* d_hist, uint32_t* d_nsites,
        void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (nblocks == 0 || n == 0) return 0;
    if (block_size == 0 || (uint64_t)nblocks * block_size < n) return (int)hipErrorInvalidValue;
    int e = (int)hipMemsetAsync(d_hist, 0, (uint64_t)nblocks * XZAMD_AB_HIST_WORDS * 4, st);
    if (!e) e = (int)hipMemsetAsync(d_nsites, 0, (uint64_t)nblocks * XZAMD_AB_NCAND * 4, st);
    if (e) return e;
    const uint32_t rpb = (uint32_t)(((uint64_t)block_size + AB_RUN * AB_TILE - 1) / (AB_RUN * AB_TILE));
    const uint64_t grid = (uint64_t)rpb * XZAMD_AB_NCAND * nblocks;
    if (grid > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bcj_stats, dim3((uint32_t)grid), dim3(256), 0, st, d_in, n, block_size, rpb, d_hist, d_nsites);
    return (int)hipGetLastError();
}

int xzk_bcj_choose(const uint32_t* d_hist, const uint32_t* d_nsites, uint32_t n, uint32_t block_size, uint32_t nblocks,
        uint32_t* d_kind, uint32_t* d_dist, void* stream_)
{
    if (nblocks == 0) return 0;
    if (block_size == 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bcj_choose, dim3(nblocks), dim3(64), 0, (hipStream_t)stream_, d_hist, d_nsites, n, block_size, nblocks,
            d_kind, d_dist);
    return (int)hipGetLastError();
}

// The fixed-chain encoders with kind[] read per Block: x86 over the Blocks of kind 4, ARM64 over those of kind 0x0A, the
// rest left as the copy.
int xzk_bcj_blocks(const uint8_t* d_in, uint8_t* d_out, uint32_t n, uint32_t block_size, uint32_t nblocks, const uint32_t* d_kind,
        int copy, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (n == 0 || nblocks == 0) return 0;
    if (block_size == 0 || (uint64_t)nblocks * block_size < n || !d_kind) return (int)hipErrorInvalidValue;
    if (copy) {
        int e = (int)hipMemcpyAsync(d_out, d_in, n, hipMemcpyDeviceToDevice, st);
        if (e) return e;
    }
    const uint32_t cpb = (block_size + BCJ_CHUNK - 1) / BCJ_CHUNK;
    const uint64_t nch = (uint64_t)cpb * nblocks;
    if (nch > 0xFFFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_x86_bcj, dim3((uint32_t)((nch + 255) / 256)), dim3(256), 0, st, d_in, d_out, n, block_size, cpb,
            (uint32_t)nch, d_kind);
    hipLaunchKernelGGL(k_arm64_bcj, dim3(grid_for((uint64_t)n / 4 + 1, 256, 65536)), dim3(256), 0, st, d_in, d_out, n, block_size, nblocks,
            d_kind);
    return (int)hipGetLastError();
}

int xzk_lclp_stats(const uint8_t* d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint32_t* d_hist, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (nblocks == 0) return 0;
    if (block_size == 0 || (uint64_t)nblocks * block_size < n) return (int)hipErrorInvalidValue;
    int e = (int)hipMemsetAsync(d_hist, 0, (uint64_t)nblocks * XZAMD_LL_HIST_WORDS * 4, st);
    if (e || n == 0) return e;
    const uint32_t wpb = (block_size + XZAMD_AD_PERIOD - 1) / XZAMD_AD_PERIOD;     // sample windows per full Block
    const uint32_t rpb = (wpb + LL_RUN - 1) / LL_RUN;
    const uint64_t grid = (uint64_t)rpb * nblocks;
    if (grid > 0x7FFFFFFFull) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lclp_stats, dim3((uint32_t)grid), dim3(256), 0, st, d_in, n, block_size, rpb, d_hist);
    return (int)hipGetLastError();
}

int xzk_lclp_choose(const uint32_t* d_hist, uint32_t nblocks, uint32_t lc, uint32_t lp, uint32_t* d_props, void* stream_)
{
    if (nblocks == 0) return 0;
    if (lc > 4 || lp > 4 || lc + lp > 4) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lclp_choose, dim3(nblocks), dim3(256), 0, (hipStream_t)stream_, d_hist, nblocks, lc, lp, d_props);
    return (int)hipGetLastError();
}

int xzk_lclp_read(const uint32_t* d_hist, const uint32_t* d_props, uint32_t nblocks, uint32_t* h_hist, uint32_t* h_props, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    int e = 0;
    if (nblocks == 0) return 0;
    if (h_hist) e = (int)hipMemcpyAsync(h_hist, d_hist, (uint64_t)nblocks * XZAMD_LL_HIST_WORDS * 4, hipMemcpyDeviceToHost, st);
    if (!e && h_props) e = (int)hipMemcpyAsync(h_props, d_props, (uint64_t)nblocks * 4, hipMemcpyDeviceToHost, st);
    if (!e) e = (int)hipStreamSynchronize(st);
    return e;
}

int xzk_sha256_blocks(const uint8_t* d_in, uint32_t n, uint32_t block_size, uint32_t nblocks, uint8_t* d_out32, void* stream_)
{
    if (nblocks == 0) return 0;
    hipLaunchKernelGGL(k_sha256_blocks, dim3((nblocks + 63) / 64), dim3(64), 0, (hipStream_t)stream_, d_in, n, block_size, nblocks, d_out32);
    return (int)hipGetLastError();
}

int xzk_crc_blocks(const uint8_t* d_in, uint32_t n, uint32_t block_size, uint32_t nblocks,
        uint32_t strip, int crc32, uint64_t* d_strip_crc, uint64_t* d_block_crc, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    const uint32_t spb = (block_size + strip - 1) / strip;
    const uint32_t ns = spb * nblocks;
    if (crc32) {
        uint32_t* strips = reinterpret_cast<uint32_t*>(d_strip_crc);
        hipLaunchKernelGGL((k_crc_strips<uint32_t>), dim3((ns + 255) / 256), dim3(256), 0, st, d_in, n, block_size, strip,
                spb, ns, strips);
        hipLaunchKernelGGL((k_crc_fold<uint32_t>), dim3(nblocks), dim3(64), 0, st, strips, n, block_size, strip, spb,
                d_block_crc);
    } else {
        hipLaunchKernelGGL((k_crc_strips<uint64_t>), dim3((ns + 255) / 256), dim3(256), 0, st, d_in, n, block_size, strip,
                spb, ns, d_strip_crc);
        hipLaunchKernelGGL((k_crc_fold<uint64_t>), dim3(nblocks), dim3(64), 0, st, d_strip_crc, n, block_size, strip, spb,
                d_block_crc);
    }
    return (int)hipGetLastError();
}

} // extern "C"
