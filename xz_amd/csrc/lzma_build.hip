// lzma_build.hip -- the match-finder structure build: hash-chain heads and the suffix order of every Block (stage
// table and design: lzma_kernels.hip).  The only unit that includes rocprim: see sort_pairs, max_scan, sum_scan.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <stdint.h>
#include "kernels_api.h"
#include "kernels_internal.h"
#include "wave.h"

namespace {

// CRC32 table[0] entry for one byte (lz_encoder_hash.h:31-39 uses lzma_crc32_table[0]).
__device__ __forceinline__ uint32_t crc_t0(uint32_t b)
{
    uint32_t r = b;
#pragma unroll
    for (int k = 0; k < 8; ++k) r = (r >> 1) ^ ((r & 1) ? 0xEDB88320u : 0u);
    return r;
}

// ------------------------------------------------------------------------------------------
// Match-finder structure build
// ------------------------------------------------------------------------------------------

// One thread per input byte: one of the hash keys of lz_encoder_hash.h:55-75 (which = 2: hash2,
// 3: hash3 of HC4, 0: the main chain hash), prefixed with the Block number so one sort serves
// every Block of the batch.  Positions with fewer than hash_bytes left in their Block are never
// inserted by the reference (lz_encoder_mf.c:190-201 "pending"): they get the sentinel bucket
// `nblocks`.  vals = iota (the position itself).
__global__ __launch_bounds__(256) void k_hash_keys(const uint8_t* __restrict__ in, uint32_t n,
        uint32_t block_size, uint32_t nblocks, uint32_t hash_bytes, uint32_t hash_mask, uint32_t hash_bits,
        uint32_t which, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    __shared__ uint32_t T[256];
    T[threadIdx.x] = crc_t0(threadIdx.x);
    __syncthreads();
    const uint32_t kbits = which == 2 ? 10u : (which == 3 ? 16u : hash_bits);
    const uint32_t need = hash_bytes;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint32_t b = g / block_size;
        const uint32_t bend = min(n, (b + 1) * block_size);   // n < 2^31, no overflow
        const uint32_t avail = bend - g;
        uint32_t key = nblocks << kbits;
        if (avail >= need) {
            const uint32_t c0 = in[g], c1 = in[g + 1], c2 = in[g + 2];
            const uint32_t temp = T[c0] ^ c1;
            uint32_t h;
            if (which == 2) h = temp & 0x3FF;
            else if (which == 3) h = (temp ^ (c2 << 8)) & 0xFFFF;
            else if (hash_bytes == 3) h = (temp ^ (c2 << 8)) & hash_mask;
            else h = (temp ^ (c2 << 8) ^ (T[in[g + 3]] << 5)) & hash_mask;
            key = (b << kbits) | h;
        }
        keys[g] = key;
        vals[g] = g;
    }
}

// After the stable sort by key_main: publish the bucket order.
//   sorted_pos[i] = position | (first-of-bucket << 31)      rank[position] = i
__global__ __launch_bounds__(256) void k_link_main(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
        uint32_t n, uint32_t* __restrict__ sorted_pos, uint32_t* __restrict__ rank)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t p = vals[i];
        const uint32_t first = (i == 0 || keys[i - 1] != keys[i]) ? 0x80000000u : 0u;
        sorted_pos[i] = p | first;
        rank[p] = i;
    }
}

// After the stable sort by key2 / key3 / key4: prev[position] = distance to the previous position of the same
// bucket (the value the reference's hash head table holds when `position` is reached, expressed as delta),
// 0 = none.
// hash2 needs no sort: its table has 1024 entries per Block, so the "previous position with the same hash" is
// found the way the reference does it -- a head table walked in text order -- with the Block cut into segments of
// H2_SEG positions, one wavefront each:
//   k_h2_last   last inserted position (+1) of every hash value inside the segment      (LDS table, ds_max)
//   k_h2_scan   per Block: exclusive running maximum of those tables over its segments   (the carry-in heads)
//   k_h2_prev   the segment again, 64 positions a step: a lane's predecessor is the highest lower lane of the
//               step with the same hash (ten ballots give every lane its set of peers), else the table entry;
//               the last lane of each peer set then updates the table.
// Positions with fewer than hash_bytes left in their Block are not inserted and get 0 (they are never looked up).
constexpr uint32_t H2_SEG = 65536;

__device__ __forceinline__ uint32_t h2_of(const uint8_t* __restrict__ in, const uint32_t* T, uint32_t p)
{
    return (T[in[p]] ^ in[p + 1]) & 0x3FFu;
}

__global__ __launch_bounds__(64) void k_h2_last(const uint8_t* __restrict__ in, uint32_t n, uint32_t block_size,
        uint32_t segs_per_block, uint32_t hash_bytes, uint32_t* __restrict__ seg_tab)
{
    __shared__ uint32_t T[256];
    __shared__ uint32_t tab[1024];
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < 256; i += 64) T[i] = crc_t0(i);
    for (uint32_t i = lane; i < 1024; i += 64) tab[i] = 0;
    const uint32_t b = blockIdx.x / segs_per_block, sg = blockIdx.x - b * segs_per_block;
    const uint32_t bs = b * block_size;
    const uint32_t bend = min(n, bs + block_size);
    const uint32_t s0 = bs + sg * H2_SEG;
    const uint32_t s1 = min(bend, s0 + H2_SEG);
    wave_sync();
    for (uint32_t x = s0 + lane; x < s1; x += 64)
        if (bend - x >= hash_bytes) atomicMax(&tab[h2_of(in, T, x)], x + 1);
    wave_sync();
    uint32_t* out = seg_tab + (uint64_t)blockIdx.x * 1024;
    for (uint32_t i = lane; i < 1024; i += 64) out[i] = tab[i];
}

__global__ __launch_bounds__(256) void k_h2_scan(uint32_t* __restrict__ seg_tab, uint32_t segs_per_block)
{
    // thread = (Block, hash value): exclusive running maximum along the Block's segments
    const uint32_t b = blockIdx.x >> 2, h = ((blockIdx.x & 3) << 8) | threadIdx.x;
    uint32_t* t = seg_tab + (uint64_t)b * segs_per_block * 1024 + h;
    uint32_t run = 0;
    for (uint32_t s = 0; s < segs_per_block; ++s) {
        const uint32_t v = t[(uint64_t)s * 1024];
        t[(uint64_t)s * 1024] = run;
        run = max(run, v);
    }
}

__global__ __launch_bounds__(64) void k_h2_prev(const uint8_t* __restrict__ in, uint32_t n, uint32_t block_size,
        uint32_t segs_per_block, uint32_t hash_bytes, const uint32_t* __restrict__ seg_tab, uint32_t* __restrict__ prev2)
{
    __shared__ uint32_t T[256];
    __shared__ uint32_t tab[1024];
    const uint32_t lane = threadIdx.x;
    const uint32_t* carry = seg_tab + (uint64_t)blockIdx.x * 1024;
    for (uint32_t i = lane; i < 256; i += 64) T[i] = crc_t0(i);
    for (uint32_t i = lane; i < 1024; i += 64) tab[i] = carry[i];
    const uint32_t b = blockIdx.x / segs_per_block, sg = blockIdx.x - b * segs_per_block;
    const uint32_t bs = b * block_size;
    const uint32_t bend = min(n, bs + block_size);
    const uint32_t s0 = bs + sg * H2_SEG;
    const uint32_t s1 = min(bend, s0 + H2_SEG);
    const uint64_t below = (1ull << lane) - 1;
    wave_sync();
    for (uint32_t x0 = s0; x0 < s1; x0 += 64) {
        const uint32_t x = x0 + lane;
        const bool ins = x < s1 && bend - x >= hash_bytes;
        const uint32_t h = ins ? h2_of(in, T, x) : 0u;
        uint64_t peers = __builtin_amdgcn_ballot_w64(ins);
#pragma unroll
        for (uint32_t k = 0; k < 10; ++k) {
            const uint64_t m = __builtin_amdgcn_ballot_w64(((h >> k) & 1u) != 0);
            peers &= ((h >> k) & 1u) ? m : ~m;
        }
        const uint32_t head = tab[h];                       // head before this step
        const uint64_t lower = peers & below;
        uint32_t d = 0;
        if (lower) d = lane - (63u - (uint32_t)__builtin_clzll(lower));
        else if (head) d = x + 1 - head;
        if (x < s1) prev2[x] = ins ? d : 0u;
        wave_sync();
        if (ins && (peers >> lane) == 1ull) tab[h] = x + 1;   // last lane of its peer set
        wave_sync();
    }
}

// The same distances, written in sorted order (d[i] belongs to position vals[i]).  A scattered 4-byte store
// costs a whole sector and 1.4 G of them run at ~30 G/s; sorting the (position, distance) pairs back by
// position (invert_perm below: two streaming radix passes and an LDS step) is more than twice as fast.
__global__ __launch_bounds__(256) void k_link_prev_seq(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
        uint32_t n, uint32_t* __restrict__ d)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        d[i] = (i > 0 && keys[i - 1] == keys[i]) ? vals[i] - vals[i - 1] : 0u;
}

__global__ __launch_bounds__(256) void k_iota(uint32_t* __restrict__ v, uint32_t n)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) v[i] = i;
}

// Last step of an inversion (invert_perm below).  The (position, value) pairs arrive sorted by position >> 15;
// the positions are a permutation of 0..n-1, so bucket b is exactly the pairs of positions [b << 15, (b + 1) << 15)
// and sits in exactly those slots.  One workgroup per bucket places the values in LDS by the low 15 bits and
// writes the 128 KiB out linearly: the last 15 key bits cost one read and one coalesced write instead of two
// radix passes.  In place is fine (a bucket reads and writes the same slots, reads first).
constexpr uint32_t INV_LOW = 15;
__global__ __launch_bounds__(1024) void k_inv_low_u32(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
        uint32_t n, uint32_t* __restrict__ out)
{
    __shared__ uint32_t lds_inv[1u << INV_LOW];             // 128 KiB of the 160 KiB a CU has
    const uint32_t base = blockIdx.x << INV_LOW;
    const uint32_t cnt = min(n - base, 1u << INV_LOW);
    for (uint32_t i = threadIdx.x; i < cnt; i += 1024) lds_inv[keys[base + i] & ((1u << INV_LOW) - 1)] = vals[base + i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += 1024) out[base + i] = lds_inv[i];
}

// 64-bit values: the two halves go to two arrays (out_lo, out_hi), one LDS round each
__global__ __launch_bounds__(1024) void k_inv_low_u64(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals,
        uint32_t n, uint32_t* __restrict__ out_lo, uint32_t* __restrict__ out_hi)
{
    __shared__ uint32_t lds_inv[1u << INV_LOW];             // 128 KiB of the 160 KiB a CU has
    const uint32_t base = blockIdx.x << INV_LOW;
    const uint32_t cnt = min(n - base, 1u << INV_LOW);
    for (uint32_t i = threadIdx.x; i < cnt; i += 1024) lds_inv[keys[base + i] & ((1u << INV_LOW) - 1)] = (uint32_t)vals[base + i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += 1024) out_lo[base + i] = lds_inv[i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += 1024) lds_inv[keys[base + i] & ((1u << INV_LOW) - 1)] = (uint32_t)(vals[base + i] >> 32);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += 1024) out_hi[base + i] = lds_inv[i];
}

// ------------------------------------------------------------------------------------------
// Suffix order of every Block by its first 32 bytes (oracle: build_sa) -- the structure behind the
// suffix-neighbourhood finder.  Order inside a Block: four 8-byte chunks compared as big-endian
// numbers (bytes past the Block end read as zero, a chunk that starts past the end sorts lowest),
// ties by position.  Built by stable LSD radix sorts (rocprim onesweep, HBM-bound):
//   round 0   sort (chunk(p), p), then stably by Block number (so the slots of a Block are exactly
//             its positions' range);
//   round h   h = 8, 16: rank[p] = 1 + first slot of p's group of equal keys; sort by
//             (rank[p], rank[p + h]) (0 = past the Block end): doubles the compared prefix.
// Group starts come from a max-scan over "slot if the key differs from its left neighbour".
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sa_chunk_keys(const uint8_t* __restrict__ in, uint32_t n, uint32_t block_size,
        uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint32_t b = g / block_size;
        const uint32_t bend = min(n, (b + 1) * block_size);
        const uint32_t avail = bend - g;
        uint64_t v = 0;
        if (avail >= 8) {
            uint64_t t;
            __builtin_memcpy(&t, in + g, 8);
            v = __builtin_bswap64(t);
        } else {
            for (uint32_t i = 0; i < avail; ++i) v |= (uint64_t)in[g + i] << (56 - 8 * i);
        }
        keys[g] = v;
        vals[g] = g;
    }
}

// grp[i] = i where the 64-bit key differs from its left neighbour (or, with block_size != 0, where a Block
// starts: the slots of a Block are its positions' range), else 0 (input of the max-scan)
__global__ __launch_bounds__(256) void k_sa_flags64(const uint64_t* __restrict__ keys, uint32_t n, uint32_t block_size,
        uint32_t* __restrict__ grp)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const bool first = i != 0 && (keys[i] != keys[i - 1] || (block_size != 0 && i % block_size == 0));
        grp[i] = first ? i : 0u;
    }
}

// round 0, second step: pack (position, chunk group) as the value, Block number as the key
__global__ __launch_bounds__(256) void k_sa_block_keys(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ grp,
        uint32_t n, uint32_t block_size, uint32_t* __restrict__ bkeys, uint64_t* __restrict__ bvals)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t p = pos[i];
        bkeys[i] = p / block_size;
        bvals[i] = (uint64_t)p | ((uint64_t)grp[i] << 32);
    }
}

// after the Block sort: positions out, group flags from (Block, chunk group)
__global__ __launch_bounds__(256) void k_sa_block_unpack(const uint32_t* __restrict__ bkeys, const uint64_t* __restrict__ bvals,
        uint32_t n, uint32_t* __restrict__ pos, uint32_t* __restrict__ grp)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t v = bvals[i];
        pos[i] = (uint32_t)v;
        const bool first = i == 0 || bkeys[i] != bkeys[i - 1] || (uint32_t)(bvals[i - 1] >> 32) != (uint32_t)(v >> 32);
        grp[i] = (first && i != 0) ? i : 0u;
    }
}

// Slot order: rk[i] = (group start + 1, distance to the left neighbour inside the group or 0) of position pos[i].
// The second word is a by-product of the sort round: inside a group of equal keys positions ascend, so the left
// neighbour of a group member is the nearest earlier position with the same 8 (round 0) / 16 (round 1) bytes.
// The pairs are then brought to position order (invert_perm): two arrays indexed by position.
__global__ __launch_bounds__(256) void k_sa_rank_seq(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ grp,
        uint32_t n, uint2* __restrict__ rk)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t g = grp[i];
        rk[i] = make_uint2(g + 1, g != i ? pos[i] - pos[i - 1] : 0u);
    }
}

// the same for the rounds that only want the rank (sa_depth > 32)
__global__ __launch_bounds__(256) void k_sa_rank_only_seq(const uint32_t* __restrict__ grp, uint32_t n, uint32_t* __restrict__ rk)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) rk[i] = grp[i] + 1;
}

// ---- rank doubling on the unresolved slots only -------------------------------------------------------------
// After the 16-byte round most positions of ordinary data are alone in their group (text: 88 %, after 32 bytes
// 99.95 %): their slot is final.  A round then only has to order the slots that still share a group with another one:
//   k_sa_unres     u[i] = 1 when slot i lies in a group of >= 2 slots            (exclusive scan -> compact index)
//   k_sa_compact   (key, position, slot) of the unresolved slots, in slot order; key = (rank, rank of p + h) as
//                  k_sa_pair_keys_pos makes it
//   radix sort of those m elements (stable: equal keys keep ascending positions, as in the full round)
//   k_sa_newgrp    group starts of the sorted elements (max-scan over "slot where the key changes")
//   k_sa_writeback the j-th sorted element goes to the j-th unresolved slot (the groups are contiguous slot ranges in
//                  ascending order, so the sorted sequence enumerates them in place); position, group start and the
//                  by-position rank of the moved elements are updated
__global__ __launch_bounds__(256) void k_sa_unres(const uint32_t* __restrict__ grp, uint32_t n, uint32_t* __restrict__ u)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        u[i] = (grp[i] != i || (i + 1 < n && grp[i + 1] == i)) ? 1u : 0u;
}

__global__ void k_sa_count(const uint32_t* __restrict__ idx, const uint32_t* __restrict__ grp, uint32_t n, uint32_t* __restrict__ count)
{
    if (blockIdx.x == 0 && threadIdx.x == 0)
        *count = idx[n - 1] + ((grp[n - 1] != n - 1) ? 1u : 0u);      // the last slot has no right neighbour
}

__global__ __launch_bounds__(256) void k_sa_compact(const uint32_t* __restrict__ pos, const uint32_t* __restrict__ grp,
        const uint32_t* __restrict__ idx, const uint32_t* __restrict__ rank, uint32_t n, uint32_t block_size, uint32_t h,
        uint32_t sbits, uint64_t* __restrict__ ckey, uint32_t* __restrict__ cval, uint32_t* __restrict__ cslot)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t g = grp[i];
        if (!(g != i || (i + 1 < n && grp[i + 1] == i))) continue;
        const uint32_t j = idx[i];
        const uint32_t p = pos[i];
        const uint32_t bs = (p / block_size) * block_size;
        const uint32_t bend = min(n, bs + block_size);
        const uint32_t second = p + h < bend ? rank[p + h] - bs : 0u;
        ckey[j] = ((uint64_t)(g + 1) << sbits) | second;
        cval[j] = p;
        cslot[j] = i;
    }
}

__global__ __launch_bounds__(256) void k_sa_newgrp(const uint64_t* __restrict__ ckey, const uint32_t* __restrict__ cslot,
        uint32_t m, uint32_t* __restrict__ gs)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride)
        gs[j] = (j == 0 || ckey[j] != ckey[j - 1]) ? cslot[j] : 0u;
}

__global__ __launch_bounds__(256) void k_sa_writeback(const uint32_t* __restrict__ cval, const uint32_t* __restrict__ cslot,
        const uint32_t* __restrict__ gs, uint32_t m, uint32_t* __restrict__ pos, uint32_t* __restrict__ grp,
        uint32_t* __restrict__ rank)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const uint32_t sl = cslot[j], p = cval[j], g = gs[j];
        pos[sl] = p;
        grp[sl] = g;
        rank[p] = g + 1;
    }
}

// By-product of a sorted round: inside a run of equal keys the positions ascend, so the left neighbour of a member is the
// nearest earlier position of its group; d[position] = distance to it (0: first of its group).  A scatter of m elements.
__global__ __launch_bounds__(256) void k_sa_prev_scatter(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
        uint32_t m, uint32_t* __restrict__ d)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += stride) {
        const uint32_t p = val[j];
        d[p] = (j > 0 && key[j] == key[j - 1]) ? p - val[j - 1] : 0u;
    }
}

// doubling key of every position, in position order: (rank[p], rank[p + h]) with 0 for a second half that
// starts past the Block end; vals = iota.  The second rank is taken relative to the Block (sbits = bits of
// block_size + 1), so the key is 31 + sbits bits wide instead of 62: one radix pass less for Blocks up to 32 MiB.  (The radix sort is stable and the members of a group ascend by
// position in slot order too, so feeding it in position order gives the same result as slot order -- without
// the random gather of rank[p + h].)
__global__ __launch_bounds__(256) void k_sa_pair_keys_pos(const uint32_t* __restrict__ rank, uint32_t n, uint32_t block_size,
        uint32_t h, uint32_t sbits, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint32_t b = p / block_size;
        const uint32_t bs = b * block_size;
        const uint32_t bend = min(n, bs + block_size);
        // the second half lies in the same Block, whose slots are [bs, bend): relative rank 1..block_size
        const uint32_t second = p + h < bend ? rank[p + h] - bs : 0u;
        keys[p] = ((uint64_t)rank[p] << sbits) | second;
        vals[p] = p;
    }
}

// final: sa[i] = position of slot i; slot[i] = i (sorted by position afterwards: sa_rank)
__global__ __launch_bounds__(256) void k_sa_final_seq(const uint32_t* __restrict__ pos, uint32_t n,
        uint32_t* __restrict__ sa, uint32_t* __restrict__ slot)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        sa[i] = pos[i];
        slot[i] = i;
    }
}

// ---- The library primitives.  Every rocprim call of the project is made by the three helpers below.  Each asks the
// library how much temporary storage the call needs, fails with hipErrorOutOfMemory when the buffer is smaller, and only
// then runs.  With `query` set nothing runs: *query receives the size.
struct Tmp { void* p; size_t bytes; hipStream_t st; };      // the temporary storage and the stream of a call
// the two buffers of a sort operand: data in `cur`, scratch in `alt`; a sort leaves its result in `cur` and may swap them
template <typename T> struct Buf2 { T* cur; T* alt; };
#define TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)

template <typename F>
hipError_t with_tmp(Tmp t, size_t* query, F call)            // call(storage, bytes): the rocprim call
{
    size_t need = 0;
    const hipError_t e = call(nullptr, need);
    if (query != nullptr) *query = need;
    if (e != hipSuccess || query != nullptr) return e;
    if (need > t.bytes) return hipErrorOutOfMemory;
    return call(t.p, t.bytes);
}

// stable radix sort of n (key, value) pairs by the key bits [begin_bit, end_bit)
template <typename K, typename V>
hipError_t sort_pairs(Buf2<K>& k, Buf2<V>& v, size_t n, uint32_t begin_bit, uint32_t end_bit, const Tmp& t, size_t* query = nullptr)
{
    rocprim::double_buffer<K> kb(k.cur, k.alt);
    rocprim::double_buffer<V> vb(v.cur, v.alt);
    TRY(with_tmp(t, query, [&](void* p, size_t& b) { return rocprim::radix_sort_pairs(p, b, kb, vb, n, begin_bit, end_bit, t.st); }));
    k = { kb.current(), kb.alternate() };
    v = { vb.current(), vb.alternate() };
    return hipSuccess;
}

// v[i] = max(v[0..i]), in place
hipError_t max_scan(uint32_t* v, size_t n, const Tmp& t, size_t* query = nullptr)
{
    return with_tmp(t, query, [&](void* p, size_t& b) { return rocprim::inclusive_scan(p, b, v, v, n, rocprim::maximum<uint32_t>(), t.st); });
}

// v[i] = v[0] + ... + v[i - 1], in place
hipError_t sum_scan(uint32_t* v, size_t n, const Tmp& t, size_t* query = nullptr)
{
    return with_tmp(t, query, [&](void* p, size_t& b) { return rocprim::exclusive_scan(p, b, v, v, 0u, n, rocprim::plus<uint32_t>(), t.st); });
}

// out[key[i]] = v[i] for a permutation `key` of 0..n-1: radix passes over the key bits above INV_LOW, then the LDS
// step.  keys.cur / vals.cur hold the pairs, the alt buffers are scratch; all four are clobbered.
// u32 values: out may be one of the value buffers.  u64 values: out_lo / out_hi must not overlap them.
template <typename V>
hipError_t invert_perm(Buf2<uint32_t> keys, Buf2<V> vals, uint32_t n, uint32_t* out_lo, uint32_t* out_hi, const Tmp& t)
{
    if (n == 0) return hipSuccess;
    uint32_t bits = 1;
    while (bits < 32 && (1ull << bits) < n) ++bits;
    if (bits > INV_LOW) TRY(sort_pairs(keys, vals, (size_t)n, INV_LOW, bits, t));
    const uint32_t nb = (n + (1u << INV_LOW) - 1) >> INV_LOW;
    if constexpr (sizeof(V) == 4)
        hipLaunchKernelGGL(k_inv_low_u32, dim3(nb), dim3(1024), 0, t.st, keys.cur,
                reinterpret_cast<const uint32_t*>(vals.cur), n, out_lo);
    else
        hipLaunchKernelGGL(k_inv_low_u64, dim3(nb), dim3(1024), 0, t.st, keys.cur,
                reinterpret_cast<const uint64_t*>(vals.cur), n, out_lo, out_hi);
    return hipGetLastError();
}

// What the three stages of xzk_build_chains share: the batch, g = grid of the one-thread-per-position kernels, bb = bits
// of a Block number (sentinel bucket included), the caller's work buffers (n u32 / n u64 each) and the library scratch.
struct Build {
    const uint8_t* in;
    uint32_t n, block_size, nblocks, g, bb;
    uint32_t *keys_a, *keys_b, *vals_a, *vals_b;
    uint64_t *key64_a, *key64_b;                  // suffix order only
    Tmp t;
};

// Stage 1, the hash-chain heads: rank / sorted_pos (exact finder) or prev4 (sn: suffix-neighbourhood finder), prev2, prev3.
// Scratch: owns keys_a, keys_b, vals_a, vals_b on entry (content dead) and leaves nothing live in them.
hipError_t build_hash_heads(const Build& B, uint32_t hash_bytes, uint32_t hash_mask, uint32_t hash_bits, bool sn,
        uint32_t* rank, uint32_t* sorted_pos, uint32_t* prev2, uint32_t* prev3, uint32_t* prev4)
{
    const uint32_t n = B.n, g = B.g;
    hipStream_t st = B.t.st;
    const uint32_t which_list[3] = { 2u, 3u, 0u };
    // hash2 heads without a sort when the segment tables fit the scratch (always, except for tiny Blocks)
    const uint32_t h2_spb = (B.block_size + H2_SEG - 1) / H2_SEG;
    const bool h2_direct = hash_bytes >= 2 && B.nblocks != 0 && (uint64_t)B.nblocks * h2_spb * 1024ull <= (uint64_t)n;
    if (h2_direct) {
        const uint32_t nseg = B.nblocks * h2_spb;
        hipLaunchKernelGGL(k_h2_last, dim3(nseg), dim3(64), 0, st, B.in, n, B.block_size, h2_spb, hash_bytes, B.keys_a);
        hipLaunchKernelGGL(k_h2_scan, dim3(B.nblocks * 4), dim3(256), 0, st, B.keys_a, h2_spb);
        hipLaunchKernelGGL(k_h2_prev, dim3(nseg), dim3(64), 0, st, B.in, n, B.block_size, h2_spb, hash_bytes, B.keys_a, prev2);
    }
    for (int w = 0; w < 3; ++w) {
        const uint32_t which = which_list[w];
        if (which == 2 && h2_direct) continue;
        if (which == 3 && (hash_bytes != 4 || sn)) continue;      // the suffix-neighbourhood finder has no hash3 head
        const uint32_t kbits = which == 2 ? 10u : (which == 3 ? 16u : hash_bits);
        hipLaunchKernelGGL(k_hash_keys, dim3(g), dim3(256), 0, st, B.in, n, B.block_size, B.nblocks, hash_bytes,
                hash_mask, hash_bits, which, B.keys_a, B.vals_a);
        Buf2<uint32_t> kb{B.keys_a, B.keys_b}, vb{B.vals_a, B.vals_b};
        TRY(sort_pairs(kb, vb, (size_t)n, 0u, kbits + B.bb, B.t));
        uint32_t* const target = which == 2 ? prev2 : which == 3 ? prev3 : sn ? prev4 : nullptr;
        if (target != nullptr) {
            // distances in sorted order, then back to position order by a sort on the position
            hipLaunchKernelGGL(k_link_prev_seq, dim3(g), dim3(256), 0, st, kb.cur, vb.cur, n, target);
            TRY(invert_perm<uint32_t>(vb, {target, kb.cur}, n, target, nullptr, B.t));
        } else {
            hipLaunchKernelGGL(k_link_main, dim3(g), dim3(256), 0, st, kb.cur, vb.cur, n, sorted_pos, rank);
        }
    }
    return hipSuccess;
}

// Stage 2, suffix-order round 0: the slots ordered by (Block, first 8 bytes, position).
// Scratch: owns all six work buffers on entry (content dead).  Leaves the positions in slot order in pos.cur (vals_a or
// vals_b; pos.alt, the other one, is free), the max-scanned group start of every slot in keys_a; keys_b, key64_* free.
hipError_t build_sa_round0(const Build& B, Buf2<uint32_t>& pos)
{
    const uint32_t n = B.n, g = B.g;
    hipStream_t st = B.t.st;
    uint32_t* const grp = B.keys_a;               // group-start scan buffer (the hash sorts are done with it)
    // round 0: chunk sort
    hipLaunchKernelGGL(k_sa_chunk_keys, dim3(g), dim3(256), 0, st, B.in, n, B.block_size, B.key64_a, B.vals_a);
    if (B.nblocks > 1 && B.nblocks <= 256) {
        // Few, large Blocks (the normal case): one sort per Block.  The positions start out in Block order, so a
        // sort that never mixes Blocks needs no sort by Block number afterwards, and no rocprim call exceeds the
        // 2^30 elements above which it splits every pass into two launches.
        int in_alt = -1;
        for (uint32_t b = 0; b < B.nblocks; ++b) {
            const size_t off = (size_t)b * B.block_size;
            if (off >= n) break;
            const size_t cnt = (size_t)n - off < B.block_size ? (size_t)n - off : B.block_size;
            Buf2<uint64_t> k{B.key64_a + off, B.key64_b + off};
            Buf2<uint32_t> v{B.vals_a + off, B.vals_b + off};
            TRY(sort_pairs(k, v, cnt, 0u, 64u, B.t));
            const int alt = k.cur == B.key64_b + off;
            if (in_alt < 0) in_alt = alt;
            else if (alt != in_alt) {
                // a Block of another size class took another route through rocprim: bring it to the common side
                TRY(hipMemcpyAsync((in_alt ? B.key64_b : B.key64_a) + off, k.cur, cnt * 8, hipMemcpyDeviceToDevice, st));
                TRY(hipMemcpyAsync((in_alt ? B.vals_b : B.vals_a) + off, v.cur, cnt * 4, hipMemcpyDeviceToDevice, st));
            }
        }
        pos = in_alt ? Buf2<uint32_t>{B.vals_b, B.vals_a} : Buf2<uint32_t>{B.vals_a, B.vals_b};
        hipLaunchKernelGGL(k_sa_flags64, dim3(g), dim3(256), 0, st, in_alt ? B.key64_b : B.key64_a, n, B.block_size, grp);
        return max_scan(grp, (size_t)n, B.t);
    }
    Buf2<uint64_t> k64{B.key64_a, B.key64_b};
    pos = {B.vals_a, B.vals_b};
    TRY(sort_pairs(k64, pos, (size_t)n, 0u, 64u, B.t));
    hipLaunchKernelGGL(k_sa_flags64, dim3(g), dim3(256), 0, st, k64.cur, n, 0u, grp);
    TRY(max_scan(grp, (size_t)n, B.t));
    if (B.nblocks <= 1) return hipSuccess;
    // many small Blocks: one sort of everything, then a stable sort by Block number; values = (position,
    // chunk group), the chunk keys are dead now
    Buf2<uint32_t> bk{B.keys_b, pos.alt};
    Buf2<uint64_t> bv{k64.alt, k64.cur};
    hipLaunchKernelGGL(k_sa_block_keys, dim3(g), dim3(256), 0, st, pos.cur, grp, n, B.block_size, bk.cur, bv.cur);
    TRY(sort_pairs(bk, bv, (size_t)n, 0u, B.bb, B.t));
    // positions go back to pos.cur (vals buffer that held them before; its content is dead)
    hipLaunchKernelGGL(k_sa_block_unpack, dim3(g), dim3(256), 0, st, bk.cur, bv.cur, n, pos.cur, grp);
    // pos.alt may have been used as a key buffer: both vals buffers are free for reuse from here on except pos.cur
    return max_scan(grp, (size_t)n, B.t);
}

// Stage 3, the doubling rounds h = 8, 16, ... up to sa_depth bytes, then sa / sa_rank.
// Scratch on entry: as build_sa_round0 leaves it.  Roles here: keys_a = group starts (grp), keys_b = compact index (idx),
// key64_a / key64_b = sort keys and inversion values (first word of key64_b: the undecided-slot count), sa / sa_rank =
// values of the compact sorts, pos.alt = their slots.  rp8 / rp16: two u32 arrays each, by-position rank at [0, n),
// left-neighbour distance at [n, 2n).  Leaves sa = slot order, sa_rank = its inverse, prev24 / prev32; work buffers dead.
hipError_t build_sa_doubling(const Build& B, Buf2<uint32_t> pos, uint32_t sa_depth, uint64_t* rp8, uint64_t* rp16,
        uint32_t* sa, uint32_t* sa_rank, uint32_t* prev24, uint32_t* prev32)
{
    const uint32_t n = B.n, g = B.g, block_size = B.block_size;
    uint64_t *const key64_a = B.key64_a, *const key64_b = B.key64_b;
    hipStream_t st = B.t.st;
    uint32_t* const grp = B.keys_a;
    uint32_t sbits = 1, fbits = 1;                    // bits of a Block-relative rank (<= block_size), of a rank (<= n)
    while (sbits < 32 && (1ull << sbits) <= (uint64_t)min(block_size, n)) ++sbits;
    while (fbits < 32 && (1ull << fbits) <= (uint64_t)n) ++fbits;
    if (sa_depth < 32) sa_depth = 32;
    // round h = 8: every slot takes part (text: 71 % of the positions still share their 8 bytes with another one)
    uint32_t* const rk32 = reinterpret_cast<uint32_t*>(rp8);         // rank at rk32[0..n), left-neighbour distance at rk32[n..2n)
    hipLaunchKernelGGL(k_sa_rank_seq, dim3(g), dim3(256), 0, st, pos.cur, grp, n, reinterpret_cast<uint2*>(key64_a));
    TRY(invert_perm<uint64_t>(pos, {key64_a, key64_b}, n, rk32, rk32 + n, B.t));
    // keys in position order (values = iota): both `pos` buffers are free again
    hipLaunchKernelGGL(k_sa_pair_keys_pos, dim3(g), dim3(256), 0, st, rk32, n, block_size, 8u, sbits, key64_a, pos.cur);
    Buf2<uint64_t> k8{key64_a, key64_b};
    TRY(sort_pairs(k8, pos, (size_t)n, 0u, sbits + fbits, B.t));
    hipLaunchKernelGGL(k_sa_flags64, dim3(g), dim3(256), 0, st, k8.cur, n, 0u, grp);
    TRY(max_scan(grp, (size_t)n, B.t));
    // rounds h = 16, 32, ...: by-position rank in rkpos (kept up to date by the compact rounds), slots in pos, groups in grp
    uint32_t* const rkpos = reinterpret_cast<uint32_t*>(rp16);
    uint32_t* const idx = B.keys_b;                   // free since round 0
    uint32_t* const d_count = reinterpret_cast<uint32_t*>(key64_b);
    bool rank_valid = false;
    const char* const cenv = getenv("XZAMD_SA_COMPACT");          // 0: every round orders all slots (measurement knob)
    const bool compact_on = !(cenv && *cenv == '0');
    for (uint32_t h = 16; 2 * h <= sa_depth; h *= 2) {
        const bool more = 4 * h <= sa_depth;
        if (h == 16) {
            // (rank, distance to the left neighbour inside the 16-byte group) of every slot, brought to position order;
            // the slot order itself stays (the inversion works on a copy of it)
            hipLaunchKernelGGL(k_sa_rank_seq, dim3(g), dim3(256), 0, st, pos.cur, grp, n, reinterpret_cast<uint2*>(key64_a));
            TRY(hipMemcpyAsync(idx, pos.cur, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
            TRY(invert_perm<uint64_t>({idx, sa}, {key64_a, key64_b}, n, rkpos, rkpos + n, B.t));
            rank_valid = true;
        } else if (!rank_valid) {
            uint32_t *const ra = reinterpret_cast<uint32_t*>(key64_a), *const rb = reinterpret_cast<uint32_t*>(key64_b);
            hipLaunchKernelGGL(k_sa_rank_only_seq, dim3(g), dim3(256), 0, st, grp, n, ra);
            TRY(hipMemcpyAsync(idx, pos.cur, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
            TRY(invert_perm<uint32_t>({idx, sa}, {ra, rb}, n, rkpos, nullptr, B.t));
            rank_valid = true;
        }
        uint32_t m = n;
        if (compact_on && n >= 2) {
            // how many slots are still undecided?  (One word back to the host: the sort below is sized by it.)
            hipLaunchKernelGGL(k_sa_unres, dim3(g), dim3(256), 0, st, grp, n, idx);
            TRY(sum_scan(idx, (size_t)n, B.t));
            hipLaunchKernelGGL(k_sa_count, dim3(1), dim3(1), 0, st, idx, grp, n, d_count);
            TRY(hipMemcpyAsync(&m, d_count, 4, hipMemcpyDeviceToHost, st));
            TRY(hipStreamSynchronize(st));
            if (m == 0) break;                        // every suffix is distinguished: the order is final
        }
        if (h == 16 && prev24 != nullptr && compact_on && n >= 2) {
            // prev24 (the nearest earlier position with the same 24 bytes): the members of the 16-byte groups once more,
            // ordered by (group, rank after 8 bytes of p + 16) -- an extra sort of the m undecided slots only; the key,
            // value and slot buffers of the compact round below are free until it runs
            uint32_t* const cslot = pos.alt;
            hipLaunchKernelGGL(k_sa_compact, dim3(g), dim3(256), 0, st, pos.cur, grp, idx, reinterpret_cast<const uint32_t*>(rp8), n,
                    block_size, 16u, sbits, key64_a, sa, cslot);
            Buf2<uint64_t> kk{key64_a, key64_b};
            Buf2<uint32_t> vv{sa, sa_rank};
            TRY(sort_pairs(kk, vv, (size_t)m, 0u, sbits + fbits, B.t));
            hipLaunchKernelGGL(k_sa_prev_scatter, dim3(grid_for(m, 256, 256 * 16)), dim3(256), 0, st, kk.cur, vv.cur, m, prev24);
        }
        if (compact_on && n >= 2 && (uint64_t)m * 10 <= (uint64_t)n * 6) {
            uint32_t* const cslot = pos.alt;
            const uint32_t gm = grid_for(m, 256, 256 * 16);
            hipLaunchKernelGGL(k_sa_compact, dim3(g), dim3(256), 0, st, pos.cur, grp, idx, rkpos, n, block_size, h, sbits,
                    key64_a, sa, cslot);
            Buf2<uint64_t> kk{key64_a, key64_b};
            Buf2<uint32_t> vv{sa, sa_rank};
            TRY(sort_pairs(kk, vv, (size_t)m, 0u, sbits + fbits, B.t));
            if (h == 16 && prev32 != nullptr)         // by-product: the 32-byte groups' left neighbours
                hipLaunchKernelGGL(k_sa_prev_scatter, dim3(gm), dim3(256), 0, st, kk.cur, vv.cur, m, prev32);
            hipLaunchKernelGGL(k_sa_newgrp, dim3(gm), dim3(256), 0, st, kk.cur, cslot, m, idx);
            TRY(max_scan(idx, (size_t)m, B.t));
            hipLaunchKernelGGL(k_sa_writeback, dim3(gm), dim3(256), 0, st, vv.cur, cslot, idx, m, pos.cur, grp, rkpos);
        } else {
            // most slots are undecided (highly repetitive data): the full round, keys made in position order
            hipLaunchKernelGGL(k_sa_pair_keys_pos, dim3(g), dim3(256), 0, st, rkpos, n, block_size, h, sbits, key64_a, pos.cur);
            Buf2<uint64_t> kk{key64_a, key64_b};
            TRY(sort_pairs(kk, pos, (size_t)n, 0u, sbits + fbits, B.t));
            if (h == 16 && prev32 != nullptr)
                hipLaunchKernelGGL(k_sa_prev_scatter, dim3(g), dim3(256), 0, st, kk.cur, pos.cur, n, prev32);
            if (more) {            // another round follows: its ranks need the groups of this order
                hipLaunchKernelGGL(k_sa_flags64, dim3(g), dim3(256), 0, st, kk.cur, n, 0u, grp);
                TRY(max_scan(grp, (size_t)n, B.t));
            }
            rank_valid = false;
        }
    }
    // sa = slot order; sa_rank = its inverse (grp = keys_a is dead: scratch of the inversion)
    hipLaunchKernelGGL(k_sa_final_seq, dim3(g), dim3(256), 0, st, pos.cur, n, sa, sa_rank);
    return invert_perm<uint32_t>(pos, {sa_rank, B.keys_a}, n, sa_rank, nullptr, B.t);
}

} // namespace

// see kernels_internal.h
hipError_t sort_launch_order(uint32_t* key_a, uint32_t* key_b, uint32_t* val_a, uint32_t* val_b, uint32_t n,
        void* tmp, size_t tmp_bytes, uint32_t** order_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_iota, dim3(grid_for(n, 256, 4096)), dim3(256), 0, st, val_a, n);
    Buf2<uint32_t> kb{key_a, key_b}, vb{val_a, val_b};
    TRY(sort_pairs(kb, vb, (size_t)n, 0u, 32u, Tmp{tmp, tmp_bytes, st}));
    *order_out = vb.cur;
    return hipSuccess;
}

extern "C" {

int xzk_sort_temp_bytes(uint32_t n, uint32_t end_bit, uint64_t* bytes)
{
    size_t sz = 0;
    Buf2<uint32_t> k{}, v{};
    const hipError_t e = sort_pairs(k, v, (size_t)n, 0u, end_bit, Tmp{nullptr, 0, (hipStream_t)0}, &sz);
    *bytes = sz;
    return (int)e;
}

// temporary storage the suffix-order build needs (largest of its three primitives)
int xzk_sa_temp_bytes(uint32_t n, uint64_t* bytes)
{
    const Tmp none = { nullptr, 0, (hipStream_t)0 };
    size_t s0 = 0, s1 = 0, s2 = 0;
    Buf2<uint64_t> w{};                           // the three primitives of the suffix order, nothing runs
    Buf2<uint32_t> u{};
    hipError_t e = sort_pairs(w, u, (size_t)n, 0u, 64u, none, &s0);
    if (e == hipSuccess) e = sort_pairs(u, w, (size_t)n, 0u, 32u, none, &s1);
    if (e == hipSuccess) e = max_scan(nullptr, (size_t)n, none, &s2);
    if (e != hipSuccess) return (int)e;
    if (s1 > s0) s0 = s1;
    *bytes = s2 > s0 ? s2 : s0;
    return 0;
}

// Builds the match-finder structure of a batch.
//   exact finder (sa == NULL):   rank / sorted_pos (main chain), prev2, prev3
//   suffix-neighbourhood finder: prev2, prev4, the suffix order sa / sa_rank and its by-products
//                                rp8 / rp16: per position (rank of the round, distance to the nearest earlier
//                                position with the same 8 / 16 bytes)
// keys_a/keys_b/vals_a/vals_b: n u32 each; key64_a/key64_b: n u64 each (sa != NULL only).
int xzk_build_chains(const uint8_t* d_in, uint32_t n, uint32_t block_size, uint32_t nblocks,
        uint32_t hash_bytes, uint32_t hash_mask, uint32_t hash_bits, uint32_t sa_depth,
        uint32_t* keys_a, uint32_t* keys_b, uint32_t* vals_a, uint32_t* vals_b,
        void* sort_tmp, uint64_t sort_tmp_bytes,
        uint32_t* rank, uint32_t* sorted_pos, uint32_t* prev2, uint32_t* prev3,
        uint32_t* prev4, uint64_t* rp8, uint64_t* rp16, uint64_t* key64_a, uint64_t* key64_b,
        uint32_t* sa, uint32_t* sa_rank, uint32_t* prev24, uint32_t* prev32, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    uint32_t bb = 0;
    while ((1u << bb) < nblocks + 1) ++bb;
    const Build B = { d_in, n, block_size, nblocks, grid_for(n, 256, 256 * 16), bb, keys_a, keys_b, vals_a, vals_b,
            key64_a, key64_b, { sort_tmp, (size_t)sort_tmp_bytes, st } };
    hipError_t e = build_hash_heads(B, hash_bytes, hash_mask, hash_bits, sa != nullptr, rank, sorted_pos, prev2, prev3, prev4);
    if (e != hipSuccess) return (int)e;
    if (sa == nullptr) return (int)hipGetLastError();
    // ---- suffix order ----
    if (prev24 != nullptr && hipMemsetAsync(prev24, 0, (size_t)n * 4, st) != hipSuccess) return (int)hipErrorUnknown;
    if (prev32 != nullptr && hipMemsetAsync(prev32, 0, (size_t)n * 4, st) != hipSuccess) return (int)hipErrorUnknown;
    Buf2<uint32_t> pos;
    e = build_sa_round0(B, pos);
    if (e == hipSuccess) e = build_sa_doubling(B, pos, sa_depth, rp8, rp16, sa, sa_rank, prev24, prev32);
    if (e != hipSuccess) return (int)e;
    return (int)hipGetLastError();
}

} // extern "C"
