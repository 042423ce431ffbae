// match_common.h -- shared by lzma_find.hip and lzma_kernels.hip: the exact HC3/HC4 finder (do_round; k_find_exact runs
// it for every position, span_encode_one<0, false> in-kernel) and the match-list records the batch finders write.
#ifndef XZAMD_MATCH_COMMON_H
#define XZAMD_MATCH_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave.h"

namespace {

constexpr uint32_t MATCH_LEN_MAX = 273;

// ------------------------------------------------------------------------------------------
// Wave-cooperative byte comparison
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ld64(const uint8_t* p)
{
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// Per-lane: length of the common prefix of in[q..] and in[x..], at most lim.  Lanes diverge.
// 32 bytes per trip: every loop iteration is a dependent HBM/L2 round trip, so the trip count
// (not the byte count) is what a long match costs.
__device__ __forceinline__ uint32_t lane_cmplen(const uint8_t* __restrict__ in, uint32_t q, uint32_t x, uint32_t lim)
{
    uint32_t len = 0;
    while (len + 32 <= lim) {
        const uint8_t* a = in + q + len;
        const uint8_t* b = in + x + len;
        const uint64_t a0 = ld64(a), a1 = ld64(a + 8), a2 = ld64(a + 16), a3 = ld64(a + 24);
        const uint64_t b0 = ld64(b), b1 = ld64(b + 8), b2 = ld64(b + 16), b3 = ld64(b + 24);
        uint64_t d = a0 ^ b0;
        if (d) return len + (uint32_t)(__builtin_ctzll(d) >> 3);
        d = a1 ^ b1;
        if (d) return len + 8 + (uint32_t)(__builtin_ctzll(d) >> 3);
        d = a2 ^ b2;
        if (d) return len + 16 + (uint32_t)(__builtin_ctzll(d) >> 3);
        d = a3 ^ b3;
        if (d) return len + 24 + (uint32_t)(__builtin_ctzll(d) >> 3);
        len += 32;
    }
    while (len + 8 <= lim) {
        const uint64_t d = ld64(in + q + len) ^ ld64(in + x + len);
        if (d) return len + (uint32_t)(__builtin_ctzll(d) >> 3);
        len += 8;
    }
    while (len < lim && in[q + len] == in[x + len]) ++len;
    return len;
}

// Whole wave: extend a known common prefix `len` of in[a..], in[b..] up to lim (64 bytes/step).
__device__ __forceinline__ uint32_t wave_cmplen(const uint8_t* __restrict__ in, uint32_t a, uint32_t b,
        uint32_t len, uint32_t lim)
{
    const uint32_t lane = threadIdx.x;
    while (len < lim) {
        const uint32_t off = len + lane;
        const bool mism = off >= lim || in[a + off] != in[b + off];
        const uint64_t m = __ballot(mism);
        if (m) { len += (uint32_t)__builtin_ctzll(m); break; }
        len += 64;
    }
    return len < lim ? len : lim;
}

__device__ __forceinline__ uint32_t prefix_max_incl(uint32_t v)
{
    const uint32_t lane = threadIdx.x;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = __shfl_up(v, s);
        if (lane >= (uint32_t)s) v = max(v, o);
    }
    return v;
}

// ------------------------------------------------------------------------------------------
// One "round": everything lzma_mf_find() would report at position x (lz_encoder_mf.c:22-79,
// HC3 :305-335, HC4 :366-413, chain walk :250-287) plus the four rep-match lengths at x.
// Lane roles: 0 = hash2 candidate, 1 = hash3 candidate, 2 = own slot (bucket flag only),
// 3..2+depth = chain candidates in chain order, 60..63 = rep0..rep3.
// ------------------------------------------------------------------------------------------
struct Round {
    uint64_t mask;      // recorded matches, in matches[] order (ascending lane)
    uint32_t L;         // per lane: recorded length (lanes 0..58), rep length (60..63)
    uint32_t D;         // per lane: distance (zero based)
    uint32_t longest;   // lzma_mf_find() return value (incl. the > nice_len extension)
};

struct Env {
    const uint8_t* __restrict__ in;
    const uint32_t* __restrict__ rank;
    const uint32_t* __restrict__ sorted_pos;
    const uint32_t* __restrict__ prev2;
    const uint32_t* __restrict__ prev3;
    uint32_t nice, depth, hb, cyclic;
    uint32_t block_end;
    uint32_t n_last;                            // last valid byte offset of the batch (prefetch clamp)
    // match lists written by k_find_sn / k_find_exact (one 32-byte record per position), read by the list-driven parser
    const uint16_t* __restrict__ mlen;
    const uint32_t* __restrict__ mdist;
    uint32_t packed;                            // lists are one u32 per entry: length << 23 | distance-1 (dict <= 8 MiB)
};
constexpr uint32_t LIST_K = 7;                // entries kept per position (the LIST_K longest)
constexpr uint32_t LIST_W = 8;                // words per position: LIST_K entries + trailer (count | len2 of the two longest)
constexpr uint32_t LEN2_MAX = 127;            // cap of the rep0 run recorded with the two longest entries

// ------------------------------------------------------------------------------------------
// Software prefetch of the parse-independent per-position data.  Rounds mostly visit consecutive
// positions (lookahead of the fast parser, every node of an optimal-parser window), so while the
// wave works on position x the loads for x+1 (chain slots) and x+2 (rank / prev links) are already
// in flight: two of the three dependent HBM round trips of a round leave the critical path.
// ------------------------------------------------------------------------------------------
struct PreA { uint32_t rk, d2, d3; };
struct Pre {
    uint32_t pos;       // position (a, ent) belong to; `an` belongs to pos + 1
    bool valid;
    PreA a;
    uint32_t ent;       // per lane: chain slot entry for this lane's role
    PreA an;
};

__device__ __forceinline__ PreA load_a(const Env& e, uint32_t x)
{
    x = x < e.n_last ? x : e.n_last;
    PreA a;
    a.rk = e.rank[x];
    a.d2 = e.prev2[x];
    a.d3 = e.hb == 4 ? e.prev3[x] : 0;
    return a;
}

__device__ __forceinline__ uint32_t load_ent(const Env& e, const PreA& a)
{
    const uint32_t lane = threadIdx.x;
    uint32_t ent = 0x80000000u;                      // out of range == "bucket start"
    const bool in_chain = lane >= 2 && lane <= 2 + e.depth;
    if (in_chain && a.rk >= lane - 2) ent = e.sorted_pos[a.rk - (lane - 2)];
    return ent;
}

__device__ __forceinline__ void fetch(const Env& e, Pre& P, uint32_t x, PreA& a, uint32_t& ent)
{
    if (!(P.valid && P.pos == x)) {                  // cold start: two dependent round trips
        P.a = load_a(e, x);
        P.ent = load_ent(e, P.a);
        P.an = load_a(e, x + 1);
    }
    a = P.a;
    ent = P.ent;
    const PreA an = P.an;                            // issued one round ago
    P.a = an;
    P.ent = load_ent(e, an);                         // for x + 1, consumed next round
    P.an = load_a(e, x + 2);
    P.pos = x + 1;
    P.valid = true;
}

template <bool REPS = true>
__device__ __forceinline__ void do_round(const Env& e, Pre& P, uint32_t x, uint32_t end,
        uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, Round& R)
{
    PreA pa;
    uint32_t pent;
    fetch(e, P, x, pa, pent);
    const uint32_t lane = threadIdx.x;
    const uint32_t avail = end - x;
    const uint32_t buf_avail = avail < MATCH_LEN_MAX ? avail : MATCH_LEN_MAX;
    uint32_t len_limit = avail;
    bool mf_ok = true;
    if (e.nice <= len_limit) len_limit = e.nice;
    else if (len_limit < e.hb) mf_ok = false;            // "pending": no matches reported

    uint32_t q = 0, lim = 0;
    bool chain_valid = false;
    if (mf_ok) {
        const uint32_t d2 = pa.d2;
        const uint32_t d3 = pa.d3;
        if (lane == 0) {
            if (d2 != 0 && d2 < e.cyclic) { q = x - d2; lim = len_limit; }
        } else if (lane == 1) {
            if (d3 != 0 && d3 != d2 && d3 < e.cyclic) { q = x - d3; lim = len_limit; }
        }
        const uint32_t ent = pent;
        const bool in_chain = lane >= 2 && lane <= 2 + e.depth;
        const uint64_t flags = __ballot(in_chain && (ent >> 31)) >> 2;   // bit j = flag of slot rank-j
        if (lane >= 3 && in_chain) {
            const uint32_t j = lane - 2;                 // candidate number 1..depth
            const bool same_bucket = (flags & ((1ull << j) - 1)) == 0;
            const uint32_t qp = ent & 0x7FFFFFFFu;
            if (same_bucket && x - qp < e.cyclic) { chain_valid = true; q = qp; lim = len_limit; }
        }
    }
    if (REPS && lane >= 60) {
        const uint32_t rep = lane == 60 ? r0 : lane == 61 ? r1 : lane == 62 ? r2 : r3;
        q = x - rep - 1;
        lim = buf_avail;
    }

    uint32_t L = lane_cmplen(e.in, q, x, lim);
    const uint32_t D = x - q - 1;

    const uint32_t L0 = lane_of(L, 0), L1 = lane_of(L, 1);
    const bool has2 = L0 >= 1;              // first byte equal => (by the hash) >= 2 bytes equal
    const bool has3 = L1 >= 1;              // lane 1 only active for HC4
    uint32_t best;
    bool done;
    if (e.hb == 4) {
        best = has3 ? L1 : (has2 ? L0 : 1);
        done = (has2 || has3) && best == len_limit;
        if (best < 3) best = 3;
    } else {
        best = has2 ? L0 : 2;
        done = has2 && best == len_limit;
    }
    const uint32_t X = chain_valid ? L : 0;
    const uint32_t incl = prefix_max_incl(X);
    uint32_t excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 0;
    bool rec = chain_valid && !done && X > max(best, excl);
    if (lane == 0) { rec = has2; if (has2 && has3) L = 2; }
    if (lane == 1) rec = has3;
    R.mask = mf_ok ? __ballot(rec) : 0ull;
    R.L = L;
    R.D = D;
    uint32_t longest = 0;
    if (R.mask) {
        const uint32_t top = 63 - (uint32_t)__builtin_clzll(R.mask);
        longest = lane_of(L, top);
        if (longest == e.nice) {
            const uint32_t dist = lane_of(D, top);
            longest = wave_cmplen(e.in, x, x - dist - 1, longest, buf_avail);
        }
    }
    R.longest = longest;
}

// ---- list-driven rounds ------------------------------------------------------------------------
// The match finder is parse independent (find and skip both insert), so k_find_t runs it for every
// position of the batch as a separate, fully parallel kernel.  The parser then streams the lists:
// positions are visited strictly in order, so the record of x+1 is always in flight while x is
// priced.  Only the four rep-match lengths depend on the parse; lanes 60..63 measure them here.
// (the record in flight is kept as it was loaded -- one register for the packed form, two for the other -- and taken apart
// when its round is worked out, not when it is loaded: it is live across the whole node in front)
struct ListPre { uint32_t pos; bool valid; uint32_t v, l16; };

// One 32-byte record per position (see k_find_sn): lanes 0..6 = entries, lane 7 = trailer.
__device__ __forceinline__ void lists_load(const Env& e, uint32_t x, uint32_t& v, uint32_t& l16)
{
    const uint32_t lane = threadIdx.x;
    x = x < e.n_last ? x : e.n_last;
    const uint64_t base = (uint64_t)x * LIST_W + (lane & (LIST_W - 1));
    v = e.mdist[base];                             // every lane loads (lanes >= LIST_W repeat the record): no exec masking
    l16 = e.packed ? 0u : (uint32_t)e.mlen[base];
}

// lane LIST_K of `tr` holds the trailer
__device__ __forceinline__ void lists_split(const Env& e, uint32_t v, uint32_t l16, uint32_t& sl, uint32_t& sd, uint32_t& tr)
{
    tr = v;
    if (e.packed) {
        sl = v >> 23; sd = v & 0x7FFFFFu;
    } else {
        sd = v;
        sl = l16;
    }
}

} // namespace

#endif
