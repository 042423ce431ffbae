// lzma_find.hip -- the batch match finders and the span plan (stage table: lzma_kernels.hip).  They read the structure
// lzma_build.hip makes and write what the parsers stream: a match list per position, and the spans of every Block.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_api.h"
#include "kernels_internal.h"
#include "wave.h"
#include "match_common.h"

namespace {

// ------------------------------------------------------------------------------------------
// Batch match finders: one wavefront per run of FIND_RUN consecutive positions.  Because find and
// skip both insert (lz_encoder_mf.c:366-441), the matches of a position depend on the data only, so
// they are computed for every position of the batch ahead of the (serial) parser, which streams
// them.  Per position one 32-byte record: LIST_K entries sorted by length (length << 23 | distance-1
// when the dictionary is <= 8 MiB, else distance-1 with the lengths in a u16 side array), the > nice_len
// extension folded into the last one, and a trailer word
//     count | len2(longest) << 8 | len2(second longest) << 16
// where len2 = length of the rep0 run behind the byte that follows the match (the "match + literal +
// rep0" edge of the parser, lzma_encoder_optimum_normal.c:728-790).
// ------------------------------------------------------------------------------------------
constexpr uint32_t FIND_RUN = 256;

// bytes matched inside one 16-byte trip (16 = all)
__device__ __forceinline__ uint32_t match16(const uint4& a, const uint4& b)
{
    const uint32_t d0 = a.x ^ b.x, d1 = a.y ^ b.y, d2 = a.z ^ b.z, d3 = a.w ^ b.w;
    const uint32_t off = d0 ? 0u : d1 ? 4u : d2 ? 8u : 12u;
    const uint32_t d = d0 ? d0 : d1 ? d1 : d2 ? d2 : d3;
    return d ? off + ((uint32_t)__builtin_ctz(d) >> 3) : 16u;
}

// continue a compare whose first `len` bytes are known equal
__device__ __forceinline__ uint32_t lane_cmplen16_from(const uint8_t* __restrict__ in, uint32_t q, uint32_t x, uint32_t len,
        uint32_t lim)
{
    while (len + 16 <= lim) {
        uint4 a, b;
        __builtin_memcpy(&a, in + q + len, 16);
        __builtin_memcpy(&b, in + x + len, 16);
        const uint32_t m = match16(a, b);
        len += m;
        if (m < 16) return len;
    }
    while (len < lim && in[q + len] == in[x + len]) ++len;
    return len;
}

// inclusive prefix maximum inside each half (32 lanes) of the wavefront
__device__ __forceinline__ uint32_t prefix_max_half(uint32_t v)
{
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false));   // row_shr:1
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false));   // row_shr:2
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false));   // row_shr:4
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false));   // row_shr:8
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false));   // row_bcast:15 -> rows 1, 3
    return v;
}

struct SnArgs {
    const uint8_t* __restrict__ in;
    const uint32_t* __restrict__ sa;        // slot -> position (Block-major: the slots of a Block are its positions' range)
    const uint32_t* __restrict__ sa_rank;   // position -> slot
    const uint32_t* __restrict__ prev2;
    const uint32_t* __restrict__ prev4;
    const uint32_t* __restrict__ prev8;
    const uint32_t* __restrict__ prev16;
    const uint32_t* __restrict__ prev24;    // nearest earlier position with the same 24 / 32 bytes
    const uint32_t* __restrict__ prev32;
    // Which runs a launch covers: 0 = all; 1 = the runs that touch the first XZAMD_SEED_LEN bytes of a Block (workgroup =
    // Block * SEED_RUNS + j); 2 = all the others.  The two-phase mode parses the seed pieces (k_parse_pieces phase 0)
    // underneath launch 2.
    uint32_t mode;
};
constexpr uint32_t SEED_RUNS = XZAMD_SEED_LEN / 256 + 1;
constexpr uint32_t SN_WMAX = 5;

// Suffix-neighbourhood finder (oracle: find_sn).  Both hot kernels of this path are bound by instruction
// issue, not by memory (this one, with the all-pairs filter it used to have: 115 vector instructions per position held
// the SIMDs for 270 of a launch's 298 ms; DESIGN.md 3.2 has the figures with the row sort below), so
// the finder gives a position only the lanes it can use: a wavefront works on FOUR
// positions at once, one per DPP row of 16 lanes, and everything "uniform per position" lives in vector
// registers (the scalar unit only runs the loop).  Lane roles inside a row, t = lane & 15, slot r = own slot:
//   t =  0..4   slots r-1 .. r-5   (left neighbours, nearest first)
//   t =  5..9   slots r+1 .. r+5   (right neighbours, nearest first)
//   t = 10 / 11 / 12   nearest previous position with equal hash2 / hash3 / hash4
//   t = 13 / 14        nearest previous position with the same 8 / 16 bytes (by-products of the sort rounds)
// A neighbour is eligible when it lies earlier in the same Block and inside the dictionary; it is a candidate
// when it is more recent than every eligible neighbour nearer on its side ("recency record": exactly the
// nodes BT4's descent would visit).  All candidates are compared with the text at x in parallel (16 bytes per
// trip) and filtered by the Pareto rule: the row's 16 candidates are sorted by distance (row_sort16: 10 DPP
// compare-exchange layers) and a candidate stays when it is longer than everything sorted before it.  From the sort
// on, a lane holds the entry of its rank in the row, not the candidate it fetched.
// Row r of the wavefront at x0 owns positions x0 + 64 r .. x0 + 64 r + 63.  The loop is software pipelined
// three deep: while position i is compared and filtered, the first 16 bytes of every candidate of i + 1 and
// the window of i + 2 are in flight.
constexpr uint32_t SN_NONE = 0xFFFFFFFFu;     // "no neighbour in this lane" (positions are < 2^31)
constexpr uint32_t ROW_RUN = FIND_RUN / 4;    // positions per row

template <int N>
__device__ __forceinline__ uint32_t row_ror(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x120 + N, 0xF, 0xF, false);    // row_ror:N
}
template <int N>
__device__ __forceinline__ uint32_t row_shr(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + N, 0xF, 0xF, false);    // row_shr:N, 0 shifted in
}

// The Pareto filter of a row: sort the row's 16 candidates by distance, then a candidate survives when it is longer
// than everything nearer (an exclusive prefix maximum), and its place in the list is the number of survivors below it.
//
// Sort key.  Packed lists (dictionary <= 8 MiB): distance - 1 < 2^23 and L <= 273 < 2^9, so (distance - 1) << 9 | L is
// one 32-bit word and a compare-exchange is v_min_u32 / v_max_u32; a lane without a candidate takes SORT_NONE, which
// sorts behind every candidate and carries length 0.  Unpacked lists: the pair (distance - 1, L), ordered by the
// distance alone, a lane without a candidate (0xFFFFFFFF, 0).
// Ties.  Two lanes with the same distance name the same source position, and a position has ONE match length at x (lim
// and the bytes are the same in every lane of the row), so wherever both are candidates their keys are identical:
// which of them the network puts first cannot be seen in the result, and no lane number is needed as a tie-break.
// (Where the lengths seem to differ -- L = 3 in the hash2 lane, whose minimum is 2, beside a lane whose minimum is 4 --
// only one of the two is a candidate.)  The earlier all-pairs filter dropped the higher lane of such a pair "whatever
// its length"; with equal lengths that is the rule "not longer than something sorted before it", which the prefix
// maximum applies.
//
// Network: bitonic, written so that every layer sorts ascending (the first layer of a merge compares with the MIRROR
// image inside the block, the others with lane ^ j), 10 layers.  Every partner is one DPP pattern inside the row
// (quad_perm for lane ^ 1, ^ 2, ^ 3; row_half_mirror = lane ^ 7; row_mirror = lane ^ 15) but lane ^ 4, which is
// row_shl:4 for banks 0 and 2 and row_shr:4 for banks 1 and 3.  No LDS, nothing crosses a row.
constexpr uint32_t SORT_NONE = 0xFFFFFE00u;
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_XOR3 = 0x1B, DPP_XOR7 = 0x141, DPP_XOR15 = 0x140;   // quad_perm / mirrors
constexpr int DPP_XOR4 = -1;

template <int CTRL>
__device__ __forceinline__ uint32_t row_partner(uint32_t v)
{
    if constexpr (CTRL == DPP_XOR4) {
        const int up = __builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xF, 0x5, false);      // row_shl:4 -> lanes 0-3, 8-11
        return (uint32_t)__builtin_amdgcn_update_dpp(up, (int)v, 0x114, 0xF, 0xA, false);   // row_shr:4 -> lanes 4-7, 12-15
    } else {
        return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
    }
}
// one layer: `low` = this lane is the lower one of its pair and keeps the smaller key
template <bool PACKED, int CTRL>
__device__ __forceinline__ void sort_layer(uint32_t& key, uint32_t& len, bool low)
{
    const uint32_t pk = row_partner<CTRL>(key);
    if constexpr (PACKED) {
        key = low ? min(key, pk) : max(key, pk);
    } else {
        const uint32_t pl = row_partner<CTRL>(len);
        const bool take = (pk < key) != !low;          // (equal keys carry equal lengths: taking the partner's changes nothing)
        key = take ? pk : key;
        len = take ? pl : len;
    }
}
template <bool PACKED>
__device__ __forceinline__ void row_sort16(uint32_t& key, uint32_t& len, bool low1, bool low2, bool low4, bool low8)
{
    sort_layer<PACKED, DPP_XOR1>(key, len, low1);
    sort_layer<PACKED, DPP_XOR3>(key, len, low2);  sort_layer<PACKED, DPP_XOR1>(key, len, low1);
    sort_layer<PACKED, DPP_XOR7>(key, len, low4);  sort_layer<PACKED, DPP_XOR2>(key, len, low2);
    sort_layer<PACKED, DPP_XOR1>(key, len, low1);
    sort_layer<PACKED, DPP_XOR15>(key, len, low8); sort_layer<PACKED, DPP_XOR4>(key, len, low4);
    sort_layer<PACKED, DPP_XOR2>(key, len, low2);  sort_layer<PACKED, DPP_XOR1>(key, len, low1);
}

// PACKED = the list format (a.list_packed): it only decides the sort key and the stores
template <bool PACKED>
__global__ __launch_bounds__(64) void k_find_sn(xzamd_span_args a, SnArgs sn, uint16_t* __restrict__ mlen,
        uint32_t* __restrict__ mdist)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t t = lane & 15, row = lane >> 4;
    uint32_t run = blockIdx.x;
    if (sn.mode == 1) {
        const uint32_t b = blockIdx.x / SEED_RUNS, j = blockIdx.x - b * SEED_RUNS;
        const uint32_t bs = b * a.block_size;
        run = bs / FIND_RUN + j;
        if ((uint64_t)run * FIND_RUN >= (uint64_t)bs + XZAMD_SEED_LEN || (uint64_t)run * FIND_RUN >= a.n) return;
    } else if (sn.mode == 2) {
        // a run belongs to launch 1 when it starts inside the seed region of its Block or reaches into the next Block
        const uint32_t x0 = run * FIND_RUN;
        const uint32_t b = x0 / a.block_size, bs = b * a.block_size;
        const uint64_t be = (uint64_t)bs + a.block_size;
        if (x0 < bs + XZAMD_SEED_LEN || ((uint64_t)x0 + FIND_RUN > be && be < a.n)) return;
    }
    const uint32_t xr0 = run * FIND_RUN + row * ROW_RUN;                 // first position of this row
    const uint8_t* __restrict__ in = sn.in;
    const uint32_t W = a.sa_window;
    const uint32_t cyclic = a.dict_size + 1;
    const uint32_t nice = a.nice_len;
    const uint32_t n = a.n;
    // lane roles
    const bool left = t < 5, right = t >= 5 && t < 10;
    const uint32_t k = left ? t : t - 5;
    const bool win_lane = (left || right) && k < W;
    // hash2 / hash4 heads and the 8- / 16-byte left neighbours.  (A hash3 head, lane 11, was measured to be worth
    // nothing on text and 0.1 % on executables next to these: its sort and inversion are not built for this finder.)
    // Lanes 11 / 15: the nearest earlier position with the same 24 / 32 bytes (by-products of the suffix-order rounds):
    // between "same 16 bytes" and the suffix-order neighbours (which share the LONGEST prefixes, at any distance) these
    // are the near candidates of medium length BT4's descent finds (measured through the oracle: -0.6 points of size on
    // a SQLite file, -0.45 on C headers, -0.9 at 9e).
    const bool hash_lane = t >= 10;
    const uint32_t* __restrict__ hp = t == 10 ? sn.prev2 : t == 11 ? sn.prev24 : t == 12 ? sn.prev4 : t == 13 ? sn.prev8
            : t == 14 ? sn.prev16 : sn.prev32;
    const uint32_t minlen = t == 10 ? 2u : 4u;
    // the row sort: is this lane the lower one of a pair 1 / 2 / 4 / 8 lanes apart; the lanes below it inside the row
    const bool low1 = !(t & 1), low2 = !(t & 2), low4 = !(t & 4), low8 = !(t & 8);
    const uint32_t below = (1u << t) - 1;
    // masks for the prefix maximum inside a side (the right side must not look into the left one)
    const bool sh1 = t != 0 && t != 5, sh2 = (left && t >= 2) || (right && t >= 7), sh4 = (left && t >= 4) || (right && t >= 9);

    // geometry of the row's current position (per lane, equal inside a row): Block start / end.  The records are
    // span independent (a match may run to the Block end): the spans are cut from these lists afterwards
    // (k_span_est / k_span_cut) and the parser clamps what it reads to its span (round_lists).
    uint32_t g_bs, g_be;
    {
        const uint32_t p = xr0 < n ? xr0 : 0u;
        const uint32_t blk = p / a.block_size;
        g_bs = blk * a.block_size;
        g_be = min(n, g_bs + a.block_size);
    }
    auto geo_next = [&](uint32_t& bs, uint32_t& be, uint32_t p) {      // (bs, be) of p - 1 -> of p
        const bool nb = p >= be;
        bs = nb ? be : bs;
        be = nb ? min(n, be + a.block_size) : be;
    };
    auto clampp = [&](uint32_t p) -> uint32_t { return p < n ? p : n - 1; };
    // neighbour of this lane for position p with rank r inside Block [bs, be)
    auto window = [&](uint32_t r, uint32_t bs, uint32_t be, bool live) -> uint32_t {
        const int32_t slot = right ? (int32_t)(r + 1 + k) : (int32_t)r - 1 - (int32_t)k;
        const bool inb = live && win_lane && slot >= (int32_t)bs && slot < (int32_t)be;
        return inb ? sn.sa[slot] : SN_NONE;
    };
    auto candidate = [&](uint32_t p, uint32_t wq, uint32_t hw, uint32_t& q, bool& valid) {
        const bool elig = wq != SN_NONE && wq < p && p - wq < cyclic;
        const uint32_t v = elig ? wq + 1 : 0u;
        uint32_t pm = v;
        { const uint32_t o = row_shr<1>(pm); pm = max(pm, sh1 ? o : 0u); }
        { const uint32_t o = row_shr<2>(pm); pm = max(pm, sh2 ? o : 0u); }
        { const uint32_t o = row_shr<4>(pm); pm = max(pm, sh4 ? o : 0u); }
        const uint32_t o1 = row_shr<1>(pm);
        const uint32_t ex = sh1 ? o1 : 0u;
        valid = elig && v > ex;
        q = elig ? wq : 0u;
        // The six hash / prefix lanes often name the same position (the nearest earlier position with the same 8 bytes is
        // usually also the one with the same 16, 24, 32): the candidate stays in the lowest of those lanes only -- which is
        // the one the Pareto rule below would keep -- and the others do not fetch its bytes again.  (hw is 0 in the
        // window lanes; computed by every lane so that the row shifts see all their source lanes.)
        bool dup = false;
        { const uint32_t o = row_shr<1>(hw); dup = dup || (t >= 11 && o == hw); }
        { const uint32_t o = row_shr<2>(hw); dup = dup || (t >= 12 && o == hw); }
        { const uint32_t o = row_shr<3>(hw); dup = dup || (t >= 13 && o == hw); }
        { const uint32_t o = row_shr<4>(hw); dup = dup || (t >= 14 && o == hw); }
        { const uint32_t o = row_shr<5>(hw); dup = dup || (t >= 15 && o == hw); }
        if (hash_lane) {
            valid = hw != 0 && hw < cyclic && hw <= p && !dup;
            q = valid ? p - hw : 0u;
        }
    };
    auto load16 = [&](uint32_t off) -> uint4 {
        uint4 v;
        __builtin_memcpy(&v, in + off, 16);
        return v;
    };

    // ---- prologue: positions i = 0, 1, 2 of the row
    const uint32_t xend = min(n, xr0 + ROW_RUN);                          // this row's positions: [xr0, xend)
    uint32_t g1_bs = g_bs, g1_be = g_be;                                  // geometry of x + 1
    geo_next(g1_bs, g1_be, xr0 + 1);
    uint32_t g2_bs = g1_bs, g2_be = g1_be;                                // geometry of x + 2
    geo_next(g2_bs, g2_be, xr0 + 2);
    uint32_t rk1 = sn.sa_rank[clampp(xr0 + 1)];
    uint32_t rk2 = sn.sa_rank[clampp(xr0 + 2)];
    uint32_t hw1 = hash_lane ? hp[clampp(xr0 + 1)] : 0u;
    uint32_t w1 = window(rk1, g1_bs, g1_be, xr0 + 1 < xend);
    uint32_t q0; bool v0;
    {
        const uint32_t rk0 = sn.sa_rank[clampp(xr0)];
        const uint32_t hw0 = hash_lane ? hp[clampp(xr0)] : 0u;
        candidate(xr0, window(rk0, g_bs, g_be, xr0 < xend), hw0, q0, v0);
        if (!(xr0 < xend)) v0 = false;
    }
    bool pf0 = xr0 + 16 <= n;
    uint4 A0 = make_uint4(0, 0, 0, 0), B0 = A0;
    if (pf0) { A0 = load16(q0); B0 = load16(xr0); }

    uint32_t macc = 0;
    uint32_t i = 0;
    for (; i < ROW_RUN; ++i) {
        const uint32_t x = xr0 + i;
        if (__builtin_amdgcn_readfirstlane((int)(blockIdx.x * FIND_RUN + i)) >= (int)n) break;   // every row is past the end
        // stage 0: window of x + 2 (its rank arrived last iteration), rank of x + 3, hash word of x + 2
        const uint32_t w2 = window(rk2, g2_bs, g2_be, x + 2 < xend);
        const uint32_t rk3 = sn.sa_rank[clampp(x + 3)];
        const uint32_t hw2 = hash_lane ? hp[clampp(x + 2)] : 0u;
        // stage 1: candidates of x + 1 and their first 16 bytes
        uint32_t q1; bool v1;
        candidate(x + 1, w1, hw1, q1, v1);
        if (!(x + 1 < xend)) { v1 = false; q1 = 0; }
        const bool pf1 = x + 1 + 16 <= n;
        uint4 A1 = A0, B1 = B0;
        if (pf1) { A1 = load16(q1); B1 = load16(x + 1); }
        // stage 2: position x
        uint32_t mval = 0;                                  // this position's 16-bit summary for the span plan (top lane)
        if (x < xend) {
            const bool valid = v0;
            const uint32_t avail = g_be - x;
            const uint32_t buf_avail = avail < MATCH_LEN_MAX ? avail : MATCH_LEN_MAX;
            const uint32_t len_limit = nice <= avail ? nice : avail;
            const bool mf_ok = nice <= avail || avail >= 4;    // "pending": nothing is reported (lz_encoder_mf.c:190-201)
            const uint64_t rec_base = (uint64_t)x * LIST_W;
            const uint32_t lim = (valid && mf_ok) ? len_limit : 0u;
            uint32_t L;
            if (pf0) {
                const uint32_t m = match16(A0, B0);
                L = m < lim ? m : lim;
                if (m == 16 && lim > 16) L = lane_cmplen16_from(in, q0, x, 16, lim);
            } else {
                L = lane_cmplen16_from(in, q0, x, 0, lim);
            }
            const bool ok = lim != 0 && L >= minlen;
            // sort the row's candidates by distance (see row_sort16): from here on a lane holds the entry of its RANK, not
            // the candidate it fetched
            uint32_t skey, slen;
            if constexpr (PACKED) {
                skey = ok ? ((x - q0 - 1) << 9) | L : SORT_NONE;
                slen = 0;
            } else {
                skey = ok ? x - q0 - 1 : SN_NONE;
                slen = ok ? L : 0u;
            }
            row_sort16<PACKED>(skey, slen, low1, low2, low4, low8);
            if constexpr (PACKED) slen = skey & 0x1FFu;
            L = slen;                                           // 0 in the lanes behind the candidates
            const uint32_t dist = (PACKED ? skey >> 9 : skey) + 1;
            const uint32_t q = x - dist;
            // Pareto set: a candidate stays when it is longer than every nearer one (the same position twice: equal
            // keys, the second one goes)
            uint32_t pm = L;
            pm = max(pm, row_shr<1>(pm)); pm = max(pm, row_shr<2>(pm)); pm = max(pm, row_shr<4>(pm)); pm = max(pm, row_shr<8>(pm));
            const bool keep = L > row_shr<1>(pm);
            // index among the kept entries in distance (= length) order, and their number
            const uint32_t kept = (uint32_t)(__ballot(keep) >> (lane & 48)) & 0xFFFFu;
            const uint32_t cnt = (uint32_t)__builtin_popcount(kept);
            const uint32_t kidx = (uint32_t)__builtin_popcount(kept & below);
            const bool top = keep && kidx + 1 == cnt, second = keep && kidx + 2 == cnt;
            uint32_t len_out = L;
            if (top && L == nice) len_out = lane_cmplen16_from(in, q, x, L, buf_avail);      // > nice_len extension
            // rep0 run behind the byte after the match, for the two longest entries
            uint32_t l2 = 0;
            if ((top || second) && len_out + 1 < avail) {
                const uint32_t lim2 = min(avail, len_out + 1 + LEN2_MAX);
                l2 = lane_cmplen16_from(in, q, x, len_out + 1, lim2) - (len_out + 1);
            }
            const uint32_t drop = cnt > LIST_K ? cnt - LIST_K : 0;
            if (keep && kidx >= drop) {
                const uint64_t o = rec_base + (kidx - drop);
                if constexpr (PACKED) {
                    mdist[o] = (len_out << 23) | (dist - 1);
                } else {
                    mlen[o] = (uint16_t)len_out;
                    mdist[o] = dist - 1;
                }
            }
            // trailer: count | len2(longest) << 8 | len2(second) << 16, written bytewise by the lanes that know
            uint8_t* tr = reinterpret_cast<uint8_t*>(mdist + rec_base + LIST_K);
            if (cnt == 0) {
                if (t == 0) mdist[rec_base + LIST_K] = 0;
            } else {
                if (top) {
                    *reinterpret_cast<uint16_t*>(tr) = (uint16_t)((cnt - drop) | (l2 << 8));
                    tr[3] = 0;
                    if (cnt == 1) tr[2] = 0;
                    // what the span plan's walk needs of this position (k_span_est), 2 bytes instead of the 32-byte record
                    mval = len_out | ((dist > 1 ? 32u - (uint32_t)__builtin_clz(dist - 1) : 0u) << 9);
                }
                if (second) tr[2] = (uint8_t)l2;
            }
        }
        // the summaries of 16 consecutive positions of a row are collected in its 16 lanes and stored together
        // (a 2-byte store per position from one lane per row costs as much as the whole 32-byte record)
        {
            uint32_t rv = mval;
            rv |= row_ror<1>(rv); rv |= row_ror<2>(rv); rv |= row_ror<4>(rv); rv |= row_ror<8>(rv);
            macc = t == (i & 15u) ? rv : macc;
            if ((i & 15u) == 15u) {
                const uint32_t px = xr0 + (i & ~15u) + t;
                if (px < xend) a.mtop[px] = (uint16_t)macc;
            }
        }
        // shift the pipeline
        q0 = q1; v0 = v1; pf0 = pf1; A0 = A1; B0 = B1;
        w1 = w2; hw1 = hw2;
        rk2 = rk3;
        g_bs = g1_bs; g_be = g1_be;
        g1_bs = g2_bs; g1_be = g2_be;
        geo_next(g2_bs, g2_be, x + 3);
    }
    if (i & 15u) {                                          // the loop ended inside a group of 16 (end of the batch)
        const uint32_t px = xr0 + (i & ~15u) + t;
        if (t < (i & 15u) && px < xend) a.mtop[px] = (uint16_t)macc;
    }
}

// ------------------------------------------------------------------------------------------
// Cost-balanced spans (oracle: est_chunk / plan_spans).  A wavefront needs one step per position the optimal
// parser visits, and positions covered by a match of nice_len bytes or more are not visited; a state reset costs a
// few hundred bytes of model learning whatever the data.  So spans are cut by estimated parser work instead of
// input bytes: the spans of a launch take about equally long whatever they hold, and highly compressible data
// gets the long spans its small output needs.
//   k_span_est   one thread per chunk of XZAMD_EST_CHUNK positions: a walk over the match lists.  A position whose
//                longest match reaches nice_len costs EST_LONG units and the walk jumps over the match, any other
//                position one unit; alongside, a greedy-parse estimate of the coded size in bits.
//   k_span_cut   one wavefront per Block: k = max(1, work of the Block / target) spans of equal estimated work.
// ------------------------------------------------------------------------------------------
constexpr uint32_t EST_LONG = 4;

__global__ __launch_bounds__(256) void k_span_est(xzamd_span_args a, uint32_t nblocks, uint32_t cpb,
        uint32_t* __restrict__ est, unsigned long long* __restrict__ totals)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nch = nblocks * cpb;
    if (t >= nch) return;
    const uint32_t b = t / cpb, c = t - b * cpb;
    const uint32_t bs = b * a.block_size;
    const uint32_t be = min(a.n, bs + a.block_size);
    const uint64_t c0_ = (uint64_t)bs + (uint64_t)c * XZAMD_EST_CHUNK;
    uint32_t w = 0, bits = 0;
    if (c0_ < be) {
        const uint32_t c0 = (uint32_t)c0_;
        const uint32_t c1 = be - c0 < XZAMD_EST_CHUNK ? be : c0 + XZAMD_EST_CHUNK;
        uint32_t x = c0, gnext = c0;
        uint32_t cb = 0xFFFFFFFFu;                       // eight summaries at a time (16 bytes) through registers
        uint4 buf = make_uint4(0, 0, 0, 0);
        while (x < c1) {
            const uint32_t base = x & ~7u;
            if (base != cb) { buf = *reinterpret_cast<const uint4*>(a.mtop + base); cb = base; }
            const uint32_t k = x & 7u;
            const uint32_t wv = k < 2 ? buf.x : k < 4 ? buf.y : k < 6 ? buf.z : buf.w;
            const uint32_t v = (k & 1u) ? wv >> 16 : wv & 0xFFFFu;
            const uint32_t len = v & 0x1FFu, bl = v >> 9;          // bl <= 7 <=> zero-based distance < 128
            if (x >= gnext) {
                if (len >= 3 || (len == 2 && bl <= 7)) {
                    bits += 14 + bl;
                    gnext = x + len;
                } else {
                    bits += 6;
                    gnext = x + 1;
                }
            }
            if (len >= a.nice_len) { w += EST_LONG; x += len; }
            else { w += 1; x += 1; }
        }
        atomicAdd(&totals[b], (unsigned long long)w);
        atomicAdd(&totals[nblocks], (unsigned long long)w);
    }
    est[t] = w;
    est[nch + t] = bits;
}

__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v)
{
    const uint32_t lane = threadIdx.x;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t o = __shfl_up(v, s);
        if (lane >= (uint32_t)s) v += o;
    }
    return v;
}

__global__ __launch_bounds__(64) void k_span_cut(xzamd_span_args a, uint32_t nblocks, uint32_t cpb,
        const uint32_t* __restrict__ est, unsigned long long* __restrict__ totals, uint32_t* __restrict__ span_tab,
        uint32_t* __restrict__ span_cnt, uint32_t cost_min, uint32_t bits_min, uint32_t min_len,
        uint32_t* __restrict__ enc_tab, uint32_t* __restrict__ enc_cnt, uint32_t* __restrict__ span_key)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t b = blockIdx.x;
    const uint32_t nch = nblocks * cpb;
    const uint32_t bs = b * a.block_size;
    const uint32_t be = min(a.n, bs + a.block_size);
    const uint32_t m = (be - bs + XZAMD_EST_CHUNK - 1) / XZAMD_EST_CHUNK;      // chunks of this Block
    // Work target of a span: cost_min, whatever the batch or the GPU -- the plan (and with it the output) of a Block is
    // a function of the Block and the options alone.
    const unsigned long long T = cost_min;
    if (b == 0 && lane == 0) totals[nblocks + 1] = T;
    const uint32_t* wk = est + (uint64_t)b * cpb;
    const uint32_t* bt = est + nch + (uint64_t)b * cpb;
    // two-phase: the first XZAMD_SEED_LEN bytes are the seed piece and the plan covers the rest
    const bool two = a.enc_bits != 0;
    const uint32_t seed_chunks = two && be - bs > XZAMD_SEED_LEN ? XZAMD_SEED_LEN / XZAMD_EST_CHUNK : 0u;
    // spans of this Block: total / T of equal estimated work, but no more than its estimated coded size allows at
    // bits_min per span (highly compressible Blocks get fewer, longer spans)
    unsigned long long total = 0, total_bits = 0, all_bits = 0;
    for (uint32_t c0 = 0; c0 < m; c0 += 64) {
        const uint32_t c = c0 + lane;
        const uint32_t vb = c < m ? bt[c] : 0u, vw = c < m ? wk[c] : 0u;
        const bool planned = c >= seed_chunks;
        all_bits += lane_of(wave_incl_sum(vb), 63);
        total_bits += lane_of(wave_incl_sum(planned ? vb : 0u), 63);
        total += lane_of(wave_incl_sum(planned ? vw : 0u), 63);
    }
    unsigned long long k = total / T;
    if (bits_min) {
        // (round 5's growth of bits_min on highly compressible Blocks is gone: oracle plan_spans_ex)
        const unsigned long long kb = total_bits / (unsigned long long)bits_min;
        if (kb < k) k = kb;
    }
    if (k == 0) k = 1;
    const unsigned long long Tb = (total + k - 1) / k;
    // encode spans (two-phase): ke of about equal estimated coded size, each closed at a piece end
    unsigned long long ke = two ? all_bits / a.enc_bits : 1ull;
    if (ke > (be - bs) / XZAMD_ENC_MIN_LEN) ke = (be - bs) / XZAMD_ENC_MIN_LEN;
    if (ke == 0) ke = 1;
    const unsigned long long Eb = (all_bits + ke - 1) / ke;
    uint32_t* tab = span_tab + 2ull * b * a.max_spb;
    uint32_t* etab = two ? enc_tab + 2ull * b * a.max_esb : nullptr;
    uint32_t ns = 1, start = 0;                       // spans so far, first chunk of the open span
    uint32_t ne = 1, estart = 0;                      // encode spans so far, first chunk of the open one
    unsigned long long carry_w = 0;                   // estimated work of the open span in front of the window
    unsigned long long carry_b = 0;                   // estimated bits of the open encode span in front of the window
    if (lane == 0) { tab[0] = bs; if (two) etab[0] = bs; }
    for (uint32_t c0 = 0; c0 < m; c0 += 64) {
        const uint32_t c = c0 + lane;
        const uint32_t pw = wave_incl_sum(c < m ? wk[c] : 0u);
        const uint32_t pb = two ? wave_incl_sum(c < m ? bt[c] : 0u) : 0u;
        uint32_t subw = 0;                            // window sum up to the last cut inside the window
        uint32_t subb = 0;                            // the same for the bits, up to the last encode cut
        for (;;) {
            const unsigned long long accw = carry_w + (pw - subw);
            const unsigned long long len = (unsigned long long)(c + 1 - start) * XZAMD_EST_CHUNK;
            const bool cut = c + 1 < m && c >= start && ns < a.max_spb
                    && (len >= XZAMD_SPAN_MAX || (accw >= Tb && len >= min_len) || c + 1 == seed_chunks);
            const uint64_t mask = __builtin_amdgcn_ballot_w64(cut);
            if (!mask) break;
            const uint32_t L = (uint32_t)__builtin_ctzll(mask);
            start = c0 + L + 1;
            const unsigned long long closed = carry_w + (lane_of(pw, L) - subw);      // estimated work of the span just closed
            subw = lane_of(pw, L);
            carry_w = 0;
            const uint32_t p = bs + start * XZAMD_EST_CHUNK;
            if (lane == 0) {
                tab[2 * ns - 1] = p;                  // end of the span just closed
                tab[2 * ns] = p;
                // launch-order key: heaviest first (ascending sort of ~work); unused slots keep 0xFFFFFFFF = last
                span_key[(uint64_t)b * a.max_spb + ns - 1] = ~(uint32_t)min(closed ? closed : 1ull, 0xFFFFFFFEull);
            }
            ++ns;
            if (two) {
                const unsigned long long accb = carry_b + (lane_of(pb, L) - subb);
                if (accb >= Eb && (unsigned long long)(start - estart) * XZAMD_EST_CHUNK >= XZAMD_ENC_MIN_LEN && ne < a.max_esb) {
                    if (lane == 0) { etab[2 * ne - 1] = p; etab[2 * ne] = p; }
                    ++ne;
                    estart = start;
                    subb = lane_of(pb, L);
                    carry_b = 0;
                }
            }
        }
        carry_w += lane_of(pw, 63) - subw;
        carry_b += lane_of(pb, 63) - subb;
    }
    if (lane == 0) {
        tab[2 * ns - 1] = be;
        span_cnt[b] = ns;
        span_key[(uint64_t)b * a.max_spb + ns - 1] = ~(uint32_t)min(carry_w ? carry_w : 1ull, 0xFFFFFFFEull);
        if (two) { etab[2 * ne - 1] = be; enc_cnt[b] = ne; }
    }
}

// Where the first part of every piece ends (oracle: part_end_of): behind the 4 KiB chunk at which an eighth of the piece's
// estimated work has been seen, at least XZAMD_PART_MIN bytes; the seed piece's part is the whole of it.  One thread per piece slot.
__global__ __launch_bounds__(256) void k_part_ends(xzamd_span_args a, uint32_t nblocks, uint32_t cpb, const uint32_t* __restrict__ est,
        uint32_t* __restrict__ part_tab)
{
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= nblocks * a.max_spb) return;
    const uint32_t blk = slot / a.max_spb, k = slot - blk * a.max_spb;
    if (k >= a.span_cnt[blk]) return;
    const uint32_t bs = blk * a.block_size;
    const uint32_t s0 = a.span_tab[2 * slot], pe = a.span_tab[2 * slot + 1];
    uint32_t end = pe;
    if (k != 0 && pe - s0 > XZAMD_PART_MIN) {
        const uint32_t* wk = est + (uint64_t)blk * cpb;
        const uint32_t c0 = (s0 - bs) / XZAMD_EST_CHUNK, c1 = (pe - bs + XZAMD_EST_CHUNK - 1) / XZAMD_EST_CHUNK;
        unsigned long long total = 0, acc = 0;
        for (uint32_t c = c0; c < c1; ++c) total += wk[c];
        const unsigned long long target = (total + 7) / 8;
        for (uint32_t c = c0; c < c1; ++c) {             // the chunk boundary nearest to where the eighth is reached
            const uint64_t b64 = (uint64_t)bs + (uint64_t)c * XZAMD_EST_CHUNK;
            if (acc + wk[c] / 2 >= target && b64 >= (uint64_t)s0 + XZAMD_PART_MIN) { end = (uint32_t)b64; break; }
            acc += wk[c];
        }
    }
    part_tab[slot] = end;
}

// Exact HC3/HC4 finder in list form (optimal parser over the reference's match finder; test
// configuration).  Same record layout, len2 = 0.
__global__ __launch_bounds__(64) void k_find_exact(xzamd_span_args a, uint16_t* __restrict__ mlen,
        uint32_t* __restrict__ mdist)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t x0 = blockIdx.x * FIND_RUN;
    if (x0 >= a.n) return;
    const uint32_t x1 = min(a.n, x0 + FIND_RUN);
    Env e;
    e.in = a.in; e.rank = a.rank; e.sorted_pos = a.sorted_pos; e.prev2 = a.prev2; e.prev3 = a.prev3;
    e.nice = a.nice_len; e.depth = a.depth; e.hb = a.hash_bytes; e.cyclic = a.dict_size + 1;
    e.block_end = 0; e.n_last = a.n - 1;
    e.mlen = nullptr; e.mdist = nullptr; e.packed = a.list_packed;
    Pre P;
    P.valid = false; P.pos = 0; P.ent = 0;
    P.a.rk = P.a.d2 = P.a.d3 = 0; P.an = P.a;
    uint32_t span_end = 0;
    for (uint32_t x = x0; x < x1; ++x) {
        if (x >= span_end) {
            const uint32_t blk = x / a.block_size;
            const uint32_t block_start = blk * a.block_size;
            const uint32_t block_end = min(a.n, block_start + a.block_size);
            const uint64_t k = (x - block_start) / a.span_size;
            const uint64_t se = (uint64_t)block_start + (k + 1) * a.span_size;
            span_end = se < block_end ? (uint32_t)se : block_end;
            e.block_end = block_end;
        }
        Round R;
        do_round<false>(e, P, x, span_end, 0, 0, 0, 0, R);
        const uint64_t lt = (1ull << lane) - 1;
        const bool rec = (R.mask >> lane) & 1;
        const uint32_t idx = (uint32_t)__builtin_popcountll(R.mask & lt);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(R.mask);
        const uint32_t drop = cnt > LIST_K ? cnt - LIST_K : 0;
        const uint64_t rec_base = (uint64_t)x * LIST_W;
        if (rec && idx >= drop) {
            const uint32_t len = idx + 1 == cnt ? R.longest : R.L;
            const uint64_t o = rec_base + (idx - drop);
            if (e.packed) {
                mdist[o] = (len << 23) | R.D;
            } else {
                mlen[o] = (uint16_t)len;
                mdist[o] = R.D;
            }
        }
        if (lane == 0) mdist[rec_base + LIST_K] = cnt - drop;
    }
}

} // namespace

extern "C" {

int xzk_find_matches(const xzamd_span_args* a, const uint32_t* sa, const uint32_t* sa_rank, const uint32_t* prev4,
        const uint64_t* rp8, const uint64_t* rp16, const uint32_t* prev24, const uint32_t* prev32,
        uint16_t* mlen, uint32_t* mdist, int part, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    const uint32_t runs = (a->n + FIND_RUN - 1) / FIND_RUN;
    if (runs == 0) return 0;
    if (a->sa_window) {
        if (!sa || !sa_rank || !prev4 || !rp8 || !rp16 || !prev24 || !prev32 || !a->mtop || a->sa_window > SN_WMAX)
            return (int)hipErrorInvalidValue;
        if (part != 0 && a->block_size < XZAMD_SEED_LEN + 2 * FIND_RUN) return (int)hipErrorInvalidValue;
        SnArgs sn;
        sn.in = a->in; sn.sa = sa; sn.sa_rank = sa_rank; sn.prev2 = a->prev2; sn.prev4 = prev4;
        sn.prev8 = reinterpret_cast<const uint32_t*>(rp8) + a->n;     // second array of the round's (rank, distance) pair
        sn.prev16 = reinterpret_cast<const uint32_t*>(rp16) + a->n;
        sn.prev24 = prev24; sn.prev32 = prev32;
        sn.mode = (uint32_t)part;
        const uint32_t nblocks = (a->n + a->block_size - 1) / a->block_size;
        const dim3 grid(part == 1 ? nblocks * SEED_RUNS : runs);
        if (a->list_packed) hipLaunchKernelGGL(k_find_sn<true>, grid, dim3(64), 0, st, *a, sn, mlen, mdist);
        else hipLaunchKernelGGL(k_find_sn<false>, grid, dim3(64), 0, st, *a, sn, mlen, mdist);
    } else {
        hipLaunchKernelGGL(k_find_exact, dim3(runs), dim3(64), 0, st, *a, mlen, mdist);
    }
    return (int)hipGetLastError();
}

int xzk_span_plan(const xzamd_span_args* a, uint32_t nblocks, uint32_t* est, unsigned long long* totals,
        uint32_t* span_tab, uint32_t* span_cnt, uint32_t cost_min, uint32_t bits_min, uint32_t min_len,
        uint32_t* enc_tab, uint32_t* enc_cnt,
        uint32_t* order_bufs, void* sort_tmp, uint64_t sort_tmp_bytes, uint32_t** order_out, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (order_out) *order_out = nullptr;
    if (nblocks == 0 || a->n == 0) return 0;
    if (!a->mtop || a->max_spb == 0 || cost_min == 0 || !order_bufs || !order_out) return (int)hipErrorInvalidValue;
    if (a->enc_bits && (!enc_tab || !enc_cnt || a->max_esb == 0 || min_len < XZAMD_SEED_LEN)) return (int)hipErrorInvalidValue;
    const uint32_t cpb = (a->block_size + XZAMD_EST_CHUNK - 1) / XZAMD_EST_CHUNK;
    const uint32_t nslots = nblocks * a->max_spb;
    uint32_t* key_a = order_bufs;
    uint32_t* key_b = order_bufs + nslots;
    uint32_t* val_a = order_bufs + 2ull * nslots;
    uint32_t* val_b = order_bufs + 3ull * nslots;
    hipError_t e = hipMemsetAsync(totals, 0, (size_t)(nblocks + 2) * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(key_a, 0xFF, (size_t)nslots * 4, st);
    if (e != hipSuccess) return (int)e;
    const uint64_t nch = (uint64_t)nblocks * cpb;
    hipLaunchKernelGGL(k_span_est, dim3((uint32_t)((nch + 255) / 256)), dim3(256), 0, st, *a, nblocks, cpb, est, totals);
    hipLaunchKernelGGL(k_span_cut, dim3(nblocks), dim3(64), 0, st, *a, nblocks, cpb, est, totals, span_tab, span_cnt,
            cost_min, bits_min, min_len, enc_tab, enc_cnt, key_a);
    if (a->part_tab) {
        xzamd_span_args a2 = *a;
        a2.span_tab = span_tab; a2.span_cnt = span_cnt;
        hipLaunchKernelGGL(k_part_ends, dim3((nslots + 255) / 256), dim3(256), 0, st, a2, nblocks, cpb, est, a->part_tab);
    }
    // launch order: span slots by estimated work, heaviest first (a launch then ends with its short spans instead of
    // waiting for a heavy one that happened to start late); the order does not change a byte of the output
    e = sort_launch_order(key_a, key_b, val_a, val_b, nslots, sort_tmp, (size_t)sort_tmp_bytes, order_out, st);
    if (e != hipSuccess) return (int)e;
    return (int)hipGetLastError();
}

} // extern "C"
