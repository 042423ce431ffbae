// lzma_kernels.hip -- MI355X (gfx950 / CDNA4) device side of the LZMA2 Block encoder: the parse and encode kernels.
//
// The encoder replaces, for a whole batch of .xz Blocks resident in HBM, what one worker
// thread of the reference runs per Block (stream_encoder_mt.c:219-298).  Stage by stage, with the unit each lives in:
//
//   lz/lz_encoder_mf.c      HC3/HC4 match finder      -> k_h2_* / k_hash_keys + radix sort + k_link_*         lzma_build.hip
//                                                       (Block-global "sorted bucket" chains)
//                                                       + wave-parallel candidate evaluation (do_round)      match_common.h
//                                                       for every position (k_find_exact)                    lzma_find.hip
//   lz/lz_encoder_mf.c      BT4 (presets 4-9)         -> suffix-neighbourhood finder: k_sa_* (suffix order of every
//                                                       Block by radix sorts + rank doubling)                lzma_build.hip
//                                                       k_find_sn; span plan k_span_est / k_span_cut         lzma_find.hip
//   lzma/lzma_encoder_optimum_fast.c    parser        -> fast parser block of span_encode_one (wave-uniform)  here
//   lzma/lzma_encoder_optimum_normal.c  parser        -> optimum_window() (windowed DP, lane = length / candidate)  here
//   lzma/lzma_encoder.c     symbol coder               -> encode_symbol()                                      here
//   rangecoder/range_encoder.h  range coder            -> struct RC                                            here
//   lzma/lzma2_encoder.c    chunk framing              -> span_encode_one epilogue                             here
//   simple/*.c, delta/      filters in front of LZMA2  -> k_x86_bcj, k_riscv_bcj, k_arm64_bcj, k_bcj_simple, k_delta  lzma_filters.hip
//   check/crc64_fast.c, crc32, sha256.c                -> k_crc_strips / k_crc_fold, k_sha256_blocks           lzma_filters.hip
//   block_encoder.c / stream_encoder_mt.c assembly     -> k_assemble (gather of span outputs)                  here
//   (HIP runtime calls of the plain-C host layer)      -> xzk_malloc ... xzk_mem_info                          hip_shims.hip
//
// Design: the sequential insert-then-search structures of the
// reference are replaced by parse-independent ones built in parallel.  Hash
// chains: every position's masked hash is radix-sorted (key = block<<hash_bits
// | hash, stable, so positions ascend inside a bucket); the `depth` slots before
// a position's slot ARE the hash chain the reference would walk (same candidates,
// same order, collisions included), so one coalesced read fetches the whole
// chain and 64 lanes evaluate all candidates at once.  BT4's tree is the
// Cartesian tree of (suffix order, insertion time): its search path is the set
// of recency records around a position in suffix order, which a sort provides.
// Nothing is scattered: whatever a sort produces is brought back to position
// order by two radix passes and one LDS step (invert_perm).  The LZMA state
// machine + range coder is serial by construction; parallelism there comes from
// cutting each Block into spans that are entropy-coded independently (LZMA2
// state-reset chunks), one wavefront per span, probability model in LDS.
//
// No MFMA: there is no dense contraction anywhere on this path.

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <stdint.h>
#include "kernels_api.h"
#include "wave.h"
#include "match_common.h"

namespace {

constexpr uint32_t LITERAL = 0xFFFFFFFFu;
constexpr uint32_t NO_DELTA = 0xFFFFFFFFu;

// Probability model layout (u16 each), 7990 entries at lc+lp<=... we size for lc+lp <= 3
// (8 literal coders = 6144) which covers every preset (lc=3, lp=0).  Same order as the oracle.
enum : uint32_t {
    P_IS_MATCH = 0,
    P_IS_REP = P_IS_MATCH + 12 * 16,
    P_IS_REP0 = P_IS_REP + 12,
    P_IS_REP1 = P_IS_REP0 + 12,
    P_IS_REP2 = P_IS_REP1 + 12,
    P_IS_REP0_LONG = P_IS_REP2 + 12,
    P_DIST_SLOT = P_IS_REP0_LONG + 12 * 16,
    P_DIST_SPECIAL = P_DIST_SLOT + 4 * 64,
    P_DIST_ALIGN = P_DIST_SPECIAL + 114,
    P_MATCH_LEN = P_DIST_ALIGN + 16,
    LEN_CHOICE = 0, LEN_CHOICE2 = 1, LEN_LOW = 2, LEN_MID = 2 + 16 * 8, LEN_HIGH = 2 + 32 * 8,
    LEN_CODER_SIZE = 2 + 32 * 8 + 256,
    P_REP_LEN = P_MATCH_LEN + LEN_CODER_SIZE,
    P_LITERAL = P_REP_LEN + LEN_CODER_SIZE,       // 1846
    P_TOTAL = P_LITERAL + (0x300 << 3)            // 7990
};
static_assert(P_TOTAL <= 8192, "model must fit the 16 KiB LDS slice");

// ------------------------------------------------------------------------------------------
// Range coder (rangecoder/range_encoder.h:136-263), coding directly instead of queueing.
// All members are wave-uniform.
// ------------------------------------------------------------------------------------------
struct RC {
    uint64_t low;
    uint32_t range;
    uint32_t cache_size;
    uint32_t cache;
    uint32_t cpos;      // payload bytes written for the current chunk
    uint8_t* out;       // payload base of the current chunk
    // token sink of the two-phase model pass (rc_emit<.., TOK>): the decisions are written out instead of coded
    uint16_t* tok;      // next free token of the encode span
    uint32_t est;       // summed prices of the current chunk's decisions, 1/16 bit
    const uint8_t* ptab;
    uint32_t* log;      // k_model_bounds (rc_emit<.., BND>): the logged bits of the span, XZAMD_LOG_WORDS per probability
    uint32_t log_cap;   // at most this many per probability (XZAMD_LOG_CAP)
#ifdef XZAMD_TIMING
    uint64_t tm_run;    // cycles inside rc_run (profiling builds only)
    uint64_t tm_bits;
#endif

    __device__ __forceinline__ void reset()
    {
        low = 0; range = 0xFFFFFFFFu; cache_size = 1; cache = 0;
    }
    __device__ __forceinline__ void shift_low()
    {
        if ((uint32_t)low < 0xFF000000u || (uint32_t)(low >> 32) != 0) {
            const uint32_t carry = (uint32_t)(low >> 32);
            const uint32_t lane = threadIdx.x;
            // byte 0 = cache + carry, then cache_size-1 bytes of 0xFF + carry
            if (cache_size == 1) {                   // the usual case: one pending byte
                if (lane == 0) out[cpos] = (uint8_t)(cache + carry);
            } else {
                for (uint32_t i = lane; i < cache_size; i += 64)
                    out[cpos + i] = (uint8_t)((i == 0 ? cache : 0xFFu) + carry);
            }
            cpos += cache_size;
            cache_size = 0;
            cache = (uint32_t)(low >> 24) & 0xFF;
        }
        ++cache_size;
        low = (low & 0x00FFFFFFu) << 8;
    }
    __device__ __forceinline__ void normalize()
    {
        if (range < (1u << 24)) { shift_low(); range <<= 8; }
    }
    __device__ __forceinline__ void bit(uint16_t* probs, uint32_t idx, uint32_t b)
    {
        normalize();
        uint32_t p = uni(probs[idx]);
        const uint32_t bound = (range >> 11) * p;
        if (!b) { range = bound; p += (2048 - p) >> 5; }
        else { low += bound; range -= bound; p -= p >> 5; }
        probs[idx] = (uint16_t)p;
    }
    __device__ __forceinline__ void tree(uint16_t* probs, uint32_t base, uint32_t nbits, uint32_t sym)
    {
        uint32_t m = 1;
        do {
            const uint32_t b = (sym >> --nbits) & 1;
            bit(probs, base + m, b);
            m = (m << 1) + b;
        } while (nbits);
    }
    __device__ __forceinline__ void direct(uint32_t value, uint32_t nbits)
    {
        do {
            normalize();
            range >>= 1;
            if ((value >> --nbits) & 1) low += range;
        } while (nbits);
    }
    __device__ __forceinline__ void flush()
    {
        normalize();                     // the queue loop normalizes before the first RC_FLUSH
        for (int i = 0; i < 5; ++i) shift_low();
        reset();
    }
};

// ------------------------------------------------------------------------------------------
// LZMA symbol coder (lzma/lzma_encoder.c:23-263)
// ------------------------------------------------------------------------------------------
#ifdef XZAMD_LIT16
typedef uint16_t plit_t_fwd;
#else
typedef uint32_t plit_t_fwd;
#endif
struct Lz {
    uint32_t state;
    uint32_t rep0, rep1, rep2, rep3;
    uint32_t lc, lp, pb;
    uint32_t cnt_len, cnt_match, cnt_align;   // coded lengths / matches / align-coded matches since refresh
    plit_t_fwd* lit;                          // literal coder probabilities of this span (global memory, L2-resident)
    uint32_t* gp;                             // parse pieces (PG): every other probability of the piece's model, u32 each, global
};

// lc / lp of Block blk: the job's, or with a props table (XZAMD_F_AUTO_LCLP) the Block's own pair -- never more literal
// coders than the job's, so every slot stride (0x300 << (a.lc + a.lp), model_slots_pad) stays the job's and such a Block
// uses the front of its slots.  blk is wave-uniform; callers load once at kernel start.
__device__ __forceinline__ void block_lclp(const xzamd_span_args& a, uint32_t blk, uint32_t& lc, uint32_t& lp)
{
    lc = a.lc; lp = a.lp;
    if (a.props_tab != nullptr) {
        const uint32_t v = uni(a.props_tab[blk]);
        lc = v & 255u; lp = v >> 8;
    }
}

__device__ __forceinline__ uint32_t dist_slot_of(uint32_t d)
{
    if (d <= 4) return d;
    const uint32_t i = 31 - __builtin_clz(d);
    return (i + i) + ((d >> (i - 1)) & 1);
}

// Literal-coder probabilities (6144 of the 7990 model entries at lc=3) live in global memory, one
// 24 KiB slice per span, so the LDS footprint of a wavefront drops from 16 KiB to 3.6 KiB and the
// CU can hold 2x (and more) wavefronts: the kernel is issue-latency bound per wave and throughput
// scales with resident waves (measured: halving occupancy costs 1.8x).  A literal touches 8 of them:
// one gather and one scatter per symbol, L1 bypassed (sc1) so the wave reads back its own updates
// from L2.
// XZAMD_LIT16 (measurement build): the literal coders as u16 instead of u32 -- half the L2 footprint of a piece's model
#ifdef XZAMD_LIT16
typedef uint16_t plit_t;
#define PLIT_PER_U4 8u
#define PLIT_FLAT4 make_uint4(0x04000400u, 0x04000400u, 0x04000400u, 0x04000400u)
__device__ __forceinline__ uint32_t lit_load(const uint16_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lit_store(uint16_t* p, uint32_t v)
{
    __hip_atomic_store(p, (uint16_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#else
typedef uint32_t plit_t;
#define PLIT_PER_U4 4u
#define PLIT_FLAT4 make_uint4(1024u, 1024u, 1024u, 1024u)
#endif
__device__ __forceinline__ uint32_t lit_load(const uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void lit_store(uint32_t* p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- wave-parallel symbol coder -------------------------------------------------------------
// An LZMA symbol is a list of <= 48 (probability, bit) pairs whose probability INDICES are known
// up front (lzma_encoder.c:23-263 walks them one rc_bit at a time).  Lane k of the wavefront
// owns pair k: all probabilities are fetched with ONE LDS gather, adapted in parallel (the update
// depends only on the old value and the bit) and written back with ONE scatter; only the
// range/low recurrence (range_encoder.h:196-257) runs serially, on scalar registers, through a
// single copy of the normalise/shift_low code.
enum : uint32_t { SEG_BIT = 0, SEG_TREE = 1, SEG_REV = 2, SEG_DIRECT = 3, SEG_MATCHED = 4 };

struct SegSel {            // per lane: which segment this lane's pair belongs to
    uint32_t type, base, sym, i, n;
    bool hit;
};

__device__ __forceinline__ void seg_add(SegSel& s, uint32_t& off, uint32_t n, uint32_t type, uint32_t base, uint32_t sym)
{
    const uint32_t k = threadIdx.x;
    const bool h = k - off < n;                 // off <= k < off + n (unsigned wrap)
    s.type = h ? type : s.type;
    s.base = h ? base : s.base;
    s.sym = h ? sym : s.sym;
    s.i = h ? k - off : s.i;
    s.n = h ? n : s.n;
    s.hit = s.hit || h;
    off += n;
}

// serial part: t = p (12 bits) | bit << 12 | direct << 13, one entry per lane 0..n-1
// Entries [d0, d1) are direct bits (rc_direct), all others probability-coded; the latter are
// written without data-dependent branches (the bit only selects via a mask).
template <bool PIN>
__device__ __forceinline__ void rc_run(RC& rc, uint32_t packed, uint32_t n, uint32_t d0, uint32_t d1)
{
#ifdef XZAMD_TIMING
    const uint64_t t0_ = __builtin_amdgcn_s_memtime();
    rc.tm_bits += n;
#endif
    uint32_t k = 0;
    for (;;) {
        const uint32_t stop = k < d0 ? d0 : n;
        for (; k < stop; ++k) {
            const uint32_t t = lane_of(packed, k);
            rc.normalize();
            const uint32_t m = 0u - ((t >> 12) & 1u);          // all ones for a 1 bit
            const uint32_t bound = (rc.range >> 11) * (t & 0xFFFu);
            rc.low += bound & m;
            rc.range = bound + ((rc.range - 2 * bound) & m);   // 1: range - bound, 0: bound
            if constexpr (PIN) { pin_s(rc.range); pin_s(rc.low); }
        }
        if (k >= n) break;
        for (; k < d1; ++k) {
            const uint32_t t = lane_of(packed, k);
            rc.normalize();
            rc.range >>= 1;
            rc.low += rc.range & (0u - ((t >> 12) & 1u));
            if constexpr (PIN) { pin_s(rc.range); pin_s(rc.low); }
        }
    }
#ifdef XZAMD_TIMING
    rc.tm_run += __builtin_amdgcn_s_memtime() - t0_;
#endif
}

// CODE: run the range coder (false: the parse pieces of the two-phase mode only adapt their price model);
// LITG: literal-coder probabilities live in global memory (u32 each, `lit`), else in LDS behind P_LITERAL (u16);
// TOK: the model pass of the two-phase coder: one 16-bit token per decision goes to rc.tok and the price of the
// decisions (the parser's table, probability before its update) is added to rc.est.
// PG: the whole model lives in global memory (the parse pieces: `gp` holds what LDS holds elsewhere).
// BND: the bounds walk of the carried model (k_model_walk<1, 2>): `probs` is a u32 array, lo | hi << 11 | logged << 22 per
// probability; both bounds take the update, and while they differ the bit is logged for k_model_chain (the log is zero on entry:
// only 1 bits are written).  Tokens are only counted.
template <bool CODE, bool LITG, bool TOK = false, bool PG = false, bool BND = false>
__device__ __forceinline__ void rc_emit(RC& rc, uint16_t* probs, plit_t* lit, uint32_t* gp, const SegSel& s, uint32_t total,
        uint32_t d0, uint32_t d1)
{
    uint32_t idx = 0, bit = 0;
    bool direct = false;
    if (s.hit) {
        const uint32_t i = s.i, n = s.n, sym = s.sym;
        if (s.type == SEG_BIT) {
            idx = s.base; bit = sym & 1;
        } else if (s.type == SEG_TREE) {            // rc_bittree: MSB first
            bit = (sym >> (n - 1 - i)) & 1;
            idx = s.base + ((1u << i) | (sym >> (n - i)));
        } else if (s.type == SEG_REV) {             // rc_bittree_reverse: LSB first
            bit = (sym >> i) & 1;
            const uint32_t low = sym & ((1u << i) - 1);
            idx = s.base + ((1u << i) | (__builtin_bitreverse32(low) >> ((32 - i) & 31)));   // i == 0: low == 0
        } else if (s.type == SEG_DIRECT) {
            bit = (sym >> (n - 1 - i)) & 1;
            direct = true;
        } else {                                    // literal_matched (lzma_encoder.c:23-41)
            const uint32_t cur = sym & 0xFF, mb = sym >> 8;
            bit = (cur >> (7 - i)) & 1;
            const uint32_t pre = (0x100u | cur) >> (8 - i);
            const bool same = (mb >> (8 - i)) == (cur >> (8 - i));
            idx = s.base + (same ? 0x100u + (((mb >> (7 - i)) & 1) << 8) + pre : pre);
        }
    }
    if constexpr (BND) {
        uint32_t* const M = reinterpret_cast<uint32_t*>(probs);
        if (s.hit && !direct) {
            // (LITG: the literal coders' bounds live in the span's slice of cb_bnd in global memory, read and written past L1)
            const bool glob = LITG && idx >= P_LITERAL;
            const uint32_t v = glob ? lit_load(reinterpret_cast<const uint32_t*>(lit) + (idx - P_LITERAL)) : M[idx];
            uint32_t lo = v & 0x7FFu, hi = (v >> 11) & 0x7FFu, nb = v >> 22;
            if (lo != hi && nb < rc.log_cap) {
                if (bit) atomicOr(rc.log + (uint64_t)idx * XZAMD_LOG_WORDS + (nb >> 5), 1u << (nb & 31u));
                ++nb;
            }
            lo = bit ? lo - (lo >> 5) : lo + ((2048u - lo) >> 5);
            hi = bit ? hi - (hi >> 5) : hi + ((2048u - hi) >> 5);
            const uint32_t nv = lo | (hi << 11) | (nb << 22);
            if (glob) lit_store(reinterpret_cast<uint32_t*>(lit) + (idx - P_LITERAL), nv);
            else M[idx] = nv;
        }
        rc.tok += total;
        return;
    }
    uint32_t p = 0;
    if (s.hit && !direct) {
        if ((LITG || PG) && idx >= P_LITERAL) {
            plit_t* g = lit + (idx - P_LITERAL);
            p = lit_load(g);
            lit_store(g, bit ? p - (p >> 5) : p + ((2048 - p) >> 5));
        } else if (PG) {
            uint32_t* g = gp + idx;
            p = lit_load(g);
            lit_store(g, bit ? p - (p >> 5) : p + ((2048 - p) >> 5));
        } else {
            p = probs[idx];
            probs[idx] = (uint16_t)(bit ? p - (p >> 5) : p + ((2048 - p) >> 5));
        }
    }
    if constexpr (TOK) {
        const uint32_t k = threadIdx.x;
        uint32_t price = 0;
        if (k < total) {
            rc.tok[k] = (uint16_t)(p | (bit << 12) | (direct ? 0x8000u : 0u));
            price = direct ? 16u : (uint32_t)rc.ptab[(p ^ ((0u - bit) & 0x7FFu)) >> 4];
        }
        rc.est += wave_sum_dpp(price);
        rc.tok += total;
    } else if constexpr (PG) {
        // the parser's price of its own parse (rc.ptab set: the recorded symbols of a piece; oracle: parse_piece's return value)
        if (rc.ptab != nullptr) {
            const uint32_t price = threadIdx.x < total ? (direct ? 16u : (uint32_t)rc.ptab[(p ^ ((0u - bit) & 0x7FFu)) >> 4]) : 0u;
            rc.est += wave_sum_dpp(price);
        }
    } else if constexpr (CODE) {
        const uint32_t packed = p | (bit << 12) | (direct ? 0x2000u : 0u);
        rc_run<!LITG>(rc, packed, total, d0, d1);
    }
}

// upos = offset of the symbol inside the Block; lit3 (literals only) = byte | previous byte << 8 | match byte << 16
// (the match byte is read only in states >= 7)
template <bool CODE, bool LITG, bool TOK = false, bool PG = false, bool BND = false>
__device__ __forceinline__ void encode_symbol_t(RC& rc, uint16_t* probs, Lz& z, uint32_t upos, uint32_t back, uint32_t len,
        uint32_t lit3)
{
    if (PG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // the previous symbol's probability scatter
    const uint32_t ps = upos & ((1u << z.pb) - 1);
    SegSel s;
    s.type = 0; s.base = 0; s.sym = 0; s.i = 0; s.n = 0; s.hit = false;
    uint32_t off = 0;
    if (back == LITERAL) {
        if (LITG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // previous literal's probability scatter
        seg_add(s, off, 1, SEG_BIT, P_IS_MATCH + z.state * 16 + ps, 0);
        const uint32_t cur = lit3 & 0xFFu;
        const uint32_t prev = (lit3 >> 8) & 0xFFu;
        const uint32_t mask = (0x100u << z.lp) - (0x100u >> z.lc);
        const uint32_t sub = P_LITERAL + 3u * ((((upos << 8) + prev) & mask) << z.lc);
        if (z.state < 7) {
            z.state = z.state <= 3 ? 0 : z.state - 3;
            seg_add(s, off, 8, SEG_TREE, sub, cur);
        } else {
            z.state = z.state <= 9 ? z.state - 3 : z.state - 6;
            const uint32_t mb = (lit3 >> 16) & 0xFFu;
            seg_add(s, off, 8, SEG_MATCHED, sub, cur | (mb << 8));
        }
        rc_emit<CODE, LITG, TOK, PG, BND>(rc, probs, z.lit, z.gp, s, off, off, off);
        return;
    }
    seg_add(s, off, 1, SEG_BIT, P_IS_MATCH + z.state * 16 + ps, 1);
    uint32_t len_base, dir0 = ~0u, dir1 = ~0u;
    if (back < 4) {
        seg_add(s, off, 1, SEG_BIT, P_IS_REP + z.state, 1);
        if (back == 0) {
            seg_add(s, off, 1, SEG_BIT, P_IS_REP0 + z.state, 0);
            seg_add(s, off, 1, SEG_BIT, P_IS_REP0_LONG + z.state * 16 + ps, len != 1);
        } else {
            seg_add(s, off, 1, SEG_BIT, P_IS_REP0 + z.state, 1);
            uint32_t dist;
            if (back == 1) {
                seg_add(s, off, 1, SEG_BIT, P_IS_REP1 + z.state, 0);
                dist = z.rep1;
            } else {
                seg_add(s, off, 1, SEG_BIT, P_IS_REP1 + z.state, 1);
                seg_add(s, off, 1, SEG_BIT, P_IS_REP2 + z.state, back - 2);
                if (back == 3) { dist = z.rep3; z.rep3 = z.rep2; }
                else dist = z.rep2;
                z.rep2 = z.rep1;
            }
            z.rep1 = z.rep0;
            z.rep0 = dist;
        }
        if (len == 1) {
            z.state = z.state < 7 ? 9 : 11;
            rc_emit<CODE, LITG, TOK, PG, BND>(rc, probs, z.lit, z.gp, s, off, off, off);
            return;
        }
        len_base = P_REP_LEN;
        z.state = z.state < 7 ? 8 : 11;
        ++z.cnt_len;
    } else {
        seg_add(s, off, 1, SEG_BIT, P_IS_REP + z.state, 0);
        len_base = P_MATCH_LEN;
        z.state = z.state < 7 ? 7 : 10;
        ++z.cnt_len;
        ++z.cnt_match;
    }
    // length (lzma_encoder.c:106-134)
    {
        const uint32_t l = len - 2;
        if (l < 8) {
            seg_add(s, off, 1, SEG_BIT, len_base + LEN_CHOICE, 0);
            seg_add(s, off, 3, SEG_TREE, len_base + LEN_LOW + ps * 8, l);
        } else if (l < 16) {
            seg_add(s, off, 1, SEG_BIT, len_base + LEN_CHOICE, 1);
            seg_add(s, off, 1, SEG_BIT, len_base + LEN_CHOICE2, 0);
            seg_add(s, off, 3, SEG_TREE, len_base + LEN_MID + ps * 8, l - 8);
        } else {
            seg_add(s, off, 1, SEG_BIT, len_base + LEN_CHOICE, 1);
            seg_add(s, off, 1, SEG_BIT, len_base + LEN_CHOICE2, 1);
            seg_add(s, off, 8, SEG_TREE, len_base + LEN_HIGH, l - 16);
        }
    }
    if (back >= 4) {
        // distance (lzma_encoder.c:142-181)
        const uint32_t dist = back - 4;
        const uint32_t slot = dist_slot_of(dist);
        const uint32_t ds = len < 6 ? len - 2 : 3;
        seg_add(s, off, 6, SEG_TREE, P_DIST_SLOT + ds * 64, slot);
        if (slot >= 4) {
            const uint32_t fb = (slot >> 1) - 1;
            const uint32_t base = (2 | (slot & 1)) << fb;
            const uint32_t red = dist - base;
            if (slot < 14) {
                seg_add(s, off, fb, SEG_REV, P_DIST_SPECIAL + base - slot - 1, red);
            } else {
                dir0 = off;
                seg_add(s, off, fb - 4, SEG_DIRECT, 0, red >> 4);
                dir1 = off;
                seg_add(s, off, 4, SEG_REV, P_DIST_ALIGN, red & 15);
                ++z.cnt_align;
            }
        }
        z.rep3 = z.rep2; z.rep2 = z.rep1; z.rep1 = z.rep0; z.rep0 = dist;
    }
    if (dir0 == ~0u) dir0 = dir1 = off;
    rc_emit<CODE, LITG, TOK, PG, BND>(rc, probs, z.lit, z.gp, s, off, dir0, dir1);
}

// the bytes a literal at global offset g needs, for encode_symbol_t
__device__ __forceinline__ uint32_t literal_bytes(const uint8_t* __restrict__ in, uint32_t g, uint32_t upos, const Lz& z)
{
    const uint32_t cur = uni(in[g]);
    const uint32_t prev = upos ? uni(in[g - 1]) : 0;
    const uint32_t mb = z.state >= 7 ? uni(in[g - z.rep0 - 1]) : 0;
    return cur | (prev << 8) | (mb << 16);
}

// g = global offset of the byte, upos = its offset inside the Block (single-phase kernels: code while parsing)
__device__ __forceinline__ void encode_symbol(RC& rc, uint16_t* probs, Lz& z, const uint8_t* __restrict__ in,
        uint32_t g, uint32_t upos, uint32_t back, uint32_t len)
{
    encode_symbol_t<true, true>(rc, probs, z, upos, back, len, back == LITERAL ? literal_bytes(in, g, upos, z) : 0u);
}

__device__ __forceinline__ bool change_pair(uint32_t small_dist, uint32_t big_dist)
{
    return (big_dist >> 7) > small_dist;
}

// ------------------------------------------------------------------------------------------
// Suffix-neighbourhood match finder (the GPU successor of BT4) and the windowed optimal parser.
// Semantics are defined by oracle/lzma_fast_enc.c (build_sa / find_sn / optimum_window); the code
// below is their wave-parallel form and must stay bit-exact with them.
// ------------------------------------------------------------------------------------------
// Optimal-parser window: nodes 0..WM, a template parameter of the parser.  384 for every option set since round 5 (LDS per
// wave <= 10 KiB -> 16 waves per CU); rounds 1-4 ran 232 nodes, and 360 at 12 waves per CU for nice_len > 128.
constexpr uint32_t WMAX_STD = 384;
constexpr uint32_t PRICE_INF = 1u << 30;

#ifdef XZAMD_TIMING
#define TM_BEGIN(v) const uint64_t v = __builtin_amdgcn_s_memtime()
#define TM_END(w, k, v) do { if (threadIdx.x == 0) (w).tm[k] += __builtin_amdgcn_s_memtime() - (v); } while (0)
#define TM_COUNT(w, k) do { if (threadIdx.x == 0) (w).tm[k] += 1; } while (0)
#else
#define TM_BEGIN(v) do { } while (0)
#define TM_END(w, k, v) do { } while (0)
#define TM_COUNT(w, k) do { } while (0)
#endif

// Per-wave LDS carve for the list-based paths.
struct Work {
    // optimal parser only
    uint32_t* n_price;  // [WM+1] node price; after backtracking: out-edge `back`
    uint32_t* n_info;   // [WM+1] in-len (9) | state (4) << 9 | out-len (9) << 13 | in-edge kind (3) << 22
                        //          kind: 0..3 = rep index, 4 = match (its distance is the node's rep0), 5 = literal
    uint4* n_reps4;     // [WM+1] rep distances of the node (complete when the parser reaches it)
    uint16_t* dsp;      // [4*64]  dist-slot price (+ direct bits for slot >= 14)
    uint16_t* xt;       // [128]   price of the footer bits of distances < 128 (slots 4..13, 0 below)
    uint16_t* ap;       // [16]    align price; == xt + 128, so one table: index dist < 128 ? dist : 128 + (dist & 15)
    uint8_t* ptab;      // [128]   bit price table (price_tablegen.c:31-58)
    uint32_t* err;      // debug/consistency word block (global)
    uint32_t ptv;       // the same price table in registers: lane l (< 32) holds entries 4l..4l+3
#ifdef XZAMD_TIMING
    unsigned long long* tm;   // [16] cycle accumulators in LDS (profiling builds only)
#endif
};

struct RoundL {
    uint32_t rp[4];     // list-driven parser: the four rep-match lengths
    uint32_t rl[4];     // the same, 0 when < 2 (usable rep matches)
    uint32_t pre;       // compound precheck: some rep source has two equal bytes right behind its first mismatch
    uint32_t mlo, mhi;  // lane i < 4: mismatch mask of rep source i over the 64-byte row at x (bit o: offset o differs or is past the end)
    uint32_t l2a, l2b;  // rep0 run behind the byte after the longest / second longest match (list trailer)
    uint32_t L;         // per lane; lanes 60..63 = rep lengths (in-kernel finders)
    uint32_t SL, SD;    // kept matches sorted by length: lane r holds entry r (length, zero-based distance)
    uint32_t cnt;       // number of entries
    uint32_t longest;   // incl. the > nice_len extension
};

__device__ __forceinline__ uint64_t rm_of(const RoundL& R, uint32_t i)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)R.mhi, (int)i) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)R.mlo, (int)i);
}

// lane `dst` receives `v` from this lane (all lanes must execute; unused senders target lane 63)
__device__ __forceinline__ uint32_t lane_scatter(uint32_t dst, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_ds_permute((int)(dst << 2), (int)v);
}

// The five byte rows of a round (lane = byte offset): the text at x and the four rep sources.  They can be issued as
// soon as the node's rep distances are final -- for node j + 1 that is right after the literal / short-rep edge out of
// node j, every other edge out of j is longer -- and are only waited for when the round is worked out.
struct Rows { uint32_t cx, c0, c1, c2, c3; };

__device__ __forceinline__ void rows_issue(const Env& e, uint32_t x, uint32_t end,
        uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, Rows& W)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t avail = end - x;
    const uint32_t buf_avail = avail < MATCH_LEN_MAX ? avail : MATCH_LEN_MAX;
    const uint32_t off = lane < buf_avail ? lane : 0u;      // lanes past the end re-read byte 0 (masked by the round)
    W.cx = e.in[x + off];
    W.c0 = e.in[x - r0 - 1 + off]; W.c1 = e.in[x - r1 - 1 + off];
    W.c2 = e.in[x - r2 - 1 + off]; W.c3 = e.in[x - r3 - 1 + off];
}

// A node with the rep distances of the node in front of it (reached by a literal, or by the same match or rep at another
// length: 57 % of the nodes of the bench text): its four mismatch masks are that node's shifted down by one byte, and only
// offset 63 is new -- ONE load (lanes 0..3: byte 63 of the four rep sources, every other lane: byte 63 of the text) in place
// of the five rows.  Offset 63 is dead when fewer than 64 bytes are left (the masks' `dead` bits cover it).
__device__ __forceinline__ void rows_issue_top(const Env& e, uint32_t x, uint32_t end,
        uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, Rows& W)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t off = end - x > 63u ? 63u : 0u;
    const uint32_t back = lane == 0 ? r0 + 1 : lane == 1 ? r1 + 1 : lane == 2 ? r2 + 1 : lane == 3 ? r3 + 1 : 0u;
    W.cx = e.in[x + off - back];
}

template <bool SHIFT = false>
__device__ __forceinline__ void round_lists_rows(const Env& e, ListPre& LP, uint32_t x, uint32_t end,
        uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, const Rows& W, RoundL& R, const bool shift = false)
{
    const uint32_t lane = threadIdx.x;
    if (!(LP.valid && LP.pos == x)) lists_load(e, x, LP.v, LP.l16);
    uint32_t sl, sd, tv;
    lists_split(e, LP.v, LP.l16, sl, sd, tv);
    lists_load(e, x + 1, LP.v, LP.l16);
    LP.pos = x + 1;
    LP.valid = true;
    const uint32_t avail = end - x;
    const uint32_t buf_avail = avail < MATCH_LEN_MAX ? avail : MATCH_LEN_MAX;
    // Rep-match lengths: one 64-byte row of the text against the four rep sources, lane = byte offset, a
    // ballot each (bit o: offset o differs or lies past the end).  Everything that follows from a mask --
    // length, "usable" length, the compound precheck -- is then worked out by lane i for rep i with vector
    // instructions (the scalar unit is what bounds this kernel), and only the results go back to scalars.
    {
        const uint64_t dead = buf_avail < 64 ? ~0ull << buf_avail : 0ull;
        uint32_t lo, hi;
        if (SHIFT && shift) {
            // the masks of the node in front, one byte further on (lane i: rep i); bit 63 from the one load of rows_issue_top
            const uint32_t nb = W.cx != lane_of(W.cx, 4) ? 0x80000000u : 0u;          // lanes 0..3 can differ
            lo = (R.mlo >> 1) | (R.mhi << 31) | (uint32_t)dead;
            hi = (R.mhi >> 1) | nb | (uint32_t)(dead >> 32);
        } else {
            const uint32_t cx = W.cx, c0 = W.c0, c1 = W.c1, c2 = W.c2, c3 = W.c3;
            const uint64_t m0 = __builtin_amdgcn_ballot_w64(c0 != cx) | dead, m1 = __builtin_amdgcn_ballot_w64(c1 != cx) | dead;
            const uint64_t m2 = __builtin_amdgcn_ballot_w64(c2 != cx) | dead, m3 = __builtin_amdgcn_ballot_w64(c3 != cx) | dead;
            lo = lane == 0 ? (uint32_t)m0 : lane == 1 ? (uint32_t)m1 : lane == 2 ? (uint32_t)m2 : (uint32_t)m3;
            hi = lane == 0 ? (uint32_t)(m0 >> 32) : lane == 1 ? (uint32_t)(m1 >> 32)
                    : lane == 2 ? (uint32_t)(m2 >> 32) : (uint32_t)(m3 >> 32);
        }
        R.mlo = lo; R.mhi = hi;
        const uint32_t l = lo ? (uint32_t)__builtin_ctz(lo) : hi ? 32u + (uint32_t)__builtin_ctz(hi) : 64u;
        const uint32_t lu = l >= 2 ? l : 0u;
        // two equal bytes behind the first mismatch <=> bits l+1, l+2 clear (bit l is set)
        const uint64_t mm = ((uint64_t)hi << 32) | lo;
        const uint32_t t3 = (uint32_t)(mm >> (l & 63u)) & 7u;
        const bool okl = (l - 2u < 60u) || (lane == 0 && l == 0);
        R.pre = __builtin_amdgcn_ballot_w64(lane < 4 && okl && t3 == 1u) != 0ull;
        const uint64_t full = __builtin_amdgcn_ballot_w64(lane < 4 && l >= 64u);
        R.rp[0] = lane_of(l, 0); R.rp[1] = lane_of(l, 1); R.rp[2] = lane_of(l, 2); R.rp[3] = lane_of(l, 3);
        R.rl[0] = lane_of(lu, 0); R.rl[1] = lane_of(lu, 1); R.rl[2] = lane_of(lu, 2); R.rl[3] = lane_of(lu, 3);
        if (full) {                                             // a rep match of >= 64 bytes: the slow path
            if (full & 1) R.rl[0] = R.rp[0] = wave_cmplen(e.in, x, x - r0 - 1, 64, buf_avail);
            if (full & 2) R.rl[1] = R.rp[1] = wave_cmplen(e.in, x, x - r1 - 1, 64, buf_avail);
            if (full & 4) R.rl[2] = R.rp[2] = wave_cmplen(e.in, x, x - r2 - 1, 64, buf_avail);
            if (full & 8) R.rl[3] = R.rp[3] = wave_cmplen(e.in, x, x - r3 - 1, 64, buf_avail);
        }
    }
    const uint32_t tr = lane_of(tv, LIST_K);
    const uint32_t cnt = tr & 0xFFu;
    uint32_t slc = sl, l2a = (tr >> 8) & 0xFFu, l2b = (tr >> 16) & 0xFFu;
    uint32_t longest = cnt ? lane_of(sl, cnt - 1) : 0;
    if (avail < MATCH_LEN_MAX + 1 + LEN2_MAX) {
        // The records are made for the whole Block; a span may not reference bytes behind its end, so near the end
        // the parser clamps what it reads (oracle: do_round): lengths to the bytes left, the rep0 run of the
        // "match + literal + rep0" edge to what follows match + literal.
        const uint32_t second = cnt >= 2 ? lane_of(sl, cnt - 2) : 0;
        l2a = longest + 1 >= avail ? 0u : min(l2a, avail - longest - 1);
        l2b = second + 1 >= avail ? 0u : min(l2b, avail - second - 1);
        slc = min(sl, avail);
        longest = min(longest, avail);
    }
    R.SL = slc;
    R.SD = sd;
    R.cnt = cnt;
    R.l2a = l2a;
    R.l2b = l2b;
    R.longest = longest;
}

__device__ __forceinline__ void round_lists(const Env& e, ListPre& LP, uint32_t x, uint32_t end,
        uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, RoundL& R)
{
    Rows W;
    rows_issue(e, x, end, r0, r1, r2, r3, W);
    round_lists_rows(e, LP, x, end, r0, r1, r2, r3, W, R);
}

// ---- prices (rangecoder/price.h:28-92) ------------------------------------------------------
// The non-literal probabilities of a model behind one accessor: `const uint16_t*` (LDS: the single-phase kernels) or GProbs
// (global memory, u32 each, read past L1 like the literal coders: the parse pieces, whose LDS goes to the DP nodes).
struct GProbs {
    uint32_t* p;
    __device__ __forceinline__ uint32_t operator[](uint32_t i) const { return lit_load(p + i); }
};

template <class PR>
__device__ __forceinline__ uint32_t pr_bit(PR probs, const uint8_t* ptab, uint32_t idx, uint32_t bit)
{
    return ptab[(probs[idx] ^ ((0u - bit) & 0x7FFu)) >> 4];
}
template <class PR>
__device__ __forceinline__ uint32_t pr_tree(PR probs, const uint8_t* ptab, uint32_t base,
        uint32_t nbits, uint32_t sym)
{
    uint32_t price = 0;
    sym += 1u << nbits;
    do {
        const uint32_t bit = sym & 1;
        sym >>= 1;
        price += pr_bit(probs, ptab, base + sym, bit);
    } while (sym != 1);
    return price;
}
template <class PR>
__device__ __forceinline__ uint32_t pr_tree_rev(PR probs, const uint8_t* ptab, uint32_t base,
        uint32_t nbits, uint32_t sym)
{
    uint32_t price = 0, m = 1;
    do {
        const uint32_t bit = sym & 1;
        sym >>= 1;
        price += pr_bit(probs, ptab, base + m, bit);
        m = (m << 1) + bit;
    } while (--nbits);
    return price;
}
// price of one length under a length coder (length_update_prices, lzma_encoder.c:77-102, evaluated for a single length)
template <class PR>
__device__ __forceinline__ uint32_t pr_len_one(PR probs, const uint8_t* ptab, uint32_t base, uint32_t ps, uint32_t len)
{
    len -= 2;
    if (len < 8)
        return pr_bit(probs, ptab, base + LEN_CHOICE, 0) + pr_tree(probs, ptab, base + LEN_LOW + ps * 8, 3, len);
    len -= 8;
    if (len < 8)
        return pr_bit(probs, ptab, base + LEN_CHOICE, 1) + pr_bit(probs, ptab, base + LEN_CHOICE2, 0)
                + pr_tree(probs, ptab, base + LEN_MID + ps * 8, 3, len);
    return pr_bit(probs, ptab, base + LEN_CHOICE, 1) + pr_bit(probs, ptab, base + LEN_CHOICE2, 1)
            + pr_tree(probs, ptab, base + LEN_HIGH, 8, len - 8);
}

// Length price tables live in registers, lane = length: lane holds lengths 2 + lane + 64*it.
// The low/mid trees depend on pos_state but cover only lengths 2..17 (lanes 0..15 of it == 0);
// the high tree is shared by all pos_states.  Low 16 bits = match length coder, high 16 = rep.
struct LenTab { uint32_t lo[4]; uint32_t hi[5]; };

// tmp: 256 words of LDS that are dead while the tables are rebuilt (the parser's node array)
template <class PR>
__device__ __forceinline__ void refresh_len_tables(PR probs, const uint8_t* ptab, LenTab& t, uint32_t nps,
        uint32_t* tmp)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t m1 = pr_bit(probs, ptab, P_MATCH_LEN + LEN_CHOICE, 1), r1 = pr_bit(probs, ptab, P_REP_LEN + LEN_CHOICE, 1);
    {
        const uint32_t mh = m1 + pr_bit(probs, ptab, P_MATCH_LEN + LEN_CHOICE2, 1);
        const uint32_t rh = r1 + pr_bit(probs, ptab, P_REP_LEN + LEN_CHOICE2, 1);
#pragma unroll 1
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t sym = lane + 64u * k;
            const uint32_t pm = mh + pr_tree(probs, ptab, P_MATCH_LEN + LEN_HIGH, 8, sym);
            const uint32_t prr = rh + pr_tree(probs, ptab, P_REP_LEN + LEN_HIGH, 8, sym);
            tmp[sym] = pm | (prr << 16);
        }
    }
    wave_sync();
#pragma unroll
    for (int it = 0; it < 5; ++it) {
        const uint32_t len = 2 + lane + 64u * it;
        t.hi[it] = (len >= 18 && len <= MATCH_LEN_MAX) ? tmp[len - 18] : 0;
    }
    wave_sync();
    const uint32_t m0 = pr_bit(probs, ptab, P_MATCH_LEN + LEN_CHOICE, 0), r0 = pr_bit(probs, ptab, P_REP_LEN + LEN_CHOICE, 0);
    const uint32_t mm = m1 + pr_bit(probs, ptab, P_MATCH_LEN + LEN_CHOICE2, 0);
    const uint32_t rm = r1 + pr_bit(probs, ptab, P_REP_LEN + LEN_CHOICE2, 0);
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
        uint32_t v = 0;
        if (lane < 16 && (uint32_t)ps < nps) {
            const uint32_t sub = (lane < 8 ? LEN_LOW : LEN_MID) + (uint32_t)ps * 8, sym = lane & 7;
            const uint32_t pm = (lane < 8 ? m0 : mm) + pr_tree(probs, ptab, P_MATCH_LEN + sub, 3, sym);
            const uint32_t prr = (lane < 8 ? r0 : rm) + pr_tree(probs, ptab, P_REP_LEN + sub, 3, sym);
            v = pm | (prr << 16);
        }
        t.lo[ps] = v;
    }
}

template <class PR>
__device__ __forceinline__ void refresh_dist_tables(PR probs, const Work& w)
{
    const uint32_t lane = threadIdx.x;
#pragma unroll 1
    for (uint32_t i = lane; i < 256; i += 64) {
        const uint32_t ds = i >> 6, slot = i & 63;
        uint32_t pr = pr_tree(probs, w.ptab, P_DIST_SLOT + ds * 64, 6, slot);
        if (slot >= 14) pr += (((slot >> 1) - 1) - 4) << 4;
        w.dsp[i] = (uint16_t)pr;
    }
    // footer of distances < 128: the reverse bit tree of slots 4..13 (lzma_encoder.c:160-168); the
    // slot part is in dsp, so  price(dist < 128) = dsp[ds][slot] + xt[dist]  (the sum the reference
    // keeps in dist_prices[], optimum_normal.c:132-183)
#pragma unroll 1
    for (uint32_t d = lane; d < 128; d += 64) {
        uint32_t pr = 0;
        if (d >= 4) {
            const uint32_t slot = dist_slot_of(d);
            const uint32_t fb = (slot >> 1) - 1;
            const uint32_t base = (2 | (slot & 1)) << fb;
            pr = pr_tree_rev(probs, w.ptab, P_DIST_SPECIAL + base - slot - 1, fb, d - base);
        }
        w.xt[d] = (uint16_t)pr;
    }
    wave_sync();
}

template <class PR>
__device__ __forceinline__ void refresh_align_table(PR probs, const Work& w)
{
    const uint32_t lane = threadIdx.x;
    if (lane < 16) w.ap[lane] = (uint16_t)pr_tree_rev(probs, w.ptab, P_DIST_ALIGN, 4, lane);
    wave_sync();
}

// ---- literal prices (get_literal_price, optimum_normal.c:21-53) --------------------------------
// Probabilities do not change inside a parser window, so everything that depends only on the input
// bytes is priced once per 64 nodes, lane = node.  With N_i / A_i / B_i the price of bit i of the
// byte in the plain coder, in the matched coder when the match byte has the same bit, and in the
// matched coder when it differs, a literal costs
//     plain (state < 7):                          sum N_i
//     matched, first differing bit k of (byte ^ match byte):  sum_{i<k} A_i + B_k + sum_{i>k} N_i
//     matched, match byte == byte (k = 8):        sum A_i
// i.e. ten values per node, none of which depends on the path; the node later picks one by k.
// 24 independent gathers per lane, one memory round trip per 64 nodes.
struct LitChunk { uint32_t v[5]; };     // (V0,V1) (V2,V3) (V4,V5) (V6,V7) 16 bits each; V8 | plain << 11 | byte << 22

__device__ __forceinline__ void lit_chunk(const uint8_t* __restrict__ in, const uint8_t* ptab, const Lz& z,
        uint32_t x0, uint32_t block_start, uint32_t span_end, LitChunk& c)
{
    const uint32_t lane = threadIdx.x;
    uint32_t x = x0 + lane;
    if (x >= span_end) x = span_end - 1;
    const uint32_t cur = in[x];
    const uint32_t prev = x > block_start ? in[x - 1] : 0;
    const uint32_t upos = x - block_start;
    const uint32_t mask = (0x100u << z.lp) - (0x100u >> z.lc);
    const plit_t* sub = z.lit + 3u * ((((upos << 8) + prev) & mask) << z.lc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the coder's probability updates must have landed
    uint32_t pn[8], pa[8], pb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t pre = (0x100u | cur) >> (8 - i);
        const uint32_t bit = (cur >> (7 - i)) & 1;
        pn[i] = lit_load(sub + pre);
        pa[i] = lit_load(sub + 0x100u + (bit << 8) + pre);
        pb[i] = lit_load(sub + 0x100u + ((bit ^ 1u) << 8) + pre);
    }
    uint32_t N[8], A[8], B[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t bit = (cur >> (7 - i)) & 1;
        const uint32_t flip = (0u - bit) & 0x7FFu;
        N[i] = ptab[(pn[i] ^ flip) >> 4];
        A[i] = ptab[(pa[i] ^ flip) >> 4];
        B[i] = ptab[(pb[i] ^ flip) >> 4];
    }
    uint32_t sufN[9];                      // sufN[k] = sum_{i>=k} N_i
    sufN[8] = 0;
#pragma unroll
    for (int i = 7; i >= 0; --i) sufN[i] = sufN[i + 1] + N[i];
    uint32_t V[9], preA = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        V[k] = preA + B[k] + sufN[k + 1];
        preA += A[k];
    }
    V[8] = preA;
    c.v[0] = V[0] | (V[1] << 16);
    c.v[1] = V[2] | (V[3] << 16);
    c.v[2] = V[4] | (V[5] << 16);
    c.v[3] = V[6] | (V[7] << 16);
    c.v[4] = V[8] | (sufN[0] << 11) | (cur << 22);
}

// price of the literal at chunk node jj; mb = match byte (only used when state >= 7)
__device__ __forceinline__ uint32_t lit_price(const LitChunk& c, uint32_t jj, uint32_t state, uint32_t mb)
{
    const uint32_t w4 = lane_of(c.v[4], jj);
    if (state < 7) return (w4 >> 11) & 0x7FFu;
    const uint32_t d = ((w4 >> 22) ^ mb) & 0xFFu;
    if (d == 0) return w4 & 0x7FFu;
    const uint32_t k = (uint32_t)__builtin_clz(d) - 24;          // first differing bit, MSB first
    const uint32_t r = k < 2 ? lane_of(c.v[0], jj) : k < 4 ? lane_of(c.v[1], jj) : k < 6 ? lane_of(c.v[2], jj) : lane_of(c.v[3], jj);
    return (k & 1) ? r >> 16 : r & 0xFFFFu;
}

// Relax all rep / match lengths out of node j (lane = length).  A lane that improves its target
// node also writes the node's coder state and rep distances (they follow from this edge), so a node
// is complete the moment the parser reaches it.  Written as selects, not branches: per-lane `if`s
// cost the compiler an exec-mask save/restore and a branch each.
__device__ __forceinline__ void relax_lengths(const Work& w, const LenTab& lt, uint32_t PS, uint32_t SL, uint32_t SD, uint32_t j, uint32_t reach,
        uint32_t longest, uint32_t cnt, uint32_t rl0, uint32_t rl1, uint32_t rl2, uint32_t rl3,
        uint32_t prep0, uint32_t prep1, uint32_t prep2, uint32_t prep3, uint32_t pmatch,
        uint32_t s, uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t info_rep = (s < 7 ? 8u : 11u) << 9, info_match = (s < 7 ? 7u : 10u) << 9;
    const uint32_t lo_ps = PS == 0 ? lt.lo[0] : PS == 1 ? lt.lo[1] : PS == 2 ? lt.lo[2] : lt.lo[3];
    const uint32_t SLx = lane + 1 < cnt ? SL : 0xFFFFu;      // list lengths with everything from the last entry on = infinity
    const bool any_rep = (rl0 | rl1 | rl2 | rl3) != 0;
    // not unrolled: one pass covers 64 lengths and is all that nearly every node needs; five copies of
    // the body would only cost instruction-cache space
#pragma unroll 1
    for (uint32_t it = 0; it < 5; ++it) {
        if (2 + 64u * it > reach) break;
        const uint32_t l = 2 + lane + 64u * it;
        uint32_t idx_m = 0;                       // first entry whose length reaches l (or the last one)
#pragma unroll
        for (uint32_t k = 0; k + 1 < LIST_K; ++k) idx_m += (lane_of(SLx, k) < l) ? 1u : 0u;   // entries >= cnt-1 hold "infinity"
        const uint32_t dist_m = __shfl(SD, idx_m);
        const uint32_t cur = w.n_price[j + l];
        const uint32_t hv = it == 0 ? lt.hi[0] : it == 1 ? lt.hi[1] : it == 2 ? lt.hi[2] : it == 3 ? lt.hi[3] : lt.hi[4];
        const uint32_t lv = (it == 0 && lane < 16) ? lo_ps : hv;
        const uint32_t lpm = lv & 0xFFFFu, lpr = lv >> 16;
        // distance price = slot price (+ direct bits) + footer / align price: two table reads
        const uint32_t ds = l < 6 ? l - 2 : 3;
        const uint32_t dnz = dist_m < 4 ? 4u : dist_m;                     // branch-free slot (fastpos.h:78-86)
        const uint32_t di = 31 - (uint32_t)__builtin_clz(dnz);
        const uint32_t slot = dist_m < 4 ? dist_m : 2 * di + ((dnz >> (di - 1)) & 1);
        const uint32_t p_dist = (uint32_t)w.dsp[ds * 64 + slot] + w.xt[dist_m < 128 ? dist_m : 128 + (dist_m & 15)];
        const uint32_t c4 = l <= longest ? pmatch + lpm + p_dist : PRICE_INF;
        uint32_t best = cur, bb = 0, n0 = r0;
        if (any_rep) {                              // uniform: most nodes of a text have no usable rep match
            const uint32_t c0 = rl0 >= l ? prep0 + lpr : PRICE_INF;
            const uint32_t c1 = rl1 >= l ? prep1 + lpr : PRICE_INF;
            const uint32_t c2 = rl2 >= l ? prep2 + lpr : PRICE_INF;
            const uint32_t c3 = rl3 >= l ? prep3 + lpr : PRICE_INF;
            { const bool t = c0 < best; best = t ? c0 : best; bb = t ? 0u : bb; }
            { const bool t = c1 < best; best = t ? c1 : best; bb = t ? 1u : bb; n0 = t ? r1 : n0; }
            { const bool t = c2 < best; best = t ? c2 : best; bb = t ? 2u : bb; n0 = t ? r2 : n0; }
            { const bool t = c3 < best; best = t ? c3 : best; bb = t ? 3u : bb; n0 = t ? r3 : n0; }
        }
        { const bool t = c4 < best; best = t ? c4 : best; bb = t ? dist_m + 4 : bb; n0 = t ? dist_m : n0; }
        const uint32_t n1 = bb == 0 ? r1 : r0;
        const uint32_t n2 = bb <= 1 ? r2 : r1;
        const uint32_t n3 = bb <= 2 ? r3 : r2;
        if (l <= reach && best < cur) {
            w.n_price[j + l] = best;
            w.n_info[j + l] = l | (bb < 4 ? info_rep | (bb << 22) : info_match | (4u << 22));
            w.n_reps4[j + l] = make_uint4(n0, n1, n2, n3);
        }
    }
}

// ---- compound edges "X + literal + rep0" (lzma_encoder_optimum_normal.c:562-597, 635-687, 728-790) ----
// Seven candidates per node, one lane each: lane 0 = "literal + rep0" (X empty), lanes 1..4 = rep0..rep3
// at its full length, lanes 5 / 6 = the longest / second longest match of the list at its full length.
// Geometry (lengths, target node) depends only on the round; it is fixed before any edge of the node
// is relaxed so that the window end covers the targets.  The rep0 run behind the literal is limited to
// the 64-byte row at x for lanes 0..4 (the rep compare masks) and comes from the list trailer for 5 / 6.
struct Compound {
    uint32_t L1, l2, T;     // per lane: length of X, rep0 run, target node (valid lanes)
    uint32_t dist;          // per lane: distance X leaves in rep0 (lanes 1..6)
    uint64_t mask;          // valid candidate lanes
};

__device__ __forceinline__ uint32_t mask_run_after(uint64_t m, uint32_t first)
{
    // equal bytes behind the mismatch at offset `first` inside the row (m: bit o = offset o differs / past the end)
    const uint64_t rest = first >= 63 ? 0ull : (m >> (first + 1));
    return rest ? (uint32_t)__builtin_ctzll(rest) : 63u - min(first, 63u);
}

__device__ __forceinline__ void compound_setup(const RoundL& RL, uint32_t j, uint32_t room, uint32_t buf_avail,
        uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, Compound& c, const uint32_t WMAX)
{
    const uint32_t lane = threadIdx.x;
    // uniform per-candidate geometry
    uint32_t L1[7], l2[7];
    bool ok[7];
    L1[0] = 0;
    ok[0] = RL.rp[0] == 0;                                     // rep0's byte differs here (buf_avail >= 1 inside a span)
    l2[0] = ok[0] ? mask_run_after(rm_of(RL, 0), 0) : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t l = RL.rp[i];
        L1[1 + i] = l;
        ok[1 + i] = l >= 2 && l <= room && l < buf_avail && l < 64;
        l2[1 + i] = ok[1 + i] ? mask_run_after(rm_of(RL, i), l) : 0;
    }
    const uint32_t cnt = RL.cnt;
    L1[5] = cnt >= 1 ? RL.longest : 0;
    L1[6] = cnt >= 2 ? lane_of(RL.SL, cnt >= 2 ? cnt - 2 : 0) : 0;
    l2[5] = RL.l2a; l2[6] = RL.l2b;
    ok[5] = cnt >= 1 && L1[5] >= 2 && L1[5] <= room && L1[5] <= 61;
    ok[6] = cnt >= 2 && L1[6] >= 2 && L1[6] <= room && L1[6] <= 61;
    const uint32_t dm0 = cnt >= 1 ? lane_of(RL.SD, cnt - 1) : 0, dm1 = cnt >= 2 ? lane_of(RL.SD, cnt - 2) : 0;
    uint64_t m = 0;
    uint32_t vL1 = 0, vl2 = 0, vT = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const uint32_t T = j + L1[k] + 1 + l2[k];
        const bool v = ok[k] && l2[k] >= 2 && T <= WMAX;
        if (v) m |= 1ull << k;
        vL1 = lane == (uint32_t)k ? L1[k] : vL1;
        vl2 = lane == (uint32_t)k ? l2[k] : vl2;
        vT = lane == (uint32_t)k ? T : vT;
    }
    c.L1 = vL1; c.l2 = vl2; c.T = vT;
    c.dist = lane == 1 ? r0 : lane == 2 ? r1 : lane == 3 ? r2 : lane == 4 ? r3 : lane == 5 ? dm0 : dm1;
    c.mask = m;
}

// One window of the optimal parser (oracle: optimum_window).  Returns with the chosen symbol path
// stored as out-edges: node t -> (n_price[t] = back, out-len in n_info[t]); q_end = last node to code
// (a window cut by the node limit only commits the symbols that end WTAIL nodes before the cut).
constexpr uint32_t WTAIL = 32;
template <uint32_t WMAX, class PR>
__device__ __forceinline__ bool optimum_window(const Env& e, const Work& w, ListPre& P, PR probs, const Lz& z, LenTab& lt,
        const uint8_t* __restrict__ in, uint32_t pos, uint32_t block_start, uint32_t span_end, bool cached,
        RoundL& RL, uint32_t& q_end)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t pbm = (1u << z.pb) - 1;
    // Bit-price combinations that depend only on (state, pos_state): lane = state * 4 + pos_state
    // holds all seven of them; a node fetches its set with four readlanes.
    uint32_t c01 = 0, c23 = 0, c45 = 0, c6 = 0;
    {
        const uint32_t s = lane >> 2, ps = lane & 3;
        if (lane < 48 && ps <= pbm) {
            const uint8_t* pt = w.ptab;
            const uint32_t m0 = pr_bit(probs, pt, P_IS_MATCH + s * 16 + ps, 0), m1 = pr_bit(probs, pt, P_IS_MATCH + s * 16 + ps, 1);
            const uint32_t e0 = pr_bit(probs, pt, P_IS_REP + s, 0), e1 = pr_bit(probs, pt, P_IS_REP + s, 1);
            const uint32_t g0 = pr_bit(probs, pt, P_IS_REP0 + s, 0), g1 = pr_bit(probs, pt, P_IS_REP0 + s, 1);
            const uint32_t l0 = pr_bit(probs, pt, P_IS_REP0_LONG + s * 16 + ps, 0), l1 = pr_bit(probs, pt, P_IS_REP0_LONG + s * 16 + ps, 1);
            const uint32_t h0 = pr_bit(probs, pt, P_IS_REP1 + s, 0), h1 = pr_bit(probs, pt, P_IS_REP1 + s, 1);
            const uint32_t k0 = pr_bit(probs, pt, P_IS_REP2 + s, 0), k1 = pr_bit(probs, pt, P_IS_REP2 + s, 1);
            const uint32_t prep = m1 + e1, p11 = prep + g1 + h1;
            c01 = m0 | ((prep + g0 + l0) << 16);                 // literal | short rep
            c23 = (prep + g0 + l1) | ((prep + g1 + h0) << 16);   // rep0 | rep1
            c45 = (p11 + k0) | ((p11 + k1) << 16);               // rep2 | rep3
            c6 = m1 + e0;                                        // match
        }
    }
    for (uint32_t t = 1 + lane; t <= WMAX; t += 64) w.n_price[t] = PRICE_INF;     // once per window, not per node
    if (lane == 0) {
        w.n_price[0] = 0;
        w.n_info[0] = z.state << 9;
    }
    wave_sync();
    uint32_t n_end = 0, j = 0;
    bool next_cached = false, forced = false;
    LitChunk lc;                          // lane = node - (j & ~63): the node's literal prices
    lc.v[0] = lc.v[1] = lc.v[2] = lc.v[3] = lc.v[4] = 0;
    const uint32_t lmask = (0x100u << z.lp) - (0x100u >> z.lc);
    // node 0: the coder's state; its round may be cached from the previous window
    uint32_t s = z.state, r0 = z.rep0, r1 = z.rep1, r2 = z.rep2, r3 = z.rep3, Pj = 0;
    uint32_t b_mb = in[pos - r0 - 1];               // rep0's byte at the node: issued early, used only for a matched literal
    lit_chunk(in, w.ptab, z, pos, block_start, span_end, lc);
    if (!cached) round_lists(e, P, pos, span_end, r0, r1, r2, r3, RL);
    uint32_t longest = RL.longest;
    {
        // a window that opens with a >= nice_len rep or match is that symbol (optimum_normal.c:281-306)
        uint32_t sb = LITERAL, sl = 0;
        if (RL.rl[0] >= e.nice) { sb = 0; sl = RL.rl[0]; }
        else if (RL.rl[1] >= e.nice) { sb = 1; sl = RL.rl[1]; }
        else if (RL.rl[2] >= e.nice) { sb = 2; sl = RL.rl[2]; }
        else if (RL.rl[3] >= e.nice) { sb = 3; sl = RL.rl[3]; }
        else if (longest >= e.nice) { sb = lane_of(RL.SD, RL.cnt - 1) + 4; sl = longest; }
        if (sl) {
            wave_sync();
            if (lane == 0) { w.n_price[0] = sb; w.n_info[0] = (z.state << 9) | (sl << 13); }
            wave_sync();
            q_end = sl;
            return false;
        }
    }
    // The loop is rotated: its body prices the edges out of node j, whose state and round are already there;
    // the state and the round of node j + 1 are fetched at the bottom.
    for (;;) {
        const uint32_t x = pos + j;
        TM_COUNT(w, 9);
        TM_BEGIN(t_bits);
        const uint32_t rp0 = RL.rp[0];
        uint32_t rl0 = RL.rl[0], rl1 = RL.rl[1], rl2 = RL.rl[2], rl3 = RL.rl[3];
        const uint32_t room = WMAX - j;
        const uint32_t avail = span_end - x;
        const uint32_t buf_avail = avail < MATCH_LEN_MAX ? avail : MATCH_LEN_MAX;
        // compound candidates: geometry now, prices after the plain edges.  A cheap necessary condition first
        // (two equal bytes behind the first mismatch of a rep source, or a run recorded with the list): text
        // rarely has any, and then none of the compound code runs.
        Compound cp;
        cp.mask = 0; cp.L1 = cp.l2 = cp.T = cp.dist = 0;
        {
            const bool any = (RL.l2a | RL.l2b) >= 2 || RL.pre;
            if (any) compound_setup(RL, j, room, buf_avail, r0, r1, r2, r3, cp, WMAX);
        }
        uint32_t cT_max = 0;
        for (uint64_t mm = cp.mask; mm; mm &= mm - 1) cT_max = max(cT_max, lane_of(cp.T, (uint32_t)__builtin_ctzll(mm)));
        // the three bytes each compound literal needs (lane = candidate 1..6): the byte itself, its
        // predecessor (literal context) and the match byte X leaves behind
        uint32_t c_bytes = 0;
        if (((cp.mask >> lane) & 1) && lane >= 1) {
            const uint8_t* pl = in + x + cp.L1;
            c_bytes = (uint32_t)pl[0] | ((uint32_t)*(pl - cp.dist - 1) << 8) | ((uint32_t)*(pl - 1) << 16);
        }

        uint32_t rmax = max(max(rl0, rl1), max(rl2, rl3));
        uint32_t reach = max(longest, rmax);
        if (reach > room) {                         // only the last nodes of a window can reach past its end
            longest = min(longest, room);
            rl0 = min(rl0, room); rl1 = min(rl1, room); rl2 = min(rl2, room); rl3 = min(rl3, room);
            rmax = min(rmax, room);
            reach = room;
        }
        n_end = max(max(max(n_end, j + reach), j + 1), cT_max);     // (every node price was set to infinity at the window start)

        const uint32_t upos = x - block_start;
        const uint32_t ps = upos & pbm;
        const uint32_t ci = s * 4 + ps;
        const uint32_t v01 = lane_of(c01, ci), v23 = lane_of(c23, ci), v45 = lane_of(c45, ci), v6 = lane_of(c6, ci);
        TM_END(w, 2, t_bits);

        // compound literal prices: lane = candidate * 8 + bit (candidates 1..6), one gather of the eight
        // probabilities each matched literal would use (literal_matched, lzma_encoder.c:23-41), issued
        // here and summed after the plain edges
        TM_BEGIN(t_cg);
        uint32_t cg_p = 0, cg_flip = 0;
        const bool cg_any = (cp.mask & 0x7Eull) != 0;
        if (cg_any) {
            const uint32_t packed = c_bytes;
            const uint32_t cand = lane >> 3, bit_i = lane & 7;
            const uint32_t pk = (uint32_t)__shfl((int)packed, (int)cand);
            const uint32_t cL = (uint32_t)__shfl((int)cp.L1, (int)cand);
            const bool act = cand >= 1 && cand <= 6 && ((cp.mask >> cand) & 1);
            const uint32_t cur = pk & 0xFFu, mb = (pk >> 8) & 0xFFu, prev = (pk >> 16) & 0xFFu;
            const uint32_t up = upos + cL;
            const uint32_t sub = 3u * ((((up << 8) + prev) & lmask) << z.lc);
            const uint32_t pre = (0x100u | cur) >> (8 - bit_i);
            const bool same = (mb >> (8 - bit_i)) == (cur >> (8 - bit_i));
            const uint32_t idx = same ? 0x100u + (((mb >> (7 - bit_i)) & 1u) << 8) + pre : pre;
            const uint32_t bit = (cur >> (7 - bit_i)) & 1u;
            cg_flip = (0u - bit) & 0x7FFu;
            if (act) cg_p = lit_load(z.lit + sub + idx);
        }
        TM_END(w, 15, t_cg);

        TM_BEGIN(t_lit);
        // literal and short rep -> node j+1
        const uint32_t lp = lit_price(lc, j & 63, s, s < 7 ? 0u : uni(b_mb));
        const uint32_t plit = Pj + (v01 & 0xFFFFu) + lp;
        {
            uint32_t best = uni(w.n_price[j + 1]), bb = 0, ns = 0;
            bool upd = false;
            if (plit < best) { best = plit; bb = LITERAL; upd = true; ns = s <= 3 ? 0 : (s <= 9 ? s - 3 : s - 6); }
            if (rp0 >= 1) {
                const uint32_t psr = Pj + (v01 >> 16);
                if (psr < best) { best = psr; bb = 0; upd = true; ns = s < 7 ? 9u : 11u; }
            }
            if (upd && lane == 0) {
                w.n_price[j + 1] = best; w.n_info[j + 1] = 1 | (ns << 9) | ((bb == LITERAL ? 5u : 0u) << 22);
                w.n_reps4[j + 1] = make_uint4(r0, r1, r2, r3);
            }
            wave_sync();
        }
        // Node j + 1 is final now (every other edge out of j is longer): its rows go out here and are in flight
        // while the length and compound edges of node j are priced.
        Rows NW;
        uint32_t n_mb = 0;
        const bool rows_early = j + 1 != n_end;
        if (rows_early) {
            const uint4 nr = w.n_reps4[j + 1];
            n_mb = in[x - nr.x];                         // in[(x + 1) - rep0 - 1]
            rows_issue(e, x + 1, span_end, nr.x, nr.y, nr.z, nr.w, NW);
        }
        TM_END(w, 3, t_lit);
        TM_BEGIN(t_relax);
        const uint32_t prep0 = Pj + (v23 & 0xFFFFu), prep1 = Pj + (v23 >> 16), prep2 = Pj + (v45 & 0xFFFFu), prep3 = Pj + (v45 >> 16);
        const uint32_t pmatch = Pj + v6;
        if (reach >= 2) {
            relax_lengths(w, lt, ps & 3, RL.SL, RL.SD, j, reach, longest, RL.cnt, rl0, rl1, rl2, rl3,
                    prep0, prep1, prep2, prep3, pmatch, s, r0, r1, r2, r3);
            wave_sync();
        }
        TM_END(w, 4, t_relax);

        TM_BEGIN(t_cp);
        if (cp.mask) {
            TM_COUNT(w, 13);
            // ---- price the compound candidates, lane = candidate ----
            // length prices: LenTab holds length 2 + l + 64 * it in lane l (low half match, high half rep)
            const uint32_t lo_ps = (ps & 3) == 0 ? lt.lo[0] : (ps & 3) == 1 ? lt.lo[1] : (ps & 3) == 2 ? lt.lo[2] : lt.lo[3];
            const uint32_t i1 = lane < 7 && cp.L1 >= 2 ? cp.L1 - 2 : 0u;          // L1 <= 63: first pass of the table
            const uint32_t t_lo = (uint32_t)__shfl((int)lo_ps, (int)(i1 & 63)), t_hi0 = (uint32_t)__shfl((int)lt.hi[0], (int)(i1 & 63));
            const uint32_t lenX = i1 < 16 ? t_lo : t_hi0;                           // X's length price (match | rep << 16)
            const uint32_t i2 = lane < 7 && cp.l2 >= 2 ? cp.l2 - 2 : 0u;            // l2 <= 127
            const uint32_t psn = (upos + cp.L1 + 1) & pbm & 3;
            const uint32_t u0 = (uint32_t)__shfl((int)lt.lo[0], (int)(i2 & 63)), u1 = (uint32_t)__shfl((int)lt.lo[1], (int)(i2 & 63));
            const uint32_t u2 = (uint32_t)__shfl((int)lt.lo[2], (int)(i2 & 63)), u3 = (uint32_t)__shfl((int)lt.lo[3], (int)(i2 & 63));
            const uint32_t h0v = (uint32_t)__shfl((int)lt.hi[0], (int)(i2 & 63)), h1v = (uint32_t)__shfl((int)lt.hi[1], (int)(i2 & 63));
            const uint32_t ulo = psn == 0 ? u0 : psn == 1 ? u1 : psn == 2 ? u2 : u3;
            const uint32_t len2p = (i2 < 16 ? ulo : i2 < 64 ? h0v : h1v) >> 16;     // rep length price of the rep0 run
            // state chain: X -> literal -> long rep0
            const bool isrep = lane >= 1 && lane <= 4;
            const uint32_t sX = lane == 0 ? s : isrep ? (s < 7 ? 8u : 11u) : (s < 7 ? 7u : 10u);
            const uint32_t sL = lane == 0 ? (s <= 3 ? 0u : (s <= 9 ? s - 3 : s - 6)) : isrep ? 5u : 4u;   // state after the literal
            const uint32_t psl = (upos + cp.L1) & pbm & 3;
            const uint32_t m0X = (uint32_t)__shfl((int)c01, (int)(sX * 4 + psl)) & 0xFFFFu;               // is_match = 0 before the literal
            const uint32_t rafter = ((uint32_t)__shfl((int)c23, (int)(sL * 4 + psn)) & 0xFFFFu) + len2p;  // rep0 behind the literal
            // price of X
            uint32_t pX;
            {
                const uint32_t dist_m = cp.dist;
                const uint32_t l = cp.L1;
                const uint32_t ds = l < 6 ? (l >= 2 ? l - 2 : 0u) : 3u;
                const uint32_t dnz = dist_m < 4 ? 4u : dist_m;
                const uint32_t di = 31 - (uint32_t)__builtin_clz(dnz);
                const uint32_t slot = dist_m < 4 ? dist_m : 2 * di + ((dnz >> (di - 1)) & 1);
                const bool ism = lane == 5 || lane == 6;
                const uint32_t p_dist = ism ? (uint32_t)w.dsp[ds * 64 + slot] + w.xt[dist_m < 128 ? dist_m : 128 + (dist_m & 15)] : 0u;
                const uint32_t prep_i = lane == 1 ? prep0 : lane == 2 ? prep1 : lane == 3 ? prep2 : prep3;
                pX = ism ? pmatch + (lenX & 0xFFFFu) + p_dist : prep_i + (lenX >> 16);
            }
            // matched-literal prices: sum the eight bit prices of each candidate's group of lanes
            uint32_t litp = 0;
            if (cg_any) {
                uint32_t bp = w.ptab[(cg_p ^ cg_flip) >> 4];
                const uint32_t cand = lane >> 3;
                if (!(cand >= 1 && cand <= 6 && ((cp.mask >> cand) & 1))) bp = 0;
                bp += (uint32_t)__shfl_xor((int)bp, 1);
                bp += (uint32_t)__shfl_xor((int)bp, 2);
                bp += (uint32_t)__shfl_xor((int)bp, 4);
                litp = (uint32_t)__shfl((int)bp, (int)((lane < 7 ? lane : 0u) * 8));
            }
            const uint32_t cprice = lane == 0 ? plit + rafter : pX + m0X + litp + rafter;
            // apply in candidate order (strict <, like every other edge)
            for (uint64_t mm = cp.mask; mm; mm &= mm - 1) {
                const uint32_t c = (uint32_t)__builtin_ctzll(mm);
                const uint32_t T = lane_of(cp.T, c), pr = lane_of(cprice, c);
                const uint32_t curp = uni(w.n_price[T]);
                if (pr < curp) {
                    const uint32_t cL = lane_of(cp.L1, c), cl2 = lane_of(cp.l2, c), cd = lane_of(cp.dist, c);
                    const uint32_t kind = c == 0 ? 5u : c <= 4 ? c - 1 : 4u;
                    uint4 nr;
                    if (c == 0) nr = make_uint4(r0, r1, r2, r3);
                    else if (c == 1) nr = make_uint4(r0, r1, r2, r3);
                    else if (c == 2) nr = make_uint4(r1, r0, r2, r3);
                    else if (c == 3) nr = make_uint4(r2, r0, r1, r3);
                    else if (c == 4) nr = make_uint4(r3, r0, r1, r2);
                    else nr = make_uint4(cd, r0, r1, r2);
                    if (lane == 0) {
                        w.n_price[T] = pr;
                        w.n_info[T] = cL | (8u << 9) | (kind << 22) | (cl2 << 25);
                        w.n_reps4[T] = nr;
                    }
                }
                wave_sync();
            }
        }
        TM_END(w, 14, t_cp);
        ++j;
        if (j == n_end) { forced = j >= WMAX; break; }
        // state and round of the next node
        {
            TM_BEGIN(t_derive);
            const uint4 rr = w.n_reps4[j];
            s = (uni(w.n_info[j]) >> 9) & 15;
            Pj = uni(w.n_price[j]);
            r0 = uni(rr.x); r1 = uni(rr.y); r2 = uni(rr.z); r3 = uni(rr.w);
            TM_END(w, 0, t_derive);
            TM_BEGIN(t_round);
            const uint32_t xn = pos + j;
            b_mb = n_mb;                                   // rows and rep0 byte of this node: issued by its predecessor
            if ((j & 63) == 0) lit_chunk(in, w.ptab, z, xn, block_start, span_end, lc);
            round_lists_rows(e, P, xn, span_end, r0, r1, r2, r3, NW, RL);
            longest = RL.longest;
            TM_END(w, 1, t_round);
            if (longest >= e.nice) { next_cached = true; break; }
        }
    }
    TM_BEGIN(t_back);
    // backtrack from node j: turn in-edges into out-edges.  A compound in-edge becomes three (two when
    // X is empty) out-edges through its intermediate nodes.  `cut` = largest symbol boundary that lies
    // at least WTAIL nodes before a forced window end, `first` = end of the first symbol.
    if (lane == 0) {
        const uint32_t limit = j >= WTAIL ? j - WTAIL : 0;
        uint32_t t = j, cut = 0, first = j;
        while (t > 0) {
            const uint32_t info = w.n_info[t];
            const uint32_t ilen = info & 0x1FF, kind = (info >> 22) & 7, cl2 = info >> 25;
            const uint32_t bk = kind < 4 ? kind : kind == 4 ? w.n_reps4[t].x + 4 : LITERAL;
            const uint32_t pv = t - ilen - (cl2 ? 1 + cl2 : 0);
            if (cut == 0 && t <= limit) cut = t;
            first = t;
            if (cl2) {
                const uint32_t a = pv + ilen;                 // node of the literal, a + 1 = start of the rep0 run
                w.n_price[a + 1] = 0;                          // rep0
                w.n_info[a + 1] = cl2 << 13;
                if (cut == 0 && a + 1 <= limit) cut = a + 1;
                first = a + 1;
                if (ilen) {
                    w.n_price[a] = LITERAL;
                    w.n_info[a] = 1u << 13;
                    if (cut == 0 && a <= limit) cut = a;
                    first = a;
                    w.n_price[pv] = bk;
                    w.n_info[pv] = (w.n_info[pv] & 0xFFC01FFFu) | (ilen << 13);
                } else {
                    w.n_price[pv] = LITERAL;                   // X empty: the literal leaves pv itself
                    w.n_info[pv] = (w.n_info[pv] & 0xFFC01FFFu) | (1u << 13);
                }
            } else {
                w.n_price[pv] = bk;
                w.n_info[pv] = (w.n_info[pv] & 0xFFC01FFFu) | (ilen << 13);   // keep in-len, state, in-edge kind and len2 of pv
            }
            t = pv;
        }
        w.n_info[WMAX + 1] = (forced && pos + j < span_end) ? (cut ? cut : first) : j;   // spare word behind the node arrays
    }
    wave_sync();
    q_end = uni(w.n_info[WMAX + 1]);
    TM_END(w, 5, t_back);
    TM_COUNT(w, 11);
    return next_cached;
}

// ------------------------------------------------------------------------------------------
// Span encoder: one wavefront per span.  FINDER 0 = exact HC3/HC4 of the reference evaluated inside
// the kernel (fast parser), 2 = per-position match lists written by k_find_sn / k_find_exact;
// OPT selects the parser (false = optimum_fast of the reference).
// ------------------------------------------------------------------------------------------
template <int FINDER, bool OPT, uint32_t WMAX>      // FINDER: 0 = exact HC3/HC4 in-kernel, 2 = lists from the batch finders
#ifndef XZAMD_WAVES_FAST
#define XZAMD_WAVES_FAST 4
#endif
#ifndef XZAMD_WALK_LITG_DEFAULT
#define XZAMD_WALK_LITG_DEFAULT true
#endif
#ifndef XZAMD_WAVES_OPT
#define XZAMD_WAVES_OPT 4
#endif
__device__ __forceinline__ void span_encode_one(const xzamd_span_args& a, const uint32_t span)
{
    constexpr bool LISTS = FINDER == 2;
    static_assert(!LISTS || OPT, "the fast parsers run with the in-kernel finders");
    // One LDS pool, carved by hand (a single __shared__ object: no aliasing or ordering surprises).
    constexpr uint32_t W_PROBS = 928;                                    // 1856 x u16 >= P_LITERAL (1846): all but the literal coders
    constexpr uint32_t W_LIST = 0;
    constexpr uint32_t W_NODES = OPT ? 6 * (WMAX + 1) + 2 : 0;           // reps[4], price, info (16-byte multiple)
    constexpr uint32_t W_TABS = OPT ? (128 + 72 + 32) : 0;               // dsp, xt + ap (u16), ptab (u8)
#ifndef XZAMD_LDS_PAD_WORDS
#define XZAMD_LDS_PAD_WORDS 0        /* occupancy experiments only */
#endif
    __shared__ __attribute__((aligned(16))) uint32_t pool[W_PROBS + W_LIST + W_NODES + W_TABS + XZAMD_LDS_PAD_WORDS];
#ifdef XZAMD_TIMING
    __shared__ unsigned long long tm_lds[16];
    if (threadIdx.x < 16) tm_lds[threadIdx.x] = 0;
#endif
    uint16_t* const probs = reinterpret_cast<uint16_t*>(pool);
    const uint32_t lane = threadIdx.x;
    const uint32_t blk = span / a.max_spb;
    const uint32_t k = span - blk * a.max_spb;
    if (k >= a.span_cnt[blk]) return;                  // an unused slot of the span plan
    const uint32_t block_start = blk * a.block_size;
    const uint32_t block_end = min(a.n, block_start + a.block_size);
    const uint32_t span_start = uni(a.span_tab[2 * span]), span_end = uni(a.span_tab[2 * span + 1]);
    // scratch of the slot: 9/8 of the input bytes in front of it plus XZAMD_SPAN_SLACK per slot (kernels_api.h)
    uint8_t* const outp = a.scratch + ((((uint64_t)span_start + (span_start >> 3)) + 15) & ~15ull) + (uint64_t)span * XZAMD_SPAN_SLACK;
    const uint32_t span_cap = (span_end - span_start) + ((span_end - span_start) >> 3) + 4096;
    const uint8_t* __restrict__ in = a.in;

    Env e;
    e.in = in; e.rank = a.rank; e.sorted_pos = a.sorted_pos; e.prev2 = a.prev2; e.prev3 = a.prev3;
    e.nice = a.nice_len; e.depth = a.depth; e.hb = a.hash_bytes; e.cyclic = a.dict_size + 1;
    e.block_end = block_end; e.n_last = a.n - 1;
    e.mlen = a.mlen; e.mdist = a.mdist; e.packed = a.list_packed;
    ListPre LP;
    LP.valid = false; LP.pos = 0; LP.v = LP.l16 = 0;
    Pre P;
    P.valid = false; P.pos = 0; P.ent = 0;
    P.a.rk = P.a.d2 = P.a.d3 = 0; P.an = P.a;

    Work w{};
    if constexpr (OPT) {
        uint32_t* nb = pool + W_PROBS + W_LIST;
        w.n_reps4 = reinterpret_cast<uint4*>(nb);           // 16-byte aligned: W_PROBS * 4 is a multiple of 16
        w.n_price = nb + 4 * (WMAX + 1);
        w.n_info = nb + 5 * (WMAX + 1);
        uint32_t* tb = nb + W_NODES;
        w.dsp = reinterpret_cast<uint16_t*>(tb);            // 256 x u16 = 128 words
        w.xt = reinterpret_cast<uint16_t*>(tb + 128);       // 128 x u16 = 64 words
        w.ap = w.xt + 128;                                  // 16 x u16 = 8 words, contiguous with xt
        w.ptab = reinterpret_cast<uint8_t*>(tb + 200);      // 128 x u8 = 32 words
        w.err = a.err;
#ifdef XZAMD_TIMING
        w.tm = tm_lds;
#endif
        // bit price table (price_tablegen.c:31-58)
        for (uint32_t t = lane; t < 128; t += 64) {
            uint32_t wv = t * 16 + 8, bit_count = 0;
            for (int jj = 0; jj < 4; ++jj) {
                wv *= wv;
                bit_count <<= 1;
                while (wv >= (1u << 16)) { wv >>= 1; ++bit_count; }
            }
            w.ptab[t] = (uint8_t)((11 << 4) - 15 - bit_count);
        }
        wave_sync();
        w.ptv = reinterpret_cast<const uint32_t*>(w.ptab)[lane & 31];
    }

    Lz z;
    block_lclp(a, blk, z.lc, z.lp); z.pb = a.pb;
    z.cnt_len = z.cnt_match = z.cnt_align = 0;
    const uint32_t lit_size = 0x300u << (a.lc + a.lp);       // literal coders of this span (lc + lp <= 4)
    z.lit = reinterpret_cast<plit_t*>(a.lit) + (uint64_t)span * lit_size;
    z.gp = nullptr;
    RC rc;
    rc.cpos = 0; rc.out = outp; rc.reset();

    bool need_props = true, need_dict_reset = (span_start == block_start), need_state_reset = true;
    bool initialized = (span_start != block_start);
    uint32_t cur = span_start;
    uint32_t read_ahead = 0;        // exact/fast path bookkeeping (as in the reference)
    bool cached = false;            // list paths: the round for `cur` has been done
    uint32_t out_off = 0;
    Round R;            // exact path: cached find at `cur` when read_ahead == 1
    R.mask = 0; R.L = 0; R.D = 0; R.longest = 0;
    RoundL RL;
    RL.L = 0; RL.SL = 0; RL.SD = 0; RL.cnt = 0; RL.longest = 0; RL.l2a = RL.l2b = 0;
    RL.rp[0] = RL.rp[1] = RL.rp[2] = RL.rp[3] = 0;
    RL.mlo = RL.mhi = 0;
    RL.rl[0] = RL.rl[1] = RL.rl[2] = RL.rl[3] = 0;
    RL.pre = 0;
    LenTab lt;
    uint32_t q_pos = 0, q_end = 0;  // pending path of the optimal parser (nodes in LDS)
    bool tables_valid = false;
#ifdef XZAMD_TIMING
    uint64_t tm_round1 = 0, tm_round2 = 0, tm_encode = 0, tm_rounds = 0, tm_syms = 0;
    const uint64_t tm_start = __builtin_amdgcn_s_memtime();
#endif

    while (cur < span_end) {
        if (need_state_reset) {
            // lzma_lzma_encoder_reset (lzma_encoder.c:529-598)
            uint32_t* p32 = reinterpret_cast<uint32_t*>(probs);
            for (uint32_t i = lane; i < 928; i += 64) p32[i] = 0x04000400u;
            {
                uint4* l4 = reinterpret_cast<uint4*>(z.lit);
                const uint4 v = PLIT_FLAT4;
                for (uint32_t i = lane; i < lit_size / PLIT_PER_U4; i += 64) l4[i] = v;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            wave_sync();
            z.state = 0; z.rep0 = z.rep1 = z.rep2 = z.rep3 = 0;
            tables_valid = false;
            q_pos = q_end = 0;
            // the flag stays set until an LZMA chunk header has announced the reset
        }
        const uint32_t chunk_start = cur;
        const uint32_t hl = need_props ? 6 : 5;
        rc.out = outp + out_off + hl;
        rc.cpos = 0;
        rc.reset();

        if (!initialized) {
            // encode_init (lzma_encoder.c:267-293)
            encode_symbol(rc, probs, z, in, block_start, 0, LITERAL, 1);
            cur = block_start + 1;
            initialized = true;
        }

        for (;;) {
            // lzma_encoder.c:346-351 (limit from lzma2_encoder.c:167-181)
            if (cur - chunk_start >= (1u << 21) - MATCH_LEN_MAX
                    || rc.cpos + rc.cache_size + 4 >= 65536 - 4097)
                break;
            if (cur >= span_end)
                break;

            uint32_t back = LITERAL, len = 1;
            if constexpr (OPT) {
                if (q_pos == q_end) {
                    // price-table refresh policy (oracle: refresh_tables)
                    TM_BEGIN(t_refresh);
                    if (!tables_valid || z.cnt_len >= 64) { refresh_len_tables(probs, w.ptab, lt, 1u << z.pb, reinterpret_cast<uint32_t*>(w.n_reps4)); z.cnt_len = 0; }
                    if (!tables_valid || z.cnt_match >= 128) { refresh_dist_tables(probs, w); z.cnt_match = 0; }
                    if (!tables_valid || z.cnt_align >= 16) { refresh_align_table(probs, w); z.cnt_align = 0; }
                    tables_valid = true;
                    TM_END(w, 7, t_refresh);
                    // Node 0's round is done here so that a window opening with a >= nice_len rep or
                    // match (optimum_window's j == 0 rule; the common case in binary data) is coded
                    // straight away, without building the window's price tables.
                    if (!cached) {
                        round_lists(e, LP, cur, span_end, z.rep0, z.rep1, z.rep2, z.rep3, RL);
                        cached = true;
                    }
                    uint32_t sb = LITERAL, sl = 0;
                    if (RL.rp[0] >= e.nice) { sb = 0; sl = RL.rp[0]; }
                    else if (RL.rp[1] >= e.nice) { sb = 1; sl = RL.rp[1]; }
                    else if (RL.rp[2] >= e.nice) { sb = 2; sl = RL.rp[2]; }
                    else if (RL.rp[3] >= e.nice) { sb = 3; sl = RL.rp[3]; }
                    else if (RL.longest >= e.nice) { sb = lane_of(RL.SD, RL.cnt - 1) + 4; sl = RL.longest; }
                    if (sl) {
                        back = sb; len = sl;
                        cached = false;
                        q_pos = q_end = 0;
                    } else if (RL.cnt == 0 && RL.rp[0] == 0 && RL.rp[1] < 2 && RL.rp[2] < 2 && RL.rp[3] < 2
                            && mask_run_after(rm_of(RL, 0), 0) < 2) {
                        // nothing but a literal can leave node 0 (no match, no rep of two bytes, not even
                        // a short rep, no "literal + rep0" compound): the window would be that literal
                        // (incompressible data lives here)
                        cached = false;
                        q_pos = q_end = 0;
                    } else {
                        cached = optimum_window<WMAX>(e, w, LP, probs, z, lt, in, cur, block_start, span_end, cached, RL, q_end);
                        q_pos = 0;
                        if (q_end == 0) {            // consistency failure reported by the parser
                            if (lane == 0) a.span_bytes[span] = 0;
                            return;
                        }
                    }
                }
                if (q_pos != q_end) {
                    back = uni(w.n_price[q_pos]);
                    len = (uni(w.n_info[q_pos]) >> 13) & 0x1FF;
                    q_pos += len;
                }
            } else {
            // ---------------- lzma_lzma_optimum_fast (optimum_fast.c:20-169) ----------------
#ifdef XZAMD_TIMING
            const uint64_t tt0 = __builtin_amdgcn_s_memtime();
#endif
            if (read_ahead == 0) {
                do_round(e, P, cur, span_end, z.rep0, z.rep1, z.rep2, z.rep3, R);
                read_ahead = 1;
#ifdef XZAMD_TIMING
                ++tm_rounds;
#endif
            }
#ifdef XZAMD_TIMING
            const uint64_t tt1 = __builtin_amdgcn_s_memtime();
            tm_round1 += tt1 - tt0;
#endif
            {
                const uint32_t rem = span_end - cur;
                const uint32_t buf_avail = rem < MATCH_LEN_MAX ? rem : MATCH_LEN_MAX;
                uint32_t len_main = R.longest;
                uint64_t m = R.mask;
                bool decided = false;
                if (buf_avail < 2) decided = true;          // literal

                uint32_t rep_len = 0, rep_index = 0;
                if (!decided) {
                    for (uint32_t i = 0; i < 4; ++i) {
                        const uint32_t rl = lane_of(R.L, 60 + i);
                        if (rl < 2) continue;
                        if (rl >= e.nice) {
                            back = i; len = rl; read_ahead += rl - 1; decided = true;
                            break;
                        }
                        if (rl > rep_len) { rep_index = i; rep_len = rl; }
                    }
                }
                if (!decided && len_main >= e.nice) {
                    const uint32_t top = 63 - (uint32_t)__builtin_clzll(m);
                    back = lane_of(R.D, top) + 4; len = len_main; read_ahead += len_main - 1;
                    decided = true;
                }
                uint32_t back_main = 0;
                if (!decided) {
                    if (len_main >= 2) {
                        uint32_t top = 63 - (uint32_t)__builtin_clzll(m);
                        back_main = lane_of(R.D, top);
                        while (__builtin_popcountll(m) > 1) {
                            const uint64_t m2 = m & ~(1ull << top);
                            const uint32_t t2 = 63 - (uint32_t)__builtin_clzll(m2);
                            const uint32_t l2 = lane_of(R.L, t2);
                            if (len_main != l2 + 1) break;
                            const uint32_t d2 = lane_of(R.D, t2);
                            if (!change_pair(d2, back_main)) break;
                            m = m2; top = t2; len_main = l2; back_main = d2;
                        }
                        if (len_main == 2 && back_main >= 0x80) len_main = 1;
                    }
                    if (rep_len >= 2) {
                        if (rep_len + 1 >= len_main
                                || (rep_len + 2 >= len_main && back_main > (1u << 9))
                                || (rep_len + 3 >= len_main && back_main > (1u << 15))) {
                            back = rep_index; len = rep_len; read_ahead += rep_len - 1;
                            decided = true;
                        }
                    }
                }
                if (!decided && (len_main < 2 || buf_avail <= 2)) decided = true;   // literal
                if (!decided) {
                    // lookahead: matches (and rep lengths) of the next byte
#ifdef XZAMD_TIMING
                    const uint64_t tl0 = __builtin_amdgcn_s_memtime();
#endif
                    do_round(e, P, cur + 1, span_end, z.rep0, z.rep1, z.rep2, z.rep3, R);
#ifdef XZAMD_TIMING
                    tm_round2 += __builtin_amdgcn_s_memtime() - tl0;
                    ++tm_rounds;
#endif
                    ++read_ahead;
                    const uint32_t nl = R.longest;
                    bool lit = false;
                    if (nl >= 2) {
                        const uint32_t top = 63 - (uint32_t)__builtin_clzll(R.mask);
                        const uint32_t new_dist = lane_of(R.D, top);
                        if ((nl >= len_main && new_dist < back_main)
                                || (nl == len_main + 1 && !change_pair(back_main, new_dist))
                                || (nl > len_main + 1)
                                || (nl + 1 >= len_main && len_main >= 3 && change_pair(new_dist, back_main)))
                            lit = true;
                    }
                    if (!lit) {
                        const uint32_t limit = len_main - 1 > 2 ? len_main - 1 : 2;
                        for (uint32_t i = 0; i < 4; ++i)
                            if (lane_of(R.L, 60 + i) >= limit) lit = true;
                    }
                    if (!lit) { back = back_main + 4; len = len_main; read_ahead += len_main - 2; }
                }
            }
            read_ahead -= len;
            // ------------------------------------------------------------------------------
            }
            if (len == 0 || len > MATCH_LEN_MAX || cur + len > span_end
                    || (back != LITERAL && back >= 4 && back - 4 >= cur - block_start)
                    || out_off + hl + rc.cpos + 64 > span_cap) {
                // internal consistency failure: report instead of corrupting memory
                if (lane == 0 && a.err) {
                    if (atomicCAS(a.err, 0u, 1u) == 0u) {
                        a.err[1] = span; a.err[2] = cur - block_start; a.err[3] = back; a.err[4] = len;
                        a.err[5] = q_pos; a.err[6] = q_end; a.err[7] = out_off + rc.cpos;
                    }
                }
                if (lane == 0) a.span_bytes[span] = 0;
                return;
            }
#ifdef XZAMD_TIMING
            const uint64_t te0 = __builtin_amdgcn_s_memtime();
#endif
            encode_symbol(rc, probs, z, in, cur, cur - block_start, back, len);
#ifdef XZAMD_TIMING
            tm_encode += __builtin_amdgcn_s_memtime() - te0;
            ++tm_syms;
            if constexpr (OPT) { if (lane == 0) { tm_lds[6] += __builtin_amdgcn_s_memtime() - te0; tm_lds[10] += 1; } }
#endif
            if (a.trace && lane == 0) {
                // debug only: symbol stream for the parity tests (compared with the oracle's parse)
                const uint32_t ti = atomicAdd(a.trace_count, 1u);
                if (ti < a.trace_cap) {
                    a.trace[4 * ti] = span;
                    a.trace[4 * ti + 1] = cur - block_start;
                    a.trace[4 * ti + 2] = back;
                    a.trace[4 * ti + 3] = len;
                }
            }
            cur += len;
        }
        rc.flush();

        uint32_t usize = cur - chunk_start;
        const uint32_t csize = rc.cpos;
        uint8_t* const hdr = outp + out_off;
        if (csize >= usize) {
            // lzma2_encoder.c:205-214: store the chunk raw.  Fast parser: including the lookahead
            // byte; optimal parser: pending symbols are dropped and re-parsed after the reset.
            if constexpr (!OPT) {
                usize += read_ahead;
                cur += read_ahead;
            }
            read_ahead = 0;
            cached = false;
            q_pos = q_end = 0;
            // the discarded range-coder bytes were stored by lane 0; make sure they have landed
            // before other lanes overwrite the same addresses
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (uint32_t i = lane; i < usize; i += 64) hdr[3 + i] = in[chunk_start + i];
            if (lane == 0) {
                hdr[0] = need_dict_reset ? 1 : 2;
                hdr[1] = (uint8_t)((usize - 1) >> 8);
                hdr[2] = (uint8_t)(usize - 1);
            }
            need_dict_reset = false;
            need_state_reset = true;
            out_off += 3 + usize;
            continue;
        }
        // lzma2_header_lzma (lzma2_encoder.c:54-106)
        if (lane == 0) {
            uint32_t c;
            if (need_props) c = need_dict_reset ? 0xE0 : 0xC0;
            else c = need_state_reset ? 0xA0 : 0x80;
            hdr[0] = (uint8_t)(c + ((usize - 1) >> 16));
            hdr[1] = (uint8_t)((usize - 1) >> 8);
            hdr[2] = (uint8_t)(usize - 1);
            hdr[3] = (uint8_t)((csize - 1) >> 8);
            hdr[4] = (uint8_t)(csize - 1);
            if (need_props) hdr[5] = (uint8_t)((a.pb * 5 + z.lp) * 9 + z.lc);
        }
        need_props = false; need_dict_reset = false; need_state_reset = false;
        out_off += hl + csize;
    }
    if (lane == 0) a.span_bytes[span] = out_off;
#ifdef XZAMD_TIMING
    if constexpr (OPT) {
        if (lane == 0 && a.err) {
            tm_lds[8] = __builtin_amdgcn_s_memtime() - tm_start;
            {   // per-span record for tools/gpu_span_times.py, in the (now dead) literal-coder slice of the span
                uint32_t hw_id;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
                uint32_t xcc_id;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
                uint32_t* zl = reinterpret_cast<uint32_t*>(z.lit);
                zl[0] = 0x54494D45u; zl[1] = (uint32_t)tm_lds[8]; zl[2] = (uint32_t)(tm_lds[8] >> 32);
                zl[3] = hw_id; zl[4] = xcc_id; zl[5] = (uint32_t)tm_lds[9]; zl[6] = (uint32_t)(tm_start >> 10);
                zl[7] = span_end - span_start;
            }
            unsigned long long* g = reinterpret_cast<unsigned long long*>(a.err + 16);
            for (int i = 0; i < 12; ++i) atomicAdd(g + i, tm_lds[i]);
            atomicMax(g + 12, tm_lds[8]);
            atomicAdd(g + 13, tm_lds[13]);
            atomicAdd(g + 14, tm_lds[14]);
            atomicAdd(g + 15, tm_lds[15]);
        }
    }
    if (lane == 0 && span == 0 && a.err) {
        const uint64_t tot = __builtin_amdgcn_s_memtime() - tm_start;
        a.err[8] = (uint32_t)(tot >> 8); a.err[9] = (uint32_t)(tm_round1 >> 8); a.err[10] = (uint32_t)(tm_round2 >> 8);
        a.err[11] = (uint32_t)(tm_encode >> 8); a.err[12] = (uint32_t)tm_rounds; a.err[13] = (uint32_t)tm_syms;
    }
#endif
}

// Persistent form: a launch has at most as many wavefronts as the GPU holds at once (the host passes the
// count); each pulls span numbers from a counter until none is left, so a launch is not a sequence of rounds
// of equally long spans and fewer resident wavefronts can be asked for (leaving room for other streams).
template <int FINDER, bool OPT, uint32_t WMAX = WMAX_STD>
__global__ __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(OPT ? 2 : XZAMD_WAVES_FAST, OPT ? 2 : XZAMD_WAVES_FAST)))      // OPT: the single-phase optimal kernel keeps its model in LDS (14 KiB per wave); a test mode
void k_span_encode_t(xzamd_span_args a, uint32_t nspans, uint32_t* __restrict__ counter)
{
    for (;;) {
        uint32_t s = blockIdx.x;            // counter == nullptr: one wavefront per span
        if (counter != nullptr) {
            if (threadIdx.x == 0) s = atomicAdd(counter, 1u);
            s = uni(s);
        }
        if (s >= nspans) break;
        span_encode_one<FINDER, OPT, WMAX>(a, a.order ? a.order[s] : s);
        if (counter == nullptr) break;
        __builtin_amdgcn_s_waitcnt(0);      // this span's stores are out before the LDS pool is reused
        wave_sync();
    }
}

// ------------------------------------------------------------------------------------------
// Two-phase mode (oracle: parse_piece / parse_block / snapshot_walk / encode_block_syms).  The optimal parser is the
// expensive part and needs thousands of independent units to fill the GPU; the coder is cheap, but every reset of its
// model costs output bytes -- and a parser that prices with the wrong model chooses badly.  So the two are decoupled:
//   k_parse_pieces   one wavefront per PIECE of the span plan: optimum_window with an adaptive price model that codes
//                    nothing.  The first XZAMD_SEED_LEN bytes of every Block are the seed piece (phase 0, flat model).
//                    Iteration 1 (XZAMD_ITER_PARTIAL): the first eighth of every other piece, from the seed's model + a
//                    greedy warm-up walk + a pre-roll; iteration 2 (XZAMD_ITER_SNAP): every piece in full from the snapshot
//                    the carried model walk over iteration 1's records left in its slot.  Symbols are recorded per position
//                    in a coder-independent form: (length, distance) or literal bytes.
//   k_model_walk     one wavefront per ENCODE SPAN (>= 256 KiB of input): the recorded symbols through the coder's model
//                    (all of it in LDS), rep / short rep / match chosen from the coder's own rep distances.  <1>, <2>: the
//                    bounds of every probability whatever the span's start model is; k_model_chain: the true model at every
//                    span start -- ONE continuous model per Block; <0>: tokens and the LZMA2 chunk table; <3>: snapshots.
//   k_rc_chunks      one LANE per LZMA2 chunk: the range coder over the chunk's tokens.
// ------------------------------------------------------------------------------------------
// The stage of a launch (xzk_parse_pieces picks it from `phase` and a.iter): what a piece starts from and where it ends are
// compile-time facts of the instance, so each kernel carries the code of its own stage only -- the generic kernel kept the
// walk, the pre-roll and the prior copy live (in registers) across the node loop of launches that never run them.
//   SEED        phase 0: flat model, the whole seed piece; serves both halves of pinfo
//   PART_PRIOR  XZAMD_ITER_PARTIAL: the seed's prior + warm-up walk + pre-roll, ends at part_tab; lane-0 half of pinfo
//   PART_SNAP   PARTIAL | SNAP (part_iters > 1): from the snapshot, ends at part_tab; lane-0 half of pinfo
//   FULL        XZAMD_ITER_SNAP: from the snapshot, the whole piece; lane-1 half of pinfo
enum ParseStage : int { STAGE_SEED = 0, STAGE_PART_PRIOR = 1, STAGE_PART_SNAP = 2, STAGE_FULL = 3 };

template <uint32_t WMAX, bool PACKED, ParseStage STAGE>
__device__ __forceinline__ void parse_piece_one(const xzamd_span_args& a, const uint32_t span)
{
    constexpr bool SEED = STAGE == STAGE_SEED;
    constexpr bool PRIOR = STAGE == STAGE_PART_PRIOR;                    // prior copy, warm-up walk, pre-roll
    constexpr bool PARTIAL = STAGE == STAGE_PART_PRIOR || STAGE == STAGE_PART_SNAP;
    constexpr bool FROM_SNAP = STAGE == STAGE_PART_SNAP || STAGE == STAGE_FULL;
    // LDS per wavefront: the DP nodes and the price tables -- 10,176 bytes at WMAX = 384 -> 16 wavefronts per CU.  The
    // probabilities of the piece's price model live in global memory (a.prior / a.lit, one slot per piece, L2-resident
    // while the piece runs): a parser window reads them once (bit-price table, length / distance tables on refresh), a
    // recorded symbol gathers and scatters <= 48 of them -- the 3.7 KiB they took in LDS buy 152 more nodes per window.
    constexpr uint32_t W_NODES = 6 * (WMAX + 1) + 2;                     // reps[4], price, info (16-byte multiple)
    constexpr uint32_t W_TABS = 128 + 72 + 32;                           // dsp, xt + ap (u16), ptab (u8)
    __shared__ __attribute__((aligned(16))) uint32_t pool[W_NODES + W_TABS];
#ifdef XZAMD_TIMING
    __shared__ unsigned long long tm_lds[16];
    if (threadIdx.x < 16) tm_lds[threadIdx.x] = 0;
    const uint64_t tm_start = __builtin_amdgcn_s_memtime();
#endif
    const uint32_t lane = threadIdx.x;
    const uint32_t blk = span / a.max_spb;
    const uint32_t k = SEED ? 0u : span - blk * a.max_spb;               // (the kernel hands SEED slot 0 of a Block, the others never)
    const uint32_t block_start = blk * a.block_size;
    const uint32_t block_end = min(a.n, block_start + a.block_size);
    uint32_t span_start, span_end;
    uint32_t piece_end;
    if constexpr (SEED) {
        // the seed piece is the same whatever the plan says (k_span_cut: seed_chunks), so it can run before the plan exists
        span_start = block_start;
        span_end = block_end - block_start > XZAMD_SEED_LEN ? block_start + XZAMD_SEED_LEN : block_end;
        piece_end = span_end;
    } else {
        if (k >= a.span_cnt[blk]) return;              // an unused slot of the span plan
        span_start = uni(a.span_tab[2 * span]); span_end = uni(a.span_tab[2 * span + 1]);
        piece_end = span_end;
        // a partial iteration parses only the first part of the piece (oracle: part_len); symbols never cross its end
        if constexpr (PARTIAL) span_end = uni(a.part_tab[span]);
    }
    // FROM_SNAP: the price model, coder state and rep distances come from the carried model walk over the records of
    // the partial iteration before (k_model_walk<3>: this piece's slot of a.prior / a.lit, a.snap_sr) -- no prior, no walk, no pre-roll
    const uint8_t* __restrict__ in = a.in;

    Env e;
    e.in = in; e.rank = a.rank; e.sorted_pos = a.sorted_pos; e.prev2 = a.prev2; e.prev3 = a.prev3;
    e.nice = a.nice_len; e.depth = a.depth; e.hb = a.hash_bytes; e.cyclic = a.dict_size + 1;
    e.block_end = block_end; e.n_last = a.n - 1;
    // (the list format is a template parameter: the packed records -- every dictionary up to 8 MiB -- need neither the branch
    // nor the pointer to the length array)
    e.mlen = PACKED ? nullptr : a.mlen; e.mdist = a.mdist; e.packed = PACKED ? 1u : 0u;
    ListPre LP;
    LP.valid = false; LP.pos = 0; LP.v = LP.l16 = 0;

    Work w{};
#ifdef XZAMD_TIMING
    w.tm = tm_lds;
#endif
    {
        uint32_t* nb = pool;
        w.n_reps4 = reinterpret_cast<uint4*>(nb);
        w.n_price = nb + 4 * (WMAX + 1);
        w.n_info = nb + 5 * (WMAX + 1);
        uint32_t* tb = nb + W_NODES;
        w.dsp = reinterpret_cast<uint16_t*>(tb);
        w.xt = reinterpret_cast<uint16_t*>(tb + 128);
        w.ap = w.xt + 128;
        w.ptab = reinterpret_cast<uint8_t*>(tb + 200);
        w.err = a.err;
        for (uint32_t t = lane; t < 128; t += 64) {     // bit price table (price_tablegen.c:31-58)
            uint32_t wv = t * 16 + 8, bit_count = 0;
            for (int jj = 0; jj < 4; ++jj) {
                wv *= wv;
                bit_count <<= 1;
                while (wv >= (1u << 16)) { wv >>= 1; ++bit_count; }
            }
            w.ptab[t] = (uint8_t)((11 << 4) - 15 - bit_count);
        }
        wave_sync();
        w.ptv = reinterpret_cast<const uint32_t*>(w.ptab)[lane & 31];
    }

    Lz z;
    // pb = 3, 4: the piece's price model -- which is the parser's alone, the coder keeps its own (k_model_syms, the real
    // pb) -- takes a pb = 2 view of the positions; the bit-price and length tables of the window cover four position
    // states (oracle: parse_block).  The recorded symbols are valid under any pb.
    block_lclp(a, blk, z.lc, z.lp); z.pb = a.pb < 2u ? a.pb : 2u;
    z.cnt_len = z.cnt_match = z.cnt_align = 0;
    const uint32_t lit_size = 0x300u << (a.lc + a.lp);
    z.lit = reinterpret_cast<plit_t*>(a.lit) + (uint64_t)span * lit_size;
    z.gp = a.prior + (uint64_t)span * XZAMD_PRIOR_WORDS;
    z.state = 0; z.rep0 = z.rep1 = z.rep2 = z.rep3 = 0;
    RC rc;                                              // never codes: encode_symbol_t<false, .> only adapts the model
    rc.cpos = 0; rc.out = nullptr; rc.reset();
    rc.ptab = nullptr; rc.est = 0; rc.tok = nullptr; rc.log = nullptr; rc.log_cap = 0;
    const GProbs probs{z.gp};
    uint16_t* const no_lds = nullptr;                   // encode_symbol_t<.., PG = true> never touches its LDS argument

    // price model: flat for the seed piece (slot 0 of the Block), else the model the seed left in ITS slot
    {
        uint4* g4 = reinterpret_cast<uint4*>(z.gp);
        uint4* l4 = reinterpret_cast<uint4*>(z.lit);
        if constexpr (SEED) {
            const uint4 v = make_uint4(1024u, 1024u, 1024u, 1024u);
            for (uint32_t i = lane; i < XZAMD_PRIOR_WORDS / 4; i += 64) g4[i] = v;
            const uint4 vl = PLIT_FLAT4;
            for (uint32_t i = lane; i < lit_size / PLIT_PER_U4; i += 64) l4[i] = vl;
        } else if constexpr (FROM_SNAP) {
            const uint32_t* sr = a.snap_sr + (uint64_t)span * 8u;
            z.state = uni(sr[0]); z.rep0 = uni(sr[1]); z.rep1 = uni(sr[2]); z.rep2 = uni(sr[3]); z.rep3 = uni(sr[4]);
        } else {
            const uint4* p4 = reinterpret_cast<const uint4*>(a.prior + (uint64_t)blk * a.max_spb * XZAMD_PRIOR_WORDS);
            for (uint32_t i = lane; i < XZAMD_PRIOR_WORDS / 4; i += 64) g4[i] = p4[i];
            const uint4* s4 = reinterpret_cast<const uint4*>(reinterpret_cast<const plit_t*>(a.lit) + (uint64_t)blk * a.max_spb * lit_size);
            for (uint32_t i = lane; i < lit_size / PLIT_PER_U4; i += 64) l4[i] = s4[i];
        }
        (void)g4; (void)l4;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wave_sync();
    }

    uint32_t cur = span_start;
    // Pre-roll (oracle: parse_piece, ORC_PREROLL): every piece but the seed first parses the XZAMD_PREROLL bytes in front
    // of it once more, from the prior, and throws the symbols away: the piece proper then starts with prices that have seen
    // the local data and with rep distances / a coder state like the ones the previous piece ends with.  `lim` is what the
    // parser may not cross: the piece start while pre-rolling, then the piece end.
    // (PRIOR instances only: everywhere else `rec` is the constant true and `lim` the piece end)
    uint32_t lim = span_end;
    bool rec = true;
    if constexpr (PRIOR) {
        if (span_start - block_start > XZAMD_PREROLL) {
            cur = span_start - XZAMD_PREROLL;
            lim = span_start;
            rec = false;
        }
    }
    // Warm-up (oracle: parse_piece, ORC_WARM): the prior is what the Block's first 64 KiB teach; data that has drifted since
    // (float arrays, PCM, ...) needs more than the pre-roll to re-train the model, so the XZAMD_WARM bytes in front of the
    // pre-roll -- never the seed piece's -- are walked greedily first: at every symbol boundary the longest entry of the
    // position's list record when it is cheap by a fixed rule, else a literal; each symbol adapts the model, nothing is
    // recorded, no prices, no DP.  64 positions per trip: lane = position (its longest entry, its byte, the byte before it,
    // the byte at rep0), the walk itself runs on readlanes.
    if (PRIOR && span_start - block_start > XZAMD_PREROLL + XZAMD_SEED_LEN) {
        const uint32_t w1 = span_start - XZAMD_PREROLL;
        uint32_t x0 = w1 - block_start - XZAMD_SEED_LEN > XZAMD_WARM ? w1 - XZAMD_WARM : block_start + XZAMD_SEED_LEN;
        // the distances of the last four candidates the walk rejected as too expensive: one that comes up again is a distance a
        // continuous parse would be carrying in its rep stack (periodic numeric data) and goes into the oldest rep slot -- nothing
        // is coded (oracle: parse_piece)
        uint32_t rj0 = 0, rj1 = 0, rj2 = 0, rj3 = 0, nrej = 0;
        // what the walk may not teach: is_rep / is_rep0 / is_rep1 / is_rep2 (48 probabilities) keep the seed piece's values -- its
        // rep decisions are the least like the optimal parser's (oracle: parse_piece)
        static_assert(P_IS_REP0_LONG - P_IS_REP == 48, "the rep-choice probabilities");
        const uint32_t keep_rep = lane < 48 ? lit_load(z.gp + P_IS_REP + lane) : 0u;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // in hand before the walk's first scatter
        while (x0 < w1) {
            const uint32_t px = min(x0 + lane, w1 - 1);
            const uint64_t rb = (uint64_t)px * LIST_W;
            const uint32_t tr = e.mdist[rb + LIST_K];
            const uint32_t cnt = tr & 0xFFu;
            const uint32_t ev = cnt ? e.mdist[rb + cnt - 1] : 0u;
            uint32_t L = 0, D = 0;
            if (cnt) {
                if (e.packed) { L = ev >> 23; D = ev & 0x7FFFFFu; }
                else { D = ev; L = e.mlen[rb + cnt - 1]; }
            }
            const uint32_t tc = in[px], tp = in[px - 1];
            uint32_t tm = in[px - z.rep0 - 1];
            uint32_t i = 0;
            const uint32_t rowlen = min(64u, w1 - x0);
            while (i < rowlen) {
                const uint32_t x = x0 + i;
                uint32_t len = min(lane_of(L, i), w1 - x);
                const uint32_t dist = lane_of(D, i);
                const uint32_t bl = dist ? 32u - (uint32_t)__builtin_clz(dist) : 0u;         // bit length of the distance
                const bool in_reps = dist == z.rep0 || dist == z.rep1 || dist == z.rep2 || dist == z.rep3;
                const bool take = len >= 2 && (14 + bl < 6 * len || in_reps);
                if (!take && len >= 3) {
                    const bool seen = (nrej > 0 && rj0 == dist) || (nrej > 1 && rj1 == dist) || (nrej > 2 && rj2 == dist) || (nrej > 3 && rj3 == dist);
                    if (seen) z.rep3 = dist;
                    else if (nrej < 4) { rj0 = nrej == 0 ? dist : rj0; rj1 = nrej == 1 ? dist : rj1; rj2 = nrej == 2 ? dist : rj2; rj3 = nrej == 3 ? dist : rj3; ++nrej; }
                    else { rj0 = rj1; rj1 = rj2; rj2 = rj3; rj3 = dist; }
                }
                if (take) {
                    // rep or match?  When the distance is one of the rep distances the current prices decide, as they do in
                    // the optimal parser (oracle: parse_piece -- data made of fixed-size records has two self-reinforcing
                    // ways to code the same copy; the walk must train the model into the one the parser lives in)
                    uint32_t back = dist + 4;
                    const uint32_t ri = dist == z.rep0 ? 0u : dist == z.rep1 ? 1u : dist == z.rep2 ? 2u : dist == z.rep3 ? 3u : 4u;
                    if (ri < 4) {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the model updates so far
                        const uint32_t ps = (x - block_start) & ((1u << z.pb) - 1), st = z.state;
                        const uint8_t* pt = w.ptab;
                        uint32_t prep = pr_bit(probs, pt, P_IS_REP + st, 1);
                        if (ri == 0) prep += pr_bit(probs, pt, P_IS_REP0 + st, 0) + pr_bit(probs, pt, P_IS_REP0_LONG + st * 16 + ps, 1);
                        else {
                            prep += pr_bit(probs, pt, P_IS_REP0 + st, 1);
                            if (ri == 1) prep += pr_bit(probs, pt, P_IS_REP1 + st, 0);
                            else prep += pr_bit(probs, pt, P_IS_REP1 + st, 1) + pr_bit(probs, pt, P_IS_REP2 + st, ri - 2);
                        }
                        prep += pr_len_one(probs, pt, P_REP_LEN, ps, len);
                        uint32_t pm = pr_bit(probs, pt, P_IS_REP + st, 0) + pr_len_one(probs, pt, P_MATCH_LEN, ps, len);
                        {
                            const uint32_t slot = dist_slot_of(dist);
                            pm += pr_tree(probs, pt, P_DIST_SLOT + (len < 6 ? len - 2 : 3u) * 64, 6, slot);
                            if (slot >= 4) {
                                const uint32_t fb = (slot >> 1) - 1;
                                const uint32_t base = (2 | (slot & 1)) << fb;
                                const uint32_t red = dist - base;
                                if (slot < 14) pm += pr_tree_rev(probs, pt, P_DIST_SPECIAL + base - slot - 1, fb, red);
                                else pm += ((fb - 4) << 4) + pr_tree_rev(probs, pt, P_DIST_ALIGN, 4, red & 15);
                            }
                        }
                        if (uni(prep) <= uni(pm)) back = ri;
                    }
                    const bool rep = back == 0;                              // rep0 stays what it was
                    encode_symbol_t<false, true, false, true>(rc, no_lds, z, x - block_start, back, len, 0u);
                    i += len;
                    if (!rep && i < rowlen) tm = in[max(px, x0 + i) - z.rep0 - 1];   // rep0 changed: the match bytes of the rest of the row
                                                                                     // (lanes behind the walk would reach in front of the Block)
                } else {
                    const uint32_t l3 = lane_of(tc, i) | (lane_of(tp, i) << 8) | (lane_of(tm, i) << 16);
                    encode_symbol_t<false, true, false, true>(rc, no_lds, z, x - block_start, LITERAL, 1, l3);
                    i += 1;
                }
            }
            x0 += i;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane < 48) lit_store(z.gp + P_IS_REP + lane, keep_rep);
    }
    bool cached = false;
    RoundL RL;
    RL.L = 0; RL.SL = 0; RL.SD = 0; RL.cnt = 0; RL.longest = 0; RL.l2a = RL.l2b = 0;
    RL.rp[0] = RL.rp[1] = RL.rp[2] = RL.rp[3] = 0;
    RL.mlo = RL.mhi = 0;
    RL.rl[0] = RL.rl[1] = RL.rl[2] = RL.rl[3] = 0;
    RL.pre = 0;
    LenTab lt;
    uint32_t q_pos = 0, q_end = 0;
    bool tables_valid = false;

    // What the coder will read out of this piece's records WITHOUT knowing its state and rep distances at the piece start
    // (oracle: lookback): twelve candidate states side by side (lane = candidate; they agree after a few symbols), rep
    // distances the piece does not name stay XZAMD_REP_UNKNOWN.  The walk of the encode span that starts behind this piece
    // begins with them (k_model_walk).
    uint32_t tl_st = lane < 12 ? lane : 0u;
    uint32_t tl_r0 = XZAMD_REP_UNKNOWN, tl_r1 = XZAMD_REP_UNKNOWN, tl_r2 = XZAMD_REP_UNKNOWN, tl_r3 = XZAMD_REP_UNKNOWN;
    if (rec) rc.ptab = w.ptab;                           // the price of the piece: its recorded symbols only
    if constexpr (SEED) {
        // encode_init (lzma_encoder.c:267-293): the first byte of a Block is a literal in the initial contexts (the seed
        // piece is the only one that starts a Block)
        const uint32_t l3 = literal_bytes(in, block_start, 0, z);
        if (lane == 0) { a.sym_len[block_start] = 0; a.sym_dist[block_start] = l3; }
        encode_symbol_t<false, true, false, true>(rc, no_lds, z, 0, LITERAL, 1, l3);
        tl_st = tl_st <= 3 ? 0u : tl_st <= 9 ? tl_st - 3 : tl_st - 6;
        cur = block_start + 1;
    }
    for (;;) {
        if (cur >= lim) {
            if (!PRIOR || rec) break;
            rec = true;                                  // the pre-roll is over: the piece proper
            rc.ptab = w.ptab; rc.est = 0;
            lim = span_end;
            cached = false;
            q_pos = q_end = 0;
            continue;
        }
        uint32_t back = LITERAL, len = 1;
        if (q_pos == q_end) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the model updates of the symbols so far: the prices read them
            TM_BEGIN(t_refresh);
            if (!tables_valid || z.cnt_len >= 64) { refresh_len_tables(probs, w.ptab, lt, 1u << z.pb, reinterpret_cast<uint32_t*>(w.n_reps4)); z.cnt_len = 0; }
            if (!tables_valid || z.cnt_match >= 128) { refresh_dist_tables(probs, w); z.cnt_match = 0; }
            if (!tables_valid || z.cnt_align >= 16) { refresh_align_table(probs, w); z.cnt_align = 0; }
            tables_valid = true;
            TM_END(w, 7, t_refresh);
            if (!cached) {
                round_lists(e, LP, cur, lim, z.rep0, z.rep1, z.rep2, z.rep3, RL);
                cached = true;
            }
            uint32_t sb = LITERAL, sl = 0;
            if (RL.rp[0] >= e.nice) { sb = 0; sl = RL.rp[0]; }
            else if (RL.rp[1] >= e.nice) { sb = 1; sl = RL.rp[1]; }
            else if (RL.rp[2] >= e.nice) { sb = 2; sl = RL.rp[2]; }
            else if (RL.rp[3] >= e.nice) { sb = 3; sl = RL.rp[3]; }
            else if (RL.longest >= e.nice) { sb = lane_of(RL.SD, RL.cnt - 1) + 4; sl = RL.longest; }
            if (sl) {
                back = sb; len = sl;
                cached = false;
                q_pos = q_end = 0;
            } else if (RL.cnt == 0 && RL.rp[0] == 0 && RL.rp[1] < 2 && RL.rp[2] < 2 && RL.rp[3] < 2
                    && mask_run_after(rm_of(RL, 0), 0) < 2) {
                cached = false;                         // nothing but a literal can leave this node
                q_pos = q_end = 0;
            } else {
                cached = optimum_window<WMAX>(e, w, LP, probs, z, lt, in, cur, block_start, lim, cached, RL, q_end);
                q_pos = 0;
                if (q_end == 0) {                       // consistency failure reported by the parser
                    if (lane == 0 && a.err) atomicCAS(a.err, 0u, 2u);
                    return;
                }
            }
        }
        if (q_pos != q_end) {
            back = uni(w.n_price[q_pos]);
            len = (uni(w.n_info[q_pos]) >> 13) & 0x1FF;
            q_pos += len;
        }
        if (len == 0 || len > MATCH_LEN_MAX || cur + len > lim
                || (back != LITERAL && back >= 4 && back - 4 >= cur - block_start)) {
            if (lane == 0 && a.err) {
                if (atomicCAS(a.err, 0u, 1u) == 0u) {
                    a.err[1] = span; a.err[2] = cur - block_start; a.err[3] = back; a.err[4] = len;
                    a.err[5] = q_pos; a.err[6] = q_end; a.err[7] = 0;
                }
            }
            return;
        }
        uint32_t l3 = 0;
        if (back == LITERAL) {
            l3 = literal_bytes(in, cur, cur - block_start, z) | (z.state >= 7 ? 1u << 24 : 0u);
            // the match byte of the record is the coder's only when the coder has coded the symbol in front of it, i.e. not
            // for the first symbol of a piece (the pre-roll in front of it is the parser's alone): there the coder fetches
            // the byte itself
            const uint32_t l3r = cur == span_start ? (l3 & 0xFFFFu) : l3;
            if (lane == 0 && rec) { a.sym_len[cur] = 0; a.sym_dist[cur] = l3r; }
        } else if (lane == 0 && rec) {
            // bit 15: the parser chose a MATCH -- the coder then codes a match even when the distance is one of its rep
            // distances (oracle: parse_piece)
            a.sym_len[cur] = (uint16_t)(len | (back >= 4 ? 0x8000u : 0u));
            a.sym_dist[cur] = back >= 4 ? back - 4 : back == 0 ? z.rep0 : back == 1 ? z.rep1 : back == 2 ? z.rep2 : z.rep3;
        }
        if (rec) {
            // the coder's reading of the record (k_model_walk) with unknown rep distances: 0 literal, 1 match, 2 rep, 3 short rep
            uint32_t type = 0;
            if (back != LITERAL) {
                const uint32_t dd = back >= 4 ? back - 4 : back == 0 ? z.rep0 : back == 1 ? z.rep1 : back == 2 ? z.rep2 : z.rep3;
                if (back >= 4) type = 1;
                else if (len == 1) type = dd == tl_r0 ? 3u : 0u;
                else {
                    const uint32_t ri = dd == tl_r0 ? 0u : dd == tl_r1 ? 1u : dd == tl_r2 ? 2u : dd == tl_r3 ? 3u : 4u;
                    type = ri < 4 ? 2u : 1u;
                    if (ri == 1) { tl_r1 = tl_r0; tl_r0 = dd; }
                    else if (ri == 2) { tl_r2 = tl_r1; tl_r1 = tl_r0; tl_r0 = dd; }
                    else if (ri == 3) { tl_r3 = tl_r2; tl_r2 = tl_r1; tl_r1 = tl_r0; tl_r0 = dd; }
                }
                if (type == 1) { tl_r3 = tl_r2; tl_r2 = tl_r1; tl_r1 = tl_r0; tl_r0 = dd; }
            }
            tl_st = type == 0 ? (tl_st <= 3 ? 0u : tl_st <= 9 ? tl_st - 3 : tl_st - 6)
                    : tl_st < 7 ? (type == 1 ? 7u : type == 2 ? 8u : 9u) : (type == 1 ? 10u : 11u);
        }
        {
            TM_BEGIN(t_sym);
            encode_symbol_t<false, true, false, true>(rc, no_lds, z, cur - block_start, back, len, l3);
            TM_END(w, 6, t_sym);
            TM_COUNT(w, 10);
        }
        if (a.trace && lane == 0 && rec) {
            const uint32_t ti = atomicAdd(a.trace_count, 1u);
            if (ti < a.trace_cap) {
                a.trace[4 * ti] = span;
                a.trace[4 * ti + 1] = cur - block_start;
                a.trace[4 * ti + 2] = back;
                a.trace[4 * ti + 3] = len;
            }
        }
        cur += len;
    }
    // (the seed piece leaves the prior of the Block where it is: its own slot of a.prior / a.lit)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    {
        // what the walk of the encode span behind this piece starts from, and whether the coder stores the piece raw: its
        // parser's own price says it does not shrink (oracle: parse_block)
        const uint32_t s0 = lane_of(tl_st, 0);
        const bool agree = __builtin_amdgcn_ballot_w64(lane < 12 && tl_st != s0) == 0;
        if (lane < 2 && a.pinfo) {
            // lane 0: the half the walk over iteration 1's records reads, lane 1: the half the coder's walk reads (the seed
            // piece is parsed once and serves both)
            const bool mine = SEED || (lane == 0) == PARTIAL;
            if (mine) {
                uint32_t* pi = a.pinfo + (uint64_t)span * XZAMD_PINFO_WORDS + lane * (XZAMD_PINFO_WORDS / 2);
                pi[0] = s0 | (agree ? XZAMD_PI_STATE_OK : 0u);
                pi[1] = tl_r0; pi[2] = tl_r1; pi[3] = tl_r2; pi[4] = tl_r3;
                const uint32_t plen = piece_end - span_start;
                pi[5] = (span_end == piece_end && plen >= XZAMD_RAW_MIN_LEN && rc.est / 128u >= plen) ? 1u : 0u;
            }
        }
    }
#ifdef XZAMD_TIMING
    if (lane == 0 && a.err) {
        tm_lds[8] = __builtin_amdgcn_s_memtime() - tm_start;
        unsigned long long* g = reinterpret_cast<unsigned long long*>(a.err + 16);
        for (int i = 0; i < 12; ++i) atomicAdd(g + i, tm_lds[i]);
        atomicMax(g + 12, tm_lds[8]);
        atomicAdd(g + 13, tm_lds[13]);
        atomicAdd(g + 14, tm_lds[14]);
        atomicAdd(g + 15, tm_lds[15]);
    }
#endif
}

// One kernel per (list format, stage); each holds exactly one inlined copy of parse_piece_one -- and so one LDS pool.
// XZAMD_WAVES_SEED (measurement knob): the seed launch is one wavefront per Block, a latency chain that occupancy does
// nothing for; DESIGN.md 3.3 has what a lower value measured.
#ifndef XZAMD_WAVES_SEED
#define XZAMD_WAVES_SEED XZAMD_WAVES_OPT
#endif
template <uint32_t WMAX, bool PACKED, ParseStage STAGE>
__global__ __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(STAGE == STAGE_SEED ? XZAMD_WAVES_SEED : XZAMD_WAVES_OPT,
                                   STAGE == STAGE_SEED ? XZAMD_WAVES_SEED : XZAMD_WAVES_OPT)))
void k_parse_pieces(xzamd_span_args a, uint32_t nslots, uint32_t* __restrict__ counter)
{
    for (;;) {
        uint32_t s = blockIdx.x;
        if (counter != nullptr) {
            if (threadIdx.x == 0) s = atomicAdd(counter, 1u);
            s = uni(s);
        }
        if (s >= nslots) break;
        // SEED: s = Block, its seed piece is slot 0; the others: every slot but the seed's
        const uint32_t slot = STAGE == STAGE_SEED ? s * a.max_spb : a.order ? a.order[s] : s;
        if (STAGE == STAGE_SEED || slot % a.max_spb != 0) parse_piece_one<WMAX, PACKED, STAGE>(a, slot);
        if (counter == nullptr) break;
        __builtin_amdgcn_s_waitcnt(0);
        wave_sync();
    }
}

// ---- phase 2: the recorded symbols of one encode span through the coder's model ----
struct SymRow {
    uint32_t base;          // position of lane 0 of `l` / `d`
    uint32_t l, d;          // records of positions base + lane
    uint32_t nl, nd;        // records of positions base + 64 + lane (in flight)
};

__device__ __forceinline__ void symrow_load(const xzamd_span_args& a, uint32_t pos, uint32_t& l, uint32_t& d)
{
    uint32_t x = pos + threadIdx.x;
    x = x < a.n ? x : a.n - 1;
    l = a.sym_len[x];
    d = a.sym_dist[x];
}

// The walk of one encode span over its recorded symbols (oracle: encode_block_syms / snapshot_walk), in four forms:
//   MODE 0  k_model_syms      the coder's model pass: from the span's TRUE start model (k_model_chain) every binary decision
//                             leaves a token, chunks are cut by the summed prices of their decisions (the range coder runs
//                             later, one lane per chunk: k_rc_chunks), stored pieces are copied
//   MODE 1  k_model_bounds    the same walk with two values per probability, lo (from 31) and hi (from 2017): whatever the
//                             start model is, the true value stays between them (the update is monotone); until they meet the
//                             slot's bits are logged for k_model_chain
//   MODE 2  bounds, and MODE 3 snapshots, over the records of parse iteration 1 (only the first part of a piece, a.part_tab, of a
//                             piece have them): the model every piece starts iteration 2 from goes into ITS slot of
//                             a.prior / a.lit (u32 each), coder state and rep distances into a.snap_sr
// LITG: the literal coders (6,144 of the 7,990 probabilities at lc = 3) live in global memory -- the span's slice of cb_bnd,
// u32 each, L2-resident while the span is walked -- and LDS holds the 1,846 others: 7.4 KiB (bounds) / 3.8 KiB per wavefront instead
// of 32 / 16 KiB, so that a CU holds several times the wavefronts (these walks are bound by the latency of their dependent
// instructions; the single-phase span kernels made the same trade).
template <int MODE, bool LITG>
__global__ __launch_bounds__(64) void k_model_walk(xzamd_span_args a, uint32_t nslots)
{
    constexpr bool BND = MODE == 1 || MODE == 2, SUB = MODE >= 2, TOKM = MODE == 0;
    extern __shared__ __attribute__((aligned(16))) uint32_t enc_pool[];
    uint16_t* const probs = reinterpret_cast<uint16_t*>(enc_pool);
    const uint32_t lane = threadIdx.x;
    const uint32_t slot = blockIdx.x;
    if (slot >= nslots) return;
    const uint32_t blk = slot / a.max_esb;
    const uint32_t k = slot - blk * a.max_esb;
    if (k >= a.enc_cnt[blk]) return;
    const uint32_t block_start = blk * a.block_size;
    const uint32_t span_start = uni(a.enc_tab[2 * slot]), span_end = uni(a.enc_tab[2 * slot + 1]);
    const uint8_t* __restrict__ in = a.in;
    const uint32_t nprob = P_LITERAL + (0x300u << (a.lc + a.lp));
    const uint32_t nlds = LITG ? (uint32_t)P_LITERAL : nprob;                  // probabilities held in LDS
    const uint32_t model_words = BND ? nlds : (nlds + 1) / 2;
    uint8_t* const ptab = reinterpret_cast<uint8_t*>(enc_pool + model_words);
    // LITG: the literal coders' working array (bounds, or plain probabilities: k_model_chain has read the bounds by then)
    uint32_t* const litw = a.cb_bnd + (uint64_t)slot * a.model_slots_pad + P_LITERAL;
    const uint32_t nlit = nprob - P_LITERAL;
    if (!BND) {
        for (uint32_t t = lane; t < 128; t += 64) {         // bit price table (price_tablegen.c:31-58)
            uint32_t wv = t * 16 + 8, bit_count = 0;
            for (int jj = 0; jj < 4; ++jj) {
                wv *= wv;
                bit_count <<= 1;
                while (wv >= (1u << 16)) { wv >>= 1; ++bit_count; }
            }
            ptab[t] = (uint8_t)((11 << 4) - 15 - bit_count);
        }
    }
    // the piece that starts at the span start (encode spans are closed at piece ends)
    const uint32_t pcnt = uni(a.span_cnt[blk]);
    const uint32_t* __restrict__ ptb = a.span_tab + 2ull * blk * a.max_spb;
    uint32_t pj = 0;
    for (uint32_t j0 = 0; j0 < pcnt; j0 += 64) {
        const uint32_t jj = j0 + lane;
        const uint64_t m = __builtin_amdgcn_ballot_w64(jj < pcnt && ptb[2 * jj] == span_start);
        if (m) { pj = j0 + (uint32_t)__builtin_ctzll(m); break; }
    }
    // (the half of a piece's info written by the parse iteration whose records this walk reads)
    const uint32_t* __restrict__ pinfo = a.pinfo + (uint64_t)blk * a.max_spb * XZAMD_PINFO_WORDS + (SUB ? 0u : XZAMD_PINFO_WORDS / 2);

    Lz z;
    block_lclp(a, blk, z.lc, z.lp); z.pb = SUB ? min(a.pb, 2u) : a.pb;     // (the snapshots are the PARSER's price model: its pb view)
    z.cnt_len = z.cnt_match = z.cnt_align = 0;
    z.lit = LITG ? reinterpret_cast<plit_t*>(litw) : nullptr;
    z.gp = nullptr;
    z.state = 0; z.rep0 = z.rep1 = z.rep2 = z.rep3 = 0;
    RC rc;
    rc.cpos = 0; rc.out = nullptr; rc.reset();
    rc.log = BND ? a.cb_log + (uint64_t)slot * a.model_slots_pad * XZAMD_LOG_WORDS : nullptr;
    rc.log_cap = a.log_cap ? a.log_cap : XZAMD_LOG_CAP;

    // how the span starts
    uint32_t hflags = 0;
    bool known = k == 0;                    // the model at the span start does not depend on the spans in front
    if (k != 0) {
        const uint32_t* pi = pinfo + (uint64_t)(pj - 1) * XZAMD_PINFO_WORDS;
        if (!SUB && uni(pi[5])) known = true;          // behind a stored piece: state reset
        else {
            const uint32_t w0 = uni(pi[0]);
            if (!(w0 & XZAMD_PI_STATE_OK)) hflags |= XZAMD_CB_BAD_START;
            z.state = w0 & 15u;
            z.rep0 = uni(pi[1]); z.rep1 = uni(pi[2]); z.rep2 = uni(pi[3]); z.rep3 = uni(pi[4]);
        }
    }
    if (known) hflags |= XZAMD_CB_KNOWN_START;
    uint32_t carry = 1;                     // MODE 0 / 3: 0 = round 5's reset (+ properties), 1 = carried, 2 = flat start, no properties
    if (!BND && k != 0) carry = uni(a.cb_carry[slot]);
    if (BND) {
        const uint32_t v0 = known ? (1024u | 1024u << 11) : (31u | 2017u << 11);
        for (uint32_t i = lane; i < nlds; i += 64) enc_pool[i] = v0;
        if (LITG) for (uint32_t i = lane; i < nlit; i += 64) lit_store(litw + i, v0);
    } else if (k != 0 && carry == 1) {
        const uint16_t* s16 = a.cb_start + (uint64_t)slot * a.model_slots_pad;
        const uint32_t* s32 = reinterpret_cast<const uint32_t*>(s16);
        for (uint32_t i = lane; i < model_words; i += 64) enc_pool[i] = s32[i];
        if (LITG) for (uint32_t i = lane; i < nlit; i += 64) lit_store(litw + i, (uint32_t)s16[P_LITERAL + i]);
    } else {
        for (uint32_t i = lane; i < model_words; i += 64) enc_pool[i] = 0x04000400u;
        if (LITG) for (uint32_t i = lane; i < nlit; i += 64) lit_store(litw + i, 1024u);
        z.state = 0; z.rep0 = z.rep1 = z.rep2 = z.rep3 = 0;
    }
    if (LITG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_sync();
    if (TOKM && a.resume_sr != nullptr && lane == 0) {
        // what this span's coder starts from, for the span's record of the resume table (k_resume_export)
        uint32_t* sr = a.resume_sr + (uint64_t)slot * 8u;
        sr[0] = z.state; sr[1] = z.rep0; sr[2] = z.rep1; sr[3] = z.rep2; sr[4] = z.rep3;
        sr[5] = k == 0 ? XZAMD_RK_RESET : carry;
    }

    uint16_t* const tok0 = TOKM ? a.tok + XZAMD_TOK_BASE(span_start, slot) : nullptr;
    // Token budget of the span.  The buffer holds XZAMD_TOK_PER_BYTE tokens per input byte (+ 4096); a.tok_limit (tests only,
    // <= XZAMD_TOK_PER_BYTE) lowers the budget without changing the layout.  Data made of far three-byte matches needs more
    // (32 ... 41 tokens per 3 bytes): when the budget runs out the chunk is closed where it stands and the REST of the span
    // is stored as raw LZMA2 chunks (lzma2_encoder.c:110-131) -- valid output instead of a failed Stream -- and no later span
    // of the Block is carried (oracle: encode_block_syms).  The walks over iteration 1's records write no tokens: no budget.
    const uint64_t tok_cap = (uint64_t)(span_end - span_start) * (a.tok_limit ? a.tok_limit : XZAMD_TOK_PER_BYTE) + 4096u - 64u;
    rc.tok = tok0; rc.est = 0; rc.ptab = ptab;
    const uint32_t cbase = XZAMD_CHUNK_BASE(span_start, slot);
    const uint32_t ccap = XZAMD_CHUNK_CAP(span_end - span_start);
    uint32_t nchunks = 0;

    bool need_props = k == 0 || carry == 0, need_dict_reset = (span_start == block_start), need_state_reset = k == 0 || carry != 1;
    bool failed = false, tok_full = false;
    uint32_t f_pos = 0, f_back = 0, f_len = 0, f_d = 0;
    uint32_t cur = span_start;
    uint32_t p_end = uni(ptb[2 * pj + 1]);                           // end of the piece that holds cur
    const uint32_t* __restrict__ ptp = a.part_tab + (uint64_t)blk * a.max_spb;           // SUB: where the parsed part of a piece ends
    uint32_t seg_end = SUB ? uni(ptp[pj]) : p_end;   // end of what is walked of it (the seed piece has all its records)
    uint32_t raw_until = (!SUB && uni(pinfo[(uint64_t)pj * XZAMD_PINFO_WORDS + 5])) ? p_end : span_start;
    bool fresh_piece = true;                                          // cur is a piece start that has not been looked at
    SymRow R;
    R.base = span_start;
    symrow_load(a, span_start, R.l, R.d);
    symrow_load(a, span_start + 64, R.nl, R.nd);

    while (cur < span_end) {
        if (cur < raw_until) {
            // a stored piece, or the rest of a span that ran out of tokens: raw chunks of 64 KiB (lzma2_encoder.c:110-131)
            if (TOKM) {
                const uint32_t usize = min(raw_until - cur, 65536u);
                const uint32_t cidx = cbase + nchunks;
                if (nchunks + 1 >= ccap) { f_pos = cur - block_start; f_back = 0xFFFFFFF0u; failed = true; break; }
                uint8_t* const hdr = a.scratch + XZAMD_CHUNK_OUT(cur, cidx);
                for (uint32_t i = lane; i < usize; i += 64) hdr[3 + i] = in[cur + i];
                if (lane == 0) {
                    hdr[0] = need_dict_reset ? 1 : 2;
                    hdr[1] = (uint8_t)((usize - 1) >> 8);
                    hdr[2] = (uint8_t)(usize - 1);
                    xzamd_chunk c;
                    c.in_start = cur; c.usize = usize; c.tok_lo = 0; c.tok_hi = 0;
                    c.ntok = 0; c.csize = 3u + usize; c.flags = XZAMD_CH_RAW; c.pad_ = 0;
                    a.chunks[cidx] = c;
                }
                need_dict_reset = false;
                ++nchunks;
                cur += usize;
            } else
                cur = raw_until;
            need_state_reset = true;
            if (cur == p_end && cur < span_end) {                    // (a stored piece ends where the next piece starts)
                ++pj;
                p_end = uni(ptb[2 * pj + 1]);
                seg_end = p_end;
                if (uni(pinfo[(uint64_t)pj * XZAMD_PINFO_WORDS + 5])) raw_until = p_end;
            }
            continue;
        }
        if (need_state_reset && !(k != 0 && carry == 1 && cur == span_start)) {
            // lzma_lzma_encoder_reset (lzma_encoder.c:529-598); the flag stays set until a chunk header has announced it
            if (BND) { for (uint32_t i = lane; i < nlds; i += 64) enc_pool[i] = 1024u | 1024u << 11; }
            else { for (uint32_t i = lane; i < model_words; i += 64) enc_pool[i] = 0x04000400u; }
            if (LITG) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                for (uint32_t i = lane; i < nlit; i += 64) lit_store(litw + i, BND ? (1024u | 1024u << 11) : 1024u);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            wave_sync();
            z.state = 0; z.rep0 = z.rep1 = z.rep2 = z.rep3 = 0;
        }
        const uint32_t chunk_start = cur;
        uint16_t* const chunk_tok = rc.tok;
        rc.est = 0;
        bool piece_break = false;
        for (;;) {
            // the chunk rule of the two-phase coder (oracle: encode_block_syms): input limit of lzma2_encoder.c:167-181, and
            // the summed prices in place of the coded size
            if (TOKM && (cur - chunk_start >= (1u << 21) - MATCH_LEN_MAX || rc.est >= XZAMD_CHUNK_EST))
                break;
            if (cur >= span_end)
                break;
            if (cur >= seg_end) {
                // the next piece (SUB: behind the part of this one that iteration 1 parsed)
                cur = p_end;
                if (cur >= span_end) break;
                ++pj;
                p_end = uni(ptb[2 * pj + 1]);
                seg_end = SUB ? uni(ptp[pj]) : p_end;
                fresh_piece = true;
                if (!SUB && uni(pinfo[(uint64_t)pj * XZAMD_PINFO_WORDS + 5])) { raw_until = p_end; piece_break = true; break; }
            }
            if (MODE == 3 && fresh_piece && cur != block_start) {
                // snapshot: the price model piece pj starts iteration 2 from (its slot of a.prior / a.lit), state, rep distances
                const uint64_t ps_ = (uint64_t)blk * a.max_spb + pj;
                uint32_t* gp = a.prior + ps_ * XZAMD_PRIOR_WORDS;
                plit_t* gl = reinterpret_cast<plit_t*>(a.lit) + ps_ * (0x300ull << (a.lc + a.lp));
                for (uint32_t i = lane; i < P_LITERAL; i += 64) gp[i] = probs[i];
                if (LITG) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the literal updates so far
                    for (uint32_t i = lane; i < nlit; i += 64) gl[i] = (plit_t)lit_load(litw + i);
                } else
                    for (uint32_t i = lane; i < nlit; i += 64) gl[i] = (plit_t)probs[P_LITERAL + i];
                if (lane == 0) {
                    uint32_t* sr = a.snap_sr + ps_ * 8u;
                    sr[0] = z.state;                  // a parser's rep distances must be real ones: unknown -> 0, as after a reset
                    sr[1] = z.rep0 == XZAMD_REP_UNKNOWN ? 0u : z.rep0; sr[2] = z.rep1 == XZAMD_REP_UNKNOWN ? 0u : z.rep1;
                    sr[3] = z.rep2 == XZAMD_REP_UNKNOWN ? 0u : z.rep2; sr[4] = z.rep3 == XZAMD_REP_UNKNOWN ? 0u : z.rep3;
                }
            }
            fresh_piece = false;
            if (!SUB && (uint64_t)(rc.tok - tok0) + 64u > tok_cap) { tok_full = true; break; }
            uint32_t off = cur - R.base;
            if (off >= 64) {
                if (off < 128) {
                    R.l = R.nl; R.d = R.nd; R.base += 64; off -= 64;
                } else {
                    R.base = cur; off = 0;
                    symrow_load(a, cur, R.l, R.d);
                }
                symrow_load(a, R.base + 64, R.nl, R.nd);
            }
            uint32_t len = lane_of(R.l, off);
            const uint32_t d = lane_of(R.d, off);
            const uint32_t as_match = len >> 15;         // the parser's choice: a match, whatever the coder's rep distances are
            len &= 0x7FFFu;
            uint32_t back, l3 = 0;
            if (len == 0) {
                back = LITERAL; len = 1; l3 = d;
                if (z.state >= 7 && !(d >> 24))          // no match byte with the record (first symbol of a piece): fetch it
                    l3 = (d & 0xFFFFu) | (uni(in[cur - z.rep0 - 1]) << 16);
            } else if (as_match) {
                back = d + 4;
            } else if (len == 1) {
                if (d == z.rep0) back = 0;
                else { back = LITERAL; l3 = literal_bytes(in, cur, cur - block_start, z); }   // a short rep0 of another distance: code the byte
            } else if (d == z.rep0) back = 0;
            else if (d == z.rep1) back = 1;
            else if (d == z.rep2) back = 2;
            else if (d == z.rep3) back = 3;
            else back = d + 4;
            if (len > MATCH_LEN_MAX || cur + len > seg_end
                    || (back != LITERAL && back >= 4 && back - 4 >= cur - block_start)
                    || (TOKM && nchunks + 1 >= ccap)) {
                // internal consistency failure: report it and leave through the loop conditions (an early return from
                // inside the loops costs the compiler its proof that the coder state is wave-uniform)
                f_pos = cur - block_start; f_back = back; f_len = len; f_d = d;
                failed = true;
                cur = span_end;
                break;
            }
            encode_symbol_t<false, LITG, TOKM, false, BND>(rc, probs, z, cur - block_start, back, len, l3);
            cur += len;
        }
        if (failed) break;
        if (TOKM) {
            const uint32_t usize = cur - chunk_start;
            if (usize != 0) {
                const uint32_t ntok = (uint32_t)(rc.tok - chunk_tok);
                const uint32_t cidx = cbase + nchunks;
                uint32_t flags = 0u;
                if (need_props) flags |= XZAMD_CH_PROPS;
                if (need_dict_reset) flags |= XZAMD_CH_DICT_RESET;
                if (need_state_reset) flags |= XZAMD_CH_STATE_RESET;
                need_props = false; need_dict_reset = false; need_state_reset = false;
                if (lane == 0) {
                    const uint64_t tix = (uint64_t)(chunk_tok - a.tok);
                    xzamd_chunk c;
                    c.in_start = chunk_start; c.usize = usize; c.tok_lo = (uint32_t)tix; c.tok_hi = (uint32_t)(tix >> 32);
                    c.ntok = ntok; c.csize = 0u; c.flags = flags; c.pad_ = 0;
                    a.chunks[cidx] = c;
                }
                ++nchunks;
            }
        } else if (cur != chunk_start)
            need_state_reset = false;
        (void)piece_break;
        if (tok_full) raw_until = span_end;                // the rest of the span goes out raw
    }
    if (BND) {
        // what k_model_chain needs of the span: the bounds, and whether the span can hand its model on at all
        uint32_t* gb = a.cb_bnd + (uint64_t)slot * a.model_slots_pad;
        bool bad = false;
        if (LITG) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        for (uint32_t i = lane; i < nprob; i += 64) {
            const uint32_t v = (LITG && i >= P_LITERAL) ? lit_load(gb + i) : enc_pool[i];
            if (!(LITG && i >= P_LITERAL)) gb[i] = v;
            bad = bad || ((v & 0x7FFu) != ((v >> 11) & 0x7FFu) && (v >> 22) >= rc.log_cap);
        }
        if (__builtin_amdgcn_ballot_w64(bad) != 0 || tok_full) hflags |= XZAMD_CB_BAD_END;
        if (lane == 0) a.cb_hdr[slot] = hflags;
    }
    if (failed && lane == 0 && a.err) {
        if (atomicCAS(a.err, 0u, 3u + (uint32_t)MODE * 16u) == 0u) {
            a.err[1] = slot; a.err[2] = f_pos; a.err[3] = f_back; a.err[4] = f_len;
            a.err[5] = f_d; a.err[6] = nchunks; a.err[7] = (uint32_t)(rc.tok - tok0);
        }
    }
}

// The model of every encode span at its start (oracle: the `failed` / lookback logic of encode_block_syms): one thread
// per probability and Block walks the Block's spans in order -- start value of span k + 1 = lo where the slot's bounds met
// in span k, else the slot's logged bits replayed on its start value in span k.  A span that cannot hand its model on
// (XZAMD_CB_BAD_END), or whose start state the piece in front does not name (XZAMD_CB_BAD_START), ends the carrying: every
// later span of the Block starts with round 5's reset.  cb_carry: 0 = reset + properties, 1 = carried, 2 = flat, no properties
// (behind a stored piece).
__global__ __launch_bounds__(256) void k_model_chain(xzamd_span_args a, uint32_t nblocks)
{
    const uint32_t blk = blockIdx.y;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (blk >= nblocks) return;
    const uint32_t nprob = P_LITERAL + (0x300u << (a.lc + a.lp));
    const uint32_t cnt = a.enc_cnt[blk];
    uint32_t p = 1024;
    bool ok = true;
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t slot = blk * a.max_esb + k;
        const uint32_t hf = a.cb_hdr[slot];
        if (k != 0 && (hf & XZAMD_CB_BAD_START)) ok = false;
        const bool known = (hf & XZAMD_CB_KNOWN_START) != 0;
        if (!ok || known) p = 1024;
        if (k != 0) {
            if (i == 0) a.cb_carry[slot] = !ok ? 0u : known ? 2u : 1u;
            if (i < a.model_slots_pad) a.cb_start[(uint64_t)slot * a.model_slots_pad + i] = (uint16_t)(i < nprob ? p : 1024u);
        }
        if (hf & XZAMD_CB_BAD_END) ok = false;
        if (i < nprob && ok) {
            const uint32_t v = a.cb_bnd[(uint64_t)slot * a.model_slots_pad + i];
            const uint32_t lo = v & 0x7FFu, hi = (v >> 11) & 0x7FFu, nb = v >> 22;
            if (lo == hi) p = lo;
            else {
                const uint32_t* lg = a.cb_log + ((uint64_t)slot * a.model_slots_pad + i) * XZAMD_LOG_WORDS;
                uint32_t w = 0;
                for (uint32_t t = 0; t < nb; ++t) {
                    if ((t & 31u) == 0) w = lg[t >> 5];
                    const uint32_t bit = (w >> (t & 31u)) & 1u;
                    p = bit ? p - (p >> 5) : p + ((2048u - p) >> 5);
                }
            }
        }
    }
}

// The resume table of a verified encode: one workgroup per encode-span slot gathers what the span's coder started from
// (a.resume_sr: k_model_syms; a.cb_start: k_model_chain) into the span's record, and compacts the slots blk * max_esb + k
// to consecutive records (Stream order: the batches, their Blocks and the spans of a Block all come in order).  The
// model is copied as it is, 16 bytes per lane: coder and decoder index it alike (kernels_api.h).
static_assert(XZAMD_RK_RESET == 0u && XZAMD_RK_CARRIED == 1u && XZAMD_RK_FLAT == 2u, "record kinds = the values of cb_carry");
constexpr uint32_t offs[] = XZAMD_MODEL_OFFSETS;
static_assert(offs[0] == P_IS_MATCH && offs[1] == P_IS_REP && offs[2] == P_IS_REP0 && offs[3] == P_IS_REP1 && offs[4] == P_IS_REP2
            && offs[5] == P_IS_REP0_LONG && offs[6] == P_DIST_SLOT && offs[7] == P_DIST_SPECIAL && offs[8] == P_DIST_ALIGN
            && offs[9] == P_MATCH_LEN && offs[10] == P_REP_LEN && offs[11] == P_LITERAL, "the coder's model layout");
__global__ __launch_bounds__(256) void k_resume_export(xzamd_span_args a, uint32_t nblocks, uint32_t block0,
        uint8_t* __restrict__ table, uint32_t rec_base, uint32_t rec_cap)
{
    __shared__ uint32_t part[4];
    const uint32_t slot = blockIdx.x;
    const uint32_t blk = slot / a.max_esb;
    const uint32_t k = slot - blk * a.max_esb;
    if (blk >= nblocks || k >= a.enc_cnt[blk]) return;          // (uniform over the workgroup)
    // records of the batch's Blocks in front of this one
    uint32_t s = 0;
    for (uint32_t b = threadIdx.x; b < blk; b += 256) s += a.enc_cnt[b];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    const uint64_t r = (uint64_t)rec_base + part[0] + part[1] + part[2] + part[3] + k;
    if (r >= rec_cap) return;
    const uint32_t stride = XZAMD_RESUME_BYTES(a.model_slots_pad);
    uint8_t* const rec = table + r * stride;
    const uint32_t* sr = a.resume_sr + (uint64_t)slot * 8u;
    const uint32_t kind = sr[5];
    if (threadIdx.x < 8) {
        const uint32_t t = threadIdx.x;
        uint32_t w = sr[t < 3 ? 0u : t - 3u];                       // t = 3 .. 7: state, rep distances
        if (t == 0) w = block0 + blk;
        if (t == 1) w = a.enc_tab[2 * slot] - blk * a.block_size;
        if (t == 2) {
            uint32_t lc, lp;                                        // (the Block's own pair: what a decoder resumes with)
            block_lclp(a, blk, lc, lp);
            w = lc | lp << 8 | a.pb << 16 | kind << 24;
        }
        reinterpret_cast<uint32_t*>(rec)[t] = w;
    }
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(a.cb_start + (uint64_t)slot * a.model_slots_pad);
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(rec + XZAMD_RESUME_HDR);
    const uint32_t nq = a.model_slots_pad / 8u;
    const uint4 flat = make_uint4(0x04000400u, 0x04000400u, 0x04000400u, 0x04000400u);
    for (uint32_t q = threadIdx.x; q < nq; q += 256) dst[q] = kind == XZAMD_RK_CARRIED ? src[q] : flat;
}

// Range coder of the two-phase mode: one LANE per LZMA2 chunk (rangecoder/range_encoder.h:136-263 per lane).  A chunk's
// coder starts from the reset state, so the chunks of a batch -- thousands -- are independent given their tokens; the
// serial recurrence that costs a wavefront ~16 scalar instructions per decision when it runs one span costs a lane of
// this kernel one vector instruction slot shared with 63 other chunks.
__global__ __launch_bounds__(64) void k_rc_chunks(xzamd_span_args a, uint32_t nchunk_slots)
{
    const uint32_t idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= nchunk_slots) return;
    const xzamd_chunk c = a.chunks[idx];
    if (c.usize == 0 || (c.flags & XZAMD_CH_RAW)) return;
    const uint16_t* __restrict__ tk = a.tok + (((uint64_t)c.tok_hi << 32) | c.tok_lo);
    uint8_t* const hdr = a.scratch + XZAMD_CHUNK_OUT(c.in_start, idx);
    const uint32_t hl = (c.flags & XZAMD_CH_PROPS) ? 6u : 5u;
    uint8_t* const out = hdr + hl;
    uint32_t low_lo = 0, low_hi = 0, range = 0xFFFFFFFFu, cache = 0, cache_size = 1, cpos = 0;
    const uint32_t cap = c.usize + (c.usize >> 3) + 8u;           // never reached: the chunk was estimated to shrink
    auto shift_low = [&]() {
        if (low_lo < 0xFF000000u || low_hi != 0) {
            uint32_t b = cache + low_hi;
            for (uint32_t i = 0; i < cache_size; ++i) {
                if (cpos < cap) out[cpos] = (uint8_t)b;
                ++cpos;
                b = 0xFFu + low_hi;
            }
            cache_size = 0;
            cache = low_lo >> 24;
        }
        ++cache_size;
        low_lo <<= 8;
        low_hi = 0;
    };
    auto code = [&](uint32_t t) {
        if (range < (1u << 24)) { shift_low(); range <<= 8; }
        const uint32_t bit = (t >> 12) & 1u;
        uint32_t add;
        if (t & 0x8000u) {
            range >>= 1;
            add = bit ? range : 0u;
        } else {
            const uint32_t bound = (range >> 11) * (t & 0xFFFu);
            add = bit ? bound : 0u;
            range = bit ? range - bound : bound;
        }
        const uint32_t nl = low_lo + add;
        low_hi += nl < low_lo ? 1u : 0u;
        low_lo = nl;
    };
    // tokens eight at a time (one 16-byte load per lane), the next eight in flight while these are coded: a lane's token
    // stream is sequential, but a 2-byte load per decision would put the cache latency in front of every one of them
    auto load8 = [&](uint32_t i) -> uint4 {
        uint4 v;
        __builtin_memcpy(&v, tk + i, 16);        // (the token buffer has 64 spare entries behind the last token)
        return v;
    };
    uint4 cur = make_uint4(0, 0, 0, 0);
    if (c.ntok) cur = load8(0);
    for (uint32_t i = 0; i < c.ntok; i += 8) {
        uint4 nxt = cur;
        if (i + 8 < c.ntok) nxt = load8(i + 8);
        const uint32_t left = c.ntok - i;
        code(cur.x & 0xFFFFu);
        if (left > 1) code(cur.x >> 16);
        if (left > 2) code(cur.y & 0xFFFFu);
        if (left > 3) code(cur.y >> 16);
        if (left > 4) code(cur.z & 0xFFFFu);
        if (left > 5) code(cur.z >> 16);
        if (left > 6) code(cur.w & 0xFFFFu);
        if (left > 7) code(cur.w >> 16);
        cur = nxt;
    }
    if (range < (1u << 24)) { shift_low(); range <<= 8; }     // the queue loop normalizes before the first RC_FLUSH
    for (int i = 0; i < 5; ++i) shift_low();
    const uint32_t csize = cpos;
    uint32_t ctl;
    if (c.flags & XZAMD_CH_PROPS) ctl = (c.flags & XZAMD_CH_DICT_RESET) ? 0xE0u : 0xC0u;
    else ctl = (c.flags & XZAMD_CH_STATE_RESET) ? 0xA0u : 0x80u;
    hdr[0] = (uint8_t)(ctl + ((c.usize - 1) >> 16));
    hdr[1] = (uint8_t)((c.usize - 1) >> 8);
    hdr[2] = (uint8_t)(c.usize - 1);
    hdr[3] = (uint8_t)((csize - 1) >> 8);
    hdr[4] = (uint8_t)(csize - 1);
    if (c.flags & XZAMD_CH_PROPS) {
        // (a lane per chunk: the Block of the chunk, hence its pair, differs from lane to lane)
        const uint32_t pr = a.props_tab != nullptr ? a.props_tab[c.in_start / a.block_size] : (a.lc | a.lp << 8);
        hdr[5] = (uint8_t)((a.pb * 5 + (pr >> 8)) * 9 + (pr & 255u));
    }
    a.chunks[idx].csize = hl + csize;
    if ((csize > 65536u || csize >= cap) && a.err) atomicCAS(a.err, 0u, 4u);      // the price sum was far off: cannot happen
}

// ------------------------------------------------------------------------------------------
// Assembly: gather span outputs (and small literal pieces prepared by the host: headers,
// end markers, padding, checks, index, footer) into the final stream buffer.
// One workgroup per copy segment.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_assemble(const xzamd_copy_seg* __restrict__ segs, uint32_t nsegs,
        const uint8_t* __restrict__ scratch, const uint8_t* __restrict__ lits, const uint8_t* __restrict__ in,
        uint8_t* __restrict__ out)
{
    const uint32_t s = blockIdx.x;
    if (s >= nsegs) return;
    const xzamd_copy_seg sg = segs[s];
    const uint8_t* src = sg.kind == 0 ? scratch + sg.src : (sg.kind == 1 ? lits + sg.src : in + sg.src);
    uint8_t* dst = out + sg.dst;
    uint64_t len = sg.len;
    // byte-granular head to 16-byte destination alignment, then 16-byte body when the source
    // happens to be co-aligned, else dword/bytes.
    const uint32_t t = threadIdx.x;
    const uint64_t head = min<uint64_t>(len, (16 - ((uintptr_t)dst & 15)) & 15);
    if (t < head) dst[t] = src[t];
    src += head; dst += head; len -= head;
    if ((((uintptr_t)src) & 15) == 0) {
        const uint64_t nv = len / 16;
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (uint64_t i = t; i < nv; i += 256) d4[i] = s4[i];
        const uint64_t done = nv * 16;
        for (uint64_t i = done + t; i < len; i += 256) dst[i] = src[i];
    } else {
        const uint64_t nv = len / 16;
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (uint64_t i = t; i < nv; i += 256) {
            uint4 v;
            __builtin_memcpy(&v, src + i * 16, 16);
            d4[i] = v;
        }
        const uint64_t done = nv * 16;
        for (uint64_t i = done + t; i < len; i += 256) dst[i] = src[i];
    }
}

} // namespace

// ==========================================================================================
// extern "C" launch wrappers (internal ABI between the plain-C host layer and the kernels)
// ==========================================================================================
extern "C" {

// waves = 0: one wavefront per span; else a persistent launch of min(waves, nspans) wavefronts that pull
// span numbers from *counter (must be zero at launch).
int xzk_span_encode(const xzamd_span_args* a, uint32_t nspans, uint32_t waves, uint32_t* counter, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (nspans == 0) return 0;
    if (!a->span_tab || !a->span_cnt || a->max_spb == 0) return (int)hipErrorInvalidValue;
    const bool persist = waves != 0 && counter != nullptr && waves < nspans;
    const uint32_t grid = persist ? waves : nspans;
    uint32_t* cnt = persist ? counter : nullptr;
    if (a->parser) {
        if ((!a->mlen && !a->list_packed) || !a->mdist) return (int)hipErrorInvalidValue;
        // (the single-phase optimal-parser kernel: explicit spans with the parser -- a test configuration, one window size)
        hipLaunchKernelGGL((k_span_encode_t<2, true>), dim3(grid), dim3(64), 0, st, *a, nspans, cnt);
    } else {
        if (a->sa_window) return (int)hipErrorInvalidValue;      // the fast parser runs on the exact finder only
        hipLaunchKernelGGL((k_span_encode_t<0, false>), dim3(grid), dim3(64), 0, st, *a, nspans, cnt);
    }
    return (int)hipGetLastError();
}

// Two-phase mode, phase 1 of the pipeline: the parse pieces.  phase 0 = the seed piece of every Block, 1 = the others.
int xzk_parse_pieces(const xzamd_span_args* a, uint32_t nblocks, int phase, uint32_t waves, uint32_t* counter, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (nblocks == 0) return 0;
    if ((phase != 0 && (!a->span_tab || !a->span_cnt)) || a->max_spb == 0 || !a->sym_len || !a->sym_dist || !a->prior || !a->lit
            || (!a->mlen && !a->list_packed) || !a->mdist || !a->parser)
        return (int)hipErrorInvalidValue;
    const uint32_t nitems = phase == 0 ? nblocks : nblocks * a->max_spb;
    const bool persist = phase != 0 && waves != 0 && counter != nullptr && waves < nitems;
    const uint32_t grid = persist ? waves : nitems;
    uint32_t* cnt = persist ? counter : nullptr;
    // (specialised for the list format and the stage: launch-time constants the compiler cannot see)
    ParseStage stage;
    if (phase == 0) stage = STAGE_SEED;
    else if (a->iter == XZAMD_ITER_PARTIAL) stage = STAGE_PART_PRIOR;
    else if (a->iter == (XZAMD_ITER_PARTIAL | XZAMD_ITER_SNAP)) stage = STAGE_PART_SNAP;
    else if (a->iter == XZAMD_ITER_SNAP) stage = STAGE_FULL;
    else return (int)hipErrorInvalidValue;               // (pieces in full from the prior: no launch of the pipeline asks for it)
    if (stage != STAGE_SEED && stage != STAGE_FULL && !a->part_tab) return (int)hipErrorInvalidValue;
    if ((stage == STAGE_PART_SNAP || stage == STAGE_FULL) && !a->snap_sr) return (int)hipErrorInvalidValue;
#define XZK_PARSE_LAUNCH(P, S) \
    hipLaunchKernelGGL((k_parse_pieces<WMAX_STD, P, S>), dim3(grid), dim3(64), 0, st, *a, nitems, cnt)
#define XZK_PARSE_STAGE(S) \
    case S: if (a->list_packed) XZK_PARSE_LAUNCH(true, S); else XZK_PARSE_LAUNCH(false, S); break
    switch (stage) {
        XZK_PARSE_STAGE(STAGE_SEED);
        XZK_PARSE_STAGE(STAGE_PART_PRIOR);
        XZK_PARSE_STAGE(STAGE_PART_SNAP);
        XZK_PARSE_STAGE(STAGE_FULL);
    }
#undef XZK_PARSE_STAGE
#undef XZK_PARSE_LAUNCH
    return (int)hipGetLastError();
}

// Two-phase mode, phase 2: the model pass (one wavefront per encode-span slot, the whole model in LDS) and the range
// coder (one lane per chunk slot).
// XZAMD_WALK_LITG=0 / 1 (measurement knob): the literal coders of the model walks in LDS / in global memory
static bool walk_litg()
{
    const char* e = getenv("XZAMD_WALK_LITG");
    return e ? *e == '1' : XZAMD_WALK_LITG_DEFAULT;
}
static uint32_t walk_lds(const xzamd_span_args* a)
{
    const uint32_t n = walk_litg() ? (uint32_t)P_LITERAL : P_LITERAL + (0x300u << (a->lc + a->lp));
    return ((((n + 1) / 2) * 4 + 128) + 15) & ~15u;
}

// the bounds walk and the chain: what every encode span starts from (sub: over the records of parse iteration 1)
static int carried_starts(const xzamd_span_args* a, uint32_t nblocks, bool sub, hipStream_t st)
{
    if (!a->cb_bnd || !a->cb_log || !a->cb_hdr || !a->cb_start || !a->cb_carry || !a->pinfo || !a->span_tab || !a->span_cnt
            || a->model_slots_pad == 0)
        return (int)hipErrorInvalidValue;
    const uint32_t nslots = nblocks * a->max_esb;
    const uint32_t nprob = P_LITERAL + (0x300u << (a->lc + a->lp));
    hipError_t e = hipMemsetAsync(a->cb_log, 0, (size_t)nslots * a->model_slots_pad * XZAMD_LOG_WORDS * 4, st);
    if (e != hipSuccess) return (int)e;
    const bool litg = walk_litg();
    const uint32_t lds = ((litg ? (uint32_t)P_LITERAL : nprob) * 4 + 15) & ~15u;
    if (sub) {
        if (litg) hipLaunchKernelGGL((k_model_walk<2, true>), dim3(nslots), dim3(64), lds, st, *a, nslots);
        else hipLaunchKernelGGL((k_model_walk<2, false>), dim3(nslots), dim3(64), lds, st, *a, nslots);
    } else {
        if (litg) hipLaunchKernelGGL((k_model_walk<1, true>), dim3(nslots), dim3(64), lds, st, *a, nslots);
        else hipLaunchKernelGGL((k_model_walk<1, false>), dim3(nslots), dim3(64), lds, st, *a, nslots);
    }
    hipLaunchKernelGGL(k_model_chain, dim3((a->model_slots_pad + 255) / 256, nblocks), dim3(256), 0, st, *a, nblocks);
    return (int)hipGetLastError();
}

int xzk_encode_syms(const xzamd_span_args* a, uint32_t nblocks, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (nblocks == 0) return 0;
    if (!a->enc_tab || !a->enc_cnt || a->max_esb == 0 || !a->sym_len || !a->sym_dist || !a->scratch || !a->tok || !a->chunks)
        return (int)hipErrorInvalidValue;
    const uint32_t nslots = nblocks * a->max_esb;
    const uint32_t nch = XZAMD_CHUNK_SLOTS(a->n, nslots);
    int r = carried_starts(a, nblocks, false, st);
    if (r) return r;
    hipError_t e = hipMemsetAsync(a->chunks, 0, (size_t)nch * sizeof(xzamd_chunk), st);
    if (e != hipSuccess) return (int)e;
    const uint32_t lds = walk_lds(a);
    if (walk_litg()) hipLaunchKernelGGL((k_model_walk<0, true>), dim3(nslots), dim3(64), lds, st, *a, nslots);
    else hipLaunchKernelGGL((k_model_walk<0, false>), dim3(nslots), dim3(64), lds, st, *a, nslots);
    hipLaunchKernelGGL(k_rc_chunks, dim3((nch + 63) / 64), dim3(64), 0, st, *a, nch);
    return (int)hipGetLastError();
}

int xzk_resume_export(const xzamd_span_args* a, uint32_t nblocks, uint32_t block0, uint8_t* table, uint32_t rec_base,
        uint32_t rec_cap, void* stream_)
{
    if (nblocks == 0) return 0;
    if (!a->enc_tab || !a->enc_cnt || a->max_esb == 0 || !a->resume_sr || !a->cb_start || !table || a->model_slots_pad == 0
            || (a->model_slots_pad & 63u))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_resume_export, dim3(nblocks * a->max_esb), dim3(256), 0, (hipStream_t)stream_, *a, nblocks, block0, table,
            rec_base, rec_cap);
    return (int)hipGetLastError();
}

int xzk_model_snapshots(const xzamd_span_args* a, uint32_t nblocks, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (nblocks == 0) return 0;
    if (!a->enc_tab || !a->enc_cnt || a->max_esb == 0 || !a->sym_len || !a->sym_dist || !a->prior || !a->lit || !a->snap_sr)
        return (int)hipErrorInvalidValue;
    const uint32_t nslots = nblocks * a->max_esb;
    int r = carried_starts(a, nblocks, true, st);
    if (r) return r;
    const uint32_t lds = walk_lds(a);
    if (walk_litg()) hipLaunchKernelGGL((k_model_walk<3, true>), dim3(nslots), dim3(64), lds, st, *a, nslots);
    else hipLaunchKernelGGL((k_model_walk<3, false>), dim3(nslots), dim3(64), lds, st, *a, nslots);
    return (int)hipGetLastError();
}

// wavefronts of the span kernel one CU holds at once (what the launch geometry of the span plan is sized for)
int xzk_span_occupancy(int parser, uint32_t nice_len, int* waves_per_cu)
{
    int nb = 0;
    hipError_t e = !parser ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_span_encode_t<0, false>, 64, 0)
            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_span_encode_t<2, true>, 64, 0);
    *waves_per_cu = nb;
    return (int)e;
}

int xzk_assemble(const xzamd_copy_seg* d_segs, uint32_t nsegs, const uint8_t* d_scratch, const uint8_t* d_lits,
        const uint8_t* d_in, uint8_t* d_out, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (nsegs == 0) return 0;
    hipLaunchKernelGGL(k_assemble, dim3(nsegs), dim3(256), 0, st, d_segs, nsegs, d_scratch, d_lits, d_in, d_out);
    return (int)hipGetLastError();
}

} // extern "C"
