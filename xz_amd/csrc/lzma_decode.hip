// lzma_decode.hip -- MI355X (gfx950) LZMA2 Block decoder: the "other side" of the encode path
// (SURVEY.md 8f.3).  Replaces, for every Block of an .xz Stream resident in HBM, what a worker of the
// reference's threaded decoder runs (common/stream_decoder_mt.c -> block_decoder.c ->
//   lzma/lzma2_decoder.c:54-232   chunk grammar, reset rules
//   lzma/lzma_decoder.c:286-700   symbol decoding, state machine, literal / length / distance trees
//   rangecoder/range_decoder.h    rc init (5 bytes, first must be 0), normalisation, "code == 0" at chunk end).
//
// Parallelism.  LZMA decoding is a serial bit-by-bit recurrence, so a decode unit is one wavefront whose
// control flow is wave-uniform (the scalar unit decodes, the 64 lanes copy match bytes).  Units:
//   * any Stream:            one unit per Block (Blocks never reference each other, doc/faq.txt:156-196);
//   * verification decode:   the caller also passes the ORIGINAL data.  Every LZMA2 chunk that resets the
//                            coder state (control >= 0xA0: our span starts) begins an independent unit,
//                            because match bytes that reach back before the unit are read from the
//                            original instead of from a neighbour's unfinished output.  The decoded bytes
//                            are written out and compared with the original afterwards, so a stream that
//                            only decodes correctly "by luck of the oracle" cannot pass.
//   * plain decode:          every chunk that resets the DICTIONARY (control 0x01 or >= 0xE0) begins an
//                            independent unit: nothing in front of it can be referenced (a distance that
//                            reaches there is DEC_BAD_DISTANCE), so the unit reads only what it wrote itself.
//                            A Block of one dictionary reset -- everything the MT encoders write -- is one unit.
// k_dec_scan walks the chunk headers of every Block (grammar checks of lzma2_decoder.c:67-127) and lists
// the unit starts; k_dec_units decodes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_api.h"
#include "wave.h"
#include "bcj_rules.h"
#include "xzamd_block_parse.h"
#include "xzamd_walk_parse.h"

namespace {

enum : uint32_t {      // error codes (xzamd_dec_block.error)
    DEC_OK = 0, DEC_BAD_CONTROL = 1, DEC_NEED_DICT_RESET = 2, DEC_NEED_PROPS = 3, DEC_BAD_PROPS = 4,
    DEC_TRUNCATED = 5, DEC_SIZE_MISMATCH = 6, DEC_BAD_DISTANCE = 7, DEC_RC_INIT = 8, DEC_RC_END = 9,
    DEC_CHUNK_OVERRUN = 10, DEC_UNIT_OVERFLOW = 11, DEC_MISMATCH = 12, DEC_RESUME_MISMATCH = 13
};

// header words of a resume record (xzamd_resume_hdr): [0] Block, [1] upos, [2] lc | lp << 8 | pb << 16 | kind << 24,
// [3] state, [4..7] rep distances
__device__ __forceinline__ const uint32_t* rec_hdr(const uint8_t* tab, uint32_t stride, uint32_t r)
{
    return reinterpret_cast<const uint32_t*>(tab + (uint64_t)r * stride);
}

// One thread per Block: walk the LZMA2 chunk chain, validate the grammar, list the units.
// CHAINS: the table names BARE chunk chains (the segments of a single-Block Stream, XZAMD_F_SEGMENTS) instead of the LZMA2 data
// of Blocks: a chain is exactly csize bytes, has no 0x00 end marker (the byte behind it is the first control byte of the next
// chain, or lies outside the buffer) and ends at c == csize with u == usize; a 0x00 inside it is DEC_SIZE_MISMATCH.  It must
// start with a dictionary reset like any Block's data, so it is a unit of its own on the same grounds.  A template parameter:
// the Block instance compiles to what it compiled to without it.
template <bool CHAINS>
__global__ __launch_bounds__(64) void k_dec_scan(const uint8_t* __restrict__ xz, xzamd_dec_block* __restrict__ blocks,
        uint32_t nblocks, xzamd_dec_unit* __restrict__ units, uint32_t units_cap, int split,
        const uint8_t* __restrict__ rec_tab, uint32_t rec_stride, uint32_t nrec)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    xzamd_dec_block& B = blocks[b];
    const uint8_t* p = xz + B.cpos;
    uint64_t c = 0, u = 0;
    uint32_t nunits = 0, err = DEC_OK;
    uint64_t dbase = 0;                     // Block offset of the last dictionary reset
    bool need_dict_reset = true, need_props = true, ended = false;
    xzamd_dec_unit* U = units + (uint64_t)b * units_cap;
    // split 3: the Block's slice of the sorted records starts at the first record of a Block >= b; `r` is its cursor.  A
    // record is only ever COMPARED here (Block, upos) -- nothing of it becomes an address before a chunk start has met it.
    uint32_t r = 0, nrecs = 0;
    bool self_units = false;
    if (split == 3) {
        uint32_t lo = 0, hi = nrec;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (rec_hdr(rec_tab, rec_stride, mid)[0] < b) lo = mid + 1; else hi = mid; }
        r = lo;
        // a Block all of whose records are void and that is coded all the same (a repaired Block: re-encoded single-phase)
        // gets the units of split 1; a stored Block has no such chunk, so nothing changes for it
        uint32_t q = r;
        while (q < nrec && rec_hdr(rec_tab, rec_stride, q)[0] == b && (rec_hdr(rec_tab, rec_stride, q)[2] >> 24) == XZAMD_RK_VOID) ++q;
        self_units = q > r && !(q < nrec && rec_hdr(rec_tab, rec_stride, q)[0] == b);
    }
    while (c < B.csize) {
        const uint32_t ctl = p[c];
        if (ctl == 0x00) {
            if (CHAINS) { err = DEC_SIZE_MISMATCH; break; }
            ++c; ended = true; break;
        }
        bool starts_unit = nunits == 0;
        uint64_t hs, cs, us;
        if (ctl >= 0x80) {
            if (c + 5 > B.csize) { err = DEC_TRUNCATED; break; }
            us = ((((uint64_t)ctl & 0x1F) << 16) | ((uint64_t)p[c + 1] << 8) | p[c + 2]) + 1;
            cs = (((uint64_t)p[c + 3] << 8) | p[c + 4]) + 1;
            hs = 5;
            if (ctl >= 0xE0) { need_dict_reset = false; dbase = u; }
            if (need_dict_reset) { err = DEC_NEED_DICT_RESET; break; }
            if (ctl >= 0xC0) {
                if (c + 6 > B.csize) { err = DEC_TRUNCATED; break; }
                // lzma_lzma_lclppb_decode: (pb * 5 + lp) * 9 + lc, at most 224, and lc + lp <= 4 -- a properties byte no
                // decoder takes is a defect of the chain's grammar, not of the data coded under it
                if (p[c + 5] > (4 * 5 + 4) * 9 + 8 || (p[c + 5] % 45u) / 9u + p[c + 5] % 9u > 4u) { err = DEC_BAD_PROPS; break; }
                hs = 6;
                need_props = false;
            }
            if (need_props) { err = DEC_NEED_PROPS; break; }
            if (ctl >= 0xC0 && (split == 1 || self_units)) starts_unit = true; // carries the properties and resets the state: self-contained
            if (ctl >= 0xE0 && split == 2) starts_unit = true; // dictionary reset: nothing in front of it is referenced
        } else if (ctl == 0x01 || ctl == 0x02) {
            if (c + 3 > B.csize) { err = DEC_TRUNCATED; break; }
            if (ctl == 0x01) { need_dict_reset = false; need_props = true; dbase = u; }     // lzma2_decoder.c:121-127
            if (need_dict_reset) { err = DEC_NEED_DICT_RESET; break; }
            us = (((uint64_t)p[c + 1] << 8) | p[c + 2]) + 1;
            cs = us;
            hs = 3;
            if (ctl == 0x01 && split == 2) starts_unit = true;
        } else { err = DEC_BAD_CONTROL; break; }
        if (c + hs + cs > B.csize || u + us > B.usize) { err = DEC_SIZE_MISMATCH; break; }
        // split 2: the unit count is data.  A full table is no error there: further resets stay inside the last unit
        // (decode_units follows a dictionary reset in the middle of a unit)
        if (starts_unit && split == 2 && nunits == units_cap) starts_unit = false;
        uint32_t urec = XZAMD_RESUME_NONE;
        if (split == 3) {
            // (the records of a Block that went out stored match nothing: skipped)
            while (r < nrec && rec_hdr(rec_tab, rec_stride, r)[0] == b && (rec_hdr(rec_tab, rec_stride, r)[2] >> 24) == XZAMD_RK_VOID) ++r;
            if (r < nrec && rec_hdr(rec_tab, rec_stride, r)[0] == b) {
                const uint32_t ru = rec_hdr(rec_tab, rec_stride, r)[1];
                if (ru == u) { starts_unit = true; urec = r; ++r; ++nrecs; }
                else if (ru < u) { err = DEC_RESUME_MISMATCH; break; }      // no chunk starts where the record says its span does
            }
        }
        if (starts_unit) {
            if (nunits == units_cap) { err = DEC_UNIT_OVERFLOW; break; }
            U[nunits].cpos = B.cpos + c;
            U[nunits].upos = u;
            U[nunits].block = b;
            U[nunits].dbase = (uint32_t)dbase;
            U[nunits].rec = urec;
            U[nunits].pad_ = 0;
            ++nunits;
        }
        c += hs + cs;
        u += us;
    }
    if (err == DEC_OK && ((!CHAINS && !ended) || c != B.csize || u != B.usize)) err = DEC_SIZE_MISMATCH;
    if (err == DEC_OK && split == 3) {
        // a record left over: its span start lies behind the Block's last chunk
        while (r < nrec && rec_hdr(rec_tab, rec_stride, r)[0] == b && (rec_hdr(rec_tab, rec_stride, r)[2] >> 24) == XZAMD_RK_VOID) ++r;
        if (r < nrec && rec_hdr(rec_tab, rec_stride, r)[0] == b) err = DEC_RESUME_MISMATCH;
    }
    B.nrecs = nrecs;
    B.nunits = nunits;
    B.error = err;
}

// One thread per Block of a whole .xz file (any number of Streams): what the host loop of xzamd_stream_decode_device
// does per Block with three device-to-host reads -- Block Header (size byte, CRC32, flags, VLIs, Filter Flags, padding,
// chain rule), sizes against the Index record, Block Padding, the stored Check -- in the same order (xzb_block is that
// loop's text), so that the first defect of a Block gives the code the host parser gives.  Latency-bound table work:
// every thread reads a few dozen bytes of its own Block, one upload / launch / read-back per file instead of three
// synchronous reads per Block.  No read outside [hpos, end) of the Block's record, and `end` is clamped to the file.
__global__ __launch_bounds__(64) void k_dec_headers(const uint8_t* __restrict__ xz, uint64_t xz_size,
        const xzamd_hdr_rec* __restrict__ recs, uint32_t nblocks, xzamd_dec_block* __restrict__ blocks,
        xzamd_dec_chain* __restrict__ chains, uint8_t* __restrict__ stored, xzamd_hdr_err* __restrict__ errs)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    xzamd_hdr_rec r = recs[b];
    xzamd_dec_block B;
    xzamd_dec_chain ch;
    uint32_t step = XZB_S_NONE, code;
    if (r.end > xz_size) {
        // a record the host must never write: nothing of the file is read for it
        r.hpos = r.end = 0;
    }
    code = xzb_block(xz, &r, &B, &ch, stored + (uint64_t)b * XZAMD_HDR_CHECK_BYTES, &step);
    blocks[b] = B;
    chains[b] = ch;
    errs[b].code = code;
    errs[b].step = step;
}

// The forward walk: the Block table of one Stream without its Index (xzw_walk, xzamd_walk_parse.h: the text the CPU harness
// runs too).  Header -> sizes -> next header is a dependent chain, so one wavefront is all that can be spent on it: every
// lane follows the same addresses, the loaded header bytes are made wave-uniform (readfirstlane) so that the branches are
// scalar, and lane 0 alone stores the rows and the result with plain vector stores.  About one HBM-miss load per hop: a Block
// with both sizes in its header is one hop, any other one hop per LZMA2 chunk.  No atomics, no waits on other wavefronts;
// every read is bounded by `size`, and each iteration moves its offset forward, so the walk ends after at most `size` steps.
__global__ __launch_bounds__(64) void k_dec_walk(const uint8_t* __restrict__ xz, uint64_t size, uint64_t pos0, uint32_t csz,
        uint64_t upos0, xzamd_hdr_rec* __restrict__ rows, uint32_t cap, xzamd_walk_result* __restrict__ res)
{
    xzw_walk(xz, size, pos0, csz, upos0, rows, cap, res);
}

// ---- range decoder + LZMA symbol decoder, wave-uniform -------------------------------------------------
enum : uint32_t {
    D_IS_MATCH = 0, D_IS_REP = 192, D_IS_REP0 = 204, D_IS_REP1 = 216, D_IS_REP2 = 228, D_IS_REP0_LONG = 240,
    D_DIST_SLOT = 432, D_DIST_SPECIAL = 688, D_DIST_ALIGN = 802, D_MATCH_LEN = 818,
    L_CHOICE = 0, L_CHOICE2 = 1, L_LOW = 2, L_MID = 2 + 128, L_HIGH = 2 + 256, L_SIZE = 2 + 256 + 256,
    D_REP_LEN = D_MATCH_LEN + L_SIZE, D_TOTAL = D_REP_LEN + L_SIZE          // 1846
};

struct Rd {
    const uint8_t* in;      // chunk payload
    uint32_t pos, end;      // next byte / payload size
    uint32_t range, code;
    bool over;              // read past the payload
};

__device__ __forceinline__ uint32_t rd_byte(Rd& r)
{
    if (r.pos >= r.end) { r.over = true; return 0; }
    return uni(r.in[r.pos++]);
}
__device__ __forceinline__ void rd_norm(Rd& r)
{
    if (r.range < (1u << 24)) { r.range <<= 8; r.code = (r.code << 8) | rd_byte(r); }
}
__device__ __forceinline__ uint32_t rd_bit(Rd& r, uint16_t* probs, uint32_t idx)
{
    rd_norm(r);
    uint32_t p = uni(probs[idx]);
    const uint32_t bound = (r.range >> 11) * p;
    uint32_t bit;
    if (r.code < bound) { r.range = bound; p += (2048 - p) >> 5; bit = 0; }
    else { r.range -= bound; r.code -= bound; p -= p >> 5; bit = 1; }
    if (threadIdx.x == 0) probs[idx] = (uint16_t)p;
    wave_sync();
    return bit;
}
__device__ __forceinline__ uint32_t rd_tree(Rd& r, uint16_t* probs, uint32_t base, uint32_t nbits)
{
    uint32_t m = 1;
    for (uint32_t i = 0; i < nbits; ++i) m = (m << 1) | rd_bit(r, probs, base + m);
    return m - (1u << nbits);
}
__device__ __forceinline__ uint32_t rd_tree_rev(Rd& r, uint16_t* probs, uint32_t base, uint32_t nbits)
{
    uint32_t m = 1, sym = 0;
    for (uint32_t i = 0; i < nbits; ++i) {
        const uint32_t b = rd_bit(r, probs, base + m);
        m = (m << 1) | b;
        sym |= b << i;
    }
    return sym;
}
__device__ __forceinline__ uint32_t rd_direct(Rd& r, uint32_t nbits)
{
    uint32_t v = 0;
    for (uint32_t i = 0; i < nbits; ++i) {
        rd_norm(r);
        r.range >>= 1;
        const uint32_t t = (r.code >= r.range) ? 1u : 0u;
        if (t) r.code -= r.range;
        v = (v << 1) | t;
    }
    return v;
}
__device__ __forceinline__ uint32_t rd_len(Rd& r, uint16_t* probs, uint32_t base, uint32_t ps)
{
    if (!rd_bit(r, probs, base + L_CHOICE)) return 2 + rd_tree(r, probs, base + L_LOW + ps * 8, 3);
    if (!rd_bit(r, probs, base + L_CHOICE2)) return 10 + rd_tree(r, probs, base + L_MID + ps * 8, 3);
    return 18 + rd_tree(r, probs, base + L_HIGH, 8);
}

// literal-coder probabilities in global memory (one slice per resident wavefront): uniform accesses
__device__ __forceinline__ uint32_t rd_bit_g(Rd& r, uint16_t* g, uint32_t idx)
{
    rd_norm(r);
    uint32_t p = uni(__hip_atomic_load(g + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const uint32_t bound = (r.range >> 11) * p;
    uint32_t bit;
    if (r.code < bound) { r.range = bound; p += (2048 - p) >> 5; bit = 0; }
    else { r.range -= bound; r.code -= bound; p -= p >> 5; bit = 1; }
    if (threadIdx.x == 0) __hip_atomic_store(g + idx, (uint16_t)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return bit;
}

__device__ __forceinline__ uint8_t dict_byte(const uint8_t* src, uint64_t off)
{
    return __hip_atomic_load(src + off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr uint32_t offs[] = XZAMD_MODEL_OFFSETS;

// Decode the units [u0, u1) of one Block in order.  `hist` = where bytes before the current position are
// read from: the output itself (plain decode) or the original data (verification decode).
__device__ __noinline__ void decode_units(const uint8_t* __restrict__ xz, const xzamd_dec_block& B, const xzamd_dec_unit* U,
        uint32_t u0, uint32_t u1, uint8_t* __restrict__ out, const uint8_t* hist, bool plain, uint16_t* probs, uint16_t* lit,
        uint32_t* err_out, const uint8_t* __restrict__ rec_tab, uint32_t rec_stride)
{
    static_assert(offs[0] == D_IS_MATCH && offs[1] == D_IS_REP && offs[2] == D_IS_REP0 && offs[3] == D_IS_REP1 && offs[4] == D_IS_REP2
            && offs[5] == D_IS_REP0_LONG && offs[6] == D_DIST_SLOT && offs[7] == D_DIST_SPECIAL && offs[8] == D_DIST_ALIGN
            && offs[9] == D_MATCH_LEN && offs[10] == D_REP_LEN && offs[11] == D_TOTAL, "the layout the resume records are written in");
    const uint32_t lane = threadIdx.x;
    uint8_t* const bout = out + B.upos;                 // this Block's output
    const uint8_t* const bhist = hist + B.upos;         // this Block's history source
    uint32_t err = DEC_OK;
    uint32_t lc = 0, lp = 0, pb = 0, state = 0, rep0 = 0, rep1 = 0, rep2 = 0, rep3 = 0;
    for (uint32_t ui = u0; ui < u1 && err == DEC_OK; ++ui) {
        uint64_t c = U[ui].cpos - B.cpos;               // offset of the unit's first chunk inside the Block's data
        uint64_t u = U[ui].upos;
        uint64_t dbase = U[ui].dbase;                   // bytes before it are outside the dictionary (lz_decoder.h:195-198)
        const uint64_t c_end = ui + 1 < B.nunits ? U[ui + 1].cpos - B.cpos : B.csize;
        const uint8_t* p = xz + B.cpos;
        const uint32_t urec = rec_tab != nullptr ? uni(U[ui].rec) : XZAMD_RESUME_NONE;
        if (urec != XZAMD_RESUME_NONE) {
            // Unit at a resume record (k_dec_scan has met it at this chunk start): properties, coder state, rep distances
            // and the model come from the record instead of from a state reset.  What the record says is checked like
            // stream data: values no coder can be in end the unit, and the rep distance a literal in a match state reads its
            // match byte at lies inside the Block's data so far -- every later use of a distance passes the test at `copy`.
            const uint8_t* R = rec_tab + (uint64_t)urec * rec_stride;
            const uint32_t* H = reinterpret_cast<const uint32_t*>(R);
            const uint32_t w2 = uni(H[2]);
            lc = w2 & 0xFFu; lp = (w2 >> 8) & 0xFFu; pb = (w2 >> 16) & 0xFFu;
            state = uni(H[3]);
            rep0 = uni(H[4]); rep1 = uni(H[5]); rep2 = uni(H[6]); rep3 = uni(H[7]);
            if (lc + lp > 4 || lc > 4 || lp > 4 || pb > 4 || state >= 12) { err = DEC_RESUME_MISMATCH; break; }
            const uint32_t nl = 0x300u << (lc + lp);
            if ((rec_stride & 15u) != 0 || XZAMD_RESUME_HDR + 2u * (D_TOTAL + nl) > rec_stride) { err = DEC_RESUME_MISMATCH; break; }
            if ((w2 >> 24) == XZAMD_RK_CARRIED) {
                // 16 bytes per lane; word w holds probabilities 2 w, 2 w + 1 (D_TOTAL is even: no word straddles LDS and `lit`)
                static_assert(D_TOTAL % 2 == 0, "model words");
                const uint4* __restrict__ M = reinterpret_cast<const uint4*>(R + XZAMD_RESUME_HDR);
                const uint32_t nw = (D_TOTAL + nl) / 2u;
                uint32_t* const lit32 = reinterpret_cast<uint32_t*>(lit);
                for (uint32_t q = lane; q * 4u < nw; q += 64) {
                    const uint4 v = M[q];
                    const uint32_t wv[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                    for (uint32_t t = 0; t < 4; ++t) {
                        const uint32_t w = q * 4u + t;
                        if (w < D_TOTAL / 2u) { probs[2 * w] = (uint16_t)wv[t]; probs[2 * w + 1] = (uint16_t)(wv[t] >> 16); }
                        else if (w < nw) lit32[w - D_TOTAL / 2u] = wv[t];
                    }
                }
            } else {
                for (uint32_t i = lane; i < D_TOTAL; i += 64) probs[i] = 1024;
                for (uint32_t i = lane; i < nl; i += 64) lit[i] = 1024;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            wave_sync();
            if (state >= 7 && (uint64_t)rep0 >= u - dbase) { err = DEC_BAD_DISTANCE; break; }
        }
        while (c < c_end && err == DEC_OK) {
            const uint32_t ctl = uni(p[c]);
            if (ctl == 0x00) { ++c; break; }
            if (ctl == 0x01 || ctl >= 0xE0) dbase = u;      // dictionary reset
            if (ctl < 0x80) {
                // uncompressed chunk: copy
                const uint32_t us = ((uni(p[c + 1]) << 8) | uni(p[c + 2])) + 1;
                for (uint32_t i = lane; i < us; i += 64) bout[u + i] = p[c + 3 + i];
                if (plain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                c += 3 + us; u += us;
                continue;
            }
            const uint32_t us = (((ctl & 0x1F) << 16) | (uni(p[c + 1]) << 8) | uni(p[c + 2])) + 1;
            const uint32_t cs = ((uni(p[c + 3]) << 8) | uni(p[c + 4])) + 1;
            uint32_t hs = 5;
            if (ctl >= 0xC0) {
                uint32_t d = uni(p[c + 5]);
                pb = d / 45; d -= pb * 45; lp = d / 9; lc = d - lp * 9;
                if (lc + lp > 4) { err = DEC_BAD_PROPS; break; }
                hs = 6;
            }
            if (ctl >= 0xA0) {
                // state reset (lzma_decoder.c:1052-1100)
                for (uint32_t i = lane; i < D_TOTAL; i += 64) probs[i] = 1024;
                const uint32_t nl = 0x300u << (lc + lp);
                for (uint32_t i = lane; i < nl; i += 64) lit[i] = 1024;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                wave_sync();
                state = 0; rep0 = rep1 = rep2 = rep3 = 0;
            }
            Rd r;
            r.in = p + c + hs; r.pos = 0; r.end = cs; r.over = false;
            // rc init: range_decoder.h:85-100 (first byte must be 0, then 4 bytes of code)
            if (cs < 5 || uni(r.in[0]) != 0) { err = DEC_RC_INIT; break; }
            r.pos = 1; r.range = 0xFFFFFFFFu; r.code = 0;
            for (int i = 0; i < 4; ++i) r.code = (r.code << 8) | rd_byte(r);
            const uint64_t u_end = u + us;
            const uint32_t pbm = (1u << pb) - 1, lpm = (1u << lp) - 1;
            while (u < u_end) {
                const uint32_t ps = (uint32_t)(u - dbase) & pbm;      // positions count from the last dictionary reset
                if (!rd_bit(r, probs, D_IS_MATCH + state * 16 + ps)) {
                    // literal (lzma_decoder.c:330-400)
                    const uint32_t prev = u > dbase ? (plain ? dict_byte(bout, u - 1) : bhist[u - 1]) : 0u;
                    uint16_t* sub = lit + 0x300u * ((((uint32_t)(u - dbase) & lpm) << lc) + (uni(prev) >> (8 - lc)));
                    uint32_t sym = 1;
                    if (state < 7) {
                        do { sym = (sym << 1) | rd_bit_g(r, sub, sym); } while (sym < 0x100);
                    } else {
                        uint32_t mb = uni(plain ? dict_byte(bout, u - rep0 - 1) : bhist[u - rep0 - 1]);
                        uint32_t off = 0x100;
                        do {
                            mb <<= 1;
                            const uint32_t mbit = mb & off;
                            const uint32_t b = rd_bit_g(r, sub, off + mbit + sym);
                            sym = (sym << 1) | b;
                            off &= b ? mbit : ~mbit;
                        } while (sym < 0x100);
                    }
                    if (lane == 0) bout[u] = (uint8_t)sym;
                    if (plain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    state = state <= 3 ? 0 : (state <= 9 ? state - 3 : state - 6);
                    ++u;
                    continue;
                }
                uint32_t len;
                if (rd_bit(r, probs, D_IS_REP + state)) {
                    if (!rd_bit(r, probs, D_IS_REP0 + state)) {
                        if (!rd_bit(r, probs, D_IS_REP0_LONG + state * 16 + ps)) {
                            // short rep
                            state = state < 7 ? 9 : 11;
                            len = 1;
                            goto copy;
                        }
                    } else {
                        uint32_t d;
                        if (!rd_bit(r, probs, D_IS_REP1 + state)) { d = rep1; }
                        else {
                            if (!rd_bit(r, probs, D_IS_REP2 + state)) { d = rep2; }
                            else { d = rep3; rep3 = rep2; }
                            rep2 = rep1;
                        }
                        rep1 = rep0;
                        rep0 = d;
                    }
                    state = state < 7 ? 8 : 11;
                    len = rd_len(r, probs, D_REP_LEN, ps);
                } else {
                    rep3 = rep2; rep2 = rep1; rep1 = rep0;
                    len = rd_len(r, probs, D_MATCH_LEN, ps);
                    state = state < 7 ? 7 : 10;
                    const uint32_t ds = len < 6 ? len - 2 : 3;
                    const uint32_t slot = rd_tree(r, probs, D_DIST_SLOT + ds * 64, 6);
                    if (slot < 4) rep0 = slot;
                    else {
                        const uint32_t fb = (slot >> 1) - 1;
                        rep0 = (2 | (slot & 1)) << fb;
                        if (slot < 14) rep0 += rd_tree_rev(r, probs, D_DIST_SPECIAL + rep0 - slot - 1, fb);
                        else {
                            rep0 += rd_direct(r, fb - 4) << 4;
                            rep0 += rd_tree_rev(r, probs, D_DIST_ALIGN, 4);
                        }
                    }
                }
            copy:
                // dict_is_distance_valid (lzma_decoder.c:530,549): inside the data so far and the dictionary
                if ((uint64_t)rep0 >= u - dbase || rep0 >= B.dict_size) { err = DEC_BAD_DISTANCE; break; }
                if (u + len > u_end) { err = DEC_CHUNK_OVERRUN; break; }
                {
                    const uint32_t period = rep0 + 1;
                    for (uint32_t i = lane; i < len; i += 64) {
                        // bytes the match copies from itself repeat with period rep0 + 1
                        const uint64_t so = u - period + (i % period);
                        bout[u + i] = plain ? dict_byte(bout, so) : bhist[so];
                    }
                    if (plain) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                u += len;
            }
            if (err != DEC_OK) break;
            // chunk end: all payload used, code back to 0 (range_decoder.h:139-140, lzma2_decoder.c:196-212)
            rd_norm(r);
            if (r.over) { err = DEC_TRUNCATED; break; }
            if (r.pos != r.end || r.code != 0) { err = DEC_RC_END; break; }
            c += hs + cs;
        }
    }
    // plain decode: units of a Block may run side by side, the Block's code is that of its lowest-numbered failing unit
    // (code in the low byte; the host reads "not zero")
    if (err != DEC_OK && lane == 0) {
        if (plain) atomicMax(err_out, ((0xFFFFFFu - min(u0, 0xFFFFFEu)) << 8) | err);
        else atomicCAS(err_out, 0u, err);
    }
}

// expected == nullptr, per_unit == 0: one wavefront per Block; verification (expected): one wavefront per unit of the
// flattened list, history = original data; plain with per_unit (units start at dictionary resets): one wavefront per
// unit, history = the output itself -- dbase of such a unit is its own start, so no unit reads what another writes
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_dec_units(const uint8_t* __restrict__ xz, const xzamd_dec_block* __restrict__ blocks,
        uint32_t nblocks, const xzamd_dec_unit* __restrict__ units, uint32_t units_cap, const uint32_t* __restrict__ unit_first,
        uint32_t total_units, uint8_t* __restrict__ out, const uint8_t* __restrict__ expected,
        uint16_t* __restrict__ lit_pool, uint32_t* __restrict__ counter, uint32_t* __restrict__ block_err, int per_unit,
        const uint8_t* __restrict__ rec_tab, uint32_t rec_stride)
{
    __shared__ uint16_t probs[D_TOTAL + 2];
    uint16_t* lit = lit_pool + (uint64_t)blockIdx.x * (0x300u << 4);
    const bool flat = expected != nullptr || per_unit != 0;       // kernel arguments: wave-uniform
    const uint32_t total = flat ? total_units : nblocks;
    for (;;) {
        uint32_t w = 0;
        if (threadIdx.x == 0) w = atomicAdd(counter, 1u);
        w = uni(w);
        if (w >= total) break;
        uint32_t bi = w, k0 = 0, k1 = 0;
        if (flat) {
            // unit w of the flattened list: find its Block (unit_first = exclusive prefix sum of nunits)
            uint32_t lo = 0, hi = nblocks;
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (unit_first[mid] <= w) lo = mid; else hi = mid; }
            bi = lo;
            k0 = w - unit_first[lo];
            k1 = k0 + 1;
        } else {
            k1 = blocks[w].nunits;
        }
        const xzamd_dec_block& B = blocks[bi];
        if (B.error == DEC_OK)
            decode_units(xz, B, units + (uint64_t)bi * units_cap, k0, k1, out, expected ? expected : out, expected == nullptr,
                    probs, lit, block_err + bi, rec_tab, rec_stride);
        __builtin_amdgcn_s_waitcnt(0);
        wave_sync();
    }
}

// verification: count bytes that differ from the original
__global__ __launch_bounds__(256) void k_dec_compare(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n,
        unsigned long long* __restrict__ mismatches)
{
    uint64_t bad = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; i < n; i += stride) {
        if (i + 16 <= n) {
            uint4 x, y;
            __builtin_memcpy(&x, a + i, 16);
            __builtin_memcpy(&y, b + i, 16);
            bad += (x.x != y.x) + (x.y != y.y) + (x.z != y.z) + (x.w != y.w);
        } else {
            for (uint64_t k = i; k < n; ++k) bad += a[k] != b[k];
        }
    }
    if (bad) atomicAdd(mismatches, (unsigned long long)bad);
}

// bytes of a 32-bit word that are not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
    w |= w >> 4; w |= w >> 2; w |= w >> 1;
    return (uint32_t)__popc(w & 0x01010101u);
}

// Per-Block verification: bytes of every Block that differ from the original, one 64-bit count per Block.  One workgroup
// per tile of XZAMD_UNF_TILE bytes of a Block; tile_first (nblocks + 1, exclusive prefix sum) maps a tile to its Block as in
// unf_locate, and a Block the host gives no tiles (one that failed an earlier step) is not read.  A Block starts at any
// byte offset: the tile's head up to the next 16-byte boundary of the decoded bytes and its tail go byte by byte, the
// interior in 16-byte loads (the original is read unaligned when it is not co-aligned).  The count is summed over the
// wavefront on the DPP network; a wavefront that found differences issues one atomic.
__global__ __launch_bounds__(256) void k_dec_compare_blocks(const uint8_t* __restrict__ out, const uint8_t* __restrict__ expected,
        const xzamd_dec_block* __restrict__ blocks, const uint32_t* __restrict__ tile_first, uint32_t nblocks,
        unsigned long long* __restrict__ counts)
{
    const uint32_t tile = blockIdx.x;
    uint32_t lo = 0, hi = nblocks;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (tile_first[mid] <= tile) lo = mid; else hi = mid; }
    const uint64_t usize = blocks[lo].usize;
    const uint64_t p0 = (uint64_t)(tile - tile_first[lo]) * XZAMD_UNF_TILE;
    if (tile < tile_first[lo] || tile >= tile_first[lo + 1] || p0 >= usize) return;     // (a table that does not cover the tile)
    const uint32_t len = (uint32_t)(usize - p0 < XZAMD_UNF_TILE ? usize - p0 : XZAMD_UNF_TILE);
    const uint8_t* a = out + blocks[lo].upos + p0;
    const uint8_t* e = expected + blocks[lo].upos + p0;
    const uint32_t t = threadIdx.x;
    uint32_t head = (16u - (uint32_t)((uintptr_t)a & 15u)) & 15u;
    if (head > len) head = len;
    const uint32_t nvec = (len - head) / 16u, tail0 = head + nvec * 16u;
    uint32_t bad = 0;
    if (t < head) bad += a[t] != e[t];
    if (t < len - tail0) bad += a[tail0 + t] != e[tail0 + t];
    const uint4* a4 = reinterpret_cast<const uint4*>(a + head);
    const bool co_aligned = ((uintptr_t)(e + head) & 15u) == 0;       // wave-uniform
    for (uint32_t v = t; v < nvec; v += 256) {
        const uint4 x = a4[v];
        uint4 y;
        if (co_aligned) y = reinterpret_cast<const uint4*>(e + head)[v];
        else __builtin_memcpy(&y, e + head + 16u * v, 16);
        const uint32_t d0 = x.x ^ y.x, d1 = x.y ^ y.y, d2 = x.z ^ y.z, d3 = x.w ^ y.w;
        if (d0 | d1 | d2 | d3) bad += nonzero_bytes(d0) + nonzero_bytes(d1) + nonzero_bytes(d2) + nonzero_bytes(d3);
    }
    const uint32_t sum = wave_sum_dpp(bad);
    if (sum != 0 && (t & 63u) == 0) atomicAdd(counts + lo, (unsigned long long)sum);
}

// Repair: the records of the Blocks flagged in `bad` (one byte per Block of the Stream) match nothing any more
__global__ __launch_bounds__(256) void k_resume_void_blocks(uint8_t* __restrict__ tab, uint32_t stride, uint32_t nrec,
        const uint8_t* __restrict__ bad, uint32_t nblocks)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    const uint32_t b = rec_hdr(tab, stride, r)[0];
    if (b < nblocks && bad[b]) tab[(uint64_t)r * stride + XZAMD_RESUME_KIND_OFF] = (uint8_t)XZAMD_RK_VOID;
}

// ------------------------------------------------------------------------------------------
// Inverse filters: what the reference's decoder chain runs behind the LZMA2 decoder of a Block
// (simple/simple_coder.c with the decoder branch of x86.c, powerpc.c, ia64.c, arm.c, armthumb.c, sparc.c,
// arm64.c, riscv.c:633-753; delta/delta_decoder.c), one fresh filter per Block, start offset 0.
// A stage reads one buffer and writes another (xzamd_unf_args), because the chunk owners of the x86 and
// RISC-V walks read bytes a neighbouring owner is about to patch.  Work is cut into tiles of
// XZAMD_UNF_TILE bytes of a Block; tile_first maps a tile to its Block, so Blocks may differ in length
// and in chain.
// ------------------------------------------------------------------------------------------
constexpr uint32_t UNF_TILE = XZAMD_UNF_TILE;
constexpr uint32_t UNF_ROW = XZAMD_UNF_ROW;
constexpr uint32_t UNF_CHUNK = UNF_TILE / 256;       // bytes per owner thread of the x86 / RISC-V walks

struct UnfTile {
    const uint8_t* src;     // the Block's bytes before this stage
    uint8_t* dst;           // ... and after it
    uint32_t usize;         // the Block's length
    uint32_t t;             // tile inside the Block
    uint32_t ntiles;
    uint32_t filt;          // id | parameter << 8; 0 = copy
    uint32_t block;
};

// wave-uniform: which Block a tile of the stage belongs to
__device__ __forceinline__ void unf_locate(const xzamd_unf_args& a, uint32_t tile, UnfTile& T)
{
    uint32_t lo = 0, hi = a.nblocks;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (a.tile_first[mid] <= tile) lo = mid; else hi = mid; }
    const xzamd_dec_chain& ch = a.chains[lo];
    const uint64_t upos = a.blocks[lo].upos;
    T.block = lo;
    T.usize = (uint32_t)a.blocks[lo].usize;
    T.t = tile - a.tile_first[lo];
    T.ntiles = a.tile_first[lo + 1] - a.tile_first[lo];
    T.filt = ch.n > a.stage ? ch.f[ch.n - 1 - a.stage] : 0u;
    T.src = ((a.stage & 1) ? a.t1 : a.t0) + upos;
    T.dst = (a.stage + 1 >= ch.n ? a.out : ((a.stage & 1) ? a.t0 : a.t1)) + upos;
}

// 16 bytes from / to any address; `valid` < 16: only that many bytes exist (the rest read as zero)
__device__ __forceinline__ uint4 ld16(const uint8_t* p, uint32_t valid)
{
    uint4 v;
    if (valid >= 16) {
        if (((uintptr_t)p & 15) == 0) return *reinterpret_cast<const uint4*>(p);
        __builtin_memcpy(&v, p, 16);
        return v;
    }
    uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
        if (i < valid) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    return v;
}
__device__ __forceinline__ void st16(uint8_t* p, uint4 v, uint32_t valid)
{
    if (valid >= 16) {
        if (((uintptr_t)p & 15) == 0) *reinterpret_cast<uint4*>(p) = v;
        else __builtin_memcpy(p, &v, 16);
        return;
    }
    const uint32_t w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
        if (i < valid) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

// dst = src for every tile of the stage that is not delta (the BCJ kernels below write converted operands only)
__global__ __launch_bounds__(256) void k_unf_copy(xzamd_unf_args a)
{
    UnfTile T;
    unf_locate(a, blockIdx.x, T);
    if ((T.filt & 0xFFu) == 3u) return;
    const uint32_t base = T.t * UNF_TILE;
#pragma unroll
    for (uint32_t i = 0; i < UNF_TILE / 4096; ++i) {
        const uint32_t p = base + i * 4096 + threadIdx.x * 16;
        if (p >= T.usize) break;
        const uint32_t valid = min(16u, T.usize - p);
        st16(T.dst + p, ld16(T.src + p, valid), valid);
    }
}

// x86 (simple/x86.c:26-118, is_encoder = false).  The argument above k_x86_bcj (lzma_filters.hip) holds for this
// direction word for word: every decision of the decoder reads its own INPUT only (the filtered bytes: a converted
// operand is skipped, never read again), and (prev_mask, prev_pos) are void at a position with five bytes without
// E8 / E9 in front of it.  So the owner of chunk k starts at the first such synchronisation point of its chunk and
// runs to the first one at or behind the chunk end; without synchronisation points one thread walks on: serial, exact.
__device__ void unf_x86(const uint8_t* __restrict__ b, uint8_t* __restrict__ o, uint32_t size, uint32_t k)
{
    if (size < 5) return;
    const uint32_t limit = size - 5;                 // last position the filter examines
    const uint32_t s = k * UNF_CHUNK;
    if (s > limit) return;
    const uint32_t e = s + UNF_CHUNK;
    uint32_t pos = 0, run = 0;                       // run = non-opcode bytes immediately before pos
    if (k != 0) {
        bool found = false;
        for (uint32_t q = s - 5; q <= limit && q < e; ++q) {
            if (q >= s && run >= 5) { pos = q; found = true; break; }
            run = x86_is_op(b[q]) ? 0u : run + 1;
        }
        if (!found) return;                           // the previous owner runs through this chunk
    }
    uint32_t prev_mask = 0, prev_pos = pos - 6;       // "long ago"
    while (pos <= limit) {
        if (pos >= e && run >= 5) break;              // the next owner's start
        const uint32_t c = b[pos];
        if (!x86_is_op(c)) { ++pos; ++run; continue; }
        const uint32_t offset = pos - prev_pos;
        prev_pos = pos;
        if (offset > 5) prev_mask = 0;
        else for (uint32_t i = 0; i < offset; ++i) prev_mask = (prev_mask & 0x77u) << 1;
        const uint32_t b4 = b[pos + 4];
        if (x86_ms(b4) && (prev_mask >> 1) <= 4 && (prev_mask >> 1) != 3) {
            const uint32_t b1 = b[pos + 1], b2 = b[pos + 2], b3 = b[pos + 3];
            uint32_t src = (b4 << 24) | (b3 << 16) | (b2 << 8) | b1;
            uint32_t dest;
            for (;;) {
                dest = src - (pos + 5);
                if (prev_mask == 0) break;
                const uint32_t pm = prev_mask >> 1;
                const uint32_t i = pm == 0 ? 0u : pm == 1 ? 1u : pm <= 3 ? 2u : 3u;
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

// RISC-V (simple/riscv.c:633-753, decoder).  The decoder examines a position with the same tests as the encoder
// (a JAL with rd x1 / x5; an AUIPC whose rd is not x0 / x2 and that pairs with the next instruction: the "fake" pair it
// re-encodes; an AUIPC in the special form: the real pair it restores) and jumps 2, 4, 6 or 8 bytes accordingly, reading
// only bytes no earlier conversion wrote.  So the walk is cut into chunks by the rule of k_riscv_bcj: a position that
// none of its three predecessors can jump over is examined by every walk.
__device__ __forceinline__ void rv_wr32(uint8_t* p, uint32_t v)
{
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

__device__ void unf_riscv(const uint8_t* __restrict__ b, uint8_t* __restrict__ o, uint32_t size, uint32_t k)
{
    if (size < 8) return;
    const uint32_t limit = size - 8;                 // last position the filter examines
    const uint32_t s = k * UNF_CHUNK;                // even
    if (s > limit) return;
    const uint32_t e = s + UNF_CHUNK;
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
            // JAL: absolute address, big endian -> the pc-relative immediate in its four pieces
            const uint32_t b1 = b[pos + 1];
            if (b1 & 0x0Du) { pos += 2; continue; }
            const uint32_t b2 = b[pos + 2], b3 = b[pos + 3];
            uint32_t addr = ((b1 & 0xF0u) << 13) | (b2 << 9) | (b3 << 1);
            addr -= pos;
            o[pos + 1] = (uint8_t)((b1 & 0x0Fu) | ((addr >> 8) & 0xF0u));
            o[pos + 2] = (uint8_t)(((addr >> 16) & 0x0Fu) | ((addr >> 7) & 0x10u) | ((addr << 4) & 0xE0u));
            o[pos + 3] = (uint8_t)(((addr >> 4) & 0x7Fu) | ((addr >> 13) & 0x80u));
            pos += 4;
        } else if ((b0 & 0x7Fu) == 0x17u) {
            uint32_t inst = rv_rd32(b + pos), inst2;
            if (inst & 0xE80u) {
                // rd other than x0 / x2: a "fake" pair goes back into the special form (no sign extension, no pc)
                inst2 = rv_rd32(b + pos + 4);
                if (rv_not_pair(inst, inst2)) { pos += 6; continue; }
                const uint32_t addr = (inst & 0xFFFFF000u) + (inst2 >> 20);
                inst = 0x17u | (2u << 7) | (inst2 << 12);
                inst2 = addr;
            } else {
                // rd x0 / x2: the special form the encoder wrote becomes the real AUIPC pair again
                if (!rv_special(inst)) { pos += 4; continue; }
                const uint32_t rs1 = inst >> 27;
                const uint8_t* q = b + pos + 4;
                uint32_t addr = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
                addr -= pos;
                inst2 = (inst >> 12) | (addr << 20);
                inst = 0x17u | (rs1 << 7) | ((addr + 0x800u) & 0xFFFFF000u);
            }
            rv_wr32(o + pos, inst);
            rv_wr32(o + pos + 4, inst2);
            pos += 8;
        } else {
            pos += 2;
        }
    }
}

// PowerPC / IA-64 / ARM / ARM-Thumb / SPARC / ARM64: one aligned slot = one thread's work item, pc = offset in the
// Block, subtraction where the encoder adds; the tail shorter than a slot stays as it is.  An ARM-Thumb BL pair keeps
// its 0xF0 / 0xF8 marker bits when it is converted, so here too the halfword behind a pair cannot start another one
// and the slots are independent.
__device__ void unf_slot(const uint8_t* __restrict__ b, uint8_t* __restrict__ o, uint32_t blen, uint32_t pc, uint32_t kind)
{
    const uint8_t* p = b + pc;
    uint8_t* q = o + pc;
    if (kind == 8) {                                      // ARM-Thumb BL pair
        if (blen < 4 || pc > blen - 4) return;
        if ((p[1] & 0xF8u) != 0xF0u || (p[3] & 0xF8u) != 0xF8u) return;
        uint32_t src = ((uint32_t)(p[1] & 7u) << 19) | ((uint32_t)p[0] << 11) | ((uint32_t)(p[3] & 7u) << 8) | p[2];
        src <<= 1;
        const uint32_t dest = (src - (pc + 4)) >> 1;
        q[1] = (uint8_t)(0xF0u | ((dest >> 19) & 7u));
        q[0] = (uint8_t)(dest >> 11);
        q[3] = (uint8_t)(0xF8u | ((dest >> 8) & 7u));
        q[2] = (uint8_t)dest;
    } else if (kind == 6) {                               // IA-64 bundle
        if (pc + 16 > (blen & ~15u)) return;
        uint8_t bun[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) bun[i] = p[i];
        const uint32_t tmpl = bun[0] & 0x1Fu;
        // branch slots by template: 16,17: 4  18,19: 6  22,23: 7  24,25,28,29: 4
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
            const uint32_t dest = (src - pc) >> 4;
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
        if (pc + 4 > (blen & ~3u)) return;
        if (kind == 0x0A) {                               // ARM64 BL / ADRP (little endian)
            uint32_t instr = rv_rd32(p);
            if ((instr >> 26) == 0x25) {
                instr = 0x94000000u | ((instr - (pc >> 2)) & 0x03FFFFFFu);
                rv_wr32(q, instr);
            } else if ((instr & 0x9F000000u) == 0x90000000u) {
                const uint32_t src = ((instr >> 29) & 3) | ((instr >> 3) & 0x001FFFFCu);
                if ((src + 0x00020000u) & 0x001C0000u) return;      // outside +/-512 MiB: not converted, in either direction
                instr &= 0x9000001Fu;
                const uint32_t dest = src - (pc >> 12);
                instr |= (dest & 3) << 29;
                instr |= (dest & 0x0003FFFCu) << 3;
                instr |= (0u - (dest & 0x00020000u)) & 0x00E00000u;
                rv_wr32(q, instr);
            }
        } else if (kind == 7) {                           // ARM BL (little endian, condition "always")
            if (p[3] != 0xEBu) return;
            uint32_t src = ((uint32_t)p[2] << 16) | ((uint32_t)p[1] << 8) | p[0];
            src <<= 2;
            const uint32_t dest = (src - (pc + 8)) >> 2;
            q[2] = (uint8_t)(dest >> 16); q[1] = (uint8_t)(dest >> 8); q[0] = (uint8_t)dest;
        } else if (kind == 5) {                           // PowerPC b/bl with AA = 0, LK = 1 (big endian)
            if ((p[0] >> 2) != 0x12u || (p[3] & 3u) != 1u) return;
            const uint32_t src = ((uint32_t)(p[0] & 3u) << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (p[3] & ~3u);
            const uint32_t dest = src - pc;
            q[0] = (uint8_t)(0x48u | ((dest >> 24) & 3u));
            q[1] = (uint8_t)(dest >> 16);
            q[2] = (uint8_t)(dest >> 8);
            q[3] = (uint8_t)((p[3] & 3u) | (dest & 0xFFu));
        } else if (kind == 9) {                           // SPARC call (big endian)
            if (!((p[0] == 0x40u && (p[1] & 0xC0u) == 0x00u) || (p[0] == 0x7Fu && (p[1] & 0xC0u) == 0xC0u))) return;
            uint32_t src = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            src <<= 2;
            uint32_t dest = (src - pc) >> 2;
            dest = (((0u - ((dest >> 22) & 1u)) << 22) & 0x3FFFFFFFu) | (dest & 0x3FFFFFu) | 0x40000000u;
            q[0] = (uint8_t)(dest >> 24); q[1] = (uint8_t)(dest >> 16); q[2] = (uint8_t)(dest >> 8); q[3] = (uint8_t)dest;
        }
    }
}

// one workgroup per tile: the Block's BCJ filter of this stage (k_unf_copy has made dst a copy of src)
__global__ __launch_bounds__(256) void k_unf_bcj(xzamd_unf_args a)
{
    UnfTile T;
    unf_locate(a, blockIdx.x, T);
    const uint32_t kind = T.filt & 0xFFu;
    if (kind < 4u || kind > 0x0Bu) return;                // copy or delta
    if (kind == 4u) unf_x86(T.src, T.dst, T.usize, T.t * 256 + threadIdx.x);
    else if (kind == 0x0Bu) unf_riscv(T.src, T.dst, T.usize, T.t * 256 + threadIdx.x);
    else {
        const uint32_t unit = kind == 8u ? 2u : kind == 6u ? 16u : 4u;
        const uint32_t base = T.t * UNF_TILE;
        for (uint32_t s = threadIdx.x; s < UNF_TILE / unit; s += 256) {
            const uint32_t pc = base + s * unit;
            if (pc >= T.usize) break;
            unf_slot(T.src, T.dst, T.usize, pc, kind);
        }
    }
}

// ---- delta (delta/delta_decoder.c): out[i] = in[i] + out[i - dist] inside a Block, zero history -----------------
// = dist interleaved prefix sums of bytes (mod 256), as a three-step segmented scan over tiles of UNF_TILE bytes:
//   k_delta_tile_sums   per tile, the byte sum of every residue class i mod dist;
//   k_delta_block_scan  per Block, the exclusive scan of the tile vectors (one lane per residue class);
//   k_delta_apply       per tile, the local scan with its carry-in, written out.
// A wavefront holds 1024 consecutive bytes, 16 per lane (one dwordx4), and scans them by doubling: v += v shifted up
// by dist, 2 dist, 4 dist ... bytes, each shift a lane shift (ds_bpermute) plus a byte alignment, the adds packed
// 4 x u8 without carries between bytes.  It walks its tile in 16 such pieces; the carry from piece to piece (and
// from tile to tile) is "the dist output bytes in front of the piece", added to the piece's first dist input bytes --
// which is the recurrence itself, so no per-class bookkeeping is needed inside a tile.
__device__ __forceinline__ uint32_t padd8(uint32_t a, uint32_t b)
{
    return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
}
__device__ __forceinline__ uint4 padd8(uint4 a, uint4 b)
{
    return make_uint4(padd8(a.x, b.x), padd8(a.y, b.y), padd8(a.z, b.z), padd8(a.w, b.w));
}
__device__ __forceinline__ uint4 lane_get(uint4 v, int lane, int src)
{
    const bool ok = src >= 0 && src < 64;
    const int addr = (ok ? src : lane) << 2;
    uint4 r;
    r.x = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v.x);
    r.y = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v.y);
    r.z = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v.z);
    r.w = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)v.w);
    return ok ? r : make_uint4(0, 0, 0, 0);
}
// The 16 bytes at byte offset 16 * lane + off of the wavefront's 1024-byte vector (zeros outside it); off is wave-uniform.
__device__ __forceinline__ uint4 wave_bytes_at(uint4 v, int off)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int fq = off >> 4;                              // floor
    const uint32_t r = (uint32_t)off & 15u;
    const uint4 A = lane_get(v, lane, lane + fq);
    if (r == 0) return A;
    const uint4 B = lane_get(v, lane, lane + fq + 1);
    const uint32_t rb = r & 3u;
#define XZ_AB(hi, lo) __builtin_amdgcn_alignbyte((hi), (lo), rb)
    switch (r >> 2) {
    case 0: return make_uint4(XZ_AB(A.y, A.x), XZ_AB(A.z, A.y), XZ_AB(A.w, A.z), XZ_AB(B.x, A.w));
    case 1: return make_uint4(XZ_AB(A.z, A.y), XZ_AB(A.w, A.z), XZ_AB(B.x, A.w), XZ_AB(B.y, B.x));
    case 2: return make_uint4(XZ_AB(A.w, A.z), XZ_AB(B.x, A.w), XZ_AB(B.y, B.x), XZ_AB(B.z, B.y));
    default: return make_uint4(XZ_AB(B.x, A.w), XZ_AB(B.y, B.x), XZ_AB(B.z, B.y), XZ_AB(B.w, B.z));
    }
#undef XZ_AB
}

// Scan one tile (bytes [t0, t0 + UNF_TILE) of a Block of `usize` bytes; bytes behind the Block count as zeros).
// `tail` = vector whose first dist bytes are the dist output bytes in front of the tile; returns the same for the
// position behind the tile.
template <bool WRITE>
__device__ __forceinline__ uint4 delta_tile(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t usize,
        uint32_t t0, uint32_t dist, uint4 tail)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t c = 0; c < UNF_TILE; c += 1024) {
        if (WRITE && t0 + c >= usize) break;
        const uint32_t p = t0 + c + lane * 16;
        const uint32_t valid = p < usize ? min(16u, usize - p) : 0u;
        uint4 v = padd8(ld16(src + p, valid), tail);
        for (uint32_t k = dist; k < 1024; k <<= 1) v = padd8(v, wave_bytes_at(v, -(int)k));
        if (WRITE) st16(dst + p, v, valid);
        tail = wave_bytes_at(v, 1024 - (int)dist);
    }
    return tail;
}

__global__ __launch_bounds__(64) void k_delta_tile_sums(xzamd_unf_args a)
{
    UnfTile T;
    unf_locate(a, blockIdx.x, T);
    if ((T.filt & 0xFFu) != 3u || T.t + 1 >= T.ntiles) return;     // nobody reads the sums of a Block's last tile
    const uint32_t dist = (T.filt >> 8) + 1;
    const uint4 tail = delta_tile<false>(T.src, nullptr, T.usize, T.t * UNF_TILE, dist, make_uint4(0, 0, 0, 0));
    // byte j of the row = sum of the residue class of Block offset (tile end + j), j < dist; zeros behind
    if (threadIdx.x < UNF_ROW / 16)
        *reinterpret_cast<uint4*>(a.tile_sum + (uint64_t)blockIdx.x * UNF_ROW + threadIdx.x * 16) = tail;
}

// One workgroup per Block, lane r = residue class r: carry row of tile t, byte j = the output byte at Block offset
// (tile start - dist + j) = the sum of class (tile start + j) mod dist over the tiles in front.
__global__ __launch_bounds__(256) void k_delta_block_scan(xzamd_unf_args a)
{
    const uint32_t b = blockIdx.x;
    const xzamd_dec_chain& ch = a.chains[b];
    const uint32_t filt = ch.n > a.stage ? ch.f[ch.n - 1 - a.stage] : 0u;
    if ((filt & 0xFFu) != 3u) return;
    const uint32_t first = a.tile_first[b], ntiles = a.tile_first[b + 1] - first;
    const uint32_t dist = (filt >> 8) + 1, step = UNF_TILE % dist;
    const uint32_t r = threadIdx.x;
    const bool active = r < dist;
    const uint8_t* __restrict__ S = a.tile_sum + (uint64_t)first * UNF_ROW;
    uint8_t* __restrict__ C = a.tile_carry + (uint64_t)first * UNF_ROW;
    uint32_t acc = 0, jc = active ? r : 0u;               // jc: class r's byte in the carry row of tile t
    for (uint32_t t = 0; t < ntiles; t += 8) {
        uint32_t j[9], s[8];
        j[0] = jc;
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            j[u + 1] = j[u] >= step ? j[u] - step : j[u] + dist - step;     // ... = its byte in the sum row of tile t
            s[u] = (active && t + u + 1 < ntiles) ? S[(uint64_t)(t + u) * UNF_ROW + j[u + 1]] : 0u;
        }
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) {
            if (t + u >= ntiles) break;
            C[(uint64_t)(t + u) * UNF_ROW + (active ? j[u] : r)] = active ? (uint8_t)acc : (uint8_t)0;
            acc += s[u];
        }
        jc = j[8];
    }
}

__global__ __launch_bounds__(64) void k_delta_apply(xzamd_unf_args a)
{
    UnfTile T;
    unf_locate(a, blockIdx.x, T);
    if ((T.filt & 0xFFu) != 3u) return;
    const uint32_t dist = (T.filt >> 8) + 1;
    uint4 tail = make_uint4(0, 0, 0, 0);
    if (threadIdx.x < UNF_ROW / 16)
        tail = *reinterpret_cast<const uint4*>(a.tile_carry + (uint64_t)blockIdx.x * UNF_ROW + threadIdx.x * 16);
    delta_tile<true>(T.src, T.dst, T.usize, T.t * UNF_TILE, dist, tail);
}

} // namespace

extern "C" {

int xzk_dec_scan(const uint8_t* d_xz, xzamd_dec_block* d_blocks, uint32_t nblocks, xzamd_dec_unit* d_units,
        uint32_t units_cap, int split, const uint8_t* d_rec, uint32_t rec_stride, uint32_t nrec, void* stream_)
{
    if (nblocks == 0) return 0;
    if (split == 3 && (!d_rec || rec_stride < XZAMD_RESUME_HDR || (rec_stride & 15u))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dec_scan<false>, dim3((nblocks + 63) / 64), dim3(64), 0, (hipStream_t)stream_, d_xz, d_blocks, nblocks,
            d_units, units_cap, split, d_rec, rec_stride, split == 3 ? nrec : 0u);
    return (int)hipGetLastError();
}

int xzk_dec_scan_chains(const uint8_t* d_chains, xzamd_dec_block* d_blocks, uint32_t nchains, xzamd_dec_unit* d_units,
        uint32_t units_cap, int split, const uint8_t* d_rec, uint32_t rec_stride, uint32_t nrec, void* stream_)
{
    if (nchains == 0) return 0;
    if (split == 3 && (!d_rec || rec_stride < XZAMD_RESUME_HDR || (rec_stride & 15u))) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dec_scan<true>, dim3((nchains + 63) / 64), dim3(64), 0, (hipStream_t)stream_, d_chains, d_blocks, nchains,
            d_units, units_cap, split, d_rec, rec_stride, split == 3 ? nrec : 0u);
    return (int)hipGetLastError();
}

int xzk_dec_headers(const uint8_t* d_xz, uint64_t xz_size, const xzamd_hdr_rec* d_recs, uint32_t nblocks, void* d_table, void* stream_)
{
    if (nblocks == 0) return 0;
    uint8_t* t = (uint8_t*)d_table;
    xzamd_dec_block* blocks = (xzamd_dec_block*)t;
    xzamd_dec_chain* chains = (xzamd_dec_chain*)(blocks + nblocks);
    uint8_t* stored = (uint8_t*)(chains + nblocks);
    xzamd_hdr_err* errs = (xzamd_hdr_err*)(stored + (uint64_t)nblocks * XZAMD_HDR_CHECK_BYTES);
    hipLaunchKernelGGL(k_dec_headers, dim3((nblocks + 63) / 64), dim3(64), 0, (hipStream_t)stream_, d_xz, xz_size, d_recs, nblocks,
            blocks, chains, stored, errs);
    return (int)hipGetLastError();
}

int xzk_dec_walk(const uint8_t* d_xz, uint64_t size, uint64_t pos0, uint32_t csz, uint64_t upos0, xzamd_hdr_rec* d_rows, uint32_t cap,
        xzamd_walk_result* d_res, void* stream_)
{
    if (!d_xz || !d_rows || !d_res || cap == 0 || pos0 > size) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_dec_walk, dim3(1), dim3(64), 0, (hipStream_t)stream_, d_xz, size, pos0, csz, upos0, d_rows, cap, d_res);
    return (int)hipGetLastError();
}

int xzk_dec_units(const uint8_t* d_xz, const xzamd_dec_block* d_blocks, uint32_t nblocks, const xzamd_dec_unit* d_units,
        uint32_t units_cap, const uint32_t* d_unit_first, uint32_t total_units, uint8_t* d_out, const uint8_t* d_expected,
        uint16_t* d_lit_pool, uint32_t waves, uint32_t* d_counter, uint32_t* d_block_err, int per_unit,
        const uint8_t* d_rec, uint32_t rec_stride, void* stream_)
{
    if (d_rec && !d_expected) return (int)hipErrorInvalidValue;        // records belong to the verification decode
    const uint32_t total = (d_expected || per_unit) ? total_units : nblocks;
    if (total == 0) return 0;
    const uint32_t grid = waves < total ? waves : total;
    hipLaunchKernelGGL(k_dec_units, dim3(grid), dim3(64), 0, (hipStream_t)stream_, d_xz, d_blocks, nblocks, d_units, units_cap,
            d_unit_first, total_units, d_out, d_expected, d_lit_pool, d_counter, d_block_err, per_unit, d_rec, rec_stride);
    return (int)hipGetLastError();
}

int xzk_dec_compare(const uint8_t* a, const uint8_t* b, uint64_t n, unsigned long long* d_mismatches, void* stream_)
{
    if (n == 0) return 0;
    uint64_t g = (n / 16 + 255) / 256;
    if (g > 65536) g = 65536;
    if (g == 0) g = 1;
    hipLaunchKernelGGL(k_dec_compare, dim3((uint32_t)g), dim3(256), 0, (hipStream_t)stream_, a, b, n, d_mismatches);
    return (int)hipGetLastError();
}

int xzk_dec_compare_blocks(const uint8_t* d_out, const uint8_t* d_expected, const xzamd_dec_block* d_blocks,
        const uint32_t* d_tile_first, uint32_t nblocks, uint32_t total_tiles, unsigned long long* d_counts, void* stream_)
{
    if (total_tiles == 0 || nblocks == 0) return 0;
    hipLaunchKernelGGL(k_dec_compare_blocks, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream_, d_out, d_expected, d_blocks,
            d_tile_first, nblocks, d_counts);
    return (int)hipGetLastError();
}

int xzk_resume_void_blocks(uint8_t* d_table, uint32_t rec_stride, uint32_t nrec, const uint8_t* d_bad, uint32_t nblocks, void* stream_)
{
    if (nrec == 0 || nblocks == 0) return 0;
    hipLaunchKernelGGL(k_resume_void_blocks, dim3((nrec + 255) / 256), dim3(256), 0, (hipStream_t)stream_, d_table, rec_stride, nrec,
            d_bad, nblocks);
    return (int)hipGetLastError();
}

int xzk_dec_unfilter(const xzamd_unf_args* a, uint32_t total_tiles, uint32_t kinds, void* stream_)
{
    hipStream_t st = (hipStream_t)stream_;
    if (total_tiles == 0 || a->nblocks == 0) return 0;
    if (kinds & XZAMD_UNF_COPY) hipLaunchKernelGGL(k_unf_copy, dim3(total_tiles), dim3(256), 0, st, *a);
    if (kinds & XZAMD_UNF_BCJ) hipLaunchKernelGGL(k_unf_bcj, dim3(total_tiles), dim3(256), 0, st, *a);
    if (kinds & XZAMD_UNF_DELTA) {
        hipLaunchKernelGGL(k_delta_tile_sums, dim3(total_tiles), dim3(64), 0, st, *a);
        hipLaunchKernelGGL(k_delta_block_scan, dim3(a->nblocks), dim3(256), 0, st, *a);
        hipLaunchKernelGGL(k_delta_apply, dim3(total_tiles), dim3(64), 0, st, *a);
    }
    return (int)hipGetLastError();
}

} // extern "C"
