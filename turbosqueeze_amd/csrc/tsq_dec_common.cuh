// tsq_dec_common.cuh -- the chunk phases of the byte-lane block decoders, each written once, and the instrumentation macros.
//
// The reference walks the stream with one dependent load per symbol (tsq_decode.cpp:62-88) and copies every symbol with a
// 16-byte load/store.  Here each 6 KiB chunk of stream is staged in LDS and handled in data-parallel phases by a workgroup of
// 16 wavefronts, with aligned, conflict-free LDS traffic only (an unaligned ds access costs 3.5x an aligned one on gfx950,
// tools/micro/lds_unaligned.hip):
//
//   P0  stage the chunk (prefetched into registers a chunk ahead).
//   P1  every byte offset is parsed AS IF a group (control byte + 4 pairs) started there.
//   P2  pointer doubling: next^2, next^4, next^8, next^16 (all kept).
//   P3  the chain of next^16 hops from the chunk's first group (one dependent LDS hop per 16 groups).
//   P4  one lane per group: its start from the hop it hangs on and the bits of its index, its four pairs' stream positions and
//       output offsets; a block-wide scan gives the groups' output positions.
//   P5  symbols -> bytes: (a) one record word per run of bytes that come from one place, (b) every byte takes its run's record,
//       (c) every byte fetches its value from the stream buffer or the ring of previous output -- or, when its source lies in this
//       same chunk, a pointer to it, (d) asynchronous pointer jumping resolves those pointers, (e) the bytes go to the ring: the
//       chunk is composed IN the ring (77 KiB of LDS: 64 KiB of history + the chunk being built).
//   P7  the chunk's bytes go from the ring to HBM with aligned 16-byte stores (a range read: only those inside its window).
//
// dec_sym_kernel (tsq_dec_sym.cuh) runs all of them on one workgroup per block (dec_range_kernel the same, inside a window);
// dec_duo_kernel (tsq_dec_duo.cuh) runs P0..P4 on PARSE workgroups and P5, P7 on a COPY workgroup.  The kernels are schedules: they call the phases in their own order and keep
// their waits, hand-overs and error exits to themselves.  The LDS layout is a template parameter L (SymLds, DuoCopyLds): every
// layout names its regions sbuf, recw, ent, plist, wsum, misc and ring; P1..P4 also use j1 .. j16, gstart, glen, gout, pairs and sn.
// misc[0] super nodes, [1] groups in chunk, [2] first group over the image budget, [3] group that completes the block, [4] error,
// [5] exit offset of the chain.  The barriers inside a phase are its own; the one that closes P4 and each step of P5 is the
// caller's, which puts work of its own under it.
// Offsets and stream bounds are validated (the reference validates nothing); status codes as the oracle's decoder.
#pragma once

#include <type_traits>

#include "tsq_common.cuh"
#include "tsq_crc32.h"

namespace tsq {

#ifdef TSQ_STATS
__device__ unsigned long long g_dec_stats[16];
__device__ unsigned long long g_dec_wave[48];      // per wavefront of block 0: cycles in the pointer jumping, waiting bytes, loop iterations
#define TSQD_T0() unsigned long long t0_ = __builtin_amdgcn_s_memtime()
#define TSQD_ACC(slot) do { unsigned long long t1_ = __builtin_amdgcn_s_memtime(); st_[slot] += t1_ - t0_; t0_ = t1_; } while (0)
#define TSQD_CNT(slot, v) st_[slot] += (v)
#else
#define TSQD_T0() do {} while (0)
#define TSQD_ACC(slot) do {} while (0)
#define TSQD_CNT(slot, v) do {} while (0)
#endif

struct SymCfg {
    static constexpr uint32_t T = 1024;
    static constexpr uint32_t S = 6144;                    // stream bytes per chunk
    static constexpr uint32_t SPAD = 160;                  // a group is at most 133 bytes
    static constexpr uint32_t OUTC = 2 * S;                // output bytes per chunk at most
    static constexpr uint32_t HOP = 16;
    static constexpr uint32_t MAXG = 512;                  // >= S / 13 + 2 * HOP, a multiple of HOP
    static constexpr uint32_t MAXSN = MAXG / HOP + 2;
    static constexpr uint32_t PER = S / T;                 // stream offsets per lane in P1 / P2
    static constexpr uint32_t TERM = S + SPAD;             // "no group here": beyond every real offset
    static constexpr uint32_t R = 65536 + OUTC + 64;       // ring: 64 KiB of history + the chunk being built (a multiple of 16)
    static constexpr uint32_t RPAD = 64;                   // slack behind the ring (the bytes past an image's end inherit its last record)
    static constexpr uint32_t SWORDS = (S + SPAD + 16) / 16;   // 16-byte words of stream staged per chunk
};
static_assert(SymCfg::R % 16 == 0, "ring phase");
static_assert(SymCfg::R == 77888 && SymCfg::R % 64 == 0, "the record scan skews the ring by out_at & 63: the 64-position grid of the bit map falls on the ring's");
static_assert(SymCfg::OUTC == 12 * SymCfg::T, "twelve bytes per lane");
static_assert(SymCfg::S % SymCfg::T == 0 && SymCfg::SWORDS <= SymCfg::T, "lane counts");
static_assert(SymCfg::MAXG <= SymCfg::T / 2 && SymCfg::MAXG % SymCfg::HOP == 0 && SymCfg::MAXG >= SymCfg::S / 13 + 2 * SymCfg::HOP, "group table");
static_assert(4 * SymCfg::MAXG <= 2 * SymCfg::T, "at most two pairs per lane");

// stream bytes and output bytes of the pair whose size byte is `sb` and whose control bits are `cc` (bit 1: first symbol is a
// literal, bit 0: second) (tsq_decode.cpp:66-88,174-224)
__device__ __forceinline__ void pair_lens(uint32_t sb, uint32_t cc, uint32_t ext, uint32_t& slen, uint32_t& olen)
{
    const uint32_t hi = sb >> 4, lo = sb & 15u;
    const uint32_t lit_hi = cc & 2u, lit_lo = cc & 1u;
    const uint32_t o_hi = (!lit_hi && ext && hi < 3u) ? (hi + 2u) << 4 : hi + 1u;
    const uint32_t o_lo = (!lit_lo && ext && lo < 3u) ? (lo + 2u) << 4 : lo + 1u;
    slen = 1u + (lit_hi ? hi + 1u : 2u) + (lit_lo ? lo + 1u : 2u);
    olen = o_hi + o_lo;
}

// A chunk's image: output bytes [op, op + len), composed in the ring from ring address `at` (the ring address of position op).
// Image index i = (position - op) + lead, where lead = bytes of the ring word that holds position op which belong to the chunk
// before: index 0 is the 4-byte aligned ring address a0, lane t owns indices [12 t, 12 t + 12) = three aligned ring words.
struct Image {
    uint32_t op, len, at;
    __device__ __forceinline__ uint32_t lead() const { return at & 3u; }
    __device__ __forceinline__ uint32_t a0() const { return at & ~3u; }
};

// ---------------- P0
// 16-byte word `tid` of the chunk that starts at stream offset `at` (`av` stream bytes from there).  (Unaligned 16-byte global loads: the stream
// buffer in LDS then starts exactly at the chunk, and every LDS access to it is naturally aligned.)  Only whole words are loaded
// here, with no control flow behind the load, so that nothing waits for it before the chunk is staged; the last, partial word of a
// stream is fetched byte by byte in stage_words.
__device__ __forceinline__ uint4 prefetch_words(const uint8_t* in, uint32_t at, uint32_t av)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    const uint32_t lim = av < C::S + C::SPAD ? av : C::S + C::SPAD;
    uint4 w = make_uint4(0, 0, 0, 0);
    if (tid < C::SWORDS && (tid << 4) + 16u <= lim) __builtin_memcpy(&w, in + at + (tid << 4), 16);
    return w;
}
// the words prefetched into `pre` go to the stream buffer: sbuf[k] = in[at + k]; zeros beyond the stream
template <class L>
__device__ __forceinline__ void stage_words(uint8_t* lds, const uint8_t* in, uint32_t at, uint32_t av, uint4 pre)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    if (tid < C::SWORDS) {
        uint4 w = pre;
        const uint32_t lim = av < C::S + C::SPAD ? av : C::S + C::SPAD, o = tid << 4;
        if (o < lim && o + 16u > lim) {                                       // the stream's last, partial word (once per block)
            uint32_t b[4] = {0, 0, 0, 0};
            for (uint32_t k = 0; o + k < lim; ++k) b[k >> 2] |= (uint32_t)in[at + o + k] << (8u * (k & 3u));
            w = make_uint4(b[0], b[1], b[2], b[3]);
        }
        *reinterpret_cast<uint4*>(lds + L::sbuf + (tid << 4)) = w;
    }
}

// ---------------- P1: speculative group parse at every offset.  Lane t owns offsets t, t + T, ...: the lanes of a wavefront touch
// consecutive bytes, so neither their own entries nor the entries they point to (about one group further on, again consecutive)
// collide in the LDS banks.  x[k] is left at the next group's offset from offset tid + k T for P2 (TERM at or beyond slim).
template <class L>
__device__ __forceinline__ void parse_groups(uint8_t* lds, uint32_t slim, uint32_t (&x)[SymCfg::PER])
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const sbuf = lds + L::sbuf;
    uint32_t y[C::PER], c[C::PER];
    // (A) every byte of the chunk taken as a size byte: the stream length of the pair it would head, for each of the four
    //     control-bit pairs, packed in one word: 5 | 4 + lo << 8 | 4 + hi << 16 | 3 + hi + lo << 24 (tsq_decode.cpp:66-88: a
    //     literal takes nibble + 1 bytes, a match two).  One lane per aligned word of the chunk, arithmetic only.  The table
    //     lies over the doubling tables (dead until P2).
    {
        uint32_t* const pl = reinterpret_cast<uint32_t*>(lds + L::j4);
        constexpr uint32_t NW = (C::S + C::SPAD) / 4u;
#pragma unroll
        for (uint32_t k = 0; k < (NW + C::T - 1u) / C::T; ++k) {
            const uint32_t w = tid + k * C::T;
            if (w < NW) {
                const uint32_t v = reinterpret_cast<const uint32_t*>(sbuf)[w];
                uint32_t q[4];
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint32_t hi = (v >> (8u * b + 4u)) & 15u, lo = (v >> (8u * b)) & 15u;
                    q[b] = 0x03040405u + (lo << 8) + (hi << 16) + ((lo + hi) << 24);
                }
                *reinterpret_cast<uint4*>(pl + 4u * w) = make_uint4(q[0], q[1], q[2], q[3]);
            }
        }
    }
    __syncthreads();
    // (B) the four pairs of the group that would start at each offset: one table word per pair
    {
        const uint32_t* const pl = reinterpret_cast<const uint32_t*>(lds + L::j4);
#pragma unroll
        for (uint32_t k = 0; k < C::PER; ++k) { const uint32_t o = tid + k * C::T; c[k] = (uint32_t)sbuf[o] << 3; x[k] = o + 1u; }
#pragma unroll
        for (uint32_t pr = 0; pr < 4; ++pr) {
#pragma unroll
            for (uint32_t k = 0; k < C::PER; ++k) y[k] = pl[x[k]];                     // x < S + 133: inside the padded buffer
#pragma unroll
            for (uint32_t k = 0; k < C::PER; ++k) x[k] += __builtin_amdgcn_ubfe(y[k], (c[k] >> (6u - 2u * pr)) & 0x18u, 8u);
        }
    }
    uint8_t* const j1 = lds + L::j1;
#pragma unroll
    for (uint32_t k = 0; k < C::PER; ++k) { const uint32_t o = tid + k * C::T; j1[o] = (uint8_t)(x[k] - o); x[k] = o < slim ? x[k] : C::TERM; }
    __syncthreads();
}

// ---------------- P2: next^2 .. next^16 of every offset.  A lane keeps its own entries in registers from pass to pass.  The
// entries S .. TERM of every table hold TERM ("the chain has left the chunk": a fixed point), so that a look-up needs no range test.
template <class L>
__device__ __forceinline__ void double_pointers(uint8_t* lds, uint32_t slim, uint32_t (&x)[SymCfg::PER])
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const j1 = lds + L::j1;
    uint16_t* const j2 = reinterpret_cast<uint16_t*>(lds + L::j2);
    uint16_t* const j4 = reinterpret_cast<uint16_t*>(lds + L::j4);
    uint16_t* const j8 = reinterpret_cast<uint16_t*>(lds + L::j8);
    uint16_t* const j16 = reinterpret_cast<uint16_t*>(lds + L::j16);
    uint32_t y[C::PER];
#pragma unroll
    for (uint32_t k = 0; k < C::PER; ++k) { const uint32_t a = x[k] < slim ? x[k] : 0u; y[k] = a + j1[a]; }
#pragma unroll
    for (uint32_t k = 0; k < C::PER; ++k) { x[k] = x[k] < slim ? y[k] : C::TERM; j2[tid + k * C::T] = (uint16_t)x[k]; }
    if (tid <= C::SPAD) { j2[C::S + tid] = (uint16_t)C::TERM; j4[C::S + tid] = (uint16_t)C::TERM; j8[C::S + tid] = (uint16_t)C::TERM; j16[C::S + tid] = (uint16_t)C::TERM; }
    __syncthreads();
    const uint16_t* src = j2;
    uint16_t* const dsts[3] = {j4, j8, j16};
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d) {
#pragma unroll
        for (uint32_t k = 0; k < C::PER; ++k) y[k] = src[x[k]];                       // x <= TERM, and src[TERM] == TERM
#pragma unroll
        for (uint32_t k = 0; k < C::PER; ++k) { x[k] = y[k]; dsts[d][tid + k * C::T] = (uint16_t)x[k]; }
        __syncthreads();
        src = dsts[d];
    }
}

// ---------------- P3: the first wavefront follows next^16 from the chunk's first group at `first`; returns the number of super
// nodes.  (The whole wavefront walks, every lane the same chain: no lane mask to set up and restore; two hops per loop test -- the
// table's tail is a fixed point, so the second look-up is safe wherever the first one lands.)
template <class L>
__device__ __forceinline__ uint32_t walk_chain(uint8_t* lds, uint32_t first, uint32_t slim)
{
    using C = SymCfg;
    const uint16_t* const j16 = reinterpret_cast<const uint16_t*>(lds + L::j16);
    uint16_t* const sn = reinterpret_cast<uint16_t*>(lds + L::sn);
    uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + L::misc);
    if (threadIdx.x < 64u) {
        uint32_t x = first, k = 0;
        while (x < slim && k < C::MAXSN) {
            const uint32_t x1 = j16[x];
            const uint32_t x2 = j16[x1];                                        // x1 <= TERM, and j16[TERM] == TERM
            sn[k++] = (uint16_t)x;
            if (x1 < slim && k < C::MAXSN) { sn[k++] = (uint16_t)x1; x = x2; }
            else x = x1;
        }
        if (threadIdx.x == 0) { misc[0] = k; if (k >= C::MAXSN && x < slim) misc[4] = kErrStream; }
    }
    __syncthreads();
    return misc[0];
}

// ---------------- P4: one lane per group.  Group 16 k + r starts where r's bits lead from super node k.  The chunk's output
// starts at position op; the closing barrier is the caller's.
template <class L>
__device__ __forceinline__ void group_lanes(uint8_t* lds, uint32_t nsn, uint32_t slim, uint32_t op, uint32_t size, uint32_t ext)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint8_t* const sbuf = lds + L::sbuf;
    const uint8_t* const j1 = lds + L::j1;
    const uint16_t* const j2 = reinterpret_cast<const uint16_t*>(lds + L::j2);
    const uint16_t* const j4 = reinterpret_cast<const uint16_t*>(lds + L::j4);
    const uint16_t* const j8 = reinterpret_cast<const uint16_t*>(lds + L::j8);
    const uint16_t* const sn = reinterpret_cast<const uint16_t*>(lds + L::sn);
    uint16_t* const gstart = reinterpret_cast<uint16_t*>(lds + L::gstart);
    uint16_t* const glen = reinterpret_cast<uint16_t*>(lds + L::glen);
    uint32_t* const gout = reinterpret_cast<uint32_t*>(lds + L::gout);
    uint32_t* const pairs = reinterpret_cast<uint32_t*>(lds + L::pairs);
    uint32_t* const wsum = reinterpret_cast<uint32_t*>(lds + L::wsum);
    uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + L::misc);
    uint32_t x = C::TERM;
    if (tid < nsn * C::HOP) {
        x = sn[tid >> 4];
        if (tid & 8u) x = j8[x];
        if (tid & 4u) x = j4[x];
        if (tid & 2u) x = j2[x];
        if (tid & 1u) x = x < slim ? (uint32_t)(x + j1[x]) : C::TERM;
    }
    uint32_t v = 0;
    if (x < slim) {
        gstart[tid] = (uint16_t)x;
        const uint32_t c = sbuf[x];
        uint32_t p = x + 1u, pw[4];
#pragma unroll
        for (uint32_t pr = 0; pr < 4; ++pr) {
            const uint32_t cc = (c >> (6u - 2u * pr)) & 3u;
            pw[pr] = p | (v << 13) | (cc << 30);                  // p < 2^13, v < 2^14 (the image budget)
            uint32_t sl, ol;
            pair_lens(sbuf[p], cc, ext, sl, ol);
            p += sl;
            v += ol;
        }
        *reinterpret_cast<uint4*>(pairs + tid * 4u) = make_uint4(pw[0], pw[1], pw[2], pw[3]);
        glen[tid] = (uint16_t)v;
        if (p >= slim) { misc[1] = tid + 1u; misc[5] = p; }       // the chunk's last group: the chain leaves the chunk here
    }
    const uint32_t incl = wave_scan_add(v);
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    // output bytes of the wavefronts before this one: lane w takes wavefront w's total, one more scan, one readlane
    const uint32_t totals = wave_scan_add(lane < C::T / 64u ? wsum[lane] : 0u);
    const uint32_t before = wid ? (uint32_t)__builtin_amdgcn_readlane((int)totals, (int)wid - 1) : 0u;
    const uint32_t excl = before + incl - v;
    if (x < slim) {
        gout[tid] = op + excl;
        if (excl + 512u + 16u > C::OUTC) atomicMin(&misc[2], tid);
        if (op + excl + v >= size) atomicMin(&misc[3], tid);
    }
}

// ---------------- where the chunk ends, from P4's results (read after the barrier that closes P4)
struct ChunkEnd {
    uint32_t ng;          // groups in the chunk
    uint32_t next_at;     // stream offset of the next chunk's first group, from this chunk's start (0 after the block's last chunk)
    uint32_t next_op;     // output position of the next chunk
    bool last;            // the chunk completes the block
    bool cut;             // the LDS image budget cut the chunk short
};
template <class L>
__device__ __forceinline__ ChunkEnd chunk_end(const uint8_t* lds, uint32_t op, uint32_t size)
{
    const uint16_t* const gstart = reinterpret_cast<const uint16_t*>(lds + L::gstart);
    const uint16_t* const glen = reinterpret_cast<const uint16_t*>(lds + L::glen);
    const uint32_t* const gout = reinterpret_cast<const uint32_t*>(lds + L::gout);
    const uint32_t* const misc = reinterpret_cast<const uint32_t*>(lds + L::misc);
    const uint32_t ng = misc[1], cut = misc[2], fin = misc[3];
    if (fin != 0xFFFFFFFFu && fin < cut) return {fin + 1u, 0u, size, true, false};
    if (cut != 0xFFFFFFFFu) return {cut, gstart[cut], gout[cut], false, true};
    return {ng, misc[5], ng ? gout[ng - 1] + glen[ng - 1] : op, false, false};
}

// ---------------- P5 (a): records.  A record word lies at the first byte index of every run of bytes that come from one place:
// 0x40000000 | pointer flag << 31 | 24-bit signed D.
//   flag 0: the byte at index i is found at LDS address i + D (stream buffer for literals, ring for history);
//   flag 1: the byte at index i is a copy of the byte at index i + D of this same chunk (D < 0).
// A literal is one run; a match is up to three (history before the ring's end, history after it, bytes of this chunk).
// The record words are cleared first, by clear_records, under a barrier of the caller's.
template <class L>
__device__ __forceinline__ void clear_records(uint8_t* lds)
{
    uint32_t* const recw = reinterpret_cast<uint32_t*>(lds + L::recw);
    for (uint32_t w = threadIdx.x; w < (SymCfg::OUTC + 16) / 4; w += SymCfg::T) *reinterpret_cast<uint4*>(recw + 4u * w) = make_uint4(0, 0, 0, 0);
}
// One lane per PAIR of the chunk's ng groups: pair_at(rep, gi) gives the pair word (stream position | output offset in the group
// << 13 | control bits << 30) of pair gi = tid + rep T and the output position of its group.  Every pair's two symbols are decoded,
// validated against the chunk's `avail` stream bytes and the block's `size`, and their records dropped; a malformed pair sets misc[4].
template <class L, class PairAt>
__device__ __forceinline__ void drop_records(uint8_t* lds, uint32_t ng, const Image& im, uint32_t size, uint32_t avail, uint32_t ext,
                                             PairAt pair_at)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const sbuf = lds + L::sbuf;
    uint32_t* const recw = reinterpret_cast<uint32_t*>(lds + L::recw);
    const uint32_t op = im.op, lead = im.lead(), a0 = im.a0();
    if (tid == 0 && lead) recw[0] = 0x40000000u | (L::ring + a0);             // the bytes in front of position op in the first word: kept
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t rep = 0; rep < 2; ++rep) {
        const uint32_t gi = tid + rep * C::T;
        if (gi >= ng * 4u) break;
        const uint2 pg = pair_at(rep, gi);
        const uint32_t pw = pg.x;
        uint32_t p = pw & 0x1FFFu, j = pg.y + ((pw >> 13) & 0x3FFFu);
        const uint32_t origin = j;
        uint32_t sb = 0;
        if (j < size) { if (p >= avail) bad = 1; sb = sbuf[p]; p++; }
#pragma unroll
        for (uint32_t sidx = 0; sidx < 2; ++sidx) {
            if (j < size && !bad) {
                const uint32_t nib = sidx == 0 ? sb >> 4 : sb & 15u;
                const uint32_t lit = (pw >> (31u - sidx)) & 1u;
                const uint32_t room = size - j;
                const uint32_t ij = j - op + lead;
                if (lit) {
                    const uint32_t len = nib + 1u, take = len < room ? len : room;
                    if (p + take > avail) bad = 1;
                    else recw[ij] = 0x40000000u | ((L::sbuf + p - ij) & 0xFFFFFFu);
                    p += len; j += take;
                } else {
                    if (p + 2u > avail) bad = 1;
                    const uint32_t off = (uint32_t)sbuf[p] | ((uint32_t)sbuf[p + 1] << 8);
                    p += 2;
                    const uint32_t len = ext ? nibble_span(nib) : nib + 1u;       // (tsq_decode.cpp:174-224)
                    const uint32_t take = len < room ? len : room;
                    if (off > origin || take > off) bad = 1;
                    if (!bad) {
                        const uint32_t a = origin - off;                          // source position
                        const uint32_t n_hist = a >= op ? 0u : (op - a < take ? op - a : take);
                        if (n_hist) {
                            uint32_t x0 = a0 + C::R - ((op - a) - lead);            // ring address of the first source byte (index a - op + lead < lead)
                            x0 -= x0 >= C::R ? C::R : 0u;
                            recw[ij] = 0x40000000u | ((L::ring + x0 - ij) & 0xFFFFFFu);
                            if (x0 + n_hist > C::R) { const uint32_t n1 = C::R - x0; recw[ij + n1] = 0x40000000u | ((L::ring - (ij + n1)) & 0xFFFFFFu); }
                        }
                        if (n_hist < take) recw[ij + n_hist] = 0xC0000000u | ((a - j) & 0xFFFFFFu);   // source index - own index < 0
                    }
                    j += take;
                }
            }
        }
    }
    if (bad) reinterpret_cast<uint32_t*>(lds + L::misc)[4] = kErrStream;
}

typedef __attribute__((address_space(3))) uint16_t lds_u16;

// ---------------- P5 (b) + (c), after the barrier behind (a).  (b) one lane per 12 bytes: every byte takes the record of the symbol
// it lies in (the last record at or before it).  (c) every byte whose record names an LDS address is fetched at once (literal bytes,
// history bytes, the bytes kept in the first word); every byte whose source lies in this chunk points at it and goes onto the
// wavefront's waiting list.  Entry per byte: 0x8000 | value when final, else the index of the source byte.  Returns the length of
// the wavefront's waiting list (wavefront-uniform); the closing barrier is the caller's.
template <class L>
__device__ __forceinline__ uint32_t fetch_bytes(uint8_t* lds, const Image& im)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t* const recw = reinterpret_cast<const uint32_t*>(lds + L::recw);
    uint32_t* const wsum = reinterpret_cast<uint32_t*>(lds + L::wsum);
    lds_u16* const wl = (lds_u16*)(lds + L::plist) + 768u * wid;                 // this wavefront's waiting list
    const uint32_t own = 12u * tid;
    uint32_t r[12];
    {
        const uint4 q0 = *reinterpret_cast<const uint4*>(recw + own), q1 = *reinterpret_cast<const uint4*>(recw + own + 4u),
                    q2 = *reinterpret_cast<const uint4*>(recw + own + 8u);
        r[0] = q0.x; r[1] = q0.y; r[2] = q0.z; r[3] = q0.w; r[4] = q1.x; r[5] = q1.y; r[6] = q1.z; r[7] = q1.w; r[8] = q2.x; r[9] = q2.y; r[10] = q2.z; r[11] = q2.w;
#pragma unroll
        for (uint32_t k = 1; k < 12; ++k) r[k] = r[k] ? r[k] : r[k - 1];
        // the last record of the lanes before this one: a scan with "the later non-zero word wins" over the lanes' last records
        // (six DPP steps on the record itself; round 5 scanned a lane number and fetched the record with two ds_bpermute: two
        // LDS round trips per chunk on every wavefront)
        const uint32_t upto = wave_scan_last(r[11]);                                                            // inclusive
        uint32_t carry = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)upto, 0x138, 0xF, 0xF, false);           // wave_shr:1 : the lanes strictly before
        if (lane == 63) wsum[wid] = upto;
        __syncthreads();                                                       // (also: every lane has taken its records out of `recw`)
        {   // the last record of the wavefronts before this one: lane w looks at wavefront w's, the highest one that has any wins
            const uint32_t ws = lane < 16u ? wsum[lane] : 0u;
            const uint64_t m = __ballot(ws != 0u && lane < wid);
            const uint32_t prev = m ? (uint32_t)__builtin_amdgcn_readlane((int)ws, 63 - __builtin_clzll(m)) : 0u;
            carry = carry ? carry : prev;
        }
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) r[k] = r[k] ? r[k] : carry;
    }
    uint32_t pend = 0;
    if (own < im.lead() + im.len) {
        uint32_t v[12], by[12];
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) {
            v[k] = own + k + (uint32_t)((int32_t)(r[k] << 8) >> 8);               // LDS address of the byte, or index of its source
            pend |= (r[k] >> 31) << k;
        }
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) by[k] = lds[(r[k] >> 31) ? 0u : v[k]];
#pragma unroll
        for (uint32_t k = 0; k < 12; ++k) v[k] = (r[k] >> 31) ? v[k] : (0x8000u | by[k]);
#pragma unroll
        for (uint32_t w = 0; w < 3; ++w)
            *reinterpret_cast<uint2*>(lds + L::ent + 2u * own + 8u * w) = make_uint2(v[4 * w] | (v[4 * w + 1] << 16), v[4 * w + 2] | (v[4 * w + 3] << 16));
    }
    const uint32_t cnt = (uint32_t)__builtin_popcount(pend);
    const uint32_t incl = wave_scan_add(cnt);
    const uint32_t n_wait = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    uint32_t at = incl - cnt;
#pragma unroll
    for (uint32_t k = 0; k < 12; ++k) {
        if ((pend >> k) & 1u) wl[at] = (uint16_t)(own + k);
        at += (pend >> k) & 1u;
    }
    return n_wait;
}

// ---------------- P5 (d): asynchronous pointer jumping, no barriers, one lane per waiting byte: it reads its source's entry; a final
// entry carries the value, any other entry is a pointer further back (entries only ever move towards the chain's root, so a stale
// read is still a valid ancestor).  Chains of any depth (every occurrence of a frequent word copies the one before it; runs of a
// short period) shrink geometrically.  Relaxed LDS atomics: plain ds_read / ds_write that the compiler neither caches nor
// serialises.  Returns the loop's iterations (instrumented builds count them).
template <class L>
__device__ __forceinline__ uint32_t jump_pointers(uint8_t* lds, uint32_t n_wait)
{
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    lds_u16* const le = (lds_u16*)(lds + L::ent);
    lds_u16* const wl = (lds_u16*)(lds + L::plist) + 768u * wid;
    // The list is padded to whole passes of 64 with a spare entry of this wavefront (final from the start: a lane that sits on it
    // re-writes what it read), and the loop is compiled for the number of passes so that it is straight-line code: all reads of an
    // iteration in flight together, no branches.
    // (Round 6 tried two ways of evening out the wavefronts' lists -- the last wavefronts hold 340 waiting bytes per chunk, the
    //  first 54, the ones beyond the image's end none: tools/phase_stats.py --: the image's rows of sixteen lanes dealt round the
    //  wavefronts DOUBLES the loop's iterations, 4.74 ms against 4.49; ONE list for the workgroup cut into sixteen equal stretches
    //  takes 900 cycles per chunk off this phase and puts 1 350 onto the one before it (a barrier and a prefix over the
    //  wavefronts' counts in front of the list's stores), 4.52 against 4.46.)
    const uint32_t spare = SymCfg::OUTC + wid;
    if (lane == 0) le[spare] = 0x8000u;
    const uint32_t passes = (n_wait + 63u) >> 6;
    const uint32_t padded = passes <= 2u ? 2u : passes <= 4u ? 4u : passes <= 6u ? 6u : passes <= 8u ? 8u : 12u;
    if (passes) for (uint32_t it = n_wait + lane; it < padded * 64u; it += 64u) wl[it] = (uint16_t)spare;
    uint32_t iters = 0;
    auto jump = [&](auto passes_c) {
        constexpr uint32_t P = decltype(passes_c)::value;
        uint32_t q[P], ptr[P];
#pragma unroll
        for (uint32_t ps = 0; ps < P; ++ps) q[ps] = wl[ps * 64u + lane];
#pragma unroll
        for (uint32_t ps = 0; ps < P; ++ps) ptr[ps] = __hip_atomic_load(&le[q[ps]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        for (;;) {
            uint32_t e[P], open = 0;
#pragma unroll
            for (uint32_t ps = 0; ps < P; ++ps) e[ps] = __hip_atomic_load(&le[(ptr[ps] & 0x8000u) ? q[ps] : ptr[ps]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
            for (uint32_t ps = 0; ps < P; ++ps) {
                __hip_atomic_store(&le[q[ps]], (uint16_t)e[ps], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                ptr[ps] = e[ps];
                open |= (e[ps] & 0x8000u) ^ 0x8000u;
            }
            iters++;
            if (__ballot(open != 0u) == 0ull) break;
        }
    };
    if (passes == 0u) {}
    else if (passes <= 2u) jump(std::integral_constant<uint32_t, 2>{});
    else if (passes <= 4u) jump(std::integral_constant<uint32_t, 4>{});
    else if (passes <= 6u) jump(std::integral_constant<uint32_t, 6>{});
    else if (passes <= 8u) jump(std::integral_constant<uint32_t, 8>{});
    else jump(std::integral_constant<uint32_t, 12>{});
    return iters;
}

// ---------------- P5 (e), after the barrier behind (d): every entry is final now; three aligned ring words per lane
template <class L>
__device__ __forceinline__ void write_ring(uint8_t* lds, const Image& im)
{
    using C = SymCfg;
    const uint32_t own = 12u * threadIdx.x;
    if (own >= im.lead() + im.len) return;
    const uint2 e0 = *reinterpret_cast<const uint2*>(lds + L::ent + 2u * own), e1 = *reinterpret_cast<const uint2*>(lds + L::ent + 2u * own + 8u),
                e2 = *reinterpret_cast<const uint2*>(lds + L::ent + 2u * own + 16u);
    const uint32_t ev[6] = {e0.x, e0.y, e1.x, e1.y, e2.x, e2.y};
#pragma unroll
    for (uint32_t w = 0; w < 3; ++w) {
        uint32_t x = im.a0() + own + 4u * w; x -= x >= C::R ? C::R : 0u;
        const uint32_t lo = ev[2 * w], hi = ev[2 * w + 1];
        *reinterpret_cast<uint32_t*>(lds + L::ring + x) = (lo & 0xFFu) | ((lo >> 8) & 0xFF00u) | ((hi & 0xFFu) << 16) | ((hi >> 16) << 24);
    }
}

// ---------------- P7: the image's bytes from the ring to HBM (out is the block's output): head bytes up to the first aligned
// word, aligned 16-byte words, tail bytes.  Threads first_tid .. first_tid + n_threads - 1 take part.
template <class L>
__device__ __forceinline__ void flush_image(const uint8_t* lds, uint8_t* out, const Image& im, uint32_t first_tid, uint32_t n_threads)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const ring = lds + L::ring;
    if (im.len == 0 || tid < first_tid) return;
    const uint32_t t = tid - first_tid;
    const uint32_t head = (16u - (im.at & 15u)) & 15u;
    const uint32_t hb = head < im.len ? head : im.len;
    if (t < hb) out[im.op + t] = ring[im.at + t];                              // (the ring end is a multiple of 16: no wrap inside the head)
    const uint32_t words = (im.len - hb) >> 4;
    uint32_t ra = im.at + hb; ra -= ra >= C::R ? C::R : 0u;
    for (uint32_t w = t; w < words; w += n_threads) {
        uint32_t a = ra + (w << 4); a -= a >= C::R ? C::R : 0u;
        *reinterpret_cast<uint4*>(out + im.op + hb + (w << 4)) = *reinterpret_cast<const uint4*>(ring + a);
    }
    const uint32_t tail_at = hb + (words << 4);
    if (t < im.len - tail_at) { uint32_t a = ra + (words << 4) + t; a -= a >= C::R ? C::R : 0u; out[im.op + tail_at + t] = ring[a]; }
}

// ---------------- P7 of a range read: only the image's bytes in the window [lo, hi) of the block are written, byte p to out[p - lo].
// out - lo is the block's virtual base (oskew is taken from it), so the clipped image keeps its ring words on HBM words: aligned
// 16-byte stores in the middle, single bytes at the edges (flush_image on the clipped image).
template <class L>
__device__ __forceinline__ void flush_window(const uint8_t* lds, uint8_t* out, const Image& im, uint32_t lo, uint32_t hi, uint32_t first_tid,
                                             uint32_t n_threads)
{
    using C = SymCfg;
    const uint32_t a = im.op > lo ? im.op : lo, b = im.op + im.len < hi ? im.op + im.len : hi;
    if (a >= b) return;
    uint32_t at = im.at + (a - im.op); at -= at >= C::R ? C::R : 0u;
    flush_image<L>(lds, out, Image{a - lo, b - a, at}, first_tid, n_threads);
}

// ---------------- P7 of a record scan (dec_mark_kernel): no byte of the image goes to HBM.  Its bytes are compared with `delim`, and
// one BIT per byte goes to a bit map that the caller has cleared: bit G & 63 of 64-bit word (G >> 6) + blk stands for position G
// of the concatenation, G = base + p for byte p of block blk (base: the block's out_at).  The block's words are its own: the next
// block's first word, ((base + len) >> 6) + blk + 1, lies above this block's last, ((base + len - 1) >> 6) + blk.  The ring's skew
// is base & 63, so the image is walked as flush_image walks it, by the aligned 16-byte ring words it touches, and ring word and
// 16-bit cell of the map coincide; the ring's size is a multiple of 16, so no cell wraps.  A lane masks its word's bytes outside
// the image (the first and last cell are shared with the neighbouring images, whose lanes bring the other bits) and ORs the mask
// into the 32-bit half that holds the cell -- only where a bit is set, which in text is one cell in four.  A cell at or past
// map_words (a descriptor that lies about its place) is not written.  No barrier inside.
template <class L>
__device__ __forceinline__ void flush_mark(const uint8_t* lds, uint32_t* map32, uint64_t map_words, uint64_t base, uint32_t blk, const Image& im,
                                           uint32_t delim, uint32_t first_tid, uint32_t n_threads)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const ring = lds + L::ring;
    if (im.len == 0 || tid < first_tid) return;
    const uint32_t skew = im.at & 15u, cells = (skew + im.len + 15u) >> 4;
    const uint32_t c0 = im.at & ~15u;
    const uint64_t g0 = (base + im.op) & ~15ull;                                // position of the first cell's byte 0 (base + op = at mod 16)
    const uint32_t splat = delim * 0x01010101u;
    for (uint32_t w = tid - first_tid; w < cells; w += n_threads) {
        uint32_t a = c0 + (w << 4); a -= a >= C::R ? C::R : 0u;
        const uint4 x = *reinterpret_cast<const uint4*>(ring + a);
        const uint32_t v[4] = {x.x ^ splat, x.y ^ splat, x.z ^ splat, x.w ^ splat};
        uint32_t m = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            // bit 7 of every byte of v[i] that is zero, exactly (no borrow runs from byte to byte), then the four bits side by side
            const uint32_t z = ~(((v[i] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v[i] | 0x7F7F7F7Fu);
            m |= ((((z >> 7) * 0x00204081u) >> 21) & 0xFu) << (4u * i);
        }
        const uint32_t lo = w == 0u ? skew : 0u, left = skew + im.len - (w << 4), hi = left < 16u ? left : 16u;   // the image's bytes [lo, hi) of the cell
        m &= (0xFFFFu << lo) & (0xFFFFu >> (16u - hi));
        const uint64_t g = g0 + ((uint64_t)w << 4), word = (g >> 6) + blk;
        if (m != 0u && word < map_words) atomicOr(map32 + 2u * word + ((uint32_t)(g >> 5) & 1u), m << ((uint32_t)g & 16u));
    }
}

// ---------------- P7 of a find (dec_find_kernel): flush_mark with a needle of m bytes, 1 <= m <= 16, in place of one byte.  The
// needle travels in two 64-bit words (byte k of the needle is byte k of lo, k < 8, of hi behind that).  The map's layout, the
// ring's skew and the walk by aligned 16-byte cells are flush_mark's; bit G stands for a hit that ENDS at position G of the
// concatenation.  A hit that ends in a cell starts in it or in the cell in front, so a lane reads that one too (with the ring's
// wrap): the bytes in front of the image are earlier images of the same block, which the ring keeps (64 KiB of history, and
// write_ring of the next chunk comes behind this flush).  Ends at block positions p < m - 1 would start in front of the block:
// they are left to the seam launch (tsq_find.cuh), which has the neighbouring blocks' edges.
// The comparison: the equality mask of the needle's LAST byte over the cell is the filter -- in text most cells end here --, and
// only a cell that passes it takes the other bytes' masks over the 32-byte window, each shifted to the hit's end and ANDed, until
// nothing is left.
// Edge bytes: edges[32 blk + j], j < 15, is byte j of the block, and edges[32 blk + 16 + j] is byte size - 15 + j (the last 15
// bytes, right-aligned; positions in front of the block are not written).  Each flush writes those that lie in its image.
// No barrier inside.
struct FindNeedle { uint64_t lo, hi; uint32_t m; };

__device__ __forceinline__ uint32_t find_needle_byte(const FindNeedle& nd, uint32_t k)
{
    return (uint32_t)((k < 8u ? nd.lo >> (8u * k) : nd.hi >> (8u * (k - 8u))) & 0xFFull);
}

// bit j: byte j of the cell equals the byte that `splat` repeats (flush_mark's zero-byte test)
__device__ __forceinline__ uint32_t find_cell_mask(const uint4& x, uint32_t splat)
{
    const uint32_t v[4] = {x.x ^ splat, x.y ^ splat, x.z ^ splat, x.w ^ splat};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t z = ~(((v[i] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v[i] | 0x7F7F7F7Fu);
        m |= ((((z >> 7) * 0x00204081u) >> 21) & 0xFu) << (4u * i);
    }
    return m;
}

template <class L>
__device__ __forceinline__ void flush_find(const uint8_t* lds, uint32_t* map32, uint64_t map_words, uint64_t base, uint32_t blk, const Image& im,
                                           const FindNeedle& nd, uint32_t size, uint8_t* edges, uint32_t first_tid, uint32_t n_threads)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const ring = lds + L::ring;
    if (im.len == 0 || tid < first_tid) return;
    const uint32_t t = tid - first_tid;
    if (t < 31u && t != 15u) {                               // the block's edges: lanes 0..14 its head, 16..30 its tail
        const uint32_t j = t & 15u;
        uint32_t p = 0xFFFFFFFFu;
        if (t < 15u) { if (j < size) p = j; }
        else if (size + j >= 15u) p = size + j - 15u;
        if (p != 0xFFFFFFFFu && p >= im.op && p - im.op < im.len) {
            uint32_t a = im.at + (p - im.op); a -= a >= C::R ? C::R : 0u;
            edges[((size_t)blk << 5) + t] = ring[a];
        }
    }
    const uint32_t skew = im.at & 15u, cells = (skew + im.len + 15u) >> 4;
    const uint32_t c0 = im.at & ~15u;
    const uint64_t g0 = (base + im.op) & ~15ull;
    const uint32_t m = nd.m;
    const uint32_t last = find_needle_byte(nd, m - 1u) * 0x01010101u;
    for (uint32_t w = t; w < cells; w += n_threads) {
        uint32_t a = c0 + (w << 4); a -= a >= C::R ? C::R : 0u;
        const uint4 x = *reinterpret_cast<const uint4*>(ring + a);
        uint32_t ends = find_cell_mask(x, last);
        // the image's bytes [lo, hi) of the cell, less the ends in front of block position m - 1: byte j of the cell is block
        // position op + 16 w + j - skew
        uint32_t lo = w == 0u ? skew : 0u;
        const uint32_t left = skew + im.len - (w << 4), hi = left < 16u ? left : 16u;
        const int32_t from = (int32_t)(m - 1u + skew) - (int32_t)(im.op + (w << 4));
        if (from > (int32_t)lo) lo = from < 16 ? (uint32_t)from : 16u;
        ends &= ((0xFFFFu << lo) & 0xFFFFu) & (0xFFFFu >> (16u - hi));
        if (ends != 0u && m > 1u) {
            const uint32_t b = a == 0u ? C::R - 16u : a - 16u;                // the cell in front (the ring's size is a multiple of 16)
            const uint4 y = *reinterpret_cast<const uint4*>(ring + b);
            uint32_t acc = ends << 16;                                        // bits 16..31: this cell, 0..15: the one in front
            for (uint32_t k = m - 1u; k-- > 0u && acc != 0u; ) {
                const uint32_t splat = find_needle_byte(nd, k) * 0x01010101u;
                const uint32_t eq = find_cell_mask(y, splat) | (find_cell_mask(x, splat) << 16);
                acc &= eq << (m - 1u - k);                                    // needle byte k lies m - 1 - k in front of the end
            }
            ends = acc >> 16;
        }
        const uint64_t g = g0 + ((uint64_t)w << 4), word = (g >> 6) + blk;
        if (ends != 0u && word < map_words) atomicOr(map32 + 2u * word + ((uint32_t)(g >> 5) & 1u), ends << ((uint32_t)g & 16u));
    }
}

// ---------------- P7 of a CRC (dec_crc_kernel): no byte of the image goes anywhere.  The image is walked as flush_mark walks it, by
// the aligned 16-byte ring cells it touches (c0, skew, cells, the wrap at C::R, the bytes outside [lo, hi) of the first and last
// cell masked to zero), and what leaves is ONE word per image, XORed into *word (LDS, zero before the flush):
//     W = xor over the cells w of  R(cell w, masked) (x) x^(128 (cells - 1 - w))
// which is R(image | z zero bytes), z = the bytes between the image's last byte and the END of its last cell.  Every exponent is
// thus a whole number of cells, and one table of x^(128 k) serves the cells and the block's running fold alike; the partial last
// cell costs nothing here -- the zeros behind the block's last byte are taken off once per block, with x^(-8 z) (crc_block_fold).
// Zeros in FRONT of a cell's bytes do not count at all, which is why the first cell's mask is enough.
// A cell's R: four rounds of four look-ups in slice[4][256] (tsq_crc32.h), the register XORed with the next four bytes in
// between.  Its shift: one 32-step product (crc_mul, tsq_crc32.h) with pow[cells - 1 - w].  Both tables are in LDS at `tab` (slice, then pow).
// The lanes' words are XORed across the wavefront by shuffles, and one lane of each wavefront that had a cell sends one LDS
// atomic XOR.  No barrier inside.
template <class L>
__device__ __forceinline__ void flush_crc(const uint8_t* lds, const uint32_t* tab, uint32_t* word, const Image& im, uint32_t first_tid,
                                          uint32_t n_threads)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    const uint8_t* const ring = lds + L::ring;
    if (im.len == 0 || tid < first_tid) return;
    const uint32_t skew = im.at & 15u, cells = (skew + im.len + 15u) >> 4;
    const uint32_t c0 = im.at & ~15u;
    if (((tid - first_tid) & ~63u) >= cells) return;                            // (a whole wavefront with no cell)
    const uint32_t* const pow = tab + 1024;
    uint32_t acc = 0;
    for (uint32_t w = tid - first_tid; w < cells; w += n_threads) {
        uint32_t a = c0 + (w << 4); a -= a >= C::R ? C::R : 0u;
        const uint4 x = *reinterpret_cast<const uint4*>(ring + a);
        const uint32_t lo = w == 0u ? skew : 0u, left = skew + im.len - (w << 4), hi = left < 16u ? left : 16u;   // the image's bytes [lo, hi) of the cell
        const uint32_t keep = (0xFFFFu << lo) & (0xFFFFu >> (16u - hi));
        const uint32_t v[4] = {x.x, x.y, x.z, x.w};
        uint32_t c = 0;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            // the four bits of `keep` that belong to this word, one to a byte, then whole bytes
            const uint32_t bytes = ((((keep >> (4u * i)) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu;
            c ^= v[i] & bytes;
            c = tab[768u + (c & 0xFFu)] ^ tab[512u + ((c >> 8) & 0xFFu)] ^ tab[256u + ((c >> 16) & 0xFFu)] ^ tab[c >> 24];
        }
        acc ^= crc_mul(c, pow[cells - 1u - w]);
    }
#pragma unroll
    for (uint32_t d = 32u; d != 0u; d >>= 1) acc ^= (uint32_t)__shfl_xor((int)acc, (int)d);
    if ((tid & 63u) == 0u && acc != 0u) atomicXor(word, acc);
}

// One image joins the block's running word: A is R(the block's bytes so far | the zeros up to the end of the last cell touched).
// The image's first cell is the last image's last cell when it starts inside one (skew != 0), so the grid moves on by cells - 1
// cells then, by `cells` otherwise.
__device__ __forceinline__ uint32_t crc_image_fold(uint32_t acc, const uint32_t* tab, const Image& im, uint32_t word)
{
    const uint32_t skew = im.at & 15u, cells = (skew + im.len + 15u) >> 4;
    const uint32_t moved = cells - (skew != 0u && cells != 0u ? 1u : 0u);
    return crc_mul(acc, tab[1024u + moved]) ^ word;
}

}  // namespace tsq
