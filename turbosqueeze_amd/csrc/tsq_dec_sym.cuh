// tsq_dec_sym.cuh -- block decoder on one workgroup per block (kernel variant 0): the chunk phases of tsq_dec_common.cuh one after
// the other, with the next chunk staged beside the pointer jumping and the previous chunk's bytes written out beside P4.
#pragma once

#include "tsq_common.cuh"
#include "tsq_dec_common.cuh"

namespace tsq {

struct SymLds {
    static constexpr uint32_t sbuf = 0;                                             // u8[S + SPAD + 16]
    static constexpr uint32_t j1 = sbuf + 16 * SymCfg::SWORDS;                      // u8[S]: next - offset
    // u16[JN] each: next^2 .. next^16 of every offset; the entries S .. TERM hold TERM ("the chain has left the chunk": a fixed
    // point), so that a look-up needs no range test
    static constexpr uint32_t JN = (SymCfg::S + SymCfg::SPAD + 8u) & ~7u;
    static constexpr uint32_t j2 = j1 + SymCfg::S;
    static constexpr uint32_t j4 = j2 + 2 * JN;
    static constexpr uint32_t j8 = j4 + 2 * JN;
    static constexpr uint32_t j16 = j8 + 2 * JN;
    static constexpr uint32_t recw = j1;                                            // P5: u32[OUTC + 16] symbol records by first byte index, over j1 .. j16
    static constexpr uint32_t ent = j1;                                             // P5: u16[OUTC + 16] byte entries (once the records are read)
    static constexpr uint32_t plist = ent + 2 * (SymCfg::OUTC + 16);                // P5: u16[OUTC] per wavefront, the bytes that wait for a source
    static constexpr uint32_t gstart = j16 + 2 * JN;                                // u16[MAXG]
    static constexpr uint32_t glen = gstart + 2 * SymCfg::MAXG;                     // u16[MAXG]
    static constexpr uint32_t gout = glen + 2 * SymCfg::MAXG;                       // u32[MAXG]
    static constexpr uint32_t pairs = gout + 4 * SymCfg::MAXG;                      // u32[4 * MAXG]: stream pos | out offset << 13 | 2 control bits << 30
    static constexpr uint32_t sn = pairs + 16 * SymCfg::MAXG;                       // u16[MAXSN + pad]
    static constexpr uint32_t wsum = (sn + 2 * ((SymCfg::MAXSN + 7) & ~7u) + 15) & ~15u;   // u32[16]
    static constexpr uint32_t misc = wsum + 64;                                     // u32[16]
    static constexpr uint32_t ring = (misc + 64 + 15) & ~15u;                       // u8[R + RPAD]
    static constexpr uint32_t total = ring + SymCfg::R + SymCfg::RPAD;               // (the product asks for nothing it does not use)
    static_assert(recw % 16 == 0 && recw + 4 * (SymCfg::OUTC + 16) <= gstart && plist % 16 == 0 && plist + 2 * SymCfg::OUTC <= gstart,
                  "records, byte entries and waiting lists fit the dead doubling tables");
};
static_assert(SymLds::total <= 160 * 1024, "LDS budget");

// One item of a range read (tsqa_range_item): output bytes [lo, hi) of block `block` go to out + out_at (byte lo lands there).
struct RangeItem {
    uint32_t block, lo, hi, pad;
    uint64_t out_at;
};

// One decode of a record read (tsqa_block_group): block `block` is decoded once, up to its byte `hi`, for the items
// [first, first + count) of the item array, which are sorted by lo.
struct BlockGroup {
    uint32_t block, first, count, hi;
};

enum DecMode : int { kDecWhole, kDecWindow, kDecGroup, kDecMark, kDecFind, kDecCrc };

// LDS of dec_crc_kernel behind the decoder's own: the CRC tables of flush_crc (slice[4][256], then pow[kCrcCells + 1]: tsq_crc32.h)
// and the two words into which the images' flushes XOR, by turns.  The other kernels ask for SymLds::total as before.
struct CrcLds {
    static constexpr uint32_t tab = (SymLds::total + 15u) & ~15u;                  // u32[kCrcLdsWords]
    static constexpr uint32_t word = tab + 4u * ((kCrcLdsWords + 3u) & ~3u);        // u32[2]
    static constexpr uint32_t total = word + 16u;
};
static_assert(CrcLds::total <= 160 * 1024, "LDS budget");
static_assert(kCrcCells >= ((15u + SymCfg::OUTC + 15u) >> 4) + 1u, "a power for every cell count of an image");

// ---------------- P7 of a record read: the image's bytes go to every item of the group that they meet (byte p of the block to
// out[it.out_at + p - it.lo]).  The items are sorted by lo, so those that meet the image are a run of the list that only moves
// forward: the cursor `gc.cur` (one per wavefront, it advances lazily) is the first item that an image at or behind this one can still meet, and
// the run ends with the first item that starts behind the image.  The items stay in HBM / L2; every wavefront reads the run 64
// items at a time, one per lane.
//
// The work is dealt by destination bytes, not by items: each item's stretch is cut into the 16-byte words of HBM that it touches,
// the words of a batch are numbered across its items (a prefix sum over the lanes), and pass j of the numbering -- 64 words, one
// per lane -- belongs to wavefront j mod n.  A 12 KiB stretch of one long window and two hundred records of 64 bytes both keep
// every lane of every wavefront busy.  The destinations have unrelated alignments, so no skew of the ring serves them: a lane
// reads the two ALIGNED 16-byte ring words that hold its sixteen source bytes (an unaligned ds access costs 3.5x an aligned one,
// tools/micro/lds_unaligned.hip), shifts them into place in registers and stores one aligned 16-byte word; the words at a stretch's
// edges (all of a short record) go as aligned dwords where a dword is whole and as single bytes where it is not.  Nothing outside
// [a, b) of an item is written.  Threads first_tid .. first_tid + n_threads - 1 take part (whole wavefronts); no barrier inside.
//
// Most chunks of a record read meet no item, and a long window meets the same item for hundreds of chunks: the cursor keeps the
// lo of its item (no image that ends at or before it has anything to write: no memory is touched) and the batch of 64 items it
// last read around the cursor (read again only when the cursor has left it).
struct GroupCursor {
    uint32_t cur = 0, cur_lo = 0;           // the first item that is still needed, and its lo (0: not known yet)
    uint32_t held = 0xFFFFFFFFu;            // `it` holds item held + lane (held: a multiple of 64)
    RangeItem it = {0u, 0u, 0u, 0u, 0ull};
};

template <class L>
__device__ __forceinline__ void flush_group(const uint8_t* lds, uint8_t* out, const Image& im, const RangeItem* items, uint32_t count, GroupCursor& gc,
                                            uint32_t first_tid, uint32_t n_threads)
{
    using C = SymCfg;
    const uint32_t tid = threadIdx.x;
    if (im.len == 0 || tid < first_tid || gc.cur >= count || gc.cur_lo >= im.op + im.len) return;
    uint32_t& cur = gc.cur;
    const uint8_t* const ring = lds + L::ring;
    const uint32_t lane = tid & 63u, w = (tid - first_tid) >> 6, nw = n_threads >> 6;
    const uint32_t im_end = im.op + im.len;
    uint32_t pass0 = 0;                     // passes of the batches before this one
    bool leading = true;                    // no item that is still needed has been seen yet: the cursor moves
    // The batches lie on a grid of 64 items from the group's first, whatever the cursor: every wavefront that takes part numbers
    // the words alike even where its cursor lags behind the others' (the items in front of the true cursor give no word).
    for (uint32_t base = cur & ~63u; base < count; base += 64u) {
        const uint32_t k = base + lane;
        RangeItem it = {0u, 0xFFFFFFFFu, 0u, 0u, 0ull};                           // behind the list: an item that starts behind every image
        if (base == gc.held) it = gc.it;
        else if (k < count) it = items[k];
        const bool in_run = it.lo < im_end;
        if (leading) {
            gc.held = base; gc.it = it;                                           // (the batch at the cursor's place, or the one it moves into)
            const uint64_t done = __ballot(k < count && it.hi <= im.op);         // behind this image and every later one
            const uint32_t n = ~done == 0ull ? 64u : (uint32_t)__builtin_ctzll(~done);
            cur = base + n;                                                       // (the lanes in front of the old cursor are done, too)
            leading = n == 64u;
            // the cursor's item is lane n of this batch (behind the list: no item, and cur >= count ends every later call at once)
            if (!leading) gc.cur_lo = (uint32_t)__builtin_amdgcn_readlane((int)it.lo, (int)n);
        }
        const uint32_t a = it.lo > im.op ? it.lo : im.op, b = it.hi < im_end ? it.hi : im_end;
        const bool live = in_run && a < b;
        const uint32_t len = live ? b - a : 0u;
        const uint64_t addr = (uint64_t)(uintptr_t)out + it.out_at + (a - it.lo);  // where byte a goes
        const uint32_t nwords = live ? (((uint32_t)addr & 15u) + len + 15u) >> 4 : 0u;
        uint32_t ra = im.at + (a - im.op); ra -= ra >= C::R ? C::R : 0u;          // ring address of byte a
        uint32_t incl = nwords;                                                   // inclusive prefix over the lanes
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t passes = (total + 63u) >> 6;
        const uint32_t packed = len | (ra << 14);                                 // len <= OUTC < 2^14, ra < R < 2^17
        for (uint32_t j = (w + nw - pass0 % nw) % nw; j < passes; j += nw) {
            const uint32_t q = (j << 6) + lane;
            // the word's item: the first lane whose inclusive count exceeds q (= the number of lanes whose count does not)
            uint32_t t = 0;
#pragma unroll
            for (uint32_t step = 32u; step != 0u; step >>= 1) {
                const uint32_t v = __shfl(incl, (int)(t + step - 1u));
                t += v <= q ? step : 0u;
            }
            const bool act = q < total;
            const int src = (int)(t & 63u);
            const uint32_t excl_s = __shfl(incl - nwords, src), alo = __shfl((uint32_t)addr, src), ahi = __shfl((uint32_t)(addr >> 32), src),
                           pk = __shfl(packed, src);
            if (act) {      // (the shuffles above are the whole wavefront's; what follows is each lane's own)
                const uint32_t kk = q - excl_s, slen = pk & 0x3FFFu, sra = pk >> 14, s = alo & 15u;
                uint8_t* const word = reinterpret_cast<uint8_t*>((uintptr_t)((((uint64_t)ahi << 32) | alo) & ~15ull)) + ((size_t)kk << 4);
                // bytes [e0, e1) of the word belong to the stretch; the word's byte 0 is the stretch's byte i0
                const int32_t i0 = (int32_t)(kk << 4) - (int32_t)s;
                const uint32_t e0 = kk == 0u ? s : 0u;
                const uint32_t left = (uint32_t)((int32_t)slen - i0), e1 = left < 16u ? left : 16u;
                int32_t r = (int32_t)sra + i0;
                r += r < 0 ? (int32_t)C::R : 0; r -= r >= (int32_t)C::R ? (int32_t)C::R : 0;
                const uint32_t r0 = (uint32_t)r & ~15u;
                uint32_t r1 = r0 + 16u; r1 -= r1 >= C::R ? C::R : 0u;                  // (the ring's size is a multiple of 16)
                const uint4 x = *reinterpret_cast<const uint4*>(ring + r0), y = *reinterpret_cast<const uint4*>(ring + r1);
                const uint32_t v8[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
                const uint32_t dsh = ((uint32_t)r >> 2) & 3u, bsh = ((uint32_t)r & 3u) << 3;
                uint32_t u[5], o[4];
#pragma unroll
                for (uint32_t i = 0; i < 5u; ++i) u[i] = dsh == 0u ? v8[i] : dsh == 1u ? v8[i + 1] : dsh == 2u ? v8[i + 2] : v8[i + 3];
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) o[i] = (uint32_t)((((uint64_t)u[i + 1] << 32) | u[i]) >> bsh);
                if (e0 == 0u && e1 == 16u) {
                    *reinterpret_cast<uint4*>(word) = make_uint4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 4u; ++i) {
                        if (e0 <= 4u * i && 4u * i + 4u <= e1) {
                            *reinterpret_cast<uint32_t*>(word + 4u * i) = o[i];
                        } else {
#pragma unroll
                            for (uint32_t c = 0; c < 4u; ++c)
                                if (4u * i + c >= e0 && 4u * i + c < e1) word[4u * i + c] = (uint8_t)(o[i] >> (8u * c));
                        }
                    }
                }
            }
        }
        pass0 += passes;
        if (__ballot(!in_run) != 0ull) break;                                     // the run ends in this batch
    }
}

// The decoder of one block on one workgroup.  kDecWhole (dec_sym_kernel): block blockIdx.x, whole.  kDecWindow
// (dec_range_kernel): item blockIdx.x -- only the bytes [lo, hi) of its block are written, and the chunk loop ends with the chunk
// that reaches hi.  kDecGroup (dec_group_kernel): group blockIdx.x -- its block is decoded up to the group's hi, and every chunk's
// bytes go to each of the group's items that they meet (flush_group).  Every chunk that is decoded is validated as in the
// whole-block decode.  kDecMark (dec_mark_kernel): block blockIdx.x, whole, and nothing of it is written: `outbuf` is the bit map of
// flush_mark, map_words long, and every chunk's image is compared with `delim` there.  Every use of that mode sits behind
// `if constexpr`, so the other three are compiled as they were.  kDecFind (dec_find_kernel): kDecMark with a needle of up to 16
// bytes in place of the delimiter (flush_find), and the block's first and last 15 bytes left in `edges`; it sits behind
// `if constexpr` in the same places.  kDecCrc (dec_crc_kernel): like kDecMark no byte is written; every image leaves one word
// (flush_crc), which one thread folds into the block's running word A = A (x) x^(128 cells moved) xor W, and `outbuf` is a table
// of one u32 per block that takes R(block) at the end.  The fold of an image is made one chunk late, by the first thread of the
// upper half in front of its next flush: the barrier that closes a P4 lies behind that P4's flush, so the word is complete then,
// and the images' words take turns so that the flush under way XORs into the other one.  The last image is flushed by all lanes
// behind the loop and ONE barrier, the only one this mode adds, stands between that flush and its fold.  It too sits behind
// `if constexpr`.  (The pointers carry no __restrict__ here: the kernels' own parameters do, and restrict parameters of an
// inlined function would give dec_sym_kernel other code than before.)
template <DecMode kMode>
__device__ __forceinline__ void sym_decode_block(const uint8_t* container, const FrameInfo* frames, uint32_t n_frames, const RangeItem* items,
                                                 uint8_t* outbuf, int32_t* status, const BlockGroup* groups = nullptr, uint32_t n_items = 0u,
                                                 [[maybe_unused]] uint32_t delim = 0u, [[maybe_unused]] uint64_t map_words = 0ull,
                                                 [[maybe_unused]] FindNeedle needle = {0ull, 0ull, 0u}, [[maybe_unused]] uint8_t* edges = nullptr)
{
    constexpr bool kWindow = kMode == kDecWindow, kGroup = kMode == kDecGroup, kMark = kMode == kDecMark, kFind = kMode == kDecFind;
    constexpr bool kCrc = kMode == kDecCrc;
    using C = SymCfg;
    using L = SymLds;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t* const gout = reinterpret_cast<const uint32_t*>(lds + L::gout);
    const uint32_t* const pairs = reinterpret_cast<const uint32_t*>(lds + L::pairs);
    uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + L::misc);
    // misc[0..5]: tsq_dec_common.cuh; [9], [10] instrumented builds only; [12] group: the upper wavefronts' cursor, for the last write-out

    const uint32_t tid = threadIdx.x;
    // Another block may have reported an error: leave, but all together (thread 0 reads the word, the workgroup branches on its copy
    // in LDS -- a per-thread read could split the workgroup while other blocks are still writing the word).
    if (tid == 0) misc[11] = (uint32_t)*status;
    __syncthreads();
    if (misc[11] != 0u) return;
    // window: the item's block and its bytes [lo, hi); the whole block otherwise
    uint32_t blk = blockIdx.x, lo = 0, hi = 0;
    uint64_t out_at = 0;
    if constexpr (kWindow) {
        const RangeItem it = items[blockIdx.x];
        if (it.block >= n_frames) {
            if (tid == 0) atomicMax(status, kErrStream);
            return;
        }
        blk = it.block; lo = it.lo; hi = it.hi; out_at = it.out_at;
    }
    // group: the items it serves, and how far each wavefront has come in them (flush_group)
    [[maybe_unused]] const RangeItem* gitems = nullptr;
    [[maybe_unused]] uint32_t gcount = 0;
    [[maybe_unused]] GroupCursor gcur;
    if constexpr (kGroup) {
        const BlockGroup g = groups[blockIdx.x];
        if (g.block >= n_frames || g.count == 0u || g.first > n_items || g.count > n_items - g.first) {
            if (tid == 0) atomicMax(status, kErrStream);
            return;
        }
        blk = g.block; hi = g.hi; gitems = items + g.first; gcount = g.count;
    }
    const FrameInfo f = frames[blk];
    // The descriptor may come straight from an untrusted container (tsqa_decode_blocks_async): a stream shorter than its 3-byte
    // header, longer than a block slot, or an output longer than a block is refused before anything is read through it.
    if (f.stream_len < 3u || f.stream_len > kSlotSize || f.out_len > kBlockSize || ((kWindow || kGroup) && (lo >= hi || hi > f.out_len))) {
        if (tid == 0) atomicMax(status, kErrStream);
        return;
    }
    const uint8_t* const in = container + f.stream_at;
    // window: `out` is where byte lo goes; byte p of the block goes to out + (p - lo)
    // (group: every item has a destination of its own in outbuf; no skew of the ring can serve them all)
    // (mark: outbuf is the bit map, and no byte of the block has a destination)
    // (crc: outbuf is the blocks' table of words)
    uint8_t* const out = kGroup || kMark || kFind || kCrc ? outbuf : outbuf + (kWindow ? out_at : f.out_at);
    const uint32_t in_len = f.stream_len, size = f.out_len, ext = f.ext;
    // ring address of output position p: (p + oskew) mod R, so that 16-byte words of the ring are 16-byte words of HBM (window: of
    // the block's virtual base out - lo)
    // (mark: the 64-position grid of the concatenation falls on the ring's 64-byte grid, flush_mark)
    // (crc: no grid outside the block matters; the block starts on a cell)
    const uint32_t oskew = kCrc ? 0u : kMark || kFind ? (uint32_t)(f.out_at & 63u) : kGroup ? 0u : (uint32_t)(((uintptr_t)out - lo) & 15u);

#ifdef TSQ_STATS
    const uint32_t lane = tid & 63u, wid = tid >> 6;
    unsigned long long st_[16] = {0};
    unsigned long long wj_[3] = {0, 0, 0};
#endif
    TSQD_T0();
    if (tid == 0) { misc[4] = 0; misc[9] = 0; misc[10] = 0; }
    // crc: the tables come to LDS and the images' two words are cleared, under the barrier below; what the fold carries: the
    // running word, the images made so far and the image in front of `prev`, whose word is still to be folded
    [[maybe_unused]] const uint32_t* const ctab = reinterpret_cast<const uint32_t*>(lds + CrcLds::tab);
    [[maybe_unused]] uint32_t* const cword = reinterpret_cast<uint32_t*>(lds + CrcLds::word);
    [[maybe_unused]] uint32_t crc_acc = 0, n_img = 0;
    [[maybe_unused]] Image prev2 = {0, 0, 0};
    if constexpr (kCrc) {
        const uint32_t* const src = reinterpret_cast<const uint32_t*>(&g_crc_tables);
        for (uint32_t k = tid; k < kCrcLdsWords; k += C::T) reinterpret_cast<uint32_t*>(lds + CrcLds::tab)[k] = src[k];
        if (tid < 2u) cword[tid] = 0u;
    }
    uint32_t sp = 3, op = 0;
    uint32_t ring_op = oskew;            // ring address of position op
    Image prev = {0, 0, 0};              // what P7 still has to write out: the previous chunk's image
    uint4 pre = prefetch_words(in, sp, in_len - sp);
    bool staged_ahead = false;
    __syncthreads();

    while (op < size) {
        const uint32_t avail = in_len - sp;
        const uint32_t slim = avail < C::S ? avail : C::S;
        // ---------------- P0: the chunk goes to LDS.  (Only the block's first chunk is staged here: every later one goes to LDS
        // during the chunk before it, behind its byte fetch, beside its pointer jumping.)
        if (!staged_ahead) stage_words<L>(lds, in, sp, avail, pre);
        if (tid == 0) { misc[0] = 0; misc[1] = 0; misc[2] = 0xFFFFFFFFu; misc[3] = 0xFFFFFFFFu; misc[5] = 0; }
        // (this barrier also ends the previous chunk's ring write, which reads the byte entries the parse tables now overwrite)
        __syncthreads();
        TSQD_ACC(0); TSQD_CNT(12, 1);

        uint32_t x[C::PER];
        parse_groups<L>(lds, slim, x);                                                   // P1
        TSQD_ACC(1);
        double_pointers<L>(lds, slim, x);                                                // P2
        TSQD_ACC(2);
        const uint32_t nsn = walk_chain<L>(lds, 0u, slim);                                // P3
        TSQD_ACC(3);

        // ---------------- P4.  The upper half of the workgroup has no group to look after: it writes the PREVIOUS chunk's bytes to
        // HBM meanwhile (P7).  (measured in round 5: a build without this flush runs 4.558 against 4.553 ms, the flush beside P3's
        // chain instead 4.572 -- it hides completely)
        if (tid >= C::T / 2) {
            if constexpr (kCrc) {
                // image n_img - 2 joins the running word (its flush lies behind the last chunk's barriers), then image n_img - 1
                // is flushed into the other word
                if (tid == C::T / 2 && n_img >= 2u) { crc_acc = crc_image_fold(crc_acc, ctab, prev2, cword[n_img & 1u]); cword[n_img & 1u] = 0u; }
                flush_crc<L>(lds, ctab, cword + ((n_img + 1u) & 1u), prev, C::T / 2, C::T / 2);
            }
            else if constexpr (kFind) flush_find<L>(lds, reinterpret_cast<uint32_t*>(out), map_words, f.out_at, blk, prev, needle, size, edges, C::T / 2, C::T / 2);
            else if constexpr (kMark) flush_mark<L>(lds, reinterpret_cast<uint32_t*>(out), map_words, f.out_at, blk, prev, delim, C::T / 2, C::T / 2);
            else if constexpr (kGroup) flush_group<L>(lds, out, prev, gitems, gcount, gcur, C::T / 2, C::T / 2);
            else if constexpr (kWindow) flush_window<L>(lds, out, prev, lo, hi, C::T / 2, C::T / 2);
            else flush_image<L>(lds, out, prev, C::T / 2, C::T / 2);
        }
        group_lanes<L>(lds, nsn, slim, op, size, ext);
        // the doubling tables are dead from here on (every lane is past its last look-up in them): the record words of P5, which lie
        // over them, are cleared now, under the barrier that is needed anyway
        clear_records<L>(lds);
        __syncthreads();
        const ChunkEnd e = chunk_end<L>(lds, op, size);
        const uint32_t next_sp = sp + e.next_at;
        if (misc[4] != 0 || e.ng == 0 || (!e.last && next_sp >= in_len)) {
            if (tid == 0) atomicMax(status, kErrStream);
            return;
        }
        const Image im = {op, e.next_op - op, ring_op};
        // (window, group: the chunk that reaches hi is the last one decoded)
        const bool more = !e.last && !((kWindow || kGroup) && e.next_op >= hi);
        // the next chunk's stream is on its way while this one is copied
        if (more) pre = prefetch_words(in, next_sp, in_len - next_sp);
        TSQD_ACC(4);

        // ---------------- P5: symbols -> bytes
        drop_records<L>(lds, e.ng, im, size, avail, ext,                                   // (a)
                        [&](uint32_t, uint32_t gi) { return make_uint2(pairs[gi], gout[gi >> 2]); });
        __syncthreads();
        if (misc[4] != 0) { if (tid == 0) atomicMax(status, (int32_t)misc[4]); return; }
        TSQD_ACC(5);
        const uint32_t n_wait = fetch_bytes<L>(lds, im);                                  // (b) + (c)
        __syncthreads();
        TSQD_ACC(6);
        // the NEXT chunk's stream goes to LDS now (P0 of chunk k + 1): the byte fetch that the barrier above closed was the last reader
        // of the stream buffer (the literal bytes), and the words were requested behind P4, a dozen thousand cycles ago
        if (more) { stage_words<L>(lds, in, next_sp, in_len - next_sp, pre); staged_ahead = true; }
#ifdef TSQ_STATS
        const unsigned long long wj0_ = __builtin_amdgcn_s_memtime();
#endif
        [[maybe_unused]] const uint32_t iters = jump_pointers<L>(lds, n_wait);           // (d)
#ifdef TSQ_STATS
        if (lane == 0) { atomicMax(&misc[9], iters); atomicAdd(&misc[10], n_wait); }
        // per wavefront: when it left the pointer jumping (imbalance between the wavefronts shows as the barrier wait behind it)
        if (lane == 0 && blockIdx.x == 0) { wj_[0] += __builtin_amdgcn_s_memtime() - wj0_; wj_[1] += n_wait; wj_[2] += iters; }
#endif
        __syncthreads();
        write_ring<L>(lds, im);                                                           // (e)
        // (no barrier here: nothing reads the ring, and nothing overwrites the entries, before the barrier at the top of the next chunk)
        TSQD_ACC(7);
#ifdef TSQ_STATS
        if (tid == 0) { st_[14] += misc[9]; st_[11] += misc[10]; misc[9] = 0; misc[10] = 0; }
#endif

        // ---------------- the image is complete: it goes to HBM during the next chunk's P4 (or right now, after the last chunk)
        if constexpr (kCrc) { prev2 = prev; ++n_img; }
        prev = im;
        ring_op += im.len; ring_op -= ring_op >= C::R ? C::R : 0u;
        op = e.next_op;
        sp = next_sp;
        TSQD_ACC(8);
        if (!more) break;
    }
    // (group: the lower wavefronts have written nothing out so far; they take the cursor of the upper ones instead of walking the
    // item list from its start)
    if constexpr (kGroup) { if (tid == C::T / 2) misc[12] = gcur.cur; }
    __syncthreads();
    if constexpr (kGroup) { if (tid < C::T / 2) gcur.cur = misc[12]; }
    if constexpr (kCrc) {
        if (tid == C::T / 2 && n_img >= 2u) { crc_acc = crc_image_fold(crc_acc, ctab, prev2, cword[n_img & 1u]); cword[n_img & 1u] = 0u; }
        flush_crc<L>(lds, ctab, cword + ((n_img + 1u) & 1u), prev, 0, C::T);
        __syncthreads();                                     // (the one barrier of this mode: the last image's word is complete behind it)
        if (tid == C::T / 2) {
            crc_acc = crc_image_fold(crc_acc, ctab, prev, cword[(n_img + 1u) & 1u]);
            // the zeros between the block's last byte and the end of its last cell come off again: R(block)
            const uint32_t pad = (16u - ((prev.at + prev.len) & 15u)) & 15u;
            reinterpret_cast<uint32_t*>(out)[blk] = crc_mul(crc_acc, g_crc_tables.inv[pad]);
        }
    }
    else if constexpr (kFind) flush_find<L>(lds, reinterpret_cast<uint32_t*>(out), map_words, f.out_at, blk, prev, needle, size, edges, 0, C::T);
    else if constexpr (kMark) flush_mark<L>(lds, reinterpret_cast<uint32_t*>(out), map_words, f.out_at, blk, prev, delim, 0, C::T);
    else if constexpr (kGroup) flush_group<L>(lds, out, prev, gitems, gcount, gcur, 0, C::T);
    else if constexpr (kWindow) flush_window<L>(lds, out, prev, lo, hi, 0, C::T);
    else flush_image<L>(lds, out, prev, 0, C::T);
#ifdef TSQ_STATS
    if (blockIdx.x == 0 && tid == 0) for (int q = 0; q < 16; ++q) g_dec_stats[q] = st_[q];
    if (blockIdx.x == 0 && lane == 0) for (int q = 0; q < 3; ++q) g_dec_wave[wid * 3 + q] = wj_[q];
#endif
}

__global__ __launch_bounds__(1024) void dec_sym_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames,
                                                       uint8_t* __restrict__ outbuf, int32_t* __restrict__ status)
{
    sym_decode_block<kDecWhole>(container, frames, 0u, nullptr, outbuf, status);
}

// dec_sym_kernel with a status word per batch item (tsqa_decompress_batch_items_async): block blockIdx.x reads and reports into the
// word of the item that owns it (owner[]: batch_walk_kernel<kWalkPerItem>), so a fault ends that item's remaining blocks and nobody
// else's.  live_blocks != NULL: a batch whose block count is made on the device (tsqa_decompress_batch_packed_dense_async): the launch
// has as many workgroups as the caller has room for blocks, and those at or past *live_blocks (batch_layout_kernel) leave before
// they touch a descriptor or an owner.  NULL: every workgroup is live.
__global__ __launch_bounds__(1024) void dec_item_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames,
                                                        const uint32_t* __restrict__ owner, uint8_t* __restrict__ outbuf,
                                                        int32_t* __restrict__ item_status, const uint32_t* __restrict__ live_blocks)
{
    if (live_blocks && blockIdx.x >= *live_blocks) return;
    sym_decode_block<kDecWhole>(container, frames, 0u, nullptr, outbuf, item_status + owner[blockIdx.x]);
}

// Range reads (tsqa_decompress_ranges_async): one workgroup per item; nothing outside [out_at, out_at + hi - lo) of `outbuf` is written.
__global__ __launch_bounds__(1024) void dec_range_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames, uint32_t n_frames,
                                                         const RangeItem* __restrict__ items, uint8_t* __restrict__ outbuf, int32_t* __restrict__ status)
{
    sym_decode_block<kDecWindow>(container, frames, n_frames, items, outbuf, status);
}

// Record reads (tsqa_decompress_item_ranges_async): one workgroup per touched block, which serves all of the block's items;
// nothing outside the items' destinations is written.
__global__ __launch_bounds__(1024) void dec_group_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames, uint32_t n_frames,
                                                         const RangeItem* __restrict__ items, uint32_t n_items, const BlockGroup* __restrict__ groups,
                                                         uint8_t* __restrict__ outbuf, int32_t* __restrict__ status)
{
    sym_decode_block<kDecGroup>(container, frames, n_frames, items, outbuf, status, groups, n_items);
}

// The record scan (tsqa_records_async): one workgroup per block of the index, the block decoded whole and validated as in
// dec_sym_kernel, and nothing of it written: bit G of `map` (flush_mark's layout, map_words 64-bit words, cleared by the caller) is
// set where byte G of the index's data equals `delim`.  verdict (may be NULL): a sized index's word; where it is nonzero no
// descriptor is read.
__global__ __launch_bounds__(1024) void dec_mark_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames,
                                                        const int32_t* __restrict__ verdict, uint32_t delim, uint64_t* __restrict__ map,
                                                        uint64_t map_words, int32_t* __restrict__ status)
{
    if (verdict && *verdict != 0) return;
    sym_decode_block<kDecMark>(container, frames, 0u, nullptr, reinterpret_cast<uint8_t*>(map), status, nullptr, 0u, delim, map_words);
}

// The find (tsqa_find_async): dec_mark_kernel with a needle of m bytes (n0..n3: its bytes, little-endian, zeros behind m) in place
// of the delimiter.  Bit G of `map` is set where a hit ENDS at byte G of the index's data and starts inside the same block; the
// block's first and last 15 bytes go to edges + 32 * block for the seam launch (tsq_find.cuh).
__global__ __launch_bounds__(1024) void dec_find_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames,
                                                        const int32_t* __restrict__ verdict, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3,
                                                        uint32_t m, uint64_t* __restrict__ map, uint64_t map_words, uint8_t* __restrict__ edges,
                                                        int32_t* __restrict__ status)
{
    if (verdict && *verdict != 0) return;
    const FindNeedle needle = {((uint64_t)n1 << 32) | n0, ((uint64_t)n3 << 32) | n2, m};
    sym_decode_block<kDecFind>(container, frames, 0u, nullptr, reinterpret_cast<uint8_t*>(map), status, nullptr, 0u, 0u, map_words, needle, edges);
}

// The CRC (tsqa_crc32_async): one workgroup per block of the index, the block decoded whole and validated as in dec_sym_kernel, and
// nothing of it written but block_r[block] = R(block) (tsq_crc32.h), which crc_fold_kernel (tsq_crc.cuh) carries to the items.  The
// block's item is found here, by bisection in item_first (NULL: one item owns every block) as records_count_kernel finds it, and
// the decoder reads and raises THAT item's status word, as dec_item_kernel does: a malformed stream ends the rest of its item
// and nobody else's.  A workgroup that leaves with its item's word raised raises *any as well, for the call's status.
__global__ __launch_bounds__(1024) void dec_crc_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames,
                                                       const int32_t* __restrict__ verdict, const uint64_t* __restrict__ item_first,
                                                       uint32_t n_items, uint32_t* __restrict__ block_r, int32_t* __restrict__ item_status,
                                                       int32_t* __restrict__ any)
{
    if (verdict && *verdict != 0) return;
    uint32_t it = 0;
    if (item_first) {
        uint32_t lo = 0, hi = n_items;
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (item_first[mid] <= blockIdx.x) lo = mid; else hi = mid; }
        it = lo;
    }
    sym_decode_block<kDecCrc>(container, frames, 0u, nullptr, reinterpret_cast<uint8_t*>(block_r), item_status + it);
    if (threadIdx.x == 0u) {
        const int32_t st = __hip_atomic_load(item_status + it, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st != 0) atomicMax(any, st);
    }
}

}  // namespace tsq
