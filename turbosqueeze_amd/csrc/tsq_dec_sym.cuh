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

// The decoder of one block on one workgroup.  kWindow = false (dec_sym_kernel): block blockIdx.x, whole.  kWindow = true
// (dec_range_kernel): item blockIdx.x -- only the bytes [lo, hi) of its block are written, and the chunk loop ends with the chunk
// that reaches hi.  Every chunk that is decoded is validated as in the whole-block decode.  (The pointers carry no __restrict__ here:
// the kernels' own parameters do, and restrict parameters of an inlined function would give dec_sym_kernel other code than before.)
template <bool kWindow>
__device__ __forceinline__ void sym_decode_block(const uint8_t* container, const FrameInfo* frames, uint32_t n_frames, const RangeItem* items,
                                                 uint8_t* outbuf, int32_t* status)
{
    using C = SymCfg;
    using L = SymLds;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t* const gout = reinterpret_cast<const uint32_t*>(lds + L::gout);
    const uint32_t* const pairs = reinterpret_cast<const uint32_t*>(lds + L::pairs);
    uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + L::misc);
    // misc[0..5]: tsq_dec_common.cuh; [9], [10] instrumented builds only

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
    const FrameInfo f = frames[blk];
    // The descriptor may come straight from an untrusted container (tsqa_decode_blocks_async): a stream shorter than its 3-byte
    // header, longer than a block slot, or an output longer than a block is refused before anything is read through it.
    if (f.stream_len < 3u || f.stream_len > kSlotSize || f.out_len > kBlockSize || (kWindow && (lo >= hi || hi > f.out_len))) {
        if (tid == 0) atomicMax(status, kErrStream);
        return;
    }
    const uint8_t* const in = container + f.stream_at;
    // window: `out` is where byte lo goes; byte p of the block goes to out + (p - lo)
    uint8_t* const out = outbuf + (kWindow ? out_at : f.out_at);
    const uint32_t in_len = f.stream_len, size = f.out_len, ext = f.ext;
    // ring address of output position p: (p + oskew) mod R, so that 16-byte words of the ring are 16-byte words of HBM (window: of
    // the block's virtual base out - lo)
    const uint32_t oskew = (uint32_t)(((uintptr_t)out - lo) & 15u);

#ifdef TSQ_STATS
    const uint32_t lane = tid & 63u, wid = tid >> 6;
    unsigned long long st_[16] = {0};
    unsigned long long wj_[3] = {0, 0, 0};
#endif
    TSQD_T0();
    if (tid == 0) { misc[4] = 0; misc[9] = 0; misc[10] = 0; }
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
            if constexpr (kWindow) flush_window<L>(lds, out, prev, lo, hi, C::T / 2, C::T / 2);
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
        // (window: the chunk that reaches hi is the last one decoded)
        const bool more = !e.last && !(kWindow && e.next_op >= hi);
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
        prev = im;
        ring_op += im.len; ring_op -= ring_op >= C::R ? C::R : 0u;
        op = e.next_op;
        sp = next_sp;
        TSQD_ACC(8);
        if (!more) break;
    }
    __syncthreads();
    if constexpr (kWindow) flush_window<L>(lds, out, prev, lo, hi, 0, C::T);
    else flush_image<L>(lds, out, prev, 0, C::T);
#ifdef TSQ_STATS
    if (blockIdx.x == 0 && tid == 0) for (int q = 0; q < 16; ++q) g_dec_stats[q] = st_[q];
    if (blockIdx.x == 0 && lane == 0) for (int q = 0; q < 3; ++q) g_dec_wave[wid * 3 + q] = wj_[q];
#endif
}

__global__ __launch_bounds__(1024) void dec_sym_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames,
                                                       uint8_t* __restrict__ outbuf, int32_t* __restrict__ status)
{
    sym_decode_block<false>(container, frames, 0u, nullptr, outbuf, status);
}

// Range reads (tsqa_decompress_ranges_async): one workgroup per item; nothing outside [out_at, out_at + hi - lo) of `outbuf` is written.
__global__ __launch_bounds__(1024) void dec_range_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames, uint32_t n_frames,
                                                         const RangeItem* __restrict__ items, uint8_t* __restrict__ outbuf, int32_t* __restrict__ status)
{
    sym_decode_block<true>(container, frames, n_frames, items, outbuf, status);
}

}  // namespace tsq
