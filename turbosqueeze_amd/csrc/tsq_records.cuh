// tsq_records.cuh -- the record tables of an index from a delimiter byte (tsqa_records_async).  dec_mark_kernel (tsq_dec_sym.cuh)
// decodes every block and leaves one bit per byte in a map: bit G & 63 of word (G >> 6) + b for position G of the concatenation in
// block b, so no word belongs to two blocks.  What follows is a count, a scan and a placement over that map, in the cut's shape
// (tsq_cut.cuh): no workgroup waits for another.  The launches:
//   records_count_kernel   one workgroup per block: its delimiters, its last one, whether its last byte is one, its item
//   records_sum_kernel     (a) each group of 256 blocks: the record starts summed, the last boundary in front of each block
//   records_scan_kernel    (b) ONE workgroup: the groups' bases, 256 groups per pass; the need words, the count's status
//   records_place_kernel   (c) each block's first record number and the start of the record that is open where it begins
//   records_items_kernel   d_item_first_record
//   records_emit_kernel    one workgroup per block: every record that ENDS in the block, numbered, below cap_records
//   records_close_kernel   the call's status word
//
// The rule (turbosqueeze_amd.h) in the terms of a block.  A block HOLDS the record start behind each of its delimiters, less the
// one behind a delimiter at its item's last byte, and its item's start where the item's first byte lies in it.  The exclusive sum
// of that over the blocks numbers the records: block b's first held start is record base[b], and an item's first record is the
// base of its first block.  The delimiter of rank r in block b ends the record base[b] + first + r - 1 (first: the item's start
// lies in the block), which began behind the delimiter in front of it -- in the same block, or the last one of an earlier block, or
// at the item's start: `open`, an exclusive MAXIMUM over the blocks of "one past my last delimiter, or my item's start", since
// positions only grow.  So whoever holds a record's end knows its start, and writes the whole entry; the item's last record, which
// has no terminator, is written by the item's last block.  Nothing is read from the tables, and a record at or past cap_records
// is measured (d_need[1]) and not written.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"
#include "tsq_gather.cuh"

namespace tsq {

constexpr uint32_t kRecordsKeepDelim = 1u, kRecordsFlat = 2u;  // TSQA_RECORDS_KEEP_DELIM, TSQA_RECORDS_FLAT
constexpr uint32_t kRecordsGroup = 256;                      // blocks per workgroup of launches (a) and (c), groups per pass of launch (b)

// What the call keeps per block in the context's scratch.  starts: the record starts it holds, then (c) their first number.
// edge: on the way in where a record that is open behind the block started -- one past its last delimiter, or its item's start --
// kept one up so that 0 says "neither"; then (c) the start of the record that is open where the block begins.  item_at, item_end:
// its item's extent in the concatenation.  flags: 1 the item's first byte lies in the block, 2 its last byte does, 4 the block's
// last byte is a delimiter.
struct RecordBlock { uint64_t starts, edge, item_at, item_end; uint32_t item, flags; };

// The call's words in the context's scratch: the decoders' word (zero until one meets a malformed stream), and the count's verdict.
struct RecordWords { int32_t stream, worst; };

// Exclusive MAXIMUM of v over the 256 threads of a workgroup (0 in front of the first), *total = the workgroup's: the sibling of
// group_scan_excl64, with shuffles (nothing here is hot).  Every thread calls it.
__device__ __forceinline__ uint64_t group_max_excl64(uint64_t v, uint64_t* wave_max /* LDS, 4 */, uint64_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t up = __shfl_up(incl, d);
        if (lane >= d && up > incl) incl = up;
    }
    uint64_t excl = __shfl_up(incl, 1u);
    if (lane == 0u) excl = 0;
    __syncthreads();                                         // (the previous call's maxima have been read)
    if (lane == 63u) wave_max[wid] = incl;
    __syncthreads();
    uint64_t all = 0;
    for (uint32_t w = 0; w < 4u; ++w) { const uint64_t m = wave_max[w]; if (w < wid && m > excl) excl = m; if (m > all) all = m; }
    *total = all;
    return excl;
}

// The words of block b in the map: [w0, w1], none when the block is empty.  Clamped to the map (a descriptor is the index's, but
// no read or write here leaves the scratch whatever it says).
__device__ __forceinline__ bool records_words_of(const FrameInfo& f, uint32_t b, uint64_t map_words, uint64_t* w0, uint64_t* w1)
{
    if (f.out_len == 0u) return false;
    *w0 = (f.out_at >> 6) + b;
    *w1 = ((f.out_at + f.out_len - 1u) >> 6) + b;
    if (*w0 >= map_words) return false;
    if (*w1 >= map_words) *w1 = map_words - 1u;
    return true;
}

// One workgroup of 256 threads per block.  verdict nonzero: no descriptor is read and the block holds nothing.  The block's item is
// found by bisection in item_first (NULL: one item, which owns every block); the item's extent comes from the descriptors of its
// first block and of the block behind its last.
__global__ __launch_bounds__(256) void records_count_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint64_t total,
                                                            const int32_t* __restrict__ verdict, const uint64_t* __restrict__ item_first,
                                                            uint32_t n_items, const uint64_t* __restrict__ map, uint64_t map_words,
                                                            RecordBlock* __restrict__ blocks)
{
    __shared__ uint64_t wave_sum[4], wave_max[4];
    const uint32_t b = blockIdx.x;
    if (verdict && *verdict != 0) {
        if (threadIdx.x == 0u) blocks[b] = RecordBlock{0ull, 0ull, 0ull, 0ull, 0u, 0u};
        return;
    }
    const FrameInfo f = frames[b];
    uint64_t w0 = 0, w1 = 0;
    const bool any = records_words_of(f, b, map_words, &w0, &w1);
    uint64_t count = 0, last = 0;                            // this thread's delimiters, and one past its last one's position
    if (any)
        for (uint64_t w = w0 + threadIdx.x; w <= w1; w += 256u) {
            const uint64_t x = map[w];
            if (x != 0ull) { count += (uint32_t)__builtin_popcountll(x); last = ((w - b) << 6) + (64u - (uint32_t)__builtin_clzll(x)); }
        }
    uint64_t delims, edge;
    (void)group_scan_excl64(count, wave_sum, &delims);
    (void)group_max_excl64(last, wave_max, &edge);
    if (threadIdx.x != 0u) return;
    RecordBlock r{0ull, 0ull, 0ull, 0ull, 0u, 0u};
    if (any) {
        uint32_t it = 0;
        uint64_t fb = 0, fe = n_blocks;
        if (item_first) {                                    // the last item whose first block is at or before b (an item may own no blocks)
            uint32_t lo = 0, hi = n_items;
            while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (item_first[mid] <= b) lo = mid; else hi = mid; }
            it = lo; fb = item_first[it]; fe = item_first[it + 1u];
            if (fe > n_blocks) fe = n_blocks;
        }
        const uint64_t end = f.out_at + f.out_len;
        r.item = it;
        r.item_at = gather_block_start(frames, n_blocks, total, fb);
        r.item_end = gather_block_start(frames, n_blocks, total, fe);
        if (fb > b || fe <= b || r.item_at > f.out_at || r.item_end < end) { r.item_at = f.out_at; r.item_end = end; }   // (tables that disagree: the block alone)
        // (flags 1 and 2 fall on the item's first and last block WITH BYTES, whatever empty blocks it has: an empty block in front
        //  shares its out_at with the first block that has bytes, which therefore starts at item_at, and empty blocks behind start
        //  where the last one with bytes ends; empty blocks themselves hold nothing and carry no flag)
        const uint64_t lw = ((end - 1u) >> 6) + b;
        const bool last_is = lw < map_words && ((map[lw] >> ((end - 1u) & 63u)) & 1ull) != 0ull;
        r.flags = (f.out_at == r.item_at ? 1u : 0u) | (end == r.item_end ? 2u : 0u) | (last_is ? 4u : 0u);
        r.starts = delims + (r.flags & 1u) - ((r.flags & 6u) == 6u ? 1u : 0u);
        // (where the open record starts behind this block, kept one up so that 0 says "nothing here" and position 0 still counts)
        r.edge = edge != 0ull ? edge + 1u : (r.flags & 1u) ? r.item_at + 1u : 0ull;
    }
    blocks[b] = r;
}

// Launch (a).  Workgroup g of exactly 256 threads: group_sum[g] = the starts of the blocks [256 g, 256 g + 256), group_edge[g] the
// largest edge among them; each block keeps the starts and the largest edge of the group's blocks in front of it.
__global__ __launch_bounds__(256) void records_sum_kernel(RecordBlock* __restrict__ blocks, uint32_t n_blocks, uint64_t* __restrict__ group_sum,
                                                          uint64_t* __restrict__ group_edge)
{
    __shared__ uint64_t wave_sum[4], wave_max[4];
    const uint64_t b = (uint64_t)blockIdx.x * kRecordsGroup + threadIdx.x;
    const bool valid = b < n_blocks;
    uint64_t sum, edge;
    const uint64_t own = group_scan_excl64(valid ? blocks[b].starts : 0ull, wave_sum, &sum);
    const uint64_t open = group_max_excl64(valid ? blocks[b].edge : 0ull, wave_max, &edge);
    if (valid) { blocks[b].starts = own; blocks[b].edge = open; }
    if (threadIdx.x == 0u) { group_sum[blockIdx.x] = sum; group_edge[blockIdx.x] = edge; }
}

// Launch (b).  cut_scan_kernel's scan with a maximum beside the sum: ONE workgroup of exactly 256 threads.  need[0] = the records
// of all items, need[1] is zeroed for the emit's atomicMax, and the count's verdict goes to words->worst: kErrFormat behind a
// refused index, kErrOverflow when the records exceed cap_records.
__global__ __launch_bounds__(256) void records_scan_kernel(uint64_t* __restrict__ group_sum, uint64_t* __restrict__ group_edge, uint32_t n_groups,
                                                           const int32_t* __restrict__ verdict, uint64_t cap_records, uint64_t* __restrict__ need,
                                                           RecordWords* __restrict__ words)
{
    __shared__ uint64_t wave_sum[4], wave_max[4];
    uint64_t base = 0, open = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += kRecordsGroup) {   // (no thread leaves the loop early: the scans need them all)
        const uint32_t g = g0 + threadIdx.x;
        const bool valid = g < n_groups;
        uint64_t sum, edge;
        const uint64_t before = base + group_scan_excl64(valid ? group_sum[g] : 0ull, wave_sum, &sum);
        uint64_t in_front = group_max_excl64(valid ? group_edge[g] : 0ull, wave_max, &edge);
        if (open > in_front) in_front = open;
        base += sum;
        if (edge > open) open = edge;
        if (valid) { group_sum[g] = before; group_edge[g] = in_front; }
    }
    if (threadIdx.x == 0u) {
        need[0] = base; need[1] = 0ull;
        words->worst = verdict && *verdict != 0 ? kErrFormat : base > cap_records ? kErrOverflow : kOk;
    }
}

// Launch (c).  One lane per block: its first record number is the group's base and its own; the record open where it begins
// started at its item's start when that lies in the block, else behind the last delimiter in front of it.
__global__ __launch_bounds__(256) void records_place_kernel(RecordBlock* __restrict__ blocks, uint32_t n_blocks, const uint64_t* __restrict__ group_base,
                                                            const uint64_t* __restrict__ group_open)
{
    const uint64_t b = (uint64_t)blockIdx.x * kRecordsGroup + threadIdx.x;
    if (b >= n_blocks) return;
    RecordBlock r = blocks[b];
    r.starts += group_base[blockIdx.x];
    uint64_t open = r.edge > group_open[blockIdx.x] ? r.edge : group_open[blockIdx.x];      // one past the position, 0: none
    open = open != 0ull ? open - 1u : 0ull;
    if ((r.flags & 1u) || open < r.item_at) open = r.item_at;
    r.edge = open;
    blocks[b] = r;
}

// One lane per entry of d_item_first_record (n_items + 1): an item's first record is the first number of its first block; an item
// without blocks starts where the next one does, and the last entry is the count of all records.
__global__ __launch_bounds__(256) void records_items_kernel(const RecordBlock* __restrict__ blocks, uint32_t n_blocks, const uint64_t* __restrict__ item_first,
                                                            uint32_t n_items, const uint64_t* __restrict__ need, uint64_t* __restrict__ item_first_record)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i > n_items) return;
    const uint64_t fb = item_first ? item_first[i] : i == 0u ? 0ull : (uint64_t)n_blocks;
    item_first_record[i] = fb < n_blocks ? blocks[fb].starts : need[0];
}

// One workgroup of 256 threads per block, the block's words in passes of one per lane.  A prefix over the popcounts ranks the
// delimiters; an exclusive maximum over "one past my word's last delimiter" gives each word the delimiter in front of its first.
// Every delimiter writes the record it ends; thread 0 writes the item's last record where the block holds the item's last byte and
// that is no delimiter.  A record numbered at or past cap_records is measured and not written; rec_items may be NULL.
__global__ __launch_bounds__(256) void records_emit_kernel(const FrameInfo* __restrict__ frames, const int32_t* __restrict__ verdict,
                                                           const uint64_t* __restrict__ map, uint64_t map_words, const RecordBlock* __restrict__ blocks,
                                                           uint32_t flags, uint64_t cap_records, uint32_t* __restrict__ rec_items,
                                                           uint64_t* __restrict__ rec_offsets, uint64_t* __restrict__ rec_lengths,
                                                           uint64_t* __restrict__ need)
{
    __shared__ uint64_t wave_sum[4], wave_max[4];
    __shared__ unsigned long long longest;
    if (verdict && *verdict != 0) return;
    const uint32_t b = blockIdx.x;
    const FrameInfo f = frames[b];
    uint64_t w0 = 0, w1 = 0;
    if (!records_words_of(f, b, map_words, &w0, &w1)) return;
    if (threadIdx.x == 0u) longest = 0ull;
    const RecordBlock r = blocks[b];
    const uint64_t keep = flags & kRecordsKeepDelim ? 1u : 0u, origin = flags & kRecordsFlat ? 0ull : r.item_at;
    // the record that the block's delimiter of rank 0 ends
    const uint64_t first_no = r.starts + (r.flags & 1u) - 1u;   // (wraps for a block whose rank 0 does not exist: unused then)
    uint64_t rank0 = 0, open = r.edge, mine = 0;                 // delimiters in front of this pass; start of the open record; this thread's longest
    auto put = [&](uint64_t no, uint64_t start, uint64_t len) {
        if (len > mine) mine = len;
        if (no < cap_records) {
            if (rec_items) rec_items[no] = r.item;
            rec_offsets[no] = start - origin;
            rec_lengths[no] = len;
        }
    };
    for (uint64_t p0 = w0; p0 <= w1; p0 += 256u) {          // (no thread leaves the loop early: the scans need them all)
        const uint64_t w = p0 + threadIdx.x;
        const uint64_t x = w <= w1 ? map[w] : 0ull;
        const uint64_t at = (w - b) << 6;                    // position of the word's bit 0
        uint64_t sum, edge;
        uint64_t rank = rank0 + group_scan_excl64((uint64_t)__builtin_popcountll(x), wave_sum, &sum);
        uint64_t prev = group_max_excl64(x != 0ull ? at + (64u - (uint32_t)__builtin_clzll(x)) + 1u : 0ull, wave_max, &edge);
        uint64_t start = prev != 0ull ? prev - 1u : open;    // (one past the delimiter in front, itself kept one up so that 0 says none)
        for (uint64_t bits = x; bits != 0ull; bits &= bits - 1u) {
            const uint64_t p = at + (uint32_t)__builtin_ctzll(bits);
            put(first_no + rank, start, p - start + keep);
            start = p + 1u; ++rank;
        }
        rank0 += sum;
        if (edge != 0ull) open = edge - 1u;
    }
    // the item's last record has no terminator: it runs from `open` to the item's end
    if (threadIdx.x == 0u && (r.flags & 6u) == 2u) put(first_no + rank0, open, r.item_end - open);
    __syncthreads();
    if (mine != 0ull) atomicMax(&longest, (unsigned long long)mine);
    __syncthreads();
    if (threadIdx.x == 0u && longest != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(&need[1]), longest);
}

// The call's status word: the count's verdict, raised by what a decoder met (gather_close_kernel's rule).  One thread.
__global__ void records_close_kernel(const RecordWords* __restrict__ words, int32_t* __restrict__ status)
{
    *status = words->worst > words->stream ? words->worst : words->stream;
}

// An index of 0 blocks, or a call that is refused on the device: the first-record table cleared.
__global__ __launch_bounds__(256) void records_clear_kernel(uint64_t* __restrict__ item_first_record, uint32_t n_items)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i <= n_items) item_first_record[i] = 0ull;
}

}  // namespace tsq
