// tsq_find.cuh -- where a byte string occurs in an index's data (tsqa_find_async).  dec_find_kernel (tsq_dec_sym.cuh) decodes every
// block and leaves one bit per byte in the records' map (tsq_records.cuh: bit G & 63 of word (G >> 6) + b for position G of the
// concatenation in block b): the bit of every position at which a hit ENDS whose start lies in the same block.  It also leaves
// each block's first and last 15 bytes in a table of 32 bytes per block.  What follows here:
//   find_seam_kernel       one lane per block: the ends at its first m - 1 positions, whose hits start in earlier blocks of its item
//   find_count_kernel      one workgroup per block: its hits (the popcount of its words), its item
//   records_sum_kernel, records_scan_kernel, records_place_kernel, records_items_kernel (tsq_records.cuh, unchanged): the blocks'
//                          first hit numbers, the count, the count's verdict, d_item_first_hit
//   find_emit_kernel       one workgroup per block: every hit that ends in the block, numbered, below cap_hits
//   find_close_kernel      the count and the call's status word
// A block's entry is a RecordBlock whose `starts` is its hit count, then its first hit's number, and whose edge and flags stay 0:
// there is no open record and no boundary maximum, and the records' sum, scan and placement then do exactly what is needed.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_dec_common.cuh"
#include "tsq_format.h"
#include "tsq_gather.cuh"
#include "tsq_records.cuh"

namespace tsq {

constexpr uint32_t kFindFlat = 2u;                           // TSQA_FIND_FLAT
constexpr uint32_t kFindMaxNeedle = 16u;                     // TSQA_FIND_MAX_NEEDLE
constexpr uint32_t kFindEdge = 15u;                          // bytes kept of each end of a block: kFindMaxNeedle - 1

// Block b's item and the item's extent in the concatenation, as records_count_kernel finds them: the last item whose first block
// is at or before b (item_first NULL: one item, which owns every block); tables that disagree leave the block alone.
__device__ __forceinline__ void find_item_of(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint64_t total, const uint64_t* __restrict__ item_first,
                                             uint32_t n_items, uint32_t b, const FrameInfo& f, uint32_t* item, uint64_t* item_at, uint64_t* item_end)
{
    uint32_t it = 0;
    uint64_t fb = 0, fe = n_blocks;
    if (item_first) {
        uint32_t lo = 0, hi = n_items;
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (item_first[mid] <= b) lo = mid; else hi = mid; }
        it = lo; fb = item_first[it]; fe = item_first[it + 1u];
        if (fe > n_blocks) fe = n_blocks;
    }
    const uint64_t end = f.out_at + f.out_len;
    *item = it;
    *item_at = gather_block_start(frames, n_blocks, total, fb);
    *item_end = gather_block_start(frames, n_blocks, total, fe);
    if (fb > b || fe <= b || *item_at > f.out_at || *item_end < end) { *item_at = f.out_at; *item_end = end; }
}

// 32 bytes in four words: byte i
__device__ __forceinline__ uint32_t find_window_byte(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint32_t i)
{
    const uint64_t w = i < 8u ? w0 : i < 16u ? w1 : i < 24u ? w2 : w3;
    return (uint32_t)(w >> (8u * (i & 7u))) & 0xFFu;
}

// The seams.  One lane per block that has bytes and is not the first such block of its item: it decides the ends at its positions
// p < min(len, m - 1), which dec_find_kernel left open.  The window is 30 bytes: window[15 - k] is the byte at concatenation
// position out_at - k, k = 1 .. min(m - 1, out_at - item_at), read from the TAIL entry of the block that holds it -- that position
// lies in the last 15 bytes of its block, since the block ends at or before out_at --, and window[15 + j] is byte j of the block's
// own head.  So a run of 1-byte blocks, or empty blocks in between, cost one look-up per byte and no walk.  The bits are ORed into
// the block's own words, which no other lane touches.  No decoded data is read: none exists.
__global__ __launch_bounds__(256) void find_seam_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint64_t total, uint32_t shift,
                                                        const int32_t* __restrict__ verdict, const uint64_t* __restrict__ item_first, uint32_t n_items,
                                                        uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t m,
                                                        const uint8_t* __restrict__ edges, uint64_t* __restrict__ map, uint64_t map_words)
{
    const uint64_t b64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b64 >= n_blocks || m < 2u || (verdict && *verdict != 0)) return;
    const uint32_t b = (uint32_t)b64;
    const FrameInfo f = frames[b];
    if (f.out_len == 0u) return;
    uint32_t item;
    uint64_t item_at, item_end;
    find_item_of(frames, n_blocks, total, item_first, n_items, b, f, &item, &item_at, &item_end);
    if (f.out_at <= item_at) return;                         // the item's first block with bytes: no hit starts in front of it
    const uint64_t room = f.out_at - item_at;
    const uint32_t n_front = room < m - 1u ? (uint32_t)room : m - 1u;
    uint64_t w[4] = {0ull, 0ull, 0ull, 0ull};
    auto put = [&](uint32_t i, uint32_t v) {
        const uint64_t x = (uint64_t)v << (8u * (i & 7u));
        if (i < 8u) w[0] |= x; else if (i < 16u) w[1] |= x; else if (i < 24u) w[2] |= x; else w[3] |= x;
    };
    for (uint32_t k = 1; k <= n_front; ++k) {
        const uint64_t q = f.out_at - k;
        const uint32_t bq = gather_block_of(frames, n_blocks, shift, q);
        if (bq >= b) return;                                 // (descriptors that disagree: nothing is decided)
        const FrameInfo fq = frames[bq];
        const uint64_t d = fq.out_at + fq.out_len - q;       // the byte's distance from its block's end, 1 .. 15
        if (d < 1u || d > kFindEdge) return;
        put(15u - k, edges[((size_t)bq << 5) + 16u + (kFindEdge - (uint32_t)d)]);
    }
    const uint32_t n_head = f.out_len < kFindEdge ? f.out_len : kFindEdge;
    for (uint32_t j = 0; j < n_head; ++j) put(15u + j, edges[((size_t)b << 5) + j]);
    const FindNeedle nd = {((uint64_t)n1 << 32) | n0, ((uint64_t)n3 << 32) | n2, m};
    const uint32_t n_ends = f.out_len < m - 1u ? f.out_len : m - 1u;
    for (uint32_t p = 0; p < n_ends; ++p) {
        if (m - 1u - p > n_front) continue;                  // the hit would start in front of the item
        const uint32_t s = 15u + p - (m - 1u);
        bool hit = true;
        for (uint32_t k = 0; k < m && hit; ++k) hit = find_window_byte(w[0], w[1], w[2], w[3], s + k) == find_needle_byte(nd, k);
        if (!hit) continue;
        const uint64_t g = f.out_at + p, word = (g >> 6) + b;
        // (a plain read-modify-write: no map word belongs to two blocks, one lane has the block, and the decode that ORed into
        //  these words with atomics is an earlier launch on the same stream)
        if (word < map_words) map[word] |= 1ull << (g & 63u);
    }
}

// One workgroup of 256 threads per block: its hits are the bits of its words.  verdict nonzero: no descriptor is read and the
// block holds nothing.
__global__ __launch_bounds__(256) void find_count_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint64_t total,
                                                         const int32_t* __restrict__ verdict, const uint64_t* __restrict__ item_first,
                                                         uint32_t n_items, const uint64_t* __restrict__ map, uint64_t map_words,
                                                         RecordBlock* __restrict__ blocks)
{
    __shared__ uint64_t wave_sum[4];
    const uint32_t b = blockIdx.x;
    if (verdict && *verdict != 0) {
        if (threadIdx.x == 0u) blocks[b] = RecordBlock{0ull, 0ull, 0ull, 0ull, 0u, 0u};
        return;
    }
    const FrameInfo f = frames[b];
    uint64_t w0 = 0, w1 = 0;
    const bool any = records_words_of(f, b, map_words, &w0, &w1);
    uint64_t count = 0;
    if (any)
        for (uint64_t w = w0 + threadIdx.x; w <= w1; w += 256u) count += (uint32_t)__builtin_popcountll(map[w]);
    uint64_t hits;
    (void)group_scan_excl64(count, wave_sum, &hits);
    if (threadIdx.x != 0u) return;
    RecordBlock r{0ull, 0ull, 0ull, 0ull, 0u, 0u};
    if (any) {
        find_item_of(frames, n_blocks, total, item_first, n_items, b, f, &r.item, &r.item_at, &r.item_end);
        r.starts = hits;
    }
    blocks[b] = r;
}

// One workgroup of 256 threads per block, the block's words in passes of one per lane: a prefix over the popcounts ranks the set
// bits, and the bit of rank r is hit number first + r, which starts m - 1 in front of its end.  A hit numbered at or past cap_hits
// is not written; hit_items may be NULL.
__global__ __launch_bounds__(256) void find_emit_kernel(const FrameInfo* __restrict__ frames, const int32_t* __restrict__ verdict,
                                                        const uint64_t* __restrict__ map, uint64_t map_words, const RecordBlock* __restrict__ blocks,
                                                        uint32_t m, uint32_t flags, uint64_t cap_hits, uint32_t* __restrict__ hit_items,
                                                        uint64_t* __restrict__ hit_offsets)
{
    __shared__ uint64_t wave_sum[4];
    if (cap_hits == 0ull || (verdict && *verdict != 0)) return;
    const uint32_t b = blockIdx.x;
    const FrameInfo f = frames[b];
    uint64_t w0 = 0, w1 = 0;
    if (!records_words_of(f, b, map_words, &w0, &w1)) return;
    const RecordBlock r = blocks[b];
    if (r.starts >= cap_hits) return;                        // (the whole workgroup: the block's first hit is past the tables)
    const uint64_t origin = (flags & kFindFlat ? 0ull : r.item_at) + (m - 1u);
    uint64_t rank0 = r.starts;
    for (uint64_t p0 = w0; p0 <= w1; p0 += 256u) {          // (no thread leaves the loop early: the scan needs them all)
        const uint64_t w = p0 + threadIdx.x;
        const uint64_t x = w <= w1 ? map[w] : 0ull;
        const uint64_t at = (w - b) << 6;                    // position of the word's bit 0
        uint64_t sum;
        uint64_t rank = rank0 + group_scan_excl64((uint64_t)__builtin_popcountll(x), wave_sum, &sum);
        for (uint64_t bits = x; bits != 0ull && rank < cap_hits; bits &= bits - 1u, ++rank) {
            const uint64_t end = at + (uint32_t)__builtin_ctzll(bits);
            if (hit_items) hit_items[rank] = r.item;
            hit_offsets[rank] = end - origin;
        }
        rank0 += sum;
    }
}

// The call's words: the count of all hits, and the status -- the count's verdict, raised by what a decoder met
// (records_close_kernel's rule).  One thread.
__global__ void find_close_kernel(const RecordWords* __restrict__ words, const uint64_t* __restrict__ count, uint64_t* __restrict__ need,
                                  int32_t* __restrict__ status)
{
    need[0] = count[0];
    *status = words->worst > words->stream ? words->worst : words->stream;
}

}  // namespace tsq
