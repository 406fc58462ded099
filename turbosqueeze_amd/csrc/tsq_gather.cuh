// tsq_gather.cuh -- record reads whose ranges lie in device memory (tsqa_gather_async): the plan that plan_ranges and
// plan_item_ranges make on the host (tsq_runtime.hip) is made on the device, with nothing trusted and nothing read back, and the
// output is dense: each range's place is a prefix sum, so no two destinations can overlap.  The launches:
//   gather_measure_kernel   the index's verdict, the range rule, each range's first block and piece count
//   gather_layout_kernel    the places, the piece numbers, the ranges that fit, the largest status
//   gather_pieces_kernel    every fitting range cut at the block edges, in range order, and each piece's key (block, lo)
//   (the sort)              the (key, slot) pairs by key, stable: tsq_gather.hip
//   gather_groups_kernel    the pieces in sorted order, and each touched block's group numbered
//   gather_spans_kernel     each group's count and its largest hi
//   dec_group_live_kernel   dec_group_kernel behind a group count made on the device
//   gather_close_kernel     the call's status word
// Each reads what the ones before it leave; a refused index leaves ranges without bytes, and then nothing is placed, cut or decoded.
// The order of the pieces is the host plan's: range order, then a stable sort by (block, lo) -- std::stable_sort there, a stable
// radix sort of block << 22 | lo here --, so the items and groups are the host's entry for entry.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_dec_sym.cuh"
#include "tsq_format.h"

namespace tsq {

// What the call keeps per range in the context's scratch: where the range starts in the concatenation of the index's data, its
// length (0 for a refused range), its first block and piece count, and the number of its first piece.
struct GatherRange { uint64_t at, len, piece_at; uint32_t first_block, pieces; };

// The call's words in the context's scratch.  fit_pieces: the pieces of the fitting ranges; n_groups: the touched blocks; worst:
// the largest range status; stream: the decoders' word, zero until one of them meets a malformed stream.
struct GatherWords { uint64_t fit_pieces; uint32_t n_groups; int32_t worst, stream; uint32_t pad; };

constexpr uint32_t kGatherLoBits = 22;                       // lo < 2^22: a block holds at most kBlockSize bytes
static_assert(kBlockSize <= (1u << kGatherLoBits), "a piece's lo fits the key's low bits");

// Where block b starts in the concatenation; b == n_blocks: the total.
__device__ __forceinline__ uint64_t gather_block_start(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint64_t total, uint64_t b)
{
    return b < n_blocks ? frames[b].out_at : total;
}

// plan_ranges' first_block: the last block that starts at or before byte `at` (blocks of length 0 are passed over).  at < total,
// so n_blocks >= 1, and block 0 starts at 0.
__device__ __forceinline__ uint32_t gather_block_of(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint32_t shift, uint64_t at)
{
    if (shift) return (uint32_t)(at >> shift);               // a sized index: block b starts at b << shift (index_check_kernel)
    uint32_t lo = 0, hi = n_blocks;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (frames[mid].out_at <= at) lo = mid; else hi = mid;
    }
    return lo;
}

// One lane per range.  The tables are not trusted.  verdict (may be NULL): the word of an index made from a size table; where it is
// nonzero every range gets kErrFormat and no descriptor is read.  d_items == NULL: the range is of the whole data; else of item
// d_items[k], which must exist and own blocks (item_first: the index's n_items + 1 first blocks; NULL for an index of one item,
// which owns [0, n_blocks)).  The range must end inside its total, compared so that offset + length is never formed.  A refused
// range gets kErrArg, no bytes and no pieces.  An accepted one its place, its first block and the blocks with bytes from there to
// its last byte's: on a sized index that is arithmetic, elsewhere the descriptors in between are read (a block may be empty).
// kLive: a batch index made on the device and not fetched (tsq_index_packed.cuh), whose total the host does not know: it is read
// from live[1], and n_blocks is the index's cap_blocks -- the descriptors past the live ones start at the total and are empty, so
// every look-up above finds what it finds over the live ones.  The other instantiation does not look at `live`.
template <bool kLive>
__global__ __launch_bounds__(256) void gather_measure_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint64_t total, uint32_t shift,
                                                             const int32_t* __restrict__ verdict, const uint64_t* __restrict__ item_first,
                                                             uint32_t n_items, const uint32_t* __restrict__ d_items,
                                                             const uint64_t* __restrict__ d_offsets, const uint64_t* __restrict__ d_lengths,
                                                             uint32_t n_ranges, GatherRange* __restrict__ ranges, int32_t* __restrict__ range_status,
                                                             const uint64_t* __restrict__ live)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_ranges) return;
    if constexpr (kLive) total = live[1];
    GatherRange r{0, 0, 0, 0u, 0u};
    int32_t st = kOk;
    if (verdict && *verdict != 0) st = kErrFormat;
    else {
        const uint64_t offset = d_offsets[k], len = d_lengths[k];
        uint64_t base = 0, mine = total;
        if (d_items) {
            const uint32_t it = d_items[k];
            if (it >= n_items) st = kErrArg;
            else {
                const uint64_t fb = item_first ? item_first[it] : 0ull, fe = item_first ? item_first[it + 1u] : (uint64_t)n_blocks;
                if (fb >= fe || fe > n_blocks) st = kErrArg;                                  // (a refused item owns no blocks)
                else { base = gather_block_start(frames, n_blocks, total, fb); mine = gather_block_start(frames, n_blocks, total, fe) - base; }
            }
        }
        if (st == kOk && (len > mine || offset > mine - len)) st = kErrArg;
        if (st == kOk && len != 0u) {
            r.at = base + offset; r.len = len;
            const uint32_t first = gather_block_of(frames, n_blocks, shift, r.at), last = gather_block_of(frames, n_blocks, shift, r.at + (len - 1u));
            r.first_block = first;
            if (shift) r.pieces = last - first + 1u;
            else for (uint32_t b = first; b <= last && b < n_blocks; ++b) r.pieces += frames[b].out_len != 0u;
        }
    }
    ranges[k] = r;
    range_status[k] = st;
}

// Behind gather_measure_kernel: tsqa_plan_packed's rule applied to the accepted ranges' lengths, and the piece numbers.  ONE
// workgroup of exactly 256 threads, 256 ranges per pass as cut_scan_kernel takes its groups, with two sums carried: round_up(length,
// align) -- every place is a multiple of align, and the last length is not rounded -- and the piece counts.  A refused range counts
// as nothing.  The places are complete whatever fits.  An accepted range fits when its bytes end at or before out_cap and its pieces
// at or before cap_pieces (one without bytes asks for neither); both sums only grow, so the fitting ranges are a prefix of the
// accepted ones, and the kernel holds on to that as batch_layout_kernel does: the first range that does not fit ends the prefix, a
// range without bytes behind it included.
// One that does not fit gets kErrOverflow and loses its bytes: nothing of it is cut or written.  *need_pieces = the accepted ranges'
// pieces; words: the fitting ranges' pieces, the largest status (into *status too), and the decoders' word and group count cleared.
// The host has seen to it that n_ranges times the largest padded length, and times the block count, stay below 2^55.
__global__ __launch_bounds__(256) void gather_layout_kernel(GatherRange* __restrict__ ranges, uint32_t n_ranges, uint32_t align, uint64_t out_cap,
                                                            uint32_t cap_pieces, uint64_t* __restrict__ d_out_offsets,
                                                            int32_t* __restrict__ range_status, uint64_t* __restrict__ need_pieces,
                                                            GatherWords* __restrict__ words, int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ unsigned long long fit_pieces;
    __shared__ uint32_t first_unfit;
    __shared__ int32_t worst;
    const uint64_t mask = (uint64_t)align - 1u;
    if (threadIdx.x == 0) { fit_pieces = 0ull; first_unfit = ~0u; worst = kOk; }
    uint64_t out_base = 0, piece_base = 0;
    for (uint64_t k0 = 0; k0 < n_ranges; k0 += 256u) {       // (no lane leaves the loop early: the scans and the barrier need them all)
        const uint64_t k = k0 + threadIdx.x;
        const bool valid = k < n_ranges;
        uint64_t len = 0;
        uint32_t pieces = 0;
        int32_t st = kOk;
        if (valid) { len = ranges[k].len; pieces = ranges[k].pieces; st = range_status[k]; }
        uint64_t sum;
        const uint64_t at = out_base + group_scan_excl64((len + mask) & ~mask, wave_sum, &sum);
        out_base += sum;
        const uint64_t piece_at = piece_base + group_scan_excl64(pieces, wave_sum, &sum);
        piece_base += sum;
        const bool accepted = valid && st == kOk;
        const bool fits = accepted && (len == 0u || (at + len <= out_cap && piece_at + pieces <= cap_pieces));
        if (accepted && !fits) atomicMin(&first_unfit, (uint32_t)k);
        __syncthreads();
        if (!valid) continue;                                // (nothing below is a barrier)
        if (accepted) {
            if (k < first_unfit) { ranges[k].piece_at = piece_at; atomicMax(&fit_pieces, (unsigned long long)(piece_at + pieces)); }
            else { ranges[k].len = 0; ranges[k].pieces = 0u; range_status[k] = st = kErrOverflow; }
        }
        if (st != kOk) atomicMax(&worst, st);
        d_out_offsets[k] = at;
        if (k + 1u == n_ranges) d_out_offsets[n_ranges] = at + len;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    *need_pieces = piece_base;
    *status = worst;
    *words = GatherWords{fit_pieces, 0u, worst, kOk, 0u};
}

// Lane i, two jobs.  As range i: a range that fits is cut at the block edges from its first block on, and its pieces go to the
// slots [piece_at, piece_at + pieces) in block order, each as the RangeItem {block, lo, hi, 0, out_at} that plan_ranges makes, with
// the key block << 22 | lo and its own slot number as the value.  As slot i: a slot from the fitting pieces' total up to cap_pieces
// gets the key of all ones, which sorts behind every piece.  The slots below the total are all some range's: the piece numbers are
// an exclusive sum of the very counts the ranges fill.  No slot at or past piece_at + pieces is written, whatever the descriptors say.
__global__ __launch_bounds__(256) void gather_pieces_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, const GatherRange* __restrict__ ranges,
                                                            uint32_t n_ranges, const int32_t* __restrict__ range_status,
                                                            const uint64_t* __restrict__ d_out_offsets, const GatherWords* __restrict__ words,
                                                            uint32_t cap_pieces, RangeItem* __restrict__ items, uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ slots)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < cap_pieces && i >= words->fit_pieces) { keys[i] = ~0ull; slots[i] = (uint32_t)i; }
    if (i >= n_ranges || range_status[i] != kOk) return;
    const GatherRange r = ranges[i];
    if (r.len == 0u) return;
    const uint64_t end = r.at + r.len, out_at = d_out_offsets[i], m_end = r.piece_at + r.pieces;
    uint64_t m = r.piece_at;
    for (uint32_t b = r.first_block; b < n_blocks && m < m_end; ++b) {
        const FrameInfo f = frames[b];
        if (f.out_at >= end) break;
        const uint64_t a = r.at > f.out_at ? r.at : f.out_at, e = end < f.out_at + f.out_len ? end : f.out_at + f.out_len;
        if (a >= e) continue;
        const uint32_t lo = (uint32_t)(a - f.out_at);
        items[m] = RangeItem{b, lo, (uint32_t)(e - f.out_at), 0u, out_at + (a - r.at)};
        keys[m] = (uint64_t)b << kGatherLoBits | lo;
        slots[m] = (uint32_t)m;
        ++m;
    }
}

// Behind the sort.  Workgroups 1 and up: the pieces go into sorted order, sorted[i] = items[slots[i]] for i below the fitting
// pieces' total.  Workgroup 0 (exactly 256 threads) numbers the groups from the sorted keys alone: a head flag where the block
// (key >> 22) changes, an exclusive sum of the flags for the group's number -- 256 pieces per pass, the sum carried -- and each head
// writes its group's block and first piece.  words->n_groups = the groups: what the decode launch is cut to.  cap_groups bounds
// every write to `groups`; there are never more groups than pieces or blocks.
__global__ __launch_bounds__(256) void gather_groups_kernel(const RangeItem* __restrict__ items, const uint64_t* __restrict__ keys,
                                                            const uint32_t* __restrict__ slots, GatherWords* __restrict__ words,
                                                            uint32_t cap_pieces, RangeItem* __restrict__ sorted, BlockGroup* __restrict__ groups,
                                                            uint32_t cap_groups)
{
    const uint64_t fit = words->fit_pieces < cap_pieces ? words->fit_pieces : cap_pieces;
    if (blockIdx.x != 0u) {
        for (uint64_t i = (uint64_t)(blockIdx.x - 1u) * 256u + threadIdx.x; i < fit; i += (uint64_t)(gridDim.x - 1u) * 256u) {
            const uint32_t from = slots[i];
            if (from < cap_pieces) sorted[i] = items[from];
        }
        return;
    }
    __shared__ uint64_t wave_sum[4];
    uint64_t base = 0;
    for (uint64_t i0 = 0; i0 < fit; i0 += 256u) {            // (no lane leaves the loop early: the scan needs them all)
        const uint64_t i = i0 + threadIdx.x;
        const bool valid = i < fit;
        const uint64_t block = valid ? keys[i] >> kGatherLoBits : 0ull;
        const bool head = valid && (i == 0u || block != keys[i - 1u] >> kGatherLoBits);
        uint64_t sum;
        const uint64_t g = base + group_scan_excl64(head ? 1ull : 0ull, wave_sum, &sum);
        base += sum;
        if (head && g < cap_groups) groups[g] = BlockGroup{(uint32_t)block, (uint32_t)i, 0u, 0u};
    }
    if (threadIdx.x == 0u) words->n_groups = (uint32_t)(base < cap_groups ? base : cap_groups);
}

// Behind gather_groups_kernel, one lane per group: the count is where the next group starts, and hi the largest hi of the group's
// pieces (they are sorted by lo, not by hi).  A launch of its own, so that the groups are closed by as many lanes as there can be
// groups and not by one workgroup's 256.
__global__ __launch_bounds__(256) void gather_spans_kernel(const RangeItem* __restrict__ sorted, const GatherWords* __restrict__ words,
                                                           uint32_t cap_pieces, BlockGroup* __restrict__ groups, uint32_t cap_groups)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t n_groups = words->n_groups < cap_groups ? words->n_groups : cap_groups;
    if (g >= n_groups) return;
    const uint64_t fit = words->fit_pieces < cap_pieces ? words->fit_pieces : cap_pieces;
    const uint32_t first = groups[g].first, next = g + 1u < n_groups ? groups[g + 1u].first : (uint32_t)fit;
    uint32_t hi = 0;
    for (uint32_t j = first; j < next && j < fit; ++j) { const uint32_t h = sorted[j].hi; hi = h > hi ? h : hi; }
    groups[g].count = next - first;
    groups[g].hi = hi;
}

// dec_group_kernel for a group count made on the device: the launch has as many workgroups as there can be groups, and those at or
// past *live_groups leave before they touch a group, LDS or a barrier, as dec_item_kernel's do behind live_blocks.
__global__ __launch_bounds__(1024) void dec_group_live_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames, uint32_t n_frames,
                                                              const RangeItem* __restrict__ items, uint32_t n_items, const BlockGroup* __restrict__ groups,
                                                              uint8_t* __restrict__ outbuf, int32_t* __restrict__ status,
                                                              const uint32_t* __restrict__ live_groups)
{
    if (blockIdx.x >= *live_groups) return;
    sym_decode_block<kDecGroup>(container, frames, n_frames, items, outbuf, status, groups, n_items);
}

// Behind the decode: the decoders report into a word of their own, which has to be zero for them to run at all, so the call's word
// is put together here: the largest range status, raised by what a decoder met.  One thread.
__global__ void gather_close_kernel(const GatherWords* __restrict__ words, int32_t* __restrict__ status)
{
    *status = words->worst > words->stream ? words->worst : words->stream;
}

}  // namespace tsq
