// tsq_cut.cuh -- block ranges cut out of an index, each as a container of its own: out of one indexed container (tsqa_cut_async) or,
// with the item of every range named in device memory, out of ANY index (tsqa_cut_items_async, the "take").  Nothing is decoded: the
// frames of a block range of one item are one span of the index's buffer and are copied behind a new header.  The five launches:
//   cut_measure_kernel   the index's verdict, the item rule, the range rule, each range's size, total and source place
//   cut_sum_kernel       (a) each group of 256 ranges: its padded sizes summed, each range's place inside its group
//   cut_scan_kernel      (b) ONE workgroup: the groups' bases, 256 groups per pass; the two words (c) raises are zeroed
//   cut_place_kernel     (c) the places, the ranges that fit, the headers, the call's status, where the written output ends
//   cut_emit_kernel      the copy, balanced over the output
// No workgroup waits for another: the shape of the sized index's walk (tsq_index.cuh).  The last four read what the first leaves: a
// refused index leaves sizes of 0, and then nothing is placed, fits or is copied.  The container format itself: tsq_format.h.  The
// packed layout: tsqa_plan_packed.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"
#include "tsq_join.cuh"

namespace tsq {

constexpr uint32_t kTakeGroup = 256;                         // ranges per workgroup of launches (a) and (c), groups per pass of launch (b)

// What the call keeps per range in the context's scratch: where the range's first frame starts in the index's buffer, and the two
// fields of its header.  All zero for a refused range.  Entry n_ranges: src_at = where the last fitting container ends in the output.
struct CutRange { uint64_t src_at, total, count; };

// One lane per range.  Nothing in the tables is trusted.  verdict (may be NULL): the word of an index made from a size table; where
// it is nonzero the descriptors are not to be believed, none is read, and every range gets kErrFormat.  d_items == NULL: every range
// is of item 0.  The item must exist and own blocks (item_first: the index's n_items + 1 first blocks; NULL for an index of one item,
// which owns [0, n_blocks)); a refused or unfit item owns none, and its ranges get kErrArg as in gather_measure_kernel.  live (may be
// NULL): the words of a batch index made on the device and not fetched, whose live block count the host does not know: it is
// live[0], n_blocks is the index's cap_blocks, and no descriptor at or past the live count is read.  d_first and d_count, both NULL:
// the whole item; else block ranges counted from the item's own first block: a range must hold a block and lie inside the item,
// compared so that first + count is never formed.  An accepted range gets its size -- 16 + the bytes from its first frame to the end
// of its last --, its total and status 0; a refused one kErrArg, size 0 and total 0, and no descriptor is read for it.  The
// descriptors' stream_at count from the index's buffer and out_at in the concatenation, so the size and the total are differences
// inside one item.
__global__ __launch_bounds__(256) void cut_measure_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, const int32_t* __restrict__ verdict,
                                                          const uint64_t* __restrict__ item_first, uint32_t n_items,
                                                          const uint64_t* __restrict__ live, const uint32_t* __restrict__ d_items,
                                                          const uint64_t* __restrict__ d_first, const uint64_t* __restrict__ d_count,
                                                          uint32_t n_ranges, CutRange* __restrict__ ranges, uint64_t* __restrict__ d_sizes,
                                                          uint64_t* __restrict__ d_totals, int32_t* __restrict__ item_status)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_ranges) return;
    CutRange r{0, 0, 0};
    uint64_t size = 0;
    int32_t st = kOk;
    if (verdict && *verdict != 0) st = kErrFormat;
    else {
        uint64_t all = n_blocks;
        if (live && live[0] < all) all = live[0];
        const uint32_t it = d_items ? d_items[k] : 0u;
        uint64_t fb = 0, fe = 0;                             // (no blocks: refused)
        if (it < n_items) { fb = item_first ? item_first[it] : 0ull; fe = item_first ? item_first[it + 1u] : all; }
        if (fb >= fe || fe > all) st = kErrArg;
        else {
            const uint64_t nb = fe - fb, first = d_first ? d_first[k] : 0ull, count = d_count ? d_count[k] : nb;
            if (count < 1u || first >= nb || count > nb - first) st = kErrArg;
            else {
                const FrameInfo a = frames[fb + first], z = frames[fb + first + count - 1u];
                r.src_at = a.stream_at - kFrameWordSize;
                r.total = z.out_at + z.out_len - a.out_at;
                r.count = count;
                size = kHeaderSize + (z.stream_at + z.stream_len) - r.src_at;
            }
        }
    }
    ranges[k] = r;
    d_sizes[k] = size;
    if (d_totals) d_totals[k] = r.total;
    item_status[k] = st;
}

// Launches (a), (b) and (c) are tsqa_plan_packed's rule applied to the sizes: round_up(size, align) is summed, as every place is a
// multiple of align, and the last place is not rounded.  The places are complete whatever fits.
//
// Launch (a).  Workgroup g of exactly 256 threads: group_sum[g] = round_up(size, align) summed over the ranges [256 g, 256 g + 256),
// and d_offsets[k] = the sum of the group's ranges in front of range k, which (c) puts on top of the group's base.  Every padded
// size is below the index's buffer + 4096, and the host has seen to it that n_ranges of them stay below 2^55 (group_scan_excl64).
__global__ __launch_bounds__(256) void cut_sum_kernel(const uint64_t* __restrict__ d_sizes, uint32_t n_ranges, uint32_t align,
                                                      uint64_t* __restrict__ d_offsets, uint64_t* __restrict__ group_sum)
{
    __shared__ uint64_t wave_sum[4];
    const uint64_t mask = (uint64_t)align - 1u;
    const uint64_t k = (uint64_t)blockIdx.x * kTakeGroup + threadIdx.x;
    const bool valid = k < n_ranges;
    uint64_t sum;
    const uint64_t own = group_scan_excl64(valid ? (d_sizes[k] + mask) & ~mask : 0ull, wave_sum, &sum);
    if (valid) d_offsets[k] = own;                           // (behind the scan, which needs every thread)
    if (threadIdx.x == 0u) group_sum[blockIdx.x] = sum;
}

// Launch (b).  ONE workgroup of exactly 256 threads: group_sum[g] becomes the sum of the groups before g, 256 groups -- 65 536
// ranges -- per pass with the running sum carried in a register (index_scan_kernel's scan, tsq_index.cuh); the sums are (a)'s, all
// of them together below 2^55.  Thread 0 also zeroes the two words that (c) raises with atomicMax: where the written output ends,
// and the call's status.
__global__ __launch_bounds__(256) void cut_scan_kernel(uint64_t* __restrict__ group_sum, uint32_t n_groups, uint64_t* __restrict__ fit_end,
                                                       int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    if (threadIdx.x == 0u) { *fit_end = 0ull; *status = kOk; }
    uint64_t base = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += kTakeGroup) { // (no thread leaves the loop early: the scan needs them all; n_groups <= 2^24)
        const uint32_t g = g0 + threadIdx.x;
        const bool valid = g < n_groups;
        uint64_t sum;
        const uint64_t before = base + group_scan_excl64(valid ? group_sum[g] : 0ull, wave_sum, &sum);
        base += sum;
        if (valid) group_sum[g] = before;                    // (its own entry, which nobody else reads)
    }
}

// Launch (c).  One lane per range: the place is the group's base and the range's own; an accepted range fits when its container
// ends at or before out_size -- a test of the range alone: the places only grow and no accepted range is empty, so the fitting
// ranges are a prefix of the accepted ones by themselves, a range behind one that does not fit cannot fit, in whatever group it
// lies, and no verdict has to be carried from one group to the next.  A range that fits gets its header; one that does not,
// kErrOverflow.  The workgroup's largest fitting end and largest status are gathered in LDS and raised into *fit_end (where the last
// fitting container ends: ranges[n_ranges].src_at) and *status (the largest item status) by one atomicMax each per workgroup, and
// only where there is something to raise: both start at 0 (launch (b)).
__global__ __launch_bounds__(256) void cut_place_kernel(const CutRange* __restrict__ ranges, uint32_t n_ranges, const uint64_t* __restrict__ group_base,
                                                        uint8_t* __restrict__ out, uint64_t out_size, const uint64_t* __restrict__ d_sizes,
                                                        uint64_t* __restrict__ d_offsets, int32_t* __restrict__ item_status,
                                                        uint64_t* __restrict__ fit_end, int32_t* __restrict__ status)
{
    __shared__ unsigned long long group_end;
    __shared__ int32_t worst;
    if (threadIdx.x == 0u) { group_end = 0ull; worst = kOk; }
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kTakeGroup + threadIdx.x;
    if (k < n_ranges) {
        const uint64_t size = d_sizes[k], at = group_base[blockIdx.x] + d_offsets[k];
        int32_t st = item_status[k];
        if (st == kOk) {
            if (at + size <= out_size) {
                write_header(out + at, (uint32_t)ranges[k].count, ranges[k].total);
                atomicMax(&group_end, (unsigned long long)(at + size));
            } else item_status[k] = st = kErrOverflow;
        }
        if (st != kOk) atomicMax(&worst, st);
        d_offsets[k] = at;
        if (k + 1u == n_ranges) d_offsets[n_ranges] = at + size;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    if (group_end != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(fit_end), group_end);
    if (worst != kOk) atomicMax(status, worst);
}

// The copy, balanced over the output as join_emit_kernel's is: a workgroup takes one piece of kJoinPiece bytes of the output after
// the other, up to the end of the last fitting container, cut at multiples of 16 of the destination ADDRESS.  The range that holds
// the piece's first byte is found by bisection in d_offsets (join_item_of: ranges without bytes share their place with the next
// one, and the last of them is found).  Every nonempty range below that end is accepted and fits.  Its body is
// [d_offsets[j] + 16, d_offsets[j] + d_sizes[j]), from ranges[j].src_at on in the index's buffer; its header is
// cut_place_kernel's and the padding behind it is nobody's.  A piece inside one body is join_copy_piece's; elsewhere each word finds
// its own range, and a word cut by a header, a seam, padding or that end goes byte by byte, each byte to the body that holds it, if
// one does.  No 16-byte load runs past its body's end, and no byte outside an accepted range's frames is read.
__global__ __launch_bounds__(256) void cut_emit_kernel(const uint8_t* __restrict__ in, const CutRange* __restrict__ ranges, uint32_t n_ranges,
                                                       const uint64_t* __restrict__ d_offsets, const uint64_t* __restrict__ d_sizes,
                                                       uint8_t* __restrict__ out)
{
    const uint64_t skew = (uintptr_t)out & 15u, v_end = skew + ranges[n_ranges].src_at;          // v = o + skew, as in join_emit_kernel
    for (uint64_t p = blockIdx.x; p * kJoinPiece < v_end; p += gridDim.x) {
        const uint64_t p0 = p * kJoinPiece, p1 = p0 + kJoinPiece;
        const uint64_t lo = p0 > skew ? p0 : skew, hi = p1 < v_end ? p1 : v_end;                // the piece's bytes, as v
        if (lo >= hi) continue;
        const uint32_t j0 = join_item_of(d_offsets, 0u, n_ranges, lo - skew);
        const uint64_t body0 = d_offsets[j0] + kHeaderSize, end0 = d_offsets[j0] + d_sizes[j0];
        if (lo == p0 && hi == p1 && lo - skew >= body0 && hi - skew <= end0) {
            // every word of the piece is whole and of one body: the source of the byte at v is in[delta + v]
            const uint64_t v0 = p0 + ((uint64_t)threadIdx.x << 4);
            join_copy_piece(in + (ranges[j0].src_at - body0 - skew + v0), out + (v0 - skew));
            continue;
        }
        const uint32_t j1 = join_item_of(d_offsets, j0, n_ranges, hi - 1u - skew);
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint64_t v = p0 + ((uint64_t)(u * 256u + threadIdx.x) << 4);
            const uint64_t a = v > lo ? v : lo, b = v + 16u < hi ? v + 16u : hi;
            if (a >= b) continue;
            uint64_t o = a - skew;
            const uint64_t o_end = b - skew;
            uint32_t j = join_item_of(d_offsets, j0, j1 + 1u, o);
            uint64_t at = d_offsets[j];
            if (b - a == 16u && o >= at + kHeaderSize && o_end <= at + d_sizes[j]) {
                uint4 w;
                __builtin_memcpy(&w, in + ranges[j].src_at + (o - at - kHeaderSize), 16);
                *reinterpret_cast<uint4*>(out + o) = w;
                continue;
            }
            for (; o < o_end; ++o) {
                while (o >= d_offsets[j + 1u]) ++j;          // (o < d_offsets[n_ranges]: j stays below n_ranges)
                at = d_offsets[j];
                if (o >= at + kHeaderSize && o < at + d_sizes[j]) out[o] = in[ranges[j].src_at + (o - at - kHeaderSize)];
            }
        }
    }
}

}  // namespace tsq
