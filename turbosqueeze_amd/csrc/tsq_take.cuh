// tsq_take.cuh -- items, and block ranges inside items, cut out of ANY index, each as a container of its own (tsqa_cut_items_async):
// the cut of tsq_cut.cuh with the item of every range named in device memory, for the batch indexes that tsqa_cut_async refuses.
// The frames of a block range of one item are one span of the index's buffer, so the copy is cut_emit_kernel itself.  The launches:
//   take_measure_kernel  the index's verdict, the item rule, the range rule, each range's size, total and source place
//   take_sum_kernel      (a) each group of 256 ranges: its padded sizes summed, each range's place inside its group
//   take_scan_kernel     (b) ONE workgroup: the groups' bases, 256 groups per pass; the two words (c) raises are zeroed
//   take_place_kernel    (c) the places, the ranges that fit, the headers, the call's status, where the written output ends
//   cut_emit_kernel      the copy, balanced over the output (tsq_cut.cuh)
// No workgroup waits for another: the shape of the sized index's walk (tsq_index.cuh).  What (a), (b) and (c) leave is what
// cut_layout_kernel leaves for the same sizes, entry for entry.  The packed layout: tsqa_plan_packed.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_cut.cuh"
#include "tsq_format.h"

namespace tsq {

constexpr uint32_t kTakeGroup = 256;                         // ranges per workgroup of launches (a) and (c), groups per pass of launch (b)

// One lane per range.  Nothing in the tables is trusted.  verdict (may be NULL): as in cut_measure_kernel, a nonzero word refuses
// every range with kErrFormat and nothing else is read.  d_items == NULL: every range is of item 0.  The item must exist and own
// blocks (item_first: the index's n_items + 1 first blocks; NULL for an index of one item, which owns [0, n_blocks)); a refused or
// unfit item owns none, and its ranges get kErrArg as in gather_measure_kernel.  live (may be NULL): the words of a batch index made
// on the device and not fetched, whose live block count the host does not know: it is live[0], n_blocks is the index's cap_blocks,
// and no descriptor at or past the live count is read.  d_first and d_count, both NULL: the whole item; else block ranges counted
// from the item's own first block, held to cut_measure_kernel's rule with the item's block count, first + count never formed.
// An accepted range gets what cut_measure_kernel gives it: the descriptors' stream_at count from the index's buffer and out_at in
// the concatenation, so the size and the total are differences inside one item.
__global__ __launch_bounds__(256) void take_measure_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, const int32_t* __restrict__ verdict,
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

// Launch (a).  Workgroup g of exactly 256 threads: group_sum[g] = round_up(size, align) summed over the ranges [256 g, 256 g + 256),
// and d_offsets[k] = the sum of the group's ranges in front of range k, which (c) puts on top of the group's base.  Every padded
// size is below the index's buffer + 4096, and the host has seen to it that n_ranges of them stay below 2^55 (group_scan_excl64).
__global__ __launch_bounds__(256) void take_sum_kernel(const uint64_t* __restrict__ d_sizes, uint32_t n_ranges, uint32_t align,
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
// ranges -- per pass with the running sum carried in a register (index_scan_kernel's scan, tsq_index.cuh).  Thread 0 also zeroes
// the two words that (c) raises with atomicMax: where the written output ends, and the call's status.
__global__ __launch_bounds__(256) void take_scan_kernel(uint64_t* __restrict__ group_sum, uint32_t n_groups, uint64_t* __restrict__ fit_end,
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

// Launch (c).  One lane per range, what the body of cut_layout_kernel's loop does: the place is the group's base and the range's
// own; an accepted range fits when its container ends at or before out_size -- a test of the range alone: the places only grow and
// no accepted range is empty, so a range behind one that does not fit cannot fit, in whatever group it lies, and no verdict has to
// be carried from one group to the next.  A range that fits gets its header; one that does not, kErrOverflow.  The workgroup's
// largest fitting end and largest status are gathered in LDS and raised into *fit_end and *status by one atomicMax each per
// workgroup, and only where there is something to raise: both start at 0 (launch (b)).
__global__ __launch_bounds__(256) void take_place_kernel(const CutRange* __restrict__ ranges, uint32_t n_ranges, const uint64_t* __restrict__ group_base,
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

}  // namespace tsq
