// tsq_batch_split.cuh -- the pack scan of a packed batch of short blocks (tsqa_compress_batch_packed_split*,
// tsqa_compress_batch_packed_tables_split_async): batch_pack_scan_packed_body (tsq_batch.cuh) made parallel over the launch's blocks.
// There one lane walks an item's blocks in the launch, twice; with blocks of TSQ_BLOCK_SZ an item rarely owns more than a few of a
// launch, with short blocks one item can own all 2 x CUs of them, behind an encode that lasts about as long as one 4 KiB chain.
#pragma once

#include "tsq_batch.cuh"
#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"

namespace tsq {

constexpr uint32_t kSplitScanBlocks = 1024;   // the most blocks of one encode launch that the scan takes (the chip's 2 x CUs is 512)

// After an encode launch of the batch's blocks [b0, b0 + nb) (block b in slot b - b0, nb <= kSplitScanBlocks), whose items with
// blocks in it -- and, from device tables, the items without blocks among them -- are [i0, i0 + ni).  ONE workgroup of exactly 256
// threads, three steps, no lane ever walking an item's blocks:
//   1. E[0 .. nb] in LDS: the exclusive sum of (3 + sizes[k]) over the launch's blocks, 256 per pass.
//   2. One lane per item, 256 per pass, as batch_pack_scan_packed_body has them: the item's bytes so far are carry + E[l] - E[f] for
//      its blocks [f, l) of the launch, carry = 16 where it begins in the launch (its header goes out here), else run_at[i], what
//      its previous launch left.  The same scan over round_up(size, align) of the items complete in the launch makes the starts;
//      d_offsets, d_sizes, run_at and the verdicts are written exactly as there.  Only the window's first item can have begun in
//      an earlier launch, so one word (carry0) keeps the carry that its lane has overwritten.
//   3. Behind a barrier, one lane per block: frame_at[k] = start + carry + E[k] - E[f] of its item block_item[b0 + k], whose start
//      is d_offsets[i]: the window's first item found it there, every other one had it written in step 2 by the lane of the item
//      in front of it (all but the window's last are complete).  Then the fit rule -- a header or frame is written only if it ends
//      at or before out_size --, write_frame or kNoFrame, and d_block_sizes[b0 + k] (may be NULL) = the stream length, whatever fits.
// max_stream: the longest stream the copy behind this kernel moves whole (its pieces are counted from block_bound(block_len)); a
// longer one -- the encoder never makes it -- is kErrOverflow in *status, not a silent cut.  All sums stay below 2^55.
__device__ __forceinline__ void batch_split_scan_body(const BatchItem* __restrict__ items, uint32_t n_items, uint32_t i0, uint32_t ni,
                                                      uint64_t b0, uint32_t nb, const uint32_t* __restrict__ sizes,
                                                      const uint32_t* __restrict__ block_item, uint32_t ext, uint32_t align,
                                                      uint32_t max_stream, uint8_t* __restrict__ out, uint64_t out_size,
                                                      uint64_t* __restrict__ run_at, uint64_t* __restrict__ frame_at, uint64_t* d_offsets,
                                                      uint64_t* __restrict__ d_sizes, uint32_t* __restrict__ d_block_sizes,
                                                      int32_t* __restrict__ item_status, int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ uint64_t E[kSplitScanBlocks + 1];
    __shared__ uint64_t carry0;
    const uint32_t t = threadIdx.x;
    const uint64_t mask = (uint64_t)align - 1u, launch_end = b0 + nb;

    uint64_t run = 0;
    for (uint32_t k0 = 0; k0 < nb; k0 += 256u) {             // (no thread leaves a loop early: the scans need them all)
        const uint32_t k = k0 + t;
        const bool valid = k < nb;
        uint64_t sum;
        const uint64_t e = run + group_scan_excl64(valid ? kFrameWordSize + (uint64_t)sizes[k] : 0ull, wave_sum, &sum);
        if (valid) E[k] = e;
        run += sum;
    }
    if (t == 0u) E[nb] = run;
    __syncthreads();

    const uint64_t start0 = b0 == 0 ? 0ull : d_offsets[i0];  // where the launch's first item starts
    uint64_t base = start0;
    if (b0 == 0 && t == 0u) d_offsets[0] = 0;
    for (uint32_t j0 = 0; j0 < ni; j0 += 256u) {
        const uint32_t j = j0 + t, i = i0 + (j < ni ? j : 0u);
        const bool valid = j < ni;
        const BatchItem it = valid ? items[i] : BatchItem{0, 0, 0, 0, 0, 0u, 0u};
        const uint64_t first = it.first_block, end = first + it.n_blocks;
        // (an item without blocks: no header either; the window holds no item with blocks that has none in the launch)
        const bool has = it.n_blocks != 0u && first < launch_end && end > b0, begins = first >= b0;
        const uint64_t carry = has && !begins ? run_at[i] : (uint64_t)kHeaderSize;
        const uint64_t at = has ? carry + E[(end < launch_end ? end : launch_end) - b0] - E[begins ? first - b0 : 0u] : 0ull;
        const bool complete = valid && end <= launch_end;    // (only the launch's last item can be incomplete: it adds nothing)
        uint64_t total;
        const uint64_t start = base + group_scan_excl64(complete ? (at + mask) & ~mask : 0ull, wave_sum, &total);
        base += total;
        if (valid) {
            if (has && begins && start + kHeaderSize <= out_size) write_header(out + start, it.n_blocks, it.in_len);
            if (has && !begins) carry0 = carry;
            run_at[i] = at;
        }
        if (complete) {
            const bool last = i + 1u == n_items, over = start + at > out_size;
            d_sizes[i] = at;
            d_offsets[i + 1u] = last ? start + at : start + ((at + mask) & ~mask);
            if (item_status ? over && it.n_blocks != 0u : over && last) atomicMax(status, kErrOverflow);
            if (item_status && over && it.n_blocks != 0u) item_status[i] = kErrOverflow;
        }
    }
    __syncthreads();                                         // (carry0, and the starts in d_offsets, for the lanes below)

    for (uint32_t k = t; k < nb; k += 256u) {
        const uint64_t b = b0 + k;
        const uint32_t i = block_item[b], sz = sizes[k];
        const uint64_t first = items[i].first_block;
        const bool begins = first >= b0;
        const uint64_t at = (i == i0 ? start0 : d_offsets[i]) + (begins ? (uint64_t)kHeaderSize : carry0) + E[k] - E[begins ? first - b0 : 0u];
        const bool fits = at + kFrameWordSize + sz <= out_size;
        if (fits) write_frame(out + at, sz, ext);
        frame_at[k] = fits ? at : kNoFrame;
        if (d_block_sizes) d_block_sizes[b] = sz;
        if (sz > max_stream) atomicMax(status, kErrOverflow);
    }
}

// The items [i0, i0 + ni) with blocks in the launch of the batch's blocks [b0, b0 + nb), found on the host
// (tsqa_compress_batch_packed_split_async).
__global__ __launch_bounds__(256) void batch_split_scan_kernel(const BatchItem* __restrict__ items, uint32_t n_items, uint32_t i0, uint32_t ni,
                                                               uint64_t b0, uint32_t nb, const uint32_t* __restrict__ sizes,
                                                               const uint32_t* __restrict__ block_item, uint32_t ext, uint32_t align,
                                                               uint32_t max_stream, uint8_t* __restrict__ out, uint64_t out_size,
                                                               uint64_t* __restrict__ run_at, uint64_t* __restrict__ frame_at,
                                                               uint64_t* d_offsets, uint64_t* __restrict__ d_sizes,
                                                               uint32_t* __restrict__ d_block_sizes, int32_t* __restrict__ status)
{
    batch_split_scan_body(items, n_items, i0, ni, b0, nb, sizes, block_item, ext, align, max_stream, out, out_size, run_at, frame_at, d_offsets,
                          d_sizes, d_block_sizes, nullptr, status);
}

// The same behind launch l of a batch whose item table was made on the device (tsqa_compress_batch_packed_tables_split_async): the
// window rules are batch_pack_scan_tables_kernel's, word for word -- launch_item, *live_blocks, dead launches, and the items
// without blocks carried over in the launch that completes the item with blocks in front of them.
__global__ __launch_bounds__(256) void batch_split_scan_tables_kernel(const BatchItem* __restrict__ items, uint32_t n_items,
                                                                      const uint32_t* __restrict__ launch_item, uint32_t l, uint32_t budget,
                                                                      const uint32_t* __restrict__ live_blocks,
                                                                      const uint32_t* __restrict__ sizes,
                                                                      const uint32_t* __restrict__ block_item, uint32_t ext, uint32_t align,
                                                                      uint32_t max_stream, uint8_t* __restrict__ out, uint64_t out_size,
                                                                      uint64_t* __restrict__ run_at, uint64_t* __restrict__ frame_at,
                                                                      uint64_t* d_offsets, uint64_t* __restrict__ d_sizes,
                                                                      uint32_t* __restrict__ d_block_sizes, int32_t* __restrict__ item_status,
                                                                      int32_t* __restrict__ status)
{
    const uint64_t live = *live_blocks, b0 = (uint64_t)l * budget;
    if (l != 0u && b0 >= live) return;                       // (the whole workgroup, before any barrier)
    const uint64_t end = b0 + budget < live ? b0 + budget : live;
    const uint32_t i0 = l != 0u ? launch_item[l] : 0u;
    uint32_t i1 = n_items;
    if (end < live) { const uint32_t e = launch_item[l + 1u]; i1 = e + (items[e].first_block < end ? 1u : 0u); }
    batch_split_scan_body(items, n_items, i0, i1 - i0, b0, (uint32_t)(end - b0), sizes, block_item, ext, align, max_stream, out, out_size, run_at,
                          frame_at, d_offsets, d_sizes, d_block_sizes, item_status, status);
}

}  // namespace tsq
