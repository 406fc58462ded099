// tsq_batch.cuh -- batches of independent items (tsqa_compress_batch*, tsqa_decompress_batch*): the container pack across encode
// launches, the frame walk and the header gather.  The container format itself: tsq_format.h.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"

namespace tsq {

// One item of a batch as the kernels see it, planned on the host (tsqa_plan_batch): its input and output ranges, relative to the
// batch's input and output, its first block in the batch and its block count.  The dense decompress makes the table on the device
// (batch_measure_kernel, batch_layout_kernel); only there is unfit used: 1 marks an item that did not fit the caller's room.  The
// compress from device tables makes it there too (batch_measure_tables_kernel, batch_layout_tables_kernel): a refused or unfit item
// is all zeros there, and an item without blocks has no container: size 0, nothing written.
struct BatchItem { uint64_t in_at, in_len, out_at, out_cap, first_block; uint32_t n_blocks, unfit; };

constexpr uint64_t kNoFrame = ~0ull;      // frame_at of a block whose frame does not fit its item: batch_pack_copy_kernel skips it

// The frames of item `it` in the encode launch of the batch's blocks [b0, b0 + nb) (block b in slot b - b0), for
// batch_pack_scan_kernel.  The item's frame offsets run on from where its previous launch left them (*run_at; the caller stores
// what this returns), and its header goes out with its first block.  The item's container starts at out + start, and a header or
// frame is written only if it ends at or before out + limit: frame_at[b - b0] is the frame's offset in `out`, or kNoFrame.
__device__ __forceinline__ uint64_t batch_item_frames(const BatchItem& it, const uint64_t* run_at, uint64_t b0, uint32_t nb,
                                                     const uint32_t* __restrict__ sizes, uint32_t ext, uint8_t* out, uint64_t start,
                                                     uint64_t limit, uint64_t* frame_at)
{
    if (it.n_blocks == 0u) return 0;                         // (the planner refuses an empty item; one without blocks has no header either)
    const uint64_t first = it.first_block, end = first + it.n_blocks, launch_end = b0 + nb;
    const bool begins = first >= b0;
    if (begins && start + kHeaderSize <= limit) write_header(out + start, it.n_blocks, it.in_len);
    uint64_t at = begins ? kHeaderSize : *run_at;
    for (uint64_t b = begins ? first : b0; b < end && b < launch_end; ++b) {
        const uint32_t k = (uint32_t)(b - b0), sz = sizes[k];
        const uint64_t next = at + kFrameWordSize + sz;
        const bool fits = start + next <= limit;
        if (fits) write_frame(out + start + at, sz, ext);
        frame_at[k] = fits ? start + at : kNoFrame;
        at = next;
    }
    return at;
}

// After an encode launch of the batch's blocks [b0, b0 + nb): one lane per item with blocks in the launch, items [i0, i0 + ni),
// writes the item's frames into the caller's range for it (batch_item_frames; the planner has left room for the header and a minimal
// frame per block: out_cap >= 16 + 6 * n_blocks).  The item's size and the capacity check go out with its last block.
__global__ __launch_bounds__(256) void batch_pack_scan_kernel(const BatchItem* __restrict__ items, uint32_t i0, uint32_t ni, uint64_t b0,
                                                              uint32_t nb, const uint32_t* __restrict__ sizes, uint32_t ext,
                                                              uint8_t* __restrict__ out, uint64_t* __restrict__ run_at,
                                                              uint64_t* __restrict__ frame_at, uint64_t* __restrict__ d_sizes,
                                                              int32_t* __restrict__ status)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= ni) return;
    const uint32_t i = i0 + j;
    const BatchItem it = items[i];
    const uint64_t at = batch_item_frames(it, run_at + i, b0, nb, sizes, ext, out, it.out_at, it.out_at + it.out_cap, frame_at);
    run_at[i] = at;
    if (it.first_block + it.n_blocks <= b0 + nb) {
        d_sizes[i] = at;
        if (at > it.out_cap) atomicMax(status, kErrOverflow);
    }
}

constexpr uint32_t kPackScanBlocks = 1024;    // the most blocks of one encode launch that the scan takes (the chip's 2 x CUs is 512)

// The pack scan of a packed batch (tsqa_compress_batch_packed*, the split forms and the calls from device tables, at every block
// length): the items' places are made here, not taken from the caller.  Item i starts at offsets[i]; offsets[i + 1] =
// round_up(offsets[i] + sizes[i], align), the last without the rounding.  ONE workgroup per encode launch: a launch holds at most
// 2 x CUs blocks, hence at most 2 x CUs + 1 items with blocks, and every one of them but the last is complete in it, so their starts
// are offsets[i0] + an exclusive sum of round_up(size, align) over the launch's items (offsets[i] is a multiple of align, so the
// rounding may be done per item).  offsets[] is the carry between launches: the first launch writes offsets[0] = 0, an item that a
// launch completes writes its successor's start, and the next launch reads offsets[i0] whether its first item continues (its
// start) or begins there (what the last complete item left).  sizes[] and offsets[] are complete whatever fits.
// item_status == NULL: the batch planned on the host, one word: the places only grow, so the last item tells whether the arena was
// too small.  Else (the batch made from device tables, whose window may also hold any number of items without blocks: they take
// no room) each item that ends past out_size gets kErrOverflow for itself.
//
// It runs after an encode launch of the batch's blocks [b0, b0 + nb) (block b in slot b - b0, nb <= kPackScanBlocks), whose items
// with blocks in it -- and, from device tables, the items without blocks among them -- are [i0, i0 + ni).  Exactly 256 threads,
// three steps, no lane ever walking an item's blocks: with blocks of TSQ_BLOCK_SZ an item rarely owns more than a few of a
// launch, with short blocks one item can own all 2 x CUs of them, behind an encode that lasts about as long as one 4 KiB chain.
//   1. E[0 .. nb] in LDS: the exclusive sum of (3 + sizes[k]) over the launch's blocks, 256 per pass.
//   2. One lane per item, 256 per pass: the item's bytes so far are carry + E[l] - E[f] for its blocks [f, l) of the launch,
//      carry = 16 where it begins in the launch (its header goes out here), else run_at[i], what its previous launch left.  The
//      same scan over round_up(size, align) of the items complete in the launch makes the starts.  Only the window's first item
//      can have begun in an earlier launch, so one word (carry0) keeps the carry that its lane has overwritten.
//   3. Behind a barrier, one lane per block: frame_at[k] = start + carry + E[k] - E[f] of its item block_item[b0 + k], whose start
//      is d_offsets[i]: the window's first item found it there, every other one had it written in step 2 by the lane of the item
//      in front of it (all but the window's last are complete).  Then the fit rule -- a header or frame is written only if it ends
//      at or before out_size --, write_frame or kNoFrame, and d_block_sizes[b0 + k] (may be NULL) = the stream length, whatever fits.
// max_stream: the longest stream the copy behind this kernel moves whole (its pieces are counted from block_bound(block_len)); a
// longer one -- the encoder never makes it -- is kErrOverflow in *status, not a silent cut.  All sums stay below 2^55.
__device__ __forceinline__ void batch_pack_scan_packed_body(const BatchItem* __restrict__ items, uint32_t n_items, uint32_t i0, uint32_t ni,
                                                            uint64_t b0, uint32_t nb, const uint32_t* __restrict__ sizes,
                                                            const uint32_t* __restrict__ block_item, uint32_t ext, uint32_t align,
                                                            uint32_t max_stream, uint8_t* __restrict__ out, uint64_t out_size,
                                                            uint64_t* __restrict__ run_at, uint64_t* __restrict__ frame_at, uint64_t* d_offsets,
                                                            uint64_t* __restrict__ d_sizes, uint32_t* __restrict__ d_block_sizes,
                                                            int32_t* __restrict__ item_status, int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ uint64_t E[kPackScanBlocks + 1];
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
// (tsqa_compress_batch_packed_async, tsqa_compress_batch_packed_split_async).
__global__ __launch_bounds__(256) void batch_pack_scan_packed_kernel(const BatchItem* __restrict__ items, uint32_t n_items, uint32_t i0, uint32_t ni,
                                                                     uint64_t b0, uint32_t nb, const uint32_t* __restrict__ sizes,
                                                                     const uint32_t* __restrict__ block_item, uint32_t ext, uint32_t align,
                                                                     uint32_t max_stream, uint8_t* __restrict__ out, uint64_t out_size,
                                                                     uint64_t* __restrict__ run_at, uint64_t* __restrict__ frame_at,
                                                                     uint64_t* d_offsets, uint64_t* __restrict__ d_sizes,
                                                                     uint32_t* __restrict__ d_block_sizes, int32_t* __restrict__ status)
{
    batch_pack_scan_packed_body(items, n_items, i0, ni, b0, nb, sizes, block_item, ext, align, max_stream, out, out_size, run_at, frame_at,
                                d_offsets, d_sizes, d_block_sizes, nullptr, status);
}

// The same behind launch l (blocks [l * budget, (l + 1) * budget) of the batch) of a batch whose item table was made on the device
// (tsqa_compress_batch_packed_tables_async and its split form): the launch's items are found here, not on the host.  The live blocks
// of the launch end at min((l + 1) * budget, *live_blocks); a launch past them has nothing to do and leaves, and the sizes and
// frame places of the dead blocks of a live launch are never looked at.  launch_item[l] (batch_enc_blocks_kernel) is the item that
// holds the launch's first block.  The items without blocks -- refused, or unfit for cap_blocks -- get their size 0 and carry
// offsets[] over them in the launch that completes the item with blocks in front of them: the window of launch l runs from the item
// that holds its first block (launch 0: from item 0, and launch 0 is never dead: a batch without a live block has its tables
// written there) to the item that holds the first block behind the launch, that item included only if it starts inside the
// launch; behind the last live block it runs to the end of the table.  So the windows of the live launches cover every item, and
// an item is complete in exactly one of them.  A fitting item that ends past out_size: item_status[i] = kErrOverflow.
__global__ __launch_bounds__(256) void batch_pack_scan_tables_kernel(const BatchItem* __restrict__ items, uint32_t n_items,
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
    batch_pack_scan_packed_body(items, n_items, i0, i1 - i0, b0, (uint32_t)(end - b0), sizes, block_item, ext, align, max_stream, out, out_size,
                                run_at, frame_at, d_offsets, d_sizes, d_block_sizes, item_status, status);
}

// Before batch_walk_kernel in the packed decompress calls: one lane per item takes its container's place from tables in
// device memory (what batch_pack_scan_packed_kernel wrote, or anything else: they are not trusted).  A place that does not lie
// inside the arena, or that is too short for a header or for the item's block count, becomes an empty input range, which
// batch_walk_kernel refuses (kErrFormat, d_sizes[i] = 0) without reading a byte of it.
__global__ __launch_bounds__(256) void batch_place_kernel(BatchItem* __restrict__ items, uint32_t n_items,
                                                          const uint64_t* __restrict__ d_offsets, const uint64_t* __restrict__ d_sizes,
                                                          uint64_t arena_size)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const uint64_t at = d_offsets[i], n = d_sizes[i];
    const bool ok = n <= arena_size && at <= arena_size - n && n >= kHeaderSize && items[i].n_blocks <= (n - kHeaderSize) / kMinFrameSize;
    items[i].in_at = ok ? at : 0ull;
    items[i].in_len = ok ? n : 0ull;
}

// First kernel of tsqa_decompress_batch_packed_dense_async, which takes nothing about the items from the host: one lane per item
// makes the item's descriptor from the 16 header bytes in the arena.  The place is checked as batch_place_kernel checks it and the
// header with read_header, whose limits are the host planner's (count >= 1, count <= (size - 16) / 6, total <= count * TSQ_BLOCK_SZ);
// only the header of a well-placed item is read.  An accepted item gets in_at, in_len, n_blocks and out_cap = its total, and status
// 0; a refused one an empty input range, no blocks and kErrFormat.  out_at and first_block are batch_layout_kernel's.
__global__ __launch_bounds__(256) void batch_measure_kernel(const uint8_t* __restrict__ in, BatchItem* __restrict__ items, uint32_t n_items,
                                                            const uint64_t* __restrict__ d_offsets, const uint64_t* __restrict__ d_sizes,
                                                            uint64_t arena_size, int32_t* __restrict__ item_status)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const uint64_t at = d_offsets[i], n = d_sizes[i];
    uint32_t nb = 0;
    uint64_t total = 0;
    const bool ok = n <= arena_size && at <= arena_size - n && n >= kHeaderSize && read_header(in + at, n, &nb, &total) == kHeaderOk;
    items[i] = ok ? BatchItem{at, n, 0, total, 0, nb, 0u} : BatchItem{0, 0, 0, 0, 0, 0u, 0u};
    item_status[i] = ok ? kOk : kErrFormat;
}

constexpr uint64_t kDenseRoomMax = 1ull << 48;  // batch_layout_kernel looks at no more of out_size: sums of fitting items stay far below 2^55

// Behind batch_measure_kernel: the places of a dense output, made from the measured totals and block counts.  ONE workgroup of
// exactly 256 threads walks the items 256 at a time, as batch_pack_scan_packed_kernel does, with two group_scan_excl64 sums per pass
// -- block counts, and round_up(total, align): every start is a multiple of align, so the rounding may be done per item -- and
// carries both between passes.  A refused item counts as no blocks and no bytes.  The public tables follow tsqa_plan_dense and are
// complete whatever fits:
//   first_block[i + 1] = first_block[i] + blocks_i;  out_offsets[i + 1] = round_up(out_offsets[i] + total_i, align), the last not rounded.
// An accepted item fits when first_block[i] + blocks_i <= cap_blocks and out_offsets[i] + total_i <= out_size.  Both sums only grow,
// so the fitting items are a prefix of the accepted ones, and the kernel holds on to that: the first item that does not fit
// (first_unfit) ends the prefix whatever the sums behind it say, so the sums that a verdict rests on are sums of items that fit --
// at most cap_blocks blocks and kDenseRoomMax bytes -- and cannot wrap, whatever the headers claim.  An item that does not fit gets
// kErrOverflow, an empty input range and no blocks (unfit = 1 keeps that verdict through the walk), so nothing of it is read or
// written.  *live_blocks = the blocks of the fitting prefix: dec_item_kernel's workgroups at or past it leave at once.
// status != NULL (the measure-only call, which runs nothing behind this kernel): *status = the largest item status.
__global__ __launch_bounds__(256) void batch_layout_kernel(BatchItem* __restrict__ items, uint32_t n_items, uint32_t align, uint64_t out_size,
                                                           uint32_t cap_blocks, uint64_t* __restrict__ d_out_offsets,
                                                           uint64_t* __restrict__ d_out_sizes, uint64_t* __restrict__ d_first_block,
                                                           int32_t* __restrict__ item_status, uint32_t* __restrict__ live_blocks,
                                                           int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ uint32_t first_unfit, live;
    const uint64_t mask = (uint64_t)align - 1u, room = out_size < kDenseRoomMax ? out_size : kDenseRoomMax;
    if (threadIdx.x == 0) { first_unfit = ~0u; live = 0u; d_out_offsets[0] = 0; d_first_block[0] = 0; }
    uint64_t block_base = 0, out_base = 0;
    for (uint64_t i0 = 0; i0 < n_items; i0 += 256u) {
        const uint64_t i = i0 + threadIdx.x;
        const bool valid = i < n_items;
        uint64_t total = 0;
        uint32_t nb = 0;
        int32_t st = kOk;
        if (valid) { nb = items[i].n_blocks; total = items[i].out_cap; st = item_status[i]; }
        const uint64_t padded = (total + mask) & ~mask;
        uint64_t sum;
        const uint64_t first = block_base + group_scan_excl64(nb, wave_sum, &sum);
        block_base += sum;
        const uint64_t at = out_base + group_scan_excl64(padded, wave_sum, &sum);
        out_base += sum;
        const bool accepted = valid && st == kOk;
        const bool fits = accepted && first + nb <= cap_blocks && at <= room && total <= room - at;
        if (accepted && !fits) atomicMin(&first_unfit, (uint32_t)i);
        __syncthreads();                                     // (no lane leaves the loop early: the scans and this barrier need them all)
        if (valid) {
            const bool fit = fits && i < first_unfit, over = accepted && !fit;
            if (fit) { items[i].out_at = at; items[i].first_block = first; atomicMax(&live, (uint32_t)(first + nb)); }
            else items[i] = BatchItem{0, 0, 0, 0, 0, 0u, over ? 1u : 0u};
            if (over) item_status[i] = kErrOverflow;
            if (status && !fit) atomicMax(status, over ? kErrOverflow : st);
            d_out_sizes[i] = fit ? total : 0ull;
            d_out_offsets[i + 1u] = at + (i + 1u == n_items ? total : padded);
            d_first_block[i + 1u] = first + nb;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *live_blocks = live;
}

// First kernel of tsqa_compress_batch_packed_tables_async, which reads the items' places from tables in device memory: one lane per
// item.  The tables are not trusted: an item must have at least one byte and lie inside the input (tsqa_plan_batch's checks, which
// cost the whole call there and the item here), and its blocks of 2^block_shift bytes (22: TSQ_BLOCK_SZ; less: the split form) must
// be counted in 32 bits.  An accepted item gets in_at, in_len, its block count and status 0; a refused one is all zeros and
// kErrArg, and not one byte of it is read.  first_block is batch_layout_tables_kernel's.
__global__ __launch_bounds__(256) void batch_measure_tables_kernel(BatchItem* __restrict__ items, uint32_t n_items,
                                                                   const uint64_t* __restrict__ d_in_offsets,
                                                                   const uint64_t* __restrict__ d_in_sizes, uint64_t in_size,
                                                                   uint32_t block_shift, int32_t* __restrict__ item_status)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const uint64_t at = d_in_offsets[i], n = d_in_sizes[i];
    // (in_size <= 2^48, the call's own limit: at most 2^26 blocks of TSQ_BLOCK_SZ per item, at most 2^36 of 4 KiB)
    const uint64_t nb = (n >> block_shift) + ((n & (((uint64_t)1 << block_shift) - 1u)) != 0u);
    const bool ok = n >= 1u && n <= in_size && at <= in_size - n && nb <= 0xFFFFFFFFull;
    items[i] = ok ? BatchItem{at, n, 0, 0, 0, (uint32_t)nb, 0u} : BatchItem{0, 0, 0, 0, 0, 0u, 0u};
    item_status[i] = ok ? kOk : kErrArg;
}

// Behind batch_measure_tables_kernel: batch_layout_kernel for a compress, whose arena places exist only once the sizes do.  ONE
// workgroup of exactly 256 threads, the same two sums per pass with both carries: block counts, and round_up(split_bound(in_len,
// 2^block_shift), align) of the accepted items (block_shift 22: batch_bound) -- *d_bound (may be NULL), the room that always holds
// the arena; a refused item adds nothing to either, so a lying size cannot inflate them.  first_block[i + 1] = first_block[i] +
// blocks_i is complete whatever fits.  An accepted item fits when first_block[i] + blocks_i <= cap_blocks; the fitting items are a
// prefix of the accepted ones, held as batch_layout_kernel holds it (first_unfit), so a verdict rests on a sum of at most
// cap_blocks; the whole block sum stays below 2^64 (fewer than 2^32 items of fewer than 2^32 blocks each; 2^59 with blocks of
// TSQ_BLOCK_SZ) and cannot wrap.  An item that does not fit gets kErrOverflow and becomes all zeros: nothing of it is read.
// *live_blocks = the blocks of the fitting prefix; *status (zero before) = the largest verdict given here.
// d_offsets != NULL: the measure-only call, which runs nothing behind this kernel (cap_blocks is 0: nothing fits): d_offsets and
// d_sizes are written, all 0.
__global__ __launch_bounds__(256) void batch_layout_tables_kernel(BatchItem* __restrict__ items, uint32_t n_items, uint32_t align,
                                                                  uint32_t block_shift, uint32_t cap_blocks,
                                                                  uint64_t* __restrict__ d_offsets, uint64_t* __restrict__ d_sizes,
                                                                  uint64_t* __restrict__ d_first_block,
                                                                  uint64_t* __restrict__ d_bound, int32_t* __restrict__ item_status,
                                                                  uint32_t* __restrict__ live_blocks, int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ uint32_t first_unfit, live;
    const uint64_t mask = (uint64_t)align - 1u, in_block = ((uint64_t)1 << block_shift) - 1u;
    if (threadIdx.x == 0) { first_unfit = ~0u; live = 0u; d_first_block[0] = 0; if (d_offsets) d_offsets[0] = 0; }
    uint64_t block_base = 0, bound_base = 0;
    for (uint64_t i0 = 0; i0 < n_items; i0 += 256u) {
        const uint64_t i = i0 + threadIdx.x;
        const bool valid = i < n_items;
        uint64_t len = 0;
        uint32_t nb = 0;
        int32_t st = kOk;
        if (valid) { nb = items[i].n_blocks; len = items[i].in_len; st = item_status[i]; }
        const bool accepted = valid && st == kOk;
        uint64_t sum;
        const uint64_t first = block_base + group_scan_excl64(nb, wave_sum, &sum);
        block_base += sum;
        // (split_bound(len, 2^block_shift), its division a shift)
        const uint64_t rest = len & in_block;
        const uint64_t room = kHeaderSize + (len >> block_shift) * block_bound(in_block + 1u) + (rest ? block_bound(rest) : 0ull);
        group_scan_excl64(accepted ? (room + mask) & ~mask : 0ull, wave_sum, &sum);
        bound_base += sum;
        const bool fits = accepted && first + nb <= cap_blocks;
        if (accepted && !fits) atomicMin(&first_unfit, (uint32_t)i);
        __syncthreads();                                     // (no lane leaves the loop early: the scans and this barrier need them all)
        if (valid) {
            const bool fit = fits && i < first_unfit, over = accepted && !fit;
            if (fit) { items[i].first_block = first; atomicMax(&live, (uint32_t)(first + nb)); }
            else items[i] = BatchItem{0, 0, 0, 0, 0, 0u, over ? 1u : 0u};
            if (over) item_status[i] = kErrOverflow;
            if (!fit) atomicMax(status, over ? kErrOverflow : st);
            if (d_offsets) { d_sizes[i] = 0; d_offsets[i + 1u] = 0; }
            d_first_block[i + 1u] = first + nb;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) { *live_blocks = live; if (d_bound) *d_bound = bound_base; }
}

// Behind batch_layout_tables_kernel: one lane per live block b makes its EncBatchBlock, in slot b % budget of its launch: the
// block_len bytes of its item from (b - first_block) * block_len on, or what is left of the item, and the look-ahead ends with the
// item.  The block's item is the last one whose first_block is at or below b (the items without blocks in front of it share its
// first_block; the ones behind it, and every unfit item, start past b), found by bisection in d_first_block; launch_item[l] = the
// item that holds block l * budget, for batch_pack_scan_tables_kernel; block_item[b] = the block's item, for step 3 of the pack
// scan (batch_pack_scan_packed_body).  Lanes at or past *live_blocks leave: the descriptors and table entries of
// dead blocks are never written and never read.
__global__ __launch_bounds__(256) void batch_enc_blocks_kernel(const BatchItem* __restrict__ items, uint32_t n_items,
                                                               const uint64_t* __restrict__ d_first_block,
                                                               const uint32_t* __restrict__ live_blocks, uint32_t budget, uint32_t block_len,
                                                               EncBatchBlock* __restrict__ blocks, uint32_t* __restrict__ launch_item,
                                                               uint32_t* __restrict__ block_item)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= *live_blocks) return;
    uint32_t lo = 0, hi = n_items;                           // first_block[lo] <= b < first_block[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (d_first_block[mid] <= b) lo = mid; else hi = mid;
    }
    const BatchItem it = items[lo];
    const uint64_t off = (b - it.first_block) * block_len, left = it.in_len - off;
    blocks[b] = EncBatchBlock{it.in_at + off, left, left < block_len ? (uint32_t)left : block_len, (uint32_t)(b % budget)};
    if (b % budget == 0u) launch_item[b / budget] = lo;
    if (block_item) block_item[b] = lo;
}

// Each block stream of the launch from its slot to its frame (pack_copy_piece); the blocks of items that did not fit are skipped.
// grid = (pieces, blocks of the launch).  live_blocks != NULL (the batch made from device tables, its launch sized by cap_blocks;
// b0: the launch's first block in the batch): a block at or past *live_blocks was never encoded, and its size and frame place are
// stale: not read.
__global__ __launch_bounds__(256) void batch_pack_copy_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                              const uint64_t* __restrict__ frame_at, uint8_t* __restrict__ out,
                                                              uint32_t b0, const uint32_t* __restrict__ live_blocks)
{
    const uint32_t b = blockIdx.y;
    if (live_blocks && b0 + b >= *live_blocks) return;
    const uint32_t size = sizes[b];
    const uint32_t piece_at = blockIdx.x * kPackPiece;
    const uint64_t at = frame_at[b];
    if (piece_at >= size || at == kNoFrame) return;
    pack_copy_piece(slots + (size_t)b * kSlotSize, size, out + at + kFrameWordSize, piece_at);
}

constexpr uint64_t kItemRefused = ~0ull;  // sizes[i] of an item whose container batch_walk_kernel<kWalkIndex> refuses

// What batch_walk_kernel checks besides the walk, and where a refusal goes:
//   kWalkOneWord  tsqa_decompress_batch_async: the total against the item's capacity; *status = kErrFormat, sizes[i] = 0.
//   kWalkPerItem  tsqa_decompress_batch_items_async and the dense call: the same checks; status[i] = kErrFormat, or kErrOverflow for
//                 an item that batch_layout_kernel found no room for (unfit, an empty input range); sizes[i] = 0.  Every block of
//                 every item learns its owner first: owner[first_block_i + k] = i, for a refused item too -- its workgroups are
//                 launched like the others and find their item's word through the table in order to leave (dec_item_kernel).
//                 status[] is zero before the kernel runs, apart from the verdicts of the dense call's own kernels, which it repeats.
//   kWalkIndex    tsqa_index_create_batch: no capacity; n_blocks is the count the item's header states (0: the host has refused the
//                 header already); sizes[i] = kItemRefused (its descriptors are then not to be used), status is not used.
//   kWalkJoin     tsqa_join_async (tsq_join.cuh): no capacity; sizes[i] = the item's frame bytes, from its start to the end of its
//                 last frame (what lies behind that is legal and is not part of the join), 0 for a refused item; status[i] as
//                 kWalkPerItem, behind the verdicts of the join's own kernels; no owners.
enum BatchWalkMode : int { kWalkOneWord, kWalkPerItem, kWalkIndex, kWalkJoin };

// One lane per item of a batch: the item's container is walked and validated as frame_walk_kernel walks one (the header, its block
// count against the caller's -- a count of 0 is refused in every mode, as no header states it --, the mode's checks, walk_frames).
// Frame k of item i lands at frames[first_block_i + k], stream_at relative to the batch's input, out_at to its output (kWalkIndex:
// the item's out_at is its start in the concatenation of the items' data).  sizes[i] = the item's total when it passes; a refused
// item gets the mode's verdict and descriptors with no stream, which every decoder refuses.
template <BatchWalkMode M>
__global__ __launch_bounds__(256) void batch_walk_kernel(const uint8_t* __restrict__ in, const BatchItem* __restrict__ items, uint32_t n_items,
                                                         FrameInfo* __restrict__ frames, uint32_t* __restrict__ owner,
                                                         uint64_t* __restrict__ sizes, int32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const BatchItem it = items[i];
    const uint8_t* const c = in + it.in_at;
    FrameInfo* const fr = frames + it.first_block;
    if constexpr (M == kWalkPerItem) for (uint32_t b = 0; b < it.n_blocks; ++b) owner[it.first_block + b] = i;
    uint32_t nb = 0;
    uint64_t total = 0, end = kHeaderSize;
    const bool ok = it.n_blocks != 0u && read_header(c, it.in_len, &nb, &total) == kHeaderOk && nb == it.n_blocks &&
                    (M == kWalkIndex || M == kWalkJoin || total <= it.out_cap) &&
                    walk_frames(c, it.in_len, nb, total, [&](uint32_t b, uint64_t, FrameInfo f) {
                        if constexpr (M == kWalkJoin) end = f.stream_at + f.stream_len;
                        f.stream_at += it.in_at; f.out_at += it.out_at;
                        fr[b] = f;
                        return true;
                    }) == kWalkOk;
    sizes[i] = ok ? (M == kWalkJoin ? end : total) : M == kWalkIndex ? kItemRefused : 0ull;
    if (ok) return;
    for (uint32_t b = 0; b < it.n_blocks; ++b) fr[b] = FrameInfo{0, 0, 0, 0, 0, 0};
    if constexpr (M == kWalkOneWord) atomicMax(status, kErrFormat);
    if constexpr (M == kWalkPerItem || M == kWalkJoin) status[i] = it.unfit ? kErrOverflow : kErrFormat;
}

// Behind the decode with a verdict per item, one lane per item: an item that the walk or a decoder refused gives no size, and the
// batch's word is the largest item status.  No other kernel of that path writes *status.
__global__ __launch_bounds__(256) void batch_close_items_kernel(uint32_t n_items, const int32_t* __restrict__ item_status,
                                                                uint64_t* __restrict__ d_sizes, int32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const int32_t st = item_status[i];
    if (st == 0) return;
    d_sizes[i] = 0;
    atomicMax(status, st);
}

// The first 16 bytes of every item's container, zeros past a short one: the synchronous batch decompress reads every header with
// one copy.  One thread per byte.
__global__ __launch_bounds__(256) void batch_heads_kernel(const uint8_t* __restrict__ in, const BatchItem* __restrict__ items, uint32_t n_items,
                                                          uint8_t* __restrict__ heads)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, i = t / kHeaderSize, k = t % kHeaderSize;
    if (i >= n_items) return;
    const BatchItem it = items[i];
    heads[t] = k < it.in_len ? in[it.in_at + k] : (uint8_t)0;
}

}  // namespace tsq
