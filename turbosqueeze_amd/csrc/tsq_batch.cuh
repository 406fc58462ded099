// tsq_batch.cuh -- batches of independent items (tsqa_compress_batch*, tsqa_decompress_batch*): the container pack across encode
// launches, the frame walk and the header gather.  The container format itself: tsq_format.h.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"

namespace tsq {

// One item of a batch as the kernels see it, planned on the host (tsqa_plan_batch): its input and output ranges, relative to the
// batch's input and output, its first block in the batch and its block count.  The dense decompress makes the table on the device
// (batch_measure_kernel, batch_layout_kernel); only there is pad used: 1 marks an item that did not fit the caller's room.
struct BatchItem { uint64_t in_at, in_len, out_at, out_cap, first_block; uint32_t n_blocks, pad; };

constexpr uint64_t kNoFrame = ~0ull;      // frame_at of a block whose frame does not fit its item: batch_pack_copy_kernel skips it

// After an encode launch of the batch's blocks [b0, b0 + nb) (block b in slot b - b0): one lane per item with blocks in the launch,
// items [i0, i0 + ni).  An item's frame offsets run on from where its previous launch left them (run_at[i]); its header goes out
// with its first block, its size and the capacity check with its last.  A frame is written only if it ends inside the item's
// capacity: frame_at[b - b0] is its offset in the output, or kNoFrame.
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
    const uint64_t first = it.first_block, end = first + it.n_blocks, launch_end = b0 + nb;
    uint8_t* const base = out + it.out_at;
    // (the planner has left room for the header and a minimal frame per block: out_cap >= 16 + 6 * n_blocks)
    if (first >= b0) write_header(base, it.n_blocks, it.in_len);
    uint64_t at = first >= b0 ? kHeaderSize : run_at[i];
    for (uint64_t b = first > b0 ? first : b0; b < end && b < launch_end; ++b) {
        const uint32_t k = (uint32_t)(b - b0), sz = sizes[k];
        const uint64_t next = at + kFrameWordSize + sz;
        if (next <= it.out_cap) { write_frame(base + at, sz, ext); frame_at[k] = it.out_at + at; }
        else frame_at[k] = kNoFrame;
        at = next;
    }
    run_at[i] = at;
    if (end <= launch_end) {
        d_sizes[i] = at;
        if (at > it.out_cap) atomicMax(status, kErrOverflow);
    }
}

// Exclusive sum of v over the 256 threads of a workgroup, for sums below 2^55 (a batch has at most 2^32 - 1 blocks, so every sum of
// container sizes is): two 32-bit DPP scans per wavefront, of the low 24 bits and of the rest, then the four wavefront totals through
// LDS.  *total = the workgroup's sum.  Every thread of the workgroup calls it (the DPP steps read the neighbouring lanes): the
// workgroup is exactly 256 threads, four full wavefronts, and wave_scan_add is an inclusive sum over 64 active lanes.
__device__ __forceinline__ uint64_t group_scan_excl64(uint64_t v, uint64_t* wave_sum /* LDS, 4 */, uint64_t* total)
{
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t incl = ((uint64_t)wave_scan_add((uint32_t)(v >> 24)) << 24) + wave_scan_add((uint32_t)v & 0xFFFFFFu);
    __syncthreads();                                         // (the previous call's totals have been read)
    if (lane == 63u) wave_sum[wid] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
    for (uint32_t w = 0; w < 4u; ++w) { const uint64_t s = wave_sum[w]; if (w < wid) before += s; all += s; }
    *total = all;
    return before + incl - v;
}

// batch_pack_scan_kernel for a packed batch (tsqa_compress_batch_packed*): the items' places are made here, not taken from the
// caller.  Item i starts at offsets[i]; offsets[i + 1] = round_up(offsets[i] + sizes[i], align), the last without the rounding.
// ONE workgroup per encode launch: a launch holds at most 2 x CUs blocks, hence at most 2 x CUs + 1 items, and every one of them
// but the last is complete in it, so their starts are offsets[i0] + an exclusive sum of round_up(size, align) over the launch's
// items (offsets[i] is a multiple of align, so the rounding may be done per item).  offsets[] is the carry between launches: the
// first launch writes offsets[0] = 0, an item that a launch completes writes its successor's start, and the next launch reads
// offsets[i0] whether its first item continues (its start) or begins there (what the last complete item left).  An item that
// continues keeps its running frame offset in run_at[i], as in batch_pack_scan_kernel.  A header or frame is written only if it ends
// inside out_size; sizes[] and offsets[] are complete whatever fits.
__global__ __launch_bounds__(256) void batch_pack_scan_packed_kernel(const BatchItem* __restrict__ items, uint32_t n_items, uint32_t i0,
                                                                     uint32_t ni, uint64_t b0, uint32_t nb,
                                                                     const uint32_t* __restrict__ sizes, uint32_t ext, uint32_t align,
                                                                     uint8_t* __restrict__ out, uint64_t out_size,
                                                                     uint64_t* __restrict__ run_at, uint64_t* __restrict__ frame_at,
                                                                     uint64_t* __restrict__ d_offsets, uint64_t* __restrict__ d_sizes,
                                                                     int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    const uint64_t launch_end = b0 + nb, mask = (uint64_t)align - 1u;
    uint64_t base = b0 == 0 ? 0ull : d_offsets[i0];          // where the launch's first item starts
    if (b0 == 0 && threadIdx.x == 0) d_offsets[0] = 0;
    for (uint32_t j0 = 0; j0 < ni; j0 += 256u) {
        const uint32_t j = j0 + threadIdx.x, i = i0 + (j < ni ? j : 0u);
        const bool valid = j < ni;
        uint64_t first = 0, end = 0, at0 = 0, at = 0, in_len = 0;
        uint32_t n_blocks = 0;
        if (valid) {
            const BatchItem it = items[i];
            first = it.first_block; end = first + it.n_blocks; in_len = it.in_len; n_blocks = it.n_blocks;
            at0 = at = first >= b0 ? kHeaderSize : run_at[i];
            for (uint64_t b = first > b0 ? first : b0; b < end && b < launch_end; ++b) at += kFrameWordSize + sizes[(uint32_t)(b - b0)];
        }
        const bool complete = valid && end <= launch_end;    // (only the launch's last item can be incomplete: it adds nothing)
        uint64_t total;
        const uint64_t start = base + group_scan_excl64(complete ? (at + mask) & ~mask : 0ull, wave_sum, &total);
        base += total;
        if (valid) {                                         // (no lane leaves the loop early: the scan above needs them all)
            if (first >= b0 && start + kHeaderSize <= out_size) write_header(out + start, n_blocks, in_len);
            uint64_t w = at0;
            for (uint64_t b = first > b0 ? first : b0; b < end && b < launch_end; ++b) {
                const uint32_t k = (uint32_t)(b - b0), sz = sizes[k];
                const uint64_t next = w + kFrameWordSize + sz;
                if (start + next <= out_size) { write_frame(out + start + w, sz, ext); frame_at[k] = start + w; }
                else frame_at[k] = kNoFrame;
                w = next;
            }
            run_at[i] = at;
        }
        if (complete) {
            const bool last = i + 1u == n_items;
            d_sizes[i] = at;
            d_offsets[i + 1u] = last ? start + at : start + ((at + mask) & ~mask);
            if (last && start + at > out_size) atomicMax(status, kErrOverflow);
        }
    }
}

// Before batch_walk_kernel in tsqa_decompress_batch_packed_async: one lane per item takes its container's place from tables in
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
// kErrOverflow, an empty input range and no blocks (pad = 1 marks it for batch_overflow_kernel), so nothing of it is read or
// written.  *live_blocks = the blocks of the fitting prefix: dec_dense_kernel's workgroups at or past it leave at once.
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

// Behind batch_walk_items_kernel in the dense call: the walk refuses every item with an empty input range as a malformed container,
// the items that did not fit among them; they get their own verdict back.
__global__ __launch_bounds__(256) void batch_overflow_kernel(const BatchItem* __restrict__ items, uint32_t n_items, int32_t* __restrict__ item_status)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    if (items[i].pad) item_status[i] = kErrOverflow;
}

// Each block stream of the launch from its slot to its frame (pack_copy_piece); the blocks of items that did not fit are skipped.
// grid = (pieces, blocks of the launch).
__global__ __launch_bounds__(256) void batch_pack_copy_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                              const uint64_t* __restrict__ frame_at, uint8_t* __restrict__ out)
{
    const uint32_t b = blockIdx.y;
    const uint32_t size = sizes[b];
    const uint32_t piece_at = blockIdx.x * kPackPiece;
    const uint64_t at = frame_at[b];
    if (piece_at >= size || at == kNoFrame) return;
    pack_copy_piece(slots + (size_t)b * kSlotSize, size, out + at + kFrameWordSize, piece_at);
}

// One lane per item of a decompress batch: the item's container is walked and validated as frame_walk_kernel walks one (the
// header, its block count against the caller's, its total against the item's capacity, every frame, lengths that add up to the
// total).  Frame k of item i lands at frames[first_block_i + k], stream_at relative to the batch's input, out_at to its output.
// A refused item gets d_sizes[i] = 0, *status kErrFormat, and descriptors with no stream, which every decoder refuses.
__global__ __launch_bounds__(256) void batch_walk_kernel(const uint8_t* __restrict__ in, const BatchItem* __restrict__ items, uint32_t n_items,
                                                         FrameInfo* __restrict__ frames, uint64_t* __restrict__ d_sizes,
                                                         int32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const BatchItem it = items[i];
    const uint8_t* const c = in + it.in_at;
    const uint64_t n = it.in_len;
    FrameInfo* const fr = frames + it.first_block;
    uint32_t nb = 0;
    uint64_t total = 0, at = kHeaderSize, oat = 0;
    bool bad = read_header(c, n, &nb, &total) != kHeaderOk || nb != it.n_blocks || total > it.out_cap;
    for (uint32_t b = 0; b < it.n_blocks && !bad; ++b) {
        FrameInfo f;
        if (at + kMinFrameSize > n || !read_frame(c + at, at, n, &f) || oat + f.out_len > total) { bad = true; break; }
        f.stream_at = it.in_at + at + kFrameWordSize; f.out_at = it.out_at + oat;
        fr[b] = f;
        oat += f.out_len;
        at += kFrameWordSize + f.stream_len;
    }
    if (!bad && oat != total) bad = true;
    d_sizes[i] = bad ? 0 : total;
    if (!bad) return;
    for (uint32_t b = 0; b < it.n_blocks; ++b) fr[b] = FrameInfo{0, 0, 0, 0, 0, 0};
    atomicMax(status, kErrFormat);
}

// batch_walk_kernel with a verdict per item (tsqa_decompress_batch_items_async): the same walk and the same validation, but a
// refusal goes to item_status[i] (kErrFormat) and not to a word of the batch, and every block of every item learns its owner:
// owner[first_block_i + k] = i, for a refused item too -- its workgroups are launched like the others and find their item's word
// through the table in order to leave (dec_item_kernel).  d_sizes[i] = the item's total, 0 when it is refused here; the closing
// kernel clears it for an item that a decoder refuses.  item_status is zero before this kernel runs and nothing else writes it yet.
__global__ __launch_bounds__(256) void batch_walk_items_kernel(const uint8_t* __restrict__ in, const BatchItem* __restrict__ items,
                                                               uint32_t n_items, FrameInfo* __restrict__ frames, uint32_t* __restrict__ owner,
                                                               uint64_t* __restrict__ d_sizes, int32_t* __restrict__ item_status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const BatchItem it = items[i];
    const uint8_t* const c = in + it.in_at;
    const uint64_t n = it.in_len;
    FrameInfo* const fr = frames + it.first_block;
    uint32_t* const own = owner + it.first_block;
    for (uint32_t b = 0; b < it.n_blocks; ++b) own[b] = i;
    uint32_t nb = 0;
    uint64_t total = 0, at = kHeaderSize, oat = 0;
    bool bad = read_header(c, n, &nb, &total) != kHeaderOk || nb != it.n_blocks || total > it.out_cap;
    for (uint32_t b = 0; b < it.n_blocks && !bad; ++b) {
        FrameInfo f;
        if (at + kMinFrameSize > n || !read_frame(c + at, at, n, &f) || oat + f.out_len > total) { bad = true; break; }
        f.stream_at = it.in_at + at + kFrameWordSize; f.out_at = it.out_at + oat;
        fr[b] = f;
        oat += f.out_len;
        at += kFrameWordSize + f.stream_len;
    }
    if (!bad && oat != total) bad = true;
    d_sizes[i] = bad ? 0 : total;
    if (!bad) return;
    for (uint32_t b = 0; b < it.n_blocks; ++b) fr[b] = FrameInfo{0, 0, 0, 0, 0, 0};
    item_status[i] = kErrFormat;
}

// Behind the decode of tsqa_decompress_batch_items_async, one lane per item: an item that the walk or a decoder refused gives no
// size, and the batch's word is the largest item status.  No other kernel of that path writes *status.
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

constexpr uint64_t kItemRefused = ~0ull;  // verdicts[i] of an item whose container batch_index_walk_kernel refuses

// One lane per item of a batch index (tsqa_index_create_batch): batch_walk_kernel's walk with a verdict per item instead of one
// for the batch, and no capacity.  n_blocks is the count the item's header states (0: the host has refused the header already);
// frame k of item i lands at frames[first_block_i + k], stream_at relative to the batch's input, out_at = the item's out_at (its
// start in the concatenation of the items' data) + the block's start in the item.  verdicts[i] = the item's total, or kItemRefused
// (its descriptors are then not to be used).
__global__ __launch_bounds__(256) void batch_index_walk_kernel(const uint8_t* __restrict__ in, const BatchItem* __restrict__ items, uint32_t n_items,
                                                               FrameInfo* __restrict__ frames, uint64_t* __restrict__ verdicts)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items) return;
    const BatchItem it = items[i];
    const uint8_t* const c = in + it.in_at;
    const uint64_t n = it.in_len;
    FrameInfo* const fr = frames + it.first_block;
    uint32_t nb = 0;
    uint64_t total = 0, at = kHeaderSize, oat = 0;
    bool bad = it.n_blocks == 0u || read_header(c, n, &nb, &total) != kHeaderOk || nb != it.n_blocks;
    for (uint32_t b = 0; b < it.n_blocks && !bad; ++b) {
        FrameInfo f;
        if (at + kMinFrameSize > n || !read_frame(c + at, at, n, &f) || oat + f.out_len > total) { bad = true; break; }
        f.stream_at = it.in_at + at + kFrameWordSize; f.out_at = it.out_at + oat;
        fr[b] = f;
        oat += f.out_len;
        at += kFrameWordSize + f.stream_len;
    }
    if (!bad && oat != total) bad = true;
    verdicts[i] = bad ? kItemRefused : total;
    if (bad) for (uint32_t b = 0; b < it.n_blocks; ++b) fr[b] = FrameInfo{0, 0, 0, 0, 0, 0};
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
