// tsq_index_packed.cuh -- the index of a packed batch, made from the arena and its tables in device memory with nothing read back
// (tsqa_index_create_packed_async): what tsqa_index_create_batch does with two waits and a host pass in between.  The launches, in
// order, behind batch_measure_kernel (tsq_batch.cuh):
//   pidx_tables_kernel       (sized form) each accepted item's words of the caller's size table, and its geometry
//   join_blocks_kernel       the block prefix and the items that fit cap_blocks (tsq_join.cuh)
//   the walk                 provisional descriptors in the context's scratch, at the places join_blocks_kernel made:
//       plain form           batch_walk_kernel<kWalkIndex>: one lane per item
//       sized form           pidx_sum_kernel, pidx_scan_kernel, pidx_place_kernel, pidx_check_kernel: one lane per block
//   pidx_close_kernel        the items the walk refused leave gaps: the healthy items' blocks and totals are summed again
//   pidx_move_kernel         the healthy items' descriptors behind each other in the index's own table, out_at in the concatenation
// Each reads what the ones before it leave.  Nothing in the tables or the arena is trusted.
#pragma once

#include "tsq_batch.cuh"
#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"
#include "tsq_split.cuh"

namespace tsq {

constexpr uint32_t kPidxGroup = 256;                         // blocks per workgroup of the sized walk, groups per pass of its scan
constexpr uint32_t kNoOwner = ~0u;                           // owner[b] of a provisional block that no fitting item holds

// The words the index keeps beside its tables: [0] the healthy items' blocks, [1] the sum of their totals, [2] the blocks of all
// items whose header (and table) passed: the cap_blocks a retry needs.
constexpr uint32_t kPidxWords = 3;

// Sized form, behind batch_measure_kernel and in front of the fit: one lane per item.  Item i's words are table[table_first[i] ..
// table_first[i + 1]); the bounds must not decrease and must end inside table_words, else kErrArg.  The header must state as many
// blocks as the item has words, and its total must be what that many blocks of block_len hold with the last one not empty, else
// kErrFormat.  A refused item becomes all zeros, as one that batch_measure_kernel refused: it has no blocks and is never read.  An
// accepted one keeps its first word's place in out_at, which the sized walk has no other use for.
__global__ __launch_bounds__(256) void pidx_tables_kernel(BatchItem* __restrict__ items, uint32_t n_items, uint32_t block_len,
                                                          const uint64_t* __restrict__ table_first, uint64_t table_words,
                                                          int32_t* __restrict__ item_status)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_items || item_status[i] != kOk) return;
    const uint64_t w0 = table_first[i], w1 = table_first[i + 1u];
    const BatchItem it = items[i];
    int32_t st = kOk;
    if (w0 > w1 || w1 > table_words) st = kErrArg;
    else if (w1 - w0 != it.n_blocks || it.out_cap > (uint64_t)it.n_blocks * block_len ||
             it.out_cap + block_len <= (uint64_t)it.n_blocks * block_len) st = kErrFormat;
    if (st == kOk) { items[i].out_at = w0; return; }
    items[i] = BatchItem{0, 0, 0, 0, 0, 0u, 0u};
    item_status[i] = st;
}

// The item that holds provisional block b, or kNoOwner: the last item whose first block is at or below b (items without blocks in
// front of it share its first block), found by bisection in the prefix that join_blocks_kernel left, and then asked itself: an
// unfit item has become all zeros, and a block at or past the fitting prefix's end is past its candidate's last block.
__device__ __forceinline__ uint32_t pidx_owner_of(const BatchItem* __restrict__ items, uint32_t n_items, const uint64_t* __restrict__ first_block, uint64_t b)
{
    uint32_t lo = 0, hi = n_items;                           // first_block[lo] <= b < first_block[hi] wherever b has an owner
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (first_block[mid] <= b) lo = mid; else hi = mid;
    }
    const BatchItem it = items[lo];
    return it.n_blocks != 0u && b >= it.first_block && b - it.first_block < it.n_blocks ? lo : kNoOwner;
}

// What provisional block b adds to the places behind it, and whose it is.  The word is read only for a block that has an owner,
// at a place inside [0, table_words): pidx_tables_kernel has checked the item's bounds.  A word that stream_len_ok refuses counts
// as 0 and refuses its item in pidx_check_kernel, so no sum can wrap: at most 2^32 frames of less than 2^23 bytes.
__device__ __forceinline__ uint64_t pidx_frame_room(const BatchItem* __restrict__ items, uint32_t owner, uint64_t b, const uint32_t* __restrict__ table,
                                                    uint32_t* s_out, bool* s_ok)
{
    *s_out = 0u; *s_ok = false;
    if (owner == kNoOwner) return 0ull;
    const uint32_t s = table[items[owner].out_at + (b - items[owner].first_block)];
    *s_out = s; *s_ok = stream_len_ok(s);
    return *s_ok ? kFrameWordSize + (uint64_t)s : 0ull;
}

// Sized walk, launch 1.  Workgroup g of exactly 256 threads: each lane finds its block's owner (kept for the launches behind) and
// group_sum[g] = the room of the frames [256 g, 256 g + 256) of the whole batch.
__global__ __launch_bounds__(256) void pidx_sum_kernel(const BatchItem* __restrict__ items, uint32_t n_items, const uint64_t* __restrict__ first_block,
                                                       uint32_t cap_blocks, const uint32_t* __restrict__ table, uint32_t* __restrict__ owner,
                                                       uint64_t* __restrict__ group_sum)
{
    __shared__ uint64_t wave_sum[4];
    const uint64_t b = (uint64_t)blockIdx.x * kPidxGroup + threadIdx.x;
    uint32_t own = kNoOwner, s;
    bool s_ok;
    if (b < cap_blocks) { own = pidx_owner_of(items, n_items, first_block, b); owner[b] = own; }
    uint64_t sum;
    (void)group_scan_excl64(pidx_frame_room(items, own, b, table, &s, &s_ok), wave_sum, &sum);
    if (threadIdx.x == 0u) group_sum[blockIdx.x] = sum;
}

// Sized walk, launch 2.  ONE workgroup of exactly 256 threads: group_sum[g] becomes the sum of the groups before g, 256 groups per
// pass with the running sum carried in a register (index_scan_kernel's scan, tsq_index.cuh, without a header to check).
__global__ __launch_bounds__(256) void pidx_scan_kernel(uint64_t* __restrict__ group_sum, uint32_t n_groups)
{
    __shared__ uint64_t wave_sum[4];
    uint64_t base = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += kPidxGroup) { // (no thread leaves the loop early: the scan needs them all; n_groups <= 2^24)
        const uint32_t g = g0 + threadIdx.x;
        const bool valid = g < n_groups;
        uint64_t sum;
        const uint64_t before = base + group_scan_excl64(valid ? group_sum[g] : 0ull, wave_sum, &sum);
        base += sum;
        if (valid) group_sum[g] = before;
    }
}

// Sized walk, launch 3.  room_before[b] = the room of all the batch's frames in front of provisional block b: the group's base
// and the group's own scan.  A frame's place inside its item is a difference of two of these (pidx_check_kernel), which is why
// this is a launch of its own: an item's first block may lie in another workgroup's group.
__global__ __launch_bounds__(256) void pidx_place_kernel(const BatchItem* __restrict__ items, const uint32_t* __restrict__ owner, uint32_t cap_blocks,
                                                         const uint32_t* __restrict__ table, const uint64_t* __restrict__ group_base,
                                                         uint64_t* __restrict__ room_before)
{
    __shared__ uint64_t wave_sum[4];
    const uint64_t b = (uint64_t)blockIdx.x * kPidxGroup + threadIdx.x;
    const bool valid = b < cap_blocks;
    uint32_t s;
    bool s_ok;
    uint64_t sum;
    const uint64_t at = group_base[blockIdx.x] + group_scan_excl64(pidx_frame_room(items, valid ? owner[b] : kNoOwner, b, table, &s, &s_ok), wave_sum, &sum);
    if (valid) room_before[b] = at;                          // (behind the scan, which needs every thread)
}

// Sized walk, launch 4.  One lane per provisional block.  Block j of item i lies at 16 + the room of the item's frames before it;
// sized_frame_ok there, against the item's own bytes (tsq_split.cuh: the six bytes inside the item before one is read, read_frame,
// the frame word's length the table's); and the geometry: out_len is block_len, or for the item's last block what the header's
// total leaves.  A frame that passes gets the descriptor batch_walk_kernel<kWalkIndex> makes for it with the item's data starting
// at 0; one that does not gets a descriptor with no stream and refuses its item alone.
__global__ __launch_bounds__(256) void pidx_check_kernel(const uint8_t* __restrict__ in, const BatchItem* __restrict__ items,
                                                         const uint32_t* __restrict__ owner, uint32_t cap_blocks, uint32_t block_len,
                                                         const uint32_t* __restrict__ table, const uint64_t* __restrict__ room_before,
                                                         FrameInfo* __restrict__ frames, int32_t* __restrict__ item_status)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= cap_blocks) return;
    const uint32_t own = owner[b];
    if (own == kNoOwner) return;
    const BatchItem it = items[own];
    const uint64_t j = b - it.first_block;
    uint32_t s;
    bool s_ok;
    (void)pidx_frame_room(items, own, b, table, &s, &s_ok);
    const uint64_t at = kHeaderSize + (room_before[b] - room_before[it.first_block]);
    const uint64_t out_at = j * block_len;
    const uint64_t want_len = j + 1u < it.n_blocks ? (uint64_t)block_len : it.out_cap - out_at;
    FrameInfo f{0, 0, 0, 0, 0, 0};
    if (sized_frame_ok(in + it.in_at, it.in_len, at, s_ok, s, &f) && f.out_len == want_len) {
        f.stream_at = it.in_at + at + kFrameWordSize; f.out_at = out_at;
        frames[b] = f;
    } else {
        frames[b] = FrameInfo{0, 0, 0, 0, 0, 0};
        atomicMax(item_status + own, kErrFormat);
    }
}

// Behind the walk: ONE workgroup of exactly 256 threads, 256 items per pass, two sums carried: the blocks and the totals of the
// healthy items only -- status 0 and, in the plain form (walked != NULL), not kItemRefused by the walk, which costs the item
// kErrFormat here.  item_first[i] = the healthy items' blocks before item i (n_items + 1 entries: a refused or unfit item owns
// none), item_at[i] = where item i's data starts in the concatenation, words = {blocks, total, the blocks of all accepted items:
// what join_blocks_kernel's prefix ends at}, *status = the largest item status; out_status (may be NULL): a copy of the verdicts
// for the caller.  The sums are of items that fit cap_blocks: fewer than 2^32 blocks and 2^54 bytes.
__global__ __launch_bounds__(256) void pidx_close_kernel(const BatchItem* __restrict__ items, uint32_t n_items, const uint64_t* __restrict__ walked,
                                                         const uint64_t* __restrict__ first_block, int32_t* __restrict__ item_status,
                                                         int32_t* __restrict__ out_status, uint64_t* __restrict__ item_first,
                                                         uint64_t* __restrict__ item_at, uint64_t* __restrict__ words, int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ int32_t worst;
    if (threadIdx.x == 0) worst = kOk;
    uint64_t block_base = 0, at_base = 0;
    for (uint64_t i0 = 0; i0 < n_items; i0 += 256u) {        // (no lane leaves the loop early: the scans need them all)
        const uint64_t i = i0 + threadIdx.x;
        const bool valid = i < n_items;
        int32_t st = valid ? item_status[i] : kOk;
        if (valid && st == kOk && walked && walked[i] == kItemRefused) st = kErrFormat;
        const bool healthy = valid && st == kOk;
        const uint32_t nb = healthy ? items[i].n_blocks : 0u;
        const uint64_t total = healthy ? items[i].out_cap : 0ull;
        uint64_t sum;
        const uint64_t first = block_base + group_scan_excl64(nb, wave_sum, &sum);
        block_base += sum;
        const uint64_t at = at_base + group_scan_excl64(total, wave_sum, &sum);
        at_base += sum;
        if (valid) {
            item_first[i] = first; item_at[i] = at;
            item_status[i] = st;
            if (out_status) out_status[i] = st;
            if (st != kOk) atomicMax(&worst, st);
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    item_first[n_items] = block_base;
    words[0] = block_base; words[1] = at_base; words[2] = first_block[n_items];
    *status = worst;
}

// Behind pidx_close_kernel, one lane per descriptor of the index, cap_blocks of them.  Below the healthy items' block count: the
// block's item is the last one whose item_first is at or below it (a refused item in front of it shares that entry and owns
// nothing), and its descriptor is the provisional one of the same block of that item, out_at moved to the item's start in the
// concatenation.  From there on: out_at = the total and everything else zero, so that a bisection over all cap_blocks descriptors
// (gather_block_of) finds what it finds over the live ones.
__global__ __launch_bounds__(256) void pidx_move_kernel(const BatchItem* __restrict__ items, uint32_t n_items, const FrameInfo* __restrict__ walked,
                                                        const uint64_t* __restrict__ item_first, const uint64_t* __restrict__ item_at,
                                                        const uint64_t* __restrict__ words, uint32_t cap_blocks, FrameInfo* __restrict__ frames)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= cap_blocks) return;
    if (b >= words[0]) { frames[b] = FrameInfo{0, words[1], 0, 0, 0, 0}; return; }
    uint32_t lo = 0, hi = n_items;                           // item_first[lo] <= b < item_first[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (item_first[mid] <= b) lo = mid; else hi = mid;
    }
    FrameInfo f = walked[items[lo].first_block + (b - item_first[lo])];
    f.out_at += item_at[lo];
    frames[b] = f;
}

}  // namespace tsq
