// tsq_join.cuh -- the join of device-resident containers into one container (tsqa_join_async): nothing is decoded, the frames of
// every item are copied behind one new header.  The launches, in order, behind batch_measure_kernel (tsq_batch.cuh):
//   join_blocks_kernel       the block prefix and the items that fit cap_blocks
//   batch_walk_kernel<kWalkJoin>   every fitting item walked as a reader walks it; leaves the item's frame bytes
//   join_bodies_kernel       the body places, the call's verdict and size, the header
//   join_emit_kernel         the copy, balanced over the output
//   join_block_sizes_kernel  the table of stream lengths, where asked for
// The last two read the verdict and leave when it is nonzero.  The container format itself: tsq_format.h.
#pragma once

#include "tsq_batch.cuh"
#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"

namespace tsq {

// Behind batch_measure_kernel: batch_layout_kernel's block sum without an output to place.  ONE workgroup of exactly 256 threads
// walks the items 256 at a time and carries the sum between passes.  first_block[i + 1] = first_block[i] + blocks_i is complete
// whatever fits; a refused item counts as no blocks.  An accepted item fits when first_block[i] + blocks_i <= cap_blocks; the
// fitting items are a prefix of the accepted ones, held as batch_layout_kernel holds it (first_unfit), so every sum a verdict rests
// on is at most cap_blocks.  An item that does not fit gets kErrOverflow and becomes all zeros with unfit = 1: the walk reads
// nothing of it and keeps that verdict.
__global__ __launch_bounds__(256) void join_blocks_kernel(BatchItem* __restrict__ items, uint32_t n_items, uint32_t cap_blocks,
                                                          uint64_t* __restrict__ d_first_block, int32_t* __restrict__ item_status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ uint32_t first_unfit;
    if (threadIdx.x == 0) { first_unfit = ~0u; d_first_block[0] = 0; }
    uint64_t block_base = 0;
    for (uint64_t i0 = 0; i0 < n_items; i0 += 256u) {
        const uint64_t i = i0 + threadIdx.x;
        const bool valid = i < n_items;
        uint32_t nb = 0;
        int32_t st = kOk;
        if (valid) { nb = items[i].n_blocks; st = item_status[i]; }
        uint64_t sum;
        const uint64_t first = block_base + group_scan_excl64(nb, wave_sum, &sum);
        block_base += sum;
        const bool accepted = valid && st == kOk;
        const bool fits = accepted && first + nb <= cap_blocks;
        if (accepted && !fits) atomicMin(&first_unfit, (uint32_t)i);
        __syncthreads();                                     // (no lane leaves the loop early: the scan and this barrier need them all)
        if (valid) {
            const bool fit = fits && i < first_unfit, over = accepted && !fit;
            if (fit) items[i].first_block = first;
            else items[i] = BatchItem{0, 0, 0, 0, 0, 0u, over ? 1u : 0u};
            if (over) item_status[i] = kErrOverflow;
            d_first_block[i + 1u] = first + nb;
        }
    }
}

// Behind the walk: the places of the bodies.  ONE workgroup of exactly 256 threads, 256 items per pass, two sums carried: the
// bodies (frame_bytes_i - 16, from 16 on: tsqa_plan_join's body_at) and the headers' totals.  Only items whose status is 0 count,
// and the call is all or nothing: *status = the largest item status; where that is 0, *out_size = body_at[n_items], kErrOverflow
// when it exceeds out_cap (measuring: out_cap 0), and otherwise the joined header is written.  In every other case *out_size = 0.
// The bodies of items that fit cap_blocks add up to less than 2^55 (at most 2^32 frames of 3 + TSQ_OUTPUT_SZ bytes), and so do
// their totals.
__global__ __launch_bounds__(256) void join_bodies_kernel(const BatchItem* __restrict__ items, uint32_t n_items,
                                                          const uint64_t* __restrict__ frame_bytes, const uint64_t* __restrict__ d_first_block,
                                                          const int32_t* __restrict__ item_status, uint8_t* __restrict__ out, uint64_t out_cap,
                                                          uint64_t* __restrict__ body_at, uint64_t* __restrict__ out_size,
                                                          int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ int32_t worst;
    if (threadIdx.x == 0) worst = kOk;
    uint64_t at = kHeaderSize, total = 0;
    for (uint64_t i0 = 0; i0 < n_items; i0 += 256u) {        // (no lane leaves the loop early: the scans need them all)
        const uint64_t i = i0 + threadIdx.x;
        const bool valid = i < n_items;
        const int32_t st = valid ? item_status[i] : kOk;
        const bool ok = valid && st == kOk;
        uint64_t sum;
        const uint64_t mine = at + group_scan_excl64(ok ? frame_bytes[i] - kHeaderSize : 0ull, wave_sum, &sum);
        at += sum;
        (void)group_scan_excl64(ok ? items[i].out_cap : 0ull, wave_sum, &sum);
        total += sum;
        if (valid) { body_at[i] = mine; if (st != kOk) atomicMax(&worst, st); }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    body_at[n_items] = at;
    int32_t st = worst;
    *out_size = st == kOk ? at : 0ull;
    if (st == kOk && at > out_cap) st = kErrOverflow;
    *status = st;
    if (st == kOk) write_header(out, (uint32_t)d_first_block[n_items], total);
}

// The item whose body holds byte o of the joined container: body_at[lo] <= o < body_at[hi].
__device__ __forceinline__ uint32_t join_item_of(const uint64_t* __restrict__ body_at, uint32_t lo, uint32_t hi, uint64_t o)
{
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (body_at[mid] <= o) lo = mid; else hi = mid;
    }
    return lo;
}

// The copy.  Its work is balanced over the output, not over the items: a workgroup takes one piece of kJoinPiece bytes of the
// joined container after the other (grid-stride; the host sizes the grid from out_cap and the chip), cut at multiples of 16 of the
// destination ADDRESS, so every full word of a piece is one aligned 16-byte store.  The item that holds the piece's first byte is
// found by bisection in body_at.  Where the piece lies inside one body it is copied as pack_copy_piece copies: an unaligned 16-byte
// load per destination word, four in flight per lane.  Elsewhere each word finds its own item between the piece's first and last:
// a word wholly inside one body takes the same load and store, a word across a seam -- a body may be 6 bytes, so a word can touch
// four items -- or cut by the header or the container's end goes byte by byte.  No 16-byte load runs past its body's end, and no
// byte outside an item's frames is read.  Bytes 0 .. 15 are join_bodies_kernel's.
constexpr uint32_t kJoinPiece = 16384;                       // 256 lanes x 4 words

// A lane's share of a piece whose every word is whole and of one body (also cut_emit_kernel's, tsq_cut.cuh): its four words lie
// 4096 bytes apart from dst on, which is a multiple of 16; four unaligned loads in flight, then four aligned stores.
__device__ __forceinline__ void join_copy_piece(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    uint4 a, b, c, d;
    __builtin_memcpy(&a, src, 16); __builtin_memcpy(&b, src + 4096, 16);
    __builtin_memcpy(&c, src + 8192, 16); __builtin_memcpy(&d, src + 12288, 16);
    *reinterpret_cast<uint4*>(dst) = a; *reinterpret_cast<uint4*>(dst + 4096) = b;
    *reinterpret_cast<uint4*>(dst + 8192) = c; *reinterpret_cast<uint4*>(dst + 12288) = d;
}

__global__ __launch_bounds__(256) void join_emit_kernel(const uint8_t* __restrict__ in, const BatchItem* __restrict__ items, uint32_t n_items,
                                                        const uint64_t* __restrict__ body_at, uint8_t* __restrict__ out,
                                                        const uint64_t* __restrict__ out_size, const int32_t* __restrict__ status)
{
    if (*status != 0) return;
    // v = o + skew: the place of output byte o counted from the aligned address in front of `out`
    const uint64_t skew = (uintptr_t)out & 15u, v_first = skew + kHeaderSize, v_end = skew + *out_size;
    for (uint64_t p = blockIdx.x; p * kJoinPiece < v_end; p += gridDim.x) {
        const uint64_t p0 = p * kJoinPiece, p1 = p0 + kJoinPiece;
        const uint64_t lo = p0 > v_first ? p0 : v_first, hi = p1 < v_end ? p1 : v_end;      // the piece's bytes, as v
        if (lo >= hi) continue;
        const uint32_t j0 = join_item_of(body_at, 0u, n_items, lo - skew);
        if (hi - skew <= body_at[j0 + 1u]) {
            // one body: the source of the byte at v is in[delta + v]
            const uint64_t delta = items[j0].in_at + kHeaderSize - body_at[j0] - skew;
            const uint64_t v0 = p0 + ((uint64_t)threadIdx.x << 4);                            // this lane's words: v0 + u * 4096
            if (lo == p0 && hi == p1) {                      // every word of the piece is whole: four loads in flight, then four stores
                join_copy_piece(in + (delta + v0), out + (v0 - skew));
                continue;
            }
            for (uint32_t u = 0; u < 4u; ++u) {              // the first and the last piece of the container: cut by the header or the end
                const uint64_t v = v0 + u * 4096u;
                const uint64_t a = v > lo ? v : lo, b = v + 16u < hi ? v + 16u : hi;
                if (a >= b) continue;
                if (b - a == 16u) {
                    uint4 w;
                    __builtin_memcpy(&w, in + (delta + v), 16);
                    *reinterpret_cast<uint4*>(out + (v - skew)) = w;
                } else for (uint64_t k = a; k < b; ++k) out[k - skew] = in[delta + k];
            }
            continue;
        }
        const uint32_t j1 = join_item_of(body_at, j0, n_items, hi - 1u - skew);
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint64_t v = p0 + ((uint64_t)(u * 256u + threadIdx.x) << 4);
            const uint64_t a = v > lo ? v : lo, b = v + 16u < hi ? v + 16u : hi;
            if (a >= b) continue;
            uint64_t o = a - skew;
            const uint64_t o_end = b - skew;
            uint32_t j = join_item_of(body_at, j0, j1 + 1u, o);
            if (b - a == 16u && o_end <= body_at[j + 1u]) {
                uint4 w;
                __builtin_memcpy(&w, in + items[j].in_at + kHeaderSize + (o - body_at[j]), 16);
                *reinterpret_cast<uint4*>(out + o) = w;
                continue;
            }
            for (; o < o_end; ++o) {
                while (o >= body_at[j + 1u]) ++j;            // (o < body_at[n_items]: j stays below n_items)
                out[o] = in[items[j].in_at + kHeaderSize + (o - body_at[j])];
            }
        }
    }
}

// The joined container's table of stream lengths, in joined order, from the descriptors the walk left: what
// tsqa_decompress_device_sized* takes.  One lane per block; lanes at or past first_block[n_items] leave, and all of them when the
// verdict is nonzero (then not every descriptor below cap_blocks was written).
__global__ __launch_bounds__(256) void join_block_sizes_kernel(const FrameInfo* __restrict__ frames, const uint64_t* __restrict__ d_first_block,
                                                               uint32_t n_items, uint32_t* __restrict__ d_block_sizes,
                                                               const int32_t* __restrict__ status)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (*status != 0 || b >= d_first_block[n_items]) return;
    d_block_sizes[b] = frames[b].stream_len;
}

}  // namespace tsq
