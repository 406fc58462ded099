// tsq_rows.cuh -- the gather into fixed-stride padded rows (tsqa_gather_rows_async): the ranges lie in device memory as the
// gather's do (tsq_gather.cuh), but range k does not land at a prefix sum: it lands in row k, at k * row_stride, the rest of the row
// is filled with a pad byte, and a table says how many bytes each row got.  Row k owns [k * stride, (k + 1) * stride) whatever the
// tables say, so no two destinations can overlap, and no byte scan is needed.  The launches:
//   rows_measure_kernel     gather_measure_kernel's rule, the NULL tables, the stride rule and the truncation
//   rows_sum_kernel         (a) each group of 256 rows: its piece counts summed, each row's piece number inside its group
//   rows_scan_kernel        (b) ONE workgroup: the groups' bases, 256 groups per pass; the words (c) raises are zeroed
//   rows_place_kernel       (c) the piece numbers, the rows that fit cap_pieces, the places, the lengths, the need words
//   gather_pieces_kernel .. gather_close_kernel   the gather's own, unchanged: the places it reads are k * stride
//   rows_pad_kernel         every byte of [0, n_rows * stride) that is no row's data gets the pad byte
// (a), (b) and (c) are the cut's shape (tsq_cut.cuh): no workgroup waits for another.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"
#include "tsq_gather.cuh"

namespace tsq {

constexpr uint32_t kRowsTruncate = 1u;                       // TSQA_ROWS_TRUNCATE
constexpr uint32_t kRowsGroup = 256;                         // rows per workgroup of launches (a) and (c), groups per pass of launch (b)

// One lane per row.  The tables are not trusted.  The gate and the item rule are gather_measure_kernel's, word for word: a nonzero
// verdict gives kErrFormat to every row and no descriptor is read; d_items == NULL addresses the whole data, else item d_items[k],
// which must exist and own blocks.  d_offsets == NULL: every offset is 0.  d_lengths == NULL: the row runs from its offset to the
// end of its item (or of the data), and an offset past that end is refused; else the range must end inside its total, compared so
// that offset + length is never formed.  A refused row gets kErrArg.  An accepted length above row_stride: with kRowsTruncate the row
// reads its first row_stride bytes and only those are counted in pieces; without, the row gets kErrOverflow, no bytes and no pieces.
// row_lengths[k] = the accepted length BEFORE the truncation (0 for a refused row): rows_place_kernel takes the largest from there
// and then puts the delivered length in its place.  kLive: as in gather_measure_kernel.
template <bool kLive>
__global__ __launch_bounds__(256) void rows_measure_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint64_t total, uint32_t shift,
                                                           const int32_t* __restrict__ verdict, const uint64_t* __restrict__ item_first,
                                                           uint32_t n_items, const uint32_t* __restrict__ d_items,
                                                           const uint64_t* __restrict__ d_offsets, const uint64_t* __restrict__ d_lengths,
                                                           uint32_t n_rows, uint64_t row_stride, uint32_t flags, GatherRange* __restrict__ ranges,
                                                           uint64_t* __restrict__ row_lengths, int32_t* __restrict__ row_status,
                                                           const uint64_t* __restrict__ live)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_rows) return;
    if constexpr (kLive) total = live[1];
    GatherRange r{0, 0, 0, 0u, 0u};
    uint64_t accepted = 0;
    int32_t st = kOk;
    if (verdict && *verdict != 0) st = kErrFormat;
    else {
        const uint64_t offset = d_offsets ? d_offsets[k] : 0ull;
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
        uint64_t len = 0;
        if (st == kOk) {
            if (d_lengths) { len = d_lengths[k]; if (len > mine || offset > mine - len) st = kErrArg; }
            else if (offset > mine) st = kErrArg;
            else len = mine - offset;
        }
        if (st == kOk) {
            accepted = len;
            if (len > row_stride) {
                if (flags & kRowsTruncate) len = row_stride;
                else { st = kErrOverflow; len = 0; }
            }
        }
        if (st == kOk && len != 0u) {
            r.at = base + offset; r.len = len;
            const uint32_t first = gather_block_of(frames, n_blocks, shift, r.at), last = gather_block_of(frames, n_blocks, shift, r.at + (len - 1u));
            r.first_block = first;
            if (shift) r.pieces = last - first + 1u;
            else for (uint32_t b = first; b <= last && b < n_blocks; ++b) r.pieces += frames[b].out_len != 0u;
        }
    }
    ranges[k] = r;
    row_lengths[k] = accepted;
    row_status[k] = st;
}

// Launch (a).  Workgroup g of exactly 256 threads: group_sum[g] = the pieces of the rows [256 g, 256 g + 256), and
// ranges[k].piece_at = the pieces of the group's rows in front of row k, which (c) puts on top of the group's base.  A refused row
// has no pieces.  A row has at most one piece per block, and the host has seen to it that n_rows times the block count stays below
// 2^55 (group_scan_excl64).
__global__ __launch_bounds__(256) void rows_sum_kernel(GatherRange* __restrict__ ranges, uint32_t n_rows, uint64_t* __restrict__ group_sum)
{
    __shared__ uint64_t wave_sum[4];
    const uint64_t k = (uint64_t)blockIdx.x * kRowsGroup + threadIdx.x;
    const bool valid = k < n_rows;
    uint64_t sum;
    const uint64_t own = group_scan_excl64(valid ? (uint64_t)ranges[k].pieces : 0ull, wave_sum, &sum);
    if (valid) ranges[k].piece_at = own;                     // (behind the scan, which needs every thread)
    if (threadIdx.x == 0u) group_sum[blockIdx.x] = sum;
}

// Launch (b).  cut_scan_kernel's scan: ONE workgroup of exactly 256 threads, group_sum[g] becomes the sum of the groups before g,
// 256 groups -- 65 536 rows -- per pass with the running sum carried in a register.  Thread 0 zeroes what (c) raises with atomicMax
// -- the fitting pieces, the largest status (words) and the largest accepted length (need[1]) -- and clears the decoders' word and
// the group count; need[0] = the pieces of all accepted rows.
__global__ __launch_bounds__(256) void rows_scan_kernel(uint64_t* __restrict__ group_sum, uint32_t n_groups, uint64_t* __restrict__ need,
                                                        GatherWords* __restrict__ words)
{
    __shared__ uint64_t wave_sum[4];
    if (threadIdx.x == 0u) { *words = GatherWords{0ull, 0u, kOk, kOk, 0u}; need[1] = 0ull; }
    uint64_t base = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += kRowsGroup) { // (no thread leaves the loop early: the scan needs them all; n_groups <= 2^24)
        const uint32_t g = g0 + threadIdx.x;
        const bool valid = g < n_groups;
        uint64_t sum;
        const uint64_t before = base + group_scan_excl64(valid ? group_sum[g] : 0ull, wave_sum, &sum);
        base += sum;
        if (valid) group_sum[g] = before;                    // (its own entry, which nobody else reads)
    }
    if (threadIdx.x == 0u) need[0] = base;
}

// Launch (c).  One lane per row: its piece number is the group's base and its own; an accepted row fits when its pieces end at or
// before cap_pieces -- a test of the row alone, as in cut_place_kernel: the numbers only grow, so a row behind one that does not
// fit starts past cap_pieces and cannot fit either, in whatever group it lies, a row without bytes included.  One that does not fit
// gets kErrOverflow and loses its bytes: nothing of it is cut or written.  places[k] = k * row_stride, what gather_pieces_kernel
// reads as the row's place.  row_lengths[k], on entry the accepted length, leaves as the bytes delivered: the row's (truncated)
// length where its status is 0, else 0.  The workgroup's largest accepted length, largest fitting piece end and largest status are
// gathered in LDS and raised by one atomicMax each, and only where there is something to raise: all start at 0 (launch (b)).
__global__ __launch_bounds__(256) void rows_place_kernel(GatherRange* __restrict__ ranges, uint32_t n_rows, const uint64_t* __restrict__ group_base,
                                                         uint64_t row_stride, uint32_t cap_pieces, uint64_t* __restrict__ places,
                                                         uint64_t* __restrict__ row_lengths, int32_t* __restrict__ row_status,
                                                         uint64_t* __restrict__ need, GatherWords* __restrict__ words)
{
    __shared__ unsigned long long group_fit, group_len;
    __shared__ int32_t worst;
    if (threadIdx.x == 0u) { group_fit = 0ull; group_len = 0ull; worst = kOk; }
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kRowsGroup + threadIdx.x;
    if (k < n_rows) {
        const uint64_t piece_at = group_base[blockIdx.x] + ranges[k].piece_at;
        const uint32_t pieces = ranges[k].pieces;
        const uint64_t accepted = row_lengths[k];
        uint64_t len = ranges[k].len;
        int32_t st = row_status[k];
        if (accepted != 0ull) atomicMax(&group_len, (unsigned long long)accepted);
        if (st == kOk) {
            if (piece_at + pieces <= cap_pieces) {
                ranges[k].piece_at = piece_at;
                if (pieces != 0u) atomicMax(&group_fit, (unsigned long long)(piece_at + pieces));
            } else { ranges[k].len = len = 0; ranges[k].pieces = 0u; row_status[k] = st = kErrOverflow; }
        }
        if (st != kOk) { atomicMax(&worst, st); len = 0; }
        places[k] = k * row_stride;
        row_lengths[k] = len;
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    if (group_fit != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(&words->fit_pieces), group_fit);
    if (group_len != 0ull) atomicMax(reinterpret_cast<unsigned long long*>(&need[1]), group_len);
    if (worst != kOk) atomicMax(&words->worst, worst);
}

// The padding: every byte of [0, n_rows * row_stride) past its row's delivered length gets `pad`.  The output is taken as the
// 16-byte words of the destination ADDRESS (v = o + skew, as in join_emit_kernel and cut_emit_kernel), one lane per word, the
// workgroups striding over them.  A word that lies wholly inside the output and holds no data byte of any row goes as one 16-byte
// store.  Every other word -- one cut by the output's first or last byte, or one that holds a data byte of any row: many rows when
// row_stride < 16, at most two otherwise -- goes byte by byte, and only its pad bytes.  So no data byte is written or read here and
// no byte outside the output: the decoders, which write data bytes alone, and this kernel write disjoint bytes in either order.
// row_lengths is rows_place_kernel's, at most row_stride per row (bounded again here, so that no table moves a row's edge).
__global__ __launch_bounds__(256) void rows_pad_kernel(uint8_t* __restrict__ out, uint32_t n_rows, uint64_t row_stride,
                                                       const uint64_t* __restrict__ row_lengths, uint32_t pad)
{
    const uint64_t skew = (uintptr_t)out & 15u, bytes = (uint64_t)n_rows * row_stride, v_end = skew + bytes;
    const uint64_t n_words = (v_end + 15u) >> 4;
    const uint32_t splat = pad * 0x01010101u;
    const uint4 word = make_uint4(splat, splat, splat, splat);
    for (uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * 256u) {
        const uint64_t v0 = w << 4, v1 = v0 + 16u;
        const uint64_t o0 = v0 > skew ? v0 - skew : 0ull, o1 = v1 < v_end ? v1 - skew : bytes;   // the word's bytes of the output
        if (o0 >= o1) continue;
        // the rows that the word meets, and whether any of them has data in it
        const uint64_t r0 = o0 / row_stride, r1 = (o1 - 1u) / row_stride;
        bool data = false;
        for (uint64_t r = r0, at = r0 * row_stride; r <= r1; ++r, at += row_stride) {
            const uint64_t len = row_lengths[r] < row_stride ? row_lengths[r] : row_stride;
            data = data || (at + len > o0 && len != 0u);     // (at < o1: the row's data starts in front of the word's end)
        }
        if (!data && o1 - o0 == 16u) { *reinterpret_cast<uint4*>(out + o0) = word; continue; }
        uint64_t r = r0, at = r0 * row_stride;
        uint64_t len = row_lengths[r] < row_stride ? row_lengths[r] : row_stride;
        for (uint64_t o = o0; o < o1; ++o) {
            if (o >= at + row_stride) { ++r; at += row_stride; len = row_lengths[r] < row_stride ? row_lengths[r] : row_stride; }
            if (o - at >= len) out[o] = (uint8_t)pad;
        }
    }
}

}  // namespace tsq
