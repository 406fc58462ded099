// tsq_cut.cuh -- block ranges cut out of an indexed container, each as a container of its own (tsqa_cut_async): nothing is decoded,
// the frames of blocks [first, first + count) are one span of the container and are copied behind a new header.  The launches:
//   cut_measure_kernel   the index's verdict, the range rule, each range's size, total and source place
//   cut_layout_kernel    the packed places, the ranges that fit, the call's status, the headers
//   cut_emit_kernel      the copy, balanced over the output
// The last two read what the first leaves: a refused index leaves sizes of 0, and then nothing is placed, fits or is copied.
// The container format itself: tsq_format.h.  The packed layout: tsqa_plan_packed.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"
#include "tsq_join.cuh"

namespace tsq {

// What the call keeps per range in the context's scratch: where the range's first frame starts in the index's container, and the two
// fields of its header.  All zero for a refused range.  Entry n_ranges: src_at = where the last fitting container ends in the output.
struct CutRange { uint64_t src_at, total, count; };

// One lane per range.  The tables are not trusted: a range must hold a block and lie inside the index, compared so that
// first + count is never formed.  An accepted range gets its size -- 16 + the bytes from its first frame to the end of its last --,
// its total and status 0; a refused one kErrArg, size 0 and total 0, and no descriptor is read for it.  verdict (may be NULL): the
// word of an index made from a size table; where it is nonzero the descriptors are not to be believed, none is read, and every
// range gets kErrFormat.
__global__ __launch_bounds__(256) void cut_measure_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, const int32_t* __restrict__ verdict,
                                                          const uint64_t* __restrict__ d_first, const uint64_t* __restrict__ d_count,
                                                          uint32_t n_ranges, CutRange* __restrict__ ranges, uint64_t* __restrict__ d_sizes,
                                                          uint64_t* __restrict__ d_totals, int32_t* __restrict__ item_status)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= n_ranges) return;
    const uint64_t first = d_first[k], count = d_count[k];
    CutRange r{0, 0, 0};
    uint64_t size = 0;
    int32_t st = kOk;
    if (verdict && *verdict != 0) st = kErrFormat;
    else if (count < 1u || first >= n_blocks || count > n_blocks - first) st = kErrArg;
    else {
        const FrameInfo a = frames[first], z = frames[first + count - 1u];
        r.src_at = a.stream_at - kFrameWordSize;
        r.total = z.out_at + z.out_len - a.out_at;
        r.count = count;
        size = kHeaderSize + (z.stream_at + z.stream_len) - r.src_at;
    }
    ranges[k] = r;
    d_sizes[k] = size;
    if (d_totals) d_totals[k] = r.total;
    item_status[k] = st;
}

// Behind cut_measure_kernel: tsqa_plan_packed's rule applied to the sizes.  ONE workgroup of exactly 256 threads, 256 ranges per
// pass, the running sum carried: round_up(size, align) is summed, as every place is a multiple of align, and the last place is not
// rounded.  The places are complete whatever fits.  An accepted range fits when its container ends at or before out_size; the
// places only grow and no accepted range is empty, so the fitting ranges are a prefix of the accepted ones by themselves.  A range
// that fits gets its header; one that does not, kErrOverflow.  *status = the largest item status; ranges[n_ranges].src_at = where
// the last fitting container ends.  The host has seen to it that n_ranges times the largest padded size stays below 2^55.
__global__ __launch_bounds__(256) void cut_layout_kernel(CutRange* __restrict__ ranges, uint32_t n_ranges, uint32_t align, uint8_t* __restrict__ out,
                                                         uint64_t out_size, const uint64_t* __restrict__ d_sizes, uint64_t* __restrict__ d_offsets,
                                                         int32_t* __restrict__ item_status, int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ unsigned long long fit_end;
    __shared__ int32_t worst;
    const uint64_t mask = (uint64_t)align - 1u;
    if (threadIdx.x == 0) { fit_end = 0ull; worst = kOk; }
    uint64_t base = 0;
    for (uint64_t k0 = 0; k0 < n_ranges; k0 += 256u) {       // (no lane leaves the loop early: the scan needs them all)
        const uint64_t k = k0 + threadIdx.x;
        const bool valid = k < n_ranges;
        const uint64_t size = valid ? d_sizes[k] : 0ull;
        int32_t st = valid ? item_status[k] : kOk;           // (in front of the scan: both loads are in flight together)
        uint64_t sum;
        const uint64_t at = base + group_scan_excl64((size + mask) & ~mask, wave_sum, &sum);
        base += sum;
        if (!valid) continue;                                // (behind the scan; nothing below is a barrier)
        if (st == kOk) {
            if (at + size <= out_size) {
                write_header(out + at, (uint32_t)ranges[k].count, ranges[k].total);
                atomicMax(&fit_end, (unsigned long long)(at + size));
            } else item_status[k] = st = kErrOverflow;
        }
        if (st != kOk) atomicMax(&worst, st);
        d_offsets[k] = at;
        if (k + 1u == n_ranges) d_offsets[n_ranges] = at + size;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    *status = worst;
    ranges[n_ranges].src_at = fit_end;
}

// The copy, balanced over the output as join_emit_kernel's is: a workgroup takes one piece of kJoinPiece bytes of the output after
// the other, up to the end of the last fitting container, cut at multiples of 16 of the destination ADDRESS.  The range that holds
// the piece's first byte is found by bisection in d_offsets (join_item_of: ranges without bytes share their place with the next
// one, and the last of them is found).  Every nonempty range below that end is accepted and fits.  Its body is
// [d_offsets[j] + 16, d_offsets[j] + d_sizes[j]), from ranges[j].src_at on in the index's container; its header is
// cut_layout_kernel's and the padding behind it is nobody's.  A piece inside one body is join_copy_piece's; elsewhere each word finds
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
