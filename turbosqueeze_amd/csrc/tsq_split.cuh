// tsq_split.cuh -- one container of short blocks (tsqa_compress_device_split*): the block descriptors and the container pack across
// encode launches; and the frame walk from a table of stream sizes (tsqa_decompress_device_sized*), made in parallel and checked
// against the container.  The container format itself: tsq_format.h.
#pragma once

#include "tsq_batch.cuh"
#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"

namespace tsq {

// One lane per block of an input of n bytes cut every block_len bytes: block b is the bytes [b * block_len, min(n, (b + 1) *
// block_len)), its look-ahead runs on into the bytes that follow it and sees zeros past n (avail: what is left of the input), and
// its slot is b % budget, its place in its encode launch.
__global__ __launch_bounds__(256) void split_blocks_kernel(uint64_t n, uint32_t block_len, uint32_t n_blocks, uint32_t budget,
                                                           EncBatchBlock* __restrict__ blocks)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blocks) return;
    const uint64_t at = b * block_len, left = n - at;
    blocks[b] = EncBatchBlock{at, left, left < block_len ? (uint32_t)left : block_len, (uint32_t)(b % budget)};
}

// After the encode launch of the container's blocks [b0, b0 + nb) (block b in slot b - b0): pack_scan_kernel for one launch of
// several.  ONE workgroup of exactly 256 threads: exclusive sums of (3 + size), 256 blocks per pass, on top of the offset that the
// launch before left in *run_at (launch 0: the header's 16 bytes, and the header goes out with it).  A header or frame is written
// only if it ends at or before out_cap: frame_at[b - b0] is the frame's offset, or kNoFrame, which batch_pack_copy_kernel skips.
// block_sizes (may be NULL) gets every stream length, whatever fits.  The last launch gives *out_size, the size needed, and
// kErrOverflow when that exceeds out_cap.  max_stream: the longest stream the copy behind this kernel moves whole (its pieces
// are counted from block_bound(block_len)); a longer one -- the encoder never makes it -- is kErrOverflow too, not a silent cut.
__global__ __launch_bounds__(256) void split_pack_scan_kernel(const uint32_t* __restrict__ sizes, uint32_t b0, uint32_t nb, uint32_t n_blocks,
                                                              uint64_t n_total, uint32_t ext, uint32_t max_stream, uint8_t* __restrict__ out,
                                                              uint64_t out_cap,
                                                              uint64_t* __restrict__ run_at, uint64_t* __restrict__ frame_at,
                                                              uint64_t* __restrict__ out_size, uint32_t* __restrict__ block_sizes,
                                                              int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    const uint32_t t = threadIdx.x;
    uint64_t base = b0 == 0u ? (uint64_t)kHeaderSize : *run_at;
    if (b0 == 0u && t == 0u && kHeaderSize <= out_cap) write_header(out, n_blocks, n_total);
    for (uint32_t k0 = 0; k0 < nb; k0 += 256u) {             // (no thread leaves the loop early: the scan needs them all)
        const uint32_t k = k0 + t;
        const bool valid = k < nb;
        const uint32_t sz = valid ? sizes[k] : 0u;
        uint64_t sum;
        const uint64_t at = base + group_scan_excl64(valid ? kFrameWordSize + (uint64_t)sz : 0ull, wave_sum, &sum);
        base += sum;
        if (valid) {
            const bool fits = at + kFrameWordSize + sz <= out_cap;
            if (fits) write_frame(out + at, sz, ext);
            frame_at[k] = fits ? at : kNoFrame;
            if (block_sizes) block_sizes[b0 + k] = sz;
            if (sz > max_stream) atomicMax(status, kErrOverflow);
        }
    }
    if (t != 0u) return;                                     // (every thread has read *run_at in front of the first scan's barrier)
    *run_at = base;
    if (b0 + nb == n_blocks) {
        *out_size = base;
        if (base > out_cap) atomicMax(status, kErrOverflow);
    }
}

// What both walks from a size table (frame_walk_sized_kernel; index_check_kernel, tsq_index.cuh) ask of the frame that the table
// puts at `at` with the stream length s (s_ok: stream_len_ok(s), and the lane has a frame at all): its six bytes lie inside n,
// before one of them is read; read_frame accepts what lies there; and the frame word's length is s.  *f: read_frame's fields.
__device__ __forceinline__ bool sized_frame_ok(const uint8_t* container, uint64_t n, uint64_t at, bool s_ok, uint32_t s, FrameInfo* f)
{
    return s_ok && at + kMinFrameSize <= n && read_frame(container + at, at, n, f) && f->stream_len == s;
}

// frame_walk_kernel from a table of stream sizes, which is not trusted.  ONE workgroup of exactly 256 threads, 256 frames per pass,
// both running sums carried in registers.  The header is checked as frame_walk_kernel checks it.  Then lane b takes its frame's
// place from the table alone, at_b = 16 + sum over j < b of (3 + s_j), and asks of it: stream_len_ok(s_b) -- a size that fails
// counts as 0 in the sum and refuses the container, so no sum can wrap (at most 2^32 frames of less than 2^23 bytes) --; at_b + 6
// <= n, before a byte of the frame is read; read_frame accepts what lies there; the frame word's length is s_b.  at_0 = 16 is
// true, and if frames 0 .. b - 1 are where the table says with the lengths it says, at_b is true: where every lane agrees, every
// place is the one walk_frames finds.  A second sum over the out_len read there places the output: oat_b + out_len_b <= total per
// frame, and the whole sum equal to total.  A refused container gets *out_size = 0 and kErrFormat, as from frame_walk_kernel; the
// descriptors of the frames that passed are written either way.
__global__ __launch_bounds__(256) void frame_walk_sized_kernel(const uint8_t* __restrict__ container, uint64_t n, uint32_t n_blocks,
                                                               const uint32_t* __restrict__ table, uint64_t out_cap,
                                                               FrameInfo* __restrict__ frames, uint64_t* __restrict__ out_size,
                                                               int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    const uint32_t t = threadIdx.x;
    uint32_t nb = 0;
    uint64_t total = 0;
    // (the same 16 bytes and the same verdict in every thread: the workgroup leaves together)
    if (!(read_header(container, n, &nb, &total) == kHeaderOk && nb == n_blocks && total <= out_cap)) {
        if (t == 0u) { *out_size = 0; atomicMax(status, kErrFormat); }
        return;
    }
    uint64_t at_base = kHeaderSize, oat_base = 0;
    bool bad = false;
    for (uint64_t b0 = 0; b0 < nb; b0 += 256u) {             // (no thread leaves the loop early: the scans need them all)
        const uint64_t b = b0 + t;
        const bool valid = b < nb;
        const uint32_t s = valid ? table[b] : 0u;
        const bool s_ok = valid && stream_len_ok(s);
        uint64_t sum;
        const uint64_t at = at_base + group_scan_excl64(s_ok ? kFrameWordSize + (uint64_t)s : 0ull, wave_sum, &sum);
        at_base += sum;
        FrameInfo f{0, 0, 0, 0, 0, 0};
        const bool f_ok = sized_frame_ok(container, n, at, s_ok, s, &f);
        const uint32_t out_len = f_ok ? f.out_len : 0u;
        const uint64_t oat = oat_base + group_scan_excl64(out_len, wave_sum, &sum);
        oat_base += sum;
        const bool fits = f_ok && oat + out_len <= total;
        if (fits) { f.stream_at = at + kFrameWordSize; f.out_at = oat; frames[b] = f; }
        if (valid && !fits) bad = true;
    }
    const bool refused = __syncthreads_or(bad ? 1 : 0) != 0 || oat_base != total;
    if (t != 0u) return;
    *out_size = refused ? 0ull : total;
    if (refused) atomicMax(status, kErrFormat);
}

}  // namespace tsq
