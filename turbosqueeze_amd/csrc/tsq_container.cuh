// tsq_container.cuh -- device-side .tsq container assembly and frame walk (the format itself: tsq_format.h).
#pragma once

#include "tsq_common.cuh"
#include "tsq_format.h"

namespace tsq {

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

// One workgroup of exactly 256 threads: exclusive scan of (3 + size_b), 256 blocks per pass with the running sum carried in a
// register; header + frame bytes, total size.  Replaces compression_write_worker's serial frame emission (tsq_threads.cpp:192-275).
__global__ __launch_bounds__(256) void pack_scan_kernel(const uint32_t* __restrict__ sizes, uint32_t n_blocks,
                                                        uint64_t n_total, uint32_t ext, uint8_t* __restrict__ container,
                                                        uint64_t out_cap, uint64_t* __restrict__ frame_at,
                                                        uint64_t* __restrict__ out_size, int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    const uint32_t t = threadIdx.x;
    uint64_t total = kHeaderSize;
    for (uint32_t base = 0; base < n_blocks; base += 256) {  // (no thread leaves the loop early: the scan needs them all)
        const uint32_t b = base + t;
        uint64_t sum;
        const uint64_t at = total + group_scan_excl64(b < n_blocks ? kFrameWordSize + (uint64_t)sizes[b] : 0ull, wave_sum, &sum);
        if (b < n_blocks) frame_at[b] = at;
        total += sum;
    }
    if (t == 0) {
        frame_at[n_blocks] = total;
        *out_size = total;
        if (total > out_cap) atomicMax(status, kErrOverflow);
    }
    if (total > out_cap) return;
    if (t == 0) write_header(container, n_blocks, n_total);
    for (uint32_t b = t; b < n_blocks; b += 256) write_frame(container + frame_at[b], sizes[b], ext);   // (frame_at[b]: this thread's own)
}

// Copy each block stream from its slot to its place in the container.  Destination offsets are
// arbitrary bytes, so each thread stores one destination-aligned 16-byte word assembled from an
// unaligned 16-byte load; head and tail bytes go singly.  One workgroup moves the piece of the
// stream's size bytes that starts at piece_at.
constexpr uint32_t kPackPiece = 32768;
__device__ __forceinline__ void pack_copy_piece(const uint8_t* src, uint32_t size, uint8_t* dst, uint32_t piece_at)
{
    // Piece p moves the destination-aligned words [head + p*P, head + (p+1)*P); piece 0 also
    // moves the `head` bytes in front of the first aligned word.
    const uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    const uint32_t begin = piece_at + head;
    const uint32_t end_all = size;
    uint32_t end = begin + kPackPiece;
    if (end > end_all) end = end_all;
    if (piece_at == 0) for (uint32_t k = threadIdx.x; k < head && k < size; k += 256) dst[k] = src[k];
    if (begin >= end_all) return;
    const uint32_t words = (end - begin) >> 4;
    for (uint32_t w = threadIdx.x; w < words; w += 256) {
        uint4 v;
        __builtin_memcpy(&v, src + begin + (w << 4), 16);
        *reinterpret_cast<uint4*>(dst + begin + (w << 4)) = v;
    }
    // the last piece that reaches the end carries the tail bytes
    if (end == end_all) for (uint32_t k = begin + (words << 4) + threadIdx.x; k < end_all; k += 256) dst[k] = src[k];
}

// grid = (pieces, n_blocks)
__global__ __launch_bounds__(256) void pack_copy_kernel(const uint8_t* __restrict__ slots, const uint32_t* __restrict__ sizes,
                                                        const uint64_t* __restrict__ frame_at, uint8_t* __restrict__ container,
                                                        const int32_t* __restrict__ status)
{
    const uint32_t b = blockIdx.y;
    const uint32_t size = sizes[b];
    const uint32_t piece_at = blockIdx.x * kPackPiece;
    if (piece_at >= size || *status != 0) return;
    pack_copy_piece(slots + (size_t)b * kSlotSize, size, container + frame_at[b] + 3, piece_at);
}

// The frame walk of one container (walk_frames), validated as the reader validates it: the header, its block count against the
// caller's, its total against the capacity, every frame, lengths that add up to the total.  One wavefront; lane 0 walks.  A
// refused container gets *out_size = 0 and *status kErrFormat; the descriptors written by then stay as they are.
__global__ __launch_bounds__(64) void frame_walk_kernel(const uint8_t* __restrict__ container, uint64_t n, uint32_t n_blocks,
                                                        uint64_t out_cap, FrameInfo* __restrict__ frames,
                                                        uint64_t* __restrict__ out_size, int32_t* __restrict__ status)
{
    if (threadIdx.x != 0) return;
    uint32_t nb = 0;
    uint64_t total = 0;
    const bool ok = read_header(container, n, &nb, &total) == kHeaderOk && nb == n_blocks && total <= out_cap &&
                    walk_frames(container, n, nb, total, [&](uint32_t b, uint64_t, const FrameInfo& f) { frames[b] = f; return true; }) == kWalkOk;
    *out_size = ok ? total : 0;
    if (!ok) atomicMax(status, kErrFormat);
}

}  // namespace tsq
