// tsq_container.cuh -- device-side .tsq container assembly and frame walk (the format itself: tsq_format.h).
#pragma once

#include "tsq_common.cuh"
#include "tsq_format.h"

namespace tsq {

// One workgroup: exclusive scan of (3 + size_b), header + frame bytes, total size.
// Replaces compression_write_worker's serial frame emission (tsq_threads.cpp:192-275).
__global__ __launch_bounds__(256) void pack_scan_kernel(const uint32_t* __restrict__ sizes, uint32_t n_blocks,
                                                        uint64_t n_total, uint32_t ext, uint8_t* __restrict__ container,
                                                        uint64_t out_cap, uint64_t* __restrict__ frame_at,
                                                        uint64_t* __restrict__ out_size, int32_t* __restrict__ status)
{
    __shared__ uint64_t wave_sum[4];
    __shared__ uint64_t carry;
    const uint32_t t = threadIdx.x, lane = t & 63u, wid = t >> 6;
    if (t == 0) carry = kHeaderSize;
    __syncthreads();
    for (uint32_t base = 0; base < n_blocks; base += 256) {
        uint32_t b = base + t;
        uint64_t v = b < n_blocks ? kFrameWordSize + (uint64_t)sizes[b] : 0ull;
        uint64_t incl = v;                                   // inclusive wave scan
        for (uint32_t d = 1; d < 64; d <<= 1) {
            uint64_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_sum[wid] = incl;
        __syncthreads();
        uint64_t before = carry;
        for (uint32_t w = 0; w < wid; ++w) before += wave_sum[w];
        if (b < n_blocks) frame_at[b] = before + incl - v;
        __syncthreads();
        if (t == 255) carry = before + incl;
        __syncthreads();
    }
    const uint64_t total = carry;
    if (t == 0) {
        frame_at[n_blocks] = total;
        *out_size = total;
        if (total > out_cap) atomicMax(status, kErrOverflow);
    }
    if (total > out_cap) return;
    if (t == 0) write_header(container, n_blocks, n_total);
    for (uint32_t b = t; b < n_blocks; b += 256) write_frame(container + frame_at[b], sizes[b], ext);
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

// Serial frame walk of a container (tsq_threads.cpp:444-543: block k starts at 16 + sum(3+size_j)).
// One wavefront; lane 0 walks, since each frame position depends on the previous one.
__global__ __launch_bounds__(64) void frame_walk_kernel(const uint8_t* __restrict__ container, uint64_t n, uint32_t n_blocks,
                                                        uint64_t out_cap, FrameInfo* __restrict__ frames,
                                                        uint64_t* __restrict__ out_size, int32_t* __restrict__ status)
{
    if (threadIdx.x != 0) return;
    uint32_t nb = 0;
    uint64_t total = 0, at = kHeaderSize, oat = 0;
    bool bad = read_header(container, n, &nb, &total) != kHeaderOk || nb != n_blocks || total > out_cap;
    for (uint32_t b = 0; b < n_blocks && !bad; ++b) {
        FrameInfo f;
        if (at + kMinFrameSize > n || !read_frame(container + at, at, n, &f) || oat + f.out_len > total) { bad = true; break; }
        f.stream_at = at + kFrameWordSize; f.out_at = oat;
        frames[b] = f;
        oat += f.out_len;
        at += kFrameWordSize + f.stream_len;
    }
    if (!bad && oat != total) bad = true;
    *out_size = bad ? 0 : total;
    if (bad) atomicMax(status, kErrFormat);
}

}  // namespace tsq
