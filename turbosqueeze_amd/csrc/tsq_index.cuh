// tsq_index.cuh -- the index of a container of short blocks, made from its table of stream sizes (tsqa_index_create_sized*): the
// frame walk of frame_walk_sized_kernel (tsq_split.cuh) spread over the chip, and the gate in front of the reads of such an index.
//
// The caller states the geometry (n_total bytes cut every block_len), so block b's output starts at b * block_len and only the
// frames' places are left to sum: place_b = 16 + sum over j < b of (3 + s_j).  Three plain launches, 256 frames per workgroup, and
// no workgroup waits for another: (1) each group's sum, (2) ONE workgroup's exclusive scan of the group sums, and the header,
// (3) each group's own scan on top of its base, the frame checks and the descriptors.  Nothing in the table or the container is
// trusted; a refusal is kErrFormat in *verdict, which starts at 0, as every descriptor does.
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"
#include "tsq_split.cuh"

namespace tsq {

constexpr uint32_t kIndexGroup = 256;                        // frames per workgroup of launches 1 and 3, groups per pass of launch 2

// What frame b adds to the places behind it: a size that stream_len_ok refuses counts as 0 (and refuses the container in launch 3),
// so no sum can wrap: at most 2^32 frames of less than 2^23 bytes.
__device__ __forceinline__ uint64_t index_frame_room(const uint32_t* __restrict__ table, uint64_t b, uint32_t n_blocks)
{
    if (b >= n_blocks) return 0ull;
    const uint32_t s = table[b];
    return stream_len_ok(s) ? kFrameWordSize + (uint64_t)s : 0ull;
}

// Launch 1.  Workgroup g of exactly 256 threads: group_sum[g] = the room of the frames [256 g, 256 g + 256).
__global__ __launch_bounds__(256) void index_sum_kernel(const uint32_t* __restrict__ table, uint32_t n_blocks, uint64_t* __restrict__ group_sum)
{
    __shared__ uint64_t wave_sum[4];
    uint64_t sum;
    (void)group_scan_excl64(index_frame_room(table, (uint64_t)blockIdx.x * kIndexGroup + threadIdx.x, n_blocks), wave_sum, &sum);
    if (threadIdx.x == 0u) group_sum[blockIdx.x] = sum;
}

// Launch 2.  ONE workgroup of exactly 256 threads: group_sum[g] becomes the sum of the groups before g, 256 groups per pass with the
// running sum carried in a register (a group's sum is below 2^31, a pass's below 2^39).  Thread 0 also checks the header, once for
// the whole walk: read_header for n, the caller's block count and the caller's total.
__global__ __launch_bounds__(256) void index_scan_kernel(const uint8_t* __restrict__ container, uint64_t n, uint32_t n_blocks, uint64_t n_total,
                                                         uint64_t* __restrict__ group_sum, uint32_t n_groups, int32_t* __restrict__ verdict)
{
    __shared__ uint64_t wave_sum[4];
    const uint32_t t = threadIdx.x;
    if (t == 0u) {
        uint32_t nb = 0;
        uint64_t total = 0;
        if (!(read_header(container, n, &nb, &total) == kHeaderOk && nb == n_blocks && total == n_total)) atomicMax(verdict, kErrFormat);
    }
    uint64_t base = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += kIndexGroup) {   // (no thread leaves the loop early: the scan needs them all; g0 cannot wrap: n_groups <= 2^24)
        const uint32_t g = g0 + t;
        const bool valid = g < n_groups;
        uint64_t sum;
        const uint64_t before = base + group_scan_excl64(valid ? group_sum[g] : 0ull, wave_sum, &sum);
        base += sum;
        if (valid) group_sum[g] = before;                    // (its own entry, which nobody else reads)
    }
}

// Launch 3.  Workgroup g of exactly 256 threads, lane b = 256 g + t: the frame's place is 16 + group_base[g] + the room of the
// group's frames before it; sized_frame_ok there (the predicate of frame_walk_sized_kernel); and the geometry: out_len is
// block_len, or for the last block what n_total leaves.  A frame that passes gets the descriptor frame_walk_kernel makes for it,
// with out_at = b * block_len; one that does not leaves its descriptor as it was (zeros) and refuses the container.
__global__ __launch_bounds__(256) void index_check_kernel(const uint8_t* __restrict__ container, uint64_t n, uint32_t n_blocks, uint64_t n_total,
                                                          uint32_t block_len, const uint32_t* __restrict__ table,
                                                          const uint64_t* __restrict__ group_base, FrameInfo* __restrict__ frames,
                                                          int32_t* __restrict__ verdict)
{
    __shared__ uint64_t wave_sum[4];
    const uint64_t b = (uint64_t)blockIdx.x * kIndexGroup + threadIdx.x;
    const bool valid = b < n_blocks;
    const uint32_t s = valid ? table[b] : 0u;
    const bool s_ok = valid && stream_len_ok(s);
    uint64_t sum;
    const uint64_t at = kHeaderSize + group_base[blockIdx.x] + group_scan_excl64(s_ok ? kFrameWordSize + (uint64_t)s : 0ull, wave_sum, &sum);
    if (!valid) return;                                      // (behind the scan, which needs every thread)
    FrameInfo f{0, 0, 0, 0, 0, 0};
    const uint64_t out_at = b * block_len;
    const uint64_t want_len = b + 1u < n_blocks ? (uint64_t)block_len : n_total - out_at;
    if (sized_frame_ok(container, n, at, s_ok, s, &f) && f.out_len == want_len) {
        f.stream_at = at + kFrameWordSize; f.out_at = out_at;
        frames[b] = f;
    } else {
        atomicMax(verdict, kErrFormat);
    }
}

// In front of a read through an index made from a size table, behind the memset of the read's status word: a refused index refuses
// the read, and sym_decode_block leaves as a whole when it finds *status nonzero.  One thread.
__global__ void index_gate_kernel(const int32_t* __restrict__ verdict, int32_t* __restrict__ status)
{
    const int32_t v = *verdict;
    if (v != 0) atomicMax(status, v);
}

}  // namespace tsq
