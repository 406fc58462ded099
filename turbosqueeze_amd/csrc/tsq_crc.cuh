// tsq_crc.cuh -- zlib's CRC-32 of every item of an index (tsqa_crc32_async).  dec_crc_kernel (tsq_dec_sym.cuh) decodes every block
// and leaves R(block) -- the CRC register behind the block's bytes with init 0 and no final xor, tsq_crc32.h -- in a table of one
// word per block, and raises the status word of the item whose block holds a malformed stream.  What follows here:
//   crc_fold_kernel    one lane per block: R(block) (x) x^(8 * bytes between the block's end and its item's end) is XORed into the
//                      item's word, and the same against the end of the whole data into d_all_crc; d_block_crc.  One lane per item,
//                      and one for the whole data, adds what crc32 adds to R: 0xFFFFFFFF (x) x^(8 T) xor 0xFFFFFFFF.
//   crc_close_kernel   one lane per item: the CRC of an item whose status is nonzero becomes 0; the call's status; d_all_crc
//                      becomes 0 when an item was raised to TSQA_ERR_STREAM or the index was refused.
// An index of no blocks runs the same launches but the decode: its CRCs are 0 and its items keep the index's statuses.
// R is linear, so the terms of an item may arrive in any order: the atomic XORs make an exact and deterministic sum, and there is
// no scan.  Nothing here is hot: x^(8 n) is made by square and multiply over the 64-bit byte count (crc_xpow8).
#pragma once

#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_crc32.h"
#include "tsq_find.cuh"
#include "tsq_format.h"
#include "tsq_gather.cuh"

namespace tsq {

__global__ __launch_bounds__(256) void crc_fold_kernel(const FrameInfo* __restrict__ frames, uint32_t n_blocks, uint64_t total,
                                                       const int32_t* __restrict__ verdict, const uint64_t* __restrict__ item_first,
                                                       uint32_t n_items, const uint32_t* __restrict__ block_r,
                                                       const int32_t* __restrict__ item_status, uint32_t* __restrict__ item_crc,
                                                       uint32_t* __restrict__ block_crc, uint32_t* __restrict__ all_crc)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (verdict && *verdict != 0) return;
    if (k < n_blocks) {
        const uint32_t b = (uint32_t)k;
        const FrameInfo f = frames[b];
        uint32_t item;
        uint64_t item_at, item_end;
        find_item_of(frames, n_blocks, total, item_first, n_items, b, f, &item, &item_at, &item_end);
        if (item_status[item] == 0) {                        // (a raised item's blocks may have left no word; its CRC becomes 0)
            const uint32_t r = block_r[b];
            const uint64_t end = f.out_at + f.out_len;
            if (r != 0u) atomicXor(item_crc + item, crc_mul(r, crc_xpow8(item_end - end)));
            if (all_crc && r != 0u && end <= total) atomicXor(all_crc, crc_mul(r, crc_xpow8(total - end)));
            if (block_crc) block_crc[b] = r ^ crc_init_term(f.out_len);
        }
    }
    if (k < n_items) {
        uint64_t len = total;
        if (item_first) {
            const uint64_t fb = item_first[k], fe = item_first[k + 1u];
            const uint64_t at = gather_block_start(frames, n_blocks, total, fb), end = gather_block_start(frames, n_blocks, total, fe);
            len = fb <= fe && at <= end ? end - at : 0ull;
        }
        const uint32_t term = crc_init_term(len);
        if (term != 0u) atomicXor(item_crc + k, term);
    }
    if (k == n_items && all_crc) {
        const uint32_t term = crc_init_term(total);
        if (term != 0u) atomicXor(all_crc, term);
    }
}

// any: the call's word of dec_crc_kernel (zero, or kErrStream once a workgroup left with its item's word raised)
__global__ __launch_bounds__(256) void crc_close_kernel(const int32_t* __restrict__ verdict, const int32_t* __restrict__ any, uint32_t n_items,
                                                        int32_t* __restrict__ item_status, uint32_t* __restrict__ item_crc,
                                                        uint32_t* __restrict__ all_crc, int32_t* __restrict__ status)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool refused = verdict && *verdict != 0;
    if (k < n_items) {
        if (refused) item_status[k] = kErrFormat;
        if (refused || item_status[k] != 0) item_crc[k] = 0u;
    }
    if (k == 0u) {
        const int32_t st = refused ? kErrFormat : *any != 0 ? kErrStream : kOk;
        if (st != kOk && all_crc) *all_crc = 0u;
        *status = st;
    }
}

}  // namespace tsq
