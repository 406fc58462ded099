// tsq_format.h -- the .tsq container format, for host and device code alike: constants and inline readers and writers, no kernels.
//
// Container (turbosqueeze.cpp:64-83, tsq_threads.cpp:218-239,333-335): 16-byte header
// "TSQ1" | u32 n_blocks | u64 total, then per block a u24 frame word (stream length | ext << 23) and the stream, whose first three
// bytes are the block's uncompressed size (u24).  All fields are little-endian.
#pragma once

#include "tsq_common.cuh"

namespace tsq {

constexpr uint32_t kMagic         = 0x31515354u;   // "TSQ1" read as a little-endian u32
constexpr uint32_t kHeaderSize    = 16;
constexpr uint32_t kFrameWordSize = 3;
constexpr uint32_t kMinFrameSize  = 6;             // the frame word and the stream's own size word
constexpr uint32_t kFrameLenMask  = 0x7FFFFFu;     // tsq_threads.cpp:513-517
constexpr uint32_t kFrameExtBit   = 0x800000u;     // tsq_threads.cpp:218-219

__host__ __device__ inline uint64_t load_le(const uint8_t* p, uint32_t bytes)
{
    uint64_t v = 0; for (uint32_t k = 0; k < bytes; ++k) v |= (uint64_t)p[k] << (8 * k); return v;
}
__host__ __device__ inline void store_le(uint8_t* p, uint64_t v, uint32_t bytes) { for (uint32_t k = 0; k < bytes; ++k) p[k] = (uint8_t)(v >> (8 * k)); }

// A block stream the writer may emit and the reader accepts: its size word and at most TSQ_OUTPUT_SZ bytes in all
// (tsq_threads.cpp:526-531).
__host__ __device__ inline bool stream_len_ok(uint64_t len) { return len >= 3 && len <= kSlotSize; }

__host__ __device__ inline void write_header(uint8_t* p, uint32_t n_blocks, uint64_t total)
{
    store_le(p, kMagic, 4); store_le(p + 4, n_blocks, 4); store_le(p + 8, total, 8);
}
__host__ __device__ inline void write_frame(uint8_t* p, uint32_t stream_len, uint32_t ext)
{
    store_le(p, stream_len | (ext ? kFrameExtBit : 0u), kFrameWordSize);
}

// Room that always holds the frame of a block of k bytes: its frame word and a stream of at most every byte a literal of its own,
// never more than a slot (a full block: 3 + TSQ_OUTPUT_SZ).
__host__ __device__ inline uint64_t block_bound(uint64_t k)
{
    const uint64_t worst = 11 + k + (k >> 3) + (k >> 1);
    return kFrameWordSize + (worst < kSlotSize ? worst : (uint64_t)kSlotSize);
}

// Room that always holds the container of n bytes cut into blocks of block_len (tsqa_plan_split): the header, then block_bound
// per block.
__host__ __device__ inline uint64_t split_bound(uint64_t n, uint64_t block_len)
{
    const uint64_t full = n / block_len, rest = n % block_len;
    return kHeaderSize + full * block_bound(block_len) + (rest ? block_bound(rest) : 0);
}

// Room that always holds the container of an n-byte item (tsqa_batch_bound).
__host__ __device__ inline uint64_t batch_bound(uint64_t n) { return split_bound(n, kBlockSize); }

// read_header's verdicts.  The first two are the reader's own refusals (tsq_threads.cpp:732-768); an implausible header has block
// counts that a container of n bytes cannot hold: more blocks than 6-byte frames fit, or more output than they can make.
enum HeaderVerdict : int { kHeaderOk = 0, kHeaderBadMagic, kHeaderNoBlocks, kHeaderImplausible };

// The header of a container of n bytes; `head` holds its first 16 bytes and is not read when n < 16.  *n_blocks and *total are
// set whenever the magic is there.
__host__ __device__ inline int read_header(const uint8_t* head, uint64_t n, uint32_t* n_blocks, uint64_t* total)
{
    if (n < kHeaderSize || load_le(head, 4) != kMagic) return kHeaderBadMagic;
    const uint32_t nb = (uint32_t)load_le(head + 4, 4);
    const uint64_t tot = load_le(head + 8, 8);
    *n_blocks = nb; *total = tot;
    if (nb == 0) return kHeaderNoBlocks;
    if (nb > (n - kHeaderSize) / kMinFrameSize || tot > (uint64_t)nb * kBlockSize) return kHeaderImplausible;
    return kHeaderOk;
}

// The frame whose word starts at byte `at` of a container of n bytes; `six` holds its first six bytes (the frame word and the
// stream's size word).  Fills stream_len, ext and out_len; the offsets are the caller's.  False for a stream length outside
// [3, TSQ_OUTPUT_SZ], a stream that runs past n, or a block larger than TSQ_BLOCK_SZ.
__host__ __device__ inline bool read_frame(const uint8_t* six, uint64_t at, uint64_t n, FrameInfo* f)
{
    const uint32_t word = (uint32_t)load_le(six, kFrameWordSize);
    f->stream_len = word & kFrameLenMask;
    f->ext = word >> 23;
    f->out_len = (uint32_t)load_le(six + kFrameWordSize, 3);
    f->pad = 0;
    return stream_len_ok(f->stream_len) && at + kFrameWordSize + f->stream_len <= n && f->out_len <= kBlockSize;
}

// walk_frames' verdicts: every frame passed, a malformed or truncated frame, block sizes that do not add up to the header's total
// (a block that runs past it, or a sum short of it), or a visitor that ended the walk.
enum WalkVerdict : int { kWalkOk = 0, kWalkBadFrame, kWalkBadSum, kWalkEnded };

// THE reader's frame walk (tsq_threads.cpp:444-543: block k starts at 16 + sum(3 + size_j)), for host and device: over the nb frames
// of the container of n bytes at p, whose header read_header has accepted with that count and `total`.  Serial, since each frame's
// place depends on the one before.  visit(b, at, f) per frame that passes -- `at`: its frame word; f: read_frame's fields, with
// stream_at and out_at relative to the container and its data -- returns false to end the walk.
template <class Visit>
__host__ __device__ inline WalkVerdict walk_frames(const uint8_t* p, uint64_t n, uint32_t nb, uint64_t total, Visit&& visit)
{
    uint64_t at = kHeaderSize, oat = 0;
    for (uint32_t b = 0; b < nb; ++b) {
        FrameInfo f;
        if (at + kMinFrameSize > n || !read_frame(p + at, at, n, &f)) return kWalkBadFrame;
        if (oat + f.out_len > total) return kWalkBadSum;
        f.stream_at = at + kFrameWordSize; f.out_at = oat;
        if (!visit(b, at, f)) return kWalkEnded;
        oat += f.out_len;
        at += kFrameWordSize + f.stream_len;
    }
    return oat == total ? kWalkOk : kWalkBadSum;
}

}  // namespace tsq
