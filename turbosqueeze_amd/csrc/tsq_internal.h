// tsq_internal.h -- host-side context shared by the runtime and the reference-API layer.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <utility>
#include <vector>

#include "../../include/turbosqueeze_amd.h"

namespace tsq { struct FrameInfo; struct BatchItem; struct EncBatchBlock; struct CutRange; struct GatherRange; struct GatherWords; struct RangeItem; struct BlockGroup; struct RecordBlock; struct RecordWords; }

struct tsqa_ctx;

// One scratch buffer in device memory: the pointer, which it reads as, and the capacity in elements.  grow() frees before it
// allocates, so the peak does not double; the caller has waited for whatever may still use the old buffer.  A failed allocation is
// reported through the context (TSQA_ERR_HIP) and leaves a null pointer and capacity 0: the next call tries again.  Freed with its owner.
template <class T> struct tsqa_scratch {
    T* p = nullptr;
    size_t cap = 0;
    tsqa_scratch() = default;
    tsqa_scratch(const tsqa_scratch&) = delete;
    tsqa_scratch& operator=(const tsqa_scratch&) = delete;
    ~tsqa_scratch() { reset(); }
    operator T*() const { return p; }
    bool needs(size_t n) const { return n > cap; }
    void reset() { (void)hipFree(p); p = nullptr; cap = 0; }
    bool grow(tsqa_ctx* c, size_t n);          // to n elements where needs(n); false: refused, the error is set
};

// Its sibling in pinned host memory, with the same rules: grow() frees before it allocates, and a failed allocation -- returned, for
// the caller to report -- leaves a null pointer and capacity 0.  How the memory is pinned belongs to the buffer: hipHostMallocPortable
// where threads that have other devices current copy from it (the scheduler's lanes), hipHostMallocDefault otherwise.
template <class T> struct tsqa_pinned {
    T* p = nullptr;
    size_t cap = 0;
    const unsigned flags;
    explicit tsqa_pinned(unsigned f = hipHostMallocDefault) : flags(f) {}
    tsqa_pinned(const tsqa_pinned&) = delete;
    tsqa_pinned& operator=(const tsqa_pinned&) = delete;
    ~tsqa_pinned() { reset(); }
    operator T*() const { return p; }
    bool needs(size_t n) const { return n > cap; }
    void reset() { (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t grow(size_t n)                  // to n elements where needs(n)
    {
        if (!needs(n)) return hipSuccess;
        reset();
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), flags);
        if (e != hipSuccess) p = nullptr; else cap = n;
        return e;
    }
};

// Descriptors a call plans on the host for its kernels (range-read items, batch descriptors): a ring of two slots, used in turn, each a
// pinned host buffer and its copy on the device, grown by doubling.  A slot is reused once the call that used it has finished: two
// calls can be in flight, the third waits for the first.
class tsqa_uploads {
    tsqa_pinned<uint8_t> host_[2];
    tsqa_scratch<uint8_t> dev_[2];             // (the capacity of both copies, in bytes)
    hipEvent_t done_[2] = {nullptr, nullptr};
    bool pending_[2] = {false, false};
    int next_ = 0;

public:
    // An acquired slot: fill host<T>(at), send(), launch what reads dev<T>(at), commit().  A call that ends before anything is
    // enqueued simply drops it: the slot is not pending.  (`at`: the byte offset of a second table in the same buffer.)
    struct Slot {
        tsqa_uploads* u = nullptr;
        int k = 0;
        template <class T> T* host(size_t at = 0) const { return reinterpret_cast<T*>(u->host_[k] + at); }
        template <class T> T* dev(size_t at = 0) const { return reinterpret_cast<T*>(u->dev_[k] + at); }
        size_t cap() const { return u->dev_[k].cap; }
        hipError_t send(size_t bytes, hipStream_t s) const { return hipMemcpyAsync(u->dev_[k], u->host_[k], bytes, hipMemcpyHostToDevice, s); }
        // Behind the LAST kernel of the call that reads the slot, however that launch went: neither copy of the descriptors is touched
        // again before the work that uses them has finished.
        hipError_t commit(hipStream_t s) const
        {
            const hipError_t e = hipEventRecord(u->done_[k], s);
            if (e == hipSuccess) u->pending_[k] = true;
            return e;
        }
    };
    // the next slot, once the call that used it last has finished, with room for `bytes`
    int acquire(tsqa_ctx* c, size_t bytes, Slot* slot);
    void destroy();
};

struct tsqa_ctx {
    int device = 0;
    int n_cus = 0;
    hipStream_t stream = nullptr;
    // scratch in HBM (tsqa_scratch: each buffer knows its capacity and is freed with the context)
    tsqa_scratch<uint8_t> slots;               // n_blocks x TSQ_OUTPUT_SZ encoded block streams, and 256 bytes
    tsqa_scratch<uint32_t> sizes;              // n_blocks stream sizes
    tsqa_scratch<uint64_t> frame_at;           // n_blocks + 1 frame offsets in the container
    tsqa_scratch<tsq::FrameInfo> frames;       // n_blocks frame descriptors (decode)
    tsqa_scratch<uint32_t> block_owner;        // n_blocks: the batch item each frame belongs to (tsqa_decompress_batch_items_async)
    tsqa_scratch<uint16_t> tables;             // n_blocks x 2^17 u16 position tables of the encoders
    tsqa_pinned<tsq::FrameInfo> host_frames;   // frame descriptors built on the host (sharded fetch + decode)
    std::vector<uint64_t> host_frame_src;      // where each owned frame's stream starts in the host container
    hipEvent_t host_frames_copied = nullptr;   // recorded behind the descriptors' copy to the device
    bool host_frames_pending = false;
    // what the last tsqa_sharded_fetch_decode_async left on the device for tsqa_sharded_decode_again_async: the descriptor count and
    // the buffers they refer to.  Zero / null whenever `frames` may hold anything else (every other writer of `frames`, a reallocation).
    uint32_t sharded_n_local = 0;
    const void* sharded_streams = nullptr;
    void* sharded_out = nullptr;
    void forget_sharded() { sharded_n_local = 0; sharded_streams = nullptr; sharded_out = nullptr; }
    tsqa_uploads range_up, batch_up;           // range-read items; batch descriptors
    // batches: per item, the running frame offset of a compress batch across its launches, and the sizes, the offsets of a packed
    // batch (one more than items), the headers the synchronous forms read back and the item statuses of the synchronous decompress
    tsqa_scratch<int32_t> batch_status;
    tsqa_scratch<uint64_t> batch_at, batch_sizes, batch_offsets;
    tsqa_scratch<uint8_t> batch_heads;
    // the item table that tsqa_decompress_batch_packed_dense_async makes on the device, and the block count of its fitting items
    tsqa_scratch<tsq::BatchItem> batch_items;
    tsqa_scratch<uint32_t> batch_live;
    // every packed compress, host-planned or from device tables: the block descriptors made on the device (batch_enc_blocks_kernel)
    // and, per encode launch, the item that holds the launch's first block
    tsqa_scratch<tsq::EncBatchBlock> table_blocks;
    tsqa_scratch<uint32_t> table_launch_item;
    // and, per block descriptor, the item it belongs to: step 3 of the pack scan (batch_pack_scan_packed_body) places each frame from it
    tsqa_scratch<uint32_t> table_block_item;
    // tsqa_join_async: where each item's body starts in the joined container (one more than items)
    tsqa_scratch<uint64_t> join_at;
    // tsqa_cut_async and tsqa_cut_items_async (tsq_cut.cuh): per range its source place and its header's fields (one more than
    // ranges: where the written output ends), and per group of 256 ranges the sum of its padded sizes, then its base
    tsqa_scratch<tsq::CutRange> cut_ranges;
    tsqa_scratch<uint64_t> cut_groups;
    // tsqa_gather_async (tsq_gather.cuh): per range its place and piece count; per piece slot -- cap_pieces of them -- the item as
    // it is cut and as it is sorted (two halves of gather_items), the key and the slot number in front of and behind the sort (two
    // halves each); one group per block that can be touched; the sort's temporary storage, asked for gather_sort_n pairs; the words
    tsqa_scratch<tsq::GatherRange> gather_ranges;
    tsqa_scratch<tsq::RangeItem> gather_items;
    tsqa_scratch<uint64_t> gather_keys;
    tsqa_scratch<uint32_t> gather_slots;
    tsqa_scratch<tsq::BlockGroup> gather_groups;
    tsqa_scratch<uint8_t> gather_sort;
    tsqa_scratch<tsq::GatherWords> gather_words;
    // tsqa_gather_rows_async (tsq_rows.cuh) on top of those: per row its place, k * row_stride, and per group of 256 rows its pieces
    tsqa_scratch<uint64_t> gather_places;
    tsqa_scratch<uint64_t> gather_row_groups;
    size_t gather_sort_n = 0, gather_sort_bytes = 0;
    // tsqa_records_async (tsq_records.cuh): the bit map of the delimiters, (total >> 6) + n_blocks + 1 words -- an eighth of the
    // data and 8 bytes per block --, per block its record starts and edges, per group of 256 blocks their sum and their last edge
    // (two halves of records_groups), and the call's words
    tsqa_scratch<uint64_t> records_map;
    tsqa_scratch<tsq::RecordBlock> records_blocks;
    tsqa_scratch<uint64_t> records_groups;
    tsqa_scratch<tsq::RecordWords> records_words;
    // tsqa_find_async (tsq_find.cuh) uses the records' scratch -- the map holds the hits' ends, cleared per call like the records'
    // -- and beside it 32 bytes per block for the blocks' first and last 15 bytes, and two words for the scan's count
    tsqa_scratch<uint8_t> find_edges;
    tsqa_scratch<uint64_t> find_need;
    // tsqa_crc32_async (tsq_crc.cuh): the call's word, then one word per block, R of the block; cleared per call
    tsqa_scratch<uint32_t> crc_blocks;
    char probe_shape[160] = {0};               // what tsqa_measure_copy chose (tsqa_copy_probe_shape)
    tsqa_scratch<uint32_t> duo_ring;           // two-workgroup decoder: chunk records handed from the PARSE to the COPY workgroup of a block
    tsqa_scratch<uint32_t> duo_flags;          // and their progress counters
    tsqa_scratch<uint64_t> d_size;             // result words of the synchronous entry points
    tsqa_scratch<int32_t> d_status;
    int enc_variant = 0, dec_variant = 0;
    uint32_t decode_wait_limit = 1u << 24;   // polls before a multi-workgroup decode gives up on a sibling workgroup (TSQA_ERR_STALL)
    char err[256] = {0};
    // optional timing (tsqa_profile_*): HIP event pairs on the launch stream, taken from a pool made when profiling is
    // switched on (nothing is created or destroyed between the events).  Kinds: 0 encode kernel, 1 decode kernel,
    // 2 whole compress call (encode + container pack), 3 whole decompress call (frame walk + decode), 4 the join's copy kernel,
    // 5 the cut's copy kernel (tsqa_cut_async and tsqa_cut_items_async), 6 the gather's planner (its launches in front of the decode), 7 the decode kernel of a record read
    // (tsqa_decompress_item_ranges_async, tsqa_gather_async and tsqa_gather_rows_async, whose planner is kind 6 too), 8 the pad kernel
    // of tsqa_gather_rows_async, 9 the mark decode of tsqa_records_async (dec_mark_kernel), 10 its table launches (tsq_records.cuh),
    // 11 the find decode of tsqa_find_async (dec_find_kernel), 12 its seam and table launches (tsq_find.cuh),
    // 13 the CRC decode of tsqa_crc32_async (dec_crc_kernel), 14 its fold and close launches (tsq_crc.cuh).
    static constexpr int kProfKinds = 15, kProfPairs = 256;
    bool profiling = false;
    std::vector<hipEvent_t> prof_pool;                     // kProfKinds * kProfPairs * 2 events
    uint32_t prof_used[kProfKinds] = {0};

    void set_error(const char* fmt, ...) __attribute__((format(printf, 2, 3)));
    // what a growing reserve waits for before it frees scratch: the context's own stream and `s`, the stream the call was given
    void wait_for(hipStream_t s) { (void)hipStreamSynchronize(stream); if (s && s != stream) (void)hipStreamSynchronize(s); }
    int reserve(size_t n_blocks, bool want_tables, bool want_slots = true, bool all_streams = false, hipStream_t s = nullptr);
    int reserve_duo(size_t n_blocks, hipStream_t s = nullptr);
    int reserve_host_frames(size_t n);
    int reserve_batch(size_t n_items);
    int reserve_tables(size_t n_blocks, size_t n_launches, bool want_items = false);
    int reserve_join(size_t n_items);
    int reserve_cut(size_t n_ranges);
    int reserve_gather(size_t n_ranges, size_t cap_pieces, size_t cap_groups);
    int reserve_records(size_t map_words, size_t n_blocks);
    int reserve_find(size_t map_words, size_t n_blocks);
    int reserve_crc(size_t n_blocks);
    // `readable` >= n: bytes of d_in that may be read (look-ahead halo); zeros are seen beyond it
    int launch_encode(const void* d_in, size_t n, size_t readable, uint32_t ext, int32_t* status, hipStream_t s);
    // general form: block b at d_in + b * stride, streams to slots_out[b * TSQ_OUTPUT_SZ], sizes to sizes_out[b]
    int launch_encode_to(const void* d_in, size_t n, size_t readable, size_t stride, uint32_t ext, uint8_t* slots_out,
                         uint32_t* sizes_out, int32_t* status, hipStream_t s);
    // (variant < 0: the context's decode variant; decode_again passes 4 -- one workgroup per block -- without touching the context's
    //  setting, which other threads of the scheduler read)
    int launch_decode_frames(const void* d_streams, const tsq::FrameInfo* d_frames, uint32_t n_blocks, void* d_out, int32_t* status, hipStream_t s, int variant = -1);
    // After *status came back TSQA_ERR_STALL (a sibling workgroup of a several-workgroups-per-block decode did not get onto the GPU in
    // time; the frames are not at fault): clear *status and decode the same frames again with one workgroup per block, which waits for
    // nobody.
    int decode_again(const void* d_streams, const tsq::FrameInfo* d_frames, uint32_t n_blocks, void* d_out, int32_t* status, hipStream_t s);
    int launch_pack(size_t n, uint32_t ext, void* d_out, size_t out_cap, uint64_t* d_out_size, int32_t* status, hipStream_t s);
};

template <class T> bool tsqa_scratch<T>::grow(tsqa_ctx* c, size_t n)
{
    if (!needs(n)) return true;
    reset();
    const hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) { p = nullptr; c->set_error("hipMalloc of %zu B failed: %s", n * sizeof(T), hipGetErrorString(e)); return false; }
    cap = n;
    return true;
}

// A container's frame table, kept for range reads (tsqa_index_create), or the frame table of a batch of containers in one buffer
// (tsqa_index_create_batch): the healthy items' blocks one after the other, stream_at relative to the buffer.  The containers
// themselves are the caller's.  Or the frame table of a container of short blocks, made on the device from its table of stream
// sizes (tsqa_index_create_sized*): out_start is the caller's geometry, host_frames stays empty, and `verdict` says on the device
// whether the container has that geometry.
struct tsqa_index {
    int device = 0;
    const uint8_t* container = nullptr;
    size_t n = 0;
    uint32_t n_blocks = 0;
    uint64_t total = 0;
    tsq::FrameInfo* frames = nullptr;          // n_blocks descriptors on the device (frame_walk_kernel)
    // a sized index only, in the allocation of `frames` behind the descriptors: the group sums of its walk (tsq_index.cuh), which
    // is why two creations on one stream do not share them, and the walk's verdict, which gates every read (NULL otherwise)
    uint64_t* group_sum = nullptr;
    int32_t* verdict = nullptr;
    // tsqa_gather_async: log2 of a sized index's block_len (0 otherwise: the block of a byte is found by bisection), and, for a batch
    // index, item_first on the device (n_items + 1; NULL for an index of one item, which owns every block)
    uint32_t block_shift = 0;
    uint64_t* d_item_first = nullptr;
    // a batch index made on the device (tsqa_index_create_packed*, tsq_index_packed.cuh): `frames` holds cap_blocks descriptors, and
    // behind d_item_first in its allocation lie each item's start in the concatenation (n_items), the words {blocks, total, blocks
    // needed} and the item statuses.  Until tsqa_index_fetch the host tables below are empty, n_blocks and total are 0, and
    // pending_items says how many items the device tables describe (0: any other index, or fetched).
    uint32_t cap_blocks = 0, pending_items = 0, packed_block_len = 0;
    uint64_t* d_item_at = nullptr;
    uint64_t* d_words = nullptr;
    int32_t* d_item_status = nullptr;
    std::vector<tsqa_frame> host_frames;       // their host copy
    std::vector<uint64_t> out_start;           // n_blocks + 1: where each block's output starts, then the total
    // items (one for a single container): item i owns the blocks [item_first[i], item_first[i + 1]), none when it was refused
    std::vector<uint64_t> item_first;          // n_items + 1
    std::vector<int32_t> item_status;          // TSQA_OK or TSQA_ERR_FORMAT
};
