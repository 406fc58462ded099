/*
 * turbosqueeze_amd.h -- C ABI of libturbosqueeze_amd.so, the MI355X (gfx950) implementation
 * of turbosqueeze's per-block encode/decode hot path.
 *
 * Plain C: pointers, sizes and function pointers only.  Two groups of entry points:
 *
 *  (1) the reference's own block-codec and scheduler API, same names, argument meaning and
 *      error behaviour as /root/reference/turbosqueeze.h:441-674, so that a program built
 *      against the reference links against this library instead.  The two reference functions
 *      that take std::function are additionally exported as tsqa_*_cb twins with C function
 *      pointers (for cgo / ctypes / JNI callers); the std::function forms themselves are
 *      declared in include/turbosqueeze.h (C++).
 *
 *  (2) tsqa_* device-resident entry points: the same path with input and output already in
 *      HBM (what bench.py times, and what a GPU-side consumer of .tsq data would bind).
 *
 * Every call runs hand-written HIP kernels; there is no CPU fallback.  If no gfx950 device is
 * usable the calls fail (tsqa_* return TSQA_ERR_NO_DEVICE, the tsq* forms report failure the way
 * the reference reports a failed job) -- they never compute on the host.
 */
#ifndef TURBOSQUEEZE_AMD_H
#define TURBOSQUEEZE_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- format constants (reference turbosqueeze.h:37-43) ---- */
#ifndef TSQ_BLOCK_BITS
#define TSQ_BLOCK_BITS (22)
#define TSQ_BLOCK_SZ   (1 << TSQ_BLOCK_BITS)
#define TSQ_OUTPUT_SZ  ((1 << TSQ_BLOCK_BITS) + (1 << (TSQ_BLOCK_BITS - 2)))
#define TSQ_HASH_BITS  (17)
#define TSQ_HASH_SZ    ((1 << TSQ_HASH_BITS) * sizeof(uint16_t))
#define TSQ_HASH_MASK  ((1 << TSQ_HASH_BITS) - 1)
#endif

/* ---- status codes of the tsqa_* entry points ---- */
enum {
    TSQA_OK            = 0,
    TSQA_ERR_NO_DEVICE = 1,   /* no usable HIP device / kernels not loadable */
    TSQA_ERR_HIP       = 2,   /* a HIP runtime call failed (tsqa_last_error has the text) */
    TSQA_ERR_ARG       = 3,   /* null pointer, zero size, capacity too small */
    TSQA_ERR_FORMAT    = 4,   /* bad magic, n_blocks == 0, frame size 0 or > TSQ_OUTPUT_SZ, truncated */
    TSQA_ERR_STREAM    = 5,   /* a block stream is malformed (bad offset, overrun) */
    TSQA_ERR_OVERFLOW  = 6,   /* a block expanded beyond TSQ_OUTPUT_SZ */
    TSQA_ERR_STALL     = 7    /* a decode on several workgroups per block gave up waiting for a sibling workgroup (the GPU was busy
                                 with other work for seconds): the container may be fine.  The synchronous entry points and the
                                 reference-named API decode again on one workgroup per block by themselves; the stream-ordered
                                 (*_async) entry points report it in *d_status -- decode again with decode variant 4 */
};

/* =====================================================================================
 * (2) Device-resident path
 * ================================================================================== */

typedef struct tsqa_ctx tsqa_ctx;   /* one per (process, device): streams + scratch in HBM */

/* device < 0: use the current HIP device.  Scratch is grown on demand and kept.
 * A context owns ONE set of scratch buffers (block slots, sizes, frame tables): calls on the same context must be
 * ordered on one stream at a time -- issue the next call on the same stream, or after the previous one has drained.
 * Two streams that want to run concurrently take two contexts.
 * Every *_async call reports into the status, size and table words it was GIVEN (d_status, d_out_size, d_sizes, d_offsets), and a
 * later call never clears an earlier call's words unless the caller passes the same ones (the Python DeviceCodec passes one shared
 * word to every call, so its status() is the last call's). */
int         tsqa_create(int device, tsqa_ctx **out);
void        tsqa_destroy(tsqa_ctx *ctx);
const char *tsqa_last_error(const tsqa_ctx *ctx);
int         tsqa_device_id(const tsqa_ctx *ctx);

/* ceil(n / TSQ_BLOCK_SZ): the job split of tsq_threads.cpp:313. */
size_t tsqa_block_count(size_t n);
/* Capacity that always holds the container of an n-byte input:
 * 16 + n_blocks * (3 + TSQ_OUTPUT_SZ)  (tsq_threads.cpp:339). */
size_t tsqa_container_bound(size_t n);

/* What this library was compiled as: a static string of the form
 *   "arch=gfx950 timing_only=0 instrumented=0 ab_variants=0 lm=4 lf=3 records=11 [switches: none]"
 * timing_only = 1 means a TSQ_X_* switch that gives WRONG streams on purpose (an experiment library, csrc/tsq_experiment.h);
 * the product library always reports timing_only=0 instrumented=0 and "switches: none" (tests/test_abi_cpu.py asserts it). */
const char* tsqa_build_info(void);

/*
 * Compress n bytes resident at d_in into a complete .tsq container at d_out
 * (header "TSQ1" | u32 n_blocks | u64 n, then per block u24 (size | ext<<23) + stream;
 * turbosqueeze.cpp:64-83).  Replaces the loop tsqInit + tsqEncode over all blocks
 * (tsq_threads.cpp:176-177) plus the writer's frame assembly (tsq_threads.cpp:218-239).
 * Bytes past d_in[n-1] are never read: the encoder's look-ahead beyond the input end sees
 * zeros (canonical conditions).  Work is enqueued on `hip_stream` (a hipStream_t, NULL =
 * the context's own stream); the call returns after the stream has drained and *out_size
 * holds the container size.
 */
int tsqa_compress_device(tsqa_ctx *ctx, const void *d_in, size_t n,
                         void *d_out, size_t out_cap, size_t *out_size,
                         uint32_t ext, void *hip_stream);

/* Asynchronous form: nothing is waited for; the container size lands in *d_out_size
 * (a device uint64).  Used by bench.py so that HIP events see only kernel time. */
int tsqa_compress_device_async(tsqa_ctx *ctx, const void *d_in, size_t n,
                               void *d_out, size_t out_cap, uint64_t *d_out_size,
                               int32_t *d_status, uint32_t ext, void *hip_stream);

/*
 * Decompress a .tsq container resident at d_in (n bytes) into d_out.  Replaces the frame
 * walk (tsq_threads.cpp:513-524) + tsqDecode per block (tsq_threads.cpp:590) + the ordered
 * writer (tsq_threads.cpp:648).  *out_size = header total.  Fails with TSQA_ERR_FORMAT /
 * TSQA_ERR_STREAM instead of over-running like tsq_decode.cpp does on corrupt input.
 */
int tsqa_decompress_device(tsqa_ctx *ctx, const void *d_in, size_t n,
                           void *d_out, size_t out_cap, size_t *out_size,
                           void *hip_stream);

/* Asynchronous form: the caller states n_blocks (the header's count, which the host cannot
 * read without a sync); the frame-walk kernel checks it against the header.  *d_status
 * (device int32) becomes nonzero (a TSQA_ERR_*) on a bad container or stream; the total
 * uncompressed size lands in *d_out_size. */
int tsqa_decompress_device_async(tsqa_ctx *ctx, const void *d_in, size_t n, uint32_t n_blocks,
                                 void *d_out, size_t out_cap, uint64_t *d_out_size,
                                 int32_t *d_status, void *hip_stream);

/*
 * Sharded operation: blocks are independent, so a job can be cut across devices or ranks --
 * block i -> worker i % num_cores in the reference (tsq_threads.cpp:71,463).  These two entry points work on
 * whatever subset of a job's blocks a device owns and leave the gather (frames in block order,
 * tsq_threads.cpp:192-275; blocks at their offsets, :648) to the caller.
 *
 * tsqa_encode_blocks_async: block b of the call is read at d_in + b * stride; every block is TSQ_BLOCK_SZ long
 * except the last (last_len), and each is IMMEDIATELY followed by its look-ahead bytes (the first 128 bytes of
 * the block that follows it in the job; zeros after the job's last block) -- so stride = TSQ_BLOCK_SZ for one
 * contiguous buffer, TSQ_BLOCK_SZ + 128 for a shard that holds every N-th block.  With a stride in between, the call's last block
 * sees stride - TSQ_BLOCK_SZ look-ahead bytes, then zeros; with stride = TSQ_BLOCK_SZ it sees zeros, whatever follows the buffer.
 * What lies behind those bytes changes no stream.  Stream b lands at
 * d_slots + b * TSQ_OUTPUT_SZ, its size in d_sizes[b] (both device memory).  Replaces tsqInit + tsqEncode per
 * owned block (tsq_threads.cpp:176-177).
 */
int tsqa_encode_blocks_async(tsqa_ctx *ctx, const void *d_in, uint32_t n_blocks, size_t stride, uint32_t last_len,
                             uint32_t ext, void *d_slots, uint32_t *d_sizes, int32_t *d_status, void *hip_stream);

/* One block stream to decode: where it starts (relative to d_streams), where its bytes go (relative to d_out). */
typedef struct tsqa_frame {
    uint64_t stream_at;   /* first byte of the block stream (the u24 size header) */
    uint64_t out_at;      /* where the decoded block goes */
    uint32_t stream_len;  /* frame & 0x7FFFFF (tsq_threads.cpp:513-517) */
    uint32_t ext;         /* frame >> 23 */
    uint32_t out_len;     /* the stream's u24 header: decoded bytes (<= TSQ_BLOCK_SZ) */
    uint32_t pad;
} tsqa_frame;

/* tsqa_decode_blocks_async: decode n_blocks streams described by d_frames (device memory).  Replaces tsqDecode
 * per owned block (tsq_threads.cpp:590).  *d_status becomes TSQA_ERR_STREAM on a malformed stream.
 * Trust: the descriptors may be taken from an untrusted container.  The kernels refuse (TSQA_ERR_STREAM) a stream_len
 * below 3 or above TSQ_OUTPUT_SZ and an out_len above TSQ_BLOCK_SZ, and never read a stream beyond stream_len bytes nor write
 * a block beyond out_len bytes.  stream_at and out_at are the CALLER's responsibility: stream_at + stream_len must lie inside
 * d_streams and out_at + out_len inside d_out (the library has no way to know the sizes of those allocations). */
int tsqa_decode_blocks_async(tsqa_ctx *ctx, const void *d_streams, const tsqa_frame *d_frames, uint32_t n_blocks,
                             void *d_out, int32_t *d_status, void *hip_stream);

/* The gather / scatter that goes with them: one DMA per owned block between its slot in HBM (b * TSQ_OUTPUT_SZ) and
 * its frame in a container in HOST memory (pinned or hipHostRegister'ed for full DMA speed).  frame_at[b] is the
 * container offset of block b's three frame bytes (16 + sum over earlier blocks of 3 + size); sizes and frame_at are
 * host arrays.  to_host also writes the frame bytes (size | ext << 23, tsq_threads.cpp:218-219).  Both check every size (3 to
 * TSQ_OUTPUT_SZ) before the first byte is written or the first copy enqueued, as tsqa_sharded_place_async does: a refusal
 * (TSQA_ERR_ARG from to_host, TSQA_ERR_FORMAT from from_host) leaves the host container and d_streams as they were. */
int tsqa_frames_to_host_async(tsqa_ctx *ctx, const void *d_slots, const uint32_t *sizes, const uint64_t *frame_at,
                              uint32_t n_blocks, uint32_t ext, void *host_container, void *hip_stream);
int tsqa_frames_from_host_async(tsqa_ctx *ctx, const void *host_container, const uint64_t *frame_at, const uint32_t *sizes,
                                uint32_t n_blocks, void *d_streams, void *hip_stream);

/* Kernel timing for bench.py: when enabled, every encode / decode kernel launch is bracketed by
 * HIP events recorded on the stream it is launched on (up to 256 launches are kept).
 * tsqa_profile_read waits for those events and returns, per kernel, the summed elapsed
 * milliseconds and the number of launches since the last read. */
int tsqa_profile_enable(tsqa_ctx *ctx, int on);
int tsqa_profile_read(tsqa_ctx *ctx, double *encode_ms, uint32_t *encode_launches,
                      double *decode_ms, uint32_t *decode_launches);
/* The same for whole calls: tsqa_compress_device_async (encode kernel + container pack) and
 * tsqa_decompress_device_async (frame walk + decode kernel). */
int tsqa_profile_read_calls(tsqa_ctx *ctx, double *compress_ms, uint32_t *compress_calls,
                            double *decompress_ms, uint32_t *decompress_calls);
/* The same for the copy kernel of tsqa_join_async alone (its other launches are short and lie outside the span). */
int tsqa_profile_read_join(tsqa_ctx *ctx, double *emit_ms, uint32_t *emit_launches);
/* The same for the copy kernel of tsqa_cut_async alone. */
int tsqa_profile_read_cut(tsqa_ctx *ctx, double *emit_ms, uint32_t *emit_launches);
/* The same for record reads: the planner of tsqa_gather_async (its launches in front of the decode, as one span per call) and
 * the decode kernel of a record read (tsqa_decompress_item_ranges_async and tsqa_gather_async). */
int tsqa_profile_read_gather(tsqa_ctx *ctx, double *plan_ms, uint32_t *plan_calls, double *decode_ms, uint32_t *decode_launches);
/* The pad kernel of tsqa_gather_rows_async (its planner and decode are counted by tsqa_profile_read_gather). */
int tsqa_profile_read_rows(tsqa_ctx *ctx, double *pad_ms, uint32_t *pad_launches);
/* tsqa_records_async: its mark decode (the decoder that writes one bit per byte) and, per call, its table launches together. */
int tsqa_profile_read_records(tsqa_ctx *ctx, double *mark_ms, uint32_t *mark_launches, double *table_ms, uint32_t *table_calls);
/* tsqa_find_async: its find decode (the decoder that compares with the needle) and, per call, its seam and table launches together. */
int tsqa_profile_read_find(tsqa_ctx *ctx, double *find_ms, uint32_t *find_launches, double *table_ms, uint32_t *table_calls);
/* tsqa_crc32_async: its CRC decode (the decoder that checksums) and, per call, its fold and close launches together. */
int tsqa_profile_read_crc(tsqa_ctx *ctx, double *decode_ms, uint32_t *decode_launches, double *fold_ms, uint32_t *fold_calls);

/* One step of a block-sharded job on one rank (block b of the job belongs to rank b % world; what bench.py --gpus N and
 * turbosqueeze_amd/sharding.py run).  The only exchange between ranks is the all-gather of the u32 stream sizes, made by the
 * caller (torch.distributed / RCCL); everything else is here, one call per side:
 *
 * tsqa_frame_offsets / tsqa_walk_frames: host-only helpers (no device): the writer's prefix sum of 3 + size
 *   (tsq_threads.cpp:226-239) and the reader's frame walk with validation (tsq_threads.cpp:513-524) over a container in host
 *   memory.  TSQA_ERR_FORMAT on a malformed container.
 * tsqa_sharded_place_async: after tsqa_encode_blocks_async and the all-gather, every owned stream (block b's at
 *   d_slots + (b / world) * TSQ_OUTPUT_SZ) goes by DMA to its final place in ONE container in host memory, with its three
 *   frame bytes; rank 0 also writes the 16-byte header.  *container_size is the same on every rank.
 * tsqa_sharded_fetch_decode_async: walks the container, brings this rank's frames back to d_streams (k-th owned frame at
 *   k * TSQ_OUTPUT_SZ) and decodes them back to back into d_out (k-th owned block at k * TSQ_BLOCK_SZ).  The container is not
 *   trusted: its whole frame walk is validated against container_size and against streams_cap / out_cap (the bytes the two device
 *   buffers hold) before any copy is enqueued; TSQA_ERR_FORMAT otherwise, with nothing written.
 * Both replace the Python loops of round 2's sharding.py; the host container should be pinned / hipHostRegister'ed. */
int tsqa_frame_offsets(const uint32_t *sizes, uint32_t n_blocks, uint64_t *frame_at, uint64_t *container_size);
int tsqa_walk_frames(const void *container, size_t size, uint32_t cap_blocks, uint64_t *frame_at, uint32_t *sizes, uint32_t *ext,
                     uint32_t *out_len, uint32_t *n_blocks, uint64_t *total);
int tsqa_sharded_place_async(tsqa_ctx *ctx, const void *d_slots, const uint32_t *all_sizes, uint32_t n_blocks, uint64_t n_total,
                             uint32_t rank, uint32_t world, uint32_t ext, void *host_container, size_t host_cap,
                             uint64_t *container_size, void *hip_stream);
int tsqa_sharded_fetch_decode_async(tsqa_ctx *ctx, const void *host_container, size_t container_size, uint32_t rank, uint32_t world,
                                    void *d_streams, size_t streams_cap, void *d_out, size_t out_cap, int32_t *d_status, uint64_t *total,
                                    void *hip_stream);
/* When *d_status of tsqa_sharded_fetch_decode_async reads TSQA_ERR_STALL: the owned frames and their descriptors are still on the
 * device; this decodes them again with one workgroup per block (which waits for nobody) and reports in *d_status again. */
int tsqa_sharded_decode_again_async(tsqa_ctx *ctx, const void *d_streams, void *d_out, int32_t *d_status, void *hip_stream);

/* The measured copy bandwidth of this GPU (bytes read + bytes written per second, GB/s = 1e9 B/s) by a plain
 * grid-stride 16-byte copy kernel over `bytes` of HBM: the second denominator beside the 8 TB/s specification when a
 * kernel is priced against the HBM roofline. */
int tsqa_measure_copy(tsqa_ctx *ctx, size_t bytes, int reps, double *best_gbps, double *median_gbps);
/* which launch shape the last tsqa_measure_copy on this context chose (text; "" before the first probe) */
const char *tsqa_copy_probe_shape(const tsqa_ctx *ctx);

/* Kernel variant selection.  Encoder: 0 = default (staged encoder, one workgroup of fourteen working wavefronts per block; its lean layout -- twelve -- by itself when there are
 * more blocks than CUs), 1 = serial kernel (one lane walks the block; correctness baseline), 6 = force the lean layout
 * (two blocks per CU), 7 = never lean.  Decoder: 0 = default (byte-lane decoder; on two workgroups per block when a
 * launch has at most half as many blocks as the device has CUs, three -- two of them parsing alternate windows of the stream --
 * when it has at most a third), 1 = serial kernel, 3 = several workgroups per block whatever the block count (three when the
 * CUs allow), 4 = always one, 5 = always three, 6 = always two.  The previous round's production encoder (encoder 5) exists only in the A/B library
 * built by `make ab`; the product library rejects it. */
void tsqa_set_kernel_variant(tsqa_ctx *ctx, int encode_variant, int decode_variant);
/* How many polls (of ~0.1 us) a decode on several workgroups per block waits for a sibling workgroup before it reports
 * TSQA_ERR_STALL (default 2^24: seconds).  Tests set it to 1 to exercise the retry. */
void tsqa_set_decode_wait_limit(tsqa_ctx *ctx, uint32_t polls);

/*
 * Range reads: bytes [offset, offset + length) of a container's uncompressed data, straight from the container in HBM.  Blocks
 * are independent, so a read decodes only the blocks it touches, and each of them only up to the chunk that reaches the read's
 * last byte there: its cost grows with how far the read reaches into its last block, not with the size of the container.
 *
 * tsqa_index_create: synchronous (on the context's own stream; the container's bytes must be in place).  Validates the container
 *   (magic, block count, every frame, sizes that add up to the header's total) and keeps its frame table, on the device and a host
 *   copy.  TSQA_ERR_FORMAT on a malformed container, and no index is made.  The index refers to the container: it must stay alive
 *   and unchanged while the index is used.  An index belongs to the device of the context it was made on.
 * tsqa_index_destroy: no read that uses the index may still be in flight.
 */
typedef struct tsqa_index tsqa_index;
int      tsqa_index_create(tsqa_ctx *ctx, const void *d_container, size_t n, tsqa_index **out);
void     tsqa_index_destroy(tsqa_index *idx);
uint32_t tsqa_index_blocks(const tsqa_index *idx);   /* the container's block count (0 for NULL) */
uint64_t tsqa_index_total(const tsqa_index *idx);    /* its uncompressed size (0 for NULL) */

typedef struct tsqa_range { uint64_t offset, length, out_at; } tsqa_range;      /* bytes [offset, offset+length) -> d_out + out_at */
typedef struct tsqa_range_item { uint32_t block, lo, hi, pad; uint64_t out_at; } tsqa_range_item;   /* block bytes [lo, hi) -> d_out + out_at */

/* Host-only (no device): cut ranges into one item per block they touch, given the blocks' output starts out_start[0..n_blocks]
 * (out_start[0] = 0, then the prefix sum of the blocks' lengths; a block may be shorter than TSQ_BLOCK_SZ anywhere).  Items come
 * in range order; zero-length ranges give none.  *n_items = the item count.  TSQA_ERR_ARG, with nothing written to items, when a
 * range ends past out_start[n_blocks], when out_at + length > out_cap, when the destinations of two ranges overlap, or when the
 * items do not fit cap_items (*n_items then holds the count needed). */
int tsqa_plan_ranges(const uint64_t *out_start, uint32_t n_blocks, const tsqa_range *ranges, uint32_t n_ranges,
                     size_t out_cap, tsqa_range_item *items, uint32_t cap_items, uint32_t *n_items);

/* Read the ranges (a host array) into d_out (out_cap bytes), on hip_stream (NULL = the context's own).  The ranges are planned
 * (tsqa_plan_ranges) before anything is enqueued: argument errors are returned, and nothing is written.  *d_status (device int32)
 * becomes nonzero (a TSQA_ERR_*) on a malformed stream.  The asynchronous form returns at once and may be called again on the
 * same stream before the first has run.  tsqa_decompress_ranges waits and returns the status.
 * Trust: a read reports TSQA_ERR_STREAM when a stream byte it consumed is malformed; damage that lies beyond the last chunk a read
 * needs may go unreported.  A read of the whole range consumes every stream and agrees with tsqa_decompress_device.  Nothing
 * outside the ranges' destinations is ever written. */
int tsqa_decompress_ranges_async(tsqa_ctx *ctx, const tsqa_index *idx, const tsqa_range *ranges, uint32_t n_ranges,
                                 void *d_out, size_t out_cap, int32_t *d_status, void *hip_stream);
int tsqa_decompress_ranges(tsqa_ctx *ctx, const tsqa_index *idx, const tsqa_range *ranges, uint32_t n_ranges,
                           void *d_out, size_t out_cap, void *hip_stream);

/*
 * Batches: many independent items in one call.  A batch is one input buffer and one output buffer in HBM plus a host array of
 * items: item i reads bytes [in_at, in_at + in_len) of d_in (in_size bytes) and writes its result to [out_at, out_at + out_cap) of
 * d_out (out_size bytes).  The blocks of all items run side by side, one workgroup each, in launches of at most 2 x CUs blocks, so
 * a batch of small items fills the chip where one call per item holds one CU at a time.
 */
typedef struct tsqa_batch_item { uint64_t in_at, in_len, out_at, out_cap; } tsqa_batch_item;

/* Host-only (no device): validate a batch and give each item's first block in the batch; first_block[n_items] = the batch's
 * block count.  n_blocks == NULL: a compress batch (item i has ceil(in_len / TSQ_BLOCK_SZ) blocks); else a decompress batch with
 * the stated block counts.  TSQA_ERR_ARG, with nothing written, for: no items; an item with in_len == 0; an input range past
 * in_size or an output range past out_size; two output ranges that overlap (input ranges may); compress: out_cap < 16 + 6 * blocks;
 * decompress: in_len < 16, a block count of 0 or above (in_len - 16) / 6. */
int tsqa_plan_batch(const tsqa_batch_item *items, uint32_t n_items, size_t in_size, size_t out_size,
                    const uint32_t *n_blocks, uint64_t *first_block);

/* Compress every item.  Item i's container is byte for byte what tsqa_compress_device gives for its bytes alone: the encoder's
 * look-ahead ends at the item's last byte and never sees the next item.  d_sizes[i] (device) = its container size; when that
 * exceeds out_cap, *d_status (device) becomes TSQA_ERR_OVERFLOW and the frames that do not fit are not written.  Nothing is written
 * outside the items' output ranges, and the other items are complete.  The batch is planned (tsqa_plan_batch) before anything is
 * enqueued.  Encoder variants 0, 6 and 7; the others are refused (TSQA_ERR_ARG).  The asynchronous form returns at once and may be
 * called again on the same stream before the first has run.  tsqa_compress_batch waits, fills sizes (host) and returns
 * TSQA_ERR_OVERFLOW when an item did not fit: retry those items with more room. */
int tsqa_compress_batch_async(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items, uint32_t n_items,
                              uint32_t ext, void *d_out, size_t out_size, uint64_t *d_sizes, int32_t *d_status, void *hip_stream);
int tsqa_compress_batch(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items, uint32_t n_items,
                        uint32_t ext, void *d_out, size_t out_size, uint64_t *sizes, void *hip_stream);

/* Decompress every item (a container) into its output range.  The asynchronous form takes each container's block count (host
 * array n_blocks) and validates each container as tsqa_decompress_device_async validates one: the header with that block count,
 * total <= out_cap, every frame, frame lengths that add up to the total.  d_sizes[i] = the item's uncompressed size, 0 when it was
 * refused; any refusal or malformed stream sets *d_status, and the decode then leaves at once: all or nothing.  TSQA_ERR_STALL as
 * for tsqa_decompress_device_async (decode again with decode variant 4).
 * tsqa_decompress_batch reads every header itself (one gather, one copy), leaves items with a refused header out (item_status:
 * TSQA_ERR_FORMAT, or TSQA_ERR_ARG when the total exceeds out_cap), decodes the rest in one batch, retries once after
 * TSQA_ERR_STALL on one workgroup per block, and when the batch reports a malformed container sends the same items once more
 * through the form with a verdict per item (tsqa_decompress_batch_items_async below): one more launch whatever the item count, and
 * the statuses and sizes come back with one wait.  item_status (host, may be NULL) and sizes (host) per item; every healthy item is
 * delivered; the return value is the largest item status.  Nothing is written outside the items' output ranges. */
int tsqa_decompress_batch_async(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items,
                                const uint32_t *n_blocks, uint32_t n_items, void *d_out, size_t out_size,
                                uint64_t *d_sizes, int32_t *d_status, void *hip_stream);
int tsqa_decompress_batch(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items, uint32_t n_items,
                          void *d_out, size_t out_size, uint64_t *sizes, int32_t *item_status, void *hip_stream);

/* tsqa_decompress_batch_async with a verdict per item, made on the device: a damaged container costs its own item and nothing
 * else.  Arguments as for tsqa_decompress_batch_async, plus d_item_status (device, n_items words).
 *   - Item i's bytes and d_sizes[i] are exactly those of tsqa_decompress_batch_async whenever d_item_status[i] == 0, whatever the
 *     other items are.
 *   - d_item_status[i] is the word that tsqa_decompress_device_async leaves for container i alone with the same block count and
 *     capacity: TSQA_ERR_FORMAT for anything the frame walk refuses (a total above out_cap and, in the packed form, a bad place
 *     included), else the decoder's code for a malformed stream (TSQA_ERR_STREAM), else 0.
 *   - An item refused by the walk has nothing written to its output range.  An item refused by a decoder has undefined contents
 *     in its own range.  Either way d_sizes[i] = 0.  Nothing outside the items' ranges is ever written.
 *   - *d_status = the largest item status.
 *   - TSQA_ERR_ARG before anything is enqueued, with nothing written, as for tsqa_decompress_batch_async; a NULL d_item_status is
 *     one more such error.
 * Every block runs on one workgroup of its own (the decoder of decode variant 4) at any block count: the context's decode variant
 * and wait limit are not looked at, and TSQA_ERR_STALL is never reported.  The several-workgroups decoders end their waits on
 * "another block has reported an error", which means the launch, not the item, so they are not offered here; the price is that a
 * batch with fewer blocks than half the CUs decodes at the one-workgroup latency per block (4.68 against 2.66 ms at 30 blocks of
 * 4 MiB).  Where every item is expected to be healthy and the batch is that small, tsqa_decompress_batch_async is the faster call.
 * tsqa_decompress_batch_packed_items_async: the same for tsqa_decompress_batch_packed_async's arguments; a bad place is that
 * item's TSQA_ERR_FORMAT and is never read. */
int tsqa_decompress_batch_items_async(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items,
                                      const uint32_t *n_blocks, uint32_t n_items, void *d_out, size_t out_size,
                                      uint64_t *d_sizes, int32_t *d_item_status, int32_t *d_status, void *hip_stream);

/*
 * Packed batches: the same compress, with every container's place chosen on the device once its size exists, so that the arena is
 * dense.  The caller gives no out_at / out_cap; the call gives back the places.
 *
 * Layout rule (align: a power of two, 1 to 4096):
 *   offsets[0] = 0
 *   offsets[i + 1] = round_up(offsets[i] + sizes[i], align)     for i + 1 < n_items
 *   offsets[n_items] = offsets[n_items - 1] + sizes[n_items - 1]     (the bytes used: no padding behind the last container)
 * Container i is bytes [offsets[i], offsets[i] + sizes[i]) of the arena.  The padding bytes between containers are never written.
 *
 * tsqa_batch_bound: host only.  Room that always holds the container of an n-byte item, much tighter than tsqa_container_bound below
 *   a block: 16, then per block 3 + min(TSQ_OUTPUT_SZ, 11 + k + k/8 + k/2) for its k bytes.  The sum over a batch's items (plus
 *   align - 1 per item) always holds its packed arena.
 * tsqa_plan_packed: host only.  The rule above: sizes[n_items] -> offsets[n_items + 1].  TSQA_ERR_ARG for n_items == 0, an align
 *   that is not a power of two from 1 to 4096, or a NULL pointer.
 */
size_t tsqa_batch_bound(size_t n);
int    tsqa_plan_packed(const uint64_t *sizes, uint32_t n_items, uint32_t align, uint64_t *offsets);

/* Compress every item into a dense arena.  items: in_at and in_len as for tsqa_compress_batch_async (input ranges may overlap);
 * out_at and out_cap are ignored.  Container i is byte for byte what tsqa_compress_device gives for item i alone, at d_out +
 * offsets[i].  d_offsets (device, n_items + 1) and d_sizes (device, n_items) follow the layout rule and are always complete and
 * correct for every item, also when the arena is too small.  Overflow: a frame is written only if it ends at or before out_size,
 * and nothing at or past d_out + out_size is ever written; when offsets[n_items] > out_size, *d_status (device) becomes
 * TSQA_ERR_OVERFLOW, every item that lies wholly inside out_size is complete and exact, and a retry with offsets[n_items] bytes of
 * room succeeds.  TSQA_ERR_ARG before anything is enqueued, with nothing written, for: a NULL pointer, n_items == 0, an empty item,
 * an input range past in_size, a bad align, out_size < 16.  Encoder variants 0, 6 and 7; the others are refused (TSQA_ERR_ARG).
 * The asynchronous form returns at once and may be called again on the same stream before the first has run (a call that needs
 * more scratch than any before it, more items or more blocks per launch, first waits for the device, then grows the scratch).
 * tsqa_compress_batch_packed waits, fills offsets and sizes (host) and returns TSQA_ERR_OVERFLOW, with both tables filled, when
 * the arena was too small. */
int tsqa_compress_batch_packed_async(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items, uint32_t n_items,
                                     uint32_t ext, uint32_t align, void *d_out, size_t out_size, uint64_t *d_offsets,
                                     uint64_t *d_sizes, int32_t *d_status, void *hip_stream);
int tsqa_compress_batch_packed(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items, uint32_t n_items,
                               uint32_t ext, uint32_t align, void *d_out, size_t out_size, uint64_t *offsets, uint64_t *sizes,
                               void *hip_stream);

/* tsqa_decompress_batch_async with each container's place read on the device: container i is bytes [d_offsets[i], d_offsets[i] +
 * d_sizes[i]) of d_arena (both tables in device memory, as tsqa_compress_batch_packed_async leaves them: the two calls chain on one
 * stream with no host read between them).  items (host): out_at and out_cap are used, in_at and in_len ignored; n_blocks (host) as
 * for tsqa_decompress_batch_async.  The tables are not trusted: an item with offsets[i] + sizes[i] > arena_size, sizes[i] < 16 or a
 * block count that sizes[i] bytes cannot hold is refused on the device like a malformed container (TSQA_ERR_FORMAT in *d_status,
 * d_out_sizes[i] = 0, all or nothing) and is never read.  The host checks the output ranges (inside out_size, no overlap) and
 * n_blocks[i] >= 1: TSQA_ERR_ARG.  TSQA_ERR_STALL as for tsqa_decompress_batch_async. */
int tsqa_decompress_batch_packed_async(tsqa_ctx *ctx, const void *d_arena, size_t arena_size, const uint64_t *d_offsets,
                                       const uint64_t *d_sizes, const tsqa_batch_item *items, const uint32_t *n_blocks,
                                       uint32_t n_items, void *d_out, size_t out_size, uint64_t *d_out_sizes, int32_t *d_status,
                                       void *hip_stream);
int tsqa_decompress_batch_packed_items_async(tsqa_ctx *ctx, const void *d_arena, size_t arena_size, const uint64_t *d_offsets,
                                             const uint64_t *d_sizes, const tsqa_batch_item *items, const uint32_t *n_blocks,
                                             uint32_t n_items, void *d_out, size_t out_size, uint64_t *d_out_sizes,
                                             int32_t *d_item_status, int32_t *d_status, void *hip_stream);

/*
 * Dense decompress of a packed batch that takes nothing about the items from the host: block counts and output places are made on
 * the device from the 16 header bytes of each container, and the items land one after the other in d_out.  What a consumer that
 * only received an arena and its two tables needs (another rank, a file staged into device memory, an earlier pipeline stage).
 *
 * Layout rule: tsqa_plan_packed's, applied to the uncompressed sizes (align: a power of two, 1 to 4096):
 *   out_offsets[0] = 0;  out_offsets[i + 1] = round_up(out_offsets[i] + total_i, align) for i + 1 < n_items;  the last entry is not
 *   rounded: out_offsets[n_items] = the bytes needed.  first_block[0] = 0;  first_block[i + 1] = first_block[i] + blocks_i:
 *   first_block[n_items] = the blocks needed.  An item refused at its header counts as total 0, blocks 0.  Item i's data is
 *   d_out[out_offsets[i], out_offsets[i] + out_sizes[i]); padding bytes are never written.
 *
 * tsqa_plan_dense: host only.  The rule above from totals[] and blocks[] (blocks[i] == 0: a refused item, its total is not looked
 *   at) -> out_offsets[n_items + 1], first_block[n_items + 1].  *n_fit = the index of the first accepted item that does not fit
 *   cap_blocks blocks and out_size bytes, n_items when all do.  TSQA_ERR_ARG for a NULL pointer, n_items == 0 or a bad align.
 *
 * tsqa_decompress_batch_packed_dense_async: d_offsets, d_sizes (device, n_items) place the containers in d_arena, as
 * tsqa_compress_batch_packed_async leaves them; nothing in them or in the arena is trusted.  Per item, on the device:
 *   1. Place: sizes[i] <= arena_size, offsets[i] <= arena_size - sizes[i], sizes[i] >= 16, else TSQA_ERR_FORMAT and not one byte
 *      of the item is read.
 *   2. Header: the magic, 1 <= count <= (sizes[i] - 16) / 6, total <= count * TSQ_BLOCK_SZ, else TSQA_ERR_FORMAT; only the 16
 *      header bytes have been read by then.
 *   3. Fit: first_block[i] + blocks_i <= cap_blocks and out_offsets[i] + total_i <= out_size.  Both sums only grow, so the fitting
 *      items are a prefix of the accepted ones.  An accepted item that does not fit gets TSQA_ERR_OVERFLOW, and nothing of it is
 *      read or written.  d_out_offsets (n_items + 1), d_first_block (n_items + 1) and d_out_sizes are complete and correct for
 *      every item whatever fits (sums below 2^55), and a retry with out_offsets[n_items] bytes and first_block[n_items] blocks
 *      succeeds: the contract of the packed compress.
 *   4. Decode: the fitting items go through tsqa_decompress_batch_packed_items_async's kernels.  d_item_status[i] is the word
 *      that call leaves for the item when given the header's block count and out_cap = total_i; d_out_sizes[i] = the uncompressed
 *      size, 0 for any nonzero status; *d_status = the largest item status.  One workgroup per block: TSQA_ERR_STALL is never
 *      reported.  Nothing outside the fitting items' ranges is written.
 * cap_blocks: the blocks the call may decode (it sizes the context's frame scratch and the decode launch: pass a tight value).
 * Measure only: d_out == NULL with out_size == 0 (cap_blocks is not looked at).  The tables are filled, every accepted item reads
 * TSQA_ERR_OVERFLOW, d_out_sizes is all 0 and nothing else is written: one small read of out_offsets[n_items] and
 * first_block[n_items] tells a caller the room a decode needs.
 * TSQA_ERR_ARG before anything is enqueued, with nothing written, for: a NULL arena, table or status pointer, n_items == 0, a bad
 * align, a non-NULL d_out with out_size == 0 or cap_blocks == 0, a NULL d_out with out_size != 0.
 * The item table lives in the context's scratch and nothing is uploaded; the call returns at once and may be enqueued again on the
 * same stream before the first has run (a call with more items or blocks than any before it first waits for the device, then
 * grows the scratch).
 */
int tsqa_plan_dense(const uint64_t *totals, const uint32_t *blocks, uint32_t n_items, uint32_t align, uint64_t out_size,
                    uint32_t cap_blocks, uint64_t *out_offsets, uint64_t *first_block, uint32_t *n_fit);
int tsqa_decompress_batch_packed_dense_async(tsqa_ctx *ctx, const void *d_arena, size_t arena_size, const uint64_t *d_offsets,
                                             const uint64_t *d_sizes, uint32_t n_items, uint32_t align, uint32_t cap_blocks,
                                             void *d_out, size_t out_size, uint64_t *d_out_offsets, uint64_t *d_out_sizes,
                                             uint64_t *d_first_block, int32_t *d_item_status, int32_t *d_status, void *hip_stream);

/*
 * Packed compress whose item table is made on the device: the mirror of the dense decompress.  Item i is bytes [in_offsets[i],
 * in_offsets[i] + in_sizes[i]) of d_in, both tables in device memory (lengths a kernel has just computed, the d_out_offsets /
 * d_out_sizes that the dense decompress leaves, the tables of an arena to be repacked); input ranges may overlap.  Nothing is
 * uploaded and nothing in the tables is trusted.  Per item, on the device:
 *   1. Place: in_sizes[i] >= 1, in_sizes[i] <= in_size, in_offsets[i] <= in_size - in_sizes[i], else TSQA_ERR_ARG: no blocks, and not
 *      one byte of the item is read.  (tsqa_compress_batch_packed_async refuses the whole call for these; here they cost the item.)
 *   2. Blocks: blocks_i = ceil(in_sizes[i] / TSQ_BLOCK_SZ), 0 for a refused item; first_block[0] = 0, first_block[i + 1] =
 *      first_block[i] + blocks_i.  An accepted item fits when first_block[i] + blocks_i <= cap_blocks; the fitting items are a
 *      prefix of the accepted ones (the first unfit item ends it, whatever would fit behind it).  An unfit item gets
 *      TSQA_ERR_OVERFLOW and is not read.  d_first_block (n_items + 1) is complete whatever fits: first_block[n_items] is the
 *      cap_blocks a retry needs.  The sums stay below 2^59 and cannot wrap (in_size <= 2^48).
 *   3. Arena: every fitting item is encoded; its container is byte for byte tsqa_compress_device's for its bytes alone.  d_sizes[i]
 *      = its size, 0 for a refused or unfit item; d_offsets (n_items + 1) = tsqa_plan_packed's rule applied to d_sizes, so an item
 *      of size 0 takes no room.  A header or frame is written only if it ends at or before out_size; nothing at or past d_out +
 *      out_size is written, padding never.  A fitting item with offsets[i] + sizes[i] > out_size gets TSQA_ERR_OVERFLOW; its size and
 *      place are still correct, and a retry with offsets[n_items] bytes succeeds.
 *   4. Bound: *d_bound (one word, may be NULL) = the sum over the accepted items of round_up(tsqa_batch_bound(in_sizes[i]), align):
 *      room that always holds the arena.  Refused items add nothing: a lying size cannot inflate it.
 *   5. Status: d_item_status[i] == 0 means that the item's container is complete and exact, whatever the other items are;
 *      *d_status = the largest item status.
 * cap_blocks: the blocks the call may encode.  It sizes the descriptor scratch (24 B each) and the encode launches, 2 x CUs blocks
 * each, whose workgroups past the live blocks leave at once: a loose value costs empty launches, and -- the layout of the staged
 * encoder follows the launch's workgroup count -- may pick the lean layout for few live blocks.  Pass a tight value
 * (first_block[n_items] of a measuring call, or tsqa_plan_compress_tables).
 * Measure only: d_out == NULL with out_size == 0 (cap_blocks is not looked at).  d_item_status, d_first_block and *d_bound are made,
 * every accepted item reads TSQA_ERR_OVERFLOW, d_sizes and d_offsets are all 0, and no encoder is launched.
 * TSQA_ERR_ARG before anything is enqueued, with nothing written, for: a NULL table, input or status pointer, n_items == 0, a bad
 * align, in_size > 2^48, a non-NULL d_out with out_size < 16 or cap_blocks == 0, a NULL d_out with out_size != 0, an encoder variant
 * other than 0, 6 or 7.
 * The item table, the block descriptors and the per-launch tables live in the context's scratch; the call returns at once and may
 * be enqueued again on the same stream before the first has run (a call with more items or a larger cap_blocks than any before it
 * first waits for the device, then grows the scratch).
 *
 * tsqa_plan_compress_tables: host only.  Rules 1, 2 and 4 from host copies of the tables -> first_block[n_items + 1],
 *   item_status[n_items] (0, TSQA_ERR_ARG, or TSQA_ERR_OVERFLOW for an accepted item outside the fitting prefix), *bound, and *n_fit =
 *   the index of the first accepted item that does not fit cap_blocks, n_items when all do.  TSQA_ERR_ARG for a NULL pointer,
 *   n_items == 0, a bad align or in_size > 2^48.
 */
int tsqa_plan_compress_tables(const uint64_t *in_offsets, const uint64_t *in_sizes, uint32_t n_items, uint64_t in_size,
                              uint32_t align, uint32_t cap_blocks, uint64_t *first_block, int32_t *item_status, uint64_t *bound,
                              uint32_t *n_fit);
int tsqa_compress_batch_packed_tables_async(tsqa_ctx *ctx, const void *d_in, size_t in_size, const uint64_t *d_in_offsets,
                                            const uint64_t *d_in_sizes, uint32_t n_items, uint32_t cap_blocks, uint32_t ext,
                                            uint32_t align, void *d_out, size_t out_size, uint64_t *d_offsets, uint64_t *d_sizes,
                                            uint64_t *d_first_block, uint64_t *d_bound, int32_t *d_item_status, int32_t *d_status,
                                            void *hip_stream);

/*
 * Join: the containers of a packed batch into ONE container, at copy speed.  The batch calls leave N containers in device memory;
 * tsqa_decompress_device*, tsqa_index_create, the range and record reads, tsq_cli, tsqDecompress* and the reference's readers take
 * one.  The format permits the cheap way from the first to the second: a reader starts block k where the blocks before it end, and
 * every frame carries its own ext bit, so the join of c_0 .. c_{N-1} is
 *   "TSQ1" | u32 sum(n_blocks_i) | u64 sum(total_i) | body_0 | body_1 | ... | body_{N-1}
 *   body_i = the bytes of c_i from 16 to the end of its last frame
 * and decodes to the concatenation of the items' data.  Nothing is decoded and nothing is changed in place; an append is the join
 * of the old container and the new one, and the same container listed twice gives its data twice.
 *
 * tsqa_plan_join: host only.  frame_bytes[i] = the bytes of container i from its start to the end of its last frame.
 *   body_at[0] = 16, body_at[i + 1] = body_at[i] + frame_bytes[i] - 16; first_block = the prefix sum of blocks (both n_items + 1);
 *   *n_blocks and *total = the joined header's fields, *size = body_at[n_items].  TSQA_ERR_ARG for a NULL pointer, n_items == 0,
 *   blocks[i] == 0, frame_bytes[i] < 16 + 6 * blocks[i] or totals[i] > blocks[i] * TSQ_BLOCK_SZ; TSQA_ERR_OVERFLOW when the block sum
 *   does not fit 32 bits (the tables are still filled).
 *
 * tsqa_join_async: the arguments of the dense decompress.  Container i is [d_offsets[i], d_offsets[i] + d_sizes[i]) of d_arena, the
 * tables in device memory; nothing is uploaded, nothing in the tables or the arena is trusted, and ranges may overlap.  The call is
 * all or nothing -- a join with an item left out would silently be other data -- and still leaves a verdict per item:
 *   1. Place and header: rules 1 and 2 of the dense decompress, else TSQA_ERR_FORMAT in d_item_status[i]; the item counts as 0
 *      blocks, and only its 16 header bytes have been read.
 *   2. Blocks: d_first_block (n_items + 1) = the prefix sum of the accepted headers' counts, complete whatever fits:
 *      first_block[n_items] is the cap_blocks a retry needs.  The items that fit cap_blocks are a prefix of the accepted ones (the
 *      first unfit item ends it); an accepted item outside it gets TSQA_ERR_OVERFLOW and is not walked.
 *   3. Walk: every fitting item is walked as tsqa_decompress_device_async walks a single container, without a capacity check;
 *      a refusal is TSQA_ERR_FORMAT.  ONE lane walks one item, so an item of many short blocks costs its serial walk (262 144
 *      blocks of 4 KiB: that many dependent loads on one lane, whatever the other items are).  Bytes of an item behind its last
 *      frame are legal and are left out of the join.
 *   4. Size: *d_status = the largest item status.  When every item is accepted and fits, *d_out_size = tsqa_plan_join's size, also
 *      when that exceeds out_cap: then *d_status = TSQA_ERR_OVERFLOW, and a retry with that much room succeeds.  In every other
 *      case *d_out_size = 0.
 *   5. Emit: only while *d_status == 0: the header, the bodies at body_at, and -- d_block_sizes (device, may be NULL) -- the
 *      first_block[n_items] stream lengths in joined order, the table tsqa_decompress_device_sized* takes.  On any nonzero status
 *      not one byte of d_out and not one word of d_block_sizes is written.  Nothing at or past d_out + out_cap is ever written,
 *      nothing past first_block[n_items] words of the table, and the copy reads no arena byte outside an accepted item's frames.
 *   6. Measure only: d_out == NULL with out_cap == 0.  cap_blocks still bounds the walk; the tables, the verdicts and *d_out_size
 *      are made, and *d_status = TSQA_ERR_OVERFLOW when every item passes.
 * cap_blocks sizes the context's per-block descriptor scratch (48 B per block): pass a tight value.
 * TSQA_ERR_ARG before anything is enqueued, with nothing written, for: a NULL arena, table or status pointer (d_out and
 * d_block_sizes may be NULL), n_items == 0, cap_blocks == 0, a non-NULL d_out with out_cap < 16, a NULL d_out with out_cap != 0,
 * [d_out, d_out + out_cap) overlapping [d_arena, d_arena + arena_size).
 * The item table, the frame descriptors and the body places live in the context's scratch; the call returns at once and may be
 * enqueued again on the same stream before the first has run (a call with more items or blocks than any before it first waits
 * for the device, then grows the scratch).
 * tsqa_join: the same, then waits.  *out_size (host) = *d_out_size, *n_blocks = first_block[n_items] (saturated at 2^32 - 1): behind
 *   TSQA_OK the joined container's size and block count, behind TSQA_ERR_OVERFLOW what a retry needs.  Returns the status.
 */
int tsqa_plan_join(const uint64_t *frame_bytes, const uint32_t *blocks, const uint64_t *totals, uint32_t n_items,
                   uint64_t *body_at, uint64_t *first_block, uint32_t *n_blocks, uint64_t *total, uint64_t *size);
int tsqa_join_async(tsqa_ctx *ctx, const void *d_arena, size_t arena_size, const uint64_t *d_offsets, const uint64_t *d_sizes,
                    uint32_t n_items, uint32_t cap_blocks, void *d_out, size_t out_cap, uint64_t *d_out_size,
                    uint64_t *d_first_block, uint32_t *d_block_sizes, int32_t *d_item_status, int32_t *d_status, void *hip_stream);
int tsqa_join(tsqa_ctx *ctx, const void *d_arena, size_t arena_size, const uint64_t *d_offsets, const uint64_t *d_sizes,
              uint32_t n_items, uint32_t cap_blocks, void *d_out, size_t out_cap, size_t *out_size, uint32_t *n_blocks,
              uint64_t *d_first_block, uint32_t *d_block_sizes, int32_t *d_item_status, void *hip_stream);

/*
 * Cut: block ranges of an indexed container, each as a container of its own, at copy speed -- the way back from the join.  The
 * frames of blocks [first, first + count) are one contiguous span of the container, every frame carries its own ext bit, and a
 * reader starts block k where the blocks before it end, so
 *   "TSQ1" | u32 count | u64 totals[k] | the container's bytes [frame(first), end(first + count - 1))
 * is a valid container and decodes to exactly those blocks' data.  Nothing is decoded, so -- unlike a range read that is
 * compressed again -- the bytes are the source's own.  cut(join(items)) at the join's d_first_block gives the items back byte for
 * byte; join([cut(a, 0..k), new, cut(a, k+1..nb)]) is the edit of block k; with short blocks a block is a page.
 * The cut leaves d_offsets / d_sizes in the packed-arena shape: tsqa_join_async, tsqa_decompress_batch_packed_dense_async and the
 * other calls that take a packed batch take its output unchanged.
 *
 * tsqa_plan_cut: host only, rules 2 to 5 below from host tables.  frame_at: the n_blocks + 1 frame boundaries (tsqa_walk_frames'
 *   frame_at with the end of the last frame appended); out_start: the array tsqa_plan_ranges takes.  offsets (n_ranges + 1), sizes,
 *   totals (may be NULL) and item_status (n_ranges) are filled; *n_fit = the first accepted range that does not fit out_size,
 *   n_ranges when all do.  TSQA_ERR_ARG for a NULL pointer, n_blocks == 0, n_ranges == 0, a bad align, frame_at[0] < 16, a frame
 *   shorter than 6 bytes or a block longer than TSQ_BLOCK_SZ.
 *
 * tsqa_cut_async: idx is an index of ONE item (tsqa_index_items(idx) == 1): tsqa_index_create, tsqa_index_create_sized*, or a batch
 * index of a single item made by tsqa_index_create_batch (one made by tsqa_index_create_packed* is refused whatever it holds; tsqa_cut_items_async, below, takes every index).  d_first and d_count (n_ranges each) are tables in device memory; nothing is uploaded, nothing in them is
 * trusted, and ranges may overlap and repeat.  Per range k, on the device, all arithmetic in 64 bits:
 *   1. Gate: where the index carries a verdict (a sized index) and it is nonzero, every range gets TSQA_ERR_FORMAT, sizes, totals
 *      and offsets are all 0 and not one byte of d_out is written.
 *   2. Range: count >= 1, first < n_blocks and count <= n_blocks - first (first + count is never formed), else TSQA_ERR_ARG for
 *      that range: size 0, total 0, no room taken, nothing of it read.
 *   3. Size: d_sizes[k] = 16 + end(first + count - 1) - frame(first); d_totals[k] (may be NULL) = the uncompressed bytes of the
 *      range's blocks.
 *   4. Layout: d_offsets (n_ranges + 1) = tsqa_plan_packed's rule applied to d_sizes with align, complete and correct for every
 *      range whatever fits.  Padding is never written.
 *   5. Fit: a container is written only if it ends at or before out_size, and nothing at or past d_out + out_size is written.  An
 *      accepted range that does not fit gets TSQA_ERR_OVERFLOW, its size, total and place still correct; a retry with
 *      d_offsets[n_ranges] bytes of room succeeds.  The written ranges are a prefix of the accepted ones.
 *   6. Status: d_item_status[k] == 0 means container k is complete and exact, whatever the other ranges are; *d_status = the
 *      largest item status.
 *   7. Measure only: d_out == NULL with out_size == 0: the tables are made, every accepted range reads TSQA_ERR_OVERFLOW.
 * TSQA_ERR_ARG before anything is enqueued, with nothing written, for: a NULL index, table or status pointer (d_totals and, when
 * measuring, d_out may be NULL), n_ranges == 0, a bad align, an index of several items (tsqa_cut_items_async cuts those), a
 * NULL d_out with out_size != 0, a non-NULL d_out with out_size < 16, [d_out, d_out + out_size) overlapping the index's container,
 * n_ranges * (container bytes + 4096) >= 2^55.
 * The call must be ordered behind the index's creation, as reads are (a sized index: the same stream).  What it keeps per range
 * lives in the context's scratch; it returns at once and may be enqueued again on the same stream before the first has run (a
 * call with more ranges than any before it first waits for the device, then grows the scratch).
 * tsqa_cut: the same with host tables (offsets n_ranges + 1, sizes, totals -- may be NULL --, item_status), filled after one
 *   wait.  Returns the status.
 */
int tsqa_plan_cut(const uint64_t *frame_at, const uint64_t *out_start, uint32_t n_blocks, const uint64_t *first, const uint64_t *count,
                  uint32_t n_ranges, uint32_t align, uint64_t out_size, uint64_t *offsets, uint64_t *sizes, uint64_t *totals,
                  int32_t *item_status, uint32_t *n_fit);
int tsqa_cut_async(tsqa_ctx *ctx, const tsqa_index *idx, const uint64_t *d_first, const uint64_t *d_count, uint32_t n_ranges,
                   uint32_t align, void *d_out, size_t out_size, uint64_t *d_offsets, uint64_t *d_sizes, uint64_t *d_totals,
                   int32_t *d_item_status, int32_t *d_status, void *hip_stream);
int tsqa_cut(tsqa_ctx *ctx, const tsqa_index *idx, const uint64_t *d_first, const uint64_t *d_count, uint32_t n_ranges,
             uint32_t align, void *d_out, size_t out_size, uint64_t *offsets, uint64_t *sizes, uint64_t *totals,
             int32_t *item_status, void *hip_stream);

/*
 * Take: items, and block ranges inside items, out of ANY index, each as a container of its own, at copy speed -- the cut with the
 * item of every range named in device memory.  A batch of containers is filtered, shuffled, compacted or split into pages by a
 * table of item numbers that a kernel has just made, with nothing decoded and no host read: packed compress -> index -> choose ->
 * take -> join, dense decompress, index or gather, on one stream.  The output is a dense arena with the packed tables, as the cut's.
 *
 * idx: tsqa_index_create, tsqa_index_create_sized*, tsqa_index_create_batch, or tsqa_index_create_packed* fetched or not.
 * d_items (n_ranges, device): the item of each range; NULL: item 0 for every range, which an index of one item allows.
 * d_first, d_count (n_ranges each, device): block ranges counted from the item's own first block; both NULL: the whole item.
 * Nothing is uploaded, nothing in the tables is trusted, ranges may overlap and repeat.  Per range k, on the device, in 64 bits:
 *   1. Gate: tsqa_cut_async's rule 1.
 *   2. Item: d_items[k] < tsqa_index_items(idx), and the item owns blocks.  A refused or unfit item owns none: TSQA_ERR_ARG for
 *      the range, size 0, total 0, no room taken, nothing of it read.  An index of one item made without an item table owns all
 *      its blocks.  For an index made on the device and not fetched the live block count is read on the device
 *      (d_blocks_total[0]); descriptors from there to cap_blocks are never read.
 *   3. Range: with nb = the item's blocks, count >= 1, first < nb and count <= nb - first (first + count is never formed), else
 *      TSQA_ERR_ARG as above.  The whole-item form is first = 0, count = nb.
 *   4. Size, layout, fit, status, measure only: tsqa_cut_async's rules 3 to 7, with the frames and totals of the item's blocks.
 * The kernels are tsqa_cut_async's, which is this call through an index of one item with d_items NULL: the layout is made by
 * three launches of which none waits for another, and the tables are the ones tsqa_plan_cut_items makes, entry for entry.
 * TSQA_ERR_ARG before anything is enqueued, with nothing written, for: a NULL index, table or status pointer (d_items as above;
 * d_totals and, when measuring, d_out may be NULL), exactly one of d_first / d_count NULL, d_items NULL with an index of several
 * items, n_ranges == 0, a bad align, a NULL d_out with out_size != 0, a non-NULL d_out with out_size < 16, [d_out, d_out +
 * out_size) overlapping the index's buffer (the container, or the whole arena of a batch index), n_ranges * (buffer bytes +
 * 4096) >= 2^55.
 * Ordering and scratch: as tsqa_cut_async (behind the index's creation on the same stream or an event; the scratch per range
 * lives in the context and grows as the cut's).
 * tsqa_cut_items: the same with host tables, filled after one wait, as tsqa_cut.  Returns the status.
 * tsqa_plan_cut_items: host only, rules 2 to 4 from host tables.  frame_at (n_blocks + 1): boundaries whose differences inside an
 *   item are its frames' bytes -- for one container tsqa_plan_cut's frame_at, for a batch the running sum of the healthy items'
 *   frame bytes from 16 on --; out_start as tsqa_plan_cut; item_first_block (n_items + 1, non-decreasing, ending at or below
 *   n_blocks; NULL for one item that owns every block); items, first, count: host copies of the device tables, NULL as there.
 *   Fills what tsqa_plan_cut fills.  TSQA_ERR_ARG for what that refuses (n_blocks == 0 is allowed: every range is refused),
 *   n_items == 0, one of first / count NULL, and items or item_first_block NULL with several items.
 */
int tsqa_plan_cut_items(const uint64_t *frame_at, const uint64_t *out_start, uint32_t n_blocks,
                        const uint64_t *item_first_block, uint32_t n_items,
                        const uint32_t *items, const uint64_t *first, const uint64_t *count, uint32_t n_ranges,
                        uint32_t align, uint64_t out_size,
                        uint64_t *offsets, uint64_t *sizes, uint64_t *totals, int32_t *item_status, uint32_t *n_fit);
int tsqa_cut_items_async(tsqa_ctx *ctx, const tsqa_index *idx, const uint32_t *d_items,
                         const uint64_t *d_first, const uint64_t *d_count, uint32_t n_ranges, uint32_t align,
                         void *d_out, size_t out_size, uint64_t *d_offsets, uint64_t *d_sizes, uint64_t *d_totals,
                         int32_t *d_item_status, int32_t *d_status, void *hip_stream);
int tsqa_cut_items(tsqa_ctx *ctx, const tsqa_index *idx, const uint32_t *d_items,
                   const uint64_t *d_first, const uint64_t *d_count, uint32_t n_ranges, uint32_t align,
                   void *d_out, size_t out_size, uint64_t *offsets, uint64_t *sizes, uint64_t *totals,
                   int32_t *item_status, void *hip_stream);

/*
 * Short blocks: ONE container whose blocks are block_len bytes long instead of TSQ_BLOCK_SZ.  A job's speed follows its block
 * count -- a block is one serial chain on one workgroup -- and tsqa_compress_device leaves a mid-size buffer with few: 64 MiB are 16
 * blocks on a chip of 256 CUs.  The format allows any block length up to TSQ_BLOCK_SZ (block k starts where the blocks before it
 * end), so every decode entry point of this library reads such a container: whole, batch, range and record reads, and
 * tsqDecompress / tsqDecompress_MT.  The reference's readers append the blocks as they come and take it too (INTEGRATION.md,
 * section 4, says what was tried).  The price is ratio: a block finds no match in the bytes before it (the table is there as well).
 *
 * tsqa_plan_split: host only.  block_len: a power of two from 2^12 to 2^22.  *n_blocks = ceil(n / block_len); *bound = the room
 *   that always holds the container: 16, then per block of k bytes 3 + min(TSQ_OUTPUT_SZ, 11 + k + k/8 + k/2) (tsqa_batch_bound's
 *   term per block; with block_len = TSQ_BLOCK_SZ, tsqa_batch_bound(n)).  TSQA_ERR_ARG for n == 0, a bad block_len, a block count
 *   that does not fit 32 bits, or a NULL pointer.
 *
 * tsqa_compress_device_split_async: the container is the header (n_blocks, n), then block b = the bytes [b * block_len,
 *   min(n, (b + 1) * block_len)), encoded as tsqa_compress_device encodes a block: its look-ahead runs on into the bytes that
 *   follow it in the input and sees zeros past n.  So block_len = TSQ_BLOCK_SZ gives tsqa_compress_device's container byte for byte.
 *   d_block_sizes (device, may be NULL): n_blocks words, word b = block b's stream length (what tsqa_decompress_device_sized*
 *   takes); complete whatever fits.  A header or frame is written only if it ends at or before out_cap, and nothing at or past
 *   d_out + out_cap is written; *d_out_size = the size needed, TSQA_ERR_OVERFLOW in *d_status when it exceeds out_cap, and a retry
 *   with that much room succeeds.  TSQA_ERR_ARG, before anything is enqueued or written: tsqa_plan_split's refusals, a NULL
 *   pointer other than d_block_sizes, out_cap < 16 + 6 * n_blocks, an encoder variant other than 0, 6 or 7.  The blocks are encoded
 *   in launches of at most 2 x CUs, as a batch's are, with the block descriptors made on the device: nothing is uploaded, and the
 *   scratch does not grow with n (it grows as in the batch calls: the call first waits for the device).
 * tsqa_compress_device_split: the same, then waits; *out_size (host) = the size needed, behind TSQA_ERR_OVERFLOW too.
 */
int tsqa_plan_split(size_t n, uint32_t block_len, uint32_t *n_blocks, size_t *bound);
int tsqa_compress_device_split_async(tsqa_ctx *ctx, const void *d_in, size_t n, uint32_t block_len, void *d_out, size_t out_cap,
                                     uint64_t *d_out_size, uint32_t *d_block_sizes, int32_t *d_status, uint32_t ext, void *hip_stream);
int tsqa_compress_device_split(tsqa_ctx *ctx, const void *d_in, size_t n, uint32_t block_len, void *d_out, size_t out_cap,
                               size_t *out_size, uint32_t *d_block_sizes, uint32_t ext, void *hip_stream);

/*
 * Short blocks in a packed batch: tsqa_compress_batch_packed* and tsqa_compress_batch_packed_tables_async with every item cut every
 * block_len bytes, as tsqa_compress_device_split cuts one buffer.  A batch's speed follows its block count too: 64 items of 1 MiB
 * are 64 serial chains on 256 CUs.  The pack scan behind each encode launch is parallel over the launch's blocks (one item may own
 * all 2 x CUs of them), and every call that takes a packed batch takes the result: the batch decodes, the dense decompress,
 * tsqa_index_create_batch, join, cut, gather, and per item tsqa_decompress_device_sized* and tsqa_index_create_sized*.
 *
 * tsqa_plan_batch_split: host only.  block_len: tsqa_plan_split's rule, a power of two from 2^12 to 2^22.  Item i has
 *   ceil(in_len / block_len) blocks; first_block (n_items + 1) is their prefix sum.  *bound = the sum over the items of
 *   round_up(tsqa_plan_split(in_len, block_len)'s bound, align): room that always holds the arena.  TSQA_ERR_ARG for
 *   tsqa_compress_batch_packed_async's refusals (a NULL pointer, n_items == 0, an empty item, an input range past in_size, a bad
 *   align), a bad block_len, or block counts that do not fit 32 bits.
 *
 * tsqa_compress_batch_packed_split_async: the arguments of tsqa_compress_batch_packed_async, block_len, and d_block_sizes (device,
 *   may be NULL).  Container i, at d_out + offsets[i], is byte for byte what tsqa_compress_device_split gives for item i's bytes
 *   alone at that block_len and ext: block j's look-ahead runs on into the item's following bytes and ends at the item's last
 *   byte; it never sees the next item.  d_offsets and d_sizes follow tsqa_plan_packed's rule and are complete and correct whatever
 *   fits.  The overflow contract is the packed compress's: a header or frame is written only if it ends at or before out_size,
 *   nothing at or past d_out + out_size is written, padding never; offsets[n_items] > out_size gives TSQA_ERR_OVERFLOW in *d_status,
 *   every item that lies wholly inside out_size is exact, and a retry with offsets[n_items] bytes succeeds.  d_block_sizes holds
 *   first_block[n_items] words, word first_block[i] + j = the stream length of block j of item i, complete whatever fits: words
 *   [first_block[i], first_block[i + 1]) are the table that tsqa_decompress_device_sized* and tsqa_index_create_sized* take for item
 *   i, and laid end to end they are the table tsqa_join_async leaves for the joined container.  With block_len = TSQ_BLOCK_SZ the
 *   arena and both tables are tsqa_compress_batch_packed_async's, byte for byte.  The copy pieces per block are counted from the
 *   split bound of a block; a stream longer than that -- the encoder never makes one -- is TSQA_ERR_OVERFLOW, not a silent cut.
 *   TSQA_ERR_ARG before anything is enqueued or written: tsqa_compress_batch_packed_async's refusals and a bad block_len.  Encoder
 *   variants 0, 6 and 7.  Only the item table and first_block are uploaded: the block descriptors are made on the device.
 * tsqa_compress_batch_packed_split: the waiting form, with host offsets and sizes, as tsqa_compress_batch_packed.
 *
 * tsqa_plan_compress_tables_split, tsqa_compress_batch_packed_tables_split_async: the same extension of the device-tables form.
 *   Rules 1 to 5 of tsqa_compress_batch_packed_tables_async hold with blocks_i = ceil(in_sizes[i] / block_len); an item whose block
 *   count exceeds 2^32 - 1 is TSQA_ERR_ARG for that item; the bound's term is tsqa_plan_split's bound; d_block_sizes (device, may be
 *   NULL) is as above, cap_blocks words at most: no word is written past first_block[n_items] or cap_blocks, and the words of
 *   refused and unfit items do not exist (they have no blocks).  Measure-only and every TSQA_ERR_ARG of that call carry over; a bad
 *   block_len is one more.  Nothing is uploaded.
 */
int tsqa_plan_batch_split(const tsqa_batch_item *items, uint32_t n_items, size_t in_size, uint32_t block_len, uint32_t align,
                          uint64_t *first_block, uint64_t *bound);
int tsqa_compress_batch_packed_split_async(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items,
                                           uint32_t n_items, uint32_t ext, uint32_t align, uint32_t block_len, void *d_out,
                                           size_t out_size, uint64_t *d_offsets, uint64_t *d_sizes, uint32_t *d_block_sizes,
                                           int32_t *d_status, void *hip_stream);
int tsqa_compress_batch_packed_split(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items, uint32_t n_items,
                                     uint32_t ext, uint32_t align, uint32_t block_len, void *d_out, size_t out_size, uint64_t *offsets,
                                     uint64_t *sizes, uint32_t *d_block_sizes, void *hip_stream);
int tsqa_plan_compress_tables_split(const uint64_t *in_offsets, const uint64_t *in_sizes, uint32_t n_items, uint64_t in_size,
                                    uint32_t block_len, uint32_t align, uint32_t cap_blocks, uint64_t *first_block,
                                    int32_t *item_status, uint64_t *bound, uint32_t *n_fit);
int tsqa_compress_batch_packed_tables_split_async(tsqa_ctx *ctx, const void *d_in, size_t in_size, const uint64_t *d_in_offsets,
                                                  const uint64_t *d_in_sizes, uint32_t n_items, uint32_t cap_blocks, uint32_t ext,
                                                  uint32_t align, uint32_t block_len, void *d_out, size_t out_size,
                                                  uint64_t *d_offsets, uint64_t *d_sizes, uint64_t *d_first_block, uint64_t *d_bound,
                                                  uint32_t *d_block_sizes, int32_t *d_item_status, int32_t *d_status, void *hip_stream);

/*
 * tsqa_decompress_device_sized_async: tsqa_decompress_device_async with the frame walk made in parallel.  A frame carries no
 *   marker, so the plain walk is one lane reading frame after frame (16 384 dependent loads for 1 GiB in 64 KiB blocks); with
 *   d_block_sizes (device, n_blocks words: what the split compress left, or any table of the frames' stream lengths) every frame's
 *   place is a prefix sum.  NOTHING in the table is trusted: each frame is looked up where the table puts it -- a size outside
 *   [3, TSQ_OUTPUT_SZ] refuses the container and counts as 0, so no sum can wrap; the frame's six bytes must lie inside n before
 *   one of them is read; the frame must pass the plain walk's checks; and the length in its frame word must be the table's.  Frame
 *   0 is at 16 whatever the table says, so where every frame agrees, every place is the plain walk's.  For a true table, status,
 *   size and output are tsqa_decompress_device_async's, for every container, valid or not; a false table gives TSQA_ERR_FORMAT
 *   with *d_out_size = 0 and nothing decoded.  Nothing outside [d_out, d_out + out_cap) is ever written, and no byte at or past
 *   d_in + n is ever read.  TSQA_ERR_STALL is reported as by tsqa_decompress_device_async.
 *   The table is read as n_blocks words, the count the CALLER states, and only behind a header that states the same count: a
 *   container never decides how far the table is read.
 * tsqa_decompress_device_sized: the waiting form, as tsqa_decompress_device (it reads the header itself, and decodes again by
 *   itself after TSQA_ERR_STALL).  n_blocks = the words d_block_sizes holds: a header that states another count is refused with
 *   TSQA_ERR_FORMAT and *out_size = 0 before anything is enqueued, and n_blocks == 0 is TSQA_ERR_ARG.
 */
int tsqa_decompress_device_sized_async(tsqa_ctx *ctx, const void *d_in, size_t n, uint32_t n_blocks, const uint32_t *d_block_sizes,
                                       void *d_out, size_t out_cap, uint64_t *d_out_size, int32_t *d_status, void *hip_stream);
int tsqa_decompress_device_sized(tsqa_ctx *ctx, const void *d_in, size_t n, uint32_t n_blocks, const uint32_t *d_block_sizes, void *d_out,
                                 size_t out_cap, size_t *out_size, void *hip_stream);

/*
 * The index of a container of short blocks, made from its size table with no host wait.  tsqa_index_create reads the header to
 * the host, walks the frames on one lane and copies every descriptor back; for a split container none of that is needed.  The
 * caller knows n_total and block_len, so block b's output starts at b * block_len and the host plans every read from arithmetic
 * alone; the device places the frames from the table (three plain launches, 256 frames per workgroup, no workgroup waiting for
 * another) and proves that the container has that geometry.  So compress -> index -> read runs on one stream with no host read.
 *
 * tsqa_index_create_sized_async: n = the readable room at d_container, not necessarily the container's size (as
 *   tsqa_decompress_device_sized_async takes it).  n_blocks = tsqa_plan_split(n_total, block_len)'s count, from the caller's
 *   numbers and never from the container; d_block_sizes (device): n_blocks words, as tsqa_compress_device_split* leaves them.
 *   TSQA_ERR_ARG, with nothing enqueued and *out = NULL: a NULL pointer, one of tsqa_plan_split's refusals, n < 16 + 6 * n_blocks.
 *   Otherwise the call reads no device memory on the host and waits for no stream (it allocates the index's descriptors); it
 *   enqueues on hip_stream a zero fill of the descriptors and the walk.  tsqa_index_blocks, tsqa_index_total and tsqa_index_items
 *   answer from the caller's numbers (n_blocks, n_total, 1).
 *   The verdict, made on the device with NOTHING trusted, is TSQA_ERR_FORMAT when: the header is refused for n, or states another
 *   block count than n_blocks or another total than n_total; a table word is outside [3, TSQ_OUTPUT_SZ] (it counts as 0 in the
 *   sums, so none can wrap); a frame's six bytes do not lie inside n (checked before one of them is read); the frame fails the
 *   plain walk's checks; the length in its frame word is not the table's; or its block's size is not block_len (the last block:
 *   n_total - (n_blocks - 1) * block_len).  Otherwise it is TSQA_OK, every descriptor is the one tsqa_index_create makes for
 *   that container, and every read equals the same read through tsqa_index_create.  No byte at or past d_container + n is read.
 *   tsqa_decompress_ranges* and tsqa_decompress_item_ranges* take the index unchanged (one item).  They must be ordered behind the
 *   creation: the same stream, or an event.  On a refused index every read gives TSQA_ERR_FORMAT in *d_status and writes no
 *   destination byte: a one-thread kernel in front of the read hands the verdict on, and the decoders leave when they find it.
 * tsqa_index_create_sized: the same, then waits for hip_stream: TSQA_ERR_FORMAT and no index when the verdict refuses.
 * tsqa_index_d_status: the device word that holds the verdict (to read it: order the read behind the creation); NULL for an index
 *   made by tsqa_index_create or tsqa_index_create_batch, and for NULL.  It lives as long as the index.
 * The index holds d_container and must be destroyed before it; d_block_sizes is not needed once the walk has run.
 */
int tsqa_index_create_sized_async(tsqa_ctx *ctx, const void *d_container, size_t n, uint64_t n_total, uint32_t block_len,
                                  const uint32_t *d_block_sizes, tsqa_index **out, void *hip_stream);
int tsqa_index_create_sized(tsqa_ctx *ctx, const void *d_container, size_t n, uint64_t n_total, uint32_t block_len,
                            const uint32_t *d_block_sizes, tsqa_index **out, void *hip_stream);
const int32_t *tsqa_index_d_status(const tsqa_index *idx);

/*
 * Record reads from a batch: many short ranges out of many small containers (pages, records, tensors) that lie in one buffer in
 * HBM -- what tsqa_compress_batch makes.  One index covers the whole batch, a read names its item, and a block that several
 * ranges touch is decoded ONCE for all of them: the cost of a call follows the blocks touched, not the ranges asked for.
 *
 * tsqa_index_create_batch: synchronous, like tsqa_index_create, and at a constant number of launches, copies and waits whatever
 *   n_items is (one header gather, one frame walk with a lane per item, one frame table).  items: the items of a decompress batch
 *   (in_at, in_len locate container i in d_in; out_at, out_cap are not used).  Every container is validated as
 *   tsqa_index_create validates one; a refused item gets TSQA_ERR_FORMAT in item_status (host, may be NULL) and the healthy items
 *   are indexed.  The index is made whenever the arguments are valid (tsqa_plan_batch's checks of the input ranges: TSQA_ERR_ARG
 *   and no index otherwise); the return value is the largest item status.  tsqa_index_blocks / tsqa_index_total of such an index:
 *   the healthy items' blocks and the sum of their totals, and tsqa_decompress_ranges* on it reads the concatenation of the healthy
 *   items' data in item order.  The same tsqa_index type: tsqa_index_destroy frees it.
 */
int      tsqa_index_create_batch(tsqa_ctx *ctx, const void *d_in, size_t in_size, const tsqa_batch_item *items,
                                 uint32_t n_items, tsqa_index **out, int32_t *item_status);
uint32_t tsqa_index_items(const tsqa_index *idx);                   /* 1 for an index made by tsqa_index_create (0 for NULL) */
uint64_t tsqa_index_item_total(const tsqa_index *idx, uint32_t i);  /* item i's uncompressed size; 0 when refused */
int      tsqa_index_item_status(const tsqa_index *idx, uint32_t i); /* TSQA_OK or TSQA_ERR_FORMAT (TSQA_ERR_ARG: no such item) */
/* (An index made by tsqa_index_create_packed*, below: until tsqa_index_fetch the host has none of its tables -- tsqa_index_items
 * answers n_items, the totals 0, every item status TSQA_ERR_ARG; afterwards an item status may also be TSQA_ERR_ARG or
 * TSQA_ERR_OVERFLOW.) */

/* bytes [offset, offset + length) of item `item`'s own data -> d_out + out_at */
typedef struct tsqa_item_range { uint32_t item, pad; uint64_t offset, length, out_at; } tsqa_item_range;
/* one decode: block `block`, its items [first, first + count) of the item array (ascending lo), decoded up to `hi` */
typedef struct tsqa_block_group { uint32_t block, first, count, hi; } tsqa_block_group;

/* Host-only (no device), like tsqa_plan_ranges: out_start[0..n_blocks] as there; item i owns the blocks
 * [item_first_block[i], item_first_block[i + 1]) (n_items + 1 entries, from 0 to n_blocks; a refused item owns none).  The ranges
 * are cut into one item per block they touch, the items are sorted by (block, lo), and every touched block gets one group.
 * Sources may overlap freely (two ranges may read the same bytes); destinations may not.  Zero-length ranges give nothing.
 * TSQA_ERR_ARG, with nothing written to items and groups, for: an item number >= n_items, a range of a refused item, a range
 * past its item's total, out_at + length > out_cap, destinations that overlap, or arrays too small (*n_range_items and *n_groups
 * then hold the counts needed). */
int tsqa_plan_item_ranges(const uint64_t *out_start, uint32_t n_blocks, const uint64_t *item_first_block, uint32_t n_items,
                          const tsqa_item_range *ranges, uint32_t n_ranges, size_t out_cap,
                          tsqa_range_item *items, uint32_t cap_items, uint32_t *n_range_items,
                          tsqa_block_group *groups, uint32_t cap_groups, uint32_t *n_groups);

/* Read the ranges (a host array) into d_out: one workgroup per touched block decodes it once, up to the last byte any of its
 * ranges needs, and writes every range's bytes as the chunks that hold them appear.  Planning, the status word, stream ordering
 * and repeated calls on one stream: exactly as tsqa_decompress_ranges*.  The index may also be one made by tsqa_index_create
 * (a batch of one item).
 * Trust: as for range reads, damage beyond the last chunk a group needs may go unreported; when *d_status is nonzero the
 * destinations' contents are undefined, and nothing outside them has been written. */
int tsqa_decompress_item_ranges_async(tsqa_ctx *ctx, const tsqa_index *idx, const tsqa_item_range *ranges, uint32_t n_ranges,
                                      void *d_out, size_t out_cap, int32_t *d_status, void *hip_stream);
int tsqa_decompress_item_ranges(tsqa_ctx *ctx, const tsqa_index *idx, const tsqa_item_range *ranges, uint32_t n_ranges,
                                void *d_out, size_t out_cap, void *hip_stream);

/*
 * Gather: record reads whose ranges lie in DEVICE memory -- sampler indices, a filter's result, offsets a kernel has just
 * computed.  Nothing is uploaded, read back or waited for: the plan that the host makes for tsqa_decompress_item_ranges* is made
 * on the device, and the output is dense, each range's place a prefix sum, so no two destinations can overlap.  Any index:
 * tsqa_index_create, tsqa_index_create_batch, tsqa_index_create_sized*, tsqa_index_create_packed* (fetched or not: below).
 *
 * Range k is bytes [d_offsets[k], d_offsets[k] + d_lengths[k]) -- of the index's whole data when d_items is NULL (a batch index:
 * the concatenation, as tsqa_decompress_ranges* reads it), else of item d_items[k]'s own data.  Its bytes land at
 * d_out + d_out_offsets[k].  Nothing in the tables is trusted; per range, in this order:
 *   1. Gate: where the index carries a verdict (a sized index) and it is nonzero, every range gets TSQA_ERR_FORMAT and no
 *      descriptor is read.
 *   2. Range: the item number below tsqa_index_items, the item not refused, length <= its total and offset <= total - length
 *      (offset + length is never formed), else TSQA_ERR_ARG.  A refused range takes no room and has no pieces.
 *   3. Layout: d_out_offsets (n_ranges + 1) = tsqa_plan_packed's rule applied to the accepted ranges' lengths with align (a power
 *      of two, 1 to 4096): every place is a multiple of align and the last length is not rounded; a refused or zero-length range
 *      takes no room.  Complete whatever fits; d_out_offsets[n_ranges] is the room a retry needs.
 *   4. Fit: a range is cut into one piece per block it touches.  An accepted range fits when its bytes end at or before out_cap
 *      and its pieces, numbered on from the accepted ranges before it, at or before cap_pieces (a zero-length range asks for
 *      neither).  Both only grow: the fitting ranges are a prefix of the accepted ones, the first unfit range ends it, and every
 *      accepted range behind gets TSQA_ERR_OVERFLOW.  *d_need_pieces = the pieces of all accepted ranges.
 *   5. Decode: one workgroup per touched block, as tsqa_decompress_item_ranges_async; the launch has min(cap_pieces, blocks)
 *      workgroups, and those past the touched blocks leave at once.  The scratch, in the context, follows cap_pieces too.
 * *d_status = the largest range status, raised to TSQA_ERR_STREAM when a decoder met a malformed stream (while it is
 * TSQA_ERR_OVERFLOW it stays that).  Trust as for record reads: when *d_status is TSQA_ERR_STREAM the destinations' contents are
 * undefined.  In every case nothing is written outside the fitting ranges' destinations; padding between them is nobody's.
 * TSQA_ERR_ARG before anything is enqueued, with nothing written, for: a NULL pointer other than d_items, a bad align,
 * cap_pieces == 0, an index of another device, or n_ranges * (tsqa_index_total + 4096) >= 2^55 or n_ranges * tsqa_index_blocks
 * >= 2^55 (what lets a sum of the layout wrap).  n_ranges == 0 clears *d_status, *d_need_pieces and d_out_offsets[0].  d_items with
 * an index of one item is allowed: only item 0 exists.  Calls that share a context share its scratch: order them on one stream.
 *
 * tsqa_gather: the same, then waits for hip_stream and returns *d_status.
 *
 * tsqa_plan_gather: host only, the same rule on host tables (out_start and item_first_block as tsqa_plan_item_ranges takes them;
 *   items may be NULL): out_offsets[n_ranges + 1], range_status[n_ranges], *n_pieces = what *d_need_pieces reads, *n_groups = the
 *   blocks the fitting ranges touch.  With out_cap = UINT64_MAX and cap_pieces = UINT32_MAX it sizes a call.  Returns TSQA_OK
 *   whatever the ranges' statuses; TSQA_ERR_ARG for a NULL pointer other than items, n_items == 0, a bad align, cap_pieces == 0,
 *   tables that do not run from 0 upwards, a block longer than TSQ_BLOCK_SZ, or the size limits above.
 */
int tsqa_plan_gather(const uint64_t *out_start, uint32_t n_blocks, const uint64_t *item_first_block, uint32_t n_items,
                     const uint32_t *items, const uint64_t *offsets, const uint64_t *lengths, uint32_t n_ranges,
                     uint32_t align, uint64_t out_cap, uint32_t cap_pieces,
                     uint64_t *out_offsets, int32_t *range_status, uint64_t *n_pieces, uint32_t *n_groups);
int tsqa_gather_async(tsqa_ctx *ctx, const tsqa_index *idx, const uint32_t *d_items, const uint64_t *d_offsets,
                      const uint64_t *d_lengths, uint32_t n_ranges, uint32_t align, uint32_t cap_pieces, void *d_out, size_t out_cap,
                      uint64_t *d_out_offsets, int32_t *d_range_status, uint64_t *d_need_pieces, int32_t *d_status, void *hip_stream);
int tsqa_gather(tsqa_ctx *ctx, const tsqa_index *idx, const uint32_t *d_items, const uint64_t *d_offsets,
                const uint64_t *d_lengths, uint32_t n_ranges, uint32_t align, uint32_t cap_pieces, void *d_out, size_t out_cap,
                uint64_t *d_out_offsets, int32_t *d_range_status, uint64_t *d_need_pieces, int32_t *d_status, void *hip_stream);

/*
 * Gather into fixed-stride padded rows: the ranges of tsqa_gather_async, but range k lands in ROW k, at d_out + k * row_stride,
 * the rest of every row is filled with a pad byte, and d_row_lengths says how many bytes each row got: one [n_rows, row_stride]
 * tensor of variable-length samples with no host read, no memset and no second pass.  Row k owns
 * [k * row_stride, (k + 1) * row_stride) whatever the tables say, so a fixed stride is the one layout besides the prefix sum in
 * which destinations chosen on the device cannot overlap; the trust statement is the gather's.  Any index the gather takes, a batch
 * index made on the device and not fetched included.
 *
 * d_items NULL: offsets into the whole data, else into item d_items[k]'s.  d_offsets NULL: every offset is 0.  d_lengths NULL:
 * the row runs from its offset to the end of its item (or of the data); with d_items alone every row is a whole item.  Per row, in
 * this order:
 *   1. Gate and range: rules 1 and 2 of tsqa_gather_async (TSQA_ERR_FORMAT for every row of a refused sized index, TSQA_ERR_ARG for
 *      a bad or refused item or a range past its total).  With d_lengths NULL the length is total - offset, and offset > total is
 *      TSQA_ERR_ARG.
 *   2. Stride: an accepted length above row_stride gets TSQA_ERR_OVERFLOW for that row ALONE -- this is no prefix: the rows behind
 *      it are delivered -- and has no pieces; with TSQA_ROWS_TRUNCATE in flags the row reads its first row_stride bytes instead,
 *      and only those are cut into pieces and decoded.  d_need[1] = the largest accepted length before truncation: the stride at
 *      which no row is too long.
 *   3. Pieces: one per block a row's delivered bytes touch, numbered by an exclusive sum over the accepted rows.  The rows whose
 *      pieces end at or before cap_pieces are a prefix; every accepted row behind it gets TSQA_ERR_OVERFLOW.  d_need[0] = the
 *      sum: the cap_pieces a retry at this stride and these flags needs (a retry at another stride measures again).
 *   4. d_row_lengths[k] = the bytes delivered into row k: 0 for any nonzero status.  d_row_status[k] = the row's status.
 *   5. Padding: pad in 0..255: after the call EVERY byte of [0, n_rows * row_stride) is defined: each row's data, then pad up to
 *      the stride; a refused or unfit row is all pad.  pad == -1 writes the data bytes alone.
 * *d_status = the largest row status, raised to TSQA_ERR_STREAM by a decoder exactly as in tsqa_gather_async.  Nothing outside
 * [d_out, d_out + n_rows * row_stride) is ever written, for any alignment of d_out.  d_out == NULL measures: the lengths, the
 * statuses and both need words are made, nothing is decoded or padded.
 * TSQA_ERR_ARG before anything is enqueued for: a NULL among idx, d_row_lengths, d_row_status, d_need and d_status, row_stride == 0,
 * cap_pieces == 0, an index of another device, unknown flags, pad outside -1..255, d_out != NULL with out_cap < n_rows * row_stride,
 * or n_rows * (row_stride + 4096) >= 2^55 or n_rows * tsqa_index_blocks >= 2^55.  n_rows == 0 clears *d_status and both need words.
 * The scratch is the gather's: order the calls of one context on one stream.
 *
 * tsqa_gather_rows: the same, then waits for hip_stream and returns *d_status.
 *
 * tsqa_plan_gather_rows: host only, rules 1 (without the gate) to 4 on host tables (as tsqa_plan_gather takes them; items, offsets
 *   and lengths may each be NULL): row_lengths[n_rows], row_status[n_rows], need[2], *n_groups = the blocks the delivered rows touch.
 */
#define TSQA_ROWS_TRUNCATE 1u
int tsqa_plan_gather_rows(const uint64_t *out_start, uint32_t n_blocks, const uint64_t *item_first_block, uint32_t n_items,
                          const uint32_t *items, const uint64_t *offsets, const uint64_t *lengths, uint32_t n_rows,
                          uint64_t row_stride, uint32_t flags, uint32_t cap_pieces,
                          uint64_t *row_lengths, int32_t *row_status, uint64_t *need, uint32_t *n_groups);
int tsqa_gather_rows_async(tsqa_ctx *ctx, const tsqa_index *idx, const uint32_t *d_items, const uint64_t *d_offsets,
                           const uint64_t *d_lengths, uint32_t n_rows, uint64_t row_stride, uint32_t flags, int pad,
                           uint32_t cap_pieces, void *d_out, size_t out_cap, uint64_t *d_row_lengths, int32_t *d_row_status,
                           uint64_t *d_need, int32_t *d_status, void *hip_stream);
int tsqa_gather_rows(tsqa_ctx *ctx, const tsqa_index *idx, const uint32_t *d_items, const uint64_t *d_offsets,
                     const uint64_t *d_lengths, uint32_t n_rows, uint64_t row_stride, uint32_t flags, int pad,
                     uint32_t cap_pieces, void *d_out, size_t out_cap, uint64_t *d_row_lengths, int32_t *d_row_status,
                     uint64_t *d_need, int32_t *d_status, void *hip_stream);

/*
 * Record tables from a delimiter byte: where the records of an index's data are -- the tables that tsqa_gather_async and
 * tsqa_gather_rows_async take -- made on the device with NO decoded copy.  Every block is decoded and validated as in the
 * whole-block decode, but its bytes are compared with the delimiter instead of being stored: the one thing written per decoded
 * byte is a bit, into a map in the context's scratch of (tsqa_index_total >> 6) + tsqa_index_blocks + 1 words of 8 bytes: an eighth
 * of the data and 8 bytes per block.  A count, a scan and a placement over that map make the tables.  Any index but a batch index
 * made on the device and not yet fetched.
 *
 * The rule.  The index has n_items items.  A container index has one item.  Item i has data D_i of T_i bytes.  A refused item,
 * whose item status is nonzero, has no records.  So does an item with T_i == 0.  The delimiter is one byte value delim, 0..255.
 *   - A record STARTS at byte 0 of the item.  It also starts at p + 1 for every p with D_i[p] == delim and p + 1 < T_i.
 *   - A record ENDS in front of the next delimiter at or behind its start.  Where there is none, it ends at T_i: the last record
 *     needs no terminator.
 *   - A terminator at T_i - 1 starts no record.
 *   - Two delimiters side by side give a record of length 0, which is a record.
 *   - TSQA_RECORDS_KEEP_DELIM (flag 1): a record's length includes its terminating delimiter where it has one.
 *   - TSQA_RECORDS_FLAT (flag 2): offsets count from the start of the index's whole data, the concatenation that
 *     tsqa_decompress_ranges* and a gather with d_items == NULL read.  Without the flag they count from the item's own start, which
 *     is what a gather with d_items takes.
 *   - Records are numbered item by item in item order, and by start inside an item.  No record crosses an item.
 * Outputs:
 *   - d_item_first_record has n_items + 1 entries.  It is the exclusive sum of the items' record counts.  Its last entry is the
 *     count of all records.  It is always complete, whatever cap_records.
 *   - d_need[0] is that count, the cap_records a retry needs.
 *   - d_need[1] is the largest record length under the call's flags.  It is the row_stride at which tsqa_gather_rows_async
 *     truncates nothing.  It is taken over all records, those beyond cap_records included.
 *   - Records numbered below cap_records are written to the three tables.  Records at or past it are not.  They are a prefix.
 *     Nothing of a table is written at or beyond cap_records.
 *   - d_rec_items may be NULL.  d_rec_offsets and d_rec_lengths may both be NULL together with cap_records == 0.  That call only
 *     measures.
 * Status: *d_status is TSQA_OK when every record fits.  It is TSQA_ERR_OVERFLOW when the count of all records exceeds cap_records,
 * with the prefix written.  It is TSQA_ERR_FORMAT for a sized index whose verdict is nonzero.  Then no descriptor is read, every
 * entry of d_item_first_record is 0 and both need words are 0.  It is raised to TSQA_ERR_STREAM when a decoder met a malformed
 * stream (while it is TSQA_ERR_OVERFLOW it stays that, as in tsqa_gather_async).  Then the tables' contents are undefined and
 * nothing outside them was written.
 * Trust: nothing in the container is trusted.  Every decoded chunk is validated as in the whole-block decode.  Nothing is written
 * outside the stated extents of the caller's tables.  The tables are aligned as their element types ask -- 8 bytes for the 64-bit
 * tables and d_need (which is raised with 64-bit atomics), 4 for d_rec_items and d_status --, and at any such address: nothing
 * wider than an element is stored.
 * TSQA_ERR_ARG before anything is enqueued for: a NULL among idx, d_item_first_record, d_need and d_status; delim > 255; unknown
 * flags; cap_records > 0 with a NULL offsets or lengths table; an index of another device; an index made on the device and not yet
 * fetched (the host sizes the scratch from the total and the block count: tsqa_index_fetch first).  An index of 0 blocks clears
 * the three words and the first-record table.  Calls that share a context share its scratch: order them on one stream.
 *
 * tsqa_records: the same, then waits for hip_stream and returns *d_status.
 *
 * tsqa_plan_records: host only, the same rule on decoded bytes on the host.  data is the concatenation, item_at[n_items + 1]
 *   holds the items' starts in it, item_status may be NULL (no item is refused).  Fills rec_items (may be NULL), rec_offsets and
 *   rec_lengths below cap_records, item_first_record[n_items + 1] and need[2].  Returns TSQA_OK whatever fits; TSQA_ERR_ARG for
 *   NULL or unordered tables, n_items == 0, a bad delim or bad flags.
 */
#define TSQA_RECORDS_KEEP_DELIM 1u
#define TSQA_RECORDS_FLAT 2u
int tsqa_plan_records(const void *data, const uint64_t *item_at, const int32_t *item_status, uint32_t n_items,
                      uint32_t delim, uint32_t flags, uint64_t cap_records,
                      uint32_t *rec_items, uint64_t *rec_offsets, uint64_t *rec_lengths,
                      uint64_t *item_first_record, uint64_t *need);
int tsqa_records_async(tsqa_ctx *ctx, const tsqa_index *idx, uint32_t delim, uint32_t flags, uint64_t cap_records,
                       uint32_t *d_rec_items, uint64_t *d_rec_offsets, uint64_t *d_rec_lengths,
                       uint64_t *d_item_first_record, uint64_t *d_need, int32_t *d_status, void *hip_stream);
int tsqa_records(tsqa_ctx *ctx, const tsqa_index *idx, uint32_t delim, uint32_t flags, uint64_t cap_records,
                 uint32_t *d_rec_items, uint64_t *d_rec_offsets, uint64_t *d_rec_lengths,
                 uint64_t *d_item_first_record, uint64_t *d_need, int32_t *d_status, void *hip_stream);

/*
 * Find a byte string: where a needle of 1 .. TSQA_FIND_MAX_NEEDLE bytes occurs in an index's data, made on the device with NO
 * decoded copy.  Every block is decoded and validated as in the whole-block decode, and its bytes are compared with the needle
 * instead of being stored: the one thing written per hit is a bit, into the map that tsqa_records_async uses (an eighth of the
 * data and 8 bytes per block, cleared by every call), and 32 bytes per block keep the blocks' first and last 15 bytes, from
 * which a small launch decides the hits that lie across block seams.  The records' scan over the map makes the tables.  Any
 * index but a batch index made on the device and not yet fetched.
 *
 * The rule.  The index has n_items items.  A container index has one item.  Item i has data D_i of T_i bytes.  The needle has m
 * bytes, 1 <= m <= TSQA_FIND_MAX_NEEDLE.
 *   - A HIT is a pair (i, p) with p + m <= T_i and D_i[p .. p + m) == needle.
 *   - Overlapping hits all count: "aa" occurs twice in "aaa".
 *   - A hit never runs from one item into the next.
 *   - A refused item, whose item status is nonzero, has no hits.
 *   - Hits are numbered item by item in item order, and by p inside an item.
 *   - TSQA_FIND_FLAT (flag 2, the value of TSQA_RECORDS_FLAT): offsets count from the start of the index's whole data.  Without the
 *     flag they count from the item's own start.
 * Outputs:
 *   - d_item_first_hit has n_items + 1 entries.  It is the exclusive sum of the items' hit counts.  Its last entry is the count of
 *     all hits.  It is always complete, whatever cap_hits.
 *   - d_need[0] is that count, the cap_hits a retry needs.  d_need is ONE word.
 *   - Hits numbered below cap_hits are written to d_hit_offsets (the hit's first byte) and d_hit_items (may be NULL).  They are a
 *     prefix.  Nothing of a table is written at or beyond cap_hits.
 *   - d_hit_offsets may be NULL together with cap_hits == 0.  That call only measures.
 * Status: *d_status is TSQA_OK when every hit fits.  It is TSQA_ERR_OVERFLOW when the count of all hits exceeds cap_hits, with the
 * prefix written.  It is TSQA_ERR_FORMAT for a sized index whose verdict is nonzero.  Then no descriptor is read, every entry of
 * d_item_first_hit is 0 and the need word is 0.  It is raised to TSQA_ERR_STREAM when a decoder met a malformed stream (while it
 * is TSQA_ERR_OVERFLOW it stays that, as in tsqa_records_async).  Then the tables' contents are undefined and nothing outside
 * them was written.
 * The needle is read on the host during the call and travels as kernel arguments: there is no upload and no wait, and the
 * caller's buffer may be reused as soon as the call returns.
 * Trust and alignment: as tsqa_records_async.
 * TSQA_ERR_ARG before anything is enqueued for: a NULL among idx, needle, d_item_first_hit, d_need and d_status; needle_len == 0 or
 * needle_len > TSQA_FIND_MAX_NEEDLE; unknown flags; cap_hits > 0 with a NULL offsets table; an index of another device; an index made
 * on the device and not yet fetched.  An index of 0 blocks clears the status, the need word and the first-hit table.  Calls that
 * share a context share its scratch -- a records call and a find call share the map --: order them on one stream.
 *
 * tsqa_find: the same, then waits for hip_stream and returns *d_status.
 *
 * tsqa_plan_find: host only, the same rule on decoded bytes on the host, with tsqa_plan_records' shape: data is the concatenation,
 *   item_at[n_items + 1] holds the items' starts in it, item_status may be NULL.  Fills hit_items (may be NULL) and hit_offsets
 *   below cap_hits, item_first_hit[n_items + 1] and need[1].  Returns TSQA_OK whatever fits; TSQA_ERR_ARG for NULL or unordered
 *   tables, n_items == 0, a bad needle length or bad flags.
 */
#define TSQA_FIND_FLAT 2u
#define TSQA_FIND_MAX_NEEDLE 16u
int tsqa_plan_find(const void *data, const uint64_t *item_at, const int32_t *item_status, uint32_t n_items,
                   const void *needle, uint32_t needle_len, uint32_t flags, uint64_t cap_hits,
                   uint32_t *hit_items, uint64_t *hit_offsets, uint64_t *item_first_hit, uint64_t *need);
int tsqa_find_async(tsqa_ctx *ctx, const tsqa_index *idx, const void *needle, uint32_t needle_len, uint32_t flags,
                    uint64_t cap_hits, uint32_t *d_hit_items, uint64_t *d_hit_offsets,
                    uint64_t *d_item_first_hit, uint64_t *d_need, int32_t *d_status, void *hip_stream);
int tsqa_find(tsqa_ctx *ctx, const tsqa_index *idx, const void *needle, uint32_t needle_len, uint32_t flags,
              uint64_t cap_hits, uint32_t *d_hit_items, uint64_t *d_hit_offsets,
              uint64_t *d_item_first_hit, uint64_t *d_need, int32_t *d_status, void *hip_stream);

/*
 * CRC-32 of every item: zlib's crc32 (polynomial 0xEDB88320, init and final xor 0xFFFFFFFF -- the value zlib, gzip, zip and png give)
 * of the data behind an index, made on the device with NO decoded copy.  Every block is decoded and validated as in the whole-block
 * decode, and its bytes are checksummed instead of being stored: the one thing written per block is a word of scratch (4 bytes
 * per block, cleared by every call).  The CRC is linear, so the blocks' words combine into the items' whatever block_len, ext or
 * route (join, cut, take, a transcode) made the container: equal data gives equal CRCs.  Any index but a batch index made on the
 * device and not yet fetched.
 *
 * The rule.  The index has n_items items.  A container index has one item.  Item i has data D_i of T_i bytes.
 *   - d_item_crc[i] is crc32(D_i).  It is 0 for an item of 0 bytes.
 *   - d_item_status[i] is 0 for a healthy item; the index's own item status for an item the index refused, whose CRC is 0; and
 *     TSQA_ERR_STREAM for an item one of whose blocks holds a malformed stream, whose CRC is 0.
 *   - A malformed stream costs that item alone: every other item is delivered exactly (the decoders of an item's blocks share the
 *     item's status word, as in tsqa_decompress_batch_items_async, and leave early on it).
 *   - d_block_crc[b] (may be NULL) is crc32 of block b's own data: tsqa_crc32_combine folds an item's blocks into the item's CRC on
 *     the host.  It is undefined for the blocks of an item whose status is nonzero.
 *   - d_all_crc (may be NULL) is the CRC-32 of the index's whole data, the concatenation that tsqa_decompress_ranges* reads.  Refused
 *     items contribute no bytes to it, as they contribute none to tsqa_index_total.  It is 0 when any item got TSQA_ERR_STREAM in
 *     this call.
 * Status: *d_status is TSQA_OK; TSQA_ERR_FORMAT for a sized index whose verdict is nonzero -- then no descriptor is read, every CRC
 * is 0 and every item status is TSQA_ERR_FORMAT --; TSQA_ERR_STREAM when any item was raised to it.  An index of 0 blocks leaves
 * every CRC 0 and the items' statuses the index's own.
 * flags must be 0.
 * Trust and alignment: as tsqa_records_async -- nothing in the container is trusted, nothing is written outside the stated
 * extents (n_items entries of d_item_crc and d_item_status, n_blocks of d_block_crc, one of d_all_crc and d_status), the tables
 * are aligned as their elements (4 bytes) and nothing wider than an element is stored.
 * TSQA_ERR_ARG before anything is enqueued for: a NULL among idx, d_item_crc, d_item_status and d_status; nonzero flags; an index of
 * another device; an index made on the device and not yet fetched.  Calls that share a context share its scratch: order them on
 * one stream.
 *
 * tsqa_crc32: the same, then waits for hip_stream and returns *d_status.
 *
 * tsqa_plan_crc32: host only, the same rule on decoded bytes on the host, with tsqa_plan_records' shape: data is the concatenation,
 *   item_at[n_items + 1] holds the items' starts in it, item_status may be NULL.  Fills item_crc[n_items] (0 for an empty or a
 *   refused item) and *all_crc (may be NULL; the bytes of refused items are left out).  TSQA_ERR_ARG for NULL or unordered tables or
 *   n_items == 0.
 * tsqa_crc32_host: zlib's crc32(crc, buf, n) on the host (crc 0 starts a new checksum).
 * tsqa_crc32_combine: zlib's crc32_combine -- crc32(A | B) from crc32(A), crc32(B) and B's length in bytes; the length is 64-bit
 *   (8 * len_b passes 2^32 at 512 MiB).  Both are written here: libz is neither linked nor copied.
 */
int tsqa_plan_crc32(const void *data, const uint64_t *item_at, const int32_t *item_status, uint32_t n_items, uint32_t *item_crc,
                    uint32_t *all_crc);
uint32_t tsqa_crc32_host(uint32_t crc, const void *buf, size_t n);
uint32_t tsqa_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
int tsqa_crc32_async(tsqa_ctx *ctx, const tsqa_index *idx, uint32_t flags, uint32_t *d_item_crc, int32_t *d_item_status,
                     uint32_t *d_block_crc, uint32_t *d_all_crc, int32_t *d_status, void *hip_stream);
int tsqa_crc32(tsqa_ctx *ctx, const tsqa_index *idx, uint32_t flags, uint32_t *d_item_crc, int32_t *d_item_status,
               uint32_t *d_block_crc, uint32_t *d_all_crc, int32_t *d_status, void *hip_stream);

/*
 * The index of a packed batch from its tables in DEVICE memory, with no host wait: the last step of packed compress -> index ->
 * choose -> gather that was not stream-ordered.  tsqa_index_create_batch wants the items' places on the host, reads the headers
 * back, waits, walks, copies every descriptor back, waits again and closes the gaps of refused items on the host.  Here the arena
 * and its tables are taken as tsqa_compress_batch_packed*_async and the ..._tables* forms leave them, everything is made on the
 * device, and tsqa_gather_async takes the result at once, in both addressing modes.
 *
 * tsqa_index_create_packed_async: container i is [d_offsets[i], d_offsets[i] + d_sizes[i]) of d_arena (n_items entries each, device
 * memory).  The call reads no device memory on the host and waits for no stream; it allocates the index's own device memory
 * (cap_blocks descriptors of 32 B, 20 B per item) and enqueues its launches on hip_stream.  cap_blocks: the blocks the index may
 * hold; it sizes the descriptors, the context's scratch and the launches of this call and of every gather through the index: pass
 * a tight value (d_first_block[n_items] of the compress, or a bound the caller knows).  Nothing in the tables or the arena is
 * trusted.  d_block_sizes == NULL is the plain form (block_len 0, d_table_first NULL, table_words 0); else the sized form.
 * Plain form, per item, in this order:
 *   1. Measure: rules 1 and 2 of the dense decompress (the place inside the arena, the header), else TSQA_ERR_FORMAT: no blocks,
 *      no bytes, and only the 16 header bytes of a well-placed item have been read.
 *   2. Fit: the accepted headers' block counts are summed; an item fits when the blocks of the accepted items before it and its
 *      own are at most cap_blocks.  The fitting items are a prefix of the accepted ones (the first unfit item ends it); an accepted
 *      item outside it gets TSQA_ERR_OVERFLOW and is not walked.  d_blocks_total[2] = the blocks of all accepted items: the
 *      cap_blocks a retry needs.  Every sum a verdict rests on is a sum of items that fit, so none can wrap.
 *   3. Walk: every fitting item is walked as tsqa_index_create_batch walks it, ONE lane per item (an item of many short blocks
 *      costs its serial walk), into provisional descriptors in the context's scratch; a refusal is TSQA_ERR_FORMAT.
 *   4. Close up: the healthy items' blocks and totals are summed again -- a refused or unfit item owns no blocks -- and their
 *      descriptors are put behind each other in the index, out_at in the concatenation of the healthy items' data.  Descriptors
 *      from the live count to cap_blocks are empty and start at the total.
 *   5. d_item_status[i] (device, may be NULL; the index keeps its own copy) = the item's verdict; *d_status = the largest.
 *   For every item the status, the first block and the descriptors are what tsqa_index_create_batch makes for the same containers,
 *   entry for entry; TSQA_ERR_OVERFLOW is the one status that call does not have.
 * Sized form: step 3 is made from a table of stream lengths, one lane per BLOCK of the whole batch and no workgroup waiting for
 *   another, as tsqa_index_create_sized_async walks one container.  Item i's words are d_block_sizes[d_table_first[i] ..
 *   d_table_first[i + 1]) (d_table_first: n_items + 1 entries, device; d_first_block of tsqa_compress_batch_packed_tables_split_async,
 *   or tsqa_plan_batch_split's first_block uploaded).  Between steps 1 and 2, per accepted item: d_table_first[i] <=
 *   d_table_first[i + 1] <= table_words, else TSQA_ERR_ARG; the header must state as many blocks as the item has words, and a total
 *   that this many blocks of block_len hold with the last one not empty, else TSQA_ERR_FORMAT; such an item has no blocks.  Then
 *   per block: a word outside [3, TSQ_OUTPUT_SZ] counts as 0 in the sums and refuses its item; the frame's place is 16 plus the
 *   room (3 + length) of the item's words before it; the frame's six bytes must lie inside the item before one is read; the frame
 *   must pass the plain walk's checks; the length in its frame word must be the table's; and its block is block_len bytes long,
 *   the item's last what the header's total leaves.  A failing block refuses its item alone (TSQA_ERR_FORMAT); the others are
 *   delivered.  No word at or past table_words and no byte at or past d_arena + arena_size is read.  For a true table the result
 *   is the plain form's, entry for entry.
 * TSQA_ERR_ARG before anything is enqueued, with *out = NULL: a NULL arena, table, out or d_status pointer; n_items == 0;
 *   cap_blocks == 0; a plain form with block_len, d_table_first or table_words set; a sized form with a NULL d_table_first or a
 *   block_len that tsqa_plan_split refuses.
 * The provisional descriptors and the item table live in the context's scratch: calls that share a context are ordered on one
 * stream (a call with more items or blocks than any before it first waits for the device, then grows the scratch).
 *
 * Using the index before tsqa_index_fetch: tsqa_gather_async takes it unchanged, ordered behind the creation (the same stream, or
 *   an event).  It launches with cap_blocks as the block count and reads the total on the device; the host's size check of that
 *   call uses the bound cap_blocks * (block_len ? block_len : TSQ_BLOCK_SZ) in place of tsqa_index_total.  Ranges of refused and
 *   unfit items are TSQA_ERR_ARG.  On the host, tsqa_index_items answers n_items; tsqa_index_blocks, tsqa_index_total and
 *   tsqa_index_item_total answer 0 and tsqa_index_item_status TSQA_ERR_ARG: the host does not know yet.  The reads the host plans
 *   (tsqa_decompress_ranges*, tsqa_decompress_item_ranges*) return TSQA_ERR_ARG with a message that names tsqa_index_fetch, and
 *   tsqa_cut* refuses it as it refuses a batch index -- fetched or not, and an index of one item too.  tsqa_cut_items_async takes
 *   it, fetched or not: items and their block ranges out of the batch, the live block count read on the device.
 * tsqa_index_fetch: copies the tables and the live descriptors to the host and waits for hip_stream (behind the creation).  From
 *   then on the index is a tsqa_index_create_batch index in every respect (tsqa_index_item_status may also read TSQA_ERR_ARG or
 *   TSQA_ERR_OVERFLOW).  TSQA_OK at once for an index whose tables the host already has.
 * tsqa_index_device_tables: the device tables of an index made by these calls, valid as long as it lives (any pointer may be
 *   NULL): d_item_first (n_items + 1: item i owns the blocks [d_item_first[i], d_item_first[i + 1])), d_item_status (n_items),
 *   d_blocks_total (three words: the live blocks, the total, the blocks of all accepted items).  TSQA_ERR_ARG and NULLs for any
 *   other index.
 * tsqa_index_create_packed: the async call, then tsqa_index_fetch; item_status (host, may be NULL) is filled.  As
 *   tsqa_index_create_batch, the index is made whenever the arguments are valid, and the return value is the largest item status.
 * tsqa_plan_index_packed: host only, steps 2 and 4 from host tables.  head_status[i]: what steps 1 (and, sized, the table check)
 *   say of item i, blocks[i] and totals[i] its header's fields (looked at where head_status[i] == 0), walk_status[i] what the walk
 *   says of it (looked at where it fits).  -> item_first (n_items + 1), item_at (n_items: each item's start in the concatenation),
 *   item_status, blocks_total (three words, as above), *status.  TSQA_ERR_ARG for a NULL pointer, n_items == 0, cap_blocks == 0, or
 *   an accepted item with no blocks or more than blocks * TSQ_BLOCK_SZ bytes.
 */
int tsqa_plan_index_packed(const uint32_t *blocks, const uint64_t *totals, const int32_t *head_status, const int32_t *walk_status,
                           uint32_t n_items, uint32_t cap_blocks, uint64_t *item_first, uint64_t *item_at, int32_t *item_status,
                           uint64_t *blocks_total, int32_t *status);
int tsqa_index_create_packed_async(tsqa_ctx *ctx, const void *d_arena, size_t arena_size, const uint64_t *d_offsets,
                                   const uint64_t *d_sizes, uint32_t n_items, uint32_t cap_blocks, uint32_t block_len,
                                   const uint64_t *d_table_first, const uint32_t *d_block_sizes, uint64_t table_words, tsqa_index **out,
                                   int32_t *d_item_status, int32_t *d_status, void *hip_stream);
int tsqa_index_create_packed(tsqa_ctx *ctx, const void *d_arena, size_t arena_size, const uint64_t *d_offsets, const uint64_t *d_sizes,
                             uint32_t n_items, uint32_t cap_blocks, uint32_t block_len, const uint64_t *d_table_first,
                             const uint32_t *d_block_sizes, uint64_t table_words, tsqa_index **out, int32_t *item_status,
                             void *hip_stream);
int tsqa_index_fetch(tsqa_ctx *ctx, tsqa_index *idx, void *hip_stream);
int tsqa_index_device_tables(const tsqa_index *idx, const uint64_t **d_item_first, const int32_t **d_item_status,
                             const uint64_t **d_blocks_total);

/* =====================================================================================
 * (1) The reference API (turbosqueeze.h:441-674), C-callable subset
 * ================================================================================== */

struct TSQCompressionContext {      /* turbosqueeze.h:57-63; tests memset refhash (test/test.cpp:42) */
    uint16_t *refhash;
};
struct TSQCompressionContext_MT;    /* opaque here; first field is uint32_t num_cores (turbosqueeze.h:343) */
struct TSQDecompressionContext_MT;

/* turbosqueeze.h:625,634,643 -- the 256 KiB CPU-visible table is kept for source
 * compatibility; the device keeps its own tables in HBM. */
struct TSQCompressionContext *tsqAllocateContext(void);
void tsqDeallocateContext(struct TSQCompressionContext *ctx);
void tsqInit(struct TSQCompressionContext *ctx);

/* turbosqueeze.h:657 -- one block, synchronous.  inputSize <= TSQ_BLOCK_SZ; outputBlock must
 * hold TSQ_OUTPUT_SZ bytes.  As in the reference (tsq_encode.cpp:74,108,126,162; its scheduler hands workers pointers
 * into the caller's contiguous buffer, tsq_threads.cpp:109) the encoder looks up to 128 bytes past
 * inputBlock[inputSize-1]: what is readable there is used (so a loop over the blocks of one buffer gives the
 * reference's bytes), what is not mapped is seen as zeros instead of faulting.  The look-ahead is taken with
 * process_vm_readv(2) on the calling process; where a sandbox refuses that call (EPERM / ENOSYS) every block sees zeros behind
 * it -- the library says so once on stderr -- and TSQ_AMD_ENCODE_NO_LOOKAHEAD=1 asks for that behaviour explicitly.  Callers that
 * must not depend on either use tsqa_encode_blocks_async, which takes the look-ahead bytes as part of its input layout. */
void tsqEncode(struct TSQCompressionContext *ctx, uint8_t *inputBlock, uint8_t *outputBlock,
               uint32_t *outputSize, uint32_t inputSize, uint32_t withExtensions);
/* turbosqueeze.h:670 -- *outputSize = 0 on an oversize header or a malformed stream. */
void tsqDecode(uint8_t *inputBlock, uint8_t *outputBlock, uint32_t *outputSize,
               uint32_t inputSize, uint32_t withExtensions);

/* turbosqueeze.h:458,470 -- FILE* to FILE*; level is ignored as in the reference. */
void tsqCompress(FILE *in, FILE *out, bool useextensions, uint32_t level);
void tsqDecompress(FILE *in, FILE *out);

/* turbosqueeze.h:480,489,554,563 */
struct TSQCompressionContext_MT   *tsqAllocateContextCompression_MT(bool verbose);
void                               tsqDeallocateContextCompression_MT(struct TSQCompressionContext_MT *ctx);
struct TSQDecompressionContext_MT *tsqAllocateContextDecompression_MT(bool verbose);
void                               tsqDeallocateContextDecompression_MT(struct TSQDecompressionContext_MT *ctx);

/* turbosqueeze.h:508,580 -- infile: `in` is a path; outfile: `*out` is a path; memory output is
 * malloc()ed by the library and free()d by the caller. */
bool tsqCompress_MT(struct TSQCompressionContext_MT *ctx, uint8_t *in, size_t szin, bool infile,
                    uint8_t **out, size_t *szout, bool outfile, bool useextensions, uint32_t level);
bool tsqDecompress_MT(struct TSQDecompressionContext_MT *ctx, uint8_t *in, size_t szin, bool infile,
                      uint8_t **out, size_t *szout, bool outfile);

/* C twins of tsqCompressAsync_MT / tsqDecompressAsync_MT (turbosqueeze.h:543-544,615-616):
 * callbacks are plain function pointers + a user pointer; either may be NULL.  Return the
 * job id (>= 1) or 0 after calling done(0,false,user). */
typedef void (*tsqa_done_fn)(uint32_t jobid, bool ok, void *user);
typedef void (*tsqa_progress_fn)(uint32_t jobid, double fraction, void *user);
uint32_t tsqa_compress_async_cb(struct TSQCompressionContext_MT *ctx, uint8_t *in, size_t szin, bool infile,
                                uint8_t **out, size_t *szout, bool outfile, bool useextensions, uint32_t level,
                                tsqa_done_fn done, tsqa_progress_fn progress, void *user);
uint32_t tsqa_decompress_async_cb(struct TSQDecompressionContext_MT *ctx, uint8_t *in, size_t szin, bool infile,
                                  uint8_t **out, size_t *szout, bool outfile,
                                  tsqa_done_fn done, tsqa_progress_fn progress, void *user);

/* tsqEncode takes the reference encoder's look-ahead (the ~67 bytes it reads behind inputBlock[inputSize-1],
 * tsq_encode.cpp:74,108,126,162) with process_vm_readv, which stops at an unmapped page instead of faulting.  Where a seccomp
 * profile or sandbox refuses that call the look-ahead is seen as zeros and a loop over the blocks of ONE buffer no longer gives the
 * container's streams at block edges (every stream stays valid).  One line on stderr says so the first time; this call lets a
 * caller detect it: 0 = not yet known (no tsqEncode call so far), 1 = look-ahead read from the caller's memory,
 * 2 = refused by the system (zeros), 3 = switched off with TSQ_AMD_ENCODE_NO_LOOKAHEAD. */
int tsqa_encode_lookahead_state(void);

#ifdef __cplusplus
}
#endif
#endif /* TURBOSQUEEZE_AMD_H */
