// tsq_runtime.hip -- device context, kernel launches and the tsqa_* device-resident C ABI.
//
// One tsqa_ctx per (process, device).  All work of a call is enqueued on ONE HIP stream in
// this order (compress):  encode kernel (one workgroup per 4 MiB block)  ->  pack_scan (frame
// offsets, header, frame bytes)  ->  pack_copy (streams into the container);
// (decompress):  frame_walk  ->  decode kernel (one workgroup per block).
// There is no host computation on the data path and no CPU fallback.
#include "tsq_internal.h"

#include "tsq_batch.cuh"
#include "tsq_common.cuh"
#include "tsq_container.cuh"
#include "tsq_format.h"
#include "tsq_serial.cuh"
#include "tsq_split.cuh"
#include "tsq_index.cuh"
#include "tsq_index_packed.cuh"
#include "tsq_join.cuh"
#include "tsq_cut.cuh"
#include "tsq_launch.cuh"
#include "tsq_gather.cuh"
#include "tsq_gather_sort.h"
#include "tsq_rows.cuh"
#include "tsq_records.cuh"
#include "tsq_find.cuh"
#include "tsq_crc.cuh"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

using namespace tsq;

#define TSQ_HIP(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (ctx)->set_error("%s failed: %s", #call, hipGetErrorString(e_));                     \
            return TSQA_ERR_HIP;                                                                 \
        }                                                                                        \
    } while (0)

void tsqa_ctx::set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, sizeof(err), fmt, ap);
    va_end(ap);
}

static hipStream_t stream_of(const tsqa_ctx* c, void* hip_stream) { return hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream; }

extern "C" size_t tsqa_block_count(size_t n) { return (n + kBlockSize - 1) / kBlockSize; }

extern "C" size_t tsqa_container_bound(size_t n) { return 16 + tsqa_block_count(n) * (size_t)(3 + kSlotSize); }

// What this library was compiled as (csrc/tsq_experiment.h): the product reports no timing-only switch and no instrumentation.
#define TSQ_STR2(x) #x
#define TSQ_STR(x) TSQ_STR2(x)
#if !defined(TSQ_LM) || !defined(TSQ_LF) || !defined(TSQ_RECORDS)
#error "tsqa_build_info stringifies TSQ_LM, TSQ_LF and TSQ_RECORDS: tsq_enc_stage.cuh (through tsq_launch.cuh) goes above it"
#endif
extern "C" const char* tsqa_build_info(void)
{
    return "arch=gfx950 timing_only=" TSQ_STR(TSQ_TIMING_ONLY_BUILD) " instrumented=" TSQ_STR(TSQ_INSTRUMENTED_BUILD)
#ifdef TSQ_AB_VARIANTS
           " ab_variants=1"
#else
           " ab_variants=0"
#endif
           " lm=" TSQ_STR(TSQ_LM) " lf=" TSQ_STR(TSQ_LF) " records=" TSQ_STR(TSQ_RECORDS) " [switches:"
#ifdef TSQ_X_NOHAZ
           " TSQ_X_NOHAZ"
#endif
#ifdef TSQ_X_NOCOMMITWAIT
           " TSQ_X_NOCOMMITWAIT"
#endif
#ifdef TSQ_X_NOPATCH
           " TSQ_X_NOPATCH"
#endif
#ifdef TSQ_X_FAKE_TABLE
           " TSQ_X_FAKE_TABLE"
#endif
#ifdef TSQ_X_FAKE_CAND
           " TSQ_X_FAKE_CAND"
#endif
#ifdef TSQ_X_FREE_QUERY
           " TSQ_X_FREE_QUERY"
#endif
#ifdef TSQ_X_DELAY_STAGE
           " TSQ_X_DELAY_STAGE"
#endif
#ifdef TSQ_STATS
           " TSQ_STATS"
#endif
#ifdef TSQ_SPINS
           " TSQ_SPINS"
#endif
#ifdef TSQ_TRACEONLY
           " TSQ_TRACEONLY"
#endif
#ifdef TSQ_JITTER
           " TSQ_JITTER"
#endif
#if !TSQ_TIMING_ONLY_BUILD && !TSQ_INSTRUMENTED_BUILD
           " none"
#endif
           "]";
}

extern "C" int tsqa_create(int device, tsqa_ctx** out)
{
    if (!out) return TSQA_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return TSQA_ERR_NO_DEVICE;
    if (device < 0) { if (hipGetDevice(&device) != hipSuccess) return TSQA_ERR_NO_DEVICE; }
    if (device >= count) return TSQA_ERR_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return TSQA_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "turbosqueeze_amd: device %d is %s; this library carries gfx950 code only\n", device, prop.gcnArchName);
        return TSQA_ERR_NO_DEVICE;
    }
    tsqa_ctx* c = new (std::nothrow) tsqa_ctx();
    if (!c) return TSQA_ERR_ARG;
    c->device = device;
    c->n_cus = prop.multiProcessorCount;
    // (tests: the reference-named API makes its contexts itself; the wait limit of its multi-workgroup decodes comes from here)
    if (const char* e = getenv("TSQ_AMD_DECODE_WAIT_LIMIT")) { const long v = atol(e); if (v > 0) c->decode_wait_limit = (uint32_t)v; }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return TSQA_ERR_HIP;
    }
    if (!c->d_size.grow(c, 1) || !c->d_status.grow(c, 1)) {
        tsqa_destroy(c);
        return TSQA_ERR_HIP;
    }
    *out = c;
    return TSQA_OK;
}

extern "C" void tsqa_destroy(tsqa_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
    for (hipEvent_t e : c->prof_pool) if (e) (void)hipEventDestroy(e);
    if (c->host_frames_copied) (void)hipEventDestroy(c->host_frames_copied);
    c->range_up.destroy(); c->batch_up.destroy();
    delete c;                                            // (the scratch and pinned buffers free themselves)
}

extern "C" const char* tsqa_last_error(const tsqa_ctx* c) { return c ? c->err : "null context"; }
extern "C" int tsqa_device_id(const tsqa_ctx* c) { return c ? c->device : -1; }
extern "C" void tsqa_set_kernel_variant(tsqa_ctx* c, int ev, int dv) { if (c) { c->enc_variant = ev; c->dec_variant = dv; } }
extern "C" void tsqa_set_decode_wait_limit(tsqa_ctx* c, uint32_t polls) { if (c) c->decode_wait_limit = polls ? polls : 1u; }

// Scratch in HBM, grown on demand and kept: slots (TSQ_OUTPUT_SZ per block, the reference's
// per-block output buffer, tsq_context.cpp:89-143), per-block sizes, frame offsets, frame
// descriptors with the batch item that owns each, and one 256 KiB position table per block for the encoders (want_tables).
// Every reserve* says which buffers its call needs and how many elements of each, waits -- once, only where one of them must grow,
// and before the first is freed -- for whatever may still be using them, and grows those that must (tsqa_scratch::grow).
// Here the wait is for the context's stream and for `s`, the stream the call was given (a call enqueued there before this one may
// still be using what is freed), or (all_streams: the batch entry points) for the whole device.
int tsqa_ctx::reserve(size_t n_blocks, bool want_tables, bool want_slots, bool all_streams, hipStream_t s)
{
    (void)hipSetDevice(device);
    const size_t nb = n_blocks, n_at = nb ? nb + 1 : 0;
    // (callers that bring their own slots -- the sharded block API -- never pay for these)
    const size_t n_slots = want_slots && nb ? nb * (size_t)kSlotSize + 256 : 0, n_tables = want_tables ? nb * (size_t)kHashEntries : 0;
    const bool descriptors = sizes.needs(nb) || frame_at.needs(n_at) || frames.needs(nb) || block_owner.needs(nb);
    if (!descriptors && !slots.needs(n_slots) && !tables.needs(n_tables)) return TSQA_OK;
    if (all_streams) (void)hipDeviceSynchronize(); else wait_for(s);
    if (descriptors) forget_sharded();                   // (the descriptors of a sharded decode go with `frames`)
    return sizes.grow(this, nb) && frame_at.grow(this, n_at) && frames.grow(this, nb) && block_owner.grow(this, nb) &&
           slots.grow(this, n_slots) && tables.grow(this, n_tables) ? TSQA_OK : TSQA_ERR_HIP;
}

// Scratch of the two-workgroup decoder (tsq_dec_duo.cuh): four chunk records and two counters per block.
int tsqa_ctx::reserve_duo(size_t n_blocks, hipStream_t s)
{
    (void)hipSetDevice(device);
    const size_t n_ring = n_blocks * (size_t)DuoCfg::SLOTS * DuoCfg::REC_WORDS, n_flags = n_blocks * (size_t)DuoCfg::FLAG_STRIDE;
    if (!duo_ring.needs(n_ring) && !duo_flags.needs(n_flags)) return TSQA_OK;
    wait_for(s);                                         // (a multi-workgroup decode enqueued on `s` may still be using the ring)
    return duo_ring.grow(this, n_ring) && duo_flags.grow(this, n_flags) ? TSQA_OK : TSQA_ERR_HIP;
}

// What a buffer that grows by doubling from `from` holds once it takes n elements (nothing asked: nothing held).
static size_t doubled(size_t from, size_t n)
{
    if (n == 0) return 0;
    while (from < n) from *= 2;
    return from;
}

// Frame descriptors built on the host (sharded fetch + decode): pinned, so that their copy to the device is a DMA ordered on the
// caller's stream; the previous call's copy is waited for before they are overwritten.
int tsqa_ctx::reserve_host_frames(size_t n)
{
    (void)hipSetDevice(device);
    if (host_frames_pending) { (void)hipEventSynchronize(host_frames_copied); host_frames_pending = false; }
    if (!host_frames_copied) TSQ_HIP(this, hipEventCreateWithFlags(&host_frames_copied, hipEventDisableTiming));
    if (host_frames.needs(n)) TSQ_HIP(this, host_frames.grow(doubled(64, n)));
    host_frame_src.resize(host_frames.cap);
    return TSQA_OK;
}

int tsqa_uploads::acquire(tsqa_ctx* c, size_t bytes, Slot* slot)
{
    (void)hipSetDevice(c->device);
    const int k = next_;
    next_ ^= 1;
    if (pending_[k]) { (void)hipEventSynchronize(done_[k]); pending_[k] = false; }
    if (!done_[k]) TSQ_HIP(c, hipEventCreateWithFlags(&done_[k], hipEventDisableTiming));
    if (dev_[k].needs(bytes)) {
        const size_t want = doubled(4096, bytes);
        host_[k].reset(); dev_[k].reset();
        TSQ_HIP(c, host_[k].grow(want));
        if (!dev_[k].grow(c, want)) return TSQA_ERR_HIP;
    }
    *slot = Slot{this, k};
    return TSQA_OK;
}

void tsqa_uploads::destroy()
{
    for (int k = 0; k < 2; ++k)
        if (done_[k]) (void)hipEventDestroy(done_[k]);
}

// Per-item scratch of the batch entry points (tsq_internal.h), doubled from 256 items.
int tsqa_ctx::reserve_batch(size_t n_items)
{
    (void)hipSetDevice(device);
    const size_t want = doubled(256, n_items), one = want ? 1 : 0;
    if (!batch_at.needs(want) && !batch_sizes.needs(want) && !batch_offsets.needs(want + one) && !batch_heads.needs(want * kHeaderSize) &&
        !batch_status.needs(want) && !batch_items.needs(want) && !batch_live.needs(one)) return TSQA_OK;
    // (batch calls run on callers' streams too, and one enqueued there may still be using the tables that are freed below)
    (void)hipDeviceSynchronize();
    return batch_at.grow(this, want) && batch_sizes.grow(this, want) && batch_offsets.grow(this, want + one) &&
           batch_heads.grow(this, want * kHeaderSize) && batch_status.grow(this, want) && batch_items.grow(this, want) &&
           batch_live.grow(this, one) ? TSQA_OK : TSQA_ERR_HIP;
}

// Scratch of the calls whose block descriptors are made on the device (tsq_internal.h): the descriptors doubled from 256, the launch
// table from 16, each on its own; want_items (every packed batch): a word per block for its item, as many as descriptors.
int tsqa_ctx::reserve_tables(size_t n_blocks, size_t n_launches, bool want_items)
{
    (void)hipSetDevice(device);
    const size_t blocks = doubled(256, n_blocks), launches = doubled(16, n_launches), owners = want_items ? blocks : 0;
    if (!table_blocks.needs(blocks) && !table_launch_item.needs(launches) && !table_block_item.needs(owners)) return TSQA_OK;
    (void)hipDeviceSynchronize();                        // (as in reserve_batch: a call enqueued on any stream may still be using them)
    return table_blocks.grow(this, blocks) && table_launch_item.grow(this, launches) && table_block_item.grow(this, owners) ? TSQA_OK : TSQA_ERR_HIP;
}

// Scratch of the join (tsq_internal.h) beside the batch tables: the body places, doubled from 256 items like them.
int tsqa_ctx::reserve_join(size_t n_items)
{
    if (int rc = reserve_batch(n_items)) return rc;
    const size_t want = doubled(256, n_items) + 1;
    if (!join_at.needs(want)) return TSQA_OK;
    (void)hipDeviceSynchronize();                        // (as in reserve_batch)
    return join_at.grow(this, want) ? TSQA_OK : TSQA_ERR_HIP;
}

// Scratch of the cut (tsq_internal.h): one entry per range and one more, doubled from 256 ranges as the join's grows, and one word
// per group of 256 ranges, doubled with them.
int tsqa_ctx::reserve_cut(size_t n_ranges)
{
    (void)hipSetDevice(device);
    const size_t ranges = doubled(256, n_ranges) + 1, groups = doubled(256, n_ranges) / 256;
    if (!cut_ranges.needs(ranges) && !cut_groups.needs(groups)) return TSQA_OK;
    (void)hipDeviceSynchronize();                        // (as in reserve_batch)
    return cut_ranges.grow(this, ranges) && cut_groups.grow(this, groups) ? TSQA_OK : TSQA_ERR_HIP;
}

// Scratch of the gather (tsq_internal.h): the ranges doubled from 256 as the cut's, the piece slots and groups as many as the call
// names (cap_pieces is the caller's statement of what the call may hold, and the sort runs over exactly that many pairs), each
// buffer on its own.  The sort's temporary storage is asked for here, once per cap_pieces, not per call.  The rows' places and
// group sums (tsqa_gather_rows_async) grow with the ranges.
int tsqa_ctx::reserve_gather(size_t n_ranges, size_t cap_pieces, size_t cap_groups)
{
    (void)hipSetDevice(device);
    if (gather_sort_n != cap_pieces) {
        size_t bytes = 0;
        TSQ_HIP(this, gather_sort_storage(cap_pieces > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)cap_pieces, &bytes));
        gather_sort_n = cap_pieces; gather_sort_bytes = bytes ? bytes : 1;
    }
    const size_t want = doubled(256, n_ranges);
    if (!gather_ranges.needs(want) && !gather_items.needs(2 * cap_pieces) && !gather_keys.needs(2 * cap_pieces) && !gather_slots.needs(2 * cap_pieces) &&
        !gather_groups.needs(cap_groups) && !gather_sort.needs(gather_sort_bytes) && !gather_words.needs(1) && !gather_places.needs(want) &&
        !gather_row_groups.needs(want / 256)) return TSQA_OK;
    (void)hipDeviceSynchronize();                        // (as in reserve_batch)
    return gather_ranges.grow(this, want) && gather_items.grow(this, 2 * cap_pieces) && gather_keys.grow(this, 2 * cap_pieces) &&
           gather_slots.grow(this, 2 * cap_pieces) && gather_groups.grow(this, cap_groups) && gather_sort.grow(this, gather_sort_bytes) &&
           gather_words.grow(this, 1) && gather_places.grow(this, want) && gather_row_groups.grow(this, want / 256) ? TSQA_OK : TSQA_ERR_HIP;
}

// Scratch of the record scan (tsq_internal.h): the bit map as many words as the call names -- it is the one buffer here that
// follows the data's size, an eighth of it, and is not doubled --, the per-block entries doubled from 256 and two words per group of
// 256 blocks with them.
int tsqa_ctx::reserve_records(size_t map_words, size_t n_blocks)
{
    (void)hipSetDevice(device);
    const size_t blocks = doubled(256, n_blocks), groups = 2 * (blocks / 256);
    if (!records_map.needs(map_words) && !records_blocks.needs(blocks) && !records_groups.needs(groups) && !records_words.needs(1)) return TSQA_OK;
    (void)hipDeviceSynchronize();                        // (as in reserve_batch)
    return records_map.grow(this, map_words) && records_blocks.grow(this, blocks) && records_groups.grow(this, groups) &&
           records_words.grow(this, 1) ? TSQA_OK : TSQA_ERR_HIP;
}

// Scratch of the find: the records' (the map is shared; every call clears it), 32 edge bytes per block and the scan's two words.
int tsqa_ctx::reserve_find(size_t map_words, size_t n_blocks)
{
    if (int rc = reserve_records(map_words, n_blocks)) return rc;
    const size_t edges = 32 * doubled(256, n_blocks);
    if (!find_edges.needs(edges) && !find_need.needs(2)) return TSQA_OK;
    (void)hipDeviceSynchronize();                        // (as in reserve_batch)
    return find_edges.grow(this, edges) && find_need.grow(this, 2) ? TSQA_OK : TSQA_ERR_HIP;
}

// Scratch of the CRC: the call's word, then one word per block (R of the block); every call clears it.
int tsqa_ctx::reserve_crc(size_t n_blocks)
{
    const size_t words = 1 + doubled(256, n_blocks);
    if (!crc_blocks.needs(words)) return TSQA_OK;
    (void)hipDeviceSynchronize();                        // (as in reserve_batch)
    return crc_blocks.grow(this, words) ? TSQA_OK : TSQA_ERR_HIP;
}

// ---- kernel timing ----
// One timed span of `kind` on `s`, where profiling is on and the kind has a pair left: the opening event is recorded here, the
// closing one by end(); cancel() gives the pair back when what the span was to time was never enqueued.
struct ProfSpan {
    tsqa_ctx* const c;
    const int kind;
    const hipStream_t s;
    size_t at = 0;
    bool timed = false;
    ProfSpan(tsqa_ctx* c_, int kind_, hipStream_t s_) : c(c_), kind(kind_), s(s_)
    {
        if (!c->profiling || c->prof_used[kind] >= (uint32_t)tsqa_ctx::kProfPairs) return;
        at = ((size_t)kind * tsqa_ctx::kProfPairs + c->prof_used[kind]++) * 2;
        (void)hipEventRecord(c->prof_pool[at], s);
        timed = true;
    }
    void end() { if (timed) (void)hipEventRecord(c->prof_pool[at + 1], s); }
    void cancel() { if (timed) c->prof_used[kind]--; }
};

extern "C" int tsqa_profile_enable(tsqa_ctx* c, int on)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (on && c->prof_pool.empty()) {
        c->prof_pool.resize((size_t)tsqa_ctx::kProfKinds * tsqa_ctx::kProfPairs * 2, nullptr);
        for (auto& e : c->prof_pool)
            if (hipEventCreate(&e) != hipSuccess) {
                // all or nothing: a half-made pool would hand null events to hipEventRecord later
                for (hipEvent_t made : c->prof_pool) if (made) (void)hipEventDestroy(made);
                c->prof_pool.clear();
                c->profiling = false;
                c->set_error("hipEventCreate failed");
                return TSQA_ERR_HIP;
            }
    }
    c->profiling = on != 0;
    return TSQA_OK;
}

static void drain_events(tsqa_ctx* c, int kind, double* ms, uint32_t* count)
{
    double sum = 0; uint32_t n = 0;
    for (uint32_t k = 0; k < c->prof_used[kind]; ++k) {
        const size_t at = ((size_t)kind * tsqa_ctx::kProfPairs + k) * 2;
        float t = 0;
        if (hipEventSynchronize(c->prof_pool[at + 1]) == hipSuccess && hipEventElapsedTime(&t, c->prof_pool[at], c->prof_pool[at + 1]) == hipSuccess) { sum += t; n++; }
    }
    c->prof_used[kind] = 0;
    if (ms) *ms = sum;
    if (count) *count = n;
}

extern "C" int tsqa_profile_read(tsqa_ctx* c, double* enc_ms, uint32_t* enc_n, double* dec_ms, uint32_t* dec_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (enc_ms) *enc_ms = 0; if (enc_n) *enc_n = 0; if (dec_ms) *dec_ms = 0; if (dec_n) *dec_n = 0; return TSQA_OK; }
    drain_events(c, 0, enc_ms, enc_n);
    drain_events(c, 1, dec_ms, dec_n);
    return TSQA_OK;
}

extern "C" int tsqa_profile_read_calls(tsqa_ctx* c, double* comp_ms, uint32_t* comp_n, double* decomp_ms, uint32_t* decomp_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (comp_ms) *comp_ms = 0; if (comp_n) *comp_n = 0; if (decomp_ms) *decomp_ms = 0; if (decomp_n) *decomp_n = 0; return TSQA_OK; }
    drain_events(c, 2, comp_ms, comp_n);
    drain_events(c, 3, decomp_ms, decomp_n);
    return TSQA_OK;
}

extern "C" int tsqa_profile_read_join(tsqa_ctx* c, double* emit_ms, uint32_t* emit_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (emit_ms) *emit_ms = 0; if (emit_n) *emit_n = 0; return TSQA_OK; }
    drain_events(c, 4, emit_ms, emit_n);
    return TSQA_OK;
}

extern "C" int tsqa_profile_read_cut(tsqa_ctx* c, double* emit_ms, uint32_t* emit_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (emit_ms) *emit_ms = 0; if (emit_n) *emit_n = 0; return TSQA_OK; }
    drain_events(c, 5, emit_ms, emit_n);
    return TSQA_OK;
}

extern "C" int tsqa_profile_read_gather(tsqa_ctx* c, double* plan_ms, uint32_t* plan_n, double* dec_ms, uint32_t* dec_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (plan_ms) *plan_ms = 0; if (plan_n) *plan_n = 0; if (dec_ms) *dec_ms = 0; if (dec_n) *dec_n = 0; return TSQA_OK; }
    drain_events(c, 6, plan_ms, plan_n);
    drain_events(c, 7, dec_ms, dec_n);
    return TSQA_OK;
}

extern "C" int tsqa_profile_read_rows(tsqa_ctx* c, double* pad_ms, uint32_t* pad_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (pad_ms) *pad_ms = 0; if (pad_n) *pad_n = 0; return TSQA_OK; }
    drain_events(c, 8, pad_ms, pad_n);
    return TSQA_OK;
}

extern "C" int tsqa_profile_read_records(tsqa_ctx* c, double* mark_ms, uint32_t* mark_n, double* table_ms, uint32_t* table_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (mark_ms) *mark_ms = 0; if (mark_n) *mark_n = 0; if (table_ms) *table_ms = 0; if (table_n) *table_n = 0; return TSQA_OK; }
    drain_events(c, 9, mark_ms, mark_n);
    drain_events(c, 10, table_ms, table_n);
    return TSQA_OK;
}

extern "C" int tsqa_profile_read_find(tsqa_ctx* c, double* find_ms, uint32_t* find_n, double* table_ms, uint32_t* table_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (find_ms) *find_ms = 0; if (find_n) *find_n = 0; if (table_ms) *table_ms = 0; if (table_n) *table_n = 0; return TSQA_OK; }
    drain_events(c, 11, find_ms, find_n);
    drain_events(c, 12, table_ms, table_n);
    return TSQA_OK;
}

extern "C" int tsqa_profile_read_crc(tsqa_ctx* c, double* decode_ms, uint32_t* decode_n, double* fold_ms, uint32_t* fold_n)
{
    if (!c) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    if (c->prof_pool.empty()) { if (decode_ms) *decode_ms = 0; if (decode_n) *decode_n = 0; if (fold_ms) *fold_ms = 0; if (fold_n) *fold_n = 0; return TSQA_OK; }
    drain_events(c, 13, decode_ms, decode_n);
    drain_events(c, 14, fold_ms, fold_n);
    return TSQA_OK;
}

// ---- internal launches (also used by the reference-API layer in tsq_compat.hip) ----

int tsqa_ctx::launch_encode_to(const void* d_in, size_t n, size_t readable, size_t stride, uint32_t ext, uint8_t* slots_out,
                               uint32_t* sizes_out, int32_t* status, hipStream_t s)
{
    const uint32_t nb = (uint32_t)tsqa_block_count(n);
    int rc = reserve(nb, true, false, false, s);         // (the streams go to the caller's slots: the context's own are not needed here)
    if (rc) return rc;
    ProfSpan span(this, 0, s);
    rc = launch_encode_kernels(this, static_cast<const uint8_t*>(d_in), n, readable, stride, ext, slots_out, sizes_out, status, s);
    if (rc) { span.cancel(); return rc; }
    span.end();
    TSQ_HIP(this, hipGetLastError());
    return TSQA_OK;
}

int tsqa_ctx::launch_encode(const void* d_in, size_t n, size_t readable, uint32_t ext, int32_t* status, hipStream_t s)
{
    int rc = reserve((uint32_t)tsqa_block_count(n), true, true, false, s);
    if (rc) return rc;
    return launch_encode_to(d_in, n, readable, kBlockSize, ext, slots, sizes, status, s);
}

// Every scan in this file -- the pack scans, the sized frame walk, the batch layouts, the index scans -- is launched with workgroups of
// exactly 256 threads: group_scan_excl64 sums four full wavefronts.

// The copy pieces a block's stream takes when no stream is longer than max_stream.
static uint32_t pack_pieces(uint32_t max_stream = kSlotSize) { return (max_stream + kPackPiece - 1) / kPackPiece + 1; }

int tsqa_ctx::launch_pack(size_t n, uint32_t ext, void* d_out, size_t out_cap, uint64_t* d_out_size, int32_t* status, hipStream_t s)
{
    const uint32_t nb = (uint32_t)tsqa_block_count(n);
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(256), 0, s, sizes, nb, (uint64_t)n, ext,
                       static_cast<uint8_t*>(d_out), (uint64_t)out_cap, frame_at, d_out_size, status);
    hipLaunchKernelGGL(pack_copy_kernel, dim3(pack_pieces(), nb), dim3(256), 0, s, slots, sizes, frame_at,
                       static_cast<uint8_t*>(d_out), status);
    TSQ_HIP(this, hipGetLastError());
    return TSQA_OK;
}

int tsqa_ctx::launch_decode_frames(const void* d_streams, const FrameInfo* d_frames, uint32_t n_blocks, void* d_out, int32_t* status, hipStream_t s, int variant)
{
    ProfSpan span(this, 1, s);
    int rc = launch_decode_kernels(this, static_cast<const uint8_t*>(d_streams), d_frames, n_blocks, static_cast<uint8_t*>(d_out), status, s, variant);
    if (rc) { span.cancel(); return rc; }
    span.end();
    TSQ_HIP(this, hipGetLastError());
    return TSQA_OK;
}

int tsqa_ctx::decode_again(const void* d_streams, const FrameInfo* d_frames, uint32_t n_blocks, void* d_out, int32_t* status, hipStream_t s)
{
    TSQ_HIP(this, hipMemsetAsync(status, 0, sizeof(int32_t), s));
    return launch_decode_frames(d_streams, d_frames, n_blocks, d_out, status, s, 4);
}

// ---- public device-resident entry points ----

extern "C" int tsqa_compress_device_async(tsqa_ctx* c, const void* d_in, size_t n, void* d_out, size_t out_cap,
                                          uint64_t* d_out_size, int32_t* d_status, uint32_t ext, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_in || !d_out || !d_out_size || !d_status || n == 0) { c->set_error("compress: null pointer or zero size"); return TSQA_ERR_ARG; }
    if (out_cap < 16 + 6 * tsqa_block_count(n)) { c->set_error("compress: output capacity too small"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    ProfSpan span(c, 2, s);
    int rc = c->launch_encode(d_in, n, n, ext, d_status, s);
    if (rc) { span.cancel(); return rc; }
    rc = c->launch_pack(n, ext, d_out, out_cap, d_out_size, d_status, s);
    span.end();
    return rc;
}

static int status_to_rc(tsqa_ctx* c, int32_t st, const char* what)
{
    if (st == 0) return TSQA_OK;
    c->set_error("%s: device reported status %d", what, st);
    return st;
}

// The tail of the synchronous entry points: the context's status word comes back behind whatever the caller has queued on `s`
// (the call itself, copies of its sizes or offsets to the host), and the stream is waited for.  out_size != NULL: the context's
// size word comes back with it, and is stored before the status is judged.
static int read_status(tsqa_ctx* c, hipStream_t s, int32_t* st, size_t* out_size = nullptr)
{
    uint64_t sz = 0;
    if (out_size) TSQ_HIP(c, hipMemcpyAsync(&sz, c->d_size, sizeof(sz), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipMemcpyAsync(st, c->d_status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    if (out_size) *out_size = (size_t)sz;
    return TSQA_OK;
}
static int finish_sync(tsqa_ctx* c, hipStream_t s, const char* what, size_t* out_size = nullptr)
{
    int32_t st = 0;
    if (int rc = read_status(c, s, &st, out_size)) return rc;
    return status_to_rc(c, st, what);
}

extern "C" int tsqa_compress_device(tsqa_ctx* c, const void* d_in, size_t n, void* d_out, size_t out_cap,
                                    size_t* out_size, uint32_t ext, void* hip_stream)
{
    if (!c || !out_size) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    int rc = tsqa_compress_device_async(c, d_in, n, d_out, out_cap, c->d_size, c->d_status, ext, s);
    if (rc) return rc;
    return finish_sync(c, s, "compress", out_size);
}

// (variant < 0: the context's decode variant; the retry after TSQA_ERR_STALL passes 4 without touching the context's setting.
//  sized: the frame walk is made in parallel from d_block_sizes, frame_walk_sized_kernel; else that table is not looked at.)
static int decompress_device_async_impl(tsqa_ctx* c, const void* d_in, size_t n, uint32_t n_blocks, void* d_out,
                                        size_t out_cap, uint64_t* d_out_size, int32_t* d_status, void* hip_stream, int variant,
                                        bool sized = false, const uint32_t* d_block_sizes = nullptr)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_in || !d_out || !d_out_size || !d_status || n < 16 || n_blocks == 0 || (sized && !d_block_sizes)) { c->set_error("decompress: bad argument"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    int rc = c->reserve(n_blocks, false, false, false, s);
    if (rc) return rc;
    c->forget_sharded();                                 // the frame walk below overwrites c->frames
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    ProfSpan span(c, 3, s);
    if (sized)
        hipLaunchKernelGGL(frame_walk_sized_kernel, dim3(1), dim3(256), 0, s, static_cast<const uint8_t*>(d_in), (uint64_t)n, n_blocks,
                           d_block_sizes, (uint64_t)out_cap, c->frames, d_out_size, d_status);
    else
        hipLaunchKernelGGL(frame_walk_kernel, dim3(1), dim3(64), 0, s, static_cast<const uint8_t*>(d_in), (uint64_t)n, n_blocks,
                           (uint64_t)out_cap, c->frames, d_out_size, d_status);
    rc = c->launch_decode_frames(d_in, c->frames, n_blocks, d_out, d_status, s, variant);
    span.end();
    return rc;
}

extern "C" int tsqa_decompress_device_async(tsqa_ctx* c, const void* d_in, size_t n, uint32_t n_blocks, void* d_out,
                                            size_t out_cap, uint64_t* d_out_size, int32_t* d_status, void* hip_stream)
{
    return decompress_device_async_impl(c, d_in, n, n_blocks, d_out, out_cap, d_out_size, d_status, hip_stream, -1);
}

extern "C" int tsqa_decompress_device_sized_async(tsqa_ctx* c, const void* d_in, size_t n, uint32_t n_blocks, const uint32_t* d_block_sizes,
                                                  void* d_out, size_t out_cap, uint64_t* d_out_size, int32_t* d_status, void* hip_stream)
{
    return decompress_device_async_impl(c, d_in, n, n_blocks, d_out, out_cap, d_out_size, d_status, hip_stream, -1, true, d_block_sizes);
}

// ---- sharded operation: a device owns some of a job's blocks ----

extern "C" int tsqa_encode_blocks_async(tsqa_ctx* c, const void* d_in, uint32_t n_blocks, size_t stride, uint32_t last_len,
                                        uint32_t ext, void* d_slots, uint32_t* d_sizes, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_in || !d_slots || !d_sizes || !d_status || n_blocks == 0 || last_len == 0 || last_len > kBlockSize || stride < kBlockSize) {
        c->set_error("encode_blocks: bad argument");
        return TSQA_ERR_ARG;
    }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    // the virtual total gives every block but the last 4 MiB; what may be read ends with the last block's look-ahead
    const size_t n = (size_t)(n_blocks - 1) * kBlockSize + last_len;
    const size_t tail = stride > kBlockSize ? (stride - kBlockSize < 128 ? stride - kBlockSize : 128) : 0;
    const size_t readable = (size_t)(n_blocks - 1) * stride + last_len + tail;
    return c->launch_encode_to(d_in, n, readable, stride, ext, static_cast<uint8_t*>(d_slots), d_sizes, d_status, s);
}

extern "C" int tsqa_decode_blocks_async(tsqa_ctx* c, const void* d_streams, const tsqa_frame* d_frames, uint32_t n_blocks,
                                        void* d_out, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_streams || !d_frames || !d_out || !d_status || n_blocks == 0) { c->set_error("decode_blocks: bad argument"); return TSQA_ERR_ARG; }
    static_assert(sizeof(tsqa_frame) == sizeof(FrameInfo), "public frame descriptor = kernel frame descriptor");
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    return c->launch_decode_frames(d_streams, reinterpret_cast<const FrameInfo*>(d_frames), n_blocks, d_out, d_status, s);
}

// Both waiting forms (sized: tsqa_decompress_device_sized, the frame walk from the table_words words at d_block_sizes).
static int decompress_device_wait(tsqa_ctx* c, const void* d_in, size_t n, void* d_out, size_t out_cap, size_t* out_size, void* hip_stream,
                                  bool sized, uint32_t table_words, const uint32_t* d_block_sizes)
{
    if (!c || !out_size) return TSQA_ERR_ARG;
    if (!d_in || n < 16 || (sized && (!d_block_sizes || table_words == 0))) { c->set_error("decompress: bad argument"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    uint8_t head[kHeaderSize];
    TSQ_HIP(c, hipMemcpyAsync(head, d_in, kHeaderSize, hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    uint32_t nb = 0; uint64_t total = 0;
    const int h = read_header(head, n, &nb, &total);
    if (h == kHeaderBadMagic || h == kHeaderNoBlocks) { c->set_error("decompress: bad magic or no blocks"); return TSQA_ERR_FORMAT; }
    if (total > out_cap) { c->set_error("decompress: output capacity %zu < %llu", out_cap, (unsigned long long)total); return TSQA_ERR_ARG; }
    // (an implausible header is refused with *out_size = 0, as the frame walk would refuse it)
    if (h != kHeaderOk) { *out_size = 0; c->set_error("decompress: more blocks or bytes than a container of %zu B can hold", n); return TSQA_ERR_FORMAT; }
    // (the table holds as many words as the caller says, not as many as the container says: no kernel walks a table by a count
    //  the caller has not vouched for)
    if (sized && nb != table_words) { *out_size = 0; c->set_error("decompress: the header states %u blocks, the size table holds %u", nb, table_words); return TSQA_ERR_FORMAT; }
    int32_t st = 0;
    // after TSQA_ERR_STALL -- a workgroup of a several-workgroups-per-block decode did not get onto the GPU in time (other work held
    // the CUs): the container is not at fault -- once more with one workgroup per block, which waits for nobody
    for (int variant : {-1, 4}) {
        if (int rc = decompress_device_async_impl(c, d_in, n, nb, d_out, out_cap, c->d_size, c->d_status, s, variant, sized, d_block_sizes)) return rc;
        if (int rc = read_status(c, s, &st, out_size)) return rc;
        if (st != kErrStall) break;
    }
    return status_to_rc(c, st, "decompress");
}

extern "C" int tsqa_decompress_device(tsqa_ctx* c, const void* d_in, size_t n, void* d_out, size_t out_cap,
                                      size_t* out_size, void* hip_stream)
{
    return decompress_device_wait(c, d_in, n, d_out, out_cap, out_size, hip_stream, false, 0u, nullptr);
}

extern "C" int tsqa_decompress_device_sized(tsqa_ctx* c, const void* d_in, size_t n, uint32_t n_blocks, const uint32_t* d_block_sizes, void* d_out,
                                            size_t out_cap, size_t* out_size, void* hip_stream)
{
    return decompress_device_wait(c, d_in, n, d_out, out_cap, out_size, hip_stream, true, n_blocks, d_block_sizes);
}

// Host gather / scatter of a shard's frames (what compression_write_worker and decompression_read_worker do with
// memcpy, tsq_threads.cpp:226-239,513-524): one DMA per owned block between its slot in HBM and its place in the
// container in host memory.  The three frame bytes are written / skipped here.
extern "C" int tsqa_frames_to_host_async(tsqa_ctx* c, const void* d_slots, const uint32_t* sizes, const uint64_t* frame_at,
                                         uint32_t n_blocks, uint32_t ext, void* host_container, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_slots || !sizes || !frame_at || !host_container) { c->set_error("frames_to_host: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    uint8_t* base = static_cast<uint8_t*>(host_container);
    // every size is checked before anything is written or enqueued (no partial container on an error)
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (!stream_len_ok(sizes[b])) { c->set_error("frames_to_host: block %u has size %u", b, sizes[b]); return TSQA_ERR_ARG; }
    for (uint32_t b = 0; b < n_blocks; ++b) {
        uint8_t* p = base + frame_at[b];
        write_frame(p, sizes[b], ext);
        TSQ_HIP(c, hipMemcpyAsync(p + kFrameWordSize, static_cast<const uint8_t*>(d_slots) + (size_t)b * kSlotSize, sizes[b], hipMemcpyDeviceToHost, s));
    }
    return TSQA_OK;
}

extern "C" int tsqa_frames_from_host_async(tsqa_ctx* c, const void* host_container, const uint64_t* frame_at, const uint32_t* sizes,
                                           uint32_t n_blocks, void* d_streams, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_streams || !sizes || !frame_at || !host_container) { c->set_error("frames_from_host: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    const uint8_t* base = static_cast<const uint8_t*>(host_container);
    // every size is checked before a copy is enqueued (a refusal writes nothing to d_streams)
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (!stream_len_ok(sizes[b])) { c->set_error("frames_from_host: block %u has size %u", b, sizes[b]); return TSQA_ERR_FORMAT; }
    for (uint32_t b = 0; b < n_blocks; ++b) {
        TSQ_HIP(c, hipMemcpyAsync(static_cast<uint8_t*>(d_streams) + (size_t)b * kSlotSize, base + frame_at[b] + kFrameWordSize, sizes[b], hipMemcpyHostToDevice, s));
    }
    return TSQA_OK;
}

// ---- one step of a block-sharded job on this rank (block b of the job belongs to rank b % world) ----
// Host-only helpers first (no device involved): the writer's frame offsets and the reader's frame walk
// (tsq_threads.cpp:226-239,513-524) over a container in host memory.
extern "C" int tsqa_frame_offsets(const uint32_t* sizes, uint32_t n_blocks, uint64_t* frame_at, uint64_t* container_size)
{
    if (!sizes || !frame_at || !container_size) return TSQA_ERR_ARG;
    uint64_t at = kHeaderSize;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        if (!stream_len_ok(sizes[b])) return TSQA_ERR_ARG;
        frame_at[b] = at;
        at += kFrameWordSize + (uint64_t)sizes[b];
    }
    *container_size = at;
    return TSQA_OK;
}

extern "C" int tsqa_walk_frames(const void* container, size_t size, uint32_t cap_blocks, uint64_t* frame_at, uint32_t* sizes, uint32_t* ext,
                                uint32_t* out_len, uint32_t* n_blocks, uint64_t* total)
{
    if (!container || !frame_at || !sizes || !ext || !out_len || !n_blocks || !total) return TSQA_ERR_ARG;
    const uint8_t* p = static_cast<const uint8_t*>(container);
    uint32_t nb; uint64_t tot;
    if (read_header(p, size, &nb, &tot) != kHeaderOk || nb > cap_blocks) return TSQA_ERR_FORMAT;
    const WalkVerdict v = walk_frames(p, size, nb, tot, [&](uint32_t b, uint64_t at, const FrameInfo& f) {
        frame_at[b] = at; sizes[b] = f.stream_len; ext[b] = f.ext; out_len[b] = f.out_len;
        return true;
    });
    if (v != kWalkOk) return TSQA_ERR_FORMAT;
    *n_blocks = nb; *total = tot;
    return TSQA_OK;
}

// After the encode of the owned blocks and the all-gather of every block's stream size: this rank's frames go to their final
// place in ONE container in host memory (rank 0 also writes the 16-byte header).  The whole "gather" of the writer thread
// (tsq_threads.cpp:192-275) is this prefix sum and one DMA per owned block.
extern "C" int tsqa_sharded_place_async(tsqa_ctx* c, const void* d_slots, const uint32_t* all_sizes, uint32_t n_blocks, uint64_t n_total,
                                        uint32_t rank, uint32_t world, uint32_t ext, void* host_container, size_t host_cap,
                                        uint64_t* container_size, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_slots || !all_sizes || !host_container || !container_size || world == 0 || rank >= world || n_blocks == 0) { c->set_error("sharded_place: bad argument"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    uint8_t* base = static_cast<uint8_t*>(host_container);
    // every size and the capacity are checked before anything is written or enqueued (no partial container on an error)
    uint64_t at = kHeaderSize;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t sz = all_sizes[b];
        if (!stream_len_ok(sz)) { c->set_error("sharded_place: block %u has size %u", b, sz); return TSQA_ERR_ARG; }
        at += kFrameWordSize + (uint64_t)sz;
    }
    if (at > host_cap) { c->set_error("sharded_place: the host container is too small (%llu > %zu)", (unsigned long long)at, host_cap); return TSQA_ERR_ARG; }
    at = kHeaderSize;
    for (uint32_t b = 0; b < n_blocks; ++b) {
        const uint32_t sz = all_sizes[b];
        if (b % world == rank) {
            write_frame(base + at, sz, ext);
            TSQ_HIP(c, hipMemcpyAsync(base + at + kFrameWordSize, static_cast<const uint8_t*>(d_slots) + (size_t)(b / world) * kSlotSize, sz, hipMemcpyDeviceToHost, s));
        }
        at += kFrameWordSize + (uint64_t)sz;
    }
    if (rank == 0) write_header(base, n_blocks, n_total);                                 // tsq_threads.cpp:333-335
    *container_size = at;
    return TSQA_OK;
}

// The reader's side: walk the container's frames (host memory), bring this rank's frames to d_streams (frame k of the rank at
// k * TSQ_OUTPUT_SZ) and decode them back to back into d_out (block k of the rank at k * TSQ_BLOCK_SZ).
extern "C" int tsqa_sharded_fetch_decode_async(tsqa_ctx* c, const void* host_container, size_t container_size, uint32_t rank, uint32_t world,
                                               void* d_streams, size_t streams_cap, void* d_out, size_t out_cap, int32_t* d_status, uint64_t* total,
                                               void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!host_container || !d_streams || !d_out || !d_status || !total || world == 0 || rank >= world) { c->set_error("sharded_fetch_decode: bad argument"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    const uint8_t* p = static_cast<const uint8_t*>(host_container);
    c->forget_sharded();                                 // whatever happens below, an older call's descriptors are not to be decoded again
    uint32_t nb; uint64_t tot;
    if (read_header(p, container_size, &nb, &tot) != kHeaderOk) { c->set_error("sharded_fetch_decode: bad header"); return TSQA_ERR_FORMAT; }
    const uint32_t n_local = nb > rank ? (nb - rank + world - 1) / world : 0;
    // The container is not trusted: the whole frame walk is validated -- against the container's own size and against what the caller's
    // buffers can hold -- before a single copy is enqueued (a container with more, shorter blocks than the job the buffers were sized
    // for must not overrun them).
    if ((uint64_t)n_local * kSlotSize > streams_cap) { c->set_error("sharded_fetch_decode: %u owned frames do not fit d_streams (%zu B)", n_local, streams_cap); return TSQA_ERR_FORMAT; }
    if (int rc = c->reserve(n_local ? n_local : 1, false, false, false, s)) return rc;
    if (int rc = c->reserve_host_frames(n_local ? n_local : 1)) return rc;
    const WalkVerdict v = walk_frames(p, container_size, nb, tot, [&](uint32_t b, uint64_t at, FrameInfo f) {
        if (b % world != rank) return true;
        const uint32_t k = b / world;
        if ((uint64_t)k * kBlockSize + f.out_len > out_cap) return false;
        f.stream_at = (uint64_t)k * kSlotSize; f.out_at = (uint64_t)k * kBlockSize;
        c->host_frames[k] = f;
        c->host_frame_src[k] = at + kFrameWordSize;
        return true;
    });
    if (v != kWalkOk) {
        c->set_error("sharded_fetch_decode: %s", v == kWalkBadFrame ? "malformed or truncated frame" :
                                                 v == kWalkBadSum ? "block sizes do not add up to the total" : "an owned block does not fit d_out");
        return TSQA_ERR_FORMAT;
    }
    *total = tot;
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    if (n_local == 0) return TSQA_OK;
    for (uint32_t k = 0; k < n_local; ++k)
        TSQ_HIP(c, hipMemcpyAsync(static_cast<uint8_t*>(d_streams) + (size_t)k * kSlotSize, p + c->host_frame_src[k], c->host_frames[k].stream_len, hipMemcpyHostToDevice, s));
    // (the descriptors live in pinned memory: the copy is a real DMA ordered on `s`, and reserve_host_frames has waited for the
    //  previous call's copy before they were overwritten)
    TSQ_HIP(c, hipMemcpyAsync(c->frames, c->host_frames, (size_t)n_local * sizeof(FrameInfo), hipMemcpyHostToDevice, s));
    TSQ_HIP(c, hipEventRecord(c->host_frames_copied, s));
    c->host_frames_pending = true;
    c->sharded_n_local = n_local; c->sharded_streams = d_streams; c->sharded_out = d_out;
    return c->launch_decode_frames(d_streams, c->frames, n_local, d_out, d_status, s);
}

// After *d_status of tsqa_sharded_fetch_decode_async came back TSQA_ERR_STALL: the owned frames and their descriptors are still on the
// device -- decode them again with one workgroup per block (decode variant 4), which waits for nobody.  A GPU of a sharded job holds
// few blocks, so its first attempt always takes the several-workgroups-per-block decoder; a busy GPU must not fail a valid container.
extern "C" int tsqa_sharded_decode_again_async(tsqa_ctx* c, const void* d_streams, void* d_out, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_streams || !d_out || !d_status) { c->set_error("sharded_decode_again: null pointer"); return TSQA_ERR_ARG; }
    if (c->sharded_n_local == 0) { c->set_error("sharded_decode_again: no sharded decode to repeat on this context (none yet, or another call has used the context since)"); return TSQA_ERR_ARG; }
    // the descriptors hold offsets into the buffers of THAT call: a retry into other buffers would decode them against the wrong memory
    if (d_streams != c->sharded_streams || d_out != c->sharded_out) { c->set_error("sharded_decode_again: not the buffers of the sharded decode being repeated"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    return c->decode_again(d_streams, c->frames, c->sharded_n_local, d_out, d_status, s);
}

// ---- range reads: an index of a device-resident container, and reads of byte ranges of its uncompressed data ----

// An index under construction: destroyed with whatever it holds by then, unless it is released to the caller.
struct IndexDeleter { void operator()(tsqa_index* idx) const { tsqa_index_destroy(idx); } };
using IndexPtr = std::unique_ptr<tsqa_index, IndexDeleter>;

// A new index for `who` (the caller's name in the error text; null when the host has no memory for it).  one_item: of a single
// container of nb blocks and `total` bytes, with out_start sized and, where host_copy, host_frames too; else the index of a batch,
// whose tables are made behind its walk.
static IndexPtr index_begin(tsqa_ctx* c, const char* who, const void* d_container, size_t n, uint32_t nb, uint64_t total, bool one_item, bool host_copy)
{
    IndexPtr idx(new (std::nothrow) tsqa_index());
    try {
        if (!idx) throw std::bad_alloc();
        idx->device = c->device; idx->container = static_cast<const uint8_t*>(d_container); idx->n = n; idx->n_blocks = nb; idx->total = total;
        if (host_copy) idx->host_frames.resize(nb);
        if (one_item) {
            idx->out_start.resize((size_t)nb + 1);
            idx->item_first = {0ull, (uint64_t)nb};
            idx->item_status = {TSQA_OK};
        }
    } catch (...) { c->set_error("%s: out of host memory", who); idx.reset(); }
    return idx;
}

extern "C" int tsqa_index_create(tsqa_ctx* c, const void* d_container, size_t n, tsqa_index** out)
{
    if (!out) return TSQA_ERR_ARG;
    *out = nullptr;
    if (!c) return TSQA_ERR_ARG;
    if (!d_container) { c->set_error("index_create: null container"); return TSQA_ERR_ARG; }
    if (n < kHeaderSize) { c->set_error("index_create: a container of %zu B has no header", n); return TSQA_ERR_FORMAT; }
    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    uint8_t head[kHeaderSize];
    TSQ_HIP(c, hipMemcpyAsync(head, d_container, kHeaderSize, hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    uint32_t nb; uint64_t total;
    if (read_header(head, n, &nb, &total) != kHeaderOk) { c->set_error("index_create: bad header"); return TSQA_ERR_FORMAT; }
    IndexPtr idx = index_begin(c, "index_create", d_container, n, nb, total, true, true);
    if (!idx) return TSQA_ERR_ARG;
    // the frame walk of a full decompress, into the index's own descriptors (the context's are left alone)
    int32_t st = 0;
    TSQ_HIP(c, hipMalloc(&idx->frames, (size_t)nb * sizeof(FrameInfo)));
    TSQ_HIP(c, hipMemsetAsync(c->d_status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(frame_walk_kernel, dim3(1), dim3(64), 0, s, idx->container, (uint64_t)n, nb, total, idx->frames, c->d_size, c->d_status);
    TSQ_HIP(c, hipGetLastError());
    TSQ_HIP(c, hipMemcpyAsync(&st, c->d_status, sizeof(st), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipMemcpyAsync(idx->host_frames.data(), idx->frames, (size_t)nb * sizeof(FrameInfo), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    if (st != 0) { c->set_error("index_create: malformed container (status %d)", st); return TSQA_ERR_FORMAT; }
    for (uint32_t b = 0; b < nb; ++b) idx->out_start[b] = idx->host_frames[b].out_at;
    idx->out_start[nb] = total;
    *out = idx.release();
    return TSQA_OK;
}

// The index of a container of short blocks from its table of stream sizes: the host plans from the caller's geometry alone, the
// device places the frames and proves the geometry (tsq_index.cuh).  Nothing is read back and no stream is waited for.
extern "C" int tsqa_index_create_sized_async(tsqa_ctx* c, const void* d_container, size_t n, uint64_t n_total, uint32_t block_len,
                                             const uint32_t* d_block_sizes, tsqa_index** out, void* hip_stream)
{
    if (!out) return TSQA_ERR_ARG;
    *out = nullptr;
    if (!c) return TSQA_ERR_ARG;
    if (!d_container || !d_block_sizes) { c->set_error("index_create_sized: null pointer"); return TSQA_ERR_ARG; }
    uint32_t nb = 0;
    size_t bound = 0;
    if (n_total > (uint64_t)SIZE_MAX || tsqa_plan_split((size_t)n_total, block_len, &nb, &bound)) {
        c->set_error("index_create_sized: no data, a block_len that is no power of two from 2^12 to 2^22, or more than 2^32 - 1 blocks");
        return TSQA_ERR_ARG;
    }
    if (n < kHeaderSize + (uint64_t)kMinFrameSize * nb) { c->set_error("index_create_sized: %zu B cannot hold %u frames", n, nb); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    IndexPtr idx = index_begin(c, "index_create_sized", d_container, n, nb, n_total, true, false);
    if (!idx) return TSQA_ERR_ARG;
    for (uint32_t b = 0; b < nb; ++b) idx->out_start[b] = (uint64_t)b * block_len;
    idx->out_start[nb] = n_total;
    idx->block_shift = (uint32_t)__builtin_ctz(block_len);
    // one allocation: the descriptors, the group sums, the verdict; all zero in front of the walk
    const uint32_t n_groups = (uint32_t)(((uint64_t)nb + kIndexGroup - 1u) / kIndexGroup);
    const size_t frames_bytes = (size_t)nb * sizeof(FrameInfo), bytes = frames_bytes + ((size_t)n_groups + 1u) * sizeof(uint64_t);
    TSQ_HIP(c, hipMalloc(&idx->frames, bytes));
    idx->group_sum = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(idx->frames) + frames_bytes);
    idx->verdict = reinterpret_cast<int32_t*>(idx->group_sum + n_groups);
    TSQ_HIP(c, hipMemsetAsync(idx->frames, 0, bytes, s));
    hipLaunchKernelGGL(index_sum_kernel, dim3(n_groups), dim3(256), 0, s, d_block_sizes, nb, idx->group_sum);
    hipLaunchKernelGGL(index_scan_kernel, dim3(1), dim3(256), 0, s, idx->container, (uint64_t)n, nb, n_total, idx->group_sum, n_groups, idx->verdict);
    hipLaunchKernelGGL(index_check_kernel, dim3(n_groups), dim3(256), 0, s, idx->container, (uint64_t)n, nb, n_total, block_len, d_block_sizes,
                       static_cast<const uint64_t*>(idx->group_sum), idx->frames, idx->verdict);
    TSQ_HIP(c, hipGetLastError());
    *out = idx.release();
    return TSQA_OK;
}

extern "C" int tsqa_index_create_sized(tsqa_ctx* c, const void* d_container, size_t n, uint64_t n_total, uint32_t block_len,
                                       const uint32_t* d_block_sizes, tsqa_index** out, void* hip_stream)
{
    if (!out) return TSQA_ERR_ARG;
    tsqa_index* made = nullptr;
    *out = nullptr;
    if (int rc = tsqa_index_create_sized_async(c, d_container, n, n_total, block_len, d_block_sizes, &made, hip_stream)) return rc;
    IndexPtr idx(made);
    hipStream_t s = stream_of(c, hip_stream);
    int32_t st = 0;
    TSQ_HIP(c, hipMemcpyAsync(&st, idx->verdict, sizeof(st), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    if (st != 0) { c->set_error("index_create_sized: the container is not what the size table and the geometry say (status %d)", st); return TSQA_ERR_FORMAT; }
    *out = idx.release();
    return TSQA_OK;
}

extern "C" const int32_t* tsqa_index_d_status(const tsqa_index* idx) { return idx ? idx->verdict : nullptr; }

// Behind the memset of a read's status word: an index made from a size table carries its walk's verdict, and a refused one
// refuses the read (index_gate_kernel).  The other kinds of index launch nothing here.
static void gate_read(const tsqa_index* idx, int32_t* d_status, hipStream_t s)
{
    if (idx->verdict) hipLaunchKernelGGL(index_gate_kernel, dim3(1), dim3(1), 0, s, static_cast<const int32_t*>(idx->verdict), d_status);
}

extern "C" void tsqa_index_destroy(tsqa_index* idx)
{
    if (!idx) return;
    (void)hipSetDevice(idx->device);
    (void)hipFree(idx->frames);
    (void)hipFree(idx->d_item_first);
    delete idx;
}

extern "C" uint32_t tsqa_index_blocks(const tsqa_index* idx) { return idx ? idx->n_blocks : 0u; }
extern "C" uint64_t tsqa_index_total(const tsqa_index* idx) { return idx ? idx->total : 0ull; }
extern "C" uint32_t tsqa_index_items(const tsqa_index* idx)
{
    return !idx ? 0u : idx->pending_items ? idx->pending_items : (uint32_t)idx->item_status.size();
}
extern "C" uint64_t tsqa_index_item_total(const tsqa_index* idx, uint32_t i)
{
    if (!idx || i >= idx->item_status.size()) return 0ull;
    return idx->out_start[idx->item_first[i + 1]] - idx->out_start[idx->item_first[i]];
}
extern "C" int tsqa_index_item_status(const tsqa_index* idx, uint32_t i)
{
    return idx && i < idx->item_status.size() ? idx->item_status[i] : TSQA_ERR_ARG;
}

// What a host-planned read says of a batch index made on the device whose tables have not come to the host (tsqa_index_create_packed_async).
static const char* const kNeedsFetch = "the index was made on the device and the host has none of its tables: call tsqa_index_fetch first (tsqa_gather_async needs none)";

// Two workgroups writing the same bytes would race: the destinations (at, length) of a call may touch, not overlap.  Sorts them.
static bool destinations_overlap(std::vector<std::pair<uint64_t, uint64_t>>& dst)
{
    std::sort(dst.begin(), dst.end());
    for (size_t k = 1; k < dst.size(); ++k)
        if (dst[k - 1].first + dst[k - 1].second > dst[k].first) return true;
    return false;
}

// tsqa_plan_ranges, with the reason for a refusal.  count_only: validate and count, write no item.
static int plan_ranges(const uint64_t* out_start, uint32_t nb, const tsqa_range* r, uint32_t nr, size_t out_cap, tsqa_range_item* items,
                       uint32_t cap_items, uint32_t* n_items, const char** why, bool count_only = false)
{
    *why = "";
    if (!out_start || !n_items || (nr && !r) || nb == 0) { *why = "null pointer or no blocks"; return TSQA_ERR_ARG; }
    if (out_start[0] != 0) { *why = "out_start[0] is not 0"; return TSQA_ERR_ARG; }
    for (uint32_t b = 0; b < nb; ++b)
        if (out_start[b + 1] < out_start[b] || out_start[b + 1] - out_start[b] > kBlockSize) { *why = "a block is longer than TSQ_BLOCK_SZ"; return TSQA_ERR_ARG; }
    const uint64_t total = out_start[nb];
    // the first block of a range: the last one that starts at or before its offset (blocks of length 0 are passed over)
    auto first_block = [&](uint64_t at) -> uint32_t { return (uint32_t)(std::upper_bound(out_start, out_start + nb + 1, at) - out_start) - 1u; };
    std::vector<std::pair<uint64_t, uint64_t>> dst;
    uint64_t count = 0;
    for (uint32_t k = 0; k < nr; ++k) {
        const tsqa_range& x = r[k];
        if (x.length == 0) continue;
        if (x.length > total || x.offset > total - x.length) { *why = "a range ends past the total"; return TSQA_ERR_ARG; }
        if (x.length > out_cap || x.out_at > out_cap - x.length) { *why = "a range does not fit the output"; return TSQA_ERR_ARG; }
        dst.emplace_back(x.out_at, x.length);
        const uint64_t end = x.offset + x.length;
        for (uint32_t b = first_block(x.offset); b < nb && out_start[b] < end; ++b) count += out_start[b + 1] > out_start[b];
    }
    if (destinations_overlap(dst)) { *why = "the destinations of two ranges overlap"; return TSQA_ERR_ARG; }
    if (count > 0xFFFFFFFFull) { *why = "more than 2^32 - 1 items"; return TSQA_ERR_ARG; }
    *n_items = (uint32_t)count;
    if (count_only) return TSQA_OK;
    if (count > cap_items) { *why = "the items do not fit cap_items"; return TSQA_ERR_ARG; }
    uint32_t m = 0;
    for (uint32_t k = 0; k < nr; ++k) {
        const tsqa_range& x = r[k];
        if (x.length == 0) continue;
        const uint64_t end = x.offset + x.length;
        for (uint32_t b = first_block(x.offset); b < nb && out_start[b] < end; ++b) {
            const uint64_t a = x.offset > out_start[b] ? x.offset : out_start[b], e = end < out_start[b + 1] ? end : out_start[b + 1];
            if (a >= e) continue;
            items[m++] = tsqa_range_item{b, (uint32_t)(a - out_start[b]), (uint32_t)(e - out_start[b]), 0u, x.out_at + (a - x.offset)};
        }
    }
    return TSQA_OK;
}

extern "C" int tsqa_plan_ranges(const uint64_t* out_start, uint32_t n_blocks, const tsqa_range* ranges, uint32_t n_ranges, size_t out_cap,
                                tsqa_range_item* items, uint32_t cap_items, uint32_t* n_items)
{
    const char* why;
    if (!items && cap_items) return TSQA_ERR_ARG;
    return plan_ranges(out_start, n_blocks, ranges, n_ranges, out_cap, items, cap_items, n_items, &why);
}

extern "C" int tsqa_decompress_ranges_async(tsqa_ctx* c, const tsqa_index* idx, const tsqa_range* ranges, uint32_t n_ranges, void* d_out,
                                            size_t out_cap, int32_t* d_status, void* hip_stream)
{
    static_assert(sizeof(tsqa_range_item) == sizeof(RangeItem), "public range item = kernel range item");
    if (!c) return TSQA_ERR_ARG;
    if (!idx || !d_out || !d_status || (n_ranges && !ranges)) { c->set_error("decompress_ranges: null pointer"); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("decompress_ranges: the index belongs to device %d, the context to %d", idx->device, c->device); return TSQA_ERR_ARG; }
    if (idx->pending_items) { c->set_error("decompress_ranges: %s", kNeedsFetch); return TSQA_ERR_ARG; }
    const char* why;
    uint32_t n_items = 0;
    if (plan_ranges(idx->out_start.data(), idx->n_blocks, ranges, n_ranges, out_cap, nullptr, 0, &n_items, &why, true)) {
        c->set_error("decompress_ranges: %s", why);
        return TSQA_ERR_ARG;
    }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    tsqa_uploads::Slot up;
    if (int rc = c->range_up.acquire(c, (size_t)(n_items ? n_items : 1) * sizeof(tsqa_range_item), &up)) return rc;
    // (the items are planned straight into the pinned buffer)
    if (plan_ranges(idx->out_start.data(), idx->n_blocks, ranges, n_ranges, out_cap, up.host<tsqa_range_item>(), (uint32_t)(up.cap() / sizeof(tsqa_range_item)), &n_items, &why)) {
        c->set_error("decompress_ranges: %s", why);
        return TSQA_ERR_ARG;
    }
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    gate_read(idx, d_status, s);
    if (n_items == 0) return TSQA_OK;
    TSQ_HIP(c, up.send((size_t)n_items * sizeof(tsqa_range_item), s));
    const int rc = launch_read_kernel<dec_range_kernel>(c, n_items, s, idx->container, idx->frames, idx->n_blocks, up.dev<RangeItem>(),
                                                        static_cast<uint8_t*>(d_out), d_status);
    TSQ_HIP(c, up.commit(s));
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_decompress_ranges(tsqa_ctx* c, const tsqa_index* idx, const tsqa_range* ranges, uint32_t n_ranges, void* d_out,
                                      size_t out_cap, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    int rc = tsqa_decompress_ranges_async(c, idx, ranges, n_ranges, d_out, out_cap, c->d_status, s);
    if (rc) return rc;
    return finish_sync(c, s, "decompress_ranges");
}

// ---- record reads: ranges addressed by item, one decode per touched block ----

// tsqa_plan_item_ranges, with the reason for a refusal: the ranges become ranges of the concatenation (plan_ranges cuts them at the
// block edges and checks the destinations), the items are sorted by (block, lo), and each block's items become one group.
static int plan_item_ranges(const uint64_t* out_start, uint32_t nb, const uint64_t* item_first, uint32_t n_items, const tsqa_item_range* r,
                            uint32_t nr, size_t out_cap, std::vector<tsqa_range_item>& items, std::vector<tsqa_block_group>& groups,
                            const char** why)
{
    *why = "";
    items.clear(); groups.clear();
    if (!out_start || !item_first || n_items == 0 || (nr && !r)) { *why = "null pointer or no items"; return TSQA_ERR_ARG; }
    if (item_first[0] != 0 || item_first[n_items] != nb) { *why = "item_first does not run from 0 to n_blocks"; return TSQA_ERR_ARG; }
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_first[i + 1] < item_first[i]) { *why = "item_first decreases"; return TSQA_ERR_ARG; }
    uint32_t n = 0;
    if (nb && plan_ranges(out_start, nb, nullptr, 0, out_cap, nullptr, 0, &n, why, true)) return TSQA_ERR_ARG;     // the block starts themselves
    std::vector<tsqa_range> flat;
    flat.reserve(nr);
    for (uint32_t k = 0; k < nr; ++k) {
        const tsqa_item_range& x = r[k];
        if (x.item >= n_items) { *why = "an item number past the index"; return TSQA_ERR_ARG; }
        const uint64_t fb = item_first[x.item], fe = item_first[x.item + 1];
        if (fb == fe) { *why = "a range of a refused item"; return TSQA_ERR_ARG; }
        const uint64_t total = out_start[fe] - out_start[fb];
        if (x.length > total || x.offset > total - x.length) { *why = "a range ends past its item's total"; return TSQA_ERR_ARG; }
        if (x.length) flat.push_back(tsqa_range{out_start[fb] + x.offset, x.length, x.out_at});
    }
    if (flat.empty()) return TSQA_OK;
    if (plan_ranges(out_start, nb, flat.data(), (uint32_t)flat.size(), out_cap, nullptr, 0, &n, why, true)) return TSQA_ERR_ARG;
    items.resize(n);
    if (plan_ranges(out_start, nb, flat.data(), (uint32_t)flat.size(), out_cap, items.data(), n, &n, why)) return TSQA_ERR_ARG;
    std::stable_sort(items.begin(), items.end(), [](const tsqa_range_item& p, const tsqa_range_item& q) {
        return p.block != q.block ? p.block < q.block : p.lo < q.lo;
    });
    for (uint32_t k = 0; k < n; ++k) {
        if (groups.empty() || groups.back().block != items[k].block) groups.push_back(tsqa_block_group{items[k].block, k, 0u, 0u});
        tsqa_block_group& g = groups.back();
        g.count++;
        g.hi = std::max(g.hi, items[k].hi);
    }
    return TSQA_OK;
}

extern "C" int tsqa_plan_item_ranges(const uint64_t* out_start, uint32_t n_blocks, const uint64_t* item_first_block, uint32_t n_items,
                                     const tsqa_item_range* ranges, uint32_t n_ranges, size_t out_cap, tsqa_range_item* items,
                                     uint32_t cap_items, uint32_t* n_range_items, tsqa_block_group* groups, uint32_t cap_groups,
                                     uint32_t* n_groups)
{
    const char* why;
    if (!n_range_items || !n_groups || (!items && cap_items) || (!groups && cap_groups)) return TSQA_ERR_ARG;
    std::vector<tsqa_range_item> vi;
    std::vector<tsqa_block_group> vg;
    try {
        if (plan_item_ranges(out_start, n_blocks, item_first_block, n_items, ranges, n_ranges, out_cap, vi, vg, &why)) return TSQA_ERR_ARG;
    } catch (...) { return TSQA_ERR_ARG; }
    *n_range_items = (uint32_t)vi.size();
    *n_groups = (uint32_t)vg.size();
    if (vi.size() > cap_items || vg.size() > cap_groups) return TSQA_ERR_ARG;
    std::copy(vi.begin(), vi.end(), items);
    std::copy(vg.begin(), vg.end(), groups);
    return TSQA_OK;
}

extern "C" int tsqa_decompress_item_ranges_async(tsqa_ctx* c, const tsqa_index* idx, const tsqa_item_range* ranges, uint32_t n_ranges,
                                                 void* d_out, size_t out_cap, int32_t* d_status, void* hip_stream)
{
    static_assert(sizeof(tsqa_block_group) == sizeof(BlockGroup) && sizeof(tsqa_item_range) == 32, "public group = kernel group");
    if (!c) return TSQA_ERR_ARG;
    if (!idx || !d_out || !d_status || (n_ranges && !ranges)) { c->set_error("decompress_item_ranges: null pointer"); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("decompress_item_ranges: the index belongs to device %d, the context to %d", idx->device, c->device); return TSQA_ERR_ARG; }
    if (idx->pending_items) { c->set_error("decompress_item_ranges: %s", kNeedsFetch); return TSQA_ERR_ARG; }
    const char* why = "out of host memory";
    std::vector<tsqa_range_item> vi;
    std::vector<tsqa_block_group> vg;
    int prc = TSQA_ERR_ARG;
    try {
        prc = plan_item_ranges(idx->out_start.data(), idx->n_blocks, idx->item_first.data(), (uint32_t)idx->item_status.size(), ranges, n_ranges,
                               out_cap, vi, vg, &why);
    } catch (...) {}
    if (prc) { c->set_error("decompress_item_ranges: %s", why); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    const uint32_t n_items = (uint32_t)vi.size(), n_groups = (uint32_t)vg.size();
    // one upload: the items, then (on a 16-byte boundary) the groups
    const size_t groups_at = ((size_t)n_items * sizeof(tsqa_range_item) + 15u) & ~(size_t)15u, bytes = groups_at + (size_t)n_groups * sizeof(tsqa_block_group);
    tsqa_uploads::Slot up;
    if (int rc = c->range_up.acquire(c, bytes ? bytes : 16, &up)) return rc;
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    gate_read(idx, d_status, s);
    if (n_groups == 0) return TSQA_OK;
    memset(up.host<uint8_t>(), 0, bytes);
    std::copy(vi.begin(), vi.end(), up.host<tsqa_range_item>());
    std::copy(vg.begin(), vg.end(), up.host<tsqa_block_group>(groups_at));
    TSQ_HIP(c, up.send(bytes, s));
    ProfSpan span(c, 7, s);
    const int rc = launch_read_kernel<dec_group_kernel>(c, n_groups, s, idx->container, idx->frames, idx->n_blocks, up.dev<RangeItem>(), n_items,
                                                        up.dev<BlockGroup>(groups_at), static_cast<uint8_t*>(d_out), d_status);
    span.end();
    TSQ_HIP(c, up.commit(s));
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_decompress_item_ranges(tsqa_ctx* c, const tsqa_index* idx, const tsqa_item_range* ranges, uint32_t n_ranges, void* d_out,
                                           size_t out_cap, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    int rc = tsqa_decompress_item_ranges_async(c, idx, ranges, n_ranges, d_out, out_cap, c->d_status, s);
    if (rc) return rc;
    return finish_sync(c, s, "decompress_item_ranges");
}

// ---- batches: many independent items at offsets in one input and one output buffer ----

enum BatchPlan { kPlanCompress, kPlanDecompress, kPlanRangesOnly, kPlanPlaced, kPlanPacked };

// tsqa_plan_batch, with the reason for a refusal.  kPlanRangesOnly: the ranges and input lengths of a decompress batch whose block
// counts are not known yet (first_block is not written).  kPlanPlaced: a decompress batch whose containers are placed by tables on
// the device (tsqa_decompress_batch_packed_async): the output ranges and the block counts; in_at and in_len are not looked at.
// kPlanPacked: a compress batch whose output places are made on the device (tsqa_compress_batch_packed_async): kPlanCompress
// without output ranges; out_at and out_cap are not looked at.  block_len: what a compress batch cuts its items into.
static int plan_batch(const tsqa_batch_item* items, uint32_t n_items, size_t in_size, size_t out_size, const uint32_t* n_blocks,
                      uint64_t* first_block, const char** why, BatchPlan mode, uint32_t block_len = kBlockSize)
{
    *why = "";
    if (!items || n_items == 0) { *why = "no items"; return TSQA_ERR_ARG; }
    auto blocks_of = [&](uint32_t i) -> uint64_t {
        return mode == kPlanCompress || mode == kPlanPacked ? items[i].in_len / block_len + (items[i].in_len % block_len != 0)
               : mode == kPlanDecompress || mode == kPlanPlaced ? n_blocks[i] : 0;
    };
    std::vector<std::pair<uint64_t, uint64_t>> dst;
    dst.reserve(n_items);
    uint64_t blocks = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        const tsqa_batch_item& x = items[i];
        const uint64_t nb = blocks_of(i);
        if (mode == kPlanPlaced) {
            if (nb == 0) { *why = "a block count of 0"; return TSQA_ERR_ARG; }
        } else {
            if (x.in_len == 0) { *why = "an item is empty"; return TSQA_ERR_ARG; }
            if (x.in_len > in_size || x.in_at > in_size - x.in_len) { *why = "an input range ends past in_size"; return TSQA_ERR_ARG; }
        }
        if (mode == kPlanPacked) { blocks += nb; continue; }
        if (x.out_cap > out_size || x.out_at > out_size - x.out_cap) { *why = "an output range ends past out_size"; return TSQA_ERR_ARG; }
        if (mode == kPlanCompress && x.out_cap < kHeaderSize + kMinFrameSize * nb) { *why = "an output range holds less than 16 + 6 bytes per block"; return TSQA_ERR_ARG; }
        if ((mode == kPlanDecompress || mode == kPlanRangesOnly) && x.in_len < kHeaderSize) { *why = "an input range is shorter than a header"; return TSQA_ERR_ARG; }
        if (mode == kPlanDecompress && (nb == 0 || nb > (x.in_len - kHeaderSize) / kMinFrameSize)) { *why = "a block count that the container cannot hold"; return TSQA_ERR_ARG; }
        if (x.out_cap) dst.emplace_back(x.out_at, x.out_cap);
        blocks += nb;
    }
    if (destinations_overlap(dst)) { *why = "two output ranges overlap"; return TSQA_ERR_ARG; }          // (input ranges may)
    if (blocks > 0xFFFFFFFFull) { *why = "more than 2^32 - 1 blocks"; return TSQA_ERR_ARG; }
    if (mode == kPlanRangesOnly) return TSQA_OK;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_items; ++i) { first_block[i] = at; at += blocks_of(i); }
    first_block[n_items] = at;
    return TSQA_OK;
}

extern "C" int tsqa_plan_batch(const tsqa_batch_item* items, uint32_t n_items, size_t in_size, size_t out_size, const uint32_t* n_blocks,
                               uint64_t* first_block)
{
    const char* why;
    if (!first_block) return TSQA_ERR_ARG;
    return plan_batch(items, n_items, in_size, out_size, n_blocks, first_block, &why, n_blocks ? kPlanDecompress : kPlanCompress);
}

// The batch route: n_blocks blocks, each encoded from its descriptor into slot b % budget, in launches of at most `budget` = 2 x n_cus
// blocks, the lean layout's chip-filling count, so that the scratch -- a slot and a position table per block -- stays bounded whatever
// the count.  Items may span launches.  Its callers reserve min(n_blocks, budget) blocks with tables and slots for all streams.
static uint32_t batch_budget(const tsqa_ctx* c) { return 2u * (uint32_t)c->n_cus; }

// The launches of the batch route, in turn: the encode of blocks [b0, b0 + nb) (a kind-0 span), scan(b0, nb, launch) -- the caller's
// pack scan, which places the launch's frames in c->frame_at --, the copy of the streams to `out` in `pieces` pieces each.  live !=
// NULL: descriptors made on the device, of which *live are in use (launch_batch_encode_kernels); launches past them do nothing.
// Ends at an encode launch that is refused, with its error.
template <class Scan>
static int batch_route_enqueue(tsqa_ctx* c, const uint8_t* in, const EncBatchBlock* blocks, uint64_t n_blocks, uint32_t ext, uint32_t pieces,
                               uint8_t* out, const uint32_t* live, int32_t* d_status, hipStream_t s, Scan scan)
{
    const uint32_t budget = batch_budget(c);
    uint32_t launch = 0;
    for (uint64_t b0 = 0; b0 < n_blocks; b0 += budget, ++launch) {
        const uint32_t nb = (uint32_t)(n_blocks - b0 < budget ? n_blocks - b0 : budget), first = live ? (uint32_t)b0 : 0u;
        ProfSpan span(c, 0, s);
        const int rc = launch_batch_encode_kernels(c, in, blocks + b0, nb, ext, c->slots, c->sizes, d_status, s, first, live);
        if (rc) { span.cancel(); return rc; }
        span.end();
        scan(b0, nb, launch);
        hipLaunchKernelGGL(batch_pack_copy_kernel, dim3(pieces, nb), dim3(256), 0, s, c->slots, c->sizes, c->frame_at, out, first, live);
    }
    return TSQA_OK;
}

// The items with blocks in the launch of blocks [b0, b0 + nb) of a batch planned on the host (first[]: its block plan, no item
// without blocks): from *i0, the one that holds block b0, to the last that starts before b0 + nb.  Returns their count.
static uint32_t launch_items(const std::vector<uint64_t>& first, uint32_t n_items, uint64_t b0, uint32_t nb, uint32_t* i0)
{
    *i0 = (uint32_t)(std::upper_bound(first.begin(), first.end(), b0) - first.begin()) - 1u;
    return (uint32_t)(std::lower_bound(first.begin(), first.begin() + n_items, b0 + nb) - first.begin()) - *i0;
}

// The launches of tsqa_compress_batch_async, whose arguments have been checked; first[] is its block plan (tsqa_plan_batch).  The
// frames go into the caller's output ranges.
static int compress_batch_enqueue(tsqa_ctx* c, const void* d_in, const tsqa_batch_item* items, uint32_t n_items, const std::vector<uint64_t>& first,
                                  uint32_t ext, void* d_out, uint64_t* d_sizes, int32_t* d_status, hipStream_t s)
{
    static_assert(sizeof(tsqa_batch_item) == 32 && sizeof(BatchItem) == 48 && sizeof(EncBatchBlock) == 24, "descriptor layouts");
    (void)hipSetDevice(c->device);
    const uint64_t n_blocks = first[n_items];
    const uint32_t budget = batch_budget(c);
    const size_t item_bytes = (size_t)n_items * sizeof(BatchItem), bytes = item_bytes + n_blocks * sizeof(EncBatchBlock);
    tsqa_uploads::Slot up;
    if (int rc = c->batch_up.acquire(c, bytes, &up)) return rc;
    if (int rc = c->reserve(n_blocks < budget ? n_blocks : budget, true, true, true)) return rc;
    if (int rc = c->reserve_batch(n_items)) return rc;
    BatchItem* const hi = up.host<BatchItem>();
    EncBatchBlock* const hb = up.host<EncBatchBlock>(item_bytes);
    for (uint32_t i = 0; i < n_items; ++i) {
        const tsqa_batch_item& x = items[i];
        const uint32_t nb = (uint32_t)(first[i + 1] - first[i]);
        hi[i] = BatchItem{x.in_at, x.in_len, x.out_at, x.out_cap, first[i], nb, 0u};
        for (uint32_t j = 0; j < nb; ++j) {
            const uint64_t b = first[i] + j, off = (uint64_t)j * kBlockSize, left = x.in_len - off;
            hb[b] = EncBatchBlock{x.in_at + off, left, left < kBlockSize ? (uint32_t)left : kBlockSize, (uint32_t)(b % budget)};
        }
    }
    const BatchItem* const di = up.dev<BatchItem>();
    const EncBatchBlock* const db = up.dev<EncBatchBlock>(item_bytes);
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    uint8_t* const out = static_cast<uint8_t*>(d_out);
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    TSQ_HIP(c, up.send(bytes, s));
    const int rc = batch_route_enqueue(c, in, db, n_blocks, ext, pack_pieces(), out, nullptr, d_status, s, [&](uint64_t b0, uint32_t nb, uint32_t) {
        uint32_t i0;
        const uint32_t ni = launch_items(first, n_items, b0, nb, &i0);
        hipLaunchKernelGGL(batch_pack_scan_kernel, dim3((ni + 255u) / 256u), dim3(256), 0, s, di, i0, ni, b0, nb, c->sizes, ext, out, c->batch_at,
                           c->frame_at, d_sizes, d_status);
    });
    TSQ_HIP(c, up.commit(s));                            // (behind a refused launch too: those before it may still read the descriptors)
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

static bool batch_encoder_ok(tsqa_ctx* c, const char* who)
{
    const int v = c->enc_variant;
    if (v == 0 || v == 6 || v == 7) return true;
    c->set_error("%s: encoder variant %d does not take batches (0, 6 and 7 do)", who, v);
    return false;
}

extern "C" int tsqa_compress_batch_async(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items,
                                         uint32_t ext, void* d_out, size_t out_size, uint64_t* d_sizes, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_in || !d_out || !d_sizes || !d_status) { c->set_error("compress_batch: null pointer"); return TSQA_ERR_ARG; }
    if (!batch_encoder_ok(c, "compress_batch")) return TSQA_ERR_ARG;
    std::vector<uint64_t> first((size_t)n_items + 1);
    const char* why;
    if (plan_batch(items, n_items, in_size, out_size, nullptr, first.data(), &why, kPlanCompress)) { c->set_error("compress_batch: %s", why); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    return compress_batch_enqueue(c, d_in, items, n_items, first, ext, d_out, d_sizes, d_status, s);
}

extern "C" int tsqa_compress_batch(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items, uint32_t ext,
                                   void* d_out, size_t out_size, uint64_t* sizes, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!sizes) { c->set_error("compress_batch: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    if (int rc = c->reserve_batch(n_items)) return rc;
    int rc = tsqa_compress_batch_async(c, d_in, in_size, items, n_items, ext, d_out, out_size, c->batch_sizes, c->d_status, s);
    if (rc) return rc;
    TSQ_HIP(c, hipMemcpyAsync(sizes, c->batch_sizes, (size_t)n_items * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    return finish_sync(c, s, "compress_batch");
}

// ---- packed batches: the items' containers one after the other in a dense arena, their places made on the device ----

extern "C" size_t tsqa_batch_bound(size_t n) { return (size_t)batch_bound(n); }

static bool packed_align_ok(uint32_t align) { return align >= 1 && align <= 4096 && (align & (align - 1)) == 0; }

extern "C" int tsqa_plan_packed(const uint64_t* sizes, uint32_t n_items, uint32_t align, uint64_t* offsets)
{
    if (!sizes || !offsets || n_items == 0 || !packed_align_ok(align)) return TSQA_ERR_ARG;
    const uint64_t mask = (uint64_t)align - 1;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        offsets[i] = at;
        at += sizes[i];
        if (i + 1 < n_items) at = (at + mask) & ~mask;
    }
    offsets[n_items] = at;
    return TSQA_OK;
}

// ---- the host-planned packed compress: every item cut every block_len bytes, TSQ_BLOCK_SZ or the caller's shorter one ----

static bool split_block_len_ok(uint32_t block_len) { return block_len >= 4096u && block_len <= kBlockSize && (block_len & (block_len - 1u)) == 0u; }
static uint32_t log2_of(uint32_t pow2) { uint32_t k = 0; while ((1u << k) < pow2) ++k; return k; }

extern "C" int tsqa_plan_batch_split(const tsqa_batch_item* items, uint32_t n_items, size_t in_size, uint32_t block_len, uint32_t align,
                                     uint64_t* first_block, uint64_t* bound)
{
    const char* why;
    if (!first_block || !bound || !split_block_len_ok(block_len) || !packed_align_ok(align)) return TSQA_ERR_ARG;
    if (int rc = plan_batch(items, n_items, in_size, 0, nullptr, first_block, &why, kPlanPacked, block_len)) return rc;
    const uint64_t mask = (uint64_t)align - 1;
    uint64_t room = 0;
    for (uint32_t i = 0; i < n_items; ++i) room += (split_bound(items[i].in_len, block_len) + mask) & ~mask;
    *bound = room;
    return TSQA_OK;
}

// Every host-planned packed compress (`who`: the caller, for the error texts; block_len: kBlockSize for tsqa_compress_batch_packed*,
// which cannot fail its check): the argument checks, then the launches.  Nothing is reserved, enqueued or written before the checks
// pass.  d_offsets, d_sizes: the caller's device tables, or NULL for the context's own (the waiting forms).  Only the item table,
// first_block and the block count are uploaded: the block descriptors and each block's item are made on the device
// (batch_enc_blocks_kernel), as the compress from device tables makes them.
static int compress_batch_packed_split_enqueue(tsqa_ctx* c, const char* who, const void* d_in, size_t in_size, const tsqa_batch_item* items,
                                               uint32_t n_items, uint32_t ext, uint32_t align, uint32_t block_len, void* d_out, size_t out_size,
                                               uint64_t* d_offsets, uint64_t* d_sizes, uint32_t* d_block_sizes, int32_t* d_status, hipStream_t s)
{
    if (!d_in || !d_out || !d_status || !items) { c->set_error("%s: null pointer", who); return TSQA_ERR_ARG; }
    if (!batch_encoder_ok(c, who)) return TSQA_ERR_ARG;
    if (!packed_align_ok(align)) { c->set_error("%s: align %u is not a power of two from 1 to 4096", who, align); return TSQA_ERR_ARG; }
    if (!split_block_len_ok(block_len)) { c->set_error("%s: block_len %u is not a power of two from 2^12 to 2^22", who, block_len); return TSQA_ERR_ARG; }
    if (out_size < kHeaderSize) { c->set_error("%s: out_size holds less than a header", who); return TSQA_ERR_ARG; }
    if (n_items == 0) { c->set_error("%s: no items", who); return TSQA_ERR_ARG; }
    std::vector<uint64_t> first((size_t)n_items + 1);
    const char* why;
    if (plan_batch(items, n_items, in_size, out_size, nullptr, first.data(), &why, kPlanPacked, block_len)) { c->set_error("%s: %s", who, why); return TSQA_ERR_ARG; }
    (void)hipSetDevice(c->device);
    const uint64_t n_blocks = first[n_items];
    const uint32_t budget = batch_budget(c);
    if (budget > kPackScanBlocks) { c->set_error("%s: %u blocks per launch, the pack scan takes %u", who, budget, kPackScanBlocks); return TSQA_ERR_HIP; }
    const size_t item_bytes = (size_t)n_items * sizeof(BatchItem), first_bytes = ((size_t)n_items + 1) * sizeof(uint64_t);
    const size_t bytes = item_bytes + first_bytes + sizeof(uint32_t);
    tsqa_uploads::Slot up;
    if (int rc = c->batch_up.acquire(c, bytes, &up)) return rc;
    if (int rc = c->reserve(n_blocks < budget ? n_blocks : budget, true, true, true)) return rc;
    if (int rc = c->reserve_batch(n_items)) return rc;
    if (int rc = c->reserve_tables(n_blocks, (n_blocks + budget - 1) / budget, true)) return rc;
    if (!d_offsets) { d_offsets = c->batch_offsets; d_sizes = c->batch_sizes; }
    BatchItem* const hi = up.host<BatchItem>();
    for (uint32_t i = 0; i < n_items; ++i) hi[i] = BatchItem{items[i].in_at, items[i].in_len, 0, 0, first[i], (uint32_t)(first[i + 1] - first[i]), 0u};
    memcpy(up.host<uint8_t>(item_bytes), first.data(), first_bytes);
    *up.host<uint32_t>(item_bytes + first_bytes) = (uint32_t)n_blocks;
    const BatchItem* const di = up.dev<BatchItem>();
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    uint8_t* const out = static_cast<uint8_t*>(d_out);
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    TSQ_HIP(c, up.send(bytes, s));
    hipLaunchKernelGGL(batch_enc_blocks_kernel, dim3((uint32_t)((n_blocks + 255u) / 256u)), dim3(256), 0, s, di, n_items,
                       static_cast<const uint64_t*>(up.dev<uint64_t>(item_bytes)), static_cast<const uint32_t*>(up.dev<uint32_t>(item_bytes + first_bytes)),
                       budget, block_len, c->table_blocks, c->table_launch_item, c->table_block_item);
    // (no stream of these blocks is longer than block_bound says: short blocks need few copy pieces, full ones a slot's: kSlotSize)
    const uint32_t max_stream = (uint32_t)(block_bound(block_len) - kFrameWordSize);
    const int rc = batch_route_enqueue(c, in, c->table_blocks, n_blocks, ext, pack_pieces(max_stream), out, nullptr, d_status, s, [&](uint64_t b0, uint32_t nb, uint32_t) {
        uint32_t i0;
        const uint32_t ni = launch_items(first, n_items, b0, nb, &i0);
        hipLaunchKernelGGL(batch_pack_scan_packed_kernel, dim3(1), dim3(256), 0, s, di, n_items, i0, ni, b0, nb, static_cast<const uint32_t*>(c->sizes),
                           static_cast<const uint32_t*>(c->table_block_item), ext, align, max_stream, out, (uint64_t)out_size, c->batch_at, c->frame_at,
                           d_offsets, d_sizes, d_block_sizes, d_status);
    });
    TSQ_HIP(c, up.commit(s));                            // (behind a refused launch too: those before it may still read the tables)
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

// The waiting tail of the packed calls: the context's own offsets (n_items + 1) and sizes (n_items) back to the host.
static int finish_packed_sync(tsqa_ctx* c, hipStream_t s, const char* what, uint32_t n_items, uint64_t* offsets, uint64_t* sizes)
{
    TSQ_HIP(c, hipMemcpyAsync(offsets, c->batch_offsets, ((size_t)n_items + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipMemcpyAsync(sizes, c->batch_sizes, (size_t)n_items * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    return finish_sync(c, s, what);
}

extern "C" int tsqa_compress_batch_packed_async(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items,
                                                uint32_t ext, uint32_t align, void* d_out, size_t out_size, uint64_t* d_offsets,
                                                uint64_t* d_sizes, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_offsets || !d_sizes) { c->set_error("compress_batch_packed: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    return compress_batch_packed_split_enqueue(c, "compress_batch_packed", d_in, in_size, items, n_items, ext, align, kBlockSize, d_out, out_size,
                                               d_offsets, d_sizes, nullptr, d_status, s);
}

extern "C" int tsqa_compress_batch_packed(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items,
                                          uint32_t ext, uint32_t align, void* d_out, size_t out_size, uint64_t* offsets, uint64_t* sizes,
                                          void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!offsets || !sizes) { c->set_error("compress_batch_packed: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    int rc = compress_batch_packed_split_enqueue(c, "compress_batch_packed", d_in, in_size, items, n_items, ext, align, kBlockSize, d_out, out_size,
                                                 nullptr, nullptr, nullptr, c->d_status, s);
    if (rc) return rc;
    return finish_packed_sync(c, s, "compress_batch_packed", n_items, offsets, sizes);
}

extern "C" int tsqa_compress_batch_packed_split_async(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items,
                                                      uint32_t ext, uint32_t align, uint32_t block_len, void* d_out, size_t out_size,
                                                      uint64_t* d_offsets, uint64_t* d_sizes, uint32_t* d_block_sizes, int32_t* d_status,
                                                      void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_offsets || !d_sizes) { c->set_error("compress_batch_packed_split: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    return compress_batch_packed_split_enqueue(c, "compress_batch_packed_split", d_in, in_size, items, n_items, ext, align, block_len, d_out,
                                               out_size, d_offsets, d_sizes, d_block_sizes, d_status, s);
}

extern "C" int tsqa_compress_batch_packed_split(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items,
                                                uint32_t ext, uint32_t align, uint32_t block_len, void* d_out, size_t out_size, uint64_t* offsets,
                                                uint64_t* sizes, uint32_t* d_block_sizes, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!offsets || !sizes) { c->set_error("compress_batch_packed_split: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    int rc = compress_batch_packed_split_enqueue(c, "compress_batch_packed_split", d_in, in_size, items, n_items, ext, align, block_len, d_out,
                                                 out_size, nullptr, nullptr, d_block_sizes, c->d_status, s);
    if (rc) return rc;
    return finish_packed_sync(c, s, "compress_batch_packed_split", n_items, offsets, sizes);
}

// ---- packed compress whose item table is made on the device from tables in device memory ----

constexpr uint64_t kTablesInMax = 1ull << 48;    // in_size above this is refused: the block sums then stay below 2^59

// tsqa_plan_compress_tables and its split form: the items cut every block_len bytes.
static int plan_compress_tables(const uint64_t* in_offsets, const uint64_t* in_sizes, uint32_t n_items, uint64_t in_size, uint32_t block_len,
                                uint32_t align, uint32_t cap_blocks, uint64_t* first_block, int32_t* item_status, uint64_t* bound, uint32_t* n_fit)
{
    if (!in_offsets || !in_sizes || !first_block || !item_status || !bound || !n_fit || n_items == 0 || !packed_align_ok(align) ||
        in_size > kTablesInMax) return TSQA_ERR_ARG;
    const uint64_t mask = (uint64_t)align - 1;
    uint64_t fb = 0, room = 0;
    uint32_t fit = n_items;
    for (uint32_t i = 0; i < n_items; ++i) {
        const uint64_t at = in_offsets[i], n = in_sizes[i];
        const uint64_t blocks = n / block_len + (n % block_len != 0);
        const bool ok = n >= 1 && n <= in_size && at <= in_size - n && blocks <= 0xFFFFFFFFull;
        const uint64_t nb = ok ? blocks : 0;
        first_block[i] = fb;
        if (ok && fit == n_items && fb + nb > cap_blocks) fit = i;           // (the first unfit item ends the prefix)
        item_status[i] = !ok ? TSQA_ERR_ARG : i >= fit ? TSQA_ERR_OVERFLOW : TSQA_OK;
        fb += nb;
        if (ok) room += (split_bound(n, block_len) + mask) & ~mask;
    }
    first_block[n_items] = fb;
    *bound = room;
    *n_fit = fit;
    return TSQA_OK;
}

extern "C" int tsqa_plan_compress_tables(const uint64_t* in_offsets, const uint64_t* in_sizes, uint32_t n_items, uint64_t in_size,
                                         uint32_t align, uint32_t cap_blocks, uint64_t* first_block, int32_t* item_status, uint64_t* bound,
                                         uint32_t* n_fit)
{
    return plan_compress_tables(in_offsets, in_sizes, n_items, in_size, kBlockSize, align, cap_blocks, first_block, item_status, bound, n_fit);
}

extern "C" int tsqa_plan_compress_tables_split(const uint64_t* in_offsets, const uint64_t* in_sizes, uint32_t n_items, uint64_t in_size,
                                               uint32_t block_len, uint32_t align, uint32_t cap_blocks, uint64_t* first_block,
                                               int32_t* item_status, uint64_t* bound, uint32_t* n_fit)
{
    if (!split_block_len_ok(block_len)) return TSQA_ERR_ARG;
    return plan_compress_tables(in_offsets, in_sizes, n_items, in_size, block_len, align, cap_blocks, first_block, item_status, bound, n_fit);
}

// tsqa_compress_batch_packed_tables_async (block_len == 0: blocks of TSQ_BLOCK_SZ, no size table) and its split form.
static int compress_tables_enqueue(tsqa_ctx* c, const char* who, const void* d_in, size_t in_size, const uint64_t* d_in_offsets,
                                   const uint64_t* d_in_sizes, uint32_t n_items, uint32_t cap_blocks, uint32_t ext, uint32_t align,
                                   uint32_t block_len, void* d_out, size_t out_size, uint64_t* d_offsets, uint64_t* d_sizes,
                                   uint64_t* d_first_block, uint64_t* d_bound, uint32_t* d_block_sizes, int32_t* d_item_status,
                                   int32_t* d_status, void* hip_stream)
{
    const bool split = block_len != 0u;
    if (!split) block_len = kBlockSize;
    if (!d_in || !d_in_offsets || !d_in_sizes || !d_offsets || !d_sizes || !d_first_block || !d_item_status || !d_status) {
        c->set_error("%s: null pointer", who);
        return TSQA_ERR_ARG;
    }
    if (n_items == 0) { c->set_error("%s: no items", who); return TSQA_ERR_ARG; }
    if (!packed_align_ok(align)) { c->set_error("%s: align %u is not a power of two from 1 to 4096", who, align); return TSQA_ERR_ARG; }
    if ((uint64_t)in_size > kTablesInMax) { c->set_error("%s: in_size above 2^48", who); return TSQA_ERR_ARG; }
    if (d_out ? (out_size < kHeaderSize || cap_blocks == 0) : out_size != 0) {
        c->set_error("%s: an arena needs out_size >= 16 and cap_blocks above 0; measuring takes d_out NULL and out_size 0", who);
        return TSQA_ERR_ARG;
    }
    if (split && !split_block_len_ok(block_len)) { c->set_error("%s: block_len %u is not a power of two from 2^12 to 2^22", who, block_len); return TSQA_ERR_ARG; }
    if (!batch_encoder_ok(c, who)) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    const uint32_t budget = batch_budget(c);             // (the launches are sized by cap_blocks, not by a planned count)
    if (budget > kPackScanBlocks) { c->set_error("%s: %u blocks per launch, the pack scan takes %u", who, budget, kPackScanBlocks); return TSQA_ERR_HIP; }
    if (int rc = c->reserve_batch(n_items)) return rc;
    if (d_out) {
        if (int rc = c->reserve(cap_blocks < budget ? cap_blocks : budget, true, true, true)) return rc;
        if (int rc = c->reserve_tables(cap_blocks, ((size_t)cap_blocks + budget - 1) / budget, true)) return rc;
    }
    const dim3 per_item((uint32_t)(((uint64_t)n_items + 255u) / 256u));
    const uint32_t block_shift = log2_of(block_len);
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(batch_measure_tables_kernel, per_item, dim3(256), 0, s, c->batch_items, n_items, d_in_offsets, d_in_sizes,
                       (uint64_t)in_size, block_shift, d_item_status);
    // (measuring: nothing fits, and the kernel writes the two arena tables itself)
    hipLaunchKernelGGL(batch_layout_tables_kernel, dim3(1), dim3(256), 0, s, c->batch_items, n_items, align, block_shift, d_out ? cap_blocks : 0u,
                       d_out ? (uint64_t*)nullptr : d_offsets, d_sizes, d_first_block, d_bound, d_item_status, c->batch_live, d_status);
    if (!d_out) { TSQ_HIP(c, hipGetLastError()); return TSQA_OK; }
    const BatchItem* const di = c->batch_items;
    const uint32_t* const live = c->batch_live;
    hipLaunchKernelGGL(batch_enc_blocks_kernel, dim3((uint32_t)(((uint64_t)cap_blocks + 255u) / 256u)), dim3(256), 0, s, di, n_items,
                       static_cast<const uint64_t*>(d_first_block), live, budget, block_len, c->table_blocks, c->table_launch_item,
                       c->table_block_item);
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    uint8_t* const out = static_cast<uint8_t*>(d_out);
    // (no stream is longer than block_bound says: short blocks need few copy pieces, full ones a slot's: kSlotSize)
    const uint32_t max_stream = (uint32_t)(block_bound(block_len) - kFrameWordSize);
    const int rc = batch_route_enqueue(c, in, c->table_blocks, cap_blocks, ext, pack_pieces(max_stream), out, live, d_status, s, [&](uint64_t, uint32_t, uint32_t launch) {
        hipLaunchKernelGGL(batch_pack_scan_tables_kernel, dim3(1), dim3(256), 0, s, di, n_items, static_cast<const uint32_t*>(c->table_launch_item),
                           launch, budget, live, static_cast<const uint32_t*>(c->sizes), static_cast<const uint32_t*>(c->table_block_item), ext,
                           align, max_stream, out, (uint64_t)out_size, c->batch_at, c->frame_at, d_offsets, d_sizes, d_block_sizes, d_item_status,
                           d_status);
    });
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_compress_batch_packed_tables_async(tsqa_ctx* c, const void* d_in, size_t in_size, const uint64_t* d_in_offsets,
                                                       const uint64_t* d_in_sizes, uint32_t n_items, uint32_t cap_blocks, uint32_t ext,
                                                       uint32_t align, void* d_out, size_t out_size, uint64_t* d_offsets, uint64_t* d_sizes,
                                                       uint64_t* d_first_block, uint64_t* d_bound, int32_t* d_item_status, int32_t* d_status,
                                                       void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    return compress_tables_enqueue(c, "compress_batch_packed_tables", d_in, in_size, d_in_offsets, d_in_sizes, n_items, cap_blocks, ext, align, 0u,
                                   d_out, out_size, d_offsets, d_sizes, d_first_block, d_bound, nullptr, d_item_status, d_status, hip_stream);
}

extern "C" int tsqa_compress_batch_packed_tables_split_async(tsqa_ctx* c, const void* d_in, size_t in_size, const uint64_t* d_in_offsets,
                                                             const uint64_t* d_in_sizes, uint32_t n_items, uint32_t cap_blocks, uint32_t ext,
                                                             uint32_t align, uint32_t block_len, void* d_out, size_t out_size,
                                                             uint64_t* d_offsets, uint64_t* d_sizes, uint64_t* d_first_block, uint64_t* d_bound,
                                                             uint32_t* d_block_sizes, int32_t* d_item_status, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (block_len == 0u) { c->set_error("compress_batch_packed_tables_split: block_len 0"); return TSQA_ERR_ARG; }
    return compress_tables_enqueue(c, "compress_batch_packed_tables_split", d_in, in_size, d_in_offsets, d_in_sizes, n_items, cap_blocks, ext, align,
                                   block_len, d_out, out_size, d_offsets, d_sizes, d_first_block, d_bound, d_block_sizes, d_item_status, d_status,
                                   hip_stream);
}

// ---- one container of short blocks: the input cut every block_len bytes, encoded by the batch route ----

extern "C" int tsqa_plan_split(size_t n, uint32_t block_len, uint32_t* n_blocks, size_t* bound)
{
    if (!n_blocks || !bound || n == 0 || !split_block_len_ok(block_len)) return TSQA_ERR_ARG;
    const uint64_t nb = (uint64_t)n / block_len + ((uint64_t)n % block_len != 0);
    if (nb > 0xFFFFFFFFull) return TSQA_ERR_ARG;
    *n_blocks = (uint32_t)nb;
    *bound = (size_t)split_bound(n, block_len);
    return TSQA_OK;
}

extern "C" int tsqa_compress_device_split_async(tsqa_ctx* c, const void* d_in, size_t n, uint32_t block_len, void* d_out, size_t out_cap,
                                                uint64_t* d_out_size, uint32_t* d_block_sizes, int32_t* d_status, uint32_t ext, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    uint32_t n_blocks = 0;
    size_t bound = 0;
    if (tsqa_plan_split(n, block_len, &n_blocks, &bound)) {
        c->set_error("compress_split: no input, a block_len that is no power of two from 2^12 to 2^22, or more than 2^32 - 1 blocks");
        return TSQA_ERR_ARG;
    }
    if (!d_in || !d_out || !d_out_size || !d_status) { c->set_error("compress_split: null pointer"); return TSQA_ERR_ARG; }
    if (out_cap < kHeaderSize + (uint64_t)kMinFrameSize * n_blocks) { c->set_error("compress_split: output capacity too small"); return TSQA_ERR_ARG; }
    if (!batch_encoder_ok(c, "compress_split")) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    const uint32_t budget = batch_budget(c);             // (the descriptors are made on the device, and nothing is uploaded)
    if (int rc = c->reserve(n_blocks < budget ? n_blocks : budget, true, true, true)) return rc;
    if (int rc = c->reserve_batch(1)) return rc;         // (batch_at[0]: the running frame offset between the launches)
    if (int rc = c->reserve_tables(n_blocks, 0)) return rc;
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    uint8_t* const out = static_cast<uint8_t*>(d_out);
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(split_blocks_kernel, dim3((uint32_t)(((uint64_t)n_blocks + 255u) / 256u)), dim3(256), 0, s, (uint64_t)n, block_len, n_blocks,
                       budget, c->table_blocks);
    // (no stream of these blocks is longer than block_bound says: short blocks need few copy pieces)
    const uint32_t max_stream = (uint32_t)(block_bound(block_len) - kFrameWordSize);
    const int rc = batch_route_enqueue(c, in, c->table_blocks, n_blocks, ext, pack_pieces(max_stream), out, nullptr, d_status, s, [&](uint64_t b0, uint32_t nb, uint32_t) {
        hipLaunchKernelGGL(split_pack_scan_kernel, dim3(1), dim3(256), 0, s, static_cast<const uint32_t*>(c->sizes), (uint32_t)b0, nb, n_blocks,
                           (uint64_t)n, ext, max_stream, out, (uint64_t)out_cap, c->batch_at, c->frame_at, d_out_size, d_block_sizes, d_status);
    });
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_compress_device_split(tsqa_ctx* c, const void* d_in, size_t n, uint32_t block_len, void* d_out, size_t out_cap,
                                          size_t* out_size, uint32_t* d_block_sizes, uint32_t ext, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!out_size) { c->set_error("compress_split: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    int rc = tsqa_compress_device_split_async(c, d_in, n, block_len, d_out, out_cap, c->d_size, d_block_sizes, c->d_status, ext, s);
    if (rc) return rc;
    return finish_sync(c, s, "compress_split", out_size);            // (the size needed, behind TSQA_ERR_OVERFLOW too)
}

// What every batch decompress with host-planned items starts with (`who`: the caller, for the error texts): the plan, an upload slot
// with the items, the scratch, zeroed status words (d_item_status may be NULL) and, for a packed batch (d_offsets != NULL), the items'
// places, which batch_place_kernel reads from d_offsets and d_packed_sizes (items' in_at, in_len unused).  The caller launches what
// reads up->dev<BatchItem>() and commits the slot behind it, however those launches went.
static int stage_decompress_batch(tsqa_ctx* c, const char* who, size_t in_size, const tsqa_batch_item* items, const uint32_t* n_blocks,
                                  uint32_t n_items, size_t out_size, int32_t* d_item_status, int32_t* d_status, hipStream_t s,
                                  const uint64_t* d_offsets, const uint64_t* d_packed_sizes, tsqa_uploads::Slot* up, uint32_t* total_blocks)
{
    std::vector<uint64_t> first((size_t)n_items + 1);
    const char* why;
    if (plan_batch(items, n_items, in_size, out_size, n_blocks, first.data(), &why, d_offsets ? kPlanPlaced : kPlanDecompress)) {
        c->set_error("%s: %s", who, why);
        return TSQA_ERR_ARG;
    }
    (void)hipSetDevice(c->device);
    *total_blocks = (uint32_t)first[n_items];
    if (int rc = c->batch_up.acquire(c, (size_t)n_items * sizeof(BatchItem), up)) return rc;
    if (int rc = c->reserve(*total_blocks, false, false, true)) return rc;
    c->forget_sharded();                                 // the frame walk behind this overwrites c->frames
    BatchItem* const hi = up->host<BatchItem>();
    for (uint32_t i = 0; i < n_items; ++i)
        hi[i] = BatchItem{items[i].in_at, items[i].in_len, items[i].out_at, items[i].out_cap, first[i], n_blocks[i], 0u};
    if (d_item_status) TSQ_HIP(c, hipMemsetAsync(d_item_status, 0, (size_t)n_items * sizeof(int32_t), s));
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    TSQ_HIP(c, up->send((size_t)n_items * sizeof(BatchItem), s));
    if (d_offsets)                       // (the one kernel that writes a slot's device copy: the items' places)
        hipLaunchKernelGGL(batch_place_kernel, dim3((n_items + 255u) / 256u), dim3(256), 0, s, up->dev<BatchItem>(), n_items,
                           d_offsets, d_packed_sizes, (uint64_t)in_size);
    return TSQA_OK;
}

// (variant < 0: the context's decode variant; the synchronous form's retry after TSQA_ERR_STALL passes 4.  d_offsets != NULL: a
//  packed batch)
static int decompress_batch_async_impl(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, const uint32_t* n_blocks,
                                       uint32_t n_items, void* d_out, size_t out_size, uint64_t* d_sizes, int32_t* d_status, hipStream_t s,
                                       int variant, const uint64_t* d_offsets = nullptr, const uint64_t* d_packed_sizes = nullptr)
{
    if (!d_in || !d_out || !d_sizes || !d_status || !n_blocks) { c->set_error("decompress_batch: null pointer"); return TSQA_ERR_ARG; }
    tsqa_uploads::Slot up;
    uint32_t total_blocks;
    if (int rc = stage_decompress_batch(c, "decompress_batch", in_size, items, n_blocks, n_items, out_size, nullptr, d_status, s, d_offsets,
                                        d_packed_sizes, &up, &total_blocks)) return rc;
    hipLaunchKernelGGL(batch_walk_kernel<kWalkOneWord>, dim3((n_items + 255u) / 256u), dim3(256), 0, s, static_cast<const uint8_t*>(d_in),
                       up.dev<BatchItem>(), n_items, c->frames, (uint32_t*)nullptr, d_sizes, d_status);
    // one decode over every frame of the batch (launch_decode_kernels picks the decoder by the block count, as for one container)
    const int rc = c->launch_decode_frames(d_in, c->frames, total_blocks, d_out, d_status, s, variant);
    TSQ_HIP(c, up.commit(s));
    return rc;
}

extern "C" int tsqa_decompress_batch_async(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, const uint32_t* n_blocks,
                                           uint32_t n_items, void* d_out, size_t out_size, uint64_t* d_sizes, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    return decompress_batch_async_impl(c, d_in, in_size, items, n_blocks, n_items, d_out, out_size, d_sizes, d_status, s, -1);
}

extern "C" int tsqa_decompress_batch_packed_async(tsqa_ctx* c, const void* d_arena, size_t arena_size, const uint64_t* d_offsets,
                                                  const uint64_t* d_sizes, const tsqa_batch_item* items, const uint32_t* n_blocks,
                                                  uint32_t n_items, void* d_out, size_t out_size, uint64_t* d_out_sizes, int32_t* d_status,
                                                  void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_offsets || !d_sizes) { c->set_error("decompress_batch_packed: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    return decompress_batch_async_impl(c, d_arena, arena_size, items, n_blocks, n_items, d_out, out_size, d_out_sizes, d_status, s, -1, d_offsets,
                                       d_sizes);
}

// The decode with a verdict per item, behind a table of n_items items in device memory: batch_walk_kernel with owners, one
// dec_item_kernel workgroup per block whatever the context's decode variant (it waits for nobody: no TSQA_ERR_STALL) -- n_groups
// of them; live_blocks as dec_item_kernel takes it --, batch_close_items_kernel.  The walk and the close are enqueued however the
// decode launch went, and a caller with an upload slot commits it behind this call whatever it returns (a refused decode launch
// returns before hipGetLastError is asked).
static int decode_items_enqueue(tsqa_ctx* c, const uint8_t* in, const BatchItem* d_items, uint32_t n_items, uint32_t n_groups,
                                const uint32_t* live_blocks, void* d_out, uint64_t* d_sizes, int32_t* d_item_status, int32_t* d_status, hipStream_t s)
{
    const dim3 per_item((uint32_t)(((uint64_t)n_items + 255u) / 256u));
    hipLaunchKernelGGL(batch_walk_kernel<kWalkPerItem>, per_item, dim3(256), 0, s, in, d_items, n_items, c->frames, c->block_owner, d_sizes,
                       d_item_status);
    ProfSpan span(c, 1, s);
    const int rc = launch_read_kernel<dec_item_kernel>(c, n_groups, s, in, static_cast<const FrameInfo*>(c->frames),
                                                       static_cast<const uint32_t*>(c->block_owner), static_cast<uint8_t*>(d_out), d_item_status,
                                                       live_blocks);
    if (rc) span.cancel(); else span.end();
    hipLaunchKernelGGL(batch_close_items_kernel, per_item, dim3(256), 0, s, n_items, static_cast<const int32_t*>(d_item_status), d_sizes, d_status);
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

// The batch decompress with a verdict per item (tsqa_decompress_batch_items_async; d_offsets != NULL: the packed form).
static int decompress_batch_items_async_impl(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, const uint32_t* n_blocks,
                                             uint32_t n_items, void* d_out, size_t out_size, uint64_t* d_sizes, int32_t* d_item_status,
                                             int32_t* d_status, hipStream_t s, const uint64_t* d_offsets = nullptr,
                                             const uint64_t* d_packed_sizes = nullptr)
{
    if (!d_in || !d_out || !d_sizes || !d_item_status || !d_status || !n_blocks) { c->set_error("decompress_batch_items: null pointer"); return TSQA_ERR_ARG; }
    tsqa_uploads::Slot up;
    uint32_t total_blocks;
    if (int rc = stage_decompress_batch(c, "decompress_batch_items", in_size, items, n_blocks, n_items, out_size, d_item_status, d_status, s,
                                        d_offsets, d_packed_sizes, &up, &total_blocks)) return rc;
    const int rc = decode_items_enqueue(c, static_cast<const uint8_t*>(d_in), up.dev<BatchItem>(), n_items, total_blocks, nullptr, d_out, d_sizes,
                                        d_item_status, d_status, s);
    TSQ_HIP(c, up.commit(s));                            // (however the decode launch went: the walk has been enqueued)
    return rc;
}

extern "C" int tsqa_decompress_batch_items_async(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items,
                                                 const uint32_t* n_blocks, uint32_t n_items, void* d_out, size_t out_size, uint64_t* d_sizes,
                                                 int32_t* d_item_status, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    return decompress_batch_items_async_impl(c, d_in, in_size, items, n_blocks, n_items, d_out, out_size, d_sizes, d_item_status, d_status, s);
}

extern "C" int tsqa_decompress_batch_packed_items_async(tsqa_ctx* c, const void* d_arena, size_t arena_size, const uint64_t* d_offsets,
                                                        const uint64_t* d_sizes, const tsqa_batch_item* items, const uint32_t* n_blocks,
                                                        uint32_t n_items, void* d_out, size_t out_size, uint64_t* d_out_sizes,
                                                        int32_t* d_item_status, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_offsets || !d_sizes) { c->set_error("decompress_batch_packed_items: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    return decompress_batch_items_async_impl(c, d_arena, arena_size, items, n_blocks, n_items, d_out, out_size, d_out_sizes, d_item_status,
                                             d_status, s, d_offsets, d_sizes);
}

// ---- dense decompress of a packed batch: block counts and output places made on the device from the headers ----

extern "C" int tsqa_plan_dense(const uint64_t* totals, const uint32_t* blocks, uint32_t n_items, uint32_t align, uint64_t out_size,
                               uint32_t cap_blocks, uint64_t* out_offsets, uint64_t* first_block, uint32_t* n_fit)
{
    if (!totals || !blocks || !out_offsets || !first_block || !n_fit || n_items == 0 || !packed_align_ok(align)) return TSQA_ERR_ARG;
    const uint64_t mask = (uint64_t)align - 1;
    uint64_t at = 0, fb = 0;
    uint32_t fit = n_items;
    for (uint32_t i = 0; i < n_items; ++i) {
        const uint64_t nb = blocks[i], total = nb ? totals[i] : 0;           // (an item refused at its header: no blocks, no bytes)
        out_offsets[i] = at; first_block[i] = fb;
        if (nb && fit == n_items && (fb + nb > cap_blocks || at > out_size || total > out_size - at)) fit = i;
        fb += nb;
        at += total;
        if (i + 1 < n_items) at = (at + mask) & ~mask;
    }
    out_offsets[n_items] = at; first_block[n_items] = fb;
    *n_fit = fit;
    return TSQA_OK;
}

extern "C" int tsqa_decompress_batch_packed_dense_async(tsqa_ctx* c, const void* d_arena, size_t arena_size, const uint64_t* d_offsets,
                                                        const uint64_t* d_sizes, uint32_t n_items, uint32_t align, uint32_t cap_blocks,
                                                        void* d_out, size_t out_size, uint64_t* d_out_offsets, uint64_t* d_out_sizes,
                                                        uint64_t* d_first_block, int32_t* d_item_status, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_arena || !d_offsets || !d_sizes || !d_out_offsets || !d_out_sizes || !d_first_block || !d_item_status || !d_status) {
        c->set_error("decompress_batch_packed_dense: null pointer");
        return TSQA_ERR_ARG;
    }
    if (n_items == 0) { c->set_error("decompress_batch_packed_dense: no items"); return TSQA_ERR_ARG; }
    if (!packed_align_ok(align)) { c->set_error("decompress_batch_packed_dense: align %u is not a power of two from 1 to 4096", align); return TSQA_ERR_ARG; }
    if (d_out ? (out_size == 0 || cap_blocks == 0) : out_size != 0) {
        c->set_error("decompress_batch_packed_dense: an output needs out_size and cap_blocks above 0; measuring takes d_out NULL and out_size 0");
        return TSQA_ERR_ARG;
    }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    if (int rc = c->reserve_batch(n_items)) return rc;
    if (d_out) {
        if (int rc = c->reserve(cap_blocks, false, false, true)) return rc;
        c->forget_sharded();                             // the frame walk below overwrites c->frames
    }
    const uint8_t* const in = static_cast<const uint8_t*>(d_arena);
    const dim3 per_item((uint32_t)(((uint64_t)n_items + 255u) / 256u));
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(batch_measure_kernel, per_item, dim3(256), 0, s, in, c->batch_items, n_items, d_offsets, d_sizes, (uint64_t)arena_size,
                       d_item_status);
    // (measuring: nothing fits, and the kernel closes the batch's word itself)
    hipLaunchKernelGGL(batch_layout_kernel, dim3(1), dim3(256), 0, s, c->batch_items, n_items, align, (uint64_t)out_size, d_out ? cap_blocks : 0u,
                       d_out_offsets, d_out_sizes, d_first_block, d_item_status, c->batch_live, d_out ? nullptr : d_status);
    if (!d_out) { TSQ_HIP(c, hipGetLastError()); return TSQA_OK; }
    return decode_items_enqueue(c, in, static_cast<const BatchItem*>(c->batch_items), n_items, cap_blocks, static_cast<const uint32_t*>(c->batch_live),
                                d_out, d_out_sizes, d_item_status, d_status, s);
}

// ---- join: the containers of a packed batch into one container, nothing decoded (tsq_join.cuh) ----

extern "C" int tsqa_plan_join(const uint64_t* frame_bytes, const uint32_t* blocks, const uint64_t* totals, uint32_t n_items, uint64_t* body_at,
                              uint64_t* first_block, uint32_t* n_blocks, uint64_t* total, uint64_t* size)
{
    if (!frame_bytes || !blocks || !totals || !body_at || !first_block || !n_blocks || !total || !size || n_items == 0) return TSQA_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (blocks[i] == 0 || frame_bytes[i] < kHeaderSize + (uint64_t)kMinFrameSize * blocks[i] || totals[i] > (uint64_t)blocks[i] * kBlockSize)
            return TSQA_ERR_ARG;
    uint64_t at = kHeaderSize, fb = 0, tot = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        body_at[i] = at; first_block[i] = fb;
        at += frame_bytes[i] - kHeaderSize; fb += blocks[i]; tot += totals[i];
    }
    body_at[n_items] = at; first_block[n_items] = fb;
    *n_blocks = (uint32_t)fb; *total = tot; *size = at;
    return fb > 0xFFFFFFFFull ? TSQA_ERR_OVERFLOW : TSQA_OK;
}

// The workgroups of join_emit_kernel: one per piece of the room, at most eight per CU (they stride over the pieces).
static uint32_t join_emit_groups(const tsqa_ctx* c, size_t out_cap)
{
    const uint64_t pieces = ((uint64_t)out_cap + 15u) / kJoinPiece + 1u, most = 8ull * (uint64_t)c->n_cus;
    return (uint32_t)(pieces < most ? pieces : most);
}

extern "C" int tsqa_join_async(tsqa_ctx* c, const void* d_arena, size_t arena_size, const uint64_t* d_offsets, const uint64_t* d_sizes,
                               uint32_t n_items, uint32_t cap_blocks, void* d_out, size_t out_cap, uint64_t* d_out_size, uint64_t* d_first_block,
                               uint32_t* d_block_sizes, int32_t* d_item_status, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_arena || !d_offsets || !d_sizes || !d_out_size || !d_first_block || !d_item_status || !d_status) {
        c->set_error("join: null pointer");
        return TSQA_ERR_ARG;
    }
    if (n_items == 0) { c->set_error("join: no items"); return TSQA_ERR_ARG; }
    if (cap_blocks == 0) { c->set_error("join: cap_blocks is 0"); return TSQA_ERR_ARG; }
    if (d_out ? out_cap < kHeaderSize : out_cap != 0) {
        c->set_error("join: an output needs out_cap of at least 16; measuring takes d_out NULL and out_cap 0");
        return TSQA_ERR_ARG;
    }
    {
        const uintptr_t a = (uintptr_t)d_arena, o = (uintptr_t)d_out;
        if (d_out && o < a + arena_size && a < o + out_cap) { c->set_error("join: the output overlaps the arena"); return TSQA_ERR_ARG; }
    }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    if (int rc = c->reserve_join(n_items)) return rc;
    if (int rc = c->reserve(cap_blocks, false, false, true)) return rc;
    c->forget_sharded();                                 // the frame walk below overwrites c->frames
    const uint8_t* const in = static_cast<const uint8_t*>(d_arena);
    const BatchItem* const items = c->batch_items;
    const dim3 per_item((uint32_t)(((uint64_t)n_items + 255u) / 256u));
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(batch_measure_kernel, per_item, dim3(256), 0, s, in, c->batch_items, n_items, d_offsets, d_sizes, (uint64_t)arena_size,
                       d_item_status);
    hipLaunchKernelGGL(join_blocks_kernel, dim3(1), dim3(256), 0, s, c->batch_items, n_items, cap_blocks, d_first_block, d_item_status);
    hipLaunchKernelGGL(batch_walk_kernel<kWalkJoin>, per_item, dim3(256), 0, s, in, items, n_items, c->frames, (uint32_t*)nullptr, c->batch_sizes,
                       d_item_status);
    hipLaunchKernelGGL(join_bodies_kernel, dim3(1), dim3(256), 0, s, items, n_items, static_cast<const uint64_t*>(c->batch_sizes),
                       static_cast<const uint64_t*>(d_first_block), static_cast<const int32_t*>(d_item_status), static_cast<uint8_t*>(d_out),
                       (uint64_t)out_cap, c->join_at, d_out_size, d_status);
    if (d_out) {
        ProfSpan span(c, 4, s);
        hipLaunchKernelGGL(join_emit_kernel, dim3(join_emit_groups(c, out_cap)), dim3(256), 0, s, in, items, n_items,
                           static_cast<const uint64_t*>(c->join_at), static_cast<uint8_t*>(d_out), static_cast<const uint64_t*>(d_out_size),
                           static_cast<const int32_t*>(d_status));
        span.end();
        if (d_block_sizes)
            hipLaunchKernelGGL(join_block_sizes_kernel, dim3((uint32_t)(((uint64_t)cap_blocks + 255u) / 256u)), dim3(256), 0, s,
                               static_cast<const FrameInfo*>(c->frames), static_cast<const uint64_t*>(d_first_block), n_items, d_block_sizes,
                               static_cast<const int32_t*>(d_status));
    }
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_join(tsqa_ctx* c, const void* d_arena, size_t arena_size, const uint64_t* d_offsets, const uint64_t* d_sizes, uint32_t n_items,
                         uint32_t cap_blocks, void* d_out, size_t out_cap, size_t* out_size, uint32_t* n_blocks, uint64_t* d_first_block,
                         uint32_t* d_block_sizes, int32_t* d_item_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!out_size || !n_blocks) { c->set_error("join: null pointer"); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    if (int rc = tsqa_join_async(c, d_arena, arena_size, d_offsets, d_sizes, n_items, cap_blocks, d_out, out_cap, c->d_size, d_first_block,
                                 d_block_sizes, d_item_status, c->d_status, s)) return rc;
    uint64_t blocks = 0;
    TSQ_HIP(c, hipMemcpyAsync(&blocks, d_first_block + n_items, sizeof(blocks), hipMemcpyDeviceToHost, s));
    const int rc = finish_sync(c, s, "join", out_size);
    if (rc == TSQA_OK || rc == TSQA_ERR_FORMAT || rc == TSQA_ERR_OVERFLOW) *n_blocks = blocks > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)blocks;
    return rc;
}

// ---- cut and take: block ranges of an indexed container, or of the items of any index, each as a container of its own, nothing
// decoded (tsq_cut.cuh) ----

// One container is one item that owns [0, n_blocks); the cut names its ranges and has blocks to cut them from.
extern "C" int tsqa_plan_cut(const uint64_t* frame_at, const uint64_t* out_start, uint32_t n_blocks, const uint64_t* first, const uint64_t* count,
                             uint32_t n_ranges, uint32_t align, uint64_t out_size, uint64_t* offsets, uint64_t* sizes, uint64_t* totals,
                             int32_t* item_status, uint32_t* n_fit)
{
    if (!first || !count || n_blocks == 0) return TSQA_ERR_ARG;
    return tsqa_plan_cut_items(frame_at, out_start, n_blocks, nullptr, 1, nullptr, first, count, n_ranges, align, out_size, offsets, sizes, totals,
                               item_status, n_fit);
}

extern "C" int tsqa_plan_cut_items(const uint64_t* frame_at, const uint64_t* out_start, uint32_t n_blocks, const uint64_t* item_first_block,
                                   uint32_t n_items, const uint32_t* items, const uint64_t* first, const uint64_t* count, uint32_t n_ranges,
                                   uint32_t align, uint64_t out_size, uint64_t* offsets, uint64_t* sizes, uint64_t* totals, int32_t* item_status,
                                   uint32_t* n_fit)
{
    if (!frame_at || !out_start || !offsets || !sizes || !item_status || !n_fit || n_items == 0 || n_ranges == 0 || !packed_align_ok(align))
        return TSQA_ERR_ARG;
    if ((first == nullptr) != (count == nullptr) || (!items && n_items != 1) || (!item_first_block && n_items != 1)) return TSQA_ERR_ARG;
    if (n_blocks != 0 && frame_at[0] < kHeaderSize) return TSQA_ERR_ARG;
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (frame_at[b + 1] < frame_at[b] || frame_at[b + 1] - frame_at[b] < kMinFrameSize || out_start[b + 1] < out_start[b] ||
            out_start[b + 1] - out_start[b] > kBlockSize) return TSQA_ERR_ARG;
    if (item_first_block) {
        for (uint32_t i = 0; i < n_items; ++i) if (item_first_block[i + 1] < item_first_block[i]) return TSQA_ERR_ARG;
        if (item_first_block[n_items] > n_blocks) return TSQA_ERR_ARG;
    }
    const uint64_t mask = (uint64_t)align - 1;
    uint64_t at = 0;
    uint32_t fit = n_ranges;
    for (uint32_t k = 0; k < n_ranges; ++k) {
        const uint32_t it = items ? items[k] : 0u;
        uint64_t fb = 0, fe = 0;
        if (it < n_items) { fb = item_first_block ? item_first_block[it] : 0; fe = item_first_block ? item_first_block[it + 1] : n_blocks; }
        const uint64_t nb = fe - fb, f = first ? first[k] : 0, n = count ? count[k] : nb;
        const bool ok = nb >= 1 && n >= 1 && f < nb && n <= nb - f;
        const uint64_t size = ok ? kHeaderSize + frame_at[fb + f + n] - frame_at[fb + f] : 0;
        offsets[k] = at; sizes[k] = size;
        if (totals) totals[k] = ok ? out_start[fb + f + n] - out_start[fb + f] : 0;
        const bool fits = ok && size <= out_size && at <= out_size - size;
        if (ok && !fits && fit == n_ranges) fit = k;
        item_status[k] = !ok ? TSQA_ERR_ARG : fits ? TSQA_OK : TSQA_ERR_OVERFLOW;
        at += size;
        if (k + 1 < n_ranges) at = (at + mask) & ~mask;
    }
    offsets[n_ranges] = at;
    *n_fit = fit;
    return TSQA_OK;
}

// Both async entry points: the checks, with the caller's name (`who`) and its word for what the index reads (`source`) in the texts,
// and the five launches.
static int cut_enqueue(tsqa_ctx* c, const char* who, const char* source, const tsqa_index* idx, const uint32_t* d_items, const uint64_t* d_first,
                       const uint64_t* d_count, uint32_t n_ranges, uint32_t align, void* d_out, size_t out_size, uint64_t* d_offsets,
                       uint64_t* d_sizes, uint64_t* d_totals, int32_t* d_item_status, int32_t* d_status, hipStream_t s)
{
    if (!idx || !d_offsets || !d_sizes || !d_item_status || !d_status) { c->set_error("%s: null pointer", who); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("%s: the index belongs to device %d, the context to %d", who, idx->device, c->device); return TSQA_ERR_ARG; }
    if (n_ranges == 0) { c->set_error("%s: no ranges", who); return TSQA_ERR_ARG; }
    if (!packed_align_ok(align)) { c->set_error("%s: align %u is not a power of two from 1 to 4096", who, align); return TSQA_ERR_ARG; }
    if ((d_first == nullptr) != (d_count == nullptr)) { c->set_error("%s: d_first and d_count go together; both NULL takes whole items", who); return TSQA_ERR_ARG; }
    const uint32_t n_items = tsqa_index_items(idx);
    if (!d_items && n_items != 1) { c->set_error("%s: an index of %u items needs d_items", who, n_items); return TSQA_ERR_ARG; }
    if (d_out ? out_size < kHeaderSize : out_size != 0) {
        c->set_error("%s: an output needs out_size of at least 16; measuring takes d_out NULL and out_size 0", who);
        return TSQA_ERR_ARG;
    }
    {
        const uintptr_t a = (uintptr_t)idx->container, o = (uintptr_t)d_out;
        if (d_out && o < a + idx->n && a < o + out_size) { c->set_error("%s: the output overlaps the index's %s", who, source); return TSQA_ERR_ARG; }
    }
    // (the sizes go through group_scan_excl64, whose sums stay below 2^55; one source byte may be counted once per range)
    if ((unsigned __int128)n_ranges * ((unsigned __int128)idx->n + 4096u) >= (unsigned __int128)1 << 55) { c->set_error("%s: %u ranges of a %s of %zu B", who, n_ranges, source, idx->n); return TSQA_ERR_ARG; }
    (void)hipSetDevice(c->device);
    if (int rc = c->reserve_cut(n_ranges)) return rc;
    CutRange* const ranges = c->cut_ranges;
    uint64_t* const groups = c->cut_groups;
    uint64_t* const fit_end = &ranges[n_ranges].src_at;  // where cut_emit_kernel looks for the end of the written output
    // (a batch index made on the device and not fetched: cap_blocks descriptors, the live count in its words)
    const bool live = idx->pending_items != 0u;
    const uint32_t n_groups = (uint32_t)(((uint64_t)n_ranges + kTakeGroup - 1u) / kTakeGroup);
    hipLaunchKernelGGL(cut_measure_kernel, dim3(n_groups), dim3(256), 0, s, static_cast<const FrameInfo*>(idx->frames),
                       live ? idx->cap_blocks : idx->n_blocks, static_cast<const int32_t*>(idx->verdict),
                       static_cast<const uint64_t*>(idx->d_item_first), n_items, live ? static_cast<const uint64_t*>(idx->d_words) : nullptr, d_items,
                       d_first, d_count, n_ranges, ranges, d_sizes, d_totals, d_item_status);
    hipLaunchKernelGGL(cut_sum_kernel, dim3(n_groups), dim3(256), 0, s, static_cast<const uint64_t*>(d_sizes), n_ranges, align, d_offsets, groups);
    hipLaunchKernelGGL(cut_scan_kernel, dim3(1), dim3(256), 0, s, groups, n_groups, fit_end, d_status);
    hipLaunchKernelGGL(cut_place_kernel, dim3(n_groups), dim3(256), 0, s, static_cast<const CutRange*>(ranges), n_ranges,
                       static_cast<const uint64_t*>(groups), static_cast<uint8_t*>(d_out), (uint64_t)out_size, static_cast<const uint64_t*>(d_sizes),
                       d_offsets, d_item_status, fit_end, d_status);
    if (d_out) {
        ProfSpan span(c, 5, s);
        hipLaunchKernelGGL(cut_emit_kernel, dim3(join_emit_groups(c, out_size)), dim3(256), 0, s, idx->container,
                           static_cast<const CutRange*>(ranges), n_ranges, static_cast<const uint64_t*>(d_offsets),
                           static_cast<const uint64_t*>(d_sizes), static_cast<uint8_t*>(d_out));
        span.end();
    }
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_cut_async(tsqa_ctx* c, const tsqa_index* idx, const uint64_t* d_first, const uint64_t* d_count, uint32_t n_ranges,
                              uint32_t align, void* d_out, size_t out_size, uint64_t* d_offsets, uint64_t* d_sizes, uint64_t* d_totals,
                              int32_t* d_item_status, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!idx || !d_first || !d_count) { c->set_error("cut: null pointer"); return TSQA_ERR_ARG; }
    // (fetched or not, and of one item too: its descriptors count from the arena's start, not from a container's)
    if (idx->d_words) { c->set_error("cut: a batch index made on the device; its items already are separate containers"); return TSQA_ERR_ARG; }
    if (idx->item_status.size() != 1) { c->set_error("cut: an index of %zu items; its items already are separate containers", idx->item_status.size()); return TSQA_ERR_ARG; }
    return cut_enqueue(c, "cut", "container", idx, nullptr, d_first, d_count, n_ranges, align, d_out, out_size, d_offsets, d_sizes, d_totals,
                       d_item_status, d_status, stream_of(c, hip_stream));
}

extern "C" int tsqa_cut_items_async(tsqa_ctx* c, const tsqa_index* idx, const uint32_t* d_items, const uint64_t* d_first, const uint64_t* d_count,
                                    uint32_t n_ranges, uint32_t align, void* d_out, size_t out_size, uint64_t* d_offsets, uint64_t* d_sizes,
                                    uint64_t* d_totals, int32_t* d_item_status, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    return cut_enqueue(c, "cut_items", "buffer", idx, d_items, d_first, d_count, n_ranges, align, d_out, out_size, d_offsets, d_sizes, d_totals,
                       d_item_status, d_status, stream_of(c, hip_stream));
}

// Both waiting forms: `enqueue` is the async call into the context's batch tables, which are then copied to the host's.
template <class Enqueue>
static int cut_wait(tsqa_ctx* c, const char* who, uint32_t n_ranges, uint64_t* offsets, uint64_t* sizes, uint64_t* totals, int32_t* item_status,
                    void* hip_stream, Enqueue enqueue)
{
    if (!c) return TSQA_ERR_ARG;
    if (!offsets || !sizes || !item_status) { c->set_error("%s: null pointer", who); return TSQA_ERR_ARG; }
    if (n_ranges == 0) { c->set_error("%s: no ranges", who); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    if (int rc = c->reserve_batch(n_ranges)) return rc;      // (the device tables of the waiting form are the batch calls')
    if (int rc = enqueue(s)) return rc;
    TSQ_HIP(c, hipMemcpyAsync(offsets, c->batch_offsets, ((size_t)n_ranges + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipMemcpyAsync(sizes, c->batch_sizes, (size_t)n_ranges * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (totals) TSQ_HIP(c, hipMemcpyAsync(totals, c->batch_at, (size_t)n_ranges * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipMemcpyAsync(item_status, c->batch_status, (size_t)n_ranges * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return finish_sync(c, s, who);
}

extern "C" int tsqa_cut(tsqa_ctx* c, const tsqa_index* idx, const uint64_t* d_first, const uint64_t* d_count, uint32_t n_ranges, uint32_t align,
                        void* d_out, size_t out_size, uint64_t* offsets, uint64_t* sizes, uint64_t* totals, int32_t* item_status,
                        void* hip_stream)
{
    return cut_wait(c, "cut", n_ranges, offsets, sizes, totals, item_status, hip_stream, [&](hipStream_t s) {
        return tsqa_cut_async(c, idx, d_first, d_count, n_ranges, align, d_out, out_size, c->batch_offsets, c->batch_sizes, c->batch_at,
                              c->batch_status, c->d_status, s);
    });
}

extern "C" int tsqa_cut_items(tsqa_ctx* c, const tsqa_index* idx, const uint32_t* d_items, const uint64_t* d_first, const uint64_t* d_count,
                              uint32_t n_ranges, uint32_t align, void* d_out, size_t out_size, uint64_t* offsets, uint64_t* sizes, uint64_t* totals,
                              int32_t* item_status, void* hip_stream)
{
    return cut_wait(c, "cut_items", n_ranges, offsets, sizes, totals, item_status, hip_stream, [&](hipStream_t s) {
        return tsqa_cut_items_async(c, idx, d_items, d_first, d_count, n_ranges, align, d_out, out_size, c->batch_offsets, c->batch_sizes,
                                    c->batch_at, c->batch_status, c->d_status, s);
    });
}

// ---- gather: record reads whose ranges lie in device memory, planned there, into a dense output (tsq_gather.cuh) ----

// What keeps every sum of the gather's scans below 2^55 (group_scan_excl64): a range is at most the index's total and is padded by
// less than 4096, and it has at most one piece per block.
static bool gather_sums_ok(uint32_t n_ranges, uint64_t total, uint32_t n_blocks)
{
    const unsigned __int128 limit = (unsigned __int128)1 << 55;
    return (unsigned __int128)n_ranges * ((unsigned __int128)total + 4096u) < limit && (unsigned __int128)n_ranges * n_blocks < limit;
}

extern "C" int tsqa_plan_gather(const uint64_t* out_start, uint32_t n_blocks, const uint64_t* item_first_block, uint32_t n_items,
                                const uint32_t* items, const uint64_t* offsets, const uint64_t* lengths, uint32_t n_ranges, uint32_t align,
                                uint64_t out_cap, uint32_t cap_pieces, uint64_t* out_offsets, int32_t* range_status, uint64_t* n_pieces,
                                uint32_t* n_groups)
{
    if (!out_start || !item_first_block || !offsets || !lengths || !out_offsets || !range_status || !n_pieces || !n_groups || n_items == 0 ||
        !packed_align_ok(align) || cap_pieces < 1) return TSQA_ERR_ARG;
    if (out_start[0] != 0 || item_first_block[0] != 0 || item_first_block[n_items] != n_blocks) return TSQA_ERR_ARG;
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (out_start[b + 1] < out_start[b] || out_start[b + 1] - out_start[b] > kBlockSize) return TSQA_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_first_block[i + 1] < item_first_block[i]) return TSQA_ERR_ARG;
    if (!gather_sums_ok(n_ranges, out_start[n_blocks], n_blocks)) return TSQA_ERR_ARG;
    const uint64_t mask = (uint64_t)align - 1;
    uint64_t at = 0, pieces_at = 0, last_len = 0;
    bool open = true;                                        // no accepted range has failed to fit yet
    std::vector<uint32_t> touched;
    try {
        for (uint32_t k = 0; k < n_ranges; ++k) {
            uint64_t base = 0, mine = out_start[n_blocks];
            bool ok = true;
            if (items) {
                ok = items[k] < n_items && item_first_block[items[k]] < item_first_block[items[k] + 1];
                if (ok) { base = out_start[item_first_block[items[k]]]; mine = out_start[item_first_block[items[k] + 1]] - base; }
            }
            ok = ok && lengths[k] <= mine && offsets[k] <= mine - lengths[k];
            const uint64_t len = ok ? lengths[k] : 0, a = base + offsets[k], e = a + len;
            uint64_t first = 0, pieces = 0;
            if (len) {
                first = (uint64_t)(std::upper_bound(out_start, out_start + n_blocks + 1, a) - out_start) - 1;
                for (uint64_t b = first; b < n_blocks && out_start[b] < e; ++b) pieces += out_start[b + 1] > out_start[b];
            }
            const bool fits = ok && open && (len == 0 || (len <= out_cap && at <= out_cap - len && pieces <= cap_pieces && pieces_at <= cap_pieces - pieces));
            if (ok && !fits) open = false;
            range_status[k] = !ok ? TSQA_ERR_ARG : fits ? TSQA_OK : TSQA_ERR_OVERFLOW;
            out_offsets[k] = at;
            if (fits && len)
                for (uint64_t b = first; b < n_blocks && out_start[b] < e; ++b)
                    if (out_start[b + 1] > out_start[b]) touched.push_back((uint32_t)b);
            last_len = len;
            at += (len + mask) & ~mask;
            pieces_at += pieces;
        }
        std::sort(touched.begin(), touched.end());
        *n_groups = (uint32_t)(std::unique(touched.begin(), touched.end()) - touched.begin());
    } catch (...) { return TSQA_ERR_ARG; }
    out_offsets[n_ranges] = n_ranges ? at - ((last_len + mask) & ~mask) + last_len : 0;
    *n_pieces = pieces_at;
    return TSQA_OK;
}

extern "C" int tsqa_gather_async(tsqa_ctx* c, const tsqa_index* idx, const uint32_t* d_items, const uint64_t* d_offsets, const uint64_t* d_lengths,
                                 uint32_t n_ranges, uint32_t align, uint32_t cap_pieces, void* d_out, size_t out_cap, uint64_t* d_out_offsets,
                                 int32_t* d_range_status, uint64_t* d_need_pieces, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!idx || !d_offsets || !d_lengths || !d_out || !d_out_offsets || !d_range_status || !d_need_pieces || !d_status) { c->set_error("gather: null pointer"); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("gather: the index belongs to device %d, the context to %d", idx->device, c->device); return TSQA_ERR_ARG; }
    if (!packed_align_ok(align)) { c->set_error("gather: align %u is not a power of two from 1 to 4096", align); return TSQA_ERR_ARG; }
    if (cap_pieces < 1) { c->set_error("gather: cap_pieces of 0"); return TSQA_ERR_ARG; }
    // (the lengths and the piece counts go through group_scan_excl64, whose sums stay below 2^55)
    // (a batch index made on the device and not fetched: its total is the device's, and the host bounds it by what cap_blocks hold)
    const bool live = idx->pending_items != 0u;
    const uint32_t n_blocks = live ? idx->cap_blocks : idx->n_blocks;
    const uint64_t total_bound = live ? (uint64_t)idx->cap_blocks * (idx->packed_block_len ? idx->packed_block_len : kBlockSize) : idx->total;
    if (!gather_sums_ok(n_ranges, total_bound, n_blocks)) {
        c->set_error("gather: %u ranges of an index of %s%llu B in %u blocks", n_ranges, live ? "at most " : "", (unsigned long long)total_bound, n_blocks);
        return TSQA_ERR_ARG;
    }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    if (n_ranges == 0) {
        TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
        TSQ_HIP(c, hipMemsetAsync(d_need_pieces, 0, sizeof(uint64_t), s));
        TSQ_HIP(c, hipMemsetAsync(d_out_offsets, 0, sizeof(uint64_t), s));
        return TSQA_OK;
    }
    const uint32_t cap_groups = cap_pieces < n_blocks ? cap_pieces : n_blocks;
    if (int rc = c->reserve_gather(n_ranges, cap_pieces, cap_groups ? cap_groups : 1)) return rc;
    GatherRange* const ranges = c->gather_ranges;
    GatherWords* const words = c->gather_words;
    RangeItem* const items = c->gather_items;
    RangeItem* const sorted = items + cap_pieces;
    uint64_t* const keys = c->gather_keys;
    uint32_t* const slots = c->gather_slots;
    BlockGroup* const groups = c->gather_groups;
    const uint32_t n_items = tsqa_index_items(idx);
    ProfSpan plan(c, 6, s);
    // (two instantiations: the one that reads the total from the index's device words serves the unfetched batch index alone)
    void (*const measure)(const FrameInfo*, uint32_t, uint64_t, uint32_t, const int32_t*, const uint64_t*, uint32_t, const uint32_t*, const uint64_t*,
                          const uint64_t*, uint32_t, GatherRange*, int32_t*, const uint64_t*) = live ? gather_measure_kernel<true> : gather_measure_kernel<false>;
    hipLaunchKernelGGL(measure, dim3((uint32_t)(((uint64_t)n_ranges + 255u) / 256u)), dim3(256), 0, s,
                       static_cast<const FrameInfo*>(idx->frames), n_blocks, idx->total, idx->block_shift, static_cast<const int32_t*>(idx->verdict),
                       static_cast<const uint64_t*>(idx->d_item_first), n_items, d_items, d_offsets, d_lengths, n_ranges, ranges, d_range_status,
                       static_cast<const uint64_t*>(idx->d_words));
    hipLaunchKernelGGL(gather_layout_kernel, dim3(1), dim3(256), 0, s, ranges, n_ranges, align, (uint64_t)out_cap, cap_pieces, d_out_offsets,
                       d_range_status, d_need_pieces, words, d_status);
    int rc = TSQA_OK;
    if (n_blocks) {
        const uint64_t lanes = n_ranges > cap_pieces ? n_ranges : cap_pieces, piece_groups = ((uint64_t)cap_pieces + 255u) / 256u;
        hipLaunchKernelGGL(gather_pieces_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, s, static_cast<const FrameInfo*>(idx->frames),
                           n_blocks, static_cast<const GatherRange*>(ranges), n_ranges, static_cast<const int32_t*>(d_range_status),
                           static_cast<const uint64_t*>(d_out_offsets), static_cast<const GatherWords*>(words), cap_pieces, items, keys, slots);
        TSQ_HIP(c, gather_sort_pairs(c->gather_sort, c->gather_sort_bytes, keys, keys + cap_pieces, slots, slots + cap_pieces, cap_pieces, s));
        const uint64_t movers = piece_groups < 4ull * (uint64_t)c->n_cus ? piece_groups : 4ull * (uint64_t)c->n_cus;
        hipLaunchKernelGGL(gather_groups_kernel, dim3((uint32_t)(1u + movers)), dim3(256), 0, s, static_cast<const RangeItem*>(items),
                           static_cast<const uint64_t*>(keys + cap_pieces), static_cast<const uint32_t*>(slots + cap_pieces), words, cap_pieces,
                           sorted, groups, cap_groups);
        hipLaunchKernelGGL(gather_spans_kernel, dim3((cap_groups + 255u) / 256u), dim3(256), 0, s, static_cast<const RangeItem*>(sorted),
                           static_cast<const GatherWords*>(words), cap_pieces, groups, cap_groups);
        plan.end();
        ProfSpan dec(c, 7, s);
        rc = launch_read_kernel<dec_group_live_kernel>(c, cap_groups, s, idx->container, static_cast<const FrameInfo*>(idx->frames), n_blocks,
                                                       static_cast<const RangeItem*>(sorted), cap_pieces, static_cast<const BlockGroup*>(groups),
                                                       static_cast<uint8_t*>(d_out), &words->stream, static_cast<const uint32_t*>(&words->n_groups));
        dec.end();
    } else plan.end();
    hipLaunchKernelGGL(gather_close_kernel, dim3(1), dim3(1), 0, s, static_cast<const GatherWords*>(words), d_status);
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_gather(tsqa_ctx* c, const tsqa_index* idx, const uint32_t* d_items, const uint64_t* d_offsets, const uint64_t* d_lengths,
                           uint32_t n_ranges, uint32_t align, uint32_t cap_pieces, void* d_out, size_t out_cap, uint64_t* d_out_offsets,
                           int32_t* d_range_status, uint64_t* d_need_pieces, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    if (int rc = tsqa_gather_async(c, idx, d_items, d_offsets, d_lengths, n_ranges, align, cap_pieces, d_out, out_cap, d_out_offsets,
                                   d_range_status, d_need_pieces, d_status, s)) return rc;
    int32_t st = 0;
    TSQ_HIP(c, hipMemcpyAsync(&st, d_status, sizeof(st), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    return status_to_rc(c, st, "gather");
}

// ---- record tables from a delimiter byte: a decode that writes one bit per byte, then a count, a scan and a placement (tsq_records.cuh) ----

extern "C" int tsqa_plan_records(const void* data, const uint64_t* item_at, const int32_t* item_status, uint32_t n_items, uint32_t delim,
                                 uint32_t flags, uint64_t cap_records, uint32_t* rec_items, uint64_t* rec_offsets, uint64_t* rec_lengths,
                                 uint64_t* item_first_record, uint64_t* need)
{
    if (!item_at || !item_first_record || !need || n_items == 0 || delim > 255u || (flags & ~(TSQA_RECORDS_KEEP_DELIM | TSQA_RECORDS_FLAT)) != 0u)
        return TSQA_ERR_ARG;
    if (cap_records > 0 && (!rec_offsets || !rec_lengths)) return TSQA_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_at[i + 1] < item_at[i]) return TSQA_ERR_ARG;
    if (!data && item_at[n_items] != item_at[0]) return TSQA_ERR_ARG;
    const uint8_t* const bytes = static_cast<const uint8_t*>(data);
    const uint64_t keep = flags & TSQA_RECORDS_KEEP_DELIM ? 1u : 0u;
    uint64_t no = 0, longest = 0;
    auto put = [&](uint32_t item, uint64_t offset, uint64_t len) {
        if (len > longest) longest = len;
        if (no < cap_records) { if (rec_items) rec_items[no] = item; rec_offsets[no] = offset; rec_lengths[no] = len; }
        ++no;
    };
    for (uint32_t i = 0; i < n_items; ++i) {
        item_first_record[i] = no;
        const uint64_t a = item_at[i], e = item_at[i + 1], origin = flags & TSQA_RECORDS_FLAT ? 0ull : a;
        if (a == e || (item_status && item_status[i] != 0)) continue;
        uint64_t start = a;
        while (start < e) {
            const uint8_t* const hit = static_cast<const uint8_t*>(memchr(bytes + start, (int)delim, (size_t)(e - start)));
            if (!hit) { put(i, start - origin, e - start); break; }
            const uint64_t p = (uint64_t)(hit - bytes);
            put(i, start - origin, p - start + keep);
            start = p + 1;                                   // (a terminator at the item's last byte starts no record)
        }
    }
    item_first_record[n_items] = no;
    need[0] = no; need[1] = longest;
    return TSQA_OK;
}

extern "C" int tsqa_records_async(tsqa_ctx* c, const tsqa_index* idx, uint32_t delim, uint32_t flags, uint64_t cap_records, uint32_t* d_rec_items,
                                  uint64_t* d_rec_offsets, uint64_t* d_rec_lengths, uint64_t* d_item_first_record, uint64_t* d_need,
                                  int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!idx || !d_item_first_record || !d_need || !d_status) { c->set_error("records: null pointer"); return TSQA_ERR_ARG; }
    if (delim > 255u) { c->set_error("records: delim %u is no byte value", delim); return TSQA_ERR_ARG; }
    if ((flags & ~(TSQA_RECORDS_KEEP_DELIM | TSQA_RECORDS_FLAT)) != 0u) { c->set_error("records: unknown flags 0x%x", flags); return TSQA_ERR_ARG; }
    if (cap_records > 0 && (!d_rec_offsets || !d_rec_lengths)) { c->set_error("records: cap_records of %llu with a NULL offsets or lengths table", (unsigned long long)cap_records); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("records: the index belongs to device %d, the context to %d", idx->device, c->device); return TSQA_ERR_ARG; }
    // (the host sizes the bit map from the total and the block count, which it does not have before the fetch)
    if (idx->pending_items != 0u) { c->set_error("records: %s", kNeedsFetch); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    const uint32_t n_blocks = idx->n_blocks, n_items = tsqa_index_items(idx);
    const uint32_t item_groups = (uint32_t)(((uint64_t)n_items + 1u + 255u) / 256u);
    if (n_blocks == 0) {
        TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
        TSQ_HIP(c, hipMemsetAsync(d_need, 0, 2 * sizeof(uint64_t), s));
        hipLaunchKernelGGL(records_clear_kernel, dim3(item_groups), dim3(256), 0, s, d_item_first_record, n_items);
        TSQ_HIP(c, hipGetLastError());
        return TSQA_OK;
    }
    const uint64_t map_words = (idx->total >> 6) + n_blocks + 1u;
    if (int rc = c->reserve_records((size_t)map_words, n_blocks)) return rc;
    uint64_t* const map = c->records_map;
    RecordBlock* const blocks = c->records_blocks;
    const uint32_t n_groups = (n_blocks + kRecordsGroup - 1u) / kRecordsGroup;
    uint64_t* const group_sum = c->records_groups;
    uint64_t* const group_edge = group_sum + c->records_groups.cap / 2;
    RecordWords* const words = c->records_words;
    const FrameInfo* const frames = idx->frames;
    const int32_t* const verdict = idx->verdict;
    const uint64_t* const item_first = idx->d_item_first;
    TSQ_HIP(c, hipMemsetAsync(words, 0, sizeof(RecordWords), s));
    TSQ_HIP(c, hipMemsetAsync(map, 0, (size_t)map_words * sizeof(uint64_t), s));
    ProfSpan mark(c, 9, s);
    const int rc = launch_read_kernel<dec_mark_kernel>(c, n_blocks, s, idx->container, frames, verdict, delim, map, map_words, &words->stream);
    if (rc) { mark.cancel(); return rc; }
    mark.end();
    ProfSpan table(c, 10, s);
    hipLaunchKernelGGL(records_count_kernel, dim3(n_blocks), dim3(256), 0, s, frames, n_blocks, idx->total, verdict, item_first, n_items,
                       static_cast<const uint64_t*>(map), map_words, blocks);
    hipLaunchKernelGGL(records_sum_kernel, dim3(n_groups), dim3(256), 0, s, blocks, n_blocks, group_sum, group_edge);
    hipLaunchKernelGGL(records_scan_kernel, dim3(1), dim3(256), 0, s, group_sum, group_edge, n_groups, verdict, cap_records, d_need, words);
    hipLaunchKernelGGL(records_place_kernel, dim3(n_groups), dim3(256), 0, s, blocks, n_blocks, static_cast<const uint64_t*>(group_sum),
                       static_cast<const uint64_t*>(group_edge));
    hipLaunchKernelGGL(records_items_kernel, dim3(item_groups), dim3(256), 0, s, static_cast<const RecordBlock*>(blocks), n_blocks, item_first, n_items,
                       static_cast<const uint64_t*>(d_need), d_item_first_record);
    hipLaunchKernelGGL(records_emit_kernel, dim3(n_blocks), dim3(256), 0, s, frames, verdict, static_cast<const uint64_t*>(map), map_words,
                       static_cast<const RecordBlock*>(blocks), flags, cap_records, d_rec_items, d_rec_offsets, d_rec_lengths, d_need);
    hipLaunchKernelGGL(records_close_kernel, dim3(1), dim3(1), 0, s, static_cast<const RecordWords*>(words), d_status);
    table.end();
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_records(tsqa_ctx* c, const tsqa_index* idx, uint32_t delim, uint32_t flags, uint64_t cap_records, uint32_t* d_rec_items,
                            uint64_t* d_rec_offsets, uint64_t* d_rec_lengths, uint64_t* d_item_first_record, uint64_t* d_need, int32_t* d_status,
                            void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    if (int rc = tsqa_records_async(c, idx, delim, flags, cap_records, d_rec_items, d_rec_offsets, d_rec_lengths, d_item_first_record, d_need,
                                    d_status, s)) return rc;
    int32_t st = 0;
    TSQ_HIP(c, hipMemcpyAsync(&st, d_status, sizeof(st), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    return status_to_rc(c, st, "records");
}

// ---- where a byte string occurs: a decode that compares with the needle and writes one bit per hit's end, the seams between the
// blocks from their edge bytes, then the records' count, scan and placement over the map (tsq_find.cuh) ----

extern "C" int tsqa_plan_find(const void* data, const uint64_t* item_at, const int32_t* item_status, uint32_t n_items, const void* needle,
                              uint32_t needle_len, uint32_t flags, uint64_t cap_hits, uint32_t* hit_items, uint64_t* hit_offsets,
                              uint64_t* item_first_hit, uint64_t* need)
{
    if (!item_at || !item_first_hit || !need || !needle || n_items == 0 || needle_len == 0 || needle_len > TSQA_FIND_MAX_NEEDLE ||
        (flags & ~TSQA_FIND_FLAT) != 0u)
        return TSQA_ERR_ARG;
    if (cap_hits > 0 && !hit_offsets) return TSQA_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_at[i + 1] < item_at[i]) return TSQA_ERR_ARG;
    if (!data && item_at[n_items] != item_at[0]) return TSQA_ERR_ARG;
    const uint8_t* const bytes = static_cast<const uint8_t*>(data);
    const uint8_t* const nd = static_cast<const uint8_t*>(needle);
    const uint64_t m = needle_len;
    uint64_t no = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        item_first_hit[i] = no;
        const uint64_t a = item_at[i], e = item_at[i + 1], origin = flags & TSQA_FIND_FLAT ? 0ull : a;
        if (e - a < m || (item_status && item_status[i] != 0)) continue;
        for (uint64_t p = a; p + m <= e; ++p) {
            // (the first byte is the filter; overlapping hits all count, so the walk advances by one)
            const uint8_t* const hit = static_cast<const uint8_t*>(memchr(bytes + p, nd[0], (size_t)(e - m + 1 - p)));
            if (!hit) break;
            p = (uint64_t)(hit - bytes);
            if (memcmp(bytes + p, nd, (size_t)m) != 0) continue;
            if (no < cap_hits) { if (hit_items) hit_items[no] = i; hit_offsets[no] = p - origin; }
            ++no;
        }
    }
    item_first_hit[n_items] = no;
    need[0] = no;
    return TSQA_OK;
}

extern "C" int tsqa_find_async(tsqa_ctx* c, const tsqa_index* idx, const void* needle, uint32_t needle_len, uint32_t flags, uint64_t cap_hits,
                               uint32_t* d_hit_items, uint64_t* d_hit_offsets, uint64_t* d_item_first_hit, uint64_t* d_need, int32_t* d_status,
                               void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!idx || !needle || !d_item_first_hit || !d_need || !d_status) { c->set_error("find: null pointer"); return TSQA_ERR_ARG; }
    if (needle_len == 0u || needle_len > TSQA_FIND_MAX_NEEDLE) { c->set_error("find: a needle of %u bytes (1 .. %u)", needle_len, TSQA_FIND_MAX_NEEDLE); return TSQA_ERR_ARG; }
    if ((flags & ~TSQA_FIND_FLAT) != 0u) { c->set_error("find: unknown flags 0x%x", flags); return TSQA_ERR_ARG; }
    if (cap_hits > 0 && !d_hit_offsets) { c->set_error("find: cap_hits of %llu with a NULL offsets table", (unsigned long long)cap_hits); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("find: the index belongs to device %d, the context to %d", idx->device, c->device); return TSQA_ERR_ARG; }
    // (the host sizes the bit map from the total and the block count, which it does not have before the fetch)
    if (idx->pending_items != 0u) { c->set_error("find: %s", kNeedsFetch); return TSQA_ERR_ARG; }
    // the needle is read here and travels as kernel arguments: the caller's buffer is free when the call returns
    uint32_t nw[4] = {0u, 0u, 0u, 0u};
    memcpy(nw, needle, needle_len);
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    const uint32_t n_blocks = idx->n_blocks, n_items = tsqa_index_items(idx);
    const uint32_t item_groups = (uint32_t)(((uint64_t)n_items + 1u + 255u) / 256u);
    if (n_blocks == 0) {
        TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
        TSQ_HIP(c, hipMemsetAsync(d_need, 0, sizeof(uint64_t), s));
        hipLaunchKernelGGL(records_clear_kernel, dim3(item_groups), dim3(256), 0, s, d_item_first_hit, n_items);
        TSQ_HIP(c, hipGetLastError());
        return TSQA_OK;
    }
    const uint64_t map_words = (idx->total >> 6) + n_blocks + 1u;
    if (int rc = c->reserve_find((size_t)map_words, n_blocks)) return rc;
    uint64_t* const map = c->records_map;
    RecordBlock* const blocks = c->records_blocks;
    const uint32_t n_groups = (n_blocks + kRecordsGroup - 1u) / kRecordsGroup;
    uint64_t* const group_sum = c->records_groups;
    uint64_t* const group_edge = group_sum + c->records_groups.cap / 2;
    RecordWords* const words = c->records_words;
    uint8_t* const edges = c->find_edges;
    uint64_t* const count = c->find_need;
    const FrameInfo* const frames = idx->frames;
    const int32_t* const verdict = idx->verdict;
    const uint64_t* const item_first = idx->d_item_first;
    TSQ_HIP(c, hipMemsetAsync(words, 0, sizeof(RecordWords), s));
    TSQ_HIP(c, hipMemsetAsync(map, 0, (size_t)map_words * sizeof(uint64_t), s));
    ProfSpan find(c, 11, s);
    const int rc = launch_read_kernel<dec_find_kernel>(c, n_blocks, s, idx->container, frames, verdict, nw[0], nw[1], nw[2], nw[3], needle_len, map,
                                                       map_words, edges, &words->stream);
    if (rc) { find.cancel(); return rc; }
    find.end();
    ProfSpan table(c, 12, s);
    if (needle_len > 1u)
        hipLaunchKernelGGL(find_seam_kernel, dim3(n_groups), dim3(256), 0, s, frames, n_blocks, idx->total, idx->block_shift, verdict, item_first, n_items,
                           nw[0], nw[1], nw[2], nw[3], needle_len, static_cast<const uint8_t*>(edges), map, map_words);
    hipLaunchKernelGGL(find_count_kernel, dim3(n_blocks), dim3(256), 0, s, frames, n_blocks, idx->total, verdict, item_first, n_items,
                       static_cast<const uint64_t*>(map), map_words, blocks);
    hipLaunchKernelGGL(records_sum_kernel, dim3(n_groups), dim3(256), 0, s, blocks, n_blocks, group_sum, group_edge);
    hipLaunchKernelGGL(records_scan_kernel, dim3(1), dim3(256), 0, s, group_sum, group_edge, n_groups, verdict, cap_hits, count, words);
    hipLaunchKernelGGL(records_place_kernel, dim3(n_groups), dim3(256), 0, s, blocks, n_blocks, static_cast<const uint64_t*>(group_sum),
                       static_cast<const uint64_t*>(group_edge));
    hipLaunchKernelGGL(records_items_kernel, dim3(item_groups), dim3(256), 0, s, static_cast<const RecordBlock*>(blocks), n_blocks, item_first, n_items,
                       static_cast<const uint64_t*>(count), d_item_first_hit);
    hipLaunchKernelGGL(find_emit_kernel, dim3(n_blocks), dim3(256), 0, s, frames, verdict, static_cast<const uint64_t*>(map), map_words,
                       static_cast<const RecordBlock*>(blocks), needle_len, flags, cap_hits, d_hit_items, d_hit_offsets);
    hipLaunchKernelGGL(find_close_kernel, dim3(1), dim3(1), 0, s, static_cast<const RecordWords*>(words), static_cast<const uint64_t*>(count), d_need,
                       d_status);
    table.end();
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_find(tsqa_ctx* c, const tsqa_index* idx, const void* needle, uint32_t needle_len, uint32_t flags, uint64_t cap_hits,
                         uint32_t* d_hit_items, uint64_t* d_hit_offsets, uint64_t* d_item_first_hit, uint64_t* d_need, int32_t* d_status,
                         void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    if (int rc = tsqa_find_async(c, idx, needle, needle_len, flags, cap_hits, d_hit_items, d_hit_offsets, d_item_first_hit, d_need, d_status, s))
        return rc;
    int32_t st = 0;
    TSQ_HIP(c, hipMemcpyAsync(&st, d_status, sizeof(st), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    return status_to_rc(c, st, "find");
}

// ---- zlib's CRC-32 of every item: a decode that keeps one word per block, a fold of the blocks' words into the items' and a
// close (tsq_crc.cuh); the arithmetic and its host forms (tsq_crc32.h) ----

static constexpr CrcTables kCrcHostTables = crc_make_tables();

extern "C" uint32_t tsqa_crc32_host(uint32_t crc, const void* buf, size_t n)
{
    return buf ? crc_update_host(kCrcHostTables, crc, static_cast<const uint8_t*>(buf), n) : crc;
}

extern "C" uint32_t tsqa_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b)
{
    return crc_mul(crc_a, crc_xpow8(len_b)) ^ crc_b;
}

extern "C" int tsqa_plan_crc32(const void* data, const uint64_t* item_at, const int32_t* item_status, uint32_t n_items, uint32_t* item_crc,
                               uint32_t* all_crc)
{
    if (!item_at || !item_crc || n_items == 0) return TSQA_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_at[i + 1] < item_at[i]) return TSQA_ERR_ARG;
    if (!data && item_at[n_items] != item_at[0]) return TSQA_ERR_ARG;
    const uint8_t* const bytes = static_cast<const uint8_t*>(data);
    uint32_t all = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        const uint64_t a = item_at[i], e = item_at[i + 1];
        item_crc[i] = 0;
        if (a == e || (item_status && item_status[i] != 0)) continue;       // (a refused item has no bytes in the whole data either)
        all = crc_update_host(kCrcHostTables, all, bytes + a, (size_t)(e - a));
        item_crc[i] = crc_update_host(kCrcHostTables, 0u, bytes + a, (size_t)(e - a));
    }
    if (all_crc) *all_crc = all;
    return TSQA_OK;
}

extern "C" int tsqa_crc32_async(tsqa_ctx* c, const tsqa_index* idx, uint32_t flags, uint32_t* d_item_crc, int32_t* d_item_status,
                                uint32_t* d_block_crc, uint32_t* d_all_crc, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!idx || !d_item_crc || !d_item_status || !d_status) { c->set_error("crc32: null pointer"); return TSQA_ERR_ARG; }
    if (flags != 0u) { c->set_error("crc32: unknown flags 0x%x", flags); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("crc32: the index belongs to device %d, the context to %d", idx->device, c->device); return TSQA_ERR_ARG; }
    // (the host sizes the blocks' table from the block count, which it does not have before the fetch)
    if (idx->pending_items != 0u) { c->set_error("crc32: %s", kNeedsFetch); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    const uint32_t n_blocks = idx->n_blocks, n_items = tsqa_index_items(idx);
    if (int rc = c->reserve_crc(n_blocks)) return rc;
    int32_t* const any = reinterpret_cast<int32_t*>(static_cast<uint32_t*>(c->crc_blocks));
    uint32_t* const block_r = c->crc_blocks + 1;
    const FrameInfo* const frames = idx->frames;
    const int32_t* const verdict = idx->verdict;
    const uint64_t* const item_first = idx->d_item_first;
    // the items' status words start as the index's own: zeros, but for the items it refused (which own no block)
    bool refused = false;
    for (size_t i = 0; i < idx->item_status.size() && i < n_items; ++i) refused = refused || idx->item_status[i] != 0;
    if (refused) {
        tsqa_uploads::Slot up;
        if (int rc = c->range_up.acquire(c, (size_t)n_items * sizeof(int32_t), &up)) return rc;
        for (uint32_t i = 0; i < n_items; ++i) up.host<int32_t>()[i] = i < idx->item_status.size() ? idx->item_status[i] : 0;
        TSQ_HIP(c, hipMemcpyAsync(d_item_status, up.host<int32_t>(), (size_t)n_items * sizeof(int32_t), hipMemcpyHostToDevice, s));
        TSQ_HIP(c, up.commit(s));
    } else {
        TSQ_HIP(c, hipMemsetAsync(d_item_status, 0, (size_t)n_items * sizeof(int32_t), s));
    }
    TSQ_HIP(c, hipMemsetAsync(d_item_crc, 0, (size_t)n_items * sizeof(uint32_t), s));
    if (d_all_crc) TSQ_HIP(c, hipMemsetAsync(d_all_crc, 0, sizeof(uint32_t), s));
    TSQ_HIP(c, hipMemsetAsync(c->crc_blocks, 0, ((size_t)n_blocks + 1) * sizeof(uint32_t), s));
    if (n_blocks != 0) {
        ProfSpan decode(c, 13, s);
        TSQ_RAISE_LDS(c, lds_need(dec_crc_kernel, CrcLds::total));
        hipLaunchKernelGGL(dec_crc_kernel, dim3(n_blocks), dim3(SymCfg::T), CrcLds::total, s, idx->container, frames, verdict, item_first, n_items, block_r,
                           d_item_status, any);
        decode.end();
    }
    ProfSpan fold(c, 14, s);
    const uint64_t lanes = std::max<uint64_t>(n_blocks, (uint64_t)n_items + 1u);
    hipLaunchKernelGGL(crc_fold_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, s, frames, n_blocks, idx->total, verdict, item_first, n_items,
                       static_cast<const uint32_t*>(block_r), static_cast<const int32_t*>(d_item_status), d_item_crc, d_block_crc, d_all_crc);
    hipLaunchKernelGGL(crc_close_kernel, dim3(std::max(1u, (uint32_t)(((uint64_t)n_items + 255u) / 256u))), dim3(256), 0, s, verdict, static_cast<const int32_t*>(any), n_items, d_item_status,
                       d_item_crc, d_all_crc, d_status);
    fold.end();
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_crc32(tsqa_ctx* c, const tsqa_index* idx, uint32_t flags, uint32_t* d_item_crc, int32_t* d_item_status, uint32_t* d_block_crc,
                          uint32_t* d_all_crc, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    if (int rc = tsqa_crc32_async(c, idx, flags, d_item_crc, d_item_status, d_block_crc, d_all_crc, d_status, s)) return rc;
    int32_t st = 0;
    TSQ_HIP(c, hipMemcpyAsync(&st, d_status, sizeof(st), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    return status_to_rc(c, st, "crc32");
}

// ---- gather into fixed-stride padded rows: the same ranges, row k at k * row_stride, the tails filled (tsq_rows.cuh) ----

// What keeps the sums of the rows' scans, and n_rows * row_stride itself, below 2^55.
static bool rows_sums_ok(uint32_t n_rows, uint64_t row_stride, uint32_t n_blocks)
{
    const unsigned __int128 limit = (unsigned __int128)1 << 55;
    return (unsigned __int128)n_rows * ((unsigned __int128)row_stride + 4096u) < limit && (unsigned __int128)n_rows * n_blocks < limit;
}

extern "C" int tsqa_plan_gather_rows(const uint64_t* out_start, uint32_t n_blocks, const uint64_t* item_first_block, uint32_t n_items,
                                     const uint32_t* items, const uint64_t* offsets, const uint64_t* lengths, uint32_t n_rows,
                                     uint64_t row_stride, uint32_t flags, uint32_t cap_pieces, uint64_t* row_lengths, int32_t* row_status,
                                     uint64_t* need, uint32_t* n_groups)
{
    if (!out_start || !item_first_block || !row_lengths || !row_status || !need || !n_groups || n_items == 0 || row_stride == 0 ||
        (flags & ~(uint32_t)TSQA_ROWS_TRUNCATE) || cap_pieces < 1) return TSQA_ERR_ARG;
    if (out_start[0] != 0 || item_first_block[0] != 0 || item_first_block[n_items] != n_blocks) return TSQA_ERR_ARG;
    for (uint32_t b = 0; b < n_blocks; ++b)
        if (out_start[b + 1] < out_start[b] || out_start[b + 1] - out_start[b] > kBlockSize) return TSQA_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (item_first_block[i + 1] < item_first_block[i]) return TSQA_ERR_ARG;
    if (!rows_sums_ok(n_rows, row_stride, n_blocks)) return TSQA_ERR_ARG;
    uint64_t pieces_at = 0, longest = 0;
    std::vector<uint32_t> touched;
    try {
        for (uint32_t k = 0; k < n_rows; ++k) {
            uint64_t base = 0, mine = out_start[n_blocks];
            const uint64_t offset = offsets ? offsets[k] : 0;
            bool ok = true;
            if (items) {
                ok = items[k] < n_items && item_first_block[items[k]] < item_first_block[items[k] + 1];
                if (ok) { base = out_start[item_first_block[items[k]]]; mine = out_start[item_first_block[items[k] + 1]] - base; }
            }
            ok = ok && (lengths ? lengths[k] <= mine && offset <= mine - lengths[k] : offset <= mine);
            const uint64_t accepted = !ok ? 0 : lengths ? lengths[k] : mine - offset;
            if (accepted > longest) longest = accepted;
            const bool too_long = accepted > row_stride && !(flags & TSQA_ROWS_TRUNCATE);
            const uint64_t len = !ok || too_long ? 0 : accepted < row_stride ? accepted : row_stride, a = base + offset, e = a + len;
            uint64_t first = 0, pieces = 0;
            if (len) {
                first = (uint64_t)(std::upper_bound(out_start, out_start + n_blocks + 1, a) - out_start) - 1;
                for (uint64_t b = first; b < n_blocks && out_start[b] < e; ++b) pieces += out_start[b + 1] > out_start[b];
            }
            const bool fits = ok && !too_long && pieces_at + pieces <= cap_pieces;
            row_status[k] = !ok ? TSQA_ERR_ARG : fits ? TSQA_OK : TSQA_ERR_OVERFLOW;
            row_lengths[k] = fits ? len : 0;
            if (fits && len)
                for (uint64_t b = first; b < n_blocks && out_start[b] < e; ++b)
                    if (out_start[b + 1] > out_start[b]) touched.push_back((uint32_t)b);
            pieces_at += pieces;
        }
        std::sort(touched.begin(), touched.end());
        *n_groups = (uint32_t)(std::unique(touched.begin(), touched.end()) - touched.begin());
    } catch (...) { return TSQA_ERR_ARG; }
    need[0] = pieces_at;
    need[1] = longest;
    return TSQA_OK;
}

extern "C" int tsqa_gather_rows_async(tsqa_ctx* c, const tsqa_index* idx, const uint32_t* d_items, const uint64_t* d_offsets, const uint64_t* d_lengths,
                                      uint32_t n_rows, uint64_t row_stride, uint32_t flags, int pad, uint32_t cap_pieces, void* d_out, size_t out_cap,
                                      uint64_t* d_row_lengths, int32_t* d_row_status, uint64_t* d_need, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!idx || !d_row_lengths || !d_row_status || !d_need || !d_status) { c->set_error("gather_rows: null pointer"); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("gather_rows: the index belongs to device %d, the context to %d", idx->device, c->device); return TSQA_ERR_ARG; }
    if (row_stride == 0) { c->set_error("gather_rows: row_stride of 0"); return TSQA_ERR_ARG; }
    if (cap_pieces < 1) { c->set_error("gather_rows: cap_pieces of 0"); return TSQA_ERR_ARG; }
    if (flags & ~(uint32_t)TSQA_ROWS_TRUNCATE) { c->set_error("gather_rows: unknown flags %#x", flags); return TSQA_ERR_ARG; }
    if (pad < -1 || pad > 255) { c->set_error("gather_rows: pad %d is neither a byte nor -1", pad); return TSQA_ERR_ARG; }
    // (a batch index made on the device and not fetched: cap_blocks descriptors, the total in its words)
    const bool live = idx->pending_items != 0u;
    const uint32_t n_blocks = live ? idx->cap_blocks : idx->n_blocks;
    if (!rows_sums_ok(n_rows, row_stride, n_blocks)) {
        c->set_error("gather_rows: %u rows of %llu B out of an index of %u blocks", n_rows, (unsigned long long)row_stride, n_blocks);
        return TSQA_ERR_ARG;
    }
    if (d_out && (uint64_t)out_cap < (uint64_t)n_rows * row_stride) {
        c->set_error("gather_rows: %u rows of %llu B need %llu B, out_cap is %zu", n_rows, (unsigned long long)row_stride,
                     (unsigned long long)((uint64_t)n_rows * row_stride), out_cap);
        return TSQA_ERR_ARG;
    }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    if (n_rows == 0) {
        TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
        TSQ_HIP(c, hipMemsetAsync(d_need, 0, 2 * sizeof(uint64_t), s));
        return TSQA_OK;
    }
    const uint32_t cap_groups = cap_pieces < n_blocks ? cap_pieces : n_blocks;
    if (int rc = c->reserve_gather(n_rows, cap_pieces, cap_groups ? cap_groups : 1)) return rc;
    GatherRange* const ranges = c->gather_ranges;
    GatherWords* const words = c->gather_words;
    RangeItem* const items = c->gather_items;
    RangeItem* const sorted = items + cap_pieces;
    uint64_t* const keys = c->gather_keys;
    uint32_t* const slots = c->gather_slots;
    BlockGroup* const groups = c->gather_groups;
    uint64_t* const places = c->gather_places;
    uint64_t* const row_groups = c->gather_row_groups;
    const uint32_t n_items = tsqa_index_items(idx), n_row_groups = (uint32_t)(((uint64_t)n_rows + kRowsGroup - 1u) / kRowsGroup);
    ProfSpan plan(c, 6, s);
    void (*const measure)(const FrameInfo*, uint32_t, uint64_t, uint32_t, const int32_t*, const uint64_t*, uint32_t, const uint32_t*, const uint64_t*,
                          const uint64_t*, uint32_t, uint64_t, uint32_t, GatherRange*, uint64_t*, int32_t*, const uint64_t*) =
        live ? rows_measure_kernel<true> : rows_measure_kernel<false>;
    hipLaunchKernelGGL(measure, dim3(n_row_groups), dim3(256), 0, s, static_cast<const FrameInfo*>(idx->frames), n_blocks, idx->total,
                       idx->block_shift, static_cast<const int32_t*>(idx->verdict), static_cast<const uint64_t*>(idx->d_item_first), n_items, d_items,
                       d_offsets, d_lengths, n_rows, row_stride, flags, ranges, d_row_lengths, d_row_status, static_cast<const uint64_t*>(idx->d_words));
    hipLaunchKernelGGL(rows_sum_kernel, dim3(n_row_groups), dim3(256), 0, s, ranges, n_rows, row_groups);
    hipLaunchKernelGGL(rows_scan_kernel, dim3(1), dim3(256), 0, s, row_groups, n_row_groups, d_need, words);
    hipLaunchKernelGGL(rows_place_kernel, dim3(n_row_groups), dim3(256), 0, s, ranges, n_rows, static_cast<const uint64_t*>(row_groups), row_stride,
                       cap_pieces, places, d_row_lengths, d_row_status, d_need, words);
    int rc = TSQA_OK;
    if (d_out && n_blocks) {
        const uint64_t lanes = n_rows > cap_pieces ? n_rows : cap_pieces, piece_groups = ((uint64_t)cap_pieces + 255u) / 256u;
        hipLaunchKernelGGL(gather_pieces_kernel, dim3((uint32_t)((lanes + 255u) / 256u)), dim3(256), 0, s, static_cast<const FrameInfo*>(idx->frames),
                           n_blocks, static_cast<const GatherRange*>(ranges), n_rows, static_cast<const int32_t*>(d_row_status),
                           static_cast<const uint64_t*>(places), static_cast<const GatherWords*>(words), cap_pieces, items, keys, slots);
        TSQ_HIP(c, gather_sort_pairs(c->gather_sort, c->gather_sort_bytes, keys, keys + cap_pieces, slots, slots + cap_pieces, cap_pieces, s));
        const uint64_t movers = piece_groups < 4ull * (uint64_t)c->n_cus ? piece_groups : 4ull * (uint64_t)c->n_cus;
        hipLaunchKernelGGL(gather_groups_kernel, dim3((uint32_t)(1u + movers)), dim3(256), 0, s, static_cast<const RangeItem*>(items),
                           static_cast<const uint64_t*>(keys + cap_pieces), static_cast<const uint32_t*>(slots + cap_pieces), words, cap_pieces,
                           sorted, groups, cap_groups);
        hipLaunchKernelGGL(gather_spans_kernel, dim3((cap_groups + 255u) / 256u), dim3(256), 0, s, static_cast<const RangeItem*>(sorted),
                           static_cast<const GatherWords*>(words), cap_pieces, groups, cap_groups);
        plan.end();
        ProfSpan dec(c, 7, s);
        rc = launch_read_kernel<dec_group_live_kernel>(c, cap_groups, s, idx->container, static_cast<const FrameInfo*>(idx->frames), n_blocks,
                                                       static_cast<const RangeItem*>(sorted), cap_pieces, static_cast<const BlockGroup*>(groups),
                                                       static_cast<uint8_t*>(d_out), &words->stream, static_cast<const uint32_t*>(&words->n_groups));
        dec.end();
    } else plan.end();
    if (d_out && pad >= 0) {
        // (the decoders write data bytes alone and the pad kernel pad bytes alone: neither order between them matters)
        const uint64_t n_words = ((uint64_t)n_rows * row_stride + 15u + 15u) >> 4, want = (n_words + 255u) / 256u;
        const uint64_t most = 16ull * (uint64_t)c->n_cus;
        ProfSpan span(c, 8, s);
        hipLaunchKernelGGL(rows_pad_kernel, dim3((uint32_t)(want < most ? want : most)), dim3(256), 0, s, static_cast<uint8_t*>(d_out), n_rows,
                           row_stride, static_cast<const uint64_t*>(d_row_lengths), (uint32_t)pad);
        span.end();
    }
    hipLaunchKernelGGL(gather_close_kernel, dim3(1), dim3(1), 0, s, static_cast<const GatherWords*>(words), d_status);
    if (rc) return rc;
    TSQ_HIP(c, hipGetLastError());
    return TSQA_OK;
}

extern "C" int tsqa_gather_rows(tsqa_ctx* c, const tsqa_index* idx, const uint32_t* d_items, const uint64_t* d_offsets, const uint64_t* d_lengths,
                                uint32_t n_rows, uint64_t row_stride, uint32_t flags, int pad, uint32_t cap_pieces, void* d_out, size_t out_cap,
                                uint64_t* d_row_lengths, int32_t* d_row_status, uint64_t* d_need, int32_t* d_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    hipStream_t s = stream_of(c, hip_stream);
    if (int rc = tsqa_gather_rows_async(c, idx, d_items, d_offsets, d_lengths, n_rows, row_stride, flags, pad, cap_pieces, d_out, out_cap,
                                        d_row_lengths, d_row_status, d_need, d_status, s)) return rc;
    int32_t st = 0;
    TSQ_HIP(c, hipMemcpyAsync(&st, d_status, sizeof(st), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    return status_to_rc(c, st, "gather_rows");
}

// The 16-byte headers of a batch's items, to the host with one gather kernel and one copy (and to c->batch_heads).  Waits for `s`.
static int gather_heads(tsqa_ctx* c, const void* d_in, const tsqa_batch_item* items, uint32_t n_items, hipStream_t s, std::vector<uint8_t>& heads)
{
    if (int rc = c->reserve_batch(n_items)) return rc;
    tsqa_uploads::Slot up;
    if (int rc = c->batch_up.acquire(c, (size_t)n_items * sizeof(BatchItem), &up)) return rc;
    BatchItem* const hi = up.host<BatchItem>();
    for (uint32_t i = 0; i < n_items; ++i) hi[i] = BatchItem{items[i].in_at, items[i].in_len, 0, 0, 0, 0, 0};    // (the kernel reads no more)
    heads.resize((size_t)n_items * kHeaderSize);
    TSQ_HIP(c, up.send((size_t)n_items * sizeof(BatchItem), s));
    hipLaunchKernelGGL(batch_heads_kernel, dim3((uint32_t)(((uint64_t)n_items * kHeaderSize + 255u) / 256u)), dim3(256), 0, s,
                       static_cast<const uint8_t*>(d_in), up.dev<BatchItem>(), n_items, c->batch_heads);
    TSQ_HIP(c, up.commit(s));
    TSQ_HIP(c, hipMemcpyAsync(heads.data(), c->batch_heads, heads.size(), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    return TSQA_OK;
}

// The synchronous form's decode of a (sub-)batch: the status lands in *st, the items' sizes in sizes[]; after TSQA_ERR_STALL once
// more with one workgroup per block.  The return value is a call error (nothing decoded) or TSQA_OK.
static int decompress_batch_wait(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, const uint32_t* n_blocks,
                                 uint32_t n_items, void* d_out, size_t out_size, uint64_t* sizes, int32_t* st, hipStream_t s)
{
    for (int variant : {-1, 4}) {
        if (int rc = decompress_batch_async_impl(c, d_in, in_size, items, n_blocks, n_items, d_out, out_size, c->batch_sizes, c->d_status, s, variant)) return rc;
        TSQ_HIP(c, hipMemcpyAsync(sizes, c->batch_sizes, (size_t)n_items * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (int rc = read_status(c, s, st)) return rc;
        if (*st != kErrStall) break;
    }
    return TSQA_OK;
}

extern "C" int tsqa_decompress_batch(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items,
                                     void* d_out, size_t out_size, uint64_t* sizes, int32_t* item_status, void* hip_stream)
{
    if (!c) return TSQA_ERR_ARG;
    if (!d_in || !d_out || !sizes) { c->set_error("decompress_batch: null pointer"); return TSQA_ERR_ARG; }
    const char* why;
    if (plan_batch(items, n_items, in_size, out_size, nullptr, nullptr, &why, kPlanRangesOnly)) { c->set_error("decompress_batch: %s", why); return TSQA_ERR_ARG; }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    std::vector<int32_t> own;
    if (!item_status) { own.resize(n_items); item_status = own.data(); }
    std::vector<uint8_t> heads;
    if (int rc = gather_heads(c, d_in, items, n_items, s, heads)) return rc;
    // items whose header is refused are reported and left out of the launch
    std::vector<tsqa_batch_item> ok_items;
    std::vector<uint32_t> ok_blocks, ok_index;
    for (uint32_t i = 0; i < n_items; ++i) {
        sizes[i] = 0;
        uint32_t nb = 0; uint64_t total = 0;
        if (read_header(&heads[(size_t)i * kHeaderSize], items[i].in_len, &nb, &total) != kHeaderOk) item_status[i] = TSQA_ERR_FORMAT;
        else if (total > items[i].out_cap) item_status[i] = TSQA_ERR_ARG;            // (as tsqa_decompress_device refuses it)
        else { item_status[i] = TSQA_OK; ok_items.push_back(items[i]); ok_blocks.push_back(nb); ok_index.push_back(i); }
    }
    if (!ok_items.empty()) {
        const uint32_t m = (uint32_t)ok_items.size();
        std::vector<uint64_t> got(m);
        int32_t st = 0;
        if (int rc = decompress_batch_wait(c, d_in, in_size, ok_items.data(), ok_blocks.data(), m, d_out, out_size, got.data(), &st, s)) return rc;
        if (st == 0) {
            for (uint32_t j = 0; j < m; ++j) sizes[ok_index[j]] = got[j];
        } else {
            // (the error path only) the same items once more with a status word each: the items at fault are found on the device, in
            // one launch, and every healthy item's bytes are delivered; sizes and statuses come back with one wait
            std::vector<int32_t> verdict(m);
            if (int rc = decompress_batch_items_async_impl(c, d_in, in_size, ok_items.data(), ok_blocks.data(), m, d_out, out_size, c->batch_sizes,
                                                           c->batch_status, c->d_status, s)) return rc;
            TSQ_HIP(c, hipMemcpyAsync(got.data(), c->batch_sizes, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            TSQ_HIP(c, hipMemcpyAsync(verdict.data(), c->batch_status, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            if (int rc = read_status(c, s, &st)) return rc;
            for (uint32_t j = 0; j < m; ++j) {
                item_status[ok_index[j]] = verdict[j];
                sizes[ok_index[j]] = verdict[j] ? 0 : got[j];
            }
        }
    }
    int32_t worst = TSQA_OK;
    uint32_t refused = 0;
    for (uint32_t i = 0; i < n_items; ++i) { worst = std::max(worst, item_status[i]); refused += item_status[i] != TSQA_OK; }
    if (worst) c->set_error("decompress_batch: %u of %u items refused (worst status %d)", refused, n_items, worst);
    return worst;
}

// ---- an index over a batch of containers (record reads: tsqa_decompress_item_ranges*) ----

// tsqa_index_create_batch behind its argument checks; a host allocation may throw.
static int index_create_batch(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items,
                              tsqa_index** out, int32_t* item_status)
{
    // the batch planner's checks of the input ranges (the output ranges of the items are not used)
    std::vector<tsqa_batch_item> plain;
    if (items && n_items) {
        plain.assign(items, items + n_items);
        for (tsqa_batch_item& x : plain) { x.out_at = 0; x.out_cap = 0; }
    }
    const char* why;
    if (plan_batch(plain.empty() ? nullptr : plain.data(), n_items, in_size, 0, nullptr, nullptr, &why, kPlanRangesOnly)) {
        c->set_error("index_create_batch: %s", why);
        return TSQA_ERR_ARG;
    }
    hipStream_t s = c->stream;
    (void)hipSetDevice(c->device);
    const uint8_t* const in = static_cast<const uint8_t*>(d_in);
    std::vector<uint8_t> heads;
    if (int rc = gather_heads(c, d_in, items, n_items, s, heads)) return rc;
    // the block counts the headers state (0: refused here), each item's first block, and its start in the concatenation of the data
    std::vector<uint32_t> nbs(n_items);
    std::vector<uint64_t> first((size_t)n_items + 1), verdicts(n_items);
    tsqa_uploads::Slot up;
    if (int rc = c->batch_up.acquire(c, (size_t)n_items * sizeof(BatchItem), &up)) return rc;
    BatchItem* const hi = up.host<BatchItem>();
    uint64_t blocks = 0, cat = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        uint32_t nb = 0; uint64_t total = 0;
        if (read_header(&heads[(size_t)i * kHeaderSize], items[i].in_len, &nb, &total) != kHeaderOk) { nb = 0; total = 0; }
        nbs[i] = nb; first[i] = blocks;
        hi[i] = BatchItem{items[i].in_at, items[i].in_len, cat, 0, blocks, nb, 0u};
        blocks += nb; cat += total;
    }
    first[n_items] = blocks;
    if (blocks > 0xFFFFFFFFull) { c->set_error("index_create_batch: more than 2^32 - 1 blocks"); return TSQA_ERR_ARG; }
    IndexPtr idx = index_begin(c, "index_create_batch", d_in, in_size, 0u, 0ull, false, false);
    if (!idx) return TSQA_ERR_ARG;
    std::vector<tsqa_frame> walked(blocks);
    // one frame walk over all items, one lane each, into the index's own descriptors; verdicts and descriptors come back together
    TSQ_HIP(c, hipMalloc(&idx->frames, (size_t)(blocks ? blocks : 1) * sizeof(FrameInfo)));
    TSQ_HIP(c, up.send((size_t)n_items * sizeof(BatchItem), s));
    hipLaunchKernelGGL(batch_walk_kernel<kWalkIndex>, dim3((n_items + 255u) / 256u), dim3(256), 0, s, in, up.dev<BatchItem>(), n_items, idx->frames,
                       (uint32_t*)nullptr, c->batch_sizes, (int32_t*)nullptr);
    TSQ_HIP(c, hipGetLastError());
    TSQ_HIP(c, up.commit(s));
    TSQ_HIP(c, hipMemcpyAsync(verdicts.data(), c->batch_sizes, (size_t)n_items * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (blocks) TSQ_HIP(c, hipMemcpyAsync(walked.data(), idx->frames, (size_t)blocks * sizeof(FrameInfo), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    // the healthy items' blocks, one after the other.  (An item whose header passed and whose frames did not leaves a gap in the
    // table the walk wrote: the table is closed up here and goes to the device once more.  Rare, and still a constant number of copies.)
    idx->item_first.resize((size_t)n_items + 1);
    idx->item_status.resize(n_items);
    bool gaps = false;
    uint64_t total = 0;
    int32_t worst = TSQA_OK;
    uint32_t refused = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        const bool ok = verdicts[i] != kItemRefused;
        idx->item_first[i] = idx->host_frames.size();
        idx->item_status[i] = ok ? TSQA_OK : TSQA_ERR_FORMAT;
        if (item_status) item_status[i] = idx->item_status[i];
        if (!ok) { gaps |= nbs[i] != 0u; refused++; worst = TSQA_ERR_FORMAT; continue; }
        for (uint64_t b = first[i]; b < first[i + 1]; ++b) {
            tsqa_frame f = walked[b];
            f.out_at = total;
            idx->out_start.push_back(total);
            idx->host_frames.push_back(f);
            total += f.out_len;
        }
    }
    idx->item_first[n_items] = idx->host_frames.size();
    idx->out_start.push_back(total);
    idx->n_blocks = (uint32_t)idx->host_frames.size();
    idx->total = total;
    if (gaps && idx->n_blocks) {
        const hipError_t e = hipMemcpy(idx->frames, idx->host_frames.data(), (size_t)idx->n_blocks * sizeof(FrameInfo), hipMemcpyHostToDevice);
        if (e != hipSuccess) { c->set_error("index_create_batch: hipMemcpy failed: %s", hipGetErrorString(e)); return TSQA_ERR_HIP; }
    }
    // each item's first block, for the reads that name their items in device memory (tsqa_gather_async)
    TSQ_HIP(c, hipMalloc(&idx->d_item_first, ((size_t)n_items + 1) * sizeof(uint64_t)));
    TSQ_HIP(c, hipMemcpy(idx->d_item_first, idx->item_first.data(), ((size_t)n_items + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
    if (worst) c->set_error("index_create_batch: %u of %u items refused", refused, n_items);
    *out = idx.release();
    return worst;
}

extern "C" int tsqa_index_create_batch(tsqa_ctx* c, const void* d_in, size_t in_size, const tsqa_batch_item* items, uint32_t n_items,
                                       tsqa_index** out, int32_t* item_status)
{
    if (!out) return TSQA_ERR_ARG;
    *out = nullptr;
    if (!c) return TSQA_ERR_ARG;
    if (!d_in) { c->set_error("index_create_batch: null pointer"); return TSQA_ERR_ARG; }
    // (the block counts come from the containers' own headers: the host tables may be refused by the allocator)
    try { return index_create_batch(c, d_in, in_size, items, n_items, out, item_status); }
    catch (...) { c->set_error("index_create_batch: out of host memory"); return TSQA_ERR_ARG; }
}

// ---- the index of a packed batch from its device tables, with no host wait (tsq_index_packed.cuh) ----

extern "C" int tsqa_plan_index_packed(const uint32_t* blocks, const uint64_t* totals, const int32_t* head_status, const int32_t* walk_status,
                                      uint32_t n_items, uint32_t cap_blocks, uint64_t* item_first, uint64_t* item_at, int32_t* item_status,
                                      uint64_t* blocks_total, int32_t* status)
{
    if (!blocks || !totals || !head_status || !walk_status || !item_first || !item_at || !item_status || !blocks_total || !status ||
        n_items == 0 || cap_blocks == 0) return TSQA_ERR_ARG;
    for (uint32_t i = 0; i < n_items; ++i)
        if (head_status[i] == TSQA_OK && (blocks[i] == 0 || totals[i] > (uint64_t)blocks[i] * kBlockSize)) return TSQA_ERR_ARG;
    uint64_t accepted = 0, fb = 0, at = 0;
    bool open = true;                                        // no accepted item has failed to fit yet
    int32_t worst = TSQA_OK;
    for (uint32_t i = 0; i < n_items; ++i) {
        int32_t st = head_status[i];
        const uint64_t nb = st == TSQA_OK ? blocks[i] : 0;
        if (st == TSQA_OK && (!open || accepted + nb > cap_blocks)) { open = false; st = TSQA_ERR_OVERFLOW; }
        accepted += nb;
        if (st == TSQA_OK && walk_status[i] != TSQA_OK) st = walk_status[i];
        item_first[i] = fb; item_at[i] = at; item_status[i] = st;
        if (st == TSQA_OK) { fb += nb; at += totals[i]; }
        worst = std::max(worst, st);
    }
    item_first[n_items] = fb;
    blocks_total[0] = fb; blocks_total[1] = at; blocks_total[2] = accepted;
    *status = worst;
    return TSQA_OK;
}

extern "C" int tsqa_index_create_packed_async(tsqa_ctx* c, const void* d_arena, size_t arena_size, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                              uint32_t n_items, uint32_t cap_blocks, uint32_t block_len, const uint64_t* d_table_first,
                                              const uint32_t* d_block_sizes, uint64_t table_words, tsqa_index** out, int32_t* d_item_status,
                                              int32_t* d_status, void* hip_stream)
{
    if (!out) return TSQA_ERR_ARG;
    *out = nullptr;
    if (!c) return TSQA_ERR_ARG;
    if (!d_arena || !d_offsets || !d_sizes || !d_status) { c->set_error("index_create_packed: null pointer"); return TSQA_ERR_ARG; }
    if (n_items == 0) { c->set_error("index_create_packed: no items"); return TSQA_ERR_ARG; }
    if (cap_blocks == 0) { c->set_error("index_create_packed: cap_blocks is 0"); return TSQA_ERR_ARG; }
    const bool sized = d_block_sizes != nullptr;
    if (!sized && (block_len != 0 || d_table_first || table_words != 0)) {
        c->set_error("index_create_packed: the plain form (no d_block_sizes) takes block_len 0, no d_table_first and table_words 0");
        return TSQA_ERR_ARG;
    }
    if (sized) {
        uint32_t nb = 0;
        size_t bound = 0;
        if (!d_table_first) { c->set_error("index_create_packed: null d_table_first"); return TSQA_ERR_ARG; }
        if (tsqa_plan_split(1, block_len, &nb, &bound)) { c->set_error("index_create_packed: block_len %u is no power of two from 2^12 to 2^22", block_len); return TSQA_ERR_ARG; }
    }
    hipStream_t s = stream_of(c, hip_stream);
    (void)hipSetDevice(c->device);
    if (int rc = c->reserve_batch(n_items)) return rc;
    if (int rc = c->reserve(cap_blocks, false, false, true)) return rc;
    c->forget_sharded();                                 // the walk below overwrites c->frames
    IndexPtr idx = index_begin(c, "index_create_packed", d_arena, arena_size, 0u, 0ull, false, false);
    if (!idx) return TSQA_ERR_ARG;
    idx->cap_blocks = cap_blocks; idx->pending_items = n_items; idx->packed_block_len = block_len;
    // two allocations, the two that tsqa_index_destroy frees: the descriptors; and item_first (n_items + 1), item_at (n_items), the
    // words, the sized walk's group sums, the item statuses
    const uint32_t n_groups = sized ? (uint32_t)(((uint64_t)cap_blocks + kPidxGroup - 1u) / kPidxGroup) : 0u;
    const size_t n_u64 = 2 * (size_t)n_items + 1 + kPidxWords + n_groups;
    TSQ_HIP(c, hipMalloc(&idx->frames, (size_t)cap_blocks * sizeof(FrameInfo)));
    TSQ_HIP(c, hipMalloc(&idx->d_item_first, n_u64 * sizeof(uint64_t) + (size_t)n_items * sizeof(int32_t)));
    idx->d_item_at = idx->d_item_first + n_items + 1;
    idx->d_words = idx->d_item_at + n_items;
    uint64_t* const group_sum = idx->d_words + kPidxWords;
    idx->d_item_status = reinterpret_cast<int32_t*>(idx->d_item_first + n_u64);
    const uint8_t* const in = static_cast<const uint8_t*>(d_arena);
    BatchItem* const items = c->batch_items;
    uint64_t* const first_block = c->batch_offsets;      // the provisional places: the prefix over every item whose header passed
    const dim3 per_item((uint32_t)(((uint64_t)n_items + 255u) / 256u)), per_block((uint32_t)(((uint64_t)cap_blocks + 255u) / 256u));
    TSQ_HIP(c, hipMemsetAsync(d_status, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(batch_measure_kernel, per_item, dim3(256), 0, s, in, items, n_items, d_offsets, d_sizes, (uint64_t)arena_size, idx->d_item_status);
    if (sized)
        hipLaunchKernelGGL(pidx_tables_kernel, per_item, dim3(256), 0, s, items, n_items, block_len, d_table_first, table_words, idx->d_item_status);
    hipLaunchKernelGGL(join_blocks_kernel, dim3(1), dim3(256), 0, s, items, n_items, cap_blocks, first_block, idx->d_item_status);
    if (sized) {
        hipLaunchKernelGGL(pidx_sum_kernel, dim3(n_groups), dim3(256), 0, s, static_cast<const BatchItem*>(items), n_items,
                           static_cast<const uint64_t*>(first_block), cap_blocks, d_block_sizes, c->block_owner, group_sum);
        hipLaunchKernelGGL(pidx_scan_kernel, dim3(1), dim3(256), 0, s, group_sum, n_groups);
        hipLaunchKernelGGL(pidx_place_kernel, dim3(n_groups), dim3(256), 0, s, static_cast<const BatchItem*>(items),
                           static_cast<const uint32_t*>(c->block_owner), cap_blocks, d_block_sizes, static_cast<const uint64_t*>(group_sum), c->frame_at);
        hipLaunchKernelGGL(pidx_check_kernel, per_block, dim3(256), 0, s, in, static_cast<const BatchItem*>(items),
                           static_cast<const uint32_t*>(c->block_owner), cap_blocks, block_len, d_block_sizes,
                           static_cast<const uint64_t*>(c->frame_at), c->frames, idx->d_item_status);
    } else {
        hipLaunchKernelGGL(batch_walk_kernel<kWalkIndex>, per_item, dim3(256), 0, s, in, static_cast<const BatchItem*>(items), n_items, c->frames,
                           (uint32_t*)nullptr, c->batch_sizes, (int32_t*)nullptr);
    }
    hipLaunchKernelGGL(pidx_close_kernel, dim3(1), dim3(256), 0, s, static_cast<const BatchItem*>(items), n_items,
                       sized ? (const uint64_t*)nullptr : static_cast<const uint64_t*>(c->batch_sizes), static_cast<const uint64_t*>(first_block),
                       idx->d_item_status, d_item_status, idx->d_item_first, idx->d_item_at, idx->d_words, d_status);
    hipLaunchKernelGGL(pidx_move_kernel, per_block, dim3(256), 0, s, static_cast<const BatchItem*>(items), n_items,
                       static_cast<const FrameInfo*>(c->frames), static_cast<const uint64_t*>(idx->d_item_first),
                       static_cast<const uint64_t*>(idx->d_item_at), static_cast<const uint64_t*>(idx->d_words), cap_blocks, idx->frames);
    TSQ_HIP(c, hipGetLastError());
    *out = idx.release();
    return TSQA_OK;
}

// tsqa_index_fetch behind its argument checks; a host allocation may throw.
static int index_fetch(tsqa_ctx* c, tsqa_index* idx, hipStream_t s)
{
    const uint32_t n_items = idx->pending_items;
    std::vector<uint64_t> first((size_t)n_items + 1);
    std::vector<int32_t> status(n_items);
    uint64_t words[kPidxWords] = {0, 0, 0};
    TSQ_HIP(c, hipMemcpyAsync(first.data(), idx->d_item_first, first.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipMemcpyAsync(status.data(), idx->d_item_status, status.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipMemcpyAsync(words, idx->d_words, sizeof(words), hipMemcpyDeviceToHost, s));
    TSQ_HIP(c, hipStreamSynchronize(s));
    const uint64_t live = words[0];
    if (live > idx->cap_blocks || first[n_items] != live) { c->set_error("index_fetch: the device tables are not an index's (was the creation enqueued on this stream?)"); return TSQA_ERR_ARG; }
    std::vector<tsqa_frame> frames(live);
    std::vector<uint64_t> out_start(live + 1);
    if (live) {
        TSQ_HIP(c, hipMemcpyAsync(frames.data(), idx->frames, (size_t)live * sizeof(FrameInfo), hipMemcpyDeviceToHost, s));
        TSQ_HIP(c, hipStreamSynchronize(s));
    }
    for (uint64_t b = 0; b < live; ++b) out_start[b] = frames[b].out_at;
    out_start[live] = words[1];
    idx->host_frames.swap(frames); idx->out_start.swap(out_start); idx->item_first.swap(first); idx->item_status.swap(status);
    idx->n_blocks = (uint32_t)live; idx->total = words[1];
    idx->pending_items = 0;
    return TSQA_OK;
}

extern "C" int tsqa_index_fetch(tsqa_ctx* c, tsqa_index* idx, void* hip_stream)
{
    static_assert(sizeof(tsqa_frame) == sizeof(FrameInfo), "public frame = kernel frame");
    if (!c) return TSQA_ERR_ARG;
    if (!idx) { c->set_error("index_fetch: null index"); return TSQA_ERR_ARG; }
    if (idx->device != c->device) { c->set_error("index_fetch: the index belongs to device %d, the context to %d", idx->device, c->device); return TSQA_ERR_ARG; }
    if (!idx->pending_items) return TSQA_OK;             // the host has its tables already
    (void)hipSetDevice(c->device);
    try { return index_fetch(c, idx, stream_of(c, hip_stream)); }
    catch (...) { c->set_error("index_fetch: out of host memory"); return TSQA_ERR_ARG; }
}

extern "C" int tsqa_index_device_tables(const tsqa_index* idx, const uint64_t** d_item_first, const int32_t** d_item_status, const uint64_t** d_blocks_total)
{
    const bool made = idx && idx->d_words;
    if (d_item_first) *d_item_first = made ? idx->d_item_first : nullptr;
    if (d_item_status) *d_item_status = made ? idx->d_item_status : nullptr;
    if (d_blocks_total) *d_blocks_total = made ? idx->d_words : nullptr;
    return made ? TSQA_OK : TSQA_ERR_ARG;
}

extern "C" int tsqa_index_create_packed(tsqa_ctx* c, const void* d_arena, size_t arena_size, const uint64_t* d_offsets, const uint64_t* d_sizes,
                                        uint32_t n_items, uint32_t cap_blocks, uint32_t block_len, const uint64_t* d_table_first,
                                        const uint32_t* d_block_sizes, uint64_t table_words, tsqa_index** out, int32_t* item_status, void* hip_stream)
{
    if (!out) return TSQA_ERR_ARG;
    *out = nullptr;
    if (!c) return TSQA_ERR_ARG;
    tsqa_index* made = nullptr;
    hipStream_t s = stream_of(c, hip_stream);
    if (int rc = tsqa_index_create_packed_async(c, d_arena, arena_size, d_offsets, d_sizes, n_items, cap_blocks, block_len, d_table_first,
                                                d_block_sizes, table_words, &made, nullptr, c->d_status, s)) return rc;
    IndexPtr idx(made);
    if (int rc = tsqa_index_fetch(c, idx.get(), s)) return rc;
    int32_t worst = TSQA_OK;
    uint32_t refused = 0;
    for (uint32_t i = 0; i < n_items; ++i) {
        const int32_t st = idx->item_status[i];
        if (item_status) item_status[i] = st;
        worst = std::max(worst, st); refused += st != TSQA_OK;
    }
    if (worst) c->set_error("index_create_packed: %u of %u items refused (worst status %d)", refused, n_items, worst);
    *out = idx.release();
    return worst;
}

// ---- the second roofline denominator: what a plain device copy reaches on this GPU ----
// MODE 0: grid-stride, four independent 16-byte loads in flight per lane; 1: the same with non-temporal loads and stores;
// 2: one pass, every thread moves four words 256 apart (no loop: as many workgroups as the buffer needs).
typedef uint32_t probe_u32x4 __attribute__((ext_vector_type(4)));
template <int MODE>
__global__ __launch_bounds__(256) void copy_probe_kernel(const probe_u32x4* __restrict__ src, probe_u32x4* __restrict__ dst, size_t words)
{
    if (MODE == 2) {
        const size_t i = (size_t)blockIdx.x * 1024u + threadIdx.x;
        if (i + 768u < words) {
            const probe_u32x4 a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + 256), c = __builtin_nontemporal_load(src + i + 512),
                                d = __builtin_nontemporal_load(src + i + 768);
            __builtin_nontemporal_store(a, dst + i); __builtin_nontemporal_store(b, dst + i + 256);
            __builtin_nontemporal_store(c, dst + i + 512); __builtin_nontemporal_store(d, dst + i + 768);
        } else for (size_t k = i; k < words && k < i + 1024u; k += 256u) dst[k] = src[k];
        return;
    }
    const size_t step = (size_t)gridDim.x * 256u;
    size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    for (; i + 3 * step < words; i += 4 * step) {
        if (MODE == 1) {
            const probe_u32x4 a = __builtin_nontemporal_load(src + i), b = __builtin_nontemporal_load(src + i + step), c = __builtin_nontemporal_load(src + i + 2 * step),
                                d = __builtin_nontemporal_load(src + i + 3 * step);
            __builtin_nontemporal_store(a, dst + i); __builtin_nontemporal_store(b, dst + i + step);
            __builtin_nontemporal_store(c, dst + i + 2 * step); __builtin_nontemporal_store(d, dst + i + 3 * step);
        } else {
            const probe_u32x4 a = src[i], b = src[i + step], c = src[i + 2 * step], d = src[i + 3 * step];
            dst[i] = a; dst[i + step] = b; dst[i + 2 * step] = c; dst[i + 3 * step] = d;
        }
    }
    for (; i < words; i += step) dst[i] = src[i];
}

extern "C" int tsqa_measure_copy(tsqa_ctx* c, size_t bytes, int reps, double* best_gbps, double* median_gbps)
{
    if (!c || bytes < (size_t(1) << 20) || reps < 1 || reps > 64) return TSQA_ERR_ARG;
    (void)hipSetDevice(c->device);
    probe_u32x4 *a = nullptr, *b = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const size_t words = bytes / 16;
    int rc = TSQA_OK;
    double rates[64];
    if (hipMalloc(&a, words * 16) != hipSuccess || hipMalloc(&b, words * 16) != hipSuccess ||
        hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess ||
        hipMemsetAsync(a, 0x5a, words * 16, c->stream) != hipSuccess) rc = TSQA_ERR_HIP;
    // the shape that copies fastest is found first -- grid-stride kernels with 8, 16, 32 or 64 workgroups of 256 per CU, with default
    // and with non-temporal accesses, and the one-pass kernel -- then measured `reps` times
    uint32_t grid = (uint32_t)c->n_cus * 8u;
    int mode = 0;
    auto launch = [&](int m, uint32_t g) {
        if (m == 0) hipLaunchKernelGGL(copy_probe_kernel<0>, dim3(g), dim3(256), 0, c->stream, a, b, words);
        else if (m == 1) hipLaunchKernelGGL(copy_probe_kernel<1>, dim3(g), dim3(256), 0, c->stream, a, b, words);
        else hipLaunchKernelGGL(copy_probe_kernel<2>, dim3((uint32_t)((words + 1023u) / 1024u)), dim3(256), 0, c->stream, a, b, words);
    };
    {
        float best_ms = 1e30f;
        for (int m = 0; m < 3 && rc == TSQA_OK; ++m)
            for (uint32_t per_cu = 8; per_cu <= (m == 2 ? 8u : 64u) && rc == TSQA_OK; per_cu *= 2) {
                const uint32_t g = (uint32_t)c->n_cus * per_cu;
                float ms = 1e30f;
                for (int k = 0; k < 2; ++k) {
                    (void)hipEventRecord(e0, c->stream);
                    launch(m, g);
                    (void)hipEventRecord(e1, c->stream);
                    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) { rc = TSQA_ERR_HIP; break; }
                }
                if (ms < best_ms) { best_ms = ms; grid = g; mode = m; }
            }
    }
    for (int r = -1; r < reps && rc == TSQA_OK; ++r) {          // r == -1 warms up
        (void)hipEventRecord(e0, c->stream);
        launch(mode, grid);
        (void)hipEventRecord(e1, c->stream);
        float ms = 0;
        if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || ms <= 0) { rc = TSQA_ERR_HIP; break; }
        if (r >= 0) rates[r] = 2.0 * (double)(words * 16) / (ms * 1e-3) / 1e9;    // bytes read + bytes written
    }
    if (rc == TSQA_OK) {
        for (int i = 1; i < reps; ++i) for (int j = i; j > 0 && rates[j] < rates[j - 1]; --j) { double t = rates[j]; rates[j] = rates[j - 1]; rates[j - 1] = t; }
        if (best_gbps) *best_gbps = rates[reps - 1];
        if (median_gbps) *median_gbps = rates[reps / 2];
        snprintf(c->probe_shape, sizeof(c->probe_shape), "copy probe: mode %d (0 grid-stride, 1 grid-stride non-temporal, 2 one pass non-temporal), %u workgroups", mode, mode == 2 ? (uint32_t)((words + 1023u) / 1024u) : grid);
    } else c->set_error("copy probe failed");
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(a); (void)hipFree(b);
    return rc;
}

extern "C" const char* tsqa_copy_probe_shape(const tsqa_ctx* c) { return c ? c->probe_shape : ""; }

#ifdef TSQ_SPINS
extern "C" int tsqa_debug_spins(uint32_t* out16)
{
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(tsq::g_enc_spins), 20 * sizeof(uint32_t)) == hipSuccess ? TSQA_OK : TSQA_ERR_HIP;
}
#endif
#if defined(TSQ_STATS) || defined(TSQ_TRACEONLY)
extern "C" int tsqa_debug_trace(uint32_t* out4096)
{
    return hipMemcpyFromSymbol(out4096, HIP_SYMBOL(tsq::g_enc_trace), 4096 * sizeof(uint32_t)) == hipSuccess ? TSQA_OK : TSQA_ERR_HIP;
}
#endif
#ifdef TSQ_STATS
// instrumented builds only: counters published by block 0 of the last encode / decode launch
extern "C" int tsqa_debug_stats(unsigned long long* enc64, unsigned long long* dec16)
{
    if (enc64 && hipMemcpyFromSymbol(enc64, HIP_SYMBOL(tsq::g_enc_stats), 64 * sizeof(unsigned long long)) != hipSuccess) return TSQA_ERR_HIP;
    if (dec16 && hipMemcpyFromSymbol(dec16, HIP_SYMBOL(tsq::g_dec_stats), 16 * sizeof(unsigned long long)) != hipSuccess) return TSQA_ERR_HIP;
    return TSQA_OK;
}
extern "C" int tsqa_debug_dec_waves(unsigned long long* out48)
{
    return hipMemcpyFromSymbol(out48, HIP_SYMBOL(tsq::g_dec_wave), 48 * sizeof(unsigned long long)) == hipSuccess ? TSQA_OK : TSQA_ERR_HIP;
}
extern "C" int tsqa_debug_duo_xcc(uint32_t* out2048)
{
    return hipMemcpyFromSymbol(out2048, HIP_SYMBOL(tsq::g_duo_xcc), 2048 * sizeof(uint32_t)) == hipSuccess ? TSQA_OK : TSQA_ERR_HIP;
}
extern "C" int tsqa_debug_syms(uint32_t* out8192)
{
    return hipMemcpyFromSymbol(out8192, HIP_SYMBOL(tsq::g_dbg_syms), 8192 * sizeof(uint32_t)) == hipSuccess ? TSQA_OK : TSQA_ERR_HIP;
}
#endif
