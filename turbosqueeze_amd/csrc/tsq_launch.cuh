// tsq_launch.cuh -- kernel selection and launch for the device context.
//
// The product library carries three kernel families: the staged encoder (tsq_enc_stage.cuh: fourteen working wavefronts per block, twelve in the lean layout; standard and lean
// layouts, with and without extensions), the byte-lane decoder (tsq_dec_sym.cuh, tsq_dec_duo.cuh; their phases in tsq_dec_common.cuh) and the serial correctness
// baselines (tsq_serial.cuh, variant 1).  The previous round's production encoder (ab/tsq_enc_stage_r05.cuh, encoder variant 5) is
// compiled only into the A/B library (`make ab`, -DTSQ_AB_VARIANTS), which tests/test_gpu_parity.py holds against the same oracle.
#pragma once

#include <atomic>
#include <initializer_list>

#include "tsq_common.cuh"
#include "tsq_emit.cuh"
#include "tsq_internal.h"
#include "tsq_serial.cuh"
#include "tsq_dec_sym.cuh"
#include "tsq_dec_duo.cuh"
#include "tsq_enc_stage.cuh"
#ifdef TSQ_AB_VARIANTS
#include "ab/tsq_enc_stage_r05.cuh"
#endif

namespace tsq {

// The dynamic-LDS limit is a per-device attribute of a kernel function: raised once per device the process uses (`done`: the devices
// that have it).  TSQ_RAISE_LDS(c, lds_need(kernel, bytes), ...) is that for the kernels of one launcher, which it leaves on a failure.
struct LdsNeed { const void* fn; uint32_t bytes; };
template <class K> inline LdsNeed lds_need(K kernel, uint32_t bytes) { return {reinterpret_cast<const void*>(kernel), bytes}; }
inline int raise_lds_limit(tsqa_ctx* c, std::atomic<uint64_t>& done, std::initializer_list<LdsNeed> needs)
{
    const uint64_t dev_bit = 1ull << (c->device & 63);
    if (done.load() & dev_bit) return 0;
    for (const LdsNeed& k : needs)
        if (hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes) != hipSuccess) {
            c->set_error("cannot reserve %u B of LDS", k.bytes);
            return TSQA_ERR_HIP;
        }
    done.fetch_or(dev_bit);
    return 0;
}
#define TSQ_RAISE_LDS(c, ...)                                                                                                       \
    do {                                                                                                                            \
        static std::atomic<uint64_t> raised_{0};                                                                                    \
        if (int rc_ = raise_lds_limit((c), raised_, {__VA_ARGS__})) return rc_;                                                     \
    } while (0)

// One generation of the staged encoder in one role: its four builds in the order <ext, standard>, <plain, standard>, <ext, lean>,
// <plain, lean>, and the workgroup size and LDS of its two layouts ([0] standard, [1] lean).
template <class K> struct StagedFamily { K kernel[4]; uint32_t threads[2], lds[2]; std::atomic<uint64_t> raised{0}; };
#define TSQ_STAGED_FAMILY(KERNEL, CFG)                                                                                              \
    {{KERNEL<true, true>, KERNEL<false, true>, KERNEL<true, false>, KERNEL<false, false>}, {CFG<true>::THREADS, CFG<false>::THREADS_LEAN}, {CFG<true>::total, CFG<false>::total}}

// The staged pipeline (tsq_enc_stage.cuh) over nb blocks, one workgroup each.  More blocks than CUs: the lean layout (no input window
// in LDS, candidate bytes from L2) lets several blocks share a CU; each is a little slower, together they are faster.  Variant 6
// takes the lean layout at any count, variants 0 and 5 (the frozen generation) by the count, every other one the standard layout.
// (`args` by reference: a scratch buffer of the context, which cannot be copied, becomes its pointer at the launch.)
template <class K, class... Args>
inline int launch_staged(tsqa_ctx* c, StagedFamily<K>& f, uint32_t ext, uint32_t nb, hipStream_t s, const Args&... args)
{
    if (int rc = raise_lds_limit(c, f.raised, {lds_need(f.kernel[0], f.lds[0]), lds_need(f.kernel[1], f.lds[0]), lds_need(f.kernel[2], f.lds[1]), lds_need(f.kernel[3], f.lds[1])})) return rc;
    const int v = c->enc_variant;
    const int lean = v == 6 || ((v == 0 || v == 5) && nb > (uint32_t)c->n_cus);
    hipLaunchKernelGGL(f.kernel[2 * lean + (ext ? 0 : 1)], dim3(nb), dim3(f.threads[lean]), f.lds[lean], s, args...);
    return 0;
}

// Encode nb = ceil(n / 4 MiB) blocks; block b is read at in + b * stride, streams land in slots[b], sizes in sizes[b].
inline int launch_encode_kernels(tsqa_ctx* c, const uint8_t* in, size_t n, size_t readable, size_t stride, uint32_t ext,
                                 uint8_t* slots, uint32_t* sizes, int32_t* status, hipStream_t s)
{
    const uint32_t nb = (uint32_t)((n + kBlockSize - 1) / kBlockSize);
    static StagedFamily<decltype(&enc_stage_kernel<true, true>)> staged = TSQ_STAGED_FAMILY(enc_stage_kernel, StageCfgT);
    const int v = c->enc_variant;
    if (v == 1) {                       // one lane walks the block: the correctness baseline
        hipLaunchKernelGGL(ext ? enc_serial_kernel<true> : enc_serial_kernel<false>, dim3(nb), dim3(64), 0, s, in, (uint64_t)n, (uint64_t)readable,
                           (uint64_t)stride, slots, sizes, c->tables, status);
        return 0;
    }
#ifdef TSQ_AB_VARIANTS
    if (v == 5) {                       // round 5's production encoder, frozen (ab/tsq_enc_stage_r05.cuh)
        static StagedFamily<decltype(&r05::enc_stage_kernel<true, true>)> frozen = TSQ_STAGED_FAMILY(r05::enc_stage_kernel, r05::StageCfgT);
        return launch_staged(c, frozen, ext, nb, s, in, (uint64_t)n, (uint64_t)readable, (uint64_t)stride, slots, sizes, c->tables, status);
    }
#else
    if (v == 5) { c->set_error("kernel variant %d lives in the A/B library only (make ab)", v); return TSQA_ERR_ARG; }
#endif
    if (v >= 2 && v <= 4) { c->set_error("kernel variant %d is not built", v); return TSQA_ERR_ARG; }
    return launch_staged(c, staged, ext, nb, s, in, (uint64_t)n, (uint64_t)readable, (uint64_t)stride, slots, sizes, c->tables, status);
}

// Encode nb blocks of a batch (tsqa_compress_batch_async) from their descriptors: the staged encoder in the layout
// launch_encode_kernels takes for nb blocks.  Encoder variants 0, 6 and 7 only.  live_blocks != NULL: descriptors made on the device
// (blocks[0] is block b0 of the batch): enc_batch_live_kernel, whose workgroups at or past *live_blocks leave at once; the layout
// follows nb all the same.
inline int launch_batch_encode_kernels(tsqa_ctx* c, const uint8_t* in, const EncBatchBlock* blocks, uint32_t nb, uint32_t ext,
                                       uint8_t* slots, uint32_t* sizes, int32_t* status, hipStream_t s, uint32_t b0 = 0u,
                                       const uint32_t* live_blocks = nullptr)
{
    static StagedFamily<decltype(&enc_batch_kernel<true, true>)> staged = TSQ_STAGED_FAMILY(enc_batch_kernel, StageCfgT);
    static StagedFamily<decltype(&enc_batch_live_kernel<true, true>)> staged_live = TSQ_STAGED_FAMILY(enc_batch_live_kernel, StageCfgT);
    const int v = c->enc_variant;
    if (v != 0 && v != 6 && v != 7) { c->set_error("kernel variant %d does not encode batches (0, 6 and 7 do)", v); return TSQA_ERR_ARG; }
    if (live_blocks) return launch_staged(c, staged_live, ext, nb, s, in, blocks, slots, sizes, c->tables, status, b0, live_blocks);
    return launch_staged(c, staged, ext, nb, s, in, blocks, slots, sizes, c->tables, status);
}

inline int launch_decode_kernels(tsqa_ctx* c, const uint8_t* container, const FrameInfo* frames, uint32_t n_blocks, uint8_t* out,
                                 int32_t* status, hipStream_t s, int variant = -1)
{
    TSQ_RAISE_LDS(c, lds_need(dec_sym_kernel, SymLds::total));
    const int v = variant >= 0 ? variant : c->dec_variant;
    if (v == 1) { hipLaunchKernelGGL(dec_serial_kernel, dim3(n_blocks), dim3(64), 0, s, container, frames, out, status); return 0; }
    if (v == 8 || v == 9) { c->set_error("kernel variant %d is not built", v); return TSQA_ERR_ARG; }
    // Few blocks (every GPU of a multi-GPU job on enwik9): several workgroups per block on different CUs of one XCD -- the block's
    // copy chain on one, its parse on one (at most half as many blocks as CUs) or two (at most a third) (tsq_dec_duo.cuh).
    auto launch_multi = [&](const FrameInfo* fr, uint32_t nblk, bool three) -> int {
        const uint32_t lds_bytes = DuoCopyLds::total > SymLds::total ? DuoCopyLds::total : SymLds::total;
        TSQ_RAISE_LDS(c, lds_need(dec_duo_kernel<1>, lds_bytes), lds_need(dec_duo_kernel<2>, lds_bytes));
        if (int rc = c->reserve_duo(nblk, s)) return rc;
        if (hipMemsetAsync(c->duo_flags, 0, (size_t)nblk * DuoCfg::FLAG_STRIDE * sizeof(uint32_t), s) != hipSuccess) { c->set_error("hipMemsetAsync failed"); return TSQA_ERR_HIP; }
        const uint32_t groups = (nblk + 7u) / 8u;
        if (three) hipLaunchKernelGGL(dec_duo_kernel<2>, dim3(24u * groups), dim3(SymCfg::T), lds_bytes, s, container, fr, nblk, out, status, c->duo_ring, c->duo_flags, c->decode_wait_limit);
        else hipLaunchKernelGGL(dec_duo_kernel<1>, dim3(16u * groups), dim3(SymCfg::T), lds_bytes, s, container, fr, nblk, out, status, c->duo_ring, c->duo_flags, c->decode_wait_limit);
        return 0;
    };
    const uint32_t cus = (uint32_t)c->n_cus;
    const bool trio = v == 5 || ((v == 0 || v == 3) && 3u * n_blocks <= cus);
    if (trio || v == 3 || v == 6 || (v == 0 && 2u * n_blocks <= cus)) return launch_multi(frames, n_blocks, trio && v != 6);
    // More blocks than CUs, one workgroup per block: the blocks run in rounds of n_cus, and a last round with few blocks would
    // leave most of the chip idle for a whole block latency (321 blocks: 256 + 65).  The blocks of such a partial round get several
    // workgroups each, in a launch of their own behind the full rounds (tsq_threads.cpp:71 deals blocks to workers the same way:
    // whoever is free takes the next).
    if (v == 0 && n_blocks > cus) {
        const uint32_t tail = n_blocks % cus, full = n_blocks - tail;
        if (tail != 0u && 2u * tail <= cus) {
            hipLaunchKernelGGL(dec_sym_kernel, dim3(full), dim3(SymCfg::T), SymLds::total, s, container, frames, out, status);
            return launch_multi(frames + full, tail, 3u * tail <= cus);
        }
    }
    // one workgroup per block at any block count: with more blocks than CUs the blocks simply queue (the decoder needs its 150 KB
    // of LDS; the two-per-CU layout of the byte-granular decoder was 1.85x slower per byte, tools/config5_sweep.py)
    hipLaunchKernelGGL(dec_sym_kernel, dim3(n_blocks), dim3(SymCfg::T), SymLds::total, s, container, frames, out, status);
    return 0;
}

// Range reads (dec_range_kernel, one workgroup per item), record reads (dec_group_kernel, one per group) and the batch decode with
// a verdict per item (dec_item_kernel, one per block), at any count: `args` are the kernel's own.  Items, groups and owners are in
// device memory.
template <auto Kernel, class... Args>
inline int launch_read_kernel(tsqa_ctx* c, uint32_t n_groups, hipStream_t s, Args... args)
{
    TSQ_RAISE_LDS(c, lds_need(Kernel, SymLds::total));
    hipLaunchKernelGGL(Kernel, dim3(n_groups), dim3(SymCfg::T), SymLds::total, s, args...);
    return 0;
}

}  // namespace tsq
