// tsq_dec_duo.cuh -- block decoder on two or three workgroups per block (decoder variants 3, 5 and 6; chosen by itself when a launch has at
// most half as many blocks as the device has CUs -- every GPU of a multi-GPU enwik9 job).
//
// A block's decode is two serial chains (tsq_decode.cpp:62-88): the PARSE chain -- where a chunk of the stream starts follows from
// where the previous one ended -- and the COPY chain -- a chunk's bytes may copy the 64 KiB before them.  dec_sym_kernel runs both
// on one CU, one after the other per chunk.  Here they run on different CUs of the same XCD, side by side:
//
//   PARSE workgroups  phases P0..P4 (tsq_dec_common.cuh) on fixed windows of the stream, then hand the chunk's pair words, group
//                     output offsets and a header to the COPY workgroup through a four-deep ring of records in global memory (they
//                     stay in the XCD's L2) and move on to the next window at once.
//   COPY workgroup    phase P5 (pairs -> records -> bytes, history in the 64 KiB LDS ring) and P7, the stores to HBM.
//
// Workgroup w runs on XCD w % 8 (the hardware deals workgroups round-robin): w -> (xcd = w % 8, slot = w / 8), role = slot % (NP + 1),
// block = (slot / (NP + 1)) * 8 + xcd puts a block's workgroups on one XCD, the PARSE ones dispatched first.  Every wait is bounded
// and also ends when another block has reported an error.
#pragma once

#include "tsq_common.cuh"
#include "tsq_dec_common.cuh"
#include "tsq_dec_sym.cuh"

namespace tsq {

struct DuoCfg {
    static constexpr uint32_t SLOTS = 4;                                   // chunk records in flight per block
    static constexpr uint32_t HDR = 8;                                     // header words: 0 sp, 1 op, 2 groups, 3 next op, 4 flags, 5 next sp
    static constexpr uint32_t REC_WORDS = ((HDR + 5 * SymCfg::MAXG) + 63u) & ~63u;
    static constexpr uint32_t FLAG_STRIDE = 64;                            // u32 words per block: [0] records produced, [32] records consumed,
                                                                           // [8 + 8 p ..]: the entry mailbox of PARSE workgroup p (sequence, delta | flags << 16, op, record)
    static constexpr uint32_t kLast = 1, kError = 2;
    static constexpr uint32_t kAbort = 0xFFFFFFFFu;
    static constexpr uint32_t kSpinLimit = 1u << 24;                       // default number of polls (with s_sleep) before a wait gives up: seconds
                                                                           // (the launch passes the context's limit: tsqa_set_decode_wait_limit)
};

// polls are relaxed loads (an acquire load invalidates the CU's vector cache every time: hundreds of polling workgroups would keep
// the L2 busy with nothing); one acquire fence follows the poll that succeeds
__device__ __forceinline__ uint32_t duo_load_acquire(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void duo_acquire_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
__device__ __forceinline__ void duo_store_release(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------------------------------------------------------ PARSE
// The stream is parsed in FIXED windows: window k covers stream offsets [3 + k S, 3 + (k + 1) S + pad).  The speculative part of the
// parse (P0..P2: every offset parsed as if a group started there, pointer doubling) does not depend on where the chunk's first group
// really starts, only the chain (P3) and the groups (P4) do -- and the first group of window k + 1 starts less than 133 bytes into it
// (where the last group of window k ends).  So NP PARSE workgroups take the windows in turn: each prepares its window on its own and
// waits only for the ENTRY (offset of the first group, output position, record number) that the workgroup of the window before
// publishes as soon as its own chain has reached its window's end.  The block's serial parse chain is then P3 + P4 per window.
// NP = 1: the same code, the entry is handed over in registers.
template <uint32_t NP>
__device__ __forceinline__ void duo_parse(const uint8_t* __restrict__ in, uint32_t in_len, uint32_t size, uint32_t ext, uint32_t me,
                                          uint32_t* __restrict__ ring_g, uint32_t* __restrict__ flags, int32_t* __restrict__ status, uint8_t* lds,
                                          uint32_t spin_limit)
{
    using C = SymCfg;
    using L = SymLds;
    const uint32_t* const gout = reinterpret_cast<const uint32_t*>(lds + L::gout);
    const uint32_t* const pairs = reinterpret_cast<const uint32_t*>(lds + L::pairs);
    uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + L::misc);
    const uint32_t tid = threadIdx.x;

    if (size == 0u) return;                              // (an empty block has no chunks: no workgroup has anything to do)
    if (tid == 0) misc[4] = 0;
    // the entry of this workgroup's next window, when it is handed over in registers (NP == 1, or window 0)
    uint32_t e_delta = 0, e_op = 0, e_rec = 0;
    bool e_known = me == 0u;
    uint32_t* const entry_in = flags + 8u + 8u * me;                        // [0] sequence, [1] delta | flags << 16, [2] op, [3] record number
    uint32_t* const entry_out = flags + 8u + 8u * ((me + 1u) % NP);
    uint32_t n_in = 0, n_out = 0;                                           // entries received / sent so far
    // whole 16-byte words of window q, loaded an iteration ahead (the windows lie at fixed places)
    auto prefetch = [&](uint32_t q) {
        const uint64_t at = 3ull + (uint64_t)q * C::S;
        return at < in_len ? prefetch_words(in, (uint32_t)at, in_len - (uint32_t)at) : make_uint4(0, 0, 0, 0);
    };
    uint4 pre = prefetch(me);
    auto give_up = [&](uint32_t why) {
        // (uniform: every thread calls it) tell the others and leave
        if (tid == 0) {
            if (why == 2u) atomicMax(status, kErrStall);       // (a sibling workgroup did not show up in time: not the stream's fault)
            duo_store_release(flags + 32, DuoCfg::kAbort);
        }
    };
    __syncthreads();

    for (uint32_t k = me;; k += NP) {
        const uint64_t w64 = 3ull + (uint64_t)k * C::S;
        const bool beyond = w64 >= in_len;                                   // no such window: only the "finished" entry can come
        const uint32_t W = beyond ? in_len : (uint32_t)w64;
        const uint32_t avail = in_len - W;
        const uint32_t slim = avail < C::S ? avail : C::S;
        if (!beyond) {
            stage_words<L>(lds, in, W, avail, pre);                            // P0
            pre = prefetch(k + NP);                                              // this workgroup's next window is on its way
            __syncthreads();
            uint32_t x[C::PER];
            parse_groups<L>(lds, slim, x);                                       // P1
            double_pointers<L>(lds, slim, x);                                    // P2
        }
        // ---------------- the window's entry: where its first group starts, the output position there, the record number
        uint32_t delta, op, rec_no;
        if (e_known) { delta = e_delta; op = e_op; rec_no = e_rec; e_known = false; }
        else {
            if (tid == 0) {
                uint32_t why = 0, spins = 0;
                for (;;) {
                    if (duo_load_acquire(entry_in) > n_in) break;
                    if ((spins & 63u) == 63u && (duo_load_acquire(flags + 32) == DuoCfg::kAbort || __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) { why = 1; break; }
                    if (++spins > spin_limit) { why = 2; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                duo_acquire_fence();
                misc[6] = why;
                if (!why) { misc[7] = __builtin_nontemporal_load(entry_in + 1); misc[8] = __builtin_nontemporal_load(entry_in + 2); misc[9] = __builtin_nontemporal_load(entry_in + 3); }
            }
            __syncthreads();
            if (misc[6] != 0) { give_up(misc[6]); return; }
            n_in++;
            const uint32_t d = misc[7];
            if (d >> 16) return;                                                 // finished (or failed) in an earlier window
            delta = d & 0xFFFFu; op = misc[8]; rec_no = misc[9];
            __syncthreads();                                                     // (misc[7..9] are read: they may be written again)
        }
        if (beyond) {                                                            // the chain runs past the stream's end: malformed
            if (tid == 0) atomicMax(status, kErrStream);
            // tell the COPY workgroup (through a record, in order)
            // (fall through to the hand-over below with `bad`; the chain and the groups find nothing below slim = 0)
        }
        // ---------------- the chunks of this window: normally one; more when the LDS image budget of the COPY workgroup cuts one short
        for (;;) {
            if (tid == 0) { misc[0] = 0; misc[1] = 0; misc[2] = 0xFFFFFFFFu; misc[3] = 0xFFFFFFFFu; misc[5] = 0; }
            __syncthreads();
            const uint32_t nsn = walk_chain<L>(lds, delta, slim);                // P3
            group_lanes<L>(lds, nsn, slim, op, size, ext);                       // P4
            __syncthreads();
            const ChunkEnd e = chunk_end<L>(lds, op, size);
            const uint32_t next_delta = e.last || e.cut ? e.next_at : e.next_at - C::S;
            // (a chunk that neither completes the block nor is cut short must have run to the end of a FULL window)
            const bool bad = beyond || misc[4] != 0 || e.ng == 0 || (!e.last && !e.cut && (slim < C::S || e.next_at < C::S || next_delta >= C::SPAD));
            // ---------------- the next window's workgroup gets its entry as early as possible
            if (!e.cut || bad) {
                const uint32_t fl = bad ? 2u : e.last ? 1u : 0u;
                if (NP == 1u) {
                    if (fl) { /* nothing to hand over */ } else { e_delta = next_delta; e_op = e.next_op; e_rec = rec_no + 1u; e_known = true; }
                } else {
                    if (tid == 0) {
                        __builtin_nontemporal_store((fl << 16) | next_delta, entry_out + 1);
                        __builtin_nontemporal_store(e.next_op, entry_out + 2);
                        __builtin_nontemporal_store(rec_no + 1u, entry_out + 3);
                        duo_store_release(entry_out, n_out + 1u);
                    }
                    n_out++;
                }
            }
            // ---------------- hand the chunk to the COPY workgroup: records go out in order, into a free slot
            if (tid == 0) {
                uint32_t why = 0, spins = 0;
                for (;;) {
                    const uint32_t done = duo_load_acquire(flags + 32);
                    if (done == DuoCfg::kAbort || ((spins & 255u) == 255u && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) { why = 1; break; }
                    if (rec_no - done < DuoCfg::SLOTS && (NP == 1u || duo_load_acquire(flags) == rec_no)) break;
                    if (++spins > spin_limit) { why = 2; break; }
                    __builtin_amdgcn_s_sleep(8);                                   // (nobody waits for this workgroup while its ring is full)
                }
                duo_acquire_fence();
                misc[6] = why;
            }
            __syncthreads();
            if (misc[6] != 0) { give_up(misc[6]); return; }
            uint32_t* const rec = ring_g + (size_t)(rec_no % DuoCfg::SLOTS) * DuoCfg::REC_WORDS;
            if (!bad) {
                for (uint32_t w = tid; w < 4u * e.ng; w += C::T) rec[DuoCfg::HDR + w] = pairs[w];
                for (uint32_t w = tid; w < e.ng; w += C::T) rec[DuoCfg::HDR + 4u * C::MAXG + w] = gout[w];
            }
            if (tid == 0) {
                rec[0] = W; rec[1] = op; rec[2] = e.ng; rec[3] = e.next_op;
                rec[4] = (e.last ? DuoCfg::kLast : 0u) | (bad ? DuoCfg::kError : 0u);
                rec[5] = e.cut ? W : W + C::S;                                 // where the next record's window starts (for the COPY side's prefetch)
            }
            // Every wavefront waits for ITS record stores to be acknowledged before the barrier (the workgroup-scope fence of
            // __syncthreads() does not: no s_waitcnt vmcnt(0)), so that they are complete when thread 0 releases at agent scope (its
            // release writes the L2 back once for the whole workgroup; an agent-scope release fence in every thread -- tried -- costs
            // a write-back per wavefront and more than doubled the kernel's time).
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) duo_store_release(flags, rec_no + 1u);            // ... and thread 0 publishes them
            if (bad) { if (tid == 0) atomicMax(status, kErrStream); return; }
            if (e.last) return;
            if (!e.cut) break;
            delta = next_delta; op = e.next_op; rec_no++;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- COPY
struct DuoCopyLds {
    static constexpr uint32_t sbuf = 0;                                             // u8[S + SPAD + 16]
    static constexpr uint32_t recw = sbuf + 16 * SymCfg::SWORDS;                     // u32[OUTC + 16] symbol records, then u16 byte entries over them
    static constexpr uint32_t ent = recw;
    static constexpr uint32_t plist = ent + 2 * (SymCfg::OUTC + 16);                // u16[OUTC] waiting lists
    static constexpr uint32_t wsum = recw + 4 * (SymCfg::OUTC + 16);                // u32[16]
    static constexpr uint32_t misc = wsum + 64;                                     // u32[16]
    static constexpr uint32_t ring = (misc + 64 + 15) & ~15u;                       // u8[R + RPAD]
    static constexpr uint32_t total = ring + SymCfg::R + SymCfg::RPAD;
    static_assert(recw % 16 == 0 && plist % 16 == 0 && plist + 2 * SymCfg::OUTC <= wsum, "records, byte entries and waiting lists");
};
static_assert(DuoCopyLds::total <= 160 * 1024 && SymLds::total <= 160 * 1024, "LDS budget");

__device__ __forceinline__ void duo_copy(const uint8_t* __restrict__ in, uint32_t in_len, uint32_t size, uint32_t ext, uint8_t* __restrict__ out,
                                         const uint32_t* __restrict__ ring_g, uint32_t* __restrict__ flags, int32_t* __restrict__ status, uint8_t* lds,
                                         uint32_t spin_limit)
{
    using C = SymCfg;
    using L = DuoCopyLds;
    uint32_t* const misc = reinterpret_cast<uint32_t*>(lds + L::misc);
    const uint32_t tid = threadIdx.x;
    // ring address of output position p: (p + oskew) mod R, so that 16-byte words of the ring are 16-byte words of HBM
    const uint32_t oskew = (uint32_t)((uintptr_t)out & 15u);
    uint32_t ring_op = oskew;
    Image prev = {0, 0, 0};                                                           // the image P7 writes out next
    uint32_t k = 0, made_seen = 0;
    uint32_t hdr_n[6] = {0, 0, 0, 0, 0, 0}, pw_n[2] = {0, 0}, go_n[2] = {0, 0};
    bool have_next = false;
    if (size == 0u) return;
    if (tid == 0) { misc[4] = 0; }
    // the record's header, this thread's pair words and group output offsets
    auto fetch_record = [&](const uint32_t* rec) {
#pragma unroll
        for (uint32_t q = 0; q < 6; ++q) hdr_n[q] = __builtin_nontemporal_load(rec + q);
#pragma unroll
        for (uint32_t rep = 0; rep < 2; ++rep) {
            const uint32_t gi = tid + rep * C::T;
            pw_n[rep] = rec[DuoCfg::HDR + gi];
            go_n[rep] = rec[DuoCfg::HDR + 4u * C::MAXG + (gi >> 2)];
        }
    };
    uint4 pre = prefetch_words(in, 3u, in_len - 3u);
    uint32_t pre_sp = 3u;                                                             // the stream offset `pre` was loaded from
    __syncthreads();

    for (;;) {
        // ---------------- the previous chunk's bytes go to HBM (P7); thread 0 waits for this chunk's record, if it is not known to be there
        flush_image<L>(lds, out, prev, 0, C::T);
        if (made_seen <= k) {
            if (tid == 0) {
                uint32_t give_up = 0, spins = 0, made = 0;
                for (;;) {
                    made = duo_load_acquire(flags);
                    if (made > k) break;
                    if ((spins & 255u) == 255u && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { give_up = 1; break; }
                    if (++spins > spin_limit) { give_up = 2; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                duo_acquire_fence();
                misc[6] = give_up; misc[7] = made;
            }
            __syncthreads();
            if (misc[6] != 0) {
                if (tid == 0) { duo_store_release(flags + 32, DuoCfg::kAbort); if (misc[6] == 2) atomicMax(status, kErrStall); }
                return;
            }
            made_seen = misc[7];
            have_next = false;
        }
        // the record: fetched during the previous chunk when it was already there (the PARSE side runs up to four chunks ahead), else now
        if (!have_next) fetch_record(ring_g + (size_t)(k % DuoCfg::SLOTS) * DuoCfg::REC_WORDS);
        const uint32_t sp = hdr_n[0], op = hdr_n[1], ng = hdr_n[2], next_op = hdr_n[3], flg = hdr_n[4], next_sp = hdr_n[5];
        have_next = false;
        if (flg & DuoCfg::kError) return;                                              // (the PARSE workgroup has reported it)
        const bool last_chunk = (flg & DuoCfg::kLast) != 0u;
        const Image im = {op, next_op - op, ring_op};
        const uint32_t avail = in_len - sp;
        // ---------------- P0: the chunk's stream to LDS (prefetched a chunk ago when the header was there in time), the records cleared
        if (pre_sp != sp) pre = prefetch_words(in, sp, avail);
        stage_words<L>(lds, in, sp, avail, pre);
        clear_records<L>(lds);
        if (!last_chunk) { pre = prefetch_words(in, next_sp, in_len - next_sp); pre_sp = next_sp; }
        __syncthreads();

        // ---------------- P5: symbols -> bytes
        drop_records<L>(lds, ng, im, size, avail, ext, [&](uint32_t rep, uint32_t) { return make_uint2(pw_n[rep], go_n[rep]); });   // (a)
        __syncthreads();
        k++;
        if (misc[4] != 0) {
            if (tid == 0) { atomicMax(status, (int32_t)misc[4]); duo_store_release(flags + 32, DuoCfg::kAbort); }
            return;
        }
        // the record's slot is free (every thread holds what it needed from it in registers: the barrier above waited for the loads)
        if (tid == 0) __hip_atomic_store(flags + 32, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!last_chunk && made_seen > k) {                                          // the next record is there already: fetch it now
            fetch_record(ring_g + (size_t)(k % DuoCfg::SLOTS) * DuoCfg::REC_WORDS);
            have_next = true;
        }
        const uint32_t n_wait = fetch_bytes<L>(lds, im);                                 // (b) + (c)
        __syncthreads();
        jump_pointers<L>(lds, n_wait);                                                  // (d)
        __syncthreads();
        write_ring<L>(lds, im);                                                          // (e)
        prev = im;
        ring_op += im.len; ring_op -= ring_op >= C::R ? C::R : 0u;
        __syncthreads();                                                               // the image is complete in the ring
        if (last_chunk) break;
    }
    flush_image<L>(lds, out, prev, 0, C::T);
}

// NP PARSE workgroups and one COPY workgroup per block, all on one XCD: workgroup w -> (xcd = w % 8, slot = w / 8), role = slot % (NP + 1),
// block = (slot / (NP + 1)) * 8 + xcd; the COPY workgroup (role NP) is dispatched last.
#ifdef TSQ_STATS
// instrumented builds: the XCD (XCC_ID) every workgroup of the last launch really ran on (tools/duo_xcd.py: how often do a block's
// workgroups share one, as the index mapping below assumes?)
__device__ uint32_t g_duo_xcc[2048];
#endif
template <uint32_t NP>
__global__ __launch_bounds__(1024) void dec_duo_kernel(const uint8_t* __restrict__ container, const FrameInfo* __restrict__ frames, uint32_t n_blocks,
                                                       uint8_t* __restrict__ outbuf, int32_t* __restrict__ status,
                                                       uint32_t* __restrict__ ring_g, uint32_t* __restrict__ flags_g, uint32_t spin_limit)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t w = blockIdx.x, xcd = w & 7u, slot = w >> 3;
    const uint32_t role = slot % (NP + 1u), b = (slot / (NP + 1u)) * 8u + xcd;
#ifdef TSQ_STATS
    if (threadIdx.x == 0 && w < 2048u) { uint32_t id; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id)); g_duo_xcc[w] = 0x80000000u | (id & 15u); }
#endif
    if (b >= n_blocks) return;
    // An error reported before this launch (the frame walk refused the container: the descriptors are not even written) or by
    // another block: leave, all threads together.  (A block's workgroups may read different values while another block is failing;
    // every wait inside also watches the status word, so none is left waiting for a partner that left here.)
    {
        uint32_t* const seen = reinterpret_cast<uint32_t*>(lds);
        if (threadIdx.x == 0) seen[0] = (uint32_t)__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const uint32_t st = seen[0];
        __syncthreads();
        if (st != 0u) return;
    }
    const FrameInfo f = frames[b];
    // (the frame descriptor may come from an untrusted container through tsqa_decode_blocks_async: bounds first)
    if (f.stream_len < 3u || f.stream_len > kSlotSize || f.out_len > kBlockSize) {
        if (threadIdx.x == 0) atomicMax(status, kErrStream);
        return;
    }
    uint32_t* const ring_b = ring_g + (size_t)b * DuoCfg::SLOTS * DuoCfg::REC_WORDS;
    uint32_t* const flags = flags_g + (size_t)b * DuoCfg::FLAG_STRIDE;
    if (role < NP) duo_parse<NP>(container + f.stream_at, f.stream_len, f.out_len, f.ext, role, ring_b, flags, status, lds, spin_limit);
    else duo_copy(container + f.stream_at, f.stream_len, f.out_len, f.ext, outbuf + f.out_at, ring_b, flags, status, lds, spin_limit);
}

}  // namespace tsq
