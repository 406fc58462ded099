/*
 * tsq_oracle.h -- CPU restatement of turbosqueeze's per-block codec.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product
 * path: only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg
 * may load this library, and only as the checker.  The shipped library
 * (turbosqueeze_amd/csrc -> libturbosqueeze_amd.so) never links or calls it.
 *
 * Pinning: checked against the known-answer vectors K0..K7 of SURVEY.md
 * section 8c (tests/test_oracle_kat.py) and, in the build container, against
 * the reference's own tsq_encode.cpp / tsq_decode.cpp compiled unmodified
 * into oracle/_ref (tests/test_oracle_vs_ref.py, oracle/Makefile).
 */
#ifndef TSQ_ORACLE_H
#define TSQ_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSQO_BLOCK_BITS   22
#define TSQO_BLOCK_SZ     (1u << TSQO_BLOCK_BITS)            /* turbosqueeze.h:37-38 */
#define TSQO_OUTPUT_SZ    (TSQO_BLOCK_SZ + (TSQO_BLOCK_SZ >> 2)) /* turbosqueeze.h:39 */
#define TSQO_HASH_BITS    17                                 /* turbosqueeze.h:41 */
#define TSQO_HASH_ENTRIES (1u << TSQO_HASH_BITS)
#define TSQO_HALO         128  /* readable bytes required after every block */

/* Upper bound of the compressed size of an n-byte block (all 16-byte literals):
 * 3 (size) + n + one control per 8 symbols + one size byte per 2 symbols + 2. */
uint32_t tsqo_bound(uint32_t n);

/*
 * Encode one block under the canonical oracle conditions of SURVEY.md 8c:
 *   - `in` must have TSQO_HALO readable bytes after in[n-1] (the next block's
 *     first bytes, or zeros after the final block);
 *   - the output is produced as if `out` had been zero-filled beforehand
 *     (the function zero-fills tsqo_bound(n)+16 bytes itself);
 *   - `table` is the 2^17 x u16 position table; it is zeroed here
 *     (tsqInit, tsq_context.cpp:77-80) and left in its final state.
 * Returns the compressed size.  Follows tsq_encode.cpp:48-189 (ext == 0) and
 * tsq_encode.cpp:192-342 (ext != 0).
 */
uint32_t tsqo_encode_block(const uint8_t *in, uint32_t n, uint8_t *out,
                           uint32_t ext, uint16_t *table);

/*
 * The same encoder, instrumented and mutable (tsq_oracle.c compiles ONE body into both entry points:
 * tsqo_encode_block carries no trace or mutant test in its loops).  tests/encgen.py turns the trace
 * into a census of the encoder's rules and the mutants into a kill matrix.
 *
 * Trace: one record per probed position, in the scan loop and in the chain loop.
 */
typedef struct {
    uint32_t i;                 /* probed position */
    uint32_t pos;               /* the candidate the table gave */
    uint32_t origin_at_offset;  /* pair origin when `offset` was computed (before a forced flush) */
    uint32_t origin_at_test;    /* pair origin when the match was tested / its length clamped */
    uint32_t offset;            /* origin_at_offset - pos (the value the acceptance test saw) */
    uint32_t k_raw;             /* raw common prefix, 0xFFFFFFFF where none was computed */
    uint32_t k;                 /* after the room clamp */
    uint32_t outcome;           /* TSQO_OUT_* */
    uint32_t flags;             /* TSQO_TF_*; the match's nibble in bits 8..11 */
    uint32_t flush;             /* TSQO_FL_*; the bytes flushed before a match in bits 8.. */
} tsqo_trace_rec;

enum {
    TSQO_OUT_LITERAL = 0,           /* scan probe refused: the byte stays pending */
    TSQO_OUT_MATCH = 1,
    TSQO_OUT_BREAK_WORD = 2,        /* chain probe: four bytes differ */
    TSQO_OUT_BREAK_OFFSET = 3,      /* chain probe: offset outside [4, 0xFFFE] */
    TSQO_OUT_BREAK_SHORT = 4,       /* accepted probe, but k < 4 after the room clamp */
    TSQO_OUT_BREAK_TAIL = 5,        /* chain probe at i >= n - 5 */
    TSQO_OUT_END = 6,               /* scan reached n */
    TSQO_OUT_BREAK_OFFSET_LATE = 7  /* accepted scan probe whose offset the forced flush moved out of range */
};
enum { TSQO_TF_WORD_EQUAL = 1, TSQO_TF_CHAIN_PROBE = 2 };
enum { TSQO_FL_FORCED = 1, TSQO_FL_BEFORE_MATCH = 2 };

/* Mutants: one deliberate single-rule error each.  0 is the oracle. */
enum {
    TSQO_MUT_NONE = 0,
    TSQO_MUT_OFFSET_BOUND_PLUS,    /* offsets up to 0xFFFF accepted */
    TSQO_MUT_OFFSET_BOUND_MINUS,   /* offsets up to 0xFFFD only */
    TSQO_MUT_LO_GT,                /* lo > (i & 0xFFFF): a candidate 65 536 back becomes the position itself */
    TSQO_MUT_ROOM_WHOLE,           /* the room clamp yields room, not room - 1 */
    TSQO_MUT_ROOM_DROPPED,         /* no room clamp */
    TSQO_MUT_CHAIN_N4,             /* chain goes on while i < n - 4 */
    TSQO_MUT_CHAIN_N6,             /* chain goes on while i < n - 6 */
    TSQO_MUT_FLUSH_AT_32,          /* forced flush at 33 pending bytes instead of 32 */
    TSQO_MUT_OFFSET_AFTER_FLUSH,   /* offset recomputed after the forced flush */
    TSQO_MUT_NIB17_PLUS, TSQO_MUT_NIB32_PLUS, TSQO_MUT_NIB32_MINUS, TSQO_MUT_NIB48_PLUS, TSQO_MUT_NIB48_MINUS,
    TSQO_MUT_NIB64_PLUS, TSQO_MUT_NIB64_MINUS,   /* length_nibble thresholds off by one */
    TSQO_MUT_CAP48,                /* extension cap 48 */
    TSQO_MUT_NO_CHAIN_INSERT,      /* the table is not updated at chain positions */
    TSQO_MUT_INSERT_POS0,          /* the table is updated for position 0 (no effect: it stores the 0 the table starts with) */
    TSQO_MUT_SECOND_RECENT,        /* second most recent insertion when the most recent is at most 256 back: a missed twin */
    TSQO_MUT_SKIP_PREV_TILE,       /* insertions of the previous 64-aligned tile ignored: a missed patch */
    TSQO_MUT_TRIM_SPILL,           /* literal stores trimmed to their length: no spill into control / size bytes */
    TSQO_MUT_COUNT
};

/* As tsqo_encode_block.  Writes at most `trace_cap` records (trace may be NULL) and stores the number
 * of probes in *trace_count.  Returns 0 for an unknown mutant.  A mutant's stream may be invalid. */
uint32_t tsqo_encode_block_traced(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t ext, uint16_t *table,
                                  uint32_t mutant, tsqo_trace_rec *trace, uint64_t trace_cap, uint64_t *trace_count);

/*
 * Decode one block stream.  `in_len` bounds the reads (the reference ignores
 * it and over-reads; we stop instead).  Writes exactly the header's size
 * bytes to `out` (never beyond) and returns that size; returns 0 with
 * *status != 0 on an oversize header (tsq_decode.cpp:53,146) or a malformed
 * stream.  Follows tsq_decode.cpp:42-126 / 129-315.
 *   status: 0 ok, 1 size header > 4 MiB, 2 stream truncated,
 *           3 match source before block start, 4 match source overlaps pair.
 */
uint32_t tsqo_decode_block(const uint8_t *in, uint32_t in_len, uint8_t *out,
                           uint32_t ext, int *status);

/*
 * Container helpers (turbosqueeze.cpp:64-83, tsq_threads.cpp:218-239,333-335):
 * 16-byte header "TSQ1" | u32 n_blocks | u64 total, then per block a u24
 * frame (compressed size | ext << 23) followed by the block stream.
 * `in` needs TSQO_HALO zero bytes after in[n-1].  Returns bytes written.
 * `threads` > 1 splits the blocks over that many pthreads (block b -> b % T).
 */
size_t tsqo_compress_bound(size_t n);
size_t tsqo_compress(const uint8_t *in, size_t n, uint8_t *out, uint32_t ext, int threads);
/* Returns the decompressed size, or (size_t)-1 on a malformed container. */
size_t tsqo_decompressed_size(const uint8_t *in, size_t n);
size_t tsqo_decompress(const uint8_t *in, size_t n, uint8_t *out, size_t out_cap, int threads);

/* CPU baseline for bench.py: block-parallel encode+decode on `threads` pthreads, best of `reps`
 * warm passes.  enc/dec: addresses of the reference's tsqEncode/tsqDecode (oracle/_ref) or NULL
 * for the port.  Returns 0 when the round trip reproduced the input. */
int tsqo_cpubench2(void *enc, void *dec, const uint8_t *in, size_t n, uint32_t ext, int threads, int reps, int shape, int pin,
                   double *enc_seconds, double *dec_seconds, uint64_t *compressed_bytes);
int tsqo_cpubench(void *enc, void *dec, const uint8_t *in, size_t n, uint32_t ext, int threads, int reps,
                  double *enc_seconds, double *dec_seconds, uint64_t *compressed_bytes);

/* FNV-1a 64 (basis cbf29ce484222325, prime 100000001b3). */
uint64_t tsqo_fnv1a64(const uint8_t *p, size_t n);

#ifdef __cplusplus
}
#endif
#endif
