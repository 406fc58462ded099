"""Seeded inputs for the scheduler behind the reference's own API (turbosqueeze_amd/csrc/tsq_compat.hip: tsqCompress_MT,
tsqDecompress_MT, the async forms, tsqCompress / tsqDecompress on FILE*).  No GPU here: containers, expectations that come from the
builders of tests/streamgen.py or from the oracle, and the few lines of the scheduler that the inputs are aimed at, restated.

  ramp_containers      block counts on and around the ramped schedule of Scheduler::job_batches, plus the containers of uneven blocks
  twin_containers      every invalid twin of the decoder catalogue as block k of six: a job that fails with batches in flight
  damaged_containers   byte damage, lying headers, trailing bytes and cuts, on containers small enough for the oracle to judge all
  lookahead_jobs       compress jobs (A, B) through one lane: B's look-ahead falls where the lane still holds A's bytes

What is restated from tsq_compat.hip, and must be re-derived when it changes there:
  decompress_schedule  Scheduler::job_batch / job_batches (the decompress branch), for a memory-to-memory job on one device with the
                       default TSQ_AMD_LANES (4) and TSQ_AMD_BATCH_BLOCKS (512); RAMP_COUNTS are chosen from it
  lane_leftovers       what a lane's input buffer holds behind a batch (run_compress: a batch is copied to the buffer's start, with up
                       to 128 bytes of look-ahead), for one lane; the (A, B) pairs are chosen from it
  The twins' places (block 0, 2, 3, 5 of six at two blocks per batch) assume equal batches below 64 blocks, and the progress tests
  assume one call per block whatever Scheduler::progress_piece makes of a batch.
"""
from __future__ import annotations

import numpy as np

import encgen
import streamgen
from streamgen import CATALOGUE

BLOCK = streamgen.BLOCK
HALO = 128
HEALTHY = "soup_5000_default_noext"


# ---------------------------------------------------------------------------------------------------------------- the ramp

def decompress_schedule(nb: int, lanes: int = 4, batch_blocks: int = 512, ramp: bool = True) -> list[int]:
    """Scheduler::job_batches(nb, through_files = false, compress = false) on one device: equal batches below 64 blocks (one per
    lane, at least 32 blocks each), else a first batch of max(8, nb / 16) blocks, every next one half again as large, and a rest of
    fewer than 8 blocks is taken into the batch before it.  RE-DERIVE when job_batch or job_batches changes."""
    if nb < 64 or not ramp:
        batch = min(batch_blocks, max(32, -(-nb // lanes)))
        return [min(batch, nb - b) for b in range(0, nb, batch)]
    out, left, size = [], nb, max(8, nb // 16)
    while left:
        take = min(size, left)
        if left - take < 8:
            take = left
        take = min(take, batch_blocks)
        out.append(take)
        left -= take
        size += size // 2
    return out


def _first_count_ending_in_8(above: int) -> int:
    """the smallest block count above `above` whose schedule ends with a batch of exactly 8 blocks that was not merged"""
    n = above + 1
    while decompress_schedule(n)[-1] != 8:
        n += 1
    return n


# 63: not ramped; 64: the threshold; 70: the last batch swallows a crumb of 5; 73: it does not (a tail of 8 stays); the last: the
# next count after 73 whose schedule ends in a batch of exactly 8, one ramp step further
RAMP_COUNTS = (63, 64, 70, 73, _first_count_ending_in_8(73))


def _joined(blocks):
    return streamgen.container(blocks), b"".join(p for _, _, p in blocks)


def ramp_containers():
    """-> [(name, container, plain, expected batch sizes)]: blocks_for(n) for RAMP_COUNTS, then the uneven unit and the region
    container (their schedules are the unramped ones)"""
    out = []
    for n in RAMP_COUNTS:
        blob, plain = _joined(streamgen.blocks_for(n))
        out.append((f"ramp_{n}", blob, plain, decompress_schedule(n)))
    for name, blocks in (("uneven_unit", streamgen.uneven_unit()), ("regions", streamgen.region_container()[0])):
        blob, plain = _joined(blocks)
        out.append((name, blob, plain, decompress_schedule(len(blocks))))
    return out


def block_count(blob: bytes) -> int:
    return int.from_bytes(blob[4:8], "little")


# ---------------------------------------------------------------------------------------------------------------- twins

TWIN_PLACES = (0, 2, 3, 5)          # of six blocks at two per batch: first batch, second batch, its second block, last batch


def walk_refuses(stream: bytes) -> bool:
    """the frame walk refuses it before any kernel sees it (tsq_format.h read_frame; test_gpu_stream_conformance.refusal_code)"""
    return len(stream) < 3 or int.from_bytes(stream[:3], "little") > BLOCK


def healthy_six():
    return _joined([CATALOGUE.valid[HEALTHY]] * 6)


def twin_containers():
    """-> [(name, container, k, 'stream' | 'walk')]: every invalid twin as block k of six, the other five the healthy soup; the
    header counts the twin with the size its own size word claims.  'stream': the frames are well formed and the decoder refuses
    the block, so the batches before it have been issued and some have come back; 'walk': the frame walk refuses the frame."""
    healthy = CATALOGUE.valid[HEALTHY]
    out = []
    for i, (name, (ext, stream)) in enumerate(CATALOGUE.invalid.items()):
        k = TWIN_PLACES[i % len(TWIN_PLACES)]
        claimed = int.from_bytes(stream[:3].ljust(3, b"\0"), "little")
        blocks = [healthy] * 6
        blocks[k] = (ext, stream, bytes(claimed))
        out.append((name, streamgen.container(blocks), k, "walk" if walk_refuses(stream) else "stream"))
    return out


# ---------------------------------------------------------------------------------------------------------------- damage

DAMAGE_SEED = 20260


def frames_of(raw):
    """(stream_at, stream_len) of every frame of a well-formed container"""
    at, out = 16, []
    for _ in range(int.from_bytes(bytes(raw[4:8]), "little")):
        ln = int(raw[at]) | int(raw[at + 1]) << 8 | (int(raw[at + 2]) & 0x7F) << 16
        out.append((at + 3, ln))
        at += 3 + ln
    return out


def damage_bases():
    """three containers of 8, 10 and 12 small catalogue blocks, both ext bits, each container under 400 KB of stream"""
    rng = np.random.default_rng(DAMAGE_SEED)
    small = [CATALOGUE.valid[n] for n in sorted(CATALOGUE.valid) if 16 <= len(CATALOGUE.valid[n][1]) <= 40_000]
    assert len(small) >= 30
    bases = []
    for nb in (8, 10, 12):
        blocks = [small[int(j)] for j in rng.choice(len(small), size=nb, replace=False)]
        assert {e for e, _, _ in blocks} == {0, 1} and sum(len(s) for _, s, _ in blocks) < 400_000
        bases.append(_joined(blocks))
    return bases


def damaged_containers(n_cases: int = 120, seed: int = DAMAGE_SEED):
    """-> [(name, container)].  n_cases of byte damage: 1 to 5 bytes at offsets >= 16, six in ten inside one frame's stream body,
    a byte replaced or one bit flipped (the recipe of test_gpu_range.test_damaged_containers); then the deterministic header and
    tail cases on the first base.  The expectation is expected_of_the_scheduler's."""
    rng = np.random.default_rng(seed)
    bases = [np.frombuffer(b, dtype=np.uint8) for b, _ in damage_bases()]
    out = []
    for case in range(n_cases):
        blob = bases[case % len(bases)]
        fr = frames_of(blob)
        bad = blob.copy()
        body_only = rng.random() < 0.6
        k = int(rng.integers(0, len(fr)))
        for _ in range(int(rng.integers(1, 6))):
            at = int(rng.integers(fr[k][0] + 3, fr[k][0] + fr[k][1])) if body_only else int(rng.integers(16, bad.size))
            bad[at] = rng.integers(0, 256) if rng.random() < 0.7 else bad[at] ^ (1 << int(rng.integers(0, 8)))
        out.append((f"damage_{case:03d}", bad.tobytes()))
    return out + header_and_tail_cases()


def header_and_tail_cases():
    good = damage_bases()[0][0]
    nb, total = int.from_bytes(good[4:8], "little"), int.from_bytes(good[8:16], "little")
    fr = frames_of(good)
    head = lambda n, t: good[:4] + n.to_bytes(4, "little") + t.to_bytes(8, "little") + good[16:]
    mid = len(fr) // 2
    word_at, stream_at, stream_len = fr[mid][0] - 3, fr[mid][0], fr[mid][1]
    assert stream_len > 8
    return [("total_plus_1", head(nb, total + 1)), ("total_minus_1", head(nb, total - 1)),
            ("n_blocks_plus_1", head(nb + 1, total)), ("n_blocks_minus_1", head(nb - 1, total)),
            ("trailing_1", good + b"\x5a"), ("trailing_100", good + bytes(range(1, 101))),
            ("cut_in_header", good[:10]), ("cut_in_frame_word", good[:word_at + 1]), ("cut_in_size_word", good[:stream_at + 2]),
            ("cut_mid_stream", good[:stream_at + stream_len // 2]), ("cut_at_frame_end", good[:stream_at + stream_len])]


# What the oracle says of the deterministic cases: the decoded length, or None where it refuses (test_mt_cases_cpu.py holds the
# oracle against this record).  Like the reference (tsq_threads.cpp:640-650,825) the oracle delivers what the frames hold, so it
# lets a header pass that promises a byte or a block too many.
def header_and_tail_record():
    good, plain = damage_bases()[0]
    last_block = int.from_bytes(good[frames_of(good)[-1][0]:][:3], "little")
    return {"total_plus_1": len(plain), "total_minus_1": None, "n_blocks_plus_1": None, "n_blocks_minus_1": len(plain) - last_block,
            "trailing_1": len(plain), "trailing_100": len(plain), "cut_in_header": None, "cut_in_frame_word": None,
            "cut_in_size_word": None, "cut_mid_stream": None, "cut_at_frame_end": None}


def expected_of_the_scheduler(oracle, blob: bytes):
    """What tsqDecompress_MT owes for a container: the oracle's bytes, or None (a false return) where the oracle refuses it.  One
    rule of the library's own comes on top, the integrity check that every decompress entry point of it makes
    (include/turbosqueeze_amd.h: "sizes that add up to the header's total"; run_decompress: produced != total): where the oracle
    decodes the frames to a length other than the one the header states, the library refuses the container rather than deliver
    bytes the header does not vouch for.  The check is stricter than the reference and stays."""
    want = oracle.decompress(blob)
    if want is not None and len(want) != int.from_bytes(blob[8:16], "little"):
        return None
    return want


# ---------------------------------------------------------------------------------------------------------------- look-ahead

def _nonzero(rng, n):
    return rng.integers(1, 256, size=n, dtype=np.uint8)


def _ends_in_a_match_over(rng, n, behind: bytes, back: int = 6):
    """n non-zero random bytes that end, as encgen.tails' tail_match_n_minus_*_zero cases do, with the first `back` bytes of a
    phrase that stood 40-odd bytes earlier, where it went on with `behind` and then zeros: the match that starts `back` bytes
    before the end runs on through the look-ahead exactly when `behind` + zeros is what follows the data."""
    ph = _nonzero(rng, 70)
    ph[back:] = 0
    ph[back:back + len(behind)] = np.frombuffer(behind, dtype=np.uint8)
    rest = n - (70 + 40 + back + back)
    return np.concatenate([_nonzero(rng, rest), ph, _nonzero(rng, 40 + back), ph[:back]])


def lane_leftovers(jobs, batch_blocks):
    """RE-DERIVE with run_compress.  One lane, jobs in order, each cut into batches of batch_blocks blocks; a batch of n bytes at
    `at` is copied to the start of the lane's input buffer with its look-ahead, got = min(n + 128, total - at) bytes in all.
    -> for the LAST job, per batch: (at, n, got, what the buffer holds in [got, n + 128) from earlier batches, zero-padded)."""
    lane = bytearray()
    last = []
    for j, data in enumerate(jobs):
        step = batch_blocks * BLOCK
        for at in range(0, len(data), step):
            n = min(step, len(data) - at)
            got = min(n + HALO, len(data) - at)
            if j == len(jobs) - 1:
                last.append((at, n, got, bytes(lane[got:n + HALO]).ljust(n + HALO - got, b"\0")))
            if len(lane) < got:
                lane.extend(bytes(got - len(lane)))
            lane[0:got] = data[at:at + got]
    return last


def lookahead_differs(oracle, a: bytes, b: bytes, ext: int, batch_blocks: int) -> bool:
    """the criterion: some block of B encodes differently with the lane's leftovers of A (and of B's own earlier batches) behind the
    bytes that were copied than with zeros there"""
    for at, n, got, stale in lane_leftovers([a, b], batch_blocks):
        if not any(stale):
            continue
        true_buf = b[at:at + got] + bytes(len(stale))
        stale_buf = b[at:at + got] + stale
        for b0 in range(0, n, BLOCK):
            ln = min(BLOCK, n - b0)
            if b0 + ln + HALO <= got:
                continue                                  # this block's look-ahead was copied in full
            t = oracle.encode_block(true_buf[b0:b0 + ln], ext, halo=true_buf[b0 + ln:b0 + ln + HALO])
            s = oracle.encode_block(stale_buf[b0:b0 + ln], ext, halo=stale_buf[b0 + ln:b0 + ln + HALO])
            if t != s:
                return True
    return False


MEM_BATCH = 32          # a memory-to-memory job below 33 blocks on one lane is one batch (job_batch)
FILE_BATCH = 1          # TSQ_AMD_FILE_BATCH_BLOCKS=1 in the streamed runs


def lookahead_candidates():
    """-> (A, [(name, B)]).  A: two blocks and a bit of non-zero random bytes.  B: the encoder catalogue's inputs of a whole number
    of blocks, then inputs built the way encgen.tails builds its tail_match_* cases -- the catalogue's own whole-block case ends in
    a match that only a CONTINUING look-ahead lengthens, which neither zeros nor A's bytes are -- : one and two full blocks whose
    last match runs on over zeros, and a full block plus the catalogue's random tail of n bytes, n in TAIL_NS[:8], whose first block
    ends in a match that runs on over the tail and the zeros behind it."""
    rng = np.random.default_rng(7001)
    a = _nonzero(rng, 2 * BLOCK + 5000).tobytes()
    # (encgen.catalogue() holds what full_blocks() and tails() give, built once per process)
    cands = [(f"catalogue_{c.name}", c.data) for c in encgen.catalogue() if len(c.data) and len(c.data) % BLOCK == 0]
    cands.append(("built_one_block_match_over_zeros", _ends_in_a_match_over(rng, BLOCK, b"", back=6).tobytes()))
    two = np.concatenate([_nonzero(rng, BLOCK), _ends_in_a_match_over(rng, BLOCK, b"", back=4)])
    cands.append(("built_two_blocks_match_over_zeros", two.tobytes()))
    tails = {len(c.data): c.data for c in encgen.catalogue() if c.name.startswith("tail_random_")}
    for n in encgen.TAIL_NS[:8]:
        first = _ends_in_a_match_over(rng, BLOCK, tails[n], back=5)
        cands.append((f"built_block_plus_{n}", first.tobytes() + tails[n]))
    return a, cands


_LOOKAHEAD = None


def lookahead_jobs(oracle):
    """-> (A, [(name, B, ext)]): the candidates whose container, memory to memory, differs at level `ext` (the first of 0, 1 that
    shows it) when A's leftovers are seen behind B instead of zeros.  Made once per process: a verdict costs two encodes of 4 MiB."""
    global _LOOKAHEAD
    if _LOOKAHEAD is None:
        a, cands = lookahead_candidates()
        kept, dropped = [], []
        for name, b in cands:
            ext = next((e for e in (0, 1) if lookahead_differs(oracle, a, b, e, MEM_BATCH)), None)
            if ext is not None:
                kept.append((name, b, ext))
            else:
                dropped.append(name)
        _LOOKAHEAD = (a, kept, dropped)
    return _LOOKAHEAD[:2]


def lookahead_dropped(oracle):
    """the candidates that do not meet the criterion"""
    lookahead_jobs(oracle)
    return _LOOKAHEAD[2]
