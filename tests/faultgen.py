"""The seeded batch of the per-item batch decompress tests (test_batch_faults_cpu.py, test_gpu_batch_faults.py): containers the
decoders refuse among containers they deliver, assembled from what the suite already has, so that every verdict is the oracle's.
Host only: numpy, the oracle, the catalogue of hand-assembled streams.

  mtgen.twin_containers()     every invalid twin of the decoder catalogue as block 0, 2, 3 or 5 of six: refused, two of them by
                              the frame walk, the others by a block decoder
  mtgen.damaged_containers()  byte damage, lying headers, trailing bytes and cuts on containers of 8 to 12 blocks: about half are
                              refused, the others are damaged yet valid and must be delivered like any healthy item
  clean items                 small fuzzgen / kat inputs of 1 B to 300 KB compressed by the oracle, both ext bits; the container of
                              uneven blocks (streamgen.uneven_unit: blocks of 0 bytes, a full 4 MiB block); two healthy containers
                              with one byte of room too little; three healthy containers whose place the packed form falsifies

The order alternates accepted and refused items from the first item on, so every refused item has an accepted one on both sides;
the accepted items that are left over follow, the three place items among them.

An item's verdict is `want`: the bytes mtgen.expected_of_the_scheduler gives (the oracle's, and None where the oracle refuses or
decodes to another length than the header states), except for the two tight items, which the oracle would decode and the library
must refuse for the room they are given.

What is restated from the library, and must be re-derived when it changes there:
  walk_refuses        batch_walk_kernel / frame_walk_kernel (tsq_batch.cuh, tsq_container.cuh) with read_header and walk_frames
                      (tsq_format.h, the one frame walk of host and device; test_batch_faults_cpu.py holds it against this
                      restatement): which items the frame walk refuses (TSQA_ERR_FORMAT, nothing written to their range) as
                      opposed to a block decoder (TSQA_ERR_STREAM, the range undefined)
  stated_count, MIN_ITEM   plan_batch (tsq_runtime.hip): an item is at least a header long and states a block count from 1 to
                      (in_len - 16) / 6, or the whole call is refused.  A container cut inside its header therefore travels padded
                      with zeros to MIN_ITEM bytes, and a header whose count the planner would not take travels with the nearest
                      count it does; the walk refuses both for the count (test_batch_faults_cpu.py checks that the oracle refuses
                      the padded form too)
  bad_places          batch_place_kernel (tsq_batch.cuh): what makes a place of the packed form bad
"""
from __future__ import annotations

import numpy as np

import fuzzgen
import kat
import mtgen
import streamgen

BLOCK = streamgen.BLOCK
SLOT = streamgen.OUTPUT_SZ
HEADER, MIN_FRAME = 16, 6
MIN_ITEM = HEADER + MIN_FRAME
OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_STALL = 0, 3, 4, 5, 7
SEED = 4170
N_CLEAN = 124
ALIGN = 16

REFUSED_CLASSES = ("twin_walk", "twin_stream", "damaged_refused", "tight")
ACCEPTED_CLASSES = ("clean", "uneven", "place", "damaged_valid")


def header_of(blob):
    """(magic ok, block count, total) of a container of at least 16 bytes"""
    return bytes(blob[:4]) == b"TSQ1", int.from_bytes(bytes(blob[4:8]), "little"), int.from_bytes(bytes(blob[8:16]), "little")


def stated_count(blob) -> int:
    """the block count the caller states for a container: the header's, brought into the range plan_batch takes"""
    return min(max(header_of(blob)[1], 1), (len(blob) - HEADER) // MIN_FRAME)


def walk_refuses(blob, n_blocks: int, cap: int) -> bool:
    """RE-DERIVE with batch_walk_kernel and walk_frames (tsq_format.h): the header (magic, a count and a total the container can hold), the count against the
    caller's, the total against the capacity, every frame (a stream of 3 .. TSQ_OUTPUT_SZ bytes inside the container, a block of at
    most 4 MiB, output that stays inside the total), and block sizes that add up to the total."""
    n = len(blob)
    if n < HEADER:
        return True
    magic, nb, total = header_of(blob)
    if not magic or nb == 0 or nb > (n - HEADER) // MIN_FRAME or total > nb * BLOCK:
        return True
    if nb != n_blocks or total > cap:
        return True
    at, oat = HEADER, 0
    for _ in range(n_blocks):
        if at + MIN_FRAME > n:
            return True
        stream_len = int.from_bytes(bytes(blob[at:at + 3]), "little") & 0x7FFFFF
        out_len = int.from_bytes(bytes(blob[at + 3:at + 6]), "little")
        if not 3 <= stream_len <= SLOT or at + 3 + stream_len > n or out_len > BLOCK or oat + out_len > total:
            return True
        oat += out_len
        at += 3 + stream_len
    return oat != total


class Item:
    """one container of the batch: `klass`, the bytes as they travel (`blob`), the stated block count, the room it is given, the
    verdict (`want`: its data, or None) and who refuses it (`by_walk`: the frame walk, so nothing may be written to its range)"""

    def __init__(self, name, klass, blob, cap, want):
        blob = bytes(blob)
        self.name, self.klass, self.cap, self.want = name, klass, int(cap), want
        self.blob = blob.ljust(MIN_ITEM, b"\0")
        self.n_blocks = stated_count(self.blob)
        self.by_walk = walk_refuses(self.blob, self.n_blocks, self.cap)
        assert not (self.by_walk and want is not None), name

    @property
    def refused(self) -> bool:
        return self.want is None

    @property
    def status(self) -> int:
        """what the library owes: the walk's code, the decoders' code, or 0"""
        return OK if not self.refused else ERR_FORMAT if self.by_walk else ERR_STREAM


def _clean_data(rng, k):
    n = int(rng.integers(1, 300_000)) if k % 8 == 0 else int(rng.integers(1, 2000)) if k % 8 == 1 else int(rng.integers(1, 24_000))
    kind = k % 3
    if kind == 0:
        return fuzzgen.structured(rng, n)
    if kind == 1:
        return kat.k7_textlike(n, seed=5000 + k)
    return kat.xorshift32_bytes(n, seed=91 + k)


def _capacity(blob, want) -> int:
    """room for a damaged container: what its header asks for where that is plausible, and at least what the oracle delivers"""
    _, nb, total = header_of(blob.ljust(HEADER, b"\0"))
    room = total if total <= max(nb, 1) * BLOCK and nb <= 64 else 0
    return max(room, len(want) if want is not None else 0, 1)


_BATCH = None


def batch(oracle):
    """-> [Item], made once per process"""
    global _BATCH
    if _BATCH is not None:
        return _BATCH
    rng = np.random.default_rng(SEED)
    accepted, refused = [], []
    for name, blob, k, how in mtgen.twin_containers():
        it = Item(f"twin_{name}_at_{k}", "twin_walk" if how == "walk" else "twin_stream", blob, _capacity(blob, None), None)
        assert it.by_walk == (how == "walk"), name
        refused.append(it)
    for name, blob in mtgen.damaged_containers():
        want = mtgen.expected_of_the_scheduler(oracle, blob)
        it = Item(name, "damaged_valid" if want is not None else "damaged_refused", blob, _capacity(blob, want), want)
        (accepted if want is not None else refused).append(it)
    clean = []
    for k in range(N_CLEAN):
        data = _clean_data(rng, k)
        clean.append(Item(f"clean_{k:03d}_{data.size}", "clean", oracle.compress(data, k & 1), data.size, data.tobytes()))
    blob, plain = mtgen._joined(streamgen.uneven_unit())
    clean.append(Item("uneven_unit", "uneven", blob, len(plain), plain))
    six, six_plain = mtgen.healthy_six()
    for k, (b, p) in enumerate(((six, six_plain), (clean[0].blob, clean[0].want), (clean[8].blob, clean[8].want))):
        clean.append(Item(f"place_{k}", "place", b, len(p), p))
    for k, src in enumerate((clean[16], Item("six", "clean", six, len(six_plain), six_plain))):
        refused.append(Item(f"tight_{k}_{src.name}", "tight", src.blob, src.cap - 1, None))
    accepted += [it for it in clean if it.klass != "place"]
    accepted = [accepted[i] for i in rng.permutation(len(accepted))]
    refused = [refused[i] for i in rng.permutation(len(refused))]
    # (the packed form refuses the place items: they go where the refused items have run out, with accepted items around them)
    for k, it in enumerate(it for it in clean if it.klass == "place"):
        accepted.insert(len(refused) + 10 + 20 * k, it)
    assert len(accepted) > len(refused) + 60
    out = []
    for k, it in enumerate(accepted):
        out.append(it)
        if k < len(refused):
            out.append(refused[k])
    _BATCH = out
    return out


def packed_layout(items, align: int = ALIGN):
    """the containers one after the other, each start a multiple of align -> (arena bytes, offsets, sizes)"""
    at, offsets = 0, []
    for it in items:
        at = -(-at // align) * align
        offsets.append(at)
        at += len(it.blob)
    arena = np.full(at, 0xEE, dtype=np.uint8)
    for it, o in zip(items, offsets):
        arena[o:o + len(it.blob)] = np.frombuffer(it.blob, dtype=np.uint8)
    return arena, offsets, [len(it.blob) for it in items]


def bad_places(items, offsets, sizes, arena_size: int):
    """RE-DERIVE with batch_place_kernel.  The tables of the packed form with the three `place` items' places falsified -> (offsets,
    sizes, {item index: what is wrong}): an offset past the arena (by the table's value only: offset + size ends behind the last byte
    of the allocation), a size below a header, and a size that cannot hold the stated block count (the six-block item)."""
    offsets, sizes, bad = list(offsets), list(sizes), {}
    places = [i for i, it in enumerate(items) if it.klass == "place"]
    multi = next(i for i in places if items[i].n_blocks > 1)
    past, short = [i for i in places if i != multi]
    offsets[past] = arena_size - 3
    bad[past] = "an offset past the arena"
    sizes[short] = HEADER - 1
    bad[short] = "a size below 16"
    sizes[multi] = HEADER + MIN_FRAME * items[multi].n_blocks - 1
    bad[multi] = "a size too short for the stated block count"
    return offsets, sizes, bad
