"""Seeded batches for the packed compress whose item table is made on the device (tsqa_compress_batch_packed_tables_async,
tsqa_plan_compress_tables), shared by test_compress_tables_cpu.py -- which shows from the restatement alone that each batch reaches
what it aims at -- and by test_gpu_compress_tables.py, which runs the same batches through the kernels.  Nothing here calls a kernel.
Expected containers are the oracle's, Oracle.compress(item bytes, ext): an item's container is that of its bytes alone.  Items are
text of 1 B to 4 KiB (turbosqueeze_amd.synth.text) unless a batch says otherwise, so that a block costs little.

What is restated from the library, and must be re-derived when it changes there:
  measure      batch_measure_tables_kernel (tsq_batch.cuh): size >= 1, size <= in_size, offset <= in_size - size; blocks = ceil(size / 4 MiB)
  layout       batch_layout_tables_kernel and tsqa_plan_compress_tables: the block sum over the accepted items, the fitting prefix
               that the first unfit item ends, and the bound: the sum of round_up(batch_bound(size), align) over the accepted items
  GROUP        batch_layout_tables_kernel and the pack scan are ONE workgroup of 256 threads that takes its items 256 at a time
  budget       an encode launch takes 2 x CUs blocks (tsqa_compress_batch_packed_tables_async); DEFAULT_BUDGET is the MI355X's
  packed       tsqa_plan_packed's rule, applied to the container sizes (a size of 0 takes no room)
  pieces       a header or frame is written only if it ends at or before out_size (batch_pack_scan_packed_body)
"""
from __future__ import annotations

import functools

import numpy as np

BLOCK = 1 << 22
OUTPUT_SZ = BLOCK + (BLOCK >> 2)
HEADER, FRAME_WORD = 16, 3
GROUP = 256
DEFAULT_BUDGET = 2 * 256
IN_MAX = 1 << 48
OK, ERR_ARG, ERR_OVERFLOW = 0, 3, 6
SEED = 7310
LOOP_COUNTS = (1, 255, 256, 257, 513)
ALIGNS = (1, 16, 4096)
EXTS = (0, 1)
U64 = 1 << 64


def round_up(v: int, align: int) -> int:
    return -(-v // align) * align


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def batch_bound(n: int) -> int:
    """RE-DERIVE with tsqa_batch_bound"""
    full, rest = divmod(n, BLOCK)
    return HEADER + full * (FRAME_WORD + OUTPUT_SZ) + ((FRAME_WORD + min(OUTPUT_SZ, 11 + rest + (rest >> 3) + (rest >> 1))) if rest else 0)


def measure(in_size: int, at: int, n: int) -> int:
    """RE-DERIVE with batch_measure_tables_kernel -> the blocks of an accepted item, 0 for a refused one.  at and n are 64-bit
    words: nothing is added that could wrap."""
    assert 0 <= at < U64 and 0 <= n < U64
    return -(-n // BLOCK) if 1 <= n <= in_size and at <= in_size - n else 0


def layout(in_offsets, in_sizes, in_size: int, align: int, cap_blocks: int):
    """RE-DERIVE with batch_layout_tables_kernel / tsqa_plan_compress_tables -> (first_block n + 1, item statuses, bound, n_fit)"""
    n, fb, bound = len(in_sizes), 0, 0
    first, status, n_fit = [], [], len(in_sizes)
    for i, (at, sz) in enumerate(zip(in_offsets, in_sizes)):
        nb = measure(in_size, at, sz)
        first.append(fb)
        if nb and n_fit == n and fb + nb > cap_blocks:
            n_fit = i
        status.append(ERR_ARG if nb == 0 else ERR_OVERFLOW if i >= n_fit else OK)
        fb += nb
        if nb:
            bound += round_up(batch_bound(sz), align)
    return first + [fb], status, bound, n_fit


def packed(sizes, align: int):
    """RE-DERIVE with tsqa_plan_packed"""
    at, offsets = 0, []
    for i, z in enumerate(sizes):
        offsets.append(at)
        at += z
        if i + 1 < len(sizes):
            at = round_up(at, align)
    return offsets + [at]


def pieces(blob: bytes):
    """the ends of a container's header and frames, in order"""
    nb = int.from_bytes(blob[4:8], "little")
    ends, at = [HEADER], HEADER
    for _ in range(nb):
        at += FRAME_WORD + (int.from_bytes(blob[at:at + FRAME_WORD], "little") & 0x7FFFFF)
        ends.append(at)
    assert at == len(blob)
    return ends


# ---- the oracle's containers ----------------------------------------------------------------------------------------------------------

_ORACLE = None


def _oracle():
    global _ORACLE
    if _ORACLE is None:
        from oracle.pyoracle import Oracle
        _ORACLE = Oracle()
    return _ORACLE


@functools.lru_cache(maxsize=None)
def container(data: bytes, ext: int) -> bytes:
    return _oracle().compress(data, ext, threads=4 if len(data) > BLOCK // 2 else 1)


@functools.lru_cache(maxsize=None)
def text(n: int, seed: int) -> bytes:
    from turbosqueeze_amd import synth
    return synth.text(n, seed=seed).tobytes()


POOL = 61


@functools.lru_cache(maxsize=None)
def _pool_lengths():
    return [int(x) for x in np.random.default_rng(SEED).integers(1, 4097, POOL)]


def small(k: int) -> bytes:
    """one of POOL texts of 1 B to 4 KiB: the batches share them, so the oracle compresses each once"""
    k %= POOL
    return text(_pool_lengths()[k], 100 + k)


# ---- batches --------------------------------------------------------------------------------------------------------------------------

REFUSAL_KINDS = ("size_0", "size_in_size_plus_1", "offset_one_past", "wraps", "size_2_63")


class Refused:
    """an item whose place the rule refuses; the words are made once in_size is known"""

    def __init__(self, kind):
        assert kind in REFUSAL_KINDS
        self.kind = kind

    def place(self, in_size: int):
        return {"size_0": (in_size // 2, 0), "size_in_size_plus_1": (0, in_size + 1), "offset_one_past": (in_size - 100 + 1, 100),
                "wraps": (U64 - 50, 100), "size_2_63": (0, 1 << 63)}[self.kind]


class Alias:
    """an item over the first `n` bytes of item `of`'s own bytes"""

    def __init__(self, of: int, n=None):
        self.of, self.n = of, n


class Lie:
    """an item whose size word is `size` at offset 0: refused whenever size > in_size"""

    def __init__(self, size):
        self.size = size


class Batch:
    """specs: bytes (the item's own data, laid one after the other into the input), Refused, Alias or Lie; slack: input bytes behind
    them that belong to no item"""

    def __init__(self, name, specs, align=16, slack=b""):
        self.name, self.align, self.specs = name, align, specs
        own = [s for s in specs if isinstance(s, bytes)]
        self.data = np.frombuffer(b"".join(own) + slack, dtype=np.uint8)
        self.in_size = in_size = self.data.size
        at, places = 0, []
        for s in specs:
            if isinstance(s, bytes):
                places.append((at, len(s)))
                at += len(s)
            else:
                places.append(None)
        for k, s in enumerate(specs):
            if isinstance(s, Refused):
                places[k] = s.place(in_size)
            elif isinstance(s, Alias):
                places[k] = (places[s.of][0], places[s.of][1] if s.n is None else s.n)
            elif isinstance(s, Lie):
                places[k] = (0, s.size)
        self.in_offsets = [p[0] for p in places]
        self.in_sizes = [p[1] for p in places]
        self.blocks = [measure(in_size, a, z) for a, z in places]
        self.need_blocks = sum(self.blocks)

    def item_bytes(self, i: int) -> bytes:
        assert self.blocks[i]
        return self.data[self.in_offsets[i]:self.in_offsets[i] + self.in_sizes[i]].tobytes()

    def containers(self, ext: int):
        """the oracle's container of every accepted item, None for a refused one"""
        return [container(self.item_bytes(i), ext) if nb else None for i, nb in enumerate(self.blocks)]

    def tables_u64(self):
        """-> (in_offsets, in_sizes) as uint64 arrays"""
        return np.array(self.in_offsets, dtype=np.uint64), np.array(self.in_sizes, dtype=np.uint64)

    def expect(self, ext: int, cap_blocks: int, out_size: int, measuring: bool = False):
        """-> dict of what the call owes: first_block, bound, status, sizes, offsets, and `writes`: per item the bytes of its
        container that land in the arena (the whole of it for status 0; for a fitting item that ends past out_size the header
        and the frames that end inside; nothing otherwise)"""
        first, status, bound, n_fit = layout(self.in_offsets, self.in_sizes, self.in_size, self.align, 0 if measuring else cap_blocks)
        n = len(self.specs)
        if measuring:
            return dict(first_block=first, bound=bound, status=status, sizes=[0] * n, offsets=[0] * (n + 1), writes=[0] * n, n_fit=n_fit)
        blobs = self.containers(ext)
        sizes = [len(blobs[i]) if st == OK else 0 for i, st in enumerate(status)]
        offsets = packed(sizes, self.align)
        writes = []
        for i, st in enumerate(status):
            if st != OK:
                writes.append(0)
                continue
            if offsets[i] + sizes[i] > out_size:
                status[i] = ERR_OVERFLOW
            writes.append(max([e for e in pieces(blobs[i]) if offsets[i] + e <= out_size], default=0))
        return dict(first_block=first, bound=bound, status=status, sizes=sizes, offsets=offsets, writes=writes, n_fit=n_fit)


def launches_of(b: Batch, budget: int, cap_blocks=None):
    """-> per item the encode launches its blocks lie in (a range; empty for an item without live blocks)"""
    first, status, _, _ = layout(b.in_offsets, b.in_sizes, b.in_size, b.align, b.need_blocks if cap_blocks is None else cap_blocks)
    return [range(first[i] // budget, (first[i + 1] - 1) // budget + 1) if st == OK else range(0) for i, st in enumerate(status)]


@functools.lru_cache(maxsize=None)
def loop_edges():
    """1, 255, 256, 257 and 513 small items: the 256-lane passes of the layout scan and of the pack scan"""
    return tuple(Batch(f"loop_edges_{n}", [small(k) for k in range(n)]) for n in LOOP_COUNTS)


def launch_counts(budget: int):
    return (budget - 1, budget, budget + 1, 2 * budget + 1)


@functools.lru_cache(maxsize=None)
def launch_edges(budget: int):
    """one-block items around one and two launches; a two-block item whose blocks straddle the first launch edge; a three-block
    item at index 0"""
    out = [Batch(f"launch_edges_{n}", [small(7 * k) for k in range(n)]) for n in launch_counts(budget)]
    out.append(Batch("launch_straddle", [small(3 * k) for k in range(budget - 1)] + [text(BLOCK + 1, 950)] + [small(k) for k in range(3)]))
    out.append(Batch("three_blocks_first", [text(2 * BLOCK + 1, 951)] + [small(k) for k in range(4)]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def refusals(budget: int):
    """every kind of refusal between healthy one-block items: at index 0, directly behind the item that ends the first launch (two
    of them there), in the middle, and at the last index"""
    specs = [Refused("size_0")] + [small(5 * k) for k in range(budget)]
    specs += [Refused("size_in_size_plus_1"), Refused("offset_one_past")] + [small(k) for k in range(3)]
    specs += [Refused("wraps")] + [small(k) for k in range(3, 6)] + [Refused("size_2_63")]
    return Batch("refusals", specs)


@functools.lru_cache(maxsize=None)
def refused_run():
    """300 refused items in a row, longer than one pass of either scan, between healthy items"""
    return Batch("refused_run", [small(k) for k in range(3)] + [Refused(REFUSAL_KINDS[k % 5]) for k in range(300)] + [small(k) for k in range(3, 6)])


@functools.lru_cache(maxsize=None)
def all_refused():
    """nothing but refused items: no live block at all, and the tables are still owed"""
    return Batch("all_refused", [Refused(k) for k in REFUSAL_KINDS], slack=small(0))


CUT_BIG_AT = 5


@functools.lru_cache(maxsize=None)
def cuts_batch():
    """ten items, the sixth of two blocks"""
    specs = [small(11 * k) for k in range(10)]
    specs[CUT_BIG_AT] = text(BLOCK + 1, 950)
    return Batch("cuts", specs)


def cap_cuts(budget: int):
    """-> (batch, [(what, cap_blocks, n_fit)])"""
    b = cuts_batch()
    n, need = len(b.specs), b.need_blocks
    return b, [("exactly the blocks needed", need, n), ("one block less", need - 1, n - 1),
               ("between the two blocks of item 5: it ends the prefix although item 6 would fit", CUT_BIG_AT + 1, CUT_BIG_AT),
               ("one block", 1, 1), ("two dead launches and a dead tail", need + 2 * budget + 1, n)]


def arena_cuts(ext: int):
    """-> (batch, [(what, out_size)]) around item 5 (k), whose container has two frames"""
    b = cuts_batch()
    e = b.expect(ext, b.need_blocks, 1 << 40)
    used, at = e["offsets"][-1], e["offsets"][CUT_BIG_AT]
    ends = pieces(b.containers(ext)[CUT_BIG_AT])
    return b, [("used", used), ("used - 1", used - 1), ("the end of item 5's header", at + HEADER),
               ("the middle of item 5's first frame", at + (ends[0] + ends[1]) // 2), ("the end of item 5's first frame", at + ends[1]),
               ("a header and no more", 16)]


@functools.lru_cache(maxsize=None)
def _text_with_container_size(target: int, ext: int) -> bytes:
    """text whose container has exactly `target` bytes: the size grows with the length by small steps, so bisect, then look around"""
    for seed in range(400, 420):
        lo, hi = 1, 4 * target + 64
        while lo < hi:
            mid = (lo + hi) // 2
            if len(container(text(mid, seed), ext)) < target:
                lo = mid + 1
            else:
                hi = mid
        for n in range(max(1, lo - 48), lo + 48):
            if len(container(text(n, seed), ext)) == target:
                return text(n, seed)
    raise AssertionError(f"no text with a container of {target} bytes (ext {ext})")


@functools.lru_cache(maxsize=None)
def alignment(align: int):
    """for each ext, containers of k * align - 1, k * align and k * align + 1 bytes, each followed by a small item"""
    k = {1: 50, 16: 3, 4096: 1}[align]                     # (sizes every text length reaches: 41 and 74 are skipped)
    specs = []
    for ext in EXTS:
        for d in (-1, 0, 1):
            specs += [_text_with_container_size(k * align + d, ext), small(len(specs))]
    return Batch(f"alignment_{align}", specs, align)


@functools.lru_cache(maxsize=None)
def overlaps():
    """two items over the same bytes, and an item that is a prefix of another"""
    return Batch("overlaps", [small(1), small(2), Alias(1), small(3), Alias(3, 17), Alias(0)])


LIES = (1 << 54, (1 << 54) + BLOCK, (1 << 54) - 1, (1 << 63) + 5, U64 - 1)


@functools.lru_cache(maxsize=None)
def lying():
    """sizes whose blocks, were they counted, would wrap a 32-bit sum back to a small number (2^54 B = 2^32 blocks), between
    healthy items"""
    specs = [small(0), Lie(LIES[0]), small(1), Lie(LIES[1]), Lie(LIES[2]), small(2), Lie(LIES[3]), Lie(LIES[4]), small(3)]
    return Batch("lying", specs)


def every_batch(budget: int = DEFAULT_BUDGET):
    return (list(loop_edges()) + list(launch_edges(budget)) + [refusals(budget), refused_run(), cuts_batch()] +
            [alignment(a) for a in ALIGNS] + [overlaps(), lying()])
