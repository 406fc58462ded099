"""Seeded cases for the record tables (tsqa_plan_records, tsqa_records_async, tsqa_records): where the records of an index's data
are, for a delimiter byte.  Shared by test_records_cpu.py -- which shows with the oracle, the host frame walk and the host-only
planners that each case reaches what it aims at -- and by test_gpu_records.py, which runs the same cases through the kernels.
Nothing here calls a kernel.  An index is gathergen's Index (what a tsqa_index holds of its data); the sources are the existing
generators' where they fit (cutgen's 600 tiny blocks, its 257 blocks of 4 096 bytes, its two blocks of 4 MiB + 1; joingen's ragged
arena of 1 to 40 byte items; gathergen's batch of 300 containers with six of densegen's damaged headers; mtgen's cut containers,
which only the frame walk refuses, and its stream twins; the refused sized index) and small containers made here with the oracle.
The expected tables are made here in numpy from the sources' BYTES alone, by the rule of include/turbosqueeze_amd.h.

What is restated from the library, and must be re-derived when it changes there:
  restate      the rule: per item, a record starts at byte 0 and behind every delimiter but one at the item's last byte, and ends in
               front of the next delimiter or at the item's end; numbered item by item; the two flags; the prefix below cap_records;
               d_item_first_record, both need words and the status
  OUTC, RING   the decoder's chunk holds at most 12 288 output bytes (SymCfg::OUTC) and its ring 77 888 (SymCfg::R): where the
               ring-wrap case puts its delimiters
  GROUP, SPLIT the table launches take 256 blocks per workgroup and 256 groups per pass; group_scan_excl64 sums v & 0xFFFFFF and
               v >> 24 apart
"""
from __future__ import annotations

import functools

import numpy as np

import cutgen as cg
import densegen as dg
import gathergen as gg
import joingen as jg
import mtgen
import splitgen as sg

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = gg.OK, gg.ERR_ARG, gg.ERR_FORMAT, gg.ERR_STREAM, gg.ERR_OVERFLOW
KEEP_DELIM, FLAT = 1, 2
FLAGS = (0, KEEP_DELIM, FLAT, KEEP_DELIM | FLAT)
DELIMS = (0, 10, 255)
OUTC, RING = 12288, 77888
GROUP, SPLIT = 256, 1 << 24
SEED = 9310
BLOCK = 1 << 22
ITEM_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097)
PLACES = ("first", "last", "both", "nowhere", "everywhere")
COUNTS = jg.COUNTS
BIG_BLOCKS = (65535, 65536, 65537)
BIG_LEN = 4096


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def item_records(data, delim: int, keep: bool):
    """RE-DERIVE with the rule -> (starts, lengths) of the records of ONE item's bytes (a uint8 array), as int64 arrays"""
    t = data.size
    if t == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pos = np.flatnonzero(data == delim).astype(np.int64)
    starts = np.concatenate([np.zeros(1, np.int64), pos + 1])
    if pos.size and pos[-1] == t - 1:                    # a terminator at the last byte starts no record
        starts = starts[:-1]
        ends, kept = pos, np.full(pos.size, int(keep), np.int64)
    else:                                                # the last record needs no terminator
        ends, kept = np.concatenate([pos, np.array([t], np.int64)]), np.concatenate([np.full(pos.size, int(keep), np.int64), np.zeros(1, np.int64)])
    return starts, ends - starts + kept


def restate(idx: gg.Index, delim: int, flags: int = 0, cap=None, data=None):
    """RE-DERIVE with tsqa_records_async -> dict: items, offsets, lengths (int64 arrays: the records below cap, all when cap is
    None), item_first (n_items + 1), need [the count, the largest length], status"""
    n_items = idx.n_items
    if idx.refused:
        return dict(items=np.zeros(0, np.int64), offsets=np.zeros(0, np.int64), lengths=np.zeros(0, np.int64), item_first=[0] * (n_items + 1),
                    need=[0, 0], status=ERR_FORMAT)
    src = np.frombuffer(idx.data, dtype=np.uint8) if data is None else data
    first, longest, written, parts = [0], 0, 0, []
    for i in range(n_items):
        a, t = idx.item_span(i) if idx.item_first[i] < idx.item_first[i + 1] else (0, 0)
        starts, lens = item_records(src[a:a + t], delim, bool(flags & KEEP_DELIM))
        if lens.size:
            longest = max(longest, int(lens.max()))
        take = starts.size if cap is None else max(0, min(starts.size, cap - written))
        if take:
            parts.append((np.full(take, i, np.int64), starts[:take] + (a if flags & FLAT else 0), lens[:take]))
            written += take
        first.append(first[-1] + starts.size)
    cat = lambda k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, np.int64)
    return dict(items=cat(0), offsets=cat(1), lengths=cat(2), item_first=first, need=[first[-1], longest],
                status=OK if cap is None or first[-1] <= cap else ERR_OVERFLOW)


class Case:
    """an index and a delimiter"""

    def __init__(self, name: str, index: gg.Index, delim: int):
        self.name, self.index, self.delim = name, index, int(delim)
        self._expect = {}

    def expect(self, flags: int = 0, cap=None):
        key = (flags, cap)
        if key not in self._expect:
            self._expect[key] = restate(self.index, self.delim, flags, cap)
        return self._expect[key]

    def item_at(self):
        """the items' starts in the concatenation, n_items + 1, as tsqa_plan_records takes them (a refused item: where the next starts)"""
        i = self.index
        return [i.out_start[fb] for fb in i.item_first]

    def item_status(self):
        i = self.index
        return [0 if i.item_first[k] < i.item_first[k + 1] else ERR_FORMAT for k in range(i.n_items)]      # (no case has an empty item)


# ---- sources made here ------------------------------------------------------------------------------------------------------------------

def _oracle():
    return dg._oracle()


def plain_of(name: str, data, ext: int = 1) -> gg.Index:
    """one container of `data` (a uint8 array) as the oracle compresses it, through tsqa_index_create"""
    blob = _oracle().compress(data, ext, threads=4 if data.size > BLOCK // 2 else 1)
    _, out_start = cg.walk(blob)
    return gg.Index(name, "plain", bytes(blob), data.tobytes(), out_start)


def batch_of(name: str, blobs, datas) -> gg.Index:
    """containers in one arena at multiples of 16, through tsqa_index_create_batch; datas[k] None: a container the index refuses"""
    at, spans = 0, []
    for b in blobs:
        at = gg.round_up(at, 16)
        spans.append((at, len(b)))
        at += len(b)
    arena = np.full(at, 0xEE, dtype=np.uint8)
    for (o, n), b in zip(spans, blobs):
        arena[o:o + n] = np.frombuffer(b, dtype=np.uint8)
    out_start, item_first, cat = [], [], bytearray()
    for b, d in zip(blobs, datas):
        item_first.append(len(out_start))
        if d is None:
            continue
        _, starts = cg.walk(b)
        out_start += [len(cat) + s for s in starts[:-1]]
        cat += d
    item_first.append(len(out_start))
    out_start.append(len(cat))
    return gg.Index(name, "batch", arena.tobytes(), bytes(cat), out_start, item_first=item_first, spans=spans)


def filler(n: int, seed: int):
    """n seeded bytes none of which is 0, 10 or 255"""
    v = np.random.default_rng(seed).integers(1, 253, n, dtype=np.uint8)          # 1 .. 252
    v[v >= 10] += 1                                                                # 1 .. 9, 11 .. 253
    return v


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def places(delim: int) -> Case:
    """1: fifty items in one batch: every length of ITEM_LENGTHS with the delimiter at byte 0, at the last byte, at both, nowhere and
    everywhere (a length of 1: first, last and both are the same item)"""
    blobs, datas = [], []
    for n in ITEM_LENGTHS:
        for k, where in enumerate(PLACES):
            d = filler(n, SEED + 7 * n + k)
            if where in ("first", "both"):
                d[0] = delim
            if where in ("last", "both"):
                d[-1] = delim
            if where == "everywhere":
                d[:] = delim
            blobs.append(bytes(_oracle().compress(d, (n + k) & 1, threads=1)))
            datas.append(d.tobytes())
    return Case(f"places_delim_{delim}", batch_of(f"places_{delim}", blobs, datas), delim)


@functools.lru_cache(maxsize=None)
def ragged(n: int) -> Case:
    """2: joingen's ragged arena of n items of 1 to 40 bytes as a batch index: one block per item, so dozens of blocks lie inside
    one 64-position span of the concatenation -- the `+ b` of the bit map's word number keeps their words apart.  delim: a space"""
    c = jg.counts()[COUNTS.index(n)]
    out_start = [0]
    for it in c.items:
        out_start.append(out_start[-1] + len(it.data))
    idx = gg.Index(f"ragged_{n}", "batch", c.arena.tobytes(), c.data(), out_start, item_first=list(range(n + 1)),
                   spans=list(zip(c.offsets, c.sizes)))
    return Case(f"ragged_{n}", idx, 0x20)


@functools.lru_cache(maxsize=None)
def tiny() -> Case:
    """2: cutgen's 600 blocks of 1 to 40 bytes in ONE container: records that run across dozens of blocks"""
    return Case("tiny_600", gg.tiny(), 0x20)


CHUNK_N = 3 * OUTC + 5
CHUNK_KINDS = ("text", "random", "zeros", "random_drawn")


@functools.lru_cache(maxsize=None)
def chunk_edges(kind: str) -> Case:
    """3: 3 x 12 288 + 5 bytes, more than three chunks whatever the decoder's chunking: text (delim: newline), random bytes with the
    delimiter a byte of the data, zeros with delim 0 -- EVERY byte is a delimiter, so the first and the last byte of every chunk
    are, wherever the chunks end, and a chunk holds OUTC of them -- and random bytes with a drawn delimiter"""
    rng = np.random.default_rng(SEED + 3)
    if kind == "text":
        data, delim = dg._text(CHUNK_N, SEED), 10
    elif kind == "zeros":
        data, delim = np.zeros(CHUNK_N, dtype=np.uint8), 0
    else:
        data = rng.integers(0, 256, CHUNK_N, dtype=np.uint8)
        delim = int(data[OUTC]) if kind == "random" else int(rng.integers(0, 256))
    return Case(f"chunk_edges_{kind}", plain_of(f"chunks_{kind}", data), delim)


RING_N = 1 << 18
RING_DELIMS = sorted({k * RING + d for k in (1, 2, 3) for d in (-1, 0, 1)} | {65535, 65536})


@functools.lru_cache(maxsize=None)
def ring_wrap() -> Case:
    """4: one block of 2^18 bytes of text without newlines, with newlines at k * 77 888 - 1, k * 77 888 and k * 77 888 + 1 -- where the
    ring wraps when its skew is 0 -- and at 65 535 and 65 536"""
    data = dg._text(RING_N, SEED + 4).copy()
    data[data == 10] = 0x20
    data[RING_DELIMS] = 10
    return Case("ring_wrap", plain_of("ring_wrap", data), 10)


SKEW_ITEMS = (1, 200000, 37, 200000)


def skew_delims(a: int, n: int):
    """the places, inside an item of n bytes that starts at byte `a` of the concatenation, whose ring addresses are R - 1, 0 and 1:
    the decoder skews the ring by the block's start mod 64, so position p of the block lies at ring address (p + a % 64) mod R"""
    return sorted({k * RING - a % 64 + d for k in (1, 2) for d in (-1, 0, 1) if 0 <= k * RING - a % 64 + d < n} | {65535, 65536})


@functools.lru_cache(maxsize=None)
def ring_wrap_skewed() -> Case:
    """4: the ring wrap with a skew that is not 0: a batch of items of 1, 200 000, 37 and 200 000 bytes, so the two long blocks
    start at bytes 1 and 200 038 of the concatenation (1 and 38 mod 64) and are longer than the ring; text without newlines, with
    newlines where the ring address is R - 1, 0 and 1, and at 65 535 and 65 536 of each item"""
    blobs, datas, at = [], [], 0
    for k, n in enumerate(SKEW_ITEMS):
        d = dg._text(n, SEED + 40 + k).copy()
        d[d == 10] = 0x20
        if n > RING:
            d[skew_delims(at, n)] = 10
        blobs.append(bytes(_oracle().compress(d, 1, threads=1)))
        datas.append(d.tobytes())
        at += n
    return Case("ring_wrap_skewed", batch_of("ring_wrap_skewed", blobs, datas), 10)


@functools.lru_cache(maxsize=None)
def two_blocks() -> Case:
    """4: cutgen's 4 MiB + 1 random bytes: two blocks, the second one byte long; the delimiter is drawn so that the last record
    before the edge runs across it"""
    s = cg.two_blocks()
    data = np.frombuffer(s.data, dtype=np.uint8)
    delim = next(d for d in range(256) if data[BLOCK - 1] != d and data[BLOCK] != d)
    return Case("two_blocks", gg.from_source(s, "plain"), delim)


@functools.lru_cache(maxsize=None)
def short_blocks(kind: str) -> Case:
    """5: cutgen's 257 blocks of 4 096 bytes through a sized index and through tsqa_index_create"""
    return Case(f"split_{kind}", gg.split(kind), 10)


CARRY_ITEMS, CARRY_UNIT = 300, 1 << 16


@functools.lru_cache(maxsize=None)
def carries(front: bool) -> Case:
    """6: 300 items of 2^16 zero bytes with delim 0: 19.66 million records, and d_item_first_record passes 2^24 at item 256 -- the
    first lane of the second pass over the groups.  front: one item of 66 x 2^16 zeros in front (two blocks: 64 and 2 units), so that
    the block whose first record is number 2^24 is block 192, the first lane of the fourth wavefront"""
    unit = np.zeros(CARRY_UNIT, dtype=np.uint8)
    one = bytes(_oracle().compress(unit, 1, threads=1))
    blobs, datas = [one] * CARRY_ITEMS, [unit.tobytes()] * CARRY_ITEMS
    if front:
        big = np.zeros(66 * CARRY_UNIT, dtype=np.uint8)
        blobs, datas = [bytes(_oracle().compress(big, 1, threads=4))] + blobs, [big.tobytes()] + datas
    name = "carry_at_a_wavefront_edge" if front else "carry_between_passes"
    return Case(name, batch_of(name, blobs, datas), 0)


CARRY_CAP = 1000


@functools.lru_cache(maxsize=None)
def damaged() -> Case:
    """7: gathergen's batch of 300 containers with densegen's damaged headers, reordered so that the refused ones are items 0 (refused
    by the frame walk), 17, 100, 255, 256 (by the walk) and 299: these give no records, and every other item stays exact"""
    b = gg.batch()
    order = list(range(gg.BATCH_ITEMS))
    order[0], order[101] = order[101], order[0]
    blocks = lambda i: b.item_first[i + 1] - b.item_first[i]
    out_start, item_first, cat = [], [], bytearray()
    for i in order:
        item_first.append(len(out_start))
        if not blocks(i):
            continue
        a, t = b.item_span(i)
        out_start += [len(cat) + (s - a) for s in b.out_start[b.item_first[i]:b.item_first[i + 1]]]
        cat += b.data[a:a + t]
    item_first.append(len(out_start))
    out_start.append(len(cat))
    idx = gg.Index("batch300_reordered", "batch", b.blob, bytes(cat), out_start, item_first=item_first, spans=[b.spans[i] for i in order])
    return Case("damaged_items", idx, 0x20)


DAMAGED_AT = (0, 17, 100, 255, 256, 299)


CUT_AT = {0: "cut_in_size_word", 100: "cut_in_frame_word", 256: "cut_mid_stream", 299: "cut_at_frame_end"}


@functools.lru_cache(maxsize=None)
def cut_items() -> Case:
    """7: 300 items, joingen's small ones, with mtgen's cut containers -- whole headers that state the true count and total, the
    bytes cut off inside a frame word, inside a stream's size word, in the middle of a stream and at a frame's end: only the frame
    walk refuses them -- as items 0, 100, 256 (the first lane of the second pass) and 299 (the last).  These give no records, and
    every other item stays exact"""
    cut = dict(mtgen.header_and_tail_cases())
    blobs, datas = [], []
    for k in range(300):
        if k in CUT_AT:
            blobs.append(bytes(cut[CUT_AT[k]])); datas.append(None)
        else:
            it = jg.tiny(k)
            blobs.append(it.blob); datas.append(it.data)
    return Case("cut_items", batch_of("cut_items", blobs, datas), 0x20)


FLIP_FROM = 400


@functools.lru_cache(maxsize=None)
def flipped():
    """7: the container of chunk_edges('text') with ONE byte of its stream flipped (all eight bits), the first byte from offset 400
    on at which the oracle's decoder refuses the block; the header and the frame word are whole, so the index is made and only a
    decoder meets the damage -> (name, container, offset)"""
    good = chunk_edges("text").index.blob
    for at in range(FLIP_FROM, len(good)):
        bad = good[:at] + bytes([good[at] ^ 0xFF]) + good[at + 1:]
        if _oracle().decompress(bad, threads=1) is None:
            return "flipped_text", bad, at
    raise AssertionError("no flip of one stream byte is refused by the oracle")


@functools.lru_cache(maxsize=None)
def refused_case() -> Case:
    """7: a sized index whose container the device refuses (one of seekgen's false tables): TSQA_ERR_FORMAT and zeros"""
    return Case("refused_index", gg.refused(), 10)


def healthy_cases():
    """every case whose index can be made from host bytes and is not refused"""
    return ([places(d) for d in DELIMS] + [ragged(n) for n in COUNTS] + [tiny()] + [chunk_edges(k) for k in CHUNK_KINDS] +
            [ring_wrap(), ring_wrap_skewed(), two_blocks(), short_blocks("sized"), short_blocks("plain"), damaged(), cut_items()])


def caps(case: Case):
    """8: -> [(what, cap_records)]: exact, one short, ending inside a middle item, 0"""
    e = case.expect()
    n, first = e["need"][0], e["item_first"]
    n_items = len(first) - 1
    mid = next((i for i in list(range(n_items // 2, n_items)) + list(range(n_items // 2)) if first[i + 1] - first[i] >= 2), None)
    inside = first[mid] + 1 if mid is not None else n // 2   # (no item with two records: a cap in the middle of the table)
    return [("exactly the records", n), ("one short", n - 1), ("ending inside a middle item", inside), ("none", 0)]
