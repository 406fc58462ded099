"""Seeded cases for the find (tsqa_plan_find, tsqa_find_async, tsqa_find): where a byte string of 1 to 16 bytes occurs in an index's
data.  Shared by test_find_cpu.py -- which holds the host-only rule against the restatement below and shows that each case reaches
what it aims at -- and by test_gpu_find.py, which runs the same cases through the kernels.  Nothing here calls a kernel.  An index is
gathergen's Index; the sources are the existing generators' where they fit (recordgen's chunk-edge containers, its carries, its
damaged batch of 300 from gathergen and densegen; cutgen's two blocks of 4 MiB + 1; splitgen's phrase; joingen's ragged lengths;
mtgen's twins and the refused sized index through recordgen) and small containers made here with the oracle, one of them assembled
by hand in cutgen's manner.  The expected tables are made here from the sources' BYTES alone: per item a loop of bytes.find that
advances by 1.

What is restated from the library, and must be re-derived when it changes there:
  restate      the rule (include/turbosqueeze_amd.h): a hit is (i, p) with p + m <= T_i and D_i[p .. p + m) == needle; overlapping hits
               all count; none crosses an item; a refused item has none; numbered item by item and by p; the flat flag; the prefix
               below cap_hits; d_item_first_hit, the need word and the status
  CELL         flush_find walks an image by the aligned 16-byte ring cells it touches and reads the cell in front: where the
               cell-edge case puts its hits (every residue mod 16, and 62 .. 66 around a map word's edge)
  OUTC, RING   the decoder's chunk holds at most 12 288 output bytes (SymCfg::OUTC) and its ring 77 888 (SymCfg::R); the ring's skew
               is the block's out_at & 63: where the ring-wrap cases put their needles
  EDGE         the seam launch sees 15 bytes of each end of a block (needles of up to 16 bytes)
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
import recordgen as rg
import splitgen as sg

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = gg.OK, gg.ERR_ARG, gg.ERR_FORMAT, gg.ERR_STREAM, gg.ERR_OVERFLOW
FLAT = 2
FLAGS = (0, FLAT)
MAX_NEEDLE = 16
CELL, EDGE = 16, 15
OUTC, RING = rg.OUTC, rg.RING
GROUP, SPLIT = rg.GROUP, rg.SPLIT
SEED = 9520
BLOCK = 1 << 22
NEEDLE_LENGTHS = (1, 2, 3, 4, 5, 8, 15, 16)
ITEM_LENGTHS = (15, 16, 17, 63, 64, 65, 4095, 4096, 4097)     # and m - 1, m, m + 1 for the needle's m
PLACES = ("first", "last", "both", "nowhere", "everywhere")
COUNTS = jg.COUNTS
BIG_BLOCKS, BIG_LEN = rg.BIG_BLOCKS, rg.BIG_LEN
CARRY_CAP = 1000


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=64)
def item_hits(data: bytes, needle: bytes):
    """RE-DERIVE with the rule -> the places of `needle` in ONE item's bytes, as an int64 array: bytes.find, advancing by 1"""
    out, p = [], data.find(needle)
    while p >= 0:
        out.append(p)
        p = data.find(needle, p + 1)
    return np.array(out, dtype=np.int64)


def restate(idx: gg.Index, needle: bytes, flags: int = 0, cap=None, data=None):
    """RE-DERIVE with tsqa_find_async -> dict: items, offsets (int64 arrays: the hits below cap, all when cap is None), item_first
    (n_items + 1), need [the count], status"""
    n_items = idx.n_items
    if idx.refused:
        return dict(items=np.zeros(0, np.int64), offsets=np.zeros(0, np.int64), item_first=[0] * (n_items + 1), need=[0], status=ERR_FORMAT)
    src = idx.data if data is None else data
    first, written, parts = [0], 0, []
    for i in range(n_items):
        a, t = idx.item_span(i) if idx.item_first[i] < idx.item_first[i + 1] else (0, 0)
        hits = item_hits(bytes(src[a:a + t]), needle) if data is None else item_hits.__wrapped__(src[a:a + t], needle)   # (not kept: may be large)
        take = hits.size if cap is None else max(0, min(hits.size, cap - written))
        if take:
            parts.append((np.full(take, i, np.int64), hits[:take] + (a if flags & FLAT else 0)))
            written += take
        first.append(first[-1] + hits.size)
    cat = lambda k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, np.int64)
    return dict(items=cat(0), offsets=cat(1), item_first=first, need=[first[-1]], status=OK if cap is None or first[-1] <= cap else ERR_OVERFLOW)


class Case(rg.Case):
    """an index and a needle (item_at and item_status: recordgen's)"""

    def __init__(self, name: str, index: gg.Index, needle: bytes):
        self.name, self.index, self.needle = name, index, bytes(needle)
        assert 1 <= len(self.needle) <= MAX_NEEDLE
        self._expect = {}

    def expect(self, flags: int = 0, cap=None):
        key = (flags, cap)
        if key not in self._expect:
            self._expect[key] = restate(self.index, self.needle, flags, cap)
        return self._expect[key]


def blocks_of_hit(idx: gg.Index, at: int, m: int) -> int:
    """in how many blocks the bytes [at, at + m) of the concatenation lie (empty blocks in between hold none of them)"""
    return len({gg.block_of(idx.out_start, p) for p in range(at, at + m)})


def _oracle():
    return dg._oracle()


# ---- 1: lengths and places --------------------------------------------------------------------------------------------------------------

def mixed_needle(m: int) -> bytes:
    """m bytes of 0 and 10 that no shift of itself matches: one 10, then zeros"""
    return bytes([10] + [0] * (m - 1))


def equal_needle(m: int) -> bytes:
    return bytes([255]) * m


def place_lengths(m: int):
    return tuple(sorted({n for n in (m - 1, m, m + 1) + ITEM_LENGTHS if n >= 1}))


@functools.lru_cache(maxsize=None)
def places_index(m: int) -> gg.Index:
    """per item length and place one item of recordgen's filler (no byte of it is 0, 10 or 255): mixed_needle(m) written at byte 0, at
    the item's end, at both, nowhere -- where the item has room for it --, and an item of 255 throughout, in which equal_needle(m)
    occurs at EVERY place"""
    blobs, datas, nd = [], [], np.frombuffer(mixed_needle(m), dtype=np.uint8)
    for n in place_lengths(m):
        for k, where in enumerate(PLACES):
            d = rg.filler(n, SEED + 7 * n + k + 1000 * m)
            if n >= m and where in ("first", "both"):
                d[:m] = nd
            if n >= m and where in ("last", "both"):
                d[n - m:] = nd
            if where == "everywhere":
                d[:] = 255
            blobs.append(bytes(_oracle().compress(d, (n + k) & 1, threads=1)))
            datas.append(d.tobytes())
    return rg.batch_of(f"find_places_{m}", blobs, datas)


def places(m: int, everywhere: bool) -> Case:
    return Case(f"places_m{m}_{'equal' if everywhere else 'mixed'}", places_index(m), equal_needle(m) if everywhere else mixed_needle(m))


# ---- 2: cell and word edges ---------------------------------------------------------------------------------------------------------------

CELL_ITEM = 200
CELL_STARTS = (0, 1, 38, 63)
CELL_NEEDLES = (3, 16)


def cell_runs(m: int):
    """-> [(first byte, length)] of the runs of 255 in the item of 200 bytes: one run that gives hits ENDING at 62, 63, 64, 65 and 66,
    and runs of exactly m bytes -- one hit each -- whose ends take the residues mod 16 that are still missing, as far as the item
    has room (a byte apart at least, so that no run meets another)"""
    runs = [(62 - (m - 1), m + 4)]
    seen = {e % CELL for e in range(62, 67)}
    taken = lambda a, n: any(a <= b + k and b <= a + n for b, k in runs)          # (touching counts as meeting)
    for e in range(m - 1, CELL_ITEM):
        a = e - (m - 1)
        if e % CELL not in seen and not taken(a, m):
            runs.append((a, m))
            seen.add(e % CELL)
    return sorted(runs)


@functools.lru_cache(maxsize=None)
def cell_edges(m: int, start: int) -> Case:
    """a batch of a pad item of `start` bytes (none at 0) and ONE item of 200 bytes that starts at byte `start` of the concatenation,
    filler with cell_runs(m) of 255; the needle: m times 255"""
    d = rg.filler(CELL_ITEM, SEED + 31 * m + start)
    for a, n in cell_runs(m):
        d[a:a + n] = 255
    parts = ([rg.filler(start, SEED + start)] if start else []) + [d]
    blobs = [bytes(_oracle().compress(p, k & 1, threads=1)) for k, p in enumerate(parts)]
    return Case(f"cell_edges_m{m}_at_{start}", rg.batch_of(f"find_cells_{m}_{start}", blobs, [p.tobytes() for p in parts]), equal_needle(m))


# ---- 3: chunk edges -----------------------------------------------------------------------------------------------------------------------

CHUNK_CASES = ("zeros_2", "zeros_16", "random_4", "text_3")


@functools.lru_cache(maxsize=None)
def chunk_edges(kind: str) -> Case:
    """recordgen's containers of 3 x 12 288 + 5 bytes: zeros with needles of 2 and 16 zeros -- a hit ends at every position from m - 1
    on, wherever the decoder cuts its chunks --, random bytes with the 4 bytes around position OUTC, text with its most frequent 3
    bytes"""
    if kind.startswith("zeros"):
        return Case(f"chunks_{kind}", rg.chunk_edges("zeros").index, bytes(int(kind.split("_")[1])))
    if kind == "random_4":
        idx = rg.chunk_edges("random").index
        return Case("chunks_random_4", idx, idx.data[OUTC - 2:OUTC + 2])
    idx = rg.chunk_edges("text").index
    d = np.frombuffer(idx.data, dtype=np.uint8).astype(np.int64)
    tri = (d[:-2] << 16) | (d[1:-1] << 8) | d[2:]
    vals, counts = np.unique(tri, return_counts=True)
    v = int(vals[int(np.argmax(counts))])
    return Case("chunks_text_3", idx, bytes([v >> 16, (v >> 8) & 255, v & 255]))


# ---- 4: the ring wrap ---------------------------------------------------------------------------------------------------------------------

RING_N = 1 << 18
RING_M = 16


def ring_starts(skew: int, n: int):
    """the starts k * R - skew - j, j = 0 .. 16, inside a block of n bytes whose ring is skewed by `skew`: needles of 16 bytes that
    end just in front of the ring's wrap, lie across it by every split, and start right on it; and 65 528, across 65 535 | 65 536"""
    out = {k * RING - skew - j for k in (1, 2, 3) for j in range(17)}
    return sorted({s for s in out if 0 <= s and s + RING_M <= n} | {65536 - 8})


def _ring_block(n: int, skew: int, seed: int):
    """n bytes of text without 255, with 255 over every needle of ring_starts (the starts are consecutive, so each k gives one run of 32)"""
    d = dg._text(n, seed).copy()
    d[d == 255] = 0x20
    for s in ring_starts(skew, n):
        d[s:s + RING_M] = 255
    return d


@functools.lru_cache(maxsize=None)
def ring_wrap() -> Case:
    """one block of 2^18 bytes at byte 0 of the concatenation: the skew is 0"""
    return Case("ring_wrap", rg.plain_of("find_ring_wrap", _ring_block(RING_N, 0, SEED + 4)), equal_needle(RING_M))


@functools.lru_cache(maxsize=None)
def ring_wrap_skewed() -> Case:
    """the batch of recordgen.ring_wrap_skewed -- items of 1, 200 000, 37 and 200 000 bytes, so the long blocks start at 1 and 38 mod
    64 -- with the needles where THEIR ring wraps"""
    blobs, datas, at = [], [], 0
    for k, n in enumerate(rg.SKEW_ITEMS):
        d = _ring_block(n, at % 64, SEED + 40 + k) if n > RING else rg.filler(n, SEED + 40 + k)
        blobs.append(bytes(_oracle().compress(d, 1, threads=1)))
        datas.append(d.tobytes())
        at += n
    return Case("ring_wrap_skewed", rg.batch_of("find_ring_wrap_skewed", blobs, datas), equal_needle(RING_M))


# ---- 5: block seams -----------------------------------------------------------------------------------------------------------------------

SEAM_PERIOD = b"abcdefg"
SEAM_LENGTHS = [1] * 20 + [5, 0, 3] + [1 + (k * 23) % 40 for k in range(40)] + [0, 1, 0, 1, 1, 0, 2, 40, 1]
SEAM_NEEDLES = (2, 3, 16)


@functools.lru_cache(maxsize=None)
def seam_source() -> cg.Source:
    """ONE container assembled by hand from the oracle's block streams, as cutgen.tiny is, the ext bit mixed per frame: a run of 20
    blocks of 1 byte, blocks of 1 to 40 bytes, and EMPTY blocks among them (the format's frame word states a block's length, and
    the walk accepts 0).  The data is 'abcdefg' over and over, so a needle cut from it occurs every 7 bytes whatever the blocks are"""
    total = sum(SEAM_LENGTHS)
    data = (SEAM_PERIOD * (total // len(SEAM_PERIOD) + 1))[:total]
    blob, at = bytearray(), 0
    for k, n in enumerate(SEAM_LENGTHS):
        ext = (k ^ (k >> 2)) & 1
        st = _oracle().encode_block(np.frombuffer(data[at:at + n], dtype=np.uint8), ext)
        blob += (len(st) | (ext << 23)).to_bytes(cg.WORD, "little") + bytes(st)
        at += n
    head = b"TSQ1" + len(SEAM_LENGTHS).to_bytes(4, "little") + total.to_bytes(8, "little")
    return cg.Source("find_seams", head + bytes(blob), data)


def seams(m: int) -> Case:
    return Case(f"seams_m{m}", gg.from_source(seam_source(), "plain"), (SEAM_PERIOD * 3)[2:2 + m])


@functools.lru_cache(maxsize=None)
def two_blocks(m: int) -> Case:
    """cutgen's 4 MiB + 1 random bytes: the needle is the data's last m bytes, so a hit ENDS in the second block, which is one byte long"""
    s = cg.two_blocks()
    return Case(f"two_blocks_m{m}", gg.from_source(s, "plain"), s.data[BLOCK + 1 - m:])


PHRASE_BLOCKS, PHRASE_LEN = 257, 4096


@functools.lru_cache(maxsize=None)
def phrase_source() -> cg.Source:
    """splitgen's phrase of 64 bytes over 257 blocks of 4 096 bytes (less 7), with its table of stream sizes"""
    data, block_len = sg.edge_input(PHRASE_LEN, PHRASE_BLOCKS)
    blob, table = sg.expected_split(_oracle(), data, block_len, 1)
    return cg.Source("find_phrase", blob, data.tobytes(), block_len, table)


def phrase(kind: str, m: int) -> Case:
    """the needle: the phrase's last m // 2 bytes and its first m - m // 2, which lie across EVERY block edge (64 divides 4 096)"""
    s = phrase_source()
    return Case(f"phrase_{kind}_m{m}", gg.from_source(s, kind), s.data[64 - m // 2:64 - m // 2 + m])


# ---- 6: item seams ------------------------------------------------------------------------------------------------------------------------

RAGGED_BYTE = 0x61


@functools.lru_cache(maxsize=None)
def ragged_index(n: int) -> gg.Index:
    """joingen's ragged arena of n items, their lengths of 1 to 40 bytes kept and EVERY byte 'a': a needle of 'a's would occur at every
    place of the concatenation; the only hits are those inside an item"""
    c = jg.counts()[COUNTS.index(n)]
    datas = [bytes([RAGGED_BYTE]) * len(it.data) for it in c.items]
    blobs = [bytes(_oracle().compress(np.frombuffer(d, dtype=np.uint8), k & 1, threads=1)) for k, d in enumerate(datas)]
    return rg.batch_of(f"find_ragged_{n}", blobs, datas)


def ragged(n: int, m: int) -> Case:
    return Case(f"ragged_{n}_m{m}", ragged_index(n), bytes([RAGGED_BYTE]) * m)


DAMAGED_AT = rg.DAMAGED_AT


def damaged(needle: bytes = b"ef ") -> Case:
    """recordgen's reordering of gathergen's batch of 300 with six damaged headers: the refused items have no hits"""
    return Case(f"damaged_{needle.hex()}", rg.damaged().index, needle)


# ---- 7: the scans -------------------------------------------------------------------------------------------------------------------------

def carries(front: bool) -> Case:
    """recordgen's 300 items of 2^16 zeros (front: one of 66 x 2^16 zeros in front) with a needle of ONE zero: every byte is a hit, so
    d_item_first_hit passes 2^24 where d_item_first_record does"""
    return Case(rg.carries(front).name, rg.carries(front).index, b"\0")


# ---- 9: refusals --------------------------------------------------------------------------------------------------------------------------

def refused_case() -> Case:
    return Case("refused_index", gg.refused(), b"ef ")


@functools.lru_cache(maxsize=None)
def no_blocks() -> Case:
    """a batch index of two containers whose magic is wrong: both items are refused at the header, so the index has 0 blocks and 0
    bytes -- the call clears the status, the need word and the first-hit table and launches no decoder"""
    blob = dg._with_header(bytes(_oracle().compress(rg.filler(100, SEED + 9), 1, threads=1)), magic=b"TSQ2")
    return Case("no_blocks", rg.batch_of("find_no_blocks", [blob, blob], [None, None]), b"ef ")


def caps(case: Case):
    """8: -> [(what, cap_hits)]: exact, one short, ending inside a middle item, 0"""
    e = case.expect()
    n, first = e["need"][0], e["item_first"]
    n_items = len(first) - 1
    mid = next((i for i in list(range(n_items // 2, n_items)) + list(range(n_items // 2)) if first[i + 1] - first[i] >= 2), None)
    inside = first[mid] + 1 if mid is not None else n // 2
    return [("exactly the hits", n), ("one short", max(n - 1, 0)), ("ending inside a middle item", inside), ("none", 0)]


def healthy_cases():
    """every case whose index can be made from host bytes and is not refused (the carries apart: their tables are large)"""
    return ([places(m, e) for m in NEEDLE_LENGTHS for e in (False, True)] + [cell_edges(m, s) for m in CELL_NEEDLES for s in CELL_STARTS] +
            [chunk_edges(k) for k in CHUNK_CASES] + [ring_wrap(), ring_wrap_skewed()] + [seams(m) for m in SEAM_NEEDLES] +
            [two_blocks(2), two_blocks(16)] + [phrase(k, m) for k in ("sized", "plain") for m in (2, 16)] +
            [ragged(n, m) for n in COUNTS for m in (2, 16)] + [damaged(b"ef "), damaged(b"e")])
