"""Seeded cases for the cut of block ranges out of an indexed container (tsqa_plan_cut, tsqa_cut_async, tsqa_cut), shared by
test_cut_cpu.py -- which shows with the oracle, the host frame walk and the host-only planner that each case reaches what it aims
at -- and by test_gpu_cut.py, which runs the same cases through the kernels.  Nothing here calls a kernel.  The sources are the
oracle's containers; the expected containers, tables and statuses are made here in pure Python from the source's bytes, by the rule
of include/turbosqueeze_amd.h:
    container k = "TSQ1" | u32 count | u64 total | the source's bytes [frame(first), end(first + count - 1))

What is restated from the library, and must be re-derived when it changes there:
  walk         walk_frames (tsq_format.h), as tsqa_index_create keeps it: every frame's place and every block's output place
  measure      cut_measure_kernel (tsq_cut.cuh) for the one item of a container: the gate, the range rule written without
               first + count, the size and the total
  layout       cut_sum_kernel, cut_scan_kernel, cut_place_kernel: tsqa_plan_packed's rule on the sizes, the fit of every range
               against out_size by itself, the largest status
  plan_cut     tsqa_plan_cut (tsq_runtime.hip): rules 2 to 5 from host tables, and n_fit
  expect       the order of the launches of tsqa_cut_async: what a refused index, a refused range and an unfit range leave
  GROUP, WAVE, SPLIT   cut_sum_kernel and cut_place_kernel take 256 ranges per workgroup (four wavefronts of 64): a group's places
               are summed inside it, cut_scan_kernel -- ONE workgroup, 256 groups per pass -- turns the groups' sums into their
               bases, and the place is base + own; group_scan_excl64 (tsq_container.cuh) sums v & 0xFFFFFF and v >> 24 apart
  WORD16       cut_emit_kernel moves 16-byte words cut at multiples of 16 of the destination address
"""
from __future__ import annotations

import functools

import numpy as np

import densegen as dg
import seekgen as kg
import splitgen as sg

BLOCK, SLOT = sg.BLOCK, sg.OUTPUT_SZ
HEADER, WORD, MIN_FRAME = sg.HEADER, sg.WORD, sg.MIN_FRAME
GROUP, WAVE, SPLIT = dg.GROUP, dg.WAVE, dg.SPLIT
WORD16 = 16
OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = 0, 3, 4, 6
SEED = 7310
COUNTS = (1, 2, 255, 256, 257, 513)
ALIGNS = (1, 16, 4096)
TINY_BLOCKS = 600
SPLIT_BLOCKS, SPLIT_LEN = 257, 4096
ALL_ONES = (1 << 64) - 1


def round_up(v: int, align: int) -> int:
    return (v + align - 1) // align * align


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def walk(blob: bytes):
    """RE-DERIVE with walk_frames -> (frame_at n_blocks + 1: every frame word's place, then the end of the last frame; out_start
    n_blocks + 1) of a well-formed container"""
    nb, total = int.from_bytes(blob[4:8], "little"), int.from_bytes(blob[8:16], "little")
    assert blob[:4] == b"TSQ1" and nb >= 1
    at, oat, frame_at, out_start = HEADER, 0, [], []
    for _ in range(nb):
        ln = int.from_bytes(blob[at:at + 3], "little") & 0x7FFFFF
        out_len = int.from_bytes(blob[at + 3:at + 6], "little")
        assert 3 <= ln <= SLOT and at + WORD + ln <= len(blob) and out_len <= BLOCK
        frame_at.append(at)
        out_start.append(oat)
        at, oat = at + WORD + ln, oat + out_len
    assert oat == total
    return frame_at + [at], out_start + [oat]


def measure(frame_at, out_start, first: int, count: int):
    """RE-DERIVE with cut_measure_kernel -> (size, total, src_at) of an accepted range, None of a refused one.  first and count are
    any 64-bit values; first + count is never formed."""
    nb = len(frame_at) - 1
    if count < 1 or first >= nb or count > nb - first:
        return None
    return HEADER + frame_at[first + count] - frame_at[first], out_start[first + count] - out_start[first], frame_at[first]


def layout(sizes, align: int):
    """RE-DERIVE with cut_sum_kernel, cut_scan_kernel, cut_place_kernel and tsqa_plan_packed -> offsets (n + 1): every place a multiple of align, the last entry
    not rounded"""
    at, out = 0, []
    for k, s in enumerate(sizes):
        out.append(at)
        at += s
        if k + 1 < len(sizes):
            at = round_up(at, align)
    return out + [at]


def plan_cut(frame_at, out_start, ranges, align: int, out_size: int):
    """RE-DERIVE with tsqa_plan_cut -> (offsets, sizes, totals, item_status, n_fit)"""
    got = [measure(frame_at, out_start, f, n) for f, n in ranges]
    sizes = [m[0] if m else 0 for m in got]
    totals = [m[1] if m else 0 for m in got]
    offsets = layout(sizes, align)
    status = [ERR_ARG if m is None else OK if o + s <= out_size else ERR_OVERFLOW for m, o, s in zip(got, offsets, sizes)]
    n_fit = next((k for k, st in enumerate(status) if st == ERR_OVERFLOW), len(ranges))
    return offsets, sizes, totals, status, n_fit


# ---- sources --------------------------------------------------------------------------------------------------------------------------

class Source:
    """a well-formed container, its data, and its walk"""

    def __init__(self, name: str, blob: bytes, data: bytes, block_len=None, table=None):
        self.name, self.blob, self.data, self.block_len, self.table = name, bytes(blob), bytes(data), block_len, table
        self.frame_at, self.out_start = walk(self.blob)
        self.n_blocks = len(self.frame_at) - 1
        assert self.out_start[-1] == len(self.data)

    @property
    def frame_bytes(self) -> int:
        return self.frame_at[-1]


def _oracle():
    return dg._oracle()


@functools.lru_cache(maxsize=None)
def tiny() -> Source:
    """600 blocks of 1 to 40 bytes of text, the ext bit mixed per frame, assembled by hand from the oracle's block streams (the
    format allows any block length): frames of 9 bytes and up"""
    text = dg._text(TINY_BLOCKS * 40, SEED)
    blob, at = bytearray(), 0
    for k in range(TINY_BLOCKS):
        n, ext = 1 + (k * 23 + k // 40) % 40, (k ^ (k >> 3)) & 1
        st = _oracle().encode_block(text[at:at + n], ext)
        blob += (len(st) | (ext << 23)).to_bytes(WORD, "little") + st
        at += n
    head = b"TSQ1" + TINY_BLOCKS.to_bytes(4, "little") + at.to_bytes(8, "little")
    return Source("tiny", head + bytes(blob), text[:at].tobytes())


@functools.lru_cache(maxsize=None)
def two_blocks() -> Source:
    """a plain container of 4 MiB + 1 random bytes: two blocks"""
    data = np.random.default_rng(SEED).integers(0, 256, BLOCK + 1, dtype=np.uint8)
    return Source("two_blocks", _oracle().compress(data, 1, threads=2), data.tobytes())


@functools.lru_cache(maxsize=None)
def split() -> Source:
    """a container of 257 blocks of 4 096 bytes (splitgen.expected_split) with its table of stream sizes, for a sized index"""
    data = sg.count_input(512)[:SPLIT_BLOCKS * SPLIT_LEN]
    blob, table = sg.expected_split(_oracle(), data, SPLIT_LEN, 1)
    return Source("split", blob, data.tobytes(), SPLIT_LEN, table)


@functools.lru_cache(maxsize=None)
def random8() -> Source:
    """eight blocks of 2^16 random bytes: every frame is longer than its block"""
    data = np.random.default_rng(SEED + 1).integers(0, 256, 8 << 16, dtype=np.uint8)
    blob, table = sg.expected_split(_oracle(), data, 1 << 16, 1)
    return Source("random8", blob, data.tobytes(), 1 << 16, table)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

class Case:
    """ranges (first, count) of a source, packed at `align`"""

    def __init__(self, name: str, source: Source, ranges, align: int = 16):
        self.name, self.source, self.ranges, self.align = name, source, [(int(f), int(n)) for f, n in ranges], align

    @functools.lru_cache(maxsize=None)
    def expect(self, out_size: int, refused_index: bool = False):
        """RE-DERIVE with tsqa_cut_async -> dict: offsets, sizes, totals, item_status, status, need (offsets[n]) and containers: per
        range the bytes the call owes at its place, None where it owes none.  refused_index: the verdict of a sized index is
        nonzero."""
        s, n = self.source, len(self.ranges)
        if refused_index:
            return dict(offsets=[0] * (n + 1), sizes=[0] * n, totals=[0] * n, item_status=[ERR_FORMAT] * n, status=ERR_FORMAT, need=0,
                        containers=[None] * n, n_fit=n)
        offsets, sizes, totals, status, n_fit = plan_cut(s.frame_at, s.out_start, self.ranges, self.align, out_size)
        containers = []
        for (f, c), st, t in zip(self.ranges, status, totals):
            if st != OK:
                containers.append(None)
                continue
            containers.append(b"TSQ1" + c.to_bytes(4, "little") + t.to_bytes(8, "little") + s.blob[s.frame_at[f]:s.frame_at[f + c]])
        return dict(offsets=offsets, sizes=sizes, totals=totals, item_status=status, status=max(status), need=offsets[n],
                    containers=containers, n_fit=n_fit)

    @property
    def need(self) -> int:
        return self.expect(1 << 62)["need"]

    def data(self, k: int) -> bytes:
        f, c = self.ranges[k]
        return self.source.data[self.source.out_start[f]:self.source.out_start[f + c]]

    def arena(self, e, fill):
        """the output the call owes: `fill` (a uint8 array of the room's length) with every owed container at its place"""
        out = fill.copy()
        for o, blob in zip(e["offsets"], e["containers"]):
            if blob is not None:
                out[o:o + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        return out


def tiny_ranges(n: int):
    """range k of the list over tiny(): every start, counts 1 to 5 with single blocks most often, overlapping and repeating"""
    return [((k * 37 + k // 16) % TINY_BLOCKS, 1 if k % 3 else 1 + k % 5) for k in range(n)]


def _clip(ranges, nb):
    return [(f, min(c, nb - f)) for f, c in ranges]


@functools.lru_cache(maxsize=None)
def counts():
    """1, 2, 255, 256, 257 and 513 ranges over tiny() at align 1 (prefixes of one list): containers of 25 bytes and up at every residue"""
    return tuple(Case(f"tiny_{n}", tiny(), _clip(tiny_ranges(n), TINY_BLOCKS), 1) for n in COUNTS)


@functools.lru_cache(maxsize=None)
def aligned(align: int):
    return Case(f"tiny_257_align_{align}", tiny(), _clip(tiny_ranges(257), TINY_BLOCKS), align)


@functools.lru_cache(maxsize=None)
def whole(name: str):
    s = {"tiny": tiny, "two_blocks": two_blocks, "split": split, "random8": random8}[name]()
    return Case(f"whole_{name}", s, [(0, s.n_blocks)], 16)


WHOLE = ("tiny", "two_blocks", "split", "random8")


@functools.lru_cache(maxsize=None)
def two_block_parts():
    """each block of the two-block container, the second one first"""
    return Case("two_blocks_each", two_blocks(), [(1, 1), (0, 1)], 16)


@functools.lru_cache(maxsize=None)
def split_ranges():
    """the sized index's ranges: the first block, the last two, the last, and all"""
    return Case("split_ranges", split(), [(0, 1), (255, 2), (256, 1), (0, 257)], 16)


@functools.lru_cache(maxsize=None)
def carry_inside():
    """300 single blocks of random8(), repeated: every container is longer than 2^16, so the places pass 2^24 inside range 246"""
    return Case("carry_inside_a_wavefront", random8(), [(k % 8, 1) for k in range(300)], 16)


CARRY_EDGE_CROSSING = 3 * WAVE


@functools.lru_cache(maxsize=None)
def carry_edge():
    """the same with one long range (all eight blocks) in front and as many two-block ranges behind it as it takes for the first
    place at or above 2^24 to be range 192's: lane 0 of the fourth wavefront, whose place is made of the other wavefronts' totals"""
    s = random8()
    ranges = [(0, 8)] + [(k % 8, 1) for k in range(1, 300)]
    for k in range(1, CARRY_EDGE_CROSSING - 1):
        if layout([measure(s.frame_at, s.out_start, f, c)[0] for f, c in ranges], 16)[CARRY_EDGE_CROSSING] >= SPLIT:
            break
        ranges[k] = (k % 7, 2)
    return Case("carry_at_a_wavefront_edge", s, ranges, 16)


def crossing(case: Case) -> int:
    """the first range whose place is at or above 2^24"""
    return next(k for k, o in enumerate(case.expect(1 << 62)["offsets"]) if o >= SPLIT)


def healthy_cases():
    return (list(counts()) + [aligned(a) for a in ALIGNS] + [whole(n) for n in WHOLE] +
            [two_block_parts(), split_ranges(), carry_inside(), carry_edge()])


def seams(case: Case):
    """-> (destination residues of the containers' starts, destination residues of their ends, (source - destination) % 16 of the
    bodies, the number of 16-byte words of the output that hold bytes of two containers, the most containers one word holds) of a
    healthy case whose output starts at a multiple of 16"""
    e = case.expect(1 << 62)
    s = case.source
    starts = np.array(e["offsets"][:-1], dtype=np.int64)
    ends = starts + np.array(e["sizes"], dtype=np.int64)
    shift = {(s.frame_at[f] - (o + HEADER)) % WORD16 for (f, _), o in zip(case.ranges, e["offsets"])}
    words = np.arange(0, (e["need"] + WORD16 - 1) // WORD16, dtype=np.int64) * WORD16
    # the containers a word holds bytes of: those that start before its end and end after its start
    first = np.searchsorted(ends, words, side="right")
    last = np.searchsorted(starts, words + WORD16, side="left") - 1
    held = np.maximum(last - first + 1, 0)
    return {int(o) % WORD16 for o in starts}, {int(o) % WORD16 for o in ends}, shift, int((held == 2).sum()), int(held.max())


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

REFUSAL_AT = (0, 256, 299)          # of 300 ranges: the first, the first lane of the second group, the last
REFUSALS = {"count_0": (5, 0), "first_is_n_blocks": (TINY_BLOCKS, 1), "one_block_too_many": (TINY_BLOCKS - 2, 3),
            "first_2_to_the_32": (1 << 32, 1), "count_2_to_the_63": (1, 1 << 63), "all_ones": (ALL_ONES, ALL_ONES)}


@functools.lru_cache(maxsize=None)
def refusal(name: str, at: int):
    """300 ranges over tiny() with the refused range `name` as range `at`"""
    ranges = _clip(tiny_ranges(300), TINY_BLOCKS)
    ranges[at] = REFUSALS[name]
    return Case(f"refusal_{name}_at_{at}", tiny(), ranges, 16)


def refusal_cases():
    return [(name, at) for name in REFUSALS for at in REFUSAL_AT]


# ---- room -----------------------------------------------------------------------------------------------------------------------------

ROOM_MIDDLE = 130


def rooms():
    """-> [(what, case, out_size, n_fit)]; out_size None: measure only"""
    c = aligned(16)
    e = c.expect(1 << 62)
    o, n = e["offsets"], len(c.ranges)
    return [("exactly the room needed", c, e["need"], n),
            ("one byte short of the last container", c, e["need"] - 1, n - 1),
            ("room that ends inside a header", c, o[ROOM_MIDDLE] + 7, ROOM_MIDDLE),
            ("room that ends inside a middle container", c, o[ROOM_MIDDLE] + HEADER + 3, ROOM_MIDDLE),
            ("measure only", c, None, 0)]


# ---- a refused index ------------------------------------------------------------------------------------------------------------------

REFUSED_TABLE = "entry_256_plus_1"


@functools.lru_cache(maxsize=None)
def refused_index():
    """a valid container of 300 blocks of 4 096 bytes with one of seekgen's false tables, which a sized index refuses on the device
    -> (container, table, n_total, block_len, a Case over it)"""
    data = sg.count_input(512)[:300 * SPLIT_LEN]
    blob, sizes = sg.expected_split(_oracle(), data, SPLIT_LEN, 1)
    name, c, n, table, _ = next(t for t in kg.false_tables(blob, sizes) if t[0] == REFUSED_TABLE)
    assert c == blob and n == len(blob) and table != sizes
    case = Case("refused_index", Source("split_300", blob, data.tobytes(), SPLIT_LEN, sizes), [(0, 1), (255, 2), (299, 1), (0, 300), (300, 1)], 16)
    return blob, table, data.size, SPLIT_LEN, case
