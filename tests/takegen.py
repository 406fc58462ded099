"""Seeded cases for the take: items and block ranges inside items cut out of a batch index (tsqa_plan_cut_items,
tsqa_cut_items_async, tsqa_cut_items), shared by test_take_cpu.py -- which shows with the oracle, the host frame walk and the
host-only planner that each case reaches what it aims at -- and by test_gpu_take.py, which runs the same cases through the kernels.
Nothing here calls a kernel, and almost no input is made here: the arenas are joingen's, packedindexgen's (densegen's, mtgen's and
batchsplitgen's containers) and cutgen's sources.  The expected containers, tables and statuses are made here in pure Python from the
arena's bytes, by the rule of include/turbosqueeze_amd.h:
    container k = "TSQ1" | u32 count | u64 total | the arena's bytes [frame(item's first + first), end(item's first + first + count - 1))

What is restated from the library, and must be re-derived when it changes there:
  Index        what tsqa_index_create_batch and tsqa_index_create_packed* leave (tsq_index_packed.cuh), through packedindexgen's
               measure, fit, walk and close_up: which items are healthy, their first blocks, every live block's frame and output place
  measure      cut_measure_kernel (tsq_cut.cuh): the gate, the item rule (an item that does not exist, was refused or is unfit owns
               no blocks), the range rule (cutgen.measure) inside the item without first + count, the size and the total
  layout       cut_sum_kernel, cut_scan_kernel, cut_place_kernel: tsqa_plan_packed's rule on the sizes (cutgen.layout), the fit
               of every range against out_size by itself, the largest status
  plan         tsqa_plan_cut_items (tsq_runtime.hip): the same from host tables, and n_fit
  expect       the order of the launches of tsqa_cut_items_async: what a refused index, a refused range and an unfit range leave
  GROUP, PASS, WAVE, SPLIT   launches (a) and (c) take 256 ranges per workgroup (four wavefronts of 64), launch (b) is ONE workgroup
               that takes 256 groups -- 65 536 ranges -- per pass; group_scan_excl64 (tsq_container.cuh) sums v & 0xFFFFFF and
               v >> 24 apart
  WORD16       cut_emit_kernel (tsq_cut.cuh) moves 16-byte words cut at multiples of 16 of the destination address
"""
from __future__ import annotations

import functools

import numpy as np

import batchsplitgen as bsg
import cutgen as cg
import joingen as jg
import packedindexgen as pg

HEADER, WORD = cg.HEADER, cg.WORD
GROUP, WAVE, SPLIT = cg.GROUP, cg.WAVE, cg.SPLIT
PASS = GROUP * 256
WORD16 = 16
OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = 0, 3, 4, 6
SEED = 7420
COUNTS = (1, 2, 255, 256, 257, 513)
ALIGNS = (1, 16, 4096)
PASS_COUNTS = (PASS - 1, PASS, PASS + 1)
ALL_ONES = (1 << 64) - 1


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

class Index:
    """RE-DERIVE with tsqa_index_create_batch / tsqa_index_create_packed*: the index of the containers arena[offsets[i]:][:sizes[i]].
    cap_blocks None: every accepted item fits (tsqa_index_create_batch has no cap).  -> item_status, item_first (n + 1: a refused or
    unfit item owns no blocks) and, per live block, src (where its frame word lies in the arena), end (where its stream ends) and
    out_start (n_blocks + 1, in the concatenation of the healthy items' data)."""

    def __init__(self, arena, offsets, sizes, cap_blocks=None):
        heads = [pg.measure(arena, len(arena), o, n) for o, n in zip(offsets, sizes)]
        blocks, totals = [b for b, _ in heads], [t for _, t in heads]
        _, n_fit = pg.fit(blocks, sum(blocks) if cap_blocks is None else cap_blocks)
        self.item_status, self.src, self.end, self.out_start = [], [], [], [0]
        for i, (o, n, b, t) in enumerate(zip(offsets, sizes, blocks, totals)):
            st = ERR_FORMAT
            if b:
                blob = bytes(arena[o:o + n])
                st = ERR_OVERFLOW if i >= n_fit else OK if pg.walk(blob, b, t) is not None else ERR_FORMAT
            self.item_status.append(st)
            if st == OK:
                frame_at, out_start = cg.walk(blob)
                self.src += [o + a for a in frame_at[:-1]]
                self.end += [o + a for a in frame_at[1:]]
                base = self.out_start[-1]
                self.out_start += [base + z for z in out_start[1:]]
        self.item_first, _, self.n_blocks, self.total = pg.close_up(blocks, totals, self.item_status)
        self.n_items, self.need_blocks = len(offsets), sum(blocks)

    def plan_tables(self):
        """-> (frame_at, out_start) as tsqa_plan_cut_items takes them: boundaries from 16 on whose differences are the frames' bytes"""
        frame_at = [HEADER]
        for a, z in zip(self.src, self.end):
            frame_at.append(frame_at[-1] + z - a)
        return frame_at, self.out_start


def measure(ix: Index, item: int, first, count):
    """RE-DERIVE with cut_measure_kernel -> (size, total, src_at, end_at, count) of an accepted range, None of a refused one.  item,
    first and count are any unsigned values; first and count None: the whole item; first + count is never formed."""
    if item >= ix.n_items:
        return None
    fb, fe = ix.item_first[item], ix.item_first[item + 1]
    if fb >= fe:
        return None
    nb = fe - fb
    first, count = (0, nb) if first is None else (first, count)
    if count < 1 or first >= nb or count > nb - first:
        return None
    a, z = fb + first, fb + first + count
    return HEADER + ix.end[z - 1] - ix.src[a], ix.out_start[z] - ix.out_start[a], ix.src[a], ix.end[z - 1], count


def plan(ix: Index, items, ranges, align: int, out_size: int):
    """RE-DERIVE with tsqa_plan_cut_items and the three layout launches -> (offsets, sizes, totals, item_status, n_fit, measured)"""
    n = len(items)
    got = [measure(ix, items[k], *(ranges[k] if ranges is not None else (None, None))) for k in range(n)]
    sizes, totals = [m[0] if m else 0 for m in got], [m[1] if m else 0 for m in got]
    offsets = cg.layout(sizes, align)
    status = [ERR_ARG if m is None else OK if o + s <= out_size else ERR_OVERFLOW for m, o, s in zip(got, offsets, sizes)]
    n_fit = next((k for k, st in enumerate(status) if st == ERR_OVERFLOW), n)
    return offsets, sizes, totals, status, n_fit, got


# ---- batches --------------------------------------------------------------------------------------------------------------------------

class Batch:
    """containers in an arena with the tables a caller hands over, and each item's data (None where no decode owes any)"""

    def __init__(self, name, arena, offsets, sizes, datas, block_len=None, table_first=None, table=None):
        self.name, self.arena, self.offsets, self.sizes, self.datas = name, np.asarray(arena, dtype=np.uint8), list(offsets), list(sizes), list(datas)
        self.block_len, self.table_first, self.table = block_len, table_first, table
        self.n = len(self.offsets)

    @functools.lru_cache(maxsize=None)
    def index(self, cap_blocks=None) -> Index:
        return Index(self.arena, self.offsets, self.sizes, cap_blocks)


def _of_join(c: jg.Case) -> Batch:
    return Batch(c.name, c.arena, c.offsets, c.sizes, [it.data for it in c.items])


def _of_packed(c: pg.Case) -> Batch:
    return Batch(c.name, c.arena, c.offsets, c.sizes, c.datas, c.block_len, c.table_first, c.table)


def _of_source(s: cg.Source) -> Batch:
    """one container as a batch of one item at the buffer's start: what tsqa_index_create and tsqa_index_create_sized* index"""
    return Batch(s.name, np.frombuffer(s.blob, dtype=np.uint8), [0], [len(s.blob)], [s.data], s.block_len, [0, s.n_blocks], s.table)


@functools.lru_cache(maxsize=None)
def ragged(n: int) -> Batch:
    """joingen's ragged arena of n items of 1 to 40 bytes: containers of 25 bytes and up, 7 k % 16 unused bytes in front of item k"""
    return _of_join(jg.counts()[jg.COUNTS.index(n)])


@functools.lru_cache(maxsize=None)
def random8() -> Batch:
    """eight items of 2^16 random bytes (joingen's): every container is longer than 2^16"""
    return _of_join(jg.Case("random8", [jg.random_item(1 << 16, 8000 + k, k & 1) for k in range(8)], 16))


LONG_CROSSING = 3 * WAVE


@functools.lru_cache(maxsize=None)
def random8_long() -> Batch:
    """the same with a ninth item of random bytes, long enough that with it as range 0 and the eight in turn behind it the first place
    at or above 2^24 is range 192's: lane 0 of the fourth wavefront, whose place is made of the other wavefronts' totals"""
    small = [jg.random_item(1 << 16, 8000 + k, k & 1) for k in range(8)]
    step = cg.round_up(len(small[0].blob), 16)
    assert all(cg.round_up(len(it.blob), 16) == step for it in small)
    want = SPLIT - (LONG_CROSSING - 1) * step + step // 2     # the long container, padded: half a container below the crossing
    n = want * (1 << 16) // len(small[0].blob)                # (random bytes grow by the same share at every length)
    return _of_join(jg.Case("random8_long", small + [jg.random_item(n, 8999, 1)], 16))


@functools.lru_cache(maxsize=None)
def pages() -> Batch:
    """batchsplitgen's item of 2B + 1 blocks of 4 096 bytes between one-block items, with its true tables"""
    return _of_packed(pg._of_split("pages", bsg.ownership(bsg.DEFAULT_BUDGET)[5], sized=True))


PAGES_ITEM = 2


@functools.lru_cache(maxsize=None)
def three_blocks() -> Batch:
    """batchsplitgen.cap_batch: ten items, the sixth of three blocks of 4 KiB, with its true tables"""
    return _of_packed(pg._of_split("three_blocks", bsg.cap_batch(), sized=True))


THREE_ITEM = bsg.CAP_MID


DAMAGED = {"headers": ("count_0", "count_above", "total_above"), "walks": ("mt_cut_in_size_word", "mt_cut_mid_stream", "mt_cut_at_frame_end")}


@functools.lru_cache(maxsize=None)
def damaged(which: str) -> Batch:
    """packedindexgen's batch of 300 items whose items 0, 256 and 299 are refused -- 'headers': three of densegen's damaged headers;
    'walks': three of mtgen's cut containers, whose headers pass and which only the walk refuses"""
    case = next(c for c in pg.refusals() if c.kinds == DAMAGED[which])
    b = _of_packed(case)
    b.kinds = case.kinds
    return b


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

class Case:
    """ranges of a batch's index, packed at `align`.  items: the item of each range (any 32-bit values); ranges: (first, count) per
    range, or None for whole items; cap_blocks: of a device-made index (None: the blocks needed)."""

    def __init__(self, name, batch: Batch, items, ranges=None, align: int = 16, cap_blocks=None):
        self.name, self.batch, self.items, self.align, self.cap_blocks = name, batch, [int(i) for i in items], align, cap_blocks
        self.ranges = None if ranges is None else [(int(f), int(c)) for f, c in ranges]
        self.n = len(self.items)

    @property
    def index(self) -> Index:
        return self.batch.index(self.cap_blocks)

    @functools.lru_cache(maxsize=None)
    def expect(self, out_size: int, refused_index: bool = False):
        """RE-DERIVE with tsqa_cut_items_async -> dict: offsets, sizes, totals, item_status, status, need (offsets[n]), n_fit and
        spans: per range (src_at, end_at, count, total) of the container the call owes at its place, None where it owes none.
        refused_index: the verdict of a sized index is nonzero."""
        n = self.n
        if refused_index:
            return dict(offsets=[0] * (n + 1), sizes=[0] * n, totals=[0] * n, item_status=[ERR_FORMAT] * n, status=ERR_FORMAT, need=0,
                        spans=[None] * n, n_fit=n)
        offsets, sizes, totals, status, n_fit, got = plan(self.index, self.items, self.ranges, self.align, out_size)
        spans = [(m[2], m[3], m[4], m[1]) if st == OK else None for m, st in zip(got, status)]
        return dict(offsets=offsets, sizes=sizes, totals=totals, item_status=status, status=max(status), need=offsets[n], spans=spans, n_fit=n_fit)

    @property
    def need(self) -> int:
        return self.expect(1 << 62)["need"]

    def container(self, e, k: int):
        """the container the call owes for range k, None where it owes none"""
        if e["spans"][k] is None:
            return None
        a, z, count, total = e["spans"][k]
        return b"TSQ1" + count.to_bytes(4, "little") + total.to_bytes(8, "little") + self.batch.arena[a:z].tobytes()

    def data(self, k: int):
        """what range k decodes to (of an accepted range of an item whose data is known)"""
        ix, it = self.index, self.items[k]
        fb, nb = ix.item_first[it], ix.item_first[it + 1] - ix.item_first[it]
        f, c = (0, nb) if self.ranges is None else self.ranges[k]
        base = ix.out_start[fb]
        return self.batch.datas[it][ix.out_start[fb + f] - base:ix.out_start[fb + f + c] - base]

    def arena(self, e, fill):
        """the output the call owes: `fill` (a uint8 array of the room's length) with every owed container at its place"""
        out = fill.copy()
        src = self.batch.arena
        for o, span in zip(e["offsets"], e["spans"]):
            if span is None:
                continue
            a, z, count, total = span
            out[o:o + HEADER] = np.frombuffer(b"TSQ1" + count.to_bytes(4, "little") + total.to_bytes(8, "little"), dtype=np.uint8)
            out[o + HEADER:o + HEADER + z - a] = src[a:z]
        return out


@functools.lru_cache(maxsize=None)
def counts():
    """1, 2, 255, 256, 257 and 513 whole items of the ragged arenas, in order, at align 1: a seam at every destination residue"""
    return tuple(Case(f"ragged_{n}", ragged(n), range(n), None, 1) for n in COUNTS)


@functools.lru_cache(maxsize=None)
def aligned(align: int):
    return Case(f"ragged_257_align_{align}", ragged(257), range(257), None, align)


@functools.lru_cache(maxsize=None)
def pass_edge(n: int):
    """n ranges over the 513 items, item 37 k + k // 16 mod 513 as range k: launch (b)'s second pass starts at range 65 536"""
    return Case(f"pass_edge_{n}", ragged(513), [(k * 37 + k // 16) % 513 for k in range(n)], None, 1)


@functools.lru_cache(maxsize=None)
def carry_inside():
    """600 whole-item ranges over the eight items of 2^16 random bytes: the sum passes 2^24 at lane 247 of every full group of
    launch (a), and every group word of launch (b) but the first lies above it"""
    return Case("carry_inside_a_group", random8(), [k % 8 for k in range(600)], None, 16)


@functools.lru_cache(maxsize=None)
def carry_edge():
    """the same with the long item as range 0: the first place at or above 2^24 is range 192's, lane 0 of a wavefront"""
    return Case("carry_at_a_wavefront_edge", random8_long(), [8] + [k % 8 for k in range(1, 600)], None, 16)


def crossing(case: Case) -> int:
    """the first range whose place is at or above 2^24"""
    return next(k for k, o in enumerate(case.expect(1 << 62)["offsets"]) if o >= SPLIT)


@functools.lru_cache(maxsize=None)
def identity():
    """every item of joingen's arena of 257 items at multiples of 16, in order, at that align"""
    return Case("identity", _of_join(jg.aligned(16)), range(257), None, 16)


@functools.lru_cache(maxsize=None)
def permutation():
    """300 draws from the 257 items of the ragged arena, seeded: a shuffle with repeats and gaps"""
    rng = np.random.default_rng(SEED)
    return Case("permutation", ragged(257), rng.integers(0, 257, 300).tolist(), None, 16)


@functools.lru_cache(maxsize=None)
def page_ranges():
    """the item of 2B + 1 blocks cut into pages: (item, j, 1) for every j"""
    b = pages()
    nb = b.table_first[PAGES_ITEM + 1] - b.table_first[PAGES_ITEM]
    assert nb == 2 * bsg.DEFAULT_BUDGET + 1
    return Case("pages", b, [PAGES_ITEM] * nb, [(j, 1) for j in range(nb)], 16)


@functools.lru_cache(maxsize=None)
def inner_ranges():
    """ranges inside the item of three blocks between one-block items: each block, both pairs, all three, and one-block items"""
    i = THREE_ITEM
    items = [i, i, i, i, i, i, i - 1, i + 1, 0, 9]
    return Case("inner_ranges", three_blocks(), items, [(0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (0, 3), (0, 1), (0, 1), (0, 1), (0, 1)], 16)


def healthy_cases():
    return (list(counts()) + [aligned(a) for a in ALIGNS] + [pass_edge(n) for n in PASS_COUNTS] +
            [carry_inside(), carry_edge(), identity(), permutation(), page_ranges(), inner_ranges()])


def seams(case: Case):
    """-> (destination residues of the containers' starts, of their ends, (source - destination) % 16 of the bodies) of a healthy
    case whose output starts at a multiple of 16"""
    e = case.expect(1 << 62)
    starts = {o % WORD16 for o in e["offsets"][:-1]}
    ends = {(o + s) % WORD16 for o, s in zip(e["offsets"], e["sizes"])}
    shift = {(span[0] - (o + HEADER)) % WORD16 for o, span in zip(e["offsets"], e["spans"])}
    return starts, ends, shift


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

REFUSAL_AT = (0, 256, 299)          # of 300 ranges: the first, the first lane of the second group, the last
BAD_ITEMS = {"item_is_n_items": 300, "item_all_ones": 0xFFFFFFFF}
# (first, count) inside the item of three blocks: nb = 3
BAD_RANGES = {"count_0": (1, 0), "first_is_nb": (3, 1), "one_past_nb": (1, 3), "first_all_ones_count_2": (ALL_ONES, 2),
              "count_2_to_the_63": (1, 1 << 63)}
EDGE_RANGE = (1, 2)                 # first + count == nb exactly: accepted


@functools.lru_cache(maxsize=None)
def bad_item(name: str, at: int):
    """the 300 items of _ragged_300, whole and in order, with the item number `name` as range `at`"""
    items = list(range(300))
    items[at] = BAD_ITEMS[name]
    return Case(f"refusal_{name}_at_{at}", _ragged_300(), items, None, 16)


@functools.lru_cache(maxsize=None)
def _ragged_300() -> Batch:
    """the first 300 items of the ragged arena of 513 as a batch of 300: item 300 is the first that does not exist"""
    b = ragged(513)
    return Batch("ragged_300", b.arena, b.offsets[:300], b.sizes[:300], b.datas[:300])


@functools.lru_cache(maxsize=None)
def bad_range(name: str, at: int):
    """300 ranges over the batch of ten items, the first block of item k % 10 as range k, with the range `name` of the item of three
    blocks as range `at`"""
    items, ranges = [k % 10 for k in range(300)], [(0, 1)] * 300
    items[at], ranges[at] = THREE_ITEM, BAD_RANGES[name]
    return Case(f"refusal_{name}_at_{at}", three_blocks(), items, ranges, 16)


@functools.lru_cache(maxsize=None)
def edge_range(at: int):
    """the same with first + count == nb as range `at`: accepted"""
    items, ranges = [k % 10 for k in range(300)], [(0, 1)] * 300
    items[at], ranges[at] = THREE_ITEM, EDGE_RANGE
    return Case(f"edge_range_at_{at}", three_blocks(), items, ranges, 16)


@functools.lru_cache(maxsize=None)
def refused_items(which: str):
    """every item of damaged(which) in order: ranges 0, 256 and 299 name refused items"""
    return Case("refused_items_" + which, damaged(which), range(300), None, 16)


UNFIT_FROM = 257


@functools.lru_cache(maxsize=None)
def unfit_items():
    """the 300 items of _ragged_300 through a device-made index whose cap_blocks holds the first 257 of them: range k is item k,
    which leaves ranges 257 to 299 unfit, and ranges 0 and 256 name the unfit items 299 and 258"""
    items = list(range(300))
    items[0], items[256] = 299, 258
    return Case("unfit_items", _ragged_300(), items, None, 16, cap_blocks=UNFIT_FROM)


def refusal_cases():
    return ([bad_item(name, at) for name in BAD_ITEMS for at in REFUSAL_AT] + [bad_range(name, at) for name in BAD_RANGES for at in REFUSAL_AT] +
            [edge_range(at) for at in REFUSAL_AT] + [refused_items(w) for w in DAMAGED] + [unfit_items()])


# ---- room -----------------------------------------------------------------------------------------------------------------------------

ROOM_MIDDLE = 130


def rooms():
    """-> [(what, case, out_size, n_fit)]; out_size None: measure only"""
    c = aligned(16)
    e = c.expect(1 << 62)
    o, n = e["offsets"], c.n
    return [("exactly the room needed", c, e["need"], n),
            ("one byte short of the last container", c, e["need"] - 1, n - 1),
            ("room that ends inside a header", c, o[ROOM_MIDDLE] + 7, ROOM_MIDDLE),
            ("room that ends inside a middle container", c, o[ROOM_MIDDLE] + HEADER + 3, ROOM_MIDDLE),
            ("measure only", c, None, 0)]


# ---- index kinds ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def kinds_case():
    """the 257 ranges that every kind of batch index must cut alike"""
    return aligned(16)


@functools.lru_cache(maxsize=None)
def sized_batch_case():
    """257 ranges over batchsplitgen's ten items with their true tables: whole items and pages of the item of three blocks"""
    return Case("sized_batch", three_blocks(), [k % 10 for k in range(257)], [(0, 1) if k % 10 != THREE_ITEM else (k % 3, 3 - k % 3) for k in range(257)], 16)


@functools.lru_cache(maxsize=None)
def single(name: str):
    """cutgen's ranges over one of its sources as a take of item 0 -> (Case, the cutgen case): tsqa_cut_async owes the same"""
    c = {"tiny": cg.aligned(16), "split": cg.split_ranges()}[name]
    return Case("single_" + c.name, _of_source(c.source), [0] * len(c.ranges), c.ranges, c.align), c


@functools.lru_cache(maxsize=None)
def refused_index():
    """cutgen.refused_index as a take -> (container, false table, n_total, block_len, Case)"""
    blob, table, n_total, block_len, c = cg.refused_index()
    return blob, table, n_total, block_len, Case("refused_index", _of_source(c.source), [0] * len(c.ranges), c.ranges, c.align)
