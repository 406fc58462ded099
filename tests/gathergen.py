"""Seeded cases for the gather (tsqa_plan_gather, tsqa_gather_async, tsqa_gather): record reads whose items, offsets and lengths
lie in device memory.  Shared by test_gather_cpu.py -- which shows with the oracle, the host frame walk and the host-only planners
that each case reaches what it aims at -- and by test_gpu_gather.py, which runs the same cases through the kernels.  Nothing here
calls a kernel.  The sources are cutgen's containers and a batch made here; the expected places, verdicts, pieces, groups and bytes
are made here in pure Python from the sources' data, by the rule of include/turbosqueeze_amd.h.

What is restated from the library, and must be re-derived when it changes there:
  range_rule   gather_measure_kernel (tsq_gather.cuh): the gate, the item rule, the range rule written without offset + length
  block_of     gather_block_of / plan_ranges' first_block: the last block that starts at or before a byte
  cut          gather_pieces_kernel / plan_ranges: a range cut at the block edges, empty blocks passed over
  plan         gather_layout_kernel and tsqa_plan_gather: tsqa_plan_packed's rule on the accepted lengths, the piece numbers, both
               fits, the first unfit range ending the prefix, d_out_offsets[n], *d_need_pieces, the largest status;
               then the sort by (block, lo) that keeps range order among equals (plan_item_ranges' std::stable_sort, the device's
               stable radix sort of block << 22 | lo) and the groups {block, first, count, largest hi} of gather_groups_kernel and
               gather_spans_kernel
  GROUP, WAVE, SPLIT   gather_layout_kernel is ONE workgroup of 256 threads (four wavefronts of 64) that takes the ranges 256 at a
               time; group_scan_excl64 (tsq_container.cuh) sums v & 0xFFFFFF and v >> 24 apart
  FLUSH        flush_group (tsq_dec_sym.cuh) reads a group's items 64 at a time
  KEY_LO_BITS  the sort key is block << 22 | lo
"""
from __future__ import annotations

import bisect
import functools

import numpy as np

import cutgen as cg
import densegen as dg
import seekgen as kg
import splitgen as sg

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = 0, 3, 4, 5, 6
GROUP, WAVE, SPLIT = dg.GROUP, dg.WAVE, dg.SPLIT
FLUSH = 64
KEY_LO_BITS = 22
SEED = 8420
ALL_ONES = (1 << 64) - 1
NO_LIMIT_BYTES, NO_LIMIT_PIECES = ALL_ONES, (1 << 32) - 1
COUNTS = (1, 2, 255, 256, 257, 513)
ALIGNS = (1, 16, 4096)
ONE_BLOCK_COUNTS = (63, 64, 65, 129, 1000)
BIG_BLOCKS, BIG_LEN = 65537, 4096


def round_up(v: int, align: int) -> int:
    return (v + align - 1) // align * align


# ---- what is read: an index as the library keeps it ----------------------------------------------------------------------------------------

class Index:
    """what a tsqa_index holds of its data: every block's start in the concatenation (out_start, n_blocks + 1), every item's first
    block (item_first, n_items + 1; a refused item owns no blocks) and the concatenation itself.  kind: 'plain' (tsqa_index_create
    of `blob`), 'sized' (tsqa_index_create_sized of `blob` with `table` and `block_len`) or 'batch' (tsqa_index_create_batch over
    `spans` of `blob`)."""

    def __init__(self, name, kind, blob, data, out_start, item_first=None, block_len=None, table=None, spans=None, refused=False):
        self.name, self.kind, self.blob, self.data = name, kind, blob, data
        self.out_start, self.block_len, self.table, self.spans, self.refused = list(out_start), block_len, table, spans, refused
        self.n_blocks = len(self.out_start) - 1
        self.item_first = list(item_first) if item_first is not None else [0, self.n_blocks]
        self.n_items = len(self.item_first) - 1
        self.total = self.out_start[-1]
        assert data is None or len(data) == self.total

    def item_span(self, i: int):
        """-> (start in the concatenation, total) of item i"""
        fb, fe = self.item_first[i], self.item_first[i + 1]
        return self.out_start[fb], self.out_start[fe] - self.out_start[fb]


def from_source(s: cg.Source, kind: str) -> Index:
    return Index(f"{s.name}_{kind}", kind, s.blob, s.data, s.out_start, block_len=s.block_len if kind == "sized" else None,
                 table=s.table if kind == "sized" else None)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def range_rule(idx: Index, item, offset: int, length: int):
    """RE-DERIVE with gather_measure_kernel -> (status, start in the concatenation, length); a refused range has no bytes.  item,
    offset and length are any 32- and 64-bit values; offset + length is never formed."""
    if idx.refused:
        return ERR_FORMAT, 0, 0
    base, total = 0, idx.total
    if item is not None:
        if item >= idx.n_items or idx.item_first[item] >= idx.item_first[item + 1]:
            return ERR_ARG, 0, 0
        base, total = idx.item_span(item)
    if length > total or offset > total - length:
        return ERR_ARG, 0, 0
    return OK, (base + offset if length else 0), length


def block_of(out_start, at: int) -> int:
    """RE-DERIVE with gather_block_of: the last block that starts at or before byte `at` (at < the total)"""
    return bisect.bisect_right(out_start, at) - 1


def cut(out_start, at: int, length: int):
    """RE-DERIVE with gather_pieces_kernel -> [(block, lo, hi, bytes of the range in front of the piece)], in block order"""
    out, end, nb = [], at + length, len(out_start) - 1
    if not length:
        return out
    b = block_of(out_start, at)
    while b < nb and out_start[b] < end:
        a, e = max(at, out_start[b]), min(end, out_start[b + 1])
        if a < e:
            out.append((b, a - out_start[b], e - out_start[b], a - at))
        b += 1
    return out


def plan(idx: Index, items, offsets, lengths, align: int, out_cap: int, cap_pieces: int):
    """RE-DERIVE with gather_layout_kernel, gather_pieces_kernel, the sort and gather_groups_kernel -> dict: out_offsets (n + 1),
    range_status, status, need (out_offsets[n]), need_pieces, fit_pieces, places [(start in the concatenation, length)] with
    length 0 wherever nothing is owed, items [(block, lo, hi, out_at)] in sorted order, groups [(block, first, count, hi)]"""
    n = len(offsets)
    rules = [range_rule(idx, None if items is None else items[k], offsets[k], lengths[k]) for k in range(n)]
    at, pieces_at, last, open_, out_offsets, status, places, cut_items = 0, 0, 0, True, [], [], [], []
    for st, start, ln in rules:
        pieces = cut(idx.out_start, start, ln)
        fits = st == OK and open_ and (ln == 0 or (at + ln <= out_cap and pieces_at + len(pieces) <= cap_pieces))
        if st == OK and not fits:
            open_ = False
        status.append(st if st != OK else OK if fits else ERR_OVERFLOW)
        out_offsets.append(at)
        places.append((start, ln if fits else 0))
        if fits:
            cut_items += [(b, lo, hi, at + d) for b, lo, hi, d in pieces]
        at, pieces_at, last = at + round_up(ln, align), pieces_at + len(pieces), ln
    out_offsets.append(at - round_up(last, align) + last if n else 0)
    order = sorted(range(len(cut_items)), key=lambda m: (cut_items[m][0], cut_items[m][1]))      # (sorted is stable)
    sorted_items = [cut_items[m] for m in order]
    groups = []
    for m, (b, lo, hi, _) in enumerate(sorted_items):
        if not groups or groups[-1][0] != b:
            groups.append([b, m, 0, 0])
        groups[-1][2] += 1
        groups[-1][3] = max(groups[-1][3], hi)
    return dict(out_offsets=out_offsets, range_status=status, status=max(status, default=OK), need=out_offsets[n], need_pieces=pieces_at,
                fit_pieces=len(cut_items), places=places, items=sorted_items, groups=[tuple(g) for g in groups])


class Case:
    """ranges of an index: items (None: offsets into the whole data), offsets, lengths, packed at `align`"""

    def __init__(self, name: str, index: Index, offsets, lengths, items=None, align: int = 1):
        self.name, self.index, self.align = name, index, align
        self.offsets, self.lengths = [int(x) for x in offsets], [int(x) for x in lengths]
        self.items = None if items is None else [int(x) for x in items]
        assert len(self.offsets) == len(self.lengths) and (self.items is None or len(self.items) == len(self.offsets))
        self._expect = {}

    @property
    def n(self) -> int:
        return len(self.offsets)

    def expect(self, out_cap: int = NO_LIMIT_BYTES, cap_pieces: int = NO_LIMIT_PIECES):
        key = (out_cap, cap_pieces)
        if key not in self._expect:
            self._expect[key] = plan(self.index, self.items, self.offsets, self.lengths, self.align, out_cap, cap_pieces)
        return self._expect[key]

    def item_ranges(self, e):
        """the fitting ranges as tsqa_plan_item_ranges takes them, (item, offset, length, out_at), with out_at from the layout; a
        case without items addresses the whole data as one item"""
        return [(0 if self.items is None else self.items[k], self.offsets[k], self.lengths[k], e["out_offsets"][k])
                for k in range(self.n) if e["range_status"][k] == OK]

    def output(self, e, fill, data=None):
        """the output the call owes: `fill` (a uint8 array of the room's length) with every owed range at its place"""
        out = fill.copy()
        src = np.frombuffer(self.index.data, dtype=np.uint8) if data is None else data
        for o, (start, ln) in zip(e["out_offsets"], e["places"]):
            if ln:
                out[o:o + ln] = src[start:start + ln]
        return out


# ---- sources --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny() -> Index:
    """cutgen's 600 blocks of 1 to 40 bytes"""
    return from_source(cg.tiny(), "plain")


@functools.lru_cache(maxsize=None)
def split(kind: str) -> Index:
    """cutgen's 257 blocks of 4 096 bytes, through a sized index or through tsqa_index_create"""
    return from_source(cg.split(), kind)


@functools.lru_cache(maxsize=None)
def random8() -> Index:
    """cutgen's eight blocks of 2^16 random bytes, through a sized index"""
    return from_source(cg.random8(), "sized")


BATCH_ITEMS = 300
BATCH_DAMAGE = {17: "bad_magic", 100: "count_0", 101: "total_plus_1", 255: "bad_magic", 256: "total_minus_1", 299: "count_0"}


@functools.lru_cache(maxsize=None)
def batch() -> Index:
    """300 small containers in one arena at multiples of 16: texts of 1 to 4 096 bytes in one block, every seventh one three
    blocks of 4 096 bytes (splitgen.expected_split), and six with densegen's damaged headers -- four refused at the header, two
    (total_plus_1, total_minus_1) by the frame walk, which leaves a gap in the table the index closes up"""
    rng = np.random.default_rng(SEED)
    pool = sg.count_input(64)
    blobs, datas = [], []
    for k in range(BATCH_ITEMS):
        if k % 7 == 3:
            data = pool[k * 64:k * 64 + 3 * 4096 - 5 * (k % 11)]
            blob, _ = sg.expected_split(dg._oracle(), data, 4096, k & 1)
            data = data.tobytes()
        else:
            it = dg._small(rng, 5000 + k)
            blob, data = it.blob, it.want
        how = BATCH_DAMAGE.get(k)
        if how == "bad_magic":
            blob = dg._with_header(blob, magic=b"TSQ2")
        elif how == "count_0":
            blob = dg._with_header(blob, count=0)
        elif how == "total_plus_1":
            blob = dg._with_header(blob, total=len(data) + 1)
        elif how == "total_minus_1":
            blob = dg._with_header(blob, total=len(data) - 1)
        blobs.append(blob)
        datas.append(None if how else data)
    at, spans = 0, []
    for b in blobs:
        at = round_up(at, 16)
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
    return Index("batch300", "batch", arena.tobytes(), bytes(cat), out_start, item_first=item_first, spans=spans)


@functools.lru_cache(maxsize=None)
def refused() -> Index:
    """cutgen's valid container of 300 blocks of 4 096 bytes with one of seekgen's false tables: a sized index refuses it on the device"""
    blob, table, n_total, block_len, case = cg.refused_index()
    return Index("refused_sized", "sized", blob, case.source.data, case.source.out_start, block_len=block_len, table=table, refused=True)


@functools.lru_cache(maxsize=None)
def big() -> Index:
    """65 537 blocks of 4 096 bytes of seekgen.scan_edge_input, the last one byte long; the container is made on the GPU by the
    split compress, so here there is only the geometry (data and blob None: the test compares with slices of the input)"""
    n_total = (BIG_BLOCKS - 1) * BIG_LEN + 1
    return Index("big", "sized", None, None, kg.out_start(n_total, BIG_LEN), block_len=BIG_LEN)


def big_input():
    return kg.scan_edge_input((BIG_BLOCKS - 1) * BIG_LEN + 1)


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

def tiny_ranges(n: int):
    """range k over tiny(): seeded offsets all over the data, lengths 0 to 200 (about one in sixteen empty): up to ~15 blocks each"""
    rng = np.random.default_rng(SEED + 1)
    total = tiny().total
    lengths = [0 if k % 16 == 5 else int(x) for k, x in enumerate(rng.integers(1, 201, n))]
    offsets = [int(rng.integers(0, total - ln + 1)) for ln in lengths]
    return offsets, lengths


@functools.lru_cache(maxsize=None)
def counts():
    """1: 1, 2, 255, 256, 257 and 513 ranges over tiny() at align 1 (prefixes of one list)"""
    offsets, lengths = tiny_ranges(max(COUNTS))
    return tuple(Case(f"tiny_{n}", tiny(), offsets[:n], lengths[:n]) for n in COUNTS)


@functools.lru_cache(maxsize=None)
def aligned(align: int):
    """2: the same 257 at an alignment"""
    offsets, lengths = tiny_ranges(max(COUNTS))
    return Case(f"tiny_257_align_{align}", tiny(), offsets[:257], lengths[:257], align=align)


def split_ranges():
    """offsets and lengths over cutgen's split source: inside a block, across one edge, across two, a whole block, the last bytes"""
    total = split("sized").total
    offsets = [0, 4090, 4096 * 3 - 1, 4096 * 10, 4096 * 200 + 17, total - 1, total - 4097, 4096 * 255 + 4000]
    lengths = [1, 12, 4098, 4096, 9000, 1, 4097, 192]
    rng = np.random.default_rng(SEED + 2)
    for _ in range(249):
        ln = int(rng.integers(1, 6000))
        offsets.append(int(rng.integers(0, total - ln + 1)))
        lengths.append(ln)
    return offsets, lengths


@functools.lru_cache(maxsize=None)
def shift_and_bisect():
    """3: the same 257 ranges over the same container through a sized index (the block by a shift) and tsqa_index_create (by bisection)"""
    offsets, lengths = split_ranges()
    return tuple(Case(f"split_{kind}", split(kind), offsets, lengths, align=16) for kind in ("sized", "plain"))


UNIT = 1 << 16


@functools.lru_cache(maxsize=None)
def carries():
    """4: ranges of 2^16 bytes out of random8(), so every place is a multiple of 2^16 and the places pass 2^24 at a known range:
    300 whole blocks (range 256: the first lane of the second pass, whose place is the carried sum); one range over all eight
    blocks in front (range 249: lane 57 of the fourth wavefront); nine such ranges and one of two blocks in front (range 192: lane
    0 of the fourth wavefront, whose place is made of the other wavefronts' totals)"""
    idx = random8()
    plain = [((k % 8) * UNIT, UNIT) for k in range(300)]
    long_front = [(0, 8 * UNIT)] + plain[1:]
    edge = [(0, 8 * UNIT)] * 9 + [(3 * UNIT, 2 * UNIT)] + plain[10:]
    return tuple(Case(name, idx, [o for o, _ in r], [ln for _, ln in r], align=16)
                 for name, r in (("carry_between_passes", plain), ("carry_inside_a_wavefront", long_front), ("carry_at_a_wavefront_edge", edge)))


CARRY_CROSSINGS = {"carry_between_passes": 256, "carry_inside_a_wavefront": 249, "carry_at_a_wavefront_edge": 192}


def crossing(case: Case) -> int:
    """the first range whose place is at or above 2^24"""
    return next(k for k, o in enumerate(case.expect()["out_offsets"]) if o >= SPLIT)


@functools.lru_cache(maxsize=None)
def whole():
    """5: one range over the whole data of tiny(): as many pieces as blocks"""
    return Case("whole_tiny", tiny(), [0], [tiny().total])


ONE_BLOCK = 5


@functools.lru_cache(maxsize=None)
def one_block(n: int):
    """6: n ranges of 1 to 200 bytes inside block 5 of random8(): one group.  Range 1 is range 0 again, range 2 starts where range 0
    does and is longer, range 3 starts there and is one byte long"""
    rng = np.random.default_rng(SEED + 3)
    lengths = [int(x) for x in rng.integers(1, 201, n)]
    offsets = [ONE_BLOCK * UNIT + int(rng.integers(0, UNIT - ln + 1)) for ln in lengths]
    if n >= 4:
        offsets[1], lengths[1] = offsets[0], lengths[0]
        offsets[2], lengths[2] = offsets[0], min(lengths[0] + 31, UNIT - (offsets[0] - ONE_BLOCK * UNIT))
        offsets[3], lengths[3] = offsets[0], 1
    return Case(f"one_block_{n}", random8(), offsets, lengths, align=1)


@functools.lru_cache(maxsize=None)
def shuffled():
    """7: 1 000 ranges over all of tiny(), in a seeded shuffle: unsorted, overlapping and repeating in the source"""
    rng = np.random.default_rng(SEED + 4)
    total = tiny().total
    lengths = [int(x) for x in rng.integers(1, 120, 1000)]
    offsets = [min(k * total // 1000, total - ln) for k, ln in enumerate(lengths)]
    order = rng.permutation(1000)
    return Case("shuffled_1000", tiny(), [offsets[k] for k in order], [lengths[k] for k in order], align=4)


BATCH_REFUSED_PROBE = (17, 101)      # ranges of refused items among the healthy ones: refused at the header, by the walk


@functools.lru_cache(maxsize=None)
def batch_items():
    """8: 600 ranges addressed by item over batch(): every healthy item twice -- a range at its start and one that ends with it --,
    the three-block items across their block edges, and ranges of refused items"""
    idx = batch()
    rng = np.random.default_rng(SEED + 5)
    items, offsets, lengths = [], [], []
    for k in range(2 * BATCH_ITEMS):
        i = k % BATCH_ITEMS
        _, total = idx.item_span(i) if idx.item_first[i] < idx.item_first[i + 1] else (0, 0)
        if total == 0:
            items.append(i); offsets.append(0); lengths.append(1 if i in BATCH_REFUSED_PROBE else 0)
            continue
        ln = int(rng.integers(1, min(total, 5000) + 1))
        items.append(i); lengths.append(ln); offsets.append(0 if k < BATCH_ITEMS else total - ln)
    return Case("batch_by_item", idx, offsets, lengths, items=items, align=16)


@functools.lru_cache(maxsize=None)
def batch_flat():
    """8: the flat form over the same index: offsets into the concatenation of the healthy items, across item edges"""
    idx = batch()
    rng = np.random.default_rng(SEED + 6)
    lengths = [int(x) for x in rng.integers(1, 9000, 300)]
    offsets = [int(rng.integers(0, idx.total - ln + 1)) for ln in lengths]
    return Case("batch_flat", idx, offsets, lengths, align=1)


REFUSAL_AT = (0, 256, 299)           # of 300 ranges: the first, the first lane of the second pass, the last
REFUSAL_ITEM = 10                    # a healthy item of batch()
REFUSALS = ("offset_at_total_length_1", "length_all_ones", "offset_all_ones", "item_is_items", "item_all_ones")


@functools.lru_cache(maxsize=None)
def refusal(name: str, at: int):
    """9: the first 300 ranges of batch_items() with the refused range `name` as range `at`"""
    c = batch_items()
    items, offsets, lengths = c.items[:300], c.offsets[:300], c.lengths[:300]
    _, total = c.index.item_span(REFUSAL_ITEM)
    items[at], offsets[at], lengths[at] = {
        "offset_at_total_length_1": (REFUSAL_ITEM, total, 1),
        "length_all_ones": (REFUSAL_ITEM, 1, ALL_ONES),
        "offset_all_ones": (REFUSAL_ITEM, ALL_ONES, 1),
        "item_is_items": (BATCH_ITEMS, 0, 1),
        "item_all_ones": ((1 << 32) - 1, 0, 1),
    }[name]
    return Case(f"refusal_{name}_at_{at}", c.index, offsets, lengths, items=items, align=16)


def refusal_cases():
    return [(name, at) for name in REFUSALS for at in REFUSAL_AT]


ROOM_MIDDLE = 130


def rooms():
    """10: -> [(what, case, out_cap, cap_pieces)] over aligned(16)"""
    c = aligned(16)
    e = c.expect()
    o = e["out_offsets"]
    mid = next(k for k in range(ROOM_MIDDLE, c.n) if c.lengths[k] > 3)
    before_mid = sum(len(cut(c.index.out_start, c.offsets[k], c.lengths[k])) for k in range(mid))
    return [("exactly the room needed", c, e["need"], e["need_pieces"]),
            ("one byte short of the last range", c, e["need"] - 1, e["need_pieces"]),
            ("room that ends inside a middle range", c, o[mid] + 3, e["need_pieces"]),
            ("one piece short", c, e["need"], e["need_pieces"] - 1),
            ("pieces that end inside a middle range", c, e["need"], before_mid + 1),
            ("one piece", c, e["need"], 1)]


@functools.lru_cache(maxsize=None)
def refused_case():
    """11: ranges of a sized index whose container the device refuses: every one TSQA_ERR_FORMAT, the bad ones too"""
    idx = refused()
    return Case("refused_index", idx, [0, 4090, idx.total - 1, idx.total, 0], [1, 100, 1, 1, 0], align=16)


@functools.lru_cache(maxsize=None)
def big_case():
    """12: over big(): ranges that straddle blocks 65 534 to 65 536 -- block numbers of 17 bits in the sort key -- and forty spread
    ones, unsorted"""
    idx = big()
    edge = (BIG_BLOCKS - 3) * BIG_LEN
    r = [(edge - 7, 20), (edge + BIG_LEN - 1, 2), (edge + 2 * BIG_LEN - 100, 101), (idx.total - 1, 1), (edge - 1, 2 * BIG_LEN + 2),
         (edge + 5, 1)]
    rng = np.random.default_rng(SEED + 7)
    for k in range(40):
        ln = int(rng.integers(1, 10000))
        r.append((int(rng.integers(0, idx.total - ln + 1)), ln))
    order = rng.permutation(len(r))
    return Case("big_65537", idx, [r[k][0] for k in order], [r[k][1] for k in order], align=16)


def healthy_cases():
    """every case whose index can be made from host bytes and is not refused"""
    return (list(counts()) + [aligned(a) for a in ALIGNS] + list(shift_and_bisect()) + list(carries()) + [whole()] +
            [one_block(n) for n in ONE_BLOCK_COUNTS] + [shuffled(), batch_items(), batch_flat()])
