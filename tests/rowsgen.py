"""Seeded cases for the gather into fixed-stride padded rows (tsqa_plan_gather_rows, tsqa_gather_rows_async, tsqa_gather_rows):
gathergen's ranges, but range k lands in row k, at k * stride, and the rest of the row is padding.  Shared by test_rows_cpu.py --
which shows with the oracle, the host frame walk and the host-only planner that each case reaches what it aims at -- and by
test_gpu_rows.py, which runs the same cases through the kernels.  Nothing here calls a kernel, and no input is made here: the
sources are gathergen's (cutgen's 600 tiny blocks, the 257 blocks of 4 096 bytes through both kinds of index, the batch of 300
containers with six damaged ones, the refused sized index).  The expected bytes of every row, the lengths, the statuses, both need
words and the full padded image are made here in pure Python by the rule of include/turbosqueeze_amd.h.

What is restated from the library, and must be re-derived when it changes there:
  row_rule     rows_measure_kernel (tsq_rows.cuh): gathergen.range_rule's gate and item rule, the NULL tables, the stride rule
  plan         rows_sum_kernel, rows_scan_kernel, rows_place_kernel and tsqa_plan_gather_rows: the piece numbers as an exclusive
               sum over the accepted rows, the fit of each row alone, the delivered lengths, both need words, the largest status
  image        rows_pad_kernel and the decoders: data, then the pad byte up to the stride; pad -1 leaves what was there
  GROUP        (a) and (c) take 256 rows per workgroup, (b) 256 groups per pass: the second pass starts at row 65 536
  WORD         rows_pad_kernel works in the 16-byte words of the destination address
"""
from __future__ import annotations

import functools

import numpy as np

import gathergen as gg

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = gg.OK, gg.ERR_ARG, gg.ERR_FORMAT, gg.ERR_STREAM, gg.ERR_OVERFLOW
GROUP, WORD = 256, 16
SEED = 9130
ALL_ONES = gg.ALL_ONES
NO_LIMIT_PIECES = (1 << 32) - 1
TRUNCATE = 1
COUNTS = (1, 2, 255, 256, 257, 513)
REPEATS = (65535, 65536, 65537)
STRIDES = (1, 5, 15, 16, 17, 40, 200, 4097)
PADS = (0, 0xA5, -1)
RESIDUES = tuple(range(16))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def row_rule(idx: gg.Index, item, offset, length, stride: int, truncate: bool):
    """RE-DERIVE with rows_measure_kernel -> (status, start in the concatenation, delivered length, accepted length).  offset None:
    0; length None: from the offset to the end of the item (or of the data)."""
    if idx.refused:
        return ERR_FORMAT, 0, 0, 0
    base, total = 0, idx.total
    offset = 0 if offset is None else offset
    if item is not None:
        if item >= idx.n_items or idx.item_first[item] >= idx.item_first[item + 1]:
            return ERR_ARG, 0, 0, 0
        base, total = idx.item_span(item)
    if length is None:
        if offset > total:
            return ERR_ARG, 0, 0, 0
        length = total - offset
    elif length > total or offset > total - length:
        return ERR_ARG, 0, 0, 0
    if length > stride:
        if not truncate:
            return ERR_OVERFLOW, 0, 0, length
        return OK, base + offset, stride, length
    return OK, (base + offset if length else 0), length, length


def plan(idx: gg.Index, n: int, items, offsets, lengths, stride: int, truncate: bool, cap_pieces: int):
    """RE-DERIVE with rows_place_kernel and tsqa_plan_gather_rows -> dict: row_lengths, row_status, status, need [pieces, largest
    accepted length], places [(start in the concatenation, delivered length)], pieces [[(block, lo, hi, out_at)] per row],
    fit_pieces, groups (the blocks the delivered rows touch)"""
    pick = lambda t, k: None if t is None else t[k]
    pieces_at, longest, row_lengths, status, places, pieces, touched = 0, 0, [], [], [], [], set()
    for k in range(n):
        st, start, ln, accepted = row_rule(idx, pick(items, k), pick(offsets, k), pick(lengths, k), stride, truncate)
        longest = max(longest, accepted)
        cut = gg.cut(idx.out_start, start, ln) if st == OK else []
        if st == OK and pieces_at + len(cut) > cap_pieces:
            st, ln = ERR_OVERFLOW, 0
        fits = st == OK
        status.append(st)
        row_lengths.append(ln if fits else 0)
        places.append((start, ln if fits else 0))
        pieces.append([(b, lo, hi, k * stride + d) for b, lo, hi, d in cut] if fits else [])
        if fits:
            touched.update(b for b, _, _, _ in cut)
        pieces_at += len(cut)
    return dict(row_lengths=row_lengths, row_status=status, status=max(status, default=OK), need=[pieces_at, longest], places=places,
                pieces=pieces, fit_pieces=sum(len(p) for p in pieces), groups=len(touched))


class Case:
    """n rows of `stride` bytes out of an index: items, offsets and lengths may each be None"""

    def __init__(self, name: str, index: gg.Index, stride: int, offsets=None, lengths=None, items=None, truncate: bool = False, data=None):
        ints = lambda t: None if t is None else [int(x) for x in t]
        self.name, self.index, self.stride, self.truncate = name, index, int(stride), bool(truncate)
        self.items, self.offsets, self.lengths = ints(items), ints(offsets), ints(lengths)
        tables = [t for t in (self.items, self.offsets, self.lengths) if t is not None]
        assert tables and all(len(t) == len(tables[0]) for t in tables)
        self.n = len(tables[0])
        self._expect = {}

    @property
    def flags(self) -> int:
        return TRUNCATE if self.truncate else 0

    def expect(self, cap_pieces: int = NO_LIMIT_PIECES):
        if cap_pieces not in self._expect:
            self._expect[cap_pieces] = plan(self.index, self.n, self.items, self.offsets, self.lengths, self.stride, self.truncate, cap_pieces)
        return self._expect[cap_pieces]

    def rows(self, e, data=None):
        """the bytes of every row: [uint8 array of row_lengths[k] bytes]"""
        src = np.frombuffer(self.index.data, dtype=np.uint8) if data is None else data
        return [src[start:start + ln] for start, ln in e["places"]]

    def image(self, e, pad: int, fill, data=None):
        """RE-DERIVE with rows_pad_kernel: the n * stride bytes the call owes over `fill` (what was there): every row's data, then
        pad up to the stride; pad -1: what was there"""
        out = np.array(fill[:self.n * self.stride], dtype=np.uint8, copy=True)
        assert len(out) == self.n * self.stride
        if pad >= 0:
            out[:] = pad
        for k, row in enumerate(self.rows(e, data)):
            out[k * self.stride:k * self.stride + len(row)] = row
        return out

    def dense_ranges(self, e):
        """the delivered rows as the dense gather takes them: (offsets into the concatenation, lengths), one range per row, a row
        without bytes as a range of length 0 at 0"""
        return [start if ln else 0 for start, ln in e["places"]], [ln for _, ln in e["places"]]


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def counts():
    """1: 1, 2, 255, 256, 257 and 513 rows over tiny(): gathergen's ranges of 0 to 200 bytes in rows of 200"""
    offsets, lengths = gg.tiny_ranges(max(COUNTS))
    return tuple(Case(f"rows_tiny_{n}", gg.tiny(), 200, offsets[:n], lengths[:n]) for n in COUNTS)


REPEAT_STRIDE = 16
REPEAT_UNIT = ((0, 16), (3, 5), (100, 0), (250, 16), (7000, 1), (41, 15), (9000, 16), (12, 12), (600, 7), (77, 16), (5, 3))


@functools.lru_cache(maxsize=None)
def repeated(n: int):
    """2: n rows of 16 bytes that repeat eleven ranges of tiny() (eleven does not divide 256: the groups' sums differ); at 65 537 rows
    the group scan makes a second pass, whose base is the carried sum"""
    total = gg.tiny().total
    unit = [(min(o, total - ln), ln) for o, ln in REPEAT_UNIT]
    return Case(f"rows_repeated_{n}", gg.tiny(), REPEAT_STRIDE, [unit[k % len(unit)][0] for k in range(n)], [unit[k % len(unit)][1] for k in range(n)])


def stride_source(stride: int) -> gg.Index:
    return gg.tiny() if stride <= 200 else gg.split("sized")


@functools.lru_cache(maxsize=None)
def strided(stride: int, truncate: bool):
    """3: rows of lengths 0, 1, stride - 1, stride and stride + 1 -- one of these ends, truncated, exactly on a block edge and one a
    byte past one --, then seeded lengths of 0 to stride + 1, 37 rows in all: at stride 1 a 16-byte word holds sixteen rows"""
    idx = stride_source(stride)
    rng = np.random.default_rng(SEED + stride)
    starts = idx.out_start
    edge = next(b for b in range(len(starts) // 2, len(starts) - 1) if starts[b] >= stride + 1 and starts[b] + 2 <= idx.total)
    rows = [(5, 0), (9, 1), (0, stride - 1), (starts[3], stride), (17, stride + 1),
            (starts[edge] - stride, stride + 1),             # its first `stride` bytes end exactly where block `edge` starts
            (starts[edge] - stride + 1, stride + 1)]         # ... one byte into block `edge`
    for _ in range(30):
        ln = int(rng.integers(0, stride + 2))
        rows.append((int(rng.integers(0, idx.total - ln + 1)), ln))
    return Case(f"rows_stride_{stride}{'_truncate' if truncate else ''}", idx, stride, [o for o, _ in rows], [ln for _, ln in rows], truncate=truncate)


EDGE_ROWS = (5, 6)                   # of strided(): the truncation that ends on a block edge, and the one a byte past it


@functools.lru_cache(maxsize=None)
def null_tables():
    """4: d_lengths NULL (to the end of the data: only a truncation fits, but for the last bytes), d_offsets NULL (from byte 0), and
    both NULL by item over the batch: whole items as rows, with and without truncation (the three-block items are too long for a
    row of 4 096 bytes, between fitting rows)"""
    tiny, batch = gg.tiny(), gg.batch()
    ends = [0, 1, tiny.total - 41, tiny.total - 40, tiny.total - 39, tiny.total - 1, tiny.total, tiny.total + 1, ALL_ONES, 977]
    items = list(range(gg.BATCH_ITEMS)) + [gg.BATCH_ITEMS, (1 << 32) - 1, 3, 3]
    by_item_offsets = [k % 5 for k in range(len(items))]
    return (Case("rows_lengths_null_truncate", tiny, 40, offsets=ends, truncate=True),
            Case("rows_lengths_null", tiny, 40, offsets=ends),
            Case("rows_offsets_null", tiny, 40, lengths=[0, 1, 39, 40, 41, tiny.total, tiny.total + 1, ALL_ONES, 17]),
            Case("rows_offsets_null_truncate", tiny, 40, lengths=[0, 1, 39, 40, 41, tiny.total, tiny.total + 1, ALL_ONES, 17], truncate=True),
            Case("rows_whole_items", batch, 4096, items=items),
            Case("rows_whole_items_truncate", batch, 4096, items=items, truncate=True),
            Case("rows_items_lengths_null", batch, 4096, items=items, offsets=by_item_offsets, truncate=True),
            Case("rows_items_offsets_null", batch, 64, items=items, lengths=[k % 3 for k in range(len(items))]))


REFUSAL_STRIDE = 5000                # gathergen's batch ranges are of up to 5 000 bytes
REFUSALS = gg.REFUSALS + ("offset_past_total_lengths_null",)


@functools.lru_cache(maxsize=None)
def refusal(name: str, at: int):
    """5: gathergen's 300 ranges by item with the refused one as row `at`; the last name is the rows' own: lengths NULL and an offset
    one past the item's total (an offset AT the total is accepted: a row without bytes)"""
    if name != "offset_past_total_lengths_null":
        c = gg.refusal(name, at)
        return Case(f"rows_{c.name}", c.index, REFUSAL_STRIDE, c.offsets, c.lengths, items=c.items)
    c = gg.batch_items()
    items, offsets = c.items[:300], c.offsets[:300]
    _, total = c.index.item_span(gg.REFUSAL_ITEM)
    items[at], offsets[at] = gg.REFUSAL_ITEM, total + 1
    other = (at + 1) % 300
    items[other], offsets[other] = gg.REFUSAL_ITEM, total
    return Case(f"rows_refusal_{name}_at_{at}", c.index, REFUSAL_STRIDE, offsets, None, items=items, truncate=True)


def refusal_cases():
    return [(name, at) for name in REFUSALS for at in gg.REFUSAL_AT]


@functools.lru_cache(maxsize=None)
def too_long():
    """6: rows longer than the stride between rows that fit, without truncation: each is refused alone"""
    return Case("rows_too_long_between", gg.tiny(), 40, [0, 100, 200, 300, 400, 500, 600], [10, 41, 40, 100, 0, 5, 4000])


ROOM_MIDDLE = 130


def rooms():
    """7: -> [(what, case, cap_pieces)] over the 257 rows of counts()"""
    c = counts()[4]
    e = c.expect()
    mid = next(k for k in range(ROOM_MIDDLE, c.n) if len(e["pieces"][k]) >= 3)
    before_mid = sum(len(p) for p in e["pieces"][:mid])
    return [("exactly the pieces needed", c, e["need"][0]),
            ("one piece short", c, e["need"][0] - 1),
            ("pieces that end inside a row of several", c, before_mid + 1),
            ("one piece", c, 1)]


@functools.lru_cache(maxsize=None)
def refused_case():
    """8: rows of a sized index whose container the device refuses: every one TSQA_ERR_FORMAT and all padding"""
    c = gg.refused_case()
    return Case("rows_refused_index", c.index, 128, c.offsets, c.lengths)


def healthy_cases():
    """every case whose index is not refused"""
    return (list(counts()) + [repeated(n) for n in REPEATS] + [strided(s, t) for s in STRIDES for t in (False, True)] + list(null_tables()) +
            [refusal(name, at) for name, at in refusal_cases()] + [too_long()])
