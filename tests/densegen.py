"""Seeded batches for the dense decompress of a packed batch (tsqa_decompress_batch_packed_dense_async, tsqa_plan_dense), shared by
test_dense_cpu.py -- which shows with the oracle and the host-only planner that each batch reaches what it aims at -- and by
test_gpu_dense.py, which runs the same batches through the kernels.  Nothing here calls a kernel.  Containers are the oracle's, of
text (turbosqueeze_amd.synth.text, the tsq_synth generator): this codec expands zeros.

What is restated from the library, and must be re-derived when it changes there:
  measure      batch_measure_kernel (tsq_batch.cuh): the place rule of batch_place_kernel, then read_header (tsq_format.h), whose
               limits are plan_batch's (tsq_runtime.hip): count >= 1, count <= (size - 16) / 6, total <= count * TSQ_BLOCK_SZ
  layout       batch_layout_kernel and tsqa_plan_dense: tsqa_plan_packed's rule on the totals, the block sum, the fitting prefix
  GROUP, WAVE  batch_layout_kernel is ONE workgroup of 256 threads (four wavefronts of 64) that takes the items 256 at a time
  SPLIT        group_scan_excl64 sums v & 0xFFFFFF and v >> 24 apart
  walk verdicts   faultgen.walk_refuses (batch_walk_kernel<kWalkPerItem>)
"""
from __future__ import annotations

import functools

import numpy as np

import faultgen as fg
import mtgen

BLOCK = fg.BLOCK
HEADER, MIN_FRAME = fg.HEADER, fg.MIN_FRAME
GROUP, WAVE = 256, 64
SPLIT = 1 << 24
OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = 0, 3, 4, 5, 6
SEED = 5180
LOOP_COUNTS = (1, 255, 256, 257, 513)
ALIGNS = (1, 16, 4096)


def round_up(v: int, align: int) -> int:
    return -(-v // align) * align


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def measure(arena, arena_size: int, at: int, n: int):
    """RE-DERIVE with batch_measure_kernel -> (blocks, total) of an accepted item, (0, 0) of a refused one.  `arena` is indexed only
    inside [at, at + 16) of a well-placed item."""
    if not (n <= arena_size and at <= arena_size - n and n >= HEADER):
        return 0, 0
    head = bytes(arena[at:at + HEADER])
    if head[:4] != b"TSQ1":
        return 0, 0
    nb, total = int.from_bytes(head[4:8], "little"), int.from_bytes(head[8:16], "little")
    if nb == 0 or nb > (n - HEADER) // MIN_FRAME or total > nb * BLOCK:
        return 0, 0
    return nb, total


def layout(totals, blocks, align: int, out_size: int, cap_blocks: int):
    """RE-DERIVE with batch_layout_kernel / tsqa_plan_dense -> (out_offsets n + 1, first_block n + 1, n_fit): n_fit = the first
    accepted item (blocks > 0) that does not fit, len(totals) when all do."""
    n, at, fb = len(totals), 0, 0
    offsets, first, n_fit = [], [], len(totals)
    for i, (t, b) in enumerate(zip(totals, blocks)):
        t = t if b else 0
        offsets.append(at)
        first.append(fb)
        if b and n_fit == n and (fb + b > cap_blocks or at + t > out_size):
            n_fit = i
        fb += b
        at += t
        if i + 1 < n:
            at = round_up(at, align)
    return offsets + [at], first + [fb], n_fit


# ---- items and batches ----------------------------------------------------------------------------------------------------------------

class Item:
    """one container as it lies in the arena (`blob`), what a decode of it alone owes (`want`: its data, or None), the code a
    refusal carries (`fault`) and a falsified place (`place`: None, 'past' or 'short')"""

    def __init__(self, name, blob, want, fault=OK, place=None):
        self.name, self.blob, self.want, self.fault, self.place = name, bytes(blob), want, fault, place
        assert (want is None) == (fault != OK), name


class Batch:
    """items in a packed arena (tsqa_plan_packed's rule at 16) behind which nothing lies: the last container ends the arena"""

    def __init__(self, name, items, align):
        self.name, self.items, self.align = name, items, align
        at, self.offsets = 0, []
        for it in items:
            at = round_up(at, 16)
            self.offsets.append(at)
            at += len(it.blob)
        self.arena = np.full(at, 0xEE, dtype=np.uint8)
        for it, o in zip(items, self.offsets):
            self.arena[o:o + len(it.blob)] = np.frombuffer(it.blob, dtype=np.uint8)
        self.sizes = [len(it.blob) for it in items]
        for k, it in enumerate(items):
            if it.place == "past":                           # (by the table's value only: the place ends three bytes behind the arena)
                self.offsets[k] = at - len(it.blob) + 3
            elif it.place == "short":
                self.sizes[k] = HEADER - 1
        measured = [measure(self.arena, at, o, n) for o, n in zip(self.offsets, self.sizes)]
        self.blocks = [b for b, _ in measured]
        self.totals = [t for _, t in measured]
        self.need_bytes, self.need_blocks = (x[-1] for x in layout(self.totals, self.blocks, align, 0, 0)[:2])

    def expect(self, out_size: int, cap_blocks: int):
        """-> (out_offsets, first_block, statuses, out_sizes) the dense call owes with this room"""
        offsets, first, n_fit = layout(self.totals, self.blocks, self.align, out_size, cap_blocks)
        status = []
        for i, (it, b) in enumerate(zip(self.items, self.blocks)):
            status.append(ERR_FORMAT if b == 0 else ERR_OVERFLOW if i >= n_fit else it.fault)
        return offsets, first, status, [t if s == OK else 0 for t, s in zip(self.totals, status)]


@functools.lru_cache(maxsize=None)
def _text(n: int, seed: int):
    from turbosqueeze_amd import synth
    return synth.text(n, seed=seed)


_ORACLE = None


def _oracle():
    global _ORACLE
    if _ORACLE is None:
        from oracle.pyoracle import Oracle
        _ORACLE = Oracle()
    return _ORACLE


@functools.lru_cache(maxsize=None)
def healthy(n: int, seed: int, ext: int = 1) -> Item:
    data = _text(n, seed)
    return Item(f"text_{n}_{seed}", _oracle().compress(data, ext, threads=4 if n > BLOCK // 2 else 1), data.tobytes())


def _small(rng, k, lo=1, hi=4096) -> Item:
    return healthy(int(rng.integers(lo, hi + 1)), 100 + k, k & 1)


# ---- carry_totals ---------------------------------------------------------------------------------------------------------------------

CARRY_BIG_AT = {"inside_a_wavefront": (3, 10, 20, 40, 200), "across_a_wavefront_edge": (5, 30, 60, 66, 130)}


@functools.lru_cache(maxsize=None)
def carry_totals():
    """two batches of 300 items, 1 B to 4 KiB but for five of 4 MiB.  'inside_a_wavefront': four of them among the first 64 items,
    so the sum of that wavefront's own lanes passes 2^24; 'across_a_wavefront_edge': three among the first 64 and the fourth in the
    second wavefront, so only the first wavefront's total plus the second's own sum passes it."""
    rng = np.random.default_rng(SEED + 1)
    smalls = [_small(rng, k) for k in range(300)]
    out = []
    for name, big in CARRY_BIG_AT.items():
        items = [healthy(BLOCK, 900 + big.index(k)) if k in big else smalls[k] for k in range(300)]
        out.append(Batch(f"carry_totals_{name}", items, 16))
    return tuple(out)


def carry_reach(b: Batch):
    """the facts that make a carry_totals batch a test of the 24-bit split.  Raises AssertionError naming the one that fails."""
    padded = [round_up(t, b.align) for t in b.totals]
    assert sum(t == BLOCK for t in b.totals) == 5 and max(b.totals) == BLOCK
    waves = [padded[w:w + WAVE] for w in range(0, GROUP, WAVE)]
    own = [int(np.sum(w)) for w in waves]                              # each wavefront's own sum (first pass of the loop)
    low = [sum(v & (SPLIT - 1) for v in w) for w in waves]
    if b.name.endswith("inside_a_wavefront"):
        assert own[0] >= SPLIT and low[0] >= SPLIT, "the first wavefront's own low parts do not add up past 2^24"
        cum = np.cumsum(waves[0])
        assert cum[0] < SPLIT <= cum[-1] and int(np.argmax(cum >= SPLIT)) < WAVE - 1, "no lane of the wavefront sees the crossing"
    else:
        assert own[0] < SPLIT and own[1] < SPLIT <= own[0] + own[1], "the crossing is not made of the first wavefront's total"
        first_over = int(np.argmax(np.cumsum(padded) >= SPLIT))
        assert WAVE <= first_over < 2 * WAVE - 1, f"the sum passes 2^24 at item {first_over}, not inside the second wavefront"
    assert b.need_bytes > SPLIT and any(o >= SPLIT for o in layout(b.totals, b.blocks, b.align, 0, 0)[0][GROUP:]), "no start above 2^24 in the second pass"


# ---- loop_edges -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def loop_edges():
    """batches of 1, 255, 256, 257 and 513 items of 1 B to 4 KiB (prefixes of one list)"""
    rng = np.random.default_rng(SEED + 2)
    items = [_small(rng, 1000 + k) for k in range(max(LOOP_COUNTS))]
    return tuple(Batch(f"loop_edges_{n}", items[:n], 16) for n in LOOP_COUNTS)


def loop_reach(b: Batch):
    n = len(b.items)
    offsets, first, _ = layout(b.totals, b.blocks, b.align, 0, 0)
    assert all(1 <= t <= 4096 for t in b.totals) and all(x == 1 for x in b.blocks)
    for edge in (GROUP, 2 * GROUP):
        if n > edge:
            assert offsets[edge] > 0 and first[edge] == edge, f"no carry into the pass that starts at item {edge}"


# ---- two_blocks, alignment ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def two_blocks():
    """an item of 4 MiB + 1 B (two blocks) between small ones: first_block is not the item number behind it"""
    rng = np.random.default_rng(SEED + 3)
    items = [_small(rng, 2000 + k) for k in range(9)]
    items[4] = healthy(BLOCK + 1, 950)
    return Batch("two_blocks", items, 16)


@functools.lru_cache(maxsize=None)
def alignment(align: int):
    """totals of k * align - 1, k * align and k * align + 1, twice over, each followed by a small item"""
    rng = np.random.default_rng(SEED + 4 + align)
    items = []
    for k in ((2, 5) if align == 1 else (1, 3)):
        for d in (-1, 0, 1):
            items.append(healthy(k * align + d, 3000 + len(items)))
            items.append(_small(rng, 3100 + len(items)))
    return Batch(f"alignment_{align}", items, align)


def alignment_reach(b: Batch):
    a = b.align
    assert {t % a for t in b.totals[0::2]} == ({0} if a == 1 else {a - 1, 0, 1}), b.totals[0::2]
    offsets = layout(b.totals, b.blocks, a, 0, 0)[0]
    assert all(o % a == 0 for o in offsets[:-1])
    if a > 1:
        assert any(offsets[i + 1] - offsets[i] > b.totals[i] for i in range(len(b.items) - 1)), "no padding anywhere"


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def _with_header(blob: bytes, count=None, total=None, magic=None) -> bytes:
    nb, tot = int.from_bytes(blob[4:8], "little"), int.from_bytes(blob[8:16], "little")
    return (magic or blob[:4]) + (nb if count is None else count).to_bytes(4, "little") + (tot if total is None else total).to_bytes(8, "little") + blob[16:]


REFUSAL_NAMES = ("place_past", "place_short", "bad_magic", "count_0", "count_above", "total_above", "total_plus_1", "total_minus_1",
                 "stream_damaged")


@functools.lru_cache(maxsize=None)
def refusals():
    """one refused item per rule, each between two healthy ones (the batch starts and ends healthy).  The first six are refused at
    the header (no blocks, no room); the next two by the walk, with the room their headers ask for; the last by a block decoder."""
    rng = np.random.default_rng(SEED + 5)
    base = healthy(3000, 4000)
    nb_room = (len(base.blob) - HEADER) // MIN_FRAME
    twin = next(blob for _, blob, _, how in mtgen.twin_containers() if how == "stream")
    bad = [
        Item("place_past", base.blob, None, ERR_FORMAT, place="past"),
        Item("place_short", base.blob, None, ERR_FORMAT, place="short"),
        Item("bad_magic", _with_header(base.blob, magic=b"TSQ2"), None, ERR_FORMAT),
        Item("count_0", _with_header(base.blob, count=0), None, ERR_FORMAT),
        Item("count_above", _with_header(base.blob, count=nb_room + 1), None, ERR_FORMAT),
        Item("total_above", _with_header(base.blob, total=BLOCK + 1), None, ERR_FORMAT),
        Item("total_plus_1", _with_header(base.blob, total=len(base.want) + 1), None, ERR_FORMAT),
        Item("total_minus_1", _with_header(base.blob, total=len(base.want) - 1), None, ERR_FORMAT),
        Item("stream_damaged", twin, None, ERR_STREAM),
    ]
    assert tuple(it.name for it in bad) == REFUSAL_NAMES
    items = [_small(rng, 4100)]
    for k, it in enumerate(bad):
        items += [it, _small(rng, 4101 + k)]
    # ('past' moves the LAST container's worth of bytes: the place item must not be the last one, and it is not)
    return Batch("refusals", items, 16)


def refusal_reach(b: Batch, oracle):
    """every refused item is refused where its name says, and by the oracle too (or, for a place, never looked at)"""
    by = {it.name: (k, it) for k, it in enumerate(b.items)}
    assert [it.fault != OK for it in b.items] == [k % 2 == 1 for k in range(len(b.items))], "refused and accepted items do not alternate"
    n = b.arena.size
    for name in REFUSAL_NAMES:
        k, it = by[name]
        header_refuses = b.blocks[k] == 0
        assert header_refuses == (name in REFUSAL_NAMES[:6]), f"{name}: measured as {b.blocks[k]} blocks"
        if name == "place_past":
            assert b.offsets[k] < n < b.offsets[k] + b.sizes[k]
        elif name == "place_short":
            assert b.sizes[k] == HEADER - 1 and b.offsets[k] + b.sizes[k] <= n
        elif name == "count_above":
            assert int.from_bytes(it.blob[4:8], "little") == (len(it.blob) - HEADER) // MIN_FRAME + 1
        elif name == "total_above":
            assert int.from_bytes(it.blob[8:16], "little") == int.from_bytes(it.blob[4:8], "little") * BLOCK + 1
        if not header_refuses:
            walk = fg.walk_refuses(it.blob, b.blocks[k], b.totals[k])
            assert walk == (it.fault == ERR_FORMAT), f"{name}: the walk {'refuses' if walk else 'accepts'} it"
        if it.place is None:
            assert mtgen.expected_of_the_scheduler(oracle, it.blob) is None, f"{name}: the oracle delivers it"
    assert b.totals[by["total_plus_1"][0]] == 3001 and b.totals[by["total_minus_1"][0]] == 2999


# ---- cuts -----------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cuts():
    """-> (batch, [(what, out_size, cap_blocks, n_fit)]): twelve items, the fifth of two blocks, the eighth refused at its header;
    room exactly as needed and one byte or one block less, and cuts in the middle of the batch by bytes and by blocks"""
    rng = np.random.default_rng(SEED + 6)
    items = [_small(rng, 5000 + k, lo=100) for k in range(12)]
    items[4] = healthy(BLOCK + 1, 950)
    items[7] = Item("count_0", _with_header(items[7].blob, count=0), None, ERR_FORMAT)
    b = Batch("cuts", items, 16)
    offsets, first, _ = layout(b.totals, b.blocks, b.align, 0, 0)
    n, k = len(items), 6
    table = [
        ("exactly the room needed", b.need_bytes, b.need_blocks, n),
        ("one byte less", b.need_bytes - 1, b.need_blocks, n - 1),
        ("one block less", b.need_bytes, b.need_blocks - 1, n - 1),
        ("one byte short of the end of item 6", offsets[k] + b.totals[k] - 1, b.need_blocks, k),
        ("exactly the end of item 6 (the refused item 7 takes no room, item 8 does not fit)", offsets[k] + b.totals[k], b.need_blocks, k + 2),
        ("blocks for the items before the two-block item and one of its two", b.need_bytes, first[4] + 1, 4),
        ("no room at all", 1, 1, 0),
    ]
    return b, table


def every_batch():
    """every batch of the catalogue, each with the room it needs"""
    return list(carry_totals()) + list(loop_edges()) + [two_blocks()] + [alignment(a) for a in ALIGNS] + [refusals(), cuts()[0]]
