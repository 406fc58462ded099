"""Seeded batches for the packed batch compress of short blocks (tsqa_plan_batch_split, tsqa_compress_batch_packed_split*,
tsqa_plan_compress_tables_split, tsqa_compress_batch_packed_tables_split_async), shared by test_batch_split_cpu.py -- which shows with
the oracle and the host-only planners that each batch reaches what it aims at -- and by test_gpu_batch_split.py, which runs the same
batches through the kernels.  Nothing here calls a kernel.  An item's expected container is splitgen.expected_split of the item's own
bytes: its blocks' look-ahead runs on inside the item and sees zeros behind its last byte, whatever lies there in the input.

What is restated from the library, and must be re-derived when it changes there:
  plan_batch_split  tsqa_plan_batch_split (tsq_runtime.hip): the blocks per item, their prefix sum, and the bound, the sum of
                    round_up(splitgen.plan_split's bound, align) -- split_bound and block_bound (tsq_format.h)
  measure, layout   batch_measure_tables_kernel and batch_layout_tables_kernel (tsq_batch.cuh) with a block_len, and
                    tsqa_plan_compress_tables_split: an item of more than 2^32 - 1 blocks is refused like a bad place
  packed            tsqa_plan_packed's rule, applied to the container sizes (a size of 0 takes no room)
  image             the fit rule of batch_pack_scan_packed_body (tsq_batch.cuh): a header or frame is written only if it ends at or
                    before out_size
  DEFAULT_BUDGET    an encode launch takes 2 x CUs blocks (batch_budget, tsq_runtime.hip); the MI355X's 256 CUs.  The GPU tests take
                    the device's
  GROUP, WAVE       the pack scan is ONE workgroup of 256 threads, four wavefronts of 64, that takes the launch's blocks -- and its
                    items -- 256 at a time
  SPLIT             group_scan_excl64 (tsq_container.cuh) sums the low 24 bits and the rest of every value apart; the scan over a
                    launch's blocks starts from 0 in every launch (E[], batch_pack_scan_packed_body)
"""
from __future__ import annotations

import functools

import numpy as np

import splitgen as sg
import tablegen as tg
from tablegen import Alias, Refused  # noqa: F401  (the specs of the tables form)

BLOCK_LEN = 4096
DEFAULT_BUDGET = 2 * 256
GROUP, WAVE = 256, 64
SPLIT = 1 << 24
HEADER, WORD = sg.HEADER, sg.WORD
OK, ERR_ARG, ERR_OVERFLOW = 0, 3, 6
IN_MAX = 1 << 48
ALIGNS = (1, 16, 4096)
U32 = 0xFFFFFFFF


def round_up(v: int, align: int) -> int:
    return -(-v // align) * align


def align_ok(align) -> bool:
    return 1 <= align <= 4096 and align & (align - 1) == 0


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def packed(sizes, align: int):
    """RE-DERIVE with tsqa_plan_packed"""
    at, offsets = 0, []
    for i, z in enumerate(sizes):
        offsets.append(at)
        at += z
        if i + 1 < len(sizes):
            at = round_up(at, align)
    return offsets + [at]


def plan_batch_split(places, in_size: int, block_len: int, align: int):
    """RE-DERIVE with tsqa_plan_batch_split: places = (in_at, in_len) -> (first_block n + 1, bound), None where it answers TSQA_ERR_ARG"""
    if not places or block_len not in sg.BLOCK_LENS or not align_ok(align):
        return None
    first = [0]
    for at, n in places:
        if n == 0 or n > in_size or at > in_size - n:
            return None
        first.append(first[-1] + -(-n // block_len))
    if first[-1] > U32:
        return None
    return first, sum(round_up(sg.plan_split(n, block_len)[1], align) for _, n in places)


def measure(in_size: int, at: int, n: int, block_len: int) -> int:
    """RE-DERIVE with batch_measure_tables_kernel -> the blocks of an accepted item, 0 for a refused one"""
    nb = -(-n // block_len)
    return nb if 1 <= n <= in_size and at <= in_size - n and nb <= U32 else 0


def layout(in_offsets, in_sizes, in_size: int, block_len: int, align: int, cap_blocks: int):
    """RE-DERIVE with batch_layout_tables_kernel / tsqa_plan_compress_tables_split -> (first_block n + 1, item statuses, bound, n_fit)"""
    n, fb, bound = len(in_sizes), 0, 0
    first, status, n_fit = [], [], len(in_sizes)
    for i, (at, sz) in enumerate(zip(in_offsets, in_sizes)):
        nb = measure(in_size, at, sz, block_len)
        first.append(fb)
        if nb and n_fit == n and fb + nb > cap_blocks:
            n_fit = i
        status.append(ERR_ARG if nb == 0 else ERR_OVERFLOW if i >= n_fit else OK)
        fb += nb
        if nb:
            bound += round_up(sg.plan_split(sz, block_len)[1], align)
    return first + [fb], status, bound, n_fit


def launch_sums(block_sizes, budget: int):
    """E[] of every encode launch: the exclusive sums of 3 + size over the launch's blocks, from 0 -> [(b0, E)]"""
    out = []
    for b0, nb in sg.launches(len(block_sizes), budget):
        e = [0]
        for s in block_sizes[b0:b0 + nb]:
            e.append(e[-1] + WORD + s)
        out.append((b0, e))
    return out


def scan_crossings(block_sizes, budget: int):
    """the blocks at which a pass of the block scan first carries out of its low 24 bits: E[k] >= 2^24 while the pass's first
    block lies below it -> [(block, lane)]"""
    out = []
    for b0, e in launch_sums(block_sizes, budget):
        for k0 in range(0, len(e) - 1, GROUP):
            ks = [k for k in range(k0, min(len(e) - 1, k0 + GROUP)) if e[k0] < SPLIT <= e[k]]
            if ks:
                out.append((b0 + ks[0], ks[0] % GROUP))
    return out


# ---- batches --------------------------------------------------------------------------------------------------------------------------

class Batch:
    """specs: uint8 arrays (the item's own bytes, laid one after the other into the input with NO gap: the byte behind an item is
    the next item's first), tablegen.Refused or tablegen.Alias (the tables form only); slack: bytes behind them that belong to no item"""

    def __init__(self, name, specs, block_len=BLOCK_LEN, align=16, slack=64):
        self.name, self.specs, self.block_len, self.align = name, specs, block_len, align
        own = [s for s in specs if isinstance(s, np.ndarray)]
        self.data = np.concatenate(own + [sg.mixed(slack, 5) | 1])
        self.in_size = in_size = self.data.size
        at, places = 0, []
        for s in specs:
            places.append((at, s.size) if isinstance(s, np.ndarray) else None)
            at += s.size if isinstance(s, np.ndarray) else 0
        for k, s in enumerate(specs):
            if isinstance(s, Refused):
                places[k] = s.place(in_size)
            elif isinstance(s, Alias):
                places[k] = (places[s.of][0], places[s.of][1] if s.n is None else s.n)
        self.places = places
        self.in_offsets, self.in_sizes = [p[0] for p in places], [p[1] for p in places]
        self.blocks = [measure(in_size, a, z, block_len) for a, z in places]
        self.need_blocks = sum(self.blocks)
        self.host_form = all(self.blocks)                   # (the host forms refuse the whole call for a bad place)
        self._made = {}

    def item(self, i: int) -> np.ndarray:
        assert self.blocks[i]
        return self.data[self.in_offsets[i]:self.in_offsets[i] + self.in_sizes[i]]

    def made(self, oracle, ext: int):
        """-> per item (container, stream sizes), None for a refused item"""
        if ext not in self._made:
            self._made[ext] = [sg.expected_split(oracle, self.item(i), self.block_len, ext) if nb else None for i, nb in enumerate(self.blocks)]
        return self._made[ext]

    def expect(self, oracle, ext: int, cap_blocks=None, out_size=None, measuring: bool = False, per_item: bool = True):
        """-> dict of what a call owes.  per_item: the tables form (a verdict per item); else the host forms (one word: the last
        item tells).  cap_blocks None: the blocks needed; out_size None: all the room in the world.  block_sizes: the words
        [0, live); writes: per item the bytes of its container that land in the arena."""
        n = len(self.specs)
        cap = 0 if measuring else self.need_blocks if cap_blocks is None else cap_blocks
        first, status, bound, n_fit = layout(self.in_offsets, self.in_sizes, self.in_size, self.block_len, self.align, cap)
        if measuring:
            return dict(first_block=first, bound=bound, status=status, sizes=[0] * n, offsets=[0] * (n + 1), writes=[0] * n, n_fit=n_fit,
                        block_sizes=[], word=max(status))
        room = 1 << 62 if out_size is None else out_size
        made = self.made(oracle, ext)
        sizes = [len(made[i][0]) if st == OK else 0 for i, st in enumerate(status)]
        offsets = packed(sizes, self.align)
        writes, table = [], []
        for i, st in enumerate(status):
            if st != OK:
                writes.append(0)
                continue
            table += made[i][1]
            if offsets[i] + sizes[i] > room:
                status[i] = ERR_OVERFLOW
            writes.append(max([e for e in tg.pieces(made[i][0]) if offsets[i] + e <= room], default=0))
        word = max(status) if per_item else ERR_OVERFLOW if offsets[-1] > room else OK
        return dict(first_block=first, bound=bound, status=status, sizes=sizes, offsets=offsets, writes=writes, n_fit=n_fit,
                    block_sizes=table, word=word)

    def image(self, oracle, ext: int, e, guard):
        """the arena as it must be: `guard` with every owed piece laid in"""
        want = np.array(guard, dtype=np.uint8, copy=True)
        for i, w in enumerate(e["writes"]):
            if w:
                want[e["offsets"][i]:e["offsets"][i] + w] = np.frombuffer(self.made(oracle, ext)[i][0], dtype=np.uint8)[:w]
        return want


def small(k: int) -> np.ndarray:
    """one of tablegen's texts of 1 B to 4 KiB: one block at every block_len"""
    return np.frombuffer(tg.small(k), dtype=np.uint8)


def big(budget: int, n_blocks: int, last: int = BLOCK_LEN) -> np.ndarray:
    """n_blocks blocks of 4 KiB, the last of `last` bytes: a prefix of splitgen.count_input, so the oracle's blocks are shared"""
    assert n_blocks <= 2 * budget + 1
    return sg.count_input(budget)[:(n_blocks - 1) * BLOCK_LEN + last]


EDGE_SIZES = (1, 4095, 4096, 4097, 2 * 4096 + 1)


@functools.lru_cache(maxsize=None)
def edge_items():
    """items of 1, 4095, 4096, 4097 and 2 x 4096 + 1 bytes of text, random bytes and zeros"""
    from turbosqueeze_amd import synth
    rng = np.random.default_rng(8101)
    specs = []
    for n in EDGE_SIZES:
        specs += [synth.text(n, seed=n), rng.integers(0, 256, n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)]
    return Batch("edge_items", specs)


ITEM_COUNTS = (1, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def item_counts():
    return tuple(Batch(f"items_{n}", [small(k) for k in range(n)]) for n in ITEM_COUNTS)


@functools.lru_cache(maxsize=None)
def ownership(budget: int):
    """one item of exactly B blocks, of B + 1 and of 2B + 1 (a launch, or two, whose blocks all belong to it), alone and between
    one-block items; an item of three blocks that starts on the last block of a launch; one that ends on the first block of a launch"""
    out = []
    for nb, last in ((budget, BLOCK_LEN), (budget + 1, 1), (2 * budget + 1, 4095)):
        out.append(Batch(f"alone_{nb}", [big(budget, nb, last)]))
        out.append(Batch(f"between_{nb}", [small(1), small(2), big(budget, nb, last), small(3)]))
    out.append(Batch("starts_on_last_block", [small(k) for k in range(budget - 1)] + [big(budget, 3, 17), small(4)]))
    out.append(Batch("ends_on_first_block", [small(k) for k in range(budget - 2)] + [big(budget, 3, 17), small(4)]))
    return tuple(out)


def owners(b: Batch, budget: int):
    """-> per launch the set of items with blocks in it"""
    first = layout(b.in_offsets, b.in_sizes, b.in_size, b.block_len, b.align, b.need_blocks)[0]
    out = []
    for b0, nb in sg.launches(first[-1], budget):
        out.append({i for i in range(len(b.specs)) if first[i] < b0 + nb and first[i + 1] > b0})
    return out


CROSS_LEN = 1 << 16


@functools.lru_cache(maxsize=None)
def crossing_alone():
    """splitgen.carry_input: ONE item of 300 blocks of 2^16 random bytes, every stream longer than its block: inside one launch and
    inside one item, E[] and the frame places pass 2^24 before block 256"""
    data, bl = sg.carry_input()
    assert bl == CROSS_LEN
    return Batch("crossing_alone", [data], block_len=bl)


def crossing_fronted(oracle, budget: int):
    """the same behind an item of splitgen's phrase (streams of a few KiB), so long that the block at which the scan carries is a
    wavefront's first lane inside a pass"""
    data, bl = sg.carry_input()
    sizes = sg.expected_split(oracle, data, bl, 1)[1]
    for front in range(1, 3 * WAVE):
        long = sg.edge_input(bl, front)[0]
        hits = scan_crossings(sg.expected_split(oracle, long, bl, 1)[1] + sizes, budget)
        if hits and hits[0][1] % WAVE == 0 and hits[0][0] >= front:
            return Batch("crossing_fronted", [long, data], block_len=bl), hits[0]
    raise AssertionError("no front length puts the crossing at a wavefront's first lane")


@functools.lru_cache(maxsize=None)
def lookahead():
    """splitgen's phrase, whose matches cross every block edge, cut into two adjacent items in the middle of the phrase: the match
    under way at the first item's last byte would run on into the second item"""
    whole, bl = sg.edge_input(BLOCK_LEN, 6)
    cut = 3 * BLOCK_LEN - 7
    return Batch("lookahead", [whole[:cut].copy(), whole[cut:].copy()]), whole


@functools.lru_cache(maxsize=None)
def align_mix(align: int):
    """257 items, every 40th of three to five blocks"""
    specs = [sg.mixed((3 + k % 3) * BLOCK_LEN - k, 30 + k) if k % 40 == 7 else small(k) for k in range(257)]
    return Batch(f"align_mix_{align}", specs, align=align)


ROOM_MID = 4


@functools.lru_cache(maxsize=None)
def room_batch():
    """nine items, the fifth of four blocks"""
    specs = [small(13 * k) for k in range(9)]
    specs[ROOM_MID] = sg.mixed(3 * BLOCK_LEN + 55, 77)
    return Batch("room", specs)


def room_cuts(oracle, ext: int):
    """-> (batch, [(what, out_size)])"""
    b = room_batch()
    e = b.expect(oracle, ext)
    used, at = e["offsets"][-1], e["offsets"][ROOM_MID]
    ends = tg.pieces(b.made(oracle, ext)[ROOM_MID][0])
    return b, [("exact", used), ("one byte short", used - 1), ("inside a header", at + 9), ("inside a frame word", at + ends[1] + 1),
               ("inside a middle item", at + (ends[2] + ends[3]) // 2), ("a header and no more", 16)]


@functools.lru_cache(maxsize=None)
def refusals(budget: int):
    """every refused place as item 0, as item 256, directly behind the item that ends the first launch, and as the last item, between
    healthy one-block items and one of three blocks"""
    specs = [Refused("size_0")] + [small(5 * k) for k in range(255)] + [Refused("size_in_size_plus_1")]
    specs += [small(3 * k) for k in range(budget - 255)]                       # (item 256 + budget - 255 holds block budget - 1)
    specs += [Refused("offset_one_past"), Refused("wraps")] + [small(1), big(budget, 3, 9), small(2)] + [Refused("size_2_63")]
    return Batch("refusals", specs)


CAP_MID = 5


@functools.lru_cache(maxsize=None)
def cap_batch():
    """ten items, the sixth of three blocks"""
    specs = [small(11 * k) for k in range(10)]
    specs[CAP_MID] = sg.mixed(2 * BLOCK_LEN + 9, 78)
    return Batch("caps", specs)


def cap_cuts(budget: int):
    """-> (batch, [(what, cap_blocks, n_fit)])"""
    b = cap_batch()
    n, need = len(b.specs), b.need_blocks
    return b, [("exact", need, n), ("one short", need - 1, n - 1), ("inside item 5: it ends the prefix although item 6 would fit", CAP_MID + 1, CAP_MID),
               ("a dead launch and a dead tail", need + budget + 1, n)]


@functools.lru_cache(maxsize=None)
def overlaps():
    """two items over the same bytes, an item that is a prefix of a three-block item and ends inside its second block"""
    return Batch("overlaps", [small(1), sg.mixed(2 * BLOCK_LEN + 100, 79), Alias(1), small(3), Alias(1, BLOCK_LEN + 17), Alias(0)])


def every_batch(budget: int = DEFAULT_BUDGET):
    """every batch whose expectation needs nothing but the oracle (crossing_fronted is made with it)"""
    return ([edge_items()] + list(item_counts()) + list(ownership(budget)) + [crossing_alone(), lookahead()[0]] +
            [align_mix(a) for a in ALIGNS] + [room_batch(), refusals(budget), cap_batch(), overlaps()])
