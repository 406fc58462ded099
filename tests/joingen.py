"""Seeded cases for the join of device-resident containers (tsqa_plan_join, tsqa_join_async, tsqa_join), shared by test_join_cpu.py
-- which shows with the oracle, the host frame walk and the host-only planner that each case reaches what it aims at -- and by
test_gpu_join.py, which runs the same cases through the kernels.  Nothing here calls a kernel.  The items are the oracle's
containers (densegen.healthy, splitgen.expected_split) and the damaged ones of densegen and mtgen; the expected join is made here in
pure Python from the containers' bytes, by the rule of include/turbosqueeze_amd.h:
    "TSQ1" | u32 sum(n_blocks_i) | u64 sum(total_i) | body_0 | ... | body_{N-1},  body_i = container i from 16 to the end of its last frame

What is restated from the library, and must be re-derived when it changes there:
  measure      batch_measure_kernel (tsq_batch.cuh), through densegen.measure: the place rule, then read_header (tsq_format.h)
  layout       join_blocks_kernel (tsq_join.cuh): the block prefix sum, complete whatever fits, and the prefix that fits cap_blocks
  walk         batch_walk_kernel<kWalkJoin> with walk_frames (tsq_format.h): the walk of one item without a capacity, and its frame
               bytes -- where its last frame ends
  plan_join    tsqa_plan_join (tsq_runtime.hip) and join_bodies_kernel: body_at, the joined header's fields, the size
  expect       the order of the five launches of tsqa_join_async: which verdict an item keeps, when the call's size is made, and
               that a nonzero status leaves the output and the table untouched
  GROUP, WAVE, SPLIT   both layout kernels are ONE workgroup of 256 threads (four wavefronts of 64) that takes the items 256 at a
               time; group_scan_excl64 (tsq_container.cuh) sums v & 0xFFFFFF and v >> 24 apart
  WORD16       join_emit_kernel moves 16-byte words cut at multiples of 16 of the destination address
"""
from __future__ import annotations

import functools

import numpy as np

import densegen as dg
import mtgen
import splitgen as sg

BLOCK, SLOT = sg.BLOCK, sg.OUTPUT_SZ
HEADER, WORD, MIN_FRAME = sg.HEADER, sg.WORD, sg.MIN_FRAME
GROUP, WAVE, SPLIT = dg.GROUP, dg.WAVE, dg.SPLIT
WORD16 = 16
OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = 0, 3, 4, 6
SEED = 6240
COUNTS = (1, 2, 255, 256, 257, 513)
ALIGNS = (1, 16, 4096)
TAILS = (1, 7, 4096)
SPLIT_BLOCKS = 2 * 512 + 1          # the short-block item: 2B + 1 blocks of 4 096 bytes at B = 2 x 256 CUs


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def measure(arena, arena_size: int, at: int, n: int):
    """RE-DERIVE with batch_measure_kernel -> (blocks, total) of an accepted item, (0, 0) of a refused one"""
    return dg.measure(arena, arena_size, at, n)


def layout(blocks, cap_blocks: int):
    """RE-DERIVE with join_blocks_kernel -> (first_block n + 1, n_fit): n_fit = the first accepted item (blocks > 0) whose blocks
    end past cap_blocks, len(blocks) when none does"""
    fb, first, n_fit = 0, [], len(blocks)
    for i, b in enumerate(blocks):
        first.append(fb)
        if b and n_fit == len(blocks) and fb + b > cap_blocks:
            n_fit = i
        fb += b
    return first + [fb], n_fit


def walk(blob, n_blocks: int, total: int):
    """RE-DERIVE with walk_frames as batch_walk_kernel<kWalkJoin> calls it, on a container whose header measure() has accepted with
    that count and total -> (frame_bytes, [stream_len]), or None where the walk refuses.  No capacity is asked."""
    n = len(blob)
    at, oat, sizes = HEADER, 0, []
    for _ in range(n_blocks):
        if at + MIN_FRAME > n:
            return None
        ln = int.from_bytes(bytes(blob[at:at + 3]), "little") & 0x7FFFFF
        out_len = int.from_bytes(bytes(blob[at + 3:at + 6]), "little")
        if not 3 <= ln <= SLOT or at + WORD + ln > n or out_len > BLOCK or oat + out_len > total:
            return None
        sizes.append(ln)
        oat += out_len
        at += WORD + ln
    return (at, sizes) if oat == total else None


def plan_join(frame_bytes, blocks, totals):
    """RE-DERIVE with tsqa_plan_join -> None where it answers TSQA_ERR_ARG, else (body_at n + 1, first_block n + 1, the header's block
    count as 32 bits, the header's total, the size, the return value: 0, or TSQA_ERR_OVERFLOW for a block sum of 2^32 or more)"""
    if not frame_bytes or not len(frame_bytes) == len(blocks) == len(totals):
        return None
    if any(b == 0 or f < HEADER + MIN_FRAME * b or t > b * BLOCK for f, b, t in zip(frame_bytes, blocks, totals)):
        return None
    at, fb, body_at, first = HEADER, 0, [], []
    for f, b in zip(frame_bytes, blocks):
        body_at.append(at)
        first.append(fb)
        at += f - HEADER
        fb += b
    return body_at + [at], first + [fb], fb & 0xFFFFFFFF, sum(totals), at, ERR_OVERFLOW if fb > 0xFFFFFFFF else OK


def joined(blobs):
    """the join of well-formed containers by the rule of the header, in pure Python -> (container, [stream_len of every block])"""
    bodies, sizes, nb, total = [], [], 0, 0
    for blob in blobs:
        k, t = int.from_bytes(blob[4:8], "little"), int.from_bytes(blob[8:16], "little")
        end, ln = walk(blob, k, t)
        bodies.append(bytes(blob[HEADER:end]))
        sizes += ln
        nb, total = nb + k, total + t
    return b"TSQ1" + nb.to_bytes(4, "little") + total.to_bytes(8, "little") + b"".join(bodies), sizes


# ---- items and cases ------------------------------------------------------------------------------------------------------------------

class Item:
    """one container as it lies in the arena (`blob`: the container, then `tail` bytes that d_sizes[i] claims behind its last
    frame), its data (None: a damaged container), the rule that refuses it (`rule`: None, 'place', 'header' or 'walk'), a
    falsified place ('past' or 'short') and `same_as`: the index of an earlier item whose place this one repeats"""

    def __init__(self, name, blob, data, rule=None, place=None, tail=0, same_as=None):
        self.name, self.data, self.rule, self.place, self.tail, self.same_as = name, data, rule, place, tail, same_as
        self.blob = bytes(blob) + bytes((7 * k + 3) & 0xFF for k in range(tail))
        assert (data is None) == (rule is not None), name


class Case:
    """items in an arena, each start a multiple of `align` (ragged: 7 k % 16 unused bytes in front of item k, so that the source
    and the destination of a body differ by every residue); behind the last container nothing lies"""

    def __init__(self, name, items, align=1, ragged=False):
        self.name, self.items, self.align = name, list(items), align
        at, self.offsets = 0, []
        for k, it in enumerate(self.items):
            if it.same_as is not None:
                self.offsets.append(self.offsets[it.same_as])
                continue
            at = dg.round_up(at + (7 * k % 16 if ragged else 0), align)
            self.offsets.append(at)
            at += len(it.blob)
        self.arena = np.full(at, 0xEE, dtype=np.uint8)
        for it, o in zip(self.items, self.offsets):
            self.arena[o:o + len(it.blob)] = np.frombuffer(it.blob, dtype=np.uint8)
        self.sizes = [len(it.blob) for it in self.items]
        for k, it in enumerate(self.items):
            if it.place == "past":                           # (by the table's value only: the place ends three bytes behind the arena)
                self.offsets[k] = at - len(it.blob) + 3
            elif it.place == "short":
                self.sizes[k] = HEADER - 1
        measured = [measure(self.arena, at, o, n) for o, n in zip(self.offsets, self.sizes)]
        self.blocks = [b for b, _ in measured]
        self.totals = [t for _, t in measured]
        self.need_blocks = sum(self.blocks)

    @property
    def healthy(self) -> bool:
        return all(it.rule is None for it in self.items)

    def walks(self):
        """per item: walk() of an item that measure() accepted, None of one it refused"""
        out = []
        for o, n, b, t in zip(self.offsets, self.sizes, self.blocks, self.totals):
            out.append(walk(self.arena[o:o + n], b, t) if b else None)
        return out

    def refused_by(self, k: int):
        """which of place, header and walk refuses item k, or None"""
        o, n = self.offsets[k], self.sizes[k]
        if not (n <= self.arena.size and o <= self.arena.size - n and n >= HEADER):
            return "place"
        if self.blocks[k] == 0:
            return "header"
        return "walk" if self.walks()[k] is None else None

    def expect(self, cap_blocks: int, out_cap: int):
        """RE-DERIVE with tsqa_join_async -> dict: item_status, first_block, status, out_size, and -- status 0 only -- container and
        block_sizes; on any other status not one byte of the output and not one word of the table is written"""
        first, n_fit = layout(self.blocks, cap_blocks)
        walks = self.walks()
        status = [ERR_FORMAT if b == 0 else ERR_OVERFLOW if i >= n_fit else OK if walks[i] is not None else ERR_FORMAT
                  for i, b in enumerate(self.blocks)]
        out = {"item_status": status, "first_block": first, "status": max(status), "out_size": 0, "container": None, "block_sizes": None}
        if out["status"] != OK:
            return out
        body_at, _, nb, total, size, rc = plan_join([w[0] for w in walks], self.blocks, self.totals)
        assert rc == OK
        out["out_size"], out["body_at"] = size, body_at
        if size > out_cap:
            out["status"] = ERR_OVERFLOW
            return out
        blob = bytearray(b"TSQ1" + nb.to_bytes(4, "little") + total.to_bytes(8, "little"))
        for o, w in zip(self.offsets, walks):
            blob += self.arena[o + HEADER:o + w[0]].tobytes()
        out["container"], out["block_sizes"] = bytes(blob), [s for w in walks for s in w[1]]
        return out

    def data(self) -> bytes:
        return b"".join(it.data for it in self.items)


def _oracle():
    return dg._oracle()


def _of(item: dg.Item, **kw) -> Item:
    return Item(item.name, item.blob, item.want, **kw)


@functools.lru_cache(maxsize=None)
def tiny(k: int) -> Item:
    """item k of the list of small items: 1 to 40 bytes of text, ext alternating; its container is 25 bytes and up"""
    n = 1 + (k * 23 + k // 40) % 40
    return _of(dg.healthy(n, 7000 + k, k & 1))


@functools.lru_cache(maxsize=None)
def random_item(n: int, seed: int, ext: int = 1) -> Item:
    data = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    return Item(f"random_{n}_{seed}", _oracle().compress(data, ext, threads=4 if n > BLOCK // 2 else 1), data.tobytes())


# ---- healthy cases --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def counts():
    """1, 2, 255, 256, 257 and 513 small items in a ragged arena (prefixes of one list): bodies of 9 bytes and up at every residue"""
    return tuple(Case(f"tiny_{n}", [tiny(k) for k in range(n)], 1, ragged=True) for n in COUNTS)


@functools.lru_cache(maxsize=None)
def aligned(align: int):
    """the 257 small items with every start a multiple of align"""
    return Case(f"tiny_257_align_{align}", [tiny(k) for k in range(257)], align)


@functools.lru_cache(maxsize=None)
def mix():
    """1 B, 2 B, 5 B, 70 000 B of text, 4 096 zeros and 4 MiB + 1 random bytes, ext alternating 0 / 1"""
    datas = [dg._text(1, 1), dg._text(2, 2), dg._text(5, 3), dg._text(70_000, 4), np.zeros(4096, dtype=np.uint8),
             np.random.default_rng(SEED).integers(0, 256, BLOCK + 1, dtype=np.uint8)]
    return Case("mix", [Item(f"mix_{k}_{d.size}", _oracle().compress(d, k & 1, threads=2), d.tobytes()) for k, d in enumerate(datas)], 16)


@functools.lru_cache(maxsize=None)
def short_blocks():
    """a container of 2B + 1 blocks of 4 096 bytes (splitgen.expected_split) between small items"""
    data = sg.count_input(512)[:(SPLIT_BLOCKS - 1) * 4096 + 1]
    blob, _ = sg.expected_split(_oracle(), data, 4096, 1)
    items = [tiny(k) for k in range(6)]
    items[3:3] = [Item("short_blocks", blob, data.tobytes())]
    return Case("short_blocks", items, 16)


@functools.lru_cache(maxsize=None)
def carry_inside():
    """300 items of 2^16 random bytes: their containers are longer than their data, so the body places pass 2^24 inside item 246:
    item 247's place is the first at or above it"""
    return Case("carry_inside_a_wavefront", [random_item(1 << 16, 8000 + k, k & 1) for k in range(300)], 16)


CARRY_EDGE_BIG_AT, CARRY_EDGE_CROSSING = 5, 3 * WAVE


@functools.lru_cache(maxsize=None)
def carry_edge():
    """the same items with one big item (under 4 MiB of random bytes) as item 5, sized so that the first body place at or above
    2^24 is item 192's: lane 0 of the fourth wavefront, whose place is made of the other wavefronts' totals alone"""
    small = [random_item(1 << 16, 8000 + k, k & 1) for k in range(299)]
    rest = sum(len(it.blob) - HEADER for it in small[:CARRY_EDGE_CROSSING - 1])       # the 191 small bodies before item 192
    body = len(small[0].blob) - HEADER
    n = int((SPLIT - HEADER - rest + body // 2) / (len(small[0].blob) / (1 << 16)))     # aim half a body past the crossing
    big = random_item(n, 8999, 1)
    items = small[:CARRY_EDGE_BIG_AT] + [big] + small[CARRY_EDGE_BIG_AT:]
    return Case("carry_at_a_wavefront_edge", items, 16)


def crossing(case: Case) -> int:
    """the first item whose body place is at or above 2^24"""
    body_at = case.expect(case.need_blocks, 1 << 62)["body_at"]
    return next(i for i, a in enumerate(body_at) if a >= SPLIT)


@functools.lru_cache(maxsize=None)
def twice():
    """the same container listed twice: item 2 repeats item 0's place"""
    a, b, c = tiny(3), tiny(8), dg.healthy(3000, 4000)
    return Case("twice", [_of(c), Item(a.name, a.blob, a.data), Item("again", c.blob, c.want, same_as=0), Item(b.name, b.blob, b.data)], 16)


@functools.lru_cache(maxsize=None)
def tails():
    """items whose d_sizes[i] claims 1, 7 and 4 096 bytes behind the last frame, each between small items"""
    items = [tiny(0)]
    for k, t in enumerate(TAILS):
        src = dg.healthy(500 + k, 4200 + k, k & 1)
        items += [Item(f"tail_{t}", src.blob, src.want, tail=t), tiny(10 + k)]
    return Case("tails", items, 1)


def healthy_cases():
    return list(counts()) + [aligned(a) for a in ALIGNS] + [mix(), short_blocks(), carry_inside(), carry_edge(), twice(), tails()]


def seams(case: Case):
    """-> (source residues of the body starts, destination residues of the seams, (source - destination) % 16 of the seams, the most
    items one 16-byte word of the output touches) of a healthy case whose output starts at a multiple of 16"""
    e = case.expect(case.need_blocks, 1 << 62)
    body_at = e["body_at"]
    src = {(o + HEADER) % WORD16 for o in case.offsets}
    dst = {a % WORD16 for a in body_at[1:-1]}
    shift = {(o + HEADER - a) % WORD16 for o, a in zip(case.offsets[1:], body_at[1:-1])}
    starts = np.array(body_at[:-1], dtype=np.int64)
    words = np.arange(body_at[0] // WORD16, (body_at[-1] + WORD16 - 1) // WORD16, dtype=np.int64) * WORD16
    first = np.searchsorted(starts, words, side="right") - 1
    last = np.searchsorted(starts, np.minimum(words + WORD16, body_at[-1]) - 1, side="right") - 1
    return src, dst, shift, int((last - first).max()) + 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

REFUSAL_AT = (0, 299, 256)          # of 300 items: the first, the last, and the first lane of the second pass
REFUSAL_NAMES = ("place_past", "place_short", "bad_magic", "count_0", "count_above", "total_above", "total_plus_1", "total_minus_1",
                 "n_blocks_plus_1", "n_blocks_minus_1", "cut_in_header", "cut_in_frame_word", "cut_in_size_word", "cut_mid_stream",
                 "cut_at_frame_end", "twin_walk")


@functools.lru_cache(maxsize=None)
def damaged():
    """-> ((name, rule, blob, place), ...): one damaged container per rule of place, header and walk.  The header rules are
    densegen.refusals'; the walk's are a total one off either way, a block count one off either way and every cut of
    mtgen.header_and_tail_cases, and the first container of mtgen.twin_containers whose frame the walk itself refuses."""
    base = dg.healthy(3000, 4000)
    nb_room = (len(base.blob) - HEADER) // MIN_FRAME
    out = [("place_past", "place", base.blob, "past"), ("place_short", "place", base.blob, "short"),
           ("bad_magic", "header", dg._with_header(base.blob, magic=b"TSQ2"), None),
           ("count_0", "header", dg._with_header(base.blob, count=0), None),
           ("count_above", "header", dg._with_header(base.blob, count=nb_room + 1), None),
           ("total_above", "header", dg._with_header(base.blob, total=BLOCK + 1), None)]
    for name, blob in mtgen.header_and_tail_cases():
        if name.startswith("trailing"):
            continue                                         # (legal: tails())
        out.append((name, "place" if len(blob) < HEADER else "walk", blob, None))
    name, blob = next((name, blob) for name, blob, _, how in mtgen.twin_containers() if how == "walk")
    out.append(("twin_walk", "walk", blob, None))
    assert tuple(n for n, _, _, _ in out) == REFUSAL_NAMES
    return tuple(out)


@functools.lru_cache(maxsize=None)
def refusal(name: str, at: int):
    """300 small items with the damaged container `name` as item `at`"""
    rule, blob, place = next((r, b, p) for n, r, b, p in damaged() if n == name)
    items = [tiny(k) for k in range(300)]
    items[at] = Item(name, blob, None, rule=rule, place=place)
    return Case(f"refusal_{name}_at_{at}", items, 16)


def refusal_cases():
    return [(name, at) for name in REFUSAL_NAMES for at in REFUSAL_AT]


# ---- room -----------------------------------------------------------------------------------------------------------------------------

def rooms():
    """-> [(what, case, cap_blocks, out_cap)]: blocks and bytes exactly as needed and one less, and a cut inside the item of many blocks"""
    c, s = aligned(16), short_blocks()
    size = c.expect(c.need_blocks, 1 << 62)["out_size"]
    first = layout(s.blocks, 0)[0]
    return [("exactly the room needed", c, c.need_blocks, size),
            ("one block short", c, c.need_blocks - 1, size),
            ("one byte short", c, c.need_blocks, size - 1),
            ("blocks for the items before the item of many blocks and one of its own", s, first[3] + 1, 1 << 24),
            ("one block", s, 1, 1 << 24)]
