"""Seeded cases and expectations for the index of a packed batch made from its device tables (tsqa_index_create_packed*,
tsqa_plan_index_packed), shared by test_packed_index_cpu.py -- which shows with the oracle, tsqa_walk_frames and the host-only
planner that each case reaches what it aims at -- and by test_gpu_packed_index.py, which runs the same cases through the kernels.
Nothing here calls a kernel, and no input is made here: the containers are densegen's, splitgen's, batchsplitgen's, mtgen's and
seekgen's.

What is restated from the library, and must be re-derived when it changes there:
  measure         batch_measure_kernel (tsq_batch.cuh): densegen.measure
  tables          pidx_tables_kernel (tsq_index_packed.cuh): the item's words inside the table, the header's count against them, the
                  header's total against the geometry
  fit             join_blocks_kernel (tsq_join.cuh): the block prefix over the accepted items, the first unfit item ends it
  walk            batch_walk_kernel<kWalkIndex>: splitgen.walk_refuses without a capacity
  sized_refuses   pidx_sum / scan / place / check_kernel: every frame's place from the item's words, sized_frame_ok, the geometry
  close_up        pidx_close_kernel and pidx_move_kernel: the healthy items' blocks and totals summed again
  GROUP, WAVE     the scans over the items are ONE workgroup of 256 threads (four wavefronts of 64), 256 items per pass; the sized
                  walk takes 256 blocks per workgroup and 256 groups per pass of its scan
  SPLIT           group_scan_excl64 (tsq_container.cuh) sums the low 24 bits and the rest of every value apart
"""
from __future__ import annotations

import functools

import numpy as np

import batchsplitgen as bsg
import densegen as dg
import mtgen
import seekgen as kg
import splitgen as sg

BLOCK = sg.BLOCK
HEADER, WORD, MIN_FRAME = sg.HEADER, sg.WORD, sg.MIN_FRAME
GROUP, WAVE, SPLIT = 256, 64, 1 << 24
OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = 0, 3, 4, 6
BUDGET = bsg.DEFAULT_BUDGET
SEED = 6270
EXT = 1


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

measure = dg.measure


def tables(nb: int, total: int, w0: int, w1: int, table_words: int, block_len: int) -> int:
    """RE-DERIVE with pidx_tables_kernel: the verdict on an item that measure accepted with nb blocks and `total` bytes"""
    if w0 > w1 or w1 > table_words:
        return ERR_ARG
    if w1 - w0 != nb or total > nb * block_len or total + block_len <= nb * block_len:
        return ERR_FORMAT
    return OK


def fit(blocks, cap_blocks: int):
    """RE-DERIVE with join_blocks_kernel: blocks[i] = an accepted item's count, 0 for a refused one -> (first_block n + 1 over the
    accepted items, the fitting prefix's end: the first accepted item that does not fit, len(blocks) when all do)"""
    first, fb, n_fit = [], 0, len(blocks)
    for i, b in enumerate(blocks):
        first.append(fb)
        if b and n_fit == len(blocks) and fb + b > cap_blocks:
            n_fit = i
        fb += b
    return first + [fb], n_fit


def walk(blob: bytes, nb: int, total: int):
    """RE-DERIVE with batch_walk_kernel<kWalkIndex> on a container whose header measure accepted -> the blocks' out_len, or None
    where the walk refuses"""
    n, at, oat, lens = len(blob), HEADER, 0, []
    for _ in range(nb):
        if at + MIN_FRAME > n:
            return None
        ln, out_len = int.from_bytes(blob[at:at + 3], "little") & 0x7FFFFF, int.from_bytes(blob[at + 3:at + 6], "little")
        if not sg.stream_len_ok(ln) or at + WORD + ln > n or out_len > BLOCK or oat + out_len > total:
            return None
        lens.append(out_len)
        oat += out_len
        at += WORD + ln
    return lens if oat == total else None


def sized_refuses(blob: bytes, nb: int, total: int, words, block_len: int):
    """RE-DERIVE with pidx_check_kernel on an item that `tables` accepted -> the blocks' out_len, or None where a block refuses
    its item.  A word outside [3, TSQ_OUTPUT_SZ] counts as nothing in the places behind it."""
    n, at, lens, bad = len(blob), HEADER, [], False
    for j in range(nb):
        s = int(words[j])
        if not sg.stream_len_ok(s):
            bad = True
            continue
        want = block_len if j + 1 < nb else total - j * block_len
        ok = at + MIN_FRAME <= n
        if ok:
            ln, out_len = int.from_bytes(blob[at:at + 3], "little") & 0x7FFFFF, int.from_bytes(blob[at + 3:at + 6], "little")
            ok = sg.stream_len_ok(ln) and at + WORD + ln <= n and out_len <= BLOCK and ln == s and out_len == want
        if ok:
            lens.append(out_len)
        else:
            bad = True
        at += WORD + s
    return None if bad else lens


def close_up(blocks, totals, status):
    """RE-DERIVE with pidx_close_kernel: the healthy items (status 0) alone -> (item_first n + 1, item_at n, live blocks, total)"""
    first, at, fb, t = [], [], 0, 0
    for b, tot, st in zip(blocks, totals, status):
        first.append(fb)
        at.append(t)
        if st == OK:
            fb += b
            t += tot
    return first + [fb], at, fb, t


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

class Case:
    """containers in an arena at multiples of 16, with the tables as a caller would hand them over (`offsets`, `sizes`; sized form:
    block_len, table_first, table, table_words -- the words the call may read, which may be fewer than the table holds) and what
    every item's data is (`datas`: bytes, or None where no decode owes any).  cap_blocks None: the blocks of all accepted items."""

    def __init__(self, name, blobs, datas, places=None, cap_blocks=None, block_len=None, table_first=None, table=None, table_words=None):
        self.name, self.blobs, self.datas, self.cap_blocks = name, [bytes(b) for b in blobs], list(datas), cap_blocks
        at, self.offsets = 0, []
        for b in self.blobs:
            at = dg.round_up(at, 16)
            self.offsets.append(at)
            at += len(b)
        self.arena = np.full(max(at, 1), 0xEE, dtype=np.uint8)
        for b, o in zip(self.blobs, self.offsets):
            self.arena[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        self.sizes = [len(b) for b in self.blobs]
        for k, how in (places or {}).items():                # (falsified by the tables' values only, as densegen.Batch does it)
            if how == "past":
                self.offsets[k] = at - self.sizes[k] + 3
            elif how == "short":
                self.sizes[k] = HEADER - 1
        self.block_len, self.table_first = block_len, table_first
        self.table = None if table is None else [int(x) & 0xFFFFFFFF for x in table]
        self.table_words = None if table is None else len(self.table) if table_words is None else table_words
        self.n = len(self.blobs)

    @property
    def sized(self):
        return self.table is not None

    def container(self, i):
        """the bytes the tables give item i, where they lie inside the arena"""
        return bytes(self.arena[self.offsets[i]:self.offsets[i] + self.sizes[i]])

    def expect(self, cap_blocks=None, plain=False):
        """-> dict of what the call owes: head (the verdict of measure and, sized, tables), blocks and totals (the headers' fields
        of the items head accepts, else 0), walk (what the walk says of an accepted item: 0 or ERR_FORMAT), item_status, item_first,
        item_at, words = [live blocks, total, blocks needed], status, out_len (per live block).  plain: the plain form on the same
        arena, whatever tables the case carries."""
        sized = self.sized and not plain
        size = self.arena.size
        head, blocks, totals = [], [], []
        for i in range(self.n):
            nb, total = measure(self.arena, size, self.offsets[i], self.sizes[i])
            st = OK if nb else ERR_FORMAT
            if st == OK and sized:
                st = tables(nb, total, self.table_first[i], self.table_first[i + 1], self.table_words, self.block_len)
            head.append(st)
            blocks.append(nb if st == OK else 0)
            totals.append(total if st == OK else 0)
        need = sum(blocks)
        cap = (self.cap_blocks if self.cap_blocks is not None else max(need, 1)) if cap_blocks is None else cap_blocks
        first, n_fit = fit(blocks, cap)
        status, walked, lens = [], [], []
        for i in range(self.n):
            st, w, mine = head[i], OK, None
            if st == OK:
                blob = self.container(i)
                mine = (sized_refuses(blob, blocks[i], totals[i], self.table[self.table_first[i]:self.table_first[i + 1]], self.block_len)
                        if sized else walk(blob, blocks[i], totals[i]))
                w = OK if mine is not None else ERR_FORMAT
                st = ERR_OVERFLOW if i >= n_fit else w
            status.append(st)
            walked.append(w)
            if st == OK:
                lens += mine
        item_first, item_at, live, total = close_up(blocks, totals, status)
        return dict(head=head, blocks=blocks, totals=totals, walk=walked, item_status=status, item_first=item_first, item_at=item_at,
                    words=[live, total, need], status=max(status), out_len=lens, cap_blocks=cap, first_block=first, n_fit=n_fit)


def _oracle():
    return dg._oracle()


def _of_dense(name, items, cap_blocks=None) -> Case:
    """a densegen batch's items as a case: its falsified places carried over"""
    places = {k: it.place for k, it in enumerate(items) if it.place}
    return Case(name, [it.blob for it in items], [it.want for it in items], places, cap_blocks)


def _of_split(name, b: bsg.Batch, cap_blocks=None, sized=False, ext=EXT) -> Case:
    """a batchsplitgen batch's expected containers as a case; sized: with its true tables"""
    made = b.made(_oracle(), ext)
    assert all(m is not None for m in made), name
    first, table = [0], []
    for _, sizes in made:
        table += sizes
        first.append(len(table))
    return Case(name, [m[0] for m in made], [b.item(i).tobytes() for i in range(len(made))], None, cap_blocks,
                *((b.block_len, first, table) if sized else ()))


ITEM_COUNTS = (1, 2, 255, 256, 257, 513)


@functools.lru_cache(maxsize=None)
def item_counts():
    """1, 2, 255, 256, 257 and 513 one-block items (prefixes of densegen.loop_edges' list)"""
    items = dg.loop_edges()[-1].items
    return tuple(_of_dense(f"items_{n}", items[:n]) for n in ITEM_COUNTS)


@functools.lru_cache(maxsize=None)
def three_blocks():
    """batchsplitgen.cap_batch: ten items, the sixth of three blocks of 4 KiB"""
    return _of_split("three_blocks", bsg.cap_batch())


@functools.lru_cache(maxsize=None)
def carry_totals():
    """densegen.carry_totals: 300 items, five of 4 MiB, placed so that the totals' scan passes 2^24 inside the first wavefront, and
    in the second wavefront out of the first one's total"""
    return tuple(_of_dense("totals_" + b.name, b.items) for b in dg.carry_totals())


@functools.lru_cache(maxsize=None)
def carry_places():
    """splitgen's 300 blocks of 2^16 random bytes as one item (batchsplitgen.crossing_alone), and behind a long item
    (crossing_fronted): in the sized form the frame places pass 2^24 inside a pass.  Both carry their true tables."""
    fronted, hit = bsg.crossing_fronted(_oracle(), BUDGET)
    return (_of_split("places_alone", bsg.crossing_alone(), sized=True), _of_split("places_fronted", fronted, sized=True)), hit


REFUSAL_AT = (0, 256, 299)


def _refusal_kinds():
    """-> [(name, dg.Item)]: densegen's damaged headers and bad places, mtgen's cut containers and a twin whose frame the walk refuses"""
    bad = [it for it in dg.refusals().items if it.fault == ERR_FORMAT]
    good = mtgen.damage_bases()[0][0]
    for name, blob in mtgen.header_and_tail_cases():
        if name.startswith("cut_") or name in ("n_blocks_plus_1", "n_blocks_minus_1"):
            bad.append(dg.Item("mt_" + name, blob, None, ERR_FORMAT))
    bad.append(dg.Item("mt_twin_walk", next(blob for _, blob, _, how in mtgen.twin_containers() if how == "walk"), None, ERR_FORMAT))
    assert len(good) > HEADER
    return bad


@functools.lru_cache(maxsize=None)
def refusals():
    """batches of 300 items: every refusal as item 0, item 256 and the last item, three kinds per batch in each of their three
    rotations, so that every kind -- the falsified places and the twin included -- stands in every one of the three places in some
    batch; healthy one-block items and mtgen's healthy container of eight blocks between them.  (A 'past' place is falsified by
    the table's value alone and ends three bytes behind the arena wherever the item stands, the last item included.)  Each case
    carries `kinds`: the names of its three refusals in the order of REFUSAL_AT."""
    kinds = _refusal_kinds()
    healthy = list(dg.loop_edges()[-1].items[:300])
    base, plain = mtgen.damage_bases()[0]
    healthy[5] = healthy[257] = dg.Item("mt_base", base, plain)
    out = []
    for r in range(0, len(kinds), 3):
        trio = [kinds[(r + j) % len(kinds)] for j in range(3)]
        for shift in range(3):
            order = trio[shift:] + trio[:shift]
            items = list(healthy)
            for at, it in zip(REFUSAL_AT, order):
                items[at] = it
            case = _of_dense("refusals_" + "_".join(it.name for it in order), items)
            case.kinds = tuple(it.name for it in order)
            out.append(case)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cap_cuts():
    """batchsplitgen.cap_cuts: cap_blocks exact, one short, ending inside the three-block item, and loose -> [(case, n_fit)]"""
    b, table = bsg.cap_cuts(BUDGET)
    return tuple((_of_split("cap_" + what.split(":")[0].replace(" ", "_"), b, cap_blocks=cap), n_fit) for what, cap, n_fit in table)


@functools.lru_cache(maxsize=None)
def sized_true():
    """batchsplitgen's batches at block_len 4096 with their true tables"""
    return (tuple(_of_split("sized_" + b.name, b, sized=True) for b in bsg.item_counts()) +
            (_of_split("sized_caps", bsg.cap_batch(), sized=True), _of_split("sized_edge_items", bsg.edge_items(), sized=True),
             _of_split("sized_align_mix", bsg.align_mix(16), sized=True)))


FALSE_AT = 100
FALSE_BLOCKS = 300


@functools.lru_cache(maxsize=None)
def sized_false():
    """batchsplitgen's 257 one-block items with item 100 an item of 300 blocks of 4 KiB (a prefix of splitgen.count_input), offered
    with each of seekgen's false tables -> [(case, why)]"""
    b = bsg.Batch("false_base", [bsg.small(k) for k in range(FALSE_AT)] + [bsg.big(BUDGET, FALSE_BLOCKS, 4095)] +
                  [bsg.small(k) for k in range(FALSE_AT + 1, 257)])
    made = b.made(_oracle(), EXT)
    blobs, datas = [m[0] for m in made], [b.item(i).tobytes() for i in range(257)]
    first, true = [0], []
    for _, sizes in made:
        true += sizes
        first.append(len(true))
    out = []
    for name, blob, n, table, why in kg.false_tables(*made[FALSE_AT]):
        mine = list(blobs)
        mine[FALSE_AT] = blob[:n]
        t = true[:first[FALSE_AT]] + list(table) + true[first[FALSE_AT + 1]:]
        d = list(datas)
        d[FALSE_AT] = None
        out.append((Case("false_" + name, mine, d, None, None, 4096, first, t), why))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sized_bad_first():
    """batchsplitgen.cap_batch with true words and a d_table_first that decreases at item 3, that ends one word past table_words,
    and that gives the three-block item one word too many -> [(case, {item: status})]"""
    base = _of_split("base", bsg.cap_batch(), sized=True)
    first, table, mid = base.table_first, base.table, bsg.CAP_MID
    make = lambda name, f, t, words=None: Case(name, base.blobs, base.datas, None, None, 4096, f, t, words)
    down = list(first)
    down[4] = first[3] - 1
    more = first[:mid + 1] + [x + 1 for x in first[mid + 1:]]
    return ((make("first_decreases", down, table), {3: ERR_ARG, 4: ERR_FORMAT}),
            (make("first_past_table_words", first, table, len(table) - 1), {base.n - 1: ERR_ARG}),
            (make("first_one_block_too_many", more, table[:first[mid + 1]] + [table[first[mid + 1] - 1]] + table[first[mid + 1]:]), {mid: ERR_FORMAT}))


@functools.lru_cache(maxsize=None)
def sized_geometry():
    """seekgen.geometry's plain item of one 4 MiB block offered as block_len 2^21 (two words), between one-block items"""
    name, blob, table, n_total, block_len, _ = next(g for g in kg.geometry(_oracle(), EXT) if g[0] == "plain_4mib_as_2mib")
    smalls = [sg.expected_split(_oracle(), bsg.small(k), block_len, EXT) for k in range(4)]
    blobs = [s[0] for s in smalls[:2]] + [blob] + [s[0] for s in smalls[2:]]
    datas = [bsg.small(k).tobytes() for k in range(2)] + [None] + [bsg.small(k).tobytes() for k in range(2, 4)]
    words = [s[1] for s in smalls[:2]] + [list(table)] + [s[1] for s in smalls[2:]]
    first, flat = [0], []
    for w in words:
        flat += w
        first.append(len(flat))
    return Case("geometry_" + name, blobs, datas, None, None, block_len, first, flat)


def plain_cases():
    return list(item_counts()) + [three_blocks()] + list(carry_totals()) + list(refusals()) + [c for c, _ in cap_cuts()]


def sized_cases():
    return (list(carry_places()[0]) + list(sized_true()) + [c for c, _ in sized_false()] + [c for c, _ in sized_bad_first()] +
            [sized_geometry()])


def every_case():
    return plain_cases() + sized_cases()


def ranges(case: Case, e, seed: int = SEED, per_item: int = 2, most: int = 48):
    """seeded record reads -> [(item, offset, length)]: of every item that is not healthy one range (which must be refused), of up
    to `most` healthy items `per_item` ranges inside their data -- the first and last healthy item, the items around every refused
    one and a seeded choice --, short and across block edges where the item has several blocks"""
    rng = np.random.default_rng(seed + case.n)
    healthy = [i for i in range(case.n) if e["item_status"][i] == OK]
    sick = [i for i in range(case.n) if e["item_status"][i] != OK]
    pick = set(healthy[:1] + healthy[-1:])
    for i in sick:
        pick |= {j for j in (i - 1, i + 1) if 0 <= j < case.n and e["item_status"][j] == OK}
    rest = [i for i in healthy if i not in pick]
    pick |= {int(i) for i in rng.choice(rest, size=min(len(rest), max(most - len(pick), 0)), replace=False)} if rest else set()
    out = [(i, 0, 1) for i in sick[:most]]
    for i in sorted(pick):
        total = e["totals"][i]
        for _ in range(per_item):
            ln = int(rng.integers(1, min(total, 5000) + 1))
            out.append((i, int(rng.integers(0, total - ln + 1)), ln))
        if total > 4096 + 3:
            out.append((i, 4096 - 3, 6))
    return out
