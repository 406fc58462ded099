"""Seeded inputs for the packed batch entry points (tsqa_compress_batch_packed*, tsqa_decompress_batch_packed_async), shared by
test_packed_edges_cpu.py -- which shows with the oracle and the host-only planners that each input reaches what it aims at -- and by
the GPU tests, which run the same inputs through the kernels.  Nothing here calls a kernel: the only library code used is host code
(plan_packed, plan_batch, batch_bound, the synthetic-input helpers).

The constants mirror batch_pack_scan_packed_kernel and batch_route_enqueue (tsq_batch.cuh, tsq_runtime.hip) and must be re-derived
with them: an encode launch takes 2 x CUs blocks, the place-making kernel is ONE workgroup of 256 threads (four wavefronts of 64) that
takes the launch's blocks, and then its items, 256 at a time, and group_scan_excl64 sums the low 24 bits and the rest of every size
separately."""
from __future__ import annotations

import bisect
import functools

import numpy as np

import fuzzgen
import kat

MiB4 = 1 << 22
GROUP, WAVE = 256, 64           # items per iteration of the place-making loop; lanes of one DPP scan
SPLIT = 1 << 24                 # group_scan_excl64: v & 0xFFFFFF and v >> 24 are summed apart
HEADER, WORD = 16, 3            # container header, frame word (tsq_format.h)


def budget(cus):
    """blocks per encode launch"""
    return 2 * cus


def small_item(rng, k, n):
    from turbosqueeze_amd import synth
    kind = k % 4
    if kind == 0:
        return fuzzgen.structured(rng, n)
    if kind == 1:
        return kat.k7_textlike(n, seed=1000 + k)
    if kind == 2:
        return kat.xorshift32_bytes(n, seed=77 + k)
    return synth.text(n, seed=k)


def tiny(rng, k):
    return small_item(rng, k, int(rng.integers(64, 301)))


def first_blocks(lengths):
    """tsqa_plan_batch of a compress batch of items of these lengths -> each item's first block, then the block count"""
    import turbosqueeze_amd as tsq
    items, a, o = [], 0, 0
    for n in lengths:
        cap = tsq.batch_bound(n)
        items.append((a, n, o, cap))
        a += n
        o += cap
    return tsq.plan_batch(items, a, o)


def launches(lengths, cus):
    """the encode launches of a compress batch, as batch_route_enqueue cuts them and launch_items finds their items: (i0, i1, b0, nb)
    -- items [i0, i1) have blocks among the launch's blocks [b0, b0 + nb)"""
    first = first_blocks(lengths)
    n, out = len(lengths), []
    for b0 in range(0, first[-1], budget(cus)):
        nb = min(budget(cus), first[-1] - b0)
        out.append((bisect.bisect_right(first, b0) - 1, bisect.bisect_left(first, b0 + nb, 0, n), b0, nb))
    return out


# ---- sums above 2^24 ---------------------------------------------------------------------------------------------------------------

class CarryBatch:
    """datas: the items; big: the positions of the four items whose containers exceed 2^24 bytes"""

    def __init__(self, datas, big):
        self.datas, self.big = datas, big


@functools.lru_cache(maxsize=2)
def carry_batch(cus):
    """2 x CUs + 300 items of 64..300 bytes, but for four of 4 full blocks of incompressible bytes (a container of about 17.4 MB:
    its size has bits above the 24-bit split).  Three sit in the first launch, at item 3 (the first wavefront of the first
    iteration), 70 (the second wavefront) and 260 (the second iteration); the fourth sits in the second launch, at its item 100.
    Tiny items follow each, so that a sum with a high part is what places them."""
    rng = np.random.default_rng(31)
    n = budget(cus) + 300
    in_first = budget(cus) - 3 * 4 + 3            # items of the first launch: every block a tiny item's but the 12 of the big three
    big = [3, 70, 260, in_first + 100]
    datas = [kat.xorshift32_bytes(4 * MiB4, seed=900 + k) if k in big else tiny(rng, k) for k in range(n)]
    return CarryBatch(datas, big)


def carry_reach(cb, cus, sizes_by_ext):
    """the facts that make carry_batch(cus) a test of the scan's high half and of both carries; sizes_by_ext: the oracle's container
    lengths per level.  Raises AssertionError naming the fact that does not hold."""
    import turbosqueeze_amd as tsq
    ls = launches([d.size for d in cb.datas], cus)
    first = first_blocks([d.size for d in cb.datas])
    assert len(ls) == 2, f"{len(ls)} launches, not 2"
    (a0, a1, _, _), (c0, c1, _, _) = ls
    assert a0 == 0 and c0 == a1, f"an item straddles the launch seam: launches {ls}"
    for ext, sizes in sizes_by_ext.items():
        for b in cb.big:
            assert sizes[b] >= SPLIT, f"ext {ext}: big item {b} has a container of {sizes[b]} bytes, below 2^24"
        assert all(s < 1000 for k, s in enumerate(sizes) if k not in cb.big)
        for align in (16, 4096):
            assert tsq.plan_packed(sizes, align)[c0] >= SPLIT, f"ext {ext}, align {align}: the second launch starts below 2^24"
    p = [b - a0 for b in cb.big[:3]]
    assert p[0] < WAVE <= p[1] < 2 * WAVE and GROUP <= p[2] < a1 - a0, f"the big items of the first launch are its items {p}"
    assert c0 <= cb.big[3] < c1, f"big item {cb.big[3]} is not in the second launch {ls[1]}"
    for b, (i0, i1, b0, nb) in zip(cb.big, (ls[0], ls[0], ls[0], ls[1])):
        assert b0 <= first[b] and first[b + 1] <= b0 + nb, f"big item {b} is not complete in its launch"
        assert b + 1 < i1 and b + 1 not in cb.big, f"no tiny item follows big item {b} in its launch"
    assert (cb.big[3] - c0) // GROUP < (c1 - 1 - c0) // GROUP, "the second launch has no iteration behind the big item's"


# ---- the edges of the 256-item loop ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)
def loop_edge_batches(cus):
    """three batches of single-block tiny items whose last launch holds exactly 256, 257 and 1 items"""
    rng = np.random.default_rng(32)
    return tuple([tiny(rng, k) for k in range(budget(cus) + last)] for last in (GROUP, GROUP + 1, 1))


LOOP_EDGES = (GROUP, GROUP + 1, 1)


def last_launch_items(datas, cus):
    i0, i1, _, _ = launches([d.size for d in datas], cus)[-1]
    return i1 - i0


# ---- launch seams ---------------------------------------------------------------------------------------------------------------------

def seam_batch(cus):
    """-> (datas, a_at, b_at): item a_at's three blocks (text) straddle the first launch seam, item b_at's two blocks end the second
    launch exactly; every other item is tiny"""
    from turbosqueeze_amd import synth
    rng = np.random.default_rng(23)
    datas, blocks = [], 0
    while len(datas) < 2 * budget(cus) + 40:
        if blocks == budget(cus) - 2:
            n, a_at = 2 * MiB4 + 1, len(datas)
        elif blocks == 2 * budget(cus) - 2:
            n, b_at = 2 * MiB4, len(datas)
        else:
            n = int(rng.integers(64, 301))
        datas.append(synth.text(n, seed=len(datas)) if n > 300 else small_item(rng, len(datas), n))
        blocks += -(-n // MiB4)
    return datas, a_at, b_at


def inside_batch():
    """-> (datas, a_at, b_at): a three-block item of text and a two-block item among tiny ones, all in one launch"""
    from turbosqueeze_amd import synth
    rng = np.random.default_rng(33)
    datas = [tiny(rng, k) for k in range(30)]
    a_at, b_at = 7, 19
    datas[a_at] = synth.text(2 * MiB4 + 1, seed=a_at)
    datas[b_at] = synth.mix(2 * MiB4, seed=b_at)
    return datas, a_at, b_at


# ---- overflow cuts --------------------------------------------------------------------------------------------------------------------

def frames_of(raw):
    """(stream_at, stream_len) of every frame of a container (host bytes), as in test_gpu_range.py"""
    nb = int.from_bytes(bytes(raw[4:8]), "little")
    at, out = HEADER, []
    for _ in range(nb):
        ln = int(raw[at]) | int(raw[at + 1]) << 8 | (int(raw[at + 2]) & 0x7F) << 16
        out.append((at + WORD, ln))
        at += WORD + ln
    return out


def align_with_padding(sizes, k, aligns=(16, 256, 4096)):
    """the first of `aligns` that leaves at least two bytes of padding behind item k"""
    import turbosqueeze_amd as tsq
    for align in aligns:
        offsets = tsq.plan_packed(sizes, align)
        if offsets[k + 1] - offsets[k] - sizes[k] >= 2:
            return align
    raise AssertionError(f"no align of {aligns} leaves padding behind item {k}")


def cut_points(want, offsets, sizes, k=None):
    """named out_size values around item k of a packed batch (want: the oracle's containers; offsets: tsqa_plan_packed of sizes).
    k: an item of two or three blocks, not the first and not the last, with at least two bytes of padding behind it (by default the
    first item of three blocks, else the first of two)."""
    if k is None:
        nbs = [len(frames_of(w)) for w in want]
        k = nbs.index(3) if 3 in nbs else nbs.index(2)
    fr = frames_of(want[k])
    assert 0 < k < len(want) - 1 and len(fr) in (2, 3) and offsets[k + 1] - offsets[k] - sizes[k] >= 2
    end = [offsets[k] + at + ln for at, ln in fr]
    return {
        "header of item k fits, its first frame does not": offsets[k] + HEADER + 2,
        "exactly the end of item k's first frame": end[0],
        "one byte short of the end of item k's second frame": end[1] - 1,
        "exactly the end of item k": offsets[k] + sizes[k],
        "one byte into the padding behind item k": offsets[k] + sizes[k] + 1,
        "the start of item k + 1": offsets[k + 1],
        "exactly a header": HEADER,
    }


def fitting_image(want, offsets, out_size):
    """what a packed compress into out_size bytes must have written, as (lo, bytes) pieces: per item its header if it ends at or
    before out_size, then every frame (word and stream) that does; behind a frame that does not fit, none of that item's"""
    pieces = []
    for w, o in zip(want, offsets):
        if o + HEADER <= out_size:
            pieces.append((o, w[:HEADER]))
        for at, ln in frames_of(w):
            if o + at + ln > out_size:
                break
            pieces.append((o + at - WORD, w[at - WORD:at + ln]))
    return pieces


# ---- container sizes around a multiple of align --------------------------------------------------------------------------------------

_ORACLE = None


def _oracle():
    global _ORACLE
    if _ORACLE is None:
        from oracle.pyoracle import Oracle
        _ORACLE = Oracle()
    return _ORACLE


RESIDUES = {"an exact multiple": 0, "1 past a multiple": 1, "1 short of a multiple": -1}


@functools.lru_cache(maxsize=None)
def alignment_batch(align, ext=1):
    """at most 40 items: for each of the three residues two items of incompressible bytes whose container (at level ext) has that
    size modulo align -- found by a seeded walk over the item's length -- each followed by tiny items"""
    rng = np.random.default_rng(34 + align)
    orc = _oracle()
    datas, k = [], 0
    for copy in range(2):
        for r in RESIDUES.values():
            src = kat.xorshift32_bytes(40000, seed=300 + 7 * copy + (r % 5))
            n = int(rng.integers(200, 4000))
            for _ in range(400):
                assert n <= src.size
                d = (r - len(orc.compress(src[:n], ext))) % align
                if d == 0:
                    break
                n += max(1, d * 7 // 8) if d > 8 else 1      # (a literal-only stream grows by a little more than a byte per byte)
            else:
                raise AssertionError(f"no length found for residue {r} of align {align}")
            datas.append(src[:n].copy())
            for _ in range(int(rng.integers(1, 4))):
                datas.append(tiny(rng, k))
                k += 1
    assert len(datas) <= 40
    return tuple(datas)


def residues_present(sizes, align):
    """which of RESIDUES occur among the sizes of all items but the last (whose end is not rounded)"""
    return {name for name, r in RESIDUES.items() if any(s % align == r % align for s in sizes[:-1])}


# ---- the encoder catalogue in one input arena ------------------------------------------------------------------------------------------

def catalogue_arena(cases):
    """The encoder catalogue (encgen.catalogue()) as the input of one packed batch -> (arena, items), items = (case, in_at, in_len,
    with_halo).

    First every case back to back, no gap: the byte behind an item is the next item's first byte, and the look-ahead of an encoder
    that read past the item would see it.  Then, behind non-zero filler gaps of 0..47 bytes, every case that carries a halo once
    more with that halo laid behind it, as two overlapping input ranges: the data alone (with_halo False: the container is the
    case's own; the bytes behind the item are the very ones its builder chose to continue its last match) and the data with the
    halo (with_halo True: the container of data + halo, whose last bytes the first range must not have seen)."""
    rng = np.random.default_rng(35)
    items, at = [], 0
    for c in cases:
        items.append((c, at, len(c.data), False))
        at += len(c.data)
    lay = []
    for c in cases:
        if c.halo:
            at += int(rng.integers(0, 48))
            lay.append((at, c.data + c.halo))
            items.append((c, at, len(c.data), False))
            items.append((c, at, len(c.data) + len(c.halo), True))
            at += len(c.data) + len(c.halo)
    arena = rng.integers(1, 256, at + 64, dtype=np.uint8)
    for c, a, _, _ in items[:len(cases)]:
        arena[a:a + len(c.data)] = np.frombuffer(c.data, dtype=np.uint8)
    for a, b in lay:
        arena[a:a + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return arena, items


def item_bytes(item):
    c, _, _, with_halo = item
    return c.data + c.halo if with_halo else c.data
