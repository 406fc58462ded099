"""The call-chain generator (tests/chaingen.py) reaches its aim, checked without a GPU: the pair matrix is complete, the large
shapes exceed the small ones and the runtime's first capacities, every failing link fails by the oracle, every passing link's
container is accepted by it, and the host-only planners accept every link's arguments."""
import ctypes as C

import numpy as np
import pytest

import chaingen as cg
from chaingen import KINDS, SHAPES


@pytest.fixture(scope="module")
def tsq():
    import turbosqueeze_amd
    return turbosqueeze_amd


@pytest.fixture(scope="module")
def gen(oracle, tsq):
    return cg.Gen(oracle, tsq.synth)


@pytest.fixture(scope="module")
def every_link(gen):
    """every link the GPU tests enqueue: the pair matrix, the default-decoder pairs, the triples, both walks, and the failing link
    of every kind that has one"""
    links = [x for pair in gen.pairs() + gen.default_decoder_pairs() for x in pair]
    links += [x for chain in gen.triples() for x in chain] + [x for seed in (0, 1) for x in gen.walk(seed)]
    links += [gen.link(kind, "small", v, what) for (kind, what) in cg.FAILURES for v in range(4)]
    return list({id(x): x for x in links}.values())


def test_the_pair_matrix_holds_all_121_ordered_pairs_in_both_orders_of_shape(gen):
    pairs = gen.pairs()
    assert len(KINDS) == 11 and len(pairs) == 242
    seen = {(a.kind, b.kind, a.shape, b.shape) for a, b in pairs}
    assert seen == {(a, b, sa, sb) for a in KINDS for b in KINDS for sa, sb in (("small", "large"), ("large", "small"))}
    assert all(x.fail is None and x.source is None for pair in pairs for x in pair)
    assert set(cg.ENTRY) == set(KINDS) and len(set(cg.ENTRY.values())) == 11
    both_large = gen.default_decoder_pairs()
    assert {(a.kind, b.kind) for a, b in both_large} == {(a, b) for a in KINDS for b in KINDS if a in cg.DECODERS or b in cg.DECODERS}
    assert len(both_large) == 121 - 4 * 4 and all(a.shape == b.shape == "large" for a, b in both_large)


def test_large_shapes_exceed_the_small_ones_and_the_first_capacities(gen, tsq):
    # the restated constants against what this library was built from: the descriptor layouts the header publishes
    assert C.sizeof(tsq.RangeItem) == cg.SIZEOF_RANGE_ITEM == 24 and C.sizeof(tsq.BlockGroup) == cg.SIZEOF_BLOCK_GROUP == 16
    assert cg.SIZEOF_BATCH_ITEM == 48 and cg.SIZEOF_ENC_BATCH_BLOCK == 24 and cg.FIRST_BATCH_ITEMS == 256 and cg.FIRST_UPLOAD_BYTES == 4096
    assert cg.LARGE_ITEMS * 48 + cg.LARGE_ITEMS * 24 > 4096 and cg.LARGE_ITEMS > 256 and cg.LARGE_RANGES * 24 > 4096
    for kind in KINDS:
        smalls = [cg.scratch_quantities(gen.link(kind, "small", v)) for v in range(4)]
        larges = [cg.scratch_quantities(gen.link(kind, "large", v)) for v in range(4)]
        assert smalls[0] and all(q.keys() == smalls[0].keys() for q in smalls + larges), kind
        for name in smalls[0]:
            assert min(q[name] for q in larges) > max(q[name] for q in smalls), (kind, name)
        for q in smalls:
            # (a small batch is three one-block items, as many blocks as the large block work: behind a small batch only the large
            #  batches and reads grow the per-block scratch; every other order of kinds grows it)
            assert q.get("blocks", 1) == (cg.SMALL_ITEMS if kind in ("BC", "BD", "PC", "PD") else 1) and q.get("items", 0) <= cg.FIRST_BATCH_ITEMS and q.get("upload", 0) <= cg.FIRST_UPLOAD_BYTES, (kind, q)
        for q in larges:
            assert q.get("blocks", 2) >= 2, (kind, q)
            assert q.get("items", cg.FIRST_BATCH_ITEMS + 1) > cg.FIRST_BATCH_ITEMS, (kind, q)
            assert q.get("upload", cg.FIRST_UPLOAD_BYTES + 1) > cg.FIRST_UPLOAD_BYTES, (kind, q)
    # the shapes the issue fixes
    assert gen.link("C", "large").data.size == 2 * cg.BLOCK + 12_345 and gen.link("C", "large").blocks == 3
    assert all(5_000 <= gen.link("C", "small", v).data.size <= 70_000 for v in range(4))
    assert len(gen.link("BC", "large").spans) == 300 and len(gen.link("R", "large").ranges) == 400 == len(gen.link("I", "large").ranges)
    assert all(1 <= n <= 3_000 for _, n in gen.link("BC", "large").spans)
    assert {(gen.link("S", s, v).world, gen.link("S", s, v).rank) for s in SHAPES for v in range(4)} == {(1, 0), (2, 1)}


def test_every_failing_link_fails_by_the_oracle(gen, oracle):
    for v in range(4):
        for kind in ("D", "R"):
            x = gen.link(kind, "small", v, "twin")
            assert oracle.decompress(x.blob) is None and x.want_status == cg.ERR_STREAM, (kind, x.twin)
        for kind in ("BD", "PD"):
            x = gen.link(kind, "small", v, "twin")
            spans = x.spans if kind == "BD" else list(zip(x.offsets, x.sizes))
            verdicts = [oracle.decompress(x.arena[o:o + n]) for o, n in spans]
            assert [w is None for w in verdicts] == [i == x.bad for i in range(len(spans))] and x.want_status == cg.ERR_STREAM
            assert all(w == p.tobytes() for w, p in zip(verdicts, x.plains) if p is not None)
        x = gen.link("BC", "small", v, "room")
        sizes = [len(oracle.compress(x.arena[o:o + n], x.ext)) for o, n in x.spans]
        assert [s > r for s, r in zip(sizes, x.rooms)] == [i == x.tight for i in range(len(sizes))] and x.want_status == cg.ERR_OVERFLOW
        x = gen.link("PC", "small", v, "room")
        sizes = [len(oracle.compress(x.arena[o:o + n], x.ext)) for o, n in x.spans]
        assert sizes == x.sizes and x.offsets == cg.plan_packed(sizes, cg.ALIGN)
        assert x.offsets[x.tight] + sizes[x.tight] > x.out_size >= x.offsets[x.tight] and x.tight == len(sizes) - 1
        assert all(o + s <= x.out_size for o, s in zip(x.offsets[:x.tight], sizes)) and x.want_status == cg.ERR_OVERFLOW
        x = gen.link("D", "small", v, "count")
        assert x.stated != int.from_bytes(bytes(x.blob[4:8]), "little") and oracle.decompress(x.blob) == x.plain.tobytes()
        assert x.want_status == cg.ERR_FORMAT
    for seed in (0, 1):
        chain = gen.walk(seed)
        assert len(chain) == 40 and sorted((x.kind, x.fail) for x in chain if x.fail) == sorted(gen.WALK_FAILURES[seed])
        for k, x in enumerate(chain):
            if x.kind == "PD" and not x.fail:
                assert x.source is [y for y in chain[:k] if y.kind == "PC"][-1] and not x.source.fail
            if x.kind == "F":
                assert x.source is [y for y in chain[:k] if y.kind == "E"][-1]
    assert {x.shape for seed in (0, 1) for x in gen.walk(seed)} == set(SHAPES)
    assert {x.kind for seed in (0, 1) for x in gen.walk(seed)} == set(KINDS)


def test_every_passing_container_is_accepted_by_the_oracle(every_link, oracle):
    checked = 0
    for x in every_link:
        if x.fail:
            continue
        if x.kind in ("D", "S", "R"):
            blobs, plains = [x.blob], [x.plain.tobytes() if x.kind != "S" else None]
        elif x.kind == "F" and x.streams is not None:
            blobs, plains = [x.streams], [x.plain.tobytes()]
        elif x.kind in ("I", "BD"):
            blobs, plains = [x.arena[o:o + n] for o, n in x.spans], [p.tobytes() for p in x.plains]
        elif x.kind == "PD" and x.arena is not None:
            blobs, plains = [x.arena[o:o + n] for o, n in zip(x.offsets, x.sizes)], [p.tobytes() for p in x.plains]
        elif x.kind in ("C", "BC", "PC"):
            wants = [x.want] if x.kind == "C" else x.want
            blobs, plains = wants, [None] * len(wants)
        else:
            continue
        for blob, plain in zip(blobs, plains):
            got = oracle.decompress(np.ascontiguousarray(blob), threads=4)
            assert got is not None and (plain is None or got == plain), x
            checked += 1
        if x.kind == "S":
            whole = np.frombuffer(oracle.decompress(x.blob, threads=4), dtype=np.uint8)
            assert whole.size == x.total
            for k, (at, piece) in enumerate(x.pieces):
                b = x.rank + k * x.world
                assert at == k * cg.BLOCK and np.array_equal(piece, whole[b * cg.BLOCK:(b + 1) * cg.BLOCK])
    assert checked > 1000


def test_the_planners_accept_every_link(every_link, tsq):
    rng = np.random.default_rng(3)
    counted = dict.fromkeys(("R", "I", "BC", "BD", "PC"), 0)
    for x in every_link:
        if x.kind == "R":
            starts = [min(b * cg.BLOCK, x.total) for b in range(x.n_blocks)] + [x.total]
            outs, cap = fenced(rng, [ln for _, ln in x.ranges])
            items = tsq.plan_ranges(starts, [(o, ln, a) for (o, ln), a in zip(x.ranges, outs)], cap)
            assert len(items) >= len(x.ranges) and len(items) * cg.SIZEOF_RANGE_ITEM >= x.upload
        elif x.kind == "I":
            totals = [p.size for p in x.plains]
            starts = np.concatenate([[0], np.cumsum(totals)]).tolist()
            outs, cap = fenced(rng, [ln for _, _, ln in x.ranges])
            items, groups = tsq.plan_item_ranges(starts, list(range(len(totals) + 1)), [(i, o, ln, a) for (i, o, ln), a in zip(x.ranges, outs)], cap)
            assert len(items) == len(x.ranges) and len(groups) == x.n_groups
            assert ((len(items) * cg.SIZEOF_RANGE_ITEM + 15) & ~15) + len(groups) * cg.SIZEOF_BLOCK_GROUP == x.upload
        elif x.kind == "BC":
            outs, cap = fenced(rng, x.rooms)
            first = tsq.plan_batch([(o, n, a, r) for (o, n), a, r in zip(x.spans, outs, x.rooms)], x.arena.size, cap)
            assert first[-1] == x.blocks == len(x.spans)
        elif x.kind == "PC":
            bounds = [tsq.batch_bound(n) for _, n in x.spans]
            first = tsq.plan_batch([(o, n, sum(bounds[:k]), bounds[k]) for k, (o, n) in enumerate(x.spans)], x.arena.size, sum(bounds))
            assert first[-1] == x.blocks and tsq.plan_packed(x.sizes, cg.ALIGN) == x.offsets
        elif x.kind == "BD":
            outs, cap = fenced(rng, x.lengths)
            first = tsq.plan_batch([(o, n, a, ln) for (o, n), a, ln in zip(x.spans, outs, x.lengths)], x.arena.size, cap, [1] * len(x.spans))
            assert first[-1] == x.blocks
        else:
            continue
        counted[x.kind] += 1
    assert all(n >= 4 for n in counted.values()), counted


def fenced(rng, lengths):
    """as test_gpu_range.fenced: destinations behind gaps of 1..47 guard bytes"""
    at, outs = 0, []
    for ln in lengths:
        at += int(rng.integers(1, 48))
        outs.append(at)
        at += int(ln)
    return outs, at + 64
