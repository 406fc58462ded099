"""The call-chain generator (tests/chaingen.py) reaches its aim, checked without a GPU: the pair matrix is complete, the large
shapes exceed the small ones and the runtime's first capacities, every failing link fails by the oracle, every passing link's
container is accepted by it, and the host-only planners accept every link's arguments."""
import ctypes as C

import numpy as np
import pytest

import chaingen as cg
import splitgen as sg
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
    assert set(cg.ENTRY) == set(cg.ALL_KINDS) and len({cg.ENTRY[k] for k in KINDS}) == 11 and len(set(cg.ENTRY.values())) == 23
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


# ---- the second catalogue (chaingen.NEW_KINDS, tests/test_gpu_call_chains_device.py) ---------------------------------------------------

NEW = cg.NEW_KINDS


@pytest.fixture(scope="module")
def every_new_link(gen):
    """every link of a new kind that the GPU tests of the second catalogue enqueue: the pair matrix, the default-decoder pairs,
    both walks with their wired links, the pipelines, and the failing link of every kind that has one"""
    links = [x for pair in gen.pairs2() + gen.default_decoder_pairs2() for x in pair]
    links += [x for seed in (0, 1) for x in gen.walk2(seed)] + [x for chain in gen.pipelines() for x in chain]
    links += [gen.link(kind, "small", v, what) for (kind, what) in cg.FAILURES2 for v in range(4)]
    return [x for x in {id(x): x for x in links}.values() if x.kind in NEW]


def walk_host(tsq, blob):
    """tsqa_walk_frames -> (rc, stream sizes, out_lens, total)"""
    L = tsq.lib()
    raw = np.frombuffer(bytes(blob), dtype=np.uint8)
    cap = int.from_bytes(bytes(blob[4:8]), "little") + 1
    frame_at, sizes, ext, out_len = (C.c_uint64 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    nb, total = C.c_uint32(0), C.c_uint64(0)
    rc = L.tsqa_walk_frames(raw.ctypes.data, raw.size, cap, frame_at, sizes, ext, out_len, C.byref(nb), C.byref(total))
    return rc, list(sizes[:nb.value]), list(out_len[:nb.value]), total.value


def test_the_second_pair_matrix_names_every_pair_with_a_new_kind_once_per_order_of_shape(gen):
    pairs = gen.pairs2()
    assert len(cg.ALL_KINDS) == 23 and len(NEW) == 12 and cg.ALL_KINDS[:11] == KINDS and len(pairs) == 816 == 2 * (23 * 23 - 11 * 11)
    seen = [(a.kind, b.kind, a.shape, b.shape) for a, b in pairs]
    assert len(set(seen)) == 816
    assert set(seen) == {(a, b, sa, sb) for a in cg.ALL_KINDS for b in cg.ALL_KINDS if a in NEW or b in NEW
                         for sa, sb in (("small", "large"), ("large", "small"))}
    assert all(x.fail is None and x.source is None for pair in pairs for x in pair)
    # both variants of the kinds that have two entry points or two addressing modes occur, in both shapes
    for kind, field in (("DI", "packed"), ("TC", "split"), ("XP", "sized")):
        assert {(x.shape, getattr(x, field)) for pair in pairs for x in pair if x.kind == kind} == {(s, f) for s in SHAPES for f in (False, True)}, kind
    assert {(x.shape, x.g_items is None) for pair in pairs for x in pair if x.kind == "G"} == {(s, f) for s in SHAPES for f in (False, True)}
    assert {(x.shape, x.ranges is None) for pair in pairs for x in pair if x.kind == "T"} == {(s, f) for s in SHAPES for f in (False, True)}
    both_large = gen.default_decoder_pairs2()
    assert {(a.kind, b.kind) for a, b in both_large} == {(a, b) for a in cg.ALL_KINDS for b in cg.ALL_KINDS if "SD" in (a, b)}
    assert len(both_large) == 45 and all(a.shape == b.shape == "large" for a, b in both_large)
    assert set(cg.WRITES_FRAMES2) <= set(NEW) and not set(cg.WRITES_FRAMES2) & set(cg.WRITES_FRAMES)


def test_new_small_links_lie_under_the_first_capacities_and_large_links_over_them(gen):
    firsts = {"items": cg.FIRST_BATCH_ITEMS, "ranges": cg.FIRST_CUT_RANGES, "table_blocks": cg.FIRST_TABLE_BLOCKS, "upload": cg.FIRST_UPLOAD_BYTES}
    assert cg.FIRST_JOIN_ITEMS == cg.FIRST_BATCH_ITEMS == cg.FIRST_CUT_RANGES == cg.FIRST_GATHER_RANGES == cg.FIRST_TABLE_BLOCKS == 256
    for kind in NEW:
        smalls = [cg.scratch_quantities2(gen.link(kind, "small", v)) for v in range(4)]
        larges = [cg.scratch_quantities2(gen.link(kind, "large", v)) for v in range(4)]
        assert smalls[0] and all(q.keys() == smalls[0].keys() for q in smalls + larges), kind
        for name in smalls[0]:
            assert min(q[name] for q in larges) > max(q[name] for q in smalls), (kind, name)
        for q in smalls:
            assert all(q[name] <= first for name, first in firsts.items() if name in q), (kind, q)
            assert q.get("blocks", 1) <= 6 and q.get("pieces", 1) <= 2 * cg.SMALL_RANGES, (kind, q)
        for q in larges:
            assert all(q[name] > first for name, first in firsts.items() if name in q), (kind, q)
            assert q.get("blocks", 257) > 256 and q.get("pieces", 257) > 256, (kind, q)
            # (the launch table of 16 entries is not exceeded: an encode launch takes 2 x CUs blocks, 64 on the smallest chip thought of)
            assert -(-q.get("table_blocks", 1) // 64) <= cg.FIRST_TABLE_LAUNCHES, (kind, q)
    # the shapes the issue fixes
    for v in range(4):
        for kind in ("SC", "SD"):
            small, large = gen.link(kind, "small", v), gen.link(kind, "large", v)
            assert (small.blocks, large.blocks) == (3, 300)
        for shape, nb in (("small", 3), ("large", 300)):
            n = gen.link("SC", shape, v).data.size
            assert (nb - 1) * cg.SPLIT_LEN < n < nb * cg.SPLIT_LEN, "no short last block"
        assert sorted(gen.link("PS", "small", v).item_blocks) == [1, 2, 3] and max(gen.link("PS", "large", v).item_blocks) == 3
        assert sum(gen.link("PS", "large", v).item_blocks) > 256 < sum(gen.link("TC", "large", v).item_blocks)
        for kind in ("DI", "DD", "TC", "XP", "J"):
            assert (gen.link(kind, "small", v).items, gen.link(kind, "large", v).items) == (3, 300), kind
        for kind in ("K", "T", "G"):
            assert (gen.link(kind, "small", v).n_ranges, gen.link(kind, "large", v).n_ranges) == (3, 400), kind
        assert (len(gen.link("XS", "small", v).ranges), len(gen.link("XS", "large", v).ranges)) == (3, 400)
        assert (gen.link("XS", "small", v).n_blocks, gen.link("XS", "large", v).n_blocks) == (3, 300)
        for kind in ("DI", "DD", "TC", "XP", "J"):
            x = gen.link(kind, "large", v)
            sizes = x.lengths if kind == "DI" else [len(p) for p in (x.plains if kind in ("DD", "TC") else x.case.datas if kind == "XP" else [])]
            assert all(1 <= n <= 3_000 for n in sizes), kind
    g = gen.link("G", "large", 0)
    assert any(o // cg.BLOCK != (o + n - 1) // cg.BLOCK for o, n in zip(g.offsets, g.lengths)), "no gather range across a block edge"
    x = gen.link("XS", "large", 0)
    assert any(o // cg.SPLIT_LEN != (o + n - 1) // cg.SPLIT_LEN for o, n in x.ranges)


def test_every_new_expectation_is_consistent_with_the_oracle(every_new_link, gen, oracle, tsq):
    dec = lambda blob: oracle.decompress(np.frombuffer(bytes(blob), dtype=np.uint8), threads=4)
    seen = dict.fromkeys(NEW, 0)
    for x in every_new_link:
        k = x.kind
        if k == "DI":
            for (o, n), p in zip(x.spans, x.plains):
                assert dec(x.arena[o:o + n]) == p.tobytes(), x
        elif k == "DD":
            assert x.out_offsets == cg.plan_packed([len(p) if p is not None else s for p, s in zip(x.plains, x.batch.totals)], cg.ALIGN)
            for i, (o, n, p) in enumerate(zip(x.offsets, x.sizes, x.plains)):
                got = dec(x.batch.arena[o:o + n])
                assert (got is None and x.item_status[i] == cg.ERR_STREAM and x.out_sizes[i] == 0) if p is None else (got == p and x.out_sizes[i] == len(p)), (x, i)
        elif k in ("TC", "PS"):
            spans = list(zip(x.in_offsets, x.in_sizes)) if k == "TC" else x.spans
            for i, ((o, n), c) in enumerate(zip(spans, x.containers)):
                if c is None:
                    assert k == "TC" and i == x.bad and o + n > x.data.size and x.sizes[i] == 0 and x.item_status[i] == cg.ERR_ARG
                    continue
                item = x.data[o:o + n]
                assert item.tobytes() == x.plains[i] and dec(c) == x.plains[i] and x.sizes[i] == len(c), (x, i)
                if k == "PS" or x.split:
                    assert c == sg.expected_split(oracle, item, cg.SPLIT_LEN, x.ext)[0], (x, i)
                    assert walk_host(tsq, c)[1] == x.block_sizes[x.first_block[i]:x.first_block[i + 1]], (x, i)
                else:
                    assert c == oracle.compress(item, x.ext), (x, i)
            assert x.offsets == cg.plan_packed(x.sizes, cg.ALIGN) and x.out_size == x.offsets[-1]
        elif k == "SC":
            want, sizes = sg.expected_split(oracle, x.data, cg.SPLIT_LEN, x.ext)
            assert x.want.tobytes() == want and x.want_sizes == sizes and dec(want) == x.data.tobytes()
            assert walk_host(tsq, want) == (0, sizes, [min(cg.SPLIT_LEN, x.data.size - b * cg.SPLIT_LEN) for b in range(x.blocks)], x.data.size)
        elif k == "SD":
            if x.source is None:
                assert dec(x.blob) == x.plain.tobytes() and walk_host(tsq, x.blob)[1] == x.table and x.n == x.blob.size
            else:
                assert x.source.kind == "SC" and x.plain is x.source.data and x.n == x.source.want.size
        elif k == "XS":
            rc, sizes, _, total = walk_host(tsq, x.blob)
            assert rc == 0 and total == x.n_total and dec(x.blob) is not None
            assert (x.table != sizes and x.plain is None) if x.fail else (x.table == sizes and dec(x.blob) == x.plain.tobytes())
        elif k == "XP":
            for i in range(x.case.n):
                assert dec(x.case.container(i)) == x.case.datas[i], (x, i)
            assert x.e["item_status"] == [0] * x.case.n and x.e["item_first"][-1] == x.cap_blocks
        elif k == "J":
            if x.fail:
                assert x.container is None and x.out_cap == x.out_size - 1
            else:
                assert dec(x.container) == x.plain and walk_host(tsq, x.container)[:2] == (0, x.block_sizes) and len(x.container) == x.out_size
        elif k in ("K", "T"):
            for r in range(x.n_ranges):
                blob = x.e["containers"][r] if k == "K" else x.case.container(x.e, r)
                if blob is None:
                    assert x.fail and x.e["item_status"][r] == cg.ERR_ARG
                    continue
                rc, _, out_lens, total = walk_host(tsq, blob)
                assert rc == 0 and total == x.e["totals"][r] and dec(blob) == bytes(x.case.data(r)) and len(blob) == x.e["sizes"][r], (x, r)
            assert x.e["offsets"] == cg.plan_packed(x.e["sizes"], cg.ALIGN)
        elif k == "G":
            for r in range(x.n_ranges):
                start, ln = x.e["places"][r]
                if x.e["range_status"][r] != 0:
                    assert x.fail and ln == 0
                    continue
                if x.g_items is None:
                    plain = x.through.plain
                elif x.source is None:
                    plain = x.through.plains[x.g_items[r]]
                else:
                    plain = np.frombuffer(x.source.case.datas[x.g_items[r]], dtype=np.uint8)
                owed = np.frombuffer(x.case.index.data, dtype=np.uint8)[start:start + ln]
                assert ln == x.lengths[r] and np.array_equal(owed, plain[x.offsets[r]:x.offsets[r] + ln]), (x, r)
        seen[k] += 1
    assert all(n >= 8 for n in seen.values()), seen


def test_the_planners_agree_with_every_new_link(every_new_link, gen, tsq):
    counted = dict.fromkeys(NEW, 0)
    for x in every_new_link:
        k = x.kind
        if k == "DI":
            rng = np.random.default_rng(5)
            outs, cap = fenced(rng, x.lengths)
            first = tsq.plan_batch([(o, n, a, ln) for (o, n), a, ln in zip(x.spans, outs, x.lengths)], x.arena_size, cap, [1] * x.items)
            assert first[-1] == x.blocks
        elif k == "DD":
            got = tsq.plan_dense(x.batch.totals, x.batch.blocks, cg.ALIGN, x.out_size, x.cap_blocks)
            assert got == (x.out_offsets, x.first_block, x.items)
        elif k == "TC":
            plan = tsq.plan_compress_tables_split if x.split else tsq.plan_compress_tables
            args = (x.in_offsets, x.in_sizes, x.data.size) + ((cg.SPLIT_LEN,) if x.split else ()) + (cg.ALIGN, x.cap_blocks)
            assert plan(*args) == (x.first_block, [0 if s == 0 else s for s in x.item_status], x.bound, x.items)
        elif k == "PS":
            first, bound = tsq.plan_batch_split(x.spans, x.data.size, cg.SPLIT_LEN, cg.ALIGN)
            assert first == x.first_block and bound >= x.out_size
        elif k == "SC":
            nb, bound = tsq.plan_split(x.data.size, cg.SPLIT_LEN)
            assert nb == x.blocks and bound >= x.want.size >= 16 + 6 * nb
        elif k == "SD":
            assert tsq.plan_split(x.out_len, cg.SPLIT_LEN)[0] == x.blocks
        elif k == "XS":
            assert tsq.plan_split(x.n_total, cg.SPLIT_LEN)[0] == x.n_blocks
            starts = [min(b * cg.SPLIT_LEN, x.n_total) for b in range(x.n_blocks)] + [x.n_total]
            items = tsq.plan_ranges(starts, [(o, ln, 0) for o, ln in x.ranges[:1]], 1 << 20)
            assert len(items) == 2, "range 0 does not cross a block edge"
        elif k == "XP":
            e = x.e
            got = tsq.plan_index_packed(e["blocks"], e["totals"], e["head"], e["walk"], x.cap_blocks)
            assert got == (e["item_first"], e["item_at"], e["item_status"], e["words"], e["status"])
        elif k == "J":
            if x.source is None:
                blobs = [bytes(x.arena[o:o + n]) for o, n in zip(x.offsets, x.sizes)]
            else:
                blobs = gen.packed_output(x.source)[0]
            heads = [(int.from_bytes(b[4:8], "little"), int.from_bytes(b[8:16], "little")) for b in blobs]
            body_at, first, nb, total, size = tsq.plan_join([len(b) for b in blobs], [h[0] for h in heads], [h[1] for h in heads])
            assert first == x.first_block and size == x.out_size and nb == x.cap_blocks and total == len(x.plain)
        elif k == "K":
            s = x.case.source
            got = tsq.plan_cut(s.frame_at, s.out_start, x.ranges, cg.ALIGN, x.out_size)
            e = x.e
            assert got == (e["offsets"], e["sizes"], e["totals"], e["item_status"], e["n_fit"])
        elif k == "T":
            ix, e = x.case.index, x.e
            frame_at, out_start = ix.plan_tables()
            got = tsq.plan_cut_items(frame_at, out_start, ix.item_first, x.take_items, x.ranges, cg.ALIGN, x.out_size)
            assert got == (e["offsets"], e["sizes"], e["totals"], e["item_status"], e["n_fit"])
        elif k == "G":
            ix, e = x.case.index, x.e
            got = tsq.plan_gather(ix.out_start, ix.item_first, x.g_items, x.offsets, x.lengths, cg.ALIGN, x.out_cap, x.cap_pieces)
            assert got == (e["out_offsets"], e["range_status"], e["need_pieces"], len(e["groups"]))
        counted[k] += 1
    assert all(n >= 8 for n in counted.values()), counted


def test_walk2_holds_exactly_its_six_failing_links_and_no_link_reads_a_failed_source(gen):
    rules = set()
    for seed in (0, 1):
        chain = gen.walk2(seed)
        assert len(chain) == 40 and sorted((x.kind, x.fail) for x in chain if x.fail) == sorted(cg.FAILURES2)
        for x in chain:
            if x.fail:
                assert x.want_status == cg.FAILURES2[(x.kind, x.fail)] != 0 and x.source is None
        for k, x in enumerate(chain):
            before = lambda kinds: [y for y in chain[:k] if y.kind in kinds and not y.fail]
            if x.fail:
                continue
            wanted = {"PD": ("PC",), "F": ("E",), "SD": ("SC",), "DD": cg.PACKED_SOURCES, "J": cg.PACKED_SOURCES, "XP": cg.PACKED_SOURCES,
                      "G": ("XP",), "T": ("XP",)}.get(x.kind)
            if wanted and before(wanted):
                assert x.source is before(wanted)[-1] and not x.source.fail, (seed, k, x)
                rules.add((x.kind, x.source.kind))
            else:
                assert x.source is None, (seed, k, x)
        assert {x.shape for x in chain} == set(SHAPES)
    assert {a for a, _ in rules} == {"PD", "F", "SD", "DD", "J", "XP", "G", "T"}, rules
    assert {x.kind for seed in (0, 1) for x in gen.walk2(seed)} >= set(NEW)
    for chain in gen.pipelines():
        assert all(not x.fail for x in chain) and all(x.source is None or x.source in chain[:k] for k, x in enumerate(chain))
    assert {(x.kind, x.source.kind) for chain in gen.pipelines() for x in chain if x.source is not None} >= {
        ("SD", "SC"), ("DD", "PC"), ("DD", "PS"), ("DD", "TC"), ("DD", "T"), ("J", "PC"), ("J", "PS"), ("J", "TC"), ("J", "T"),
        ("XP", "PC"), ("XP", "PS"), ("XP", "TC"), ("XP", "T"), ("G", "XP"), ("T", "XP"), ("SD", "SC")}
