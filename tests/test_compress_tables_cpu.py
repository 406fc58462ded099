"""CPU side of the packed compress from device tables: tsqa_plan_compress_tables (host only) against the Python restatement of the
place rule, the block sum, the fitting prefix and the bound on every batch of tests/tablegen.py, and the facts that make each batch a
test of what it aims at -- which items cross a pass of the 256-lane scans or an encode launch's edge, where each refusal sits, where
each cut falls.  No kernel runs here; test_gpu_compress_tables.py runs the same batches on the device."""
import ctypes as C

import numpy as np
import pytest

import tablegen as tg

BUDGET = tg.DEFAULT_BUDGET


@pytest.fixture(scope="module")
def tsq():
    import turbosqueeze_amd
    return turbosqueeze_amd


def check_plan(tsq, b, cap_blocks):
    want = tg.layout(b.in_offsets, b.in_sizes, b.in_size, b.align, cap_blocks)
    at, sz = b.tables_u64()
    got = tsq.plan_compress_tables(at, sz, b.in_size, b.align, cap_blocks)
    assert got == want, f"{b.name}: tsqa_plan_compress_tables and the restatement differ (cap_blocks {cap_blocks})"
    return want


def test_plan_agrees_with_the_restatement_on_every_batch(tsq):
    for b in tg.every_batch(BUDGET):
        first, status, bound, n_fit = check_plan(tsq, b, b.need_blocks)
        assert first[-1] == b.need_blocks and n_fit == len(b.specs)
        assert status == [tg.OK if nb else tg.ERR_ARG for nb in b.blocks]
        assert bound == sum(tg.round_up(tsq.batch_bound(z), b.align) for z, nb in zip(b.in_sizes, b.blocks) if nb)
        # measuring: nothing fits, the first accepted item ends the prefix, and the tables do not depend on the room
        m = check_plan(tsq, b, 0)
        assert m[0] == first and m[2] == bound and m[3] == next(k for k, nb in enumerate(b.blocks) if nb)
        assert m[1] == [tg.ERR_OVERFLOW if nb else tg.ERR_ARG for nb in b.blocks]
    b, table = tg.cap_cuts(BUDGET)
    for what, cap_blocks, n_fit in table:
        assert check_plan(tsq, b, cap_blocks)[3] == n_fit, what


def test_batch_bound_restated(tsq):
    for n in (1, 2, 100, 4096, tg.BLOCK - 1, tg.BLOCK, tg.BLOCK + 1, 2 * tg.BLOCK + 1, 3 * tg.BLOCK):
        assert tg.batch_bound(n) == tsq.batch_bound(n) == tsq.lib().tsqa_batch_bound(n)


def test_plan_refuses_bad_arguments(tsq):
    L = tsq.lib()
    at, sz = (C.c_uint64 * 2)(0, 5), (C.c_uint64 * 2)(5, 6)
    first, status, bound, n_fit = (C.c_uint64 * 3)(7, 7, 7), (C.c_int32 * 2)(7, 7), C.c_uint64(7), C.c_uint32(7)
    call = lambda **kw: L.tsqa_plan_compress_tables(kw.get("at", at), kw.get("sz", sz), kw.get("n", 2), kw.get("in_size", 11), kw.get("align", 16),
                                                    2, kw.get("first", first), kw.get("status", status), kw.get("bound", C.byref(bound)),
                                                    kw.get("fit", C.byref(n_fit)))
    for bad in (dict(at=None), dict(sz=None), dict(first=None), dict(status=None), dict(bound=None), dict(fit=None), dict(n=0), dict(align=0),
                dict(align=24), dict(align=8192), dict(in_size=(1 << 48) + 1)):
        assert call(**bad) == tg.ERR_ARG, bad
    assert list(first) == [7, 7, 7] and list(status) == [7, 7] and bound.value == 7 and n_fit.value == 7
    assert call() == 0 and list(first) == [0, 1, 2] and list(status) == [0, 0] and n_fit.value == 2
    assert bound.value == tg.round_up(tg.batch_bound(5), 16) + tg.round_up(tg.batch_bound(6), 16)
    assert call(in_size=1 << 48) == 0


def test_a_refused_item_adds_nothing_whatever_its_size(tsq):
    got = tsq.plan_compress_tables([0, 0, 4], [4, 1 << 60, 2 * tg.BLOCK + 1], 3 * tg.BLOCK, 16, 4)
    assert got == ([0, 1, 1, 4], [0, tg.ERR_ARG, 0], tg.round_up(tg.batch_bound(4), 16) + tg.round_up(tg.batch_bound(2 * tg.BLOCK + 1), 16), 3)
    # one block short: the three-block item is unfit as a whole
    assert tsq.plan_compress_tables([0, 0, 4], [4, 1 << 60, 2 * tg.BLOCK + 1], 3 * tg.BLOCK, 16, 3)[1:] == ([0, tg.ERR_ARG, tg.ERR_OVERFLOW], got[2], 2)


def test_expected_offsets_are_plan_packed_of_the_expected_sizes(tsq):
    for b in [tg.loop_edges()[3], tg.refusals(BUDGET), tg.refused_run(), tg.overlaps(), tg.lying()] + [tg.alignment(a) for a in tg.ALIGNS]:
        for ext in tg.EXTS:
            e = b.expect(ext, b.need_blocks, 1 << 40)
            assert tsq.plan_packed(e["sizes"], b.align) == e["offsets"], b.name
            assert e["offsets"][-1] <= e["bound"], f"{b.name}: the bound does not hold the arena"
    b, table = tg.cap_cuts(BUDGET)
    for what, cap_blocks, _ in table:
        e = b.expect(1, cap_blocks, 1 << 40)
        assert tsq.plan_packed(e["sizes"], b.align) == e["offsets"], what


def test_loop_edges_cross_the_scan_passes():
    assert [len(b.specs) for b in tg.loop_edges()] == list(tg.LOOP_COUNTS) == [1, 255, 256, 257, 513]
    for b in tg.loop_edges():
        n = len(b.specs)
        assert all(1 <= z <= 4096 for z in b.in_sizes) and b.blocks == [1] * n
        first, _, bound, _ = tg.layout(b.in_offsets, b.in_sizes, b.in_size, b.align, n)
        e = b.expect(1, n, 1 << 40)
        for edge in (tg.GROUP, 2 * tg.GROUP):
            if n > edge:                                     # both sums of the layout scan and the offsets of the pack scan carry into the pass
                assert first[edge] == edge and e["offsets"][edge] > 0
    # the 257 items are one launch: the pack scan's window holds every one of them, in two passes
    assert all(set(r) == {0} for r in tg.launches_of(tg.loop_edges()[3], BUDGET))


def test_launch_edges_fall_where_they_aim():
    by = {b.name: b for b in tg.launch_edges(BUDGET)}
    assert tg.launch_counts(BUDGET) == (BUDGET - 1, BUDGET, BUDGET + 1, 2 * BUDGET + 1)
    for n, launches in zip(tg.launch_counts(BUDGET), (1, 1, 2, 3)):
        b = by[f"launch_edges_{n}"]
        assert b.blocks == [1] * n and -(-b.need_blocks // BUDGET) == launches
        where = tg.launches_of(b, BUDGET)
        assert [list(r) for r in where] == [[k // BUDGET] for k in range(n)]
    b = by["launch_straddle"]
    where = tg.launches_of(b, BUDGET)
    assert b.in_sizes[BUDGET - 1] == tg.BLOCK + 1 and b.blocks[BUDGET - 1] == 2 and list(where[BUDGET - 1]) == [0, 1], "the item's blocks are not one in each launch"
    assert all(list(r) == [1] for r in where[BUDGET:]) and len(where) == BUDGET + 3
    b = by["three_blocks_first"]
    assert b.in_sizes[0] == 2 * tg.BLOCK + 1 and b.blocks[0] == 3
    assert tg.layout(b.in_offsets, b.in_sizes, b.in_size, 16, 99)[0] == [0, 3, 4, 5, 6, 7]
    assert len(tg.pieces(b.containers(1)[0])) == 4            # a header and three frames


def test_refusals_sit_where_they_aim():
    b = tg.refusals(BUDGET)
    n = len(b.specs)
    kinds = {k: s.kind for k, s in enumerate(b.specs) if isinstance(s, tg.Refused)}
    assert sorted(kinds.values()) == sorted(tg.REFUSAL_KINDS)
    assert 0 in kinds and n - 1 in kinds
    where = tg.launches_of(b, BUDGET)
    assert list(where[BUDGET]) == [0] and list(where[BUDGET + 3]) == [1], "item BUDGET does not end the first launch"
    assert BUDGET + 1 in kinds and BUDGET + 2 in kinds, "no refused item directly behind the item that ends a launch"
    at, sz, size = b.in_offsets, b.in_sizes, b.in_size
    for k, kind in kinds.items():
        assert b.blocks[k] == 0, kind
        if kind == "size_0":
            assert sz[k] == 0 and at[k] < size
        elif kind == "size_in_size_plus_1":
            assert sz[k] == size + 1
        elif kind == "offset_one_past":
            assert sz[k] <= size and at[k] == size - sz[k] + 1
        elif kind == "wraps":
            assert at[k] + sz[k] >= tg.U64 and (at[k] + sz[k]) % tg.U64 <= size, "a wrapped sum would not look like a place inside the input"
        else:
            assert sz[k] == 1 << 63
    e = b.expect(1, b.need_blocks, 1 << 40)
    assert [st for st in e["status"] if st] == [tg.ERR_ARG] * 5 and all(e["sizes"][k] == 0 and e["offsets"][k + 1] == e["offsets"][k] for k in kinds)
    r = tg.refused_run()
    run = [k for k, nb in enumerate(r.blocks) if nb == 0]
    assert run == list(range(3, 303)) and len(run) > tg.GROUP and len(r.specs) == 306
    assert {s.kind for s in r.specs[3:303]} == set(tg.REFUSAL_KINDS)


def test_a_batch_of_refused_items_only_owes_empty_tables(tsq):
    b = tg.all_refused()
    assert b.blocks == [0] * 5 and b.in_size > 100
    assert tsq.plan_compress_tables(*b.tables_u64(), b.in_size, 16, 3) == ([0] * 6, [tg.ERR_ARG] * 5, 0, 5)
    e = b.expect(1, 3, 64)
    assert e["offsets"] == [0] * 6 and e["sizes"] == [0] * 5 and e["writes"] == [0] * 5


def test_cap_cuts_fall_where_they_aim():
    b, table = tg.cap_cuts(BUDGET)
    k = tg.CUT_BIG_AT
    assert b.blocks[k] == 2 and b.need_blocks == 11 and len(b.specs) == 10
    assert [(cap, fit) for _, cap, fit in table] == [(11, 10), (10, 9), (k + 1, k), (1, 1), (11 + 2 * BUDGET + 1, 10)]
    for what, cap_blocks, n_fit in table:
        e = b.expect(1, cap_blocks, 1 << 40)
        assert e["status"] == [0 if i < n_fit else tg.ERR_OVERFLOW for i in range(10)], what
        assert e["first_block"][-1] == 11, "first_block does not depend on the room"
        assert [z > 0 for z in e["sizes"]] == [i < n_fit for i in range(10)], what
    first = b.expect(1, k + 1, 1 << 40)["first_block"]
    assert first[k] + 1 == k + 1 < first[k + 1] and first[k] + 1 + b.blocks[k + 1] <= k + 1 + 1     # item 6 alone would have fit behind item 4
    assert -(-table[4][1] // BUDGET) - -(-11 // BUDGET) == 2 and table[4][1] % BUDGET not in (0, 11)


@pytest.mark.parametrize("ext", tg.EXTS)
def test_arena_cuts_fall_where_they_aim(ext):
    b, table = tg.arena_cuts(ext)
    k = tg.CUT_BIG_AT
    full = b.expect(ext, b.need_blocks, 1 << 40)
    used, at, size = full["offsets"][-1], full["offsets"][k], full["sizes"][k]
    ends = tg.pieces(b.containers(ext)[k])
    assert len(ends) == 3 and ends[2] == size
    want_writes = {"used": size, "used - 1": size, "the end of item 5's header": 16, "the middle of item 5's first frame": 16,
                   "the end of item 5's first frame": ends[1], "a header and no more": 0}
    for what, out_size in table:
        e = b.expect(ext, b.need_blocks, out_size)
        assert e["offsets"] == full["offsets"] and e["sizes"] == full["sizes"], "sizes and places do not depend on the room"
        assert e["status"] == [0 if o + z <= out_size else tg.ERR_OVERFLOW for o, z in zip(full["offsets"], full["sizes"])], what
        assert e["writes"][k] == want_writes[what], what
        assert all(w == 0 or o + w <= out_size for o, w in zip(e["offsets"], e["writes"])), what
    assert b.expect(ext, b.need_blocks, used)["status"] == [0] * 10
    last = b.expect(ext, b.need_blocks, used - 1)
    assert last["status"] == [0] * 9 + [tg.ERR_OVERFLOW] and last["writes"][9] == 16
    tiny = b.expect(ext, b.need_blocks, 16)
    assert tiny["writes"] == [16] + [0] * 9 and tiny["status"] == [tg.ERR_OVERFLOW] * 10


@pytest.mark.parametrize("align", tg.ALIGNS)
def test_alignment_container_sizes_sit_around_a_multiple(align):
    b = tg.alignment(align)
    for ext in tg.EXTS:
        e = b.expect(ext, b.need_blocks, 1 << 40)
        aimed = e["sizes"][6 * ext:6 * ext + 6:2]
        assert [z % align for z in aimed] == ([0] * 3 if align == 1 else [align - 1, 0, 1]), (ext, aimed)
        assert all(o % align == 0 for o in e["offsets"][:-1])
        if align > 1:
            assert any(e["offsets"][i + 1] - e["offsets"][i] > e["sizes"][i] for i in range(len(b.specs) - 1)), "no padding anywhere"


def test_overlapping_items_are_whole_items():
    b = tg.overlaps()
    assert (b.in_offsets[2], b.in_sizes[2]) == (b.in_offsets[1], b.in_sizes[1]) and b.in_offsets[5] == 0
    assert b.in_offsets[4] == b.in_offsets[3] and b.in_sizes[4] == 17 < b.in_sizes[3]
    blobs = b.containers(1)
    assert blobs[2] == blobs[1] and blobs[4] == tg.container(b.item_bytes(3)[:17], 1) and b.blocks == [1] * 6


def test_lying_sizes_would_wrap_a_32_bit_block_sum():
    b = tg.lying()
    lies = [k for k, s in enumerate(b.specs) if isinstance(s, tg.Lie)]
    unclamped = sum(-(-b.in_sizes[k] // tg.BLOCK) for k in range(len(b.specs)))
    assert unclamped > 1 << 32 and any((-(-b.in_sizes[k] // tg.BLOCK)) % (1 << 32) == 0 for k in lies), "no size whose blocks are 0 mod 2^32"
    cap = b.need_blocks
    assert cap == 4 and unclamped > cap
    first, status, bound, n_fit = tg.layout(b.in_offsets, b.in_sizes, b.in_size, 16, cap)
    assert [status[k] for k in lies] == [tg.ERR_ARG] * 5 and [st for k, st in enumerate(status) if k not in lies] == [0] * 4
    assert first == [0, 1, 1, 2, 2, 2, 3, 3, 3, 4] and n_fit == len(b.specs)
    assert bound == sum(tg.round_up(tg.batch_bound(z), 16) for k, z in enumerate(b.in_sizes) if k not in lies) < 1 << 20


def test_containers_are_the_oracles_and_round_trip(oracle):
    for b in (tg.overlaps(), tg.cuts_batch()):
        for ext in tg.EXTS:
            for i, blob in enumerate(b.containers(ext)):
                assert oracle.decompress(blob) == b.item_bytes(i)
