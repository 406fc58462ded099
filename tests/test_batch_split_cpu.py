"""CPU-only: batchsplitgen's batches reach what they aim at, shown with the oracle; its restatement of the two host planners
(tsqa_plan_batch_split, tsqa_plan_compress_tables_split) is held against them, refusals included; both bounds hold every expected arena;
and the new entry points are exported."""
import ctypes as C

import numpy as np
import pytest

import batchsplitgen as bg
import splitgen as sg
import tablegen as tg

import turbosqueeze_amd as tsq

BUDGET = bg.DEFAULT_BUDGET
NEW_NAMES = ("tsqa_plan_batch_split", "tsqa_compress_batch_packed_split_async", "tsqa_compress_batch_packed_split",
             "tsqa_plan_compress_tables_split", "tsqa_compress_batch_packed_tables_split_async")


def test_new_names_are_exported_and_declared():
    import os
    L = tsq.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "turbosqueeze_amd.h")).read()
    for name in NEW_NAMES:
        assert hasattr(L, name), name
        assert f" {name}(" in header, name


def plan_host(places, in_size, block_len, align):
    try:
        return tsq.plan_batch_split(places, in_size, block_len, align)
    except tsq.TsqError as e:
        assert e.code == bg.ERR_ARG
        return None


def test_plan_batch_split_is_restated():
    for b in bg.every_batch(BUDGET):
        if b.host_form:
            for align in bg.ALIGNS:
                assert plan_host(b.places, b.in_size, b.block_len, align) == bg.plan_batch_split(b.places, b.in_size, b.block_len, align), b.name
    places = [(0, 1), (1, 4097), (10, 2 * 4096 + 1), (0, 1 << 22), (5, (1 << 22) + 1)]
    for bl in sg.BLOCK_LENS:
        for align in bg.ALIGNS:
            got = plan_host(places, 1 << 23, bl, align)
            assert got == bg.plan_batch_split(places, 1 << 23, bl, align) and got is not None
            assert got[0][-1] == sum(-(-n // bl) for _, n in places)


def test_plan_batch_split_refusals():
    ok = [(0, 100), (100, 5000)]
    assert plan_host(ok, 5100, 4096, 16) is not None
    for bl in (0, 1, 2048, 4095, 4097, 3 << 12, 1 << 23, 1 << 31):
        assert plan_host(ok, 5100, bl, 16) is None and bg.plan_batch_split(ok, 5100, bl, 16) is None, bl
    for align in (0, 3, 8192):
        assert plan_host(ok, 5100, 4096, align) is None and bg.plan_batch_split(ok, 5100, 4096, align) is None
    for bad in ([], [(0, 0)], [(0, 100), (5001, 100)], [(0, 5101)], [((1 << 64) - 50, 100)]):
        assert plan_host(bad, 5100, 4096, 16) is None and bg.plan_batch_split(bad, 5100, 4096, 16) is None, bad
    # block counts that do not fit 32 bits: one item of 2^32 blocks, and two items that reach 2^32 together
    huge = 1 << 45
    for bad in ([(0, 1 << 44)], [(0, (1 << 44) - 4096), (0, 4097)]):
        assert plan_host(bad, huge, 4096, 16) is None and bg.plan_batch_split(bad, huge, 4096, 16) is None
    assert plan_host([(0, (1 << 44) - 4096)], huge, 4096, 16) == bg.plan_batch_split([(0, (1 << 44) - 4096)], huge, 4096, 16)
    L = tsq.lib()
    first, bound = (C.c_uint64 * 3)(), C.c_uint64(0)
    arr = tsq.api._batch_array([(0, 100, 0, 0), (100, 5000, 0, 0)])
    assert L.tsqa_plan_batch_split(arr, 2, 5100, 4096, 16, first, C.byref(bound)) == 0 and list(first) == [0, 1, 3]
    assert L.tsqa_plan_batch_split(None, 2, 5100, 4096, 16, first, C.byref(bound)) == bg.ERR_ARG
    assert L.tsqa_plan_batch_split(arr, 2, 5100, 4096, 16, None, C.byref(bound)) == bg.ERR_ARG
    assert L.tsqa_plan_batch_split(arr, 2, 5100, 4096, 16, first, None) == bg.ERR_ARG


def test_plan_compress_tables_split_is_restated():
    for b in bg.every_batch(BUDGET):
        for cap in sorted({0, 1, b.need_blocks - 1, b.need_blocks, b.need_blocks + 1} - {-1}):
            got = tsq.plan_compress_tables_split(b.in_offsets, b.in_sizes, b.in_size, b.block_len, b.align, cap)
            assert got == bg.layout(b.in_offsets, b.in_sizes, b.in_size, b.block_len, b.align, cap), (b.name, cap)
    b, cuts = bg.cap_cuts(BUDGET)
    for what, cap, n_fit in cuts:
        assert tsq.plan_compress_tables_split(b.in_offsets, b.in_sizes, b.in_size, b.block_len, b.align, cap)[3] == n_fit, what
    # an item of more than 2^32 - 1 blocks costs the item, not the call; the same size is fine in longer blocks
    at, sz = [0, 0, 7], [100, 1 << 44, 50]
    first, status, bound, n_fit = tsq.plan_compress_tables_split(at, sz, bg.IN_MAX, 4096, 16, 10)
    assert (first, status, n_fit) == ([0, 1, 1, 2], [0, bg.ERR_ARG, 0], 3) == bg.layout(at, sz, bg.IN_MAX, 4096, 16, 10)[:2] + (3,)
    assert bound == bg.layout(at, sz, bg.IN_MAX, 4096, 16, 10)[2]
    assert tsq.plan_compress_tables_split(at, sz, bg.IN_MAX, 8192, 16, 10)[1] == [0, bg.ERR_OVERFLOW, bg.ERR_OVERFLOW]
    for bl in (0, 2048, 4097, 1 << 23):
        with pytest.raises(tsq.TsqError) as e:
            tsq.plan_compress_tables_split(at, sz, bg.IN_MAX, bl, 16, 10)
        assert e.value.code == bg.ERR_ARG
    for kw in (dict(align=3), dict(in_size=bg.IN_MAX + 1)):
        with pytest.raises(tsq.TsqError):
            tsq.plan_compress_tables_split(at, sz, kw.get("in_size", bg.IN_MAX), 4096, kw.get("align", 16), 10)
    # with blocks of TSQ_BLOCK_SZ it is tsqa_plan_compress_tables
    b = bg.refusals(BUDGET)
    assert tsq.plan_compress_tables_split(b.in_offsets, b.in_sizes, b.in_size, 1 << 22, 16, 600) == \
        tsq.plan_compress_tables(b.in_offsets, b.in_sizes, b.in_size, 16, 600)


def walk(blob):
    """tsqa_walk_frames -> (rc, stream sizes, total)"""
    cap = int.from_bytes(blob[4:8], "little") + 1
    frame_at, sizes = (C.c_uint64 * cap)(), (C.c_uint32 * cap)()
    ext, out_len = (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    nb, total = C.c_uint32(0), C.c_uint64(0)
    buf = np.frombuffer(blob, dtype=np.uint8)
    rc = tsq.lib().tsqa_walk_frames(buf.ctypes.data, buf.size, cap, frame_at, sizes, ext, out_len, C.byref(nb), C.byref(total))
    return rc, list(sizes[:nb.value]), int(total.value)


def all_batches(oracle):
    return bg.every_batch(BUDGET) + [bg.crossing_fronted(oracle, BUDGET)[0]]


def test_every_expected_container_walks_decodes_and_fits_both_bounds(oracle):
    for b in all_batches(oracle):
        for ext in (0, 1):
            made = b.made(oracle, ext)
            for i, m in enumerate(made):
                if m is None:
                    continue
                blob, sizes = m
                rc, got, total = walk(blob)
                assert rc == 0 and got == sizes and total == b.in_sizes[i], (b.name, i)
                assert oracle.decompress(blob) == b.item(i).tobytes(), (b.name, i)
                assert len(blob) <= sg.plan_split(b.in_sizes[i], b.block_len)[1]
                assert max(sizes) <= sg.block_bound(b.block_len) - sg.WORD
            e = b.expect(oracle, ext)
            assert e["offsets"][-1] <= e["bound"], b.name
            assert e["bound"] == tsq.plan_compress_tables_split(b.in_offsets, b.in_sizes, b.in_size, b.block_len, b.align, 0)[2]
            if b.host_form:
                assert e["offsets"][-1] <= tsq.plan_batch_split(b.places, b.in_size, b.block_len, b.align)[1], b.name
                assert e["block_sizes"] == [s for m in made for s in m[1]] and len(e["block_sizes"]) == e["first_block"][-1]


def test_edge_items_and_item_counts():
    b = bg.edge_items()
    assert sorted(set(b.in_sizes)) == [1, 4095, 4096, 4097, 8193] and len(b.specs) == 15
    assert sorted(set(b.blocks)) == [1, 2, 3]
    assert [len(x.specs) for x in bg.item_counts()] == [1, 255, 256, 257, 513]
    assert all(set(x.blocks) == {1} for x in bg.item_counts())


def test_launch_ownership_falls_where_stated():
    B = BUDGET
    by_name = {b.name: b for b in bg.ownership(B)}
    assert bg.owners(by_name[f"alone_{B}"], B) == [{0}]
    assert bg.owners(by_name[f"alone_{B + 1}"], B) == [{0}, {0}]
    assert bg.owners(by_name[f"alone_{2 * B + 1}"], B) == [{0}, {0}, {0}]
    assert bg.owners(by_name[f"between_{B}"], B) == [{0, 1, 2}, {2, 3}]
    assert bg.owners(by_name[f"between_{B + 1}"], B) == [{0, 1, 2}, {2, 3}]
    # the middle launch of the long item holds that item alone, neither begun nor completed in it
    assert bg.owners(by_name[f"between_{2 * B + 1}"], B) == [{0, 1, 2}, {2}, {2, 3}]
    s = by_name["starts_on_last_block"]
    first = bg.layout(s.in_offsets, s.in_sizes, s.in_size, 4096, 16, s.need_blocks)[0]
    assert first[B - 1] == B - 1 and first[B] == B + 2 and s.blocks[B - 1] == 3
    e = by_name["ends_on_first_block"]
    first = bg.layout(e.in_offsets, e.in_sizes, e.in_size, 4096, 16, e.need_blocks)[0]
    assert first[B - 2] == B - 2 and first[B - 1] == B + 1 and e.blocks[B - 2] == 3          # (its last block is block B)
    r = bg.refusals(B)
    first, status, _, _ = bg.layout(r.in_offsets, r.in_sizes, r.in_size, 4096, 16, r.need_blocks)
    refused = [i for i, st in enumerate(status) if st == bg.ERR_ARG]
    assert refused[0] == 0 and 256 in refused and refused[-1] == len(r.specs) - 1
    k = next(i for i in range(len(r.specs)) if r.blocks[i] and first[i + 1] == B)          # the item that ends the first launch
    assert status[k + 1] == status[k + 2] == bg.ERR_ARG
    assert {s.kind for s in r.specs if isinstance(s, tg.Refused)} == set(tg.REFUSAL_KINDS)


@pytest.mark.parametrize("ext", [0, 1])
def test_crossings_are_where_they_are_claimed(oracle, ext):
    b = bg.crossing_alone()
    sizes = b.made(oracle, ext)[0][1]
    assert len(sizes) == 300 and min(sizes) > b.block_len and len(b.specs) == 1
    hits = bg.scan_crossings(sizes, BUDGET)
    assert len(hits) == 1 and 0 < hits[0][0] < bg.GROUP, "E[] passes 2^24 inside the first pass of one launch, inside one item"
    places = sg.frame_places(sizes)
    assert places[hits[0][0] - 1] < bg.SPLIT <= places[hits[0][0] + 1]


def test_fronted_crossing_falls_on_a_wavefronts_first_lane(oracle):
    b, (block, lane) = bg.crossing_fronted(oracle, BUDGET)
    table = b.expect(oracle, 1)["block_sizes"]
    assert bg.scan_crossings(table, BUDGET)[0] == (block, lane) and lane % bg.WAVE == 0
    assert block >= b.blocks[0], "the crossing lies inside the second item"
    assert len(b.specs) == 2 and lane != 0 and len(table) <= BUDGET, "inside a pass, inside one launch"


@pytest.mark.parametrize("ext", [0, 1])
def test_lookahead_case_tells_an_encoder_that_reads_past_the_item(oracle, ext):
    b, whole = bg.lookahead()
    cut = b.in_sizes[0]
    assert b.data[:whole.size].tobytes() == whole.tobytes() and b.in_offsets[1] == cut
    own = b.made(oracle, ext)[0][0]
    # the first item's container, had its last block's look-ahead seen the second item's bytes
    streams = sg.block_streams(oracle, whole, b.block_len, ext)[:b.blocks[0] - 1]
    last = whole[(b.blocks[0] - 1) * b.block_len:cut]
    streams.append(oracle.encode_block(last, ext, halo=whole[cut:cut + sg.HALO]))
    assert sg.container_of(streams, cut, ext) != own
    # and every block edge inside an item is crossed by a match: zero halos give another container
    assert sg.container_of(sg.block_streams(oracle, b.item(0), b.block_len, ext, zero_halo=True), cut, ext) != own


def test_align_mix_and_room_cuts(oracle):
    for align in bg.ALIGNS:
        b = bg.align_mix(align)
        assert len(b.specs) == 257 and max(b.blocks) >= 4 and b.align == align
        e = b.expect(oracle, 1)
        assert all(o % align == 0 for o in e["offsets"][:-1])
    assert bg.align_mix(4096).expect(oracle, 1)["offsets"][-1] > bg.align_mix(1).expect(oracle, 1)["offsets"][-1]
    for ext in (0, 1):
        b, cuts = bg.room_cuts(oracle, ext)
        full = b.expect(oracle, ext)
        used = full["offsets"][-1]
        for what, room in cuts:
            e = b.expect(oracle, ext, out_size=room, per_item=False)
            assert (e["offsets"], e["sizes"], e["block_sizes"]) == (full["offsets"], full["sizes"], full["block_sizes"]), what
            assert e["word"] == (bg.OK if room >= used else bg.ERR_OVERFLOW), what
            whole = [i for i in range(len(b.specs)) if e["writes"][i] == e["sizes"][i]]
            assert whole == [i for i in range(len(b.specs)) if e["offsets"][i] + e["sizes"][i] <= room], what
        mid = dict(cuts)["inside a middle item"]
        e = b.expect(oracle, ext, out_size=mid, per_item=True)
        assert 16 < e["writes"][bg.ROOM_MID] < e["sizes"][bg.ROOM_MID] and e["status"][bg.ROOM_MID] == bg.ERR_OVERFLOW
        assert dict(cuts)["inside a header"] - full["offsets"][bg.ROOM_MID] < 16
        e = b.expect(oracle, ext, out_size=dict(cuts)["inside a frame word"])
        assert e["writes"][bg.ROOM_MID] == tg.pieces(b.made(oracle, ext)[bg.ROOM_MID][0])[1]


def test_image_restates_the_fit_rule(oracle):
    b = bg.room_batch()
    e = b.expect(oracle, 1, out_size=10 ** 9)
    guard = np.full(e["offsets"][-1] + 100, 0xEE, dtype=np.uint8)
    img = b.image(oracle, 1, e, guard)
    for i, (o, z) in enumerate(zip(e["offsets"], e["sizes"])):
        assert img[o:o + z].tobytes() == b.made(oracle, 1)[i][0]
        assert (img[o + z:e["offsets"][i + 1]] == 0xEE).all()
    assert (img[e["offsets"][-1]:] == 0xEE).all()


def test_overlaps_and_caps(oracle):
    b = bg.overlaps()
    assert b.places[2] == b.places[1] and b.places[4] == (b.places[1][0], 4096 + 17) and b.places[5] == b.places[0]
    made = b.made(oracle, 1)
    assert made[2] == made[1] and made[4][0] != made[1][0][:len(made[4][0])]
    c, cuts = bg.cap_cuts(BUDGET)
    for what, cap, n_fit in cuts:
        e = c.expect(oracle, 1, cap_blocks=cap)
        assert e["n_fit"] == n_fit and len(e["block_sizes"]) == sum(c.blocks[:n_fit]) <= cap, what
        assert e["first_block"][-1] == c.need_blocks
