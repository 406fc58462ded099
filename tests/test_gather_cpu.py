"""CPU-only: gathergen's restatements against the host-only planners (tsqa_plan_gather, tsqa_plan_item_ranges), the host frame walk
(tsqa_walk_frames) and the oracle, and that each of its cases reaches what it aims at.  The kernels' side of the same cases:
test_gpu_gather.py."""
import ctypes as C

import numpy as np
import pytest

import cutgen as cg
import gathergen as gg
import turbosqueeze_amd as tsq
from test_cut_cpu import host_walk

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = gg.OK, gg.ERR_ARG, gg.ERR_FORMAT, gg.ERR_OVERFLOW


def library_plan(case, out_cap=None, cap_pieces=None):
    """tsqa_plan_gather on a case's index tables -> (out_offsets, range_status, need_pieces, n_groups)"""
    i = case.index
    return tsq.plan_gather(i.out_start, i.item_first, case.items, case.offsets, case.lengths, case.align, out_cap, cap_pieces)


def restated(e):
    return e["out_offsets"], e["range_status"], e["need_pieces"], len(e["groups"])


def all_cases():
    return (gg.healthy_cases() + [gg.refusal(name, at) for name, at in gg.refusal_cases()])


def test_the_symbols_are_there():
    for name in ("tsqa_plan_gather", "tsqa_gather_async", "tsqa_gather", "tsqa_profile_read_gather"):
        assert hasattr(tsq.lib(), name), name


def test_the_sort_adds_no_shared_library():
    """rocPRIM is header-only: the library names no rocPRIM file among the ones it needs"""
    with open(tsq.lib_path(), "rb") as f:
        blob = f.read()
    assert b"librocprim" not in blob and b"librocthrust" not in blob and b"libhipcub" not in blob


def test_the_batch_is_what_the_restatement_says(oracle):
    b = gg.batch()
    assert b.n_items == gg.BATCH_ITEMS and len(b.spans) == gg.BATCH_ITEMS
    refused = [i for i in range(b.n_items) if b.item_first[i] == b.item_first[i + 1]]
    assert refused == sorted(gg.BATCH_DAMAGE), "the refused items are not the damaged ones"
    blocks = [b.item_first[i + 1] - b.item_first[i] for i in range(b.n_items)]
    assert set(blocks) == {0, 1, 3} and blocks.count(3) >= 40
    at = 0
    for i, (o, n) in enumerate(b.spans):
        blob = b.blob[o:o + n]
        assert o % 16 == 0
        rc, nb, total, _, _, out_len = host_walk(blob)
        if i in gg.BATCH_DAMAGE:
            assert rc != 0, f"the host walk accepts damaged item {i} ({gg.BATCH_DAMAGE[i]})"
            continue
        assert rc == 0 and nb == blocks[i] and [int(x) for x in np.cumsum([0] + out_len)] == [s - at for s in b.out_start[b.item_first[i]:b.item_first[i] + nb]] + [total]
        assert bytes(oracle.decompress(blob)) == b.data[at:at + total], i
        at += total
    assert at == b.total
    # the walk-refused items state blocks in a header that passes: the index has to close the gap they leave in its table
    for i in (101, 256):
        blob = b.blob[b.spans[i][0]:b.spans[i][0] + b.spans[i][1]]
        assert blob[:4] == b"TSQ1" and int.from_bytes(blob[4:8], "little") >= 1


def test_plan_gather_is_restated():
    for case in all_cases():
        e = case.expect()
        assert library_plan(case) == restated(e), case.name
        mid = e["out_offsets"][case.n // 2] + 1
        for out_cap, cap_pieces in ((e["need"], e["need_pieces"]), (max(e["need"] - 1, 0), None), (mid, None), (None, max(e["need_pieces"] - 1, 1)),
                                    (None, 1), (0, None)):
            want = case.expect(gg.NO_LIMIT_BYTES if out_cap is None else out_cap, gg.NO_LIMIT_PIECES if cap_pieces is None else cap_pieces)
            assert library_plan(case, out_cap, cap_pieces) == restated(want), (case.name, out_cap, cap_pieces)
    for what, case, out_cap, cap_pieces in gg.rooms():
        assert library_plan(case, out_cap, cap_pieces) == restated(case.expect(out_cap, cap_pieces)), what


def test_the_places_follow_plan_packed():
    for case in gg.healthy_cases():
        e = case.expect()
        sizes = [ln if st == OK else 0 for ln, st in zip(case.lengths, e["range_status"])]
        assert e["out_offsets"] == tsq.plan_packed(sizes, case.align), case.name
        assert all(o % case.align == 0 for o in e["out_offsets"][:-1]), case.name


def test_the_pieces_and_groups_are_the_host_plan_s():
    """what the device's stable sort must reproduce: for every accepted and fitting set of ranges, the restated pieces and groups
    are tsqa_plan_item_ranges' on the same ranges with out_at from the layout"""
    rooms = [(c, gg.NO_LIMIT_BYTES, gg.NO_LIMIT_PIECES) for c in all_cases()] + [(c, oc, cp) for _, c, oc, cp in gg.rooms()]
    for case, out_cap, cap_pieces in rooms:
        e = case.expect(out_cap, cap_pieces)
        i = case.index
        first = i.item_first if case.items is not None else [0, i.n_blocks]
        items, groups = tsq.plan_item_ranges(i.out_start, first, case.item_ranges(e), max(e["need"], 1))
        assert items == e["items"], (case.name, out_cap, cap_pieces)
        assert groups == e["groups"], (case.name, out_cap, cap_pieces)
        assert len(items) == e["fit_pieces"] <= e["need_pieces"]
        keys = [(b << gg.KEY_LO_BITS) | lo for b, lo, _, _ in items]
        assert keys == sorted(keys) and all(lo < 1 << gg.KEY_LO_BITS for _, lo, _, _ in items), case.name


def test_counts_reach_bisection_many_pieces_and_empty_ranges():
    for case in gg.counts():
        e = case.expect()
        assert e["status"] == OK
    c = gg.counts()[-1]
    per_range = [len(gg.cut(c.index.out_start, o, ln)) for o, ln in zip(c.offsets, c.lengths)]
    assert max(per_range) >= 8 and per_range.count(0) == c.lengths.count(0) >= 20
    assert [k.n for k in gg.counts()] == list(gg.COUNTS)
    firsts = {gg.block_of(c.index.out_start, o) for o, ln in zip(c.offsets, c.lengths) if ln}
    assert len(firsts) > 250 and min(firsts) < 5 and max(firsts) > 590, "the bisection is not asked all over the table"


def test_alignment_leaves_padding():
    outs = {a: gg.aligned(a).expect() for a in gg.ALIGNS}
    assert outs[1]["need"] == sum(gg.aligned(1).lengths)
    assert outs[16]["need"] > outs[1]["need"] and outs[4096]["need"] > 200 * 4096
    assert outs[1]["items"] != outs[16]["items"] and [i[:3] for i in outs[1]["items"]] == [i[:3] for i in outs[16]["items"]]


def test_the_shift_and_the_bisection_see_the_same_blocks():
    sized, plain = gg.shift_and_bisect()
    assert sized.index.kind == "sized" and plain.index.kind == "plain" and sized.index.blob == plain.index.blob
    starts = sized.index.out_start
    assert starts[:-1] == [b * 4096 for b in range(257)], "the descriptors' out_at are not b << 12"
    for o, ln in zip(sized.offsets, sized.lengths):
        assert gg.block_of(starts, o) == o >> 12 and gg.block_of(starts, o + ln - 1) == (o + ln - 1) >> 12
    assert sized.expect() == plain.expect()
    per_range = [len(gg.cut(starts, o, ln)) for o, ln in zip(sized.offsets, sized.lengths)]
    assert {1, 2, 3} <= set(per_range)


def test_the_places_pass_2_to_the_24_where_claimed():
    for case in gg.carries():
        k = gg.crossing(case)
        assert k == gg.CARRY_CROSSINGS[case.name], (case.name, k)
        assert case.expect()["out_offsets"][k] == gg.SPLIT, "the crossing is not exact"
    assert gg.CARRY_CROSSINGS["carry_between_passes"] == gg.GROUP
    assert gg.CARRY_CROSSINGS["carry_inside_a_wavefront"] % gg.WAVE == 57 and gg.CARRY_CROSSINGS["carry_inside_a_wavefront"] // gg.WAVE == 3
    assert gg.CARRY_CROSSINGS["carry_at_a_wavefront_edge"] == 3 * gg.WAVE


def test_one_range_over_everything_has_a_piece_per_block():
    e = gg.whole().expect()
    assert e["need_pieces"] == gg.tiny().n_blocks == len(e["groups"]) == 600 and e["need"] == gg.tiny().total


def test_one_block_groups_have_the_stated_sizes():
    for n in gg.ONE_BLOCK_COUNTS:
        case = gg.one_block(n)
        e = case.expect()
        assert len(e["groups"]) == 1 and e["groups"][0][:3] == (gg.ONE_BLOCK, 0, n), n
        assert e["groups"][0][3] == max(hi for _, _, hi, _ in e["items"])
    assert [n for n in gg.ONE_BLOCK_COUNTS if n > gg.FLUSH] == [65, 129, 1000] and gg.FLUSH in gg.ONE_BLOCK_COUNTS
    c = gg.one_block(1000)
    e = c.expect()
    assert (c.offsets[1], c.lengths[1]) == (c.offsets[0], c.lengths[0]), "the same range twice"
    assert c.offsets[2] == c.offsets[0] == c.offsets[3] and len({c.lengths[0], c.lengths[2], c.lengths[3]}) == 3
    lo0 = c.offsets[0] - gg.ONE_BLOCK * gg.UNIT
    same = [it for it in e["items"] if it[1] == lo0]
    assert len(same) >= 4
    # equal keys keep range order: their places in the output ascend as the ranges' numbers do
    assert [it[3] for it in same[:4]] == [e["out_offsets"][k] for k in range(4)]
    # the largest hi of the group is not its last item's: the group's hi has to be a maximum, not the last
    assert max(it[2] for it in e["items"]) >= e["items"][-1][2]


def test_the_shuffle_is_unsorted_and_overlapping():
    c = gg.shuffled()
    e = c.expect()
    assert c.n == 1000 and len(e["groups"]) == 600
    assert sum(a > b for a, b in zip(c.offsets, c.offsets[1:])) > 400
    spans = sorted(zip(c.offsets, c.lengths))
    assert sum(a + ln > b for (a, ln), (b, _) in zip(spans, spans[1:])) > 100, "the ranges do not overlap in the source"
    cut_order = [it for k in range(c.n) for it in [(b, lo) for b, lo, _, _ in gg.cut(c.index.out_start, c.offsets[k], c.lengths[k])]]
    assert cut_order != sorted(cut_order)


def test_the_batch_cases_reach_items_edges_and_refused_items():
    c = gg.batch_items()
    e = c.expect()
    assert e["status"] == ERR_ARG
    bad = [k for k, st in enumerate(e["range_status"]) if st != OK]
    # a range of a refused item is refused whatever it asks for, nothing included
    assert {c.items[k] for k in bad} == set(gg.BATCH_DAMAGE) and len(bad) == 2 * len(gg.BATCH_DAMAGE)
    assert {c.lengths[k] for k in bad} == {0, 1} and {c.items[k] for k in bad if c.lengths[k]} == set(gg.BATCH_REFUSED_PROBE)
    i = c.index
    three = [k for k in range(c.n) if i.item_first[c.items[k] + 1] - i.item_first[c.items[k]] == 3]
    assert any(len(gg.cut(i.out_start, i.item_span(c.items[k])[0] + c.offsets[k], c.lengths[k])) >= 2 for k in three)
    f = gg.batch_flat().expect()
    assert f["status"] == OK and f["need_pieces"] > gg.batch_flat().n


def test_every_refusal_is_refused_for_its_reason():
    i = gg.batch()
    base, total = i.item_span(gg.REFUSAL_ITEM)
    assert total > 1 and i.n_items == gg.BATCH_ITEMS
    for name, at in gg.refusal_cases():
        c = gg.refusal(name, at)
        e = c.expect()
        item, off, ln = c.items[at], c.offsets[at], c.lengths[at]
        assert e["range_status"][at] == ERR_ARG and e["places"][at][1] == 0, (name, at)
        if name == "offset_at_total_length_1":
            assert (item, off, ln) == (gg.REFUSAL_ITEM, total, 1) and gg.range_rule(i, item, off - 1, 1)[0] == OK
        elif name == "length_all_ones":
            assert ln == gg.ALL_ONES and (off + ln) % (1 << 64) <= total, "offset + length does not wrap into the item"
        elif name == "offset_all_ones":
            assert off == gg.ALL_ONES and (off + ln) % (1 << 64) <= total
        elif name == "item_is_items":
            assert item == i.n_items and gg.range_rule(i, item - 2, 0, 1)[0] == OK
        else:
            assert item == (1 << 32) - 1
        # the others keep their places: a refused range takes no room
        clean = gg.Case("clean", i, c.offsets[:at] + c.offsets[at + 1:], c.lengths[:at] + c.lengths[at + 1:], items=c.items[:at] + c.items[at + 1:], align=16).expect()
        # (tsqa_plan_packed rounds every place but the end: behind a refused LAST range the end is the rounded one)
        got = e["out_offsets"][:at] + e["out_offsets"][at + 1:]
        assert got[:-1] == clean["out_offsets"][:-1] and got[-1] == (gg.round_up(clean["need"], 16) if at == c.n - 1 else clean["need"]), (name, at)
    assert gg.REFUSAL_AT == (0, gg.GROUP, 299)


def test_the_unfit_ranges_are_a_suffix_of_the_accepted_ones():
    seen = set()
    for what, case, out_cap, cap_pieces in gg.rooms():
        e = case.expect(out_cap, cap_pieces)
        st = [s for s in e["range_status"] if s != ERR_ARG]
        first = st.index(ERR_OVERFLOW) if ERR_OVERFLOW in st else len(st)
        assert st == [OK] * first + [ERR_OVERFLOW] * (len(st) - first), what
        assert e["need"] == case.expect()["need"] and e["need_pieces"] == case.expect()["need_pieces"], "the sums are not complete whatever fits"
        assert e["out_offsets"] == case.expect()["out_offsets"]
        seen.add(first)
        if what == "exactly the room needed":
            assert first == len(st) and e["status"] == OK
        elif what in ("one byte short of the last range", "one piece short"):
            last = max(k for k in range(case.n) if case.lengths[k])
            assert e["range_status"][last] == ERR_OVERFLOW and e["range_status"][:last].count(ERR_OVERFLOW) == 0
        elif what == "one piece":
            k = next(k for k in range(case.n) if case.lengths[k])
            assert e["fit_pieces"] <= 1 and e["range_status"][k] == (OK if len(gg.cut(case.index.out_start, case.offsets[k], case.lengths[k])) == 1 else ERR_OVERFLOW)
        else:
            assert 100 < first < len(st), (what, first)
    assert len(seen) >= 4


def test_a_refused_index_refuses_every_range():
    c = gg.refused_case()
    e = c.expect()
    assert e["range_status"] == [ERR_FORMAT] * c.n and e["status"] == ERR_FORMAT and e["need"] == 0 and e["need_pieces"] == 0 and not e["items"]
    blob, table, n_total, block_len, _ = cg.refused_index()
    rc, nb, total, _, sizes, _ = host_walk(blob)
    assert rc == 0 and total == n_total and sizes != list(table), "the container is valid; only the table is false"


def test_the_big_case_has_block_numbers_of_17_bits():
    c = gg.big_case()
    e = c.expect()
    assert c.index.n_blocks == gg.BIG_BLOCKS == (1 << 16) + 1 and c.index.total == (1 << 28) + 1
    blocks = {b for b, _, _, _ in e["items"]}
    assert {65534, 65535, 65536} <= blocks and e["status"] == OK and c.n == 46
    assert e["items"][-1][:3] == (65536, 0, 1)


def test_the_size_limits():
    """n_ranges * (total + 4096) and n_ranges * n_blocks stay below 2^55: what keeps the layout's sums inside group_scan_excl64"""
    L = tsq.lib()
    nb = 8192
    starts = (np.arange(nb + 1, dtype=np.uint64) << np.uint64(22))
    first = np.array([0, nb], dtype=np.uint64)

    def call(n):
        zeros = np.zeros(n, dtype=np.uint64)
        offs, st = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        pieces, groups = C.c_uint64(0), C.c_uint32(0)
        return L.tsqa_plan_gather(starts.ctypes.data, nb, first.ctypes.data, 1, None, zeros.ctypes.data, zeros.ctypes.data, n, 1, 0, 1,
                                  offs.ctypes.data, st.ctypes.data, C.byref(pieces), C.byref(groups))

    assert int(starts[-1]) == 1 << 35
    assert call((1 << 20) - 1) == OK, "2^55 - 2^35 + 2^32 - 4096 is below the bound"
    assert call(1 << 20) == ERR_ARG, "2^20 ranges of 2^35 + 4096 bytes reach 2^55"


def test_bad_arguments_are_refused():
    c = gg.counts()[1]
    i = c.index
    for kw in (dict(align=0), dict(align=3), dict(align=8192), dict(cap_pieces=0)):
        with pytest.raises(tsq.TsqError) as err:
            tsq.plan_gather(i.out_start, i.item_first, None, c.offsets, c.lengths, **{"align": 1, **kw})
        assert err.value.code == ERR_ARG, kw
    with pytest.raises(tsq.TsqError):
        tsq.plan_gather([1] + i.out_start[1:], i.item_first, None, c.offsets, c.lengths)
    with pytest.raises(tsq.TsqError):
        tsq.plan_gather(i.out_start, [0, i.n_blocks - 1], None, c.offsets, c.lengths)
    # d_items with an index of one item is allowed: only item 0 exists
    assert tsq.plan_gather(i.out_start, i.item_first, [0, 1], c.offsets, c.lengths)[1] == [OK, ERR_ARG]
    assert tsq.plan_gather(i.out_start, i.item_first, None, [], []) == ([0], [], 0, 0)
