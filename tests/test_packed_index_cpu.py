"""CPU-only: packedindexgen's restatement of the index of a packed batch made from its device tables against the oracle,
tsqa_walk_frames and the host-only planner tsqa_plan_index_packed, that each of its cases reaches what it aims at, and the new
names.  The kernels' side: test_gpu_packed_index.py.

Which tests guard what.  The FEATURE (they fail where the new symbols are missing): test_the_new_names_are_declared_and_exported,
test_the_planner_refuses_what_it_says and test_the_planner_equals_the_restatement, which hold tsqa_plan_index_packed -- the fit and
the close-up that the kernels must reproduce -- against the restatement for every case and room.  The CASES (they use the
generator and library calls there were before, and pass without the feature; they show that the GPU file's inputs are what their
names say): every other test here -- the plain walk against tsqa_walk_frames and the oracle, the tables against
tsqa_plan_item_ranges, and the reach tests of the counts, the 2^24 crossings, the refusals' kinds and places, the caps and the
false tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import packedindexgen as pg
import turbosqueeze_amd as tsq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = pg.OK, pg.ERR_ARG, pg.ERR_FORMAT, pg.ERR_OVERFLOW


def lib_walk(blob):
    """tsqa_walk_frames -> (rc, out_lens)"""
    L = tsq.lib()
    cap = 1 << 12
    frame_at, sizes, ext, out_len = (C.c_uint64 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    nb, total = C.c_uint32(0), C.c_uint64(0)
    raw = np.frombuffer(bytes(blob) + b"\0", dtype=np.uint8)
    rc = L.tsqa_walk_frames(raw.ctypes.data, len(blob), cap, frame_at, sizes, ext, out_len, C.byref(nb), C.byref(total))
    return rc, list(out_len[:nb.value])


def test_the_new_names_are_declared_and_exported():
    head = open(os.path.join(ROOT, "include", "turbosqueeze_amd.h")).read()
    L = tsq.lib()
    for name in ("tsqa_plan_index_packed", "tsqa_index_create_packed_async", "tsqa_index_create_packed", "tsqa_index_fetch",
                 "tsqa_index_device_tables"):
        assert re.search(r"\b" + name + r"\s*\(", head) and hasattr(L, name), name
    assert callable(tsq.DeviceBatchIndex) and callable(tsq.plan_index_packed)
    assert hasattr(tsq.DeviceCodec, "index_packed_async")


def test_the_planner_refuses_what_it_says():
    good = ([1, 2], [5, 9000], [0, 0], [0, 0])
    assert tsq.plan_index_packed(*good, 3)[4] == OK
    for args in (([], [], [], [], 3), (*good, 0), ([1, 0], [5, 0], [0, 0], [0, 0], 3), ([1, 1], [5, pg.BLOCK + 1], [0, 0], [0, 0], 3)):
        with pytest.raises(tsq.TsqError):
            tsq.plan_index_packed(*args)
    # an item that the header check refused is not looked at
    assert tsq.plan_index_packed([1, 0], [5, 1 << 60], [0, ERR_FORMAT], [0, 0], 3)[2] == [OK, ERR_FORMAT]


def rooms(e):
    """every cap_blocks at which the fit changes, and the one the case runs at"""
    need = e["words"][2]
    return sorted({1, max(need - 1, 1), max(need, 1), need + 1, e["cap_blocks"]} | {max(x, 1) for x in e["first_block"][1:]})[:12]


@pytest.mark.parametrize("case", pg.every_case(), ids=lambda c: c.name)
def test_the_planner_equals_the_restatement(case):
    base = case.expect()
    for cap in rooms(base):
        e = case.expect(cap_blocks=cap)
        got = tsq.plan_index_packed(e["blocks"], e["totals"], e["head"], e["walk"], cap)
        assert got == (e["item_first"], e["item_at"], e["item_status"], e["words"], e["status"]), (case.name, cap)
        # the rule itself: the unfit items are exactly the accepted ones from the first that does not fit
        assert [i for i, st in enumerate(e["item_status"]) if st == ERR_OVERFLOW] == [i for i in range(e["n_fit"], case.n) if e["head"][i] == OK]
        assert e["words"][0] <= cap and e["words"][0] == sum(b for b, st in zip(e["blocks"], e["item_status"]) if st == OK)


@pytest.mark.parametrize("case", pg.plain_cases(), ids=lambda c: c.name)
def test_the_plain_walk_is_the_librarys_and_the_oracles(case, oracle):
    e = case.expect()
    seen = set()
    for i in range(case.n):
        if e["head"][i] != OK:
            continue
        blob = case.container(i)
        if blob in seen:
            continue
        seen.add(blob)
        rc, out_len = lib_walk(blob)
        mine = pg.walk(blob, e["blocks"][i], e["totals"][i])
        assert (rc == 0) == (mine is not None), (case.name, i)
        if mine is not None:
            assert out_len == mine and sum(mine) == e["totals"][i]
            if case.datas[i] is not None and len(blob) < 1 << 20:
                assert oracle.decompress(blob) == case.datas[i], (case.name, i)


def plan_item_ranges_takes(e, ranges):
    out_start = np.cumsum([0] + e["out_len"]).tolist()
    assert out_start[-1] == e["words"][1] and len(e["out_len"]) == e["words"][0]
    return tsq.plan_item_ranges(out_start, e["item_first"], ranges, 1 << 40)


@pytest.mark.parametrize("case", pg.every_case(), ids=lambda c: c.name)
def test_the_tables_are_what_the_record_reads_plan_from(case):
    """item_first, item_at and the blocks' lengths fit together as tsqa_plan_item_ranges expects of a batch index: every healthy
    item owns the blocks that hold its bytes, and a refused or unfit one owns none"""
    e = case.expect()
    out_start = np.cumsum([0] + e["out_len"]).tolist()
    for i in range(case.n):
        fb, fe = e["item_first"][i], e["item_first"][i + 1]
        if e["item_status"][i] == OK:
            assert fe - fb == e["blocks"][i] and out_start[fb] == e["item_at"][i] and out_start[fe] - out_start[fb] == e["totals"][i]
        else:
            assert fb == fe
    healthy = [(i, o, n) for i, o, n in pg.ranges(case, e) if e["item_status"][i] == OK]
    at, quads = 0, []
    for i, o, n in healthy:
        quads.append((i, o, n, at))
        at += n
    if quads:
        items, groups = plan_item_ranges_takes(e, quads)
        assert sum(hi - lo for _, lo, hi, _ in items) == at and len(groups) <= e["words"][0]
    sick = [r for r in pg.ranges(case, e) if e["item_status"][r[0]] != OK]
    for i, o, n in sick[:3]:
        with pytest.raises(tsq.TsqError):
            plan_item_ranges_takes(e, [(i, o, n, 0)])


def test_item_counts_reach_the_scans_passes():
    assert [c.n for c in pg.item_counts()] == [1, 2, 255, 256, 257, 513]
    for c in pg.item_counts():
        e = c.expect()
        assert e["item_status"] == [OK] * c.n and e["blocks"] == [1] * c.n and e["item_first"] == list(range(c.n + 1))
        assert all(1 <= t <= 4096 for t in e["totals"])
    e = pg.three_blocks().expect()
    assert sorted(e["blocks"]) == [1] * 9 + [3] and e["blocks"][5] == 3 and e["item_first"][6:] == [8, 9, 10, 11, 12]


def test_the_totals_scan_passes_2_24_where_the_names_say():
    inside, across = pg.carry_totals()
    for c in (inside, across):
        e = c.expect()
        assert e["status"] == OK and c.n == 300 and sum(t == pg.BLOCK for t in e["totals"]) == 5
        cum = np.cumsum(e["totals"])
        k = int(np.argmax(cum >= pg.SPLIT))                  # the first item whose inclusive sum is at or past 2^24
        if c is inside:
            assert 0 < k < pg.WAVE - 1, k                    # lanes of the first wavefront see the crossing in their own sum
        else:
            own = [int(np.sum(e["totals"][w:w + pg.WAVE])) for w in (0, pg.WAVE)]
            assert own[0] < pg.SPLIT and own[1] < pg.SPLIT <= own[0] + own[1] and pg.WAVE <= k < 2 * pg.WAVE
        assert e["item_at"][pg.GROUP] > pg.SPLIT              # and the second pass starts above it


def test_the_frame_places_pass_2_24_inside_a_pass():
    (alone, fronted), hit = pg.carry_places()
    for c in (alone, fronted):
        e = c.expect()
        assert e["status"] == OK and e["item_status"] == [OK] * c.n
        # the sized walk sums the rooms of the whole batch's frames, 256 per workgroup: the sum in front of frame k
        rooms = np.cumsum([0] + [pg.WORD + s for s in c.table])
        k = int(np.argmax(rooms >= pg.SPLIT))
        assert 0 < k < len(c.table) and k % pg.GROUP != 0, "a workgroup's own scan carries out of its low 24 bits"
        if c is alone:
            assert k < pg.GROUP and rooms[pg.GROUP] > pg.SPLIT, "and the second group's base has an upper part"
        else:
            assert pg.GROUP < k and 0 < rooms[pg.GROUP] < pg.SPLIT, "here the crossing is made of the second group's base and its own scan"
    assert alone.n == 1 and alone.expect()["blocks"] == [300]
    assert fronted.n == 2 and fronted.expect()["blocks"][1] == 300 and hit[1] % pg.WAVE == 0


def test_every_refusal_is_refused_by_its_rule_in_its_place():
    seen = {}
    for c in pg.refusals():
        e = c.expect()
        assert c.n == 300 and e["status"] == ERR_FORMAT
        assert [i for i, st in enumerate(e["item_status"]) if st != OK] == list(pg.REFUSAL_AT), c.name
        names = c.name[len("refusals_"):]
        for at in pg.REFUSAL_AT:
            by_header = e["head"][at] != OK
            assert e["item_status"][at] == ERR_FORMAT and (by_header or e["walk"][at] == ERR_FORMAT)
            seen.setdefault(at, set()).add(by_header)
        # the walk-refused items leave gaps in the provisional table: blocks that the header claimed and the index does not hold
        assert e["words"][2] - e["words"][0] == sum(e["blocks"][at] for at in pg.REFUSAL_AT), names
        assert e["item_first"][-1] == e["words"][0] == 295 + 2 * 8      # 295 one-block items and mtgen's eight blocks twice
    kinds = pg._refusal_kinds()
    assert len(kinds) == 16 and sum(1 for it in kinds if it.place) == 2
    # every kind, the bad places and the twin included, stands as item 0, as item 256 and as the last item in some batch
    stood = {}
    for c in pg.refusals():
        for at, name in zip(pg.REFUSAL_AT, c.kinds):
            stood.setdefault(name, set()).add(at)
    assert stood == {it.name: set(pg.REFUSAL_AT) for it in kinds}, {k: sorted(v) for k, v in stood.items() if v != set(pg.REFUSAL_AT)}
    assert {"place_past", "place_short", "bad_magic", "mt_twin_walk", "mt_cut_mid_stream"} <= set(stood)
    past = next(c for c in pg.refusals() if c.kinds[2] == "place_past")
    assert past.offsets[-1] + past.sizes[-1] == past.arena.size + 3 and past.expect()["head"][-1] == ERR_FORMAT
    assert all(seen[at] == {True, False} for at in pg.REFUSAL_AT), "both a header refusal and a walk refusal in every place"
    gaps = [c for c in pg.refusals() if any(c.expect()["head"][at] == OK for at in pg.REFUSAL_AT)]
    assert len(gaps) >= 6


def test_the_caps_cut_where_they_say():
    cuts = pg.cap_cuts()
    assert [n_fit for _, n_fit in cuts] == [10, 9, 5, 10]
    for c, n_fit in cuts:
        e = c.expect()
        assert e["n_fit"] == n_fit and e["words"][2] == 12
        assert [st == ERR_OVERFLOW for st in e["item_status"]] == [i >= n_fit for i in range(c.n)]
    inside = cuts[2][0].expect()
    assert inside["cap_blocks"] == 6 and inside["words"][0] == 5 and inside["blocks"][6] == 1      # item 6 would fit, and does not count


def test_true_tables_give_the_plain_forms_result():
    for c in list(pg.sized_true()) + list(pg.carry_places()[0]):
        e, p = c.expect(), c.expect(plain=True)
        assert e["status"] == OK
        for key in ("item_status", "item_first", "item_at", "words", "out_len"):
            assert e[key] == p[key], (c.name, key)
    assert [c.n for c in pg.sized_true()[:5]] == [1, 255, 256, 257, 513]


def test_false_tables_refuse_their_item_alone():
    cases = pg.sized_false()
    assert len(cases) == 15
    for c, why in cases:
        e, p = c.expect(), c.expect(plain=True)
        assert e["item_status"] == [ERR_FORMAT if i == pg.FALSE_AT else OK for i in range(c.n)], (c.name, why)
        assert e["head"][pg.FALSE_AT] == OK and e["blocks"][pg.FALSE_AT] == pg.FALSE_BLOCKS          # the walk refuses it, not the header
        assert e["item_first"][pg.FALSE_AT + 1:] == list(range(pg.FALSE_AT, 257))
        # the plain walk takes the container wherever only the table lies
        assert (p["item_status"][pg.FALSE_AT] == OK) == (why in (pg.kg.WORD, pg.kg.LENGTH)), (c.name, why)
    for c, verdicts in pg.sized_bad_first():
        e = c.expect()
        assert {i: st for i, st in enumerate(e["item_status"]) if st != OK} == verdicts, c.name
        assert c.expect(plain=True)["status"] == OK
    g = pg.sized_geometry()
    assert g.expect()["item_status"] == [OK, OK, ERR_FORMAT, OK, OK] and g.expect(plain=True)["status"] == OK
    assert g.block_len == 1 << 21 and g.table_first[3] - g.table_first[2] == 2
