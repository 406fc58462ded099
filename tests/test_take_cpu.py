"""CPU-only: takegen's restatements against the host-only planners (tsqa_plan_cut_items, tsqa_plan_cut), the host frame walk
(tsqa_walk_frames) and the oracle, and that each of its cases reaches what it aims at.  The kernels' side of the same cases:
test_gpu_take.py.  The new names of the C ABI are checked here too."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cutgen as cg
import joingen as jg
import takegen as tk
import turbosqueeze_amd as tsq

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = tk.OK, tk.ERR_ARG, tk.ERR_FORMAT, tk.ERR_OVERFLOW
NEW_NAMES = ("tsqa_plan_cut_items", "tsqa_cut_items_async", "tsqa_cut_items")


def host_walk(blob: bytes):
    """tsqa_walk_frames on a container -> (rc, n_blocks, total, frame_at, [stream_len], [out_len])"""
    raw = np.frombuffer(blob, dtype=np.uint8)
    cap = max(int.from_bytes(blob[4:8], "little"), 1)
    frame_at, sizes, ext, out_len = (np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32),
                                     np.zeros(cap, dtype=np.uint32))
    nb, total = C.c_uint32(0), C.c_uint64(0)
    rc = tsq.lib().tsqa_walk_frames(raw.ctypes.data, raw.size, cap, frame_at.ctypes.data, sizes.ctypes.data, ext.ctypes.data,
                                    out_len.ctypes.data, C.byref(nb), C.byref(total))
    k = nb.value
    return rc, k, total.value, [int(a) for a in frame_at[:k]], [int(s) for s in sizes[:k]], [int(n) for n in out_len[:k]]


def library_plan(case, out_size):
    ix = case.index
    frame_at, out_start = ix.plan_tables()
    return tsq.plan_cut_items(frame_at, out_start, ix.item_first, case.items, case.ranges, case.align, out_size)


def restated_plan(case, out_size):
    return tk.plan(case.index, case.items, case.ranges, case.align, out_size)[:5]


@pytest.fixture(scope="module")
def healthy():
    return {c.name: (c, c.expect(1 << 62)) for c in tk.healthy_cases()}


def test_the_new_names_are_exported_declared_and_bound():
    L = tsq.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "turbosqueeze_amd.h")).read()
    for name in NEW_NAMES:
        assert getattr(L, name).argtypes is not None, name
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert hasattr(tsq.DeviceCodec, "cut_items_async") and callable(tsq.BatchIndex.cut_items) and callable(tsq.PackedBatch.take)
    assert tsq.DeviceBatchIndex.cut_items is tsq.BatchIndex.cut_items and not hasattr(tsq.RangeIndex, "cut_items")


def test_the_index_restatement_walks_the_items_as_the_library_does():
    for b in (tk.ragged(513), tk.random8_long(), tk.pages(), tk.three_blocks(), tk.damaged("headers"), tk.damaged("walks")):
        ix = b.index()
        at = 0
        for i, (o, n) in enumerate(zip(b.offsets, b.sizes)):
            blob = bytes(b.arena[o:o + n]) if o + n <= b.arena.size else b""
            rc, nb, total, frame_at, sizes, out_len = host_walk(blob) if len(blob) >= 16 else (ERR_FORMAT, 0, 0, [], [], [])
            assert (rc == 0) == (ix.item_status[i] == OK), (b.name, i)
            if rc:
                assert ix.item_first[i + 1] == ix.item_first[i]
                continue
            fb = ix.item_first[i]
            assert ix.item_first[i + 1] - fb == nb and ix.src[fb:fb + nb] == [o + a for a in frame_at], (b.name, i)
            assert ix.end[fb:fb + nb] == [o + a + 3 + s for a, s in zip(frame_at, sizes)], (b.name, i)
            assert ix.out_start[fb:fb + nb + 1] == [at + int(x) for x in np.cumsum([0] + out_len)], (b.name, i)
            assert b.datas[i] is None or len(b.datas[i]) == total
            at += total
        assert ix.total == at and ix.n_blocks == len(ix.src)
    for which in tk.DAMAGED:
        d = tk.damaged(which)
        assert [i for i, st in enumerate(d.index().item_status) if st] == list(tk.REFUSAL_AT), "the refused items are not items 0, 256 and 299"
        assert d.kinds == tk.DAMAGED[which]
        for at in tk.REFUSAL_AT:                             # a cut container's header passes: only the walk refuses it
            nb, _ = tk.pg.measure(d.arena, d.arena.size, d.offsets[at], d.sizes[at])
            assert (nb != 0) == (which == "walks"), (which, at)


def test_plan_cut_items_is_restated(healthy):
    for name, (case, e) in healthy.items():
        mid = e["offsets"][case.n // 2] + 20
        for out_size in (1 << 62, e["need"], e["need"] - 1, mid, 0):
            assert library_plan(case, out_size) == restated_plan(case, out_size), (name, out_size)
        assert e["item_status"] == [0] * case.n and e["status"] == 0 and e["n_fit"] == case.n, name
        if case.n <= 1024:
            assert e["offsets"] == tsq.plan_packed(e["sizes"], case.align), name
    for case in tk.refusal_cases():
        for out_size in (1 << 62, 0):
            assert library_plan(case, out_size) == restated_plan(case, out_size), (case.name, out_size)
    for what, case, out_size, _ in tk.rooms():
        assert library_plan(case, out_size or 0) == restated_plan(case, out_size or 0), what
    for c in (tk.kinds_case(), tk.sized_batch_case()):
        assert library_plan(c, 1 << 62) == restated_plan(c, 1 << 62), c.name


def test_one_item_is_the_cut(healthy):
    """through an index of one item the take owes what tsqa_plan_cut and cutgen owe for the same ranges"""
    for name in ("tiny", "split"):
        case, cut = tk.single(name)
        s = cut.source
        for out_size in (1 << 62, cut.need - 1, 0):
            want = tsq.plan_cut(s.frame_at, s.out_start, cut.ranges, cut.align, out_size)
            assert restated_plan(case, out_size) == want == cg.plan_cut(s.frame_at, s.out_start, cut.ranges, cut.align, out_size), name
            # item_first_block NULL and items NULL: one item that owns every block
            assert tsq.plan_cut_items(s.frame_at, s.out_start, None, None, cut.ranges, cut.align, out_size) == want, name
        e, ce = case.expect(1 << 62), cut.expect(1 << 62)
        assert [case.container(e, k) for k in range(case.n)] == ce["containers"], name
    *_, case = tk.refused_index()
    e = case.expect(1 << 62, True)
    assert e["item_status"] == [ERR_FORMAT] * case.n and e["need"] == 0 and e["spans"] == [None] * case.n


def test_every_expected_container_is_walked_by_the_host_walk_and_decoded_by_the_oracle(healthy, oracle):
    seen = set()
    for name, (case, e) in healthy.items():
        for k in range(case.n):
            key = (case.batch.name, case.items[k], case.ranges[k] if case.ranges else None)
            if key in seen:
                continue
            seen.add(key)
            blob = case.container(e, k)
            assert len(blob) == e["sizes"][k] and e["offsets"][k] % case.align == 0, (name, k)
            rc, nb, total, frame_at, sizes, _ = host_walk(blob)
            assert rc == 0 and total == e["totals"][k] == len(case.data(k)), (name, k)
            assert frame_at[-1] + 3 + sizes[-1] == len(blob), (name, k)
            got = oracle.decompress(blob, threads=2 if total > cg.BLOCK else 1)
            assert got is not None and bytes(got) == case.data(k), (name, k)
    assert len(seen) > 1500, len(seen)


def test_the_identity_gives_the_items_back(healthy):
    case, e = healthy["identity"]
    b = case.batch
    assert case.items == list(range(b.n)) and all(o % 16 == 0 for o in b.offsets)
    for k in range(case.n):
        blob = bytes(b.arena[b.offsets[k]:b.offsets[k] + b.sizes[k]])
        assert case.container(e, k) == blob[:e["sizes"][k]] and e["sizes"][k] == len(blob), k     # (no tails here: up to the last frame is all)
    assert e["offsets"][:-1] == b.offsets, "the taken arena is not laid out as the source"


def test_the_permutation_joins_to_the_permuted_data(healthy, oracle):
    case, e = healthy["permutation"]
    assert len(set(case.items)) < case.n and sorted(set(case.items)) != list(range(257)), "no repeats, or no gaps"
    assert case.items != sorted(case.items)
    container, _ = jg.joined([case.container(e, k) for k in range(case.n)])
    want = b"".join(case.batch.datas[i] for i in case.items)
    got = oracle.decompress(container, threads=1)
    assert got is not None and bytes(got) == want


def test_small_containers_put_seams_at_every_residue(healthy):
    case, e = healthy["ragged_513"]
    assert min(e["sizes"]) >= 22 and case.align == 1
    starts, ends, shift = tk.seams(case)
    print("ragged_513: start residues", sorted(starts), "end residues", sorted(ends), "shifts", sorted(shift), "smallest container", min(e["sizes"]))
    assert starts == ends == shift == set(range(16))
    for align in tk.ALIGNS:
        c, ea = healthy[f"ragged_257_align_{align}"]
        starts, ends, shift = tk.seams(c)
        assert all(o % align == 0 for o in ea["offsets"][:-1]) and len(ends) == 16 and len(shift) == 16, align
    assert [c.n for c in tk.counts()] == list(tk.COUNTS)


def test_the_counts_sit_on_the_pass_edge(healthy):
    assert tk.PASS == 65536 and tk.PASS_COUNTS == (65535, 65536, 65537)
    for n in tk.PASS_COUNTS:
        case, e = healthy[f"pass_edge_{n}"]
        groups = (n + tk.GROUP - 1) // tk.GROUP
        assert case.n == n and groups == (257 if n > tk.PASS else 256)
        assert (groups + 255) // 256 == (2 if n > tk.PASS else 1), "launch (b)'s passes"
        assert e["need"] < 8 << 20 and len(set(case.items)) == 513
    # the last range of the largest case is the only one of its group and of its pass
    assert (tk.PASS_COUNTS[2] - 1) % tk.GROUP == 0 and (tk.PASS_COUNTS[2] - 1) // tk.GROUP == 256


def test_places_pass_2_to_the_24_where_they_aim(healthy):
    inside, edge = healthy["carry_inside_a_group"][0], healthy["carry_at_a_wavefront_edge"][0]
    e = inside.expect(1 << 62)
    pad = [cg.round_up(s, 16) for s in e["sizes"]]
    for g in range(0, 600, tk.GROUP):
        own = [int(x) for x in np.cumsum([0] + pad[g:g + tk.GROUP])]
        if g + tk.GROUP <= 600:                              # inside the group's own scan, away from a wavefront's edge
            lane = next(k for k, o in enumerate(own) if o >= tk.SPLIT)
            assert lane == 247 and lane % tk.WAVE not in (0, tk.WAVE - 1), lane
    bases = [sum(pad[:g]) for g in range(0, 600, tk.GROUP)]
    print("carry_inside_a_group: group bases", bases, "first place at or above 2^24: range", tk.crossing(inside))
    assert bases[0] == 0 and all(b >= tk.SPLIT for b in bases[1:]) and tk.crossing(inside) == 247
    at = tk.crossing(edge)
    print("carry_at_a_wavefront_edge: the first place at or above 2^24 is range", at)
    assert at == tk.LONG_CROSSING and at % tk.WAVE == 0 and 0 < at < tk.GROUP
    assert edge.items[0] == 8 and max(edge.expect(1 << 62)["sizes"]) == edge.expect(1 << 62)["sizes"][0]
    for c in (inside, edge):
        assert c.n == 600 and tk.SPLIT < c.need < 48_000_000 and len(set(c.items)) <= 9


def test_the_ranges_inside_items_are_what_they_say(healthy):
    case, e = healthy["pages"]
    nb = case.n
    assert nb == 1025 and e["totals"] == [4096] * (nb - 1) + [4095] and all(c == (j, 1) for j, c in enumerate(case.ranges))
    assert b"".join(case.data(k) for k in range(nb)) == case.batch.datas[tk.PAGES_ITEM]
    ix = case.index
    assert [ix.item_first[i + 1] - ix.item_first[i] for i in range(4)] == [1, 1, nb, 1], "the long item is not between one-block items"
    case, e = healthy["inner_ranges"]
    ix = case.index
    assert ix.item_first[tk.THREE_ITEM + 1] - ix.item_first[tk.THREE_ITEM] == 3
    assert ix.item_first[tk.THREE_ITEM] - ix.item_first[tk.THREE_ITEM - 1] == 1 == ix.item_first[tk.THREE_ITEM + 2] - ix.item_first[tk.THREE_ITEM + 1]
    whole = case.container(e, 5)
    item = bytes(case.batch.arena[case.batch.offsets[tk.THREE_ITEM]:][:case.batch.sizes[tk.THREE_ITEM]])
    assert whole == item and e["totals"][:6] == [4096, 4096, len(case.batch.datas[tk.THREE_ITEM]) - 8192, 8192, e["totals"][1] + e["totals"][2],
                                                 len(case.batch.datas[tk.THREE_ITEM])]
    assert whole.endswith(case.container(e, 4)[16:]) and case.container(e, 4).endswith(case.container(e, 2)[16:])


def test_each_refusal_is_refused_alone():
    for case in tk.refusal_cases():
        e, m = case.expect(1 << 62), case.expect(0)
        bad = [k for k, st in enumerate(e["item_status"]) if st]
        assert all(e["item_status"][k] == ERR_ARG and e["sizes"][k] == 0 and e["totals"][k] == 0 and e["offsets"][k + 1] == e["offsets"][k] and
                   e["spans"][k] is None for k in bad), case.name
        assert m["item_status"] == [ERR_ARG if k in bad else ERR_OVERFLOW for k in range(case.n)] and m["offsets"] == e["offsets"], case.name
        if case.name.startswith("refusal_"):
            at = int(case.name.rsplit("_", 1)[1])
            assert bad == [at] and case.n == 300 and at in tk.REFUSAL_AT, case.name
            keep = [k for k in range(300) if k != at]
            clean = tk.Case("clean", case.batch, [case.items[k] for k in keep], None if case.ranges is None else [case.ranges[k] for k in keep],
                            16, case.cap_blocks).expect(1 << 62)
            assert [e["spans"][k] for k in keep] == clean["spans"] and [e["offsets"][k] for k in keep] == clean["offsets"][:-1], case.name
        elif case.name.startswith("edge_range"):
            assert bad == [], case.name
    for which in tk.DAMAGED:
        assert [k for k, st in enumerate(tk.refused_items(which).expect(1 << 62)["item_status"]) if st] == list(tk.REFUSAL_AT)
    u = tk.unfit_items()
    assert u.index.item_status == [OK] * tk.UNFIT_FROM + [ERR_OVERFLOW] * (300 - tk.UNFIT_FROM) and u.index.need_blocks == 300
    assert [k for k, st in enumerate(u.expect(1 << 62)["item_status"]) if st] == [0, 256] + list(range(257, 300))
    f, c = tk.BAD_RANGES["one_past_nb"]
    assert f + c == 3 + 1 and sum(tk.EDGE_RANGE) == 3
    f, c = tk.BAD_RANGES["first_all_ones_count_2"]
    assert (f + c) % (1 << 64) == 1, "this sum wraps in 64 bits, to a block inside the item"
    assert tk.BAD_ITEMS["item_is_n_items"] == tk._ragged_300().n
    assert len(tk.refusal_cases()) == 27


def test_rooms_cut_the_fitting_prefix():
    for what, case, out_size, n_fit in tk.rooms():
        e, full = case.expect(out_size if out_size is not None else 0), case.expect(1 << 62)
        assert e["n_fit"] == n_fit and e["item_status"] == [0] * n_fit + [ERR_OVERFLOW] * (case.n - n_fit), what
        assert (e["offsets"], e["sizes"], e["totals"]) == (full["offsets"], full["sizes"], full["totals"]), what
        assert e["spans"][:n_fit] == full["spans"][:n_fit] and e["spans"][n_fit:] == [None] * (case.n - n_fit), what
        if out_size is not None and n_fit < case.n:
            assert e["offsets"][n_fit] <= out_size < e["offsets"][n_fit] + e["sizes"][n_fit], what
    c = tk.aligned(16)
    assert c.expect(c.expect(0)["need"])["status"] == 0


def test_plan_cut_items_refuses_bad_arguments():
    L = tsq.lib()
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    u32 = lambda *v: (C.c_uint32 * len(v))(*v)
    frame_at, out_start, item_first = u64(16, 30, 50, 80), u64(0, 10, 20, 25), u64(0, 2, 2, 3)
    items, first, count = u32(0, 2, 1), u64(0, 0, 0), u64(2, 1, 1)
    offsets, sizes, totals, status, n_fit = u64(7, 7, 7, 7), u64(7, 7, 7), u64(7, 7, 7), (C.c_int32 * 3)(7, 7, 7), C.c_uint32(7)
    full = [frame_at, out_start, 3, item_first, 3, items, first, count, 3, 16, 1000, offsets, sizes, totals, status, C.byref(n_fit)]
    for k in (0, 1, 3, 5, 6, 7, 11, 12, 14, 15):               # (first or count alone; items or item_first with three items)
        args = list(full)
        args[k] = None
        assert L.tsqa_plan_cut_items(*args) == ERR_ARG, k
    for k, v in [(4, 0), (8, 0), (9, 0), (9, 3), (9, 8192)]:
        args = list(full)
        args[k] = v
        assert L.tsqa_plan_cut_items(*args) == ERR_ARG, (k, v)
    for k, v in [(0, u64(15, 30, 50, 80)), (0, u64(16, 21, 50, 80)), (1, u64(0, 10, 5, 25)), (3, u64(0, 2, 1, 3)), (3, u64(0, 2, 2, 4))]:
        args = list(full)
        args[k] = v
        assert L.tsqa_plan_cut_items(*args) == ERR_ARG, (k, list(v))
    assert list(offsets) == [7] * 4 and list(status) == [7] * 3 and n_fit.value == 7, "a refused call wrote"
    assert L.tsqa_plan_cut_items(*full) == 0
    # item 0 owns blocks 0 and 1, item 1 none, item 2 block 2
    assert (list(offsets), list(sizes), list(totals), list(status), n_fit.value) == ([0, 64, 112, 112], [50, 46, 0], [20, 5, 0], [0, 0, ERR_ARG], 3)
    args = list(full)
    args[6] = args[7] = args[13] = None                      # whole items; totals may be NULL
    args[10] = 99
    assert L.tsqa_plan_cut_items(*args) == 0 and list(status) == [0, ERR_OVERFLOW, ERR_ARG] and n_fit.value == 1
    with pytest.raises(tsq.TsqError):
        tsq.plan_cut_items([16, 30], [0, 10, 20], None, None, [(0, 1)])
