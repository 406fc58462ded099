"""CPU-only: cutgen's restatements against the host-only planner (tsqa_plan_cut), the host frame walk (tsqa_walk_frames) and the
oracle, and that each of its cases reaches what it aims at.  The kernels' side of the same cases: test_gpu_cut.py."""
import ctypes as C

import numpy as np
import pytest

import cutgen as cg
import turbosqueeze_amd as tsq


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


@pytest.fixture(scope="module")
def healthy():
    return {c.name: (c, c.expect(1 << 62)) for c in cg.healthy_cases()}


def plan(source, ranges, align, out_size):
    try:
        return tsq.plan_cut(source.frame_at, source.out_start, ranges, align, out_size)
    except tsq.TsqError as err:
        assert err.code == cg.ERR_ARG
        return None


def test_the_sources_walk_as_the_library_walks_them():
    for s in (cg.tiny(), cg.two_blocks(), cg.split(), cg.random8()):
        rc, nb, total, frame_at, sizes, out_len = host_walk(s.blob)
        assert rc == 0 and nb == s.n_blocks and total == len(s.data), s.name
        assert frame_at == s.frame_at[:-1] and s.frame_at[-1] == frame_at[-1] + 3 + sizes[-1] == len(s.blob), s.name
        assert [int(a) for a in np.cumsum([0] + out_len)] == s.out_start, s.name
        if s.table is not None:
            assert sizes == s.table, s.name
    t = cg.tiny()
    lens = [b - a for a, b in zip(t.out_start, t.out_start[1:])]
    assert t.n_blocks == 600 and min(lens) == 1 and max(lens) == 40
    exts = [t.blob[a + 2] >> 7 for a in t.frame_at[:-1]]
    assert 200 < sum(exts) < 400 and any(a != b for a, b in zip(exts, exts[1:])), "the ext bits are not mixed per frame"
    frames = [b - a for a, b in zip(t.frame_at, t.frame_at[1:])]
    assert min(frames) == 9, min(frames)
    assert cg.two_blocks().n_blocks == 2 and len(cg.two_blocks().data) == cg.BLOCK + 1
    assert cg.split().n_blocks == 257 and set(b - a for a, b in zip(cg.split().out_start, cg.split().out_start[1:])) == {4096}
    assert cg.random8().n_blocks == 8 and all(b - a > 1 << 16 for a, b in zip(cg.random8().frame_at, cg.random8().frame_at[1:]))


def test_plan_cut_is_restated(healthy):
    for name, (case, e) in healthy.items():
        for out_size in (1 << 62, e["need"], e["need"] - 1, e["offsets"][len(case.ranges) // 2] + 20, 0):
            want = cg.plan_cut(case.source.frame_at, case.source.out_start, case.ranges, case.align, out_size)
            assert plan(case.source, case.ranges, case.align, out_size) == want, (name, out_size)
        assert e["item_status"] == [0] * len(case.ranges) and e["status"] == 0 and e["n_fit"] == len(case.ranges), name
        assert e["offsets"] == tsq.plan_packed(e["sizes"], case.align), name
    for name, at in cg.refusal_cases():
        case = cg.refusal(name, at)
        for out_size in (1 << 62, 0):
            want = cg.plan_cut(case.source.frame_at, case.source.out_start, case.ranges, case.align, out_size)
            assert plan(case.source, case.ranges, case.align, out_size) == want, (name, at, out_size)


def test_every_expected_container_is_walked_by_the_host_walk_and_decoded_by_the_oracle(healthy, oracle):
    seen = set()
    for name, (case, e) in healthy.items():
        s = case.source
        for k, ((f, c), blob) in enumerate(zip(case.ranges, e["containers"])):
            if (s.name, f, c) in seen:
                continue
            seen.add((s.name, f, c))
            assert len(blob) == e["sizes"][k] and e["offsets"][k] % case.align == 0, (name, k)
            rc, nb, total, frame_at, sizes, _ = host_walk(blob)
            assert rc == 0 and nb == c and total == e["totals"][k] == len(case.data(k)), (name, k)
            assert frame_at[-1] + 3 + sizes[-1] == len(blob), (name, k)
            got = oracle.decompress(blob, threads=2 if total > cg.BLOCK else 1)
            assert got is not None and bytes(got) == case.data(k), (name, k)
            assert case.data(k) == s.data[s.out_start[f]:s.out_start[f + c]]
    assert len(seen) > 500


def test_the_whole_range_is_the_source_up_to_the_end_of_its_last_frame(healthy):
    for n in cg.WHOLE:
        case, e = healthy[f"whole_{n}"]
        s = case.source
        assert case.ranges == [(0, s.n_blocks)] and e["containers"][0] == s.blob[:s.frame_bytes] and e["need"] == s.frame_bytes, n


def test_small_containers_put_seams_at_every_residue(healthy):
    """A container is at least 16 + 6 bytes, so a 16-byte word holds bytes of at most two containers: a word across a seam is
    cut by the tail of one body and the header of the next, at every residue where align is 1."""
    case, e = healthy["tiny_513"]
    assert min(e["sizes"]) == 25 and case.align == 1
    starts, ends, shift, two, most = cg.seams(case)
    print("tiny_513: start residues", sorted(starts), "end residues", sorted(ends), "shifts", sorted(shift), "words of two containers", two,
          "containers per word at most", most)
    assert starts == ends == shift == set(range(16)) and most == 2 and two >= 400
    per_residue = {}
    for o in e["offsets"][1:-1]:
        per_residue[o % 16] = per_residue.get(o % 16, 0) + 1
    print("tiny_513: seams per destination residue", sorted(per_residue.items()))
    assert len(per_residue) == 16 and min(per_residue.values()) >= 8
    for align in cg.ALIGNS:
        c, ea = healthy[f"tiny_257_align_{align}"]
        starts, ends, shift, two, most = cg.seams(c)
        assert all(o % align == 0 for o in ea["offsets"][:-1]) and len(ends) == 16 and len(shift) == 16, align
        if align >= 16:
            assert starts == {0} and two == 0 and most == 1       # (padding between them: a word is cut by a container's end alone)
            assert any(b - a > s for a, b, s in zip(ea["offsets"], ea["offsets"][1:-1], ea["sizes"])), "no padding"
    assert sorted(len(c.ranges) for c in cg.counts()) == list(cg.COUNTS)
    counts = {c for _, c in healthy["tiny_513"][0].ranges}
    assert counts == {1, 2, 3, 4, 5}


def test_places_pass_2_to_the_24_where_they_aim(healthy):
    inside, edge = healthy["carry_inside_a_wavefront"][0], healthy["carry_at_a_wavefront_edge"][0]
    at = cg.crossing(inside)
    print("carry_inside_a_wavefront: the first place at or above 2^24 is range", at)
    assert at == 247 and at % cg.WAVE not in (0, cg.WAVE - 1) and at < cg.GROUP
    at = cg.crossing(edge)
    print("carry_at_a_wavefront_edge: the first place at or above 2^24 is range", at)
    assert at == cg.CARRY_EDGE_CROSSING and at % cg.WAVE == 0 and at < cg.GROUP
    assert edge.ranges[0] == (0, 8) and edge.ranges[at - 1][1] == 1 and {c for _, c in edge.ranges[1:]} == {1, 2}
    for c in (inside, edge):
        assert len(c.ranges) == 300 and c.source.n_blocks == 8 and cg.SPLIT < c.need < 30_000_000
        assert len(set(c.ranges)) <= 16, "the ranges do not repeat"


def test_the_sized_ranges_are_what_they_say(healthy):
    case, e = healthy["split_ranges"]
    assert case.ranges == [(0, 1), (255, 2), (256, 1), (0, 257)] and case.source.block_len == 4096
    assert e["totals"] == [4096, 8192, 4096, 257 * 4096]
    assert e["containers"][3] == case.source.blob and e["containers"][1].endswith(e["containers"][2][16:])
    case, e = healthy["two_blocks_each"]
    assert e["totals"] == [1, cg.BLOCK] and sum(e["sizes"]) == case.source.frame_bytes + 16


def test_each_refused_range_is_refused_alone():
    for name, at in cg.refusal_cases():
        case = cg.refusal(name, at)
        f, c = case.ranges[at]
        assert cg.measure(case.source.frame_at, case.source.out_start, f, c) is None, name
        e = case.expect(1 << 62)
        assert e["item_status"] == [cg.ERR_ARG if k == at else 0 for k in range(300)] and e["status"] == cg.ERR_ARG, (name, at)
        assert e["sizes"][at] == 0 and e["totals"][at] == 0 and e["offsets"][at + 1] == e["offsets"][at] and e["containers"][at] is None
        # the others keep their places but for the room the refused one gives up
        clean = cg.Case("clean", case.source, case.ranges[:at] + case.ranges[at + 1:], 16).expect(1 << 62)
        assert e["containers"][:at] + e["containers"][at + 1:] == clean["containers"]
        assert e["offsets"][:at] + e["offsets"][at + 1:-1] == clean["offsets"][:-1]
        m = case.expect(0)
        assert m["item_status"] == [cg.ERR_ARG if k == at else cg.ERR_OVERFLOW for k in range(300)] and m["offsets"] == e["offsets"]
    f, c = cg.REFUSALS["one_block_too_many"]
    assert f + c == cg.TINY_BLOCKS + 1 and cg.measure(cg.tiny().frame_at, cg.tiny().out_start, f, c - 1) is not None
    assert (cg.ALL_ONES + cg.ALL_ONES) % (1 << 64) == cg.ALL_ONES - 1 and ((1 << 32) + 1) % (1 << 32) == 1, "these sums wrap in 64 and 32 bits"
    assert len(cg.refusal_cases()) == 18


def test_rooms_cut_the_fitting_prefix():
    for what, case, out_size, n_fit in cg.rooms():
        e = case.expect(out_size if out_size is not None else 0)
        full = case.expect(1 << 62)
        n = len(case.ranges)
        assert e["n_fit"] == n_fit, what
        assert e["item_status"] == [0] * n_fit + [cg.ERR_OVERFLOW] * (n - n_fit), what
        assert (e["offsets"], e["sizes"], e["totals"]) == (full["offsets"], full["sizes"], full["totals"]), what
        assert e["containers"][:n_fit] == full["containers"][:n_fit] and e["containers"][n_fit:] == [None] * (n - n_fit), what
        assert e["status"] == (0 if n_fit == n else cg.ERR_OVERFLOW), what
        if out_size is not None and n_fit < n:
            assert e["offsets"][n_fit] <= out_size < e["offsets"][n_fit] + e["sizes"][n_fit], what
    table = {what: (out_size, n_fit) for what, _, out_size, n_fit in cg.rooms()}
    c = cg.aligned(16)
    o = c.expect(1 << 62)["offsets"]
    assert o[cg.ROOM_MIDDLE] < table["room that ends inside a header"][0] < o[cg.ROOM_MIDDLE] + 16
    assert o[cg.ROOM_MIDDLE] + 16 < table["room that ends inside a middle container"][0] < o[cg.ROOM_MIDDLE] + 25
    assert table["one byte short of the last container"] == (c.need - 1, 256)
    # a retry with the reported room fits everything
    assert c.expect(c.expect(0)["need"])["status"] == 0


def test_plan_cut_refuses_bad_arguments():
    L = tsq.lib()
    u64 = lambda *v: (C.c_uint64 * len(v))(*v)
    frame_at, out_start, first, count = u64(16, 30, 50), u64(0, 10, 20), u64(0, 1), u64(2, 1)
    offsets, sizes, totals, status, n_fit = u64(7, 7, 7), u64(7, 7), u64(7, 7), (C.c_int32 * 2)(7, 7), C.c_uint32(7)
    full = [frame_at, out_start, 2, first, count, 2, 16, 1000, offsets, sizes, totals, status, C.byref(n_fit)]
    for k in (0, 1, 3, 4, 8, 9, 11, 12):
        args = list(full)
        args[k] = None
        assert L.tsqa_plan_cut(*args) == cg.ERR_ARG, k
    for k, v in [(2, 0), (5, 0), (6, 0), (6, 3), (6, 8192)]:
        args = list(full)
        args[k] = v
        assert L.tsqa_plan_cut(*args) == cg.ERR_ARG, (k, v)
    for bad in (dict(frame_at=u64(15, 30, 50)), dict(frame_at=u64(16, 21, 50)), dict(frame_at=u64(16, 60, 50)),
                dict(out_start=u64(0, 10, 5)), dict(out_start=u64(0, 10, 11 + cg.BLOCK))):
        args = list(full)
        if "frame_at" in bad:
            args[0] = bad["frame_at"]
        else:
            args[1] = bad["out_start"]
        assert L.tsqa_plan_cut(*args) == cg.ERR_ARG, bad
    assert list(offsets) == [7, 7, 7] and list(status) == [7, 7] and n_fit.value == 7, "a refused call wrote"
    assert L.tsqa_plan_cut(*full) == 0
    assert (list(offsets), list(sizes), list(totals), list(status), n_fit.value) == ([0, 64, 100], [50, 36], [20, 10], [0, 0], 2)
    args = list(full)
    args[10] = None                                          # totals may be NULL
    args[7] = 99
    assert L.tsqa_plan_cut(*args) == 0 and list(status) == [0, cg.ERR_OVERFLOW] and n_fit.value == 1
    with pytest.raises(tsq.TsqError):
        tsq.plan_cut([16, 30], [0, 10, 20], [(0, 1)])
