"""CPU-only: findgen's restatement against the host-only rule (tsqa_plan_find), the host frame walk and the oracle, and that each of
its cases reaches what it aims at.  The kernels' side of the same cases: test_gpu_find.py."""
import os

import numpy as np
import pytest

import findgen as fg
import gathergen as gg
import recordgen as rg
import turbosqueeze_amd as tsq
from test_cut_cpu import host_walk

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = fg.OK, fg.ERR_ARG, fg.ERR_FORMAT, fg.ERR_OVERFLOW


def library_plan(case, flags=0, cap=None):
    """tsqa_plan_find on a case's decoded bytes -> (items, offsets, item_first, need) as lists"""
    items, offsets, first, need = tsq.plan_find(case.index.data, case.item_at(), case.needle, case.item_status(), flat=bool(flags & fg.FLAT), cap_hits=cap)
    return items.tolist(), offsets.tolist(), first.tolist(), [need]


def restated(e):
    return e["items"].tolist(), e["offsets"].tolist(), e["item_first"], e["need"]


def test_the_symbols_are_there():
    for name in ("tsqa_plan_find", "tsqa_find_async", "tsqa_find", "tsqa_profile_read_find"):
        assert hasattr(tsq.lib(), name), name
    assert (tsq.FIND_FLAT, tsq.FIND_MAX_NEEDLE) == (fg.FLAT, fg.MAX_NEEDLE) == (2, 16) and tsq.FIND_FLAT == tsq.RECORDS_FLAT
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "turbosqueeze_amd.h")) as f:
        header = f.read()
    assert "#define TSQA_FIND_FLAT 2u" in header and "#define TSQA_FIND_MAX_NEEDLE 16u" in header
    for name in ("RangeIndex", "SizedIndex", "BatchIndex", "DeviceBatchIndex"):
        assert hasattr(getattr(tsq, name), "find"), name
    assert hasattr(tsq.DeviceCodec, "find_async") and hasattr(tsq.DeviceCodec, "profile_read_find")
    assert hasattr(tsq.RecordTable, "containing") and hasattr(tsq.HitTable, "n") and callable(tsq.plan_find)


def test_the_sources_made_here_are_what_the_oracle_and_the_walk_say(oracle):
    """the hits are found in `data` and numbered by `item_first`: both are the containers' own"""
    for case in (fg.ring_wrap(), fg.seams(2), fg.phrase("plain", 2)):
        idx = case.index
        rc, nb, total, _, _, out_len = host_walk(idx.blob)
        assert rc == 0 and nb == idx.n_blocks and total == idx.total, case.name
        assert [int(x) for x in np.cumsum([0] + out_len)] == idx.out_start, case.name
        assert bytes(oracle.decompress(idx.blob)) == idx.data, case.name
    batches = [fg.places(m, False) for m in fg.NEEDLE_LENGTHS] + [fg.cell_edges(3, s) for s in fg.CELL_STARTS] + [fg.ring_wrap_skewed(), fg.ragged(257, 2)]
    for case in batches:
        idx, blocks, cat = case.index, 0, b""
        for k, (o, n) in enumerate(idx.spans):
            rc, nb, total, _, _, _ = host_walk(idx.blob[o:o + n])
            assert rc == 0 and nb == idx.item_first[k + 1] - idx.item_first[k] and total == idx.item_span(k)[1], (case.name, k)
            cat += bytes(oracle.decompress(idx.blob[o:o + n]))
            blocks += nb
        assert blocks == idx.n_blocks and cat == idx.data, case.name
    assert fg.phrase("sized", 2).index.blob == fg.phrase("plain", 2).index.blob


def test_lengths_and_places_reach_their_aim():
    """1: every needle length against every item length with the needle first, last, at both ends, nowhere and everywhere"""
    for m in fg.NEEDLE_LENGTHS:
        lengths = fg.place_lengths(m)
        assert set(fg.ITEM_LENGTHS) <= set(lengths) and {m, m + 1} <= set(lengths) and (m == 1 or m - 1 in lengths)
        mixed, equal = fg.places(m, False), fg.places(m, True)
        assert len(mixed.needle) == len(equal.needle) == m and mixed.index is equal.index
        idx, first_m, first_e = mixed.index, mixed.expect()["item_first"], equal.expect()["item_first"]
        assert idx.n_items == len(lengths) * len(fg.PLACES)
        for k in range(idx.n_items):
            n, where = lengths[k // 5], fg.PLACES[k % 5]
            a, t = idx.item_span(k)
            got = fg.item_hits(idx.data[a:a + t], mixed.needle).tolist()
            assert t == n and first_m[k + 1] - first_m[k] == len(got)
            if n < m:
                assert got == [] and first_e[k + 1] == first_e[k], "an item shorter than the needle has no hit"
            elif where == "everywhere":
                assert got == [] and first_e[k + 1] - first_e[k] == n - m + 1, "overlapping hits at every place"
            elif n >= 2 * m or where in ("first", "last", "nowhere"):
                # (an item shorter than two needles: 'both' holds what the two overlapping writes leave, which the restatement reads)
                assert got == {"first": [0], "last": [n - m], "both": sorted({0, n - m}), "nowhere": []}[where], (m, k)
                assert first_e[k + 1] == first_e[k]


def test_cell_and_word_edges_reach_their_aim():
    """2: in the item of 200 bytes, hits END at 62, 63, 64, 65 and 66 and -- for the needle of 3 -- at every residue mod 16; the items
    start at 0, 1, 38 and 63 of the concatenation"""
    for m in fg.CELL_NEEDLES:
        residues = set()
        for start in fg.CELL_STARTS:
            case = fg.cell_edges(m, start)
            idx = case.index
            a, t = idx.item_span(idx.n_items - 1)
            assert (a, t) == (start, fg.CELL_ITEM) and idx.n_items == (2 if start else 1)
            e = case.expect()
            ends = (e["offsets"][e["items"] == idx.n_items - 1] + m - 1).tolist()
            assert set(range(62, 67)) <= set(ends)
            assert {x % fg.CELL for x in ends} == set(range(16)) or m != 3
            residues |= {(x + start) % fg.CELL for x in ends}
        assert residues == set(range(16)), m


def test_chunk_edges_reach_their_aim():
    """3: in the zeros a hit ends at every position from m - 1 on; the other two needles occur, the text's often"""
    for m in (2, 16):
        case = fg.chunk_edges(f"zeros_{m}")
        assert case.index.total == 3 * fg.OUTC + 5 and case.expect()["offsets"].tolist() == list(range(3 * fg.OUTC + 5 - m + 1))
    assert fg.OUTC - 2 in fg.chunk_edges("random_4").expect()["offsets"].tolist()
    assert fg.chunk_edges("text_3").expect()["need"][0] > 100


def test_the_ring_wrap_reaches_its_aim():
    """4: needles of 16 bytes at every start k * R - skew - j, j = 0 .. 16, and one across 65 535 | 65 536; with the skew of the
    block's start mod 64 in the batch"""
    case = fg.ring_wrap()
    hits = set(case.expect()["offsets"].tolist())
    assert case.index.n_blocks == 1 and case.index.total == 1 << 18 and len(case.needle) == 16
    assert {k * fg.RING - j for k in (1, 2, 3) for j in range(17)} <= hits and 65528 in hits and 3 * fg.RING + 16 <= 1 << 18
    case = fg.ring_wrap_skewed()
    idx, e = case.index, case.expect()
    assert idx.n_blocks == 4 and [idx.out_start[1] % 64, idx.out_start[3] % 64] == [1, 38]
    for b in (1, 3):
        a, n = idx.out_start[b], idx.out_start[b + 1] - idx.out_start[b]
        got = set(e["offsets"][e["items"] == b].tolist())
        assert n > 2 * fg.RING and set(fg.ring_starts(a % 64, n)) <= got
        # a hit's first byte at the ring addresses R - 16 .. 0: the needle ends at the wrap, lies across it by every split, starts on it
        assert {(p + a % 64) % fg.RING for p in got} >= {(fg.RING - j) % fg.RING for j in range(17)}


def test_the_seams_reach_their_aim(oracle):
    """5: the hand-assembled container has a run of 20 one-byte blocks, blocks of 1 to 40 bytes, empty blocks and both ext bits; its
    hits lie in 2, 3 and 16 different blocks; the two-block and phrase cases have hits across their edges"""
    s = fg.seam_source()
    lens = [s.out_start[b + 1] - s.out_start[b] for b in range(s.n_blocks)]
    assert lens == fg.SEAM_LENGTHS and lens[:20] == [1] * 20 and 0 in lens and set(range(1, 41)) <= set(lens) | {0}
    exts = {s.blob[s.frame_at[b] + 2] >> 7 for b in range(s.n_blocks)}
    assert exts == {0, 1}
    for m in fg.SEAM_NEEDLES:
        case = fg.seams(m)
        e = case.expect()
        spans = {fg.blocks_of_hit(case.index, int(p), m) for p in e["offsets"]}
        assert e["need"][0] >= s.out_start[-1] // 7 - 2 and m in spans and (m == 2 or 2 in spans), (m, spans)
        # a hit whose bytes have empty blocks between them (the short needles occur every 7 bytes and may miss those places)
        assert m < 16 or any(gg.block_of(case.index.out_start, int(p) + m - 1) - gg.block_of(case.index.out_start, int(p)) + 1 > fg.blocks_of_hit(case.index, int(p), m)
                   for p in e["offsets"])
    for m in (2, 16):
        case = fg.two_blocks(m)
        assert case.index.out_start == [0, fg.BLOCK, fg.BLOCK + 1] and case.expect()["offsets"].tolist()[-1] == fg.BLOCK + 1 - m
        for kind in ("sized", "plain"):
            case = fg.phrase(kind, m)
            hits = set(case.expect()["offsets"].tolist())
            assert case.index.n_blocks == fg.PHRASE_BLOCKS
            assert all(b * fg.PHRASE_LEN - m // 2 in hits for b in range(1, fg.PHRASE_BLOCKS)), "a hit across every block edge"


def test_the_item_seams_reach_their_aim():
    """6: every byte of the ragged arenas is the same, and the only hits are those inside an item; the damaged items have none"""
    assert [fg.ragged(n, 2).index.n_items for n in fg.COUNTS] == [1, 2, 255, 256, 257, 513]
    for n in fg.COUNTS:
        idx = fg.ragged(n, 2).index
        assert set(idx.data) == {fg.RAGGED_BYTE}
        for m in (2, 16):
            e = fg.ragged(n, m).expect()
            want = [max(0, idx.item_span(k)[1] - m + 1) for k in range(n)]
            assert np.diff(e["item_first"]).tolist() == want and e["need"][0] < idx.total - m + 1 or n == 1
    lens = {fg.ragged(513, 2).index.item_span(k)[1] for k in range(513)}
    assert min(lens) == 1 and max(lens) == 40
    dm = fg.damaged()
    first = dm.expect()["item_first"]
    assert all(first[k] == first[k + 1] for k in fg.DAMAGED_AT) and first[-1] > 50
    assert [k for k in range(300) if dm.index.item_first[k] == dm.index.item_first[k + 1]] == list(fg.DAMAGED_AT)


def test_the_first_hit_numbers_pass_2_to_the_24():
    """7: 300 items of 2^16 hits each: item 256 starts at hit 2^24 -- the first lane of the second pass over the groups --; with the
    long item in front, the block whose first hit is number 2^24 is block 192, lane 0 of the fourth wavefront"""
    for front in (False, True):
        case = fg.carries(front)
        e = case.expect(0, fg.CARRY_CAP)
        first, idx = e["item_first"], case.index
        assert e["status"] == ERR_OVERFLOW and e["need"] == [idx.total] and len(e["offsets"]) == fg.CARRY_CAP
        crossing = next(b for b, v in enumerate(idx.out_start[:-1]) if v >= fg.SPLIT)
        assert idx.out_start[crossing] == fg.SPLIT and crossing == (192 if front else 256)
        item = crossing - 1 if front else crossing
        assert idx.item_first[item] == crossing and first[item] == fg.SPLIT and first[-1] == idx.total > fg.SPLIT
        assert library_plan(case, 0, fg.CARRY_CAP) == restated(e), case.name


def test_plan_find_is_restated():
    for case in fg.healthy_cases():
        for flags in fg.FLAGS:
            assert library_plan(case, flags) == restated(case.expect(flags)), (case.name, flags)
        for what, cap in fg.caps(case):
            e = case.expect(fg.FLAT, cap)
            assert library_plan(case, fg.FLAT, cap) == restated(e), (case.name, what)
            assert len(e["offsets"]) == min(cap, e["need"][0]) and e["need"] == case.expect()["need"]


def test_the_rule_in_small():
    """the header's clauses one by one, on bytes written out here"""
    def hits(text, needle, at=None, status=None, **kw):
        items, offsets, first, need = tsq.plan_find(text, at or [0, len(text)], needle, status, **kw)
        return list(zip(items.tolist(), offsets.tolist())), first.tolist(), need
    assert hits(b"aaa", b"aa") == ([(0, 0), (0, 1)], [0, 2], 2)                       # overlapping hits all count
    assert hits(b"abcabc", b"bc") == ([(0, 1), (0, 4)], [0, 2], 2)
    assert hits(b"abc", b"abcd") == ([], [0, 0], 0) and hits(b"", b"a") == ([], [0, 0], 0)
    assert hits(b"abc", b"c") == ([(0, 2)], [0, 1], 1) and hits(b"x" * 16, b"x" * 16) == ([(0, 0)], [0, 1], 1)
    # items: no hit runs from one into the next; a refused item has none; flat offsets count from the whole data
    text, at = b"xab" b"abab" b"" b"ab", [0, 3, 7, 7, 9]
    assert hits(text, b"ab", at) == ([(0, 1), (1, 0), (1, 2), (3, 0)], [0, 1, 3, 3, 4], 4)
    assert hits(text, b"ba", at) == ([(1, 1)], [0, 0, 1, 1, 1], 1)                   # not the one across items 0 | 1, nor 1 | 3
    assert hits(text, b"ab", at, [0, 4, 0, 0], flat=True) == ([(0, 1), (3, 7)], [0, 1, 1, 1, 2], 2)
    # the prefix: nothing at or past cap_hits is written
    L = tsq.lib()
    buf, at8, nd = np.frombuffer(b"ababab", dtype=np.uint8), np.array([0, 6], dtype=np.uint64), np.frombuffer(b"ab", dtype=np.uint8)
    offs, its = np.full(6, 77, dtype=np.uint64), np.full(6, 77, dtype=np.uint32)
    first, need = np.zeros(2, dtype=np.uint64), np.full(2, 55, dtype=np.uint64)
    assert L.tsqa_plan_find(buf.ctypes.data, at8.ctypes.data, None, 1, nd.ctypes.data, 2, 0, 2, its.ctypes.data, offs.ctypes.data,
                            first.ctypes.data, need.ctypes.data) == OK
    assert offs.tolist() == [0, 2, 77, 77, 77, 77] and its.tolist() == [0, 0, 77, 77, 77, 77]
    assert first.tolist() == [0, 3] and need.tolist() == [3, 55], "need is ONE word"


def test_the_host_rule_refuses_bad_arguments():
    L = tsq.lib()
    buf, at, nd = np.frombuffer(b"abab", dtype=np.uint8), np.array([0, 4], dtype=np.uint64), np.frombuffer(b"ab" * 9, dtype=np.uint8)
    t = [np.zeros(4, dtype=np.uint64) for _ in range(3)]
    its = np.zeros(4, dtype=np.uint32)
    good = dict(data=buf.ctypes.data, at=at.ctypes.data, n=1, needle=nd.ctypes.data, m=2, flags=0, cap=4, items=its.ctypes.data, offs=t[0].ctypes.data,
                first=t[1].ctypes.data, need=t[2].ctypes.data)
    call = lambda **kw: (lambda a: L.tsqa_plan_find(a["data"], a["at"], None, a["n"], a["needle"], a["m"], a["flags"], a["cap"], a["items"], a["offs"],
                                                    a["first"], a["need"]))({**good, **kw})
    assert call() == OK and call(items=None) == OK and call(cap=0, offs=None) == OK and call(flags=2) == OK and call(m=16) == OK and call(m=1) == OK
    for what, kw in (("null item_at", dict(at=None)), ("null first", dict(first=None)), ("null need", dict(need=None)), ("null needle", dict(needle=None)),
                     ("m 0", dict(m=0)), ("m 17", dict(m=17)), ("unknown flags", dict(flags=1)), ("unknown flags", dict(flags=4)),
                     ("null offsets", dict(offs=None)), ("no items", dict(n=0)), ("null data", dict(data=None)),
                     ("unordered", dict(at=np.array([4, 0], dtype=np.uint64).ctypes.data))):
        assert call(**kw) == ERR_ARG, what
    with pytest.raises(tsq.TsqError) as err:
        tsq.plan_find(b"abc", [0, 3], b"")
    assert err.value.code == ERR_ARG


def test_a_one_byte_needle_finds_the_records_terminators():
    """10, on the host: the hits of [delim] are offset + length - 1 of every terminated record with keep_delim on"""
    for rcase in (rg.places(10), rg.chunk_edges("text")):
        hits = fg.restate(rcase.index, bytes([rcase.delim]), fg.FLAT)
        recs = rcase.expect(rg.KEEP_DELIM | rg.FLAT)
        src = np.frombuffer(rcase.index.data, dtype=np.uint8)
        ends = recs["offsets"] + recs["lengths"] - 1
        terminated = recs["lengths"] > 0
        terminated[terminated] = src[ends[terminated]] == rcase.delim
        assert hits["offsets"].tolist() == ends[terminated].tolist() and hits["need"][0] > 0
