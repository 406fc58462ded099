"""CPU-only: recordgen's restatement against the host-only rule (tsqa_plan_records), the host frame walk (tsqa_walk_frames), the
oracle and the gather's host planners, and that each of its cases reaches what it aims at.  The kernels' side of the same cases:
test_gpu_records.py."""
import os

import numpy as np
import pytest

import gathergen as gg
import recordgen as rc_gen
import turbosqueeze_amd as tsq
from test_cut_cpu import host_walk

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = rc_gen.OK, rc_gen.ERR_ARG, rc_gen.ERR_FORMAT, rc_gen.ERR_OVERFLOW


def library_plan(case, flags=0, cap=None):
    """tsqa_plan_records on a case's decoded bytes -> (items, offsets, lengths, item_first, need) as lists"""
    items, offsets, lengths, first, need = tsq.plan_records(case.index.data, case.item_at(), case.item_status(), case.delim,
                                                            keep_delim=bool(flags & rc_gen.KEEP_DELIM), flat=bool(flags & rc_gen.FLAT), cap_records=cap)
    return items.tolist(), offsets.tolist(), lengths.tolist(), first.tolist(), need


def restated(e):
    return e["items"].tolist(), e["offsets"].tolist(), e["lengths"].tolist(), e["item_first"], e["need"]


def test_the_symbols_are_there():
    for name in ("tsqa_plan_records", "tsqa_records_async", "tsqa_records", "tsqa_profile_read_records"):
        assert hasattr(tsq.lib(), name), name
    assert (tsq.RECORDS_KEEP_DELIM, tsq.RECORDS_FLAT) == (rc_gen.KEEP_DELIM, rc_gen.FLAT) == (1, 2)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "turbosqueeze_amd.h")) as f:
        header = f.read()
    assert "#define TSQA_RECORDS_KEEP_DELIM 1u" in header and "#define TSQA_RECORDS_FLAT 2u" in header
    for name in ("RangeIndex", "SizedIndex", "BatchIndex", "DeviceBatchIndex"):
        assert hasattr(getattr(tsq, name), "records"), name
    assert hasattr(tsq.DeviceCodec, "records_async") and hasattr(tsq.DeviceCodec, "profile_read_records")
    assert hasattr(tsq.RecordTable, "gather_rows") and callable(tsq.plan_records)


def test_the_sources_are_what_the_oracle_and_the_walk_say(oracle):
    """the records are found in `data` and numbered by `item_first`: both are the containers' own"""
    singles = [rc_gen.chunk_edges(k) for k in rc_gen.CHUNK_KINDS] + [rc_gen.ring_wrap(), rc_gen.two_blocks(), rc_gen.tiny()]
    for case in singles:
        idx = case.index
        rc, nb, total, _, _, out_len = host_walk(idx.blob)
        assert rc == 0 and nb == idx.n_blocks and total == idx.total, case.name
        assert [int(x) for x in np.cumsum([0] + out_len)] == idx.out_start, case.name
        assert bytes(oracle.decompress(idx.blob)) == idx.data, case.name
    for case in [rc_gen.places(d) for d in rc_gen.DELIMS] + [rc_gen.ragged(257), rc_gen.damaged(), rc_gen.cut_items(), rc_gen.ring_wrap_skewed()]:
        idx, blocks, cat = case.index, 0, b""
        refused_at = rc_gen.DAMAGED_AT if case is rc_gen.damaged() else tuple(rc_gen.CUT_AT) if case is rc_gen.cut_items() else ()
        for k, (o, n) in enumerate(idx.spans):
            rc, nb, total, _, _, out_len = host_walk(idx.blob[o:o + n])
            owned = idx.item_first[k + 1] - idx.item_first[k]
            if rc != 0 or not owned:
                assert not owned and (rc != 0 or k in rc_gen.DAMAGED_AT), (case.name, k, rc)
                assert k in refused_at, (case.name, k)
                continue
            assert k not in refused_at or case is rc_gen.damaged(), (case.name, k)
            assert nb == owned and total == idx.item_span(k)[1], (case.name, k)
            cat += bytes(oracle.decompress(idx.blob[o:o + n]))
            blocks += nb
        assert blocks == idx.n_blocks and cat == idx.data, case.name


def test_each_case_reaches_its_aim():
    # 1: every length with the delimiter at byte 0, at the last byte, at both, nowhere and everywhere, for three byte values
    for d in rc_gen.DELIMS:
        case = rc_gen.places(d)
        idx, e = case.index, case.expect()
        assert idx.n_items == len(rc_gen.ITEM_LENGTHS) * len(rc_gen.PLACES)
        data = np.frombuffer(idx.data, dtype=np.uint8)
        for k in range(idx.n_items):
            n, where = rc_gen.ITEM_LENGTHS[k // 5], rc_gen.PLACES[k % 5]
            a, t = idx.item_span(k)
            hits = np.flatnonzero(data[a:a + t] == d).tolist()
            assert t == n and hits == {"first": [0], "last": [n - 1], "both": sorted({0, n - 1}), "nowhere": [], "everywhere": list(range(n))}[where]
            count = e["item_first"][k + 1] - e["item_first"][k]
            assert count == {"first": 2 if n > 1 else 1, "last": 1, "both": 2 if n > 1 else 1, "nowhere": 1, "everywhere": n}[where], (d, k)
    # 2: many blocks inside one 64-position span of the concatenation
    for case in [rc_gen.ragged(n) for n in rc_gen.COUNTS] + [rc_gen.tiny()]:
        starts = case.index.out_start
        per_span = np.bincount(np.array(starts[:-1]) >> 6)
        assert case.index.n_blocks == 1 or per_span.max() >= 2, case.name
    assert np.bincount(np.array(rc_gen.ragged(513).index.out_start[:-1]) >> 6).max() >= 5
    assert [rc_gen.ragged(n).index.n_items for n in rc_gen.COUNTS] == [1, 2, 255, 256, 257, 513]
    # 3: more than three chunks, and delimiters on the first and last byte of every chunk.  The decoder's chunking depends on the
    # stream (a chunk ends where 6 144 stream bytes or 12 288 output bytes do), and the oracle gives no trace of it: the case of
    # zeros with delim 0 covers it, since EVERY byte is a delimiter wherever the chunks end.
    zeros = rc_gen.chunk_edges("zeros")
    assert zeros.expect()["need"] == [rc_gen.CHUNK_N, 0] and zeros.index.total == 3 * rc_gen.OUTC + 5
    assert zeros.expect(rc_gen.KEEP_DELIM)["need"] == [rc_gen.CHUNK_N, 1]
    for kind in rc_gen.CHUNK_KINDS:
        case = rc_gen.chunk_edges(kind)
        assert case.index.total == rc_gen.CHUNK_N and case.index.n_blocks == 1
        if kind != "random_drawn":
            assert case.expect()["need"][0] > 1, kind
    # 4: delimiters around every place where the ring wraps, and around 2^16; a record across the edge of two blocks
    ring = rc_gen.ring_wrap()
    data = np.frombuffer(ring.index.data, dtype=np.uint8)
    assert np.flatnonzero(data == 10).tolist() == rc_gen.RING_DELIMS and ring.index.n_blocks == 1 and ring.index.total == 1 << 18
    assert all(k * rc_gen.RING + d in rc_gen.RING_DELIMS for k in (1, 2, 3) for d in (-1, 0, 1)) and 3 * rc_gen.RING + 1 < 1 << 18
    two = rc_gen.two_blocks()
    e = two.expect()
    assert two.index.out_start == [0, rc_gen.BLOCK, rc_gen.BLOCK + 1]
    last = e["offsets"][-1], e["lengths"][-1]
    assert last[0] < rc_gen.BLOCK and last[0] + last[1] == rc_gen.BLOCK + 1, "the last record runs across the block edge"
    # 5: 257 blocks of 4 096 bytes, both kinds of index over one container
    assert rc_gen.short_blocks("sized").index.blob == rc_gen.short_blocks("plain").index.blob
    assert restated(rc_gen.short_blocks("sized").expect()) == restated(rc_gen.short_blocks("plain").expect())
    # 7: the refused items give no records, and they are items 0, 256 and the last among others
    dm = rc_gen.damaged()
    first = dm.expect()["item_first"]
    assert [k for k in range(dm.index.n_items) if dm.index.item_first[k] == dm.index.item_first[k + 1]] == list(rc_gen.DAMAGED_AT)
    assert all(first[k] == first[k + 1] for k in rc_gen.DAMAGED_AT) and all(first[k] < first[k + 1] for k in range(300) if k not in rc_gen.DAMAGED_AT)


def test_the_cut_containers_are_refused_by_the_walk_alone(oracle):
    """mtgen's cut containers as items 0, 100, 256 and 299 of 300: each has a whole header that states a count its bytes could hold
    and a total its blocks could hold -- what the header rule asks --, the host walk refuses exactly these four items, the oracle
    refuses them too, and they give no records while every other item has its own"""
    case = rc_gen.cut_items()
    idx = case.index
    assert sorted(rc_gen.CUT_AT) == [0, 100, 256, 299] and set(rc_gen.CUT_AT.values()) == {"cut_in_frame_word", "cut_in_size_word", "cut_mid_stream", "cut_at_frame_end"}
    refused = []
    for k, (o, n) in enumerate(idx.spans):
        blob = idx.blob[o:o + n]
        if host_walk(blob)[0] != 0:
            refused.append(k)
            count, total = int.from_bytes(blob[4:8], "little"), int.from_bytes(blob[8:16], "little")
            assert blob[:4] == b"TSQ1" and 1 <= count <= (n - 16) // 6 and total <= count * rc_gen.BLOCK, (k, "the header alone is accepted")
            assert oracle.decompress(blob, threads=1) is None, k
    assert refused == sorted(rc_gen.CUT_AT)
    first = case.expect()["item_first"]
    assert all((first[k] == first[k + 1]) == (k in rc_gen.CUT_AT) for k in range(300))
    assert case.item_status() == [rc_gen.ERR_FORMAT if k in rc_gen.CUT_AT else 0 for k in range(300)]


def test_the_flipped_byte_and_the_twins_are_refused_by_the_oracles_decoder(oracle):
    """one byte flipped inside the stream of a container whose header and frame word stay whole: the walk accepts it, the oracle's
    decoder refuses it.  The same holds of mtgen's stream twins, which test_gpu_records.py runs beside it: damage in block 0, 2, 3
    and 5 of six"""
    import mtgen
    name, bad, at = rc_gen.flipped()
    good = rc_gen.chunk_edges("text").index.blob
    assert len(bad) == len(good) and [k for k in range(len(good)) if good[k] != bad[k]] == [at] and at >= 16 + 3 + 3, "inside the stream, behind its length"
    rc, nb, total, _, sizes, _ = host_walk(bad)
    assert rc == 0 and nb == 1 and total == rc_gen.CHUNK_N and at < 19 + sizes[0]
    assert oracle.decompress(bad, threads=1) is None and bytes(oracle.decompress(good, threads=1)) == rc_gen.chunk_edges("text").index.data
    twins = [t for t in mtgen.twin_containers() if t[3] == "stream"][:4]
    assert sorted(k for _, _, k, _ in twins) == [0, 2, 3, 5]
    for _, blob, _, _ in twins:
        assert host_walk(blob)[0] == 0 and oracle.decompress(blob, threads=1) is None


def test_the_ring_wraps_at_a_skew(oracle):
    """the two long blocks of ring_wrap_skewed start at 1 and 38 mod 64 of the concatenation, are longer than the ring, and carry
    their delimiters where the skewed ring address is R - 1, 0 and 1"""
    case = rc_gen.ring_wrap_skewed()
    idx = case.index
    data = np.frombuffer(idx.data, dtype=np.uint8)
    assert idx.n_blocks == 4 and [idx.out_start[1] % 64, idx.out_start[3] % 64] == [1, 38]
    for b in (1, 3):
        a, n = idx.out_start[b], idx.out_start[b + 1] - idx.out_start[b]
        hits = np.flatnonzero(data[a:a + n] == 10)
        assert n > 2 * rc_gen.RING and hits.tolist() == rc_gen.skew_delims(a, n)
        assert {int((p + a % 64) % rc_gen.RING) for p in hits} >= {rc_gen.RING - 1, 0, 1}
    assert not (data[:1] == 10).any() and not (data[idx.out_start[2]:idx.out_start[3]] == 10).any()


def test_the_first_record_numbers_pass_2_to_the_24():
    """300 items of 2^16 records each: item 256 starts at record 2^24; with the long item in front, the block whose first record
    is number 2^24 is block 192 -- lane 0 of the fourth wavefront of the first group"""
    for front in (False, True):
        case = rc_gen.carries(front)
        e = case.expect(0, rc_gen.CARRY_CAP)
        first, idx = e["item_first"], case.index
        assert e["status"] == ERR_OVERFLOW and e["need"] == [idx.total, 0] and len(e["offsets"]) == rc_gen.CARRY_CAP
        block_first = idx.out_start[:-1]                     # a block of zeros holds as many records as it has bytes
        crossing = next(b for b, v in enumerate(block_first) if v >= rc_gen.SPLIT)
        assert block_first[crossing] == rc_gen.SPLIT and crossing == (192 if front else 256)
        item = crossing - 1 if front else crossing           # (the item in front owns two blocks)
        assert idx.item_first[item] == crossing and first[item] == rc_gen.SPLIT and first[-1] == idx.total
        assert e["offsets"].tolist() == list(range(rc_gen.CARRY_CAP)) and e["items"].tolist() == [0] * rc_gen.CARRY_CAP


def test_plan_records_is_restated():
    for case in rc_gen.healthy_cases():
        for flags in rc_gen.FLAGS:
            e = case.expect(flags)
            assert library_plan(case, flags) == restated(e), (case.name, flags)
        for what, cap in rc_gen.caps(case):
            for flags in (0, rc_gen.KEEP_DELIM | rc_gen.FLAT):
                e = case.expect(flags, cap)
                assert library_plan(case, flags, cap) == restated(e), (case.name, what, flags)
                assert len(e["offsets"]) == min(cap, e["need"][0]) and e["need"] == case.expect(flags)["need"]
    for front in (False, True):
        case = rc_gen.carries(front)
        assert library_plan(case, 0, rc_gen.CARRY_CAP) == restated(case.expect(0, rc_gen.CARRY_CAP)), case.name


def test_the_rule_in_small():
    """the header's clauses one by one, on bytes written out here"""
    def records(text, **kw):
        items, offsets, lengths, first, need = tsq.plan_records(text, [0, len(text)], None, ord("\n"), **kw)
        return list(zip(offsets.tolist(), lengths.tolist())), first.tolist(), need
    assert records(b"ab\ncd") == ([(0, 2), (3, 2)], [0, 2], [2, 2])                  # the last record needs no terminator
    assert records(b"ab\ncd\n") == ([(0, 2), (3, 2)], [0, 2], [2, 2])                # a terminator at the last byte starts no record
    assert records(b"\n") == ([(0, 0)], [0, 1], [1, 0])
    assert records(b"a\n\nb") == ([(0, 1), (2, 0), (3, 1)], [0, 3], [3, 1])          # two delimiters side by side: a record of length 0
    assert records(b"a\n\nb", keep_delim=True) == ([(0, 2), (2, 1), (3, 1)], [0, 3], [3, 2])
    assert records(b"") == ([], [0, 0], [0, 0])
    # items: no record crosses one; a refused item and an empty one have none; flat offsets count from the whole data
    text, at = b"a\nbc" b"de\nf" b"" b"\n\n", [0, 4, 8, 8, 10]
    items, offsets, lengths, first, need = tsq.plan_records(text, at, [0, 0, 0, 0], 10)
    assert (items.tolist(), offsets.tolist(), lengths.tolist()) == ([0, 0, 1, 1, 3, 3], [0, 2, 0, 3, 0, 1], [1, 2, 2, 1, 0, 0])
    assert first.tolist() == [0, 2, 4, 4, 6] and need == [6, 2]
    items, offsets, lengths, first, need = tsq.plan_records(text, at, [0, 4, 0, 0], 10, flat=True)
    assert (items.tolist(), offsets.tolist(), first.tolist()) == ([0, 0, 3, 3], [0, 2, 8, 9], [0, 2, 2, 2, 4])
    # the prefix: nothing at or past cap_records is written
    L = tsq.lib()
    buf, at8 = np.frombuffer(b"a\nb\nc\nd", dtype=np.uint8), np.array([0, 7], dtype=np.uint64)
    offs, lens, its = (np.full(6, 77, dtype=np.uint64), np.full(6, 77, dtype=np.uint64), np.full(6, 77, dtype=np.uint32))
    first, need = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    assert L.tsqa_plan_records(buf.ctypes.data, at8.ctypes.data, None, 1, 10, 0, 2, its.ctypes.data, offs.ctypes.data, lens.ctypes.data,
                               first.ctypes.data, need.ctypes.data) == OK
    assert offs.tolist() == [0, 2, 77, 77, 77, 77] and lens.tolist() == [1, 1, 77, 77, 77, 77] and its.tolist() == [0, 0, 77, 77, 77, 77]
    assert first.tolist() == [0, 4] and need.tolist() == [4, 1]


def test_the_host_rule_refuses_bad_arguments():
    L = tsq.lib()
    buf, at = np.frombuffer(b"a\nb", dtype=np.uint8), np.array([0, 3], dtype=np.uint64)
    t = [np.zeros(4, dtype=np.uint64) for _ in range(4)]
    its = np.zeros(4, dtype=np.uint32)
    good = dict(data=buf.ctypes.data, at=at.ctypes.data, n=1, delim=10, flags=0, cap=4, items=its.ctypes.data, offs=t[0].ctypes.data,
                lens=t[1].ctypes.data, first=t[2].ctypes.data, need=t[3].ctypes.data)
    call = lambda **kw: (lambda a: L.tsqa_plan_records(a["data"], a["at"], None, a["n"], a["delim"], a["flags"], a["cap"], a["items"], a["offs"],
                                                       a["lens"], a["first"], a["need"]))({**good, **kw})
    assert call() == OK and call(items=None) == OK and call(cap=0, offs=None, lens=None) == OK and call(flags=3) == OK and call(delim=255) == OK
    for what, kw in (("null item_at", dict(at=None)), ("null first", dict(first=None)), ("null need", dict(need=None)), ("delim 256", dict(delim=256)),
                     ("unknown flags", dict(flags=4)), ("null offsets", dict(offs=None)), ("null lengths", dict(lens=None)), ("no items", dict(n=0)),
                     ("null data", dict(data=None)), ("unordered", dict(at=np.array([3, 0], dtype=np.uint64).ctypes.data))):
        assert call(**kw) == ERR_ARG, what


def test_the_tables_drive_the_gather_planners():
    """every record is an accepted range of tsqa_plan_gather, by item and flat; the rows at stride need[1] truncate nothing, and at
    need[1] - 1 a row overflows"""
    for case in (rc_gen.places(10), rc_gen.ragged(257), rc_gen.tiny(), rc_gen.short_blocks("sized"), rc_gen.damaged(), rc_gen.chunk_edges("text")):
        idx = case.index
        for flags in (rc_gen.KEEP_DELIM, rc_gen.KEEP_DELIM | rc_gen.FLAT):
            e = case.expect(flags)
            items = None if flags & rc_gen.FLAT else e["items"].tolist()
            offsets, lengths, longest = e["offsets"].tolist(), e["lengths"].tolist(), e["need"][1]
            _, status, _, _ = tsq.plan_gather(idx.out_start, idx.item_first, items, offsets, lengths)
            assert status == [OK] * len(offsets), (case.name, flags)
            row_lengths, row_status, need, _ = tsq.plan_gather_rows(idx.out_start, idx.item_first, items, offsets, lengths, longest)
            assert row_status == [OK] * len(offsets) and row_lengths == lengths and need[1] == longest, (case.name, flags)
            if longest > 1:
                _, row_status, _, _ = tsq.plan_gather_rows(idx.out_start, idx.item_first, items, offsets, lengths, longest - 1)
                assert row_status.count(ERR_OVERFLOW) == lengths.count(longest) >= 1, (case.name, flags)
            # and the records are the data cut at the delimiters: joined with them they give every item back
            src = np.frombuffer(idx.data, dtype=np.uint8)
            if flags & rc_gen.FLAT:
                got = b"".join(src[o:o + n].tobytes() for o, n in zip(offsets, lengths))
                assert got == idx.data, case.name
