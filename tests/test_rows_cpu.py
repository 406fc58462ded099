"""CPU-only: rowsgen's restatement against the host-only planner (tsqa_plan_gather_rows), the host frame walk (tsqa_walk_frames) and
the oracle, and that each of its cases reaches what it aims at.  The kernels' side of the same cases: test_gpu_rows.py."""
import ctypes as C
import os

import numpy as np
import pytest

import gathergen as gg
import rowsgen as rg
import turbosqueeze_amd as tsq
from test_cut_cpu import host_walk

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = rg.OK, rg.ERR_ARG, rg.ERR_FORMAT, rg.ERR_OVERFLOW


def library_plan(case, cap_pieces=None):
    """tsqa_plan_gather_rows on a case's index tables -> (row_lengths, row_status, need, n_groups)"""
    i = case.index
    return tsq.plan_gather_rows(i.out_start, i.item_first, case.items, case.offsets, case.lengths, case.stride, case.truncate, cap_pieces, n_rows=case.n)


def restated(e):
    return e["row_lengths"], e["row_status"], e["need"], e["groups"]


def test_the_symbols_are_there():
    for name in ("tsqa_plan_gather_rows", "tsqa_gather_rows_async", "tsqa_gather_rows", "tsqa_profile_read_rows"):
        assert hasattr(tsq.lib(), name), name
    assert tsq.api.ROWS_TRUNCATE == rg.TRUNCATE == 1
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "turbosqueeze_amd.h")) as f:
        header = f.read()
    assert "#define TSQA_ROWS_TRUNCATE 1u" in header
    for name in ("RangeIndex", "BatchIndex"):
        assert hasattr(getattr(tsq.api, name), "gather_rows"), name
    assert hasattr(tsq.DeviceCodec, "gather_rows_async")


def test_the_sources_are_what_the_oracle_and_the_walk_say(oracle):
    """the rows' bytes are slices of `data`, and the pieces are cut at `out_start`: both are the containers' own"""
    for idx in (gg.tiny(), gg.split("sized"), gg.split("plain")):
        rc, nb, total, _, _, out_len = host_walk(idx.blob)
        assert rc == 0 and nb == idx.n_blocks and total == idx.total
        assert [int(x) for x in np.cumsum([0] + out_len)] == idx.out_start
        assert bytes(oracle.decompress(idx.blob)) == idx.data
    assert gg.split("sized").out_start[:-1] == [b * 4096 for b in range(257)]


def test_plan_gather_rows_is_restated():
    for case in rg.healthy_cases():
        e = case.expect()
        assert library_plan(case) == restated(e), case.name
        for cap in {e["need"][0], max(e["need"][0] - 1, 1), max(e["need"][0] // 2, 1), 1}:
            assert library_plan(case, cap) == restated(case.expect(cap)), (case.name, cap)
    for what, case, cap in rg.rooms():
        assert library_plan(case, cap) == restated(case.expect(cap)), what


def test_the_planner_refuses_what_the_call_refuses():
    c = rg.too_long()
    i = c.index
    for kw in (dict(row_stride=0), dict(cap_pieces=0)):
        a = dict(row_stride=c.stride, cap_pieces=None)
        a.update(kw)
        with pytest.raises(tsq.TsqError) as err:
            tsq.plan_gather_rows(i.out_start, i.item_first, None, c.offsets, c.lengths, a["row_stride"], False, a["cap_pieces"])
        assert err.value.code == ERR_ARG
    L = tsq.lib()
    starts, first = np.array(i.out_start, dtype=np.uint64), np.array(i.item_first, dtype=np.uint64)
    tables = [np.zeros(4, dtype=np.uint64) for _ in range(3)]
    status, groups = np.zeros(4, dtype=np.int32), np.zeros(1, dtype=np.uint32)
    call = lambda n, stride, flags: L.tsqa_plan_gather_rows(starts.ctypes.data, i.n_blocks, first.ctypes.data, 1, None, tables[0].ctypes.data, None, n, stride,
                                                           flags, 1, tables[1].ctypes.data, status.ctypes.data, tables[2].ctypes.data,
                                                           groups.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert call(4, 40, 0) == OK and call(4, 40, 1) == OK
    assert call(4, 40, 2) == ERR_ARG, "unknown flags"
    assert call(4, (1 << 55) // 4, 0) == ERR_ARG, "n_rows * (row_stride + 4096) >= 2^55"
    assert call(4, (1 << 55) // 4 - 4097, 0) == OK


def test_without_truncation_the_pieces_are_the_gather_s_at_k_times_the_stride():
    """the accepted rows of a case with every table and no truncation, as a gathergen case of the same ranges with the too-long
    ones taken out: the same pieces, block by block, and each at k * stride where the dense layout has its prefix sum"""
    n = 0
    for case in rg.healthy_cases():
        if case.truncate or case.offsets is None or case.lengths is None:
            continue
        e = case.expect()
        keep = [k for k in range(case.n) if e["row_status"][k] != ERR_OVERFLOW]
        dense = gg.Case(case.name, case.index, [case.offsets[k] for k in keep], [case.lengths[k] for k in keep],
                        items=None if case.items is None else [case.items[k] for k in keep])
        d = dense.expect()
        assert d["range_status"] == [e["row_status"][k] for k in keep], case.name
        assert d["need_pieces"] == e["need"][0] and len(d["groups"]) == e["groups"], case.name
        cuts = [gg.cut(case.index.out_start, *d["places"][j]) for j in range(len(keep))]
        assert sorted(d["items"]) == sorted((b, lo, hi, d["out_offsets"][j] + delta) for j, c in enumerate(cuts) for b, lo, hi, delta in c), case.name
        want = sorted((b, lo, hi, keep[j] * case.stride + delta) for j, c in enumerate(cuts) for b, lo, hi, delta in c)
        assert sorted(p for row in e["pieces"] for p in row) == want, case.name
        n += 1
    assert n >= 20


def test_the_counts_and_the_second_scan_pass():
    assert [c.n for c in rg.counts()] == list(rg.COUNTS)
    for c in rg.counts():
        e = c.expect()
        assert e["status"] == OK and e["row_lengths"] == c.lengths and max(c.lengths) == c.stride == e["need"][1]
    e = rg.counts()[-1].expect()
    sums = [sum(len(p) for p in e["pieces"][g:g + rg.GROUP]) for g in range(0, 513, rg.GROUP)]
    assert len(sums) == 3 and all(s > 0 for s in sums), "the piece sum does not cross a group"
    assert any(len(p) >= 8 for p in e["pieces"]) and e["row_lengths"].count(0) >= 20
    for n in rg.REPEATS:
        c = rg.repeated(n)
        e = c.expect()
        groups = (n + rg.GROUP - 1) // rg.GROUP
        assert (groups > rg.GROUP) == (n == 65537), "the group scan's second pass starts with group 256"
        assert e["status"] == OK and e["need"][0] > n and e["need"][1] == c.stride
        per_group = {sum(len(p) for p in e["pieces"][g:g + rg.GROUP]) for g in range(0, n - rg.GROUP, rg.GROUP)}
        assert len(per_group) > 1, "every group sums to the same"
    last = rg.repeated(65537).expect()
    assert len(last["pieces"][65536]) >= 1 and last["row_lengths"][65536] > 0, "the row of the second pass has nothing to place"


def test_the_strides_reach_the_words_and_the_edges():
    assert set(rg.STRIDES) >= {1, 15, 16, 17, 40, 200, 4097}
    for stride in rg.STRIDES:
        plain, cut = rg.strided(stride, False), rg.strided(stride, True)
        starts = plain.index.out_start
        assert {0, 1, stride - 1, stride, stride + 1} <= set(plain.lengths)
        e, t = plain.expect(), cut.expect()
        long_rows = [k for k in range(plain.n) if plain.lengths[k] == stride + 1]
        assert all(e["row_status"][k] == ERR_OVERFLOW and e["row_lengths"][k] == 0 for k in long_rows)
        assert all(t["row_status"][k] == OK and t["row_lengths"][k] == stride for k in long_rows)
        assert e["need"][1] == t["need"][1] == stride + 1 and e["status"] == ERR_OVERFLOW and t["status"] == OK
        assert any(e["row_status"][k] == OK and e["row_lengths"][k] for k in range(long_rows[0] + 1, plain.n)), "no row is delivered behind a too-long one"
        on_edge, past_edge = rg.EDGE_ROWS
        assert cut.offsets[on_edge] + stride in starts, "the truncation does not end on a block edge"
        assert cut.offsets[past_edge] + stride - 1 in starts, "the truncation does not end one byte past a block edge"
        whole = gg.cut(starts, cut.offsets[on_edge], stride + 1)
        assert len(t["pieces"][on_edge]) == len(whole) - 1, "the truncated row drops no piece"
        assert len(t["pieces"][past_edge]) == len(gg.cut(starts, cut.offsets[past_edge], stride + 1))
        assert t["pieces"][past_edge][-1][2] - t["pieces"][past_edge][-1][1] == 1, "the last piece is not the one byte past the edge"
        # the words of the pad kernel: rows per 16-byte word, for every residue of the output's address
        for skew in rg.RESIDUES:
            per_word = {}
            for k in range(plain.n):
                for w in range((skew + k * stride) // rg.WORD, (skew + (k + 1) * stride - 1) // rg.WORD + 1):
                    per_word.setdefault(w, set()).add(k)
            most = max(len(v) for v in per_word.values())
            want = {1: 16, 5: 4, 15: 2}.get(stride, 1 if stride % 16 == 0 and skew == 0 else 2)
            assert most == want, (stride, skew, most)
    five = rg.strided(5, False)
    assert any(len({(o // 5) for o in range(w * 16, w * 16 + 16)}) >= 3 for w in range(five.n * 5 // 16)), "no word holds three rows at stride 5"
    # a word that holds data of one row and padding of the next: the bytewise path is taken for pad bytes too
    e = rg.strided(17, False).expect()
    assert any(0 < e["row_lengths"][k] < 17 and e["row_lengths"][k + 1] < 17 for k in range(36))


def test_the_null_tables_mean_what_the_header_says():
    by_name = {c.name: c for c in rg.null_tables()}
    tiny = gg.tiny()
    c = by_name["rows_lengths_null_truncate"]
    e = c.expect()
    assert c.lengths is None and c.items is None
    assert e["row_lengths"] == [40, 40, 40, 40, 39, 1, 0, 0, 0, 40]
    assert e["row_status"] == [OK] * 7 + [ERR_ARG, ERR_ARG, OK] and e["need"][1] == tiny.total
    assert bytes(c.rows(e)[4]) == tiny.data[-39:] and bytes(c.rows(e)[0]) == tiny.data[:40]
    e = by_name["rows_lengths_null"].expect()
    assert e["row_status"] == [ERR_OVERFLOW] * 3 + [OK] * 4 + [ERR_ARG, ERR_ARG, ERR_OVERFLOW]
    c = by_name["rows_offsets_null"]
    e = c.expect()
    assert c.offsets is None and e["row_status"] == [OK] * 4 + [ERR_OVERFLOW] * 2 + [ERR_ARG] * 2 + [OK]
    assert all(bytes(r) == tiny.data[:len(r)] for r in c.rows(e))
    e = by_name["rows_offsets_null_truncate"].expect()
    assert e["row_lengths"] == [0, 1, 39, 40, 40, 40, 0, 0, 17]
    batch = gg.batch()
    c = by_name["rows_whole_items"]
    e = c.expect()
    assert c.offsets is None and c.lengths is None and c.n == gg.BATCH_ITEMS + 4
    for i in range(gg.BATCH_ITEMS):
        if i in gg.BATCH_DAMAGE:
            assert e["row_status"][i] == ERR_ARG
            continue
        start, total = batch.item_span(i)
        assert e["row_status"][i] == (OK if total <= 4096 else ERR_OVERFLOW)
        if total <= 4096:
            assert bytes(c.rows(e)[i]) == batch.data[start:start + total]
    assert e["row_status"][gg.BATCH_ITEMS:gg.BATCH_ITEMS + 2] == [ERR_ARG, ERR_ARG]
    too_long = [i for i in range(gg.BATCH_ITEMS) if e["row_status"][i] == ERR_OVERFLOW]
    assert len(too_long) >= 30 and all(e["row_status"][i + 1] == OK for i in too_long if i + 1 not in gg.BATCH_DAMAGE), "nothing is delivered behind a too-long row"
    t = by_name["rows_whole_items_truncate"].expect()
    assert all(t["row_status"][i] == OK and t["row_lengths"][i] == 4096 and len(t["pieces"][i]) == 1 for i in too_long), "a truncated item is not one block"
    assert t["need"][1] == e["need"][1] == max(batch.item_span(i)[1] for i in range(gg.BATCH_ITEMS) if i not in gg.BATCH_DAMAGE) > 8192


def test_the_refusals_the_too_long_rows_and_the_rooms():
    assert set(rg.REFUSALS) > set(gg.REFUSALS)
    for name, at in rg.refusal_cases():
        c = rg.refusal(name, at)
        e = c.expect()
        assert c.n == 300 and at in (0, 256, 299) and e["row_status"][at] == ERR_ARG and e["row_lengths"][at] == 0, c.name
        assert sum(st == OK and ln > 0 for st, ln in zip(e["row_status"], e["row_lengths"])) > 250, c.name
        if name == "offset_past_total_lengths_null":
            other = (at + 1) % 300
            assert c.lengths is None and e["row_status"][other] == OK and e["row_lengths"][other] == 0
    e = rg.too_long().expect()
    assert e["row_status"] == [OK, ERR_OVERFLOW, OK, ERR_OVERFLOW, OK, OK, ERR_OVERFLOW] and e["row_lengths"] == [10, 0, 40, 0, 0, 5, 0]
    assert e["need"][1] == 4000 and e["status"] == ERR_OVERFLOW
    assert e["need"][0] == sum(len(p) for p in e["pieces"]), "a too-long row's pieces are counted"
    what = [w for w, _, _ in rg.rooms()]
    assert len(what) == 4
    for w, c, cap in rg.rooms():
        full, e = c.expect(), c.expect(cap)
        assert e["need"] == full["need"], w
        unfit = [k for k in range(c.n) if e["row_status"][k] == ERR_OVERFLOW]
        if w == "exactly the pieces needed":
            assert not unfit and cap == full["need"][0]
        else:
            first = unfit[0]
            assert unfit and all(e["row_status"][k] == ERR_OVERFLOW for k in range(first, c.n)), (w, "the fitting rows are no prefix")
            assert all(e["row_status"][k] == OK for k in range(first)) and e["fit_pieces"] <= cap
        if w == "one piece short":
            assert unfit[0] == max(k for k in range(c.n) if full["pieces"][k])
        if w == "pieces that end inside a row of several":
            assert len(full["pieces"][unfit[0]]) >= 3 and unfit[0] >= rg.ROOM_MIDDLE
        if w == "one piece":
            assert e["fit_pieces"] <= 1 and unfit[0] <= 2


def test_the_refused_index_is_all_format_and_all_padding():
    c = rg.refused_case()
    e = c.expect()
    assert c.index.refused and e["row_status"] == [ERR_FORMAT] * c.n and e["row_lengths"] == [0] * c.n and e["need"] == [0, 0]
    fill = np.full(c.n * c.stride, 0x11, dtype=np.uint8)
    assert (c.image(e, 0xA5, fill) == 0xA5).all() and (c.image(e, -1, fill) == 0x11).all()


def test_the_image_is_data_then_padding():
    c = rg.too_long()
    e = c.expect()
    fill = np.arange(c.n * c.stride, dtype=np.uint64).astype(np.uint8)
    img = c.image(e, 0xA5, fill).reshape(c.n, c.stride)
    raw = c.image(e, -1, fill).reshape(c.n, c.stride)
    for k, row in enumerate(c.rows(e)):
        assert bytes(img[k, :len(row)]) == bytes(row) == bytes(raw[k, :len(row)]) == c.index.data[c.offsets[k]:c.offsets[k] + len(row)]
        assert (img[k, len(row):] == 0xA5).all() and bytes(raw[k, len(row):]) == bytes(fill.reshape(c.n, c.stride)[k, len(row):])
