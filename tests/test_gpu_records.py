"""GPU tests of the record tables (tsqa_records_async, tsqa_records, DeviceCodec.records_async, RangeIndex.records, RecordTable): the
cases are recordgen's, the expected tables are made there in numpy from the sources' bytes, and test_records_cpu.py shows that each
case reaches what it aims at.  Every call runs on a side stream; every table the library may write sits between guard words, is
filled with the guard first, and is compared WHOLE: the entries owed, the guard in every entry at or past cap_records, and both
fences.  The tables are also placed one element past a multiple of 16 bytes (8 mod 16 for the 64-bit tables, 4 mod 8 for the item
numbers): every alignment a table of that type can have."""
import ctypes as C

import numpy as np
import pytest

import gathergen as gg
import recordgen as rc_gen
from test_gpu_cut import FENCE, Index, sentinel, to_dev, u64_dev
from test_gpu_gather import index_of, u32_dev

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = rc_gen.OK, rc_gen.ERR_ARG, rc_gen.ERR_FORMAT, rc_gen.ERR_STREAM, rc_gen.ERR_OVERFLOW
GUARD, TABLE_FENCE = -0x5A5A5A5B, 32


@pytest.fixture(scope="module")
def tsq():
    import torch
    assert torch.cuda.is_available()
    import turbosqueeze_amd
    return turbosqueeze_amd


@pytest.fixture(scope="module")
def codec(tsq):
    c = tsq.DeviceCodec(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def default_variants(codec):
    codec.set_variant(0, 0)
    yield
    codec.set_variant(0, 0)


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream()


class Table:
    """n words the call may write, filled with the guard, between guard words; skew: the table starts that many elements further on"""

    def __init__(self, n, dtype, skew=0):
        import torch
        self.n, self.at = n, TABLE_FENCE + skew
        self.buf = torch.full((n + 2 * TABLE_FENCE + 2,), GUARD, dtype=dtype, device="cuda")

    def ptr(self):
        return self.buf.data_ptr() + self.at * self.buf.element_size()

    @property
    def t(self):
        return self.buf[self.at:self.at + self.n]

    def values(self):
        host = self.buf.cpu().numpy()
        assert (host[:self.at] == GUARD).all() and (host[self.at + self.n:] == GUARD).all(), "a table's fence"
        return host[self.at:self.at + self.n]


class Room:
    """the call's outputs for cap_records entries and n_items items"""

    def __init__(self, cap, n_items, skew=0):
        import torch
        self.items, self.offsets, self.lengths = Table(cap, torch.int32, skew), Table(cap, torch.int64, skew), Table(cap, torch.int64, skew)
        self.first, self.need, self.word = Table(n_items + 1, torch.int64, skew), Table(2, torch.int64), Table(1, torch.int32)
        if skew:
            assert self.offsets.ptr() % 16 == 8 and self.items.ptr() % 8 == 4

    def tables(self):
        return (self.items, self.offsets, self.lengths, self.first, self.need, self.word)


def records_call(codec, index, delim, flags, cap, room, sync=False, over=()):
    """tsqa_records_async (sync: tsqa_records) on the current stream -> its return value.  over: arguments replaced."""
    a = dict(ctx=codec.h, idx=index.h, delim=delim, flags=flags, cap=cap, items=room.items.ptr(), offsets=room.offsets.ptr(),
             lengths=room.lengths.ptr(), first=room.first.ptr(), need=room.need.ptr(), status=room.word.ptr())
    a.update(dict(over))
    f = codec.L.tsqa_records if sync else codec.L.tsqa_records_async
    return f(a["ctx"], a["idx"], a["delim"], a["flags"], a["cap"], a["items"], a["offsets"], a["lengths"], a["first"], a["need"], a["status"],
             codec._stream())


def check(room, e, cap, what):
    """every table whole: the prefix owed, the guard at and past it, the fences"""
    k = min(cap, e["need"][0])
    assert room.word.values().tolist() == [e["status"]], f"{what}: *d_status is {room.word.values().tolist()}, owed {e['status']}"
    assert room.need.values().tolist() == e["need"], f"{what}: d_need is {room.need.values().tolist()}, owed {e['need']}"
    got = room.first.values()
    assert got.tolist() == e["item_first"], f"{what}: d_item_first_record differs first at item {int(np.flatnonzero(got != np.array(e['item_first']))[0])}"
    for name, tab, want in (("offsets", room.offsets, e["offsets"]), ("lengths", room.lengths, e["lengths"]), ("items", room.items, e["items"])):
        got = tab.values()
        if not np.array_equal(got[:k], want[:k]):
            at = int(np.flatnonzero(got[:k] != want[:k])[0])
            raise AssertionError(f"{what}: {name}[{at}] is {int(got[at])} for {int(want[at])} ({k} records)")
        assert (got[k:] == GUARD).all(), f"{what}: {name} was written at or past record {k}"


def run(codec, side, case, flags=0, cap=None, skew=0, index=None, data=None, what="", items=True):
    """one call on the side stream, checked against recordgen -> (Room, expectation)"""
    import torch
    e = case.expect(flags, cap) if data is None else rc_gen.restate(case.index, case.delim, flags, cap, data)
    room_cap = e["need"][0] if cap is None else cap
    index = index or index_of(codec, case.index)
    room = Room(room_cap, case.index.n_items, skew)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rc = records_call(codec, index, case.delim, flags, room_cap, room, over=() if items else dict(items=None))
    assert rc == 0, codec.last_error()
    side.synchronize()
    if not items:
        assert (room.items.values() == GUARD).all()
        e = dict(e, items=np.full(len(e["items"]), GUARD))
    check(room, e, room_cap, f"{what or case.name} (flags {flags}, cap {room_cap}, skew {skew})")
    return room, e


@pytest.mark.parametrize("delim", rc_gen.DELIMS)
def test_item_lengths_and_delimiter_places(codec, side, delim):
    for k, flags in enumerate(rc_gen.FLAGS):
        run(codec, side, rc_gen.places(delim), flags, skew=k & 1)


@pytest.mark.parametrize("n", rc_gen.COUNTS)
def test_a_ragged_arena_of_many_blocks_in_one_span(codec, side, n):
    for flags in (0, rc_gen.KEEP_DELIM | rc_gen.FLAT):
        run(codec, side, rc_gen.ragged(n), flags, skew=n & 1)


def test_records_across_dozens_of_tiny_blocks(codec, side):
    for flags in rc_gen.FLAGS:
        run(codec, side, rc_gen.tiny(), flags)


@pytest.mark.parametrize("kind", rc_gen.CHUNK_KINDS)
def test_chunk_edges(codec, side, kind):
    for k, flags in enumerate(rc_gen.FLAGS):
        run(codec, side, rc_gen.chunk_edges(kind), flags, skew=k & 1)


def test_the_ring_wraps_between_delimiters(codec, side):
    for flags in (0, rc_gen.KEEP_DELIM):
        room, e = run(codec, side, rc_gen.ring_wrap(), flags)
    assert e["need"][0] == len(rc_gen.RING_DELIMS) + 1


def test_the_ring_wraps_at_a_skew(codec, side):
    """blocks longer than the ring that start at 1 and 38 mod 64 of the concatenation: the ring's skew is the block's start mod 64"""
    for k, flags in enumerate(rc_gen.FLAGS):
        room, e = run(codec, side, rc_gen.ring_wrap_skewed(), flags, skew=k & 1)
    assert e["need"][0] == 20


def test_a_record_across_two_blocks(codec, side):
    run(codec, side, rc_gen.two_blocks(), rc_gen.KEEP_DELIM, skew=1)


@pytest.mark.parametrize("kind", ("sized", "plain"))
def test_short_blocks_through_both_kinds_of_index(codec, side, kind):
    for flags in (0, rc_gen.FLAT | rc_gen.KEEP_DELIM):
        run(codec, side, rc_gen.short_blocks(kind), flags)


@pytest.mark.parametrize("n_blocks", rc_gen.BIG_BLOCKS)
def test_around_the_second_pass_of_the_group_scan(codec, tsq, side, n_blocks):
    """containers of 65 535, 65 536 and 65 537 blocks of 4 096 bytes made on the GPU by the split compress (the last block one byte
    long); the tables are compared with the restatement over the input"""
    import torch
    import seekgen as kg
    n_total = (n_blocks - 1) * rc_gen.BIG_LEN + 1
    data = kg.scan_edge_input(n_total)
    blob, table = codec.compress_split(to_dev(data), 1, rc_gen.BIG_LEN, block_sizes=True)
    idx = codec.index_sized(blob, n_total, rc_gen.BIG_LEN, table)
    assert idx.n_blocks == n_blocks
    case = rc_gen.Case(f"big_{n_blocks}", gg.Index(f"big_{n_blocks}", "sized", None, None, kg.out_start(n_total, rc_gen.BIG_LEN), block_len=rc_gen.BIG_LEN), 10)
    try:
        run(codec, side, case, rc_gen.KEEP_DELIM, index=idx, data=data, skew=n_blocks & 1)
    finally:
        torch.cuda.synchronize()
        idx.close()


@pytest.mark.parametrize("front", (False, True))
def test_first_record_numbers_past_2_to_the_24(codec, side, front):
    """19.66 million records and room for 1 000: the whole first-record table, both need words and the prefix"""
    room, e = run(codec, side, rc_gen.carries(front), 0, cap=rc_gen.CARRY_CAP)
    assert e["status"] == ERR_OVERFLOW and rc_gen.SPLIT in e["item_first"]


@pytest.mark.parametrize("name", ("places", "ragged", "damaged", "chunks"))
def test_cap_records_keeps_a_prefix(codec, side, name):
    case = dict(places=rc_gen.places(10), ragged=rc_gen.ragged(257), damaged=rc_gen.damaged(), chunks=rc_gen.chunk_edges("text"))[name]
    full = case.expect()["need"]
    for k, (what, cap) in enumerate(rc_gen.caps(case)):
        room, e = run(codec, side, case, rc_gen.FLAT if k & 1 else 0, cap=cap, skew=k & 1, what=f"{case.name}: {what}")
        assert e["status"] == (OK if cap >= full[0] else ERR_OVERFLOW) and e["need"][0] == full[0]
    # room to spare changes nothing, and d_rec_items may be NULL
    run(codec, side, case, 0, cap=full[0] + 77)
    run(codec, side, case, rc_gen.KEEP_DELIM, items=False)


def test_the_measuring_call(codec, side):
    """cap_records 0 with all three tables NULL: the first-record table and both need words, and TSQA_ERR_OVERFLOW"""
    import torch
    for case in (rc_gen.places(0), rc_gen.tiny()):
        room, e = Room(0, case.index.n_items), case.expect(rc_gen.KEEP_DELIM, 0)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            rc = records_call(codec, index_of(codec, case.index), case.delim, rc_gen.KEEP_DELIM, 0, room, over=dict(items=None, offsets=None, lengths=None))
        assert rc == 0, codec.last_error()
        side.synchronize()
        check(room, e, 0, case.name)
        assert e["status"] == ERR_OVERFLOW and e["need"] == case.expect(rc_gen.KEEP_DELIM)["need"]


def test_refused_items_give_no_records(codec, side):
    for flags in (0, rc_gen.FLAT):
        room, e = run(codec, side, rc_gen.damaged(), flags, skew=1)
    first = e["item_first"]
    assert all(first[k] == first[k + 1] for k in rc_gen.DAMAGED_AT)


def test_cut_containers_give_no_records(codec, side):
    """mtgen's cut containers, which only the frame walk refuses, as items 0, 100, 256 and 299 of 300: no records of theirs, and
    every other item exact"""
    for flags in (0, rc_gen.KEEP_DELIM | rc_gen.FLAT):
        room, e = run(codec, side, rc_gen.cut_items(), flags, skew=1)
    first = e["item_first"]
    assert all((first[k] == first[k + 1]) == (k in rc_gen.CUT_AT) for k in range(300))


def test_a_refused_sized_index_gives_format_and_zeros(codec, side):
    import torch
    case = rc_gen.refused_case()
    with torch.cuda.stream(side):
        idx = index_of(codec, case.index)                     # (made on the side stream, nothing waited for: the call reads its verdict)
    room, e = run(codec, side, case, 0, cap=64, index=idx)
    assert room.word.values().tolist() == [ERR_FORMAT] and room.need.values().tolist() == [0, 0] and room.first.values().tolist() == [0, 0]


STREAM_TWINS = 4                # as test_gpu_gather.py: the catalogue's first invalid twins that only a decoder refuses


def test_a_malformed_stream_raises_the_status_to_err_stream(codec, side):
    """recordgen's container with one byte flipped inside its stream, and mtgen's twin containers: six well-formed frames of which
    one holds a stream the decoder refuses.  test_records_cpu.py shows that the host walk accepts every one of them and that the
    oracle's decoder refuses it.  The tables' contents are undefined; nothing outside them is written."""
    import torch
    import mtgen
    twins = [t for t in mtgen.twin_containers() if t[3] == "stream"][:STREAM_TWINS]
    name, bad, at = rc_gen.flipped()
    for name, blob, k, _ in [(name, bad, 0, "stream")] + twins:
        dev = to_dev(np.frombuffer(blob, dtype=np.uint8))
        idx = Index(codec, "plain", dev)
        room = Room(5000, 1)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert records_call(codec, idx, 10, 0, 5000, room) == 0, codec.last_error()
        side.synchronize()
        assert room.word.values().tolist() == [ERR_STREAM], (name, room.word.values().tolist())
        for tab in room.tables():
            tab.values()                                     # (the fences)
        idx.close()


def test_arguments_refused_on_the_host(codec, tsq, side):
    import torch
    case = rc_gen.places(10)
    idx = index_of(codec, case.index)
    cap = case.expect()["need"][0]
    torch.cuda.synchronize()
    for what, over in (("null index", dict(idx=None)), ("null first", dict(first=None)), ("null need", dict(need=None)), ("null status", dict(status=None)),
                       ("delim 256", dict(delim=256)), ("unknown flags", dict(flags=4)), ("unknown flags", dict(flags=0x80000000)),
                       ("null offsets", dict(offsets=None)), ("null lengths", dict(lengths=None))):
        for sync in (False, True):
            room = Room(cap, case.index.n_items)
            with torch.cuda.stream(side):
                rc = records_call(codec, idx, 10, 0, cap, room, sync=sync, over=over)
            side.synchronize()
            assert rc == ERR_ARG, (what, rc)
            assert all((tab.values() == GUARD).all() for tab in room.tables()), what
    # the waiting form returns the status
    room = Room(3, case.index.n_items)
    with torch.cuda.stream(side):
        rc = records_call(codec, idx, 10, 0, 3, room, sync=True)
    assert rc == ERR_OVERFLOW
    check(room, case.expect(0, 3), 3, "the waiting form")
    # a batch index made on the device and not yet fetched: the host cannot size the map
    fresh = tsq.DeviceCodec(0)
    try:
        parts = [tsq.synth.text(n, seed=70 + n) for n in (100, 5000, 300)]
        sizes = [p.size for p in parts]
        starts = [0, sizes[0], sizes[0] + sizes[1]]
        arena = torch.empty(sum(tsq.batch_bound(z) + 16 for z in sizes), dtype=torch.uint8, device="cuda")
        d_offsets, d_sizes = torch.empty(4, dtype=torch.int64, device="cuda"), torch.empty(3, dtype=torch.int64, device="cuda")
        fresh.compress_batch_packed_async(to_dev(np.concatenate(parts)), list(zip(starts, sizes)), 1, 16, arena, d_offsets, d_sizes)
        index = fresh.index_packed_async(arena, d_offsets, d_sizes, 3, 3)
        with pytest.raises(tsq.TsqError) as err:
            index.records()
        assert err.value.code == ERR_ARG and "tsqa_index_fetch" in str(err.value)
        table = index.fetch().records(keep_delim=True)
        torch.cuda.synchronize()
        want = rc_gen.restate(gg.Index("three", "batch", None, np.concatenate(parts).tobytes(), [0] + np.cumsum(sizes).tolist(), item_first=[0, 1, 2, 3]),
                              10, rc_gen.KEEP_DELIM)
        assert table.n == want["need"][0] and table.max_length == want["need"][1] and int(table.status.item()) == OK
        assert table.offsets.cpu().tolist() == want["offsets"].tolist() and table.items.cpu().tolist() == want["items"].tolist()
        index.close()
    finally:
        fresh.close()


@pytest.mark.parametrize("kind", ("plain", "sized", "batch"))
def test_the_records_drive_a_gather(codec, side, kind):
    """tsqa_gather_async over the record tables returns the bytes that Python slicing of the source gives"""
    import torch
    case = dict(plain=rc_gen.chunk_edges("text"), sized=rc_gen.short_blocks("sized"), batch=rc_gen.places(10))[kind]
    flags = rc_gen.KEEP_DELIM | (0 if kind == "batch" else rc_gen.FLAT)
    room, e = run(codec, side, case, flags)
    n, idx = e["need"][0], index_of(codec, case.index)
    total = int(e["lengths"].sum())
    out = to_dev(sentinel(total + FENCE))
    places, st, pieces = Table(n + 1, torch.int64), Table(n, torch.int32), Table(1, torch.int64)
    with torch.cuda.stream(side):
        codec.gather_async(idx, room.items.t if kind == "batch" else None, room.offsets.t.contiguous(), room.lengths.t.contiguous(), n, 1,
                           n + case.index.n_blocks + 8, out[:max(total, 1)], places.t, st.t, pieces.t, out_cap=total)
    side.synchronize()
    assert st.values().tolist() == [OK] * n and codec.status() == OK
    src = np.frombuffer(case.index.data, dtype=np.uint8)
    at = [case.index.item_span(int(i))[0] for i in e["items"]] if kind == "batch" else [0] * n
    want = np.concatenate([src[a + o:a + o + ln] for a, o, ln in zip(at, e["offsets"].tolist(), e["lengths"].tolist())])
    host = out.cpu().numpy()
    assert np.array_equal(host[:total], want) and np.array_equal(host[total:], sentinel(host.size)[total:])
    if kind != "batch":
        assert want.tobytes() == case.index.data, "the records with their terminators are the data"


def lines(tsq, n_lines, longest, seed):
    """text in lines of 1 to `longest` bytes with their newlines, the longest one present -> (uint8 array, line starts, lengths without newline)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, longest, n_lines)
    lens[n_lines // 2] = longest - 1
    body = tsq.synth.text(int(lens.sum()) + n_lines, seed=seed).copy()
    body[body == 10] = 0x20
    ends = np.cumsum(lens + 1) - 1
    body[ends] = 10
    return body, np.concatenate([[0], ends[:-1] + 1]), lens


def test_one_chain_on_one_stream(codec, tsq, side):
    """split compress -> sized index -> records -> record numbers drawn on the device -> gather_rows at the stride d_need[1] will
    read: one stream, no synchronise and no host read in between (cap_records is given).  Twice back to back, the second time with
    data and blocks that make the scratch grow."""
    import torch
    bl, stride = 4096, 96
    runs = []
    for n_lines, m, seed in ((3000, 400, 61), (40000, 2500, 62)):
        data, starts, lens = lines(tsq, n_lines, stride, seed)
        nb, room = tsq.plan_split(data.size, bl)
        i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device="cuda")
        runs.append(dict(data=data, starts=starts, lens=lens, n=n_lines, m=m, src=to_dev(data), blob=to_dev(sentinel(room)),
                         table=torch.full((nb,), -1, dtype=torch.int32, device="cuda"), cap=n_lines + 50, offsets=i64(n_lines + 50),
                         lengths=i64(n_lines + 50), first=i64(2), need=i64(2), st=torch.full((1,), -1, dtype=torch.int32, device="cuda"),
                         out=to_dev(sentinel(m * stride + FENCE)), row_len=i64(m), row_st=torch.full((m,), -1, dtype=torch.int32, device="cuda"),
                         row_need=i64(2), words=i64(2)))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(777)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for r in runs:
            m = r["m"]
            codec.compress_split_async(r["src"], 1, bl, r["blob"], r["table"])
            r["idx"] = codec.index_sized(r["blob"], r["src"].numel(), bl, r["table"], sync=False)
            codec.records_async(r["idx"], 10, rc_gen.KEEP_DELIM | rc_gen.FLAT, r["cap"], None, r["offsets"], r["lengths"], r["first"], r["need"], r["st"])
            r["sel"] = torch.randint(0, 1 << 30, (m,), device="cuda", generator=gen) % r["need"][0]
            codec.gather_rows_async(r["idx"], None, r["offsets"][r["sel"]], r["lengths"][r["sel"]], m, stride, 0, 0, 3 * m, r["out"][:m * stride],
                                    r["row_len"], r["row_st"], r["row_need"])
            r["words"][0:1].copy_(codec._status)
    side.synchronize()
    for r in runs:
        m, data, n = r["m"], r["data"], r["n"]
        assert r["st"].cpu().tolist() == [OK] and r["need"].cpu().tolist() == [n, stride] and r["first"].cpu().tolist() == [0, n]
        assert r["offsets"].cpu().numpy()[:n].tolist() == r["starts"].tolist() and (r["offsets"].cpu().numpy()[n:] == -1).all()
        assert r["lengths"].cpu().numpy()[:n].tolist() == (r["lens"] + 1).tolist()
        assert r["words"].cpu().tolist()[0] == 0 and r["row_st"].cpu().tolist() == [0] * m and r["row_need"].cpu().tolist()[1] <= stride
        sel = r["sel"].cpu().numpy()
        want = np.zeros((m, stride), dtype=np.uint8)
        for k, j in enumerate(sel):
            want[k, :r["lens"][j] + 1] = data[r["starts"][j]:r["starts"][j] + r["lens"][j] + 1]
        out = r["out"].cpu().numpy()
        assert np.array_equal(out[:m * stride].reshape(m, stride), want) and np.array_equal(out[m * stride:], sentinel(out.size)[m * stride:])
        assert r["row_len"].cpu().numpy().tolist() == (r["lens"][sel] + 1).tolist()
        r["idx"].close()


def test_the_chain_through_a_packed_batch(tsq, side):
    """packed compress -> a batch index made on the device -> fetch -> records with d_rec_items -> rows by item"""
    import torch
    fresh = tsq.DeviceCodec(0)
    try:
        n_items, stride = 120, 80
        parts = [lines(tsq, 5 + 3 * (k % 40), stride, 900 + k) for k in range(n_items)]
        sizes = [p[0].size for p in parts]
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
        data = np.concatenate([p[0] for p in parts])
        with torch.cuda.stream(side):
            arena = torch.empty(sum(tsq.batch_bound(z) + 16 for z in sizes), dtype=torch.uint8, device="cuda")
            d_offsets, d_sizes = torch.empty(n_items + 1, dtype=torch.int64, device="cuda"), torch.empty(n_items, dtype=torch.int64, device="cuda")
            fresh.compress_batch_packed_async(to_dev(data), list(zip(starts, sizes)), 1, 16, arena, d_offsets, d_sizes)
            index = fresh.index_packed_async(arena, d_offsets, d_sizes, n_items, n_items).fetch()
            table = index.records(cap_records=sum(len(p[1]) for p in parts), sync=False)
            sel = torch.arange(table.offsets.numel() - 1, -1, -7, device="cuda")
            rows, lens = table.gather_rows(sel, row_stride=stride, pad=0x2E, cap_pieces=2 * sel.numel())
        side.synchronize()
        want = rc_gen.restate(gg.Index("packed", "batch", None, data.tobytes(), [0] + np.cumsum(sizes).tolist(), item_first=list(range(n_items + 1))), 10)
        assert int(table.status.item()) == OK and table.n == want["need"][0] and table.max_length == want["need"][1] == stride - 1
        assert table.items.cpu().tolist() == want["items"].tolist() and table.offsets.cpu().tolist() == want["offsets"].tolist()
        assert table.item_first.cpu().tolist() == want["item_first"]
        got, picked = rows.cpu().numpy(), sel.cpu().numpy()
        assert lens.cpu().tolist() == want["lengths"][picked].tolist()
        for k, j in enumerate(picked):
            a = starts[int(want["items"][j])] + int(want["offsets"][j])
            ln = int(want["lengths"][j])
            assert bytes(got[k, :ln]) == data[a:a + ln].tobytes() and (got[k, ln:] == 0x2E).all(), (k, j)
        index.close()
    finally:
        fresh.close()


def test_the_command_line_tool_counts_records(tmp_path):
    """tools/tsq_cli r: the record count and the longest record of a file, one run per delimiter"""
    import json
    import os
    import subprocess
    case = rc_gen.chunk_edges("text")
    packed = tmp_path / "in.tsq"
    packed.write_bytes(case.index.blob)
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tsq_cli")
    for args, delim in (([], 10), (["32"], 32)):
        r = subprocess.run([cli, "r", str(packed)] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        need = rc_gen.restate(case.index, delim)["need"]
        assert json.loads(r.stdout) == dict(bytes=case.index.total, delim=delim, records=need[0], longest_record=need[1])
    assert subprocess.run([cli, "r", str(packed), "256"], capture_output=True, text=True, timeout=300).returncode != 0


def test_the_python_wrapper_measures_then_fills(codec, tsq):
    import torch
    data, starts, lens = lines(tsq, 700, 120, 33)
    blob = codec.compress(to_dev(data), 1)
    idx = codec.index(blob)
    table = idx.records()
    assert table.n == 700 and table.max_length == 119 and int(table.status.item()) == OK
    assert table.offsets.cpu().tolist() == starts.tolist() and table.lengths.cpu().tolist() == lens.tolist() and table.item_first.cpu().tolist() == [0, 700]
    rows, got = table.gather_rows(torch.tensor([5, 0, 699], device="cuda"))
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (3, 119) and got.cpu().tolist() == lens[[5, 0, 699]].tolist()
    assert bytes(rows[0, :lens[5]].cpu().numpy()) == data[starts[5]:starts[5] + lens[5]].tobytes()
    short = idx.records(cap_records=10)
    assert int(short.status.item()) == ERR_OVERFLOW and short.n == 700 and short.offsets.cpu().tolist() == starts[:10].tolist()
    with pytest.raises(tsq.TsqError) as err:
        idx.records(delim=256)
    assert err.value.code == ERR_ARG
    mm, mn, tm, tn = codec.profile_read_records()
    assert (mn, tn) == (0, 0)
    idx.close()
