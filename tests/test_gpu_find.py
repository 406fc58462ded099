"""GPU tests of the find (tsqa_find_async, tsqa_find, DeviceCodec.find_async, RangeIndex.find, HitTable, RecordTable.containing):
the cases are findgen's, the expected tables are made there from the sources' bytes with bytes.find, and test_find_cpu.py shows that
each case reaches what it aims at.  Every call runs on a side stream; every table the library may write sits between guard words,
is filled with the guard first, and is compared WHOLE: the entries owed, the guard in every entry at or past cap_hits, and both
fences.  The tables are also placed one element past a multiple of 16 bytes."""
import numpy as np
import pytest

import findgen as fg
import gathergen as gg
import recordgen as rg
from test_gpu_cut import FENCE, Index, sentinel, to_dev
from test_gpu_gather import index_of
from test_gpu_records import GUARD, Table, lines, records_call
from test_gpu_records import Room as RecordRoom
from test_gpu_records import check as check_records

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = fg.OK, fg.ERR_ARG, fg.ERR_FORMAT, fg.ERR_STREAM, fg.ERR_OVERFLOW


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


class Room:
    """the call's outputs for cap_hits entries and n_items items; d_need is ONE word between its fences"""

    def __init__(self, cap, n_items, skew=0):
        import torch
        self.items, self.offsets = Table(cap, torch.int32, skew), Table(cap, torch.int64, skew)
        self.first, self.need, self.word = Table(n_items + 1, torch.int64, skew), Table(1, torch.int64), Table(1, torch.int32)
        if skew:
            assert self.offsets.ptr() % 16 == 8 and self.items.ptr() % 8 == 4

    def tables(self):
        return (self.items, self.offsets, self.first, self.need, self.word)


def find_call(codec, index, needle, flags, cap, room, sync=False, over=()):
    """tsqa_find_async (sync: tsqa_find) on the current stream -> its return value.  over: arguments replaced."""
    a = dict(ctx=codec.h, idx=index.h, needle=bytes(needle), m=len(needle), flags=flags, cap=cap, items=room.items.ptr(), offsets=room.offsets.ptr(),
             first=room.first.ptr(), need=room.need.ptr(), status=room.word.ptr())
    a.update(dict(over))
    f = codec.L.tsqa_find if sync else codec.L.tsqa_find_async
    return f(a["ctx"], a["idx"], a["needle"], a["m"], a["flags"], a["cap"], a["items"], a["offsets"], a["first"], a["need"], a["status"], codec._stream())


def check(room, e, cap, what):
    """every table whole: the prefix owed, the guard at and past it, the fences"""
    k = min(cap, e["need"][0])
    assert room.word.values().tolist() == [e["status"]], f"{what}: *d_status is {room.word.values().tolist()}, owed {e['status']}"
    assert room.need.values().tolist() == e["need"], f"{what}: d_need is {room.need.values().tolist()}, owed {e['need']}"
    got = room.first.values()
    assert got.tolist() == e["item_first"], f"{what}: d_item_first_hit differs first at item {int(np.flatnonzero(got != np.array(e['item_first']))[0])}"
    for name, tab, want in (("offsets", room.offsets, e["offsets"]), ("items", room.items, e["items"])):
        got = tab.values()
        if not np.array_equal(got[:k], want[:k]):
            at = int(np.flatnonzero(got[:k] != want[:k])[0])
            raise AssertionError(f"{what}: {name}[{at}] is {int(got[at])} for {int(want[at])} ({k} hits)")
        assert (got[k:] == GUARD).all(), f"{what}: {name} was written at or past hit {k}"


def run(codec, side, case, flags=0, cap=None, skew=0, index=None, data=None, what="", items=True):
    """one call on the side stream, checked against findgen -> (Room, expectation)"""
    import torch
    e = case.expect(flags, cap) if data is None else fg.restate(case.index, case.needle, flags, cap, data)
    room_cap = e["need"][0] if cap is None else cap
    index = index or index_of(codec, case.index)
    room = Room(room_cap, case.index.n_items, skew)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rc = find_call(codec, index, case.needle, flags, room_cap, room, over=() if items else dict(items=None))
    assert rc == 0, codec.last_error()
    side.synchronize()
    if not items:
        assert (room.items.values() == GUARD).all()
        e = dict(e, items=np.full(len(e["items"]), GUARD))
    check(room, e, room_cap, f"{what or case.name} (flags {flags}, cap {room_cap}, skew {skew})")
    return room, e


# ---- 1: lengths and places ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", fg.NEEDLE_LENGTHS)
def test_needle_lengths_item_lengths_and_places(codec, side, m):
    for everywhere in (False, True):
        for k, flags in enumerate(fg.FLAGS):
            room, e = run(codec, side, fg.places(m, everywhere), flags, skew=k & 1)
            assert e["need"][0] > 0


# ---- 2: cell and word edges ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("start", fg.CELL_STARTS)
def test_hits_ending_at_every_cell_residue_and_around_a_word_edge(codec, side, start):
    for m in fg.CELL_NEEDLES:
        for flags in fg.FLAGS:
            run(codec, side, fg.cell_edges(m, start), flags, skew=start & 1)


# ---- 3: chunk edges -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", fg.CHUNK_CASES)
def test_chunk_edges(codec, side, kind):
    for k, flags in enumerate(fg.FLAGS):
        run(codec, side, fg.chunk_edges(kind), flags, skew=k & 1)


# ---- 4: the ring wrap ---------------------------------------------------------------------------------------------------------------------

def test_needles_across_the_ring_wrap(codec, side):
    room, e = run(codec, side, fg.ring_wrap(), 0)
    assert e["need"][0] >= 3 * 17 + 1


def test_needles_across_the_ring_wrap_at_a_skew(codec, side):
    for k, flags in enumerate(fg.FLAGS):
        room, e = run(codec, side, fg.ring_wrap_skewed(), flags, skew=k & 1)
    assert e["need"][0] >= 2 * (2 * 17 + 1)


# ---- 5: block seams -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", fg.SEAM_NEEDLES)
def test_hits_across_runs_of_tiny_and_empty_blocks(codec, side, m):
    for k, flags in enumerate(fg.FLAGS):
        run(codec, side, fg.seams(m), flags, skew=k & 1)


@pytest.mark.parametrize("m", (2, 16))
def test_a_hit_that_ends_in_a_block_of_one_byte(codec, side, m):
    room, e = run(codec, side, fg.two_blocks(m), fg.FLAT, skew=1)
    assert e["offsets"].tolist()[-1] == fg.BLOCK + 1 - m


@pytest.mark.parametrize("kind", ("sized", "plain"))
def test_hits_across_every_edge_of_257_short_blocks(codec, side, kind):
    for m in (2, 16):
        run(codec, side, fg.phrase(kind, m), fg.FLAT if m == 2 else 0)


# ---- 6: item seams ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", fg.COUNTS)
def test_no_hit_runs_from_one_item_into_the_next(codec, side, n):
    for m in (2, 16):
        for flags in fg.FLAGS:
            run(codec, side, fg.ragged(n, m), flags, skew=n & 1)


def test_refused_items_give_no_hits(codec, side):
    for needle in (b"ef ", b"e"):
        for flags in fg.FLAGS:
            room, e = run(codec, side, fg.damaged(needle), flags, skew=1)
        first = e["item_first"]
        assert all(first[k] == first[k + 1] for k in fg.DAMAGED_AT) and first[-1] > 0


# ---- 7: the scans -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_blocks", fg.BIG_BLOCKS)
def test_around_the_second_pass_of_the_group_scan(codec, tsq, side, n_blocks):
    """containers of 65 535, 65 536 and 65 537 blocks of 4 096 bytes made on the GPU by the split compress (the last block one byte
    long); the needle is 'e ', frequent in the text third and present in the random third by chance, so blocks of the last group of
    256 hold hits whose numbers need the bases of both passes"""
    import torch
    import seekgen as kg
    n_total = (n_blocks - 1) * fg.BIG_LEN + 1
    data = kg.scan_edge_input(n_total)
    blob, table = codec.compress_split(to_dev(data), 1, fg.BIG_LEN, block_sizes=True)
    idx = codec.index_sized(blob, n_total, fg.BIG_LEN, table)
    assert idx.n_blocks == n_blocks
    case = fg.Case(f"big_{n_blocks}", gg.Index(f"big_{n_blocks}", "sized", None, None, kg.out_start(n_total, fg.BIG_LEN), block_len=fg.BIG_LEN), b"e ")
    try:
        room, e = run(codec, side, case, fg.FLAT, index=idx, data=data.tobytes(), skew=n_blocks & 1)
        assert e["need"][0] > 1000 and int(e["offsets"][-1]) >= (n_blocks - 1 - fg.GROUP) * fg.BIG_LEN
    finally:
        torch.cuda.synchronize()
        idx.close()


@pytest.mark.parametrize("front", (False, True))
def test_first_hit_numbers_past_2_to_the_24(codec, side, front):
    """19.66 million hits and room for 1 000: the whole first-hit table, the need word and the prefix"""
    room, e = run(codec, side, fg.carries(front), 0, cap=fg.CARRY_CAP)
    assert e["status"] == ERR_OVERFLOW and fg.SPLIT in e["item_first"]


# ---- 8: caps and the measuring call -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("places", "ragged", "damaged", "chunks", "seams"))
def test_cap_hits_keeps_a_prefix(codec, side, name):
    case = dict(places=fg.places(3, True), ragged=fg.ragged(257, 2), damaged=fg.damaged(b"e"), chunks=fg.chunk_edges("text_3"), seams=fg.seams(16))[name]
    full = case.expect()["need"]
    for k, (what, cap) in enumerate(fg.caps(case)):
        room, e = run(codec, side, case, fg.FLAT if k & 1 else 0, cap=cap, skew=k & 1, what=f"{case.name}: {what}")
        assert e["status"] == (OK if cap >= full[0] else ERR_OVERFLOW) and e["need"] == full
    # room to spare changes nothing, and d_hit_items may be NULL
    run(codec, side, case, 0, cap=full[0] + 77)
    run(codec, side, case, fg.FLAT, items=False)


def test_the_measuring_call(codec, side):
    """cap_hits 0 with both tables NULL: the first-hit table and the need word, and TSQA_ERR_OVERFLOW"""
    import torch
    for case in (fg.places(2, False), fg.seams(3)):
        room, e = Room(0, case.index.n_items), case.expect(0, 0)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            rc = find_call(codec, index_of(codec, case.index), case.needle, 0, 0, room, over=dict(items=None, offsets=None))
        assert rc == 0, codec.last_error()
        side.synchronize()
        check(room, e, 0, case.name)
        assert e["status"] == ERR_OVERFLOW and e["need"] == case.expect()["need"]


# ---- 9: refusals --------------------------------------------------------------------------------------------------------------------------

def test_a_refused_sized_index_gives_format_and_zeros(codec, side):
    import torch
    case = fg.refused_case()
    with torch.cuda.stream(side):
        idx = index_of(codec, case.index)                     # (made on the side stream, nothing waited for: the call reads its verdict)
    room, e = run(codec, side, case, 0, cap=64, index=idx)
    assert room.word.values().tolist() == [ERR_FORMAT] and room.need.values().tolist() == [0] and room.first.values().tolist() == [0, 0]


def test_an_index_of_no_blocks_clears_its_tables(codec, side):
    """both items refused at the header: 0 blocks.  The status, the need word and the first-hit table are cleared, the hit tables
    stay as they were, and the waiting form returns 0"""
    import torch
    case = fg.no_blocks()
    assert case.index.n_blocks == 0 and case.index.total == 0 and case.index.n_items == 2
    for flags in fg.FLAGS:
        room, e = run(codec, side, case, flags, cap=8, skew=1)
        assert e["status"] == OK and room.first.values().tolist() == [0, 0, 0] and room.need.values().tolist() == [0]
    room = Room(8, 2)
    with torch.cuda.stream(side):
        assert find_call(codec, index_of(codec, case.index), case.needle, 0, 8, room, sync=True) == OK
    check(room, case.expect(0, 8), 8, "no blocks, the waiting form")


def test_the_profile_slots_of_the_find(tsq, side):
    """with profiling on, one find call fills one span of the find decode and one of its seam and table launches -- and none of the
    records' --, a records call the other way round, and a read empties the slots"""
    import torch
    fresh = tsq.DeviceCodec(0)
    try:
        case = fg.phrase("plain", 16)
        idx = Index(fresh, "plain", to_dev(np.frombuffer(case.index.blob, dtype=np.uint8)))
        room = Room(case.expect()["need"][0], 1)
        fresh.profile(True)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert find_call(fresh, idx, case.needle, 0, room.offsets.n, room) == 0, fresh.last_error()
        side.synchronize()
        fm, fn, tm, tn = fresh.profile_read_find()
        assert (fn, tn) == (1, 1) and fm > 0 and tm > 0
        assert fresh.profile_read_records()[1::2] == (0, 0) and fresh.profile_read_find()[1::2] == (0, 0)
        check(room, case.expect(), room.offsets.n, "profiled")
        rec = RecordRoom(0, 1)
        with torch.cuda.stream(side):
            assert records_call(fresh, idx, 10, 0, 0, rec, over=dict(items=None, offsets=None, lengths=None)) == 0
        side.synchronize()
        assert fresh.profile_read_find()[1::2] == (0, 0) and fresh.profile_read_records()[1::2] == (1, 1)
        fresh.profile(False)
        idx.close()
    finally:
        fresh.close()


def test_a_malformed_stream_raises_the_status_to_err_stream(codec, side):
    """mtgen's twin containers: six well-formed frames of which one holds a stream the decoder refuses (test_records_cpu.py shows that
    the host walk accepts them and the oracle's decoder does not).  The tables' contents are undefined; nothing outside them is written."""
    import torch
    import mtgen
    twins = [t for t in mtgen.twin_containers() if t[3] == "stream"][:2]
    for name, blob, k, _ in twins:
        dev = to_dev(np.frombuffer(blob, dtype=np.uint8))
        idx = Index(codec, "plain", dev)
        room = Room(5000, 1)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert find_call(codec, idx, b"ef ", 0, 5000, room) == 0, codec.last_error()
        side.synchronize()
        assert room.word.values().tolist() == [ERR_STREAM], (name, room.word.values().tolist())
        for tab in room.tables():
            tab.values()                                     # (the fences)
        idx.close()


def test_arguments_refused_on_the_host(codec, tsq, side):
    import torch
    case = fg.places(2, False)
    idx = index_of(codec, case.index)
    cap = case.expect()["need"][0]
    torch.cuda.synchronize()
    for what, over in (("null index", dict(idx=None)), ("null needle", dict(needle=None)), ("null first", dict(first=None)), ("null need", dict(need=None)),
                       ("null status", dict(status=None)), ("m 0", dict(m=0)), ("m 17", dict(needle=b"x" * 17, m=17)), ("unknown flags", dict(flags=1)),
                       ("unknown flags", dict(flags=0x80000000)), ("null offsets", dict(offsets=None))):
        for sync in (False, True):
            room = Room(cap, case.index.n_items)
            with torch.cuda.stream(side):
                rc = find_call(codec, idx, case.needle, 0, cap, room, sync=sync, over=over)
            side.synchronize()
            assert rc == ERR_ARG, (what, rc)
            assert all((tab.values() == GUARD).all() for tab in room.tables()), what
    # the waiting form returns the status
    room = Room(3, case.index.n_items)
    with torch.cuda.stream(side):
        rc = find_call(codec, idx, case.needle, 0, 3, room, sync=True)
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
            index.find(b"ef ")
        assert err.value.code == ERR_ARG and "tsqa_index_fetch" in str(err.value)
        table = index.fetch().find(b"ef ")
        torch.cuda.synchronize()
        want = fg.restate(gg.Index("three", "batch", None, np.concatenate(parts).tobytes(), [0] + np.cumsum(sizes).tolist(), item_first=[0, 1, 2, 3]), b"ef ")
        assert table.n == want["need"][0] > 0 and int(table.status.item()) == OK
        assert table.offsets.cpu().tolist() == want["offsets"].tolist() and table.items.cpu().tolist() == want["items"].tolist()
        index.close()
    finally:
        fresh.close()


# ---- 10: the records cross-check ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("places", "chunks"))
def test_a_one_byte_needle_finds_the_records_terminators(codec, side, name):
    """the hits of [delim] are offset + length - 1 of every terminated record with keep_delim on: both from the device"""
    import torch
    rcase = dict(places=rg.places(10), chunks=rg.chunk_edges("text"))[name]
    idx, flags = index_of(codec, rcase.index), rg.KEEP_DELIM | rg.FLAT
    e = rcase.expect(flags)
    rec = RecordRoom(e["need"][0], rcase.index.n_items)
    case = fg.Case(f"{rcase.name}_as_a_needle", rcase.index, bytes([rcase.delim]))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert records_call(codec, idx, rcase.delim, flags, e["need"][0], rec) == 0, codec.last_error()
    side.synchronize()
    check_records(rec, e, e["need"][0], rcase.name)
    room, h = run(codec, side, case, fg.FLAT)
    offsets, lengths = rec.offsets.values(), rec.lengths.values()
    ends = offsets + lengths - 1
    src = np.frombuffer(rcase.index.data, dtype=np.uint8)
    terminated = lengths > 0
    terminated[terminated] = src[ends[terminated]] == rcase.delim
    assert room.offsets.values().tolist() == ends[terminated].tolist() and h["need"][0] > 0


# ---- 11: chains -----------------------------------------------------------------------------------------------------------------------------

def grep(data: bytes, needle: bytes):
    """the lines of `data` (terminated by newlines) that contain `needle`, in pure Python -> [(line number, the line with its newline)]"""
    out = []
    for k, line in enumerate(data.split(b"\n")[:-1]):
        if needle in line:
            out.append((k, line + b"\n"))
    return out


def test_one_chain_on_one_stream(codec, tsq, side):
    """split compress -> sized index -> find -> records(flat) -> RecordTable.containing -> gather_rows: one stream, and the library is
    given both caps, so it neither synchronises nor reads anything back in between (torch.unique inside containing waits for its
    own count).  Twice back to back, the second time with data and blocks that make the scratch grow.  The rows are exactly the
    lines that contain the needle."""
    import torch
    bl, stride, needle = 4096, 96, b"ef "
    runs = []
    for n_lines, seed in ((3000, 61), (40000, 62)):
        data, starts, lens = lines(tsq, n_lines, stride, seed)
        nb, room = tsq.plan_split(data.size, bl)
        want = grep(data.tobytes(), needle)
        runs.append(dict(data=data, n=n_lines, want=want, src=to_dev(data), blob=to_dev(sentinel(room)),
                         table=torch.full((nb,), -1, dtype=torch.int32, device="cuda"), cap_hits=data.size // 8))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for r in runs:
            codec.compress_split_async(r["src"], 1, bl, r["blob"], r["table"])
            r["idx"] = codec.index_sized(r["blob"], r["src"].numel(), bl, r["table"], sync=False)
            r["hits"] = r["idx"].find(needle, flat=True, cap_hits=r["cap_hits"], sync=False)
            r["recs"] = r["idx"].records(keep_delim=True, flat=True, cap_records=r["n"] + 50, sync=False)
            # (both tables have room to spare: containing leaves the entries past the counts out, on the device)
            r["sel"] = r["recs"].containing(r["hits"])
            k = len(r["want"])                               # (the row count is the host's: it sizes the output)
            r["rows"], r["row_len"] = r["recs"].gather_rows(r["sel"][:k], row_stride=stride, cap_pieces=3 * k + 8)
    side.synchronize()
    for r in runs:
        want = r["want"]
        assert int(r["hits"].status.item()) == OK and int(r["recs"].status.item()) == OK and r["recs"].n == r["n"]
        assert r["hits"].n == sum(line.count(needle) for line in r["data"].tobytes().split(b"\n")) > 100
        assert r["sel"].cpu().tolist() == [k for k, _ in want]
        rows, got = r["rows"].cpu().numpy(), r["row_len"].cpu().tolist()
        assert got == [len(line) for _, line in want]
        for j, (_, line) in enumerate(want):
            assert bytes(rows[j, :len(line)]) == line and not rows[j, len(line):].any(), j
        r["idx"].close()


def test_records_find_records_share_the_scratch(codec, tsq, side):
    """a records call, a find call and a records call in that order on one stream with nothing waited for in between: the three share
    the context and its bit map, and none sees another's bits.  Twice, the second time larger."""
    import torch
    for n_lines, seed in ((2000, 71), (30000, 72)):
        data, starts, lens = lines(tsq, n_lines, 120, seed)
        blob = codec.compress(to_dev(data), 1)
        idx = codec.index(blob)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            first = idx.records(flat=True, cap_records=n_lines, sync=False)
            hits = idx.find(b" tl", flat=True, cap_hits=data.size // 8, sync=False)
            second = idx.records(flat=True, cap_records=n_lines, sync=False)
        side.synchronize()
        want = fg.item_hits(data.tobytes(), b" tl")
        assert hits.n == want.size > 50 and hits.offsets.cpu().numpy()[:want.size].tolist() == want.tolist()
        for table in (first, second):
            assert table.n == n_lines and int(table.status.item()) == OK
            assert table.offsets.cpu().tolist() == starts.tolist() and table.lengths.cpu().tolist() == lens.tolist()
        idx.close()


def test_the_command_line_tool_finds_a_needle(tmp_path):
    """tools/tsq_cli f: the hit count and the first hit's offset"""
    import json
    import os
    import subprocess
    case = fg.chunk_edges("text_3")
    packed = tmp_path / "in.tsq"
    packed.write_bytes(case.index.blob)
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tsq_cli")
    for needle in (case.needle.decode("latin-1"), "ef ", "no such text"):
        r = subprocess.run([cli, "f", str(packed), needle], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        want = fg.item_hits(case.index.data, needle.encode("latin-1"))
        assert json.loads(r.stdout) == dict(bytes=case.index.total, needle_bytes=len(needle), hits=int(want.size), first_hit=int(want[0]) if want.size else None)
    assert subprocess.run([cli, "f", str(packed), "x" * 17], capture_output=True, text=True, timeout=300).returncode != 0


def test_the_python_wrapper_measures_then_fills(codec, tsq):
    import torch
    data, starts, lens = lines(tsq, 700, 120, 33)
    blob = codec.compress(to_dev(data), 1)
    idx = codec.index(blob)
    want = fg.item_hits(data.tobytes(), b" ef ")
    table = idx.find(b" ef ")
    assert table.n == want.size > 10 and int(table.status.item()) == OK and table.needle_len == 4 and not table.flat
    assert table.offsets.cpu().tolist() == want.tolist() and table.items.cpu().tolist() == [0] * want.size and table.item_first.cpu().tolist() == [0, want.size]
    short = idx.find(b" ef ", cap_hits=10)
    assert int(short.status.item()) == ERR_OVERFLOW and short.n == want.size and short.offsets.cpu().tolist() == want[:10].tolist()
    none = idx.find(b"\xff\xfe\xfd")
    assert none.n == 0 and none.offsets.numel() == 0 and int(none.status.item()) == OK
    for bad in (b"", b"x" * 17):
        with pytest.raises(tsq.TsqError) as err:
            idx.find(bad)
        assert err.value.code == ERR_ARG
    recs = idx.records(keep_delim=True)
    with pytest.raises(ValueError):
        recs.containing(idx.find(b" ef ", flat=True))
    with pytest.raises(ValueError):
        idx.records(flat=True).containing(table)
    sel = idx.records(keep_delim=True, flat=True).containing(idx.find(b" ef ", flat=True))
    torch.cuda.synchronize()
    assert sel.cpu().tolist() == [k for k, _ in grep(data.tobytes(), b" ef ")]
    fm, fn, tm, tn = codec.profile_read_find()
    assert (fn, tn) == (0, 0)
    idx.close()
