"""GPU tests of the gather into fixed-stride padded rows (tsqa_gather_rows_async, tsqa_gather_rows, DeviceCodec.gather_rows_async,
RangeIndex.gather_rows, BatchIndex.gather_rows): the cases are rowsgen's, the expected lengths, verdicts, need words and the whole
padded image are made there in pure Python, and test_rows_cpu.py shows that each case reaches what it aims at.  Every call runs on a
side stream with its tables uploaded as tensors; the output and every table the library may write sit between fences and are
filled with a sentinel first, and the WHOLE buffer is compared: the image, where pad -1 must leave the sentinel in every byte that
is no row's data, and both fences."""
import ctypes as C

import numpy as np
import pytest

import gathergen as gg
import rowsgen as rg
from test_gpu_cut import FENCE, Table, sentinel, to_dev, u64_dev
from test_gpu_gather import index_of, u32_dev

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = rg.OK, rg.ERR_ARG, rg.ERR_FORMAT, rg.ERR_OVERFLOW
SPARE_PIECES = 100              # slots past the pieces needed, which get the key that sorts behind every piece


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
    """the call's outputs: fenced tables, and a fenced output of n * stride bytes that starts `skew` bytes past a multiple of 16"""

    def __init__(self, n, size, skew=0):
        import torch
        self.row_lengths, self.row_status = Table(n, torch.int64), Table(n, torch.int32)
        self.need, self.word = Table(2, torch.int64), Table(1, torch.int32)
        self.size, self.at = size, FENCE + skew
        self.buf = to_dev(sentinel(2 * FENCE + 16 + size))
        assert self.buf.data_ptr() % 16 == 0

    def out_ptr(self):
        return self.buf.data_ptr() + self.at

    def tables(self):
        return (self.row_lengths, self.row_status, self.need, self.word)


class Tables:
    """a case's tables as device tensors, None where the case has none"""

    def __init__(self, case):
        self.items = None if case.items is None else u32_dev(case.items)
        self.offsets = None if case.offsets is None else u64_dev(case.offsets)
        self.lengths = None if case.lengths is None else u64_dev(case.lengths)


def rows_call(codec, index, t, case, pad, cap_pieces, room, sync=False, over=()):
    """tsqa_gather_rows_async (sync: tsqa_gather_rows) on the current stream -> its return value.  over: arguments replaced."""
    ptr = lambda x: x.data_ptr() if x is not None else None
    a = dict(ctx=codec.h, idx=index.h, items=ptr(t.items), offsets=ptr(t.offsets), lengths=ptr(t.lengths), n=case.n, stride=case.stride,
             flags=case.flags, pad=pad, cap_pieces=cap_pieces, out=room.out_ptr(), out_cap=room.size, row_lengths=room.row_lengths.ptr(),
             row_status=room.row_status.ptr(), need=room.need.ptr(), status=room.word.ptr())
    a.update(dict(over))
    f = codec.L.tsqa_gather_rows if sync else codec.L.tsqa_gather_rows_async
    return f(a["ctx"], a["idx"], a["items"], a["offsets"], a["lengths"], a["n"], a["stride"], a["flags"], a["pad"], a["cap_pieces"], a["out"],
             a["out_cap"], a["row_lengths"], a["row_status"], a["need"], a["status"], codec._stream())


def check_tables(room, e, what):
    got = room.row_status.values()
    assert got == e["row_status"], f"{what}: row statuses {[(k, g, w) for k, (g, w) in enumerate(zip(got, e['row_status'])) if g != w][:8]} (row, got, owed)"
    got = room.row_lengths.values()
    assert got == e["row_lengths"], f"{what}: row lengths {[(k, g, w) for k, (g, w) in enumerate(zip(got, e['row_lengths'])) if g != w][:8]} (row, got, owed)"
    assert room.need.values() == e["need"], f"{what}: d_need is {room.need.values()}, owed {e['need']}"
    assert room.word.values() == [e["status"]], f"{what}: *d_status is {room.word.values()}, owed {e['status']}"


def check(case, room, e, pad, what, data=None):
    """the tables, and every byte of the fenced buffer: the padded image and both fences"""
    check_tables(room, e, what)
    want = sentinel(room.buf.numel())
    want[room.at:room.at + room.size] = case.image(e, pad, want[room.at:room.at + room.size], data)
    host = room.buf.cpu().numpy()
    if not np.array_equal(host, want):
        at = int(np.flatnonzero(host != want)[0]) - room.at
        raise AssertionError(f"{what}: byte {at} of the output (row {at // case.stride}, byte {at % case.stride} of it; the output is {room.size} B at "
                             f"residue {room.at % 16}) is {int(host[at + room.at])} for {int(want[at + room.at])}")
    return host


def run(codec, side, case, pad=0xA5, cap_pieces=None, skew=0, what="", index=None, data=None):
    """one call on the side stream, checked against rowsgen -> (Room, expectation)"""
    import torch
    spare = cap_pieces is None
    cap_pieces = case.expect()["need"][0] + SPARE_PIECES if spare else cap_pieces
    e = case.expect(cap_pieces)
    index = index or index_of(codec, case.index)
    room, t = Room(case.n, case.n * case.stride, skew), Tables(case)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rc = rows_call(codec, index, t, case, pad, cap_pieces, room)
    assert rc == 0, codec.last_error()
    side.synchronize()
    check(case, room, e, pad, f"{what or case.name} (pad {pad}, residue {skew})", data)
    return room, e


@pytest.mark.parametrize("k", range(len(rg.COUNTS)))
def test_row_counts(codec, side, k):
    run(codec, side, rg.counts()[k], pad=rg.PADS[k % 3], skew=k)


@pytest.mark.parametrize("n", rg.REPEATS)
def test_the_second_pass_of_the_group_scan(codec, side, n):
    case = rg.repeated(n)
    room, e = run(codec, side, case, pad=0, cap_pieces=case.expect()["need"][0], skew=n % 16)
    assert e["status"] == OK and e["fit_pieces"] == e["need"][0]


@pytest.mark.parametrize("stride", rg.STRIDES)
def test_strides_at_every_residue(codec, side, stride):
    """lengths 0, 1, stride - 1, stride and stride + 1, with and without truncation, the output at every residue of a 16-byte word,
    the three pads taking turns"""
    for truncate in (False, True):
        for skew in rg.RESIDUES:
            run(codec, side, rg.strided(stride, truncate), pad=rg.PADS[(skew + truncate) % 3], skew=skew)


@pytest.mark.parametrize("k", range(8))
def test_null_tables(codec, side, k):
    case = rg.null_tables()[k]
    for pad, skew in ((0xA5, 0), (-1, 7)):
        run(codec, side, case, pad=pad, skew=skew)


@pytest.mark.parametrize("name", rg.REFUSALS)
def test_refused_rows(codec, side, name):
    for at in gg.REFUSAL_AT:
        room, e = run(codec, side, rg.refusal(name, at), pad=0, skew=at % 16)
        assert e["row_status"][at] == ERR_ARG and e["status"] == ERR_ARG


def test_a_too_long_row_is_refused_alone(codec, side):
    for pad in rg.PADS:
        room, e = run(codec, side, rg.too_long(), pad=pad, skew=3)
    assert e["status"] == ERR_OVERFLOW and room.row_lengths.values() == [10, 0, 40, 0, 0, 5, 0]


@pytest.mark.parametrize("k", range(4))
def test_rooms(codec, side, k):
    what, case, cap = rg.rooms()[k]
    room, e = run(codec, side, case, pad=0xA5, cap_pieces=cap, skew=5, what=what)
    assert e["status"] == (OK if k == 0 else ERR_OVERFLOW), what


def test_a_refused_sized_index_gives_format_and_padding(codec, side):
    import torch
    case = rg.refused_case()
    with torch.cuda.stream(side):
        idx = index_of(codec, case.index)                     # (made on the side stream, nothing waited for: the call reads its verdict)
    for pad in (0xA5, -1):
        room, e = run(codec, side, case, pad=pad, cap_pieces=64, skew=9, index=idx)
        assert room.row_status.values() == [ERR_FORMAT] * case.n and room.word.values() == [ERR_FORMAT] and room.need.values() == [0, 0]


def test_the_measuring_call(codec, side):
    import torch
    for case in (rg.counts()[4], rg.strided(40, False), rg.strided(40, True), rg.null_tables()[4]):
        room, t = Room(case.n, case.n * case.stride), Tables(case)
        idx = index_of(codec, case.index)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            rc = rows_call(codec, idx, t, case, 0xA5, 1, room, over=dict(out=None, out_cap=0))
        assert rc == 0, codec.last_error()
        side.synchronize()
        e, full = case.expect(1), case.expect()
        check_tables(room, e, case.name)
        assert room.need.values() == full["need"], "the need words do not depend on the room"
        assert np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel())), "a measuring call wrote to the output"


def test_arguments_refused_on_the_host(codec, side):
    import torch
    case = rg.counts()[2]
    idx = index_of(codec, case.index)
    t = Tables(case)
    torch.cuda.synchronize()
    for what, over in (("null index", dict(idx=None)), ("null row_lengths", dict(row_lengths=None)), ("null row_status", dict(row_status=None)),
                       ("null need", dict(need=None)), ("null status", dict(status=None)), ("stride 0", dict(stride=0)),
                       ("cap_pieces 0", dict(cap_pieces=0)), ("unknown flags", dict(flags=2)), ("unknown flags", dict(flags=0x80000001)),
                       ("pad 256", dict(pad=256)), ("pad -2", dict(pad=-2)), ("out_cap one short", dict(out_cap=case.n * case.stride - 1)),
                       ("rows times stride at 2^55", dict(stride=(1 << 55) // case.n, out=None, out_cap=0))):
        for sync in (False, True):
            room = Room(case.n, case.n * case.stride)
            with torch.cuda.stream(side):
                rc = rows_call(codec, idx, t, case, 0, 64, room, sync=sync, over=over)
            side.synchronize()
            assert rc == ERR_ARG, (what, rc)
            assert all(tab.untouched() for tab in room.tables()) and np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel())), what
    # no rows: the words are cleared and nothing else is touched
    room = Room(0, 64)
    with torch.cuda.stream(side):
        rc = rows_call(codec, idx, t, case, 0, 8, room, sync=True, over=dict(n=0))
    assert rc == OK and room.word.values() == [0] and room.need.values() == [0, 0]
    assert np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel()))
    # the waiting form returns the largest row status
    case = rg.too_long()
    room = Room(case.n, case.n * case.stride)
    with torch.cuda.stream(side):
        rc = rows_call(codec, index_of(codec, case.index), Tables(case), case, 0, 64, room, sync=True)
    assert rc == ERR_OVERFLOW
    check(case, room, case.expect(64), 0, "the waiting form")


def test_the_dense_gather_reads_the_same_bytes(codec, side):
    """the delivered rows, as ranges of the dense gather through the same index: the same data bytes"""
    import torch
    for case in (rg.counts()[5], rg.strided(4097, True), rg.strided(17, True), rg.null_tables()[5]):
        e = case.expect()
        idx = index_of(codec, case.index)
        room, _ = run(codec, side, case, pad=0)
        offsets, lengths = case.dense_ranges(e)
        need = sum(lengths)
        dense = to_dev(sentinel(need + FENCE))
        offs, st, pieces = Table(case.n + 1, torch.int64), Table(case.n, torch.int32), Table(1, torch.int64)
        with torch.cuda.stream(side):
            codec.gather_async(idx, None, u64_dev(offsets), u64_dev(lengths), case.n, 1, e["need"][0] + SPARE_PIECES, dense[:max(need, 1)], offs.t, st.t, pieces.t,
                               out_cap=need)
        side.synchronize()
        assert st.values() == [OK] * case.n and pieces.values() == [e["fit_pieces"]] and codec.status() == OK
        places, host, rows = offs.values(), dense.cpu().numpy(), room.buf.cpu().numpy()[room.at:room.at + room.size].reshape(case.n, case.stride)
        for k, ln in enumerate(lengths):
            assert np.array_equal(host[places[k]:places[k] + ln], rows[k, :ln]), (case.name, k)
        assert np.array_equal(host[need:], sentinel(host.size)[need:])


def test_the_python_wrappers(codec, tsq, side):
    import torch
    data = tsq.synth.text(40 * 4096 + 33, seed=91)
    blob, table = codec.compress_split(to_dev(data), 1, 4096, block_sizes=True)
    offsets, lengths = [5, 4090, 100000, data.size - 7, data.size, 0, 8000], [100, 5000, 0, 7, 1, data.size + 1, 128]
    d_off, d_len = u64_dev(offsets), u64_dev(lengths)
    for idx in (codec.index(blob), codec.index_sized(blob, data.size, 4096, table)):
        rows, lens, st = idx.gather_rows(d_off, d_len, 128, pad=0x20, row_status=True)
        torch.cuda.synchronize()
        assert tuple(rows.shape) == (7, 128) and rows.dtype == torch.uint8
        assert st.cpu().tolist() == [0, ERR_OVERFLOW, 0, 0, ERR_ARG, ERR_ARG, 0] and codec.status() == ERR_OVERFLOW
        assert lens.cpu().tolist() == [100, 0, 0, 7, 0, 0, 128]
        want = np.full((7, 128), 0x20, dtype=np.uint8)
        for k, (o, ln) in enumerate(zip(offsets, lens.cpu().tolist())):
            want[k, :ln] = data[o:o + ln]
        assert np.array_equal(rows.cpu().numpy(), want)
        # truncation, the room given: nothing is measured, nothing is waited for on a stream of the caller's
        out = torch.full((7 * 128 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side):
            rows2, lens2 = idx.gather_rows(d_off, d_len, 128, pad=-1, truncate=True, out=out, cap_pieces=32)
        side.synchronize()
        assert rows2.data_ptr() == out.data_ptr() and lens2.cpu().tolist() == [100, 128, 0, 7, 0, 0, 128] and codec.status() == ERR_ARG
        want = np.full(out.numel(), 0xEE, dtype=np.uint8)
        for k, (o, ln) in enumerate(zip(offsets, lens2.cpu().tolist())):
            want[k * 128:k * 128 + ln] = data[o:o + ln]
        assert np.array_equal(out.cpu().numpy(), want)
        # no rows: empty results, not a refusal
        none, no_lens = idx.gather_rows(d_off[:0], d_len[:0], 16)
        torch.cuda.synchronize()
        assert tuple(none.shape) == (0, 16) and no_lens.numel() == 0 and codec.status() == 0
        for bad in ((d_off.to(torch.int32), d_len, 16), (d_off, d_len[:3], 16), (d_off.cpu(), d_len, 16), (d_off, d_len, 0), (None, None, 16)):
            with pytest.raises(tsq.TsqError) as err:
                idx.gather_rows(*bad)
            assert err.value.code == ERR_ARG
        idx.close()
    parts = [tsq.synth.text(n, seed=92 + n) for n in (10, 5000, 300)]
    bidx = codec.index_batch([codec.compress(to_dev(p), 1) for p in parts])
    rows, lens, st = bidx.gather_rows(u32_dev([2, 0, 1, 3]), row_stride=512, row_status=True)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, 0, ERR_OVERFLOW, ERR_ARG] and lens.cpu().tolist() == [300, 10, 0, 0]
    host = rows.cpu().numpy()
    assert bytes(host[0, :300]) == parts[2].tobytes() and bytes(host[1, :10]) == parts[0].tobytes() and not host[2:].any() and not host[0, 300:].any()
    rows, lens = bidx.gather_rows(u32_dev([1, 2]), row_stride=64, truncate=True, pad=7)
    torch.cuda.synchronize()
    assert lens.cpu().tolist() == [64, 64] and bytes(rows.cpu().numpy().tobytes()) == parts[1][:64].tobytes() + parts[2][:64].tobytes()
    rows, lens = bidx.gather_rows(u32_dev([1, 0]), u64_dev([4990, 2]), u64_dev([10, 8]), row_stride=16, pad=9)
    torch.cuda.synchronize()
    assert bytes(rows.cpu().numpy().tobytes()) == parts[1][4990:].tobytes() + bytes([9] * 6) + parts[0][2:].tobytes() + bytes([9] * 8)


def test_one_chain_on_one_stream(codec, tsq, side):
    """split compress -> sized index -> row numbers drawn on the device -> gather_rows -> a second gather_rows whose offsets are read
    from the first one's rows: one stream, no synchronise, nothing about the rows on the host.  Twice back to back, the second time
    with more rows and a cap_pieces that make the scratch grow."""
    import torch
    bl, rec, stride = 4096, 100, 128
    runs = []
    for n_recs, m, cap, seed in ((3000, 500, 1200, 83), (9000, 2500, 700000, 84)):
        data = tsq.synth.text(n_recs * rec, seed=seed)
        runs.append(dict(data=data, src=to_dev(data), n_recs=n_recs, m=m, cap=cap))
    for r in runs:
        m, (nb, room) = r["m"], tsq.plan_split(r["src"].numel(), bl)
        r["blob"], r["table"] = to_dev(sentinel(room)), torch.full((nb,), -1, dtype=torch.int32, device="cuda")
        r["out1"], r["out2"] = to_dev(sentinel(m * stride + FENCE)), to_dev(sentinel(m * stride + FENCE))
        i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device="cuda")
        r["len1"], r["len2"], r["need1"], r["need2"] = i64(m), i64(m), i64(2), i64(2)
        r["st1"], r["st2"] = (torch.full((m,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        r["words"] = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4343)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for r in runs:
            m, w = r["m"], r["words"]
            codec.compress_split_async(r["src"], 1, bl, r["blob"], r["table"])
            w[0:1].copy_(codec._status)
            r["idx"] = codec.index_sized(r["blob"], r["src"].numel(), bl, r["table"], sync=False)
            r["rows"] = torch.randint(0, r["n_recs"], (m,), device="cuda", generator=gen)
            r["lens"] = 1 + (r["rows"] * 37) % rec                # records of 1 to 100 bytes
            codec.gather_rows_async(r["idx"], None, r["rows"] * rec, r["lens"], m, stride, 0, 0, r["cap"], r["out1"][:m * stride], r["len1"], r["st1"], r["need1"])
            w[1:2].copy_(codec._status)
            # the next rows from the bytes just read: the first byte of every row and its padding's last
            first = r["out1"][:m * stride].view(m, stride).to(torch.int64)
            r["rows2"] = (first[:, 0] * 251 + first[:, stride - 1] + torch.arange(m, device="cuda")) % r["n_recs"]
            codec.gather_rows_async(r["idx"], None, r["rows2"] * rec, None, m, stride, rg.TRUNCATE, 0xA5, r["cap"], r["out2"][:m * stride], r["len2"], r["st2"],
                                    r["need2"])
            w[2:3].copy_(codec._status)
    side.synchronize()
    for r in runs:
        m, data = r["m"], r["data"]
        assert r["words"].cpu().tolist()[:3] == [0, 0, 0]
        assert r["st1"].cpu().tolist() == [0] * m and r["st2"].cpu().tolist() == [0] * m
        rows = r["rows"].cpu().numpy()
        lens = 1 + (rows * 37) % rec
        assert np.array_equal(r["len1"].cpu().numpy(), lens)
        want = np.zeros((m, stride), dtype=np.uint8)
        for k in range(m):
            want[k, :lens[k]] = data[rows[k] * rec:rows[k] * rec + lens[k]]
        out1 = r["out1"].cpu().numpy()
        assert np.array_equal(out1[:m * stride].reshape(m, stride), want) and np.array_equal(out1[m * stride:], sentinel(out1.size)[m * stride:])
        rows2 = (want[:, 0].astype(np.int64) * 251 + np.arange(m)) % r["n_recs"]
        assert np.array_equal(r["rows2"].cpu().numpy(), rows2)
        # lengths NULL: to the end of the data, truncated to the stride (the last record's row is shorter)
        lens2 = np.minimum(data.size - rows2 * rec, stride)
        assert np.array_equal(r["len2"].cpu().numpy(), lens2)
        want2 = np.full((m, stride), 0xA5, dtype=np.uint8)
        for k in range(m):
            want2[k, :lens2[k]] = data[rows2[k] * rec:rows2[k] * rec + lens2[k]]
        out2 = r["out2"].cpu().numpy()
        assert np.array_equal(out2[:m * stride].reshape(m, stride), want2) and np.array_equal(out2[m * stride:], sentinel(out2.size)[m * stride:])
        pieces = lambda at, ln: int(sum(1 + ((int(a) + int(n) - 1) // bl > int(a) // bl) for a, n in zip(at, ln)))
        assert r["need1"].cpu().tolist() == [pieces(rows * rec, lens), int(lens.max())]
        assert r["need2"].cpu().tolist() == [pieces(rows2 * rec, lens2), int((data.size - rows2 * rec).max())]
        r["idx"].close()


def test_a_batch_index_made_on_the_device_and_not_fetched(tsq, side):
    """compress_batch_packed_async -> index_packed_async -> gather_rows by item, on one stream with no synchronise: the host knows
    neither the index's blocks nor its total, and the rows call reads both on the device.  Whole items, truncated ones, ranges, and
    items that do not exist."""
    import torch
    fresh = tsq.DeviceCodec(0)
    try:
        n_items, stride = 280, 4096
        rng = np.random.default_rng(rg.SEED + 9)
        sizes = [int(x) for x in rng.integers(200, 9000, n_items)]
        data = tsq.synth.text(sum(sizes), seed=12)
        starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
        items = list(range(n_items - 1, -1, -1)) + [n_items, (1 << 32) - 1]
        n = len(items)
        with torch.cuda.stream(side):
            arena = torch.empty(sum(tsq.batch_bound(z) + 16 for z in sizes), dtype=torch.uint8, device="cuda")
            d_offsets, d_sizes = torch.empty(n_items + 1, dtype=torch.int64, device="cuda"), torch.empty(n_items, dtype=torch.int64, device="cuda")
            fresh.compress_batch_packed_async(to_dev(data), list(zip(starts, sizes)), 1, 16, arena, d_offsets, d_sizes)
            index = fresh.index_packed_async(arena, d_offsets, d_sizes, n_items, n_items)
            d_items = u32_dev(items)
            whole = index.gather_rows(d_items, row_stride=stride, pad=0xA5, out=to_dev(sentinel(n * stride + FENCE)), cap_pieces=n, row_status=True)
            st_whole = fresh._status.clone()
            cut = index.gather_rows(d_items, row_stride=stride, pad=-1, truncate=True, out=to_dev(sentinel(n * stride + FENCE)), cap_pieces=n, row_status=True)
            st_cut = fresh._status.clone()
            part = index.gather_rows(d_items, u64_dev([50] * n), u64_dev([150] * n), row_stride=160, pad=0, out=to_dev(sentinel(n * 160 + FENCE)),
                                     cap_pieces=n, row_status=True)
            st_part = fresh._status.clone()
        side.synchronize()
        assert [int(s.item()) for s in (st_whole, st_cut, st_part)] == [ERR_OVERFLOW, ERR_ARG, ERR_ARG]
        for (rows, lens, st), truncate, pad, width in ((whole, False, 0xA5, stride), (cut, True, -1, stride), (part, None, 0, 160)):
            base = rows.data_ptr()
            got, lens, st = rows.cpu().numpy(), lens.cpu().tolist(), st.cpu().tolist()
            fill = sentinel(n * width + FENCE)
            for k, i in enumerate(items):
                row = fill[k * width:(k + 1) * width].copy()
                if i >= n_items:
                    want_st, want = ERR_ARG, b""
                elif truncate is None:
                    want_st, want = OK, data[starts[i] + 50:starts[i] + 200]
                elif sizes[i] > width and not truncate:
                    want_st, want = ERR_OVERFLOW, b""
                else:
                    want_st, want = OK, data[starts[i]:starts[i] + min(sizes[i], width)]
                assert st[k] == want_st and lens[k] == len(want), (k, i, st[k], lens[k])
                if pad >= 0:
                    row[:] = pad
                row[:len(want)] = np.frombuffer(bytes(want), dtype=np.uint8)
                assert np.array_equal(got[k], row), (truncate, k, i)
            assert base % 16 == 0
        index.close()
    finally:
        fresh.close()


def test_between_the_older_calls_that_share_the_scratch(codec, tsq, side):
    """on one stream with nothing waited for: rows, a dense gather, rows, a take, rows, a dense decompress, rows -- every call through
    the same context, and every result checked"""
    import torch
    batch = gg.batch()
    idx = index_of(codec, batch)
    cases = [rg.null_tables()[4], rg.refusal("item_is_items", 256), rg.null_tables()[5], rg.null_tables()[7]]
    rooms = [(c, Room(c.n, c.n * c.stride, skew), Tables(c), pad) for c, skew, pad in zip(cases, (0, 5, 11, 15), (0xA5, 0, -1, 0x5A))]
    healthy = list(range(16))
    assert not set(healthy) & set(gg.BATCH_DAMAGE)
    dense_case = gg.batch_flat()
    de = dense_case.expect()
    dense_out = to_dev(sentinel(de["need"] + FENCE))
    d_offs, d_st, d_need = Table(dense_case.n + 1, torch.int64), Table(dense_case.n, torch.int32), Table(1, torch.int64)
    d_tables = (u64_dev(dense_case.offsets), u64_dev(dense_case.lengths))
    spans = [batch.spans[i] for i in healthy]
    take_room = sum((n + 15) // 16 * 16 for _, n in spans)
    take_out = to_dev(sentinel(take_room + FENCE))
    t_offs, t_sizes, t_st = Table(len(healthy) + 1, torch.int64), Table(len(healthy), torch.int64), Table(len(healthy), torch.int32)
    t_items = u32_dev(healthy)
    arena = index_of(codec, batch).blob
    a_offs, a_sizes = u64_dev([o for o, _ in spans]), u64_dev([n for _, n in spans])
    totals = [batch.item_span(i)[1] for i in healthy]
    dec_out = to_dev(sentinel(sum(totals) + FENCE))
    x_offs, x_sizes, x_first, x_st = (Table(len(healthy) + 1, torch.int64), Table(len(healthy), torch.int64), Table(len(healthy) + 1, torch.int64),
                                      Table(len(healthy), torch.int32))
    words = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        def rows(j):
            c, room, t, pad = rooms[j]
            assert rows_call(codec, idx, t, c, pad, c.expect()["need"][0] + SPARE_PIECES, room) == 0, codec.last_error()
        rows(0)
        codec.gather_async(idx, None, d_tables[0], d_tables[1], dense_case.n, 1, de["need_pieces"] + 7, dense_out[:de["need"]], d_offs.t, d_st.t, d_need.t)
        words[0:1].copy_(codec._status)
        rows(1)
        codec.cut_items_async(idx, t_items, None, None, len(healthy), 16, take_out[:take_room], t_offs.t, t_sizes.t, None, t_st.t)
        words[1:2].copy_(codec._status)
        rows(2)
        codec.decompress_batch_packed_dense_async(arena, a_offs, a_sizes, len(healthy), 64, 1, dec_out[:sum(totals)], x_offs.t, x_sizes.t, x_first.t, x_st.t)
        words[2:3].copy_(codec._status)
        rows(3)
    side.synchronize()
    assert words.cpu().tolist()[:3] == [0, 0, 0]
    for c, room, t, pad in rooms:
        check(c, room, c.expect(), pad, c.name)
    # the dense gather
    assert d_st.values() == de["range_status"] and d_offs.values() == de["out_offsets"] and d_need.values() == [de["need_pieces"]]
    fill = sentinel(dense_out.numel())
    want = fill.copy()
    want[:de["need"]] = dense_case.output(de, fill[:de["need"]])
    assert np.array_equal(dense_out.cpu().numpy(), want)
    # the take: every healthy item as a container of its own, byte for byte the one in the arena
    assert t_st.values() == [0] * len(healthy) and t_sizes.values() == [n for _, n in spans]
    places, host, src = t_offs.values(), take_out.cpu().numpy(), np.frombuffer(batch.blob, dtype=np.uint8)
    assert all(p % 16 == 0 for p in places[:-1])
    for p, (o, n) in zip(places, spans):
        assert np.array_equal(host[p:p + n], src[o:o + n])
    assert np.array_equal(host[take_room:], sentinel(host.size)[take_room:])
    # the dense decompress
    assert x_st.values() == [0] * len(healthy) and x_sizes.values() == totals
    host, at = dec_out.cpu().numpy(), 0
    assert x_offs.values() == [int(v) for v in np.cumsum([0] + totals)]
    for i, total in zip(healthy, totals):
        start, _ = batch.item_span(i)
        assert bytes(host[at:at + total]) == batch.data[start:start + total]
        at += total
    assert np.array_equal(host[at:], sentinel(host.size)[at:])
