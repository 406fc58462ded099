"""GPU tests of the gather (tsqa_gather_async, tsqa_gather, DeviceCodec.gather_async, RangeIndex.gather, BatchIndex.gather): the
cases are gathergen's, the expected places, verdicts and bytes are made there in pure Python from the sources' data, and
test_gather_cpu.py shows that each case reaches what it aims at.  Every call runs on a side stream with its tables uploaded as
tensors; the output and every table the library may write are filled with a sentinel first, with a fence on both sides, and must
keep it wherever the call owes nothing: padding, the room of ranges that are refused or do not fit, everything behind a refusal.
Each case also goes through the host-planned record read (tsqa_decompress_item_ranges; the flat form of a batch index through
tsqa_decompress_ranges) with the same ranges and the layout's places, and both outputs must be equal."""
import ctypes as C

import numpy as np
import pytest

import gathergen as gg
from test_gpu_cut import FENCE, Index, Table, sentinel, to_dev, u64_dev

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = gg.OK, gg.ERR_ARG, gg.ERR_FORMAT, gg.ERR_STREAM, gg.ERR_OVERFLOW
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


def u32_dev(values):
    """any 32-bit values as an int32 CUDA tensor"""
    return to_dev(np.array([int(v) for v in values], dtype=np.uint32).view(np.int32))


_INDEXES = {}


class BatchOf:
    """tsqa_index_create_batch over a gathergen batch, whose refused items the call reports and leaves out"""

    def __init__(self, codec, i: gg.Index, blob):
        import torch
        from turbosqueeze_amd.api import _batch_array
        self.codec, self.blob, self.h = codec, blob, C.c_void_p()
        status = (C.c_int32 * i.n_items)()
        torch.cuda.synchronize()
        rc = codec.L.tsqa_index_create_batch(codec.h, blob.data_ptr(), blob.numel(), _batch_array([(a, n, 0, 0) for a, n in i.spans]), i.n_items,
                                             C.byref(self.h), status)
        refused = [k for k in range(i.n_items) if i.item_first[k] == i.item_first[k + 1]]
        assert self.h and rc == (ERR_FORMAT if refused else OK), codec.last_error()
        assert [k for k in range(i.n_items) if status[k]] == refused and all(status[k] == ERR_FORMAT for k in refused)
        assert codec.L.tsqa_index_blocks(self.h) == i.n_blocks and codec.L.tsqa_index_total(self.h) == i.total


def index_of(codec, i: gg.Index):
    """-> the tsqa_index of a gathergen index, made once"""
    if i.name not in _INDEXES:
        blob = to_dev(np.frombuffer(i.blob, dtype=np.uint8))
        _INDEXES[i.name] = (Index(codec, "sized", blob, i.total, i.block_len, i.table) if i.kind == "sized" else
                            BatchOf(codec, i, blob) if i.kind == "batch" else Index(codec, "plain", blob))
    return _INDEXES[i.name]


class Room:
    """the call's outputs: fenced tables, and a fenced output of out_cap bytes"""

    def __init__(self, n, out_cap):
        import torch
        self.out_offsets, self.range_status = Table(n + 1, torch.int64), Table(n, torch.int32)
        self.need, self.word = Table(1, torch.int64), Table(1, torch.int32)
        self.out_cap, self.at = out_cap, FENCE
        self.buf = to_dev(sentinel(2 * FENCE + out_cap))

    def out_ptr(self):
        return self.buf.data_ptr() + self.at

    def tables(self):
        return (self.out_offsets, self.range_status, self.need, self.word)


class Tables:
    """a case's ranges as device tensors"""

    def __init__(self, case):
        self.items = None if case.items is None else u32_dev(case.items)
        self.offsets, self.lengths = u64_dev(case.offsets), u64_dev(case.lengths)


def gather_call(codec, index, t, n, align, cap_pieces, room, sync=False, over=()):
    """tsqa_gather_async (sync: tsqa_gather) on the current stream -> its return value.  over: arguments replaced."""
    a = dict(ctx=codec.h, idx=index.h, items=t.items.data_ptr() if t.items is not None else None, offsets=t.offsets.data_ptr(),
             lengths=t.lengths.data_ptr(), n=n, align=align, cap_pieces=cap_pieces, out=room.out_ptr(), out_cap=room.out_cap,
             out_offsets=room.out_offsets.ptr(), range_status=room.range_status.ptr(), need=room.need.ptr(), status=room.word.ptr())
    a.update(dict(over))
    f = codec.L.tsqa_gather if sync else codec.L.tsqa_gather_async
    return f(a["ctx"], a["idx"], a["items"], a["offsets"], a["lengths"], a["n"], a["align"], a["cap_pieces"], a["out"], a["out_cap"],
             a["out_offsets"], a["range_status"], a["need"], a["status"], codec._stream())


def check(case, room, e, what, data=None):
    """the tables, the statuses and every byte of the fenced output against gathergen's `e`"""
    got_status = room.range_status.values()
    assert got_status == e["range_status"], (f"{what}: range statuses "
                                             f"{[(k, g, w) for k, (g, w) in enumerate(zip(got_status, e['range_status'])) if g != w][:8]} (range, got, owed)")
    assert room.word.values() == [e["status"]], f"{what}: *d_status is {room.word.values()}, owed {e['status']}"
    got = room.out_offsets.values()
    assert got == e["out_offsets"], f"{what}: d_out_offsets {[(k, g, w) for k, (g, w) in enumerate(zip(got, e['out_offsets'])) if g != w][:8]} (range, got, owed)"
    assert room.need.values() == [e["need_pieces"]], f"{what}: *d_need_pieces is {room.need.values()}, owed {e['need_pieces']}"
    want = sentinel(room.buf.numel())
    want[room.at:room.at + room.out_cap] = case.output(e, want[room.at:room.at + room.out_cap], data)
    host = room.buf.cpu().numpy()
    if not np.array_equal(host, want):
        at = int(np.flatnonzero(host != want)[0]) - room.at
        k = int(np.searchsorted(np.array(e["out_offsets"]), at, side="right")) - 1
        raise AssertionError(f"{what}: byte {at} of the output is {int(host[at + room.at])} for {int(want[at + room.at])} (range {k} at "
                             f"{e['out_offsets'][max(k, 0)]}, out_cap {room.out_cap})")
    return host


def host_planned(codec, case, index, e, room, what):
    """the same fitting ranges through the host-planned record read, at the layout's places -> the fenced output"""
    import torch
    from turbosqueeze_amd.api import _item_range_array, _range_array
    quads = case.item_ranges(e)
    other = to_dev(sentinel(room.buf.numel()))
    ptr = other.data_ptr() + room.at
    torch.cuda.synchronize()
    if case.items is None and case.index.kind == "batch":
        triples = [(off, ln, at) for _, off, ln, at in quads]
        rc = codec.L.tsqa_decompress_ranges(codec.h, index.h, _range_array(triples), len(triples), ptr, room.out_cap, codec._stream())
    else:
        rc = codec.L.tsqa_decompress_item_ranges(codec.h, index.h, _item_range_array(quads), len(quads), ptr, room.out_cap, codec._stream())
    assert rc == 0, f"{what}: the host-planned read of the same ranges: {codec.last_error()}"
    torch.cuda.synchronize()
    return other.cpu().numpy()


def run(codec, side, case, out_cap=None, cap_pieces=None, what="", index=None, data=None, twin=True):
    """one call with this room on the side stream, checked against gathergen -> (Room, expectation)"""
    import torch
    e_all = case.expect()
    out_cap = e_all["need"] if out_cap is None else out_cap
    cap_pieces = e_all["need_pieces"] + SPARE_PIECES if cap_pieces is None else cap_pieces
    e = case.expect(out_cap, cap_pieces)
    index = index or index_of(codec, case.index)
    room, t = Room(case.n, out_cap), Tables(case)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rc = gather_call(codec, index, t, case.n, case.align, cap_pieces, room)
    assert rc == 0, codec.last_error()
    side.synchronize()
    host = check(case, room, e, what or case.name, data)
    if twin and e["fit_pieces"]:
        with torch.cuda.stream(side):
            other = host_planned(codec, case, index, e, room, what or case.name)
        assert np.array_equal(host, other), f"{what or case.name}: the gather and the host-planned read of the same ranges differ"
    return room, e


@pytest.mark.parametrize("k", range(len(gg.COUNTS)))
def test_range_counts(codec, side, k):
    run(codec, side, gg.counts()[k])


@pytest.mark.parametrize("align", gg.ALIGNS)
def test_alignments(codec, side, align):
    run(codec, side, gg.aligned(align))


def test_the_shift_and_the_bisection_read_the_same_bytes(codec, side):
    sized, plain = gg.shift_and_bisect()
    a, _ = run(codec, side, sized)
    b, _ = run(codec, side, plain)
    assert np.array_equal(a.buf.cpu().numpy(), b.buf.cpu().numpy())


@pytest.mark.parametrize("k", range(3))
def test_places_past_2_to_the_24(codec, side, k):
    run(codec, side, gg.carries()[k])


def test_one_range_over_everything(codec, side):
    run(codec, side, gg.whole())


@pytest.mark.parametrize("n", gg.ONE_BLOCK_COUNTS)
def test_many_ranges_inside_one_block(codec, side, n):
    run(codec, side, gg.one_block(n))


def test_a_shuffle_over_all_blocks(codec, side):
    run(codec, side, gg.shuffled())


def test_a_batch_index_by_item_and_flat(codec, side):
    run(codec, side, gg.batch_items())
    run(codec, side, gg.batch_flat())


@pytest.mark.parametrize("name", gg.REFUSALS)
def test_refused_ranges(codec, side, name):
    for at in gg.REFUSAL_AT:
        room, e = run(codec, side, gg.refusal(name, at))
        assert e["range_status"][at] == ERR_ARG and e["status"] == ERR_ARG


@pytest.mark.parametrize("k", range(6))
def test_rooms(codec, side, k):
    what, case, out_cap, cap_pieces = gg.rooms()[k]
    room, e = run(codec, side, case, out_cap, cap_pieces, what)
    assert e["status"] == (OK if k == 0 else ERR_OVERFLOW), what


def test_a_refused_sized_index_refuses_every_range(codec, side):
    import torch
    case = gg.refused_case()
    with torch.cuda.stream(side):
        idx = index_of(codec, case.index)                     # (made on the side stream, nothing waited for: the gather reads its verdict)
    room, e = run(codec, side, case, out_cap=4096, cap_pieces=64, index=idx)
    assert room.range_status.values() == [ERR_FORMAT] * case.n and room.word.values() == [ERR_FORMAT]


def test_block_numbers_of_17_bits(codec, tsq, side):
    """one container of 65 537 blocks of 4 096 bytes made on the GPU by the split compress; compared with slices of the input"""
    import torch
    case = gg.big_case()
    data = gg.big_input()
    src = to_dev(data)
    blob, table = codec.compress_split(src, 1, gg.BIG_LEN, block_sizes=True)
    idx = codec.index_sized(blob, data.size, gg.BIG_LEN, table)
    assert idx.n_blocks == gg.BIG_BLOCKS
    try:
        run(codec, side, case, index=idx, data=data)
    finally:
        torch.cuda.synchronize()
        idx.close()


STREAM_TWINS = 4                # the catalogue's first invalid twins that only a decoder refuses: one at each of the places 0, 2, 3 and 5


def test_a_malformed_stream_raises_the_status_to_err_stream(codec, side):
    """mtgen's twin containers: six well-formed frames of which one holds a stream the decoder refuses in its first chunk, so the
    index is made and the read of that block meets the damage.  The decoders report into a word of their own and the last launch
    raises *d_status to TSQA_ERR_STREAM, as the host-planned read of the same ranges reports it; the verdicts per range stay 0,
    nothing outside the destinations is written, and beside a range that does not fit the status stays TSQA_ERR_OVERFLOW."""
    import torch
    import cutgen as cg
    import mtgen
    from turbosqueeze_amd.api import _item_range_array
    twins = [t for t in mtgen.twin_containers() if t[3] == "stream"][:STREAM_TWINS]
    assert sorted(k for _, _, k, _ in twins) == [0, 2, 3, 5]
    for name, blob, k, _ in twins:
        _, out_start = cg.walk(blob)
        i = gg.Index(name, "plain", blob, None, out_start)
        idx = Index(codec, "plain", to_dev(np.frombuffer(blob, dtype=np.uint8)))
        healthy = (k + 1) % 6
        case = gg.Case(name, i, [out_start[k], out_start[healthy] + 10, out_start[k] + 1], [out_start[k + 1] - out_start[k], 700, 50], align=16)
        e = case.expect()
        assert e["status"] == OK and {b for b, _, _, _ in e["items"]} == {k, healthy}
        for out_cap, want in ((e["need"], ERR_STREAM), (e["need"] - 1, ERR_OVERFLOW)):
            room, t = Room(case.n, out_cap), Tables(case)
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                assert gather_call(codec, idx, t, case.n, 16, 8, room) == 0, codec.last_error()
            side.synchronize()
            fit = case.expect(out_cap, 8)
            assert room.word.values() == [want], (name, out_cap, room.word.values())
            assert room.range_status.values() == fit["range_status"] and room.out_offsets.values() == e["out_offsets"], name
            host, fill = room.buf.cpu().numpy(), sentinel(room.buf.numel())
            owed = np.zeros(host.size, dtype=bool)
            for o, (_, ln) in zip(fit["out_offsets"], fit["places"]):
                owed[room.at + o:room.at + o + ln] = True
            assert np.array_equal(host[~owed], fill[~owed]), f"{name}: a byte outside the destinations was written"
        other = to_dev(sentinel(room.buf.numel()))
        rc = codec.L.tsqa_decompress_item_ranges(codec.h, idx.h, _item_range_array(case.item_ranges(e)), case.n, other.data_ptr() + FENCE, e["need"],
                                                 codec._stream())
        torch.cuda.synchronize()
        assert rc == ERR_STREAM, f"{name}: the host-planned read of the same ranges reports {rc}"
        idx.close()


def test_arguments_refused_on_the_host(codec, side):
    import torch
    case = gg.counts()[2]
    idx = index_of(codec, case.index)
    t = Tables(case)
    torch.cuda.synchronize()
    for what, over in (("null index", dict(idx=None)), ("null offsets", dict(offsets=None)), ("null lengths", dict(lengths=None)),
                       ("null output", dict(out=None)), ("null out_offsets", dict(out_offsets=None)), ("null range_status", dict(range_status=None)),
                       ("null need_pieces", dict(need=None)), ("null status", dict(status=None)), ("align 0", dict(align=0)),
                       ("align 24", dict(align=24)), ("align 8192", dict(align=8192)), ("cap_pieces 0", dict(cap_pieces=0))):
        for sync in (False, True):
            room = Room(case.n, 256)
            with torch.cuda.stream(side):
                rc = gather_call(codec, idx, t, case.n, 1, 64, room, sync=sync, over=over)
            side.synchronize()
            assert rc == ERR_ARG, (what, rc)
            assert all(tab.untouched() for tab in room.tables()) and np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel())), what
    # d_items with an index of one item is allowed: only item 0 exists
    room = Room(2, 64)
    with torch.cuda.stream(side):
        rc = gather_call(codec, idx, Tables(gg.Case("one_item", case.index, [0, 0], [4, 4], items=[0, 1])), 2, 1, 8, room, sync=True)
    assert rc == ERR_ARG and room.range_status.values() == [OK, ERR_ARG] and room.out_offsets.values() == [0, 4, 4]
    # no ranges: the words are cleared and nothing else is touched
    room = Room(0, 64)
    with torch.cuda.stream(side):
        rc = gather_call(codec, idx, t, 0, 1, 8, room, sync=True)
    assert rc == OK and room.word.values() == [0] and room.need.values() == [0] and room.out_offsets.values() == [0]
    assert np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel()))


def test_one_chain_on_one_stream(codec, tsq, side):
    """split compress -> sized index -> row numbers drawn on the device -> offsets by a multiply -> gather -> a second gather whose
    offsets are computed from the first one's output bytes: one stream, no synchronise, nothing about the ranges on the host.  Twice
    back to back, the second time with a cap_pieces that makes the scratch grow."""
    import torch
    bl, rec = 4096, 100
    runs = []
    for n_rows, m, cap, seed in ((3000, 500, 1200, 81), (9000, 2500, 700000, 82)):
        data = tsq.synth.text(n_rows * rec, seed=seed)
        runs.append(dict(data=data, src=to_dev(data), n_rows=n_rows, m=m, cap=cap))
    for r in runs:
        m, (nb, room) = r["m"], tsq.plan_split(r["src"].numel(), bl)
        r["blob"], r["table"] = to_dev(sentinel(room)), torch.full((nb,), -1, dtype=torch.int32, device="cuda")
        r["out1"], r["out2"] = to_dev(sentinel(m * rec + FENCE)), to_dev(sentinel(m * rec + FENCE))
        i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device="cuda")
        r["offs1"], r["offs2"], r["need"] = i64(m + 1), i64(m + 1), i64(2)
        r["st1"], r["st2"] = (torch.full((m,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        r["words"] = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        r["lengths"] = torch.full((m,), rec, dtype=torch.int64, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4242)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for r in runs:
            m, w = r["m"], r["words"]
            codec.compress_split_async(r["src"], 1, bl, r["blob"], r["table"])
            w[0:1].copy_(codec._status)
            r["idx"] = codec.index_sized(r["blob"], r["src"].numel(), bl, r["table"], sync=False)
            r["rows"] = torch.randint(0, r["n_rows"], (m,), device="cuda", generator=gen)
            codec.gather_async(r["idx"], None, r["rows"] * rec, r["lengths"], m, 1, r["cap"], r["out1"][:m * rec], r["offs1"], r["st1"], r["need"][0:1])
            w[1:2].copy_(codec._status)
            # the next rows from the bytes just read: the first two bytes of every record
            first = r["out1"][:m * rec].view(m, rec)[:, :2].to(torch.int64)
            r["rows2"] = (first[:, 0] * 251 + first[:, 1] * 7 + torch.arange(m, device="cuda")) % r["n_rows"]
            codec.gather_async(r["idx"], None, r["rows2"] * rec, r["lengths"], m, 1, r["cap"], r["out2"][:m * rec], r["offs2"], r["st2"], r["need"][1:2])
            w[2:3].copy_(codec._status)
    side.synchronize()
    for r in runs:
        m, recs = r["m"], r["data"].reshape(r["n_rows"], rec)
        assert r["words"].cpu().tolist()[:3] == [0, 0, 0]
        assert r["st1"].cpu().tolist() == [0] * m and r["st2"].cpu().tolist() == [0] * m
        assert r["offs1"].cpu().tolist() == [k * rec for k in range(m + 1)] == r["offs2"].cpu().tolist()
        rows = r["rows"].cpu().numpy()
        out1 = r["out1"].cpu().numpy()
        assert np.array_equal(out1[:m * rec].reshape(m, rec), recs[rows]) and np.array_equal(out1[m * rec:], sentinel(out1.size)[m * rec:])
        rows2 = (recs[rows][:, 0].astype(np.int64) * 251 + recs[rows][:, 1].astype(np.int64) * 7 + np.arange(m)) % r["n_rows"]
        assert np.array_equal(r["rows2"].cpu().numpy(), rows2)
        out2 = r["out2"].cpu().numpy()
        assert np.array_equal(out2[:m * rec].reshape(m, rec), recs[rows2]) and np.array_equal(out2[m * rec:], sentinel(out2.size)[m * rec:])
        want = [sum(1 + ((int(x) * rec + rec - 1) // bl > int(x) * rec // bl) for x in rr) for rr in (rows, rows2)]
        assert r["need"].cpu().tolist() == want
        r["idx"].close()


def test_the_python_wrappers_defaults(codec, tsq):
    import torch
    data = tsq.synth.text(40 * 4096 + 33, seed=91)
    blob, table = codec.compress_split(to_dev(data), 1, 4096, block_sizes=True)
    offsets, lengths = [5, 4090, 100000, data.size - 7, data.size, 0], [100, 5000, 0, 7, 1, data.size + 1]
    d_off, d_len = u64_dev(offsets), u64_dev(lengths)
    want_st = [0, 0, 0, 0, ERR_ARG, ERR_ARG]
    for idx in (codec.index(blob), codec.index_sized(blob, data.size, 4096, table)):
        out, d_offs, st = idx.gather(d_off, d_len, align=16, range_status=True)
        torch.cuda.synchronize()
        assert st.cpu().tolist() == want_st and codec.status() == ERR_ARG
        offs = d_offs.cpu().tolist()
        assert offs == [0, 112, 5120, 5120, 5136, 5136, 5136] and out.numel() == offs[-1]
        host = out.cpu().numpy()
        for o, a, ln, s in zip(offs, offsets, lengths, want_st):
            if s == 0:
                assert np.array_equal(host[o:o + ln], data[a:a + ln])
        # with the room given nothing is measured
        out2, d_offs2 = idx.gather(d_off[:4], d_len[:4], out=torch.zeros(6000, dtype=torch.uint8, device="cuda"), cap_pieces=16)
        torch.cuda.synchronize()
        assert codec.status() == 0 and d_offs2.cpu().tolist() == [0, 100, 5100, 5100, 5107]
        assert np.array_equal(out2.cpu().numpy()[5100:5107], data[-7:])
        # no ranges: empty results, not a refusal
        none, d_none = idx.gather(d_off[:0], d_len[:0])
        torch.cuda.synchronize()
        assert none.numel() == 0 and d_none.cpu().tolist() == [0] and codec.status() == 0
        # tables of another type are refused before anything is read through them
        for bad in ((d_off.to(torch.int32), d_len), (d_off, d_len[:3]), (d_off.cpu(), d_len)):
            with pytest.raises(tsq.TsqError) as err:
                idx.gather(*bad)
            assert err.value.code == ERR_ARG
        idx.close()
    parts = [tsq.synth.text(n, seed=92 + n) for n in (10, 5000, 300)]
    blobs = [codec.compress(to_dev(p), 1) for p in parts]
    bidx = codec.index_batch(blobs)
    out, d_offs, st = bidx.gather(u32_dev([2, 0, 1, 3]), u64_dev([100, 0, 4000, 0]), u64_dev([200, 10, 1000, 1]), range_status=True)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, 0, 0, ERR_ARG] and d_offs.cpu().tolist() == [0, 200, 210, 1210, 1210]
    assert bytes(out.cpu().numpy()) == parts[2][100:300].tobytes() + parts[0].tobytes() + parts[1][4000:5000].tobytes()
    flat, d_offs = bidx.gather(None, u64_dev([5, 10 + 4999]), u64_dev([10, 3]))
    torch.cuda.synchronize()
    cat = np.concatenate(parts)
    assert bytes(flat.cpu().numpy()) == cat[5:15].tobytes() + cat[5009:5012].tobytes()
    bidx.close()
