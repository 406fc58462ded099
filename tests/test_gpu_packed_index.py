"""GPU tests of the index of a packed batch made from its device tables (tsqa_index_create_packed*, tsqa_index_fetch,
tsqa_index_device_tables, DeviceCodec.index_packed_async, PackedBatch.index(sync=False)): the cases are packedindexgen's, what each
owes is restated there in pure Python, and test_packed_index_cpu.py shows that each case reaches what it aims at.  Every creation
runs on a side stream; the arena and every table lie between fences, and so do the words the call writes.  Each case is also
indexed by tsqa_index_create_batch, and the two indexes must answer alike: the gather through the unfetched index, and after
tsqa_index_fetch the host's accessors and the host-planned reads."""
import ctypes as C

import numpy as np
import pytest

import packedindexgen as pg
from test_gpu_cut import FENCE, TABLE_FENCE, TABLE_GUARD, Table, sentinel, to_dev, u64_dev

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = pg.OK, pg.ERR_ARG, pg.ERR_FORMAT, pg.ERR_OVERFLOW


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


class Fenced:
    """words the call may only read, with guard words on both sides: nothing of the buffer may change"""

    def __init__(self, values, dtype):
        guard = [TABLE_GUARD] * TABLE_FENCE
        host = np.array(guard + [int(v) for v in values] + guard, dtype=np.uint64 if dtype == np.int64 else np.uint32).view(dtype)
        self.host, self.buf, self.n = host, to_dev(host), len(values)

    @property
    def t(self):
        return self.buf[TABLE_FENCE:TABLE_FENCE + self.n]

    def untouched(self):
        return np.array_equal(self.buf.cpu().numpy(), self.host)


class Device:
    """a case on the device: the arena between fences of FENCE bytes, its tables fenced"""

    def __init__(self, case):
        self.case = case
        self.host = sentinel(case.arena.size + 2 * FENCE)
        self.host[FENCE:FENCE + case.arena.size] = case.arena
        self.buf = to_dev(self.host)
        self.arena = self.buf[FENCE:FENCE + case.arena.size]
        self.offsets, self.sizes = Fenced(case.offsets, np.int64), Fenced(case.sizes, np.int64)
        self.first = Fenced(case.table_first, np.int64) if case.sized else None
        self.table = Fenced(case.table, np.int32) if case.sized else None

    def untouched(self):
        return (np.array_equal(self.buf.cpu().numpy(), self.host) and self.offsets.untouched() and self.sizes.untouched() and
                (self.first is None or (self.first.untouched() and self.table.untouched())))


class Made:
    """tsqa_index_create_packed_async through the C ABI on the current stream, its outputs fenced"""

    def __init__(self, codec, d: Device, cap_blocks, plain=False):
        import torch
        case = d.case
        self.codec, self.blob, self.h, self.n, self.cap = codec, d.arena, C.c_void_p(), case.n, cap_blocks
        self.item_status, self.word = Table(case.n, torch.int32), Table(1, torch.int32)
        sized = case.sized and not plain
        rc = codec.L.tsqa_index_create_packed_async(codec.h, d.arena.data_ptr(), d.arena.numel(), d.offsets.t.data_ptr(), d.sizes.t.data_ptr(),
                                                    case.n, cap_blocks, case.block_len if sized else 0, d.first.t.data_ptr() if sized else None,
                                                    d.table.t.data_ptr() if sized else None, case.table_words if sized else 0, C.byref(self.h),
                                                    self.item_status.ptr(), self.word.ptr(), codec._stream())
        assert rc == OK and self.h, codec.last_error()

    def device_tables(self, tsq):
        """-> (item_first, item_status, words) read from the index's own device tables"""
        import torch
        from turbosqueeze_amd.api import _DeviceWords
        first, status, words = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert self.codec.L.tsqa_index_device_tables(self.h, C.byref(first), C.byref(status), C.byref(words)) == OK
        view = lambda p, n, kind: torch.as_tensor(_DeviceWords(p.value, n, kind), device=self.codec.device).cpu().tolist()
        return view(first, self.n + 1, "<i8"), view(status, self.n, "<i4"), view(words, 3, "<i8")

    def close(self):
        if self.h:
            self.codec.L.tsqa_index_destroy(self.h)
            self.h = C.c_void_p()


class HostMade:
    """tsqa_index_create_batch over the same containers.  That call refuses the whole batch for a place outside the buffer or
    shorter than a header, and knows no cap_blocks: such items, and the unfit ones, are offered as 16 bytes that are no container,
    which it refuses for themselves.  So are the items that only a size table refuses: the plain walk may take them."""

    def __init__(self, codec, d: Device, e):
        import torch
        from turbosqueeze_amd.api import _batch_array
        case, size = d.case, d.case.arena.size
        spans = []
        for i, (a, n) in enumerate(zip(case.offsets, case.sizes)):
            placed = n <= size and a <= size - n and n >= pg.HEADER
            st = e["item_status"][i]
            spans.append((a, n) if st == OK or (placed and st == ERR_FORMAT and not case.sized) else (1, 16))
        self.codec, self.blob, self.h = codec, d.arena, C.c_void_p()
        status = (C.c_int32 * case.n)()
        torch.cuda.synchronize()
        rc = codec.L.tsqa_index_create_batch(codec.h, d.arena.data_ptr(), d.arena.numel(), _batch_array([(a, n, 0, 0) for a, n in spans]), case.n,
                                             C.byref(self.h), status)
        assert self.h and rc in (OK, ERR_FORMAT), codec.last_error()
        self.status = list(status)

    close = Made.close


def gather(codec, index, ranges, by_item, e):
    """tsqa_gather_async of (item, offset, length) ranges on the current stream, by item or flat -> what it left, on the host"""
    import torch
    n = len(ranges)
    items = to_dev(np.array([r[0] for r in ranges], dtype=np.uint32).view(np.int32)) if by_item else None
    offsets = u64_dev([r[1] if by_item else e["item_at"][r[0]] + r[1] for r in ranges])
    lengths = u64_dev([r[2] for r in ranges])
    room = sum(r[2] for r in ranges)
    out = to_dev(sentinel(room + 2 * FENCE))
    out_offsets, status, need, word = Table(n + 1, torch.int64), Table(n, torch.int32), Table(1, torch.int64), Table(1, torch.int32)
    rc = codec.L.tsqa_gather_async(codec.h, index.h, items.data_ptr() if by_item else None, offsets.data_ptr(), lengths.data_ptr(), n, 1,
                                   4 * n + 16, out.data_ptr() + FENCE, room, out_offsets.ptr(), status.ptr(), need.ptr(), word.ptr(),
                                   codec._stream())
    assert rc == OK, codec.last_error()
    torch.cuda.synchronize()
    return dict(out=out.cpu().numpy(), out_offsets=out_offsets.values(), status=status.values(), need=need.values(), word=word.values())


def owed_bytes(case, ranges, got):
    """every accepted range's bytes are its item's data, and nothing else of the output is written"""
    want = sentinel(got["out"].size)
    for k, (i, o, n) in enumerate(ranges):
        if got["status"][k] == OK:
            at = FENCE + got["out_offsets"][k]
            want[at:at + n] = np.frombuffer(case.datas[i], dtype=np.uint8)[o:o + n]
    assert np.array_equal(got["out"], want), case.name


def check_case(tsq, codec, side, case, cap_blocks=None):
    import torch
    from turbosqueeze_amd.api import _item_range_array, _range_array
    e = case.expect(cap_blocks=cap_blocks)
    cap = e["cap_blocks"]
    d = Device(case)
    with torch.cuda.stream(side):
        made = Made(codec, d, cap)
    side.synchronize()
    host = None
    try:
        # the device's tables against the restatement
        first, status, words = made.device_tables(tsq)
        print(case.name, "cap", cap, "words", words, "status", made.word.values())
        assert made.item_status.values() == e["item_status"] == status, case.name
        assert made.word.values() == [e["status"]]
        assert first == e["item_first"] and words == e["words"], case.name
        assert d.untouched(), "the call wrote to its inputs or their fences"
        # before a fetch the host knows nothing, and says so
        L = codec.L
        assert (L.tsqa_index_items(made.h), L.tsqa_index_blocks(made.h), L.tsqa_index_total(made.h)) == (case.n, 0, 0)
        assert L.tsqa_index_item_total(made.h, 0) == 0 and L.tsqa_index_item_status(made.h, 0) == ERR_ARG
        one = torch.empty(16, dtype=torch.uint8, device="cuda")
        for rc in (L.tsqa_decompress_ranges(codec.h, made.h, _range_array([(0, 1, 0)]), 1, one.data_ptr(), 16, None),
                   L.tsqa_decompress_item_ranges(codec.h, made.h, _item_range_array([(0, 0, 1, 0)]), 1, one.data_ptr(), 16, None)):
            assert rc == ERR_ARG and "tsqa_index_fetch" in codec.last_error()
        # the gather through the unfetched index and through the host-made one, range for range
        host = HostMade(codec, d, e)
        assert [st != OK for st in host.status] == [st != OK for st in e["item_status"]], case.name
        ranges = pg.ranges(case, e)
        healthy = [r for r in ranges if e["item_status"][r[0]] == OK]
        for by_item, rr in ((True, ranges), (False, healthy)):
            if not rr:
                continue
            mine, theirs = gather(codec, made, rr, by_item, e), gather(codec, host, rr, by_item, e)
            for key in ("out_offsets", "status", "need", "word"):
                assert mine[key] == theirs[key], (case.name, by_item, key)
            assert np.array_equal(mine["out"], theirs["out"]), (case.name, by_item)
            assert mine["status"] == [OK if e["item_status"][i] == OK else ERR_ARG for i, _, _ in rr], (case.name, by_item)
            owed_bytes(case, rr, mine)
        # after the fetch: a tsqa_index_create_batch index in every respect
        assert L.tsqa_index_fetch(codec.h, made.h, None) == OK, codec.last_error()
        assert L.tsqa_index_fetch(codec.h, made.h, None) == OK
        assert (L.tsqa_index_items(made.h), L.tsqa_index_blocks(made.h), L.tsqa_index_total(made.h)) == \
               (L.tsqa_index_items(host.h), L.tsqa_index_blocks(host.h), L.tsqa_index_total(host.h)) == (case.n, e["words"][0], e["words"][1])
        for i in sorted({0, case.n - 1} | {r[0] for r in ranges}):
            assert L.tsqa_index_item_total(made.h, i) == L.tsqa_index_item_total(host.h, i) == (e["totals"][i] if e["item_status"][i] == OK else 0)
            assert L.tsqa_index_item_status(made.h, i) == e["item_status"][i]
            assert (L.tsqa_index_item_status(host.h, i) != OK) == (e["item_status"][i] != OK)
        if healthy:
            at, quads, flat = 0, [], []
            for i, o, n in healthy:
                quads.append((i, o, n, at))
                flat.append((e["item_at"][i] + o, n, at))
                at += n
            outs = []
            for index in (made, host):
                a, b = torch.zeros(at, dtype=torch.uint8, device="cuda"), torch.zeros(at, dtype=torch.uint8, device="cuda")
                assert L.tsqa_decompress_item_ranges(codec.h, index.h, _item_range_array(quads), len(quads), a.data_ptr(), at, None) == OK, codec.last_error()
                assert L.tsqa_decompress_ranges(codec.h, index.h, _range_array(flat), len(flat), b.data_ptr(), at, None) == OK, codec.last_error()
                outs.append((a.cpu().numpy(), b.cpu().numpy()))
            want = np.concatenate([np.frombuffer(case.datas[i], dtype=np.uint8)[o:o + n] for i, o, n in healthy])
            for a, b in outs:
                assert np.array_equal(a, want) and np.array_equal(b, want), case.name
            # and the gather takes the fetched index as before
            again = gather(codec, made, healthy, True, e)
            assert again["status"] == [OK] * len(healthy)
            owed_bytes(case, healthy, again)
        assert d.untouched()
        return made.device_tables(tsq)
    finally:
        made.close()
        if host is not None:
            host.close()


@pytest.mark.parametrize("case", pg.plain_cases(), ids=lambda c: c.name)
def test_plain_form(tsq, codec, side, case):
    check_case(tsq, codec, side, case)


@pytest.mark.parametrize("case", pg.sized_cases(), ids=lambda c: c.name)
def test_sized_form(tsq, codec, side, case):
    check_case(tsq, codec, side, case)


def test_sized_and_plain_agree_on_true_tables(tsq, codec, side):
    import torch
    for case in list(pg.sized_true()) + list(pg.carry_places()[0]):
        e = case.expect()
        d = Device(case)
        with torch.cuda.stream(side):
            a, b = Made(codec, d, e["cap_blocks"]), Made(codec, d, e["cap_blocks"], plain=True)
        side.synchronize()
        try:
            assert a.device_tables(tsq) == b.device_tables(tsq) == (e["item_first"], e["item_status"], e["words"]), case.name
            ranges = pg.ranges(case, e)
            x, y = gather(codec, a, ranges, True, e), gather(codec, b, ranges, True, e)
            assert all(np.array_equal(x[k], y[k]) if k == "out" else x[k] == y[k] for k in x), case.name
        finally:
            a.close()
            b.close()


def test_rooms_one_short_and_loose(tsq, codec, side):
    """every case of cap_cuts runs in test_plain_form at its own room; here the three-block batch at every room from 1 to two more
    than it needs, and a sized batch one block short"""
    case = pg.three_blocks()
    for cap in range(1, case.expect()["words"][2] + 3):
        check_case(tsq, codec, side, case, cap_blocks=cap)
    sized = pg.sized_true()[5]
    check_case(tsq, codec, side, sized, cap_blocks=sized.expect()["words"][2] - 1)


def test_arguments_are_refused_before_anything_is_enqueued(tsq, codec, side):
    import torch
    case = pg.sized_true()[5]
    d = Device(case)
    L = codec.L
    word, status = Table(1, torch.int32), Table(case.n, torch.int32)
    base = dict(arena=d.arena.data_ptr(), size=d.arena.numel(), offsets=d.offsets.t.data_ptr(), sizes=d.sizes.t.data_ptr(), n=case.n, cap=12,
                block_len=4096, first=d.first.t.data_ptr(), table=d.table.t.data_ptr(), words=case.table_words, word=word.ptr())

    def call(**over):
        a = dict(base, **over)
        h = C.c_void_p(1)
        rc = L.tsqa_index_create_packed_async(codec.h, a["arena"], a["size"], a["offsets"], a["sizes"], a["n"], a["cap"], a["block_len"], a["first"],
                                              a["table"], a["words"], C.byref(h), status.ptr(), a["word"], None)
        if rc == OK:
            L.tsqa_index_destroy(h)
        else:
            assert not h.value
        return rc

    plain = dict(block_len=0, first=None, table=None, words=0)
    for over in (dict(arena=None), dict(offsets=None), dict(sizes=None), dict(word=None), dict(n=0), dict(cap=0), dict(first=None),
                 dict(block_len=0), dict(block_len=2048), dict(block_len=4097), dict(block_len=1 << 23),
                 dict(plain, block_len=4096), dict(plain, first=base["first"]), dict(plain, words=1)):
        assert call(**over) == ERR_ARG, over
    torch.cuda.synchronize()
    assert word.untouched() and status.untouched()
    assert L.tsqa_index_create_packed_async(codec.h, base["arena"], base["size"], base["offsets"], base["sizes"], case.n, 12, 0, None, None, 0, None,
                                            None, word.ptr(), None) == ERR_ARG
    assert call() == OK and call(**plain) == OK
    # the cut refuses it, as it refuses a batch index
    with torch.cuda.stream(side):
        made = Made(codec, d, 12)
        first, count = u64_dev([0]), u64_dev([1])
        tables = [Table(2, torch.int64), Table(1, torch.int64), Table(1, torch.int32), Table(1, torch.int32)]
        assert L.tsqa_cut_async(codec.h, made.h, first.data_ptr(), count.data_ptr(), 1, 16, None, 0, tables[0].ptr(), tables[1].ptr(), None,
                                tables[2].ptr(), tables[3].ptr(), codec._stream()) == ERR_ARG and "batch index" in codec.last_error()
    side.synchronize()
    made.close()
    # and a fetched index of ONE item too, which tsqa_index_items alone would let through
    single = Device(pg.item_counts()[0])
    h1 = C.c_void_p()
    assert L.tsqa_index_create_packed(codec.h, single.arena.data_ptr(), single.arena.numel(), single.offsets.t.data_ptr(), single.sizes.t.data_ptr(),
                                      1, 1, 0, None, None, 0, C.byref(h1), None, None) == OK and L.tsqa_index_items(h1) == 1
    assert L.tsqa_index_blocks(h1) == 1 and L.tsqa_index_item_status(h1, 0) == OK
    assert L.tsqa_cut_async(codec.h, h1, first.data_ptr(), count.data_ptr(), 1, 16, None, 0, tables[0].ptr(), tables[1].ptr(), None,
                            tables[2].ptr(), tables[3].ptr(), None) == ERR_ARG and "batch index" in codec.last_error()
    torch.cuda.synchronize()
    L.tsqa_index_destroy(h1)
    assert all(t.untouched() for t in tables)
    # the other indexes have no device tables, and a fetch of them has nothing to do
    plain_index = tsq.RangeIndex(codec, to_dev(np.frombuffer(case.blobs[0], dtype=np.uint8).copy()))
    p = C.c_void_p(1)
    assert L.tsqa_index_device_tables(plain_index.h, C.byref(p), None, None) == ERR_ARG and not p.value
    assert L.tsqa_index_fetch(codec.h, plain_index.h, None) == OK and L.tsqa_index_fetch(codec.h, None, None) == ERR_ARG
    # the waiting form: the index is made whatever the items are, the statuses come to the host
    bad, verdicts = pg.sized_bad_first()[0]
    db = Device(bad)
    h, st = C.c_void_p(), (C.c_int32 * bad.n)()
    rc = L.tsqa_index_create_packed(codec.h, db.arena.data_ptr(), db.arena.numel(), db.offsets.t.data_ptr(), db.sizes.t.data_ptr(), bad.n, 64, 4096,
                                    db.first.t.data_ptr(), db.table.t.data_ptr(), bad.table_words, C.byref(h), st, None)
    try:
        e = bad.expect(cap_blocks=64)
        assert rc == e["status"] == ERR_FORMAT and h and list(st) == e["item_status"]
        assert L.tsqa_index_blocks(h) == e["words"][0] and L.tsqa_index_total(h) == e["words"][1]
    finally:
        L.tsqa_index_destroy(h)


def rows(torch, data, in_offsets, items, lengths):
    """the first lengths[k] bytes of item items[k], on the host"""
    return [data[in_offsets[i]:in_offsets[i] + n] for i, n in zip(items, lengths)]


def test_chain_tables_compress_sized_index_gather(tsq, codec, side):
    """compress_batch_packed_tables_split_async -> index_packed_async (sized, from the tables it left) -> row numbers drawn on the
    device -> gather, on one stream with no synchronise in between; twice back to back, the second with more items and blocks"""
    import torch
    fresh = tsq.DeviceCodec(0)
    try:
        runs = []
        with torch.cuda.stream(side):
            for n_items, seed in ((24, 1), (300, 2)):
                rng = np.random.default_rng(pg.SEED + seed)
                sizes = [int(x) for x in rng.integers(100, 3 * 4096 + 50, n_items)]
                data = tsq.synth.text(sum(sizes), seed=seed)
                in_offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
                first, _, bound, _ = tsq.plan_compress_tables_split(in_offsets, sizes, data.size, 4096, 16, 1 << 20)
                cap, n_rows = first[-1], 2000
                d_data, d_at, d_sz = to_dev(data), u64_dev(in_offsets), u64_dev(sizes)
                arena = torch.empty(bound, dtype=torch.uint8, device="cuda")
                i64 = lambda k: torch.empty(k, dtype=torch.int64, device="cuda")
                d_offsets, d_sizes, d_first, d_status = i64(n_items + 1), i64(n_items), i64(n_items + 1), torch.empty(n_items, dtype=torch.int32, device="cuda")
                table = torch.empty(cap, dtype=torch.int32, device="cuda")
                out, status = torch.empty(100 * n_rows, dtype=torch.uint8, device="cuda"), []
                fresh.compress_batch_packed_tables_split_async(d_data, d_at, d_sz, n_items, cap, 1, 16, 4096, arena, d_offsets, d_sizes, d_first, None,
                                                               table, d_status)
                status.append(fresh._status.clone())
                index = fresh.index_packed_async(arena, d_offsets, d_sizes, n_items, cap, 4096, d_first, table)
                status.append(fresh._status.clone())
                d_items = torch.randint(0, n_items, (n_rows,), device="cuda", dtype=torch.int32)
                d_off, d_len = torch.zeros(n_rows, dtype=torch.int64, device="cuda"), torch.full((n_rows,), 100, dtype=torch.int64, device="cuda")
                got = index.gather(d_items, d_off, d_len, out=out, cap_pieces=2 * n_rows, range_status=True)
                status.append(fresh._status.clone())
                runs.append((data, in_offsets, index, d_items, got, status, cap))
        side.synchronize()
        for data, in_offsets, index, d_items, (out, d_out_offsets, d_range_status), status, cap in runs:
            assert [int(s.item()) for s in status] == [OK, OK, OK]
            assert d_range_status.cpu().tolist() == [OK] * 2000 and d_out_offsets.cpu().tolist() == list(range(0, 200001, 100))
            want = np.concatenate(rows(torch, data, in_offsets, d_items.cpu().tolist(), [100] * 2000))
            assert np.array_equal(out.cpu().numpy(), want)
            assert index.d_item_status.cpu().tolist() == [OK] * index.items and index.d_blocks_total.cpu().tolist() == [cap, data.size, cap]
            index.close()
    finally:
        fresh.close()


def test_chain_packed_compress_plain_index_gather(tsq, codec, side):
    """compress_batch_packed_async -> index_packed_async (plain) -> gather, on one stream with no synchronise in between; twice
    back to back, the second with more items"""
    import torch
    fresh = tsq.DeviceCodec(0)
    try:
        runs = []
        with torch.cuda.stream(side):
            for n_items, seed in ((16, 3), (280, 4)):
                rng = np.random.default_rng(pg.SEED + seed)
                sizes = [int(x) for x in rng.integers(200, 9000, n_items)]
                data = tsq.synth.text(sum(sizes), seed=seed)
                in_offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
                d_data = to_dev(data)
                arena = torch.empty(sum(tsq.batch_bound(z) + 16 for z in sizes), dtype=torch.uint8, device="cuda")
                d_offsets, d_sizes = torch.empty(n_items + 1, dtype=torch.int64, device="cuda"), torch.empty(n_items, dtype=torch.int64, device="cuda")
                fresh.compress_batch_packed_async(d_data, list(zip(in_offsets, sizes)), 1, 16, arena, d_offsets, d_sizes)
                index = fresh.index_packed_async(arena, d_offsets, d_sizes, n_items, n_items)
                d_items = torch.arange(n_items - 1, -1, -1, device="cuda", dtype=torch.int32)
                d_off = torch.full((n_items,), 50, dtype=torch.int64, device="cuda")
                d_len = torch.full((n_items,), 150, dtype=torch.int64, device="cuda")
                out = torch.empty(150 * n_items, dtype=torch.uint8, device="cuda")
                got = index.gather(d_items, d_off, d_len, out=out, cap_pieces=n_items, range_status=True)
                runs.append((data, in_offsets, n_items, index, got, fresh._status.clone()))
        side.synchronize()
        for data, in_offsets, n_items, index, (out, d_out_offsets, d_range_status), status in runs:
            assert int(status.item()) == OK and d_range_status.cpu().tolist() == [OK] * n_items
            want = np.concatenate([data[in_offsets[i] + 50:in_offsets[i] + 200] for i in range(n_items - 1, -1, -1)])
            assert np.array_equal(out.cpu().numpy(), want)
            assert index.d_item_first.cpu().tolist() == list(range(n_items + 1))
            index.close()
    finally:
        fresh.close()


def test_python_from_device_indexes_with_no_host_read(tsq, codec, side, monkeypatch):
    """PackedBatch.from_device(...).index(sync=False) and a gather with its room given read nothing on the host; fetch() then makes
    it a BatchIndex; PackedBatch.index(sync=False) of a batch of short blocks takes the sized form; index() stays what it was"""
    import torch
    srcs = [to_dev(tsq.synth.text(n, seed=n)) for n in (5000, 100, 3 * 4096 + 1, 70000)]
    batch = codec.compress_batch_packed(srcs, 1, block_len=4096)
    d_offsets, d_sizes = u64_dev(batch.offsets), u64_dev(batch.sizes)
    d_items = to_dev(np.array([3, 0, 2, 1], dtype=np.int32))
    d_off, d_len = u64_dev([60000, 10, 4090, 0]), u64_dev([5000, 4000, 10, 100])
    out = torch.empty(9110, dtype=torch.uint8, device="cuda")

    def boom(*a, **k):
        raise AssertionError("a host read on the way")

    with torch.cuda.stream(side):
        with monkeypatch.context() as m:
            for name in ("cpu", "item", "tolist", "numpy"):
                m.setattr(torch.Tensor, name, boom)
            received = tsq.PackedBatch.from_device(codec, batch.arena, d_offsets, d_sizes)
            index = received.index(sync=False, cap_blocks=batch.first_block[-1])
            with pytest.raises(tsq.TsqError) as no_count:   # nothing on the host says how many blocks there are
                received.index(sync=False)
            loose = received.index(sync=False, cap_blocks=batch.first_block[-1] + 1000)
            sized = batch.index(sync=False)
            got = [ix.gather(d_items, d_off, d_len, out=torch.empty_like(out), cap_pieces=64) for ix in (index, loose, sized)]
    side.synchronize()
    want = np.concatenate([srcs[i].cpu().numpy()[o:o + n] for i, o, n in ((3, 60000, 5000), (0, 10, 4000), (2, 4090, 10), (1, 0, 100))])
    for o, d_out_offsets in got:
        assert np.array_equal(o.cpu().numpy(), want) and d_out_offsets.cpu().tolist() == [0, 5000, 9000, 9010, 9110]
    assert isinstance(index, tsq.DeviceBatchIndex) and (index.n_blocks, index.total, index.items, index.fetched) == (0, 0, 4, False)
    assert sized.d_blocks_total.cpu().tolist() == [batch.first_block[-1], sum(batch.lengths), batch.first_block[-1]]
    assert loose.cap_blocks > index.cap_blocks == batch.first_block[-1]
    assert no_count.value.code == ERR_ARG and "cap_blocks" in str(no_count.value)
    with pytest.raises(tsq.TsqError) as err:
        index.read(0, 0, 10)
    assert err.value.code == ERR_ARG and "tsqa_index_fetch" in str(err.value)
    host = batch.index()
    assert type(host) is tsq.BatchIndex
    with torch.cuda.stream(side):
        assert index.fetch() is index
    assert (index.n_blocks, index.total, index.worst_status) == (host.n_blocks, host.total, OK)
    assert [index.item_total(i) for i in range(4)] == [host.item_total(i) for i in range(4)] == batch.lengths
    reads = [(3, 60000, 5000), (2, 4090, 10)]
    assert torch.equal(index.read_many(reads)[0], host.read_many(reads)[0])
    assert torch.equal(index.read_flat_many([(5090, 20)])[0], host.read_flat_many([(5090, 20)])[0])
    assert received.lengths == batch.lengths and received.offsets == batch.offsets
    # once measured, the batch knows its own count: the headers', whatever block length the containers were cut at
    counted = received.index(sync=False)
    assert counted.cap_blocks == received.n_blocks == batch.first_block[-1] and counted.fetch().worst_status == OK and counted.total == host.total
    for ix in (index, loose, sized, host, counted):
        ix.close()
