"""GPU tests of the take (tsqa_cut_items_async, tsqa_cut_items, DeviceCodec.cut_items_async, BatchIndex.cut_items,
PackedBatch.take): the cases are takegen's, the expected arena, tables and statuses are made there in pure Python from the arena's
bytes, and test_take_cpu.py shows that each case reaches what it aims at.  Every buffer and table the library may write is filled
with a sentinel first, with a fence on both sides, and must keep it wherever the call owes nothing: padding, the room of ranges
that do not fit, and everything behind a refusal."""
import ctypes as C

import numpy as np
import pytest

import cutgen as cg
import takegen as tk

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = tk.OK, tk.ERR_ARG, tk.ERR_FORMAT, tk.ERR_OVERFLOW
FENCE = 4096
TABLE_GUARD, TABLE_FENCE = 0x5EA1ED, 8


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


def to_dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (the pattern repeats every 251 bytes): test_gpu_cut.py's"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


def u64_dev(values):
    """any 64-bit values as an int64 CUDA tensor"""
    return to_dev(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64))


def u32_dev(values):
    """any 32-bit values as an int32 CUDA tensor"""
    return to_dev(np.array([int(v) for v in values], dtype=np.uint32).view(np.int32))


class Table:
    """n words the call may write, filled with the guard, with guard words on both sides"""

    def __init__(self, n, dtype):
        import torch
        self.n = n
        self.buf = torch.full((n + 2 * TABLE_FENCE,), TABLE_GUARD, dtype=dtype, device="cuda")

    def ptr(self):
        return self.buf.data_ptr() + TABLE_FENCE * self.buf.element_size()

    @property
    def t(self):
        return self.buf[TABLE_FENCE:TABLE_FENCE + self.n]

    def values(self):
        host = self.buf.cpu().numpy()
        assert (host[:TABLE_FENCE] == TABLE_GUARD).all() and (host[TABLE_FENCE + self.n:] == TABLE_GUARD).all(), "a table's fence"
        return host[TABLE_FENCE:TABLE_FENCE + self.n].tolist()

    def untouched(self):
        return self.values() == [TABLE_GUARD] * self.n


class Room:
    """the call's outputs: fenced tables, and a fenced output of out_size bytes that starts `skew` bytes past a multiple of 16
    (out_size None: measure only)"""

    def __init__(self, n, out_size, skew=0):
        import torch
        self.offsets, self.sizes, self.totals = Table(n + 1, torch.int64), Table(n, torch.int64), Table(n, torch.int64)
        self.item_status, self.word = Table(n, torch.int32), Table(1, torch.int32)
        self.out_size, self.at = out_size, FENCE + skew
        self.buf = to_dev(sentinel(2 * FENCE + 16 + out_size)) if out_size is not None else None
        if self.buf is not None:
            assert self.buf.data_ptr() % 16 == 0

    def out_ptr(self):
        return self.buf.data_ptr() + self.at if self.buf is not None else None

    def arena(self):
        return self.buf[self.at:self.at + self.out_size]

    def tables(self):
        return (self.offsets, self.sizes, self.totals, self.item_status, self.word)


_INDEXES = {}


def index_of(tsq, codec, batch, kind="device", cap_blocks=None):
    """-> the index of a takegen batch, made once per kind: 'batch' (tsqa_index_create_batch), 'device' (tsqa_index_create_packed_async,
    plain form, NOT fetched), 'fetched' (the same after tsqa_index_fetch), 'sized' (its sized form, not fetched), 'plain'
    (tsqa_index_create of the one container), 'sized_one' (tsqa_index_create_sized_async of the one container)"""
    import torch
    key = (batch.name, kind, cap_blocks)
    if key in _INDEXES:
        return _INDEXES[key]
    arena = to_dev(batch.arena)
    torch.cuda.synchronize()
    if kind == "batch":
        idx = tsq.BatchIndex(codec, arena, list(zip(batch.offsets, batch.sizes)))
    elif kind == "plain":
        idx = tsq.RangeIndex(codec, arena)
    elif kind == "sized_one":
        idx = tsq.SizedIndex(codec, arena, len(batch.datas[0]), batch.block_len, to_dev(batch.table, np.int32), sync=False)
    else:
        cap = cap_blocks if cap_blocks is not None else max(batch.index().need_blocks, 1)
        sized = (batch.block_len, u64_dev(batch.table_first), to_dev(np.array(batch.table, dtype=np.uint32).view(np.int32))) if kind == "sized" else ()
        idx = tsq.DeviceBatchIndex(codec, arena, u64_dev(batch.offsets), u64_dev(batch.sizes), batch.n, cap, *sized)
        if kind == "fetched":
            idx.fetch()
    torch.cuda.synchronize()
    _INDEXES[key] = idx
    return idx


@pytest.fixture(scope="module", autouse=True)
def close_indexes():
    yield
    import torch
    torch.cuda.synchronize()
    for idx in _INDEXES.values():
        idx.close()
    _INDEXES.clear()


class Tables:
    """a case's tables in device memory"""

    def __init__(self, case):
        self.items = u32_dev(case.items)
        self.first = u64_dev(f for f, _ in case.ranges) if case.ranges is not None else None
        self.count = u64_dev(c for _, c in case.ranges) if case.ranges is not None else None


def take_call(codec, index, t, n_ranges, align_to, room, **over):
    """tsqa_cut_items_async on the current stream -> its return value.  over: arguments replaced."""
    ptr = lambda x: x.data_ptr() if x is not None else None
    a = dict(ctx=codec.h, idx=index.h, items=ptr(t.items), first=ptr(t.first), count=ptr(t.count), n=n_ranges, align=align_to, out=room.out_ptr(),
             out_size=room.out_size or 0, offsets=room.offsets.ptr(), sizes=room.sizes.ptr(), totals=room.totals.ptr(),
             item_status=room.item_status.ptr(), status=room.word.ptr())
    a.update(over)
    return codec.L.tsqa_cut_items_async(a["ctx"], a["idx"], a["items"], a["first"], a["count"], a["n"], a["align"], a["out"], a["out_size"],
                                        a["offsets"], a["sizes"], a["totals"], a["item_status"], a["status"], codec._stream())


def first_difference(got, want):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return [(int(k), int(got[k]), int(want[k])) for k in bad[:8]]


def check(case, room, e, what):
    """the tables, the statuses and every byte of the fenced output against takegen's `e`"""
    got_status = room.item_status.values()
    assert got_status == e["item_status"], f"{what}: item statuses {first_difference(got_status, e['item_status'])} (range, got, owed)"
    assert room.word.values() == [e["status"]], f"{what}: *d_status is {room.word.values()}, owed {e['status']}"
    for name, table in (("offsets", room.offsets), ("sizes", room.sizes), ("totals", room.totals)):
        got = table.values()
        assert got == e[name], f"{what}: d_{name} {first_difference(got, e[name])} (range, got, owed)"
    if room.buf is not None:
        want = sentinel(room.buf.numel())
        want[room.at:room.at + room.out_size] = case.arena(e, want[room.at:room.at + room.out_size])
        host = room.buf.cpu().numpy()
        if not np.array_equal(host, want):
            at = int(np.flatnonzero(host != want)[0]) - room.at
            k = int(np.searchsorted(np.array(e["offsets"]), at, side="right")) - 1
            raise AssertionError(f"{what}: byte {at} of the output is {int(host[at + room.at])} for {int(want[at + room.at])} (range {k} at "
                                 f"{e['offsets'][max(k, 0)]} of {e['sizes'][max(k, 0)] if k < len(e['sizes']) else '-'} bytes, out_size {room.out_size})")


def run(tsq, codec, case, out_size, what="", skew=0, idx=None, kind="device", refused_index=False):
    """one call with this room (out_size None: measure only), checked against takegen -> (Room, expectation)"""
    import torch
    idx = idx or index_of(tsq, codec, case.batch, kind, case.cap_blocks)
    room, t = Room(case.n, out_size, skew), Tables(case)
    torch.cuda.synchronize()
    rc = take_call(codec, idx, t, case.n, case.align, room)
    assert rc == 0, codec.last_error()
    torch.cuda.synchronize()
    e = case.expect(out_size if out_size is not None else 0, refused_index)
    check(case, room, e, what or case.name)
    return room, e


def decodes_to(codec, case, room, e, what):
    """the fitting prefix of the take, through tsqa_decompress_batch_packed_dense_async on the take's own tables, is the ranges' data"""
    import torch
    n = e["n_fit"]
    if n == 0:
        return
    assert e["item_status"][:n] == [0] * n
    want = b"".join(case.data(k) for k in range(n))
    blocks = sum(span[2] for span in e["spans"][:n])
    out = to_dev(sentinel(len(want) + FENCE))
    tables = codec._dense_tables(n)
    codec._join()
    codec.decompress_batch_packed_dense_async(room.arena(), room.offsets.t, room.sizes.t, n, blocks, 1, out[:len(want)], *tables)
    codec._join()
    assert codec.status() == 0 and not tables[3].any().item(), f"{what}: the dense decompress of the take refuses it"
    assert tables[1].cpu().tolist() == e["totals"][:n], what
    host = out.cpu().numpy()
    assert bytes(host[:len(want)]) == want and np.array_equal(host[len(want):], sentinel(host.size)[len(want):]), f"{what}: the take's data"
    del out
    torch.cuda.synchronize()


HEALTHY = None


def healthy(name):
    global HEALTHY
    if HEALTHY is None:
        HEALTHY = {c.name: c for c in tk.healthy_cases()}
    return HEALTHY[name]


HEALTHY_NAMES = ([f"ragged_{n}" for n in tk.COUNTS] + [f"ragged_257_align_{a}" for a in tk.ALIGNS] + [f"pass_edge_{n}" for n in tk.PASS_COUNTS] +
                 ["carry_inside_a_group", "carry_at_a_wavefront_edge", "identity", "permutation", "pages", "inner_ranges"])


def test_every_healthy_case_is_listed():
    assert sorted(HEALTHY_NAMES) == sorted(c.name for c in tk.healthy_cases())


@pytest.mark.parametrize("name", HEALTHY_NAMES)
def test_the_take_is_the_expected_arena_and_decodes_to_the_ranges(tsq, codec, name):
    case = healthy(name)
    room, e = run(tsq, codec, case, case.need)
    assert e["status"] == OK and e["n_fit"] == case.n
    decodes_to(codec, case, room, e, name)


def test_an_output_at_any_address(tsq, codec):
    """d_out need not be aligned: the words are cut at multiples of 16 of the address"""
    case = healthy("ragged_257_align_1")
    for skew in range(16):
        run(tsq, codec, case, case.need, f"{case.name} at skew {skew}", skew=skew)


def test_room_to_spare_changes_nothing(tsq, codec):
    case = healthy("ragged_513")
    run(tsq, codec, case, case.need + 100_001)


@pytest.mark.parametrize("k", range(27))
def test_a_refusal_is_refused_alone(tsq, codec, k):
    case = tk.refusal_cases()[k]
    room, e = run(tsq, codec, case, case.need)
    bad = [j for j, st in enumerate(e["item_status"]) if st]
    if case.name.startswith("edge_range"):
        assert bad == [] and e["status"] == OK
        return
    assert bad and e["status"] == ERR_ARG and all(e["item_status"][j] == ERR_ARG for j in bad)
    assert set(tk.REFUSAL_AT) & set(bad) or case.name.startswith("refusal_")
    run(tsq, codec, case, None, case.name + ", measured")


def test_the_refusal_cases_are_27():
    assert len(tk.refusal_cases()) == 27


@pytest.mark.parametrize("k", range(5))
def test_rooms_and_the_retry_with_the_reported_room(tsq, codec, k):
    what, case, out_size, n_fit = tk.rooms()[k]
    room, e = run(tsq, codec, case, out_size, what)
    assert e["n_fit"] == n_fit
    if out_size is not None:
        decodes_to(codec, case, room, e, what)
    if e["status"] == OK:
        return
    assert e["status"] == ERR_OVERFLOW
    need = room.offsets.values()[-1]
    room, e = run(tsq, codec, case, need, what + ", the retry")
    assert e["status"] == OK and need == case.need


@pytest.mark.parametrize("name", ["pass_edge_65537", "carry_at_a_wavefront_edge", "refusal"])
def test_the_three_launches_lay_out_what_the_host_planner_does(tsq, codec, name):
    """d_offsets, d_sizes, d_totals, the statuses and d_offsets[n] against tsqa_plan_cut_items, entry for entry, for all the room in
    the world, a room that ends in the middle, and none"""
    import torch
    case = tk.bad_range("first_all_ones_count_2", 256) if name == "refusal" else healthy(name)
    ix = case.index
    frame_at, out_start = ix.plan_tables()
    idx, t = index_of(tsq, codec, case.batch, "device", case.cap_blocks), Tables(case)
    mid = case.expect(1 << 62)["offsets"][case.n // 2] + 20
    for out_size in (case.need, mid, None):
        room = Room(case.n, out_size)
        torch.cuda.synchronize()
        assert take_call(codec, idx, t, case.n, case.align, room) == 0, codec.last_error()
        torch.cuda.synchronize()
        offsets, sizes, totals, status, n_fit = tsq.plan_cut_items(frame_at, out_start, ix.item_first, case.items, case.ranges, case.align, out_size or 0)
        assert room.offsets.values() == offsets and room.sizes.values() == sizes and room.totals.values() == totals, (name, out_size)
        got = room.item_status.values()
        assert got == status and room.word.values() == [max(status)], (name, out_size)
        assert next((k for k, st in enumerate(got) if st == ERR_OVERFLOW), case.n) == n_fit


def test_through_one_container_the_take_is_the_cut(tsq, codec):
    """tsqa_cut_async and tsqa_cut_items_async with d_items NULL on the same index and the same ranges: the same tables and the same
    arena, for few ranges and for more than launch (b) takes in a pass.  Both calls run the same kernels, so each of them is also
    held, entry for entry, to two sources that share nothing with the kernels: the host planner (tsqa_plan_cut) and cutgen's
    pure-Python layout and containers; every byte of the fenced output outside a fitting container keeps its sentinel."""
    import torch
    case, cut = tk.single("tiny")
    idx = index_of(tsq, codec, case.batch, "plain")
    many = [cut.ranges[k % len(cut.ranges)] for k in range(tk.PASS + 1)]
    for ranges, align in ((cut.ranges, cut.align), (many, 1)):
        n = len(ranges)
        model = cg.Case(f"tiny_{n}_ranges_through_both_calls", cut.source, ranges, align)
        d_first, d_count = u64_dev(f for f, _ in ranges), u64_dev(c for _, c in ranges)
        need = cg.plan_cut(cut.source.frame_at, cut.source.out_start, ranges, align, 1 << 62)[0][-1]
        for out_size in (need, need // 2, None):
            e = model.expect(out_size or 0)
            offsets, sizes, totals, status, n_fit = tsq.plan_cut(cut.source.frame_at, cut.source.out_start, ranges, align, out_size or 0)
            assert (offsets, sizes, totals, status, n_fit) == (e["offsets"], e["sizes"], e["totals"], e["item_status"], e["n_fit"]), (n, out_size)
            a, b = Room(n, out_size), Room(n, out_size)
            torch.cuda.synchronize()
            rc = codec.L.tsqa_cut_async(codec.h, idx.h, d_first.data_ptr(), d_count.data_ptr(), n, align, a.out_ptr(), out_size or 0, a.offsets.ptr(),
                                        a.sizes.ptr(), a.totals.ptr(), a.item_status.ptr(), a.word.ptr(), codec._stream())
            assert rc == 0, codec.last_error()
            rc = codec.L.tsqa_cut_items_async(codec.h, idx.h, None, d_first.data_ptr(), d_count.data_ptr(), n, align, b.out_ptr(), out_size or 0,
                                              b.offsets.ptr(), b.sizes.ptr(), b.totals.ptr(), b.item_status.ptr(), b.word.ptr(), codec._stream())
            assert rc == 0, codec.last_error()
            torch.cuda.synchronize()
            for ta, tb in zip(a.tables(), b.tables()):
                assert torch.equal(ta.buf, tb.buf), (n, out_size)
            assert out_size is None or torch.equal(a.buf, b.buf), (n, out_size)
            assert a.word.values() == [OK if out_size == need else ERR_OVERFLOW]
            for room, who in ((a, "tsqa_cut_async"), (b, "tsqa_cut_items_async")):
                what = f"{who}, {n} ranges, out_size {out_size}"
                check(model, room, e, what + ", against cutgen")
                got = (room.offsets.values(), room.sizes.values(), room.totals.values(), room.item_status.values())
                for name, table, owed in zip(("offsets", "sizes", "totals", "item_status"), got, (offsets, sizes, totals, status)):
                    assert table == owed, f"{what}: d_{name} against tsqa_plan_cut {first_difference(table, owed)} (range, got, owed)"
                assert room.word.values() == [max(status)], what
                assert next((k for k, st in enumerate(got[3]) if st == ERR_OVERFLOW), n) == n_fit, what
    run(tsq, codec, case, case.need, "a plain index, item 0 named", idx=idx)


def test_every_kind_of_index_gives_the_same_arena(tsq, codec):
    import torch
    case = tk.kinds_case()
    rooms = [run(tsq, codec, case, case.need, f"{case.name} through a {kind} index", kind=kind)[0] for kind in ("batch", "device", "fetched")]
    for r in rooms[1:]:
        assert torch.equal(r.buf, rooms[0].buf) and all(torch.equal(a.buf, b.buf) for a, b in zip(r.tables(), rooms[0].tables()))
    fetched, device = index_of(tsq, codec, case.batch, "fetched"), index_of(tsq, codec, case.batch, "device")
    assert fetched.fetched and not device.fetched and device.n_blocks == 0 and fetched.n_blocks == case.index.n_blocks
    case = tk.sized_batch_case()
    a, e = run(tsq, codec, case, case.need, "the sized form", kind="sized")
    b, _ = run(tsq, codec, case, case.need, "the plain form on the same batch", kind="device")
    assert torch.equal(a.buf, b.buf) and e["status"] == OK
    decodes_to(codec, case, a, e, "the sized form")
    case, _ = tk.single("split")
    run(tsq, codec, case, case.need, "a sized index of one container", kind="sized_one")
    # a batch index of one item whose container starts 48 bytes into its buffer: d_items NULL names item 0
    case, cut = tk.single("tiny")
    blob = np.frombuffer(cut.source.blob, dtype=np.uint8)
    buf = to_dev(np.concatenate([sentinel(48), blob, sentinel(100)]))
    torch.cuda.synchronize()
    one = tsq.BatchIndex(codec, buf, [(48, blob.size + 5)])
    room, t = Room(case.n, case.need), Tables(case)
    assert take_call(codec, one, t, case.n, case.align, room, items=None) == 0, codec.last_error()
    torch.cuda.synchronize()
    e = case.expect(case.need)
    moved = dict(e, spans=[(a + 48, z + 48, c, tot) for a, z, c, tot in e["spans"]])
    shifted = tk.Case("shifted", tk.Batch("shifted", buf.cpu().numpy(), [48], [blob.size + 5], [None]), case.items, case.ranges, case.align)
    check(shifted, room, moved, "a batch index of one item, d_items NULL")
    one.close()


def test_a_refused_sized_index_refuses_every_range_and_nothing_is_written(tsq, codec):
    import torch
    blob, table, n_total, block_len, case = tk.refused_index()
    d_blob = to_dev(np.frombuffer(blob, dtype=np.uint8))
    bad = tsq.SizedIndex(codec, d_blob, n_total, block_len, to_dev(table, np.int32), sync=False)
    room, e = run(tsq, codec, case, case.need, "a sized index with a false table", idx=bad, refused_index=True)
    assert e["status"] == ERR_FORMAT and e["item_status"] == [ERR_FORMAT] * case.n and e["offsets"] == [0] * (case.n + 1)
    assert np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel()))
    run(tsq, codec, case, None, "a sized index with a false table, measured", idx=bad, refused_index=True)
    torch.cuda.synchronize()
    bad.close()
    good = tsq.SizedIndex(codec, d_blob, n_total, block_len, to_dev(case.batch.table, np.int32), sync=False)
    room, e = run(tsq, codec, case, case.need, "the same container with its true table", idx=good)
    assert e["item_status"] == [0, 0, 0, 0, ERR_ARG]
    torch.cuda.synchronize()
    good.close()


def test_the_waiting_form_fills_host_tables(tsq, codec):
    import torch
    case = tk.inner_ranges()
    n, idx, t = case.n, index_of(tsq, codec, case.batch, "device"), Tables(case)
    offsets, sizes, totals, status = (C.c_uint64 * (n + 1))(), (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_int32 * n)()
    for out_size in (case.need, case.need - 1, None):
        room = Room(n, out_size)
        torch.cuda.synchronize()
        rc = codec.L.tsqa_cut_items(codec.h, idx.h, t.items.data_ptr(), t.first.data_ptr(), t.count.data_ptr(), n, 16, room.out_ptr(), out_size or 0,
                                    offsets, sizes, totals, status, codec._stream())
        e = case.expect(out_size or 0)
        assert rc == e["status"] and (list(offsets), list(sizes), list(totals), list(status)) == (e["offsets"], e["sizes"], e["totals"], e["item_status"])
        if out_size:
            assert np.array_equal(room.arena().cpu().numpy(), case.arena(e, sentinel(room.buf.numel())[room.at:room.at + out_size]))
    room = Room(n, case.need)
    args = [codec.h, idx.h, t.items.data_ptr(), t.first.data_ptr(), t.count.data_ptr(), n, 16, room.out_ptr(), case.need, offsets, sizes, None, status,
            codec._stream()]
    assert codec.L.tsqa_cut_items(*args) == 0, "totals may be NULL"
    for k in (1, 2, 3, 4, 9, 10, 12):                        # (items: the index has ten; first or count alone)
        refused = list(args)
        refused[k] = None
        assert codec.L.tsqa_cut_items(*refused) == ERR_ARG, k


def test_host_refusals_write_nothing(tsq, codec):
    import torch
    case = tk.inner_ranges()
    n, idx, t = case.n, index_of(tsq, codec, case.batch, "device"), Tables(case)
    fetched, size = index_of(tsq, codec, case.batch, "fetched"), case.need
    src = idx.blob
    inside = src.data_ptr()
    bad = [("a NULL index", dict(idx=None)), ("NULL firsts alone", dict(first=None)), ("NULL counts alone", dict(count=None)),
           ("NULL items with ten items", dict(items=None)), ("NULL items with ten items, fetched", dict(idx=fetched.h, items=None)),
           ("NULL offsets", dict(offsets=None)), ("NULL sizes", dict(sizes=None)), ("NULL item statuses", dict(item_status=None)),
           ("a NULL status word", dict(status=None)), ("no ranges", dict(n=0)), ("align 0", dict(align=0)), ("align 24", dict(align=24)),
           ("align 8192", dict(align=8192)), ("an output of 15 bytes", dict(out_size=15)), ("no output but a size", dict(out=None, out_size=size)),
           ("an output that starts inside the arena", dict(out=inside + 8, out_size=size)),
           ("an output that ends inside the arena", dict(out=inside - size + 1, out_size=size)),
           ("an output that holds the arena", dict(out=inside - 16, out_size=src.numel() + 32)),
           ("sums that could pass 2^55", dict(n=2**32 - 1, out=None, out_size=0) if (2**32 - 1) * (src.numel() + 4096) >= 1 << 55 else dict(n=0))]
    for what, over in bad:
        room = Room(n, size)
        torch.cuda.synchronize()
        assert take_call(codec, idx, t, n, 16, room, **over) == ERR_ARG, what
        torch.cuda.synchronize()
        assert all(tb.untouched() for tb in room.tables()), what
        assert np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel())), what
    room = Room(n, size)
    assert take_call(codec, idx, t, n, 16, room, ctx=None) == ERR_ARG, "a NULL context"
    # what is refused above is accepted one step inside the rule: whole items, no totals, another align
    room = Room(n, 10 * 4096 + (1 << 16))
    assert take_call(codec, idx, t, n, 4096, room, first=None, count=None, totals=None) == 0, codec.last_error()
    torch.cuda.synchronize()
    assert room.word.values() == [0] and room.totals.untouched() and room.offsets.values()[1] % 4096 == 0
    whole = tk.Case("whole", case.batch, case.items, None, 4096)
    assert room.sizes.values() == whole.expect(1 << 62)["sizes"]


def _texts(tsq, n, seed, lo=1, hi=20_000):
    rng = np.random.default_rng(seed)
    return [tsq.synth.text(int(rng.integers(lo, hi + 1)), seed=seed + k) for k in range(n)]


def test_chain_compress_index_choose_take_decompress_on_one_stream(tsq):
    """packed compress -> plain device index -> item numbers drawn on the device -> take -> dense decompress, on one stream with no
    host read in between; twice back to back, the second with more items and ranges than the scratch holds"""
    import torch
    fresh = tsq.DeviceCodec(0)
    side = torch.cuda.Stream()
    try:
        runs = []
        with torch.cuda.stream(side):
            side.wait_stream(torch.cuda.default_stream())
            for n_items, n_take, seed in ((16, 40, 3), (280, 700, 4)):
                rng = np.random.default_rng(tk.SEED + seed)
                sizes = [int(x) for x in rng.integers(200, 9000, n_items)]
                data = tsq.synth.text(sum(sizes), seed=seed)
                in_offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).tolist()
                d_data = to_dev(data)
                arena = torch.empty(sum(tsq.batch_bound(z) + 16 for z in sizes), dtype=torch.uint8, device="cuda")
                i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device="cuda")
                d_offsets, d_sizes = i64(n_items + 1), i64(n_items)
                status = []
                fresh.compress_batch_packed_async(d_data, list(zip(in_offsets, sizes)), 1, 16, arena, d_offsets, d_sizes)
                status.append(fresh._status.clone())
                index = fresh.index_packed_async(arena, d_offsets, d_sizes, n_items, n_items)
                status.append(fresh._status.clone())
                d_items = torch.randint(0, n_items, (n_take,), device="cuda", dtype=torch.int32)
                taken = to_dev(sentinel(3 * arena.numel() + FENCE))
                t_offsets, t_sizes, t_totals, t_status = i64(n_take + 1), i64(n_take), i64(n_take), torch.full((n_take,), -1, dtype=torch.int32, device="cuda")
                fresh.cut_items_async(index, d_items, None, None, n_take, 16, taken[:3 * arena.numel()], t_offsets, t_sizes, t_totals, t_status)
                status.append(fresh._status.clone())
                back = to_dev(sentinel(3 * data.size + FENCE))
                tables = fresh._dense_tables(n_take)
                fresh.decompress_batch_packed_dense_async(taken[:3 * arena.numel()], t_offsets, t_sizes, n_take, n_take, 1, back[:3 * data.size], *tables)
                status.append(fresh._status.clone())
                runs.append((data, in_offsets, sizes, index, d_items, taken, arena, t_offsets, t_totals, t_status, back, tables, status))
        side.synchronize()
        for data, in_offsets, sizes, index, d_items, taken, arena, t_offsets, t_totals, t_status, back, tables, status in runs:
            assert [int(s.item()) for s in status] == [OK] * 4
            chosen = d_items.cpu().tolist()
            assert not t_status.any().item() and t_totals.cpu().tolist() == [sizes[i] for i in chosen]
            want = np.concatenate([data[in_offsets[i]:in_offsets[i] + sizes[i]] for i in chosen])
            assert want.size <= 3 * data.size and tables[0][-1].item() == want.size
            host = back.cpu().numpy()
            assert np.array_equal(host[:want.size], want) and np.array_equal(host[want.size:], sentinel(host.size)[want.size:])
            used = int(t_offsets[-1].item())
            assert np.array_equal(taken.cpu().numpy()[used:], sentinel(taken.numel())[used:]), "bytes behind the taken arena"
            index.close()
    finally:
        fresh.close()


def test_chain_take_join_decompress(tsq, codec):
    """take -> join -> tsqa_decompress_device_async on one stream: the permuted concatenation"""
    import torch
    datas = _texts(tsq, 120, 900)
    batch = codec.compress_batch_packed([to_dev(d) for d in datas], 1, align=16)
    perm = np.random.default_rng(tk.SEED).integers(0, 120, 200)
    want = np.concatenate([datas[i] for i in perm])
    side = torch.cuda.Stream()
    n = len(perm)
    with torch.cuda.stream(side):
        side.wait_stream(torch.cuda.default_stream())
        index = batch.index(sync=False)
        d_items = to_dev(perm.astype(np.int32))
        i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device="cuda")
        room = 3 * batch.arena.numel()
        taken, t_offsets, t_sizes, t_status = torch.empty(room, dtype=torch.uint8, device="cuda"), i64(n + 1), i64(n), torch.full((n,), -1, dtype=torch.int32, device="cuda")
        codec.cut_items_async(index, d_items, None, None, n, 16, taken, t_offsets, t_sizes, None, t_status)
        st_take = codec._status.clone()
        joined, j_first, j_status = to_dev(sentinel(room)), i64(n + 1), torch.full((n,), -1, dtype=torch.int32, device="cuda")
        codec.join_async(taken, t_offsets, t_sizes, n, n, joined, j_first, None, j_status)
        st_join, size = codec._status.clone(), codec._size.clone()
        back = to_dev(sentinel(want.size + FENCE))
        codec.decompress_async(joined, n, back[:want.size])
        st_back, got = codec._status.clone(), codec._size.clone()
    side.synchronize()
    assert (int(st_take.item()), int(st_join.item()), int(st_back.item())) == (OK, OK, OK)
    assert not t_status.any().item() and not j_status.any().item() and int(got.item()) == want.size
    host = back.cpu().numpy()
    assert np.array_equal(host[:want.size], want) and np.array_equal(host[want.size:], sentinel(host.size)[want.size:])
    # the joined container is the taken containers' frames behind one header
    arena, offs, szs = taken.cpu().numpy(), t_offsets.cpu().tolist(), t_sizes.cpu().tolist()
    assert bytes(joined[16:int(size.item())].cpu().numpy()) == b"".join(arena[o + 16:o + z].tobytes() for o, z in zip(offs, szs))
    index.close()


def test_python_take_round_trips(tsq, codec):
    import torch
    datas = [tsq.synth.text(n, seed=n) for n in (5000, 100, 3 * 4096 + 1, 70000, 1)]
    srcs = [to_dev(d) for d in datas]
    for batch in (codec.compress_batch_packed(srcs, 1), codec.compress_batch_packed(srcs, 1, block_len=4096)):
        pick = [3, 0, 0, 4, 2]
        taken = batch.take(pick)
        assert isinstance(taken, tsq.PackedBatch) and taken.lengths == [datas[i].size for i in pick]
        assert taken.arena.numel() == taken.offsets[-1] and all(o % 16 == 0 for o in taken.offsets[:-1])
        for v, i in zip(taken.views, pick):
            assert torch.equal(v, batch.views[i])
        for v, i in zip(taken.decompress(), pick):
            assert np.array_equal(v.cpu().numpy(), datas[i])
        assert np.array_equal(codec.decompress(taken.join()).cpu().numpy(), np.concatenate([datas[i] for i in pick]))
        # item numbers born on the device, nothing waited for: a from_device batch
        d_items = to_dev(np.array(pick, dtype=np.int32))
        later = batch.take(to_dev(np.array([4, 3, 2, 1, 0], dtype=np.int32)), align=4096, sync=False)     # (no repeats: the default room holds it)
        assert codec.status() == OK and not later.d_item_status.any().item() and later.lengths == [d.size for d in datas[::-1]]
        assert all(torch.equal(v, w) for v, w in zip(later.views, batch.views[::-1]))
        roomy = batch.take(d_items, align=4096, out=torch.empty(6 * 4096 + batch.arena.numel() * 3, dtype=torch.uint8, device="cuda"), sync=False)
        assert codec.status() == OK and not roomy.d_item_status.any().item() and roomy.lengths == taken.lengths
        assert all(o % 4096 == 0 for o in roomy.offsets[:-1]) and [bytes(v.cpu().numpy()) for v in roomy.views] == [bytes(v.cpu().numpy()) for v in taken.views]
        # pages of the long item through the batch's index, before and after fetch()
        index = batch.index(sync=False)
        assert not hasattr(index, "cut")
        if batch.block_len:
            d3 = to_dev(np.array([3] * 18, dtype=np.int32))
            pages = index.cut_items(d3, u64_dev(range(18)), u64_dev([1] * 18))
            assert pages.lengths == [4096] * 17 + [70000 - 17 * 4096]
            assert np.array_equal(torch.cat(pages.decompress()).cpu().numpy(), datas[3])
            again = index.fetch().cut_items(d3, u64_dev(range(18)), u64_dev([1] * 18))
            assert again.offsets == pages.offsets and all(torch.equal(v, w) for v, w in zip(again.views, pages.views))     # (padding is nobody's)
        # a refused range, and an `out` that is too small
        with pytest.raises(tsq.TsqError) as err:
            index.cut_items([0, 5, 1])
        assert err.value.code == ERR_ARG and err.value.item_status == [ERR_OVERFLOW, ERR_ARG, ERR_OVERFLOW]
        with pytest.raises(tsq.TsqError) as err:
            index.cut_items(pick, out=torch.empty(taken.offsets[-1] - 1, dtype=torch.uint8, device="cuda"))
        assert err.value.code == ERR_OVERFLOW and err.value.needed == taken.offsets[-1] and err.value.item_status == [0, 0, 0, 0, ERR_OVERFLOW]
        index.close()
    both = codec.index_batch([batch.views[0], batch.views[1]])
    got = both.cut_items([1, 0])
    assert torch.equal(got.views[0], batch.views[1]) and torch.equal(got.views[1], batch.views[0])
    both.close()


def test_the_copy_kernel_is_timed_alone(tsq, codec):
    case = healthy("carry_inside_a_group")
    codec.profile(True)
    codec.profile_read_cut()
    try:
        run(tsq, codec, case, case.need)
        run(tsq, codec, case, None, "measured: no copy")
        ms, launches = codec.profile_read_cut()
        assert launches == 1 and 0 < ms < 100
    finally:
        codec.profile(False)
