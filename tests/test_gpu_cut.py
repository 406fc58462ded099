"""GPU tests of the cut (tsqa_cut_async, tsqa_cut, DeviceCodec.cut_async, RangeIndex.cut): the cases are cutgen's, the expected
arena, tables and statuses are made there in pure Python from the source's bytes, and test_cut_cpu.py shows that each case reaches
what it aims at.  Every buffer and table the library may write is filled with a sentinel first, with a fence on both sides, and must
keep it wherever the call owes nothing: padding, the room of ranges that do not fit, and everything behind a refusal."""
import ctypes as C

import numpy as np
import pytest

import cutgen as cg

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = cg.OK, cg.ERR_ARG, cg.ERR_FORMAT, cg.ERR_OVERFLOW
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
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (the pattern repeats every 251 bytes): test_gpu_join.py's"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


def u64_dev(values):
    """any 64-bit values as an int64 CUDA tensor"""
    return to_dev(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64))


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
        host = self.buf.cpu().tolist()
        assert host[:TABLE_FENCE] == [TABLE_GUARD] * TABLE_FENCE and host[TABLE_FENCE + self.n:] == [TABLE_GUARD] * TABLE_FENCE, "a table's fence"
        return host[TABLE_FENCE:TABLE_FENCE + self.n]

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


class Index:
    """a tsqa_index through the C ABI: kind 'plain' (tsqa_index_create), 'sized' (tsqa_index_create_sized_async on the current
    stream, nothing waited for) or 'batch' (tsqa_index_create_batch over `spans` of the buffer)"""

    def __init__(self, codec, kind, blob, n_total=None, block_len=None, table=None, spans=None):
        import torch
        from turbosqueeze_amd.api import _batch_array
        self.codec, self.blob, self.h = codec, blob, C.c_void_p()
        if kind == "plain":
            torch.cuda.synchronize()
            rc = codec.L.tsqa_index_create(codec.h, blob.data_ptr(), blob.numel(), C.byref(self.h))
        elif kind == "sized":
            self.table = to_dev(table, np.int32) if not hasattr(table, "data_ptr") else table
            rc = codec.L.tsqa_index_create_sized_async(codec.h, blob.data_ptr(), blob.numel(), n_total, block_len, self.table.data_ptr(),
                                                       C.byref(self.h), codec._stream())
        else:
            torch.cuda.synchronize()
            rc = codec.L.tsqa_index_create_batch(codec.h, blob.data_ptr(), blob.numel(), _batch_array([(a, n, 0, 0) for a, n in spans]), len(spans),
                                                 C.byref(self.h), None)
        assert rc == 0, codec.last_error()

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.codec.L.tsqa_index_destroy(self.h)


_SOURCES = {}


def index_of(codec, source, kind=None):
    """-> the Index of a cutgen source, made once: sized where the source has a table and a block length below a block, else plain"""
    kind = kind or ("sized" if source.name == "split" else "plain")
    key = (source.name, kind)
    if key not in _SOURCES:
        blob = to_dev(np.frombuffer(source.blob, dtype=np.uint8))
        _SOURCES[key] = (Index(codec, kind, blob, len(source.data), source.block_len, source.table) if kind == "sized" else
                         Index(codec, kind, blob))
    return _SOURCES[key]


def cut_call(codec, index, d_first, d_count, n_ranges, align_to, room, **over):
    """tsqa_cut_async on the current stream -> its return value.  over: arguments replaced."""
    a = dict(ctx=codec.h, idx=index.h, first=d_first.data_ptr(), count=d_count.data_ptr(), n=n_ranges, align=align_to, out=room.out_ptr(),
             out_size=room.out_size or 0, offsets=room.offsets.ptr(), sizes=room.sizes.ptr(), totals=room.totals.ptr(),
             item_status=room.item_status.ptr(), status=room.word.ptr())
    a.update(over)
    return codec.L.tsqa_cut_async(a["ctx"], a["idx"], a["first"], a["count"], a["n"], a["align"], a["out"], a["out_size"], a["offsets"], a["sizes"],
                                  a["totals"], a["item_status"], a["status"], codec._stream())


def check(case, room, e, what):
    """the tables, the statuses and every byte of the fenced output against cutgen's `e`"""
    got_status = room.item_status.values()
    assert got_status == e["item_status"], (f"{what}: item statuses "
                                            f"{[(k, g, w) for k, (g, w) in enumerate(zip(got_status, e['item_status'])) if g != w][:8]} (range, got, owed)")
    assert room.word.values() == [e["status"]], f"{what}: *d_status is {room.word.values()}, owed {e['status']}"
    for name, table in (("offsets", room.offsets), ("sizes", room.sizes), ("totals", room.totals)):
        got = table.values()
        assert got == e[name], f"{what}: d_{name} {[(k, g, w) for k, (g, w) in enumerate(zip(got, e[name])) if g != w][:8]} (range, got, owed)"
    if room.buf is not None:
        want = sentinel(room.buf.numel())
        want[room.at:room.at + room.out_size] = case.arena(e, want[room.at:room.at + room.out_size])
        host = room.buf.cpu().numpy()
        if not np.array_equal(host, want):
            at = int(np.flatnonzero(host != want)[0]) - room.at
            k = int(np.searchsorted(np.array(e["offsets"]), at, side="right")) - 1
            raise AssertionError(f"{what}: byte {at} of the output is {int(host[at + room.at])} for {int(want[at + room.at])} (range {k} at "
                                 f"{e['offsets'][max(k, 0)]} of {e['sizes'][max(k, 0)] if k < len(e['sizes']) else '-'} bytes, out_size {room.out_size})")


def run(codec, case, out_size, what="", skew=0, idx=None, refused_index=False):
    """one call with this room (out_size None: measure only), checked against cutgen -> (Room, expectation)"""
    import torch
    n = len(case.ranges)
    idx = idx or index_of(codec, case.source)
    room = Room(n, out_size, skew)
    d_first, d_count = u64_dev(f for f, _ in case.ranges), u64_dev(c for _, c in case.ranges)
    torch.cuda.synchronize()
    rc = cut_call(codec, idx, d_first, d_count, n, case.align, room)
    assert rc == 0, codec.last_error()
    torch.cuda.synchronize()
    e = case.expect(out_size if out_size is not None else 0, refused_index)
    check(case, room, e, what or case.name)
    return room, e


def decodes_to(codec, case, room, e, what):
    """the fitting prefix of the cut, through tsqa_decompress_batch_packed_dense_async on the cut's own tables, is the ranges' data"""
    import torch
    n = e["n_fit"]
    if n == 0:
        return
    assert e["item_status"][:n] == [0] * n
    want = b"".join(case.data(k) for k in range(n))
    blocks = sum(c for _, c in case.ranges[:n])
    out = to_dev(sentinel(len(want) + FENCE))
    tables = codec._dense_tables(n)
    codec._join()
    codec.decompress_batch_packed_dense_async(room.arena(), room.offsets.t, room.sizes.t, n, blocks, 1, out[:len(want)], *tables)
    codec._join()
    assert codec.status() == 0 and tables[3].cpu().tolist() == [0] * n, f"{what}: the dense decompress of the cut refuses it"
    assert tables[1].cpu().tolist() == e["totals"][:n], what
    host = out.cpu().numpy()
    assert bytes(host[:len(want)]) == want and np.array_equal(host[len(want):], sentinel(host.size)[len(want):]), f"{what}: the cut's data"
    del out
    torch.cuda.synchronize()


HEALTHY = None


def healthy(name):
    global HEALTHY
    if HEALTHY is None:
        HEALTHY = {c.name: c for c in cg.healthy_cases()}
    return HEALTHY[name]


HEALTHY_NAMES = ([f"tiny_{n}" for n in cg.COUNTS] + [f"tiny_257_align_{a}" for a in cg.ALIGNS] + [f"whole_{n}" for n in cg.WHOLE] +
                 ["two_blocks_each", "split_ranges", "carry_inside_a_wavefront", "carry_at_a_wavefront_edge"])


def test_every_healthy_case_is_listed():
    assert sorted(HEALTHY_NAMES) == sorted(c.name for c in cg.healthy_cases())


@pytest.mark.parametrize("name", HEALTHY_NAMES)
def test_the_cut_is_the_expected_arena_and_decodes_to_the_ranges(codec, name):
    case = healthy(name)
    room, e = run(codec, case, case.need)
    assert e["status"] == OK and e["n_fit"] == len(case.ranges)
    decodes_to(codec, case, room, e, name)


@pytest.mark.parametrize("align", cg.ALIGNS)
def test_an_output_at_any_address(codec, align):
    """d_out need not be aligned: the words are cut at multiples of 16 of the address"""
    case = healthy(f"tiny_257_align_{align}")
    for skew in range(16):
        run(codec, case, case.need, f"{case.name} at skew {skew}", skew=skew)


def test_room_to_spare_changes_nothing(codec):
    case = healthy("tiny_513")
    run(codec, case, case.need + 100_001)
    case = healthy("split_ranges")
    run(codec, case, case.need + 17)


@pytest.mark.parametrize("name,at", cg.refusal_cases())
def test_a_refused_range_is_refused_alone(codec, name, at):
    case = cg.refusal(name, at)
    room, e = run(codec, case, case.need)
    assert e["status"] == ERR_ARG and e["item_status"][at] == ERR_ARG and sum(e["item_status"]) == ERR_ARG


@pytest.mark.parametrize("k", range(5))
def test_rooms_and_the_retry_with_the_reported_room(codec, k):
    what, case, out_size, n_fit = cg.rooms()[k]
    room, e = run(codec, case, out_size, what)
    assert e["n_fit"] == n_fit
    if out_size is not None:
        decodes_to(codec, case, room, e, what)
    if e["status"] == OK:
        return
    assert e["status"] == ERR_OVERFLOW
    need = room.offsets.values()[-1]
    room, e = run(codec, case, need, what + ", the retry")
    assert e["status"] == OK and need == case.need


def test_the_waiting_form_fills_host_tables(codec):
    import torch
    case = healthy("tiny_257_align_16")
    n, idx = len(case.ranges), index_of(codec, case.source)
    d_first, d_count = u64_dev(f for f, _ in case.ranges), u64_dev(c for _, c in case.ranges)
    for out_size in (case.need, case.need - 1, None):
        room = Room(n, out_size)
        offsets, sizes, totals, status = (C.c_uint64 * (n + 1))(), (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_int32 * n)()
        torch.cuda.synchronize()
        rc = codec.L.tsqa_cut(codec.h, idx.h, d_first.data_ptr(), d_count.data_ptr(), n, 16, room.out_ptr(), out_size or 0, offsets, sizes, totals,
                              status, codec._stream())
        e = case.expect(out_size or 0)
        assert rc == e["status"] and (list(offsets), list(sizes), list(totals), list(status)) == (e["offsets"], e["sizes"], e["totals"], e["item_status"])
        if out_size:
            assert np.array_equal(room.arena().cpu().numpy(), case.arena(e, sentinel(room.buf.numel())[room.at:room.at + out_size]))
    room = Room(n, case.need)
    args = [codec.h, idx.h, d_first.data_ptr(), d_count.data_ptr(), n, 16, room.out_ptr(), case.need, offsets, sizes, None, status, codec._stream()]
    assert codec.L.tsqa_cut(*args) == 0, "totals may be NULL"
    for k in (1, 2, 3, 8, 9, 11):
        refused = list(args)
        refused[k] = None
        assert codec.L.tsqa_cut(*refused) == ERR_ARG, k


def test_host_refusals_write_nothing(codec):
    import torch
    case = healthy("tiny_2")
    n, idx = 2, index_of(codec, case.source)
    size = case.need
    d_first, d_count = u64_dev(f for f, _ in case.ranges), u64_dev(c for _, c in case.ranges)
    src = idx.blob
    inside = src.data_ptr()
    both = Index(codec, "batch", src, spans=[(0, src.numel()), (0, src.numel())])
    # a small container in front of 9 MiB: n_ranges * (bytes + 4096) reaches 2^55 at 2^32 - 1 ranges
    wide = torch.zeros(9 << 20, dtype=torch.uint8, device="cuda")
    wide[:src.numel()] = src
    roomy = Index(codec, "plain", wide)
    assert (2**32 - 1) * (wide.numel() + 4096) >= 1 << 55 > (2**32 - 1) * (src.numel() + 4096)
    bad = [("a NULL index", dict(idx=None)), ("NULL firsts", dict(first=None)), ("NULL counts", dict(count=None)),
           ("NULL offsets", dict(offsets=None)), ("NULL sizes", dict(sizes=None)), ("NULL item statuses", dict(item_status=None)),
           ("a NULL status word", dict(status=None)), ("no ranges", dict(n=0)), ("align 0", dict(align=0)), ("align 24", dict(align=24)),
           ("align 8192", dict(align=8192)), ("an index of two items", dict(idx=both.h)),
           ("an output of 15 bytes", dict(out_size=15)), ("no output but a size", dict(out=None, out_size=size)),
           ("an output that starts inside the container", dict(out=inside + 8, out_size=size)),
           ("an output that ends inside the container", dict(out=inside - size + 1, out_size=size)),
           ("an output that holds the container", dict(out=inside - 16, out_size=src.numel() + 32)),
           ("sums that could pass 2^55", dict(idx=roomy.h, n=2**32 - 1))]
    for what, over in bad:
        room = Room(n, size)
        torch.cuda.synchronize()
        assert cut_call(codec, idx, d_first, d_count, n, 16, room, **over) == ERR_ARG, what
        torch.cuda.synchronize()
        assert all(t.untouched() for t in room.tables()), what
        assert np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel())), what
    room = Room(n, size)
    assert cut_call(codec, idx, d_first, d_count, n, 16, room, ctx=None) == ERR_ARG, "a NULL context"
    # what is refused above is accepted one step inside the rule
    room = Room(n, size)
    assert cut_call(codec, roomy, d_first, d_count, n, case.align, room) == 0
    torch.cuda.synchronize()
    check(case, room, case.expect(size), "an index of 9 MiB of room")
    room = Room(n, size + 4096)
    assert cut_call(codec, idx, d_first, d_count, n, 4096, room, totals=None) == 0
    torch.cuda.synchronize()
    assert room.word.values() == [0] and room.totals.untouched() and room.offsets.values()[1] == 4096
    both.close()
    roomy.close()


def test_a_batch_index_of_one_item_is_cut_like_its_container(codec):
    """its descriptors are relative to the buffer: the container starts 48 bytes into it"""
    case = healthy("tiny_257_align_16")
    blob = np.frombuffer(case.source.blob, dtype=np.uint8)
    buf = to_dev(np.concatenate([sentinel(48), blob, sentinel(100)]))
    one = Index(codec, "batch", buf, spans=[(48, blob.size + 5)])
    assert codec.L.tsqa_index_items(one.h) == 1
    run(codec, case, case.need, "through a batch index of one item", idx=one)
    one.close()


def test_a_refused_sized_index_refuses_every_range_and_nothing_is_written(codec):
    import torch
    blob, table, n_total, block_len, case = cg.refused_index()
    d_blob = to_dev(np.frombuffer(blob, dtype=np.uint8))
    bad = Index(codec, "sized", d_blob, n_total, block_len, table)
    room, e = run(codec, case, case.need, "a sized index with a false table", idx=bad, refused_index=True)
    assert e["status"] == ERR_FORMAT and e["item_status"] == [ERR_FORMAT] * 5 and e["offsets"] == [0] * 6
    assert np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel()))
    run(codec, case, None, "a sized index with a false table, measured", idx=bad, refused_index=True)
    bad.close()
    # the true table: the same ranges are cut, and the one past the last block is refused alone
    good = Index(codec, "sized", d_blob, n_total, block_len, case.source.table)
    room, e = run(codec, case, case.need, "the same container with its true table", idx=good)
    assert e["item_status"] == [0, 0, 0, 0, ERR_ARG]
    good.close()


def _texts(tsq, n, seed, lo=1, hi=20_000):
    rng = np.random.default_rng(seed)
    return [tsq.synth.text(int(rng.integers(lo, hi + 1)), seed=seed + k) for k in range(n)]


@pytest.mark.parametrize("uniform", [False, True])
def test_unjoin_gives_the_packed_arena_back(codec, tsq, uniform):
    """packed compress -> join -> index -> cut at the join's d_first_block: the packed arena's containers, byte for byte"""
    import torch
    n = 300
    datas = [tsq.synth.text(4096, seed=40 + k) for k in range(n)] if uniform else _texts(tsq, n, 500)
    batch = codec.compress_batch_packed([to_dev(d) for d in datas], 1, align=16)
    d_offsets, d_sizes = to_dev(batch.offsets, np.int64), to_dev(batch.sizes, np.int64)
    joined = torch.empty(batch.arena.numel(), dtype=torch.uint8, device="cuda")
    d_first = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    table = torch.empty(n, dtype=torch.int32, device="cuda")
    d_status = torch.empty(n, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        stream.wait_stream(torch.cuda.default_stream())
        codec.join_async(batch.arena, d_offsets, d_sizes, n, n, joined, d_first, table, d_status)
        if uniform:
            idx = codec.index_sized(joined, n * 4096, 4096, table, sync=False)      # (the join's own table: nothing waited for)
        else:
            stream.synchronize()
            idx = codec.index(joined[:codec.last_size_status()[0]])
        d_count = d_first[1:] - d_first[:-1]
        room = Room(n, batch.arena.numel())
        rc = cut_call(codec, idx, d_first, d_count, n, 16, room)
        assert rc == 0, codec.last_error()
        stream.synchronize()
    assert room.word.values() == [0] and room.item_status.values() == [0] * n
    assert room.offsets.values() == batch.offsets and room.sizes.values() == batch.sizes and room.totals.values() == [d.size for d in datas]
    got, want = room.arena().cpu().numpy(), sentinel(room.buf.numel())[room.at:room.at + room.out_size]
    arena = batch.arena.cpu().numpy()
    for o, z in zip(batch.offsets, batch.sizes):
        want[o:o + z] = arena[o:o + z]
    assert np.array_equal(got, want)
    assert np.array_equal(room.buf.cpu().numpy()[:room.at], sentinel(room.at))
    idx.close()


@pytest.mark.parametrize("kind", ["sized", "plain"])
def test_edit_is_cut_then_join_on_one_stream(codec, tsq, kind):
    """cut(a, 0..k) and cut(a, k+1..nb), a new container between them, join, decompress: one stream, nothing read on the host
    between the calls but what tsqa_index_create itself reads; twice back to back, the second time with more ranges and items than
    the scratch holds"""
    import torch
    bl = 4096
    stream = torch.cuda.Stream()
    runs = []
    for nb, k, single in ((40, 17, False), (700, 300, True)):
        data = tsq.synth.text(nb * bl - 100, seed=60 + nb)
        new = tsq.synth.text(bl, seed=61 + nb)
        ranges = ([(b, 1) for b in range(nb) if b != k] if single else [(0, k), (k + 1, nb - k - 1)])
        at = k if single else 1                              # the new container's index among the join's items
        runs.append(dict(nb=nb, k=k, at=at, ranges=ranges, n=len(ranges), src=to_dev(data), new=to_dev(new),
                         want=np.concatenate([data[:k * bl], new, data[(k + 1) * bl:]])))
    for r in runs:
        n, room = r["n"], tsq.plan_split(r["src"].numel(), bl)[1]
        r["blob"] = to_dev(sentinel(room))
        r["table"] = torch.full((r["nb"],), TABLE_GUARD, dtype=torch.int32, device="cuda")
        r["new_blob"] = to_dev(sentinel(tsq.batch_bound(bl)))
        r["arena"] = to_dev(sentinel(room + 32 * n + 8192))       # the cuts at align 16 (a header and padding each), then the new container
        r["new_at"] = room + 32 * n
        r["first"], r["count"] = u64_dev(f for f, _ in r["ranges"]), u64_dev(c for _, c in r["ranges"])
        i64 = lambda m: torch.full((m,), -1, dtype=torch.int64, device="cuda")
        r["cut_offsets"], r["cut_sizes"], r["cut_status"] = i64(n + 1), i64(n), torch.full((n,), -1, dtype=torch.int32, device="cuda")
        r["joined"] = to_dev(sentinel(room + 8192))
        r["join_first"], r["join_table"] = i64(n + 2), torch.full((r["nb"],), TABLE_GUARD, dtype=torch.int32, device="cuda")
        r["join_status"] = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
        r["back"] = to_dev(sentinel(r["want"].size + FENCE))
        r["words"] = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for r in runs:
            n, at, w = r["n"], r["at"], r["words"]
            codec.compress_split_async(r["src"], 1, bl, r["blob"], r["table"])
            w[0:1].copy_(codec._size)
            codec.compress_async(r["new"], 0, r["new_blob"])
            w[1:2].copy_(codec._size)
            r["arena"][r["new_at"]:r["new_at"] + r["new_blob"].numel()].copy_(r["new_blob"])
            r["idx"] = (codec.index_sized(r["blob"], r["src"].numel(), bl, r["table"], sync=False) if kind == "sized" else
                        codec.index(r["blob"]))              # (plain: tsqa_index_create waits and reads the frames itself)
            codec.cut_async(r["idx"], r["first"], r["count"], n, 16, r["arena"][:r["new_at"]], r["cut_offsets"], r["cut_sizes"], None,
                            r["cut_status"])
            w[2:3].copy_(codec._status)
            # the join's tables, made on the device from the cut's
            new_place = torch.full((1,), r["new_at"], dtype=torch.int64, device="cuda")
            offsets = torch.cat([r["cut_offsets"][:at], new_place, r["cut_offsets"][at:n]])
            sizes = torch.cat([r["cut_sizes"][:at], w[1:2], r["cut_sizes"][at:n]])
            codec.join_async(r["arena"], offsets, sizes, n + 1, r["nb"], r["joined"], r["join_first"], r["join_table"], r["join_status"])
            w[3:4].copy_(codec._size)
            w[4:5].copy_(codec._status)
            if kind == "sized":
                codec.decompress_sized_async(r["joined"], r["nb"], r["join_table"], r["back"][:r["want"].size])
            else:
                codec.decompress_async(r["joined"], r["nb"], r["back"][:r["want"].size])
            w[5:6].copy_(codec._size)
            w[6:7].copy_(codec._status)
    stream.synchronize()
    for r in runs:
        w = r["words"].cpu().tolist()
        assert (w[2], w[4], w[6]) == (0, 0, 0), f"cut, join, decompress: {w}"
        assert r["cut_status"].cpu().tolist() == [0] * r["n"] and r["join_status"].cpu().tolist() == [0] * (r["n"] + 1)
        assert w[5] == r["want"].size
        back = r["back"].cpu().numpy()
        assert np.array_equal(back[:w[5]], r["want"]) and np.array_equal(back[w[5]:], sentinel(back.size)[w[5]:])
        assert r["join_first"][-1].item() == r["nb"]
        # the edited container: the source's frames around the new block's, which is the new container's own
        src, new, got = bytes(r["blob"][:w[0]].cpu().numpy()), bytes(r["new_blob"][:w[1]].cpu().numpy()), bytes(r["joined"][:w[3]].cpu().numpy())
        frame_at, _ = cg.walk(src)
        k = r["k"]
        assert got[16:] == src[16:frame_at[k]] + new[16:] + src[frame_at[k + 1]:frame_at[-1]]
        r["idx"].close()


def test_python_cut_round_trips(codec, tsq):
    import torch
    data = tsq.synth.text(50 * 4096 + 77, seed=70)
    src = to_dev(data)
    blob, table = codec.compress_split(src, 1, 4096, block_sizes=True)
    ranges = [(0, 3), (5, 2), (50, 1), (0, 51), (5, 2)]
    want = [data[f * 4096:(f + c) * 4096] for f, c in ranges]
    for idx in (codec.index(blob), codec.index_sized(blob, data.size, 4096, table)):
        batch = idx.cut(ranges)
        assert isinstance(batch, tsq.PackedBatch) and batch.lengths == [w.size for w in want]
        assert batch.arena.numel() == batch.offsets[-1] and all(o % 16 == 0 for o in batch.offsets[:-1])
        assert bytes(batch.views[3].cpu().numpy()) == bytes(blob.cpu().numpy())
        for v, w in zip(batch.decompress(), want):
            assert np.array_equal(v.cpu().numpy(), w)
        assert np.array_equal(codec.decompress(batch.join()).cpu().numpy(), np.concatenate(want))
        again = tsq.PackedBatch.from_device(codec, batch.arena, to_dev(batch.offsets, np.int64), to_dev(batch.sizes, np.int64))
        assert again.lengths == batch.lengths
        # ranges born on the device, another align, a caller's arena
        pair = (u64_dev(f for f, _ in ranges), u64_dev(c for _, c in ranges))
        out = to_dev(sentinel(batch.offsets[-1] + 5 * 4096))
        packed = idx.cut(pair, align=4096, out=out)
        assert packed.arena.data_ptr() == out.data_ptr() and [bytes(v.cpu().numpy()) for v in packed.views] == [bytes(v.cpu().numpy()) for v in batch.views]
        assert all(o % 4096 == 0 for o in packed.offsets[:-1])
        # an `out` that is too small: the bytes a retry needs
        with pytest.raises(tsq.TsqError) as err:
            idx.cut(ranges, out=torch.empty(batch.offsets[-1] - 1, dtype=torch.uint8, device="cuda"))
        assert err.value.code == ERR_OVERFLOW and err.value.needed == batch.offsets[-1] and err.value.item_status == [0, 0, 0, 0, ERR_OVERFLOW]
        assert "item statuses [0, 0, 0, 0, 6]" in str(err.value)
        retry = idx.cut(ranges, out=torch.empty(err.value.needed, dtype=torch.uint8, device="cuda"))
        assert retry.offsets == batch.offsets and all(torch.equal(a, b) for a, b in zip(retry.views, batch.views))
        with pytest.raises(tsq.TsqError) as err:
            idx.cut([(0, 1), (51, 1)])
        assert err.value.code == ERR_ARG and err.value.item_status == [ERR_OVERFLOW, ERR_ARG]
        idx.close()
    both = codec.index_batch([blob, blob])
    assert not hasattr(both, "cut") and hasattr(codec.index(blob), "cut")
    both.close()


def test_the_copy_kernel_is_timed_alone(codec):
    import torch
    case = healthy("carry_inside_a_wavefront")
    codec.profile(True)
    codec.profile_read_cut()
    try:
        run(codec, case, case.need)
        run(codec, case, None, "measured: no copy")
        ms, launches = codec.profile_read_cut()
        assert launches == 1 and 0 < ms < 100
        assert codec.profile_read_cut() == (0.0, 0) and codec.profile_read_join() == (0.0, 0)
    finally:
        codec.profile(False)
