"""GPU tests of the join (tsqa_join_async, tsqa_join, DeviceCodec.join, PackedBatch.join): the cases are joingen's, the expected
container is made there in pure Python from the items' bytes, and test_join_cpu.py shows that each case reaches what it aims at.
Every buffer the library writes is filled with a sentinel first, with a fence on both sides, and must keep it wherever the call owes
nothing: on any nonzero status that is the whole output and the whole table."""
import ctypes as C

import numpy as np
import pytest

import joingen as jg

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = jg.OK, jg.ERR_ARG, jg.ERR_FORMAT, jg.ERR_OVERFLOW
FENCE = 4096
TABLE_GUARD, TABLE_FENCE = 0x5EA1ED, 64


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
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (the pattern repeats every 251 bytes)"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


_ON_DEVICE = {}


def on_device(case):
    """-> (arena, d_offsets, d_sizes) of a case in device memory, made once"""
    if case.name not in _ON_DEVICE:
        _ON_DEVICE[case.name] = (to_dev(case.arena), to_dev(case.offsets, np.int64), to_dev(case.sizes, np.int64))
    return _ON_DEVICE[case.name]


class Room:
    """the call's outputs, filled with -1 or the table guard, and a fenced output of out_cap bytes that starts `skew` bytes past a
    multiple of 16 (out_cap None: measure only); table_words: the words of d_block_sizes the call may write (None: no table)"""

    def __init__(self, n, out_cap, table_words, skew=0):
        import torch
        self.first_block = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        self.item_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.word = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        self.out_cap, self.at = out_cap, FENCE + skew
        self.buf = to_dev(sentinel(2 * FENCE + 16 + out_cap)) if out_cap is not None else None
        if self.buf is not None:
            assert self.buf.data_ptr() % 16 == 0
        self.table = torch.full((table_words + TABLE_FENCE,), TABLE_GUARD, dtype=torch.int32, device="cuda") if table_words is not None else None

    def out_ptr(self):
        return self.buf.data_ptr() + self.at if self.buf is not None else None

    def container(self, size):
        return self.buf[self.at:self.at + size]


def join_call(codec, dev, n_items, room, blocks, **over):
    """tsqa_join_async on the current stream -> its return value.  over: arguments replaced."""
    arena, offsets, sizes = dev
    a = dict(arena=arena.data_ptr(), arena_size=arena.numel(), offsets=offsets.data_ptr(), sizes=sizes.data_ptr(), n=n_items, cap_blocks=blocks,
             out=room.out_ptr(), out_cap=room.out_cap or 0, size=room.size.data_ptr(),
             first_block=room.first_block.data_ptr(), table=room.table.data_ptr() if room.table is not None else None,
             item_status=room.item_status.data_ptr(), status=room.word.data_ptr())
    a.update(over)
    return codec.L.tsqa_join_async(codec.h, a["arena"], a["arena_size"], a["offsets"], a["sizes"], a["n"], a["cap_blocks"], a["out"], a["out_cap"],
                                   a["size"], a["first_block"], a["table"], a["item_status"], a["status"], codec._stream())


def check(case, room, e, what):
    """the tables, the verdicts, the size, and every byte of the fenced output and every word of the table against joingen's `e`"""
    got_status = room.item_status.cpu().tolist()
    assert room.first_block.cpu().tolist() == e["first_block"], f"{what}: d_first_block"
    assert got_status == e["item_status"], (f"{what}: item statuses "
                                            f"{[(k, g, w) for k, (g, w) in enumerate(zip(got_status, e['item_status'])) if g != w][:8]} (item, got, owed)")
    assert int(room.word.item()) == e["status"], f"{what}: *d_status is {int(room.word.item())}, owed {e['status']}"
    assert int(room.size.item()) == e["out_size"], f"{what}: *d_out_size is {int(room.size.item())}, owed {e['out_size']}"
    if room.buf is not None:
        want = sentinel(room.buf.numel())
        if e["container"] is not None:
            want[room.at:room.at + len(e["container"])] = np.frombuffer(e["container"], dtype=np.uint8)
        host = room.buf.cpu().numpy()
        if not np.array_equal(host, want):
            at = int(np.flatnonzero(host != want)[0]) - room.at
            raise AssertionError(f"{what}: byte {at} of the output is {int(host[at + room.at])} for {int(want[at + room.at])} "
                                 f"(the container is {e['out_size']} bytes, out_cap {room.out_cap})")
    if room.table is not None:
        want = np.full(room.table.numel(), TABLE_GUARD, dtype=np.int32)
        if e["block_sizes"] is not None:
            want[:len(e["block_sizes"])] = e["block_sizes"]
        assert np.array_equal(room.table.cpu().numpy(), want), f"{what}: d_block_sizes or its guard words"


def run(codec, case, cap_blocks, out_cap, what="", skew=0, table=True):
    """one call with this room (out_cap None: measure only), checked against joingen -> (Room, expectation)"""
    import torch
    n = len(case.items)
    room = Room(n, out_cap, cap_blocks if table and out_cap is not None else None, skew)
    torch.cuda.synchronize()
    rc = join_call(codec, on_device(case), n, room, cap_blocks)
    assert rc == 0, codec.last_error()
    torch.cuda.synchronize()
    e = case.expect(cap_blocks, out_cap if out_cap is not None else 0)
    check(case, room, e, what or case.name)
    return room, e


def decodes_to(codec, case, room, e, what):
    """tsqa_decompress_device of the joined container, and tsqa_decompress_device_sized with the join's table, give the items' data"""
    import torch
    data = np.frombuffer(case.data(), dtype=np.uint8)
    blob = room.container(e["out_size"]).clone()
    got = codec.decompress(blob)
    assert got.numel() == data.size and np.array_equal(got.cpu().numpy(), data), f"{what}: tsqa_decompress_device of the join"
    table = room.table[:len(e["block_sizes"])].clone()
    got = codec.decompress_sized(blob, table)
    assert got.numel() == data.size and np.array_equal(got.cpu().numpy(), data), f"{what}: tsqa_decompress_device_sized of the join"
    del got, blob
    torch.cuda.synchronize()


HEALTHY = None


def healthy(name):
    global HEALTHY
    if HEALTHY is None:
        HEALTHY = {c.name: c for c in jg.healthy_cases()}
    return HEALTHY[name]


HEALTHY_NAMES = ([f"tiny_{n}" for n in jg.COUNTS] + [f"tiny_257_align_{a}" for a in jg.ALIGNS] +
                 ["mix", "short_blocks", "carry_inside_a_wavefront", "carry_at_a_wavefront_edge", "twice", "tails"])


def test_every_healthy_case_is_listed():
    assert sorted(HEALTHY_NAMES) == sorted(c.name for c in jg.healthy_cases())


@pytest.mark.parametrize("name", HEALTHY_NAMES)
def test_the_join_is_the_expected_container_and_decodes_to_the_items(codec, name):
    case = healthy(name)
    size = case.expect(case.need_blocks, 1 << 62)["out_size"]
    room, e = run(codec, case, case.need_blocks, size)
    assert e["status"] == OK and len(e["container"]) == size
    decodes_to(codec, case, room, e, name)


@pytest.mark.parametrize("skew", [1, 7, 8, 15])
def test_an_output_at_any_address(codec, skew):
    """d_out need not be aligned: the words are cut at multiples of 16 of the address"""
    for name in ("tiny_513", "mix"):
        case = healthy(name)
        size = case.expect(case.need_blocks, 1 << 62)["out_size"]
        run(codec, case, case.need_blocks, size, f"{name} at skew {skew}", skew=skew)


def test_room_to_spare_changes_nothing(codec):
    case = healthy("tiny_513")
    size = case.expect(case.need_blocks, 1 << 62)["out_size"]
    run(codec, case, case.need_blocks + 1000, size + 100_001)
    run(codec, case, case.need_blocks, size, "without a table", table=False)


@pytest.mark.parametrize("name,at", jg.refusal_cases())
def test_a_refused_item_refuses_the_join_and_nothing_is_written(codec, name, at):
    case = jg.refusal(name, at)
    room, e = run(codec, case, case.need_blocks, 1 << 16)
    assert e["status"] == ERR_FORMAT and e["item_status"][at] == ERR_FORMAT and sum(e["item_status"]) == ERR_FORMAT
    _ON_DEVICE.pop(case.name)


def test_measure_only(codec):
    case = healthy("short_blocks")
    room, e = run(codec, case, case.need_blocks, None)
    assert e["status"] == ERR_OVERFLOW and e["out_size"] > 16 and e["item_status"] == [0] * 7
    # cap_blocks still bounds the walk: with one block too few the last item is not walked, and there is no size
    room, e = run(codec, case, case.need_blocks - 1, None)
    assert e["status"] == ERR_OVERFLOW and e["out_size"] == 0 and e["item_status"] == [0] * 6 + [ERR_OVERFLOW]
    assert e["first_block"][-1] == case.need_blocks
    name, at = "cut_mid_stream", 256
    bad = jg.refusal(name, at)
    room, e = run(codec, bad, bad.need_blocks, None)
    assert e["status"] == ERR_FORMAT and e["out_size"] == 0
    _ON_DEVICE.pop(bad.name)


@pytest.mark.parametrize("k", range(5))
def test_rooms_and_the_retry_with_the_reported_room(codec, k):
    what, case, cap_blocks, out_cap = jg.rooms()[k]
    room, e = run(codec, case, cap_blocks, out_cap, what)
    if e["status"] == OK:
        decodes_to(codec, case, room, e, what)
        return
    assert e["status"] == ERR_OVERFLOW and e["container"] is None
    need_blocks = int(room.first_block[-1].item())
    need = int(room.size.item())
    if need == 0:                                            # (blocks were short: the size is made once they are not)
        measured, m = run(codec, case, need_blocks, None, what + ", measured")
        need = int(measured.size.item())
    room, e = run(codec, case, need_blocks, need, what + ", the retry")
    assert e["status"] == OK and need_blocks == case.need_blocks
    decodes_to(codec, case, room, e, what)


def test_host_refusals_write_nothing(codec):
    import torch
    case = healthy("tiny_2")
    n, dev = 2, on_device(case)
    size = case.expect(2, 1 << 62)["out_size"]
    arena = dev[0]
    inside = arena.data_ptr()
    bad = [("a NULL arena", dict(arena=None)), ("NULL offsets", dict(offsets=None)), ("NULL sizes", dict(sizes=None)),
           ("a NULL size word", dict(size=None)), ("a NULL first_block", dict(first_block=None)), ("NULL item statuses", dict(item_status=None)),
           ("a NULL status word", dict(status=None)), ("no items", dict(n=0)), ("cap_blocks 0", dict(cap_blocks=0)),
           ("an output of 15 bytes", dict(out_cap=15)), ("no output but a capacity", dict(out=None, out_cap=size)),
           ("an output that starts inside the arena", dict(out=inside + 8, out_cap=size)),
           ("an output that ends inside the arena", dict(out=inside - size + 1, out_cap=size)),
           ("an output that holds the arena", dict(out=inside - 16, out_cap=arena.numel() + 32))]
    for what, over in bad:
        room = Room(n, size, 2)
        torch.cuda.synchronize()
        assert join_call(codec, dev, n, room, 2, **over) == ERR_ARG, what
        torch.cuda.synchronize()
        assert room.first_block.cpu().tolist() == [-1] * 3 and room.item_status.cpu().tolist() == [-1] * 2, what
        assert int(room.word.item()) == -1 and int(room.size.item()) == -1, what
        assert np.array_equal(room.buf.cpu().numpy(), sentinel(room.buf.numel())), what
        assert (room.table == TABLE_GUARD).all().item(), what
    room = Room(n, size, 2)
    assert codec.L.tsqa_join_async(None, arena.data_ptr(), arena.numel(), dev[1].data_ptr(), dev[2].data_ptr(), n, 2, room.out_ptr(), size,
                                   room.size.data_ptr(), room.first_block.data_ptr(), None, room.item_status.data_ptr(), room.word.data_ptr(),
                                   codec._stream()) == ERR_ARG, "a NULL context"
    # the waiting form
    out_size, blocks = C.c_size_t(7), C.c_uint32(7)
    room = Room(n, size, 2)
    args = [codec.h, arena.data_ptr(), arena.numel(), dev[1].data_ptr(), dev[2].data_ptr(), n, 2, room.out_ptr(), size, C.byref(out_size),
            C.byref(blocks), room.first_block.data_ptr(), room.table.data_ptr(), room.item_status.data_ptr(), codec._stream()]
    for k in (9, 10):
        refused = list(args)
        refused[k] = None
        assert codec.L.tsqa_join(*refused) == ERR_ARG and (out_size.value, blocks.value) == (7, 7)
    assert codec.L.tsqa_join(*args) == 0 and (out_size.value, blocks.value) == (size, 2)
    assert bytes(room.container(size).cpu().numpy()) == case.expect(2, size)["container"]
    args[8] = size - 1
    assert codec.L.tsqa_join(*args) == ERR_OVERFLOW and (out_size.value, blocks.value) == (size, 2)


def _texts(tsq, n, seed):
    rng = np.random.default_rng(seed)
    return [tsq.synth.text(int(rng.integers(1, 20_000)), seed=seed + k) for k in range(n)]


@pytest.mark.parametrize("variant", [0, 6, 7])
def test_compress_join_decompress_on_one_stream_with_no_host_read(codec, tsq, variant):
    """compress_batch_packed_async -> join_async -> decompress_sized_async, twice back to back with more items the second time (the
    scratch grows between them), nothing read on the host until both have been enqueued; then an index of the join and a range read
    across an item seam"""
    import torch
    codec.set_variant(variant, 0)
    stream = torch.cuda.Stream()
    runs = []
    for n, seed in ((40, 100), (700, 300)):
        datas = _texts(tsq, n, seed)
        at = np.concatenate([[0], np.cumsum([d.size for d in datas])]).astype(np.int64)
        runs.append(dict(n=n, datas=datas, plain=np.concatenate(datas), items=[(int(at[k]), int(datas[k].size)) for k in range(n)],
                         room=sum(tsq.batch_bound(d.size) + 15 for d in datas)))
    for r in runs:
        r["src"] = to_dev(r["plain"])
        r["arena"] = to_dev(sentinel(r["room"]))
        r["joined"] = to_dev(sentinel(r["room"]))
        r["back"] = to_dev(sentinel(r["plain"].size + FENCE))
        r["offsets"] = torch.full((r["n"] + 1,), -1, dtype=torch.int64, device="cuda")
        r["sizes"] = torch.full((r["n"],), -1, dtype=torch.int64, device="cuda")
        r["first"] = torch.full((r["n"] + 1,), -1, dtype=torch.int64, device="cuda")
        r["status"] = torch.full((r["n"],), -1, dtype=torch.int32, device="cuda")
        r["table"] = torch.full((r["n"],), TABLE_GUARD, dtype=torch.int32, device="cuda")
        r["words"] = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        for r in runs:
            n = r["n"]
            codec.compress_batch_packed_async(r["src"], r["items"], n & 1, 16, r["arena"], r["offsets"], r["sizes"])
            codec.join_async(r["arena"], r["offsets"], r["sizes"], n, n, r["joined"], r["first"], r["table"], r["status"])
            r["words"][0:1].copy_(codec._size)               # (device to device, on the stream: the join's size and status)
            r["words"][1:2].copy_(codec._status)
            codec.decompress_sized_async(r["joined"], n, r["table"], r["back"][:r["plain"].size])
            r["words"][2:3].copy_(codec._size)
            r["words"][3:4].copy_(codec._status)
    stream.synchronize()
    for r in runs:
        n = r["n"]
        join_size, join_status, size, status = r["words"].cpu().tolist()
        assert (join_status, status) == (0, 0) and size == r["plain"].size
        assert r["status"].cpu().tolist() == [0] * n and r["first"].cpu().tolist() == list(range(n + 1))
        back = r["back"].cpu().numpy()
        assert np.array_equal(back[:size], r["plain"]) and np.array_equal(back[size:], sentinel(back.size)[size:])
        arena, offs, sizes = r["arena"].cpu().numpy(), r["offsets"].cpu().tolist(), r["sizes"].cpu().tolist()
        want, want_sizes = jg.joined([arena[o:o + z].tobytes() for o, z in zip(offs, sizes)])
        assert join_size == len(want) and bytes(r["joined"][:join_size].cpu().numpy()) == want
        assert np.array_equal(r["joined"][join_size:].cpu().numpy(), sentinel(r["room"])[join_size:])
        assert r["table"].cpu().tolist() == want_sizes
    r = runs[1]
    with torch.cuda.stream(stream):
        idx = codec.index(r["joined"][:int(r["words"][0].item())])
        seam = r["items"][350][0]                            # where item 350's data starts
        got = idx.read(seam - 100, 300)
        stream.synchronize()
        assert np.array_equal(got.cpu().numpy(), r["plain"][seam - 100:seam + 200])
        idx.close()


def test_python_join_of_a_packed_batch_and_of_separate_tensors(codec, tsq):
    import torch
    datas = _texts(tsq, 9, 900) + [tsq.synth.text(jg.BLOCK + 77, seed=5)]
    plain = np.concatenate(datas)
    srcs = [to_dev(d) for d in datas]
    batch = codec.compress_batch_packed(srcs, 1, align=16)
    blob, table = batch.join(block_sizes=True)
    want, want_sizes = jg.joined([bytes(v.cpu().numpy()) for v in batch.views])
    assert bytes(blob.cpu().numpy()) == want and table.cpu().tolist() == want_sizes and table.numel() == 11
    assert np.array_equal(codec.decompress(blob).cpu().numpy(), plain)
    assert np.array_equal(codec.decompress_sized(blob, table).cpu().numpy(), plain)
    # separate allocations, an append: join([old, new])
    old = codec.compress(srcs[0], 0).clone()
    new = codec.compress(srcs[9], 1).clone()
    both = codec.join([old, new])
    assert bytes(both.cpu().numpy()) == jg.joined([bytes(old.cpu().numpy()), bytes(new.cpu().numpy())])[0]
    assert np.array_equal(codec.decompress(both).cpu().numpy(), np.concatenate([datas[0], datas[9]]))
    # an `out` that is too small: the bytes a retry needs
    with pytest.raises(tsq.TsqError) as err:
        codec.join([old, new], out=torch.empty(both.numel() - 1, dtype=torch.uint8, device="cuda"))
    assert err.value.code == ERR_OVERFLOW and err.value.needed == both.numel() and err.value.item_status == [0, 0]
    out = torch.empty(err.value.needed, dtype=torch.uint8, device="cuda")
    assert torch.equal(codec.join([old, new], out=out), both) and out.data_ptr() == codec.join([old, new], out=out).data_ptr()
    # a damaged item: all or nothing, and the verdict per item
    cut = new[:new.numel() // 2].clone()
    out = to_dev(sentinel(both.numel()))
    with pytest.raises(tsq.TsqError) as err:
        codec.join([old, cut, old], out=out)
    assert err.value.code == ERR_FORMAT and err.value.item_status == [0, ERR_FORMAT, 0]
    assert np.array_equal(out.cpu().numpy(), sentinel(both.numel()))
