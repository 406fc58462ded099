"""GPU tests of the dense decompress of a packed batch (tsqa_decompress_batch_packed_dense_async): block counts and output places made
on the device from the containers' headers.  The batches are those of tests/densegen.py (test_dense_cpu.py shows that each reaches
its aim); every call goes through the C ABI.  The output lies between two guards of 4 KiB in a buffer filled with a pattern, and the
whole buffer is compared with one image: the pattern, overlaid with the data of the items that must be delivered.  Only the range of
a fitting item that a block decoder refuses is left out (its contents are undefined); padding, the ranges of items refused at the
header or by the walk, of items that do not fit, and both guards must still hold the pattern."""
import ctypes as C

import numpy as np
import pytest

import chaingen as cg
import densegen as dg
from turbosqueeze_amd.api import PackedBatch, _batch_array

pytestmark = pytest.mark.gpu

GUARD = 4096
OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW = dg.OK, dg.ERR_ARG, dg.ERR_FORMAT, dg.ERR_STREAM, dg.ERR_OVERFLOW


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


def to_dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


class OnDevice:
    """a batch's arena and place tables in device memory"""

    def __init__(self, b):
        self.b, self.n = b, len(b.items)
        self.arena, self.offsets, self.sizes = to_dev(b.arena), to_dev(b.offsets, np.int64), to_dev(b.sizes, np.int64)


_ON_DEVICE = {}


def on_device(b) -> OnDevice:
    if b.name not in _ON_DEVICE:
        _ON_DEVICE[b.name] = OnDevice(b)
    return _ON_DEVICE[b.name]


class Tables:
    """the call's outputs, filled with -1, and a fenced output buffer (None: measure only)"""

    def __init__(self, n, out_size=None):
        import torch
        i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device="cuda")
        self.out_offsets, self.out_sizes, self.first_block = i64(n + 1), i64(n), i64(n + 1)
        self.item_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.word = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.out_size = out_size
        self.buf = to_dev(sentinel(out_size + 2 * GUARD)) if out_size is not None else None

    def out_ptr(self):
        return self.buf.data_ptr() + GUARD if self.buf is not None else None

    def host(self):
        return (self.out_offsets.cpu().tolist(), self.first_block.cpu().tolist(), self.item_status.cpu().tolist(), self.out_sizes.cpu().tolist())


def dense_call(codec, d, t, cap_blocks, align=None, **over):
    """tsqa_decompress_batch_packed_dense_async on the current stream -> its return value.  over: arguments replaced."""
    a = dict(arena=d.arena.data_ptr(), arena_size=d.arena.numel(), offsets=d.offsets.data_ptr(), sizes=d.sizes.data_ptr(), n=d.n,
             align=d.b.align if align is None else align, cap_blocks=cap_blocks, out=t.out_ptr(), out_size=t.out_size or 0,
             out_offsets=t.out_offsets.data_ptr(), out_sizes=t.out_sizes.data_ptr(), first_block=t.first_block.data_ptr(),
             item_status=t.item_status.data_ptr(), status=t.word.data_ptr())
    a.update(over)
    return codec.L.tsqa_decompress_batch_packed_dense_async(codec.h, a["arena"], a["arena_size"], a["offsets"], a["sizes"], a["n"], a["align"],
                                                            a["cap_blocks"], a["out"], a["out_size"], a["out_offsets"], a["out_sizes"],
                                                            a["first_block"], a["item_status"], a["status"], codec._stream())


def image(b, offsets, status, out_size):
    """-> (the bytes the fenced buffer must hold, which of them count)"""
    expect = sentinel(out_size + 2 * GUARD)
    defined = np.ones(expect.size, dtype=bool)
    for it, o, nb, t, st in zip(b.items, offsets, b.blocks, b.totals, status):
        if st == OK:
            expect[GUARD + o:GUARD + o + t] = np.frombuffer(it.want, dtype=np.uint8)
        elif st == ERR_STREAM:
            defined[GUARD + o:GUARD + o + t] = False
    return expect, defined


def same_image(host, expect, defined, b, offsets, what):
    same = (host == expect) | ~defined
    if same.all():
        return
    at = int(np.flatnonzero(~same)[0]) - GUARD
    k = max((j for j, o in enumerate(offsets[:-1]) if o <= at), default=-1)
    raise AssertionError(f"{what}: byte {at} of the output is {int(host[at + GUARD])} for {int(expect[at + GUARD])} "
                         f"(item {k}, {b.items[k].name if k >= 0 else 'the front guard'}, which starts at {offsets[k] if k >= 0 else 0})")


def run(codec, tsq, b, out_size, cap_blocks, what=""):
    """one dense call with this room, checked against tsqa_plan_dense, the restatement and the oracle -> (Tables, statuses)"""
    import torch
    what = what or b.name
    d = on_device(b)
    t = Tables(d.n, out_size)
    torch.cuda.synchronize()
    rc = dense_call(codec, d, t, cap_blocks)
    assert rc == 0, codec.last_error()
    torch.cuda.synchronize()
    offsets, first, status, sizes = b.expect(out_size, cap_blocks)
    got = t.host()
    planned = tsq.plan_dense(b.totals, b.blocks, b.align, out_size, cap_blocks)
    assert planned[:2] == (offsets, first)
    assert got[0] == offsets, f"{what}: d_out_offsets"
    assert got[1] == first, f"{what}: d_first_block"
    assert got[2] == status, f"{what}: item statuses {[(k, g, w) for k, (g, w) in enumerate(zip(got[2], status)) if g != w][:8]} (item, got, owed)"
    assert got[3] == sizes, f"{what}: d_out_sizes"
    assert int(t.word.item()) == max(status), f"{what}: *d_status"
    expect, defined = image(b, offsets, status, out_size)
    same_image(t.buf.cpu().numpy(), expect, defined, b, offsets, what)
    return t, status


BATCHES = None


def batch_by_name(name):
    global BATCHES
    if BATCHES is None:
        BATCHES = {b.name: b for b in dg.every_batch()}
    return BATCHES[name]


BATCH_NAMES = ([f"carry_totals_{k}" for k in dg.CARRY_BIG_AT] + [f"loop_edges_{n}" for n in dg.LOOP_COUNTS] + ["two_blocks"] +
               [f"alignment_{a}" for a in dg.ALIGNS] + ["refusals", "cuts"])


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_tables_bytes_and_fence_with_exactly_the_room_needed(codec, tsq, name):
    b = batch_by_name(name)
    _, status = run(codec, tsq, b, b.need_bytes, b.need_blocks)
    assert status == [it.fault if nb else ERR_FORMAT for it, nb in zip(b.items, b.blocks)]
    assert any(s == OK for s in status)


def test_every_batch_is_listed():
    assert sorted(BATCH_NAMES) == sorted(b.name for b in dg.every_batch())


def test_refusals_cost_only_themselves(codec, tsq):
    b = dg.refusals()
    _, status = run(codec, tsq, b, b.need_bytes, b.need_blocks)
    assert [s for s in status if s] == [ERR_FORMAT] * 8 + [ERR_STREAM] and status[0::2] == [OK] * (len(status) // 2 + 1)


@pytest.mark.parametrize("k", range(7))
def test_cuts_deliver_the_fitting_prefix(codec, tsq, k):
    b, table = dg.cuts()
    what, out_size, cap_blocks, n_fit = table[k]
    t, status = run(codec, tsq, b, out_size, cap_blocks, what)
    assert [s == OK for i, s in enumerate(status) if i != 7] == [i < n_fit for i in range(12) if i != 7], what
    # the tables of any cut are those a retry needs
    assert int(t.out_offsets[-1].item()) == b.need_bytes and int(t.first_block[-1].item()) == b.need_blocks


@pytest.mark.parametrize("name", ["two_blocks", "refusals", "alignment_4096", "loop_edges_257", "carry_totals_across_a_wavefront_edge"])
def test_differential_against_the_per_item_call(codec, tsq, name):
    """the same arena through tsqa_decompress_batch_packed_items_async, its host items built from the dense call's own tables (an
    item refused at its header has no blocks there; the planner wants a count of at least 1 and gets 1: it is refused again)"""
    import torch
    b = batch_by_name(name)
    d = on_device(b)
    t, status = run(codec, tsq, b, b.need_bytes, b.need_blocks)
    offsets, first = t.out_offsets.cpu().tolist(), t.first_block.cpu().tolist()
    quads = [(0, 0, offsets[i], offsets[i + 1] - offsets[i]) for i in range(d.n)]
    blocks = np.array([max(first[i + 1] - first[i], 1) for i in range(d.n)], dtype=np.uint32)
    u = Tables(d.n, b.need_bytes)
    torch.cuda.synchronize()
    rc = codec.L.tsqa_decompress_batch_packed_items_async(codec.h, d.arena.data_ptr(), d.arena.numel(), d.offsets.data_ptr(), d.sizes.data_ptr(),
                                                          _batch_array(quads), blocks.ctypes.data, d.n, u.out_ptr(), b.need_bytes,
                                                          u.out_sizes.data_ptr(), u.item_status.data_ptr(), u.word.data_ptr(), codec._stream())
    assert rc == 0, codec.last_error()
    torch.cuda.synchronize()
    assert u.item_status.cpu().tolist() == status and torch.equal(u.out_sizes, t.out_sizes) and int(u.word.item()) == int(t.word.item())
    _, defined = image(b, offsets, status, b.need_bytes)
    same_image(u.buf.cpu().numpy(), t.buf.cpu().numpy(), defined, b, offsets, f"{name}: the per-item call against the dense call")


@pytest.mark.parametrize("name", ["refusals", "two_blocks", "loop_edges_513"])
def test_measure_only_then_a_retry_with_the_reported_room(codec, tsq, name):
    import torch
    b = batch_by_name(name)
    d = on_device(b)
    t = Tables(d.n)
    before = d.arena.clone()
    torch.cuda.synchronize()
    assert dense_call(codec, d, t, 0) == 0, codec.last_error()
    torch.cuda.synchronize()
    offsets, first, status, sizes = b.expect(0, 0)
    assert t.host() == (offsets, first, status, sizes) and set(status) <= {ERR_FORMAT, ERR_OVERFLOW} and not any(sizes)
    assert int(t.word.item()) == max(status) == ERR_OVERFLOW and torch.equal(before, d.arena)
    # a cap_blocks that nobody looks at changes nothing
    t2 = Tables(d.n)
    torch.cuda.synchronize()
    assert dense_call(codec, d, t2, 1000) == 0
    torch.cuda.synchronize()
    assert t2.host() == t.host()
    _, status = run(codec, tsq, b, offsets[-1], first[-1], f"{name}: the retry")
    assert [s for s, it in zip(status, b.items) if it.want is not None] == [OK] * sum(it.want is not None for it in b.items)


def _sources(n_items, seed, big_at=None):
    """source items for the chain: text of 1 B to 4 KiB, one of 4 MiB + 1 B at big_at -> (arena, (in_at, in_len) items)"""
    from turbosqueeze_amd import synth
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(1, 4097, n_items)]
    if big_at is not None:
        lens[big_at] = dg.BLOCK + 1
    src = synth.text(sum(lens), seed=seed)
    ats = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    return src, list(zip(ats, lens))


def test_chain_behind_the_packed_compress_on_one_stream(codec, tsq):
    """compress_batch_packed_async, then the dense call, nothing waited for between them, twice back to back: the first shape under
    reserve_batch's first size, the second above it, so the context's item table grows between the calls.  The room is what the
    producer knows: the source lengths."""
    import torch
    side = torch.cuda.Stream()
    fresh = tsq.DeviceCodec(0)                            # (a context whose scratch has not grown yet)
    shapes = [_sources(40, 71, big_at=17), _sources(cg.FIRST_BATCH_ITEMS + 44, 72)]
    assert len(shapes[0][1]) < cg.FIRST_BATCH_ITEMS < len(shapes[1][1])
    runs = []
    try:
        with torch.cuda.stream(side):
            for src, items in shapes:
                n, lens = len(items), [ln for _, ln in items]
                offsets, first, _ = tsq.plan_dense(lens, [-(-ln // dg.BLOCK) for ln in lens], 16)
                d_src = to_dev(src)
                packed = torch.empty(sum(tsq.batch_bound(ln) + 15 for ln in lens), dtype=torch.uint8, device="cuda")
                d_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
                d_sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
                t = Tables(n, offsets[-1])
                fresh.compress_batch_packed_async(d_src, items, 1, 16, packed, d_offsets, d_sizes)
                rc = fresh.L.tsqa_decompress_batch_packed_dense_async(fresh.h, packed.data_ptr(), packed.numel(), d_offsets.data_ptr(),
                                                                      d_sizes.data_ptr(), n, 16, first[-1], t.out_ptr(), offsets[-1],
                                                                      t.out_offsets.data_ptr(), t.out_sizes.data_ptr(), t.first_block.data_ptr(),
                                                                      t.item_status.data_ptr(), t.word.data_ptr(), fresh._stream())
                assert rc == 0, fresh.last_error()
                runs.append((src, items, offsets, first, packed, d_offsets, d_sizes, t))
        side.synchronize()
        for src, items, offsets, first, packed, d_offsets, d_sizes, t in runs:
            lens = [ln for _, ln in items]
            assert t.host() == (offsets, first, [OK] * len(items), lens) and int(t.word.item()) == OK
            expect = sentinel(offsets[-1] + 2 * GUARD)
            for (a, ln), o in zip(items, offsets):
                expect[GUARD + o:GUARD + o + ln] = src[a:a + ln]
            assert np.array_equal(t.buf.cpu().numpy(), expect)
        # the Python round trip from the device tables alone
        src, items, offsets, first, packed, d_offsets, d_sizes, _ = runs[0]
        pb = PackedBatch.from_device(fresh, packed, d_offsets, d_sizes)
        assert pb.lengths == [ln for _, ln in items] and pb.offsets == d_offsets.cpu().tolist()
        for v, (a, ln) in zip(pb.decompress(), items):
            assert np.array_equal(v.cpu().numpy(), src[a:a + ln])
        views = fresh.decompress_packed(packed, d_offsets[:-1], d_sizes, align=64)
        assert all(v.data_ptr() % 64 == views[0].data_ptr() % 64 for v in views)
        for v, (a, ln) in zip(views, items):
            assert np.array_equal(v.cpu().numpy(), src[a:a + ln])
    finally:
        fresh.close()


def test_python_decompress_packed_reports_item_statuses(codec, tsq):
    b = dg.refusals()
    d = on_device(b)
    views, status = codec.decompress_packed(d.arena, d.offsets, d.sizes, item_status=True)
    assert status == b.expect(b.need_bytes, b.need_blocks)[2]
    for it, v, st in zip(b.items, views, status):
        assert (v is None) == (st != OK)
        if v is not None:
            assert v.cpu().numpy().tobytes() == it.want, it.name
    with pytest.raises(tsq.TsqError) as e:
        codec.decompress_packed(d.arena, d.offsets, d.sizes)
    assert e.value.item_status == status and e.value.code == ERR_STREAM
    import torch
    small = torch.empty(b.need_bytes - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(tsq.TsqError) as e:
        codec.decompress_packed(d.arena, d.offsets, d.sizes, out=small)
    assert e.value.code == ERR_OVERFLOW and e.value.needed == b.need_bytes


def test_refused_arguments_write_nothing(codec):
    import torch
    b = dg.two_blocks()
    d = on_device(b)
    t = Tables(d.n, b.need_bytes)
    torch.cuda.synchronize()
    call = lambda **over: dense_call(codec, d, t, over.pop("cap_blocks", b.need_blocks), **over)
    for name in ("arena", "offsets", "sizes", "out_offsets", "out_sizes", "first_block", "item_status", "status"):
        assert call(**{name: None}) == ERR_ARG, name
        assert "null pointer" in codec.last_error()
    assert call(n=0) == ERR_ARG
    for align in (0, 3, 24, 8192):
        assert call(align=align) == ERR_ARG, align
    assert call(cap_blocks=0) == ERR_ARG                      # an output and no blocks
    assert call(out_size=0) == ERR_ARG                        # an output of no bytes
    assert call(out=None) == ERR_ARG                          # measuring takes out_size 0
    assert codec.L.tsqa_decompress_batch_packed_dense_async(None, d.arena.data_ptr(), d.arena.numel(), d.offsets.data_ptr(), d.sizes.data_ptr(),
                                                            d.n, 16, b.need_blocks, t.out_ptr(), b.need_bytes, t.out_offsets.data_ptr(),
                                                            t.out_sizes.data_ptr(), t.first_block.data_ptr(), t.item_status.data_ptr(),
                                                            t.word.data_ptr(), codec._stream()) == ERR_ARG      # no context
    torch.cuda.synchronize()
    assert np.array_equal(t.buf.cpu().numpy(), sentinel(b.need_bytes + 2 * GUARD))
    assert t.host() == ([-1] * (d.n + 1), [-1] * (d.n + 1), [-1] * d.n, [-1] * d.n) and int(t.word.item()) == -1
