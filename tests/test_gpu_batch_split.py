"""GPU tests of the packed batch compress of short blocks (tsqa_compress_batch_packed_split*, tsqa_compress_batch_packed_tables_split_async):
batchsplitgen's batches through both asynchronous forms and the waiting form.  The arena, both tables, the table of stream lengths and
the verdicts are the expectation's, made with the oracle; every buffer the library writes is filled with a pattern first and must keep
it wherever the call owes nothing (padding, the room past a cut, the words past the live blocks).  Every healthy arena goes back
through the dense decompress and, item by item, through the sized decompress with the item's slice of the table."""
import ctypes as C

import numpy as np
import pytest

import batchsplitgen as bg
import packedgen as pg
import tablegen as tg

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_OVERFLOW = bg.OK, bg.ERR_ARG, bg.ERR_OVERFLOW
FENCE = 4096
TABLE_GUARD = 0x5EA1ED
WORD_GUARD = 0x0123456789ABCDE


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
def budget():
    """B: the blocks of one encode launch, 2 x CUs"""
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream()


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (the pattern repeats every 251 bytes)"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


def words(n, dtype=np.int64):
    return to_dev(np.full(n, WORD_GUARD if dtype == np.int64 else TABLE_GUARD, dtype=dtype))


_on_device = {}


def dev(b):
    """the batch's input and its two tables on the device, made once"""
    if b.name not in _on_device:
        _on_device[b.name] = (to_dev(b.data), to_dev(np.array(b.in_offsets, dtype=np.uint64).view(np.int64)),
                              to_dev(np.array(b.in_sizes, dtype=np.uint64).view(np.int64)))
    return _on_device[b.name]


def host_items(tsq, b):
    return tsq.api._batch_array([(a, n, 0, 0) for a, n in b.places])


def run_host(codec, tsq, side, b, ext, room, form):
    """one of the two host forms into the first `room` bytes of a pattern-filled buffer -> dict of everything it wrote"""
    import torch
    d_in = dev(b)[0]
    n, nb = len(b.specs), b.need_blocks
    guard = sentinel(room + FENCE)
    out, table = to_dev(guard), words(nb + 16, np.int32)
    if form == "wait":
        offsets, sizes = (C.c_uint64 * (n + 1))(), (C.c_uint64 * n)()
        rc = codec.L.tsqa_compress_batch_packed_split(codec.h, d_in.data_ptr(), d_in.numel(), host_items(tsq, b), n, ext, b.align, b.block_len,
                                                      out.data_ptr(), room, offsets, sizes, table.data_ptr(), codec._stream())
        word = rc
        offsets, sizes = [int(x) for x in offsets], [int(x) for x in sizes]
    else:
        d_offsets, d_sizes, d_status = words(n + 1), words(n), words(1, np.int32)
        with torch.cuda.stream(side):
            rc = codec.L.tsqa_compress_batch_packed_split_async(codec.h, d_in.data_ptr(), d_in.numel(), host_items(tsq, b), n, ext, b.align,
                                                                b.block_len, out.data_ptr(), room, d_offsets.data_ptr(), d_sizes.data_ptr(),
                                                                table.data_ptr(), d_status.data_ptr(), codec._stream())
        assert rc == OK, codec.last_error()
        side.synchronize()
        offsets, sizes, word = d_offsets.cpu().tolist(), d_sizes.cpu().tolist(), int(d_status.item())
    return dict(arena=out.cpu().numpy(), guard=guard, offsets=offsets, sizes=sizes, table=table.cpu().numpy(), word=word, d_out=out,
                d_table=table)


def run_tables(codec, side, b, ext, cap, room, measuring=False):
    """the device-tables form -> dict of everything it wrote"""
    import torch
    d_in, d_at, d_sz = dev(b)
    n = len(b.specs)
    guard = sentinel(room + FENCE)
    out, table = to_dev(guard), words(cap + 16, np.int32)
    d_offsets, d_sizes, d_first, d_bound = words(n + 1), words(n), words(n + 1), words(1)
    d_item, d_status = words(n, np.int32), words(1, np.int32)
    with torch.cuda.stream(side):
        rc = codec.L.tsqa_compress_batch_packed_tables_split_async(codec.h, d_in.data_ptr(), d_in.numel(), d_at.data_ptr(), d_sz.data_ptr(), n,
                                                                   cap, ext, b.align, b.block_len, None if measuring else out.data_ptr(),
                                                                   0 if measuring else room, d_offsets.data_ptr(), d_sizes.data_ptr(),
                                                                   d_first.data_ptr(), d_bound.data_ptr(), table.data_ptr(), d_item.data_ptr(),
                                                                   d_status.data_ptr(), codec._stream())
    assert rc == OK, codec.last_error()
    side.synchronize()
    return dict(arena=out.cpu().numpy(), guard=guard, offsets=d_offsets.cpu().tolist(), sizes=d_sizes.cpu().tolist(),
                table=table.cpu().numpy(), word=int(d_status.item()), first_block=d_first.cpu().tolist(), bound=int(d_bound.item()),
                status=d_item.cpu().tolist(), d_out=out, d_table=table, d_offsets=d_offsets, d_sizes=d_sizes)


def compare(b, oracle, ext, got, e, what):
    assert got["offsets"] == e["offsets"], f"{b.name}, {what}: d_offsets"
    assert got["sizes"] == e["sizes"], f"{b.name}, {what}: d_sizes"
    live = len(e["block_sizes"])
    assert got["table"][:live].tolist() == e["block_sizes"], f"{b.name}, {what}: d_block_sizes"
    assert (got["table"][live:] == TABLE_GUARD).all(), f"{b.name}, {what}: words past the live blocks were written"
    assert got["word"] == e["word"], f"{b.name}, {what}: the status word"
    want = b.image(oracle, ext, e, got["guard"])
    if not np.array_equal(got["arena"], want):
        at = int(np.flatnonzero(got["arena"] != want)[0])
        item = max(i for i, o in enumerate(e["offsets"][:-1]) if o <= at) if at >= 0 else -1
        raise AssertionError(f"{b.name}, {what}: the arena differs first at byte {at} (item {item} starts at {e['offsets'][item]})")
    if "status" in got:
        assert got["status"] == e["status"], f"{b.name}, {what}: the item statuses"
        assert got["first_block"] == e["first_block"] and got["bound"] == e["bound"], f"{b.name}, {what}: first_block, bound"


def round_trips(codec, b, got, e):
    """the arena through the dense decompress, and every item through the sized decompress with its slice of the table"""
    used = e["offsets"][-1]
    d_offsets, d_sizes = to_dev(np.array(e["offsets"], dtype=np.int64)), to_dev(np.array(e["sizes"], dtype=np.int64))
    views, status = codec.decompress_packed(got["d_out"][:used], d_offsets, d_sizes, align=1, item_status=True)
    at = 0
    for i, nb in enumerate(b.blocks):
        if not nb:
            assert views[i] is None
            continue
        assert status[i] == OK and views[i].cpu().numpy().tobytes() == b.item(i).tobytes(), f"{b.name}: item {i} through decompress_packed"
        blob = got["d_out"][e["offsets"][i]:e["offsets"][i] + e["sizes"][i]]
        back = codec.decompress_sized(blob, got["d_table"][at:at + nb])
        assert back.cpu().numpy().tobytes() == b.item(i).tobytes(), f"{b.name}: item {i} through decompress_sized"
        at += nb


def check(codec, tsq, oracle, side, b, ext, out_size=None, cap_blocks=None, back=True):
    """the batch through every form it can take; out_size None: exactly the room the arena needs"""
    if b.host_form and cap_blocks is None:
        e = b.expect(oracle, ext, out_size=out_size, per_item=False)
        room = max(e["offsets"][-1], 16) if out_size is None else out_size
        for form in ("async", "wait"):
            compare(b, oracle, ext, run_host(codec, tsq, side, b, ext, room, form), e, f"the {form} form, ext {ext}, room {room}")
    cap = b.need_blocks if cap_blocks is None else cap_blocks
    e = b.expect(oracle, ext, cap_blocks=cap, out_size=out_size, per_item=True)
    room = max(e["offsets"][-1], 16) if out_size is None else out_size
    got = run_tables(codec, side, b, ext, cap, room)
    compare(b, oracle, ext, got, e, f"the tables form, ext {ext}, room {room}, cap_blocks {cap}")
    if back and out_size is None and cap_blocks is None:
        round_trips(codec, b, got, e)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 6, 7])
@pytest.mark.parametrize("ext", [0, 1])
def test_edge_items(codec, tsq, oracle, side, ext, variant):
    """items of 1, 4095, 4096, 4097 and 2 x 4096 + 1 bytes of text, random bytes and zeros"""
    codec.set_variant(variant, 0)
    check(codec, tsq, oracle, side, bg.edge_items(), ext)


@pytest.mark.parametrize("ext", [0, 1])
def test_item_counts(codec, tsq, oracle, side, ext):
    """1, 255, 256, 257 and 513 one-block items: the item passes of the scan"""
    for b in bg.item_counts():
        check(codec, tsq, oracle, side, b, ext)


def test_launch_ownership_and_edges(codec, tsq, oracle, side, budget):
    """one item that owns a whole launch, and two, alone and between one-block items; an item that starts on a launch's last block;
    one that ends on a launch's first block"""
    for b in bg.ownership(budget):
        check(codec, tsq, oracle, side, b, 1)
    check(codec, tsq, oracle, side, bg.ownership(budget)[-1], 0)


@pytest.mark.parametrize("ext", [0, 1])
def test_scan_crosses_2_to_24_inside_a_launch_and_an_item(codec, tsq, oracle, side, budget, ext):
    b = bg.crossing_alone()
    assert bg.scan_crossings(b.made(oracle, ext)[0][1], budget), "the case does not reach its aim on this device"
    check(codec, tsq, oracle, side, b, ext)


def test_scan_crossing_at_a_wavefronts_first_lane(codec, tsq, oracle, side, budget):
    b, (block, lane) = bg.crossing_fronted(oracle, budget)
    assert lane % bg.WAVE == 0 and lane != 0
    check(codec, tsq, oracle, side, b, 1)


@pytest.mark.parametrize("variant", [0, 6, 7])
@pytest.mark.parametrize("ext", [0, 1])
def test_lookahead_ends_with_the_item(codec, tsq, oracle, side, ext, variant):
    codec.set_variant(variant, 0)
    check(codec, tsq, oracle, side, bg.lookahead()[0], ext)


@pytest.mark.parametrize("align", bg.ALIGNS)
def test_aligns(codec, tsq, oracle, side, align):
    check(codec, tsq, oracle, side, bg.align_mix(align), 1)


@pytest.mark.parametrize("ext", [0, 1])
def test_room(codec, tsq, oracle, side, ext):
    """exact; one byte short; ending inside a header, inside a frame word and inside a middle item: the tables are complete, every
    item that lies wholly inside the room is exact, nothing at or past the room is written, and a retry with offsets[n] bytes succeeds"""
    b, cuts = bg.room_cuts(oracle, ext)
    for what, room in cuts:
        check(codec, tsq, oracle, side, b, ext, out_size=room)
    short = run_host(codec, tsq, side, b, ext, dict(cuts)["inside a middle item"], "wait")
    assert short["word"] == ERR_OVERFLOW
    again = run_host(codec, tsq, side, b, ext, short["offsets"][-1], "wait")
    assert again["word"] == OK
    compare(b, oracle, ext, again, b.expect(oracle, ext, per_item=False), "the retry")


def test_full_size_blocks_are_the_packed_call(codec, tsq, side):
    """block_len = 2^22: the arena and both tables of tsqa_compress_batch_packed_async, byte for byte"""
    import torch
    rng = np.random.default_rng(21)
    sizes = [1, 2, 15, 16, 17, 699, 4096, 65535, (1 << 22) + 1]
    datas = [tsq.synth.text(n, seed=n) if k % 2 else tsq.synth.mix(n, seed=n) for k, n in enumerate(sizes)]
    datas += [pg.small_item(rng, k, int(rng.integers(1, 20_000))) for k in range(30)]
    d_in = to_dev(np.concatenate(datas))
    items, at = [], 0
    for d in datas:
        items.append((at, d.size))
        at += d.size
    first, bound = tsq.plan_batch_split(items, at, 1 << 22, 16)
    assert first[-1] == len(datas) + 1
    for ext in (0, 1):
        outs = []
        for split in (False, True):
            out = to_dev(sentinel(bound + FENCE))
            d_offsets, d_sizes = words(len(items) + 1), words(len(items))
            with torch.cuda.stream(side):
                if split:
                    table = words(first[-1], np.int32)
                    codec.compress_batch_packed_split_async(d_in, items, ext, 16, 1 << 22, out, d_offsets, d_sizes, table)
                else:
                    codec.compress_batch_packed_async(d_in, items, ext, 16, out, d_offsets, d_sizes)
            side.synchronize()
            assert codec._status.item() == OK
            outs.append((out.cpu().numpy(), d_offsets.cpu().tolist(), d_sizes.cpu().tolist()))
        assert outs[0][1:] == outs[1][1:] and np.array_equal(outs[0][0], outs[1][0])
        offs, szs = outs[1][1], outs[1][2]
        want = []
        for i in range(len(items)):                          # (the frame words of the containers are the table)
            ends = tg.pieces(outs[1][0][offs[i]:offs[i] + szs[i]].tobytes())
            want += [ends[k + 1] - ends[k] - 3 for k in range(len(ends) - 1)]
        assert table.cpu().tolist() == want


# ---- the tables form ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", [0, 1])
def test_refused_places(codec, tsq, oracle, side, budget, ext):
    """every refused place as item 0, as item 256, directly behind the item that ends a launch, and as the last item"""
    check(codec, tsq, oracle, side, bg.refusals(budget), ext)


def test_cap_blocks(codec, tsq, oracle, side, budget):
    """exact, one short, cutting inside an item, and loose enough for a dead launch: no word of the table past the live blocks"""
    b, cuts = bg.cap_cuts(budget)
    for what, cap, n_fit in cuts:
        check(codec, tsq, oracle, side, b, 1, cap_blocks=cap)


def test_measure_only(codec, oracle, side, budget):
    for b in (bg.refusals(budget), bg.cap_batch(), bg.overlaps()):
        got = run_tables(codec, side, b, 1, 0, 16, measuring=True)
        e = b.expect(oracle, 1, measuring=True)
        compare(b, oracle, 1, got, e, "measuring")
        assert got["first_block"][-1] == b.need_blocks


@pytest.mark.parametrize("ext", [0, 1])
def test_overlapping_input_ranges(codec, tsq, oracle, side, ext):
    check(codec, tsq, oracle, side, bg.overlaps(), ext)


# ---- refusals of the calls ---------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_anything_is_written(codec, tsq, side):
    b = bg.room_batch()
    d_in, d_at, d_sz = dev(b)
    n = len(b.specs)
    L, h, s = codec.L, codec.h, codec._stream()
    guard = sentinel(1 << 16)
    out = to_dev(guard)
    d_offsets, d_sizes, d_first, d_bound = words(n + 1), words(n), words(n + 1), words(1)
    table, d_item, d_status = words(64, np.int32), words(n, np.int32), words(1, np.int32)
    items = host_items(tsq, b)
    offsets, sizes = (C.c_uint64 * (n + 1))(), (C.c_uint64 * n)()

    def host_async(block_len=4096, d_in_=d_in.data_ptr(), out_=out.data_ptr(), off_=d_offsets.data_ptr(), sz_=d_sizes.data_ptr(),
                   st_=d_status.data_ptr(), items_=items, align=16, n_=n):
        return L.tsqa_compress_batch_packed_split_async(h, d_in_, d_in.numel(), items_, n_, 1, align, block_len, out_, 1 << 16, off_, sz_,
                                                        table.data_ptr(), st_, s)

    def host_wait(block_len=4096, off_=offsets, sz_=sizes):
        return L.tsqa_compress_batch_packed_split(h, d_in.data_ptr(), d_in.numel(), items, n, 1, 16, block_len, out.data_ptr(), 1 << 16, off_,
                                                  sz_, table.data_ptr(), s)

    def tables(block_len=4096, at_=d_at.data_ptr(), st_=d_status.data_ptr(), item_=d_item.data_ptr(), first_=d_first.data_ptr()):
        return L.tsqa_compress_batch_packed_tables_split_async(h, d_in.data_ptr(), d_in.numel(), at_, d_sz.data_ptr(), n, 64, 1, 16, block_len,
                                                               out.data_ptr(), 1 << 16, d_offsets.data_ptr(), d_sizes.data_ptr(), first_,
                                                               d_bound.data_ptr(), table.data_ptr(), item_, st_, s)

    for bl in (0, 2048, 4097, 1 << 23):
        assert host_async(block_len=bl) == ERR_ARG and host_wait(block_len=bl) == ERR_ARG and tables(block_len=bl) == ERR_ARG, bl
    for kw in (dict(d_in_=None), dict(out_=None), dict(off_=None), dict(sz_=None), dict(st_=None), dict(items_=None), dict(align=3), dict(n_=0)):
        assert host_async(**kw) == ERR_ARG, kw
    assert host_wait(off_=None) == ERR_ARG and host_wait(sz_=None) == ERR_ARG
    for kw in (dict(at_=None), dict(st_=None), dict(item_=None), dict(first_=None)):
        assert tables(**kw) == ERR_ARG, kw
    for variant in (1, 2, 3, 4, 5):
        codec.set_variant(variant, 0)
        assert host_async() == ERR_ARG and host_wait() == ERR_ARG and tables() == ERR_ARG, variant
    codec.set_variant(0, 0)
    import torch
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), guard)
    for t in (d_offsets, d_sizes, d_first, d_bound):
        assert (t.cpu().numpy() == WORD_GUARD).all()
    for t in (table, d_item, d_status):
        assert (t.cpu().numpy() == TABLE_GUARD).all()


# ---- the Python face ---------------------------------------------------------------------------------------------------------------------

def test_packed_batch_of_short_blocks_decompresses_indexes_and_joins(codec, tsq, oracle):
    """PackedBatch.decompress, .index() and .join() on the result, unchanged"""
    b = bg.room_batch()
    srcs = [to_dev(b.item(i)) for i in range(len(b.specs))]
    for ext in (0, 1):
        e = b.expect(oracle, ext)
        batch = codec.compress_batch_packed(srcs, ext, block_len=4096)
        assert (batch.offsets, batch.sizes, batch.first_block, batch.block_len) == (e["offsets"], e["sizes"], e["first_block"], 4096)
        assert batch.d_block_sizes.cpu().tolist() == e["block_sizes"]
        for i, v in enumerate(batch.views):
            assert v.cpu().numpy().tobytes() == b.made(oracle, ext)[i][0]
        for i, v in enumerate(batch.decompress()):
            assert v.cpu().numpy().tobytes() == b.item(i).tobytes()
        idx = batch.index()
        mid = bg.ROOM_MID
        assert idx.read(mid, 4000, 5000).cpu().numpy().tobytes() == b.item(mid)[4000:9000].tobytes()
        assert idx.read(0, 0, b.in_sizes[0]).cpu().numpy().tobytes() == b.item(0).tobytes()
        idx.close()
        joined, table = batch.join(block_sizes=True)
        assert table.cpu().tolist() == e["block_sizes"], "the tables laid end to end are the joined container's"
        whole = np.concatenate([b.item(i) for i in range(len(b.specs))])
        assert codec.decompress_sized(joined, batch.d_block_sizes).cpu().numpy().tobytes() == whole.tobytes()
        lo, hi = batch.first_block[mid], batch.first_block[mid + 1]
        sized = codec.index_sized(batch.views[mid], b.in_sizes[mid], 4096, batch.d_block_sizes[lo:hi])
        assert sized.read(4090, 100).cpu().numpy().tobytes() == b.item(mid)[4090:4190].tobytes()
        sized.close()
        import torch
        with pytest.raises(tsq.TsqError) as err:
            codec.compress_batch_packed(srcs, ext, out=torch.empty(e["offsets"][-1] - 1, dtype=torch.uint8, device="cuda"), block_len=4096)
        assert err.value.code == ERR_OVERFLOW and err.value.needed == e["offsets"][-1]
    d_in, d_at, d_sz = dev(b)
    batch = codec.compress_packed_tables(d_in, d_at, d_sz, 1, block_len=4096)
    e = b.expect(oracle, 1)
    assert (batch.offsets, batch.sizes, batch.first_block) == (e["offsets"], e["sizes"], e["first_block"])
    assert batch.d_block_sizes.cpu().tolist() == e["block_sizes"]
    assert [v.cpu().numpy().tobytes() for v in batch.decompress()] == [b.item(i).tobytes() for i in range(len(b.specs))]
    assert codec.compress_batch_packed(srcs, 1).block_len is None


# ---- chains on one stream ----------------------------------------------------------------------------------------------------------------

def chain_inputs(budget):
    """a batch, and a second with more items and more blocks, so that the scratch grows between the two links"""
    return bg.room_batch(), bg.ownership(budget)[-1]


def enqueue_split(codec, b, ext):
    """the split packed compress of b on the current stream, nothing waited for -> (arena, d_offsets, d_sizes, table, bound)"""
    import torch
    import turbosqueeze_amd as tsq
    first, bound = tsq.plan_batch_split(b.places, b.in_size, b.block_len, b.align)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    d_offsets, d_sizes = words(len(b.specs) + 1), words(len(b.specs))
    table = words(first[-1], np.int32)
    codec.compress_batch_packed_split_async(dev(b)[0], b.places, ext, b.align, b.block_len, out, d_offsets, d_sizes, table)
    return out, d_offsets, d_sizes, table, first


def test_chain_to_the_dense_decompress(codec, oracle, side, budget):
    import torch
    results = []
    for b in chain_inputs(budget):
        dev(b)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for b in chain_inputs(budget):
            n = len(b.specs)
            arena, d_offsets, d_sizes, table, first = enqueue_split(codec, b, 1)
            back = torch.zeros(b.in_size + 16 * n, dtype=torch.uint8, device="cuda")
            t = (words(n + 1), words(n), words(n + 1), words(n, np.int32))
            codec.decompress_batch_packed_dense_async(arena, d_offsets, d_sizes, n, first[-1], 16, back, *t)
            results.append((b, back, t))
    side.synchronize()
    for b, back, t in results:
        assert codec._status.item() == OK and not t[3].cpu().numpy().any(), b.name
        host, at = back.cpu().numpy(), t[0].cpu().tolist()
        for i in range(len(b.specs)):
            assert host[at[i]:at[i] + b.in_sizes[i]].tobytes() == b.item(i).tobytes(), (b.name, i)


def test_chain_to_join_and_the_sized_decompress(codec, oracle, side, budget):
    import torch
    results = []
    for b in chain_inputs(budget):
        dev(b)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for b in chain_inputs(budget):
            n = len(b.specs)
            arena, d_offsets, d_sizes, table, first = enqueue_split(codec, b, 1)
            joined = torch.zeros(arena.numel(), dtype=torch.uint8, device="cuda")
            d_first, jt, d_item = words(n + 1), words(first[-1], np.int32), words(n, np.int32)
            codec.join_async(arena, d_offsets, d_sizes, n, first[-1], joined, d_first, jt, d_item)
            back = torch.zeros(b.in_size, dtype=torch.uint8, device="cuda")
            codec.decompress_sized_async(joined, first[-1], jt, back)
            results.append((b, back, table, jt, d_first, first, codec._size.clone(), codec._status.clone()))
    side.synchronize()
    for b, back, table, jt, d_first, first, size, status in results:
        total = sum(b.in_sizes)
        assert status.item() == OK and size.item() == total, b.name
        assert back.cpu().numpy()[:total].tobytes() == b.data[:total].tobytes(), b.name
        assert jt.cpu().tolist() == table.cpu().tolist() and d_first.cpu().tolist() == first, b.name


def test_chain_to_index_batch_and_gather(codec, oracle, side, budget):
    import torch
    results = []
    for b in chain_inputs(budget):
        dev(b)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for k, b in enumerate(chain_inputs(budget)):
            n = len(b.specs)
            e = b.expect(oracle, 1)
            arena, d_offsets, d_sizes, table, first = enqueue_split(codec, b, 1)
            idx = codec.index_batch([arena[o:o + z] for o, z in zip(e["offsets"], e["sizes"])])
            rng = np.random.default_rng(900 + k)
            items = rng.integers(0, n, 40)
            offs = np.array([rng.integers(0, b.in_sizes[i]) for i in items])
            lens = np.array([rng.integers(0, b.in_sizes[i] - o + 1) for i, o in zip(items, offs)])
            out, d_out_offsets = idx.gather(to_dev(items.astype(np.int32)), to_dev(offs.astype(np.int64)), to_dev(lens.astype(np.int64)),
                                            out=torch.zeros(int(lens.sum()) + 1, dtype=torch.uint8, device="cuda"), cap_pieces=4 * 40 + int(lens.sum()) // 4096)
            results.append((b, idx, items, offs, lens, out, d_out_offsets))
    side.synchronize()
    for b, idx, items, offs, lens, out, d_out_offsets in results:
        host, at = out.cpu().numpy(), d_out_offsets.cpu().tolist()
        assert codec._status.item() == OK
        for k, (i, o, ln) in enumerate(zip(items, offs, lens)):
            assert host[at[k]:at[k] + ln].tobytes() == b.item(int(i))[o:o + ln].tobytes(), (b.name, k)
        idx.close()
