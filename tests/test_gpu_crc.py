"""GPU tests of the CRC (tsqa_crc32_async, tsqa_crc32, DeviceCodec.crc32_async, RangeIndex.crc32, CrcTable, tsq_cli k): the cases are
crcgen's, every expected value is zlib.crc32 of the generators' bytes, and test_crc_cpu.py shows that each case reaches what it aims
at.  Every call runs on a side stream; every table the library may write sits between guard words, is filled with the guard first
and is compared WHOLE with its fences.  With skew 1 the tables start one element past a multiple of 16 bytes: 4-aligned, not
8-aligned."""
import ctypes as C
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import crcgen as kg
import findgen as fg
from test_gpu_cut import FENCE, Index, sentinel, to_dev
from test_gpu_gather import index_of
from test_gpu_records import GUARD, Table
from test_gpu_records import Room as RecordRoom
from test_gpu_records import records_call

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM = kg.OK, kg.ERR_ARG, kg.ERR_FORMAT, kg.ERR_STREAM


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


def u32(values):
    return [int(v) & 0xFFFFFFFF for v in values]


class Room:
    """the call's outputs for n_items items and n_blocks blocks, each between its fences"""

    def __init__(self, n_items, n_blocks, skew=0):
        import torch
        self.items, self.status = Table(n_items, torch.int32, skew), Table(n_items, torch.int32, skew)
        self.blocks, self.all, self.word = Table(n_blocks, torch.int32, skew), Table(1, torch.int32, skew), Table(1, torch.int32)
        if skew:
            assert self.items.ptr() % 8 == 4 and self.blocks.ptr() % 8 == 4

    def tables(self):
        return (self.items, self.status, self.blocks, self.all, self.word)


def crc_call(codec, index, room, sync=False, over=()):
    """tsqa_crc32_async (sync: tsqa_crc32) on the current stream -> its return value.  over: arguments replaced."""
    a = dict(ctx=codec.h, idx=index.h, flags=0, items=room.items.ptr(), status=room.status.ptr(), blocks=room.blocks.ptr(), all=room.all.ptr(),
             word=room.word.ptr())
    a.update(dict(over))
    f = codec.L.tsqa_crc32 if sync else codec.L.tsqa_crc32_async
    return f(a["ctx"], a["idx"], a["flags"], a["items"], a["status"], a["blocks"], a["all"], a["word"], codec._stream())


def check(room, e, what, blocks=True, whole=True):
    assert room.word.values().tolist() == [e["d_status"]], f"{what}: *d_status is {room.word.values().tolist()}, owed {e['d_status']}"
    got = room.status.values().tolist()
    assert got == e["status"], f"{what}: item statuses {[(k, g, w) for k, (g, w) in enumerate(zip(got, e['status'])) if g != w][:8]} (item, got, owed)"
    got = u32(room.items.values())
    assert got == e["items"], f"{what}: item CRCs {[(k, hex(g), hex(w)) for k, (g, w) in enumerate(zip(got, e['items'])) if g != w][:8]} (item, got, owed)"
    if whole:
        assert u32(room.all.values()) == [e["all"]], f"{what}: the whole data's CRC is {hex(u32(room.all.values())[0])}, owed {hex(e['all'])}"
    else:
        assert (room.all.values() == GUARD).all(), what
    got = u32(room.blocks.values())
    if blocks:
        bad = [(b, hex(g), hex(w)) for b, (g, w) in enumerate(zip(got, e["blocks"])) if w is not None and g != w]
        assert not bad, f"{what}: block CRCs {bad[:8]} (block, got, owed)"
    else:
        assert (room.blocks.values() == GUARD).all(), what


def run(codec, side, case, skew=0, index=None, blocks=True, whole=True, sync=False):
    import torch
    e = case.expect()
    index = index or index_of(codec, case.index)
    room = Room(case.index.n_items, case.index.n_blocks, skew)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rc = crc_call(codec, index, room, sync=sync, over=dict(**({} if blocks else dict(blocks=None)), **({} if whole else dict(all=None))))
    assert rc == (e["d_status"] if sync else 0), codec.last_error()
    side.synchronize()
    check(room, e, f"{case.name} (skew {skew})", blocks, whole)
    return room, e


# ---- cell and image edges -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", kg.COUNTS)
def test_cell_masks_and_skews_on_ragged_items(codec, side, n):
    """items of 1 to 40 bytes: as a batch every block is an item of its own, joined they are parts of one item"""
    for k, joined in enumerate((False, True)):
        room, e = run(codec, side, kg.ragged(n, joined), skew=k ^ (n & 1))
        if joined:
            # the blocks' CRCs of the batch, folded on the host, are the joined item's
            b = kg.ragged(n, False)
            folded = 0
            for i, crc in enumerate(b.expect()["items"]):
                folded = codec.L.tsqa_crc32_combine(folded, crc, b.index.item_span(i)[1])
            assert u32(room.items.values()) == [folded]


def test_bit_order_and_byte_order(codec, side):
    room, e = run(codec, side, kg.bits(), skew=1)
    assert len(set(u32(room.items.values()))) == 256


@pytest.mark.parametrize("byte", (0, 255))
def test_runs_of_one_byte_differ_by_the_init_term(codec, side, byte):
    room, e = run(codec, side, kg.runs(byte))
    got = u32(room.items.values())
    assert len(set(got)) == 32 and got[0] == 0


@pytest.mark.parametrize("kind", kg.CHUNK_CASES + kg.IMAGE_CASES)
def test_image_edges_and_the_running_fold(codec, side, kind):
    case = kg.chunks(kind) if kind in kg.CHUNK_CASES else kg.images(kind)
    run(codec, side, case, skew=len(kind) & 1)


def test_the_ring_wrap(codec, side):
    for k, case in enumerate(kg.ring_cases()):
        run(codec, side, case, skew=k)


# ---- shifts and folds -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", (1, 0))
def test_the_largest_shift_inside_a_block(codec, side, ext):
    run(codec, side, kg.two_blocks(ext), skew=ext)


@pytest.mark.parametrize("kind", ("sized", "plain"))
def test_the_fold_over_257_blocks(codec, side, kind):
    import torch
    case = kg.phrase(kind)
    with torch.cuda.stream(side):
        idx = index_of(codec, case.index)                     # (sized: made on the side stream, nothing waited for)
    room, e = run(codec, side, case, index=idx, skew=1)
    # d_block_crc folded on the host with tsqa_crc32_combine gives d_item_crc
    folded = 0
    for b, crc in enumerate(u32(room.blocks.values())):
        folded = codec.L.tsqa_crc32_combine(folded, crc, case.index.out_start[b + 1] - case.index.out_start[b])
    assert [folded] == u32(room.items.values()) == e["items"]


def test_the_fold_over_65537_blocks(codec, tsq, side):
    """seekgen.scan_edge_input at 65 537 blocks of 4 096 bytes, the last one byte long, made on the GPU"""
    import seekgen
    import torch
    bl, nb = 4096, 65537
    data = seekgen.scan_edge_input((nb - 1) * bl + 1)
    with torch.cuda.stream(side):
        blob = codec.compress_split(to_dev(data), 1, bl)
        idx = codec.index(blob)
        assert idx.n_blocks == nb
        t = idx.crc32(blocks=True)
    want = zlib.crc32(data.tobytes())
    assert u32(t.items.cpu().tolist()) == [want] and u32(t.all.cpu().tolist()) == [want] and int(t.d_status.item()) == OK
    got = u32(t.blocks.cpu().tolist())
    for b in (0, 1, 255, 256, 65535, 65536):
        assert got[b] == zlib.crc32(data[b * bl:(b + 1) * bl].tobytes()), b
    idx.close()


def test_an_item_past_512_mib(codec, tsq, side):
    """one item of 2^29 + 4 096 + 1 bytes at block_len 2^12, made on the GPU from a seeded tile of 1 MiB: the smallest item at which
    8 * len passes 2^32.  zlib is fed tile by tile."""
    import torch
    n, tile_n = (1 << 29) + 4096 + 1, 1 << 20
    tile = np.random.default_rng(kg.SEED + 29).integers(0, 256, tile_n, dtype=np.uint8)
    tile[: tile_n // 2] = tsq.synth.text(tile_n // 2, seed=29)
    with torch.cuda.stream(side):
        src = to_dev(tile).repeat(n // tile_n + 1)[:n].contiguous()
        blob = codec.compress_split(src, 1, 1 << 12)
        del src
        idx = codec.index(blob)
        t = idx.crc32()
    want, tb = 0, tile.tobytes()
    for _ in range(n // tile_n):
        want = zlib.crc32(tb, want)
    want = zlib.crc32(tb[:n % tile_n], want)
    assert idx.total == n and idx.n_blocks == (n + 4095) // 4096
    assert u32(t.items.cpu().tolist()) == [want] and u32(t.all.cpu().tolist()) == [want] and int(t.d_status.item()) == OK
    idx.close()


# ---- identity across routes -----------------------------------------------------------------------------------------------------------

def test_the_crc_does_not_depend_on_the_route(codec, tsq, side):
    """the same 1 MiB of text at block_len 2^12, 2^16 and 2^22, ext on and off; the join of items against the items' CRCs folded;
    a cut of the join at the items' first blocks gives the items' CRCs back"""
    import torch
    data = tsq.synth.text(1 << 20, seed=77)
    want = zlib.crc32(data.tobytes())
    with torch.cuda.stream(side):
        src = to_dev(data)
        for bl in (1 << 12, 1 << 16, 1 << 22):
            for ext in (1, 0):
                idx = codec.index(codec.compress_split(src, ext, bl))
                t = idx.crc32()
                assert u32(t.items.cpu().tolist()) == [want] == u32(t.all.cpu().tolist()), (bl, ext)
                idx.close()
        parts = [data[:70001], data[70001:70002], data[70002:500000], data[500000:]]
        batch = codec.compress_batch_packed([to_dev(p) for p in parts], 1, block_len=1 << 14)
        tb = batch.crc32()
        crcs = u32(tb.items.cpu().tolist())
        assert crcs == [zlib.crc32(p.tobytes()) for p in parts] and u32(tb.all.cpu().tolist()) == [want]
        joined = codec.index(batch.join())
        tj = joined.crc32()
        folded = 0
        for c, p in zip(crcs, parts):
            folded = tsq.crc32_combine(folded, c, p.size)
        assert u32(tj.items.cpu().tolist()) == [folded] == [want] == u32(tj.all.cpu().tolist())
        # cut(join(items)) at the items' first blocks: the items back, as a packed batch
        first = batch.first_block
        back = joined.cut([(first[k], first[k + 1] - first[k]) for k in range(len(parts))])
        assert u32(back.crc32().items.cpu().tolist()) == crcs
        joined.close()


# ---- verdicts -------------------------------------------------------------------------------------------------------------------------

def test_items_the_index_refused_keep_its_status(codec, side):
    """densegen's damaged headers as items 0, 17, 100, 255, 256 and the last of 300: status 4 and CRC 0, the 294 others exact"""
    room, e = run(codec, side, kg.damaged(), skew=1)
    assert [k for k, st in enumerate(room.status.values().tolist()) if st] == list(kg.rg.DAMAGED_AT)


@pytest.mark.parametrize("which", (0, 1))
def test_a_malformed_stream_costs_its_item_alone(codec, side, which):
    """an invalid twin as one block of a six-block item between healthy items: that item is TSQA_ERR_STREAM with CRC 0, the others
    are exact, *d_status is TSQA_ERR_STREAM and d_all_crc is 0; the waiting form returns the status"""
    case = kg.twin(which)
    room, e = run(codec, side, case)
    assert room.status.values().tolist() == [0, ERR_STREAM, 0] and u32(room.all.values()) == [0]
    run(codec, side, case, sync=True, skew=1)


def test_a_refused_sized_index_gives_format_and_zeros(codec, side):
    import torch
    case = kg.refused_case()
    with torch.cuda.stream(side):
        idx = index_of(codec, case.index)                     # (made on the side stream, nothing waited for: the call reads its verdict)
    room, e = run(codec, side, case, index=idx)
    assert room.word.values().tolist() == [ERR_FORMAT] and set(room.status.values().tolist()) == {ERR_FORMAT} and u32(room.all.values()) == [0]
    assert set(u32(room.blocks.values())) == {GUARD & 0xFFFFFFFF}, "no descriptor is read and no block word written"


def test_no_blocks_and_empty_items(codec, side):
    """an index of no blocks (both items refused at the header): CRCs 0, the statuses the index's own, the call's status 0"""
    case = kg.no_blocks()
    assert case.index.n_blocks == 0 and case.index.n_items == 2
    room, e = run(codec, side, case, skew=1)
    assert u32(room.items.values()) == [0, 0] and room.word.values().tolist() == [OK] and u32(room.all.values()) == [0]
    run(codec, side, case, sync=True)
    # an item of 0 bytes among others: CRC 0 with status 0 (runs' item 0), alone too
    one = kg.Case("empty_item", kg.rg.batch_of("crc_empty_item", [kg.one_block(b"", 1)], [b""]))
    room, e = run(codec, side, one)
    assert u32(room.items.values()) == [0] and room.status.values().tolist() == [0] and u32(room.all.values()) == [0]


def test_arguments_refused_on_the_host(codec, tsq, side):
    import torch
    case = kg.ragged(2, False)
    idx = index_of(codec, case.index)
    torch.cuda.synchronize()
    for what, over in (("null index", dict(idx=None)), ("null items", dict(items=None)), ("null item status", dict(status=None)),
                       ("null status", dict(word=None)), ("flags 1", dict(flags=1)), ("flags 2^31", dict(flags=0x80000000))):
        for sync in (False, True):
            room = Room(case.index.n_items, case.index.n_blocks)
            with torch.cuda.stream(side):
                rc = crc_call(codec, idx, room, sync=sync, over=over)
            side.synchronize()
            assert rc == ERR_ARG, (what, rc)
            assert all((tab.values() == GUARD).all() for tab in room.tables()), what
    # the optional tables may be NULL: nothing of them is written
    run(codec, side, case, blocks=False, whole=False)
    # a batch index made on the device and not yet fetched
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
            index.crc32()
        assert err.value.code == ERR_ARG and "tsqa_index_fetch" in str(err.value)
        table = index.fetch().crc32()
        assert u32(table.items.cpu().tolist()) == [zlib.crc32(p.tobytes()) for p in parts] and table.status.cpu().tolist() == [0, 0, 0]
        index.close()
    finally:
        fresh.close()


# ---- pipelines and wrappers -----------------------------------------------------------------------------------------------------------

def test_one_chain_on_one_stream(tsq, side):
    """split compress -> index_sized(sync=False) -> crc32_async -> a records call -> crc32_async of a larger container (the scratch
    grows): one stream, one shared context, nothing read back before the end"""
    import torch
    fresh = tsq.DeviceCodec(0)
    try:
        runs = []
        for n, bl, seed in ((300001, 4096, 81), (5 << 20, 4096, 82)):
            data = tsq.synth.text(n, seed=seed)
            nb, room = tsq.plan_split(n, bl)
            runs.append(dict(data=data, bl=bl, nb=nb, src=to_dev(data), blob=to_dev(sentinel(room)), table=torch.full((nb,), -1, dtype=torch.int32, device="cuda")))
        rec = RecordRoom(0, 1)
        torch.cuda.synchronize()
        tables = []
        with torch.cuda.stream(side):
            for k, r in enumerate(runs):
                fresh.compress_split_async(r["src"], 1, r["bl"], r["blob"], r["table"])
                r["idx"] = fresh.index_sized(r["blob"], r["data"].size, r["bl"], r["table"], sync=False)
                tables.append(fresh.crc32_async(r["idx"], blocks=True))
                if k == 0:
                    assert records_call(fresh, r["idx"], 10, 0, 0, rec, over=dict(items=None, offsets=None, lengths=None)) == 0
        side.synchronize()
        for r, t in zip(runs, tables):
            want = zlib.crc32(r["data"].tobytes())
            assert u32(t.items.cpu().tolist()) == [want] == u32(t.all.cpu().tolist()) and int(t.d_status.item()) == OK
            got = u32(t.blocks.cpu().tolist())
            assert got == [zlib.crc32(r["data"][b * r["bl"]:(b + 1) * r["bl"]].tobytes()) for b in range(r["nb"])]
        assert int(rec.need.values()[0]) == int((runs[0]["data"] == 10).sum()) + (runs[0]["data"][-1] != 10)
        for r in runs:
            r["idx"].close()
    finally:
        fresh.close()


def test_the_profile_slots_of_the_crc(tsq, side):
    import torch
    fresh = tsq.DeviceCodec(0)
    try:
        case = kg.phrase("plain")
        idx = Index(fresh, "plain", to_dev(np.frombuffer(case.index.blob, dtype=np.uint8)))
        room = Room(1, case.index.n_blocks)
        fresh.profile(True)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            assert crc_call(fresh, idx, room) == 0, fresh.last_error()
        side.synchronize()
        dm, dn, fm, fn = fresh.profile_read_crc()
        assert (dn, fn) == (1, 1) and dm > 0 and fm > 0
        assert fresh.profile_read_crc()[1::2] == (0, 0) and fresh.profile_read_find()[1::2] == (0, 0) and fresh.profile_read_records()[1::2] == (0, 0)
        check(room, case.expect(), "profiled")
        fresh.profile(False)
        idx.close()
    finally:
        fresh.close()


def test_the_command_line_tool_prints_the_crc(tmp_path):
    """tools/tsq_cli k: the total and the CRC-32 of the original file"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "tools", "tsq_cli")
    data = kg.dg._text(300000, kg.SEED + 5).tobytes()
    src, packed = tmp_path / "in.bin", tmp_path / "in.tsq"
    src.write_bytes(data)
    subprocess.run([cli, "c", str(src), str(packed)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([cli, "k", str(packed)], check=True, capture_output=True, timeout=120).stdout.decode()
    got = json.loads(out)
    assert got == {"bytes": len(data), "crc32": hex(zlib.crc32(data))}, out


def test_the_python_wrapper_and_check(codec, tsq):
    import torch
    data = tsq.synth.text(200000, seed=91)
    idx = codec.index(codec.compress_split(to_dev(data), 1, 1 << 14))
    t = idx.crc32(blocks=True)
    assert isinstance(t, tsq.CrcTable) and t.check() is t
    assert u32(t.items.cpu().tolist()) == [zlib.crc32(data.tobytes())] == u32(t.all.cpu().tolist())
    assert t.blocks.numel() == idx.n_blocks and t.status.cpu().tolist() == [0]
    t = idx.crc32(all=False)
    assert t.all is None and t.blocks is None
    idx.close()
    # a refused sized index raises from check()
    case = kg.refused_case()
    i = case.index
    with pytest.raises(tsq.TsqError) as err:
        bad = codec.index_sized(to_dev(np.frombuffer(i.blob, dtype=np.uint8)), i.total, i.block_len, to_dev(i.table, np.int32), sync=False)
        bad.crc32()
    assert err.value.code == ERR_FORMAT
    # a malformed stream that costs one of three items does not raise: the table says which
    twin = kg.twin().index
    t = tsq.BatchIndex(codec, to_dev(np.frombuffer(twin.blob, dtype=np.uint8)), list(twin.spans)).crc32()
    assert t.status.cpu().tolist() == [0, ERR_STREAM, 0] and int(t.d_status.item()) == ERR_STREAM and u32(t.all.cpu().tolist()) == [0]
