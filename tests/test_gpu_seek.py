"""GPU tests of the index made from a size table (tsqa_index_create_sized*): seekgen's cases through the kernels.  Every read goes
into a sentinel-filled buffer with a fence behind it, through tsqa_decompress_ranges_async and tsqa_decompress_item_ranges_async,
and is held against the input bytes and against the same read through tsqa_index_create.  The reads of refused indexes are safe
because a descriptor the walk did not write is all zeros (the read kernels refuse stream_len < 3), one it did write passed
read_frame (its stream lies inside n), and the gate in front of the read kernel hands the verdict on before any block is decoded."""
import ctypes as C

import numpy as np
import pytest

import seekgen as kg
import splitgen as sg

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT = 0, kg.ERR_ARG, kg.ERR_FORMAT
ENTRIES = ("ranges", "item_ranges")
FENCE = 4096
TABLE_GUARD = 0x5EA1ED


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (the pattern repeats every 251 bytes)"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


class Input:
    """an input and the container and size table the split compress owes for its prefixes (splitgen.expected_split, made with
    the oracle), made once per (n, block_len, ext)"""

    def __init__(self, data, oracle):
        self.data, self.oracle, self._want = data, oracle, {}

    def want(self, n, block_len, ext):
        key = (n, block_len, ext)
        if key not in self._want:
            self._want[key] = sg.expected_split(self.oracle, self.data[:n], block_len, ext)
        return self._want[key]


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


@pytest.fixture(scope="module")
def budget():
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def counts(oracle, budget):
    return Input(sg.count_input(budget), oracle)


@pytest.fixture(scope="module")
def carry(oracle):
    data, bl = kg.carry()
    return Input(data, oracle), bl


def table_dev(table):
    return to_dev(np.array([int(x) for x in table], dtype=np.uint32).view(np.int32))


def blob_dev(blob, n):
    """the first n bytes of the container, at the very end of their allocation"""
    return to_dev(np.frombuffer(bytes(blob[:n]), dtype=np.uint8))


def create(codec, d_blob, n, n_total, block_len, d_tab, wait=False, stream=None):
    """-> (rc, handle): tsqa_index_create_sized_async, or the waiting form"""
    h = C.c_void_p(0x1234)
    f = codec.L.tsqa_index_create_sized if wait else codec.L.tsqa_index_create_sized_async
    rc = f(codec.h, d_blob.data_ptr() if d_blob is not None else None, n, n_total, block_len, d_tab.data_ptr() if d_tab is not None else None,
           C.byref(h), stream if stream is not None else codec._stream())
    return rc, h


def classic(codec, d_blob, n):
    h = C.c_void_p()
    rc = codec.L.tsqa_index_create(codec.h, d_blob.data_ptr(), n, C.byref(h))
    assert rc == OK, codec.last_error()
    return h


def verdict(codec, h):
    """the verdict word of a sized index, as a read of nothing hands it on (the waiting form returns the status word)"""
    import torch
    one = torch.empty(1, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return codec.L.tsqa_decompress_ranges(codec.h, h, None, 0, one.data_ptr(), 1, codec._stream())


def enqueue_read(tsq, codec, h, ranges, entry, out, out_cap, status, stream):
    """ranges: (offset, length) pairs, packed back to back from out[0]"""
    at, triples = 0, []
    for off, ln in ranges:
        triples.append((off, ln, at))
        at += ln
    assert at <= out_cap
    if entry == "ranges":
        return codec.L.tsqa_decompress_ranges_async(codec.h, h, tsq.api._range_array(triples), len(triples), out.data_ptr(), out_cap,
                                                    status.data_ptr(), stream)
    return codec.L.tsqa_decompress_item_ranges_async(codec.h, h, tsq.api._item_range_array([(0, o, l, a) for o, l, a in triples]), len(triples),
                                                     out.data_ptr(), out_cap, status.data_ptr(), stream)


def read(tsq, codec, h, ranges, entry):
    """-> (rc, *d_status, the output buffer with its fence, the sentinel it started from, out_cap)"""
    import torch
    out_cap = sum(ln for _, ln in ranges)
    guard = sentinel(out_cap + FENCE)
    out, status = to_dev(guard), torch.full((1,), 55, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()             # (the call runs on the context's own stream, which does not wait for torch's fills)
    rc = enqueue_read(tsq, codec, h, ranges, entry, out, out_cap, status, codec._stream())
    torch.cuda.synchronize()
    return rc, int(status.item()), out.cpu().numpy(), guard, out_cap


def expect(data, ranges, guard):
    want = np.array(guard, copy=True)
    at = 0
    for off, ln in ranges:
        want[at:at + ln] = data[off:off + ln]
        at += ln
    return want


def check_reads(tsq, codec, sized, plain, data, ranges, what):
    """each entry point, through the sized index and through tsqa_index_create's: the input's bytes, the fence intact, and equal"""
    for entry in ENTRIES:
        got = read(tsq, codec, sized, ranges, entry)
        ref = read(tsq, codec, plain, ranges, entry)
        assert got[:2] == (OK, OK) == ref[:2], (what, entry, got[:2], ref[:2], codec.last_error())
        want = expect(data, ranges, got[3])
        assert np.array_equal(got[2], want), f"{what}, {entry}: not the input's bytes, or the fence was written"
        assert np.array_equal(got[2], ref[2]), f"{what}, {entry}: differs from the read through tsqa_index_create"


# ---- true containers ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", [0, 1])
def test_true_cases(tsq, codec, counts, carry, budget, ext):
    import torch
    cases = [(counts, n, 4096) for _, n in kg.true_cases(budget)] + [(carry[0], carry[0].data.size, carry[1])]
    for inp, n, bl in cases:
        blob, sizes = inp.want(n, bl, ext)
        d_blob, d_tab = blob_dev(blob, len(blob)), table_dev(sizes)
        torch.cuda.synchronize()
        rc, h = create(codec, d_blob, len(blob), n, bl, d_tab)
        assert rc == OK and h.value, codec.last_error()
        assert verdict(codec, h) == OK, (n, bl)
        L = codec.L
        assert (L.tsqa_index_blocks(h), L.tsqa_index_total(h), L.tsqa_index_items(h)) == (len(sizes), n, 1)
        assert L.tsqa_index_item_total(h, 0) == n and L.tsqa_index_item_status(h, 0) == OK
        plain = classic(codec, d_blob, len(blob))
        check_reads(tsq, codec, h, plain, inp.data, kg.reads(n, bl), (n, bl))
        # the waiting form hands out an index that reads the same
        rc, hw = create(codec, d_blob, len(blob), n, bl, d_tab, wait=True)
        assert rc == OK and hw.value
        got = read(tsq, codec, hw, [(n - 1, 1), (0, min(n, 5000))], "ranges")
        assert got[:2] == (OK, OK) and np.array_equal(got[2], expect(inp.data, [(n - 1, 1), (0, min(n, 5000))], got[3]))
        for x in (h, hw, plain):
            L.tsqa_index_destroy(x)


def test_scan_loop_edge(tsq, codec):
    """256 groups - 1 frame, exactly 256 groups, and one frame more: launch 2 makes one pass, one full pass, and a second pass of
    one group that starts from the carried sum (seekgen.scan_edge_counts: re-derive them if the pass width changes)"""
    import torch
    counts_ = kg.scan_edge_counts()
    data = kg.scan_edge_input(max(counts_) * 4096)
    d_data = to_dev(data)
    _, bound = tsq.plan_split(data.size, 4096)
    out = torch.empty(bound, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(4204)
    for nb in counts_:
        n = nb * 4096 - 7
        tab = torch.full((nb,), TABLE_GUARD, dtype=torch.int32, device="cuda")
        size = C.c_size_t(0)
        torch.cuda.synchronize()
        rc = codec.L.tsqa_compress_device_split(codec.h, d_data.data_ptr(), n, 4096, out.data_ptr(), bound, C.byref(size), tab.data_ptr(), 1,
                                                codec._stream())
        assert rc == OK, codec.last_error()
        rc, h = create(codec, out, bound, n, 4096, tab)
        assert rc == OK and h.value, codec.last_error()
        assert verdict(codec, h) == OK, nb
        blocks = [0, nb - 3, nb - 2, nb - 1] + sorted(int(b) for b in rng.choice(nb - 4, 64, replace=False) + 1)
        ranges = [(b * 4096, min(4096, n - b * 4096)) for b in blocks]
        for entry in ENTRIES:
            got = read(tsq, codec, h, ranges, entry)
            assert got[:2] == (OK, OK), (nb, entry, got[:2])
            assert np.array_equal(got[2], expect(data, ranges, got[3])), (nb, entry)
        codec.L.tsqa_index_destroy(h)


# ---- refused containers ------------------------------------------------------------------------------------------------------------------

def refused_reads(n_total, block_len):
    nb = sg.plan_split(n_total, block_len)[0]
    out = [(0, min(n_total, 2 * block_len + 5)), (n_total - 1, 1)]
    return out + [(b * block_len - 3, 6) for b in sorted({1, nb // 2, nb - 1}) if 0 < b and b * block_len + 3 <= n_total]


def check_refused(tsq, codec, name, blob, n, table, n_total, block_len):
    import torch
    d_blob, d_tab = blob_dev(blob, n), table_dev(table)
    torch.cuda.synchronize()
    rc, h = create(codec, d_blob, n, n_total, block_len, d_tab, wait=True)
    assert rc == ERR_FORMAT and not h.value, (name, rc, codec.last_error())
    rc, h = create(codec, d_blob, n, n_total, block_len, d_tab)
    assert rc == OK and h.value, (name, codec.last_error())
    assert verdict(codec, h) == ERR_FORMAT, name
    for entry in ENTRIES:
        rc, st, host, guard, _ = read(tsq, codec, h, refused_reads(n_total, block_len), entry)
        assert (rc, st) == (OK, ERR_FORMAT), (name, entry, rc, st)
        assert np.array_equal(host, guard), f"{name}, {entry}: a read through a refused index wrote to its output"
    codec.L.tsqa_index_destroy(h)


@pytest.mark.parametrize("ext", [0, 1])
def test_false_tables(tsq, codec, carry, ext):
    inp, bl = carry
    blob, sizes = inp.want(inp.data.size, bl, ext)
    for name, c, n, table, why in kg.false_tables(blob, sizes):
        assert why in kg.index_refuses(c, n, table, inp.data.size, bl), name
        check_refused(tsq, codec, name, c, n, table, inp.data.size, bl)


@pytest.mark.parametrize("ext", [0, 1])
def test_geometry_cases(tsq, codec, oracle, ext):
    for name, blob, table, n_total, bl, why in kg.geometry(oracle, ext):
        assert why in kg.index_refuses(blob, len(blob), table, n_total, bl), name
        check_refused(tsq, codec, name, blob, len(blob), table, n_total, bl)


@pytest.mark.parametrize("ext", [0, 1])
def test_cuts(tsq, codec, counts, ext):
    n = 40 * 4096 - 5
    blob, sizes = counts.want(n, 4096, ext)
    for name, room, why in kg.cuts(blob, sizes):
        assert why in kg.index_refuses(blob, room, sizes, n, 4096), name
        check_refused(tsq, codec, name, blob, room, sizes, n, 4096)


@pytest.mark.parametrize("ext", [0, 1])
def test_damage_inside_a_stream_is_the_decoders_to_find(tsq, codec, counts, ext):
    import torch
    n, bl, k = 9 * 4096, 4096, 4
    blob, sizes = counts.want(n, bl, ext)
    bad = kg.damaged(blob, sizes, k)
    d_blob, d_tab = blob_dev(bad, len(bad)), table_dev(sizes)
    torch.cuda.synchronize()
    rc, h = create(codec, d_blob, len(bad), n, bl, d_tab)
    assert rc == OK and verdict(codec, h) == OK
    plain = classic(codec, d_blob, len(bad))
    for entry in ENTRIES:
        got, ref = read(tsq, codec, h, [(k * bl, bl)], entry), read(tsq, codec, plain, [(k * bl, bl)], entry)
        assert got[:2] == ref[:2] and np.array_equal(got[2], ref[2]), (entry, got[:2], ref[:2])
        assert np.array_equal(got[2][bl:], got[3][bl:])
    others = [(b * bl, bl) for b in range(9) if b != k]
    check_reads(tsq, codec, h, plain, counts.data, others, "the blocks beside the damaged one")
    codec.L.tsqa_index_destroy(h)
    codec.L.tsqa_index_destroy(plain)


def test_host_refusals_make_no_index_and_enqueue_nothing(tsq, codec, counts):
    import torch
    n, bl = 40_000, 4096
    blob, sizes = counts.want(n, bl, 0)
    nb = len(sizes)
    d_blob, d_tab = blob_dev(blob, len(blob)), table_dev(sizes)
    torch.cuda.synchronize()
    for wait in (False, True):
        def call(blob=d_blob, room=len(blob), total=n, block_len=bl, tab=d_tab):
            rc, h = create(codec, blob, room, total, block_len, tab, wait=wait)
            assert not h.value, "a refused call handed out an index"
            return rc
        assert call(blob=None) == ERR_ARG and call(tab=None) == ERR_ARG
        assert call(total=0) == ERR_ARG
        for bad in (0, 1, 2048, 4097, 12288, 1 << 23, 0xFFFFFFFF):
            assert call(block_len=bad) == ERR_ARG, bad
        assert call(total=1 << 44, room=1 << 40) == ERR_ARG          # 2^32 blocks
        assert call(room=sg.HEADER + sg.MIN_FRAME * nb - 1) == ERR_ARG
        assert codec.L.tsqa_index_create_sized_async(codec.h, d_blob.data_ptr(), len(blob), n, bl, d_tab.data_ptr(), None, codec._stream()) == ERR_ARG
    # a read without an index: refused before anything is enqueued, the status word and the output keep their sentinels
    for entry in ENTRIES:
        rc, st, host, guard, _ = read(tsq, codec, None, [(0, 100)], entry)
        assert (rc, st) == (ERR_ARG, 55) and np.array_equal(host, guard), entry
    # and the least room the host takes is taken
    rc, h = create(codec, d_blob, len(blob), n, bl, d_tab)
    assert rc == OK and verdict(codec, h) == OK
    codec.L.tsqa_index_destroy(h)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", [0, 1])
def test_chain_on_one_stream_without_a_wait(tsq, codec, ext):
    """split compress -> index from its table -> range read -> record read, twice, enqueued back to back on one stream with one
    synchronise at the end.  Index and reads are told the container's room, not its size; the table never leaves the device."""
    import torch
    L, s = codec.L, torch.cuda.Stream()
    i32 = lambda k, v: torch.full((k,), v, dtype=torch.int32, device="cuda")
    chains = []
    for data, bl in ((sg.mixed(700_003, 11), 1 << 13), (sg.mixed(300_001, 10), 1 << 12)):
        n = data.size
        nb, bound = tsq.plan_split(n, bl)
        ranges = kg.reads(n, bl)
        cap = sum(ln for _, ln in ranges)
        chains.append(dict(data=data, n=n, bl=bl, nb=nb, bound=bound, ranges=ranges, cap=cap, src=to_dev(np.concatenate([data, sentinel(256) | 1])),
                           blob=to_dev(sentinel(bound + FENCE)), tab=i32(nb + 16, TABLE_GUARD), outs=[to_dev(sentinel(cap + FENCE)) for _ in ENTRIES],
                           size=torch.full((1,), 777, dtype=torch.int64, device="cuda"), status=[i32(1, 55) for _ in range(3)], h=C.c_void_p()))
    torch.cuda.synchronize()
    rcs = []
    with torch.cuda.stream(s):
        hs = C.c_void_p(s.cuda_stream)
        for c in chains:
            rcs.append(L.tsqa_compress_device_split_async(codec.h, c["src"].data_ptr(), c["n"], c["bl"], c["blob"].data_ptr(), c["bound"],
                                                          c["size"].data_ptr(), c["tab"].data_ptr(), c["status"][0].data_ptr(), ext, hs))
            rcs.append(L.tsqa_index_create_sized_async(codec.h, c["blob"].data_ptr(), c["bound"], c["n"], c["bl"], c["tab"].data_ptr(),
                                                       C.byref(c["h"]), hs))
            for k, entry in enumerate(ENTRIES):
                rcs.append(enqueue_read(tsq, codec, c["h"], c["ranges"], entry, c["outs"][k], c["cap"], c["status"][1 + k], hs))
    s.synchronize()
    assert rcs == [OK] * len(rcs), (rcs, codec.last_error())
    for c in chains:
        assert [int(x.item()) for x in c["status"]] == [OK] * 3
        size = int(c["size"].item())
        host, t = c["blob"].cpu().numpy(), c["tab"].cpu().numpy()
        assert 16 + 6 * c["nb"] <= size <= c["bound"] and np.array_equal(host[size:], sentinel(c["bound"] + FENCE)[size:])
        assert (t[c["nb"]:] == TABLE_GUARD).all() and sg.frame_places([int(x) for x in t[:c["nb"]]])[-1] == size
        guard = sentinel(c["cap"] + FENCE)
        for k, entry in enumerate(ENTRIES):
            assert np.array_equal(c["outs"][k].cpu().numpy(), expect(c["data"], c["ranges"], guard)), (c["bl"], entry)
        torch.cuda.synchronize()
        assert verdict(codec, c["h"]) == OK
        L.tsqa_index_destroy(c["h"])


# ---- the Python face and the other kinds of index ----------------------------------------------------------------------------------------

def test_python_face(tsq, codec):
    import torch
    data = sg.mixed(300_001, 10)
    n, bl = data.size, 1 << 14
    src = to_dev(data)
    blob, table = codec.compress_split(src, 1, bl, block_sizes=True)
    for sync in (True, False):
        idx = codec.index_sized(blob, n, bl, table, sync=sync)
        assert isinstance(idx, tsq.SizedIndex) and (idx.n_blocks, idx.total) == (len(table), n)
        for off, ln in ((bl - 100, 200), (3 * bl - 1, 2), (5 * bl - 7, 2 * bl + 14), (n - 50, 50), (0, n)):
            assert idx.read(off, ln).cpu().numpy().tobytes() == data[off:off + ln].tobytes(), (sync, off, ln)
        packed, views = idx.read_many_async([(7, 100), (n - 9, 9)])
        torch.cuda.synchronize()
        assert codec.status() == OK and views[0].cpu().numpy().tobytes() == data[7:107].tobytes() and views[1].cpu().numpy().tobytes() == data[n - 9:].tobytes()
        assert idx.status() == OK
        idx.close()
    bad = table.clone()
    bad[3] += 1
    with pytest.raises(tsq.TsqError) as e:
        codec.index_sized(blob, n, bl, bad)
    assert e.value.code == ERR_FORMAT
    idx = codec.index_sized(blob, n, bl, bad, sync=False)        # nothing waited for: the refusal shows in the status
    assert idx.status() == ERR_FORMAT
    with pytest.raises(tsq.TsqError) as e:
        idx.read(0, 100)
    assert e.value.code == ERR_FORMAT
    idx.close()
    for args, code in (((blob, n, 3 << 12, table), ERR_ARG), ((blob, n, bl, table[:5].clone()), ERR_ARG), ((blob, n, bl, table.to(torch.int64)), ERR_ARG)):
        with pytest.raises(tsq.TsqError) as e:
            codec.index_sized(*args)
        assert e.value.code == code


def test_the_verdict_word_belongs_to_sized_indexes_alone(tsq, codec):
    import torch
    data = sg.mixed(100_000, 12)
    blob, table = codec.compress_split(to_dev(data), 0, 4096, block_sizes=True)
    plain, batch, sized = codec.index(blob), codec.index_batch([blob, blob]), codec.index_sized(blob, data.size, 4096, table)
    L = codec.L
    assert L.tsqa_index_d_status(plain.h) is None and L.tsqa_index_d_status(batch.h) is None and L.tsqa_index_d_status(None) is None
    assert L.tsqa_index_d_status(sized.h)
    # the flat reads of the other kinds are what they were
    assert plain.read(4090, 12).cpu().numpy().tobytes() == data[4090:4102].tobytes()
    assert batch.read(1, 4090, 12).cpu().numpy().tobytes() == data[4090:4102].tobytes()
    assert sized.read(4090, 12).cpu().numpy().tobytes() == data[4090:4102].tobytes()
    for x in (plain, batch, sized):
        x.close()
