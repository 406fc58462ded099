"""GPU tests of record reads from a batch of containers (tsqa_index_create_batch + tsqa_decompress_item_ranges*): every byte read
is compared with a slice of the oracle's decompress of that item's container (inputs from turbosqueeze_amd.synth), and nothing outside
a read's destination may change: outputs are sentinel-filled, with gaps of 1..47 guard bytes in front of every destination (every
residue mod 16 occurs)."""
import json
import os

import numpy as np
import pytest

import kat

pytestmark = pytest.mark.gpu

MiB4 = 1 << 22
ERR_ARG, ERR_FORMAT, ERR_STREAM = 3, 4, 5


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


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(n):
    return ((np.arange(n, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5


def fenced(rng, lengths):
    """destinations for ranges of the given lengths, each behind a gap of 1..47 guard bytes"""
    at, outs = 0, []
    for ln in lengths:
        at += int(rng.integers(1, 48))
        outs.append(at)
        at += int(ln)
    return outs, at + 64


def read_fenced(idx, ranges, outs, cap, sync=True):
    """read (item, offset, length) ranges to the destinations `outs` of a sentinel-filled buffer; -> (buffer on the host, error code
    or 0), after checking that every byte outside the destinations still holds the sentinel"""
    from turbosqueeze_amd import TsqError
    import torch
    guard = sentinel(cap)
    out = to_dev(guard)
    rc = 0
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            idx.read_items_into([(i, o, ln, a) for (i, o, ln), a in zip(ranges, outs)], out, sync=sync)
        side.synchronize()
        if not sync:
            rc = idx.codec.status()
    except TsqError as e:
        rc = e.code
    host = out.cpu().numpy()
    mask = np.ones(cap, dtype=bool)
    for (_, _, ln), a in zip(ranges, outs):
        mask[a:a + ln] = False
    assert np.array_equal(host[mask], guard[mask]), "a read wrote outside its destination"
    return host, rc


def check_item_ranges(idx, plains, ranges, rng):
    outs, cap = fenced(rng, [ln for _, _, ln in ranges])
    host, rc = read_fenced(idx, ranges, outs, cap)
    assert rc == 0
    for (i, o, ln), a in zip(ranges, outs):
        assert np.array_equal(host[a:a + ln], plains[i][o:o + ln]), f"item {i} range ({o}, {ln}) at {a} differs"
    return outs


MIXED_SIZES = [1, 2, 100, 5000, 65536, MiB4, MiB4 + 1, 2 * MiB4 + 12345, 300_000, MiB4 - 1, 17, 3 * MiB4, 1_000_000]


@pytest.fixture(scope="module", params=[0, 1])
def mixed(request, tsq, codec, oracle):
    """a batch of mixed items (1 B ... three blocks; text and mix) made by compress_batch -> (ext, blobs, oracle-decoded plains, index)"""
    ext = request.param
    datas = [(tsq.synth.text if k % 2 == 0 else tsq.synth.mix)(n, seed=100 + 7 * k + ext) for k, n in enumerate(MIXED_SIZES)]
    blobs = codec.compress_batch([to_dev(d) for d in datas], ext)
    plains = []
    for d, b in zip(datas, blobs):
        p = np.frombuffer(oracle.decompress(b.cpu().numpy(), threads=4), dtype=np.uint8)
        assert np.array_equal(p, d)
        plains.append(p)
    idx = codec.index_batch(blobs)
    yield ext, blobs, plains, idx
    idx.close()


def test_index_of_a_mixed_batch(mixed):
    _, _, plains, idx = mixed
    assert idx.items == len(plains) and idx.worst_status == 0
    assert [idx.item_total(i) for i in range(idx.items)] == [p.size for p in plains]
    assert all(idx.item_status(i) == 0 for i in range(idx.items))
    assert idx.total == sum(p.size for p in plains)
    assert idx.n_blocks == sum((p.size + MiB4 - 1) // MiB4 for p in plains)
    assert idx.item_status(idx.items) == ERR_ARG and idx.item_total(idx.items) == 0


def test_thousands_of_item_ranges_in_one_call(mixed):
    _, _, plains, idx = mixed
    rng = np.random.default_rng(31)
    ranges = []
    for k in range(3000):
        i = int(rng.integers(0, len(plains)))
        n = plains[i].size
        if k % 100 == 0:
            ln = int(rng.integers(1, n + 1))                       # long: often across block edges
        else:
            ln = int(rng.integers(1, min(n, 400) + 1))             # records: many per block
        ranges.append((i, int(rng.integers(0, n - ln + 1)), ln))
    # ranges across every block edge, duplicates of the same source, overlapping sources, whole items, empty ranges
    for i, p in enumerate(plains):
        for edge in range(MiB4, p.size, MiB4):
            ranges += [(i, edge - 77, min(200, p.size - edge + 77)), (i, edge - 1, 2), (i, edge, 1), (i, edge - 1, 1)]
        ranges += [(i, 0, p.size), (i, 0, p.size), (i, p.size - 1, 1), (i, 0, 0)]
    ranges += [ranges[5], ranges[5], ranges[17], (7, 100, 50_000), (7, 120, 50_000), (7, 100, 50_000)]
    order = rng.permutation(len(ranges))
    ranges = [ranges[k] for k in order]
    outs = check_item_ranges(idx, plains, ranges, rng)
    assert {a % 16 for a in outs} == set(range(16))
    # one range per call, and the packed forms
    for i, o, ln in ranges[:40]:
        assert np.array_equal(idx.read(i, o, ln).cpu().numpy(), plains[i][o:o + ln])
    some = ranges[40:140]
    packed, views = idx.read_many(some)
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([plains[i][o:o + ln] for i, o, ln in some]))
    assert all(np.array_equal(v.cpu().numpy(), plains[i][o:o + ln]) for v, (i, o, ln) in zip(views, some))


def test_many_records_in_one_block_and_one_long_window(mixed):
    """five hundred records of 64 bytes and a window of three MiB in one block: both kinds of work in the same group"""
    _, _, plains, idx = mixed
    i = MIXED_SIZES.index(MiB4)
    rng = np.random.default_rng(77)
    ranges = [(i, int(o), 64) for o in rng.integers(0, MiB4 - 64, 500)] + [(i, 500_000, 3 * (1 << 20))]
    ranges += [(i, 4096 * k, 64) for k in range(100)] + [(i, 64 * k, 64) for k in range(400)]        # dense runs inside single chunks
    check_item_ranges(idx, plains, ranges, rng)


def test_flat_reads_see_the_concatenation(mixed):
    _, _, plains, idx = mixed
    cat = np.concatenate(plains)
    rng = np.random.default_rng(41)
    ranges = [(0, cat.size), (0, 1), (cat.size - 1, 1)]
    starts = np.cumsum([0] + [p.size for p in plains])
    ranges += [(int(s) - 3, 7) for s in starts[2:-1]]                                       # across item edges
    ranges += [(int(o), int(rng.integers(1, 100_000))) for o in rng.integers(0, cat.size - 100_000, 200)]
    packed, views = idx.read_flat_many(ranges)
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([cat[o:o + ln] for o, ln in ranges]))
    assert np.array_equal(views[0].cpu().numpy(), cat)


def test_refusals_leave_the_output_untouched(mixed, tsq):
    _, _, plains, idx = mixed
    cap = 100_000
    big = MIXED_SIZES.index(3 * MiB4)
    for quads in ([(len(plains), 0, 1, 0)],                          # an item number past the index
                  [(3, 4990, 11, 0)],                                # past the item's total
                  [(0, 1, 1, 0)],
                  [(big, 0, 1000, cap - 999)],                       # past the output
                  [(big, 0, 1000, 0), (4, 0, 1000, 999)]):           # overlapping destinations
        guard = sentinel(cap)
        out = to_dev(guard)
        for sync in (True, False):
            with pytest.raises(tsq.TsqError) as e:
                idx.read_items_into(quads, out, sync=sync)
            assert e.value.code == ERR_ARG
        assert np.array_equal(out.cpu().numpy(), guard)


def test_four_thousand_pages(tsq, codec, oracle):
    """4 096 x 64 KiB: one index_batch call; totals and statuses equal the per-item codec.index(blob) answers for a sample of
    items, and reads equal slices.  (That the creation costs a constant number of launches is shown by the kernel trace of
    tools/record_time.py under profiles/, not by a wall time here.)"""
    n_pages, page = 4096, 65536
    data = tsq.synth.text(n_pages * page, seed=4096)
    src = to_dev(data)
    blobs = codec.compress_batch([src[k * page:(k + 1) * page] for k in range(n_pages)], 1)
    idx = codec.index_batch(blobs)
    assert idx.items == n_pages and idx.n_blocks == n_pages and idx.total == n_pages * page and idx.worst_status == 0
    rng = np.random.default_rng(12)
    for i in rng.integers(0, n_pages, 12).tolist() + [0, n_pages - 1]:
        one = codec.index(blobs[i])
        assert (idx.item_total(i), idx.item_status(i)) == (one.total, 0) and one.n_blocks == 1
        one.close()
        assert np.array_equal(np.frombuffer(oracle.decompress(blobs[i].cpu().numpy()), dtype=np.uint8), data[i * page:(i + 1) * page])
    plains = [data[k * page:(k + 1) * page] for k in range(n_pages)]
    ranges = [(int(i), int(o), 100) for i, o in zip(rng.integers(0, n_pages, 2000), rng.integers(0, page - 100, 2000))]
    ranges += [(0, 0, page), (n_pages - 1, 0, page), (n_pages - 1, page - 1, 1)]
    check_item_ranges(idx, plains, ranges, rng)
    idx.close()


def test_refused_items_and_a_damaged_stream(tsq, codec, oracle):
    """One container with a broken magic, one truncated: item_status TSQA_ERR_FORMAT, reads of them TSQA_ERR_ARG, reads of every
    other item exact.  A flipped stream byte inside one item: the call either reports TSQA_ERR_STREAM or returns the bytes the
    validating oracle returns for that item; the fence holds either way (containment: the decoder's refusals are ordinary status
    returns)."""
    rng = np.random.default_rng(99)
    sizes = [70_000, 300_000, MiB4 + 5, 1000, 2 * MiB4 + 9, 65536]
    datas = [tsq.synth.text(n, seed=500 + k) if k % 2 else tsq.synth.mix(n, seed=500 + k) for k, n in enumerate(sizes)]
    good = [np.frombuffer(oracle.compress(d, k & 1, threads=4), dtype=np.uint8) for k, d in enumerate(datas)]
    bad = [g.copy() for g in good]
    bad[1][0] ^= 0x01                                    # magic
    bad[4] = bad[4][: bad[4].size // 2]                  # truncated: its second frame runs past the end
    idx = codec.index_batch([to_dev(b) for b in bad])
    assert idx.worst_status == ERR_FORMAT and idx.items == len(sizes)
    want_status = [0, ERR_FORMAT, 0, 0, ERR_FORMAT, 0]
    assert [idx.item_status(i) for i in range(idx.items)] == want_status
    assert [idx.item_total(i) for i in range(idx.items)] == [0 if s else n for s, n in zip(want_status, sizes)]
    healthy = [i for i, s in enumerate(want_status) if not s]
    assert idx.total == sum(sizes[i] for i in healthy) and idx.n_blocks == sum((sizes[i] + MiB4 - 1) // MiB4 for i in healthy)
    for i in (1, 4):
        guard = sentinel(1000)
        out = to_dev(guard)
        with pytest.raises(tsq.TsqError) as e:
            idx.read_items_into([(i, 0, 1, 0)], out)
        assert e.value.code == ERR_ARG and np.array_equal(out.cpu().numpy(), guard)
    ranges = [(i, 0, sizes[i]) for i in healthy]
    for _ in range(300):
        i = healthy[int(rng.integers(0, len(healthy)))]
        ln = int(rng.integers(1, min(sizes[i], 3000) + 1))
        ranges.append((i, int(rng.integers(0, sizes[i] - ln + 1)), ln))
    check_item_ranges(idx, datas, ranges, rng)
    # the flat view: the concatenation of the healthy items
    cat = np.concatenate([datas[i] for i in healthy])
    packed, _ = idx.read_flat_many([(0, cat.size), (sizes[0] - 5, 10)])
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([cat, cat[sizes[0] - 5:sizes[0] + 5]]))
    idx.close()
    # a flipped byte in the body of item 2's first stream
    n_agree = n_refused = 0
    for case in range(12):
        hurt = [g.copy() for g in good]
        first_len = int(hurt[2][16]) | int(hurt[2][17]) << 8 | (int(hurt[2][18]) & 0x7F) << 16
        at = int(rng.integers(16 + 3 + 3, 16 + 3 + first_len))
        hurt[2][at] ^= 1 << int(rng.integers(0, 8))
        want = oracle.decompress(hurt[2])
        idx = codec.index_batch([to_dev(b) for b in hurt])
        assert idx.worst_status == 0
        ranges = [(2, 0, sizes[2]), (0, 100, 5000), (5, 0, 65536), (2, MiB4 - 10, 15)]
        outs, cap = fenced(rng, [ln for _, _, ln in ranges])
        host, rc = read_fenced(idx, ranges, outs, cap)
        if rc != 0:
            assert rc == ERR_STREAM, f"case {case}"
            n_refused += 1
        else:
            assert want is not None and bytes(host[outs[0]:outs[0] + sizes[2]]) == want, f"case {case}: accepted, but not the oracle's bytes"
            assert np.array_equal(host[outs[1]:outs[1] + 5000], datas[0][100:5100]) and np.array_equal(host[outs[2]:outs[2] + 65536], datas[5])
            n_agree += 1
        # reads that do not touch the damaged item are exact
        check_item_ranges(idx, datas, [(0, 0, sizes[0]), (3, 10, 900), (4, MiB4 - 100, 300)], rng)
        idx.close()
    assert n_agree + n_refused == 12


def test_async_calls_back_to_back(mixed, codec):
    """Two calls on one stream with no synchronise between them, with different range sets: the second may not overwrite the first's
    staged items and groups."""
    import torch
    _, _, plains, idx = mixed
    rng = np.random.default_rng(6)
    sets = []
    for s in range(2):
        rs = []
        for _ in range(700 + 300 * s):
            i = int(rng.integers(0, len(plains)))
            ln = int(rng.integers(1, min(plains[i].size, 100_000) + 1))
            rs.append((i, int(rng.integers(0, plains[i].size - ln + 1)), ln))
        sets.append(rs)
    results = []
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for rs in sets:
            packed, views = idx.read_many_async(rs)
            results.append((rs, packed, views))
    side.synchronize()
    assert codec.status() == 0
    for rs, packed, views in results:
        assert np.array_equal(packed.cpu().numpy(), np.concatenate([plains[i][o:o + ln] for i, o, ln in rs]))
        i, o, ln = rs[-1]
        assert np.array_equal(views[-1].cpu().numpy(), plains[i][o:o + ln])


def test_three_async_calls_in_flight(tsq, codec, oracle):
    """Three calls on one stream with no synchronise between them: the staged items and groups go through a ring of two slots, so
    the third call takes the slot of the first, once that one has finished.  One container of two blocks, three ranges of 1..100
    bytes per call, one of them across the block edge."""
    import torch
    n = MiB4 + 1000
    blob = oracle.compress(tsq.synth.text(n, seed=62), 1, threads=2)
    plain = np.frombuffer(oracle.decompress(blob, threads=2), dtype=np.uint8)
    idx = codec.index_batch([to_dev(np.frombuffer(blob, dtype=np.uint8))])
    sets = [[(0, 1), (MiB4 - 40, 100), (n - 7, 7)], [(123457, 100), (MiB4 - 1, 2), (MiB4, 33)], [(5, 64), (MiB4 + 900, 100), (MiB4 - 99, 100)]]
    results = []
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for rs in sets:
            results.append((rs, idx.read_many_async([(0, o, ln) for o, ln in rs])[0]))
    side.synchronize()
    assert codec.status() == 0
    for rs, packed in results:
        assert np.array_equal(packed.cpu().numpy(), np.concatenate([plain[o:o + ln] for o, ln in rs])), rs
    idx.close()


def test_an_index_of_one_container_takes_item_reads(tsq, codec, oracle):
    """tsqa_index_create's index is a batch of one item"""
    n = 2 * MiB4 + 4321
    data = tsq.synth.text(n, seed=8)
    blob = to_dev(np.frombuffer(oracle.compress(data, 1, threads=4), dtype=np.uint8))
    idx = codec.index_batch([blob])
    assert idx.items == 1 and idx.item_total(0) == n
    rng = np.random.default_rng(8)
    check_item_ranges(idx, [data], [(0, int(o), 100) for o in rng.integers(0, n - 100, 256)] + [(0, 0, n)], rng)
    idx.close()
    # the same reads through the index tsqa_index_create makes
    flat = codec.index(blob)
    L = tsq.lib()
    assert int(L.tsqa_index_items(flat.h)) == 1 and int(L.tsqa_index_item_total(flat.h, 0)) == n
    offs = rng.integers(0, n - 100, 300).tolist() + [MiB4 - 50, 2 * MiB4 - 1]
    rr = tsq.api._item_range_array([(0, o, 100, 3 + 100 * k) for k, o in enumerate(offs)])
    guard = sentinel(3 + 100 * len(offs) + 9)
    out = to_dev(guard)
    assert L.tsqa_decompress_item_ranges(codec.h, flat.h, rr, len(offs), out.data_ptr(), out.numel(), None) == 0
    host = out.cpu().numpy()
    assert np.array_equal(host[3:-9], np.concatenate([data[o:o + 100] for o in offs]))
    assert np.array_equal(host[:3], guard[:3]) and np.array_equal(host[-9:], guard[-9:])
    rr = tsq.api._item_range_array([(1, 0, 1, 0)])
    assert L.tsqa_decompress_item_ranges(codec.h, flat.h, rr, 1, out.data_ptr(), out.numel(), None) == ERR_ARG
    flat.close()


def read_tiled(idx, plains, tiles, rec, pitch, front):
    """Read records of `rec` bytes tiled over bytes [0, upto) of each (item, upto) of `tiles` in ONE call, record k of the call to
    front + pitch * k of a sentinel-filled buffer, and hold every byte of the buffer against the model: the records' bytes inside
    their destinations, the sentinel everywhere else.  No range of the call is longer than a record."""
    quads, k = [], 0
    for item, upto in tiles:
        for o in range(0, upto, rec):
            quads.append((item, o, min(rec, upto - o), front + pitch * k))
            k += 1
    cap = front + pitch * k + 40
    want = sentinel(cap)
    for item, o, ln, a in quads:
        want[a:a + ln] = plains[item][o:o + ln]
    out = to_dev(sentinel(cap))
    idx.read_items_into(quads, out)
    host = out.cpu().numpy()
    wrong = np.flatnonzero(host != want)
    assert wrong.size == 0, f"{wrong.size} bytes differ, the first at {int(wrong[0])} (record {(int(wrong[0]) - front) // pitch})"


TILED_SIZES = [1 << 20, MiB4, 3_000_000, 231_000, 109_888, 2 * MiB4 + 70_001]


@pytest.fixture(scope="module")
def tiled(tsq, codec):
    datas = [tsq.synth.text(n, seed=900 + k) if k % 2 == 0 else tsq.synth.mix(n, seed=900 + k) for k, n in enumerate(TILED_SIZES)]
    page = 65536
    pages = tsq.synth.text(48 * page, seed=77)
    datas += [pages[k * page:(k + 1) * page] for k in range(48)]
    blobs = codec.compress_batch([to_dev(d) for d in datas], 1)
    idx = codec.index_batch(blobs)
    assert idx.worst_status == 0
    yield datas, idx
    idx.close()


@pytest.mark.parametrize("rec,pitch,front", [(64, 64, 5), (64, 64, 16), (100, 100, 5), (100, 112, 32), (64, 67, 1), (24, 24, 7)])
def test_every_record_of_whole_items(tiled, rec, pitch, front):
    """Every record of multi-chunk blocks and of 64 KiB pages in one call, packed at odd and at 16-byte aligned destinations, with
    no long range in the call: every chunk of every block, the last one included, carries dozens to hundreds of live records, and
    the cursor moves with every chunk."""
    datas, idx = tiled
    read_tiled(idx, datas, [(i, d.size) for i, d in enumerate(datas)], rec, pitch, front)


def test_groups_that_end_anywhere_in_a_chunk(tiled):
    """Records tiled over [0, upto) of a block for many values of upto: the group's hi falls early, in the middle and late in its
    last chunk, and that chunk's records are written out by all sixteen wavefronts after the chunk loop."""
    datas, idx = tiled
    rng = np.random.default_rng(15)
    for rec, pitch, front in ((64, 64, 5), (64, 64, 16), (100, 100, 3)):
        uptos = [109_888, 231_000, 64 * 1717, 11_000, 22_000, 9 * 1024, 700_000] + rng.integers(5_000, 1 << 20, 25).tolist()
        for upto in uptos:
            read_tiled(idx, datas, [(0, int(upto))], rec, pitch, front)
        # several blocks at once, each ending somewhere else
        read_tiled(idx, datas, [(i, int(rng.integers(8_000, min(d.size, 1 << 20)))) for i, d in enumerate(datas[:8])], rec, pitch, front)


def test_containers_of_reference_streams_in_one_arena(codec, tsq):
    """The golden block streams the compiled reference produced, framed as one-block containers (as
    test_gpu_range.py::test_containers_of_reference_streams frames them), all of them in one arena under one index."""
    golden = kat.GOLDEN
    manifest = json.load(open(os.path.join(golden, "manifest.json")))
    names = sorted(k for k in manifest if os.path.exists(os.path.join(golden, k + ".in")))
    blobs, plains = [], []
    for name in names:
        data = np.fromfile(os.path.join(golden, name + ".in"), dtype=np.uint8)
        for ext, tag in ((0, "noext"), (1, "ext")):
            stream = open(os.path.join(golden, f"{name}.{tag}"), "rb").read()
            frame = len(stream) | (ext << 23)
            blob = b"TSQ1" + (1).to_bytes(4, "little") + data.size.to_bytes(8, "little") + frame.to_bytes(3, "little") + stream
            blobs.append(to_dev(np.frombuffer(blob, dtype=np.uint8)))
            plains.append(data)
    assert len(blobs) >= 4
    idx = codec.index_batch(blobs)
    assert idx.worst_status == 0 and [idx.item_total(i) for i in range(idx.items)] == [p.size for p in plains]
    rng = np.random.default_rng(5)
    ranges = []
    for i, p in enumerate(plains):
        n = p.size
        ranges += [(i, 0, n), (i, n - 1, 1), (i, n // 2, n - n // 2)]
        ranges += [(i, int(o), int(rng.integers(1, n - o + 1))) for o in rng.integers(0, n, 20).tolist()]
    check_item_ranges(idx, plains, ranges, rng)
    idx.close()
