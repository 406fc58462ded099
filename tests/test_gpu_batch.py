"""GPU tests of batches (tsqa_compress_batch*, tsqa_decompress_batch*): every container is compared with the oracle's container of
that item alone, every round trip with the item itself; outputs are sentinel-filled with gaps of 1..47 guard bytes between items (every
residue mod 16 occurs), and nothing outside the items' output ranges may change."""
import ctypes as C

import numpy as np
import pytest

import fuzzgen
import kat
from turbosqueeze_amd.api import _batch_array

pytestmark = pytest.mark.gpu

MiB4 = 1 << 22
ERR_ARG, ERR_FORMAT, ERR_OVERFLOW, ERR_STALL = 3, 4, 6, 7


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


def fenced(rng, lengths, gap_lo=1):
    """offsets for pieces of the given lengths, each behind a gap of gap_lo..47 bytes -> (offsets, total size)"""
    at, outs = 0, []
    for ln in lengths:
        at += int(rng.integers(gap_lo, 48))
        outs.append(at)
        at += int(ln)
    return outs, at + 64


def arena_of(rng, datas, gap_lo=1):
    """the items in one host arena behind non-zero filler gaps -> (arena, offsets)"""
    outs, size = fenced(rng, [d.size for d in datas], gap_lo)
    arena = rng.integers(1, 256, size, dtype=np.uint8)
    for d, o in zip(datas, outs):
        arena[o:o + d.size] = d
    return arena, outs


def call_compress(codec, d_in, items, ext, out_size):
    """tsqa_compress_batch into a sentinel-filled output -> (host output, sizes, rc), the guards checked"""
    guard = sentinel(out_size)
    out = to_dev(guard)
    sizes = (C.c_uint64 * len(items))()
    rc = codec.L.tsqa_compress_batch(codec.h, d_in.data_ptr(), d_in.numel(), _batch_array(items), len(items), ext, out.data_ptr(),
                                     out_size, sizes, codec._stream())
    host = out.cpu().numpy()
    mask = np.ones(out_size, dtype=bool)
    for _, _, o, cap in items:
        mask[o:o + cap] = False
    assert np.array_equal(host[mask], guard[mask]), "a batch compress wrote outside its items' output ranges"
    return host, [int(s) for s in sizes], rc


def call_decompress(codec, d_in, items, out_size):
    """tsqa_decompress_batch into a sentinel-filled output -> (host output, sizes, item statuses, rc), the guards checked"""
    guard = sentinel(out_size)
    out = to_dev(guard)
    sizes = (C.c_uint64 * len(items))()
    status = (C.c_int32 * len(items))()
    rc = codec.L.tsqa_decompress_batch(codec.h, d_in.data_ptr(), d_in.numel(), _batch_array(items), len(items), out.data_ptr(), out_size,
                                       sizes, status, codec._stream())
    host = out.cpu().numpy()
    mask = np.ones(out_size, dtype=bool)
    for _, _, o, cap in items:
        mask[o:o + cap] = False
    assert np.array_equal(host[mask], guard[mask]), "a batch decompress wrote outside its items' output ranges"
    return host, [int(s) for s in sizes], [int(s) for s in status], rc


@pytest.fixture(autouse=True)
def default_variants(codec):
    codec.set_variant(0, 0)
    yield
    codec.set_variant(0, 0)


def round_trip(codec, oracle, tsq, datas, ext, rng, gap_lo=1, want=None):
    """compress the items as one batch and check every container against the oracle's container of the item alone; decompress the
    containers in place as one batch and check every item; -> the containers"""
    arena, offs = arena_of(rng, datas, gap_lo)
    d_in = to_dev(arena)
    caps = [tsq.batch_bound(d.size) for d in datas]
    outs, out_size = fenced(rng, caps)
    items = [(o, d.size, a, cap) for o, d, a, cap in zip(offs, datas, outs, caps)]
    host, sizes, rc = call_compress(codec, d_in, items, ext, out_size)
    assert rc == 0, codec.last_error()
    blobs = []
    for k, d in enumerate(datas):
        blob = host[outs[k]:outs[k] + sizes[k]].tobytes()
        w = want[k] if want is not None else oracle.compress(d, ext)
        assert blob == w, f"item {k} ({d.size} B): container differs from the oracle's of the item alone"
        blobs.append(blob)
    # the containers where they lie (in the compress output, which is sentinel-filled around them) back to the items
    d_blobs = to_dev(host)
    back_outs, back_size = fenced(rng, [d.size for d in datas])
    ditems = [(outs[k], sizes[k], back_outs[k], datas[k].size) for k in range(len(datas))]
    back, bsizes, status, rc = call_decompress(codec, d_blobs, ditems, back_size)
    assert rc == 0 and not any(status), (rc, codec.last_error())
    for k, d in enumerate(datas):
        assert bsizes[k] == d.size and np.array_equal(back[back_outs[k]:back_outs[k] + d.size], d), f"item {k}: round trip"
    return blobs


def fuzz_items(rng, count, tsq):
    out = []
    for k in range(count):
        n = int(rng.integers(1, 300_000)) if k % 5 else int(rng.integers(1, 2000))
        kind = k % 4
        if kind == 0:
            out.append(fuzzgen.structured(rng, n))
        elif kind == 1:
            out.append(kat.k7_textlike(n, seed=1000 + k))
        elif kind == 2:
            out.append(kat.xorshift32_bytes(n, seed=77 + k))
        else:
            out.append(tsq.synth.text(n, seed=k))
    return out


@pytest.mark.parametrize("ext", [0, 1])
def test_mixed_sizes_equal_oracle(codec, oracle, tsq, ext):
    rng = np.random.default_rng(10 + ext)
    sizes = [1, 2, 15, 16, 17, 699, 4096, 65535, MiB4 - 1, MiB4, MiB4 + 1, 9 * (1 << 20) + 5]
    datas = [tsq.synth.text(n, seed=n) if k % 2 else tsq.synth.mix(n, seed=n) for k, n in enumerate(sizes)]
    datas += fuzz_items(rng, 240, tsq)
    order = rng.permutation(len(datas))
    round_trip(codec, oracle, tsq, [datas[i] for i in order], ext, rng)


def test_lookahead_stays_inside_each_item(codec, oracle, tsq):
    """Items back to back, every one followed by non-zero bytes of the next: each container must be the oracle's of the item alone
    (a contiguous encode of the arena gives other streams where an item's look-ahead reaches into its neighbour)."""
    rng = np.random.default_rng(3)
    datas = [tsq.synth.text(int(n), seed=int(n)) for n in rng.integers(1, 150_000, 60)] + [tsq.synth.text(MiB4, seed=5), tsq.synth.text(99, seed=6)]
    sensitive = 0
    for a, b in zip(datas, datas[1:]):
        if a.size <= MiB4:
            sensitive += oracle.encode_block(a, 1, halo=b[:128]) != oracle.encode_block(a, 1)
    assert sensitive > 0, "no item of this batch would see its neighbour: the test would not tell"
    round_trip(codec, oracle, tsq, datas, 1, rng, gap_lo=0)


def test_more_blocks_than_one_launch(codec, oracle, tsq):
    """About 1 300 small items and multi-block items that straddle the launch boundaries (2 x CUs blocks per launch)."""
    import torch
    budget = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(4)
    big = {budget - 1: 9 * (1 << 20) + 5, 2 * budget - 2: 3 * MiB4 + 1, 3 * budget - 1: 2 * MiB4}
    datas, blocks = [], 0
    while len(datas) < 1300 or blocks < 3 * budget + 2:
        n = big.pop(blocks, 4096 + int(rng.integers(0, 64)))
        datas.append(tsq.synth.text(n, seed=len(datas)) if len(datas) % 3 else fuzzgen.structured(rng, n))
        blocks += -(-n // MiB4)
    assert not big
    round_trip(codec, oracle, tsq, datas, len(datas) & 1, rng)


def test_one_item_equals_the_single_call(codec, tsq):
    import torch
    host = tsq.synth.text(2 * MiB4 + 12345, seed=8)
    src = to_dev(host)
    for ext in (0, 1):
        single = codec.compress(src, ext)
        [batched] = codec.compress_batch([src], ext)
        assert torch.equal(single, batched)
        [back] = codec.decompress_batch([batched])
        assert torch.equal(back, codec.decompress(single)) and torch.equal(back, src)


def test_python_batches_views_and_copies(codec, tsq):
    import torch
    rng = np.random.default_rng(12)
    whole = to_dev(tsq.synth.text(3_000_000, seed=12))
    views = [whole[0:1000], whole[1000:500_000], whole[400_000:2_999_999]]       # one storage, overlapping inputs
    apart = [to_dev(tsq.synth.mix(int(n), seed=int(n))) for n in rng.integers(1, 200_000, 5)]
    for srcs in (views, apart):
        blobs = codec.compress_batch(srcs, 1)
        assert all(torch.equal(b, codec.compress(s, 1)) for s, b in zip(srcs, blobs))
        backs = codec.decompress_batch(blobs)
        assert all(torch.equal(b, s) for s, b in zip(srcs, backs))


def test_too_small_output_ranges_report_overflow(codec, oracle, tsq):
    rng = np.random.default_rng(5)
    datas = fuzz_items(rng, 40, tsq) + [tsq.synth.text(MiB4 + 100, seed=1)]
    want = [oracle.compress(d, 0) for d in datas]
    short = set(rng.choice(len(datas), 12, replace=False).tolist()) | {len(datas) - 1}
    caps = [max(16 + 6 * -(-d.size // MiB4), len(w) - int(rng.integers(1, 200))) if k in short else len(w) + int(rng.integers(0, 3))
            for k, (d, w) in enumerate(zip(datas, want))]
    arena, offs = arena_of(rng, datas)
    outs, out_size = fenced(rng, caps)
    items = [(o, d.size, a, cap) for o, d, a, cap in zip(offs, datas, outs, caps)]
    host, sizes, rc = call_compress(codec, to_dev(arena), items, 0, out_size)
    assert rc == ERR_OVERFLOW
    for k, w in enumerate(want):
        assert sizes[k] == len(w)
        if k in short:
            assert sizes[k] > caps[k]
        else:
            assert host[outs[k]:outs[k] + sizes[k]].tobytes() == w, f"item {k}"


def test_damaged_containers_among_healthy_ones(codec, oracle, tsq):
    import torch
    rng = np.random.default_rng(6)
    datas = fuzz_items(rng, 60, tsq) + [tsq.synth.mix(2 * MiB4 + 7, seed=3)]
    blobs = [np.frombuffer(oracle.compress(d, k & 1), dtype=np.uint8).copy() for k, d in enumerate(datas)]
    for k in range(0, len(blobs), 2):
        b = blobs[k]
        where = k % 6
        if where == 0:
            b[int(rng.integers(0, 10))] ^= 1 << int(rng.integers(0, 8))                # header (the total's low bytes: the oracle sizes its output by it)
        elif where == 2:
            b[16 + int(rng.integers(0, 3))] ^= 1 << int(rng.integers(0, 8))           # the first frame word
        else:
            for _ in range(int(rng.integers(1, 6))):                                  # stream bytes
                at = int(rng.integers(19, b.size))
                b[at] = rng.integers(0, 256)
    expect = [oracle.decompress(b) for b in blobs]
    arena, offs = arena_of(rng, blobs)
    d_in = to_dev(arena)
    outs, out_size = fenced(rng, [d.size for d in datas])
    items = [(o, b.size, a, d.size) for o, b, a, d in zip(offs, blobs, outs, datas)]
    host, sizes, status, rc = call_decompress(codec, d_in, items, out_size)
    refused = [k for k, w in enumerate(expect) if w is None]
    assert refused and rc != 0
    for k, w in enumerate(expect):
        assert (status[k] != 0) == (w is None), f"item {k}: status {status[k]}, the oracle {'refuses' if w is None else 'accepts'}"
        if w is not None:
            assert sizes[k] == len(w) and host[outs[k]:outs[k] + sizes[k]].tobytes() == w, f"item {k}"
    # the asynchronous form: all or nothing, the batch status is set
    nbs = [int.from_bytes(bytes(b[4:8]), "little") for b in blobs]
    ok = [k for k in range(len(blobs)) if 1 <= nbs[k] <= (blobs[k].size - 16) // 6]
    d_sizes = torch.zeros(len(ok), dtype=torch.int64, device="cuda")
    out = torch.empty(out_size, dtype=torch.uint8, device="cuda")
    codec.decompress_batch_async(d_in, [items[k] for k in ok], [nbs[k] for k in ok], out, d_sizes)
    torch.cuda.synchronize()
    assert any(expect[k] is None for k in ok) and codec.status() != 0
    with pytest.raises(tsq.TsqError) as e:
        codec.decompress_batch([to_dev(b) for b in blobs])
    assert [s != 0 for s in e.value.item_status] == [w is None for w in expect]
    assert all((r is None) == (w is None) for r, w in zip(e.value.results, expect))


def test_decode_variants_and_stall_retry(codec, oracle, tsq):
    import torch
    rng = np.random.default_rng(7)
    datas = [tsq.synth.text(int(n), seed=int(n)) for n in rng.integers(1, 3 * MiB4, 12)]
    blobs = [np.frombuffer(oracle.compress(d, 1), dtype=np.uint8) for d in datas]
    arena, offs = arena_of(rng, blobs)
    d_in = to_dev(arena)
    outs, out_size = fenced(rng, [d.size for d in datas])
    items = [(o, b.size, a, d.size) for o, b, a, d in zip(offs, blobs, outs, datas)]
    for v in (0, 3, 4, 5, 6):
        codec.set_variant(0, v)
        host, sizes, status, rc = call_decompress(codec, d_in, items, out_size)
        assert rc == 0 and not any(status), (v, codec.last_error())
        for k, d in enumerate(datas):
            assert np.array_equal(host[outs[k]:outs[k] + d.size], d), (v, k)
    # a wait limit of one poll: the several-workgroups decode stalls, the synchronous form decodes again on one workgroup per block
    codec.set_variant(0, 5)
    codec.set_decode_wait_limit(1)
    try:
        host, sizes, status, rc = call_decompress(codec, d_in, items, out_size)
        assert rc == 0 and not any(status)
        for k, d in enumerate(datas):
            assert np.array_equal(host[outs[k]:outs[k] + d.size], d), k
        nbs = [-(-d.size // MiB4) for d in datas]
        out = torch.empty(out_size, dtype=torch.uint8, device="cuda")
        codec.decompress_batch_async(d_in, items, nbs, out, torch.zeros(len(items), dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()
        assert codec.status() in (0, ERR_STALL)
    finally:
        codec.set_decode_wait_limit(1 << 24)


def test_two_async_batches_back_to_back(codec, oracle, tsq):
    import torch
    rng = np.random.default_rng(8)
    side = torch.cuda.Stream()                  # (a stream of its own: NULL would mean the context's stream to the library)
    sets = [fuzz_items(rng, 300, tsq), fuzz_items(rng, 200, tsq)]
    runs = []
    with torch.cuda.stream(side):
        for datas in sets:
            arena, offs = arena_of(rng, datas)
            d_in = to_dev(arena)
            caps = [tsq.batch_bound(d.size) for d in datas]
            outs, out_size = fenced(rng, caps)
            items = [(o, d.size, a, cap) for o, d, a, cap in zip(offs, datas, outs, caps)]
            out = torch.empty(out_size, dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(len(items), dtype=torch.int64, device="cuda")
            codec.compress_batch_async(d_in, items, 0, out, d_sizes)
            runs.append((datas, outs, out, d_sizes, d_in))
    side.synchronize()
    assert codec.status() == 0
    for datas, outs, out, d_sizes, _ in runs:
        host, sizes = out.cpu().numpy(), d_sizes.cpu().numpy()
        for k, d in enumerate(datas):
            assert host[outs[k]:outs[k] + int(sizes[k])].tobytes() == oracle.compress(d, 0), k


def test_three_async_batches_in_flight(codec, oracle, tsq):
    """Three batches on one stream with no synchronise between them: the descriptors go through a ring of two slots, so the third
    batch takes the slot of the first, once that one has finished.  Three items of 1000 bytes each."""
    import torch
    rng = np.random.default_rng(9)
    side = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(side):
        for b in range(3):
            datas = [tsq.synth.text(1000, seed=900 + 3 * b + k) for k in range(3)]
            arena, offs = arena_of(rng, datas)
            d_in = to_dev(arena)
            caps = [tsq.batch_bound(d.size) for d in datas]
            outs, out_size = fenced(rng, caps)
            out = torch.empty(out_size, dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(3, dtype=torch.int64, device="cuda")
            codec.compress_batch_async(d_in, [(o, d.size, a, cap) for o, d, a, cap in zip(offs, datas, outs, caps)], 0, out, d_sizes)
            runs.append((datas, outs, out, d_sizes, d_in))
    side.synchronize()
    assert codec.status() == 0
    for datas, outs, out, d_sizes, _ in runs:
        host, sizes = out.cpu().numpy(), d_sizes.cpu().numpy()
        for k, d in enumerate(datas):
            assert host[outs[k]:outs[k] + int(sizes[k])].tobytes() == oracle.compress(d, 0), k


def test_refused_arguments_write_nothing(codec, tsq):
    import torch
    src = to_dev(tsq.synth.text(10_000, seed=1))
    out = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(2, dtype=torch.int64, device="cuda")
    for items in ([(0, 5000, 0, 600), (5000, 5000, 599, 400)], [(0, 10_001, 0, 600)], [(0, 100, 0, 21)]):
        with pytest.raises(tsq.TsqError) as e:
            codec.compress_batch_async(src, items, 0, out, d_sizes)
        assert e.value.code == ERR_ARG
    codec.set_variant(1, 0)
    with pytest.raises(tsq.TsqError) as e:
        codec.compress_batch_async(src, [(0, 100, 0, 600)], 0, out, d_sizes)
    assert e.value.code == ERR_ARG
    torch.cuda.synchronize()
    assert not out.any() and not d_sizes.any()


def test_one_gib_batch(codec, oracle, tsq):
    """256 x 4 MiB of text, extensions on, every container and every byte compared"""
    import torch
    n_items = 256
    host = tsq.synth.text(n_items * MiB4, seed=31)
    src = to_dev(host)
    srcs = [src[k * MiB4:(k + 1) * MiB4] for k in range(n_items)]
    blobs = codec.compress_batch(srcs, 1)
    for k in range(n_items):
        stream = oracle.encode_block(host[k * MiB4:(k + 1) * MiB4], 1)
        want = b"TSQ1" + (1).to_bytes(4, "little") + MiB4.to_bytes(8, "little") + (len(stream) | 1 << 23).to_bytes(3, "little") + stream
        assert blobs[k].cpu().numpy().tobytes() == want, k
    backs = codec.decompress_batch(blobs)
    assert all(torch.equal(b, s) for b, s in zip(backs, srcs))
