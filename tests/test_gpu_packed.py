"""GPU tests of packed batches (tsqa_compress_batch_packed*, tsqa_decompress_batch_packed_async): the offsets and sizes are
tsqa_plan_packed of the oracle's container lengths, every container is the oracle's container of that item alone, every round trip
gives the item; outputs are sentinel-filled, and the padding between containers, everything behind the bytes used and every guard
byte between decoded items must stay as it was."""
import ctypes as C

import numpy as np
import pytest

import packedgen as pg
from turbosqueeze_amd.api import _batch_array

pytestmark = pytest.mark.gpu

MiB4 = 1 << 22
ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = 3, 4, 6


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


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (the pattern repeats every 251 bytes)"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


def small_item(rng, k, n, tsq):
    return pg.small_item(rng, k, n)


def arena_of(rng, datas):
    """the items in one host arena behind non-zero filler gaps of 0..47 bytes -> (arena, offsets)"""
    at, offs = 0, []
    for d in datas:
        at += int(rng.integers(0, 48))
        offs.append(at)
        at += d.size
    arena = rng.integers(1, 256, at + 64, dtype=np.uint8)
    for d, o in zip(datas, offs):
        arena[o:o + d.size] = d
    return arena, offs


class Batch:
    """a seeded batch on the device, with the oracle's containers of its items (made once per ext, shared by the tests)"""

    def __init__(self, datas, seed, oracle):
        self.datas, self.oracle, self._want = datas, oracle, {}
        arena, self.offs = arena_of(np.random.default_rng(seed), datas)
        self.d_in = to_dev(arena)
        self.items = [(o, d.size, 0, 0) for o, d in zip(self.offs, datas)]

    def want(self, ext):
        if ext not in self._want:
            self._want[ext] = [self.oracle.compress(d, ext, threads=8 if d.size > MiB4 else 1) for d in self.datas]
        return self._want[ext]


@pytest.fixture(scope="module")
def mixed(tsq, oracle):
    rng = np.random.default_rng(21)
    sizes = [1, 2, 15, 16, 17, 699, 4096, 65535, MiB4 + 1]
    datas = [tsq.synth.text(n, seed=n) if k % 2 else tsq.synth.mix(n, seed=n) for k, n in enumerate(sizes)]
    datas += [small_item(rng, k, int(rng.integers(1, 20_000)), tsq) for k in range(30)]
    return Batch([datas[i] for i in rng.permutation(len(datas))], 22, oracle)


def call_packed(codec, batch, ext, align, out_size, buf_size=None):
    """tsqa_compress_batch_packed into the first out_size bytes of a sentinel-filled buffer -> (buffer, guard, offsets, sizes, rc)"""
    guard = sentinel(buf_size or out_size)
    out = to_dev(guard)
    n = len(batch.items)
    offsets, sizes = (C.c_uint64 * (n + 1))(), (C.c_uint64 * n)()
    rc = codec.L.tsqa_compress_batch_packed(codec.h, batch.d_in.data_ptr(), batch.d_in.numel(), _batch_array(batch.items), n, ext, align,
                                            out.data_ptr(), out_size, offsets, sizes, codec._stream())
    return out.cpu().numpy(), guard, [int(x) for x in offsets], [int(x) for x in sizes], rc


def check_layout(tsq, host, guard, want, align, offsets, sizes, complete=None):
    """the tables against tsqa_plan_packed of the oracle's lengths; the first `complete` containers (all by default) exact; every
    other byte of the buffer as the sentinel left it"""
    assert sizes == [len(w) for w in want]
    assert offsets == tsq.plan_packed(sizes, align)
    untouched = np.ones(host.size, dtype=bool)
    for k, w in enumerate(want[:complete]):
        assert host[offsets[k]:offsets[k] + sizes[k]].tobytes() == w, f"item {k} ({sizes[k]} B at {offsets[k]}): not the oracle's container"
        untouched[offsets[k]:offsets[k] + sizes[k]] = False
    assert np.array_equal(host[untouched], guard[untouched]), "bytes outside the containers were written"


def round_trip(codec, batch, host, offsets, sizes):
    """the containers where they lie in the packed arena, back to the items (tsqa_decompress_batch)"""
    at, items = 0, []
    for o, n, d in zip(offsets, sizes, batch.datas):
        items.append((o, n, at, d.size))
        at += d.size
    out = to_dev(sentinel(at + 64))
    got, status = (C.c_uint64 * len(items))(), (C.c_int32 * len(items))()
    rc = codec.L.tsqa_decompress_batch(codec.h, to_dev(host).data_ptr(), host.size, _batch_array(items), len(items), out.data_ptr(), at + 64,
                                       got, status, codec._stream())
    assert rc == 0 and not any(status), codec.last_error()
    back = out.cpu().numpy()
    for k, (d, (_, _, a, _)) in enumerate(zip(batch.datas, items)):
        assert int(got[k]) == d.size and np.array_equal(back[a:a + d.size], d), f"item {k}: round trip"
    assert np.array_equal(back[at:], sentinel(at + 64)[at:])


@pytest.mark.parametrize("align", [1, 16, 256])
@pytest.mark.parametrize("ext", [0, 1])
def test_layout_and_exactness(codec, tsq, mixed, ext, align):
    want = mixed.want(ext)
    used = tsq.plan_packed([len(w) for w in want], align)[-1]
    host, guard, offsets, sizes, rc = call_packed(codec, mixed, ext, align, used + 5000)
    assert rc == 0, codec.last_error()
    assert offsets[-1] == used
    check_layout(tsq, host, guard, want, align, offsets, sizes)
    round_trip(codec, mixed, host, offsets, sizes)


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def seam(tsq, oracle, cus):
    """packedgen.seam_batch for the device's launch budget -> (batch, a_at, b_at, each item's first block)"""
    datas, a_at, b_at = pg.seam_batch(cus)
    batch = Batch(datas, 24, oracle)
    caps = [tsq.batch_bound(d.size) for d in datas]
    first = tsq.plan_batch([(o, d.size, sum(caps[:k]), caps[k]) for k, (o, d) in enumerate(zip(batch.offs, datas))], batch.d_in.numel(), sum(caps))
    return batch, a_at, b_at, first


def test_launch_seams(codec, tsq, seam, cus):
    """Launches of 2 x CUs blocks: item A's three blocks straddle the first seam (it continues into the second launch with its start
    and running frame offset carried), item B's two blocks end a launch exactly (the next item begins one and takes its start from
    what the launch before left).

    Not reached here: an item of more than 2 x CUs blocks, whose middle launches hold that one item alone, neither begun nor completed
    in them (its input alone would be over 2 GiB).  By the kernel's code that launch reads its start from d_offsets[i0], adds an
    exclusive sum of nothing, and carries the frame offset in run_at, the two carries that items A and B check one at a time."""
    budget = 2 * cus
    batch, a_at, b_at, first = seam
    assert first[a_at] < budget < first[a_at + 1] == first[a_at] + 3, "item A does not straddle the first launch seam"
    assert first[b_at + 1] == 2 * budget and first[b_at + 1] - first[b_at] == 2, "item B does not end the second launch"
    assert first[-1] > 2 * budget and b_at + 1 < len(batch.datas)
    want = batch.want(1)
    used = tsq.plan_packed([len(w) for w in want], 16)[-1]
    host, guard, offsets, sizes, rc = call_packed(codec, batch, 1, 16, used + 999)
    assert rc == 0, codec.last_error()
    check_layout(tsq, host, guard, want, 16, offsets, sizes)
    round_trip(codec, batch, host, offsets, sizes)


def check_offsets(tsq, want, align, offsets, sizes):
    """the first item whose place differs from tsqa_plan_packed of the oracle's lengths, with the difference in hex: a lost or doubled
    high half of the scan shows as a multiple of 1 << 24"""
    plan = tsq.plan_packed([len(w) for w in want], align)
    for i, (got, exp) in enumerate(zip(offsets, plan)):
        assert got == exp, (f"offsets[{i}] is {got:#x}, the plan says {exp:#x}: off by {'-' if got < exp else '+'}{abs(got - exp):#x} "
                            f"({abs(got - exp) / (1 << 24):g} x 2^24)")
    for i, (got, w) in enumerate(zip(sizes, want)):
        assert got == len(w), f"sizes[{i}] is {got}, the oracle's container has {len(w)} bytes"


def test_scan_carries_above_2_to_24(codec, tsq, oracle, cus):
    """Four containers of more than 2^24 bytes among tiny ones (packedgen.carry_batch): the place-making scan's high half, the
    (hi << 24) + lo recombination, the carry from one 256-item iteration to the next and the carry through d_offsets[i0] from one
    launch to the next all have something other than zero to carry.

    Not reached here, as in test_launch_seams: an item of more than 2 x CUs blocks (over 2 GiB of input), and an arena past 4 GiB.
    By the code every offset is a 64-bit value from the scan on; no test goes there."""
    cb = pg.carry_batch(cus)
    batch = Batch(list(cb.datas), 36, oracle)
    pg.carry_reach(cb, cus, {ext: [len(w) for w in batch.want(ext)] for ext in (0, 1)})        # (fails, never skips)
    for ext in (0, 1):
        want = batch.want(ext)
        for align in (16, 4096):
            used = tsq.plan_packed([len(w) for w in want], align)[-1]
            host, guard, offsets, sizes, rc = call_packed(codec, batch, ext, align, used + 4096)
            assert rc == 0, codec.last_error()
            check_offsets(tsq, want, align, offsets, sizes)
            check_layout(tsq, host, guard, want, align, offsets, sizes)
            round_trip(codec, batch, host, offsets, sizes)


def test_last_launch_of_256_257_and_1_items(codec, tsq, oracle, cus):
    """the place-making loop walks a launch's items 256 at a time: a last launch of exactly one full iteration, of one valid lane in
    a second iteration, and of one item"""
    batches = pg.loop_edge_batches(cus)
    assert [pg.last_launch_items(datas, cus) for datas in batches] == [256, 257, 1]
    for k, datas in enumerate(batches):
        batch = Batch(list(datas), 37 + k, oracle)
        want = batch.want(1)
        for align in (1, 256):
            used = tsq.plan_packed([len(w) for w in want], align)[-1]
            host, guard, offsets, sizes, rc = call_packed(codec, batch, 1, align, used + 300)
            assert rc == 0, codec.last_error()
            check_offsets(tsq, want, align, offsets, sizes)
            check_layout(tsq, host, guard, want, align, offsets, sizes)
            round_trip(codec, batch, host, offsets, sizes)


@pytest.mark.parametrize("align", [2, 16, 4096])
def test_alignment_residues(codec, tsq, oracle, align):
    """containers whose size is an exact multiple of align (no padding behind them), 1 past one (align - 1 bytes) and 1 short (1)"""
    batch = Batch(list(pg.alignment_batch(align)), 40 + align, oracle)
    want = batch.want(1)
    sizes = [len(w) for w in want]
    assert pg.residues_present(sizes, align) == set(pg.RESIDUES)
    host, guard, offsets, sizes, rc = call_packed(codec, batch, 1, align, tsq.plan_packed(sizes, align)[-1] + 2 * align)
    assert rc == 0, codec.last_error()
    check_offsets(tsq, want, align, offsets, sizes)
    check_layout(tsq, host, guard, want, align, offsets, sizes)


def test_overflow_keeps_tables_and_fitting_items(codec, tsq, mixed):
    ext, align = 1, 16
    want = mixed.want(ext)
    roomy = tsq.plan_packed([len(w) for w in want], align)
    k = len(want) // 2
    out_size = roomy[k] + 7
    host, guard, offsets, sizes, rc = call_packed(codec, mixed, ext, align, out_size, buf_size=roomy[-1] + 4096)
    assert rc == ERR_OVERFLOW
    assert offsets == roomy
    # the items before k exact, and nothing else written: not item k's place (its header does not fit), nothing at or past out_size
    check_layout(tsq, host, guard, want, align, offsets, sizes, complete=k)
    host, guard, offsets, sizes, rc = call_packed(codec, mixed, ext, align, roomy[-1], buf_size=roomy[-1] + 4096)
    assert rc == 0, codec.last_error()
    check_layout(tsq, host, guard, want, align, offsets, sizes)


def first_difference(host, expected):
    bad = np.flatnonzero(host != expected)
    return f"{bad.size} bytes differ, the first at {int(bad[0])}: {int(host[bad[0]])} for {int(expected[bad[0]])}" if bad.size else "equal"


@pytest.mark.parametrize("placing", ["inside_a_launch", "across_a_launch_seam"])
def test_overflow_cut_at_every_seam(codec, tsq, oracle, seam, cus, placing):
    """out_size cut at every place where batch_pack_scan_packed_kernel decides (packedgen.cut_points), around a three-block item of
    text and around a two-block item: inside one launch, and with the three-block item across the first launch seam, where its
    later frames are placed from run_at[i] and d_offsets[i0].  Whatever is cut: TSQA_ERR_OVERFLOW, both tables complete, and the
    buffer is the sentinel overlaid with exactly the headers and frames that end at or before out_size (packedgen.fitting_image) --
    over the whole buffer, so nothing at or past out_size and no padding byte may change."""
    if placing == "inside_a_launch":
        datas, a_at, b_at = pg.inside_batch()
        batch = Batch(datas, 38, oracle)
        assert len(pg.launches([d.size for d in datas], cus)) == 1
    else:
        batch, a_at, b_at, first = seam
        assert first[a_at] < 2 * cus < first[a_at + 1] == first[a_at] + 3, "item A does not straddle the first launch seam"
    ext = 1
    want = batch.want(ext)
    lengths = [len(w) for w in want]
    for k in (a_at, b_at):
        align = pg.align_with_padding(lengths, k)
        roomy = tsq.plan_packed(lengths, align)
        cuts = pg.cut_points(want, roomy, lengths, k)
        assert len(set(cuts.values())) == 7
        for name, cut in cuts.items():
            host, guard, offsets, sizes, rc = call_packed(codec, batch, ext, align, cut, buf_size=roomy[-1] + 4096)
            assert rc == ERR_OVERFLOW, f"{name} (out_size {cut}, item {k}): rc {rc}"
            assert offsets == roomy and sizes == lengths, f"{name} (out_size {cut}, item {k}): the tables are not the roomy plan's"
            expected = guard.copy()
            for lo, piece in pg.fitting_image(want, roomy, cut):
                expected[lo:lo + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
            assert np.array_equal(host, expected), f"{name} (out_size {cut}, item {k} at {roomy[k]}): {first_difference(host, expected)}"
        host, guard, offsets, sizes, rc = call_packed(codec, batch, ext, align, roomy[-1], buf_size=roomy[-1] + 4096)
        assert rc == 0, codec.last_error()
        check_layout(tsq, host, guard, want, align, offsets, sizes)


def fenced_outputs(rng, lengths):
    at, outs = 0, []
    for ln in lengths:
        at += int(rng.integers(1, 48))
        outs.append(at)
        at += int(ln)
    return outs, at + 64


def test_compress_then_decompress_without_a_host_read(codec, tsq, mixed, oracle):
    """two chains compress_batch_packed_async -> decompress_batch_packed_async enqueued back to back on one stream; the second
    call of each chain takes the containers' places from the tables the first leaves on the device"""
    import torch
    rng = np.random.default_rng(25)
    other = Batch([small_item(rng, k, int(rng.integers(1, 9000)), tsq) for k in range(70)] + [tsq.synth.text(MiB4 + 77, seed=9)], 26, oracle)
    codec.set_variant(0, 4)                      # one workgroup per block waits for nobody: a busy GPU cannot show as TSQA_ERR_STALL
    side = torch.cuda.Stream()
    runs = []
    with torch.cuda.stream(side):
        for batch, ext, align in ((mixed, 1, 16), (other, 0, 256)):
            n = len(batch.datas)
            lengths = [d.size for d in batch.datas]
            packed = torch.empty(sum(tsq.batch_bound(x) + align for x in lengths), dtype=torch.uint8, device="cuda")
            d_offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            d_sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
            outs, out_size = fenced_outputs(rng, lengths)
            guard = sentinel(out_size)
            out = to_dev(guard)
            d_out_sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
            codec.compress_batch_packed_async(batch.d_in, batch.items, ext, align, packed, d_offsets, d_sizes)
            codec.decompress_batch_packed_async(packed, d_offsets, d_sizes, list(zip(outs, lengths)), [-(-x // MiB4) for x in lengths], out, d_out_sizes)
            runs.append((batch, ext, align, packed, d_offsets, d_sizes, outs, guard, out, d_out_sizes))
    side.synchronize()
    assert codec.status() == 0
    for batch, ext, align, packed, d_offsets, d_sizes, outs, guard, out, d_out_sizes in runs:
        want = batch.want(ext)
        offsets, sizes = d_offsets.cpu().tolist(), d_sizes.cpu().tolist()
        assert sizes == [len(w) for w in want] and offsets == tsq.plan_packed(sizes, align)
        arena = packed.cpu().numpy()
        assert all(arena[o:o + n].tobytes() == w for o, n, w in zip(offsets, sizes, want))
        assert d_out_sizes.cpu().tolist() == [d.size for d in batch.datas]
        back = out.cpu().numpy()
        untouched = np.ones(back.size, dtype=bool)
        for k, (d, a) in enumerate(zip(batch.datas, outs)):
            assert np.array_equal(back[a:a + d.size], d), f"item {k}"
            untouched[a:a + d.size] = False
        assert np.array_equal(back[untouched], guard[untouched]), "guard bytes between the outputs changed"


def test_larger_batch_enqueued_behind_a_smaller_one(tsq, oracle):
    """a fresh context's per-item tables hold 256 items: a chain of 300 items enqueued behind a chain of 40 grows them while the
    first chain may still be running on the caller's stream, which must not pull them from under it.

    This exercises the growth behind an enqueued chain; it does not prove the wait.  The first chain is short and the host prepares
    the second batch between the two enqueues, so the tables are rarely freed under a running kernel, and a wait for the
    context's own stream alone would very likely pass too."""
    import torch
    rng = np.random.default_rng(29)
    fresh = tsq.DeviceCodec(0)
    fresh.set_variant(0, 4)
    side = torch.cuda.Stream()
    runs = []
    try:
        with torch.cuda.stream(side):
            for count in (40, 300):
                batch = Batch([small_item(rng, k, int(rng.integers(1, 3000)), tsq) for k in range(count)], 30 + count, oracle)
                lengths = [d.size for d in batch.datas]
                packed = torch.empty(sum(tsq.batch_bound(x) + 16 for x in lengths), dtype=torch.uint8, device="cuda")
                d_offsets = torch.full((count + 1,), -1, dtype=torch.int64, device="cuda")
                d_sizes = torch.full((count,), -1, dtype=torch.int64, device="cuda")
                outs, out_size = fenced_outputs(rng, lengths)
                out = to_dev(sentinel(out_size))
                d_out_sizes = torch.full((count,), -1, dtype=torch.int64, device="cuda")
                fresh.compress_batch_packed_async(batch.d_in, batch.items, 1, 16, packed, d_offsets, d_sizes)
                fresh.decompress_batch_packed_async(packed, d_offsets, d_sizes, list(zip(outs, lengths)), [1] * count, out, d_out_sizes)
                runs.append((batch, packed, d_offsets, d_sizes, outs, out, d_out_sizes))
        side.synchronize()
        assert fresh.status() == 0
    finally:
        fresh.close()
    for batch, packed, d_offsets, d_sizes, outs, out, d_out_sizes in runs:
        want = batch.want(1)
        offsets, sizes = d_offsets.cpu().tolist(), d_sizes.cpu().tolist()
        assert sizes == [len(w) for w in want] and offsets == tsq.plan_packed(sizes, 16)
        arena, back = packed.cpu().numpy(), out.cpu().numpy()
        assert all(arena[o:o + n].tobytes() == w for o, n, w in zip(offsets, sizes, want))
        assert d_out_sizes.cpu().tolist() == [d.size for d in batch.datas]
        assert all(np.array_equal(back[a:a + d.size], d) for d, a in zip(batch.datas, outs))


def test_device_tables_are_not_trusted(codec, tsq, mixed):
    import torch
    ext, align = 1, 16
    want = mixed.want(ext)
    host, guard, offsets, sizes, rc = call_packed(codec, mixed, ext, align, tsq.plan_packed([len(w) for w in want], align)[-1])
    assert rc == 0
    arena = to_dev(host)                          # exactly the bytes used: the last container ends the allocation's payload
    n = len(want)
    lengths = [d.size for d in mixed.datas]
    blocks = [-(-x // MiB4) for x in lengths]
    outs, out_size = fenced_outputs(np.random.default_rng(27), lengths)
    guard = sentinel(out_size)
    tiny = min(range(n), key=lambda i: sizes[i])
    assert sizes[tiny] < 16 + 6 * 2
    codec.set_variant(0, 4)

    def run(offsets, sizes, blocks):
        out = to_dev(guard)
        d_out_sizes = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        wrap = lambda xs: torch.tensor([x - (1 << 64) if x >= 1 << 63 else x for x in xs], dtype=torch.int64, device="cuda")
        codec.decompress_batch_packed_async(arena, wrap(offsets), wrap(sizes), list(zip(outs, lengths)), blocks, out, d_out_sizes)
        torch.cuda.synchronize()
        back = out.cpu().numpy()
        untouched = np.ones(back.size, dtype=bool)
        for a, ln in zip(outs, lengths):
            untouched[a:a + ln] = False
        assert np.array_equal(back[untouched], guard[untouched]), "bytes outside the output ranges were written"
        return codec.status(), d_out_sizes.cpu().tolist(), back

    status, got, back = run(offsets, sizes, blocks)
    assert status == 0 and got == lengths and all(np.array_equal(back[a:a + d.size], d) for a, d in zip(outs, mixed.datas))
    j = n // 3
    cases = {
        "the last container ends one byte past the arena": (offsets, sizes[:-1] + [sizes[-1] + 1], blocks, n - 1),
        "an offset + size past the arena": (offsets[:j] + [arena.numel() - 3] + offsets[j + 1:], sizes, blocks, j),
        "an offset near 2^64": (offsets[:j] + [(1 << 64) - 8] + offsets[j + 1:], sizes, blocks, j),
        "a size near 2^64": (offsets, sizes[:j] + [(1 << 64) - 8] + sizes[j + 1:], blocks, j),
        "a size of 7": (offsets, sizes[:j] + [7] + sizes[j + 1:], blocks, j),
        "more blocks than the container can hold": (offsets, sizes, blocks[:tiny] + [2] + blocks[tiny + 1:], tiny),
    }
    for name, (offs, szs, nbs, item) in cases.items():
        status, got, _ = run(offs, szs, nbs)
        assert status == ERR_FORMAT and got[item] == 0, f"{name}: status {status}, size {got[item]}"


def test_refused_arguments_write_nothing(codec, tsq):
    import torch
    src = to_dev(tsq.synth.text(10_000, seed=1))
    out = torch.zeros(4000, dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(3, dtype=torch.int64, device="cuda")
    d_sizes = torch.zeros(2, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    good = [(0, 5000, 0, 0), (5000, 5000, 0, 0)]

    def call(items=good, n_items=2, align=16, out_size=4000, offsets=d_offsets.data_ptr(), sizes=d_sizes.data_ptr()):
        return codec.L.tsqa_compress_batch_packed_async(codec.h, src.data_ptr(), src.numel(), _batch_array(items), n_items, 0, align, out.data_ptr(),
                                                        out_size, offsets, sizes, status.data_ptr(), codec._stream())

    for align in (0, 3, 24, 8192):
        assert call(align=align) == ERR_ARG
    assert call(n_items=0) == ERR_ARG
    assert call(items=[(0, 5000, 0, 0), (5000, 0, 0, 0)]) == ERR_ARG            # an empty item
    assert call(items=[(0, 5000, 0, 0), (5001, 5000, 0, 0)]) == ERR_ARG         # an input range past in_size
    assert call(offsets=None) == ERR_ARG and call(sizes=None) == ERR_ARG
    assert call(out_size=15) == ERR_ARG
    codec.set_variant(1, 0)
    assert call() == ERR_ARG
    host_offsets, host_sizes = (C.c_uint64 * 3)(), (C.c_uint64 * 2)()
    assert codec.L.tsqa_compress_batch_packed(codec.h, src.data_ptr(), src.numel(), _batch_array(good), 2, 0, 16, out.data_ptr(), 4000,
                                              host_offsets, host_sizes, codec._stream()) == ERR_ARG
    with pytest.raises(tsq.TsqError) as e:
        codec.compress_batch_packed([src[:100]], 0)
    assert e.value.code == ERR_ARG
    codec.set_variant(0, 0)
    with pytest.raises(tsq.TsqError) as e:
        codec.compress_batch_packed([src[:100]], 0, align=48)
    assert e.value.code == ERR_ARG
    torch.cuda.synchronize()
    assert not out.any() and not d_offsets.any() and not d_sizes.any() and not status.any()
    assert not any(host_offsets) and not any(host_sizes)


def test_python_packed_batches(codec, tsq):
    import torch
    rng = np.random.default_rng(28)
    whole = to_dev(tsq.synth.text(3_000_000, seed=12))
    views = [whole[0:1000], whole[1000:500_000], whole[400_000:2_999_999]]       # one storage, overlapping inputs
    apart = [to_dev(tsq.synth.mix(int(n), seed=int(n))) for n in rng.integers(1, 200_000, 5)]
    for srcs in (views, apart):
        pb = codec.compress_batch_packed(srcs, 1)
        assert len(pb.offsets) == len(srcs) + 1 and pb.arena.numel() == pb.offsets[-1]
        assert pb.offsets == tsq.plan_packed(pb.sizes, 16) and pb.lengths == [s.numel() for s in srcs]
        assert all(torch.equal(v, codec.compress(s, 1)) for s, v in zip(srcs, pb.views))
        assert all(torch.equal(b, s) for s, b in zip(srcs, pb.decompress()))
        index = pb.index()
        for item, s in enumerate(srcs):
            off = s.numel() // 3
            ln = min(1000, s.numel() - off)
            assert torch.equal(index.read(item, off, ln), s[off:off + ln])
        index.close()
        # exactly the bytes used is enough; one byte less is not, and says what a retry needs
        again = codec.compress_batch_packed(srcs, 1, out=torch.empty(pb.offsets[-1], dtype=torch.uint8, device="cuda"))
        assert again.offsets == pb.offsets and again.sizes == pb.sizes and again.arena.numel() == pb.offsets[-1]
        assert all(torch.equal(a, b) for a, b in zip(again.views, pb.views))      # (the padding between them is never written)
        with pytest.raises(tsq.TsqError) as e:
            codec.compress_batch_packed(srcs, 1, out=torch.empty(pb.offsets[-1] - 1, dtype=torch.uint8, device="cuda"))
        assert e.value.code == ERR_OVERFLOW and e.value.needed == pb.offsets[-1]
