"""CPU-only: the record-read entry points are exported, and tsqa_plan_item_ranges (host code) agrees with a brute-force Python
model -- on layouts taken from containers made by the oracle (walked with tsqa_walk_frames) and on hand-made layouts with short
blocks in the middle: every byte of every range is covered by exactly one range item, the items are sorted by (block, lo), the
groups partition them, and every refusal leaves the output arrays untouched."""
import ctypes as C

import numpy as np
import pytest

import turbosqueeze_amd as tsq

MiB4 = 1 << 22
SYMBOLS = ["tsqa_index_create_batch", "tsqa_index_items", "tsqa_index_item_total", "tsqa_index_item_status", "tsqa_plan_item_ranges",
           "tsqa_decompress_item_ranges_async", "tsqa_decompress_item_ranges"]


def walked_lens(blob: bytes):
    """the output lengths of a container's blocks (tsqa_walk_frames)"""
    L = tsq.lib()
    cap = len(blob) // 6 + 1
    frame_at, sizes, ext, out_len = (np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32))
    nb, total = C.c_uint32(0), C.c_uint64(0)
    buf = C.create_string_buffer(blob, len(blob))
    assert L.tsqa_walk_frames(buf, len(blob), cap, frame_at.ctypes.data, sizes.ctypes.data, ext.ctypes.data, out_len.ctypes.data,
                              C.byref(nb), C.byref(total)) == 0
    lens = [int(out_len[b]) for b in range(nb.value)]
    assert sum(lens) == total.value
    return lens


def layout(items_lens):
    """per item the output lengths of its blocks ([] = a refused item) -> (out_start, item_first_block)"""
    starts, first = [0], [0]
    for lens in items_lens:
        for ln in lens:
            starts.append(starts[-1] + ln)
        first.append(len(starts) - 1)
    return starts, first


def refused(starts, first, ranges, out_cap):
    """the brute-force model's verdict: must tsqa_plan_item_ranges refuse these (item, offset, length, out_at) ranges?"""
    dst = []
    for item, off, ln, at in ranges:
        if item >= len(first) - 1:
            return True
        if first[item] == first[item + 1]:
            return True                                     # a refused item, whatever the range
        total = starts[first[item + 1]] - starts[first[item]]
        if off + ln > total:
            return True
        if ln == 0:
            continue
        if at + ln > out_cap:
            return True
        dst.append((at, ln))
    dst.sort()
    return any(a[0] + a[1] > b[0] for a, b in zip(dst, dst[1:]))


def plan(starts, first, ranges, out_cap, **caps):
    try:
        return tsq.plan_item_ranges(starts, first, ranges, out_cap, **caps)
    except tsq.TsqError as e:
        assert e.code == 3
        return None


def check(starts, first, ranges, out_cap):
    """plan, and hold the answer against the model byte by byte"""
    got = plan(starts, first, ranges, out_cap)
    if refused(starts, first, ranges, out_cap):
        assert got is None, f"{ranges} should have been refused"
        return None
    assert got is not None, f"{ranges} should have been planned"
    items, groups = got
    # every byte of every range is covered by exactly one item: the multiset of (source byte, destination byte) pairs, kept as
    # runs (absolute source start, length, destination start) cut at the block edges
    want = []
    for item, off, ln, at in ranges:
        a, e = starts[first[item]] + off, starts[first[item]] + off + ln
        for b in range(len(starts) - 1):
            lo, hi = max(a, starts[b]), min(e, starts[b + 1])
            if lo < hi:
                want.append((b, lo - starts[b], hi - starts[b], at + lo - a))
    assert sorted(items) == sorted(want)
    assert all(lo < hi and hi <= starts[b + 1] - starts[b] for b, lo, hi, _ in items)
    # sorted by (block, lo); the groups partition the items, one per touched block, hi = the group's largest hi
    assert [(b, lo) for b, lo, _, _ in items] == sorted((b, lo) for b, lo, _, _ in items)
    at = 0
    for block, f, count, hi in groups:
        assert f == at and count > 0
        mine = items[f:f + count]
        assert all(b == block for b, *_ in mine) and hi == max(h for _, _, h, _ in mine)
        at += count
    assert at == len(items)
    assert [g[0] for g in groups] == sorted({b for b, *_ in items})
    return items, groups


def test_symbols_exported():
    L = tsq.lib()
    assert all(hasattr(L, n) for n in SYMBOLS)
    assert C.sizeof(tsq.ItemRange) == 32 and C.sizeof(tsq.BlockGroup) == 16 and C.sizeof(tsq.RangeItem) == 24


def test_python_surface_exists():
    assert callable(tsq.DeviceCodec.index_batch) and callable(tsq.plan_item_ranges)
    for m in ("item_total", "item_status", "read", "read_many", "read_many_async", "read_items_into", "close"):
        assert callable(getattr(tsq.BatchIndex, m))
    assert issubclass(tsq.BatchIndex, tsq.RangeIndex)


def test_calls_without_context_are_argument_errors():
    L = tsq.lib()
    out = C.c_void_p(1)
    blob = C.create_string_buffer(b"TSQ1" + bytes(12))
    items = (tsq.BatchItem * 1)(tsq.BatchItem(0, 16, 0, 0))
    assert L.tsqa_index_create_batch(None, blob, 16, items, 1, C.byref(out), None) == 3
    assert not out.value
    assert L.tsqa_index_create_batch(None, blob, 16, items, 1, None, None) == 3
    assert L.tsqa_index_items(None) == 0 and L.tsqa_index_item_total(None, 0) == 0 and L.tsqa_index_item_status(None, 0) == 3
    rr = (tsq.ItemRange * 1)(tsq.ItemRange(0, 0, 0, 1, 0))
    assert L.tsqa_decompress_item_ranges(None, None, rr, 1, None, 1, None) == 3
    assert L.tsqa_decompress_item_ranges_async(None, None, rr, 1, None, 1, None, None) == 3


@pytest.fixture(scope="module")
def oracle_layout(oracle):
    """items of 1 byte, 4 MiB exactly, 4 MiB + 1 and several blocks: their block lengths as the oracle's containers state them"""
    sizes = [1, MiB4, MiB4 + 1, 3 * MiB4 + 5000, 70_000]
    items_lens = []
    for k, n in enumerate(sizes):
        data = tsq.synth.text(n, seed=40 + k) if k % 2 == 0 else tsq.synth.mix(n, seed=40 + k)
        items_lens.append(walked_lens(oracle.compress(data, k & 1, threads=4)))
    assert [sum(x) for x in items_lens] == sizes and [len(x) for x in items_lens] == [1, 1, 2, 4, 1]
    return sizes, layout(items_lens)


def test_plan_on_oracle_containers(oracle_layout):
    sizes, (starts, first) = oracle_layout
    cap = 1 << 26
    cases = [
        [(0, 0, 1, 0)],                                                  # the one-byte item
        [(1, 0, MiB4, 0)], [(1, MiB4 - 1, 1, 5)],                        # a block exactly
        [(2, MiB4 - 1, 2, 0)], [(2, MiB4, 1, 0)], [(2, 0, MiB4 + 1, 3)],     # 4 MiB + 1: the one-byte last block
        [(3, MiB4 - 10, 2 * MiB4 + 20, 0)], [(3, 0, sizes[3], 0)],       # across two and three block edges
        [(k, 0, n, sum(sizes[:k])) for k, n in enumerate(sizes)],        # every item whole
        [(4, 100, 64, 0), (4, 50, 64, 64), (4, 100, 64, 128), (4, 0, 70_000, 200)],   # many in one block
        [(4, 10, 0, 0), (0, 1, 0, cap), (3, sizes[3], 0, 0)],            # zero-length ranges give nothing
    ]
    for ranges in cases:
        assert check(starts, first, ranges, cap) is not None
    assert check(starts, first, [(4, 10, 0, 0)], cap) == ([], [])
    # two ranges over the same source bytes both survive
    items, groups = check(starts, first, [(3, MiB4 + 5, 100, 0), (3, MiB4 + 5, 100, 100), (3, MiB4 + 50, 10, 200)], cap)
    b = first[3] + 1
    assert items == [(b, 5, 105, 0), (b, 5, 105, 100), (b, 50, 60, 200)] and groups == [(b, 0, 3, 105)]
    # a group's hi is its largest, not its last
    items, groups = check(starts, first, [(1, 0, 5000, 0), (1, 100, 10, 6000)], cap)
    assert groups == [(first[1], 0, 2, 5000)]
    # random sets
    rng = np.random.default_rng(3)
    for _ in range(200):
        ranges, at = [], int(rng.integers(0, 50))
        for _ in range(int(rng.integers(1, 12))):
            i = int(rng.integers(0, len(sizes)))
            off = int(rng.integers(0, sizes[i]))
            ln = int(rng.integers(0, sizes[i] - off + 1)) if rng.random() < 0.2 else int(rng.integers(0, min(500, sizes[i] - off) + 1))
            ranges.append((i, off, ln, at))
            at += ln + int(rng.integers(0, 20))
        check(starts, first, ranges, cap)


def test_plan_with_short_middle_blocks_and_refused_items():
    # short blocks in the middle (one of them empty), as test_range_cpu.py::test_plan_with_short_middle_blocks; items 1 and 4 refused
    items_lens = [[MiB4, 1000, 0, 37, MiB4], [], [5], [1 << 20, 17], [], [MiB4]]
    starts, first = layout(items_lens)
    totals = [sum(x) for x in items_lens]
    cap = 4 * starts[-1]
    rng = np.random.default_rng(7)
    n_refused = 0
    for _ in range(400):
        ranges, at = [], int(rng.integers(0, 50))
        for _ in range(int(rng.integers(1, 8))):
            i = int(rng.choice([0, 2, 3, 5]))
            off = int(rng.integers(0, totals[i]))
            ln = int(rng.integers(0, totals[i] - off + 1)) if rng.random() < 0.3 else int(rng.integers(0, min(3000, totals[i] - off) + 1))
            ranges.append((i, off, ln, at))
            at += ln + int(rng.integers(0, 20))
        dice = rng.random()
        if dice < 0.05:
            ranges.append((0, 0, 10, ranges[0][3] + 1) if ranges[0][2] > 1 else (0, 0, 10, cap - 5))
        elif dice < 0.10:
            ranges.append((int(rng.choice([1, 4, 6, 1000])), 0, int(rng.integers(0, 2)), at))
        n_refused += check(starts, first, ranges, cap) is None
    assert 0 < n_refused < 200
    # the empty block is never an item; the block edges of item 0, alone and in pairs
    items, _ = check(starts, first, [(0, 0, totals[0], 0)], cap)
    assert [b for b, *_ in items] == [0, 1, 3, 4]
    for s in (MiB4, MiB4 + 1000, MiB4 + 1037):
        for off, ln in ((s - 1, 1), (s, 1), (s - 1, 2)):
            assert check(starts, first, [(0, off, ln, 0)], cap) is not None


def test_every_refusal_leaves_the_arrays_untouched(oracle_layout):
    sizes, (starts, first) = oracle_layout
    L = tsq.lib()
    st, fi = np.array(starts, dtype=np.uint64), np.array(first, dtype=np.uint64)
    cap = 100_000
    # a layout with a refused item (item 1 owns no block)
    starts_r, first_r = layout([[1000], [], [500]])
    st_r, fi_r = np.array(starts_r, dtype=np.uint64), np.array(first_r, dtype=np.uint64)

    def call(st, fi, quads, cap_items=8, cap_groups=8, out_cap=cap):
        items, groups = (tsq.RangeItem * 8)(), (tsq.BlockGroup * 8)()
        for k in range(8):
            items[k].block, items[k].out_at, groups[k].block, groups[k].hi = 77, 78, 79, 80
        rr = (tsq.ItemRange * max(len(quads), 1))(*[tsq.ItemRange(i, 0, o, n, a) for i, o, n, a in quads])
        ni, ng = C.c_uint32(12345), C.c_uint32(12345)
        rc = L.tsqa_plan_item_ranges(st.ctypes.data, st.size - 1, fi.ctypes.data, fi.size - 1, rr, len(quads), out_cap,
                                     items, cap_items, C.byref(ni), groups, cap_groups, C.byref(ng))
        untouched = all(items[k].block == 77 and items[k].out_at == 78 and groups[k].block == 79 and groups[k].hi == 80 for k in range(8))
        return rc, untouched, ni.value, ng.value

    assert call(st, fi, [(4, 0, 100, 0), (3, MiB4 - 1, 2, 100)])[:2] == (0, False)
    for quads in ([(len(sizes), 0, 1, 0)],                              # an item number past the index
                  [(4, 70_000 - 5, 6, 0)], [(0, 1, 1, 0)], [(4, 70_001, 0, 0)],     # past the item's total
                  [(4, 0, 100, cap - 99)],                              # past out_cap
                  [(4, 0, 100, 0), (3, 5, 100, 99)]):                   # overlapping destinations
        rc, untouched, ni, ng = call(st, fi, [(1, 5, 5, 50_000)] + quads)
        assert rc == 3 and untouched and (ni, ng) == (12345, 12345), quads
    assert call(st, fi, [(4, 0, 100, 100), (3, 5, 100, 0)])[0] == 0      # touching destinations are fine
    rc, untouched, _, _ = call(st_r, fi_r, [(0, 0, 10, 0), (1, 0, 1, 10)])      # a refused item
    assert rc == 3 and untouched
    rc, untouched, _, _ = call(st_r, fi_r, [(1, 0, 0, 0)])                      # ... even for no bytes
    assert rc == 3 and untouched
    assert call(st_r, fi_r, [(0, 990, 10, 0), (2, 0, 500, 10)])[0] == 0
    # arrays too small: nothing written, the counts needed are reported
    quads = [(3, MiB4 - 1, 2, 0), (4, 0, 10, 10)]                        # three items, three groups
    assert call(st, fi, quads, cap_items=2) == (3, True, 3, 3)
    assert call(st, fi, quads, cap_groups=2) == (3, True, 3, 3)
    assert call(st, fi, quads, cap_items=3, cap_groups=3)[0] == 0
    with pytest.raises(tsq.TsqError) as e:
        tsq.plan_item_ranges(starts, first, quads, cap, cap_items=1, cap_groups=1)
    assert e.value.code == 3 and e.value.needed == (3, 3)
    # bad layouts and pointers
    ni, ng = C.c_uint32(0), C.c_uint32(0)
    assert L.tsqa_plan_item_ranges(None, 1, fi.ctypes.data, 1, None, 0, 10, None, 0, C.byref(ni), None, 0, C.byref(ng)) == 3
    assert L.tsqa_plan_item_ranges(st.ctypes.data, st.size - 1, None, 1, None, 0, 10, None, 0, C.byref(ni), None, 0, C.byref(ng)) == 3
    assert L.tsqa_plan_item_ranges(st.ctypes.data, st.size - 1, fi.ctypes.data, fi.size - 1, None, 0, 10, None, 0, None, None, 0, C.byref(ng)) == 3
    assert plan(starts, [0, 1, 2], [(0, 0, 1, 0)], 10) is None           # item_first does not end at the block count
    assert plan(starts, [1] + first[1:], [(0, 0, 1, 0)], 10) is None     # ... or start at 0
    assert plan([0, 10, 20, 30], [0, 2, 1, 3], [(0, 0, 1, 0)], 10) is None      # decreasing
    assert plan([0, MiB4 + 1], [0, 1], [(0, 0, 1, 0)], 10) is None       # a block longer than 4 MiB
