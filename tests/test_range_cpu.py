"""CPU-only: the range-read entry points are exported, and tsqa_plan_ranges (host code) cuts ranges into per-block items exactly as a
small Python model does -- on containers made by the oracle and walked with tsqa_walk_frames, and on hand-made block layouts with
short blocks in the middle."""
import ctypes as C

import numpy as np
import pytest

import turbosqueeze_amd as tsq

MiB4 = 1 << 22
RANGE_SYMBOLS = ["tsqa_index_create", "tsqa_index_destroy", "tsqa_index_blocks", "tsqa_index_total", "tsqa_plan_ranges",
                 "tsqa_decompress_ranges_async", "tsqa_decompress_ranges"]


def model(out_start, ranges, out_cap):
    """-> the items tsqa_plan_ranges must give, or None where it must refuse (TSQA_ERR_ARG)"""
    total = out_start[-1]
    items, dst = [], []
    for off, ln, at in ranges:
        if ln == 0:
            continue
        if off + ln > total or at + ln > out_cap:
            return None
        dst.append((at, ln))
        for b in range(len(out_start) - 1):
            lo, hi = max(off, out_start[b]), min(off + ln, out_start[b + 1])
            if lo < hi:
                items.append((b, lo - out_start[b], hi - out_start[b], at + lo - off))
    dst.sort()
    if any(a[0] + a[1] > b[0] for a, b in zip(dst, dst[1:])):
        return None
    return items


def plan(out_start, ranges, out_cap, cap_items=None):
    try:
        return tsq.plan_ranges(out_start, ranges, out_cap, cap_items)
    except tsq.TsqError as e:
        assert e.code == 3
        return None


def check(out_start, ranges, out_cap):
    want = model(out_start, ranges, out_cap)
    assert plan(out_start, ranges, out_cap) == want
    return want


def walked_starts(blob: bytes):
    L = tsq.lib()
    cap = len(blob) // 6 + 1
    frame_at, sizes, ext, out_len = (np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32))
    nb, total = C.c_uint32(0), C.c_uint64(0)
    buf = C.create_string_buffer(blob, len(blob))
    assert L.tsqa_walk_frames(buf, len(blob), cap, frame_at.ctypes.data, sizes.ctypes.data, ext.ctypes.data, out_len.ctypes.data,
                              C.byref(nb), C.byref(total)) == 0
    starts = [0]
    for b in range(nb.value):
        starts.append(starts[-1] + int(out_len[b]))
    assert starts[-1] == total.value
    return starts


def test_range_symbols_exported():
    L = tsq.lib()
    assert all(hasattr(L, n) for n in RANGE_SYMBOLS)
    assert C.sizeof(tsq.Range) == 24 and C.sizeof(tsq.RangeItem) == 24


def test_python_surface_exists():
    assert callable(tsq.DeviceCodec.index)
    for m in ("read", "read_many", "read_many_async", "read_into", "close"):
        assert callable(getattr(tsq.RangeIndex, m))


def test_index_create_without_context_is_an_argument_error():
    L = tsq.lib()
    out = C.c_void_p()
    blob = C.create_string_buffer(b"TSQ1" + bytes(12))
    assert L.tsqa_index_create(None, blob, 16, C.byref(out)) == 3
    assert not out.value
    assert L.tsqa_index_blocks(None) == 0 and L.tsqa_index_total(None) == 0
    L.tsqa_index_destroy(None)
    rr = (tsq.Range * 1)(tsq.Range(0, 1, 0))
    assert L.tsqa_decompress_ranges(None, None, rr, 1, None, 1, None) == 3
    assert L.tsqa_decompress_ranges_async(None, None, rr, 1, None, 1, None, None) == 3


def test_plan_on_oracle_containers(oracle):
    host = np.concatenate([tsq.synth.text(2 * MiB4 + 5000, seed=11), tsq.synth.mix(MiB4 + 333, seed=12)])
    starts = walked_starts(oracle.compress(host, 1, threads=4))
    assert starts == [0, MiB4, 2 * MiB4, 3 * MiB4, host.size]          # three full blocks and a short last one
    total = host.size
    cap = total + 64
    cases = [
        [(100, 5000, 0)],                                   # inside one block
        [(MiB4 - 10, 20, 7)],                               # across one boundary
        [(MiB4 - 10, MiB4 + 20, 0)],                        # across two boundaries (three blocks)
        [(5, total - 5, 0)],                                # all four blocks
        [(0, 1, 0), (total - 1, 1, 1)],                     # the first and the last byte
        [(3 * MiB4 + 1, total - 3 * MiB4 - 1, 0)],          # the short last block
        [(0, total, 0)],                                    # everything
        [(42, 0, 0), (0, 0, cap), (total, 0, 0)],           # zero-length ranges give no item
    ]
    for ranges in cases:
        got = check(starts, ranges, cap)
        assert got is not None and all(lo < hi for _, lo, hi, _ in got)
    assert len(check(starts, [(5, total - 5, 0)], cap)) == 4
    assert check(starts, [(42, 0, 0)], cap) == []
    # each refusal
    assert check(starts, [(total - 5, 6, 0)], cap) is None             # past the total
    assert check(starts, [(total, 1, 0)], cap) is None
    assert check(starts, [(0, 100, cap - 99)], cap) is None            # past the output
    assert check(starts, [(0, 100, 0), (500, 100, 99)], cap) is None   # overlapping destinations
    assert check(starts, [(0, 100, 100), (500, 100, 0)], cap) is not None     # touching is fine
    assert plan(starts, [(MiB4 - 10, 20, 0)], cap, cap_items=1) is None         # the items do not fit
    assert plan(starts, [(MiB4 - 10, 20, 0)], cap, cap_items=2) == model(starts, [(MiB4 - 10, 20, 0)], cap)


def test_plan_with_short_middle_blocks():
    lens = [MiB4, 1000, 0, 37, MiB4, 5, 1 << 20]            # short blocks in the middle, one of them empty
    starts = [0] + list(np.cumsum(lens).tolist())
    total = starts[-1]
    rng = np.random.default_rng(7)
    cap = 3 * total
    for _ in range(300):
        n = int(rng.integers(1, 6))
        ranges, at = [], int(rng.integers(0, 50))
        for _ in range(n):
            off = int(rng.integers(0, total))
            ln = int(rng.integers(0, total - off + 1)) if rng.random() < 0.3 else int(rng.integers(0, min(3000, total - off) + 1))
            ranges.append((off, ln, at))
            at += ln + int(rng.integers(0, 20))
        if rng.random() < 0.1:                                   # a deliberate overlap or overflow now and then
            ranges.append((0, 10, ranges[0][2] + 1) if rng.random() < 0.5 else (0, 10, cap - 5))
        check(starts, ranges, cap)
    # every boundary byte, alone and paired with its neighbour
    for s in starts[1:-1]:
        for off, ln in ((s - 1, 1), (s, 1), (s - 1, 2)):
            if 0 <= off and off + ln <= total:
                assert check(starts, [(off, ln, 0)], cap)
    # the empty block is never an item
    assert all(b != 2 for b, *_ in check(starts, [(0, total, 0)], cap))


def test_plan_refuses_bad_layouts_and_pointers():
    L = tsq.lib()
    assert plan([5, MiB4], [(0, 1, 0)], 10) is None            # out_start[0] must be 0
    assert plan([0, MiB4 + 1], [(0, 1, 0)], 10) is None        # a block longer than 4 MiB
    assert plan([0, 10, 5], [(0, 1, 0)], 10) is None           # decreasing
    n = C.c_uint32(0)
    starts = np.array([0, 10], dtype=np.uint64)
    assert L.tsqa_plan_ranges(None, 1, None, 0, 10, None, 0, C.byref(n)) == 3
    assert L.tsqa_plan_ranges(starts.ctypes.data, 1, None, 1, 10, None, 0, C.byref(n)) == 3
    assert L.tsqa_plan_ranges(starts.ctypes.data, 1, None, 0, 10, None, 0, C.byref(n)) == 0 and n.value == 0
    # the refusal for too few items writes nothing and reports the count needed
    items = (tsq.RangeItem * 4)()
    items[0].block = 77
    rr = (tsq.Range * 1)(tsq.Range(2, 5, 0))
    assert L.tsqa_plan_ranges(starts.ctypes.data, 1, rr, 1, 10, items, 0, C.byref(n)) == 3
    assert n.value == 1 and items[0].block == 77


@pytest.mark.parametrize("ext", [0, 1])
def test_plan_on_small_containers(oracle, ext):
    for n in (1, 777, MiB4, MiB4 + 1):
        starts = walked_starts(oracle.compress(tsq.synth.text(n, seed=n), ext))
        assert starts[-1] == n
        assert check(starts, [(0, n, 0)], n) == [(b, 0, starts[b + 1] - starts[b], starts[b]) for b in range(len(starts) - 1)]
        assert check(starts, [(n - 1, 1, 0)], 1)
