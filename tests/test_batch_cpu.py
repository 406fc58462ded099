"""CPU-only: the batch entry points are exported and declared in the header, and tsqa_plan_batch (host code) agrees with a small
Python model on random batches -- each item's first block and every refusal -- and writes nothing when it refuses."""
import ctypes as C

import numpy as np

import turbosqueeze_amd as tsq
from test_abi_cpu import declared_symbols

MiB4 = 1 << 22
BATCH_SYMBOLS = ["tsqa_plan_batch", "tsqa_compress_batch_async", "tsqa_compress_batch", "tsqa_decompress_batch_async",
                 "tsqa_decompress_batch"]


def test_batch_symbols_exported_and_declared():
    L = tsq.lib()
    assert all(hasattr(L, n) for n in BATCH_SYMBOLS)
    assert set(BATCH_SYMBOLS) <= declared_symbols()


def model(items, in_size, out_size, n_blocks=None):
    """-> the first blocks tsqa_plan_batch must give (n_items + 1 entries), or None where it must refuse (TSQA_ERR_ARG)"""
    if not items:
        return None
    first, at, dst = [], 0, []
    for k, (a, n, o, cap) in enumerate(items):
        if n == 0 or a + n > in_size or o + cap > out_size:
            return None
        if n_blocks is None:
            nb = -(-n // MiB4)
            if cap < 16 + 6 * nb:
                return None
        else:
            nb = n_blocks[k]
            if n < 16 or nb == 0 or nb > (n - 16) // 6:
                return None
        if cap:
            dst.append((o, cap))
        first.append(at)
        at += nb
    dst.sort()
    if any(x[0] + x[1] > y[0] for x, y in zip(dst, dst[1:])):
        return None
    return first + [at]


def plan(items, in_size, out_size, n_blocks=None):
    """tsqa_plan_batch through ctypes on a sentinel-filled first-block array: None when refused, after checking nothing was written"""
    first = np.full(len(items) + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    nb = None if n_blocks is None else np.ascontiguousarray(n_blocks, dtype=np.uint32)
    rc = tsq.lib().tsqa_plan_batch(tsq.api._batch_array(items), len(items), in_size, out_size, None if nb is None else nb.ctypes.data,
                                   first.ctypes.data)
    if rc:
        assert rc == 3 and (first == 0xA5A5A5A5A5A5A5A5).all(), "a refused batch wrote first blocks"
        return None
    return [int(x) for x in first]


def check(items, in_size, out_size, n_blocks=None):
    want = model(items, in_size, out_size, n_blocks)
    assert plan(items, in_size, out_size, n_blocks) == want, (items, in_size, out_size, n_blocks)
    return want


def test_compress_first_blocks():
    items = [(0, 1, 0, 22), (5, MiB4, 22, 22), (0, MiB4 + 1, 44, 28), (7, 9 * MiB4 + 5, 72, 1000), (3, 3, 1072, 22)]
    assert check(items, 10 * MiB4, 1094) == [0, 1, 2, 4, 14, 15]
    assert tsq.plan_batch(items, 10 * MiB4, 1094) == [0, 1, 2, 4, 14, 15]


def test_each_refusal():
    ok = [(0, 100, 0, 100), (50, 100, 100, 100)]                  # input ranges may overlap; output ranges may touch
    assert check(ok, 150, 200) == [0, 1, 2]
    assert check([], 150, 200) is None                             # no items
    assert check([(0, 0, 0, 100)], 150, 200) is None               # an empty item
    assert check([(100, 51, 0, 100)], 150, 200) is None            # input past in_size
    assert check([(0, 100, 101, 100)], 150, 200) is None           # output past out_size
    assert check([(0, 100, 0, 100), (0, 100, 99, 100)], 150, 200) is None    # output ranges overlap
    assert check([(0, MiB4 + 1, 0, 27)], MiB4 + 1, 200) is None    # compress: below 16 + 6 per block
    assert check([(0, MiB4 + 1, 0, 28)], MiB4 + 1, 200) == [0, 2]
    # decompress: in_len >= 16, 1 <= n_blocks <= (in_len - 16) / 6
    assert check([(0, 15, 0, 0)], 100, 0, [1]) is None
    assert check([(0, 22, 0, 0)], 100, 0, [0]) is None
    assert check([(0, 22, 0, 0)], 100, 0, [1]) == [0, 1]
    assert check([(0, 27, 0, 0)], 100, 0, [2]) is None
    assert check([(0, 28, 0, 10), (28, 40, 10, 5)], 100, 15, [2, 4]) == [0, 2, 6]


def test_random_batches_agree_with_model():
    rng = np.random.default_rng(7)
    seen_ok = seen_refused = 0
    for case in range(3000):
        decompress = bool(case & 1)
        n_items = int(rng.integers(0, 10))
        in_size = int(rng.integers(1, 12 * MiB4))
        items, nbs, out_at = [], [], 0
        for _ in range(n_items):
            ln = int(rng.choice([0, 1, 15, 16, 21, 22, 100, MiB4 - 1, MiB4, MiB4 + 1, 3 * MiB4 + 5, int(rng.integers(1, 4 * MiB4))]))
            a = int(rng.integers(0, max(1, in_size - ln + 3)))
            nb = -(-ln // MiB4)
            cap = int(rng.choice([0, 16 + 6 * nb - 1, 16 + 6 * nb, ln + 100, int(rng.integers(0, 2000))]))
            o = max(0, out_at + int(rng.integers(-3, 40)) if rng.random() < 0.95 else out_at - int(rng.integers(1, 50)))
            out_at = o + cap
            items.append((a, ln, o, cap))
            most = (ln - 16) // 6 if ln >= 16 else 0
            nbs.append(int(rng.choice([0, 1, max(nb, 1), most, most + 1])))
        out_size = max(0, out_at + int(rng.integers(-20, 20)))
        want = check(items, in_size, out_size, nbs if decompress else None)
        seen_ok += want is not None
        seen_refused += want is None
    assert seen_ok > 50 and seen_refused > 1000


def test_batch_bound_holds_the_format_minimum():
    for n in (1, 2, 699, MiB4 - 1, MiB4, MiB4 + 1, 9 * MiB4 + 5):
        nb = -(-n // MiB4)
        assert tsq.batch_bound(n) >= 16 + nb * (3 + 3) and tsq.batch_bound(n) <= tsq.container_bound(n)
