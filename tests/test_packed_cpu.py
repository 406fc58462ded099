"""CPU-only: the packed-batch entry points are exported and declared in the header, tsqa_batch_bound (host code) is batch_bound, and
tsqa_plan_packed (host code) is the layout rule of the header -- restated here in plain Python -- with its refusals."""
import numpy as np
import pytest

import turbosqueeze_amd as tsq
from test_abi_cpu import declared_symbols

MiB4 = 1 << 22
PACKED_SYMBOLS = ["tsqa_batch_bound", "tsqa_plan_packed", "tsqa_compress_batch_packed_async", "tsqa_compress_batch_packed",
                  "tsqa_decompress_batch_packed_async"]
FILL = 0xA5A5A5A5A5A5A5A5


def test_packed_symbols_exported_and_declared():
    L = tsq.lib()
    assert all(hasattr(L, n) for n in PACKED_SYMBOLS)
    assert set(PACKED_SYMBOLS) <= declared_symbols()


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, MiB4 - 1, MiB4, MiB4 + 1, 3 * MiB4 + 5])
def test_batch_bound_is_the_python_one(n):
    assert int(tsq.lib().tsqa_batch_bound(n)) == tsq.batch_bound(n)


def rule(sizes, align):
    """the layout rule of include/turbosqueeze_amd.h -> offsets, n + 1 of them"""
    offsets = [0]
    for i, n in enumerate(sizes):
        end = offsets[i] + n
        offsets.append(end if i + 1 == len(sizes) else -(-end // align) * align)
    return offsets


def plan(sizes, n_items, align, null=None):
    """tsqa_plan_packed on a sentinel-filled offsets array -> (rc, offsets)"""
    sz = np.ascontiguousarray(sizes, dtype=np.uint64)
    offsets = np.full(len(sizes) + 1, FILL, dtype=np.uint64)
    rc = tsq.lib().tsqa_plan_packed(None if null == "sizes" else sz.ctypes.data, n_items, align, None if null == "offsets" else offsets.ctypes.data)
    return rc, [int(x) for x in offsets]


@pytest.mark.parametrize("align", [1, 2, 16, 256, 4096])
def test_plan_packed_follows_the_rule(align):
    rng = np.random.default_rng(align)
    cases = [[22], [align], [align, align, 3 * align], [1, align - 1 or 1, align + 1, 2 * align, 22, 5 * MiB4 + 3, 16]]
    cases += [[int(x) for x in rng.integers(1, 3 * align + 50, int(rng.integers(1, 40)))] for _ in range(50)]
    for sizes in cases:
        rc, offsets = plan(sizes, len(sizes), align)
        assert rc == 0 and offsets == rule(sizes, align), (sizes, align)
        assert offsets == tsq.plan_packed(sizes, align)
        assert all(o % align == 0 for o in offsets[:-1]) and offsets[-1] == offsets[-2] + sizes[-1]


def test_plan_packed_refusals_write_nothing():
    sizes = [22, 100, 7]
    for align in (0, 3, 8192):
        assert plan(sizes, 3, align) == (3, [FILL] * 4)
    assert plan(sizes, 0, 16) == (3, [FILL] * 4)
    assert plan(sizes, 3, 16, null="sizes") == (3, [FILL] * 4)
    assert plan(sizes, 3, 16, null="offsets")[0] == 3
    with pytest.raises(tsq.TsqError) as e:
        tsq.plan_packed(sizes, 24)
    assert e.value.code == 3
