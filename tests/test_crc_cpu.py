"""CPU-only: the CRC arithmetic of the issue against zlib, the library's host forms (tsqa_crc32_host, tsqa_crc32_combine, tsqa_plan_crc32
and the shared crc_mul / crc_xpow8 behind them) against zlib and the Python restatement, and that crcgen's cases are what they say.
The kernels' side of the same cases: test_gpu_crc.py."""
import os
import zlib

import numpy as np
import pytest

import crcgen as kg
import turbosqueeze_amd as tsq
from test_cut_cpu import host_walk


def seeded(n, seed=kg.SEED):
    return np.random.default_rng(seed + n).integers(0, 256, n, dtype=np.uint8).tobytes()


def test_the_identities_against_zlib():
    """the issue's script: R is linear, zeros in front do not count, parts shift to the end, and crc32 adds the init and final term"""
    for n in kg.IDENTITY_SIZES:
        m = seeded(n)
        r = kg.reg(m)
        assert kg.reg(bytes(7) + m) == r
        assert zlib.crc32(m) == r ^ kg.mul(0xFFFFFFFF, kg.xpow8(n)) ^ 0xFFFFFFFF, n
        for cut in sorted({0, 1, n // 3, n - 1, n} & set(range(n + 1))):
            a, b = m[:cut], m[cut:]
            assert r == kg.mul(kg.reg(a), kg.xpow8(len(b))) ^ kg.reg(b), (n, cut)
            assert zlib.crc32(m) == kg.combine(zlib.crc32(a), zlib.crc32(b), len(b)), (n, cut)
        # parts in any order
        if n >= 3:
            parts = [(0, n // 3), (n // 3, n // 2), (n // 2, n)]
            acc = 0
            for lo, hi in reversed(parts):
                acc ^= kg.mul(kg.reg(m[lo:hi]), kg.xpow8(n - hi))
            assert acc == r
    assert kg.mul(0x80000000, 0x12345678) == 0x12345678 and kg.xpow8(0) == 0x80000000 and kg.xpow8(1) == 0x00800000
    assert kg.xpow8(2 ** 32 - 1) == kg.xpow8(0), "x has order 2^32 - 1: byte counts reduce mod 2^32 - 1"


def test_the_symbols_are_there():
    for name in ("tsqa_crc32_async", "tsqa_crc32", "tsqa_plan_crc32", "tsqa_crc32_host", "tsqa_crc32_combine", "tsqa_profile_read_crc"):
        assert hasattr(tsq.lib(), name), name
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "turbosqueeze_amd.h")) as f:
        header = f.read()
    for name in ("tsqa_crc32_async(", "tsqa_crc32(", "tsqa_plan_crc32(", "tsqa_crc32_host(", "tsqa_crc32_combine(", "tsqa_profile_read_crc("):
        assert name in header, name
    for name in ("RangeIndex", "SizedIndex", "BatchIndex", "DeviceBatchIndex", "PackedBatch"):
        assert hasattr(getattr(tsq, name), "crc32"), name
    assert hasattr(tsq.DeviceCodec, "crc32_async") and hasattr(tsq.DeviceCodec, "profile_read_crc")
    assert hasattr(tsq.CrcTable, "check") and callable(tsq.crc32_combine) and callable(tsq.plan_crc32) and callable(tsq.crc32_host)


def test_the_host_crc_is_zlibs():
    for n in kg.IDENTITY_SIZES + (4, 7, 8, 65537):
        m = seeded(n, 3)
        assert tsq.crc32_host(m) == zlib.crc32(m), n
        assert tsq.crc32_host(m, 0xDEADBEEF) == zlib.crc32(m, 0xDEADBEEF), n
        assert tsq.crc32_host(m[n // 2:], tsq.crc32_host(m[:n // 2])) == zlib.crc32(m), n
    assert tsq.lib().tsqa_crc32_host(77, None, 0) == 77


def test_combine_against_zlib_and_the_restatement():
    a, b = seeded(777, 5), seeded(3000, 6)
    for cut in (0, 1, 100, 3000):
        assert tsq.crc32_combine(zlib.crc32(a + b[:3000 - cut]), zlib.crc32(b[3000 - cut:]), cut) == zlib.crc32(a + b), cut
    # lengths at which a 32-bit exponent (8 * len passes 2^32 at 2^29) or a missing reduction mod 2^32 - 1 shows
    for len_b in kg.COMBINE_LENGTHS:
        for ca, cb in ((0xDEADBEEF, 0x12345678), (zlib.crc32(a), 0), (0, 0xFFFFFFFF), (1, 0x80000000)):
            assert tsq.crc32_combine(ca, cb, len_b) == kg.combine(ca, cb, len_b), (len_b, hex(ca))
    # against zlib itself on zeros, whose CRC is cheap to extend: crc32(A | 0^n) at a length past 2^29
    n = 2 ** 29 + 1
    zeros = zlib.crc32(bytes(1 << 20))
    z = 0
    for _ in range(n >> 20):
        z = tsq.crc32_combine(z, zeros, 1 << 20)
    z = tsq.crc32_combine(z, zlib.crc32(bytes(n & ((1 << 20) - 1))), n & ((1 << 20) - 1))
    c = zlib.crc32(b"")
    chunk = bytes(1 << 24)
    for _ in range(n >> 24):
        c = zlib.crc32(chunk, c)
    c = zlib.crc32(bytes(n & ((1 << 24) - 1)), c)
    assert z == c and tsq.crc32_combine(zlib.crc32(a), c, n) == zlib.crc32(bytes(n & ((1 << 24) - 1)), _extend(zlib.crc32(a), chunk, n >> 24))


def _extend(crc, chunk, times):
    for _ in range(times):
        crc = zlib.crc32(chunk, crc)
    return crc


@pytest.mark.parametrize("case", kg.host_cases(), ids=lambda c: c.name)
def test_the_host_plan_against_zlib(case):
    e = case.expect()
    idx = case.index
    crc, whole = tsq.plan_crc32(idx.data, case.item_at(), case.statuses)
    assert crc.tolist() == e["items"], case.name
    assert whole == e["all"] == zlib.crc32(idx.data), case.name
    # the blocks' CRCs fold into the items' with the library's combine
    for k in range(idx.n_items):
        if e["status"][k]:
            assert e["items"][k] == 0
            continue
        folded = 0
        for b in range(idx.item_first[k], idx.item_first[k + 1]):
            folded = tsq.crc32_combine(folded, e["blocks"][b], idx.out_start[b + 1] - idx.out_start[b])
        assert folded == e["items"][k], (case.name, k)


def test_the_host_plan_refuses():
    L = tsq.lib()
    at = np.array([0, 3, 2], dtype=np.uint64)
    out = np.zeros(2, dtype=np.uint32)
    assert L.tsqa_plan_crc32(b"abc", at.ctypes.data, None, 2, out.ctypes.data, None) == kg.ERR_ARG      # unordered
    at = np.array([0, 3], dtype=np.uint64)
    assert L.tsqa_plan_crc32(b"abc", at.ctypes.data, None, 0, out.ctypes.data, None) == kg.ERR_ARG      # no items
    assert L.tsqa_plan_crc32(b"abc", None, None, 1, out.ctypes.data, None) == kg.ERR_ARG
    assert L.tsqa_plan_crc32(b"abc", at.ctypes.data, None, 1, None, None) == kg.ERR_ARG
    assert L.tsqa_plan_crc32(None, at.ctypes.data, None, 1, out.ctypes.data, None) == kg.ERR_ARG        # bytes owed, none given
    assert L.tsqa_plan_crc32(b"abc", at.ctypes.data, None, 1, out.ctypes.data, None) == 0 and int(out[0]) == zlib.crc32(b"abc")


def test_the_cases_reach_their_aim(oracle):
    # the sources are what the walk and the oracle say
    for case in (kg.images("zeros_outc_1"), kg.chunks("random_4"), kg.ragged(257, True), kg.two_blocks(0)):
        idx = case.index
        rc, nb, total, _, _, out_len = host_walk(idx.blob)
        assert rc == 0 and nb == idx.n_blocks and total == idx.total, case.name
        assert bytes(oracle.decompress(idx.blob)) == idx.data, case.name
    # ragged: every tail length 1 .. 16 of a block's last cell occurs in the batch (each item is a block that starts a cell), and
    # joined every residue mod 16 of a block's distance to its item's end occurs against every tail length class
    idx = kg.ragged(513, False).index
    lens = [idx.item_span(k)[1] for k in range(idx.n_items)]
    assert min(lens) == 1 and max(lens) == 40 and {(n - 1) % 16 + 1 for n in lens} == set(range(1, 17))
    j = kg.ragged(513, True).index
    assert j.n_items == 1 and j.n_blocks == 513 and j.data == idx.data
    behind = {((j.total - j.out_start[b + 1]) % 16, (j.out_start[b + 1] - j.out_start[b]) % 16) for b in range(j.n_blocks)}
    assert len(behind) >= 128, len(behind)
    # images: OUTC is a whole number of cells, OUTC + 1 ends one byte into a cell; the chunk cases end off a cell edge
    assert kg.OUTC % kg.CELL == 0 and kg.images("zeros_outc").index.total == kg.OUTC and kg.images("zeros_outc_1").index.total % kg.CELL == 1
    assert kg.chunks("zeros_2").index.total == 3 * kg.OUTC + 5 and (3 * kg.OUTC + 5) % kg.CELL == 5
    # the ring: blocks longer than the ring, so cell addresses wrap
    for case in kg.ring_cases():
        idx = case.index
        assert max(idx.out_start[b + 1] - idx.out_start[b] for b in range(idx.n_blocks)) > kg.RING, case.name
    # bits and runs: all CRCs differ, and the runs of zeros differ only by the init term (R of zeros is 0)
    e = kg.bits().expect()
    assert len(set(e["items"])) == 256
    for byte in (0, 255):
        e = kg.runs(byte).expect()
        assert len(set(e["items"])) == 32 and e["items"][0] == 0 and kg.runs(byte).index.item_span(0)[1] == 0
    assert all(kg.reg(bytes(n)) == 0 for n in range(32))
    # two blocks: the first block's word travels over ONE byte, the item is 4 MiB + 1
    for ext in (0, 1):
        idx = kg.two_blocks(ext).index
        assert idx.n_blocks == 2 and idx.total == (1 << 22) + 1 and idx.out_start[1] == 1 << 22
    assert kg.two_blocks(0).index.blob != kg.two_blocks(1).index.blob and kg.two_blocks(0).index.data == kg.two_blocks(1).index.data
    # verdicts
    d = kg.damaged()
    assert [k for k, st in enumerate(d.statuses) if st] == list(kg.rg.DAMAGED_AT) and d.index.n_items == 300
    t = kg.twin()
    assert t.index.n_items == 3 and t.index.item_first[2] - t.index.item_first[1] == 6 and t.expect()["status"] == [0, kg.ERR_STREAM, 0]
    assert t.expect()["all"] == 0 and t.expect()["d_status"] == kg.ERR_STREAM
    assert kg.refused_case().index.refused and kg.no_blocks().index.n_blocks == 0
    assert kg.phrase("sized").index.n_blocks == kg.phrase("plain").index.n_blocks == 257
