"""CPU-only: seekgen's restatement of the sized index's verdict against the oracle and tsqa_walk_frames, that each of its cases
reaches what it aims at, the new names, and the refusals that need no device.  The kernels' side: test_gpu_seek.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seekgen as kg
import splitgen as sg
import turbosqueeze_amd as tsq

BUDGET = 512        # 2 x 256 CUs; the GPU tests take the device's own


def walk(blob, n):
    """tsqa_walk_frames on the first n bytes -> (rc, frame places, sizes, out_lens)"""
    L = tsq.lib()
    cap = 1 << 12
    frame_at, sizes, ext, out_len = (C.c_uint64 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    nb, total = C.c_uint32(0), C.c_uint64(0)
    raw = np.frombuffer(bytes(blob[:n]), dtype=np.uint8)
    rc = L.tsqa_walk_frames(raw.ctypes.data, n, cap, frame_at, sizes, ext, out_len, C.byref(nb), C.byref(total))
    k = nb.value
    return rc, list(frame_at[:k]), list(sizes[:k]), list(out_len[:k])


@pytest.mark.parametrize("ext", [0, 1])
def test_true_cases_are_accepted_and_the_plan_is_the_walks(oracle, ext):
    data = sg.count_input(BUDGET)
    cases = [(data[:n], 4096) for _, n in kg.true_cases(BUDGET)] + [kg.carry()]
    assert {nb for nb, _ in kg.true_cases(BUDGET)} == {1, 2, 255, 256, 257, 511, 512, 513, 1025}
    for d, bl in cases:
        blob, sizes = sg.expected_split(oracle, d, bl, ext)
        assert not kg.host_refuses(len(blob), d.size, bl)
        assert kg.index_refuses(blob, len(blob), sizes, d.size, bl) == set(), (d.size, bl)
        # the room, not the size: what lies behind the last frame is not looked at
        assert kg.index_refuses(blob + b"\xEE" * 100, len(blob) + 100, sizes, d.size, bl) == set()
        rc, places, walked, out_len = walk(blob, len(blob))
        assert rc == 0 and walked == sizes and places == sg.frame_places(sizes)[:-1]
        # block b's output starts at b * block_len: the geometry is the walk's
        starts = kg.out_start(d.size, bl)
        assert [starts[b + 1] - starts[b] for b in range(len(sizes))] == out_len and starts[-1] == d.size
        for off, ln in kg.reads(d.size, bl):
            assert 0 <= off and ln > 0 and off + ln <= d.size


def test_reads_cover_every_edge_and_the_one_byte_block():
    r = kg.reads(2 * 4096 + 1, 4096)
    assert (0, 2 * 4096 + 1) in r and (0, 1) in r and (2 * 4096, 1) in r and (4093, 6) in r
    assert (8189, 6) not in r                                # (would end past the total: the one-byte block is read alone)
    assert r.count((2 * 4096, 1)) == 2                       # the last byte and the one-byte last block
    assert (4093, 6) in kg.reads(3 * 4096, 4096) and (8189, 6) in kg.reads(3 * 4096, 4096)


@pytest.mark.parametrize("ext", [0, 1])
def test_carry_aims_at_both_24_bit_splits(oracle, ext):
    data, bl = kg.carry()
    _, sizes = sg.expected_split(oracle, data, bl, ext)
    at = sg.frame_places(sizes)
    assert len(sizes) == 300 > kg.GROUP
    # launch 3: inside group 0 the local sums pass 2^24 (a carry out of the low 24 bits); launch 2: group 1's base is above it
    assert at[0] < sg.SPLIT <= at[kg.GROUP - 1] and at[kg.GROUP] - sg.HEADER >= sg.SPLIT
    assert sum(3 + s for s in sizes[:kg.GROUP]) >= sg.SPLIT


@pytest.mark.parametrize("ext", [0, 1])
def test_false_tables_are_refused_for_the_reason_aimed_at(oracle, ext):
    data, bl = kg.carry()
    blob, sizes = sg.expected_split(oracle, data, bl, ext)
    cases = kg.false_tables(blob, sizes)
    assert len(cases) == 15 and {w for *_, w in cases} == {kg.WORD, kg.FRAME, kg.TOTAL, kg.LENGTH}
    for name, c, n, table, why in cases:
        assert not kg.host_refuses(n, data.size, bl), name
        assert why in kg.index_refuses(c, n, table, data.size, bl), name
        assert sg.sized_refuses(c, n, table, len(sizes), data.size), name


@pytest.mark.parametrize("ext", [0, 1])
def test_geometry_cases_pass_both_walks_and_are_refused_for_the_geometry(oracle, ext):
    cases = kg.geometry(oracle, ext)
    assert [name for name, *_ in cases] == ["cuts_4096_1_4096", "cuts_4096_4095_4096_4096", "plain_4mib_as_2mib", "total_plus_1",
                                            "total_minus_1", "block_len_doubled"]
    for name, blob, table, n_total, bl, why in cases:
        nb, total = int.from_bytes(blob[4:8], "little"), int.from_bytes(blob[8:16], "little")
        # a valid container with a true table: the plain walk and the sized walk take it, and so does tsqa_walk_frames
        assert not sg.walk_refuses(blob, len(blob), nb, total), name
        assert not sg.sized_refuses(blob, len(blob), table[:nb], nb, total), name
        rc, _, walked, out_len = walk(blob, len(blob))
        assert rc == 0 and walked == table[:nb] and sum(out_len) == total, name
        assert len(oracle.decompress(blob)) == total, name
        assert not kg.host_refuses(len(blob), n_total, bl), name
        assert len(table) >= sg.plan_split(n_total, bl)[0], name
        got = kg.index_refuses(blob, len(blob), table, n_total, bl)
        assert why in got, (name, got)
    # the two containers of uneven cuts have the caller's count and total: the geometry alone refuses them
    for name, blob, table, n_total, bl, why in cases[:2]:
        assert kg.index_refuses(blob, len(blob), table, n_total, bl) == {kg.GEOMETRY}, name


@pytest.mark.parametrize("ext", [0, 1])
def test_cuts_are_refused_and_the_host_takes_them(oracle, ext):
    data = sg.count_input(BUDGET)[:40 * 4096 - 5]
    blob, sizes = sg.expected_split(oracle, data, 4096, ext)
    for name, n, why in kg.cuts(blob, sizes):
        assert not kg.host_refuses(n, data.size, 4096), name
        assert why in kg.index_refuses(blob, n, sizes, data.size, 4096), name
        assert walk(blob, n)[0] == sg.ERR_FORMAT, name
    assert kg.host_refuses(sg.HEADER + sg.MIN_FRAME * len(sizes) - 1, data.size, 4096)


def test_damage_inside_a_stream_is_not_the_walks_to_find(oracle):
    data = sg.count_input(BUDGET)[:9 * 4096]
    blob, sizes = sg.expected_split(oracle, data, 4096, 1)
    bad = kg.damaged(blob, sizes, 4)
    assert bad != blob and kg.index_refuses(bad, len(bad), sizes, data.size, 4096) == set()


def test_scan_edge_counts_are_the_pass_width():
    assert kg.scan_edge_counts() == [65535, 65536, 65537]
    assert [-(-c // kg.GROUP) for c in kg.scan_edge_counts()] == [kg.PASS, kg.PASS, kg.PASS + 1]
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "turbosqueeze_amd", "csrc", "tsq_index.cuh")
    assert re.search(r"kIndexGroup\s*=\s*256\b", open(csrc).read()), "launch 2's pass width changed: re-derive scan_edge_counts"


def test_new_names_are_exported():
    L = tsq.lib()
    names = ["tsqa_index_create_sized_async", "tsqa_index_create_sized", "tsqa_index_d_status"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "turbosqueeze_amd.h")).read()
    for n in names:
        assert hasattr(L, n) and re.search(r"\b%s\s*\(" % n, header), n
    assert callable(tsq.DeviceCodec.index_sized) and issubclass(tsq.SizedIndex, tsq.RangeIndex) and callable(tsq.SizedIndex.status)


def test_refusals_that_need_no_device():
    L = tsq.lib()
    out = C.c_void_p(0x1234)
    some = C.c_void_p(0x1000)
    for f in (L.tsqa_index_create_sized_async, L.tsqa_index_create_sized):
        assert f(None, some, 1 << 20, 40_000, 4096, some, C.byref(out), None) == kg.ERR_ARG       # NULL ctx
        assert not out.value, "*out is NULL behind a refusal"
        out.value = 0x1234
        assert f(None, some, 1 << 20, 40_000, 4096, some, None, None) == kg.ERR_ARG               # NULL out (and ctx)
    assert L.tsqa_index_d_status(None) is None
    # the restated host refusals follow tsqa_plan_split
    assert kg.host_refuses(1 << 20, 0, 4096) and kg.host_refuses(1 << 20, 100, 2048) and kg.host_refuses(1 << 20, 100, 12288)
    assert kg.host_refuses(21, 100, 4096) and not kg.host_refuses(22, 100, 4096)
