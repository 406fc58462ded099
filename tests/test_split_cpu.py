"""CPU-only: splitgen's restatements against the host-only planner and the oracle, and that each of its inputs reaches what it aims
at.  The kernels' side of the same inputs: test_gpu_split.py."""
import numpy as np
import pytest

import splitgen as sg
import turbosqueeze_amd as tsq

BUDGET = 512        # 2 x 256 CUs; the GPU tests take the device's own


def test_plan_split_is_restated():
    ns = [1, 2, 4095, 4096, 4097, (1 << 22) - 1, 1 << 22, (1 << 22) + 5, 10**9, (1 << 44) - 4096, (1 << 44) - 4095, 1 << 44]
    for bl in sg.BLOCK_LENS:
        for n in ns:
            want = sg.plan_split(n, bl)
            if want is None:
                with pytest.raises(tsq.TsqError) as e:
                    tsq.plan_split(n, bl)
                assert e.value.code == sg.ERR_ARG
            else:
                assert tsq.plan_split(n, bl) == want, (n, bl)
    assert sg.plan_split((1 << 44) - 4095, 4096) is None and sg.plan_split(1 << 44, 4096) is None    # 2^32 blocks
    assert sg.plan_split((1 << 44) - 4096, 4096)[0] == 0xFFFFFFFF and sg.plan_split(1 << 44, 8192) is not None
    for n, bl in [(0, 4096), (100, 0), (100, 2048), (100, 1 << 23), (100, 4097), (100, 12288), (100, 3 << 12)]:
        assert sg.plan_split(n, bl) is None
        with pytest.raises(tsq.TsqError) as e:
            tsq.plan_split(n, bl)
        assert e.value.code == sg.ERR_ARG


def test_plan_split_null_pointers_and_the_batch_bound():
    import ctypes as C
    L = tsq.lib()
    nb, bound = C.c_uint32(7), C.c_size_t(7)
    assert L.tsqa_plan_split(100, 4096, None, C.byref(bound)) == sg.ERR_ARG
    assert L.tsqa_plan_split(100, 4096, C.byref(nb), None) == sg.ERR_ARG
    assert (nb.value, bound.value) == (7, 7)
    # the term per block is tsqa_batch_bound's: at 4 MiB the two agree for every n
    for n in (1, 77, 4096, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, 3 * (1 << 22) + 12345, 10**9):
        blocks, room = tsq.plan_split(n, 1 << 22)
        assert blocks == L.tsqa_block_count(n) and room == L.tsqa_batch_bound(n) == tsq.batch_bound(n), n


def test_at_4_mib_it_is_the_oracles_container(oracle):
    data = sg.mixed((1 << 22) + 5, 7)
    for ext in (0, 1):
        blob, sizes = sg.expected_split(oracle, data, 1 << 22, ext)
        assert blob == oracle.compress(data, ext)
        assert len(sizes) == 2


@pytest.mark.parametrize("ext", [0, 1])
def test_every_case_round_trips_through_the_oracle(oracle, ext):
    cases = [(sg.count_input(BUDGET)[:n], 4096) for _, n in sg.count_cases(BUDGET)]
    cases += [sg.carry_input(), sg.edge_input(), (sg.mixed(300_000, 9), 1 << 16), (sg.mixed(300_001, 10), 1 << 14)]
    for data, bl in cases:
        blob, sizes = sg.expected_split(oracle, data, bl, ext)
        nb, bound = sg.plan_split(data.size, bl)
        assert len(sizes) == nb and len(blob) == sg.frame_places(sizes)[-1] <= bound
        assert oracle.decompress(blob) == data.tobytes(), (data.size, bl)
        assert not sg.walk_refuses(blob, len(blob), nb, data.size) and not sg.sized_refuses(blob, len(blob), sizes, nb, data.size)


def test_count_cases_reach_the_pass_and_launch_edges(oracle):
    cases = sg.count_cases(BUDGET)
    assert {nb for nb, _ in cases} == {1, 2, 255, 256, 257, 511, 512, 513, 1025}
    assert max(n for _, n in cases) == sg.count_input(BUDGET).size <= (1 << 22) + 4096
    for nb, n in cases:
        assert sg.plan_split(n, 4096)[0] == nb and (n - 1) % 4096 + 1 in (1, 4095, 4096)
    assert [len(sg.launches(nb, BUDGET)) for nb in (511, 512, 513, 1025)] == [1, 1, 2, 3]
    # sizes vary: streams shorter and longer than their blocks (text; random bytes and zeros, which find no match)
    _, sizes = sg.expected_split(oracle, sg.count_input(BUDGET), 4096, 0)
    assert min(sizes) < 3500 and max(sizes) > 4096 and len(set(sizes)) > 50


@pytest.mark.parametrize("ext", [0, 1])
def test_edge_case_differs_with_zero_halos_at_every_edge(oracle, ext):
    data, bl = sg.edge_input()
    want = sg.block_streams(oracle, data, bl, ext)
    zero = sg.block_streams(oracle, data, bl, ext, zero_halo=True)
    assert len(want) == 9
    assert all(w != z for w, z in zip(want[:-1], zero[:-1])), [w != z for w, z in zip(want, zero)]
    assert want[-1] == zero[-1]
    assert sg.container_of(zero, data.size, ext) != sg.expected_split(oracle, data, bl, ext)[0]
    assert oracle.decompress(sg.container_of(zero, data.size, ext)) == data.tobytes()       # valid all the same, only not what is owed


@pytest.mark.parametrize("ext", [0, 1])
def test_carry_case_crosses_2_to_24_inside_a_pass(oracle, ext):
    data, bl = sg.carry_input()
    _, sizes = sg.expected_split(oracle, data, bl, ext)
    assert len(sizes) == 300 and min(sizes) > bl
    for budget in (BUDGET, 2 * 304, 2 * 228):
        crossing = sg.carry_crossing(sizes, budget)
        assert crossing and 0 < crossing[0] % sg.GROUP, "no pass of 256 blocks carries out of the low 24 bits"
        assert len(crossing) > 1, "no block of the same pass behind the carry"
        assert sg.frame_places(sizes)[-1] >= sg.SPLIT


def test_pack_cut_restates_the_rule():
    sizes = [10, 20, 30]
    blob = sg.container_of([bytes([k]) * s for k, s in enumerate(sizes)], 99, 0)
    guard = np.full(len(blob) + 8, 0xEE, dtype=np.uint8)
    want, need, st = sg.pack_cut(blob, sizes, len(blob), guard)
    assert (need, st) == (len(blob), 0) and want[:need].tobytes() == blob and (want[need:] == 0xEE).all()
    want, need, st = sg.pack_cut(blob, sizes, len(blob) - 1, guard)
    assert (need, st) == (len(blob), sg.ERR_OVERFLOW)
    assert want[:16 + 13 + 23].tobytes() == blob[:52] and (want[52:] == 0xEE).all()
    want, _, _ = sg.pack_cut(blob, sizes, 16 + 13 + 5, guard)               # the middle frame cut: the last one does not fit either
    assert want[:29].tobytes() == blob[:29] and (want[29:] == 0xEE).all()


@pytest.mark.parametrize("ext", [0, 1])
def test_false_tables_are_refused_and_the_container_is_valid(oracle, ext):
    data, bl = sg.carry_input()
    blob, sizes = sg.expected_split(oracle, data, bl, ext)
    nb, cap = len(sizes), data.size + 64
    assert not sg.walk_refuses(blob, len(blob), nb, cap) and not sg.sized_refuses(blob, len(blob), sizes, nb, cap)
    cases = sg.false_tables(blob, sizes)
    assert len(cases) == 8 + 3 + 1 + 1 + 2
    for name, c, n, table in cases:
        assert sg.sized_refuses(c, n, table, nb, cap), name
        if c is blob and n == len(blob):
            assert table != sizes, name                                     # the container is the valid one: the table is what is false
        else:
            assert table == sizes and sg.walk_refuses(c, n, nb, cap), name  # the table is true and the plain walk refuses too


def test_new_names_are_exported():
    import re
    import os
    L = tsq.lib()
    names = ["tsqa_plan_split", "tsqa_compress_device_split_async", "tsqa_compress_device_split", "tsqa_decompress_device_sized_async",
             "tsqa_decompress_device_sized"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "turbosqueeze_amd.h")).read()
    for n in names:
        assert hasattr(L, n) and re.search(r"\b%s\s*\(" % n, header), n
    assert callable(tsq.plan_split)
    for m in ("compress_split", "compress_split_async", "decompress_sized", "decompress_sized_async"):
        assert callable(getattr(tsq.DeviceCodec, m)), m
