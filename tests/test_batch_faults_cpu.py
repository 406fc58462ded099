"""No GPU: the seeded batch of tests/faultgen.py reaches what test_gpu_batch_faults.py needs of it.  Every verdict here is the
oracle's; the generator's restatement of the frame walk is held against the oracle where the two can be compared."""
import collections
import ctypes as C

import numpy as np
import pytest

import faultgen as fg
import mtgen
import turbosqueeze_amd as tsq


@pytest.fixture(scope="module")
def batch(oracle):
    return fg.batch(oracle)


def test_every_class_is_present_with_its_count(batch, oracle):
    count = collections.Counter(it.klass for it in batch)
    assert count["twin_walk"] == 2 and count["twin_stream"] == 38, "forty twins: two for the frame walk, 38 for a block decoder"
    assert count["damaged_valid"] + count["damaged_refused"] == 131
    # the oracle alone refuses 66 of the damaged containers and decodes 65; two of those 65 (a header that promises a byte too many,
    # a header that counts a block too few) decode to another length than their header states, which every decompress entry point of
    # the library refuses (mtgen.expected_of_the_scheduler): 68 refused, 63 damaged yet valid
    raw = {name: oracle.decompress(blob) for name, blob in mtgen.damaged_containers()}
    assert sum(w is None for w in raw.values()) == 66 and sum(w is not None for w in raw.values()) == 65
    stricter = sorted(it.name for it in batch if it.klass == "damaged_refused" and raw[it.name] is not None)
    assert stricter == ["n_blocks_minus_1", "total_plus_1"]
    assert count["damaged_refused"] == 68 and count["damaged_valid"] == 63
    assert count["uneven"] == 1 and count["tight"] == 2 and count["place"] == 3 and 120 <= count["clean"] <= 135
    assert set(count) == set(fg.REFUSED_CLASSES) | set(fg.ACCEPTED_CLASSES)
    for it in batch:
        assert it.refused == (it.klass in fg.REFUSED_CLASSES), it.name


def test_the_oracle_gives_every_verdict(batch, oracle):
    for it in batch:
        got = oracle.decompress(it.blob)
        if it.klass == "tight":
            assert got is not None and len(got) == it.cap + 1 and it.by_walk, it.name      # refused for its room, by the walk
        elif it.refused:
            assert got is None or len(got) != fg.header_of(it.blob)[2], it.name           # (the padded and the re-counted forms too)
        else:
            assert got == it.want and len(got) <= it.cap, it.name
    # the generator's frame walk against the oracle: what the walk refuses, the oracle refuses (or decodes to another length)
    assert all(it.refused for it in batch if it.by_walk)


def test_the_planner_takes_every_item(batch):
    for it in batch:
        assert len(it.blob) >= fg.MIN_ITEM and 1 <= it.n_blocks <= (len(it.blob) - fg.HEADER) // fg.MIN_FRAME, it.name
        if it.n_blocks != fg.header_of(it.blob)[1]:
            assert it.by_walk, it.name


def test_who_refuses_what(batch):
    by_walk = {it.name for it in batch if it.by_walk}
    header_cases = {name for name, _ in mtgen.header_and_tail_cases()} - {"trailing_1", "trailing_100"}
    assert header_cases <= by_walk
    assert sum(it.klass in ("twin_walk", "tight") for it in batch if it.by_walk) == 4
    assert sum(it.klass == "twin_stream" and not it.by_walk for it in batch) == 38
    assert sum(it.klass == "damaged_refused" and not it.by_walk for it in batch) >= 40, "byte damage that only a block decoder finds"
    # faults in the first, a middle and the last block of multi-block items
    assert {int(it.name.rsplit("_", 1)[1]) for it in batch if it.klass == "twin_stream"} == {0, 2, 3, 5}


def test_refused_items_have_healthy_neighbours(batch):
    assert not batch[0].refused and not batch[-1].refused
    for k, it in enumerate(batch):
        if it.refused:
            assert not batch[k - 1].refused and not batch[k + 1].refused, it.name


def test_sizes_cross_the_seams(batch):
    assert len(batch) > 256, "reserve_batch's first size and the 256-lane workgroups of the walk and closing kernels"
    blocks = sum(it.n_blocks for it in batch)
    assert blocks > 512 and 1500 <= blocks <= 1900, "more than 2 x CUs blocks"
    uneven = next(it for it in batch if it.klass == "uneven")
    assert uneven.n_blocks == 6 and len(uneven.want) > fg.BLOCK
    assert min(it.cap for it in batch if it.klass == "clean") < 100
    assert max(it.cap for it in batch if it.klass == "clean") > 100_000


def test_bad_places(batch):
    arena, offsets, sizes = fg.packed_layout(batch)
    assert all(o % fg.ALIGN == 0 for o in offsets)
    off2, sz2, bad = fg.bad_places(batch, offsets, sizes, arena.size)
    assert sorted(bad.values()) == ["a size below 16", "a size too short for the stated block count", "an offset past the arena"]
    for i, what in bad.items():
        assert batch[i].klass == "place" and not batch[i - 1].refused and not batch[i + 1].refused
        n, at = sz2[i], off2[i]
        assert n > arena.size or at > arena.size - n or n < fg.HEADER or batch[i].n_blocks > (n - fg.HEADER) // fg.MIN_FRAME, what
    assert [i for i in range(len(batch)) if (off2[i], sz2[i]) != (offsets[i], sizes[i])] == sorted(bad)


def test_the_host_walk_refuses_what_the_restated_walk_refuses(batch):
    """tsqa_walk_frames (the library's one frame walk, on the host) over every item as it travels, with the count and the total
    its own header states and no capacity: TSQA_ERR_FORMAT exactly where faultgen.walk_refuses says so, the header's total elsewhere"""
    L = tsq.lib()
    refused = []
    for it in batch:
        _, nb, total = fg.header_of(it.blob)
        cap = max(len(it.blob) // 6, 1)
        frame_at = np.zeros(cap, dtype=np.uint64)
        sizes, ext, out_len = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
        got_nb, got_total = C.c_uint32(0), C.c_uint64(0)
        rc = L.tsqa_walk_frames(it.blob, len(it.blob), cap, frame_at.ctypes.data, sizes.ctypes.data, ext.ctypes.data, out_len.ctypes.data,
                                C.byref(got_nb), C.byref(got_total))
        want = fg.walk_refuses(it.blob, nb, total)
        assert rc == (fg.ERR_FORMAT if want else fg.OK), it.name
        if want:
            refused.append(it.name)
        else:
            assert got_total.value == total and got_nb.value == nb, it.name
    assert len(refused) == 11 and len(batch) - len(refused) == 290
    # (the two tight items are healthy containers: only a capacity refuses them)
    assert sorted(refused) == sorted(it.name for it in batch if it.by_walk and it.klass != "tight")
