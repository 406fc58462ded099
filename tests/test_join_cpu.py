"""CPU-only: joingen's restatements against the host-only planner (tsqa_plan_join), the host frame walk (tsqa_walk_frames) and the
oracle, and that each of its cases reaches what it aims at.  The kernels' side of the same cases: test_gpu_join.py."""
import ctypes as C

import numpy as np
import pytest

import joingen as jg
import turbosqueeze_amd as tsq


def host_walk(blob: bytes):
    """tsqa_walk_frames on a container -> (rc, n_blocks, total, [stream_len])"""
    raw = np.frombuffer(blob, dtype=np.uint8)
    cap = max(int.from_bytes(blob[4:8], "little"), 1)
    frame_at, sizes, ext, out_len = (np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32),
                                     np.zeros(cap, dtype=np.uint32))
    nb, total = C.c_uint32(0), C.c_uint64(0)
    rc = tsq.lib().tsqa_walk_frames(raw.ctypes.data, raw.size, cap, frame_at.ctypes.data, sizes.ctypes.data, ext.ctypes.data,
                                    out_len.ctypes.data, C.byref(nb), C.byref(total))
    return rc, nb.value, total.value, [int(s) for s in sizes[:nb.value]]


@pytest.fixture(scope="module")
def healthy():
    return {c.name: (c, c.expect(c.need_blocks, 1 << 62)) for c in jg.healthy_cases()}


def test_every_healthy_join_is_walked_by_the_host_walk_and_decoded_by_the_oracle(healthy, oracle):
    for name, (case, e) in healthy.items():
        assert case.healthy and e["status"] == jg.OK and e["item_status"] == [0] * len(case.items), name
        blob = e["container"]
        assert len(blob) == e["out_size"], name
        rc, nb, total, sizes = host_walk(blob)
        assert rc == 0 and nb == case.need_blocks == len(sizes) and total == len(case.data()), name
        assert sizes == e["block_sizes"], name
        got = oracle.decompress(blob, threads=4)
        assert got is not None and bytes(got) == case.data(), name
        # the rule of the header, from the containers' bytes alone
        again, again_sizes = jg.joined([it.blob[:len(it.blob) - it.tail] for it in case.items])
        assert again == blob and again_sizes == sizes, name


def test_the_same_container_twice_gives_its_data_twice(healthy, oracle):
    case, e = healthy["twice"]
    assert case.offsets[2] == case.offsets[0] and case.items[2].data == case.items[0].data
    assert bytes(oracle.decompress(e["container"])) == case.data() and case.data().count(case.items[0].data) >= 2


def test_bytes_behind_the_last_frame_are_left_out(healthy):
    case, e = healthy["tails"]
    assert [it.tail for it in case.items if it.tail] == list(jg.TAILS)
    walks = case.walks()
    for k, it in enumerate(case.items):
        assert case.sizes[k] - walks[k][0] == it.tail, it.name
    assert e["out_size"] == 16 + sum(case.sizes[k] - it.tail - 16 for k, it in enumerate(case.items))


def plan(frame_bytes, blocks, totals):
    try:
        return tsq.plan_join(frame_bytes, blocks, totals) + (0,)
    except tsq.TsqError as err:
        if err.code == jg.ERR_OVERFLOW:
            return err.body_at, err.first_block, None, None, None, jg.ERR_OVERFLOW
        assert err.code == jg.ERR_ARG
        return None


def test_plan_join_is_restated(healthy):
    for name, (case, e) in healthy.items():
        fb = [w[0] for w in case.walks()]
        want = jg.plan_join(fb, case.blocks, case.totals)
        assert plan(fb, case.blocks, case.totals) == want, name
        assert want[0] == e["body_at"] and want[4] == e["out_size"] and want[1] == e["first_block"], name
    ok = ([22, 40, 16 + 6 * 7], [1, 2, 7], [0, 2 * jg.BLOCK, 5])
    assert plan(*ok) == jg.plan_join(*ok) and jg.plan_join(*ok)[5] == 0
    for what, k, v in [("frame_bytes", 0, 21), ("frame_bytes", 1, 16 + 6 * 2 - 1), ("blocks", 2, 0), ("totals", 0, jg.BLOCK + 1),
                       ("totals", 1, 2 * jg.BLOCK + 1)]:
        args = [list(a) for a in ok]
        args[("frame_bytes", "blocks", "totals").index(what)][k] = v
        assert jg.plan_join(*args) is None and plan(*args) is None, (what, k, v)
    assert jg.plan_join([], [], []) is None


def test_plan_join_block_sum_of_2_to_the_32():
    half = 1 << 31
    args = ([16 + 6 * half] * 2, [half] * 2, [1, 2])
    want = jg.plan_join(*args)
    assert want[5] == jg.ERR_OVERFLOW and want[1] == [0, half, 1 << 32]
    got = plan(*args)
    assert got[5] == jg.ERR_OVERFLOW and (got[0], got[1]) == (want[0], want[1])      # the tables are still filled
    args = ([16 + 6 * half, 16 + 6 * (half - 1)], [half, half - 1], [1, 2])
    assert plan(*args) == jg.plan_join(*args) and jg.plan_join(*args)[2] == 0xFFFFFFFF


def test_plan_join_null_pointers():
    L = tsq.lib()
    one64, one32 = (C.c_uint64 * 2)(22, 0), (C.c_uint32 * 2)(1, 0)
    out = [(C.c_uint64 * 2)(7, 7), (C.c_uint64 * 2)(7, 7), C.c_uint32(7), C.c_uint64(7), C.c_uint64(7)]
    full = [one64, one32, one64, 1, out[0], out[1], C.byref(out[2]), C.byref(out[3]), C.byref(out[4])]
    for k in (0, 1, 2, 4, 5, 6, 7, 8):
        args = list(full)
        args[k] = None
        assert L.tsqa_plan_join(*args) == jg.ERR_ARG, k
    args = list(full)
    args[3] = 0
    assert L.tsqa_plan_join(*args) == jg.ERR_ARG
    assert list(out[0]) == [7, 7] and out[4].value == 7
    assert L.tsqa_plan_join(*full) == 0 and list(out[0]) == [16, 22] and out[4].value == 22


def test_small_bodies_put_seams_at_every_residue(healthy):
    case, _ = healthy["tiny_513"]
    assert min(len(it.blob) for it in case.items) == 25 and all(1 <= len(it.data) <= 40 for it in case.items)
    src, dst, shift, most = jg.seams(case)
    print("tiny_513: source residues", sorted(src), "destination residues", sorted(dst), "shifts", sorted(shift), "items per word", most)
    assert src == dst == shift == set(range(16))
    assert most >= 3, "no 16-byte word touches three items"
    for align in jg.ALIGNS:
        c, _ = healthy[f"tiny_257_align_{align}"]
        src, dst, _, _ = jg.seams(c)
        assert (src == {0} or align == 1) and dst == set(range(16)) and all(o % align == 0 for o in c.offsets)


def test_body_places_pass_2_to_the_24_where_they_aim(healthy):
    inside, edge = healthy["carry_inside_a_wavefront"][0], healthy["carry_at_a_wavefront_edge"][0]
    at = jg.crossing(inside)
    print("carry_inside_a_wavefront: the first body place at or above 2^24 is item", at)
    assert at == 247 and at % jg.WAVE not in (0, jg.WAVE - 1) and at < jg.GROUP      # (byte 2^24 of the join lies in item 246)
    assert all(abs(n - 68119) < 200 for n in inside.sizes)
    at = jg.crossing(edge)
    print("carry_at_a_wavefront_edge: the first body place at or above 2^24 is item", at)
    assert at == jg.CARRY_EDGE_CROSSING and at % jg.WAVE == 0 and at < jg.GROUP
    big = edge.items[jg.CARRY_EDGE_BIG_AT]
    assert len(big.data) <= jg.BLOCK and sum(len(it.data) > 1 << 16 for it in edge.items) == 1
    for c in (inside, edge):
        assert len(c.items) == 300 and c.arena.size < 26_000_000


def test_the_other_cases_are_what_they_say(healthy):
    mix = healthy["mix"][0]
    assert [len(it.data) for it in mix.items] == [1, 2, 5, 70_000, 4096, jg.BLOCK + 1] and mix.blocks == [1, 1, 1, 1, 1, 2]
    exts = [it.blob[18] >> 7 for it in mix.items]
    assert exts == [0, 1, 0, 1, 0, 1]
    sb = healthy["short_blocks"][0]
    assert sb.blocks == [1, 1, 1, jg.SPLIT_BLOCKS, 1, 1, 1] and jg.SPLIT_BLOCKS > 4 * jg.GROUP


def test_each_damaged_item_is_refused_by_its_rule(oracle):
    rules = {}
    for name, at in jg.refusal_cases():
        case = jg.refusal(name, at)
        it = case.items[at]
        assert case.refused_by(at) == it.rule, (name, at, case.refused_by(at))
        assert [k for k in range(len(case.items)) if case.refused_by(k)] == [at]
        rules[name] = it.rule
        e = case.expect(case.need_blocks, 1 << 30)
        assert e["status"] == jg.ERR_FORMAT and e["out_size"] == 0 and e["container"] is None
        assert e["item_status"] == [jg.ERR_FORMAT if k == at else 0 for k in range(300)]
        if it.place is None and len(it.blob) >= 16:
            from mtgen import expected_of_the_scheduler
            assert expected_of_the_scheduler(oracle, it.blob) is None, f"{name}: the oracle delivers it"
    print("refused by:", rules)
    assert set(rules.values()) == {"place", "header", "walk"} and len(rules) >= 14


def test_rooms():
    table = {what: (case, cap, room, case.expect(cap, room)) for what, case, cap, room in jg.rooms()}
    case, cap, room, e = table["exactly the room needed"]
    assert e["status"] == 0 and e["out_size"] == room and cap == 257
    for what in ("one block short", "one byte short"):
        case, cap, room, e = table[what]
        assert e["status"] == jg.ERR_OVERFLOW and e["container"] is None
    assert table["one block short"][3]["item_status"] == [0] * 256 + [jg.ERR_OVERFLOW] and table["one block short"][3]["out_size"] == 0
    assert table["one byte short"][3]["item_status"] == [0] * 257 and table["one byte short"][3]["out_size"] == table["one byte short"][2] + 1
    e = table["blocks for the items before the item of many blocks and one of its own"][3]
    assert e["item_status"] == [0, 0, 0, 6, 6, 6, 6] and e["first_block"][-1] == jg.SPLIT_BLOCKS + 6
    assert table["one block"][3]["item_status"] == [0] + [6] * 6
