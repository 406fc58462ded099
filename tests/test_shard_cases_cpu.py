"""The cases of the block and sharded entry points (tests/shardgen.py), checked without a GPU: the containers decode to the
generator's plain bytes under the oracle (and the compiled reference, where it is built), the library's own host frame walk
(tsqa_walk_frames: walk_frames of tsq_format.h, which tsqa_sharded_fetch_decode_async shares) gives the generator's frame table and
refuses exactly the damage the generator marks TSQA_ERR_FORMAT, the ownership arithmetic is the runtime's, the per-rank place images
add up to the container, and the whole set is the one pinned by tests/golden/shard_cases.json."""
import json
import os

import numpy as np
import pytest

import shardgen
import streamgen
from shardgen import BLOCK, OUTPUT_SZ, ERR_FORMAT, ERR_STREAM, OK

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shard_cases.json")


def sentinel(n):
    return ((np.arange(n, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5


def walk(blob, size):
    from turbosqueeze_amd import sharding
    return sharding.walk_frames(np.frombuffer(bytes(blob), dtype=np.uint8), size)


def test_the_seven_symbols_are_exported():
    import turbosqueeze_amd
    L = turbosqueeze_amd.lib()
    missing = [s for s in shardgen.SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    assert len(shardgen.SYMBOLS) == 7


def test_oracle_decodes_every_deal_container_to_the_generators_bytes(oracle):
    for d in shardgen.deals():
        assert oracle.decompress(d.container) == d.plain, d.name
        assert max(d.sizes) <= shardgen.SMALL and max(len(p) for _, _, p in d.blocks) <= shardgen.SMALL, d.name
    for dmg in shardgen.damage_cases():
        if dmg.bad is not None:                       # a damaged stream: the oracle's decoder refuses it too
            assert oracle.decompress(np.frombuffer(dmg.blob, dtype=np.uint8)) is None, dmg.name


def test_reference_decodes_every_deal_block_to_the_generators_bytes(reference):
    for d in shardgen.deals():
        for ext, stream, plain in d.blocks:
            assert reference.decode_block(stream, ext) == plain, d.name


def test_walk_frames_gives_the_generators_frame_table():
    for d in shardgen.deals():
        total, frame_at, sizes, ext, out_len = walk(d.container, len(d.container))
        assert total == d.total and frame_at.tolist() == d.frame_at and sizes.tolist() == d.sizes, d.name
        assert ext.tolist() == [e for e, _, _ in d.blocks] and out_len.tolist() == [len(p) for _, _, p in d.blocks], d.name


def test_walk_frames_gives_the_place_tables_frame_table(oracle):
    """the tables whose streams are the oracle's are healthy containers too, with one level in every frame word"""
    walked = 0
    for t in shardgen.place_tables(oracle):
        if OUTPUT_SZ in t.sizes:
            continue                                  # (random bytes in a slot: place moves them, nobody walks them)
        total, frame_at, sizes, ext, out_len = walk(t.container, t.size)
        assert total == t.n_total and frame_at.tolist() == t.frame_at and sizes.tolist() == t.sizes, t.name
        assert ext.tolist() == [t.ext] * t.nb and int(out_len.sum()) == t.n_total, t.name
        assert [int.from_bytes(s[:3], "little") for s in t.streams] == out_len.tolist(), t.name
        walked += 1
    assert walked == 5


def test_walk_frames_refuses_exactly_the_damage_marked_err_format():
    cases = shardgen.damage_cases()
    assert sum(1 for c in cases if c.bad is None) == 6 and sum(1 for c in cases if c.bad is not None) >= 1
    for c in cases:
        want_format = c.bad is None
        assert all(code == ERR_FORMAT for codes in c.codes.values() for code in codes) == want_format, c.name
        if want_format:
            with pytest.raises(ValueError):
                walk(c.blob, c.size)
        else:
            # a twin's frames are well formed: the walk passes it, its stream is the decoder's to refuse, on its owner alone
            total, frame_at, sizes, _, out_len = walk(c.blob, c.size)
            assert sizes.tolist() == [len(st) for _, st, _ in c.blocks] and total == sum(len(p) for _, _, p in c.blocks), c.name
            for w, codes in c.codes.items():
                assert codes == [ERR_STREAM if r == c.bad % w else OK for r in range(w)], (c.name, w)
            assert streamgen.model_decode(c.blocks[c.bad][1], c.blocks[c.bad][0]) is None, c.name


def test_ownership_is_the_runtimes_formula_and_a_partition():
    for nb in (1, 2, 7, 11):
        for world in shardgen.worlds_of(nb):
            owned = [list(range(r, nb, world)) for r in range(world)]
            for r in range(world):
                # tsq_runtime.hip, tsqa_sharded_fetch_decode_async: n_local = nb > rank ? (nb - rank + world - 1) / world : 0
                assert len(owned[r]) == shardgen.n_local(nb, world, r) == ((nb - r + world - 1) // world if nb > r else 0)
            assert sorted(b for o in owned for b in o) == list(range(nb))
        assert {nb, nb + 3} <= set(shardgen.worlds_of(nb)) and {1, 2, 3, 5, 8} <= set(shardgen.worlds_of(nb))
    for d in shardgen.deals():
        for w, r in d.triples():
            s = d.shard(w, r)
            assert s.n_local == shardgen.n_local(d.nb, w, r)
            assert [a for a, _ in s.stream_pieces] == [k * OUTPUT_SZ for k in range(s.n_local)]
            assert [a for a, _ in s.out_pieces] == [k * BLOCK for k in range(s.n_local)]
    # n_local == 0, nb == world and nb == world + 1 all occur
    shapes = {(d.nb - w) for d in shardgen.deals() for w in d.worlds()}
    assert 0 in shapes and 1 in shapes and min(shapes) < 0


def test_per_rank_place_images_add_up_to_the_container(oracle):
    tables = shardgen.place_tables(oracle)
    assert {t.ext for t in tables} == {0, 1}
    assert any(3 in t.sizes for t in tables) and any(OUTPUT_SZ in t.sizes for t in tables)
    for t in tables:
        fill = sentinel(t.size + 100)
        for world in t.worlds():
            written = np.zeros(fill.size, dtype=np.int32)
            union = fill.copy()
            for rank in range(world):
                img = shardgen.image(fill, t.host_pieces(world, rank))
                diff = img != fill
                # (a written byte may equal the sentinel by chance: count the pieces, not the differences)
                for at, data in t.host_pieces(world, rank):
                    written[at:at + len(data)] += 1
                union[diff] = img[diff]
            assert np.all(written[:t.size] == 1) and not written[t.size:].any(), (t.name, world)
            assert bytes(union[:t.size]) == t.container and np.array_equal(union[t.size:], fill[t.size:]), (t.name, world)
    # the deals' containers are streamgen.container of their blocks, and a table of a deal's own streams is that container
    for d in shardgen.deals():
        if len({e for e, _, _ in d.blocks}) == 1:
            t = shardgen.PlaceTable(d.name, d.blocks[0][0], [st for _, st, _ in d.blocks], d.total)
            assert t.container == streamgen.container(d.blocks)


def test_encode_calls_hold_filler_behind_what_may_be_read(oracle):
    by_stride = {}
    for name, cases in shardgen.arrangements().items():
        for stride in shardgen.STRIDES:
            call = shardgen.encode_arrangement(name, cases, stride)
            # tsq_runtime.hip, tsqa_encode_blocks_async
            tail = min(stride - BLOCK, 128) if stride > BLOCK else 0
            readable = (call.n_blocks - 1) * stride + call.last_len + tail
            assert call.buffer.size > readable + 128 and call.buffer[readable:].min() >= 1, call.name
            for k in range(call.n_blocks - 1):
                gap = call.buffer[k * stride + BLOCK + tail:(k + 1) * stride]
                assert gap.size == stride - BLOCK - tail and (gap.size == 0 or gap.min() >= 1), call.name
            by_stride[name, stride] = [h for _, h in call.sees]
        # what a block sees does not depend on the stride, but for the last block of a contiguous buffer: zeros
        a, b, c = (by_stride[name, s] for s in shardgen.STRIDES)
        assert a[:2] == b[:2] == c[:2] and b == c and a[2] == bytes(128) and b[2] != bytes(128), name
    for case in shardgen.one_block_cases():
        for stride in (BLOCK + 128,) + shardgen.ODD_STRIDES:
            call = shardgen.encode_one_block(case, stride)
            tail = stride - BLOCK
            assert call.buffer[call.last_len + tail:].min() >= 1, case.name
            seen = call.sees[0][1]
            assert len(seen) == 128 and seen[tail:] == bytes(128 - tail), case.name
            assert seen[:tail] == call.buffer[call.last_len:call.last_len + tail].tobytes(), case.name
    # the look-ahead matters: some case's stream changes with the bytes a narrower stride hides
    changed = [c.name for c in shardgen.one_block_cases() if c.halo is not None and
               oracle.encode_block(c.data, 1, shardgen.encode_one_block(c, BLOCK + 5).sees[0][1]) != oracle.encode_block(c.data, 1, c.halo)]
    assert changed, "no case tells a look-ahead of 5 bytes from one of 128"


def test_packing_for_decode_blocks_reaches_every_residue_and_shuffles():
    blocks = [tuple(v[1:]) for v in shardgen.valid_blocks()][:40]
    arena, frames, outs, cap, order = shardgen.pack_for_decode(blocks, np.random.default_rng(3))
    assert {int(a) % 16 for a in frames["stream_at"]} == set(range(16))
    assert sorted(order) == list(range(40)) and order != sorted(order)
    at = frames["out_at"].astype(np.int64)
    assert (np.diff(at) < 0).any()
    spans = sorted((int(a), int(a) + int(n)) for a, n in outs)
    assert all(lo2 > hi1 for (_, hi1), (lo2, _) in zip(spans, spans[1:])) and spans[0][0] >= 1 and spans[-1][1] < cap
    for i, b in enumerate(order):
        ext, st, plain = blocks[b]
        f = frames[i]
        assert bytes(arena[int(f["stream_at"]):int(f["stream_at"]) + int(f["stream_len"])]) == st
        assert (int(f["ext"]), int(f["out_len"])) == (ext, len(plain))
    assert frames.dtype.itemsize == 32


def test_cases_are_the_pinned_ones(oracle):
    pinned = json.load(open(GOLDEN))
    now = json.loads(json.dumps(shardgen.pins(oracle)))
    for part in pinned:
        assert now[part] == pinned[part], f"{part} differs from tests/golden/shard_cases.json (python tests/golden/make_shard_cases.py)"
    assert set(now) == set(pinned)
    c = pinned["counts"]
    # the floor of the issue's own list: 1, 2, 7 and 11 blocks at worlds {1, 2, 3, 5, 8, nb, nb + 3}, every rank of each
    assert c["deal_triples"] == sum(w for nb in (1, 2, 7, 11) for w in shardgen.worlds_of(nb)) == 122
    assert c["deal_triples_owning_nothing"] >= 10 and c["damage_triples"] == 6 * len(pinned["damage"])
    assert c["decode_valid"] >= 150 and c["decode_twins"] >= 40 and c["encode_one_block"] >= 75 and c["encode_arrangements"] == 6
