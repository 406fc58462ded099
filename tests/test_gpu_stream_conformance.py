"""GPU side of the decoder conformance catalogue (tests/streamgen.py): every valid hand-assembled stream goes through every decode
schedule and must give the generator's plain bytes; every invalid twin must be refused with the library's code for a malformed
stream (TSQA_ERR_STREAM) or frame (TSQA_ERR_FORMAT), with nothing written outside a destination.  The expected bytes come from the
builders, never from a decoder; that the model, the oracle and the compiled reference agree with them is what
test_stream_conformance_cpu.py and tests/golden/conformance_streams.json establish.

Order: the block API and the serial decoder (variant 1) see every case first, then the data-parallel schedules.  No case is
dropped: each entry point counts the cases it ran and the last test compares the counts with the catalogue's size.
(A block of 0 bytes has no byte to read: range and record entry points index it, check its total and count it.)"""
import re

import numpy as np
import pytest

import streamgen
from streamgen import CATALOGUE, blocks_for, region_container, uneven_unit  # noqa: F401
from test_gpu_range import ERR_FORMAT, ERR_STREAM, check_ranges, codec, fenced, read_fenced, to_dev, tsq  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

MiB4 = 1 << 22
COUNTS: dict = {}


def count(entry):
    COUNTS[entry] = COUNTS.get(entry, 0) + 1


def one_block(ext, stream, plain):
    return np.frombuffer(streamgen.container([(ext, stream, plain)]), dtype=np.uint8)


def refusal_code(stream):
    """what a one-block container around an invalid stream is refused with: the frame walk refuses a stream shorter than its size
    word or a block over 4 MiB (tsq_format.h read_frame), everything else is the block decoder's to find"""
    return ERR_FORMAT if len(stream) < 3 or int.from_bytes(stream[:3], "little") > streamgen.BLOCK else ERR_STREAM


def decompress_case(tsq, codec, name, ext, stream, plain):
    """plain is None: an invalid twin"""
    if plain is not None:
        got = codec.decompress(to_dev(one_block(ext, stream, plain)))
        assert bytes(got.cpu().numpy()) == plain, name
    else:
        blob = np.frombuffer(streamgen.bad_container(ext, stream), dtype=np.uint8)
        with pytest.raises(tsq.TsqError) as e:
            codec.decompress(to_dev(blob), out_cap=MiB4 + 64)
        assert e.value.code == refusal_code(stream), (name, e.value.code)


def all_cases():
    for name, (ext, stream, plain) in CATALOGUE.valid.items():
        yield name, ext, stream, plain
    for name, (ext, stream) in CATALOGUE.invalid.items():
        yield name, ext, stream, None


def test_block_api_and_serial_decoder(tsq, codec):
    codec.set_variant(0, 1)
    try:
        for name, ext, stream, plain in all_cases():
            got = tsq.tsq_decode(stream, ext)
            assert got == (plain if plain is not None else b""), name
            count("block_api")
            decompress_case(tsq, codec, name, ext, stream, plain)
            count("decompress_variant_1")
    finally:
        codec.set_variant(0, 0)


@pytest.mark.parametrize("variant", [4, 6, 5, 3, 0])
def test_one_block_container_at_every_schedule(tsq, codec, variant):
    """4: one workgroup per block; 6: two; 5: three; 3: two or three by the block count; 0: the library's own choice"""
    codec.set_variant(0, variant)
    try:
        for name, ext, stream, plain in all_cases():
            decompress_case(tsq, codec, name, ext, stream, plain)
            count(f"decompress_variant_{variant}")
    finally:
        codec.set_variant(0, 0)


# ---------------------------------------------------------------- containers of uneven blocks

def test_containers_of_uneven_blocks_at_every_launch_shape(tsq, codec, oracle):
    """Block counts from the device's CU count, so that the default variant takes the three-workgroup, the two-workgroup and the
    one-workgroup path and the "full rounds + multi-workgroup tail" path of launch_decode_kernels with a tail of three and of two workgroups per block
    (tsq_launch.cuh:150-166)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    counts = {"three": max(6, cus // 3), "two": cus // 2, "one": cus - 5, "rounds_and_tail_of_three": cus + 7,
              "rounds_and_tail_of_two": cus + cus // 2 - 1}
    assert 3 * counts["three"] <= cus < 3 * counts["two"] and 2 * counts["two"] <= cus < 2 * counts["one"] and counts["one"] <= cus
    tail3, tail2 = counts["rounds_and_tail_of_three"] % cus, counts["rounds_and_tail_of_two"] % cus
    assert tail3 and 3 * tail3 <= cus and 2 * tail2 <= cus < 3 * tail2
    codec.set_variant(0, 0)
    for shape, n in counts.items():
        blocks = blocks_for(n)
        blob = streamgen.container(blocks)
        plain = b"".join(p for _, _, p in blocks)
        assert int.from_bytes(blob[8:16], "little") == len(plain)
        got = codec.decompress(to_dev(np.frombuffer(blob, dtype=np.uint8)))
        assert got.numel() == len(plain) and bytes(got.cpu().numpy()) == plain, shape


# ---------------------------------------------------------------- range reads

def test_range_reads_inside_the_adversarial_regions_and_over_uneven_block_edges(tsq, codec):
    blocks, names = region_container()
    blob = streamgen.container(blocks)
    plain = np.frombuffer(b"".join(p for _, _, p in blocks), dtype=np.uint8)
    idx = codec.index(to_dev(np.frombuffer(blob, dtype=np.uint8)))
    assert idx.n_blocks == len(blocks) and idx.total == plain.size
    rng = np.random.default_rng(77)
    starts = np.concatenate([[0], np.cumsum([len(p) for _, _, p in blocks])]).tolist()
    ranges = [(0, plain.size)]
    kinds = set()
    for b, name in enumerate(names):
        if name is None:
            continue
        for region, (lo, hi) in CATALOGUE.regions[name].items():
            kinds.add(re.sub(r"_\d+$", "", region))
            lo, hi = starts[b] + lo, starts[b] + hi
            w = hi - lo
            assert w >= 4
            ranges += [(lo + w // 3, w // 3 + 1), (lo + 1, min(w - 2, 5000)), (hi - min(w, 300), min(w, 300) - 1), (lo + w // 2, 1)]
            ranges += [(int(rng.integers(lo, hi - 1)), 1 + int(rng.integers(0, min(w // 2, 20000)))) for _ in range(4)]
    assert {"dense", "match64", "edge_sweep", "clamped", "source_across_chunk_start", "ring_end", "in_chunk", "chain"} <= kinds
    ranges = [(o, min(ln, plain.size - o)) for o, ln in ranges]
    # the uneven block edges, zero-length blocks included
    for e in sorted(set(starts[1:-1])):
        for o, ln in ((e - 5, 10), (e - 1, 1), (e, 1), (e - 1, 2), (e - 100, 20000), (e, 77), (e - 78, 79)):
            if 0 <= o and o + ln <= plain.size:
                ranges.append((o, ln))
    ranges.append((starts[1], starts[6] - starts[1]))            # from the 1-byte block to the end of the 3 MiB one
    check_ranges(idx, plain, ranges, rng)
    for o, ln in ranges[1:40]:                                    # one range per call
        assert np.array_equal(idx.read(o, ln).cpu().numpy(), plain[o:o + ln]), (o, ln)
    idx.close()


def test_whole_range_read_of_every_case(tsq, codec):
    rng = np.random.default_rng(5)
    healthy = CATALOGUE.valid["soup_5000_default_noext"]
    for name, ext, stream, plain in all_cases():
        if plain is not None:
            idx = codec.index(to_dev(one_block(ext, stream, plain)))
            assert idx.total == len(plain) and idx.n_blocks == 1, name
            if plain:
                n = len(plain)
                check_ranges(idx, np.frombuffer(plain, dtype=np.uint8), [(0, n), (n - 1, 1), (n // 2, n - n // 2)], rng)
            idx.close()
        elif refusal_code(stream) == ERR_FORMAT:
            with pytest.raises(tsq.TsqError) as e:
                codec.index(to_dev(np.frombuffer(streamgen.bad_container(ext, stream), dtype=np.uint8)))
            assert e.value.code == ERR_FORMAT, name
        else:
            # the twin between two healthy blocks: the whole range is refused, ranges wholly inside a healthy block are exact
            claimed = int.from_bytes(stream[:3], "little")
            h = len(healthy[2])
            blob = streamgen.container([healthy, (ext, stream, bytes(claimed)), healthy])
            idx = codec.index(to_dev(np.frombuffer(blob, dtype=np.uint8)))
            total = 2 * h + claimed
            assert idx.total == total and idx.n_blocks == 3, name
            outs, cap = fenced(rng, [total])
            _, rc = read_fenced(idx, [(0, total)], outs, cap)
            assert rc == ERR_STREAM, (name, rc)
            outs, cap = fenced(rng, [claimed])
            _, rc = read_fenced(idx, [(h, claimed)], outs, cap)   # the bad block alone
            assert rc == ERR_STREAM, (name, rc)
            hp = np.frombuffer(healthy[2], dtype=np.uint8)
            both = np.concatenate([hp, np.zeros(claimed, dtype=np.uint8), hp])
            check_ranges(idx, both, [(0, h), (h + claimed, h), (17, h - 17), (h + claimed + 5, 1000), (h - 1, 1), (h + claimed, 1)], rng)
            idx.close()
        count("range_read")


# ---------------------------------------------------------------- batches

def test_batches_of_catalogue_containers(tsq, codec):
    names, blobs, plains, want_status = [], [], [], []
    for name, ext, stream, plain in all_cases():
        names.append(name)
        if plain is not None:
            blobs.append(one_block(ext, stream, plain)); plains.append(np.frombuffer(plain, dtype=np.uint8)); want_status.append(0)
        else:
            blobs.append(np.frombuffer(streamgen.bad_container(ext, stream), dtype=np.uint8)); plains.append(None)
            want_status.append(refusal_code(stream))
    arena = to_dev(np.concatenate(blobs))
    at, views = 0, []
    for b in blobs:
        views.append(arena[at:at + b.size]); at += b.size
    with pytest.raises(tsq.TsqError) as e:
        codec.decompress_batch(views)
    assert e.value.item_status == want_status, [(n, s, w) for n, s, w in zip(names, e.value.item_status, want_status) if s != w]
    for name, res, plain in zip(names, e.value.results, plains):
        assert (res is None) == (plain is None), name
        if plain is not None:
            assert np.array_equal(res.cpu().numpy(), plain), name
        count("batch_decompress")

    # record reads through the grouped kernel
    idx = codec.index_batch(views)
    assert idx.items == len(blobs)
    rng = np.random.default_rng(11)
    records = []
    for i, (name, plain) in enumerate(zip(names, plains)):
        if plain is None:
            st = idx.item_status(i)
            if want_status[i] == ERR_FORMAT:
                assert st == ERR_FORMAT, name
            else:
                assert st == 0, name                              # its frames are well formed: the stream is the decoder's to refuse
                with pytest.raises(tsq.TsqError) as e:
                    idx.read(i, 0, idx.item_total(i))
                assert e.value.code == ERR_STREAM, (name, e.value.code)
        else:
            assert idx.item_status(i) == 0 and idx.item_total(i) == plain.size, name
            n = plain.size
            if n:
                records.append((i, 0, n))
                for _ in range(3):
                    o = int(rng.integers(0, n))
                    records.append((i, o, int(rng.integers(1, min(n - o, 4096) + 1))))
        count("batch_records")
    # several hundred records inside one adversarial block: dec_group_kernel decodes it once for all
    for name in ("match64_groups_cut_by_image_budget_ext", "dense13_five_chunks_noext", "chain_of_6000_pairs_noext"):
        i = names.index(name)
        n = plains[i].size
        for o in rng.integers(0, n - 64, 400).tolist():
            records.append((i, int(o), int(rng.integers(1, 65))))
    order = rng.permutation(len(records)).tolist()
    records = [records[k] for k in order]
    packed, rviews = idx.read_many(records)
    got = packed.cpu().numpy()
    at = 0
    for (i, o, ln) in records:
        assert np.array_equal(got[at:at + ln], plains[i][o:o + ln]), (names[i], o, ln)
        at += ln
    idx.close()


# ---------------------------------------------------------------- packed batches

ERR_STALL = 7


def packed_decode(tsq, codec, arena, offsets, sizes, caps, rng, variant):
    """decompress_batch_packed_async of the containers at `offsets` of the host arena, tables in device memory, outputs behind
    1..47 guard bytes -> (status, d_out_sizes, the output buffer on the host, the destinations), after checking that every byte
    outside the destinations still holds the sentinel"""
    import torch
    from test_gpu_range import sentinel
    outs, cap = fenced(rng, caps)
    guard = sentinel(cap)
    out = to_dev(guard)
    d_offsets = torch.tensor(offsets[:len(sizes)], dtype=torch.int64, device="cuda")
    d_sizes = torch.tensor(sizes, dtype=torch.int64, device="cuda")
    d_out_sizes = torch.full((len(sizes),), -1, dtype=torch.int64, device="cuda")
    codec.set_variant(0, variant)
    try:
        codec.decompress_batch_packed_async(to_dev(arena), d_offsets, d_sizes, list(zip(outs, caps)), [1] * len(sizes), out, d_out_sizes)
        torch.cuda.synchronize()
        status = codec.status()
    finally:
        codec.set_variant(0, 0)
    back = out.cpu().numpy()
    untouched = np.ones(cap, dtype=bool)
    for a, ln in zip(outs, caps):
        untouched[a:a + ln] = False
    assert np.array_equal(back[untouched], guard[untouched]), "a packed decode wrote outside its destinations"
    return status, d_out_sizes.cpu().tolist(), back, outs


def test_packed_batches_of_catalogue_containers(tsq, codec):
    """tsqa_decompress_batch_packed_async (batch_place_kernel, then batch_walk_kernel, then one decode over every frame): every valid
    stream's one-block container in a host arena at tsqa_plan_packed's places -- align 1: the containers start at every residue --
    with non-zero filler in the padding, on one workgroup per block (decode variant 4) and at the library's own choice (0).  Then
    every invalid twin in a call of its own between two healthy items."""
    valid = list(CATALOGUE.valid.items())
    blobs = [one_block(ext, stream, plain) for _, (ext, stream, plain) in valid]
    plains = [np.frombuffer(plain, dtype=np.uint8) for _, (_, _, plain) in valid]
    sizes, lengths = [b.size for b in blobs], [p.size for p in plains]
    rng = np.random.default_rng(13)
    stalls = 0
    for align in (1, 16):
        offsets = tsq.plan_packed(sizes, align)
        arena = rng.integers(1, 256, offsets[-1], dtype=np.uint8)
        for b, o in zip(blobs, offsets):
            arena[o:o + b.size] = b
        if align == 1:
            assert {o % 16 for o in offsets[:-1]} == set(range(16))
        for variant in (4, 0):
            status, got, back, outs = packed_decode(tsq, codec, arena, offsets, sizes, lengths, rng, variant)
            if variant == 0 and status == ERR_STALL:
                # the documented outcome of a decode on several workgroups per block on a busy machine, and its remedy
                stalls += 1
                print(f"packed decode (align {align}) at decode variant 0 reported TSQA_ERR_STALL: decoding again with decode variant 4")
                status, got, back, outs = packed_decode(tsq, codec, arena, offsets, sizes, lengths, rng, 4)
            assert status == 0, (align, variant, status)
            assert got == lengths, [(n, g, w) for (n, _), g, w in zip(valid, got, lengths) if g != w]
            for (name, _), a, p in zip(valid, outs, plains):
                assert np.array_equal(back[a:a + p.size], p), (name, align, variant)
    print(f"packed decode: {stalls} stall(s) at decode variant 0")
    for _ in valid:
        count("packed_decompress")

    healthy = CATALOGUE.valid["soup_5000_default_noext"]
    hb, hn = one_block(*healthy), len(healthy[2])
    for name, (ext, stream) in CATALOGUE.invalid.items():
        twin = np.frombuffer(streamgen.bad_container(ext, stream), dtype=np.uint8)
        three = [hb, twin, hb]
        sizes = [b.size for b in three]
        offsets = tsq.plan_packed(sizes, 1)
        status, got, _, _ = packed_decode(tsq, codec, np.concatenate(three), offsets, sizes, [hn, MiB4 + 64, hn], rng, 4)
        assert status == refusal_code(stream), (name, status)
        if status == ERR_FORMAT:
            assert got[1] == 0, (name, got)
        count("packed_decompress")


def test_every_case_ran_through_every_entry_point():
    n = len(CATALOGUE.valid) + len(CATALOGUE.invalid)
    # the catalogue's own floor (streamgen's families: tests/golden/conformance_streams.json pins the exact set): a catalogue that
    # shrank on this machine must not pass by shrinking both sides of the comparison below
    assert len(CATALOGUE.valid) >= 150 and len(CATALOGUE.invalid) >= 40, (len(CATALOGUE.valid), len(CATALOGUE.invalid))
    print("conformance counts:", n, dict(sorted(COUNTS.items())))
    entries = ["block_api", "range_read", "batch_decompress", "batch_records", "packed_decompress"] \
        + [f"decompress_variant_{v}" for v in (0, 1, 3, 4, 5, 6)]
    assert {k: COUNTS.get(k, 0) for k in entries} == {k: n for k in entries}
