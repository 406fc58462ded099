"""GPU side of the encoder catalogue (tests/encgen.py): every case, at both levels, through every encoder layout and every encode entry
point, must be byte for byte the oracle's stream / container and come back through the default decoder.  That the oracle's streams are
the compiled reference's, that the catalogue reaches every seam of its census and tells every mutant from the truth is what
test_encoder_catalogue_cpu.py and tests/golden/encoder_catalogue.json establish.

No case is dropped: each entry point counts the cases it ran and the last test compares the counts with the catalogue's size."""
import os
import types

import numpy as np
import pytest

import encgen
import packedgen
from test_gpu_packed import call_packed, round_trip
from test_gpu_parity import codec, to_bytes, to_dev, tsq  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

COUNTS: dict = {}
CASES = encgen.catalogue()


def count(entry):
    COUNTS[entry] = COUNTS.get(entry, 0) + 1


def same(got, want, case, ext, entry):
    if got != want:
        first = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail(f"case {case.name}, ext={ext}, {entry}: {len(got)} bytes against the oracle's {len(want)}, first difference at "
                    f"stream offset {first}; the case aims at {case.aims[ext]}")


@pytest.fixture(scope="module")
def wanted(oracle):
    """the oracle's container of every case, per level"""
    return {(c.name, ext): oracle.compress(np.frombuffer(c.data, dtype=np.uint8), ext, threads=2) for c in CASES for ext in (0, 1)}


def test_block_api_with_and_without_the_halo(tsq, oracle):
    for case in CASES:
        for ext in (0, 1):
            for data, halo in case.blocks():
                got = tsq.tsq_encode(data, ext)
                same(got, oracle.encode_block(data, ext), case, ext, "tsq_encode without halo")
                assert tsq.tsq_decode(got, ext) == data, (case.name, ext)
                if halo is not None:
                    got = tsq.tsq_encode(data, ext, halo=halo)
                    same(got, oracle.encode_block(data, ext, halo), case, ext, "tsq_encode with halo")
                    assert tsq.tsq_decode(got, ext) == data, (case.name, ext)
        count("block_api")


@pytest.mark.parametrize("variant", [1, 7, 6, 0])
def test_container_at_every_encoder_layout(tsq, codec, wanted, variant):
    """1: the serial encoder; 7: the staged encoder's standard layout; 6: its lean layout; 0: the library's own choice"""
    try:
        for case in CASES:
            src = to_dev(np.frombuffer(case.data, dtype=np.uint8))
            for ext in (0, 1):
                codec.set_variant(variant, 0)
                blob = codec.compress(src, ext)
                same(to_bytes(blob), wanted[case.name, ext], case, ext, f"compress at encoder variant {variant}")
                codec.set_variant(0, 0)
                assert to_bytes(codec.decompress(blob)) == case.data, (case.name, ext, variant)
            count(f"compress_variant_{variant}")
    finally:
        codec.set_variant(0, 0)


@pytest.mark.parametrize("variant", [7, 6])
def test_all_cases_of_a_level_as_one_batch(tsq, codec, wanted, variant):
    """enc_batch_kernel: the small cases sit side by side on the chip"""
    srcs = [to_dev(np.frombuffer(c.data, dtype=np.uint8)) for c in CASES]
    try:
        for ext in (0, 1):
            codec.set_variant(variant, 0)
            blobs = codec.compress_batch(srcs, ext)
            codec.set_variant(0, 0)
            assert len(blobs) == len(CASES)
            for case, blob in zip(CASES, blobs):
                same(to_bytes(blob), wanted[case.name, ext], case, ext, f"compress_batch at encoder variant {variant}")
                assert to_bytes(codec.decompress(blob)) == case.data, (case.name, ext, variant)
        for case in CASES:
            count(f"batch_variant_{variant}")
    finally:
        codec.set_variant(0, 0)


@pytest.fixture(scope="module")
def packed_input(oracle, wanted):
    """packedgen.catalogue_arena on the device, and per level the oracle's container of every item of it"""
    arena, items = packedgen.catalogue_arena(CASES)
    datas = [np.frombuffer(packedgen.item_bytes(it), dtype=np.uint8) for it in items]
    batch = types.SimpleNamespace(d_in=to_dev(arena), items=[(at, ln, 0, 0) for _, at, ln, _ in items], datas=datas)
    want = {ext: [oracle.compress(d, ext, threads=2) if it[3] else wanted[it[0].name, ext] for it, d in zip(items, datas)] for ext in (0, 1)}
    return batch, items, want


@pytest.mark.parametrize("variant", [7, 6])
def test_all_cases_of_a_level_as_one_packed_batch(tsq, codec, packed_input, variant):
    """tsqa_compress_batch_packed over one input arena (packedgen.catalogue_arena): every case with the next case's bytes directly
    behind its last byte, and every case that carries a halo once more with that halo behind it -- the bytes its builder chose to
    continue its last match -- as two overlapping input ranges.  Each container must be the oracle's container of the item alone:
    the encoder's look-ahead ends at the item's last byte.  Both staged layouts; align 1, 16 and 4096 occur."""
    batch, items, want = packed_input
    assert [it[0] for it in items[:len(CASES)]] == CASES
    try:
        for ext in (0, 1):
            align = {(7, 0): 1, (7, 1): 16, (6, 0): 4096, (6, 1): 1}[variant, ext]
            lengths = [len(w) for w in want[ext]]
            plan = tsq.plan_packed(lengths, align)
            codec.set_variant(variant, 0)
            host, guard, offsets, sizes, rc = call_packed(codec, batch, ext, align, plan[-1] + 5000)
            codec.set_variant(0, 0)
            assert rc == 0, codec.last_error()
            entry = f"compress_batch_packed (align {align}) at encoder variant {variant}"
            assert offsets == tsq.plan_packed(sizes, align), f"{entry}: the places do not follow the layout rule for the sizes given"
            untouched = np.ones(host.size, dtype=bool)
            for k, (it, w) in enumerate(zip(items, want[ext])):
                # (where a size is wrong the places behind it move: the bytes at the place the device reports, of the length it reports)
                got = host[offsets[k]:offsets[k] + sizes[k]].tobytes()
                same(got, w, it[0], ext, entry + (", second copy with its halo" if it[3] else ", second copy before its halo" if k >= len(CASES) else ""))
                untouched[offsets[k]:offsets[k] + sizes[k]] = False
            assert sizes == lengths
            assert offsets == plan
            assert np.array_equal(host[untouched], guard[untouched]), "bytes outside the containers were written"
            round_trip(codec, batch, host, offsets, sizes)
        for case in CASES:
            count(f"packed_variant_{variant}")
    finally:
        codec.set_variant(0, 0)


@pytest.mark.parametrize("variant", [0, 6])
def test_small_cases_under_jitter(tsq, codec, wanted, variant):
    """the hand-off stress build delays every publication by a pseudo-random time that differs from block to block: the small cases,
    three times over in one batch, so that every case runs under three delay patterns; the larger ones one container at a time"""
    assert os.path.exists(tsq.lib_path("jitter")), "run __graft_entry__.build() first"
    c = tsq.DeviceCodec(0, ab="jitter")
    try:
        small = [case for case in CASES if len(case.data) <= encgen.SMALL]
        large = [case for case in CASES if len(case.data) > encgen.SMALL]
        srcs = [to_dev(np.frombuffer(case.data, dtype=np.uint8)) for case in small]
        c.set_variant(variant, 0)
        for ext in (0, 1):
            blobs = c.compress_batch(srcs * 3, ext)
            assert len(blobs) == 3 * len(small)
            for k, blob in enumerate(blobs):
                case = small[k % len(small)]
                same(to_bytes(blob), wanted[case.name, ext], case, ext, f"jitter compress_batch (copy {k // len(small)}) at encoder variant {variant}")
            for case in large:
                blob = c.compress(to_dev(np.frombuffer(case.data, dtype=np.uint8)), ext)
                same(to_bytes(blob), wanted[case.name, ext], case, ext, f"jitter compress at encoder variant {variant}")
            for k, case in enumerate(small):
                assert to_bytes(codec.decompress(blobs[k])) == case.data, (case.name, ext, variant)
        for case in CASES:
            count(f"jitter_variant_{variant}")
    finally:
        c.close()


def test_every_case_ran_through_every_entry_point():
    n = len(CASES)
    assert n >= 80, n                                        # tests/golden/encoder_catalogue.json pins the exact set
    print("encoder catalogue counts:", n, dict(sorted(COUNTS.items())))
    entries = ["block_api"] + [f"compress_variant_{v}" for v in (1, 7, 6, 0)] + [f"batch_variant_{v}" for v in (7, 6)] \
        + [f"packed_variant_{v}" for v in (7, 6)] + [f"jitter_variant_{v}" for v in (0, 6)]
    assert {k: COUNTS.get(k, 0) for k in entries} == {k: n for k in entries}
