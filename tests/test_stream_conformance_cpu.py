"""CPU side of the decoder conformance catalogue (tests/streamgen.py), on 100 % of it.

The premise: every stream the rest of the suite gives a decoder is an encoder's output (ours, the oracle's, the reference's: the
same greedy encoder by construction) or such an output with a few bytes damaged, and that encoder never emits a match shorter than
4 bytes or an offset outside [4, 0xFFFE] (oracle/tsq_oracle.c:111-112, 177-180) -- test_encoder_never_emits_what_the_catalogue_adds
asserts exactly that; if an encoder change widens the set, it fails and this claim no longer holds.

Valid cases: the model (streamgen.model_decode), the oracle's decoder and, where oracle/_ref is built, the compiled reference
decoder all give the builder's plain bytes.  Invalid twins: the model and the oracle reject them (the reference decoder validates
nothing and is not run on them).  tests/golden/conformance_streams.json pins every case by digest and records the reference's
verdict, which is how that verdict reaches a machine that has no reference."""
import json
import os

import numpy as np
import pytest

import fuzzgen
import kat
import streamgen
from streamgen import CATALOGUE

PINNED = os.path.join(kat.GOLDEN, "conformance_streams.json")


def hexd(b):
    return "%016x" % fuzzgen.stream_digest(b)


def test_model_and_oracle_give_the_builders_bytes(oracle):
    ran = 0
    for name, (ext, stream, plain) in CATALOGUE.valid.items():
        assert streamgen.model_decode(stream, ext) == plain, name
        got, status = oracle.decode_block(stream, ext)
        assert status == 0 and got == plain, (name, status)
        ran += 1
    assert ran == len(CATALOGUE.valid) >= 150


def test_reference_decoder_gives_the_builders_bytes(reference):
    ran = 0
    for name, (ext, stream, plain) in CATALOGUE.valid.items():
        assert reference.decode_block(stream, ext) == plain, name
        ran += 1
    assert ran == len(CATALOGUE.valid)


def test_invalid_twins_are_rejected_by_model_and_oracle(oracle):
    ran = 0
    for name, (ext, stream) in CATALOGUE.invalid.items():
        assert streamgen.model_decode(stream, ext) is None, name
        got, status = oracle.decode_block(stream, ext)
        assert status != 0 and got == b"", (name, status)
        assert oracle.decompress(streamgen.bad_container(ext, stream)) is None, name
        ran += 1
    assert ran == len(CATALOGUE.invalid) >= 40
    # every rule, at every place the issue names
    for rule in ("off_eq_origin_plus_1", "take_eq_off_plus_1", "offset_second_byte_missing", "literal_take_minus_1_bytes_present",
                 "control_byte_missing", "size_byte_missing"):
        for where in ("first_chunk", "chunk_edge", "last_symbol"):
            assert any(n.startswith(f"twin_{rule}_{where}") for n in CATALOGUE.invalid), (rule, where)
    assert "twin_size_word_4MiB_plus_1_noext" in CATALOGUE.invalid and "twin_size_1_with_a_3_byte_stream_ext" in CATALOGUE.invalid
    assert len(set(CATALOGUE.invalid.values())) == len(CATALOGUE.invalid)          # forty different streams


def test_containers_of_catalogue_blocks(oracle):
    """the containers the GPU tests assemble: uneven blocks (0, 1, 4 MiB, 77, 0, about 3 MiB), ext bits mixed per frame"""
    for blocks in (streamgen.uneven_unit(), streamgen.region_container()[0], streamgen.blocks_for(40)):
        blob = streamgen.container(blocks)
        assert oracle.decompress(blob, threads=4) == b"".join(p for _, _, p in blocks)
    for name, (ext, stream, plain) in CATALOGUE.valid.items():
        assert oracle.decompress(streamgen.container([(ext, stream, plain)])) == plain, name


def test_catalogue_reaches_the_geometry_it_aims_at():
    """the structure constants restated in streamgen.py are the source's (tsq_dec_common.cuh:48-61), and the builders reached them"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "turbosqueeze_amd", "csrc", "tsq_dec_common.cuh")).read()
    for text in ("S = 6144;", "OUTC = 2 * S;", "HOP = 16;", "MAXG = 512;", "MAXSN = MAXG / HOP + 2;", "R = 65536 + OUTC + 64;",
                 "excl + 512u + 16u > C::OUTC", "768u * wid"):
        assert text in src, f"tsq_dec_common.cuh no longer says `{text}`: re-derive the geometry families of tests/streamgen.py"
    assert (streamgen.S, streamgen.OUTC, streamgen.MAXG, streamgen.MAXSN, streamgen.R) == (6144, 12288, 512, 34, 77888)
    _ = CATALOGUE.valid
    # density switches, per level: a chunk's first group lies at offset 0 and the groups are 13, 21 or 133 bytes long, so a switch
    # can lie at 13 a + 21 b + 133 c; at least nine in ten of those offsets below S are hit (the block's 4 MiB end the walk), all
    # six ordered transitions occur a thousand times and more, and the case holds matches
    for tag in ("noext", "ext"):
        f = CATALOGUE.facts[f"switch_{tag}"]
        assert f["reachable"] == 6024 and f["chunk_offsets"] * 10 >= f["reachable"] * 9, (tag, f)
        assert len(f["transitions"]) == 6 and min(f["transitions"].values()) >= 1000, (tag, f)
        assert f["matches"] >= 30000 and f["chunks"] >= 300, (tag, f)
        trace = []
        ext, stream, plain = CATALOGUE.valid[f"density_switches_{tag}"]
        assert streamgen.model_decode(stream, ext, trace=trace) == plain
        assert sum(1 for t in trace if t[0] == 0) == f["matches"]
    # ext: chunks that the image budget cuts lie next to chunks that end with their stream byte S
    f = CATALOGUE.facts["switch_ext"]
    assert f["cut_chunks"] >= 20 and f["chunks"] - f["cut_chunks"] >= 100 and f["long_runs"] >= 10, f
    assert CATALOGUE.facts["switch_noext"]["cut_chunks"] == 0
    # the group across a chunk's edge: every split of a 13-byte group, the listed ones of a 133-byte group (0: the group starts the
    # next chunk), on the decoders' rolling chunks and on a grid of S bytes
    for kind in ("rolling", "grid"):
        assert CATALOGUE.facts[f"edge13_{kind}"] == list(range(14)), kind
        assert CATALOGUE.facts[f"edge133_{kind}"] == [0, 1, 2, 3, 17, 66, 67, 116, 131, 132, 133], kind
    # no two cases are the same bytes at the same level
    keys = [(e, st) for e, st, _ in CATALOGUE.valid.values()] + list(CATALOGUE.invalid.values())
    assert len(set(keys)) == len(keys)
    assert CATALOGUE.facts["stream_residues"] == 16                # stream lengths at every residue mod 16
    assert len(CATALOGUE.valid["stream_of_exactly_TSQ_OUTPUT_SZ_noext"][1]) == streamgen.OUTPUT_SZ
    assert any(len(p) == streamgen.BLOCK for _, _, p in CATALOGUE.valid.values())
    # the densest chunk holds S / 13 + 1 = 473 groups, in MAXG = 512 and in MAXSN = 34 super nodes of HOP groups
    assert streamgen.S // 13 + 1 <= streamgen.MAXG and -(-(streamgen.S // 13 + 1) // streamgen.HOP) <= streamgen.MAXSN


def test_catalogue_is_the_pinned_one():
    pinned = json.load(open(PINNED))
    mine = {}
    for name, (ext, stream, plain) in CATALOGUE.valid.items():
        mine[name] = {"ext": ext, "stream": hexd(stream), "plain": hexd(plain)}
    for name, (ext, stream) in CATALOGUE.invalid.items():
        mine[name] = {"ext": ext, "stream": hexd(stream), "plain": None}
    assert sorted(mine) == sorted(pinned), sorted(set(mine) ^ set(pinned))
    for name, entry in mine.items():
        got = {k: pinned[name][k] for k in ("ext", "stream", "plain")}
        assert got == entry, f"{name}: the generator no longer produces the pinned case (numpy or builder change?)"
        if entry["plain"] is not None:
            assert pinned[name]["reference_agrees"] is True, f"{name}: the fixture does not record the reference decoder's agreement"
        else:
            assert pinned[name]["reference_agrees"] is None


def test_encoder_never_emits_what_the_catalogue_adds(oracle):
    """Over the corpus of test_fuzz_containers_vs_oracle (both levels): no match shorter than 4 bytes, no offset outside [4, 0xFFFE].
    (A source at byte 0 of the block, off == origin, does occur in encoder output: the zeroed hash table makes position 0 the
    candidate of every hash not seen yet, tsq_oracle.c:150.  The catalogue still places it on purpose, with short matches.)"""
    rng = np.random.default_rng(2024)
    symbols = matches = 0
    for case in range(120):
        n = int(rng.integers(1, 200000)) if case % 4 else int(rng.integers(1, 64))
        data = fuzzgen.structured(rng, n).tobytes()
        for ext in (0, 1):
            stream = oracle.encode_block(data, ext)
            trace = []
            assert streamgen.model_decode(stream, ext, trace=trace) == data, (case, ext)
            t = np.array(trace, dtype=np.int64).reshape(-1, 5)
            m = t[t[:, 0] == 0]
            symbols += len(t); matches += len(m)
            if len(m):
                lens = np.where((ext == 1) & (m[:, 1] < 3), (m[:, 1] + 2) << 4, m[:, 1] + 1)
                assert lens.min() >= 4, (case, ext)
                assert m[:, 2].min() >= 4 and m[:, 2].max() <= 0xFFFE, (case, ext)
    assert matches > 100_000 and symbols > matches


# ---------------------------------------------------------------- mutation check: the catalogue notices a subtly wrong decoder

def mutant(kind):
    """model_decode with one rule changed, as a stand-in for a device decoder that is wrong in that way"""
    def decode(stream, ext):
        n = len(stream)
        size = int.from_bytes(stream[:3], "little")
        if n < 3 or size > streamgen.BLOCK:
            return None
        out, i = bytearray(), 3
        chunk_at, groups = 3, 0
        while len(out) < size:
            if i >= n:
                return None
            if i - chunk_at >= streamgen.S:
                chunk_at, groups = i, 0
            groups += 1
            if kind == "maxg_halved" and groups > streamgen.MAXG // 2:
                return None
            ctl = stream[i]; i += 1
            for p in range(4):
                if len(out) >= size:
                    break
                if i >= n:
                    return None
                sb = stream[i]; i += 1
                origin = len(out)
                for s in range(2):
                    room = size - len(out)
                    if room <= 0:
                        break
                    nib = sb >> 4 if s == 0 else sb & 15
                    if (ctl >> (7 - (2 * p + s))) & 1:
                        ln = nib + 1
                        take = min(ln, room)
                        if i + (ln if kind == "clamp_by_len" else take) > n:
                            return None
                        out += stream[i:i + take]; i += ln
                    else:
                        if i + 2 > n:
                            return None
                        off = stream[i] | stream[i + 1] << 8; i += 2
                        ln = streamgen.span(nib, ext)
                        take = min(ln, room)
                        lim = ln if kind == "clamp_by_len" else take
                        if off > origin or (lim >= off if kind == "take_ge_off" else lim > off) or (kind == "min_offset_4" and off < 4):
                            return None
                        out += out[origin - off:origin - off + take]
        return bytes(out)
    return decode


@pytest.mark.parametrize("kind,expect", [
    ("take_ge_off", "ext_long_matches_offset_eq_len"),
    ("min_offset_4", "short_head_noext"),
    ("maxg_halved", "dense13_five_chunks_noext"),
    ("clamp_by_len", "last_match_legal_only_clamped_first_ext"),
])
def test_a_subtly_wrong_decoder_fails_named_cases(kind, expect):
    decode = mutant(kind)
    failing = [name for name, (ext, stream, plain) in CATALOGUE.valid.items() if decode(stream, ext) != plain]
    assert expect in failing, (kind, failing[:10])
    # and the unmutated stand-in is the model
    same = mutant("none")
    for name in list(CATALOGUE.valid)[:40]:
        ext, stream, plain = CATALOGUE.valid[name]
        assert same(stream, ext) == plain
