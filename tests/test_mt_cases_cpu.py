"""The inputs of tests/mtgen.py reach what they aim at.  CPU only: the restated schedule, the oracle's verdict on every container, the
look-ahead criterion.  (What the scheduler makes of them is test_gpu_mt_conformance.py's.)"""
import os

import mtgen
from streamgen import CATALOGUE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restated_schedule_gives_the_stated_batches():
    assert mtgen.RAMP_COUNTS == (63, 64, 70, 73, 113)
    want = {63: [32, 31],                   # not ramped: one batch per lane, at least 32 blocks
            64: [8, 12, 18, 26],            # the threshold: a sixteenth is below 8, so 8, then half again each time
            70: [8, 12, 18, 32],            # 27 would leave 5: the crumb is merged
            73: [8, 12, 18, 27, 8],         # 27 leaves exactly 8: not merged
            113: [8, 12, 18, 27, 40, 8]}    # one step further, again a tail of exactly 8
    for n, sizes in want.items():
        assert mtgen.decompress_schedule(n) == sizes and sum(sizes) == n
    assert mtgen.decompress_schedule(70, ramp=False) == [32, 32, 6]
    got = {name: sizes for name, _, _, sizes in mtgen.ramp_containers()}
    assert [got[f"ramp_{n}"] for n in want] == list(want.values()) and got["uneven_unit"] == [6] and got["regions"] == [18]
    # the lines that are restated are still the source's
    src = open(os.path.join(ROOT, "turbosqueeze_amd", "csrc", "tsq_compat.hip")).read()
    for text in ("nb < 64 || getenv(\"TSQ_AMD_NO_RAMP\")", "size = nb / 16u < 8u ? 8u : nb / 16u", "if (left - take < 8u) take = left;",
                 "size += size / 2u;", "const uint32_t cut = per_lane < 32u ? 32u : per_lane;", "env_size(\"TSQ_AMD_LANES\", 4)",
                 "env_size(\"TSQ_AMD_BATCH_BLOCKS\", 512)", "got = total - at < n + kHalo ? total - at : n + kHalo"):
        assert text in src, f"tsq_compat.hip no longer says `{text}`: re-derive tests/mtgen.py"


def test_oracle_decodes_every_valid_container(oracle):
    ramp = mtgen.ramp_containers()
    for name, blob, plain, sizes in ramp:
        assert mtgen.block_count(blob) == sum(sizes) and int.from_bytes(blob[8:16], "little") == len(plain), name
        assert oracle.decompress(blob, threads=4) == plain, name
    assert all(len(plain) < 12 << 20 for _, _, plain, _ in ramp)              # sizes: nothing above the uneven unit's order
    blob, plain = mtgen.healthy_six()
    assert oracle.decompress(blob) == plain
    for blob, plain in mtgen.damage_bases():
        assert 8 <= mtgen.block_count(blob) <= 12 and len(blob) < 400_000
        assert oracle.decompress(blob) == plain


def test_oracle_rejects_every_twin_container(oracle):
    twins = mtgen.twin_containers()
    assert [t[0] for t in twins] == list(CATALOGUE.invalid) and len(twins) >= 40
    assert {k for _, _, k, _ in twins} == set(mtgen.TWIN_PLACES)
    kinds = [kind for *_, kind in twins]
    assert kinds.count("walk") == 2 and kinds.count("stream") == len(twins) - 2
    healthy = CATALOGUE.valid[mtgen.HEALTHY]
    for name, blob, k, kind in twins:
        assert mtgen.block_count(blob) == 6
        assert oracle.decompress(blob) is None, name
        # the blocks around the twin are sound: block k alone makes the verdict
        for b, (at, ln) in enumerate(mtgen.frames_of(blob)):
            if b != k:
                assert blob[at:at + ln] == healthy[1], (name, b)


def test_damaged_cases_split_both_ways_and_the_header_cases_are_on_record(oracle):
    cases = mtgen.damaged_containers()
    assert len(cases) == 120 + 11 and len({n for n, _ in cases}) == len(cases)
    assert cases == mtgen.damaged_containers()                   # seeded
    bases = mtgen.damage_bases()
    plains = [p for _, p in bases]
    accepted = rejected = changed = 0
    for name, blob in cases[:120]:
        assert blob[:16] in [b[:16] for b, _ in bases], name     # (offsets >= 16: the header is whole)
        got = oracle.decompress(blob)
        if got is None:
            rejected += 1
        else:
            accepted += 1
            changed += got not in plains
            assert mtgen.expected_of_the_scheduler(oracle, blob) in (got, None), name
    # a condition on the inputs, not on the library: both verdicts occur often, and accepted cases decode to other bytes
    assert accepted >= 15 and rejected >= 15 and changed >= 15, (accepted, rejected, changed)
    record = mtgen.header_and_tail_record()
    assert [n for n, _ in cases[120:]] == list(record)
    for name, blob in cases[120:]:
        got = oracle.decompress(blob)
        assert (None if got is None else len(got)) == record[name], name
        if got is not None:
            assert got == plains[0][:len(got)], name
    # the scheduler's expectation: the oracle's, and a refusal where the frames do not make the header's total
    want = {name: mtgen.expected_of_the_scheduler(oracle, blob) for name, blob in cases[120:]}
    assert [n for n, w in want.items() if w is not None] == ["trailing_1", "trailing_100"]
    assert want["trailing_1"] == want["trailing_100"] == plains[0]


def test_every_kept_lookahead_case_meets_its_criterion(oracle):
    a, kept = mtgen.lookahead_jobs(oracle)
    assert len(a) == 2 * mtgen.BLOCK + 5000 and 0 not in a
    names = [n for n, _, _ in kept]
    assert mtgen.lookahead_dropped(oracle) == ["catalogue_full_block"]
    # (the catalogue's own whole-block case ends in a match that only a continuing look-ahead lengthens: it does not meet the
    #  criterion, so the kept cases are the built ones -- mtgen.lookahead_candidates says how they are built)
    assert "built_one_block_match_over_zeros" in names and "built_two_blocks_match_over_zeros" in names
    assert [n for n in names if n.startswith("built_block_plus_")] == [f"built_block_plus_{n}" for n in range(1, 9)]
    for name, b, ext in kept:
        assert mtgen.lookahead_differs(oracle, a, b, ext, mtgen.MEM_BATCH), name
        assert len(b) % mtgen.BLOCK == 0 or mtgen.BLOCK < len(b) <= mtgen.BLOCK + 8, name
    # the criterion once more, from the other side, and for the streamed runs (one block per batch): the block's stream differs when
    # the bytes behind the input do
    name, b, ext = kept[0]
    assert len(b) == mtgen.BLOCK
    assert oracle.encode_block(b, ext) != oracle.encode_block(b, ext, halo=a[len(b):len(b) + mtgen.HALO]), name
    assert mtgen.lookahead_differs(oracle, a, b, ext, mtgen.FILE_BATCH), name
    name, b, ext = kept[-1]                                      # a block and 8 bytes: the first block's look-ahead shows it
    assert mtgen.lookahead_differs(oracle, a, b, ext, mtgen.FILE_BATCH), name
