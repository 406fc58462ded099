"""CPU side of the encoder catalogue (tests/encgen.py): the catalogue reaches every seam its census names, tells every mutant of the
oracle's encoder from the truth, and gives the streams pinned in tests/golden/encoder_catalogue.json (which were compared with the
compiled reference when they were made: tests/golden/make_encoder_catalogue.py).  No GPU, no reference build needed."""
import json
import os

import pytest

import encgen
import kat
from oracle import pyoracle as po

PINS = json.load(open(os.path.join(kat.GOLDEN, "encoder_catalogue.json")))


@pytest.fixture(scope="module")
def regenerated(oracle):
    return encgen.pins(oracle)


def test_catalogue_is_the_pinned_one_and_was_checked_against_the_reference(regenerated):
    assert sorted(regenerated) == sorted(PINS)
    assert len(PINS) >= 80
    for name, want in PINS.items():
        assert want["reference_checked"] is True, name
        got = regenerated[name]
        assert (got["input"], got["bytes"]) == (want["input"], want["bytes"]), f"{name}: the builder no longer gives the pinned input"
        for ext in ("0", "1"):
            assert got["levels"][ext]["streams"] == want["levels"][ext]["streams"], f"{name} ext={ext}: stream differs from the pinned one"
            assert got["levels"][ext]["census"] == want["levels"][ext]["census"], f"{name} ext={ext}: census differs from the pinned one"


def test_every_aimed_counter_is_hit(regenerated):
    missed = []
    for case in encgen.catalogue():
        for ext in (0, 1):
            known = set(encgen.counter_names(ext))
            census = regenerated[case.name]["levels"][str(ext)]["census"]
            for aim in case.aims[ext]:
                assert aim in known, (case.name, ext, aim)
                if census.get(aim, 0) < 1:
                    missed.append((case.name, ext, aim))
    assert not missed, missed


def test_every_counter_is_hit_by_the_catalogue_at_each_level(regenerated):
    for ext in (0, 1):
        total = dict.fromkeys(encgen.counter_names(ext), 0)
        for entry in regenerated.values():
            for k, v in entry["levels"][str(ext)]["census"].items():
                total[k] += v
        print(f"census over the catalogue, ext={ext}:", total)
        assert [k for k, v in total.items() if v < 1] == [], ext


def test_every_mutant_is_killed(oracle):
    inputs = [(f"{c.name}#{b}", d, h) for c in encgen.catalogue() for b, (d, h) in enumerate(c.blocks())]
    kills = encgen.kill_matrix(oracle, inputs)
    assert sorted(kills) == sorted(po.MUTANTS[1:])
    for mutant, hits in kills.items():
        still_decodes = sorted({name for name, _, ok in hits if ok})[:3]
        broken = sorted({name for name, _, ok in hits if not ok})[:3]
        print(f"{mutant}: {len(hits)} kills; stream still decodes to the input in {still_decodes}, does not in {broken}")
        if mutant in encgen.EQUIVALENT_MUTANTS:
            # the table starts as zeros and position 0's entry is the value 0: no input can tell this mutant from the truth
            assert hits == [], mutant
        else:
            assert hits, f"no catalogue case tells mutant {mutant} from the oracle"
