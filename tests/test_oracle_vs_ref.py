"""Differential test: oracle/tsq_oracle.c vs the reference's own tsq_encode.cpp/tsq_decode.cpp.
The reference's streams for these inputs are stored as length + digest in tests/golden/ref_streams.npz
(tests/golden/make_golden.py, which also checked that every one decodes back under the reference), so the
test needs no reference build.  CPU only."""
import os

import numpy as np
import pytest

import fuzzgen
import kat

REF = np.load(os.path.join(kat.GOLDEN, "ref_streams.npz"))


def assert_reference_stream(group, i, ext, stream):
    """`stream` is byte for byte the reference's stream of case i of `group`."""
    want = (int(REF[f"{group}_len"][i, ext]), int(REF[f"{group}_digest"][i, ext]))
    assert (len(stream), fuzzgen.stream_digest(stream)) == want, (group, i, ext)


def assert_input(group, i, data, halo):
    assert fuzzgen.stream_digest(data + (halo or b"")) == int(REF[f"{group}_input"][i]), \
        f"case {i} of {group}: not the input the stored reference streams were made from"


@pytest.mark.parametrize("name", sorted(kat.KATS))
def test_kat_bytes_equal_reference(oracle, name):
    i = list(REF["kat_names"]).index(name)
    data = bytes(kat.KATS[name][0]())
    assert_input("kat", i, data, None)
    for ext in (0, 1):
        a = oracle.encode_block(data, ext)
        assert_reference_stream("kat", i, ext, a)
        back, st = oracle.decode_block(a, ext)
        assert st == 0 and back == data


def test_fuzz_small(oracle):
    n_cases = int(os.environ.get("TSQ_FUZZ_CASES", "3000"))
    assert n_cases <= len(REF["small_len"]), f"reference streams are stored for {len(REF['small_len'])} cases"
    for case, (data, halo) in enumerate(fuzzgen.oracle_vs_ref_small(n_cases)):
        assert_input("small", case, data, halo)
        for ext in (0, 1):
            a = oracle.encode_block(data, ext, halo)
            assert_reference_stream("small", case, ext, a)
            back, st = oracle.decode_block(a, ext)
            assert st == 0 and back == data, (case, len(data), ext)


def test_fuzz_large_blocks(oracle):
    for case, (data, halo) in enumerate(fuzzgen.oracle_vs_ref_large()):
        assert_input("large", case, data, halo)
        for ext in (0, 1):
            a = oracle.encode_block(data, ext, halo)
            assert_reference_stream("large", case, ext, a)
            back, st = oracle.decode_block(a, ext)
            assert st == 0 and back == data


def test_traced_form_equals_plain_form_and_reference(oracle):
    """tsqo_encode_block_traced is the same body as tsqo_encode_block (oracle/tsq_oracle.c: encode_body): with mutant 0 its bytes are
    the plain form's and the reference's on the fuzz above, and it writes one record per probed position, none for position 0."""
    n_cases = min(int(os.environ.get("TSQ_FUZZ_CASES", "3000")), len(REF["small_len"]))
    groups = [("small", fuzzgen.oracle_vs_ref_small(n_cases)), ("large", fuzzgen.oracle_vs_ref_large())]
    for group, cases in groups:
        for case, (data, halo) in enumerate(cases):
            for ext in (0, 1):
                a, trace = oracle.encode_block_traced(data, ext, halo)
                assert a == oracle.encode_block(data, ext, halo), (group, case, ext)
                assert_reference_stream(group, case, ext, a)
                assert trace.size >= 1 and int(trace["i"][0]) == 1 and np.all(np.diff(trace["i"].astype(np.int64)) > 0), (group, case, ext)

