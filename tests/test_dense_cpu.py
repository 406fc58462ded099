"""CPU side of the dense decompress of a packed batch: tsqa_plan_dense (host only) against the Python restatement of the layout rule
on every batch of tests/densegen.py, and the facts that make each batch a test of what it aims at -- sums that cross the scan's
24-bit split inside a wavefront and across a wavefront edge, the edges of the 256-item loop, a block sum that is not the item
number, totals around a multiple of align, one refusal per rule with the oracle's own verdict, and the fitting prefix of every cut.
No kernel runs here; test_gpu_dense.py runs the same batches on the device."""
import ctypes as C

import numpy as np
import pytest

import densegen as dg


@pytest.fixture(scope="module")
def tsq():
    import turbosqueeze_amd
    return turbosqueeze_amd


def check_plan(tsq, b, out_size, cap_blocks):
    want = dg.layout(b.totals, b.blocks, b.align, out_size, cap_blocks)
    got = tsq.plan_dense(b.totals, b.blocks, b.align, out_size, cap_blocks)
    assert got == want, f"{b.name}: tsqa_plan_dense and the restatement differ (out_size {out_size}, cap_blocks {cap_blocks})"
    return want


def test_plan_dense_agrees_with_the_restatement_on_every_batch(tsq):
    for b in dg.every_batch():
        offsets, first, n_fit = check_plan(tsq, b, b.need_bytes, b.need_blocks)
        assert n_fit == len(b.items) and offsets[-1] == b.need_bytes and first[-1] == b.need_blocks == sum(b.blocks)
        # measuring: nothing fits, the first accepted item ends the prefix
        assert check_plan(tsq, b, 0, 0)[2] == next(k for k, nb in enumerate(b.blocks) if nb)
    b, table = dg.cuts()
    for what, out_size, cap_blocks, n_fit in table:
        assert check_plan(tsq, b, out_size, cap_blocks)[2] == n_fit, what


def test_plan_dense_refuses_bad_arguments(tsq):
    L = tsq.lib()
    tot, nb = (C.c_uint64 * 2)(5, 6), (C.c_uint32 * 2)(1, 1)
    offs, first, n_fit = (C.c_uint64 * 3)(7, 7, 7), (C.c_uint64 * 3)(7, 7, 7), C.c_uint32(7)
    ok = lambda **kw: L.tsqa_plan_dense(kw.get("tot", tot), kw.get("nb", nb), kw.get("n", 2), kw.get("align", 16), 100, 10, kw.get("offs", offs),
                                        kw.get("first", first), kw.get("fit", C.byref(n_fit)))
    for bad in (dict(tot=None), dict(nb=None), dict(offs=None), dict(first=None), dict(fit=None), dict(n=0), dict(align=0), dict(align=24),
                dict(align=8192)):
        assert ok(**bad) == dg.ERR_ARG, bad
    assert list(offs) == [7, 7, 7] and list(first) == [7, 7, 7] and n_fit.value == 7
    assert ok() == 0 and list(offs) == [0, 16, 22] and list(first) == [0, 1, 2] and n_fit.value == 2


def test_a_refused_item_takes_no_room_whatever_its_total(tsq):
    assert tsq.plan_dense([10, 1 << 60, 3], [1, 0, 2], 16, 19, 3) == ([0, 16, 16, 19], [0, 1, 1, 3], 3)
    assert tsq.plan_dense([10, 1 << 60, 3], [1, 0, 2], 16, 18, 3)[2] == 2 and tsq.plan_dense([10, 1 << 60, 3], [1, 0, 2], 16, 19, 2)[2] == 2


def test_carry_totals_cross_the_split(tsq):
    for b in dg.carry_totals():
        dg.carry_reach(b)
        check_plan(tsq, b, b.need_bytes, b.need_blocks)


def test_loop_edges_carry_both_sums(tsq):
    assert [len(b.items) for b in dg.loop_edges()] == list(dg.LOOP_COUNTS) == [1, 255, 256, 257, 513]
    for b in dg.loop_edges():
        dg.loop_reach(b)


def test_two_block_item_shifts_the_block_table():
    b = dg.two_blocks()
    first = dg.layout(b.totals, b.blocks, b.align, 0, 0)[1]
    assert b.blocks[4] == 2 and b.totals[4] == dg.BLOCK + 1 and 0 < 4 < len(b.items) - 1
    assert first[:5] == [0, 1, 2, 3, 4] and first[5:] == [k + 1 for k in range(5, len(b.items) + 1)]


@pytest.mark.parametrize("align", dg.ALIGNS)
def test_alignment_totals_sit_around_a_multiple(align):
    dg.alignment_reach(dg.alignment(align))


def test_refusals_one_per_rule_between_healthy_items(oracle):
    b = dg.refusals()
    dg.refusal_reach(b, oracle)
    _, _, status, sizes = b.expect(b.need_bytes, b.need_blocks)
    assert [s for s in status if s] == [dg.ERR_FORMAT] * 8 + [dg.ERR_STREAM]
    # the walk-refused items keep the room their headers ask for; the header-refused ones take none
    offsets = dg.layout(b.totals, b.blocks, b.align, 0, 0)[0]
    for k, it in enumerate(b.items):
        assert (offsets[k + 1] == offsets[k]) == (b.blocks[k] == 0), it.name


def test_healthy_items_are_what_the_oracle_decodes(oracle):
    for b in (dg.two_blocks(), dg.refusals(), dg.alignment(16)):
        for it in b.items:
            if it.want is not None:
                assert oracle.decompress(it.blob) == it.want, it.name


def test_cuts_expect_the_fitting_prefix():
    b, table = dg.cuts()
    assert b.blocks[4] == 2 and b.blocks[7] == 0
    assert [n_fit for *_, n_fit in table] == [12, 11, 11, 6, 8, 4, 0]
    for what, out_size, cap_blocks, n_fit in table:
        offsets, first, status, sizes = b.expect(out_size, cap_blocks)
        assert status[7] == dg.ERR_FORMAT, what
        assert [s for k, s in enumerate(status) if k != 7] == [0 if k < n_fit else dg.ERR_OVERFLOW for k in range(12) if k != 7], what
        assert offsets[-1] == b.need_bytes and first[-1] == b.need_blocks, "the tables do not depend on the room"
        fit_end = max((offsets[k] + b.totals[k] for k in range(12) if status[k] == 0), default=0)
        assert fit_end <= out_size and sum(b.blocks[k] for k in range(12) if status[k] == 0) <= cap_blocks
