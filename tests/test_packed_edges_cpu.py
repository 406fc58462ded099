"""CPU-only: the inputs of tests/packedgen.py reach what they aim at.  With the oracle's container sizes and the host-only planners
(plan_batch, plan_packed, batch_bound) alone: the carry batch has sums above 2^24 where the place-making scan carries them, the loop
edge batches end in launches of 256, 257 and 1 items, the overflow cuts fall where they are named and the expected image is made of
container prefixes, the alignment batches hold the three residues, and the encoder catalogue's arena holds every case where its
item says.  A pass of the GPU tests over the same inputs then means that the kernels handled those places."""
import numpy as np
import pytest

import encgen
import packedgen as pg
import turbosqueeze_amd as tsq

CUS = 256       # the GPU tests recompute with the device's count


def sizes_of(oracle, datas, ext):
    return [len(oracle.compress(d, ext, threads=8)) for d in datas]


def test_carry_batch_has_sums_above_2_to_24_where_the_scan_carries_them(oracle):
    cb = pg.carry_batch(CUS)
    assert abs(len(cb.datas) - (2 * CUS + 300)) <= 16 and len(cb.big) == 4
    assert all(64 <= d.size <= 300 for k, d in enumerate(cb.datas) if k not in cb.big)
    assert all(cb.datas[b].size == 4 * pg.MiB4 for b in cb.big)
    sizes = {ext: sizes_of(oracle, cb.datas, ext) for ext in (0, 1)}
    pg.carry_reach(cb, CUS, sizes)
    # spelled out once more, from plan_batch: three big items in launch 0, the fourth in launch 1, tiny items behind each
    ls = pg.launches([d.size for d in cb.datas], CUS)
    (a0, a1, _, _), (c0, c1, _, _) = ls
    assert [b - a0 for b in cb.big[:3]] == [3, 70, 260] and a1 - a0 > 261
    assert c0 <= cb.big[3] < c1 - 1
    for ext in (0, 1):
        assert all(sizes[ext][b] >= 1 << 24 for b in cb.big)
        assert tsq.plan_packed(sizes[ext], 16)[c0] >= 1 << 24


def test_loop_edge_batches_end_in_launches_of_256_257_and_1_items():
    batches = pg.loop_edge_batches(CUS)
    assert [len(b) for b in batches] == [2 * CUS + 256, 2 * CUS + 257, 2 * CUS + 1]
    for datas, last in zip(batches, pg.LOOP_EDGES):
        assert all(d.size <= 300 for d in datas)
        ls = pg.launches([d.size for d in datas], CUS)
        assert len(ls) == 2 and ls[0][:2] == (0, 2 * CUS) and ls[0][3] == 2 * CUS
        assert pg.last_launch_items(datas, CUS) == last
    assert [pg.last_launch_items(b, CUS) for b in batches] == [256, 257, 1]


@pytest.mark.parametrize("which", ["inside", "seam"])
def test_cut_points_and_fitting_image(oracle, which):
    datas, a_at, b_at = pg.inside_batch() if which == "inside" else pg.seam_batch(CUS)
    assert datas[a_at].size == 2 * pg.MiB4 + 1 and datas[b_at].size == 2 * pg.MiB4
    if which == "seam":
        first = pg.first_blocks([d.size for d in datas])
        assert first[a_at] < 2 * CUS < first[a_at + 1] == first[a_at] + 3, "item A does not straddle the first launch seam"
    else:
        assert len(pg.launches([d.size for d in datas], CUS)) == 1
    want = [oracle.compress(d, 1, threads=8) for d in datas]
    sizes = [len(w) for w in want]
    for k in (a_at, b_at):
        align = pg.align_with_padding(sizes, k)
        offsets = tsq.plan_packed(sizes, align)
        roomy = offsets[-1]
        cuts = pg.cut_points(want, offsets, sizes, k)
        assert len(cuts) == 7 and len(set(cuts.values())) == 7, cuts
        assert k != a_at or pg.cut_points(want, offsets, sizes) == cuts           # the default item is the three-block one
        for name, cut in cuts.items():
            assert 16 <= cut < roomy, name
            covered = np.zeros(roomy, dtype=bool)
            for lo, piece in pg.fitting_image(want, offsets, cut):
                assert lo + len(piece) <= cut, name
                assert not covered[lo:lo + len(piece)].any(), name
                covered[lo:lo + len(piece)] = True
            # each item's pieces together are a prefix of its container, and of items wholly below the cut the whole container
            for i, (w, o) in enumerate(zip(want, offsets)):
                got = int(np.count_nonzero(covered[o:o + len(w)]))
                assert covered[o:o + got].all(), (name, i)
                assert got == len(w) or o + len(w) > cut, (name, i)
                assert got in [0, 16] + [at + ln for at, ln in pg.frames_of(w)], (name, i)
            image = np.zeros(roomy, dtype=np.uint8)
            for lo, piece in pg.fitting_image(want, offsets, cut):
                image[lo:lo + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
            for i, (w, o) in enumerate(zip(want, offsets)):
                got = int(np.count_nonzero(covered[o:o + len(w)]))
                assert image[o:o + got].tobytes() == w[:got], (name, i)
        # what each cut leaves of item k
        left = lambda cut: int(sum(len(p) for lo, p in pg.fitting_image(want, offsets, cut) if offsets[k] <= lo < offsets[k + 1]))
        fr = pg.frames_of(want[k])
        ends = [at + ln for at, ln in fr]
        assert left(cuts["header of item k fits, its first frame does not"]) == 16
        assert left(cuts["exactly the end of item k's first frame"]) == ends[0]
        assert left(cuts["one byte short of the end of item k's second frame"]) == ends[0]
        assert left(cuts["exactly the end of item k"]) == sizes[k] == left(cuts["one byte into the padding behind item k"])
        assert left(cuts["the start of item k + 1"]) == sizes[k]
        assert pg.fitting_image(want, offsets, cuts["the start of item k + 1"])[-1][0] < offsets[k + 1]     # nothing of item k + 1
        assert pg.fitting_image(want, offsets, 16) == [(0, want[0][:16])]
        full = pg.fitting_image(want, offsets, roomy)
        image = bytearray(roomy)
        for lo, piece in full:
            image[lo:lo + len(piece)] = piece
        assert all(bytes(image[o:o + len(w)]) == w for w, o in zip(want, offsets))
        assert sum(len(p) for _, p in full) == sum(sizes)


@pytest.mark.parametrize("align", [2, 16, 4096])
def test_alignment_batch_holds_the_three_residues(oracle, align):
    datas = pg.alignment_batch(align)
    assert len(datas) <= 40
    sizes = sizes_of(oracle, datas, 1)
    assert pg.residues_present(sizes, align) == set(pg.RESIDUES)
    offsets = tsq.plan_packed(sizes, align)
    pads = {offsets[k + 1] - offsets[k] - sizes[k] for k in range(len(sizes) - 1)}
    assert {0, 1 % align, align - 1} <= pads


def test_catalogue_arena_item_ranges():
    cases = encgen.catalogue()
    arena, items = pg.catalogue_arena(cases)
    assert [it[0] for it in items[:len(cases)]] == cases
    raw = arena.tobytes()
    for it in items:
        case, in_at, in_len, with_halo = it
        assert raw[in_at:in_at + in_len] == pg.item_bytes(it) and in_len == len(pg.item_bytes(it)), case.name
        assert raw[in_at:in_at + len(case.data)] == case.data, case.name
    # back to back: the byte behind a case is the next case's first byte
    for (a, a_at, a_len, _), (b, b_at, _, _) in zip(items[:len(cases) - 1], items[1:len(cases)]):
        assert a_at + a_len == b_at and raw[b_at] == b.data[0], a.name
    # the second copies: the halo lies right behind the data, and the two ranges overlap
    extra = items[len(cases):]
    haloed = [c for c in cases if c.halo]
    assert len(haloed) >= 30 and len(extra) == 2 * len(haloed)
    for (c, at, ln, h), (c2, at2, ln2, h2) in zip(extra[0::2], extra[1::2]):
        assert c is c2 and at == at2 and not h and h2 and ln2 == ln + len(c.halo)
        assert raw[at + ln:at + ln2] == c.halo, c.name
    assert arena.size < 30 << 20 and not (arena[items[-1][1] + items[-1][2]:] == 0).any()
