"""GPU tests of the packed compress whose item table is made on the device (tsqa_compress_batch_packed_tables_async).  The batches are
those of tests/tablegen.py (test_compress_tables_cpu.py shows that each reaches its aim); every call goes through the C ABI, with
both ext values.  The arena lies between two guards of 4 KiB in a buffer filled with test_gpu_dense.py's pattern, all six output
tables are filled with -1 before the call, and the whole buffer is compared with one image: the pattern, overlaid with the oracle's
containers of the items whose status is 0, at tsqa_plan_packed's places, and with the header and the frames that end inside out_size
of a fitting item that the arena cut.  Padding, both guards and everything past out_size must still hold the pattern."""

import numpy as np
import pytest

import chaingen as cg
import tablegen as tg
from turbosqueeze_amd.api import _batch_array

pytestmark = pytest.mark.gpu

GUARD = 4096
OK, ERR_ARG, ERR_OVERFLOW = tg.OK, tg.ERR_ARG, tg.ERR_OVERFLOW
ROOMY = 1 << 40


@pytest.fixture(scope="module")
def tsq():
    import torch
    assert torch.cuda.is_available()
    import turbosqueeze_amd
    return turbosqueeze_amd


@pytest.fixture(scope="module")
def codec(tsq):
    c = tsq.DeviceCodec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def budget():
    """RE-DERIVE with tsqa_compress_batch_packed_tables_async: an encode launch takes 2 x CUs blocks"""
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def to_dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def words_to_dev(values):
    """64-bit words (up to 2^64 - 1) as an int64 tensor"""
    return to_dev(np.array(values, dtype=np.uint64).view(np.int64))


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (test_gpu_dense.py's pattern)"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


class OnDevice:
    """a batch's input and place tables in device memory"""

    def __init__(self, b):
        self.b, self.n = b, len(b.specs)
        self.data, self.in_offsets, self.in_sizes = to_dev(b.data), words_to_dev(b.in_offsets), words_to_dev(b.in_sizes)


_ON_DEVICE = {}


def on_device(b) -> OnDevice:
    if b.name not in _ON_DEVICE:
        _ON_DEVICE[b.name] = OnDevice(b)
    return _ON_DEVICE[b.name]


class Tables:
    """the call's six output tables, filled with -1, and a fenced arena (out_size None: measure only)"""

    def __init__(self, n, out_size=None):
        import torch
        i64 = lambda k: torch.full((k,), -1, dtype=torch.int64, device="cuda")
        self.offsets, self.sizes, self.first_block, self.bound = i64(n + 1), i64(n), i64(n + 1), i64(1)
        self.item_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        self.word = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.out_size = out_size
        self.buf = to_dev(sentinel(out_size + 2 * GUARD)) if out_size is not None else None

    def out_ptr(self):
        return self.buf.data_ptr() + GUARD if self.buf is not None else None

    def host(self):
        return dict(offsets=self.offsets.cpu().tolist(), sizes=self.sizes.cpu().tolist(), first_block=self.first_block.cpu().tolist(),
                    bound=int(self.bound.item()), status=self.item_status.cpu().tolist(), word=int(self.word.item()))

    def untouched(self, n):
        return self.host() == dict(offsets=[-1] * (n + 1), sizes=[-1] * n, first_block=[-1] * (n + 1), bound=-1, status=[-1] * n, word=-1)


def tables_call(codec, d, t, ext, cap_blocks, **over):
    """tsqa_compress_batch_packed_tables_async on the current stream -> its return value.  over: arguments replaced."""
    a = dict(ctx=codec.h, data=d.data.data_ptr(), in_size=d.data.numel(), in_offsets=d.in_offsets.data_ptr(), in_sizes=d.in_sizes.data_ptr(),
             n=d.n, cap_blocks=cap_blocks, ext=ext, align=d.b.align, out=t.out_ptr(), out_size=t.out_size or 0, offsets=t.offsets.data_ptr(),
             sizes=t.sizes.data_ptr(), first_block=t.first_block.data_ptr(), bound=t.bound.data_ptr(), item_status=t.item_status.data_ptr(),
             status=t.word.data_ptr())
    a.update(over)
    return codec.L.tsqa_compress_batch_packed_tables_async(a["ctx"], a["data"], a["in_size"], a["in_offsets"], a["in_sizes"], a["n"], a["cap_blocks"],
                                                           a["ext"], a["align"], a["out"], a["out_size"], a["offsets"], a["sizes"], a["first_block"],
                                                           a["bound"], a["item_status"], a["status"], codec._stream())


def image(b, ext, e, out_size):
    """the bytes the fenced buffer must hold"""
    expect = sentinel(out_size + 2 * GUARD)
    for blob, o, w in zip(b.containers(ext), e["offsets"], e["writes"]):
        if w:
            expect[GUARD + o:GUARD + o + w] = np.frombuffer(blob, dtype=np.uint8)[:w]
    return expect


def same_image(host, expect, e, what):
    if np.array_equal(host, expect):
        return
    at = int(np.flatnonzero(host != expect)[0]) - GUARD
    k = max((j for j, o in enumerate(e["offsets"][:-1]) if o <= at), default=-1)
    raise AssertionError(f"{what}: byte {at} of the arena is {int(host[at + GUARD])} for {int(expect[at + GUARD])} "
                         f"(item {k}, which starts at {e['offsets'][k] if k >= 0 else 0} with {e['sizes'][k] if k >= 0 else 0} bytes)")


def check_tables(got, e, what):
    assert got["first_block"] == e["first_block"], f"{what}: d_first_block"
    assert got["bound"] == e["bound"], f"{what}: *d_bound"
    assert got["status"] == e["status"], f"{what}: item statuses {[(k, g, w) for k, (g, w) in enumerate(zip(got['status'], e['status'])) if g != w][:8]} (item, got, owed)"
    assert got["sizes"] == e["sizes"], f"{what}: d_sizes {[(k, g, w) for k, (g, w) in enumerate(zip(got['sizes'], e['sizes'])) if g != w][:8]}"
    assert got["offsets"] == e["offsets"], f"{what}: d_offsets"
    assert got["word"] == max(e["status"]), f"{what}: *d_status"


def run(codec, tsq, b, ext, cap_blocks=None, out_size=None, what=""):
    """one call with this room (default: exactly what the batch needs), checked against the restatement, tsqa_plan_compress_tables,
    tsqa_plan_packed and the oracle -> (Tables, expectation)"""
    import torch
    what = f"{what or b.name} (ext {ext})"
    cap_blocks = b.need_blocks if cap_blocks is None else cap_blocks
    if out_size is None:
        out_size = b.expect(ext, cap_blocks, ROOMY)["offsets"][-1]
    e = b.expect(ext, cap_blocks, out_size)
    d = on_device(b)
    t = Tables(d.n, out_size)
    torch.cuda.synchronize()
    rc = tables_call(codec, d, t, ext, cap_blocks)
    assert rc == 0, codec.last_error()
    torch.cuda.synchronize()
    got = t.host()
    planned = tsq.plan_compress_tables(*b.tables_u64(), b.in_size, b.align, cap_blocks)
    assert planned[0] == e["first_block"] and planned[2] == e["bound"] and planned[3] == e["n_fit"]
    check_tables(got, e, what)
    assert tsq.plan_packed(got["sizes"], b.align) == got["offsets"], f"{what}: d_offsets is not tsqa_plan_packed(d_sizes)"
    same_image(t.buf.cpu().numpy(), image(b, ext, e, out_size), e, what)
    return t, e


# ---- the families ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", tg.EXTS)
@pytest.mark.parametrize("k", range(len(tg.LOOP_COUNTS)))
def test_loop_edges(codec, tsq, k, ext):
    _, e = run(codec, tsq, tg.loop_edges()[k], ext)
    assert e["status"] == [OK] * tg.LOOP_COUNTS[k]


@pytest.mark.parametrize("ext", tg.EXTS)
@pytest.mark.parametrize("k", range(6))
def test_launch_edges(codec, tsq, budget, k, ext):
    b = tg.launch_edges(budget)[k]
    _, e = run(codec, tsq, b, ext)
    assert e["status"] == [OK] * len(b.specs)
    if b.name == "launch_straddle":
        assert [list(r) for r in tg.launches_of(b, budget)[budget - 2:budget + 1]] == [[0], [0, 1], [1]]


@pytest.mark.parametrize("ext", tg.EXTS)
def test_refusals_cost_only_themselves(codec, tsq, budget, ext):
    b = tg.refusals(budget)
    _, e = run(codec, tsq, b, ext)
    assert [s for s in e["status"] if s] == [ERR_ARG] * 5 and e["status"][0] == e["status"][-1] == ERR_ARG
    assert e["status"][budget + 1:budget + 3] == [ERR_ARG] * 2 and e["status"][budget] == OK


@pytest.mark.parametrize("ext", tg.EXTS)
def test_a_run_of_refused_items_longer_than_a_scan_pass(codec, tsq, ext):
    _, e = run(codec, tsq, tg.refused_run(), ext)
    assert e["status"] == [OK] * 3 + [ERR_ARG] * 300 + [OK] * 3


@pytest.mark.parametrize("ext", tg.EXTS)
def test_nothing_but_refused_items(codec, tsq, ext):
    b = tg.all_refused()
    _, e = run(codec, tsq, b, ext, cap_blocks=3, out_size=64)
    assert e["status"] == [ERR_ARG] * 5 and e["offsets"] == [0] * 6 and e["first_block"] == [0] * 6 and e["bound"] == 0


@pytest.mark.parametrize("ext", tg.EXTS)
@pytest.mark.parametrize("k", range(5))
def test_cap_blocks_cuts(codec, tsq, budget, k, ext):
    b, table = tg.cap_cuts(budget)
    what, cap_blocks, n_fit = table[k]
    t, e = run(codec, tsq, b, ext, cap_blocks=cap_blocks, what=what)
    assert e["status"] == [OK if i < n_fit else ERR_OVERFLOW for i in range(len(b.specs))], what
    assert int(t.first_block[-1].item()) == b.need_blocks, "first_block[n_items] is what a retry needs"


@pytest.mark.parametrize("ext", tg.EXTS)
@pytest.mark.parametrize("k", range(6))
def test_arena_cuts(codec, tsq, k, ext):
    b, table = tg.arena_cuts(ext)
    what, out_size = table[k]
    t, e = run(codec, tsq, b, ext, out_size=out_size, what=what)
    full = b.expect(ext, b.need_blocks, ROOMY)
    assert e["sizes"] == full["sizes"] and e["offsets"] == full["offsets"], "sizes and places are complete whatever the room"
    assert e["status"] == [OK if o + z <= out_size else ERR_OVERFLOW for o, z in zip(full["offsets"], full["sizes"])]
    assert (max(e["status"]) == OK) == (what == "used")


@pytest.mark.parametrize("ext", tg.EXTS)
@pytest.mark.parametrize("align", tg.ALIGNS)
def test_aligns(codec, tsq, align, ext):
    b = tg.alignment(align)
    _, e = run(codec, tsq, b, ext)
    assert all(o % align == 0 for o in e["offsets"][:-1]) and e["status"] == [OK] * len(b.specs)


@pytest.mark.parametrize("ext", tg.EXTS)
def test_overlapping_and_identical_input_ranges(codec, tsq, ext):
    t, e = run(codec, tsq, tg.overlaps(), ext)
    assert e["sizes"][2] == e["sizes"][1] and e["status"] == [OK] * 6


@pytest.mark.parametrize("ext", tg.EXTS)
def test_lying_sizes_follow_the_rule_not_a_wrapped_sum(codec, tsq, ext):
    b = tg.lying()
    _, e = run(codec, tsq, b, ext)
    assert [st for s, st in zip(b.specs, e["status"]) if isinstance(s, tg.Lie)] == [ERR_ARG] * 5
    assert [st for s, st in zip(b.specs, e["status"]) if not isinstance(s, tg.Lie)] == [OK] * 4 and e["first_block"][-1] == 4


# ---- measure only ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["refusals", "cuts", "loop_edges_513", "lying"])
def test_measure_only_then_a_retry_with_the_reported_room(codec, tsq, budget, name):
    import torch
    b = {x.name: x for x in tg.every_batch(budget)}[name]
    d = on_device(b)
    before = d.data.clone()
    for cap_blocks in (0, 1000):                              # (a cap_blocks that nobody looks at changes nothing)
        t = Tables(d.n)
        codec.profile(True)
        codec.profile_read()
        torch.cuda.synchronize()
        assert tables_call(codec, d, t, 1, cap_blocks) == 0, codec.last_error()
        torch.cuda.synchronize()
        launches = codec.profile_read()[1]
        codec.profile(False)
        e = b.expect(1, 0, 0, measuring=True)
        check_tables(t.host(), e, f"{name}: measuring")
        assert launches == 0, "measuring launched an encoder"
        assert set(e["status"]) <= {ERR_ARG, ERR_OVERFLOW} and not any(e["sizes"]) and not any(e["offsets"])
    assert torch.equal(before, d.data)
    need_blocks, bound = int(t.first_block[-1].item()), int(t.bound.item())
    assert need_blocks == b.need_blocks
    _, e = run(codec, tsq, b, 1, cap_blocks=need_blocks, out_size=bound, what=f"{name}: the retry")
    assert [st for st, nb in zip(e["status"], b.blocks) if nb] == [OK] * sum(1 for nb in b.blocks if nb)


# ---- equality with the host form ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [0, 6, 7])
def test_equal_to_the_host_form(tsq, budget, variant):
    import torch
    b = tg.launch_edges(budget)[4]                            # the straddling batch: two launches, an item across them
    d = on_device(b)
    fresh = tsq.DeviceCodec(0)
    try:
        fresh.set_variant(variant, 0)
        for ext in tg.EXTS:
            t, e = run(fresh, tsq, b, ext)
            used = e["offsets"][-1]
            u = Tables(d.n, used)
            quads = [(a, z, 0, 0) for a, z in zip(b.in_offsets, b.in_sizes)]
            torch.cuda.synchronize()
            rc = fresh.L.tsqa_compress_batch_packed_async(fresh.h, d.data.data_ptr(), d.data.numel(), _batch_array(quads), d.n, ext, b.align,
                                                          u.out_ptr(), used, u.offsets.data_ptr(), u.sizes.data_ptr(), u.word.data_ptr(),
                                                          fresh._stream())
            assert rc == 0, fresh.last_error()
            torch.cuda.synchronize()
            assert torch.equal(u.buf, t.buf) and torch.equal(u.offsets, t.offsets) and torch.equal(u.sizes, t.sizes)
            assert int(u.word.item()) == int(t.word.item()) == OK
    finally:
        fresh.close()


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 5])
def test_other_encoder_variants_are_refused(tsq, variant):
    import torch
    b = tg.overlaps()
    d = on_device(b)
    fresh = tsq.DeviceCodec(0)
    try:
        fresh.set_variant(variant, 0)
        for out_size in (4096, None):                         # (compressing and measuring)
            t = Tables(d.n, out_size)
            torch.cuda.synchronize()
            assert tables_call(fresh, d, t, 1, b.need_blocks) == ERR_ARG
            torch.cuda.synchronize()
            assert t.untouched(d.n)
    finally:
        fresh.close()


# ---- argument errors ------------------------------------------------------------------------------------------------------------------

def test_refused_arguments_write_nothing(codec):
    import torch
    b = tg.overlaps()
    d = on_device(b)
    out_size = 1 << 16
    t = Tables(d.n, out_size)
    torch.cuda.synchronize()
    call = lambda **over: tables_call(codec, d, t, 1, over.pop("cap_blocks", b.need_blocks), **over)
    for name in ("data", "in_offsets", "in_sizes", "offsets", "sizes", "first_block", "item_status", "status"):
        assert call(**{name: None}) == ERR_ARG, name
        assert "null pointer" in codec.last_error()
    assert call(ctx=None) == ERR_ARG
    assert call(n=0) == ERR_ARG
    for align in (0, 3, 24, 8192):
        assert call(align=align) == ERR_ARG, align
    assert call(in_size=(1 << 48) + 1) == ERR_ARG
    assert call(out_size=15) == ERR_ARG                       # an arena that holds no header
    assert call(cap_blocks=0) == ERR_ARG                      # an arena and no blocks
    assert call(out=None) == ERR_ARG                          # measuring takes out_size 0
    torch.cuda.synchronize()
    assert np.array_equal(t.buf.cpu().numpy(), sentinel(out_size + 2 * GUARD))
    assert t.untouched(d.n)
    assert call(bound=None) == 0                              # (the bound word alone may be left out)
    torch.cuda.synchronize()
    assert int(t.bound.item()) == -1 and int(t.word.item()) == OK


# ---- chains on one stream, nothing waited for until the end ---------------------------------------------------------------------------

def _sources(n_items, seed, big_at=None):
    """text items of 1 B to 4 KiB, one of 4 MiB + 1 B at big_at -> (bytes, lengths)"""
    from turbosqueeze_amd import synth
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(1, 4097, n_items)]
    if big_at is not None:
        lens[big_at] = tg.BLOCK + 1
    return synth.text(sum(lens), seed=seed), lens


def test_chain_from_a_device_cumsum_to_the_dense_decompress(tsq):
    """(a) lengths -> torch.cumsum on the device -> the new call -> tsqa_decompress_batch_packed_dense_async -> the items' bytes"""
    import torch
    side = torch.cuda.Stream()
    fresh = tsq.DeviceCodec(0)
    src, lens = _sources(70, 81, big_at=33)
    n, blocks = len(lens), sum(-(-ln // tg.BLOCK) for ln in lens)
    out_offsets = tsq.plan_dense(lens, [-(-ln // tg.BLOCK) for ln in lens], 16)[0]
    try:
        with torch.cuda.stream(side):
            d_src, d_lens = to_dev(src), to_dev(lens, np.int64)
            d_at = torch.cumsum(d_lens, 0) - d_lens
            arena = torch.empty(sum(tsq.batch_bound(ln) + 15 for ln in lens), dtype=torch.uint8, device="cuda")
            t = Tables(n, arena.numel())
            rc = fresh.L.tsqa_compress_batch_packed_tables_async(fresh.h, d_src.data_ptr(), d_src.numel(), d_at.data_ptr(), d_lens.data_ptr(), n,
                                                                 blocks, 1, 16, arena.data_ptr(), arena.numel(), t.offsets.data_ptr(),
                                                                 t.sizes.data_ptr(), t.first_block.data_ptr(), t.bound.data_ptr(),
                                                                 t.item_status.data_ptr(), t.word.data_ptr(), fresh._stream())
            assert rc == 0, fresh.last_error()
            u = Tables(n, out_offsets[-1])
            rc = fresh.L.tsqa_decompress_batch_packed_dense_async(fresh.h, arena.data_ptr(), arena.numel(), t.offsets.data_ptr(), t.sizes.data_ptr(),
                                                                  n, 16, blocks, u.out_ptr(), out_offsets[-1], u.offsets.data_ptr(),
                                                                  u.sizes.data_ptr(), u.first_block.data_ptr(), u.item_status.data_ptr(),
                                                                  u.word.data_ptr(), fresh._stream())
            assert rc == 0, fresh.last_error()
        side.synchronize()
        assert t.item_status.cpu().tolist() == [OK] * n and int(t.word.item()) == OK and int(t.bound.item()) <= arena.numel()
        assert u.item_status.cpu().tolist() == [OK] * n and u.sizes.cpu().tolist() == lens and u.offsets.cpu().tolist() == out_offsets
        expect, at = sentinel(out_offsets[-1] + 2 * GUARD), 0
        for ln, o in zip(lens, out_offsets):
            expect[GUARD + o:GUARD + o + ln] = src[at:at + ln]
            at += ln
        assert np.array_equal(u.buf.cpu().numpy(), expect)
    finally:
        fresh.close()


def test_chain_transcode_behind_the_dense_decompress(tsq):
    """(b) the dense decompress of an ext 0 arena hands its d_out_offsets / d_out_sizes straight to the new call with ext 1; one
    container of the source is damaged, so its out_sizes word of 0 becomes that item's TSQA_ERR_ARG and every other item is exact"""
    import torch
    side = torch.cuda.Stream()
    fresh = tsq.DeviceCodec(0)
    src, lens = _sources(40, 82)
    n, bad = len(lens), 11
    ats = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
    items = [src[a:a + ln].tobytes() for a, ln in zip(ats, lens)]
    blobs0 = [tg.container(x, 0) for x in items]
    src_offsets = tg.packed([len(x) for x in blobs0], 16)
    arena0 = np.full(src_offsets[-1], 0xEE, dtype=np.uint8)
    for o, blob in zip(src_offsets, blobs0):
        arena0[o:o + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
    arena0[src_offsets[bad]] ^= 0xFF                          # the magic: refused at its header, no room in the dense output
    mid_offsets = tsq.plan_dense([0 if k == bad else ln for k, ln in enumerate(lens)], [0 if k == bad else 1 for k in range(n)], 16)[0]
    want = [None if k == bad else tg.container(x, 1) for k, x in enumerate(items)]
    sizes = [0 if blob is None else len(blob) for blob in want]
    offsets = tg.packed(sizes, 16)
    try:
        with torch.cuda.stream(side):
            d_arena0, d_off0, d_sz0 = to_dev(arena0), to_dev(src_offsets[:-1], np.int64), to_dev([len(x) for x in blobs0], np.int64)
            u = Tables(n, mid_offsets[-1])
            rc = fresh.L.tsqa_decompress_batch_packed_dense_async(fresh.h, d_arena0.data_ptr(), d_arena0.numel(), d_off0.data_ptr(), d_sz0.data_ptr(),
                                                                  n, 16, n, u.out_ptr(), mid_offsets[-1], u.offsets.data_ptr(), u.sizes.data_ptr(),
                                                                  u.first_block.data_ptr(), u.item_status.data_ptr(), u.word.data_ptr(),
                                                                  fresh._stream())
            assert rc == 0, fresh.last_error()
            t = Tables(n, offsets[-1])
            rc = fresh.L.tsqa_compress_batch_packed_tables_async(fresh.h, u.out_ptr(), mid_offsets[-1], u.offsets.data_ptr(), u.sizes.data_ptr(), n,
                                                                 n, 1, 16, t.out_ptr(), offsets[-1], t.offsets.data_ptr(), t.sizes.data_ptr(),
                                                                 t.first_block.data_ptr(), t.bound.data_ptr(), t.item_status.data_ptr(),
                                                                 t.word.data_ptr(), fresh._stream())
            assert rc == 0, fresh.last_error()
        side.synchronize()
        assert u.sizes.cpu().tolist() == [0 if k == bad else ln for k, ln in enumerate(lens)]
        got = t.host()
        assert got["status"] == [ERR_ARG if k == bad else OK for k in range(n)] and got["word"] == ERR_ARG
        assert got["sizes"] == sizes and got["offsets"] == offsets and got["first_block"] == [k - (k > bad) for k in range(n + 1)]
        expect = sentinel(offsets[-1] + 2 * GUARD)
        for o, blob in zip(offsets, want):
            if blob is not None:
                expect[GUARD + o:GUARD + o + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
        assert np.array_equal(t.buf.cpu().numpy(), expect)
    finally:
        fresh.close()


def test_chain_twice_back_to_back_the_second_grows_the_scratch(tsq):
    """(c) two calls on one stream of a fresh context, the second with more items than reserve_batch's first size and more blocks"""
    import torch
    side = torch.cuda.Stream()
    fresh = tsq.DeviceCodec(0)
    shapes = [_sources(40, 83, big_at=17), _sources(cg.FIRST_BATCH_ITEMS + 44, 84)]
    assert len(shapes[0][1]) < cg.FIRST_BATCH_ITEMS < len(shapes[1][1])
    runs = []
    try:
        with torch.cuda.stream(side):
            for src, lens in shapes:
                n, blocks = len(lens), sum(-(-ln // tg.BLOCK) for ln in lens)
                ats = np.concatenate([[0], np.cumsum(lens)[:-1]]).tolist()
                d_src, d_at, d_lens = to_dev(src), to_dev(ats, np.int64), to_dev(lens, np.int64)
                room = sum(tsq.batch_bound(ln) + 15 for ln in lens)
                t = Tables(n, room)
                rc = fresh.L.tsqa_compress_batch_packed_tables_async(fresh.h, d_src.data_ptr(), d_src.numel(), d_at.data_ptr(), d_lens.data_ptr(),
                                                                     n, blocks, 1, 16, t.out_ptr(), room, t.offsets.data_ptr(), t.sizes.data_ptr(),
                                                                     t.first_block.data_ptr(), t.bound.data_ptr(), t.item_status.data_ptr(),
                                                                     t.word.data_ptr(), fresh._stream())
                assert rc == 0, fresh.last_error()
                runs.append((src, ats, lens, room, t, (d_src, d_at, d_lens)))
        side.synchronize()
        for src, ats, lens, room, t, _ in runs:
            blobs = [tg.container(src[a:a + ln].tobytes(), 1) for a, ln in zip(ats, lens)]
            got = t.host()
            assert got["status"] == [OK] * len(lens) and got["word"] == OK and got["sizes"] == [len(x) for x in blobs]
            assert got["offsets"] == tg.packed(got["sizes"], 16) and got["bound"] == sum(tg.round_up(tsq.batch_bound(ln), 16) for ln in lens) <= room
            expect = sentinel(room + 2 * GUARD)
            for o, blob in zip(got["offsets"], blobs):
                expect[GUARD + o:GUARD + o + len(blob)] = np.frombuffer(blob, dtype=np.uint8)
            assert np.array_equal(t.buf.cpu().numpy(), expect)
    finally:
        fresh.close()


# ---- the Python face ------------------------------------------------------------------------------------------------------------------

def test_python_compress_packed_tables_round_trip(codec, tsq):
    import torch
    b = tg.cuts_batch()
    d = on_device(b)
    for ext in tg.EXTS:
        e = b.expect(ext, b.need_blocks, ROOMY)
        for kw in (dict(), dict(cap_blocks=b.need_blocks), dict(cap_blocks=b.need_blocks, out=torch.empty(e["offsets"][-1], dtype=torch.uint8, device="cuda"))):
            pb = codec.compress_packed_tables(d.data, d.in_offsets, d.in_sizes, ext, **kw)
            assert pb.offsets == e["offsets"] and pb.sizes == e["sizes"] and pb.lengths == b.in_sizes
            for v, blob in zip(pb.views, b.containers(ext)):
                assert v.cpu().numpy().tobytes() == blob
            for i, v in enumerate(pb.decompress()):
                assert v.cpu().numpy().tobytes() == b.item_bytes(i)


def test_python_compress_packed_tables_reports_item_statuses(codec, tsq):
    b = tg.refused_run()
    d = on_device(b)
    with pytest.raises(tsq.TsqError) as err:
        codec.compress_packed_tables(d.data, d.in_offsets, d.in_sizes, 1)
    e = b.expect(1, b.need_blocks, ROOMY)
    assert err.value.code == ERR_ARG and err.value.item_status == e["status"]
    pb, status = codec.compress_packed_tables(d.data, d.in_offsets, d.in_sizes, 1, item_status=True)
    assert status == e["status"] and pb.sizes == e["sizes"] and pb.offsets[:-1] == e["offsets"][:-1]
    small = tg.cuts_batch()
    ds = on_device(small)
    with pytest.raises(tsq.TsqError) as err:
        codec.compress_packed_tables(ds.data, ds.in_offsets, ds.in_sizes, 1, cap_blocks=3)
    assert err.value.code == ERR_OVERFLOW and err.value.item_status == [OK] * 3 + [ERR_OVERFLOW] * 7
    assert tsq.plan_compress_tables(small.in_offsets, small.in_sizes, small.in_size, 16, 3)[3] == 3
