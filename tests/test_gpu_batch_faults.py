"""GPU tests of the batch decompress with a verdict per item (tsqa_decompress_batch_items_async, its packed twin, and the
synchronous tsqa_decompress_batch that now uses it on its error path), on the seeded batch of tests/faultgen.py: 301 containers,
110 of them refused, every refused one between two that must be delivered.  Every verdict and every expected byte is the oracle's.
Outputs are sentinel-filled with gaps of 1..47 guard bytes between the items' ranges; the whole output is compared with one image:
the sentinel, overlaid with the data of the accepted items.  Only the ranges of items that a block decoder refuses are left out
of the comparison (their contents are undefined); the ranges of items that the frame walk refuses must still hold the sentinel.

The verdicts are those of mtgen.expected_of_the_scheduler: the oracle's, and a refusal where the oracle decodes to another length
than the header states (the library's own integrity rule; two of the 131 damaged containers, test_batch_faults_cpu.py names them)."""
import ctypes as C

import numpy as np
import pytest

import faultgen as fg
from turbosqueeze_amd.api import PackedBatch, _batch_array

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_STALL = fg.OK, fg.ERR_ARG, fg.ERR_FORMAT, fg.ERR_STREAM, fg.ERR_STALL


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


@pytest.fixture(autouse=True)
def default_variants(codec):
    codec.set_variant(0, 0)
    yield
    codec.set_variant(0, 0)
    codec.set_decode_wait_limit(1 << 24)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (the pattern repeats every 251 bytes)"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


class Sub:
    """some items of the batch with fenced output ranges of their own: the image the output must equal, and the bytes that count"""

    def __init__(self, items, in_ats, seed, refused_too=()):
        rng = np.random.default_rng(seed)
        self.items, self.in_ats = items, in_ats
        at, self.outs = 0, []
        for it in items:
            at += int(rng.integers(1, 48))
            self.outs.append(at)
            at += it.cap
        self.out_size = at + 64
        self.guard = sentinel(self.out_size)
        self.expect = self.guard.copy()
        self.defined = np.ones(self.out_size, dtype=bool)
        self.refused = [it.refused or k in refused_too for k, it in enumerate(items)]
        for k, (it, o) in enumerate(zip(items, self.outs)):
            if not self.refused[k]:
                assert len(it.want) == it.cap
                self.expect[o:o + it.cap] = np.frombuffer(it.want, dtype=np.uint8)
            elif not (it.by_walk or k in refused_too):
                self.defined[o:o + it.cap] = False              # refused by a block decoder: undefined contents in its own range
        self.quads = [(a, len(it.blob), o, it.cap) for it, a, o in zip(items, in_ats, self.outs)]
        self.blocks = [it.n_blocks for it in items]
        self.sizes = [0 if r else len(it.want) for it, r in zip(items, self.refused)]

    def fresh(self, wait=True):
        """-> (sentinel-filled output, d_sizes, d_item_status) on the device, the tables filled with -1.  wait: the fills are
        finished on return (the library's own stream does not wait for torch's default stream); False on a stream that the call
        itself is enqueued on."""
        import torch
        n = len(self.items)
        made = (to_dev(self.guard), torch.full((n,), -1, dtype=torch.int64, device="cuda"),
                torch.full((n,), -1, dtype=torch.int32, device="cuda"))
        if wait:
            torch.cuda.synchronize()
        return made

    def check(self, out, d_sizes, d_item_status, what=""):
        """the verdicts, the sizes and the whole output image -> the item statuses"""
        status = d_item_status.cpu().tolist()
        for k, it in enumerate(self.items):
            assert (status[k] != 0) == self.refused[k], (f"{what}item {k} ({it.name}): status {status[k]}, the oracle "
                                                        f"{'refuses' if self.refused[k] else 'accepts'} it")
        assert d_sizes.cpu().tolist() == self.sizes, f"{what}d_sizes"
        host = out.cpu().numpy()
        same = (host == self.expect) | ~self.defined
        if not same.all():
            at = int(np.flatnonzero(~same)[0])
            k = max(j for j, o in enumerate(self.outs) if o <= at) if at >= self.outs[0] else -1
            inside = k >= 0 and at < self.outs[k] + self.items[k].cap
            raise AssertionError(f"{what}byte {at} is {int(host[at])} for {int(self.expect[at])}: " +
                                 (f"item {k} ({self.items[k].name}, {'refused' if self.refused[k] else 'accepted'}) at its byte {at - self.outs[k]}"
                                  if inside else f"a guard byte behind item {k}"))
        return status


class Faults:
    """the whole batch on the device: the containers in one arena behind non-zero filler gaps of 0..47 bytes"""

    def __init__(self, items):
        rng = np.random.default_rng(fg.SEED + 1)
        at, self.in_ats = 0, []
        for it in items:
            at += int(rng.integers(0, 48))
            self.in_ats.append(at)
            at += len(it.blob)
        arena = rng.integers(1, 256, at + 64, dtype=np.uint8)
        for it, a in zip(items, self.in_ats):
            arena[a:a + len(it.blob)] = np.frombuffer(it.blob, dtype=np.uint8)
        self.items, self.d_in = items, to_dev(arena)
        self.all = Sub(items, self.in_ats, fg.SEED + 2)

    def sub(self, lo, hi, seed):
        return Sub(self.items[lo:hi], self.in_ats[lo:hi], seed)


@pytest.fixture(scope="module")
def faults(tsq, oracle):
    return Faults(fg.batch(oracle))


def run_items(codec, faults, sub, what=""):
    import torch
    out, d_sizes, d_item_status = sub.fresh()
    codec.decompress_batch_items_async(faults.d_in, sub.quads, sub.blocks, out, d_sizes, d_item_status)
    torch.cuda.synchronize()
    status = sub.check(out, d_sizes, d_item_status, what)
    assert codec.status() == max(status), f"{what}*d_status is {codec.status()}, the largest item status {max(status)}"
    return status


def test_whole_batch_one_verdict_per_item(codec, faults):
    sub = faults.all
    status = run_items(codec, faults, sub)
    walked = [k for k, it in enumerate(sub.items) if it.by_walk]
    assert {sub.items[k].klass for k in walked} == {"twin_walk", "tight", "damaged_refused"} and len(walked) == 13
    assert all(status[k] == ERR_FORMAT for k in walked)             # (their ranges held the sentinel: Sub.check compares them)
    assert sum(s != 0 for s in status) == 110 and sum(it.klass == "damaged_valid" for it in sub.items) == 63


def test_status_codes_equal_the_single_call(codec, faults):
    """every refused item alone through tsqa_decompress_device_async on one workgroup per block (decode variant 4), with the same
    block count and capacity: the word it leaves is the item's"""
    import torch
    sub = faults.all
    status = run_items(codec, faults, sub)
    codec.set_variant(0, 4)
    room = torch.empty(max(it.cap for it in sub.items if it.refused), dtype=torch.uint8, device="cuda")
    for k, it in enumerate(sub.items):
        if not it.refused:
            continue
        a = faults.in_ats[k]
        codec.decompress_async(faults.d_in[a:a + len(it.blob)], it.n_blocks, room[:it.cap])
        torch.cuda.synchronize()                          # (the call ran on the library's own stream, which torch's does not wait for)
        size, single = codec.last_size_status()
        assert single == status[k] == it.status, f"item {k} ({it.name}): alone {single}, in the batch {status[k]}, owed {it.status}"


def test_packed_form_and_bad_places(codec, faults):
    import torch
    items = faults.items
    arena, offsets, sizes = fg.packed_layout(items)
    d_arena = to_dev(arena)                              # exactly the bytes used: the last container ends the allocation's payload
    offsets, sizes, bad = fg.bad_places(items, offsets, sizes, arena.size)
    past = next(i for i, what in bad.items() if what == "an offset past the arena")
    assert offsets[past] < d_arena.numel() < offsets[past] + sizes[past], "the place ends behind the allocation by the table's value only"
    sub = Sub(items, [0] * len(items), fg.SEED + 3, refused_too=set(bad))
    out, d_out_sizes, d_item_status = sub.fresh()
    d_offsets = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    d_sizes = torch.tensor(sizes, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    codec.decompress_batch_packed_items_async(d_arena, d_offsets, d_sizes, [(o, it.cap) for o, it in zip(sub.outs, items)], sub.blocks,
                                              out, d_out_sizes, d_item_status)
    torch.cuda.synchronize()
    status = sub.check(out, d_out_sizes, d_item_status)
    assert codec.status() == max(status)
    for i, what in bad.items():
        assert status[i] == ERR_FORMAT, f"{what}: status {status[i]}"
    assert [s for k, s in enumerate(status) if k not in bad] == [it.status for k, it in enumerate(items) if k not in bad]


def test_synchronous_call_finds_the_faults_in_a_constant_number_of_launches(codec, faults):
    """the first attempt (the fast decoders, all or nothing), then ONE pass with a verdict per item: at most three timed decode
    launches where the one-by-one search took one per item"""
    sub = faults.all
    out = to_dev(sub.guard)
    n = len(sub.items)
    sizes, status = (C.c_uint64 * n)(), (C.c_int32 * n)()
    codec.profile(True)
    try:
        codec.profile_read()
        rc = codec.L.tsqa_decompress_batch(codec.h, faults.d_in.data_ptr(), faults.d_in.numel(), _batch_array(sub.quads), n, out.data_ptr(),
                                           sub.out_size, sizes, status, codec._stream())
        launches = codec.profile_read()[3]
    finally:
        codec.profile(False)
    print(f"decode launches of the synchronous call: {launches}")
    assert launches <= 3, f"{launches} decode launches for {n} items"
    import torch
    d_sizes = torch.tensor([int(s) for s in sizes], dtype=torch.int64)
    d_status = torch.tensor([int(s) for s in status], dtype=torch.int32)
    got = sub.check(out, d_sizes, d_status)
    assert rc == max(got) and "110 of 301 items refused" in codec.last_error()
    # (the synchronous form refuses a total above out_cap on the host, as tsqa_decompress_device does: TSQA_ERR_ARG)
    assert [s for s, it in zip(got, sub.items) if it.klass != "tight"] == [it.status for it in sub.items if it.klass != "tight"]
    assert [s for s, it in zip(got, sub.items) if it.klass == "tight"] == [ERR_ARG, ERR_ARG]


def test_calls_in_stream_order(codec, faults):
    """two calls with different faults and a third that waits for an upload slot, each with its own tables, nothing waited for
    between them; then the all-or-nothing form with healthy items on the same stream"""
    import torch
    side = torch.cuda.Stream()
    subs = [faults.sub(0, 70, 11), faults.sub(70, 150, 12), faults.sub(150, 200, 13)]
    assert all(any(s.refused) for s in subs) and [it.name for it in subs[0].items] != [it.name for it in subs[1].items]
    healthy = [k for k, it in enumerate(faults.items) if not it.refused][:90]
    plain = Sub([faults.items[k] for k in healthy], [faults.in_ats[k] for k in healthy], 14)
    runs = []
    with torch.cuda.stream(side):
        for s in subs:
            out, d_sizes, d_item_status = s.fresh(wait=False)
            own = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            nb = np.ascontiguousarray(s.blocks, dtype=np.uint32)
            rc = codec.L.tsqa_decompress_batch_items_async(codec.h, faults.d_in.data_ptr(), faults.d_in.numel(), _batch_array(s.quads),
                                                           nb.ctypes.data, len(s.items), out.data_ptr(), s.out_size, d_sizes.data_ptr(),
                                                           d_item_status.data_ptr(), own.data_ptr(), codec._stream())
            assert rc == 0, codec.last_error()
            runs.append((s, out, d_sizes, d_item_status, own))
        p_out, p_sizes, _ = plain.fresh(wait=False)
        codec.decompress_batch_async(faults.d_in, plain.quads, plain.blocks, p_out, p_sizes)
    side.synchronize()
    for k, (s, out, d_sizes, d_item_status, own) in enumerate(runs):
        status = s.check(out, d_sizes, d_item_status, f"call {k}: ")
        assert int(own.item()) == max(status) != 0
    assert codec.status() == 0
    plain.check(p_out, p_sizes, torch.zeros(len(plain.items), dtype=torch.int32))


@pytest.mark.parametrize("variant", [0, 3, 5, 6])
def test_the_decode_variant_changes_nothing(codec, faults, variant):
    codec.set_variant(0, variant)
    codec.set_decode_wait_limit(1)                       # (one poll: every several-workgroups decode would stall)
    status = run_items(codec, faults, faults.all, f"variant {variant}: ")
    assert ERR_STALL not in status and status == [it.status for it in faults.items]


def test_refused_arguments_write_nothing(codec, faults):
    import torch
    sub = faults.sub(0, 6, 15)
    n = len(sub.items)
    out, d_sizes, d_item_status = sub.fresh()
    word = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nb = np.ascontiguousarray(sub.blocks, dtype=np.uint32)
    size = faults.d_in.numel()

    def call(quads=sub.quads, blocks=nb, n_items=n, in_size=size, out_size=sub.out_size, item_status=d_item_status.data_ptr(),
             status=word.data_ptr(), sizes=d_sizes.data_ptr()):
        return codec.L.tsqa_decompress_batch_items_async(codec.h, faults.d_in.data_ptr(), in_size, _batch_array(quads), blocks.ctypes.data,
                                                         n_items, out.data_ptr(), out_size, sizes, item_status, status, codec._stream())

    assert call(item_status=None) == ERR_ARG and "null pointer" in codec.last_error()
    assert call(status=None) == ERR_ARG and call(sizes=None) == ERR_ARG
    assert call(n_items=0) == ERR_ARG
    q = sub.quads
    assert call(quads=[q[0], (q[1][0], q[1][1], q[0][2], q[1][3])] + q[2:]) == ERR_ARG            # two output ranges overlap
    assert call(in_size=q[-1][0] + q[-1][1] - 1) == ERR_ARG                                        # an input range past in_size
    assert call(out_size=q[-1][2] + q[-1][3] - 1) == ERR_ARG                                       # an output range past out_size
    assert call(blocks=np.array([0] + sub.blocks[1:], dtype=np.uint32)) == ERR_ARG                 # a block count of 0
    too_many = (len(sub.items[0].blob) - 16) // 6 + 1
    assert call(blocks=np.array([too_many] + sub.blocks[1:], dtype=np.uint32)) == ERR_ARG          # more blocks than the item can hold
    tables = torch.zeros(n, dtype=torch.int64, device="cuda")
    packed = lambda offs, szs, item_status: codec.L.tsqa_decompress_batch_packed_items_async(
        codec.h, faults.d_in.data_ptr(), size, offs, szs, _batch_array(sub.quads), nb.ctypes.data, n, out.data_ptr(), sub.out_size,
        d_sizes.data_ptr(), item_status, word.data_ptr(), codec._stream())
    assert packed(None, tables.data_ptr(), d_item_status.data_ptr()) == ERR_ARG
    assert packed(tables.data_ptr(), None, d_item_status.data_ptr()) == ERR_ARG
    assert packed(tables.data_ptr(), tables.data_ptr(), None) == ERR_ARG
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), sub.guard)
    assert (d_sizes == -1).all() and (d_item_status == -1).all() and int(word.item()) == -1


def test_python_packed_batch_gives_item_statuses(codec, tsq, faults):
    """PackedBatch.decompress(item_status=True): the refused items are reported, the others delivered; without it the call raises"""
    import torch
    items = faults.items[:9]
    arena, offsets, sizes = fg.packed_layout(items)
    pb = PackedBatch(codec, to_dev(arena), offsets + [arena.size], sizes, [it.cap for it in items])
    views, status = pb.decompress(item_status=True)
    assert [s != 0 for s in status] == [it.refused for it in items] and any(status)
    for it, v in zip(items, views):
        assert (v is None) == it.refused
        if v is not None:
            assert v.cpu().numpy().tobytes() == it.want, it.name
    with pytest.raises(tsq.TsqError):
        pb.decompress()


def test_batch_index_walks_every_item_without_a_capacity(codec, faults):
    """tsqa_index_create_batch over the arena: the frame walk with the count each header states and no capacity refuses what
    faultgen.walk_refuses refuses with those arguments, item for item, and indexes every other item"""
    items, n = faults.items, len(faults.items)
    heads = [fg.header_of(it.blob) for it in items]
    refused = [fg.walk_refuses(it.blob, nb, total) for it, (_, nb, total) in zip(items, heads)]
    assert sum(refused) == 11
    h = C.c_void_p()
    verdicts = (C.c_int32 * n)(*([-1] * n))
    rc = codec.L.tsqa_index_create_batch(codec.h, faults.d_in.data_ptr(), faults.d_in.numel(),
                                         _batch_array([(a, len(it.blob), 0, 0) for a, it in zip(faults.in_ats, items)]), n, C.byref(h), verdicts)
    try:
        assert rc == ERR_FORMAT and h, codec.last_error()
        assert list(verdicts) == [ERR_FORMAT if r else OK for r in refused]
        assert [int(codec.L.tsqa_index_item_total(h, i)) for i in range(n)] == [0 if r else total for r, (_, _, total) in zip(refused, heads)]
        assert int(codec.L.tsqa_index_blocks(h)) == sum(nb for r, (_, nb, _) in zip(refused, heads) if not r)
    finally:
        codec.L.tsqa_index_destroy(h)


def test_one_word_form_refuses_what_the_walk_refuses(codec, faults):
    """every item that the frame walk refuses, the two that only their capacity refuses among them, between its two healthy
    neighbours through tsqa_decompress_batch_async: the batch's word, no size, and nothing written to its range.  (Nothing is
    asserted about the neighbours' bytes: the one-word form promises none after a refusal.)"""
    import torch
    walked = [k for k, it in enumerate(faults.items) if it.by_walk]
    assert len(walked) == 13 and sum(faults.items[k].klass == "tight" for k in walked) == 2
    for k in walked:
        sub = faults.sub(k - 1, k + 2, 100 + k)
        before, it, after = sub.items
        out, d_sizes, _ = sub.fresh()
        codec.decompress_batch_async(faults.d_in, sub.quads, sub.blocks, out, d_sizes)
        torch.cuda.synchronize()
        assert codec.status() == ERR_FORMAT, it.name
        assert d_sizes.cpu().tolist() == [len(before.want), 0, len(after.want)], it.name
        o = sub.outs[1]
        assert np.array_equal(out[o:o + it.cap].cpu().numpy(), sub.guard[o:o + it.cap]), it.name
