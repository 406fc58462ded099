"""GPU tests of mixed stream-ordered calls on ONE context (tests/chaingen.py): different entry points enqueued behind one another
on one stream of the test's own with no synchronise between them, each with its OWN destination, status word and size words or
tables.  After one synchronise every destination holds the oracle's bytes, every byte outside a destination still holds the
sentinel, every status word holds what its own call must leave and every size word or table the oracle's values.

Making "in flight" real: every chain starts behind a gate on the same stream (repeated torch.sort of a large tensor, a few tens of
milliseconds, timed once), and an event recorded behind the last link is queried straight after the last enqueue: "not ready"
means the whole chain was queued before it could finish.  A link that grows the context's scratch waits for the device by design
and so ends the gate early; the link behind it is then the one enqueued behind running work.  The share of chains whose gate held
is printed per test; correctness is asserted regardless.

What these tests cannot prove: that a wait inside the library is the one that protects a buffer.  hipFree itself waits for the
device, so a missing stream wait in front of it would very likely pass here too; the chains prove that descriptors, upload slots,
frame tables and status words of neighbouring calls do not leak into one another, not that every free is fenced."""
import ctypes as C
import time

import numpy as np
import pytest

import chaingen as cg
from chaingen import ERR_ARG, ERR_STALL, KINDS, SLOT
from test_gpu_range import fenced, sentinel, to_dev, tsq  # noqa: F401 (tsq: fixture)
from turbosqueeze_amd.api import _batch_array, _item_range_array, _range_array

pytestmark = pytest.mark.gpu

FRAME = np.dtype([("stream_at", "<u8"), ("out_at", "<u8"), ("stream_len", "<u4"), ("ext", "<u4"), ("out_len", "<u4"), ("pad", "<u4")])
SLOTS_FRONT = 256                    # guard bytes in front of a caller's slots (the slots themselves stay aligned)
STATS: dict = {}                     # test -> [chains whose gate held, chains]
PAIRS_DONE: dict = {}                # (first kind, second kind, first shape, second shape) -> 1
STALLS = [0]


class Env:
    """what the chains of this module share: the generator, device copies of the read-only inputs, the indexes of the reads
    (made once, on a context of their own: an index belongs to the device, not to a context) and a long sentinel"""

    def __init__(self, tsq, oracle):
        import torch
        self.torch, self.tsq, self.L = torch, tsq, tsq.lib()
        self.gen = cg.Gen(oracle, tsq.synth)
        self.indexer = tsq.DeviceCodec(0)
        self._dev, self._idx, self._pinned = {}, {}, {}
        self.guard = sentinel(3 * SLOT + 4096)
        self.guard_dev = to_dev(self.guard)

    def dev(self, a):
        if id(a) not in self._dev:
            self._dev[id(a)] = (a, to_dev(a))
        return self._dev[id(a)][1]

    def pinned(self, a):
        if id(a) not in self._pinned:
            self._pinned[id(a)] = (a, self.torch.from_numpy(a.copy()).pin_memory())
        return self._pinned[id(a)][1]

    def fresh(self, n):
        """a sentinel-filled device buffer of n bytes and its host image"""
        return self.guard_dev[:n].clone(), self.guard[:n]

    def index(self, link):
        if id(link) not in self._idx:
            h = C.c_void_p()
            if link.kind == "R":
                blob = self.dev(link.blob)
                rc = self.L.tsqa_index_create(self.indexer.h, blob.data_ptr(), blob.numel(), C.byref(h))
            else:
                arena = self.dev(link.arena)
                rc = self.L.tsqa_index_create_batch(self.indexer.h, arena.data_ptr(), arena.numel(), _batch_array([(a, n, 0, 0) for a, n in link.spans]),
                                                    len(link.spans), C.byref(h), None)
            assert rc == 0 and h, (link, rc, self.indexer.last_error())
            self._idx[id(link)] = (link, h)
        return self._idx[id(link)][1]

    def close(self):
        for _, h in self._idx.values():
            self.L.tsqa_index_destroy(h)
        self.indexer.close()


@pytest.fixture(scope="module")
def env(tsq, oracle):
    e = Env(tsq, oracle)
    yield e
    e.close()


class Gate:
    def __init__(self):
        import torch
        self.torch = torch
        self.x = torch.randint(0, 1 << 30, (1 << 24,), dtype=torch.int32, device="cuda")

        def timed(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                torch.sort(self.x)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        timed(2)                                          # (the first sort loads its kernels)
        self.reps = max(1, int(np.ceil(25.0 / max(timed(1), 0.05))))          # about 25 ms of sorting
        self.ms = timed(self.reps)

    def run(self):
        """on the current stream"""
        for _ in range(self.reps):
            self.torch.sort(self.x)


@pytest.fixture(scope="module")
def gate():
    g = Gate()
    print(f"gate: {g.reps} x torch.sort of 2^24 int32 = {g.ms:.1f} ms")
    return g


class Run:
    """one link made ready: device buffers, the call, and what must be there afterwards"""

    def __init__(self, link, env):
        torch = env.torch
        self.link, self.env = link, env
        self.status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.buffers = []            # (device buffer, host guard image, [(at, length, wanted bytes or None: undefined)])
        self.words = []              # (device table, wanted values)
        self.host_total = None
        self.keep = []
        self.call = None             # (context, stream) -> rc
        self.sync_call = None        # the synchronous form of the same call, for the four kinds that have one here

    def table(self, n, dtype=None):
        """a size word or table of the caller's own, poisoned"""
        return self.env.torch.full((n,), -1, dtype=dtype or self.env.torch.int64, device="cuda")


def prepare(link, rng, env, earlier=()):
    """-> Run.  `earlier`: the runs of the chain so far (a PD or F with a source finds its source's buffers there)"""
    L, torch = env.L, env.torch
    r = Run(link, env)
    st = r.status.data_ptr()
    k = link.kind
    if k == "C":
        src, n = env.dev(link.data), link.want.size
        outs, cap = fenced(rng, [n])
        out, guard = env.fresh(cap)
        size = r.table(1)
        r.buffers.append((out, guard, [(outs[0], n, link.want)]))
        r.words.append((size, [n]))
        r.call = lambda h, s: L.tsqa_compress_device_async(h, src.data_ptr(), src.numel(), out.data_ptr() + outs[0], n, size.data_ptr(), st, link.ext, s)

        def sync(h, s):
            got = C.c_size_t(0)
            rc = L.tsqa_compress_device(h, src.data_ptr(), src.numel(), out.data_ptr() + outs[0], n, C.byref(got), link.ext, s)
            return rc, [got.value]
        r.sync_call = sync
    elif k == "D":
        blob = env.dev(link.blob)
        outs, cap = fenced(rng, [link.out_len])
        out, guard = env.fresh(cap)
        size = r.table(1)
        r.buffers.append((out, guard, [(outs[0], link.out_len, None if link.fail else link.plain)]))
        if not link.fail:
            r.words.append((size, [link.out_len]))
        r.call = lambda h, s: L.tsqa_decompress_device_async(h, blob.data_ptr(), blob.numel(), link.stated, out.data_ptr() + outs[0], link.out_len,
                                                             size.data_ptr(), st, s)

        def sync(h, s):
            got = C.c_size_t(0)
            rc = L.tsqa_decompress_device(h, blob.data_ptr(), blob.numel(), out.data_ptr() + outs[0], link.out_len, C.byref(got), s)
            return rc, [got.value]
        r.sync_call = sync
    elif k == "E":
        src = env.dev(link.packed)
        out, guard = env.fresh(SLOTS_FRONT + link.n_blocks * SLOT + 64)
        sizes = r.table(link.n_blocks, torch.int32)
        # a slot holds its stream; what lies behind the stream inside the slot is the encoder's to use
        r.buffers.append((out, guard, [(SLOTS_FRONT + b * SLOT, SLOT, np.frombuffer(w, dtype=np.uint8)) for b, w in enumerate(link.want_streams)]))
        r.words.append((sizes, link.want_sizes))
        r.slots = out
        r.call = lambda h, s: L.tsqa_encode_blocks_async(h, src.data_ptr(), link.n_blocks, cg.STRIDE, link.last_len, link.ext,
                                                         out.data_ptr() + SLOTS_FRONT, sizes.data_ptr(), st, s)
    elif k == "F":
        if link.source is None:
            streams = env.dev(link.streams).data_ptr()
        else:
            streams = [x for x in earlier if x.link is link.source][-1].slots.data_ptr() + SLOTS_FRONT
        table = np.zeros(len(link.frames), dtype=FRAME)
        for b, (sa, oa, ln, ext, ol) in enumerate(link.frames):
            table[b] = (sa, oa, ln, ext, ol, 0)
        frames = to_dev(table.view(np.uint8))
        outs, cap = fenced(rng, [link.out_len])
        out, guard = env.fresh(cap)
        r.buffers.append((out, guard, [(outs[0], link.out_len, link.plain)]))
        r.keep.append(frames)
        r.call = lambda h, s: L.tsqa_decode_blocks_async(h, streams, frames.data_ptr(), len(link.frames), out.data_ptr() + outs[0], st, s)
    elif k == "S":
        host = env.pinned(link.blob)
        streams = torch.empty(link.n_local * SLOT, dtype=torch.uint8, device="cuda")
        outs, cap = fenced(rng, [link.out_len])
        out, guard = env.fresh(cap)
        r.buffers.append((out, guard, [(outs[0] + at, p.size, p) for at, p in link.pieces]))
        r.host_total = C.c_uint64(0)
        r.streams, r.out, r.out_at = streams, out, outs[0]
        r.call = lambda h, s: L.tsqa_sharded_fetch_decode_async(h, host.data_ptr(), host.numel(), link.rank, link.world, streams.data_ptr(),
                                                                streams.numel(), out.data_ptr() + outs[0], link.out_len, st,
                                                                C.byref(r.host_total), s)
    elif k == "R":
        idx = env.index(link)
        outs, cap = fenced(rng, [ln for _, ln in link.ranges])
        out, guard = env.fresh(cap)
        rr = _range_array([(o, ln, a) for (o, ln), a in zip(link.ranges, outs)])
        r.buffers.append((out, guard, [(a, ln, None if link.plain is None else link.plain[o:o + ln]) for (o, ln), a in zip(link.ranges, outs)]))
        r.call = lambda h, s: L.tsqa_decompress_ranges_async(h, idx, rr, len(link.ranges), out.data_ptr(), cap, st, s)
        r.sync_call = lambda h, s: (L.tsqa_decompress_ranges(h, idx, rr, len(link.ranges), out.data_ptr(), cap, s), None)
    elif k == "I":
        idx = env.index(link)
        outs, cap = fenced(rng, [ln for _, _, ln in link.ranges])
        out, guard = env.fresh(cap)
        rr = _item_range_array([(i, o, ln, a) for (i, o, ln), a in zip(link.ranges, outs)])
        r.buffers.append((out, guard, [(a, ln, link.plains[i][o:o + ln]) for (i, o, ln), a in zip(link.ranges, outs)]))
        r.call = lambda h, s: L.tsqa_decompress_item_ranges_async(h, idx, rr, len(link.ranges), out.data_ptr(), cap, st, s)
    elif k == "BC":
        arena, n = env.dev(link.arena), len(link.spans)
        outs, cap = fenced(rng, link.rooms)
        out, guard = env.fresh(cap)
        items = _batch_array([(o, ln, a, room) for (o, ln), a, room in zip(link.spans, outs, link.rooms)])
        sizes = r.table(n)
        r.buffers.append((out, guard, [(a, room, None if i == link.tight else w) for i, (a, room, w) in enumerate(zip(outs, link.rooms, link.want))]))
        r.words.append((sizes, [w.size for w in link.want]))
        r.call = lambda h, s: L.tsqa_compress_batch_async(h, arena.data_ptr(), arena.numel(), items, n, link.ext, out.data_ptr(), cap,
                                                          sizes.data_ptr(), st, s)

        def sync(h, s):
            got = (C.c_uint64 * n)()
            rc = L.tsqa_compress_batch(h, arena.data_ptr(), arena.numel(), items, n, link.ext, out.data_ptr(), cap, got, s)
            return rc, [int(x) for x in got]
        r.sync_call = sync
    elif k == "BD":
        arena, n = env.dev(link.arena), len(link.spans)
        outs, cap = fenced(rng, link.lengths)
        out, guard = env.fresh(cap)
        items = _batch_array([(o, ln, a, room) for (o, ln), a, room in zip(link.spans, outs, link.lengths)])
        blocks = np.ones(n, dtype=np.uint32)
        sizes = r.table(n)
        # (a refused batch is all or nothing: the destinations of its healthy items are undefined too)
        r.buffers.append((out, guard, [(a, ln, None if link.fail else p) for a, ln, p in zip(outs, link.lengths, link.plains)]))
        if not link.fail:
            r.words.append((sizes, link.lengths))
        r.call = lambda h, s: L.tsqa_decompress_batch_async(h, arena.data_ptr(), arena.numel(), items, blocks.ctypes.data, n, out.data_ptr(), cap,
                                                            sizes.data_ptr(), st, s)
    elif k == "PC":
        arena, n = env.dev(link.arena), len(link.spans)
        front = int(rng.integers(1, 48))
        out, guard = env.fresh(front + link.offsets[n] + 64)
        items = _batch_array([(o, ln, 0, 0) for o, ln in link.spans])
        offsets, sizes = r.table(n + 1), r.table(n)
        dests = [(front + o, sz, w) for o, sz, w in zip(link.offsets, link.sizes, link.want)]
        if link.fail:                # the cut container: what of it fits may be written, nothing at or past out_size
            dests[link.tight] = (front + link.offsets[link.tight], link.out_size - link.offsets[link.tight], None)
        r.buffers.append((out, guard, dests))
        r.words += [(offsets, link.offsets), (sizes, link.sizes)]
        r.arena, r.front, r.offsets, r.sizes = out, front, offsets, sizes
        r.call = lambda h, s: L.tsqa_compress_batch_packed_async(h, arena.data_ptr(), arena.numel(), items, n, link.ext, cg.ALIGN,
                                                                 out.data_ptr() + front, link.out_size, offsets.data_ptr(), sizes.data_ptr(), st, s)
    elif k == "PD":
        n = len(link.lengths)
        if link.source is None:
            arena = env.dev(link.arena).data_ptr()
            offsets, sizes = to_dev(np.array(link.offsets, dtype=np.int64)), to_dev(np.array(link.sizes, dtype=np.int64))
        else:
            pc = [x for x in earlier if x.link is link.source][-1]
            arena, offsets, sizes = pc.arena.data_ptr() + pc.front, pc.offsets, pc.sizes
        outs, cap = fenced(rng, link.lengths)
        out, guard = env.fresh(cap)
        items = _batch_array([(0, 0, a, ln) for a, ln in zip(outs, link.lengths)])
        blocks = np.ones(n, dtype=np.uint32)
        out_sizes = r.table(n)
        r.buffers.append((out, guard, [(a, ln, None if link.fail else p) for a, ln, p in zip(outs, link.lengths, link.plains)]))
        if not link.fail:
            r.words.append((out_sizes, link.lengths))
        r.keep += [offsets, sizes]
        r.call = lambda h, s: L.tsqa_decompress_batch_packed_async(h, arena, link.arena_size, offsets.data_ptr(), sizes.data_ptr(), items,
                                                                   blocks.ctypes.data, n, out.data_ptr(), cap, out_sizes.data_ptr(), st, s)
    return r


def check_buffers(r):
    """every destination the oracle's bytes (a shorter expectation: the region's first bytes), every other byte the sentinel"""
    for out, guard, dests in r.buffers:
        host = out.cpu().numpy()
        expected = guard.copy()
        for at, ln, want in dests:
            expected[at:at + ln] = host[at:at + ln]                       # undefined unless stated
            if want is not None:
                expected[at:at + len(want)] = want
        if not np.array_equal(host, expected):
            bad = np.flatnonzero(host != expected)
            where = [i for i, (at, ln, _) in enumerate(dests) if at <= bad[0] < at + ln]
            raise AssertionError(f"{r.link}: {bad.size} bytes differ, the first at {int(bad[0])} "
                                 f"({'destination %d' % where[0] if where else 'outside every destination'}): "
                                 f"{int(host[bad[0]])} for {int(expected[bad[0]])}")


def check(r, status=None):
    link = r.link
    got = int(r.status.item()) if status is None else status
    assert got == link.want_status, f"{link}: status word {got}, expected {link.want_status}"
    for table, want in r.words:
        assert table.cpu().tolist() == list(want), f"{link}: a size word or table differs from the oracle's values"
    if r.host_total is not None:
        assert r.host_total.value == link.total, link
    check_buffers(r)


def run_chain(codec, links, rng, env, gate, side, key, make=None):
    """prepare every link (make: a prepare that knows more kinds, test_gpu_call_chains_device.py's), open the gate's work on `side`,
    enqueue every link behind it with no synchronise, wait once -> the runs"""
    torch = env.torch
    runs = []
    for x in links:
        runs.append((make or prepare)(x, rng, env, runs))
    torch.cuda.synchronize()
    stream = C.c_void_p(side.cuda_stream)
    with torch.cuda.stream(side):
        gate.run()
        for r in runs:
            rc = r.call(codec.h, stream)
            assert rc == 0, f"{r.link} in {links}: the call returned {rc} ({codec.last_error()})"
        done = torch.cuda.Event()
        done.record(side)
        held = not done.query()
    side.synchronize()
    s = STATS.setdefault(key, [0, 0])
    s[0] += held
    s[1] += 1
    return runs


def report(key):
    held, n = STATS.get(key, [0, 0])
    print(f"{key}: the gate held for {held} of {n} chains")


def fresh_codec(tsq, decode_variant=4):
    c = tsq.DeviceCodec(0)
    c.set_variant(0, decode_variant)
    return c


@pytest.fixture(scope="module")
def shared(tsq):
    c = fresh_codec(tsq)
    yield c
    c.close()


@pytest.mark.parametrize("first", KINDS)
def test_every_ordered_pair(tsq, env, gate, shared, first):
    """Every ordered pair of entry points with `first` in front, the second link enqueued behind the first with no synchronise.
    (small, large): on a fresh context per pair, so the second link grows the scratch the first has just been given -- the growth
    waits, so this order exercises "grown safely behind what is enqueued", not overlap.  (large, small): on one shared context
    whose scratch is already large, so nothing waits and the second link is enqueued behind the running gate and first link.
    Decode variant 4 (one workgroup per block) waits for nobody.  Cannot prove: that the stream wait in reserve() is what keeps a
    freed buffer from a running kernel (hipFree waits for the device by itself)."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng([51, KINDS.index(first)])
    t0 = time.time()
    for a, b in env.gen.pairs():
        if a.kind != first:
            continue
        growing = (a.shape, b.shape) == ("small", "large")
        codec = fresh_codec(tsq) if growing else shared
        try:
            shared.set_variant(0, 4)
            runs = run_chain(codec, [a, b], rng, env, gate, side, "test_every_ordered_pair")
            for r in runs:
                check(r)
        finally:
            if growing:
                codec.close()
        PAIRS_DONE[(a.kind, b.kind, a.shape, b.shape)] = 1
    report("test_every_ordered_pair")
    print(f"row {first}: {time.time() - t0:.2f} s")


def test_every_pair_was_run():
    assert len(PAIRS_DONE) == 242, f"{len(PAIRS_DONE)} of 242 pairs ran"
    print("pairs run: 242 of 242")


def test_triples_through_both_upload_rings(tsq, env, gate):
    """Three calls in flight on one ring of two upload slots: the third takes the first's slot (and waits for the first on the
    host).  Ring range_up: R, I, R and I, R, I; ring batch_up: BC, BD, PC; PD, BC, BD; BD, PC, PD; each as (small, small, large),
    where the third call regrows the first's slot while the second is pending, and as (large, small, small); a fresh context per
    triple.  Then tsqa_index_create_batch, which takes two batch_up slots itself, on the drained context.  Cannot prove that the
    event wait in acquire() is needed for these sizes: the first call of a triple has usually finished when the third is made."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng(52)
    spare = env.gen.link("I", "small", 1)
    for chain in env.gen.triples():
        codec = fresh_codec(tsq)
        try:
            runs = run_chain(codec, chain, rng, env, gate, side, "test_triples_through_both_upload_rings")
            for r in runs:
                check(r)
            arena, h = env.dev(spare.arena), C.c_void_p()
            verdicts = (C.c_int32 * len(spare.spans))(*([-1] * len(spare.spans)))
            rc = env.L.tsqa_index_create_batch(codec.h, arena.data_ptr(), arena.numel(), _batch_array([(a, n, 0, 0) for a, n in spare.spans]),
                                               len(spare.spans), C.byref(h), verdicts)
            assert rc == 0 and h and not any(verdicts), (chain, rc, codec.last_error())
            assert [int(env.L.tsqa_index_item_total(h, i)) for i in range(len(spare.spans))] == [p.size for p in spare.plains]
            env.L.tsqa_index_destroy(h)
        finally:
            codec.close()
    report("test_triples_through_both_upload_rings")


@pytest.mark.parametrize("seed", [0, 1])
def test_a_seeded_walk_of_forty_links(tsq, env, gate, seed):
    """Forty links drawn over all eleven kinds and both shapes on ONE fresh context and one stream, one synchronise at the end.
    Every PD reads the tables and the arena the nearest earlier PC left on the device, every F the slots of the nearest earlier E
    through a frame table of the oracle's sizes.  Four links fail (chaingen.WALK_FAILURES[seed]; a failing PD brings its own
    tables): each leaves exactly its code in its OWN status word, its destination undefined but fenced; every other link is exact
    with status 0.  Then one synchronous call of four kinds on the same stream: TSQA_OK and exact, so the context's internal status
    word carries no neighbour's failure.  Cannot prove: overlap between any two particular links (links that grow scratch or
    reuse an upload slot wait on the host)."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng([53, seed])
    chain = env.gen.walk(seed)
    codec = fresh_codec(tsq)
    try:
        t0 = time.time()
        runs = run_chain(codec, chain, rng, env, gate, side, "test_a_seeded_walk_of_forty_links")
        for r in runs:
            check(r)
        stream = C.c_void_p(side.cuda_stream)
        for kind, v in (("C", 1), ("D", 2), ("R", 3), ("BC", 0)):
            link = env.gen.link(kind, "small", v)
            r = prepare(link, rng, env)
            torch.cuda.synchronize()
            rc, sizes = r.sync_call(codec.h, stream)
            assert rc == 0, f"synchronous {link} behind the walk: {rc} ({codec.last_error()})"
            if sizes is not None:
                assert sizes == list(r.words[0][1]), link
            check_buffers(r)
        print(f"walk {seed}: {time.time() - t0:.2f} s, failing links at {[k for k, x in enumerate(chain) if x.fail]}")
    finally:
        codec.close()
    report("test_a_seeded_walk_of_forty_links")


@pytest.mark.parametrize("first", KINDS)
def test_pairs_at_the_default_decoder(tsq, env, gate, first):
    """The pairs with a decoding kind (D, F, S, BD, PD, R, I) in first or second place, both links large, at decode variant 0 on
    one context: the library picks several workgroups per block for three blocks and for the 44-block tail of a 300-block batch,
    so reserve_duo grows the ring behind a multi-workgroup decode.  TSQA_ERR_STALL in a link's own word is the documented outcome
    on a busy machine: that link alone is decoded again at variant 4 after the synchronise.  No other code is accepted and no
    link is left unchecked.  Cannot prove that a stall would be reported rather than hang: none is provoked."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng([54, KINDS.index(first)])
    codec = fresh_codec(tsq, decode_variant=0)
    stalls = 0
    try:
        for a, b in env.gen.default_decoder_pairs():
            if a.kind != first:
                continue
            codec.set_variant(0, 0)
            runs = run_chain(codec, [a, b], rng, env, gate, side, "test_pairs_at_the_default_decoder")
            for r in runs:
                if int(r.status.item()) == ERR_STALL and r.link.kind in cg.DECODERS:
                    stalls += 1
                    print(f"{r.link} behind/in front of its neighbour reported TSQA_ERR_STALL: decoding it again with decode variant 4")
                    codec.set_variant(0, 4)
                    r = run_chain(codec, [r.link], rng, env, gate, side, "test_pairs_at_the_default_decoder (again)")[0]
                check(r)
    finally:
        codec.close()
    STALLS[0] += stalls
    print(f"row {first} at the default decoder: {stalls} stall(s), {STALLS[0]} so far")
    report("test_pairs_at_the_default_decoder")


@pytest.mark.parametrize("between", ["R I BC", "R D BC", "I BD"])
def test_sharded_decode_again_after_a_chain(tsq, env, gate, between):
    """A large sharded fetch-and-decode, then other calls behind it, then the S link's destination overwritten with the sentinel
    on the stream, then tsqa_sharded_decode_again_async.  Behind R, I and BC, none of which writes the context's frame
    descriptors, it must reproduce S's output.  With D or BD in between the descriptors are gone: TSQA_ERR_ARG on the host,
    nothing enqueued, the destination stays the sentinel and the status word given to it untouched."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng(55)
    kinds = between.split()
    s_link = env.gen.link("S", "large", 0)
    # (the batches small: three blocks, no more than S's three, so the per-block scratch -- the descriptors with it -- is not regrown)
    chain = [s_link] + [env.gen.link(k, "large" if k in ("R", "I") else "small", n) for n, k in enumerate(kinds)]
    forgotten = any(k in cg.WRITES_FRAMES for k in kinds)
    codec = fresh_codec(tsq)
    try:
        runs = run_chain(codec, chain, rng, env, gate, side, "test_sharded_decode_again_after_a_chain")
        for r in runs:
            check(r)
        s = runs[0]
        again = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        stream = C.c_void_p(side.cuda_stream)
        with torch.cuda.stream(side):
            s.out.copy_(env.guard_dev[:s.out.numel()])
            rc = env.L.tsqa_sharded_decode_again_async(codec.h, s.streams.data_ptr(), s.out.data_ptr() + s.out_at, again.data_ptr(), stream)
        side.synchronize()
        if forgotten:
            assert rc == ERR_ARG, (between, rc)
            assert int(again.item()) == -1 and np.array_equal(s.out.cpu().numpy(), s.buffers[0][1]), "a refused decode_again wrote something"
        else:
            assert rc == 0, (between, rc, codec.last_error())
            check(s, status=int(again.item()))
    finally:
        codec.close()
    report("test_sharded_decode_again_after_a_chain")
