"""GPU tests of the second call-chain catalogue (tests/chaingen.py, NEW_KINDS): the twelve stream-ordered entry points whose plans
are made on the device -- the per-item and the dense batch decompress, the compress from device tables and the split compresses,
the sized decompress, the sized and the packed index, the join, the cut, the take and the gather -- enqueued behind one another
and behind the eleven kinds of the first catalogue on ONE context and one stream, with no synchronise between them.  The host
never clears the scratch these calls share (the batch tables, the per-block descriptors, the table, cut and gather scratch): each
kernel family has to initialise what it reads, and a word that one entry point leaves dirty is what the next one finds.

The harness is test_gpu_call_chains.py's: every link has its own destinations behind 1 to 47 guard bytes in a sentinel-filled
buffer, a status word poisoned with -1 and poisoned size words and tables; after one synchronise every status, every table and
every byte inside and outside the destinations is held against the generator's expectation, none of which comes from the library.

What these tests cannot prove is what test_gpu_call_chains.py cannot: that a wait inside the library is the one that protects a
buffer (hipFree waits for the device by itself), and overlap between two particular links: a link that grows scratch waits."""
import ctypes as C
import time

import numpy as np
import pytest

import chaingen as cg
from chaingen import ALIGN, ALL_KINDS, ERR_ARG, ERR_STALL, NEW_KINDS, SPLIT_LEN
from test_gpu_call_chains import Env, Gate, Run, check, check_buffers, fresh_codec, prepare, report, run_chain  # noqa: F401
from test_gpu_range import fenced, to_dev, tsq  # noqa: F401 (tsq: fixture)
from turbosqueeze_amd.api import _DeviceWords, _batch_array, _range_array

pytestmark = pytest.mark.gpu

PAIRS2_DONE: dict = {}               # (first kind, second kind, first shape, second shape) -> 1
STALLS = [0]


class Env2(Env):
    """Env with the indexes of the cut (tsqa_index_create over the link's container) and the take (tsqa_index_create_batch: the
    base class's, the link has an arena and spans)"""

    def index(self, link):
        if link.kind == "K" and id(link) not in self._idx:
            h, blob = C.c_void_p(), self.dev(link.blob)
            rc = self.L.tsqa_index_create(self.indexer.h, blob.data_ptr(), blob.numel(), C.byref(h))
            assert rc == 0 and h, (link, rc, self.indexer.last_error())
            self._idx[id(link)] = (link, h)
        return super().index(link)


@pytest.fixture(scope="module")
def env(tsq, oracle):
    e = Env2(tsq, oracle)
    yield e
    e.close()


@pytest.fixture(scope="module")
def gate():
    g = Gate()
    print(f"gate: {g.reps} x torch.sort of 2^24 int32 = {g.ms:.1f} ms")
    return g


def u64(values):
    return to_dev(np.array([int(v) for v in values], dtype=np.uint64).view(np.int64))


def u32(values):
    return to_dev(np.array([int(v) for v in values], dtype=np.uint32).view(np.int32))


def padded(values, n):
    """a table of n words of which the call owes the first len(values): the rest keeps its poison"""
    return list(values) + [-1] * (n - len(values))


def hold(link, tables):
    """the device tables that a waiting form has filled, against the expectation"""
    for table, want in tables:
        assert table.cpu().tolist() == list(want), f"synchronous {link}: a size word or table differs from the expectation"


def packed_source(link, env, earlier):
    """-> (arena address, d_offsets, d_sizes, what keeps them alive): the link's own packed arena from the host, or what its source
    has left on the device"""
    if link.source is None:
        arena, offsets, sizes = env.dev(link.arena), u64(link.offsets), u64(link.sizes)
        return arena.data_ptr(), offsets, sizes, [arena, offsets, sizes]
    src = [x for x in earlier if x.link is link.source][-1]
    return src.arena.data_ptr() + src.front, src.offsets, src.sizes, []


def prepare2(link, rng, env, earlier=()):
    """test_gpu_call_chains.prepare with the kinds of the second catalogue -> Run.  r.after: checks that need the host after the
    synchronise (an index's own tables); r.idx: an index the link has made, destroyed by close_run."""
    k = link.kind
    if k not in NEW_KINDS:
        return prepare(link, rng, env, earlier)
    L, torch = env.L, env.torch
    r = Run(link, env)
    r.after, r.idx = [], None
    st = r.status.data_ptr()
    i32 = torch.int32
    if k == "DI":
        arena, n = env.dev(link.arena), link.items
        outs, cap = fenced(rng, link.lengths)
        out, guard = env.fresh(cap)
        blocks = np.ones(n, dtype=np.uint32)
        sizes, verdicts = r.table(n), r.table(n, i32)
        r.buffers.append((out, guard, [(a, ln, p) for a, ln, p in zip(outs, link.lengths, link.plains)]))
        r.words += [(sizes, link.lengths), (verdicts, [0] * n)]
        if link.packed:
            offsets, places = u64([o for o, _ in link.spans]), u64([z for _, z in link.spans])
            items = _batch_array([(0, 0, a, ln) for a, ln in zip(outs, link.lengths)])
            r.call = lambda h, s: L.tsqa_decompress_batch_packed_items_async(h, arena.data_ptr(), link.arena_size, offsets.data_ptr(), places.data_ptr(),
                                                                             items, blocks.ctypes.data, n, out.data_ptr(), cap, sizes.data_ptr(),
                                                                             verdicts.data_ptr(), st, s)
        else:
            items = _batch_array([(o, z, a, ln) for (o, z), a, ln in zip(link.spans, outs, link.lengths)])
            r.call = lambda h, s: L.tsqa_decompress_batch_items_async(h, arena.data_ptr(), arena.numel(), items, blocks.ctypes.data, n, out.data_ptr(),
                                                                      cap, sizes.data_ptr(), verdicts.data_ptr(), st, s)
    elif k == "DD":
        arena, offsets, places, keep = packed_source(link, env, earlier)
        n, front = link.items, int(rng.integers(1, 48))
        out, guard = env.fresh(front + link.out_size + 64)
        out_offsets, out_sizes, first, verdicts = r.table(n + 1), r.table(n), r.table(n + 1), r.table(n, i32)
        # (an item that a decoder refuses: its own range is undefined, and as long as its header says)
        r.buffers.append((out, guard, [(front + o, len(p) if p is not None else t, None if p is None else np.frombuffer(p, dtype=np.uint8))
                                       for o, p, t in zip(link.out_offsets, link.plains, link.batch.totals)]))
        r.words += [(out_offsets, link.out_offsets), (out_sizes, link.out_sizes), (first, link.first_block), (verdicts, link.item_status)]
        r.keep += keep
        r.call = lambda h, s: L.tsqa_decompress_batch_packed_dense_async(h, arena, link.arena_size, offsets.data_ptr(), places.data_ptr(), n, ALIGN,
                                                                         link.cap_blocks, out.data_ptr() + front, link.out_size, out_offsets.data_ptr(),
                                                                         out_sizes.data_ptr(), first.data_ptr(), verdicts.data_ptr(), st, s)
    elif k == "TC":
        data, n = env.dev(link.data), link.items
        in_offsets, in_sizes = u64(link.in_offsets), u64(link.in_sizes)
        front = int(rng.integers(1, 48))
        out, guard = env.fresh(front + link.out_size + 64)
        offsets, sizes, first, bound, verdicts = r.table(n + 1), r.table(n), r.table(n + 1), r.table(1), r.table(n, i32)
        r.buffers.append((out, guard, [(front + o, len(c), np.frombuffer(c, dtype=np.uint8)) for o, c in zip(link.offsets, link.containers) if c]))
        r.words += [(offsets, link.offsets), (sizes, link.sizes), (first, link.first_block), (bound, [link.bound]), (verdicts, link.item_status)]
        r.arena, r.front, r.offsets, r.sizes = out, front, offsets, sizes
        if link.split:
            table = r.table(link.cap_blocks, i32)
            r.words.append((table, padded(link.block_sizes, link.cap_blocks)))
            r.call = lambda h, s: L.tsqa_compress_batch_packed_tables_split_async(h, data.data_ptr(), data.numel(), in_offsets.data_ptr(),
                                                                                  in_sizes.data_ptr(), n, link.cap_blocks, link.ext, ALIGN, SPLIT_LEN,
                                                                                  out.data_ptr() + front, link.out_size, offsets.data_ptr(),
                                                                                  sizes.data_ptr(), first.data_ptr(), bound.data_ptr(), table.data_ptr(),
                                                                                  verdicts.data_ptr(), st, s)
        else:
            r.call = lambda h, s: L.tsqa_compress_batch_packed_tables_async(h, data.data_ptr(), data.numel(), in_offsets.data_ptr(), in_sizes.data_ptr(),
                                                                            n, link.cap_blocks, link.ext, ALIGN, out.data_ptr() + front, link.out_size,
                                                                            offsets.data_ptr(), sizes.data_ptr(), first.data_ptr(), bound.data_ptr(),
                                                                            verdicts.data_ptr(), st, s)
    elif k == "PS":
        data, n = env.dev(link.data), link.items
        front = int(rng.integers(1, 48))
        out, guard = env.fresh(front + link.out_size + 64)
        items = _batch_array([(o, z, 0, 0) for o, z in link.spans])
        offsets, sizes, table = r.table(n + 1), r.table(n), r.table(link.blocks, i32)
        r.buffers.append((out, guard, [(front + o, len(c), np.frombuffer(c, dtype=np.uint8)) for o, c in zip(link.offsets, link.containers)]))
        r.words += [(offsets, link.offsets), (sizes, link.sizes), (table, link.block_sizes)]
        r.arena, r.front, r.offsets, r.sizes = out, front, offsets, sizes
        r.call = lambda h, s: L.tsqa_compress_batch_packed_split_async(h, data.data_ptr(), data.numel(), items, n, link.ext, ALIGN, SPLIT_LEN,
                                                                       out.data_ptr() + front, link.out_size, offsets.data_ptr(), sizes.data_ptr(),
                                                                       table.data_ptr(), st, s)
    elif k == "SC":
        src, n = env.dev(link.data), link.want.size
        outs, cap = fenced(rng, [n])
        out, guard = env.fresh(cap)
        size, table = r.table(1), r.table(link.blocks, i32)
        r.buffers.append((out, guard, [(outs[0], n, link.want)]))
        r.words += [(size, [n]), (table, link.want_sizes)]
        r.out, r.out_at, r.block_sizes = out, outs[0], table
        r.call = lambda h, s: L.tsqa_compress_device_split_async(h, src.data_ptr(), src.numel(), SPLIT_LEN, out.data_ptr() + outs[0], n, size.data_ptr(),
                                                                 table.data_ptr(), st, link.ext, s)

        def sync(h, s):
            got = C.c_size_t(0)
            rc = L.tsqa_compress_device_split(h, src.data_ptr(), src.numel(), SPLIT_LEN, out.data_ptr() + outs[0], n, C.byref(got), table.data_ptr(),
                                              link.ext, s)
            hold(link, r.words[1:])
            return rc, [got.value]
        r.sync_call = sync
    elif k == "SD":
        if link.source is None:
            blob, table = env.dev(link.blob), u32(link.table)
            blob_at = blob.data_ptr()
            r.keep += [blob, table]
        else:
            sc = [x for x in earlier if x.link is link.source][-1]
            blob_at, table = sc.out.data_ptr() + sc.out_at, sc.block_sizes
        outs, cap = fenced(rng, [link.out_len])
        out, guard = env.fresh(cap)
        size = r.table(1)
        r.buffers.append((out, guard, [(outs[0], link.out_len, link.plain)]))
        r.words.append((size, [link.out_len]))
        r.call = lambda h, s: L.tsqa_decompress_device_sized_async(h, blob_at, link.n, link.blocks, table.data_ptr(), out.data_ptr() + outs[0],
                                                                   link.out_len, size.data_ptr(), st, s)
    elif k == "XS":
        blob, table = env.dev(link.blob), u32(link.table)
        outs, cap = fenced(rng, [ln for _, ln in link.ranges])
        out, guard = env.fresh(cap)
        rr = _range_array([(o, ln, a) for (o, ln), a in zip(link.ranges, outs)])
        # (a refused index: the read writes no destination byte at all)
        r.buffers.append((out, guard, [] if link.fail else [(a, ln, link.plain[o:o + ln]) for (o, ln), a in zip(link.ranges, outs)]))
        r.idx = C.c_void_p()

        def call(h, s):
            rc = L.tsqa_index_create_sized_async(h, blob.data_ptr(), blob.numel(), link.n_total, SPLIT_LEN, table.data_ptr(), C.byref(r.idx), s)
            return rc or L.tsqa_decompress_ranges_async(h, r.idx, rr, len(link.ranges), out.data_ptr(), cap, st, s)
        r.call = call

        def verdict():
            word = L.tsqa_index_d_status(r.idx)
            assert word, f"{link}: a sized index without a verdict word"
            got = torch.as_tensor(_DeviceWords(word, 1, "<i4"), device="cuda").cpu().tolist()
            assert got == [link.want_status], f"{link}: the index's verdict word {got}, expected {link.want_status}"
            assert (L.tsqa_index_blocks(r.idx), L.tsqa_index_total(r.idx), L.tsqa_index_items(r.idx)) == (link.n_blocks, link.n_total, 1), link
        r.after.append(verdict)
    elif k == "XP":
        arena, offsets, places, keep = packed_source(link, env, earlier)
        case, e, n = link.case, link.e, link.items
        first, table = (u64(case.table_first), u32(case.table)) if link.sized else (None, None)
        verdicts = r.table(n, i32)
        r.words.append((verdicts, e["item_status"]))
        r.keep += keep
        r.idx = C.c_void_p()
        r.call = lambda h, s: L.tsqa_index_create_packed_async(h, arena, link.arena_size, offsets.data_ptr(), places.data_ptr(), n, link.cap_blocks,
                                                               case.block_len if link.sized else 0, first.data_ptr() if link.sized else None,
                                                               table.data_ptr() if link.sized else None, case.table_words if link.sized else 0,
                                                               C.byref(r.idx), verdicts.data_ptr(), st, s)

        def tables():
            d_first, d_status, d_words = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert L.tsqa_index_device_tables(r.idx, C.byref(d_first), C.byref(d_status), C.byref(d_words)) == 0, link
            view = lambda p, count, kind: torch.as_tensor(_DeviceWords(p.value, count, kind), device="cuda").cpu().tolist()
            got = view(d_first, n + 1, "<i8"), view(d_status, n, "<i4"), view(d_words, 3, "<i8")
            assert got == (e["item_first"], e["item_status"], e["words"]), f"{link}: the index's device tables differ from the restatement"
            assert (L.tsqa_index_items(r.idx), L.tsqa_index_blocks(r.idx), L.tsqa_index_total(r.idx)) == (n, 0, 0), f"{link}: fetched already"
            rc = L.tsqa_index_fetch(env.indexer.h, r.idx, None)
            assert rc == 0, (link, rc, env.indexer.last_error())
            assert (L.tsqa_index_items(r.idx), L.tsqa_index_blocks(r.idx), L.tsqa_index_total(r.idx)) == (n, e["words"][0], e["words"][1]), link
            assert [int(L.tsqa_index_item_total(r.idx, i)) for i in range(n)] == e["totals"], link
            assert [L.tsqa_index_item_status(r.idx, i) for i in range(n)] == e["item_status"], link
            # the descriptors: one waiting read of everything through the fetched index, on the indexer's context
            total = e["words"][1]
            whole = torch.empty(total, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = L.tsqa_decompress_ranges(env.indexer.h, r.idx, _range_array([(0, total, 0)]), 1, whole.data_ptr(), total, None)
            assert rc == 0, (link, rc, env.indexer.last_error())
            assert whole.cpu().numpy().tobytes() == b"".join(case.datas), f"{link}: a read through the fetched index differs from the items' data"
        r.after.append(tables)
    elif k == "J":
        arena, offsets, places, keep = packed_source(link, env, earlier)
        n, front = link.items, int(rng.integers(1, 48))
        out, guard = env.fresh(front + link.out_size + 64)
        size, first, table, verdicts = r.table(1), r.table(n + 1), r.table(link.cap_blocks, i32), r.table(n, i32)
        # (all or nothing: on any nonzero status not one byte of the output and not one word of the size table)
        r.buffers.append((out, guard, [] if link.fail else [(front, link.out_size, np.frombuffer(link.container, dtype=np.uint8))]))
        r.words += [(size, [link.out_size]), (first, link.first_block), (verdicts, link.item_status),
                    (table, [-1] * link.cap_blocks if link.fail else link.block_sizes)]
        r.keep += keep
        r.call = lambda h, s: L.tsqa_join_async(h, arena, link.arena_size, offsets.data_ptr(), places.data_ptr(), n, link.cap_blocks,
                                                out.data_ptr() + front, link.out_cap, size.data_ptr(), first.data_ptr(), table.data_ptr(),
                                                verdicts.data_ptr(), st, s)

        def sync(h, s):
            got, nb = C.c_size_t(0), C.c_uint32(0)
            rc = L.tsqa_join(h, arena, link.arena_size, offsets.data_ptr(), places.data_ptr(), n, link.cap_blocks, out.data_ptr() + front,
                             link.out_cap, C.byref(got), C.byref(nb), first.data_ptr(), table.data_ptr(), verdicts.data_ptr(), s)
            assert nb.value == link.cap_blocks, link
            hold(link, r.words[1:])
            return rc, [got.value]
        r.sync_call = sync
    elif k in ("K", "T"):
        e, n = link.e, link.n_ranges
        if k == "T" and link.source is not None:
            idx = [x for x in earlier if x.link is link.source][-1].idx
        else:
            idx = env.index(link)
        items = u32(link.take_items) if k == "T" else None
        first, count = (u64([f for f, _ in link.ranges]), u64([c for _, c in link.ranges])) if link.ranges is not None else (None, None)
        front = int(rng.integers(1, 48))
        out, guard = env.fresh(front + link.out_size + 64)
        offsets, sizes, totals, verdicts = r.table(n + 1), r.table(n), r.table(n), r.table(n, i32)
        blobs = e["containers"] if k == "K" else [link.case.container(e, j) for j in range(n)]
        r.buffers.append((out, guard, [(front + o, len(b), np.frombuffer(b, dtype=np.uint8)) for o, b in zip(e["offsets"], blobs) if b is not None]))
        r.words += [(offsets, e["offsets"]), (sizes, e["sizes"]), (totals, e["totals"]), (verdicts, e["item_status"])]
        r.arena, r.front, r.offsets, r.sizes = out, front, offsets, sizes
        ptr = lambda t: t.data_ptr() if t is not None else None
        if k == "K":
            r.call = lambda h, s: L.tsqa_cut_async(h, idx, first.data_ptr(), count.data_ptr(), n, ALIGN, out.data_ptr() + front, link.out_size,
                                                   offsets.data_ptr(), sizes.data_ptr(), totals.data_ptr(), verdicts.data_ptr(), st, s)
        else:
            r.call = lambda h, s: L.tsqa_cut_items_async(h, idx, items.data_ptr(), ptr(first), ptr(count), n, ALIGN, out.data_ptr() + front,
                                                         link.out_size, offsets.data_ptr(), sizes.data_ptr(), totals.data_ptr(), verdicts.data_ptr(),
                                                         st, s)

            def sync(h, s):
                h_offsets, h_sizes, h_totals = np.full(n + 1, 7, dtype=np.uint64), np.full(n, 7, dtype=np.uint64), np.full(n, 7, dtype=np.uint64)
                h_status = np.full(n, -1, dtype=np.int32)
                rc = L.tsqa_cut_items(h, idx, items.data_ptr(), ptr(first), ptr(count), n, ALIGN, out.data_ptr() + front, link.out_size,
                                      h_offsets.ctypes.data, h_sizes.ctypes.data, h_totals.ctypes.data, h_status.ctypes.data, s)
                assert (h_offsets.tolist(), h_sizes.tolist(), h_totals.tolist(), h_status.tolist()) == (e["offsets"], e["sizes"], e["totals"],
                                                                                                     e["item_status"]), link
                return rc, None
            r.sync_call = sync
    elif k == "G":
        e, n = link.e, link.n_ranges
        idx = [x for x in earlier if x.link is link.source][-1].idx if link.source is not None else env.index(link.through)
        items = u32(link.g_items) if link.g_items is not None else None
        offsets, lengths = u64(link.offsets), u64(link.lengths)
        front = int(rng.integers(1, 48))
        out, guard = env.fresh(front + link.room + 64)
        out_offsets, verdicts, need = r.table(n + 1), r.table(n, i32), r.table(1)
        data = np.frombuffer(link.case.index.data, dtype=np.uint8)
        r.buffers.append((out, guard, [(front + o, ln, data[start:start + ln]) for o, (start, ln) in zip(e["out_offsets"], e["places"]) if ln]))
        r.words += [(out_offsets, e["out_offsets"]), (verdicts, e["range_status"]), (need, [e["need_pieces"]])]
        args = lambda h, s: (h, idx, items.data_ptr() if items is not None else None, offsets.data_ptr(), lengths.data_ptr(), n, ALIGN,
                             link.cap_pieces, out.data_ptr() + front, link.out_cap, out_offsets.data_ptr(), verdicts.data_ptr(), need.data_ptr(), st, s)
        r.call = lambda h, s: L.tsqa_gather_async(*args(h, s))

        def sync(h, s):
            rc = L.tsqa_gather(*args(h, s))
            hold(link, r.words)
            assert int(r.status.item()) == rc, link
            return rc, None
        r.sync_call = sync
    return r


def check2(r):
    check(r)
    for f in getattr(r, "after", ()):
        f()


def close_runs(env, runs):
    for r in runs:
        if getattr(r, "idx", None):
            env.L.tsqa_index_destroy(r.idx)
            r.idx = None


def chain2(codec, links, rng, env, gate, side, key):
    """run_chain with prepare2, every link checked, every index that a link has made destroyed -> the runs"""
    runs = []
    try:
        runs = run_chain(codec, links, rng, env, gate, side, key, make=prepare2)
        for r in runs:
            check2(r)
    finally:
        close_runs(env, runs)
    return runs


@pytest.fixture(scope="module")
def shared(tsq):
    c = fresh_codec(tsq)
    yield c
    c.close()


@pytest.mark.parametrize("first", ALL_KINDS)
def test_every_ordered_pair_with_a_new_kind(tsq, env, gate, shared, first):
    """Every ordered pair of chaingen.pairs2() with `first` in front -- 23 second kinds behind a new kind, the 12 new ones behind an
    old kind, each in both orders of shape: 46 or 24 chains --, the second link enqueued behind the first with no synchronise.
    (small, large): on a fresh context per pair, so the second link grows the scratch that the first has just been given -- the
    growth waits, so this order exercises "grown safely behind what is enqueued", not overlap.  (large, small): on one shared
    context whose scratch is large and dirty from every pair before, so nothing waits and the second link is enqueued behind the
    running gate and first link, onto words that another entry point wrote last.  Decode variant 4 waits for nobody.  Cannot
    prove: that a wait in a reserve* is the one that keeps a freed buffer from a running kernel (hipFree waits for the device by
    itself)."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng([61, ALL_KINDS.index(first)])
    key = "test_every_ordered_pair_with_a_new_kind"
    t0, n = time.time(), 0
    for a, b in env.gen.pairs2():
        if a.kind != first:
            continue
        growing = (a.shape, b.shape) == ("small", "large")
        codec = fresh_codec(tsq) if growing else shared
        try:
            shared.set_variant(0, 4)
            chain2(codec, [a, b], rng, env, gate, side, key)
        finally:
            if growing:
                codec.close()
        PAIRS2_DONE[(a.kind, b.kind, a.shape, b.shape)] = 1
        n += 1
    report(key)
    print(f"row {first} ({n} chains): {time.time() - t0:.2f} s")


def test_every_pair_with_a_new_kind_was_run():
    assert len(PAIRS2_DONE) == 816, f"{len(PAIRS2_DONE)} of 816 pairs ran"
    print("pairs run: 816 of 816")


def test_the_pipelines_read_what_their_producers_left(tsq, env, gate):
    """chaingen.pipelines(): split compress -> sized decode; packed, split and tables compress -> dense decompress, join and index of
    the arena -> gather and take through the index nobody has fetched -> dense decompress, join and index of the take's arena; one
    fresh context per chain, one synchronise at its end, no host read between the links.  Cannot prove overlap: the links depend on
    one another, and the stream orders them."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng(62)
    t0 = time.time()
    for chain in env.gen.pipelines():
        codec = fresh_codec(tsq)
        try:
            chain2(codec, chain, rng, env, gate, side, "test_the_pipelines_read_what_their_producers_left")
        finally:
            codec.close()
    report("test_the_pipelines_read_what_their_producers_left")
    print(f"pipelines: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("seed", [0, 1])
def test_a_seeded_walk_over_all_kinds(tsq, env, gate, seed):
    """Forty links drawn over all 23 kinds and both shapes on ONE fresh context and one stream, one synchronise at the end, wired
    by chaingen's source rules: an SD reads the container and the size table of the nearest earlier SC; a DD, J or XP the arena and
    the tables of the nearest earlier PC, PS, TC or T; a G or T the index of the nearest earlier XP, which nobody has fetched.  Six
    links fail (chaingen.FAILURES2, each with inputs of its own): each leaves exactly its codes in its OWN status word and tables,
    and what the contract leaves undefined stays fenced; every other link is exact with status 0.  Then one synchronous tsqa_join,
    tsqa_cut_items, tsqa_gather and tsqa_compress_device_split on the same stream: TSQA_OK and exact, so the context's internal
    status and size words carry no neighbour's failure.  Cannot prove: overlap between any two particular links."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng([63, seed])
    chain = env.gen.walk2(seed)
    codec = fresh_codec(tsq)
    runs = []
    try:
        t0 = time.time()
        runs = chain2(codec, chain, rng, env, gate, side, "test_a_seeded_walk_over_all_kinds")
        stream = C.c_void_p(side.cuda_stream)
        for kind, v in (("J", 1), ("T", 2), ("G", 3), ("SC", 0)):
            link = env.gen.link(kind, "small", v)
            r = prepare2(link, rng, env)
            torch.cuda.synchronize()
            rc, sizes = r.sync_call(codec.h, stream)
            assert rc == 0, f"synchronous {link} behind the walk: {rc} ({codec.last_error()})"
            if sizes is not None:
                assert sizes == list(r.words[0][1]), link
            check_buffers(r)
        print(f"walk2 {seed}: {time.time() - t0:.2f} s, failing links at {[(k, repr(x)) for k, x in enumerate(chain) if x.fail]}, "
              f"wired links at {[(k, repr(x), repr(x.source)) for k, x in enumerate(chain) if x.source is not None]}")
    finally:
        codec.close()
    report("test_a_seeded_walk_over_all_kinds")


@pytest.mark.parametrize("place", ["first", "second"])
def test_new_pairs_at_the_default_decoder(tsq, env, gate, place):
    """Of the new kinds only SD goes through launch_decode_frames with the context's decode variant (DI and DD always decode on one
    workgroup per block, and so do the reads of XS and G): the pairs with SD in `place` against all 23 kinds, both links large, at
    decode variant 0 on one context -- 300 blocks, so the library takes its several-workgroups decoder for the 44-block tail.
    TSQA_ERR_STALL in a decoding link's own word is the documented outcome on a busy machine: that link alone is decoded again at
    variant 4 after the synchronise.  No other code is accepted and no link is left unchecked.  Cannot prove that a stall would be
    reported rather than hang: none is provoked."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng([64, place == "second"])
    codec = fresh_codec(tsq, decode_variant=0)
    key = "test_new_pairs_at_the_default_decoder"
    stalls, t0 = 0, time.time()
    try:
        for a, b in env.gen.default_decoder_pairs2():
            if (a if place == "first" else b).kind != "SD" or (place == "second" and a.kind == "SD"):
                continue
            codec.set_variant(0, 0)
            runs = run_chain(codec, [a, b], rng, env, gate, side, key, make=prepare2)
            try:
                for r in runs:
                    if int(r.status.item()) == ERR_STALL and r.link.kind in cg.DECODERS + ("SD",):
                        stalls += 1
                        print(f"{r.link} behind/in front of its neighbour reported TSQA_ERR_STALL: decoding it again with decode variant 4")
                        codec.set_variant(0, 4)
                        r = run_chain(codec, [r.link], rng, env, gate, side, key + " (again)", make=prepare2)[0]
                    check2(r)
            finally:
                close_runs(env, runs)
    finally:
        codec.close()
    STALLS[0] += stalls
    print(f"SD {place} at the default decoder: {time.time() - t0:.2f} s, {stalls} stall(s), {STALLS[0]} so far")
    report(key)


@pytest.mark.parametrize("between", ["DI", "DD", "SD", "J", "XP", "TC PS SC XS K T G"])
def test_sharded_decode_again_behind_the_new_kinds(tsq, env, gate, between):
    """A large split compress that grows the per-block descriptors to 300 once and for all (tsqa_ctx::reserve forgets a sharded
    decode whenever they grow, whoever asks), then a large sharded fetch-and-decode of three blocks, then small links of the new
    kinds, then S's destination overwritten with the sentinel on the stream, then tsqa_sharded_decode_again_async.  Behind each
    kind of chaingen.WRITES_FRAMES2, alone, the descriptors are gone: TSQA_ERR_ARG on the host, nothing enqueued, the destination
    stays the sentinel and the status word given to it untouched.  Behind the seven kinds that do not write c->frames, all in one
    chain, it must reproduce S's output.  Cannot prove that a new writer of c->frames which is no kind here forgets."""
    import torch
    side = torch.cuda.Stream()
    rng = np.random.default_rng(65)
    kinds = between.split()
    assert set(kinds) <= set(NEW_KINDS) and (set(kinds) <= set(cg.WRITES_FRAMES2) or not set(kinds) & set(cg.WRITES_FRAMES2))
    s_link = env.gen.link("S", "large", 0)
    chain = [env.gen.link("SC", "large", 1), s_link] + [env.gen.link(k, "small", n) for n, k in enumerate(kinds)]
    assert s_link.blocks == 3 and all(x.blocks <= 300 for x in chain if hasattr(x, "blocks"))
    forgotten = any(k in cg.WRITES_FRAMES2 for k in kinds)
    codec = fresh_codec(tsq)
    runs = []
    try:
        runs = run_chain(codec, chain, rng, env, gate, side, "test_sharded_decode_again_behind_the_new_kinds", make=prepare2)
        for r in runs:
            check2(r)
        s = runs[1]
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
        close_runs(env, runs)
        codec.close()
    report("test_sharded_decode_again_behind_the_new_kinds")
