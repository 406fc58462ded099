"""Seeded links and chains for the call-chain tests (test_call_chains_cpu.py, test_gpu_call_chains.py).  Host only: numpy, the
oracle and the catalogue of hand-assembled streams; nothing here touches a device.

A link is ONE stream-ordered call of the C ABI with everything it needs: its inputs, the lengths of its destinations, the status
it must leave and the bytes, sizes and tables it must produce.  Every expected value is the oracle's (oracle.compress for
containers and block streams, the original bytes for decodes, after oracle.decompress(container) == original has been checked once
per input); none comes from the library.  A chain is a list of links for one stream with no synchronise between them.

Eleven kinds (KINDS), two shapes each: "small" stays under a fresh context's first capacities, "large" exceeds every capacity the
small shape establishes.  The capacities are restated from the runtime; each constant names its source line and has to be derived
again when that line changes (README.md lists them).

Twelve more kinds (NEW_KINDS: the second catalogue, test_gpu_call_chains_device.py): the entry points whose plans are made on the
device.  Their expectations are the feature generators' pure-Python restatements (joingen, cutgen, takegen, gathergen, densegen,
tablegen, batchsplitgen, splitgen, seekgen, packedindexgen), which the features' own CPU tests hold against the oracle and the
host-only planners; here they are fed with this module's inputs.  KINDS, pairs() and walk() are untouched by them."""
from __future__ import annotations

import numpy as np

import batchsplitgen as bsg
import cutgen
import densegen as dg
import fuzzgen
import gathergen as gg
import joingen as jg
import packedindexgen as pg
import seekgen as kg
import splitgen as sg
import streamgen
import tablegen as tg
import takegen as tk

BLOCK = 1 << 22                      # TSQ_BLOCK_SZ (include/turbosqueeze_amd.h)
SLOT = BLOCK + (BLOCK >> 2)          # TSQ_OUTPUT_SZ
HALO = 128                           # the look-ahead bytes behind a block of tsqa_encode_blocks_async
STRIDE = BLOCK + HALO

# ---- restated from the runtime (test_call_chains_cpu.py holds the shapes against them)
FIRST_BATCH_ITEMS = 256              # tsq_runtime.hip, tsqa_ctx::reserve_batch: `size_t want = 256; while (want < n_items) want *= 2;`
FIRST_UPLOAD_BYTES = 4096            # tsq_runtime.hip, tsqa_uploads::acquire: `size_t want = 4096; while (want < bytes) want *= 2;`
SIZEOF_BATCH_ITEM = 48               # tsq_runtime.hip, compress_batch_enqueue: static_assert(... sizeof(BatchItem) == 48 ...)
SIZEOF_ENC_BATCH_BLOCK = 24          # the same static_assert: sizeof(EncBatchBlock) == 24 (uploaded by tsqa_compress_batch_async alone)
SIZEOF_RANGE_ITEM = 24               # include/turbosqueeze_amd.h: tsqa_range_item {u32 block, lo, hi, pad; u64 out_at}
SIZEOF_BLOCK_GROUP = 16              # include/turbosqueeze_amd.h: tsqa_block_group {u32 block, first, count, hi}
# which entry points write the context's frame descriptors (c->frames) and so forget a sharded decode: tsq_runtime.hip,
# decompress_device_async_impl, decompress_batch_async_impl (both call forget_sharded) and tsqa_sharded_fetch_decode_async itself
WRITES_FRAMES = ("D", "S", "BD", "PD")
# ---- restated for the second catalogue
FIRST_JOIN_ITEMS = 256               # tsq_runtime.hip, tsqa_ctx::reserve_join: reserve_batch(n_items), then `doubled(256, n_items) + 1`
FIRST_CUT_RANGES = 256               # tsq_runtime.hip, tsqa_ctx::reserve_cut: `ranges = doubled(256, n_ranges) + 1, groups = doubled(256, n_ranges) / 256`
FIRST_GATHER_RANGES = 256            # tsq_runtime.hip, tsqa_ctx::reserve_gather: `const size_t want = doubled(256, n_ranges);` (the piece slots: cap_pieces itself)
FIRST_TABLE_BLOCKS = 256             # tsq_runtime.hip, tsqa_ctx::reserve_tables: `blocks = doubled(256, n_blocks), launches = doubled(16, n_launches)`
FIRST_TABLE_LAUNCHES = 16            # the same line; not exceeded here (thousands of blocks: test_gpu_scratch_growth.py grows it)
SPLIT_LEN = 4096                     # the block_len of every short-block link
# the new kinds that write c->frames and so call forget_sharded(): tsq_runtime.hip, decompress_device_async_impl (SD, the sized walk),
# stage_decompress_batch (DI, both forms), tsqa_decompress_batch_packed_dense_async (DD, where it has an output), tsqa_join_async (J),
# tsqa_index_create_packed_async (XP).  The compressing kinds (TC, PS, SC) write c->sizes and c->frame_at, the cut, the take and the
# gather (K, T, G) scratch of their own, and XS the new index's own descriptors; its read is an R.  (tsqa_ctx::reserve forgets too
# whenever the per-block descriptors grow, whoever asks: the test keeps the links behind S at S's block count or pre-grows them.)
WRITES_FRAMES2 = ("DI", "DD", "SD", "J", "XP")

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW, ERR_STALL = 0, 3, 4, 5, 6, 7

KINDS = ("C", "D", "E", "F", "S", "R", "I", "BC", "BD", "PC", "PD")
ENTRY = {"C": "tsqa_compress_device_async", "D": "tsqa_decompress_device_async", "E": "tsqa_encode_blocks_async",
         "F": "tsqa_decode_blocks_async", "S": "tsqa_sharded_fetch_decode_async", "R": "tsqa_decompress_ranges_async",
         "I": "tsqa_decompress_item_ranges_async", "BC": "tsqa_compress_batch_async", "BD": "tsqa_decompress_batch_async",
         "PC": "tsqa_compress_batch_packed_async", "PD": "tsqa_decompress_batch_packed_async"}
NEW_KINDS = ("DI", "DD", "TC", "PS", "SC", "SD", "XS", "XP", "J", "K", "T", "G")
ALL_KINDS = KINDS + NEW_KINDS
ENTRY.update({"DI": "tsqa_decompress_batch_items_async / tsqa_decompress_batch_packed_items_async",
              "DD": "tsqa_decompress_batch_packed_dense_async",
              "TC": "tsqa_compress_batch_packed_tables_async / tsqa_compress_batch_packed_tables_split_async",
              "PS": "tsqa_compress_batch_packed_split_async", "SC": "tsqa_compress_device_split_async",
              "SD": "tsqa_decompress_device_sized_async", "XS": "tsqa_index_create_sized_async + tsqa_decompress_ranges_async",
              "XP": "tsqa_index_create_packed_async", "J": "tsqa_join_async", "K": "tsqa_cut_async", "T": "tsqa_cut_items_async",
              "G": "tsqa_gather_async"})
SHAPES = ("small", "large")
DECODERS = ("D", "F", "S", "BD", "PD", "R", "I")
# the failing links: (kind, what is wrong) -> the status the call must leave in its own word
FAILURES = {("D", "twin"): ERR_STREAM, ("BD", "twin"): ERR_STREAM, ("PD", "twin"): ERR_STREAM, ("R", "twin"): ERR_STREAM,
            ("BC", "room"): ERR_OVERFLOW, ("PC", "room"): ERR_OVERFLOW, ("D", "count"): ERR_FORMAT}
# the second catalogue's: the statuses are the features' own restatements' (each link asserts that its expect() gives this one)
FAILURES2 = {("J", "room"): ERR_OVERFLOW, ("G", "room"): ERR_OVERFLOW, ("DD", "twin"): ERR_STREAM, ("TC", "place"): ERR_ARG,
             ("XS", "table"): ERR_FORMAT, ("K", "range"): ERR_ARG}
FAILURES.update(FAILURES2)
# which new kinds leave a packed arena with its two tables on the device, and which read one
PACKED_SOURCES = ("PC", "PS", "TC", "T")
PACKED_READERS = ("DD", "J", "XP")

LARGE_BLOCK_BYTES = 2 * BLOCK + 12_345       # three blocks
LARGE_ITEMS, LARGE_RANGES = 300, 400
SMALL_ITEMS, SMALL_RANGES = 3, 3
SMALL_SPLIT_BLOCKS, LARGE_SPLIT_BLOCKS = 3, 300      # SC, SD, XS, K: blocks of SPLIT_LEN bytes, the last one short
INDEXED_ITEMS = 40                                   # the items behind a batch index (as the I link's)
ALIGN = 16


def frames_of(blob):
    """(stream_at, stream_len, ext, out_len) of every frame of a container"""
    raw = bytes(blob)
    at, out = 16, []
    for _ in range(int.from_bytes(raw[4:8], "little")):
        word = int.from_bytes(raw[at:at + 3], "little")
        ln = word & 0x7FFFFF
        out.append((at + 3, ln, word >> 23, int.from_bytes(raw[at + 3:at + 6], "little")))
        at += 3 + ln
    return out


def refusal_code(stream):
    """what a one-block container around an invalid stream is refused with (tsq_format.h read_frame refuses a stream shorter than
    its size word and a block over 4 MiB: TSQA_ERR_FORMAT; the rest is the block decoder's to find: TSQA_ERR_STREAM)"""
    return ERR_FORMAT if len(stream) < 3 or int.from_bytes(stream[:3], "little") > BLOCK else ERR_STREAM


def twin_name(v):
    """the v-th choice among the catalogue's invalid twins that the library refuses with TSQA_ERR_STREAM, that are more than 100
    bytes long and claim 1 to 20 000 bytes (Gen.twin's selection; tests/shardgen.py places the same twins in a sharded container)"""
    names = sorted(n for n, (_, st) in streamgen.CATALOGUE.invalid.items()
                   if refusal_code(st) == ERR_STREAM and len(st) > 100 and 0 < int.from_bytes(st[:3], "little") <= 20_000)
    assert len(names) >= 8
    return names[(5 * v + 1) % len(names)]


class Link:
    """one call: `kind`, `shape`, `fail` (None, or what is wrong: a key of FAILURES), `want_status`, and the kind's own fields"""

    def __init__(self, kind, shape, fail=None, **fields):
        assert kind in ALL_KINDS and shape in SHAPES and (fail is None or (kind, fail) in FAILURES)
        self.kind, self.shape, self.fail = kind, shape, fail
        self.want_status = FAILURES[(kind, fail)] if fail else OK
        self.source = None                       # the earlier link of the chain whose device outputs this one consumes (PD: a PC; F: an E)
        self.__dict__.update(fields)

    def __repr__(self):
        return f"{self.kind}/{self.shape}" + (f"/{self.fail}" if self.fail else "")


class Gen:
    """the links of one oracle, inputs and oracle results made once and shared (a link object may be enqueued many times: it holds
    no destination)"""

    def __init__(self, oracle, synth):
        self.oracle, self.synth, self._cache = oracle, synth, {}

    # ---- inputs
    def _memo(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def container(self, data, ext):
        """the oracle's container of `data`, accepted by the oracle's own decoder and equal to the original"""
        blob = self.oracle.compress(data, ext, threads=4 if data.size > BLOCK else 1)
        assert self.oracle.decompress(blob, threads=4) == data.tobytes(), "the oracle does not give its own input back"
        return np.frombuffer(blob, dtype=np.uint8).copy()

    def block_data(self, shape, v, blocks=None):
        """small: one short block of 5 000 to 70 000 bytes (text, mix or structured); large: three blocks (text or mix).  `blocks`:
        the sharded links' other sizes (2: a full block and a short one; 5: four blocks and 12 345 bytes)"""
        def make():
            rng = np.random.default_rng([11, v, SHAPES.index(shape), blocks or 0])
            short = int(rng.integers(5_000, 70_001))
            n = {None: short if shape == "small" else LARGE_BLOCK_BYTES, 2: BLOCK + short, 5: 4 * BLOCK + 12_345}[blocks]
            if n <= 70_000 and v % 3 == 2:
                return np.ascontiguousarray(fuzzgen.structured(rng, n))
            return (self.synth.text if v % 2 == 0 else self.synth.mix)(n, seed=100 + 7 * v + n % 97)
        return self._memo(("block", shape, v, blocks), make)

    def block_container(self, shape, v, ext, blocks=None):
        return self._memo(("blob", shape, v, ext, blocks), lambda: self.container(self.block_data(shape, v, blocks), ext))

    def items(self, shape, v):
        """small: 3 items; large: 300 items; of 1 to 3 000 bytes each, every third one structured"""
        def make():
            rng = np.random.default_rng([13, v, SHAPES.index(shape)])
            out = []
            for k in range(SMALL_ITEMS if shape == "small" else LARGE_ITEMS):
                n = int(rng.integers(1, 3_001))
                out.append(np.ascontiguousarray(fuzzgen.structured(rng, n)) if k % 3 == 0
                           else (self.synth.text if k % 3 == 1 else self.synth.mix)(n, seed=1000 * v + k))
            return out
        return self._memo(("items", shape, v), make)

    def item_containers(self, shape, v, ext):
        return self._memo(("item_blobs", shape, v, ext), lambda: [self.container(d, ext) for d in self.items(shape, v)])

    def twin(self, v):
        """a one-block container around an invalid twin of the catalogue that the library refuses with TSQA_ERR_STREAM -> (name,
        container, the size its header claims); the oracle refuses it too"""
        def make():
            name = twin_name(v)
            ext, st = streamgen.CATALOGUE.invalid[name]
            blob = np.frombuffer(streamgen.bad_container(ext, st), dtype=np.uint8).copy()
            assert self.oracle.decompress(blob) is None, name
            return name, blob, int.from_bytes(st[:3], "little")
        return self._memo(("twin", v), make)

    @staticmethod
    def arena_of(rng, pieces):
        """the pieces in one arena behind non-zero filler gaps of 0..47 bytes -> (arena, offsets)"""
        at, offs = 0, []
        for p in pieces:
            at += int(rng.integers(0, 48))
            offs.append(at)
            at += p.size
        arena = rng.integers(1, 256, at + 64, dtype=np.uint8)
        for p, o in zip(pieces, offs):
            arena[o:o + p.size] = p
        return arena, offs

    # ---- the eleven kinds
    def link(self, kind, shape, v=0, fail=None):
        return self._memo(("link", kind, shape, v, fail), lambda: getattr(self, "_" + kind)(shape, v, fail))

    def _C(self, shape, v, fail):
        data, ext = self.block_data(shape, v), v & 1
        return Link("C", shape, data=data, ext=ext, want=self.block_container(shape, v, ext), blocks=-(-data.size // BLOCK))

    def _D(self, shape, v, fail):
        if fail == "twin":
            name, blob, claimed = self.twin(v)
            return Link("D", shape, fail, blob=blob, stated=1, out_len=claimed, plain=None, blocks=1, twin=name)
        data, ext = self.block_data(shape, v + 1), (v + 1) & 1
        blob = self.block_container(shape, v + 1, ext)
        nb = -(-data.size // BLOCK)
        assert int.from_bytes(bytes(blob[4:8]), "little") == nb
        stated = nb + 1 if fail == "count" else nb
        return Link("D", shape, fail, blob=blob, stated=stated, out_len=data.size, plain=data, blocks=stated, header_blocks=nb)

    def _E(self, shape, v, fail):
        data, ext = self.block_data(shape, v), (v + 1) & 1
        nb = -(-data.size // BLOCK)
        last = data.size - (nb - 1) * BLOCK
        packed = np.zeros((nb - 1) * STRIDE + last + HALO, dtype=np.uint8)
        for b in range(nb):
            piece = data[b * BLOCK:(b + 1) * BLOCK + HALO]               # the block and the first bytes of the next (zeros behind the last)
            packed[b * STRIDE:b * STRIDE + piece.size] = piece
        blob = self.block_container(shape, v, ext)
        fr = frames_of(blob)
        return Link("E", shape, data=data, packed=packed, n_blocks=nb, last_len=last, ext=ext, blocks=nb,
                    want_streams=[bytes(blob[a:a + ln]) for a, ln, _, _ in fr], want_sizes=[ln for _, ln, _, _ in fr])

    def _F(self, shape, v, fail):
        data, ext = self.block_data(shape, v + 1), v & 1
        blob = self.block_container(shape, v + 1, ext)
        frames = [(a, b * BLOCK, ln, e, ol) for b, (a, ln, e, ol) in enumerate(frames_of(blob))]
        return Link("F", shape, streams=blob, frames=frames, plain=data, out_len=data.size, blocks=len(frames))

    def F_of(self, e):
        """the decode of what the E link `e` leaves in its slots, through a frame table of the oracle's sizes"""
        frames = [(b * SLOT, b * BLOCK, ln, e.ext, min(BLOCK, e.data.size - b * BLOCK)) for b, ln in enumerate(e.want_sizes)]
        f = Link("F", e.shape, streams=None, frames=frames, plain=e.data, out_len=e.data.size, blocks=len(frames))
        f.source = e
        return f

    def _S(self, shape, v, fail):
        """world 1: the block work's own sizes; world 2 / rank 1 (odd v): a full block and a short one (small: the rank owns the
        short block), four blocks and 12 345 bytes (large: it owns two)"""
        world, rank = (2, 1) if v & 1 else (1, 0)
        blocks = None if world == 1 else (2 if shape == "small" else 5)
        data, ext = self.block_data(shape, v, blocks), (v >> 1) & 1
        blob = self.block_container(shape, v, ext, blocks)
        nb = -(-data.size // BLOCK)
        owned = list(range(rank, nb, world))
        pieces = [(k * BLOCK, data[b * BLOCK:(b + 1) * BLOCK]) for k, b in enumerate(owned)]
        return Link("S", shape, blob=blob, world=world, rank=rank, n_local=len(owned), pieces=pieces, total=data.size,
                    out_len=pieces[-1][0] + pieces[-1][1].size, blocks=len(owned))

    def _ranges(self, rng, total, count):
        out = []
        for k in range(count):
            ln = int(rng.integers(1, min(total, 100) + 1))
            out.append((int(rng.integers(0, total - ln + 1)), ln))
        if total > BLOCK:                                               # one of them across a block edge
            out[0] = (BLOCK - 40, 100)
        return out

    def _R(self, shape, v, fail):
        if fail == "twin":
            name, blob, claimed = self.twin(v + 1)
            return Link("R", shape, fail, blob=blob, ranges=[(0, claimed)], plain=None, total=claimed, n_blocks=1, twin=name,
                        upload=SIZEOF_RANGE_ITEM)
        data, ext = self.block_data(shape, v), v & 1
        blob = self.block_container(shape, v, ext)
        count = SMALL_RANGES if shape == "small" else LARGE_RANGES
        ranges = self._ranges(np.random.default_rng([17, v, count]), data.size, count)
        return Link("R", shape, blob=blob, ranges=ranges, plain=data, total=data.size, n_blocks=-(-data.size // BLOCK),
                    upload=count * SIZEOF_RANGE_ITEM)                   # (at least: a range across a block edge gives two items)

    def _I(self, shape, v, fail):
        datas, ext = self.items("small" if shape == "small" else "large", v)[:40], v & 1
        blobs = self.item_containers(shape, v, ext)[:40]
        rng = np.random.default_rng([19, v, SHAPES.index(shape)])
        arena, offs = self.arena_of(rng, blobs)
        count = SMALL_RANGES if shape == "small" else LARGE_RANGES
        ranges = []
        for k in range(count):
            i = k % len(datas)
            ln = int(rng.integers(1, min(datas[i].size, 64) + 1))
            ranges.append((i, int(rng.integers(0, datas[i].size - ln + 1)), ln))
        touched = len({i for i, _, _ in ranges})                        # one block per item: one group per touched item
        groups_at = (count * SIZEOF_RANGE_ITEM + 15) & ~15
        return Link("I", shape, arena=arena, spans=[(o, b.size) for o, b in zip(offs, blobs)], plains=datas, ranges=ranges,
                    upload=groups_at + touched * SIZEOF_BLOCK_GROUP, n_groups=touched)

    def _BC(self, shape, v, fail):
        datas, ext = self.items(shape, v), v & 1
        want = self.item_containers(shape, v, ext)
        arena, offs = self.arena_of(np.random.default_rng([23, v, SHAPES.index(shape)]), datas)
        rooms = [w.size for w in want]                                  # exactly the oracle's container: the range IS the destination
        tight = None
        if fail == "room":
            tight = max(range(len(want)), key=lambda i: want[i].size)
            rooms[tight] -= 1
            assert rooms[tight] >= 16 + 6                               # (tsqa_plan_batch accepts it: the overflow is the device's to find)
        n = len(datas)
        return Link("BC", shape, fail, arena=arena, spans=[(o, d.size) for o, d in zip(offs, datas)], ext=ext, want=want, rooms=rooms,
                    tight=tight, items=n, blocks=n, upload=n * SIZEOF_BATCH_ITEM + n * SIZEOF_ENC_BATCH_BLOCK)

    def _BD(self, shape, v, fail):
        datas, ext = self.items(shape, v + 1), (v + 1) & 1
        blobs = list(self.item_containers(shape, v + 1, ext))
        lengths, plains, bad = [d.size for d in datas], list(datas), None
        if fail == "twin":
            name, twin, claimed = self.twin(v + 2)
            bad = len(blobs) // 2
            blobs[bad], lengths[bad], plains[bad] = twin, claimed, None
        arena, offs = self.arena_of(np.random.default_rng([29, v, SHAPES.index(shape)]), blobs)
        n = len(blobs)
        return Link("BD", shape, fail, arena=arena, spans=[(o, b.size) for o, b in zip(offs, blobs)], lengths=lengths, plains=plains,
                    bad=bad, items=n, blocks=n, upload=n * SIZEOF_BATCH_ITEM)

    def _PC(self, shape, v, fail):
        datas, ext = self.items(shape, v + 1), v & 1
        want = self.item_containers(shape, v + 1, ext)
        arena, offs = self.arena_of(np.random.default_rng([31, v, SHAPES.index(shape)]), datas)
        sizes = [w.size for w in want]
        offsets = plan_packed(sizes, ALIGN)
        n = len(datas)
        out_size = offsets[n] - 1 if fail == "room" else offsets[n]     # one byte short of the last container / exactly the bytes used
        return Link("PC", shape, fail, arena=arena, spans=[(o, d.size) for o, d in zip(offs, datas)], datas=datas, ext=ext, want=want,
                    sizes=sizes, offsets=offsets, out_size=out_size, tight=n - 1 if fail else None, items=n, blocks=n,
                    upload=n * SIZEOF_BATCH_ITEM + (n + 1) * 8 + 4)     # the item table, first_block, the block count: no descriptors

    def _PD(self, shape, v, fail):
        datas, ext = self.items(shape, v), (v + 1) & 1
        blobs = list(self.item_containers(shape, v, ext))
        lengths, plains, bad = [d.size for d in datas], list(datas), None
        if fail == "twin":
            name, twin, claimed = self.twin(v + 3)
            bad = len(blobs) // 2
            blobs[bad], lengths[bad], plains[bad] = twin, claimed, None
        sizes = [b.size for b in blobs]
        offsets = plan_packed(sizes, ALIGN)
        arena = np.random.default_rng([37, v]).integers(1, 256, offsets[-1] + 32, dtype=np.uint8)
        for b, o in zip(blobs, offsets):
            arena[o:o + b.size] = b
        n = len(blobs)
        return Link("PD", shape, fail, arena=arena, arena_size=offsets[-1], offsets=offsets, sizes=sizes, lengths=lengths, plains=plains,
                    bad=bad, items=n, blocks=n, upload=n * SIZEOF_BATCH_ITEM)

    def PD_of(self, pc):
        """the decode of what the PC link `pc` leaves on the device: its arena and its two tables"""
        n = len(pc.datas)
        pd = Link("PD", pc.shape, arena=None, arena_size=pc.out_size, offsets=pc.offsets, sizes=pc.sizes, lengths=[d.size for d in pc.datas],
                  plains=list(pc.datas), bad=None, items=n, blocks=n, upload=n * SIZEOF_BATCH_ITEM)
        pd.source = pc
        return pd

    # ---- the second catalogue: inputs
    def split_data(self, shape, v):
        """small: 3 blocks of SPLIT_LEN bytes, large: 300, the last one 1 to 4 095 bytes long (text or mix)"""
        def make():
            rng = np.random.default_rng([43, v, SHAPES.index(shape)])
            nb = SMALL_SPLIT_BLOCKS if shape == "small" else LARGE_SPLIT_BLOCKS
            n = (nb - 1) * SPLIT_LEN + int(rng.integers(1, SPLIT_LEN))
            return (self.synth.text if v % 2 == 0 else self.synth.mix)(n, seed=300 + 11 * v + nb)
        return self._memo(("split", shape, v), make)

    def split_container(self, shape, v, ext):
        """splitgen.expected_split of split_data: what the split compress owes, made of the oracle's block streams -> (container as
        a uint8 array, the table of stream sizes); the oracle's decoder gives the input back"""
        def make():
            data = self.split_data(shape, v)
            blob, sizes = sg.expected_split(self.oracle, data, SPLIT_LEN, ext)
            assert self.oracle.decompress(blob, threads=4) == data.tobytes(), "the oracle does not give its own input back"
            return np.frombuffer(blob, dtype=np.uint8).copy(), sizes
        return self._memo(("split_blob", shape, v, ext), make)

    def indexed_batch(self, shape, v, ext):
        """up to 40 of the items' containers in an arena behind filler gaps, as the I link's -> (arena, spans, datas)"""
        def make():
            datas = self.items(shape, v)[:INDEXED_ITEMS]
            blobs = self.item_containers(shape, v, ext)[:INDEXED_ITEMS]
            arena, offs = self.arena_of(np.random.default_rng([47, v, SHAPES.index(shape)]), blobs)
            return arena, [(o, b.size) for o, b in zip(offs, blobs)], datas
        return self._memo(("indexed", shape, v, ext), make)

    @staticmethod
    def packed_output(src):
        """what a passing link of PACKED_SOURCES leaves on the device, from its expectation -> (containers as bytes, their data as
        bytes, their block counts, the bytes of the arena that the tables speak of)"""
        assert src.kind in PACKED_SOURCES and not src.fail
        if src.kind == "PC":
            return [w.tobytes() for w in src.want], [d.tobytes() for d in src.datas], [1] * len(src.want), src.out_size
        if src.kind == "T":
            e = src.e
            return ([src.case.container(e, k) for k in range(src.case.n)], [bytes(src.case.data(k)) for k in range(src.case.n)],
                    [s[2] for s in e["spans"]], e["need"])
        return list(src.containers), list(src.plains), list(src.item_blocks), src.out_size

    # ---- the twelve kinds of the second catalogue
    def _DI(self, shape, v, fail):
        """v even: tsqa_decompress_batch_items_async (the containers behind filler gaps, their places from the host); v odd:
        tsqa_decompress_batch_packed_items_async (a packed arena, the places in device tables)"""
        datas, ext = self.items(shape, v + 1), v & 1
        blobs = self.item_containers(shape, v + 1, ext)
        n = len(blobs)
        packed = bool(v & 1)
        if packed:
            sizes = [b.size for b in blobs]
            offsets = plan_packed(sizes, ALIGN)
            arena = np.random.default_rng([53, v]).integers(1, 256, offsets[-1] + 32, dtype=np.uint8)
            for b, o in zip(blobs, offsets):
                arena[o:o + b.size] = b
            spans, arena_size = list(zip(offsets, sizes)), offsets[-1]
        else:
            arena, offs = self.arena_of(np.random.default_rng([53, v, SHAPES.index(shape)]), blobs)
            spans, arena_size = [(o, b.size) for o, b in zip(offs, blobs)], arena.size
        return Link("DI", shape, packed=packed, arena=arena, arena_size=arena_size, spans=spans, lengths=[d.size for d in datas],
                    plains=list(datas), items=n, blocks=n, upload=n * SIZEOF_BATCH_ITEM)

    def _dense(self, kind, shape, name, blobs, plains, faults, source=None, arena_size=None):
        """a dense decompress of the containers `blobs` (bytes; plains[i] None and faults[i] the code of one a decoder refuses) in
        densegen's packed arena, with exactly the room and the blocks needed"""
        batch = dg.Batch(name, [dg.Item(f"{name}_{i}", b, p, f) for i, (b, p, f) in enumerate(zip(blobs, plains, faults))], ALIGN)
        offsets, first, status, out_sizes = batch.expect(batch.need_bytes, batch.need_blocks)
        return dict(batch=batch, arena=batch.arena if source is None else None, arena_size=batch.arena.size if arena_size is None else arena_size,
                    offsets=batch.offsets, sizes=batch.sizes, out_offsets=offsets, first_block=first, item_status=status, out_sizes=out_sizes,
                    plains=plains, out_size=batch.need_bytes, cap_blocks=batch.need_blocks, items=len(blobs), blocks=batch.need_blocks)

    def _DD(self, shape, v, fail):
        datas, ext = self.items(shape, v), (v + 1) & 1
        blobs = [b.tobytes() for b in self.item_containers(shape, v, ext)]
        plains, faults = [d.tobytes() for d in datas], [OK] * len(datas)
        if fail == "twin":
            name, twin, claimed = self.twin(v + 1)
            bad = len(blobs) // 2
            blobs[bad], plains[bad], faults[bad] = twin.tobytes(), None, ERR_STREAM
        f = self._dense("DD", shape, f"dd_{shape}_{v}_{fail}", blobs, plains, faults)
        x = Link("DD", shape, fail, **f)
        assert max(x.item_status) == x.want_status and (not fail or [s != OK for s in x.item_status] == [i == bad for i in range(x.items)])
        return x

    def DD_of(self, src):
        """the dense decompress of the arena and the tables that the link `src` (of PACKED_SOURCES) leaves on the device"""
        blobs, plains, _, arena_size = self.packed_output(src)
        f = self._dense("DD", src.shape, f"dd_of_{src!r}", blobs, plains, [OK] * len(blobs), source=src, arena_size=arena_size)
        x = Link("DD", src.shape, **f)
        x.source = src
        return x

    def _TC(self, shape, v, fail):
        """v even: tsqa_compress_batch_packed_tables_async; v odd: ..._tables_split_async at SPLIT_LEN (the items are at most 3 000
        bytes: one block each at either block length, 300 blocks in the large shape).  fail 'place': the middle item's place ends
        one byte past the input (tablegen.Refused('offset_one_past'))"""
        datas, ext = self.items(shape, v + 1), v & 1
        n, split = len(datas), bool(v & 1)
        bad = n // 2 if fail == "place" else None
        if split:
            specs = [tg.Refused("offset_one_past") if i == bad else d for i, d in enumerate(datas)]
            b = bsg.Batch(f"tc_{shape}_{v}_{fail}", specs, SPLIT_LEN, ALIGN, slack=128)
            e = b.expect(self.oracle, ext)
            made = b.made(self.oracle, ext)
            containers, block_sizes = [m[0] if m else None for m in made], e["block_sizes"]
        else:
            specs = [tg.Refused("offset_one_past") if i == bad else d.tobytes() for i, d in enumerate(datas)]
            b = tg.Batch(f"tc_{shape}_{v}_{fail}", specs, ALIGN, slack=bytes(range(1, 129)))
            e = b.expect(ext, b.need_blocks, 1 << 40)
            containers, block_sizes = b.containers(ext), None
        out_size = e["offsets"][-1]
        assert all(w == (len(c) if c else 0) for w, c in zip(e["writes"], containers)), "with exactly the room needed every container is whole"
        x = Link("TC", shape, fail, split=split, data=np.array(b.data), in_offsets=b.in_offsets, in_sizes=b.in_sizes, ext=ext, cap_blocks=b.need_blocks,
                 out_size=out_size, offsets=e["offsets"], sizes=e["sizes"], first_block=e["first_block"], bound=e["bound"],
                 item_status=e["status"], block_sizes=block_sizes, containers=containers, bad=bad,
                 plains=[None if i == bad else d.tobytes() for i, d in enumerate(datas)], item_blocks=list(b.blocks), items=n,
                 blocks=b.need_blocks, table_blocks=b.need_blocks)
        assert max(x.item_status) == x.want_status and [s != OK for s in x.item_status] == [i == bad for i in range(n)]
        return x

    def _PS(self, shape, v, fail):
        """small: 3 items of 1, 2 and 3 blocks of SPLIT_LEN; large: 300 items, every seventh of 2 or 3 blocks: more than 256 blocks"""
        def make_specs():
            rng = np.random.default_rng([59, v, SHAPES.index(shape)])
            if shape == "small":
                sizes = [int(rng.integers(1, SPLIT_LEN)) + k * SPLIT_LEN for k in rng.permutation(3)]
            else:
                sizes = [int(rng.integers(1, 3_001)) + (int(rng.integers(1, 3)) * SPLIT_LEN if k % 7 == 3 else 0) for k in range(LARGE_ITEMS)]
            return [(self.synth.text if k % 2 else self.synth.mix)(n, seed=2000 * v + k) for k, n in enumerate(sizes)]
        specs, ext = self._memo(("ps_specs", shape, v), make_specs), v & 1
        b = bsg.Batch(f"ps_{shape}_{v}", specs, SPLIT_LEN, ALIGN)
        e = b.expect(self.oracle, ext, per_item=False)
        n = len(specs)
        assert e["word"] == OK and e["first_block"][-1] == b.need_blocks
        return Link("PS", shape, data=np.array(b.data), spans=list(zip(b.in_offsets, b.in_sizes)), ext=ext, offsets=e["offsets"], sizes=e["sizes"],
                    out_size=e["offsets"][-1], first_block=e["first_block"], block_sizes=e["block_sizes"],
                    containers=[m[0] for m in b.made(self.oracle, ext)], plains=[d.tobytes() for d in specs], item_blocks=list(b.blocks),
                    items=n, blocks=b.need_blocks, table_blocks=b.need_blocks,
                    upload=n * SIZEOF_BATCH_ITEM + (n + 1) * 8 + 4)     # the item table, first_block, the block count: no descriptors

    def _SC(self, shape, v, fail):
        data, ext = self.split_data(shape, v), v & 1
        want, sizes = self.split_container(shape, v, ext)
        return Link("SC", shape, data=data, ext=ext, want=want, want_sizes=sizes, blocks=len(sizes), table_blocks=len(sizes))

    def _SD(self, shape, v, fail):
        data, ext = self.split_data(shape, v + 1), (v + 1) & 1
        blob, sizes = self.split_container(shape, v + 1, ext)
        return Link("SD", shape, blob=blob, n=blob.size, table=sizes, plain=data, out_len=data.size, blocks=len(sizes))

    def SD_of(self, sc):
        """the sized decode of the container and the size table that the SC link `sc` leaves on the device"""
        sd = Link("SD", sc.shape, blob=None, n=sc.want.size, table=None, plain=sc.data, out_len=sc.data.size, blocks=sc.blocks)
        sd.source = sc
        return sd

    def _XS(self, shape, v, fail):
        """the sized index of a split container, then ONE tsqa_decompress_ranges_async of 3 or 400 ranges through it.  fail 'table':
        seekgen's false table 'entry_256_plus_1' -- which takes a container of more than 257 blocks, so the failing link has the
        large container and three ranges"""
        big = shape == "large" or fail == "table"
        data, ext = self.split_data("large" if big else "small", v + 2), v & 1
        blob, sizes = self.split_container("large" if big else "small", v + 2, ext)
        table = list(sizes)
        if fail == "table":
            name, c, n, table, why = next(t for t in kg.false_tables(blob.tobytes(), sizes) if t[0] == cutgen.REFUSED_TABLE)
            assert c == blob.tobytes() and n == blob.size and table != sizes
        assert bool(kg.index_refuses(blob.tobytes(), blob.size, table, data.size, SPLIT_LEN)) == bool(fail)
        count = SMALL_RANGES if shape == "small" else LARGE_RANGES
        ranges = self._ranges(np.random.default_rng([61, v, count]), data.size, count)
        ranges[0] = (SPLIT_LEN - 40, 100)                               # one of them across a block edge
        return Link("XS", shape, fail, blob=blob, table=table, n_total=data.size, plain=None if fail else data, ranges=ranges,
                    n_blocks=len(sizes), upload=count * SIZEOF_RANGE_ITEM)   # (at least: a range across a block edge gives two items)

    def _packed_index(self, shape, name, blobs, datas, sized_tables=None, source=None):
        block_len, first, table = sized_tables if sized_tables else (None, None, None)
        case = pg.Case(name, blobs, datas, None, None, block_len, first, table)
        e = case.expect()
        assert e["status"] == OK and e["words"][0] == e["words"][2] == e["cap_blocks"]
        return dict(case=case, e=e, arena=case.arena if source is None else None, arena_size=case.arena.size, offsets=case.offsets,
                    sizes=case.sizes, cap_blocks=e["cap_blocks"], sized=bool(sized_tables), items=case.n, blocks=e["cap_blocks"])

    def _XP(self, shape, v, fail):
        """v even: the plain form over the oracle's containers; v odd: the sized form over split containers of the same items (one
        block each at SPLIT_LEN) with their true tables"""
        datas, ext = self.items(shape, v), (v >> 1) & 1
        if v & 1:
            made = [sg.expected_split(self.oracle, d, SPLIT_LEN, ext) for d in datas]
            first, table = [0], []
            for _, sizes in made:
                table += sizes
                first.append(len(table))
            f = self._packed_index(shape, f"xp_{shape}_{v}", [m[0] for m in made], [d.tobytes() for d in datas], (SPLIT_LEN, first, table))
        else:
            f = self._packed_index(shape, f"xp_{shape}_{v}", [b.tobytes() for b in self.item_containers(shape, v, ext)], [d.tobytes() for d in datas])
        return Link("XP", shape, **f)

    def XP_of(self, src):
        """the plain index of the arena and the tables that the link `src` (of PACKED_SOURCES) leaves on the device"""
        blobs, plains, _, arena_size = self.packed_output(src)
        f = self._packed_index(src.shape, f"xp_of_{src!r}", blobs, plains, source=src)
        f["arena_size"] = arena_size
        x = Link("XP", src.shape, **f)
        x.source = src
        return x

    def _J(self, shape, v, fail):
        """the oracle's containers in joingen's ragged arena; fail 'room': an output one byte short"""
        datas, ext = self.items(shape, v), v & 1
        blobs = self.item_containers(shape, v, ext)
        case = jg.Case(f"j_{shape}_{v}", [jg.Item(f"item_{k}", b.tobytes(), d.tobytes()) for k, (b, d) in enumerate(zip(blobs, datas))], ALIGN, ragged=True)
        cap = case.need_blocks
        size = case.expect(cap, 1 << 62)["out_size"]
        out_cap = size - 1 if fail == "room" else size
        e = case.expect(cap, out_cap)
        assert e["status"] == (ERR_OVERFLOW if fail else OK) and e["out_size"] == size and (e["container"] is None) == bool(fail)
        n = len(blobs)
        return Link("J", shape, fail, arena=case.arena, arena_size=case.arena.size, offsets=case.offsets, sizes=case.sizes, cap_blocks=cap,
                    out_cap=out_cap, out_size=size, first_block=e["first_block"], item_status=e["item_status"], container=e["container"],
                    block_sizes=e["block_sizes"], plain=case.data(), items=n, blocks=cap)

    def J_of(self, src):
        """the join of the arena and the tables that the link `src` (of PACKED_SOURCES) leaves on the device"""
        blobs, plains, blocks, arena_size = self.packed_output(src)
        container, sizes = jg.joined(blobs)
        first = [sum(blocks[:i]) for i in range(len(blocks) + 1)]
        j = Link("J", src.shape, arena=None, arena_size=arena_size, offsets=None, sizes=None, cap_blocks=first[-1], out_cap=len(container),
                 out_size=len(container), first_block=first, item_status=[OK] * len(blobs), container=container, block_sizes=sizes,
                 plain=b"".join(plains), items=len(blobs), blocks=first[-1])
        j.source = src
        return j

    def _K(self, shape, v, fail):
        """3 or 400 block ranges of 1 to 3 blocks out of a split container of 3 or 300 blocks, through tsqa_index_create.  fail
        'range': the middle range's first is n_blocks"""
        data, ext = self.split_data(shape, v + 3), v & 1
        blob, sizes = self.split_container(shape, v + 3, ext)
        source = self._memo(("cut_source", shape, v), lambda: cutgen.Source(f"k_{shape}_{v}", blob.tobytes(), data.tobytes(), SPLIT_LEN, sizes))
        nb, count = source.n_blocks, SMALL_RANGES if shape == "small" else LARGE_RANGES
        rng = np.random.default_rng([67, v, count])
        ranges = []
        for _ in range(count):
            f = int(rng.integers(0, nb))
            ranges.append((f, int(rng.integers(1, min(3, nb - f) + 1))))
        if fail == "range":
            ranges[count // 2] = (nb, 1)
        case = cutgen.Case(f"k_{shape}_{v}_{fail}", source, ranges, ALIGN)
        e = case.expect(case.need)
        x = Link("K", shape, fail, blob=blob, case=case, e=e, ranges=ranges, out_size=case.need, n_blocks=nb, n_ranges=count)
        assert e["status"] == x.want_status and [s != OK for s in e["item_status"]] == [bool(fail) and k == count // 2 for k in range(count)]
        return x

    def _take(self, shape, name, batch, items, ranges, cap_blocks=None, source=None):
        case = tk.Case(name, batch, items, ranges, ALIGN, cap_blocks)
        e = case.expect(case.need)
        assert e["status"] == OK
        x = Link("T", shape, case=case, e=e, take_items=list(items), ranges=ranges, out_size=case.need, n_ranges=len(items),
                 arena=batch.arena if source is None else None, spans=list(zip(batch.offsets, batch.sizes)))
        x.source = source
        return x

    def _T(self, shape, v, fail):
        """3 or 400 ranges through a batch index (tsqa_index_create_batch) of up to 40 items: whole items (v even: d_first and
        d_count NULL) or the one block of each (v odd)"""
        arena, spans, datas = self.indexed_batch(shape, v, v & 1)
        batch = self._memo(("take_batch", shape, v), lambda: tk.Batch(f"t_{shape}_{v}", arena, [o for o, _ in spans], [n for _, n in spans],
                                                                      [d.tobytes() for d in datas]))
        count = SMALL_RANGES if shape == "small" else LARGE_RANGES
        rng = np.random.default_rng([71, v, count])
        items = [int(i) for i in rng.integers(0, len(spans), count)]
        return self._take(shape, f"t_{shape}_{v}", batch, items, [(0, 1)] * count if v & 1 else None)

    def T_of(self, xp, v=0):
        """whole items out of the index that the XP link `xp` has just made and nobody has fetched"""
        c = xp.case
        batch = tk.Batch(f"t_of_{xp!r}", c.arena, c.offsets, c.sizes, c.datas)
        count = SMALL_RANGES if xp.shape == "small" else LARGE_RANGES
        items = [int(i) for i in np.random.default_rng([73, v, count]).integers(0, c.n, count)]
        return self._take(xp.shape, f"t_of_{xp!r}", batch, items, None, cap_blocks=xp.cap_blocks, source=xp)

    def _gather(self, shape, fail, name, index, items, offsets, lengths, through, source=None):
        case = gg.Case(name, index, offsets, lengths, items, ALIGN)
        free = case.expect()
        cap_pieces, out_cap = max(free["need_pieces"], 1), free["need"]
        if fail == "room":                                              # out_cap ends inside a middle range
            mid = next(k for k in range(case.n // 2, case.n) if lengths[k] >= 2)
            out_cap = free["out_offsets"][mid] + 1
        e = case.expect(out_cap, cap_pieces)
        x = Link("G", shape, fail, case=case, e=e, g_items=items, offsets=list(offsets), lengths=list(lengths), out_cap=out_cap,
                 cap_pieces=cap_pieces, n_ranges=case.n, through=through, room=free["need"])
        x.source = source
        assert e["status"] == x.want_status and e["need"] == free["need"] and e["need_pieces"] == free["need_pieces"]
        if fail:
            assert e["range_status"][:mid] == [OK] * mid and set(e["range_status"][mid:]) == {ERR_OVERFLOW} and mid > 0
        return x

    def _G(self, shape, v, fail):
        """v even: offsets into the data of the R link's container, through its index (large: three blocks, range 0 across a block
        edge); v odd: ranges by item through the I link's batch index.  fail 'room': out_cap ends one byte into a middle range"""
        count = SMALL_RANGES if shape == "small" else LARGE_RANGES
        if v & 1:
            through = self.link("I", shape, v)
            cat = b"".join(p.tobytes() for p in through.plains)
            starts = np.concatenate([[0], np.cumsum([p.size for p in through.plains])]).tolist()
            index = gg.Index(f"g_{shape}_{v}", "batch", None, cat, starts, item_first=list(range(len(through.plains) + 1)), spans=through.spans)
            rng = np.random.default_rng([79, v, count])
            items = [k % len(through.plains) for k in range(count)]
            lengths = [int(rng.integers(1, min(through.plains[i].size, 64) + 1)) for i in items]
            offsets = [int(rng.integers(0, through.plains[i].size - ln + 1)) for i, ln in zip(items, lengths)]
        else:
            through = self.link("R", shape, v)
            nb = through.n_blocks
            index = gg.Index(f"g_{shape}_{v}", "plain", None, through.plain.tobytes(), [min(b * BLOCK, through.total) for b in range(nb)] + [through.total])
            items = None
            ranges = self._ranges(np.random.default_rng([83, v, count]), through.total, count)
            offsets, lengths = [o for o, _ in ranges], [ln for _, ln in ranges]
        return self._gather(shape, fail, f"g_{shape}_{v}_{fail}", index, items, offsets, lengths, through)

    def G_of(self, xp, v=0):
        """ranges by item through the index that the XP link `xp` has just made and nobody has fetched"""
        c, e = xp.case, xp.e
        starts = np.concatenate([[0], np.cumsum(e["out_len"])]).tolist()
        index = gg.Index(f"g_of_{xp!r}", "batch", None, b"".join(c.datas), starts, item_first=e["item_first"])
        count = SMALL_RANGES if xp.shape == "small" else LARGE_RANGES
        rng = np.random.default_rng([89, v, count])
        items = [int(i) for i in rng.integers(0, c.n, count)]
        lengths = [int(rng.integers(1, min(len(c.datas[i]), 64) + 1)) for i in items]
        offsets = [int(rng.integers(0, len(c.datas[i]) - ln + 1)) for i, ln in zip(items, lengths)]
        return self._gather(xp.shape, None, f"g_of_{xp!r}", index, items, offsets, lengths, None, source=xp)

    # ---- chains
    def pairs(self):
        """all 121 ordered pairs of kinds, each as (small, large) and (large, small): (first link, second link)"""
        out = []
        for i, a in enumerate(KINDS):
            for j, b in enumerate(KINDS):
                for sa, sb in (("small", "large"), ("large", "small")):
                    out.append((self.link(a, sa, (i + j) % 2), self.link(b, sb, (i + j + 1) % 2 + 2)))
        return out

    def default_decoder_pairs(self):
        """the ordered pairs with a decoding kind in first or second place, both large"""
        return [(self.link(a, "large", (i + j) % 2), self.link(b, "large", (i + j + 1) % 2 + 2))
                for i, a in enumerate(KINDS) for j, b in enumerate(KINDS) if a in DECODERS or b in DECODERS]

    TRIPLES = (("R", "I", "R"), ("I", "R", "I"), ("BC", "BD", "PC"), ("PD", "BC", "BD"), ("BD", "PC", "PD"))
    TRIPLE_SHAPES = (("small", "small", "large"), ("large", "small", "small"))

    def triples(self):
        """the third call takes the first's upload slot; a PD behind a passing PC of its own shape reads that PC's tables"""
        out = []
        for kinds in self.TRIPLES:
            for shapes in self.TRIPLE_SHAPES:
                chain = []
                for k, (kind, shape) in enumerate(zip(kinds, shapes)):
                    pcs = [x for x in chain if x.kind == "PC" and x.shape == shape]
                    chain.append(self.PD_of(pcs[-1]) if kind == "PD" and pcs else self.link(kind, shape, k))
                out.append(chain)
        return out

    WALK_FAILURES = ((("D", "count"), ("BD", "twin"), ("PC", "room"), ("R", "twin")),
                     (("D", "twin"), ("PD", "twin"), ("BC", "room"), ("R", "twin")))

    @staticmethod
    def _no_reader(kinds, k):
        """no PD between position k and the next PC"""
        later = kinds[k + 1:]
        return "PD" not in later[:later.index("PC") if "PC" in later else len(later)]

    def walk(self, seed, length=40):
        """`length` links drawn over all kinds and both shapes.  Every PD reads the device tables of the nearest earlier PC (a PD
        drawn before any PC becomes a PC; only a failing PD brings tables of its own), every F the slots of the nearest earlier E
        (likewise).  Four positions hold the failing links of WALK_FAILURES[seed]: each replaces a drawn link of its kind; a
        failing PC is the last PC before the end or before the next PC has been drawn with no PD between them."""
        rng = np.random.default_rng([41, seed])
        kinds = [KINDS[int(k)] for k in rng.integers(0, len(KINDS), length)]
        shapes = [SHAPES[int(s)] for s in rng.integers(0, 2, length)]
        for first, then in (("PC", "PD"), ("E", "F")):
            for k, kind in enumerate(kinds):
                if kind == then and first not in kinds[:k]:
                    kinds[k] = first
        failing = {}
        for kind, what in self.WALK_FAILURES[seed]:
            spots = [k for k, x in enumerate(kinds) if x == kind and k not in failing]
            if kind == "PC":                                            # no PD may read a cut arena
                spots = [k for k in spots if self._no_reader(kinds, k)]
            if not spots:                                               # the draw has no such link left: one becomes that kind
                free = [k for k in range(length) if k not in failing and kinds[k] in ("C", "R", "I", "BC", "BD", "D", "S")]
                if kind == "PC":
                    free = [k for k in free if self._no_reader(kinds, k)]
                k = free[int(rng.integers(0, len(free)))]
                kinds[k] = kind
                spots = [k]
            failing[spots[int(rng.integers(0, len(spots)))]] = what
        chain = []
        for k, (kind, shape) in enumerate(zip(kinds, shapes)):
            if k in failing:
                chain.append(self.link(kind, "small", k % 4, failing[k]))
            elif kind == "PD":
                chain.append(self.PD_of([x for x in chain if x.kind == "PC"][-1]))
            elif kind == "F":
                chain.append(self.F_of([x for x in chain if x.kind == "E"][-1]))
            else:
                chain.append(self.link(kind, shape, k % 4))
        assert sum(1 for x in chain if x.fail) == 4
        assert all(x.source is None or not x.source.fail for x in chain)
        return chain

    # ---- chains of the second catalogue
    def pairs2(self):
        """every ordered pair of ALL_KINDS with at least one new kind, 23^2 - 11^2 = 408 of them, each as (small, large) and (large,
        small), the variants drawn as pairs() draws them: (first link, second link).  Every link brings its own inputs."""
        out = []
        for i, a in enumerate(ALL_KINDS):
            for j, b in enumerate(ALL_KINDS):
                if a in KINDS and b in KINDS:
                    continue
                for sa, sb in (("small", "large"), ("large", "small")):
                    out.append((self.link(a, sa, (i + j) % 2), self.link(b, sb, (i + j + 1) % 2 + 2)))
        return out

    def default_decoder_pairs2(self):
        """of the new kinds only SD decodes with the context's variant: the ordered pairs with SD in first or second place against
        all 23 kinds, both large"""
        return [(self.link(a, "large", (i + j) % 2), self.link(b, "large", (i + j + 1) % 2 + 2))
                for i, a in enumerate(ALL_KINDS) for j, b in enumerate(ALL_KINDS) if "SD" in (a, b)]

    WALK2_FAILURES = tuple(FAILURES2)

    def _wire(self, kind, shape, v, chain):
        """the link of `kind` at the end of `chain`, by the source rules: PD reads the nearest earlier passing PC and F the nearest E
        (the caller has made sure there is one); SD reads the nearest earlier SC; DD, J and XP the nearest earlier passing link that
        leaves a packed arena (PC, PS, TC, T); G and T the nearest earlier XP, whose index nobody has fetched.  Without such a link
        in front the link brings its own inputs."""
        last = lambda kinds: next((x for x in reversed(chain) if x.kind in kinds and not x.fail), None)
        if kind == "PD":
            return self.PD_of(last(("PC",)))
        if kind == "F":
            return self.F_of(last(("E",)))
        if kind == "SD" and last(("SC",)):
            return self.SD_of(last(("SC",)))
        if kind in PACKED_READERS and last(PACKED_SOURCES):
            return {"DD": self.DD_of, "J": self.J_of, "XP": self.XP_of}[kind](last(PACKED_SOURCES))
        if kind in ("G", "T") and last(("XP",)):
            return {"G": self.G_of, "T": self.T_of}[kind](last(("XP",)), v)
        return self.link(kind, shape, v)

    PIPELINES = (("SC", "SD"), ("PC", "DD", "J", "XP", "G", "T", "DD", "J", "XP"), ("PS", "DD", "J", "XP", "T", "G"),
                 ("TC", "DD", "J", "XP"), ("TC", "XP", "G", "T", "J", "DD"))

    def pipelines(self):
        """the chains the features advertise, every consumer reading what its producer has just left on the device (_wire): the
        split compress and its sized decode; a packed, a split and a tables compress (the fourth pipeline's split, the fifth's
        plain) followed by the dense decompress, the join and the index of their arena, and by a gather and a take through that
        index while nobody has fetched it, whose arena is decoded, joined and indexed in turn.  Each in both shapes."""
        out = []
        for n, kinds in enumerate(self.PIPELINES):
            for shape in SHAPES:
                chain = []
                for k, kind in enumerate(kinds):
                    chain.append(self._wire(kind, shape, n % 2 + 2 * (k % 2), chain))
                assert all(x.source is not None for x in chain[1:])
                out.append(chain)
        return out

    def walk2(self, seed, length=40):
        """`length` links drawn over all 23 kinds and both shapes, wired by _wire.  Six positions hold the failing links of
        FAILURES2, each with inputs of its own in place of a drawn link of its kind (or, where the draw has none left, of a drawn
        link that nobody could read: C, R, I, BC, BD, D, S).  No link reads a failed one: _wire passes them over."""
        rng = np.random.default_rng([103, seed])                        # (a stream with which walks 0 and 1 together hold every source rule)
        kinds = [ALL_KINDS[int(k)] for k in rng.integers(0, len(ALL_KINDS), length)]
        shapes = [SHAPES[int(s)] for s in rng.integers(0, 2, length)]
        for first, then in (("PC", "PD"), ("E", "F")):
            for k, kind in enumerate(kinds):
                if kind == then and first not in kinds[:k]:
                    kinds[k] = first
        failing = {}
        for kind, what in self.WALK2_FAILURES:
            spots = [k for k, x in enumerate(kinds) if x == kind and k not in failing]
            if not spots:
                free = [k for k in range(length) if k not in failing and kinds[k] in ("C", "R", "I", "BC", "BD", "D", "S")]
                k = free[int(rng.integers(0, len(free)))]
                kinds[k] = kind
                spots = [k]
            failing[spots[int(rng.integers(0, len(spots)))]] = what
        chain = []
        for k, (kind, shape) in enumerate(zip(kinds, shapes)):
            chain.append(self.link(kind, "small", k % 4, failing[k]) if k in failing else self._wire(kind, shape, k % 4, chain))
        assert sorted((x.kind, x.fail) for x in chain if x.fail) == sorted(self.WALK2_FAILURES)
        assert all(x.source is None or not x.source.fail for x in chain)
        return chain


def plan_packed(sizes, align):
    """the layout rule of packed batches (include/turbosqueeze_amd.h), restated: offsets[i + 1] = round_up(offsets[i] + sizes[i],
    align), the last without the rounding"""
    at, out = 0, []
    for i, s in enumerate(sizes):
        out.append(at)
        at += s
        if i + 1 < len(sizes):
            at = (at + align - 1) & ~(align - 1)
    return out + [at]


def scratch_quantities(link):
    """what the runtime sizes scratch by for this link: blocks per call (tsqa_ctx::reserve; the sharded decode: the owned frames),
    items (tsqa_ctx::reserve_batch: the compressing batch calls), upload bytes (tsqa_uploads::acquire)"""
    q = {"blocks": link.blocks} if hasattr(link, "blocks") else {}
    if link.kind in ("BC", "PC"):
        q["items"] = link.items
    if hasattr(link, "upload"):
        q["upload"] = link.upload
    return q


def scratch_quantities2(link):
    """scratch_quantities for the second catalogue: blocks (tsqa_ctx::reserve: the per-block descriptors; the compressing kinds ask
    for min(blocks, 2 x CUs)), items (reserve_batch and reserve_join), ranges (reserve_cut and reserve_gather), table_blocks
    (reserve_tables) and upload bytes (tsqa_uploads::acquire), each where the kind's entry point asks for it"""
    q = {name: getattr(link, name) for name in ("blocks", "table_blocks", "upload") if hasattr(link, name)}
    if link.kind in ("DD", "TC", "PS", "XP", "J"):
        q["items"] = link.items
    if link.kind in ("K", "T", "G"):
        q["ranges"] = link.n_ranges
    if link.kind == "G":
        q["pieces"] = link.cap_pieces
    return q
