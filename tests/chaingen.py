"""Seeded links and chains for the call-chain tests (test_call_chains_cpu.py, test_gpu_call_chains.py).  Host only: numpy, the
oracle and the catalogue of hand-assembled streams; nothing here touches a device.

A link is ONE stream-ordered call of the C ABI with everything it needs: its inputs, the lengths of its destinations, the status
it must leave and the bytes, sizes and tables it must produce.  Every expected value is the oracle's (oracle.compress for
containers and block streams, the original bytes for decodes, after oracle.decompress(container) == original has been checked once
per input); none comes from the library.  A chain is a list of links for one stream with no synchronise between them.

Eleven kinds (KINDS), two shapes each: "small" stays under a fresh context's first capacities, "large" exceeds every capacity the
small shape establishes.  The capacities are restated from the runtime; each constant names its source line and has to be derived
again when that line changes (README.md lists them)."""
from __future__ import annotations

import numpy as np

import fuzzgen
import streamgen

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

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_OVERFLOW, ERR_STALL = 0, 3, 4, 5, 6, 7

KINDS = ("C", "D", "E", "F", "S", "R", "I", "BC", "BD", "PC", "PD")
ENTRY = {"C": "tsqa_compress_device_async", "D": "tsqa_decompress_device_async", "E": "tsqa_encode_blocks_async",
         "F": "tsqa_decode_blocks_async", "S": "tsqa_sharded_fetch_decode_async", "R": "tsqa_decompress_ranges_async",
         "I": "tsqa_decompress_item_ranges_async", "BC": "tsqa_compress_batch_async", "BD": "tsqa_decompress_batch_async",
         "PC": "tsqa_compress_batch_packed_async", "PD": "tsqa_decompress_batch_packed_async"}
SHAPES = ("small", "large")
DECODERS = ("D", "F", "S", "BD", "PD", "R", "I")
# the failing links: (kind, what is wrong) -> the status the call must leave in its own word
FAILURES = {("D", "twin"): ERR_STREAM, ("BD", "twin"): ERR_STREAM, ("PD", "twin"): ERR_STREAM, ("R", "twin"): ERR_STREAM,
            ("BC", "room"): ERR_OVERFLOW, ("PC", "room"): ERR_OVERFLOW, ("D", "count"): ERR_FORMAT}

LARGE_BLOCK_BYTES = 2 * BLOCK + 12_345       # three blocks
LARGE_ITEMS, LARGE_RANGES = 300, 400
SMALL_ITEMS, SMALL_RANGES = 3, 3
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
    """one call: `kind`, `shape`, `fail` (None, "twin", "room" or "count"), `want_status`, and the kind's own fields"""

    def __init__(self, kind, shape, fail=None, **fields):
        assert kind in KINDS and shape in SHAPES and (fail is None or (kind, fail) in FAILURES)
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
