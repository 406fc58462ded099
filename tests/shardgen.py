"""Cases for the block and sharded entry points (tsqa_encode_blocks_async, tsqa_decode_blocks_async, tsqa_frames_to_host_async,
tsqa_frames_from_host_async, tsqa_sharded_place_async, tsqa_sharded_fetch_decode_async, tsqa_sharded_decode_again_async), and the
bytes every one of them must leave.  Host only: numpy, the oracle and the two catalogues; nothing here touches a device or calls the
library under test.

Where the expected bytes come from:
  plain bytes    streamgen's builders (the third element of a catalogue block)
  streams        the catalogue's hand-assembled streams for the deals; oracle.encode_block(data, ext, halo) wherever something is
                 encoded (place tables, encode cases)
  containers     streamgen.container(blocks)

  deals()              containers of 1, 2, 7 and 11 tiny, uneven, zero-length, mixed-ext blocks; Deal.shard(world, rank) says what a
                       rank owns and what d_streams and d_out must hold afterwards
  place_tables()       block lists of one level for tsqa_sharded_place_async and the two frame copies
  damage_cases()       the 7-block deal damaged: TSQA_ERR_FORMAT on every rank, or a TSQA_ERR_STREAM twin that costs its owner alone
  encode_one_block()   every encoder-catalogue case of at most one block
  encode_arrangements()   two three-block layouts at every stride
  pack_for_decode()    streams in one arena at every residue mod 16, fenced destinations, descriptors shuffled
  pins()               what tests/golden/shard_cases.json holds

Deals use blocks of bytes to a few KiB (SMALL): a sharded call copies and decodes whatever it owns, and what can go wrong is which
bytes go where.  The only 4 MiB blocks are those of the two encode arrangements and the one TSQ_OUTPUT_SZ stream of a place table.

Restated from the runtime and to be derived again when the line changes:
  tsq_runtime.hip, tsqa_sharded_fetch_decode_async:  n_local = nb > rank ? (nb - rank + world - 1) / world : 0
  tsq_runtime.hip, tsqa_encode_blocks_async:         tail = stride > BLOCK ? min(stride - BLOCK, 128) : 0;
                                                     readable = (n_blocks - 1) * stride + last_len + tail
"""
from __future__ import annotations

import hashlib

import numpy as np

import chaingen
import encgen
import streamgen
from streamgen import BLOCK, OUTPUT_SZ, CATALOGUE

HALO = 128
HEADER = 16
OK, ERR_ARG, ERR_FORMAT, ERR_STREAM, ERR_STALL = 0, 3, 4, 5, 7
SMALL = 8192                                  # a deal's blocks: streams and plain bytes up to this
WORLDS = (1, 2, 3, 5, 8)                      # and nb, nb + 3 per block list
STRIDES = (BLOCK, BLOCK + HALO, BLOCK + HALO + 4096 + 1)
ODD_STRIDES = (BLOCK + 5, BLOCK + 127)
ENC_VARIANTS = (1, 7, 6, 0)
FETCH_VARIANTS = (4, 6, 5, 1, 0)
DECODE_VARIANTS = (1, 4, 5, 6, 3)
SYMBOLS = ("tsqa_encode_blocks_async", "tsqa_decode_blocks_async", "tsqa_frames_to_host_async", "tsqa_frames_from_host_async",
           "tsqa_sharded_place_async", "tsqa_sharded_fetch_decode_async", "tsqa_sharded_decode_again_async")
# include/turbosqueeze_amd.h: tsqa_frame {u64 stream_at, out_at; u32 stream_len, ext, out_len, pad}
FRAME_DTYPE = np.dtype([("stream_at", "<u8"), ("out_at", "<u8"), ("stream_len", "<u4"), ("ext", "<u4"), ("out_len", "<u4"), ("pad", "<u4")])


def digest(data) -> str:
    return hashlib.blake2b(bytes(data), digest_size=16).hexdigest()


def worlds_of(nb):
    return sorted(set(WORLDS) | {nb, nb + 3})


def n_local(nb, world, rank):
    """tsq_runtime.hip, tsqa_sharded_fetch_decode_async"""
    return (nb - rank + world - 1) // world if nb > rank else 0


def image(fill, pieces):
    """`fill` (a numpy uint8 array: the sentinel) with the (offset, bytes) pieces laid over it"""
    out = np.array(fill, dtype=np.uint8, copy=True)
    for at, data in pieces:
        assert 0 <= at and at + len(data) <= out.size, (at, len(data), out.size)
        out[at:at + len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    return out


def frame_table(sizes):
    """the container offset of every block's frame word (16 + the sum over earlier blocks of 3 + size) and the container's size"""
    at, out = HEADER, []
    for s in sizes:
        out.append(at)
        at += 3 + int(s)
    return out, at


def frame_word(size, ext) -> bytes:
    return (int(size) | (int(ext) << 23)).to_bytes(3, "little")


# ----------------------------------------------------------------------------------------------------------------------- deals

class Shard:
    """what rank `rank` of `world` owns of a container: the block indices, and per owned block k its slot (k * OUTPUT_SZ) and its
    output place (k * BLOCK) with the bytes that belong there"""

    def __init__(self, blocks, world, rank):
        self.world, self.rank = world, rank
        self.owned = list(range(rank, len(blocks), world))
        self.n_local = len(self.owned)
        self.stream_pieces = [(k * OUTPUT_SZ, blocks[b][1]) for k, b in enumerate(self.owned)]
        self.out_pieces = [(k * BLOCK, blocks[b][2]) for k, b in enumerate(self.owned)]
        self.out_lens = [len(blocks[b][2]) for b in self.owned]
        # what d_out has to hold for the call to be accepted: the last owned block's end
        self.out_need = (self.n_local - 1) * BLOCK + self.out_lens[-1] if self.owned else 0
        self.streams_need = self.n_local * OUTPUT_SZ


class Deal:
    def __init__(self, name, blocks):
        self.name, self.blocks = name, list(blocks)
        self.nb = len(self.blocks)
        self.container = streamgen.container(self.blocks)
        self.plain = b"".join(p for _, _, p in self.blocks)
        self.total = len(self.plain)
        self.sizes = [len(st) for _, st, _ in self.blocks]
        self.frame_at, size = frame_table(self.sizes)
        assert size == len(self.container)

    def worlds(self):
        return worlds_of(self.nb)

    def shard(self, world, rank):
        return Shard(self.blocks, world, rank)

    def triples(self):
        return [(w, r) for w in self.worlds() for r in range(w)]


def _small(blocks):
    return [b for b in blocks if len(b[1]) <= SMALL and len(b[2]) <= SMALL]


_DEALS = None


def deals():
    """Four containers, of 1, 2, 7 and 11 blocks, dealt from the small blocks of streamgen.uneven_unit() (0, 1, 77 and 0 bytes),
    streamgen.region_container() (the two clamped last matches) and streamgen.blocks_for() (the catalogue's valid streams in turn)"""
    global _DEALS
    if _DEALS is None:
        unit = _small(streamgen.uneven_unit())
        region = _small(streamgen.region_container()[0][6:])
        turn = _small(streamgen.blocks_for(6 + len(CATALOGUE.valid))[6:])
        assert [len(p) for _, _, p in unit] == [0, 1, 77, 0] and len(region) >= 2 and len(turn) >= 40
        zero_ext, one, b77, zero_noext = unit
        out = [Deal("one_block_of_77_bytes", [b77]),
               Deal("zero_length_block_then_a_clamped_match", [zero_noext, region[0]]),
               Deal("seven_uneven_blocks", [zero_ext, one, region[1], b77, turn[3], zero_noext, turn[10]]),
               Deal("eleven_blocks_zero_length_first_and_last", [zero_noext, turn[17], one, region[0], turn[5], b77, turn[23], zero_ext,
                                                                 turn[31], turn[12], zero_ext])]
        assert [d.nb for d in out] == [1, 2, 7, 11]
        for d in out[1:]:
            assert {e for e, _, _ in d.blocks} == {0, 1} and 0 in (len(p) for _, _, p in d.blocks), d.name
            assert len(set(d.sizes)) >= min(d.nb, 4), d.name
        _DEALS = out
    return _DEALS


# ----------------------------------------------------------------------------------------------------------------------- place tables

class PlaceTable:
    """a block list of one level: `streams` in block order.  Place and the frame copies move bytes and do not decode."""

    def __init__(self, name, ext, streams, n_total):
        self.name, self.ext, self.streams, self.n_total = name, ext, [bytes(s) for s in streams], n_total
        self.nb = len(self.streams)
        self.sizes = [len(s) for s in self.streams]
        self.frame_at, self.size = frame_table(self.sizes)
        self.container = (b"TSQ1" + self.nb.to_bytes(4, "little") + int(n_total).to_bytes(8, "little")
                          + b"".join(frame_word(len(s), ext) + s for s in self.streams))
        assert len(self.container) == self.size

    def worlds(self):
        return worlds_of(self.nb)

    def triples(self):
        return [(w, r) for w in self.worlds() for r in range(w)]

    def owned(self, world, rank):
        return list(range(rank, self.nb, world))

    def slot_pieces(self, world, rank):
        """the rank's d_slots: block b's stream in slot b / world"""
        return [(k * OUTPUT_SZ, self.streams[b]) for k, b in enumerate(self.owned(world, rank))]

    def host_pieces(self, world, rank, header=True):
        """what that rank alone writes to the host container: its frames with their three frame bytes, and rank 0 the header"""
        out = [(self.frame_at[b], frame_word(self.sizes[b], self.ext) + self.streams[b]) for b in self.owned(world, rank)]
        if header and rank == 0:
            out.append((0, self.container[:HEADER]))
        return out


def place_tables(oracle):
    """The plain bytes of the 7- and the 11-block deal encoded by the oracle at one level each way (their zero-length blocks keep the
    catalogue's 3-byte streams), one block alone, and one list that holds a stream of exactly TSQ_OUTPUT_SZ bytes (random bytes)."""
    d7, d11 = deals()[2], deals()[3]
    rng = np.random.default_rng(20)
    out = []
    for tag, deal in (("seven", d7), ("eleven", d11)):
        for ext in (0, 1):
            # (the encoder spends six bytes on an empty block; the 3-byte stream of a zero-length block is the catalogue's own)
            streams = [oracle.encode_block(p, ext, None) if p else st for _, st, p in deal.blocks]
            assert min(len(s) for s in streams) == 3
            out.append(PlaceTable(f"{tag}_blocks_{'ext' if ext else 'noext'}", ext, streams, deal.total))
    p = deals()[0].blocks[0][2]
    out.append(PlaceTable("one_block_ext", 1, [oracle.encode_block(p, 1, None)], len(p)))
    full = rng.integers(0, 256, OUTPUT_SZ, dtype=np.uint8).tobytes()
    out.append(PlaceTable("three_bytes_then_a_full_slot_noext", 0, [bytes(3), full], 77))
    assert {t.ext for t in out} == {0, 1} and max(max(t.sizes) for t in out) == OUTPUT_SZ
    return out


# ----------------------------------------------------------------------------------------------------------------------- damage

class Damage:
    """`blob` with `size` as its container_size; `codes[world][rank]`; for a twin, `blocks` (the twin's claimed bytes as zeros) and
    `bad` (its block index)"""

    def __init__(self, name, blob, size, code, blocks=None, bad=None):
        self.name, self.blob, self.size, self.blocks, self.bad = name, bytes(blob), size, blocks, bad
        self.codes = {w: [code if bad is None or bad % w == r else OK for r in range(w)] for w in (1, 2, 3)}

    def triples(self):
        return [(w, r) for w in (1, 2, 3) for r in range(w)]


def damage_cases():
    deal = deals()[2]
    good = bytearray(deal.container)
    n = len(good)
    out = []

    def fmt(name, blob, size=None):
        out.append(Damage(name, blob, len(blob) if size is None else size, ERR_FORMAT))

    b = bytearray(good); b[4:8] = (deal.nb + 1).to_bytes(4, "little")
    fmt("header_count_one_too_high", b)
    fmt("container_size_short_by_1", good, n - 1)
    fmt("container_size_short_by_a_frame", good, n - 3 - deal.sizes[-1])
    b = bytearray(good); b[8:16] = (deal.total + 1).to_bytes(8, "little")
    fmt("total_is_not_the_sum", b)
    b = bytearray(good); at = deal.frame_at[3]; b[at:at + 3] = frame_word(2, deal.blocks[3][0])
    fmt("frame_word_below_3", b)
    b = bytearray(good); at = deal.frame_at[2] + 3
    b[at:at + 3] = (BLOCK + 1).to_bytes(3, "little")
    b[8:16] = (deal.total - len(deal.blocks[2][2]) + BLOCK + 1).to_bytes(8, "little")      # (the header's total follows: one rule is broken)
    fmt("block_over_4MiB", b)
    for v in (0, 1, 2):
        name = chaingen.twin_name(v)
        ext, st = CATALOGUE.invalid[name]
        claimed = int.from_bytes(st[:3], "little")
        blocks = list(deal.blocks)
        blocks[4] = (ext, st, bytes(claimed))
        blob = streamgen.container(blocks)
        out.append(Damage("stream_twin_in_block_4_" + name, blob, len(blob), ERR_STREAM, blocks, 4))
    return out


# ----------------------------------------------------------------------------------------------------------------------- encode cases

def filler(rng, n):
    return rng.integers(1, 256, n, dtype=np.uint8)


def halo_bytes(halo, n=HALO):
    """the first n look-ahead bytes, zeros where the case gives none"""
    return (bytes(halo or b"")[:n]).ljust(n, b"\0")


class EncodeCall:
    """one tsqa_encode_blocks_async call: `buffer` (numpy), n_blocks, stride, last_len, and per block the (data, halo) the oracle is
    asked about (`sees`): the look-ahead the block has at that stride"""

    def __init__(self, name, buffer, n_blocks, stride, last_len, sees):
        self.name, self.buffer, self.n_blocks, self.stride, self.last_len, self.sees = name, buffer, n_blocks, stride, last_len, sees

    def want(self, oracle, ext):
        return [oracle.encode_block(d, ext, h) for d, h in self.sees]

    def datas(self):
        return [d for d, _ in self.sees]


def one_block_cases():
    return [c for c in encgen.catalogue() if 0 < len(c.data) <= BLOCK]


def encode_one_block(case, stride=BLOCK + HALO):
    """the case alone, its halo directly behind last_len, non-zero filler behind what the call may read: behind the 128 look-ahead
    bytes, or behind the stride - BLOCK (< 128) bytes of a narrower stride, which then sees zeros from there on"""
    tail = min(stride - BLOCK, HALO)
    n = len(case.data)
    rng = np.random.default_rng([31, n, stride % 1000])
    seen = halo_bytes(halo_bytes(case.halo)[:tail])
    buf = np.concatenate([np.frombuffer(case.data, dtype=np.uint8), np.frombuffer(halo_bytes(case.halo)[:tail], dtype=np.uint8),
                          filler(rng, 256)])
    return EncodeCall(case.name, buf, 1, stride, n, [(case.data, seen)])


def arrangements():
    """[full_block, two_blocks_edge's first block, a short case] and [two_blocks_edge's first block, full_block, another short case]"""
    by = {c.name: c for c in encgen.catalogue()}
    full, edge = by["full_block"], by["two_blocks_edge"]
    edge0 = encgen.Case("two_blocks_edge_first_block", edge.data[:BLOCK], edge.data[BLOCK:BLOCK + HALO])
    assert len(full.data) == BLOCK and len(edge0.data) == BLOCK
    a, b = by["tail_match_n_minus_5_cont"], by["sweep_1"]
    assert a.halo is not None and b.halo is not None and len(a.data) < BLOCK and len(b.data) < BLOCK
    return {"full_edge_tailmatch": [full, edge0, a], "edge_full_sweep": [edge0, full, b]}


def encode_arrangement(name, cases, stride):
    """The three blocks at `stride`.  Each block is followed by the next block's first 128 bytes and the last by its case's halo;
    every byte that the call may not read holds non-zero filler.  At stride == BLOCK the blocks are contiguous: a block sees the next
    block's own bytes, and the last one zeros although filler follows it."""
    rng = np.random.default_rng([32, stride % 1000, len(name)])
    last = cases[-1]
    buf = filler(rng, 2 * stride + len(last.data) + HALO + 512)
    sees = []
    for k, c in enumerate(cases):
        d = np.frombuffer(c.data, dtype=np.uint8)
        buf[k * stride:k * stride + d.size] = d
        ahead = halo_bytes(cases[k + 1].data) if k + 1 < len(cases) else halo_bytes(c.halo)
        if stride > BLOCK:
            buf[k * stride + d.size:k * stride + d.size + HALO] = np.frombuffer(ahead, dtype=np.uint8)
        elif k + 1 == len(cases):
            ahead = bytes(HALO)
        sees.append((c.data, ahead))
    return EncodeCall(f"{name}@{stride - BLOCK}", buf, len(cases), stride, len(last.data), sees)


# ----------------------------------------------------------------------------------------------------------------------- decode_blocks

def pack_for_decode(blocks, rng, shuffle=True):
    """(ext, stream, plain) blocks -> (arena, frames, outs, out_cap): the k-th stream at a stream_at with residue k mod 16, non-zero
    filler in between; destinations behind gaps of 1..47 bytes (every residue occurs); the descriptors in shuffled order, so out_at is
    not monotonic.  outs[i] = (out_at, out_len) of frames[i]; blocks[order[i]] is what frames[i] describes (`order` is returned last)."""
    at, places = 0, []
    for k, (_, st, _) in enumerate(blocks):
        at += (k - at) % 16
        places.append(at)
        at += len(st)
    arena = filler(rng, at + 64)
    for (_, st, _), a in zip(blocks, places):
        arena[a:a + len(st)] = np.frombuffer(st, dtype=np.uint8)
    oat, outs = 0, []
    for _, _, p in blocks:
        oat += int(rng.integers(1, 48))
        outs.append(oat)
        oat += len(p)
    order = rng.permutation(len(blocks)) if shuffle else np.arange(len(blocks))
    frames = np.zeros(len(blocks), dtype=FRAME_DTYPE)
    for i, b in enumerate(order.tolist()):
        ext, st, p = blocks[b]
        frames[i] = (places[b], outs[b], len(st), ext, len(p), 0)
    return arena, frames, [(outs[b], len(blocks[b][2])) for b in order.tolist()], oat + 64, order.tolist()


def valid_blocks():
    return [(name,) + tuple(v) for name, v in CATALOGUE.valid.items()]


def twin_blocks():
    """every invalid twin -> (name, ext, stream, claimed): the size word as it stands, which the test gives the twin as its
    destination's length and its descriptor's out_len (a claim above 4 MiB is refused by that out_len, and nothing is written)"""
    out = []
    for name, (ext, st) in CATALOGUE.invalid.items():
        claimed = int.from_bytes(st[:3].ljust(3, b"\0"), "little")
        out.append((name, ext, st, claimed))
    return out


# ----------------------------------------------------------------------------------------------------------------------- pins

def counts(oracle=None):
    """how many cases each GPU test has to run (tests/golden/shard_cases.json pins them)"""
    tables = place_tables(oracle) if oracle is not None else None
    out = {"deal_triples": sum(len(d.triples()) for d in deals()),
           "deal_triples_owning_nothing": sum(1 for d in deals() for w, r in d.triples() if n_local(d.nb, w, r) == 0),
           "damage_triples": sum(len(d.triples()) for d in damage_cases()),
           "encode_one_block": len(one_block_cases()),
           "encode_one_block_with_halo": sum(1 for c in one_block_cases() if c.halo is not None),
           "encode_arrangements": len(arrangements()) * len(STRIDES),
           "decode_valid": len(CATALOGUE.valid), "decode_twins": len(CATALOGUE.invalid)}
    if tables is not None:
        out["place_triples"] = sum(len(t.triples()) for t in tables)
    return out


def pins(oracle):
    out = {"deals": {}, "place_tables": {}, "damage": {}, "encode_one_block": {}, "encode_arrangements": {}}
    for d in deals():
        out["deals"][d.name] = {"blocks": d.nb, "container": digest(d.container), "plain": digest(d.plain), "worlds": d.worlds(),
                                "sizes": d.sizes, "out_lens": [len(p) for _, _, p in d.blocks], "ext": [e for e, _, _ in d.blocks]}
    for t in place_tables(oracle):
        out["place_tables"][t.name] = {"blocks": t.nb, "ext": t.ext, "sizes": t.sizes, "container": digest(t.container), "worlds": t.worlds()}
    for d in damage_cases():
        out["damage"][d.name] = {"container": digest(d.blob), "size": d.size, "codes": {str(w): c for w, c in d.codes.items()}}
    for c in one_block_cases():
        call = encode_one_block(c)
        out["encode_one_block"][c.name] = {"input": digest(call.buffer.tobytes()), "streams": [digest(call.want(oracle, e)[0]) for e in (0, 1)]}
    for name, cases in arrangements().items():
        for stride in STRIDES:
            call = encode_arrangement(name, cases, stride)
            out["encode_arrangements"][call.name] = {"input": digest(call.buffer.tobytes()),
                                                     "streams": [[digest(s) for s in call.want(oracle, e)] for e in (0, 1)]}
    out["decode_blocks"] = {"valid": digest("\n".join(sorted(CATALOGUE.valid)).encode()), "twins": digest("\n".join(sorted(CATALOGUE.invalid)).encode())}
    out["counts"] = counts(oracle)
    return out
