"""Cases and expectations of the CRC tests (test_crc_cpu.py, test_gpu_crc.py).  Every expected value is zlib.crc32 of bytes that the
generators hold -- nothing expected comes from the library under test -- and the arithmetic of the issue is restated here in Python
(mul, xpow8) so that the tests can hold the library's own against it.

The constants restated here and the kernel lines they follow from:
  CELL = 16        flush_crc walks the image by aligned 16-byte ring cells (tsq_dec_common.cuh: `cells = (skew + im.len + 15u) >> 4`)
  OUTC = 12 288    an image is at most SymCfg::OUTC = 2 * S bytes (tsq_dec_common.cuh: `OUTC = 2 * S`, S = 6144)
  RING = 77 888    the ring's size SymCfg::R = 65536 + OUTC + 64, where a cell address wraps (`a -= a >= C::R ? C::R : 0u`)
  the ring's skew of a block is 0 in dec_crc_kernel (tsq_dec_sym.cuh: `oskew = kCrc ? 0u : ...`), so position p of a block lies
  in cell p // 16 at byte p % 16, and an image that starts at block position op starts at byte op % 16 of its first cell."""
import functools
import zlib

import numpy as np

import cutgen as cg
import densegen as dg
import findgen as fg
import gathergen as gg
import joingen as jg
import recordgen as rg

OK, ERR_ARG, ERR_FORMAT, ERR_STREAM = 0, 3, 4, 5
P = 0xEDB88320
CELL, OUTC, RING = 16, 12288, 65536 + 12288 + 64
SEED = 9710
IDENTITY_SIZES = (0, 1, 3, 16, 17, 100, 5000)
COMBINE_LENGTHS = (0, 1, 2 ** 29 - 1, 2 ** 29, 2 ** 29 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7)
COUNTS = jg.COUNTS


# ---- the arithmetic, as the issue states it -------------------------------------------------------------------------------------------

def mul(a, b):
    r = 0
    for i in range(32):
        if a & (1 << (31 - i)):
            r ^= b
        b = (b >> 1) ^ (P if b & 1 else 0)
    return r


def xpow8(n):            # x^(8n): square and multiply; n is 64-bit
    r, b = 0x80000000, 0x00800000
    while n:
        if n & 1:
            r = mul(r, b)
        b = mul(b, b)
        n >>= 1
    return r


def reg(m: bytes) -> int:
    """R(M): the CRC register behind M with init 0 and no final xor, bit by bit"""
    c = 0
    for byte in m:
        c ^= byte
        for _ in range(8):
            c = (c >> 1) ^ (P if c & 1 else 0)
    return c


def combine(a: int, b: int, len_b: int) -> int:
    return mul(a, xpow8(len_b)) ^ b


# ---- cases ----------------------------------------------------------------------------------------------------------------------------

class Case:
    """an index and what tsqa_crc32_async owes for it.  stream_items: the items one of whose blocks holds a malformed stream."""

    def __init__(self, name: str, index: gg.Index, statuses=None, stream_items=()):
        self.name, self.index, self.stream_items = name, index, tuple(stream_items)
        self.statuses = list(statuses) if statuses is not None else [0] * index.n_items

    def item_at(self):
        i = self.index
        return [i.out_start[fb] for fb in i.item_first]

    def expect(self):
        """-> dict: items, status (per item), all, blocks (None inside an item whose status is nonzero: undefined), d_status"""
        i = self.index
        if i.refused:
            return dict(items=[0] * i.n_items, status=[ERR_FORMAT] * i.n_items, all=0, blocks=[None] * i.n_blocks, d_status=ERR_FORMAT)
        status = [ERR_STREAM if k in self.stream_items else st for k, st in enumerate(self.statuses)]
        items, blocks = [], [None] * i.n_blocks
        for k in range(i.n_items):
            a, t = i.item_span(k)
            items.append(zlib.crc32(i.data[a:a + t]) if status[k] == 0 else 0)
            if status[k] == 0:
                for b in range(i.item_first[k], i.item_first[k + 1]):
                    blocks[b] = zlib.crc32(i.data[i.out_start[b]:i.out_start[b + 1]])
        bad = bool(self.stream_items)
        return dict(items=items, status=status, all=0 if bad else zlib.crc32(i.data), blocks=blocks, d_status=ERR_STREAM if bad else OK)


def _oracle():
    return dg._oracle()


def _compress(data: bytes, ext: int) -> bytes:
    return bytes(_oracle().compress(np.frombuffer(data, dtype=np.uint8), ext, threads=1))


@functools.lru_cache(maxsize=None)
def ragged(n: int, joined: bool) -> Case:
    """joingen's ragged batch of n items of 1 to 40 bytes of text: as a batch index every item is a block that starts a cell and ends
    at every tail length; joined into ONE container the same blocks are parts of one item, which the fold shifts by every residue"""
    items = jg.counts()[COUNTS.index(n)].items
    blobs, datas = [it.blob for it in items], [it.data for it in items]
    if not joined:
        return Case(f"ragged_{n}", rg.batch_of(f"crc_ragged_{n}", blobs, datas))
    blob, _ = jg.joined(blobs)
    _, out_start = cg.walk(blob)
    return Case(f"ragged_{n}_joined", gg.Index(f"crc_ragged_{n}_joined", "plain", bytes(blob), b"".join(datas), out_start))


def bit_items():
    """256 items of 32 bytes, item k with bit k of the 256 set and nothing else: a wrong bit or byte order moves the CRC"""
    out = []
    for k in range(256):
        d = bytearray(32)
        d[k >> 3] = 1 << (k & 7)
        out.append(bytes(d))
    return out


@functools.lru_cache(maxsize=None)
def bits() -> Case:
    datas = bit_items()
    return Case("bits", rg.batch_of("crc_bits", [_compress(d, k & 1) for k, d in enumerate(datas)], datas))


def one_block(data: bytes, ext: int) -> bytes:
    """a container of ONE block assembled by hand from the oracle's block stream, as findgen.seam_source is: the only way to an item
    of 0 bytes that an index accepts (the container of no bytes has no block, and a block count of 0 is refused)"""
    st = bytes(_oracle().encode_block(np.frombuffer(data, dtype=np.uint8), ext))
    return b"TSQ1" + (1).to_bytes(4, "little") + len(data).to_bytes(8, "little") + (len(st) | (ext << 23)).to_bytes(cg.WORD, "little") + st


@functools.lru_cache(maxsize=None)
def runs(byte: int) -> Case:
    """32 items of 0 to 31 bytes of one value (0 or 0xFF): R of zeros is 0 whatever their number, so only the init term tells the
    lengths apart; the item of 0 bytes owes 0"""
    datas = [bytes([byte]) * n for n in range(32)]
    return Case(f"runs_{byte:02x}", rg.batch_of(f"crc_runs_{byte:02x}", [one_block(d, k & 1) for k, d in enumerate(datas)], datas))


CHUNK_CASES = fg.CHUNK_CASES
IMAGE_CASES = ("zeros_outc", "zeros_outc_1", "random_outc", "random_outc_1", "text_2outc_1")


@functools.lru_cache(maxsize=None)
def chunks(kind: str) -> Case:
    return Case(f"chunks_{kind}", fg.chunk_edges(kind).index)


@functools.lru_cache(maxsize=None)
def images(kind: str) -> Case:
    """blocks of exactly OUTC bytes and of OUTC + 1: zeros, which the decoder takes in images as long as an image can be, and random
    bytes and text, whose images end wherever the stream's chunks do"""
    what, size = kind.split("_", 1)
    n = {"outc": OUTC, "outc_1": OUTC + 1, "2outc_1": 2 * OUTC + 1}[size]
    data = (np.zeros(n, dtype=np.uint8) if what == "zeros" else dg._text(n, SEED) if what == "text" else
            np.random.default_rng(SEED + n).integers(0, 256, n, dtype=np.uint8))
    return Case(f"images_{kind}", rg.plain_of(f"crc_images_{kind}", data))


def ring_cases():
    return [Case("ring_wrap", fg.ring_wrap().index), Case("ring_wrap_skewed", fg.ring_wrap_skewed().index)]


@functools.lru_cache(maxsize=None)
def two_blocks(ext: int) -> Case:
    """4 MiB + 1 random bytes: the first block's word is shifted over one byte only, and its own cells over the largest distance
    inside a block"""
    s = cg.two_blocks()
    if ext:
        return Case("two_blocks_ext", gg.from_source(s, "plain"))
    return Case("two_blocks_plain", rg.plain_of("crc_two_blocks_plain", np.frombuffer(s.data, dtype=np.uint8), ext=0))


def phrase(kind: str) -> Case:
    """257 blocks of 4 096 bytes through a sized index and through tsqa_index_create"""
    return Case(f"phrase_{kind}", gg.from_source(fg.phrase_source(), kind))


def damaged() -> Case:
    """recordgen's batch of 300 with densegen's damaged headers: the index refuses items DAMAGED_AT"""
    c = rg.damaged()
    return Case("damaged", c.index, c.item_status())


@functools.lru_cache(maxsize=None)
def twin(which: int = 0) -> Case:
    """mtgen's twin container -- six well-formed frames, one with a stream the decoder refuses -- as the middle item of three, between
    two healthy ones: its blocks' data is unknown (zeros stand in), its CRC owed is 0"""
    import mtgen
    name, blob, k, _ = [t for t in mtgen.twin_containers() if t[3] == "stream"][which]
    total = int.from_bytes(blob[8:16], "little")
    a, b = dg._text(5000, SEED + 1).tobytes(), dg._text(70000, SEED + 2).tobytes()
    return Case(f"twin_{name}", rg.batch_of(f"crc_twin_{which}", [_compress(a, 1), bytes(blob), _compress(b, 0)], [a, bytes(total), b]), stream_items=(1,))


def refused_case() -> Case:
    return Case("refused_index", gg.refused())


def no_blocks() -> Case:
    return Case("no_blocks", fg.no_blocks().index, [ERR_FORMAT, ERR_FORMAT])


def host_cases():
    """the cases whose decoded bytes the CPU tests put through tsqa_plan_crc32"""
    return ([ragged(n, j) for n in (1, 2, 257) for j in (False, True)] + [bits(), runs(0), runs(255), damaged(), no_blocks()] +
            [chunks(k) for k in CHUNK_CASES] + [images(k) for k in IMAGE_CASES] + ring_cases() + [phrase("plain")])
