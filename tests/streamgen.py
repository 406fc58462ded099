"""Hand-assembled .tsq block streams: valid input that the greedy encoder never emits, and invalid twins one step past each rule.

Every other stream of the suite is the output of an encoder (ours, the oracle's, the reference's golden fixtures: the same greedy
encoder by construction) or such an output with a few bytes damaged.  The block format admits far more: matches of 1..3 bytes,
offsets 1..3 and 0xFFFF, symbols clamped by the block's end, junk behind the last symbol, the
densest (13-byte) and fattest (8 x 64 bytes out of 21) groups for chunks on end, in-chunk copy chains thousands of pairs deep.
`test_stream_conformance_cpu.py::test_encoder_never_emits_what_the_catalogue_adds` states that premise as a test.

  assemble      symbols -> block stream (numpy: a block may hold millions of symbols)
  model_decode  a decoder written from the format description alone: the third statement of the decoder beside
                oracle/tsq_oracle.c and the device kernels
  Builder       writes symbols and the plain bytes together: the expected output of a valid case never comes from a decoder
  CATALOGUE     the fixed, seeded, named cases; pinned by tests/golden/conformance_streams.json

The geometry families aim at the decoder's structure constants.  They are restated here from
turbosqueeze_amd/csrc/tsq_dec_common.cuh (struct SymCfg, lines 48-61) and must be re-derived when one of them changes:
  S = 6144 (line 50), OUTC = 2 S (52), HOP = 16 (53), MAXG = 512 (54), MAXSN = MAXG / HOP + 2 (55), R = 65536 + OUTC + 64 (58);
  the image budget cuts a chunk in front of the group whose output offset in the chunk exceeds OUTC - 528 (group_lanes, line 284);
  a chunk ends with the group that reaches stream offset S of the chunk, and the next one starts behind it (lines 273, 307);
  the waiting list of a wavefront holds 768 entries = 12 passes of 64 (fetch_bytes line 397, jump_pointers lines 472, 496-501).
"""
from __future__ import annotations

import hashlib
from array import array

import numpy as np

BLOCK = 1 << 22                     # TSQ_BLOCK_SZ
OUTPUT_SZ = BLOCK + (BLOCK >> 2)    # TSQ_OUTPUT_SZ: the longest stream a frame may carry

# struct SymCfg, tsq_dec_common.cuh:48-61
S = 6144
OUTC = 2 * S
HOP = 16
MAXG = 512
MAXSN = MAXG // HOP + 2
R = 65536 + OUTC + 64
WAITING = 768                       # entries of a wavefront's waiting list (tsq_dec_common.cuh:397)
CUT_AT = OUTC - 512 - 16            # a group whose output offset in the chunk exceeds this starts the next chunk (line 284)


def span(nib: int, ext: int) -> int:
    """output bytes of a match with that nibble"""
    return (nib + 2) << 4 if (ext and nib < 3) else nib + 1


# ----------------------------------------------------------------------------------------------------------------- assembler

class Symbols:
    """Symbols as arrays: kind (1 literal, 0 match), nibble, offset (0 for literals), and the literals' bytes back to back."""

    def __init__(self, kind, nib, off, payload):
        self.kind = np.asarray(kind, dtype=np.uint8)
        self.nib = np.asarray(nib, dtype=np.uint8)
        self.off = np.asarray(off, dtype=np.uint16)
        self.payload = np.asarray(payload, dtype=np.uint8)

    @classmethod
    def of(cls, symbols) -> "Symbols":
        """from a list: a literal is bytes of length 1..16, a match is (offset, nibble)"""
        if isinstance(symbols, cls):
            return symbols
        kind, nib, off, payload = bytearray(), bytearray(), [], bytearray()
        for s in symbols:
            if isinstance(s, (bytes, bytearray)):
                assert 1 <= len(s) <= 16
                kind.append(1); nib.append(len(s) - 1); off.append(0); payload += s
            else:
                o, nb = s
                assert 0 <= o <= 0xFFFF and 0 <= nb <= 15
                kind.append(0); nib.append(nb); off.append(o)
        return cls(np.frombuffer(bytes(kind), dtype=np.uint8), np.frombuffer(bytes(nib), dtype=np.uint8), off,
                   np.frombuffer(bytes(payload), dtype=np.uint8))

    def __len__(self):
        return int(self.kind.size)


def assemble(symbols, size: int, ext: int, *, pad_bits: int = 1, low_nibble: int = 0, tail: bytes = b"") -> bytes:
    """The block stream of `symbols`: a u24 size, then groups of a control byte (one bit per symbol, first symbol in bit 7, 1 =
    literal) and four pairs, each a size byte (first symbol's nibble high) followed by its two symbols (a literal's bytes, a
    match's u16 offset).  The stream ends right behind the last symbol.  The control bits of the symbols a last group lacks are
    `pad_bits`, the low nibble of a last pair with one symbol is `low_nibble`, `tail` is appended as it is.  `ext` does not change
    the stream's layout (it changes what nibbles 0..2 of a match mean); it is an argument so that a case states its level once."""
    sy = Symbols.of(symbols)
    n = len(sy)
    head = int(size).to_bytes(3, "little")
    if n == 0:
        return head + bytes(tail)
    lit = sy.kind.astype(bool)
    slen = np.where(lit, sy.nib.astype(np.int64) + 1, 2)
    idx = np.arange(n, dtype=np.int64)
    before = np.cumsum(slen) - slen
    pos = 3 + (idx // 8 + 1) + (idx // 2 + 1) + before            # first stream byte of every symbol
    total = int(pos[-1] + slen[-1])
    out = np.zeros(total, dtype=np.uint8)
    out[:3] = np.frombuffer(head, dtype=np.uint8)
    # control bytes
    ng = (n + 7) // 8
    bits = np.full(ng * 8, 1 if pad_bits else 0, dtype=np.uint8)
    bits[:n] = sy.kind
    out[pos[0::8] - 2] = np.packbits(bits.reshape(ng, 8), axis=1, bitorder="big")[:, 0]
    # size bytes
    npair = (n + 1) // 2
    nibs = np.full(npair * 2, low_nibble & 15, dtype=np.uint8)
    nibs[:n] = sy.nib
    out[pos[0::2] - 1] = (nibs[0::2] << 4) | nibs[1::2]
    # matches: the offset, little endian
    mpos = pos[~lit]
    out[mpos] = (sy.off[~lit] & 0xFF).astype(np.uint8)
    out[mpos + 1] = (sy.off[~lit] >> 8).astype(np.uint8)
    # literals: their bytes
    lpos, llen = pos[lit], slen[lit]
    assert int(llen.sum()) == sy.payload.size, "the payload does not hold the literals' bytes"
    if lpos.size:
        pstart = np.cumsum(llen) - llen
        out[np.repeat(lpos - pstart, llen) + np.arange(sy.payload.size, dtype=np.int64)] = sy.payload
    return out.tobytes() + bytes(tail)


# ----------------------------------------------------------------------------------------------------------------- the model

def model_decode(stream: bytes, ext: int, trace: list | None = None):
    """The block format, decoded as it is described: a u24 size (at most 4 MiB); while output is missing, a control byte, then up
    to four pairs: a size byte, then two symbols, both positioned at the output cursor of the pair's start (`origin`).  A literal
    copies nibble + 1 stream bytes, a match its length from `origin - offset`; the last symbol is clamped at `size` (`take`).
    None where a rule is broken: size > 4 MiB; a control byte, size byte, offset byte or one of a literal's `take` bytes past
    the stream's end; offset > origin; take > offset.  `trace` receives (is_literal, nibble, offset, origin, take) per symbol."""
    n = len(stream)
    if n < 3:
        return None
    size = int.from_bytes(stream[:3], "little")
    if size > BLOCK:
        return None
    out = bytearray()
    i = 3
    while len(out) < size:
        if i >= n:
            return None
        ctl = stream[i]; i += 1
        for p in range(4):
            if len(out) >= size:
                break
            if i >= n:
                return None
            sb = stream[i]; i += 1
            origin = len(out)
            for s in range(2):
                room = size - len(out)
                if room <= 0:
                    break
                nib = sb >> 4 if s == 0 else sb & 15
                if (ctl >> (7 - (2 * p + s))) & 1:
                    ln = nib + 1
                    take = ln if ln < room else room
                    if i + take > n:
                        return None
                    out += stream[i:i + take]; i += ln
                    if trace is not None:
                        trace.append((1, nib, 0, origin, take))
                else:
                    if i + 2 > n:
                        return None
                    off = stream[i] | stream[i + 1] << 8; i += 2
                    ln = span(nib, ext)
                    take = ln if ln < room else room
                    if off > origin or take > off:
                        return None
                    src = origin - off
                    out += out[src:src + take]
                    if trace is not None:
                        trace.append((0, nib, off, origin, take))
    return bytes(out)


# ----------------------------------------------------------------------------------------------------------------- builders

class Builder:
    """Symbols and the bytes they stand for, written together.  Also keeps the stream cursor and a model of where the one-workgroup
    decoder starts its chunks (tsq_dec_common.cuh:273,284,307), so that a builder can aim at a chunk's edge, and a dictionary of
    named output regions (`mark`) for the range reads of the GPU tests."""

    def __init__(self, ext: int, seed: int = 0):
        self.ext = ext
        self.rng = np.random.default_rng(seed)
        self.plain = bytearray()
        self.kind, self.nib, self.off, self.payload = bytearray(), bytearray(), array("H"), bytearray()
        self.origin = 0
        self.slen = 0               # stream bytes behind the size word so far
        self.chunk_s = 0            # stream offset (behind the size word) and output position where the current chunk starts
        self.chunk_o = 0
        self.chunks = 1
        self.cut_chunks = 0         # chunks that the image budget started (the others start behind stream byte S of the one before)
        self.closed = False         # a clamped symbol was written: nothing may follow
        self.regions: dict[str, tuple[int, int]] = {}
        self._pool = self.rng.integers(0, 256, size=1 << 16, dtype=np.uint8).tobytes()
        self._pool_at = 0

    # -- state
    @property
    def n(self) -> int:
        return len(self.kind)

    @property
    def pos(self) -> int:
        return len(self.plain)

    def at_group(self) -> bool:
        return self.n % 8 == 0

    def rand(self, k: int) -> bytes:
        if self._pool_at + k > len(self._pool):
            self._pool = self.rng.integers(0, 256, size=max(1 << 16, k), dtype=np.uint8).tobytes()
            self._pool_at = 0
        self._pool_at += k
        return self._pool[self._pool_at - k:self._pool_at]

    def _group_starts(self, pos: int) -> None:
        """a group starts at stream offset slen, output position pos: does it start a chunk?  (the chunk before ended with the
        group that reached its stream byte S, or the image budget cuts the chunk in front of this group)"""
        by_stream = self.slen - self.chunk_s >= S
        if by_stream or pos - self.chunk_o > CUT_AT:
            self.chunk_s, self.chunk_o = self.slen, pos
            self.chunks += 1
            self.cut_chunks += not by_stream

    def next_chunk_s(self) -> int:
        """at a group's start: the stream offset where the chunk of the NEXT group starts (the model moves only when it opens)"""
        assert self.at_group()
        return self.slen if (self.slen - self.chunk_s >= S or self.pos - self.chunk_o > CUT_AT) else self.chunk_s

    def _open(self, stream_bytes: int) -> None:
        assert not self.closed, "a clamped symbol ends the block"
        if self.n % 8 == 0:
            self._group_starts(self.pos)
            self.slen += 1
        if self.n % 2 == 0:
            self.origin = self.pos
            self.slen += 1
        self.slen += stream_bytes

    # -- symbols
    def lit(self, data: bytes, take: int | None = None) -> None:
        """a literal; `take` < len(data): the block ends inside it (all of its bytes are in the stream)"""
        assert 1 <= len(data) <= 16
        self._open(len(data))
        self.kind.append(1); self.nib.append(len(data) - 1); self.off.append(0)
        self.payload += data
        if take is None:
            self.plain += data
        else:
            assert 1 <= take < len(data)
            self.plain += data[:take]
            self.closed = True

    def rlit(self, k: int) -> None:
        self.lit(self.rand(k))

    def match(self, off: int, nib: int, take: int | None = None) -> None:
        """a match from `origin - off`; `take` < its length: the block ends inside it (then only take <= off is required)"""
        ln = span(nib, self.ext)
        self._open(2)
        t = ln if take is None else take
        assert 1 <= t <= ln and t <= off <= self.origin and off <= 0xFFFF, (off, nib, t, self.origin)
        a = self.origin - off
        self.plain += self.plain[a:a + t]
        self.kind.append(0); self.nib.append(nib); self.off.append(off)
        if take is not None and take < ln:
            self.closed = True

    def lits(self, data: bytes, length: int) -> None:
        """len(data) / length literals of `length` bytes each, in bulk, from a group's start"""
        k, rest = divmod(len(data), length)
        assert rest == 0 and self.at_group() and k % 8 == 0 and not self.closed
        per_group = 5 + 8 * length
        # the chunk model, group by group, without a Python loop per symbol
        pos = self.pos
        for _ in range(k // 8):
            self._group_starts(pos)
            self.slen += per_group
            pos += 8 * length
        self.kind += b"\x01" * k
        self.nib += bytes([length - 1]) * k
        self.off.frombytes(bytes(2 * k))
        self.payload += data
        self.plain += data
        self.origin = self.pos - 2 * length

    # -- stream geometry
    def literal_group(self, stream_len: int) -> None:
        """one group of eight random literals that is `stream_len` (13..133) stream bytes long"""
        assert self.at_group() and 13 <= stream_len <= 133
        left = stream_len - 5 - 8
        for k in range(8):
            extra = min(15, left) if k < 7 else left
            if k < 7 and extra:
                extra = min(extra, int(self.rng.integers(0, 16)))
                # keep what the later literals can still take
                extra = max(extra, left - 15 * (7 - k))
            self.rlit(1 + extra)
            left -= extra
        assert left == 0

    def fill_to(self, target: int, prefer: int = 0) -> None:
        """literal groups up to stream offset `target` (behind the size word) exactly; `prefer`: the group length to use while it fits"""
        assert self.at_group()
        while self.slen < target:
            left = target - self.slen
            assert left >= 13, "a group is at least 13 bytes"
            lo, hi = 13, min(133, left)
            g = prefer if (prefer and lo <= prefer <= hi) else int(self.rng.integers(lo, hi + 1))
            if left - g != 0 and left - g < 13:
                g = left - 13 if left - 13 >= 13 else left
                if g > 133:
                    g = 133 if left - 133 >= 13 else 120
            self.literal_group(g)

    def fill_to_chunk_start(self, prefer: int = 13) -> None:
        """literal groups until the next group is the first of a new chunk"""
        assert self.at_group()
        while self.slen - self.chunk_s < S:
            self.literal_group(prefer)

    def pad_group(self) -> None:
        while not self.at_group():
            self.rlit(int(self.rng.integers(1, 5)))

    def mark(self, name: str, lo: int, hi: int | None = None) -> None:
        self.regions[name] = (lo, self.pos if hi is None else hi)

    # -- result
    def symbols(self) -> Symbols:
        return Symbols(np.frombuffer(bytes(self.kind), dtype=np.uint8), np.frombuffer(bytes(self.nib), dtype=np.uint8),
                       np.frombuffer(self.off.tobytes(), dtype=np.uint16), np.frombuffer(bytes(self.payload), dtype=np.uint8))

    def stream(self, **kw) -> bytes:
        return assemble(self.symbols(), self.pos, self.ext, **kw)


def soup(b: Builder, size: int, p_match: float = 0.7, short: bool = False, maxoff: int = 65535, exact: bool = True) -> None:
    """random legal symbols up to `size` output bytes; the last symbol is clamped where it would pass it (`exact`), or left whole"""
    rng = b.rng
    while b.pos < size:
        m = min(1 << 16, size - b.pos + 8)
        u = rng.random((m, 3))
        ll = rng.integers(1, 3 if short else 17, size=m)
        for k in range(m):
            room = size - b.pos
            if room <= 0:
                break
            if not exact:
                room = 1 << 30
            origin = b.pos if b.n % 2 == 0 else b.origin
            nib = int(u[k, 1] * (3 if (short and not b.ext) else 16))
            ln = span(nib, b.ext)
            if u[k, 0] < p_match and ln <= origin:
                hi = min(origin, maxoff)
                r = u[k, 2]
                off = ln if r < 0.3 else hi if r < 0.45 else ln + int((r - 0.45) / 0.55 * (hi - ln + 1))
                off = max(ln, min(off, hi))
                b.match(off, nib, take=room if room < ln else None)
            else:
                ln = int(ll[k])
                data = b.rand(ln)
                b.lit(data, take=room if room < ln else None)


# ----------------------------------------------------------------------------------------------------------------- catalogue

class Catalogue:
    """valid: name -> (ext, stream, plain); invalid: name -> (ext, stream); regions: name -> {region: (lo, hi)} for valid cases.
    Built on first use (a few seconds), then kept."""

    def __init__(self):
        self._built = False
        self._valid: dict[str, tuple[int, bytes, bytes]] = {}
        self._invalid: dict[str, tuple[int, bytes]] = {}
        self._regions: dict[str, dict[str, tuple[int, int]]] = {}
        self.facts: dict[str, object] = {}       # what a builder reached, for the tests that assert the catalogue's geometry

    def _build(self):
        if not self._built:
            self._built = True
            _build_catalogue(self)

    @property
    def valid(self):
        self._build()
        return self._valid

    @property
    def invalid(self):
        self._build()
        return self._invalid

    @property
    def regions(self):
        self._build()
        return self._regions

    # -- used by the builders
    def add(self, name: str, b: Builder, stream: bytes | None = None, **kw) -> None:
        assert name not in self._valid and name not in self._invalid, name
        st = b.stream(**kw) if stream is None else stream
        assert len(st) <= OUTPUT_SZ and b.pos <= BLOCK, name
        self._valid[name] = (b.ext, st, bytes(b.plain))
        self._regions[name] = dict(b.regions)

    def add_invalid(self, name: str, ext: int, stream: bytes) -> None:
        assert name not in self._valid and name not in self._invalid, name
        self._invalid[name] = (ext, stream)


CATALOGUE = Catalogue()


def _seed(name: str) -> int:
    return int.from_bytes(hashlib.blake2b(name.encode(), digest_size=8).digest(), "little")


def _family_short_and_extreme(c: Catalogue) -> None:
    """1. matches of 1..3 bytes; offsets 1, 2, 3, len, 0xFFFE, 0xFFFF, origin; ext: 32/48/64 at offset == length; each as the
    first and as the second symbol of its pair"""
    # the very start of a block: sources at byte 0 while origin is 1, 2, 3
    b = Builder(0, _seed("short_head"))
    b.lit(b"Q"); b.lit(b"r")                        # pair 0: origin 0
    b.match(2, 0); b.match(2, 1)                    # origin 2: off == origin, source at byte 0: 1 byte, then 2 bytes
    b.match(1, 0); b.lit(b"xyz")                    # origin 5: offset 1
    b.lit(b"ab"); b.match(9, 2)                     # origin 9: second symbol, off == origin, 3 bytes from byte 0
    b.match(3, 2); b.match(2, 1)                    # origin 14: off == len for both
    b.match(19, 0); b.match(19, 2)                  # origin 19: off == origin, both symbols
    b.match(23, 1); b.match(23, 0)                  # origin 23: 2 bytes from byte 0 as the first symbol
    b.match(26, 2); b.match(26, 1)                  # origin 26: 3 bytes from byte 0 as the first symbol
    assert b.pos == 31
    b.mark("all", 0)
    c.add("short_head_noext", b)

    for ext in (0, 1):
        b = Builder(ext, _seed(f"short_far{ext}"))
        b.lits(b.rand(16 * 4104), 16)               # 65 664 bytes of history, from a group's start
        nibs = (0, 1, 2) if not ext else (0, 1, 2, 3, 9, 15)
        lo = b.pos
        for nib in nibs:
            ln = span(nib, ext)
            offs = [1, 2, 3, ln, ln + 1, 0xFFFE, 0xFFFF]      # (off == origin: short_head_noext and source_at_byte0_from_0xFFFF_*)
            for off in offs:
                for second in (0, 1):
                    if b.n % 2:
                        b.rlit(1)
                    origin = b.pos
                    o = off
                    if o < ln:
                        continue
                    if second:
                        # the first symbol advances the cursor; the second one's source is still taken from the pair's origin
                        # (off == ln: it ends directly in front of the origin)
                        b.rlit(int(b.rng.integers(1, 17)))
                        b.match(o, nib)
                    else:
                        b.match(o, nib)
                        b.rlit(int(b.rng.integers(1, 4)))
        b.mark("extremes", lo)
        c.add(f"short_and_far_offsets_{'ext' if ext else 'noext'}", b)

    # ext: 32 / 48 / 64 at offset == length, both positions, and both symbols of one pair at once
    b = Builder(1, _seed("ext_eq_len"))
    for k in range(8):
        b.rlit(16)
    for rep in range(40):
        for nib in (0, 1, 2):
            ln = span(nib, 1)
            if b.n % 2:
                b.rlit(3)
            if rep % 3 == 0:
                b.match(ln, nib); b.rlit(1 + rep % 16)
            elif rep % 3 == 1:
                b.rlit(1 + rep % 16); b.match(ln, nib)
            else:
                b.match(ln, nib); b.match(ln, nib)
    c.add("ext_long_matches_offset_eq_len", b)

    # a source at byte 0 of the block from far away: off == origin at 0xFFFF exactly, first and second symbol
    for ext in (0, 1):
        b = Builder(ext, _seed(f"origin_ffff{ext}"))
        b.lits(b.rand(16 * 4088), 16)               # 65 408
        while b.pos < 0xFFFF - 16 or b.n % 2:
            b.rlit(min(16, max(1, 0xFFFF - 16 - b.pos)) if b.pos < 0xFFFF - 16 else 1)
        while b.pos + 2 <= 0xFFFF:                  # literal pairs up to origin 0xFFFF exactly
            left = 0xFFFF - b.pos
            a = min(16, left - 1)
            b.rlit(a); b.rlit(min(16, left - a))
        assert b.pos == 0xFFFF and b.n % 2 == 0, b.pos
        b.match(0xFFFF, 2 if ext else 15); b.match(0xFFFF, 7)
        c.add(f"source_at_byte0_from_0xFFFF_{'ext' if ext else 'noext'}", b)


def _dense_run(b: Builder, groups: int) -> None:
    b.lits(b.rand(8 * groups), 1)


def _fat_run(b: Builder, groups: int) -> None:
    b.lits(b.rand(128 * groups), 16)


def _match_run(b: Builder, groups: int, nibs, near: bool = False) -> None:
    """all-match groups (21 stream bytes each); sources anywhere in the history, or `near`: within the last 2 lengths"""
    for _ in range(8 * groups):
        origin = b.pos if b.n % 2 == 0 else b.origin
        nib = int(nibs[int(b.rng.integers(0, len(nibs)))])
        ln = span(nib, b.ext)
        while ln > origin:
            nib = nib - 1 if nib else 0
            ln = span(nib, b.ext)
            assert ln <= origin
        hi = min(origin, 0xFFFF)
        off = int(b.rng.integers(ln, min(hi, 2 * ln) + 1)) if near else int(b.rng.integers(ln, hi + 1))
        b.match(off, nib)


def _family_density(c: Catalogue) -> None:
    """2. the densest group (13 bytes: MAXG, MAXSN), the longest (133), the fattest (21 bytes -> 512: the image budget OUTC)"""
    per_chunk = S // 13 + 1                                       # 473 groups in a chunk of 13-byte groups
    assert per_chunk + 2 * HOP <= MAXG + HOP and per_chunk <= MAXG
    for ext in (0, 1):
        tag = "ext" if ext else "noext"
        b = Builder(ext, _seed("dense13" + tag))
        _dense_run(b, 5 * per_chunk + 7)
        b.mark("dense", 0)
        assert b.chunks >= 5
        c.add(f"dense13_five_chunks_{tag}", b)
        b = Builder(ext, _seed("fat133" + tag))
        _fat_run(b, 5 * (S // 133 + 1))
        c.add(f"literal133_five_chunks_{tag}", b)
    # the dense run starts at offset 0, 1, 12, 13 of the S-byte grid (and of a chunk of the rolling kind, where the lead-in allows)
    for at in (0, 1, 12, 13):
        b = Builder(0, _seed(f"dense_at{at}"))
        if at:
            b.fill_to(2 * S + at)
        lo = b.pos
        _dense_run(b, 2 * per_chunk + 40)
        b.mark("dense", lo)
        c.add(f"dense13_from_grid_offset_{at}", b, pad_bits=at & 1)
    # 8 x 64 out of 21 bytes: every chunk is cut by the image budget after 23 groups
    b = Builder(1, _seed("fat64"))
    for _ in range(8):
        b.rlit(16)
    lo = b.pos
    _match_run(b, 600, (2,))
    b.mark("match64", lo)
    assert b.chunks >= 600 // 24 and b.pos > 3 * R                # the ring wraps three times
    c.facts["match64_chunks"] = b.chunks
    c.add("match64_groups_cut_by_image_budget_ext", b)
    b = Builder(1, _seed("fat64near"))
    for _ in range(8):
        b.rlit(16)
    _match_run(b, 120, (0, 1, 2), near=True)
    c.add("match_32_48_64_near_sources_ext", b)
    # 8 x 1 out of 21 bytes
    b = Builder(0, _seed("thin1"))
    for _ in range(8):
        b.rlit(3)
    _match_run(b, 4 * (S // 21 + 1), (0,))
    c.add("match1_groups_four_chunks_noext", b)
    b = Builder(0, _seed("thin123"))
    for _ in range(8):
        b.rlit(3)
    _match_run(b, 3 * (S // 21 + 1), (0, 1, 2), near=True)
    c.add("match_1_2_3_near_sources_noext", b)
    # Switches between the three extremes.  A chunk's first group lies at its offset 0 and these groups are 13, 21 or 133 bytes
    # long, so a switch can lie at the offsets 13 a + 21 b + 133 c of its chunk: every such offset below S is aimed at, per level,
    # with all six ordered transitions 13 <-> 21, 133 <-> 21, 13 <-> 133; the residues of the stream position mod S come with it.
    # Under ext the 21-byte groups are 8 x 64 bytes: now and then a run of 30 of them, so that chunks which the image budget cuts
    # (chunk_end's `cut`, tsq_dec_common.cuh:304-307) lie next to chunks that end with their stream byte S (`ng`).
    reach = np.zeros(S, dtype=bool)
    reach[0] = True
    for o in range(S):
        if reach[o]:
            for g in (13, 21, 133):
                if o + g < S:
                    reach[o + g] = True
    kinds = (13, 133, 21)
    for ext in (0, 1):
        tag = "ext" if ext else "noext"
        b = Builder(ext, _seed("switch" + tag))
        for _ in range(8):
            b.rlit(16)
        seen_roll, seen_grid = np.zeros(S, dtype=bool), np.zeros(S, dtype=bool)
        trans = {(p, q): 0 for p in kinds for q in kinds if p != q}
        top = {13: 12, 133: 3 if ext else 6, 21: 1 if ext else 12}
        cur, steps, long_runs = 133, 0, 0
        while b.slen < OUTPUT_SZ - 8192 and b.pos < BLOCK - 40000 and not (seen_roll | ~reach).all():
            off = b.slen - b.next_chunk_s()
            cands = []
            for kind in kinds:
                if kind == cur or (ext and kind == 21 and steps % 4):     # (few enough 8 x 64 groups that most chunks end by stream)
                    continue
                o = off
                for k in range(1, top[kind] + 1):
                    o = (0 if o >= S else o) + kind
                    if not seen_roll[0 if o >= S else o]:
                        cands.append((trans[(cur, kind)], k, kind))
                        break
            if cands:
                _, k, kind = min(cands)
            else:
                kind = min((q for q in kinds if q != cur and not (ext and q == 21 and steps % 4)), key=lambda q: trans[(cur, q)])
                k = 1 + int(b.rng.integers(0, top[kind]))
            if ext and kind == 21 and steps % 211 == 5:
                k, long_runs = 30, long_runs + 1
            if kind == 13:
                _dense_run(b, k)
            elif kind == 133:
                _fat_run(b, k)
            else:
                _match_run(b, k, (2,) if ext else (0, 1, 2))
            trans[(cur, kind)] += 1
            cur, steps = kind, steps + 1
            seen_roll[b.slen - b.next_chunk_s()] = True
            seen_grid[b.slen % S] = True
        c.facts[f"switch_{tag}"] = {"chunk_offsets": int((seen_roll & reach).sum()), "reachable": int(reach.sum()),
                                   "grid_residues": int(seen_grid.sum()), "transitions": dict(trans), "chunks": b.chunks,
                                   "cut_chunks": b.cut_chunks, "matches": int(b.kind.count(0)), "long_runs": long_runs}
        c.add(f"density_switches_{tag}", b)
    # a stream of exactly TSQ_OUTPUT_SZ bytes: 13-byte groups, the rest junk behind the last symbol
    g = (OUTPUT_SZ - 3) // 13
    b = Builder(0, _seed("outputsz"))
    _dense_run(b, g)
    st = b.stream(tail=b.rand(OUTPUT_SZ - 3 - 13 * g))
    assert len(st) == OUTPUT_SZ
    c.add("stream_of_exactly_TSQ_OUTPUT_SZ_noext", b, stream=st)


def _family_geometry(c: Catalogue) -> None:
    """3. chunk edges (S), sources across a chunk's first byte, the ring's end (R) and its wrap, offsets 65 535 / 65 534 just past
    position 65 536"""
    # the group that straddles a chunk's edge, at every split of a 13-byte group: on the rolling chunks of the one-workgroup
    # decoder (the next chunk starts behind the group) and on the fixed grid of S bytes
    def aim(b, k, glen, rolling, prefer, reached):
        """the next group of glen bytes starts k bytes in front of its chunk's stream byte S (0: on it, the next chunk's first)"""
        while True:
            base = b.next_chunk_s() if rolling else (b.slen // S) * S
            target = base + S - k
            if not rolling and target - b.slen < 13:
                target += S
            if target == b.slen or target - b.slen >= 13:
                break
            b.literal_group(13)                                   # too close: go on, into the next chunk if need be
        b.fill_to(target, prefer=prefer)
        starts_chunk = b.next_chunk_s() == b.slen
        b.literal_group(glen)
        if rolling:
            # what the one-workgroup decoder sees: the group lies in the chunk and reaches its byte S (k >= 1), or starts the next
            assert starts_chunk == (k == 0) and (k == 0 or b.next_chunk_s() == b.slen)
        reached.append(k)

    for rolling in (True, False):
        kind = "rolling" if rolling else "grid"
        b = Builder(0, _seed(f"edge13{rolling}"))
        lo, reached = b.pos, []
        for k in list(range(0, 14)) * 2:
            aim(b, k, 13, rolling, 13, reached)
        b.mark("edge_sweep", lo)
        c.facts[f"edge13_{kind}"] = sorted(set(reached))
        c.add(f"edge_sweep_13_byte_group_{kind}", b)
        b = Builder(1, _seed(f"edge133{rolling}"))
        reached = []
        for k in (0, 1, 2, 3, 17, 66, 67, 116, 131, 132, 133):
            aim(b, k, 133, rolling, 0, reached)
        c.facts[f"edge133_{kind}"] = sorted(set(reached))
        c.add(f"edge_sweep_133_byte_group_{kind}", b)
    # sources that begin d1 bytes in front of a chunk's first output byte and end d2 behind it
    for ext in (0, 1):
        b = Builder(ext, _seed(f"srcedge{ext}"))
        lens = (32, 48, 64) if ext else (2, 3, 9, 16)
        combos = [(d1, ln - d1) for ln in lens for d1 in sorted({1, 2, ln // 2, ln - 2, ln - 1}) if 0 < d1 < ln]
        lo = None
        for d1, d2 in combos:
            b.fill_to_chunk_start(prefer=13 if (d1 & 1) else 40)
            start = b.pos                                        # the next group is a chunk's first: its output starts here
            if lo is None:
                lo = start
            e = 0
            while e < d2 or b.n % 2:
                k = min(16, max(1, d2 - e)); b.rlit(k); e += k
            ln = d1 + d2
            nib = {32: 0, 48: 1, 64: 2}[ln] if ext else ln - 1
            assert b.chunk_o == start and b.pos == start + e
            b.match(e + d1, nib)                                  # first symbol of its pair
            b.rlit(5)
            origin = b.pos                                        # the same source once more, as the second symbol of a pair
            b.rlit(3); b.match(origin - (start - d1), nib)
            b.pad_group()
        b.mark("source_across_chunk_start", lo)
        c.add(f"sources_across_chunk_start_{'ext' if ext else 'noext'}", b)
    # the ring: blocks larger than R, sources across the positions congruent to the ring's end for every skew 0..15 of the
    # destination, and offsets 65 535 / 65 534 right behind position 65 536
    for ext in (0, 1):
        b = Builder(ext, _seed(f"ring{ext}"))
        for m in (1, 2, 3):
            while b.pos < m * R + 80:
                if m * R + 80 - b.pos > 4096 and b.at_group():
                    b.lits(b.rand(2048), 16)
                else:
                    b.rlit(16 if m * R + 80 - b.pos >= 16 else 1)
            lo = b.pos
            ln, nib = (64, 2) if ext else (16, 15)
            for skew in range(16):
                for left in (1, ln // 2, ln - 1):
                    if b.n % 2:
                        b.rlit(1)
                    a = m * R - skew - left                        # the source starts `left` bytes in front of the ring's end
                    b.match(b.pos - a, nib)
                    b.rlit(1 + skew % 3); b.match(b.origin - a, nib)   # and as a second symbol
            b.mark(f"ring_end_{m}", lo)
        soup(b, b.pos + 30000, p_match=0.8)
        c.add(f"ring_wraps_and_sources_across_its_end_{'ext' if ext else 'noext'}", b)
    for ext in (0, 1):
        b = Builder(ext, _seed(f"past64k{ext}"))
        b.lits(b.rand(16 * 4088), 16)
        while b.pos < 65536 - 40:
            b.rlit(8)
        for k in range(60):
            if b.n % 2:
                b.rlit(1)
            origin = b.pos
            for off in (65535, 65534):
                if off <= origin:
                    nib = (k % 3) if k % 2 else 3 + k % 13
                    if span(nib, ext) <= off:
                        b.match(off, nib)
            b.rlit(1 + k % 2)
        c.add(f"offsets_65535_65534_past_64k_{'ext' if ext else 'noext'}", b)


def _family_dependencies(c: Catalogue) -> None:
    """4. chunks in which nearly every byte waits for a byte of the same chunk (waiting lists of 768 = 12 passes), chains in which
    every pair copies the pair before it"""
    for ext in (0, 1):
        tag = "ext" if ext else "noext"
        b = Builder(ext, _seed("inchunk" + tag))
        for _ in range(4):
            b.rlit(16)                                            # a 64-byte head
        for _ in range(4):
            b.match(64, 15)                                       # (the head's group is completed by matches)
        lo = b.pos
        groups = 3 * (S // 21 + 1) if not ext else 80
        _match_run(b, groups, (2,) if ext else (15,), near=True)
        b.mark("in_chunk", lo)
        assert b.chunks >= 3
        c.add(f"every_byte_an_in_chunk_pointer_{tag}", b)
    # every pair copies the pair before it: 2 + 3 bytes, offsets 5 and 3 (the second symbol's source is taken from the origin)
    b = Builder(0, _seed("chain"))
    b.lit(b"\x11\x22"); b.lit(b"\x33\x44\x55")
    for _ in range(6000):
        b.match(5, 1); b.match(3, 2)
    assert b.chunks >= 4
    b.mark("chain", 5)
    c.add("chain_of_6000_pairs_noext", b)
    # ... of length-1 matches at offset 1 and 2 (the deepest chain a chunk can hold)
    b = Builder(0, _seed("chain1"))
    b.lit(b"\xA1"); b.lit(b"\xB2")
    for _ in range(5500):
        b.match(2, 0); b.match(1, 0)
    c.add("chain_of_5500_pairs_of_1_byte_noext", b)
    # alternating: this chunk, the previous chunk
    for ext in (0, 1):
        b = Builder(ext, _seed(f"chainalt{ext}"))
        b.lits(b.rand(16 * 1280), 16)                             # 20 480 bytes of history
        w = 64 if ext else 9
        n0, n1 = ((0, 0) if ext else (3, 4))                      # 32 + 32, or 4 + 5
        l0 = span(n0, ext)
        for k in range(5200):
            if k % 2 == 0:
                b.match(w, n0); b.match(w - l0, n1)               # the pair before
            else:
                far = int(b.rng.integers(OUTC + 600, 20000))     # behind the image budget: never this chunk
                b.match(far, n0); b.match(far - l0 if far - l0 >= span(n1, ext) else far, n1)
            if ext and b.pos > BLOCK - 4096:
                break
        c.add(f"chain_alternating_this_and_previous_chunk_{'ext' if ext else 'noext'}", b)


def _family_ends(c: Catalogue) -> None:
    """5. tiny blocks (and one of 77 bytes for the containers of uneven blocks), ends exactly at a pair / group / chunk, clamped last symbols, junk behind the stream, every stream length
    mod 16 (the last, partial word of stage_words, tsq_dec_common.cuh:112)"""
    for size in (0, 1, 2, 15, 16, 17, 77):
        for ext in (0, 1):
            b = Builder(ext, _seed(f"tiny{size}{ext}"))
            left = size
            while left:
                k = min(left, 16 if size != 17 else 9); b.rlit(k); left -= k
            c.add(f"block_of_{size}_bytes_{'ext' if ext else 'noext'}", b, pad_bits=ext)
    b = Builder(0, _seed("tiny_match"))
    b.lit(b"z"); b.lit(b"y"); b.match(2, 1)
    c.add("block_of_4_bytes_with_a_match_noext", b, low_nibble=9, pad_bits=0)
    for where in ("pair", "group", "chunk"):
        for ext in (0, 1):
            b = Builder(ext, _seed(f"endat{where}{ext}"))
            soup(b, 3000, p_match=0.6, exact=False)
            if where == "pair":
                while b.n % 2 == 0 or b.n % 8 == 7:
                    b.rlit(2)
                b.rlit(3)
                assert b.n % 2 == 0 and b.n % 8
            elif where == "group":
                b.pad_group()
            else:
                b.pad_group()
                b.fill_to_chunk_start(prefer=29)
                assert b.slen - b.chunk_s >= S
            c.add(f"ends_exactly_at_a_{where}_{'ext' if ext else 'noext'}", b)
    # a chunk that ends with the stream byte S - 1 exactly, and the block with it
    b = Builder(0, _seed("endchunkexact"))
    b.fill_to(S)
    c.add("ends_with_stream_byte_S_of_the_chunk_noext", b)
    # clamped last symbols
    for ext in (0, 1):
        tag = "ext" if ext else "noext"
        for first in (True, False):
            pos_tag = "first" if first else "second"
            b = Builder(ext, _seed(f"clamplit{ext}{first}"))
            soup(b, 700, exact=False)
            if (b.n % 2 == 0) != first:
                b.rlit(2)
            b.lit(b.rand(16), take=5)
            c.add(f"last_literal_clamped_{pos_tag}_{tag}", b, low_nibble=0xF if first else 0, pad_bits=0)
            # the same block, the stream stopping at `take`: the 11 bytes the block does not need are absent
            b2 = Builder(ext, _seed(f"clamplit{ext}{first}"))
            soup(b2, 700, exact=False)
            if (b2.n % 2 == 0) != first:
                b2.rlit(2)
            b2.lit(b2.rand(16), take=5)
            c.add(f"last_literal_stops_at_take_{pos_tag}_{tag}", b2, stream=b2.stream()[:-11])
            b = Builder(ext, _seed(f"clampmatch{ext}{first}"))
            soup(b, 900, exact=False)
            if (b.n % 2 == 0) != first:
                b.rlit(2)
            nib = 2 if ext else 15
            b.match(span(nib, ext) + 3, nib, take=7)
            c.add(f"last_match_clamped_{pos_tag}_{tag}", b, low_nibble=3 if first else 0)
            # legal only because the block's end clamps it: take <= off < len
            b = Builder(ext, _seed(f"clamplegal{ext}{first}"))
            soup(b, 900, exact=False)
            if (b.n % 2 == 0) != first:
                b.rlit(2)
            b.match(6, nib, take=6)                               # take == off
            b.mark("clamped", b.pos - 6)
            c.add(f"last_match_legal_only_clamped_{pos_tag}_{tag}", b, low_nibble=0xA if first else 0, pad_bits=first)
    # every stream length mod 16, with junk behind the stream, both pad bits, junk low nibbles
    residues = set()
    for t in range(1, 17):
        ext = t & 1
        b = Builder(ext, _seed(f"mod16_{t}"))
        soup(b, 1200 + 77 * t, p_match=0.5, exact=False)
        b.pad_group()
        b.rlit(t)                                                 # a lone first symbol of a last pair
        st = b.stream(pad_bits=(t >> 1) & 1, low_nibble=(t * 7) & 15)
        residues.add(len(st) % 16)
        c.add(f"stream_length_variation_{t:02d}", b, stream=st)
    for tail in (1, 2, 3, 15, 16, 17, 39, 40):
        ext = tail & 1
        b = Builder(ext, _seed(f"tail{tail}"))
        soup(b, 2000 + tail, p_match=0.7)
        if b.n % 2 == 0 and not b.closed:
            b.rlit(1)
        st = b.stream(pad_bits=tail & 1, low_nibble=0xF - (tail & 15), tail=b"\xff" * (tail // 2) + b.rand(tail - tail // 2))
        residues.add(len(st) % 16)
        c.add(f"junk_of_{tail:02d}_bytes_behind_the_stream", b, stream=st)
    # whatever residue is still missing: literal-only blocks of the right length
    for r in range(16):
        if r in residues:
            continue
        b = Builder(0, _seed(f"res{r}"))
        k = 1
        while (3 + 2 + k) % 16 != r:
            k += 1
        b.rlit(k)
        residues.add(len(b.stream()) % 16)
        c.add(f"stream_length_residue_{r:02d}", b)
    c.facts["stream_residues"] = len(residues)


def _family_soups(c: Catalogue) -> None:
    """6. seeded random legal symbol sequences"""
    plan = [(1, {}), (17, {}), (5000, {}), (200_000, {}), (200_000, dict(short=True)), (300_000, dict(p_match=0.97)),
            (150_000, dict(p_match=0.0, short=True)), (400_000, dict(maxoff=300)), (1_000_000, dict(p_match=0.97, maxoff=65535))]
    for ext in (0, 1):
        for k, (size, kw) in enumerate(plan):
            b = Builder(ext, _seed(f"soup{ext}_{k}"))
            soup(b, size, **kw)
            tagk = "_".join(f"{a}{v}" for a, v in sorted(kw.items())).replace(".", "p").replace("True", "")
            c.add(f"soup_{size}_{tagk or 'default'}_{'ext' if ext else 'noext'}", b)
        b = Builder(ext, _seed(f"soupfull{ext}"))
        b.lits(b.rand(16 * 8 * 8192), 16)                         # a MiB of literals in bulk, then the soup up to the full block
        soup(b, BLOCK, p_match=0.85)
        assert b.pos == BLOCK
        c.add(f"soup_full_4MiB_block_{'ext' if ext else 'noext'}", b)


# ---- invalid twins: for every rule of model_decode one stream exactly on it (valid) and one a single step past it

def _prefix(b: Builder, where: str) -> None:
    """the stream in front of a twin's last symbols: a short one (first chunk), or two chunks and a bit, the next group a chunk's first"""
    if where == "first_chunk":
        soup(b, 300, p_match=0.6, exact=False)
        b.pad_group()
    else:
        soup(b, 2000, p_match=0.6, exact=False)
        b.pad_group()
        b.fill_to_chunk_start(prefer=13)
        b.literal_group(21)                                       # the second chunk's first group
        b.fill_to_chunk_start(prefer=21)
        assert b.chunks >= 2 and b.slen - b.chunk_s >= S          # two chunks lie in front; the next group starts the third


def _twins(c: Catalogue) -> None:
    for where in ("first_chunk", "chunk_edge", "last_symbol"):
        for ext in (0, 1):
            tag = f"{where}_{'ext' if ext else 'noext'}"
            pre = "first_chunk" if where == "last_symbol" else where
            more = where != "last_symbol"                          # symbols follow the one on the rule

            def base(name):
                b = Builder(ext, _seed(name + tag))
                _prefix(b, pre)
                return b

            def finish(b):
                if more:
                    b.pad_group()
                    soup(b, b.pos + 200, p_match=0.5)

            # off == origin (valid) / origin + 1
            b = base("origin")
            b.rlit(4); b.rlit(1)
            origin = b.pos
            assert origin <= 0xFFFE
            nib = 3
            b.match(origin, nib)
            at = b.n - 1
            finish(b)
            c.add(f"twin_off_eq_origin_{tag}", b)
            sy = b.symbols()
            sy.off = sy.off.copy(); sy.off[at] = origin + 1
            c.add_invalid(f"twin_off_eq_origin_plus_1_{tag}", ext, assemble(sy, b.pos, ext))
            # take == off (valid) / take == off + 1
            b = base("take")
            b.rlit(4); b.rlit(3)
            nib = 2 if ext else 7
            ln = span(nib, ext)
            b.rlit(2); b.match(ln, nib)
            at = b.n - 1
            finish(b)
            c.add(f"twin_take_eq_off_{tag}", b)
            sy = b.symbols()
            sy.off = sy.off.copy(); sy.off[at] = ln - 1
            c.add_invalid(f"twin_take_eq_off_plus_1_{tag}", ext, assemble(sy, b.pos, ext))

    # the truncations end the stream by their nature; `where` is what lies in front of them
    for where in ("first_chunk", "chunk_edge", "last_symbol"):
        for ext in (0, 1):
            tag = f"{where}_{'ext' if ext else 'noext'}"
            pre = "first_chunk" if where == "last_symbol" else where
            size_extra = 0 if where == "last_symbol" else 50       # bytes the size word asks for behind the truncated symbol

            def base(name):
                b = Builder(ext, _seed(name + tag))
                _prefix(b, pre)
                return b

            def emit(name_ok, name_bad, b, ok_cut, bad_cut):
                """the valid twin holds the block up to and with the last symbol; the invalid one asks for `size_extra` more bytes
                (or for the symbol itself) and stops bad_cut bytes early"""
                st = b.stream()
                c.add(name_ok + "_" + tag, b, stream=st[:len(st) - ok_cut] if ok_cut else st)
                bad = bytearray(st[:len(st) - bad_cut])
                bad[0:3] = (b.pos + size_extra).to_bytes(3, "little")
                c.add_invalid(name_bad + "_" + tag, ext, bytes(bad))

            # the offset's second byte: present / missing
            b = base("offbyte")
            b.rlit(6); b.rlit(2); b.match(5, 4)
            emit("twin_offset_complete", "twin_offset_second_byte_missing", b, 0, 1)
            # a literal's `take` bytes: all / take - 1 present (a literal with take < len is the block's last symbol by nature:
            # `where` varies what lies in front of it)
            b = base("litbytes")
            b.rlit(6); b.lit(b.rand(12), take=8)
            st = b.stream()
            c.add(f"twin_literal_take_bytes_present_{tag}", b, stream=st[:-4])
            c.add_invalid(f"twin_literal_take_minus_1_bytes_present_{tag}", ext, st[:-5])
            # control byte: the block is complete with a group's last symbol (no further control byte needed) / one more byte is
            # asked for and the control byte of the group that would hold it is missing
            b = base("ctl")
            b.rlit(3)
            b.pad_group()
            st = b.stream()
            c.add(f"twin_no_control_byte_needed_{tag}", b)
            bad = bytearray(st); bad[0:3] = (b.pos + 1).to_bytes(3, "little")
            c.add_invalid(f"twin_control_byte_missing_{tag}", ext, bytes(bad))
            # size byte: the block is complete with a pair's second symbol inside a group / one more byte is asked for: the control
            # byte is there, the pair's size byte is missing
            b = base("szb")
            b.rlit(3); b.rlit(2)
            assert b.n % 8 == 2
            st = b.stream()
            c.add(f"twin_no_size_byte_needed_{tag}", b)
            bad = bytearray(st); bad[0:3] = (b.pos + 1).to_bytes(3, "little")
            c.add_invalid(f"twin_size_byte_missing_{tag}", ext, bytes(bad))

    # the size word: 4 MiB exactly / 4 MiB + 1; size 0 with a 3-byte stream / size 1 with a 3-byte stream
    b = Builder(0, _seed("full_literals"))
    b.lits(b.rand(BLOCK), 16)
    st = b.stream()
    c.add("twin_size_word_4MiB_noext", b, stream=st)
    c.add_invalid("twin_size_word_4MiB_plus_1_noext", 0, (BLOCK + 1).to_bytes(3, "little") + st[3:] + b"\x80\x00\x41")
    # (the valid twin of the next one is block_of_0_bytes_ext: size 0, a 3-byte stream)
    c.add_invalid("twin_size_1_with_a_3_byte_stream_ext", 1, (1).to_bytes(3, "little"))
    c.add_invalid("twin_size_4MiB_with_a_3_byte_stream_noext", 0, BLOCK.to_bytes(3, "little"))
    c.add_invalid("twin_stream_of_2_bytes_noext", 0, b"\x00\x00")


def _build_catalogue(c: Catalogue) -> None:
    _family_short_and_extreme(c)
    _family_density(c)
    _family_geometry(c)
    _family_dependencies(c)
    _family_ends(c)
    _family_soups(c)
    _twins(c)


def container(blocks) -> bytes:
    """A .tsq container of the given (ext, stream, plain) blocks, in that order: magic, block count, the sum of the blocks' sizes,
    then per block a u24 frame word (stream length, ext in bit 23) and the stream (tsq_container.cuh)."""
    total = sum(len(p) for _, _, p in blocks)
    out = bytearray(b"TSQ1" + len(blocks).to_bytes(4, "little") + total.to_bytes(8, "little"))
    for ext, st, _ in blocks:
        out += (len(st) | (int(ext) << 23)).to_bytes(3, "little") + st
    return bytes(out)


def bad_container(ext: int, stream: bytes, claimed: int | None = None) -> bytes:
    """a one-block container around an invalid stream; the header's total is the stream's own size word unless `claimed`"""
    size = int.from_bytes(stream[:3].ljust(3, b"\0"), "little") if claimed is None else claimed
    return b"TSQ1" + (1).to_bytes(4, "little") + size.to_bytes(8, "little") + (len(stream) | (int(ext) << 23)).to_bytes(3, "little") + stream


# ---- the containers of uneven blocks that the CPU and the GPU tests assemble from the catalogue

MiB4 = BLOCK


def uneven_unit():
    """blocks of 0, 1, 4 MiB, 77, 0 and about 3 MiB, in that order, ext bits mixed"""
    v = CATALOGUE.valid
    names = ["block_of_0_bytes_ext", "block_of_1_bytes_noext", "soup_full_4MiB_block_ext", "block_of_77_bytes_noext",
             "block_of_0_bytes_noext", "stream_of_exactly_TSQ_OUTPUT_SZ_noext"]
    unit = [v[n] for n in names]
    assert [len(p) for _, _, p in unit][:5] == [0, 1, MiB4, 77, 0] and 3_000_000 < len(unit[5][2]) < 3_400_000
    assert {e for e, _, _ in unit} == {0, 1}
    return unit


def blocks_for(n):
    """n blocks: the uneven unit, then the catalogue's smaller valid streams in turn"""
    small = [c for c in CATALOGUE.valid.values() if len(c[1]) <= 400_000]
    out = uneven_unit()
    k = 0
    while len(out) < n:
        out.append(small[k % len(small)]); k += 1
    return out[:n]


def region_container():
    """the uneven unit plus the blocks whose builders marked adversarial regions -> (blocks, names)"""
    names = ["dense13_five_chunks_noext", "match64_groups_cut_by_image_budget_ext", "edge_sweep_13_byte_group_rolling",
             "edge_sweep_13_byte_group_grid", "last_match_legal_only_clamped_first_ext", "last_match_legal_only_clamped_second_noext",
             "sources_across_chunk_start_ext", "sources_across_chunk_start_noext", "ring_wraps_and_sources_across_its_end_ext",
             "ring_wraps_and_sources_across_its_end_noext", "every_byte_an_in_chunk_pointer_noext", "chain_of_6000_pairs_noext"]
    blocks = uneven_unit() + [CATALOGUE.valid[n] for n in names]
    return blocks, [None] * 6 + names
