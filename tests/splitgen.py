"""Seeded inputs and expectations for the short-block entry points (tsqa_plan_split, tsqa_compress_device_split*,
tsqa_decompress_device_sized*), shared by test_split_cpu.py -- which shows with the oracle and the host-only planner that each input
reaches what it aims at -- and by test_gpu_split.py, which runs the same inputs through the kernels.  Nothing here calls a kernel.

What is restated here, and must be re-derived with it:
  plan_split        tsqa_plan_split (tsq_runtime.hip), split_bound and block_bound (tsq_format.h)
  expected_split    the container tsqa_compress_device_split_async owes: split_blocks_kernel's cut of the input and its look-ahead
                    (tsq_split.cuh), write_header and write_frame (tsq_format.h)
  pack_cut          split_pack_scan_kernel's rule for an out_cap: what is written, the size needed, the status
  launches, passes  the encode launches of 2 x CUs blocks (tsqa_compress_device_split_async) and the scan's passes of 256 blocks;
                    group_scan_excl64 (tsq_container.cuh) sums the low 24 bits and the rest of every value apart
  sized_refuses     frame_walk_sized_kernel's verdict (tsq_split.cuh) on a container and a table of stream sizes"""
from __future__ import annotations

import numpy as np

BLOCK = 1 << 22                     # TSQ_BLOCK_SZ
OUTPUT_SZ = BLOCK + (BLOCK >> 2)    # TSQ_OUTPUT_SZ
HEADER, WORD, MIN_FRAME = 16, 3, 6  # tsq_format.h
HALO = 128                          # the encoder's look-ahead past a block's end
GROUP = 256                         # blocks per pass of both scans
SPLIT = 1 << 24                     # group_scan_excl64: v & 0xFFFFFF and v >> 24 are summed apart
ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = 3, 4, 6
BLOCK_LENS = tuple(1 << k for k in range(12, 23))


# ---- tsqa_plan_split ------------------------------------------------------------------------------------------------------------------

def block_bound(k):
    return WORD + min(OUTPUT_SZ, 11 + k + (k >> 3) + (k >> 1))


def plan_split(n, block_len):
    """-> (n_blocks, bound), or None where tsqa_plan_split answers TSQA_ERR_ARG"""
    if n <= 0 or block_len not in BLOCK_LENS:
        return None
    nb = -(-n // block_len)
    if nb > 0xFFFFFFFF:
        return None
    rest = n % block_len
    return nb, HEADER + (n // block_len) * block_bound(block_len) + (block_bound(rest) if rest else 0)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------

def mixed(n, seed):
    """n bytes: a third of wordy text, a third of random bytes, a third of zeros, so that the blocks' stream sizes vary"""
    from turbosqueeze_amd import synth
    rng = np.random.default_rng(seed)
    a, b = n // 3, n // 3
    out = np.zeros(n, dtype=np.uint8)
    if a:
        out[:a] = synth.text(a, seed=seed)
    out[a:a + b] = rng.integers(0, 256, b, dtype=np.uint8)
    return out


def count_cases(budget):
    """block counts at block_len 4096 around the scan's pass of 256 and the launch of `budget` = 2 x CUs blocks, each with a last
    block of 1 byte, of block_len - 1 bytes and full -> [(n_blocks, n)], the largest about 4 MiB on a chip of 256 CUs"""
    counts = sorted({1, 2, GROUP - 1, GROUP, GROUP + 1, budget - 1, budget, budget + 1, 2 * budget + 1})
    return [(nb, (nb - 1) * 4096 + last) for nb in counts for last in (1, 4095, 4096)]


COUNT_SEED = 4101


def count_input(budget):
    """one input for all of count_cases: each case is a prefix of it"""
    return mixed((2 * budget + 1) * 4096, COUNT_SEED)


def carry_input():
    """300 blocks of 2^16 random bytes: every stream is longer than its block, so the frame offsets pass 2^24 before block 256"""
    return np.random.default_rng(4102).integers(0, 256, 300 << 16, dtype=np.uint8), 1 << 16


def edge_input(block_len=4096, n_blocks=9):
    """matches run across every block edge: a phrase of 64 bytes over and over, so that a match is under way wherever a block ends
    and what the encoder does in a block's last bytes depends on the bytes behind it.  The phrase divides block_len: every edge
    cuts it at the same place, and what holds at one edge holds at all (test_split_cpu.py shows it for each)."""
    phrase = np.frombuffer(b"the quick brown fox jumps over the lazy dog and runs off again. ", dtype=np.uint8)
    assert phrase.size == 64
    return np.resize(phrase, n_blocks * block_len - 7).copy(), block_len


# ---- the container ---------------------------------------------------------------------------------------------------------------------

_streams: dict = {}


def _stream(oracle, block, halo, ext):
    key = (int(ext), block.tobytes(), halo.tobytes())
    if key not in _streams:
        _streams[key] = oracle.encode_block(block, ext, halo=halo if halo.size else None)
    return _streams[key]


def block_streams(oracle, data, block_len, ext, zero_halo=False):
    """each block's stream: Oracle.encode_block of the block with the input's next 128 bytes as halo, zeros past the end
    (zero_halo: zeros everywhere, which is NOT what the library owes)"""
    n = data.size
    out = []
    for at in range(0, n, block_len):
        end = min(n, at + block_len)
        halo = data[end:end] if zero_halo else data[end:min(n, end + HALO)]
        out.append(_stream(oracle, data[at:end], halo, ext))
    return out


def container_of(streams, n, ext):
    out = bytearray(b"TSQ1" + len(streams).to_bytes(4, "little") + int(n).to_bytes(8, "little"))
    for st in streams:
        out += (len(st) | (int(ext) << 23)).to_bytes(WORD, "little") + st
    return bytes(out)


def expected_split(oracle, data, block_len, ext):
    """-> (the container, the table of stream sizes) that tsqa_compress_device_split owes for `data` (a uint8 array)"""
    streams = block_streams(oracle, data, block_len, ext)
    return container_of(streams, data.size, ext), [len(s) for s in streams]


def frame_places(sizes):
    """-> the offset of every frame word, then the container's size"""
    at, out = HEADER, []
    for s in sizes:
        out.append(at)
        at += WORD + s
    return out + [at]


def pack_cut(container, sizes, out_cap, guard):
    """split_pack_scan_kernel and batch_pack_copy_kernel for an out_cap: the header and every frame that ENDS at or before out_cap
    are written, nothing else -> (the buffer as it must be, starting from `guard`; the size needed; the status)"""
    at = frame_places(sizes)
    want = np.array(guard, dtype=np.uint8, copy=True)
    blob = np.frombuffer(container, dtype=np.uint8)
    if HEADER <= out_cap:
        want[:HEADER] = blob[:HEADER]
    for b, s in enumerate(sizes):
        if at[b] + WORD + s <= out_cap:
            want[at[b]:at[b] + WORD + s] = blob[at[b]:at[b] + WORD + s]
    return want, at[-1], ERR_OVERFLOW if at[-1] > out_cap else 0


def launches(n_blocks, budget):
    return [(b0, min(budget, n_blocks - b0)) for b0 in range(0, n_blocks, budget)]


def carry_crossing(sizes, budget):
    """the blocks b whose frame offset is at or above 2^24 while the first block of b's pass lies below it: there the pass's
    exclusive sum carries out of its low 24 bits.  A pass is 256 blocks of one launch."""
    at = frame_places(sizes)
    out = []
    for b0, nb in launches(len(sizes), budget):
        for k0 in range(0, nb, GROUP):
            lo = at[b0 + k0]
            out += [b for b in range(b0 + k0, b0 + min(nb, k0 + GROUP)) if lo < SPLIT <= at[b]]
    return out


# ---- the sized walk --------------------------------------------------------------------------------------------------------------------

def stream_len_ok(s):
    return 3 <= s <= OUTPUT_SZ


def header_ok(blob, n, n_blocks, out_cap):
    """read_header, the stated block count and the capacity, as both walk kernels ask them -> (ok, total)"""
    if n < HEADER or blob[:4] != b"TSQ1":
        return False, 0
    nb, total = int.from_bytes(blob[4:8], "little"), int.from_bytes(blob[8:16], "little")
    ok = nb >= 1 and nb <= (n - HEADER) // MIN_FRAME and total <= nb * BLOCK and nb == n_blocks and total <= out_cap
    return ok, total


def sized_refuses(blob, n, table, n_blocks, out_cap):
    """frame_walk_sized_kernel on the first n bytes of blob: True where it gives TSQA_ERR_FORMAT.  Frame b is looked for at 16 + the
    sum of 3 + s_j over the table's entries before it, a bad s_j counting as nothing."""
    blob = bytes(blob[:n])
    ok, total = header_ok(blob, n, n_blocks, out_cap)
    if not ok:
        return True
    at, oat, bad = HEADER, 0, False
    for b in range(n_blocks):
        s = int(table[b])
        if not stream_len_ok(s):
            bad = True
            continue
        f_ok = at + MIN_FRAME <= n
        if f_ok:
            word = int.from_bytes(blob[at:at + 3], "little")
            ln, out_len = word & 0x7FFFFF, int.from_bytes(blob[at + 3:at + 6], "little")
            f_ok = stream_len_ok(ln) and at + WORD + ln <= n and out_len <= BLOCK and ln == s
        if f_ok and oat + out_len <= total:
            oat += out_len
        else:
            bad = True
        at += WORD + s
    return bad or oat != total


def walk_refuses(blob, n, n_blocks, out_cap):
    """frame_walk_kernel (walk_frames, tsq_format.h) on the first n bytes of blob"""
    blob = bytes(blob[:n])
    ok, total = header_ok(blob, n, n_blocks, out_cap)
    if not ok:
        return True
    at, oat = HEADER, 0
    for _ in range(n_blocks):
        if at + MIN_FRAME > n:
            return True
        ln, out_len = int.from_bytes(blob[at:at + 3], "little") & 0x7FFFFF, int.from_bytes(blob[at + 3:at + 6], "little")
        if not stream_len_ok(ln) or at + WORD + ln > n or out_len > BLOCK or oat + out_len > total:
            return True
        oat += out_len
        at += WORD + ln
    return oat != total


def false_tables(container, sizes):
    """-> [(name, container, n, table)]: the container is valid and the table or the stated size is not.  One entry off by one at
    index 0, 255, 256 and the last; an entry of 0; one of TSQ_OUTPUT_SZ + 1 and one of 2^32 - 1; two unequal neighbours swapped;
    n cut inside the last frame; and (the table true, the container not) a total off by one."""
    nb = len(sizes)
    assert nb > 257
    out = []

    def add(name, table, blob=container, n=None):
        out.append((name, blob, len(blob) if n is None else n, [int(x) & 0xFFFFFFFF for x in table]))

    for at in (0, 255, 256, nb - 1):
        for d in (1, -1):
            t = list(sizes)
            t[at] += d
            add(f"entry_{at}_{'plus' if d > 0 else 'minus'}_1", t)
    for name, v in (("zero", 0), ("output_sz_plus_1", OUTPUT_SZ + 1), ("all_ones", 0xFFFFFFFF)):
        t = list(sizes)
        t[nb // 2] = v
        add(f"entry_{name}", t)
    k = next(k for k in range(nb // 3, nb - 1) if sizes[k] != sizes[k + 1])
    t = list(sizes)
    t[k], t[k + 1] = t[k + 1], t[k]
    add("neighbours_swapped", t)
    add("n_cut_inside_last_frame", sizes, n=len(container) - max(1, sizes[-1] // 2))
    total = int.from_bytes(container[8:16], "little")
    for d in (1, -1):
        add(f"total_{'plus' if d > 0 else 'minus'}_1", sizes, blob=container[:8] + (total + d).to_bytes(8, "little") + container[16:])
    return out
