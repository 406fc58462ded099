"""Seeded cases and expectations for the index of a short-block container made from its size table (tsqa_index_create_sized*),
shared by test_seek_cpu.py -- which shows with the oracle and tsqa_walk_frames that each case reaches what it aims at -- and by
test_gpu_seek.py, which runs the same cases through the kernels.  Nothing here calls a kernel.

What is restated here, and must be re-derived with it:
  host_refuses      tsqa_index_create_sized_async's TSQA_ERR_ARG (tsq_runtime.hip): tsqa_plan_split's refusals, n < 16 + 6 * n_blocks
  index_refuses     the walk's verdict (tsq_index.cuh): the header against the caller's count and total (index_scan_kernel); every
                    frame's place from the table, sized_frame_ok (tsq_split.cuh) and the uniform geometry (index_check_kernel)
  GROUP, PASS       index_sum_kernel and index_check_kernel take 256 frames per workgroup, index_scan_kernel 256 groups per pass:
                    scan_edge_counts are PASS * GROUP - 1, PASS * GROUP and PASS * GROUP + 1 frames
  out_start, reads  the host's plan of a sized index: block b's output starts at min(b * block_len, n_total)
The inputs and the false tables are splitgen's; what splitgen restates is named there."""
from __future__ import annotations

import numpy as np

import splitgen as sg

GROUP = 256                         # frames per workgroup of launches 1 and 3 (kIndexGroup)
PASS = 256                          # groups per pass of launch 2
ERR_ARG, ERR_FORMAT = sg.ERR_ARG, sg.ERR_FORMAT

# why the walk refuses: one word per check of the verdict
HEADER, COUNT, TOTAL, WORD, OUTSIDE, FRAME, LENGTH, GEOMETRY = "header", "count", "total", "table_word", "frame_outside_n", "read_frame", "length", "geometry"


def scan_edge_counts():
    return [PASS * GROUP - 1, PASS * GROUP, PASS * GROUP + 1]


def host_refuses(n, n_total, block_len):
    plan = sg.plan_split(n_total, block_len)
    return plan is None or n < sg.HEADER + sg.MIN_FRAME * plan[0]


def index_refuses(blob, n, table, n_total, block_len):
    """the verdict of tsqa_index_create_sized_async on the first n bytes of blob, for arguments the host takes: the set of the
    reasons for TSQA_ERR_FORMAT, empty where the verdict is TSQA_OK"""
    assert not host_refuses(n, n_total, block_len)
    blob = bytes(blob[:n])
    n_blocks = sg.plan_split(n_total, block_len)[0]
    why = set()
    if n < sg.HEADER or blob[:4] != b"TSQ1":
        why.add(HEADER)
    else:
        nb, total = int.from_bytes(blob[4:8], "little"), int.from_bytes(blob[8:16], "little")
        if nb == 0 or nb > (n - sg.HEADER) // sg.MIN_FRAME or total > nb * sg.BLOCK:
            why.add(HEADER)
        else:
            if nb != n_blocks:
                why.add(COUNT)
            if total != n_total:
                why.add(TOTAL)
    at = sg.HEADER
    for b in range(n_blocks):
        s = int(table[b])
        if not sg.stream_len_ok(s):
            why.add(WORD)                                    # (counts as 0: the frames behind it are looked for as if it were not there)
            continue
        if at + sg.MIN_FRAME > n:
            why.add(OUTSIDE)
        else:
            ln, out_len = int.from_bytes(blob[at:at + 3], "little") & 0x7FFFFF, int.from_bytes(blob[at + 3:at + 6], "little")
            if not sg.stream_len_ok(ln) or at + sg.WORD + ln > n or out_len > sg.BLOCK:
                why.add(FRAME)
            elif ln != s:
                why.add(LENGTH)
            elif out_len != (block_len if b + 1 < n_blocks else n_total - b * block_len):
                why.add(GEOMETRY)
        at += sg.WORD + s
    return why


def out_start(n_total, block_len):
    nb = sg.plan_split(n_total, block_len)[0]
    return [min(b * block_len, n_total) for b in range(nb + 1)]


def reads(n_total, block_len):
    """the reads of a true case -> [(offset, length)]: the whole range; six bytes across every block edge; byte 0; the last byte;
    the last block (one byte long in a third of count_cases)"""
    nb = sg.plan_split(n_total, block_len)[0]
    out = [(0, n_total), (0, 1), (n_total - 1, 1), ((nb - 1) * block_len, n_total - (nb - 1) * block_len)]
    out += [(b * block_len - 3, 6) for b in range(1, nb) if b * block_len + 3 <= n_total]
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------------------------

def true_cases(budget):
    """-> [(n_blocks, n)] at block_len 4096, prefixes of splitgen.count_input(budget): 1, 2, 255, 256, 257, B - 1, B, B + 1 and
    2B + 1 blocks, the last of 1 byte, of 4095 and full"""
    return sg.count_cases(budget)


def carry():
    """splitgen.carry_input(): 300 blocks of 2^16 random bytes.  The frame places pass 2^24 inside the first group of 256 frames
    (launch 3's scan carries out of its low 24 bits) and the second group's base is above 2^24 already (launch 2 hands on a sum
    whose upper part is not 0)."""
    return sg.carry_input()


def false_tables(container, sizes):
    """splitgen.false_tables with what each aims at -> [(name, container, n, table, reason)]"""
    out = []
    for name, blob, n, table in sg.false_tables(container, sizes):
        why = (WORD if name in ("entry_zero", "entry_output_sz_plus_1", "entry_all_ones") else
               FRAME if name == "n_cut_inside_last_frame" else TOTAL if name.startswith("total_") else LENGTH)
        out.append((name, blob, n, table, why))
    return out


def cut_container(oracle, data, cuts, ext):
    """the container of `data` cut where `cuts` says, each piece encoded as the split compress encodes a block (the next 128 bytes
    as look-ahead) -> (container, sizes)"""
    assert sum(cuts) == data.size
    streams, at = [], 0
    for k in cuts:
        streams.append(oracle.encode_block(data[at:at + k], ext, halo=data[at + k:at + k + sg.HALO] if at + k < data.size else None))
        at += k
    return sg.container_of(streams, data.size, ext), [len(s) for s in streams]


GEOMETRY_SEED = 4201


def geometry(oracle, ext):
    """containers that walk_frames and a true table accept, offered with a geometry they do not have
    -> [(name, container, table, n_total, block_len, reason)]"""
    out = []
    for cuts in ([4096, 1, 4096], [4096, 4095, 4096, 4096]):
        data = sg.mixed(sum(cuts), GEOMETRY_SEED)
        blob, sizes = cut_container(oracle, data, cuts, ext)
        out.append(("cuts_" + "_".join(map(str, cuts)), blob, sizes, data.size, 4096, GEOMETRY))
    data = sg.mixed((1 << 21) + 5, GEOMETRY_SEED + 1)
    blob, sizes = sg.expected_split(oracle, data, sg.BLOCK, ext)
    # (the table is padded to the two words that the stated geometry reads: the header's count refuses the container)
    out.append(("plain_4mib_as_2mib", blob, sizes + [3], data.size, 1 << 21, COUNT))
    data = sg.mixed(5 * 4096 - 7, GEOMETRY_SEED + 2)
    blob, sizes = sg.expected_split(oracle, data, 4096, ext)
    out.append(("total_plus_1", blob, sizes, data.size + 1, 4096, TOTAL))
    out.append(("total_minus_1", blob, sizes, data.size - 1, 4096, TOTAL))
    out.append(("block_len_doubled", blob, sizes, data.size, 8192, COUNT))
    return out


def cuts(container, sizes):
    """a true container with less room than it needs -> [(name, n, reason)]"""
    return [("one_byte_short", len(container) - 1, FRAME), ("least_room", sg.HEADER + sg.MIN_FRAME * len(sizes), OUTSIDE)]


def damaged(container, sizes, k):
    """one byte flipped in the middle of block k's stream: the walk does not look there"""
    at = sg.frame_places(sizes)[k] + sg.WORD + sizes[k] // 2
    assert sizes[k] // 2 >= 3
    out = bytearray(container)
    out[at] ^= 0x5A
    return bytes(out)


def scan_edge_input(n):
    """n bytes in splitgen.mixed's style with a zero-filled middle: text, zeros, random bytes, a third each"""
    from turbosqueeze_amd import synth
    a = n // 3
    out = np.zeros(n, dtype=np.uint8)
    out[:a] = synth.text(a, seed=4202)
    out[n - a:] = np.random.default_rng(4203).integers(0, 256, a, dtype=np.uint8)
    return out
