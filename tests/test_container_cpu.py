"""CPU-only: the host-side container helpers tsqa_walk_frames and tsqa_frame_offsets, on containers made by the oracle and on
hand-made and hand-damaged ones.  Every case pins the exact return code; a walk that succeeds must give the frame table that a
plain Python walk gives, and one that fails must leave *n_blocks and *total alone."""
import ctypes as C
import struct

import numpy as np
import pytest

import turbosqueeze_amd as tsq

MiB4 = 1 << 22
SLOT = MiB4 + (MiB4 >> 2)          # TSQ_OUTPUT_SZ: the largest stream a frame may hold
OK, ARG, FORMAT = 0, 3, 4
SENTINEL = 0xA5A5A5A5


def header(nb, total, magic=b"TSQ1"):
    return magic + struct.pack("<IQ", nb, total)


def frame(length, ext, usize):
    """A frame word and a stream of `length` bytes whose first three are the block's output size (the rest is not read by a walk)."""
    word = (length & 0x7FFFFF) | (ext << 23)
    stream = struct.pack("<I", usize)[:3][:length] + bytes(max(length - 3, 0))
    return struct.pack("<I", word)[:3] + stream


def container(frames, nb=None, total=None, magic=b"TSQ1"):
    """frames: (stream length, ext, output size) per block; nb / total default to what the frames say."""
    nb = len(frames) if nb is None else nb
    total = sum(u for _, _, u in frames) if total is None else total
    return header(nb, total, magic) + b"".join(frame(*f) for f in frames)


def py_walk(blob):
    """-> (frame_at, sizes, ext, out_len, total) of a well-formed container"""
    nb, total = struct.unpack_from("<IQ", blob, 4)
    at, rows = 16, []
    for _ in range(nb):
        word = blob[at] | blob[at + 1] << 8 | blob[at + 2] << 16
        ln = word & 0x7FFFFF
        usize = blob[at + 3] | blob[at + 4] << 8 | blob[at + 5] << 16
        rows.append((at, ln, word >> 23, usize))
        at += 3 + ln
    assert at == len(blob)
    return [np.array([r[k] for r in rows], dt) for k, dt in enumerate((np.uint64, np.uint32, np.uint32, np.uint32))] + [total]


def walk(blob, cap=None, size=None):
    """-> (rc, n_blocks, total, frame_at, sizes, ext, out_len) from tsqa_walk_frames"""
    L = tsq.lib()
    size = len(blob) if size is None else size
    cap = max(len(blob) // 6, 1) if cap is None else cap
    arrays = [np.full(cap + 1, SENTINEL, dt) for dt in (np.uint64, np.uint32, np.uint32, np.uint32)]
    nb, total = C.c_uint32(SENTINEL), C.c_uint64(SENTINEL)
    buf = C.create_string_buffer(bytes(blob), max(len(blob), 1))
    rc = L.tsqa_walk_frames(buf, size, cap, *(a.ctypes.data for a in arrays), C.byref(nb), C.byref(total))
    return (rc, nb.value, total.value, *arrays)


def assert_walks(blob, cap=None):
    rc, nb, total, *arrays = walk(blob, cap)
    assert rc == OK
    *want, want_total = py_walk(blob)
    assert nb == len(want[0]) and total == want_total
    for got, exp in zip(arrays, want):
        assert np.array_equal(got[:nb], exp)
        assert (got[nb:] == got.dtype.type(SENTINEL)).all()        # nothing past the last block
    return arrays, nb


def assert_refused(blob, cap=None, size=None):
    rc, nb, total, *_ = walk(blob, cap, size)
    assert rc == FORMAT
    assert nb == SENTINEL and total == SENTINEL                      # written only on success


def offsets(sizes):
    L = tsq.lib()
    sizes = np.ascontiguousarray(sizes, np.uint32)
    frame_at = np.full(len(sizes) + 1, SENTINEL, np.uint64)
    total = C.c_uint64(SENTINEL)
    rc = L.tsqa_frame_offsets(sizes.ctypes.data, len(sizes), frame_at.ctypes.data, C.byref(total))
    return rc, frame_at, total.value


# ---- oracle containers ----

@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("n", [50000, MiB4, 2 * MiB4 + 300000], ids=["one-short-block", "one-full-block", "three-blocks-short-last"])
def test_walk_oracle_container(oracle, ext, n):
    data = tsq.synth.text(n, seed=11)[:n]
    blob = oracle.compress(data, ext, threads=2)
    (frame_at, sizes, exts, out_len), nb = assert_walks(blob)
    assert nb == (n + MiB4 - 1) // MiB4
    assert (exts[:nb] == ext).all()
    assert out_len[:nb].sum() == n and (out_len[:nb - 1] == MiB4).all()
    # the writer's prefix sum over the walked sizes lands every frame where the reader found it
    rc, at, size = offsets(sizes[:nb])
    assert rc == OK and size == len(blob)
    assert np.array_equal(at[:nb], frame_at[:nb]) and at[nb] == SENTINEL


def test_walk_cap_is_exact(oracle):
    blob = oracle.compress(tsq.synth.text(MiB4 + 1000, seed=5)[:MiB4 + 1000], 1, threads=2)
    assert_walks(blob, cap=2)
    assert_refused(blob, cap=1)


# ---- hand-made containers ----

def test_walk_smallest_frames():
    frames = [(3, k & 1, k * 1000) for k in range(9)]               # six bytes each: the stream is only its size word
    blob = container(frames)
    assert len(blob) == 16 + 6 * 9
    assert_walks(blob)
    assert_walks(container([(3, 0, 0)]))                             # one block of nothing
    assert_walks(container([(SLOT, 1, MiB4), (7, 0, 5)]))            # the largest stream, a full block
    assert_refused(container(frames, nb=10))                         # one block more than 16 + 6 * 9 bytes can hold
    assert_refused(container(frames, nb=10) + bytes(5))              # still one byte short of a tenth frame


def test_walk_header_refusals():
    good = container([(40, 0, 1000), (12, 1, 77)])
    assert_walks(good)
    assert_refused(container([(40, 0, 1000), (12, 1, 77)], magic=b"TSQ2"))
    assert_refused(b"\x00" + good[1:])
    assert_refused(good[:15])                                        # no whole header
    assert_refused(good, size=15)
    assert_refused(header(0, 0))
    assert_refused(container([(40, 0, 1000), (12, 1, 77)], nb=0))
    assert_refused(header(1, 0))                                     # a block but no frame
    assert_refused(container([(40, 0, 1000), (12, 1, 77)], nb=3))
    assert_refused(container([(40, 0, 1000), (12, 1, 77)], nb=1))    # the second frame is left over: 1000 != 1077


@pytest.mark.parametrize("length", [0, 1, 2, SLOT + 1, 0x7FFFFF])
def test_walk_bad_frame_length(length):
    good = (20, 0, 100)
    body = frame(length, 1, 100) if length >= 3 else frame(length, 1, 0)
    blob = header(2, 200) + frame(*good) + body + bytes(max(0, 20 - length))
    assert_refused(blob)
    blob = header(2, 200) + body + bytes(max(0, 20 - length)) + frame(*good)
    assert_refused(blob)


def test_walk_frame_past_the_end():
    blob = container([(30, 0, 10), (30, 1, 20)])
    assert_walks(blob)
    assert_refused(blob[:-1])
    assert_refused(blob, size=len(blob) - 1)
    assert_refused(blob[:16 + 33 + 5])                               # the second frame's word is there, its size word is not
    assert_refused(container([(30, 0, 10)], nb=2, total=10))


def test_walk_block_sizes():
    assert_walks(container([(9, 0, MiB4), (9, 0, MiB4)]))
    assert_refused(container([(9, 0, MiB4 + 1)]))
    assert_refused(container([(9, 0, MiB4), (9, 0, MiB4 + 1)]))
    assert_refused(container([(9, 0, (1 << 24) - 1)]))
    assert_refused(container([(9, 0, 100), (9, 0, 200)], total=301))     # sum != total
    assert_refused(container([(9, 0, 100), (9, 0, 200)], total=299))
    assert_refused(container([(9, 0, MiB4), (9, 0, MiB4)], total=2 * MiB4 + 1))   # total > nb * 4 MiB
    assert_refused(container([(9, 0, 100)], total=1 << 40))


# ---- the writer's offsets ----

def test_frame_offsets():
    sizes = [3, SLOT, 1000, 17]
    rc, at, size = offsets(sizes)
    assert rc == OK
    want = np.cumsum([16] + [3 + s for s in sizes])
    assert np.array_equal(at[:4], want[:4]) and size == want[4] and at[4] == SENTINEL
    rc, at, size = offsets([])
    assert rc == OK and size == 16 and at[0] == SENTINEL


@pytest.mark.parametrize("bad", [0, 2, SLOT + 1, 0xFFFFFFFF])
def test_frame_offsets_refusals(bad):
    for sizes in ([bad], [100, bad], [bad, 100, 100]):
        rc, _, size = offsets(sizes)
        assert rc == ARG and size == SENTINEL


def test_null_pointers():
    L = tsq.lib()
    a64, a32 = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    nb, total = C.c_uint32(0), C.c_uint64(0)
    blob = C.create_string_buffer(container([(3, 0, 1)]), 22)
    assert L.tsqa_walk_frames(None, 22, 4, a64.ctypes.data, a32.ctypes.data, a32.ctypes.data, a32.ctypes.data, C.byref(nb), C.byref(total)) == ARG
    assert L.tsqa_walk_frames(blob, 22, 4, None, a32.ctypes.data, a32.ctypes.data, a32.ctypes.data, C.byref(nb), C.byref(total)) == ARG
    assert L.tsqa_walk_frames(blob, 22, 4, a64.ctypes.data, a32.ctypes.data, a32.ctypes.data, a32.ctypes.data, C.byref(nb), None) == ARG
    assert L.tsqa_frame_offsets(None, 1, a64.ctypes.data, C.byref(total)) == ARG
    assert L.tsqa_frame_offsets(a32.ctypes.data, 1, a64.ctypes.data, None) == ARG
