"""GPU side of tests/shardgen.py: the block and sharded entry points (the family bench.py --gpus N runs) against hand-assembled
containers, with guard bytes round every destination -- the host container, d_streams, d_slots, d_sizes and d_out.

Every expected byte is the generator's (streamgen's builders, oracle.encode_block, streamgen.container); none comes from the
library.  That the generator is right is what test_shard_cases_cpu.py and tests/golden/shard_cases.json establish.  All "ranks"
live in this process: one DeviceCodec per rank, used in turn.  Device buffers are compared on the device, whole: d_streams and d_out
hold eleven slots / blocks (the 11-block deal at world 1) plus a fence, filled with test_gpu_range.sentinel before every call.

Stalls: the decoders on several workgroups per block may report TSQA_ERR_STALL on a busy GPU.  That is documented behaviour; the
documented remedy is applied exactly once (tsqa_sharded_decode_again_async behind a fetch, decode variant 4 for
tsqa_decode_blocks_async), the same bytes are then checked, and the last test prints how many there were.

Ordering: torch's default stream has the handle 0, which the library reads as "the context's own stream", so torch's fills and the
library's calls are not ordered by a stream here.  Every buffer is therefore filled and waited for before a call (Fenced.reset), and
every call is waited for before its buffers are looked at.

No case is dropped: every test counts its cases and the last test compares the counts with the golden's."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import shardgen
from shardgen import BLOCK, OUTPUT_SZ, ERR_STALL, FRAME_DTYPE
from test_gpu_range import ERR_ARG, ERR_FORMAT, ERR_STREAM, codec, sentinel, to_dev, tsq  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shard_cases.json")))
COUNTS: dict = {}
STALLS: dict = {}
SLOTS = 11                                     # the most blocks a rank owns here
FENCE = 4096
MAX_WORLD = 14                                 # nb + 3 of the 11-block deal


def count(entry, k=1):
    COUNTS[entry] = COUNTS.get(entry, 0) + k


def stall(entry):
    STALLS[entry] = STALLS.get(entry, 0) + 1
    print(f"{entry}: TSQA_ERR_STALL, applying the documented remedy once")


def fill(n):
    """test_gpu_range.sentinel(n), without the 8-byte temporaries: its period is 251"""
    return np.tile(sentinel(251), n // 251 + 1)[:n]


def sync():
    import torch
    torch.cuda.synchronize()


def as_u8(data):
    return np.frombuffer(bytes(data), dtype=np.uint8).copy()


class Fenced:
    """a device buffer of n bytes, its sentinel, and a scratch for the image it must hold after a call"""

    def __init__(self, n):
        self.n = n
        self.master = to_dev(fill(n))
        self.buf = self.master.clone()
        self.want = self.master.clone()
        sync()

    def reset(self, pieces=()):
        self.buf.copy_(self.master)
        for at, data in pieces:
            if len(data):
                self.buf[at:at + len(data)] = to_dev(as_u8(data))
        sync()                                     # (torch's default stream is not the context's own: see the module's docstring)

    def check(self, pieces, what):
        """the whole buffer: the pieces where they belong, the sentinel in between and behind"""
        import torch
        self.want.copy_(self.master)
        for at, data in pieces:
            if len(data):
                self.want[at:at + len(data)] = to_dev(as_u8(data))
        if not torch.equal(self.buf, self.want):
            first = int(torch.nonzero(self.buf != self.want)[0])
            inside = [(at, len(d)) for at, d in pieces if at <= first < at + len(d)]
            pytest.fail(f"{what}: byte {first} of {self.n} differs ({'inside the destination at %d of %d bytes' % inside[0] if inside else 'OUTSIDE every destination'})")

    def check_outside(self, spans, what):
        """nothing outside the (offset, length) spans was written"""
        import torch
        diff = self.buf != self.master
        for at, ln in spans:
            diff[at:at + ln] = False
        if bool(diff.any()):
            pytest.fail(f"{what}: byte {int(torch.nonzero(diff)[0])} outside every destination was written")


class Host:
    """a pinned host buffer"""

    def __init__(self, n):
        import torch
        self.t = torch.empty(n, dtype=torch.uint8).pin_memory()
        self.np = self.t.numpy()
        self.ptr = self.t.data_ptr()
        self.n = n


@pytest.fixture(scope="module")
def ranks(tsq):
    cs = [tsq.DeviceCodec(0) for _ in range(MAX_WORLD)]
    yield cs
    for c in cs:
        c.close()


@pytest.fixture(scope="module")
def bufs(tsq):
    class B:
        streams = Fenced(SLOTS * OUTPUT_SZ + FENCE)
        out = Fenced(SLOTS * BLOCK + FENCE)
        streams2 = Fenced(6 * OUTPUT_SZ + FENCE)
        out2 = Fenced(6 * BLOCK + FENCE)
    assert np.array_equal(fill(100_000), sentinel(100_000))
    return B


@pytest.fixture(scope="module")
def host(tsq):
    return Host(OUTPUT_SZ + (1 << 16)), Host(1 << 16)


@pytest.fixture(scope="module")
def tables(oracle):
    return shardgen.place_tables(oracle)


# ------------------------------------------------------------------------------------------------ raw calls (status and caps chosen here)

def fetch(c, host_ptr, size, rank, world, d_streams, streams_cap, d_out, out_cap, status=None):
    total = C.c_uint64(0xDEAD)
    st = c._status if status is None else status
    rc = c.L.tsqa_sharded_fetch_decode_async(c.h, host_ptr, size, rank, world, d_streams.data_ptr(), streams_cap, d_out.data_ptr(), out_cap,
                                             st.data_ptr(), C.byref(total), c._stream())
    return rc, int(total.value)


def decode_again_refused(tsq, c, d_streams, d_out):
    with pytest.raises(tsq.TsqError) as e:
        c.sharded_decode_again_async(d_streams, d_out)
    assert e.value.code == ERR_ARG, e.value


def settle_fetch(c, entry, d_streams, d_out):
    """wait; after TSQA_ERR_STALL decode the frames, still on the device, once more on one workgroup per block -> status"""
    sync()
    st = c.status()
    if st == ERR_STALL:
        stall(entry)
        c.sharded_decode_again_async(d_streams, d_out)
        sync()
        st = c.status()
    return st


def table_arrays(t, world, rank):
    """the explicit form of a rank's frames: sizes and frame_at of its owned blocks (one spare entry, so that no pointer is null
    for a rank that owns nothing)"""
    owned = t.owned(world, rank)
    sizes = np.array([t.sizes[b] for b in owned] + [0], dtype=np.uint32)
    frame_at = np.array([t.frame_at[b] for b in owned] + [0], dtype=np.uint64)
    return owned, sizes, frame_at


def frames_to_host(c, d_slots, sizes, frame_at, n, ext, host_ptr):
    return c.L.tsqa_frames_to_host_async(c.h, d_slots.data_ptr(), sizes.ctypes.data, frame_at.ctypes.data, n, ext, host_ptr, c._stream())


def frames_from_host(c, host_ptr, frame_at, sizes, n, d_streams):
    return c.L.tsqa_frames_from_host_async(c.h, host_ptr, frame_at.ctypes.data, sizes.ctypes.data, n, d_streams.data_ptr(), c._stream())


# ------------------------------------------------------------------------------------------------ 1. tsqa_sharded_place_async

def test_place_writes_its_own_frames_and_nothing_else(tsq, ranks, bufs, host, tables):
    hc = host[0]
    for t in tables:
        window = t.size + FENCE
        guard = fill(window)
        sizes = np.array(t.sizes, dtype=np.uint32)
        for world in t.worlds():
            # every rank alone over a fresh sentinel, then all ranks into one container with host_cap exact
            for alone in (True, False):
                hc.np[:window] = guard
                for rank in range(world):
                    if alone:
                        hc.np[:window] = guard
                    slots = t.slot_pieces(world, rank)
                    bufs.streams.reset(slots)
                    got = ranks[rank].sharded_place_async(bufs.streams.buf, sizes, t.n_total, rank, world, t.ext, hc.ptr, window if alone else t.size)
                    sync()
                    assert got == t.size, (t.name, world, rank)
                    if alone:
                        want = shardgen.image(guard, t.host_pieces(world, rank))
                        assert np.array_equal(hc.np[:window], want), (t.name, world, rank, int(np.flatnonzero(hc.np[:window] != want)[0]))
                        bufs.streams.check(slots, f"d_slots of {t.name} world {world} rank {rank}")
                        count("place")
                if not alone:
                    assert bytes(hc.np[:t.size]) == t.container, (t.name, world)
                    assert np.array_equal(hc.np[t.size:window], guard[t.size:]), (t.name, world)


def test_place_refusals_write_nothing(tsq, ranks, bufs, host, tables):
    hc = host[0]
    n = 0
    for t in tables:
        window = t.size + FENCE
        guard = fill(window)
        for world in (1, 2, 3):
            for rank in range(world):
                c = ranks[rank]
                slots = t.slot_pieces(world, rank)
                foreign = [b for b in range(t.nb) if b % world != rank]
                calls = [(np.array(t.sizes, dtype=np.uint32), t.size - 1)]
                for bad in (2, OUTPUT_SZ + 1):
                    if foreign:
                        sizes = np.array(t.sizes, dtype=np.uint32)
                        sizes[foreign[-1]] = bad
                        calls.append((sizes, window))
                for sizes, cap in calls:
                    hc.np[:window] = guard
                    bufs.streams.reset(slots)
                    with pytest.raises(tsq.TsqError) as e:
                        c.sharded_place_async(bufs.streams.buf, sizes, t.n_total, rank, world, t.ext, hc.ptr, cap)
                    assert e.value.code == ERR_ARG, (t.name, world, rank, e.value)
                    sync()
                    assert np.array_equal(hc.np[:window], guard), (t.name, world, rank, "a refused place wrote to the host container")
                    bufs.streams.check(slots, f"d_slots of {t.name} world {world} rank {rank} after a refusal")
                    n += 1
    assert n >= 6 * len(tables)
    count("place_refusals", n)


# ------------------------------------------------------------------------------------------------ 2. the two frame copies

def test_frames_to_host_and_from_host_in_the_explicit_form(tsq, ranks, bufs, host, tables):
    hc = host[0]
    for t in tables:
        window = t.size + FENCE
        guard = fill(window)
        for world, rank in t.triples():
            c = ranks[rank]
            owned, sizes, frame_at = table_arrays(t, world, rank)
            slots = t.slot_pieces(world, rank)
            # to host: the frames with their frame words (size | ext << 23), no header, nothing else
            hc.np[:window] = guard
            bufs.streams.reset(slots)
            assert frames_to_host(c, bufs.streams.buf, sizes, frame_at, len(owned), t.ext, hc.ptr) == 0, c.last_error()
            sync()
            want = shardgen.image(guard, t.host_pieces(world, rank, header=False))
            assert np.array_equal(hc.np[:window], want), (t.name, world, rank, int(np.flatnonzero(hc.np[:window] != want)[0]))
            for b in owned:
                word = int.from_bytes(bytes(hc.np[t.frame_at[b]:t.frame_at[b] + 3]), "little")
                assert word == t.sizes[b] | t.ext << 23, (t.name, b)
            bufs.streams.check(slots, f"d_slots of {t.name} world {world} rank {rank}")
            count("frames_to_host")
            # from host: exactly sizes[b] bytes per slot
            hc.np[:t.size] = as_u8(t.container)
            bufs.streams.reset()
            assert frames_from_host(c, hc.ptr, frame_at, sizes, len(owned), bufs.streams.buf) == 0, c.last_error()
            sync()
            bufs.streams.check(slots, f"d_streams of {t.name} world {world} rank {rank}")
            assert bytes(hc.np[:t.size]) == t.container
            count("frames_from_host")


def test_frame_copies_validate_every_size_before_they_copy(tsq, ranks, bufs, host, tables):
    """a bad size in the LAST block: the copies of the blocks in front of it must not have been enqueued, and no frame word written"""
    hc = host[0]
    n = 0
    for t in tables:
        window = t.size + FENCE
        guard = fill(window)
        for world in (1, 2):
            for rank in range(world):
                owned, sizes, frame_at = table_arrays(t, world, rank)
                if len(owned) < 2:
                    continue
                c = ranks[rank]
                slots = t.slot_pieces(world, rank)
                for bad in (2, 0, OUTPUT_SZ + 1):
                    wrong = sizes.copy()
                    wrong[len(owned) - 1] = bad
                    hc.np[:window] = guard
                    bufs.streams.reset(slots)
                    assert frames_to_host(c, bufs.streams.buf, wrong, frame_at, len(owned), t.ext, hc.ptr) == ERR_ARG
                    sync()
                    assert np.array_equal(hc.np[:window], guard), (t.name, world, rank, bad, "a refused frames_to_host wrote to the host")
                    hc.np[:t.size] = as_u8(t.container)
                    bufs.streams.reset()
                    assert frames_from_host(c, hc.ptr, frame_at, wrong, len(owned), bufs.streams.buf) == ERR_FORMAT
                    sync()
                    bufs.streams.check([], f"d_streams of {t.name} world {world} rank {rank} after a refused frames_from_host (size {bad})")
                    n += 1
    assert n >= 12
    count("frame_copy_refusals", n)


# ------------------------------------------------------------------------------------------------ 3. tsqa_sharded_fetch_decode_async

def put_container(hc, blob):
    hc.np[:] = fill(hc.n)
    hc.np[:len(blob)] = as_u8(blob)


@pytest.mark.parametrize("variant", shardgen.FETCH_VARIANTS)
def test_fetch_decode_of_every_deal_on_every_rank(tsq, ranks, bufs, host, variant):
    """4: one workgroup per block; 6: two; 5: three; 1: the serial decoder (this one reads its container from a plain pageable numpy
    array); 0: the library's own choice, which for so few blocks is three"""
    hc = host[1]
    for d in shardgen.deals():
        if variant == 1:
            pageable = np.concatenate([as_u8(d.container), fill(256)])
            ptr = pageable.ctypes.data
        else:
            put_container(hc, d.container)
            ptr = hc.ptr
        for world, rank in d.triples():
            c = ranks[rank]
            s = d.shard(world, rank)
            c.set_variant(0, variant)
            bufs.streams.reset(); bufs.out.reset()
            what = f"{d.name} world {world} rank {rank} variant {variant}"
            rc, total = fetch(c, ptr, len(d.container), rank, world, bufs.streams.buf, bufs.streams.n, bufs.out.buf, bufs.out.n)
            assert rc == 0 and total == d.total, (what, rc, total, c.last_error())
            st = settle_fetch(c, f"fetch_variant_{variant}", bufs.streams.buf, bufs.out.buf)
            c.set_variant(0, 0)
            assert st == 0, (what, st)
            bufs.streams.check(s.stream_pieces, "d_streams of " + what)
            bufs.out.check(s.out_pieces, "d_out of " + what)
            if s.n_local == 0:
                decode_again_refused(tsq, c, bufs.streams.buf, bufs.out.buf)
                count("fetch_owning_nothing")
            count(f"fetch_variant_{variant}")


def test_fetch_decode_capacities(tsq, ranks, bufs, host):
    hc = host[1]
    for d in shardgen.deals():
        put_container(hc, d.container)
        for world, rank in d.triples():
            c = ranks[rank]
            s = d.shard(world, rank)
            if s.n_local == 0:
                continue
            what = f"{d.name} world {world} rank {rank}"
            # exactly what the rank needs: (n_local - 1) * BLOCK + out_len(last), n_local * OUTPUT_SZ
            bufs.streams.reset(); bufs.out.reset()
            rc, total = fetch(c, hc.ptr, len(d.container), rank, world, bufs.streams.buf, s.streams_need, bufs.out.buf, s.out_need)
            assert rc == 0 and total == d.total, (what, rc, c.last_error())
            assert settle_fetch(c, "fetch_capacities", bufs.streams.buf, bufs.out.buf) == 0, what
            bufs.streams.check(s.stream_pieces, "d_streams of " + what)
            bufs.out.check(s.out_pieces, "d_out of " + what)
            short = [(s.streams_need - 1, s.out_need)] + ([(s.streams_need, s.out_need - 1)] if s.out_need else [])
            for streams_cap, out_cap in short:
                # over a fresh sentinel: a refusal that had enqueued the accepted call's copies again would show
                bufs.streams.reset(); bufs.out.reset()
                rc, _ = fetch(c, hc.ptr, len(d.container), rank, world, bufs.streams.buf, streams_cap, bufs.out.buf, out_cap)
                assert rc == ERR_FORMAT, (what, streams_cap, out_cap, rc)
                decode_again_refused(tsq, c, bufs.streams.buf, bufs.out.buf)
                sync()
                bufs.streams.check([], "d_streams of " + what + " after a refused fetch")
                bufs.out.check([], "d_out of " + what + " after a refused fetch")
            count("fetch_capacities")


def test_fetch_decode_of_damaged_containers(tsq, ranks, bufs, host):
    """a damaged frame is refused on every rank with nothing written; a damaged stream costs the rank that owns it and nobody else"""
    hc = host[1]
    good = shardgen.deals()[2]
    for dmg in shardgen.damage_cases():
        for world, rank in dmg.triples():
            c = ranks[rank]
            want = dmg.codes[world][rank]
            what = f"{dmg.name} world {world} rank {rank}"
            # a healthy fetch first: a refusal has something to forget
            put_container(hc, good.container)
            rc, _ = fetch(c, hc.ptr, len(good.container), rank, world, bufs.streams.buf, bufs.streams.n, bufs.out.buf, bufs.out.n)
            assert rc == 0 and settle_fetch(c, "fetch_damage", bufs.streams.buf, bufs.out.buf) == 0, what
            put_container(hc, dmg.blob)
            bufs.streams.reset(); bufs.out.reset()
            rc, total = fetch(c, hc.ptr, dmg.size, rank, world, bufs.streams.buf, bufs.streams.n, bufs.out.buf, bufs.out.n)
            if want == ERR_FORMAT:
                assert rc == ERR_FORMAT, (what, rc)
                decode_again_refused(tsq, c, bufs.streams.buf, bufs.out.buf)
                sync()
                bufs.streams.check([], "d_streams of " + what)
                bufs.out.check([], "d_out of " + what)
            else:
                assert rc == 0 and total == sum(len(p) for _, _, p in dmg.blocks), (what, rc, total)
                st = settle_fetch(c, "fetch_damage", bufs.streams.buf, bufs.out.buf)
                assert st == want, (what, st)
                s = shardgen.Shard(dmg.blocks, world, rank)
                bufs.streams.check(s.stream_pieces, "d_streams of " + what)
                if want == 0:
                    bufs.out.check(s.out_pieces, "d_out of " + what)
                else:
                    bufs.out.check_outside([(at, len(p)) for at, p in s.out_pieces], "d_out of " + what)
            count("fetch_damage")


def test_two_fetches_back_to_back_on_one_context(tsq, ranks, bufs, host):
    """no synchronise in between: the second call overwrites the context's pinned descriptor table only behind the first call's copy
    of it (host_frames_copied).  Other containers, worlds and buffers; one workgroup per block, which waits for nobody."""
    import torch
    c = ranks[0]
    d_a, d_b = shardgen.deals()[3], shardgen.deals()[2]
    s_a, s_b = d_a.shard(2, 1), d_b.shard(3, 0)
    assert s_a.n_local == 5 and s_b.n_local == 3
    ha, hb = host
    put_container(ha, d_a.container); put_container(hb, d_b.container)
    st_a = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    st_b = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    bufs.streams.reset(); bufs.out.reset(); bufs.streams2.reset(); bufs.out2.reset()
    c.set_variant(0, 4)
    try:
        sync()
        rc_a, tot_a = fetch(c, ha.ptr, len(d_a.container), 1, 2, bufs.streams.buf, bufs.streams.n, bufs.out.buf, bufs.out.n, st_a)
        rc_b, tot_b = fetch(c, hb.ptr, len(d_b.container), 0, 3, bufs.streams2.buf, bufs.streams2.n, bufs.out2.buf, bufs.out2.n, st_b)
        sync()
    finally:
        c.set_variant(0, 0)
    assert (rc_a, tot_a, rc_b, tot_b) == (0, d_a.total, 0, d_b.total)
    assert int(st_a.item()) == 0 and int(st_b.item()) == 0
    bufs.streams.check(s_a.stream_pieces, "d_streams of the first call"); bufs.out.check(s_a.out_pieces, "d_out of the first call")
    bufs.streams2.check(s_b.stream_pieces, "d_streams of the second call"); bufs.out2.check(s_b.out_pieces, "d_out of the second call")
    count("fetch_back_to_back")


# ------------------------------------------------------------------------------------------------ 4. tsqa_decode_blocks_async

def decode_blocks(c, entry, d_arena, frames, fb, variant, remedy=True):
    """one call at `variant`; after TSQA_ERR_STALL once more at decode variant 4 -> status"""
    d_frames = to_dev(frames.view(np.uint8))
    st = None
    for v in (variant, 4):
        c.set_variant(0, v)
        try:
            c.decode_blocks_async(d_arena, d_frames, len(frames), fb.buf)
            sync()
            st = c.status()
        finally:
            c.set_variant(0, 0)
        if st != ERR_STALL or not remedy or v == 4:
            break
        stall(entry)
    return st


@pytest.fixture(scope="module")
def full_list(tsq):
    """every valid catalogue stream in one d_streams, at every residue mod 16, descriptors shuffled, destinations fenced"""
    named = shardgen.valid_blocks()
    blocks = [tuple(v[1:]) for v in named]
    arena, frames, outs, cap, order = shardgen.pack_for_decode(blocks, np.random.default_rng(41))
    assert {int(a) % 16 for a in frames["stream_at"]} == set(range(16)) and (np.diff(frames["out_at"].astype(np.int64)) < 0).any()
    pieces = [(at, blocks[b][2]) for (at, _), b in zip(outs, order)]
    return named, to_dev(arena), frames, pieces, Fenced(cap), order


@pytest.mark.parametrize("variant", shardgen.DECODE_VARIANTS)
def test_decode_blocks_of_the_whole_catalogue(tsq, codec, full_list, variant):
    named, d_arena, frames, pieces, fb, order = full_list
    fb.reset()
    st = decode_blocks(codec, f"decode_blocks_variant_{variant}", d_arena, frames, fb, variant)
    assert st == 0, (variant, st)
    fb.check(pieces, f"d_out of the whole catalogue at decode variant {variant}")
    count(f"decode_blocks_variant_{variant}", len(named))


def test_decode_blocks_at_every_launch_shape(tsq, codec):
    """block counts from the CU count: the default variant takes three workgroups per block, two, one, and full rounds with a tail
    of three and of two (launch_decode_kernels; the arithmetic of test_containers_of_uneven_blocks_at_every_launch_shape)"""
    import torch
    import streamgen
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    counts = {"three": max(6, cus // 3), "two": cus // 2, "one": cus - 5, "rounds_and_tail_of_three": cus + 7,
              "rounds_and_tail_of_two": cus + cus // 2 - 1}
    assert 3 * counts["three"] <= cus < 3 * counts["two"] and 2 * counts["two"] <= cus < 2 * counts["one"] and counts["one"] <= cus
    tail3, tail2 = counts["rounds_and_tail_of_three"] % cus, counts["rounds_and_tail_of_two"] % cus
    assert tail3 and 3 * tail3 <= cus and 2 * tail2 <= cus < 3 * tail2
    for shape, n in counts.items():
        blocks = streamgen.blocks_for(n)
        arena, frames, outs, cap, order = shardgen.pack_for_decode(blocks, np.random.default_rng(n))
        fb = Fenced(cap)
        st = decode_blocks(codec, "decode_blocks_launch_shapes", to_dev(arena), frames, fb, 0)
        assert st == 0, (shape, n, st)
        fb.check([(at, blocks[b][2]) for (at, _), b in zip(outs, order)], f"d_out of {n} blocks ({shape})")
        del fb
        count("decode_blocks_launch_shapes")


@pytest.mark.parametrize("variant", [1, 4, 6, 0])
def test_decode_blocks_with_a_twin_between_healthy_blocks(tsq, codec, variant):
    """Every invalid twin lies between two healthy blocks, in d_streams and in d_out.  Through this entry all of them are the
    decoder's to refuse (TSQA_ERR_STREAM): a stream of two bytes and a size word above 4 MiB by their descriptors.  Nothing outside
    the three destinations is written.

    Variants 1 and 4, one workgroup per block.  The verdict of a call is the call's: a workgroup looks at the status word once, at
    its start, and leaves if another block has reported by then (dec_serial_kernel, sym_decode_block); past that point it never
    looks again.  So each healthy destination holds either exactly its plain bytes or nothing but the sentinel, never a part, and
    the same descriptors without the twin give both blocks exactly.  That a healthy block beside a twin IS decoded depends on when
    its workgroup starts and is not promised; how many were is printed."""
    from streamgen import CATALOGUE
    healthy = CATALOGUE.valid["soup_5000_default_noext"]
    other = CATALOGUE.valid["last_match_clamped_second_ext"]
    rng = np.random.default_rng(variant)
    decoded = untouched = 0
    for name, ext, st, claimed in shardgen.twin_blocks():
        blocks = [healthy, (ext, st, bytes(claimed)), other]
        arena, frames, outs, cap, _ = shardgen.pack_for_decode(blocks, rng, shuffle=False)
        frames = frames[[0, 2, 1]].copy()                      # the twin's descriptor last
        fb = Fenced(cap)
        d_arena = to_dev(arena)
        got = decode_blocks(codec, f"decode_blocks_twins_variant_{variant}", d_arena, frames, fb, variant)
        assert got == ERR_STREAM, (name, variant, got)
        fb.check_outside(outs, f"d_out around {name} at decode variant {variant}")
        if variant in (1, 4):
            back = fb.buf.cpu().numpy()
            guard = fb.master.cpu().numpy()
            for (at, ln), (_, _, plain) in ((outs[0], healthy), (outs[2], other)):
                exact = bytes(back[at:at + ln]) == plain
                assert exact or np.array_equal(back[at:at + ln], guard[at:at + ln]), (name, variant, "a healthy block beside the twin was written in part")
                decoded += exact
                untouched += not exact
            # the same two descriptors without the twin
            fb.reset()
            got = decode_blocks(codec, f"decode_blocks_twins_variant_{variant}", d_arena, frames[:2].copy(), fb, variant)
            assert got == 0, (name, variant, got)
            fb.check([(outs[0][0], healthy[2]), (outs[2][0], other[2])], f"d_out around {name} without it at decode variant {variant}")
        count(f"decode_blocks_twins_variant_{variant}")
    if variant in (1, 4):
        print(f"decode variant {variant}: {decoded} healthy blocks beside a twin decoded, {untouched} left untouched")


def test_decode_blocks_does_not_trust_its_descriptors(tsq, codec):
    """stream_len 0, 2 and TSQ_OUTPUT_SZ + 1 and out_len TSQ_BLOCK_SZ + 1 are refused with nothing written; an out_len below the
    stream's own size word writes nothing past out_at + out_len.  stream_at and out_at always lie inside the buffers (the header
    leaves those to the caller)."""
    from streamgen import CATALOGUE
    rng = np.random.default_rng(8)
    ext, stream, plain = CATALOGUE.valid["soup_5000_default_noext"]
    arena = shardgen.filler(rng, OUTPUT_SZ + 64)
    arena[7:7 + len(stream)] = as_u8(stream)
    d_arena = to_dev(arena)
    fb = Fenced(BLOCK + 256)
    n = 0
    for stream_len, out_len in ((0, len(plain)), (2, len(plain)), (OUTPUT_SZ + 1, len(plain)), (len(stream), BLOCK + 1)):
        for variant in (1, 4, 6, 5, 0):
            frames = np.zeros(1, dtype=FRAME_DTYPE)
            frames[0] = (7, 33, stream_len, ext, out_len, 0)
            fb.reset()
            st = decode_blocks(codec, "decode_blocks_trust", d_arena, frames, fb, variant)
            assert st == ERR_STREAM, (stream_len, out_len, variant, st)
            fb.check([], f"d_out after a refused descriptor (stream_len {stream_len}, out_len {out_len}, variant {variant})")
            n += 1
    # out_len below the size word
    names = ["soup_5000_default_noext", "soup_200000_default_ext", "chain_of_6000_pairs_noext", "last_match_clamped_first_ext",
             "match64_groups_cut_by_image_budget_ext", "block_of_17_bytes_noext"]
    ok = serial = 0
    for name in names:
        ext, stream, plain = CATALOGUE.valid[name]
        arena = shardgen.filler(rng, len(stream) + 64)
        arena[5:5 + len(stream)] = as_u8(stream)
        d_arena = to_dev(arena)
        fb = Fenced(len(plain) + 256)
        for cut in sorted({1, 7, len(plain) // 2, len(plain) - 1, len(plain)}):
            out_len = len(plain) - cut
            for variant in (1, 4, 6, 0):
                frames = np.zeros(1, dtype=FRAME_DTYPE)
                frames[0] = (5, 41, len(stream), ext, out_len, 0)
                fb.reset()
                st = decode_blocks(codec, "decode_blocks_trust", d_arena, frames, fb, variant)
                assert st in (0, ERR_STREAM), (name, cut, variant, st)
                if variant == 1:
                    # the serial decoder stops at out_len and has nothing to refuse in a valid stream's prefix
                    assert st == 0, (name, cut, st)
                    serial += 1
                fb.check_outside([(41, out_len)], f"d_out of {name} with out_len {out_len} at decode variant {variant}")
                if st == 0:
                    fb.check([(41, plain[:out_len])], f"d_out of {name} with out_len {out_len} at decode variant {variant}")
                    ok += 1
                n += 1
    print(f"out_len below the size word: {ok} calls accepted (the bytes were the plain's prefix)")
    assert serial >= 24 and ok >= serial
    count("decode_blocks_trust", n)


# ------------------------------------------------------------------------------------------------ 5. tsqa_encode_blocks_async

_DEV: dict = {}


def cached(key, make):
    if key not in _DEV:
        _DEV[key] = make()
    return _DEV[key]


def encode_call(codec, call, ext, want, variant, slots, sizes_guard, out, entry):
    """one tsqa_encode_blocks_async call, straight into tsqa_decode_blocks_async of the result, one wait: every stream and size is
    the oracle's, every slot is fenced at its end, d_sizes behind n_blocks entries, and the decode gives the input back"""
    import torch
    nb = call.n_blocks
    d_in = cached(("in", call.name, call.stride), lambda: to_dev(call.buffer))
    slots.reset()
    d_sizes = sizes_guard.clone()
    frames = np.zeros(nb, dtype=FRAME_DTYPE)
    datas = call.datas()
    for b in range(nb):
        frames[b] = (b * OUTPUT_SZ, b * BLOCK, len(want[b]), ext, len(datas[b]), 0)
    d_frames = to_dev(frames.view(np.uint8))
    out.reset()                                    # (waits: d_sizes and the descriptors are in place too)
    codec.set_variant(variant, 0)
    try:
        codec.encode_blocks_async(d_in, nb, call.stride, call.last_len, ext, slots.buf, d_sizes)
        sync()
        st = codec.status()
        codec.decode_blocks_async(slots.buf, d_frames, nb, out.buf)
        sync()
        dst = codec.status()
        if dst == ERR_STALL:
            stall(entry)
            codec.set_variant(variant, 4)
            codec.decode_blocks_async(slots.buf, d_frames, nb, out.buf)
            sync()
            dst = codec.status()
    finally:
        codec.set_variant(0, 0)
    what = f"{call.name} (stride BLOCK + {call.stride - BLOCK}) ext {ext} encoder variant {variant}"
    assert st == 0, (what, st)
    got = d_sizes.cpu().numpy()
    assert got[:nb].tolist() == [len(w) for w in want], (what, got[:nb].tolist(), [len(w) for w in want])
    assert np.array_equal(got[nb:], sizes_guard.cpu().numpy()[nb:]), (what, "d_sizes was written behind n_blocks entries")
    for b in range(nb):
        w = cached(("want", call.name, call.stride, ext, b), lambda: to_dev(as_u8(want[b])))
        lo = b * OUTPUT_SZ
        if not torch.equal(slots.buf[lo:lo + len(want[b])], w):
            first = int(torch.nonzero(slots.buf[lo:lo + len(want[b])] != w)[0])
            pytest.fail(f"{what}: block {b} differs from the oracle's stream at offset {first} of {len(want[b])}")
    # (bytes behind sizes[b] may hold the documented over-store: the fence is at the slot's end)
    slots.check_outside([(b * OUTPUT_SZ, OUTPUT_SZ) for b in range(nb)], "d_slots of " + what)
    assert dst == 0, (what, dst)
    out.check([(b * BLOCK, datas[b]) for b in range(nb)], "the decode of " + what)


@pytest.fixture(scope="module")
def enc_bufs(tsq):
    import torch
    class B:
        slots1, out1 = Fenced(OUTPUT_SZ + FENCE), Fenced(BLOCK + FENCE)
        slots3, out3 = Fenced(3 * OUTPUT_SZ + FENCE), Fenced(3 * BLOCK + FENCE)
        sizes = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    return B


@pytest.fixture(scope="module")
def wanted(oracle):
    memo = {}

    def get(call, ext):
        key = (call.name, call.stride, ext)
        if key not in memo:
            memo[key] = call.want(oracle, ext)
        return memo[key]
    return get


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("variant", shardgen.ENC_VARIANTS)
def test_encode_blocks_of_every_one_block_case(tsq, codec, enc_bufs, wanted, variant, ext):
    """1: the serial encoder; 7: the staged encoder's standard layout; 6: its lean layout; 0: the library's own choice.  Every case
    at stride BLOCK + 128, its halo directly behind last_len and filler behind the halo"""
    for case in shardgen.one_block_cases():
        call = cached(("call", case.name, BLOCK + 128), lambda: shardgen.encode_one_block(case))
        entry = f"encode_variant_{variant}_ext_{ext}"
        encode_call(codec, call, ext, wanted(call, ext), variant, enc_bufs.slots1, enc_bufs.sizes, enc_bufs.out1, entry)
        count(entry)


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("variant", shardgen.ENC_VARIANTS)
def test_encode_blocks_at_strides_between_block_and_block_plus_128(tsq, codec, enc_bufs, wanted, variant, ext):
    """stride BLOCK + 5 and BLOCK + 127, the cases that carry a halo: the block sees stride - BLOCK look-ahead bytes, then zeros,
    although filler follows them"""
    for case in shardgen.one_block_cases():
        if case.halo is None:
            continue
        for stride in shardgen.ODD_STRIDES:
            call = cached(("call", case.name, stride), lambda: shardgen.encode_one_block(case, stride))
            entry = f"encode_odd_stride_variant_{variant}_ext_{ext}"
            encode_call(codec, call, ext, wanted(call, ext), variant, enc_bufs.slots1, enc_bufs.sizes, enc_bufs.out1, entry)
            count(entry)


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("variant", shardgen.ENC_VARIANTS)
def test_encode_blocks_of_three_blocks_at_every_stride(tsq, codec, enc_bufs, wanted, variant, ext):
    """stride BLOCK: a block sees the next block's own bytes and the last one zeros, although filler follows; BLOCK + 128: the
    documented look-ahead; BLOCK + 128 + 4096 + 1: the same bytes at unaligned block starts, filler behind them"""
    for name, cases in shardgen.arrangements().items():
        for stride in shardgen.STRIDES:
            call = cached(("arr", name, stride), lambda: shardgen.encode_arrangement(name, cases, stride))
            entry = f"encode_arrangements_variant_{variant}_ext_{ext}"
            encode_call(codec, call, ext, wanted(call, ext), variant, enc_bufs.slots3, enc_bufs.sizes, enc_bufs.out3, entry)
            count(entry)


# ------------------------------------------------------------------------------------------------ the counts

def test_every_case_ran_and_the_counts_are_the_goldens(tables):
    g = GOLDEN["counts"]
    assert g == json.loads(json.dumps(shardgen.counts())) | {"place_triples": g["place_triples"]}
    want = {"place": g["place_triples"], "frames_to_host": g["place_triples"], "frames_from_host": g["place_triples"],
            "fetch_owning_nothing": len(shardgen.FETCH_VARIANTS) * g["deal_triples_owning_nothing"],
            "fetch_capacities": g["deal_triples"] - g["deal_triples_owning_nothing"], "fetch_damage": g["damage_triples"],
            "fetch_back_to_back": 1, "decode_blocks_launch_shapes": 5}
    want.update({f"fetch_variant_{v}": g["deal_triples"] for v in shardgen.FETCH_VARIANTS})
    want.update({f"decode_blocks_variant_{v}": g["decode_valid"] for v in shardgen.DECODE_VARIANTS})
    want.update({f"decode_blocks_twins_variant_{v}": g["decode_twins"] for v in (1, 4, 6, 0)})
    for v in shardgen.ENC_VARIANTS:
        for e in (0, 1):
            want[f"encode_variant_{v}_ext_{e}"] = g["encode_one_block"]
            want[f"encode_odd_stride_variant_{v}_ext_{e}"] = len(shardgen.ODD_STRIDES) * g["encode_one_block_with_halo"]
            want[f"encode_arrangements_variant_{v}_ext_{e}"] = g["encode_arrangements"]
    print("shard conformance counts:", dict(sorted(COUNTS.items())))
    print("stalls:", sum(STALLS.values()), dict(sorted(STALLS.items())))
    assert {k: COUNTS.get(k, 0) for k in want} == want
    # the refusals, from the tables: per (table, world 1..3, rank) a short host_cap, and two bad sizes where another rank owns a block;
    # per (table, world 1..2, rank that owns two blocks or more) three bad sizes; four bad descriptors at five variants and the
    # 30 (stream, out_len) pairs at four
    place = sum(1 + 2 * any(b % w != r for b in range(t.nb)) for t in tables for w in (1, 2, 3) for r in range(w))
    copies = sum(3 for t in tables for w in (1, 2) for r in range(w) if len(t.owned(w, r)) >= 2)
    assert (COUNTS.get("place_refusals"), COUNTS.get("frame_copy_refusals"), COUNTS.get("decode_blocks_trust")) == (place, copies, 4 * 5 + 30 * 4)
