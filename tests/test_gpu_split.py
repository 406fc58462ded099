"""GPU tests of the short-block entry points (tsqa_compress_device_split*, tsqa_decompress_device_sized*): the container and the size
table are splitgen.expected_split's, made with the oracle; every buffer the library writes is filled with a sentinel first and must
keep it wherever the call owes nothing; the sized decompress is held against tsqa_decompress_device_async on the same container."""
import ctypes as C

import numpy as np
import pytest

import mtgen
import splitgen as sg
import streamgen

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_FORMAT, ERR_OVERFLOW = 0, sg.ERR_ARG, sg.ERR_FORMAT, sg.ERR_OVERFLOW
FENCE = 4096


@pytest.fixture(scope="module")
def tsq():
    import torch
    assert torch.cuda.is_available()
    import turbosqueeze_amd
    return turbosqueeze_amd


@pytest.fixture(scope="module")
def codec(tsq):
    c = tsq.DeviceCodec(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def default_variants(codec):
    codec.set_variant(0, 0)
    yield
    codec.set_variant(0, 0)


@pytest.fixture(scope="module")
def budget():
    """B: the blocks of one encode launch, 2 x CUs"""
    import torch
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(n):
    """((i * 37 + 11) % 251) ^ 0xA5 at byte i (the pattern repeats every 251 bytes)"""
    return np.resize(((np.arange(251, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5, n)


TABLE_GUARD = 0x5EA1ED


class Input:
    """an input on the device with non-zero bytes behind it (the look-ahead past n must see zeros all the same), and what the
    library owes for its prefixes, made once per (n, block_len, ext)"""

    def __init__(self, data, oracle):
        self.data, self.oracle, self._want = data, oracle, {}
        self.dev = to_dev(np.concatenate([data, sentinel(256) | 1]))

    def want(self, n, block_len, ext):
        key = (n, block_len, ext)
        if key not in self._want:
            self._want[key] = sg.expected_split(self.oracle, self.data[:n], block_len, ext)
        return self._want[key]


def split_call(codec, inp, n, block_len, ext, out_cap, table=True):
    """tsqa_compress_device_split of the first n bytes into out_cap bytes of a sentinel-filled buffer with a fence behind them
    -> (buffer, guard, *out_size, table without its fence or None, rc)"""
    nb = -(-n // block_len)
    guard = sentinel(out_cap + FENCE)
    out = to_dev(guard)
    tab = to_dev(np.full(nb + 16, TABLE_GUARD, dtype=np.int32)) if table else None
    size = C.c_size_t(0)
    rc = codec.L.tsqa_compress_device_split(codec.h, inp.dev.data_ptr(), n, block_len, out.data_ptr(), out_cap, C.byref(size),
                                            tab.data_ptr() if table else None, ext, codec._stream())
    got = None
    if table:
        host = tab.cpu().numpy()
        assert (host[nb:] == TABLE_GUARD).all(), "the size table was written past n_blocks words"
        got = [int(x) for x in host[:nb]]
        # (the copy behind the scan moves streams of at most block_bound's length whole: a longer one would be cut)
        assert rc != OK or max(got) <= sg.block_bound(block_len) - sg.WORD, "a stream longer than block_bound"
    return out.cpu().numpy(), guard, int(size.value), got, rc


def check_exact(codec, inp, n, block_len, ext):
    """the whole container and the table, in exactly the room tsqa_plan_split states, and nothing written behind the container"""
    import turbosqueeze_amd as tsq
    blob, sizes = inp.want(n, block_len, ext)
    nb, bound = tsq.plan_split(n, block_len)
    host, guard, size, table, rc = split_call(codec, inp, n, block_len, ext, bound)
    assert rc == OK, codec.last_error()
    assert size == len(blob) and table == sizes and nb == len(sizes)
    assert host[:size].tobytes() == blob, f"n {n}, block_len {block_len}: not the expected container"
    assert np.array_equal(host[size:], guard[size:]), "bytes behind the container were written"
    return host[:size]


VARIANTS = [0, 6, 7]


@pytest.fixture(scope="module")
def counts(oracle, budget):
    return Input(sg.count_input(budget), oracle)


@pytest.fixture(scope="module")
def carry(oracle):
    data, bl = sg.carry_input()
    return Input(data, oracle), bl


# ---- compress ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ext", [0, 1])
def test_block_counts(codec, counts, budget, ext, variant):
    """block_len 4096 and 1, 2, 255, 256, 257, B - 1, B, B + 1 and 2B + 1 blocks, the last of 1 byte, of 4095 and full: one pass
    of the scan and several, one launch and three, the carry between launches"""
    codec.set_variant(variant, 0)
    for nb, n in sg.count_cases(budget):
        check_exact(codec, counts, n, 4096, ext)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ext", [0, 1])
def test_offsets_cross_2_to_24_inside_a_pass(codec, carry, budget, ext, variant):
    inp, bl = carry
    codec.set_variant(variant, 0)
    assert sg.carry_crossing(inp.want(inp.data.size, bl, ext)[1], budget), "the case does not reach its aim on this device"
    check_exact(codec, inp, inp.data.size, bl, ext)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ext", [0, 1])
def test_at_4_mib_it_is_the_plain_container(codec, oracle, ext, variant):
    inp = Input(sg.mixed((1 << 22) + 5, 7), oracle)
    codec.set_variant(variant, 0)
    got = check_exact(codec, inp, inp.data.size, 1 << 22, ext)
    plain = codec.compress(inp.dev[:inp.data.size], ext).cpu().numpy()
    assert got.tobytes() == plain.tobytes()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("ext", [0, 1])
def test_matches_across_every_block_edge(codec, oracle, ext, variant):
    data, bl = sg.edge_input()
    codec.set_variant(variant, 0)
    check_exact(codec, Input(data, oracle), data.size, bl, ext)


@pytest.mark.parametrize("ext", [0, 1])
def test_without_a_table_and_through_the_python_face(codec, tsq, oracle, ext):
    data = sg.mixed(300_001, 10)
    inp = Input(data, oracle)
    blob, sizes = inp.want(data.size, 1 << 14, ext)
    host, guard, size, _, rc = split_call(codec, inp, data.size, 1 << 14, ext, len(blob) + 100, table=False)
    assert rc == OK and host[:size].tobytes() == blob and np.array_equal(host[size:], guard[size:])
    src = inp.dev[:data.size]
    got, table = codec.compress_split(src, ext, 1 << 14, block_sizes=True)
    assert got.cpu().numpy().tobytes() == blob and table.cpu().tolist() == sizes
    assert codec.compress_split(src, ext, 1 << 14).cpu().numpy().tobytes() == blob
    assert codec.decompress_sized(got, table).cpu().numpy().tobytes() == data.tobytes()
    import torch
    small = torch.empty(len(blob) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(tsq.TsqError) as e:
        codec.compress_split(src, ext, 1 << 14, out=small)
    assert e.value.code == ERR_OVERFLOW and e.value.needed == len(blob)
    bad = table.clone()
    bad[3] += 1
    with pytest.raises(tsq.TsqError) as e:
        codec.decompress_sized(got, bad)
    assert e.value.code == ERR_FORMAT


@pytest.mark.parametrize("ext", [0, 1])
def test_every_existing_reader_takes_a_split_container(codec, oracle, ext):
    data = sg.mixed(300_001, 10)
    bl = 1 << 14
    blob = codec.compress_split(to_dev(data), ext, bl)
    assert blob.cpu().numpy().tobytes() == Input(data, oracle).want(data.size, bl, ext)[0]
    assert codec.decompress(blob).cpu().numpy().tobytes() == data.tobytes()
    other = codec.compress(to_dev(data[:5000]), ext)
    views = codec.decompress_batch([other, blob, other])
    assert views[1].cpu().numpy().tobytes() == data.tobytes() and views[0].cpu().numpy().tobytes() == data[:5000].tobytes()
    idx = codec.index(blob)
    assert idx.n_blocks == -(-data.size // bl) and idx.total == data.size
    for off, ln in ((bl - 100, 200), (3 * bl - 1, 2), (5 * bl - 7, 2 * bl + 14), (data.size - 50, 50)):
        assert idx.read(off, ln).cpu().numpy().tobytes() == data[off:off + ln].tobytes(), (off, ln)
    idx.close()


# ---- room --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ext", [0, 1])
def test_room(codec, counts, budget, ext):
    """out_cap: the size needed; one byte less; a cut in the middle of a frame of the second launch; the least the call takes.  The
    frames that end at or before out_cap are exact, nothing else is written, the size needed and the table are complete."""
    nb = budget + 5
    n = nb * 4096 - 17
    blob, sizes = counts.want(n, 4096, ext)
    at = sg.frame_places(sizes)
    need = at[-1]
    assert len(sg.launches(nb, budget)) == 2
    for cap in (need, need - 1, at[budget + 2] + sg.WORD + sizes[budget + 2] // 2, sg.HEADER + sg.MIN_FRAME * nb):
        host, guard, size, table, rc = split_call(codec, counts, n, 4096, ext, cap)
        want, want_size, want_rc = sg.pack_cut(blob, sizes, cap, guard)
        assert rc == want_rc == (OK if cap == need else ERR_OVERFLOW), (cap, rc, codec.last_error())
        assert size == want_size == need and table == sizes
        assert np.array_equal(host[cap:], guard[cap:]), f"out_cap {cap}: the fence behind it was written"
        assert np.array_equal(host, want), f"out_cap {cap}: not the frames that fit, or more than them"
        # the retry with the room the call asked for
        host, guard, size, table, rc = split_call(codec, counts, n, 4096, ext, size)
        assert rc == OK and host[:size].tobytes() == blob and np.array_equal(host[size:], guard[size:]) and table == sizes


def test_refusals_write_nothing(codec, counts):
    import torch
    L, n, bl = codec.L, 40_000, 4096
    nb = -(-n // bl)
    guard = sentinel(100_000)

    def call(d_in=True, n=n, bl=bl, d_out=True, cap=100_000, d_size=True, d_status=True):
        out, tab = to_dev(guard), to_dev(np.full(nb + 16, TABLE_GUARD, dtype=np.int32))
        size, status = torch.full((1,), 777, dtype=torch.int64, device="cuda"), torch.full((1,), 55, dtype=torch.int32, device="cuda")
        rc = L.tsqa_compress_device_split_async(codec.h, counts.dev.data_ptr() if d_in else None, n, bl, out.data_ptr() if d_out else None, cap,
                                                size.data_ptr() if d_size else None, tab.data_ptr(), status.data_ptr() if d_status else None,
                                                0, codec._stream())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), guard) and (tab.cpu().numpy() == TABLE_GUARD).all()
        assert int(size.item()) == 777 and int(status.item()) == 55
        return rc

    assert call(n=0) == ERR_ARG
    for bad in (0, 1, 2048, 4097, 12288, 1 << 23, 0xFFFFFFFF):
        assert call(bl=bad) == ERR_ARG, bad
    assert call(n=1 << 44, bl=4096, cap=1 << 40) == ERR_ARG          # 2^32 blocks
    assert call(d_in=False) == ERR_ARG and call(d_out=False) == ERR_ARG and call(d_size=False) == ERR_ARG and call(d_status=False) == ERR_ARG
    assert call(cap=sg.HEADER + sg.MIN_FRAME * nb - 1) == ERR_ARG
    for v in (1, 2, 5):
        codec.set_variant(v, 0)
        assert call() == ERR_ARG, v
    codec.set_variant(0, 0)
    size = C.c_size_t(0)
    assert L.tsqa_compress_device_split(codec.h, counts.dev.data_ptr(), n, bl, to_dev(guard).data_ptr(), 100_000, None, None, 0,
                                        codec._stream()) == ERR_ARG
    assert L.tsqa_compress_device_split(None, counts.dev.data_ptr(), n, bl, to_dev(guard).data_ptr(), 100_000, C.byref(size), None, 0,
                                        None) == ERR_ARG


# ---- sized decompress ------------------------------------------------------------------------------------------------------------------

def decode_pair(codec, blob, n, n_blocks, table, out_cap):
    """tsqa_decompress_device_async and tsqa_decompress_device_sized_async on the first n bytes of blob, each into out_cap bytes of
    its own sentinel-filled, fenced buffer -> ((rc, status, size, buffer) of the plain call, the same of the sized call, guard).
    The container lies at the very end of its allocation."""
    import torch
    raw = np.frombuffer(bytes(blob[:n]), dtype=np.uint8)
    d_in = to_dev(raw) if n else torch.empty(1, dtype=torch.uint8, device="cuda")
    d_tab = to_dev(np.array([int(x) for x in table] or [0], dtype=np.uint32).view(np.int32))
    guard = sentinel(out_cap + FENCE)
    res = []
    for sized in (False, True):
        out = to_dev(guard)
        size, status = torch.full((1,), 777, dtype=torch.int64, device="cuda"), torch.full((1,), 55, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()         # (the call runs on the context's own stream, which does not wait for torch's fills)
        if sized:
            rc = codec.L.tsqa_decompress_device_sized_async(codec.h, d_in.data_ptr(), n, n_blocks, d_tab.data_ptr(), out.data_ptr(), out_cap,
                                                            size.data_ptr(), status.data_ptr(), codec._stream())
        else:
            rc = codec.L.tsqa_decompress_device_async(codec.h, d_in.data_ptr(), n, n_blocks, out.data_ptr(), out_cap, size.data_ptr(),
                                                      status.data_ptr(), codec._stream())
        torch.cuda.synchronize()
        res.append((rc, int(status.item()), int(size.item()), out.cpu().numpy()))
    return res[0], res[1], guard


def walk_table(L, blob):
    """tsqa_walk_frames on the host -> (the block count to state, the stream sizes as far as the walk came, zeros behind)"""
    n = len(blob)
    stated = int.from_bytes(blob[4:8], "little") if n >= 8 else 0
    cap = max(1, min(stated, 1 << 12))
    frame_at, sizes, ext, out_len = (C.c_uint64 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    nb, total = C.c_uint32(0), C.c_uint64(0)
    raw = np.frombuffer(blob, dtype=np.uint8)
    L.tsqa_walk_frames(raw.ctypes.data, n, cap, frame_at, sizes, ext, out_len, C.byref(nb), C.byref(total))
    return cap, [int(x) for x in sizes]


def same_as_plain(codec, name, blob):
    """the contract for a true table: return value, status, size and output are the plain call's, whatever the container is.
    Behind a decoder's refusal (TSQA_ERR_STREAM) the output holds what the other blocks' workgroups wrote before they saw the status
    word, which two runs of the SAME call do not share: there the two outputs are held to the fence, not to each other -- but for
    a container of ONE block, which both calls then decode once more with one workgroup per block (decode variant 4): nobody races
    that workgroup, and what it wrote before it refused must be the same bytes."""
    n = len(blob)
    nb, table = walk_table(codec.L, blob)
    stated = int.from_bytes(blob[8:16], "little") if n >= 16 else 0
    out_cap = stated if 0 < stated <= (64 << 20) else 64
    plain, sized, guard = decode_pair(codec, blob, n, nb, table, out_cap)
    assert plain[:3] == sized[:3], f"{name}: plain {plain[:3]}, sized {sized[:3]}"
    for r in (plain, sized):
        assert np.array_equal(r[3][out_cap:], guard[out_cap:]), f"{name}: the fence behind out_cap was written"
    if plain[1] in (OK, ERR_FORMAT) or plain[0] != OK:
        assert np.array_equal(plain[3], sized[3]), f"{name}: outputs differ"
    if plain[0] != OK or plain[1] == ERR_FORMAT:
        assert np.array_equal(sized[3], guard), f"{name}: a refused container was decoded"
    elif plain[1] != OK and nb == 1:
        codec.set_variant(0, 4)
        plain4, sized4, _ = decode_pair(codec, blob, n, nb, table, out_cap)
        codec.set_variant(0, 0)
        assert plain4[:3] == sized4[:3] == plain[:3], f"{name}: one workgroup per block: plain {plain4[:3]}, sized {sized4[:3]}"
        assert np.array_equal(plain4[3], sized4[3]), f"{name}: one workgroup per block: outputs differ"
    return plain[0], plain[1], plain[2]


@pytest.mark.parametrize("ext", [0, 1])
def test_sized_true_tables_over_the_split_cases(codec, counts, carry, budget, ext):
    cases = [(counts, n, 4096) for nb, n in sg.count_cases(budget)]
    cases.append((carry[0], carry[0].data.size, carry[1]))
    edge, edge_len = sg.edge_input()
    cases += [(Input(edge, counts.oracle), edge.size, edge_len), (Input(sg.mixed((1 << 22) + 5, 7), counts.oracle), (1 << 22) + 5, 1 << 22)]
    for inp, n, bl in cases:
        blob, sizes = inp.want(n, bl, ext)
        plain, sized, guard = decode_pair(codec, blob, len(blob), len(sizes), sizes, n)
        assert sized[:3] == (OK, OK, n) == plain[:3], (n, bl, sized[:3], plain[:3])
        assert sized[3][:n].tobytes() == inp.data[:n].tobytes() and np.array_equal(sized[3][n:], guard[n:])
        assert np.array_equal(plain[3], sized[3])


def test_sized_equals_plain_on_the_stream_catalogue(codec):
    """every valid stream of streamgen's catalogue as a container of its own, and every invalid twin"""
    for name, block in streamgen.CATALOGUE.valid.items():
        rc, st, size = same_as_plain(codec, name, streamgen.container([block]))
        assert (rc, st, size) == (OK, OK, len(block[2])), name
    for name, (ext, stream) in streamgen.CATALOGUE.invalid.items():
        # (what a one-block container around it is refused with: the walk refuses a stream shorter than its size word or a block
        #  over 4 MiB, tsq_format.h read_frame; everything else is the block decoder's to find)
        want = ERR_FORMAT if len(stream) < 3 or int.from_bytes(stream[:3], "little") > streamgen.BLOCK else 5
        assert same_as_plain(codec, name, streamgen.bad_container(ext, stream))[:2] == (OK, want), name


def test_sized_equals_plain_on_the_scheduler_catalogue(codec):
    """mtgen's containers of many uneven blocks, and its twins: an invalid stream among five healthy ones"""
    for name, blob, plain, _ in mtgen.ramp_containers():
        assert same_as_plain(codec, name, blob) == (OK, OK, len(plain)), name
    for name, blob, k, where in mtgen.twin_containers():
        rc, st, _ = same_as_plain(codec, name, blob)
        assert rc == OK and st != OK and (st == ERR_FORMAT) == (where == "walk"), (name, st, where)


def test_sized_equals_plain_on_damaged_and_cut_containers(codec):
    seen = set()
    for name, blob in mtgen.damaged_containers():
        seen.add(same_as_plain(codec, name, blob)[:2])
    assert (OK, OK) in seen and (OK, ERR_FORMAT) in seen and (ERR_ARG, 55) in seen      # (cut_in_header: refused before anything is enqueued)


def test_a_header_count_that_is_not_the_tables_is_refused_by_the_waiting_form(codec, tsq, counts):
    """tsqa_decompress_device_sized reads the header itself, but the table is as long as the CALLER says: a container whose header
    states more blocks than the table holds (a damaged blob, or the wrong blob for the table) is TSQA_ERR_FORMAT before anything is
    enqueued, so no kernel reads the table past its end.  The table lies at the very end of its allocation."""
    import torch
    n = 40 * 4096 - 5
    blob, sizes = counts.want(n, 4096, 1)
    nb = len(sizes)
    guard = sentinel(n + FENCE)

    def call(container, table, words):
        d_in, d_tab, out = to_dev(np.frombuffer(container, dtype=np.uint8)), to_dev(np.array(table, dtype=np.uint32).view(np.int32)), to_dev(guard)
        size = C.c_size_t(12345)
        torch.cuda.synchronize()
        rc = codec.L.tsqa_decompress_device_sized(codec.h, d_in.data_ptr(), len(container), words, d_tab.data_ptr(), out.data_ptr(), n,
                                                  C.byref(size), codec._stream())
        torch.cuda.synchronize()
        return rc, int(size.value), out.cpu().numpy()

    rc, size, host = call(blob, sizes, nb)
    assert (rc, size) == (OK, n) and host[:n].tobytes() == counts.data[:n].tobytes() and np.array_equal(host[n:], guard[n:])
    more = blob[:4] + (nb + 1000).to_bytes(4, "little") + blob[8:]          # (plausible for the container's size: 6 bytes a frame)
    assert nb + 1000 <= (len(blob) - 16) // 6
    for container, table, words in ((more, sizes, nb), (blob, sizes[:7], 7), (blob, sizes[:nb - 1], nb - 1), (blob, sizes + [3], nb + 1)):
        rc, size, host = call(container, table, words)
        assert (rc, size) == (ERR_FORMAT, 0), (words, rc, size, codec.last_error())
        assert np.array_equal(host, guard), "a refused call wrote to the output"
    rc, size, host = call(blob, sizes, 0)
    assert rc == ERR_ARG and size == 12345 and np.array_equal(host, guard)
    # the Python face states the table's own length, and refuses what is no table
    d_blob, d_more = to_dev(np.frombuffer(blob, dtype=np.uint8)), to_dev(np.frombuffer(more, dtype=np.uint8))
    d_tab = to_dev(np.array(sizes, dtype=np.int32))
    assert codec.decompress_sized(d_blob, d_tab).cpu().numpy().tobytes() == counts.data[:n].tobytes()
    for b, t, code in ((d_more, d_tab, ERR_FORMAT), (d_blob, d_tab[:7].clone(), ERR_FORMAT), (d_blob, d_tab.to(torch.int64), ERR_ARG),
                       (d_blob, d_tab.to(torch.uint8), ERR_ARG), (d_blob, d_tab.cpu(), ERR_ARG), (d_blob, d_tab[::2], ERR_ARG)):
        with pytest.raises(tsq.TsqError) as e:
            codec.decompress_sized(b, t)
        assert e.value.code == code
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    with pytest.raises(tsq.TsqError) as e:
        codec.decompress_sized_async(d_blob, nb, d_tab[:7].clone(), out)
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("ext", [0, 1])
def test_false_tables_are_refused_and_nothing_is_decoded(codec, carry, ext):
    inp, bl = carry
    n = inp.data.size
    blob, sizes = inp.want(n, bl, ext)
    out_cap = n + 64
    for name, c, cn, table in sg.false_tables(blob, sizes):
        assert sg.sized_refuses(c, cn, table, len(sizes), out_cap), name
        _, sized, guard = decode_pair(codec, c, cn, len(sizes), table, out_cap)
        assert sized[:3] == (OK, ERR_FORMAT, 0), (name, sized[:3])
        assert np.array_equal(sized[3][out_cap:], guard[out_cap:]), f"{name}: written behind out_cap"
        assert np.array_equal(sized[3], guard), f"{name}: a refused container was decoded"


@pytest.mark.parametrize("ext", [0, 1])
def test_chain_on_one_stream_without_a_wait(codec, tsq, oracle, ext):
    """split compress -> sized decompress -> split compress at another block_len, enqueued back to back on one stream: the size
    table never leaves the device, and the decompress is told the container's room, not its size (what lies behind the last frame
    is not looked at)."""
    import torch
    data = sg.mixed(700_003, 11)
    inp = Input(data, oracle)
    n, bl_a, bl_b = data.size, 1 << 13, 1 << 16
    (nb_a, bound_a), (nb_b, bound_b) = tsq.plan_split(n, bl_a), tsq.plan_split(n, bl_b)
    want_a, want_b = inp.want(n, bl_a, ext), inp.want(n, bl_b, ext)
    i32 = lambda k, v: torch.full((k,), v, dtype=torch.int32, device="cuda")
    i64 = lambda v: torch.full((1,), v, dtype=torch.int64, device="cuda")
    out_a, out_b, back = to_dev(sentinel(bound_a + FENCE)), to_dev(sentinel(bound_b + FENCE)), to_dev(sentinel(n + FENCE))
    tab_a, tab_b = i32(nb_a + 16, TABLE_GUARD), i32(nb_b + 16, TABLE_GUARD)
    sizes, status = [i64(777) for _ in range(3)], [i32(1, 55) for _ in range(3)]
    L, s = codec.L, torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        h = C.c_void_p(s.cuda_stream)
        rcs = [L.tsqa_compress_device_split_async(codec.h, inp.dev.data_ptr(), n, bl_a, out_a.data_ptr(), bound_a, sizes[0].data_ptr(),
                                                  tab_a.data_ptr(), status[0].data_ptr(), ext, h),
               L.tsqa_decompress_device_sized_async(codec.h, out_a.data_ptr(), bound_a, nb_a, tab_a.data_ptr(), back.data_ptr(), n,
                                                    sizes[1].data_ptr(), status[1].data_ptr(), h),
               L.tsqa_compress_device_split_async(codec.h, back.data_ptr(), n, bl_b, out_b.data_ptr(), bound_b, sizes[2].data_ptr(),
                                                  tab_b.data_ptr(), status[2].data_ptr(), ext, h)]
    s.synchronize()
    assert rcs == [OK] * 3, codec.last_error()
    assert [int(x.item()) for x in status] == [OK] * 3
    assert [int(x.item()) for x in sizes] == [len(want_a[0]), n, len(want_b[0])]
    for out, tab, (blob, table), bound in ((out_a, tab_a, want_a, bound_a), (out_b, tab_b, want_b, bound_b)):
        host, t = out.cpu().numpy(), tab.cpu().numpy()
        assert host[:len(blob)].tobytes() == blob and np.array_equal(host[len(blob):], sentinel(bound + FENCE)[len(blob):])
        assert t[:len(table)].tolist() == table and (t[len(table):] == TABLE_GUARD).all()
    host = back.cpu().numpy()
    assert host[:n].tobytes() == data.tobytes() and np.array_equal(host[n:], sentinel(n + FENCE)[n:])
