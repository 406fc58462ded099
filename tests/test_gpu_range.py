"""GPU tests of range reads (tsqa_index_create + tsqa_decompress_ranges*): every byte read is compared with a slice of
oracle.decompress(container), and nothing outside a read's destination may change."""
import json
import os
import subprocess

import numpy as np
import pytest

import fuzzgen
import kat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB4 = 1 << 22
ERR_ARG, ERR_FORMAT, ERR_STREAM = 3, 4, 5


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


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sentinel(n):
    return ((np.arange(n, dtype=np.uint64) * 37 + 11) % 251).astype(np.uint8) ^ 0xA5


def frames_of(raw):
    """(stream_at, stream_len) of every frame of a container (host bytes)"""
    nb = int.from_bytes(bytes(raw[4:8]), "little")
    at, out = 16, []
    for _ in range(nb):
        ln = int(raw[at]) | int(raw[at + 1]) << 8 | (int(raw[at + 2]) & 0x7F) << 16
        out.append((at + 3, ln))
        at += 3 + ln
    return out


def fenced(rng, lengths):
    """destinations for ranges of the given lengths, each behind a gap of 1..47 guard bytes: every residue mod 16 occurs"""
    at, outs = 0, []
    for ln in lengths:
        at += int(rng.integers(1, 48))
        outs.append(at)
        at += int(ln)
    return outs, at + 64


def read_fenced(idx, ranges, outs, cap, sync=True):
    """read (offset, length) ranges to the destinations `outs` of a sentinel-filled buffer; -> (buffer on the host, error code or 0),
    after checking that every byte outside the destinations still holds the sentinel"""
    from turbosqueeze_amd import TsqError
    import torch
    guard = sentinel(cap)
    out = to_dev(guard)
    rc = 0
    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            idx.read_into([(o, ln, a) for (o, ln), a in zip(ranges, outs)], out, sync=sync)
        side.synchronize()
        if not sync:
            rc = idx.codec.status()
    except TsqError as e:
        rc = e.code
    host = out.cpu().numpy()
    mask = np.ones(cap, dtype=bool)
    for (o, ln), a in zip(ranges, outs):
        mask[a:a + ln] = False
    assert np.array_equal(host[mask], guard[mask]), "a read wrote outside its destination"
    return host, rc


def check_ranges(idx, plain, ranges, rng):
    outs, cap = fenced(rng, [ln for _, ln in ranges])
    host, rc = read_fenced(idx, ranges, outs, cap)
    assert rc == 0
    for (o, ln), a in zip(ranges, outs):
        assert np.array_equal(host[a:a + ln], plain[o:o + ln]), f"range ({o}, {ln}) differs"


def standard_ranges(total):
    last = (total - 1) // MiB4 * MiB4
    return [(0, total), (0, 5000), (MiB4 // 2 - 100, 70000), (MiB4 - 3000, 3000), (123457, 1), (total - 1, 1),
            (MiB4 - 77, 200), (MiB4 - 500, 2 * MiB4 + 1000), (last - 9, total - last + 9), (last, total - last), (1, total - 2)]


@pytest.mark.parametrize("kind", ["text", "mix"])
@pytest.mark.parametrize("ext", [0, 1])
def test_reads_equal_oracle_slices(codec, oracle, tsq, kind, ext):
    n = 10 * MiB4 - 777_777                          # about 40 MiB, the last block short
    host = getattr(tsq.synth, kind)(n, seed=21 + ext)
    blob = oracle.compress(host, ext, threads=8)
    plain = np.frombuffer(oracle.decompress(blob, threads=8), dtype=np.uint8)
    assert plain.size == n
    idx = codec.index(to_dev(np.frombuffer(blob, dtype=np.uint8)))
    assert idx.n_blocks == 10 and idx.total == n
    rng = np.random.default_rng(ext)
    check_ranges(idx, plain, standard_ranges(n), rng)
    for off, ln in standard_ranges(n):                # one range per call, through read()
        assert np.array_equal(idx.read(off, ln).cpu().numpy(), plain[off:off + ln])
    packed, views = idx.read_many([(5, 10), (MiB4 - 1, 2), (n - 3, 3)])
    assert np.array_equal(packed.cpu().numpy(), np.concatenate([plain[5:15], plain[MiB4 - 1:MiB4 + 1], plain[n - 3:]]))
    assert np.array_equal(views[1].cpu().numpy(), plain[MiB4 - 1:MiB4 + 1])


def test_two_thousand_fenced_ranges_in_one_call(codec, oracle, tsq):
    n = 9 * MiB4 + 4321
    host = tsq.synth.mix(n, seed=5)
    blob = oracle.compress(host, 1, threads=8)
    plain = np.frombuffer(oracle.decompress(blob, threads=8), dtype=np.uint8)
    idx = codec.index(to_dev(np.frombuffer(blob, dtype=np.uint8)))
    rng = np.random.default_rng(2000)
    ranges = []
    for k in range(2000):
        ln = int(rng.integers(1, 70000)) if k % 50 else int(rng.integers(1, 2 * MiB4))
        off = int(rng.integers(0, n - ln + 1))
        ranges.append((off, ln))
    outs, cap = fenced(rng, [ln for _, ln in ranges])
    assert {a % 16 for a in outs} == set(range(16))
    host_out, rc = read_fenced(idx, ranges, outs, cap)
    assert rc == 0
    for (o, ln), a in zip(ranges, outs):
        assert np.array_equal(host_out[a:a + ln], plain[o:o + ln]), f"range ({o}, {ln}) at {a} differs"


def test_refusals_leave_the_output_untouched(codec, oracle, tsq):
    n = 2 * MiB4 + 999
    blob = oracle.compress(tsq.synth.text(n, seed=3), 0, threads=4)
    idx = codec.index(to_dev(np.frombuffer(blob, dtype=np.uint8)))
    cap = 100_000
    for triples in ([(n - 10, 11, 0)],                            # past the total
                    [(0, 1000, cap - 999)],                       # past the output
                    [(0, 1000, 0), (MiB4, 1000, 999)]):           # overlapping destinations
        guard = sentinel(cap)
        out = to_dev(guard)
        with pytest.raises(tsq.TsqError) as e:
            idx.read_into(triples, out)
        assert e.value.code == ERR_ARG
        with pytest.raises(tsq.TsqError) as e:
            idx.read_into(triples, out, sync=False)
        assert e.value.code == ERR_ARG
        assert np.array_equal(out.cpu().numpy(), guard)
    # malformed containers: no index (the same cases as test_container_errors)
    good = oracle.compress(tsq.synth.text(300000, 2), 0)
    for bad in (b"TSQ2" + good[4:], good[:4] + (0).to_bytes(4, "little") + good[8:], good[: len(good) // 2],
                good[:16] + b"\xff\xff\x7f" + good[19:], good[:10]):
        with pytest.raises(tsq.TsqError) as e:
            codec.index(to_dev(np.frombuffer(bad, dtype=np.uint8)))
        assert e.value.code == ERR_FORMAT


def test_damaged_containers(codec, oracle, tsq):
    """Byte damage as in test_corrupted_containers_agree_with_oracle, on containers of three or four blocks.  A whole-range read
    agrees with the oracle; when the damage lies only in block k's stream body, ranges wholly in other blocks are exact; guards hold
    and every call returns."""
    rng = np.random.default_rng(4242)
    bases = []
    for s in range(4):
        n = int(rng.integers(2 * MiB4 + 1, 4 * MiB4))
        ext = s & 1
        data = fuzzgen.structured(rng, n) if s < 2 else tsq.synth.mix(n, seed=s)
        blob = np.frombuffer(oracle.compress(data, ext, threads=8), dtype=np.uint8)
        bases.append((blob, np.frombuffer(oracle.decompress(blob, threads=8), dtype=np.uint8)))
    n_cases = int(os.environ.get("TSQ_GPU_CORRUPT_CASES", "150"))
    agree_ok = agree_bad = exact_other = 0
    for case in range(n_cases):
        blob, plain = bases[case % len(bases)]
        fr = frames_of(blob)
        bad = blob.copy()
        body_only = rng.random() < 0.6
        k = int(rng.integers(0, len(fr)))
        for _ in range(int(rng.integers(1, 6))):
            at = int(rng.integers(fr[k][0] + 3, fr[k][0] + fr[k][1])) if body_only else int(rng.integers(16, bad.size))
            bad[at] = rng.integers(0, 256) if rng.random() < 0.7 else bad[at] ^ (1 << int(rng.integers(0, 8)))
        want = oracle.decompress(bad)
        try:
            idx = codec.index(to_dev(bad))
        except tsq.TsqError as e:
            assert e.code == ERR_FORMAT and not body_only and want is None, f"case {case}"
            agree_bad += 1
            continue
        total = idx.total
        outs, cap = fenced(rng, [total])
        host, rc = read_fenced(idx, [(0, total)], outs, cap)
        if want is None:
            assert rc != 0, f"case {case}: the oracle rejects this container, the range read gave {total} bytes"
            agree_bad += 1
        else:
            assert rc == 0 and bytes(host[outs[0]:outs[0] + total]) == want, f"case {case}: both accept the container but disagree"
            agree_ok += 1
        # ranges of their own: wholly outside block k, and inside it (those must only return and keep the guards)
        starts = [b * MiB4 for b in range(len(fr))] + [total]
        others = [b for b in range(len(fr)) if b != k]
        ranges = []
        for _ in range(6):
            b = others[int(rng.integers(0, len(others)))]
            lo = int(rng.integers(starts[b], starts[b + 1]))
            ranges.append((lo, int(rng.integers(1, starts[b + 1] - lo + 1))))
        if body_only:
            outs, cap = fenced(rng, [ln for _, ln in ranges])
            host, rc = read_fenced(idx, ranges, outs, cap)
            assert rc == 0, f"case {case}: a read outside the damaged block {k} failed"
            for (o, ln), a in zip(ranges, outs):
                assert np.array_equal(host[a:a + ln], plain[o:o + ln]), f"case {case}: range ({o}, {ln}) outside block {k}"
            exact_other += 1
        if total == plain.size:
            inside = [(int(starts[k] + (starts[k + 1] - starts[k]) // 3), 1000), (starts[k], starts[k + 1] - starts[k])]
            outs, cap = fenced(rng, [ln for _, ln in inside])
            read_fenced(idx, inside, outs, cap)
        idx.close()
    assert agree_ok + agree_bad == n_cases and exact_other > 0


def test_containers_of_reference_streams(codec, tsq):
    """The golden block streams the compiled reference produced, framed as one-block containers (tsq_threads.cpp:218-239)"""
    golden = kat.GOLDEN
    manifest = json.load(open(os.path.join(golden, "manifest.json")))
    names = sorted(k for k in manifest if os.path.exists(os.path.join(golden, k + ".in")))
    rng = np.random.default_rng(5)
    for name in names:
        data = np.fromfile(os.path.join(golden, name + ".in"), dtype=np.uint8)
        for ext, tag in ((0, "noext"), (1, "ext")):
            stream = open(os.path.join(golden, f"{name}.{tag}"), "rb").read()
            frame = len(stream) | (ext << 23)
            blob = b"TSQ1" + (1).to_bytes(4, "little") + data.size.to_bytes(8, "little") + frame.to_bytes(3, "little") + stream
            idx = codec.index(to_dev(np.frombuffer(blob, dtype=np.uint8)))
            n = data.size
            ranges = [(0, n), (n - 1, 1), (n // 2, n - n // 2)] + [(o, int(rng.integers(1, n - o + 1))) for o in rng.integers(0, n, 20).tolist()]
            check_ranges(idx, data, ranges, rng)


def test_async_calls_back_to_back(codec, oracle, tsq):
    """Two batched calls on one stream with no synchronise between them: the second may not overwrite the first's staged items."""
    import torch
    n = 6 * MiB4 + 17
    host = tsq.synth.text(n, seed=61)
    blob = oracle.compress(host, 1, threads=8)
    plain = np.frombuffer(oracle.decompress(blob, threads=8), dtype=np.uint8)
    idx = codec.index(to_dev(np.frombuffer(blob, dtype=np.uint8)))
    rng = np.random.default_rng(6)
    sets = []
    for _ in range(2):
        sets.append([(int(o), int(rng.integers(1, 200_000))) for o in rng.integers(0, n - 200_000, 600)])
    results = []
    side = torch.cuda.Stream()               # (a stream of its own: NULL would mean the context's stream to the library)
    with torch.cuda.stream(side):
        for rs in sets:
            packed, views = idx.read_many_async(rs)
            results.append((rs, packed, views))
    side.synchronize()
    assert codec.status() == 0
    for rs, packed, views in results:
        want = np.concatenate([plain[o:o + ln] for o, ln in rs])
        assert np.array_equal(packed.cpu().numpy(), want)
        assert np.array_equal(views[-1].cpu().numpy(), plain[rs[-1][0]:rs[-1][0] + rs[-1][1]])


def test_three_async_calls_in_flight(codec, oracle, tsq):
    """Three calls on one stream with no synchronise between them: the staged items go through a ring of two slots, so the third
    call takes the slot of the first, once that one has finished.  One container of two blocks, three ranges of 1..100 bytes per
    call, one of them across the block edge."""
    import torch
    n = MiB4 + 1000
    blob = oracle.compress(tsq.synth.text(n, seed=62), 1, threads=2)
    plain = np.frombuffer(oracle.decompress(blob, threads=2), dtype=np.uint8)
    idx = codec.index(to_dev(np.frombuffer(blob, dtype=np.uint8)))
    sets = [[(0, 1), (MiB4 - 40, 100), (n - 7, 7)], [(123457, 100), (MiB4 - 1, 2), (MiB4, 33)], [(5, 64), (MiB4 + 900, 100), (MiB4 - 99, 100)]]
    results = []
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for rs in sets:
            results.append((rs, idx.read_many_async(rs)[0]))
    side.synchronize()
    assert codec.status() == 0
    for rs, packed in results:
        assert np.array_equal(packed.cpu().numpy(), np.concatenate([plain[o:o + ln] for o, ln in rs])), rs
    idx.close()


def test_index_owns_its_frames(codec, oracle, tsq):
    import torch
    a = tsq.synth.text(5 * MiB4 + 3, seed=71)
    b = tsq.synth.mix(3 * MiB4 + 5, seed=72)
    blob_a = oracle.compress(a, 0, threads=8)
    idx = codec.index(to_dev(np.frombuffer(blob_a, dtype=np.uint8)))
    assert np.array_equal(idx.read(MiB4 - 5, 2 * MiB4).cpu().numpy(), a[MiB4 - 5:3 * MiB4 - 5])
    back = codec.decompress(to_dev(np.frombuffer(oracle.compress(b, 1, threads=8), dtype=np.uint8)))
    assert torch.equal(back, to_dev(b))
    assert np.array_equal(idx.read(3 * MiB4 + 100, 2 * MiB4 - 97).cpu().numpy(), a[3 * MiB4 + 100:])


def test_enwik9_sized_batch(codec, oracle, tsq):
    import torch
    n = 1_000_000_000
    host = tsq.synth.text(n, seed=9)
    blob = codec.compress(to_dev(host), 1)
    plain = np.frombuffer(oracle.decompress(blob.cpu().numpy(), threads=os.cpu_count() or 8), dtype=np.uint8)
    assert plain.size == n
    idx = codec.index(blob)
    assert idx.n_blocks == 239
    rng = np.random.default_rng(9)
    ranges = [(0, n)] + [(int(o), int(rng.integers(1, 300_000))) for o in rng.integers(0, n - 300_000, 1000)]
    packed, views = idx.read_many(ranges)
    assert torch.equal(views[0], to_dev(plain))
    got = packed[n:].cpu().numpy()
    at = 0
    for o, ln in ranges[1:]:
        assert np.array_equal(got[at:at + ln], plain[o:o + ln]), f"range ({o}, {ln})"
        at += ln


def test_cli_range_read(tmp_path, oracle, tsq):
    n = 3 * MiB4 + 12345
    host = tsq.synth.mix(n, seed=91)
    packed = tmp_path / "in.tsq"
    packed.write_bytes(oracle.compress(host, 1, threads=4))
    plain = np.frombuffer(oracle.decompress(packed.read_bytes(), threads=4), dtype=np.uint8)
    cli = os.path.join(ROOT, "tools", "tsq_cli")
    for off, ln in ((MiB4 - 1000, MiB4 + 2000), (0, n), (n - 1, 1)):
        out = tmp_path / "slice.bin"
        r = subprocess.run([cli, "x", str(packed), str(off), str(ln), str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        assert out.read_bytes() == plain[off:off + ln].tobytes()
    r = subprocess.run([cli, "x", str(packed), str(n - 1), "2", str(tmp_path / "no.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
