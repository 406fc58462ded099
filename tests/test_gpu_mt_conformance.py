"""The scheduler behind the reference's own API (tsq_compat.hip: tsqDecompress_MT, tsqCompress_MT, the async forms, FILE* to FILE*) on
the inputs of tests/mtgen.py: containers of uneven blocks and block counts around the ramped schedule down every source and sink,
jobs that fail with batches in flight and the job after them on the same lanes, damaged and cut containers against the oracle,
failures inside a queue of async jobs, compress jobs whose look-ahead falls on a lane's leftovers, and one context of each direction
through jobs that change mode and size, so that every job meets the buffers the one before it left.

Expected bytes are the builders' plain bytes or the oracle's output, never the output of a library entry point.  Everything runs in
this process, on a few long-lived contexts; the environment is set before a context is allocated (TSQ_AMD_LANES, _BATCH_BLOCKS,
_FILE_BATCH_BLOCKS, _DEVICES are read there) or before a job (TSQ_AMD_FILE_INMEM_MAX, _FILE_MAP_MIN, _FILE_NO_MMAP, _NO_RAMP).
No case is dropped: the paths count what they ran and the last test compares the counts with the generators' sizes."""
import ctypes as C
import threading

import pytest

import mtgen
from streamgen import CATALOGUE
from test_gpu_range import codec, tsq  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

COUNTS: dict = {}


def count(path, n=1):
    COUNTS[path] = COUNTS.get(path, 0) + n


_CACHE: dict = {}


def cached(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def valid_containers():
    return cached("valid", mtgen.ramp_containers)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the valid containers as files, written once"""
    d = tmp_path_factory.mktemp("mt_containers")
    out = {}
    for name, blob, _, _ in valid_containers():
        p = d / f"{name}.tsq"
        p.write_bytes(blob)
        out[name] = p
    return out


# ---------------------------------------------------------------- ctypes helpers

class Context:
    """one scheduler context; allocate it after the environment is set"""

    def __init__(self, tsq, compress=False):
        self.L, self.compress = tsq.lib(), compress
        self.free = tsq.api._libc.free
        self.h = (self.L.tsqAllocateContextCompression_MT if compress else self.L.tsqAllocateContextDecompression_MT)(False)
        assert self.h

    def close(self):
        if self.h:
            (self.L.tsqDeallocateContextCompression_MT if self.compress else self.L.tsqDeallocateContextDecompression_MT)(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _call(self, src, n, infile, outpp, szp, outfile, ext):
        if self.compress:
            return self.L.tsqCompress_MT(self.h, src, n, infile, outpp, szp, outfile, bool(ext), 0)
        return self.L.tsqDecompress_MT(self.h, src, n, infile, outpp, szp, outfile)

    def run(self, src, dst=None, ext=0):
        """src: bytes (memory) or a path (file); dst: None (memory) or a path.  -> the result's bytes (memory sink) or True (file
        sink), None for a false return -- after which *out and *szout must be as they were, NULL and 0"""
        if isinstance(src, (bytes, bytearray)):
            buf, n, infile = C.create_string_buffer(bytes(src), len(src)), len(src), False
        else:
            buf, n, infile = C.c_char_p(str(src).encode()), 0, True
        if dst is None:
            out, sz = C.c_void_p(), C.c_size_t(0)
            ok = self._call(buf, n, infile, C.byref(out), C.byref(sz), False, ext)
            if not ok:
                assert out.value is None and sz.value == 0, "a failed job left something in *out / *szout"
                return None
            assert out.value is not None
            try:
                return C.string_at(out, sz.value)
            finally:
                self.free(out)
        path = C.c_char_p(str(dst).encode())
        ok = self._call(buf, n, infile, C.cast(C.pointer(path), C.POINTER(C.c_void_p)), None, True, ext)
        return True if ok else None


def job_env(monkeypatch, streamed=False, sink=""):
    """per-job switches: a file source streamed through pinned staging; a file sink mapped, or written with positional writes
    ("" leaves a small file sink collected in memory)"""
    for k in ("TSQ_AMD_FILE_INMEM_MAX", "TSQ_AMD_FILE_MAP_MIN", "TSQ_AMD_FILE_NO_MMAP"):
        monkeypatch.delenv(k, raising=False)
    if streamed:
        monkeypatch.setenv("TSQ_AMD_FILE_INMEM_MAX", "1")
    if sink in ("map", "pwrite"):
        monkeypatch.setenv("TSQ_AMD_FILE_MAP_MIN", "1")
    if sink == "pwrite":
        monkeypatch.setenv("TSQ_AMD_FILE_NO_MMAP", "1")


# ---------------------------------------------------------------- a. valid containers down every path

# name: (allocation environment, source, streamed, sink)
PATHS = {
    "mem_to_mem": ({}, "mem", False, None),
    "file_in_memory_to_mem": ({}, "file", False, None),
    "file_in_memory_to_collected_file": ({}, "file", False, ""),
    "streamed_1_to_mem": ({"TSQ_AMD_FILE_BATCH_BLOCKS": "1"}, "file", True, None),
    "streamed_1_to_mapped_file": ({"TSQ_AMD_FILE_BATCH_BLOCKS": "1"}, "file", True, "map"),
    "streamed_5_to_mem": ({"TSQ_AMD_FILE_BATCH_BLOCKS": "5"}, "file", True, None),
    "streamed_5_to_pwrite_file": ({"TSQ_AMD_FILE_BATCH_BLOCKS": "5"}, "file", True, "pwrite"),
    "mem_to_collected_file": ({}, "mem", False, ""),
    "mem_to_mapped_file": ({}, "mem", False, "map"),
    "mem_to_pwrite_file": ({}, "mem", False, "pwrite"),
    "batch_blocks_1": ({"TSQ_AMD_BATCH_BLOCKS": "1"}, "mem", False, None),
    "batch_blocks_2": ({"TSQ_AMD_BATCH_BLOCKS": "2"}, "mem", False, None),
    "batch_blocks_3": ({"TSQ_AMD_BATCH_BLOCKS": "3"}, "mem", False, None),
    "one_lane": ({"TSQ_AMD_LANES": "1"}, "mem", False, None),
    "one_lane_batch_blocks_3_streamed_to_mapped_file": ({"TSQ_AMD_LANES": "1", "TSQ_AMD_BATCH_BLOCKS": "3"}, "file", True, "map"),
    "device_listed_twice": ({"TSQ_AMD_DEVICES": "0,0"}, "mem", False, None),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_valid_containers_down_every_path(tsq, files, tmp_path, monkeypatch, path):
    alloc_env, source, streamed, sink = PATHS[path]
    for k in ("TSQ_AMD_LANES", "TSQ_AMD_BATCH_BLOCKS", "TSQ_AMD_FILE_BATCH_BLOCKS", "TSQ_AMD_DEVICES", "TSQ_AMD_NO_RAMP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in alloc_env.items():
        monkeypatch.setenv(k, v)
    job_env(monkeypatch, streamed, sink or "")
    dst = tmp_path / "back.bin"
    with Context(tsq) as ctx:
        for name, blob, plain, sizes in valid_containers():
            # the ramped schedule is the memory-to-memory one: there every ramp container runs with and without it
            ramps = (False, True) if (path == "mem_to_mem" and name.startswith("ramp_")) else (False,)
            for no_ramp in ramps:
                if no_ramp:
                    monkeypatch.setenv("TSQ_AMD_NO_RAMP", "1")
                src = blob if source == "mem" else files[name]
                if sink is None:
                    got = ctx.run(src)
                else:
                    assert ctx.run(src, dst) is True, (path, name)
                    got = dst.read_bytes()
                monkeypatch.delenv("TSQ_AMD_NO_RAMP", raising=False)
                assert got is not None and len(got) == len(plain) and got == plain, (path, name, no_ramp)
            count(path)


def progress_job(tsq, ctx, blob):
    """one async memory-to-memory decompress with both callbacks -> (ok, result bytes, progress fractions, how many progress calls
    had come when the completion callback ran)"""
    L = ctx.L
    seen, done, finished = [], [], threading.Event()

    def on_done(jobid, ok, user):
        done.append((jobid, bool(ok), len(seen)))
        finished.set()
    pcb = tsq.api.PROGRESS_FN(lambda jobid, frac, user: seen.append((jobid, frac)))
    dcb = tsq.api.DONE_FN(on_done)
    buf = C.create_string_buffer(blob, len(blob))
    out, sz = C.c_void_p(), C.c_size_t(0)
    jid = L.tsqa_decompress_async_cb(ctx.h, buf, len(blob), False, C.byref(out), C.byref(sz), False, C.cast(dcb, C.c_void_p),
                                     C.cast(pcb, C.c_void_p), None)
    assert jid >= 1
    assert finished.wait(120), "the completion callback never came"
    assert len(done) == 1 and done[0][0] == jid and {j for j, _ in seen} <= {jid}
    got = C.string_at(out, sz.value) if done[0][1] else None
    if done[0][1]:
        ctx.free(out)
    return done[0][1], got, [f for _, f in seen], done[0][2]


def test_progress_once_per_block_of_uneven_and_ramped_containers(tsq, monkeypatch):
    """tsq_threads.cpp:648-655: one call per block as it lands, fractions (k + 1) / n_blocks in order, all before the completion
    callback -- blocks of 0 bytes included, whatever pieces the batches come back in"""
    for k in ("TSQ_AMD_LANES", "TSQ_AMD_BATCH_BLOCKS", "TSQ_AMD_DEVICES", "TSQ_AMD_NO_RAMP"):
        monkeypatch.delenv(k, raising=False)
    by_name = {name: (blob, plain) for name, blob, plain, _ in valid_containers()}
    with Context(tsq) as ctx:
        for name in ("uneven_unit", "ramp_73"):
            blob, plain = by_name[name]
            nb = mtgen.block_count(blob)
            ok, got, fractions, before_done = progress_job(tsq, ctx, blob)
            assert ok and got == plain, name
            assert fractions == [(k + 1) / nb for k in range(nb)], (name, len(fractions))
            assert before_done == nb, name
            count("progress")


def test_file_pointer_api_on_the_uneven_unit(tsq, files, tmp_path):
    """tsqDecompress(FILE*, FILE*) (turbosqueeze.cpp:98-147)"""
    L, libc = tsq.lib(), tsq.api._libc
    libc.fopen.restype = C.c_void_p
    libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
    libc.fclose.argtypes = [C.c_void_p]
    plain = {name: p for name, _, p, _ in valid_containers()}["uneven_unit"]
    dst = tmp_path / "back.bin"
    fin, fout = libc.fopen(str(files["uneven_unit"]).encode(), b"rb"), libc.fopen(str(dst).encode(), b"wb")
    assert fin and fout
    L.tsqDecompress(fin, fout)
    libc.fclose(fin); libc.fclose(fout)
    assert dst.read_bytes() == plain
    count("file_pointer_api")


# ---------------------------------------------------------------- b. twins: a job that fails with batches in flight

def test_twins_fail_the_job_and_the_next_job_is_exact(tsq, tmp_path, monkeypatch):
    """Two blocks per batch, six blocks, the twin in the first batch, the second, as the second block of the second, and in the
    last: the job returns false with *out and *szout untouched (Context.run), whatever was in flight, and the next job on the same
    lanes decodes six healthy blocks exactly.  Then the same through a streamed file source and a mapped file sink."""
    for k in ("TSQ_AMD_LANES", "TSQ_AMD_FILE_BATCH_BLOCKS", "TSQ_AMD_DEVICES", "TSQ_AMD_NO_RAMP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TSQ_AMD_BATCH_BLOCKS", "2")
    job_env(monkeypatch)
    twins = mtgen.twin_containers()
    healthy, plain = mtgen.healthy_six()
    with Context(tsq) as ctx:
        assert ctx.run(healthy) == plain
        for name, blob, k, kind in twins:
            assert ctx.run(blob) is None, (name, k, kind)
            assert ctx.run(healthy) == plain, f"the job after {name} (twin in block {k})"
            count("twins_mem_to_mem")
        job_env(monkeypatch, streamed=True, sink="map")
        src, good, dst = tmp_path / "twin.tsq", tmp_path / "healthy.tsq", tmp_path / "back.bin"
        good.write_bytes(healthy)
        for name, blob, k, kind in twins:
            src.write_bytes(blob)
            assert ctx.run(src, dst) is None, (name, k, kind)
            assert ctx.run(good, dst) is True and dst.read_bytes() == plain, f"the job after {name} (twin in block {k})"
            count("twins_streamed_to_mapped_file")


# ---------------------------------------------------------------- c. damage against the oracle

def damage_cases(oracle):
    return cached("damage", lambda: [(name, blob, mtgen.expected_of_the_scheduler(oracle, blob)) for name, blob in mtgen.damaged_containers()])


def test_damaged_containers_agree_with_the_oracle(tsq, oracle, tmp_path, monkeypatch):
    for k in ("TSQ_AMD_LANES", "TSQ_AMD_FILE_BATCH_BLOCKS", "TSQ_AMD_DEVICES", "TSQ_AMD_NO_RAMP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TSQ_AMD_BATCH_BLOCKS", "3")
    job_env(monkeypatch)
    cases = damage_cases(oracle)
    src = tmp_path / "damaged.tsq"
    with Context(tsq) as ctx:
        for i, (name, blob, want) in enumerate(cases):
            got = ctx.run(blob)
            print(name, "oracle:", None if want is None else len(want), "scheduler:", None if got is None else len(got))
            assert (got is None) == (want is None), f"{name}: the verdicts differ (scheduler {'refuses' if got is None else 'accepts'})"
            assert got == want, f"{name}: both accept the container but disagree"
            count("damage_mem_to_mem")
            if i % 3 == 0:
                job_env(monkeypatch, streamed=True)
                src.write_bytes(blob)
                got = ctx.run(src)
                job_env(monkeypatch)
                assert (got is None) == (want is None) and got == want, f"{name}, streamed"
                count("damage_streamed")


# ---------------------------------------------------------------- d. failures inside a FIFO

def fifo_jobs(oracle, n):
    """n jobs, every third one a failing one (twins and rejected damaged cases in turn) -> [(container, expected bytes or None)]"""
    healthy = [(blob, plain) for _, blob, plain, _ in valid_containers() if len(blob) < 10 << 20][:2] + [mtgen.healthy_six()]
    healthy += [(blob, want) for _, blob, want in damage_cases(oracle) if want is not None][:6]
    twins = [blob for _, blob, _, kind in mtgen.twin_containers() if len(blob) < 1 << 20]
    rejected = [blob for _, blob, want in damage_cases(oracle) if want is None]
    failing = [x for pair in zip(twins, rejected) for x in pair]
    return [(failing[k // 3 % len(failing)], None) if k % 3 == 2 else healthy[k % len(healthy)] for k in range(n)]


def submit(tsq, ctx, blob, slot, cb):
    buf = C.create_string_buffer(blob, len(blob))
    slot.update(buf=buf, out=C.c_void_p(), sz=C.c_size_t(0))
    return ctx.L.tsqa_decompress_async_cb(ctx.h, buf, len(blob), False, C.byref(slot["out"]), C.byref(slot["sz"]), False,
                                          C.cast(cb, C.c_void_p), None, None)


def test_failures_inside_a_queue_of_async_jobs(tsq, oracle, monkeypatch):
    for k in ("TSQ_AMD_LANES", "TSQ_AMD_DEVICES", "TSQ_AMD_NO_RAMP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TSQ_AMD_BATCH_BLOCKS", "2")
    job_env(monkeypatch)
    jobs = fifo_jobs(oracle, 30)
    assert sum(1 for _, want in jobs if want is None) == 10
    order, slots = [], [dict() for _ in jobs]
    cb = tsq.api.DONE_FN(lambda jobid, ok, user: order.append((jobid, bool(ok))))
    ctx = Context(tsq)
    ids = [submit(tsq, ctx, blob, slot, cb) for (blob, _), slot in zip(jobs, slots)]
    ctx.close()                                                   # returns once every queued job and its callback has run
    assert ids == list(range(1, len(jobs) + 1))
    assert [j for j, _ in order] == ids, "completions out of submission order"
    assert [ok for _, ok in order] == [want is not None for _, want in jobs]
    for k, ((_, want), slot) in enumerate(zip(jobs, slots)):
        if want is None:
            assert slot["out"].value is None and slot["sz"].value == 0, f"job {k + 1} failed and left something in *out / *szout"
        else:
            assert C.string_at(slot["out"], slot["sz"].value) == want, f"job {k + 1}"
            tsq.api._libc.free(slot["out"])
    count("fifo", len(jobs))


def test_completion_callback_of_a_failed_job_submits_the_next(tsq, oracle, monkeypatch):
    """a chain driven from the scheduler thread: every completion callback, those of the failed jobs included, submits the next job"""
    for k in ("TSQ_AMD_LANES", "TSQ_AMD_DEVICES", "TSQ_AMD_NO_RAMP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TSQ_AMD_BATCH_BLOCKS", "2")
    job_env(monkeypatch)
    jobs = [j for j in fifo_jobs(oracle, 12)[2:]]                 # starts with a failing job: fail, good, good, fail, ...
    assert jobs[0][1] is None and jobs[1][1] is not None and jobs[3][1] is None
    slots, order, ids = [dict() for _ in jobs], [], []
    ctx = Context(tsq)

    def on_done(jobid, ok, user):
        order.append((jobid, bool(ok)))
        k = len(order)
        if k < len(jobs):
            ids.append(submit(tsq, ctx, jobs[k][0], slots[k], cb))
    cb = tsq.api.DONE_FN(on_done)
    ids.append(submit(tsq, ctx, jobs[0][0], slots[0], cb))
    ctx.close()                                                   # waits for the whole chain: a callback submits before its job is retired
    assert ids == list(range(1, len(jobs) + 1)) and [j for j, _ in order] == ids
    assert [ok for _, ok in order] == [want is not None for _, want in jobs]
    for k, ((_, want), slot) in enumerate(zip(jobs, slots)):
        if want is not None:
            assert C.string_at(slot["out"], slot["sz"].value) == want, f"job {k + 1}"
            tsq.api._libc.free(slot["out"])
    count("chain", len(jobs))


# ---------------------------------------------------------------- e. compress: the look-ahead at the end of input

def oracle_containers(oracle, kept):
    return cached("lookahead_want", lambda: {(name, ext): oracle.compress(b, ext, threads=2) for name, b, _ in kept for ext in (0, 1)})


@pytest.mark.parametrize("mode", ["memory", "streamed"])
def test_lookahead_behind_the_input_is_zeros_on_a_reused_lane(tsq, oracle, tmp_path, monkeypatch, mode):
    """One lane: job A leaves its bytes in the lane's buffers, job B ends inside them.  B's container is the oracle's -- zeros behind
    the input -- memory to memory (one batch) and from a streamed file at one block per batch."""
    for k in ("TSQ_AMD_BATCH_BLOCKS", "TSQ_AMD_DEVICES", "TSQ_AMD_NO_RAMP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("TSQ_AMD_LANES", "1")
    monkeypatch.setenv("TSQ_AMD_FILE_BATCH_BLOCKS", "1")
    job_env(monkeypatch, streamed=mode == "streamed")
    a, kept = mtgen.lookahead_jobs(oracle)
    want = oracle_containers(oracle, kept)
    fa, fb = tmp_path / "a.bin", tmp_path / "b.bin"
    fa.write_bytes(a)
    with Context(tsq, compress=True) as ctx:
        assert ctx.run(a, ext=1) == oracle.compress(a, 1, threads=3)
        for name, b, _ in kept:
            fb.write_bytes(b)
            for ext in (0, 1):
                assert ctx.run(a if mode == "memory" else fa, ext=ext) is not None
                assert ctx.run(b if mode == "memory" else fb, ext=ext) == want[(name, ext)], (name, ext, mode)
            count(f"lookahead_{mode}")
        if mode == "streamed":
            return
        job_env(monkeypatch)
        # inputs of 1 to 8 bytes, behind A once more
        assert ctx.run(a, ext=0) is not None
        tails = {len(c.data): c.data for c in mtgen.encgen.catalogue() if c.name.startswith("tail_random_")}
        for n in range(1, 9):
            for ext in (0, 1):
                assert ctx.run(tails[n], ext=ext) == oracle.compress(tails[n], ext), (n, ext)
            count("tiny_inputs")
        # failure returns, each followed by a good job on the same context
        small = kept[0][1][:300_000]
        want = oracle.compress(small, 1)
        assert ctx.run(tmp_path / "no_such_input.bin", ext=1) is None
        assert ctx.run(small, ext=1) == want
        assert ctx.run(small, tmp_path / "no_such_directory" / "out.tsq", ext=1) is None
        assert ctx.run(fb, tmp_path / "no_such_directory" / "out.tsq", ext=1) is None
        assert ctx.run(small, tmp_path / "out.tsq", ext=1) is True and (tmp_path / "out.tsq").read_bytes() == want
        count("compress_failures")


# ---------------------------------------------------------------- f. one lane's buffers across jobs that change mode and size

# (which container, streamed file source, sink): on ONE context, so that each job meets the buffers the one before it left --
# device buffers made without staging; staging wanted on both sides at an unchanged device capacity; device buffers that grow and
# release their staging; staging made again at the new capacity; the small job once more, in buffers larger than it needs
SEAM_JOBS = (("small", False, None), ("small", True, "map"), ("large", False, None), ("large", True, "pwrite"), ("small", True, None))


@pytest.mark.parametrize("lanes", ["1", None])
def test_one_context_through_jobs_that_change_mode_and_size(tsq, oracle, files, tmp_path, monkeypatch, lanes):
    """The uneven unit and the largest valid container, decompressed by one context in the order of SEAM_JOBS: the builders' plain
    bytes.  Then those plain bytes through one compression context in the same order and modes, with and without extensions: the
    oracle's containers.  With one lane every job lands in the same buffers; then with the default lane count."""
    for k in ("TSQ_AMD_LANES", "TSQ_AMD_BATCH_BLOCKS", "TSQ_AMD_FILE_BATCH_BLOCKS", "TSQ_AMD_DEVICES", "TSQ_AMD_NO_RAMP"):
        monkeypatch.delenv(k, raising=False)
    if lanes:
        monkeypatch.setenv("TSQ_AMD_LANES", lanes)
    by_name = {name: (name, blob, plain) for name, blob, plain, _ in valid_containers()}
    which = {"small": by_name["uneven_unit"], "large": max(by_name.values(), key=lambda c: len(c[2]))}
    assert mtgen.block_count(which["large"][1]) > mtgen.block_count(which["small"][1]) and len(which["large"][1]) > len(which["small"][1])
    assert all(len(plain) < 12 << 20 for _, _, plain in which.values())
    want = cached("seam_want", lambda: {(size, ext): oracle.compress(plain, ext, threads=2)
                                        for size, (_, _, plain) in which.items() for ext in (0, 1)})
    plain_files = {}
    for size, (name, _, plain) in which.items():
        plain_files[size] = tmp_path / f"{name}.bin"
        plain_files[size].write_bytes(plain)
    dst = tmp_path / "out.bin"

    def run(ctx, src, streamed, sink, ext=0):
        job_env(monkeypatch, streamed, sink or "")
        if sink is None:
            return ctx.run(src, ext=ext)
        assert ctx.run(src, dst, ext=ext) is True
        return dst.read_bytes()

    with Context(tsq) as ctx:
        for step, (size, streamed, sink) in enumerate(SEAM_JOBS):
            name, blob, plain = which[size]
            got = run(ctx, files[name] if streamed else blob, streamed, sink)
            assert got is not None and len(got) == len(plain) and got == plain, (lanes, step, name)
            count("seam_decompress")
    with Context(tsq, compress=True) as ctx:
        for step, (size, streamed, sink) in enumerate(SEAM_JOBS):
            name, _, plain = which[size]
            for ext in (0, 1):
                got = run(ctx, plain_files[size] if streamed else plain, streamed, sink, ext)
                assert got == want[(size, ext)], (lanes, step, name, ext)
                count("seam_compress")


# ---------------------------------------------------------------- no case was dropped

def test_every_case_ran_down_every_path(oracle):
    n_valid, n_twins, n_damaged = len(valid_containers()), len(CATALOGUE.invalid), len(mtgen.damaged_containers())
    assert n_valid == 7 and n_twins >= 40 and n_damaged == 131
    a, kept = mtgen.lookahead_jobs(oracle)
    want = {path: n_valid for path in PATHS}
    want.update(progress=2, file_pointer_api=1, twins_mem_to_mem=n_twins, twins_streamed_to_mapped_file=n_twins,
                damage_mem_to_mem=n_damaged, damage_streamed=(n_damaged + 2) // 3, fifo=30, chain=10, lookahead_memory=len(kept), lookahead_streamed=len(kept),
                tiny_inputs=8, compress_failures=1, seam_decompress=2 * len(SEAM_JOBS), seam_compress=4 * len(SEAM_JOBS))
    print("scheduler conformance counts:", dict(sorted(COUNTS.items())))
    assert {k: COUNTS.get(k, 0) for k in want} == want
