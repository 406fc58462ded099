"""Timing of the index made from a size table (tsqa_index_create_sized*) against tsqa_index_create on the same short-block container,
synth text, extensions on.  Warm-ups first, then --reps rounds in which the ways under comparison take turns; the median of the reps
with their minimum and maximum beside every figure.  One JSON line per measurement, printed and appended to --out
(profiles/seek_time.jsonl), with the source fingerprint.

  index_create   tsqa_index_create (host clock: the call waits twice) against tsqa_index_create_sized_async -- host clock of the call
                 alone (what the caller's thread pays: the allocation, the host's plan, four enqueues) and event span on an idle
                 stream (the host's enqueue and the device's work, whichever ends last) -- and against tsqa_index_create_sized
                 (host clock, waits once).
                 Shapes: --create-shapes, MiB:log2(block_len).
  walk           the three launches against the one-workgroup frame_walk_sized_kernel on the same container and table.  The
                 one-workgroup walk as tools/split_time.py takes it: the sized decompress call's span minus its decode span
                 (tsqa_profile_enable).  The three launches: the event span of tsqa_index_create_sized_async behind a filler kernel
                 that keeps the stream busy while the host enqueues, so the span holds device work only: the zero fill of the
                 descriptors and the three kernels.  The fill is part of the figure (the one-workgroup walk has none), and both
                 figures are at the resolution of device events, not kernel times from a trace.  host_hidden says whether the
                 filler outlasted the host's enqueue in every rep; where it did not, the span holds host time too.
  records        --records records of 100 B out of --record-mib MiB through tsqa_decompress_item_ranges_async at each of
                 --record-block-lens: the read alone (event span) through either index, and creation plus read (host clock from
                 the first call to the end of the stream) with either creation.
  chain          compress_split_async -> index_create_sized_async -> decompress_item_ranges_async as ONE event span on one stream
                 with nothing waited for in between, and its host clock; against the same steps with tsqa_index_create, which
                 needs the stream drained in front of it (host clock).

three_launch_beats_one_workgroup, sized_create_beats_classic and chain_sized_beats_classic say whether a median beats the other
way's by more than that way's own spread (max - min of its reps)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--create-shapes", default="256:16,1024:12", help="MiB:log2(block_len) of the index_create and walk cases")
    ap.add_argument("--record-mib", type=int, default=64)
    ap.add_argument("--record-block-lens", default="22,16,12", help="log2 of the block lengths of the records and chain cases")
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--filler-mib", type=int, default=4096, help="bytes the filler kernel zeroes in front of a device-only span")
    ap.add_argument("--cases", default="index_create,walk,records,chain")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seek_time.jsonl"), help="the JSON lines are appended to this file")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import turbosqueeze_amd as tsq

    torch.cuda.set_device(0)
    codec = tsq.DeviceCodec(0)
    L = codec.L
    # a stream of its own: the library takes a NULL stream (torch's default) as the context's own, which torch's events do not see
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    hs = C.c_void_p(s.cuda_stream)
    ext = 1
    d_size, d_status = codec._size.data_ptr(), codec._status.data_ptr()
    fingerprint = tsq.source_fingerprint()
    cases = args.cases.split(",")

    def emit(res):
        res.update(source=fingerprint, reps=args.reps, warmup=args.warmup, ext=ext, input="synth_text")
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    class Made:
        """the index of the last creation; in_turns destroys it before the next"""
        h = None

        def drop(self):
            if self.h:
                L.tsqa_index_destroy(self.h)
            self.h = None

    made = Made()

    def in_turns(ways, keep_index=False):
        """ways: name -> call() -> ms (or a tuple of them).  -> name -> the list of results of the timed rounds.  The index of the
        call before is destroyed in front of every call, outside what is timed (hipFree waits for the device), unless keep_index."""
        times = {k: [] for k in ways}
        for r in range(args.warmup + args.reps):
            for name, call in ways.items():
                if not keep_index:
                    made.drop()
                torch.cuda.synchronize()
                t = call()
                if r >= args.warmup:
                    times[name].append(t)
        return times

    med = lambda ts: round(statistics.median(ts), 4)
    spread = lambda ts: [round(min(ts), 4), round(max(ts), 4)]
    beats = lambda new, old: bool(statistics.median(old) - statistics.median(new) > max(old) - min(old))

    def figures(res, name, ts):
        res[name + "_ms"], res[name + "_spread_ms"] = med(ts), spread(ts)

    def wall(call):
        """host clock of call() and of draining the stream behind it"""
        t0 = time.perf_counter()
        call()
        s.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def span(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        call()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def split_container(src, n, block_len):
        nb, bound = tsq.plan_split(n, block_len)
        blob = torch.empty(bound, dtype=torch.uint8, device="cuda")
        table = torch.empty(nb, dtype=torch.int32, device="cuda")

        def compress():
            rc = L.tsqa_compress_device_split_async(codec.h, src.data_ptr(), n, block_len, blob.data_ptr(), bound, d_size, table.data_ptr(), d_status,
                                                    ext, hs)
            assert rc == 0, codec.last_error()

        compress()
        s.synchronize()
        size, st = codec.last_size_status()
        assert st == 0
        return nb, bound, blob, table, size, compress

    def creators(blob, room, n, block_len, table):
        def classic():
            assert made.h is None
            made.h = C.c_void_p()
            rc = L.tsqa_index_create(codec.h, blob.data_ptr(), room, C.byref(made.h))
            assert rc == 0, codec.last_error()

        def sized_async():
            assert made.h is None
            made.h = C.c_void_p()
            rc = L.tsqa_index_create_sized_async(codec.h, blob.data_ptr(), room, n, block_len, table.data_ptr(), C.byref(made.h), hs)
            assert rc == 0, codec.last_error()

        def sized_wait():
            assert made.h is None
            made.h = C.c_void_p()
            rc = L.tsqa_index_create_sized(codec.h, blob.data_ptr(), room, n, block_len, table.data_ptr(), C.byref(made.h), hs)
            assert rc == 0, codec.last_error()

        return classic, sized_async, sized_wait

    # ---- index creation, and the walk alone ----
    if "index_create" in cases or "walk" in cases:
        filler = torch.empty(args.filler_mib * MiB, dtype=torch.uint8, device="cuda")
        for shape in args.create_shapes.split(","):
            size_mib, log2 = (int(x) for x in shape.split(":"))
            n, block_len = size_mib * MiB, 1 << log2
            src = torch.from_numpy(tsq.synth.text(n, seed=5)).cuda()
            nb, bound, blob, table, size, _ = split_container(src, n, block_len)
            classic, sized_async, sized_wait = creators(blob, size, n, block_len, table)
            base = {"mib": size_mib, "bytes": n, "block_len": block_len, "blocks": nb, "container_bytes": size}

            if "index_create" in cases:
                def host_only():
                    t0 = time.perf_counter()
                    sized_async()
                    t1 = time.perf_counter()
                    s.synchronize()
                    return (t1 - t0) * 1e3

                t = in_turns({"classic": lambda: wall(classic), "sized_async_host": host_only, "sized_async_span": lambda: span(sized_async),
                              "sized_wait": lambda: wall(sized_wait)})
                res = dict(base, case="index_create")
                figures(res, "index_create_classic_wall", t["classic"])
                figures(res, "index_create_sized_async_host", t["sized_async_host"])
                figures(res, "index_create_sized_async_idle_span", t["sized_async_span"])
                figures(res, "index_create_sized_wait_wall", t["sized_wait"])
                res["classic_over_sized_wait"] = round(statistics.median(t["classic"]) / statistics.median(t["sized_wait"]), 2)
                res["sized_create_beats_classic"] = beats(t["sized_wait"], t["classic"])
                assert int(L.tsqa_decompress_ranges(codec.h, made.h, None, 0, filler.data_ptr(), 1, hs)) == 0, "the sized index was refused"
                emit(res)

            if "walk" in cases:
                back = torch.empty(n, dtype=torch.uint8, device="cuda")

                def one_workgroup():
                    rc = L.tsqa_decompress_device_sized_async(codec.h, blob.data_ptr(), size, nb, table.data_ptr(), back.data_ptr(), n, d_size,
                                                              d_status, hs)
                    assert rc == 0, codec.last_error()
                    s.synchronize()
                    _, _, dec_ms, dec_n = codec.profile_read()
                    _, _, call_ms, call_n = codec.profile_read_calls()
                    assert dec_n >= 1 and call_n == 1 and codec.status() == 0
                    return call_ms - dec_ms

                def three_launches():
                    """-> (the device's span, the filler's, the host's enqueue)"""
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    e[0].record(s)
                    filler.zero_()
                    e[1].record(s)
                    t0 = time.perf_counter()
                    sized_async()
                    host = (time.perf_counter() - t0) * 1e3
                    e[2].record(s)
                    e[2].synchronize()
                    return e[1].elapsed_time(e[2]), e[0].elapsed_time(e[1]), host

                codec.profile(True)
                codec.profile_read(), codec.profile_read_calls()
                t = in_turns({"one": one_workgroup, "three": three_launches})
                codec.profile(False)
                three = [x[0] for x in t["three"]]
                res = dict(base, case="walk", descriptor_fill_bytes=nb * 32, round_trip_ok=bool(torch.equal(back, src)))
                figures(res, "walk_one_workgroup", t["one"])
                figures(res, "walk_three_launches_with_fill", three)
                figures(res, "filler", [x[1] for x in t["three"]])
                figures(res, "sized_async_host_enqueue", [x[2] for x in t["three"]])
                res["host_hidden"] = bool(all(x[2] < x[1] for x in t["three"]))
                res["one_over_three"] = round(statistics.median(t["one"]) / statistics.median(three), 2)
                res["three_launch_beats_one_workgroup"] = beats(three, t["one"])
                emit(res)
                del back
            made.drop()
            del src, blob, table
            torch.cuda.empty_cache()
        del filler
        torch.cuda.empty_cache()

    # ---- record reads, and the chain ----
    if "records" in cases or "chain" in cases:
        n, R = args.record_mib * MiB, args.records
        data = tsq.synth.text(n, seed=5)
        src = torch.from_numpy(data).cuda()
        offs = np.random.default_rng(1).integers(0, n - 100, R).tolist()
        item_rr = tsq.api._item_range_array([(0, o, 100, 100 * k) for k, o in enumerate(offs)])
        want = np.concatenate([data[o:o + 100] for o in offs])
        out = torch.zeros(100 * R, dtype=torch.uint8, device="cuda")
        for log2 in [int(x) for x in args.record_block_lens.split(",")]:
            block_len = 1 << log2
            nb, bound, blob, table, size, compress = split_container(src, n, block_len)
            classic, sized_async, _ = creators(blob, bound, n, block_len, table)     # (the room, not the size)
            base = {"mib": args.record_mib, "bytes": n, "block_len": block_len, "blocks": nb, "records": R, "record_bytes": 100,
                    "blocks_touched": len({o // block_len for o in offs} | {(o + 99) // block_len for o in offs})}

            def read():
                rc = L.tsqa_decompress_item_ranges_async(codec.h, made.h, item_rr, R, out.data_ptr(), out.numel(), d_status, hs)
                assert rc == 0, codec.last_error()

            def checked(ms):
                assert codec.status() == 0 and np.array_equal(out.cpu().numpy(), want), "a record read gave other bytes than the input's"
                out.zero_()
                return ms

            if "records" in cases:
                res = dict(base, case="records")
                for name, create in (("classic", classic), ("sized", sized_async)):
                    made.drop()
                    create()
                    s.synchronize()
                    figures(res, f"read_alone_{name}_index", in_turns({"read": lambda: checked(span(read))}, keep_index=True)["read"])
                t = in_turns({"classic": lambda: checked(wall(lambda: (classic(), read()))), "sized": lambda: checked(wall(lambda: (sized_async(), read())))})
                figures(res, "create_and_read_classic_wall", t["classic"])
                figures(res, "create_and_read_sized_wall", t["sized"])
                res["classic_over_sized"] = round(statistics.median(t["classic"]) / statistics.median(t["sized"]), 2)
                res["sized_create_beats_classic"] = beats(t["sized"], t["classic"])
                emit(res)

            if "chain" in cases:
                def chain_sized():
                    compress(), sized_async(), read()

                def chain_classic():
                    compress()
                    s.synchronize()                          # (tsqa_index_create reads the container on the context's own stream)
                    classic(), read()

                t = in_turns({"sized_span": lambda: checked(span(chain_sized)), "sized_wall": lambda: checked(wall(chain_sized)),
                              "classic_wall": lambda: checked(wall(chain_classic))})
                res = dict(base, case="chain")
                figures(res, "chain_sized_span", t["sized_span"])
                figures(res, "chain_sized_wall", t["sized_wall"])
                figures(res, "chain_classic_wall", t["classic_wall"])
                res["classic_over_sized"] = round(statistics.median(t["classic_wall"]) / statistics.median(t["sized_wall"]), 3)
                res["chain_sized_beats_classic"] = beats(t["sized_wall"], t["classic_wall"])
                emit(res)
            made.drop()
            del blob, table
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
