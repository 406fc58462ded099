"""Timing of the index of a packed batch made from its device tables (tsqa_index_create_packed_async) against the path there was
before it: copy d_offsets and d_sizes to the host, wait, tsqa_index_create_batch, then gather.  synth text, extensions on.  Warm-ups
first, then --reps rounds in which the ways under comparison take turns; the median of the reps with their minimum and maximum
beside every figure.  One JSON line per measurement, printed and appended to --out (profiles/packed_index_time.jsonl), with the
source fingerprint.  --ways host runs the host path alone and touches no entry point younger than tsqa_gather_async, so the same
file measures the parent commit's library when it is started from a checkout of that commit.

  records   --items items of --item-kib KiB in one packed arena (4 MiB blocks: one block per item).  The index alone, and the index
            followed by a gather of --records records of 100 B whose item numbers lie in device memory.  Host clock from the first
            call to the end of the stream (what a caller waits), and for the device path also the event span on the stream.
  blocks    --big-items items of --big-mib MiB at each of --block-lens: the plain form (one lane walks an item's frames one after
            the other), the sized form (one lane per block, from the size table the compress left) and the host path; index alone.
  tiny      --tiny-items containers of one byte: what the one-workgroup scans over the items cost shows here, where nothing else
            has work.  The plain form's event span, and the host path's clock.

*_beats_* says whether a median beats the other way's by more than that way's own spread (max - min of its reps)."""
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
    ap.add_argument("--items", type=int, default=4096)
    ap.add_argument("--item-kib", type=int, default=64)
    ap.add_argument("--records", type=int, default=2000)
    ap.add_argument("--big-items", type=int, default=16)
    ap.add_argument("--big-mib", type=int, default=16)
    ap.add_argument("--block-lens", default="12,16", help="log2 of the block lengths of the blocks case")
    ap.add_argument("--tiny-items", type=int, default=262144)
    ap.add_argument("--cases", default="records,blocks,tiny")
    ap.add_argument("--ways", default="host,device", help="host: the path there was before; device: tsqa_index_create_packed_async")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "packed_index_time.jsonl"), help="the JSON lines are appended to this file")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import turbosqueeze_amd as tsq
    from turbosqueeze_amd.api import _batch_array

    torch.cuda.set_device(0)
    codec = tsq.DeviceCodec(0)
    L = codec.L
    # a stream of its own: the library takes a NULL stream (torch's default) as the context's own, which torch's events do not see
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    hs = C.c_void_p(s.cuda_stream)
    fingerprint = tsq.source_fingerprint()
    cases, ways = args.cases.split(","), args.ways.split(",")

    def emit(res):
        res.update(source=fingerprint, reps=args.reps, warmup=args.warmup, ext=1, input="synth_text", ways=ways)
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    made = []

    def drop():
        while made:
            L.tsqa_index_destroy(made.pop())

    def in_turns(calls):
        """calls: name -> call() -> ms.  The indexes of the calls before are destroyed in front of every call, outside what is timed
        (hipFree waits for the device)."""
        times = {k: [] for k in calls}
        for r in range(args.warmup + args.reps):
            for name, call in calls.items():
                drop()
                torch.cuda.synchronize()
                t = call()
                if r >= args.warmup:
                    times[name].append(t)
        drop()
        return times

    med = lambda ts: round(statistics.median(ts), 4)
    spread = lambda ts: [round(min(ts), 4), round(max(ts), 4)]
    beats = lambda new, old: bool(statistics.median(old) - statistics.median(new) > max(old) - min(old))

    def figures(res, t):
        for name, ts in t.items():
            res[name + "_ms"], res[name + "_spread_ms"] = med(ts), spread(ts)

    def wall(call):
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

    def host_index(arena, d_offsets, d_sizes, n):
        """the path there was before: the tables come to the host (a copy and a wait), then tsqa_index_create_batch, which runs on
        the context's own stream and waits twice"""
        places = torch.stack([d_offsets[:n], d_sizes[:n]]).cpu().tolist()
        h = C.c_void_p()
        rc = L.tsqa_index_create_batch(codec.h, arena.data_ptr(), arena.numel(), _batch_array([(a, z, 0, 0) for a, z in zip(*places)]), n,
                                       C.byref(h), None)
        assert rc == 0 and h, codec.last_error()
        made.append(h)
        return h

    def device_index(arena, d_offsets, d_sizes, n, cap, block_len=0, d_first=None, table=None):
        h = C.c_void_p()
        rc = L.tsqa_index_create_packed_async(codec.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(), n, cap, block_len,
                                              d_first.data_ptr() if table is not None else None, table.data_ptr() if table is not None else None,
                                              table.numel() if table is not None else 0, C.byref(h), None, codec._status.data_ptr(), hs)
        assert rc == 0 and h, codec.last_error()
        made.append(h)
        return h

    def packed(data, sizes, block_len=None):
        """the items laid end to end in `data`, compressed into a packed arena from device tables -> (the PackedBatch, and its two
        tables in device memory, as a consumer receives them)"""
        at = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        batch = codec.compress_packed_tables(data, torch.from_numpy(at).cuda(), torch.from_numpy(np.asarray(sizes, dtype=np.int64)).cuda(), 1,
                                             block_len=block_len)
        i64 = lambda values: torch.tensor(values, dtype=torch.int64, device="cuda")
        tables = i64(batch.offsets), i64(batch.sizes)
        s.synchronize()
        return batch, tables[0], tables[1]

    # ---- many items of one block: the index alone, and index + gather ----
    if "records" in cases:
        n, size, R = args.items, args.item_kib << 10, args.records
        host = tsq.synth.text(n * size, seed=5)
        data = torch.from_numpy(host).cuda()
        batch, d_offsets, d_sizes = packed(data, [size] * n)
        arena = batch.arena
        rng = np.random.default_rng(1)
        items, offs = rng.integers(0, n, R), rng.integers(0, size - 100, R)
        d_items = torch.from_numpy(items.astype(np.int32)).cuda()
        d_off, d_len = torch.from_numpy(offs.astype(np.int64)).cuda(), torch.full((R,), 100, dtype=torch.int64, device="cuda")
        out = torch.zeros(100 * R, dtype=torch.uint8, device="cuda")
        d_out_offsets, d_rs = torch.empty(R + 1, dtype=torch.int64, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda")
        d_need = torch.empty(1, dtype=torch.int64, device="cuda")
        want = np.concatenate([host[i * size + o:i * size + o + 100] for i, o in zip(items.tolist(), offs.tolist())])

        def gather(h):
            rc = L.tsqa_gather_async(codec.h, h, d_items.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), R, 1, 2 * R, out.data_ptr(), out.numel(),
                                     d_out_offsets.data_ptr(), d_rs.data_ptr(), d_need.data_ptr(), codec._status.data_ptr(), hs)
            assert rc == 0, codec.last_error()

        def checked(ms):
            assert codec.status() == 0 and np.array_equal(out.cpu().numpy(), want), "the gather gave other bytes than the input's"
            out.zero_()
            return ms

        calls = {}
        if "host" in ways:
            calls["index_host_path_wall"] = lambda: wall(lambda: host_index(arena, d_offsets, d_sizes, n))
            calls["index_and_gather_host_path_wall"] = lambda: checked(wall(lambda: gather(host_index(arena, d_offsets, d_sizes, n))))
        if "device" in ways:
            calls["index_device_wall"] = lambda: wall(lambda: device_index(arena, d_offsets, d_sizes, n, n))
            calls["index_device_span"] = lambda: span(lambda: device_index(arena, d_offsets, d_sizes, n, n))
            calls["index_and_gather_device_wall"] = lambda: checked(wall(lambda: gather(device_index(arena, d_offsets, d_sizes, n, n))))
            calls["index_and_gather_device_span"] = lambda: checked(span(lambda: gather(device_index(arena, d_offsets, d_sizes, n, n))))
        t = in_turns(calls)
        res = dict(case="records", items=n, item_bytes=size, blocks=n, records=R, record_bytes=100, arena_bytes=arena.numel())
        figures(res, t)
        if "host" in ways and "device" in ways:
            res["index_device_beats_host_path"] = beats(t["index_device_wall"], t["index_host_path_wall"])
            res["index_and_gather_device_beats_host_path"] = beats(t["index_and_gather_device_wall"], t["index_and_gather_host_path_wall"])
        emit(res)
        del data, batch, arena
        torch.cuda.empty_cache()

    # ---- few items of many short blocks: the walk ----
    if "blocks" in cases:
        n, size = args.big_items, args.big_mib * MiB
        data = torch.from_numpy(tsq.synth.text(n * size, seed=6)).cuda()
        for log2 in [int(x) for x in args.block_lens.split(",")]:
            block_len = 1 << log2
            batch, d_offsets, d_sizes = packed(data, [size] * n, block_len)
            arena, cap = batch.arena, batch.first_block[-1]
            calls = {}
            if "host" in ways:
                calls["index_host_path_wall"] = lambda: wall(lambda: host_index(arena, d_offsets, d_sizes, n))
            if "device" in ways:
                d_first = torch.tensor(batch.first_block, dtype=torch.int64, device="cuda")
                table = batch.d_block_sizes
                for name, extra in (("plain", ()), ("sized", (block_len, d_first, table))):
                    calls[f"index_{name}_wall"] = lambda extra=extra: wall(lambda: device_index(arena, d_offsets, d_sizes, n, cap, *extra))
                    calls[f"index_{name}_span"] = lambda extra=extra: span(lambda: device_index(arena, d_offsets, d_sizes, n, cap, *extra))
            t = in_turns(calls)
            res = dict(case="blocks", items=n, item_bytes=size, block_len=block_len, blocks=cap, frames_per_item=cap // n, arena_bytes=arena.numel())
            figures(res, t)
            if "device" in ways:
                res["sized_beats_plain"] = beats(t["index_sized_span"], t["index_plain_span"])
                if "host" in ways:
                    res["plain_beats_host_path"] = beats(t["index_plain_wall"], t["index_host_path_wall"])
                    res["sized_beats_host_path"] = beats(t["index_sized_wall"], t["index_host_path_wall"])
            emit(res)
            del batch, arena
            torch.cuda.empty_cache()
        del data

    # ---- very many items of one byte: the scans over the items ----
    if "tiny" in cases:
        n = args.tiny_items
        one = codec.compress(torch.full((1,), 65, dtype=torch.uint8, device="cuda"), 1)
        pitch = -(-one.numel() // 16) * 16
        cell = torch.zeros(pitch, dtype=torch.uint8, device="cuda")
        cell[:one.numel()] = one
        arena = cell.repeat(n)
        d_offsets = torch.arange(n, dtype=torch.int64, device="cuda") * pitch
        d_sizes = torch.full((n,), one.numel(), dtype=torch.int64, device="cuda")
        s.synchronize()
        calls = {}
        if "host" in ways:
            calls["index_host_path_wall"] = lambda: wall(lambda: host_index(arena, d_offsets, d_sizes, n))
        if "device" in ways:
            calls["index_device_wall"] = lambda: wall(lambda: device_index(arena, d_offsets, d_sizes, n, n))
            calls["index_device_span"] = lambda: span(lambda: device_index(arena, d_offsets, d_sizes, n, n))
        t = in_turns(calls)
        res = dict(case="tiny", items=n, item_bytes=1, blocks=n, container_bytes=one.numel(), scan_passes=-(-n // 256))
        figures(res, t)
        emit(res)


if __name__ == "__main__":
    main()
