"""Batch timing: one tsqa_*_batch_async call against a loop of single-item tsqa_*_device_async calls on one stream, device events around
each, warm-ups first, the median of --reps.  Shapes (text):
  text_4096x64KiB     4 096 items of 64 KiB
  text_1024x1MiB      1 024 items of 1 MiB
  mixed_1B_9MiB       300 items of 1 B ... 9 MiB (log-uniform)
Prints one JSON line per shape (and writes them to --out): compress / decompress milliseconds of both ways, their ratio, and whether
the batch's bytes equal the loop's.  The loop's items get the same input and output offsets as the batch's.
The packed column per shape (one more JSON line each, written to --packed-out, profiles/packed_time.jsonl unless --no-packed):
tsqa_compress_batch_packed_async into a dense arena; the route to the same arena without it (the unpacked tsqa_compress_batch_async, a
synchronise, the sizes read back, torch.cat of the trimmed views); the unpacked compress alone before and after, whose reps give the
run-to-run spread; the arena bytes used against the unpacked arena.  --only-packed skips the loops and the decompress side.  The packed
call does strictly less than the dense route: the tool ends with status 1, its lines written, when a shape's packed median is above
its dense route's.  profiles/packed_time.jsonl is `python tools/batch_time.py --only-packed`."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ext", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--packed-out", default=os.path.join(ROOT, "profiles", "packed_time.jsonl"), help="the packed column's JSON lines go to this file")
    ap.add_argument("--no-packed", action="store_true", help="skip the packed column")
    ap.add_argument("--only-packed", action="store_true", help="skip the single-call loops and the decompress side")
    ap.add_argument("--align", type=int, default=16, help="alignment of the packed containers")
    args = ap.parse_args()
    if args.no_packed:
        args.packed_out = None
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
    rng = np.random.default_rng(1)
    shapes = {
        "text_4096x64KiB": [1 << 16] * 4096,
        "text_1024x1MiB": [1 << 20] * 1024,
        "mixed_1B_9MiB": [int(x) for x in np.exp(rng.uniform(0, np.log(9 << 20), 300))],
    }

    def timed(enqueue, spread=None):
        times = []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            enqueue()
            e1.record(s)
            e1.synchronize()
            if codec.status() != 0:
                raise SystemExit(f"device status {codec.status()}")
            if r >= args.warmup:
                times.append(e0.elapsed_time(e1))
        if spread is not None:
            spread.extend(times)
        return round(statistics.median(times), 3)

    def packed_column(name, lengths, src, items, arr, out, d_sizes, caps):
        """the packed call, today's dense route and the unpacked compress alone (before and after), alternating"""
        n, st = len(items), codec._status.data_ptr()
        arena = torch.zeros(sum(caps) + n * (args.align - 1), dtype=torch.uint8, device="cuda")
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_psizes = torch.zeros(n, dtype=torch.int64, device="cuda")
        dense = {}

        def unpacked():
            rc = L.tsqa_compress_batch_async(codec.h, src.data_ptr(), src.numel(), arr, n, args.ext, out.data_ptr(), out.numel(),
                                             d_sizes.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        def packed(align=args.align):
            rc = L.tsqa_compress_batch_packed_async(codec.h, src.data_ptr(), src.numel(), arr, n, args.ext, align, arena.data_ptr(), arena.numel(),
                                                    d_offsets.data_ptr(), d_psizes.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        def route():
            unpacked()
            s.synchronize()
            sizes = d_sizes.cpu().tolist()
            dense["arena"] = torch.cat([out[a:a + z] for (_, _, a, _), z in zip(items, sizes)])

        res = {"shape": name, "items": n, "bytes": sum(lengths), "reps": args.reps, "align": args.align}
        before, after = [], []
        res["unpacked_ms"] = timed(unpacked, before)
        res["packed_ms"] = timed(packed)
        res["dense_route_ms"] = timed(route)
        res["unpacked_again_ms"] = timed(unpacked, after)
        # the packed call against the unpacked compress alone, and the unpacked reps' own spread about their median (both runs pooled)
        pooled = statistics.median(before + after)
        res["unpacked_spread_ms"] = [round(min(before + after), 3), round(max(before + after), 3)]
        res["unpacked_spread_over_median"] = [round(min(before + after) / pooled, 3), round(max(before + after) / pooled, 3)]
        res["packed_over_unpacked"] = round(res["packed_ms"] / pooled, 3)
        res["packed_exceeds_unpacked_spread"] = res["packed_ms"] > max(before + after)
        res["packed_over_dense_route"] = round(res["packed_ms"] / res["dense_route_ms"], 3)
        res["packed_not_slower_than_dense_route"] = res["packed_ms"] <= res["dense_route_ms"]
        offsets = d_offsets.cpu().tolist()
        res["arena_used_bytes"] = offsets[-1]
        res["arena_unpacked_bytes"] = sum(caps)
        res["arena_used_over_unpacked"] = round(offsets[-1] / sum(caps), 4)
        res["offsets_follow_plan"] = offsets == tsq.plan_packed(d_psizes.cpu().tolist(), args.align)
        # align 1 gives the very arena of the dense route
        packed(1)
        s.synchronize()
        res["same_bytes_as_dense_route"] = bool(torch.equal(arena[:int(d_offsets[-1])], dense["arena"]))
        return res

    lines, packed_lines, slower = [], [], 0
    for name, lengths in shapes.items():
        total = sum(lengths)
        src = torch.from_numpy(tsq.synth.text(total, seed=5)).cuda()
        offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
        caps = [tsq.batch_bound(n) for n in lengths]
        out_at = np.concatenate([[0], np.cumsum(caps)[:-1]]).tolist()
        out = torch.zeros(sum(caps), dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros(len(lengths), dtype=torch.int64, device="cuda")
        items = [(o, n, a, c) for o, n, a, c in zip(offs, lengths, out_at, caps)]
        arr = tsq.api._batch_array(items)
        st, sz = codec._status.data_ptr(), codec._size.data_ptr()

        def batch_c():
            rc = L.tsqa_compress_batch_async(codec.h, src.data_ptr(), src.numel(), arr, len(items), args.ext, out.data_ptr(), out.numel(),
                                             d_sizes.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        def loop_c():
            for o, n, a, c in items:
                rc = L.tsqa_compress_device_async(codec.h, src.data_ptr() + o, n, out.data_ptr() + a, c, sz, st, args.ext, hs)
                assert rc == 0, codec.last_error()

        if args.packed_out:
            col = packed_column(name, lengths, src, items, arr, out, d_sizes, caps)
            slower += not col["packed_not_slower_than_dense_route"]
            packed_lines.append(json.dumps(col))
            print(packed_lines[-1], flush=True)
            if args.only_packed:
                del src, out
                torch.cuda.empty_cache()
                continue
        res = {"shape": name, "items": len(lengths), "bytes": total, "blocks": sum(-(-n // tsq.BLOCK_SZ) for n in lengths), "reps": args.reps}
        res["compress_loop_ms"] = timed(loop_c)
        loop_bytes = out.clone()
        out.zero_()
        res["compress_batch_ms"] = timed(batch_c)
        res["compress_same_bytes"] = bool(torch.equal(out, loop_bytes))
        sizes = d_sizes.cpu().tolist()
        res["ratio"] = round(sum(sizes) / total, 4)
        # decompress the containers where they lie
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")
        ditems = [(a, z, o, n) for a, z, o, n in zip(out_at, sizes, offs, lengths)]
        darr = tsq.api._batch_array(ditems)
        nbs = np.array([-(-n // tsq.BLOCK_SZ) for n in lengths], dtype=np.uint32)

        def batch_d():
            rc = L.tsqa_decompress_batch_async(codec.h, out.data_ptr(), out.numel(), darr, nbs.ctypes.data, len(ditems), back.data_ptr(),
                                               back.numel(), d_sizes.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        def loop_d():
            for (a, z, o, n), nb in zip(ditems, nbs.tolist()):
                rc = L.tsqa_decompress_device_async(codec.h, out.data_ptr() + a, z, nb, back.data_ptr() + o, n, sz, st, hs)
                assert rc == 0, codec.last_error()

        res["decompress_loop_ms"] = timed(loop_d)
        loop_ok = bool(torch.equal(back, src))
        back.zero_()
        res["decompress_batch_ms"] = timed(batch_d)
        res["decompress_round_trip_ok"] = loop_ok and bool(torch.equal(back, src))
        res["compress_speedup"] = round(res["compress_loop_ms"] / res["compress_batch_ms"], 2)
        res["decompress_speedup"] = round(res["decompress_loop_ms"] / res["decompress_batch_ms"], 2)
        res["compress_batch_GBps"] = round(total / res["compress_batch_ms"] / 1e6, 2)
        res["decompress_batch_GBps"] = round(total / res["decompress_batch_ms"] / 1e6, 2)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del src, out, back
        torch.cuda.empty_cache()
    if args.out and lines:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.packed_out:
        with open(args.packed_out, "w") as f:
            f.write("\n".join(packed_lines) + "\n")
    if slower:
        raise SystemExit(f"the packed call is slower than the dense route on {slower} shape(s)")


if __name__ == "__main__":
    main()
