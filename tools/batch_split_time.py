"""Timing of the packed batch compress of short blocks (tsqa_compress_batch_packed_split_async) on synth text with extensions on,
align 16: per shape and block_len, in rounds in which the calls under comparison take turns,
  split        the new call
  packed       tsqa_compress_batch_packed_async on the same items (blocks of 4 MiB), the same commit
  loop         a loop of tsqa_compress_device_split_async per item on the same stream, into the places the new call's bound gives
  decompress   DeviceCodec.decompress_packed of the new call's arena (it measures, waits once, allocates nothing here, decodes): host time
and the arena bytes against the 4 MiB arena, the ratio's price.  Device events on one stream, warm-ups first, the median of --reps
with the minimum and maximum beside every figure.  One JSON line per (shape, block_len), printed and appended to --out
(profiles/batch_split_time.jsonl).  Shapes: 16 x 16 MiB, 64 x 16 MiB, 64 x 1 MiB, 1 024 x 1 MiB, and the 300 mixed items of
tools/batch_time.py.

  --kernels-only    one item of 2 x CUs blocks of 4 KiB through the new call a few times and nothing else, for a run under
                    `rocprofv3 --kernel-trace --stats`: every encode launch's blocks all belong to that item.  --kernel-stats CSV then
                    turns that run's kernel statistics into one line: the pack scan's span next to the encode launch's.
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
KERNELS = ("batch_pack_scan_packed_kernel", "enc_batch_kernel", "batch_enc_blocks_kernel", "batch_pack_copy_kernel")


def kernel_stats(path, emit):
    """rocprofv3's kernel statistics -> the average span of the pack scan and of the kernels around it"""
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            short = next((k for k in KERNELS if k in r["Name"]), None)
            if short:
                calls, total = rows.get(short, (0, 0))
                rows[short] = (calls + int(r["Calls"]), total + int(r["TotalDurationNs"]))
    avg = {k: round(t / c / 1e3, 2) for k, (c, t) in rows.items()}
    emit({"measurement": "kernel_stats", "source": "rocprofv3 --kernel-trace --stats, one item of 2 x CUs blocks of 4 KiB",
          "kernels": {k: {"calls": rows[k][0], "average_us": avg[k]} for k in sorted(rows)},
          "scan_below_encode": avg.get("batch_pack_scan_packed_kernel", 0) < avg.get("enc_batch_kernel", 0)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="16x16MiB,64x16MiB,64x1MiB,1024x1MiB,mixed_1B_9MiB")
    ap.add_argument("--block-lens", default="22,18,16,12", help="log2 of the block lengths")
    ap.add_argument("--no-loop", action="store_true", help="leave the loop of single calls out of the rounds (its columns read null)")
    ap.add_argument("--kernels-only", action="store_true", help="run the new call a few times on one item of 2 x CUs blocks and time nothing")
    ap.add_argument("--kernel-stats", default=None, help="a kernel statistics CSV of rocprofv3 to summarise; nothing runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_split_time.jsonl"), help="the JSON lines are appended to this file")
    args = ap.parse_args()

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, emit)

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
    ext, align = 1, 16
    d_size, d_status = codec._size.data_ptr(), codec._status.data_ptr()

    if args.kernels_only:
        n = 2 * torch.cuda.get_device_properties(0).multi_processor_count * 4096
        src = torch.from_numpy(tsq.synth.text(n, seed=5)).cuda()
        first, bound = tsq.plan_batch_split([(0, n)], n, 4096, align)
        out = torch.empty(bound, dtype=torch.uint8, device="cuda")
        d_offsets, d_sizes = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        table = torch.empty(first[-1], dtype=torch.int32, device="cuda")
        for _ in range(12):
            codec.compress_batch_packed_split_async(src, [(0, n)], ext, align, 4096, out, d_offsets, d_sizes, table)
        s.synchronize()
        assert codec.status() == 0
        return

    rng = np.random.default_rng(1)
    shapes = {"16x16MiB": [16 * MiB] * 16, "64x16MiB": [16 * MiB] * 64, "64x1MiB": [MiB] * 64, "1024x1MiB": [MiB] * 1024,
              "mixed_1B_9MiB": [int(x) for x in np.exp(rng.uniform(0, np.log(9 << 20), 300))]}

    def once(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        call()
        e1.record(s)
        e1.synchronize()
        assert codec.status() == 0, codec.status()
        return e0.elapsed_time(e1)

    def in_turns(calls):
        """-> one list of times per call; in every round each call runs once, in order"""
        times = [[] for _ in calls]
        for r in range(args.warmup + args.reps):
            for k, call in enumerate(calls):
                t = once(call)
                if r >= args.warmup:
                    times[k].append(t)
        return times

    med = lambda ts: round(statistics.median(ts), 4)
    spread = lambda ts: [round(min(ts), 4), round(max(ts), 4)]

    for name in args.shapes.split(","):
        lengths = shapes[name]
        total, n = sum(lengths), len(lengths)
        src = torch.from_numpy(tsq.synth.text(total, seed=5)).cuda()
        offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
        items = [(o, z) for o, z in zip(offs, lengths)]
        arr = tsq.api._batch_array([(o, z, 0, 0) for o, z in items])
        back = torch.empty(total + 16 * n, dtype=torch.uint8, device="cuda")
        d_offsets, d_sizes = torch.zeros(n + 1, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
        plain = torch.empty(sum(tsq.batch_bound(z) for z in lengths) + n * (align - 1), dtype=torch.uint8, device="cuda")

        def packed():
            rc = L.tsqa_compress_batch_packed_async(codec.h, src.data_ptr(), total, arr, n, ext, align, plain.data_ptr(), plain.numel(),
                                                    d_offsets.data_ptr(), d_sizes.data_ptr(), d_status, hs)
            assert rc == 0, codec.last_error()

        packed()
        s.synchronize()
        plain_used = int(d_offsets[n].item())

        for log2 in [int(x) for x in args.block_lens.split(",")]:
            block_len = 1 << log2
            first, bound = tsq.plan_batch_split(items, total, block_len, align)
            arena = torch.empty(bound, dtype=torch.uint8, device="cuda")
            table = torch.empty(first[-1], dtype=torch.int32, device="cuda")
            places, at = [], 0                               # the loop's places: each item's split bound, rounded up
            for z in lengths:
                places.append(at)
                at += -(-tsq.plan_split(z, block_len)[1] // align) * align

            def split():
                rc = L.tsqa_compress_batch_packed_split_async(codec.h, src.data_ptr(), total, arr, n, ext, align, block_len, arena.data_ptr(),
                                                              bound, d_offsets.data_ptr(), d_sizes.data_ptr(), table.data_ptr(), d_status, hs)
                assert rc == 0, codec.last_error()

            def loop():
                for (o, z), a, fb in zip(items, places, first):
                    rc = L.tsqa_compress_device_split_async(codec.h, src.data_ptr() + o, z, block_len, arena.data_ptr() + a, bound - a, d_size,
                                                            table.data_ptr() + 4 * fb, d_status, ext, hs)
                    assert rc == 0, codec.last_error()

            ts, tp, tl = in_turns([split, packed] + ([] if args.no_loop else [loop])) + ([[]] if args.no_loop else [])
            split()
            s.synchronize()
            used = int(d_offsets[n].item())
            td = []
            for r in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                views = codec.decompress_packed(arena[:used], d_offsets, d_sizes, align=align, out=back)
                torch.cuda.synchronize()
                if r >= args.warmup:
                    td.append((time.perf_counter() - t0) * 1e3)
            ok = all(bool(torch.equal(v, src[o:o + z])) for v, (o, z) in zip(views, items))
            gbps = lambda t: round(total / statistics.median(t) / 1e6, 2)
            emit({"input": "synth_text", "shape": name, "items": n, "bytes": total, "ext": ext, "align": align, "block_len": block_len,
                  "blocks": first[-1], "blocks_4mib": sum(-(-z // tsq.BLOCK_SZ) for z in lengths), "reps": args.reps, "warmup": args.warmup,
                  "split_ms": med(ts), "split_spread_ms": spread(ts), "split_gbps": gbps(ts),
                  "packed_4mib_ms": med(tp), "packed_4mib_spread_ms": spread(tp),
                  "loop_of_split_ms": med(tl) if tl else None, "loop_of_split_spread_ms": spread(tl) if tl else None,
                  "split_over_packed_4mib": round(statistics.median(ts) / statistics.median(tp), 4),
                  "split_over_loop": round(statistics.median(ts) / statistics.median(tl), 4) if tl else None,
                  "decompress_packed_host_ms": med(td), "decompress_packed_host_spread_ms": spread(td),
                  "arena_bytes": used, "arena_bytes_4mib": plain_used, "arena_over_4mib": round(used / plain_used, 4), "round_trip_ok": ok})
            del arena, table
        del src, back, plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
