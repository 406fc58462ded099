"""Timing of the packed compress whose item table is made on the device (tsqa_compress_batch_packed_tables_async) against the form
that takes its items from the host.  Text, extensions on, align 16, a tight cap_blocks, device events on one stream, warm-ups first,
the median of --reps with each rep's minimum and maximum kept.  One JSON line per measurement, printed and appended to --out
(profiles/tables_time.jsonl).  Shapes: text_4096x64KiB and text_1024x1MiB; the items' places are two int64 tables in device memory.

  compress row   (ii) tsqa_compress_batch_packed_async with host items, (i) the new call, (iv) the measure-only form of the new call
                 -- its measure and layout kernels alone --, then (ii) once more, alternating in one session; and (iii) what a caller
                 whose tables exist only on the device does without the new call: both tables to the host, a wait, the host items made
                 from them, then (ii); its events bracket the copies and the wait.  The line says whether (i)'s median lies inside
                 (ii)'s own min .. max, widened by (iv)'s median.
  --baseline-only   only (ii), which exists without the new call: the same tool times a checkout from before it (--tree DIR imports
                    turbosqueeze_amd from that checkout, built there; --label names it).
  --kernels-only    a few runs of the new call and nothing else, for a run under `rocprofv3 --kernel-trace --stats`; --kernel-stats CSV
                    then turns that run's kernel statistics into one line per shape-independent kernel: the three kernels the call adds
                    (measure, layout, descriptors) next to the encoder's.
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ("batch_measure_tables_kernel", "batch_layout_tables_kernel", "batch_enc_blocks_kernel")


def kernel_stats(path, emit, label):
    """rocprofv3's kernel statistics -> the average time of each new kernel and of the kernels around them"""
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            short = next((k for k in NEW_KERNELS + ("enc_batch_live_kernel", "batch_pack_scan_tables_kernel", "batch_pack_copy_kernel") if k in r["Name"]), None)
            if short:
                calls, total = rows.get(short, (0, 0))
                rows[short] = (calls + int(r["Calls"]), total + int(r["TotalDurationNs"]))
    emit({"measurement": "kernel_stats", "checkout": label, "source": "rocprofv3 --kernel-trace --stats, both shapes together",
          "kernels": {k: {"calls": c, "average_us": round(t / c / 1e3, 2)} for k, (c, t) in sorted(rows.items())},
          "new_kernels_per_call_us": round(sum(rows[k][1] / rows[k][0] for k in NEW_KERNELS if k in rows) / 1e3, 2)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-only", action="store_true", help="the host form only")
    ap.add_argument("--kernels-only", action="store_true", help="run the new call a few times and time nothing")
    ap.add_argument("--kernel-stats", default=None, help="a kernel statistics CSV of rocprofv3 to summarise; nothing runs")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import turbosqueeze_amd from (built there)")
    ap.add_argument("--label", default="branch", help="which checkout the lines belong to")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tables_time.jsonl"), help="the JSON lines are appended to this file")
    args = ap.parse_args()

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, emit, args.label)

    sys.path.insert(0, os.path.abspath(args.tree))
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

    def timed(call):
        times = []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            e1.synchronize()
            if r >= args.warmup:
                times.append(e0.elapsed_time(e1))
        return times

    med = lambda ts: round(statistics.median(ts), 3)
    spread = lambda ts: [round(min(ts), 3), round(max(ts), 3)]

    for name, lengths in (("text_4096x64KiB", [1 << 16] * 4096), ("text_1024x1MiB", [1 << 20] * 1024)):
        n, total = len(lengths), sum(lengths)
        src = torch.from_numpy(tsq.synth.text(total, seed=5)).cuda()
        in_at = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        d_at, d_len = torch.from_numpy(in_at).cuda(), torch.tensor(lengths, dtype=torch.int64, device="cuda")
        blocks = sum(-(-x // tsq.BLOCK_SZ) for x in lengths)
        room = sum(tsq.batch_bound(x) + align for x in lengths)
        arena, arena2 = (torch.empty(room, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_offsets, d_offsets2 = (torch.zeros(n + 1, dtype=torch.int64, device="cuda") for _ in range(2))
        d_sizes, d_sizes2 = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
        st = codec._status.data_ptr()
        res = {"shape": name, "checkout": args.label, "items": n, "bytes": total, "blocks": blocks, "reps": args.reps, "align": align, "ext": ext}

        def items_of(at, ln):
            quads = np.zeros((n, 4), dtype=np.uint64)                          # tsqa_batch_item: in_at, in_len, out_at, out_cap
            quads[:, 0], quads[:, 1] = at, ln
            return quads

        host_items = items_of(in_at, lengths)

        def host_form(items=host_items):
            rc = L.tsqa_compress_batch_packed_async(codec.h, src.data_ptr(), total, items.ctypes.data, n, ext, align, arena.data_ptr(), room,
                                                    d_offsets.data_ptr(), d_sizes.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        if args.baseline_only:
            a = timed(host_form)
            emit({**res, "measurement": "compress_baseline", "host_form_ms": med(a), "host_form_spread_ms": spread(a)})
            del src, arena, arena2
            torch.cuda.empty_cache()
            continue

        d_first = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_bound = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_item_status = torch.zeros(n, dtype=torch.int32, device="cuda")

        def tables(out=arena2, cap=blocks):
            rc = L.tsqa_compress_batch_packed_tables_async(codec.h, src.data_ptr(), total, d_at.data_ptr(), d_len.data_ptr(), n, cap, ext, align,
                                                           out.data_ptr() if out is not None else None, room if out is not None else 0,
                                                           d_offsets2.data_ptr(), d_sizes2.data_ptr(), d_first.data_ptr(), d_bound.data_ptr(),
                                                           d_item_status.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        if args.kernels_only:
            for _ in range(args.warmup + args.reps):
                tables()
            s.synchronize()
            continue

        def today():
            at, ln = d_at.cpu().numpy(), d_len.cpu().numpy()                   # (each .cpu() waits for the stream)
            host_form(items_of(at, ln))

        before = timed(host_form)
        t = timed(tables)
        s.synchronize()
        used = int(d_offsets[n].item())
        ok = (not bool(d_item_status.any()) and codec.status() == 0 and torch.equal(d_offsets, d_offsets2) and torch.equal(d_sizes, d_sizes2) and
              bool(torch.equal(arena[:used], arena2[:used])) and int(d_first[n].item()) == blocks and used <= int(d_bound.item()) <= room)
        m = timed(lambda: tables(None, 0))
        after = timed(host_form)
        u = timed(today)
        base = before + after
        lo, hi = min(base), max(base) + statistics.median(m)
        emit({**res, "measurement": "compress", "host_form_ms": med(base), "host_form_spread_ms": spread(base), "tables_ms": med(t),
              "tables_spread_ms": spread(t), "measure_and_layout_alone_ms": med(m), "measure_and_layout_spread_ms": spread(m),
              "tables_to_host_then_host_form_ms": med(u), "tables_to_host_then_host_form_spread_ms": spread(u),
              "tables_over_host_form": round(statistics.median(t) / statistics.median(base), 3), "tables_equal_host_form": ok,
              "tables_inside_host_form_spread_plus_new_kernels": lo <= statistics.median(t) <= hi})
        del src, arena, arena2
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
