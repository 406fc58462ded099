"""Timing of the dense decompress of a packed batch (tsqa_decompress_batch_packed_dense_async: block counts and output places made on
the device from the headers) against the forms that take the same facts from the host.  Text, extensions on, align 16, device events
on one stream, warm-ups first, the median of --reps with each rep's minimum and maximum kept.  One JSON line per measurement,
printed and appended to --out (profiles/dense_time.jsonl).  Shapes: text_4096x64KiB and text_1024x1MiB, packed by
tsqa_compress_batch_packed_async.

  async row   tsqa_decompress_batch_packed_items_async with host-known block counts and places, the dense call, the dense call's two
              new kernels alone (the measure-only form), then the per-item form once more, alternating in one session.  The line says
              whether the dense median lies inside the per-item reps' own min .. max, widened by the new kernels' median.
  sync row    DeviceCodec.decompress_batch over the containers (header gather to the host, numpy parsing, then the decode) against
              DeviceCodec.decompress_packed (measure, one read of two words, decode).  The events bracket the whole call, host waits
              included.
  --baseline-only   only what exists without the dense call (the per-item form and decompress_batch): the same tool times a checkout
                    from before it (--tree DIR imports turbosqueeze_amd from that checkout, built there; --label names it).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-only", action="store_true", help="the existing entry points only")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import turbosqueeze_amd from (built there)")
    ap.add_argument("--label", default="branch", help="which checkout the lines belong to")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_time.jsonl"), help="the JSON lines are appended to this file")
    args = ap.parse_args()
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

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

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
        in_at = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
        arena = torch.empty(sum(tsq.batch_bound(x) + align for x in lengths), dtype=torch.uint8, device="cuda")
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
        codec.compress_batch_packed_async(src, list(zip(in_at, lengths)), ext, align, arena, d_offsets, d_sizes)
        s.synchronize()
        assert codec.status() == 0
        nbs = np.array([-(-x // tsq.BLOCK_SZ) for x in lengths], dtype=np.uint32)
        blocks = int(nbs.sum())
        back = torch.zeros(total, dtype=torch.uint8, device="cuda")          # (every length is a multiple of align: the dense places are in_at)
        quads = tsq.api._batch_array([(0, 0, a, x) for a, x in zip(in_at, lengths)])
        d_out_sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_item_status = torch.zeros(n, dtype=torch.int32, device="cuda")
        st = codec._status.data_ptr()
        res = {"shape": name, "checkout": args.label, "items": n, "bytes": total, "blocks": blocks, "reps": args.reps, "align": align}

        def per_item():
            rc = L.tsqa_decompress_batch_packed_items_async(codec.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(), quads,
                                                            nbs.ctypes.data, n, back.data_ptr(), back.numel(), d_out_sizes.data_ptr(),
                                                            d_item_status.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        host_offsets = d_offsets.cpu().tolist()
        blobs = [arena[o:o + z] for o, z in zip(host_offsets, d_sizes.cpu().tolist())]

        def gather_decode():
            codec.decompress_batch(blobs, out=back)

        if args.baseline_only:
            a = timed(per_item)
            emit({**res, "measurement": "async_baseline", "per_item_ms": med(a), "per_item_spread_ms": spread(a)})
            g = timed(gather_decode)
            emit({**res, "measurement": "sync_baseline", "decompress_batch_ms": med(g), "decompress_batch_spread_ms": spread(g)})
            del src, arena, back, blobs
            torch.cuda.empty_cache()
            continue

        d_out_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_first_block = torch.zeros(n + 1, dtype=torch.int64, device="cuda")

        def dense(out=back, cap=blocks):
            rc = L.tsqa_decompress_batch_packed_dense_async(codec.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(), n, align,
                                                            cap, out.data_ptr() if out is not None else None, out.numel() if out is not None else 0,
                                                            d_out_offsets.data_ptr(), d_out_sizes.data_ptr(), d_first_block.data_ptr(),
                                                            d_item_status.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        before = timed(per_item)
        back.zero_()
        d = timed(dense)
        s.synchronize()
        ok = bool(torch.equal(back, src)) and not bool(d_item_status.any()) and codec.status() == 0 and d_out_offsets.cpu().tolist() == in_at + [total]
        m = timed(lambda: dense(None, 0))
        after = timed(per_item)
        base = before + after
        lo, hi = min(base), max(base) + statistics.median(m)
        emit({**res, "measurement": "async", "per_item_ms": med(base), "per_item_spread_ms": spread(base), "dense_ms": med(d),
              "dense_spread_ms": spread(d), "measure_and_layout_alone_ms": med(m), "measure_and_layout_spread_ms": spread(m),
              "dense_over_per_item": round(statistics.median(d) / statistics.median(base), 3), "dense_round_trip_ok": ok,
              "dense_inside_per_item_spread_plus_new_kernels": lo <= statistics.median(d) <= hi})

        g = timed(gather_decode)
        back.zero_()
        p = timed(lambda: codec.decompress_packed(arena, d_offsets[:n], d_sizes, align=align, out=back))
        s.synchronize()
        emit({**res, "measurement": "sync", "decompress_batch_ms": med(g), "decompress_batch_spread_ms": spread(g), "decompress_packed_ms": med(p),
              "decompress_packed_spread_ms": spread(p), "decompress_packed_over_decompress_batch": round(statistics.median(p) / statistics.median(g), 3),
              "decompress_packed_round_trip_ok": bool(torch.equal(back, src))})
        del src, arena, back, blobs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
