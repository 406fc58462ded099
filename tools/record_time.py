"""Record-read timing (tsqa_index_create_batch + tsqa_decompress_item_ranges_async), device events around each call on a drained
device, warm-ups first, the median of --reps and the spread (min .. max); the two ways of a comparison alternate inside the loop.
  one_container   R ranges of 100 B at random offsets in ONE 16 MiB text container (4 blocks), R = 1, 16, 256, 2 000: the flat
                  tsqa_decompress_ranges_async (one workgroup per range, dec_range_kernel) against the item call on a one-item batch
                  index (one workgroup per touched block, dec_group_kernel)
  pages           2 000 records of 100 B from 4 096 x 64 KiB pages: the index creation (a synchronous call: host clock), the record
                  read, and tsqa_decompress_batch_async of the touched pages followed by one gather of the slices
  index_only      nothing but --reps creations of the index over --pages pages (for a kernel trace: the launches per creation do not
                  depend on --pages)
Prints one JSON line per measurement (and writes them to --out) with the source fingerprint; every read is checked against the input."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ext", type=int, default=1)
    ap.add_argument("--pages", type=int, default=4096)
    ap.add_argument("--cases", default="one_container,pages")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
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
    st = codec._status.data_ptr()
    fingerprint = tsq.source_fingerprint()
    lines = []

    def emit(res):
        res["source"] = fingerprint
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    def timed(ways):
        """ways: name -> enqueue().  -> name -> (median, min, max) ms; the ways take turns inside every repetition"""
        times = {k: [] for k in ways}
        for r in range(args.warmup + args.reps):
            for name, enqueue in ways.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                enqueue()
                e1.record(s)
                e1.synchronize()
                if codec.status() != 0:
                    raise SystemExit(f"{name}: device status {codec.status()}")
                if r >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        return {k: (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)) for k, v in times.items()}

    cases = args.cases.split(",")
    rng = np.random.default_rng(1)

    if "one_container" in cases:
        n = 16 << 20
        data = tsq.synth.text(n, seed=5)
        src = torch.from_numpy(data).cuda()
        blob = codec.compress(src, args.ext)
        flat = codec.index(blob)
        batch = codec.index_batch([blob])
        for R in (1, 16, 256, 2000):
            offs = rng.integers(0, n - 100, R).tolist()
            flat_rr = tsq.api._range_array([(o, 100, 100 * k) for k, o in enumerate(offs)])
            item_rr = tsq.api._item_range_array([(0, o, 100, 100 * k) for k, o in enumerate(offs)])
            out_a = torch.zeros(100 * R, dtype=torch.uint8, device="cuda")
            out_b = torch.zeros(100 * R, dtype=torch.uint8, device="cuda")

            def way_flat():
                rc = L.tsqa_decompress_ranges_async(codec.h, flat.h, flat_rr, R, out_a.data_ptr(), out_a.numel(), st, hs)
                assert rc == 0, codec.last_error()

            def way_items():
                rc = L.tsqa_decompress_item_ranges_async(codec.h, batch.h, item_rr, R, out_b.data_ptr(), out_b.numel(), st, hs)
                assert rc == 0, codec.last_error()

            t = timed({"ranges": way_flat, "item_ranges": way_items})
            want = np.concatenate([data[o:o + 100] for o in offs])
            ok = bool(np.array_equal(out_a.cpu().numpy(), want) and np.array_equal(out_b.cpu().numpy(), want))
            emit({"case": "one_container_16MiB", "ranges": R, "range_bytes": 100, "reps": args.reps,
                  "blocks_touched": len({o // tsq.BLOCK_SZ for o in offs} | {(o + 99) // tsq.BLOCK_SZ for o in offs}),
                  "ranges_ms": t["ranges"][0], "ranges_min_max_ms": t["ranges"][1:],
                  "item_ranges_ms": t["item_ranges"][0], "item_ranges_min_max_ms": t["item_ranges"][1:],
                  "ranges_over_item_ranges": round(t["ranges"][0] / t["item_ranges"][0], 2), "bytes_ok": ok})
        flat.close()
        batch.close()
        del src, blob

    if "pages" in cases or "index_only" in cases:
        page, n_pages = 1 << 16, args.pages
        data = tsq.synth.text(n_pages * page, seed=7)
        src = torch.from_numpy(data).cuda()
        blobs = codec.compress_batch([src[k * page:(k + 1) * page] for k in range(n_pages)], args.ext)
        arena, offs = codec._arena(blobs)
        spans = tsq.api._batch_array([(o, b.numel(), 0, 0) for o, b in zip(offs, blobs)])

        def create():
            h = C.c_void_p()
            rc = L.tsqa_index_create_batch(codec.h, arena.data_ptr(), arena.numel(), spans, n_pages, C.byref(h), None)
            assert rc == 0 and h, codec.last_error()
            return h

        walls = []
        for r in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = create()
            t1 = time.perf_counter()
            L.tsqa_index_destroy(h)
            if r >= args.warmup:
                walls.append((t1 - t0) * 1e3)
        emit({"case": "index_create_batch", "pages": n_pages, "page_bytes": page, "reps": args.reps,
              "create_ms": round(statistics.median(walls), 4), "create_min_max_ms": [round(min(walls), 4), round(max(walls), 4)]})

    if "pages" in cases:
        idx = codec.index_batch(blobs)
        R = 2000
        pages = rng.integers(0, n_pages, R).tolist()
        inside = rng.integers(0, page - 100, R).tolist()
        item_rr = tsq.api._item_range_array([(p, o, 100, 100 * k) for k, (p, o) in enumerate(zip(pages, inside))])
        out_a = torch.zeros(100 * R, dtype=torch.uint8, device="cuda")
        # the other way: the touched pages decoded whole, then one gather of the slices
        touched = sorted(set(pages))
        slot = {p: k for k, p in enumerate(touched)}
        ditems = tsq.api._batch_array([(offs[p], blobs[p].numel(), slot[p] * page, page) for p in touched])
        nbs = np.ones(len(touched), dtype=np.uint32)
        whole = torch.zeros(len(touched) * page, dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros(len(touched), dtype=torch.int64, device="cuda")
        gather = torch.from_numpy(np.concatenate([slot[p] * page + o + np.arange(100) for p, o in zip(pages, inside)]).astype(np.int64)).cuda()
        out_b = torch.zeros(100 * R, dtype=torch.uint8, device="cuda")

        def way_items():
            rc = L.tsqa_decompress_item_ranges_async(codec.h, idx.h, item_rr, R, out_a.data_ptr(), out_a.numel(), st, hs)
            assert rc == 0, codec.last_error()

        def way_batch():
            rc = L.tsqa_decompress_batch_async(codec.h, arena.data_ptr(), arena.numel(), ditems, nbs.ctypes.data, len(touched), whole.data_ptr(),
                                               whole.numel(), d_sizes.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()
            torch.index_select(whole, 0, gather, out=out_b)

        t = timed({"item_ranges": way_items, "batch_then_slice": way_batch})
        want = np.concatenate([data[p * page + o:p * page + o + 100] for p, o in zip(pages, inside)])
        ok = bool(np.array_equal(out_a.cpu().numpy(), want) and np.array_equal(out_b.cpu().numpy(), want))
        emit({"case": "records_from_pages", "pages": n_pages, "page_bytes": page, "records": R, "record_bytes": 100, "pages_touched": len(touched),
              "reps": args.reps, "item_ranges_ms": t["item_ranges"][0], "item_ranges_min_max_ms": t["item_ranges"][1:],
              "batch_then_slice_ms": t["batch_then_slice"][0], "batch_then_slice_min_max_ms": t["batch_then_slice"][1:],
              "batch_over_item_ranges": round(t["batch_then_slice"][0] / t["item_ranges"][0], 2), "bytes_ok": ok})
        idx.close()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
