"""Timing of the gather into fixed-stride padded rows (tsqa_gather_rows_async) against the route there was before it.  Per shape,
with the offsets and lengths (and items) in device tensors, the median of --reps and the spread (min .. max) of
  rows          tsqa_gather_rows_async alone, pad 0: host clock from the call to the end of the stream, and device events around it
  old_route     the same rows as a user had to make them: tsqa_gather_async into a dense buffer, hipMemsetAsync of the padded
                tensor, and a torch scatter of every dense byte to its row from d_out_offsets (searchsorted for the row, a subtraction
                for the column, an indexed store); nothing waited for in between: host clock and device events
  spans         the profile kinds: the planner's launches of either call on the same ranges, the decode kernel of either, and the
                pad kernel, whose rate (bytes it writes per second) stands next to the copy probe's for as many bytes written
The two routes alternate inside the loop, on a drained device, warm-ups first.  Shapes (tools/gather_time.py's):
  text_12, text_16   2 000 records of 100 B out of 64 MiB of text cut every 2^12, 2^16 bytes (a sized index), rows of 128 B
  pages              2 000 records of 100 B out of 4 096 pages of 64 KiB (a batch index, addressed by item), rows of 128 B
  big                200 000 records of 100 B out of 1 GiB cut every 2^12, rows of 128 B
  whole              the 4 096 pages as whole items, truncated to rows of 4 096 B (no offsets, no lengths)
Prints one JSON line per measurement (and writes them to --out) with the source fingerprint; every image is checked against the input."""
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ext", type=int, default=1)
    ap.add_argument("--cases", default="text_12,text_16,pages,big,whole")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import turbosqueeze_amd as tsq

    torch.cuda.set_device(0)
    codec = tsq.DeviceCodec(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    # a stream of its own: the library takes a NULL stream (torch's default) as the context's own, which torch's events do not see
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    hs = C.c_void_p(s.cuda_stream)
    fingerprint = tsq.source_fingerprint()
    lines = []
    rng = np.random.default_rng(3)

    def emit(res):
        res["source"] = fingerprint
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    def stats(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    def measure(name, idx, items, offsets, lengths, stride, truncate, starts, cap_pieces, data, extra):
        """items: None or a uint32 array; offsets, lengths: None or int64 arrays; starts: where each row's bytes start in `data`"""
        n = len(starts)
        dev = lambda a, view=None: None if a is None else torch.from_numpy(a if view is None else a.view(view)).cuda()
        d_items, d_off, d_len = dev(items, np.int32), dev(offsets), dev(lengths)
        want_len = np.minimum(lengths, stride) if lengths is not None else np.full(n, stride, dtype=np.int64)
        # the old route has no NULL tables and no truncation: it is given the lengths the rows deliver
        o_off = d_off if d_off is not None else torch.zeros(n, dtype=torch.int64, device="cuda")
        o_len = torch.from_numpy(want_len).cuda()
        room = int(want_len.sum())
        rows = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
        dense, padded = torch.empty(room, dtype=torch.uint8, device="cuda"), torch.empty(n * stride, dtype=torch.uint8, device="cuda")
        d_row_lengths, d_out_offsets = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_status, d_need = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
        pos = torch.arange(room, dtype=torch.int64, device="cuda")
        flags = tsq.api.ROWS_TRUNCATE if truncate else 0
        codec.profile(True)
        codec.profile_read_gather(); codec.profile_read_rows()
        keys = ("rows_wall", "rows_events", "old_route_wall", "old_route_events", "rows_plan_span", "dense_plan_span", "rows_decode_span",
                "dense_decode_span", "pad_span", "old_gather_events", "old_memset_events", "old_scatter_events")
        t = {k: [] for k in keys}
        for r in range(args.warmup + args.reps):
            keep = r >= args.warmup
            # (a) the rows
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(s)
            codec.gather_rows_async(idx, d_items, d_off, d_len, n, stride, flags, 0, cap_pieces, rows, d_row_lengths, d_status, d_need)
            e1.record(s)
            s.synchronize()
            t1 = time.perf_counter()
            if codec.status() != 0:
                raise SystemExit(f"{name}: rows: device status {codec.status()}")
            plan_ms, _, dec_ms, _ = codec.profile_read_gather()
            pad_ms, _ = codec.profile_read_rows()
            if keep:
                t["rows_wall"].append((t1 - t0) * 1e3); t["rows_events"].append(e0.elapsed_time(e1))
                t["rows_plan_span"].append(plan_ms); t["rows_decode_span"].append(dec_ms); t["pad_span"].append(pad_ms)
            # (b) the dense gather, the memset, the scatter
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            t0 = time.perf_counter()
            ev[0].record(s)
            codec.gather_async(idx, d_items, o_off, o_len, n, 1, cap_pieces, dense, d_out_offsets, d_status, d_need[0:1])
            ev[1].record(s)
            rc = hip.hipMemsetAsync(padded.data_ptr(), 0, padded.numel(), hs)
            assert rc == 0, rc
            ev[2].record(s)
            row = torch.searchsorted(d_out_offsets[1:], pos, right=True)
            padded[row * stride + (pos - d_out_offsets[row])] = dense
            ev[3].record(s)
            s.synchronize()
            t1 = time.perf_counter()
            if codec.status() != 0:
                raise SystemExit(f"{name}: old route: device status {codec.status()}")
            plan_ms, _, dec_ms, _ = codec.profile_read_gather()
            if keep:
                t["old_route_wall"].append((t1 - t0) * 1e3); t["old_route_events"].append(ev[0].elapsed_time(ev[3]))
                t["dense_plan_span"].append(plan_ms); t["dense_decode_span"].append(dec_ms)
                for k, (a, b) in zip(("old_gather_events", "old_memset_events", "old_scatter_events"), ((0, 1), (1, 2), (2, 3))):
                    t[k].append(ev[a].elapsed_time(ev[b]))
        codec.profile(False)
        want = np.zeros((n, stride), dtype=np.uint8)
        for k in range(n):
            want[k, :want_len[k]] = data[starts[k]:starts[k] + want_len[k]]
        ok = bool(np.array_equal(rows.cpu().numpy().reshape(n, stride), want) and np.array_equal(padded.cpu().numpy().reshape(n, stride), want)
                  and np.array_equal(d_row_lengths.cpu().numpy(), want_len))
        pad_bytes = n * stride - room
        res = {"case": name, "rows": n, "row_stride": stride, "truncate": truncate, "data_bytes": room, "pad_bytes": pad_bytes, "cap_pieces": cap_pieces,
               "need": d_need.cpu().tolist(), "reps": args.reps, "image_ok": ok}
        res.update(extra)
        for k, v in t.items():
            res[k + "_ms"], res[k + "_min_max_ms"] = stats(v)[0], stats(v)[1:]
        res["old_route_over_rows_events"] = round(res["old_route_events_ms"] / res["rows_events_ms"], 2)
        lo, hi = res["old_route_events_min_max_ms"]
        res["rows_slower_than_old_route_max"] = bool(res["rows_events_ms"] > hi)
        res["pad_write_gbps"] = round(pad_bytes / (res["pad_span_ms"] * 1e-3) / 1e9, 1) if res["pad_span_ms"] > 0 and pad_bytes else None
        best, med = codec.measure_copy(max(pad_bytes, 1 << 20), 9)
        res["copy_probe_bytes"], res["copy_probe_read_plus_write_gbps"], res["copy_probe_write_gbps"] = max(pad_bytes, 1 << 20), round(med, 1), round(med / 2, 1)
        emit(res)

    cases = args.cases.split(",")
    text = {"text_12": 12, "text_16": 16}
    if any(c in text for c in cases):
        n = 64 << 20
        data = tsq.synth.text(n, seed=5)
        src = torch.from_numpy(data).cuda()
        offs = rng.integers(0, n - 100, 2000).astype(np.int64)
        lens = np.full(2000, 100, dtype=np.int64)
        for c in cases:
            if c not in text:
                continue
            bl = 1 << text[c]
            blob, table = codec.compress_split(src, args.ext, bl, block_sizes=True)
            idx = codec.index_sized(blob, n, bl, table)
            pieces = int(((offs + 99) // bl - offs // bl + 1).sum())
            measure(f"text_64MiB_block_2^{text[c]}", idx, None, offs, lens, 128, False, offs, pieces, data, {"block_len": bl, "blocks": idx.n_blocks})
            idx.close()
        del src
    if "pages" in cases or "whole" in cases:
        page, n_pages = 1 << 16, 4096
        data = tsq.synth.text(n_pages * page, seed=7)
        src = torch.from_numpy(data).cuda()
        blobs = codec.compress_batch([src[k * page:(k + 1) * page] for k in range(n_pages)], args.ext)
        idx = codec.index_batch(blobs)
        if "pages" in cases:
            pages = rng.integers(0, n_pages, 2000).astype(np.uint32)
            inside = rng.integers(0, page - 100, 2000).astype(np.int64)
            measure("records_from_pages", idx, pages, inside, np.full(2000, 100, dtype=np.int64), 128, False, pages.astype(np.int64) * page + inside, 2000,
                    data, {"pages": n_pages, "page_bytes": page})
        if "whole" in cases:
            every = np.arange(n_pages, dtype=np.uint32)
            measure("whole_pages_truncated", idx, every, None, None, 4096, True, every.astype(np.int64) * page, n_pages, data,
                    {"pages": n_pages, "page_bytes": page})
        idx.close()
        del src, blobs
    if "big" in cases:
        n, bl, R = 1 << 30, 4096, 200000
        data = tsq.synth.text(n, seed=9)
        src = torch.from_numpy(data).cuda()
        blob, table = codec.compress_split(src, args.ext, bl, block_sizes=True)
        del src
        idx = codec.index_sized(blob, n, bl, table)
        offs = rng.integers(0, n - 100, R).astype(np.int64)
        lens = np.full(R, 100, dtype=np.int64)
        pieces = int(((offs + 99) // bl - offs // bl + 1).sum())
        measure("text_1GiB_block_2^12", idx, None, offs, lens, 128, False, offs, pieces, data, {"block_len": bl, "blocks": idx.n_blocks})
        idx.close()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
