"""Timing of the record tables (tsqa_records_async) against the route there was before them.  Per shape, the median of --reps and
the spread (min .. max), device events on a stream of the tool's own unless said otherwise:
  records_cap    tsqa_records_async with cap_records given: one enqueue, no host read (device events, and the host clock from the
                 call to the end of the stream, which is what the other two routes are held against)
  records_pair   the measuring call, one host read of the count, the filling call (host clock: it waits in the middle)
  old_route      what a user had to do: decompress into a buffer as large as the data, (buf == delim).nonzero(), and the torch
                 arithmetic that makes offsets and lengths by the same rule (host clock too: nonzero() waits for its count)
  mark_span      the mark decode alone (profile kind 9) beside plain_span, the plain decode kernel of the same container in the same
                 run (profile kind 1, from the old route's decompress), whose min .. max is the yardstick
  table_span     the table launches alone (profile kind 10)
  memory         what each route holds in device memory beyond the container: the library's scratch as hipMemGetInfo sees it grow
                 over the first call on a fresh context, and torch's peak over the old route
The routes alternate inside the loop, on a drained device, warm-ups first.  Shapes:
  text_16, text_22   64 MiB of synth text cut every 2^16 and 2^22 bytes
  big                1 GiB of text cut every 2^16
  pages              4 096 pages of 64 KiB through a batch index
Prints one JSON line per shape (and writes them to --out) with the source fingerprint; the tables of both routes are compared."""
import argparse
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ext", type=int, default=1)
    ap.add_argument("--delim", type=int, default=10)
    ap.add_argument("--cases", default="text_16,text_22,pages,big")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    import turbosqueeze_amd as tsq

    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    fingerprint = tsq.source_fingerprint()
    lines = []
    delim = args.delim

    def stats(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    def old_tables(buf, item_len):
        """offsets (flat) and lengths by the rule, from the decoded bytes: torch only"""
        total = buf.numel()
        pos = (buf == delim).nonzero().flatten()
        behind = pos + 1
        behind = behind[(behind % item_len != 0) & (behind < total)]      # a terminator at an item's last byte starts no record
        starts = torch.cat([torch.arange(0, total, item_len, device=buf.device), behind])
        if item_len < total:                                  # (one item: [0] and the places behind the delimiters are in order already)
            starts = starts.sort().values
        nxt = torch.cat([starts[1:], torch.tensor([total], device=buf.device)])
        lengths = nxt - starts - (buf[nxt - 1] == delim).to(torch.int64)
        return starts, lengths

    def measure(name, codec_of, decompress, total, item_len, n_items, extra):
        codec, idx = codec_of()
        free0 = torch.cuda.mem_get_info()[0]
        i64 = lambda k: torch.empty(max(k, 1), dtype=torch.int64, device="cuda")
        first, need, st = i64(n_items + 1), i64(2), torch.empty(1, dtype=torch.int32, device="cuda")
        codec.records_async(idx, delim, tsq.RECORDS_FLAT, 0, None, None, None, first, need, st)
        s.synchronize()
        scratch = free0 - torch.cuda.mem_get_info()[0]
        n, longest = (int(x) for x in need.cpu().tolist())
        offsets, lengths = i64(n), i64(n)
        buf = torch.empty(total, dtype=torch.uint8, device="cuda")
        codec.profile(True)
        codec.profile_read(); codec.profile_read_records()
        keys = ("records_cap_events", "records_cap_wall", "records_pair_wall", "old_route_wall", "old_decompress_events", "mark_span", "plain_span", "table_span")
        t = {k: [] for k in keys}
        old_peak = 0
        for r in range(args.warmup + args.reps):
            keep = r >= args.warmup
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(s)
            codec.records_async(idx, delim, tsq.RECORDS_FLAT, n, None, offsets, lengths, first, need, st)
            e1.record(s)
            s.synchronize()
            t1 = time.perf_counter()
            if int(st.item()) != 0:
                raise SystemExit(f"{name}: records: device status {int(st.item())}")
            mark_ms, _, table_ms, _ = codec.profile_read_records()
            if keep:
                t["records_cap_events"].append(e0.elapsed_time(e1)); t["records_cap_wall"].append((t1 - t0) * 1e3); t["mark_span"].append(mark_ms); t["table_span"].append(table_ms)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            codec.records_async(idx, delim, tsq.RECORDS_FLAT, 0, None, None, None, first, need, st)
            k = int(need[0].item())
            codec.records_async(idx, delim, tsq.RECORDS_FLAT, k, None, offsets, lengths, first, need, st)
            s.synchronize()
            t1 = time.perf_counter()
            codec.profile_read_records()
            if keep:
                t["records_pair_wall"].append((t1 - t0) * 1e3)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            codec.profile_read()
            t0 = time.perf_counter()
            e0.record(s)
            decompress(codec, buf)
            e1.record(s)
            o_starts, o_lengths = old_tables(buf, item_len)
            s.synchronize()
            t1 = time.perf_counter()
            old_peak = max(old_peak, torch.cuda.max_memory_allocated() - base + buf.numel())
            _, _, dec_ms, _ = codec.profile_read()
            if keep:
                t["old_route_wall"].append((t1 - t0) * 1e3); t["old_decompress_events"].append(e0.elapsed_time(e1)); t["plain_span"].append(dec_ms)
        codec.profile(False)
        ok = bool(torch.equal(o_starts, offsets) and torch.equal(o_lengths, lengths))
        del o_starts, o_lengths
        res = {"case": name, "bytes": total, "records": n, "longest": longest, "reps": args.reps, "tables_ok": ok,
               "scratch_bytes": int(scratch), "map_bytes": ((total >> 6) + idx.n_blocks + 1) * 8, "old_route_peak_bytes": int(old_peak),
               "blocks": idx.n_blocks}
        res.update(extra)
        for k, v in t.items():
            res[k + "_ms"], res[k + "_min_max_ms"] = stats(v)[0], stats(v)[1:]
        lo, hi = res["plain_span_min_max_ms"]
        res["mark_inside_plain_spread"] = bool(lo <= res["mark_span_ms"] <= hi)
        # (host clock against host clock: from the call to the end of the stream, for both routes)
        res["records_slower_than_old_route"] = bool(res["records_cap_wall_ms"] > res["old_route_wall_min_max_ms"][1])
        res["source"] = fingerprint
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        idx.close()
        codec.close()

    cases = args.cases.split(",")
    for name, n, bl in (("text_16", 64 << 20, 1 << 16), ("text_22", 64 << 20, 1 << 22), ("big", 1 << 30, 1 << 16)):
        if name not in cases:
            continue
        src = torch.from_numpy(tsq.synth.text(n, seed=5)).cuda()
        maker = tsq.DeviceCodec(0)
        blob, table = maker.compress_split(src, args.ext, bl, block_sizes=True)
        del src

        def codec_of():
            c = tsq.DeviceCodec(0)
            return c, c.index_sized(blob, n, bl, table)
        measure(f"text_{n >> 20}MiB_block_2^{bl.bit_length() - 1}", codec_of,
                lambda c, buf: c.decompress_sized_async(blob, table.numel(), table, buf), n, n, 1, {"block_len": bl})
        maker.close()
        del blob, table
    if "pages" in cases:
        page, n_pages = 1 << 16, 4096
        src = torch.from_numpy(tsq.synth.text(n_pages * page, seed=7)).cuda()
        maker = tsq.DeviceCodec(0)
        blobs = maker.compress_batch([src[k * page:(k + 1) * page] for k in range(n_pages)], args.ext)
        del src

        def codec_of():
            c = tsq.DeviceCodec(0)
            return c, c.index_batch(blobs)
        measure("pages_4096_x_64KiB", codec_of, lambda c, buf: c.decompress_batch(blobs, out=buf), n_pages * page, page, n_pages,
                {"pages": n_pages, "page_bytes": page})
        maker.close()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
