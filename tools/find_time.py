"""Timing of the find (tsqa_find_async) against the route there was before it.  Per shape and needle, the median of --reps and the
spread (min .. max), device events on a stream of the tool's own unless said otherwise:
  find_cap       tsqa_find_async with cap_hits given: one enqueue, no host read (device events, and the host clock from the call to
                 the end of the stream, which is what the other two routes are held against)
  find_pair      the measuring call, one host read of the count, the filling call (host clock: it waits in the middle)
  old_route      what a user had to do: decompress into a buffer as large as the data, one shifted torch comparison per needle byte
                 ANDed together, nonzero(), and the hits that run across an item's end masked out (host clock too: nonzero() waits
                 for its count)
  find_span      the find decode alone (profile kind 11) beside mark_span, the records' mark decode (kind 9, a measuring records
                 call), and plain_span, the plain decode kernel (kind 1, from the old route's decompress), all of the same container
                 in the same run; the plain decode's min .. max is the yardstick
  table_span     the seam launch and the table launches alone (profile kind 12)
  memory         what each route holds in device memory beyond the container: the library's scratch as hipMemGetInfo sees it grow
                 over the first call on a fresh context, and torch's peak over the old route
The routes alternate inside the loop, on a drained device, warm-ups first.  Shapes:
  text_16, text_22   64 MiB of synth text cut every 2^16 and 2^22 bytes
  big                1 GiB of text cut every 2^16
  pages              4 096 pages of 64 KiB through a batch index
Needles: 1, 4 and 16 bytes, of each length one that occurs (a space; ' ef ', frequent in the synthetic text; 16 bytes taken from
the middle of the data) and one that never does (bytes of 0xFF).  Prints one JSON line per shape and needle (and writes them to --out) with the source fingerprint;
the tables of both routes are compared."""
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
    ap.add_argument("--cases", default="text_16,text_22,pages,big")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    import torch
    import turbosqueeze_amd as tsq

    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    fingerprint = tsq.source_fingerprint()
    lines = []

    def stats(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    def old_hits(buf, needle, item_len):
        """the hits' flat offsets by the rule, from the decoded bytes: torch only"""
        total, m = buf.numel(), len(needle)
        span = total - m + 1
        mask = buf[:span] == needle[0]
        for k in range(1, m):
            mask &= buf[k:span + k] == needle[k]
        pos = mask.nonzero().flatten()
        if item_len < total:                                 # no hit runs from one item into the next
            pos = pos[(pos % item_len) + m <= item_len]
        return pos

    def measure(name, codec_of, decompress, total, item_len, n_items, needles, extra):
        for what, needle in needles:
            codec, idx = codec_of()
            free0 = torch.cuda.mem_get_info()[0]
            i64 = lambda k: torch.empty(max(k, 1), dtype=torch.int64, device="cuda")
            first, need, need2, st = i64(n_items + 1), i64(1), i64(2), torch.empty(1, dtype=torch.int32, device="cuda")
            codec.find_async(idx, needle, tsq.FIND_FLAT, 0, None, None, first, need, st)
            s.synchronize()
            scratch = free0 - torch.cuda.mem_get_info()[0]
            n = int(need[0].item())
            offsets = i64(n)
            buf = torch.empty(total, dtype=torch.uint8, device="cuda")
            codec.profile(True)
            codec.profile_read(); codec.profile_read_records(); codec.profile_read_find()
            keys = ("find_cap_events", "find_cap_wall", "find_pair_wall", "old_route_wall", "old_decompress_events", "find_span", "mark_span",
                    "plain_span", "table_span")
            t = {k: [] for k in keys}
            old_peak = 0
            for r in range(args.warmup + args.reps):
                keep = r >= args.warmup
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(s)
                codec.find_async(idx, needle, tsq.FIND_FLAT, n, None, offsets if n else None, first, need, st)
                e1.record(s)
                s.synchronize()
                t1 = time.perf_counter()
                if int(st.item()) != 0:
                    raise SystemExit(f"{name}: find: device status {int(st.item())}")
                find_ms, _, table_ms, _ = codec.profile_read_find()
                if keep:
                    t["find_cap_events"].append(e0.elapsed_time(e1)); t["find_cap_wall"].append((t1 - t0) * 1e3); t["find_span"].append(find_ms); t["table_span"].append(table_ms)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                codec.find_async(idx, needle, tsq.FIND_FLAT, 0, None, None, first, need, st)
                k = int(need[0].item())
                codec.find_async(idx, needle, tsq.FIND_FLAT, k, None, offsets if k else None, first, need, st)
                s.synchronize()
                t1 = time.perf_counter()
                codec.profile_read_find()
                if keep:
                    t["find_pair_wall"].append((t1 - t0) * 1e3)
                # the records' mark decode of the same container, for the span alone
                codec.records_async(idx, 10, tsq.RECORDS_FLAT, 0, None, None, None, first, need2, st)
                s.synchronize()
                mark_ms, _, _, _ = codec.profile_read_records()
                if keep:
                    t["mark_span"].append(mark_ms)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                codec.profile_read()
                t0 = time.perf_counter()
                e0.record(s)
                decompress(codec, buf)
                e1.record(s)
                o_hits = old_hits(buf, needle, item_len)
                s.synchronize()
                t1 = time.perf_counter()
                old_peak = max(old_peak, torch.cuda.max_memory_allocated() - base + buf.numel())
                _, _, dec_ms, _ = codec.profile_read()
                if keep:
                    t["old_route_wall"].append((t1 - t0) * 1e3); t["old_decompress_events"].append(e0.elapsed_time(e1)); t["plain_span"].append(dec_ms)
            codec.profile(False)
            ok = bool(o_hits.numel() == n and torch.equal(o_hits, offsets[:n]))
            del o_hits
            res = {"case": name, "needle": what, "needle_bytes": len(needle), "bytes": total, "hits": n, "reps": args.reps, "tables_ok": ok,
                   "scratch_bytes": int(scratch), "map_bytes": ((total >> 6) + idx.n_blocks + 1) * 8, "edge_bytes": 32 * idx.n_blocks,
                   "old_route_peak_bytes": int(old_peak), "blocks": idx.n_blocks}
            res.update(extra)
            for k, v in t.items():
                res[k + "_ms"], res[k + "_min_max_ms"] = stats(v)[0], stats(v)[1:]
            lo, hi = res["plain_span_min_max_ms"]
            res["find_inside_plain_spread"] = bool(lo <= res["find_span_ms"] <= hi)
            # (host clock against host clock: from the call to the end of the stream, for both routes)
            res["find_beats_old_route"] = bool(res["find_cap_wall_ms"] < res["old_route_wall_min_max_ms"][0])
            res["source"] = fingerprint
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
            idx.close()
            codec.close()
            del buf, offsets

    def needles_of(host):
        mid = host.size // 2
        return (("1_often", b" "), ("1_never", b"\xff"), ("4_often", b" ef "), ("4_never", b"\xff" * 4), ("16_present", host[mid:mid + 16].tobytes()),
                ("16_never", b"\xff" * 16))

    cases = args.cases.split(",")
    for name, n, bl in (("text_16", 64 << 20, 1 << 16), ("text_22", 64 << 20, 1 << 22), ("big", 1 << 30, 1 << 16)):
        if name not in cases:
            continue
        host = tsq.synth.text(n, seed=5)
        needles = needles_of(host)
        src = torch.from_numpy(host).cuda()
        del host
        maker = tsq.DeviceCodec(0)
        blob, table = maker.compress_split(src, args.ext, bl, block_sizes=True)
        del src

        def codec_of():
            c = tsq.DeviceCodec(0)
            return c, c.index_sized(blob, n, bl, table)
        measure(f"text_{n >> 20}MiB_block_2^{bl.bit_length() - 1}", codec_of,
                lambda c, buf: c.decompress_sized_async(blob, table.numel(), table, buf), n, n, 1, needles, {"block_len": bl})
        maker.close()
        del blob, table
    if "pages" in cases:
        page, n_pages = 1 << 16, 4096
        host = tsq.synth.text(n_pages * page, seed=7)
        needles = needles_of(host)
        src = torch.from_numpy(host).cuda()
        del host
        maker = tsq.DeviceCodec(0)
        blobs = maker.compress_batch([src[k * page:(k + 1) * page] for k in range(n_pages)], args.ext)
        del src

        def codec_of():
            c = tsq.DeviceCodec(0)
            return c, c.index_batch(blobs)
        measure("pages_4096_x_64KiB", codec_of, lambda c, buf: c.decompress_batch(blobs, out=buf), n_pages * page, page, n_pages, needles,
                {"pages": n_pages, "page_bytes": page})
        maker.close()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
