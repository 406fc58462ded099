"""Timing of the CRC (tsqa_crc32_async) against the route there was before it.  Per shape, the median of --reps and the spread
(min .. max), device events on a stream of the tool's own unless said otherwise:
  crc            tsqa_crc32_async with d_all_crc and no d_block_crc: one enqueue, no host read (device events, and the host clock
                 from the call to the value in hand -- one read of the item words at the end --, which is what the old route is
                 held against)
  old_route      what a user had to do: decompress into a buffer as large as the data, copy it to the host, zlib.crc32 there (host
                 clock from the call to the value in hand)
  crc_span       the CRC decode alone (profile kind 13) beside mark_span, the records' mark decode (kind 9, a measuring records
                 call), and plain_span, the plain decode kernel (kind 1, from the old route's decompress), all of the same container
                 in the same run; the plain decode's min .. max is the yardstick
  fold_span      the fold and close launches alone (profile kind 14)
  memory         what each route holds in device memory beyond the container: the library's scratch as hipMemGetInfo sees it grow
                 over the first call on a fresh context (4 bytes per block), and the decoded buffer of the old route
The routes alternate inside the loop, on a drained device, warm-ups first.  Shapes:
  text_16, text_22   64 MiB of synth text cut every 2^16 and 2^22 bytes
  big                1 GiB of text cut every 2^16
  pages              4 096 pages of 64 KiB through a batch index
Prints one JSON line per shape (and writes them to --out) with the source fingerprint; the CRCs of both routes are compared."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

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

    def measure(name, codec_of, decompress, total, item_len, n_items, extra):
        codec, idx = codec_of()
        free0 = torch.cuda.mem_get_info()[0]
        table = codec.crc32_async(idx)
        s.synchronize()
        scratch = free0 - torch.cuda.mem_get_info()[0]
        i64 = lambda k: torch.empty(max(k, 1), dtype=torch.int64, device="cuda")
        first, need2, st = i64(n_items + 1), i64(2), torch.empty(1, dtype=torch.int32, device="cuda")
        buf = torch.empty(total, dtype=torch.uint8, device="cuda")
        host = torch.empty(total, dtype=torch.uint8, pin_memory=True)
        codec.profile(True)
        codec.profile_read(); codec.profile_read_records(); codec.profile_read_crc()
        keys = ("crc_events", "crc_wall", "old_route_wall", "old_decompress_events", "old_copy_wall", "old_zlib_wall", "crc_span", "mark_span", "plain_span",
                "fold_span")
        t = {k: [] for k in keys}
        new_crcs = old_crcs = None
        for r in range(args.warmup + args.reps):
            keep = r >= args.warmup
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(s)
            table = codec.crc32_async(idx, d_items=table.d_items, d_item_status=table.status, d_all=table.d_all, d_status=table.d_status)
            e1.record(s)
            new_crcs = table.d_items.cpu()
            t1 = time.perf_counter()
            if int(table.d_status.item()) != 0:
                raise SystemExit(f"{name}: crc32: device status {int(table.d_status.item())}")
            crc_ms, _, fold_ms, _ = codec.profile_read_crc()
            if keep:
                t["crc_events"].append(e0.elapsed_time(e1)); t["crc_wall"].append((t1 - t0) * 1e3); t["crc_span"].append(crc_ms); t["fold_span"].append(fold_ms)
            # the records' mark decode of the same container, for the span alone
            codec.records_async(idx, 10, tsq.RECORDS_FLAT, 0, None, None, None, first, need2, st)
            s.synchronize()
            mark_ms, _, _, _ = codec.profile_read_records()
            if keep:
                t["mark_span"].append(mark_ms)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            codec.profile_read()
            t0 = time.perf_counter()
            e0.record(s)
            decompress(codec, buf)
            e1.record(s)
            host.copy_(buf, non_blocking=True)
            s.synchronize()
            t1 = time.perf_counter()
            view = memoryview(host.numpy())
            old_crcs = [zlib.crc32(view[k * item_len:(k + 1) * item_len]) for k in range(n_items)]
            t2 = time.perf_counter()
            _, _, dec_ms, _ = codec.profile_read()
            if keep:
                t["old_route_wall"].append((t2 - t0) * 1e3); t["old_decompress_events"].append(e0.elapsed_time(e1)); t["plain_span"].append(dec_ms)
                t["old_copy_wall"].append((t1 - t0) * 1e3 - e0.elapsed_time(e1)); t["old_zlib_wall"].append((t2 - t1) * 1e3)
        codec.profile(False)
        ok = bool([int(v) & 0xFFFFFFFF for v in new_crcs.tolist()] == old_crcs)
        res = {"case": name, "bytes": total, "items": n_items, "blocks": idx.n_blocks, "reps": args.reps, "crcs_ok": ok, "scratch_bytes": int(scratch),
               "block_words_bytes": 4 * (idx.n_blocks + 1), "old_route_device_bytes": total, "old_route_host_bytes": total}
        res.update(extra)
        for k, v in t.items():
            res[k + "_ms"], res[k + "_min_max_ms"] = stats(v)[0], stats(v)[1:]
        lo, hi = res["plain_span_min_max_ms"]
        res["crc_over_plain"] = round(res["crc_span_ms"] / res["plain_span_ms"], 4)
        res["crc_over_mark"] = round(res["crc_span_ms"] / res["mark_span_ms"], 4)
        res["crc_inside_plain_spread"] = bool(lo <= res["crc_span_ms"] <= hi)
        res["crc_beats_old_route"] = bool(res["crc_wall_ms"] < res["old_route_wall_min_max_ms"][0])
        res["source"] = fingerprint
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        idx.close()
        codec.close()
        del buf, host

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
