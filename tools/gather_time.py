"""Gather timing (tsqa_gather_async): record reads whose ranges start in DEVICE memory, against the path there was before it.
Per shape, with the offsets and lengths (and items) in device tensors, the median of --reps and the spread (min .. max) of
  gather        tsqa_gather_async alone: host clock from the call to the end of the stream, and device events around it
  host_plan     the same ranges through the host planner: both tables copied to the host and waited for, the tsqa_item_range array
                made with numpy, tsqa_decompress_item_ranges_async, the stream waited for: host clock
  spans         the profile kinds: the gather's planner (its launches in front of the decode) and the decode kernel of either way
Each line also says how many blocks the ranges touch (`groups`: the decode's live workgroups, and all the host plan launches), how
many workgroups the gather's decode launches (min(cap_pieces, blocks)) and how many of those are dead.
The two ways alternate inside the loop, on a drained device, warm-ups first.  Shapes:
  text_2^12, text_2^16, text_2^22   2 000 records of 100 B out of 64 MiB of text cut every 2^12, 2^16, 2^22 bytes (a sized index)
  pages                             2 000 records of 100 B out of 4 096 pages of 64 KiB (a batch index, addressed by item)
  big                               200 000 records of 100 B out of 1 GiB cut every 2^12, cap_pieces exact and generous (4 x)
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ext", type=int, default=1)
    ap.add_argument("--cases", default="text_12,text_16,text_22,pages,big")
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
    item_range = np.dtype([("item", "<u4"), ("pad", "<u4"), ("offset", "<u8"), ("length", "<u8"), ("out_at", "<u8")])
    rng = np.random.default_rng(3)

    def emit(res):
        res["source"] = fingerprint
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)

    def stats(v):
        return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]

    def measure(name, idx, items, offsets, lengths, data_of, cap_pieces, extra):
        """items: None or a uint32 array; offsets, lengths: int64 arrays; data_of(k) -> the bytes range k owes"""
        n = len(offsets)
        d_items = None if items is None else torch.from_numpy(items.view(np.int32)).cuda()
        d_off, d_len = torch.from_numpy(offsets).cuda(), torch.from_numpy(lengths).cuda()
        room = int(lengths.sum())
        out_a, out_b = (torch.zeros(room, dtype=torch.uint8, device="cuda") for _ in range(2))
        d_out_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_range_status = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_need = torch.zeros(1, dtype=torch.int64, device="cuda")
        codec.profile(True)
        codec.profile_read_gather()
        t = {k: [] for k in ("gather_wall", "gather_events", "host_plan_wall", "plan_span", "gather_decode_span", "host_plan_decode_span")}
        for r in range(args.warmup + args.reps):
            keep = r >= args.warmup
            # (a) the gather
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(s)
            codec.gather_async(idx, d_items, d_off, d_len, n, 1, cap_pieces, out_a, d_out_offsets, d_range_status, d_need)
            e1.record(s)
            s.synchronize()
            t1 = time.perf_counter()
            if codec.status() != 0:
                raise SystemExit(f"{name}: gather: device status {codec.status()}")
            plan_ms, _, dec_ms, _ = codec.profile_read_gather()
            if keep:
                t["gather_wall"].append((t1 - t0) * 1e3); t["gather_events"].append(e0.elapsed_time(e1))
                t["plan_span"].append(plan_ms); t["gather_decode_span"].append(dec_ms)
            # (b) the tables to the host, the host planner, the record read
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_off, h_len = d_off.cpu().numpy(), d_len.cpu().numpy()
            rr = np.zeros(n, dtype=item_range)
            if d_items is not None:
                rr["item"] = d_items.cpu().numpy().view(np.uint32)
            rr["offset"], rr["length"] = h_off, h_len
            rr["out_at"][1:] = np.cumsum(h_len[:-1])
            rc = L.tsqa_decompress_item_ranges_async(codec.h, idx.h, rr.ctypes.data, n, out_b.data_ptr(), out_b.numel(), st, hs)
            assert rc == 0, codec.last_error()
            s.synchronize()
            t1 = time.perf_counter()
            if codec.status() != 0:
                raise SystemExit(f"{name}: host plan: device status {codec.status()}")
            _, _, dec_ms, _ = codec.profile_read_gather()
            if keep:
                t["host_plan_wall"].append((t1 - t0) * 1e3); t["host_plan_decode_span"].append(dec_ms)
        codec.profile(False)
        want = np.concatenate([data_of(k) for k in range(n)])
        ok = bool(np.array_equal(out_a.cpu().numpy(), want) and np.array_equal(out_b.cpu().numpy(), want))
        launched = min(cap_pieces, idx.n_blocks)
        res = {"case": name, "records": n, "record_bytes": int(lengths[0]), "cap_pieces": cap_pieces, "need_pieces": int(d_need.item()),
               "groups": extra.pop("groups"), "gather_decode_workgroups": launched, "reps": args.reps, "bytes_ok": ok}
        res["gather_dead_workgroups"] = launched - res["groups"]
        res.update(extra)
        for k, v in t.items():
            res[k + "_ms"], res[k + "_min_max_ms"] = stats(v)[0], stats(v)[1:]
        res["host_plan_over_gather"] = round(res["host_plan_wall_ms"] / res["gather_wall_ms"], 2)
        lo, hi = res["host_plan_decode_span_min_max_ms"]
        res["gather_decode_inside_host_plan_min_max"] = bool(lo <= res["gather_decode_span_ms"] <= hi)
        emit(res)

    cases = args.cases.split(",")
    text = {"text_12": 12, "text_16": 16, "text_22": 22}
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
            measure(f"text_64MiB_block_2^{text[c]}", idx, None, offs, lens, lambda k: data[offs[k]:offs[k] + 100], pieces,
                    {"block_len": bl, "blocks": idx.n_blocks, "groups": int(np.unique(np.concatenate([offs // bl, (offs + 99) // bl])).size)})
            idx.close()
        del src
    if "pages" in cases:
        page, n_pages = 1 << 16, 4096
        data = tsq.synth.text(n_pages * page, seed=7)
        src = torch.from_numpy(data).cuda()
        blobs = codec.compress_batch([src[k * page:(k + 1) * page] for k in range(n_pages)], args.ext)
        idx = codec.index_batch(blobs)
        pages = rng.integers(0, n_pages, 2000).astype(np.uint32)
        inside = rng.integers(0, page - 100, 2000).astype(np.int64)
        measure("records_from_pages", idx, pages, inside, np.full(2000, 100, dtype=np.int64),
                lambda k: data[int(pages[k]) * page + inside[k]:int(pages[k]) * page + inside[k] + 100], 2000,
                {"pages": n_pages, "page_bytes": page, "pages_touched": len(set(pages.tolist())), "groups": len(set(pages.tolist()))})
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
        for what, cap in (("exact", pieces), ("generous", 4 * pieces)):
            measure(f"text_1GiB_block_2^12_cap_{what}", idx, None, offs, lens, lambda k: data[offs[k]:offs[k] + 100], cap,
                    {"block_len": bl, "blocks": idx.n_blocks, "groups": int(np.unique(np.concatenate([offs // bl, (offs + 99) // bl])).size)})
        idx.close()

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
