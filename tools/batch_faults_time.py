"""Timing of the batch decompress with a verdict per item (tsqa_decompress_batch_items_async) and of the synchronous
tsqa_decompress_batch on a batch that holds damaged items.  Text, extensions on, device events on one stream, warm-ups first, the
median of --reps.  One JSON line per measurement, printed and appended to --out (profiles/batch_faults.jsonl).

  healthy (the default)  text_4096x64KiB and text_1024x1MiB, every item healthy, alternating in one session: the existing
                         tsqa_decompress_batch_async at decode variant 4 (one workgroup per block: the same decoder body), the form
                         with a verdict per item, the existing form at variant 0, then variant 4 once more.  The variant-4 reps of
                         both runs give the existing form's own spread about its median; the line says whether the per-item form's
                         median lies inside it.
  --sync-only            text_4096x64KiB with 1 and with 64 of the items damaged, through the synchronous tsqa_decompress_batch
                         alone: this mode uses no entry point that the per-item form added, so the same tool times a checkout from
                         before it (--tree DIR imports turbosqueeze_amd from that checkout; --label names it in the lines).  An item
                         is damaged by raising its first frame word's stream length by one: the frame then runs past its container,
                         which the frame walk refuses on the device (TSQA_ERR_FORMAT) without a decoder reading it.
  --ratios               no GPU: for every --sync-only measurement that --out holds from two checkouts, one more line with both
                         numbers and their ratio.
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
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sync-only", action="store_true", help="the synchronous call on a batch with damaged items, the existing API only")
    ap.add_argument("--ratios", action="store_true", help="append the ratios of the --sync-only lines of two checkouts in --out (no GPU)")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import turbosqueeze_amd from (built there)")
    ap.add_argument("--label", default="branch", help="which checkout the lines belong to")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_faults.jsonl"), help="the JSON lines are appended to this file")
    args = ap.parse_args()
    if args.ratios:
        rows = [json.loads(line) for line in open(args.out) if line.strip()]
        sync = {(r["checkout"], r["damaged"]): r for r in rows if r["measurement"] == "sync_with_damaged_items"}
        with open(args.out, "a") as f:
            for (who, damaged), r in sorted(sync.items()):
                base = sync.get(("parent", damaged))
                if who == "parent" or base is None:
                    continue
                line = json.dumps({"measurement": "sync_with_damaged_items_ratio", "shape": r["shape"], "items": r["items"], "damaged": damaged,
                                   "parent_ms": base["decompress_batch_ms"], f"{who}_ms": r["decompress_batch_ms"],
                                   f"parent_over_{who}": round(base["decompress_batch_ms"] / r["decompress_batch_ms"], 1)})
                print(line)
                f.write(line + "\n")
        return
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
    ext = 1

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    def timed(call, keep=None):
        times = []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            call()
            e1.record(s)
            e1.synchronize()
            if r >= args.warmup:
                times.append(e0.elapsed_time(e1))
        if keep is not None:
            keep.extend(times)
        return round(statistics.median(times), 3)

    def compressed(lengths):
        """the items' containers, made by one tsqa_compress_batch_async -> (src, containers' buffer, decompress items, block counts)"""
        total = sum(lengths)
        src = torch.from_numpy(tsq.synth.text(total, seed=5)).cuda()
        offs = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
        caps = [tsq.batch_bound(n) for n in lengths]
        out_at = np.concatenate([[0], np.cumsum(caps)[:-1]]).tolist()
        out = torch.zeros(sum(caps), dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros(len(lengths), dtype=torch.int64, device="cuda")
        codec.compress_batch_async(src, [(o, n, a, c) for o, n, a, c in zip(offs, lengths, out_at, caps)], ext, out, d_sizes)
        s.synchronize()
        assert codec.status() == 0
        sizes = d_sizes.cpu().tolist()
        ditems = [(a, z, o, n) for a, z, o, n in zip(out_at, sizes, offs, lengths)]
        return src, out, ditems, np.array([-(-n // tsq.BLOCK_SZ) for n in lengths], dtype=np.uint32)

    if args.sync_only:
        lengths = [1 << 16] * 4096
        src, out, ditems, _ = compressed(lengths)
        n = len(ditems)
        back = torch.zeros(sum(lengths), dtype=torch.uint8, device="cuda")
        darr = tsq.api._batch_array(ditems)
        sizes, status = (C.c_uint64 * n)(), (C.c_int32 * n)()
        clean = out.clone()
        for damaged in (1, 64):
            out.copy_(clean)
            hit = [int(k) for k in np.linspace(n // 8, n - n // 8, damaged).astype(int)] if damaged > 1 else [n // 2]
            for k in hit:
                at = ditems[k][0] + 16
                word = int.from_bytes(bytes(out[at:at + 3].cpu().numpy()), "little") + 1
                out[at:at + 3] = torch.tensor(list(word.to_bytes(3, "little")), dtype=torch.uint8, device="cuda")
            s.synchronize()
            rcs = []

            def call():
                rcs.append(L.tsqa_decompress_batch(codec.h, out.data_ptr(), out.numel(), darr, n, back.data_ptr(), back.numel(), sizes, status, hs))

            back.zero_()
            ms = timed(call)
            refused = [k for k in range(n) if status[k] != 0]
            ok = all(bool(torch.equal(back[o:o + ln], src[o:o + ln])) for k, (_, _, o, ln) in enumerate(ditems) if k not in hit and k % 97 == 0)
            emit({"measurement": "sync_with_damaged_items", "checkout": args.label, "shape": "text_4096x64KiB", "items": n, "damaged": damaged,
                  "reps": args.reps, "decompress_batch_ms": ms, "return_values": sorted(set(rcs)), "refused_items_are_the_damaged": refused == sorted(hit),
                  "sampled_healthy_items_exact": ok})
        return

    for name, lengths in (("text_4096x64KiB", [1 << 16] * 4096), ("text_1024x1MiB", [1 << 20] * 1024)):
        src, out, ditems, nbs = compressed(lengths)
        n = len(ditems)
        back = torch.zeros(sum(lengths), dtype=torch.uint8, device="cuda")
        darr = tsq.api._batch_array(ditems)
        d_sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
        d_item_status = torch.zeros(n, dtype=torch.int32, device="cuda")
        st = codec._status.data_ptr()

        def existing():
            rc = L.tsqa_decompress_batch_async(codec.h, out.data_ptr(), out.numel(), darr, nbs.ctypes.data, n, back.data_ptr(), back.numel(),
                                               d_sizes.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        def per_item():
            rc = L.tsqa_decompress_batch_items_async(codec.h, out.data_ptr(), out.numel(), darr, nbs.ctypes.data, n, back.data_ptr(), back.numel(),
                                                     d_sizes.data_ptr(), d_item_status.data_ptr(), st, hs)
            assert rc == 0, codec.last_error()

        res = {"measurement": "healthy_batch", "checkout": args.label, "shape": name, "items": n, "bytes": sum(lengths),
               "blocks": int(nbs.sum()), "reps": args.reps}
        before, after = [], []
        codec.set_variant(0, 4)
        res["existing_v4_ms"] = timed(existing, before)
        back.zero_()
        res["per_item_ms"] = timed(per_item)
        s.synchronize()
        res["per_item_round_trip_ok"] = bool(torch.equal(back, src)) and not bool(d_item_status.any()) and codec.status() == 0
        codec.set_variant(0, 0)
        res["existing_v0_ms"] = timed(existing)
        codec.set_variant(0, 4)
        res["existing_v4_again_ms"] = timed(existing, after)
        codec.set_variant(0, 0)
        pooled = statistics.median(before + after)
        res["existing_v4_spread_ms"] = [round(min(before + after), 3), round(max(before + after), 3)]
        res["existing_v4_spread_over_median"] = [round(min(before + after) / pooled, 3), round(max(before + after) / pooled, 3)]
        res["per_item_over_existing_v4"] = round(res["per_item_ms"] / pooled, 3)
        res["per_item_inside_existing_v4_spread"] = min(before + after) <= res["per_item_ms"] <= max(before + after)
        res["per_item_over_existing_v0"] = round(res["per_item_ms"] / res["existing_v0_ms"], 3)
        emit(res)
        del src, out, back
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
