"""Timing of the short-block entry points against the plain ones on the same input: tsqa_compress_device_split_async against
tsqa_compress_device_async, and three decompresses -- tsqa_decompress_device_async on the 4 MiB container, the same call on the
split container, and tsqa_decompress_device_sized_async on it -- with the two frame walks (frame_walk_kernel,
frame_walk_sized_kernel) timed alone.  synth text, extensions on, device events on one stream, warm-ups first, then --reps rounds in
which the calls under comparison take turns; the median of the reps with their minimum and maximum beside every figure.  One JSON
line per (size, block_len), printed and appended to --out (profiles/split_time.jsonl).

A frame walk alone: the library's own timing spans (tsqa_profile_enable) put device events around the whole decompress call and around
its decode launches; the walk is the first minus the second, both read after every single call.  That figure holds the walk
kernel and the gap between it and the first decode launch, at the resolution of device events: it is not a kernel time from a trace.

The two verdict fields say whether a median beats the other call's by more than that call's own spread (max - min of its reps):
split_beats_plain (compress) and sized_walk_beats_serial (the walks alone)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="16,64,256,1024", help="input sizes in MiB")
    ap.add_argument("--block-lens", default="16,18,20,22", help="log2 of the block lengths")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_time.jsonl"), help="the JSON lines are appended to this file")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
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
    d_size, d_status = codec._size.data_ptr(), codec._status.data_ptr()

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

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

    def walks_in_turns(calls):
        """as in_turns, for decompress calls: -> per call the times of its frame walk alone (the call's span minus its decode span)"""
        codec.profile(True)
        codec.profile_read(), codec.profile_read_calls()
        times = [[] for _ in calls]
        for r in range(args.warmup + args.reps):
            for k, call in enumerate(calls):
                call()
                s.synchronize()
                _, _, dec_ms, dec_n = codec.profile_read()
                _, _, call_ms, call_n = codec.profile_read_calls()
                assert dec_n >= 1 and call_n == 1 and codec.status() == 0
                if r >= args.warmup:
                    times[k].append(call_ms - dec_ms)
        codec.profile(False)
        return times

    med = lambda ts: round(statistics.median(ts), 4)
    spread = lambda ts: [round(min(ts), 4), round(max(ts), 4)]
    beats = lambda new, old: bool(statistics.median(old) - statistics.median(new) > max(old) - min(old))

    for size_mib in [int(x) for x in args.sizes.split(",")]:
        n = size_mib * MiB
        src = torch.from_numpy(tsq.synth.text(n, seed=5)).cuda()
        back = torch.empty(n, dtype=torch.uint8, device="cuda")
        plain = torch.empty(tsq.container_bound(n), dtype=torch.uint8, device="cuda")
        nb_plain = -(-n // tsq.BLOCK_SZ)

        def compress_plain():
            rc = L.tsqa_compress_device_async(codec.h, src.data_ptr(), n, plain.data_ptr(), plain.numel(), d_size, d_status, ext, hs)
            assert rc == 0, codec.last_error()

        compress_plain()
        s.synchronize()
        plain_size, st = codec.last_size_status()
        assert st == 0

        def decompress_plain():
            rc = L.tsqa_decompress_device_async(codec.h, plain.data_ptr(), plain_size, nb_plain, back.data_ptr(), n, d_size, d_status, hs)
            assert rc == 0, codec.last_error()

        for log2 in [int(x) for x in args.block_lens.split(",")]:
            block_len = 1 << log2
            nb, bound = tsq.plan_split(n, block_len)
            split = torch.empty(bound, dtype=torch.uint8, device="cuda")
            table = torch.empty(nb, dtype=torch.int32, device="cuda")

            def compress_split():
                rc = L.tsqa_compress_device_split_async(codec.h, src.data_ptr(), n, block_len, split.data_ptr(), bound, d_size, table.data_ptr(),
                                                        d_status, ext, hs)
                assert rc == 0, codec.last_error()

            compress_split()
            s.synchronize()
            split_size, st = codec.last_size_status()
            assert st == 0

            def decompress_split():
                rc = L.tsqa_decompress_device_async(codec.h, split.data_ptr(), split_size, nb, back.data_ptr(), n, d_size, d_status, hs)
                assert rc == 0, codec.last_error()

            def decompress_sized():
                rc = L.tsqa_decompress_device_sized_async(codec.h, split.data_ptr(), split_size, nb, table.data_ptr(), back.data_ptr(), n, d_size,
                                                          d_status, hs)
                assert rc == 0, codec.last_error()

            cp, cs = in_turns([compress_plain, compress_split])
            back.zero_()
            dp, ds, dz = in_turns([decompress_plain, decompress_split, decompress_sized])
            s.synchronize()
            ok = bool(torch.equal(back, src))                # (the last call of the last round was the sized one)
            ws, wz = walks_in_turns([decompress_split, decompress_sized])
            gbps = lambda ts: round(n / statistics.median(ts) / 1e6, 2)
            emit({"input": "synth_text", "mib": size_mib, "bytes": n, "ext": ext, "block_len": block_len, "blocks": nb, "blocks_4mib": nb_plain,
                  "reps": args.reps, "warmup": args.warmup,
                  "container_bytes": split_size, "container_bytes_4mib": plain_size, "container_over_4mib": round(split_size / plain_size, 4),
                  "compress_plain_ms": med(cp), "compress_plain_spread_ms": spread(cp), "compress_plain_gbps": gbps(cp),
                  "compress_split_ms": med(cs), "compress_split_spread_ms": spread(cs), "compress_split_gbps": gbps(cs),
                  "split_over_plain": round(statistics.median(cs) / statistics.median(cp), 4), "split_beats_plain": beats(cs, cp),
                  "decompress_plain_4mib_ms": med(dp), "decompress_plain_4mib_spread_ms": spread(dp),
                  "decompress_plain_on_split_ms": med(ds), "decompress_plain_on_split_spread_ms": spread(ds),
                  "decompress_sized_on_split_ms": med(dz), "decompress_sized_on_split_spread_ms": spread(dz), "decompress_sized_gbps": gbps(dz),
                  "walk_serial_ms": med(ws), "walk_serial_spread_ms": spread(ws), "walk_sized_ms": med(wz), "walk_sized_spread_ms": spread(wz),
                  "sized_walk_beats_serial": beats(wz, ws), "round_trip_ok": ok})
            del split, table
        del src, back, plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
