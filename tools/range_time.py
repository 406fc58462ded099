"""Range-read timing on the 10^9 B enwik9-shaped container (239 blocks): device events around each call on one stream, warm-ups
first, the median of --reps calls.  Prints one JSON line:
  whole_range_ms / decompress_ms   one read of every byte against tsqa_decompress_device_async (frame walk + decode)
  head_64k_ms                      the first 64 KiB of a block
  tail_64k_ms                      the last 64 KiB of a block
  full_block_ms                    one whole block
  random_4k_x4096_ms               4 096 random 4 KiB reads in one call
The ranges are planned on the host inside each call (that time is in the numbers: the GPU waits for it)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block", type=int, default=100, help="the block of the single-block reads")
    args = ap.parse_args()
    import numpy as np
    import torch
    import turbosqueeze_amd as tsq

    torch.cuda.set_device(0)
    codec = tsq.DeviceCodec(0)
    n = args.bytes
    blob = codec.compress(torch.from_numpy(tsq.synth.text(n, seed=9)).cuda(), 1).clone()
    torch.cuda.empty_cache()
    idx = codec.index(blob)
    B = tsq.BLOCK_SZ
    blk = min(args.block, idx.n_blocks - 2)
    out = torch.empty(n + 4096 * 4096, dtype=torch.uint8, device="cuda")
    # a stream of its own: the library takes a NULL stream (torch's default) as the context's own, which torch's events do not see
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    rng = np.random.default_rng(1)
    shapes = {
        "whole_range_ms": [(0, n, 0)],
        "head_64k_ms": [(blk * B, 65536, 0)],
        "tail_64k_ms": [((blk + 1) * B - 65536, 65536, 0)],
        "full_block_ms": [(blk * B, B, 0)],
        "random_4k_x4096_ms": [(int(o), 4096, k * 4096) for k, o in enumerate(rng.integers(0, n - 4096, 4096))],
    }

    def timed(enqueue):
        times = []
        for r in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            enqueue()
            e1.record(s)
            e1.synchronize()
            if codec.status() != 0:
                raise SystemExit(f"device status {codec.status()}")
            if r >= args.warmup:
                times.append(e0.elapsed_time(e1))
        return round(statistics.median(times), 4)

    plain = codec.decompress(blob)
    assert plain.numel() == n
    out.fill_(0)
    res = {"bytes": n, "blocks": idx.n_blocks, "block_of_single_reads": blk, "reps": args.reps}
    res["decompress_ms"] = timed(lambda: codec.decompress_async(blob, idx.n_blocks, out))
    res["decompress_correct"] = bool(torch.equal(out[:n], plain))
    for name, triples in shapes.items():
        arr = tsq.api._range_array(triples)

        def call(arr=arr, k=len(triples)):
            rc = codec.L.tsqa_decompress_ranges_async(codec.h, idx.h, arr, k, out.data_ptr(), out.numel(), codec._status.data_ptr(),
                                                      C.c_void_p(s.cuda_stream))
            if rc:
                raise tsq.TsqError(rc, codec.last_error())
        res[name] = timed(call)
    # correctness of what was timed last: the 4 KiB reads against the decompressed container
    s.synchronize()
    got = out[: 4096 * 4096].view(4096, 4096)
    want = torch.stack([plain[o:o + 4096] for o, _, _ in shapes["random_4k_x4096_ms"]])
    res["random_reads_correct"] = bool(torch.equal(got, want))
    res["whole_vs_decompress"] = round(res["whole_range_ms"] / res["decompress_ms"], 4)
    res["full_block_vs_head_64k"] = round(res["full_block_ms"] / res["head_64k_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
