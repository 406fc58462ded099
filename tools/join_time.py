"""Timing of the join of device-resident containers (tsqa_join_async) against a plain device copy of the same bytes and against the
only other route to one container: decompress every item (tsqa_decompress_batch_packed_dense_async), then compress the concatenation
(tsqa_compress_device_async).  Device events on one stream with nothing else on the device, warm-ups first, the median of --reps with the
minimum and the maximum kept.  One JSON line per shape, printed and appended to --out (profiles/join_time.jsonl).  One process per
shape: --shape A, B or C.

  A   64 containers of 16 MiB of text: long bodies, the whole of every piece of the output inside one body
  B   4 096 containers of 64 KiB of text: a seam every 16th piece or so
  C   262 144 containers of one byte: bodies of 9 bytes, every 16-byte word across one or two seams

  join_ms        the whole call: five launches, the block-size table not asked for
  emit_ms        its copy kernel alone (tsqa_profile_read_join: events around that one launch, in runs of their own)
  copy_ms        tsqa_measure_copy's kernel on as many bytes as the joined container has, in the same process: its median rate turned
                 into the time for those bytes; emit_over_copy is the ratio of the two rates
  reencode_ms    the dense decompress of the arena, then compress of the concatenation, both enqueued with no host wait between them
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"A": ("text_64x16MiB", 64, 16 << 20), "B": ("text_4096x64KiB", 4096, 64 << 10), "C": ("text_262144x1B", 262144, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_time.jsonl"), help="the JSON line is appended to this file")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
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
    name, n, length = SHAPES[args.shape]

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

    med = lambda ts: round(statistics.median(ts), 4)
    spread = lambda ts: [round(min(ts), 4), round(max(ts), 4)]

    # the containers: one packed compress; shape C compresses 256 different bytes once and lists that arena 1 024 times over
    made = min(n, 256) if length == 1 else n
    src = torch.from_numpy(tsq.synth.text(made * length, seed=5)).cuda()
    in_at = [k * length for k in range(made)]
    arena = torch.empty(sum(tsq.batch_bound(length) + align for _ in range(made)), dtype=torch.uint8, device="cuda")
    d_offsets = torch.zeros(made + 1, dtype=torch.int64, device="cuda")
    d_sizes = torch.zeros(made, dtype=torch.int64, device="cuda")
    codec.compress_batch_packed_async(src, [(a, length) for a in in_at], ext, align, arena, d_offsets, d_sizes)
    s.synchronize()
    assert codec.status() == 0
    used = int(d_offsets[made].item())
    if made < n:
        reps = n // made
        step = -(-used // align) * align
        arena = torch.cat([arena[:step]] * reps)
        d_offsets = (d_offsets[:made].repeat(reps) + torch.arange(reps, device="cuda", dtype=torch.int64).repeat_interleave(made) * step)
        d_sizes = d_sizes.repeat(reps)
        src = src.repeat(reps)
    else:
        arena, d_offsets = arena[:used].clone(), d_offsets[:n].clone()
    blocks = n * (-(-length // tsq.BLOCK_SZ))
    d_first = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_size = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_word = torch.zeros(1, dtype=torch.int32, device="cuda")

    def join(out):
        rc = L.tsqa_join_async(codec.h, arena.data_ptr(), arena.numel(), d_offsets.data_ptr(), d_sizes.data_ptr(), n, blocks,
                               out.data_ptr() if out is not None else None, out.numel() if out is not None else 0, d_size.data_ptr(),
                               d_first.data_ptr(), None, d_status.data_ptr(), d_word.data_ptr(), hs)
        assert rc == 0, codec.last_error()

    join(None)
    s.synchronize()
    size = int(d_size.item())
    assert int(d_word.item()) == 6 and size > 16 and int(d_first[n].item()) == blocks
    out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    j = timed(lambda: join(out))
    s.synchronize()
    assert int(d_word.item()) == 0 and int(d_size.item()) == size
    ok = bool(torch.equal(codec.decompress(out), src))
    codec.profile(True)
    emit = []
    for r in range(args.warmup + args.reps):
        join(out)
        s.synchronize()
        ms, launches = codec.profile_read_join()
        assert launches == 1
        if r >= args.warmup:
            emit.append(ms)
    codec.profile(False)
    m = timed(lambda: join(None))
    best, median = codec.measure_copy(max(size, 1 << 20), args.reps)
    copy_ms = 2.0 * size / (median * 1e9) * 1e3
    emit_gbps = 2.0 * size / (statistics.median(emit) * 1e-3) / 1e9

    # the other route, at its best: both calls asynchronous on the stream, the block count and the room known on the host
    back = torch.zeros(src.numel(), dtype=torch.uint8, device="cuda")
    again = torch.empty(tsq.container_bound(src.numel()), dtype=torch.uint8, device="cuda")
    tables = codec._dense_tables(n)

    def reencode():
        codec.decompress_batch_packed_dense_async(arena, d_offsets, d_sizes, n, blocks, 1, back, *tables)
        codec.compress_async(back, ext, again)

    reencode()
    s.synchronize()
    again_size, again_status = codec.last_size_status()
    same = again_status == 0 and bool(torch.equal(back, src)) and bool(torch.equal(codec.decompress(again[:again_size]), src))
    r = timed(reencode)
    res = {"shape": name, "items": n, "bytes": src.numel(), "joined_bytes": size, "blocks": blocks, "reps": args.reps,
           "join_ms": med(j), "join_spread_ms": spread(j), "emit_ms": med(emit), "emit_spread_ms": spread(emit),
           "emit_gbps_read_plus_written": round(emit_gbps, 1), "measure_only_ms": med(m), "measure_only_spread_ms": spread(m),
           "copy_probe_gbps_median": round(median, 1), "copy_probe_gbps_best": round(best, 1), "copy_ms": round(copy_ms, 4),
           "copy_probe_shape": codec.copy_probe_shape(), "emit_over_copy_rate": round(emit_gbps / median, 3),
           "reencode_ms": med(r), "reencode_spread_ms": spread(r), "reencode_over_join": round(statistics.median(r) / statistics.median(j), 1),
           "join_decodes_to_the_items": ok, "reencode_decodes_to_the_items": same}
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
