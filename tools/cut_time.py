"""Timing of the cut of block ranges out of an indexed container (tsqa_cut_async) against a plain device copy of the same bytes,
against the join of the same containers back into one (join_emit_kernel: the same copy with other seams) and against the only other
route to the same containers: a range read of every range (tsqa_decompress_ranges_async), then a packed compress of the pieces
(tsqa_compress_batch_packed_async) -- whose bytes differ at block edges, since a piece compressed again does not see the 128 bytes
behind it.  Device events on one stream with nothing else on the device, warm-ups first, the median of --reps with the minimum and
the maximum kept.  One JSON line per shape, printed and appended to --out (profiles/cut_time.jsonl).  One process per shape:
--shape A, B or C.

  A   1 GiB of text at block_len 2^16 cut into 64 equal ranges: long bodies, nearly every piece of the output inside one body
  B   the same container cut into 4 096 ranges of 4 blocks: a seam every tenth piece or so
  C   64 MiB of text at block_len 2^12 cut into 16 384 ranges of one block: several seams in every piece

  cut_ms         the whole call: five launches, through a sized index made before
  emit_ms        its copy kernel alone (tsqa_profile_read_cut: events around that one launch, in runs of their own)
  copy_ms        tsqa_measure_copy's kernel on as many bytes as the cut's arena has, in the same process: its median rate turned into
                 the time for those bytes; emit_over_copy_rate is the ratio of the two rates
  join_emit_ms   the copy kernel of tsqa_join_async joining the cut's containers back (tsqa_profile_read_join)
  recompress_ms  the range reads, then the packed compress of the pieces, both enqueued with no host wait between them
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name, bytes, block_len, ranges
SHAPES = {"A": ("text_1GiB_2^16_64_ranges", 1 << 30, 1 << 16, 64), "B": ("text_1GiB_2^16_4096_ranges", 1 << 30, 1 << 16, 4096),
          "C": ("text_64MiB_2^12_16384_ranges", 64 << 20, 1 << 12, 16384)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=0, help="another input size (a rehearsal at a small one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_time.jsonl"), help="the JSON line is appended to this file")
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
    ext, align = 1, 16
    name, total, block_len, n = SHAPES[args.shape]
    total = args.bytes or total
    nb = total // block_len
    per = nb // n
    assert nb * block_len == total and per * n == nb and per >= 1

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
    i64 = lambda k: torch.zeros(k, dtype=torch.int64, device="cuda")
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda")

    # the container and its index, on the stream
    src = torch.from_numpy(tsq.synth.text(total, seed=5)).cuda()
    blob = torch.empty(tsq.plan_split(total, block_len)[1], dtype=torch.uint8, device="cuda")
    table = i32(nb)
    codec.compress_split_async(src, ext, block_len, blob, table)
    s.synchronize()
    size, status = codec.last_size_status()
    assert status == 0
    blob = blob[:size].clone()
    idx = codec.index_sized(blob, total, block_len, table, sync=False)
    d_first = torch.arange(n, dtype=torch.int64, device="cuda") * per
    d_count = torch.full((n,), per, dtype=torch.int64, device="cuda")
    d_offsets, d_sizes, d_totals, d_status, d_word = i64(n + 1), i64(n), i64(n), i32(n), i32(1)

    def cut(out):
        rc = L.tsqa_cut_async(codec.h, idx.h, d_first.data_ptr(), d_count.data_ptr(), n, align, out.data_ptr() if out is not None else None,
                              out.numel() if out is not None else 0, d_offsets.data_ptr(), d_sizes.data_ptr(), d_totals.data_ptr(),
                              d_status.data_ptr(), d_word.data_ptr(), hs)
        assert rc == 0, codec.last_error()

    cut(None)
    s.synchronize()
    need = int(d_offsets[n].item())
    assert int(d_word.item()) == 6 and need > size
    arena = torch.zeros(need, dtype=torch.uint8, device="cuda")
    c = timed(lambda: cut(arena))
    s.synchronize()
    assert int(d_word.item()) == 0 and int(d_offsets[n].item()) == need and d_totals.sum().item() == total
    # the cut decodes to the ranges' data, which here is the input in order
    back = torch.zeros(total, dtype=torch.uint8, device="cuda")
    tables = codec._dense_tables(n)
    codec.decompress_batch_packed_dense_async(arena, d_offsets, d_sizes, n, nb, 1, back, *tables)
    s.synchronize()
    ok = codec.status() == 0 and bool(torch.equal(back, src))
    codec.profile(True)
    emit = []
    for r in range(args.warmup + args.reps):
        cut(arena)
        s.synchronize()
        ms, launches = codec.profile_read_cut()
        assert launches == 1
        if r >= args.warmup:
            emit.append(ms)
    m = timed(lambda: cut(None))
    cut(arena)

    # the join of the same containers back into one: the same copy with other seams
    joined = torch.zeros(size + 64, dtype=torch.uint8, device="cuda")
    j_first, j_status = i64(n + 1), i32(n)

    def join():
        codec.join_async(arena, d_offsets, d_sizes, n, nb, joined, j_first, None, j_status)

    join_emit = []
    for r in range(args.warmup + args.reps):
        join()
        s.synchronize()
        ms, launches = codec.profile_read_join()
        assert launches == 1 and codec.status() == 0
        if r >= args.warmup:
            join_emit.append(ms)
    codec.profile(False)
    unjoined = bool(torch.equal(joined[:size], blob))
    best, median = codec.measure_copy(max(need, 1 << 20), args.reps)
    copy_ms = 2.0 * need / (median * 1e9) * 1e3
    emit_gbps = 2.0 * need / (statistics.median(emit) * 1e-3) / 1e9
    join_gbps = 2.0 * size / (statistics.median(join_emit) * 1e-3) / 1e9

    # the other route, at its best: both calls asynchronous on the stream, the places known on the host
    piece = per * block_len
    reads = [(k * piece, piece, k * piece) for k in range(n)]
    items = [(k * piece, piece) for k in range(n)]
    again = torch.empty(sum(tsq.batch_bound(piece) + align for _ in range(n)), dtype=torch.uint8, device="cuda")
    r_offsets, r_sizes = i64(n + 1), i64(n)

    def recompress():
        idx.read_into(reads, back, sync=False)
        codec.compress_batch_packed_async(back, items, ext, align, again, r_offsets, r_sizes)

    back.zero_()
    recompress()
    s.synchronize()
    same = codec.status() == 0 and bool(torch.equal(back, src))
    r = timed(recompress)
    differing = int((r_sizes != d_sizes).sum().item())
    res = {"shape": name, "ranges": n, "blocks_per_range": per, "block_len": block_len, "bytes": total, "container_bytes": size,
           "arena_bytes": need, "reps": args.reps,
           "cut_ms": med(c), "cut_spread_ms": spread(c), "emit_ms": med(emit), "emit_spread_ms": spread(emit),
           "emit_gbps_read_plus_written": round(emit_gbps, 1), "measure_only_ms": med(m), "measure_only_spread_ms": spread(m),
           "copy_probe_gbps_median": round(median, 1), "copy_probe_gbps_best": round(best, 1), "copy_ms": round(copy_ms, 4),
           "copy_probe_shape": codec.copy_probe_shape(), "emit_over_copy_rate": round(emit_gbps / median, 3),
           "join_emit_ms": med(join_emit), "join_emit_spread_ms": spread(join_emit), "join_emit_gbps_read_plus_written": round(join_gbps, 1),
           "emit_over_join_emit_rate": round(emit_gbps / join_gbps, 3),
           "recompress_ms": med(r), "recompress_spread_ms": spread(r), "recompress_over_cut": round(statistics.median(r) / statistics.median(c), 1),
           "recompressed_containers_of_another_size": differing,
           "cut_decodes_to_the_ranges": ok, "join_of_the_cut_is_the_container": unjoined, "recompress_decodes_to_the_ranges": same}
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    idx.close()


if __name__ == "__main__":
    main()
