"""Timing of the take -- items and block ranges of a packed batch cut out through its device index (tsqa_cut_items_async) -- against
the route there was before it: a decode of the chosen data (tsqa_decompress_batch_packed_dense_async of the chosen items; for pages
inside items a gather, tsqa_gather_async) followed by a packed compress from device tables (tsqa_compress_batch_packed_tables*_async)
-- whose bytes differ at block edges --, and against copy speed: its copy kernel alone (cut_emit_kernel, tsqa_profile_read_cut) and
tsqa_measure_copy's kernel on as many bytes.  Device events on one stream with nothing else on the device, warm-ups first, the
median of --reps with the minimum and the maximum kept.  One JSON line per shape, printed and appended to --out
(profiles/take_time.jsonl).  One process per shape: --shape A, B, C or D.  Text from synth, ext on.

  A   4 096 items of 64 KiB, every second item taken
  B   the same, all items in a seeded shuffle
  C   64 items of 16 MiB at block_len 2^16, every item cut into pages of 4 blocks
  D   262 144 one-byte containers, all taken

  take_ms            the whole call: the measure, the three layout launches, the copy
  emit_ms            its copy kernel alone (events around that one launch, in runs of their own)
  layout_ms          the call with no output: the measure and the three layout launches
  copy_ms            tsqa_measure_copy's median rate turned into the time for the taken arena's bytes
  recompress_ms      the decode route, both calls enqueued with no host wait between them

The lines of profiles/take_time.jsonl also hold one_group_* / three_launch_* fields: the layout alone through tsqa_cut_async, which
then had a one-workgroup layout kernel of its own, against these three launches.  That kernel is gone and both calls share the three.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name, items, bytes per item, block_len (None: plain 4 MiB blocks), what is taken
SHAPES = {"A": ("4096_items_64KiB_every_second", 4096, 1 << 16, None, "every_second"),
          "B": ("4096_items_64KiB_shuffled", 4096, 1 << 16, None, "shuffle"),
          "C": ("64_items_16MiB_2^16_pages_of_4", 64, 16 << 20, 1 << 16, "pages"),
          "D": ("262144_items_1B_all", 262144, 1, None, "all")}
PAGE_BLOCKS = 4
SEED = 11


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--items", type=int, default=0, help="another item count (a rehearsal at a small one)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "take_time.jsonl"), help="the JSON line is appended to this file")
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
    name, n_items, item_len, block_len, what = SHAPES[args.shape]
    n_items = args.items or n_items
    total = n_items * item_len

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

    # the batch: packed compress from device tables, then its device index, on the stream
    src = torch.from_numpy(tsq.synth.text(total, seed=5)).cuda()
    in_offsets = torch.arange(n_items, dtype=torch.int64, device="cuda") * item_len
    in_sizes = torch.full((n_items,), item_len, dtype=torch.int64, device="cuda")
    per_item = 1 if block_len is None else item_len // block_len
    nb = n_items * per_item
    bound = lambda n_bytes: (tsq.plan_split(n_bytes, block_len)[1] if block_len else tsq.batch_bound(n_bytes)) + align
    arena = torch.empty(n_items * bound(item_len), dtype=torch.uint8, device="cuda")
    b_offsets, b_sizes, b_first, b_status = i64(n_items + 1), i64(n_items), i64(n_items + 1), i32(n_items)
    table = i32(nb) if block_len else None
    if block_len:
        codec.compress_batch_packed_tables_split_async(src, in_offsets, in_sizes, n_items, nb, ext, align, block_len, arena, b_offsets, b_sizes, b_first,
                                                       None, table, b_status)
    else:
        codec.compress_batch_packed_tables_async(src, in_offsets, in_sizes, n_items, nb, ext, align, arena, b_offsets, b_sizes, b_first, None, b_status)
    s.synchronize()
    assert codec.status() == 0, codec.status()
    arena_bytes = int(b_offsets[n_items].item())
    arena = arena[:arena_bytes].clone()
    index = codec.index_packed_async(arena, b_offsets, b_sizes, n_items, nb, block_len, b_first if block_len else None, table)
    s.synchronize()
    assert codec.status() == 0

    # what is taken: born on the device
    g = torch.Generator(device="cuda")
    g.manual_seed(SEED)
    d_first = d_count = None
    if what == "every_second":
        d_items = torch.arange(0, n_items, 2, dtype=torch.int32, device="cuda")
    elif what == "shuffle":
        d_items = torch.randperm(n_items, generator=g, device="cuda").to(torch.int32)
    elif what == "all":
        d_items = torch.arange(n_items, dtype=torch.int32, device="cuda")
    else:
        pages = per_item // PAGE_BLOCKS
        d_items = torch.arange(n_items, dtype=torch.int32, device="cuda").repeat_interleave(pages)
        d_first = (torch.arange(pages, dtype=torch.int64, device="cuda") * PAGE_BLOCKS).repeat(n_items)
        d_count = torch.full((n_items * pages,), PAGE_BLOCKS, dtype=torch.int64, device="cuda")
    n = int(d_items.numel())
    t_offsets, t_sizes, t_totals, t_status, t_word = i64(n + 1), i64(n), i64(n), i32(n), i32(1)
    ptr = lambda t: t.data_ptr() if t is not None else None

    def take(out):
        rc = L.tsqa_cut_items_async(codec.h, index.h, d_items.data_ptr(), ptr(d_first), ptr(d_count), n, align, ptr(out),
                                    out.numel() if out is not None else 0, t_offsets.data_ptr(), t_sizes.data_ptr(), t_totals.data_ptr(),
                                    t_status.data_ptr(), t_word.data_ptr(), hs)
        assert rc == 0, codec.last_error()

    take(None)
    s.synchronize()
    need = int(t_offsets[n].item())
    assert int(t_word.item()) == 6 and need > 0
    taken = torch.zeros(need, dtype=torch.uint8, device="cuda")
    t = timed(lambda: take(taken))
    s.synchronize()
    taken_bytes = int(t_totals.sum().item())
    assert int(t_word.item()) == 0 and int(t_offsets[n].item()) == need

    # the take decodes to the chosen data
    length = PAGE_BLOCKS * block_len if d_first is not None else item_len
    items64 = d_items.to(torch.int64)
    rows = items64 if d_first is None else items64 * (item_len // length) + d_first // PAGE_BLOCKS
    want = src.view(total // length, length)[rows].reshape(-1)
    back = torch.zeros(taken_bytes, dtype=torch.uint8, device="cuda")
    tables = codec._dense_tables(n)
    blocks_taken = n * (PAGE_BLOCKS if d_first is not None else per_item)
    codec.decompress_batch_packed_dense_async(taken, t_offsets, t_sizes, n, blocks_taken, 1, back, *tables)
    s.synchronize()
    ok = codec.status() == 0 and taken_bytes == n * length and bool(torch.equal(back, want))
    del want

    codec.profile(True)
    emit = []
    for r in range(args.warmup + args.reps):
        take(taken)
        s.synchronize()
        ms, launches = codec.profile_read_cut()
        assert launches == 1
        if r >= args.warmup:
            emit.append(ms)
    codec.profile(False)
    m = timed(lambda: take(None))
    take(taken)
    best, median = codec.measure_copy(max(need, 1 << 20), args.reps)
    copy_ms = 2.0 * need / (median * 1e9) * 1e3
    emit_gbps = 2.0 * need / (statistics.median(emit) * 1e-3) / 1e9

    # the route before the take: decode the chosen data, compress it again from device tables; no host wait in between
    again = torch.empty(n * bound(length), dtype=torch.uint8, device="cuda")
    r_offsets, r_sizes, r_first, r_status = i64(n + 1), i64(n), i64(n + 1), i32(n)
    r_in_offsets = torch.arange(n, dtype=torch.int64, device="cuda") * length
    r_in_sizes = torch.full((n,), length, dtype=torch.int64, device="cuda")
    r_table = i32(blocks_taken) if block_len else None
    g_lengths = torch.full((n,), length, dtype=torch.int64, device="cuda")
    g_out_offsets, g_status, g_need = i64(n + 1), i32(n), i64(1)
    g_offsets = d_first * block_len if d_first is not None else None

    def recompress():
        if d_first is None:
            # the chosen containers' places, picked on the device
            codec.decompress_batch_packed_dense_async(arena, b_offsets[items64], b_sizes[items64], n, blocks_taken, 1, back, *tables)
            codec.compress_batch_packed_tables_async(back, r_in_offsets, r_in_sizes, n, blocks_taken, ext, align, again, r_offsets, r_sizes, r_first, None,
                                                     r_status)
        else:
            codec.gather_async(index, d_items, g_offsets, g_lengths, n, 1, blocks_taken, back, g_out_offsets, g_status, g_need)
            codec.compress_batch_packed_tables_split_async(back, r_in_offsets, r_in_sizes, n, blocks_taken, ext, align, block_len, again, r_offsets,
                                                           r_sizes, r_first, None, r_table, r_status)

    back.zero_()
    recompress()
    s.synchronize()
    same = codec.status() == 0 and int(r_status.abs().sum().item()) == 0
    rr = timed(recompress)
    differing = int((r_sizes != t_sizes).sum().item())

    res = {"shape": name, "items": n_items, "item_bytes": item_len, "block_len": block_len, "ranges": n, "blocks_per_range": blocks_taken // n,
           "arena_bytes": arena_bytes, "taken_arena_bytes": need, "taken_data_bytes": taken_bytes, "reps": args.reps,
           "take_ms": med(t), "take_spread_ms": spread(t), "emit_ms": med(emit), "emit_spread_ms": spread(emit),
           "emit_gbps_read_plus_written": round(emit_gbps, 1), "layout_ms": med(m), "layout_spread_ms": spread(m),
           "copy_probe_gbps_median": round(median, 1), "copy_probe_gbps_best": round(best, 1), "copy_ms": round(copy_ms, 4),
           "copy_probe_shape": codec.copy_probe_shape(), "emit_over_copy_rate": round(emit_gbps / median, 3),
           "recompress_ms": med(rr), "recompress_spread_ms": spread(rr), "recompress_over_take": round(statistics.median(rr) / statistics.median(t), 1),
           "recompressed_containers_of_another_size": differing,
           "take_decodes_to_the_chosen_data": ok, "recompress_route_ran_clean": same}
    line = json.dumps(res)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    index.close()


if __name__ == "__main__":
    main()
