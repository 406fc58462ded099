"""Encoder conformance catalogue: inputs aimed at the seams of the staged encoder (turbosqueeze_amd/csrc/tsq_enc_stage.cuh), and the
census that says which of the encoder's rules an input exercises.

Three parts:
  * census(): pure functions from the oracle's trace (oracle/tsq_oracle.h: tsqo_trace_rec, one record per probed position) plus plain
    geometry -- 64-position tiles, ring positions modulo WIN, hashes and folds computed here with the kernel's formulas -- to named
    counters, one per seam.  A counter never calls a kernel.
  * the catalogue: seeded, deterministic builders.  Each gives (name, data, halo or None) and declares the counters it aims at, per level.
  * kill_matrix(): which of the oracle's mutants (single-rule errors, pyoracle.MUTANTS) a set of inputs can tell from the truth.

The constants below mirror StageCfgT / the stage functions of tsq_enc_stage.cuh and must be re-derived with them: a kernel change that
moves one of them moves the seams, and the catalogue has to follow.
"""
from __future__ import annotations

import hashlib

import numpy as np

from oracle import pyoracle as po

# ---- mirrors of the kernel's constants (tsq_enc_stage.cuh) ---------------------------------------------------------------------------
TILE = 64                       # positions per tile record
WIN = 66560                     # StageCfgT<true>::WIN: the input window ring (standard layout), 32 bytes mirrored behind it
LM, LF = 4, 3                   # table lag and late-fix lag, both layouts
R = 11                          # tile records in flight (standard layout)
FOLD_BITS_STD, FOLD_BITS_LEAN = 15, 14   # owner image: OWN_MASK 0x7FFF (standard), 0x3FFF (lean)
Q, EQ, RING = 16, 64, 256       # item queue, event queue, symbol ring: chains longer than these run without a literal in between
OWNER_TILES = 4                 # the owner image names lanes of the last four tiles
BLOCK = 1 << 22
HALO = 128


def k_dmin(ext):                # a word-equal candidate nearer than this makes a hazard lane (MATCH / ORBIT: kDMin)
    return 128 if ext else 64


def hash17(words):
    w = words.astype(np.uint32)
    return (w ^ (w >> np.uint32(12))) & np.uint32(0x1FFFF)


def fold(h, bits):              # StageCfgT::fold
    return ((h.astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - bits)


def words_of(buf, n):
    """the 4-byte little-endian word at every position 0..n-1 of buf (which carries the halo)"""
    b = buf.astype(np.uint32)
    return b[0:n] | (b[1:n + 1] << 8) | (b[2:n + 2] << 16) | (b[3:n + 3] << 24)


def with_halo(data, halo):
    buf = np.zeros(len(data) + HALO, dtype=np.uint8)
    buf[:len(data)] = np.frombuffer(bytes(data), dtype=np.uint8)
    if halo is not None:
        h = np.frombuffer(bytes(halo), dtype=np.uint8)[:HALO]
        buf[len(data):len(data) + h.size] = h
    return buf


def _prev_same(keys):
    """for every index the nearest earlier index with an equal key, or -1"""
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    prev = np.full(keys.size, -1, dtype=np.int64)
    same = ks[1:] == ks[:-1]
    prev[order[1:][same]] = order[:-1][same]
    return prev


def _runs(mask):
    """lengths of the maximal runs of True"""
    if mask.size == 0:
        return np.zeros(0, dtype=np.int64)
    m = np.concatenate([[False], mask, [False]]).astype(np.int8)
    d = np.diff(m)
    return np.flatnonzero(d == -1) - np.flatnonzero(d == 1)


# ---- the counters --------------------------------------------------------------------------------------------------------------------
DISTS = (4, 5, 63, 64, 65, 127, 128, 129, 0xFFFD, 0xFFFE, 0xFFFF, 0x10000)
KRAWS_NOEXT = (4, 16)
KRAWS_EXT = (4, 16, 17, 31, 32, 47, 48, 63, 64)
LIT_RUNS = (31, 32, 33, 47, 48, 64)
TAIL_NS = tuple(range(1, 9)) + (63, 64, 65, 127, 128, 129, BLOCK - 1, BLOCK)

# Removed, because the format cannot reach them:
#   raw k == 3: the prefix is only computed after the 4-byte words compared equal, so k_raw >= 4 (k == 3 AFTER the clamp is room_clamp_lt4).
#   raw k >= 72: common_prefix adds at most 8 per step and stops at the first step that reaches the cap from below it: k_raw <= 64
#       with extensions, <= 16 without (so 17 .. 64 and the nibble-class clamps exist with extensions only).
#   offset in {0xFFFF, >= 0x10000, not wrapped} refused while i - pos alone would pass: the pair origin is never beyond i, so
#       offset <= i - pos; only a candidate INSIDE the open pair (offset wraps below zero) is refused with a passing distance.
#   a tile with no visited position inside one 64-byte match: a span is at most 64 positions and starts at a visited one, so every
#       tile a chain crosses holds a probe; the nearest thing, a tile with exactly one visited position, is counted instead.
#   run of N pending "at the forced flush": the flush fires at exactly 32 pending bytes; the counters are the literal run lengths.


def counter_names(ext):
    names = [f"dist_{d:#x}_word_equal" for d in DISTS]
    names += ["offset_4_accepted", "offset_0xfffe_accepted", "dist_0xffff_match", "dist_0x10000_match",
              "offset_3_refused_dist_ok", "offset_wrapped_refused_dist_ok", "offset_3_refused_dist_3",
              "offset_0xffff_refused_dist_fails", "offset_0x10000_refused_dist_fails"]
    names += ["empty_bucket_before_64k", "empty_bucket_at_65536", "stale_alias_word_differs", "stale_alias_word_equal",
              "stale_alias_match", "same_hash_other_word_1to3_back", "same_hash_other_word_same_tile"]
    names += [f"same_hash_other_word_{t}_tiles_back" for t in (1, 2, 3, 4, 5)]
    names += ["recent_same_hash_skipped_in_span"]
    names += ["fold15_collision_within_4_tiles", "fold14_collision_within_4_tiles", "three_lanes_one_bucket"]
    names += [f"bucket_writer_{t}_tiles_back" for t in (4, 5, 8)]
    names += ["room_clamp_ge4", "room_clamp_lt4", "match_second_after_literal", "match_second_after_match"]
    if ext:
        names += ["clamp_32_to_31", "clamp_17_to_16"]
    names += [f"k_raw_{k}" for k in (KRAWS_EXT if ext else KRAWS_NOEXT)]
    names += ["chain_ge_8", "chain_ge_64", "chain_ge_300"]
    names += [f"literal_run_{r}" for r in LIT_RUNS]
    names += ["forced_flush_decides_offset", "spill_adopted_as_control", "spill_adopted_as_size"]
    names += [f"n_{n}" for n in TAIL_NS]
    names += ["match_start_n_minus_6", "match_start_n_minus_5", "match_start_n_minus_4", "match_past_n_zero_halo",
              "match_past_n_halo_continues", "final_symbols_odd", "final_group_of_1", "final_group_of_7"]
    names += ["ring_candidate_straddles_end", "ring_own_position_straddles_end", "ring_dist_0x10000_across_wrap"]
    if ext:
        names += [f"ring_candidate_extension_{s}_straddles" for s in (16, 32, 48)]
        names += [f"ring_own_extension_{s}_straddles" for s in (16, 32, 48)]
    names += ["hazard_tile", "eight_hazard_tiles_in_a_row", "tile_all_visited"]
    if ext:
        names += ["tile_one_visited"]                        # (without extensions a span is at most 16 positions)
    return names


def census(oracle, data, halo, ext):
    """-> (stream, {counter: count}) of one block"""
    data = bytes(data)
    n = len(data)
    stream, tr = oracle.encode_block_traced(data, ext, halo)
    trimmed, _ = oracle.encode_block_traced(data, ext, halo, mutant=po.MUTANTS.index("trim_spill"), trace=False)
    buf = with_halo(data, halo)
    words = words_of(buf, n + 64)
    c = dict.fromkeys(counter_names(ext), 0)

    def put(name, mask):
        c[name] = int(np.count_nonzero(mask))

    i = tr["i"].astype(np.int64)
    pos = tr["pos"].astype(np.int64)
    pos = np.where(pos >= 1 << 31, pos - (1 << 32), pos)
    oo, ot = tr["origin_at_offset"].astype(np.int64), tr["origin_at_test"].astype(np.int64)
    offset, kraw, k, outcome = tr["offset"].astype(np.int64), tr["k_raw"].astype(np.int64), tr["k"].astype(np.int64), tr["outcome"]
    weq = (tr["flags"] & po.TF_WORD_EQUAL) != 0
    chain = (tr["flags"] & po.TF_CHAIN_PROBE) != 0
    nib = (tr["flags"] >> 8) & 15
    match = outcome == po.OUT_MATCH
    dist = i - pos
    off_ok = (offset >= 4) & (offset <= 0xFFFE)
    inside = i < n                                           # a probe at or beyond n is the end of the scan / chain
    passed = weq & off_ok & np.where(chain, i < n - 5, inside)
    refused = weq & ~off_ok & inside
    span = np.where(ext & (nib < 3), (nib + 2) << 4, nib + 1).astype(np.int64)

    for d in DISTS:
        put(f"dist_{d:#x}_word_equal", weq & (dist == d) & inside)
    put("offset_4_accepted", passed & (offset == 4))
    put("offset_0xfffe_accepted", passed & (offset == 0xFFFE))
    put("dist_0xffff_match", match & (dist == 0xFFFF))
    put("dist_0x10000_match", match & (dist == 0x10000))
    dist_ok = (dist >= 4) & (dist <= 0xFFFE)
    put("offset_3_refused_dist_ok", refused & (offset == 3) & dist_ok)
    put("offset_wrapped_refused_dist_ok", refused & (offset > 0xFFFFFF) & dist_ok)
    put("offset_3_refused_dist_3", refused & (offset == 3) & (dist == 3))
    put("offset_0xffff_refused_dist_fails", refused & (offset == 0xFFFF) & ~dist_ok)
    put("offset_0x10000_refused_dist_fails", refused & (offset == 0x10000) & ~dist_ok)

    # the table, replayed: every probe inserts its position
    wi = words[np.minimum(i, words.size - 1)]
    hi = hash17(wi)
    prev_rec = _prev_same(hi)                               # the probe that wrote the bucket last
    has_prev = prev_rec >= 0
    last_ins = np.where(has_prev, i[np.maximum(prev_rec, 0)], -1)
    put("empty_bucket_before_64k", ~has_prev & (i < 65536) & inside)
    put("empty_bucket_at_65536", ~has_prev & (i == 65536) & inside)
    stale = has_prev & (i - last_ins > 65536) & inside
    put("stale_alias_word_differs", stale & ~weq)
    put("stale_alias_word_equal", stale & weq)
    put("stale_alias_match", stale & match)
    other = has_prev & (words[np.maximum(last_ins, 0)] != wi) & inside
    back = i - last_ins
    tiles_back = (i >> 6) - (last_ins >> 6)
    put("same_hash_other_word_1to3_back", other & (back <= 3))
    put("same_hash_other_word_same_tile", other & (tiles_back == 0))
    for t in (1, 2, 3, 4, 5):
        put(f"same_hash_other_word_{t}_tiles_back", other & (tiles_back == t))
    h_all = hash17(words[:n])
    prev_any = _prev_same(h_all)                            # over every position, visited or not
    pa = prev_any[np.minimum(i, n - 1)] if n else np.zeros(0, dtype=np.int64)
    put("recent_same_hash_skipped_in_span", inside & (pa > last_ins) & (i - pa <= 65536) & (pa > 0))

    # the owner image sees every position of a tile, visited or not
    allpos = np.arange(n, dtype=np.int64)
    for bits, name in ((FOLD_BITS_STD, "fold15"), (FOLD_BITS_LEAN, "fold14")):
        f = fold(h_all, bits)
        pf = _prev_same(f)
        ok = pf >= 0
        tb = (allpos >> 6) - (np.maximum(pf, 0) >> 6)
        put(f"{name}_collision_within_4_tiles", ok & (h_all[np.maximum(pf, 0)] != h_all) & (tb <= OWNER_TILES))
        if bits == FOLD_BITS_STD:
            for t in (4, 5, 8):
                put(f"bucket_writer_{t}_tiles_back", ok & (tb == t))
            key = (allpos >> 6) * (1 << bits) + f.astype(np.int64)
            _, cnt = np.unique(key, return_counts=True)
            put("three_lanes_one_bucket", cnt >= 3)

    # room
    have_k = kraw != po.NO_K
    room = ot - pos
    clamped = have_k & (kraw > room) & (room >= 0)
    put("room_clamp_ge4", clamped & (room - 1 >= 4))
    put("room_clamp_lt4", clamped & (room - 1 < 4))
    if ext:
        put("clamp_32_to_31", clamped & (kraw >= 32) & (k == 31))
        put("clamp_17_to_16", clamped & (kraw >= 17) & (k == 16))
    put("match_second_after_literal", match & (ot != i) & ~chain)
    put("match_second_after_match", match & (ot != i) & chain)
    for kk in (KRAWS_EXT if ext else KRAWS_NOEXT):
        put(f"k_raw_{kk}", have_k & (kraw == kk))
    runs = _runs(match)
    for m in (8, 64, 300):
        put(f"chain_ge_{m}", runs >= m)

    # literal runs: from where the last chain broke (or 0) to the scan probe that ended the scan
    brk = np.isin(outcome, (po.OUT_BREAK_WORD, po.OUT_BREAK_OFFSET, po.OUT_BREAK_SHORT, po.OUT_BREAK_TAIL, po.OUT_BREAK_OFFSET_LATE))
    ends = ~chain & np.isin(outcome, (po.OUT_MATCH, po.OUT_BREAK_SHORT, po.OUT_END, po.OUT_BREAK_OFFSET_LATE))
    brk_idx = np.flatnonzero(brk)
    end_idx = np.flatnonzero(ends)
    at = np.searchsorted(brk_idx, end_idx, side="left") - 1           # the last break strictly before the end record
    start = np.where(at >= 0, i[brk_idx[np.maximum(at, 0)]] if brk_idx.size else 0, 0)
    lit = np.minimum(i[end_idx], n) - start
    for r in LIT_RUNS:
        put(f"literal_run_{r}", lit == r)
    forced = (tr["flush"] & po.FL_FORCED) != 0
    after = ot - pos
    put("forced_flush_decides_offset", forced & weq & inside & (off_ok != ((after >= 4) & (after <= 0xFFFE))))

    # symbols: matches, two literals per forced flush, the flush before a match in chunks of 16
    before = (tr["flush"] >> 8).astype(np.int64) * ((tr["flush"] & po.FL_BEFORE_MATCH) != 0)
    nsym = int(np.count_nonzero(match) + 2 * np.count_nonzero(forced) + np.sum((before + 15) // 16))
    # a literal's 16-byte store spills behind it; the spill survives only in a trailing control / size byte that no symbol shifted
    if nsym and nsym % 8 == 0 and len(stream) == len(trimmed):
        c["spill_adopted_as_control"] = int(stream[-2] != trimmed[-2])
    if nsym and nsym % 2 == 0 and len(stream) == len(trimmed):
        c["spill_adopted_as_size"] = int(stream[-1] != trimmed[-1])
    if f"n_{n}" in c:
        c[f"n_{n}"] = 1
    for back_, name in ((6, "match_start_n_minus_6"), (5, "match_start_n_minus_5"), (4, "match_start_n_minus_4")):
        put(name, match & (i == n - back_))
    past = match & (i + span > n)
    zero_halo = halo is None or not any(bytes(halo))
    c["match_past_n_zero_halo"] = int(np.count_nonzero(past)) if zero_halo else 0
    c["match_past_n_halo_continues"] = int(np.count_nonzero(past & (i + k > n))) if not zero_halo else 0
    c["final_symbols_odd"] = nsym & 1
    c["final_group_of_1"] = int(nsym % 8 == 1)
    c["final_group_of_7"] = int(nsym % 8 == 7)

    # the ring (a property of the input; only the standard layout has one)
    cand = weq & inside & (pos >= 0)
    put("ring_candidate_straddles_end", cand & (pos % WIN > WIN - 20) & (pos >= WIN - 19))
    put("ring_own_position_straddles_end", cand & (i % WIN > WIN - 20))
    put("ring_dist_0x10000_across_wrap", cand & (dist == 0x10000) & (pos // WIN != i // WIN))
    if ext:
        for s in (16, 32, 48):
            put(f"ring_candidate_extension_{s}_straddles", have_k & (kraw > s) & ((pos + s) % WIN > WIN - 16))
            put(f"ring_own_extension_{s}_straddles", have_k & (kraw > s) & ((i + s) % WIN > WIN - 16))

    # density
    ntiles = (n + TILE - 1) // TILE
    vis = np.bincount((i[inside] >> 6), minlength=ntiles)[:ntiles]
    haz = np.bincount((i[inside & weq & (dist < k_dmin(ext))] >> 6), minlength=ntiles)[:ntiles] >= 12
    put("hazard_tile", haz)
    put("eight_hazard_tiles_in_a_row", _runs(haz) >= 8)
    full = np.full(ntiles, TILE)
    if ntiles:
        full[0] = TILE - 1                                   # position 0 is never probed
        full[-1] = n - (ntiles - 1) * TILE - (1 if ntiles == 1 else 0)
    put("tile_all_visited", (vis == full) & (full >= TILE - 1))
    if ext:
        put("tile_one_visited", vis == 1)
    return stream, c


# ---- builders ------------------------------------------------------------------------------------------------------------------------

def _rng(seed):
    return np.random.default_rng(seed)


def _rnd(rng, n):
    return rng.integers(0, 256, size=n, dtype=np.uint8)


def _free_word(rng, arr):
    """four bytes whose 17-bit hash no position of arr has"""
    used = np.zeros(1 << 17, dtype=bool)
    used[hash17(words_of(np.concatenate([arr, np.zeros(4, dtype=np.uint8)]), arr.size))] = True
    while True:
        w = _rnd(rng, 4)
        if not used[int(hash17(words_of(np.concatenate([w, np.zeros(4, dtype=np.uint8)]), 1))[0])]:
            return w


class Case:
    def __init__(self, name, data, halo=None, aims=None, aims_ext=None, aims_noext=None):
        self.name, self.halo = name, (bytes(halo) if halo is not None else None)
        self.data = data.tobytes() if isinstance(data, np.ndarray) else bytes(data)
        self.aims = {0: sorted(set(aims or ()) | set(aims_noext or ())), 1: sorted(set(aims or ()) | set(aims_ext or ()))}

    def blocks(self):
        """(data, halo) of every 4 MiB block: a block's halo is the next block's head"""
        d = self.data
        if len(d) <= BLOCK:
            return [(d, self.halo)]
        return [(d[a:a + BLOCK], (d[a + BLOCK:a + BLOCK + HALO] or None) if a + BLOCK < len(d) else self.halo)
                for a in range(0, len(d), BLOCK)]


def near_periods(seed):
    """runs of period P after literal prefixes of every parity: candidates at distance P, rooms of P"""
    rng = _rng(seed)
    parts = []
    for p in list(range(1, 36)) + [47, 48, 49, 63, 64, 65, 66, 127, 128, 129, 130]:
        for gap in (int(rng.integers(1, 8)), int(rng.integers(8, 40))):
            parts += [_rnd(rng, gap), np.resize(_rnd(rng, p), p + int(rng.integers(70, 200)))]
    return Case("near_periods", np.concatenate(parts), None,
                aims=["dist_0x4_word_equal", "dist_0x5_word_equal", "dist_0x3f_word_equal", "dist_0x40_word_equal", "dist_0x41_word_equal",
                      "dist_0x7f_word_equal", "dist_0x80_word_equal", "dist_0x81_word_equal", "offset_4_accepted", "room_clamp_ge4",
                      "room_clamp_lt4", "hazard_tile", "three_lanes_one_bucket",
                      "same_hash_other_word_1to3_back"],
                aims_ext=["clamp_32_to_31"])


def far_phrases(seed):
    """40-byte phrases copied at distances around the 16-bit edge, behind literal prefixes of varied length so that the pair origin
    sits 0 .. 20 bytes before the copy: offsets 0xFFFE accepted, 0xFFFF and 0x10000 refused, a candidate 65 536 back taken"""
    rng = _rng(seed)
    dists = [0xFFFD, 0xFFFE, 0xFFFF, 0x10000, 0x10001, 0x10002, 0x10003]
    n = 0x10000 + 56000
    a = _rnd(rng, n)
    src = 1200
    for rep in range(40):
        for d in dists:
            ln = 40
            a[src + d:src + d + ln] = a[src:src + ln]
            src += ln + int(rng.integers(30, 70))
    return Case("far_phrases", a, None,
                aims=["dist_0xfffd_word_equal", "dist_0xfffe_word_equal", "dist_0xffff_word_equal", "dist_0x10000_word_equal",
                      "offset_0xfffe_accepted", "dist_0xffff_match", "dist_0x10000_match", "offset_0xffff_refused_dist_fails",
                      "offset_0x10000_refused_dist_fails", "ring_dist_0x10000_across_wrap", "tile_all_visited",
                      "empty_bucket_before_64k"])


def origin_shift(seed):
    """a copy whose candidate is right at the 16-bit edge, reached as the second symbol of a pair whose first symbol is a literal of
    every length 1 .. 16 (the pair origin that many bytes before the copy) and as a chain link after a match"""
    rng = _rng(seed)
    n = 0x10000 + 60000
    a = _rnd(rng, n)
    src = 1000
    for lit in range(1, 17):
        for extra in (0, 1, 2):
            # [copy of 24 bytes from a nearby place, closing a symbol] [lit fresh bytes] [copy of the far phrase]
            d = 0xFFFE + lit + extra - 1
            at = src + d
            a[at:at + 36] = a[src:src + 36]
            a[at - lit - 24:at - lit] = a[at - lit - 24 - 300:at - lit - 300]
            src += 36 + 24 + lit + int(rng.integers(40, 60))
    return Case("origin_shift", a, None,
                aims=["offset_0xfffe_accepted", "match_second_after_literal", "dist_0xffff_match", "dist_0x10000_match"])


def lengths(seed):
    """copies of every exact length 4 .. 70 from a dictionary of random phrases, each followed by a byte that ends the prefix; nearer
    than kDMin and farther"""
    rng = _rng(seed)
    dic = _rnd(rng, 72 * 80)
    parts = [dic]
    for rep, gaplen in enumerate((3, 9, 20)):
        for ln in range(4, 72):
            s = (ln - 4) * 80 + 3
            parts += [_rnd(rng, gaplen + int(rng.integers(0, 3))), dic[s:s + ln], np.array([dic[s + ln] ^ 0x55], dtype=np.uint8)]
    # the same nearer than kDMin: phrase, two fresh bytes, phrase again
    for ln in range(4, 72):
        ph = _rnd(rng, ln)
        parts += [_rnd(rng, 5), ph, _rnd(rng, 2), ph, _rnd(rng, 1)]
    return Case("lengths", np.concatenate(parts), None, aims=["k_raw_4", "k_raw_16", "match_second_after_literal", "match_second_after_match"],
                aims_ext=[f"k_raw_{k}" for k in KRAWS_EXT])


def chains(seed):
    """a 24 000-byte region copied whole: hundreds of back-to-back matches, no literal"""
    rng = _rng(seed)
    # no two positions of the region share a hash, so no link's table entry is overwritten before the copy reads it
    region, used = [int(x) for x in _rnd(rng, 3)], set()
    while len(region) < 20000:
        b = int(rng.integers(0, 256))
        w = region[-3] | (region[-2] << 8) | (region[-1] << 16) | (b << 24)
        h = (w ^ (w >> 12)) & 0x1FFFF
        if h not in used:
            used.add(h)
            region.append(b)
    region = np.array(region, dtype=np.uint8)
    return Case("chains", np.concatenate([_rnd(rng, 50), region, _rnd(rng, 60), region, _rnd(rng, 77), region[:9000], _rnd(rng, 20)]),
                None, aims=["chain_ge_8", "chain_ge_64", "chain_ge_300", "recent_same_hash_skipped_in_span"], aims_ext=["tile_one_visited"])


def literal_runs(seed):
    """copies separated by exactly r fresh bytes, r around the forced flush at 32 pending bytes; and a forced flush that lands on a
    word-equal candidate 20 back, which only the offset taken BEFORE the flush refuses"""
    rng = _rng(seed)
    dic = _rnd(rng, 4000)
    parts = [dic]
    at = 0
    for rep in range(3):
        for r in (1, 15, 16, 17, 30, 31, 32, 33, 34, 46, 47, 48, 49, 63, 64, 65, 95, 96, 97):
            parts += [dic[at:at + 40], _rnd(rng, r)]
            at += 44
    for rep in range(6):
        fresh = _rnd(rng, 40)
        fresh[32:36] = fresh[12:16]
        parts += [dic[at:at + 40 + rep], fresh]
        at += 50
    return Case("literal_runs", np.concatenate(parts + [dic[100:140]]), None,
                aims=[f"literal_run_{r}" for r in LIT_RUNS] + ["forced_flush_decides_offset"])


def hash_twins(seed):
    """two words that differ in bits 29..31 only (one 17-bit hash, different bytes) 1 .. 3 positions apart, in one tile, and one to
    five tiles apart; the same word again exactly 4, 5 and 8 tiles later"""
    rng = _rng(seed)
    a = _rnd(rng, 30000)
    at = 256
    for t in (0, 1, 2, 3, 4, 5):
        for rep in range(3):
            w = _free_word(rng, a)
            a[at + 5:at + 9] = w
            w2 = w.copy(); w2[3] ^= 0x20 << int(rng.integers(0, 3))
            a[at + 64 * t + 20:at + 64 * t + 24] = w2
            at += 64 * 8
    for t in (4, 5, 8):
        for rep in range(3):
            w = _free_word(rng, a)
            a[at + 7:at + 11] = w
            a[at + 64 * t + 9:at + 64 * t + 13] = w
            at += 64 * 11
    for p in (1, 2, 3):                                        # 1 .. 3 back: a run of period p whose last byte flips bit 7
        for rep in range(3):
            run = np.resize(_rnd(rng, p), 24)
            run[-1] ^= 0x80
            a[at:at + 24] = run
            at += 100
    return Case("hash_twins", a, None,
                aims=["same_hash_other_word_1to3_back", "same_hash_other_word_same_tile"] + [f"same_hash_other_word_{t}_tiles_back" for t in (1, 2, 3, 4, 5)]
                + [f"bucket_writer_{t}_tiles_back" for t in (4, 5, 8)])


def fold_collisions(seed):
    """pairs of words with different hashes and one owner bucket, at 15 bits, at 14 bits, placed one to four tiles apart"""
    rng = _rng(seed)
    a = _rnd(rng, 40000)
    pool = rng.integers(0, 1 << 32, size=20000, dtype=np.uint64).astype(np.uint32)
    h = hash17(pool)
    at = 300
    for bits in (FOLD_BITS_STD, FOLD_BITS_LEAN):
        f = fold(h, bits)
        order = np.argsort(f, kind="stable")
        pairs = [(order[j], order[j + 1]) for j in range(order.size - 1) if f[order[j]] == f[order[j + 1]] and h[order[j]] != h[order[j + 1]]]
        for j, (x, y) in enumerate(pairs[:24]):
            t = j % 5
            a[at:at + 4] = np.frombuffer(int(pool[x]).to_bytes(4, "little"), dtype=np.uint8)
            a[at + 64 * t + 11:at + 64 * t + 15] = np.frombuffer(int(pool[y]).to_bytes(4, "little"), dtype=np.uint8)
            # the first word again right behind the second: its twin now hides behind a bucket another hash owns
            a[at + 64 * t + 30:at + 64 * t + 38] = a[at:at + 8]
            at += 64 * 7
    return Case("fold_collisions", a, None, aims=["fold15_collision_within_4_tiles", "fold14_collision_within_4_tiles"])


def stale_alias(seed):
    """a bucket whose last insertion lies more than 65 536 back: the 16-bit entry names a position one window later.  There the bytes
    differ (filler), or are the same word, unvisited inside a match span -- then the alias is taken as a match"""
    rng = _rng(seed)
    n = 0x10000 + 9000
    a = _rnd(rng, n)
    q = _rnd(rng, 80)
    for rep, base in enumerate((500, 2500, 4500)):
        w = _free_word(rng, a)
        q2 = q.copy(); q2[:4] = _rnd(rng, 4); q2[21:25] = w
        a[base:base + 80] = q2                     # visited as literals: w inserted at base + 21
        a[base + 1000:base + 1080] = q2            # matched against the first: w unvisited inside a span
        b = base + 0x10000
        a[b:b + 80] = q2                           # matched against the second: w at b + 21 unvisited, one window behind the insertion
        a[b + 300 + rep:b + 304 + rep] = w         # visited: the bucket still says base + 21, read as b + 21
        v = _free_word(rng, a)
        a[base + 1500:base + 1504] = v             # and one whose alias lands in filler
        a[base + 1500 + 0x10000 + 700:base + 1504 + 0x10000 + 700] = v
    # offset 3 at distance 3: the pair origin is i itself only behind a match, whose span covers i - 3 -- not in the table, but the
    # alias of a visited position 65 536 earlier.  Both parities of the symbol count, so that one of the two closes a pair at i.
    for variant in (0, 1):
        v = 6300 + 900 * variant
        while True:
            abc = _rnd(rng, 3)
            w = np.concatenate([abc, abc[:1]])
            if not np.any(hash17(words_of(np.concatenate([a, np.zeros(4, dtype=np.uint8)]), a.size)) == hash17(words_of(np.concatenate([w, w]), 1))[0]):
                break
        a[v:v + 4] = w
        m = np.concatenate([_rnd(rng, 13), abc])                # 16 bytes: one match symbol at either level
        a[v + 200:v + 216] = m
        a[v + 216] = w[0] ^ 0x11
        i = v + 3 + 0x10000
        a[i - 16:i] = m
        a[i:i + 4] = w
        r = (5, 20)[variant]                                  # one literal symbol or two between a helper match and the match
        a[i - 16 - r - 8:i - 16 - r] = a[v + 300:v + 308]
    a[0x10000:0x10004] = _free_word(rng, a)
    return Case("stale_alias", a, None, aims=["offset_3_refused_dist_3", "stale_alias_word_differs", "stale_alias_word_equal", "stale_alias_match",
                                             "empty_bucket_at_65536", "empty_bucket_before_64k"])


def ring_wrap(seed):
    """a phrase across the first ring end, copied from every start that makes the candidate's first bytes or one of its extension steps
    straddle the end; copies whose own position and own extension steps straddle the second, third and fourth end; a candidate
    65 536 back across a wrap"""
    rng = _rng(seed)
    n = 4 * WIN + 2000
    a = _rnd(rng, n)
    ph = _rnd(rng, 160)
    a[WIN - 70:WIN + 90] = ph
    dst = WIN + 3000
    for back in (3, 10, 19, 21, 37, 53, 31, 47, 63):
        a[dst:dst + 80] = ph[70 - back:150 - back]
        dst += 80 + int(rng.integers(20, 50))
    for wrap, back in ((2, 16 + 8), (3, 32 + 8), (4, 48 + 8)):
        ph2 = _rnd(rng, 100)
        a[wrap * WIN - 9000:wrap * WIN - 8900] = ph2
        a[wrap * WIN - back:wrap * WIN - back + 100] = ph2
    far = _rnd(rng, 60)
    a[WIN - 1500:WIN - 1440] = far
    a[WIN - 1500 + 0x10000:WIN - 1440 + 0x10000] = far
    return Case("ring_wrap", a, None,
                aims=["ring_candidate_straddles_end", "ring_dist_0x10000_across_wrap"], aims_noext=["ring_own_position_straddles_end"],
                aims_ext=[f"ring_candidate_extension_{s}_straddles" for s in (16, 32, 48)] + [f"ring_own_extension_{s}_straddles" for s in (16, 32, 48)])


def dense(seed):
    """stretches where every lane has a word-equal candidate a few bytes back: period 2 and 3 (no match possible: all visited, all
    hazards), tiny alphabets (short matches everywhere)"""
    rng = _rng(seed)
    parts = [_rnd(rng, 30)]
    for p in (1, 2, 3):
        parts += [np.resize(_rnd(rng, p), 700 + p), _rnd(rng, 11)]
    parts += [rng.integers(97, 99, size=3000, dtype=np.uint8), rng.integers(97, 100, size=3000, dtype=np.uint8), _rnd(rng, 200)]
    return Case("dense", np.concatenate(parts), None,
                aims=["hazard_tile", "eight_hazard_tiles_in_a_row", "tile_all_visited", "three_lanes_one_bucket", "offset_3_refused_dist_ok",
                      "offset_wrapped_refused_dist_ok"])


def _soup(rng, n, nwords=3000):
    words = [rng.integers(97, 123, size=int(rng.integers(2, 11)), dtype=np.uint8) for _ in range(nwords)]
    idx = (rng.zipf(1.3, size=n // 4 + 16) - 1) % nwords
    out = np.concatenate([np.append(words[j], 32) for j in idx]).astype(np.uint8)
    assert out.size >= n
    return out[:n]


def tails():
    """every short length, a block one byte short of full and a full one; matches that start 6, 5 and 4 bytes before the end and run
    past it into the look-ahead, over zeros and over a halo that continues them"""
    out = []
    rng = _rng(900)
    for n in list(range(1, 9)) + [63, 64, 65, 127, 128, 129]:
        for kind in ("period3", "random", "soup"):
            d = {"period3": np.resize(np.frombuffer(b"abc", dtype=np.uint8), n), "random": _rnd(rng, n), "soup": _soup(rng, max(n, 64), 12)[:n]}[kind]
            halo = d.tobytes()[:HALO].ljust(8, b"x") if kind != "random" else None
            out.append(Case(f"tail_{kind}_{n}", d, halo, aims=[f"n_{n}"]))
    for back in (6, 5, 4):
        for halo_kind in ("zero", "cont"):
            ph = _rnd(rng, 70); ph[back:] = 0 if halo_kind == "zero" else ph[back:]
            d = np.concatenate([_rnd(rng, 9), ph, _rnd(rng, 40 + back), ph[:back]])
            halo = None if halo_kind == "zero" else ph[back:].tobytes()
            aims = [f"match_start_n_minus_{back}", "match_past_n_zero_halo" if halo_kind == "zero" else "match_past_n_halo_continues"]
            out.append(Case(f"tail_match_n_minus_{back}_{halo_kind}", d, halo, aims=aims))
    # symbol counts: literal-only inputs of 16 s - 15 .. 16 s bytes are s symbols
    for s in (1, 7, 9, 15, 8, 16, 2):
        d = _rnd(rng, 16 * s - int(rng.integers(1, 15)))
        aims = (["final_symbols_odd"] if s & 1 else []) + ([f"final_group_of_{s % 8}"] if s % 8 in (1, 7) else [])
        aims += ["spill_adopted_as_control", "spill_adopted_as_size"] if s % 8 == 0 else (["spill_adopted_as_size"] if s % 2 == 0 else [])
        out.append(Case(f"tail_symbols_{s}", d, _rnd(rng, 64).tobytes(), aims=aims))
    return out


def sweep(seed, k):
    """structured-random family: copies at the distances of the census, lengths 4 .. 70, literal gaps 0 .. 40, seeded"""
    rng = _rng(seed)
    n = int(rng.choice([3000, 40000, 140000, 300000]))
    a = _rnd(rng, n) if k % 2 else _soup(rng, n, 400)
    dists = [d for d in DISTS + (3, 16, 32, 300, 4096, 0xFFFC, 0x10001) if d + 200 < n]
    at = max(dists) + 8
    while at + 200 < n:
        d = int(rng.choice(dists))
        ln = int(rng.integers(4, 71))
        a[at:at + ln] = a[at - d:at - d + ln]
        at += ln + int(rng.integers(0, 41))
    return Case(f"sweep_{k}", a, _rnd(rng, HALO).tobytes() if k % 3 else None)


def full_blocks():
    rng = _rng(4000)
    soup = _soup(rng, BLOCK + 300000, 5000)
    # seams at the block edge: a phrase across it, a copy of the block's first bytes behind it, a far candidate just before it
    soup[BLOCK - 30:BLOCK + 50] = np.resize(np.frombuffer(b"across-the-block-edge/", dtype=np.uint8), 80)
    soup[BLOCK + 100:BLOCK + 180] = soup[0:80]
    full = np.concatenate([_soup(rng, BLOCK - 70000, 800), _rnd(rng, 70000)])
    full[BLOCK - 6:] = full[BLOCK - 6 - 0xFFF0:BLOCK - 0xFFF0]
    short = full[1:].copy()
    return [Case("two_blocks_edge", soup, None, aims=[f"n_{BLOCK}"]),
            Case("full_block", full, full[BLOCK - 0xFFF0:BLOCK - 0xFFF0 + HALO].tobytes(), aims=[f"n_{BLOCK}", "match_past_n_halo_continues"]),
            Case("full_block_less_one", short, None, aims=[f"n_{BLOCK - 1}"])]


_CATALOGUE = None


def catalogue():
    global _CATALOGUE
    if _CATALOGUE is None:
        cases = [near_periods(101), far_phrases(102), origin_shift(103), lengths(104), chains(105), literal_runs(106), hash_twins(107),
                 fold_collisions(108), stale_alias(109), ring_wrap(110), dense(111)]
        cases += tails()
        cases += [sweep(500 + k, k) for k in range(12)]
        cases += full_blocks()
        names = [c.name for c in cases]
        assert len(set(names)) == len(names)
        _CATALOGUE = cases
    return _CATALOGUE


SMALL = 300 * 1024              # cases up to this size are tiled into the jitter batch


def input_digest(case):
    return hashlib.blake2b(case.data + b"|" + (case.halo or b""), digest_size=16).hexdigest()


def case_census(oracle, case, ext):
    """-> (streams of the case's blocks, counters summed over them)"""
    streams, total = [], None
    for data, halo in case.blocks():
        s, c = census(oracle, data, halo, ext)
        streams.append(s)
        total = c if total is None else {k: total[k] + v for k, v in c.items()}
    return streams, total


def kill_matrix(oracle, inputs, mutants=None):
    """inputs: iterable of (name, data, halo).  -> {mutant name: [(input name, ext, decodes back)]}: where the mutant's stream differs
    from the oracle's, and whether the oracle's decoder still gets the input back from it"""
    mutants = list(mutants if mutants is not None else range(1, len(po.MUTANTS)))
    kills = {po.MUTANTS[m]: [] for m in mutants}
    for name, data, halo in inputs:
        data = bytes(data)
        for ext in (0, 1):
            truth = oracle.encode_block(data, ext, halo)
            for m in mutants:
                s, _ = oracle.encode_block_traced(data, ext, halo, mutant=m, trace=False)
                if s != truth:
                    back, st = oracle.decode_block(s, ext)
                    kills[po.MUTANTS[m]].append((name, ext, st == 0 and back == data))
    return kills


# insert_pos0 cannot be told from the truth by any input: the table starts as zeros and position 0's entry is the value 0.
EQUIVALENT_MUTANTS = ("insert_pos0",)


def pins(oracle, reference=None):
    """what tests/golden/encoder_catalogue.json holds: per case and level the input's digest, every block stream's length and digest and
    the census.  With the compiled reference, every stream is first compared with the reference's."""
    import fuzzgen
    out = {}
    for case in catalogue():
        entry = {"input": input_digest(case), "bytes": len(case.data), "levels": {}}
        for ext in (0, 1):
            streams, counters = case_census(oracle, case, ext)
            for (data, halo), s in zip(case.blocks(), streams):
                assert s == oracle.encode_block(data, ext, halo), (case.name, ext, "traced form differs from the plain one")
                if reference is not None:
                    assert s == reference.encode_block(data, ext, halo), (case.name, ext, "oracle differs from the compiled reference")
            entry["levels"][str(ext)] = {"streams": [[len(s), "%016x" % fuzzgen.stream_digest(s)] for s in streams],
                                         "census": {k: v for k, v in counters.items() if v}}
        entry["reference_checked"] = reference is not None
        out[case.name] = entry
    return out
