"""The scan by segments and the super-k-mer count (supersampler_amd/csrc/spsp_stats.hip) on records built to land on their seams.

k_seg_scan gives the whole stream of every -s 1 call, k_seg_count + k_seg_tail give total_superkmer_number; k_stat_count +
k_stat_fix are the chunk form behind them.  All of them cut the concatenated records at fixed places: tiles of 2048
iterations with a halo of 1024 (a chain is followed up to place LIMIT = 3072 of its tile), 7 consecutive places per lane in
the m-mer fill, ballot words of 64, rounds of 512 places in seg_events, chunks of 512 iterations with a lookback of
max(64, 8 w), a slow walk behind the halo that takes 256 iterations at a time from a budget of 512 + n_bases / 20000, and a
ring of the last 64 m-mers.  Random input meets these by luck.  The inputs here are built by tests/runs.py: a reset-free
run (a homopolymer, a tandem repeat of period <= w) fitted to the iteration between random flanks, and a filler record in
front that moves it to the place a case names.

Both forms of the scan, and both of the count, give the same numbers, so every case asserts which one answered as well:
Context.stats_counts() (spsp_stats_counts) against what runs.py derives -- scan_form: 1 by segments, 3 the product scan
after a chain was left over; count_form: 1 by segments, 2 the chunk kernels, 3 after a hand-over; count_chains = the chains
that leave their halos.

Expected values, integers only, no tolerance:
    the super-k-mer stream   orc.scan(k, m, T, bases, offsets), field by field, at T = 2^64 - 1 (-s 1) and at a directly set
                             T = 0xD000000000000000 (0.8125 x 2^64: the scan by segments unhooked, some super-k-mers dropped)
                             and, per case, at the smallest minimizer hash >= 0.8 x 2^64 of its stream (`h > threshold` met with
                             equality).  0xD0.. drops the flanks only at k = m and a run only where drop_unit finds one
    the total                the oracle's total_superkmer_number
    the form                 runs.scan_form / runs.leaving
Every input is under 20 000 bases (the slow-walk budget is exactly 512, two grants of 256) and no reset-free stretch is
longer than 5 000 iterations; Case.claim asserts both, and that the input is what its name says.  The same claims run on the
CPU (test_the_cases_are_what_they_are_called), where runs.count_model must give the oracle's total for every case.

What a wrong kernel would look like, and which case shows it:
    `>=` for `>` in `unknown` (a chain whose record ends on LIMIT handed on), next_reset one short, a reset on place 3071 / 3072
        missed or seen twice, the hand-over word's kind bit: halo_end
    the budget charged at the wrong steps or compared off by one, a chain that ran out reported as ended: walk_budget
    the ring indexed short (& 31), the clamp of the eight-at-a-time read, a rescan behind the halo that differs from the one
        in LDS: ring
    a lane's 7 places rolled across a record boundary, an m-mer or a k-mer of a short record invented, the last tile's halo
        read past the buffer: fill
    seg_events' prefix over waves and rounds off by one, tile_off of the neighbouring tile, s_cnt taken by iteration instead of
        by event, a tile without events: events
    k_seg_tail starting from the wrong state for kind 0 / kind 1, not stopping at the reset, two chains sharing a slot: tail
    a dword's 16 positions read in the wrong order at a record's start: packed
    a stale over_n or slow-walk word, st_count shared between the chunk counts and the tile counts, a stale pinned slot: one_context
    the lookback of k_stat_count / k_stat_fix off by one, a run of open chunks cut short or carried into the next record: chunks
        (SPSP_DEBUG_STATS=chunks and =tiny, the only two hooks this file reads, one subprocess each)"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import runs as rn
import supersampler_amd as sp
from oracle import oracle_py as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = rn.LIMIT                                 # spsp_stats.hip: constexpr uint32_t LIMIT = kSegIter + kSegHalo (k_seg_count, k_seg_scan)
TILE = rn.SEG_ITER                               # kSegIter
SLOW_STEP = rn.SLOW_STEP                         # k_seg_scan: `(steps & 255u) == 0 && atomicAdd(over_n + 1, 256u) + 256u > slow_budget`
SLOW_BUDGET = rn.SLOW_BASE                       # seg_scan_count: slow_budget = 512 + n_bases / 20000, n_bases < 20000
CHUNK = rn.STAT_CHUNK                            # kStatChunk
T_ALL = (1 << 64) - 1                            # spsp_threshold_host for -s 1
T_DROP = 0xD000000000000000                      # 0.8 <= T / 2^64 < 1: by segments without a hook, and it drops

cached = functools.lru_cache(maxsize=None)


@cached
def drop_unit(k, m):
    """a run whose minimizer T_DROP drops: a window's minimum over w random m-mers is almost never above 0.8 x 2^64, so for w > 1
    the only super-k-mers the second threshold can drop are those of a run -- the homopolymer or the short tandem repeat
    chosen here, whose every window has its minimum above T_DROP (the oracle selects nothing of it)"""
    import itertools
    for q in range(1, 6):
        for unit in ("".join(u) for u in itertools.product("ACTG", repeat=q)):
            rec = run_of(unit)(3 * k)
            if len(orc.scan(k, m, T_DROP, rec, np.array([0, len(rec)], np.uint64))[0]) == 0:
                return unit
    return None                                  # (none at m = 11 and m = 15: their runs are homopolymers, and the flanks drop at k = m only)


def run_of(unit):
    if isinstance(unit, str):
        u = np.frombuffer(unit.encode(), np.uint8)
    else:
        u = rn.random_bases(unit, 1000 + unit)   # a tandem repeat of period `unit`
    return lambda L: rn.tandem(u, L)


def stretch(k, m, gap, kind, by, unit=None, seed=5, flank=300):
    """-> (record, e): the record's event at iteration e is a record start (kind 0) or a reset (kind 1), the next reset (by =
    "reset") or the record's end (by = "end") lies `gap` iterations behind it, and nothing lies between"""
    run = run_of((drop_unit(k, m) or "A") if unit is None else unit)
    head = rn.random_bases(flank, seed) if kind == 1 else np.zeros(0, np.uint8)
    tail = lambda v: rn.random_bases(max(150, 2 * k), seed + 1 + 1000 * v) if by == "reset" else np.zeros(0, np.uint8)
    rec = rn.fit_gap(lambda L, v: rn.cat(head, run(L), tail(v)), gap, k, m)
    e, x, got_by = rn.longest_gap(rec, k, m)
    R = rn.record(rec, k, m)
    assert x - e == gap and got_by == by and (e == 0 if kind == 0 else e > 0 and R.reset[e]), (e, x, got_by)
    return rec, e


def layout(items, seed=300):
    """[(record, iteration, g)] -> records with random fillers between them so that `iteration` of each record is global place g"""
    recs, cur = [], 0
    for j, (rec, it, g) in enumerate(items):
        f = g - it - cur
        assert f >= 0, (j, f)
        if f:
            recs.append(rn.filler(f, seed + j))
        recs.append(rec)
        cur = g - it + len(rec)
    return recs


def left_is(want):
    """claim: the chains that leave are exactly these (tile, kind, s, by)"""
    def check(case, k, m):
        got = sorted((e.tile, kind, s, by) for e, kind, s, by in rn.leaving(case.recs, k, m))
        assert got == sorted(want), (case.name, got, want)
    return check


def event_at(g, kind, stop):
    """claim: an event of this kind at global place g whose chain stops at global place `stop`"""
    def check(case, k, m):
        ev = [e for e in rn.events(case.recs, k, m) if e.g == g]
        assert len(ev) == 1 and kind in ev[0].stop and ev[0].stop[kind] == stop, (case.name, g, kind, stop, [(e.g, e.stop) for e in ev])
    return check


def both(*checks):
    def check(case, k, m):
        for c in checks:
            c(case, k, m)
    return check


# ============================================================================================================ cases

def halo_end(k, m):
    """an event at place p of tile 1 -- 0, 2047 and, one filler base more, place 0 of tile 2 -- and its next reset at place 3071,
    3072, 3073 of tile 1; then the record's last iteration there and no reset.  leaving: none for 3071, one for 3072 and 3073
    (s = 0, 1); by the end none for 3071 (end64 == LIMIT), one for 3072, 3073 (s = 1, 2); none after the shift"""
    out = []
    for kind in (0, 1):
        for by in ("reset", "end"):
            for p in (0, 2047):
                for q in (3071, 3072, 3073):
                    stop = q if by == "reset" else q + 1                 # (the tile's place of the reset / one behind the last iteration)
                    rec, e = stretch(k, m, stop - p, kind, by, seed=5 + q + p)
                    for shift in ((0, 1) if p == 2047 else (0,)):
                        g = TILE + p + shift
                        want = [(1, kind, stop - LIMIT, by)] if shift == 0 and stop >= LIMIT and (by == "reset" or stop > LIMIT) else []
                        out.append(rn.Case("k%d_%s_p%d_q%d_shift%d" % (kind, by, p, q, shift), layout([(rec, e, g)]),
                                           both(left_is(want), event_at(g, kind, g + stop - p))))
    return out


WALK_S = (0, 1, 255, 256, 257, 511, 512, 513)


def walk_budget(k, m):
    """one chain that leaves tile 0 and stops s iterations behind LIMIT: form 1 up to s = 511 (steps 0 .. 511: grants at steps 0
    and 256), form 3 from 512 on (the grant at step 512 is the third).  two_*: two chains in two tiles; stopping at 200 each
    takes one grant each (form 1), at 300 each two each (form 3)"""
    out = []
    for by in ("reset", "end"):
        for s in WALK_S:
            if by == "end" and s == 0:
                continue                                                 # (a record that ends on LIMIT does not leave)
            kind = s & 1
            rec, e = stretch(k, m, LIMIT + s - 2000, kind, by, seed=40 + s)
            form = 1 if s < SLOW_BUDGET else 3
            def check(case, k, m, form=form, want=[(0, kind, s, by)]):
                left_is(want)(case, k, m)
                assert rn.scan_form(case.recs, k, m)[0] == form, case.name
            out.append(rn.Case("s%d_%s" % (s, by), layout([(rec, e, 2000)]), check))
    for s, form in ((200, 1), (300, 3)):
        a, ea = stretch(k, m, LIMIT + s - 2000, 1, "reset", seed=61)
        b, eb = stretch(k, m, LIMIT + s - 1900, 0, "end", unit="C", seed=62)
        def check(case, k, m, form=form, want=[(0, 1, s, "reset"), (3, 0, s, "end")]):
            left_is(want)(case, k, m)
            assert rn.scan_form(case.recs, k, m)[0] == form, case.name
        out.append(rn.Case("two_%d" % s, layout([(a, ea, 2000), (b, eb, 3 * TILE + 1900)]), check))
    return out


def ring_units(k, m):
    w = k - m + 1
    return ["A"] + [q for q in (5, 37) if q <= w]


def ring(k, m):
    """a leaving chain in a homopolymer and in tandem repeats of period 5 and 37 (where w allows: a longer period has resets),
    walked 300 iterations behind the halo: the ring of 64 wraps four times, and the model says the chain rescans there"""
    out = []
    for unit in ring_units(k, m):
        for kind, by in ((1, "reset"), (0, "end")):
            s = 300
            rec, e = stretch(k, m, LIMIT + s - 1990, kind, by, unit=unit, seed=70)
            def check(case, k, m, want=[(0, kind, s, by)]):
                left_is(want)(case, k, m)
                (lv,) = rn.leaving(case.recs, k, m)
                assert len(rn.rescans_behind_halo(case.recs, k, m, lv)) >= 3 and s >= 2 * rn.RING, case.name
                assert rn.scan_form(case.recs, k, m)[0] == 1
            out.append(rn.Case("%s_k%d_%s" % (unit, kind, by), layout([(rec, e, 1990)]), check))
    return out


FILL_BOUNDARIES = (6, 7, 8, 63, 64, 65, 2047, 2048, 2049, 3071, 3072)


def fill(k, m):
    """record boundaries in the m-mer fill (a lane's 7 places, a ballot word, the tile, the halo's last places), the record
    lengths 0, m - 1, m, k - 1, k (one k-mer, no iteration), k + 1, empty records in a row and as the last record, and buffers
    of exactly 2048, 2049 and 4096 bases"""
    out = []
    for b in FILL_BOUNDARIES:
        def check(case, k, m, b=b):
            assert b in case.offs.tolist()
        out.append(rn.Case("boundary%d" % b, [rn.random_bases(b, 100 + b), rn.random_bases(700, 200 + b)], check))
    z = np.zeros(0, np.uint8)
    lens = (0, m - 1, m, k - 1, k, k + 1)
    recs = []
    for j, n in enumerate(lens):
        recs += [rn.random_bases(n, 400 + j), rn.random_bases(101, 420 + j)]
    recs += [rn.random_bases(n, 440 + j) for j, n in enumerate(lens)]          # ... and directly behind one another
    def check_lens(case, k, m):
        assert set(lens) <= {len(r) for r in case.recs}
        assert any(rn.record(r, k, m).n_iter == 0 for r in case.recs)
    out.append(rn.Case("lengths", recs, check_lens))
    for b in (7, 64, 2048):
        recs = [rn.random_bases(b, 500 + b), z, z, z, rn.random_bases(300, 510 + b), z]
        def check_empty(case, k, m, b=b):
            assert case.offs.tolist()[1:5] == [b] * 4 and case.offs[-1] == case.offs[-2]
        out.append(rn.Case("empty_at%d" % b, recs, check_empty))
    for n in (2048, 2049, 4096):
        def check_n(case, k, m, n=n):
            assert len(case.bases) == n
        out.append(rn.Case("buffer%d" % n, [rn.random_bases(n, 600 + n)], check_n))
        out.append(rn.Case("buffer%d_two" % n, [rn.random_bases(n - k, 610 + n), rn.random_bases(k, 620 + n)], check_n))
    return out


def short_records(n, k, seed):
    """n bases as records of k - 1 bases (the last one shorter): no k-mer, no event"""
    rng = np.random.default_rng(seed)
    out = []
    while n > 0:
        out.append(rn.pl.LETTERS[rng.integers(0, 4, min(k - 1, n))])
        n -= k - 1
    return out


def events_group(k, m):
    out = []
    # a tile without events under a run: a record start in tile 0 and a run across all of tile 1 (the chain leaves; the scan is form 3)
    rec, e = stretch(k, m, 2 * TILE + 40 - 2000, 0, "reset", seed=81)
    def check_run(case, k, m):
        assert rn.tile_events(case.recs, k, m)[1] == []
        left_is([(0, 0, 2 * TILE + 40 - LIMIT, "reset")])(case, k, m)
    out.append(rn.Case("no_events_under_a_run", layout([(rec, e, 2000)]), check_run))
    # a tile without events between tiles that select: tile 1 holds records without a k-mer; tile 2: one event, a record start at 1500
    one, e1 = stretch(k, m, 700, 0, "reset", seed=82)
    recs = [rn.random_bases(TILE, 83)] + short_records(TILE + 1500, k, 84) + [one, rn.random_bases(900, 85)]
    def check_short(case, k, m):
        te = rn.tile_events(case.recs, k, m)
        assert te[1] == [] and te[2] == [1500] and len(te[0]) > 50 and len(te[3]) > 10, (te[1], te[2])
        left_is([])(case, k, m)
    out.append(rn.Case("no_events_one_event", recs, check_short))
    # every round of 512 places with events in all eight waves
    def check_full(case, k, m):
        te = rn.tile_events(case.recs, k, m)
        for t in (0, 1):
            assert len({p // 64 for p in te[t]}) == 32, t
    out.append(rn.Case("all_waves", [rn.random_bases(3 * TILE, 86)], check_full))
    # events on the last place of a round and the first of the next: two resets in a row, put on places 511 and 512 of tile 1
    rec = rn.random_bases(3000, 87)
    R = rn.record(rec, k, m)
    pair = np.nonzero(R.reset[:-1] & R.reset[1:])[0]
    i = int(pair[pair > 100][0])
    def check_pair(case, k, m):
        te = rn.tile_events(case.recs, k, m)[1]
        assert 511 in te and 512 in te
    out.append(rn.Case("places_511_512", layout([(rec, i, TILE + 511)]), check_pair))
    # an event that is a record start and a reset
    for seed in range(900, 1400):
        rec = rn.random_bases(k + 200, seed)
        if rn.record(rec, k, m).reset[0]:
            break
    else:
        raise AssertionError("no record starts with a reset")
    def check_both(case, k, m):
        ev = [e for e in rn.events(case.recs, k, m) if e.g == TILE - 3]
        assert len(ev) == 1 and ev[0].is_start and ev[0].is_reset
    out.append(rn.Case("start_and_reset", layout([(rec, 0, TILE - 3)]), check_both))
    return out


TAIL_S = (1, 1023, 1024, 1025)


def tail(k, m):
    """chains for k_seg_tail: kind 0 and kind 1, stopping by a reset 1, 1023, 1024, 1025 iterations behind LIMIT and by the
    record's end; two chains in consecutive tiles"""
    out = []
    for kind in (0, 1):
        for s in TAIL_S:
            rec, e = stretch(k, m, LIMIT + s - 2010, kind, "reset", seed=90 + s)
            out.append(rn.Case("k%d_reset_s%d" % (kind, s), layout([(rec, e, 2010)]), left_is([(0, kind, s, "reset")])))
        rec, e = stretch(k, m, LIMIT + 777 - 2010, kind, "end", seed=95)
        out.append(rn.Case("k%d_end" % kind, layout([(rec, e, 2010)]) + [rn.random_bases(200, 96)], left_is([(0, kind, 777, "end")])))
    a, ea = stretch(k, m, LIMIT + 100 - 2000, 1, "reset", seed=97)
    b, eb = stretch(k, m, LIMIT + 50 - 1900, 1, "reset", unit="C", seed=98)
    out.append(rn.Case("consecutive_tiles", layout([(a, ea, 2000), (b, eb, TILE + 1900)]), left_is([(0, 1, 100, "reset"), (1, 1, 50, "reset")])))
    return out


def packed(k, m):
    """a record start on each of the 16 positions of a dword (every scan case of this file runs packed as well)"""
    recs = [rn.random_bases(97, 700 + j) for j in range(40)]
    def check(case, k, m):
        assert set((case.offs[:-1] % np.uint64(16)).tolist()) == set(range(16))
    return [rn.Case("dword_positions", recs, check)]


def chunks(k, m):
    """the chunk form's seams (it answers only under SPSP_DEBUG_STATS): a record start at chunk place 0, 1, 511, 512; the last
    reset in front of a chunk's start at distance lookback - 1, lookback (closed: the lookback holds it) and lookback + 1 (open);
    open runs of 1, 2 and 3 chunks; a run that ends with the record; an open chunk whose chunk in front belongs to an earlier
    record; an open chunk with further records behind it in the same chunk"""
    lb = rn.lookback_of(k, m)
    out = []
    for b in (0, 1, 511, 512):
        def check(case, k, m, b=b):
            assert 2 * CHUNK + b in case.offs.tolist() and rn.open_chunks(case.recs, k, m, lb) == []
        out.append(rn.Case("start_at%d" % b, [rn.random_bases(2 * CHUNK + b, 800 + b), rn.random_bases(1500, 810 + b)], check))
    C0 = 6                                                               # the chunk the cases aim at
    for d, n_open in ((lb - 1, 0), (lb, 0), (lb + 1, 1)):
        rec, e = stretch(k, m, d + 100, 1, "reset", seed=820 + d, flank=1500)
        def check(case, k, m, n_open=n_open):
            assert rn.open_chunks(case.recs, k, m, lb) == [C0][:n_open], (case.name, rn.open_chunks(case.recs, k, m, lb))
        out.append(rn.Case("reset_%d_in_front" % d, layout([(rec, e + d, C0 * CHUNK)]), check))
    for n_run in (1, 2, 3):
        for by in ("reset", "end"):
            rec, e = stretch(k, m, lb + 1 + 100 + CHUNK * (n_run - 1), 1, by, seed=830 + n_run, flank=1500)
            def check(case, k, m, n_run=n_run):
                assert rn.open_runs(case.recs, k, m, lb) == [list(range(C0, C0 + n_run))], (case.name, rn.open_runs(case.recs, k, m, lb))
            out.append(rn.Case("open_run%d_%s" % (n_run, by), layout([(rec, e + lb + 1, C0 * CHUNK)]) + [rn.random_bases(400, 839)], check))
    if lb + 40 < CHUNK:
        a = lb + 40                                                      # the record starts inside chunk C0 - 1: a < 512
        rec, e = stretch(k, m, a + 200, 0, "reset", seed=840)
        def check_a(case, k, m):
            assert rn.open_runs(case.recs, k, m, lb) == [[C0]] and C0 * CHUNK - a in case.offs.tolist()
        out.append(rn.Case("open_behind_an_earlier_record", layout([(rec, 0, C0 * CHUNK - a)]), check_a))
    rec, e = stretch(k, m, lb + 1 + 60, 1, "end", seed=850, flank=1500)
    def check_more(case, k, m):
        assert rn.open_runs(case.recs, k, m, lb) == [[C0]]
        assert sum(C0 * CHUNK < o < (C0 + 1) * CHUNK for o in case.offs.tolist()) >= 3
    out.append(rn.Case("open_then_records", layout([(rec, e + lb + 1, C0 * CHUNK)]) + [rn.random_bases(k + 20, 851 + j) for j in range(4)], check_more))
    return out


BUILDERS = {"halo_end": halo_end, "walk_budget": walk_budget, "ring": ring, "fill": fill, "events": events_group, "tail": tail,
            "packed": packed, "chunks": chunks}
#                  (31,11)  (63,15)  (21,11)  (15,15)  (33,13)  (63,7)
CONFIGS = {"halo_end": [(31, 11), (15, 15), (33, 13)],              # (a chain of 3 000 rescans is one lane's: km = 56 is in ring, tail and chunks)
           "walk_budget": [(31, 11), (33, 13)],
           "ring": [(15, 15), (31, 11), (63, 15), (63, 7)],              # km = 0, 20, 48, 56
           "fill": [(31, 11), (63, 15), (21, 11), (15, 15)],
           "events": [(31, 11), (33, 13), (15, 15)],
           "tail": [(31, 11), (21, 11), (63, 7)],
           "packed": [(31, 11), (63, 15)],
           "chunks": [(31, 11), (15, 15), (63, 7)]}
GROUPS = [(g, km) for g, kms in CONFIGS.items() for km in kms]
GROUP_IDS = ["%s-k%dm%d" % (g, k, m) for g, (k, m) in GROUPS]
HOOKED = [(g, km) for g, km in GROUPS if g not in ("walk_budget", "packed")]       # every group with a count


@cached
def cases(group, km):
    k, m = km
    cs = BUILDERS[group](k, m)
    assert len({c.name for c in cs}) == len(cs)
    return cs


@cached
def oracle(group, km, name, T):
    """the oracle's stream and total of a case, computed once and left unchanged"""
    k, m = km
    c = next(c for c in cases(group, km) if c.name == name)
    want, st = orc.scan(k, m, T, c.bases, c.offs)
    want.setflags(write=False)
    return want, int(st["total_superkmer_number"])


def thresholds(group, km, name):
    """T_ALL, T_DROP and, where the case has one, T_EQ: the smallest hash of a minimizer of its stream that is >= 0.8 x 2^64 --
    the threshold EQUAL to a hash the kernel meets (`h > threshold` keeps it, `>=` would drop it), larger ones dropped"""
    want, _ = oracle(group, km, name, T_ALL)
    h = rn.pl.xxh64(want["minimizer"].astype(np.uint64))
    h = h[h >= np.uint64(0xCCCCCCCCCCCCCCCD)]
    return (T_ALL, T_DROP) + ((int(h.min()),) if h.size else ())


# ============================================================================================================ CPU

@pytest.mark.parametrize("group,km", GROUPS, ids=GROUP_IDS)
def test_the_cases_are_what_they_are_called(group, km):
    k, m = km
    dropped = n_eq = 0
    for c in cases(group, km):
        c.claim(k, m)
        want, total = oracle(group, km, c.name, T_ALL)
        assert rn.count_model(c.recs, k, m) == total, (c.name, rn.count_model(c.recs, k, m), total)
        few, _ = oracle(group, km, c.name, T_DROP)
        assert len(few) <= len(want)
        dropped += len(want) - len(few)
        for T in thresholds(group, km, c.name)[2:]:
            eq, _ = oracle(group, km, c.name, T)
            assert T / 2.0 ** 64 >= 0.8 and (rn.pl.xxh64(eq["minimizer"].astype(np.uint64)) == np.uint64(T)).any()
            n_eq += 1
    if (group in ("halo_end", "walk_budget", "events") and drop_unit(k, m)) or k == m:
        assert dropped > 0 and n_eq > 0                                  # the second threshold really drops (drop_unit), a third is met exactly


def test_the_models_on_plain_records():
    """the reset mask against its definition, the count model against the oracle on random, homopolymer, tandem, short and empty
    records at every configuration, and at most one leaving chain per tile"""
    for k, m in ((31, 11), (63, 15), (21, 11), (15, 15), (63, 7), (33, 13)):
        recs = [rn.random_bases(3000, 1), rn.homopolymer(2500), rn.cat(rn.random_bases(500, 2), rn.tandem(rn.random_bases(5, 3), 3000), rn.random_bases(700, 4)),
                rn.random_bases(k, 5), rn.random_bases(k - 1, 6), np.zeros(0, np.uint8), rn.cat(rn.random_bases(100, 8), rn.tandem(rn.random_bases(37, 9), 4000)),
                rn.random_bases(k + 1, 5)]
        b, o = rn.concat(recs)
        assert rn.count_model(recs, k, m) == orc.scan(k, m, T_ALL, b, o)[1]["total_superkmer_number"]
        assert len(rn.leaving(recs, k, m)) >= 1
        R = rn.record(recs[0], k, m)
        km = k - m
        for i in (0, 1, 17, R.n_iter - 1):
            assert bool(R.reset[i]) == (R.hl[i + km + 1] < min(R.hl[i:i + km + 1]))
        assert not rn.reset_mask(recs[1], k, m).any()                    # a homopolymer has no reset
    assert rn.slow_budget(19_999) == 512 and rn.lookback_of(31, 11) == 168 and rn.lookback_of(15, 15) == 64


# ============================================================================================================ GPU

def _assert_stream_equal(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for f in ("rec", "minimizer", "start", "len", "rev"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (tag, f, int(bad[0]), got[bad[0]], want[bad[0]])


HOOK = os.environ.get("SPSP_DEBUG_STATS", "")[:1]                         # "": none, "c": chunks, "t": tiny


def want_count_form(n_leaving, n_bases, k):
    """count_superkmers_impl: -> (count_form, count_chains)"""
    if n_bases < k:
        return 0, 0
    if HOOK == "c":
        return 2, 0
    return (3 if HOOK == "t" and n_leaving > 1 else 1), n_leaving


def run_scan(ctx, group, km, case, d_b, d_o):
    k, m = km
    n = len(case.bases)
    form, lo, hi = rn.scan_form(case.recs, k, m)
    for T in thresholds(group, km, case.name):
        want, _ = oracle(group, km, case.name, T)
        for pk in ((False, True) if T in (T_ALL, T_DROP) else (False,)):
            tag = (group, km, case.name, hex(T), "packed" if pk else "ascii")
            p = sp.make_params(k, m, 1, flags=sp.SPSP_SCAN_DEFAULT | (sp.SPSP_SCAN_PACKED_INPUT if pk else 0), threshold_value=T)
            ptr = ctx.pack_bases_device(d_b.data_ptr(), n) if pk else d_b.data_ptr()
            d_out, n_out = ctx.scan_device(p, ptr, n, d_o.data_ptr(), len(case.offs) - 1)
            got = ctx.to_host(d_out, n_out, sp.SUPERKMER_DTYPE) if n_out else np.zeros(0, sp.SUPERKMER_DTYPE)
            _assert_stream_equal(got, want, tag)
            st = ctx.stats_counts()
            assert st["scan_form"] == form and lo <= st["scan_left"] <= hi, (tag, st, (form, lo, hi))


def run_count(ctx, group, km, case, d_b, d_o):
    k, m = km
    _, total = oracle(group, km, case.name, T_ALL)
    got = ctx.count_superkmers_device(sp.make_params(k, m, 1), d_b.data_ptr(), len(case.bases), d_o.data_ptr(), len(case.offs) - 1)
    st = ctx.stats_counts()
    assert got == total, (group, km, case.name, got, total, st)
    want = want_count_form(len(rn.leaving(case.recs, k, m)), len(case.bases), k)
    assert (st["count_form"], st["count_chains"]) == want, (group, km, case.name, st, want)


def upload(case):
    import torch
    d_b = torch.from_numpy(np.concatenate([case.bases, np.zeros(64, np.uint8)])).cuda()
    d_o = torch.from_numpy(case.offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    return d_b, d_o


def run_group(ctx, group, km, scan=True, count=True):
    k, m = km
    for c in cases(group, km):
        c.claim(k, m)
        d_b, d_o = upload(c)
        if scan and group != "tail":
            run_scan(ctx, group, km, c, d_b, d_o)
        if count and group != "walk_budget":
            run_count(ctx, group, km, c, d_b, d_o)


@pytest.mark.gpu
@pytest.mark.parametrize("group,km", GROUPS, ids=GROUP_IDS)
def test_segment_seams(group, km):
    """every case of the group on one context: the stream at both thresholds, ASCII and packed, with the form that gave it, then
    the total with the form that gave it (walk_budget: the scan only; tail: the count only)"""
    assert HOOK == ""
    with sp.Context(0) as ctx:
        run_group(ctx, group, km)


def pick(group, km, name):
    return group, km, next(c for c in cases(group, km) if c.name == name)


@pytest.mark.gpu
def test_one_context_over_the_forms():
    """one context takes a count with a leaving chain, a scan of form 3, a scan of form 1 on a smaller input, a count without
    leaving chains and a larger scan: a stale over_n or budget word, st_count as chunk counts after tile counts, or a stale
    pinned slot of an earlier call would show in a total, a stream or in stats_counts()"""
    km = (31, 11)
    plan = [("count", pick("tail", km, "k1_reset_s1025")), ("scan", pick("walk_budget", km, "s513_reset")), ("scan", pick("fill", km, "boundary64")),
            ("count", pick("fill", km, "lengths")), ("scan", pick("events", km, "all_waves")), ("count", pick("tail", km, "consecutive_tiles")),
            ("scan", pick("walk_budget", km, "two_300")), ("scan", pick("walk_budget", km, "s511_end")), ("count", pick("packed", km, "dword_positions"))]
    forms = [rn.scan_form(c.recs, *km)[0] for what, (_, _, c) in plan if what == "scan"]
    assert forms == [3, 1, 1, 3, 1] and len(pick("fill", km, "boundary64")[2].bases) < len(pick("walk_budget", km, "s513_reset")[2].bases)
    with sp.Context(0) as ctx:
        assert ctx.stats_counts() == dict(scan_form=0, scan_left=0, count_form=0, count_chains=0)
        for what, (group, km_, c) in plan:
            d_b, d_o = upload(c)
            before = ctx.stats_counts()
            (run_scan if what == "scan" else run_count)(ctx, group, km_, c, d_b, d_o)
            after = ctx.stats_counts()
            if what == "scan":                                           # a scan leaves the count's words alone, and the other way round
                assert (after["count_form"], after["count_chains"]) == (before["count_form"], before["count_chains"])
            else:
                assert (after["scan_form"], after["scan_left"]) == (before["scan_form"], before["scan_left"])
        # an empty call and a threshold under 0.8 x 2^64: forms 0 and 2
        c = pick("fill", km, "boundary64")[2]
        d_b, d_o = upload(c)
        p = sp.make_params(31, 11, 1)
        assert ctx.scan_device(p, d_b.data_ptr(), 10, d_o.data_ptr(), 0)[1] == 0 and ctx.stats_counts()["scan_form"] == 0
        p = sp.make_params(31, 11, 50)
        d_out, n_out = ctx.scan_device(p, d_b.data_ptr(), len(c.bases), d_o.data_ptr(), len(c.offs) - 1)
        want, _ = orc.scan(31, 11, p.threshold, c.bases, c.offs)
        _assert_stream_equal(ctx.to_host(d_out, n_out, sp.SUPERKMER_DTYPE) if n_out else np.zeros(0, sp.SUPERKMER_DTYPE), want, "s50")
        assert ctx.stats_counts()["scan_form"] == 2 and ctx.stats_counts()["scan_left"] == 0


def fasta(recs, first=0):
    return b"".join(b">r%d\n" % (first + j) + bytes(r) + b"\n" for j, r in enumerate(recs))


INGEST = [("halo_end", (31, 11), "k1_reset_p2047_q3072_shift0"), ("halo_end", (31, 11), "k0_end_p0_q3073_shift0"), ("fill", (31, 11), "lengths"),
          ("fill", (63, 15), "boundary2048"), ("tail", (31, 11), "consecutive_tiles"), ("tail", (63, 7), "k0_reset_s1024")]
STAT_FIELDS = ("selected_kmer_number", "read_kmer", "nb_mmer_selected", "total_superkmer_number")


@pytest.mark.gpu
def test_the_records_through_ingest():
    """the records as FASTA text, one line each, through sketch_text with SPSP_SCAN_STATS at -s 1: the payload and the totals
    are the oracle's, and the count behind the ingest was the one by segments"""
    with sp.Context(0) as ctx:
        for group, km, name in INGEST:
            k, m = km
            c = pick(group, km, name)[2]
            text = fasta(c.recs)
            got, gst = ctx.sketch_text(text, k, m, 1, flags=sp.SPSP_SCAN_STATS)
            want, wst = orc.sketch_fasta(text, k, m, 1)
            assert got == want, (group, km, name)
            for f in STAT_FIELDS:
                assert gst[f] == wst[f], (group, km, name, f, gst[f], wst[f])
            assert ctx.stats_counts()["count_form"] == 1, (group, km, name)


@pytest.mark.gpu
def test_the_records_through_the_file_pipeline(tmp_path):
    """the same records split over several files through the batched file pipeline with SPSP_SCAN_STATS: a batch's files are
    counted by ONE launch (file_rec), so a file's total is right only if every event and every chain handed to k_seg_tail is
    booked to the file of its record.  The files end on a tile boundary (2048 bases), between two events of one wave (a random
    record cut 10 bases further) and right behind a leaving chain (the record that holds it is a file's last)"""
    k, m = 31, 11
    a = pick("tail", (k, m), "consecutive_tiles")[2].recs
    b = pick("halo_end", (k, m), "k1_reset_p2047_q3073_shift0")[2].recs
    r = rn.random_bases(5000, 990)
    files = [[r[:2048]], [r[2048:2058 + 700], r[2758:]], a[:2], a[2:], b, [rn.random_bases(900, 991)], pick("fill", (k, m), "lengths")[2].recs]
    assert len(rn.leaving(a[:2], k, m)) == 1 and rn.leaving(a[:2], k, m)[0][0].r == 1      # the file's last record leaves its halo
    ins, texts = [], []
    for i, recs in enumerate(files):
        path = tmp_path / ("f%d.fa" % i)
        texts.append(fasta(recs, 10 * i))
        path.write_bytes(texts[-1])
        ins.append(str(path))
    want = [orc.sketch_fasta(t, k, m, 1) for t in texts]
    for threads in (1, 3):
        outs = [str(tmp_path / ("o%d_%d.gz" % (threads, i))) for i in range(len(ins))]
        res, _, _ = sp.sketch_files(ins, outs, k, m, 1, threads=threads, flags=sp.SPSP_SCAN_STATS)
        for i, (rc, st, err) in enumerate(res):
            assert rc == 0 and sp.read_file(outs[i]) == want[i][0], (threads, i, rc, err)
            for f in STAT_FIELDS:
                assert st[f] == want[i][1][f], (threads, i, f, st[f], want[i][1][f])


def run_counts_under_hook():
    """(a process of its own, SPSP_DEBUG_STATS set) every count case of this file: totals exact, the form the hook asks for.  (The
    chunk kernels replay a run base by base from global memory: most of this test's seconds are theirs.)"""
    assert HOOK in ("c", "t")
    n_handed = 0
    with sp.Context(0) as ctx:
        for group, km in HOOKED:
            run_group(ctx, group, km, scan=False)
            n_handed += sum(len(rn.leaving(c.recs, *km)) > 1 for c in cases(group, km))
    assert n_handed >= 2
    print("ok")


@pytest.mark.gpu
@pytest.mark.parametrize("hook", ["chunks", "tiny"])
def test_the_chunk_form(hook):
    """k_stat_count + k_stat_fix answer only when more chains leave their halos than k_seg_tail has lanes (16 384), which no small
    input reaches: SPSP_DEBUG_STATS=chunks takes them from the start (count_form 2), =tiny gives the tail kernel one lane, so a
    call with two leaving chains is handed over (count_form 3) and every other one stays (1)"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\nimport test_segment_seams as t\nt.run_counts_under_hook()\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, SPSP_DEBUG_STATS=hook), timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (hook, r.stdout[-500:], r.stderr[-3000:])
