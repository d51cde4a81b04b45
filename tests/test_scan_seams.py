"""The scan's passes (supersampler_amd/csrc/spsp_scan.hip) on planted hits at their seams.

A hit is an m-mer whose XXH64 (seed 1312) of the canonical value is <= T.  Random sequence meets the kernels' fixed
boundaries by luck, and at the default sampling (k31 m11 s1000: 89 canonical 11-mers, 4.8e-5 of the positions) almost never.
The inputs below are built by tests/planted.py: a background without a single hit, and pool m-mers written exactly where a
boundary is -- the 16 offsets of a lane's chunk, the ends of a 1008-position wave-row, of a wave's rows, of a workgroup, of a
16 384-position tile and of the buffer, the queue and list capacities, the resolve pass's workgroups and its write offsets.

Every input under 4 128 768 bases gives a wave ONE row on a default context (one workgroup for each of 256 CUs), so the
loops that keep two or four rows in flight, the two-row queueing and a list that grows across rows never ran on small
inputs.  Each test therefore takes a context of its own with set_cu_count(g, 1), g in {1, 2, 5}: geometry(n, g) below is
plan_lists, and rows_per_wave is 1..9 on inputs of at most 330 000 bases.

Expected values, integers only, no tolerance:
    the super-k-mer stream   orc.scan(k, m, T, bases, offsets), field by field
    the hit count            planted.hit_mask(bases, m, T).sum() against scan_hits_device: all n - m + 1 positions, records
                             ignored -- a dense pass that loses or invents a hit the sparse pass would hide (an unusable
                             position, an m-mer across a record boundary, a record shorter than k) shows here
Before a case runs on the GPU, Case.claim asserts from the mask (and the survivor models) that the input is what its name
says: the hit set equals the planned positions, or a run holds the hits its case needs.  The same claims run on the CPU
(test_the_cases_are_what_they_are_called), so a case cannot drift off its seam unnoticed.

The dense forms are forced by flags (pick_dense): DIRECT_HASH, PAIR_FILTER (m = 9: the table whose second bit stands for the
position behind; m >= 10: MID, the position in front), LDS_FILTER (10-base prefix table), BLOOM_FILTER (m = 13, 15).  The pair
and Bloom forms also read 2-bit input (SPSP_SCAN_PACKED_INPUT, pack_bases_device) and must give the same stream and count.

What a wrong kernel would look like, and which case shows it:
    a survivor bit decoded to the wrong offset, the ninth lookup (PairSurv::x) or an odd offset lost, pair 0's second bit
        of the MID table not masked (the hit at offset 15 of the lane in front counted twice): chunk_offsets
    lane 63 counted as a lane of the row, a halo taken from the wrong row, a row's last m - 1 positions lost: row_ends
    a row of the 2-in-flight / 4-in-flight loops skipped, read twice or given the wrong `rel`, leftover rows dropped, a
        wave without rows reporting a stale count: rows_per_wave
    `pos <= n_mmers`, a zero-padded tail completed into a hit, full_rows / full_p off by one: buffer_lengths
    a queue that drops, repeats or reorders survivors at 64, 128 or the ring's 192 slots: queues
    a list overflow that leaves a stale capacity or table behind: overflow
    a tile's halo, the 64-hit rounds of k_expand, a ragged dword of mmer_at, the grid-stride loop: direct
    `h.pos + m < r1`, a record searched in the wrong range of k_compact, a short or empty record: records
    a staged window of k_resolve read past its end, a cut head missed beyond it, wave and chunk sums of the write pass
        off by one: sparse
    a cached table or a learned capacity of an earlier call used by this one: test_one_context_over_many_calls

The scan by segments (spsp_stats.hip: k_seg_scan, and the super-k-mer count beside it) has its seams in
tests/test_segment_seams.py; no test of this file reads an environment hook."""
import functools

import numpy as np
import pytest

import planted as pl
import supersampler_amd as sp
from oracle import oracle_py as orc

R = 1008                                         # positions of a wave-row (kRowPosPair63)
WAVES = 16                                       # waves of a dense workgroup (kPairWaves)
TILE = 16384                                     # positions of a tile of the direct form (kTilePos)
QUEUE = 64                                       # kQueueCap
PUSH_WINDOW, RING = 128, 192                     # kPushWindow, kQueueCap1
RESOLVE = 128                                    # kResolveThreads
STAGED_AFTER = 120                               # kResolveAfter
COMPACT_LISTS = 64                               # kCompactWaves
LIST_SLACK = 48                                  # plan_lists: cap = 1.5 x expected + 48

#        name        k   m   s     flag
FORMS = {
    "pair_mid": (31, 11, 1000, sp.SPSP_SCAN_PAIR_FILTER),
    "single":   (31, 11, 1000, sp.SPSP_SCAN_LDS_FILTER),
    "pair_k8":  (21, 9, 300, sp.SPSP_SCAN_PAIR_FILTER),
    "bloom13":  (33, 13, 50, sp.SPSP_SCAN_BLOOM_FILTER),
    "bloom15":  (63, 15, 100, sp.SPSP_SCAN_BLOOM_FILTER),
    "direct":   (31, 11, 1000, sp.SPSP_SCAN_DIRECT_HASH),
    "direct9":  (21, 9, 30, sp.SPSP_SCAN_DIRECT_HASH),
    # a second threshold for the forms of m = 11 (overflow, one context over many calls)
    "pair_mid_s300": (31, 11, 300, sp.SPSP_SCAN_PAIR_FILTER),
    "single_s300":   (31, 11, 300, sp.SPSP_SCAN_LDS_FILTER),
}
LIST_FORMS = ["pair_mid", "single", "pair_k8", "bloom13", "bloom15"]
DIRECT_FORMS = ["direct", "direct9"]
PACKED_FORMS = {"pair_mid", "pair_k8", "bloom13", "bloom15", "pair_mid_s300"}
OTHER_THRESHOLD = {"pair_mid": "pair_k8", "pair_k8": "pair_mid", "single": "single_s300", "bloom13": "bloom15", "bloom15": "bloom13"}

cached = functools.lru_cache(maxsize=None)


@cached
def threshold(form):
    k, m, s, _ = FORMS[form]
    return orc.threshold(k, m, s)


def kmT(form):
    k, m, _, _ = FORMS[form]
    return k, m, threshold(form)


def geometry(n, g):
    """plan_lists on a context with set_cu_count(g, 1) -> (n_rows, grid, rows_per_wave)"""
    n_rows = (n + R - 1) // R
    grid = min((n_rows + WAVES - 1) // WAVES, g)
    rpw = (n_rows + WAVES * grid - 1) // (WAVES * grid)
    return n_rows, grid, rpw


def first_call_retries(form, g, mask, n):
    """what scan_begin_impl / plan_lists give a FRESH context for this input, against the hits it has: "lists" if a wave
    finds more hits than its slice of 1.5 x expected + 48 holds (the dense pass is repeated with grown lists), "hits" if
    the input has more hits than the initial hits_cap of 4096 + 1.25 x expected (k_compact or k_expand and the resolve
    passes are repeated).  A context that has retried keeps what it learned -- the list capacity, hits per base -- so this
    holds for the first call only: the runner gives every case that retries contexts of its own"""
    k, m, T = kmT(form)
    if n < k:
        return frozenset()
    frac = T / 2.0 ** 64
    out = set()
    if form not in DIRECT_FORMS:
        rpw = geometry(n, g)[2]
        cap = min(int(rpw * R * frac * 1.5) + LIST_SLACK, rpw * R)
        per_wave = np.bincount(np.nonzero(mask)[0] // (rpw * R)) if mask.any() else np.zeros(1, np.int64)
        if int(per_wave.max()) > cap:
            out.add("lists")
    if int(mask.sum()) > min(int(n * frac * 1.25) + 4096, n):
        out.add("hits")
    return frozenset(out)


class Case:
    """one input: bases, record offsets, the context's g, and what the input claims to be"""

    def __init__(self, name, g, bases, hits=None, offs=None, check=None, rpw=None, retries=()):
        self.name, self.g = name, g
        self.retries = frozenset(retries)        # what the first call of a fresh context has to repeat: "lists", "hits"
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.offs = np.array([0, len(self.bases)], np.uint64) if offs is None else np.asarray(offs, dtype=np.uint64)
        self.hits = None if hits is None else np.array(sorted(int(p) for p in hits), dtype=np.int64)
        self.check = check
        self.rpw = rpw

    def claim(self, form):
        """-> the hit mask, after asserting that the input is what it was built to be"""
        _, m, T = kmT(form)
        mask = pl.hit_mask(self.bases, m, T)
        if self.hits is not None:
            got = np.nonzero(mask)[0]
            assert np.array_equal(got, self.hits), (self.name, got.tolist()[:20], self.hits.tolist()[:20])
        if self.rpw is not None:
            assert geometry(len(self.bases), self.g)[2] == self.rpw, (self.name, geometry(len(self.bases), self.g))
        if self.check is not None:
            self.check(mask)
        assert first_call_retries(form, self.g, mask, len(self.bases)) == self.retries, (self.name, first_call_retries(form, self.g, mask, len(self.bases)))
        assert int(self.offs[0]) == 0 and int(self.offs[-1]) == len(self.bases) and (np.diff(self.offs.astype(np.int64)) >= 0).all()
        return mask


@cached
def _background(form, n, seed):
    _, m, T = kmT(form)
    b = pl.background(n, m, T, seed)
    b.setflags(write=False)
    return b


def bg(form, n, seed=1):
    return _background(form, n, seed).copy()


def planted_case(form, name, g, n, positions, seed=1, first=0, choose=None, min_gap=None, **kw):
    _, m, T = kmT(form)
    b = bg(form, n, seed)
    pl.plant(b, positions, m, T, first=first, choose=choose, min_gap=min_gap)
    return Case(name, g, b, hits=positions, **kw)


def baited(form, n, head):
    """a background of n bases that ends with `head` and still has no hit (the bases in front of the head are drawn again
    until the m-mers across the junction are none)"""
    _, m, T = kmT(form)
    for seed in range(3, 40):
        b = pl.with_tail(bg(form, n, seed=seed), head)
        if not pl.hit_mask(b, m, T).any():
            return b
    raise AssertionError("no background takes the bait's head")


def head_j(head, m, j):
    """the bait's head for j zero bases: the pool m-mer's first m - j bases (its last bases are A)"""
    full = np.concatenate([head, np.full(m - len(head), pl.LETTERS[0], np.uint8)])
    assert 1 <= j <= m - len(head)
    return full[:m - j]


def put(b, at, run):
    assert 0 <= at and at + len(run) <= len(b), (at, len(run), len(b))
    b[at:at + len(run)] = run


# ================================================================================================ the list forms

def chunk_offsets(form):
    """rows_per_wave = 2 (lane0_lane62: 3) on one workgroup.  lanes: offset i in lane 4i of one row (one survivor per lane).
    lane0_lane62: offset i in lane 0 of row i + 1 and in lane 62 of row i + 20; from offset 16 - m + 1 on, lane 62's m-mer
    ends in lane 63, the next row.  offset15: hits that start with A at offset 15 of lanes 0, 3, 31, 58, 62 -- the MID table's ninth lookup, and the
    lane behind each sees the same m-mer as pair 0's second bit: unmasked, it decodes to A + the first m - 1 bases at the
    same position, a second hit.  offset15_in_adjacent_lanes: the lane behind holds a hit at its own offset 15 as
    well, so it has two survivor bits if pair 0's second bit is not masked, and takes the general path (push_row).  No pool
    m-mer overlaps another by m - 1 bases at this threshold (test_what_the_replaced_seams_rest_on), so "a hit at offset 0 behind a hit at offset 15" cannot be
    planted; these hits lie 16 apart, closer than 2m: the writes do not overlap, and plant() still takes the mask over
    every position a write touches"""
    n = 2 * WAVES * R
    out = [planted_case(form, "lanes", 1, n, [3 * R + 65 * i for i in range(16)], rpw=2),
           planted_case(form, "lane0_lane62", 1, 3 * WAVES * R,
                        [(i + 1) * R + i for i in range(16)] + [(i + 20) * R + 62 * 16 + i for i in range(16)], first=3, rpw=3),
           planted_case(form, "offset15", 1, n, [5 * R + 16 * lane + 15 for lane in (0, 3, 31, 58, 62)],
                        choose=lambda row: row[0] == pl.LETTERS[0], rpw=2),
           planted_case(form, "offset15_in_adjacent_lanes", 1, n, [5 * R + 16 * lane + 15 for lane in (10, 11, 40, 41, 42)],
                        first=5, min_gap=16, rpw=2)]
    return out


ROW_END_OFFSETS = [0, 15, 16] + list(range(R - 16, R))


def row_ends(form):
    """g = 2, rows_per_wave = 3, 96 rows.  One buffer per offset o (they lie closer than 2m): p = row * R + o on row 15 (the
    first row of wave 5), row 23 (the last row of wave 7: from o = R - m + 1 on the m-mer spans two waves' rows), row 47
    (the last row of workgroup 0), rows 94 and 95 (the last rows of the buffer, where the m-mer still fits)"""
    _, m, _ = kmT(form)
    n = 96 * R
    out = []
    for o in ROW_END_OFFSETS:
        pos = [r * R + o for r in (15, 23, 47, 94, 95) if r * R + o + m <= n]
        assert len(pos) >= 4
        out.append(planted_case(form, "o%d" % o, 2, n, pos, first=o, rpw=3))
    return out


def rows_per_wave(form):
    """n_rows = 16 q on one workgroup, q = rows_per_wave in {1, 2, 3, 4, 5, 8, 9}: a hit in every row of wave 3, one in the
    last row of wave 2 whose m-mer ends in wave 3's first row, one in wave 4's first row.  ragged45 / ragged29: n_rows = 16 q
    - 3 -- the last waves own fewer rows or none"""
    out = []
    for q in (1, 2, 3, 4, 5, 8, 9):
        n = WAVES * q * R
        pos = [(3 * q + j) * R + 100 + (37 * 16 * j + j) % 800 for j in range(q)]
        pos += [3 * q * R - 3, 4 * q * R + 40]
        out.append(planted_case(form, "q%d" % q, 1, n, pos, first=q, rpw=q))
    for q, rows in ((3, 45), (2, 29)):
        n = rows * R - 100
        pos = [(rows - 1) * R + 300, (rows - 2) * R + R - 2, (rows - 3) * R + 17, 5 * R + 5]
        out.append(planted_case(form, "ragged%d" % rows, 1, n, pos, first=rows, rpw=q))
    return out


LENGTHS = [1007, 1008, 1009, 1023, 1024, 1025, 2000, 2001, 2015]       # full_rows turns 1 at 64 * 16; n mod 16 = 0, 1, 15


def buffer_lengths(form):
    """n in {m - 1, m, 1007 .. 1025, 2000, 2001, 2015} and two lengths past 32 rows.  last_*: a hit on the last m-mer, n - m.
    bait<j>_*: the buffer ends with the first m - j bases of a pool m-mer that ends with j A's -- zero padding would complete
    it into a hit at n - m + j.  j = 1 is the position n - m + 1 = n_mmers itself, which `pos <= n_mmers` lets through; the
    largest j the pool has reaches furthest behind the buffer"""
    _, m, T = kmT(form)
    j, head = pl.bait(m, T)
    heads = (("bait1", head_j(head, m, 1)), ("bait%d" % j, head))         # one zero base completes the first, j the second
    out = [Case("empty_m-1", 1, bg(form, m - 1), hits=[]),
           Case("bait1_m-1", 1, head_j(head, m, 1), hits=[]),
           Case("bait%d_m-1" % j, 1, np.concatenate([bg(form, m - 1)[:m - 1 - len(head)], head]), hits=[]),
           planted_case(form, "last_m", 1, m, [0]),
           Case("bait1_m", 1, baited(form, m, head_j(head, m, 1)), hits=[]),
           Case("bait%d_m" % j, 1, baited(form, m, head), hits=[])]
    for n in LENGTHS + [2 * WAVES * R + 1, 2 * WAVES * R + 15]:
        pos = [n // 3, n - m] if n < 10000 else [n // 3, R + 3, (2 * WAVES - 1) * R - 1, n - m]
        out.append(planted_case(form, "last_%d" % n, 1, n, pos, first=n))
        for name, h in heads:
            b = baited(form, n, h)
            pl.plant(b, [n // 3], m, T, first=n)
            out.append(Case("%s_%d" % (name, n), 1, b, hits=[n // 3]))
    return out


def row_counts(mask, row):
    return int(np.count_nonzero(mask[row * R:(row + 1) * R]))


def queues(form):
    """rows_per_wave = 4 on one workgroup; wave 2 owns rows 8..11.  The cases whose first attempt fits come first, on one
    context; `tandem` (and `dense` on the Bloom form, whose survivors are hits) overflow a list and run on contexts of their own.
    tandem: a run of one hit m-mer with period m from row 8 through row 10 -- lanes with two survivors (push_row), more
        than 64 survivors to a row, the ring of the single and Bloom forms wrapping at 192; an isolated hit behind it in the
        same wave, and the wave's list overflowing its 48 slots (the host grows the lists and repeats)
    near_then_hits (m = 11): a run of a near-hit -- survivors, no hits -- through rows 8..10, isolated hits right behind
        it in rows 10, 11, 12: the order of the wave's list
    dense: more than 128 survivors to a row, from a sequence of period 5..7 -- kPushWindow (single: 10-base prefixes that
        are table keys; Bloom, m = 13: hits; pair: more than 64, drained 64 at a time on the spot)
    A near-hit shares a prefix with a hit, which only the prefix tables test: the pair form of m = 9 (whose table tests the
    whole m-mer at even positions) and the Bloom forms (the canonical m-mer) get their survivors from hits alone.  No
    sequence of period <= 7 is a hit at (63, 15, 100) -- test_what_the_replaced_seams_rest_on tries them all -- so the Bloom form of m = 15 meets
    kPushWindow only through its ring: 67 hits to a row, more than 192 to the wave"""
    _, m, T = kmT(form)
    n = WAVES * 4 * R
    out = []
    row = pl.tandem_row(m, T)
    b = bg(form, n)
    copies = (2 * R + 900) // m
    put(b, 8 * R + 100, pl.tandem(row, copies))
    pl.plant(b, [11 * R + 900, 12 * R + 7], m, T)

    def tandem_claim(mask, copies=copies):
        assert int(mask.sum()) == copies + 2
        assert row_counts(mask, 9) > QUEUE and row_counts(mask, 9) >= R // m
        assert int(mask[8 * R:12 * R].sum()) > LIST_SLACK + 1 and int(mask[8 * R:12 * R].sum()) > RING
    tandem_case = Case("tandem", 1, b, check=tandem_claim, rpw=4, retries=["lists"])

    if m == 11:
        model = pl.survivors_pair_mid if form == "pair_mid" else pl.survivors_single
        x = pl.near_hit(m, T)
        b = bg(form, n)
        put(b, 8 * R + 64, pl.tandem(x, (2 * R + 300) // m))
        iso = [10 * R + 500, 10 * R + 600, 11 * R + 5, 11 * R + 1000, 12 * R + 500]
        pl.plant(b, iso, m, T)

        def near_claim(mask, b=b):
            surv = model(b, m, T)
            assert row_counts(surv, 8) > QUEUE and int(surv[8 * R:11 * R].sum()) > RING
        out.append(Case("near_then_hits", 1, b, hits=iso, check=near_claim, rpw=4))

    if form in ("pair_mid", "single", "bloom13"):
        if form == "bloom13":
            model = lambda x, m, T: pl.hit_mask(np.concatenate([x, x[:m]]), m, T)[:len(x)]       # hits are survivors
        elif form == "pair_mid":
            model = pl.survivors_pair_mid
        else:
            model = pl.survivors_single
        u = None
        for period in (5, 6, 7):
            u = pl.periodic(m, T, period, lambda x: model(x, m, T)[m:m + period].any())
            if u is not None:
                break
        assert u is not None, "no sequence of period <= 7 passes the %s filter" % form
        b = bg(form, n)
        put(b, 8 * R + 32, np.tile(u, 2 * R // len(u)))
        pl.plant(b, [11 * R + 300], m, T)
        need = PUSH_WINDOW if form != "pair_mid" else QUEUE

        def dense_claim(mask, b=b, model=model, need=need):
            surv = model(b, m, T) if form != "bloom13" else mask
            assert row_counts(surv, 9) > need, (row_counts(surv, 9), need)
            assert mask[11 * R + 300]
        out.append(Case("dense", 1, b, check=dense_claim, rpw=4, retries=["lists"] if form == "bloom13" else []))
    out.append(tandem_case)
    return out


def survivor_sums():
    """pair form, m = 11: survivors of rows 8 and 9 of wave 2 (one handle() call: rows 8 and 9 are its first pair), counted by
    the 9-base-prefix model on a background without survivors.  40 + 24 = 64: exactly a queue-full, one survivor per lane.
    63 + 2: one more than fits.  64 + 1: a run of 64 near-hits with period m (lanes holding two)"""
    form = "pair_mid"
    _, m, T = kmT(form)
    n = WAVES * 4 * R
    x = pl.near_hit(m, T)
    clean = pl.background(n, m, T, 11, also=lambda b: pl.survivors_pair_mid(b, m, T))
    out = []
    for name, a, c in (("40+24", 40, 24), ("63+2", 63, 2), ("64+1", 64, 1)):
        for off in (3, 1, 5, 2, 4, 0):
            b = clean.copy()
            if a == 64:
                put(b, 8 * R + off, pl.tandem(x, 64))
            else:
                for lane in range(a):
                    put(b, 8 * R + 16 * lane + off, x)
            for lane in range(c):
                put(b, 9 * R + 16 * (2 * lane + 1) + off, x)
            surv = pl.survivors_pair_mid(b, m, T)
            if row_counts(surv, 8) == a and row_counts(surv, 9) == c and not pl.hit_mask(b, m, T).any():
                break
        else:
            raise AssertionError("survivor_sums: %s not reached" % name)

        def claim(mask, b=b, a=a, c=c):
            surv = pl.survivors_pair_mid(b, m, T)
            assert (row_counts(surv, 8), row_counts(surv, 9)) == (a, c)
            assert int(surv[8 * R:12 * R].sum()) == a + c
        out.append(Case(name, 1, b, hits=[], check=claim, rpw=4))
    return out


def overflow_run(form):
    """a tandem run through rows 8..10 of wave 2 (rows_per_wave = 4): more hits than the wave's 48 slots"""
    _, m, T = kmT(form)
    n = WAVES * 4 * R
    b = bg(form, n, seed=5)
    copies = (2 * R + 300) // m
    put(b, 8 * R + 500, pl.tandem(pl.tandem_row(m, T, skip=3), copies))

    def claim(mask):
        assert int(mask.sum()) == copies and copies > 3 * LIST_SLACK
    return Case("overflow_run", 1, b, check=claim, rpw=4, retries=["lists"])


# ================================================================================================ the direct form

def direct(form):
    """k_dense_direct and k_expand.  tile_ends_a/b: hits at positions {0, 31, 127, 8191, 16383} and {32, 128, 8192} of tile 1
    (the last one's m-mer crosses the tile's end).  counts: 64, 65, 128 and 129 hits in tiles 0..3 (k_expand's rounds of 64).
    mod4 / ragged_*: hit positions with pos & 3 = 0..3, n in {16384, 32768, 16385, 16387} with a hit at n - m (mmer_at's
    ragged dword) or the bait.  stride: 17 tiles on one CU, 16 workgroups: the grid-stride loop"""
    _, m, T = kmT(form)
    j, head = pl.bait(m, T)
    out = [planted_case(form, "tile_ends_a", 1, 3 * TILE, [TILE + t for t in (0, 31, 127, 8191, 16383)]),
           planted_case(form, "tile_ends_b", 1, 3 * TILE, [TILE + t for t in (32, 128, 8192)], first=1)]
    pos = []
    for tile, cnt in enumerate((64, 65, 128, 129)):
        pos += [tile * TILE + 33 + 121 * i for i in range(cnt)]
    out.append(planted_case(form, "counts", 1, 4 * TILE + 100, pos, first=5))
    out.append(planted_case(form, "mod4", 1, 2000, [400, 501, 602, 703], first=9))
    for n in (16384, 32768, 16385, 16387):
        out.append(planted_case(form, "ragged_%d" % n, 1, n, [n // 2 + 1, n - 4 * m, n - m], first=n))
        for name, h in (("bait1", head_j(head, m, 1)), ("bait%d" % j, head)):
            b = baited(form, n, h)
            pl.plant(b, [n - 5 * m], m, T, first=n)
            out.append(Case("%s_%d" % (name, n), 1, b, hits=[n - 5 * m]))
    out.append(planted_case(form, "stride", 1, 17 * TILE, [5, 15 * TILE + 77, 16 * TILE - 3, 16 * TILE + 2 * m + 5, 16 * TILE + 9001, 17 * TILE - m],
                            first=2))
    return out


# ======================================================================================================= records

def records(form):
    """record offsets against planted hits, through k_compact (list forms) and k_expand (direct form).
    straddle: a hit whose m-mer crosses a record boundary; short: a hit inside a record shorter than k; empty: three
    records of no bases at a hit's position; span: boundaries exactly on wave-span boundaries w * S, with a hit ending at,
    starting at, or crossing each; r150: 150-base records, several to a row; tile_starts: 0, 1, 2 and 4 record starts inside
    the tiles 0..3 of 16 384 positions"""
    k, m, T = kmT(form)
    n = WAVES * 2 * R
    S = 2 * R
    out = []
    pos = [3000, 5000, 7000, 9000 - m, 9000 + 2 * m]
    c = planted_case(form, "straddle", 1, n, pos, rpw=2)
    c.offs = np.array([0, 3000 + 5, 5000 + m - 1, 7000 + 1, 9000, n], np.uint64)
    out.append(c)
    c = planted_case(form, "short", 1, n, [4000, 6000, 8000], first=1, rpw=2)
    c.offs = np.array([0, 4000 - 3, 4000 + m + 3, 6000, 6000 + k - 1, 8000 - 1, 8000 - 1 + k, n], np.uint64)
    out.append(c)
    c = planted_case(form, "empty", 1, n, [4000, 6000, 6000 + 3 * m], first=2, rpw=2)
    c.offs = np.array([0, 4000, 4000, 4000, 4000, 6000 + m, 6000 + m, n, n], np.uint64)
    out.append(c)
    c = planted_case(form, "span", 1, n, [3 * S - m, 5 * S, 7 * S - 5, 9 * S - m, 9 * S + m], first=3, rpw=2)
    c.offs = np.array([0, 3 * S, 5 * S, 7 * S, 9 * S, n], np.uint64)
    out.append(c)
    n150 = 20 * R
    pos = [150 * 3 + 10, 150 * 7 + 150 - m, 150 * 12 + 150 - m + 1, 150 * 20, 150 * 31 + 75, 150 * 40 + 149, 150 * 60 + 150 - k,
           150 * 61 + 150 - k + 1, 150 * 90 + k - m, 150 * 101 + k - m + 1]
    c = planted_case(form, "r150", 1, n150, pos, first=4)
    c.offs = np.array(list(range(0, n150, 150)) + [n150], np.uint64)
    out.append(c)
    starts = [TILE + 5000, 2 * TILE + 100, 2 * TILE + 9000, 3 * TILE + 1, 3 * TILE + 4000, 3 * TILE + 4000 + k, 3 * TILE + 16000]
    pos = [100, 9000, TILE + 5000 - m, TILE + 5000 + 3 * m, 2 * TILE + 100, 2 * TILE + 8990, 2 * TILE + 12000, 3 * TILE + 1 + m, 3 * TILE + 4000 + 2,
           3 * TILE + 4000 + k + 40, 3 * TILE + 16000 - 2 * m, 3 * TILE + 16000 + 70]
    c = planted_case(form, "tile_starts", 1, 4 * TILE + 500, pos, first=5)
    c.offs = np.array([0] + starts + [4 * TILE + 500], np.uint64)
    out.append(c)
    return out


def compact_boundary(form, rpw):
    """g = 5, 80 lists: a record boundary on the boundary between k_compact's workgroups, position 64 * S, with a hit that
    ends there (a), starts there (b) or crosses it (c)"""
    _, m, _ = kmT(form)
    n = 80 * rpw * R
    edge = COMPACT_LISTS * rpw * R
    out = []
    for name, pos in (("a", [edge - m, edge + m]), ("b", [edge - 3 * m, edge]), ("c", [edge - 5, edge + 4 * m])):
        c = planted_case(form, "compact_%s_rpw%d" % (name, rpw), 5, n, pos + [100, n - m], first=rpw, rpw=rpw)
        c.offs = np.array([0, edge, n], np.uint64)
        out.append(c)
    return out


# ================================================================================================= sparse passes

def hit_index(mask, pos):
    return int(np.count_nonzero(mask[:pos]))


def sparse(form):
    """inputs for k_resolve, at (31, 11, 1000): w = k - m + 1 = 21, isolated hits 64 positions apart are clusters of one.
    head127/128/129: isolated hits put the head of a tandem run of 300 hits (no cut: equal hashes) at that hit index --
        the first and the last thread of a workgroup of 128, and a run that reaches more than 120 hits past the staged window
    head122: the run starts within 8 hits in front of a workgroup boundary
    cut_far: 260 copies of the pool m-mer of the LARGEST hash, then pool m-mers of smaller hashes: the first is a strict
        window minimum, a cut head beyond the staged window, found by head_kind on demand
    wave63/64/65: a run of differing pool m-mers (cut at its strict window minima) with its head at that hit index -- the
        wave sums of the write pass
    chunk4095/4096/4097: the same behind a tandem run of that many hits -- the chunk sums; more than 4096 + 1.25 x expected
        hits, so on a fresh context the hits-overflow retry runs too (retries holds "hits": Case.claim checks it against
        first_call_retries, and the runner gives each of these cases a context of its own -- a context that has retried
        starts its next call with room).  On the list forms the first attempt overflows the lists, the second the hits
        (k_compact again over intact lists), the third fits
    The head* and cut_far runs overflow their waves' lists on the list forms; they too run on contexts of their own, behind
    wave63/64/65, whose first attempt is what is checked"""
    k, m, T = kmT(form)
    lists = [] if form in DIRECT_FORMS else ["lists"]
    P = pl.pool(m, T)
    hashes = pl.xxh64(pl.canon(P.reshape(-1), m)[::m])
    row = pl.tandem_row(m, T)
    out = []

    def isolated(b, count, at=50):
        pos = [at + 64 * i for i in range(count)]
        pl.plant(b, pos, m, T, first=count)
        return pos[-1] + 64 if pos else at

    for name, lead, run in (("head127", 127, 300), ("head128", 128, 300), ("head129", 129, 300), ("head122", 122, 300)):
        n = 64 * lead + 300 * m + 4000
        b = bg(form, n, seed=7)
        at = isolated(b, lead) + 64
        put(b, at, pl.tandem(row, run))
        pl.plant(b, [at + run * m + 100, n - 500], m, T)

        def claim(mask, at=at, lead=lead, run=run):
            assert hit_index(mask, at) == lead and int(mask.sum()) == lead + run + 2
            assert mask[at:at + run * m:m].all() and run > RESOLVE - lead % RESOLVE + STAGED_AFTER
        out.append(Case(name, 1, b, check=claim, retries=lists))

    # cut_far
    order = np.argsort(hashes)
    big = None
    for i in order[::-1]:                                        # the largest hash that makes a clean tandem run
        t = np.tile(P[i], 6)
        want = np.zeros(len(t) - m + 1, bool)
        want[::m] = True
        if np.array_equal(pl.hit_mask(t, m, T), want):
            big = i
            break
    assert big is not None
    lead, run = 5, 260
    n = 64 * lead + (run + 40) * m + 3000
    b = bg(form, n, seed=8)
    at = isolated(b, lead) + 64
    tail = np.concatenate([P[i] for i in order[:30] if hashes[i] < hashes[big] and i != big])
    put(b, at, np.concatenate([pl.tandem(P[big], run), tail]))

    def cut_claim(mask, at=at, lead=lead, run=run):
        assert hit_index(mask, at) == lead and mask[at:at + run * m:m].all() and int(mask[at:at + run * m].sum()) == run
        assert mask[at + run * m] and lead + run > RESOLVE + STAGED_AFTER        # the cut head's index is not staged
    out.append(Case("cut_far", 1, b, check=cut_claim, retries=lists))

    for name, lead in (("wave63", 63), ("wave64", 64), ("wave65", 65)):
        n = 64 * lead + 40 * m + 3000
        b = bg(form, n, seed=9)
        at = isolated(b, lead) + 64
        put(b, at, pl.distinct_run(m, T, 30, first=lead))
        pl.plant(b, [at + 30 * m + 200, at + 30 * m + 900], m, T)

        def wave_claim(mask, at=at, lead=lead):
            assert hit_index(mask, at) == lead and mask[at:at + 30 * m:m].all()
        out.append(Case(name, 1, b, check=wave_claim))

    for name, lead in (("chunk4095", 4095), ("chunk4096", 4096), ("chunk4097", 4097)):
        n = 400 + lead * m + 40 * m + 3000
        b = bg(form, n, seed=10)
        put(b, 300, pl.tandem(row, lead))
        at = 300 + lead * m + 100
        put(b, at, pl.distinct_run(m, T, 30, first=lead))
        pl.plant(b, [at + 30 * m + 200, at + 30 * m + 900], m, T)

        def chunk_claim(mask, at=at, lead=lead, n=n):
            assert hit_index(mask, at) == lead and mask[at:at + 30 * m:m].all()
        out.append(Case(name, 1, b, check=chunk_claim, retries=lists + ["hits"]))
    return out


# =================================================================================================== the tables

LIST_GROUPS = {"chunk_offsets": chunk_offsets, "row_ends": row_ends, "rows_per_wave": rows_per_wave,
               "buffer_lengths": buffer_lengths, "queues": queues, "records": records}


@cached
def cases(group, form):
    if group in LIST_GROUPS:
        return LIST_GROUPS[group](form)
    if group == "direct":
        return direct(form)
    if group == "survivor_sums":
        return survivor_sums()
    if group == "compact_rpw1":
        return compact_boundary(form, 1)
    if group == "compact_rpw2":
        return compact_boundary(form, 2)
    if group == "sparse":
        return sparse(form)
    raise KeyError(group)


GROUPS = ([(g, f) for g in LIST_GROUPS for f in LIST_FORMS] +
          [("direct", f) for f in DIRECT_FORMS] + [("records", f) for f in DIRECT_FORMS] +
          [("survivor_sums", "pair_mid")] +
          [(g, f) for g in ("compact_rpw1", "compact_rpw2") for f in ("pair_mid", "single", "pair_k8", "bloom13")] +
          [("sparse", "pair_mid"), ("sparse", "single"), ("sparse", "direct")])
GROUP_IDS = ["%s-%s" % gf for gf in GROUPS]


# ======================================================================================================= CPU pins

def test_numpy_hash_equals_the_oracle():
    rng = np.random.default_rng(1)
    x = np.concatenate([np.array([0, 1, 4 ** 9 - 1, 4 ** 11 - 1, 4 ** 13 - 1, 4 ** 15 - 1, 2 ** 64 - 1], np.uint64),
                        rng.integers(0, 4 ** 15, 5000).astype(np.uint64), rng.integers(0, 2 ** 63, 5000).astype(np.uint64) * np.uint64(2) + np.uint64(1)])
    assert len(x) > 10 ** 4
    got = pl.xxh64(x)
    for v, h in zip(x.tolist(), got.tolist()):
        assert h == orc.xxh64(v), v


@pytest.mark.parametrize("m", [9, 11, 13, 15])
def test_canonical_values_equal_the_oracle(m):
    rng = np.random.default_rng(m)
    b = pl.LETTERS[rng.integers(0, 4, 3000)]
    f, c = pl.forward(b, m), pl.canon(b, m)
    assert len(c) == 3000 - m + 1
    for i in range(0, len(c)):
        assert int(f[i]) == orc.str2num(pl.text(b[i:i + m]))
        assert int(c[i]) == orc.canon64(int(f[i]), m)
    assert (pl.rc_values(f, m) == np.array([orc.rc64(int(v), m) for v in f], np.uint64)).all()
    assert pl.text(pl.to_bases(f[:50], m).reshape(-1)) == b"".join(pl.text(b[i:i + m]) for i in range(50))


@pytest.mark.parametrize("form", ["pair_mid", "pair_k8", "bloom13", "bloom15", "direct9"])
def test_every_superkmer_of_the_oracle_has_its_minimizer_on_a_masked_position(form):
    k, m, T = kmT(form)
    rng = np.random.default_rng(k)
    b = pl.LETTERS[rng.integers(0, 4, 200_000)]
    put(b, 5000, pl.tandem(pl.tandem_row(m, T), 40))
    mask = pl.hit_mask(b, m, T)
    c = pl.canon(b, m)
    em, _ = orc.scan(k, m, T, b, np.array([0, len(b)], np.uint64))
    assert len(em) > 5
    for e in em:
        a, z = int(e["start"]), int(e["start"]) + int(e["len"]) - m + 1          # the m-mer positions of the super-k-mer
        at = np.nonzero(mask[a:z] & (c[a:z] == np.uint64(e["minimizer"])))[0]
        assert at.size > 0, e
    # and every hit far enough from the record's ends lies inside a super-k-mer
    covered = np.zeros(len(b), bool)
    for e in em:
        covered[int(e["start"]):int(e["start"]) + int(e["len"])] = True
    assert covered[np.nonzero(mask)[0]].all()


def test_the_pools_hold_hits_on_both_strands_and_are_cached():
    for form in ("pair_mid", "pair_k8", "bloom15"):
        _, m, T = kmT(form)
        P = pl.pool(m, T)
        assert P is pl.pool(m, T) and len(P) >= 2
        v = pl.forward(P.reshape(-1), m)[::m]
        assert (pl.xxh64(np.minimum(v, pl.rc_values(v, m))) <= np.uint64(T)).all()
        assert len(np.unique(v)) == len(v) and np.isin(pl.rc_values(v, m), v).all()
    _, m, T = kmT("pair_mid")
    assert len(pl.pool_values(m, T)) == 89                       # k31 m11 s1000: 89 canonical 11-mers


def test_a_planted_plan_reproduces_its_mask_exactly():
    for form in ("pair_mid", "pair_k8", "bloom13", "bloom15"):
        _, m, T = kmT(form)
        pos = [0, 2 * m, 1000, 1000 + 2 * m, 2 * R + 7, 5000, 5000 + 2 * m, 20_000 - m]
        b = pl.planted(20_000, pos, m, T, seed=4)
        assert np.nonzero(pl.hit_mask(b, m, T))[0].tolist() == pos
    with pytest.raises(AssertionError):                          # closer than 2m: refused
        pl.planted(1000, [100, 100 + 2 * m - 1], m, T, seed=4)
    x = pl.near_hit(11, threshold("pair_mid"))
    t = pl.tandem(x, 30)
    assert not pl.hit_mask(t, 11, threshold("pair_mid")).any()
    assert pl.survivors_pair_mid(t, 11, threshold("pair_mid"))[:29 * 11:11].all()
    assert pl.survivors_single(t, 11, threshold("single"))[:29 * 11:11].all()
    j, head = pl.bait(11, threshold("pair_mid"))
    assert j >= 1 and pl.hit_mask(np.concatenate([head, np.full(j, pl.LETTERS[0], np.uint8)]), 11, threshold("pair_mid"))[0]


def test_what_the_replaced_seams_rest_on():
    """two seams of the issue cannot be built at its configurations; the reasons are pinned here, so that a change of
    threshold or seed that makes them possible fails this test instead of leaving the replacement in place"""
    # (31, 11, 1000): no hit m-mer overlaps another by m - 1 bases, so no hit at offset 0 directly behind one at offset 15
    # (chunk_offsets: offset15_in_adjacent_lanes stands in)
    _, m, T = kmT("pair_mid")
    P = pl.pool(m, T)
    assert pl.pool_complete(m) and len(P) == 178
    suffixes = pl.forward(P[:, 1:].reshape(-1), m - 1)[::m - 1]
    prefixes = pl.forward(P[:, :m - 1].reshape(-1), m - 1)[::m - 1]
    assert not np.isin(suffixes, prefixes).any()
    # (63, 15, 100): no sequence of period <= 7 is a hit, so a row of the Bloom form of m = 15 cannot hold more than 128 hits
    # (queues: `dense` exists for m = 13 only); a period of 8 gives 126 to a row
    _, m, T = kmT("bloom15")
    for period in range(1, 8):
        assert len(pl.periodic_hits(m, T, period)) == 0, period
    assert R // 8 < PUSH_WINDOW
    # and the vectorised search agrees with the mask where hits exist
    _, m, T = kmT("bloom13")
    for v in pl.periodic_hits(m, T, 6):
        assert pl.hit_mask(np.tile(pl.to_bases(v, 6), 4), m, T)[0]
    assert len(pl.periodic_hits(m, T, 6)) > 0


def test_the_survivor_models_hold_every_hit():
    """a hit passes its own table: the models are supersets of the mask"""
    _, m, T = kmT("pair_mid")
    b = planted_case("pair_mid", "x", 1, 40_000, [100 + 97 * i for i in range(300)]).bases
    mask = pl.hit_mask(b, m, T)
    assert mask.sum() == 300
    for model in (pl.survivors_pair_mid, pl.survivors_single):
        assert model(b, m, T)[:len(mask)][mask].all()


@pytest.mark.parametrize("group,form", GROUPS, ids=GROUP_IDS)
def test_the_cases_are_what_they_are_called(group, form):
    cs = cases(group, form)
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        assert len(c.bases) <= 330_000
        c.claim(form)


def second_threshold_case(form, i):
    """isolated seams for the forms that exist only as a second threshold"""
    return planted_case(form, "lanes_%d" % i, 1, 3 * WAVES * R, [(7 + 5 * i) * R + 65 * j for j in range(16)], first=i, rpw=3)


def overflow_sequence(form):
    other = OTHER_THRESHOLD[form]
    return [(form, overflow_run(form)), (form, cases("chunk_offsets", form)[0]),
            (other, cases("chunk_offsets", other)[0] if other in LIST_FORMS else second_threshold_case(other, 0)),
            (form, cases("rows_per_wave", form)[3]), (form, overflow_run(form))]


def many_calls():
    plan = [("pair_mid", "chunk_offsets", 0), ("bloom13", "rows_per_wave", 2), ("pair_k8", "chunk_offsets", 1), ("single", "queues", "tandem"),
            ("pair_mid_s300", None, 0), ("direct", "direct", 0), ("bloom15", "queues", "tandem"), ("single_s300", None, 0), ("single", "chunk_offsets", 2),
            ("pair_mid", "queues", "tandem"), ("direct9", "direct", 1), ("pair_k8", "rows_per_wave", 4), ("bloom13", "chunk_offsets", 0),
            ("bloom15", "buffer_lengths", 7), ("pair_mid", "records", 3), ("pair_mid_s300", None, 1), ("pair_mid", "chunk_offsets", 2)]
    def pick(group, form, i):
        return cases(group, form)[i] if isinstance(i, int) else next(c for c in cases(group, form) if c.name == i)
    return [(form, second_threshold_case(form, i) if group is None else pick(group, form, i)) for form, group, i in plan]


def test_the_sequences_are_what_they_are_called():
    for form in LIST_FORMS:
        seq = overflow_sequence(form)
        assert len({threshold(f) for f, _ in seq}) == 2
        for f, c in seq:
            c.claim(f)
    seq = many_calls()
    assert len({threshold(f) for f, _ in seq}) >= 6 and len({FORMS[f][3] for f, _ in seq}) == 4
    for f, c in seq:
        c.claim(f)


# ========================================================================================================= GPU

def _assert_stream_equal(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for f in ("rec", "minimizer", "start", "len", "rev"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (tag, f, int(bad[0]), got[bad[0]], want[bad[0]])


def context(g):
    c = sp.Context(0)
    c.set_cu_count(g, 1)
    return c


def run_case(ctx, form, case, packed_too=True):
    """the case through scan_device and scan_hits_device, ASCII and (pair, Bloom) packed, against the oracle and the mask.
    ctx = None: a fresh context for each of the two, so that what runs is the first call of a context"""
    import torch
    k, m, s, flag = FORMS[form]
    mask = case.claim(form)
    want_hits = int(mask.sum())
    want, _ = orc.scan(k, m, threshold(form), case.bases, case.offs)
    n = len(case.bases)
    d_b = torch.from_numpy(case.bases.copy()).cuda()
    d_o = torch.from_numpy(case.offs.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    for packed in ((False, True) if packed_too and form in PACKED_FORMS else (False,)):
        tag = (form, case.name, "packed" if packed else "ascii")
        p = sp.make_params(k, m, s, flags=flag | (sp.SPSP_SCAN_PACKED_INPUT if packed else 0))
        assert p.threshold == threshold(form)
        c = context(case.g) if ctx is None else ctx
        try:
            ptr = c.pack_bases_device(d_b.data_ptr(), n) if packed else d_b.data_ptr()
            d_out, n_out = c.scan_device(p, ptr, n, d_o.data_ptr(), len(case.offs) - 1)
            got = c.to_host(d_out, n_out, sp.SUPERKMER_DTYPE) if n_out else np.zeros(0, sp.SUPERKMER_DTYPE)
            _assert_stream_equal(got, want, tag)
            assert c.scan_hits_device(p, ptr, n) == want_hits, tag
        finally:
            if ctx is None:
                c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("group,form", GROUPS, ids=GROUP_IDS)
def test_scan_seams(group, form):
    """the cases whose first attempt fits share one context, in order; a case that makes the host retry (Case.retries) gets
    fresh contexts, so that nothing an overflow teaches a context reaches another case"""
    cs = cases(group, form)
    assert all(c.g == cs[0].g for c in cs)
    with context(cs[0].g) as ctx:
        for c in cs:
            if not c.retries:
                run_case(ctx, form, c)
    for c in cs:
        if c.retries:
            run_case(None, form, c)


@pytest.mark.gpu
@pytest.mark.parametrize("form", LIST_FORMS)
def test_list_overflow_then_isolated_seams_on_one_context(form):
    """a wave's slice holds 1.5 x expected + 48 hits: the tandem run overflows it, the host grows the lists and repeats.  The
    same context then scans isolated seams at the same threshold (the grown capacity is kept) and at another one (it is
    dropped, and the table rebuilt), and the run again"""
    with context(1) as ctx:
        for f, c in overflow_sequence(form):
            run_case(ctx, f, c)


@pytest.mark.gpu
def test_one_context_over_many_calls():
    """the forms interleaved on one context, thresholds and m alternating, packed and ASCII: the cached tables (pair_valid,
    filter_valid, bloom_valid) and the learned capacities of one call meet the next"""
    with context(1) as ctx:
        for f, c in many_calls():
            run_case(ctx, f, c)
