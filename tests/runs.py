"""Records whose resets, chains and record boundaries lie exactly where a test puts them, and models of what the scan by
segments and the super-k-mer count (supersampler_amd/csrc/spsp_stats.hip) make of them.

No GPU use: numpy and plain Python.  tests/test_segment_seams.py builds its inputs with this module and pins the models on
the CPU against the oracle.  Hashes and canonical values are tests/planted.py's.

A RESET at iteration i of a record is h[i + km + 1] < min(h[i .. i + km]), km = k - m, h the hash of the canonical m-mer at
each place: the entering m-mer beats the window.  Resets depend on the record alone.  A homopolymer or a tandem repeat of
period <= w = km + 1 has none once the window lies inside it; random sequence has one every few iterations; a filler record
of f bases in front moves everything behind it by f places.  An EVENT is a record start (len >= k) or a reset; its CHAIN are
the rescans up to the next reset or the record's end (regular_minimizer_pos with its tie rules).

The kernels cut the concatenated records at fixed places (constants below, named as in spsp_stats.hip):
    tile t       places [2048 t, 2048 t + 2048) own their events; the m-mers of 3072 + 64 places are held, so a chain is followed
                 up to place LIMIT = 3072 of its tile.  A chain LEAVES when no reset lies in [from, LIMIT) and the record's
                 iterations go past LIMIT; it then STOPS s = (next reset, or the record's end) - LIMIT iterations behind it
    chunk c      iterations [512 c, 512 c + 512) of the chunk form; its first piece is OPEN when it starts inside a record, more
                 than `lookback` iterations in, and the `lookback` iterations in front of it hold no reset

    reset_mask(rec, k, m)            the resets of a record, one flag per iteration
    events(recs, k, m)               Event per record start / reset, with tile, place and where its chain stops
    leaving(recs, k, m)              the (event, kind, s, by) whose chain leaves its tile's halo; asserts at most one per tile
    count_model(recs, k, m)          total_superkmer_number as k_seg_count + k_seg_tail count it
    scan_form(recs, k, m)            what k_seg_scan's slow-walk budget makes of the leaving chains: (form, least, most left over)
    open_chunks(recs, k, m, lookback) the chunks k_stat_count marks open
    Case                             a name, the records and a claim"""
import functools

import numpy as np

import planted as pl

SEG_ITER = 2048                  # kSegIter
SEG_HALO = 1024                  # kSegHalo
LIMIT = SEG_ITER + SEG_HALO      # k_seg_count / k_seg_scan: constexpr uint32_t LIMIT
STAT_CHUNK = 512                 # kStatChunk
SLOW_STEP = 256                  # k_seg_scan: (steps & 255u) == 0 -> atomicAdd(over_n + 1, 256u)
SLOW_BASE, SLOW_PER = 512, 20000  # seg_scan_count: slow_budget = min(1 << 20, 512 + n_bases / 20000)
RING = 64                        # seg_rescan_ring: index = m-mer place & 63

A, C, T, G = (int(x) for x in pl.LETTERS)


def random_bases(n, seed):
    return pl.LETTERS[np.random.default_rng(seed).integers(0, 4, n)]


def homopolymer(n, letter=A):
    return np.full(n, letter, np.uint8)


def tandem(unit, n):
    """n bases of the repeated unit"""
    unit = np.asarray(unit, np.uint8)
    return np.tile(unit, n // len(unit) + 1)[:n]


def cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts]) if parts else np.zeros(0, np.uint8)


def concat(recs):
    """records -> (bases, offsets)"""
    offs = np.zeros(len(recs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in recs])
    return (cat(*recs) if recs else np.zeros(0, np.uint8)), offs


def lookback_of(k, m):
    """count_superkmers_impl: max(64, 8 w)"""
    return max(64, 8 * (k - m + 1))


def slow_budget(n_bases):
    return min(1 << 20, SLOW_BASE + n_bases // SLOW_PER)


class Record:
    """one record at (k, m): hashes, canonical values, strands and resets"""

    def __init__(self, rec, k, m):
        self.n, self.k, self.m, self.km = len(rec), k, m, k - m
        self.n_iter = self.n - k if self.n >= k else -1             # iterations 0 .. n_iter - 1; -1: no k-mer, no event
        if self.n >= m:
            f = pl.forward(rec, m)
            c = pl.canon(rec, m)
            self.h = pl.xxh64(c)
            self.hl, self.cl, self.rl = self.h.tolist(), c.tolist(), (c != f).tolist()
        if self.n_iter > 0:
            mn = np.lib.stride_tricks.sliding_window_view(self.h, self.km + 1).min(axis=1)
            self.reset = self.h[self.km + 1:] < mn[:self.n_iter]
        else:
            self.reset = np.zeros(0, bool)
        self.resets = np.nonzero(self.reset)[0]

    def rescan(self, ks):
        """regular_minimizer_pos of the k-mer at ks, right to left (StatMachine::rescan, seg_rescan) -> pos"""
        km, hl, cl, rl = self.km, self.hl, self.cl, self.rl
        mini, is_rev, hm = cl[ks + km], rl[ks + km], hl[ks + km]
        pos = 0 if is_rev else km
        for i in range(1, km + 1):
            off = km - i
            h = hl[ks + off]
            if hm > h:
                pos, mini, is_rev, hm = off, cl[ks + off], rl[ks + off], h
            elif cl[ks + off] == mini and rl[ks + off] == is_rev:
                if is_rev and pos > i:
                    pos = i
                if not is_rev and pos > off:
                    pos = off
        return pos

    def next_reset(self, frm):
        """the first reset at or behind iteration frm, or n_iter"""
        j = int(np.searchsorted(self.resets, frm))
        return int(self.resets[j]) if j < len(self.resets) else self.n_iter

    def chain(self, P, stop, frm=None):
        """the iterations in [frm, stop) at which a chain with believed position P rescans"""
        out = []
        while P < stop:
            if frm is None or P >= frm:
                out.append(P)
            P = P + 1 + self.rescan(P + 1)
        return out

    def first_P(self, i, kind):
        return i + self.rescan(i) if kind == 0 else i + self.km + 1

    @functools.cached_property
    def count(self):
        """the record's super-k-mers: its start, its resets and the rescans of their chains"""
        if self.n_iter < 0:
            return 0
        total = 1 + len(self.chain(self.first_P(0, 0), self.next_reset(0)))
        for i in self.resets.tolist():
            total += 1 + len(self.chain(i + self.km + 1, self.next_reset(i + 1)))
        return total


@functools.lru_cache(maxsize=4096)
def _record(data, k, m):
    return Record(np.frombuffer(data, np.uint8), k, m)


def record(rec, k, m):
    return _record(bytes(np.asarray(rec, np.uint8)), k, m)


def reset_mask(rec, k, m):
    return record(rec, k, m).reset


class Event:
    """a record start and / or a reset at global place g = tile * 2048 + place: iteration i of record r.  stop[kind] is the
    global place of the next reset behind it or of the record's end (kind 0: the start's chain, from g; 1: the reset's, from g + 1)"""

    def __init__(self, g, r, i, is_start, is_reset, R, r0):
        self.g, self.r, self.i, self.is_start, self.is_reset = g, r, i, is_start, is_reset
        self.tile, self.place = divmod(g, SEG_ITER)
        self.end = r0 + R.n_iter
        self.stop, self.by = {}, {}
        for kind, frm in ((0, i), (1, i + 1)):
            if (is_start, is_reset)[kind]:
                x = R.next_reset(frm) if frm < R.n_iter else R.n_iter
                self.stop[kind], self.by[kind] = r0 + x, "reset" if x < R.n_iter else "end"

    def kinds(self):
        return sorted(self.stop)


def events(recs, k, m):
    out, r0 = [], 0
    for r, rec in enumerate(recs):
        R = record(rec, k, m)
        if R.n_iter >= 0:
            at = sorted(set([0] + R.resets.tolist()))
            for i in at:
                out.append(Event(r0 + i, r, i, i == 0, bool(i < R.n_iter and R.reset[i]), R, r0))
        r0 += len(rec)
    return out


def tile_events(recs, k, m):
    """tile -> its events' places, every tile of the input (ceil(n_bases / 2048)) present"""
    n = sum(len(r) for r in recs)
    out = {t: [] for t in range((n + SEG_ITER - 1) // SEG_ITER)}
    for e in events(recs, k, m):
        out[e.tile].append(e.place)
    return out


def leaving(recs, k, m):
    """[(event, kind, s, by)]: the chains that leave their tile's halo -- no reset in [from, LIMIT) of the owning tile and the
    record's iterations go past LIMIT -- with the iterations s behind LIMIT at which they stop, by a "reset" or the record's "end".
    At most one per tile: a later event of the tile would be a reset of the same record in front of LIMIT"""
    out = []
    for e in events(recs, k, m):
        lim = e.tile * SEG_ITER + LIMIT
        for kind in e.kinds():
            if e.stop[kind] >= lim and e.end > lim:
                out.append((e, kind, e.stop[kind] - lim, e.by[kind]))
    tiles = [e.tile for e, _, _, _ in out]
    assert len(set(tiles)) == len(tiles), ("two chains leave one tile", tiles)
    return out


def count_model(recs, k, m):
    return sum(record(rec, k, m).count for rec in recs)


def rescans_behind_halo(recs, k, m, left):
    """the iterations (of its record) behind LIMIT at which a leaving chain (event, kind, s, by) rescans"""
    e, kind, s, _ = left
    R = record(recs[e.r], k, m)
    r0 = e.g - e.i
    lim = e.tile * SEG_ITER + LIMIT - r0
    return R.chain(R.first_P(e.i, kind), lim + s, frm=lim)


def scan_form(recs, k, m):
    """-> (form, least, most chains left over).  A lane behind its halo takes 256 iterations from the call's budget at steps 0,
    256, 512, ...; step s is the one that meets the reset or the record's end, so a chain needs s // 256 + 1 grants.  If all
    the grants the chains need fit the budget every chain ends (form 1), whatever the order.  If they do not, some grant is
    refused whatever the order (a chain stops asking only when it has ended or was refused), so at least one chain is left
    over and the product scan takes the call (form 3)"""
    n = sum(len(r) for r in recs)
    if len(recs) == 0 or n < k:
        return 0, 0, 0
    lv = leaving(recs, k, m)
    grants = slow_budget(n) // SLOW_STEP
    need = [s // SLOW_STEP + 1 for _, _, s, _ in lv]
    if sum(need) <= grants:
        return 1, 0, 0
    return 3, 1, len(lv)


def open_chunks(recs, k, m, lookback):
    """the chunks c whose first piece k_stat_count marks open: the record that holds place 512 c has a k-mer, the chunk starts at
    its iteration a with lookback < a < n_iter, and no reset lies in [a - lookback, a).  (a <= lookback: the lane starts at
    iteration 0, which is exact.)  A reset at distance d in front of the chunk is iteration a - d: d <= lookback closes it"""
    _, offs = concat(recs)
    offs = offs.astype(np.int64)
    n = int(offs[-1])
    out = []
    for c in range((n + STAT_CHUNK - 1) // STAT_CHUNK):
        g0 = c * STAT_CHUNK
        r = int(np.searchsorted(offs[:-1], g0, side="right")) - 1       # the last record with rec_off[r] <= g0 (an empty one included)
        R = record(recs[r], k, m)
        a = g0 - int(offs[r])
        if R.n_iter < 0 or a == 0 or a >= R.n_iter or a <= lookback:
            continue
        if not R.reset[a - lookback:a].any():
            out.append(c)
    return out


def open_runs(recs, k, m, lookback):
    """the runs of consecutive open chunks inside one record, as lists"""
    _, offs = concat(recs)
    offs = offs.astype(np.int64)
    runs = []
    for c in open_chunks(recs, k, m, lookback):
        r = int(np.searchsorted(offs[:-1], c * STAT_CHUNK, side="right")) - 1
        if runs and runs[-1][-1] == c - 1 and (c - 1) * STAT_CHUNK > int(offs[r]):
            runs[-1].append(c)
        else:
            runs.append([c])
    return runs


# ------------------------------------------------------------------------------------------------------------ builders

def longest_gap(rec, k, m):
    """-> (event iteration e, stop x, by): the event of the record whose chain runs longest before the next reset or the end"""
    R = record(rec, k, m)
    pts = sorted(set([0] + R.resets.tolist()))
    best = None
    for i in pts:
        is_reset = bool(i < R.n_iter and R.reset[i])
        x = R.next_reset(i + 1) if is_reset else R.next_reset(i)
        if best is None or x - i > best[1] - best[0]:
            best = (i, x, "reset" if x < R.n_iter else "end")
    return best


def fit_gap(make, want, k, m):
    """make(L, v) -> a record with a reset-free run of L bases (v: a variant of its flanks); L is moved until the record's longest
    gap is `want` iterations.  A tandem repeat leaves its run at a phase that depends on L, so not every gap has an L with
    every flank: the next variant is tried"""
    for v in range(16):
        L = want
        for _ in range(12):
            rec = make(L, v)
            e, x, _ = longest_gap(rec, k, m)
            if x - e == want:
                return rec
            L += want - (x - e)
            if L <= 0:
                break
    raise AssertionError(("no run length gives a gap of", want))


def filler(f, seed=77):
    """a record of f random bases in front: moves everything behind it by f places"""
    return random_bases(f, seed)


def put_at(rec, iteration, g, seed=77):
    """-> [filler, rec] so that `iteration` of rec is global place g"""
    assert g >= iteration, (g, iteration)
    return [filler(g - iteration, seed), np.asarray(rec, np.uint8)]


class Case:
    """one input: a name, the records, and what the input claims to be (check(case, k, m) asserts it from the models)"""

    def __init__(self, name, recs, check=None):
        self.name = name
        self.recs = [np.ascontiguousarray(r, dtype=np.uint8) for r in recs]
        self.bases, self.offs = concat(self.recs)
        self.check = check

    def claim(self, k, m):
        assert len(self.bases) < SLOW_PER, (self.name, len(self.bases))          # the slow-walk budget is exactly 512
        for rec in self.recs:                                                    # no serial walk of more than 5 000 iterations
            R = record(rec, k, m)
            if R.n_iter > 0:
                pts = np.concatenate([[0], R.resets, [R.n_iter]])
                assert int(np.diff(pts).max()) <= 5000, (self.name, int(np.diff(pts).max()))
        leaving(self.recs, k, m)                                                 # (at most one per tile)
        if self.check is not None:
            self.check(self, k, m)
