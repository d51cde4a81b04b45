"""The comparison's row sums at their seams (supersampler_amd/csrc/spsp_compare.hip: launch_accumulate_sparse, k_accumulate_sparse and
the part scatter, grouping and list fill in front of them), on hand-built keys.

The all-vs-all path cuts its work at fixed places whatever the sketches are: holder lists in 16-byte words of eight u16 (a length,
then ids), read four words at once below 32 ids and pooled by the wave from 32 on, their length carried by the reference up to 62;
a workgroup's list of at most 1024 touched counters; column blocks of 16 384 sketches; 16-bit counters up to rows of 65 535 keys,
launches of their own for longer rows and slices for every row from 65 long rows on.  Sketches of simulated families meet those
places by luck; here a test PRESCRIBES, per key, the set of sketches that hold it.

Keys: key g has kmer_lo = mixed(g), kmer_hi = ~kmer_lo (k = 63) and a minimizer chosen for the place the key shall take in its
sketches (a sketch is sorted by (minimizer, hi, lo)); a few keys are twins of another one, equal to it but for the minimizer, for
lo, or for hi, and held by other sketches.  Expected matrix: over the keys, every pair i < j of holders, counted with np.unique on
i << 16 | j (pair_model; held to Python set algebra below).  Integers only, no tolerance anywhere.  Cells come back in no fixed
order: they are compared sorted, and no pair may come twice.

What a wrong kernel would look like, and where it shows:
    a short list read one word short or long, or a length taken from the reference where the list carries it: holders_input(),
        every holder count around 8, 16, 24, 32, 40 and 62 .. 65, as runs and as random subsets
    a pooled word given to the wrong lane's list, a prefix sum or search off by one lane or one word: the rows of holders_input()
        whose first 64 keys hold one long list at lane 0 or 63, or long lists of 127, 128 and 129 pooled words
    a key round that drops or repeats its last key: its sketches of exactly 1024, 1025, 2048 and 2049 keys
    keys taken for equal on two of their three words: the twins
    counters left over from a row that filled or overflowed the touched list, a list entry past its end: touch_one_copy(),
        rows of 1023, 1024, 1025 and 8252 partners among rows of one or two
    a column told once per copy of its counter, or a copy left out of its sum: touch_eight_copies(), 1016, 1024, 1032 touched
        counters of 127, 128, 129 columns, every cell 8
    cells of the second column block lost, doubled or written to the first block's places: blocks_input(), 16 384 (one block),
        16 385 (a block of one column) and 16 448 sketches
    a 16-bit counter that carries into its neighbour or wraps: half_input(65535), columns 4 and 5 of row 0 both 0xFFFF in one word;
        half_input(65536): the same rows one key longer, summed in slices by launches of their own
    slices that overlap or leave a key out, 16-bit counters kept for sliced rows: long_rows_input(64) and (65)

A key part that overflows would send a comparison another way (the spill); no input here may do that.  The scatter's dealing of
keys to parts is copied below (part_loads) and every input is held to it without a GPU; on the GPU the trace of
SPSP_DEBUG_SPILL_TRACE says which form ran and must not speak of a spill.

long_rows_input is k = 63: up to 128 sketches of k <= 32 take the small form, which has no row sums.  Its slices: 65 long rows make
every row two slices, of 32 768 + 32 768, 32 769 + 32 768 and 49 153 + 49 152 keys; among 64 long rows the row of 98 305 keys is
three slices of 32 769, 32 769 and 32 767.

Wall times on an MI355X are printed per child process (pytest -s)."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import supersampler_amd as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = 0x9E3779B97F4A7C15
SENTINEL = 0x5A5A5A5A                           # what the cells call's scratch matrix is filled with: still there iff the cells left the row sums directly
FIRST_MN = 1000                                 # minimizers below it are given by hand, to the keys a sketch shall begin with

# spsp_compare.hip
PART_CAP, PART_MEAN, SMALL_CAP, SMALL_MEAN, SMALL_N = 4096, 2900, 2048, 1450, 128
SPARSE_COLS, TOUCH_CAP, LONG_ROW, REF_LEN_MAX, POOLED_FROM = 16384, 1024, 65535, 63, 32

HOLDERS = (1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 39, 40, 41, 62, 63, 64, 65, 127, 128, 129, 199, 200)
PER_HOLDER_COUNT = 36                           # keys per holder count: 18 runs of consecutive sketches, 18 random subsets
SHORT = (2, 3, 9, 17, 25, 31)

cached = functools.lru_cache(maxsize=None)


def mixed(i):
    """indices -> 64-bit words that are neither the index nor near their neighbours' words (the product wraps; GOLD is odd, so
    distinct indices give distinct words)"""
    return (np.asarray(i, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLD)


# ------------------------------------------------------------------------------------------------ keys and model

class Problem:
    """n sketches as the comparison takes them (mn, lo, hi or None, off) and, per record, the key and the sketch it belongs to"""


class Builder:
    def __init__(self, n, k, salt=0):
        self.n, self.k, self.K, self.salt = n, k, 0, salt                       # salt: key g takes its words from g + salt
        self.rec_key, self.rec_sk, self.mn, self.twins = [], [], [], []

    def records(self, key, sk, n_keys, mn=None):
        """n_keys new keys; record r says that sketch sk[r] holds new key key[r] -> the keys' indices"""
        g = np.arange(self.K, self.K + n_keys, dtype=np.int64)
        self.rec_key.append(np.asarray(key, dtype=np.int64) + self.K)
        self.rec_sk.append(np.asarray(sk, dtype=np.int64))
        self.mn.append(FIRST_MN + ((mixed(g + self.salt) >> np.uint64(40)) % np.uint64(3000)).astype(np.int64) if mn is None
                       else np.broadcast_to(np.asarray(mn, dtype=np.int64), (n_keys,)))
        self.K += n_keys
        return g

    def add(self, holders, mn=None):
        """holders: keys x h array, or a list of arrays: the sketches that hold each new key -> the keys' indices"""
        if isinstance(holders, np.ndarray) and holders.ndim == 2:
            return self.records(np.repeat(np.arange(len(holders)), holders.shape[1]), holders.reshape(-1), len(holders), mn)
        cnt = [len(h) for h in holders]
        return self.records(np.repeat(np.arange(len(holders)), cnt), np.concatenate([np.asarray(h, dtype=np.int64) for h in holders]), len(holders), mn)

    def twin(self, g, word, holders):
        """a new key equal to key g but for one word ("mn", "lo" or "hi"), held by `holders`"""
        t = int(self.add([holders])[0])
        self.twins.append((t, int(g), word))
        return t

    def keys_of_sketch(self):
        return np.bincount(np.concatenate(self.rec_sk), minlength=self.n)

    def finish(self):
        P = Problem()
        P.n, P.k, P.K = self.n, self.k, self.K
        g = np.arange(self.K, dtype=np.int64)
        lo, mn = mixed(g + self.salt), np.concatenate(self.mn)
        hi = ~lo
        for t, s, word in self.twins:
            lo[t], hi[t], mn[t] = lo[s], hi[s], mn[s]
            if word == "mn":
                mn[t] = mn[s] + 1
            elif word == "lo":
                lo[t] = lo[s] ^ np.uint64(1 << 33)
            else:
                hi[t] = hi[s] ^ np.uint64(1 << 33)
        assert mn.min() >= 0 and mn.max() < 4 ** 11
        if self.k <= 32:
            hi = np.zeros(self.K, np.uint64)
        key, sk = np.concatenate(self.rec_key), np.concatenate(self.rec_sk)
        assert sk.min() >= 0 and sk.max() < self.n
        first = (sk.astype(np.uint64) << np.uint64(32)) | mn[key].astype(np.uint64)
        order = np.lexsort((lo[key], first)) if self.k <= 32 else np.lexsort((lo[key], hi[key], first))
        P.rec_key, P.rec_sk = key[order], sk[order]
        P.key_mn, P.key_lo, P.key_hi = mn.astype(np.uint32), lo, hi
        P.mn, P.lo, P.hi = P.key_mn[P.rec_key], lo[P.rec_key], (hi[P.rec_key] if self.k > 32 else None)
        P.off = np.concatenate([[0], np.cumsum(np.bincount(P.rec_sk, minlength=self.n))]).astype(np.uint64)
        P.twins = list(self.twins)
        P.want = pair_model(P.rec_key, P.rec_sk)
        return P


def pair_model(rec_key, rec_sk):
    """records (key, sketch) -> the pair matrix's non-zero cells as sorted packed words i << 48 | j << 32 | count: over the keys,
    every pair i < j of a key's holders (equal holder lists are enumerated once and weighted)"""
    order = np.lexsort((rec_sk, rec_key))
    key, sk = np.asarray(rec_key)[order], np.asarray(rec_sk, dtype=np.int64)[order]
    h = np.bincount(key)
    start = np.concatenate([[0], np.cumsum(h)])[:-1]
    codes, weights = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for hv in np.unique(h[h >= 2]).tolist():
        lists = sk[start[h == hv][:, None] + np.arange(hv)[None, :]]            # keys x hv, every row ascending
        assert (np.diff(lists, axis=1) > 0).all(), "a sketch holds a key twice"
        lists, mult = np.unique(lists, axis=0, return_counts=True)
        a, b = np.triu_indices(hv, 1)
        codes.append(((lists[:, a] << 16) | lists[:, b]).reshape(-1))
        weights.append(np.repeat(mult, len(a)))
    pair, inverse = np.unique(np.concatenate(codes), return_inverse=True)
    count = np.bincount(inverse.reshape(-1), weights=np.concatenate(weights), minlength=len(pair)).astype(np.uint64)   # (exact: far below 2**53)
    assert count.max(initial=0) < (1 << 32)
    return ((pair >> 16).astype(np.uint64) << np.uint64(48)) | ((pair & 0xffff).astype(np.uint64) << np.uint64(32)) | count


def cells_of(want):
    """packed cells -> (i, j, count)"""
    return (want >> np.uint64(48)).astype(np.int64), ((want >> np.uint64(32)) & np.uint64(0xffff)).astype(np.int64), (want & np.uint64(0xffffffff)).astype(np.int64)


def cell_dict(want):
    i, j, c = cells_of(want)
    return {(a, b): v for a, b, v in zip(i.tolist(), j.tolist(), c.tolist())}


def partners(want, n):
    """-> cells per row"""
    return np.bincount(cells_of(want)[0], minlength=n)


def mix64(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xbf58476d1ce4e5b9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94d049bb133111eb)
    return x ^ (x >> np.uint64(31))


def part_loads(P, small=False):
    """records per key part, as k_parts_scatter deals them: the part is the top of key_hash() times the number of parts"""
    h = mix64(P.key_lo ^ np.uint64(0xA0761D6478BD642F))
    h = mix64(h + P.key_mn.astype(np.uint64) * np.uint64(0xE7037ED1A0B428DB))
    if P.k > 32:
        h = mix64(h ^ P.key_hi)
    mean = SMALL_MEAN if small else PART_MEAN
    n_parts = max(1, -(-len(P.mn) // mean))
    part = (((h >> np.uint64(32)) * np.uint64(n_parts)) >> np.uint64(32)).astype(np.int64)
    return np.bincount(part, weights=np.bincount(P.rec_key, minlength=P.K), minlength=n_parts).astype(np.int64)    # (a key's records go where the key goes)


def takes_small_form(P):
    return P.k <= 32 and P.n <= SMALL_N


def holder_histogram(P):
    """from the arrays that go to the device: distinct (mn, hi, lo) keys -> {holder count: keys}"""
    words = np.stack([P.mn.astype(np.uint64), P.hi if P.hi is not None else np.zeros(len(P.mn), np.uint64), P.lo], axis=1)
    _, counts = np.unique(words, axis=0, return_counts=True)
    h, keys = np.unique(counts, return_counts=True)
    return dict(zip(h.tolist(), keys.tolist()))


def strictly_sorted(P):
    """every sketch strictly increasing by (minimizer, hi, lo)"""
    mn, lo = P.mn.astype(np.int64), P.lo
    hi = P.hi if P.hi is not None else np.zeros(len(lo), np.uint64)
    up = (mn[1:] > mn[:-1]) | ((mn[1:] == mn[:-1]) & ((hi[1:] > hi[:-1]) | ((hi[1:] == hi[:-1]) & (lo[1:] > lo[:-1]))))
    same_sketch = P.rec_sk[1:] == P.rec_sk[:-1]
    return bool((up | ~same_sketch).all()) and bool((np.diff(P.rec_sk) >= 0).all())


# ------------------------------------------------------------------------------------------------ the inputs

# holders_input(200, k): sketch -> (holder count, lane) of the long lists among its first 64 keys
POOL_ROWS = {
    1: [(40, 0)],                                                               # one long list, at lane 0
    2: [(33, 63)],                                                              # ... at lane 63
    3: [(32, l) for l in range(0, 56, 2)] + [(40, 56), (40, 58), (40, 63)],     # 28 x 4 + 3 x 5 = 127 pooled words
    4: [(32, l) for l in range(0, 64, 2)],                                      # 32 x 4 = 128
    5: [(32, l) for l in range(0, 62, 2)] + [(40, 63)],                         # 31 x 4 + 5 = 129
}
ROUND_ROWS = {6: 1024, 7: 1025, 8: 2048, 9: 2049}                               # sketch -> its exact key count
PLAIN_FROM = 10                                                                 # sketches from here on are no special rows


@cached
def holders_input(n, k, special=True, records=150_000):
    """every holder count of HOLDERS (capped at n) PER_HOLDER_COUNT times, half as runs (one from sketch 0, one up to n - 1), half
    as random subsets; twins; with `special` the rows of POOL_ROWS and ROUND_ROWS; pairs and single keys up to `records` records"""
    rng = np.random.default_rng(1000 * n + k)
    B = Builder(n, k)
    half = PER_HOLDER_COUNT // 2
    for h in sorted({min(h, n) for h in HOLDERS}):
        starts = np.array([0, n - h] + rng.integers(0, n - h + 1, half - 2).tolist())
        B.add(starts[:, None] + np.arange(h)[None, :])
        B.add(np.array([np.sort(rng.permutation(n)[:h]) for _ in range(half)]))
    # twins of the first run of 9 holders (sketches 0 .. 8), held by nine other sketches each
    g9 = sorted({min(h, n) for h in HOLDERS}).index(9) * PER_HOLDER_COUNT
    for word in ("mn", "lo", "hi") if k > 32 else ("mn", "lo"):
        B.twin(g9, word, np.sort(rng.permutation(np.arange(5, n))[:9]))
    if special:
        for s, longs in POOL_ROWS.items():
            at = dict((lane, h) for h, lane in longs)
            for lane in range(64):
                h = at.get(lane, SHORT[lane % len(SHORT)])
                others = PLAIN_FROM + rng.permutation(n - PLAIN_FROM)[:h - 1]
                B.add([np.sort(np.concatenate([[s], others]))], mn=64 * s + lane)
    # pairs and single keys thin out the long lists (a part holds what its keys' lists add up to) and bring the rows of
    # ROUND_ROWS to their counts
    have = B.keys_of_sketch()
    if special:
        for s, total in ROUND_ROWS.items():
            assert have[s] < total
            B.add(np.stack([np.full(total - have[s], s), rng.integers(PLAIN_FROM, n, total - have[s])], axis=1))
    left = max(0, records - int(B.keys_of_sketch().sum()))
    i = rng.integers(PLAIN_FROM, n - 1, left // 3)
    B.add(np.stack([i, rng.integers(i + 1, n)], axis=1))
    B.add(rng.integers(PLAIN_FROM, n, left // 3)[:, None])
    return B.finish()


@cached
def touch_one_copy():
    """8 256 sketches, so that the touched form keeps ONE copy of its counters: rows 0, 1, 2 share one key each with 1023, 1024,
    1025 later sketches, row 3 one with every later sketch, every other row has one or two cells"""
    n = 8256
    rng = np.random.default_rng(8256)
    B = Builder(n, 31)
    for r, count in ((0, 1023), (1, 1024), (2, 1025)):
        B.add(np.stack([np.full(count, r), 4 + np.sort(rng.permutation(n - 4)[:count])], axis=1))
    B.add(np.stack([np.full(n - 4, 3), np.arange(4, n)], axis=1))
    i = np.arange(4, n - 1)
    B.add(np.stack([i, i + 1], axis=1))
    i = np.arange(4, n - 3, 2)
    B.add(np.stack([i, i + 3], axis=1))
    return B.finish()


@cached
def touch_eight_copies():
    """1 100 sketches, eight copies of every counter: rows 0, 1, 2 have 127, 128, 129 partners, each sharing 8 consecutive keys of
    the row, one per copy; every other row but the last has one cell"""
    n = 1100
    rng = np.random.default_rng(1100)
    B = Builder(n, 31)
    for r, count in ((0, 127), (1, 128), (2, 129)):
        who = 3 + rng.permutation(n - 3)[:count]                                # (in no order: a column's eight keys lie anywhere in the row)
        B.add(np.stack([np.full(8 * count, r), np.repeat(who, 8)], axis=1), mn=10 + np.arange(8 * count))
    i = np.arange(3, n - 1)
    B.add(np.stack([i, i + 1], axis=1))
    return B.finish()


def straddle_lists(n):
    """holder lists around the column block boundary, cut to the sketches there are"""
    E = SPARSE_COLS
    lists = [range(E - 4, E + 7), range(E - 4, E), range(E - 1, E + 2), range(E, E + 7), range(E - 3, E + 3), [E - 4, E - 1, E, E + 6]]
    return [np.array([s for s in l if s < n]) for l in lists]


@cached
def blocks_input(n):
    """(i, i + 1) for every i; (0, 16383), (0, 16384), (16382, 16383), (16383, 16384), (16384, n - 1); lists across the block
    boundary; one key of 70 holders spread over all sketches: two to four keys per sketch but for a few"""
    E = SPARSE_COLS
    B = Builder(n, 31)
    i = np.arange(n - 1)
    B.add(np.stack([i, i + 1], axis=1))
    B.add([np.array(p) for p in ((0, E - 1), (0, E), (E - 2, E - 1), (E - 1, E), (E, n - 1)) if p[0] < p[1] < n])
    B.add([l for l in straddle_lists(n) if len(l) >= 2])
    high = np.unique(np.linspace(E, n - 1, 8).astype(np.int64)) if n > E else np.zeros(0, np.int64)
    low = np.arange(7, E - 1, (E - 8) // (69 - len(high)))[:69 - len(high)]
    B.add([np.concatenate([low, [E - 1], high])])
    return B.finish()


@cached
def half_input(L):
    """8 200 sketches (one copy of the counters where the touched form does not run): sketches 0, 4 and 5 hold the same L keys,
    sketch 6 the first 1 000 of them, the others a chain of pairs, two keys each"""
    n = 8200
    B = Builder(n, 31)
    g = np.arange(L)
    B.records(np.concatenate([np.tile(g, 3), g[:1000]]), np.concatenate([np.repeat([0, 4, 5], L), np.full(1000, 6)]), L,
              mn=np.where(g < 1000, 10, FIRST_MN + g % 3000))
    chain = np.array([1, 2, 3] + list(range(7, n)))
    B.add(np.stack([chain[:-1], chain[1:]], axis=1))
    B.add(np.array([[1], [n - 1]]))
    return B.finish()


LONG_LENGTHS = {10: 65537, 20: 98305}                                           # long row -> its key count; the others hold 65 536
# lists of up to 66 records fill 1 480 parts unevenly: with the keys numbered from 0 one part of each input runs over.  The keys are
# numbered from here instead (the fullest parts then hold 3 899 and 3 984 records; check_builder holds them to the capacity)
LONG_SALT = {64: 7 * 1000003, 65: 13 * 1000003}


@cached
def long_rows_input(R):
    """R long rows and 40 short ones, k = 63: long row r holds keys [1000 r, 1000 r + L_r), short sketch R + t the keys that are
    t modulo 500"""
    B = Builder(R + 40, 63, LONG_SALT[R])
    length = [LONG_LENGTHS.get(r, 65536) for r in range(R)]
    G = max(1000 * r + length[r] for r in range(R))
    key = [np.arange(1000 * r, 1000 * r + length[r]) for r in range(R)] + [np.arange(t, G, 500) for t in range(40)]
    B.records(np.concatenate(key), np.repeat(np.arange(R + 40), [len(x) for x in key]), G)
    return B.finish()


INPUTS = {
    "A-31": lambda: holders_input(200, 31), "A-63": lambda: holders_input(200, 63),
    "A'-127": lambda: holders_input(127, 31, False, 100_000), "A'-128": lambda: holders_input(128, 31, False, 100_000),
    "A'-129": lambda: holders_input(129, 31, False, 100_000), "A'-128-63": lambda: holders_input(128, 63, False, 100_000),
    "B-one": touch_one_copy, "B-eight": touch_eight_copies,
    "C-16384": lambda: blocks_input(16384), "C-16385": lambda: blocks_input(16385), "C-16448": lambda: blocks_input(16448),
    "D-65535": lambda: half_input(65535), "D-65536": lambda: half_input(65536),
    "D-64": lambda: long_rows_input(64), "D-65": lambda: long_rows_input(65),
}
HOLDER_INPUTS = [x for x in INPUTS if x[0] == "A"]
DIRECT = {"B-one": True, "B-eight": True, "C-16384": True, "C-16385": True, "C-16448": True, "D-65535": True,
          "D-65536": False, "D-64": False, "D-65": False}              # partition form: do the cells leave the row sums directly?
BETWEEN = "A'-129"                                                             # the smaller problem between the two runs of a B or D input


# ------------------------------------------------------------------------------------------------ not GPU

def test_the_pair_model_is_set_algebra():
    rng = np.random.default_rng(5)
    for trial in range(20):
        n, K = int(rng.integers(2, 12)), int(rng.integers(1, 40))
        holders = [np.sort(rng.permutation(n)[:rng.integers(1, n + 1)]) for _ in range(K)]
        if trial % 2:
            holders += holders[:5]                                              # keys with equal holder lists
        B = Builder(n, 63 if trial % 3 else 31)
        B.add(holders)
        P = B.finish()
        sets = [set() for _ in range(n)]
        for g, hs in enumerate(holders):
            for s in hs.tolist():
                sets[s].add(g)
        assert cell_dict(P.want) == {(i, j): len(sets[i] & sets[j]) for i in range(n) for j in range(i + 1, n) if sets[i] & sets[j]}, trial
        assert np.diff(P.off.astype(np.int64)).tolist() == [len(s) for s in sets] and strictly_sorted(P)
        assert sorted(P.want.tolist()) == P.want.tolist()
    # by hand: key 0 held by {0, 1, 2}, key 1 by {1, 2}, key 2 by {2}
    B = Builder(3, 31)
    B.add([[0, 1, 2], [1, 2], [2]])
    assert cell_dict(B.finish().want) == {(0, 1): 1, (0, 2): 1, (1, 2): 2}


def check_builder(P):
    """what every input must be: sorted, distinct keys, no part over its capacity"""
    assert strictly_sorted(P)
    words = np.stack([P.key_mn.astype(np.uint64), P.key_hi, P.key_lo], axis=1)
    assert len(np.unique(words, axis=0)) == P.K                                  # the key index IS the key: the model may count by it
    assert len(P.mn) == int(P.off[-1]) and len(P.off) == P.n + 1
    assert part_loads(P).max() <= PART_CAP, part_loads(P).max()
    if takes_small_form(P):
        assert part_loads(P, small=True).max() <= SMALL_CAP, part_loads(P, small=True).max()
    i, j, c = cells_of(P.want)
    assert (i < j).all() and (j < P.n).all() and (c > 0).all() and len(np.unique(P.want >> np.uint64(32))) == len(P.want)


@pytest.mark.parametrize("name", HOLDER_INPUTS)
def test_the_holder_inputs_hold_what_they_say(name):
    P = INPUTS[name]()
    check_builder(P)
    n, k, special = P.n, P.k, name in ("A-31", "A-63")
    hist = holder_histogram(P)
    counts = sorted({min(h, n) for h in HOLDERS})
    want = {h: PER_HOLDER_COUNT for h in counts}
    want[9] += 3 if k > 32 else 2                                               # the twins
    if special:
        for longs in POOL_ROWS.values():
            at = dict((lane, h) for h, lane in longs)
            for lane in range(64):
                h = at.get(lane, SHORT[lane % len(SHORT)])
                want[h] = want.get(h, 0) + 1
    for h in set(hist) | set(want):
        if h > 2:
            assert hist.get(h, 0) == want.get(h, 0), h
    assert hist[1] >= PER_HOLDER_COUNT and hist[2] >= PER_HOLDER_COUNT
    # runs: one from sketch 0 and one up to n - 1, of every count
    h_of_key = np.bincount(P.rec_key)
    first, last = np.full(P.K, n), np.zeros(P.K, np.int64)
    np.minimum.at(first, P.rec_key, P.rec_sk)
    np.maximum.at(last, P.rec_key, P.rec_sk)
    is_run = last - first + 1 == h_of_key
    for h in counts:
        assert (is_run & (h_of_key == h) & (first == 0)).any() and (is_run & (h_of_key == h) & (last == n - 1)).any(), h
        assert h < 3 or h > n - 3 or (~is_run & (h_of_key == h)).sum() >= PER_HOLDER_COUNT // 2 - 2, h
    # the twins differ from their key in one word, and in their holders
    assert [w for _, _, w in P.twins] == (["mn", "lo", "hi"] if k > 32 else ["mn", "lo"])
    for t, s, word in P.twins:
        same = [P.key_mn[t] == P.key_mn[s], P.key_lo[t] == P.key_lo[s], P.key_hi[t] == P.key_hi[s]]
        assert same == [word != "mn", word != "lo", word != "hi"]
        assert set(P.rec_sk[P.rec_key == t].tolist()) != set(P.rec_sk[P.rec_key == s].tolist()) and h_of_key[t] == h_of_key[s] == 9
    if special:
        for s, longs in POOL_ROWS.items():
            a = int(P.off[s])
            lanes = h_of_key[P.rec_key[a:a + 64]]                              # holder counts of the sketch's first 64 keys, in its order
            assert [(int(h), l) for l, h in enumerate(lanes) if h >= POOLED_FROM] == sorted(longs, key=lambda x: x[1]), s
            assert (P.mn[a:a + 64] < FIRST_MN).all() and P.mn[a + 64] >= FIRST_MN
        pooled = {s: sum(h >> 3 for h, _ in longs) for s, longs in POOL_ROWS.items()}
        assert pooled == {1: 5, 2: 4, 3: 127, 4: 128, 5: 129}
        assert {s: int(P.off[s + 1] - P.off[s]) for s in ROUND_ROWS} == ROUND_ROWS
    assert (n > SMALL_N or k > 32) == (not takes_small_form(P))
    print("%s: %d records, %d keys, %d cells, fullest part %d" % (name, len(P.mn), P.K, len(P.want), part_loads(P).max()))


def test_the_touch_inputs_touch_what_they_say():
    P = touch_one_copy()
    check_builder(P)
    n = P.n
    cols = (n + 63) & ~63
    assert 2 * cols * 2 > 32 * 1024 >= cols * 2                                 # one copy of 16-bit counters in the touched form's 32 KiB, not two
    per_row = partners(P.want, n)
    assert per_row[:4].tolist() == [1023, 1024, 1025, n - 4] and TOUCH_CAP == 1024
    assert set(per_row[4:n - 1].tolist()) == {1, 2} and per_row[n - 1] == 0
    assert np.diff(P.off.astype(np.int64))[:4].tolist() == [1023, 1024, 1025, n - 4] and len(P.mn) // n <= 2048
    assert set(cells_of(P.want)[2].tolist()) == {1}
    P = touch_eight_copies()
    check_builder(P)
    n = P.n
    cols = (n + 63) & ~63
    assert 16 * cols * 2 > 32 * 1024 >= 8 * cols * 2                            # eight copies
    per_row = partners(P.want, n)
    assert per_row[:3].tolist() == [127, 128, 129] and set(per_row[3:n - 1].tolist()) == {1}
    assert np.diff(P.off.astype(np.int64))[:3].tolist() == [8 * 127, 8 * 128, 8 * 129]
    i, j, c = cells_of(P.want)
    assert set(c[i < 3].tolist()) == {8} and set(c[i >= 3].tolist()) == {1}
    for r in range(3):                                                          # a partner's eight keys are consecutive in the row: one per copy
        a, z = int(P.off[r]), int(P.off[r + 1])
        partner = np.array([P.rec_sk[(P.rec_key == g) & (P.rec_sk != r)][0] for g in P.rec_key[a:z]])
        assert (partner.reshape(-1, 8) == partner.reshape(-1, 8)[:, :1]).all() and len(set(partner[::8].tolist())) == (z - a) // 8
    assert 8 * 127 < TOUCH_CAP == 8 * 128 < 8 * 129


@pytest.mark.parametrize("n", [16384, 16385, 16448])
def test_the_block_inputs_lie_across_the_column_blocks(n):
    P = blocks_input(n)
    check_builder(P)
    E = SPARSE_COLS
    cell = cell_dict(P.want)
    assert all((i, i + 1) in cell for i in range(n - 1))
    named = [(0, E - 1), (0, E), (E - 2, E - 1), (E - 1, E), (E, n - 1)]
    assert [p in cell for p in named] == [True, n > E, True, n > E, n > E + 1]
    assert cell[(E - 2, E - 1)] >= 2 and (n == E or cell[(E - 1, E)] >= 2)
    assert (-(-n // E) == 1) == (n == E)
    keys = np.diff(P.off.astype(np.int64))
    assert set(keys.tolist()) <= set(range(1, 13)) and ((keys < 2) | (keys > 4)).sum() <= 16 and keys[1] == 2
    hist = holder_histogram(P)
    assert hist[70] == 1 and max(hist) == 70
    the70 = np.sort(P.rec_sk[P.rec_key == np.flatnonzero(np.bincount(P.rec_key) == 70)[0]])
    assert the70[0] < 100 and the70[-1] == n - 1 and E - 1 in the70 and (the70 < E).sum() >= 62
    assert (the70 >= E).sum() == {16384: 0, 16385: 1, 16448: 8}[n]
    if n > E:
        rows = cells_of(P.want)
        assert {int(j) >= E for j in rows[1][rows[0] == E - 1]} == {True}       # row 16383: cells in the second block only
        assert (rows[0] >= E).any() == (n > E + 1)                              # rows that pass the first block by
        assert any(len(l) >= 2 and l[0] < E <= l[-1] for l in straddle_lists(n))


@pytest.mark.parametrize("L", [65535, 65536])
def test_the_half_inputs_fill_a_counter_word(L):
    P = half_input(L)
    check_builder(P)
    cell = cell_dict(P.want)
    assert [cell[p] for p in ((0, 4), (0, 5), (4, 5), (0, 6), (4, 6), (5, 6))] == [L, L, L, 1000, 1000, 1000]
    assert (L == 0xFFFF) == (L <= LONG_ROW) and 4 >> 1 == 5 >> 1                  # columns 4 and 5: the halves of one word
    keys = np.diff(P.off.astype(np.int64))
    assert keys[[0, 4, 5, 6]].tolist() == [L, L, L, 1000] and set(np.delete(keys, [0, 4, 5, 6]).tolist()) == {2}
    assert (keys > LONG_ROW).sum() == (3 if L > LONG_ROW else 0)
    a = int(P.off[0])
    assert set(P.rec_key[a:a + 1000].tolist()) == set(P.rec_key[int(P.off[6]):int(P.off[7])].tolist())     # sketch 6: the FIRST 1 000 keys of row 0
    assert P.n > SPARSE_COLS // 2                                                # more than 8 192 sketches: one copy of the counters in 64 KiB
    assert len(P.want) == 6 + P.n - 5


@pytest.mark.parametrize("R", [64, 65])
def test_the_long_row_inputs_have_that_many_long_rows(R):
    P = long_rows_input(R)
    check_builder(P)
    keys = np.diff(P.off.astype(np.int64))
    assert (keys > LONG_ROW).sum() == R and keys[:R].tolist() == [LONG_LENGTHS.get(r, 65536) for r in range(R)]
    assert keys[R:].max() < 400 and P.k == 63 and not takes_small_form(P)
    cell = cell_dict(P.want)
    assert cell[(0, 1)] == 64536 and cell[(0, R - 1)] == 65536 - 1000 * (R - 1) and cell[(10, 11)] == 64537 and cell[(20, 53)] == 98305 - 33000
    holders = np.bincount(P.rec_key)
    assert holders.max() == R + 1 and set(range(1, R + 2)) == set(holders.tolist())      # up to all R long rows and one short sketch
    assert cell[(0, R)] == len(np.arange(0, 65536, 500)) and cell[(R - 1, R + 39)] > 100
    assert 4.0e6 < len(P.mn) < 4.6e6


# ---------------------------------------------------------------------------------------------------- GPU

def upload(P):
    """-> torch tensors on the device, each padded by 64 bytes; the caller keeps them alive"""
    import torch
    out = []
    for a, dt, view in ((P.mn, np.uint32, np.int32), (P.lo, np.uint64, np.int64), (P.hi, np.uint64, np.int64)):
        if a is None:
            out.append(None)
            continue
        a = np.ascontiguousarray(a, dtype=dt)
        out.append(torch.from_numpy(np.concatenate([a, np.zeros(64 // a.itemsize, dt)]).view(view)).cuda())
    torch.cuda.synchronize()
    return out


def ptr(t):
    return t.data_ptr() if t is not None else None


def explain(got, want):
    g, w = cell_dict(got), cell_dict(want)
    diff = [(p[0], p[1], g.get(p), w.get(p)) for p in sorted(set(g) | set(w)) if g.get(p) != w.get(p)]
    return "%d cells differ of %d expected, %d returned; (row, column, got, expected): %s" % (len(diff), len(w), len(g), diff[:16])


def compare_on_gpu(ctx, P, tag):
    """the cells call and the dense call on one input, both held to the model -> did the cells leave the row sums directly?"""
    import torch
    d = upload(P)
    n, want = P.n, P.want
    # as cells
    scratch = torch.full((n * n,), SENTINEL, dtype=torch.int32, device="cuda")
    room = torch.zeros(len(want) + 4096, dtype=torch.int64, device="cuda")
    cnt = ctx.compare_cells_device(P.k, ptr(d[0]), ptr(d[1]), ptr(d[2]), P.off, n, scratch.data_ptr(), room.data_ptr(), room.numel())
    got = np.sort(room[:cnt].cpu().numpy().view(np.uint64))
    assert len(np.unique(got >> np.uint64(32))) == len(got), "%s: a pair comes twice among the cells" % tag
    assert np.array_equal(got, want), "%s, cells: %s" % (tag, explain(got, want))
    direct = not bool((scratch != SENTINEL).any())
    del scratch, room
    # dense, checked on the device: as many non-zero cells as expected, and the expected cells
    inter = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    ctx.compare_device(P.k, ptr(d[0]), ptr(d[1]), ptr(d[2]), P.off, n, 0, 1, inter.data_ptr())
    torch.cuda.synchronize()
    i, j, c = (torch.from_numpy(x).cuda() for x in cells_of(want))
    at = inter[i, j].to(torch.int64)
    if int(torch.count_nonzero(inter)) != len(want) or not torch.equal(at, c):
        nz = torch.nonzero(inter).cpu().numpy().astype(np.uint64)
        vals = inter[inter != 0].cpu().numpy().astype(np.uint64)
        dense = np.sort((nz[:, 0] << np.uint64(48)) | (nz[:, 1] << np.uint64(32)) | vals)
        raise AssertionError("%s, dense: %s" % (tag, explain(dense, want)))
    return direct


def compare_on_host_arrays(ctx, P, tag):
    """spsp_compare (host arrays in, whole matrix and key counts out): the key counts are the sketches'"""
    sk = [sp.Sketch(P.k, 11, P.mn[a:z].copy(), P.lo[a:z].copy(), (P.hi[a:z].copy() if P.hi is not None else np.zeros(z - a, np.uint64)))
          for a, z in zip(P.off[:-1].astype(np.int64).tolist(), P.off[1:].astype(np.int64).tolist())]
    inter, card = ctx.compare(sk)
    assert card.tolist() == np.diff(P.off.astype(np.int64)).tolist(), tag
    i, j, c = cells_of(P.want)
    dense = np.zeros((P.n, P.n), np.uint32)
    dense[i, j] = c
    assert np.array_equal(inter, dense), "%s, spsp_compare" % tag


def run_input(ctx, name):
    """an input twice on one context -- for B and D with a smaller problem in between (the touched form and the long rows' launches
    reuse buffers)"""
    P = INPUTS[name]()
    t0 = time.perf_counter()
    sys.stderr.write("input %s\n" % name)
    sys.stderr.flush()
    direct = [compare_on_gpu(ctx, P, name + ", first run")]
    if name[0] in "BD":
        compare_on_gpu(ctx, INPUTS[BETWEEN](), name + ", the smaller problem in between")
    direct.append(compare_on_gpu(ctx, P, name + ", second run"))
    if name[0] == "A":
        compare_on_host_arrays(ctx, P, name)
    if name in DIRECT and not os.environ.get("SPSP_DEBUG_SPARSE"):
        assert direct == [DIRECT[name]] * 2, (name, direct)
    print("%s: %d sketches, %d records, %d cells: %.2f s on the GPU side" % (name, P.n, len(P.mn), len(P.want), time.perf_counter() - t0))


def child(names):
    """body of a child process: its hook settings are in the environment"""
    with sp.Context(0) as ctx:
        for name in names:
            run_input(ctx, name)
    print("ok")


def forms_in(trace):
    """stderr of a child -> {input: [form of each partition-form comparison]}, and no word of a spill"""
    assert "spsp spill:" not in trace and "spill yes" not in trace, trace[-3000:]
    forms, name = {}, None
    for line in trace.splitlines():
        if line.startswith("input "):
            name = line[6:]
            forms[name] = []
        elif line.startswith("spsp compare:") and name:
            forms[name].append(line.split(" sketches, ")[1].split(" form")[0])
    return forms


ALL = list(INPUTS)
# (no SPSP_DEBUG_ACC_TOUCH for the inputs of 64 and 65 long rows: no cells leave their row sums, the hook has nothing to choose)
SETTINGS = [
    ({}, ALL),
    ({"SPSP_DEBUG_ACC_TOUCH": "0"}, [x for x in ALL if x not in ("D-64", "D-65")]),
    ({"SPSP_DEBUG_ACC_TOUCH": "s"}, [x for x in ALL if x not in ("D-64", "D-65")]),
    ({"SPSP_DEBUG_MULTI": "0"}, ALL),
    ({"SPSP_DEBUG_MULTI": "1"}, ALL),
    ({"SPSP_DEBUG_SPARSE": "1"}, HOLDER_INPUTS),
    ({"SPSP_DEBUG_SMALL": "0"}, [x for x in HOLDER_INPUTS if x[1] == "'"]),
]


@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_the_row_sums_on_a_seam(ctx, name):
    run_input(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("env,names", SETTINGS, ids=["-".join("%s=%s" % (k[11:], v) for k, v in e.items()) or "default" for e, _ in SETTINGS])
def test_the_row_sums_on_every_seam_under_a_hook(env, names):
    """one child process per hook setting (the hooks are read once per process), every input the setting applies to, each held
    to the model exactly; the trace says which form ran"""
    code = ("import sys\nsys.path.insert(0, %r); sys.path.insert(0, %r)\nimport torch\nimport test_compare_seams as t\nt.child(sys.argv[1:])\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", code] + names, env=dict(os.environ, SPSP_DEBUG_SPILL_TRACE="1", **env), capture_output=True, text=True,
                       timeout=900)
    print("%s: %d inputs in %.1f s of wall time\n%s" % (env or "default", len(names), time.perf_counter() - t0, r.stdout[-3000:]))
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (env, r.stdout[-2000:], r.stderr[-4000:])
    forms = forms_in(r.stderr)
    assert list(forms) == names
    for name in names:
        P = INPUTS[name]()
        if "SPSP_DEBUG_SPARSE" in env:
            assert forms[name] == [], (name, forms[name])                       # the global dictionary's lists: no partition form ran
        elif takes_small_form(P) and "SPSP_DEBUG_SMALL" not in env:
            assert forms[name] and set(forms[name]) == {"small"}, (name, forms[name])
        else:
            assert forms[name] and set(forms[name]) == {"partition"}, (name, forms[name])
