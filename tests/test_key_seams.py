"""Downsample and gather at their seams (include/spsp.h: spsp_keys_downsample_device, spsp_gather_device), on hand-built keys.

Both stages cut the comparator's key arrays at fixed places whatever the sketches are: the downsampling pass into tiles of
2048 keys and ballot words of 64, gather into reference tiles of 2048 and waves of 64, a pick that strides 1024 lanes over the
references, rounds queued in batches of 32, 64, 128, and both lean on a scan that changes form above 32 768 counts.  Keys
that come out of real sketches meet those places by luck; the keys below are built to put a boundary, a survivor or a match
on each of them.

The minimizers come from two pools, one whose XXH64 (seed 1312) is <= T and one whose hash is > T, so a test prescribes the
keep mask bit by bit; kmer_lo is a mixed function of the position and kmer_hi its complement, so a copy that takes the wrong
array or the wrong index shows.  Expected values: a numpy mask model (ds_model) and Python set algebra (gather_model, held to
tests/test_gather.py's model).  Integers only, no tolerance anywhere.

What a wrong kernel would look like, and where it shows:
    an offset that forgets the bits of a partial word, or takes the total from the last tile: boundaries on 1, 63, 65, 2047,
        2049 and totals of exactly 2048, 4096, 6144 keys
    `<` for `<=` at the threshold: the first kept key of every mask carries the minimizer whose hash equals T
    a search ordered (minimizer, lo, hi): order_input(), and every k = 63 input (hi falls where lo rises)
    a tie that goes to the highest index, or to whichever lane arrives first: ties_input() and the chains, whose later
        rounds are all ties
    a stop at u == min_keys: stop_input() and the chains' rounds of one key
    a block-form scan without its block offsets: 32 769 tiles, 32 819 cells, 40 000 query keys
    rows of a batch read back with the wrong stride per query: chains_input()"""
import functools
import time

import numpy as np
import pytest

import supersampler_amd as sp
from oracle import oracle_py as orc

M = 11                                          # every minimizer below lies under 4**M
TILE, WORD = 2048, 64                           # keys per workgroup and per ballot word, in both stages
SCAN_ONE_KERNEL = 4 * 8192                      # launch_scan_u32: more counts than this are scanned in blocks of 8192
GOLD = 0x9E3779B97F4A7C15
U64 = (1 << 64) - 1
SEAMS = (0, 1, 63, 64, 65, 2047, 2048, 2049)

cached = functools.lru_cache(maxsize=None)


def mixed(i):
    """positions -> 64-bit words that are neither the position nor near their neighbours' words (the product wraps)"""
    return (np.asarray(i, dtype=np.uint64) + np.uint64(1)) * np.uint64(GOLD)


def upload(mn, lo, hi=None):
    """numpy key arrays -> torch tensors on the device, each padded by 64 bytes; the caller keeps them alive"""
    import torch
    out = []
    for a, dt, view in ((mn, np.uint32, np.int32), (lo, np.uint64, np.int64), (hi, np.uint64, np.int64)):
        if a is None:
            out.append(None)
            continue
        a = np.ascontiguousarray(a, dtype=dt)
        out.append(torch.from_numpy(np.concatenate([a, np.zeros(64 // a.itemsize, dt)]).view(view)).cuda())
    torch.cuda.synchronize()
    return out


def ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------------------------------ downsample: model and keys

def keep_table(values, threshold):
    """-> bool per value: xxh64(value) <= threshold, the hash taken once per distinct minimizer"""
    distinct, inverse = np.unique(np.asarray(values, dtype=np.uint32), return_inverse=True)
    keep = np.array([orc.xxh64(int(v)) <= threshold for v in distinct], dtype=bool)
    return keep[inverse.reshape(-1)] if len(distinct) else np.zeros(0, bool)


def ds_model(mn, lo, hi, off, T):
    """-> (mn, lo, hi or None, new offsets) of the keys in [off[0], off[-1]) whose minimizer passes T, order kept"""
    off = np.asarray(off, dtype=np.int64)
    a, z = int(off[0]), int(off[-1])
    mask = keep_table(mn[a:z], T)
    in_front = np.concatenate([[0], np.cumsum(mask)])                       # survivors in front of position i; 0 for position 0
    return mn[a:z][mask], lo[a:z][mask], (hi[a:z][mask] if hi is not None else None), in_front[off - a].astype(np.uint64)


@cached
def pools():
    """-> (T, kept, dropped): 512 minimizers below 4**M split at their median hash T; every hash of `kept` is <= T and
    kept[0] is the one whose hash IS T; every hash of `dropped` is > T"""
    vals = (np.arange(1, 513, dtype=np.uint64) * np.uint64(8191) % np.uint64(4 ** M)).astype(np.uint32)
    assert len(set(vals.tolist())) == 512
    h = np.array([orc.xxh64(int(v)) for v in vals], dtype=np.uint64)
    T = int(np.sort(h)[256])
    kept = np.concatenate([vals[h == T], vals[h < T]])
    return T, kept, vals[h > T]


@cached
def bands():
    """-> (the 512 minimizers of pools(), T1 > T2 > T3): the three quartiles of their hashes"""
    _, kept, dropped = pools()
    vals = np.concatenate([kept, dropped])
    h = np.sort(np.array([orc.xxh64(int(v)) for v in vals], dtype=np.uint64))
    return vals, int(h[384]), int(h[256]), int(h[128])


def ds_keys(mask, k, lead=0):
    """-> (mn, lo, hi or None) of lead + len(mask) keys whose keep bits under pools()' T are `lead` ones, then `mask`.  The
    kept minimizers cycle through the pool by their rank among the kept, so the first kept key carries the hash equal to T"""
    _, kept, dropped = pools()
    full = np.concatenate([np.ones(lead, bool), np.asarray(mask, dtype=bool)])
    i = np.arange(len(full))
    rank = np.cumsum(full) - full
    mn = np.where(full, kept[rank % len(kept)], dropped[i % len(dropped)]).astype(np.uint32)
    lo = mixed(i)
    return mn, lo, (~lo if k > 32 else None)


def seam_offsets(R):
    """a boundary at every seam value <= R and at R - 1 and R, each twice: runs of sketches without keys on every seam, the
    first and the last sketch among them"""
    vals = sorted({v for v in SEAMS + (R - 1, R) if 0 <= v <= R})
    return np.repeat(np.array(vals, dtype=np.uint64), 2)


def word_offsets(R):
    """boundaries at 64 j and 64 j + 1 for a few j: on a word's first bit and one bit into it, in every tile"""
    inner = [64 * j + d for j in (1, 31, 32, 33, 95) for d in (0, 1)]
    assert inner == sorted(inner) and inner[-1] < R
    return np.array([0] + inner + [R], dtype=np.uint64)


def prescribed_masks(R):
    i = np.arange(R)
    last_of_its_tile = np.minimum((i // TILE + 1) * TILE, R) - 1
    return {
        "all kept": np.ones(R, bool),
        "none kept": np.zeros(R, bool),
        "bit 0 of every word": i % WORD == 0,
        "bit 63 of every word": i % WORD == WORD - 1,
        "every other word full": (i // WORD) % 2 == 0,
        "the last key of each tile": i == last_of_its_tile,
        "the first key of each tile": i % TILE == 0,
        "one survivor, at R - 1": i == R - 1,
    }


def mask_words(mask):
    """the keep mask as the kernels hold it: bit l of word j is key 64 j + l"""
    bits = np.concatenate([np.asarray(mask, dtype=np.uint8), np.zeros(-len(mask) % WORD, np.uint8)])
    return np.packbits(bits, bitorder="little").view("<u8")


# ------------------------------------------------------------------------------------------ gather: model and keys

def gather_model(sets_q, sets_r, min_keys, max_rounds=0):
    """the rule in the header of spsp_gather.hip over Python sets of (mn, hi, lo) -> [(query, rank, match, intersect, unique,
    remaining)] ordered by (query, rank); match counts from the first sketch of the list, as the rows do"""
    assert min_keys >= 1
    rows = []
    for q, Q in enumerate(sets_q):
        alive, rank = set(Q), 0
        while True:
            rank += 1
            best_u, best_j = 0, None
            for j, R in enumerate(sets_r):
                u = len(R & alive)
                if u > best_u:                                              # (strictly: the smallest j among the largest)
                    best_u, best_j = u, j
            if best_u < min_keys or (max_rounds > 0 and rank > max_rounds):
                break
            rows.append((q, rank, len(sets_q) + best_j, len(sets_r[best_j] & Q), best_u, len(alive) - best_u))
            alive -= sets_r[best_j]
    return rows


def keys_of(ids, k):
    """distinct ids -> distinct (mn, hi, lo) keys over seven minimizers: lo mixed from the id, hi its complement (0 at k <= 32)"""
    ids = np.asarray(list(ids), dtype=np.uint64)
    lo = mixed(ids)
    hi = ~lo if k > 32 else np.zeros(len(ids), np.uint64)
    return list(zip((1000 + ids % np.uint64(7)).tolist(), hi.tolist(), lo.tolist()))


def pack(sketches, lead=()):
    """sketches: lists of (mn, hi, lo) in the order given (the caller sorts) -> (mn, lo, hi, off); `lead`: keys that lie in
    front of off[0] and belong to no sketch"""
    flat, off = list(lead), [len(lead)]
    for s in sketches:
        flat += s
        off.append(len(flat))
    cols = list(zip(*flat)) if flat else ([], [], [])
    return np.array(cols[0], dtype=np.uint32), np.array(cols[2], dtype=np.uint64), np.array(cols[1], dtype=np.uint64), np.array(off, dtype=np.uint64)


def as_tuples(rows):
    assert not np.any(rows["reserved"])
    return [tuple(int(r[f]) for f in ("query", "rank", "match", "intersect", "unique", "remaining")) for r in rows]


def want_rows(sketches, nq, min_keys=1, max_rounds=0):
    return gather_model([set(s) for s in sketches[:nq]], [set(s) for s in sketches[nq:]], min_keys, max_rounds)


def gpu_rows(ctx, k, sketches, nq, min_keys=1, max_rounds=0, lead=()):
    mn, lo, hi, off = pack(sketches, lead)
    assert k > 32 or not hi.any()
    d = upload(mn, lo, hi if k > 32 else None)
    return as_tuples(ctx.gather_device(k, ptr(d[0]), ptr(d[1]), ptr(d[2]), off, len(sketches), nq, min_keys, max_rounds))


def strictly_increasing(sketch):
    return all(a < b for a, b in zip(sketch, sketch[1:]))


@cached
def order_input():
    """k = 63, one query over two neighbouring minimizers and every pair of six hi and six lo values; the references hold keys
    equal in lo and different in hi, equal in hi and different in lo, the same (hi, lo) under the other minimizer, and three
    kinds of near misses the query does not hold"""
    H = (1, 2, 3, 1 << 32, (1 << 61) + 1, (1 << 62) - 1)
    L = (0, 5, 7, 1 << 31, 1 << 63, U64)
    MN = 77
    grid = lambda mn, hs=H, ls=L: [(mn, h, l) for h in hs for l in ls]
    Q = sorted(grid(MN) + grid(MN + 1))
    refs = [
        sorted((MN, h, L[3]) for h in H),                                   # one lo under every hi
        sorted((MN, H[4], l) for l in L),                                   # one hi over every lo
        sorted(grid(MN + 1, H[::2], L[1::2])),                              # (hi, lo) pairs of the first two, under the other minimizer
        sorted((MN, l, h) for h in H for l in L),                           # hi and lo exchanged: not in the query
        sorted(grid(MN - 1) + grid(MN + 2)),                                # the query's (hi, lo) under minimizers it lacks
        sorted(grid(MN, H[:3]) + [(MN, H[5], L[5] - 1), (MN + 1, H[0] + 3, L[0])]),
    ]
    return [Q] + refs


@cached
def waves_input(k):
    """-> (sketches, matched): one query against nine references of 2 * 2048 + 1 keys in all.  Reference entry e (lane e % 64
    of wave e // 64 of tile e // 2048) is held by the query iff e is in `matched`"""
    n = 2 * TILE + 1
    e = np.arange(n, dtype=np.uint64)
    inc = ((e + np.uint64(1)) << np.uint64(20)) | (mixed(e) & np.uint64(0xfffff))   # increasing with e, low bits mixed
    mn = (500 + e // np.uint64(700)).tolist()
    hi, lo = (inc.tolist(), (~inc).tolist()) if k > 32 else ([0] * n, inc.tolist())
    keys = list(zip(mn, hi, lo))
    matched = [0, 63]                                                       # lanes 0 and 63 of a wave and no other
    matched += [5 * WORD + 17]                                              # exactly one lane of a wave
    matched += list(range(9 * WORD, 10 * WORD))                             # a full wave
    matched += [TILE + 3 * WORD, TILE + 3 * WORD + 63, TILE + 8 * WORD + 31]
    matched += list(range(2 * TILE - WORD, 2 * TILE))                       # the last wave of the second tile, full
    matched += [2 * TILE]                                                   # the single key of the ragged last tile
    held = set(matched)
    # what the query holds besides: keys below and above every reference key, and neighbours (lo + 1 or lo - 1) of unmatched ones
    extra = [(499, 0, 5), (900, 0, 5)] + [(keys[x][0], keys[x][1], keys[x][2] ^ 1) for x in range(1, n, 97) if x not in held]
    bounds = [0, 0, 700, 700, TILE, TILE, TILE, 3000, n, n]                 # no keys before, between and after; a boundary on 2048
    refs = [keys[a:z] for a, z in zip(bounds, bounds[1:])]
    return [sorted([keys[x] for x in matched] + extra)] + refs, matched


@cached
def cells_input():
    """37 queries x 887 references of 0 .. 5 keys out of 150: 32 819 cells"""
    rng = np.random.default_rng(61)
    universe = keys_of(range(150), 63)
    sizes = rng.integers(0, 6, 37 + 887)
    sizes[[0, 36, 37, 37 + 886]] = [0, 5, 0, 5]                             # an empty first query and first reference, a full last of each
    return [sorted(universe[i] for i in rng.permutation(150)[:s]) for s in sizes]


@cached
def long_query_input():
    """one query of 40 000 keys; 20 references of 1 500 .. 3 400 of them and 300 keys of their own each"""
    rng = np.random.default_rng(62)
    q = keys_of(range(40_000), 31)
    other = keys_of(range(50_000, 60_000), 31)
    refs = [sorted([q[i] for i in rng.permutation(40_000)[:1500 + 100 * j]] + [other[i] for i in rng.permutation(10_000)[:300]]) for j in range(20)]
    return [sorted(q)] + refs


@cached
def edge_room_input():
    """one query of 40 000 keys, key i held by references i % 6, (i + 1) % 6 and (i + 3) % 6: 120 000 edges"""
    q = keys_of(range(40_000), 31)
    refs = [[] for _ in range(6)]
    for i, key in enumerate(q):
        for j in {i % 6, (i + 1) % 6, (i + 3) % 6}:
            refs[j].append(key)
    return [sorted(q)] + [sorted(r) for r in refs]


def ties_input(nr, variant):
    """-> (sketches, the winner): one query of six keys; every reference holds the same three of them.  "all": nothing else.
    "three": references 1023, 1024 and 2048 (those that exist) hold a fourth.  "last": those and reference nr - 1 hold the
    fourth, and nr - 1 alone a fifth: the last reference alone is the largest, which is reference 2048 at nr = 2049, and at
    nr = 1024 and 1025 the last lane of the pick's first stride and the first lane of its second"""
    key = keys_of(range(6), 31)
    refs = [sorted(key[:3]) for _ in range(nr)]
    more = [j for j in (1023, 1024, 2048) if j < nr]
    if variant in ("three", "last"):
        for j in more:
            refs[j] = sorted(key[:4])
    if variant == "last":
        refs[nr - 1] = sorted(key[:5])
    return [sorted(key)] + refs, {"all": 0, "three": 1023, "last": nr - 1}[variant]


def chain_input(length):
    """a query of length + 4 keys; reference j holds three keys all references hold and key j of its own: the first round names
    reference 0 with four keys, every later round the next reference with one"""
    key = keys_of(range(length + 4), 63)
    return [sorted(key)] + [sorted(key[:3] + [key[3 + j]]) for j in range(length)]


def chains_input(lengths):
    """one query per length L, the first L + 3 keys of chain_input(max(lengths)), against that chain's references: query q is
    named L rows, the first of four keys and the others of one, and stops in round L + 1 whatever the other queries do"""
    sk = chain_input(max(lengths))
    return [sorted(keys_of(range(L + 3), 63)) for L in lengths] + sk[1:]


CHAINS = ((5, 100), (100, 5), (40, 100, 230), (97, 225, 33, 64))


def stop_input():
    """references of 5, 3, 3 and 2 keys of a 14-key query; the third shares one key with the first"""
    key = keys_of(range(14), 31)
    return [sorted(key)] + [sorted(key[0:5]), sorted(key[5:8]), sorted([key[4]] + key[8:10]), sorted(key[10:12])]


# ------------------------------------------------------------------------------------------------ not GPU

def test_the_models_on_hand_made_cases():
    T, kept, dropped = pools()
    mn = np.array([kept[0], dropped[0], kept[1], kept[2], dropped[1]], dtype=np.uint32)
    lo = np.array([10, 11, 12, 13, 14], dtype=np.uint64)
    w_mn, w_lo, w_hi, w_off = ds_model(mn, lo, ~lo, [0, 2, 2, 5], T)
    assert w_mn.tolist() == [kept[0], kept[1], kept[2]] and w_lo.tolist() == [10, 12, 13] and w_hi.tolist() == (~lo[[0, 2, 3]]).tolist()
    assert w_off.tolist() == [0, 1, 1, 3]
    w_mn, w_lo, w_hi, w_off = ds_model(mn, lo, None, [1, 2, 5], T)          # off[0] != 0: the first key is nobody's
    assert w_lo.tolist() == [12, 13] and w_hi is None and w_off.tolist() == [0, 0, 2]
    assert ds_model(mn, lo, None, [0, 5], 0)[3].tolist() == [0, 0] and ds_model(mn, lo, None, [0, 5], U64)[3].tolist() == [0, 5]
    K = lambda *xs: {(x, 0, x) for x in xs}
    assert gather_model([K(1, 2, 3, 4)], [K(1, 2, 3), K(2, 3, 4)], 1) == [(0, 1, 1, 3, 3, 1), (0, 2, 2, 3, 1, 0)]
    assert gather_model([K(1, 2), K(7, 8, 9)], [K(9), K(1, 2, 7, 8)], 2) == [(0, 1, 3, 2, 2, 0), (1, 1, 3, 2, 2, 1)]
    assert gather_model([K(7, 8, 9)], [K(9), K(1, 2, 7, 8)], 1, 1) == [(0, 1, 2, 2, 2, 1)]


def test_the_gather_model_is_the_model_of_test_gather():
    """one definition of the rule: test_gather's hand-made cases, with the rows they expect, and random sets"""
    import test_gather as tg
    K = lambda *xs: {(x, 0, x) for x in xs}
    Q = K(*range(10))
    Rs = [K(0, 1, 2, 3, 4, 5), K(4, 5, 6, 7, 99), K(0, 1)]
    hand = [
        (K(1, 2, 3, 4), [K(1, 2, 3), K(2, 3, 4)], 1, 0, [(1, 0, 3, 3, 1), (2, 1, 3, 1, 0)]),
        (K(1, 2, 3, 4), [K(2, 3, 4), K(1, 2, 3)], 1, 0, [(1, 0, 3, 3, 1), (2, 1, 3, 1, 0)]),
        (Q, Rs, 1, 0, [(1, 0, 6, 6, 4), (2, 1, 4, 2, 2)]),
        (Q, Rs, 3, 0, [(1, 0, 6, 6, 4)]),
        (Q, [K(0, 1, 2, 3), K(8, 9), K(3, 4, 5, 6)], 3, 0, [(1, 0, 4, 4, 6), (2, 2, 4, 3, 3)]),
        (Q, Rs, 1, 1, [(1, 0, 6, 6, 4)]),
        (Q, Rs, 1, 5, [(1, 0, 6, 6, 4), (2, 1, 4, 2, 2)]),
        (set(), Rs, 1, 0, []),
        (Q, [], 1, 0, []),
        (K(1, 2), [K(1, 2), K(1, 2)], 1, 0, [(1, 0, 2, 2, 0)]),
    ]
    for q, rs, min_keys, max_rounds, want in hand:
        assert tg.gather_model(q, rs, min_keys, max_rounds) == want
        assert gather_model([q], rs, min_keys, max_rounds) == [(0, r, 1 + j, a, u, left) for r, j, a, u, left in want]
    rng = np.random.default_rng(60)
    for trial in range(60):
        sets = [set((int(x), 0, int(x)) for x in rng.integers(0, 40, rng.integers(0, 12))) for _ in range(int(rng.integers(3, 12)))]
        nq = int(rng.integers(1, 3))
        min_keys, max_rounds = int(rng.integers(1, 4)), int(rng.integers(0, 4))
        want = []
        for q in range(nq):
            want += [(q, r, nq + j, a, u, left) for r, j, a, u, left in tg.gather_model(sets[q], sets[nq:], min_keys, max_rounds)]
        assert gather_model(sets[:nq], sets[nq:], min_keys, max_rounds) == want, trial


def test_the_pools_lie_on_both_sides_of_a_hash_that_is_met():
    T, kept, dropped = pools()
    assert len(kept) == 257 and len(dropped) == 255 and max(kept.max(), dropped.max()) < 4 ** M
    assert orc.xxh64(int(kept[0])) == T                                     # `<=` against `<` shows on this minimizer
    assert keep_table(kept, T).all() and not keep_table(dropped, T).any()
    assert not keep_table(kept[:1], T - 1).any()
    vals, t1, t2, t3 = bands()
    assert [int(keep_table(vals, t).sum()) for t in (t1, t2, t3)] == [385, 257, 129]


@pytest.mark.parametrize("R", [3 * TILE, 3 * TILE - 1])
def test_the_prescribed_masks_are_what_they_are_called(R):
    T, kept, _ = pools()
    masks = prescribed_masks(R)
    assert len(masks) == 8
    n_words, n_tiles = -(-R // WORD), -(-R // TILE)
    ragged = (1 << (R % WORD)) - 1 if R % WORD else U64                     # the bits of the last word that are keys
    for name, mask in masks.items():
        mn, lo, hi = ds_keys(mask, 63)
        assert np.array_equal(keep_table(mn, T), mask), name                # the keys carry the mask
        assert not mask.any() or mn[np.argmax(mask)] == kept[0], name
        assert len(set(lo.tolist())) == R and np.array_equal(hi, ~lo) and not np.array_equal(lo, np.arange(R))
    w = {name: mask_words(mask).tolist() for name, mask in masks.items()}
    assert all(len(x) == n_words for x in w.values())
    assert w["all kept"] == [U64] * (n_words - 1) + [ragged] and w["none kept"] == [0] * n_words
    assert w["bit 0 of every word"] == [1] * n_words
    assert w["bit 63 of every word"] == [1 << 63] * (n_words - 1) + [(1 << 63) & ragged]
    assert w["every other word full"] == [U64 if j % 2 == 0 else 0 for j in range(n_words - 1)] + [ragged if (n_words - 1) % 2 == 0 else 0]
    assert np.flatnonzero(masks["the last key of each tile"]).tolist() == [min((t + 1) * TILE, R) - 1 for t in range(n_tiles)]
    assert np.flatnonzero(masks["the first key of each tile"]).tolist() == [t * TILE for t in range(n_tiles)]
    assert np.flatnonzero(masks["one survivor, at R - 1"]).tolist() == [R - 1]
    off = word_offsets(R).tolist()
    assert {64, 65, 31 * 64, 31 * 64 + 1, TILE, TILE + 1, 2 * TILE + 31 * 64} <= set(off) and off[0] == 0 and off[-1] == R


def test_the_seam_offsets_lie_on_the_seams():
    for R in (1, 63, 64, 65, 2047, 2048, 2049, 4096, 3 * TILE + 1):
        off = seam_offsets(R).tolist()
        assert off == sorted(off) and off[:2] == [0, 0] and off[-2:] == [R, R] and R - 1 in off
        assert set(off) == {v for v in SEAMS if v <= R} | {R - 1, R}
        assert all(off.count(v) == 2 for v in set(off))                     # a sketch without keys on every boundary


def test_the_search_order_input_tells_the_two_orders_apart():
    sk = order_input()
    Q = sk[0]
    assert all(strictly_increasing(s) for s in sk)
    assert Q != sorted(Q, key=lambda t: (t[0], t[2], t[1]))                 # (mn, hi, lo) is not (mn, lo, hi) on these keys
    same_lo = [(a, b) for a in Q for b in Q if a[0] == b[0] and a[2] == b[2] and a[1] != b[1]]
    same_hi = [(a, b) for a in Q for b in Q if a[0] == b[0] and a[1] == b[1] and a[2] != b[2]]
    other_mn = [(a, b) for a in Q for b in Q if a[0] != b[0] and a[1:] == b[1:]]
    assert same_lo and same_hi and other_mn
    assert len({t[2] for t in sk[1]}) == 1 and len({t[1] for t in sk[1]}) == 6 and set(sk[1]) <= set(Q)
    assert len({t[1] for t in sk[2]}) == 1 and len({t[2] for t in sk[2]}) == 6 and set(sk[2]) <= set(Q)
    assert set(sk[3]) <= set(Q) and {t[0] for t in sk[3]} == {78} and {t[1:] for t in sk[3]} & {t[1:] for t in sk[1] + sk[2]}
    assert not set(sk[4]) & set(Q) and not set(sk[5]) & set(Q)
    rows = want_rows(sk, 1)
    assert [r[2] for r in rows] == [6, 3, 2, 1] and [r[3] for r in rows] == [18, 9, 6, 6] and [r[4] for r in rows] == [18, 9, 6, 2]


@pytest.mark.parametrize("k", [31, 63])
def test_the_waves_input_matches_where_it_says(k):
    sk, matched = waves_input(k)
    flat = [key for s in sk[1:] for key in s]
    assert len(flat) == 2 * TILE + 1 and strictly_increasing(flat) and strictly_increasing(sk[0])
    assert [e for e, key in enumerate(flat) if key in set(sk[0])] == sorted(matched)
    lanes = {}
    for e in matched:
        lanes.setdefault(e // WORD, []).append(e % WORD)
    assert lanes[0] == [0, 63] and lanes[5] == [17] and lanes[9] == list(range(64))
    assert lanes[32 + 3] == [0, 63] and lanes[32 + 8] == [31] and lanes[63] == list(range(64)) and lanes[64] == [0] and len(lanes) == 7
    sizes = [len(s) for s in sk[1:]]
    assert sizes == [0, 700, 0, 1348, 0, 0, 952, 1097, 0] and sum(sizes[:4]) == TILE       # a boundary exactly on entry 2048
    assert [r[2:5] for r in want_rows(sk, 1)] == [(2, 67, 67), (8, 65, 65), (7, 3, 3)]
    assert (k > 32) == any(key[1] for key in flat)


def test_the_block_scan_inputs_take_the_block_form():
    sk = cells_input()
    nq, nr = 37, 887
    assert len(sk) == nq + nr and nq * nr == 32_819 > SCAN_ONE_KERNEL and (nq * nr) % 8192 == 51
    assert {len(s) for s in sk} == {0, 1, 2, 3, 4, 5} and all(strictly_increasing(s) for s in sk)
    last = 36 * nr
    assert any(set(sk[36]) & set(sk[nq + j]) for j in range(nr) if last + j >= SCAN_ONE_KERNEL)   # counts in the ragged last block
    rows = want_rows(sk, nq)
    assert len({r[0] for r in rows}) > 25 and max(r[1] for r in rows) >= 4 and len(rows) > 80
    sk = long_query_input()
    assert len(sk[0]) == 40_000 > SCAN_ONE_KERNEL and 40_000 % 8192 and all(strictly_increasing(s) for s in sk)
    place = {key: i for i, key in enumerate(sk[0])}
    assert sum(1 for key in sk[1] if place.get(key, 0) >= SCAN_ONE_KERNEL) > 100      # query keys of the last block are held
    assert len(want_rows(sk, 1)) == 20


def test_the_edge_room_input_has_more_edges_than_the_first_room():
    sk = edge_room_input()
    Q = set(sk[0])
    assert len(Q) == 40_000 and all(strictly_increasing(s) for s in sk)
    assert sum(len(Q & set(r)) for r in sk[1:]) == 120_000 > max(65_536, 40_000 // 4)
    rows = want_rows(sk, 1)
    assert len(rows) >= 3 and rows[-1][5] == 0


def test_the_tie_chain_and_stop_inputs():
    for nr in (1024, 1025, 2049):
        for variant in ("all", "three", "last"):
            sk, winner = ties_input(nr, variant)
            rows = want_rows(sk, 1)
            assert len(sk) == 1 + nr and rows[0][2] == 1 + winner and rows[0][4] == {"all": 3, "three": 4, "last": 5}[variant]
            tied = [j for j, r in enumerate(sk[1:]) if len(r) == rows[0][4]]
            assert tied == {"all": list(range(nr)), "three": [j for j in (1023, 1024, 2048) if j < nr], "last": [nr - 1]}[variant]
    for length in (31, 32, 33, 96, 97, 225):
        rows = want_rows(chain_input(length), 1)
        assert [r[2] for r in rows] == list(range(1, length + 1)) and [r[4] for r in rows] == [4] + [1] * (length - 1)
        assert all(r[3] == 4 for r in rows) and rows[-1][5] == 1
    for lengths in CHAINS:                                                  # queries that stop in different batches of one call
        nq, rows = len(lengths), want_rows(chains_input(lengths), len(lengths))
        for q, L in enumerate(lengths):
            mine = [r for r in rows if r[0] == q]
            assert [r[1] for r in mine] == list(range(1, L + 1)) and [r[2] for r in mine] == list(range(nq, nq + L))
            assert [r[4] for r in mine] == [4] + [1] * (L - 1) and mine[-1][5] == 0
    batch_of = lambda L: sum(L + 1 > end for end in (32, 96, 224))           # the batch (0, 1, 2, 3) that holds the stopping round
    assert [[batch_of(L) for L in lengths] for lengths in CHAINS] == [[0, 2], [2, 0], [1, 2, 3], [2, 3, 1, 1]]
    sk = stop_input()
    assert [r[2:] for r in want_rows(sk, 1, 3)] == [(1, 5, 5, 9), (2, 3, 3, 6)]       # u == min_keys is named; 2 == min_keys - 1 stops
    assert [r[2] for r in want_rows(sk, 1, 2)] == [1, 2, 3, 4] and [r[2] for r in want_rows(sk, 1, 4)] == [1]


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def fetch(ctx, k, got):
    d_mn, d_lo, d_hi, off = got
    n = int(off[-1])
    assert (d_hi is not None) == (k > 32)
    return ctx.to_host(d_mn, n, np.uint32), ctx.to_host(d_lo, n, np.uint64), (ctx.to_host(d_hi, n, np.uint64) if k > 32 else None), off


def assert_keys(got, want, tag):
    (g_mn, g_lo, g_hi, g_off), (w_mn, w_lo, w_hi, w_off) = got, want
    assert g_off[0] == 0 and g_off.tolist() == w_off.tolist(), tag
    assert np.array_equal(g_mn, w_mn), tag
    assert np.array_equal(g_lo, w_lo), tag
    assert (g_hi is None and w_hi is None) or np.array_equal(g_hi, w_hi), tag


def check_ds(ctx, k, T, mn, lo, hi, off, tag):
    d = upload(mn, lo, hi)
    got = ctx.keys_downsample_device(k, T, ptr(d[0]), ptr(d[1]), ptr(d[2]), np.asarray(off, dtype=np.uint64))
    assert_keys(fetch(ctx, k, got), ds_model(mn, lo, hi, off, T), tag)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 2047, 2048, 2049, 4096, 3 * TILE + 1])
def test_downsample_totals_and_boundaries_on_the_seams(ctx, R, k):
    T = pools()[0]
    rng = np.random.default_rng(R)
    mask = rng.random(R) < 0.5
    mask[0] = True                                                          # (R = 1: the one key survives)
    mn, lo, hi = ds_keys(mask, k)
    check_ds(ctx, k, T, mn, lo, hi, seam_offsets(R), "random mask")
    check_ds(ctx, k, T, *ds_keys(~mask, k), seam_offsets(R), "its complement")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("R", [3 * TILE, 3 * TILE - 1])
def test_downsample_of_prescribed_masks(ctx, R, k):
    T = pools()[0]
    for name, mask in prescribed_masks(R).items():
        check_ds(ctx, k, T, *ds_keys(mask, k), word_offsets(R), name)
        check_ds(ctx, k, T, *ds_keys(mask, k), seam_offsets(R), name + ", seam offsets")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("first", [5, 64, 2049])
def test_downsample_behind_keys_that_belong_to_no_sketch(ctx, first, k):
    """off[0] != 0: the keys in front of it all pass the threshold, so a pass that began at the arrays' start would count them"""
    T = pools()[0]
    R = 3 * TILE + 1
    masks = dict(prescribed_masks(R), random=np.random.default_rng(first).random(R) < 0.5)
    for name in ("random", "none kept", "the last key of each tile", "one survivor, at R - 1"):
        mn, lo, hi = ds_keys(masks[name], k, lead=first)
        assert keep_table(mn[:first], T).all()
        for off in (seam_offsets(R), word_offsets(R)):
            check_ds(ctx, k, T, mn, lo, hi, off + np.uint64(first), name)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_downsample_chain_through_both_output_sets(ctx, k):
    """three calls in a row, each reading what the one before wrote: the third writes the arrays the first one wrote"""
    vals, t1, t2, t3 = bands()
    R = 5 * TILE + 7
    rng = np.random.default_rng(k)
    mn = vals[rng.integers(0, len(vals), R)]
    lo = mixed(np.arange(R))
    hi = ~lo if k > 32 else None
    off = np.array([0, 0, 63, TILE, TILE + 1, 3 * TILE - 1, R, R], dtype=np.uint64)
    d = upload(mn, lo, hi)
    got = (ptr(d[0]), ptr(d[1]), ptr(d[2]), off)
    want = (mn, lo, hi, off)
    first_out = None
    for step, T in enumerate((t1, t2, t3)):
        got = ctx.keys_downsample_device(k, T, *got)
        want = ds_model(*want, T)
        assert_keys(fetch(ctx, k, got), want, "step %d" % step)
        assert int(want[3][-1]) > TILE                                      # every step's input and output cross a tile
        first_out = first_out or got[0]
    assert got[0] == first_out                                              # (two sets, used in turn)
    assert_keys(fetch(ctx, k, got), ds_model(mn, lo, hi, off, t3), "10 -> 100 in one step")


@pytest.mark.gpu
def test_downsample_across_the_block_form_of_the_scan():
    """32 768 * 2048 + 1 keys are 32 769 tiles, the fewest whose counts are scanned in blocks (a last block of one count); there
    is no smaller shape for this path.  Keys made on the device; expected: a table lookup and masked_select in torch"""
    import torch
    R = SCAN_ONE_KERNEL * TILE + 1
    assert -(-R // TILE) == SCAN_ONE_KERNEL + 1
    pool = np.arange(4096, dtype=np.int64) * 1021 + 3
    assert pool.max() < 4 ** M
    hashes = np.array([orc.xxh64(int(v)) for v in pool], dtype=np.uint64)
    T = int(np.sort(hashes)[2048])
    table = np.zeros(4 ** M, dtype=bool)
    table[pool] = hashes <= T
    assert table.sum() == 2049 and int(hashes[np.argmax(hashes == T)]) == T
    gen = torch.Generator(device="cuda")
    gen.manual_seed(63)
    d_pool = torch.from_numpy(pool.astype(np.int32)).cuda()
    mn = d_pool[torch.randint(0, 4096, (R + 16,), device="cuda", dtype=torch.int32, generator=gen)]
    mn[R - 1] = int(pool[np.argmax(hashes == T)])                           # the one key of the last tile survives, by the hash equal to T
    lo = (torch.arange(R + 8, device="cuda", dtype=torch.int64) + 1) * (GOLD - (1 << 64))
    keep = torch.from_numpy(table).cuda()[mn[:R]]
    w_mn, w_lo = torch.masked_select(mn[:R], keep), torch.masked_select(lo[:R], keep)
    bounds = [0, 12_345 * TILE + 777, SCAN_ONE_KERNEL * TILE, R]
    w_off = [int(keep[:b].sum()) for b in bounds]
    total = w_off[-1]
    assert w_off[3] - w_off[2] == 1 and 0.49 * R < total < 0.51 * R
    torch.cuda.synchronize()
    with sp.Context(0) as c:
        for call in range(3):                                               # (the first reserves the output arrays; the third reuses its set)
            t0 = time.perf_counter()
            o_mn, o_lo, o_hi, o_off = c.keys_downsample_device(31, T, mn.data_ptr(), lo.data_ptr(), None, np.array(bounds, dtype=np.uint64))
            print("downsample of %d keys in %d tiles, call %d: %.2f ms of host time, the call's stream wait included"
                  % (R, SCAN_ONE_KERNEL + 1, call, 1e3 * (time.perf_counter() - t0)))
            assert o_hi is None and o_off.tolist() == w_off
        # the values: 1024 runs of 64 keys spread over the output, and its last 4096 keys
        starts = np.arange(1024, dtype=np.int64) * ((total - 4096) // 1024)
        at = torch.from_numpy((starts[:, None] + np.arange(64)[None, :]).reshape(-1)).cuda()
        s_mn, s_lo = w_mn[at].cpu().numpy().view(np.uint32).reshape(1024, 64), w_lo[at].cpu().numpy().view(np.uint64).reshape(1024, 64)
        for i, s in enumerate(starts.tolist()):
            assert np.array_equal(c.to_host(o_mn + 4 * s, 64, np.uint32), s_mn[i]), s
            assert np.array_equal(c.to_host(o_lo + 8 * s, 64, np.uint64), s_lo[i]), s
        assert np.array_equal(c.to_host(o_mn + 4 * (total - 4096), 4096, np.uint32), w_mn[-4096:].cpu().numpy().view(np.uint32))
        assert np.array_equal(c.to_host(o_lo + 8 * (total - 4096), 4096, np.uint64), w_lo[-4096:].cpu().numpy().view(np.uint64))


@pytest.mark.gpu
def test_gather_searches_by_minimizer_then_hi_then_lo(ctx):
    sk = order_input()
    want = want_rows(sk, 1)
    assert [r[2] for r in want] == [6, 3, 2, 1]
    assert gpu_rows(ctx, 63, sk, 1) == want
    assert gpu_rows(ctx, 63, [sk[0]] + sk[:0:-1], 1) == want_rows([sk[0]] + sk[:0:-1], 1)      # the references in reverse


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_gather_matches_at_the_ends_of_waves_and_tiles(ctx, k):
    sk, _ = waves_input(k)
    want = want_rows(sk, 1)
    assert [r[2:5] for r in want] == [(2, 67, 67), (8, 65, 65), (7, 3, 3)]
    assert gpu_rows(ctx, k, sk, 1) == want


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_gather_behind_keys_that_belong_to_no_sketch(ctx, k):
    """off[0] = 7.  The seven keys in front are not unrelated ones but copies of keys the query holds, in no order and one
    of them twice: an order check that began at entry 0 would refuse them, a search that began there would find them, and a
    query key numbered from entry 0 would land seven places off"""
    sk, matched = waves_input(k)
    lead = [sk[0][i] for i in (40, 3, 3, 70, 12, 0, 55)]
    want = want_rows(sk, 1)
    assert gpu_rows(ctx, k, sk, 1, lead=lead) == want
    assert gpu_rows(ctx, k, [sk[0][:30], sk[0][30:]] + sk[1:], 2, lead=lead) == want_rows([sk[0][:30], sk[0][30:]] + sk[1:], 2)


@pytest.mark.gpu
def test_gather_scans_in_blocks(ctx):
    sk = cells_input()
    assert gpu_rows(ctx, 63, sk, 37) == want_rows(sk, 37)
    assert gpu_rows(ctx, 63, sk, 37, 2, 3) == want_rows(sk, 37, 2, 3)
    sk = long_query_input()
    assert gpu_rows(ctx, 31, sk, 1) == want_rows(sk, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("nr", [1024, 1025, 2049])
def test_gather_ties_across_the_strides_of_the_pick(ctx, nr):
    for variant in ("all", "three", "last"):
        sk, winner = ties_input(nr, variant)
        want = want_rows(sk, 1)
        assert want[0][2] == 1 + winner
        assert gpu_rows(ctx, 31, sk, 1) == want, variant


@pytest.mark.gpu
@pytest.mark.parametrize("length", [31, 32, 33, 96, 97, 225])
def test_gather_rounds_that_end_on_and_past_a_batch(ctx, length):
    sk = chain_input(length)
    want = want_rows(sk, 1)
    assert len(want) == length
    assert gpu_rows(ctx, 63, sk, 1) == want
    for max_rounds in (1, 32, 33):
        assert gpu_rows(ctx, 63, sk, 1, 1, max_rounds) == want[:max_rounds], max_rounds
    assert gpu_rows(ctx, 63, sk, 1, 2) == want[:1]                          # every later round would name one key


@pytest.mark.gpu
@pytest.mark.parametrize("lengths", CHAINS)
def test_gather_queries_that_stop_in_different_batches(ctx, lengths):
    """a batch's rows are read back per query (rows[q * B + slot], B = 32, 64, 128, or what max_rounds leaves of it) while
    some queries have stopped and others go on"""
    sk = chains_input(lengths)
    nq = len(lengths)
    want = want_rows(sk, nq)
    assert len(want) == sum(lengths)
    assert gpu_rows(ctx, 63, sk, nq) == want
    for max_rounds in (33, 50, 97):
        assert gpu_rows(ctx, 63, sk, nq, 1, max_rounds) == [r for r in want if r[1] <= max_rounds], max_rounds


@pytest.mark.gpu
def test_gather_stops_below_min_keys_and_not_at_it(ctx):
    sk = stop_input()
    for min_keys in (1, 2, 3, 4, 5, 6):
        want = want_rows(sk, 1, min_keys)
        assert len(want) == {1: 4, 2: 4, 3: 2, 4: 1, 5: 1, 6: 0}[min_keys]
        assert gpu_rows(ctx, 31, sk, 1, min_keys) == want, min_keys


@pytest.mark.gpu
def test_gather_makes_room_for_the_edges_and_keeps_it():
    sk = edge_room_input()
    want = want_rows(sk, 1)
    with sp.Context(0) as fresh:
        assert gpu_rows(fresh, 31, sk, 1) == want                          # 120 000 edges, room for 65 536: the match pass runs twice
        assert gpu_rows(fresh, 31, sk, 1) == want                          # ... and once, in the room the first call left


@pytest.mark.gpu
def test_gather_order_check_at_the_seams(ctx):
    k = 63
    S = sorted(keys_of(range(100), k))
    refs = [S[0:20], S[40:65]]
    # a sketch may begin below, or at, the key the one before it ends with
    q = [S[10:50], S[5:30], [S[29]] + S[60:70]]
    assert q[1][0] < q[0][-1] and q[2][0] == q[1][-1] and all(strictly_increasing(s) for s in q)
    assert gpu_rows(ctx, k, q + refs, 3) == want_rows(q + refs, 3)
    # ... but inside a sketch every key comes strictly after the one before it
    for bad in (S[5:17] + [S[16]] + S[17:30], S[5:17] + [S[18], S[17]] + S[19:30]):
        with pytest.raises(sp.SpspError) as e:
            gpu_rows(ctx, k, [q[0], bad, q[2]] + refs, 3)
        assert e.value.code == sp.ERR_ARG and "increasing" in str(e.value)
    # the references' side, where entry 2048 is the first of the second tile
    big = sorted(keys_of(range(1000, 1000 + TILE + 30), k))
    query = [sorted(big[5:25] + big[TILE - 3:TILE + 5] + S[:10])]
    for head in (big[TILE - 1], big[100]):                                  # entry 2048 equal to entry 2047, and below it
        a, b = big[:TILE], [head] + big[TILE:]
        assert len(a) == TILE and strictly_increasing(b) and b[0] <= a[-1]
        assert gpu_rows(ctx, k, query + [a, b], 1) == want_rows(query + [a, b], 1)
        with pytest.raises(sp.SpspError) as e:
            gpu_rows(ctx, k, query + [a + b], 1)
        assert e.value.code == sp.ERR_ARG
    assert gpu_rows(ctx, k, query + [big], 1) == want_rows(query + [big], 1)
