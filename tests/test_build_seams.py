"""The sketch builder on the device (spsp_sketch_build_device: spsp_build.hip) on hand-built super-k-mer streams at its seams.

Through spsp_sketch_text the builder only ever sees what a scan of a random genome selects, so the boundaries of its own
stages -- the radix sort's lanes, rounds and tiles, the place tiles and their 64-ary search, the table at exactly half load,
the walk's grid, the assembly's 64-lane strides, the two forms of the scans -- are met by luck or never.  The streams below
are written entry by entry (tests/streams.py) so that each is met on purpose.  The expectation is streams.model(), plain
Python written from the reference's rules, byte for byte and counter for counter, file by file, no tolerance; above about
20 000 k-mer places (where the model would take too long) it is the host builder, which one CPU test holds to the model on
every smaller case, as another holds the model to the oracle on scan-made streams.

build_cases() is the one table: (name, k, m, abundance, bases, rec_off, stream, file_sk).  CLAIMS[name] is what the name
claims, as a predicate over the model's instrumentation (or, for the cases beyond the model, over the stream itself), checked
on the CPU by test_the_cases_are_what_they_are_called together with every stream's truthfulness: the minimizer occurs in
every k-mer of its super-k-mer, every entry lies inside its record.  FORMS[name]: which input forms a case runs with
(packed 0 = ASCII bases, 1 = the ingest's 2-bit words).

What a wrong kernel would look like, and where it shows:
    a sort that is not stable, or skips or mis-shifts a pass: sort_*, files_*, tiles_* (a bucket's lines are in stream order)
    a k-mer taken from the wrong window of a reverse-strand entry: rev_*
    a place tile or its search off by one: places_*, search_*
    a table probe that does not end, or merges what differs in one word: table_*, k63_*
    counts that are not reduced mod 256 before -a: counts_a*
    neighbours tried in another order than A, T, C, G: fork_*
    an output offset from the wrong scan form: buckets_32768, buckets_32769"""
import functools
import random
import zlib

import numpy as np
import pytest

import streams as S
import supersampler_amd as sp
from oracle import oracle_py as orc

RATE = 7.0
MODEL_MAX = 20000                                # k-mer places up to which the model is the expectation
RS_TILE = 2048                                   # kRsTile
BLD_TILE = 1024                                  # kBldTile
SCAN_ONE = 32768                                 # counts the one-kernel form of launch_scan_u32 takes
KM = [(31, 11), (32, 12), (33, 13), (63, 15), (21, 9), (15, 15)]

CLAIMS = {}                                      # name -> predicate(case, info) (info: streams.model's, None beyond MODEL_MAX)
FORMS = {}                                       # name -> forms other than (0, 1)
_BUILDERS = []                                   # (name, function) in table order


def case(name, forms=(0, 1)):
    def deco(fn):
        _BUILDERS.append((name, fn))
        if tuple(forms) != (0, 1):
            FORMS[name] = tuple(forms)
        return fn
    return deco


def rng_of(name):
    return random.Random(zlib.crc32(name.encode()))


def minimizers(rng, m, n):
    """n different m-mers, none of them a run of one base"""
    out = set()
    while len(out) < n:
        x = S.rnd(rng, m)
        if len(set(x)) > 1:
            out.add(x)
    out = list(out)
    rng.shuffle(out)
    return out


def total_places(k, stream):
    return int((stream["len"].astype(np.int64) - k + 1).sum())


def all_single_lines(info):
    """every k-mer was met once and every walk is its start k-mer alone"""
    return all(c == 1 for d in info["counts"].values() for c in d.values()) and all(w[2] == 0 and w[3] == 0 for w in info["walks"])


# ------------------------------------------------------------------------------------------------ sort

def dealt(name, k, m, n, n_mn=8):
    """n unrelated one-k-mer super-k-mers dealt round-robin over n_mn minimizers: every bucket's line order is its stream order
    across the sort's lanes, waves, rounds and tiles"""
    rng = rng_of(name)
    X = minimizers(rng, m, n_mn)
    s = S.Stream(k, m)
    for i in range(n):
        s.add(S.superkmer(rng, k, m, X[i % n_mn]), X[i % n_mn])
    return s


for _n in (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097):
    def _sort_n(name, n=_n):
        CLAIMS[name] = lambda c, info, n=n: (len(c[6]) == n and len(info["buckets"]) == min(n, 8) and all_single_lines(info)
                                             and max(info["entries"].values()) == (n + 7) // 8)
        return (31, 11, 1) + dealt(name, 31, 11, n).done()
    case("sort_n%d" % _n)(_sort_n)


@case("sort_one_bucket_2049")
def _(name):
    CLAIMS[name] = lambda c, info: len(info["buckets"]) == 1 and info["entries"][info["buckets"][0]] == 2049 and all_single_lines(info)
    return (31, 11, 1) + dealt(name, 31, 11, 2049, 1).done()


@case("sort_descending_2049")
def _(name):
    rng = rng_of(name)
    s = S.Stream(21, 11)
    vals = sorted(rng.sample(range(1, 4 ** 11 - 1), 2049), reverse=True)
    for v in vals:
        s.add(S.superkmer(rng, 21, 11, S.bases(v, 11)), S.bases(v, 11))
    CLAIMS[name] = lambda c, info: (len(info["buckets"]) == 2049 and (np.diff(c[6]["minimizer"].astype(np.int64)) < 0).all())
    return (21, 11, 1) + s.done()


for _byte, (_shift, _width) in enumerate([(0, 8), (8, 8), (16, 8), (24, 6)]):
    def _sort_byte(name, shift=_shift, width=_width):
        """m = 15: minimizers that differ inside ONE byte of the sort key only, in shuffled stream order, two entries each"""
        rng = rng_of(name)
        base = rng.getrandbits(30) & ~(((1 << width) - 1) << shift)
        vals = [base | (j << shift) for j in range(1 << width)] * 2
        rng.shuffle(vals)
        s = S.Stream(31, 15)
        for v in vals:
            s.add(S.superkmer(rng, 31, 15, S.bases(v, 15)), S.bases(v, 15))
        mask = ((1 << width) - 1) << shift
        CLAIMS[name] = lambda c, info: (len({int(x) & ~mask for x in c[6]["minimizer"]}) == 1 and len(info["buckets"]) == 1 << width
                                        and (np.diff(c[6]["minimizer"].astype(np.int64)) < 0).any())
        return (31, 15, 1) + s.done()
    case("sort_key_byte%d" % _byte)(_sort_byte)


def key_bits(n_files):
    b = 0
    while (1 << b) < n_files:
        b += 1
    return 30 + b


for _nf in (1, 2, 4, 5, 256, 257):
    def _files_n(name, nf=_nf):
        """every file: three entries under two minimizers that all files share, the larger minimizer first"""
        rng = rng_of(name)
        X = sorted(minimizers(rng, 11, 2), key=S.num)
        s = S.Stream(31, 11)
        for _f in range(nf):
            for x in (X[1], X[0], X[1]):
                s.add(S.superkmer(rng, 31, 11, x), x)
        want_bits = {1: 30, 2: 31, 4: 32, 5: 33, 256: 38, 257: 39}[nf]
        CLAIMS[name] = lambda c, info: key_bits(len(c[7]) - 1) == want_bits and (want_bits + 7) // 8 == (5 if nf >= 5 else 4)
        return (31, 11, 1) + s.done(list(range(0, 3 * nf + 1, 3)))
    case("files_%d" % _nf)(_files_n)


@case("files_merge_a2")
def _(name):
    """four files with the same minimizers and the same k-mers, once each, at -a 2: nothing is usable unless files are merged;
    a fifth file holds them twice"""
    rng = rng_of(name)
    X = minimizers(rng, 11, 3)
    seqs = [(S.superkmer(rng, 31, 11, x, q, None), x) for x in X for q in (1, 4)]
    s = S.Stream(31, 11)
    for f in range(6):                                               # (the fifth file: two rounds)
        for seq, x in seqs:
            s.add(seq, x)
    n = len(seqs)
    CLAIMS[name] = lambda c, info: True                              # (per file: see test_the_cases_are_what_they_are_called)
    return (31, 11, 2) + s.done([0, n, 2 * n, 3 * n, 4 * n, 6 * n])


@case("files_empty")
def _(name):
    """empty files first, in the middle, last, and two in a row"""
    rng = rng_of(name)
    X = minimizers(rng, 11, 3)
    s = S.Stream(31, 11)
    sizes = [0, 3, 0, 0, 2, 0, 4, 0]
    for i in range(sum(sizes)):
        s.add(S.superkmer(rng, 31, 11, X[i % 3], 1 + i % 3), X[i % 3])
    CLAIMS[name] = lambda c, info: np.diff(c[7].astype(np.int64)).tolist() == sizes
    return (31, 11, 1) + s.done(np.concatenate([[0], np.cumsum(sizes)]).tolist())


for _n in (RS_TILE * 128, RS_TILE * 128 + 1):
    def _tiles(name, n=_n):
        """128 and 129 sort tiles: 256 x tiles histogram counts are 32 768 (the scan's one-kernel form) and 33 024 (its block
        form).  m = 9: 2^18 minimizers for 2^18 entries, so that buckets of two, three and more unrelated k-mers from far-apart
        tiles abound"""
        rng = rng_of(name)
        b, off, st = S.shared_singles(rng, 21, 9, n, lambda i: i % 13)
        tiles = (n + RS_TILE - 1) // RS_TILE
        CLAIMS[name] = lambda c, info: (len(c[6]) == n and (256 * tiles > SCAN_ONE) == (n > RS_TILE * 128)
                                        and np.bincount(np.unique(c[6]["minimizer"], return_counts=True)[1]).size > 4)
        return (21, 9, 1, b, off, st, np.array([0, n], np.uint32))
    case("tiles_%d" % ((_n + RS_TILE - 1) // RS_TILE))(_tiles)


# ------------------------------------------------------------------------------------------------ places

def uniform(name, k, m, n, q, n_mn=4, left=None):
    rng = rng_of(name)
    X = minimizers(rng, m, n_mn)
    s = S.Stream(k, m)
    for i in range(n):
        s.add(S.superkmer(rng, k, m, X[i % n_mn], q, left), X[i % n_mn])
    return s, X, rng


for _t in (1023, 1024, 1025):
    def _places_total(name, t=_t):
        s, X, rng = uniform(name, 31, 11, t // 3, 3)
        if t % 3:
            s.add(S.superkmer(rng, 31, 11, X[0], t % 3), X[0])
        CLAIMS[name] = lambda c, info: sum(info["places"].values()) == t
        return (31, 11, 1) + s.done()
    case("places_total_%d" % _t)(_places_total)

for _q, _n in ((1, 1500), (3, 700), (21, 100)):
    def _places_q(name, q=_q, n=_n):
        s, _, _ = uniform(name, 31, 11, n, q)
        CLAIMS[name] = lambda c, info: ((c[6]["len"] == 31 + q - 1).all() and sum(info["places"].values()) > BLD_TILE
                                        and (BLD_TILE % q == 0) == (q == 1)
                                        and (q < 21 or sum(w[5] for w in info["walks"]) == n))
        return (31, 11, 1) + s.done()
    case("places_q%d" % _q)(_places_q)

for _n in (1, 2, 64, 65, 66, 4097):
    def _search(name, n=_n):
        """stream lengths around the 64-ary search's fan-out, every one with more than one place tile.  One and two entries
        have to be longer than a scan would emit for that: the minimizer every k - m + 1 bases"""
        rng = rng_of(name)
        X = minimizers(rng, 11, 3)
        s = S.Stream(31, 11)
        for i in range(n):
            x = X[i % 3]
            if n <= 2:
                s.add(S.long_superkmer(rng, 31, 11, x, 1100 - 300 * i), x)
            else:
                s.add(S.superkmer(rng, 31, 11, x, 20 if n < 100 else 1), x)
        CLAIMS[name] = lambda c, info: len(c[6]) == n and sum(info["places"].values()) > BLD_TILE
        return (31, 11, 1) + s.done()
    case("search_%d" % _n)(_search)


@case("rev_merge_a2")
def _(name):
    """reverse-strand entries whose k-mers are those of forward entries, at -a 2: they must merge into counts of 2"""
    rng = rng_of(name)
    X = minimizers(rng, 11, 2)
    s = S.Stream(31, 11)
    seqs = [(S.superkmer(rng, 31, 11, X[i % 2], q), X[i % 2]) for i, q in enumerate((1, 5, 21, 2, 9))]
    for seq, x in seqs:
        s.add(seq, x, 0)
    for seq, x in seqs:
        s.add(seq, x, 1)
    s.add(S.superkmer(rng, 31, 11, X[0], 3), X[0], 1)                # (met once: stays unusable)
    CLAIMS[name] = lambda c, info: (sorted(set(cnt for d in info["counts"].values() for cnt in d.values())) == [1, 2]
                                    and (c[6]["rev"] == 1).sum() == 6 and len(info["walks"]) == 5)
    return (31, 11, 2) + s.done()


@case("rev_fork")
def _(name):
    """a reverse-strand entry a-b-c in front of a forward k-mer b' that is a's other right neighbour: which of b and b' follows
    a, and what is left for the other, depends on a being the FIRST k-mer of its entry in the oriented direction"""
    rng = rng_of(name)
    X = minimizers(rng, 11, 1)[0]
    s = S.Stream(31, 11)
    abc = S.superkmer(rng, 31, 11, X, 3, 10)
    abc = abc[:31] + b"G" + abc[32:]                                 # b ends in G: tried last
    s.add(abc, X, 1)
    s.add(abc[1:31] + b"A", X, 0)                                    # b' ends in A: tried first
    CLAIMS[name] = lambda c, info: (info["forks"] == [(S.num(X), "R", 2)] and len(info["walks"]) == 2
                                    and info["walks"][0][1] == abc[:31] and info["walks"][0][3] == 1)
    return (31, 11, 1) + s.done()


for _k, _m in KM:
    def _km(name, k=_k, m=_m):
        """a little of everything under other word sizes: maximal super-k-mers whole and in pieces, shorter ones, both
        strands, a k-mer met twice"""
        rng = rng_of(name)
        X = minimizers(rng, m, 3)
        s = S.Stream(k, m)
        qmax = k - m + 1
        for i in range(24):
            x = X[i % 3]
            q = (1, qmax, (qmax + 1) // 2, min(2, qmax))[i % 4]
            rec = s.add(S.superkmer(rng, k, m, x, q), x, (i // 3) % 2)
            if i % 5 == 0:
                s.again(rec, x, 0, k, (i // 3) % 2)
        CLAIMS[name] = lambda c, info: (len(info["buckets"]) == 3 and max(cnt for d in info["counts"].values() for cnt in d.values()) >= 2
                                        and (qmax == 1 or any(w[5] for w in info["walks"])) and set(c[6]["rev"].tolist()) == {0, 1})
        return (k, m, 1) + s.done()
    case("km_%d_%d" % (_k, _m))(_km)


for _word, _place, _changed in (("hi", 40, (3, 17, 30)), ("lo", 5, (31, 45, 62))):
    def _k63(name, word=_word, place=_place, changed=_changed):
        """k = 63: k-mers of one bucket that differ in one base of the first 31 (the high word) or of the last 32 (the low
        word) only, each met once, and the first of them met twice"""
        rng = rng_of(name)
        X = minimizers(rng, 15, 1)[0]
        first = S.superkmer(rng, 63, 15, X, 1, place)
        s = S.Stream(63, 15)
        rec = s.add(first, X)
        for at in changed:
            other = first[:at] + (b"G" if first[at: at + 1] != b"G" else b"T") + first[at + 1:]
            s.add(other, X, at & 1)
        s.again(rec, X)

        def claim(c, info):
            d = info["counts"][S.num(X)]
            vals = [S.num(km) for km in d]
            lo, hi = (1 << 64) - 1, ((1 << 126) - 1) ^ ((1 << 64) - 1)
            keep = lo if word == "hi" else hi                         # the word that must be the same
            return len(d) == 4 and list(d.values()) == [2, 1, 1, 1] and len({v & keep for v in vals}) == 1 and len({v & ~keep for v in vals}) == 4
        CLAIMS[name] = claim
        return (63, 15, 1) + s.done()
    case("k63_%s_only" % _word)(_k63)


for _where in ("0", "end"):
    def _x_at(name, where=_where):
        """the minimizer at place 0 (or k - m) of the START k-mer, with neighbours to find: a walk that only goes left (right).
        A maximal super-k-mer as single k-mers, last (first) k-mer first"""
        rng = rng_of(name)
        X = minimizers(rng, 11, 1)[0]
        seq = S.maximal(rng, 31, 11, X)
        s = S.Stream(31, 11)
        rec = s.pad(seq)
        order = list(range(21))
        if where == "0":
            order.reverse()
        for i in order:
            s.again(rec, X, i, 31)
        s.add(S.superkmer(rng, 31, 11, X, 1, 0 if where == "0" else 20), X)      # ... and one alone
        want = (20, 0) if where == "0" else (0, 20)
        CLAIMS[name] = lambda c, info: (info["walks"][0][2:4] == want and info["walks"][0][5] and len(info["walks"]) == 2
                                        and info["walks"][0][1].find(X) == (0 if where == "0" else 20)
                                        and info["walks"][1][1].find(X) == (0 if where == "0" else 20))
        return (31, 11, 1) + s.done()
    case("x_at_%s" % _where)(_x_at)


@case("x_twice")
def _(name):
    """the minimizer twice in one k-mer: the first place counts"""
    rng = rng_of(name)
    X = minimizers(rng, 11, 1)[0]
    s = S.Stream(31, 11)
    one = S.rnd(rng, 3) + X + S.rnd(rng, 2) + X + S.rnd(rng, 4)
    s.add(one, X)
    two = S.rnd(rng, 6) + X + X + S.rnd(rng, 5)                      # three k-mers; the middle ones hold it twice
    s.add(two, X, 1)
    s.add(S.superkmer(rng, 31, 11, X, 2), X)
    CLAIMS[name] = lambda c, info: sum(km.count(X) >= 2 for km in info["counts"][S.num(X)]) >= 3 and one.find(X) == 3
    return (31, 11, 1) + s.done()


for _r in (0, 1, 15):
    def _packed_first(name, r=_r):
        """2-bit words: k-mers whose first base sits at place r of its word (q & 15 == r), forward and reverse"""
        rng = rng_of(name)
        X = minimizers(rng, 11, 2)
        s = S.Stream(31, 11)
        for i in range(6):
            s.pad(S.rnd(rng, (r - s.n_bases) % 16 + 16))              # the next record starts at place r of a word
            s.add(S.superkmer(rng, 31, 11, X[i % 2], 1), X[i % 2], i % 2)
        CLAIMS[name] = lambda c, info: all((int(c[5][int(e["rec"])]) + int(e["start"])) % 16 == r for e in c[6]) and len(c[6]) == 6
        return (31, 11, 1) + s.done()
    case("packed_first_%d" % _r, forms=(1,))(_packed_first)

    def _packed_tail(name, r=_r):
        """2-bit words: the last k-mer ends on the buffer's last base, n_bases % 16 == r: the five words read from its first
        base's word reach as far behind the bases as they ever do"""
        rng = rng_of(name)
        X = minimizers(rng, 15, 2)
        s = S.Stream(63, 15)
        body = [S.superkmer(rng, 63, 15, X[i % 2], 1 + 3 * i) for i in range(3)]
        n = sum(len(b) for b in body)
        s.pad(S.rnd(rng, (r - n) % 16 + 16))
        for i, b in enumerate(body):
            s.add(b, X[i % 2], i % 2)
        s.again(len(s.recs) - 1, X[0], len(body[2]) - 63, 63, 0)      # the last k-mer of the buffer, on its own as well
        CLAIMS[name] = lambda c, info: (len(c[4]) % 16 == r and int(c[5][int(c[6][-1]["rec"])]) + int(c[6][-1]["start"]) + 63 == len(c[4]))
        return (63, 15, 1) + s.done()
    case("packed_tail_%d" % _r, forms=(1,))(_packed_tail)


# ------------------------------------------------------------------------------------------------ table

for _t in (512, 513):
    def _table(name, t=_t):
        """a power of two of places: twice as many slots, the table exactly half full; one more: the next size"""
        s, X, rng = uniform(name, 31, 11, 128, 4, 5)
        if t == 513:
            s.add(S.superkmer(rng, 31, 11, X[0]), X[0])
        slots = 1024
        while slots < 2 * t:
            slots *= 2
        CLAIMS[name] = lambda c, info: sum(info["places"].values()) == t and slots == (1024 if t == 512 else 2048)
        return (31, 11, 1) + s.done()
    case("table_%d" % _t)(_table)

for _a in (1, 2):
    def _two_mn(name, a=_a):
        """one k-mer under two minimizers: two buckets with a count of 1 each, never one count of 2"""
        rng = rng_of(name)
        X, Y = minimizers(rng, 11, 2)
        km = S.rnd(rng, 2) + X + S.rnd(rng, 3) + Y + S.rnd(rng, 4)
        s = S.Stream(31, 11)
        rec = s.add(km, X)
        s.again(rec, Y)
        CLAIMS[name] = lambda c, info: (len(info["buckets"]) == 2 and all(list(d.items()) == [(km, 1)] for d in info["counts"].values())
                                        and len(info["walks"]) == (2 if a == 1 else 0))
        return (31, 11, a) + s.done()
    case("two_minimizers_a%d" % _a)(_two_mn)

COUNTS = (255, 256, 257, 511, 512, 513)
for _a in (1, 2, 255, 256):
    def _counts(name, a=_a):
        """six buckets of one k-mer each, met 255 ... 513 times: the count is a uint8 when -a reads it"""
        rng = rng_of(name)
        X = sorted(minimizers(rng, 11, len(COUNTS)), key=S.num)
        s = S.Stream(31, 11)
        recs = [s.pad(S.superkmer(rng, 31, 11, x)) for x in X]
        todo = [(i, j) for i, n in enumerate(COUNTS) for j in range(n)]
        rng.shuffle(todo)
        for i, _j in todo:
            s.again(recs[i], X[i])
        usable = [n for n in COUNTS if (n & 255) >= a]
        CLAIMS[name] = lambda c, info: ([list(info["counts"][S.num(x)].values()) for x in X] == [[n] for n in COUNTS]
                                        and len(info["walks"]) == len(usable)
                                        and usable == {1: [255, 257, 511, 513], 2: [255, 511], 255: [255, 511], 256: []}[a])
        return (31, 11, a) + s.done()
    case("counts_a%d" % _a)(_counts)


@case("first_in_last_entry")
def _(name):
    """a k-mer whose first (and only) occurrence lies in its bucket's last stream entry, behind entries of other buckets, and
    which the bucket's first k-mer reaches as a neighbour"""
    rng = rng_of(name)
    X, Y = minimizers(rng, 11, 2)
    s = S.Stream(31, 11)
    ab = S.superkmer(rng, 31, 11, X, 2, 10)
    s.add(ab[:31], X)
    for i in range(5):
        s.add(S.superkmer(rng, 31, 11, (X, Y)[i % 2], 2), (X, Y)[i % 2])
    s.add(S.superkmer(rng, 31, 11, Y, 3), Y)
    s.add(ab[1:], X)
    CLAIMS[name] = lambda c, info: (info["first_entry"][S.num(X)][ab[1:]] == info["entries"][S.num(X)] - 1
                                    and int(c[6][-1]["minimizer"]) == S.num(X) and (S.num(X), ab[:31], 0, 1, True, False) in info["walks"])
    return (31, 11, 1) + s.done()


# ------------------------------------------------------------------------------------------------ walk and assembly

for _parts in (2, 3, 21):
    for _order in ("forward", "reversed", "shuffled"):
        def _split(name, parts=_parts, order=_order):
            """two maximal super-k-mers of one bucket, each given as overlapping entries: one behind the other in forward or
            in reversed order, or the entries of both shuffled together"""
            rng = rng_of(name)
            X = minimizers(rng, 11, 1)[0]
            s = S.Stream(31, 11)
            ps = []
            for _two in range(2):
                seq = S.maximal(rng, 31, 11, X)
                rec = s.pad(seq)
                mine = [(rec, a, ln) for a, ln in S.pieces(seq, 31, parts)]
                ps += mine[::-1] if order == "reversed" else mine
            if order == "shuffled":
                if parts == 2:                                       # (two entries are always in one of the two orders: interleaved then)
                    ps = [ps[i] for i in (1, 2, 0, 3)]
                while parts > 2 and any(sorted(x) in (x, x[::-1]) for x in ([p for p in ps if p[0] == r] for r in (0, 1))):
                    rng.shuffle(ps)
            for rec, a, ln in ps:
                s.again(rec, X, a, ln)
            starts = [p[1] for p in ps if p[0] == 0]
            CLAIMS[name] = lambda c, info: (len(c[6]) == 2 * parts and info["distinct"][S.num(X)] == 42
                                            and sum(w[2] + w[3] + 1 for w in info["walks"]) == 42
                                            and {"forward": starts == sorted(starts), "reversed": starts == sorted(starts, reverse=True),
                                                 "shuffled": parts == 2 or starts not in (sorted(starts), sorted(starts, reverse=True))}[order]
                                            and (parts == 21 or 2 in info["counts"][S.num(X)].values()))
            return (31, 11, 1) + s.done()
        case("split_%d_%s" % (_parts, _order))(_split)

for _side in ("right", "left"):
    for _nn, _letters in ((2, b"CT"), (3, b"GCT"), (4, b"GCTA")):
        def _fork(name, side=_side, nn=_nn, letters=_letters):
            """a k-mer with two, three or four usable neighbours on one side, given in the reverse of the order they are tried in"""
            rng = rng_of(name)
            X = minimizers(rng, 11, 1)[0]
            c0 = S.superkmer(rng, 31, 11, X, 1, 10)
            s = S.Stream(31, 11)
            s.add(c0, X)
            for ch in letters:
                s.add(c0[1:] + bytes([ch]) if side == "right" else bytes([ch]) + c0[:-1], X)
            took = b"T" if nn < 4 else b"A"

            def claim(c, info):
                w = info["walks"][0]
                tail = w[1] == c0 and (w[2], w[3]) == ((0, 1) if side == "right" else (1, 0))
                line = info["text"][S.num(X)].split(b"\n")
                got = line[1][-1:] if side == "right" else line[0][:1]
                return info["forks"][0] == (S.num(X), "R" if side == "right" else "L", nn) and tail and got == took and len(info["walks"]) == nn
            CLAIMS[name] = claim
            return (31, 11, 1) + s.done()
        case("fork_%s_%d" % (_side, _nn))(_fork)


@case("left_stops_early")
def _(name):
    """the start k-mer has one left neighbour where it could take five, and three on the right"""
    rng = rng_of(name)
    X = minimizers(rng, 11, 1)[0]
    seq = S.superkmer(rng, 31, 11, X, 5, 16)                          # k-mer 1 holds X at place 15: five left steps wanted
    s = S.Stream(31, 11)
    rec = s.pad(seq)
    s.again(rec, X, 1, 31)
    s.again(rec, X)
    CLAIMS[name] = lambda c, info: info["walks"] == [(S.num(X), seq[1:32], 1, 3, True, False)]
    return (31, 11, 1) + s.done()


@case("consumed_neighbour")
def _(name):
    """a later start whose only right neighbour an earlier walk has taken"""
    rng = rng_of(name)
    X = minimizers(rng, 11, 1)[0]
    ab = S.superkmer(rng, 31, 11, X, 2, 10)
    z = (b"G" if ab[:1] != b"G" else b"T") + ab[1:31]                 # z's right neighbour is b as well
    s = S.Stream(31, 11)
    s.add(ab, X)
    s.add(z, X)
    CLAIMS[name] = lambda c, info: (info["walks"] == [(S.num(X), ab[:31], 0, 1, True, False), (S.num(X), z, 0, 0, True, False)]
                                    and info["seen_refused"] >= 1)
    return (31, 11, 1) + s.done()


@case("blob_over_64")
def _(name):
    """eight maximal super-k-mers in one bucket at k - m = 20: 320 codes, a blob of 81 bytes for the assembly's 64 lanes"""
    s, X, _ = uniform(name, 31, 11, 8, 21, 1)
    CLAIMS[name] = lambda c, info: len(info["blob"][S.num(X[0])]) == 81 and sum(w[5] for w in info["walks"]) == 8
    return (31, 11, 1) + s.done()


@case("lines_300")
def _(name):
    s, X, _ = uniform(name, 31, 11, 300, 1, 1)
    CLAIMS[name] = lambda c, info: info["text"][S.num(X[0])].count(b"\n") == 600 and len(info["text"][S.num(X[0])]) == 300 * 22
    return (31, 11, 1) + s.done()


for _n in (1, 63, 64, 65, SCAN_ONE, SCAN_ONE + 1):
    def _buckets(name, n=_n):
        """bucket counts around the walk's 64 lanes, and the two forms of the output offsets' scan"""
        rng = rng_of(name)
        vals = rng.sample(range(1, 4 ** 11 - 1), n)
        s = S.Stream(21, 11)
        for v in vals:
            s.add(S.superkmer(rng, 21, 11, S.bases(v, 11), 1 + (v & 1)), S.bases(v, 11))
        CLAIMS[name] = lambda c, info: len(set(c[6]["minimizer"].tolist())) == n and (n > SCAN_ONE) == (name == "buckets_%d" % (SCAN_ONE + 1))
        return (21, 11, 1) + s.done()
    case("buckets_%d" % _n)(_buckets)


# ------------------------------------------------------------------------------------------------ the table

@functools.lru_cache(maxsize=None)
def build_cases():
    """-> {name: (name, k, m, abundance, bases, rec_off, stream, file_sk)}, in table order"""
    out = {}
    for name, fn in _BUILDERS:
        assert name not in out
        out[name] = (name,) + tuple(fn(name))
    return out


NAMES = [n for n, _ in _BUILDERS]


def params(k, m, ab):
    return sp.make_params(k, m, RATE, ab)


def small(c):
    return total_places(c[1], c[6]) <= MODEL_MAX


def file_slice(c, f):
    """file f of a case on its own: its stretch of the stream with the records it uses rebased to start at 0"""
    _, k, m, ab, b, off, st, fsk = c
    mine = st[int(fsk[f]): int(fsk[f + 1])].copy()
    if len(mine) == 0:
        return b[:0], np.zeros(1, np.uint64), mine
    r0, r1 = int(mine["rec"].min()), int(mine["rec"].max()) + 1
    mine["rec"] -= r0
    return b[int(off[r0]): int(off[r1])], off[r0: r1 + 1] - off[r0], mine


@functools.lru_cache(maxsize=None)
def modelled(name):
    """-> [(payload, counters, info) per file] of a small case"""
    c = build_cases()[name]
    return [S.model(c[1], c[2], c[3], RATE, *file_slice(c, f)) for f in range(len(c[7]) - 1)]


@functools.lru_cache(maxsize=None)
def hosted(name):
    """-> [(payload, counters) per file] by the host builder"""
    c = build_cases()[name]
    out = []
    for f in range(len(c[7]) - 1):
        payload, st = sp.sketch_build(params(c[1], c[2], c[3]), RATE, *file_slice(c, f))
        out.append((payload, {n: st[n] for n in S.COUNTERS}))
    return out


def expected(name):
    if small(build_cases()[name]):
        return [(p, cnt) for p, cnt, _ in modelled(name)]
    return hosted(name)


# ------------------------------------------------------------------------------------------------ CPU: the model, the host builder, the cases

SCAN_MADE = [(31, 11, 4.0, 1), (63, 15, 3.0, 2), (21, 11, 1.0, 1), (33, 13, 5.0, 1), (15, 15, 2.0, 1), (31, 11, 1.0, 2)]


@pytest.mark.parametrize("k,m,s,ab", SCAN_MADE)
def test_the_model_is_the_oracle_on_scan_made_streams(k, m, s, ab):
    from supersampler_amd import synth
    rng = np.random.default_rng(9)
    a = synth.random_genome(rng, 6000).tobytes()
    text = b">a\n" + a + b"\n>b\n" + S.revcomp(a[1000:3000]) + a[:500] + b"\n>hp\n" + b"A" * 300 + b"\n"
    b, off = orc.clean_fasta(text)
    em, _ = orc.scan(k, m, orc.threshold(k, m, s), b, off)
    want, wst = orc.sketch_fasta(text, k, m, s, ab)
    got, cnt, _ = S.model(k, m, ab, s, b, off, em)
    assert len(em) > 50
    assert got == want
    assert cnt == {n: wst[n] for n in S.COUNTERS}


def test_the_host_builder_is_the_model_on_every_small_case():
    n = 0
    for name in NAMES:
        if not small(build_cases()[name]):
            continue
        assert hosted(name) == [(p, cnt) for p, cnt, _ in modelled(name)], name
        n += 1
    assert n >= len(NAMES) - 4


def test_the_names_are_distinct():
    assert len(set(NAMES)) == len(NAMES)


def test_the_cases_are_what_they_are_called():
    """every case's claim from the model's instrumentation alone (the four cases beyond the model: from the stream), and every
    stream truthful: the minimizer in every k-mer of its oriented super-k-mer, every entry inside its record"""
    cases = build_cases()
    assert set(CLAIMS) == set(NAMES)
    for name in NAMES:
        c = cases[name]
        _, k, m, ab, b, off, st, fsk = c
        n_rec = len(off) - 1
        assert int(off[0]) == 0 and (np.diff(off.astype(np.int64)) >= 0).all() and int(off[-1]) == len(b), name
        assert int(fsk[0]) == 0 and int(fsk[-1]) == len(st) and (np.diff(fsk.astype(np.int64)) >= 0).all(), name
        assert set(np.unique(b).tolist()) <= set(b"ACGT"), name
        rec = st["rec"].astype(np.int64)
        assert (rec < n_rec).all() and (st["len"] >= k).all() and (st["rev"] <= 1).all() and (st["minimizer"] < 4 ** m).all(), name
        rlen = (off[1:] - off[:-1]).astype(np.int64)
        assert (st["start"].astype(np.int64) + st["len"] <= rlen[rec]).all(), name
        if len(st) > 50000:                                          # one k-mer each over one record: vectorised
            assert (st["len"] == k).all() and (st["rev"] == 0).all() and n_rec == 1, name
            code = ((b >> 1) & 3).astype(np.uint32)
            start = st["start"].astype(np.int64)
            holds = np.zeros(len(st), bool)
            for at in range(k - m + 1):
                v = np.zeros(len(st), np.uint32)
                for j in range(m):
                    v = (v << 2) | code[start + at + j]
                holds |= v == st["minimizer"]
            assert holds.all(), name
        else:
            whole = b.tobytes()
            for r, mn, start, ln, rev in S.entries(st):
                seq = whole[int(off[r]) + start: int(off[r]) + start + ln]
                if rev:
                    seq = S.revcomp(seq)
                x = S.bases(mn, m)
                at, last = seq.find(x), -1
                assert at >= 0, name
                while at >= 0:                                       # no stretch of more than k - m + 1 starts without one
                    assert at - last <= k - m + 1, name
                    last, at = at, seq.find(x, at + 1)
                assert len(seq) - m - last <= k - m, name
        info = None
        if small(c):
            per_file = modelled(name)
            info = per_file[0][2] if len(per_file) == 1 else None
        else:
            assert name in ("tiles_128", "tiles_129", "buckets_%d" % SCAN_ONE, "buckets_%d" % (SCAN_ONE + 1)), name
        if len(fsk) == 2:
            assert info is not None or not small(c), name
        assert CLAIMS[name](c, info), name
    # the cases of more than one file, file by file
    files = modelled("files_merge_a2")
    assert [cnt["seen_superkmers_at_reconstruction"] for _, cnt, _ in files] == [0, 0, 0, 0, 6]
    assert all(cnt["seen_kmers_at_reconstruction"] == 15 and cnt["actual_minimizer_number"] == 3 for _, cnt, _ in files)
    assert len({p for p, _, _ in files[:4]}) == 1
    files = modelled("files_empty")
    assert [cnt["actual_minimizer_number"] for _, cnt, _ in files] == [0, 3, 0, 0, 2, 0, 3, 0]
    for nf in (5, 257):
        files = modelled("files_%d" % nf)
        assert len(files) == nf and len({p for p, _, _ in files}) == nf and all(len(i["buckets"]) == 2 for _, _, i in files)
    # what the sort's stability shows in: two unrelated k-mers of one bucket in either stream order give different bytes
    c = cases["sort_n2"]
    two = c[6][[0, 0]].copy()
    two[1]["rec"] = 1
    assert S.model(31, 11, 1, RATE, c[4], c[5], two)[0] != S.model(31, 11, 1, RATE, c[4], c[5], two[::-1])[0]


def test_the_library_exports_the_entry():
    assert "spsp_sketch_build_device" in sp.ABI_SYMBOLS and hasattr(sp.lib(), "spsp_sketch_build_device")


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def run(ctx, name, packed):
    c = build_cases()[name]
    return ctx.sketch_build_device(params(c[1], c[2], c[3]), RATE, c[4], c[5], c[6], c[7], packed=bool(packed))


def check(ctx, name, packed):
    payloads, counters = run(ctx, name, packed)
    want = expected(name)
    assert len(payloads) == len(want)
    for f, (p, cnt) in enumerate(want):
        assert counters[f] == cnt, (name, packed, f)
        assert payloads[f] == p, (name, packed, f)


def _forms():
    return [pytest.param(n, f, id="%s-%s" % (n, "packed" if f else "ascii")) for n in NAMES for f in FORMS.get(n, (0, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,packed", _forms())
def test_the_device_builder_is_the_model(ctx, name, packed):
    check(ctx, name, packed)


@pytest.mark.gpu
def test_no_stream_gives_header_lines(ctx):
    for nf in (1, 3):
        payloads, counters = ctx.sketch_build_device(params(31, 11, 1), RATE, np.zeros(0, np.uint8), np.zeros(1, np.uint64),
                                                     np.zeros(0, sp.SUPERKMER_DTYPE), [0] * (nf + 1))
        assert payloads == [b"51 11 0 %f\n" % RATE] * nf
        assert counters == [dict.fromkeys(S.COUNTERS, 0)] * nf


@pytest.mark.gpu
def test_one_context_over_many_calls():
    """a context of the test's own: the largest case, the smallest, k = 63, k = 31, with whole sketches of texts in between
    (they share the pinned scan-total words and the base buffers with the builder); every result is a fresh context's"""
    from supersampler_amd import synth
    order = [("tiles_129", 0), ("sort_n1", 1), ("km_63_15", 1), ("km_31_11", 0), ("buckets_%d" % (SCAN_ONE + 1), 1), ("packed_tail_15", 1),
             ("sort_n1", 0)]
    text = synth.to_fasta(synth.random_genome(np.random.default_rng(3), 30000), "g", n_records=2)
    want_text = orc.sketch_fasta(text, 31, 11, 20.0)[0]
    alone = []
    for name, packed in order:
        with sp.Context(0) as fresh:
            alone.append(run(fresh, name, packed))
    with sp.Context(0) as c:
        for (name, packed), want in zip(order, alone):
            assert run(c, name, packed) == want, name
            assert c.sketch_text(text, 31, 11, 20.0)[0] == want_text, name
    for (name, packed), got in zip(order, alone):
        assert [(p, cnt) for p, cnt in zip(*got)] == expected(name), name


def refusals():
    """-> [(what, changed arguments of a valid call, text the message holds, does the host builder refuse it too)]"""
    c = build_cases()["km_31_11"]
    st = c[6]

    def entry(i, **kw):
        out = st.copy()
        for f, v in kw.items():
            out[i][f] = v
        return out
    n = len(st)
    rlen = int(c[5][int(st[3]["rec"]) + 1] - c[5][int(st[3]["rec"])])
    return [
        ("rec", dict(stream=entry(3, rec=len(c[5]) - 1)), "super-k-mer 3 is outside its record", True),
        ("len < k", dict(stream=entry(0, len=30)), "super-k-mer 0 is outside its record", True),
        ("end", dict(stream=entry(3, len=rlen + 1)), "super-k-mer 3 is outside its record", True),
        ("start", dict(stream=entry(n - 1, start=2 ** 63)), "super-k-mer %d is outside its record" % (n - 1), True),
        ("minimizer", dict(stream=entry(2, minimizer=4 ** 11)), "super-k-mer 2", False),
        ("rev", dict(stream=entry(5, rev=2)), "super-k-mer 5", False),
        ("file_sk start", dict(file_sk=[1, n]), "file_sk", False),
        ("file_sk order", dict(file_sk=[0, 5, 4, n]), "file_sk", False),
        ("file_sk end", dict(file_sk=[0, n - 1]), "file_sk", False),
        ("file_sk end", dict(file_sk=[0, n + 1]), "file_sk", False),
        ("no file", dict(file_sk=[0]), "n_files", False),
        ("m", dict(params=sp.make_params(31, 16, threshold_value=1)), "m=16", True),
        ("k", dict(params=sp.make_params(64, 11, threshold_value=1)), "k=64", True),
        ("k < m", dict(params=sp.make_params(9, 11, threshold_value=1)), "k=9", True),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [0, 1])
def test_refusals(ctx, packed):
    c = build_cases()["km_31_11"]
    good = dict(params=params(31, 11, 1), bases=c[4], rec_off=c[5], stream=c[6], file_sk=c[7])
    want = expected("km_31_11")

    def call(a):
        if len(a["file_sk"]) == 1:                                   # (n_files == 0: not through the binding, which sizes its outputs by it)
            out = sp.C.c_void_p()
            off, cnt = np.zeros(1, np.uint64), np.zeros(4, np.uint64)
            fsk = np.zeros(1, np.uint32)
            sp._check(sp.lib().spsp_sketch_build_device(ctx._h, sp.C.byref(a["params"]), RATE, a["bases"].ctypes.data, a["rec_off"].ctypes.data,
                                                        len(a["rec_off"]) - 1, a["stream"].ctypes.data, len(a["stream"]), fsk.ctypes.data, 0, packed,
                                                        sp.C.byref(out), off.ctypes.data, cnt.ctypes.data))
        return ctx.sketch_build_device(a["params"], RATE, a["bases"], a["rec_off"], a["stream"], a["file_sk"], packed=bool(packed))

    for what, change, text, host_too in refusals():
        a = dict(good, **change)
        with pytest.raises(sp.SpspError) as e:
            call(a)
        assert e.value.code == sp.ERR_ARG and text in str(e.value), what
        if host_too and "file_sk" not in change:
            with pytest.raises(sp.SpspError) as h:
                sp.sketch_build(a["params"], RATE, a["bases"], a["rec_off"], a["stream"])
            assert h.value.code == sp.ERR_ARG and str(h.value) == str(e.value), what
        got = call(good)                                             # a refusal leaves the context as it was
        assert [(p, cnt) for p, cnt in zip(*got)] == want, what
    # NULL arguments, one at a time
    L, C = sp.lib(), sp.C
    st, fsk = np.ascontiguousarray(c[6]), np.ascontiguousarray(c[7])
    out, off, cnt = C.c_void_p(), np.zeros(2, np.uint64), np.zeros(4, np.uint64)
    p = params(31, 11, 1)
    args = [ctx._h, C.byref(p), RATE, c[4].ctypes.data, c[5].ctypes.data, len(c[5]) - 1, st.ctypes.data, len(st), fsk.ctypes.data, 1, packed,
            C.byref(out), off.ctypes.data, cnt.ctypes.data]
    for i in (0, 1, 3, 4, 6, 8, 11, 12, 13):
        bad = list(args)
        bad[i] = None
        assert L.spsp_sketch_build_device(*bad) == sp.ERR_ARG, i
        assert b"NULL" in L.spsp_last_error(), i
        assert out.value is None and not off.any() and not cnt.any(), i
    got = call(good)
    assert [(p_, cnt_) for p_, cnt_ in zip(*got)] == want
