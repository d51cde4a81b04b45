"""The sketch decoder (spsp_sketch_decode_device: spsp_decode.hip, spsp_bigkeys.hip) on hand-built payloads at its seams.

Every comparator feature reads its keys through this one path, and sketches of random genomes meet its boundaries by luck
or never: two keys that differ in ONE of (minimizer, kmer_hi, kmer_lo), a sketch of exactly the LDS sort's capacity, a bucket
of 256 keys, a large sketch that is not last in its batch, the table's 8-bit epoch wrapping.  The payloads below are written
byte by byte (tests/payloads.py) so that each of these is met on purpose, and the expectation is always payloads.model():
plain Python integers, exact equality, no tolerance.

decode_cases() is the one table: (name, k, m, [payloads], [expected keys per sketch]).  BUCKETS[name] keeps what each payload
was written from, so that test_the_cases_are_what_they_are_called can count raw keys, distinct keys, bucket sizes and tiles
from the model alone -- a case cannot drift off its seam unnoticed.

What a wrong kernel would look like, and where it shows:
    a comparison that leaves out kmer_hi (counting rank, network, unique pass, table, merge): oneword_* at k = 63
    a comparison that leaves out the minimizer: the same k-mer under two minimizers, in oneword_*
    a capacity, tile or stride off by one: sizes_*, big_d*, buckets_*, launches_*
    a large sketch's slice taken from the wrong place: batch_large_*
    a slot of an old call read as this call's: test_one_context_over_many_calls"""
import collections
import functools
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import payloads as P
import supersampler_amd as sp
from oracle import oracle_py as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = 0x9E3779B97F4A7C15
TILE = 2048                                      # keys per workgroup of the merge sort (kBigTile)
BUCKET_MAX = 256                                 # the counting sort's largest bucket (kBucketMax)
STRIDE = 1024                                    # lanes of k_decode_sort
KM = [(31, 11), (32, 12), (33, 13), (63, 15), (21, 9)]

BUCKETS = {}                                     # name -> [buckets of sketch 0, of sketch 1, ...]
HOST = {}                                        # name -> indices of the sketches written so that the host decodes them
CLAIMS = {}                                      # name -> what the name claims, checked on the CPU
NO_ORACLE = {}                                   # name -> indices of the sketches the oracle cannot read (see first_byte below)


def cap(k):
    """raw keys the LDS sort holds (kSortCapLo / kSortCapHi)"""
    return 4096 if k > 32 else 8192


def per_lane(k):
    """consecutive keys a lane of the unique pass holds"""
    return cap(k) // STRIDE


def merge_passes(distinct):
    n, run = 0, TILE
    while run < distinct:
        n, run = n + 1, run * 2
    return n


# ------------------------------------------------------------------------------------------------ building blocks

def rnd(rng, n):
    return bytes(rng.choice(P.LETTERS) for _ in range(n))


def kmer_line(k, m, i, salt=0):
    """(prefix, suffix) of k bases in all around an m-base minimizer: 'A', then k - m - 2 bases that are a one-to-one mix of
    i, then 'C'.  Whatever the minimizer, the k-mer is its own canonical form (its reverse complement starts with G), so
    different i give different keys, and both halves of the k-mer vary with i."""
    nf = k - m - 2
    x = ((i + 1) * GOLD + salt * 0xD6E8FEB86659FD93) & ((1 << (2 * nf)) - 1)
    b = P.bases(x, nf)
    p = (k - m) // 2
    return b"A" + b[: p - 1], b[p - 1:] + b"C"


def minimizer(m, j):
    """the j-th minimizer of a filler: ascending with j, never all A (oneword's and repeats' own)"""
    return P.bases(0x1000 + 37 * j, m)


def filler(k, m, n, bucket=40, first=0, reps=1, salt=0):
    """buckets of `bucket` one-k-mer lines under ascending minimizers, n different keys in all, every line written reps times"""
    out = []
    j = 0
    while n > 0:
        c = min(bucket, n)
        lines = [kmer_line(k, m, i, salt + 1000 * (first + j)) for i in range(c)]
        out.append((minimizer(m, first + j), [], lines * reps))
        n -= c
        j += 1
    return out


def ascending(buckets):
    out = sorted(buckets, key=lambda b: P.to_int(b[0]))
    assert len({b[0] for b in out}) == len(out)
    return out


def one_bucket(k, m, j, n, salt=0, reps=1):
    return (minimizer(m, j), [], [kmer_line(k, m, i, salt + 1000 * j) for i in range(n)] * reps)


def oneword(k, m):
    """-> ([buckets of the main sketch, of two sketches of two keys], pairs, minimizers to find buckets by): keys that differ in one word only, written larger key first so that a rank that ignores the
    differing word keeps the payload's (wrong) order.  pairs: [(key, key, the word that differs)] for the CPU check."""
    rng = random.Random(100 + k)
    p = 40 if k == 63 else 13                                        # k = 63: kmer_hi (the first 31 bases) lies inside the prefix
    s = k - m - p
    mn = b"C" + rnd(rng, m - 1)
    pre, suf = b"A" + rnd(rng, p - 1), rnd(rng, s - 1) + b"C"
    pre_hi = pre[:5] + (b"G" if pre[5:6] != b"G" else b"T") + pre[6:]         # another base among the first 15: the high word
    suf_lo = suf[:2] + (b"G" if suf[2:3] != b"G" else b"T") + suf[3:]         # another base among the last 16: the low word
    # the same k-mer under two minimizers: it holds both m-mers, so it is stored in two buckets with different splits
    whole = pre + mn + suf
    q = p - 3
    mn2 = whole[q: q + m]
    assert mn2 != mn
    key = lambda bucket, line: (P.to_int(bucket[0]), P.canonical_windows(k, line[0] + bucket[0] + line[1])[0])
    three = sorted([(pre_hi, suf), (pre, suf_lo), (pre, suf)], key=lambda line: key((mn,), line), reverse=True)
    a = (mn, [], three + [(pre, suf)])                               # ... and the same key stored twice
    b = (mn2, [], [(whole[:q], whole[q + m:])])
    k0 = key(a, (pre, suf))
    pairs = [(key(a, (pre_hi, suf)), k0, "hi"), (key(a, (pre, suf_lo)), k0, "lo"), (key(b, b[2][0]), k0, "mn")]
    # kmer_hi falls where kmer_lo rises, over a whole bucket: an order by kmer_lo alone is the reverse of the right one
    anti = []
    for i in range(60):
        hi_part = P.bases(59 - i, 6)
        lo_part = P.bases(i, 6)
        anti.append((b"A" + hi_part + pre[7:], lo_part + suf[6:]) if s >= 7 else (b"A" + hi_part + pre[7: p - 6] + lo_part, suf))
    c = (b"G" + mn[1:], [], anti)
    # ten keys with one kmer_lo (and one minimizer): in sorted order every neighbour differs in kmer_hi alone
    d = (b"T" + mn[1:], [], [(b"A" + P.bases(9 - i, 6) + pre[7:], suf) for i in range(10)])
    # a sketch of two keys that differ in the minimizer alone, so that they are neighbours in sorted order; and written descending
    twin = ascending([(mn, [], [(pre, suf)]), b])
    return [[a, b, c, d], twin, twin[::-1]], pairs, (P.to_int(c[0]), P.to_int(d[0]))


def words(k, key):
    """the words a comparison can leave out: (minimizer, kmer_hi, kmer_lo); at k <= 32 the halves of kmer_lo stand in"""
    mn, v = key
    return (mn, v >> 64, v & P.U64) if k > 32 else (mn, v >> 32, v & 0xFFFFFFFF)


def straddle(k, m):
    """one sketch whose SORTED raw keys hold equal neighbours across the unique pass's lane boundaries (every per_lane keys)
    and wave boundaries (every 64 * per_lane keys): the second copy is the first key of a lane / of a wave"""
    per = per_lane(k)
    at = [per, 5 * per, 64 * per, 128 * per, 128 * per + per]        # sorted raw positions of the second copies
    buckets = filler(k, m, 128 * per + 2 * per + 20, salt=7)
    ranked = sorted((P.to_int(b[0]), P.canonical_windows(k, ln[0] + b[0] + ln[1])[0], bi, li)
                    for bi, b in enumerate(buckets) for li, ln in enumerate(b[2]))
    extra = {}
    for t, q in enumerate(at):
        _, _, bi, li = ranked[q - 1 - t]                             # t copies in front have moved it up by t
        extra.setdefault(bi, []).append(buckets[bi][2][li])
    return [(b[0], b[1], b[2] + extra.get(bi, [])) for bi, b in enumerate(buckets)], at


def emit_shapes(k, m):
    """-> sketches (bucket lists) with one bucket per shape of a super-k-mer"""
    rng = random.Random(k * 100 + m)
    h = k - m
    mns = sorted({rnd(rng, m) for _ in range(40)}, key=P.to_int)
    nxt = iter(mns)
    if k == m:
        lines = [(rnd(rng, a), rnd(rng, b)) for a, b in [(0, 1), (1, 0), (1, 1), (0, 255), (255, 0), (255, 255), (7, 9)]]
        s0 = [(mn, [], []) for mn in mns[:30]] + [(mns[30], [], lines), (b"G" * m, [], []), (b"G" * m, [], [(b"", b"G")])]
        return [s0, [(mns[31], [], [])], []]
    s0 = [(next(nxt), [(rnd(rng, h), rnd(rng, h))], []), (next(nxt), [(rnd(rng, h), rnd(rng, h)) for _ in range(2)], [])]
    shapes = [(0, 255), (1, h), (h, 1), (255, 0), (255, 255), (h, h),            # prefix and suffix of 0, 1, k - m, 255; k + 1; 2k - m as a line
              (0, h), (h, 0), (h // 2, h - h // 2),                              # exactly k: one k-mer
              (0, h + 1), (h - 1, h), (h, h - 1),                                # k + 1, 2k - m - 1
              (0, h - 1), (h - 1, 0), (h // 2, h - h // 2 - 1), (1, 0), (0, 1)]  # k - 1 and less: no k-mer
    for a, b in shapes:
        s0.append((next(nxt), [], [(rnd(rng, a), rnd(rng, b))]))
    s0.append((next(nxt), [(rnd(rng, h), rnd(rng, h))], [(rnd(rng, 3), rnd(rng, h)), (rnd(rng, h), rnd(rng, 2))]))   # a blob and lines
    if m == 15:
        s0.append((b"G" * m, [], [(rnd(rng, h), rnd(rng, h))]))                  # the largest minimizer: 30 set bits
    if k == 32:
        half = rnd(rng, 16)
        pal = half + P.revcomp(half)                                             # its own reverse complement
        s0.append((pal[10: 10 + m], [], [(pal[:10], pal[10 + m:])]))
        top = b"G" + rnd(rng, 30) + b"A"                                         # forward and reverse both start with G or T: bit 63 of kmer_lo
        s0.append((top[4: 4 + m], [], [(top[:4], top[4 + m:])]))
    if k == 63:
        x = rnd(rng, 31)                                                         # forward and reverse complement agree in kmer_hi, differ in kmer_lo
        s0.append((x[5: 5 + m], [], [(x[:5], x[5 + m:] + mid + P.revcomp(x)) for mid in (b"A", b"C")]))
    s0 = ascending(s0)
    s1 = [(next(nxt), [(rnd(rng, h), rnd(rng, h)) for _ in range(300)], [])]
    s2 = [(next(nxt), [], [(rnd(rng, 0), rnd(rng, h - 1))])]                     # only a line of k - 1 bases: an empty sketch
    return [s0, s1, s2]


def descriptors(k, m, n):
    """one sketch of n stored super-k-mers, one k-mer each (k == m: n bare minimizers)"""
    if k == m:
        return [(P.bases(5 + 3 * j, m), [], []) for j in range(n)]
    return filler(k, m, n, bucket=30, salt=11)


def with_big_bucket(k, m, n, big, where, salt):
    """n raw keys in buckets of 40 and one bucket of `big` keys, the first / a middle / the last of the sketch"""
    small = filler(k, m, n - big, salt=salt)
    at = {"first": 0, "middle": len(small) // 2, "last": len(small)}[where]
    out = small[:at] + [None] + small[at:]
    # ascending minimizers: the filler's j-th minimizer grows with j, so the big bucket takes number `at` and the rest move up
    return [one_bucket(k, m, j, big, salt) if b is None else (minimizer(m, j), b[1], b[2]) for j, b in enumerate(out)]


def large(k, m, distinct, salt=0, first=0):
    """a sketch for the table in HBM: more than cap raw keys, `distinct` different ones (every line written reps times)"""
    reps = cap(k) // distinct + 1
    return filler(k, m, distinct, first=first, reps=reps, salt=salt)


def poly_a(k, m, times):
    """the key (A^m, A^k) stored `times` times: maximal super-k-mers of A (k - m + 1 windows each) and one line for the rest"""
    h = k - m
    full, rest = divmod(times, h + 1)
    lines = [(b"", b"A" * (h + rest - 1))] if rest else []
    return (b"A" * m, [(b"A" * h, b"A" * h)] * full, lines)


# ------------------------------------------------------------------------------------------------------ the table

@functools.lru_cache(maxsize=None)
def decode_cases():
    cases = []

    def add(name, k, m, sketches, host=(), writer=None, **claims):
        """sketches: bucket lists; writer[i]: payload() arguments of sketch i"""
        assert name not in BUCKETS
        writer = writer or {}
        BUCKETS[name], HOST[name], CLAIMS[name] = sketches, tuple(host), claims
        # behind a non-zero first blob byte the writer leaves part of a super-k-mer: spsp_sketch_parse_host passes it by, the
        # reference's walk (and the oracle's, line for line) runs off the end of it and throws
        NO_ORACLE[name] = tuple(i for i, w in writer.items() if w.get("first_byte"))
        cases.append((name, k, m, [P.payload(k, m, b, **writer.get(i, {})) for i, b in enumerate(sketches)],
                      [P.model(k, m, b) for b in sketches]))

    # a. emit: the shapes of a super-k-mer
    for k, m in KM + [(15, 15)]:
        add("emit_shapes_k%d_m%d" % (k, m), k, m, emit_shapes(k, m), both_orientations=k != m, large=[1] if k > 32 else [])
        for n in (255, 256, 257):
            add("emit_descriptors_%d_k%d_m%d" % (n, k, m), k, m, [descriptors(k, m, n)], raw=[n])

    for k, m in [(31, 11), (63, 15)]:
        c, tag = cap(k), "_k%d" % k
        # b. keys that differ in one word only: counting path, network path, inside a large sketch
        ow, pairs, anti = oneword(k, m)
        add("oneword_counting" + tag, k, m, [ascending(ow[0] + filler(k, m, 300, salt=1))] + ow[1:], pairs=pairs, anti=anti, max_bucket=60)
        add("oneword_network" + tag, k, m, [ascending(ow[0] + filler(k, m, 300, salt=1) + [one_bucket(k, m, 900, 300)])] + ow[1:], pairs=pairs, anti=anti, max_bucket=300)
        add("oneword_large" + tag, k, m, [ascending(ow[0] + filler(k, m, c, salt=1))] + ow[1:], pairs=pairs, anti=anti, large=[0])
        key = kmer_line(k, m, 12345, 5)
        for times in (2, 200, 300):
            dup = (minimizer(m, 500), [], [kmer_line(k, m, 0, 6)] + [key] * times + [kmer_line(k, m, i, 6) for i in range(1, 40)])
            add("repeat_%d" % times + tag, k, m, [ascending(filler(k, m, 200, salt=2) + [dup])], max_bucket=times + 40, distinct=[241])
        sk, at = straddle(k, m)
        add("straddle" + tag, k, m, [sk], equal_at=at)
        # c. sizes
        add("sizes_small" + tag, k, m, [filler(k, m, n, salt=n) for n in (1, 2, 63, 64, 65, 1023, 1024, 1025)], raw=[1, 2, 63, 64, 65, 1023, 1024, 1025])
        add("sizes_cap" + tag, k, m, [filler(k, m, c - 1, salt=3), filler(k, m, c, salt=4)], raw=[c - 1, c], large=[])
        add("sizes_cap_plus_1" + tag, k, m, [filler(k, m, c + 1, salt=5)], raw=[c + 1], distinct=[c + 1], large=[0])
        add("sizes_cap_plus_1_few_distinct" + tag, k, m, [filler(k, m, 101, reps=c // 101, salt=5) + [one_bucket(k, m, 10, 1, 5, reps=c + 1 - 101 * (c // 101))]],
            raw=[c + 1], distinct=[102], large=[0])
        for d in (2047, 2048, 2049, 4096, 4097, 3 * TILE, 5 * TILE, 8 * TILE + 1):
            add("big_d%d" % d + tag, k, m, [large(k, m, d, salt=d)], distinct=[d], large=[0], passes=merge_passes(d))
        add("big_two_pass_counts" + tag, k, m, [large(k, m, 2049, salt=21), filler(k, m, 70, salt=22), large(k, m, 5 * TILE, salt=23)],
            distinct=[2049, 70, 5 * TILE], large=[0, 2])
        if k == 31:      # 65 536 lines
            wrap = [(b"A" * m, [], [(b"", b"A" * (k - m))] * 65536), (b"C" * m, [], [kmer_line(k, m, 1, 8)] * 256)] + filler(k, m, 500, salt=8)
        else:            # the same count out of a blob
            wrap = [poly_a(k, m, 65536), (b"C" * m, [], [kmer_line(k, m, 1, 8)] * 256)] + filler(k, m, 500, salt=8)
        add("big_occurrences_wrap" + tag, k, m, [wrap], raw=[65536 + 256 + 500], distinct=[502], large=[0])
        # d. buckets and the choice of sort
        for size in (255, 256, 257):
            add("buckets_%d" % size + tag, k, m, [with_big_bucket(k, m, size + 400, size, w, size) for w in ("first", "middle", "last")], max_bucket=size)
        add("buckets_across_1024" + tag, k, m, [filler(k, m, 1000, salt=9) + [one_bucket(k, m, 100, 100, 9)] + filler(k, m, 200, first=101, salt=9)],
            bucket_over=1024, max_bucket=100)
        base = filler(k, m, 1100, bucket=32, salt=10)                # bucket boundaries on every multiple of 32: one lies at 1024
        swap = lambda b, i: b[:i] + [b[i + 1], b[i]] + b[i + 2:]
        add("order_first_two_swapped" + tag, k, m, [swap(base, 0)], inversions=[32])
        add("order_last_two_swapped" + tag, k, m, [swap(base, len(base) - 2)], inversions=[1068])
        add("order_inversion_at_1024" + tag, k, m, [swap(base, 31)], inversions=[1024])
        add("order_descending" + tag, k, m, [base[::-1]], inversions=None)
        q = 2 if k > 32 else 1                                       # the k = 63 sizes are halved
        a, b, d = 4800 // q, 4500 // q, 3000 // q
        two = [filler(k, m, a, salt=12), filler(k, m, b - 300, salt=13) + [one_bucket(k, m, 800, 300, 13)], filler(k, m, d - 300, salt=14) + [one_bucket(k, m, 800, 300, 14)]]
        add("launches_two" + tag, k, m, two, raw=[a, b, d], max_bucket=300, cap1=(a + 63) & ~63)
        add("launches_one" + tag, k, m, [filler(k, m, c, salt=15)] + two[1:], raw=[c, b, d], max_bucket=300, cap1=c)
        # e. batches
        S = [filler(k, m, 50, salt=30 + i) for i in range(3)]
        L = [large(k, m, d, salt=40 + i) for i, d in enumerate((2100, 700, 4200))]
        E = []
        add("batch_large_first" + tag, k, m, [L[0], S[0], S[1]], large=[0])
        add("batch_large_middle" + tag, k, m, [S[0], L[0], S[1]], large=[1])
        add("batch_large_last" + tag, k, m, [S[0], S[1], L[0]], large=[2])
        add("batch_large_adjacent" + tag, k, m, [S[0], L[0], L[1], S[1]], large=[1, 2])
        add("batch_large_all" + tag, k, m, [L[0], L[1], L[2]], large=[0, 1, 2])
        add("batch_large_identical" + tag, k, m, [L[0], L[0]], large=[0, 1], identical=(0, 1))
        add("batch_large_between_empty" + tag, k, m, [E, L[1], E], large=[1], raw=[0, c // 700 * 700 + 700, 0])
        # sketches the host decodes: a non-zero first blob byte, a 256-base line, a payload that ends inside a line
        rng = random.Random(k)
        h = k - m
        blobbed = filler(k, m, 60, salt=50)[:1] + [(minimizer(m, 3), [(rnd(rng, h), rnd(rng, h)) for _ in range(4)], [kmer_line(k, m, 0, 51)])] + filler(k, m, 60, first=5, salt=50)
        longline = filler(k, m, 60, salt=52) + [(minimizer(m, 9), [], [(rnd(rng, 256), rnd(rng, 3)), (rnd(rng, 2), rnd(rng, 300))])]
        openend = filler(k, m, 60, salt=53) + [(minimizer(m, 9), [], [(rnd(rng, h + 5), b"")])]
        heavy = filler(k, m, 3000, salt=54) + [(minimizer(m, 900), [], [(rnd(rng, 256), rnd(rng, 3))])]
        W = {"blob": dict(first_byte=3), "long": dict(long_lines=True), "open": dict(cut=4)}
        add("batch_host_first" + tag, k, m, [blobbed, S[0], L[1]], host=[0], writer={0: W["blob"]}, large=[2])
        add("batch_host_last" + tag, k, m, [L[1], S[0], longline], host=[2], writer={2: W["long"]}, large=[0])
        add("batch_host_beside_large" + tag, k, m, [S[0], openend, L[1], blobbed], host=[1, 3], writer={1: W["open"], 3: W["blob"]}, large=[2])
        add("batch_host_largest" + tag, k, m, [S[0], heavy, S[1]], host=[1], writer={1: W["long"]}, large=[])
        add("batch_all_host" + tag, k, m, [blobbed, longline, openend], host=[0, 1, 2], writer={0: W["blob"], 1: W["long"], 2: W["open"]}, large=[])
        # payloads that stop early and are still what the sketcher's reader takes: the device decodes them
        add("batch_short_ends" + tag, k, m, [S[0], S[1], S[2] + [(minimizer(m, 900), [], [(rnd(rng, 4), rnd(rng, h))])]], writer={0: dict(cut=2), 1: dict(cut=1), 2: dict(cut=3)})

    # k - m odd: a blob byte straddles two super-k-mers, every sketch takes the host decoder
    k, m = 32, 15
    rng = random.Random(3215)
    odd = lambda salt: [(minimizer(m, 1), [(rnd(rng, 17), rnd(rng, 17)) for _ in range(2)], [kmer_line(k, m, i, salt) for i in range(20)])] + filler(k, m, 90, first=2, salt=salt)
    add("batch_k32_m15", k, m, [odd(1), [], odd(2), filler(k, m, 5000, salt=3)], host=[0, 1, 2, 3], large=[])
    # many tiny sketches: the structure walk moves to the device at 256 sketches, in blocks of 64
    k, m = 31, 11
    for n in (255, 256, 257):
        tiny = [filler(k, m, 1 + i % 7, first=i % 5, salt=i // 3) for i in range(n)]
        tiny[100] = []
        tiny[64] = tiny[64] + [(minimizer(m, 9), [], [(b"ACGT" * 64, b"G")])]
        add("batch_tiny_%d" % n, k, m, tiny, host=[64], writer={64: dict(long_lines=True), 191: dict(cut=2)}, n_sketches=n)
    return tuple(cases)


def case(name):
    return next(c for c in decode_cases() if c[0] == name)


# ------------------------------------------------------------------------------------------------------ CPU side

def test_the_cases_are_what_they_are_called():
    """from the model alone: raw counts, distinct counts, bucket sizes, merge passes and tiles, the one-word pairs, the
    positions of equal neighbours, which sketches are large -- what every case's name says it puts on a seam"""
    seen_passes = {31: set(), 63: set()}
    for name, k, m, payloads, expected in decode_cases():
        sketches, claims = BUCKETS[name], CLAIMS[name]
        raws = [P.raw_keys(k, m, b) for b in sketches]
        for r, e in zip(raws, expected):
            assert sorted(set(r)) == e, name
        if "raw" in claims:
            assert [len(r) for r in raws] == claims["raw"], name
        if "distinct" in claims:
            assert [len(e) for e in expected] == claims["distinct"], name
        if "large" in claims:            # exactly these go through the table in HBM
            assert [i for i, r in enumerate(raws) if len(r) > cap(k) and i not in HOST[name]] == claims["large"], name
        elif not HOST[name]:
            assert all(len(r) <= cap(k) for r in raws), name
        sizes = [max(collections.Counter(key[0] for key in r).values(), default=0) for r in raws]
        if "max_bucket" in claims:
            assert max(sizes) == claims["max_bucket"], (name, sizes)
            if name.startswith("buckets_2"):
                assert sizes == [claims["max_bucket"]] * 3
                for r, where in zip(raws, ("first", "middle", "last")):
                    big = [i for i, key in enumerate(r) if sum(1 for x in r if x[0] == key[0]) == claims["max_bucket"]]
                    assert (big[0] == 0) == (where == "first") and (big[-1] == len(r) - 1) == (where == "last"), name
        elif name.startswith(("sizes_small", "sizes_cap_k", "emit_descriptors", "straddle", "order_")):
            assert max(sizes) <= BUCKET_MAX, name        # the counting path, unless the order sends it to the network
        if "pairs" in claims:
            for a, b, word in claims["pairs"]:
                wa, wb = words(k, a), words(k, b)
                assert [x != y for x, y in zip(wa, wb)] == [word == "mn", word == "hi", word == "lo"], (name, word)
                assert a in expected[0] and b in expected[0], name
                # (written larger first, in one bucket, where the minimizer is the same)
                if word != "mn":
                    assert raws[0].index(max(a, b)) < raws[0].index(min(a, b)), name
            anti = [key for key in raws[0] if key[0] == claims["anti"][0]]
            ladder = [key for key in expected[0] if key[0] == claims["anti"][1]]
            assert len(anti) == 60 and len(ladder) == 10, name
            assert all(words(k, x)[2] == words(k, y)[2] and words(k, x)[1] < words(k, y)[1] for x, y in zip(ladder, ladder[1:])), name
            assert len(expected[1]) == 2 and expected[1][0][1] == expected[1][1][1] and expected[1] == expected[2] and raws[1] == raws[2][::-1], name
            if k > 32:               # kmer_hi falls where kmer_lo rises
                assert all(P.split(x[1])[0] > P.split(y[1])[0] and P.split(x[1])[1] < P.split(y[1])[1] for x, y in zip(anti, anti[1:])), name
            assert sum(1 for key in raws[0] if key == claims["pairs"][0][1]) == 2, name
        if "equal_at" in claims:
            order = sorted(raws[0])
            assert [i for i in range(1, len(order)) if order[i] == order[i - 1]] == claims["equal_at"], name
            per = per_lane(k)
            assert all(i % per == 0 for i in claims["equal_at"]) and sum(1 for i in claims["equal_at"] if i % (64 * per) == 0) == 2, name
        if "passes" in claims:
            assert merge_passes(len(expected[0])) == claims["passes"] and -(-len(expected[0]) // TILE) == -(-claims["distinct"][0] // TILE), name
            seen_passes[k].add(claims["passes"])
        if name.startswith("big_two_pass_counts"):
            assert merge_passes(len(expected[0])) != merge_passes(len(expected[2])), name
        if name.startswith("big_occurrences_wrap"):
            counts = sorted(raws[0].count(key) for key in (raws[0][0], raws[0][65536]))
            assert counts == [256, 65536], (name, counts)
        if "bucket_over" in claims:
            idx = [i for i, key in enumerate(raws[0]) if key[0] == raws[0][claims["bucket_over"]][0]]
            assert idx[0] < claims["bucket_over"] <= idx[-1] and idx == list(range(idx[0], idx[-1] + 1)), name
        if "inversions" in claims:
            mns = [key[0] for key in raws[0]]
            inv = [i for i in range(1, len(mns)) if mns[i] < mns[i - 1]]
            if claims["inversions"] is None:
                assert mns == sorted(mns, reverse=True) and len(inv) == len(sketches[0]) - 1, name
            else:
                assert inv == claims["inversions"], (name, inv)
        if "cap1" in claims:             # the first launch's arrays hold the largest sketch: who needs the second launch
            n2 = lambda n: 1 << (n - 1).bit_length()
            assert (max(len(r) for r in raws) + 63) & ~63 == claims["cap1"] <= cap(k), name
            assert (n2(len(raws[1])) > claims["cap1"]) == name.startswith("launches_two") and n2(len(raws[2])) <= claims["cap1"], name
            assert sizes[1] > BUCKET_MAX and sizes[2] > BUCKET_MAX and sizes[0] <= BUCKET_MAX, name
        if "identical" in claims:
            i, j = claims["identical"]
            assert payloads[i] == payloads[j], name
        if "both_orientations" in claims and claims["both_orientations"]:
            fwd = rev = 0
            for mn, maximal, lines in sketches[0]:
                for pre, suf in maximal + lines:
                    s = pre + mn + suf
                    for i, w in enumerate(P.canonical_windows(k, s)):
                        fwd += w == P.to_int(s[i: i + k])
                        rev += w != P.to_int(s[i: i + k])
            assert fwd > 10 and rev > 10, name
            if k == 32:
                assert any(w == P.to_int(P.revcomp(P.bases(w, 32))) for _, w in expected[0]) and any(w >> 63 for _, w in expected[0]), name
            if k == 63:
                assert sum(1 for (_, x), (_, y) in zip(expected[0], expected[0][1:]) if x >> 64 == y >> 64) >= 1, name
            if m == 15:
                assert expected[0][-1][0] == 4 ** 15 - 1, name
            assert expected[2] == [], name
        if "n_sketches" in claims:
            assert len(payloads) == claims["n_sketches"] and expected[100] == [], name
        # what makes a sketch the host's: the first byte of a blob, a line part over 255 bases, an end inside a line, k - m odd
        for i, (b, pl) in enumerate(zip(sketches, payloads)):
            pos = pl.index(b"\n") + 1
            odd_blob = False
            for mn, maximal, lines in b:
                n = int.from_bytes(pl[pos + m: pos + m + 4], "little")
                odd_blob |= n > 0 and pl[pos + m + 4] != 0
                pos += m + 4 + n + sum(len(p) + len(s) + 2 for p, s in lines) + 2
            open_end = len(b) > 0 and len(b[-1][2]) > 0 and b[-1][2][-1][1] == b"" and not pl.endswith(b"\n")
            signs = [odd_blob, any(len(p) > 255 or len(s) > 255 for _, _, lines in b for p, s in lines), open_end, (k - m) % 2 == 1]
            assert any(signs) == (i in HOST[name]), (name, i, signs)
    assert seen_passes[31] == seen_passes[63] == {0, 1, 2, 3, 4}


def test_the_model_is_the_oracle_and_the_host_decoder():
    """payloads.model() against the oracle's reading of the same bytes (orc.sketch_keys: the reference comparator's bucket walk)
    and against spsp_sketch_parse_host, the decoder that non-standard sketches are routed to, for every payload of the table.
    The library has no entry point that tells where a payload is routed: that the host's sketches went to the host shows
    on the GPU, where the device's reading of them differs (one super-k-mer too many behind a non-zero first blob byte, line
    lengths taken mod 256)."""
    for name, k, m, payloads, expected in decode_cases():
        for i, (pl, want) in enumerate(zip(payloads, expected)):
            sk = sp.sketch_parse(pl)
            got = [(int(a), (int(h) << 64) | int(l)) for a, l, h in zip(sk.minimizer, sk.kmer_lo, sk.kmer_hi)]
            assert (sk.k, sk.m) == (k, m) and got == want, (name, i, "host decoder")
            if i in NO_ORACLE[name]:
                assert i in HOST[name]
                continue
            ok, om, w_mn, w_lo, w_hi = orc.sketch_keys(pl)
            got = [(int(a), (int(h) << 64) | int(l)) for a, l, h in zip(w_mn, w_lo, w_hi)]
            if k == m and not want and len(got) == 1:
                continue             # the comparator's first-read rule gives an empty k == m sketch a phantom key: not the decoder's
            assert (ok, om) == (k, m) and got == want, (name, i, "oracle")


# ------------------------------------------------------------------------------------------------------ GPU side

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def check(ctx, case_, what=""):
    """one decode of a batch: sk_off, d_minimizer, d_kmer_lo, d_kmer_hi (None where k <= 32), sketch by sketch, exactly"""
    name, k, m, payloads, expected = case_
    kk, mm, d_mn, d_lo, d_hi, sk_off = ctx.sketch_decode_device(list(payloads))
    assert (kk, mm) == (k, m), (name, what)
    want_off = np.concatenate([[0], np.cumsum([len(e) for e in expected])]).astype(np.uint64)
    assert sk_off.tolist() == want_off.tolist(), (name, what, "sk_off", [int(x) for x in np.diff(sk_off.astype(np.int64))][:8], [len(e) for e in expected][:8])
    assert (d_hi is None) == (k <= 32), (name, what)
    total = int(want_off[-1])
    if total == 0:
        return
    mn, lo = ctx.to_host(d_mn, total, np.uint32), ctx.to_host(d_lo, total, np.uint64)
    hi = ctx.to_host(d_hi, total, np.uint64) if k > 32 else None
    for i, e in enumerate(expected):
        a, b = int(want_off[i]), int(want_off[i + 1])
        got = list(zip(mn[a:b].tolist(), lo[a:b].tolist() if hi is None else [(h << 64) | l for h, l in zip(hi[a:b].tolist(), lo[a:b].tolist())]))
        if got != e:
            j = next(j for j in range(len(e)) if got[j] != e[j])
            raise AssertionError("%s %s: sketch %d key %d of %d: got %r, want %r" % (name, what, i, j, len(e), got[j], e[j]))


def check_all(ctx, what=""):
    for c in decode_cases():
        check(ctx, c, what)


def _names():
    # (the names alone, so that collecting the file does not build the table)
    out = []
    for k, m in KM + [(15, 15)]:
        out += ["emit_shapes_k%d_m%d" % (k, m)] + ["emit_descriptors_%d_k%d_m%d" % (n, k, m) for n in (255, 256, 257)]
    for tag in ("_k31", "_k63"):
        out += [s + tag for s in ["oneword_counting", "oneword_network", "oneword_large", "repeat_2", "repeat_200", "repeat_300", "straddle", "sizes_small", "sizes_cap",
                                  "sizes_cap_plus_1", "sizes_cap_plus_1_few_distinct"] + ["big_d%d" % d for d in (2047, 2048, 2049, 4096, 4097, 6144, 10240, 16385)]
                + ["big_two_pass_counts", "big_occurrences_wrap", "buckets_255", "buckets_256", "buckets_257", "buckets_across_1024", "order_first_two_swapped",
                   "order_last_two_swapped", "order_inversion_at_1024", "order_descending", "launches_two", "launches_one", "batch_large_first", "batch_large_middle",
                   "batch_large_last", "batch_large_adjacent", "batch_large_all", "batch_large_identical", "batch_large_between_empty", "batch_host_first",
                   "batch_host_last", "batch_host_beside_large", "batch_host_largest", "batch_all_host", "batch_short_ends"]]
    return out + ["batch_k32_m15", "batch_tiny_255", "batch_tiny_256", "batch_tiny_257"]


def test_the_names_are_the_table():
    assert _names() == [c[0] for c in decode_cases()]


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names())
def test_decoded_keys_are_the_model(ctx, name):
    """a to e: every batch of the table through spsp_sketch_decode_device with the default settings"""
    check(ctx, case(name))


@pytest.mark.gpu
def test_one_context_over_many_calls():
    """f: a context of the test's own.  The table grows (small batch, then one whose large sketches need eight times the slots),
    300 decodes of the small batch take the 8-bit epoch through its wrap whatever came before, the big batch comes back and
    finds its slots past the small mask holding words of old epochs, and large, small, large batches reuse every buffer."""
    small, big = case("sizes_cap_plus_1_few_distinct_k63"), case("big_d16385_k31")
    slots = lambda c: 1 << max(10, (2 * sum(len(P.raw_keys(c[1], c[2], b)) for b in BUCKETS[c[0]]) - 1).bit_length())
    assert slots(big) >= 4 * slots(small)
    with sp.Context(0) as own:
        check(own, small, "first")
        check(own, big, "the table grows")
        for i in range(300):
            check(own, small, "call %d" % i)
        check(own, big, "after the wrap")
        check(own, small, "last")
        for name in ("big_d10240_k63", "sizes_small_k63", "big_two_pass_counts_k63", "sizes_small_k31", "big_d4097_k31", "sizes_cap_k31", "big_d2047_k31"):
            check(own, case(name), "large, small, large")


_CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import supersampler_amd as sp
import test_decode_seams as T
with sp.Context(0) as ctx:
    T.check_all(ctx, %r)
print("all decoded")
"""


@pytest.mark.gpu
def test_decoded_keys_are_the_model_under_every_hook():
    """g: the hooks are read once per process, so the whole table runs once more in a child of its own with every sketch through
    the network, with the structure walk on the device whatever the batch size, and with it on the host.  One child after the
    other; the first that fails, ends on a signal or runs out of time ends the test."""
    for var, value in (("SPSP_DEBUG_DECODE_SORT", "network"), ("SPSP_DEBUG_DECODE_WALK", "device"), ("SPSP_DEBUG_DECODE_WALK", "host")):
        what = "%s=%s" % (var, value)
        r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), what)], env=dict(os.environ, **{var: value}),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "all decoded" in r.stdout, (what, r.returncode, r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.gpu
def test_through_the_file_loader(ctx, tmp_path):
    """h: 300 tiny hand-built sketches as files through Context.compare_files -- the pieces go up from the reader's regions
    with no staging copy -- and the CSVs back: every pair's intersection and both cardinalities are set algebra on the model's
    keys, printed by the oracle's formatter.  Every sketch holds one key that all share and two that its neighbour shares, so
    no cell is zero by default, and a containment of 1 / card tells every cardinality below 1000 apart at six digits."""
    k, m, n = 31, 11, 300
    shared = (minimizer(m, 0), [], [kmer_line(k, m, 0, 77)])
    sketches = []
    for i in range(n):
        own = filler(k, m, 3 + i % 11, first=1 + i % 4, salt=100 + i)
        link = [(minimizer(m, 50), [], [kmer_line(k, m, i, 78), kmer_line(k, m, i + 1, 78)])]
        sketches.append([shared] + own + link)
    payloads = [P.payload(k, m, b) for b in sketches]
    keys = [set(P.model(k, m, b)) for b in sketches]
    paths = []
    for i, pl in enumerate(payloads):
        paths.append(str(tmp_path / ("s%03d.gz" % i)))
        sp.write_gz(paths[-1], pl, 1)
    inter = np.zeros((n, n), np.uint32)
    for i in range(n):
        for j in range(i + 1, n):
            inter[i, j] = len(keys[i] & keys[j])
    card = np.array([len(s) for s in keys], np.uint64)
    assert inter[0, 1] == 2 and inter[0, 2] == 1
    ctx.compare_files(paths, str(tmp_path / "out"))
    for jac, suf in ((True, "_jaccard.csv.gz"), (False, "_containment.csv.gz")):
        assert gzip.open(str(tmp_path / "out") + suf, "rb").read() == orc.csv(jac, paths, inter, card, None, 6, 0.0), suf
    got_inter, got_card = ctx.compare(sp.sketches_from_payloads(payloads))
    assert got_card.tolist() == card.tolist() and (np.triu(got_inter, 1) == inter).all()
