"""Sequences whose selected m-mers ("hits": XXH64(canonical m-mer, seed 1312) <= T) lie exactly where a test puts them.

No GPU use: numpy only.  tests/test_scan_seams.py builds its inputs with this module and pins it on the CPU against the
oracle (hash, canonical values, masks).  Codes are the product's: A=0 C=1 T=2 G=3 (`(byte >> 1) & 3`), the first base of
an m-mer most significant, the complement of a code is `code ^ 2`.

    hit_mask(bases, m, T)       the hits of a buffer, at all n - m + 1 positions, records ignored
    pool(m, T)                  hit m-mers as ASCII rows, every canonical value on both strands
    background(n, m, T, seed)   random bases without a single hit
    plant(bases, positions, ..) writes one pool m-mer per position so that the mask changes at that position only
    tandem / distinct_run / near_hit / periodic / bait: runs of hits, of survivors without hits, and ends that the zero
                                padding of a kernel would complete into a hit"""
import functools

import numpy as np

SEED = 1312
LETTERS = np.frombuffer(b"ACTG", dtype=np.uint8)            # code -> letter
U = np.uint64


def xxh64(x):
    """vectorised XXH64 of one 64-bit word each, seed 1312 (the 8-byte input form: no stripes, one round, avalanche)"""
    x = np.asarray(x, dtype=np.uint64)
    P1, P2, P3, P4, P5 = (U(v) for v in (11400714785074694791, 14029467366897019727, 1609587929392839161,
                                         9650029242287828579, 2870177450012600261))

    def rotl(v, b):
        return (v << U(b)) | (v >> U(64 - b))
    with np.errstate(over="ignore"):
        h = U(SEED) + P5 + U(8)
        h = h ^ (rotl(x * P2, 31) * P1)
        h = rotl(h, 27) * P1 + P4
        h = h ^ (h >> U(33)); h = h * P2
        h = h ^ (h >> U(29)); h = h * P3
        h = h ^ (h >> U(32))
    return h


def codes(bases):
    return ((np.asarray(bases, dtype=np.uint8) >> 1) & 3).astype(np.uint64)


def rc_values(v, m):
    """reverse complement of m-mer values"""
    v = np.asarray(v, dtype=np.uint64).copy()
    r = np.zeros_like(v)
    for _ in range(m):
        r = (r << U(2)) | ((v & U(3)) ^ U(2))
        v >>= U(2)
    return r


def forward(bases, m):
    """the m-mer value at every position of an ASCII buffer (n - m + 1 of them)"""
    c = codes(bases)
    n = len(c) - m + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    f = np.zeros(n, np.uint64)
    for j in range(m):
        f = (f << U(2)) | c[j:j + n]
    return f


def canon(bases, m):
    """the canonical m-mer value (the smaller of the two strands) at every position"""
    c = codes(bases)
    n = len(c) - m + 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    f = np.zeros(n, np.uint64)
    r = np.zeros(n, np.uint64)
    for j in range(m):
        f = (f << U(2)) | c[j:j + n]
        r |= (c[j:j + n] ^ U(2)) << U(2 * j)
    return np.minimum(f, r)


def hit_mask(bases, m, T):
    return xxh64(canon(bases, m)) <= U(T)


def to_bases(v, m):
    """m-mer value(s) -> ASCII, shape (..., m)"""
    v = np.asarray(v, dtype=np.uint64)
    sh = (2 * (m - 1 - np.arange(m))).astype(np.uint64)
    return LETTERS[((v[..., None] >> sh) & U(3)).astype(np.intp)]


def text(b):
    return bytes(np.asarray(b, dtype=np.uint8))


# ------------------------------------------------------------------------------------------------------- hit pools

@functools.lru_cache(maxsize=None)
def pool_values(m, T):
    """canonical m-mer values with hash <= T, ascending.  m <= 13: all of them (the whole universe is hashed, in chunks);
    m = 15: those a seeded random sequence of 4 Mbp holds"""
    T = int(T)
    if m <= 13:
        out = []
        step = 1 << 22
        for lo in range(0, 1 << (2 * m), step):
            v = np.arange(lo, min(lo + step, 1 << (2 * m)), dtype=np.uint64)
            v = v[xxh64(v) <= U(T)]
            out.append(v[rc_values(v, m) >= v])
        return np.concatenate(out)
    rng = np.random.default_rng(1500 + m)
    c = canon(LETTERS[rng.integers(0, 4, 4_000_000)], m)
    return np.unique(c[xxh64(c) <= U(T)])


@functools.lru_cache(maxsize=None)
def pool(m, T):
    """the hit m-mers as ASCII rows, shape (P, m): every canonical value, then its other strand (palindromes once)"""
    v = pool_values(m, int(T))
    r = rc_values(v, m)
    both = np.stack([v, r], axis=1).reshape(-1)
    keep = np.ones(len(both), bool)
    keep[1::2] = r != v
    out = to_bases(both[keep], m)
    out.setflags(write=False)
    return out


def pool_complete(m):
    """pool(m, T) holds every hit m-mer there is (so a table built from it is the kernel's table)"""
    return m <= 13


# ------------------------------------------------------------------------------------------------------ background

def background(n, m, T, seed, also=None):
    """n seeded random bases without a hit.  The middle base of every hit m-mer is changed and the mask taken again, until
    it is empty.  also(bases) -> one bool per base: further positions to clear (a survivor model; behind the last m-mer it
    reads the padding, and the nearest base of the buffer is changed)"""
    rng = np.random.default_rng(seed)
    b = LETTERS[rng.integers(0, 4, n)].copy()
    for _ in range(50):
        mask = np.zeros(n, bool)
        mask[:max(n - m + 1, 0)] = hit_mask(b, m, T)
        if also is not None:
            extra = also(b)
            assert len(extra) == n, "also() gives one value per base"
            mask |= extra
        pos = np.nonzero(mask)[0]
        if pos.size == 0:
            return b
        q = np.minimum(pos + m // 2, n - 1)
        b[q] = LETTERS[(((b[q] >> 1) & 3) + rng.integers(1, 4, len(q))) & 3]
    raise AssertionError("background: hits left after 50 rounds")


# -------------------------------------------------------------------------------------------------------- planting

def plant(bases, positions, m, T, first=0, choose=None, min_gap=None):
    """writes a pool m-mer at each position, in place; -> the pool rows used.  A write stands only if the mask over every
    position it touches changes at that position alone; otherwise the next pool row is tried.  choose(row) -> bool
    restricts the rows.  A position no row can take is an AssertionError: the test fails.  Positions lie at least 2m apart;
    min_gap >= m lowers that for a seam that needs two hits in neighbouring lanes (the writes still do not overlap, and the
    mask is still taken over every position a write touches, the earlier hit among them)"""
    P = pool(m, int(T))
    n = len(bases)
    pos = sorted(int(p) for p in positions)
    gap = 2 * m if min_gap is None else min_gap
    assert gap >= m and all(b - a >= gap for a, b in zip(pos, pos[1:])), "seams planted in one buffer lie at least 2m apart"
    used = []
    for i, p in enumerate(pos):
        assert 0 <= p and p + m <= n, (p, n)
        lo, hi = max(0, p - m + 1), min(n, p + 2 * m - 1)
        before = hit_mask(bases[lo:hi], m, T)
        assert not before[p - lo], "position %d is a hit already" % p
        want = before.copy()
        want[p - lo] = True
        old = bases[p:p + m].copy()
        for t in range(len(P)):
            row = P[(first + 7 * i + t) % len(P)]
            if choose is not None and not choose(row):
                continue
            bases[p:p + m] = row
            if np.array_equal(hit_mask(bases[lo:hi], m, T), want):
                used.append(row)
                break
        else:
            bases[p:p + m] = old
            raise AssertionError("no pool m-mer of (m=%d, T=%d) can be planted at %d" % (m, T, p))
    return used


def planted(n, positions, m, T, seed, first=0, choose=None):
    """background + plant -> bases whose hits are exactly `positions`"""
    b = background(n, m, T, seed)
    plant(b, positions, m, T, first=first, choose=choose)
    return b


# ------------------------------------------------------------------------------------------------------------ runs

def tandem_row(m, T, skip=0):
    """a pool m-mer whose tandem repeat (period m) has its hits at the multiples of m and nowhere else"""
    P = pool(m, int(T))
    for i in range(len(P)):
        row = P[(i + skip) % len(P)]
        t = np.tile(row, 6)
        mask = hit_mask(t, m, T)
        want = np.zeros(len(mask), bool)
        want[::m] = True
        if np.array_equal(mask, want):
            return row
    raise AssertionError("no pool m-mer of (m=%d, T=%d) makes a clean tandem run" % (m, T))


def tandem(row, n_hits):
    """n_hits copies back to back: n_hits hits, all of one minimizer (when the row came from tandem_row)"""
    return np.tile(np.asarray(row, dtype=np.uint8), n_hits)


def distinct_run(m, T, n_hits, first=0):
    """n_hits pool m-mers back to back, neighbours of different canonical value: a hit every m positions, and whatever
    else their junctions make (the caller takes the mask)"""
    P = pool(m, int(T))
    return np.concatenate([P[(first + 2 * i) % len(P)] for i in range(n_hits)])     # stride 2: never both strands in a row


def near_hit(m, T, skip=0):
    """the first m - 1 bases of a pool m-mer and a last base that makes the canonical hash > T: every copy passes a test
    of the first 9 or 10 bases, none is a hit, and neither is any m-mer of its tandem run"""
    P = pool(m, int(T))
    for i in range(len(P)):
        row = P[(i + skip) % len(P)]
        for c in LETTERS:
            if c == row[-1]:
                continue
            x = row.copy()
            x[-1] = c
            if hit_mask(x, m, T)[0]:
                continue
            if not hit_mask(np.tile(x, 6), m, T).any():
                return x
    raise AssertionError("no near-hit for (m=%d, T=%d)" % (m, T))


def periodic(m, T, period, accept):
    """a sequence u of `period` bases such that accept(u repeated to 4 m bases) holds, or None.  All 4**period are tried
    in order"""
    for v in range(1 << (2 * period)):
        u = to_bases(np.uint64(v), period)
        if accept(np.tile(u, (4 * m + period - 1) // period)[:4 * m]):
            return u
    return None


def periodic_hits(m, T, period):
    """every sequence u of `period` bases (as a value) whose repetition starts with a hit m-mer; all 4**period are hashed, so
    every rotation is among them"""
    u = np.arange(1 << (2 * period), dtype=np.uint64)
    f = np.zeros_like(u)
    for j in range(m):
        f = (f << U(2)) | ((u >> U(2 * (period - 1 - j % period))) & U(3))
    return u[xxh64(np.minimum(f, rc_values(f, m))) <= U(T)]


def bait(m, T):
    """-> (j, head): head = the first m - j bases of a pool m-mer whose last j bases are A, j >= 1 as large as the pool
    has it.  A buffer that ends with `head` has no m-mer there; j zero bases behind it would make one, and a hit"""
    P = pool(m, int(T))
    best = None
    for row in P:
        j = 0
        while j < m and row[m - 1 - j] == LETTERS[0]:
            j += 1
        if j >= 1 and j < m and (best is None or j > best[0]):
            best = (j, row[:m - j].copy())
    assert best is not None, "no pool m-mer of (m=%d, T=%d) ends with A" % (m, T)
    return best


def with_tail(bases, tail):
    """bases whose last len(tail) bases are `tail`"""
    b = np.asarray(bases, dtype=np.uint8).copy()
    b[len(b) - len(tail):] = tail
    return b


# -------------------------------------------------------------------------------------------------- survivor models

def _prefix_set(m, T, first, count):
    """values of bases [first, first + count) of every pool m-mer, both strands (pool() holds both)"""
    assert pool_complete(m)
    P = pool(m, int(T))
    return np.unique(forward(P[:, first:first + count].reshape(-1), count)[::count]) if len(P) else np.zeros(0, np.uint64)


def _padded(bases, extra=32):
    return np.concatenate([np.asarray(bases, dtype=np.uint8), np.full(extra, LETTERS[0], np.uint8)])


def survivors_pair_mid(bases, m, T):
    """positions the pair table of m >= 10 lets through (k_build_key8 / k_build_pairtab): an even position p if the first 9
    bases of its m-mer start a hit m-mer on either strand, an odd one if they are bases 1..9 of one -- p's m-mer read from
    p + 1.  Bases behind the buffer read as A, as the kernels' zero padding does.  One value per base of the buffer"""
    n = len(bases)
    b = _padded(bases)
    k9 = _prefix_set(m, T, 0, 9)
    m9 = _prefix_set(m, T, 1, 9)
    at = forward(b, 9)
    even = np.isin(at[:n], k9)
    odd = np.isin(at[1:n + 1], m9)
    return np.where(np.arange(n) % 2 == 0, even, odd)


def survivors_single(bases, m, T):
    """positions the 10-base prefix table lets through (k_build_key10)"""
    n = len(bases)
    return np.isin(forward(_padded(bases), 10)[:n], _prefix_set(m, T, 0, 10))
