"""Prevalence: how many of the sketches hold each key (include/spsp.h: spsp_prevalence_device, spsp_prevalence_csv_host,
spsp_spectrum_csv_host, spsp_prevalence_files; bin/comparator -P).

The rule, on sets of the comparator's keys (orc.sketch_keys: the distinct (minimizer, canonical k-mer) pairs of a sketch).
n_query == 0: every sketch is a row and a reference, R = n.  n_query > 0: the first n_query sketches are rows only, the
R = n - n_query behind them the references.  h(x) = the references that hold key x.  Classes, in this order, at num / den:

    absent  h == 0
    core    h * den >= num * R
    unique  h == 1
    shell   everything else

Per row sketch the keys per class and holders = the sum of h; spectrum[t] = the distinct keys of the references' union with
h == t.  Every expected value below comes from collections.Counter over key tuples and Python integers (model): integers and
bytes, no tolerance anywhere.

Where the kernels cut, and the shapes that sit on the cuts: every kernel is workgroups of 256 lanes in waves of 64 over
consecutive entries (sketches of 63 .. 65 and 255 .. 257 keys, offsets that fall inside a wave); the spectrum bins holder counts
in windows of 8 192 (R = 8 191, 8 192, 8 193 and 65 535 with a key that everybody holds and one that all but one hold); the table
has a power of two of slots (SPSP_DEBUG_PREVALENCE_TABLE=min: exactly as many slots as reference entries, all taken)."""
import gzip
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import supersampler_amd as sp
from oracle import oracle_py as orc
from supersampler_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
KM = ((31, 11), (21, 9), (63, 15))
S = 100.0
HEADER = "sketch,keys,core,shell,unique,absent,f_core,mean_holders\n"
SPECTRUM_HEADER = "holders,keys,cumulative\n"
THRESHOLDS = ((1, 1), (95, 100), (1, 2), (1, 1_000_000), (1, 10))      # (the last one: a family of six is core among 60)
GOLD = 0x9E3779B97F4A7C15
U64 = (1 << 64) - 1


# -------------------------------------------------------------------------------------------------- the model

def key_class(h, R, num, den):
    if h == 0:
        return "absent"
    if h * den >= num * R:
        return "core"
    return "unique" if h == 1 else "shell"


def model(sets, n_query, num, den):
    """sets: one collection of key tuples per sketch -> (rows [(core, shell, unique, absent, holders)], spectrum [R + 1])"""
    refs = sets[n_query:]
    R = len(refs)
    h = Counter(x for s in refs for x in set(s))
    rows = []
    for s in (sets[:n_query] if n_query else sets):
        c = Counter(key_class(h[x], R, num, den) for x in set(s))
        rows.append((c["core"], c["shell"], c["unique"], c["absent"], sum(h[x] for x in set(s))))
    spectrum = [0] * (R + 1)
    for v in h.values():
        spectrum[v] += 1
    return rows, spectrum


def as_rows(tuples):
    rows = np.zeros(len(tuples), dtype=sp.PREVALENCE_ROW_DTYPE)
    for i, t in enumerate(tuples):
        rows[i] = t
    return rows


def as_tuples(rows):
    return [tuple(int(r[f]) for f in ("core", "shell", "unique", "absent", "holders")) for r in rows]


def py_csv(tuples, names, card, precision=6):
    text = HEADER
    for (core, shell, uniq, absent, held), name, c in zip(tuples, names, card):
        f_core = "%.*g" % (precision, core / c) if c else "0"
        mean = "%.*g" % (precision, held / c) if c else "0"
        text += "%s,%d,%d,%d,%d,%d,%s,%s\n" % (name, c, core, shell, uniq, absent, f_core, mean)
    return text.encode()


def py_spectrum_csv(spectrum):
    text = SPECTRUM_HEADER
    for t in range(1, len(spectrum)):
        if spectrum[t]:
            text += "%d,%d,%d\n" % (t, spectrum[t], sum(spectrum[t:]))
    return text.encode()


# ------------------------------------------------------------------------------------------------ not GPU

def K(*xs):
    return {(x, 0, x) for x in xs}


def test_model_on_hand_made_cases():
    # R = 20: key 1 in all, key 2 in 19, key 3 in 18, key 100 + j in sketch j alone
    sets = [K(1, 100 + j) | (K(2) if j < 19 else set()) | (K(3) if j < 18 else set()) for j in range(20)]
    for num, den in ((19, 20), (95, 100)):
        rows, spectrum = model(sets, 0, num, den)
        assert key_class(19, 20, num, den) == "core" and key_class(18, 20, num, den) == "shell"
        assert rows[0] == (2, 1, 1, 0, 20 + 19 + 18 + 1) and rows[18] == (2, 0, 1, 0, 20 + 19 + 1) and rows[19] == (1, 0, 1, 0, 21)
        assert spectrum == [0, 20] + [0] * 16 + [1, 1, 1]
    assert model(sets, 0, 1, 1)[0][0] == (1, 2, 1, 0, 58)
    assert model(sets, 0, 1, 1_000_000)[0][0] == (4, 0, 0, 0, 58)                    # everything present is core
    assert model(sets, 0, 1, 20)[0][0] == (4, 0, 0, 0, 58)                           # 1 * 20 >= 1 * 20: unique AND core is core
    assert model(sets, 0, 1, 19)[0][0] == (3, 0, 1, 0, 58)
    # R = 1: everything is core, at every threshold
    for num, den in THRESHOLDS:
        assert model([K(1, 2, 3)], 0, num, den) == ([(3, 0, 0, 0, 3)], [0, 3])
    # a query with absent keys; the queries take no part in the spectrum, and h counts references only
    q = [K(1, 2, 50, 51), K(50), set()]
    rows, spectrum = model(q + sets, 3, 95, 100)
    assert rows == [(2, 0, 0, 2, 39), (0, 0, 0, 1, 0), (0, 0, 0, 0, 0)] and spectrum == model(sets, 0, 95, 100)[1]
    assert model([K(1), K(1)], 1, 1, 1) == ([(1, 0, 0, 0, 1)], [0, 1])
    # the identities
    rows, spectrum = model(sets, 0, 1, 2)
    assert sum(spectrum) == len(set().union(*sets)) and sum(t * v for t, v in enumerate(spectrum)) == sum(len(s) for s in sets)
    assert all(sum(r[:4]) == len(s) for r, s in zip(rows, sets))


def test_prevalence_csv_equals_the_python_writer():
    names = ["a one.fa.gz", "dir/b.two", "c", "d.1.2.sketch"]
    rows = [(700, 200, 100, 0, 123456), (0, 0, 0, 0, 0), (1, 1, 1, 4, 9), (333, 0, 0, 0, 333 * 7)]
    card = [1000, 0, 7, 333]
    for precision in (6, 3):
        assert sp.prevalence_csv(as_rows(rows), names, card, precision) == py_csv(rows, names, card, precision)
        assert sp.prevalence_csv(as_rows([]), [], [], precision) == HEADER.encode()
    text = sp.prevalence_csv(as_rows(rows), names, card).decode().splitlines()
    assert text[1] == "a one.fa.gz,1000,700,200,100,0,0.7,123.456" and text[2] == "dir/b.two,0,0,0,0,0,0,0"
    assert text[3] == "c,7,1,1,1,4,0.142857,1.28571"
    assert sp.prevalence_csv(as_rows(rows), names, card, 3).decode().splitlines()[3] == "c,7,1,1,1,4,0.143,1.29"
    with pytest.raises(sp.SpspError) as e:                                             # classes that do not add up to the key count
        sp.prevalence_csv(as_rows([(1, 1, 1, 1, 4)]), ["x"], [5])
    assert e.value.code == sp.ERR_ARG


def test_spectrum_csv_equals_the_python_writer():
    gaps = [0, 5, 0, 0, 2, 0, 0, 0, 0, 0, 1, 0]
    assert sp.spectrum_csv(gaps) == py_spectrum_csv(gaps) == b"holders,keys,cumulative\n1,5,8\n4,2,3\n10,1,1\n"
    assert sp.spectrum_csv([0]) == sp.spectrum_csv([0, 0, 0]) == SPECTRUM_HEADER.encode()
    assert sp.spectrum_csv([77, 1]) == b"holders,keys,cumulative\n1,1,1\n"           # ([0] is nobody's)
    big = [0, 1 << 40, 0, (1 << 63) - (1 << 40)]                                       # a cumulative beyond 2^32, and one just below 2^63
    assert sp.spectrum_csv(big) == py_spectrum_csv(big)


def test_abi_has_the_prevalence_calls():
    calls = ("spsp_prevalence_device", "spsp_prevalence_csv_host", "spsp_spectrum_csv_host", "spsp_prevalence_files")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    assert sp.PREVALENCE_ROW_DTYPE.itemsize == 40 and sp.PREVALENCE_ROW_DTYPE.names == ("core", "shell", "unique", "absent", "holders")
    for name in calls:
        assert hasattr(sp.lib(), name)


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-P", t) for t in ("0", "1.5", "0.1234567", "0.0", "abc", "", "0.", ".5", "-0.5", "2")]
    cases += [("-P", "0.95", "-g", "3", "-q", "list.txt"), ("-P", "0.95", "-c", "0.5"), ("-P", "0.95", "-C", "0.5"), ("-P", "0.95", "-N", "5")]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and "-P" in r.stdout, (args, r.stdout, r.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


# ------------------------------------------------------------------------------------------ hand-built keys

def mixed(i):
    """positions -> 64-bit words that are neither the position nor near their neighbours' words (the product wraps)"""
    return [((int(x) + 1) * GOLD) & U64 for x in i]


def pack(sketches, k):
    """sketches: one collection of (minimizer, kmer_hi, kmer_lo) per sketch -> (mn, lo, hi or None, off, sets): every sketch
    sorted as the decoder leaves it, back to back"""
    order = [sorted(set(s)) for s in sketches]
    flat = [x for s in order for x in s]
    assert k > 32 or not any(x[1] for x in flat)
    mn = np.array([x[0] for x in flat], dtype=np.uint32)
    hi = np.array([x[1] for x in flat], dtype=np.uint64)
    lo = np.array([x[2] for x in flat], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum([len(s) for s in order])]).astype(np.uint64)
    return mn, lo, (hi if k > 32 else None), off, order


def pool(count, k, salt=0):
    """`count` distinct keys: a few minimizers, kmer_lo a mixed word of the position, kmer_hi (k > 32) its complement"""
    lo = mixed(range(salt, salt + count))
    return [(7 + (i * 5 + salt) % 11, (lo[i] ^ U64) if k > 32 else 0, lo[i]) for i in range(count)]


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


def device_call(ctx, k, mn, lo, hi, off, num, den, n_query=0):
    """-> (rows as tuples, spectrum as list, h per entry as list)"""
    d = upload(mn, lo, hi)
    n = len(off) - 1
    rows, spectrum, d_held = ctx.prevalence_device(k, ptr(d[0]), ptr(d[1]), ptr(d[2]), off, n, num, den, n_query, want_holders=True)
    assert d_held
    held = ctx.to_host(d_held, int(off[-1]), np.uint32).tolist() if int(off[-1]) else []
    del d
    return as_tuples(rows), spectrum.tolist(), held


def check(ctx, sketches, k, n_query=0, thresholds=THRESHOLDS):
    mn, lo, hi, off, order = pack(sketches, k)
    h = Counter(x for s in order[n_query:] for x in s)
    want_held = [h[x] for s in order for x in s]
    for num, den in thresholds:
        rows, spectrum, held = device_call(ctx, k, mn, lo, hi, off, num, den, n_query)
        want_rows, want_spectrum = model(order, n_query, num, den)
        assert held == want_held, (num, den, [i for i, (a, b) in enumerate(zip(held, want_held)) if a != b][:8])
        assert rows == want_rows, (num, den, [(i, a, b) for i, (a, b) in enumerate(zip(rows, want_rows)) if a != b][:4])
        assert spectrum == want_spectrum, (num, den)
    return want_rows, want_spectrum


def seam_sketches(k):
    """keys that differ only in the minimizer, only in kmer_lo, only in kmer_hi (k = 63), beside keys equal in all three"""
    hi = 0x0123456789ABCDEF if k > 32 else 0
    A, B, C = (5, hi, 9), (6, hi, 9), (5, hi, 10)
    D = [(5, hi + 1, 9), (5, hi ^ (1 << 63), 9)] if k > 32 else []
    return [[A, B, C] + D, [A], [B, A], [C], D[:1] + [A], [B, C] + D[1:], [A, C]]


def nested_lengths(k, lengths, salt=0):
    """sketch j = the first lengths[j] keys of one pool: h of pool key i = the sketches longer than i"""
    p = pool(max(lengths), k, salt)
    return [p[:c] for c in lengths]


def star(n, k):
    """n sketches: a key everybody holds, a key all but sketch 0 hold, a key of one's own (sketch 0: two of them)"""
    hi = 0x7FFFFFFFFFFFFFFF if k > 32 else 0
    own = mixed(range(n + 1))
    return [[(3, hi, 1)] + ([(3, hi, 2)] if j else [(9, hi, own[n])]) + [(4 + j % 3, hi, own[j])] for j in range(n)]


def test_the_hand_built_shapes_are_what_they_are_called():
    s = seam_sketches(63)
    assert len({x[0] for x in s[0]}) == 2 and len({x[1] for x in s[0]}) == 3 and len({x[2] for x in s[0]}) == 2
    assert model(s, 0, 1, 1)[1] == [0, 0, 2, 1, 1, 1, 0, 0]
    assert model(seam_sketches(31), 0, 1, 1)[1] == [0, 0, 0, 1, 1, 1, 0, 0]
    rows, spectrum = model(star(8193, 31), 0, 999_999, 1_000_000)
    assert spectrum[8193] == 1 and spectrum[8192] == 1 and spectrum[1] == 8194 and rows[0] == (1, 0, 2, 0, 8195) and rows[1] == (1, 1, 1, 0, 16386)
    assert 999_999 * 65_535 > 1 << 32 and 65_534 * 1_000_000 < 999_999 * 65_535 <= 65_535 * 1_000_000


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_keys_that_differ_in_one_word_only(ctx, k):
    check(ctx, seam_sketches(k), k)
    check(ctx, seam_sketches(k)[:3] + seam_sketches(k), k, n_query=3)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_empty_sketches_and_single_sketches(ctx, k):
    body = nested_lengths(k, [5, 3])
    check(ctx, [[], []] + body[:1] + [[]] + body[1:] + [[], []], k)                   # empty first, in the middle and last
    check(ctx, [[], [], []], k)                                                       # all empty
    check(ctx, [[]], k)
    rows, spectrum = check(ctx, [pool(300, k)], k)                                    # n = 1: everything is core
    assert rows == [(300, 0, 0, 0, 300)] and spectrum == [0, 300]
    check(ctx, [[], pool(5, k)] + [[], []], k, n_query=2)                             # queries against references without keys
    check(ctx, [[], pool(5, k)[:2]] + [[], pool(5, k)], k, n_query=2)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_sketch_lengths_on_wave_and_workgroup_boundaries(ctx, k):
    lengths = [63, 64, 65, 255, 256, 257, 0, 1, 511, 512, 513]
    check(ctx, nested_lengths(k, lengths), k)
    check(ctx, nested_lengths(k, lengths[::-1]), k)
    # queries of those lengths, half of whose keys nobody holds, against the same references
    p, q = pool(600, k), pool(600, k, salt=100_000)
    queries = [p[:c // 2] + q[:c - c // 2] for c in lengths]
    check(ctx, queries + nested_lengths(k, lengths), k, n_query=len(queries))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8191, 8192, 8193, 65535])
def test_a_key_that_everybody_holds(ctx, n):
    """h at its maximum in the last bin of a spectrum window, in the first bin of the next and one further, and at the largest
    n there is: 65 535 adds on one counter, 65 534 on its neighbour in the spectrum; num * R beyond 2^32"""
    k = 31 if n != 8192 else 63
    rows, spectrum = check(ctx, star(n, k), k, thresholds=((999_999, 1_000_000), (1, 2)))
    assert spectrum[n] == 1 and spectrum[n - 1] == 1 and spectrum[1] == n + 1 and sum(spectrum) == n + 3
    assert rows[1] == (2, 0, 1, 0, 2 * n)
    if n == 65535:
        assert model(star(n, k), 0, 999_999, 1_000_000)[0][1] == (1, 1, 1, 0, 2 * n)   # 65 534 holders are not 0.999999 of 65 535


@pytest.mark.gpu
def test_threshold_equality_on_the_device(ctx):
    sets = [[(1, 0, 1), (2, 0, 100 + j)] + ([(1, 0, 2)] if j < 19 else []) + ([(1, 0, 3)] if j < 18 else []) for j in range(20)]
    for num, den in ((19, 20), (95, 100)):
        rows, _ = check(ctx, sets, 31, thresholds=((num, den),))
        assert rows[0] == (2, 1, 1, 0, 58) and rows[19] == (1, 0, 1, 0, 21)
    rows, _ = check(ctx, sets, 31, thresholds=((1, 20), (1, 19), (18, 20), (9, 10), (901, 1000)))
    assert rows[0] == (2, 1, 1, 0, 58)                                                # (901 / 1000 of 20 is 18.02: 19 holders pass, 18 do not)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_smallest_table(ctx, k, monkeypatch):
    """as many slots as reference entries and every one of them taken: probe sequences wrap, chains are as long as they get, and
    a query key nobody holds goes round the whole table"""
    refs = [pool(512, k, salt=1000 * j) for j in range(8)]                            # 4 096 entries, 4 096 distinct keys
    assert len(set().union(*map(set, refs))) == 4096
    queries = [pool(40, k, salt=500_000), refs[3][:100] + pool(30, k, salt=600_000)]
    shapes = [(refs, 0), (queries + refs, 2), (nested_lengths(k, [300, 257, 256, 64, 1, 0, 211]), 0), (star(1000, k), 0)]
    plain = [check(ctx, s, k, nq, thresholds=((1, 2),)) for s, nq in shapes]
    monkeypatch.setenv("SPSP_DEBUG_PREVALENCE_TABLE", "min")
    assert [check(ctx, s, k, nq, thresholds=((1, 2),)) for s, nq in shapes] == plain


# ------------------------------------------------------------------------------------------ the collections

_cache = {}


def cached(f):
    def g(*a):
        if (f.__name__, a) not in _cache:
            _cache[(f.__name__, a)] = f(*a)
        return _cache[(f.__name__, a)]
    return g


def _references():
    """48 genomes in 8 families (blocks of six: members 0 and 3 are both the unmutated ancestor) + 12 unrelated ones"""
    refs = synth.family_genomes(5, 48, 60_000, 8, [0.0, 0.01, 0.03])
    rng = np.random.default_rng(6)
    return refs + [synth.random_genome(rng, 60_000) for _ in range(12)]


def _sketch(g, name, k, m, s=S):
    return orc.sketch_fasta(synth.to_fasta(g, name), k, m, s)[0]


@cached
def collection(k, m):
    """60 payloads of about 600 keys each, sketched by the oracle at -s 100"""
    return [_sketch(g, "g%d" % i, k, m) for i, g in enumerate(_references())]


@cached
def three_queries(k, m):
    """queries: a mixture of references and something new, a genome that shares nothing with any reference, a sequence shorter
    than k (a sketch without buckets); references: the 60 with one more sketch without buckets in the middle"""
    refs = _references()
    rng = np.random.default_rng(8)
    mix = np.concatenate([refs[1], refs[13], refs[50], synth.random_genome(np.random.default_rng(7), 60_000), refs[40][:1500]])
    empty = _sketch(synth.random_genome(rng, k - 2), "short", k, m)
    assert empty.count(b"\n") == 1
    pl = collection(k, m)
    return [_sketch(mix, "mix", k, m), _sketch(synth.random_genome(rng, 60_000), "alien", k, m), empty] + pl[:30] + [empty] + pl[30:]


def key_set(payload):
    _, _, mn, lo, hi = orc.sketch_keys(payload)
    return set(zip(mn.tolist(), hi.tolist(), lo.tolist()))


def decoded(ctx, payloads):
    """-> (k, d_mn, d_lo, d_hi, off, the key tuples of every entry in the device's order)"""
    k, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
    total = int(off[-1])
    mn, lo = ctx.to_host(d_mn, total, np.uint32), ctx.to_host(d_lo, total, np.uint64)
    hi = ctx.to_host(d_hi, total, np.uint64) if k > 32 else np.zeros(total, np.uint64)
    return k, d_mn, d_lo, d_hi, off, list(zip(mn.tolist(), hi.tolist(), lo.tolist()))


def write_files(root, payloads, tag="f"):
    paths = []
    for i, p in enumerate(payloads):
        paths.append(os.path.join(str(root), "%s %03d.sk.gz" % (tag, i)))             # (names with a space and dots)
        sp.write_gz(paths[-1], p, 1)
    return paths


def gunzip(path):
    return gzip.open(path, "rb").read()


def test_the_collections_are_what_they_are_called():
    sets = [key_set(p) for p in collection(31, 11)]
    assert len(sets) == 60 and all(400 < len(s) < 1500 for s in sets)
    rows, spectrum = model(sets, 0, 1, 10)
    assert spectrum[1] > 0 and spectrum[6] > 0 and sum(spectrum[7:]) == 0             # keys of one sketch, keys of a whole family, nothing wider
    assert any(r[2] for r in rows) and any(r[1] for r in rows) and any(r[0] for r in rows)   # unique, shell and core keys
    q = [key_set(p) for p in three_queries(31, 11)]
    rows, _ = model(q, 3, 1, 2)
    assert rows[1] == (0, 0, 0, len(q[1]), 0) and len(q[1]) > 100 and rows[2] == (0, 0, 0, 0, 0) and not q[3 + 30]
    assert rows[0][3] > 100 and rows[0][4] > 0 and sum(rows[0][:3]) > 100


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", KM)
def test_against_the_comparison_and_the_model(ctx, k, m):
    import torch
    pl = collection(k, m)
    n = len(pl)
    sets = [key_set(p) for p in pl]
    kk, d_mn, d_lo, d_hi, off, entries = decoded(ctx, pl)
    assert kk == k and [len(s) for s in sets] == np.diff(off).tolist()
    h = Counter(x for s in sets for x in s)
    first = None
    for num, den in THRESHOLDS:
        rows, spectrum, d_held = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, num, den, want_holders=True)
        want_rows, want_spectrum = model(sets, 0, num, den)
        assert as_tuples(rows) == want_rows and spectrum.tolist() == want_spectrum, (num, den)
        assert ctx.to_host(d_held, len(entries), np.uint32).tolist() == [h[x] for x in entries]
        assert sum(t * v for t, v in enumerate(spectrum.tolist())) == int(off[-1]) and sum(spectrum.tolist()) == len(h)
        first = rows if first is None else first
        assert np.array_equal(rows["holders"], first["holders"])
    # two independent kernels: the row sums of the comparison's matrix on the same arrays
    inter = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    ctx.compare_device(k, d_mn, d_lo, d_hi, off, n, 0, 1, inter.data_ptr())
    torch.cuda.synchronize()
    x = inter.cpu().numpy().astype(np.int64)
    x = np.triu(x, 1)
    x = x + x.T
    card = np.diff(off).astype(np.int64)
    assert np.array_equal(first["holders"].astype(np.int64) - card, x.sum(axis=1))
    # ... and in query mode: the first seven as queries against the rest
    rows, spectrum = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, 1, 2, n_query=7)
    assert np.array_equal(rows["holders"].astype(np.int64), x[:7, 7:].sum(axis=1))
    assert (as_tuples(rows), spectrum.tolist()) == model(sets, 7, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_three_queries_against_the_references(ctx, k, m):
    pl = three_queries(k, m)
    sets = [key_set(p) for p in pl]
    kk, d_mn, d_lo, d_hi, off, entries = decoded(ctx, pl)
    h = Counter(x for s in sets[3:] for x in s)
    for num, den in THRESHOLDS:
        rows, spectrum, d_held = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, len(pl), num, den, n_query=3, want_holders=True)
        assert (as_tuples(rows), spectrum.tolist()) == model(sets, 3, num, den), (num, den)
        assert ctx.to_host(d_held, len(entries), np.uint32).tolist() == [h[x] for x in entries]
    assert as_tuples(rows)[1] == (0, 0, 0, len(sets[1]), 0) and as_tuples(rows)[2] == (0, 0, 0, 0, 0)


@pytest.mark.gpu
def test_buffers_are_reused_and_leave_other_calls_alone(ctx):
    import torch
    small, large = nested_lengths(31, [5, 3, 0, 4]), star(3000, 31)
    fresh = sp.Context(0)
    try:
        want = [check(fresh, s, 31, thresholds=((1, 2),)) for s in (small, large)]
    finally:
        fresh.close()
    assert [check(ctx, s, 31, thresholds=((1, 2),)) for s in (small, large, small, large)] == want + want
    # directly after a comparison, and directly after a gather, on the same context
    pl = three_queries(31, 11)
    sets = [key_set(p) for p in pl]
    k, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(pl)
    n = len(pl)
    inter = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    ctx.compare_device(k, d_mn, d_lo, d_hi, off, n, 0, 1, inter.data_ptr())
    rows, spectrum = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, 95, 100, n_query=3)
    assert (as_tuples(rows), spectrum.tolist()) == model(sets, 3, 95, 100)
    assert len(ctx.gather_device(k, d_mn, d_lo, d_hi, off, n, 3, 25)) >= 3
    rows, spectrum = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, 95, 100, n_query=3)
    assert (as_tuples(rows), spectrum.tolist()) == model(sets, 3, 95, 100)
    rows, spectrum = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, 95, 100)
    assert (as_tuples(rows), spectrum.tolist()) == model(sets, 0, 95, 100)
    # the arrays are only read
    total = int(off[-1])
    before = (ctx.to_host(d_mn, total, np.uint32), ctx.to_host(d_lo, total, np.uint64))
    ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, 1, 2)
    assert np.array_equal(before[0], ctx.to_host(d_mn, total, np.uint32)) and np.array_equal(before[1], ctx.to_host(d_lo, total, np.uint64))


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(ctx):
    sketches = nested_lengths(31, [70, 3, 0, 130])
    mn, lo, hi, off, order = pack(sketches, 31)
    want = model(order, 0, 1, 2)
    d = upload(mn, lo, hi)
    n = len(off) - 1
    L = sp.lib()
    rows = np.zeros(n, dtype=sp.PREVALENCE_ROW_DTYPE)
    spectrum = np.zeros(n + 1, dtype=np.uint64)
    call = lambda n=n, nq=0, num=1, den=2, off=off, d=d: L.spsp_prevalence_device(ctx._h, 31, ptr(d[0]), ptr(d[1]), None, off.ctypes.data, n, nq, num, den,
                                                                                  rows.ctypes.data, spectrum.ctypes.data, None)
    assert call() == 0 and (as_tuples(rows), spectrum.tolist()) == want
    for kw in (dict(n=0), dict(nq=n), dict(nq=n + 1), dict(num=0), dict(num=3, den=2), dict(num=1, den=1_000_001), dict(num=1_000_001, den=1_000_001)):
        assert call(**kw) == sp.ERR_ARG, kw
    big_off = np.zeros(65536 + 1, dtype=np.uint64)
    assert call(n=65536, off=big_off) == sp.ERR_ARG
    ctx.compare_keys_unordered(True)
    try:
        assert call() == sp.ERR_ARG and "unordered" in sp.lib().spsp_last_error().decode()
    finally:
        ctx.compare_keys_unordered(False)
    # unsorted keys: two neighbours swapped inside the last sketch (a reference), inside the first (a query), and a key twice
    for nq, at in ((0, int(off[3]) + 64), (1, 10), (0, int(off[3]) + 1)):
        bad_mn, bad_lo = mn.copy(), lo.copy()
        if at == int(off[3]) + 1:
            bad_mn[at], bad_lo[at] = bad_mn[at - 1], bad_lo[at - 1]
        else:
            bad_mn[[at, at + 1]], bad_lo[[at, at + 1]] = bad_mn[[at + 1, at]], bad_lo[[at + 1, at]]
        bad = upload(bad_mn, bad_lo)
        rows[:] = (1, 1, 1, 1, 1)
        assert call(nq=nq, d=bad) == sp.ERR_ARG and "increasing" in sp.lib().spsp_last_error().decode(), (nq, at)
        assert not any(any(r) for r in as_tuples(rows)[:nq or n]) and not spectrum.any()
    assert call() == 0 and (as_tuples(rows), spectrum.tolist()) == want
    assert check(ctx, sketches, 31, thresholds=((1, 2),)) == want


@pytest.mark.gpu
def test_prevalence_files_and_the_command_line(ctx, tmp_path):
    pl = collection(31, 11)[:24]
    sets = [key_set(p) for p in pl]
    card = [len(s) for s in sets]
    paths = write_files(tmp_path, pl)
    want_rows, want_spectrum = model(sets, 0, 95, 100)
    rows, spectrum = ctx.prevalence_files(paths, str(tmp_path / "lib"), 95, 100)
    assert as_tuples(rows) == want_rows and spectrum.tolist() == want_spectrum
    texts = [py_csv(want_rows, paths, card), py_spectrum_csv(want_spectrum)]
    both = lambda tag: [gunzip(str(tmp_path / (tag + suf))) for suf in ("_prevalence.csv.gz", "_spectrum.csv.gz")]
    assert both("lib") == texts
    ctx.prevalence_files(paths, str(tmp_path / "p3"), 95, 100, precision=3)
    assert both("p3") == [py_csv(want_rows, paths, card, 3), texts[1]]
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    r = run("-P", "0.95", "-f", "bank.txt", "-o", "cli")
    assert r.returncode == 0, r.stdout + r.stderr
    assert both("cli") == texts
    assert not [f for f in os.listdir(tmp_path) if f.startswith("cli") and ("jaccard" in f or "containment" in f)]
    core_min = -(-95 * 24 // 100)
    line = "24 reference(s), %d distinct keys, %d of them core (held by %d references or more)" % (sum(want_spectrum), sum(want_spectrum[core_min:]), core_min)
    assert line in r.stdout.splitlines(), r.stdout
    # the -q form: three queries against the references, one sketch without keys on either side
    ql = three_queries(31, 11)
    qsets = [key_set(p) for p in ql]
    qpaths = write_files(tmp_path, ql, "q")
    q_rows, q_spectrum = model(qsets, 3, 1, 2)
    q_texts = [py_csv(q_rows, qpaths, [len(s) for s in qsets]), py_spectrum_csv(q_spectrum)]
    rows, spectrum = ctx.prevalence_files(qpaths, str(tmp_path / "qlib"), 1, 2, n_query=3)
    assert as_tuples(rows) == q_rows and spectrum.tolist() == q_spectrum and both("qlib") == q_texts
    (tmp_path / "q.txt").write_text("\n".join(qpaths[:3]) + "\n")
    (tmp_path / "qbank.txt").write_text("\n".join(qpaths[3:]) + "\n")
    r = run("-P", "0.5", "-q", "q.txt", "-f", "qbank.txt", "-o", "qcli")
    assert r.returncode == 0, r.stdout + r.stderr
    assert both("qcli") == q_texts
    # without -P: the two matrices, as before
    r = run("-f", "bank.txt", "-o", "plain")
    assert r.returncode == 0, r.stdout + r.stderr
    inter, c2, _, _ = orc.compare(pl)
    for jac, suf in ((True, "_jaccard.csv.gz"), (False, "_containment.csv.gz")):
        assert gunzip(str(tmp_path / ("plain" + suf))) == orc.csv(jac, paths, inter, c2, None, 6, 0.0)
    assert not os.path.exists(str(tmp_path / "plain_prevalence.csv.gz"))


@pytest.mark.gpu
def test_prevalence_files_at_a_common_rate(ctx, tmp_path):
    k, m = 31, 11
    refs = _references()
    coarse = collection(k, m)[:12]
    mixed_rates = [_sketch(g, "g%d" % i, k, m, 10.0) if i % 3 == 0 else coarse[i] for i, g in enumerate(refs[:12])]
    paths = write_files(tmp_path, mixed_rates)
    sets = [key_set(p) for p in coarse]
    want_rows, want_spectrum = model(sets, 0, 1, 2)
    rows, spectrum = ctx.prevalence_files(paths, str(tmp_path / "auto"), 1, 2, rate="auto")
    assert as_tuples(rows) == want_rows and spectrum.tolist() == want_spectrum
    assert gunzip(str(tmp_path / "auto_prevalence.csv.gz")) == py_csv(want_rows, paths, [len(s) for s in sets])
    assert gunzip(str(tmp_path / "auto_spectrum.csv.gz")) == py_spectrum_csv(want_spectrum)
    rows, spectrum = ctx.prevalence_files(paths, str(tmp_path / "r100"), 1, 2, rate=100)
    assert as_tuples(rows) == want_rows and spectrum.tolist() == want_spectrum
    # as the files are: another question with another answer
    asis = [key_set(p) for p in mixed_rates]
    rows, spectrum = ctx.prevalence_files(paths, str(tmp_path / "asis"), 1, 2)
    assert (as_tuples(rows), spectrum.tolist()) == model(asis, 0, 1, 2) and len(asis[0]) > 5 * len(sets[0])
    # a requested rate finer than a file: refused, naming the file
    with pytest.raises(sp.SpspError) as e:
        ctx.prevalence_files(paths, str(tmp_path / "no"), 1, 2, rate=10)
    assert e.value.code == sp.ERR_ARG and "upsample" in str(e.value)
    # k == m: refused with and without a rate
    kk = [_sketch(g[:5000], "g%d" % i, 11, 11) for i, g in enumerate(refs[:3])]
    p3 = write_files(tmp_path, kk, "kk")
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.prevalence_files(p3, str(tmp_path / "no"), 1, 2, rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]
