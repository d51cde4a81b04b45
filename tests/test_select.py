"""Select: the keys of a collection whose holder count lies in a band, written out as sketches again (include/spsp.h:
spsp_keys_select_device, spsp_select_band_host, spsp_sketch_from_keys_host, spsp_select_files; bin/comparator -S / -E).

The rule, on sets of the comparator's keys.  n_query == 0: every sketch is a row and a reference, R = n.  n_query > 0: the first
n_query sketches are rows only, the R = n - n_query behind them the references.  h(x) = the references that hold key x.  A key
passes the band [h_min, h_max] iff h_min <= h(x) <= h_max; h_min > h_max is the empty band.

    each    every row sketch keeps its passing keys, in their old order
    merged  the distinct keys of the references' union that pass, sorted by (minimizer, kmer_hi, kmer_lo): one sketch

Every expected value comes from collections.Counter over key tuples and Python integers (model_each, model_merged, band):
integers and bytes, no tolerance anywhere.  The hand-built shapes and the sketched collections of the prevalence tests are
shared (test_prevalence: pack, pool, star, ...): the two features read the same arrays and must agree on them.

Where the kernels cut, and the shapes that sit on the cuts: the flag kernel and the compaction work on tiles of 2048 entries in
ballot words of 64 (sketches of 63 .. 65, 255 .. 257 and 2047 .. 2049 keys in one call); the merged form's sort takes chunks of
2048 keys and merges them in passes (unions of 2047, 2048, 2049 and 4097 keys); the table has a power of two of slots
(SPSP_DEBUG_PREVALENCE_TABLE=min: every slot taken, probe sequences wrap)."""
import gzip
import os
import subprocess
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import supersampler_amd as sp
import test_prevalence as tp
from oracle import oracle_py as orc
from supersampler_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
EMPTY = (1, 0)
U64 = (1 << 64) - 1


# -------------------------------------------------------------------------------------------------- the model

def band(what, R):
    """the band a word stands for among R references; classes as tp.key_class counts them"""
    if what in ("union", "present"):
        return (1, R)
    if what == "absent":
        return (0, 0)
    if what == "all":
        return (R, R)
    if "=" in what:
        name, t = what.split("=")
        f = Fraction(t)                                                               # (exact: the text, not a float)
        core_min = -((-f.numerator * R) // f.denominator)
        if name == "core":
            return (core_min, R)
        if name == "unique":
            return (1, 1) if core_min > 1 else EMPTY
        if name == "shell":
            return (2, core_min - 1) if core_min > 2 else EMPTY
    a, b = what.split("..")
    return (int(a), int(b))


def holders(sets, n_query):
    return Counter(x for s in sets[n_query:] for x in set(s))


def model_each(sets, n_query, h_min, h_max):
    h = holders(sets, n_query)
    return [[x for x in sorted(set(s)) if h_min <= h[x] <= h_max] for s in (sets[:n_query] if n_query else sets)]


def model_merged(sets, h_min, h_max):
    return sorted(x for x, c in holders(sets, 0).items() if h_min <= c <= h_max)


# ------------------------------------------------------------------------------------------------ not GPU

def K(*xs):
    return {(x, 0, x) for x in xs}


def test_model_and_bands_on_hand_made_cases():
    # R = 20: key 1 in all, key 2 in 19, key 3 in 18, key 100 + j in sketch j alone
    sets = [K(1, 100 + j) | (K(2) if j < 19 else set()) | (K(3) if j < 18 else set()) for j in range(20)]
    assert model_merged(sets, *band("union", 20)) == sorted(set().union(*sets)) and len(model_merged(sets, *band("present", 20))) == 23
    assert model_merged(sets, *band("all", 20)) == sorted(K(1)) and model_merged(sets, *band("absent", 20)) == []
    assert band("core=0.95", 20) == (19, 20) and model_merged(sets, 19, 20) == sorted(K(1, 2))
    assert band("shell=0.95", 20) == (2, 18) and model_merged(sets, 2, 18) == sorted(K(3))
    assert band("unique=0.95", 20) == (1, 1) and model_merged(sets, 1, 1) == sorted(K(*range(100, 120)))
    assert model_each(sets, 0, 19, 20)[19] == sorted(K(1)) and model_each(sets, 0, 1, 1)[3] == sorted(K(103))
    # core=0.05 with R = 20: core_min = 1, so h = 1 is core, and unique= and shell= are empty
    assert band("core=0.05", 20) == (1, 20) and band("unique=0.05", 20) == EMPTY and band("shell=0.05", 20) == EMPTY
    assert model_merged(sets, *band("core=0.05", 20)) == model_merged(sets, 1, 20) and model_merged(sets, *EMPTY) == []
    assert band("shell=0.1", 20) == EMPTY and band("unique=0.1", 20) == (1, 1)        # core_min = 2: nothing between unique and core
    assert band("shell=0.15", 20) == (2, 2)
    # R = 1: `all` is the sketch itself, everything present is core
    assert band("all", 1) == (1, 1) == band("core=1", 1) == band("union", 1) and band("unique=1", 1) == EMPTY
    assert model_merged([K(4, 5)], *band("all", 1)) == sorted(K(4, 5)) == model_each([K(4, 5)], 0, 1, 1)[0]
    assert band("3..7", 9) == (3, 7) and band("7..3", 9) == (7, 3) and model_merged(sets, 7, 3) == []
    # the classes are the prevalence pass's, to the letter: every key of every row falls into the band of its class and no other
    for num, den, t in ((95, 100, "0.95"), (1, 20, "0.05"), (1, 10, "0.1"), (1, 1, "1")):
        q = [K(1, 2, 50), K(100)] + sets
        for nq, ss in ((0, sets), (2, q)):
            R, h = len(ss) - nq, holders(ss, nq)
            for x in set().union(*ss[:nq or len(ss)]):
                cls = tp.key_class(h[x], R, num, den)
                inside = [w for w in ("core", "shell", "unique") if band("%s=%s" % (w, t), R)[0] <= h[x] <= band("%s=%s" % (w, t), R)[1]]
                inside += ["absent"] if h[x] == 0 else []
                assert inside == [cls], (x, h[x], t, inside, cls)
    # queries: absent keys, and h counts references only
    q = [K(1, 2, 50, 51), K(50), set()]
    assert model_each(q + sets, 3, 0, 0) == [sorted(K(50, 51)), sorted(K(50)), []]
    assert model_each(q + sets, 3, 19, 20) == [sorted(K(1, 2)), [], []]


WORDS = ("union", "present", "absent", "all", "core=0.05", "unique=0.05", "shell=0.05", "core=0.95", "unique=0.95", "shell=0.95", "core=1", "shell=1",
         "unique=1", "core=0.000001", "shell=0.1", "shell=0.15", "core=0.999999", "3..7", "7..3", "0..0", "0..4294967295")


def test_select_band_equals_the_model_and_refuses_garbage():
    for R in (1, 2, 3, 20, 8193, 65535):
        for w in WORDS:
            got, want = sp.select_band(w, R), band(w, R)
            assert got == want or (want[0] > want[1] and "=" in w and got == EMPTY), (w, R, got, want)
    assert sp.select_band("core=0.05", 20) == (1, 20) and sp.select_band("unique=0.05", 20) == EMPTY and sp.select_band("shell=0.05", 20) == EMPTY
    assert sp.select_band("all", 1) == (1, 1) and sp.select_band("7..3", 9) == (7, 3)
    for w in ("", "core", "core=", "core=0", "core=1.5", "core=0.1234567", "core=.5", "kernel=0.5", "union=0.5", "1..", "..2", "1...2", "1..2..3",
              "4294967296..5", "-1..2", "5", " union", "Union", "core=0.5 ", "abc"):
        with pytest.raises(sp.SpspError) as e:
            sp.select_band(w, 5)
        assert e.value.code == sp.ERR_ARG, w
    with pytest.raises(sp.SpspError):
        sp.select_band("union", 0)


def revcomp(v, n):
    r = 0
    for _ in range(n):
        r = (r << 2) | ((v & 3) ^ 2)                                                  # A=0 C=1 T=2 G=3
        v >>= 2
    return r


def plant(kmer, mn, at, k, m):
    """the key of a k-mer with minimizer value mn written over its bases at.. at + m: (mn, kmer_hi, kmer_lo), canonical"""
    sh = 2 * (k - m - at)
    kmer = (kmer & ((1 << 2 * k) - 1) & ~(((1 << 2 * m) - 1) << sh)) | (mn << sh)
    c = min(kmer, revcomp(kmer, k))
    return (mn, c >> 64, c & U64)


def writer_keys(k, m, seed=3, count=150):
    rng = np.random.default_rng(seed + k)
    word = lambda: int.from_bytes(rng.bytes(16), "little")
    keys = [plant(word(), int(rng.integers(0, 1 << 2 * m)), (0, (k - m) // 2, k - m)[t % 3], k, m) for t in range(count)]
    own_rc = int("02" * 8, 4) >> (2 * (16 - m)) if m % 2 == 0 else None               # ATAT...: its own reverse complement (m even)
    both = int(rng.integers(0, 1 << 2 * m))
    keys.append(plant((word() & ~((1 << 2 * m) - 1)) | revcomp(both, m), both, 0, k, m))   # the minimizer on both strands
    keys += [plant(1, 5, 0, k, m), plant(U64 << 64 | U64, 5, k - m, k, m), plant(77, 2, 0, k, m)]   # two keys of one minimizer and a lone one
    if own_rc is not None:
        keys.append(plant(word(), own_rc, 1, k, m))
    return sorted(set(keys))


def arrays(keys, k):
    mn = np.array([x[0] for x in keys], dtype=np.uint32)
    hi = np.array([x[1] for x in keys], dtype=np.uint64)
    lo = np.array([x[2] for x in keys], dtype=np.uint64)
    return mn, lo, (hi if k > 32 else None)


def read_back(payload):
    """the three readers: the oracle's, the library's host parser, the header -> (key tuples, key tuples, header)"""
    _, _, mn, lo, hi = orc.sketch_keys(payload)
    s = sp.sketch_parse(payload)
    return (list(zip(mn.tolist(), hi.tolist(), lo.tolist())), list(zip(s.minimizer.tolist(), s.kmer_hi.tolist(), s.kmer_lo.tolist())),
            sp.sketch_header(payload))


@pytest.mark.parametrize("k,m", [(31, 11), (63, 15), (32, 15), (33, 15), (32, 12)])
def test_the_writer_round_trips_exactly(k, m):
    keys = writer_keys(k, m)
    assert len({x[0] for x in keys}) < len(keys) and any(x[0] == revcomp(x[0], m) for x in keys) == (m % 2 == 0)
    for part, rate in ((keys, 100.0), (keys[:1], 1.0), ([], 1000.0), ([x for x in keys if x[0] == 5], 10.5)):
        payload = sp.sketch_from_keys(k, m, rate, *arrays(part, k))
        a, b, header = read_back(payload)
        assert a == part and b == part and header == (k, m, len(part), rate)
        assert payload.startswith(b"%d %d %d %f\n" % (2 * k - m, m, len(part), rate))
    assert sp.sketch_from_keys(k, m, 100.0, [], []) == b"%d %d 0 100.000000\n" % (2 * k - m, m)
    # one bucket per distinct minimizer, a zero blob size, k - m bases and two line ends per key
    payload = sp.sketch_from_keys(k, m, 100.0, *arrays(keys, k))
    body = len(payload) - len(payload.split(b"\n", 1)[0]) - 1
    assert body == len({x[0] for x in keys}) * (m + 4 + 2) + len(keys) * (k - m + 2)
    # two written sketches compare as their sets do
    a, b = keys[::2] + keys[1::4], keys[1::2]
    pa, pb = (sp.sketch_from_keys(k, m, 100.0, *arrays(sorted(s), k)) for s in (a, b))
    inter, card, kk, mm = orc.compare([pa, pb])
    assert (kk, mm) == (k, m) and card.tolist() == [len(a), len(b)] and inter[0, 1] == len(set(a) & set(b)) > 0


def test_the_writer_refuses():
    k, m = 31, 11
    keys = writer_keys(k, m)
    mn, lo, _ = arrays(keys, k)
    for bad in (np.r_[1:len(keys), 0], np.r_[0, 0:len(keys) - 1]):                    # the first key last; a key twice
        with pytest.raises(sp.SpspError) as e:
            sp.sketch_from_keys(k, m, 100.0, mn[bad], lo[bad])
        assert e.value.code == sp.ERR_ARG and "increasing" in str(e.value)
    wrong = mn.copy()
    wrong[7] = (1 << 2 * m) - 1 if keys[7][0] != (1 << 2 * m) - 1 else 0              # a minimizer its k-mer does not hold ...
    lo7 = lo.copy()
    lo7[7] = 0                                                                        # ... AAA...A, nor its reverse complement
    with pytest.raises(sp.SpspError) as e:
        sp.sketch_from_keys(k, m, 100.0, np.sort(wrong[7:8]), lo7[7:8])
    assert e.value.code == sp.ERR_ARG and "key 0" in str(e.value) and "neither" in str(e.value)
    with pytest.raises(sp.SpspError) as e:
        sp.sketch_from_keys(11, 11, 100.0, [5], [5])
    assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    with pytest.raises(sp.SpspError):
        sp.sketch_from_keys(63, 15, 100.0, [5], [5])                                  # k > 32 without kmer_hi


def test_abi_has_the_select_calls():
    calls = ("spsp_keys_select_device", "spsp_select_band_host", "spsp_sketch_from_keys_host", "spsp_select_files")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    for name in calls:
        assert hasattr(sp.lib(), name)
    assert hasattr(sp.Context, "select_device") and hasattr(sp.Context, "select_files") and callable(sp.sketch_from_keys) and callable(sp.select_band)


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [(f, w) for f in ("-S", "-E") for w in ("", "core", "core=0", "core=1.5", "core=0.1234567", "kernel=0.5", "1..", "5", "Union")]
    cases += [("-S", "union", "-q", "list.txt"), ("-S", "union", "-E", "union"), ("-E", "all", "-E", "union")]
    for f in ("-S", "-E"):
        cases += [(f, "union") + other for other in (("-g", "3", "-q", "list.txt"), ("-c", "0.5"), ("-C", "0.5"), ("-N", "5"), ("-P", "0.5"), ("-r", "0.5"),
                                                     ("-R", "0.5"), ("-l", "0.5"), ("-L", "0.5"))]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and ("-S" in r.stdout or "-E" in r.stdout), (args, r.stdout, r.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def fetch(ctx, k, o_mn, o_lo, o_hi, off):
    """a select call's output -> one list of key tuples per output sketch"""
    total = int(off[-1])
    assert off[0] == 0 and all(int(a) <= int(b) for a, b in zip(off, off[1:]))
    if total == 0:
        return [[] for _ in off[1:]]
    mn, lo = ctx.to_host(o_mn, total, np.uint32), ctx.to_host(o_lo, total, np.uint64)
    hi = ctx.to_host(o_hi, total, np.uint64) if k > 32 else np.zeros(total, np.uint64)
    flat = list(zip(mn.tolist(), hi.tolist(), lo.tolist()))
    return [flat[int(a):int(b)] for a, b in zip(off, off[1:])]


def select(ctx, k, d, off, h_min, h_max, merged=False, n_query=0):
    return fetch(ctx, k, *ctx.select_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, len(off) - 1, h_min, h_max, merged, n_query))


def check(ctx, sketches, k, bands, n_query=0, merged=(False, True)):
    mn, lo, hi, off, order = tp.pack(sketches, k)
    d = tp.upload(mn, lo, hi)
    for h_min, h_max in bands:
        if False in merged:
            got, want = select(ctx, k, d, off, h_min, h_max, False, n_query), model_each(order, n_query, h_min, h_max)
            assert [len(s) for s in got] == [len(s) for s in want], (h_min, h_max)
            assert got == want, (h_min, h_max)
        if True in merged and not n_query:
            got, want = select(ctx, k, d, off, h_min, h_max, True), model_merged(order, h_min, h_max)
            assert len(got) == 1 and len(got[0]) == len(want) and got[0] == want, (h_min, h_max)
            assert all(a < b for a, b in zip(got[0], got[0][1:]))
    del d


def all_bands(R):
    return [(1, R), (R, R), (1, 1), (0, 0), (0, R), EMPTY, (2, max(R - 1, 2)), (0, 0xFFFFFFFF), (R + 1, R + 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_keys_that_differ_in_one_word_only(ctx, k):
    s = tp.seam_sketches(k)
    check(ctx, s, k, all_bands(len(s)) + [(2, 3), (3, 4), (5, 5)])
    check(ctx, s[:3] + s, k, all_bands(len(s)), n_query=3)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_sketch_lengths_on_word_and_tile_boundaries(ctx, k):
    lengths = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
    R = len(lengths)
    bands = [(1, R), (2, 5), (1, 1), (R - 1, R - 1), (4, R)]
    check(ctx, tp.nested_lengths(k, lengths), k, bands)                               # (h of pool key i = the sketches longer than i)
    check(ctx, tp.nested_lengths(k, lengths[::-1]), k, bands)                         # the empty sketch last
    p, q = tp.pool(2100, k), tp.pool(2100, k, salt=100_000)
    queries = [p[:c // 2] + q[:c - c // 2] for c in lengths]                          # half of whose keys nobody holds
    check(ctx, queries + tp.nested_lengths(k, lengths), k, bands + [(0, 0), (0, 2)], n_query=R)
    # empty sketches keep their place; calls without any key
    check(ctx, [[], []] + tp.nested_lengths(k, [5, 3])[:1] + [[]] + tp.nested_lengths(k, [5, 3])[1:] + [[], []], k, all_bands(7))
    check(ctx, [[], [], []], k, all_bands(3))
    check(ctx, [[]], k, all_bands(1))
    check(ctx, [[], tp.pool(5, k)] + [[], []], k, all_bands(2), n_query=2)            # queries against references without keys


@pytest.mark.gpu
def test_band_edges_on_a_nested_collection(ctx):
    k, R = 31, 9
    sketches = tp.nested_lengths(k, [40 * (j + 1) for j in range(R)])                 # h takes every value 1 .. R, 40 keys each
    order = tp.pack(sketches, k)[4]
    h = holders(order, 0)
    assert sorted(set(h.values())) == list(range(1, R + 1))
    a, b = 3, 6
    check(ctx, sketches, k, [(a, b), (a - 1, b), (a, b + 1), (a + 1, b), (a, b - 1), (a, a), EMPTY, (b, a), (0, R), (R, R), (1, R), (R + 1, U64 >> 32)])
    mn, lo, hi, off, _ = tp.pack(sketches, k)
    d = tp.upload(mn, lo, hi)
    got = select(ctx, k, d, off, a, b, True)[0]
    assert {h[x] for x in got} == {3, 4, 5, 6} and len(got) == 160                    # a - 1 and b + 1 stay outside, a and b are inside
    assert select(ctx, k, d, off, 0, R) == order                                      # [0, R] on each: the input, unchanged
    inter = sorted(set.intersection(*map(set, order)))
    assert select(ctx, k, d, off, R, R, True) == [inter] and select(ctx, k, d, off, R, R) == [inter] * R and len(inter) == 40
    assert select(ctx, k, d, off, 1, 0) == [[]] * R and select(ctx, k, d, off, 1, 0, True) == [[]]
    # [0, 0] with three queries: the keys nobody holds
    alien = tp.pool(50, k, salt=700_000)
    queries = [alien[:20] + sketches[0][:10], sketches[8][:100], alien]
    check(ctx, queries + sketches, k, [(0, 0), (1, R), (R, R), (0, R)], n_query=3)
    mn, lo, hi, off, order = tp.pack(queries + sketches, k)
    d = tp.upload(mn, lo, hi)
    got = select(ctx, k, d, off, 0, 0, False, 3)
    assert got == [sorted(alien[:20]), [], sorted(alien)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [2047, 2048, 2049, 4097])
def test_merged_sizes_on_the_sort_chunks(ctx, size):
    """the sort's chunk, one merge pass and two; every sketch's run interleaves with the others' in the sorted order"""
    k = 63 if size == 2049 else 31
    p = sorted(tp.pool(size, k))
    sketches = [p[0::3], p[1::3], p[2::3] + p[0::7], p[5::11], []]                    # neighbours in the order lie in different sketches
    order = tp.pack(sketches, k)[4]
    assert len(model_merged(order, 1, 5)) == size
    check(ctx, sketches, k, [(1, 5), (2, 5), (1, 1)], merged=(True,))
    check(ctx, sketches[::-1], k, [(1, 5)], merged=(True,))


@pytest.mark.gpu
def test_a_key_that_everybody_holds_and_the_smallest_table(ctx, monkeypatch):
    n, k = 8193, 31
    s = tp.star(n, k)
    bands = [(n, n), (n - 1, n), (1, 1)]
    mn, lo, hi, off, order = tp.pack(s, k)
    d = tp.upload(mn, lo, hi)
    want_each = {b: model_each(order, 0, *b) for b in bands}
    want_merged = {b: model_merged(order, *b) for b in bands}
    assert want_merged[(n, n)] == [(3, 0, 1)] and len(want_merged[(n - 1, n)]) == 2 and len(want_merged[(1, 1)]) == n + 1
    small = [(tp.nested_lengths(k, [300, 257, 256, 64, 1, 0, 211]), 0), ([tp.pool(40, k, salt=500_000)] + [tp.pool(512, k, salt=1000 * j) for j in range(8)], 1)]
    for table in ("", "min"):
        if table:
            monkeypatch.setenv("SPSP_DEBUG_PREVALENCE_TABLE", table)                  # every slot taken: probe sequences wrap
        for b in bands:
            assert select(ctx, k, d, off, b[0], b[1]) == want_each[b], (table, b)
            assert select(ctx, k, d, off, b[0], b[1], True) == [want_merged[b]], (table, b)
        for sk, nq in small:
            check(ctx, sk, k, [(1, 7), (2, 3), (0, 0)], n_query=nq)


def count_rows(each):
    return [len(s) for s in each]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_identities_against_the_prevalence_pass(ctx, k, m):
    """two features over one table: the selected keys per row are the prevalence pass's class counts, the merged count is its
    spectrum summed over the band -- on sketched collections, all versus all and with queries"""
    for payloads, nq in ((tp.collection(k, m), 0), (tp.three_queries(k, m), 3)):
        sets = [sorted(tp.key_set(p)) for p in payloads]
        n = len(payloads)
        R = n - nq
        kk, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
        for num, den, t in ((95, 100, "0.95"), (1, 10, "0.1"), (1, 2, "0.5")):
            rows, spectrum = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, num, den, n_query=nq)
            for word, column in (("core=" + t, "core"), ("shell=" + t, "shell"), ("unique=" + t, "unique"), ("absent", "absent")):
                h_min, h_max = sp.select_band(word, R)
                assert (h_min, h_max) == band(word, R) or band(word, R)[0] > band(word, R)[1]
                got = fetch(ctx, k, *ctx.select_device(k, d_mn, d_lo, d_hi, off, n, h_min, h_max, False, nq))
                assert count_rows(got) == rows[column].tolist(), (word, nq)
                assert got == model_each(sets, nq, h_min, h_max), (word, nq)
                if not nq:
                    merged = fetch(ctx, k, *ctx.select_device(k, d_mn, d_lo, d_hi, off, n, h_min, h_max, True))[0]
                    assert len(merged) == sum(spectrum.tolist()[h_min:h_max + 1]) and merged == model_merged(sets, h_min, h_max), word


@pytest.mark.gpu
def test_output_feeds_the_comparison_and_a_second_select(ctx):
    import torch
    k, m = 31, 11
    payloads = tp.collection(k, m)[:24]
    sets = [sorted(tp.key_set(p)) for p in payloads]
    n = len(payloads)
    _, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
    o_mn, o_lo, o_hi, o_off = ctx.select_device(k, d_mn, d_lo, d_hi, off, n, 2, n)     # every sketch without its unique keys
    first = model_each(sets, 0, 2, n)
    assert fetch(ctx, k, o_mn, o_lo, o_hi, o_off) == first
    scratch = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    cells = torch.zeros(1 << 16, dtype=torch.int64, device="cuda")
    cnt = ctx.compare_cells_device(k, o_mn, o_lo, o_hi, o_off, n, scratch.data_ptr(), cells.data_ptr(), 1 << 16)
    torch.cuda.synchronize()
    got = {(int(c) >> 48, (int(c) >> 32) & 0xFFFF): int(c) & 0xFFFFFFFF for c in cells[:cnt].cpu().numpy().view(np.uint64)}
    want = {(i, j): len(set(first[i]) & set(first[j])) for i in range(n) for j in range(i + 1, n) if set(first[i]) & set(first[j])}
    assert got == want and len(want) > 10
    # a select of the select (the other set of output arrays), then one of that (the first set again, while it reads the second)
    p_mn, p_lo, p_hi, p_off = ctx.select_device(k, o_mn, o_lo, o_hi, o_off, n, 3, 5, True)
    second = model_merged(first, 3, 5)
    assert fetch(ctx, k, p_mn, p_lo, p_hi, p_off) == [second] and len(second) > 10
    assert fetch(ctx, k, o_mn, o_lo, o_hi, o_off) == first                            # the first output is still there
    q_mn, q_lo, q_hi, q_off = ctx.select_device(k, p_mn, p_lo, p_hi, p_off, 1, 1, 1)
    assert fetch(ctx, k, q_mn, q_lo, q_hi, q_off) == [second]
    # the merged sketch as a reference of the prevalence pass: every one of its keys is held once
    rows, spectrum = ctx.prevalence_device(k, q_mn, q_lo, q_hi, q_off, 1, 1, 1)
    assert tp.as_tuples(rows) == [(len(second), 0, 0, 0, len(second))]


@pytest.mark.gpu
def test_buffers_are_reused_and_leave_other_calls_alone(ctx):
    k, m = 63, 15
    payloads = tp.three_queries(k, m)
    sets = [sorted(tp.key_set(p)) for p in payloads]
    n = len(payloads)
    kk, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
    total = int(off[-1])
    before = [ctx.to_host(p, total, t) for p, t in ((d_mn, np.uint32), (d_lo, np.uint64), (d_hi, np.uint64))]
    want = model_each(sets, 3, 1, 2)
    a = fetch(ctx, k, *ctx.select_device(k, d_mn, d_lo, d_hi, off, n, 1, 2, False, 3))
    rows, spectrum = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, 1, 2, n_query=3)
    assert (tp.as_tuples(rows), spectrum.tolist()) == tp.model([set(s) for s in sets], 3, 1, 2)
    b = fetch(ctx, k, *ctx.select_device(k, d_mn, d_lo, d_hi, off, n, 1, 2, False, 3))
    assert a == want == b and sum(map(len, want)) > 100
    small, large = tp.nested_lengths(31, [5, 3, 0, 4]), tp.star(3000, 31)
    for s in (small, large, small):
        check(ctx, s, 31, [(1, 2), (3, 3000)])
    after = [ctx.to_host(p, total, t) for p, t in ((d_mn, np.uint32), (d_lo, np.uint64), (d_hi, np.uint64))]
    assert all(np.array_equal(x, y) for x, y in zip(before, after))                   # decode's arrays are intact
    assert fetch(ctx, k, *ctx.select_device(k, d_mn, d_lo, d_hi, off[:n - 2], n - 3, 2, 9, True))[0] == model_merged(sets[:n - 3], 2, 9)


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(ctx):
    k = 31
    sketches = tp.nested_lengths(k, [70, 3, 0, 130])
    mn, lo, hi, off, order = tp.pack(sketches, k)
    d = tp.upload(mn, lo, hi)
    n = len(off) - 1
    L = sp.lib()
    import ctypes as C
    out = np.full(n + 1, 7, dtype=np.uint64)
    ptrs = [C.c_void_p() for _ in range(3)]
    call = lambda n=n, nq=0, merged=0, off=off, d=d: L.spsp_keys_select_device(ctx._h, k, tp.ptr(d[0]), tp.ptr(d[1]), None, off.ctypes.data, n, nq, 1, 2, merged,
                                                                               C.byref(ptrs[0]), C.byref(ptrs[1]), C.byref(ptrs[2]), out.ctypes.data)
    want = model_each(order, 0, 1, 2)
    assert call() == 0 and fetch(ctx, k, ptrs[0].value, ptrs[1].value, None, out) == want
    for kw in (dict(n=0), dict(nq=n), dict(nq=n + 1), dict(nq=1, merged=1)):
        assert call(**kw) == sp.ERR_ARG, kw
    assert call(n=65536, off=np.zeros(65536 + 1, dtype=np.uint64)) == sp.ERR_ARG
    ctx.compare_keys_unordered(True)
    try:
        assert call() == sp.ERR_ARG and "unordered" in L.spsp_last_error().decode()
    finally:
        ctx.compare_keys_unordered(False)
    # unsorted keys: two neighbours swapped inside the last sketch (a reference), inside the first (a query), and a key twice
    for nq, merged, at in ((0, 0, int(off[3]) + 64), (1, 0, 10), (0, 1, int(off[3]) + 1)):
        bad_mn, bad_lo = mn.copy(), lo.copy()
        if at == int(off[3]) + 1:
            bad_mn[at], bad_lo[at] = bad_mn[at - 1], bad_lo[at - 1]
        else:
            bad_mn[[at, at + 1]], bad_lo[[at, at + 1]] = bad_mn[[at + 1, at]], bad_lo[[at + 1, at]]
        bad = tp.upload(bad_mn, bad_lo)
        out[:] = 7
        assert call(nq=nq, merged=merged, d=bad) == sp.ERR_ARG and "increasing" in L.spsp_last_error().decode(), (nq, at)
        assert not out[:(2 if merged else (nq or n) + 1)].any()
    assert call() == 0 and fetch(ctx, k, ptrs[0].value, ptrs[1].value, None, out) == want
    check(ctx, sketches, k, [(1, 2)])


# ------------------------------------------------------------------------------------------ files and the command line

def gunzip(path):
    return gzip.open(path, "rb").read()


def sketched(ctx, k, m):
    """3 queries + 10 references sketched on the device at -s 100: a family of ten around one ancestor; the queries: a mixture, a
    relative, a stranger -> (payloads, key sets)"""
    refs = synth.family_genomes(11, 10, 40_000, 1, [0.0, 0.001, 0.004])
    rng = np.random.default_rng(12)
    alien = synth.random_genome(rng, 40_000)
    genomes = [np.concatenate([refs[2][:20_000], alien[:20_000]]), synth.mutate(rng, refs[0], 0.002), synth.random_genome(rng, 40_000)] + refs
    payloads = [ctx.sketch_text(synth.to_fasta(g, "g%d" % i), k, m, 100.0)[0] for i, g in enumerate(genomes)]
    return payloads, [sorted(tp.key_set(p)) for p in payloads]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_select_files_and_the_command_line(ctx, tmp_path, k, m):
    payloads, sets = sketched(ctx, k, m)
    paths = tp.write_files(tmp_path, payloads)
    q, refs, R = paths[:3], paths[3:], 10
    (tmp_path / "bank.txt").write_text("\n".join(refs) + "\n")
    (tmp_path / "q.txt").write_text("\n".join(q) + "\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    # -S core=0.9: one sketch, read back on the device
    r = run("-S", "core=0.9", "-f", "bank.txt", "-o", "cli")
    assert r.returncode == 0, r.stdout + r.stderr
    core = model_merged(sets[3:], *band("core=0.9", R))
    assert band("core=0.9", R) == (9, 10) and len(core) > 50
    written = gunzip(str(tmp_path / "cli_select.gz"))
    assert sp.sketch_header(written) == (k, m, len(core), 100.0)
    kk, mm, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device([written])
    assert (kk, mm) == (k, m) and fetch(ctx, k, d_mn, d_lo, d_hi, off) == [core]
    line = "10 reference(s), holder counts 9 .. 10: %d key(s) in, %d written to 1 sketch(es)" % (sum(len(s) for s in sets[3:]), len(core))
    assert line in r.stdout.splitlines(), r.stdout
    assert not [f for f in os.listdir(tmp_path) if f.startswith("cli") and f != "cli_select.gz"]
    # the Python call writes the same bytes
    assert ctx.select_files(refs, str(tmp_path / "lib"), "core=0.9") == (sum(len(s) for s in sets[3:]), len(core))
    assert gunzip(str(tmp_path / "lib_select.gz")) == written
    # the three queries against that one file: the intersections are the prevalence pass's core counts in query mode
    inter, card = ctx.compare([sp.sketch_parse(p) for p in payloads[:3] + [written]])
    rows, _ = ctx.prevalence_files(paths, str(tmp_path / "pv"), 9, 10, n_query=3)
    assert inter[:3, 3].tolist() == rows["core"].tolist() == [len(set(s) & set(core)) for s in sets[:3]] and rows["core"][1] > 20
    # -E unique=1: every reference's own keys, and the list of the files as an index
    r = run("-E", "unique=1", "-f", "bank.txt", "-o", "own")
    assert r.returncode == 0, r.stdout + r.stderr
    names = (tmp_path / "own_select.txt").read_text().splitlines()
    assert names == ["own_%d_%s" % (i, os.path.basename(p)) for i, p in enumerate(refs)]
    own = [gunzip(str(tmp_path / f)) for f in names]
    assert [tp.key_set(p) for p in own] == [set(s) for s in model_each(sets[3:], 0, 1, 1)] and all(sp.sketch_header(p)[3] == 100.0 for p in own)
    r = run("-f", "own_select.txt", "-o", "again")
    assert r.returncode == 0, r.stdout + r.stderr
    o_inter, o_card, _, _ = orc.compare(own)
    assert not np.triu(o_inter, 1).any() and o_card.tolist() == [len(s) for s in model_each(sets[3:], 0, 1, 1)]
    assert gunzip(str(tmp_path / "again_jaccard.csv.gz")) == orc.csv(True, names, o_inter, o_card, None, 6, 0.0)
    # -E absent -q: what the queries hold and no reference does
    r = run("-E", "absent", "-q", "q.txt", "-f", "bank.txt", "-o", "new")
    assert r.returncode == 0, r.stdout + r.stderr
    names = (tmp_path / "new_select.txt").read_text().splitlines()
    assert len(names) == 3 and [tp.key_set(gunzip(str(tmp_path / f))) for f in names] == [set(s) for s in model_each(sets, 3, 0, 0)]


@pytest.mark.gpu
def test_select_files_at_mixed_rates(ctx, tmp_path):
    k, m = 31, 11
    payloads, sets = sketched(ctx, k, m)
    refs = synth.family_genomes(11, 10, 40_000, 1, [0.0, 0.001, 0.004])
    fine = [ctx.sketch_text(synth.to_fasta(g, "g%d" % (i + 3)), k, m, 10.0)[0] if i % 3 == 0 else payloads[3 + i] for i, g in enumerate(refs)]
    assert len(tp.key_set(fine[0])) > 4 * len(sets[3])
    paths = tp.write_files(tmp_path, fine)
    with pytest.raises(sp.SpspError) as e:
        ctx.select_files(paths, str(tmp_path / "no"), "union")
    assert e.value.code == sp.ERR_ARG and "different rates" in str(e.value) and not os.path.exists(str(tmp_path / "no_select.gz"))
    union = model_merged(sets[3:], 1, 10)
    for rate in ("auto", 100):
        assert ctx.select_files(paths, str(tmp_path / "u"), "union", rate=rate)[1] == len(union)
        written = gunzip(str(tmp_path / "u_select.gz"))
        assert sp.sketch_header(written) == (k, m, len(union), 100.0) and sorted(tp.key_set(written)) == union
    assert ctx.select_files(paths, str(tmp_path / "e"), "all", each=True, rate="auto")[1] == 10 * len(model_merged(sets[3:], 10, 10))
    with pytest.raises(sp.SpspError) as e:
        ctx.select_files(paths, str(tmp_path / "no"), "union", rate=10)
    assert e.value.code == sp.ERR_ARG and "upsample" in str(e.value)
    kk = [orc.sketch_fasta(synth.to_fasta(g[:5000], "g%d" % i), 11, 11, 100.0)[0] for i, g in enumerate(refs[:3])]
    with pytest.raises(sp.SpspError) as e:
        ctx.select_files(tp.write_files(tmp_path, kk, "kk"), str(tmp_path / "no"), "union")
    assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
