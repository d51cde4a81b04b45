"""Gather: which references make up a query sketch, greedily (include/spsp.h: spsp_gather_device, spsp_gather_csv_host,
spsp_gather_files; bin/comparator -g).

The rule, on sets of the comparator's keys (orc.sketch_keys: the distinct (minimizer, canonical k-mer) pairs of a sketch).
Q = the keys of one query, R_0 .. R_{N-1} those of the references in list order, A_0 = Q.  Round r = 1, 2, ...:

    1. u_j = |R_j & A_{r-1}| for every reference
    2. j* = the SMALLEST j among those with the largest u_j
    3. stop if u_j* < min_keys (min_keys >= 1), or if max_rounds > 0 and r > max_rounds
    4. emit (query, rank = r, match = j*, intersect = |R_j* & Q|, unique = u_j*, remaining = |A_{r-1}| - u_j*)
    5. A_r = A_{r-1} - R_j*

Every expected value below comes from the ORACLE's key sets and Python set algebra (gather_model, written from the five
steps): integers and bytes, no tolerance anywhere."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
from oracle import oracle_py as orc
from supersampler_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KM = ((31, 11), (21, 9), (63, 15))
S = 100.0
HEADER = "query,rank,match,intersect,unique,f_unique_query,f_match,remaining\n"


def gather_model(Q, Rs, min_keys, max_rounds=0):
    """the five steps over Python sets -> [(rank, j, intersect, unique, remaining)]"""
    assert min_keys >= 1
    A, rows, r = set(Q), [], 0
    while True:
        r += 1
        u = [len(R & A) for R in Rs]
        best = max(u) if u else 0
        if best < min_keys or (max_rounds > 0 and r > max_rounds):
            return rows
        j = u.index(best)                                                   # the first of the largest
        rows.append((r, j, len(Rs[j] & Q), best, len(A) - best))
        A -= Rs[j]


def key_set(payload):
    _, _, mn, lo, hi = orc.sketch_keys(payload)
    return set(zip(mn.tolist(), hi.tolist(), lo.tolist()))


def model_rows(payloads, n_query, min_keys, max_rounds=0):
    """-> ([(query, rank, match (index in the list), intersect, unique, remaining)] ordered by (query, rank), key counts)"""
    sets = [key_set(p) for p in payloads]
    out = []
    for q in range(n_query):
        out += [(q, r, n_query + j, i, u, left) for r, j, i, u, left in gather_model(sets[q], sets[n_query:], min_keys, max_rounds)]
    return out, [len(s) for s in sets]


def as_tuples(rows):
    assert not np.any(rows["reserved"])
    return [tuple(int(r[f]) for f in ("query", "rank", "match", "intersect", "unique", "remaining")) for r in rows]


def as_rows(tuples):
    rows = np.zeros(len(tuples), dtype=sp.GATHER_ROW_DTYPE)
    for i, (q, r, j, a, u, left) in enumerate(tuples):
        rows[i] = (q, r, j, 0, a, u, left)
    return rows


def py_csv(tuples, names, card, precision=6):
    text = HEADER
    for q, r, j, a, u, left in tuples:
        text += "%s,%d,%s,%d,%d,%s,%s,%d\n" % (names[q], r, names[j], a, u, "%.*g" % (precision, u / card[q]), "%.*g" % (precision, a / card[j]), left)
    return text.encode()


# ------------------------------------------------------------------------------------------ the collections

_cache = {}


def cached(f):
    def g(*a):
        if (f.__name__, a) not in _cache:
            _cache[(f.__name__, a)] = f(*a)
        return _cache[(f.__name__, a)]
    return g


def _fa(genomes, ab, tag="r"):
    """one FASTA holding the genomes as records; with -a 2 every record twice, so that every k-mer is seen twice"""
    return b"".join(synth.to_fasta(g, "%s%d_%d" % (tag, i, c)) for i, g in enumerate(genomes) for c in range(ab))


def _references():
    """48 genomes in 8 families (blocks of six: members 0 and 3 are both the unmutated ancestor) + 12 unrelated ones"""
    refs = synth.family_genomes(5, 48, 60_000, 8, [0.0, 0.01, 0.03])
    rng = np.random.default_rng(6)
    return refs + [synth.random_genome(rng, 60_000) for _ in range(12)]


def _mixture_genomes():
    refs = _references()
    novel = synth.random_genome(np.random.default_rng(7), 60_000)
    return [refs[1], refs[2], refs[13], refs[26], refs[50], novel, refs[40][:1500]]


@cached
def mixture(k, m, ab):
    """payloads: the mixture query first, then the 60 references; sketched by the oracle at -s 100"""
    refs = _references()
    q = orc.sketch_fasta(_fa(_mixture_genomes(), ab, "mix"), k, m, S, ab)[0]
    return [q] + [orc.sketch_fasta(_fa([g], ab, "g%d_" % i), k, m, S, ab)[0] for i, g in enumerate(refs)]


@cached
def three_queries(k, m):
    """queries: the mixture, a genome that shares nothing with any reference, a sequence shorter than k (a sketch without
    buckets); references: the 60 with one more sketch without buckets in the middle"""
    mix = mixture(k, m, 1)
    rng = np.random.default_rng(8)
    alien = orc.sketch_fasta(synth.to_fasta(synth.random_genome(rng, 60_000), "alien"), k, m, S)[0]
    empty = orc.sketch_fasta(synth.to_fasta(synth.random_genome(rng, k - 2), "short"), k, m, S)[0]
    assert empty.count(b"\n") == 1
    return [mix[0], alien, empty] + mix[1:31] + [empty] + mix[31:]


@cached
def beyond_lds(k, m):
    """a query and a reference of more than 8 192 keys each (the decoder's table path) and 2 000 small references"""
    rng = np.random.default_rng(90 + k)
    anc = [synth.random_genome(rng, 10_000) for _ in range(8)]
    small = [synth.mutate(rng, anc[i % 8], [0.0, 0.01, 0.03][(i // 8) % 3]) for i in range(2000)]
    small[1500], small[1999] = synth.random_genome(rng, 12_000), synth.random_genome(rng, 12_000)   # two that belong to no family
    big = synth.random_genome(rng, 1_200_000)
    big_ref = np.concatenate([big[400_000:], synth.random_genome(rng, 500_000)])
    query = [big] + [small[i] for i in (6, 14, 700, 1500, 1999)] + [synth.random_genome(rng, 10_000)]
    pl = [orc.sketch_fasta(_fa(query, 1, "q"), k, m, S)[0]]
    pl += [orc.sketch_fasta(synth.to_fasta(g, "s%d" % i), k, m, S)[0] for i, g in enumerate(small[:900])]
    pl.append(orc.sketch_fasta(synth.to_fasta(big_ref, "bigref", n_records=3), k, m, S)[0])
    pl += [orc.sketch_fasta(synth.to_fasta(g, "s%d" % (900 + i)), k, m, S)[0] for i, g in enumerate(small[900:])]
    return pl


@cached
def many_rounds(k, m):
    """a query made of 150 small unrelated genomes that are all among the 200 references"""
    rng = np.random.default_rng(91)
    gs = [synth.random_genome(rng, 20_000) for _ in range(200)]
    member = sorted(rng.permutation(200)[:150].tolist())
    pl = [orc.sketch_fasta(_fa([gs[i] for i in member], 1, "m"), k, m, S)[0]]
    return pl + [orc.sketch_fasta(synth.to_fasta(g, "u%d" % i), k, m, S)[0] for i, g in enumerate(gs)]


# ------------------------------------------------------------------------------------------------ not GPU

def test_model_on_hand_made_sets():
    K = lambda *xs: {(x, 0, x) for x in xs}
    # a tie taken by the lower index: references 0 and 1 both hold three keys of the query
    assert gather_model(K(1, 2, 3, 4), [K(1, 2, 3), K(2, 3, 4)], 1) == [(1, 0, 3, 3, 1), (2, 1, 3, 1, 0)]
    assert gather_model(K(1, 2, 3, 4), [K(2, 3, 4), K(1, 2, 3)], 1) == [(1, 0, 3, 3, 1), (2, 1, 3, 1, 0)]
    # a second pick whose unique < intersect; the third reference is never named (nothing of it is left)
    Q = K(*range(10))
    Rs = [K(0, 1, 2, 3, 4, 5), K(4, 5, 6, 7, 99), K(0, 1)]
    assert gather_model(Q, Rs, 1) == [(1, 0, 6, 6, 4), (2, 1, 4, 2, 2)]
    # a stop by min_keys with a reference still at 0 < u < min_keys
    assert gather_model(Q, Rs, 3) == [(1, 0, 6, 6, 4)]
    assert gather_model(Q, [K(0, 1, 2, 3), K(8, 9), K(3, 4, 5, 6)], 3) == [(1, 0, 4, 4, 6), (2, 2, 4, 3, 3)]   # (reference 1 stays at 2)
    # max_rounds
    assert gather_model(Q, Rs, 1, max_rounds=1) == [(1, 0, 6, 6, 4)]
    assert gather_model(Q, Rs, 1, max_rounds=5) == gather_model(Q, Rs, 1)
    # an empty query, no references, a reference named at most once
    assert gather_model(set(), Rs, 1) == [] and gather_model(Q, [], 1) == []
    assert gather_model(K(1, 2), [K(1, 2), K(1, 2)], 1) == [(1, 0, 2, 2, 0)]


def test_gather_csv_equals_the_python_writer():
    names = ["q one.fa.gz", "dir/q.two", "ref a.gz", "b.1.2.sketch", "c"]
    card = [1000, 7, 333, 12345, 3]
    rows = [(0, 1, 3, 700, 700, 300), (0, 2, 2, 333, 111, 189), (0, 3, 4, 3, 1, 188), (1, 1, 4, 3, 3, 4)]
    for precision in (6, 3):
        assert sp.gather_csv(as_rows(rows), names, card, 2, precision) == py_csv(rows, names, card, precision)
        assert sp.gather_csv(as_rows([]), names, card, 2, precision) == HEADER.encode()
    assert sp.gather_csv(as_rows(rows), names, card, 2) == py_csv(rows, names, card, 6)
    assert b",0.428571,1,4\n" in sp.gather_csv(as_rows(rows), names, card, 2) and b",0.429,1,4\n" in sp.gather_csv(as_rows(rows), names, card, 2, 3)
    for bad in ((2, 1, 3, 1, 1, 1), (0, 1, 1, 1, 1, 1), (0, 1, 5, 1, 1, 1)):          # a reference as query, a query as match, beyond the list
        with pytest.raises(sp.SpspError) as e:
            sp.gather_csv(as_rows([bad]), names, card, 2)
        assert e.value.code == sp.ERR_ARG


def test_abi_has_the_gather_calls():
    assert {"spsp_gather_device", "spsp_gather_csv_host", "spsp_gather_files"} <= set(sp.ABI_SYMBOLS)
    assert C_sizeof_row() == 40 == sp.GATHER_ROW_DTYPE.itemsize


def C_sizeof_row():
    import ctypes
    return ctypes.sizeof(sp.GatherRow)


@pytest.mark.parametrize("k,m,ab", [(k, m, 1) for k, m in KM] + [(31, 11, 2)])
def test_the_mixture_shows_what_it_is_there_for(k, m, ab):
    """at least five rows; a row with unique < intersect; keys that stay unexplained; (31/11, 21/9) an unnamed reference left
    at 0 < u < min_keys when the run stops"""
    pl = mixture(k, m, ab)
    rows, card = model_rows(pl, 1, 25)
    assert len(rows) >= 5, rows
    assert any(u < a for _, _, _, a, u, _ in rows), rows
    assert rows[-1][5] > 0 and card[0] - sum(r[4] for r in rows) == rows[-1][5]
    assert [r[4] for r in rows] == sorted((r[4] for r in rows), reverse=True) and len({r[2] for r in rows}) == len(rows)
    if (k, m) != (63, 15):
        sets = [key_set(p) for p in pl]
        A = set(sets[0])
        for r in rows:
            A -= sets[r[2]]
        left = [len(R & A) for R in sets[1:]]
        assert any(0 < x < 25 for x in left) and max(left) < 25, sorted(left)[-8:]


def test_the_tie_collection_has_a_tie():
    pl = mixture(31, 11, 1)
    assert pl[1 + 0] == pl[1 + 3] and key_set(pl[1]) == key_set(pl[4]) and len(key_set(pl[1])) > 100
    rows, _ = model_rows([pl[1]] + pl[1:], 1, 25)
    assert rows[0][2] == 1 and 4 not in [r[2] for r in rows]


@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_the_three_queries_are_what_they_are_called(k, m):
    pl = three_queries(k, m)
    rows, card = model_rows(pl, 3, 25)
    assert card[2] == 0 and card[3 + 30] == 0 and card[1] > 100
    assert {r[0] for r in rows} == {0} and len(rows) >= 5
    assert not any(key_set(pl[1]) & key_set(p) for p in pl[3:])


def test_the_collection_beyond_the_lds_limits_is_beyond_them():
    pl = beyond_lds(31, 11)
    assert len(pl) == 1 + 2001
    rows, card = model_rows(pl, 1, 5)
    assert card[0] > 8192 and card[1 + 900] > 8192 and rows[0][2] == 1 + 900
    assert len(rows) >= 5 and rows[-1][5] > 0
    assert max(r[2] for r in rows) > 1 + 1024                               # a winner beyond one workgroup's first pass of counters


def test_many_rounds_are_many():
    rows, _ = model_rows(many_rounds(31, 11), 1, 5)
    assert len(rows) == 150
    assert len(model_rows(many_rounds(31, 11), 1, 5, 10)[0]) == 10


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def gpu_rows(ctx, payloads, n_query, min_keys, max_rounds=0):
    k, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
    return as_tuples(ctx.gather_device(k, d_mn, d_lo, d_hi, off, len(payloads), n_query, min_keys, max_rounds))


def write_files(root, payloads, tag="f"):
    paths = []
    for i, p in enumerate(payloads):
        paths.append(os.path.join(str(root), "%s %03d.sk.gz" % (tag, i)))  # (names with a space and dots)
        sp.write_gz(paths[-1], p, 1)
    return paths


def gunzip(path):
    return gzip.open(path, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("k,m,ab", [(k, m, 1) for k, m in KM] + [(31, 11, 2)])
def test_gather_of_a_mixture(ctx, k, m, ab):
    pl = mixture(k, m, ab)
    want, _ = model_rows(pl, 1, 25)
    assert len(want) >= 5
    assert gpu_rows(ctx, pl, 1, 25) == want
    assert gpu_rows(ctx, pl, 1, 1) == model_rows(pl, 1, 1)[0]
    assert gpu_rows(ctx, pl, 1, 25, 3) == want[:3]


@pytest.mark.gpu
def test_gather_ties_go_to_the_reference_listed_first(ctx):
    pl = mixture(31, 11, 1)
    refs = pl[1:]
    want, _ = model_rows([refs[0]] + refs, 1, 25)
    got = gpu_rows(ctx, [refs[0]] + refs, 1, 25)
    assert got == want and got[0][2] == 1 and 4 not in [r[2] for r in got]
    # the same two in the other order of files: whichever is listed first is named
    swapped = [refs[3], refs[1], refs[2], refs[0]] + refs[4:]
    assert swapped[0] == swapped[3]
    got = gpu_rows(ctx, [refs[0]] + swapped, 1, 25)
    assert got == model_rows([refs[0]] + swapped, 1, 25)[0] and got[0][2] == 1 and 4 not in [r[2] for r in got]


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_gather_three_queries_in_one_call_equal_each_alone(ctx, k, m):
    pl = three_queries(k, m)
    want, _ = model_rows(pl, 3, 25)
    got = gpu_rows(ctx, pl, 3, 25)
    assert got == want and {r[0] for r in got} == {0}
    alone = []
    for q in range(3):
        alone += [(q, r, j + 2, a, u, left) for _, r, j, a, u, left in gpu_rows(ctx, [pl[q]] + pl[3:], 1, 25)]
    assert alone == got
    # the queries in another order: the same rows under other query numbers
    perm = [pl[1], pl[2], pl[0]] + pl[3:]
    assert gpu_rows(ctx, perm, 3, 25) == [(2,) + r[1:] for r in want]


@pytest.mark.gpu
def test_gather_beyond_the_lds_limits(ctx):
    pl = beyond_lds(31, 11)
    want, card = model_rows(pl, 1, 5)
    assert card[0] > 8192 and card[901] > 8192
    assert gpu_rows(ctx, pl, 1, 5) == want


@pytest.mark.gpu
def test_gather_many_rounds(ctx):
    pl = many_rounds(31, 11)
    want, _ = model_rows(pl, 1, 5)
    assert len(want) == 150
    assert gpu_rows(ctx, pl, 1, 5) == want
    assert gpu_rows(ctx, pl, 1, 5, 10) == want[:10]
    assert gpu_rows(ctx, pl, 1, 5, 33) == want[:33]


@pytest.mark.gpu
def test_gather_device_with_too_little_room_and_bad_arguments(ctx):
    import ctypes as C
    pl = mixture(31, 11, 1)
    want, _ = model_rows(pl, 1, 25)
    k, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(pl)
    L = sp.lib()
    rows = np.zeros(2, dtype=sp.GATHER_ROW_DTYPE)
    cnt = C.c_uint64()
    call = lambda r, cap, n=len(pl), nq=1, mk=25: L.spsp_gather_device(ctx._h, k, d_mn, d_lo, d_hi, off.ctypes.data, n, nq, mk, 0, r.ctypes.data, cap, C.byref(cnt))
    assert call(rows, 2) == sp.ERR_OVERFLOW and cnt.value == len(want) and not rows["rank"].any()
    rows = np.zeros(cnt.value, dtype=sp.GATHER_ROW_DTYPE)
    assert call(rows, len(rows)) == 0 and cnt.value == len(want) and as_tuples(rows) == want
    for kw in (dict(nq=0), dict(nq=len(pl)), dict(mk=0)):
        assert call(rows, len(rows), **kw) == sp.ERR_ARG, kw
    big_off = np.zeros(65537 + 1, dtype=np.uint64)
    assert L.spsp_gather_device(ctx._h, k, d_mn, d_lo, d_hi, big_off.ctypes.data, 65537, 1, 1, 0, rows.ctypes.data, len(rows), C.byref(cnt)) == sp.ERR_ARG
    ctx.compare_keys_unordered(True)
    try:
        assert call(rows, len(rows)) == sp.ERR_ARG
    finally:
        ctx.compare_keys_unordered(False)
    assert call(rows, len(rows)) == 0 and as_tuples(rows) == want


@pytest.mark.gpu
def test_gather_files_at_a_common_rate(ctx, tmp_path):
    k, m = 31, 11
    refs = _references()
    q_fa = _fa(_mixture_genomes(), 1, "mix")
    coarse = mixture(k, m, 1)
    mixed = [orc.sketch_fasta(q_fa, k, m, 10.0)[0]] + coarse[1:]
    paths = write_files(tmp_path, mixed)
    want, card = model_rows(coarse, 1, 25)
    got = ctx.gather_files(paths, str(tmp_path / "auto"), 1, 25, rate="auto")
    assert as_tuples(got) == want
    assert gunzip(str(tmp_path / "auto_gather.csv.gz")) == py_csv(want, paths, card)
    got = ctx.gather_files(paths, str(tmp_path / "r100"), 1, 25, rate=100, precision=3)
    assert as_tuples(got) == want and gunzip(str(tmp_path / "r100_gather.csv.gz")) == py_csv(want, paths, card, 3)
    # as the files are: the fine query against coarse references is another question with another answer
    asis, card_asis = model_rows(mixed, 1, 25)
    assert as_tuples(ctx.gather_files(paths, str(tmp_path / "asis"), 1, 25)) == asis and card_asis[0] > 5 * card[0]
    assert gunzip(str(tmp_path / "asis_gather.csv.gz")) == py_csv(asis, paths, card_asis)
    # references finer than the query, and a requested rate finer than a file: refused, naming the file
    fine_refs = [orc.sketch_fasta(synth.to_fasta(g, "g%d" % i), k, m, 10.0)[0] for i, g in enumerate(refs[:4])]
    p2 = write_files(tmp_path, [coarse[0]] + fine_refs, "up")
    with pytest.raises(sp.SpspError) as e:
        ctx.gather_files(p2, str(tmp_path / "no"), 1, 25, rate=10)
    assert e.value.code == sp.ERR_ARG and os.path.basename(p2[0]) in str(e.value) and "upsample" in str(e.value)
    assert as_tuples(ctx.gather_files(p2, str(tmp_path / "yes"), 1, 25, rate="auto")) == model_rows([coarse[0]] + coarse[1:5], 1, 25)[0]
    # k == m: refused with and without a rate
    kk = [orc.sketch_fasta(synth.to_fasta(g[:5000], "g%d" % i), 11, 11, S)[0] for i, g in enumerate(refs[:3])]
    p3 = write_files(tmp_path, kk, "kk")
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.gather_files(p3, str(tmp_path / "no"), 1, 1, rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    assert not os.path.exists(str(tmp_path / "no_gather.csv.gz"))


@pytest.mark.gpu
def test_gather_files_and_the_command_line(ctx, tmp_path):
    pl = three_queries(31, 11)
    paths = write_files(tmp_path, pl)
    want, card = model_rows(pl, 3, 5)
    text = py_csv(want, paths, card)
    assert as_tuples(ctx.gather_files(paths, str(tmp_path / "lib"), 3, 5)) == want
    assert gunzip(str(tmp_path / "lib_gather.csv.gz")) == text
    (tmp_path / "q.txt").write_text("\n".join(paths[:3]) + "\n")
    (tmp_path / "bank.txt").write_text("\n".join(paths[3:]) + "\n")
    exe = os.path.join(ROOT, "bin", "comparator")
    run = lambda *a: subprocess.run([exe] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    r = run("-g", "5", "-q", "q.txt", "-f", "bank.txt", "-o", "cli")
    assert r.returncode == 0, r.stdout + r.stderr
    assert gunzip(str(tmp_path / "cli_gather.csv.gz")) == text
    assert not os.path.exists(str(tmp_path / "cli_jaccard.csv.gz")) and not os.path.exists(str(tmp_path / "cli_containment.csv.gz"))
    out = r.stdout.splitlines()
    assert out[0] == "I query 3 file(s) against the bank"
    n0 = sum(1 for x in want if x[0] == 0)
    assert "%s: %d reference(s) named, %d of %d keys remain" % (paths[0], n0, want[n0 - 1][5], card[0]) in out
    assert "%s: 0 reference(s) named, %d of %d keys remain" % (paths[1], card[1], card[1]) in out
    assert "%s: 0 reference(s) named, 0 of 0 keys remain" % paths[2] in out
    for args in (("-g", "5", "-f", "bank.txt", "-o", "bad"), ("-g", "0", "-q", "q.txt", "-f", "bank.txt", "-o", "bad"),
                 ("-g", "five", "-q", "q.txt", "-f", "bank.txt", "-o", "bad")):
        r = run(*args)
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and "-g" in r.stdout, (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
    # without -g: the oracle's two matrices, as before
    r = run("-q", "q.txt", "-f", "bank.txt", "-o", "plain")
    assert r.returncode == 0, r.stdout + r.stderr
    inter, c2, _, _ = orc.compare(pl, n_query=3)
    for jac, suf in ((True, "_jaccard.csv.gz"), (False, "_containment.csv.gz")):
        assert gunzip(str(tmp_path / ("plain" + suf))) == orc.csv(jac, paths, inter, c2, 3, 6, 0.0)
    assert not os.path.exists(str(tmp_path / "plain_gather.csv.gz"))


@pytest.mark.gpu
def test_the_context_after_a_gather(ctx, tmp_path):
    a, b = mixture(31, 11, 1), many_rounds(31, 11)
    paths = write_files(tmp_path, a[:20])
    files = lambda tag: [gunzip(str(tmp_path / (tag + suf))) for suf in ("_jaccard.csv.gz", "_containment.csv.gz")]
    ctx.compare_files(paths, str(tmp_path / "before"))
    first = gpu_rows(ctx, a, 1, 25)
    assert first == model_rows(a, 1, 25)[0]
    ctx.compare_files(paths, str(tmp_path / "after"))
    assert files("before") == files("after")
    inter, card, _, _ = orc.compare(a[:20])
    assert files("after") == [orc.csv(jac, paths, inter, card, None, 6, 0.0) for jac in (True, False)]
    # buffers that grow and are reused: a larger collection, a wider one, then the first again
    assert gpu_rows(ctx, b, 1, 5) == model_rows(b, 1, 5)[0]
    c = three_queries(63, 15)
    assert gpu_rows(ctx, c, 3, 25) == model_rows(c, 3, 25)[0]
    assert gpu_rows(ctx, a, 1, 25) == first
    # the decoder's arrays stay as the gather found them
    k, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(a)
    before = (ctx.to_host(d_mn, int(off[-1]), np.uint32), ctx.to_host(d_lo, int(off[-1]), np.uint64))
    ctx.gather_device(k, d_mn, d_lo, d_hi, off, len(a), 1, 25)
    assert np.array_equal(before[0], ctx.to_host(d_mn, int(off[-1]), np.uint32)) and np.array_equal(before[1], ctx.to_host(d_lo, int(off[-1]), np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_from_reads_to_an_answer(ctx, tmp_path, k, m):
    pl = mixture(k, m, 1)
    gs = _mixture_genomes()
    fasta = _fa(gs, 1, "mix")
    fastq = b"".join(b"@mix%d\n%s\n+\n%s\n" % (i, g.tobytes(), b"I" * len(g)) for i, g in enumerate(gs))
    want, card = model_rows(pl, 1, 25)
    ref_paths = write_files(tmp_path, pl[1:], "ref")
    for tag, text in (("fa", fasta), ("fq", fastq)):
        q = ctx.sketch_text(text, k, m, S)[0]
        qp = str(tmp_path / (tag + ".query.gz"))
        sp.write_gz(qp, q, 1)
        assert as_tuples(ctx.gather_files([qp] + ref_paths, str(tmp_path / tag), 1, 25)) == want, tag
        assert gunzip(str(tmp_path / (tag + "_gather.csv.gz"))) == py_csv(want, [qp] + ref_paths, card), tag
