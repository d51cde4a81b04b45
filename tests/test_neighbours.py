"""Neighbours: each sketch's best few partners at or above a threshold, best first (include/spsp.h: spsp_neighbours_cells_device,
spsp_neighbours_csv_host, spsp_neighbours_files; bin/comparator -N <top> [-J | -K | -I <t>] [-q]).

The rule.  Sketches are 0 .. n-1 in list order, c_i = the key count of sketch i, a cell (i, j, x), i < j, names the keys two
sketches share.

    1. rows: every sketch (n_query == n), or the queries 0 .. n_query-1 with the references n_query .. n-1 as their partners
       (a cell between two queries, or two references, is nobody's)
    2. the score of partner p for row r is the fraction x / u:  u = c_r + c_p - x (metric 0, Jaccard), min(c_r, c_p) (metric 1,
       the larger containment), c_r (metric 2, the row's containment in the partner)
    3. p passes for r iff x >= 1 and x * den >= num * u
    4. p comes before q iff x_p / u_p > x_q / u_q as fractions; the smaller index first among equals
    5. per row the first `top` passing partners as (sketch, rank, neighbour, shared), rank 1 the best; rows ordered by (sketch,
       rank); passing[r] = the partners that passed; n_pairs = the cells with a passing end, each once

Every expected value below comes from a Python model written from these five steps (neighbours_model: fractions.Fraction and
Python integers, no float anywhere); the collection tests feed it the ORACLE's key sets.  Integers and bytes, no tolerance."""
import ctypes
import gzip
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import supersampler_amd as sp
from oracle import oracle_py as orc
from supersampler_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
KM = ((31, 11), (21, 9), (63, 15))
S = 100.0
JAC, CON, INC = 0, 1, 2
HEADER = "sketch,rank,neighbour,shared,keys,neighbour_keys,score,passing\n"
NMAX = 65535
U64 = np.uint64


def under(metric, c_row, c_partner, x):
    return c_row + c_partner - x if metric == JAC else min(c_row, c_partner) if metric == CON else c_row


def neighbours_model(card, cells, metric, num, den, top, n_query=None):
    """the five steps -> ([(sketch, rank, neighbour, shared)], passing per row sketch, n_pairs); cells = [(i, j, x)], i < j"""
    n = len(card)
    nq = n if n_query is None else n_query
    cand = [[] for _ in range(nq)]
    n_pairs = 0
    for i, j, x in cells:
        assert i < j < n
        if nq == n:
            ends = ((i, j), (j, i))
        elif i < nq <= j:
            ends = ((i, j),)
        else:
            continue
        hit = False
        for r, p in ends:
            u = under(metric, card[r], card[p], x)
            if x >= 1 and x * den >= num * u:
                cand[r].append((-Fraction(x, u), p, x))
                hit = True
        n_pairs += hit
    rows = []
    for r in range(nq):
        for rank, (_, p, x) in enumerate(sorted(cand[r])[:top]):
            rows.append((r, rank + 1, p, x))
    return rows, [len(c) for c in cand], n_pairs


def neighbours_model_np(card, cells, metric, num, den, top, n_query=None):
    """the same over numpy arrays, for the cell lists too long for a Python loop (held to neighbours_model by
    test_the_array_model_is_the_model); cells = packed uint64 words.  Only for x < 2^20 and u < 2^20: every product then stays
    below 2^63, and two DIFFERENT fractions with denominators below 2^20 lie more than 2^-40 apart, so the integers
    floor(x * 2^41 / u) order them exactly as the fractions do (and equal fractions give equal integers)"""
    card = np.asarray(card, dtype=np.int64)
    n = len(card)
    nq = n if n_query is None else n_query
    i, j = (cells >> U64(48)).astype(np.int64), ((cells >> U64(32)) & U64(0xffff)).astype(np.int64)
    x = (cells & U64(0xffffffff)).astype(np.int64)
    assert ((i < j) & (j < n)).all() and (x < 1 << 20).all() and (card < 1 << 19).all()
    if nq == n:
        r, p, xx, cell = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([x, x]), np.concatenate([np.arange(len(i))] * 2)
    else:
        use = (i < nq) & (j >= nq)
        r, p, xx, cell = i[use], j[use], x[use], np.nonzero(use)[0]
    u = card[r] + card[p] - xx if metric == JAC else np.minimum(card[r], card[p]) if metric == CON else card[r]
    ok = (xx >= 1) & (xx * den >= num * u)
    r, p, xx, u, cell = r[ok], p[ok], xx[ok], u[ok], cell[ok]
    key = (xx << 41) // u
    order = np.lexsort((p, -key, r))
    r, p, xx = r[order], p[order], xx[order]
    passing = np.bincount(r, minlength=nq).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(passing)])[:-1]
    rank = np.arange(len(r)) - first[r]
    keep = rank < top
    rows = np.zeros(int(keep.sum()), dtype=sp.NEIGHBOUR_ROW_DTYPE)
    rows["sketch"], rows["rank"], rows["neighbour"], rows["shared"] = r[keep], rank[keep] + 1, p[keep], xx[keep]
    return rows, passing, len(np.unique(cell))


def pack(cells):
    return np.array([(i << 48) | (j << 32) | x for i, j, x in cells], dtype=np.uint64)


def as_tuples(rows):
    assert not np.any(rows["reserved"])
    return [tuple(int(r[f]) for f in ("sketch", "rank", "neighbour", "shared")) for r in rows]


def as_rows(tuples):
    rows = np.zeros(len(tuples), dtype=sp.NEIGHBOUR_ROW_DTYPE)
    for t, (s, rank, p, x) in enumerate(tuples):
        rows[t] = (s, rank, p, 0, x)
    return rows


def py_csv(tuples, passing, names, card, metric, precision=6):
    text = HEADER
    for s, rank, p, x in tuples:
        score = x / under(metric, card[s], card[p], x)
        text += "%s,%d,%s,%d,%d,%d,%s,%d\n" % (names[s], rank, names[p], x, card[s], card[p], "%.*g" % (precision, score), passing[s])
    return text.encode()


# ------------------------------------------------------------------------------------------ the collections

_cache = {}


def cached(f):
    def g(*a):
        if (f.__name__, a) not in _cache:
            _cache[(f.__name__, a)] = f(*a)
        return _cache[(f.__name__, a)]
    return g


def _genomes():
    """48 genomes in 8 families (blocks of six at mu = 0, 0.01, 0.03, 0, 0.01, 0.03) + 12 unrelated ones, 60 kbp each"""
    fam = synth.family_genomes(5, 48, 60_000, 8, [0.0, 0.01, 0.03])
    rng = np.random.default_rng(6)
    return fam + [synth.random_genome(rng, 60_000) for _ in range(12)]


@cached
def collection(k, m, s):
    """the 60 sketches as the oracle makes them at -s s"""
    return [orc.sketch_fasta(synth.to_fasta(g, "g%d" % i), k, m, s)[0] for i, g in enumerate(_genomes())]


def key_set(payload):
    _, _, mn, lo, hi = orc.sketch_keys(payload)
    return set(zip(mn.tolist(), hi.tolist(), lo.tolist()))


@cached
def collection_cells(k, m, s):
    """-> (card, cells) from the oracle's key sets"""
    sets = [key_set(p) for p in collection(k, m, s)]
    cells = [(i, j, len(sets[i] & sets[j])) for i in range(len(sets)) for j in range(i + 1, len(sets)) if sets[i] & sets[j]]
    return [len(x) for x in sets], cells


# what the collection is asked: (metric, num, den, top, n_query).  The first SIX are one whole family: as queries they have no
# relative among the references; the first FOUR leave two of their family in the bank
QUESTIONS = ((JAC, 0, 1, 5, None), (JAC, 1, 2, 64, None), (CON, 3, 5, 3, None), (INC, 1, 4, 4, None), (JAC, 0, 1, 3, 6), (INC, 1, 2, 64, 6), (CON, 1, 10, 2, 6),
             (JAC, 0, 1, 1, 4), (INC, 1, 2, 64, 4), (CON, 1, 10, 2, 4))
NQ = 4


# ------------------------------------------------------------------------------------------------ not GPU

def test_model_on_hand_made_cases():
    # equality at the threshold passes, one key fewer does not: Jaccard 1/3 of two sketches of 100 keys is 50 shared
    for metric, num, den in ((JAC, 1, 3), (CON, 1, 2), (INC, 1, 2)):
        assert neighbours_model([100, 100], [(0, 1, 50)], metric, num, den, 4) == ([(0, 1, 1, 50), (1, 1, 0, 50)], [1, 1], 1)
        assert neighbours_model([100, 100], [(0, 1, 49)], metric, num, den, 4) == ([], [0, 0], 0)
    # metric 2 gives the two ends of one cell different scores: 30 of 40 passes 3/4 for the small sketch, 30 of 1000 does not
    assert neighbours_model([1000, 40], [(0, 1, 30)], INC, 3, 4, 4) == ([(1, 1, 0, 30)], [0, 1], 1)
    assert neighbours_model([1000, 40], [(0, 1, 30)], CON, 3, 4, 4) == ([(0, 1, 1, 30), (1, 1, 0, 30)], [1, 1], 1)
    # ... and orders one row's partners differently from the symmetric metrics: for row 0, 60 / 100 beats 50 / 100 whatever the
    # partners hold, while the larger containment prefers the partner it fills (50 / 50)
    card, cells = [100, 400, 50], [(0, 1, 60), (0, 2, 50)]
    assert neighbours_model(card, cells, INC, 0, 1, 4)[0][:2] == [(0, 1, 1, 60), (0, 2, 2, 50)]
    assert neighbours_model(card, cells, CON, 0, 1, 4)[0][:2] == [(0, 1, 2, 50), (0, 2, 1, 60)]
    # the tie rule: equal fractions (1/2 and 2/4 and 3/6), the partner listed first comes first
    card, cells = [1000, 6, 2, 4], [(0, 1, 3), (0, 2, 1), (0, 3, 2)]
    assert neighbours_model(card, cells, CON, 0, 1, 4, 1) == ([(0, 1, 1, 3), (0, 2, 2, 1), (0, 3, 3, 2)], [3], 3)
    # top cuts the list, and passing says so
    assert neighbours_model(card, cells, CON, 0, 1, 2, 1) == ([(0, 1, 1, 3), (0, 2, 2, 1)], [3], 3)
    # query mode ignores query-query cells (and reference-reference ones); all versus all uses the same cells for both ends
    card, cells = [100, 100, 100, 100], [(0, 1, 90), (0, 2, 10), (1, 3, 20), (2, 3, 99)]
    assert neighbours_model(card, cells, JAC, 0, 1, 4, 2) == ([(0, 1, 2, 10), (1, 1, 3, 20)], [1, 1], 2)
    assert neighbours_model(card, cells, JAC, 0, 1, 1)[0] == [(0, 1, 1, 90), (1, 1, 0, 90), (2, 1, 3, 99), (3, 1, 2, 99)]
    # num == 0 passes any shared key, a cell of count 0 never passes
    assert neighbours_model([5, 5], [(0, 1, 0)], JAC, 0, 1, 4) == ([], [0, 0], 0)
    assert neighbours_model([5, 5], [(0, 1, 1)], JAC, 0, 1000000, 4)[1:] == ([1, 1], 1)


def random_small(rng, n, n_cells):
    card = rng.integers(50, 100, n)
    pairs = sorted({(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(0, n, (n_cells, 2)) if a != b})
    return card, [(i, j, int(rng.integers(0, min(card[i], card[j]) + 1))) for i, j in pairs]


def test_the_array_model_is_the_model():
    rng = np.random.default_rng(3)
    for trial in range(30):
        n = int(rng.integers(2, 40))
        card, cells = random_small(rng, n, int(rng.integers(0, 6 * n)))
        card[rng.integers(0, n, 5)] = 64                                     # (equal fractions with different x among them)
        cells = [(i, j, min(x, int(min(card[i], card[j])))) for i, j, x in cells]
        for metric, num, den, top, nq in ((JAC, 1, 3, 3, None), (CON, 1, 2, 64, None), (INC, 0, 1, 2, None), (INC, 1, 2, 3, max(1, n // 3)), (JAC, 1, 5, 1, 1)):
            rows, passing, pairs = neighbours_model(card.tolist(), cells, metric, num, den, top, nq)
            got, g_pass, g_pairs = neighbours_model_np(card, pack(cells) if cells else np.zeros(0, np.uint64), metric, num, den, top, nq)
            assert (as_tuples(got), g_pass.tolist(), g_pairs) == (rows, passing, pairs), (trial, metric, nq)


def test_neighbours_csv_equals_the_python_writer():
    names = ["a one.fa.gz", "dir/b.two", "c 3.sk.gz", "d.1.2.sketch", "e"]
    card = [1000, 700, 333, 12345, 3]
    rows = [(0, 1, 3, 300), (0, 2, 1, 70), (1, 1, 0, 70), (3, 1, 0, 300), (4, 1, 3, 3)]
    passing = [7, 1, 0, 1, 1]
    for metric in (JAC, CON, INC):
        for precision in (6, 3):
            assert sp.neighbours_csv(as_rows(rows), passing, names, card, metric, None, precision) == py_csv(rows, passing, names, card, metric, precision)
    text = sp.neighbours_csv(as_rows(rows), passing, names, card, JAC).decode().splitlines()
    assert text[0] + "\n" == HEADER and len(text) == 6
    assert text[1] == "a one.fa.gz,1,d.1.2.sketch,300,1000,12345,0.0229973,7" and text[5] == "e,1,d.1.2.sketch,3,3,12345,0.000243013,1"
    assert sp.neighbours_csv(as_rows(rows), passing, names, card, INC, None, 3).decode().splitlines()[1].endswith(",300,1000,12345,0.3,7")
    # query mode: two queries, three references
    q_rows, q_pass = [(0, 1, 3, 300), (0, 2, 2, 70), (1, 1, 4, 2)], [2, 1]
    assert sp.neighbours_csv(as_rows(q_rows), q_pass, names, card, CON, 2) == py_csv(q_rows, q_pass, names, card, CON)
    assert sp.neighbours_csv(as_rows([]), q_pass, names, card, CON, 2) == HEADER.encode()
    # a sketch beyond the list, a neighbour beyond it, the sketch as its own neighbour, an unknown metric
    for bad, nq, metric in (((5, 1, 0, 3), None, JAC), ((0, 1, 5, 3), None, JAC), ((2, 1, 2, 3), None, JAC), ((0, 1, 1, 3), None, 3),
                            ((2, 1, 3, 3), 2, JAC), ((0, 1, 1, 3), 2, JAC)):   # ... a reference as the row, a query as the neighbour
        with pytest.raises(sp.SpspError) as e:
            sp.neighbours_csv(as_rows([bad]), passing if nq is None else q_pass, names, card, metric, nq)
        assert e.value.code == sp.ERR_ARG, bad


def test_abi_has_the_neighbour_calls():
    calls = ("spsp_neighbours_cells_device", "spsp_neighbours_csv_host", "spsp_neighbours_files")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    assert ctypes.sizeof(sp.NeighbourRow) == 24 == sp.NEIGHBOUR_ROW_DTYPE.itemsize
    for name in calls:
        assert hasattr(sp.lib(), name)


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-N", "5", "-J", "0.5", "-K", "0.5"), ("-N", "5", "-J", "0.5", "-J", "0.6"), ("-N", "5", "-K", "0.5", "-I", "0.5"),
             ("-J", "0.5"), ("-K", "0.5"), ("-I", "0"), ("-I", "0.5", "-q", "list.txt"),
             ("-N", "5", "-g", "3", "-q", "list.txt"), ("-N", "5", "-c", "0.5"), ("-N", "5", "-C", "0.5"),
             ("-N", "0"), ("-N", "65"), ("-N", "-1"), ("-N", "abc"), ("-N", ""), ("-N", "5x")]
    cases += [("-N", "5", "-J", t) for t in ("1.5", "0.1234567", "abc", "", "0.", ".5", "-0.5", "1e-1", "2")]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1, (args, r.stdout, r.stderr)
        assert any(f in r.stdout for f in ("-N", "-J", "-K", "-I")), (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
    # -c / -C still refuse 0
    r = run("-c", "0", "-f", "list.txt", "-o", "bad")
    assert r.returncode == 1 and "-c" in r.stdout


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def upload(words):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(words).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def gpu_nb(ctx, cells, card, metric, num, den, top, nq=None):
    """cells: packed uint64 words on the host -> (rows, passing, n_pairs) of the device's answer"""
    d = upload(cells) if len(cells) else None
    return ctx.neighbours_cells_device(d.data_ptr() if d is not None else None, len(cells), card, len(card), metric, num, den, top, nq)


def in_three_orders(ctx, cells, card, metric, num, den, top, nq, want):
    """as built, reversed and shuffled: the same rows and counts every time; want = (rows as an array or as tuples, passing, n_pairs)"""
    cells = np.asarray(cells, dtype=np.uint64)
    rng = np.random.default_rng(len(cells))
    w_rows, w_pass, w_pairs = want
    for order in (cells, cells[::-1], rng.permutation(cells)):
        rows, passing, pairs = gpu_nb(ctx, order, card, metric, num, den, top, nq)
        assert pairs == w_pairs and passing.tolist() == list(w_pass)
        if isinstance(w_rows, np.ndarray):
            assert np.array_equal(rows, w_rows)
        else:
            assert as_tuples(rows) == w_rows


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells", [0, 1, 2047, 2048, 2049])
def test_tile_seams(ctx, n_cells):
    rng = np.random.default_rng(50)
    n = 70                                                                  # 2 415 pairs
    card = rng.integers(200, 300, n).tolist()
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pairs = [pairs[t] for t in rng.permutation(len(pairs))[:n_cells]]
    cells = [(i, j, int(rng.integers(0, min(card[i], card[j]) + 1))) for i, j in pairs]
    for metric, num, den, top, nq in ((JAC, 1, 4, 5, None), (INC, 1, 3, 64, None), (CON, 1, 2, 3, 20)):
        want = neighbours_model(card, cells, metric, num, den, top, nq)
        assert n_cells < 2047 or (len(want[0]) > 50 and want[2] < n_cells)
        in_three_orders(ctx, pack(cells) if cells else np.zeros(0, np.uint64), card, metric, num, den, top, nq, want)


@pytest.mark.gpu
@pytest.mark.parametrize("degree", [1, 63, 64, 65, 127, 128, 129])
def test_chunk_seams_of_the_selection(ctx, degree):
    """row 0 with exactly `degree` passing partners (and some that do not pass) at top = 1, 63, 64; the best partner is the last
    one listed at 65 (and at 128), the first one at 129 (and at 64)"""
    rng = np.random.default_rng(degree)
    n = degree + 6
    card = [1000] * n
    x = rng.permutation(np.arange(300, 300 + degree)).tolist()              # distinct scores
    if degree in (65, 128):
        x[x.index(max(x))], x[-1] = x[-1], max(x)
    if degree in (129, 64):
        x[x.index(max(x))], x[0] = x[0], max(x)
    cells = [(0, 1 + t, x[t]) for t in range(degree)] + [(0, degree + 1 + t, 10 + t) for t in range(5)]
    for top in (1, 63, 64):
        want = neighbours_model(card, cells, JAC, 1, 10, top)                # (300 of 1700 and more pass 1/10; 14 of 1986 do not)
        assert want[1][0] == degree and (degree not in (65, 128) or want[0][0][2] == degree) and (degree not in (129, 64) or want[0][0][2] == 1)
        assert [r for r in want[0] if r[0] == 0][-1][1] == min(top, degree)  # top above the degree returns the degree
        in_three_orders(ctx, pack(cells), card, JAC, 1, 10, top, None, want)
        q = neighbours_model(card, cells, JAC, 1, 10, top, 1)
        assert len(q[0]) == min(top, degree) and q[1] == [degree] and q[2] == degree
        in_three_orders(ctx, pack(cells), card, JAC, 1, 10, top, 1, q)


@pytest.mark.gpu
def test_ties(ctx):
    # 200 partners of one score: the 64 smallest indices in order
    n = 300
    card = [500] * n
    partners = np.random.default_rng(51).permutation(np.arange(1, n))[:200].tolist()
    cells = [(0, p, 250) for p in partners]
    want = neighbours_model(card, cells, JAC, 1, 3, 64, 1)
    assert [r[2] for r in want[0]] == sorted(partners)[:64] and want[1] == [200]
    in_three_orders(ctx, pack(cells), card, JAC, 1, 3, 64, 1, want)
    in_three_orders(ctx, pack(cells), card, JAC, 1, 3, 64, None, neighbours_model(card, cells, JAC, 1, 3, 64))
    # equal fractions with different x (1/2, 2/4, 3/6, 50/100) are ties: list order decides; 2/3 comes in front of them all
    card = [1000, 100, 3, 6, 2, 4]
    cells = [(0, 1, 50), (0, 2, 2), (0, 3, 3), (0, 4, 1), (0, 5, 2)]
    want = neighbours_model(card, cells, CON, 1, 2, 64, 1)
    assert want[0] == [(0, 1, 2, 2), (0, 2, 1, 50), (0, 3, 3, 3), (0, 4, 4, 1), (0, 5, 5, 2)]
    in_three_orders(ctx, pack(cells), card, CON, 1, 2, 64, 1, want)


def test_two_fractions_that_are_one_double():
    """the precondition of the exactness test, on the CPU"""
    card, cells = exactness_case()
    (_, a, xa), (_, b, xb) = cells[1], cells[0]
    ua, ub = under(JAC, card[0], card[a], xa), under(JAC, card[0], card[b], xb)
    assert a > b and max(card) < 1 << 47 and xa <= min(card[0], card[a]) and xb <= min(card[0], card[b])
    assert xa / ua == xb / ub and float(xa) / float(ua) == float(xb) / float(ub)     # one double ...
    assert Fraction(xa, ua) > Fraction(xb, ub)                                       # ... two fractions, A the better


def exactness_case():
    c_r = 1 << 46
    xa, ca = (1 << 31) + 1, (1 << 46) + 12345
    ua = c_r + ca - xa
    xb = xa + 1
    ub = ua * xb // xa + 1
    cb = ub - c_r + xb
    return [c_r, cb, ca], [(0, 1, xb), (0, 2, xa)]                                   # A has the LARGER index


@pytest.mark.gpu
def test_exactness_where_doubles_tie(ctx):
    """a float comparison plus the tie rule would put B (index 1) first; the fractions put A (index 2) first"""
    test_two_fractions_that_are_one_double()
    card, cells = exactness_case()
    for nq in (1, None):
        want = neighbours_model(card, cells, JAC, 0, 1, 2, nq)
        assert want[0][:2] == [(0, 1, 2, cells[1][2]), (0, 2, 1, cells[0][2])]
        in_three_orders(ctx, pack(cells), card, JAC, 0, 1, 2, nq, want)
        assert neighbours_model(card, cells, JAC, 0, 1, 1, nq)[0][0][2] == 2
        in_three_orders(ctx, pack(cells), card, JAC, 0, 1, 1, nq, neighbours_model(card, cells, JAC, 0, 1, 1, nq))


@pytest.mark.gpu
def test_threshold(ctx):
    # exactly at num / den passes, one key fewer does not: Jaccard 50 / 150 = 1/3, containment 50 / 100 = 1/2, contained 50 / 100
    for metric, num, den in ((JAC, 1, 3), (CON, 1, 2), (INC, 1, 2)):
        for x, n_rows in ((50, 2), (49, 0)):
            want = neighbours_model([100, 100], [(0, 1, x)], metric, num, den, 4)
            assert len(want[0]) == n_rows
            in_three_orders(ctx, pack([(0, 1, x)]), [100, 100], metric, num, den, 4, None, want)
    # metric 2: one cell, two verdicts
    want = neighbours_model([1000, 40], [(0, 1, 30)], INC, 3, 4, 4)
    assert want == ([(1, 1, 0, 30)], [0, 1], 1)
    in_three_orders(ctx, pack([(0, 1, 30)]), [1000, 40], INC, 3, 4, 4, None, want)
    # num == 0 passes every non-zero cell, a cell of count 0 never passes; large key counts at the largest den
    big = (1 << 47) - 1
    card = [big, big, 1 << 46, 4_000_000_000, 7]
    cells = [(0, 1, 0xffffffff), (1, 2, 1 << 31), (2, 3, 1), (3, 4, 0), (0, 4, 7), (1, 4, 0)]
    for metric in (JAC, CON, INC):
        for num, den in ((0, 1), (0, 1000000), (1, 1000000), (1000000, 1000000), (999999, 1000000), (1, 2)):
            want = neighbours_model(card, cells, metric, num, den, 3)
            if num == 0:
                assert want[1] == [2, 2, 2, 1, 1] and want[2] == 4
            in_three_orders(ctx, pack(cells), card, metric, num, den, 3, None, want)


@pytest.mark.gpu
def test_a_star_whose_centre_is_the_last_of_65535(ctx):
    """one row of 65 534 candidates, every other row has one.  x_i = 1 + 40503 i mod 65534 is a permutation of 1 .. 65534
    (40503 is coprime to 65534) and all key counts are equal, so the centre's best are the i with x_i = 65534, 65533, ..."""
    c = NMAX - 1
    card = np.full(NMAX, 70_000)
    i = np.arange(c, dtype=np.int64)
    x = 1 + (i * 40503) % c
    inv = pow(40503, -1, c)
    best = [((c - 1 - t) * inv) % c for t in range(64)]
    assert [int(x[b]) for b in best] == [c - t for t in range(64)]
    cells = i.astype(U64) << U64(48) | U64(c) << U64(32) | x.astype(U64)
    rows = np.zeros(c + 64, dtype=sp.NEIGHBOUR_ROW_DTYPE)
    rows["sketch"][:c], rows["rank"][:c], rows["neighbour"][:c], rows["shared"][:c] = i, 1, c, x
    rows["sketch"][c:], rows["rank"][c:], rows["neighbour"][c:], rows["shared"][c:] = c, np.arange(1, 65), best, x[best]
    passing = np.ones(NMAX, dtype=np.uint32)
    passing[c] = c
    in_three_orders(ctx, cells, card, JAC, 0, 1, 64, None, (rows, passing, c))


@pytest.mark.gpu
@pytest.mark.parametrize("metric,num,den", [(JAC, 1, 3), (CON, 1, 2), (INC, 2, 5)])
def test_random_cells_about_half_of_which_pass(ctx, metric, num, den):
    rng = np.random.default_rng(52 + metric)
    n = 3000
    card = rng.integers(500, 1000, n)
    pairs = rng.integers(0, n, (230_000, 2))
    a, b = pairs.min(1), pairs.max(1)
    keep = np.unique(a[a != b] * 65536 + b[a != b])
    rng.shuffle(keep)
    keep = keep[:200_000]
    a, b = keep // 65536, keep % 65536
    assert len(keep) == 200_000
    x = (rng.random(len(a)) * (np.minimum(card[a], card[b]) + 1)).astype(np.uint64)
    cells = a.astype(U64) << U64(48) | b.astype(U64) << U64(32) | x
    for nq, top in ((None, 64), (None, 7), (100, 16)):
        want = neighbours_model_np(card, cells, metric, num, den, top, nq)
        n_ends = (2 * len(cells)) if nq is None else int(((a < 100) & (b >= 100)).sum())
        assert 0.3 * n_ends < want[1].sum() < 0.7 * n_ends and want[1].max() > top and len(want[0]) < want[1].sum()
        in_three_orders(ctx, cells, card, metric, num, den, top, nq, want)


def raw_call(ctx, d_cells, n_cells, card, n, nq, metric, num, den, top, rows, cap):
    card = np.ascontiguousarray(card, dtype=np.uint64)
    passing = np.full(max(min(n, nq), 1), 77, dtype=np.uint32)
    cnt, pairs = ctypes.c_uint64(99), ctypes.c_uint64(99)
    rc = sp.lib().spsp_neighbours_cells_device(ctx._h, d_cells, n_cells, card.ctypes.data, n, nq, metric, num, den, top,
                                               rows.ctypes.data if rows is not None else None, cap, ctypes.byref(cnt), passing.ctypes.data, ctypes.byref(pairs))
    return rc, cnt.value, pairs.value, passing


@pytest.mark.gpu
def test_bad_cells_and_bad_arguments_are_refused(ctx):
    card = [100] * 10
    good = [(0, 1, 80), (2, 3, 80), (0, 2, 70)]
    w_good = neighbours_model(card, good, JAC, 1, 2, 4)
    for bad in ((3, 10, 80), (4, 4, 80), (7, 2, 80), (65535, 65535, 1)):
        with pytest.raises(sp.SpspError) as e:
            gpu_nb(ctx, pack(good + [bad] + good), card, JAC, 1, 2, 4)
        assert e.value.code == sp.ERR_ARG and "cell" in str(e.value)
        rows = np.full(16, 7, dtype=sp.NEIGHBOUR_ROW_DTYPE)                   # the rows are zeroed
        d = upload(pack(good + [bad]))
        rc, _, _, passing = raw_call(ctx, d.data_ptr(), 4, card, 10, 10, JAC, 1, 2, 4, rows, 16)
        assert rc == sp.ERR_ARG and not rows.view(np.uint8).any() and not passing.any()
        in_three_orders(ctx, pack(good), card, JAC, 1, 2, 4, None, w_good)   # ... and the context answers afterwards
    cells = upload(pack(good))
    call = lambda n=10, nq=None, metric=JAC, num=1, den=2, top=4, c=card: ctx.neighbours_cells_device(
        cells.data_ptr(), 3, c[:n] if n <= len(c) else c + [1] * (n - len(c)), n, metric, num, den, top, nq)
    for kw in (dict(n=0), dict(n=65536), dict(nq=0), dict(nq=11), dict(metric=3), dict(metric=-1), dict(num=3), dict(num=1000001, den=1000001),
               dict(den=1000001), dict(top=0), dict(top=65), dict(c=[100] * 9 + [1 << 47])):
        with pytest.raises(sp.SpspError) as e:
            call(**kw)
        assert e.value.code == sp.ERR_ARG, kw
    rows, passing, pairs = call()
    assert (as_tuples(rows), passing.tolist(), pairs) == w_good
    rows, passing, pairs = call(num=0, den=1, top=64, metric=INC, nq=10)
    assert (as_tuples(rows), passing.tolist(), pairs) == neighbours_model(card, good, INC, 0, 1, 64)
    # room one short of the need: ERR_OVERFLOW with the exact count, rows untouched; then the call with that room succeeds
    need = len(w_good[0])
    rows = np.full(need, 7, dtype=sp.NEIGHBOUR_ROW_DTYPE)
    before = rows.copy()
    rc, cnt, pairs, passing = raw_call(ctx, cells.data_ptr(), 3, card, 10, 10, JAC, 1, 2, 4, rows, need - 1)
    assert rc == sp.ERR_OVERFLOW and cnt == need and np.array_equal(rows, before)
    rc, cnt, pairs, passing = raw_call(ctx, cells.data_ptr(), 3, card, 10, 10, JAC, 1, 2, 4, rows, need)
    assert rc == 0 and cnt == need and (as_tuples(rows), passing.tolist(), pairs) == w_good
    rc, cnt, pairs, passing = raw_call(ctx, None, 0, card, 10, 10, JAC, 1, 2, 4, None, 0)      # no cells, no room: no rows
    assert (rc, cnt, pairs) == (0, 0, 0) and not passing.any()


def gpu_collection_cells(ctx, payloads):
    """decode, the all-vs-all as cells -> (device cells (kept alive by the caller), count, card)"""
    import torch
    n = len(payloads)
    k, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
    scratch = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    cells = torch.zeros(n * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cnt = ctx.compare_cells_device(k, d_mn, d_lo, d_hi, off, n, scratch.data_ptr(), cells.data_ptr(), cells.numel())
    return cells, cnt, np.diff(off.astype(np.int64)).tolist()


@pytest.mark.gpu
def test_twice_on_one_context(ctx):
    """a larger problem, then a smaller one, then the larger again: the reused work buffers leave nothing behind"""
    rng = np.random.default_rng(53)
    n = 5000
    card = rng.integers(100, 200, n)
    keep = np.unique(np.sort(rng.integers(0, n, (60_000, 2)), axis=1), axis=0)
    keep = keep[keep[:, 0] != keep[:, 1]]
    x = (rng.random(len(keep)) * np.minimum(card[keep[:, 0]], card[keep[:, 1]])).astype(np.uint64) + U64(1)
    cells = keep[:, 0].astype(U64) << U64(48) | keep[:, 1].astype(U64) << U64(32) | x
    want = neighbours_model_np(card, cells, JAC, 1, 4, 10)
    in_three_orders(ctx, cells, card, JAC, 1, 4, 10, None, want)
    small = [(0, 1, 50), (1, 2, 60), (0, 2, 70)]
    in_three_orders(ctx, pack(small), [100, 100, 100], CON, 1, 2, 1, None, neighbours_model([100, 100, 100], small, CON, 1, 2, 1))
    rows, passing, pairs = gpu_nb(ctx, np.zeros(0, np.uint64), [5] * 70, JAC, 0, 1, 64)
    assert len(rows) == 0 and not passing.any() and pairs == 0
    in_three_orders(ctx, cells, card, JAC, 1, 4, 10, None, want)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", KM)
def test_the_family_collection_from_sketches_to_neighbours(ctx, k, m):
    pl = collection(k, m, S)
    w_card, w_cells = collection_cells(k, m, S)
    d_cells, cnt, card = gpu_collection_cells(ctx, pl)
    assert card == w_card and cnt == len(w_cells)
    for metric, num, den, top, nq in QUESTIONS:
        want = neighbours_model(w_card, w_cells, metric, num, den, top, nq)
        rows, passing, pairs = ctx.neighbours_cells_device(d_cells.data_ptr(), cnt, card, len(pl), metric, num, den, top, nq)
        assert (as_tuples(rows), passing.tolist(), pairs) == want, (metric, num, den, top, nq)
        assert nq != NQ or len(want[0]) >= 2
    # what the collection is there for: a family's members find each other, an unrelated genome finds nobody at 1/2
    rows, passing, _ = neighbours_model(w_card, w_cells, JAC, 1, 2, 64)
    assert passing[0] >= 1 and passing[59] == 0 and any(p > 1 for p in passing) and rows[0][:3] == (0, 1, 3)


def write_files(root, payloads, tag="f"):
    paths = []
    for i, p in enumerate(payloads):
        paths.append(os.path.join(str(root), "%s %03d.sk.gz" % (tag, i)))  # (names with a space and dots)
        sp.write_gz(paths[-1], p, 1)
    return paths


def gunzip(path):
    return gzip.open(path, "rb").read()


@pytest.mark.gpu
def test_neighbours_files_and_the_command_line(ctx, tmp_path):
    k, m = 31, 11
    pl = collection(k, m, S)
    card, cells = collection_cells(k, m, S)
    paths = write_files(tmp_path, pl)
    nq = NQ
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    (tmp_path / "queries.txt").write_text("\n".join(paths[:nq]) + "\n")
    (tmp_path / "bank.txt").write_text("\n".join(paths[nq:]) + "\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    kmers = "kmers evaluated are of length: %d minimizer size is %d" % (k, m)
    for (metric, num, den, top), flags in (((JAC, 0, 1, 5), ()), ((JAC, 1, 2, 64), ("-J", "0.5")), ((CON, 3, 5, 3), ("-K", "0.60")), ((INC, 1, 4, 4), ("-I", "0.25"))):
        for q in (None, nq):
            want, passing, pairs = neighbours_model(card, cells, metric, num, den, top, q)
            text = py_csv(want, passing, paths, card, metric)
            rows = ctx.neighbours_files(paths, str(tmp_path / "lib"), top, metric, num, den, q)
            assert as_tuples(rows) == want and gunzip(str(tmp_path / "lib_neighbours.csv.gz")) == text
            r = run("-N", str(top), *flags, *(("-f", "list.txt") if q is None else ("-q", "queries.txt", "-f", "bank.txt")), "-o", "cli")
            assert r.returncode == 0, r.stdout + r.stderr
            assert gunzip(str(tmp_path / "cli_neighbours.csv.gz")) == text
            out = r.stdout.splitlines()
            head = ["No query file, I will perform a all versus all comparison", "I found %d documents" % len(pl)] if q is None else ["I query %d file(s) against the bank" % nq]
            assert out == head + [kmers, "%d sketches, %d passing pairs, %d rows written" % (len(pl), pairs, len(want))]
            os.remove(str(tmp_path / "cli_neighbours.csv.gz"))
    want, passing, _ = neighbours_model(card, cells, JAC, 1, 2, 64)
    ctx.neighbours_files(paths, str(tmp_path / "p3"), 64, JAC, 1, 2, precision=3)
    assert gunzip(str(tmp_path / "p3_neighbours.csv.gz")) == py_csv(want, passing, paths, card, JAC, 3)
    assert not [f for f in os.listdir(tmp_path) if "_jaccard" in f or "_containment" in f or "_gather" in f or "_clusters" in f]
    # without -N: the two matrices, as before
    r = run("-f", "list.txt", "-o", "plain")
    assert r.returncode == 0, r.stdout + r.stderr
    inter, c2, _, _ = orc.compare(pl)
    for jac, suf in ((True, "_jaccard.csv.gz"), (False, "_containment.csv.gz")):
        assert gunzip(str(tmp_path / ("plain" + suf))) == orc.csv(jac, paths, inter, c2, None, 6, 0.0)
    assert not os.path.exists(str(tmp_path / "plain_neighbours.csv.gz"))
    # bad arguments of the file call, and a k == m collection
    for kw in (dict(metric=3), dict(num=3, den=2), dict(den=1000001), dict(top=0), dict(top=65), dict(n_query=0), dict(n_query=61)):
        with pytest.raises(sp.SpspError) as e:
            ctx.neighbours_files(paths, str(tmp_path / "no"), **dict(dict(top=5), **kw))
        assert e.value.code == sp.ERR_ARG, kw
    kk = [orc.sketch_fasta(synth.to_fasta(g[:5000], "g%d" % i), 11, 11, S)[0] for i, g in enumerate(_genomes()[:3])]
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.neighbours_files(write_files(tmp_path, kk, "kk"), str(tmp_path / "no"), 5, rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no")]


@pytest.mark.gpu
def test_neighbours_files_at_a_common_rate(ctx, tmp_path):
    """some files at -s 100, the others at -s 1000, rate="auto": the neighbours of the -s 1000 sketches of the same genomes"""
    k, m = 31, 11
    coarse, fine = collection(k, m, 1000.0), collection(k, m, S)
    card, cells = collection_cells(k, m, 1000.0)
    mixed = [fine[i] if i % 3 == 1 else coarse[i] for i in range(len(coarse))]
    paths = write_files(tmp_path, mixed)
    (tmp_path / "queries.txt").write_text("\n".join(paths[:NQ]) + "\n")
    (tmp_path / "bank.txt").write_text("\n".join(paths[NQ:]) + "\n")
    for q in (None, NQ):
        want, passing, pairs = neighbours_model(card, cells, JAC, 1, 10, 8, q)
        assert len(want) > (10 if q is None else 3)
        for tag, rate in (("auto", "auto"), ("r1000", 1000)):
            rows = ctx.neighbours_files(paths, str(tmp_path / tag), 8, JAC, 1, 10, q, rate=rate)
            assert as_tuples(rows) == want
            assert gunzip(str(tmp_path / (tag + "_neighbours.csv.gz"))) == py_csv(want, passing, paths, card, JAC)
    # as the files are: another question with another answer
    assert as_tuples(ctx.neighbours_files(paths, str(tmp_path / "asis"), 8, JAC, 1, 10, NQ)) != want
    # the command line with -s auto, and its common-rate line
    r = subprocess.run([EXE, "-N", "8", "-J", "0.1", "-s", "auto", "-q", "queries.txt", "-f", "bank.txt", "-o", "cli"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert gunzip(str(tmp_path / "cli_neighbours.csv.gz")) == py_csv(want, passing, paths, card, JAC)
    assert r.stdout.splitlines()[2:] == ["60 sketches, %d passing pairs, %d rows written" % (pairs, len(want)),
                                          "Sketches compared at sampling rate 1000: 20 of 60 brought down to it"]
    # a file coarser than the asked rate: refused, naming it
    with pytest.raises(sp.SpspError) as e:
        ctx.neighbours_files(paths, str(tmp_path / "no"), 8, JAC, 1, 10, rate=100)
    assert e.value.code == sp.ERR_ARG and os.path.basename(paths[0]) in str(e.value)
