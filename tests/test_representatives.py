"""Representatives: greedy dereplication of a collection (include/spsp.h: spsp_representatives_cells_device,
spsp_representatives_files; bin/comparator -r / -R / -w).

The rule, on sets of the comparator's keys.  Sketches are 0 .. n-1 in list order, c_i = |K_i|, x_ij = |K_i & K_j|, the threshold is
the fraction num / den, w_i an optional weight (without: w_i = c_i):

    1. i < j are linked iff x_ij >= 1 and  x_ij * den >= num * (c_i + c_j - x_ij)   (metric 0, Jaccard)
                                       or  x_ij * den >= num * min(c_i, c_j)        (metric 1, the larger containment)
    2. a comes before b iff w_a > w_b, or w_a == w_b and a < b
    3. going through the sketches in that order, a sketch is a representative iff it is linked to no representative before it
    4. every other sketch goes to the best of the representatives it is linked to: p beats q iff x_p * u_q > x_q * u_p, u the
       metric's denominator for the pair; equal fractions: the representative that comes first in the order of 2
    5. row i = (cluster, representative, size, shared): clusters numbered by their first-listed member, shared = x_{i,rep}, or
       c_i for the representative itself

Every expected value below comes from a Python model written from these five steps (reps_model: plain loops, Python integers)
or its numpy form for the long lists (reps_model_np), held to each other on random small graphs: integers and bytes, no
tolerance anywhere.

What the rule promises, asserted independently of the model (check_consequences): no two representatives are linked; every
member is linked to its representative; no linked representative beats the assigned one; every member is linked to a
representative that comes BEFORE it in the order of 2; n_clusters = the representatives; a sketch without an edge is a cluster
of one.  The representative a member is FILED UNDER need not come before it: step 4 takes the best of ALL the representatives
it is linked to, and test_the_best_representative_may_come_later holds the three-sketch example."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
from oracle import oracle_py as orc
from supersampler_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
KM = ((31, 11), (21, 9), (63, 15))
S = 100.0
JAC, CON = 0, 1
FRACTIONS = ((JAC, 1, 2), (CON, 3, 5))
HEADER = "sketch,cluster,representative,size,keys,shared,score\n"
NMAX = 65535


def under(card, i, j, x, metric):
    return card[i] + card[j] - x if metric == JAC else min(card[i], card[j])


def is_link(card, i, j, x, metric, num, den):
    return x >= 1 and x * den >= num * under(card, i, j, x, metric)


def reps_model(card, cells, metric, num, den, weight=None):
    """the five steps -> ([(cluster, representative, size, shared)] per sketch, n_clusters, n_edges); cells = [(i, j, x)], i < j"""
    n = len(card)
    w = list(card) if weight is None else list(weight)
    adj = [dict() for _ in range(n)]
    edges = 0
    for i, j, x in cells:
        assert i < j < n
        if is_link(card, i, j, x, metric, num, den):
            edges += 1
            adj[i][j] = x
            adj[j][i] = x
    order = sorted(range(n), key=lambda i: (-w[i], i))
    place = {s: t for t, s in enumerate(order)}
    rep = [False] * n
    for s in order:
        rep[s] = not any(rep[t] for t in adj[s])                            # (only sketches in front of s can be representatives yet)
    of = list(range(n))
    for s in range(n):
        if rep[s]:
            continue
        best = None
        for p in sorted(adj[s]):
            if not rep[p]:
                continue
            if best is not None:
                lhs, rhs = adj[s][p] * under(card, s, best, adj[s][best], metric), adj[s][best] * under(card, s, p, adj[s][p], metric)
                if lhs < rhs or (lhs == rhs and place[p] > place[best]):
                    continue
            best = p
        assert best is not None and any(rep[p] and place[p] < place[s] for p in adj[s])
        of[s] = best
    first, size = {}, {}
    for s in range(n):
        first.setdefault(of[s], s)
        size[of[s]] = size.get(of[s], 0) + 1
    number = {r: c for c, r in enumerate(sorted(first, key=lambda r: first[r]))}
    rows = [(number[of[s]], of[s], size[of[s]], card[s] if of[s] == s else adj[s][of[s]]) for s in range(n)]
    return rows, len(first), edges


def reps_model_np(card, cells, metric, num, den, weight=None):
    """the same over numpy arrays, for the cell lists too long for a Python loop (held to reps_model by
    test_the_array_model_is_the_model); cells = packed uint64 words; every product stays below 2^63.  The representatives come
    from the rule's parallel form: rounds of "a representative puts its later neighbours out, an undecided sketch blocks them,
    undecided and not blocked becomes a representative" -> also the rounds that form takes when every state is read fresh"""
    card = np.asarray(card, dtype=np.int64)
    n = len(card)
    w = card if weight is None else np.asarray(weight, dtype=np.int64)
    prio = w * 65536 + (65535 - np.arange(n, dtype=np.int64))
    i, j = (cells >> np.uint64(48)).astype(np.int64), ((cells >> np.uint64(32)) & np.uint64(0xffff)).astype(np.int64)
    x = (cells & np.uint64(0xffffffff)).astype(np.int64)
    u = card[i] + card[j] - x if metric == JAC else np.minimum(card[i], card[j])
    assert len(x) == 0 or (float(x.max()) * den < 2.0 ** 62 and float(u.max()) * max(num, float(x.max())) < 2.0 ** 62)
    edge = (x >= 1) & (x * den >= num * u)
    i, j, x, u = i[edge], j[edge], x[edge], u[edge]
    a, b = np.where(prio[i] > prio[j], i, j), np.where(prio[i] > prio[j], j, i)
    state = np.zeros(n, dtype=np.int64)                                      # 0 undecided, 1 representative, 2 out
    rounds = 0
    while (state == 0).any():
        rounds += 1
        state[b[(state[a] == 1) & (state[b] == 0)]] = 2
        blocked = np.zeros(n, dtype=bool)
        blocked[b[(state[a] == 0) & (state[b] == 0)]] = True
        state[(state == 0) & ~blocked] = 1
    # candidates: (member, representative) over the links with one end of each kind
    mi, mj = (state[i] == 1) & (state[j] == 2), (state[j] == 1) & (state[i] == 2)
    mem, rp = np.concatenate([j[mi], i[mj]]), np.concatenate([i[mi], j[mj]])
    cx, cu = np.concatenate([x[mi], x[mj]]), np.concatenate([u[mi], u[mj]])
    hold = np.full(n, -1, dtype=np.int64)                                    # the candidate a member holds
    hold[mem] = np.arange(len(mem))
    while True:
        h = hold[mem]
        lhs, rhs = cx * cu[h], cx[h] * cu
        better = (lhs > rhs) | ((lhs == rhs) & (prio[rp] > prio[rp[h]]))
        if not better.any():
            break
        hold[mem[better]] = np.nonzero(better)[0]
    of = np.arange(n, dtype=np.int64)
    out = state == 2
    assert (hold[out] >= 0).all()
    of[out] = rp[hold[out]]
    shared = card.copy()
    shared[out] = cx[hold[out]]
    size = np.bincount(of, minlength=n)
    first = np.full(n, n, dtype=np.int64)
    np.minimum.at(first, of, np.arange(n))
    is_first = np.zeros(n, dtype=np.int64)
    is_first[first[first < n]] = 1
    number = np.cumsum(is_first) - is_first
    rows = np.zeros(n, dtype=sp.CLUSTER_ROW_DTYPE)
    rows["cluster"], rows["representative"], rows["size"], rows["shared"] = number[first[of]], of, size[of], shared
    return rows, int((state == 1).sum()), int(edge.sum()), rounds


def check_consequences(rows, n_clusters, card, cells, metric, num, den, weight=None):
    """what the rule promises, from the rows and the cells alone; rows = tuples, cells = [(i, j, x)]"""
    n = len(card)
    w = card if weight is None else weight
    before = lambda p, q: (w[p], -p) > (w[q], -q)
    x_of = {(i, j): x for i, j, x in cells if is_link(card, i, j, x, metric, num, den)}
    link = lambda p, q: x_of.get((min(p, q), max(p, q)))
    nbr = [[] for _ in range(n)]
    for (i, j) in x_of:
        nbr[i].append(j)
        nbr[j].append(i)
    reps = [s for s in range(n) if rows[s][1] == s]
    rep_set = set(reps)
    assert n_clusters == len(reps) == len({r[0] for r in rows})
    for s in range(n):
        c, r, size, shared = rows[s]
        assert r in rep_set and rows[r][0] == c and size == sum(1 for t in rows if t[1] == r)
        if s in rep_set:
            assert shared == card[s] and not any(p in rep_set for p in nbr[s])           # no two representatives are linked
            continue
        assert link(s, r) == shared and shared >= 1                                      # linked to its representative
        assert any(p in rep_set and before(p, s) for p in nbr[s])                        # a representative in front of it
        for p in nbr[s]:
            if p in rep_set and p != r:                                                  # no linked representative beats it
                lhs, rhs = link(s, p) * under(card, s, r, shared, metric), shared * under(card, s, p, link(s, p), metric)
                assert lhs < rhs or (lhs == rhs and before(r, p)), (s, r, p)
        assert nbr[s]
    for s in range(n):
        if not nbr[s]:
            assert rows[s][1:] == (s, 1, card[s])
    firsts = [min(s for s in range(n) if rows[s][1] == r) for r in reps]
    assert [rows[f][0] for f in sorted(firsts)] == list(range(len(reps)))                # numbered by first-listed member


def pack(cells):
    return np.array([(i << 48) | (j << 32) | x for i, j, x in cells], dtype=np.uint64)


def as_tuples(rows):
    assert not np.any(rows["reserved"])
    return [tuple(int(r[f]) for f in ("cluster", "representative", "size", "shared")) for r in rows]


def as_rows(tuples):
    rows = np.zeros(len(tuples), dtype=sp.CLUSTER_ROW_DTYPE)
    for i, (c, rep, size, shared) in enumerate(tuples):
        rows[i] = (c, rep, size, 0, shared)
    return rows


def py_csv(tuples, names, card, metric, precision=6):
    text = HEADER
    for i, (c, rep, size, shared) in enumerate(tuples):
        if rep == i:
            score = 1.0
        elif shared == 0:
            score = 0.0
        else:
            score = shared / (card[i] + card[rep] - shared) if metric == JAC else shared / min(card[i], card[rep])
        text += "%s,%d,%s,%d,%d,%d,%s\n" % (names[i], c, names[rep], size, card[i], shared, "%.*g" % (precision, score))
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
    """tests/test_cluster.py's recipe: 48 genomes in 8 families + 12 unrelated ones, 60 kbp each"""
    fam = synth.family_genomes(5, 48, 60_000, 8, [0.0, 0.01, 0.03])
    rng = np.random.default_rng(6)
    return fam + [synth.random_genome(rng, 60_000) for _ in range(12)]


@cached
def collection(k, m, s):
    return [orc.sketch_fasta(synth.to_fasta(g, "g%d" % i), k, m, s)[0] for i, g in enumerate(_genomes())]


def key_set(payload):
    _, _, mn, lo, hi = orc.sketch_keys(payload)
    return set(zip(mn.tolist(), hi.tolist(), lo.tolist()))


@cached
def collection_cells(k, m):
    """-> (card, cells) from the oracle's key sets"""
    sets = [key_set(p) for p in collection(k, m, S)]
    cells = [(i, j, len(sets[i] & sets[j])) for i in range(len(sets)) for j in range(i + 1, len(sets)) if sets[i] & sets[j]]
    return [len(s) for s in sets], cells


@cached
def collection_model(k, m, metric, num, den):
    card, cells = collection_cells(k, m)
    return reps_model(card, cells, metric, num, den) + (card, cells)


def single_linkage(card, cells, metric, num, den):
    """the connected components of the link graph: label per sketch"""
    lab = list(range(len(card)))

    def find(a):
        while lab[a] != a:
            a = lab[a]
        return a
    for i, j, x in cells:
        if is_link(card, i, j, x, metric, num, den):
            lab[find(j)] = find(i)
    return [find(s) for s in range(len(card))]


# ------------------------------------------------------------------------------------------------ not GPU

def test_model_on_hand_made_graphs():
    # a pair exactly at the threshold is linked, one key fewer is not: Jaccard 1/3 of two sketches of 100 keys is 50 shared
    for metric, num, den in ((JAC, 1, 3), (CON, 1, 2)):
        assert reps_model([100, 100], [(0, 1, 50)], metric, num, den) == ([(0, 0, 2, 100), (0, 0, 2, 50)], 1, 1)
        assert reps_model([100, 100], [(0, 1, 49)], metric, num, den) == ([(0, 0, 1, 100), (1, 1, 1, 100)], 2, 0)
    # a chain a-b-c with a and c unlinked and b last in the order: two representatives where single linkage makes one cluster
    card, cells = [100, 80, 90], [(0, 1, 60), (1, 2, 55)]
    rows, nc, ne = reps_model(card, cells, JAC, 1, 3)
    assert (rows, nc, ne) == ([(0, 0, 2, 100), (0, 0, 2, 60), (1, 2, 1, 90)], 2, 2)
    assert len(set(single_linkage(card, cells, JAC, 1, 3))) == 1
    # ... b first in the order: one representative, both ends filed under it
    assert reps_model([80, 100, 90], cells, JAC, 1, 3) == ([(0, 1, 3, 60), (0, 1, 3, 100), (0, 1, 3, 55)], 1, 2)
    # equal fractions with different x (30/60 against 50/100 under containment): the earlier representative wins
    card, cells = [100, 60, 1000], [(0, 2, 50), (1, 2, 30)]                  # u = min(c): 50/100 and 30/60 for member 2
    rows, nc, _ = reps_model(card, cells, CON, 1, 2, weight=[5, 9, 1])       # order: 1, 0, 2
    assert nc == 2 and rows[2] == (1, 1, 2, 30)
    rows, nc, _ = reps_model(card, cells, CON, 1, 2, weight=[9, 5, 1])       # order: 0, 1, 2
    assert nc == 2 and rows[2] == (0, 0, 2, 50)
    # ... and a larger fraction beats an earlier representative
    assert reps_model(card, [(0, 2, 50), (1, 2, 31)], CON, 1, 2, weight=[9, 5, 1])[0][2] == (1, 1, 2, 31)
    # weights that overturn the key-count order
    card, cells = [100, 90], [(0, 1, 80)]
    assert reps_model(card, cells, JAC, 1, 2)[0] == [(0, 0, 2, 100), (0, 0, 2, 80)]
    assert reps_model(card, cells, JAC, 1, 2, weight=[1, 2])[0] == [(0, 1, 2, 80), (0, 1, 2, 90)]
    # equal weights: the first listed
    assert reps_model([90, 100], cells, JAC, 1, 2, weight=[7, 7])[0] == [(0, 0, 2, 90), (0, 0, 2, 80)]
    assert reps_model([100, 100, 100], [(0, 1, 90), (1, 2, 90), (0, 2, 90)], JAC, 1, 2)[0] == [(0, 0, 3, 100), (0, 0, 3, 90), (0, 0, 3, 90)]
    # two empty sketches are two clusters; a cell of count 0 links nothing
    assert reps_model([0, 0], [], JAC, 1, 1000000) == ([(0, 0, 1, 0), (1, 1, 1, 0)], 2, 0)
    assert reps_model([0, 0], [(0, 1, 0)], CON, 1, 1000000) == ([(0, 0, 1, 0), (1, 1, 1, 0)], 2, 0)
    assert reps_model([5, 5], [(0, 1, 0)], CON, 1, 1000000)[1:] == (2, 0)
    # clusters are numbered by their first-listed member, whoever represents them
    rows, nc, _ = reps_model([10, 50, 50, 10, 70, 50], [(1, 2, 50), (2, 5, 50), (0, 3, 10), (3, 4, 10)], CON, 1, 1)
    assert [r[:3] for r in rows] == [(0, 0, 1), (1, 1, 2), (1, 1, 2), (2, 4, 2), (2, 4, 2), (3, 5, 1)] and nc == 4


def test_the_best_representative_may_come_later():
    """containment 1/2: a (100 keys) is put out by r (200 keys, 50 shared), b (90 keys) shares 85 with a and nothing with r, so b
    represents too -- and a's best representative is b, which comes behind a in the order.  r still comes before a"""
    card, cells = [200, 100, 90], [(0, 1, 50), (1, 2, 85)]
    rows, nc, ne = reps_model(card, cells, CON, 1, 2)
    assert (rows, nc, ne) == ([(0, 0, 1, 200), (1, 2, 2, 85), (1, 2, 2, 90)], 2, 2)
    check_consequences(rows, nc, card, cells, CON, 1, 2)
    got = reps_model_np(card, pack(cells), CON, 1, 2)
    assert (as_tuples(got[0]), got[1], got[2]) == (rows, nc, ne)


def random_graph(rng):
    n = int(rng.integers(1, 60))
    card = rng.integers(50, 100, n)
    pairs = sorted({(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(0, n, (int(rng.integers(0, 3 * n)), 2)) if a != b})
    cells = [(i, j, int(rng.integers(0, min(card[i], card[j]) + 1))) for i, j in pairs]
    weight = [None, rng.integers(0, 5, n).tolist(), rng.permutation(n).tolist()][int(rng.integers(0, 3))]
    return card.tolist(), cells, weight


def test_the_array_model_is_the_model():
    rng = np.random.default_rng(3)
    for trial in range(60):
        card, cells, weight = random_graph(rng)
        for metric, num, den in ((JAC, 1, 3), (CON, 1, 2), (JAC, 1, 1000000)):
            rows, nc, ne = reps_model(card, cells, metric, num, den, weight)
            got, gc, ge, _ = reps_model_np(card, pack(cells) if cells else np.zeros(0, np.uint64), metric, num, den, weight)
            assert (as_tuples(got), gc, ge) == (rows, nc, ne), (trial, metric)


def test_the_consequences_hold_on_random_graphs():
    rng = np.random.default_rng(4)
    for trial in range(60):
        card, cells, weight = random_graph(rng)
        for metric, num, den in ((JAC, 1, 3), (CON, 1, 2), (CON, 1, 1000000)):
            rows, nc, _ = reps_model(card, cells, metric, num, den, weight)
            check_consequences(rows, nc, card, cells, metric, num, den, weight)


def test_cluster_csv_prints_a_representatives_row_set():
    names = ["a one.fa.gz", "dir/b.two", "c 3.sk.gz", "d.1.2.sketch", "e"]
    card = [1000, 700, 333, 12345, 3]
    cells = [(0, 3, 900), (2, 3, 300), (0, 2, 200), (1, 4, 1)]
    for metric, num, den in ((JAC, 1, 100), (CON, 1, 2)):
        rows = reps_model(card, cells, metric, num, den)[0]
        assert rows[0][1] == 3 and rows[3][1] == 3
        for precision in (6, 3):
            assert sp.cluster_csv(as_rows(rows), names, card, metric, precision) == py_csv(rows, names, card, metric, precision)
    text = sp.cluster_csv(as_rows(reps_model(card, cells, CON, 1, 2)[0]), names, card, CON).decode().splitlines()
    assert text[0] + "\n" == HEADER and text[1] == "a one.fa.gz,0,d.1.2.sketch,3,1000,900,0.9" and text[4] == "d.1.2.sketch,0,d.1.2.sketch,3,12345,12345,1"


def test_abi_has_the_representatives_calls():
    calls = ("spsp_representatives_cells_device", "spsp_representatives_files")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    assert ctypes.sizeof(sp.ClusterRow) == 24 == sp.CLUSTER_ROW_DTYPE.itemsize
    for name in calls:
        assert hasattr(sp.lib(), name)
    assert hasattr(sp.Context, "representatives_cells_device") and hasattr(sp.Context, "representatives_files")


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    (tmp_path / "w2.txt").write_text("5\n7\n")
    (tmp_path / "w1.txt").write_text("5\n")
    (tmp_path / "w3.txt").write_text("5\n7\n9\n")
    (tmp_path / "wbad.txt").write_text("5\n7.5\n")
    (tmp_path / "wneg.txt").write_text("5\n-7\n")
    (tmp_path / "wbig.txt").write_text("5\n%d\n" % (1 << 47))
    (tmp_path / "whuge.txt").write_text("5\n99999999999999999999999999\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-r", "0.5", "-R", "0.5"), ("-r", "0.5", "-r", "0.6")]
    cases += [(f, "0.5") + other for f in ("-r", "-R") for other in (("-c", "0.5"), ("-C", "0.5"), ("-q", "list.txt"), ("-g", "3", "-q", "list.txt"),
                                                                    ("-N", "3"), ("-P", "0.5"))]
    cases += [("-w", "w2.txt"), ("-w", "w2.txt", "-c", "0.5")]
    cases += [("-r", "0.5", "-w", f) for f in ("w1.txt", "w3.txt", "wbad.txt", "wneg.txt", "wbig.txt", "whuge.txt", "no such weights.txt")]
    cases += [("-r", t) for t in ("0", "1.5", "0.1234567", "abc", "", "0.", ".5", "-0.5", "1e-1", "0.5 ", "2")] + [("-R", "0.0000000")]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1, (args, r.stdout, r.stderr)
        assert any(f in r.stdout for f in ("-r", "-R", "-w")), (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


def test_the_collection_shows_what_it_is_there_for():
    """the (31, 11) collection at Jaccard 1/2 and containment 3/5: 43 and 42 representatives, two single-linkage clusters or more
    that hold more than one of them, and a member tied in key count with its representative"""
    k, m = 31, 11
    pl = collection(k, m, S)
    assert pl[0] == pl[3] and len(pl) == 60
    for (metric, num, den), n_reps in zip(FRACTIONS, (43, 42)):
        rows, nc, ne, card, cells = collection_model(k, m, metric, num, den)
        assert nc == n_reps
        check_consequences(rows, nc, card, cells, metric, num, den)
        lab = single_linkage(card, cells, metric, num, den)
        reps_in = {}
        for s, r in enumerate(rows):
            if r[1] == s:
                reps_in[lab[s]] = reps_in.get(lab[s], 0) + 1
        assert len(set(lab)) < nc and sum(1 for c in reps_in.values() if c > 1) >= 2, metric
        assert any(r[1] != s and card[r[1]] == card[s] for s, r in enumerate(rows)), metric
        assert rows[0][:3] == rows[3][:3] and card[0] == card[3]             # the two unmutated copies of an ancestor: one cluster
        got = reps_model_np(card, pack(cells), metric, num, den)
        assert (as_tuples(got[0]), got[1], got[2]) == (rows, nc, ne)


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


def gpu_reps(ctx, cells, card, metric, num, den, weight=None):
    """cells: packed uint64 words on the host -> (rows, n_clusters, n_edges, rounds) of the device's selection"""
    d = upload(cells) if len(cells) else None
    return ctx.representatives_cells_device(d.data_ptr() if d is not None else None, len(cells), card, len(card), metric, num, den, weight)


def in_three_orders(ctx, cells, card, metric, num, den, want, weight=None):
    """sorted, reversed and shuffled: the same rows and counts every time -> the rounds of the three runs"""
    cells = np.sort(cells)
    rng = np.random.default_rng(len(cells))
    w_rows, w_nc, w_ne = want[:3]
    rounds = []
    for order in (cells, cells[::-1], rng.permutation(cells)):
        rows, nc, ne, nr = gpu_reps(ctx, order, card, metric, num, den, weight)
        assert (nc, ne) == (w_nc, w_ne)
        assert np.array_equal(rows, w_rows)
        rounds.append(nr)
    return rounds


@pytest.mark.gpu
def test_a_path_along_the_order(ctx):
    """(a) 4 097 sketches, c_i = 10^6 - i, cells (i, i + 1) that all pass: sketches 0, 2, 4, ... represent.  Representative 2t needs
    2t - 1 out, which needs 2t - 2 to BE a representative in an earlier round: 2 049 rounds or more, across the
    32 / 64 / ... / 1 024 batch boundaries; never more than one round per sketch"""
    n = 4097
    card = 10 ** 6 - np.arange(n)
    i = np.arange(n - 1, dtype=np.uint64)
    cells = i << np.uint64(48) | (i + np.uint64(1)) << np.uint64(32) | np.uint64(990_000)
    want = reps_model_np(card, cells, JAC, 9, 10)
    rows = want[0]
    assert want[1:3] == (2049, n - 1) and want[3] == 2049
    # an odd sketch sits between two representatives and shares as much with both: the smaller union wins, the one behind it
    assert (rows["representative"][::2] == np.arange(0, n, 2)).all() and (rows["representative"][1::2] == np.arange(2, n, 2)).all()
    assert rows["size"][0] == 1 and (rows["size"][1:] == 2).all() and (rows["shared"][1::2] == 990_000).all()
    assert (rows["cluster"] == (np.arange(n) + 1) // 2).all()
    for nr in in_three_orders(ctx, cells, card, JAC, 9, 10, want):
        assert 2049 <= nr <= n


@pytest.mark.gpu
def test_a_path_under_a_random_permutation(ctx):
    """(a) the same path over 65 535 indices in a random order: the shallow case"""
    rng = np.random.default_rng(41)
    p = rng.permutation(NMAX).astype(np.uint64)
    card = 1000 + (np.arange(NMAX) * 7919 % 13)
    a, b = np.minimum(p[:-1], p[1:]), np.maximum(p[:-1], p[1:])
    cells = a << np.uint64(48) | b << np.uint64(32) | np.uint64(950)
    want = reps_model_np(card, cells, JAC, 1, 2)
    assert want[2] == NMAX - 1 and NMAX // 3 < want[1] < NMAX // 2 + 2 and want[3] < 64
    for nr in in_three_orders(ctx, cells, card, JAC, 1, 2, want):
        assert 1 <= nr < 64


@pytest.mark.gpu
def test_a_star_with_its_centre_last_and_first(ctx):
    """(b) the centre last in the order: 65 534 representatives and one member whose best-representative word takes 65 534
    candidates, several equal fractions among them; the centre first: one representative, 65 534 members"""
    i = np.arange(NMAX - 1, dtype=np.uint64)
    x = np.uint64(60) + i % np.uint64(30)                                    # 89 of 100 is the best fraction, 2 184 times
    cells = i << np.uint64(48) | np.uint64(NMAX - 1) << np.uint64(32) | x
    card = np.full(NMAX, 100)
    card[NMAX - 1] = 99
    want = reps_model_np(card, cells, CON, 1, 2)
    rows = want[0]
    assert want[1:3] == (NMAX - 1, NMAX - 1) and (rows["size"] == 1).sum() == NMAX - 2
    assert tuple(rows[NMAX - 1]) == (29, 29, 2, 0, 89) and rows["size"][29] == 2
    in_three_orders(ctx, cells, card, CON, 1, 2, want)
    # the same with weights in place of key counts: the heaviest of the tied leaves wins
    weight = np.arange(NMAX) % 1000 + 5
    weight[NMAX - 1] = 0
    want = reps_model_np(card, cells, CON, 1, 2, weight)
    assert int(want[0]["representative"][NMAX - 1]) % 30 == 29 and weight[int(want[0]["representative"][NMAX - 1])] == weight[:NMAX - 1][x == 89].max()
    in_three_orders(ctx, cells, card, CON, 1, 2, want, weight)
    card[NMAX - 1] = 101
    want = reps_model_np(card, cells, CON, 1, 2)
    rows = want[0]
    assert want[1:3] == (1, NMAX - 1) and (rows["representative"] == NMAX - 1).all() and (rows["size"] == NMAX).all()
    assert (rows["shared"][:-1] == x.astype(np.int64)).all() and rows["shared"][-1] == 101
    for nr in in_three_orders(ctx, cells, card, CON, 1, 2, want):
        assert nr == 2


@pytest.mark.gpu
def test_a_complete_graph_has_one_representative(ctx):
    """(c) 1 999 000 cells: the heaviest sketch represents and every `shared` comes from its one cell"""
    n = 2000
    rng = np.random.default_rng(42)
    card = rng.integers(100, 120, n)
    card[1234] = 121
    i, j = np.triu_indices(n, 1)
    x = rng.integers(50, 101, len(i)).astype(np.uint64)
    cells = i.astype(np.uint64) << np.uint64(48) | j.astype(np.uint64) << np.uint64(32) | x
    assert len(cells) == 1_999_000
    want = reps_model_np(card, cells, JAC, 1, 4)
    rows = want[0]
    assert want[1:3] == (1, 1_999_000) and (rows["representative"] == 1234).all() and (rows["shared"] >= 50).all() and rows["shared"][1234] == 121
    in_three_orders(ctx, cells, card, JAC, 1, 4, want)


def random_cells(seed, n, n_pairs):
    rng = np.random.default_rng(seed)
    card = rng.integers(500, 1000, n)
    pairs = rng.integers(0, n, (n_pairs + n_pairs // 20, 2))
    a, b = pairs.min(1), pairs.max(1)
    keep = np.unique(a[a != b] * 65536 + b[a != b])[:n_pairs]
    rng.shuffle(keep)
    a, b = keep // 65536, keep % 65536
    x = (rng.random(len(a)) * np.minimum(card[a], card[b])).astype(np.uint64) + np.uint64(1)
    return card, a.astype(np.uint64) << np.uint64(48) | b.astype(np.uint64) << np.uint64(32) | x


@pytest.mark.gpu
@pytest.mark.parametrize("metric,num,den", [(JAC, 1, 3), (CON, 1, 2)])
def test_random_cells_about_half_of_which_pass(ctx, metric, num, den):
    """(d) 200 000 cells over 65 535 sketches"""
    card, cells = random_cells(43 + metric, NMAX, 200_000)
    assert len(cells) == 200_000
    want = reps_model_np(card, cells, metric, num, den)
    assert 60_000 < want[2] < 140_000 and 20_000 < want[1] < 60_000 and want[0]["size"].max() > 3
    for nr in in_three_orders(ctx, cells, card, metric, num, den, want):
        assert 2 <= nr <= 64


def no_cells(ctx, n):
    card = list(range(5, 5 + n))
    rows, nc, ne, nr = gpu_reps(ctx, np.zeros(0, np.uint64), card, JAC, 1, 2)
    assert (as_tuples(rows), nc, ne, nr) == ([(i, i, 1, card[i]) for i in range(n)], n, 0, 1)


@pytest.mark.gpu
def test_small_inputs(ctx):
    """(e)"""
    no_cells(ctx, 1)
    no_cells(ctx, 70)
    rows, nc, ne, _ = gpu_reps(ctx, pack([(0, 1, 0)]), [0, 0], CON, 1, 1000000)   # two empty sketches, even with a cell that names them
    assert (as_tuples(rows), nc, ne) == ([(0, 0, 1, 0), (1, 1, 1, 0)], 2, 0)
    for card, cells, weight in (([100, 80, 90], [(0, 1, 60), (1, 2, 55)], None), ([200, 100, 90], [(0, 1, 50), (1, 2, 85)], None),
                                ([100, 60, 1000], [(0, 2, 50), (1, 2, 30)], [5, 9, 1]), ([100, 60, 1000], [(0, 2, 50), (1, 2, 30)], [9, 5, 1])):
        for metric, num, den in ((JAC, 1, 3), (CON, 1, 2)):
            rows, nc, ne, _ = gpu_reps(ctx, pack(cells), card, metric, num, den, weight)
            assert (as_tuples(rows), nc, ne) == reps_model(card, cells, metric, num, den, weight)


@pytest.mark.gpu
@pytest.mark.parametrize("metric,num,den", [(JAC, 1, 3), (CON, 1, 2)])
def test_two_cliques_joined_by_one_cell_at_the_threshold(ctx, metric, num, den):
    """(f) 51 shared keys of 102 and 102 are exactly 1/3 (Jaccard) and 1/2 (containment): sketch 9 is linked to representative 4, is put
    out, and the second clique takes another representative; 50: it is not, and 9 represents"""
    card = [100] * 12
    card[4], card[9] = 102, 102                                             # (4 x = c_4 + c_9 and 2 x = min: 51 is exact under both)
    clique = lambda lo: [(i, j, 80) for i in range(lo, lo + 6) for j in range(i + 1, lo + 6)]
    for x, reps in ((51, (4, 6)), (50, (4, 9))):
        cells = clique(0) + clique(6) + [(4, 9, x)]
        want = reps_model(card, cells, metric, num, den)
        assert want[1:] == (2, 30 + (x == 51)) and tuple(sorted({r[1] for r in want[0]})) == reps
        check_consequences(want[0], want[1], card, cells, metric, num, den)
        words = pack(cells)
        for order in (words, words[::-1], np.random.default_rng(x).permutation(words)):
            rows, nc, ne, _ = gpu_reps(ctx, order, card, metric, num, den)
            assert (as_tuples(rows), nc, ne) == want


@pytest.mark.gpu
def test_fractions_that_round_to_one_double(ctx):
    """(g) key counts near 2^41.  Member 2 shares X = 2^31 keys of U = 2^41 + 1 (Jaccard's denominator) with representative 0 and
    X - 1 of U - 1024 with representative 1: X (U - 1024) - (X - 1) U = 1, the two fractions differ by 2^-72 of themselves, are one
    double, and the products are beyond 64 bits.  Representative 0 is the better one, wherever the weights put it"""
    X, U, C = 1 << 31, (1 << 41) + 1, (1 << 31) + 5
    cells = [(0, 2, X), (1, 2, X - 1)]
    card = [U - C + X, (U - 1024) - C + (X - 1), C]
    assert card[0] + C - X == U and card[1] + C - (X - 1) == U - 1024 and X / U == (X - 1) / (U - 1024) and X * (U - 1024) > (X - 1) * U > 1 << 64
    for weight in (None, [1, 2, 0], [2, 1, 0]):
        want = reps_model(card, cells, JAC, 1, 1000000, weight)
        assert want[1] == 2 and want[0][2] == (0, 0, 2, X)
        for words in (pack(cells), pack(cells)[::-1]):
            rows, nc, ne, _ = gpu_reps(ctx, words, card, JAC, 1, 1000000, weight)
            assert (as_tuples(rows), nc, ne) == want
    # 2^31 / 2^41 against 2^30 / 2^40: equal, products of 2^71: the representative that comes first, whichever the weights make it
    cells = [(0, 2, 1 << 31), (1, 2, 1 << 30)]
    card = [1 << 41, (1 << 40) - (1 << 30), 1 << 31]
    assert card[0] + card[2] - (1 << 31) == 1 << 41 and card[1] + card[2] - (1 << 30) == 1 << 40
    for weight, rep in ((None, 0), ([2, 1, 0], 0), ([1, 2, 0], 1)):
        want = reps_model(card, cells, JAC, 1, 1000000, weight)
        assert want[0][2][1] == rep and want[1] == 2
        for words in (pack(cells), pack(cells)[::-1]):
            rows, nc, ne, _ = gpu_reps(ctx, words, card, JAC, 1, 1000000, weight)
            assert (as_tuples(rows), nc, ne) == want


@pytest.mark.gpu
def test_weights(ctx):
    """(h) the reverse of the key counts, all equal, one of 2^47 - 1; 2^47 is ERR_ARG"""
    card, cells = random_cells(47, 3000, 12_000)
    for weight in (card.max() - card, np.full(len(card), 7), np.where(np.arange(len(card)) == 1500, (1 << 47) - 1, card)):
        want = reps_model_np(card, cells, CON, 1, 2, weight)
        in_three_orders(ctx, cells, card, CON, 1, 2, want, weight)
    assert as_tuples(reps_model_np(card, cells, CON, 1, 2, np.full(len(card), 7))[0]) != as_tuples(reps_model_np(card, cells, CON, 1, 2)[0])
    heavy = np.where(np.arange(len(card)) == 1500, (1 << 47) - 1, card)
    assert reps_model_np(card, cells, CON, 1, 2, heavy)[0]["representative"][1500] == 1500
    with pytest.raises(sp.SpspError) as e:
        gpu_reps(ctx, cells, card, CON, 1, 2, np.where(np.arange(len(card)) == 1500, 1 << 47, card))
    assert e.value.code == sp.ERR_ARG and "weight" in str(e.value)
    no_cells(ctx, 70)


@pytest.mark.gpu
def test_bad_cells_and_bad_arguments_are_refused(ctx):
    """(i) a cell with j == n, one with i == j, one with i > j: ERR_ARG, the rows zeroed, and the context answers afterwards"""
    card = [100] * 10
    good = [(0, 1, 80), (2, 3, 80)]
    for bad in ((3, 10, 80), (4, 4, 80), (7, 2, 80), (65535, 65535, 1)):
        d = upload(pack(good + [bad] + good))
        rows = np.ones(10, dtype=sp.CLUSTER_ROW_DTYPE)
        nc, ne, nr = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        c = np.asarray(card, dtype=np.uint64)
        rc = sp.lib().spsp_representatives_cells_device(ctx._h, d.data_ptr(), 5, c.ctypes.data, None, 10, JAC, 1, 2, rows.ctypes.data,
                                                        ctypes.byref(nc), ctypes.byref(ne), ctypes.byref(nr))
        assert rc == sp.ERR_ARG and b"cell" in sp.lib().spsp_last_error() and not rows.view(np.uint8).any()
        no_cells(ctx, 1)
        no_cells(ctx, 70)
    cells = upload(pack(good))
    call = lambda n=10, metric=JAC, num=1, den=2, c=card: ctx.representatives_cells_device(
        cells.data_ptr(), 2, c[:n] if n <= len(c) else c + [1] * (n - len(c)), n, metric, num, den)
    for kw in (dict(n=0), dict(n=65536), dict(metric=2), dict(metric=-1), dict(num=0), dict(num=3), dict(num=1000001, den=1000001),
               dict(den=1000001), dict(c=[100] * 9 + [1 << 47])):
        with pytest.raises(sp.SpspError) as e:
            call(**kw)
        assert e.value.code == sp.ERR_ARG, kw
    rows, nc, ne, _ = call()
    assert (as_tuples(rows), nc, ne) == reps_model(card, good, JAC, 1, 2)
    assert call(num=1000000, den=1000000)[1:3] == (10, 0)


def gpu_cells(ctx, payloads):
    """decode, the all-vs-all as cells -> (the cells' tensor, their number, card)"""
    import torch
    n = len(payloads)
    k, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
    scratch = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    cells = torch.zeros(n * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cnt = ctx.compare_cells_device(k, d_mn, d_lo, d_hi, off, n, scratch.data_ptr(), cells.data_ptr(), cells.numel())
    return cells, cnt, np.diff(off.astype(np.int64)).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", KM)
def test_the_family_collection_from_sketches_to_representatives(ctx, k, m):
    """(j)"""
    cells, cnt, card = gpu_cells(ctx, collection(k, m, S))
    for metric, num, den in FRACTIONS:
        want, w_nc, w_ne, w_card, _ = collection_model(k, m, metric, num, den)
        rows, nc, ne, nr = ctx.representatives_cells_device(cells.data_ptr(), cnt, card, len(card), metric, num, den)
        assert card == w_card and (as_tuples(rows), nc, ne) == (want, w_nc, w_ne) and 1 <= nr <= len(card), metric


def write_files(root, payloads, tag="f"):
    paths = []
    for i, p in enumerate(payloads):
        paths.append(os.path.join(str(root), "%s %03d.sk.gz" % (tag, i)))  # (names with a space and dots)
        sp.write_gz(paths[-1], p, 1)
    return paths


def gunzip(path):
    return gzip.open(path, "rb").read()


@pytest.mark.gpu
def test_representatives_files_and_the_command_line(ctx, tmp_path):
    """(j)"""
    k, m = 31, 11
    pl = collection(k, m, S)
    paths = write_files(tmp_path, pl)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    for (metric, num, den), flag, t in zip(FRACTIONS, ("-r", "-R"), ("0.5", "0.60")):
        want, w_nc, w_ne, card, cells = collection_model(k, m, metric, num, den)
        text = py_csv(want, paths, card, metric)
        rows, nc = ctx.representatives_files(paths, str(tmp_path / "lib"), metric, num, den)
        assert as_tuples(rows) == want and nc == w_nc
        assert gunzip(str(tmp_path / "lib_representatives.csv.gz")) == text
        rows, nc = ctx.representatives_files(paths, str(tmp_path / "p3"), metric, num, den, precision=3)
        assert as_tuples(rows) == want and gunzip(str(tmp_path / "p3_representatives.csv.gz")) == py_csv(want, paths, card, metric, 3)
        r = run(flag, t, "-f", "list.txt", "-o", "cli")
        assert r.returncode == 0, r.stdout + r.stderr
        assert gunzip(str(tmp_path / "cli_representatives.csv.gz")) == text
        out = r.stdout.splitlines()
        assert out[:2] == ["No query file, I will perform a all versus all comparison", "I found %d documents" % len(pl)]
        assert out[2] == "kmers evaluated are of length: %d minimizer size is %d" % (k, m)
        head = "%d sketches, %d edges, %d representatives, the largest cluster of %d, " % (len(pl), w_ne, w_nc, max(x[2] for x in want))
        assert out[3].startswith(head) and out[3].endswith(" rounds") and 1 <= int(out[3][len(head):].split()[0]) <= len(pl) and len(out) == 4
        # weights: the reverse of the list order
        weight = list(range(len(pl), 0, -1))
        weight[7] = weight[8]                                                # (and one tie)
        (tmp_path / "w.txt").write_text("".join("%d\n" % w for w in weight))
        w_want, w_count, _ = reps_model(card, cells, metric, num, den, weight)
        assert w_want != want
        rows, nc = ctx.representatives_files(paths, str(tmp_path / "libw"), metric, num, den, weight=weight)
        assert as_tuples(rows) == w_want and nc == w_count
        r = run(flag, t, "-w", "w.txt", "-f", "list.txt", "-o", "cliw")
        assert r.returncode == 0, r.stdout + r.stderr
        assert gunzip(str(tmp_path / "cliw_representatives.csv.gz")) == py_csv(w_want, paths, card, metric) == gunzip(str(tmp_path / "libw_representatives.csv.gz"))
        os.remove(str(tmp_path / "cli_representatives.csv.gz"))
    assert not [f for f in os.listdir(tmp_path) if "_jaccard" in f or "_containment" in f or "_clusters" in f]
    # -c and -r under one prefix do not overwrite each other
    r = run("-c", "0.5", "-f", "list.txt", "-o", "cliw")
    assert r.returncode == 0 and os.path.exists(str(tmp_path / "cliw_clusters.csv.gz")) and os.path.exists(str(tmp_path / "cliw_representatives.csv.gz"))
    with pytest.raises(sp.SpspError) as e:
        ctx.representatives_files(paths, str(tmp_path / "no"), JAC, 1, 2, weight=[1 << 47] * len(paths))
    assert e.value.code == sp.ERR_ARG and not [f for f in os.listdir(tmp_path) if f.startswith("no")]


@pytest.mark.gpu
def test_representatives_files_at_a_common_rate(ctx, tmp_path):
    """(j) some files at -s 10, the others at -s 100, rate="auto": the representatives of the -s 100 sketches of the same genomes"""
    k, m = 31, 11
    coarse, fine = collection(k, m, S), collection(k, m, 10.0)
    mixed = [fine[i] if i % 3 == 1 else coarse[i] for i in range(len(coarse))]
    paths = write_files(tmp_path, mixed)
    metric, num, den = FRACTIONS[0]
    want, w_nc, _, card, _ = collection_model(k, m, metric, num, den)
    for tag, rate in (("auto", "auto"), ("r100", 100)):
        rows, nc = ctx.representatives_files(paths, str(tmp_path / tag), metric, num, den, rate=rate)
        assert as_tuples(rows) == want and nc == w_nc
        assert gunzip(str(tmp_path / (tag + "_representatives.csv.gz"))) == py_csv(want, paths, card, metric)
    # k == m: refused with and without a rate
    kk = [orc.sketch_fasta(synth.to_fasta(g[:5000], "g%d" % i), 11, 11, S)[0] for i, g in enumerate(_genomes()[:3])]
    p3 = write_files(tmp_path, kk, "kk")
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.representatives_files(p3, str(tmp_path / "no"), metric, num, den, rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no")]


@pytest.mark.gpu
def test_single_linkage_and_representatives_on_one_context(ctx):
    """(k) in both orders, each leaves the other's result untouched"""
    card, cells = random_cells(45, 5000, 30_000)
    d = upload(cells)
    want = reps_model_np(card, cells, JAC, 1, 3)
    args = (d.data_ptr(), len(cells), card, len(card), JAC, 1, 3)
    single = ctx.cluster_cells_device(*args)
    reps = ctx.representatives_cells_device(*args)
    assert np.array_equal(reps[0], want[0]) and reps[1:3] == want[1:3] and reps[2] == single[2] and reps[1] > single[1]
    again = ctx.cluster_cells_device(*args)
    assert np.array_equal(again[0], single[0]) and again[1:] == single[1:]
    no_cells(ctx, 70)
    reps2 = ctx.representatives_cells_device(*args)
    assert np.array_equal(reps2[0], want[0]) and reps2[1:3] == want[1:3]
    fresh = sp.Context(0)
    try:
        first = fresh.representatives_cells_device(*args)
        then = fresh.cluster_cells_device(*args)
        assert np.array_equal(first[0], want[0]) and np.array_equal(then[0], single[0]) and then[1:] == single[1:]
    finally:
        fresh.close()
