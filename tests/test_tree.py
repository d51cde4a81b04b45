"""Linkage tree: the single-linkage dendrogram of a collection (include/spsp.h: spsp_tree_cells_device, spsp_tree_cut_host,
spsp_tree_csv_host, spsp_tree_newick_host, spsp_tree_files; bin/comparator -l / -L).

The rule, on sets of the comparator's keys.  Sketches are 0 .. n-1 in list order, c_i = |K_i|, a cell (i < j, x) names the x keys two
sketches share, the floor is the fraction num / den with 0 <= num <= den:

    1. a cell is a candidate iff x >= 1 and x * den >= num * u, u = c_i + c_j - x (metric 0, Jaccard) or min(c_i, c_j) (metric 1)
    2. edge a comes before edge b iff x_a / u_a > x_b / u_b as fractions, or they are equal and (i_a, j_a) < (i_b, j_b)
    3. going through the candidates in that order an edge is kept iff its ends are not yet connected by kept edges (Kruskal)
    4. one row (a, b, size, shared) per kept edge, in that order; size = the sketches of the merged cluster
    5. cut at num' / den' >= the floor: the rows that pass 1 at num' / den', their components numbered by first-listed member
       = the clustering of ALL cells at num' / den' (the cut property of a maximum spanning forest)
    6. Newick: quoted names, a row's node at height 1.0 - x / u (doubles, printed only), branch length = the difference of two
       heights, the child with the smaller sketch index first, what never merges joined at height 1.0 in first-member order

Every expected value comes from a Python model written from these steps (tree_model: fractions.Fraction and plain loops) or its
numpy form for the long lists (tree_model_np), held to each other on random small graphs: integers and bytes, no tolerance
anywhere."""
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
JAC, CON = 0, 1
HEADER = "step,a,b,shared,keys_a,keys_b,score,size,clusters\n"
NMAX = 65535
U64 = np.uint64


def under(card, i, j, x, metric):
    return card[i] + card[j] - x if metric == JAC else min(card[i], card[j])


def is_candidate(card, i, j, x, metric, num, den):
    return x >= 1 and x * den >= num * under(card, i, j, x, metric)


class Sets:
    """union-find whose root is the set's first-listed member"""

    def __init__(self, n):
        self.up, self.size = list(range(n)), [1] * n

    def find(self, a):
        r = a
        while self.up[r] != r:
            r = self.up[r]
        while self.up[a] != r:
            self.up[a], a = r, self.up[a]
        return r

    def unite(self, ra, rb):
        lo, hi = min(ra, rb), max(ra, rb)
        self.up[hi] = lo
        self.size[lo] += self.size[hi]
        return lo


def tree_model(card, cells, metric, num, den):
    """steps 1-4 -> ([(a, b, size, shared)], n_edges); cells = [(i, j, x)], i < j"""
    n = len(card)
    cand = []
    for i, j, x in cells:
        assert i < j < n
        if is_candidate(card, i, j, x, metric, num, den):
            cand.append((-Fraction(x, under(card, i, j, x, metric)), i, j, x))
    sets, rows = Sets(n), []
    for _, i, j, x in sorted(cand):
        ri, rj = sets.find(i), sets.find(j)
        if ri != rj:
            rows.append((i, j, sets.size[sets.unite(ri, rj)], x))
    return rows, len(cand)


def unpack(cells):
    return (cells >> U64(48)).astype(np.int64), ((cells >> U64(32)) & U64(0xffff)).astype(np.int64), (cells & U64(0xffffffff)).astype(np.int64)


def tree_model_np(card, cells, metric, num, den):
    """the same over numpy arrays, for the cell lists too long for a Python loop (held to tree_model by
    test_the_array_model_is_the_model); cells = packed uint64 words; every product stays below 2^63 (asserted).  The order: a
    sort by the double x / u, then (i, j) -- and then every neighbouring pair of the sorted list is held to step 2 in integers,
    which makes the whole order step 2's (a strict total order is transitive).  Kruskal: edges whose ends carry one label are
    dropped a block at a time, the others go through a union-find one by one"""
    card = np.asarray(card, dtype=np.int64)
    n = len(card)
    i, j, x = unpack(cells)
    u = card[i] + card[j] - x if metric == JAC else np.minimum(card[i], card[j])
    assert len(x) == 0 or (float(x.max()) * max(den, float(u.max())) < 2.0 ** 62 and float(u.max()) * max(num, 1) < 2.0 ** 62)
    cand = (x >= 1) & (x * den >= num * u)
    i, j, x, u = i[cand], j[cand], x[cand], u[cand]
    order = np.lexsort((j, i, -(x / u)))
    i, j, x, u = i[order], j[order], x[order], u[order]
    lhs, rhs = x[:-1] * u[1:], x[1:] * u[:-1]
    assert ((lhs > rhs) | ((lhs == rhs) & (i[:-1] * 65536 + j[:-1] < i[1:] * 65536 + j[1:]))).all()
    sets, kept, sizes = Sets(n), [], []
    label = np.arange(n)
    for s in range(0, len(i), 4096):
        live = np.nonzero(label[i[s:s + 4096]] != label[j[s:s + 4096]])[0]
        for t in (s + live).tolist():
            ri, rj = sets.find(int(i[t])), sets.find(int(j[t]))
            if ri != rj:
                kept.append(t)
                sizes.append(sets.size[sets.unite(ri, rj)])
        if len(live):
            label = np.array([sets.find(v) for v in range(n)])
    rows = np.zeros(len(kept), dtype=sp.TREE_ROW_DTYPE)
    rows["a"], rows["b"], rows["size"], rows["shared"] = i[kept], j[kept], sizes, x[kept]
    return rows, int(cand.sum())


def components(card, cells, metric, num, den):
    """the clustering of all cells at num / den -> (cluster number per sketch, by first-listed member; how many)"""
    sets = Sets(len(card))
    for i, j, x in cells:
        if is_candidate(card, i, j, x, metric, num, den):
            ri, rj = sets.find(i), sets.find(j)
            if ri != rj:
                sets.unite(ri, rj)
    number, out = {}, []
    for s in range(len(card)):
        out.append(number.setdefault(sets.find(s), len(number)))
    return out, len(number)


def cut_model(rows, card, metric, num, den):
    """step 5 from the rows alone"""
    return components(card, [(a, b, x) for a, b, _, x in rows], metric, num, den)


def pack(cells):
    return np.array([(i << 48) | (j << 32) | x for i, j, x in cells], dtype=np.uint64)


def as_tuples(rows):
    assert not np.any(rows["reserved"])
    return [tuple(int(r[f]) for f in ("a", "b", "size", "shared")) for r in rows]


def as_rows(tuples):
    rows = np.zeros(len(tuples), dtype=sp.TREE_ROW_DTYPE)
    for t, (a, b, size, shared) in enumerate(tuples):
        rows[t] = (a, b, size, 0, shared)
    return rows


def py_csv(tuples, names, card, metric, precision=6):
    text = HEADER
    for t, (a, b, size, x) in enumerate(tuples):
        text += "%d,%s,%s,%d,%d,%d,%s,%d,%d\n" % (t + 1, names[a], names[b], x, card[a], card[b], "%.*g" % (precision, x / under(card, a, b, x, metric)),
                                                 size, len(names) - (t + 1))
    return text.encode()


def py_newick(tuples, names, card, metric, precision=6):
    """step 6, without recursion"""
    n = len(names)
    left, right, above, height = {}, {}, {}, [0.0] * n
    sets, node_of = Sets(n), list(range(n))

    def join(ra, rb, h):
        lo, hi = min(ra, rb), max(ra, rb)
        node = len(height)
        left[node], right[node] = node_of[lo], node_of[hi]
        above[node_of[lo]] = above[node_of[hi]] = node
        height.append(h)
        node_of[sets.unite(lo, hi)] = node
    for a, b, _, x in tuples:
        join(sets.find(a), sets.find(b), 1.0 - x / under(card, a, b, x, metric))
    for s in range(1, n):
        if sets.find(s) == s:
            join(0, s, 1.0)
    out, stack = [], [len(height) - 1]
    while stack:
        item = stack.pop()
        if isinstance(item, str):
            out.append(item)
        elif item < n:
            out.append("'" + names[item].replace("'", "''") + "'")
        else:
            l, r = left[item], right[item]
            length = lambda c: ":" + "%.*g" % (precision, height[above[c]] - height[c])
            stack += [")", length(r), r, ",", length(l), l, "("]
    return ("".join(out) + ";\n").encode()


# ------------------------------------------------------------------------------------------ the collections

_cache = {}


def cached(f):
    def g(*a):
        if (f.__name__, a) not in _cache:
            _cache[(f.__name__, a)] = f(*a)
        return _cache[(f.__name__, a)]
    return g


def _genomes():
    """30 genomes in 5 families + 6 unrelated ones, 40 kbp each"""
    fam = synth.family_genomes(5, 30, 40_000, 5, [0.0, 0.01, 0.03])
    rng = np.random.default_rng(6)
    return fam + [synth.random_genome(rng, 40_000) for _ in range(6)]


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


def random_graph(rng):
    n = int(rng.integers(1, 60))
    card = rng.integers(50, 100, n)
    if rng.integers(0, 2):
        card[:] = 64                                                         # (many equal fractions, with different x under containment)
    pairs = sorted({(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(0, n, (int(rng.integers(0, 4 * n)), 2)) if a != b})
    cells = [(i, j, int(rng.integers(0, min(card[i], card[j]) + 1))) for i, j in pairs]
    return card.tolist(), cells


FLOORS = ((JAC, 0, 1), (JAC, 1, 3), (CON, 1, 2), (CON, 0, 1000000))


# ------------------------------------------------------------------------------------------------ not GPU

def test_model_on_hand_made_graphs():
    # a triangle: the worst edge is left out; 60/140, 50/150, 40/160
    assert tree_model([100, 100, 100], [(0, 1, 40), (0, 2, 50), (1, 2, 60)], JAC, 0, 1) == ([(1, 2, 2, 60), (0, 2, 3, 50)], 3)
    # equal fractions: the smaller (i, j) first, and the third edge of the triangle closes a cycle
    assert tree_model([100, 100, 100], [(1, 2, 50), (0, 2, 50), (0, 1, 50)], JAC, 0, 1) == ([(0, 1, 2, 50), (0, 2, 3, 50)], 3)
    # 30/60 and 50/100 under containment are one fraction
    assert tree_model([100, 60, 1000], [(1, 2, 30), (0, 2, 50)], CON, 0, 1)[0] == [(0, 2, 2, 50), (1, 2, 3, 30)]
    # a pair exactly at the floor is a candidate, one key fewer is not; x = 0 never is, whatever the floor
    for metric, num, den in ((JAC, 1, 3), (CON, 1, 2)):
        assert tree_model([100, 100], [(0, 1, 50)], metric, num, den) == ([(0, 1, 2, 50)], 1)
        assert tree_model([100, 100], [(0, 1, 49)], metric, num, den) == ([], 0)
    assert tree_model([5, 5], [(0, 1, 0)], CON, 0, 1) == ([], 0)
    # the floor takes the bridge between two groups away
    card, cells = [100] * 6, [(0, 1, 90), (1, 2, 80), (3, 4, 90), (4, 5, 80), (2, 3, 20)]
    assert tree_model(card, cells, JAC, 0, 1)[0][-1] == (2, 3, 6, 20) and len(tree_model(card, cells, JAC, 1, 5)[0]) == 4
    # sizes follow the merges, not the list: the two pairs first, then their join
    assert tree_model([100] * 4, [(0, 1, 90), (2, 3, 80), (1, 2, 70)], JAC, 0, 1)[0] == [(0, 1, 2, 90), (2, 3, 2, 80), (1, 2, 4, 70)]


def test_the_array_model_is_the_model():
    rng = np.random.default_rng(3)
    for trial in range(80):
        card, cells = random_graph(rng)
        for metric, num, den in FLOORS:
            rows, ne = tree_model(card, cells, metric, num, den)
            got, ge = tree_model_np(card, pack(cells) if cells else np.zeros(0, U64), metric, num, den)
            assert (as_tuples(got), ge) == (rows, ne), (trial, metric)


def test_the_cut_is_the_clustering_of_all_cells():
    """step 5 on random graphs: spsp_tree_cut_host over the model's rows against the components of ALL cells, at the floor and above"""
    rng = np.random.default_rng(4)
    for trial in range(60):
        card, cells = random_graph(rng)
        for metric, num, den in FLOORS:
            rows, _ = tree_model(card, cells, metric, num, den)
            assert len(rows) == len(card) - components(card, cells, metric, num, den)[1]
            for cn, cd in ((num, den), (2, 5), (1, 2), (2, 3), (9, 10), (1, 1)):
                if cn * den < num * cd:
                    continue
                want = components(card, cells, metric, cn, cd)
                assert cut_model(rows, card, metric, cn, cd) == want
                cluster, nc = sp.tree_cut(as_rows(rows), card, metric, num, den, cn, cd)
                assert (cluster.tolist(), nc) == want, (trial, metric, cn, cd)


NAMES = ["it's.fa", "a:b", "c,d", "(e)", "plain name.sk.gz", "''", "g;h"]


def test_csv_and_newick_of_hand_built_rows():
    card = [100, 90, 80, 70, 60, 50, 40]
    cells = [(0, 1, 80), (1, 2, 60), (3, 4, 55), (0, 2, 10), (5, 6, 0)]          # three components: {0,1,2} {3,4} {5} {6} -> four
    for metric in (JAC, CON):
        rows, _ = tree_model(card, cells, metric, 0, 1)
        assert len(rows) == 3
        for precision in (6, 3):
            assert sp.tree_csv(as_rows(rows), NAMES, card, metric, precision) == py_csv(rows, NAMES, card, metric, precision)
            assert sp.tree_newick(as_rows(rows), NAMES, card, metric, precision) == py_newick(rows, NAMES, card, metric, precision)
    rows, _ = tree_model(card, cells, CON, 0, 1)
    assert rows == [(3, 4, 2, 55), (0, 1, 2, 80), (1, 2, 3, 60)]                  # 55/60, 80/90, 60/80
    text = sp.tree_csv(as_rows(rows), NAMES, card, CON).decode().splitlines()
    assert text[0] + "\n" == HEADER and text[1] == "1,(e),plain name.sk.gz,55,70,60,0.916667,2,6" and text[2] == "2,it's.fa,a:b,80,100,90,0.888889,2,5" and text[3] == "3,a:b,c,d,60,90,80,0.75,3,4"
    # heights: 1 - 80/90, 1 - 60/80 for {0,1,2}; 1 - 55/60 for {3,4}; joined at 1.0 one after another: (((A,B),C),D)
    h01, h012, h34 = 1.0 - 80 / 90, 1.0 - 60 / 80, 1.0 - 55 / 60
    g = lambda v: "%.6g" % v
    want = ("(((((\'it\'\'s.fa\':%s,\'a:b\':%s):%s,\'c,d\':%s):%s,(\'(e)\':%s,\'plain name.sk.gz\':%s):%s):0,\'\'\'\'\'\':1):0,\'g;h\':1);\n"
            % (g(h01), g(h01), g(h012 - h01), g(h012), g(1.0 - h012), g(h34), g(h34), g(1.0 - h34)))
    assert sp.tree_newick(as_rows(rows), NAMES, card, CON).decode() == want
    # three components, no rows at all: ((A,B),C); one sketch: 'name';
    assert sp.tree_newick(as_rows([]), ["A", "B", "C"], [1, 1, 1], JAC) == b"(('A':1,'B':1):0,'C':1);\n" == py_newick([], ["A", "B", "C"], [1, 1, 1], JAC)
    assert sp.tree_newick(as_rows([]), ["o'ne"], [5], JAC) == b"'o''ne';\n" == py_newick([], ["o'ne"], [5], JAC)
    assert sp.tree_csv(as_rows([]), ["one"], [5], JAC) == HEADER.encode()
    cluster, nc = sp.tree_cut(as_rows([]), [5], JAC, 0, 1, 1, 1)
    assert (cluster.tolist(), nc) == ([0], 1)
    # a node's first child is the one that holds the smaller sketch, whichever end the row names first
    rows = [(2, 3, 2, 50), (0, 1, 2, 40), (1, 3, 4, 30)]
    assert sp.tree_newick(as_rows(rows), list("ABCD"), [100] * 4, CON, 2) == b"(('A':0.6,'B':0.6):0.1,('C':0.5,'D':0.5):0.2);\n"


def path_rows(n):
    """the round-budget path: 0 - 1 - ... - (n-1), x(i, i+1) = 20 - ctz(i+1), every sketch 100 keys"""
    i = np.arange(n - 1, dtype=np.int64)
    v = i + 1
    ctz = np.round(np.log2((v & -v).astype(np.float64))).astype(np.int64)   # (v & -v is a power of two: its logarithm is exact)
    x = 20 - ctz
    return i.astype(U64) << U64(48) | (i + 1).astype(U64) << U64(32) | x.astype(U64)


def test_a_path_of_65535_leaves_does_not_overflow_the_stack():
    """a caterpillar 65 534 levels deep: (i, i + 1) with falling scores, so that every row puts one leaf on top of everything before it"""
    n = NMAX
    rows = np.zeros(n - 1, dtype=sp.TREE_ROW_DTYPE)
    rows["a"], rows["b"], rows["size"], rows["shared"] = np.arange(n - 1), np.arange(1, n), np.arange(2, n + 1), 70_000 - np.arange(n - 1)
    names = ["s%d" % i for i in range(n)]
    card = [100_000] * n
    tuples = list(zip(rows["a"].tolist(), rows["b"].tolist(), rows["size"].tolist(), rows["shared"].tolist()))
    text = sp.tree_newick(rows, names, card, CON)
    assert text.startswith(b"(" * (n - 1) + b"'s0':0.3,'s1':0.3):1e-05,'s2':") and text == py_newick(tuples, names, card, CON)
    assert sp.tree_csv(rows, names, card, CON) == py_csv(tuples, names, card, CON)
    cluster, nc = sp.tree_cut(rows, card, CON, 0, 1, 1, 2)                   # x >= 50 000: the first 20 001 rows
    assert nc == n - 20_001 and cluster[:20_002].max() == 0 and cluster[-1] == nc - 1


def test_bad_rows_and_cuts_below_the_floor_are_refused():
    card, rows = [100, 100, 100], as_rows([(0, 1, 2, 60), (1, 2, 3, 50)])
    assert sp.tree_cut(rows, card, JAC, 1, 4, 1, 4)[1] == 1 and sp.tree_cut(rows, card, JAC, 1, 4, 1, 2)[1] == 3
    assert sp.tree_cut(rows, card, JAC, 1, 4, 25, 100)[1] == 1                   # the floor itself, written differently
    bad_cuts = [dict(fn=1, fd=4, n=249999, d=1000000), dict(fn=1, fd=4, n=0, d=1), dict(fn=1, fd=2, n=1, d=3), dict(fn=0, fd=0, n=1, d=2),
                dict(fn=0, fd=1, n=1, d=0), dict(fn=0, fd=1, n=3, d=2), dict(fn=2, fd=1, n=1, d=1), dict(fn=0, fd=1000001, n=1, d=2),
                dict(fn=0, fd=1, n=1, d=1000001), dict(fn=0, fd=1, n=1, d=2, metric=2)]
    for kw in bad_cuts:
        with pytest.raises(sp.SpspError) as e:
            sp.tree_cut(rows, card, kw.get("metric", JAC), kw["fn"], kw["fd"], kw["n"], kw["d"])
        assert e.value.code == sp.ERR_ARG, kw
    with pytest.raises(sp.SpspError) as e:
        sp.tree_cut(rows, card, JAC, 1, 2, 1, 3)
    assert "below the floor" in str(e.value)
    names = ["a", "b", "c"]
    for bad in ([(1, 1, 2, 5)], [(2, 1, 2, 5)], [(0, 3, 2, 5)], [(0, 1, 2, 5), (0, 2, 3, 5), (1, 2, 3, 5)]):
        for call in (lambda r: sp.tree_cut(r, card, JAC, 0, 1, 0, 1), lambda r: sp.tree_csv(r, names, card, JAC), lambda r: sp.tree_newick(r, names, card, JAC)):
            with pytest.raises(sp.SpspError) as e:
                call(as_rows(bad))
            assert e.value.code == sp.ERR_ARG, bad
    with pytest.raises(sp.SpspError) as e:                                       # two rows that join the same two sketches: no tree
        sp.tree_newick(as_rows([(0, 1, 2, 5), (0, 1, 2, 5)]), names, card, JAC)
    assert e.value.code == sp.ERR_ARG and "joined already" in str(e.value)
    for call in (sp.tree_csv, sp.tree_newick):
        with pytest.raises(sp.SpspError):
            call(rows, names, card, 2)


def test_the_device_call_refuses_its_arguments_before_it_touches_a_device():
    """n, the metric, the floor and the key counts are judged before the context is looked at: with no context at all a good set of
    arguments is refused for the missing context, a bad one for what is wrong with it"""
    def call(n=10, metric=JAC, num=1, den=2, c=None):
        card = np.asarray(c if c is not None else [100] * n, dtype=np.uint64)
        rows = np.ones(max(n, 2) - 1, dtype=sp.TREE_ROW_DTYPE)
        nr, ne, rounds = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint32(7)
        rc = sp.lib().spsp_tree_cells_device(None, None, 0, card.ctypes.data, n, metric, num, den, rows.ctypes.data, ctypes.byref(nr), ctypes.byref(ne),
                                             ctypes.byref(rounds))
        assert rc == sp.ERR_ARG and (nr.value, ne.value, rounds.value) == (0, 0, 0)
        return sp.lib().spsp_last_error().decode()
    assert "NULL" in call() and "NULL" in call(num=0, den=1) and "NULL" in call(num=1000000, den=1000000) and "NULL" in call(n=NMAX, c=[1] * NMAX)
    assert "65535" in call(n=0, c=[1]) and "65535" in call(n=65536, c=[1] * 65536)
    assert "metric" in call(metric=2) and "metric" in call(metric=-1)
    for kw in (dict(num=3, den=2), dict(num=0, den=0), dict(num=1, den=1000001), dict(num=1000001, den=1000001)):
        assert "floor" in call(**kw), kw
    assert "2^47" in call(c=[100] * 9 + [1 << 47]) and "NULL" in call(c=[100] * 9 + [(1 << 47) - 1])


def test_abi_has_the_tree_calls():
    calls = ("spsp_tree_cells_device", "spsp_tree_cut_host", "spsp_tree_csv_host", "spsp_tree_newick_host", "spsp_tree_files")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    assert ctypes.sizeof(sp.TreeRow) == 24 == sp.TREE_ROW_DTYPE.itemsize
    for name in calls:
        assert hasattr(sp.lib(), name)
    assert hasattr(sp.Context, "tree_cells_device") and hasattr(sp.Context, "tree_files")


REFUSED_WITH = (("-q", "list.txt"), ("-g", "3", "-q", "list.txt"), ("-c", "0.5"), ("-C", "0.5"), ("-N", "3"), ("-P", "0.5"), ("-r", "0.5"), ("-R", "0.5"))


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-l", "0.5", "-L", "0.5"), ("-l", "0.5", "-l", "0.6"), ("-L", "0", "-L", "0")]
    cases += [(f, "0.5") + other for f in ("-l", "-L") for other in REFUSED_WITH]
    cases += [("-l", t) for t in ("1.5", "0.1234567", "abc", "", "0.", ".5", "-0.5", "1e-1", "0.5 ", "2")] + [("-L", "1.0000001")]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1, (args, r.stdout, r.stderr)
        assert any(f in r.stdout for f in ("-l", "-L")), (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


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


def gpu_tree(ctx, cells, card, metric, num, den):
    """cells: packed uint64 words on the host -> (rows, n_edges, rounds) of the device's tree"""
    d = upload(cells) if len(cells) else None
    return ctx.tree_cells_device(d.data_ptr() if d is not None else None, len(cells), card, len(card), metric, num, den)


def in_three_orders(ctx, cells, card, metric, num, den, want):
    """sorted, reversed and shuffled: the same rows and candidate count every time -> the rounds of the three runs"""
    cells = np.sort(np.asarray(cells, dtype=U64))
    rng = np.random.default_rng(len(cells))
    w_rows, w_ne = want
    if not isinstance(w_rows, np.ndarray):
        w_rows = as_rows(w_rows)
    rounds = []
    for order in (cells, cells[::-1], rng.permutation(cells)):
        rows, ne, nr = gpu_tree(ctx, order, card, metric, num, den)
        assert ne == w_ne and len(rows) == len(w_rows)
        assert np.array_equal(rows, w_rows)
        rounds.append(nr)
    return rounds


def log2_floor(n):
    return n.bit_length() - 1


SMALL = (
    ([7], []),                                                               # n = 1
    ([100, 100], []), ([100, 100], [(0, 1, 50)]), ([100, 100], [(0, 1, 0)]),
    ([100, 90, 80, 70, 60], [(0, 1, 50), (1, 2, 60), (2, 3, 30), (3, 4, 55)]),   # a path
    ([100, 90, 80, 70, 60, 50], [(0, 3, 50), (1, 3, 60), (2, 3, 30), (3, 4, 55), (3, 5, 50)]),   # a star
    ([100, 100, 100], [(0, 1, 40), (0, 2, 50), (1, 2, 60)]),                 # a triangle: (0, 1) is left out
    ([100, 100, 100], [(0, 1, 50), (0, 2, 50), (1, 2, 50)]),
    ([100, 60, 1000], [(1, 2, 30), (0, 2, 50)]),
    ([5, 5, 9], [(0, 1, 0), (1, 2, 0), (0, 2, 3)]),                          # cells with x = 0
    ([100] * 6, [(0, 1, 90), (1, 2, 80), (3, 4, 90), (4, 5, 80), (2, 3, 20)]),   # a bridge the floor 1/5 takes away
    ([100] * 4, [(0, 1, 90), (2, 3, 80), (1, 2, 70)]),
)


@pytest.mark.gpu
def test_small_graphs(ctx):
    for card, cells in SMALL:
        for metric, num, den in FLOORS + ((JAC, 1, 5), (CON, 1, 1), (JAC, 1000000, 1000000)):
            want = tree_model(card, cells, metric, num, den)
            for nr in in_three_orders(ctx, pack(cells) if cells else np.zeros(0, U64), card, metric, num, den, want):
                assert nr <= log2_floor(len(card)) and (nr >= 1) == bool(want[0])
    card, cells = SMALL[-2]
    assert len(tree_model(card, cells, JAC, 0, 1)[0]) == 5 and len(tree_model(card, cells, JAC, 1, 5)[0]) == 4
    assert gpu_tree(ctx, np.zeros(0, U64), [5] * 70, JAC, 0, 1)[1:] == (0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [JAC, CON])
def test_random_small_graphs(ctx, metric):
    rng = np.random.default_rng(11 + metric)
    for trial in range(25):
        card, cells = random_graph(rng)
        for _, num, den in FLOORS[:2]:
            want = tree_model(card, cells, metric, num, den)
            rows, ne, nr = gpu_tree(ctx, rng.permutation(pack(cells)) if cells else np.zeros(0, U64), card, metric, num, den)
            assert (as_tuples(rows), ne) == want and nr <= log2_floor(len(card)), (trial, num)


@pytest.mark.gpu
def test_one_fraction_everywhere(ctx):
    """a complete graph with one score: the forest is (0, 1), (0, 2), ..., (0, n-1) in that order -- on 300 sketches, and on 2 100,
    where every sketch's best-edge word is offered 2 099 edges"""
    for n in (300, 2100):
        i, j = np.triu_indices(n, 1)
        cells = i.astype(U64) << U64(48) | j.astype(U64) << U64(32) | U64(50)
        rows = np.zeros(n - 1, dtype=sp.TREE_ROW_DTYPE)
        rows["b"], rows["size"], rows["shared"] = np.arange(1, n), np.arange(2, n + 1), 50
        if n == 300:
            got = tree_model_np([100] * n, cells, JAC, 0, 1)
            assert np.array_equal(got[0], rows) and got[1] == len(cells)
        for nr in in_three_orders(ctx, cells, [100] * n, JAC, 0, 1, (rows, len(cells))):
            assert nr == 1


@pytest.mark.gpu
def test_more_than_a_tile_of_equal_edges_between_two_components(ctx):
    """two stars of 50 sketches that the first round makes two components, and 2 500 cells of one score between them: more than one
    tile of live edges meets on two best-edge words in the second round, and (0, 50) must win"""
    h = 50
    star = lambda c: [(c, c + t, 90) for t in range(1, h)]
    cross = [(a, b, 30) for a in range(h) for b in range(h, 2 * h)]
    cells, card = star(0) + star(h) + cross, [100] * (2 * h)
    want = tree_model(card, cells, CON, 0, 1)
    assert len(cross) > 2048 and want[0][-1] == (0, h, 2 * h, 30) and want[1] == len(cells)
    for nr in in_three_orders(ctx, pack(cells), card, CON, 0, 1, want):
        assert nr == 2


def exactness_case():
    """tests/test_neighbours.py's construction: two Jaccard fractions that are one double, the better one at the LARGER index"""
    c_r = 1 << 46
    xa, ca = (1 << 31) + 1, (1 << 46) + 12345
    ua = c_r + ca - xa
    xb = xa + 1
    ub = ua * xb // xa + 1
    cb = ub - c_r + xb
    return [c_r, cb, ca], [(0, 1, xb), (0, 2, xa)]


def high_word_case():
    """two containment fractions whose cross products 2^77 and 2^77 - 2^64 differ only above bit 64, the better one at the larger index"""
    card = [(1 << 47) - 1, 1 << 46, (1 << 47) - (1 << 34)]
    return card, [(0, 1, 1 << 30), (0, 2, 1 << 31)]


def test_the_two_exactness_cases_are_what_they_claim():
    card, cells = exactness_case()
    (_, b, xb), (_, a, xa) = cells
    ua, ub = under(card, 0, a, xa, JAC), under(card, 0, b, xb, JAC)
    assert a > b and max(card) < 1 << 47 and xa / ua == xb / ub and Fraction(xa, ua) > Fraction(xb, ub)
    assert tree_model(card, cells, JAC, 0, 1)[0] == [(0, 2, 2, xa), (0, 1, 3, xb)]
    card, cells = high_word_case()
    (_, b, xb), (_, a, xa) = cells
    ua, ub = under(card, 0, a, xa, CON), under(card, 0, b, xb, CON)
    assert max(card) < 1 << 47 and (xa * ub) % (1 << 64) == (xb * ua) % (1 << 64) and xa * ub > xb * ua and xa * ub - xb * ua == 1 << 64
    assert tree_model(card, cells, CON, 0, 1)[0] == [(0, 2, 2, xa), (0, 1, 3, xb)]


@pytest.mark.gpu
def test_exact_order_where_doubles_and_low_words_tie(ctx):
    for (card, cells), metric in ((exactness_case(), JAC), (high_word_case(), CON)):
        # both edges leave sketch 0, which must choose (0, 2)
        want = tree_model(card, cells, metric, 0, 1)
        assert want[0][0][:2] == (0, 2)
        in_three_orders(ctx, pack(cells), card, metric, 0, 1, want)
        # ... and as the two rivals for one best-edge word in a SECOND round: 0, 1 and 2 each go to a partner of their own first
        x = (1 << 32) - 1
        card6, cells6 = card + [x] * 3, cells + [(0, 5, x), (1, 3, x), (2, 4, x)]
        want = tree_model(card6, cells6, metric, 0, 1)
        assert sorted(r[:2] for r in want[0][:3]) == [(0, 5), (1, 3), (2, 4)] and [r[:2] for r in want[0][3:]] == [(0, 2), (0, 1)]
        for nr in in_three_orders(ctx, pack(cells6), card6, metric, 0, 1, want):
            assert nr == 2


@pytest.mark.gpu
@pytest.mark.parametrize("count", [63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 2 * 2048 + 1])
def test_seams_of_the_edge_list(ctx, count):
    """`count` candidates along a path, interleaved with cells that miss the floor: the wave-append and the compaction of the rounds
    across wave, workgroup and tile ends"""
    rng = np.random.default_rng(count)
    n = count + 1
    i = np.arange(count, dtype=np.int64)
    x = rng.integers(30, 61, count)
    good = i.astype(U64) << U64(48) | (i + 1).astype(U64) << U64(32) | x.astype(U64)
    k = np.arange(n - 2, dtype=np.int64)
    poor = k.astype(U64) << U64(48) | (k + 2).astype(U64) << U64(32) | rng.integers(0, 10, n - 2).astype(U64)
    cells = np.concatenate([good[:1], np.stack([poor, good[1:]], 1).ravel()])    # good, poor, good, poor, ..., good
    card = [100] * n
    want = tree_model_np(card, cells, JAC, 1, 10)
    assert want[1] == count and len(want[0]) == count
    if count <= 257:
        assert (as_tuples(want[0]), want[1]) == tree_model(card, [(int(a), int(b), int(c)) for a, b, c in zip(*unpack(cells))], JAC, 1, 10)
    for nr in in_three_orders(ctx, cells, card, JAC, 1, 10, want):
        assert 2 <= nr <= log2_floor(n)


@pytest.mark.gpu
def test_the_round_budget(ctx):
    """the path 0 - 1 - ... - (n-1) with x(i, i+1) = 20 - ctz(i+1): a round unites the components in pairs and no faster, so
    n = 32 768 takes all of floor(log2 n) = 15 rounds -- a budget one round short leaves the last merge out; at n = 65 535 the rows
    are the model's (32 768 of them hooked in the first round alone)"""
    n = 32768
    cells = path_rows(n)
    assert int((cells & U64(0xffffffff)).min()) == 20 - 14 and int(cells[0] & U64(0xffffffff)) == 20
    card = [100] * n
    want = tree_model_np(card, cells, JAC, 0, 1)
    assert len(want[0]) == n - 1 and tuple(want[0][-1]) == (n // 2 - 1, n // 2, n, 0, 20 - 14)
    rows, ne, nr = gpu_tree(ctx, cells, card, JAC, 0, 1)
    assert nr == 15 and ne == n - 1 and np.array_equal(rows, want[0])
    n = NMAX
    cells = path_rows(n)
    card = [100] * n
    want = tree_model_np(card, cells, JAC, 0, 1)
    assert len(want[0]) == n - 1 and int(want[0]["size"][-1]) == n
    for nr in in_three_orders(ctx, cells, card, JAC, 0, 1, want):
        assert 1 <= nr <= 15


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


CUTS = {(JAC, 1, 10): ((1, 10), (1, 4), (1, 2), (3, 4), (99, 100), (1, 1)), (CON, 1, 5): ((1, 5), (2, 5), (3, 5), (9, 10), (999999, 1000000), (1, 1))}


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", KM)
def test_the_cut_against_the_cluster_pass_on_a_real_comparison(ctx, k, m):
    """the cells of a comparison of 36 sketches ((63, 15): k > 32): the tree's rows are the model's over the oracle's key sets, and its
    cut at six thresholds, the floor and 1/1 among them, is the cluster pass's answer on the same cells"""
    cells, cnt, card = gpu_cells(ctx, collection(k, m, S))
    w_card, w_cells = collection_cells(k, m)
    assert card == w_card and cnt == len(w_cells)
    n = len(card)
    for (metric, num, den), cuts in CUTS.items():
        rows, ne, nr = ctx.tree_cells_device(cells.data_ptr(), cnt, card, n, metric, num, den)
        assert (as_tuples(rows), ne) == tree_model(w_card, w_cells, metric, num, den) and 1 <= nr <= log2_floor(n)
        seen = set()
        for cn, cd in cuts:
            c_rows, nc, c_ne = ctx.cluster_cells_device(cells.data_ptr(), cnt, card, n, metric, cn, cd)
            cluster, got = sp.tree_cut(rows, card, metric, num, den, cn, cd)
            assert got == nc and np.array_equal(cluster, c_rows["cluster"]), (metric, cn, cd)
            if (cn, cd) == (num, den):
                assert len(rows) == n - nc and c_ne == ne
            seen.add(nc)
        assert len(seen) >= 3                                                # the thresholds do cut the tree at different heights
    rows, ne, _ = ctx.tree_cells_device(cells.data_ptr(), cnt, card, n, CON, 0, 1)
    assert (as_tuples(rows), ne) == tree_model(w_card, w_cells, CON, 0, 1) and ne == cnt


@pytest.mark.gpu
def test_bad_cells_are_refused_and_the_context_is_reused(ctx):
    """a cell with j == n, one with i == j, one with i > j: ERR_ARG and the rows zeroed; then a small call behind a larger one"""
    card = [100] * 10
    good = [(0, 1, 80), (2, 3, 80)]
    big_card, big_cells = [100] * 5000, path_rows(5000)
    big = tree_model_np(big_card, big_cells, JAC, 0, 1)
    for bad in ((3, 10, 80), (4, 4, 80), (7, 2, 80), (65535, 65535, 1)):
        d = upload(pack(good + [bad] + good))
        rows = np.ones(9, dtype=sp.TREE_ROW_DTYPE)
        nr, ne, rounds = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        c = np.asarray(card, dtype=np.uint64)
        rc = sp.lib().spsp_tree_cells_device(ctx._h, d.data_ptr(), 5, c.ctypes.data, 10, JAC, 1, 2, rows.ctypes.data, ctypes.byref(nr), ctypes.byref(ne),
                                             ctypes.byref(rounds))
        assert rc == sp.ERR_ARG and b"cell" in sp.lib().spsp_last_error() and not rows.view(np.uint8).any() and nr.value == 0
        got = gpu_tree(ctx, big_cells, big_card, JAC, 0, 1)                  # a larger call ...
        assert np.array_equal(got[0], big[0]) and got[1] == big[1]
        got = gpu_tree(ctx, pack(good), card, JAC, 1, 2)                     # ... and a smaller one behind it, on the same buffers
        assert (as_tuples(got[0]), got[1]) == tree_model(card, good, JAC, 1, 2)
    assert gpu_tree(ctx, np.zeros(0, U64), [9], JAC, 0, 1)[1:] == (0, 0)
    with pytest.raises(sp.SpspError) as e:                                       # n = 1: every cell is a bad one
        gpu_tree(ctx, pack([(0, 1, 5)]), [9], JAC, 0, 1)
    assert e.value.code == sp.ERR_ARG


def write_files(root, payloads, tag="f"):
    paths = []
    for i, p in enumerate(payloads):
        paths.append(os.path.join(str(root), "%s '%03d.sk.gz" % (tag, i)))  # (names with a space, a quote and dots)
        sp.write_gz(paths[-1], p, 1)
    return paths


def gunzip(path):
    return gzip.open(path, "rb").read()


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.gpu
def test_tree_files_and_the_command_line(ctx, tmp_path):
    k, m = 31, 11
    pl = collection(k, m, S)
    paths = write_files(tmp_path, pl)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    card, cells = collection_cells(k, m)
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    for (metric, num, den), flag, t in (((JAC, 1, 2), "-l", "0.5"), ((CON, 0, 1), "-L", "0")):
        want, w_ne = tree_model(card, cells, metric, num, den)
        csv, nwk = py_csv(want, paths, card, metric), py_newick(want, paths, card, metric)
        rows = ctx.tree_files(paths, str(tmp_path / "lib"), metric, num, den)
        assert as_tuples(rows) == want
        assert gunzip(str(tmp_path / "lib_tree.csv.gz")) == csv and read(str(tmp_path / "lib_tree.nwk")) == nwk
        rows = ctx.tree_files(paths, str(tmp_path / "p3"), metric, num, den, precision=3)
        assert as_tuples(rows) == want and gunzip(str(tmp_path / "p3_tree.csv.gz")) == py_csv(want, paths, card, metric, 3)
        assert read(str(tmp_path / "p3_tree.nwk")) == py_newick(want, paths, card, metric, 3)
        r = run(flag, t, "-f", "list.txt", "-o", "cli")
        assert r.returncode == 0, r.stdout + r.stderr
        assert gunzip(str(tmp_path / "cli_tree.csv.gz")) == csv and read(str(tmp_path / "cli_tree.nwk")) == nwk
        out = r.stdout.splitlines()
        assert out[:2] == ["No query file, I will perform a all versus all comparison", "I found %d documents" % len(pl)]
        assert out[2] == "kmers evaluated are of length: %d minimizer size is %d" % (k, m)
        head = "%d sketches, %d candidate edges, %d forest rows, %d components left, " % (len(pl), w_ne, len(want), len(pl) - len(want))
        assert out[3].startswith(head) and out[3].endswith(" rounds") and 1 <= int(out[3][len(head):].split()[0]) <= log2_floor(len(pl)) and len(out) == 4
        for f in ("cli_tree.csv.gz", "cli_tree.nwk"):
            os.remove(str(tmp_path / f))
    assert not [f for f in os.listdir(tmp_path) if "_jaccard" in f or "_containment" in f or "_clusters" in f]
    # every refused combination, with sketch files that exist: nothing is written
    for other in REFUSED_WITH:
        r = run(*(("-l", "0.5") + other + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and "-l / -L" in r.stdout and not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
    # without -l / -L the comparator is what it was
    r = run("-f", "list.txt", "-o", "plain")
    assert r.returncode == 0 and os.path.exists(str(tmp_path / "plain_jaccard.csv.gz")) and not os.path.exists(str(tmp_path / "plain_tree.nwk"))
    for bad in ((JAC, 3, 2), (2, 1, 2), (JAC, 0, 0)):
        with pytest.raises(sp.SpspError) as e:
            ctx.tree_files(paths, str(tmp_path / "no"), *bad)
        assert e.value.code == sp.ERR_ARG and not [f for f in os.listdir(tmp_path) if f.startswith("no")]


@pytest.mark.gpu
def test_tree_files_at_a_common_rate(ctx, tmp_path):
    """some files at -s 10, the others at -s 100, -s auto: the tree of the -s 100 sketches of the same genomes; k == m is refused"""
    k, m = 31, 11
    coarse, fine = collection(k, m, S), collection(k, m, 10.0)
    mixed = [fine[i] if i % 3 == 1 else coarse[i] for i in range(len(coarse))]
    paths = write_files(tmp_path, mixed)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    card, cells = collection_cells(k, m)
    want, _ = tree_model(card, cells, JAC, 1, 4)
    for tag, rate in (("auto", "auto"), ("r100", 100)):
        rows = ctx.tree_files(paths, str(tmp_path / tag), JAC, 1, 4, rate=rate)
        assert as_tuples(rows) == want
        assert gunzip(str(tmp_path / (tag + "_tree.csv.gz"))) == py_csv(want, paths, card, JAC)
        assert read(str(tmp_path / (tag + "_tree.nwk"))) == py_newick(want, paths, card, JAC)
    r = subprocess.run([EXE, "-l", "0.25", "-s", "auto", "-f", "list.txt", "-o", "cli"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert read(str(tmp_path / "cli_tree.nwk")) == py_newick(want, paths, card, JAC) and gunzip(str(tmp_path / "cli_tree.csv.gz")) == py_csv(want, paths, card, JAC)
    kk = [orc.sketch_fasta(synth.to_fasta(g[:5000], "g%d" % i), 11, 11, S)[0] for i, g in enumerate(_genomes()[:3])]
    p3 = write_files(tmp_path, kk, "kk")
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.tree_files(p3, str(tmp_path / "no"), JAC, 1, 4, rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no")]
