"""Clustering: single-linkage dereplication of a collection (include/spsp.h: spsp_cluster_cells_device, spsp_cluster_csv_host,
spsp_cluster_files; bin/comparator -c / -C).

The rule, on sets of the comparator's keys (orc.sketch_keys: the distinct (minimizer, canonical k-mer) pairs of a sketch).
Sketches are 0 .. n-1 in list order, c_i = |K_i|, x_ij = |K_i & K_j|, the threshold is the fraction num / den:

    1. i < j are linked iff x_ij >= 1 and  x_ij * den >= num * (c_i + c_j - x_ij)   (metric 0, Jaccard)
                                       or  x_ij * den >= num * min(c_i, c_j)        (metric 1, the larger containment)
    2. a cluster is a connected component; clusters are numbered in the order of their first-listed member
    3. the representative of a cluster is its member with the most keys, the first listed among equals
    4. row i = (cluster, representative, size, shared): shared = x_{i,rep}, or c_i for the representative itself

Every expected value below comes from the ORACLE's key sets and a Python model written from these four steps (cluster_model):
integers and bytes, no tolerance anywhere."""
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
# the fractions the family collection is clustered at (test_the_collection_shows_what_it_is_there_for holds them to their purpose)
FRACTIONS = ((JAC, 1, 2), (CON, 3, 5))
HEADER = "sketch,cluster,representative,size,keys,shared,score\n"
NMAX = 65535


def cluster_model(card, cells, metric, num, den):
    """the four steps -> ([(cluster, representative, size, shared)] per sketch, n_clusters, n_edges); cells = [(i, j, x)], i < j"""
    n, parent, edges = len(card), list(range(len(card))), 0

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    for i, j, x in cells:
        assert i < j < n
        under = card[i] + card[j] - x if metric == JAC else min(card[i], card[j])
        if x >= 1 and x * den >= num * under:
            edges += 1
            parent[find(i)] = find(j)
    members = {}
    for i in range(n):
        members.setdefault(find(i), []).append(i)
    groups = sorted(members.values())                                       # by first-listed member
    x_of = {(i, j): x for i, j, x in cells}
    rows = [None] * n
    for c, g in enumerate(groups):
        rep = max(g, key=lambda i: (card[i], -i))
        for i in g:
            rows[i] = (c, rep, len(g), card[i] if i == rep else x_of.get((min(i, rep), max(i, rep)), 0))
    return rows, len(groups), edges


def cluster_model_np(card, cells, metric, num, den):
    """the same over numpy arrays, for the cell lists too long for a Python loop (held to cluster_model by
    test_the_array_model_is_the_model); cells = packed uint64 words; every product stays below 2^63"""
    card = np.asarray(card, dtype=np.int64)
    n = len(card)
    i, j = (cells >> np.uint64(48)).astype(np.int64), ((cells >> np.uint64(32)) & np.uint64(0xffff)).astype(np.int64)
    x = (cells & np.uint64(0xffffffff)).astype(np.int64)
    under = card[i] + card[j] - x if metric == JAC else np.minimum(card[i], card[j])
    edge = (x >= 1) & (x * den >= num * under)
    ei, ej = i[edge], j[edge]
    lab = np.arange(n, dtype=np.int64)
    while True:
        a, b = lab[ei], lab[ej]
        if (a == b).all():
            break
        np.minimum.at(lab, np.maximum(a, b), np.minimum(a, b))               # the larger root goes under the smaller
        while True:
            nxt = lab[lab]
            if (nxt == lab).all():
                break
            lab = nxt
    roots, number = np.unique(lab, return_inverse=True)                      # a root is its component's first-listed member
    size = np.bincount(number, minlength=len(roots))
    key = card * 65536 + (65535 - np.arange(n))
    best = np.zeros(len(roots), dtype=np.int64)
    np.maximum.at(best, number, key)
    rep = (65535 - (best % 65536))[number]
    shared = np.zeros(n, dtype=np.int64)
    same = lab[i] == lab[j]
    to_j, to_i = same & (rep[i] == i), same & (rep[j] == j)
    shared[j[to_j]] = x[to_j]
    shared[i[to_i]] = x[to_i]
    own = rep == np.arange(n)
    shared[own] = card[own]
    rows = np.zeros(n, dtype=sp.CLUSTER_ROW_DTYPE)
    rows["cluster"], rows["representative"], rows["size"], rows["shared"] = number, rep, size[number], shared
    return rows, len(roots), int(edge.sum())


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
    """48 genomes in 8 families (blocks of six at mu = 0, 0.01, 0.03, 0, 0.01, 0.03: members 0 and 3 are both the unmutated
    ancestor) + 12 unrelated ones, 60 kbp each"""
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


def model_of(payloads, metric, num, den):
    """-> (rows, n_clusters, n_edges, card, cells) from the oracle's key sets"""
    sets = [key_set(p) for p in payloads]
    cells = [(i, j, len(sets[i] & sets[j])) for i in range(len(sets)) for j in range(i + 1, len(sets)) if sets[i] & sets[j]]
    card = [len(s) for s in sets]
    return cluster_model(card, cells, metric, num, den) + (card, cells)


@cached
def collection_model(k, m, metric, num, den):
    return model_of(collection(k, m, S), metric, num, den)


# ------------------------------------------------------------------------------------------------ not GPU

def test_model_on_hand_made_graphs():
    # a pair exactly at the threshold is linked, one key fewer is not: Jaccard 1/3 of two sketches of 100 keys is 50 shared
    for metric, num, den in ((JAC, 1, 3), (CON, 1, 2)):
        assert cluster_model([100, 100], [(0, 1, 50)], metric, num, den) == ([(0, 0, 2, 100), (0, 0, 2, 50)], 1, 1)
        assert cluster_model([100, 100], [(0, 1, 49)], metric, num, den) == ([(0, 0, 1, 100), (1, 1, 1, 100)], 2, 0)
    # the containment is the larger of the two: 30 of a sketch of 40 passes 3/4 whatever the other one holds
    assert cluster_model([1000, 40], [(0, 1, 30)], CON, 3, 4)[1:] == (1, 1) and cluster_model([1000, 40], [(0, 1, 30)], JAC, 3, 4)[1:] == (2, 0)
    # a chain a-b-c where a and c share nothing: one cluster, and the end that is not next to the representative shares 0
    rows, nc, ne = cluster_model([100, 90, 80], [(0, 1, 60), (1, 2, 55)], JAC, 1, 3)
    assert (rows, nc, ne) == ([(0, 0, 3, 100), (0, 0, 3, 60), (0, 0, 3, 0)], 1, 2)
    # ... and a cell below the threshold still tells `shared`
    assert cluster_model([100, 90, 80], [(0, 1, 60), (1, 2, 55), (0, 2, 7)], JAC, 1, 3)[0][2] == (0, 0, 3, 7)
    # the representative has the most keys; ties go to the first listed; numbering by first member
    rows, nc, _ = cluster_model([10, 50, 50, 10, 70, 50], [(1, 2, 50), (2, 5, 50), (0, 3, 10), (3, 4, 10)], CON, 1, 1)
    assert [r[:3] for r in rows] == [(0, 4, 3), (1, 1, 3), (1, 1, 3), (0, 4, 3), (0, 4, 3), (1, 1, 3)] and nc == 2
    assert rows[0][3] == 0 and rows[3][3] == 10 and rows[4][3] == 70 and rows[5][3] == 0
    # two empty sketches are two clusters; a cell of count 0 links nothing
    assert cluster_model([0, 0], [], JAC, 1, 1000000) == ([(0, 0, 1, 0), (1, 1, 1, 0)], 2, 0)
    assert cluster_model([5, 5], [(0, 1, 0)], CON, 1, 1000000)[1:] == (2, 0)


def test_the_array_model_is_the_model():
    rng = np.random.default_rng(3)
    for trial in range(40):
        n = int(rng.integers(1, 60))
        card = rng.integers(50, 100, n)
        pairs = sorted({(int(min(a, b)), int(max(a, b))) for a, b in rng.integers(0, n, (int(rng.integers(0, 3 * n)), 2)) if a != b})
        cells = [(i, j, int(rng.integers(0, min(card[i], card[j]) + 1))) for i, j in pairs]
        for metric, num, den in ((JAC, 1, 3), (CON, 1, 2), (JAC, 1, 1000000)):
            rows, nc, ne = cluster_model(card.tolist(), cells, metric, num, den)
            got, gc, ge = cluster_model_np(card, pack(cells) if cells else np.zeros(0, np.uint64), metric, num, den)
            assert (as_tuples(got), gc, ge) == (rows, nc, ne), (trial, metric)


def test_cluster_csv_equals_the_python_writer():
    names = ["a one.fa.gz", "dir/b.two", "c 3.sk.gz", "d.1.2.sketch", "e"]
    card = [1000, 700, 333, 12345, 3]
    rows = [(0, 3, 3, 300), (1, 1, 1, 700), (0, 3, 3, 0), (0, 3, 3, 12345), (2, 4, 1, 3)]
    for metric in (JAC, CON):
        for precision in (6, 3):
            assert sp.cluster_csv(as_rows(rows), names, card, metric, precision) == py_csv(rows, names, card, metric, precision)
        assert sp.cluster_csv(as_rows(rows), names, card, metric) == py_csv(rows, names, card, metric, 6)
    text = sp.cluster_csv(as_rows(rows), names, card, JAC).decode().splitlines()
    assert text[0] + "\n" == HEADER
    assert text[1] == "a one.fa.gz,0,d.1.2.sketch,3,1000,300,0.0229973" and text[3].endswith(",333,0,0")
    assert text[2] == "dir/b.two,1,dir/b.two,1,700,700,1" and text[4] == "d.1.2.sketch,0,d.1.2.sketch,3,12345,12345,1"
    assert sp.cluster_csv(as_rows(rows), names, card, CON, 3).decode().splitlines()[1].endswith(",300,0.3")
    # a representative beyond the list, and one outside its own cluster
    for bad in ((0, 5, 3, 300), (0, 1, 3, 300)):
        with pytest.raises(sp.SpspError) as e:
            sp.cluster_csv(as_rows([bad] + rows[1:]), names, card, JAC)
        assert e.value.code == sp.ERR_ARG


def test_abi_has_the_cluster_calls():
    assert {"spsp_cluster_cells_device", "spsp_cluster_csv_host", "spsp_cluster_files"} <= set(sp.ABI_SYMBOLS)
    assert ctypes.sizeof(sp.ClusterRow) == 24 == sp.CLUSTER_ROW_DTYPE.itemsize
    for name in ("spsp_cluster_cells_device", "spsp_cluster_csv_host", "spsp_cluster_files"):
        assert hasattr(sp.lib(), name)


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-c", "0.5", "-q", "list.txt"), ("-c", "0.5", "-C", "0.5"), ("-C", "0.5", "-g", "3", "-q", "list.txt")]
    cases += [("-c", t) for t in ("0", "1.5", "0.1234567", "abc", "", "0.", ".5", "-0.5", "1e-1", "0.5 ", "2")] + [("-C", "0.0000000")]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1, (args, r.stdout, r.stderr)
        assert "-c" in r.stdout or "-C" in r.stdout, (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


def test_the_collection_shows_what_it_is_there_for():
    """at both fractions the model's partition of the (31, 11) collection holds a chain (a cluster of three or more with two
    members not linked directly), a member that shares some but not all of its keys with its representative, at least 12
    clusters of one, and a representative tied in key count with another member of its cluster"""
    k, m = 31, 11
    pl = collection(k, m, S)
    assert pl[0] == pl[3]                                                   # the two unmutated copies of an ancestor
    for metric, num, den in FRACTIONS:
        rows, nc, ne, card, cells = collection_model(k, m, metric, num, den)
        x_of = {(i, j): x for i, j, x in cells}

        def linked(i, j):
            x = x_of.get((min(i, j), max(i, j)), 0)
            under = card[i] + card[j] - x if metric == JAC else min(card[i], card[j])
            return x >= 1 and x * den >= num * under
        groups = {}
        for i, r in enumerate(rows):
            groups.setdefault(r[0], []).append(i)
        assert any(len(g) >= 3 and any(not linked(a, b) for a in g for b in g if a < b) for g in groups.values()), metric
        assert any(0 < r[3] < card[i] for i, r in enumerate(rows)), metric
        assert sum(1 for g in groups.values() if len(g) == 1) >= 12, metric
        assert any(r[1] != i and card[r[1]] == card[i] for i, r in enumerate(rows)), metric
        assert rows[0][0] == 0 and rows[3][:3] == rows[0][:3] and card[3] == card[0]
        assert nc == len(groups) and ne == sum(1 for i, j, _ in cells if linked(i, j)) and 12 < nc < 60


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


def gpu_cluster(ctx, cells, card, metric, num, den):
    """cells: packed uint64 words on the host -> (rows, n_clusters, n_edges) of the device's clustering"""
    d = upload(cells) if len(cells) else None
    return ctx.cluster_cells_device(d.data_ptr() if d is not None else None, len(cells), card, len(card), metric, num, den)


def in_three_orders(ctx, cells, card, metric, num, den, want):
    """sorted, reversed and shuffled: the same rows and counts every time"""
    cells = np.sort(cells)
    rng = np.random.default_rng(len(cells))
    w_rows, w_nc, w_ne = want
    for order in (cells, cells[::-1], rng.permutation(cells)):
        rows, nc, ne = gpu_cluster(ctx, order, card, metric, num, den)
        assert (nc, ne) == (w_nc, w_ne)
        assert np.array_equal(rows, w_rows)


@pytest.mark.gpu
def test_a_path_over_all_nodes_under_a_random_permutation(ctx):
    """(a) deep trees, and the numbering by first member"""
    rng = np.random.default_rng(41)
    p = rng.permutation(NMAX).astype(np.uint64)
    card = 100 + (np.arange(NMAX) * 7919 % 13)
    a, b = np.minimum(p[:-1], p[1:]), np.maximum(p[:-1], p[1:])
    cells = a << np.uint64(48) | b << np.uint64(32) | np.uint64(95)
    want = cluster_model_np(card, cells, JAC, 1, 2)
    assert want[1:] == (1, NMAX - 1) and want[0]["size"][0] == NMAX and (want[0]["shared"] == 0).sum() > NMAX - 10
    in_three_orders(ctx, cells, card, JAC, 1, 2, want)
    # the same path cut in 1 000 places: 1 001 clusters numbered by their first member
    cut = cells.copy()
    at = rng.permutation(NMAX - 1)[:1000]
    cut[at] = (cut[at] & ~np.uint64(0xffffffff)) | np.uint64(10)            # (10 shared keys of 100 and more: below 1/2)
    want = cluster_model_np(card, cut, JAC, 1, 2)
    assert want[1:] == (1001, NMAX - 1 - 1000)
    in_three_orders(ctx, cut, card, JAC, 1, 2, want)


@pytest.mark.gpu
def test_a_star_with_its_centre_at_the_last_index(ctx):
    """(b) the root moves 65 534 times; equal key counts: sketch 0 represents, and only the centre touches it"""
    card = np.full(NMAX, 100)
    i = np.arange(NMAX - 1, dtype=np.uint64)
    cells = i << np.uint64(48) | np.uint64(NMAX - 1) << np.uint64(32) | (np.uint64(60) + i % np.uint64(30))
    want = cluster_model_np(card, cells, CON, 1, 2)
    rows = want[0]
    assert want[1:] == (1, NMAX - 1) and (rows["representative"] == 0).all() and rows["shared"][0] == 100
    assert rows["shared"][NMAX - 1] == 60 and not rows["shared"][1:NMAX - 1].any()
    in_three_orders(ctx, cells, card, CON, 1, 2, want)


@pytest.mark.gpu
def test_a_complete_graph_is_one_cluster(ctx):
    """(c) 1 999 000 cells that all fall into one component: contention on one root; every `shared` comes from its one cell"""
    n = 2000
    rng = np.random.default_rng(42)
    card = rng.integers(100, 120, n)
    card[1234] = 121
    i, j = np.triu_indices(n, 1)
    x = rng.integers(50, 101, len(i)).astype(np.uint64)
    cells = i.astype(np.uint64) << np.uint64(48) | j.astype(np.uint64) << np.uint64(32) | x
    assert len(cells) == 1_999_000
    want = cluster_model_np(card, cells, JAC, 1, 4)
    rows = want[0]
    assert want[1:] == (1, 1_999_000) and (rows["representative"] == 1234).all() and (rows["shared"] >= 50).all() and rows["shared"][1234] == 121
    in_three_orders(ctx, cells, card, JAC, 1, 4, want)


@pytest.mark.gpu
@pytest.mark.parametrize("metric,num,den", [(JAC, 1, 3), (CON, 1, 2)])
def test_random_cells_about_half_of_which_pass(ctx, metric, num, den):
    """(d) many components of every size, and n_edges"""
    rng = np.random.default_rng(43 + metric)
    card = rng.integers(500, 1000, NMAX)
    pairs = rng.integers(0, NMAX, (210_000, 2))
    a, b = pairs.min(1), pairs.max(1)
    keep = np.unique(a[a != b] * 65536 + b[a != b])[:200_000]
    rng.shuffle(keep)
    a, b = keep // 65536, keep % 65536
    assert len(keep) == 200_000
    x = (rng.random(len(a)) * np.minimum(card[a], card[b])).astype(np.uint64) + np.uint64(1)
    cells = a.astype(np.uint64) << np.uint64(48) | b.astype(np.uint64) << np.uint64(32) | x
    want = cluster_model_np(card, cells, metric, num, den)
    assert 60_000 < want[2] < 140_000 and 1000 < want[1] < 40_000 and want[0]["size"].max() > 1000
    in_three_orders(ctx, cells, card, metric, num, den, want)


def no_cells(ctx, n):
    card = list(range(5, 5 + n))
    rows, nc, ne = gpu_cluster(ctx, np.zeros(0, np.uint64), card, JAC, 1, 2)
    assert (as_tuples(rows), nc, ne) == ([(i, i, 1, card[i]) for i in range(n)], n, 0)


@pytest.mark.gpu
def test_no_cells_give_clusters_of_one(ctx):
    """(e)"""
    no_cells(ctx, 1)
    no_cells(ctx, 70)
    rows, nc, ne = gpu_cluster(ctx, pack([(0, 1, 0)]), [0, 0], CON, 1, 1000000)   # two empty sketches, even with a cell that names them
    assert (as_tuples(rows), nc, ne) == ([(0, 0, 1, 0), (1, 1, 1, 0)], 2, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("metric,num,den", [(JAC, 1, 3), (CON, 1, 2)])
def test_two_cliques_joined_by_one_cell_at_the_threshold(ctx, metric, num, den):
    """(f) 50 shared keys of 100 and 100 are exactly 1/3 (Jaccard) and 1/2 (containment): one cluster; 49: two"""
    card = [100] * 12
    clique = lambda lo: [(i, j, 80) for i in range(lo, lo + 6) for j in range(i + 1, lo + 6)]
    for x, n_clusters in ((50, 1), (49, 2)):
        cells = clique(0) + clique(6) + [(4, 9, x)]
        want = cluster_model(card, cells, metric, num, den)
        assert want[1:] == (n_clusters, 30 + (x == 50))
        words = pack(cells)
        for order in (words, words[::-1], np.random.default_rng(x).permutation(words)):
            rows, nc, ne = gpu_cluster(ctx, order, card, metric, num, den)
            assert (as_tuples(rows), nc, ne) == want


@pytest.mark.gpu
def test_representatives_ties_and_large_key_counts(ctx):
    """(g) equal key counts in one component: the first listed represents; the member with the most keys does wherever it
    is listed; key counts up to 2^47 - 1 take part without a product leaving 64 bits"""
    card = [10, 50, 50, 10, 70, 50, 33]
    cells = [(1, 2, 50), (2, 5, 50), (0, 3, 10), (3, 4, 10)]
    want = cluster_model(card, cells, CON, 1, 1)
    assert [r[1] for r in want[0]] == [4, 1, 1, 4, 4, 1, 6]
    rows, nc, ne = gpu_cluster(ctx, pack(cells), card, CON, 1, 1)
    assert (as_tuples(rows), nc, ne) == want
    big = (1 << 47) - 1
    card = [big, big, 1 << 46, 4_000_000_000, 4_000_000_000]
    cells = [(0, 1, 0xffffffff), (1, 2, 1 << 31), (3, 4, 3_999_999_999), (2, 3, 2_000_000_000)]
    for metric, num, den in ((JAC, 1000000, 1000000), (JAC, 1, 1000000), (CON, 1, 1000000), (CON, 999999, 1000000), (CON, 1, 2)):
        want = cluster_model(card, cells, metric, num, den)
        rows, nc, ne = gpu_cluster(ctx, pack(cells), card, metric, num, den)
        assert (as_tuples(rows), nc, ne) == want, (metric, num, den)


@pytest.mark.gpu
def test_bad_cells_and_bad_arguments_are_refused(ctx):
    """(h) a cell with j == n, one with i == j, one with i > j: ERR_ARG, and the context answers (e) afterwards"""
    card = [100] * 10
    good = [(0, 1, 80), (2, 3, 80)]
    for bad in ((3, 10, 80), (4, 4, 80), (7, 2, 80), (65535, 65535, 1)):
        with pytest.raises(sp.SpspError) as e:
            gpu_cluster(ctx, pack(good + [bad] + good), card, JAC, 1, 2)
        assert e.value.code == sp.ERR_ARG and "cell" in str(e.value)
        no_cells(ctx, 1)
        no_cells(ctx, 70)
    cells = upload(pack(good))
    call = lambda n=10, metric=JAC, num=1, den=2, c=card: ctx.cluster_cells_device(cells.data_ptr(), 2, c[:n] if n <= len(c) else c + [1] * (n - len(c)), n, metric, num, den)
    for kw in (dict(n=0), dict(n=65536), dict(metric=2), dict(metric=-1), dict(num=0), dict(num=3), dict(num=1000001, den=1000001),
               dict(den=1000001), dict(c=[100] * 9 + [1 << 47])):
        with pytest.raises(sp.SpspError) as e:
            call(**kw)
        assert e.value.code == sp.ERR_ARG, kw
    rows, nc, ne = call()
    assert (as_tuples(rows), nc, ne) == cluster_model(card, good, JAC, 1, 2)
    rows, nc, ne = call(num=1000000, den=1000000)
    assert (nc, ne) == (10, 0)


def gpu_collection(ctx, payloads, metric, num, den):
    """decode, the all-vs-all as cells, the cluster pass -> (rows, n_clusters, n_edges, card)"""
    import torch
    n = len(payloads)
    k, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
    scratch = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    cells = torch.zeros(n * n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cnt = ctx.compare_cells_device(k, d_mn, d_lo, d_hi, off, n, scratch.data_ptr(), cells.data_ptr(), cells.numel())
    card = np.diff(off.astype(np.int64)).tolist()
    return ctx.cluster_cells_device(cells.data_ptr(), cnt, card, n, metric, num, den) + (card,)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", KM)
def test_the_family_collection_from_sketches_to_clusters(ctx, k, m):
    pl = collection(k, m, S)
    for metric, num, den in FRACTIONS:
        want, w_nc, w_ne, w_card, _ = collection_model(k, m, metric, num, den)
        rows, nc, ne, card = gpu_collection(ctx, pl, metric, num, den)
        assert card == w_card and (as_tuples(rows), nc, ne) == (want, w_nc, w_ne), metric


@pytest.mark.gpu
def test_the_files_in_another_order_give_the_same_partition(ctx):
    k, m = 31, 11
    pl = collection(k, m, S)
    perm = np.random.default_rng(44).permutation(len(pl)).tolist()          # shuffled[t] = pl[perm[t]]
    shuffled = [pl[t] for t in perm]
    for metric, num, den in FRACTIONS:
        want, _, w_ne, card, _ = collection_model(k, m, metric, num, den)
        rows, nc, ne, s_card = gpu_collection(ctx, shuffled, metric, num, den)
        model = model_of(shuffled, metric, num, den)
        assert (as_tuples(rows), nc, ne) == model[:3] and ne == w_ne
        part = lambda rs, back: sorted(sorted(back[i] for i, r in enumerate(rs) if r[0] == c) for c in {r[0] for r in rs})
        assert part(as_tuples(rows), perm) == part(want, list(range(len(pl))))
        for t, r in enumerate(as_tuples(rows)):
            # the representative is the same sketch, or one tied with it in key count (the tie rule follows the list order)
            assert card[perm[r[1]]] == card[want[perm[t]][1]] and r[2] == want[perm[t]][2]
            assert s_card[r[1]] == max(s_card[u] for u, q in enumerate(as_tuples(rows)) if q[0] == r[0])


def write_files(root, payloads, tag="f"):
    paths = []
    for i, p in enumerate(payloads):
        paths.append(os.path.join(str(root), "%s %03d.sk.gz" % (tag, i)))  # (names with a space and dots)
        sp.write_gz(paths[-1], p, 1)
    return paths


def gunzip(path):
    return gzip.open(path, "rb").read()


@pytest.mark.gpu
def test_cluster_files_and_the_command_line(ctx, tmp_path):
    k, m = 31, 11
    pl = collection(k, m, S)
    paths = write_files(tmp_path, pl)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    for (metric, num, den), flag, t in zip(FRACTIONS, ("-c", "-C"), ("0.5", "0.60")):
        want, w_nc, w_ne, card, _ = collection_model(k, m, metric, num, den)
        text = py_csv(want, paths, card, metric)
        rows, nc = ctx.cluster_files(paths, str(tmp_path / "lib"), metric, num, den)
        assert as_tuples(rows) == want and nc == w_nc
        assert gunzip(str(tmp_path / "lib_clusters.csv.gz")) == text
        rows, nc = ctx.cluster_files(paths, str(tmp_path / "p3"), metric, num, den, precision=3)
        assert as_tuples(rows) == want and gunzip(str(tmp_path / "p3_clusters.csv.gz")) == py_csv(want, paths, card, metric, 3)
        r = run(flag, t, "-f", "list.txt", "-o", "cli")
        assert r.returncode == 0, r.stdout + r.stderr
        assert gunzip(str(tmp_path / "cli_clusters.csv.gz")) == text
        out = r.stdout.splitlines()
        assert out[:2] == ["No query file, I will perform a all versus all comparison", "I found %d documents" % len(pl)]
        assert out[2] == "kmers evaluated are of length: %d minimizer size is %d" % (k, m)
        assert out[3] == "%d sketches, %d edges, %d clusters, the largest of %d" % (len(pl), w_ne, w_nc, max(x[2] for x in want)) and len(out) == 4
        os.remove(str(tmp_path / "cli_clusters.csv.gz"))
    assert not [f for f in os.listdir(tmp_path) if "_jaccard" in f or "_containment" in f or "_gather" in f]
    # without -c / -C: the two matrices, as before
    r = run("-f", "list.txt", "-o", "plain")
    assert r.returncode == 0, r.stdout + r.stderr
    inter, c2, _, _ = orc.compare(pl)
    for jac, suf in ((True, "_jaccard.csv.gz"), (False, "_containment.csv.gz")):
        assert gunzip(str(tmp_path / ("plain" + suf))) == orc.csv(jac, paths, inter, c2, None, 6, 0.0)
    assert not os.path.exists(str(tmp_path / "plain_clusters.csv.gz"))


@pytest.mark.gpu
def test_cluster_files_at_a_common_rate(ctx, tmp_path):
    """some files at -s 10, the others at -s 100, rate="auto": the clustering of the -s 100 sketches of the same genomes"""
    k, m = 31, 11
    coarse, fine = collection(k, m, S), collection(k, m, 10.0)
    mixed = [fine[i] if i % 3 == 1 else coarse[i] for i in range(len(coarse))]
    paths = write_files(tmp_path, mixed)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    metric, num, den = FRACTIONS[0]
    want, w_nc, w_ne, card, _ = collection_model(k, m, metric, num, den)
    for tag, rate in (("auto", "auto"), ("r100", 100)):
        rows, nc = ctx.cluster_files(paths, str(tmp_path / tag), metric, num, den, rate=rate)
        assert as_tuples(rows) == want and nc == w_nc
        assert gunzip(str(tmp_path / (tag + "_clusters.csv.gz"))) == py_csv(want, paths, card, metric)
    # as the files are: another question with another answer
    asis = model_of(mixed, metric, num, den)
    rows, nc = ctx.cluster_files(paths, str(tmp_path / "asis"), metric, num, den)
    assert as_tuples(rows) == asis[0] and nc == asis[1] and asis[0] != want
    assert gunzip(str(tmp_path / "asis_clusters.csv.gz")) == py_csv(asis[0], paths, asis[3], metric)
    # the command line with -s auto, and its common-rate line
    r = subprocess.run([EXE, "-c", "0.5", "-s", "auto", "-f", "list.txt", "-o", "cli"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert gunzip(str(tmp_path / "cli_clusters.csv.gz")) == py_csv(want, paths, card, metric)
    assert r.stdout.splitlines()[3:] == ["60 sketches, %d edges, %d clusters, the largest of %d" % (w_ne, w_nc, max(x[2] for x in want)),
                                          "Sketches compared at sampling rate 100: 20 of 60 brought down to it"]
    # a file coarser than the asked rate: refused, naming it
    with pytest.raises(sp.SpspError) as e:
        ctx.cluster_files(paths, str(tmp_path / "no"), metric, num, den, rate=10)
    assert e.value.code == sp.ERR_ARG and os.path.basename(paths[0]) in str(e.value) and "upsample" in str(e.value)
    # k == m: refused with and without a rate
    kk = [orc.sketch_fasta(synth.to_fasta(g[:5000], "g%d" % i), 11, 11, S)[0] for i, g in enumerate(_genomes()[:3])]
    p3 = write_files(tmp_path, kk, "kk")
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.cluster_files(p3, str(tmp_path / "no"), metric, num, den, rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    for kw in (dict(metric=2), dict(num=0), dict(num=3, den=2), dict(den=1000001)):
        with pytest.raises(sp.SpspError) as e:
            ctx.cluster_files(paths, str(tmp_path / "no"), **dict(dict(metric=metric, num=num, den=den), **kw))
        assert e.value.code == sp.ERR_ARG, kw
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no")]


@pytest.mark.gpu
def test_cluster_files_of_a_thousand_sketches_and_one_without_keys(ctx, tmp_path):
    """n >= 1024: the cells leave the row sums directly; the room first offered (65 536 cells) is too small for
    families of 160, so the comparison is repeated; a sketch without buckets is a cluster of one"""
    n = 1100
    D = synth.direct_family_sketches(n, fam_size=160, seed=12, skm_range=(6, 10))
    pl = [D.payload(i) for i in range(n)]
    pl[500] = orc.sketch_fasta(synth.to_fasta(synth.random_genome(np.random.default_rng(9), 20), "short"), 31, 11, 1000.0)[0]
    assert pl[500].count(b"\n") == 1
    paths = write_files(tmp_path, pl, "d")
    inter, card, _, _ = orc.compare(pl)
    i, j = np.nonzero(np.triu(inter, 1))
    cells = i.astype(np.uint64) << np.uint64(48) | j.astype(np.uint64) << np.uint64(32) | inter[i, j].astype(np.uint64)
    assert len(cells) > 65536 and card[500] == 0
    for metric, num, den in ((JAC, 1, 4), (CON, 1, 2)):
        want, w_nc, _ = cluster_model_np(card, cells, metric, num, den)
        assert 1 < w_nc < n and want["size"].max() > 2
        rows, nc = ctx.cluster_files(paths, str(tmp_path / "big"), metric, num, den)
        assert np.array_equal(rows, want) and nc == w_nc and as_tuples(rows)[500][1:] == (500, 1, 0)
        assert gunzip(str(tmp_path / "big_clusters.csv.gz")) == py_csv(as_tuples(want), paths, [int(c) for c in card], metric)


@pytest.mark.gpu
def test_twice_on_one_context(ctx):
    """a larger problem, then a smaller one: the reused work buffers leave nothing behind"""
    rng = np.random.default_rng(45)
    n = 5000
    card = rng.integers(100, 200, n)
    keep = np.unique(np.sort(rng.integers(0, n, (30_000, 2)), axis=1), axis=0)
    keep = keep[keep[:, 0] != keep[:, 1]]
    x = (rng.random(len(keep)) * np.minimum(card[keep[:, 0]], card[keep[:, 1]])).astype(np.uint64) + np.uint64(1)
    cells = keep[:, 0].astype(np.uint64) << np.uint64(48) | keep[:, 1].astype(np.uint64) << np.uint64(32) | x
    want = cluster_model_np(card, cells, JAC, 1, 3)
    rows, nc, ne = gpu_cluster(ctx, cells, card, JAC, 1, 3)
    assert np.array_equal(rows, want[0]) and (nc, ne) == want[1:]
    pl = collection(31, 11, S)
    metric, num, den = FRACTIONS[0]
    small, s_nc, s_ne, s_card, _ = collection_model(31, 11, metric, num, den)
    rows, nc, ne, card2 = gpu_collection(ctx, pl, metric, num, den)
    assert (as_tuples(rows), nc, ne) == (small, s_nc, s_ne)
    no_cells(ctx, 70)
    rows, nc, ne = gpu_cluster(ctx, cells, card, JAC, 1, 3)
    assert np.array_equal(rows, want[0]) and (nc, ne) == want[1:]
