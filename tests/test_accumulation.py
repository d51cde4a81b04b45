"""Accumulation: pan and core curves of a collection over orders of its sketches (spsp_accumulation_device and what stands
around it).  Every expected value comes from `model`: literal unions and intersections of the prefixes of an order, Python sets
and Python integers -- not the first / mex form the kernels count by, so the two derivations check each other.  No tolerance
anywhere: every curve is a count of keys.

The GPU tests pass orders of their own and compare every order's two curves AND the rows.  Keys are hand-built (minimizer,
kmer_hi, kmer_lo) arrays uploaded with torch, shaped to sit on the seams of the pass: the list length at which a lane hands a
list to its wave, the 64-bit mask of a lane's mex, the bitmap a wave marks a long list's ranks in, the window of ranks of the
first-rank histogram, the number of orders one pass serves, the 2 048-entry tiles of the scans, and the table with every slot
taken (SPSP_DEBUG_PREVALENCE_TABLE=min)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
import test_prevalence as tp
from supersampler_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
HEADER = "genomes,pan_min,pan_mean,pan_max,core_min,core_mean,core_max,new_mean,pan_listed,core_listed\n"
FIELDS = ("pan_min", "pan_max", "pan_sum", "core_min", "core_max", "core_sum", "pan_first", "core_first")
U64 = (1 << 64) - 1
REDRAW_SEED = 3558559446808474027          # splitmix64's first draw from this state is 2^64 - 1 (the mixer run backwards)


# -------------------------------------------------------------------------------------------------- the model

def model(sets, orders):
    """-> (pan, core): per order the sizes of the union and of the intersection of its first j sketches, j = 1 .. n"""
    pan, core = [], []
    for o in orders:
        union, common, pu, pc = set(), None, [], []
        for s in o:
            union |= sets[s]
            common = set(sets[s]) if common is None else common & sets[s]
            pu.append(len(union))
            pc.append(len(common))
        pan.append(pu)
        core.append(pc)
    return pan, core


def rows_of(pan, core):
    """the curves of P orders -> one tuple per step in the order of spsp_accumulation_row's fields"""
    return [(min(p), max(p), sum(p), min(c), max(c), sum(c), p[0], c[0]) for p, c in zip(zip(*pan), zip(*core))]


def py_orders(n, P, seed):
    """the rule of include/spsp.h: order 0 the identity, then Fisher-Yates shuffles from one splitmix64 stream -> (orders, redraws)"""
    state, redraws, out = [seed], [0], []

    def draw():
        state[0] = (state[0] + 0x9E3779B97F4A7C15) & U64
        z = state[0]
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & U64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & U64
        return z ^ (z >> 31)

    for p in range(P):
        a = list(range(n))
        for i in range(n - 1, 0, -1) if p else ():
            z = draw()
            while z >= (1 << 64) - (1 << 64) % (i + 1):
                redraws[0] += 1
                z = draw()
            j = z % (i + 1)
            a[i], a[j] = a[j], a[i]
        out.append(a)
    return out, redraws[0]


def py_csv(rows, P, precision=6):
    text, before = HEADER, 0
    g = lambda v: "%.*g" % (precision, v)
    for j, (pmin, pmax, psum, cmin, cmax, csum, pfirst, cfirst) in enumerate(rows, 1):
        text += "%d,%d,%s,%d,%d,%s,%d,%s,%d,%d\n" % (j, pmin, g(psum / P), pmax, cmin, g(csum / P), cmax, g((psum - before) / P), pfirst, cfirst)
        before = psum
    return text.encode()


def as_rows(tuples):
    out = np.zeros(len(tuples), dtype=sp.ACCUMULATION_ROW_DTYPE)
    for i, t in enumerate(tuples):
        out[i] = t
    return out


def as_tuples(rows):
    return [tuple(int(r[f]) for f in FIELDS) for r in rows]


# ------------------------------------------------------------------------------------------------ not GPU

def K(*xs):
    return {(x, 0, x) for x in xs}


def test_model_on_a_hand_made_case():
    # key 1 in all four, key 2 in 0 1 2, key 3 in 0 and 3, keys 10 + j in sketch j alone
    sets = [K(1, 2, 3, 10), K(1, 2, 11), K(1, 2, 12), K(1, 3, 13)]
    pan, core = model(sets, [[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2]])
    assert pan == [[4, 5, 6, 7], [3, 5, 6, 7], [3, 5, 6, 7]]
    assert core == [[4, 2, 2, 1], [3, 1, 1, 1], [3, 1, 1, 1]]
    assert rows_of(pan, core) == [(3, 4, 10, 3, 4, 10, 4, 4), (5, 5, 15, 1, 2, 4, 5, 2), (6, 6, 18, 1, 2, 4, 6, 2), (7, 7, 21, 1, 1, 3, 7, 1)]
    assert py_csv(rows_of(pan, core), 3, 3).decode() == HEADER + ("1,3,3.33,4,3,3.33,4,3.33,4,4\n2,5,5,5,1,1.33,2,1.67,5,2\n"
                                                                 "3,6,6,6,1,1.33,2,1,6,2\n4,7,7,7,1,1,1,1,7,1\n")
    assert model([set(), K(1)], [[0, 1], [1, 0]]) == ([[0, 1], [1, 1]], [[0, 0], [1, 0]])


def test_abi_has_the_accumulation_calls():
    calls = ("spsp_accumulation_orders_host", "spsp_accumulation_plan_host", "spsp_accumulation_device", "spsp_accumulation_csv_host",
             "spsp_accumulation_files")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    for name in calls:
        assert hasattr(sp.lib(), name)
    assert hasattr(sp.Context, "accumulation_device") and hasattr(sp.Context, "accumulation_files")
    assert callable(sp.accumulation_orders) and callable(sp.accumulation_csv) and sp.ACCUMULATION_ROW_DTYPE.itemsize == 64
    assert sp.ACCUMULATION_ROW_DTYPE.names == FIELDS


@pytest.mark.parametrize("n", [1, 2, 3, 1000])
def test_orders_are_the_python_restatement(n):
    for P in (1, 2, 33):
        for seed in (1, 2, U64, REDRAW_SEED):
            got = sp.accumulation_orders(n, P, seed)
            want, _ = py_orders(n, P, seed)
            assert got.shape == (P, n) and got.tolist() == want, (P, seed)
            assert got[0].tolist() == list(range(n)) and all(sorted(o) == list(range(n)) for o in got.tolist())
    assert sp.accumulation_orders(n, 33, 5).tolist() == sp.accumulation_orders(n, 33, 5).tolist()            # one seed repeats
    if n > 2:
        assert sp.accumulation_orders(n, 33, 5).tolist() != sp.accumulation_orders(n, 33, 6).tolist()        # two seeds differ


def test_a_bound_that_draws_again():
    # the first draw from REDRAW_SEED is the largest word: below(3) has 2^64 mod 3 = 1 word too many, and this is it
    for n in (3, 1000):
        want, redraws = py_orders(n, 2, REDRAW_SEED)
        assert redraws >= 1 and sp.accumulation_orders(n, 2, REDRAW_SEED).tolist() == want
    # a power of two divides 2^64: the same word is taken there (below(2) of n = 2)
    want, redraws = py_orders(2, 2, REDRAW_SEED)
    assert redraws == 0 and sp.accumulation_orders(2, 2, REDRAW_SEED).tolist() == want
    for n, P in ((0, 1), (65536, 1), (1, 0), (1, 1025)):
        with pytest.raises(sp.SpspError) as e:
            sp.accumulation_orders(n, P, 1)
        assert e.value.code == sp.ERR_ARG


def test_the_plan_follows_its_formula():
    """include/spsp.h: 160 KiB less a bitmap per wave; an order costs its rank table and 4 bytes per rank of the window"""
    budget = 160 * 1024 - 8 * (8192 // 8)
    for n in (1, 2, 63, 64, 3242, 3243, 6485, 6486, 10_000, 12_970, 12_971, 25_941, 25_942, 40_000, 65_534, 65_535):
        plan = sp.accumulation_plan(n)
        rank = 2 * ((n + 1) & ~1)
        fit = budget // (rank + 4 * n)
        want = (max(g for g in (1, 2, 4, 8) if g <= fit), n) if fit else (1, (budget - rank) // 4)
        assert (plan["group"], plan["window"]) == want and plan["bitmap_bits"] == 8192 and 1 <= plan["cut"] <= 64, n
    assert sp.accumulation_plan(10_000)["group"] == 2 and sp.accumulation_plan(25_942)["window"] == 25_941 and sp.accumulation_plan(65_535)["window"] == 6144


GOOD = [(10, 12, 22, 10, 12, 22, 10, 10), (15, 15, 30, 4, 7, 11, 15, 7), (16, 16, 32, 3, 3, 6, 16, 3)]


@pytest.mark.parametrize("precision", [1, 6, 17])
def test_the_csv_is_the_python_formatter_byte_for_byte(precision):
    assert sp.accumulation_csv(as_rows(GOOD), 2, precision) == py_csv(GOOD, 2, precision)
    rng = np.random.default_rng(precision)
    for P in (1, 3, 7, 1024):
        n = 40
        pan = [np.sort(rng.integers(0, 10 ** 7, n)).tolist() for _ in range(P)]
        core = [np.sort(rng.integers(0, 10 ** 7, n))[::-1].tolist() for _ in range(P)]
        rows = rows_of(pan, core)
        text = sp.accumulation_csv(as_rows(rows), P, precision)
        assert text == py_csv(rows, P, precision) and text.count(b"\n") == n + 1


def test_the_csv_refuses_what_is_no_curve():
    def spoilt(row, **changes):
        rows = [dict(zip(FIELDS, t)) for t in GOOD]
        rows[row].update(changes)
        return as_rows([tuple(r[f] for f in FIELDS) for r in rows])
    bad = [spoilt(0, pan_min=13), spoilt(1, core_min=8), spoilt(0, pan_sum=25), spoilt(0, pan_sum=19), spoilt(1, core_sum=15), spoilt(1, core_sum=7),
           spoilt(1, pan_min=9, pan_sum=24, pan_first=9), spoilt(2, core_max=8, core_sum=11), spoilt(0, pan_first=13), spoilt(0, pan_first=9),
           spoilt(1, core_first=3), spoilt(1, core_first=8)]
    for rows in bad:
        with pytest.raises(sp.SpspError) as e:
            sp.accumulation_csv(rows, 2)
        assert e.value.code == sp.ERR_ARG and "accumulation row" in str(e.value)
    for P in (0, 1025):
        with pytest.raises(sp.SpspError) as e:
            sp.accumulation_csv(as_rows(GOOD), P)
        assert e.value.code == sp.ERR_ARG
    assert sp.accumulation_csv(spoilt(0, pan_max=U64, pan_sum=U64), 2).startswith(HEADER.encode())      # (P * max is weighed beyond 64 bits)


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-A", "0"), ("-A", "1025"), ("-A", "-3"), ("-A", "seven"), ("-A", ""), ("-z", "3"), ("-A", "7", "-z", "-1"), ("-A", "7", "-z", "x")]
    cases += [("-A", "7") + other for other in (("-q", "list.txt"), ("-P", "0.5"), ("-S", "union"), ("-E", "union"), ("-g", "3", "-q", "list.txt"),
                                                ("-c", "0.5"), ("-C", "0.5"), ("-N", "5"), ("-r", "0.5"), ("-R", "0.5"), ("-l", "0.5"), ("-L", "0.5"))]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and ("-A" in r.stdout or "-z" in r.stdout), (args, r.stdout, r.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


def test_host_functions_under_the_sanitizers():
    """tests/tools/accumulation_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs
    the order generator, the plan and the CSV writer (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "accumulation_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "accumulation host functions OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def from_holders(n, holders, k, salt=0):
    """holders[x] = the sketches that hold key x -> n lists of key tuples"""
    keys = tp.pool(len(holders), k, salt)
    sketches = [[] for _ in range(n)]
    for key, hs in zip(keys, holders):
        for s in hs:
            sketches[s].append(key)
    return sketches


def curves(ctx, sketches, k, orders):
    """-> (rows as tuples, pan, core as lists per order, the sketches as sorted lists)"""
    mn, lo, hi, off, order = tp.pack(sketches, k)
    d = tp.upload(mn, lo, hi)
    rows, pan, core = ctx.accumulation_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, len(order), np.array(orders, dtype=np.uint32).reshape(len(orders), -1),
                                              want_curves=True)
    del d
    return as_tuples(rows), pan.tolist(), core.tolist(), order


def check(ctx, sketches, k, orders, want=None):
    rows, pan, core, order = curves(ctx, sketches, k, orders)
    w_pan, w_core = want if want is not None else model([set(s) for s in order], orders)
    for p in range(len(orders)):
        assert pan[p] == w_pan[p], ("pan", p, [j for j, (a, b) in enumerate(zip(pan[p], w_pan[p])) if a != b][:8])
        assert core[p] == w_core[p], ("core", p, [j for j, (a, b) in enumerate(zip(core[p], w_core[p])) if a != b][:8])
    assert rows == rows_of(w_pan, w_core)
    return w_pan, w_core


def shuffles(n, P, seed):
    return py_orders(n, P, seed)[0] if n < 3000 else sp.accumulation_orders(n, P, seed).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_smallest_collections(ctx, k):
    keys = tp.pool(12, k)
    # one sketch: pan = core = its keys, whatever the number of orders
    for P in (1, 2, 9):
        assert check(ctx, [keys[:5]], k, [[0]] * P) == ([[5]] * P, [[5]] * P)
    # two sketches, both orders: core(2) is what they share, pan(2) + core(2) = c_0 + c_1
    pan, core = check(ctx, [keys[:7], keys[4:12]], k, [[0, 1], [1, 0]])
    assert pan == [[7, 12], [8, 12]] and core == [[7, 3], [8, 3]]
    # a sketch without keys first, in the middle and last: core is 0 from its step on, pan does not move at its step
    for at in (0, 1, 2):
        sketches = [keys[:7], keys[4:12]]
        sketches.insert(at, [])
        pan, core = check(ctx, sketches, k, [[0, 1, 2], [2, 1, 0], [1, 0, 2], [1, 2, 0]])
        for o, p, c in zip([[0, 1, 2], [2, 1, 0], [1, 0, 2], [1, 2, 0]], pan, core):
            j = o.index(at)
            assert c[j:] == [0] * (3 - j) and p[j] == (p[j - 1] if j else 0)
    # no key anywhere
    assert check(ctx, [[], [], []], k, [[0, 1, 2], [2, 0, 1]]) == ([[0, 0, 0]] * 2, [[0, 0, 0]] * 2)
    assert check(ctx, [[]], k, [[0]]) == ([[0]], [[0]])


@pytest.mark.gpu
def test_one_key_around_the_cut_and_the_mask(ctx):
    """one key held by exactly h of n sketches: a lane's list up to the cut, the wave's beyond it; h = 64 among n = 64 is a full
    64-bit mask (mex = 64), h = 65 the first list of two rounds of a wave"""
    k, cut = 31, sp.accumulation_plan(100)["cut"]
    for h in sorted({1, 2, 63, 64, 65, cut - 1, cut, cut + 1}):
        # n = h: nobody is missing
        n = h
        orders = [list(range(n)), list(range(n))[::-1]] + shuffles(n, 3, h)[1:]
        pan, core = check(ctx, from_holders(n, [range(h)], k), k, orders)
        assert all(p == [1] * n and c == [1] * n for p, c in zip(pan, core))
        # n = h + 1: the sketch without the key last (rank h), first, and in the middle
        n, missing = h + 1, h
        orders = [list(range(n)), [missing] + list(range(h)), list(range(h // 2)) + [missing] + list(range(h // 2, h))] + shuffles(n, 3, h)[1:]
        pan, core = check(ctx, from_holders(n, [range(h)], k), k, orders)
        assert core[0] == [1] * h + [0] and core[1] == [0] * n and pan[1] == [0] + [1] * h
        assert core[2] == [1] * (h // 2) + [0] * (n - h // 2)


@pytest.mark.gpu
@pytest.mark.parametrize("long_ones", [1, 5, 64, 200])
def test_short_and_long_lists_side_by_side(ctx, long_ones):
    """200 keys of which one, several, a wave's worth or all have lists beyond the cut; the others 1 .. cut holders"""
    k, n, cut = 31, 80, sp.accumulation_plan(80)["cut"]
    rng = np.random.default_rng(long_ones)
    is_long = np.zeros(200, bool)
    is_long[rng.choice(200, long_ones, replace=False)] = True
    holders = [rng.choice(n, int(rng.integers(cut + 1, n + 1)) if is_long[x] else int(rng.integers(1, cut + 1)), replace=False).tolist() for x in range(200)]
    holders[int(np.argmax(is_long))] = list(range(n))                                # one of the long ones is everybody's
    check(ctx, from_holders(n, holders, k), k, shuffles(n, 9, 17))


@pytest.mark.gpu
def test_the_bitmap_pass_boundary(ctx):
    """a key of everybody and keys of everybody but the sketch at rank B - 1, B, B + 1 (and 2 B - 1, 2 B, 2 B + 1) among n = 2 B + 3
    sketches: the least missing rank is the last bit of a pass, the first of the next, or there is none"""
    k, B = 31, sp.accumulation_plan(100)["bitmap_bits"]
    n = 2 * B + 3
    assert B == 8192
    gaps = [B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1]
    everybody = list(range(n))
    holders = [everybody] + [[s for s in everybody if s != g] for g in gaps]
    identity = list(range(n))
    orders = [identity, identity[1:] + identity[:1], identity[-1:] + identity[:-1]]    # ranks as numbered, one lower, one higher
    pan, core = check(ctx, from_holders(n, holders, k), k, orders)
    assert core[0][B - 2:B + 2] == [7, 6, 5, 4] and core[0][-1] == 1 and pan[0] == [7] * n


@pytest.mark.gpu
def test_the_histogram_windows(ctx):
    """a key per sketch alone, so that every rank's bin is hit, and one key of everybody, at the n where one window stops holding
    every rank (and one below, at it, one and two above)"""
    k = 31
    lo, hi = 1, 65535
    while lo < hi:                                                                   # the largest n whose window is all of its ranks
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if sp.accumulation_plan(mid)["window"] == mid else (lo, mid - 1)
    edge = lo
    assert sp.accumulation_plan(edge + 1)["window"] == edge and sp.accumulation_plan(edge + 1)["group"] == 1
    for n in (edge - 1, edge, edge + 1, edge + 2):
        ident = np.arange(n)
        orders = np.stack([ident, ident[::-1], sp.accumulation_orders(n, 2, n)[1]])
        steps = np.arange(1, n + 1)
        want_pan = [(steps + 1).tolist()] * 3                                        # j keys of their own and everybody's
        want_core = [[2] + [1] * (n - 1)] * 3
        check(ctx, from_holders(n, [[s] for s in range(n)] + [range(n)], k), k, orders.tolist(), (want_pan, want_core))


@pytest.mark.gpu
def test_the_largest_collection(ctx):
    """n = 65 535: a 128 KiB rank table, one order per pass, eleven windows.  One key each, one of everybody, one of all but one;
    the model follows from that structure: pan(j) = j + 1 + [somebody among the first j holds the third key]"""
    k, n, odd = 31, 65535, 40_000
    assert sp.accumulation_plan(n) == {"group": 1, "window": 6144, "bitmap_bits": 8192, "cut": sp.accumulation_plan(1)["cut"]}
    ident = np.arange(n)
    orders = np.stack([ident, ident[::-1], sp.accumulation_orders(n, 2, 9)[1]])
    steps = np.arange(1, n + 1)
    want_pan, want_core = [], []
    for o in orders:
        rank = int(np.nonzero(o == odd)[0][0])                                       # where the sketch without the third key stands
        want_pan.append((steps + 1 + ((steps >= 2) | (rank != 0))).tolist())
        want_core.append(np.where(steps == 1, 2 + (rank != 0), 1 + (steps <= rank)).tolist())
    sketches = from_holders(n, [[s] for s in range(n)] + [range(n), [s for s in range(n) if s != odd]], k)
    check(ctx, sketches, k, orders.tolist(), (want_pan, want_core))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [40, 5000, 10_000, 13_000])
def test_order_groups(ctx, n):
    """P = 1, G - 1, G, G + 1, 2 G + 1 for the G orders one pass serves at this n; orders repeat"""
    k, G = 31, sp.accumulation_plan(n)["group"]
    assert G == {40: 8, 5000: 4, 10_000: 2, 13_000: 1}[n]
    rng = np.random.default_rng(n)
    sizes = [1, 1, 2, 2, 3, 5, 20, 33, 40, n // 2, n - 1, n]
    holders = [rng.choice(n, min(sizes[x % len(sizes)], n), replace=False).tolist() for x in range(60)]
    sketches = from_holders(n, holders, k)
    pool = shuffles(n, 4, 3)
    for P in sorted({1, max(G - 1, 1), G, G + 1, 2 * G + 1}):
        check(ctx, sketches, k, [pool[p % len(pool)] for p in range(P)])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [21, 31, 63])
def test_sketch_lengths_on_wave_and_tile_boundaries(ctx, k):
    """sketches of 63 .. 65, 255 .. 257 and 2047 .. 2049 keys (and none, one, 4 097) cut from one pool at overlapping places: the
    lists start and end across the 2 048-entry tiles of the scans, in whatever sketch a key's claimer sits"""
    sizes = [63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 0, 1, 4097, 300, 2000]
    keys = tp.pool(5000, k, 1)
    sketches = [keys[(i * 211) % 900:(i * 211) % 900 + s] for i, s in enumerate(sizes)]
    check(ctx, sketches, k, shuffles(len(sizes), 6, k))
    # the same behind an offset: the first sketch of the arrays is not part of the call
    mn, lo, hi, off, order = tp.pack(sketches, k)
    d = tp.upload(mn, lo, hi)
    n = len(sizes) - 1
    orders = shuffles(n, 3, 5)
    rows, pan, core = ctx.accumulation_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off[1:], n, np.array(orders, dtype=np.uint32), want_curves=True)
    want = model([set(s) for s in order[1:]], orders)
    assert (pan.tolist(), core.tolist()) == want and as_tuples(rows) == rows_of(*want)


@pytest.mark.gpu
def test_the_smallest_table(ctx, monkeypatch):
    """SPSP_DEBUG_PREVALENCE_TABLE=min: with 4 096 entries that are 4 096 keys every slot is taken and probe sequences wrap"""
    k = 63
    keys = tp.pool(4096, k, 2)
    alone = [keys[i * 256:(i + 1) * 256] for i in range(16)]
    shared = [keys[(i * 37) % 300:(i * 37) % 300 + 256] for i in range(16)]
    for table in ("min", None):
        if table:
            monkeypatch.setenv("SPSP_DEBUG_PREVALENCE_TABLE", table)
        else:
            monkeypatch.delenv("SPSP_DEBUG_PREVALENCE_TABLE")
        check(ctx, alone, k, shuffles(16, 4, 1))
        check(ctx, shared, k, shuffles(16, 4, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_against_the_rest_of_the_library(ctx, k, m):
    """60 sketches in families of six, through the decoder: the curves' ends are the prevalence pass's spectrum, their second step
    the comparison's cell, the listed order's steps the selection's union and intersection of the first j sketches"""
    payloads = tp.collection(k, m)
    sets = [tp.key_set(p) for p in payloads]
    n = len(payloads)
    orders = py_orders(n, 6, 11)[0]
    _, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(payloads)
    rows, pan, core = ctx.accumulation_device(k, d_mn, d_lo, d_hi, off, n, np.array(orders, dtype=np.uint32), want_curves=True)
    pan, core = pan.tolist(), core.tolist()
    want = model(sets, orders)
    assert (pan, core) == want and as_tuples(rows) == rows_of(*want)
    _, spectrum = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, 1, 1)
    inter, card = ctx.compare([sp.sketch_parse(p) for p in payloads])
    for o, p, c in zip(orders, pan, core):
        assert p[-1] == int(spectrum[1:].sum()) and c[-1] == int(spectrum[n])
        assert p[0] == c[0] == int(off[o[0] + 1] - off[o[0]]) == int(card[o[0]])
        assert all(a <= b for a, b in zip(p, p[1:])) and all(a >= b for a, b in zip(c, c[1:]))
        assert c[1] == int(inter[min(o[:2]), max(o[:2])])
    assert any(c[1] > 0 for c in core)
    for j in (2, 7, n):
        union = ctx.select_device(k, d_mn, d_lo, d_hi, off[:j + 1], j, 1, j, merged=True)[3]
        assert int(union[1]) == pan[0][j - 1]
        common = ctx.select_device(k, d_mn, d_lo, d_hi, off[:j + 1], j, j, j, merged=True)[3]
        assert int(common[1]) == core[0][j - 1]


def raw_call(ctx, k, d, off, n, orders, P):
    """the C call itself, with rows, pan and core filled with ones beforehand -> (rc, rows, pan, core)"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    orders = np.ascontiguousarray(orders, dtype=np.uint32)
    rows = np.full(n * 8, U64, dtype=np.uint64)
    pan, core = np.full(max(P, 1) * n, U64, dtype=np.uint64), np.full(max(P, 1) * n, U64, dtype=np.uint64)
    rc = sp.lib().spsp_accumulation_device(ctx._h, k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off.ctypes.data, n, orders.ctypes.data, P, rows.ctypes.data,
                                           pan.ctypes.data, core.ctypes.data)
    return rc, rows, pan, core


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(ctx):
    k = 31
    keys = tp.pool(40, k, 4)
    sketches = [keys[:20], keys[10:30], keys[25:40]]
    mn, lo, hi, off, order = tp.pack(sketches, k)
    d = tp.upload(mn, lo, hi)
    ident = [[0, 1, 2], [2, 1, 0]]
    # a key twice in a sketch: the fill's own flag; everything comes back zeroed
    twice = mn.copy(), lo.copy()
    twice[0][25], twice[1][25] = twice[0][24], twice[1][24]
    d_twice = tp.upload(twice[0], twice[1], None)
    rc, rows, pan, core = raw_call(ctx, k, d_twice, off, 3, ident, 2)
    assert rc == sp.ERR_ARG and "strictly increasing" in sp.lib().spsp_last_error().decode() and not rows.any() and not pan.any() and not core.any()
    # orders that are no permutations: the message names the order and the position
    for bad, where in (([[0, 1, 2], [2, 2, 0]], "order 1 is not a permutation of 0 .. 2: position 1 holds 2 again"),
                       ([[0, 3, 2], [2, 1, 0]], "order 0 is not a permutation of 0 .. 2: position 1 holds 3")):
        rc, rows, pan, core = raw_call(ctx, k, d, off, 3, bad, 2)
        assert rc == sp.ERR_ARG and where in sp.lib().spsp_last_error().decode() and not rows.any() and not pan.any() and not core.any()
    # no order, too many of them
    for P in (0, 1025):
        rc, rows, pan, core = raw_call(ctx, k, d, off, 3, np.tile(np.array([0, 1, 2], np.uint32), max(P, 1)), P)
        assert rc == sp.ERR_ARG and "1 .. 1024 orders" in sp.lib().spsp_last_error().decode() and not rows.any()
        with pytest.raises(sp.SpspError):
            ctx.accumulation_device(k, tp.ptr(d[0]), tp.ptr(d[1]), None, off, 3, np.zeros((P, 3), np.uint32))
    # k out of range, offsets that decrease, too many entries, no sketches
    assert raw_call(ctx, 64, d, off, 3, ident, 2)[0] == sp.ERR_ARG and raw_call(ctx, 0, d, off, 3, ident, 2)[0] == sp.ERR_ARG
    assert raw_call(ctx, k, d, [0, 30, 20, 55], 3, ident, 2)[0] == sp.ERR_ARG and "offsets" in sp.lib().spsp_last_error().decode()
    assert raw_call(ctx, k, d, [0, 20, 40, 0xFFFFFFF1], 3, ident, 2)[0] == sp.ERR_OVERFLOW
    with pytest.raises(sp.SpspError):
        ctx.accumulation_device(k, tp.ptr(d[0]), tp.ptr(d[1]), None, [0], 0, np.zeros((1, 0), np.uint32))
    # a context switched to unordered keys
    other = sp.Context(0)
    other.compare_keys_unordered(True)
    rc, rows, pan, core = raw_call(other, k, d, off, 3, ident, 2)
    assert rc == sp.ERR_ARG and "unordered" in sp.lib().spsp_last_error().decode() and not rows.any() and not pan.any()
    other.compare_keys_unordered(False)
    rc, rows, pan, core = raw_call(other, k, d, off, 3, ident, 2)
    other.close()
    want = model([set(s) for s in order], ident)
    assert rc == 0 and (pan.reshape(2, 3).tolist(), core.reshape(2, 3).tolist()) == want
    # and the first context after all of that
    rows, pan, core = ctx.accumulation_device(k, tp.ptr(d[0]), tp.ptr(d[1]), None, off, 3, ident, want_curves=True)
    assert (pan.tolist(), core.tolist()) == want and as_tuples(rows) == rows_of(*want)
    assert as_tuples(ctx.accumulation_device(k, tp.ptr(d[0]), tp.ptr(d[1]), None, off, 3, ident)) == rows_of(*want)


def gunzip(path):
    return gzip.open(path, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_accumulation_files_and_the_command_line(ctx, tmp_path, k, m):
    payloads = tp.collection(k, m)[:14]
    sets = [tp.key_set(p) for p in payloads]
    n = len(payloads)
    paths = tp.write_files(tmp_path, payloads)
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    r = run("-A", "7", "-z", "3", "-f", "bank.txt", "-o", "cli")
    assert r.returncode == 0, r.stdout + r.stderr
    want = rows_of(*model(sets, py_orders(n, 7, 3)[0]))
    assert gunzip(str(tmp_path / "cli_accumulation.csv.gz")) == py_csv(want, 7)
    assert [f for f in os.listdir(tmp_path) if f.startswith("cli")] == ["cli_accumulation.csv.gz"]
    line = "%d sketch(es) over 7 order(s): %d distinct keys, %d of them in every sketch" % (n, len(set().union(*sets)), len(set.intersection(*sets)))
    assert line in r.stdout.splitlines(), r.stdout
    # the seed defaults to 1, the precision is -p's
    r = run("-A", "3", "-p", "3", "-f", "bank.txt", "-o", "one")
    assert r.returncode == 0, r.stdout + r.stderr
    assert gunzip(str(tmp_path / "one_accumulation.csv.gz")) == py_csv(rows_of(*model(sets, py_orders(n, 3, 1)[0])), 3, 3)
    # the Python call writes the same bytes and returns the rows
    rows = ctx.accumulation_files(paths, str(tmp_path / "lib"), orders=7, seed=3)
    assert as_tuples(rows) == want and gunzip(str(tmp_path / "lib_accumulation.csv.gz")) == py_csv(want, 7)
    rows = ctx.accumulation_files(paths, str(tmp_path / "p17"), orders=5, seed=U64, precision=17)
    assert gunzip(str(tmp_path / "p17_accumulation.csv.gz")) == py_csv(as_tuples(rows), 5, 17) == py_csv(rows_of(*model(sets, py_orders(n, 5, U64)[0])), 5, 17)
    for orders in (0, 1025):
        with pytest.raises(sp.SpspError) as e:
            ctx.accumulation_files(paths, str(tmp_path / "no"), orders=orders)
        assert e.value.code == sp.ERR_ARG and not os.path.exists(str(tmp_path / "no_accumulation.csv.gz"))


@pytest.mark.gpu
def test_accumulation_files_at_mixed_rates(ctx, tmp_path):
    k, m = 31, 11
    genomes = synth.family_genomes(11, 8, 40_000, 1, [0.0, 0.001, 0.004])
    coarse = [ctx.sketch_text(synth.to_fasta(g, "g%d" % i), k, m, 100.0)[0] for i, g in enumerate(genomes)]
    mixed = [ctx.sketch_text(synth.to_fasta(g, "g%d" % i), k, m, 10.0)[0] if i % 3 == 0 else coarse[i] for i, g in enumerate(genomes)]
    sets = [tp.key_set(p) for p in coarse]
    assert len(tp.key_set(mixed[0])) > 4 * len(sets[0])
    paths = tp.write_files(tmp_path, mixed)
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    want = py_csv(rows_of(*model(sets, py_orders(8, 7, 3)[0])), 7)
    r = subprocess.run([EXE, "-A", "7", "-z", "3", "-s", "auto", "-f", "bank.txt", "-o", "cli"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert gunzip(str(tmp_path / "cli_accumulation.csv.gz")) == want
    for rate in ("auto", 100):
        ctx.accumulation_files(paths, str(tmp_path / "lib"), orders=7, seed=3, rate=rate)
        assert gunzip(str(tmp_path / "lib_accumulation.csv.gz")) == want
    # as the files are, the finer sketches keep all their keys: other curves
    as_is = ctx.accumulation_files(paths, str(tmp_path / "asis"), orders=7, seed=3)
    assert as_tuples(as_is) == rows_of(*model([tp.key_set(p) for p in mixed], py_orders(8, 7, 3)[0]))
    with pytest.raises(sp.SpspError) as e:
        ctx.accumulation_files(paths, str(tmp_path / "no"), rate=10)
    assert e.value.code == sp.ERR_ARG and "upsample" in str(e.value)
