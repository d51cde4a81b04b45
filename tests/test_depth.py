"""Depth: how deep a read set covers each reference of an index (include/spsp.h: spsp_depth_begin_device, spsp_depth_add_device,
spsp_depth_read_device, spsp_depth_plan_host, spsp_depth_stage_ms, spsp_depth_csv_host, spsp_depth_files; bin/comparator -D).

The rule, on the comparator's keys.  References 0 .. R-1 with key sets K_j, U their union, h(x) the references that hold x; records
with distinct key sets Q_r:

    c(x) = #{r : x in Q_r}                     found at min_count: c(x) >= min_count
    per reference over its found keys: keys, found, sum, the lower median, max -- and the same five over its keys with h == 1

Every expected value below comes from `model`: collections.Counter, sorted and Python integers.  No tolerance anywhere.  To give key
x the count c the record-key array holds x c times, shuffled: the add takes no record offsets.

Where the kernels cut (depth_plan names the number): the reduction keeps two LDS histograms of B bins per reference, the last bin
holding every count >= B - 1; a median whose rank lands there is resolved by a radix select, byte by byte.  Every kernel works in
waves of 64 and workgroups of 256 over consecutive record keys or index entries."""
import gzip
import os
import random
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

import supersampler_amd as sp
import test_classify as tc
import test_prevalence as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
HEADER = "reference,keys,found,f_found,median,mean,max,unique_keys,unique_found,f_unique_found,unique_median,unique_mean,unique_max\n"
FIELDS = ("keys", "found", "sum", "median", "max", "unique_keys", "unique_found", "unique_sum", "unique_median", "unique_max")


# -------------------------------------------------------------------------------------------------- the model

def model(refs, record_keys, min_count=1):
    """refs: one collection of key tuples per reference; record_keys: the keys of all records, one after the other (a key as often
    as records hold it), or a Counter of them -> (rows: per reference the ten numbers of FIELDS, totals: (record_keys, hit_keys,
    index_keys, index_found), c: the Counter over the index's keys)"""
    refs = [set(K) for K in refs]
    union = set().union(*refs) if refs else set()
    h = Counter(x for K in refs for x in K)
    every = record_keys if isinstance(record_keys, Counter) else Counter(record_keys)
    c = Counter({x: n for x, n in every.items() if x in union})

    def five(keys):
        found = sorted(c[x] for x in keys if c[x] >= min_count)
        n = len(found)
        return (len(keys), n, sum(found), found[(n - 1) // 2] if n else 0, found[-1] if n else 0)

    rows = [five(K) + five([x for x in K if h[x] == 1]) for K in refs]
    totals = (sum(every.values()), sum(c.values()), len(union), sum(1 for x in union if c[x] >= min_count))
    return rows, totals, c


def as_tuples(rows):
    return [tuple(int(r[f]) for f in FIELDS) for r in rows]


def as_totals(t):
    return tuple(int(t[f]) for f in ("record_keys", "hit_keys", "index_keys", "index_found"))


def as_array(rows):
    out = np.zeros(len(rows), dtype=sp.DEPTH_ROW_DTYPE)
    for j, r in enumerate(rows):
        for f, v in zip(FIELDS, r):
            out[j][f] = v
    return out


def py_csv(rows, names, precision=6):
    g = lambda a, b: "%.*g" % (precision, a / b) if b else "0"
    text = HEADER
    for (keys, found, total, median, top, ukeys, ufound, utotal, umedian, utop), name in zip(rows, names):
        text += "%s,%d,%d,%s,%d,%s,%d,%d,%d,%s,%d,%s,%d\n" % (name, keys, found, g(found, keys), median, g(total, found), top,
                                                              ukeys, ufound, g(ufound, ukeys), umedian, g(utotal, ufound), utop)
    return text.encode()


# ------------------------------------------------------------------------------------------------ not GPU

def K(*xs):
    return [(x, 0, x) for x in xs]


def times(pairs):
    return [key for x, n in pairs for key in K(x) * n]


def test_model_on_a_hand_made_case():
    refs = [K(1, 2, 3, 4), K(3, 4, 5), K(9), K(6, 7), K()]
    # c: 1 -> 5, 2 -> 1, 3 -> 2, 4 -> 7, 5 -> 3, 6 -> 2, 9 and 7 -> 0, and 77 is no key of the index
    reads = times([(1, 5), (2, 1), (3, 2), (4, 7), (5, 3), (6, 2), (77, 4)])
    rows, totals, c = model(refs, reads)
    assert totals == (24, 20, 8, 6) and c[(4, 0, 4)] == 7 and (77, 0, 77) not in c
    assert rows[0] == (4, 4, 15, 2, 7, 2, 2, 6, 1, 5)           # even found: 1 2 5 7 -> the lower of the two middle ones; unique keys 1 and 2: 1 5
    assert rows[1] == (3, 3, 12, 3, 7, 1, 1, 3, 3, 3)           # odd found: 2 3 7; found 1 among the unique
    assert rows[2] == (1, 0, 0, 0, 0, 1, 0, 0, 0, 0) and rows[4] == (0,) * 10
    assert rows[3] == (2, 1, 2, 2, 2, 2, 1, 2, 2, 2)            # found 1
    rows2, totals2, _ = model(refs, reads, 2)
    assert rows2[0] == (4, 3, 14, 5, 7, 2, 1, 5, 5, 5) and rows2[1] == (3, 3, 12, 3, 7, 1, 1, 3, 3, 3) and totals2 == (24, 20, 8, 5)
    assert model(refs, reads, 6)[0][0] == (4, 1, 7, 7, 7, 2, 0, 0, 0, 0)
    assert model(refs, reads, 3)[0][0][:5] == (4, 2, 12, 5, 7)                       # found 2: the lower one
    rows8, totals8, _ = model(refs, reads, 8)                                       # above the maximum
    assert all(r[1:5] == (0, 0, 0, 0) and r[6:] == (0, 0, 0, 0) for r in rows8) and totals8 == (24, 20, 8, 0)
    assert model(refs, Counter(reads)) == model(refs, reads)


CALLS = ("spsp_depth_begin_device", "spsp_depth_add_device", "spsp_depth_read_device", "spsp_depth_plan_host", "spsp_depth_stage_ms",
         "spsp_depth_csv_host", "spsp_depth_files")


def test_abi_has_the_depth_calls():
    assert set(CALLS) <= set(sp.ABI_SYMBOLS)
    assert sp.DEPTH_ROW_DTYPE.itemsize == 48 and sp.DEPTH_TOTALS_DTYPE.itemsize == 24
    assert sp.DEPTH_ROW_DTYPE.names == ("sum", "unique_sum", "keys", "found", "median", "max", "unique_keys", "unique_found", "unique_median", "unique_max")
    assert sp.DEPTH_TOTALS_DTYPE.names == ("record_keys", "hit_keys", "index_keys", "index_found")
    for name in CALLS:
        assert hasattr(sp.lib(), name)


def test_depth_plan_is_the_constant_of_the_kernel():
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    bins = int(re.search(r"constexpr uint32_t kDpBins = (\d+);", text).group(1))
    assert sp.depth_plan() == bins == 4096
    assert 2 * 4 * bins <= 64 * 1024                                                   # the two histograms, with room for more workgroups on a CU


ROWS = [(6, 5, 17, 3, 9, 2, 1, 9, 9, 9), (0,) * 10, (7, 0, 0, 0, 0, 7, 0, 0, 0, 0), (3, 3, 3 * 0xffffffff - 5, 1 << 31, 0xffffffff, 3, 3, 3 * 0xffffffff - 5, 1 << 31, 0xffffffff),
        (3, 3, 7, 2, 3, 0, 0, 0, 0, 0)]
NAMES = ["a one.fa.gz", "dir/b.two", "c", "d.1.2.sketch", "e"]


def test_the_csv_writer_equals_the_python_writer():
    for precision in (6, 3):
        assert sp.depth_csv(as_array(ROWS), NAMES, precision) == py_csv(ROWS, NAMES, precision)
    lines = sp.depth_csv(as_array(ROWS), NAMES).decode().splitlines()
    assert lines[0] + "\n" == HEADER and lines[1] == "a one.fa.gz,6,5,0.833333,3,3.4,9,2,1,0.5,9,9,9" and lines[2] == "dir/b.two,0,0,0,0,0,0,0,0,0,0,0,0"
    assert sp.depth_csv(as_array(ROWS), NAMES, 3).decode().splitlines()[1] == "a one.fa.gz,6,5,0.833,3,3.4,9,2,1,0.5,9,9,9"
    assert sp.depth_csv(as_array([]), []) == HEADER.encode()


#       keys found sum median max | unique: keys found sum median max
BAD = [(6, 7, 17, 3, 9, 2, 1, 9, 9, 9),        # found > keys
       (6, 5, 17, 3, 9, 7, 1, 9, 9, 9),        # unique_keys > keys
       (6, 5, 17, 3, 9, 2, 3, 9, 3, 3),        # unique_found > unique_keys
       (6, 1, 9, 9, 9, 2, 2, 2, 1, 1),         # unique_found > found
       (6, 5, 17, 10, 9, 2, 1, 9, 9, 9),       # median > max
       (6, 1, 3, 3, 4, 2, 0, 0, 0, 0),         # max > sum
       (6, 0, 3, 0, 0, 2, 0, 0, 0, 0),         # found == 0 with a sum
       (6, 0, 0, 0, 1, 2, 0, 0, 0, 0),         # ... with a max
       (6, 5, 17, 0, 9, 2, 1, 9, 9, 9),        # found > 0 with median == 0
       (6, 5, 4, 1, 1, 2, 0, 0, 0, 0),         # sum < found
       (6, 5, 46, 3, 9, 2, 1, 9, 9, 9),        # sum > found * max
       (6, 5, 17, 3, 9, 2, 1, 9, 10, 9),       # unique: median > max
       (6, 5, 17, 3, 9, 2, 1, 8, 9, 9),        # unique: max > sum
       (6, 5, 17, 3, 9, 2, 0, 0, 0, 2),        # unique: nothing found, and a max
       (6, 5, 17, 3, 9, 2, 2, 9, 0, 9),        # unique: found with median == 0
       (6, 5, 17, 3, 9, 2, 2, 1, 1, 1),        # unique: sum < found
       (6, 5, 17, 3, 9, 2, 2, 19, 9, 9),       # unique: sum > found * max
       (6, 5, 17, 3, 9, 2, 2, 18, 9, 9)]       # unique_sum > sum


def test_the_csv_writer_refuses_rows_that_contradict_themselves():
    for row in BAD:
        with pytest.raises(sp.SpspError) as e:
            sp.depth_csv(as_array([ROWS[0], row]), ["a", "b"])
        assert e.value.code == sp.ERR_ARG and "reference 1" in str(e.value), row
    assert sp.depth_csv(as_array([ROWS[0], ROWS[0]]), ["a", "b"])


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    (tmp_path / "labels.txt").write_text("a\nb\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-D", "r.fq", o, v) for o, v in (("-q", "list.txt"), ("-g", "3"), ("-c", "0.5"), ("-C", "0.5"), ("-N", "5"), ("-J", "0.5"), ("-K", "0.5"), ("-I", "0.5"),
                                                ("-P", "0.9"), ("-r", "0.9"), ("-R", "0.9"), ("-l", "0.5"), ("-L", "0.5"), ("-S", "union"), ("-E", "union"),
                                                ("-A", "10"), ("-G", "labels.txt"), ("-X", "r.fa"))]
    cases += [("-W", "2")]
    cases += [("-D", "r.fq", "-W", v) for v in ("0", "-1", "abc", "4294967296", "")]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1, (args, r.stdout, r.stderr)
        assert any(o in r.stdout for o in ("-D", "-W")), (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


def test_host_functions_under_the_sanitizers():
    """tests/tools/depth_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the plan
    and the CSV writer with its refusals (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "depth_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "depth_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def key_arrays(keys, k):
    mn = np.array([x[0] for x in keys], dtype=np.uint32)
    hi = np.array([x[1] for x in keys], dtype=np.uint64)
    lo = np.array([x[2] for x in keys], dtype=np.uint64)
    return mn, lo, (hi if k > 32 else None)


class Index:
    """the references on the device (behind `lead` entries that are no part of the index) and the context's index over them; the
    tensors live as long as the object, and so do the record keys of every add until the object goes"""

    def __init__(self, ctx, k, refs, lead=()):
        mn, lo, hi, off, self.order = tp.pack([list(lead)] + [list(K) for K in refs], k)
        self.d = tp.upload(mn, lo, hi)
        self.ctx, self.k, self.off, self.R = ctx, k, off[1:], len(refs)
        self.entries = [x for s in self.order[1:] for x in s]
        self.alive = []
        ctx.classify_index_device(k, tp.ptr(self.d[0]), tp.ptr(self.d[1]), tp.ptr(self.d[2]), self.off, len(refs))

    def add(self, keys, seed=1, first=0, n_keys=None):
        """keys: a list of key tuples, shuffled by `seed` (0: as it is), or (mn, lo, hi) numpy arrays taken as they are"""
        if isinstance(keys, tuple):
            mn, lo, hi = keys
        else:
            keys = list(keys)
            if seed:
                random.Random(seed).shuffle(keys)
            mn, lo, hi = key_arrays(keys, self.k)
        d = tp.upload(mn, lo, hi)
        self.alive.append(d)
        self.ctx.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), first, len(mn) - first if n_keys is None else n_keys)

    def read(self, min_count=1):
        rows, totals = self.ctx.depth_read(min_count)
        self.alive = []                                                                # (the read waited: the adds are through)
        return as_tuples(rows), as_totals(totals)

    def counts(self, min_count=1):
        rows, totals, d = self.ctx.depth_read(min_count, want_counts=True)
        return self.ctx.to_host(d, len(self.entries), np.uint32).tolist() if self.entries else []


def check(ctx, k, refs, reads, min_counts=(1,), index=None, lead=(), seed=1):
    """begin, one add of `reads`, a read per min_count, each against the model"""
    index = index or Index(ctx, k, refs, lead)
    ctx.depth_begin()
    index.add(reads, seed)
    for mc in min_counts:
        want_rows, want_totals, _ = model(refs, reads, mc)
        rows, totals = index.read(mc)
        assert totals == want_totals, (mc, totals, want_totals)
        assert rows == want_rows, (mc, [(j, a, b) for j, (a, b) in enumerate(zip(rows, want_rows)) if a != b][:3])
    return index


def repeat(pairs):
    return [x for x, n in pairs for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_nothing_and_almost_nothing(ctx, k):
    p, stranger = tp.pool(40, k), tp.pool(30, k, salt=700_000)
    refs = [p[:20], p[10:40], []]                                                      # an empty reference among others
    index = Index(ctx, k, refs)
    ctx.depth_begin()
    rows, totals = index.read()                                                        # read straight after begin
    assert rows == [(20, 0, 0, 0, 0, 10, 0, 0, 0, 0), (30, 0, 0, 0, 0, 20, 0, 0, 0, 0), (0,) * 10] and totals == (0, 0, 40, 0)
    ctx.depth_add(None, None, None, 0, 0)                                              # an add of zero keys
    index.add(stranger[:5], n_keys=0)
    assert index.read() == (rows, totals)
    index.add(stranger)                                                                # record keys that miss the index entirely
    assert index.read() == (rows, (30, 0, 40, 0))
    check(ctx, k, refs, repeat([(p[0], 3), (p[15], 2), (p[39], 1), (stranger[0], 2)]), (1, 2, 3, 4), index=index)
    del index
    check(ctx, k, [p], repeat([(p[3], 2), (p[4], 1), (stranger[1], 1)]), (1, 2))      # R = 1
    index = Index(ctx, k, [[], []])                                                    # an index of empty references only
    ctx.depth_begin()
    index.add(p[:3])
    assert index.read() == ([(0,) * 10] * 2, (3, 0, 0, 0)) and index.counts() == []
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_launch_boundaries_of_the_add(ctx, k):
    p, stranger = tp.pool(1200, k), tp.pool(1200, k, salt=700_000)
    refs = [p[:500], p[400:900], p[850:1100]]
    index = Index(ctx, k, refs, lead=p[1100:1150])                                     # sk_off[0] != 0: 50 entries in front of the index
    assert int(index.off[0]) == 50
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        for reads in ([p[(i * 7) % 1100] if i % 3 else stranger[i] for i in range(n)],   # waves that mix hits and misses
                      [p[(i * 7) % 1100] for i in range(n)], stranger[:n]):               # all hits, all misses
            check(ctx, k, refs, reads, index=index, seed=0)
    # a slice of a larger array whose outside entries would hit if they were read
    inner = [p[i] for i in range(0, 300, 2)] + stranger[:33]
    ctx.depth_begin()
    index.add(key_arrays(p[:77] + inner + p[:500], k), first=77, n_keys=len(inner))
    want_rows, want_totals, c = model(refs, inner)
    assert index.read() == (want_rows, want_totals)
    assert index.counts() == [c[x] for x in index.entries]
    # the entries in front of the index are no keys of it
    ctx.depth_begin()
    index.add(p[1100:1150])
    assert index.read()[1] == (50, 0, 1100, 0)
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_a_hot_key(ctx, k):
    p = tp.pool(300, k)
    refs = [p[:100], p[50:200]]
    reads = Counter({p[60]: 70_000, p[10]: 5_000})
    reads.update({p[i]: 1 for i in range(100, 160)})
    index = Index(ctx, k, refs)
    ctx.depth_begin()
    flat = list(reads.elements())
    order = np.random.default_rng(3).permutation(len(flat))
    mn, lo, hi = key_arrays(flat, k)
    index.add((mn[order], lo[order], hi[order] if hi is not None else None))
    want_rows, want_totals, c = model(refs, reads)
    rows, totals = index.read()
    assert (rows, totals) == (want_rows, want_totals) and rows[0][4] == 70_000 == rows[1][4] and totals[1] == 75_060
    assert index.counts() == [c[x] for x in index.entries]
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_medians_around_the_last_bin(ctx, k):
    B = sp.depth_plan()
    cases = [[B - 2], [B - 1], [B], [B - 2, B - 1], [B - 1, B], [1, B - 1, B + 5, 3 * B],
             [B + 0x100 + x for x in (1, 5, 9, 200, 255)],                              # above B, the same but for their low byte
             [B + 0x0005, B + 0x0305]]                                                  # ... but for bits 8 .. 15
    assert all((v ^ cases[6][0]) < 256 for v in cases[6]) and (cases[7][0] ^ cases[7][1]) & ~0xff00 == 0
    p = tp.pool(sum(len(c) for c in cases) + 2, k)
    refs, reads, at = [], Counter(), 0
    for counts in cases:
        refs.append(p[at:at + len(counts)] + p[-2:])                                   # two keys every reference holds: unique_* differs
        reads.update(dict(zip(p[at:], counts)))
        at += len(counts)
    reads[p[-1]] = 2 * B
    assert sum(reads.values()) < 10 ** 5
    want_rows, want_totals, _ = model(refs, reads)
    assert [r[8] for r in want_rows] == [B - 2, B - 1, B, B - 2, B - 1, B - 1, B + 0x109, B + 5]   # the unique medians: below, on and inside the last bin
    assert [r[3] for r in want_rows][:3] == [B - 2, B - 1, B] and want_rows[7][3] == B + 0x305
    index = Index(ctx, k, refs)
    ctx.depth_begin()
    flat = list(reads.elements())
    order = np.random.default_rng(5).permutation(len(flat))
    mn, lo, hi = key_arrays(flat, k)
    index.add((mn[order], lo[order], hi[order] if hi is not None else None))
    for mc in (1, B - 1, B, B + 6):
        assert index.read(mc) == model(refs, reads, mc)[:2], mc
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_median_ranks_and_min_count(ctx, k):
    sizes = (1, 2, 3, 4, 255, 256, 257)
    p = tp.pool(2 * sum(sizes), k)
    refs, reads, at = [], Counter(), 0
    for n in sizes:
        refs.append(p[at:at + n]); reads.update({x: 2 + i for i, x in enumerate(p[at:at + n])}); at += n    # distinct counts 2 .. n + 1
        refs.append(p[at:at + n]); reads.update({x: 3 for x in p[at:at + n]}); at += n                      # all equal
    index = Index(ctx, k, refs)
    ctx.depth_begin()
    index.add(list(reads.elements()), seed=9)
    for mc in (1, 2, 3, 4, 257, 258, 259):     # below and at the smallest count, one above it, ..., at the maximum (258) and one above it
        want = model(refs, reads, mc)
        assert index.read(mc) == want[:2], mc
    assert index.read(259)[0][12][1:5] == (0, 0, 0, 0) and index.read(258)[0][12][1:5] == (1, 258, 258, 258) and index.read(259)[1][3] == 0
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_unique_against_shared_keys(ctx, k):
    p = tp.pool(200, k)
    everybody, pair = p[:10], p[10:30]
    refs = [everybody + pair + p[30:60],             # unique keys, keys of two, keys of all
            everybody + pair,                        # no unique key
            everybody + p[60:100],
            p[100:150],                              # unique keys only
            everybody]
    reads = Counter({x: 1 + i % 7 for i, x in enumerate(p[:160]) if i % 4})
    index = check(ctx, k, refs, list(reads.elements()), (1, 2, 5, 7, 8))
    rows, _ = index.read()
    assert rows[1][5:] == (0, 0, 0, 0, 0) and rows[3][:5] == rows[3][5:] and rows[0][6] < rows[0][1]
    del index
    refs = [everybody + p[30:40], everybody + p[40:50], everybody]                     # h = R: keys that every reference holds
    index = check(ctx, k, refs, list(reads.elements()), (1, 3))
    assert index.read()[0][2][5:] == (0, 0, 0, 0, 0)
    del index


@pytest.mark.gpu
def test_one_long_reference_among_short_ones(ctx):
    k = 31
    n_long = 100_000
    p = tp.pool(n_long + 2000, k)
    refs = [p[n_long + 6 * j:n_long + 6 * j + 1 + j % 10] for j in range(150)] + [p[:n_long]] + [p[n_long + 6 * j:n_long + 6 * j + 1 + j % 10] for j in range(150, 300)]
    count_of = [(i * 7919) % 50 for i in range(n_long)] + [i % 4 for i in range(2000)]
    reads = Counter({x: c for x, c in zip(p, count_of) if c})
    mn, lo, _ = key_arrays(p, k)
    order = np.random.default_rng(7).permutation(np.repeat(np.arange(len(p)), count_of))
    index = Index(ctx, k, refs)
    ctx.depth_begin()
    index.add((mn[order], lo[order], None))
    for mc in (1, 25):
        want = model(refs, reads, mc)
        assert index.read(mc) == want[:2], mc
        assert want[0][150][1] < n_long
    del index


def internal_constant(name):
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))


@pytest.mark.gpu
def test_long_references_go_by_segments(ctx):
    """a reference of more than kDpLongKeys entries is reduced by workgroups of kDpSegKeys entries and merged: references on and
    one beyond the threshold, a last segment of one entry, and a median that the merge resolves by the radix select"""
    k, B = 31, sp.depth_plan()
    L, S = internal_constant("kDpLongKeys"), internal_constant("kDpSegKeys")
    assert L == 65536 and S == 16384
    p = tp.pool(3 * L + S + 300, k)
    r0, r1, r2 = p[:L], p[L:2 * L + 1], p[2 * L + 1:3 * L + S + 2]
    assert (len(r0), len(r1), len(r2)) == (L, L + 1, L + S + 1)
    refs = [r0, p[3 * L + S + 2:3 * L + S + 50], r1 + r0[:100], [], r2[:-7] + r1[:7], p[3 * L + S + 50:]]       # L | short | L + 101 | none | L + S + 1 | short
    count_of = [(i * 7919) % 5 for i in range(len(p))]
    for i, c in zip((L + 5, L + 20_000, 2 * L - 3, 2 * L, L + 40_000), (B + 0x101, B + 0x105, B + 0x109, B + 0x1c8, B + 0x1ff)):
        count_of[i] = c                                                                # five keys of the second long reference, above B
    reads = Counter({x: c for x, c in zip(p, count_of) if c})
    mn, lo, _ = key_arrays(p, k)
    order = np.random.default_rng(17).permutation(np.repeat(np.arange(len(p)), count_of))
    index = Index(ctx, k, refs)
    ctx.depth_begin()
    index.add((mn[order], lo[order], None))
    for mc in (1, 3, 5, B):
        want = model(refs, reads, mc)
        assert index.read(mc) == want[:2], mc
    assert want[0][2][1:5] == (5, 5 * B + 0x101 + 0x105 + 0x109 + 0x1c8 + 0x1ff, B + 0x109, B + 0x1ff) and want[0][0][1] == 0
    assert index.counts() == [reads[x] for x in index.entries]
    del index


@pytest.mark.gpu
def test_65535_references_of_one_key(ctx):
    k, R = 63, 65535
    p = tp.pool(R, k)
    refs = [[x] for x in p]
    reads = Counter({x: j % 3 for j, x in enumerate(p) if j % 3})
    index = check(ctx, k, refs, list(reads.elements()), (1, 2))
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_adds_accumulate_and_reads_do_not_consume(ctx, k):
    p, stranger = tp.pool(400, k), tp.pool(50, k, salt=700_000)
    refs = [p[:150], p[100:300], p[290:400]]
    records = [random.Random(r).sample(p, 1 + r % 40) + stranger[r % 7:r % 7 + 2] for r in range(120)]
    flat = [x for r in records for x in r]
    index = Index(ctx, k, refs)
    whole = model(refs, flat)
    for cut in (0, 1, len(records[0]) + 3, len(flat) // 2, len(flat) - 1, len(flat)):    # any split, one inside a record
        ctx.depth_begin()
        index.add(flat[:cut], seed=0)
        if cut == len(flat) // 2:
            assert index.read() == model(refs, flat[:cut])[:2]                         # a read between the adds: the partial profile
        index.add(flat[cut:], seed=0)
        assert index.read() == whole[:2], cut
        assert index.read() == whole[:2]                                               # twice
        assert index.read(2) == model(refs, flat, 2)[:2] and index.read() == whole[:2]
    assert index.counts() == [whole[2][x] for x in index.entries]                      # parallel to the index arrays
    assert index.counts(3) == index.counts()                                           # plain c, whatever min_count
    ctx.depth_begin()                                                                  # begin clears
    assert index.read() == model(refs, [])[:2]
    ctx.timing_enable(True)
    ctx.depth_stage_ms()
    index.add(flat[:100]); index.add(flat[100:])
    assert index.read() == whole[:2]
    ms = ctx.depth_stage_ms()
    ctx.timing_enable(False)
    assert list(ms) == ["add", "entry", "reduce"] and all(v > 0 for v in ms.values()) and not any(ctx.depth_stage_ms().values())
    del index


@pytest.mark.gpu
def test_refusals(ctx):
    p31, p63 = tp.pool(100, 31), tp.pool(100, 63)
    fresh = sp.Context(0)
    d = tp.upload(*key_arrays(p31, 31))
    d63 = tp.upload(*key_arrays(p63, 63))

    def refused(call, code=sp.ERR_ARG, word=None):
        with pytest.raises(sp.SpspError) as e:
            call()
        assert e.value.code == code and (word is None or word in str(e.value)), str(e.value)

    refused(fresh.depth_begin, word="index")                                           # no index at all
    index = Index(fresh, 31, [p31[:50], p31[25:75]])
    refused(lambda: fresh.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), None, 0, 10), word="begin")    # add and read without begin
    refused(fresh.depth_read, word="begin")
    fresh.depth_begin()
    refused(lambda: fresh.depth_add(tp.ptr(d63[0]), tp.ptr(d63[1]), tp.ptr(d63[2]), 0, 10), word="kmer_hi")   # kmer_hi given for k = 31
    refused(lambda: fresh.depth_read(0), word="min_count")
    refused(lambda: fresh.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), None, 0, 0xfffffff1), sp.ERR_OVERFLOW)
    fresh.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), None, 0, 30)
    assert as_totals(fresh.depth_read()[1]) == (30, 30, 75, 30)                        # the refused adds added nothing
    fresh.prevalence_device(31, tp.ptr(index.d[0]), tp.ptr(index.d[1]), None, index.off, 2, 1, 2)      # drops the index, and the counters with it
    refused(lambda: fresh.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), None, 0, 10))
    refused(fresh.depth_read)
    refused(fresh.depth_begin, word="index")
    index = Index(fresh, 31, [p31[:50], p31[25:75]])
    fresh.depth_begin()
    index2 = Index(fresh, 31, [p31[:10]])                                              # a new index ends the old one's counters
    refused(lambda: fresh.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), None, 0, 10))
    refused(fresh.depth_read)
    fresh.depth_begin()
    assert as_tuples(fresh.depth_read()[0]) == [(10, 0, 0, 0, 0, 10, 0, 0, 0, 0)]
    index3 = Index(fresh, 63, [p63[:40]])
    fresh.depth_begin()
    refused(lambda: fresh.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), None, 0, 10), word="kmer_hi")  # kmer_hi missing for k = 63
    fresh.depth_add(tp.ptr(d63[0]), tp.ptr(d63[1]), tp.ptr(d63[2]), 35, 10)
    assert as_totals(fresh.depth_read()[1]) == (10, 5, 40, 5)
    del index, index2, index3
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_against_classify(ctx, k):
    rng = random.Random(5)
    p = tp.pool(4000, k)
    refs = [rng.sample(p, rng.randint(0, 400)) for _ in range(50)]
    recs = [rng.sample(p, rng.randint(0, 60)) + tp.pool(rng.randint(0, 5), k, salt=10 ** 6 + 10 * r) for r in range(2000)]
    mn, lo, hi, off, order = tp.pack(recs, k)
    d = tp.upload(mn, lo, hi)
    index = Index(ctx, k, refs)
    records, hits = ctx.classify_device(tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, 64)
    ctx.depth_begin()
    ctx.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), 0, int(off[-1]))
    rows, totals = ctx.depth_read()
    assert int(totals["hit_keys"]) == int(records["hit_keys"].astype(np.uint64).sum()) > 0 and int(totals["record_keys"]) == int(off[-1])
    shared = [0] * 50
    for rec, h in zip(records, hits):
        assert int(rec["passing"]) == int(rec["listed"])                               # top = 64 >= R: every sharing reference is listed
        for x in h[:int(rec["listed"])]:
            shared[int(x["reference"])] += int(x["shared"])
    assert [int(r["sum"]) for r in rows] == shared
    assert as_tuples(rows) == model(refs, [x for r in order for x in r])[0]
    del d, index


# ------------------------------------------------------------------------------------------ files and the command line

def depth_file(root, tag):
    return tp.gunzip(os.path.join(str(root), tag + "_depth.csv.gz"))


def outputs(root, tag):
    return sorted(f for f in os.listdir(str(root)) if f.startswith(tag))


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1.0, 4.0])
def test_depth_files_and_the_command_line(ctx, tmp_path, s):
    refs, recs = tc.file_case()
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, s)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    ref_sets = [tp.key_set(p) for p in payloads]
    once = [x for _, _, seq in recs for x in tc.record_keys(seq, s)]
    (tmp_path / "recs.fa").write_bytes(tc.fasta_of(recs))
    with gzip.open(str(tmp_path / "recs.fq.gz"), "wb") as f:
        f.write(tc.fastq_of(recs))
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    cli = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    for tag, files, mc, precision in (("a", ["recs.fa"], 1, 6), ("b", ["recs.fq.gz"], 1, 6), ("c", ["recs.fa", "recs.fq.gz"], 1, 6), ("d", ["recs.fa", "recs.fq.gz"], 2, 3)):
        want_rows, want_totals, _ = model(ref_sets, once * len(files), mc)
        if tag == "c":                                                                 # (every count doubles: the case cannot pass vacuously)
            assert any(r[3] >= 2 for r in want_rows) and any(r[6] < r[1] for r in want_rows)
            assert [r[2] for r in want_rows] == [2 * r[2] for r in model(ref_sets, once)[0]]
        rows, totals = ctx.depth_files(paths, [str(tmp_path / f) for f in files], str(tmp_path / ("lib" + tag)), mc, precision)
        assert as_tuples(rows) == want_rows and as_totals(totals) == want_totals
        text = py_csv(want_rows, paths, precision)
        assert depth_file(tmp_path, "lib" + tag) == text and outputs(tmp_path, "lib" + tag) == ["lib%s_depth.csv.gz" % tag]
        args = [a for f in files for a in ("-D", f)] + ["-f", "bank.txt", "-o", "cli" + tag] + (["-W", str(mc)] if mc != 1 else []) + (["-p", "3"] if precision == 3 else [])
        r = cli(*args)
        assert r.returncode == 0, r.stdout + r.stderr
        assert depth_file(tmp_path, "cli" + tag) == text and outputs(tmp_path, "cli" + tag) == ["cli%s_depth.csv.gz" % tag]     # and no matrix files
        assert "%d record(s)" % (len(recs) * len(files)) in r.stdout and "%d hit key(s)" % want_totals[1] in r.stdout
    with pytest.raises(sp.SpspError):                                                  # a reads file that is not there, behind one that is
        ctx.depth_files(paths, [str(tmp_path / "recs.fa"), str(tmp_path / "none.fa")], str(tmp_path / "no"))
    bad = tc.fastq_of(recs[:7]).replace(b"\n+\n", b"\n-\n", 3)
    (tmp_path / "bad.fq").write_bytes(bad)
    with pytest.raises(sp.SpspError) as e:                                             # a malformed FASTQ
        ctx.depth_files(paths, [str(tmp_path / "recs.fa"), str(tmp_path / "bad.fq")], str(tmp_path / "no"))
    assert e.value.code == sp.ERR_FORMAT
    r = cli("-D", "bad.fq", "-f", "bank.txt", "-o", "no")
    assert r.returncode == 1 and "Depth failed" in r.stdout
    assert not outputs(tmp_path, "no")


@pytest.mark.gpu
def test_depth_files_at_a_common_rate_and_its_refusals(ctx, tmp_path):
    from oracle import oracle_py as orc
    refs, recs = tc.file_case()
    sketch = lambda i, s: ctx.sketch_text(b">ref%d\n" % i + refs[i] + b"\n", tc.K_FILE, tc.M_FILE, s)[0]
    paths = tp.write_files(tmp_path, [sketch(i, 1.0 if i % 2 else 4.0) for i in range(len(refs))])
    coarse = [tp.key_set(sketch(i, 4.0)) for i in range(len(refs))]
    (tmp_path / "recs.fa").write_bytes(tc.fasta_of(recs))
    reads = [str(tmp_path / "recs.fa")]
    with pytest.raises(sp.SpspError) as e:                                             # the reads are scanned at one threshold
        ctx.depth_files(paths, reads, str(tmp_path / "no"))
    assert e.value.code == sp.ERR_ARG and "rate" in str(e.value)
    want = model(coarse, [x for _, _, seq in recs for x in tc.record_keys(seq, 4.0)])
    for rate, tag in ((4.0, "r4"), ("auto", "auto")):
        rows, totals = ctx.depth_files(paths, reads, str(tmp_path / tag), rate=rate)
        assert (as_tuples(rows), as_totals(totals)) == want[:2] and depth_file(tmp_path, tag) == py_csv(want[0], paths)
    kk = [orc.sketch_fasta(b">g\n" + g[:500] + b"\n", 11, 11, 4.0)[0] for g in refs[:2]]
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.depth_files(tp.write_files(tmp_path, kk, "kk"), reads, str(tmp_path / "no"), rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    assert not outputs(tmp_path, "no")


@pytest.mark.gpu
def test_65537_records_cross_the_batch_seam(ctx, tmp_path):
    """one scan, two key extractions (65 535 records and 2): a key held by records 0, 65 534, 65 535 and 65 536 has c = 4"""
    n_rec, s = 65537, 1.0
    rng = np.random.default_rng(13)
    refs = [tc.random_bases(rng, 3000) for _ in range(2)]
    marked = refs[0][100:140]
    seq_of = lambda r: marked if r in (0, 65534, 65535, 65536) else refs[1][(r * 7) % 2960:(r * 7) % 2960 + 40]
    (tmp_path / "many.fa").write_bytes(b"".join(b">r%d\n%s\n" % (r, seq_of(r)) for r in range(n_rec)))
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, s)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    ref_sets = [tp.key_set(p) for p in payloads]
    reads, keys_of = Counter(), {}
    for r in range(n_rec):
        q = seq_of(r)
        if q not in keys_of:
            keys_of[q] = tc.record_keys(q, s)
        reads.update(keys_of[q])
    want_rows, want_totals, c = model(ref_sets, reads)
    assert keys_of[marked] and all(c[x] == 4 for x in keys_of[marked]) and want_rows[0][1] > 0 and want_rows[0][3:5] == (4, 4)
    rows, totals = ctx.depth_files(paths, [str(tmp_path / "many.fa")], str(tmp_path / "many"))
    assert as_tuples(rows) == want_rows and as_totals(totals) == want_totals
