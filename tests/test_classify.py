"""Classify: the records of a sequence file assigned to the references of an index (include/spsp.h: spsp_classify_index_device,
spsp_classify_device, spsp_classify_plan_host, spsp_classify_csv_host, spsp_classify_summary_csv_host, spsp_classify_files;
bin/comparator -X).

The rule, on sets of the comparator's keys.  References 0 .. R-1 with key sets K_j, record r with key set Q_r:

    shared(r, j) = |Q_r & K_j|        hit_keys(r) = the keys of Q_r that some K_j holds
    j passes for r when shared >= min_keys and shared * den >= num * |Q_r|
    listed: the best min(top, passing) passing references by (-shared, j)

Every expected value below comes from `model`: literal set intersections and sorted(..., key=(-shared, reference)) over Python
integers.  No tolerance anywhere.

Where the kernels cut, and the shapes that sit on the cuts (classify_plan names the numbers): a record is tallied by one wave while
its work -- the sum of its keys' holder counts -- is at most small_work, by a workgroup with a counter per reference beyond; those
counters sit in LDS up to lds_refs references and in device memory above; in the workgroup form a list of more than list_cut
holders is walked by a whole wave.  Every kernel works in waves of 64 over consecutive keys or records."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
import test_prevalence as tp
from oracle import oracle_py as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
HEADER = "record,name,length,keys,hit_keys,rank,match,shared,f_shared,passing\n"
SUMMARY_HEADER = "reference,records_best,bases_best,keys_best,records_listed\n"


# -------------------------------------------------------------------------------------------------- the model

def model(refs, recs, top=1, min_keys=1, num=0, den=1):
    """refs, recs: one collection of key tuples each -> per record (keys, hit_keys, passing, [(reference, shared), ...])"""
    refs = [set(K) for K in refs]
    union = set().union(*refs) if refs else set()
    out = []
    for q in recs:
        q = set(q)
        shared = [(len(q & K), j) for j, K in enumerate(refs)]
        ok = [(x, j) for x, j in shared if x >= min_keys and x * den >= num * len(q)]
        best = sorted(ok, key=lambda t: (-t[0], t[1]))[:top]
        out.append((len(q), len(q & union), len(ok), [(j, x) for x, j in best]))
    return out


def as_arrays(rows, top, lengths=None):
    records = np.zeros(len(rows), dtype=sp.CLASSIFY_RECORD_DTYPE)
    hits = np.zeros((len(rows), top), dtype=sp.CLASSIFY_HIT_DTYPE)
    for r, (keys, hit, passing, best) in enumerate(rows):
        records[r] = (lengths[r] if lengths else 0, keys, hit, passing, len(best))
        for i, (j, x) in enumerate(best):
            hits[r, i] = (j, x)
    return records, hits


def as_rows(records, hits):
    out = []
    for rec, h in zip(records, hits):
        n = int(rec["listed"])
        assert not h[n:]["reference"].any() and not h[n:]["shared"].any(), "slots behind `listed` are zero"
        out.append((int(rec["keys"]), int(rec["hit_keys"]), int(rec["passing"]), [(int(x["reference"]), int(x["shared"])) for x in h[:n]]))
    return out


def py_csv(rows, names, lengths, ref_names, precision=6):
    text = HEADER
    for r, ((keys, hit, passing, best), name, length) in enumerate(zip(rows, names, lengths)):
        front = "%d,%s,%d,%d,%d," % (r, name, length, keys, hit)
        if not best:
            text += front + "0,,0,0,%d\n" % passing
        for i, (j, x) in enumerate(best):
            text += front + "%d,%s,%d,%s,%d\n" % (i + 1, ref_names[j], x, "%.*g" % (precision, x / keys) if keys else "0", passing)
    return text.encode()


def py_summary_csv(rows, lengths, ref_names):
    best_n, bases, keys, listed = ([0] * len(ref_names) for _ in range(4))
    none = none_bases = 0
    for (_, _, _, best), length in zip(rows, lengths):
        if not best:
            none, none_bases = none + 1, none_bases + length
            continue
        j, x = best[0]
        best_n[j] += 1; bases[j] += length; keys[j] += x
        for j, _ in best:
            listed[j] += 1
    text = SUMMARY_HEADER
    for j, name in enumerate(ref_names):
        text += "%s,%d,%d,%d,%d\n" % (name, best_n[j], bases[j], keys[j], listed[j])
    return (text + "unclassified,%d,%d,0,0\n" % (none, none_bases)).encode()


# ------------------------------------------------------------------------------------------------ not GPU

def K(*xs):
    return {(x, 0, x) for x in xs}


def test_model_on_a_hand_made_case():
    refs = [K(1, 2, 3, 4), K(3, 4, 5), K(9), K(1, 2, 3, 4)]
    recs = [K(1, 2, 3, 4, 5, 77), K(), K(77, 78), K(9), K(3, 4)]
    # record 0: shared = 4, 3, 0, 4 -> references 0 and 3 tie and 0 comes first; hit keys 1..5
    assert model(refs, recs, top=1) == [(6, 5, 3, [(0, 4)]), (0, 0, 0, []), (2, 0, 0, []), (1, 1, 1, [(2, 1)]), (2, 2, 3, [(0, 2)])]
    assert model(refs, recs[:1], top=2)[0][3] == [(0, 4), (3, 4)] and model(refs, recs[:1], top=64)[0][3] == [(0, 4), (3, 4), (1, 3)]
    assert model(refs, recs[:1], top=2, min_keys=4)[0][2:] == (2, [(0, 4), (3, 4)])
    assert model(refs, recs[:1], top=3, num=2, den=3)[0][2:] == (2, [(0, 4), (3, 4)])     # 4 * 3 >= 2 * 6 passes at equality, 3 * 3 < 12
    assert model(refs, recs[:1], top=3, num=1, den=2)[0][2] == 3                          # 3 * 2 >= 1 * 6: equality again
    assert model(refs, recs[:1], top=3, num=1, den=1)[0][2:] == (0, [])
    assert model(refs, recs[4:], top=3, num=1, den=1)[0][2:] == (3, [(0, 2), (1, 2), (3, 2)])
    assert model(refs, recs[1:2], num=1, den=1)[0] == (0, 0, 0, [])                        # min_keys >= 1 keeps the record without keys out


def test_abi_has_the_classify_calls():
    calls = ("spsp_classify_index_device", "spsp_classify_device", "spsp_classify_plan_host", "spsp_classify_csv_host",
             "spsp_classify_summary_csv_host", "spsp_classify_files", "spsp_classify_stage_ms")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    assert sp.CLASSIFY_RECORD_DTYPE.itemsize == 24 and sp.CLASSIFY_HIT_DTYPE.itemsize == 8
    assert sp.CLASSIFY_RECORD_DTYPE.names == ("length", "keys", "hit_keys", "passing", "listed")
    for name in calls:
        assert hasattr(sp.lib(), name)


def internal_constants():
    import re
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    value = lambda name: re.search(r"constexpr uint32_t %s = ([^;]+);" % name, text).group(1)
    lds = eval(value("kAcLdsBytes"))
    return {"small_work": int(value("kCfSmallWork")), "lds_refs": eval(value("kCfLdsRefs").replace("kAcLdsBytes", str(lds)).replace("/", "//")),
            "list_cut": int(value("kCfListCut"))}


def test_classify_plan_is_the_constants_of_the_kernels():
    want = internal_constants()
    assert want == {"small_work": 1024, "lds_refs": 38912, "list_cut": 32}
    for n_ref, top in ((1, 1), (38912, 64), (38913, 2), (65535, 64)):
        plan = sp.classify_plan(n_ref, top)
        assert {f: plan[f] for f in want} == want and plan["counters_in_lds"] == (n_ref <= want["lds_refs"])
    assert 4 * want["lds_refs"] + 8 * 64 * 8 + 64 <= 160 * 1024                        # the counters beside the kept matches
    for n_ref, top in ((0, 1), (65536, 1), (5, 0), (5, 65)):
        with pytest.raises(sp.SpspError) as e:
            sp.classify_plan(n_ref, top)
        assert e.value.code == sp.ERR_ARG


ROWS = [(6, 5, 3, [(0, 4), (3, 4)]), (0, 0, 0, []), (2, 0, 0, []), (1, 1, 1, [(2, 1)]), (7, 7, 5, [(1, 7), (0, 3)])]
NAMES = ["contig_1", "r/2", "", "read.4", "x"]
LENGTHS = [5000, 12, 150, 40, (1 << 40) + 7]
REFS = ["a one.fa.gz", "dir/b.two", "c", "d.1.2.sketch"]


def test_both_csv_writers_equal_the_python_writers():
    records, hits = as_arrays(ROWS, 2, LENGTHS)
    for precision in (6, 3):
        assert sp.classify_csv(records, hits, NAMES, REFS, 2, precision) == py_csv(ROWS, NAMES, LENGTHS, REFS, precision)
    lines = sp.classify_csv(records, hits, NAMES, REFS, 2).decode().splitlines()
    assert lines[1] == "0,contig_1,5000,6,5,1,a one.fa.gz,4,0.666667,3" and lines[2] == "0,contig_1,5000,6,5,2,d.1.2.sketch,4,0.666667,3"
    assert lines[3] == "1,r/2,12,0,0,0,,0,0,0" and lines[4] == "2,,150,2,0,0,,0,0,0" and len(lines) == 8
    assert sp.classify_summary_csv(records, hits, REFS, 2) == py_summary_csv(ROWS, LENGTHS, REFS)
    assert sp.classify_summary_csv(records, hits, REFS, 2).decode().splitlines()[1:] == [
        "a one.fa.gz,1,5000,4,2", "dir/b.two,1,%d,7,1" % LENGTHS[4], "c,1,40,1,1", "d.1.2.sketch,0,0,0,1", "unclassified,2,162,0,0"]
    none = as_arrays([], 2)
    assert sp.classify_csv(*none, [], REFS, 2) == HEADER.encode()
    assert sp.classify_summary_csv(*none, REFS, 2) == py_summary_csv([], [], REFS)


def test_both_csv_writers_refuse_rows_that_contradict_themselves():
    bad = [(6, 5, 1, [(0, 4), (3, 4)]),            # listed > passing
           (6, 7, 3, [(0, 4)]),                    # hit_keys > keys
           (6, 3, 3, [(0, 4)]),                    # shared > hit_keys
           (6, 5, 3, [(3, 4), (0, 4)]),            # equal shared, the higher reference first
           (6, 5, 3, [(0, 3), (3, 4)]),            # shared rising
           (6, 5, 3, [(0, 4), (0, 4)]),            # one reference twice
           (6, 5, 3, [(4, 4)]),                    # reference >= R
           (6, 5, 3, [(0, 0)])]                    # a listed match that shares nothing
    for row in bad:
        records, hits = as_arrays([ROWS[3], row], 2, [1, 2])
        for call in (lambda: sp.classify_csv(records, hits, ["a", "b"], REFS, 2), lambda: sp.classify_summary_csv(records, hits, REFS, 2)):
            with pytest.raises(sp.SpspError) as e:
                call()
            assert e.value.code == sp.ERR_ARG and "record 1" in str(e.value), row
    records, hits = as_arrays([(6, 5, 3, [(0, 4), (3, 4)])], 2, [1])
    records["listed"] = 3                                                              # listed > top
    for call in (lambda: sp.classify_csv(records, np.zeros((1, 2), sp.CLASSIFY_HIT_DTYPE), ["a"], REFS, 2),
                 lambda: sp.classify_summary_csv(records, np.zeros((1, 2), sp.CLASSIFY_HIT_DTYPE), REFS, 2),
                 lambda: sp.classify_csv(*as_arrays(ROWS[:1], 65, [1]), ["a"], REFS, 65),
                 lambda: sp.classify_csv(*as_arrays(ROWS[:1], 2, [1]), ["a"], [], 2)):
        with pytest.raises(sp.SpspError) as e:
            call()
        assert e.value.code == sp.ERR_ARG


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    (tmp_path / "labels.txt").write_text("a\nb\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-X", "r.fa", o, v) for o, v in (("-q", "list.txt"), ("-g", "3"), ("-c", "0.5"), ("-C", "0.5"), ("-N", "5"), ("-P", "0.9"), ("-r", "0.9"),
                                                ("-R", "0.9"), ("-l", "0.5"), ("-L", "0.5"), ("-S", "union"), ("-E", "union"), ("-J", "0.5"), ("-K", "0.5"), ("-A", "10"), ("-G", "labels.txt"))]
    cases += [("-Y", "3"), ("-V", "2"), ("-I", "0.5")]
    cases += [("-X", "r.fa", "-Y", v) for v in ("0", "65", "abc", "")] + [("-X", "r.fa", "-V", v) for v in ("0", "-1", "x")]
    cases += [("-X", "r.fa", "-I", v) for v in ("1.5", "abc", "0.1234567", "-0.5")]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1, (args, r.stdout, r.stderr)
        assert any(o in r.stdout for o in ("-X", "-Y", "-V", "-I")), (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


def test_host_functions_under_the_sanitizers():
    """tests/tools/classify_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the
    plan and the two CSV writers with their refusals (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "classify_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "classify_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


class Index:
    """the references on the device and the context's index over them; the tensors live as long as the object"""

    def __init__(self, ctx, k, refs):
        mn, lo, hi, off, self.refs = tp.pack(refs, k)
        self.d = tp.upload(mn, lo, hi)
        self.k, self.off = k, off
        ctx.classify_index_device(k, tp.ptr(self.d[0]), tp.ptr(self.d[1]), tp.ptr(self.d[2]), off, len(refs))


def run(ctx, k, recs, top=1, min_keys=1, num=0, den=1, shuffle=0):
    """records -> rows as the model's; shuffle: a seed for the order of the keys inside every record (0: sorted)"""
    mn, lo, hi, off, order = tp.pack(recs, k)
    if shuffle:
        rng = np.random.default_rng(shuffle)
        perm = np.concatenate([int(a) + rng.permutation(int(z) - int(a)) for a, z in zip(off[:-1], off[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
        mn, lo, hi = mn[perm], lo[perm], (hi[perm] if hi is not None else None)
    d = tp.upload(mn, lo, hi)
    records, hits = ctx.classify_device(tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, top, min_keys, num, den)
    del d
    assert not records["length"].any()
    return as_rows(records, hits)


def check(ctx, k, refs, recs, tops=(1, 2, 64), rules=((1, 0, 1),), index=None, shuffle=0):
    index = index or Index(ctx, k, refs)
    for top in tops:
        for min_keys, num, den in rules:
            got, want = run(ctx, k, recs, top, min_keys, num, den, shuffle), model(refs, recs, top, min_keys, num, den)
            assert got == want, (top, min_keys, num, den, [(r, a, b) for r, (a, b) in enumerate(zip(got, want)) if a != b][:3])
    return index


def work_of(refs, rec):
    return sum(sum(x in set(Kj) for Kj in refs) for x in set(rec))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_records_without_keys_without_hits_and_no_records(ctx, k):
    p, stranger = tp.pool(40, k), tp.pool(30, k, salt=700_000)
    refs = [p[:20], p[10:40], []]
    index = check(ctx, k, refs, [[], stranger[:5], p[:3], [], stranger[5:], []])
    check(ctx, k, refs, [[]], index=index)
    check(ctx, k, refs, [[], [], []], index=index)
    records, hits = ctx.classify_device(None, None, None, [0], 1)                      # no record at all
    assert len(records) == 0 and len(hits) == 0
    check(ctx, k, [p], [p[:7], stranger[:3], p[5:9] + stranger[:2]])                   # R = 1
    check(ctx, k, [[], []], [p[:3], []])                                               # an index without a key


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_largest_index_and_a_key_everybody_holds(ctx, k):
    R = 65535
    own = tp.pool(R + 2, k)
    refs = [[own[j]] + ([own[R]] if j == 65534 else []) for j in range(R)]
    index = check(ctx, k, refs, [[own[65534], own[R], own[5]], [own[R + 1]], [own[0], own[65534]]], tops=(1, 2))
    got = run(ctx, k, [[own[65534], own[R], own[5]]], top=2)
    assert got == [(3, 3, 2, [(65534, 2), (5, 1)])]
    del index
    # one key in every reference: h = R on one list, 65 535 references tie at shared = 1 and the lowest numbers are listed
    refs = [[own[R]] + ([own[j]] if j % 2 else []) for j in range(R)]
    index = check(ctx, k, refs, [[own[R]], [own[R], own[65533]], [own[R + 1]]], tops=(1, 64))
    assert run(ctx, k, [[own[R], own[65533]]], top=3) == [(2, 2, R, [(65533, 2), (0, 1), (1, 1)])]
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_ties_and_the_top_cut(ctx, k):
    p = tp.pool(400, k)
    # references 0..69 all share keys 0..9 with the record; 10..19 two more, 3 one more: ties across every cut, 70 passing > 64
    refs = [p[:10] + (p[10:12] if 10 <= j < 20 else []) + (p[12:13] if j == 3 else []) + [p[100 + j]] for j in range(70)]
    recs = [p[:13], p[:10], p[10:12], p[12:13], p[5:6] + p[200:203]]
    index = check(ctx, k, refs, recs, shuffle=7)
    assert run(ctx, k, recs[:1], top=2) == [(13, 13, 70, [(10, 12), (11, 12)])]
    for n_pass in (1, 2, 3, 63, 64, 65):                                               # passing below, at and above top = 1, 2, 64
        sub = [p[:10] if j < n_pass else [p[100 + j]] for j in range(70)]
        check(ctx, k, sub, [p[:10], p[3:4]])
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_thresholds_at_equality_and_one_short(ctx, k):
    p = tp.pool(100, k)
    refs = [p[:6], p[:5], p[:4] + p[50:60], p[20:30]]
    recs = [p[:6] + p[90:93], p[:4], p[20:30] + p[:2]]                                 # 9 keys: shared 6, 5, 4, 0
    rules = [(1, 6, 9), (1, 2, 3), (1, 5, 9), (1, 6, 10), (6, 0, 1), (5, 0, 1), (7, 0, 1), (11, 0, 1), (1, 1, 1), (1, 999_999, 1_000_000), (4, 4, 9), (5, 4, 9),
             (1, 0, 1_000_000), (1, 1_000_000, 1_000_000)]
    index = check(ctx, k, refs, recs, tops=(1, 3), rules=rules)
    got = [run(ctx, k, recs[:1], 3, mk, num, den)[0][2] for mk, num, den in ((1, 6, 9), (1, 2, 3), (1, 5, 9), (7, 0, 1), (1, 1, 1))]
    assert got == [1, 1, 2, 0, 0]
    assert run(ctx, k, recs[1:2], 3, 1, 1, 1)[0][2:] == (3, [(0, 4), (1, 4), (2, 4)])     # num = den: the record inside the reference
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_one_record_of_70000_keys_in_one_reference(ctx, k):
    p = tp.pool(70_000, k)
    refs = [p[:10], p, p[69_990:]]
    index = Index(ctx, k, refs)
    got = run(ctx, k, [p, p[:100]], top=3, shuffle=3)
    assert got == [(70_000, 70_000, 3, [(1, 70_000), (0, 10), (2, 10)]), (100, 100, 2, [(1, 100), (0, 10)])]
    assert run(ctx, k, [p], top=1, min_keys=70_000, num=1, den=1) == [(70_000, 70_000, 1, [(1, 70_000)])]
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_records_whose_work_sits_on_the_routing_capacities(ctx, k):
    plan = sp.classify_plan(40, 64)
    W, cut = plan["small_work"], plan["list_cut"]
    R = 40
    p = tp.pool(3000, k)
    # key i < 500 is held by references 0 .. h(i)-1 with h(i) = 1 + i % R; the keys behind are held by reference i % R alone
    refs = [[p[i] for i in range(500) if j < 1 + i % R] + [p[i] for i in range(500, 3000) if i % R == j] for j in range(R)]

    def rec_of_work(target):
        keys, w = [], 0
        for i in range(500):                                                           # the shared keys while they fit, then keys of one holder
            if w + 1 + i % R <= target:
                keys.append(p[i]); w += 1 + i % R
        i = 500
        while w < target:
            keys.append(p[i]); w += 1; i += 1
        assert work_of(refs, keys) == target
        return keys

    recs = [rec_of_work(W - 1), rec_of_work(W), rec_of_work(W + 1), rec_of_work(2 * W), rec_of_work(64), rec_of_work(65)]
    # lists of exactly list_cut and list_cut + 1 holders in a record that takes the workgroup form
    recs += [[p[cut - 1], p[cut]] + p[500:500 + W], [p[cut - 1]] + p[500:500 + W], [p[cut]] + p[500:500 + W]]
    assert 1 + (cut - 1) % R == cut and 1 + cut % R == cut + 1
    index = check(ctx, k, refs, recs, shuffle=11)
    mixed = [recs[2], [], recs[0], tp.pool(9, k, salt=900_000), recs[3], recs[4], p[7:8], recs[6]] * 3      # every form in one batch
    check(ctx, k, refs, mixed, tops=(2,), index=index)
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_counters_in_lds_and_in_device_memory(ctx, k):
    plan = sp.classify_plan(1, 1)
    for R in (plan["lds_refs"], plan["lds_refs"] + 1):
        assert sp.classify_plan(R, 1)["counters_in_lds"] == (R == plan["lds_refs"])
        own = tp.pool(R + 1, k)
        refs = [[own[j]] + ([own[R]] if j >= R - 3 else []) for j in range(R)]
        big = own[R - 1200:R + 1]                                                      # work 1 203 > small_work: the last references, the very last index
        assert work_of(refs[R - 1300:], big) > plan["small_work"]
        index = Index(ctx, k, refs)
        got = run(ctx, k, [big, own[:3], big[600:]], top=4)
        assert got[0] == (1201, 1201, 1200, [(R - 3, 2), (R - 2, 2), (R - 1, 2), (R - 1200, 1)])
        assert got[1] == (3, 3, 3, [(0, 1), (1, 1), (2, 1)]) and got[2] == (601, 601, 600, [(R - 3, 2), (R - 2, 2), (R - 1, 2), (R - 600, 1)])
        # twice on one workgroup's row: the counters are cleared between the records
        assert run(ctx, k, [big] * 3 + [big[1:]], top=4)[3] == (1200, 1200, 1199, [(R - 3, 2), (R - 2, 2), (R - 1, 2), (R - 1199, 1)])
        del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_record_counts_and_key_runs_on_wave_boundaries(ctx, k):
    p = tp.pool(700, k)
    refs = [p[:300], p[100:500], p[250:260], p[::3]]
    index = Index(ctx, k, refs)
    for n_rec in (63, 64, 65):
        recs = [p[(7 * r) % 300:(7 * r) % 300 + 1 + r % 5] for r in range(n_rec)]
        check(ctx, k, refs, recs, tops=(2,), index=index)
    lengths = [63, 64, 65, 1, 127, 128, 129, 0, 255, 256, 257, 30, 34]                # runs that end on, before and behind a 64-lane chunk
    recs = [p[17 * i:17 * i + c] for i, c in enumerate(lengths)]
    check(ctx, k, refs, recs, tops=(1, 4), index=index, shuffle=5)
    check(ctx, k, refs, recs[::-1], tops=(4,), index=index)
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_smallest_table(ctx, k, monkeypatch):
    refs = [tp.pool(512, k, salt=1000 * j) for j in range(8)]                          # 4 096 entries, 4 096 distinct keys, 4 096 slots
    recs = [tp.pool(40, k, salt=500_000), refs[3][:100] + tp.pool(30, k, salt=600_000), refs[0][500:] + refs[1][:12], refs[7] + refs[6] + refs[5]]
    index = check(ctx, k, refs, recs, tops=(3,))
    plain = run(ctx, k, recs, 3)
    del index
    monkeypatch.setenv("SPSP_DEBUG_PREVALENCE_TABLE", "min")
    index = check(ctx, k, refs, recs, tops=(3,))
    assert run(ctx, k, recs, 3) == plain
    del index


@pytest.mark.gpu
def test_two_batches_on_one_index_and_an_index_that_was_replaced(ctx):
    k = 31
    p = tp.pool(300, k)
    refs = [p[:100], p[50:200], p[150:300]]
    index = Index(ctx, k, refs)
    a, b = [p[:60], p[140:160]], [p[190:300], p[40:55], []]
    first = run(ctx, k, a, 3)
    assert first == model(refs, a, 3) and run(ctx, k, b, 3) == model(refs, b, 3) and run(ctx, k, a, 3) == first
    with pytest.raises(sp.SpspError) as e:                                             # k > 32 keys against an index of k <= 32
        run(ctx, 63, [tp.pool(5, 63)])
    assert e.value.code == sp.ERR_ARG and run(ctx, k, a, 3) == first
    for args in ((0, 1, 0, 1), (65, 1, 0, 1), (1, 0, 0, 1), (1, 1, 2, 1), (1, 1, 0, 0), (1, 1, 0, 1_000_001)):
        with pytest.raises(sp.SpspError) as e:
            run(ctx, k, a, *args)
        assert e.value.code == sp.ERR_ARG
    assert run(ctx, k, a, 3) == first
    ctx.timing_enable(True)                                                            # events between the launches: the same answer, four times
    ctx.classify_stage_ms()
    assert run(ctx, k, a, 3) == first
    ms = ctx.classify_stage_ms()
    ctx.timing_enable(False)
    assert list(ms) == ["probe", "route", "wave_form", "workgroup_form"] and all(v > 0 for v in ms.values())
    assert run(ctx, k, a, 3) == first and not any(ctx.classify_stage_ms().values())
    ctx.prevalence_device(k, tp.ptr(index.d[0]), tp.ptr(index.d[1]), None, index.off, 3, 1, 2)
    with pytest.raises(sp.SpspError) as e:
        run(ctx, k, a, 3)
    assert e.value.code == sp.ERR_ARG and "index" in str(e.value)
    index = Index(ctx, k, refs)
    assert run(ctx, k, a, 3) == first
    fresh = sp.Context(0)
    with pytest.raises(sp.SpspError) as e:                                             # never built
        run(fresh, k, a, 3)
    fresh.close()
    assert e.value.code == sp.ERR_ARG
    with pytest.raises(sp.SpspError) as e:                                             # an index of no reference
        ctx.classify_index_device(k, None, None, None, [0], 0)
    assert e.value.code == sp.ERR_ARG
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_against_the_query_mode_comparison(ctx, k):
    import torch
    rng = random.Random(5)
    p = tp.pool(4000, k)
    refs = [rng.sample(p, rng.randint(0, 400)) for _ in range(50)]
    recs = [rng.sample(p, rng.randint(0, 120)) + tp.pool(rng.randint(0, 5), k, salt=10 ** 6 + 10 * r) for r in range(100)]
    mn, lo, hi, off, order = tp.pack(recs + refs, k)
    d = tp.upload(mn, lo, hi)
    inter = torch.zeros((150, 150), dtype=torch.int32, device="cuda")
    ctx.compare_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, 150, 0, 1, inter.data_ptr(), n_query=100)
    torch.cuda.synchronize()
    cells = inter.cpu().numpy()[:100, 100:]
    # the index over the references' part of the same arrays, the records' part as the records
    ctx.classify_index_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off[100:], 50)
    records, hits = ctx.classify_device(tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off[:101], 64)
    got = as_rows(records, hits)
    assert got == model(refs, recs, 64)
    for r, (_, _, passing, best) in enumerate(got):
        assert passing == int((cells[r] > 0).sum()) and all(cells[r, j] == x for j, x in best)
        assert [j for j, _ in best] == sorted(np.nonzero(cells[r])[0].tolist(), key=lambda j: (-int(cells[r, j]), j))[:64]
    del d


# ------------------------------------------------------------------------------------------ files and the command line

K_FILE, M_FILE = 31, 11


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist())


def mutated(rng, seq, rate):
    out = bytearray(seq)
    for i in np.nonzero(rng.random(len(seq)) < rate)[0]:
        out[i] = b"ACGT"[(b"ACGT".index(out[i]) + 1 + int(rng.integers(3))) % 4]
    return bytes(out)


def file_case():
    """three random 3 kbp references and a mutated copy of each; 60 records: slices of 20 .. 2000 bases of the references (some
    shorter than k) and sequences from no reference, named with a description behind the first word"""
    rng = np.random.default_rng(11)
    anc = [random_bases(rng, 3000) for _ in range(3)]
    refs = anc + [mutated(rng, a, 0.02) for a in anc]
    recs = []
    for r in range(60):
        n = int(rng.choice([20, 30, 31, 40, 45, 100, 150, 600, 2000]))
        if r % 5 == 4:
            seq = random_bases(rng, n)
        else:
            src = refs[int(rng.integers(len(refs)))]
            a = int(rng.integers(len(src) - n + 1))
            seq = src[a:a + n]
        recs.append(("rec%d" % r, "len=%d\tslice %d" % (n, r), seq))
    return refs, recs


def fasta_of(recs, width=70):
    out = b""
    for i, (name, rest, seq) in enumerate(recs):
        out += b">" + name.encode() + (b" " + rest.encode() if i % 3 else b"") + b"\n"
        out += b"".join(seq[a:a + width] + b"\n" for a in range(0, len(seq), width)) if i % 2 else seq + b"\n"
    return out


def fastq_of(recs):
    return b"".join(b"@" + name.encode() + b" " + rest.encode() + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n" for name, rest, seq in recs)


def record_keys(seq, s):
    return tp.key_set(orc.sketch_fasta(b">r\n" + seq + b"\n", K_FILE, M_FILE, s)[0])


def both_files(root, tag):
    return [tp.gunzip(os.path.join(str(root), tag + suf)) for suf in ("_classify.csv.gz", "_classify_summary.csv.gz")]


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1.0, 4.0])
def test_classify_files_and_the_command_line(ctx, tmp_path, s):
    refs, recs = file_case()
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", K_FILE, M_FILE, s)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    ref_sets = [tp.key_set(p) for p in payloads]
    rec_sets = [record_keys(seq, s) for _, _, seq in recs]
    names, lengths = [n for n, _, _ in recs], [len(seq) for _, _, seq in recs]
    assert any(len(q) == 0 for q in rec_sets) and sum(1 for q in rec_sets if q) > 30
    (tmp_path / "recs.fa").write_bytes(fasta_of(recs))
    with gzip.open(str(tmp_path / "recs.fq.gz"), "wb") as f:
        f.write(fastq_of(recs))
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    cli = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    for tag, (top, min_keys, num, den, frac), records_file in (("a", (1, 1, 0, 1, None), "recs.fa"), ("b", (3, 2, 1, 10, "0.1"), "recs.fq.gz"),
                                                               ("c", (64, 1, 1, 1, "1"), "recs.fa")):
        rows = model(ref_sets, rec_sets, top, min_keys, num, den)
        assert tag != "a" or sum(1 for r in rows if r[3]) > 20
        records, hits = ctx.classify_files(paths, str(tmp_path / records_file), str(tmp_path / ("lib" + tag)), top, min_keys, num, den)
        assert as_rows(records, hits) == rows and records["length"].tolist() == lengths
        texts = [py_csv(rows, names, lengths, paths), py_summary_csv(rows, lengths, paths)]
        assert both_files(tmp_path, "lib" + tag) == texts
        args = ["-X", records_file, "-f", "bank.txt", "-o", "cli" + tag] + (["-Y", str(top)] if top != 1 else []) + (["-V", str(min_keys)] if min_keys != 1 else [])
        r = cli(*(args + (["-I", frac] if frac else [])))
        assert r.returncode == 0, r.stdout + r.stderr
        assert both_files(tmp_path, "cli" + tag) == texts
        assert not [f for f in os.listdir(tmp_path) if f.startswith("cli" + tag) and ("jaccard" in f or "containment" in f)]
    ctx.classify_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / "p3"), 3, precision=3)
    rows = model(ref_sets, rec_sets, 3)
    assert both_files(tmp_path, "p3") == [py_csv(rows, names, lengths, paths, 3), py_summary_csv(rows, lengths, paths)]
    # bases in front of the first header are a record of the device ingest and no header line of the host's: refused as a format error
    (tmp_path / "headless.fa").write_bytes(recs[5][2] + b"\n" + fasta_of(recs[:3]))
    with pytest.raises(sp.SpspError) as e:
        ctx.classify_files(paths, str(tmp_path / "headless.fa"), str(tmp_path / "no"))
    assert e.value.code == sp.ERR_FORMAT and "3 header line(s)" in str(e.value) and "4 record(s)" in str(e.value)
    with pytest.raises(sp.SpspError):                                                  # a records file that is not there
        ctx.classify_files(paths, str(tmp_path / "none.fa"), str(tmp_path / "no"))
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
def test_classify_files_at_a_common_rate_and_its_refusals(ctx, tmp_path):
    refs, recs = file_case()
    sketch = lambda i, s: ctx.sketch_text(b">ref%d\n" % i + refs[i] + b"\n", K_FILE, M_FILE, s)[0]
    mixed_rates = [sketch(i, 1.0 if i % 2 else 4.0) for i in range(len(refs))]
    coarse = [sketch(i, 4.0) for i in range(len(refs))]
    paths = tp.write_files(tmp_path, mixed_rates)
    (tmp_path / "recs.fa").write_bytes(fasta_of(recs))
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    names, lengths = [n for n, _, _ in recs], [len(seq) for _, _, seq in recs]
    with pytest.raises(sp.SpspError) as e:                                             # the records are scanned at one threshold
        ctx.classify_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / "no"), 2)
    assert e.value.code == sp.ERR_ARG and "rate" in str(e.value)
    rows = model([tp.key_set(p) for p in coarse], [record_keys(seq, 4.0) for _, _, seq in recs], 2)
    for rate, tag in ((4.0, "r4"), ("auto", "auto")):
        records, hits = ctx.classify_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / tag), 2, rate=rate)
        assert as_rows(records, hits) == rows
        assert both_files(tmp_path, tag) == [py_csv(rows, names, lengths, paths), py_summary_csv(rows, lengths, paths)]
    r = subprocess.run([EXE, "-X", "recs.fa", "-f", "bank.txt", "-Y", "2", "-s", "4", "-o", "cli"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and both_files(tmp_path, "cli") == both_files(tmp_path, "r4"), r.stdout + r.stderr
    r = subprocess.run([EXE, "-X", "recs.fa", "-f", "bank.txt", "-o", "no"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "rate" in r.stdout
    kk = [orc.sketch_fasta(b">g\n" + g[:500] + b"\n", 11, 11, 4.0)[0] for g in refs[:2]]
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.classify_files(tp.write_files(tmp_path, kk, "kk"), str(tmp_path / "recs.fa"), str(tmp_path / "no"), rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
def test_65537_records_cross_the_batch_seam(ctx, tmp_path):
    """one scan, two key extractions (65 535 records and 2): the rows of the records on both sides of the seam"""
    n_rec, s = 65537, 1.0
    rng = np.random.default_rng(13)
    refs = [random_bases(rng, 3000) for _ in range(2)]
    seq_of = lambda r: refs[r % 2][(r * 7) % 2960:(r * 7) % 2960 + 40]
    special = {65534: seq_of(65534), 65535: seq_of(65535), 65536: random_bases(rng, 40), 0: random_bases(rng, 40)}
    seqs = [special.get(r) or seq_of(r) for r in range(n_rec)]
    (tmp_path / "many.fa").write_bytes(b"".join(b">r%d\n%s\n" % (r, q) for r, q in enumerate(seqs)))
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", K_FILE, M_FILE, s)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    records, hits = ctx.classify_files(paths, str(tmp_path / "many.fa"), str(tmp_path / "many"), 2)
    assert len(records) == n_rec and (records["length"] == 40).all()
    ref_sets = [tp.key_set(p) for p in payloads]
    sample = sorted(set([0, 1, 2, 65533, 65534, 65535, 65536] + rng.integers(0, n_rec, 12).tolist()))
    want = model(ref_sets, [record_keys(seqs[r], s) for r in sample], 2)
    assert as_rows(records[sample], hits[sample]) == want
    assert want[sample.index(65534)][3][0][0] == 0 and want[sample.index(65535)][3][0][0] == 1 and want[sample.index(65536)][3] == [] and want[0][3] == []
    lines = tp.gunzip(str(tmp_path / "many_classify.csv.gz")).decode().splitlines()
    assert len(lines) == 1 + int(np.maximum(records["listed"], 1).sum()) and lines[-1].startswith("65536,r65536,40,") and lines[-1].endswith(",0,,0,0,0")
    assert py_csv(want[-3:], ["r65534", "r65535", "r65536"], [40] * 3, paths).decode().replace("\n0,", "\n65534,").replace("\n1,", "\n65535,").replace(
        "\n2,", "\n65536,").splitlines()[1:] == [x for x in lines if x.split(",")[0] in ("65534", "65535", "65536")]
