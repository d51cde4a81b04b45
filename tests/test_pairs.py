"""Paired records: the union of two record batches on the device and the paired forms of the record file drivers
(spsp_records_union_device, spsp_union_plan_host, spsp_union_stage_ms, spsp_pairs_names_host, spsp_classify_files_paired,
spsp_taxonomy_files_paired; bin/comparator -X <R1> -x <R2> [-H ...] [-F ...] [-u]).

The rule (include/spsp.h, "paired records"): pair p is record p of the records file and record p of the mates file; its keys are
the union of the two mates' key sets, each key once; its length the two mates' bases; its name mate 1's first word less one
trailing "/1", which mate 2's less one trailing "/2" must equal.  From there on a pair is a record.
The union is held against sorted(set(A_r) | set(B_r)) of key tuples (minimizer, kmer_hi, kmer_lo) in numpy; the road against the
existing record calls over keys that came through the existing public calls and were united on the host.  Everything is compared
exactly: there is no tolerance anywhere."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
import test_classify as tc
import test_prevalence as tp
import test_taxonomy as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
NEW_CALLS = ("spsp_pairs_names_host", "spsp_union_plan_host", "spsp_records_union_device", "spsp_union_stage_ms", "spsp_classify_files_paired",
             "spsp_taxonomy_files_paired")


# ---------------------------------------------------------------------------------------------------- not GPU

def test_abi_has_the_paired_calls():
    L = sp.lib()
    for name in NEW_CALLS:
        assert name in sp.ABI_SYMBOLS and hasattr(L, name), name
    header = open(os.path.join(ROOT, "include", "spsp.h")).read()
    for name in NEW_CALLS:
        assert "int %s(" % name in header, name


def test_union_plan_is_the_constants_of_the_kernels():
    plan = sp.union_plan()
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    value = lambda name: int(text.split("constexpr uint32_t %s = " % name)[1].split(";")[0])
    assert plan == {"threads": value("kUnThreads"), "tile": value("kUnTile")}
    assert plan["threads"] % 64 == 0 and plan["tile"] % 64 == 0


def test_pairs_names():
    assert sp.pairs_names([], []) == []
    assert sp.pairs_names(["r1/1", "r2/1"], ["r1/2", "r2/2"]) == [b"r1", b"r2"]                       # the suffixes
    assert sp.pairs_names(["r1", "x.7"], ["r1", "x.7"]) == [b"r1", b"x.7"]                          # equal names without one
    assert sp.pairs_names(["r1/1", "r2"], ["r1", "r2/2"]) == [b"r1", b"r2"]                         # a suffix on one mate only
    assert sp.pairs_names(["a/1/1"], ["a/1/2"]) == [b"a/1"]                                         # ONE trailing suffix is removed
    assert sp.pairs_names(["/1", ""], ["/2", ""]) == [b"", b""]
    for n1, n2, bad in ((["r1/1"], ["r1/1"], 0),                                                     # a /1 paired with a /1
                        (["r1/2"], ["r1/2"], 0), (["r1/2"], ["r1/1"], 0),
                        (["a", "b", "c/1", "d", "e"], ["a", "b", "d/2", "e", "f"], 2),              # slipped out of step in the middle
                        (["a", "b"], ["a", "B"], 1), (["a"], ["a "], 0), (["ab"], ["a"], 0)):
        with pytest.raises(sp.SpspError) as e:
            sp.pairs_names(n1, n2)
        assert e.value.code == sp.ERR_FORMAT and e.value.bad == bad, (n1, n2)
        assert "pair %d" % bad in str(e.value) and "'%s'" % n1[bad] in str(e.value) and "'%s'" % n2[bad] in str(e.value)
    with pytest.raises(ValueError):
        sp.pairs_names(["a"], [])


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    (tmp_path / "labels.txt").write_text("a\nb\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    r = run("-x", "r2.fq", "-f", "list.txt", "-o", "bad")                                            # -x without -X
    assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and "-x" in r.stdout and "needs -X" in r.stdout, r.stdout
    for o, v in (("-D", "reads.fq"), ("-F", "matched")):                                              # ... with what needs -X itself
        r = run("-x", "r2.fq", o, v, "-f", "list.txt", "-o", "bad")
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and "-X" in r.stdout, r.stdout
    excluded = (("-q", "list.txt"), ("-g", "3"), ("-c", "0.5"), ("-C", "0.5"), ("-N", "5"), ("-P", "0.9"), ("-r", "0.9"), ("-R", "0.9"), ("-l", "0.5"),
                ("-L", "0.5"), ("-S", "union"), ("-E", "union"), ("-J", "0.5"), ("-K", "0.5"), ("-A", "10"), ("-G", "labels.txt"), ("-D", "reads.fq"))
    for o, v in excluded:                                                                            # every exclusion of -X holds with -x
        r = run("-X", "r1.fq", "-x", "r2.fq", o, v, "-f", "list.txt", "-o", "bad")
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and "-X" in r.stdout, (o, r.stdout, r.stderr)
    r = run("-X", "r1.fq", "-x", "r2.fq", "-H", "lin.txt", "-Y", "3", "-f", "list.txt", "-o", "bad")
    assert r.returncode == 1 and "-H" in r.stdout
    assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
    usage = run().stdout
    assert any(line.startswith("-x ") and "-X" in line and "pair" in line for line in usage.splitlines()), usage


def test_host_functions_under_the_sanitizers():
    """tests/tools/pairs_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the
    names rule and the plan (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "pairs_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "pairs_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU: the union

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def side():
    c = sp.Context(0)
    yield c
    c.close()


def key(i, k, mn=7):
    """keys whose order is the order of i: (minimizer, kmer_hi, kmer_lo)"""
    return (mn, (i >> 3) if k > 32 else 0, 3 * i + 1)


def run_len(i):
    return ((i + 1) * 2654435761 >> 11) % 3                                                          # 0, 1 or 2, mixed


def union_call(ctx, k, A, B, a_pre=0, b_pre=0):
    """A, B: per record a collection of key tuples -> (the union's tuples per record, offsets); a_pre / b_pre: entries of
    another record's keys in front of the first offset"""
    junk = [key(10 ** 6 + i, k, 3) for i in range(max(a_pre, b_pre))]
    packed = []
    for recs, pre in ((A, a_pre), (B, b_pre)):
        mn, lo, hi, off, _ = tp.pack([junk[:pre]] + list(recs), k)
        packed.append((tp.upload(mn, lo, hi), off[1:]))
    (da, a_off), (db, b_off) = packed
    assert int(a_off[0]) == a_pre and int(b_off[0]) == b_pre
    d_mn, d_lo, d_hi, off = ctx.records_union_device(k, tp.ptr(da[0]), tp.ptr(da[1]), tp.ptr(da[2]), a_off, tp.ptr(db[0]), tp.ptr(db[1]), tp.ptr(db[2]), b_off)
    total = int(off[-1])
    assert (d_hi is not None) == (k > 32) and d_mn and d_lo
    mn, lo = ctx.to_host(d_mn, total, np.uint32), ctx.to_host(d_lo, total, np.uint64)
    hi = ctx.to_host(d_hi, total, np.uint64) if k > 32 else np.zeros(total, np.uint64)
    flat = list(zip(mn.tolist(), hi.tolist(), lo.tolist()))
    del da, db
    return [flat[int(a):int(z)] for a, z in zip(off[:-1], off[1:])], off


def check_union(ctx, k, A, B, a_pre=0, b_pre=0):
    got, off = union_call(ctx, k, A, B, a_pre, b_pre)
    want = [sorted(set(a) | set(b)) for a, b in zip(A, B)]
    assert int(off[0]) == 0 and np.diff(off.astype(np.int64)).tolist() == [len(w) for w in want]
    bad = [r for r, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (bad[:5], got[bad[0]][:6], want[bad[0]][:6])
    return got


KS = [31, 63]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_empty_sides_and_no_records(ctx, k):
    some = [key(i, k) for i in range(5)]
    check_union(ctx, k, [[]], [[]])
    check_union(ctx, k, [[], [], []], [[], [], []])
    check_union(ctx, k, [[], some], [some, []])                                                      # A empty, B empty
    check_union(ctx, k, [[]] * 3 + [some], [[]] * 4)                                                 # a whole side without keys
    check_union(ctx, k, [[]] * 4, [[]] * 3 + [some])
    got, off = union_call(ctx, k, [], [])                                                            # n_records = 0
    assert got == [] and off.tolist() == [0]


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_identical_disjoint_below_above_alternating(ctx, k):
    K = lambda ids: [key(i, k) for i in ids]
    n = 150
    A = [K(range(n)), K(range(0, 2 * n, 2)), K(range(n, 2 * n)), K(range(n)), K(range(0, 2 * n, 2)), K([5]), K([5]), K([5]), K([9])]
    B = [K(range(n)), K(range(3 * n, 4 * n)), K(range(n)), K(range(n, 2 * n)), K(range(1, 2 * n, 2)), K([5]), K([4]), K([6]), []]
    got = check_union(ctx, k, A, B)
    assert [len(g) for g in got] == [n, 2 * n, 2 * n, 2 * n, 2 * n, 1, 2, 2, 1]
    check_union(ctx, k, B, A)


@pytest.mark.gpu
def test_keys_that_differ_in_one_word_only(ctx):
    """a comparison that drops a word takes two of these for one key, or orders them by the wrong word"""
    base = (9, 5, 1000)
    for word in range(3):
        lower, higher = list(base), list(base)
        lower[word] -= 1
        higher[word] += 1
        lower, higher = tuple(lower), tuple(higher)
        for A, B in (([base], [higher]), ([base], [lower]), ([lower, higher], [base]), ([lower, base, higher], [lower, higher]), ([base], [base])):
            check_union(ctx, 63, [A, [base]], [B, []])
    # the order is (minimizer, kmer_hi, kmer_lo): a larger kmer_lo under a smaller kmer_hi comes first
    check_union(ctx, 63, [[(9, 5, 1000), (9, 6, 10)]], [[(9, 5, 2000), (9, 6, 5), (8, 9, 9)]])
    for word in (0, 2):                                                                              # k <= 32: no kmer_hi
        lower, higher = [9, 0, 1000], [9, 0, 1000]
        lower[word] -= 1
        higher[word] += 1
        check_union(ctx, 31, [[tuple(lower), tuple(higher)], [(9, 0, 1000)]], [[(9, 0, 1000)], [tuple(higher)]])


def placed(k, sizes_a, sizes_b, overlap):
    """records of the given sizes; record r of B shares `overlap` of min(size) keys with record r of A"""
    A, B, at = [], [], 0
    for na, nb in zip(sizes_a, sizes_b):
        A.append([key(at + 2 * i, k) for i in range(na)])
        shared = min(na, nb, int(overlap * min(na, nb) + 0.5))
        B.append(A[-1][:shared] + [key(at + 2 * i + 1, k) for i in range(nb - shared)])
        at += 2 * max(na, nb) + 2
    return A, B


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_records_on_the_lane_workgroup_and_tile_seams(ctx, k):
    plan = sp.union_plan()
    cuts = sorted({63, 64, 65, plan["threads"] - 1, plan["threads"], plan["threads"] + 1, plan["tile"] - 1, plan["tile"], plan["tile"] + 1,
                   2 * plan["tile"] - 1, 2 * plan["tile"], 2 * plan["tile"] + 1})
    for at in cuts:
        # a record that ENDS at entry `at` of either side and one that STARTS there, then a one-key record and a tail
        sizes = [at, 3, 1, at + 1, 0, 2]
        for overlap in (0.0, 0.5, 1.0):
            check_union(ctx, k, *placed(k, sizes, sizes, overlap))
        check_union(ctx, k, *placed(k, sizes, [1, 0, at - 1, 2, at, 70], 0.5))                      # the two sides' seams apart
        check_union(ctx, k, *placed(k, [1] * at + [5], [1] * at + [5], 0.5))                         # one-key records up to the seam
        check_union(ctx, k, *placed(k, sizes, sizes, 0.5), a_pre=3, b_pre=at)                        # offsets that do not start at 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_one_long_record_among_2000_one_key_records(ctx, k):
    sizes = [1] * 1000 + [5000] + [1] * 1000
    A, B = placed(k, sizes, sizes, 0.5)
    got = check_union(ctx, k, A, B)
    assert len(got[1000]) == 7500 and got[1000] == sorted(set(A[1000]) | set(B[1000]))              # the long record word for word
    assert all(len(g) == 1 for g in got[:1000] + got[1001:])


@pytest.mark.gpu
def test_65537_records_of_0_to_2_keys(ctx):
    """nothing is 16 bits wide"""
    n, k = 65537, 31
    sa, sb = [run_len(r) for r in range(n)], [run_len(r + n) for r in range(n)]
    sa[65535], sb[65535], sa[65536], sb[65536] = 2, 1, 1, 2
    A, B = placed(k, sa, sb, 0.5)
    got = check_union(ctx, k, A, B)
    assert len(got) == n and got[65536] == sorted(set(A[65536]) | set(B[65536])) and len(got[65536]) >= 2


@pytest.mark.gpu
def test_two_calls_on_one_context_and_the_clock(ctx):
    k = 63
    check_union(ctx, k, *placed(k, [700, 3, 300], [650, 0, 301], 0.5))
    got = check_union(ctx, k, [[key(1, k), key(3, k)]], [[key(2, k)]], a_pre=2, b_pre=1)              # a smaller shape: nothing of the first
    assert got == [[key(1, k), key(2, k), key(3, k)]]
    ctx.timing_enable(True)
    ctx.union_stage_ms()
    check_union(ctx, k, *placed(k, [700, 3, 300], [650, 0, 301], 0.5))
    ms = ctx.union_stage_ms()
    ctx.timing_enable(False)
    assert set(ms) == {"flags", "scan", "offsets", "write"} and all(v > 0 for v in ms.values()) and sum(ctx.union_stage_ms().values()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_a_seeded_sweep_against_the_model(ctx, seed):
    rng = np.random.default_rng(seed)
    for k in KS:
        pool = tp.pool(40000, k, seed)                                                               # mixed words, a few minimizers
        for overlap in (0.0, 0.5, 1.0):
            A, B, at = [], [], 0
            for _ in range(60):
                na, nb = (int(x) for x in rng.choice([0, 1, 2, 63, 64, 65, 300], 2))
                a = pool[at:at + na]
                shared = int(overlap * min(na, nb) + 0.5)
                picked = [a[i] for i in sorted(rng.choice(na, shared, replace=False).tolist())] if shared else []
                B.append(picked + pool[at + na:at + na + nb - shared])
                A.append(a)
                at += na + nb
            check_union(ctx, k, A, B, a_pre=int(rng.integers(0, 3)), b_pre=int(rng.integers(0, 3)))


def raw_call(ctx, k, a, a_off, b, b_off):
    """key tuples as they are given (no sorting) -> the call"""
    arrays = []
    for keys in (a, b):
        mn = np.array([x[0] for x in keys], dtype=np.uint32)
        hi = np.array([x[1] for x in keys], dtype=np.uint64)
        lo = np.array([x[2] for x in keys], dtype=np.uint64)
        arrays.append(tp.upload(mn, lo, hi))
    da, db = arrays
    hi_a, hi_b = (tp.ptr(da[2]), tp.ptr(db[2])) if k > 32 else (None, None)
    try:
        return ctx.records_union_device(k, tp.ptr(da[0]), tp.ptr(da[1]), hi_a, a_off, tp.ptr(db[0]), tp.ptr(db[1]), hi_b, b_off)
    finally:
        del da, db


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
def test_refusals_and_what_they_leave_behind(ctx, k):
    K = lambda ids: [key(i, k) for i in ids]
    good = K(range(10))
    out = raw_call(ctx, k, good, [0, 4, 10], K(range(5, 12)), [0, 3, 7])
    assert out[3].tolist() == [0, 7, 15]
    cases = [
        (K([0, 1, 2, 5, 4, 6, 7, 8, 9, 10]), [0, 3, 10], good, [0, 4, 10], "side A, record 1"),       # an unsorted record on side A
        (good, [0, 4, 10], K([0, 1, 2, 3, 3, 5, 6, 7, 8, 9]), [0, 2, 10], "side B, record 1"),       # a duplicate key on side B
        (K([1, 0] + list(range(2, 10))), [0, 4, 10], K([1, 1] + list(range(2, 10))), [0, 4, 10], "side A, record 0"),   # both: the least
        (good, [0, 4, 10], K([9, 8]), [0, 0, 2], "side B, record 1"),
    ]
    for a, a_off, b, b_off, word in cases:
        with pytest.raises(sp.SpspError) as e:
            raw_call(ctx, k, a, a_off, b, b_off)
        assert e.value.code == sp.ERR_ARG and word in str(e.value) and "strictly increasing" in str(e.value), str(e.value)
    # the first key of a record may lie below the last of the record in front of it
    out = raw_call(ctx, k, K([5, 6, 1, 2]), [0, 2, 4], K([7, 0]), [0, 1, 2])
    assert out[3].tolist() == [0, 3, 6]
    # the C call itself: the arrays NULL and the offsets all 0 behind a refusal
    C = sp.C
    for a_off, b_off, code, word in (([0, 4, 3], [0, 1, 2], sp.ERR_ARG, "side A, record 1"), ([0, 1, 2], [5, 4, 6], sp.ERR_ARG, "side B, record 0"),
                                     ([0, 1, 0xfffffff1], [0, 0, 0], sp.ERR_OVERFLOW, "too many"), ([0, 1, 0x80000000], [0, 1, 0x80000000], sp.ERR_OVERFLOW, "too many")):
        a_off, b_off = np.array(a_off, dtype=np.uint64), np.array(b_off, dtype=np.uint64)
        off = np.full(3, 77, dtype=np.uint64)
        o = [C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)]
        d = tp.upload(np.zeros(16, np.uint32), np.zeros(16, np.uint64), np.zeros(16, np.uint64))
        hi = tp.ptr(d[2]) if k > 32 else None
        rc = sp.lib().spsp_records_union_device(ctx._h, k, tp.ptr(d[0]), tp.ptr(d[1]), hi, a_off.ctypes.data, tp.ptr(d[0]), tp.ptr(d[1]), hi, b_off.ctypes.data, 2,
                                                C.byref(o[0]), C.byref(o[1]), C.byref(o[2]), off.ctypes.data)
        assert rc == code and word in sp.lib().spsp_last_error().decode() and [x.value for x in o] == [None] * 3 and off.tolist() == [0, 0, 0], (a_off, rc)
    with pytest.raises(sp.SpspError) as e:                                                           # kmer_hi against k
        d = tp.upload(np.arange(4, dtype=np.uint32), np.arange(4, dtype=np.uint64), np.arange(4, dtype=np.uint64))
        ctx.records_union_device(k, tp.ptr(d[0]), tp.ptr(d[1]), None if k > 32 else tp.ptr(d[2]), [0, 4], tp.ptr(d[0]), tp.ptr(d[1]),
                                 None if k > 32 else tp.ptr(d[2]), [0, 4])
    assert e.value.code == sp.ERR_ARG and "kmer_hi" in str(e.value) and "side A" in str(e.value)
    for bad_k in (0, 64):
        with pytest.raises(sp.SpspError) as e:
            ctx.records_union_device(bad_k, None, None, None, [0, 0], None, None, None, [0, 0])
        assert e.value.code == sp.ERR_ARG and "k=" in str(e.value)
    with pytest.raises(sp.SpspError) as e:                                                           # keys and no array
        ctx.records_union_device(31, None, None, None, [0, 2], None, None, None, [0, 0])
    assert e.value.code == sp.ERR_ARG and "NULL" in str(e.value)
    check_union(ctx, k, [good], [K(range(5, 12))])                                                   # the context works on


# ---------------------------------------------------------------------------------------------------- GPU: the road

K_ROAD, M_ROAD, S_ROAD = tc.K_FILE, tc.M_FILE, 1.0
COMP = bytes.maketrans(b"ACGT", b"TGCA")
I_PAIR = 3                                                                                           # the pair built for the -I test


def revcomp(seq):
    return seq.translate(COMP)[::-1]


def pair_case():
    """240 pairs cut from test_classify's six references: fragments of 100 (the mates overlap entirely, in reverse complement)
    to 400 bases read 100 bases from either end; a mate shorter than k now and then; every eighth pair from no reference; and
    pair I_PAIR, whose mates share 60 bases of no reference in front of 60 bases of reference 0 each"""
    refs, _ = tc.file_case()
    rng = np.random.default_rng(23)
    pairs = []
    for p in range(240):
        if p % 8 == 7:
            m1, m2 = tc.random_bases(rng, 100), tc.random_bases(rng, 100)
        else:
            src = refs[int(rng.integers(len(refs)))]
            n = int(rng.choice([100, 150, 260, 400]))
            a = int(rng.integers(len(src) - n + 1))
            frag = src[a:a + n]
            m1, m2 = frag[:100], revcomp(frag[-100:])
            if p % 8 == 5:
                m2 = m2[:20]
            if p % 8 == 6:
                m1 = m1[:25]
        pairs.append(["frag%d" % p, m1, m2])
    common = tc.random_bases(rng, 60)
    pairs[I_PAIR][1:] = [common + refs[0][500:560], common + refs[0][1500:1560]]
    return refs, pairs


def fastq_mates(pairs, which, suffix=True):
    tag = (b"/%d" % which) if suffix else b""
    return b"".join(b"@" + name.encode() + tag + (b" len=%d\tmate" % len(m[which - 1]) if i % 3 else b"") + b"\n" + m[which - 1] + b"\n+\n" + b"I" * len(m[which - 1]) + b"\n"
                    for i, (name, *m) in enumerate(pairs))


def fasta_mates(pairs, which):
    return b"".join(b">" + name.encode() + b"/%d\n" % which + m[which - 1][:60] + b"\n" + (m[which - 1][60:] + b"\n" if len(m[which - 1]) > 60 else b"")
                    for name, *m in pairs)


class Dev:
    def __init__(self, text):
        import torch
        self.t = torch.from_numpy(np.frombuffer(bytes(text) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        self.ptr, self.n = self.t.data_ptr(), len(text)


def side_keys(side, text):
    """a text's per-record key sets and base counts through the public calls: ingest, scan, key extraction with one record per genome"""
    d = Dev(text)
    clean = side.clean_fastq_device if text[:1] == b"@" else side.clean_fasta_device
    d_bases, n_bases, d_off, n_rec = clean(d.ptr, d.n)
    lengths = np.diff(side.to_host(d_off, n_rec + 1, np.uint64).astype(np.int64)).tolist()
    p = sp.make_params(K_ROAD, M_ROAD, S_ROAD)
    d_sk, n_sk = side.scan_device(p, d_bases, n_bases, d_off, n_rec)
    d_mn, d_lo, d_hi, off = side.sketch_keys_device(p, d_bases, n_bases, d_off, d_sk, n_sk, np.arange(n_rec + 1))
    total = int(off[-1])
    mn, lo = side.to_host(d_mn, total, np.uint32).tolist(), side.to_host(d_lo, total, np.uint64).tolist()
    flat = list(zip(mn, [0] * total, lo))
    return [set(flat[int(a):int(z)]) for a, z in zip(off[:-1], off[1:])], lengths


class Road:
    pass


@pytest.fixture(scope="module")
def road(ctx, side, tmp_path_factory):
    R = Road()
    R.dir = tmp_path_factory.mktemp("pairs")
    R.refs, R.pairs = pair_case()
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", K_ROAD, M_ROAD, S_ROAD)[0] for i, g in enumerate(R.refs)]
    R.paths = tp.write_files(R.dir, payloads)
    R.ref_sets = [tp.key_set(p) for p in payloads]
    R.text = {"r1.fq": fastq_mates(R.pairs, 1), "r2.fq": fastq_mates(R.pairs, 2), "r1.fa": fasta_mates(R.pairs, 1),
              "s1.fq": fastq_mates(R.pairs, 1, False), "s2.fq": fastq_mates(R.pairs, 2, False)}
    for name, text in R.text.items():
        (R.dir / name).write_bytes(text)
    with gzip.open(str(R.dir / "r2.fq.gz"), "wb") as f:
        f.write(R.text["r2.fq"])
    (R.dir / "bank.txt").write_text("\n".join(R.paths) + "\n")
    R.tree = tt.Tree(tt.file_lineages())
    (R.dir / "lin.txt").write_text(R.tree.text)
    R.sets1, R.len1 = side_keys(side, R.text["r1.fq"])
    R.sets2, R.len2 = side_keys(side, R.text["r2.fq"])
    R.names = [name for name, _, _ in R.pairs]
    R.lengths = [a + b for a, b in zip(R.len1, R.len2)]
    assert R.len1 == [len(m1) for _, m1, _ in R.pairs] and R.len2 == [len(m2) for _, _, m2 in R.pairs]
    R.f = lambda name: str(R.dir / name)
    return R


def model_classify(ctx, R, sets, top, min_keys=1, num=0, den=1):
    """the existing classify call over key sets united on the host -> (records, hits)"""
    index = tc.Index(ctx, K_ROAD, R.ref_sets)
    mn, lo, hi, off, _ = tp.pack(sets, K_ROAD)
    d = tp.upload(mn, lo, hi)
    records, hits = ctx.classify_device(tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, top, min_keys, num, den)
    del d, index
    return records, hits


def model_taxonomy(ctx, R, sets, min_keys=1, num=0, den=1):
    index = tc.Index(ctx, K_ROAD, R.ref_sets)
    ctx.taxonomy_index_device(R.tree.parent, R.tree.ref_node)
    mn, lo, hi, off, _ = tp.pack(sets, K_ROAD)
    d = tp.upload(mn, lo, hi)
    records = ctx.taxonomy_device(tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, min_keys, num, den)
    del d, index
    return records


def same_rows(got, want, lengths):
    want = want.copy()
    want["length"] = lengths
    return got.tobytes() == want.tobytes()


@pytest.mark.gpu
def test_paired_classify_files_equal_the_record_call_over_united_keys(ctx, road):
    R = road
    united = [a | b for a, b in zip(R.sets1, R.sets2)]
    assert sum(1 for a, b, u in zip(R.sets1, R.sets2, united) if a and b and len(u) == len(a) + len(b)) > 50   # disjoint mates
    assert sum(1 for a, b in zip(R.sets1, R.sets2) if a and a == b) > 20                                      # mates that overlap entirely
    assert sum(1 for a, b in zip(R.sets1, R.sets2) if not b and a) > 10 and sum(1 for a, b in zip(R.sets1, R.sets2) if not a and b) > 10
    for tag, (top, min_keys, num, den) in (("pa", (1, 1, 0, 1)), ("pb", (3, 2, 1, 10)), ("pc", (64, 1, 1, 2))):
        want_r, want_h = model_classify(ctx, R, united, top, min_keys, num, den)
        records, hits = ctx.classify_files(R.paths, R.f("r1.fq"), R.f(tag), top, min_keys, num, den, mates_path=R.f("r2.fq"))
        assert records["length"].tolist() == R.lengths and records["keys"].tolist() == [len(u) for u in united]
        assert same_rows(records, want_r, R.lengths) and hits.tobytes() == want_h.tobytes(), tag
        want_r = want_r.copy()
        want_r["length"] = R.lengths
        assert tc.both_files(R.dir, tag) == [sp.classify_csv(want_r, want_h, R.names, R.paths, top), sp.classify_summary_csv(want_r, want_h, R.paths, top)]
        assert tag != "pa" or (records["listed"] > 0).sum() > 150
    # FASTA R1 with FASTQ R2, gzip and plain: the same rows and the same files
    records, hits = ctx.classify_files(R.paths, R.f("r1.fa"), R.f("mixed"), 3, 2, 1, 10, mates_path=R.f("r2.fq.gz"))
    assert tc.both_files(R.dir, "mixed") == tc.both_files(R.dir, "pb")
    records, hits = ctx.classify_files(R.paths, R.f("r1.fa"), R.f("mixed2"), 3, 2, 1, 10, mates_path=R.f("r2.fq"))
    assert tc.both_files(R.dir, "mixed2") == tc.both_files(R.dir, "pb")


@pytest.mark.gpu
def test_paired_taxonomy_files_equal_the_record_call_over_united_keys(ctx, road):
    R = road
    united = [a | b for a, b in zip(R.sets1, R.sets2)]
    for tag, (min_keys, num, den) in (("ta", (1, 0, 1)), ("tb", (2, 1, 2))):
        want = model_taxonomy(ctx, R, united, min_keys, num, den)
        records = ctx.taxonomy_files(R.paths, R.f("r1.fq"), R.f("lin.txt"), R.f(tag), min_keys, num, den, mates_path=R.f("r2.fq.gz"))
        assert same_rows(records, want, R.lengths), tag
        want = want.copy()
        want["length"] = R.lengths
        assert tt.both_files(R.dir, tag) == [sp.taxonomy_csv(want, R.names, R.tree.parent, R.tree.names), sp.taxonomy_report_csv(want, R.tree.parent, R.tree.names, R.tree.ref_node)]
        assert tag != "ta" or ((records["node"] != tt.NONE).sum() > 150 and len(set(records["node"].tolist())) > 3)


@pytest.mark.gpu
def test_a_file_against_itself_short_mates_and_mates_in_reverse_complement(ctx, road):
    R = road
    top = 3
    single_r, single_h = ctx.classify_files(R.paths, R.f("s1.fq"), R.f("single"), top)
    assert single_r["keys"].tolist() == [len(s) for s in R.sets1]
    # held against itself: the single-file rows with `length` doubled
    records, hits = ctx.classify_files(R.paths, R.f("s1.fq"), R.f("self"), top, mates_path=R.f("s1.fq"))
    assert same_rows(records, single_r, [2 * n for n in R.len1]) and hits.tobytes() == single_h.tobytes()
    # a mate 2 of reads shorter than k: mate 1's rows, except `length`
    short = [[name, m1, m2[:20]] for name, m1, m2 in R.pairs]
    (R.dir / "short2.fq").write_bytes(fastq_mates(short, 2, False))
    records, hits = ctx.classify_files(R.paths, R.f("s1.fq"), R.f("short"), top, mates_path=R.f("short2.fq"))
    assert same_rows(records, single_r, [n + min(20, m) for n, m in zip(R.len1, R.len2)]) and hits.tobytes() == single_h.tobytes()
    # ... and as mate 1: the same rows again
    records, hits = ctx.classify_files(R.paths, R.f("short2.fq"), R.f("short1"), top, mates_path=R.f("s1.fq"))
    assert same_rows(records, single_r, [n + min(20, m) for n, m in zip(R.len1, R.len2)]) and hits.tobytes() == single_h.tobytes()
    # mates that overlap entirely in reverse complement: the keys of mate 1
    rc = [[name, m1, revcomp(m1)] for name, m1, _ in R.pairs]
    (R.dir / "rc2.fq").write_bytes(fastq_mates(rc, 2, False))
    records, hits = ctx.classify_files(R.paths, R.f("s1.fq"), R.f("rc"), top, mates_path=R.f("rc2.fq"))
    assert same_rows(records, single_r, [2 * n for n in R.len1]) and hits.tobytes() == single_h.tobytes()
    assert tc.both_files(R.dir, "rc") == tc.both_files(R.dir, "self")


@pytest.mark.gpu
def test_a_threshold_that_passes_only_with_both_mates_keys(ctx, road):
    """pair I_PAIR: each mate holds 30 keys of reference 0 among 90; the 60 keys of the shared 60 bases and of the seam behind them
    are not the reference's -- and 30 of them are the same in both mates.  Alone a mate has 30 / 90 of its keys in the reference,
    the pair 60 / 150: -I 0.37 lies between"""
    R = road
    a, b, ref = R.sets1[I_PAIR], R.sets2[I_PAIR], R.ref_sets[0]
    u = a | b
    num, den = 37, 100
    assert len(a & ref) * den < num * len(a) and len(b & ref) * den < num * len(b) and len(u & ref) * den >= num * len(u), (len(a), len(b), len(u), len(u & ref))
    one, _ = ctx.classify_files(R.paths, R.f("r1.fq"), R.f("i1"), 1, 1, num, den)
    two, _ = ctx.classify_files(R.paths, R.f("r2.fq"), R.f("i2"), 1, 1, num, den)
    both, hits = ctx.classify_files(R.paths, R.f("r1.fq"), R.f("i12"), 1, 1, num, den, mates_path=R.f("r2.fq"))
    assert one["listed"][I_PAIR] == 0 and two["listed"][I_PAIR] == 0 and both["listed"][I_PAIR] == 1
    assert int(hits[I_PAIR][0]["reference"]) == 0 and int(hits[I_PAIR][0]["shared"]) == len(u & ref) and int(both["keys"][I_PAIR]) == len(u)
    r = subprocess.run([EXE, "-X", "r1.fq", "-x", "r2.fq", "-I", "0.37", "-f", "bank.txt", "-o", "icli"], cwd=R.dir, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "pair(s)" in r.stdout and tc.both_files(R.dir, "icli") == tc.both_files(R.dir, "i12"), r.stdout + r.stderr


@pytest.mark.gpu
def test_files_out_of_step_are_refused_and_write_nothing(ctx, road):
    R = road
    (R.dir / "fewer.fq").write_bytes(fastq_mates(R.pairs[:-1], 2))
    slipped = [list(p) for p in R.pairs]
    for i in range(120, len(slipped) - 1):                                                           # a read lost in the middle of mate 2
        slipped[i][0] = R.pairs[i + 1][0]
    (R.dir / "slipped.fq").write_bytes(fastq_mates(slipped, 2))
    cases = (("fewer.fq", ("240", "239", "r1.fq", "fewer.fq")), ("slipped.fq", ("pair 120", "'frag120/1'", "'frag121/2'")), ("r1.fq", ("pair 0", "'frag0/1'")))
    for mates, words in cases:
        with pytest.raises(sp.SpspError) as e:
            ctx.classify_files(R.paths, R.f("r1.fq"), R.f("no"), mates_path=R.f(mates))
        assert e.value.code == sp.ERR_FORMAT and all(w in str(e.value) for w in words), str(e.value)
        with pytest.raises(sp.SpspError) as e:
            ctx.taxonomy_files(R.paths, R.f("r1.fq"), R.f("lin.txt"), R.f("no"), extract="classified", mates_path=R.f(mates))
        assert e.value.code == sp.ERR_FORMAT and all(w in str(e.value) for w in words), str(e.value)
    r = subprocess.run([EXE, "-X", "r1.fq", "-x", "slipped.fq", "-F", "matched", "-f", "bank.txt", "-o", "no"], cwd=R.dir, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "pair 120" in r.stdout, r.stdout + r.stderr
    with pytest.raises(sp.SpspError):                                                                # a mates file that is not there
        ctx.classify_files(R.paths, R.f("r1.fq"), R.f("no"), mates_path=R.f("none.fq"))
    assert not [f for f in os.listdir(R.dir) if f.startswith("no_")]


def gunzip(path):
    with gzip.open(str(path), "rb") as f:
        return f.read()


@pytest.mark.gpu
def test_every_extract_word_through_both_drivers_and_the_command_line(ctx, road):
    R = road
    top = 3
    t1, t2 = R.text["r1.fa"], R.text["r2.fq"]
    cli = lambda *a: subprocess.run([EXE] + list(a), cwd=R.dir, capture_output=True, text=True, timeout=600)
    ctx.classify_files(R.paths, R.f("r1.fa"), R.f("plain"), top, mates_path=R.f("r2.fq.gz"))
    csvs = tc.both_files(R.dir, "plain")
    kept_of = {}
    for i, what in enumerate(("matched", "unmatched", "best=0", "best=4", "listed=1", "listed=5")):
        tag, plain = "x%d" % i, bool(i & 1)
        records, hits = ctx.classify_files(R.paths, R.f("r1.fa"), R.f(tag), top, extract=what, gz=not plain, mates_path=R.f("r2.fq.gz"))
        keep = sp.extract_flags_classify(what, records, hits, len(R.paths))
        want1, n_kept = sp.records_extract(t1, keep)
        want2, _ = sp.records_extract(t2, keep)
        names = [tag + "_extract_1.fa" + ("" if plain else ".gz"), tag + "_extract_2.fq" + ("" if plain else ".gz")]
        got = [(R.dir / n).read_bytes() if plain else gunzip(R.dir / n) for n in names]
        assert got == [want1, want2] and ctx.last_extract == {"n_kept": n_kept, "bytes_out": len(want1) + len(want2)}, what
        assert tc.both_files(R.dir, tag) == csvs                                                     # the CSVs of the run without the word
        assert sorted(f for f in os.listdir(R.dir) if f.startswith(tag + "_")) == sorted(names + [tag + "_classify.csv.gz", tag + "_classify_summary.csv.gz"])
        # the two files hold the same pairs, in the same order
        n1 = sp.pairs_names([l[1:].split()[0] for l in want1.decode().splitlines() if l.startswith(">")], [l[1:].split()[0] for l in want2.decode().splitlines()[::4]])
        assert n1 == [R.names[r].encode() for r in np.nonzero(keep)[0]]
        r = cli("-X", "r1.fa", "-x", "r2.fq.gz", "-F", what, "-Y", str(top), "-f", "bank.txt", "-o", "c" + tag, *(["-u"] if plain else []))
        assert r.returncode == 0 and "pair(s) kept" in r.stdout, r.stdout + r.stderr
        assert [(R.dir / ("c" + n)).read_bytes() if plain else gunzip(R.dir / ("c" + n)) for n in names] == got and tc.both_files(R.dir, "c" + tag) == csvs
        kept_of[what] = keep
    assert 0 < kept_of["matched"].sum() < len(R.pairs) and (kept_of["matched"] + kept_of["unmatched"] == 1).all() and kept_of["best=0"].sum() > 0
    # what did not match, fed back as a pair, matches nothing
    records, hits = ctx.classify_files(R.paths, R.f("x1_extract_1.fa"), R.f("back"), top, mates_path=R.f("x1_extract_2.fq"))
    assert len(records) == kept_of["unmatched"].sum() and (records["listed"] == 0).all()
    # with -H
    size = sp.taxonomy_lineages(R.tree.text, len(R.paths))["size"]
    ctx.taxonomy_files(R.paths, R.f("r1.fa"), R.f("lin.txt"), R.f("tplain"), mates_path=R.f("r2.fq.gz"))
    tcsvs = tt.both_files(R.dir, "tplain")
    inner = R.tree.num[("Bacteria", "G1")]
    for i, what in enumerate(("classified", "unclassified", "taxon=%d" % inner, "clade=%d" % inner)):
        tag, plain = "y%d" % i, not (i & 1)
        records = ctx.taxonomy_files(R.paths, R.f("r1.fa"), R.f("lin.txt"), R.f(tag), extract=what, gz=not plain, mates_path=R.f("r2.fq.gz"))
        keep = sp.extract_flags_taxonomy(what, records, size)
        want = [sp.records_extract(t1, keep)[0], sp.records_extract(t2, keep)[0]]
        names = [tag + "_extract_1.fa" + ("" if plain else ".gz"), tag + "_extract_2.fq" + ("" if plain else ".gz")]
        assert [(R.dir / n).read_bytes() if plain else gunzip(R.dir / n) for n in names] == want and tt.both_files(R.dir, tag) == tcsvs, what
        assert ctx.last_extract == {"n_kept": int(keep.astype(bool).sum()), "bytes_out": len(want[0]) + len(want[1])}
        r = cli("-X", "r1.fa", "-x", "r2.fq.gz", "-H", "lin.txt", "-F", what, "-f", "bank.txt", "-o", "c" + tag, *(["-u"] if plain else []))
        assert r.returncode == 0 and "pair(s) kept" in r.stdout, r.stdout + r.stderr
        assert [(R.dir / ("c" + n)).read_bytes() if plain else gunzip(R.dir / ("c" + n)) for n in names] == want and tt.both_files(R.dir, "c" + tag) == tcsvs
        assert 0 < keep.astype(bool).sum() < len(R.pairs) or what.startswith("taxon"), what
    # without -x the comparator and the library are what they were: R1 alone, the old way
    records, hits = ctx.classify_files(R.paths, R.f("r1.fq"), R.f("old"), top, extract="matched")
    r = cli("-X", "r1.fq", "-F", "matched", "-Y", str(top), "-f", "bank.txt", "-o", "cold")
    assert r.returncode == 0 and "record(s) kept" in r.stdout and tc.both_files(R.dir, "cold") == tc.both_files(R.dir, "old"), r.stdout + r.stderr
    assert gunzip(R.dir / "cold_extract.fq.gz") == gunzip(R.dir / "old_extract.fq.gz") == sp.records_extract(R.text["r1.fq"], sp.extract_flags_classify("matched", records, hits, len(R.paths)))[0]
    assert records["keys"].tolist() == [len(s) for s in R.sets1]


@pytest.mark.gpu
def test_65537_pairs_cross_the_batch_seam(ctx, tmp_path):
    """two batches (65 535 pairs and 2): a union per batch, the rows of the pairs on both sides of the seam, one extraction per mate"""
    n_rec, s = 65537, 1.0
    rng = np.random.default_rng(17)
    refs = [tc.random_bases(rng, 3000) for _ in range(2)]
    seq1 = lambda r: refs[r % 2][(r * 7) % 2960:(r * 7) % 2960 + 40]
    seq2 = lambda r: revcomp(refs[(r // 2) % 2][(r * 11) % 2900:(r * 11) % 2900 + 40])
    none = tc.random_bases(rng, 40)
    m1 = [seq1(r) for r in range(n_rec)]
    m2 = [seq2(r) for r in range(n_rec)]
    m1[65535], m2[65535] = none, revcomp(none)                                                       # a pair of no reference between two that have one
    m1[0], m2[0] = none, none[:20]
    (tmp_path / "m1.fa").write_bytes(b"".join(b">r%d/1\n%s\n" % (r, q) for r, q in enumerate(m1)))
    (tmp_path / "m2.fa").write_bytes(b"".join(b">r%d/2\n%s\n" % (r, q) for r, q in enumerate(m2)))
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, s)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    records, hits = ctx.classify_files(paths, str(tmp_path / "m1.fa"), str(tmp_path / "many"), 2, extract="unmatched", gz=False, mates_path=str(tmp_path / "m2.fa"))
    assert len(records) == n_rec and (records["length"][1:] == 80).all() and records["length"][0] == 60
    ref_sets = [tp.key_set(p) for p in payloads]
    sample = sorted(set([0, 1, 2, 65533, 65534, 65535, 65536] + rng.integers(0, n_rec, 12).tolist()))
    want = tc.model(ref_sets, [tc.record_keys(m1[r], s) | tc.record_keys(m2[r], s) for r in sample], 2)
    assert tc.as_rows(records[sample], hits[sample]) == want
    assert want[sample.index(65534)][3] and want[sample.index(65536)][3] and want[sample.index(65535)][3] == [] and want[0][3] == []
    lines = tp.gunzip(str(tmp_path / "many_classify.csv.gz")).decode().splitlines()
    assert lines[-1].startswith("65536,r65536,80,") and len(lines) == 1 + int(np.maximum(records["listed"], 1).sum())
    keep = sp.extract_flags_classify("unmatched", records, hits, 2)
    assert keep[65535] and not keep[65534] and not keep[65536]
    for which, mates in ((1, m1), (2, m2)):
        want_text = b"".join(b">r%d/%d\n%s\n" % (r, which, mates[r]) for r in np.nonzero(keep)[0])
        assert (tmp_path / ("many_extract_%d.fa" % which)).read_bytes() == want_text
