"""Groups: per group of a labelled collection the keys it holds, shares, holds alone and is identified by (spsp_groups_device and
what stands around it: the labels reader, the bounds, the two CSV writers, spsp_groups_files, bin/comparator -G).

Sketches 0 .. n-1 with labels group[i] in 0 .. G-1.  h(x) = the sketches that hold key x, h_c(x) = the members of group c that
hold it.  in_min_c = ceil(num * size_c / den), out_max_c = floor(onum * (n - size_c) / oden).  For group c a key is present
(h_c >= 1), core (h_c >= in_min_c), exclusive (h_c == h) and a marker (core and h - h_c <= out_max_c).

Every expected value comes from `model`: collections.Counter keyed by (key, group) and by key, and literal set operations -- not
the table of cells the kernels count in.  No tolerance anywhere.  The GPU tests compare the group rows, the member rows AND the
marker keys of every group, key for key and in order.  Keys are hand-built (minimizer, kmer_hi, kmer_lo) arrays uploaded with
torch (test_prevalence's helpers)."""
import gzip
import os
import subprocess
from collections import Counter, defaultdict

import numpy as np
import pytest

import supersampler_amd as sp
import test_prevalence as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
G_HEADER = "group,members,keys,present,core,exclusive,marker,f_core,f_marker\n"
M_HEADER = "sketch,group,keys,core,exclusive,marker,f_core,f_marker\n"
G_FIELDS = ("members", "entries", "present", "core", "exclusive", "marker")
M_FIELDS = ("core", "exclusive", "marker")


# -------------------------------------------------------------------------------------------------- the model

def bounds(group, G, num, den, onum=0, oden=1):
    n, size = len(group), Counter(group)
    return ([size[c] for c in range(G)], [-(-num * size[c] // den) for c in range(G)], [onum * (n - size[c]) // oden for c in range(G)])


def model(sets, group, G, num, den, onum=0, oden=1):
    """-> (group rows, member rows, markers): tuples in the order of the two row structures, and per group its marker keys sorted"""
    sets = [set(s) for s in sets]
    size, in_min, out_max = bounds(group, G, num, den, onum, oden)
    h = Counter(x for s in sets for x in s)
    hc = Counter((x, group[i]) for i, s in enumerate(sets) for x in s)
    present = defaultdict(set)
    for x, c in hc:
        present[c].add(x)
    core = [{x for x in present[c] if hc[x, c] >= in_min[c]} for c in range(G)]
    exclusive = [{x for x in present[c] if hc[x, c] == h[x]} for c in range(G)]
    marker = [{x for x in core[c] if h[x] - hc[x, c] <= out_max[c]} for c in range(G)]
    entries = [0] * G
    for i, s in enumerate(sets):
        entries[group[i]] += len(s)
    rows = [(size[c], entries[c], len(present[c]), len(core[c]), len(exclusive[c]), len(marker[c])) for c in range(G)]
    members = [(len(s & core[group[i]]), len(s & exclusive[group[i]]), len(s & marker[group[i]])) for i, s in enumerate(sets)]
    return rows, members, [sorted(m) for m in marker]


def py_groups_csv(rows, names, precision=6):
    g = lambda v: "%.*g" % (precision, v)
    text = G_HEADER
    for name, (mem, ent, pres, core, excl, mark) in zip(names, rows):
        text += "%s,%d,%d,%d,%d,%d,%d,%s,%s\n" % (name, mem, ent, pres, core, excl, mark, g(core / pres if pres else 0.0), g(mark / core if core else 0.0))
    return text.encode()


def py_members_csv(members, sketch_names, group, card, rows, names, precision=6):
    g = lambda v: "%.*g" % (precision, v)
    text = M_HEADER
    for i, (core, excl, mark) in enumerate(members):
        of = rows[group[i]][5]
        text += "%s,%s,%d,%d,%d,%d,%s,%s\n" % (sketch_names[i], names[group[i]], card[i], core, excl, mark, g(core / card[i] if card[i] else 0.0),
                                              g(mark / of if of else 0.0))
    return text.encode()


def as_rows(tuples, dtype):
    out = np.zeros(len(tuples), dtype=dtype)
    for i, t in enumerate(tuples):
        out[i] = t
    return out


def as_tuples(rows, fields):
    return [tuple(int(r[f]) for f in fields) for r in rows]


# ------------------------------------------------------------------------------------------------ not GPU

def K(*xs):
    return {(x, 0, x) for x in xs}


A, B, C_, D, E, F, G_ = 1, 2, 3, 4, 5, 6, 7
HAND_GROUP = [0, 1, 0, 1, 0, 2]
HAND_HOLDERS = {A: {0, 2, 4}, B: {0, 1, 2}, C_: {1, 3}, D: {0}, E: {0, 1, 2, 3, 4, 5}, F: {5}, G_: {2, 4, 5}}


def hand_sets(key=lambda x: (x, 0, x)):
    return [{key(x) for x, hs in HAND_HOLDERS.items() if i in hs} for i in range(6)]


def test_model_on_the_hand_made_case():
    sets = hand_sets()
    rows, members, markers = model(sets, HAND_GROUP, 3, 2, 3)
    assert bounds(HAND_GROUP, 3, 2, 3) == ([3, 2, 1], [2, 2, 1], [0, 0, 0])
    assert rows == [(3, 11, 5, 4, 2, 1), (2, 5, 3, 2, 1, 1), (1, 3, 3, 3, 1, 1)]
    assert markers == [sorted(K(A)), sorted(K(C_)), sorted(K(F))]
    assert members == [(3, 2, 1), (2, 1, 1), (4, 1, 1), (2, 1, 1), (3, 1, 1), (3, 1, 1)]
    rows, members, markers = model(sets, HAND_GROUP, 3, 2, 3, 1, 3)
    assert bounds(HAND_GROUP, 3, 2, 3, 1, 3)[2] == [1, 1, 1]
    assert markers == [sorted(K(A, B, G_)), sorted(K(C_)), sorted(K(F))]
    assert [r[:5] for r in rows] == [(3, 11, 5, 4, 2), (2, 5, 3, 2, 1), (1, 3, 3, 3, 1)]
    # the sum over the groups of h_c is h: the entries of the groups add up to the entries of the collection
    assert sum(r[1] for r in rows) == sum(len(s) for s in sets)


def test_abi_has_the_groups_calls():
    calls = ("spsp_groups_labels_host", "spsp_groups_bounds_host", "spsp_groups_device", "spsp_groups_csv_host", "spsp_groups_members_csv_host",
             "spsp_groups_files")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    for name in calls:
        assert hasattr(sp.lib(), name)
    assert hasattr(sp.Context, "groups_device") and hasattr(sp.Context, "groups_files")
    assert callable(sp.groups_labels) and callable(sp.groups_bounds) and callable(sp.groups_csv) and callable(sp.groups_members_csv)
    assert sp.GROUP_ROW_DTYPE.itemsize == 48 and sp.GROUP_ROW_DTYPE.names == G_FIELDS
    assert sp.GROUP_MEMBER_ROW_DTYPE.itemsize == 24 and sp.GROUP_MEMBER_ROW_DTYPE.names == M_FIELDS


def test_the_labels_reader():
    group, names = sp.groups_labels("b\na\nb\nc c\na\n", 5)
    assert group.tolist() == [0, 1, 0, 2, 1] and names == ["b", "a", "c c"]                 # numbered by first appearance
    assert sp.groups_labels("b\r\na\r\nb\r\n", 3)[0].tolist() == [0, 1, 0] and sp.groups_labels("b\r\na\r\nb\r\n", 3)[1] == ["b", "a"]
    group, names = sp.groups_labels("x\ny", 2)                                              # no final newline
    assert group.tolist() == [0, 1] and names == ["x", "y"]
    assert sp.groups_labels("only", 1)[1] == ["only"] and sp.groups_labels("A\na\n", 2)[0].tolist() == [0, 1]
    group, names = sp.groups_labels("\n".join("g%d" % (i % 700) for i in range(65535)), 65535)
    assert group.tolist() == [i % 700 for i in range(65535)] and len(names) == 700
    refused = [("a\nb\n", 3, "line 3"), ("a\nb\nc\n", 2, "line 3"), ("a\nb\nc", 2, "line 3"), ("", 1, "line 1"), ("a\n\nb\n", 3, "line 2"), ("a\n\n", 2, "line 2"),
               ("\r\n", 1, "line 1"), ("a\nb,c\n", 2, "line 2"), ("a\nb\n\"c\"\n", 3, "line 3"), ("a\tb\n", 1, "line 1"), ("a\nb\x00\n", 2, "line 2"),
               ("a\nb\r\r\n", 2, "line 2"), ("a\n\x7f\n", 2, "line 2"), ("a\nb\n\n", 2, "line 3")]
    for text, n, where in refused:
        with pytest.raises(sp.SpspError) as e:
            sp.groups_labels(text, n)
        assert e.value.code == sp.ERR_ARG and where in str(e.value), (text, n, str(e.value))
    for n in (0, 65536):
        with pytest.raises(sp.SpspError) as e:
            sp.groups_labels("a\n", n)
        assert e.value.code == sp.ERR_ARG


def test_the_bounds_at_their_equalities():
    b = lambda group, G, *t: [a.tolist() for a in sp.groups_bounds(group, G, *t)]
    assert b([0] * 20 + [1] * 30, 2, 19, 20) == [[20, 30], [19, 29], [0, 0]]                # 19 / 20 of 20 is 19; of 30 it is 28.5
    assert b([0, 0, 0, 1], 2, 2, 3) == [[3, 1], [2, 1], [0, 0]]
    assert b([0] * 7 + [1], 2, 1, 1_000_000) == [[7, 1], [1, 1], [0, 0]]
    assert b([0] * 20 + [1] * 30, 2, 1, 1, 1, 10) == [[20, 30], [20, 30], [3, 2]]           # outside 1 / 10 of 30 is 3, of 20 is 2
    assert b([0] * 21 + [1] * 29, 2, 1, 1, 1, 10)[2] == [2, 2]                              # ... and of 29 it is 2.9
    assert b([0] * 5, 1, 1, 2, 1, 1) == [[5], [3], [0]]                                     # G = 1: nobody outside
    assert b([0] * 65534 + [1], 2, 999_999, 1_000_000, 999_999, 1_000_000) == [[65534, 1], [65534, 1], [0, 65533]]   # 64-bit products
    for group, G, num, den, onum, oden in (([0, 1], 2, 2, 3, 0, 1), ([0, 1, 2, 1, 0, 2, 2], 3, 1, 2, 1, 3), (HAND_GROUP, 3, 2, 3, 1, 3)):
        assert b(group, G, num, den, onum, oden) == [list(x) for x in bounds(group, G, num, den, onum, oden)]
    bad = [([], 1, 1, 1, 0, 1), ([0], 0, 1, 1, 0, 1), ([0], 2, 1, 1, 0, 1), ([0, 2], 2, 1, 1, 0, 1), ([0, 0, 2], 3, 1, 1, 0, 1), ([0], 1, 0, 1, 0, 1),
           ([0], 1, 2, 1, 0, 1), ([0], 1, 1, 1_000_001, 0, 1), ([0], 1, 1, 1, 2, 1), ([0], 1, 1, 1, 0, 0), ([0], 1, 1, 1, 0, 1_000_001)]
    for args in bad:
        with pytest.raises(sp.SpspError) as e:
            sp.groups_bounds(*args)
        assert e.value.code == sp.ERR_ARG, args
    with pytest.raises(sp.SpspError) as e:
        sp.groups_bounds([0, 0, 2], 3, 1, 1)
    assert "group 1 has no member" in str(e.value)


GOOD_ROWS = [(3, 11, 5, 4, 2, 1), (2, 5, 3, 2, 1, 1), (1, 3, 3, 3, 1, 3), (2, 0, 0, 0, 0, 0)]
GOOD_NAMES = ["ST 131", "clade-B", "x", "empty ones"]
GOOD_GROUP = [0, 1, 0, 1, 0, 2, 3, 3]
GOOD_CARD = [4, 2, 4, 3, 3, 3, 0, 0]
GOOD_MEMBERS = [(3, 2, 1), (2, 1, 1), (4, 1, 1), (2, 1, 1), (3, 1, 0), (3, 1, 3), (0, 0, 0), (0, 0, 0)]
GOOD_SKETCHES = ["dir/f %03d.sk.gz" % i for i in range(8)]


@pytest.mark.parametrize("precision", [1, 6, 17])
def test_both_csvs_are_the_python_formatters_byte_for_byte(precision):
    assert sp.groups_csv(as_rows(GOOD_ROWS, sp.GROUP_ROW_DTYPE), GOOD_NAMES, precision) == py_groups_csv(GOOD_ROWS, GOOD_NAMES, precision)
    got = sp.groups_members_csv(as_rows(GOOD_MEMBERS, sp.GROUP_MEMBER_ROW_DTYPE), GOOD_SKETCHES, GOOD_GROUP, GOOD_CARD, as_rows(GOOD_ROWS, sp.GROUP_ROW_DTYPE),
                                GOOD_NAMES, precision)
    assert got == py_members_csv(GOOD_MEMBERS, GOOD_SKETCHES, GOOD_GROUP, GOOD_CARD, GOOD_ROWS, GOOD_NAMES, precision)
    assert got.count(b"\n") == 9 and (precision != 6 or b"dir/f 004.sk.gz,ST 131,3,3,1,0,1,0\n" in got)
    rng = np.random.default_rng(precision)
    G, n = 37, 300
    rows = []
    for c in range(G):
        present = int(rng.integers(0, 10 ** 7))
        core = int(rng.integers(0, present + 1))
        rows.append((int(rng.integers(1, 9)), int(rng.integers(0, 10 ** 9)), present, core, int(rng.integers(0, present + 1)), int(rng.integers(0, core + 1))))
    names = ["g%d" % c for c in range(G)]
    assert sp.groups_csv(as_rows(rows, sp.GROUP_ROW_DTYPE), names, precision) == py_groups_csv(rows, names, precision)
    group = [int(x) for x in rng.integers(0, G, n)]
    card, members = [], []
    for i in range(n):
        r = rows[group[i]]
        core = int(rng.integers(0, r[3] + 1))
        members.append((core, int(rng.integers(0, r[4] + 1)), int(rng.integers(0, min(core, r[5]) + 1))))
        card.append(max(members[-1]) + int(rng.integers(0, 1000)))
    sk = ["s%d" % i for i in range(n)]
    got = sp.groups_members_csv(as_rows(members, sp.GROUP_MEMBER_ROW_DTYPE), sk, group, card, as_rows(rows, sp.GROUP_ROW_DTYPE), names, precision)
    assert got == py_members_csv(members, sk, group, card, rows, names, precision)


def test_the_csvs_refuse_what_cannot_be_counts():
    def spoilt(base, row, fields, **changes):
        rows = [dict(zip(fields, t)) for t in base]
        rows[row].update(changes)
        return [tuple(r[f] for f in fields) for r in rows]
    for rows in (spoilt(GOOD_ROWS, 0, G_FIELDS, core=6), spoilt(GOOD_ROWS, 1, G_FIELDS, marker=3), spoilt(GOOD_ROWS, 2, G_FIELDS, exclusive=4),
                 spoilt(GOOD_ROWS, 3, G_FIELDS, core=1)):
        with pytest.raises(sp.SpspError) as e:
            sp.groups_csv(as_rows(rows, sp.GROUP_ROW_DTYPE), GOOD_NAMES)
        assert e.value.code == sp.ERR_ARG and "group row" in str(e.value)
    g_rows = as_rows(GOOD_ROWS, sp.GROUP_ROW_DTYPE)
    call = lambda members, group=GOOD_GROUP, card=GOOD_CARD: sp.groups_members_csv(as_rows(members, sp.GROUP_MEMBER_ROW_DTYPE), GOOD_SKETCHES, group, card, g_rows,
                                                                                   GOOD_NAMES)
    bad = [spoilt(GOOD_MEMBERS, 1, M_FIELDS, core=3),                   # beyond c_i = 2 (and beyond its group's 2)
           spoilt(GOOD_MEMBERS, 3, M_FIELDS, core=3),                   # within c_i = 3, beyond its group's core = 2
           spoilt(GOOD_MEMBERS, 0, M_FIELDS, exclusive=3),              # beyond its group's exclusive = 2
           spoilt(GOOD_MEMBERS, 0, M_FIELDS, marker=2),                 # beyond its group's marker = 1
           spoilt(GOOD_MEMBERS, 5, M_FIELDS, core=2),                   # marker 3 > core 2
           spoilt(GOOD_MEMBERS, 6, M_FIELDS, exclusive=1)]              # a sketch without keys
    for members in bad:
        with pytest.raises(sp.SpspError) as e:
            call(members)
        assert e.value.code == sp.ERR_ARG and "member row" in str(e.value)
    with pytest.raises(sp.SpspError) as e:
        call(GOOD_MEMBERS, group=[0, 1, 0, 1, 0, 2, 3, 4])
    assert e.value.code == sp.ERR_ARG
    with pytest.raises(sp.SpspError) as e:
        call(GOOD_MEMBERS, card=[4, 2, 3, 3, 3, 3, 0, 0])               # sketch 2 has 4 core keys
    assert e.value.code == sp.ERR_ARG and "member row 2" in str(e.value)
    assert call(GOOD_MEMBERS).startswith(M_HEADER.encode())


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    (tmp_path / "labels.txt").write_text("a\nb\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    G = ("-G", "labels.txt")
    cases = [("-T", "0.5"), ("-U", "0.5"), ("-M",), G + ("-T", "0"), G + ("-T", "1.5"), G + ("-T", "0.1234567"), G + ("-T", "half"), G + ("-T", ""),
             G + ("-U", "1.5"), G + ("-U", "-0.1"), G + ("-U", "0.1234567"), G + ("-U", "x")]
    cases += [G + other for other in (("-q", "list.txt"), ("-P", "0.5"), ("-S", "union"), ("-E", "union"), ("-g", "3", "-q", "list.txt"), ("-c", "0.5"),
                                      ("-C", "0.5"), ("-N", "5"), ("-r", "0.5"), ("-R", "0.5"), ("-l", "0.5"), ("-L", "0.5"), ("-A", "3"))]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and any(f in r.stdout for f in ("-G", "-T", "-U", "-M")), (args, r.stdout, r.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]


def test_host_functions_under_the_sanitizers():
    """tests/tools/groups_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the
    labels reader, the bounds and the two CSV writers (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "groups_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "groups host functions OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def fetch(ctx, k, d_mn, d_lo, d_hi, off):
    """the keys of sketches on the device -> one list of (minimizer, kmer_hi, kmer_lo) per sketch, in the device's order"""
    total = int(off[-1])
    if not total:
        return [[] for _ in range(len(off) - 1)]
    mn, lo = ctx.to_host(d_mn, total, np.uint32).tolist(), ctx.to_host(d_lo, total, np.uint64).tolist()
    hi = ctx.to_host(d_hi, total, np.uint64).tolist() if k > 32 else [0] * total
    flat = list(zip(mn, hi, lo))
    return [flat[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


def device_call(ctx, sketches, k, group, G, num, den, onum=0, oden=1, lead=0):
    """-> (group rows, member rows, markers per group) as the model returns them; lead: entries in front of the first sketch"""
    mn, lo, hi, off, order = tp.pack(sketches, k)
    if lead:
        junk = tp.pool(lead, k, salt=777_000)[::-1]                                         # (unsorted, and nobody's)
        mn = np.concatenate([np.array([x[0] for x in junk], np.uint32), mn])
        lo = np.concatenate([np.array([x[2] for x in junk], np.uint64), lo])
        hi = np.concatenate([np.array([x[1] for x in junk], np.uint64), hi]) if hi is not None else None
        off = off + np.uint64(lead)
    d = tp.upload(mn, lo, hi)
    n = len(order)
    rows, members, (o_mn, o_lo, o_hi, moff) = ctx.groups_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, n, group, G, num, den, onum, oden, want_markers=True)
    assert moff[0] == 0 and np.diff(moff.astype(np.int64)).tolist() == rows["marker"].tolist()
    markers = fetch(ctx, k, o_mn, o_lo, o_hi, moff)
    plain = ctx.groups_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, n, group, G, num, den, onum, oden)
    del d
    got = (as_tuples(rows, G_FIELDS), as_tuples(members, M_FIELDS), markers)
    assert (as_tuples(plain[0], G_FIELDS), as_tuples(plain[1], M_FIELDS)) == got[:2]        # without markers: the same rows
    return got


def check(ctx, sketches, k, group, G, num, den, onum=0, oden=1, lead=0):
    got = device_call(ctx, sketches, k, group, G, num, den, onum, oden, lead)
    want = model(sketches, group, G, num, den, onum, oden)
    assert got[0] == want[0], [(c, a, b) for c, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:4]
    assert got[1] == want[1], [(i, a, b) for i, (a, b) in enumerate(zip(got[1], want[1])) if a != b][:4]
    for c in range(G):
        assert got[2][c] == want[2][c], (c, len(got[2][c]), len(want[2][c]))
    return want


def from_holders(n, holders, k, salt=0):
    """holders[x] = the sketches that hold key x -> n lists of key tuples"""
    keys = tp.pool(len(holders), k, salt)
    sketches = [[] for _ in range(n)]
    for key, hs in zip(keys, holders):
        for s in hs:
            sketches[s].append(key)
    return sketches


def hand_key(k):
    p = tp.pool(8, k, salt=40)
    return lambda x: p[x]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_smallest_collections(ctx, k):
    rows, members, markers = check(ctx, [tp.pool(300, k)], k, [0], 1, 1, 1)                 # n = 1
    assert rows == [(1, 300, 300, 300, 300, 300)] and members == [(300, 300, 300)]
    check(ctx, [[]], k, [0], 1, 1, 2)
    # the hand-made case at both outside thresholds
    sets = hand_sets(hand_key(k))
    rows, members, markers = check(ctx, sets, k, HAND_GROUP, 3, 2, 3)
    assert rows == [(3, 11, 5, 4, 2, 1), (2, 5, 3, 2, 1, 1), (1, 3, 3, 3, 1, 1)]
    assert members == [(3, 2, 1), (2, 1, 1), (4, 1, 1), (2, 1, 1), (3, 1, 1), (3, 1, 1)]
    rows, members, markers = check(ctx, sets, k, HAND_GROUP, 3, 2, 3, 1, 3)
    assert [len(m) for m in markers] == [3, 1, 1]
    check(ctx, sets, k, HAND_GROUP, 3, 2, 3, lead=5)                                        # h_sk_off[0] > 0
    check(ctx, sets, k, HAND_GROUP, 3, 1, 2, 1, 1, lead=70)
    # empty sketches first, in the middle and last; a group made only of empty sketches; nothing but empty sketches
    body = tp.nested_lengths(k, [5, 3, 4])
    sk = [[], body[0], [], body[1], [], body[2], []]
    rows, _, markers = check(ctx, sk, k, [1, 0, 1, 0, 2, 2, 1], 3, 1, 2)
    assert rows[1] == (3, 0, 0, 0, 0, 0) and markers[1] == []
    check(ctx, sk, k, [0, 0, 1, 1, 2, 2, 3], 4, 1, 1, 1, 2)
    rows, _, _ = check(ctx, [[], [], []], k, [0, 1, 0], 2, 1, 1)
    assert rows == [(2, 0, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_one_group_and_one_group_per_sketch(ctx, k):
    sketches = tp.nested_lengths(k, [300, 257, 256, 64, 1, 0, 211]) + [tp.pool(90, k, salt=9000)]
    mn, lo, hi, off, order = tp.pack(sketches, k)
    n = len(order)
    h = Counter(x for s in order for x in s)
    d = tp.upload(mn, lo, hi)
    for num, den in ((1, 1), (1, 2), (3, 8), (1, 1_000_000)):
        # G = 1: exclusive = present, marker = core, whatever the outside tolerance is
        rows, members, markers = check(ctx, sketches, k, [0] * n, 1, num, den)
        assert rows[0][2] == rows[0][4] == len(h) and rows[0][3] == rows[0][5] and check(ctx, sketches, k, [0] * n, 1, num, den, 1, 1)[0] == rows
        core_min = -(-num * n // den)
        p_rows, spectrum = ctx.prevalence_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, n, num, den)
        assert [m[0] for m in members] == p_rows["core"].tolist() and rows[0][3] == int(spectrum[core_min:].sum()) and rows[0][1] == int(p_rows["holders"].sum()) - \
            sum(hx * (hx - 1) for hx in h.values())
        s_mn, s_lo, s_hi, s_off = ctx.select_device(k, tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, n, core_min, n, merged=True)
        assert fetch(ctx, k, s_mn, s_lo, s_hi, s_off) == markers
        # G = n: h_c = 1, core = present, exclusive = the keys nobody else holds
        rows, members, markers = check(ctx, sketches, k, list(range(n)), n, num, den)
        assert all(r[2] == r[3] == r[1] for r in rows) and [m[1] for m in members] == [sum(1 for x in s if h[x] == 1) for s in order]
        assert markers == [[x for x in s if h[x] == 1] for s in order]
    del d


@pytest.mark.gpu
def test_labels_interleaved_and_renumbered(ctx):
    k, n, G = 31, 23, 4
    rng = np.random.default_rng(3)
    holders = [sorted(rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False).tolist()) for _ in range(400)]
    sketches = from_holders(n, holders, k)
    group = [i % G for i in range(n)]                                                      # interleaved in list order
    for t in ((1, 2, 0, 1), (2, 3, 1, 4), (1, 1, 1, 2)):
        rows, members, markers = check(ctx, sketches, k, group, G, *t)
        # a permutation of the sketches: the group rows and the marker sets stay, the member rows move with their sketches
        perm = rng.permutation(n).tolist()
        p_rows, p_members, p_markers = check(ctx, [sketches[i] for i in perm], k, [group[i] for i in perm], G, *t)
        assert (p_rows, p_markers) == (rows, markers) and p_members == [members[i] for i in perm]
        # the groups renumbered: the rows are permuted
        new = [2, 0, 3, 1]
        r_rows, r_members, r_markers = check(ctx, sketches, k, [new[c] for c in group], G, *t)
        assert [r_rows[new[c]] for c in range(G)] == rows and [r_markers[new[c]] for c in range(G)] == markers and r_members == members
    assert any(len(m) for m in markers) and any(r[4] for r in rows)


@pytest.mark.gpu
def test_one_key_around_each_bound(ctx):
    k, n = 31, 50
    group = [0 if i % 5 < 2 else 1 + (i % 5 > 3) for i in range(n)]                        # 20 in group 0, 20 in group 1, 10 in group 2
    assert bounds(group, 3, 19, 20, 1, 10) == ([20, 20, 10], [19, 19, 10], [3, 3, 4])
    g0 = [i for i in range(n) if group[i] == 0]
    g1 = [i for i in range(n) if group[i] == 1]
    g2 = [i for i in range(n) if group[i] == 2]
    holders = [g0[:18], g0[:19], g0[:20],                                                  # h_c = 18, 19, 20 at in_min = 19
               g0 + g1[:2], g0 + g1[:3], g0 + g1[:4], g0 + g1[:2] + g2[:1], g0 + g1[:2] + g2[:2],   # 2, 3, 4 holders outside at out_max = 3
               g0[:2] + g2[:1],                                                            # (a marker of two groups at once further down)
               g1[:19] + g0[:3], g1[1:] + g0[:4]]
    sketches = from_holders(n, holders, k)
    rows, members, markers = check(ctx, sketches, k, group, 3, 19, 20, 1, 10)
    keys = tp.pool(len(holders), k)
    assert set(markers[0]) == {keys[j] for j in (1, 2, 3, 4, 6)} and markers[1] == [keys[9]] and markers[2] == []
    assert rows[0][3] == 7 and rows[0][4] == 3 and rows[1][3] == 2 and rows[2][3] == 0
    # one key that is a marker of two groups at once: 2 of 20 and 1 of 10 are core at 1 / 10, with 1 and 2 holders outside
    assert bounds(group, 3, 1, 10, 1, 10)[1:] == ([2, 2, 1], [3, 3, 4])
    _, _, markers = check(ctx, sketches, k, group, 3, 1, 10, 1, 10)
    assert keys[8] in markers[0] and keys[8] in markers[2] and keys[8] not in markers[1]
    check(ctx, sketches, k, group, 3, 19, 20)
    check(ctx, sketches, k, group, 3, 95, 100, 100_000, 1_000_000)
    check(ctx, sketches, k, group, 3, 18, 20, 9, 100)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_one_key_in_several_groups_and_many_times_in_one(ctx, k):
    n, G = 600, 5
    group = [(i * 7) % G for i in range(n)]
    own = tp.pool(n, k, salt=50_000)
    shared = tp.pool(6, k, salt=90_000)
    sketches = [[own[i], shared[0]] + ([shared[1]] if group[i] in (1, 3) else []) + ([shared[2]] if group[i] == 2 and i % 2 else []) +
                ([shared[3]] if i % 3 == 0 else []) + ([shared[4]] if group[i] != 4 else []) for i in range(n)]
    rows, members, markers = check(ctx, sketches, k, group, G, 1, 1)
    assert [r[0] for r in rows] == [120] * 5
    assert all(r[3] >= 1 for r in rows) and markers[1] == [] and rows[4][3] == 1            # every cell of shared[0] counted to its group's size
    check(ctx, sketches, k, group, G, 1, 2, 1, 2)
    check(ctx, sketches, k, group, G, 1, 3, 1, 1)
    # seven sketches of differing word-neighbours: keys that differ in one word only never share a cell
    seam = tp.seam_sketches(k)
    check(ctx, seam, k, [0, 1, 0, 1, 2, 2, 0], 3, 1, 2, 1, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 2])
def test_the_largest_collection(ctx, G):
    """65 535 sketches that all hold one key; G = 1 is the one counter that reaches 65 535"""
    n, k = 65535, 31
    sketches = tp.star(n, k)
    group = [i % G for i in range(n)]
    assert bounds(group, G, 1, 1)[0] == ([65535] if G == 1 else [32768, 32767])
    rows, members, markers = check(ctx, sketches, k, group, G, 999_999, 1_000_000)
    everybody = (3, 0, 1)
    assert all(everybody in m for m in markers) == (G == 1) and all(r[3] >= 1 for r in rows)
    if G == 2:
        rows, _, markers = check(ctx, sketches, k, group, G, 1, 2, 1, 1)
        assert all(everybody in m for m in markers)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_smallest_table(ctx, k, monkeypatch):
    """as many slots as entries and every one of them a cell of its own: every slot is taken and probe sequences wrap"""
    p = tp.pool(640, k, salt=123)
    sketches = [p[0:256], p[128:384], p[256:512], p[0:128] + p[512:640]]                    # 1 024 entries, 640 distinct keys
    group = [0, 1, 2, 3]
    assert sum(len(s) for s in sketches) == 1024 and len(Counter((x, group[i]) for i, s in enumerate(sketches) for x in s)) == 1024
    shapes = [(sketches, group, 4, (1, 1, 0, 1)), (sketches, group, 4, (1, 2, 1, 3)), (sketches, [0, 1, 0, 1], 2, (1, 2, 0, 1)),
              (tp.star(1000, k), [i % 3 for i in range(1000)], 3, (1, 2, 1, 2))]
    plain = [check(ctx, s, k, g, G, *t) for s, g, G, t in shapes]
    monkeypatch.setenv("SPSP_DEBUG_PREVALENCE_TABLE", "min")
    assert [check(ctx, s, k, g, G, *t) for s, g, G, t in shapes] == plain


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_seams_of_the_compaction(ctx, k):
    # sketch lengths around a ballot word and a tile; two groups whose members hold one pool from both ends, so that the markers of a
    # group come from several members with interleaved key order (t <= 1 / 2: the regroup and the sort are needed)
    lengths = [63, 64, 65, 2047, 2048, 2049]
    p = tp.pool(2049, k, salt=5)
    q = tp.pool(2049, k, salt=700_000)
    sketches = [p[:c] for c in lengths] + [q[-c:] for c in lengths] + [p[60:70] + q[2040:2049]]
    group = [0] * 6 + [1] * 6 + [2]
    rows, members, markers = check(ctx, sketches, k, group, 3, 1, 2, 1, 13)
    assert rows[0][5] > 2000 and rows[1][5] > 2000
    check(ctx, sketches, k, [i % 2 for i in range(13)], 2, 1, 3)
    check(ctx, sketches, k, [i % 2 for i in range(13)], 2, 1, 6, 1, 1)
    # markers on both sides of a 64-key ballot word and of a 2 048-key tile: one sketch per entry range, alone in its group, beside a
    # group that holds every other key of it
    long = tp.pool(4200, k, salt=31)
    a = sorted(long)
    for at in (63, 64, 2047, 2048):
        other = [x for j, x in enumerate(a) if j not in (at - 1, at, at + 1)]
        rows, _, markers = check(ctx, [a, other, other], k, [0, 1, 1], 2, 1, 1)
        assert markers[0] == [a[at - 1], a[at], a[at + 1]] and rows[1][5] == 0
    # a region longer than one sort tile, made of four members' runs: at least one merge pass
    big = tp.pool(9000, k, salt=77)
    parts = [big[j::4] for j in range(4)]
    rows, _, markers = check(ctx, parts + [tp.pool(10, k, salt=1)], k, [0, 0, 0, 0, 1], 2, 1, 4)
    assert rows[0][5] == 9000 and len(markers[0]) == 9000
    check(ctx, [big[:6000], big[3000:], big[::2]], k, [0, 0, 1], 2, 1, 2, 1, 1)


@pytest.mark.gpu
def test_the_same_call_twice(ctx):
    k, n, G = 63, 40, 6
    rng = np.random.default_rng(11)
    holders = [sorted(rng.choice(n, size=int(rng.integers(1, 12)), replace=False).tolist()) for _ in range(6000)]
    sketches = from_holders(n, holders, k)
    group = [int(x) for x in rng.integers(0, G, n)]
    group[:G] = range(G)
    first = device_call(ctx, sketches, k, group, G, 1, 3, 1, 5)
    assert device_call(ctx, sketches, k, group, G, 1, 3, 1, 5) == first == model(sketches, group, G, 1, 3, 1, 5)


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_against_the_rest_of_the_library(ctx, k, m):
    pl = tp.collection(k, m)[:48]                                                           # 8 families of six
    n = len(pl)
    sets = [tp.key_set(p) for p in pl]
    kk, d_mn, d_lo, d_hi, off, entries = tp.decoded(ctx, pl)
    assert kk == k
    group, G = [i // 6 for i in range(n)], 8
    for t in ((1, 1, 0, 1), (1, 2, 0, 1), (5, 6, 1, 20), (1, 6, 1, 1)):
        rows, members, (o_mn, o_lo, o_hi, moff) = ctx.groups_device(k, d_mn, d_lo, d_hi, off, n, group, G, *t, want_markers=True)
        markers = fetch(ctx, k, o_mn, o_lo, o_hi, moff)
        w_rows, w_members, w_markers = model(sets, group, G, *t)
        assert as_tuples(rows, G_FIELDS) == w_rows and as_tuples(members, M_FIELDS) == w_members and markers == w_markers
        hc = Counter((x, group[i]) for i, s in enumerate(sets) for x in s)
        assert [sum(v for (x, c), v in hc.items() if c == g) for g in range(G)] == rows["entries"].tolist()
        _, in_min, _ = bounds(group, G, *t)
        # every group's marker sketch as a query against all sketches: each of its keys has h >= in_min_c
        if moff[-1]:
            import torch
            all_mn = torch.cat([torch.from_numpy(ctx.to_host(o_mn, int(moff[-1]), np.uint32).view(np.int32)).cuda(),
                                torch.from_numpy(ctx.to_host(d_mn, int(off[-1]), np.uint32).view(np.int32)).cuda(), torch.zeros(16, dtype=torch.int32, device="cuda")])
            all_lo = torch.cat([torch.from_numpy(ctx.to_host(o_lo, int(moff[-1]), np.uint64).view(np.int64)).cuda(),
                                torch.from_numpy(ctx.to_host(d_lo, int(off[-1]), np.uint64).view(np.int64)).cuda(), torch.zeros(8, dtype=torch.int64, device="cuda")])
            all_hi = None
            if k > 32:
                all_hi = torch.cat([torch.from_numpy(ctx.to_host(o_hi, int(moff[-1]), np.uint64).view(np.int64)).cuda(),
                                    torch.from_numpy(ctx.to_host(d_hi, int(off[-1]), np.uint64).view(np.int64)).cuda(), torch.zeros(8, dtype=torch.int64, device="cuda")])
            torch.cuda.synchronize()
            q_off = np.concatenate([moff, off[1:] + moff[-1]]).astype(np.uint64)
            _, _, d_held = ctx.prevalence_device(k, all_mn.data_ptr(), all_lo.data_ptr(), tp.ptr(all_hi), q_off, G + n, 1, 1, n_query=G, want_holders=True)
            held = ctx.to_host(d_held, int(moff[-1]), np.uint32).tolist()
            for c in range(G):
                assert all(v >= in_min[c] for v in held[int(moff[c]):int(moff[c + 1])]), c
            del all_mn, all_lo, all_hi
        if t[2] == 0:                                                                       # nobody outside: no key marks two groups
            flat = [x for mk in markers for x in mk]
            assert len(flat) == len(set(flat))
    assert sum(len(mk) for mk in model(sets, group, G, 1, 1)[2]) > 8
    # G = 1 is the prevalence spectrum's cumulative at core_min
    for num, den in ((1, 1), (1, 8), (1, 2)):
        rows, members = ctx.groups_device(k, d_mn, d_lo, d_hi, off, n, [0] * n, 1, num, den)
        _, spectrum = ctx.prevalence_device(k, d_mn, d_lo, d_hi, off, n, num, den)
        assert int(rows["core"][0]) == int(spectrum[-(-num * n // den):].sum()) == int(rows["marker"][0]) and int(rows["present"][0]) == int(spectrum.sum())


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(ctx):
    k = 31
    sketches = tp.nested_lengths(k, [70, 3, 0, 130])
    group = [0, 1, 0, 1]
    mn, lo, hi, off, order = tp.pack(sketches, k)
    want = model(order, group, 2, 1, 2)
    d = tp.upload(mn, lo, hi)
    n = len(off) - 1
    L = sp.lib()
    rows = np.zeros(4, dtype=sp.GROUP_ROW_DTYPE)
    members = np.zeros(n, dtype=sp.GROUP_MEMBER_ROW_DTYPE)
    moff = np.zeros(5, dtype=np.uint64)
    import ctypes as C
    outs = [C.c_void_p() for _ in range(3)]

    def call(n=n, group=group, G=2, num=1, den=2, onum=0, oden=1, off=off, d=d, kk=k):
        g = np.array(group, dtype=np.uint32)
        rows[:] = (1, 1, 1, 1, 1, 1)
        members[:] = (1, 1, 1)
        moff[:] = 1
        return L.spsp_groups_device(ctx._h, kk, tp.ptr(d[0]), tp.ptr(d[1]), None, off.ctypes.data, n, g.ctypes.data, G, num, den, onum, oden, rows.ctypes.data,
                                    members.ctypes.data, 1, C.byref(outs[0]), C.byref(outs[1]), C.byref(outs[2]), moff.ctypes.data)

    def good():
        assert call() == 0
        got = (as_tuples(rows[:2], G_FIELDS), as_tuples(members, M_FIELDS), fetch(ctx, k, outs[0].value, outs[1].value, None, moff[:3]))
        assert got == want

    good()
    cleared = lambda G: not rows[:G].view(np.uint64).any() and not members.view(np.uint64).any() and not moff[:G + 1].any()
    for kw in (dict(G=0), dict(G=5), dict(n=0), dict(group=[0, 2, 0, 1]), dict(group=[0, 0, 0, 0]), dict(group=[0, 2, 0, 2], G=3), dict(num=0), dict(num=3, den=2),
               dict(den=1_000_001), dict(onum=2, oden=1), dict(oden=0), dict(oden=1_000_001), dict(kk=0), dict(kk=64)):
        assert call(**kw) == sp.ERR_ARG, kw
        if 1 <= kw.get("G", 2) <= 4 and kw.get("n", n):
            assert cleared(kw.get("G", 2)), kw
    assert call(group=[0, 2, 0, 2], G=3) == sp.ERR_ARG and "group 1 has no member" in L.spsp_last_error().decode()
    big_off = np.zeros(65536 + 1, dtype=np.uint64)
    assert L.spsp_groups_device(ctx._h, k, tp.ptr(d[0]), tp.ptr(d[1]), None, big_off.ctypes.data, 65536, np.zeros(65536, np.uint32).ctypes.data, 1, 1, 1, 0, 1,
                                rows.ctypes.data, None, 0, None, None, None, None) == sp.ERR_ARG
    down = off.copy()
    down[2] = down[1] - 1
    assert call(off=down) == sp.ERR_ARG and "decrease" in L.spsp_last_error().decode() and cleared(2)
    huge = off.copy()
    huge[-1] = 0xfffffff1
    assert call(off=huge) == sp.ERR_OVERFLOW and cleared(2)
    ctx.compare_keys_unordered(True)
    try:
        assert call() == sp.ERR_ARG and "unordered" in L.spsp_last_error().decode() and cleared(2)
    finally:
        ctx.compare_keys_unordered(False)
    good()
    # keys out of order inside a sketch, and a key twice
    for at in (int(off[3]) + 64, 10, int(off[3]) + 1):
        bad_mn, bad_lo = mn.copy(), lo.copy()
        if at == int(off[3]) + 1:
            bad_mn[at], bad_lo[at] = bad_mn[at - 1], bad_lo[at - 1]
        else:
            bad_mn[[at, at + 1]], bad_lo[[at, at + 1]] = bad_mn[[at + 1, at]], bad_lo[[at + 1, at]]
        bad = tp.upload(bad_mn, bad_lo)
        assert call(d=bad) == sp.ERR_ARG and "increasing" in L.spsp_last_error().decode() and cleared(2), at
        del bad
    good()
    assert check(ctx, sketches, k, group, 2, 1, 2) == want


def gunzip(path):
    return gzip.open(path, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_groups_files_and_the_command_line(ctx, tmp_path, k, m):
    pl = tp.collection(k, m)[:24]                                                           # four families of six, listed family by family
    n = len(pl)
    order = [(i % 4) * 6 + i // 4 for i in range(n)]                                        # ... and here interleaved
    pl = [pl[i] for i in order]
    labels = ["family %d" % (i // 6) for i in order]
    names = []
    for x in labels:
        if x not in names:
            names.append(x)
    group = [names.index(x) for x in labels]
    sets = [tp.key_set(p) for p in pl]
    card = [len(s) for s in sets]
    paths = tp.write_files(tmp_path, pl)
    (tmp_path / "labels.txt").write_text("\n".join(labels) + "\n")
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    want = model(sets, group, 4, 9, 10, 5, 100)
    assert bounds(group, 4, 9, 10, 5, 100)[1:] == ([6] * 4, [0] * 4) and sum(len(mk) for mk in want[2]) > 4
    texts = [py_groups_csv(want[0], names), py_members_csv(want[1], paths, group, card, want[0], names)]
    rows, members = ctx.groups_files(paths, str(tmp_path / "lib"), str(tmp_path / "labels.txt"), 9, 10, 5, 100, markers=True)
    assert as_tuples(rows, G_FIELDS) == want[0] and as_tuples(members, M_FIELDS) == want[1]
    both = lambda tag: [gunzip(str(tmp_path / (tag + suf))) for suf in ("_groups.csv.gz", "_members.csv.gz")]
    assert both("lib") == texts
    ctx.groups_files(paths, str(tmp_path / "p3"), str(tmp_path / "labels.txt"), 9, 10, 5, 100, precision=3)
    assert both("p3") == [py_groups_csv(want[0], names, 3), py_members_csv(want[1], paths, group, card, want[0], names, 3)]
    assert not os.path.exists(str(tmp_path / "p3_markers.txt"))
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    r = run("-G", "labels.txt", "-T", "0.9", "-U", "0.05", "-M", "-f", "bank.txt", "-o", "cli")
    assert r.returncode == 0, r.stdout + r.stderr
    assert both("cli") == texts
    listed = (tmp_path / "cli_markers.txt").read_bytes()
    assert listed == "".join("cli_markers_%d.gz\n" % c for c in range(4)).encode()
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("cli")) == sorted(["cli_groups.csv.gz", "cli_members.csv.gz", "cli_markers.txt"] +
                                                                                 ["cli_markers_%d.gz" % c for c in range(4)])
    for c in range(4):
        written = gunzip(str(tmp_path / ("cli_markers_%d.gz" % c)))
        s = sp.sketch_parse(written)
        assert list(zip(s.minimizer.tolist(), s.kmer_hi.tolist(), s.kmer_lo.tolist())) == want[2][c]
        assert sp.sketch_header(written) == (k, m, len(want[2][c]), 100.0)
        assert written == gunzip(str(tmp_path / ("lib_markers_%d.gz" % c)))
    # which family is this isolate: a member as the query against the marker sketches
    (tmp_path / "q.txt").write_text(paths[0] + "\n")
    r = run("-q", "q.txt", "-f", "cli_markers.txt", "-o", "which")
    assert r.returncode == 0, r.stdout + r.stderr
    assert os.path.exists(str(tmp_path / "which_containment.csv.gz"))
    # a group without a marker gets the sketch of no keys (-T 1 -U 0 over two groups of two unrelated families each: nothing is core)
    (tmp_path / "two.txt").write_text("\n".join("even" if i % 2 == 0 else "odd" for i in range(n)) + "\n")
    two = model(sets, [i % 2 for i in range(n)], 2, 1, 1)
    r = run("-G", "two.txt", "-M", "-f", "bank.txt", "-o", "two")
    assert r.returncode == 0, r.stdout + r.stderr
    assert two[2] == [[], []] and [sp.sketch_header(gunzip(str(tmp_path / ("two_markers_%d.gz" % c)))) for c in range(2)] == [(k, m, 0, 100.0)] * 2
    assert gunzip(str(tmp_path / "two_groups.csv.gz")) == py_groups_csv(two[0], ["even", "odd"])
    # a labels file that does not fit is refused, naming the file and the line
    (tmp_path / "short.txt").write_text("a\nb\n")
    r = run("-G", "short.txt", "-f", "bank.txt", "-o", "no")
    assert r.returncode == 1 and "short.txt" in r.stdout and "line 3" in r.stdout and not [f for f in os.listdir(tmp_path) if f.startswith("no")]


@pytest.mark.gpu
def test_groups_files_at_mixed_rates(ctx, tmp_path):
    k, m = 31, 11
    refs = tp._references()
    coarse = tp.collection(k, m)[:12]
    mixed_rates = [tp._sketch(g, "g%d" % i, k, m, 10.0) if i % 3 == 0 else coarse[i] for i, g in enumerate(refs[:12])]
    paths = tp.write_files(tmp_path, mixed_rates)
    labels = str(tmp_path / "labels.txt")
    (tmp_path / "labels.txt").write_text("".join("f%d\n" % (i // 6) for i in range(12)))
    group = [i // 6 for i in range(12)]
    sets = [tp.key_set(p) for p in coarse]
    want = model(sets, group, 2, 1, 2)
    for rate in ("auto", 100):
        rows, members = ctx.groups_files(paths, str(tmp_path / "a"), labels, 1, 2, markers=True, rate=rate)
        assert as_tuples(rows, G_FIELDS) == want[0] and as_tuples(members, M_FIELDS) == want[1]
        for c in range(2):
            written = gunzip(str(tmp_path / ("a_markers_%d.gz" % c)))
            assert sorted(tp.key_set(written)) == want[2][c] and sp.sketch_header(written) == (k, m, len(want[2][c]), 100.0)
    # as the files are: another question with another answer, and no rate to write into a marker sketch
    rows, members = ctx.groups_files(paths, str(tmp_path / "asis"), labels, 1, 2)
    assert as_tuples(rows, G_FIELDS) == model([tp.key_set(p) for p in mixed_rates], group, 2, 1, 2)[0]
    with pytest.raises(sp.SpspError) as e:
        ctx.groups_files(paths, str(tmp_path / "no"), labels, 1, 2, markers=True)
    assert e.value.code == sp.ERR_ARG and "different rates" in str(e.value) and not [f for f in os.listdir(tmp_path) if f.startswith("no")]
    # ... and the same through the command line: -s auto writes what the library call wrote, no rate with -M is refused
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    r = run("-G", "labels.txt", "-T", "0.5", "-M", "-s", "auto", "-f", "bank.txt", "-o", "cli")
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("_groups.csv.gz", "_members.csv.gz", "_markers_0.gz", "_markers_1.gz"):
        assert gunzip(str(tmp_path / ("cli" + name))) == gunzip(str(tmp_path / ("a" + name))), name
    r = run("-G", "labels.txt", "-T", "0.5", "-M", "-f", "bank.txt", "-o", "no")
    assert r.returncode == 1 and "different rates" in r.stdout and not [f for f in os.listdir(tmp_path) if f.startswith("no")]
    with pytest.raises(sp.SpspError) as e:
        ctx.groups_files(paths, str(tmp_path / "no"), labels, 1, 2, rate=10)
    assert e.value.code == sp.ERR_ARG and "upsample" in str(e.value)
    kk = [tp._sketch(g[:5000], "g%d" % i, 11, 11) for i, g in enumerate(refs[:3])]
    (tmp_path / "l3.txt").write_text("a\na\nb\n")
    for rate in (0.0, "auto"):
        with pytest.raises(sp.SpspError) as e:
            ctx.groups_files(tp.write_files(tmp_path, kk, "kk"), str(tmp_path / "no"), str(tmp_path / "l3.txt"), 1, 2, rate=rate)
        assert e.value.code == sp.ERR_ARG and "k == m" in str(e.value)
