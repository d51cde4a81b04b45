"""Profile: which references a read set holds, each shared key counted once, and how deep each one is (include/spsp.h:
spsp_profile_device, spsp_profile_stage_ms, spsp_profile_counts, spsp_profile_csv_host, spsp_profile_files; bin/comparator -D .. -B).

The rule, on the comparator's keys.  Index and counts as in test_depth: references 0 .. R-1 with key sets K_j, c(x) the records that
hold x.  F = {x : c(x) >= min_count}, A_0 = F; round r: u_j = |K_j n A_(r-1)|, j* the smallest j among the largest u_j; stop if
u_j* < min_keys or (max_rounds > 0 and r > max_rounds); else one row and A_r = A_(r-1) \\ K_j*.

Every expected value below comes from `model`: Python sets over test_depth's Counter.  No tolerance anywhere.  As in test_depth,
key x gets the count c by appearing c times in the shuffled record-key array.

Where the kernels cut: the pick is one workgroup of 1 024 lanes; rounds are queued 32, 64, 128, 128, ... per host wait; the walk
hands a list of more than `list_cut` holders to a whole wave, and counts its decrements in LDS up to `lds_refs` references; the statistics are the depth reduction's (the last histogram bin,
the segments of a reference of more than kDpLongKeys entries)."""
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest

import supersampler_amd as sp
import test_depth as td
import test_gather as tg
import test_prevalence as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
HEADER = "rank,reference,keys,found,f_found,assigned,f_assigned,median,mean,max,f_weighted,remaining\n"
FIELDS = ("reference", "keys", "found", "assigned", "sum", "median", "max", "remaining")
TOTALS = ("found_keys", "found_sum", "assigned_keys", "assigned_sum")


# -------------------------------------------------------------------------------------------------- the model

def model(refs, record_keys, min_count=1, min_keys=1, max_rounds=0):
    """-> (rows: per round the eight numbers of FIELDS, totals: the four of TOTALS, assigned: per reference the keys it was given)"""
    assert min_count >= 1 and min_keys >= 1
    refs = [set(K) for K in refs]
    c = td.model(refs, record_keys)[2]
    F = {x for x, n in c.items() if n >= min_count}
    A, rows, assigned = set(F), [], [set() for _ in refs]
    while True:
        u = [len(K & A) for K in refs]
        best = max(u) if u else 0
        if best < min_keys or (max_rounds > 0 and len(rows) + 1 > max_rounds):
            break
        j = u.index(best)                                                              # the first of the largest
        got = sorted(c[x] for x in refs[j] & A)
        rows.append((j, len(refs[j]), len(refs[j] & F), best, sum(got), got[(best - 1) // 2], got[-1], len(A) - best))
        assigned[j] = refs[j] & A
        A -= refs[j]
    return rows, (len(F), sum(c[x] for x in F), sum(r[3] for r in rows), sum(r[4] for r in rows)), assigned


def as_tuples(rows):
    return [tuple(int(r[f]) for f in FIELDS) for r in rows]


def as_totals(t):
    return tuple(int(t[f]) for f in TOTALS)


def as_array(rows):
    out = np.zeros(len(rows), dtype=sp.PROFILE_ROW_DTYPE)
    for i, r in enumerate(rows):
        for f, v in zip(FIELDS, r):
            out[i][f] = v
    return out


def totals_array(t):
    out = np.zeros(1, dtype=sp.PROFILE_TOTALS_DTYPE)
    for f, v in zip(TOTALS, t):
        out[0][f] = v
    return out[0]


def py_csv(rows, totals, names, precision=6):
    g = lambda a, b: "%.*g" % (precision, a / b) if b else "0"
    text = HEADER
    for rank, (j, keys, found, assigned, total, median, top, remaining) in enumerate(rows, 1):
        text += "%d,%s,%d,%d,%s,%d,%s,%d,%s,%d,%s,%d\n" % (rank, names[j], keys, found, g(found, keys), assigned, g(assigned, totals[0]), median,
                                                           g(total, assigned), top, g(total, totals[1]), remaining)
    return text.encode()


def check_facts(rows, totals, min_keys=1, max_rounds=0):
    """the facts the rule implies (include/spsp.h), on any rows"""
    left, last = totals[0], None
    for j, keys, found, assigned, total, median, top, remaining in rows:
        assert 1 <= assigned <= found <= keys and (last is None or assigned <= last)
        assert remaining == left - assigned and assigned <= total <= assigned * top and 1 <= median <= top
        left, last = remaining, assigned
    assert len({r[0] for r in rows}) == len(rows)
    if min_keys == 1 and max_rounds == 0:
        assert left == 0


# ------------------------------------------------------------------------------------------------ not GPU

K, times = td.K, td.times


def test_model_on_a_hand_made_case():
    refs = [K(1, 2, 3), K(3, 4, 5), K(2, 3), K(6, 7), K()]
    # c: 1 -> 5, 2 -> 1, 3 -> 2, 4 -> 7, 5 -> 3, 6 -> 2, 7 -> 1, and 77 is no key of the index
    reads = times([(1, 5), (2, 1), (3, 2), (4, 7), (5, 3), (6, 2), (7, 1), (77, 4)])
    rows, totals, assigned = model(refs, reads)
    # references 0 and 1 tie at three keys: the lower index wins; reference 1 keeps 4 and 5, which ties with reference 3 and wins again;
    # reference 2, whose keys reference 0 took, is never named
    assert rows == [(0, 3, 3, 3, 8, 2, 5, 4), (1, 3, 3, 2, 10, 3, 7, 2), (3, 2, 2, 2, 3, 1, 2, 0)]
    assert totals == (7, 21, 7, 21) and assigned[2] == set() and assigned[1] == set(K(4, 5))
    check_facts(rows, totals)
    # min_count = 2 takes keys 2 and 7 out of F: reference 1 now has three live keys against two of reference 0
    rows2, totals2, assigned2 = model(refs, reads, 2)
    assert rows2 == [(1, 3, 3, 3, 12, 3, 7, 2), (0, 3, 2, 1, 5, 5, 5, 1), (3, 2, 1, 1, 2, 2, 2, 0)]
    assert totals2 == (5, 19, 5, 19) and assigned2[0] == set(K(1))
    check_facts(rows2, totals2)
    assert model(refs, reads, 1, 3)[0] == rows[:1] and model(refs, reads, 1, 2)[0] == rows                 # min_keys
    assert model(refs, reads, 1, 1, 2)[0] == rows[:2] and model(refs, reads, 1, 1, 2)[1] == (7, 21, 5, 18)   # max_rounds
    assert model(refs, reads, 8) == ([], (0, 0, 0, 0), [set()] * 5)                                          # an empty F
    assert model(refs, Counter(reads)) == model(refs, reads)


CALLS = ("spsp_profile_device", "spsp_profile_stage_ms", "spsp_profile_counts", "spsp_profile_csv_host", "spsp_profile_files")


def test_abi_has_the_profile_calls():
    assert set(CALLS) <= set(sp.ABI_SYMBOLS)
    assert sp.PROFILE_ROW_DTYPE.itemsize == 40 and sp.PROFILE_TOTALS_DTYPE.itemsize == 24
    assert sp.PROFILE_ROW_DTYPE.names == ("sum", "reference", "keys", "found", "assigned", "median", "max", "remaining", "reserved")
    assert sp.PROFILE_TOTALS_DTYPE.names == ("found_sum", "assigned_sum", "found_keys", "assigned_keys")
    for name in CALLS:
        assert hasattr(sp.lib(), name)


#        reference keys found assigned sum median max remaining
ROWS = [(2, 10, 9, 8, 40, 4, 9, 12), (0, 12, 8, 8, 30, 3, 7, 4), (1, 5, 4, 3, 3, 1, 1, 1)]
ROW_TOTALS = (20, 100, 19, 73)
NAMES = ["a one.fa.gz", "dir/b.two", "c"]


def test_the_csv_writer_equals_the_python_writer():
    big = [(0, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff * 0xffffffff, 1 << 31, 0xffffffff, 0)]
    big_totals = (0xffffffff, 0xffffffff * 0xffffffff, 0xffffffff, 0xffffffff * 0xffffffff)
    for precision in (6, 3):
        assert sp.profile_csv(as_array(ROWS), totals_array(ROW_TOTALS), NAMES, precision) == py_csv(ROWS, ROW_TOTALS, NAMES, precision)
        assert sp.profile_csv(as_array(big), totals_array(big_totals), NAMES, precision) == py_csv(big, big_totals, NAMES, precision)
    lines = sp.profile_csv(as_array(ROWS), totals_array(ROW_TOTALS), NAMES).decode().splitlines()
    assert lines[0] + "\n" == HEADER and lines[1] == "1,c,10,9,0.9,8,0.4,4,5,9,0.4,12" and lines[3] == "3,dir/b.two,5,4,0.8,3,0.15,1,1,1,0.03,1"
    assert sp.profile_csv(as_array(ROWS), totals_array(ROW_TOTALS), NAMES, 3).decode().splitlines()[2] == "2,a one.fa.gz,12,8,0.667,8,0.4,3,3.75,7,0.3,4"
    assert sp.profile_csv(as_array([]), totals_array((0, 0, 0, 0)), NAMES) == HEADER.encode()
    assert sp.profile_csv(as_array([]), totals_array((0, 0, 0, 0)), []) == HEADER.encode()
    m = model([K(1, 2, 3), K(3, 4, 5), K(6)], times([(1, 5), (3, 2), (4, 7), (6, 1)]))
    assert sp.profile_csv(as_array(m[0]), totals_array(m[1]), NAMES) == py_csv(m[0], m[1], NAMES)


#      rank 2 in the place of ROWS[1]
BAD = [(0, 12, 9, 9, 30, 3, 7, 3),             # assigned increases from one row to the next
       (0, 12, 8, 0, 0, 0, 0, 12),             # nothing assigned
       (0, 12, 7, 8, 30, 3, 7, 4),             # assigned > found
       (0, 7, 8, 8, 30, 3, 7, 4),              # found > keys
       (2, 12, 8, 8, 30, 3, 7, 4),             # a reference twice
       (3, 12, 8, 8, 30, 3, 7, 4),             # a reference the index does not have
       (0, 12, 8, 8, 30, 3, 7, 5),             # remaining is not the last remaining less assigned
       (0, 12, 8, 8, 30, 3, 7, 3),
       (0, 12, 8, 8, 7, 1, 1, 4),              # sum < assigned
       (0, 12, 8, 8, 57, 3, 7, 4),             # sum > assigned * max
       (0, 12, 8, 8, 30, 0, 7, 4),             # median == 0
       (0, 12, 8, 8, 30, 8, 7, 4)]             # median > max


def test_the_csv_writer_refuses_rows_that_contradict_the_rule():
    for row in BAD:
        with pytest.raises(sp.SpspError) as e:
            sp.profile_csv(as_array([ROWS[0], row, ROWS[2]]), totals_array(ROW_TOTALS), NAMES)
        assert e.value.code == sp.ERR_ARG and "rank 2" in str(e.value), row
    with pytest.raises(sp.SpspError) as e:                                             # remaining_0 is |F|
        sp.profile_csv(as_array(ROWS), totals_array((21, 100, 19, 73)), NAMES)
    assert e.value.code == sp.ERR_ARG and "rank 1" in str(e.value)
    with pytest.raises(sp.SpspError) as e:                                             # more rows than references
        sp.profile_csv(as_array(ROWS), totals_array(ROW_TOTALS), NAMES[:2])
    assert e.value.code == sp.ERR_ARG and "rank 3" in str(e.value)
    assert sp.profile_csv(as_array(ROWS), totals_array(ROW_TOTALS), NAMES)


def test_host_functions_under_the_sanitizers():
    """tests/tools/profile_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the CSV
    writer with its refusals (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "profile_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "profile_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-B", "1")] + [("-D", "r.fq", "-B", v) for v in ("0", "-1", "abc", "4294967296", "")] + [("-D", "r.fq", "-B", "1", "-X", "r.fa")]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1, (args, r.stdout, r.stderr)
        assert any(o in r.stdout for o in ("-B", "-D")), (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
    assert "-B" in run("-B", "1", "-f", "list.txt", "-o", "bad").stdout and "needs -D" in run("-B", "1", "-f", "list.txt", "-o", "bad").stdout


def test_with_every_count_one_the_rule_is_gathers():
    rng = random.Random(3)
    p = tp.pool(300, 31)
    refs = [rng.sample(p[:250], rng.randint(0, 60)) for _ in range(25)] + [p[:40], p[:40]]       # a tie among them
    union = sorted(set(x for K_ in refs for x in K_))
    reads = rng.sample(union, 150)                                                      # distinct: every count is 1; all of them index keys (gather's
                                                                                        # `remaining` also counts the query keys no reference holds)
    for min_keys, max_rounds in ((1, 0), (4, 0), (1, 5)):
        rows = model(refs, reads, 1, min_keys, max_rounds)[0]
        want = tg.gather_model(set(reads), [set(K) for K in refs], min_keys, max_rounds)
        assert [(r[0], r[3], r[7]) for r in rows] == [(j, unique, remaining) for _, j, _, unique, remaining in want] and rows
        assert [r[2] for r in rows] == [w[2] for w in want]                             # found is gather's intersect


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def add_counts(index, keys, counts, seed):
    """key i `counts[i]` times, shuffled"""
    mn, lo, hi = td.key_arrays(keys, index.k)
    order = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(keys)), counts))
    index.add((mn[order], lo[order], hi[order] if hi is not None else None))


def check(ctx, index, refs, reads, min_count=1, min_keys=1, max_rounds=0):
    """one profile_read against the model: rows, totals and the assigned bytes"""
    want_rows, want_totals, want_assigned = model(refs, reads, min_count, min_keys, max_rounds)
    rows, totals, d = ctx.profile_read(min_count, min_keys, max_rounds, want_assigned=True)
    index.alive = []                                                                   # (the call waited: the adds are through)
    rows = as_tuples(rows)
    assert as_totals(totals) == want_totals, (as_totals(totals), want_totals)
    assert rows == want_rows, (len(rows), len(want_rows), [(i, a, b) for i, (a, b) in enumerate(zip(rows, want_rows)) if a != b][:3])
    check_facts(rows, want_totals, min_keys, max_rounds)
    if index.entries:
        got = ctx.to_host(d, len(index.entries), np.uint8)
        want = np.array([x in want_assigned[j] for j, s in enumerate(index.order[1:]) for x in s], dtype=np.uint8)
        assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    return rows


def begin_and_add(ctx, k, refs, reads, seed=1, lead=()):
    index = td.Index(ctx, k, refs, lead)
    ctx.depth_begin()
    index.add(list(reads.elements()) if isinstance(reads, Counter) else reads, seed)
    return index


@pytest.mark.gpu
@pytest.mark.parametrize("top", [(0,), (1023,), (1024,), (2048,), (1023, 1024), (0, 2048)])
def test_the_arg_max_over_2049_references(ctx, top):
    """the pick's 1 024 lanes take two or three references each: the maximum alone at the first and last reference and on both
    sides of lane 1 023, and ties across those places, which go to the lower index"""
    k, R = 31, 2049
    p = tp.pool(3 * R, k)
    refs = [p[3 * j:3 * j + (3 if j in top else 1 + j % 2)] for j in range(R)]
    index = begin_and_add(ctx, k, refs, [x for K_ in refs for x in K_])
    rows = check(ctx, index, refs, [x for K_ in refs for x in K_], max_rounds=40)     # (past the first batch of 32 rounds)
    assert [r[0] for r in rows[:len(top)]] == list(top) and rows[len(top)][3] == 2 and len(rows) == 40
    del index


@pytest.mark.gpu
def test_rounds_across_the_batch_seams(ctx):
    """97 rounds = 32 + 64 + 1; a round limit and a stop by min_keys on the last round of a batch and on either side of it"""
    k, n = 63, 97
    p = tp.pool(n * (n + 1) // 2, k)
    refs, at = [], 0
    for j in range(n):                                                                 # disjoint, 97 keys down to 1
        refs.append(p[at:at + n - j]); at += n - j
    order = list(range(n))
    random.Random(4).shuffle(order)
    refs = [refs[j] for j in order]                                                    # (the winners come in no order of the index)
    reads = [x for K_ in refs for x in K_]
    index = begin_and_add(ctx, k, refs, reads)
    assert len(check(ctx, index, refs, reads)) == 97
    assert ctx.profile_stage_ms()["waits"] == 4 and ctx.profile_stage_ms()["rounds"] == 32 + 64 + 128     # three batches and the statistics
    for max_rounds in (31, 32, 33):
        assert len(check(ctx, index, refs, reads, max_rounds=max_rounds)) == max_rounds
    size33 = n - 32                                                                    # what the 33rd winner has
    assert len(check(ctx, index, refs, reads, min_keys=size33)) == 33                  # the stop is the second round of the second batch
    assert len(check(ctx, index, refs, reads, min_keys=size33 + 1)) == 32              # ... its first
    assert len(check(ctx, index, refs, reads, min_keys=size33 + 2)) == 31              # ... the last of the first batch
    assert check(ctx, index, refs, reads, min_keys=98) == []
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_holder_lists_on_both_sides_of_the_cut(ctx, k):
    """keys held by `cut` and by `cut + 1` references (a lane's loop, the whole wave), and one that all 300 hold: after round 1
    every other counter is down by exactly the keys it shared with the winner, or the later rounds' `assigned` are wrong"""
    cut = sp.classify_plan(300, 1)["list_cut"]
    assert cut == td.internal_constant("kCfListCut") == 32
    R = 300
    p = tp.pool(4000, k)
    shared = {cut: p[0:6], cut + 1: p[6:12], 2: p[12:40], 64: p[40:44], 65: p[44:48], R: p[48:49]}   # holders -> keys, the winner among the holders
    refs = [list(p[100:160]) + [x for xs in shared.values() for x in xs]]               # reference 0 holds them all, and 60 of its own
    for j in range(1, R):
        refs.append(p[200 + 12 * j:200 + 12 * j + 1 + j % 12] + [x for h, xs in shared.items() if j < h for x in xs])
    reads = Counter({x: 1 + i % 3 for i, x in enumerate(p[:3900])})
    index = begin_and_add(ctx, k, refs, reads)
    rows = check(ctx, index, refs, reads)
    assert rows[0][0] == 0 and len(rows) == R and rows[1][3] < rows[1][2]               # the second winner lost keys to the first
    check(ctx, index, refs, reads, min_count=2)
    check(ctx, index, refs, reads, min_count=3, min_keys=2)
    del index


@pytest.mark.gpu
def test_more_references_than_the_lds_counters_hold(ctx):
    """up to `lds_refs` references a workgroup of the walk counts its decrements in LDS; one more, and every holder gets a device
    atomic: both sides of that threshold, with keys two references share and one that 40 hold"""
    k = 31
    for R in (sp.classify_plan(300, 1)["lds_refs"] + d for d in (0, 1)):
        p = tp.pool(2 * R + 200, k)
        refs = [p[2 * j:2 * j + 1 + j % 2] for j in range(R)]
        refs[0] = refs[0] + p[2 * R:2 * R + 100] + p[-1:]
        refs[5] = refs[5] + p[2 * R:2 * R + 60] + p[2 * R + 100:2 * R + 150]
        for j in range(10, 49):
            refs[j] = refs[j] + p[-1:]
        refs[R - 1] = refs[R - 1] + p[2 * R + 150:2 * R + 160] + p[2 * R + 100:2 * R + 105]      # the last counter, and keys of reference 5's
        reads = [x for x in p for _ in range(1 + x[2] % 3)]
        index = begin_and_add(ctx, k, refs, reads)
        rows = check(ctx, index, refs, reads, max_rounds=40)
        assert [(r[0], r[3]) for r in rows[:4]] == [(5, 112), (0, 42), (R - 1, 11 + (R - 1) % 2), (1, 2)] and rows[-1][3] == 2
        check(ctx, index, refs, reads, min_count=2, max_rounds=5)
        del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_keys_one_short_of_min_count(ctx, k):
    """keys with c = min_count - 1 in the winner and in others: not assigned, not counted in u, and nothing decremented for them"""
    p = tp.pool(200, k)
    mc = 3
    low = p[0:30]                                                                       # c = 2
    refs = [p[100:105] + low[:20],                 # 5 found keys (25 if the low ones counted: it would win first)
            p[110:117] + low[10:30] + p[100:102],  # 7 of its own, 2 shared with reference 0
            p[120:126] + low[:5] + p[110:111],     # 6 and one shared with reference 1
            low]                                   # nothing found at all
    reads = Counter({x: 2 for x in low})
    reads.update({x: 3 + i % 4 for i, x in enumerate(p[100:130])})
    index = begin_and_add(ctx, k, refs, reads)
    rows = check(ctx, index, refs, reads, min_count=mc)
    assert [(r[0], r[3]) for r in rows] == [(1, 9), (2, 6), (0, 3)]
    assert check(ctx, index, refs, reads, min_count=2)[0][:4] == (3, 30, 30, 30)       # at 2 the low keys are found, and reference 3 is first
    check(ctx, index, refs, reads, min_count=1, min_keys=4)
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_statistics_of_the_assigned_keys(ctx, k):
    """medians that land in the last histogram bin (the radix select) over even and odd numbers of assigned keys that are not the
    found ones; counts that differ in one byte only"""
    B = sp.depth_plan()
    p = tp.pool(40, k)
    counts = {p[0]: B - 1, p[1]: B, p[2]: B + 5, p[3]: B + 0x105, p[4]: 2 * B, p[5]: B + 0x205,            # reference 0: six, all its own
              p[6]: B - 1, p[7]: B + 1, p[8]: B + 0x101, p[9]: B + 0x1ff,                                  # reference 1: these and p[4], p[5]
              p[10]: B + 2, p[11]: 3, p[12]: B + 0x102}                                                    # reference 2: these and p[0], p[1], p[7]
    refs = [p[0:6], p[6:10] + p[4:6], p[10:13] + [p[0], p[1], p[7]]]
    reads = Counter(counts)
    assert sum(reads.values()) < 10 ** 5
    index = begin_and_add(ctx, k, refs, reads)
    rows = check(ctx, index, refs, reads)
    assert [(r[0], r[2], r[3]) for r in rows] == [(0, 6, 6), (1, 6, 4), (2, 6, 3)]     # even, even below found, odd below found
    assert [r[5] for r in rows] == [B + 5, B + 1, B + 2]
    rows = check(ctx, index, refs, reads, min_count=B)                                 # F loses B - 1 and 3
    assert [(r[0], r[3], r[5]) for r in rows] == [(0, 5, B + 0x105), (1, 3, B + 0x101), (2, 2, B + 2)]
    del index


@pytest.mark.gpu
def test_a_long_winner_that_lost_keys_to_an_earlier_one(ctx):
    """a reference of 65 537 keys (reduced by segments and merged) wins SECOND: a smaller reference with more live keys took a part
    of its found keys first, and a third reference comes behind it"""
    k, L = 31, td.internal_constant("kDpLongKeys") + 1
    p = tp.pool(L + 30_100, k)
    long_ref, first, third = p[:L], p[20_000:40_000] + p[L:L + 30_000], p[L + 30_000:] + p[100:150]
    refs = [third, long_ref, first]
    count_of = np.array([1 + (i * 7919) % 5 if i < 40_000 or i >= L else 0 for i in range(len(p))])   # 40 000 of the long one's keys are found
    reads = Counter({x: int(c) for x, c in zip(p, count_of) if c})
    index = td.Index(ctx, k, refs)
    ctx.depth_begin()
    add_counts(index, p, count_of, 23)
    before = index.read()
    rows = check(ctx, index, refs, reads)
    assert [(r[0], r[1], r[2], r[3]) for r in rows] == [(2, 50_000, 50_000, 50_000), (1, L, 40_000, 20_000), (0, 150, 150, 100)]
    assert index.read() == before                                                      # the long reference's depth row is what it was
    check(ctx, index, refs, reads, min_count=3, min_keys=100)
    del index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_nothing_and_almost_nothing(ctx, k):
    p, stranger = tp.pool(60, k), tp.pool(30, k, salt=700_000)
    refs = [p[:20], [], p[10:40], []]                                                  # references without keys among others
    index = td.Index(ctx, k, refs, lead=p[50:57])                                      # and entries in front of the index
    ctx.depth_begin()
    assert check(ctx, index, refs, []) == []                                           # straight after begin: an empty F
    index.add(stranger)
    assert check(ctx, index, refs, stranger) == []                                     # reads that miss the index
    reads = td.repeat([(p[0], 3), (p[15], 2), (p[39], 1), (stranger[0], 2)])
    index.add(reads)
    assert [r[0] for r in check(ctx, index, refs, stranger + reads)] == [0, 2]
    assert check(ctx, index, refs, stranger + reads, min_count=4) == []                # above every count
    assert [r[0] for r in check(ctx, index, refs, stranger + reads, min_count=2)] == [0]
    del index
    index = td.Index(ctx, k, [[], []])                                                 # an index without keys
    ctx.depth_begin()
    index.add(p[:3])
    rows, totals = ctx.profile_read()
    assert len(rows) == 0 and as_totals(totals) == (0, 0, 0, 0)
    del index
    check(ctx, begin_and_add(ctx, k, [p[:9]], p[3:20]), [p[:9]], p[3:20])             # R = 1


@pytest.mark.gpu
def test_state_between_calls(ctx):
    k = 31
    p, stranger = tp.pool(400, k), tp.pool(50, k, salt=700_000)
    refs = [p[:150], p[100:300], p[290:400], p[120:140]]
    records = [random.Random(r).sample(p, 1 + r % 40) + stranger[r % 7:r % 7 + 2] for r in range(120)]
    flat = [x for r in records for x in r]
    half = len(flat) // 2
    fresh = sp.Context(0)
    index = td.Index(fresh, k, refs)

    def refused(call, word):
        with pytest.raises(sp.SpspError) as e:
            call()
        assert e.value.code == sp.ERR_ARG and word in str(e.value), str(e.value)

    refused(fresh.profile_read, "begin")                                               # an index, and no counters
    fresh.depth_begin()
    refused(lambda: fresh.profile_read(0), "min_count")
    refused(lambda: fresh.profile_read(1, 0), "min_keys")
    index.add(flat[:half], seed=0)
    depth_before = index.read()
    first = check(fresh, index, refs, flat[:half])
    assert index.read() == depth_before                                                # a read between two profiles is what it was
    assert check(fresh, index, refs, flat[:half]) == first                             # twice
    check(fresh, index, refs, flat[:half], min_count=2, min_keys=3)                    # other arguments, and back
    assert check(fresh, index, refs, flat[:half]) == first and index.read(2) == td.model(refs, flat[:half], 2)[:2]
    index.add(flat[half:], seed=0)                                                     # a further add: the longer multiset
    check(fresh, index, refs, flat)
    assert index.read() == td.model(refs, flat)[:2]
    fresh.timing_enable(True)
    fresh.profile_stage_ms()
    n_rows = len(check(fresh, index, refs, flat))
    ms = fresh.profile_stage_ms()
    fresh.timing_enable(False)
    assert list(ms) == ["start", "picks", "walks", "reduction", "rounds", "rows", "waits"] and all(ms[f] > 0 for f in ms)
    assert (ms["rounds"], ms["rows"], ms["waits"]) == (32, n_rows, 2) and not any(fresh.profile_stage_ms()[f] for f in ("start", "picks", "walks", "reduction"))
    index2 = td.Index(fresh, k, [p[:10]])                                              # a new index ends the counters
    refused(fresh.profile_read, "begin")
    fresh.depth_begin()
    assert len(fresh.profile_read()[0]) == 0
    del index, index2
    fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_order_and_the_cuts_of_the_adds_do_not_matter(ctx, k):
    rng = random.Random(11)
    p = tp.pool(900, k)
    refs = [rng.sample(p, rng.randint(20, 300)) for _ in range(12)]
    flat = [x for x in p[:700] for _ in range(1 + rng.randrange(6))]
    index = td.Index(ctx, k, refs)
    want = None
    for pieces, seed in ((1, 1), (2, 2), (7, 3)):
        keys = list(flat)
        random.Random(seed).shuffle(keys)
        cuts = [0] + sorted(random.Random(seed).sample(range(1, len(keys)), pieces - 1)) + [len(keys)]
        ctx.depth_begin()
        for a, z in zip(cuts, cuts[1:]):
            index.add(keys[a:z], seed=0)
        rows = check(ctx, index, refs, flat, min_count=2)
        assert want is None or rows == want
        want = rows
    del index


@pytest.mark.gpu
def test_random_families(ctx):
    """200 references in families of 10 that share most keys inside a family; reads drawn from 15 of them at depths 1 .. 40"""
    k = 31
    rng = random.Random(29)
    p = tp.pool(20 * 260 + 500, k)
    refs = []
    for f in range(20):
        core, own = p[260 * f:260 * f + 200], p[260 * f + 200:260 * f + 260]
        refs += [rng.sample(core, 170) + rng.sample(own, 30) + rng.sample(p[5200:], 3) for _ in range(10)]
    reads = Counter()
    for j in rng.sample(range(200), 15):
        depth = rng.randint(1, 40)
        reads.update({x: max(0, int(rng.gauss(depth, depth ** 0.5))) for x in refs[j] if rng.random() < 0.95})
    reads = Counter({x: c for x, c in reads.items() if c})
    index = begin_and_add(ctx, k, refs, reads, seed=31)
    for min_count in (1, 2):
        for min_keys in (1, 5):
            rows = check(ctx, index, refs, reads, min_count, min_keys)
            assert len(rows) >= 15
    del index


# ------------------------------------------------------------------------------------------ files and the command line

@pytest.mark.gpu
def test_profile_files_and_the_command_line(ctx, tmp_path):
    from supersampler_amd import synth
    k, m, s = 31, 11, 8
    gs = synth.family_genomes(7, 6, 20_000, 3, [0.0, 0.02])
    names = []
    for i, g in enumerate(gs):
        (tmp_path / ("g%d.fa" % i)).write_bytes(synth.to_fasta(g, "g%d" % i))
        names.append("g%d.fa" % i)
    (tmp_path / "g.txt").write_text("\n".join(names) + "\n")
    cli = lambda exe, *a: subprocess.run([os.path.join(ROOT, "bin", exe)] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    r = cli("sub_sampler", "-f", "g.txt", "-k", str(k), "-m", str(m), "-s", str(s), "-t", "1")
    assert r.returncode == 0, r.stdout + r.stderr
    paths = (tmp_path / "subsampled_g.txt").read_text().split()
    assert len(paths) == 6
    sources = (1, 4)                                                                   # reads of 150 bases: three-fold over one genome, 1.5-fold over another
    reads = [gs[j][a:a + 150].tobytes() for j, step in zip(sources, (50, 100)) for a in range(0, len(gs[j]) - 149, step)]
    random.Random(2).shuffle(reads)
    (tmp_path / "reads.fq").write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, q, b"I" * len(q)) for i, q in enumerate(reads)))
    full = [p_ if os.path.isabs(p_) else str(tmp_path / p_) for p_ in paths]
    d_rows, d_totals, rows, totals = ctx.profile_files(full, [str(tmp_path / "reads.fq")], str(tmp_path / "lib"))
    assert sorted(int(r["reference"]) for r in rows[:2]) == list(sources) and int(rows[0]["median"]) >= 2
    check_facts(as_tuples(rows), as_totals(totals))
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("lib")) == ["lib_depth.csv.gz", "lib_profile.csv.gz"]
    assert tp.gunzip(str(tmp_path / "lib_profile.csv.gz")) == sp.profile_csv(rows, totals, full)
    assert tp.gunzip(str(tmp_path / "lib_depth.csv.gz")) == sp.depth_csv(d_rows, full)
    r = cli("comparator", "-D", "reads.fq", "-B", "1", "-f", "subsampled_g.txt", "-o", "cli")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "profile: %d reference(s) named" % len(rows) in r.stdout and "%d record(s)" % len(reads) in r.stdout
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("cli")) == ["cli_depth.csv.gz", "cli_profile.csv.gz"]     # and no matrix files
    assert tp.gunzip(str(tmp_path / "cli_profile.csv.gz")) == sp.profile_csv(rows, totals, paths)
    r = cli("comparator", "-D", "reads.fq", "-f", "subsampled_g.txt", "-o", "only")    # -D alone: the same depth file, and no profile
    assert r.returncode == 0 and "profile:" not in r.stdout
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("only")) == ["only_depth.csv.gz"]
    assert tp.gunzip(str(tmp_path / "only_depth.csv.gz")) == tp.gunzip(str(tmp_path / "cli_depth.csv.gz"))
    assert open(str(tmp_path / "only_depth.csv.gz"), "rb").read() == open(str(tmp_path / "cli_depth.csv.gz"), "rb").read()
    with pytest.raises(sp.SpspError):                                                  # a reads file that is not there: nothing is written
        ctx.profile_files(full, [str(tmp_path / "reads.fq"), str(tmp_path / "none.fq")], str(tmp_path / "no"))
    with pytest.raises(sp.SpspError) as e:
        ctx.profile_files(full, [str(tmp_path / "reads.fq")], str(tmp_path / "no"), min_keys=0)
    assert e.value.code == sp.ERR_ARG and not [f for f in os.listdir(tmp_path) if f.startswith("no")]
