"""Windows: a long record called stretch by stretch (spsp_records_windows_host / _device, spsp_windows_expand_host,
spsp_windows_segments_host, spsp_segments_csv_host, spsp_mosaic_csv_host, spsp_windows_word_check_host, spsp_windows_plan_host,
spsp_windows_stage_ms, spsp_classify_files_windows, spsp_taxonomy_files_windows; bin/comparator -X <records> -y <W>[:<word>]).

The rule (include/spsp.h, "windows"), as the model below has it, written from the rule and not from the C: a record of L bases at
width W and step S = W - (k - 1) has max(1, ceil((L - k + 1) / S)) windows; window i holds [i S, min(i S + W, L)) and owns
[i S, (i + 1) S), the last one up to L.  The device pass is held against the expansion as plain loops, in both forms the ingest
writes; end to end the yardstick is the project's own unwindowed path on the text whose records are the windows.  Everything is
compared exactly, every window of every case: there is no tolerance anywhere."""
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
ABSENT = 0xFFFFFFFF
NEW_CALLS = ("spsp_windows_plan_host", "spsp_records_windows_host", "spsp_windows_expand_host", "spsp_windows_segments_host", "spsp_segments_csv_host",
             "spsp_mosaic_csv_host", "spsp_windows_word_check_host", "spsp_records_windows_device", "spsp_windows_stage_ms", "spsp_classify_files_windows",
             "spsp_taxonomy_files_windows")


# ---------------------------------------------------------------------------------------------------- the model

def model_windows(L, k, W):
    """the windows of one record -> [(begin, end)], and the stretches they own -> [(begin, end)]"""
    S = W - (k - 1)
    n = max(1, -(-(L - k + 1) // S))
    held = [(i * S, min(i * S + W, L)) for i in range(n)]
    owned = [(i * S, (i + 1) * S if i + 1 < n else L) for i in range(n)]
    return held, owned


def model_table(off, k, W):
    """-> (first_win[n_rec + 1], win_off[n_windows + 1])"""
    first, win_off = [0], [0]
    for r in range(len(off) - 1):
        held, _ = model_windows(int(off[r + 1]) - int(off[r]), k, W)
        first.append(first[-1] + len(held))
        for a, z in held:
            win_off.append(win_off[-1] + z - a)
    return first, win_off


def model_expand(bases, off, k, W):
    bases = bytes(bases)
    parts = []
    for r in range(len(off) - 1):
        rec = bases[int(off[r]):int(off[r + 1])]
        parts += [rec[a:z] for a, z in model_windows(len(rec), k, W)[0]]
    return (b"".join(parts),) + model_table(off, k, W)


def model_segments(call, keys, hit_keys, support, off, k, W, n_bins):
    """-> (segments as tuples in SEGMENT_ROW_DTYPE's field order, mosaic as tuples in MOSAIC_ROW_DTYPE's)"""
    none, segs, mosaic, w = n_bins - 1, [], [], 0
    for r in range(len(off) - 1):
        L = int(off[r + 1]) - int(off[r])
        owned = model_windows(L, k, W)[1]
        mine = []
        for i, (a, z) in enumerate(owned):
            c = int(call[w + i])
            sup = int(support[w + i]) if c != none else 0
            if mine and mine[-1]["call"] == c:
                s = mine[-1]
                s["end"] = z; s["windows"] += 1; s["keys"] += int(keys[w + i]); s["hit_keys"] += int(hit_keys[w + i]); s["support"] += sup
            else:
                mine.append({"begin": a, "end": z, "keys": int(keys[w + i]), "hit_keys": int(hit_keys[w + i]), "support": sup, "windows": 1, "call": c})
        per = {}
        for s in mine:
            if s["call"] != none:
                b, n = per.get(s["call"], (0, 0))
                per[s["call"]] = (b + s["end"] - s["begin"], n + s["windows"])
        ranked = sorted(per, key=lambda c: (-per[c][0], c))   # most owned bases first, among equals the lower number
        major, second = (ranked + [None, None])[:2]
        pick = lambda c: (ABSENT, 0, 0) if c is None else (c, per[c][1], per[c][0])
        (mj, mjw, mjb), (sc, scw, scb) = pick(major), pick(second)
        called = sum(s["windows"] for s in mine if s["call"] != none)
        mosaic.append((L, mjb, scb, sum(s["keys"] for s in mine), sum(s["hit_keys"] for s in mine), len(owned), len(mine), called, len(per), mj, mjw, sc, scw))
        segs += [(s["begin"], s["end"], s["keys"], s["hit_keys"], s["support"], r, j, s["windows"], s["call"]) for j, s in enumerate(mine)]
        w += len(owned)
    return segs, mosaic


def rows_of(a):
    return [tuple(int(x) for x in row) for row in a.tolist()]


def seam_lengths(k, W):
    S = W - (k - 1)
    return [0, k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1]


def offsets(lens):
    return np.concatenate([[0], np.cumsum(np.array(lens, dtype=np.uint64))]).astype(np.uint64)


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist()) if n else b""


# ---------------------------------------------------------------------------------------------------- not GPU

def test_abi_holds_the_new_calls_and_the_plan_is_the_headers():
    L = sp.lib()
    for name in NEW_CALLS:
        assert name in sp.ABI_SYMBOLS and hasattr(L, name), name
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    const = lambda name: text.split("constexpr uint32_t " + name + " = ")[1].split(";")[0].split(",")[0]
    assert const("kWnStretchBytes") == "16384" and const("kWnThreads") == "256" and "kWnRecsPerLane = 8" in text
    assert sp.windows_plan() == {"stretch_bases": 16384, "stretch_bases_packed": 4 * 16384, "record_tile": 256 * 8}
    assert sp.SEGMENT_ROW_DTYPE.itemsize == 56 and sp.MOSAIC_ROW_DTYPE.itemsize == 72


@pytest.mark.parametrize("k", [5, 7, 31])
def test_the_rule_on_hand_made_lengths(k):
    """every k-mer start lies in exactly one window, the owned stretches tile [0, L), every window but the last has W bases"""
    for W in (k, k + 1, k + 9, 200):
        S = W - (k - 1)
        for L in seam_lengths(k, W) + [3 * W + 2, 1]:
            held, owned = model_windows(L, k, W)
            assert len(held) == (1 if L <= W else -(-(L - W) // S) + 1), (k, W, L)
            assert all(z - a == W for a, z in held[:-1]) and (L < k or held[-1][1] - held[-1][0] >= k) and held[-1][1] == L
            seen = [0] * max(L - k + 1, 0)
            for a, z in held:
                for p in range(a, z - k + 1):
                    seen[p] += 1
            assert all(c == 1 for c in seen), (k, W, L)
            assert owned[0][0] == 0 and owned[-1][1] == L and all(owned[i][1] == owned[i + 1][0] for i in range(len(owned) - 1))
            assert all(a <= z for a, z in owned) and all(owned[i][0] == held[i][0] for i in range(len(held)))


def test_the_host_rule_and_expansion_equal_the_model():
    for seed in range(1, 6):
        rng = np.random.default_rng(seed)
        k = int(rng.choice([5, 7, 31]))
        W = int(rng.choice([k, k + 1, k + 3, 64, 257]))
        if W < k:
            W = k
        lens = seam_lengths(k, W) + [int(x) for x in rng.integers(0, 4 * W + 3, 30)]
        rng.shuffle(lens)
        off = offsets(lens)
        bases = random_bases(rng, int(off[-1]))
        want = model_expand(bases, off, k, W)
        first, win_off = sp.records_windows(off, k, W)
        assert (first.tolist(), win_off.tolist()) == want[1:], seed
        out, first, win_off = sp.windows_expand(np.frombuffer(bases, np.uint8), off, k, W)
        assert (out.tobytes(), first.tolist(), win_off.tolist()) == want, seed
    assert [x.tolist() for x in sp.records_windows([0], 7, 9)] == [[0], [0]]


def test_the_refusals():
    off = offsets([10, 0, 50])
    for W in (6, 0, 0x80000000):
        with pytest.raises(sp.SpspError, match="width") as e:
            sp.records_windows(off, 7, W)
        assert e.value.code == -1
    with pytest.raises(sp.SpspError, match="windows") as e:   # a fabricated table: 2^40 bases at S = 1
        sp.records_windows(np.array([0, 5, 5 + (1 << 40)], dtype=np.uint64), 7, 7)
    assert "record 1" in str(e.value) and e.value.code != -1
    with pytest.raises(sp.SpspError, match="decrease"):
        sp.records_windows(np.array([4, 2], dtype=np.uint64), 7, 7)
    k, W = 5, 8
    off = offsets([18, 4, 12])
    first = model_table(off, k, W)[0]
    n = first[-1]
    ones = np.ones(n, dtype=np.uint32)
    call = np.zeros(n, dtype=np.uint32)
    call[5] = 3
    with pytest.raises(sp.SpspError, match="record 2"):    # a call >= n_bins
        sp.windows_segments(call, ones, ones, ones, first, off, k, W, 3)
    bad = list(first)
    bad[2] += 1
    with pytest.raises(sp.SpspError, match="record 1"):    # first_win against the rule
        sp.windows_segments(np.zeros(n + 1, dtype=np.uint32), np.ones(n + 1), np.ones(n + 1), np.ones(n + 1), bad[:3] + [bad[3] + 1], off, k, W, 3)
    with pytest.raises(sp.SpspError, match="width"):
        sp.windows_segments(call * 0, ones, ones, ones, first, off, k, 4, 3)
    for what, taxonomy in (("best", True), ("taxon", False), ("depth=3", False), ("depth=0", True), ("depth=33", True), ("nearest", False), ("", True)):
        with pytest.raises(sp.SpspError, match="windows"):
            sp.windows_word_check(what, taxonomy)
    for what, taxonomy in (("best", False), ("taxon", True), ("depth=1", True), ("depth=32", True)):
        sp.windows_word_check(what, taxonomy)


def segments_case(calls_per_record, k=5, W=8, n_bins=4, lens=None):
    """records of as many windows as they have calls (S = 4: L = k + 4 (n - 1) + 1), addends that tell the windows apart"""
    S = W - (k - 1)
    lens = lens or [k + S * (len(c) - 1) + 1 for c in calls_per_record]
    off = offsets(lens)
    first = model_table(off, k, W)[0]
    assert [first[i + 1] - first[i] for i in range(len(lens))] == [len(c) for c in calls_per_record]
    call = np.array([c for cs in calls_per_record for c in cs], dtype=np.uint32)
    n = len(call)
    keys, hit, sup = np.arange(10, 10 + n, dtype=np.uint32), np.arange(1, 1 + n, dtype=np.uint32), np.arange(100, 100 + n, dtype=np.uint32)
    seg, mos = sp.windows_segments(call, keys, hit, sup, first, off, k, W, n_bins)
    want = model_segments(call, keys, hit, sup, off, k, W, n_bins)
    assert (rows_of(seg), rows_of(mos)) == want
    return seg, mos


def test_segments_and_mosaic_on_hand_made_calls():
    none = 3
    seg, mos = segments_case([[1, 1, 1, 1]])                                  # one call throughout
    assert rows_of(seg) == [(0, 18, 46, 10, 406, 0, 0, 4, 1)] and mos["calls"][0] == 1 and mos["second"][0] == ABSENT and mos["major_bases"][0] == 18
    seg, mos = segments_case([[0, 2, 0, 2, 0]])                               # an alternation
    assert len(seg) == 5 and seg["windows"].tolist() == [1] * 5 and mos["segments"][0] == 5 and (mos["major"][0], mos["second"][0]) == (0, 2)
    assert (mos["major_windows"][0], mos["major_bases"][0], mos["second_windows"][0], mos["second_bases"][0]) == (3, 4 + 4 + 6, 2, 8)
    # a run that ends exactly at a record's end: the next record's first window with the same call starts a NEW segment
    seg, mos = segments_case([[0, 1, 1], [1, 1, 2], [1]])
    assert seg["record"].tolist() == [0, 0, 1, 1, 2] and seg["segment"].tolist() == [0, 1, 0, 1, 0] and seg["call"].tolist() == [0, 1, 1, 2, 1]
    assert seg["begin"].tolist() == [0, 4, 0, 8, 0] and seg["end"].tolist() == [4, 14, 8, 14, 6]
    seg, mos = segments_case([[none, none, none], [none]])                    # all "none"
    assert len(seg) == 2 and seg["support"].tolist() == [0, 0] and mos["calls"].tolist() == [0, 0] and mos["called_windows"].tolist() == [0, 0]
    assert mos["major"].tolist() == [ABSENT] * 2 and mos["second"].tolist() == [ABSENT] * 2 and mos["major_bases"].tolist() == [0, 0]
    # a tie for major, in bases, that the lower number wins: call 2 owns [0, 4) and [8, 12), call 1 owns [4, 8) and [12, 16); the
    # last window (6 bases, none) belongs to nobody
    seg, mos = segments_case([[2, 1, 2, 1, none]])
    assert (mos["major"][0], mos["major_bases"][0], mos["second"][0], mos["second_bases"][0], mos["calls"][0]) == (1, 8, 2, 8, 2)
    seg, mos = segments_case([[none, 2, none]])                               # second absent
    assert (mos["major"][0], mos["second"][0], mos["second_windows"][0], mos["second_bases"][0], mos["called_windows"][0]) == (2, ABSENT, 0, 0, 1)
    # records of one window each: empty, shorter than k, exactly W
    seg, mos = segments_case([[0], [none], [1]], lens=[0, 4, 8])
    assert seg["end"].tolist() == [0, 4, 8] and mos["length"].tolist() == [0, 4, 8]


def test_both_csv_texts_to_the_byte():
    seg, mos = segments_case([[0, 1, 1, 3], [3], [1, 1]])
    names, calls = ["chr one", "c2", "c3"], ["refA.sk", "ref B", "refC"]
    assert sp.segments_csv(seg, names, calls, "unmatched") == (
        "record,name,segment,begin,end,windows,call,call_name,keys,hit_keys,support\n"
        "0,chr one,0,0,4,1,0,refA.sk,10,1,100\n"
        "0,chr one,1,4,12,2,1,ref B,23,5,203\n"
        "0,chr one,2,12,18,1,unmatched,unmatched,13,4,0\n"
        "1,c2,0,0,6,1,unmatched,unmatched,14,5,0\n"
        "2,c3,0,0,10,2,1,ref B,31,13,211\n")
    assert sp.mosaic_csv(mos, names, calls, "unmatched", 4) == (
        "record,name,length,windows,segments,called_windows,calls,major,major_name,major_windows,major_bases,f_major,second,second_name,second_windows,"
        "second_bases,keys,hit_keys\n"
        "0,chr one,18,4,3,3,2,1,ref B,2,8,0.4444,0,refA.sk,1,4,46,10\n"
        "1,c2,6,1,1,0,0,,,0,0,0,,,0,0,14,5\n"
        "2,c3,10,2,1,2,1,1,ref B,2,10,1,,,0,0,31,13\n")
    assert sp.segments_csv(seg[:0], names, calls, "unmatched").count("\n") == 1


def test_the_command_line_refuses_before_it_opens_anything(tmp_path):
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    (tmp_path / "bank.txt").write_text("a.sk.gz\n")
    cases = [("-y", "100"), ("-X", "r.fa", "-y", "abc"), ("-X", "r.fa", "-y", "0"), ("-X", "r.fa", "-y", "2147483648"), ("-X", "r.fa", "-y", "100:"),
             ("-X", "r.fa", "-y", "100:taxon"), ("-X", "r.fa", "-y", "100:nearest"), ("-X", "r.fa", "-H", "l.txt", "-y", "100:best"),
             ("-X", "r.fa", "-H", "l.txt", "-y", "100:depth=0"), ("-X", "r.fa", "-y", "100", "-Y", "2"), ("-X", "r.fa", "-y", "100", "-x", "m.fa"),
             ("-X", "r.fa", "-y", "100", "-F", "matched"), ("-X", "r.fa", "-y", "100", "-j", "best"), ("-X", "r.fa", "-y", "100x")]
    for args in cases:
        r = run(*args, "-f", "bank.txt", "-o", "no")
        assert r.returncode == 1 and "-y" in r.stdout and len(r.stdout.strip().splitlines()) == 1, (args, r.stdout)
    r = run("-X", "r.fa", "-y", "100", "-q", "q.txt", "-f", "bank.txt", "-o", "no")   # what -X excludes
    assert r.returncode == 1 and "-X" in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["bank.txt"]
    assert "-y" in run().stdout                             # the usage line


def test_host_functions_under_the_sanitizers():
    """tests/tools/windows_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the
    counting rule, the host expansion, the segment function with its refusals and the two writers (CPU only: nothing is preloaded)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "windows_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "windows_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU: the expansion

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


CODE = np.zeros(256, dtype=np.uint32)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
HALO = 256


def pack(bases):
    """16 bases per dword, the first in bits 31:30; the last word zero-filled"""
    c = CODE[np.frombuffer(bytes(bases), np.uint8)]
    c = np.concatenate([c, np.zeros(-len(c) % 16, dtype=np.uint32)]).reshape(-1, 16)
    return (c << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def unpack(words, n):
    c = (words[:, None] >> (30 - 2 * np.arange(16, dtype=np.uint32))) & 3
    return np.frombuffer(b"ACGT", np.uint8)[c.reshape(-1)[:n]].tobytes()


def check(ctx, bases, lens, k, W, packed, note=None, want=None):
    """one expansion of the bases in HBM against the model, the tail included -> (first_win, win_off)"""
    import torch
    off = offsets(lens)
    assert int(off[-1]) == len(bases)
    src = pack(bases).view(np.uint8) if packed else np.frombuffer(bytes(bases), np.uint8)
    d = torch.from_numpy(np.concatenate([src, np.zeros(HALO, np.uint8)])).cuda()   # (the readable bytes behind, as the ingest leaves them)
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    out, n_out, d_win, first, n_win = ctx.records_windows_device(d.data_ptr(), len(bases), d_off.data_ptr(), len(lens), k, W, packed)
    want = want or model_expand(bases, off, k, W)
    assert (n_out, first.tolist(), n_win) == (len(want[0]), want[1], want[1][-1]), note
    assert ctx.to_host(d_win, n_win + 1, np.uint64).tolist() == want[2], note
    assert out % 16 == 0
    stretch = sp.windows_plan()["stretch_bases_packed" if packed else "stretch_bases"]
    whole = max(1, -(-n_out // stretch)) * 16384            # the buffer is whole stretches of 16 KiB ...
    got = ctx.to_host(out, whole + HALO, np.uint8)          # ... and the bytes a scan may read behind them
    if packed:
        words = got.view(np.uint32)
        assert unpack(words[:-(-n_out // 16)], n_out) == want[0], note
        assert n_out % 16 == 0 or (int(words[n_out // 16]) & ((1 << (32 - 2 * (n_out % 16))) - 1)) == 0, note   # the last word zero-filled
        assert not words[-(-n_out // 16):].any(), note
    else:
        assert got[:n_out].tobytes() == want[0], note
        assert not got[n_out:].any(), note
    return want[1], want[2]


def both(ctx, bases, lens, k, W, note=None):
    want = model_expand(bases, offsets(lens), k, W)
    for packed in (False, True):
        check(ctx, bases, lens, k, W, packed, (note, packed), want)
    return want


def records(seed, lens):
    return random_bases(np.random.default_rng(seed), sum(lens))


@pytest.mark.gpu
def test_every_alignment_difference_of_source_and_output(ctx):
    """window i of a record lies i (k - 1) bases further on in the output than in the source, and so does everything behind it: the
    differences are the multiples of k - 1.  An odd k meets every even residue mod 16; the expansion itself asks nothing of k but
    k <= W, so k = 8 and k = 32 are run as well and meet the odd ones.  A first record of 0 .. 15 bases moves both sides along"""
    for ks in (((31, 100), (7, 40)), ((32, 100), (8, 40))):
        seen = set()
        for k, W in ks:
            for lead in range(16):
                lens = [lead, 5 * W + 3, 40, 17 * W]
                first, win_off = both(ctx, records(lead, lens), lens, k, W, (k, lead))[1:]
                off, S = offsets(lens), W - (k - 1)
                for r in range(len(lens)):
                    seen |= {(win_off[w] - (int(off[r]) + (w - first[r]) * S)) % 16 for w in range(first[r], first[r + 1])}
        assert seen == set(range(0, 16, 1 + k % 2)), ks


@pytest.mark.gpu
def test_windows_that_start_and_end_on_the_seams_of_a_dword_and_of_a_store(ctx):
    k, starts, ends = 7, set(), set()
    for lead in (0, 1, 15):
        for W in (16, 17, 31, 32, 33, 47):
            lens = [lead, 4 * W, 9, 2 * W + 1]
            win_off = both(ctx, records(W, lens), lens, k, W, (lead, W))[2]
            starts |= {x % 16 for x in win_off[:-1]}
            ends |= {(x - 1) % 16 for x in win_off[1:] if x}
    assert {0, 1, 15} <= starts and {0, 1, 15} <= ends      # base 0, 1 and 15 of a dword, byte 0, 1 and 15 of a 16-byte store


@pytest.mark.gpu
def test_several_windows_in_one_dword(ctx):
    """W = k = 5: three windows and more inside one output dword, window ends and record ends inside dwords"""
    lens = [40, 5, 4, 0, 23, 6, 64, 5, 5, 5, 1]
    first, win_off = both(ctx, records(5, lens), lens, 5, 5)[1:]
    assert max(sum(1 for x in win_off[:-1] if 16 * d <= x < 16 * d + 16) for d in range(win_off[-1] // 16)) >= 3
    both(ctx, records(6, lens), lens, 5, 6)
    both(ctx, records(7, lens), lens, 7, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_a_window_that_ends_around_a_stretch_seam(ctx, packed):
    """a window that ends one base before, on, and one base behind a workgroup's stretch, and the same for the second seam"""
    stretch = sp.windows_plan()["stretch_bases_packed" if packed else "stretch_bases"]
    k, W = 31, 1 << 17
    for d in (-1, 0, 1):
        lens = [stretch + d, 100, stretch - 100, 50, 31]   # (the third record's one window ends at 2 stretch + d)
        check(ctx, records(d + 2, lens), lens, k, W, packed, d)
    W = 1000                                                # and windows of a record that cross the seams wherever they fall
    lens = [17, 2 * stretch + 3]
    check(ctx, records(9, lens), lens, k, W, packed)


@pytest.mark.gpu
def test_record_counts_around_the_counting_tile(ctx):
    tile = sp.windows_plan()["record_tile"]
    rng = random.Random(3)
    for n in (tile - 1, tile, tile + 1, 2 * tile + 1):
        lens = [rng.choice([0, 3, 31, 32, 40, 70]) for _ in range(n)]
        both(ctx, records(n, lens), lens, 31, 33, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n_rec", [4095 * 2048, 4096 * 2048 + 1, 2 * 4096 * 2048 + 5])
def test_records_behind_the_item_scans_rounds(ctx, n_rec):
    """the record tiles' sums (2 048 records a tile) are scanned by one workgroup, 4 096 tiles a round, the rounds in front carried in
    LDS: a carry dropped or doubled shifts first_win and the output offsets of every record behind record 4 096 x 2 048.  Empty
    records, one window each, but a few of two windows and more on both sides of the rounds' seams; their counts are the host rule's"""
    import torch
    k, W, R = 31, 64, 4096 * 2048
    at = sorted({r for r in (5, R - 1, R, 2 * R - 1, 2 * R, n_rec - 1) if r < n_rec})
    lens = [65 + 70 * i for i in range(len(at))]
    few_first, few_off = sp.records_windows(offsets(lens), k, W)
    few = np.diff(few_first.astype(np.int64))
    assert (few >= 2).all()
    L = np.zeros(n_rec, dtype=np.int64)
    L[at] = lens
    n_win = np.ones(n_rec, dtype=np.int64)
    n_win[at] = few
    off = np.concatenate(([0], np.cumsum(L))).astype(np.uint64)
    d = torch.from_numpy(np.concatenate([np.frombuffer(random_bases(np.random.default_rng(n_rec), int(off[-1])), np.uint8), np.zeros(HALO, np.uint8)])).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    torch.cuda.synchronize()
    out, n_out, d_win, first, n_windows = ctx.records_windows_device(d.data_ptr(), int(off[-1]), d_off.data_ptr(), n_rec, k, W)
    want_first = np.concatenate(([0], np.cumsum(n_win)))
    assert n_windows == int(want_first[-1]) and np.array_equal(first, want_first)
    assert n_out == int((L + (n_win - 1) * (k - 1)).sum()) == int(few_off[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_one_record_of_many_stretches_among_one_window_records(ctx, packed):
    stretch = sp.windows_plan()["stretch_bases_packed" if packed else "stretch_bases"]
    k = 31
    lens = [k] * 5 + [3 * stretch + 1] + [k] * 7
    check(ctx, records(4, lens), lens, k, 1000, packed)


@pytest.mark.gpu
def test_empty_records_and_records_shorter_than_k(ctx):
    k, W = 31, 64
    for lens in ([0], [0, 0, 0], [5], [0, 100, 0], [0, 0, 30, 100, 200, 0, 7, 0, 0], [30, 30, 0, 64, 65, 1, 0], [200, 0], []):
        both(ctx, records(len(lens), lens), lens, k, W, lens)
    both(ctx, b"", [0, 0], 5, 5)


@pytest.mark.gpu
def test_two_calls_on_one_context_and_the_refusals(ctx):
    big, small = [50000, 31, 0, 700], [40, 3]
    both(ctx, records(1, big), big, 31, 500)
    both(ctx, records(2, small), small, 7, 9)              # a smaller call behind a larger one: nothing of the first shows
    both(ctx, records(1, big), big, 31, 500)
    import torch
    d = torch.zeros(1024, dtype=torch.uint8).cuda()
    d_off = torch.from_numpy(np.array([0, 600, 500], dtype=np.int64)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(sp.SpspError, match="width"):
        ctx.records_windows_device(d.data_ptr(), 500, d_off.data_ptr(), 1, 31, 30)
    with pytest.raises(sp.SpspError, match="offsets"):     # offsets that leave the bases, and offsets that decrease
        ctx.records_windows_device(d.data_ptr(), 500, d_off.data_ptr(), 1, 31, 40)
    with pytest.raises(sp.SpspError, match="offsets"):
        ctx.records_windows_device(d.data_ptr(), 1000, d_off.data_ptr(), 2, 31, 40)
    both(ctx, records(2, small), small, 7, 9)
    ctx.timing_enable(True)
    both(ctx, records(2, small), small, 7, 9)
    ms = ctx.windows_stage_ms()
    ctx.timing_enable(False)
    assert sorted(ms) == ["copy", "count", "offsets"] and all(v >= 0 for v in ms.values()) and ms["copy"] > 0
    assert ctx.windows_stage_ms() == {"count": 0.0, "offsets": 0.0, "copy": 0.0}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_a_seeded_sweep(ctx, seed):
    rng = random.Random(seed)
    for _ in range(4):
        k = rng.choice([5, 7, 31])
        W = rng.choice([k, k + 1, k + rng.randrange(2, 40), 150, 1000])
        lens = [rng.choice([0, rng.randrange(k), rng.randrange(3 * W + 2), rng.randrange(40000)]) for _ in range(rng.randrange(1, 60))]
        if W - (k - 1) < 8:                                 # (a step of a few bases: many windows)
            lens = [min(x, 3000) for x in lens]
        both(ctx, records(seed, lens), lens, k, W, (seed, k, W))


# ---------------------------------------------------------------------------------------------------- GPU: end to end

K, M = 31, 11


def fasta(recs):
    return b"".join(b">" + name + b"\n" + (seq + b"\n" if seq else b"") for name, seq in recs)


def windows_text(recs, k, W):
    """T': the text whose records are the windows of T's records"""
    out = []
    for name, seq in recs:
        out += [(name + b".%d" % i, seq[a:z]) for i, (a, z) in enumerate(model_windows(len(seq), k, W)[0])]
    return fasta(out)


@pytest.fixture(scope="module")
def bank(ctx, tmp_path_factory):
    """test_classify's file_case: three random 3 kbp references and a mutated copy of each, sketched at rate 1"""
    import test_classify as tc
    import test_prevalence as tp
    root = tmp_path_factory.mktemp("windows_bank")
    refs, _ = tc.file_case()
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", K, M, 1.0)[0] for i, g in enumerate(refs)]
    return refs, tp.write_files(root, payloads)


def text_case(refs, W, seed):
    """records of the seam lengths and one of about 40 windows: slices of the references, joined slices of two of them, and
    sequences of no reference -- so that some windows are called and some are not"""
    rng = np.random.default_rng(seed)
    S = W - (K - 1)
    recs = []
    for i, L in enumerate(seam_lengths(K, W) + [K + 39 * S + 2]):
        a, b = refs[i % 3] * 8, refs[(i + 1) % 3] * 8       # (tiled: the longest record is longer than a reference)
        h = L // 2
        seq = [a[100:100 + L], a[7:7 + h] + b[500:500 + L - h], random_bases(rng, L), a[:h] + random_bases(rng, L - h)][i % 4]
        assert len(seq) == L
        recs.append((b"rec%d" % i, seq))
    return recs


def model_of_rows(rows, support, call, n_bins, recs, W):
    off = offsets([len(seq) for _, seq in recs])
    return model_segments(call, rows["keys"], rows["hit_keys"], support, off, K, W, n_bins)


@pytest.mark.gpu
@pytest.mark.parametrize("W", [K, K + 1, 300])
def test_classify_files_over_windows_is_classify_files_over_the_windows_text(ctx, bank, tmp_path, W):
    refs, paths = bank
    recs = text_case(refs, W, W)
    (tmp_path / "t.fa").write_bytes(fasta(recs))
    (tmp_path / "w.fa").write_bytes(windows_text(recs, K, W))
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    top, min_keys, num, den = 2, 1 if W == K else 2, 1, 2
    want = ctx.classify_files(paths, str(tmp_path / "w.fa"), str(tmp_path / "plain"), top, min_keys, num, den)
    rows, hits = ctx.classify_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "win"), top, min_keys, num, den, window=W)
    assert rows.dtype == want[0].dtype and rows.tolist() == want[0].tolist() and hits.tolist() == want[1].tolist()
    assert (rows["listed"] > 0).any() and (rows["listed"] == 0).any()   # windows that pass -V and -I, and windows that fail them
    first = model_table(offsets([len(s) for _, s in recs]), K, W)[0]
    assert ctx.last_windows["first_win"].tolist() == first and len(rows) == first[-1]
    call, n_bins = sp.split_bins_classify("best", rows, hits, len(paths))
    support = np.where(rows["listed"] > 0, hits["shared"][:, 0], 0)
    segs, mosaic = model_of_rows(rows, support, call, n_bins, recs, W)
    assert rows_of(ctx.last_windows["segments"]) == segs and rows_of(ctx.last_windows["mosaic"]) == mosaic
    import test_prevalence as tp
    names = [n.decode() for n, _ in recs]
    seg_text = sp.segments_csv(ctx.last_windows["segments"], names, paths, "unmatched")
    mos_text = sp.mosaic_csv(ctx.last_windows["mosaic"], names, paths, "unmatched")
    assert tp.gunzip(tmp_path / "win_segments.csv.gz").decode() == seg_text and tp.gunzip(tmp_path / "win_mosaic.csv.gz").decode() == mos_text
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("win_")) == ["win_mosaic.csv.gz", "win_segments.csv.gz"]
    # the command line (which lists one match per window: the segments name the first alone) writes the same two files
    r = subprocess.run([EXE, "-X", "t.fa", "-y", str(W), "-f", "bank.txt", "-o", "cli", "-I", "0.5"] + (["-V", "2"] if min_keys == 2 else []), cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "%d record(s) in %d window(s)" % (len(recs), first[-1]) in r.stdout, r.stdout
    for suf in ("_segments.csv.gz", "_mosaic.csv.gz"):
        assert tp.gunzip(tmp_path / ("cli" + suf)) == tp.gunzip(tmp_path / ("win" + suf))
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("cli_")) == ["cli_mosaic.csv.gz", "cli_segments.csv.gz"]
    # a refused word or width: before any file is read (the width against k: once the sketches' headers are), nothing written
    with pytest.raises(sp.SpspError, match="windows"):
        ctx.classify_files(["no such sketch.gz"] * 3, str(tmp_path / "none.fa"), str(tmp_path / "no"), window=W, window_call="taxon")
    with pytest.raises(sp.SpspError, match="width"):
        ctx.classify_files(["no such sketch.gz"] * 3, str(tmp_path / "none.fa"), str(tmp_path / "no"), window=1 << 31)
    with pytest.raises(sp.SpspError, match="width"):
        ctx.classify_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "no"), window=K - 1)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
@pytest.mark.parametrize("word", ["taxon", "depth=1"])
def test_taxonomy_files_over_windows(ctx, bank, tmp_path, word):
    import test_prevalence as tp
    import test_taxonomy as tt
    refs, paths = bank
    W = 300
    recs = text_case(refs, W, 5)
    tree = tt.Tree(tt.file_lineages())
    (tmp_path / "t.fa").write_bytes(fasta(recs))
    (tmp_path / "w.fa").write_bytes(windows_text(recs, K, W))
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    (tmp_path / "lin.txt").write_text(tree.text)
    lin = sp.taxonomy_lineages(tree.text, len(paths))
    want = ctx.taxonomy_files(paths, str(tmp_path / "w.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "plain"), 2, 1, 2)
    rows = ctx.taxonomy_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "win"), 2, 1, 2, window=W, window_call=word)
    assert rows.tolist() == want.tolist() and (rows["node"] != sp.TAXONOMY_NONE).any() and (rows["node"] == sp.TAXONOMY_NONE).any()
    call, n_bins = sp.split_bins_taxonomy(word, rows, lin["parent"], lin["depth"])
    support = np.where(rows["node"] != sp.TAXONOMY_NONE, rows["clade"], 0)
    segs, mosaic = model_of_rows(rows, support, call, n_bins, recs, W)
    assert rows_of(ctx.last_windows["segments"]) == segs and rows_of(ctx.last_windows["mosaic"]) == mosaic
    names = [n.decode() for n, _ in recs]
    assert tp.gunzip(tmp_path / "win_segments.csv.gz").decode() == sp.segments_csv(ctx.last_windows["segments"], names, lin["names"], "unclassified")
    assert tp.gunzip(tmp_path / "win_mosaic.csv.gz").decode() == sp.mosaic_csv(ctx.last_windows["mosaic"], names, lin["names"], "unclassified")
    r = subprocess.run([EXE, "-X", "t.fa", "-H", "lin.txt", "-y", "%d:%s" % (W, word), "-V", "2", "-I", "0.5", "-f", "bank.txt", "-o", "cli"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout
    for suf in ("_segments.csv.gz", "_mosaic.csv.gz"):
        assert tp.gunzip(tmp_path / ("cli" + suf)) == tp.gunzip(tmp_path / ("win" + suf))
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("cli_")) == ["cli_mosaic.csv.gz", "cli_segments.csv.gz"]


@pytest.fixture(scope="module")
def mosaic_case(ctx, tmp_path_factory):
    """two synthetic 20 kbp genomes, sketched as two references, and one record that is the first genome followed by the second"""
    import test_prevalence as tp
    root = tmp_path_factory.mktemp("windows_mosaic")
    rng = np.random.default_rng(19)
    genomes = [random_bases(rng, 20000) for _ in range(2)]
    paths = tp.write_files(root, [ctx.sketch_text(b">g%d\n" % i + g + b"\n", K, M, 1.0)[0] for i, g in enumerate(genomes)])
    (root / "chimera.fa").write_bytes(b">chimera of two\n" + genomes[0] + b"\n" + genomes[1] + b"\n")
    return root, paths


@pytest.mark.gpu
def test_a_chimera_of_two_genomes_is_two_segments(ctx, mosaic_case):
    root, paths = mosaic_case
    W, junction = 1000, 20000
    rows, hits = ctx.classify_files(paths, str(root / "chimera.fa"), str(root / "m"), window=W)
    seg, mos = ctx.last_windows["segments"], ctx.last_windows["mosaic"]
    assert seg["call"].tolist() == [0, 1] and seg["begin"][0] == 0 and seg["end"][1] == 40000 and seg["end"][0] == seg["begin"][1]
    assert abs(int(seg["end"][0]) - junction) <= W          # the boundary lies within one window of the junction
    assert (mos["calls"][0], mos["segments"][0], mos["length"][0], mos["windows"][0]) == (2, 2, 40000, len(rows))
    assert {int(mos["major"][0]), int(mos["second"][0])} == {0, 1} and int(mos["major_bases"][0]) + int(mos["second_bases"][0]) == 40000


@pytest.mark.gpu
def test_one_record_across_the_batch_seam_of_65535_windows(ctx, bank, tmp_path):
    """65 535 S + W + 1 bases at S = 3: 65 537 windows, so the record's windows fill one batch and begin the next"""
    refs, paths = bank
    W = K + 2
    S = W - (K - 1)
    L = 65535 * S + W + 1
    rng = np.random.default_rng(23)
    seq = b"".join([refs[0], random_bases(rng, 4000), refs[1]] * (L // 10000 + 1))[:L]
    recs = [(b"short", refs[2][:W]), (b"long", seq), (b"tail", refs[1][:W])]
    (tmp_path / "t.fa").write_bytes(fasta(recs))
    (tmp_path / "w.fa").write_bytes(windows_text(recs, K, W))
    want = ctx.classify_files(paths, str(tmp_path / "w.fa"), str(tmp_path / "plain"))
    rows, hits = ctx.classify_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "win"), window=W)
    assert ctx.last_windows["first_win"].tolist() == [0, 1, 65538, 65539] and len(rows) == 65539
    assert np.array_equal(rows, want[0]) and np.array_equal(hits, want[1])
    assert rows["listed"][65534:65538].tolist() == want[0]["listed"][65534:65538].tolist() and (rows["listed"] > 0).any() and (rows["listed"] == 0).any()
    call, n_bins = sp.split_bins_classify("best", rows, hits, len(paths))
    segs, mosaic = model_of_rows(rows, np.where(rows["listed"] > 0, hits["shared"][:, 0], 0), call, n_bins, recs, W)
    assert rows_of(ctx.last_windows["segments"]) == segs and rows_of(ctx.last_windows["mosaic"]) == mosaic
