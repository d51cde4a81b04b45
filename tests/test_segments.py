"""Segments as sequence: stray windows smoothed and chosen segments written out as FASTA (spsp_windows_smooth_host,
spsp_segments_word_check_host, spsp_segments_select_host, spsp_segments_fasta_host, spsp_segments_plan_host,
spsp_segments_write_device, spsp_segments_stage_ms, spsp_classify_files_segments, spsp_taxonomy_files_segments;
bin/comparator -X <records> -y <W> -Q <q> -Z <what>[:<min>] [-u]).

The rule (include/spsp.h, "segments as sequence"), as the models below have it, written from the rule and not from the C.  A run of
a record's calls is stray when it has at most q windows, is neither the record's first nor its last run, and its two neighbours carry
one call and have more than q windows each; its windows take that call and support 0.  A selected segment of n >= max(1, min_bases)
bases is one FASTA record: '>' name ':' begin + 1 '-' end ' ' call_name, then the bases 80 a line, n + ceil(n / 80) bytes.  The device
writer is held against that text in both forms the ingest writes -- against spsp_segments_fasta_host wherever the headers are the
rule's, against the model alone where a case needs headers of a chosen length -- and the bytes behind the text up to the end of its
last 16 KiB stretch are zero.  Every comparison is exact."""
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
LINE, STRETCH = 80, 16384
NEW_CALLS = ("spsp_segments_plan_host", "spsp_windows_smooth_host", "spsp_segments_word_check_host", "spsp_segments_select_host", "spsp_segments_fasta_host",
             "spsp_segments_write_device", "spsp_segments_stage_ms", "spsp_classify_files_segments", "spsp_taxonomy_files_segments")


# ---------------------------------------------------------------------------------------------------- the models

def model_runs(calls):
    """one record's calls -> [(start, length, call)]"""
    runs = []
    for i, c in enumerate(calls):
        if runs and runs[-1][2] == c:
            runs[-1][1] += 1
        else:
            runs.append([i, 1, c])
    return runs


def model_smooth(call, support, first, q):
    """-> (call, support, n_changed); every stray run is decided on the unsmoothed runs"""
    call, support, changed = [int(c) for c in call], [int(s) for s in support], 0
    out_c, out_s = list(call), list(support)
    for r in range(len(first) - 1):
        w0 = int(first[r])
        runs = model_runs(call[w0:int(first[r + 1])])
        for j in range(1, len(runs) - 1):
            (_, ln, _), (_, ll, cl), (_, lr, cr) = runs[j], runs[j - 1], runs[j + 1]
            if q and ln <= q and cl == cr and ll > q and lr > q:
                for w in range(w0 + runs[j][0], w0 + runs[j][0] + ln):
                    out_c[w], out_s[w] = cl, 0
                changed += ln
    return out_c, out_s, changed


def model_select(segs, mosaic, n_bins, what, min_bases=1):
    none, keep = n_bins - 1, []
    for g in segs:
        call, major = int(g["call"]), int(mosaic[int(g["record"])]["major"])
        word, _, b = what.partition("=")
        k = {"all": True, "called": call != none, "none": call == none, "call": b != "" and call == int(b or 0), "not": b != "" and call != int(b or 0),
             "major": major != ABSENT and call == major, "minor": major != ABSENT and call != none and call != major}[word]
        keep.append(1 if k and int(g["end"]) - int(g["begin"]) >= max(1, min_bases) else 0)
    return keep


def model_body(seq):
    return b"".join(seq[i:i + LINE] + b"\n" for i in range(0, len(seq), LINE))


def model_header(name, begin, end, call_name):
    return b">" + name.encode() + b":%d-%d " % (begin + 1, end) + call_name.encode() + b"\n"


def model_fasta(bases, off, segs, names, call_names, last_name, keep=None):
    bases, out = bytes(bases).upper(), []
    for i, g in enumerate(segs):
        b, e, r, c = int(g["begin"]), int(g["end"]), int(g["record"]), int(g["call"])
        if (keep is not None and not keep[i]) or e == b:
            continue
        out.append(model_header(names[r], b, e, last_name if c == len(call_names) else call_names[c]) + model_body(bases[int(off[r]) + b:int(off[r]) + e]))
    return b"".join(out)


def offsets(lens):
    return np.concatenate([[0], np.cumsum(np.array(lens, dtype=np.uint64))]).astype(np.uint64)


def random_bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tolist()) if n else b""


def seg_rows(rows):
    """[(record, segment, begin, end, call)] -> SEGMENT_ROW_DTYPE"""
    a = np.zeros(len(rows), dtype=sp.SEGMENT_ROW_DTYPE)
    for i, (r, s, b, e, c) in enumerate(rows):
        a[i]["record"], a[i]["segment"], a[i]["begin"], a[i]["end"], a[i]["call"], a[i]["windows"] = r, s, b, e, c, 1
    return a


# ---------------------------------------------------------------------------------------------------- not GPU

def test_abi_holds_the_new_calls_and_the_plan_is_the_headers():
    L = sp.lib()
    for name in NEW_CALLS:
        assert name in sp.ABI_SYMBOLS and hasattr(L, name), name
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    const = lambda name: text.split("constexpr uint32_t " + name + " = ")[1].split(";")[0]
    assert const("kSgLine") == "80" and const("kSgStretch") == "16384"
    assert "#define SPSP_SEGMENTS_LINE 80u" in open(os.path.join(ROOT, "include", "spsp.h")).read()
    assert sp.segments_plan() == {"line_bases": LINE, "stretch_bytes": STRETCH} == sp.Context.segments_plan()


def smooth_case(calls_per_record, q, n_bins=4):
    first = np.concatenate([[0], np.cumsum([len(c) for c in calls_per_record])]).astype(np.uint32)
    call = np.array([c for cs in calls_per_record for c in cs], dtype=np.uint32)
    support = np.arange(100, 100 + len(call), dtype=np.uint32)
    got = sp.windows_smooth(call, support, first, n_bins, q)
    want = model_smooth(call, support, first, q)
    assert (got[0].tolist(), got[1].tolist(), got[2]) == want, (calls_per_record, q)
    assert [s for s, a, b in zip(got[1].tolist(), got[0].tolist(), call.tolist()) if a != b] == [0] * got[2]   # support is zeroed exactly on the changed windows
    assert all(s == t for s, t, a, b in zip(got[1].tolist(), support.tolist(), got[0].tolist(), call.tolist()) if a == b)
    return got[0].tolist(), got[2]


def test_smoothing_on_hand_made_calls():
    none = 3
    base = [[0, 0, 0, 1, 0, 0, 0]]
    assert smooth_case(base, 0) == (base[0], 0)                                     # q = 0 is the identity
    assert smooth_case(base, 1) == ([0] * 7, 1)
    assert smooth_case([[0, 0, 0, 1, 1, 0, 0, 0]], 2) == ([0] * 8, 2)               # a stray run of exactly q windows ...
    assert smooth_case([[0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0]], 2)[1] == 0              # ... and one of q + 1
    assert smooth_case([[0, 0, 1, 1, 0, 0, 0]], 2)[1] == 0                          # a flank of exactly q windows ...
    assert smooth_case([[0, 0, 0, 1, 1, 0, 0]], 2)[1] == 0
    assert smooth_case([[0, 0, 0, 1, 1, 0, 0, 0]], 2)[1] == 2                       # ... and flanks of q + 1
    assert smooth_case([[1, 0, 0, 0, 0]], 1)[1] == 0 and smooth_case([[0, 0, 0, 0, 1]], 1)[1] == 0   # at the record's first run and at its last
    assert smooth_case([[0, 0, 1, 2, 2]], 1)[1] == 0                                # neighbours that differ from each other
    assert smooth_case([[0, 0, none, 0, 0]], 1) == ([0] * 5, 1)                     # a stray "none" between two called runs
    assert smooth_case([[none, none, 1, none, none]], 1) == ([none] * 5, 1)         # a called stray between two none runs
    assert smooth_case([[0, 0, 1, 0, 0, 0, 2, 0, 0]], 1) == ([0] * 9, 2)            # two strays separated by one long run both change
    assert smooth_case([[0, 0, 1, 0, 1, 1]], 1) == ([0, 0, 1, 0, 1, 1], 0)          # two short runs side by side: each has a short flank, both stay
    assert smooth_case([[0, 0, 1], [0, 0, 0]], 1)[1] == 0                           # a run that ends with its record borrows no flank from the next
    assert smooth_case([[0, 0, 0], [1, 0, 0]], 1)[1] == 0
    assert smooth_case([[0], [1], [0], [none]], 5)[1] == 0                          # records of one window
    assert smooth_case([[], [0, 0, 1, 0, 0], []], 1)[1] == 1                        # (a record without a window on either side)
    assert smooth_case(base, 0x7FFFFFFF)[1] == 0                                    # no flank is longer than the largest q
    assert sp.windows_smooth([], [], [0], 4, 3)[2] == 0


def test_smoothing_refusals():
    ones = np.ones(4, dtype=np.uint32)
    with pytest.raises(sp.SpspError, match="record 1") as e:                        # a call >= n_bins
        sp.windows_smooth([0, 0, 4, 0], ones, [0, 2, 4], 4, 1)
    assert e.value.code == -1
    with pytest.raises(sp.SpspError, match="record 1"):                             # a first_win that decreases
        sp.windows_smooth([0, 0, 0, 0], ones, [0, 3, 2], 4, 1)
    with pytest.raises(sp.SpspError, match="smoothing"):
        sp.windows_smooth([0, 0, 0, 0], ones, [0, 4], 4, 0x80000000)


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_smoothing_a_seeded_sweep(seed):
    rng = random.Random(seed)
    recs = []
    for _ in range(160):
        c, calls = rng.randrange(4), []
        for _ in range(rng.choice([0, 1, 2, rng.randrange(200)])):
            if rng.random() < rng.choice([0.05, 0.3]):
                c = rng.randrange(4)
            calls.append(c)
        recs.append(calls)
    assert sum(len(c) for c in recs) > 2000                 # a few thousand windows
    changed = [smooth_case(recs, q)[1] for q in (1, 2, 3, 7)]
    assert all(changed)


SELECT_SEGS = [(0, 0, 0, 10, 1), (0, 1, 10, 14, 3), (0, 2, 14, 20, 0), (0, 3, 20, 50, 1), (1, 0, 0, 7, 3), (2, 0, 0, 0, 3), (3, 0, 0, 9, 2)]


def select_mosaic():
    mos = np.zeros(4, dtype=sp.MOSAIC_ROW_DTYPE)
    mos["major"], mos["second"] = [1, ABSENT, ABSENT, 2], [0, ABSENT, ABSENT, ABSENT]
    return mos


def test_selection_of_every_word_on_hand_made_rows():
    segs, mos = seg_rows(SELECT_SEGS), select_mosaic()
    want = {"all": [1, 1, 1, 1, 1, 0, 1], "called": [1, 0, 1, 1, 0, 0, 1], "none": [0, 1, 0, 0, 1, 0, 0], "call=1": [1, 0, 0, 1, 0, 0, 0], "call=0": [0, 0, 1, 0, 0, 0, 0],
            "not=1": [0, 1, 1, 0, 1, 0, 1],                  # the uncalled are kept
            "major": [1, 0, 0, 1, 0, 0, 1], "minor": [0, 0, 1, 0, 0, 0, 0]}   # record 1 has no major: nothing of it under either word
    for what, flags in want.items():
        keep, n_kept, n_bases = sp.segments_select(segs, mos, 4, what)
        assert keep.tolist() == flags == model_select(segs, mos, 4, what), what
        assert (n_kept, n_bases) == (sum(flags), sum(e - b for (_, _, b, e, _), f in zip(SELECT_SEGS, flags) if f)), what
    assert sp.segments_select(segs, mos, 4, "all")[0][5] == 0        # an empty record's empty segment is never written
    assert sp.segments_select(segs, mos, 4, "all", 0)[0].tolist() == want["all"]
    for least, flags in ((9, [1, 0, 0, 1, 0, 0, 1]), (10, [1, 0, 0, 1, 0, 0, 0]), (11, [0, 0, 0, 1, 0, 0, 0])):   # len - 1, len, len + 1 of the 10-base segment
        assert sp.segments_select(segs, mos, 4, "all", least)[0].tolist() == flags == model_select(segs, mos, 4, "all", least)
    keep, n_kept, n_bases = sp.segments_select(segs[:0], mos[:0], 4, "all")
    assert len(keep) == 0 and (n_kept, n_bases) == (0, 0)


def test_selection_refusals():
    segs, mos = seg_rows(SELECT_SEGS), select_mosaic()
    for what in ("", "bogus", "ALL", "call=", "call=x", "call=-1", "not=1x", "major=1", " all", "call=3", "not=3", "call=4294967295"):   # <b> = n_bins - 1 as well
        with pytest.raises(sp.SpspError, match="segments") as e:
            sp.segments_select(segs, mos, 4, what)
        assert e.value.code == -1
        with pytest.raises(sp.SpspError, match="segments"):
            sp.segments_word_check(what, False, 4)
    for what in ("all:", "all:x", "all:1:2", "all:-1", "all:9223372036854775808", "call=1:0x10"):   # a minimum that is no decimal below 2^63
        with pytest.raises(sp.SpspError, match="decimal"):
            sp.segments_word_check(what, False, 4)
    with pytest.raises(sp.SpspError, match="2\\^63"):
        sp.segments_select(segs, mos, 4, "all", 1 << 63)
    for what in ("all", "called", "none", "call=2", "not=0", "major", "minor", "all:0", "minor:9223372036854775807"):
        sp.segments_word_check(what, False, 4)
    sp.segments_word_check("call=70000", True, 0)           # the bins are not counted yet: <b> is only a number
    with pytest.raises(sp.SpspError, match="node"):
        sp.segments_word_check("call=70000", True, 70001)


def test_the_fasta_text_to_the_byte():
    rng = np.random.default_rng(5)
    lens = [1, 79, 80, 81, 159, 160, 161, 0, 500]
    off = offsets(lens)
    bases = random_bases(rng, int(off[-1]))
    names = ["r%d" % i for i in range(len(lens))]
    names[2] = "chr"                                        # (the names come as the CSV has them: the header line's first word)
    calls = ["refA.sk", "ref B"]
    rows = [(r, 0, 0, L, r % 3) for r, L in enumerate(lens)]
    rows[8:] = [(8, 0, 0, 81, 0), (8, 1, 81, 82, 2), (8, 2, 82, 242, 1), (8, 3, 242, 500, 2)]
    segs = seg_rows(rows)
    text = sp.segments_fasta(bases, off, segs, names, calls, "unmatched")
    assert text == model_fasta(bases, off, segs, names, calls, "unmatched")
    recs = text.split(b">")[1:]
    assert len(recs) == len(rows) - 1                       # the empty record's segment is not written
    for rec, (r, _, b, e, c) in zip(recs, [x for x in rows if x[3] > x[2]]):
        head, _, body = rec.partition(b"\n")
        n = e - b
        assert head == b"%s:%d-%d %s" % (names[r].encode(), b + 1, e, (calls + ["unmatched"])[c].encode())
        assert len(body) == n + -(-n // LINE) and body.endswith(b"\n") and all(len(x) == LINE for x in body.split(b"\n")[:-2]) and body.replace(b"\n", b"") == bases[int(off[r]) + b:int(off[r]) + e]
    assert recs[1].startswith(b"r1:1-79 ref B\n") and b">r8:82-82 unmatched\n" in text
    keep = [0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0]
    assert sp.segments_fasta(bases, off, segs, names, calls, "unmatched", keep) == model_fasta(bases, off, segs, names, calls, "unmatched", keep)
    assert sp.segments_fasta(bases.lower(), off, segs, names, calls, "unmatched") == text   # upper case whatever comes in
    assert sp.segments_fasta(b"", [0], segs[:0], [], calls, "unmatched") == b""
    with pytest.raises(sp.SpspError, match="leaves its record"):
        sp.segments_fasta(bases, off, seg_rows([(0, 0, 0, 2, 0)]), names, calls, "unmatched")


def test_the_command_line_refuses_before_it_opens_anything(tmp_path):
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    (tmp_path / "bank.txt").write_text("a.sk.gz\nb.sk.gz\n")
    cases = [("-Q", ("-X", "r.fa", "-Q", "1")), ("-Z", ("-X", "r.fa", "-Z", "all")), ("-Z", ("-X", "r.fa", "-y", "100", "-Z", "bogus")), ("-Q", ("-X", "r.fa", "-y", "100", "-Q", "x")),
             ("-Q", ("-X", "r.fa", "-y", "100", "-Q", "-1")), ("-Q", ("-X", "r.fa", "-y", "100", "-Q", "2147483648")), ("-Z", ("-X", "r.fa", "-y", "100", "-Z", "all:x")),
             ("-Z", ("-X", "r.fa", "-y", "100", "-Z", "call=2")), ("-Z", ("-X", "r.fa", "-y", "100", "-Z", "not=7:5"))]   # (<b> against the two references of the list)
    for letter, args in cases:
        r = run(*args, "-f", "bank.txt", "-o", "no")
        assert r.returncode == 1 and letter in r.stdout.splitlines()[-1] and len([x for x in r.stdout.strip().splitlines() if x.startswith("-")]) == 1, (args, r.stdout)
    r = run("-X", "r.fa", "-u", "-f", "bank.txt", "-o", "no")   # the old line, to the letter
    assert r.returncode == 1 and r.stdout.strip() == "-u writes the records of -F plain instead of gzipped: it needs -F"
    assert sorted(os.listdir(tmp_path)) == ["bank.txt"]
    usage = run().stdout
    assert "-Q <q>" in usage and "-Z <what>[:<min_bases>]" in usage


def test_host_functions_under_the_sanitizers():
    """tests/tools/segments_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the
    smoothing, the selection, the word check, the text and the plan (CPU only: nothing is preloaded)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "segments_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "segments_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU: the writer

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


CODE = np.zeros(256, dtype=np.uint32)
for _i, _c in enumerate(b"ACTG"):                           # the ingest's codes: (c >> 1) & 3
    CODE[_c] = _i
HALO = 256


def pack(bases):
    """16 bases per dword, the first in bits 31:30; the last word zero-filled"""
    c = CODE[np.frombuffer(bytes(bases), np.uint8)]
    c = np.concatenate([c, np.zeros(-len(c) % 16, dtype=np.uint32)]).reshape(-1, 16)
    return (c << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


class Source:
    """the bases of a case in HBM in both forms, with the readable bytes behind, uploaded once"""

    def __init__(self, bases):
        import torch
        self.bases = bytes(bases)
        self.d = [torch.from_numpy(np.concatenate([np.frombuffer(self.bases, np.uint8), np.zeros(HALO, np.uint8)])).cuda(),
                  torch.from_numpy(np.concatenate([pack(self.bases).view(np.uint8), np.zeros(HALO, np.uint8)])).cuda()]
        torch.cuda.synchronize()


def write_check(ctx, source, segs, want=None, note=None, forms=(False, True)):
    """segs: [(src, len, header bytes)] -> the text; both forms against `want` (the model's where none is given), zeros behind"""
    model = b"".join(h + model_body(source.bases[s:s + n]) for s, n, h in segs)
    want = model if want is None else want
    assert want == model, note
    hdr_off = np.concatenate([[0], np.cumsum([len(h) for _, _, h in segs])]).astype(np.uint64)
    for packed in forms:
        out, n_out = ctx.segments_write_device(source.d[packed].data_ptr(), len(source.bases), [s for s, _, _ in segs], [n for _, n, _ in segs],
                                               b"".join(h for _, _, h in segs), hdr_off, packed)
        assert n_out == len(want) and out % 16 == 0, (note, packed)
        got = ctx.to_host(out, max(1, -(-n_out // STRETCH)) * STRETCH, np.uint8)   # the buffer is whole stretches
        assert got[:n_out].tobytes() == want, (note, packed)
        assert not got[n_out:].any(), (note, packed)
    return want


def rows_check(ctx, source, lens, rows, names, note=None):
    """segments as rows of records: the yardstick is spsp_segments_fasta_host on the same tables"""
    off, segs = offsets(lens), seg_rows(rows)
    calls = ["refA", "ref B"]
    want = sp.segments_fasta(source.bases, off, segs, names, calls, "unmatched")
    table = [(int(off[r]) + b, e - b, model_header(names[r], b, e, (calls + ["unmatched"])[c])) for r, _, b, e, c in rows if e > b]
    return write_check(ctx, source, table, want, note)


@pytest.fixture(scope="module")
def source(ctx):
    return Source(random_bases(np.random.default_rng(11), 70000))


@pytest.mark.gpu
def test_a_newline_on_every_byte_of_a_store(ctx, source):
    """81 and 16 are coprime: the sixteen line ends of 16 x 80 + 7 bases fall on sixteen different bytes of their stores, and a
    header of each length 1 .. 16 moves all of them along"""
    n = 16 * LINE + 7
    for h in range(1, 17):
        header = (b">" + b"abcdefghijklmno")[:h - 1] + b"\n"
        assert len(header) == h
        write_check(ctx, source, [(3, n, header)], note=h)
        assert {(h + LINE + 81 * j) % 16 for j in range(16)} == set(range(16))


@pytest.mark.gpu
def test_segment_starts_at_every_residue_of_the_source(ctx, source):
    """ASCII: every residue mod 16 bytes; packed: every base of a dword and every dword of four (64 residues), with the output's
    alignment fixed (one header length) and moved (the header grows with the start's digits)"""
    for start in range(64):
        write_check(ctx, source, [(start, 333, b">s\n")], note=start)
    lens = [64 + 400, 70]
    for start in range(0, 64, 5):
        rows_check(ctx, source, lens, [(0, 0, start, start + 400, 0), (1, 0, 3, 70, 2)], ["chr1", "x"], start)


@pytest.mark.gpu
def test_segment_lengths_around_a_store_and_a_line(ctx, source):
    lens = [1, 15, 16, 17, 79, 80, 81, 159, 160, 161]
    rows = [(r, 0, 0, L, r % 3) for r, L in enumerate(lens)]
    rows_check(ctx, source, lens, rows, ["r%d" % i for i in range(len(lens))])
    for n in lens:                                          # and each alone, behind headers that put its end on every byte of a store
        for h in (1, 2, 7, 16):
            write_check(ctx, source, [(9, n, b">" * (h - 1) + b"\n")], note=(n, h))
    # a body's last line of one base: the line's newline and the body's last in one store
    for n in (81, 161, 82, 162):
        for h in range(1, 17):
            write_check(ctx, source, [(5, n, b"h" * (h - 1) + b"\n"), (100, 40, b">next\n")], note=(n, h))


@pytest.mark.gpu
def test_several_segments_in_one_store_and_headers_across_stores(ctx, source):
    tiny = [(i * 3, 1, b"\n") for i in range(40)]           # three bytes a segment: five whole segments inside one 16-byte store
    write_check(ctx, source, tiny)
    write_check(ctx, source, [(i, 1, b">n\n") for i in range(50)])   # length 1 with a 2-byte name
    write_check(ctx, source, [(i * 7, 2, b"") for i in range(33)])   # no header at all
    long_header = b">" + b"a header that is longer than two stores" + b"\n"
    for lead in range(16):                                  # a header that straddles a store, wherever it begins
        write_check(ctx, source, [(0, lead + 1, b">\n"), (200, 100, long_header), (50, 17, b">z\n")], note=lead)
    rows_check(ctx, source, [3000], [(0, i, 30 * i, 30 * i + 30, i % 3) for i in range(100)], ["contig_with_a_long_name"])


def bytes_of(n):
    return n + -(-n // LINE)


def fill_to(at):
    """segments whose text is exactly `at` bytes: one long one, then some of two and three bytes"""
    n = 0
    while 2 + bytes_of(n + 1) <= at - 4:
        n += 1
    segs, r = [(7, n, b">\n")], at - 2 - bytes_of(n)
    while r:
        step = 3 if r % 2 else 2
        segs.append((1, 1, b"\n" if step == 3 else b""))
        r -= step
    return segs


@pytest.mark.gpu
def test_headers_and_newlines_around_the_stretch_seam(ctx, source):
    header = b">0123456789abcdefghij\n"
    for at in range(STRETCH - len(header) - 1, STRETCH + 2):   # the header begins at byte `at`: it straddles the seam byte by byte
        table = fill_to(at)
        assert sum(len(h) + bytes_of(n) for _, n, h in table) == at
        write_check(ctx, source, table + [(300, 500, header)], note=at)
    # a body whose line's newline is the last byte of a stretch, and one whose newline is the first byte of the next
    for h, where in ((22, STRETCH - 1), (23, STRETCH)):
        assert where in [h + 81 * j + 80 for j in range(STRETCH // LINE)]
        write_check(ctx, source, [(11, STRETCH, b"x" * (h - 1) + b"\n"), (0, 33, b">t\n")], note=h)
    # the same for a body's LAST newline, and a text that ends one byte in front of the seam, on it and one byte behind it
    for total in (STRETCH - 1, STRETCH, STRETCH + 1):
        h = total - (2 + bytes_of(16100)) - bytes_of(10)
        write_check(ctx, source, [(0, 16100, b">\n"), (40, 10, b"y" * (h - 1) + b"\n")], note=total)
        write_check(ctx, source, [(0, 16100, b">\n"), (40, 10, b"y" * (h - 1) + b"\n"), (9, 100, b">behind\n")], note=total)


@pytest.mark.gpu
def test_one_long_segment_among_one_base_segments_and_more_than_the_lds_holds(ctx, source):
    lens = [5] * 5 + [3 * STRETCH + 100] + [5] * 7
    rows = [(r, 0, 0, 1, 0) if L == 5 else (r, 0, 0, L, 1) for r, L in enumerate(lens)]
    rows_check(ctx, source, lens, rows, ["n%d" % i for i in range(len(lens))])
    rng = random.Random(8)
    write_check(ctx, source, [(rng.randrange(60000), 1 + rng.randrange(3), b"") for _ in range(9000)])   # thousands of segments in a stretch: the tables are read from memory
    write_check(ctx, source, [(rng.randrange(60000), 20, b">q\n") for _ in range(2000)])   # about 630 a stretch, 512 are kept in LDS


@pytest.mark.gpu
def test_no_segment_refusals_and_two_calls_on_one_context(ctx, source):
    assert write_check(ctx, source, []) == b""              # n_seg = 0: an empty text, one stretch of zeros
    big = [(0, 50000, b">big one\n"), (123, 4567, b">second\n")]
    small = [(5, 3, b">s\n")]
    write_check(ctx, source, big)
    write_check(ctx, source, small)                         # a smaller call behind a larger one: nothing of the first shows
    write_check(ctx, source, big)
    n = len(source.bases)
    for src, ln, word in ((n - 9, 10, "leaves"), (n, 1, "leaves"), (0, n + 1, "leaves"), (1 << 63, 1 << 63, "leaves"), (5, 0, "no bases")):
        with pytest.raises(sp.SpspError, match=word) as e:   # refused with no launch: the buffer still holds the last text
            ctx.segments_write_device(source.d[0].data_ptr(), n, [0, src], [10, ln], b">a\n>b\n", [0, 3, 6])
        assert e.value.code == -1
    with pytest.raises(sp.SpspError, match="decrease"):
        ctx.segments_write_device(source.d[0].data_ptr(), n, [0, 4], [10, 10], b">a\n>b\n", [0, 5, 3])
    write_check(ctx, source, [(n - 10, 10, b">the last bases\n"), (n - 1, 1, b">e\n")])
    ctx.timing_enable(True)
    write_check(ctx, source, big, forms=(False,))
    ms = ctx.segments_stage_ms()
    ctx.timing_enable(False)
    assert sorted(ms) == ["write"] and ms["write"] > 0 and ctx.segments_stage_ms() == {"write": 0.0}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_writer_a_seeded_sweep(ctx, source, seed):
    rng = random.Random(seed)
    for _ in range(4):
        lens = [rng.choice([0, rng.randrange(20), rng.randrange(400), rng.randrange(30000)]) for _ in range(rng.randrange(1, 12))]
        while sum(lens) > len(source.bases):
            lens.pop()
        rows = []
        for r, L in enumerate(lens):
            cuts = sorted({0, L} | {rng.randrange(L + 1) for _ in range(rng.randrange(6))})
            rows += [(r, j, a, z, rng.randrange(3)) for j, (a, z) in enumerate(zip(cuts, cuts[1:])) if rng.random() < 0.8]
        rows_check(ctx, source, lens, rows, ["rec%d" % (r * 37 ** (r % 4)) for r in range(len(lens))], (seed, lens))


# ---------------------------------------------------------------------------------------------------- GPU: end to end

K, M = 31, 11


def fasta(recs):
    return b"".join(b">" + name + b"\n" + (seq + b"\n" if seq else b"") for name, seq in recs)


def gunzip(path):
    return gzip.decompress(open(path, "rb").read())


def model_windows(L, k, W):
    S = W - (k - 1)
    n = max(1, -(-(L - k + 1) // S))
    return [(i * S, min(i * S + W, L)) for i in range(n)], [(i * S, (i + 1) * S if i + 1 < n else L) for i in range(n)]


def seam_lengths(k, W):
    S = W - (k - 1)
    return [0, k - 1, k, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1]


@pytest.fixture(scope="module")
def bank(ctx, tmp_path_factory):
    """test_classify's file_case: three random 3 kbp references and a mutated copy of each, sketched at rate 1"""
    import test_classify as tc
    import test_prevalence as tp
    root = tmp_path_factory.mktemp("segments_bank")
    refs, _ = tc.file_case()
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", K, M, 1.0)[0] for i, g in enumerate(refs)]
    return refs, tp.write_files(root, payloads)


def text_case(refs, W, seed):
    """test_windows' records: the seam lengths and one of about 40 windows; slices of the references, joined slices of two of them, and
    sequences of no reference -- so that some windows are called and some are not"""
    rng = np.random.default_rng(seed)
    S = W - (K - 1)
    recs = []
    for i, L in enumerate(seam_lengths(K, W) + [K + 39 * S + 2]):
        a, b = refs[i % 3] * 8, refs[(i + 1) % 3] * 8
        h = L // 2
        seq = [a[100:100 + L], a[7:7 + h] + b[500:500 + L - h], random_bases(rng, L), a[:h] + random_bases(rng, L - h)][i % 4]
        recs.append((b"rec%d" % i, seq))
    return recs


def file_is_the_text(ctx, path, recs, call_names, last_name, what=None, min_bases=1, plain=False):
    """the written file against spsp_segments_fasta_host of last_windows (and the model); -> the text"""
    lw = ctx.last_windows
    off = offsets([len(s) for _, s in recs])
    bases = b"".join(s for _, s in recs)
    names = [n.decode().split()[0] for n, _ in recs]
    n_bins = len(call_names) + 1
    keep = None if what is None else sp.segments_select(lw["segments"], lw["mosaic"], n_bins, what, min_bases)[0]
    want = sp.segments_fasta(bases, off, lw["segments"], names, call_names, last_name, keep)
    assert want == model_fasta(bases, off, lw["segments"], names, call_names, last_name, keep)
    got = open(path, "rb").read() if plain else gunzip(path)
    assert got == want
    flags = [1] * len(lw["segments"]) if keep is None else keep.tolist()
    written = sum(1 for g, f in zip(lw["segments"], flags) if f and g["end"] > g["begin"])
    assert (lw["written"], lw["bytes_out"]) == (written, len(want))
    return want


@pytest.mark.gpu
def test_all_segments_of_a_run_and_the_smoothed_runs(ctx, bank, tmp_path):
    import test_windows as tw
    refs, paths = bank
    W = 300
    recs = text_case(refs, W, 5)
    (tmp_path / "t.fa").write_bytes(fasta(recs))
    args = (paths, str(tmp_path / "t.fa"))
    rows0, hits0 = ctx.classify_files(*args, str(tmp_path / "plain"), 2, 2, 1, 2, window=W)
    seg0 = ctx.last_windows["segments"]
    assert ctx.last_windows["written"] == 0 and not os.path.exists(tmp_path / "plain_segments.fa.gz")
    rows, hits = ctx.classify_files(*args, str(tmp_path / "all"), 2, 2, 1, 2, window=W, segments="all")
    assert np.array_equal(rows, rows0) and np.array_equal(hits, hits0) and np.array_equal(ctx.last_windows["segments"], seg0) and ctx.last_windows["changed"] == 0
    for suf in ("_segments.csv.gz", "_mosaic.csv.gz"):     # the two CSVs are those of the run without the word, byte for byte
        assert open(tmp_path / ("all" + suf), "rb").read() == open(tmp_path / ("plain" + suf), "rb").read()
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("all_")) == ["all_mosaic.csv.gz", "all_segments.csv.gz", "all_segments.fa.gz"]
    text = file_is_the_text(ctx, tmp_path / "all_segments.fa.gz", recs, paths, "unmatched")
    bodies = {}
    for rec in text.split(b">")[1:]:                        # the concatenated bodies of a record's segments are its cleaned bases
        head, _, body = rec.partition(b"\n")
        bodies.setdefault(head.split(b":")[0], []).append(body.replace(b"\n", b""))
    assert {n: b"".join(p) for n, p in bodies.items()} == {n: s for n, s in recs if s}
    assert len(seg0) > len(recs) + 3 and (seg0["call"] == len(paths)).any() and (seg0["call"] < len(paths)).any()
    # smoothing: segments and mosaic are the model's smoothing of the q = 0 run's calls; the windows' rows stay unsmoothed
    call, n_bins = sp.split_bins_classify("best", rows0, hits0, len(paths))
    support = np.where(rows0["listed"] > 0, hits0["shared"][:, 0], 0)
    first = ctx.last_windows["first_win"]
    off = offsets([len(s) for _, s in recs])
    for q in (1, 2):
        rows, hits = ctx.classify_files(*args, str(tmp_path / ("q%d" % q)), 2, 2, 1, 2, window=W, smooth=q, segments="called", segments_min=200)
        assert np.array_equal(rows, rows0) and np.array_equal(hits, hits0)
        c, s, changed = model_smooth(call, support, first, q)
        segs, mosaic = tw.model_segments(c, rows0["keys"], rows0["hit_keys"], s, off, K, W, n_bins)
        assert tw.rows_of(ctx.last_windows["segments"]) == segs and tw.rows_of(ctx.last_windows["mosaic"]) == mosaic and ctx.last_windows["changed"] == changed
        file_is_the_text(ctx, tmp_path / ("q%d_segments.fa.gz" % q), recs, paths, "unmatched", "called", 200)
    # the command line writes the same bytes, gzipped and plain
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    for extra, name in ((["-u"], "cli_segments.fa"), ([], "cli_segments.fa.gz")):
        r = subprocess.run([EXE, "-X", "t.fa", "-y", str(W), "-Q", "2", "-Z", "called:200", "-f", "bank.txt", "-o", "cli", "-I", "0.5", "-V", "2"] + extra, cwd=tmp_path,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "segments called: %d of %d segment(s) written" % (ctx.last_windows["written"], len(ctx.last_windows["segments"])) in r.stdout, r.stdout
        got = open(tmp_path / name, "rb").read()
        assert (got if extra else gzip.decompress(got)) == gunzip(tmp_path / "q2_segments.fa.gz")
        for suf in ("_segments.csv.gz", "_mosaic.csv.gz"):
            assert gunzip(tmp_path / ("cli" + suf)) == gunzip(tmp_path / ("q2" + suf))
    # a refused word, <b> or smoothing: before any file is read, nothing written
    for kw in ({"segments": "bogus"}, {"segments": "call=3"}, {"segments": "not=4"}, {"segments": "all:5"}, {"smooth": 1 << 31}, {"segments": "all", "segments_min": 1 << 63}):
        with pytest.raises((sp.SpspError, ValueError), match="segments|smooth"):
            ctx.classify_files(["no such sketch.gz"] * 3, str(tmp_path / "none.fa"), str(tmp_path / "no"), window=W, **kw)
    with pytest.raises(ValueError, match="window"):
        ctx.classify_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "no"), segments="all")
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.fixture(scope="module")
def genomes(ctx, tmp_path_factory):
    """two synthetic 20 kbp genomes, sketched as two references"""
    import test_prevalence as tp
    root = tmp_path_factory.mktemp("segments_genomes")
    rng = np.random.default_rng(19)
    g = [random_bases(rng, 20000) for _ in range(2)]
    return root, g, tp.write_files(root, [ctx.sketch_text(b">g%d\n" % i + x + b"\n", K, M, 1.0)[0] for i, x in enumerate(g)])


@pytest.mark.gpu
def test_a_spliced_window_is_absorbed_at_its_length_and_not_below(ctx, genomes):
    root, g, paths = genomes
    W = 1000
    seq = g[0][:10000] + g[1][5000:5000 + W] + g[0][10000:]
    (root / "splice.fa").write_bytes(b">spliced\n" + seq + b"\n")
    ctx.classify_files(paths, str(root / "splice.fa"), str(root / "s0"), window=W)
    seg = ctx.last_windows["segments"]
    assert seg["call"].tolist() == [0, 1, 0]
    n = int(seg["windows"][1])                              # the stray run's windows, read from the q = 0 run
    assert 1 <= n <= 2
    ctx.classify_files(paths, str(root / "splice.fa"), str(root / "s1"), window=W, smooth=n - 1)
    assert len(ctx.last_windows["segments"]) > 1
    ctx.classify_files(paths, str(root / "splice.fa"), str(root / "s2"), window=W, smooth=n, segments="major")
    seg = ctx.last_windows["segments"]
    assert len(seg) == 1 and (seg["begin"][0], seg["end"][0], seg["call"][0], ctx.last_windows["changed"]) == (0, len(seq), 0, n)
    assert gunzip(root / "s2_segments.fa.gz") == model_header("spliced", 0, len(seq), paths[0]) + model_body(seq)


@pytest.mark.gpu
def test_not_b_on_a_chimera_writes_the_other_genomes_stretch(ctx, genomes):
    root, g, paths = genomes
    (root / "chimera.fa").write_bytes(b">chimera of two\n" + g[0] + b"\n" + g[1] + b"\n")
    ctx.classify_files(paths, str(root / "chimera.fa"), str(root / "c"), window=1000, segments="not=0", gz=False)
    seg = ctx.last_windows["segments"]
    assert seg["call"].tolist() == [0, 1] and ctx.last_windows["written"] == 1
    b, e = int(seg["begin"][1]), int(seg["end"][1])
    assert e == 40000 and open(root / "c_segments.fa", "rb").read() == model_header("chimera", b, e, paths[1]) + model_body((g[0] + g[1])[b:e])
    assert not os.path.exists(root / "c_segments.fa.gz")
    for what, calls in (("minor", [int(ctx.last_windows["mosaic"]["second"][0])]), ("major", [int(ctx.last_windows["mosaic"]["major"][0])]), ("none", [])):
        ctx.classify_files(paths, str(root / "chimera.fa"), str(root / "c"), window=1000, segments=what)
        assert [int(seg["call"][i]) for i in range(2) if b">chimera:%d-" % (int(seg["begin"][i]) + 1) in gunzip(root / "c_segments.fa.gz")] == calls, what


@pytest.mark.gpu
def test_taxonomy_files_and_fastq_input(ctx, bank, tmp_path):
    import test_taxonomy as tt
    refs, paths = bank
    W = 300
    recs = text_case(refs, W, 7)
    tree = tt.Tree(tt.file_lineages())
    (tmp_path / "t.fa").write_bytes(fasta(recs))
    (tmp_path / "lin.txt").write_text(tree.text)
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    lin = sp.taxonomy_lineages(tree.text, len(paths))
    rows0 = ctx.taxonomy_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "plain"), 2, 1, 2, window=W)
    rows = ctx.taxonomy_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "tax"), 2, 1, 2, window=W, window_call="taxon", segments="all")
    assert np.array_equal(rows, rows0)
    for suf in ("_segments.csv.gz", "_mosaic.csv.gz"):
        assert gunzip(tmp_path / ("tax" + suf)) == gunzip(tmp_path / ("plain" + suf))
    text = file_is_the_text(ctx, tmp_path / "tax_segments.fa.gz", recs, list(lin["names"]), "unclassified")
    assert b" unclassified\n" in text and any((b" " + n.encode() + b"\n") in text for n in lin["names"])
    node = int(ctx.last_windows["segments"]["call"][ctx.last_windows["segments"]["call"] < len(lin["names"])][0])
    ctx.taxonomy_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "node"), 2, 1, 2, window=W, segments="call=%d" % node, segments_min=31)
    file_is_the_text(ctx, tmp_path / "node_segments.fa.gz", recs, list(lin["names"]), "unclassified", "call=%d" % node, 31)
    r = subprocess.run([EXE, "-X", "t.fa", "-H", "lin.txt", "-y", "%d:taxon" % W, "-V", "2", "-I", "0.5", "-Z", "call=%d:31" % node, "-f", "bank.txt", "-o", "cli"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and gunzip(tmp_path / "cli_segments.fa.gz") == gunzip(tmp_path / "node_segments.fa.gz"), r.stdout
    with pytest.raises(sp.SpspError, match="node"):         # <b> against the nodes, once the tree is read: no sketch is
        ctx.taxonomy_files(["no such sketch.gz"] * len(paths), str(tmp_path / "t.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "no"), window=W,
                           segments="call=%d" % len(lin["names"]))
    # FASTQ in, FASTA out: the cleaned bases carry no qualities (Ns and lower case leave and fold in the ingest)
    reads = [(b"read%d extra words" % i, s) for i, (_, s) in enumerate(recs) if s]   # (read0 would be the empty record)
    reads[1] = (reads[1][0], reads[1][1][:40].lower() + b"NNN" + reads[1][1][40:])
    (tmp_path / "t.fq").write_bytes(b"".join(b"@" + n + b"\n" + q + b"\n+\n" + b"I" * len(q) + b"\n" for n, q in reads))
    ctx.classify_files(paths, str(tmp_path / "t.fq"), str(tmp_path / "fq"), 2, 2, 1, 2, window=W, segments="all")
    clean = [(n, s.upper().replace(b"N", b"")) for n, s in reads]
    text = file_is_the_text(ctx, tmp_path / "fq_segments.fa.gz", clean, paths, "unmatched")
    assert text.startswith(b">read1:1-%d " % (K - 1)) and b"@" not in text and b"+" not in text


@pytest.mark.gpu
def test_one_record_across_the_batch_seam_of_65535_windows(ctx, bank, tmp_path):
    """65 535 S + W + 1 bases at S = 3: 65 537 windows, so the record's windows fill one batch and begin the next, and its segments
    are cut from the ingest's bases behind both"""
    refs, paths = bank
    W = K + 2
    S = W - (K - 1)
    L = 65535 * S + W + 1
    rng = np.random.default_rng(23)
    seq = b"".join([refs[0], random_bases(rng, 4000), refs[1]] * (L // 10000 + 1))[:L]
    recs = [(b"short", refs[2][:W]), (b"long", seq), (b"tail", refs[1][:W])]
    (tmp_path / "t.fa").write_bytes(fasta(recs))
    import test_windows as tw
    rows, hits = ctx.classify_files(paths, str(tmp_path / "t.fa"), str(tmp_path / "win"), window=W, smooth=3, segments="all")
    first = ctx.last_windows["first_win"]
    assert first.tolist() == [0, 1, 65538, 65539] and len(rows) == 65539
    call, n_bins = sp.split_bins_classify("best", rows, hits, len(paths))   # (the rows handed out stay unsmoothed)
    c, s, changed = model_smooth(call, np.where(rows["listed"] > 0, hits["shared"][:, 0], 0), first, 3)
    segs, mosaic = tw.model_segments(c, rows["keys"], rows["hit_keys"], s, offsets([len(x) for _, x in recs]), K, W, n_bins)
    assert tw.rows_of(ctx.last_windows["segments"]) == segs and tw.rows_of(ctx.last_windows["mosaic"]) == mosaic and ctx.last_windows["changed"] == changed
    assert len(segs) > 3 and {int(g[8]) for g in segs} >= {0, 1, n_bins - 1}   # segments of both references and of none, on both sides of the seam
    text = file_is_the_text(ctx, tmp_path / "win_segments.fa.gz", recs, paths, "unmatched")
    assert b"".join(rec.partition(b"\n")[2].replace(b"\n", b"") for rec in text.split(b">")[1:] if rec.startswith(b"long:")) == seq
