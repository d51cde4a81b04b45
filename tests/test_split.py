"""Split: every record of a FASTA / FASTQ file written to the file of its reference or taxon, all files in one pass
(spsp_records_split_host / _device, spsp_split_bins_classify_host / _taxonomy_host, spsp_split_word_check_host, spsp_split_csv_host,
spsp_split_plan_host, spsp_split_stage_ms, spsp_classify_files_split, spsp_taxonomy_files_split; bin/comparator -X <records>
[-x <mates>] [-H <lineages>] -j <word> [-u]).

The rule (include/spsp.h, "split"), as model_split below has it, on the records of test_extract's model_begin: the slices of bin 0,
1, ... follow one another; inside a bin the records' bytes come verbatim and in record order; SPLIT_DROP writes nothing; the text's
last range, where it is not empty and lacks its newline, gets one wherever it lands.  The second yardstick is the extraction: bin b
of a split is the file -F writes for the word that names the same records.  Outputs are compared as bytes: no tolerance anywhere."""
import gzip
import itertools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
from test_extract import Dev, fa_rec, model_begin, model_extract, sweep_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
DROP = 0xFFFFFFFF
NONE = 0xFFFFFFFF
NEW_CALLS = ("spsp_split_plan_host", "spsp_records_split_host", "spsp_split_bins_classify_host", "spsp_split_bins_taxonomy_host", "spsp_split_word_check_host",
             "spsp_split_csv_host", "spsp_records_split_device", "spsp_split_stage_ms", "spsp_classify_files_split", "spsp_taxonomy_files_split")


# ---------------------------------------------------------------------------------------------------- the model

def model_split(text, bins, n_bins, begin=None):
    """-> (bytes, bin_off[n_bins + 1], bin_records[n_bins])"""
    text = bytes(text)
    begin = model_begin(text) if begin is None else [int(b) for b in begin]
    assert len(bins) == len(begin) - 1
    parts, records = [[] for _ in range(n_bins)], [0] * n_bins
    for r, b in enumerate(bins):
        if b == DROP:
            continue
        records[b] += 1                                    # (an empty range counts and adds nothing)
        part = text[begin[r]:begin[r + 1]]
        if part:                                           # (only the last record of a text can lack its newline: only it is looked at)
            parts[b].append(part + b"\n" if r == len(bins) - 1 and not part.endswith(b"\n") else part)
    slices = [b"".join(p) for p in parts]
    return b"".join(slices), [0] + list(itertools.accumulate(len(s) for s in slices)), records


def random_bins(rng, n_rec, n_bins):
    return [DROP if rng.randrange(8) == 0 else rng.randrange(n_bins) for _ in range(n_rec)]


def plan():
    p = sp.split_plan()
    return p["stretch_bytes"], p["record_tile"], p["sort_tile"]


# ---------------------------------------------------------------------------------------------------- not GPU

def test_model_on_hand_made_texts():
    fa = b">a\nAC\n>b\nGG\n>c\nT\n>d\nCC"                    # the last record lacks its newline
    assert model_begin(fa) == [0, 6, 12, 17, 22]
    assert model_split(fa, [2, 0, 1, 0], 3) == (b">b\nGG\n>d\nCC\n>c\nT\n>a\nAC\n", [0, 12, 17, 23], [2, 1, 1])   # ... and sits in bin 0 of 3: the newline is interior
    assert model_split(fa, [2, 0, DROP, 0], 3) == (b">b\nGG\n>d\nCC\n>a\nAC\n", [0, 12, 12, 18], [2, 0, 1])       # a DROP, and an empty bin in the middle
    assert model_split(fa, [1, 1, 2, 2], 4) == (b">a\nAC\n>b\nGG\n>c\nT\n>d\nCC\n", [0, 0, 12, 23, 23], [0, 2, 2, 0])   # an empty bin first and last
    assert model_split(fa, [DROP] * 4, 2) == (b"", [0, 0, 0], [0, 0])
    assert model_split(fa, [0, 0, 0, DROP], 1) == (fa[:17], [0, 17], [3])                 # the last record dropped: no newline anywhere
    assert model_split(b"", [0], 2) == (b"", [0, 0, 0], [1, 0])                           # the empty text: one empty record, which counts
    fq = b"@r1\nACGT\n+\nIIII\n@r2\nAC\n+\nII"
    assert model_split(fq, [1, 0], 2) == (b"@r2\nAC\n+\nII\n@r1\nACGT\n+\nIIII\n", [0, 12, 28], [1, 1])
    assert model_split(b"abcdefghi", [1, 1, 0, 1], 2, [0, 3, 3, 7, 9]) == (b"defgabchi\n", [0, 4, 10], [1, 3])    # ranges handed in, one of them empty
    # one bin is the extraction with every flag set
    assert model_split(fa, [0] * 4, 1)[0] == model_extract(fa, [1] * 4)[0] == fa + b"\n"


def test_host_split_equals_the_model():
    S, _, _ = plan()
    for seed in range(4):
        for fastq in (False, True):
            text = sweep_text(seed, fastq, S, 60)
            begin = model_begin(text)
            for n_bins in (1, 2, 7, 300):
                bins = random_bins(random.Random(seed * 1000 + n_bins), len(begin) - 1, n_bins)
                out, off, rec = sp.records_split(text, bins, n_bins)
                assert (out, off.tolist(), rec.tolist()) == model_split(text, bins, n_bins, begin), (seed, fastq, n_bins)
    out, off, rec = sp.records_split(b"abcdefghi", [1, 1, 0, 1], 2, [0, 3, 3, 7, 9])
    assert (out, off.tolist(), rec.tolist()) == (b"defgabchi\n", [0, 4, 10], [1, 3])
    out, off, rec = sp.records_split(b"", [0], 2)
    assert (out, off.tolist(), rec.tolist()) == (b"", [0, 0, 0], [1, 0])


def classify_rows(listed_refs, top):
    records = np.zeros(len(listed_refs), dtype=sp.CLASSIFY_RECORD_DTYPE)
    hits = np.zeros((len(listed_refs), top), dtype=sp.CLASSIFY_HIT_DTYPE)
    for r, refs in enumerate(listed_refs):
        records[r]["listed"] = records[r]["passing"] = len(refs)
        for i, j in enumerate(refs):
            hits[r, i] = (j, 100 - i)
    return records, hits


# root 0 > a 1 > b 2 > {c 3, d 4}; root > e 5 > f 6
HAND_PARENT, HAND_DEPTH = [0, 0, 1, 2, 2, 0, 5], [0, 1, 2, 3, 3, 1, 2]


def model_bins_taxonomy(what, nodes, parent, depth):
    out = []
    for node in nodes:
        if node == NONE:
            out.append(len(parent))
            continue
        if what.startswith("depth="):
            while depth[node] > int(what[6:]):
                node = parent[node]
        out.append(node)
    return out


def test_bin_functions_every_word_at_equality_and_one_off():
    records, hits = classify_rows([[], [3], [4, 3], [0, 4], [0], [2, 0]], 2)
    bins, n_bins = sp.split_bins_classify("best", records, hits, 5)
    assert (bins.tolist(), n_bins) == ([5, 3, 4, 0, 0, 2], 6)                             # listed == 0 goes to bin n_ref: unmatched
    for j in range(5):                                     # bin j is what the extraction's best=<j> flags, the last bin what unmatched flags
        assert (bins == j).tolist() == sp.extract_flags_classify("best=%d" % j, records, hits, 5).astype(bool).tolist()
    assert (bins == 5).tolist() == sp.extract_flags_classify("unmatched", records, hits, 5).astype(bool).tolist()
    tx = np.zeros(8, dtype=sp.TAXONOMY_RECORD_DTYPE)
    tx["node"] = [NONE, 0, 1, 2, 3, 4, 5, 6]
    for what in ("taxon", "depth=1", "depth=2", "depth=3", "depth=4", "depth=32"):
        bins, n_bins = sp.split_bins_taxonomy(what, tx, HAND_PARENT, HAND_DEPTH)
        assert (bins.tolist(), n_bins) == (model_bins_taxonomy(what, tx["node"].tolist(), HAND_PARENT, HAND_DEPTH), 8), what
    assert sp.split_bins_taxonomy("taxon", tx, HAND_PARENT, HAND_DEPTH)[0].tolist() == [7, 0, 1, 2, 3, 4, 5, 6]   # NONE goes to bin n_nodes: unclassified
    # depth=<d> for a node at depth d - 1, d and d + 1: nodes 1 (depth 1), 2 (depth 2), 3 (depth 3) against d = 2
    assert sp.split_bins_taxonomy("depth=2", tx[2:5], HAND_PARENT, HAND_DEPTH)[0].tolist() == [1, 2, 2]
    assert sp.split_bins_taxonomy("depth=1", tx, HAND_PARENT, HAND_DEPTH)[0].tolist() == [7, 0, 1, 1, 1, 1, 5, 5]  # the root's own records keep the root
    assert sp.split_bins_taxonomy("depth=3", tx, HAND_PARENT, HAND_DEPTH)[0].tolist() == [7, 0, 1, 2, 3, 4, 5, 6]


def test_refusals_with_the_word_or_the_record_in_the_text():
    records, hits = classify_rows([[], [1]], 2)
    tx = np.zeros(2, dtype=sp.TAXONOMY_RECORD_DTYPE)
    calls = lambda what: (lambda: sp.split_bins_classify(what, records, hits, 2), lambda: sp.split_bins_taxonomy(what, tx, HAND_PARENT, HAND_DEPTH),
                          lambda: sp.split_word_check(what, False), lambda: sp.split_word_check(what, True))
    for what in ("", "bests", "Best", "best=0", "matched", "taxon=1", "clade=1", "depth", "depth=", "depth=-1", "depth= 1", "depth=1x", "depth=4294967296"):
        for call in calls(what):
            with pytest.raises(sp.SpspError) as e:
                call()
            assert e.value.code == sp.ERR_ARG and "'%s'" % what in str(e.value) and "names no bins" in str(e.value), what
    for what in ("depth=0", "depth=33"):
        for call in calls(what)[1::2]:
            with pytest.raises(sp.SpspError) as e:
                call()
            assert e.value.code == sp.ERR_ARG and "'%s'" % what in str(e.value) and "1 .. 32" in str(e.value), what
    for what in ("taxon", "depth=2", "depth=0"):           # a taxonomy word on classify's rows
        for call in calls(what)[0::2]:
            with pytest.raises(sp.SpspError) as e:
                call()
            assert e.value.code == sp.ERR_ARG and "'%s'" % what in str(e.value) and "taxonomy's rows" in str(e.value), what
    for call in calls("best")[1::2]:                       # and the reverse
        with pytest.raises(sp.SpspError) as e:
            call()
        assert e.value.code == sp.ERR_ARG and "'best'" in str(e.value) and "classify's rows" in str(e.value)
    sp.split_word_check("best", False), sp.split_word_check("taxon", True), sp.split_word_check("depth=1", True), sp.split_word_check("depth=32", True)
    text = b">a\nAC\n>b\nGG\n>c\nT\n"
    for bins, n_bins, word in (([0, 1, 2], 2, "bin[2] = 2"), ([5, 0, 0], 5, "bin[0] = 5"), ([0, 0xFFFFFFFE, 0], 3, "bin[1] = 4294967294")):
        with pytest.raises(sp.SpspError) as e:
            sp.records_split(text, bins, n_bins)
        assert e.value.code == sp.ERR_ARG and word in str(e.value)
    for n_bins in (0, sp.split_plan()["max_bins"] + 1):
        with pytest.raises(sp.SpspError) as e:
            sp.records_split(text, [0, 0, 0], n_bins)
        assert e.value.code == sp.ERR_ARG and "n_bins = %d" % n_bins in str(e.value)
    for begin in ([0, 4, 3, 9], [0, 3, 7, 18]):
        with pytest.raises(sp.SpspError) as e:
            sp.records_split(text, [0, 0, 0], 1, begin)
        assert e.value.code == sp.ERR_ARG and "begin" in str(e.value)


def test_abi_has_the_split_calls_and_the_plan_is_the_kernels_constants():
    assert set(NEW_CALLS) <= set(sp.ABI_SYMBOLS)
    for name in NEW_CALLS:
        assert hasattr(sp.lib(), name)
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    value = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))
    assert re.search(r"kExRecTile = kExThreads \* kExRecsPerLane;", text) and re.search(r"kExThreads = 256, kExRecsPerLane = 8,", text)
    assert re.search(r"kRsThreads = 256, kRsPer = 8, kRsTile = kRsThreads \* kRsPer;", text) and re.search(r"kSpMaxBins = 1u << 24;", text)
    assert sp.split_plan() == {"stretch_bytes": value("kExStretch"), "record_tile": 256 * 8, "sort_tile": 256 * 8, "max_bins": 1 << 24}
    assert sp.split_plan()["stretch_bytes"] == sp.extract_plan()["stretch_bytes"] and sp.SPLIT_DROP == DROP
    header = open(os.path.join(ROOT, "include", "spsp.h")).read()
    assert "#define SPSP_SPLIT_DROP 0xffffffffu" in header and "#define SPSP_SPLIT_MAX_BINS 16777216u" in header


def test_the_manifest():
    names = ["refA", "dir/ref B.gz", "refC"]
    got = sp.split_csv("run", names, "unmatched", [2, 0, 1, 4], [0, 10, 10, 15, 40], ".fq.gz").decode()
    assert got == ("bin,name,records,bytes,file\n0,refA,2,10,run_split_0.fq.gz\n2,refC,1,5,run_split_2.fq.gz\n"
                   "unmatched,unmatched,4,25,run_split_unmatched.fq.gz\n")
    got = sp.split_csv("run", names, "unclassified", [0, 3, 0, 0], [0, 0, 9, 9, 9], ".fa", [0, 0, 30, 30, 30], ".fq.gz").decode()
    assert got == "bin,name,records,bytes_1,file_1,bytes_2,file_2\n1,dir/ref B.gz,3,9,run_split_1_1.fa,30,run_split_1_2.fq.gz\n"


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    (tmp_path / "lin.txt").write_text("a\nb\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [(("-j", "best"), "-j"), (("-X", "r.fa", "-j", "best", "-F", "matched"), "-j"), (("-X", "r.fa", "-j", "taxon"), "-j"),
             (("-X", "r.fa", "-j", "depth=1"), "-j"), (("-X", "r.fa", "-H", "lin.txt", "-j", "best"), "-j"), (("-D", "r.fa", "-j", "best"), "-j"),
             (("-X", "r.fa", "-j", "everything"), "-j"), (("-X", "r.fa", "-H", "lin.txt", "-j", "depth=0"), "-j"),
             (("-X", "r.fa", "-H", "lin.txt", "-j", "depth=33"), "-j"), (("-u",), "-u"), (("-X", "r.fa", "-u"), "-u")]
    for args, letter in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and letter in r.stdout, (args, r.stdout, r.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
    assert run("-u", "-f", "list.txt").stdout == "-u writes the records of -F plain instead of gzipped: it needs -F\n"   # the old line, to the letter
    assert "taxonomy's rows" in run("-X", "r.fa", "-j", "taxon", "-f", "list.txt").stdout
    assert "classify's rows" in run("-X", "r.fa", "-H", "lin.txt", "-j", "best", "-f", "list.txt").stdout
    assert "-j " in run().stdout


def test_host_functions_under_the_sanitizers():
    """tests/tools/split_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the host
    split, the bin functions with their refusals and the manifest (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "split_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "split_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def upload_begin(begin):
    import torch
    t = torch.from_numpy(np.array(begin, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def check(ctx, d, bins, n_bins, begin=None, note=None):
    """one split of the text in HBM against the model (begin: starts handed in)"""
    t = None if begin is None else upload_begin(begin)
    out, off, rec = ctx.records_split_device(d.ptr, d.n, bins, n_bins, None if t is None else t.data_ptr())
    want = model_split(d.text, bins, n_bins, begin)
    assert out.tobytes() == want[0], note
    assert (off.tolist(), rec.tolist()) == want[1:], note
    return want


@pytest.mark.gpu
def test_one_bin_is_the_extraction_of_every_record(ctx):
    S, _, _ = plan()
    for text in (sweep_text(1, False, S, 60), sweep_text(0, False, S, 60), sweep_text(1, True, S, 60), sweep_text(2, True, S, 60)):
        d = Dev(text)
        n = len(model_begin(text)) - 1
        want = check(ctx, d, [0] * n, 1)
        out, kept = ctx.records_extract_device(d.ptr, d.n, [1] * n)
        assert out.tobytes() == want[0] and kept == n
        keep = [r & 1 for r in range(n)]                   # and the extraction on the same context still answers as its model says
        out, kept = ctx.records_extract_device(d.ptr, d.n, keep)
        assert (out.tobytes(), kept) == model_extract(text, keep)
        check(ctx, d, [0] * n, 1)


@pytest.mark.gpu
def test_the_copy_at_every_alignment_difference(ctx):
    """a dropped first record of 1 .. 16 bytes in front of two alternating bins: every difference of source and output alignment
    in both bins; with the bins reversed the runs move backwards in the text"""
    S, _, _ = plan()
    rest = [fa_rec(n, b"r%d" % n, b"ACGTTGCA") for n in (5000, 17, 3 * S + 5, 33, 70, 4097, 2, 161)]
    for drop in range(1, 17):
        first = b"\n" if drop == 1 else b"x" * (drop - 1) + b"\n"
        d = Dev(first + b"".join(rest))
        check(ctx, d, [DROP] + [r & 1 for r in range(len(rest))], 2, note=drop)
        check(ctx, d, [DROP] + [1 - (r & 1) for r in range(len(rest))], 2, note=drop)


@pytest.mark.gpu
def test_the_appended_newline_in_the_interior(ctx):
    """the last record lacks its newline; the records of its bin in front of it are padded so that the newline lands on the
    stretch's and a store's seams, with other bins behind it"""
    S, _, _ = plan()
    last = b">last\nACGT"
    for at in (S - 1, S, S + 1, 4096 + 15, 4096 + 16, 4096 + 17, 2 * S + 16 - 1, 15, 16, 17):
        pad = at - len(last)
        front = [fa_rec(pad, b"pad", b"AC")] if pad >= 2 else []
        text = b"".join(front) + fa_rec(100, b"b", b"G") + fa_rec(300, b"c", b"T") + last
        d = Dev(text)
        f = len(front)
        if f:
            out, off, _ = check(ctx, d, [0] * f + [1, 2, 0], 3, note=at)                  # in bin 0 of 3, behind the padding
            assert out[at:at + 1] == b"\n" and out[at - 4:at] == b"ACGT" and off[1] == at + 1
            out, off, _ = check(ctx, d, [1] * f + [0, 0, 1], 3, note=at)                  # the same with bin 1 of 3: other bins on both sides
            assert out[400 + at:401 + at] == b"\n" and off[2] == 401 + at and off[3] == off[2]
        out, off, _ = check(ctx, d, [1] * f + [1, 1, 0], 3, note=at)                      # alone in its bin, the first
        assert out[:11] == last + b"\n" and off[1] == 11
        out, off, _ = check(ctx, d, [0] * f + [2, 0, 1], 3, note=at)                      # alone in its bin, in the middle
        assert out[off[1]:off[2]] == last + b"\n"
        out, off, _ = check(ctx, d, [0] * f + [1, 1, 2], 3, note=at)                      # in the last bin: the output's last byte
        assert out.endswith(last + b"\n") and off[3] == len(text) + 1


@pytest.mark.gpu
def test_the_copy_at_the_stretch_seams(ctx):
    S, _, _ = plan()
    for n in (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1):
        # a bin that ends at output byte n, another behind it
        text = fa_rec(n - 40, b"x", b"AC") + fa_rec(50, b"y", b"G") + fa_rec(40, b"z", b"T") + fa_rec(S // 2, b"w", b"CA")
        d = Dev(text)
        _, off, _ = check(ctx, d, [0, 1, 0, 1], 2, note=n)
        assert off[1] == n
        _, off, _ = check(ctx, d, [1, 2, 1, 2], 3, note=n)                                # ... behind an empty bin
        assert off[:3] == [0, 0, n]
        check(ctx, d, [1, 0, 1, 0], 2, note=n)
        check(ctx, d, [0, DROP, 0, DROP], 2, note=n)                                      # ... and as the output's end
    for n in (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1):                               # an output of exactly n bytes
        text = fa_rec(n - n // 2, b"a") + fa_rec(n // 2, b"b", b"C")
        d = Dev(text)
        out, off, _ = check(ctx, d, [1, 0], 2, note=n)
        assert len(out) == n == off[2]
        text = fa_rec(n - n // 2, b"a") + fa_rec(n // 2 - 1, b"b", b"C")[:-1] + b"C"      # ... the appended newline among them, first bin's last byte
        out, off, _ = check(ctx, Dev(text), [1, 0], 2, note=n)
        assert len(out) == n and out[off[1] - 1:off[1]] == b"\n"


def tiny_records(n):
    return [b">%d\n" % r for r in range(n)]


@pytest.mark.gpu
def test_the_sorts_seams(ctx):
    """every record is a run of its own: run counts around the sort's tile, bin counts around its digits"""
    _, rec_tile, sort_tile = plan()
    texts = {n: Dev(b"".join(tiny_records(n))) for n in (sort_tile - 1, sort_tile, sort_tile + 1, 2 * sort_tile + 1)}
    assert rec_tile == sort_tile
    for n, d in texts.items():
        for n_bins in (255, 256, 257, 65536, 65537):
            check(ctx, d, [r % n_bins for r in range(n)], n_bins, note=(n, n_bins))
            check(ctx, d, [n_bins - 1 - r % n_bins for r in range(n)], n_bins, note=(n, n_bins))
    n = 2 * sort_tile + 1
    check(ctx, texts[n], [256 * (r % 5) for r in range(n)], 1025 + 1)                     # all runs with one low digit
    check(ctx, texts[n], [65536 * (r % 3) + 256 * (r % 5) for r in range(n)], 3 * 65536)  # ... and three digits, two of them sparse
    # stability: 300 records with names of their own in bin 7, between records of 40 other bins
    rng = random.Random(3)
    recs, bins = [], []
    for i in range(300):
        for _ in range(rng.randrange(4)):
            recs.append(b">other\nT\n")
            bins.append(rng.choice([b for b in range(41) if b != 7]))
        recs.append(b">name%d\nAC\n" % i)
        bins.append(7)
    out, off, rec = check(ctx, Dev(b"".join(recs)), bins, 41)
    assert out[off[7]:off[8]] == b"".join(b">name%d\nAC\n" % i for i in range(300)) and rec[7] == 300


@pytest.mark.gpu
def test_stores_made_of_many_runs_and_the_refusals(ctx):
    """starts handed in: ranges of 1 .. 8 bytes with bins r % 3 -- with one byte each, every byte of a 16-byte store is a run"""
    rng = random.Random(5)
    text = bytes(rng.choice(b"ACGTN\n>@") for _ in range(40000))
    d = Dev(text)
    for width in (1, 2, 3, 5, 8, None):
        begin, at = [0], 0
        while at < len(text):
            at = min(len(text), at + (width or rng.randint(1, 8)))
            begin.append(at)
        check(ctx, d, [r % 3 for r in range(len(begin) - 1)], 3, begin, note=width)
    for begin in ([0, 100, 50, 120], [0, 100, len(text) + 1], [5, 4]):                     # starts that decrease or leave the text
        t = upload_begin(begin)
        with pytest.raises(sp.SpspError) as e:
            ctx.records_split_device(d.ptr, d.n, [0] * (len(begin) - 1), 2, t.data_ptr())
        assert e.value.code == sp.ERR_ARG and "d_begin" in str(e.value)
    small = Dev(b">a\nAC\n>b\nGG\n>c\nT\n")
    with pytest.raises(sp.SpspError) as e:                 # a bin out of range names its record
        ctx.records_split_device(small.ptr, small.n, [0, 1, 2], 2)
    assert e.value.code == sp.ERR_ARG and "bin[2] = 2" in str(e.value)
    for bins in ([0, 1], [0, 1, 1, 0]):                    # bins for another number of records than the text holds
        with pytest.raises(sp.SpspError) as e:
            ctx.records_split_device(small.ptr, small.n, bins, 2)
        assert e.value.code == sp.ERR_ARG and "3 record(s)" in str(e.value)
    for n_bins in (0, sp.split_plan()["max_bins"] + 1):
        with pytest.raises(sp.SpspError) as e:
            ctx.records_split_device(small.ptr, small.n, [0, 0, 0], n_bins)
        assert e.value.code == sp.ERR_ARG and "n_bins = %d" % n_bins in str(e.value)
    check(ctx, small, [1, DROP, 0], 2)                     # and the context still answers


@pytest.mark.gpu
def test_one_long_record_among_two_byte_records(ctx):
    S, _, _ = plan()
    small = 3000
    text = b">\n" * small + fa_rec(40 * S, b"contig", b"ACGTTGCAAC") + b">\n" * small
    d = Dev(text)
    side = [2 * (r & 1) for r in range(small)]
    check(ctx, d, side + [1] + side, 3)
    check(ctx, d, [2 - b for b in side] + [1] + side, 3)
    check(ctx, d, [0] * small + [1] + [2] * small, 3)      # three runs


@pytest.mark.gpu
def test_empty_results(ctx):
    S, _, _ = plan()
    text = sweep_text(1, False, S, 40)
    d = Dev(text)
    n = len(model_begin(text)) - 1
    out, off, rec = ctx.records_split_device(d.ptr, d.n, [DROP] * n, 5)                   # everything dropped, from a grid sized by the text
    assert len(out) == 0 and off.tolist() == [0] * 6 and rec.tolist() == [0] * 5
    out, off, rec = ctx.records_split_device(None, 0, [0], 2)                             # the empty text: one empty record
    assert len(out) == 0 and off.tolist() == [0, 0, 0] and rec.tolist() == [1, 0]
    out, off, rec = ctx.records_split_device(None, 0, [DROP], 2)
    assert len(out) == 0 and off.tolist() == [0, 0, 0] and rec.tolist() == [0, 0]
    small = Dev(b"abcdefghi")
    for begin, bins in (([0, 3, 3, 7, 9], [1, 1, 0, 1]), ([0, 0, 0, 9, 9], [0, 1, 1, 1]), ([4, 4, 4], [0, 1]), ([0, 3, 3, 3, 9, 9], [0, 0, 0, 0, 0])):
        want = check(ctx, small, bins, 2, begin, note=begin)                              # empty ranges count in bin_records and add no bytes
        assert sum(want[2]) == len(bins)


@pytest.mark.gpu
def test_two_calls_on_one_context(ctx):
    S, _, _ = plan()
    big = b"".join(fa_rec(300, b"r%d" % i, b"ACGT"[i % 4:i % 4 + 1]) for i in range(800))
    small = b">s\nTT\n>t\nGG\n>u\nCC"
    d_big, d_small = Dev(big), Dev(small)
    check(ctx, d_big, [r % 7 for r in range(800)], 7)
    assert len(big) > 10 * S
    out, off, rec = ctx.records_split_device(d_small.ptr, d_small.n, [1, DROP, 0], 2)
    assert (out.tobytes(), off.tolist(), rec.tolist()) == (b">u\nCC\n>s\nTT\n", [0, 6, 12], [1, 1])   # no byte of the first call
    # the starts of an extents call handed back in, twice: the split leaves them as they are
    d_begin, n_rec = ctx.records_extents_device(d_big.ptr, d_big.n)
    for bins in ([r % 3 for r in range(800)], [DROP if r % 3 == 0 else r % 2 for r in range(800)]):
        out, off, rec = ctx.records_split_device(d_big.ptr, d_big.n, bins, 3, d_begin, n_rec)
        assert (out.tobytes(), off.tolist(), rec.tolist()) == model_split(big, bins, 3)
    assert ctx.to_host(d_begin, n_rec + 1, np.uint64).tolist() == model_begin(big)
    ctx.timing_enable(True)
    ctx.split_stage_ms()
    ctx.records_split_device(d_big.ptr, d_big.n, [r % 300 for r in range(800)], 300)
    ms = ctx.split_stage_ms()
    ctx.timing_enable(False)
    assert list(ms) == ["starts", "runs", "order", "offsets", "copy"] and all(v > 0 for v in ms.values()), ms
    assert sum(ctx.split_stage_ms().values()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_a_seeded_sweep_against_the_model(ctx, seed):
    S, _, _ = plan()
    rng = random.Random(100 + seed)
    for fastq in (False, True):
        text = sweep_text(seed, fastq, S)
        d = Dev(text)
        n = len(model_begin(text)) - 1
        for i in range(3):                                 # three of the five bin counts per text; the seeds and kinds between them take each several times
            n_bins = (1, 2, 7, 300, 70000)[(seed + 2 * fastq + i) % 5]
            check(ctx, d, random_bins(rng, n, n_bins), n_bins, note=(seed, fastq, n_bins))


# ------------------------------------------------------------------------------------------ files and the command line

def gunzip(path):
    with gzip.open(str(path), "rb") as f:
        return f.read()


def split_files(root, tag):
    return sorted(f for f in os.listdir(str(root)) if f.startswith(tag + "_split"))


def model_manifest(tag, names, last_name, bins, n_bins, texts, suffixes):
    """the manifest's lines for one text, or for the two of a paired run"""
    parts = [model_split(t, bins, n_bins) for t in texts]
    paired = len(texts) == 2
    lines = ["bin,name,records,bytes_1,file_1,bytes_2,file_2" if paired else "bin,name,records,bytes,file"]
    for b in range(n_bins):
        if parts[0][2][b]:
            label = last_name if b == n_bins - 1 else str(b)
            cols = [label, last_name if b == n_bins - 1 else names[b], str(parts[0][2][b])]
            for i, p in enumerate(parts):
                cols += [str(p[1][b + 1] - p[1][b]), "%s_split_%s%s%s" % (tag, label, "_%d" % (i + 1) if paired else "", suffixes[i])]
            lines.append(",".join(cols))
    return "\n".join(lines) + "\n", parts


@pytest.mark.gpu
def test_classify_files_with_a_split_and_the_command_line(ctx, tmp_path):
    import test_classify as tc
    import test_prevalence as tp
    refs, recs = tc.file_case()
    refs = refs[:3]                                        # three references; the records are reads of each (and of their mutated copies) and of none
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, 1.0)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    text = tc.fastq_of(recs)
    with gzip.open(str(tmp_path / "recs.fq.gz"), "wb") as f:
        f.write(text)
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    cli = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    top, rp = 2, str(tmp_path / "recs.fq.gz")
    ctx.classify_files(paths, rp, str(tmp_path / "plain"), top)
    csvs = tc.both_files(tmp_path, "plain")
    records, hits = ctx.classify_files(paths, rp, str(tmp_path / "s"), top, split="best")
    bins, n_bins = sp.split_bins_classify("best", records, hits, len(paths))
    assert n_bins == 4 and set(bins.tolist()) == {0, 1, 2, 3}                             # reads of each and of none
    manifest, (want,) = model_manifest("s", paths, "unmatched", bins.tolist(), n_bins, [text], [".fq.gz"])
    assert gunzip(tmp_path / "s_split.csv.gz").decode() == manifest
    assert ctx.last_split == {"bins": 4, "records": len(recs), "bytes_out": len(want[0])} and len(want[0]) == len(text)
    assert tc.both_files(tmp_path, "s") == csvs            # the CSVs of a run without the word, byte for byte
    assert split_files(tmp_path, "s") == sorted(["s_split.csv.gz"] + ["s_split_%s.fq.gz" % b for b in ("0", "1", "2", "unmatched")])
    for j, what in enumerate(("best=0", "best=1", "best=2", "unmatched")):                # every bin is the file -F writes for the same records
        ctx.classify_files(paths, rp, str(tmp_path / ("e%d" % j)), top, extract=what)
        label = "unmatched" if j == 3 else str(j)
        got = gunzip(tmp_path / ("s_split_%s.fq.gz" % label))
        assert got == gunzip(tmp_path / ("e%d_extract.fq.gz" % j)) == want[0][want[1][j]:want[1][j + 1]], what
    for tag, plain in (("c", False), ("cu", True)):        # the command line, gzipped and plain
        r = cli("-X", "recs.fq.gz", "-j", "best", "-Y", str(top), "-f", "bank.txt", "-o", tag, *(["-u"] if plain else []))
        assert r.returncode == 0 and "split best: 4 bin(s) written, %d record(s), %d byte(s)" % (len(recs), len(text)) in r.stdout, r.stdout + r.stderr
        assert tc.both_files(tmp_path, tag) == csvs
        suffix = ".fq" if plain else ".fq.gz"
        assert split_files(tmp_path, tag) == sorted([tag + "_split.csv.gz"] + [tag + "_split_%s%s" % (b, suffix) for b in ("0", "1", "2", "unmatched")])
        assert gunzip(tmp_path / (tag + "_split.csv.gz")).decode() == model_manifest(tag, paths, "unmatched", bins.tolist(), n_bins, [text], [suffix])[0]
        for j, label in enumerate(("0", "1", "2", "unmatched")):
            name = tmp_path / (tag + "_split_%s%s" % (label, suffix))
            assert (name.read_bytes() if plain else gunzip(name)) == want[0][want[1][j]:want[1][j + 1]]
    # only bins with records have files: the unmatched records alone, fed back, fill one bin
    records, hits = ctx.classify_files(paths, str(tmp_path / "s_split_unmatched.fq.gz"), str(tmp_path / "back"), top, split="best", gz=False)
    assert (records["listed"] == 0).all() and split_files(tmp_path, "back") == ["back_split.csv.gz", "back_split_unmatched.fq"]
    assert (tmp_path / "back_split_unmatched.fq").read_bytes() == want[0][want[1][3]:]
    # refusals write nothing, and come before any file is read
    for what, word in (("taxon", "taxonomy's rows"), ("best=0", "names no bins"), ("depth=0", "taxonomy's rows")):
        with pytest.raises(sp.SpspError) as e:
            ctx.classify_files(["no such sketch.gz"] * 3, str(tmp_path / "none.fa"), str(tmp_path / "no"), top, split=what)
        assert e.value.code == sp.ERR_ARG and word in str(e.value) and what in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
def test_taxonomy_files_with_a_split_and_the_command_line(ctx, tmp_path):
    import test_classify as tc
    import test_prevalence as tp
    import test_taxonomy as tt
    refs, recs = tc.file_case()
    tree = tt.Tree(tt.file_lineages())
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, 1.0)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    fasta = tc.fasta_of(recs)
    (tmp_path / "recs.fa").write_bytes(fasta)
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    (tmp_path / "lin.txt").write_text(tree.text)
    lin = sp.taxonomy_lineages(tree.text, len(paths))
    T = len(lin["parent"])
    args = (paths, str(tmp_path / "recs.fa"), str(tmp_path / "lin.txt"))
    ctx.taxonomy_files(*args, str(tmp_path / "plain"))
    csvs = tt.both_files(tmp_path, "plain")
    cli = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    # taxon: one file per node that was called
    records = ctx.taxonomy_files(*args, str(tmp_path / "t"), split="taxon", gz=False)
    bins, n_bins = sp.split_bins_taxonomy("taxon", records, lin["parent"], lin["depth"])
    assert n_bins == T + 1 and bins.tolist() == [T if x == NONE else x for x in records["node"].tolist()]
    manifest, (want,) = model_manifest("t", list(tree.names), "unclassified", bins.tolist(), n_bins, [fasta], [".fa"])
    assert (tmp_path / "t_split.csv.gz").exists() and gunzip(tmp_path / "t_split.csv.gz").decode() == manifest
    assert tt.both_files(tmp_path, "t") == csvs
    called = sorted(set(bins.tolist()))
    assert len(called) >= 4 and T in called and any(lin["size"][b] > 1 for b in called if b != T)   # leaves, inner nodes and none
    label = lambda b: "unclassified" if b == T else str(b)
    assert split_files(tmp_path, "t") == sorted(["t_split.csv.gz"] + ["t_split_%s.fa" % label(b) for b in called])
    assert ctx.last_split == {"bins": len(called), "records": len(recs), "bytes_out": len(fasta)}
    for b in sorted(set(called) | {0}):                    # every file equals -F taxon=<t>; a node nobody was called at has no file, and -F keeps nothing
        what = "unclassified" if b == T else "taxon=%d" % b
        ctx.taxonomy_files(*args, str(tmp_path / ("e%d" % b)), extract=what, gz=False)
        kept = (tmp_path / ("e%d_extract.fa" % b)).read_bytes()
        assert kept == want[0][want[1][b]:want[1][b + 1]], what
        assert (tmp_path / ("t_split_%s.fa" % label(b))).read_bytes() == kept if b in called else kept == b"", what
    r = cli("-X", "recs.fa", "-H", "lin.txt", "-j", "taxon", "-u", "-f", "bank.txt", "-o", "ct")
    assert r.returncode == 0 and "split taxon: %d bin(s) written" % len(called) in r.stdout, r.stdout + r.stderr
    assert tt.both_files(tmp_path, "ct") == csvs and split_files(tmp_path, "ct") == ["c" + f for f in split_files(tmp_path, "t")]
    for f in split_files(tmp_path, "t")[1:]:
        assert (tmp_path / ("c" + f)).read_bytes() == (tmp_path / f).read_bytes()
    # depth=1: a node at depth 1 takes its whole clade, the root's own records stay at the root
    records = ctx.taxonomy_files(*args, str(tmp_path / "d"), split="depth=1")
    bins, n_bins = sp.split_bins_taxonomy("depth=1", records, lin["parent"], lin["depth"])
    top_node = tree.num[("Bacteria",)]
    assert lin["depth"][top_node] == 1 and {top_node, T} <= set(bins.tolist()) <= {0, top_node, T}
    assert tt.both_files(tmp_path, "d") == csvs
    assert split_files(tmp_path, "d") == sorted(["d_split.csv.gz"] + ["d_split_%s.fa.gz" % label(b) for b in set(bins.tolist())])
    ctx.taxonomy_files(*args, str(tmp_path / "dc"), extract="clade=%d" % top_node)
    assert gunzip(tmp_path / ("d_split_%d.fa.gz" % top_node)) == gunzip(tmp_path / "dc_extract.fa.gz")
    root_own = (tmp_path / "e0_extract.fa").read_bytes()   # -F taxon=0, written above
    assert gunzip(tmp_path / "d_split_0.fa.gz") == root_own if 0 in bins.tolist() else root_own == b""
    assert gunzip(tmp_path / "d_split_unclassified.fa.gz") == (tmp_path / ("e%d_extract.fa" % T)).read_bytes()
    r = cli("-X", "recs.fa", "-H", "lin.txt", "-j", "depth=1", "-f", "bank.txt", "-o", "cd")
    assert r.returncode == 0 and "split depth=1: %d bin(s) written" % len(set(bins.tolist())) in r.stdout, r.stdout + r.stderr
    assert [gunzip(tmp_path / ("c" + f)) for f in split_files(tmp_path, "d")[1:]] == [gunzip(tmp_path / f) for f in split_files(tmp_path, "d")[1:]]
    assert gunzip(tmp_path / "cd_split.csv.gz") == gunzip(tmp_path / "d_split.csv.gz").replace(b",d_split_", b",cd_split_")
    for what, word in (("best", "classify's rows"), ("depth=33", "1 .. 32"), ("clade=1", "names no bins")):
        with pytest.raises(sp.SpspError) as e:
            ctx.taxonomy_files(["no such sketch.gz"] * len(paths), str(tmp_path / "none.fa"), str(tmp_path / "no lineages.txt"), str(tmp_path / "no"), split=what)
        assert e.value.code == sp.ERR_ARG and word in str(e.value) and what in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
def test_paired_files_with_a_split(ctx, tmp_path):
    import test_classify as tc
    import test_pairs as pairs_mod
    import test_prevalence as tp
    refs, pairs = pairs_mod.pair_case()
    refs = refs[:3]
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, 1.0)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    t1, t2 = pairs_mod.fasta_mates(pairs, 1), pairs_mod.fastq_mates(pairs, 2)
    (tmp_path / "r1.fa").write_bytes(t1)
    with gzip.open(str(tmp_path / "r2.fq.gz"), "wb") as f:
        f.write(t2)
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    top, a, m = 2, str(tmp_path / "r1.fa"), str(tmp_path / "r2.fq.gz")
    ctx.classify_files(paths, a, str(tmp_path / "plain"), top, mates_path=m)
    csvs = tc.both_files(tmp_path, "plain")
    records, hits = ctx.classify_files(paths, a, str(tmp_path / "s"), top, mates_path=m, split="best", gz=False)
    bins, n_bins = sp.split_bins_classify("best", records, hits, len(paths))
    assert set(bins.tolist()) == {0, 1, 2, 3} and tc.both_files(tmp_path, "s") == csvs
    manifest, (w1, w2) = model_manifest("s", paths, "unmatched", bins.tolist(), n_bins, [t1, t2], [".fa", ".fq"])
    assert gunzip(tmp_path / "s_split.csv.gz").decode() == manifest
    assert ctx.last_split == {"bins": 4, "records": len(pairs), "bytes_out": len(t1) + len(t2)}
    labels = ("0", "1", "2", "unmatched")
    assert split_files(tmp_path, "s") == sorted(["s_split.csv.gz"] + ["s_split_%s_%d.%s" % (b, i, "fa" if i == 1 else "fq") for b in labels for i in (1, 2)])
    for j, what in enumerate(("best=0", "best=1", "best=2", "unmatched")):
        ctx.classify_files(paths, a, str(tmp_path / ("e%d" % j)), top, mates_path=m, extract=what, gz=False)
        g1, g2 = (tmp_path / ("s_split_%s_1.fa" % labels[j])).read_bytes(), (tmp_path / ("s_split_%s_2.fq" % labels[j])).read_bytes()
        assert g1 == (tmp_path / ("e%d_extract_1.fa" % j)).read_bytes() == w1[0][w1[1][j]:w1[1][j + 1]], what
        assert g2 == (tmp_path / ("e%d_extract_2.fq" % j)).read_bytes() == w2[0][w2[1][j]:w2[1][j + 1]], what
        # the two files of a bin hold the same pairs in the same order
        n1 = [l[1:].split()[0] for l in g1.decode().splitlines() if l.startswith(">")]
        n2 = [l[1:].split()[0] for l in g2.decode().splitlines()[::4]]
        assert sp.pairs_names(n1, n2) == [pairs[r][0].encode() for r in np.nonzero(bins == j)[0]]
    r = subprocess.run([EXE, "-X", "r1.fa", "-x", "r2.fq.gz", "-j", "best", "-Y", str(top), "-f", "bank.txt", "-o", "c"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "split best: 4 bin(s) written, %d pair(s), %d + %d byte(s)" % (len(pairs), len(t1), len(t2)) in r.stdout, r.stdout + r.stderr
    assert tc.both_files(tmp_path, "c") == csvs
    for b in labels:
        assert gunzip(tmp_path / ("c_split_%s_1.fa.gz" % b)) == (tmp_path / ("s_split_%s_1.fa" % b)).read_bytes()
        assert gunzip(tmp_path / ("c_split_%s_2.fq.gz" % b)) == (tmp_path / ("s_split_%s_2.fq" % b)).read_bytes()


@pytest.mark.gpu
def test_65537_short_records_through_the_file_driver(ctx, tmp_path):
    """the batch seam: bins from the rows of two key batches (65 535 records and 2), one split with three bins"""
    import test_classify as tc
    import test_prevalence as tp
    n_rec = 65537
    rng = np.random.default_rng(13)
    refs = [tc.random_bases(rng, 3000) for _ in range(2)]
    seq_of = lambda r: refs[r % 2][(r * 7) % 2960:(r * 7) % 2960 + 40]
    special = {65534: seq_of(65535), 65535: tc.random_bases(rng, 40), 65536: seq_of(65537), 0: tc.random_bases(rng, 40)}   # reference 1, none, reference 1
    seqs = [special.get(r) or seq_of(r) for r in range(n_rec)]
    text = b"".join(b">r%d\n%s\n" % (r, q) for r, q in enumerate(seqs))
    (tmp_path / "many.fa").write_bytes(text)
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, 1.0)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    records, hits = ctx.classify_files(paths, str(tmp_path / "many.fa"), str(tmp_path / "many"), split="best", gz=False)
    assert len(records) == n_rec
    bins, n_bins = sp.split_bins_classify("best", records, hits, 2)
    assert n_bins == 3 and bins[65534] == 1 and bins[65535] == 2 and bins[65536] == 1 and bins[0] == 2   # both sides of the seam
    out, off, rec = sp.records_split(text, bins, n_bins)
    assert min(rec) > 0 and ctx.last_split == {"bins": 3, "records": n_rec, "bytes_out": len(text)}
    for b, label in enumerate(("0", "1", "unmatched")):
        assert (tmp_path / ("many_split_%s.fa" % label)).read_bytes() == out[int(off[b]):int(off[b + 1])]
