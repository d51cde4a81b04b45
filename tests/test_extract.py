"""Extract: the records a record pass calls, written out again as FASTA / FASTQ (spsp_records_extents_host / _device,
spsp_records_extract_host / _device, spsp_extract_flags_classify_host / _taxonomy_host, spsp_extract_plan_host,
spsp_classify_files_extract, spsp_taxonomy_files_extract; bin/comparator -X <records> -F <what> [-u] [-H <lineages>]).

The rule (include/spsp.h, "extract"), as the model below has it -- split and slicing, written from the rule and not from the C:
  FASTA   a line begins at byte 0 and behind every newline; line 0 and every line whose first byte is '>' or 0xFF begins a
          record; record r is text[b_r:b_(r+1)] and the last one ends with the text.
  FASTQ   (the first byte is '@') the content is the text less its trailing "\\r" and "\\n" bytes; its lines are counted, four to
          a record; record r runs from the first byte of line 4r to one past the newline that ends line 4r+3 -- for the last
          record the first newline behind the content, or the content's end where there is none.  A content of 4r + 3 lines
          with something behind that newline has an empty last quality line (the ingest's empty read): the record ends behind
          the tail's second newline, or with the text.
  output  the kept records back to back, verbatim; a kept range that is not empty and does not end in a newline gets one.
Outputs are compared as bytes: there is no tolerance anywhere."""
import gzip
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
NONE = 0xFFFFFFFF


class FormatError(Exception):
    pass


# ---------------------------------------------------------------------------------------------------- the model

def model_begin(text):
    """the records' starts and the last record's end: n_rec + 1 offsets"""
    text = bytes(text)
    n = len(text)
    if n and text[:1] == b"@":
        end = len(text.rstrip(b"\r\n"))
        lines = text[:end].split(b"\n")
        tail = text[end:].split(b"\n")                     # what follows the content, cut at its newlines
        last = end + len(tail[0]) + 1 if len(tail) > 1 else end
        if len(lines) % 4 == 3 and len(tail) > 1 and last < n:   # the empty quality line of a last, empty read is given by the blank tail
            lines.append(b"")
            last = last + len(tail[1]) + 1 if len(tail) > 2 else n
        if len(lines) % 4:
            raise FormatError(len(lines))
        starts = [0] + list(itertools.accumulate(len(x) + 1 for x in lines))[:-1]
        return starts[::4] + [last]
    lines = text.split(b"\n")
    starts = [0] + list(itertools.accumulate(len(x) + 1 for x in lines))[:-1]
    return [0] + [s for s in starts[1:] if s < n and text[s] in (0x3E, 0xFF)] + [n]


def model_extract(text, keep, begin=None):
    text = bytes(text)
    begin = model_begin(text) if begin is None else [int(b) for b in begin]
    assert len(keep) == len(begin) - 1
    parts = []
    for r, k in enumerate(keep):
        part = text[begin[r]:begin[r + 1]]
        if k and part:                                     # (only the last record of a text can lack its newline: only it is looked at)
            parts.append(part + b"\n" if r == len(keep) - 1 and not part.endswith(b"\n") else part)
    return b"".join(parts), sum(1 for k in keep if k)


def model_flags_classify(what, records, hits):
    word, _, j = what.partition("=")
    out = []
    for r in range(len(records)):
        refs = [int(x) for x in hits[r]["reference"][:int(records[r]["listed"])]]
        out.append({"matched": bool(refs), "unmatched": not refs, "best": bool(refs) and refs[0] == int(j or 0), "listed": int(j or 0) in refs}[word])
    return np.array(out, dtype=np.uint8)


def model_flags_taxonomy(what, records, size):
    word, _, t = what.partition("=")
    t = int(t or 0)
    out = []
    for r in range(len(records)):
        node = int(records[r]["node"])
        out.append({"classified": node != NONE, "unclassified": node == NONE, "taxon": node == t,
                    "clade": node != NONE and t <= node < t + int(size[t])}[word])
    return np.array(out, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- texts

def fa_rec(length, name=b"", fill=b"A"):
    """a FASTA record of exactly `length` >= 2 bytes: '>' name, a newline, one line of bases, a newline (no bases: ">...\\n")"""
    assert length >= 2
    if length < len(name) + 3:
        return b">" + name[:length - 2] + b"\n"
    body = length - len(name) - 3
    return b">" + name + b"\n" + (fill * body)[:body] + (b"\n" if length > len(name) + 2 else b"")


def fq_rec(length, rng=None):
    """a well-formed FASTQ record of exactly `length` >= 8 bytes; the quality line may begin with '@' or '>'"""
    assert length >= 8
    s = (length - 6) // 2
    h = length - 6 - 2 * s
    qual = b"@>I#"[(length % 4):(length % 4) + 1] + b"I" * (s - 1) if rng is None else bytes(rng.choice(b"@>I#5") for _ in range(s))
    seq = b"ACGT" * (s // 4 + 1)
    return b"@" + b"h" * h + b"\n" + seq[:s] + b"\n+\n" + qual[:s] + b"\n"


HAND_FASTA = [
    b"",
    b"ACGT\nAC\n",                                         # line 0 is no header: one record all the same
    b"ACGT\n>a\nAC\n",
    b">a\nAC>GT\nA\n>b x>y\nGG\n",                         # '>' in the middle of a line
    b">a\nAC\n\xffb\nGG\n",                                # a 0xFF line
    b">a\n>b\n",
    b">a\r\nAC\r\n>b\r\nGG\r\n",
    b">a\nAC\n>b\nGG",                                     # no final newline
    b"\n",
    b"\n>",
    b">",
    b">a\n\n\n>b\n\n",
]
HAND_FASTQ = [
    b"@r1\nACGT\n+\n@III\n@r2\nAC\n+r2\n>I\n",             # quality lines that begin with '@' and with '>'
    b"@r1\nACGT\n+\nIIII\n\n\r\n\n",                      # a blank tail
    b"@r1\nACGT\n+\nIIII\n@r2\nAC\n+\nII",                 # the last record without its newline
    b"@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nAC\r\n+\r\nII\r\n",
    b"@r1\nACGT\n+\nIIII\r",
    b"@r1\nACGT\n+\nIIII\r\r\n\r\n",
    b"@\n\n+\n\n@\nA\n+\nI\n",                             # empty lines inside the content
    b"@r1\nAC\n+\nII\n@e\n\n+\n\n",                        # a last, empty read: its quality line is the blank tail's
    b"@r1\nAC\n+\nII\n@e\n\n+\n\r\n\n",
    b"@e\n\n+\n\r",
]
HAND_BEGIN = {
    HAND_FASTA[0]: [0, 0], HAND_FASTA[1]: [0, 8], HAND_FASTA[2]: [0, 5, 11], HAND_FASTA[3]: [0, 11, 21], HAND_FASTA[4]: [0, 6, 12],
    HAND_FASTA[5]: [0, 3, 6], HAND_FASTA[6]: [0, 8, 16], HAND_FASTA[7]: [0, 6, 11], HAND_FASTA[8]: [0, 1], HAND_FASTA[9]: [0, 1, 2],
    HAND_FASTA[10]: [0, 1], HAND_FASTA[11]: [0, 5, 9],
    HAND_FASTQ[0]: [0, 16, 30], HAND_FASTQ[1]: [0, 16], HAND_FASTQ[2]: [0, 16, 27], HAND_FASTQ[3]: [0, 20, 36], HAND_FASTQ[4]: [0, 15],
    HAND_FASTQ[5]: [0, 18], HAND_FASTQ[6]: [0, 6, 14], HAND_FASTQ[7]: [0, 12, 19], HAND_FASTQ[8]: [0, 12, 20], HAND_FASTQ[9]: [0, 7],
}


def test_model_on_hand_made_texts():
    for text, want in HAND_BEGIN.items():
        assert model_begin(text) == want, text
    assert set(HAND_BEGIN) == set(HAND_FASTA + HAND_FASTQ)
    assert model_extract(HAND_FASTA[7], [0, 1]) == (b">b\nGG\n", 1)                       # the newline rule
    assert model_extract(HAND_FASTA[7], [1, 0]) == (b">a\nAC\n", 1)
    assert model_extract(HAND_FASTA[3], [1, 1]) == (HAND_FASTA[3], 2)
    assert model_extract(HAND_FASTA[0], [1]) == (b"", 1)
    assert model_extract(HAND_FASTQ[0], [0, 1]) == (b"@r2\nAC\n+r2\n>I\n", 1)
    assert model_extract(HAND_FASTQ[1], [1]) == (b"@r1\nACGT\n+\nIIII\n", 1)              # the blank tail belongs to no record
    assert model_extract(HAND_FASTQ[2], [1, 1]) == (HAND_FASTQ[2] + b"\n", 2)
    assert model_extract(HAND_FASTQ[4], [1]) == (b"@r1\nACGT\n+\nIIII\n", 1)              # (the "\r" of a tail without a newline is tail)
    assert model_extract(HAND_FASTQ[5], [1]) == (b"@r1\nACGT\n+\nIIII\r\r\n", 1)
    for bad in (b"@", b"@r\nAC\n+\n", b"@r\nAC\n+\nII\n@s\n", b"@r\nAC\n+\nII\n\n@s\nA\n+\nI\n"):
        with pytest.raises(FormatError):
            model_begin(bad)


def keep_patterns(n, seed=0):
    rng = random.Random(seed)
    return {"all": [1] * n, "none": [0] * n, "alternating": [r & 1 for r in range(n)], "first": [1] + [0] * (n - 1), "last": [0] * (n - 1) + [1],
            "random": [rng.randrange(2) * rng.randrange(1, 256) for _ in range(n)]}


def sweep_text(seed, fastq, stretch, n_records=160):
    """records of 1 byte .. 3 stretches (FASTQ: from 8 bytes, the shortest record there is), most of them short"""
    rng = random.Random(seed)
    lengths = [rng.choice((rng.randint(2, 9), rng.randint(2, 40), rng.randint(2, 400), rng.randint(2, 400), rng.randint(400, 3 * stretch)))
               for _ in range(n_records)]
    lengths[rng.randrange(n_records)] = 3 * stretch
    if fastq:
        text = b"".join(fq_rec(max(8, n), rng) for n in lengths)
        return text[:-1] if seed & 1 else text + b"\n\r\n" * (seed % 3)
    parts = [b"\n" if seed & 1 else b"A\n"]                # record 0 is line 0 whatever it holds: one byte in the odd seeds
    for n in lengths:
        body = bytes(rng.choice(b"ACGTNacgt>\n\r ") for _ in range(n - 2)).replace(b"\n>", b"\nA").replace(b"\n\xff", b"\nA")
        if body[:1] == b">" or not body:
            body = b"x" + body[1:]
        parts.append(b">" + body[:n - 2] + b"\n" if n > 2 else b">\n")
    text = b"".join(parts)
    return text[:-1] if seed % 3 == 0 else text


# ---------------------------------------------------------------------------------------------------- not GPU

def test_host_extents_and_extract_equal_the_model():
    stretch = sp.extract_plan()["stretch_bytes"]
    texts = HAND_FASTA + HAND_FASTQ + [sweep_text(seed, fastq, stretch, 60) for seed in range(4) for fastq in (False, True)]
    for text in texts:
        begin = model_begin(text)
        assert sp.records_extents(text).tolist() == begin, text[:60]
        for name, keep in keep_patterns(len(begin) - 1, len(text)).items():
            assert sp.records_extract(text, keep) == model_extract(text, keep), (name, text[:60])
    for bad in (b"@", b"@r\nAC\n+\n", b"@r\nAC\n+\nII\n@s\n"):
        with pytest.raises(sp.SpspError) as e:
            sp.records_extents(bad)
        assert e.value.code == sp.ERR_FORMAT and "multiple of four" in str(e.value)
    for begin in ([0, 4, 3], [0, 3, 7]):
        with pytest.raises(sp.SpspError) as e:
            sp.records_extract(b">a\n>b\n", [1, 1], begin)
        assert e.value.code == sp.ERR_ARG


def classify_rows(listed_refs, top):
    records = np.zeros(len(listed_refs), dtype=sp.CLASSIFY_RECORD_DTYPE)
    hits = np.zeros((len(listed_refs), top), dtype=sp.CLASSIFY_HIT_DTYPE)
    for r, refs in enumerate(listed_refs):
        records[r]["listed"] = records[r]["passing"] = len(refs)
        for i, j in enumerate(refs):
            hits[r, i] = (j, 100 - i)
    return records, hits


def test_flag_functions_every_word_at_equality_and_one_off():
    records, hits = classify_rows([[], [3], [4, 3], [0, 4], [0], [2, 0]], 2)              # best= against listed= with top = 2
    for what in ("matched", "unmatched", "best=0", "best=3", "best=4", "best=1", "listed=0", "listed=3", "listed=4", "listed=2", "listed=1"):
        got = sp.extract_flags_classify(what, records, hits, 5)
        assert got.tolist() == model_flags_classify(what, records, hits).tolist(), what
    assert sp.extract_flags_classify("best=3", records, hits, 5).tolist() == [0, 1, 0, 0, 0, 0]
    assert sp.extract_flags_classify("listed=3", records, hits, 5).tolist() == [0, 1, 1, 0, 0, 0]
    assert sp.extract_flags_classify("listed=0", records, hits, 5).tolist() == [0, 0, 0, 1, 1, 1]    # (the zeroed slots of a record without matches name nobody)
    assert sp.extract_flags_classify("best=4", records, hits, 5).tolist() == [0, 0, 1, 0, 0, 0]
    # tree: 0 root [0, 7), 1 [1, 4), 2, 3, 4 [4, 6), 5, 6
    size = np.array([7, 3, 1, 1, 2, 1, 1], dtype=np.uint32)
    tx = np.zeros(8, dtype=sp.TAXONOMY_RECORD_DTYPE)
    tx["node"] = [NONE, 0, 1, 3, 4, 5, 6, 2]
    for what in ("classified", "unclassified") + tuple("%s=%d" % (w, t) for w in ("taxon", "clade") for t in range(7)):
        assert sp.extract_flags_taxonomy(what, tx, size).tolist() == model_flags_taxonomy(what, tx, size).tolist(), what
    for t in (1, 4):                                       # clade=<t> with node = t, t + size[t] - 1, t + size[t]
        edge = np.zeros(4, dtype=sp.TAXONOMY_RECORD_DTYPE)
        edge["node"] = [t - 1, t, t + size[t] - 1, t + size[t]]
        assert sp.extract_flags_taxonomy("clade=%d" % t, edge, size).tolist() == [0, 1, 1, 0]
        assert sp.extract_flags_taxonomy("taxon=%d" % t, edge, size).tolist() == [0, 1, int(size[t] == 1), 0]


def test_flag_functions_refuse_with_the_word_in_the_text():
    records, hits = classify_rows([[], [1]], 2)
    size = np.array([3, 1, 1], dtype=np.uint32)
    tx = np.zeros(2, dtype=sp.TAXONOMY_RECORD_DTYPE)
    unknown = ("", "match", "matchedx", "Matched", "best", "best=", "best=-1", "best= 1", "best=1x", "best=0x1", "best=4294967296", "all", "clade", "taxon=")
    for what in unknown:
        for call in (lambda: sp.extract_flags_classify(what, records, hits, 2), lambda: sp.extract_flags_taxonomy(what, tx, size)):
            with pytest.raises(sp.SpspError) as e:
                call()
            assert e.value.code == sp.ERR_ARG and "'%s'" % what in str(e.value) and "names no records" in str(e.value), what
    for what in ("best=2", "listed=2", "listed=70000"):    # <j> >= n_ref
        with pytest.raises(sp.SpspError) as e:
            sp.extract_flags_classify(what, records, hits, 2)
        assert e.value.code == sp.ERR_ARG and what in str(e.value) and "2 reference(s)" in str(e.value)
    for what in ("taxon=3", "clade=3"):                    # <t> >= n_nodes
        with pytest.raises(sp.SpspError) as e:
            sp.extract_flags_taxonomy(what, tx, size)
        assert e.value.code == sp.ERR_ARG and what in str(e.value) and "3 node(s)" in str(e.value)
    for what in ("classified", "unclassified", "taxon=0", "clade=1"):   # a taxonomy word with classify rows
        with pytest.raises(sp.SpspError) as e:
            sp.extract_flags_classify(what, records, hits, 2)
        assert e.value.code == sp.ERR_ARG and what in str(e.value) and "taxonomy's rows" in str(e.value)
    for what in ("matched", "unmatched", "best=0", "listed=1"):        # and the reverse
        with pytest.raises(sp.SpspError) as e:
            sp.extract_flags_taxonomy(what, tx, size)
        assert e.value.code == sp.ERR_ARG and what in str(e.value) and "classify's rows" in str(e.value)
    with pytest.raises(sp.SpspError) as e:                 # a record that lists more than top
        sp.extract_flags_classify("matched", *classify_rows([[0, 1]], 2)[:1], np.zeros((1, 1), dtype=sp.CLASSIFY_HIT_DTYPE), 2)
    assert e.value.code == sp.ERR_ARG and "top = 1" in str(e.value)


def test_abi_has_the_extract_calls_and_the_plan_is_the_kernels_constants():
    calls = ("spsp_extract_plan_host", "spsp_records_extents_host", "spsp_records_extract_host", "spsp_extract_flags_classify_host",
             "spsp_extract_flags_taxonomy_host", "spsp_extract_word_check_host", "spsp_records_extents_device", "spsp_records_extract_device",
             "spsp_extract_stage_ms", "spsp_classify_files_extract", "spsp_taxonomy_files_extract")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    for name in calls:
        assert hasattr(sp.lib(), name)
    import re
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    value = lambda name: int(re.search(r"constexpr uint32_t %s = (\d+);" % name, text).group(1))
    plan = sp.extract_plan()
    assert plan == {"tile_bytes": value("kExTile"), "stretch_bytes": value("kExStretch")} == {"tile_bytes": 4096, "stretch_bytes": 16384}
    assert plan["stretch_bytes"] % (256 * 16) == 0         # whole rounds of a workgroup's 16-byte stores


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    (tmp_path / "lin.txt").write_text("a\nb\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [(("-F", "matched"), "-F"), (("-u",), "-u"), (("-X", "r.fa", "-u"), "-u"), (("-X", "r.fa", "-F", "classified"), "-F"),
             (("-X", "r.fa", "-F", "clade=1"), "-F"), (("-X", "r.fa", "-H", "lin.txt", "-F", "matched"), "-F"),
             (("-X", "r.fa", "-H", "lin.txt", "-F", "best=0"), "-F"), (("-X", "r.fa", "-F", "everything"), "-F"), (("-X", "r.fa", "-F", "best="), "-F"),
             (("-D", "r.fa", "-F", "matched"), "-F")]
    for args, letter in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1 and letter in r.stdout, (args, r.stdout, r.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
    assert "taxonomy's rows" in run("-X", "r.fa", "-F", "classified", "-f", "list.txt").stdout
    assert "classify's rows" in run("-X", "r.fa", "-H", "lin.txt", "-F", "matched", "-f", "list.txt").stdout
    usage = run().stdout
    assert "-F " in usage and "-u " in usage


def test_host_functions_under_the_sanitizers():
    """tests/tools/extract_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the
    host extents, the host extract, the flag functions and their refusals (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "extract_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "extract_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


class Dev:
    """a text in HBM (16 zero bytes behind it, as the ingest's tests upload theirs)"""

    def __init__(self, text):
        import torch
        self.text = bytes(text)
        self.t = torch.from_numpy(np.frombuffer(self.text + b"\0" * 16, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        self.ptr, self.n = self.t.data_ptr(), len(self.text)


def device_begin(ctx, d):
    d_begin, n_rec = ctx.records_extents_device(d.ptr, d.n)
    return ctx.to_host(d_begin, n_rec + 1, np.uint64).tolist()


def check_text(ctx, text, patterns=("all", "none", "alternating", "first", "last", "random")):
    """the starts and the named keep patterns of one text against the model"""
    d = Dev(text)
    begin = model_begin(text)
    assert device_begin(ctx, d) == begin
    every = keep_patterns(len(begin) - 1, len(text))
    for name in patterns:
        out, kept = ctx.records_extract_device(d.ptr, d.n, every[name])
        assert (out.tobytes(), kept) == model_extract(text, every[name], begin), name
    return d, begin


def plan():
    p = sp.extract_plan()
    return p["tile_bytes"], p["stretch_bytes"]


def seam_texts():
    """name -> text: record starts and lines laid on the tiles' ends (tests 2 and 3 of the issue), by T = tile_bytes"""
    T, _ = plan()
    out = {}
    for at in (T - 1, T, T + 1):                           # a record start at text position `at`
        out["fasta start at T%+d" % (at - T)] = fa_rec(at, b"a") + fa_rec(40, b"b", b"C") + fa_rec(T, b"c", b"G")
    out["fasta newline ends a tile, no header behind it"] = b">a\n" + b"A" * (T - 4) + b"\nACGT\n>c\nGG\n"
    out["fasta 0xFF first in a tile"] = fa_rec(T, b"a") + b"\xffb\nCC\n"
    out["fasta a line of three tiles"] = fa_rec(300, b"a") + b">long\n" + b"G" * (3 * T) + b"\n" + fa_rec(200, b"z") + fa_rec(T // 2, b"y")
    out["fasta 61..65 starts in a tile"] = b"".join(b">\nA\n" * c + b">f\n" + b"A" * (T - 4 * c - 4) + b"\n" for c in (61, 62, 63, 64, 65)) + b">tail"
    out["fasta tiny records"] = b">\n" * (3 * T) + b">x"
    reads = [fq_rec(n) for n in (T // 3, (6 * T) // 10, (12 * T) // 10, (16 * T) // 10, 8, 9, (25 * T) // 10, T, T - 1, T + 1, 31 * T // 10, 10, T // 2)]
    out["fastq records across one, two and three tile ends"] = b"".join(reads)
    out["fastq tiny records"] = fq_rec(8) * (T // 2) + fq_rec(11) * 7
    out["fastq blank tail over a tile end"] = fq_rec(T - 2) + b"\n\r\n\n"
    out["fastq no final newline"] = (fq_rec(100) * 90)[:-1]
    out["fastq one record"] = fq_rec(2 * T)
    return out


def crossed_tile_ends(text, T):
    begin = model_begin(text)
    return {(begin[r + 1] - 1) // T - begin[r] // T for r in range(len(begin) - 1)}


@pytest.mark.gpu
def test_record_count_equals_the_ingests(ctx):
    T, S = plan()
    texts = list(seam_texts().values()) + [sweep_text(3, False, S), sweep_text(2, True, S)] + [t for t in HAND_FASTA if t]
    texts += [HAND_FASTQ[0], HAND_FASTQ[1], HAND_FASTQ[3], HAND_FASTQ[7], HAND_FASTQ[8]]  # (the well-formed ones: the ingest validates)
    for text in texts:
        d = Dev(text)
        _, n_rec = ctx.records_extents_device(d.ptr, d.n)
        clean = ctx.clean_fastq_device if text[:1] == b"@" else ctx.clean_fasta_device
        assert n_rec == clean(d.ptr, d.n)[3] == len(model_begin(text)) - 1, text[:40]
    d_begin, n_rec = ctx.records_extents_device(None, 0)                                  # the empty text: one empty record, as the ingest has it
    assert n_rec == ctx.clean_fasta_device(None, 0)[3] == 1 and ctx.to_host(d_begin, 2, np.uint64).tolist() == [0, 0]
    assert n_rec == len(sp.records_extents(b"")) - 1


@pytest.mark.gpu
def test_starts_on_the_tile_seams(ctx):
    T, _ = plan()
    texts = seam_texts()
    assert {1, 2, 3} <= crossed_tile_ends(texts["fastq records across one, two and three tile ends"], T)
    for name, text in texts.items():
        assert len(text) % T != 0 or name == "fastq one record", name                     # the last tile is partial
        check_text(ctx, text, ("all", "alternating", "last"))
    for bad in (b"@r\nAC\n+\n", fq_rec(T) + b"@s\nAC\n", fq_rec(40) * 7 + b"@s\nAC\n+\nII\n@t"):
        d = Dev(bad)
        with pytest.raises(sp.SpspError) as e:
            ctx.records_extents_device(d.ptr, d.n)
        assert e.value.code == sp.ERR_FORMAT and "multiple of four" in str(e.value)
        with pytest.raises(sp.SpspError) as e:             # the same text with starts made in the extract call
            ctx.records_extract_device(d.ptr, d.n, [1, 1])
        assert e.value.code == sp.ERR_FORMAT


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [1023, 1024, 1025, 4097])
def test_one_record_per_tile_across_the_scans_lanes_and_rounds(ctx, tiles):
    """the composing scan is one workgroup of 1 024 lanes, four tiles a lane: a round covers 4 096 tiles"""
    T, _ = plan()
    text = b"".join(fa_rec(T, b"%d" % i, b"ACGT"[i % 4:i % 4 + 1]) for i in range(tiles))
    assert len(text) == tiles * T
    d, begin = check_text(ctx, text, ("alternating",))
    assert begin == [i * T for i in range(tiles + 1)]
    fq = fq_rec(T) * tiles                                 # and four newlines per tile
    check_text(ctx, fq, ("alternating",))


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [4095, 4096, 4097, 8193])
def test_starts_behind_the_item_scans_rounds(ctx, tiles):
    """the tiles' sums are scanned by one workgroup, 4 096 tiles a round, the rounds in front carried in LDS: a carry dropped or
    doubled shifts every start behind tile 4096 (8192: the third round).  One long sequence line with short records planted in
    the tiles on both sides of the rounds' seams; the starts against numpy ('>' at offset 0 or behind a newline)"""
    T, _ = plan()
    n = tiles * T + 777                                    # whole tiles and a partial last one
    a = np.full(n, ord("A"), dtype=np.uint8)
    a[:3] = np.frombuffer(b">h\n", dtype=np.uint8)
    planted = b"\n>r\nAC\n>s\nG\n>t\n"
    at = sorted({t for t in (0, 4095, 4096, 4097, 8191, 8192, tiles) if t <= tiles})
    for t in at:
        p = t * T + 100
        a[p:p + len(planted)] = np.frombuffer(planted, dtype=np.uint8)
    want = np.flatnonzero((a == ord(">")) & np.concatenate(([True], a[:-1] == ord("\n")))).astype(np.uint64)
    assert len(want) == 1 + 3 * len(at) and sorted(set((want[1:] // T).tolist())) == at
    d = Dev(a.tobytes())
    d_begin, n_rec = ctx.records_extents_device(d.ptr, d.n)
    assert n_rec == len(want)
    assert np.array_equal(ctx.to_host(d_begin, n_rec + 1, np.uint64), np.concatenate((want, np.array([n], dtype=np.uint64))))


@pytest.mark.gpu
def test_the_copy_at_every_alignment_difference(ctx):
    """a dropped first record of 1 .. 16 bytes moves every kept byte by as many: all sixteen differences of source and output
    alignment (16: none)"""
    _, S = plan()
    rest = b"".join(fa_rec(n, b"r%d" % n, b"ACGTTGCA") for n in (5000, 17, 3 * S + 5, 33))
    for drop in range(1, 17):
        first = b"\n" if drop == 1 else b"x" * (drop - 1) + b"\n"
        text = first + rest
        d = Dev(text)
        out, kept = ctx.records_extract_device(d.ptr, d.n, [0, 1, 1, 1, 1])
        assert (out.tobytes(), kept) == (rest, 4), drop
        out, kept = ctx.records_extract_device(d.ptr, d.n, [0, 1, 0, 1, 0])
        assert (out.tobytes(), kept) == model_extract(text, [0, 1, 0, 1, 0]), drop


@pytest.mark.gpu
def test_the_copy_at_the_stretch_seams(ctx):
    _, S = plan()
    for n in (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1):
        # a run that ends at output byte n, another behind it
        text = fa_rec(n, b"a", b"AC") + fa_rec(50, b"drop") + fa_rec(S // 2, b"b", b"GT") + fa_rec(9, b"drop") + fa_rec(n, b"c", b"TTA")
        d = Dev(text)
        for keep in ([1, 0, 1, 0, 1], [1, 0, 0, 0, 0], [0, 0, 1, 0, 1], [1, 1, 1, 1, 1]):
            out, kept = ctx.records_extract_device(d.ptr, d.n, keep)
            assert (out.tobytes(), kept) == model_extract(text, keep), (n, keep)
    for n in (2 * S - 1, 2 * S, 2 * S + 1, 1, 15, 16, 17):  # an output of exactly n bytes: keep all
        text = fa_rec(n - n // 2, b"a") + fa_rec(n // 2, b"b", b"C") if n >= 4 else b"x" * (n - 1) + b"\n"
        assert len(text) == n
        d = Dev(text)
        keep = [1] * (len(model_begin(text)) - 1)
        out, kept = ctx.records_extract_device(d.ptr, d.n, keep)
        assert out.tobytes() == text and kept == len(keep)
    for n in (2 * S - 1, 2 * S, 2 * S + 1):                # ... and with the appended newline as the last of them
        text = fa_rec(n - 1, b"a")[:-1] + b"A"
        d = Dev(text)
        out, kept = ctx.records_extract_device(d.ptr, d.n, [1])
        assert out.tobytes() == text + b"\n" and len(out) == n and kept == 1


@pytest.mark.gpu
def test_stores_made_of_many_runs(ctx):
    """starts handed in: ranges of 1 .. 8 bytes, alternately kept -- with one byte each, every byte of a 16-byte store is a run of
    its own; with eight, a store is made of two"""
    import torch
    rng = random.Random(5)
    text = bytes(rng.choice(b"ACGTN\n>@") for _ in range(40000))
    d = Dev(text)
    for width in (1, 2, 3, 5, 6, 8, None):
        begin, at = [0], 0
        while at < len(text):
            at = min(len(text), at + (width or rng.randint(1, 8)))
            begin.append(at)
        keep = [r & 1 for r in range(len(begin) - 1)]
        d_begin = torch.from_numpy(np.array(begin, dtype=np.uint64).view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        out, kept = ctx.records_extract_device(d.ptr, d.n, keep, d_begin.data_ptr())
        assert (out.tobytes(), kept) == model_extract(text, keep, begin), width
    # starts that decrease or leave the text are refused, and nothing is read outside it
    for begin in ([0, 100, 50, 120], [0, 100, len(text) + 1], [5, 4]):
        d_begin = torch.from_numpy(np.array(begin, dtype=np.uint64).view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        with pytest.raises(sp.SpspError) as e:
            ctx.records_extract_device(d.ptr, d.n, [1] * (len(begin) - 1), d_begin.data_ptr())
        assert e.value.code == sp.ERR_ARG and "d_begin" in str(e.value)


@pytest.mark.gpu
def test_one_long_record_among_two_byte_records(ctx):
    _, S = plan()
    small = 3000
    text = b">\n" * small + fa_rec(40 * S, b"contig", b"ACGTTGCAAC") + b">\n" * small
    d = Dev(text)
    n = 2 * small + 1
    for keep in ([1] * n, [0] * small + [1] + [0] * small, [1] * small + [0] + [1] * small, [r & 1 for r in range(n)], [1 - (r & 1) for r in range(n)]):
        out, kept = ctx.records_extract_device(d.ptr, d.n, keep)
        assert (out.tobytes(), kept) == model_extract(text, keep)


@pytest.mark.gpu
def test_flag_patterns(ctx):
    _, S = plan()
    with_newline = sweep_text(1, False, S, 40)
    without = sweep_text(0, False, S, 40)
    assert with_newline.endswith(b"\n") and not without.endswith(b"\n")
    for text in (with_newline, without, sweep_text(1, True, S, 40), sweep_text(2, True, S, 40)):
        d, begin = check_text(ctx, text)
        n = len(begin) - 1
        out, kept = ctx.records_extract_device(d.ptr, d.n, [1] * n)
        if text[:1] != b"@":
            assert out.tobytes() == (text if text.endswith(b"\n") else text + b"\n")      # keep all: the text, and the newline it lacked
        out, kept = ctx.records_extract_device(d.ptr, d.n, [0] * n)
        assert len(out) == 0 and kept == 0                 # keep none: an empty output from a grid sized by the text
    out, kept = ctx.records_extract_device(None, 0, [1])   # the empty text
    assert len(out) == 0 and kept == 1
    out, kept = ctx.records_extract_device(None, 0, [0])
    assert len(out) == 0 and kept == 0
    d = Dev(b">a\nAC\n")
    with pytest.raises(sp.SpspError) as e:                 # flags for another number of records than the text holds
        ctx.records_extract_device(d.ptr, d.n, [1, 1])
    assert e.value.code == sp.ERR_ARG and "1 record(s)" in str(e.value)


@pytest.mark.gpu
def test_two_calls_on_one_context(ctx):
    _, S = plan()
    big = b"".join(fa_rec(300, b"r%d" % i, b"ACGT"[i % 4:i % 4 + 1]) for i in range(800))
    small = b">s\nTT\n>t\nGG\n>u\nCC"
    d_big, d_small = Dev(big), Dev(small)
    out, kept = ctx.records_extract_device(d_big.ptr, d_big.n, [1] * 800)
    assert out.tobytes() == big and len(big) > 10 * S
    out, kept = ctx.records_extract_device(d_small.ptr, d_small.n, [0, 1, 1])
    assert (out.tobytes(), kept) == (b">t\nGG\n>u\nCC\n", 2)                              # no byte of the first call
    # the starts of an extents call handed back in, twice: the extraction leaves them as they are
    d_begin, n_rec = ctx.records_extents_device(d_big.ptr, d_big.n)
    for keep in ([r % 3 == 0 for r in range(800)], [r % 3 != 0 for r in range(800)]):
        out, kept = ctx.records_extract_device(d_big.ptr, d_big.n, keep, d_begin, n_rec)
        assert (out.tobytes(), kept) == model_extract(big, keep)
    assert ctx.to_host(d_begin, n_rec + 1, np.uint64).tolist() == model_begin(big)
    ctx.timing_enable(True)
    ctx.extract_stage_ms()
    ctx.records_extract_device(d_big.ptr, d_big.n, [1] * 800)
    ms = ctx.extract_stage_ms()
    ctx.timing_enable(False)
    assert set(ms) == {"starts", "offsets", "copy"} and all(v > 0 for v in ms.values()) and sum(ctx.extract_stage_ms().values()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_a_seeded_sweep_against_the_model(ctx, seed):
    _, S = plan()
    for fastq in (False, True):
        text = sweep_text(seed, fastq, S)
        lengths = np.diff(model_begin(text))
        assert lengths.max() >= 3 * S - 1 and lengths.min() <= (8 if fastq else 2)
        check_text(ctx, text, ("random", "alternating"))


# ------------------------------------------------------------------------------------------ files and the command line

def gunzip(path):
    with gzip.open(str(path), "rb") as f:
        return f.read()


@pytest.mark.gpu
def test_classify_files_with_an_extraction_and_the_command_line(ctx, tmp_path):
    import test_classify as tc
    import test_prevalence as tp
    refs, recs = tc.file_case()
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, 1.0)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    texts = {"recs.fa": tc.fasta_of(recs), "recs.fq.gz": tc.fastq_of(recs)}
    (tmp_path / "recs.fa").write_bytes(texts["recs.fa"])
    with gzip.open(str(tmp_path / "recs.fq.gz"), "wb") as f:
        f.write(texts["recs.fq.gz"])
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    cli = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    top = 3
    ctx.classify_files(paths, str(tmp_path / "recs.fq.gz"), str(tmp_path / "plain"), top)
    csvs = tc.both_files(tmp_path, "plain")
    kept_of = {}
    WORDS = ("matched", "unmatched", "best=0", "best=4", "listed=1", "listed=5")
    for i, what in enumerate(WORDS):
        tag = "w%d" % i
        records, hits = ctx.classify_files(paths, str(tmp_path / "recs.fq.gz"), str(tmp_path / tag), top, extract=what)
        keep = model_flags_classify(what, records, hits)
        want, n_kept = model_extract(texts["recs.fq.gz"], keep)
        assert gunzip(tmp_path / (tag + "_extract.fq.gz")) == want and ctx.last_extract == {"n_kept": n_kept, "bytes_out": len(want)}
        assert tc.both_files(tmp_path, tag) == csvs                                       # the CSVs of a run without the word, byte for byte
        assert sp.extract_flags_classify(what, records, hits, len(paths)).tolist() == keep.tolist()
        kept_of[what] = keep
    assert 0 < kept_of["matched"].sum() < len(recs) and (kept_of["matched"] + kept_of["unmatched"] == 1).all()   # the two part the records
    assert kept_of["best=0"].sum() > 0 and kept_of["listed=1"].sum() >= model_flags_classify("best=1", records, hits).sum()
    # what did not match, fed back, matches nothing
    records, hits = ctx.classify_files(paths, str(tmp_path / "w1_extract.fq.gz"), str(tmp_path / "back"), top)
    assert len(records) == kept_of["unmatched"].sum() and (records["listed"] == 0).all()
    # FASTA, plain and gzipped
    records, hits = ctx.classify_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / "fa"), top, extract="matched", gz=False)
    want, _ = model_extract(texts["recs.fa"], model_flags_classify("matched", records, hits))
    assert (tmp_path / "fa_extract.fa").read_bytes() == want and not (tmp_path / "fa_extract.fa.gz").exists()
    # the command line: every word, plain and gzipped in turn, against the library's file for the same word and the plain run's CSVs
    for i, what in enumerate(WORDS):
        tag, plain = "c%d" % i, bool(i & 1)
        name = tag + ("_extract.fq" if plain else "_extract.fq.gz")
        r = cli("-X", "recs.fq.gz", "-F", what, "-Y", str(top), "-f", "bank.txt", "-o", tag, *(["-u"] if plain else []))
        assert r.returncode == 0 and "record(s) kept" in r.stdout, r.stdout + r.stderr
        got = (tmp_path / name).read_bytes() if plain else gunzip(tmp_path / name)
        assert got == gunzip(tmp_path / ("w%d_extract.fq.gz" % i)), what
        assert tc.both_files(tmp_path, tag) == csvs
        assert sorted(f for f in os.listdir(tmp_path) if f.startswith(tag + "_")) == sorted([name, tag + "_classify.csv.gz", tag + "_classify_summary.csv.gz"])
    r = cli("-X", "recs.fa", "-F", "matched", "-u", "-Y", str(top), "-f", "bank.txt", "-o", "cfa")   # FASTA
    assert r.returncode == 0 and (tmp_path / "cfa_extract.fa").read_bytes() == want, r.stdout + r.stderr
    r = cli("-X", "recs.fa", "-F", "listed=6", "-Y", str(top), "-f", "bank.txt", "-o", "no")       # <j> >= n_ref: one line, no device
    assert r.returncode == 1 and "6 reference(s)" in r.stdout.splitlines()[-1] and "failed" not in r.stdout, r.stdout + r.stderr   # (the CLI's own check)
    # refusals write nothing, and come before any file is read
    for what, word in (("listed=6", "6 reference(s)"), ("classified", "taxonomy's rows"), ("most", "names no records")):
        with pytest.raises(sp.SpspError) as e:
            ctx.classify_files(["no such sketch.gz"] * len(paths), str(tmp_path / "none.fa"), str(tmp_path / "no"), top, extract=what)
        assert e.value.code == sp.ERR_ARG and word in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
def test_taxonomy_files_with_an_extraction_and_the_command_line(ctx, tmp_path):
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
    size = sp.taxonomy_lineages(tree.text, len(paths))["size"]
    ctx.taxonomy_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "plain"))
    csvs = tt.both_files(tmp_path, "plain")
    inner = tree.num[("Bacteria", "G1")]
    kept_of = {}
    WORDS = ("classified", "unclassified", "taxon=%d" % inner, "clade=%d" % inner, "clade=0", "taxon=%d" % (len(size) - 1))
    for i, what in enumerate(WORDS):
        tag = "w%d" % i
        records = ctx.taxonomy_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / "lin.txt"), str(tmp_path / tag), extract=what)
        keep = model_flags_taxonomy(what, records, size)
        want, n_kept = model_extract(fasta, keep)
        assert gunzip(tmp_path / (tag + "_extract.fa.gz")) == want and ctx.last_extract == {"n_kept": n_kept, "bytes_out": len(want)}
        assert tt.both_files(tmp_path, tag) == csvs
        kept_of[what] = keep
    assert (kept_of["classified"] + kept_of["unclassified"] == 1).all() and (kept_of["clade=0"] == kept_of["classified"]).all()
    assert kept_of["clade=%d" % inner].sum() > kept_of["taxon=%d" % inner].sum() >= 0 and kept_of["clade=%d" % inner].sum() < kept_of["classified"].sum()
    cli = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    for i, what in enumerate(WORDS):                       # every word with -H, gzipped and plain in turn
        tag, plain = "c%d" % i, bool(i & 1)
        name = tag + ("_extract.fa" if plain else "_extract.fa.gz")
        r = cli("-X", "recs.fa", "-H", "lin.txt", "-F", what, "-f", "bank.txt", "-o", tag, *(["-u"] if plain else []))
        assert r.returncode == 0 and "record(s) kept" in r.stdout, r.stdout + r.stderr
        got = (tmp_path / name).read_bytes() if plain else gunzip(tmp_path / name)
        assert got == gunzip(tmp_path / ("w%d_extract.fa.gz" % i)), what
        assert tt.both_files(tmp_path, tag) == csvs
        assert sorted(f for f in os.listdir(tmp_path) if f.startswith(tag + "_")) == sorted([name, tag + "_taxonomy.csv.gz", tag + "_taxonomy_report.csv.gz"])
    for what, word in (("clade=%d" % len(size), "%d node(s)" % len(size)), ("matched", "classify's rows")):
        with pytest.raises(sp.SpspError) as e:
            ctx.taxonomy_files(["no such sketch.gz"] * len(paths), str(tmp_path / "none.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "no"), extract=what)
        assert e.value.code == sp.ERR_ARG and word in str(e.value)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
def test_65537_short_records_through_the_file_driver(ctx, tmp_path):
    """the batch seam: flags from the rows of two batches (65 535 records and 2), one extraction"""
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
    for what in ("best=1", "unmatched"):
        records, hits = ctx.classify_files(paths, str(tmp_path / "many.fa"), str(tmp_path / "many"), extract=what, gz=False)
        assert len(records) == n_rec
        keep = model_flags_classify(what, records, hits)
        assert keep[65534] != keep[65535] and keep[65535] != keep[65536] and 0 < keep.sum() < n_rec   # both sides of the seam
        want, n_kept = model_extract(text, keep)
        assert (tmp_path / "many_extract.fa").read_bytes() == want and ctx.last_extract == {"n_kept": n_kept, "bytes_out": len(want)}
