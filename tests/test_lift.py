"""Raw coordinates: kept-base positions lifted to positions among the sequence characters of the file the user holds
(spsp_lift_plan_host, spsp_records_lift_host, spsp_segments_bed_host, spsp_records_lift_device, spsp_lift_stage_ms,
spsp_classify_files_raw, spsp_taxonomy_files_raw; bin/comparator -X <records> -y <W> -O [-u]).

The rule (include/spsp.h, "raw coordinates"), as model_lift below has it, written from the rule and not from the C.  A byte is a
sequence character when it is 0x21 .. 0x7e and lies on a FASTA line that does not begin a record (line 0; a first byte '>' or
0xFF) or on line 4r + 1 of a FASTQ text; raw(r, p) counts the sequence characters of record r in front of its kept base p; a
segment [begin, end) has the raw interval [raw(begin), raw(end - 1) + 1).  The host function is held to the model, the device pass to
the host function, on texts stamped by byte position (tests/texts.py).  Every comparison is exact."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
import texts as tx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
CHUNK, WAVE, TILE = 16, 1024, 4096
SCAN_LANE, SCAN_WAVE, SCAN_ROUND = 4, 256, 2048            # tiles a lane, a wave and a round of the lift's one-workgroup scan own
NEW_CALLS = ("spsp_lift_plan_host", "spsp_records_lift_host", "spsp_segments_bed_host", "spsp_records_lift_device", "spsp_lift_stage_ms", "spsp_classify_files_raw",
             "spsp_taxonomy_files_raw")
BASES = b"ACGTacgt"


# ---------------------------------------------------------------------------------------------------- the model

def model_lift(text):
    """-> ([(record, raw) per kept base, in text order], [raw_length per record])"""
    text = bytes(text)
    fastq = text[:1] == b"@"
    lens, out = [0], []
    for i, ln in enumerate(text.split(b"\n")):
        if fastq:
            begins = i % 4 == 0 and ln[:1] not in (b"", b"\r")   # (an empty line 4r, the blank tail's, begins no record)
            data = i % 4 == 1
        else:
            begins = i == 0 or ln[:1] in (b">", b"\xff")
            data = not begins
        if begins and i > 0:
            lens.append(0)
        for c in ln if data else b"":
            if 0x21 <= c <= 0x7E:
                if c in BASES:
                    out.append((len(lens) - 1, lens[-1]))
                lens[-1] += 1
    return out, lens


def clean(seq):
    """the ingest's rule on a string of sequence characters"""
    return bytes(c for c in bytes(seq) if c in BASES).upper()


def host_is_the_model(text, note=None):
    want, lens = model_lift(text)
    raw, rec, raw_length = sp.records_lift(text, np.arange(len(want), dtype=np.uint64))
    assert raw_length.tolist() == lens, note
    assert list(zip(rec.tolist(), raw.tolist())) == want, note
    return want, lens


# ---------------------------------------------------------------------------------------------------- not GPU

def test_abi_holds_the_new_calls_and_the_plan_is_the_ingests_tile():
    L = sp.lib()
    for name in NEW_CALLS:
        assert name in sp.ABI_SYMBOLS and hasattr(L, name), name
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()
    assert "constexpr uint32_t kLfTile = 4096, kLfChunk = 16, kLfThreads = kLfTile / kLfChunk;" in text
    assert sp.lift_plan() == {"tile_bytes": TILE, "chunk_bytes": CHUNK} == sp.Context.lift_plan()
    header = open(os.path.join(ROOT, "include", "spsp.h")).read()
    assert "raw coordinates ---- */" in header and "this pass's limitation" not in header


def seeded_text(rng, fastq, n_rec):
    soup = np.frombuffer(b"ACGTACGTacgtNnRY-* \t", np.uint8)
    run = lambda n: rng.choice(soup, n).tobytes() if n else b""
    t = b""
    for r in range(n_rec):
        if fastq:
            L = int(rng.integers(0, 200))
            t += b"@r%d ACGT\n" % r + run(L) + (b"\r\n" if rng.integers(5) == 0 else b"\n") + b"+\n" + (b">@ACGT" if rng.integers(2) else b"") + run(L) + b"\n"
        else:
            t += (b"\xff" if rng.integers(7) == 0 else b">") + b"r%d ACGT\n" % r
            for _ in range(int(rng.integers(0, 5))):
                t += run(int(rng.integers(0, 90))) + (b"\r\n" if rng.integers(5) == 0 else b"\n")
    if t and rng.integers(2):
        t = t[:-1]
    if fastq and rng.integers(3) == 0:
        t += b"\n\n\r\n"
    return t


@pytest.mark.parametrize("fastq", [False, True])
def test_the_host_function_is_the_model_on_seeded_texts(fastq):
    rng = np.random.default_rng(31 + fastq)
    for i in range(40):
        text = seeded_text(rng, fastq, int(rng.integers(1, 30)))
        want, lens = host_is_the_model(text, i)
        if want:                                            # a sorted sample with repeats
            base = np.sort(rng.integers(0, len(want), 50)).astype(np.uint64)
            raw, rec, _ = sp.records_lift(text, base)
            assert list(zip(rec.tolist(), raw.tolist())) == [want[int(g)] for g in base]


def test_hand_made_fasta_texts():
    # line 0 without '>': a header all the same, its bases are no sequence
    want, lens = host_is_the_model(b"ACGT\nACNGT\n")
    assert want == [(0, 0), (0, 1), (0, 3), (0, 4)] and lens == [5]
    # a 0xFF line begins a record as '>' does
    want, lens = host_is_the_model(b">a\nAC\n\xffb ACGT\nNGT\n")
    assert want == [(0, 0), (0, 1), (1, 1), (1, 2)] and lens == [2, 3]
    # \r\n: the '\r' is not counted
    want, lens = host_is_the_model(b">a\r\nAC\r\nGT\r\n")
    assert [w[1] for w in want] == [0, 1, 2, 3] and lens == [4]
    # blanks and tabs inside a sequence line are not counted; lower case and IUPAC codes are, and '-' and '*'
    want, lens = host_is_the_model(b">a\nA C\tG\nacRYgt-*a\n")
    assert [w[1] for w in want] == [0, 1, 2, 3, 4, 7, 8, 11] and lens == [12]
    # an empty record; a record of Ns alone between two records
    want, lens = host_is_the_model(b">a\nAC\n>empty\n>n\nNNNN\nNN\n>b\nNGNT\n")
    assert want == [(0, 0), (0, 1), (3, 1), (3, 3)] and lens == [2, 0, 6, 4]
    # a text without its last newline; a text that is one header; the empty text is one empty record
    want, lens = host_is_the_model(b">a\nACNNG")
    assert want[-1] == (0, 4) and lens == [5]
    assert host_is_the_model(b">only") == ([], [0]) and host_is_the_model(b"") == ([], [0]) and host_is_the_model(b"\n") == ([], [0])
    # '>' inside a line begins nothing and is counted
    want, lens = host_is_the_model(b">a\nAC>GT\n")
    assert [w[1] for w in want] == [0, 1, 3, 4] and lens == [5]


def test_hand_made_fastq_texts():
    # a quality line that holds ACGT, '>' and '@' (and begins with '@'): no sequence; an N in the sequence line is
    want, lens = host_is_the_model(b"@r0\nACNGT\n+\n@>ACG\n@r1 x\nNNA\n+r1\nACG\n")
    assert want == [(0, 0), (0, 1), (0, 3), (0, 4), (1, 2)] and lens == [5, 3]
    # \r\n, an empty read, no last newline, and the blank tail adds no record
    want, lens = host_is_the_model(b"@r0\r\nAC\r\n+\r\nII\r\n@r1\n\n+\n\n@r2\nnA\n+\nII")
    assert want == [(0, 0), (0, 1), (2, 1)] and lens == [2, 0, 2]
    assert host_is_the_model(b"@r0\nAC\n+\nII\n\n\r\n\n\n\n\n")[1] == [2]
    assert host_is_the_model(b"@")[1] == [0]


def test_every_refusal_of_the_host_function():
    text = b">a\nACGT\n>b\nAC\n"
    with pytest.raises(sp.SpspError, match="must not decrease"):
        sp.records_lift(text, [3, 2])
    with pytest.raises(sp.SpspError, match="not below the 6 bases"):
        sp.records_lift(text, [0, 6])
    with pytest.raises(sp.SpspError, match="not below the 0 bases"):
        sp.records_lift(b">a\nNNN\n", [0])
    with pytest.raises(ValueError):
        sp.records_lift(text, [[0, 1]])
    import ctypes as C
    room, out = C.c_uint32(3), np.zeros(3, np.uint64)       # raw_length with room for another number of records
    assert sp.lib().spsp_records_lift_host(text, len(text), None, 0, None, None, out.ctypes.data, C.byref(room)) != 0 and room.value == 2
    assert "room for 3" in sp.lib().spsp_last_error().decode()
    raw, rec, lens = sp.records_lift(text, [0, 0, 5, 5])    # equal values are allowed
    assert raw.tolist() == [0, 0, 1, 1] and rec.tolist() == [0, 0, 1, 1] and lens.tolist() == [4, 2]


def seg_rows(rows):
    """[(record, segment, begin, end, call, windows, support)] -> SEGMENT_ROW_DTYPE"""
    a = np.zeros(len(rows), dtype=sp.SEGMENT_ROW_DTYPE)
    for i, (r, s, b, e, c, w, u) in enumerate(rows):
        a[i]["record"], a[i]["segment"], a[i]["begin"], a[i]["end"], a[i]["call"], a[i]["windows"], a[i]["support"] = r, s, b, e, c, w, u
    return a


def model_bed(segs, raw_begin, raw_end, names, call_names, last_name):
    out = []
    for g, rb, re in zip(segs, raw_begin, raw_end):
        if g["end"] > g["begin"]:
            call = (list(call_names) + [last_name])[int(g["call"])].replace("\t", " ")
            out.append("\t".join([names[int(g["record"])], str(int(rb)), str(int(re)), call, "0", ".", str(int(g["segment"])), str(int(g["begin"])), str(int(g["end"])),
                                  str(int(g["windows"])), str(int(g["support"]))]) + "\n")
    return "".join(out).encode()


def test_the_bed_text_to_the_byte():
    segs = seg_rows([(0, 0, 0, 10, 0, 2, 3), (1, 0, 0, 0, 2, 1, 0), (2, 0, 10, 30, 1, 4, 0), (2, 1, 30, 31, 2, 1, 7)])
    names, calls = ["chr1", "empty", "chr2"], ["ref A", "ref\tB"]
    text = sp.segments_bed(segs, [3, 0, 17, 44], [15, 0, 40, 45], names, calls, "unmatched")
    assert text == b"chr1\t3\t15\tref A\t0\t.\t0\t0\t10\t2\t3\nchr2\t17\t40\tref B\t0\t.\t0\t10\t30\t4\t0\nchr2\t44\t45\tunmatched\t0\t.\t1\t30\t31\t1\t7\n"
    assert text == model_bed(segs, [3, 0, 17, 44], [15, 0, 40, 45], names, calls, "unmatched")
    assert sp.segments_bed(segs[:0], [], [], [], calls, "unmatched") == b""
    with pytest.raises(sp.SpspError, match="shorter"):     # a raw interval holds at least the segment's bases
        sp.segments_bed(segs, [3, 0, 17, 44], [12, 0, 40, 45], names, calls, "unmatched")
    with pytest.raises(sp.SpspError, match="out of range"):
        sp.segments_bed(segs, [3, 0, 17, 44], [15, 0, 40, 45], names[:2], calls, "unmatched")
    with pytest.raises(ValueError):
        sp.segments_bed(segs, [3, 0, 17], [15, 0, 40, 45], names, calls, "unmatched")


def test_the_command_line_refuses_o_without_y_and_keeps_the_old_u_lines(tmp_path):
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    (tmp_path / "bank.txt").write_text("a.sk.gz\nb.sk.gz\n")
    for args in (("-X", "r.fa", "-O"), ("-X", "r.fa", "-O", "-u"), ("-O",)):
        r = run(*args, "-f", "bank.txt", "-o", "no")
        lines = [x for x in r.stdout.strip().splitlines() if x.startswith("-")]
        assert r.returncode == 1 and lines == ["-O writes the segments of -y <W> in the coordinates of the records file as BED: it needs -y"], (args, r.stdout)
    r = run("-X", "r.fa", "-u", "-f", "bank.txt", "-o", "no")   # the old line, to the letter
    assert r.returncode == 1 and r.stdout.strip() == "-u writes the records of -F plain instead of gzipped: it needs -F"
    r = run("-X", "r.fa", "-y", "100", "-O", "-u", "-f", "bank.txt", "-o", "no")   # accepted: it fails on the files that are not there
    assert r.returncode == 1 and "-u writes" not in r.stdout and "it needs -y" not in r.stdout
    assert sorted(os.listdir(tmp_path)) == ["bank.txt"]
    usage = run().stdout
    assert "-O With -y" in usage and "-u Write the records of -F, or the files of -j, plain, not gzipped" in usage


def test_host_functions_under_the_sanitizers():
    """tests/tools/lift_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the lift
    as plain loops, its refusals, the BED text and the plan (CPU only: nothing is preloaded)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "lift_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "lift_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU: the pass

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def on_device(text):
    import torch
    d = torch.from_numpy(np.concatenate([np.frombuffer(bytes(text), np.uint8), np.zeros(64, np.uint8)])).cuda()
    torch.cuda.synchronize()
    return d


def lift_check(ctx, text, base=None, note=None):
    """the device pass against spsp_records_lift_host: every kept base where no indices are given.  -> (raw, rec, raw_length)"""
    text = bytes(text)
    n_bases = int(tx.survivors(text, text[:1] == b"@").sum())   # (a third account of what the ingest keeps)
    base = np.arange(n_bases, dtype=np.uint64) if base is None else np.asarray(base, dtype=np.uint64)
    want = sp.records_lift(text, base)
    d = on_device(text)
    got = ctx.records_lift_device(d.data_ptr(), len(text), n_bases, base, n_rec=len(want[2]))
    assert ctx.last_lift_records == len(want[2]), note
    for g, w, what in zip(got, want, ("raw", "rec", "raw_length")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (note, what, np.flatnonzero(g != w)[:5] if len(g) == len(w) else (len(g), len(w)))
    if text[:1] != b"@" or tx.fastq_verdict(text) is None:   # without n_rec the extraction counts the records first (it refuses a malformed FASTQ)
        again = ctx.records_lift_device(d.data_ptr(), len(text), n_bases, base)
        assert all(np.array_equal(g, w) for g, w in zip(again, want)), note
    return want


def fasta_soup(n, seed, line=0):
    """a soup with '>' on byte 0 and the first header's newline on byte 9; line: a newline every that many bytes behind it"""
    buf = tx.soup(n, seed)
    tx.header(buf, 0, 10)
    if line:
        a = np.frombuffer(buf, dtype=np.uint8)
        a[10 + line - 1::line] = 10
    return buf


@pytest.mark.gpu
def test_every_kept_base_of_a_three_tile_text(ctx):
    buf = fasta_soup(3 * TILE - 5, 1, line=61)
    for at in (700, 4090, 9000):
        tx.header(buf, at, at + 23)
    tx.header(buf, 5000, 5040, first=b"\xff")
    raw, rec, lens = lift_check(ctx, buf)
    assert len(lens) == 5 and len(raw) > 2 * TILE and int(rec[-1]) == 4 and int(raw[-1]) > int((rec == 4).sum()) - 1   # (other characters among the bases)


@pytest.mark.gpu
def test_the_16_byte_chunk(ctx):
    # a kept base on byte 0 and on byte 15 of a chunk, alone among Ns
    buf = fasta_soup(2 * TILE, 2)
    tx.put(buf, 512, b"N" * 64)
    tx.put(buf, 528, b"A")
    tx.put(buf, 528 + 15, b"c")
    lift_check(ctx, buf, note="bytes 0 and 15")
    # an N run across the chunk seam, from every byte of the chunk in front
    for start in range(16):
        buf = fasta_soup(TILE + 300, 3)
        tx.put(buf, 1024 + start, b"N" * 17)
        lift_check(ctx, buf, note=("N run", start))
    # a text whose length is 1 .. 15 past a multiple of 16, with and without a newline as its last byte
    for r in range(1, 16):
        for last in (b"", b"\n"):
            buf = fasta_soup(TILE + 48 + r, 4 + r, line=70)
            if last:
                tx.put(buf, len(buf) - 1, last)
            lift_check(ctx, buf, note=("length", r, last))


@pytest.mark.gpu
def test_the_wave_and_the_tile_seam(ctx):
    for seam in (WAVE, TILE, 2 * TILE):
        # a kept base on the last byte in front of the seam and on the first behind it, Ns around them
        buf = fasta_soup(3 * TILE, 5)
        tx.put(buf, seam - 8, b"NNNNNNNAcNNNNNNN")
        lift_check(ctx, buf, note=("bases at", seam))
        # an N run across the seam
        buf = fasta_soup(3 * TILE, 6)
        tx.put(buf, seam - 20, b"N" * 45)
        lift_check(ctx, buf, note=("N run at", seam))
        # '\n' on the last byte in front of the seam; the next line a header (a record that begins on the tile's byte 0), or data
        for first in (b">", b"\xff", None):
            buf = fasta_soup(3 * TILE, 7)
            tx.put(buf, seam - 1, b"\n")
            if first:
                tx.put(buf, seam, first)
                tx.put(buf, seam + 40, b"\n")
            raw, rec, lens = lift_check(ctx, buf, note=("newline at", seam, first))
            assert len(lens) == (2 if first else 1)
        # a header line across the seam
        buf = fasta_soup(3 * TILE, 8)
        tx.header(buf, seam - 30, seam + 30)
        lift_check(ctx, buf, note=("header across", seam))


@pytest.mark.gpu
def test_tiles_that_hold_nothing_to_count(ctx):
    # a header of 5 KiB: tile 1 is all header, and its line state is what tile 0 leaves
    buf = fasta_soup(4 * TILE, 9, line=80)
    tx.header(buf, TILE - 500, TILE - 500 + 5 * 1024)
    buf[TILE - 499:TILE - 501 + 5 * 1024] = bytes(buf[TILE - 499:TILE - 501 + 5 * 1024]).replace(b"\n", b"A")   # (one line)
    raw, rec, lens = lift_check(ctx, buf, note="a tile that is all header")
    assert len(lens) == 2
    # one tile, and two consecutive tiles, without a kept base (Ns: sequence characters all the same) between two tiles with queries
    for n_empty in (1, 2):
        buf = fasta_soup((2 + n_empty) * TILE + 100, 10 + n_empty)
        tx.put(buf, TILE, b"N" * (n_empty * TILE))
        raw, rec, lens = lift_check(ctx, buf, note=("tiles without a kept base", n_empty))
        assert (np.diff(raw.astype(np.int64)) > n_empty * TILE).sum() == 1
        # ... and with only the two queries on either side of them
        n_front = int(tx.survivors(bytes(buf[:TILE])).sum())
        lift_check(ctx, buf, base=[n_front - 1, n_front], note=("two queries around", n_empty))
    # a tile with no sequence character: blanks
    buf = fasta_soup(3 * TILE, 13)
    tx.put(buf, TILE, b" " * TILE)
    raw, rec, lens = lift_check(ctx, buf, note="a tile of blanks")
    assert int(lens[0]) == 2 * TILE - 10
    # a tile of newlines, and a text that is one tile of header and nothing else
    buf = fasta_soup(3 * TILE, 14)
    tx.put(buf, TILE, b"\n" * TILE)
    lift_check(ctx, buf, note="a tile of newlines")
    lift_check(ctx, b">" + bytes(tx.soup(TILE - 1, 15)), note="one tile of header")


@pytest.mark.gpu
def test_fastq_at_the_tile_seam(ctx):
    # '\n' on a tile's last byte for each of the four line phases
    for role in range(4):
        for crlf in (False, True):
            f = tx.Fastq(3 * TILE, 20 + role, crlf=crlf)
            f.fill(TILE - 1)
            f.land(role, TILE - 1)
            f.fill(3 * TILE - 400)
            text = f.text()
            assert text[TILE - 1:TILE] == b"\n" and tx.fastq_verdict(text) is None
            raw, rec, lens = lift_check(ctx, text, note=("phase", role, crlf))
            assert len(lens) == f.n_rec
    # a read across the seam; the text with and without its last newline, and with a blank tail
    f = tx.Fastq(3 * TILE, 30)
    f.fill(TILE - 200)
    f.record(5, 700)
    f.fill(2 * TILE - 100)
    f.record(5, 300)
    for text in (f.text(), f.text(final_newline=False), f.text() + b"\n\r\n\n"):
        raw, rec, lens = lift_check(ctx, text, note="a read across the seam")
        assert len(lens) == f.n_rec and 700 in lens.tolist()


def big_text(n_tiles, seed, fastq):
    """n_tiles tiles less a few bytes; FASTA: lines of 80, a header across every tile boundary the scan cuts at"""
    n = n_tiles * TILE - 7
    if fastq:
        f = tx.Fastq(n + 800, seed)
        f.fill(n, room=0)
        left = n - f.at                                     # the last read takes up what is left: h + s + 1 + s and four newlines
        s = (left - 9) // 2
        f.record(left - 5 - 2 * s, s)
        assert f.at == n
        return f.text()
    buf = fasta_soup(n, seed, line=80)
    for t in (SCAN_LANE, SCAN_WAVE, SCAN_ROUND):
        for at in (t - 1, t, t + 1):
            if at * TILE + 60 < n:
                tx.header(buf, at * TILE - 40, at * TILE + 40)
    return bytes(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("fastq", [False, True])
@pytest.mark.parametrize("cut", [SCAN_LANE, SCAN_WAVE, SCAN_ROUND])
def test_tile_counts_on_either_side_of_every_boundary_of_the_scan(ctx, cut, fastq):
    rng = np.random.default_rng(40)
    for n_tiles in (cut - 1, cut, cut + 1):
        text = big_text(n_tiles, 41 + n_tiles, fastq)
        assert (len(text) + TILE - 1) // TILE == n_tiles
        n_bases = int(tx.survivors(text, fastq).sum())
        base = np.unique(np.concatenate([[0, n_bases - 1], rng.integers(0, n_bases, 2000)]))
        lift_check(ctx, text, base=base, note=(n_tiles, fastq))


@pytest.mark.gpu
def test_the_queries(ctx):
    buf = fasta_soup(40 * TILE, 50, line=70)
    for at in range(3000, 40 * TILE - 100, 9973):
        tx.header(buf, at, at + 31)
    text = bytes(buf[:-3])                                  # no final newline: the last byte is soup
    n_bases = int(tx.survivors(text).sum())
    assert tx.survivors(text)[-20:].any()
    lift_check(ctx, text, base=[], note="none")
    for g in (0, 1, n_bases // 2, n_bases - 1):
        lift_check(ctx, text, base=[g], note=("one", g))
    lift_check(ctx, text, base=[0, n_bases - 1], note="only the first and the last kept base of a 40-tile text")
    lift_check(ctx, text, base=[12345] * 300, note="300 equal ones into one chunk")
    per_tile = int(tx.survivors(text[:TILE]).sum())
    assert per_tile > 1024
    lift_check(ctx, text, base=np.arange(per_tile + 50), note="more queries in one tile than the workgroup has lanes")
    lift_check(ctx, text, base=np.repeat(np.arange(5 * per_tile, 5 * per_tile + 700), 3), note="repeats across a tile")
    d = on_device(text)                                     # nothing asked: nothing launched, no record counted (the C call itself: the
    import ctypes as C                                      # Python call always asks for the lengths)
    ctx.timing_enable(True)
    try:
        ctx.lift_stage_ms()
        n_rec = C.c_uint32(7)
        assert sp.lib().spsp_records_lift_device(ctx._h, d.data_ptr(), len(text), n_bases, None, 0, None, None, None, C.byref(n_rec)) == 0
        assert n_rec.value == 0 and set(ctx.lift_stage_ms().values()) == {0.0}
        raw, rec, lens = ctx.records_lift_device(d.data_ptr(), len(text), n_bases, [], n_rec=len(model_lift(text)[1]))   # ... unless the lengths are
        assert len(raw) == 0 and lens.tolist() == model_lift(text)[1] and min(ctx.lift_stage_ms().values()) > 0.0
    finally:
        ctx.timing_enable(False)


@pytest.mark.gpu
def test_the_refusals_and_where_they_fall(ctx):
    text = bytes(fasta_soup(2 * TILE + 77, 60, line=60))
    n_bases = int(tx.survivors(text).sum())
    d = on_device(text)
    ctx.timing_enable(True)
    try:
        ctx.lift_stage_ms()
        before = (("must not decrease", dict(n_bases=n_bases, base=[5, 4])), ("without bases", dict(n_bases=0, base=[0])),
                  ("16-byte aligned", dict(n_bases=n_bases, base=[0], shift=1)), ("1 or more", dict(n_bases=n_bases, base=[0], n_rec=0)))   # (n_rec: the room of the lengths)
        for word, kw in before:                                 # refused before any launch: no stage has run
            with pytest.raises(sp.SpspError, match=word):
                ctx.records_lift_device(d.data_ptr() + kw.get("shift", 0), len(text) - kw.get("shift", 0), kw["n_bases"], kw["base"], n_rec=kw.get("n_rec", 1))
            assert set(ctx.lift_stage_ms().values()) == {0.0}, word
        behind = (("not below", dict(n_bases=n_bases, base=[0, n_bases])), ("kept base", dict(n_bases=n_bases - 1, base=[0])), ("kept base", dict(n_bases=n_bases + 1, base=[0])),
                  ("room for 2", dict(n_bases=n_bases, base=[0], n_rec=2)))
        for word, kw in behind:                                 # refused behind the wait: the pass's own counts say so
            with pytest.raises(sp.SpspError, match=word):
                ctx.records_lift_device(d.data_ptr(), len(text), kw["n_bases"], kw["base"], n_rec=kw.get("n_rec", 1))
            assert min(ctx.lift_stage_ms().values()) > 0.0, word
    finally:
        ctx.timing_enable(False)
    with pytest.raises(sp.SpspError, match="NULL"):
        ctx.records_lift_device(None, len(text), n_bases, [0])
    lift_check(ctx, text, note="the context answers as before")


@pytest.mark.gpu
def test_three_calls_on_one_context_small_large_small(ctx):
    small = bytes(fasta_soup(700, 70, line=50))
    large = big_text(300, 71, False)
    for text in (small, large, small, b">x\nA", b""):
        lift_check(ctx, text, note=len(text))


@pytest.mark.gpu
@pytest.mark.parametrize("fastq", [False, True])
def test_a_seeded_sweep(ctx, fastq):
    rng = np.random.default_rng(80 + fastq)
    for i in range(12):
        text = seeded_text(rng, fastq, int(rng.integers(1, 400)))
        want, lens = model_lift(text)
        if i % 3 == 0 or not want:
            lift_check(ctx, text, note=(fastq, i))
        else:
            lift_check(ctx, text, base=np.sort(rng.integers(0, len(want), int(rng.integers(1, 3000)))), note=(fastq, i))


# ---------------------------------------------------------------------------------------------------- GPU: end to end

def gunzip(path):
    return gzip.decompress(open(path, "rb").read())


def fa_bodies(text):
    """the -Z text -> [(header, body without newlines)]"""
    return [(rec.partition(b"\n")[0], rec.partition(b"\n")[2].replace(b"\n", b"")) for rec in text.split(b">")[1:]]


def raw_is_right(lw, seqs):
    """seqs: per record its sequence characters.  Every segment with bases: the cleaned raw interval is the segment's kept bases, it
    starts and ends on a base, and it ends in front of the next one's begin"""
    last = {}
    for g, rb, re in zip(lw["segments"], lw["raw_begin"].tolist(), lw["raw_end"].tolist()):
        r, b, e = int(g["record"]), int(g["begin"]), int(g["end"])
        if e == b:
            assert (rb, re) == (0, 0)
            continue
        seq = seqs[r]
        assert clean(seq[rb:re]) == clean(seq)[b:e] and seq[rb] in BASES and seq[re - 1] in BASES and re <= len(seq)
        assert last.get(r, 0) <= rb
        last[r] = re


CSVS = ("_segments.csv.gz", "_mosaic.csv.gz")


@pytest.fixture(scope="module")
def genomes(ctx, tmp_path_factory):
    """two synthetic 20 kbp genomes, sketched as two references"""
    import test_prevalence as tp
    import test_segments as ts
    root = tmp_path_factory.mktemp("lift_genomes")
    rng = np.random.default_rng(19)
    g = [ts.random_bases(rng, 20000) for _ in range(2)]
    return root, g, tp.write_files(root, [ctx.sketch_text(b">g%d\n" % i + x + b"\n", ts.K, ts.M, 1.0)[0] for i, x in enumerate(g)])


@pytest.fixture(scope="module")
def small_bank(ctx, tmp_path_factory):
    """test_classify's file_case: three random 3 kbp references, sketched at rate 1"""
    import test_classify as tc
    import test_prevalence as tp
    import test_segments as ts
    root = tmp_path_factory.mktemp("lift_bank")
    refs, _ = tc.file_case()
    return refs, tp.write_files(root, [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", ts.K, ts.M, 1.0)[0] for i, g in enumerate(refs)])


@pytest.mark.gpu
def test_without_ns_the_raw_interval_is_the_kept_one_and_nothing_else_changes(ctx, small_bank, tmp_path):
    import test_segments as ts
    refs, paths = small_bank
    W = 300
    recs = ts.text_case(refs, W, 5)
    (tmp_path / "t.fa").write_bytes(ts.fasta(recs))
    args = (paths, str(tmp_path / "t.fa"))
    rows0, hits0 = ctx.classify_files(*args, str(tmp_path / "plain"), 2, 2, 1, 2, window=W, smooth=1, segments="all")
    seg0 = ctx.last_windows["segments"]
    assert "raw_begin" not in ctx.last_windows and not os.path.exists(tmp_path / "plain_segments.bed.gz")
    rows, hits = ctx.classify_files(*args, str(tmp_path / "raw"), 2, 2, 1, 2, window=W, smooth=1, segments="all", raw=True)
    lw = ctx.last_windows
    assert np.array_equal(rows, rows0) and np.array_equal(hits, hits0) and np.array_equal(lw["segments"], seg0)
    for suf in CSVS + ("_segments.fa.gz",):                 # both CSVs and the -Z text are those of the run without raw, byte for byte
        assert open(tmp_path / ("raw" + suf), "rb").read() == open(tmp_path / ("plain" + suf), "rb").read()
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("raw_")) == ["raw_mosaic.csv.gz", "raw_segments.bed.gz", "raw_segments.csv.gz", "raw_segments.fa.gz"]
    has = seg0["end"] > seg0["begin"]
    assert has.sum() == len(seg0) - 1                       # (the empty record's segment has no raw interval)
    assert np.array_equal(lw["raw_begin"][has], seg0["begin"][has]) and np.array_equal(lw["raw_end"][has], seg0["end"][has])
    assert not lw["raw_begin"][~has].any() and not lw["raw_end"][~has].any()
    raw_is_right(lw, [s for _, s in recs])
    names = [n.decode() for n, _ in recs]
    bed = gunzip(tmp_path / "raw_segments.bed.gz")
    assert bed == sp.segments_bed(seg0, lw["raw_begin"], lw["raw_end"], names, paths, "unmatched") == model_bed(seg0, lw["raw_begin"], lw["raw_end"], names, paths, "unmatched")
    assert lw["bed_bytes"] == len(bed) and bed.count(b"\n") == has.sum()
    # raw without a -Z word; the command line writes the same BED, gzipped and plain, and one more line of chatter
    ctx.classify_files(*args, str(tmp_path / "noz"), 2, 2, 1, 2, window=W, smooth=1, raw=True)
    assert gunzip(tmp_path / "noz_segments.bed.gz") == bed and not os.path.exists(tmp_path / "noz_segments.fa.gz")
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    for extra, name in ((["-u"], "cli_segments.bed"), ([], "cli_segments.bed.gz")):
        r = subprocess.run([EXE, "-X", "t.fa", "-y", str(W), "-Q", "1", "-O", "-f", "bank.txt", "-o", "cli", "-I", "0.5", "-V", "2"] + extra, cwd=tmp_path, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0 and "raw coordinates: %d segment(s) lifted, their raw intervals 0 base(s) longer than the kept ones" % has.sum() in r.stdout, r.stdout
        got = open(tmp_path / name, "rb").read()
        assert (got if extra else gzip.decompress(got)) == bed
        for suf in CSVS:
            assert gunzip(tmp_path / ("cli" + suf)) == gunzip(tmp_path / ("raw" + suf))
    with pytest.raises(ValueError, match="window"):
        ctx.classify_files(*args, str(tmp_path / "no"), raw=True)


@pytest.mark.gpu
def test_a_scaffold_of_two_genomes_joined_by_ns(ctx, genomes):
    root, g, paths = genomes
    W = 1000
    first = g[0][:3000] + b"N" * 37 + g[0][3000:9000] + g[0][9000:9500].lower() + b"N" * 250 + g[0][9500:]
    seq = first + b"N" * 100 + g[1]
    junction = len(first) + 100                             # where the second genome begins, in RAW coordinates
    (root / "scaffold.fa").write_bytes(b">scaffold two genomes\n" + b"".join(seq[i:i + 60] + b"\n" for i in range(0, len(seq), 60)))
    ctx.classify_files(paths, str(root / "scaffold.fa"), str(root / "plain"), window=W, segments="all")
    ctx.classify_files(paths, str(root / "scaffold.fa"), str(root / "s"), window=W, segments="all", raw=True)
    lw = ctx.last_windows
    seg = lw["segments"]
    for suf in CSVS + ("_segments.fa.gz",):
        assert open(root / ("s" + suf), "rb").read() == open(root / ("plain" + suf), "rb").read()
    raw_is_right(lw, [seq])
    bodies = fa_bodies(gunzip(root / "s_segments.fa.gz"))   # clean(seq[raw_begin:raw_end]) is the segment's -Z all body
    assert len(bodies) == len(seg)
    for (head, body), rb, re in zip(bodies, lw["raw_begin"].tolist(), lw["raw_end"].tolist()):
        assert clean(seq[rb:re]) == body
    assert seg["call"].tolist() == [0, 1]
    # the boundary between the two calls lies within one window of the junction in RAW coordinates; the kept ones are off by the Ns
    rb1 = int(lw["raw_begin"][1])
    assert abs(rb1 - junction) <= W and rb1 - int(seg["begin"][1]) == seq[:rb1].count(b"N") >= 37 + 250
    assert int(lw["raw_end"][0]) <= int(lw["raw_begin"][1]) and int(lw["raw_begin"][0]) == 0 and int(lw["raw_end"][1]) == len(seq)
    bed = gunzip(root / "s_segments.bed.gz").decode().splitlines()
    assert [x.split("\t")[:3] for x in bed] == [["scaffold", str(int(b)), str(int(e))] for b, e in zip(lw["raw_begin"], lw["raw_end"])]


@pytest.mark.gpu
def test_taxonomy_files_and_fastq_input_with_ns(ctx, small_bank, tmp_path):
    import test_segments as ts
    import test_taxonomy as tt
    refs, paths = small_bank
    W = 300
    recs = ts.text_case(refs, W, 7)
    recs[3] = (recs[3][0], recs[3][1][:50] + b"NNNNN" + recs[3][1][50:120].lower() + b"RY" + recs[3][1][120:])
    tree = tt.Tree(tt.file_lineages())
    (tmp_path / "t.fa").write_bytes(ts.fasta(recs))
    (tmp_path / "lin.txt").write_text(tree.text)
    lin = sp.taxonomy_lineages(tree.text, len(paths))
    targs = (paths, str(tmp_path / "t.fa"), str(tmp_path / "lin.txt"))
    rows0 = ctx.taxonomy_files(*targs, str(tmp_path / "plain"), 2, 1, 2, window=W, segments="all")
    rows = ctx.taxonomy_files(*targs, str(tmp_path / "tax"), 2, 1, 2, window=W, segments="all", raw=True)
    lw = ctx.last_windows
    assert np.array_equal(rows, rows0)
    for suf in CSVS + ("_segments.fa.gz",):
        assert open(tmp_path / ("tax" + suf), "rb").read() == open(tmp_path / ("plain" + suf), "rb").read()
    raw_is_right(lw, [s for _, s in recs])
    names = [n.decode() for n, _ in recs]
    assert gunzip(tmp_path / "tax_segments.bed.gz") == model_bed(lw["segments"], lw["raw_begin"], lw["raw_end"], names, list(lin["names"]), "unclassified")
    assert (lw["raw_end"] - lw["raw_begin"] > lw["segments"]["end"] - lw["segments"]["begin"]).any()
    # FASTQ input with Ns: the raw positions count the read's sequence line, qualities and headers are nothing
    reads = [(b"read%d extra words" % i, s) for i, (_, s) in enumerate(recs) if s]
    reads[1] = (reads[1][0], reads[1][1][:40].lower() + b"NNN" + reads[1][1][40:])
    reads[2] = (reads[2][0], b"NN" + reads[2][1] + b"N")
    (tmp_path / "t.fq").write_bytes(b"".join(b"@" + n + b"\n" + q + b"\n+\n" + b"A" * len(q) + b"\n" for n, q in reads))
    ctx.classify_files(paths, str(tmp_path / "t.fq"), str(tmp_path / "fq"), 2, 2, 1, 2, window=W, raw=True, gz=False)
    lw = ctx.last_windows
    raw_is_right(lw, [q for _, q in reads])
    assert open(tmp_path / "fq_segments.bed", "rb").read() == model_bed(lw["segments"], lw["raw_begin"], lw["raw_end"], [n.split()[0].decode() for n, _ in reads], paths, "unmatched")
    first_of_2 = [i for i, g in enumerate(lw["segments"]) if g["record"] == 2][0]
    assert int(lw["raw_begin"][first_of_2]) == 2 and not os.path.exists(tmp_path / "fq_segments.bed.gz")
