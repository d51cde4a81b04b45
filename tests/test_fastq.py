"""FASTQ read sets (GPU): a text whose first byte is '@' is read as four-line FASTQ records.  The expected value is always
the CPU oracle applied to F(T), the FASTA text that holds ">" + header[1:] + "\\n" + seq + "\\n" for every record of T."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
from oracle import oracle_py as orc
from supersampler_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def fastq_to_fasta(text):
    """F(T): one FASTA record per FASTQ record (header without its '@', the sequence line as it stands)."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    while lines and lines[-1].rstrip(b"\r") == b"":
        lines.pop()
    while len(lines) % 4:                    # a blank quality line of an empty last read
        lines.append(b"")
    out = []
    for i in range(0, len(lines), 4):
        assert lines[i][:1] == b"@" and lines[i + 2][:1] == b"+"
        out.append(b">" + lines[i][1:] + b"\n" + lines[i + 1] + b"\n")
    return b"".join(out)


def fastq(records, crlf=False, final_newline=True):
    """records: (name, seq, qual or None) -> FASTQ bytes (qual None: a run of 'I' as long as seq without its '\\r')"""
    nl = b"\r\n" if crlf else b"\n"
    parts = []
    for name, seq, qual in records:
        if qual is None:
            qual = b"I" * len(seq)
        parts.append(b"@" + name + nl + seq + nl + b"+" + nl + qual + nl)
    t = b"".join(parts)
    return t if final_newline else t[:-len(nl)]


def simulate_reads(rng, genome, coverage, read_len, err):
    """reads sampled from both strands of `genome` with substitutions at rate err"""
    n = int(len(genome) * coverage / read_len)
    starts = rng.integers(0, len(genome) - read_len, size=n)
    recs = []
    for i, a in enumerate(starts):
        r = genome[a:a + read_len].copy()
        flip = rng.random(read_len) < err
        r[flip] = synth.random_genome(rng, int(flip.sum()))
        s = r.tobytes()
        if i % 2:
            s = s[::-1].translate(COMP)
        recs.append((b"read%d" % i, s, bytes(rng.integers(33, 75, size=read_len, dtype=np.uint8))))
    return fastq(recs)


def _qual(rng, n):
    """quality strings that start with '@' or '+' and hold '>', A, C, G and T"""
    alphabet = np.frombuffer(b"@+>ACGTI#5", dtype=np.uint8)
    return bytes(alphabet[rng.integers(0, len(alphabet), size=n)])


def ingest_cases():
    rng = np.random.default_rng(55)
    cases = []
    recs = [(b"r%d" % i, synth.random_genome(rng, int(rng.integers(0, 300))).tobytes(), None) for i in range(200)]
    cases.append(fastq(recs))
    # CRLF, lower case, N runs
    recs2 = []
    for i in range(150):
        s = bytearray(synth.random_genome(rng, int(rng.integers(1, 400))).tobytes())
        for a in rng.integers(0, len(s), size=3):
            n_run = int(rng.integers(1, 20))
            s[a:a + n_run] = b"N" * len(s[a:a + n_run])
        s = bytes(s)
        if i % 3 == 0:
            s = s.lower()
        recs2.append((b"c%d" % i, s, _qual(rng, len(s))))
    cases.append(fastq(recs2, crlf=True))
    # qualities that start with '@' / '+' and hold '>' and bases; 0xFF bytes in headers
    recs3 = [(b"\xff%d\xff" % i, synth.random_genome(rng, 90).tobytes(), b"@" + _qual(rng, 89) if i % 2 else b"+" + _qual(rng, 89))
             for i in range(100)]
    cases.append(fastq(recs3))
    # empty reads and reads shorter than k; no final newline; trailing blank lines
    recs4 = [(b"e%d" % i, synth.random_genome(rng, i % 7).tobytes(), None) for i in range(60)]
    cases.append(fastq(recs4, final_newline=False))
    cases.append(fastq(recs4) + b"\n\n\r\n")
    cases.append(fastq(recs4 + [(b"last", b"", b"")]) + b"\n\n")
    cases.append(fastq([(b"only", b"ACGTACGT", None)], final_newline=False))
    # a newline exactly on a 4096-byte seam, and records straddling tiles
    head = b"@x\n"
    seq = synth.random_genome(rng, 4096 - len(head) - 1).tobytes()
    cases.append(fastq([(b"x", seq, None)] + [(b"y%d" % i, synth.random_genome(rng, 5000).tobytes(), None) for i in range(5)]))
    cases.append(fastq([(b"z%d" % i, synth.random_genome(rng, int(rng.integers(1000, 12000))).tobytes(), None) for i in range(40)]))
    # more than two rounds of the tile scan (> 40 MB): 150 bp reads with N's and lower case
    g = synth.random_genome(rng, 300_000)
    reads = []
    n_reads = 44_000_000 // 318
    starts = rng.integers(0, len(g) - 150, size=n_reads)
    for i, a in enumerate(starts):
        s = g[a:a + 150].tobytes()
        if i % 97 == 0:
            s = s[:40] + b"NNNNN" + s[45:].lower()
        reads.append(b"@big%d\n%s\n+\n%s\n" % (i, s, b"F" * 150))
    big = b"".join(reads)
    assert len(big) > 40_000_000
    cases.append(big)
    return cases


def _device(text):
    import torch
    d = torch.from_numpy(np.frombuffer(text + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return d


def test_fastq_device_ingest_equals_oracle_of_fasta_form(ctx):
    """spsp_fastq_clean_device / _packed_device == orc.clean_fasta(F(T)): bases, record offsets, record count, 2-bit words."""
    for text in ingest_cases():
        want_b, want_o = orc.clean_fasta(fastq_to_fasta(text))
        d = _device(text)
        db, nb, do, nr = ctx.clean_fastq_device(d.data_ptr(), len(text))
        assert nr == len(want_o) - 1 and nb == len(want_b), (len(text), nr, nb, len(want_o) - 1, len(want_b))
        assert ctx.to_host(do, nr + 1, np.uint64).tolist() == want_o.tolist()
        assert ctx.to_host(db, nb, np.uint8).tobytes() == want_b.tobytes()
        dp, nb2, do2, nr2 = ctx.clean_fastq_packed_device(d.data_ptr(), len(text))
        assert (nb2, nr2) == (nb, nr) and ctx.to_host(do2, nr + 1, np.uint64).tolist() == want_o.tolist()
        n_dw = (nb + 15) // 16
        codes = np.zeros(n_dw * 16, dtype=np.uint32)
        codes[:nb] = (want_b.astype(np.uint32) >> 1) & 3
        want_w = (codes.reshape(-1, 16) << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)
        got_w = ctx.to_host(dp, n_dw + 64, np.uint32)
        assert (got_w[:n_dw] == want_w).all() and not got_w[n_dw:].any()


STAT_FIELDS = ("selected_kmer_number", "read_kmer", "nb_mmer_selected", "seen_kmers_at_reconstruction", "total_superkmer_number")


@pytest.mark.parametrize("k,m,s", [(31, 11, 1000), (31, 11, 100), (63, 15, 20), (21, 11, 1.0)])
def test_fastq_sketch_text_equals_oracle(ctx, k, m, s):
    rng = np.random.default_rng(k * m)
    g = synth.random_genome(rng, 60_000)
    text = simulate_reads(rng, g, 5, 150, 0.01)
    text += fastq([(b"short", b"ACGT", None), (b"n", b"NNNNNN", None), (b"low", g[:500].tobytes().lower(), None)], crlf=True)
    got, gst = ctx.sketch_text(text, k, m, s, flags=sp.SPSP_SCAN_STATS)
    want, wst = orc.sketch_fasta(fastq_to_fasta(text), k, m, s)
    assert got == want
    for f in STAT_FIELDS:
        assert gst[f] == wst[f], f


@pytest.mark.parametrize("ab", [2, 3])
def test_fastq_read_set_abundance_equals_oracle(ctx, ab):
    """-a on a simulated read set (20x coverage, both strands, 1 % substitutions): the case the floor exists for."""
    k, m, s = 31, 11, 20
    rng = np.random.default_rng(ab)
    g = synth.random_genome(rng, 50_000)
    text = simulate_reads(rng, g, 20, 150, 0.01)
    got, gst = ctx.sketch_text(text, k, m, s, abundance=ab)
    want, wst = orc.sketch_fasta(fastq_to_fasta(text), k, m, s, ab)
    assert got == want
    for f in ("selected_kmer_number", "selected_superkmer_number", "count_maximal_skmer", "seen_kmers_at_reconstruction",
              "actual_minimizer_number", "read_kmer"):
        assert gst[f] == wst[f], f


MALFORMED = [
    ("header", b"@a\nACGT\n+\nIIII\nb\nACGT\n+\nIIII\n", 1, "header"),
    ("separator", b"@a\nACGT\n+\nIIII\n@b\nACGT\n-\nIIII\n@c\nA\n+\nI\n", 1, "separator"),
    ("length", b"@a\nACGT\n+\nIIII\n@b\nAC\n+\nI\n@c\nACGT\n+\nIIIII\n", 1, "length"),
    ("truncated", b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\n", 1, "truncated"),
    ("truncated2", b"@a\nACGT\n+\nIIII\n@b\nACGT\n", 1, "truncated"),
    ("wrapped", b"@a\nACGT\n+\nIIII\n@b\nACGTAC\nGTACGT\n+\nIIIIIIIIIIII\n", 1, "separator"),
    ("crlf_length", b"@a\r\nACGT\r\n+\r\nIIII\r\n@b\r\nACGT\r\n+\r\nIII\r\n", 1, "length"),
]


@pytest.mark.parametrize("name,text,rec,rule", MALFORMED, ids=[x[0] for x in MALFORMED])
def test_fastq_malformed_is_format_error(ctx, name, text, rec, rule):
    for call in ("sketch_text", "clean", "clean_packed"):
        with pytest.raises(sp.SpspError) as e:
            if call == "sketch_text":
                ctx.sketch_text(text, 31, 11, 10)
            else:
                d = _device(text)
                (ctx.clean_fastq_device if call == "clean" else ctx.clean_fastq_packed_device)(d.data_ptr(), len(text))
        assert e.value.code == -6, (call, str(e.value))
        msg = str(e.value)
        assert re.search(r"record %d\b" % rec, msg) and rule in msg, (call, msg)
    # a malformed record far into a large text: the index is the record's
    big = fastq([(b"r%d" % i, b"ACGT" * 30, None) for i in range(30_000)]) + text
    with pytest.raises(sp.SpspError) as e:
        ctx.sketch_text(big, 31, 11, 10)
    assert re.search(r"record %d\b" % (30_000 + rec), str(e.value)), str(e.value)


def _batch_files(tmp_path, rng):
    g = synth.random_genome(rng, 40_000)
    files = []   # (path, text the oracle sketches or None when the file must fail)
    fa = synth.to_fasta(synth.random_genome(rng, 30_000), "fa", n_records=2)
    p = tmp_path / "plain.fa"; p.write_bytes(fa); files.append((str(p), fa))
    fq1 = simulate_reads(rng, g, 3, 150, 0.01)
    p = tmp_path / "reads1.fq"; p.write_bytes(fq1); files.append((str(p), fastq_to_fasta(fq1)))
    fq2 = simulate_reads(rng, g, 2, 100, 0.0)
    p = tmp_path / "reads2.fq.gz"; p.write_bytes(gzip.compress(fq2, 1)); files.append((str(p), fastq_to_fasta(fq2)))
    p = tmp_path / "empty.fq"; p.write_bytes(b""); files.append((str(p), b""))
    badfq = fastq([(b"ok%d" % i, g[i * 50:i * 50 + 120].tobytes(), None) for i in range(20)]) + b"@bad\nACGTACGT\n+\nIII\n"
    p = tmp_path / "bad.fq"; p.write_bytes(badfq); files.append((str(p), None))
    fa2 = synth.to_fasta(g[:20_000], "again")
    p = tmp_path / "again.fa.gz"; p.write_bytes(gzip.compress(fa2, 1)); files.append((str(p), fa2))
    fq3 = simulate_reads(rng, g, 1, 150, 0.0)
    fq3 = fq3.replace(b"\n", b"\r\n")
    p = tmp_path / "reads3.fastq"; p.write_bytes(fq3); files.append((str(p), fastq_to_fasta(fq3)))
    return files


@pytest.mark.parametrize("devices", [None, [0]])
def test_fastq_in_batched_file_pipeline(tmp_path, devices):
    """one list of small FASTA and FASTQ files (several share a batch): every output equals the oracle's bytes, the one
    malformed FASTQ file alone reports SPSP_ERR_FORMAT with its record index."""
    k, m, s = 31, 11, 50.0
    files = _batch_files(tmp_path, np.random.default_rng(9))
    ins = [f for f, _ in files]
    fields = ("selected_kmer_number", "selected_superkmer_number", "seen_kmers_at_reconstruction", "read_kmer", "total_superkmer_number")
    for threads, ab, s_ in ((1, 1, s), (4, 1, s), (4, 1, 1000.0), (3, 2, s)):
        outs = [str(tmp_path / ("o_%s_%d_%d_%d_%d.gz" % (bool(devices), threads, ab, int(s_), i))) for i in range(len(ins))]
        res, _, _ = sp.sketch_files(ins, outs, k, m, s_, abundance=ab, threads=threads, flags=sp.SPSP_SCAN_STATS, devices=devices)
        for i, (rc, st, err) in enumerate(res):
            want_text = files[i][1]
            if want_text is None:
                assert rc == -6 and "record 20" in err and "length" in err, (i, rc, err)
                continue
            assert rc == 0, (threads, i, rc, err)
            want, wst = orc.sketch_fasta(want_text, k, m, s_, ab)
            assert sp.read_file(outs[i]) == want, (threads, ab, i)
            if ab == 1:
                for f in fields:
                    assert st[f] == wst[f], (threads, i, f)


def test_fastq_cli(tmp_path):
    """bin/sub_sampler -i reads.fq.gz and -f over a mixed list: the sketches of F(T); the comparator's CSVs over the
    FASTQ-derived sketches equal those over the FASTA-derived ones."""
    k, m, s = 31, 11, 50
    rng = np.random.default_rng(3)
    gs = synth.family_genomes(5, 3, 40_000, 1, [0.0, 0.02])
    exe = os.path.join(ROOT, "bin", "sub_sampler")
    reads = [simulate_reads(rng, g, 4, 150, 0.005) for g in gs]
    (tmp_path / "fq").mkdir(); (tmp_path / "fa").mkdir()
    fq_names, fa_names = [], []
    for i, r in enumerate(reads):
        p = tmp_path / "fq" / ("s%d.fq.gz" % i); p.write_bytes(gzip.compress(r, 1)); fq_names.append(str(p))
        p = tmp_path / "fa" / ("s%d.fa" % i); p.write_bytes(fastq_to_fasta(r)); fa_names.append(str(p))
    r = subprocess.run([exe, "-i", fq_names[0], "-k", str(k), "-m", str(m), "-s", str(s), "-p", "one_"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    want0, _ = orc.sketch_fasta(fastq_to_fasta(reads[0]), k, m, float(np.float32(s)))
    assert gzip.open(tmp_path / "one_s0.gz", "rb").read() == want0
    mixed = [fq_names[0], fa_names[1], fq_names[2]]
    for tag, names in (("fq", mixed), ("fa", fa_names)):
        (tmp_path / (tag + ".txt")).write_text("\n".join(names) + "\n")
        r = subprocess.run([exe, "-f", tag + ".txt", "-k", str(k), "-m", str(m), "-s", str(s), "-t", "2", "-p", tag + "_"],
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        listed = (tmp_path / (tag + "_" + tag + ".txt")).read_text().split()
        assert listed == ["%s_s%d.gz" % (tag, i) for i in range(3)]
        for i, nm in enumerate(listed):
            want, _ = orc.sketch_fasta(fastq_to_fasta(reads[i]), k, m, float(np.float32(s)))
            assert gzip.open(tmp_path / nm, "rb").read() == want, nm
        r = subprocess.run([os.path.join(ROOT, "bin", "comparator"), "-f", tag + "_" + tag + ".txt", "-o", "res_" + tag],
                           cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    for fn in ("_jaccard.csv.gz", "_containment.csv.gz"):
        a = gzip.open(tmp_path / ("res_fq" + fn), "rb").read().replace(b"fq_", b"")
        b = gzip.open(tmp_path / ("res_fa" + fn), "rb").read().replace(b"fa_", b"")
        assert a == b and len(a) > 0, fn


def test_fasta_with_fastq_like_lines_is_untouched(ctx):
    """detection looks at the first byte only: a FASTA text whose lines start with '@' and '+' sketches as FASTA."""
    rng = np.random.default_rng(11)
    g = synth.random_genome(rng, 80_000).tobytes()
    text = b">r0\n" + g[:30_000] + b"\n@not_a_read\n" + g[30_000:60_000] + b"\n+\n" + g[60_000:] + b"\n"
    for k, m, s in ((31, 11, 50), (31, 11, 1000)):
        got, gst = ctx.sketch_text(text, k, m, s, flags=sp.SPSP_SCAN_STATS)
        want, wst = orc.sketch_fasta(text, k, m, s)
        assert got == want
        for f in STAT_FIELDS:
            assert gst[f] == wst[f], f
    d = _device(text)
    db, nb, do, nr = ctx.clean_fasta_device(d.data_ptr(), len(text))
    want_b, want_o = orc.clean_fasta(text)
    assert nr == len(want_o) - 1 and ctx.to_host(db, nb, np.uint8).tobytes() == want_b.tobytes()
