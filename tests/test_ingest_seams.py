"""The FASTA / FASTQ ingest (spsp_ingest.hip: k_clean_*, k_mixed_*) on hand-built texts at its seams.

Every path that starts from a file goes through these kernels, and they cut the text at fixed places whatever it holds:
16-byte lane chunks (the byte behind a chunk is fetched separately), 1 024-byte waves, 4 096-byte tiles, on the
single-workgroup scan 4 tiles per lane (16 KiB), 64 lanes per wave (1 MiB) and 1 024 lanes per round (16 MiB), and on the
output 16-byte groups that neighbouring tiles share.  Random texts meet a given seam by luck.  The texts below are stamped by
position (tests/texts.py) so that each seam is met on purpose, and every expectation is exact: the oracle's bases and offsets,
the 2-bit words with their zero tail and halo, and for FASTQ the verdict of texts.fastq_verdict.

ingest_cases() is the one table: (name, form, text or files, claims) with form "fasta", "fastq" (well-formed), "malformed"
(claims hold the expected (record, rule)) or "batch" (files: (kind, text) in the order of the batch).
test_the_cases_are_what_they_are_called recomputes every claim from the text alone, on the CPU.

What a wrong kernel would look like, and where it shows:
    the byte behind a chunk or a tile misread (next, nx / na / np): *_nl_*, fq_role*, fq_cr_lf_*, mal_* at S - 1 and S
    the entry state of a tile without a newline, across a scan lane's tiles: fa_long_*, fq_long_*
    D not carried across tiles, lanes, waves or rounds: fq_D_*, fq_role2_*, fq_16m, mal_len_*, mal_rebalanced
    a tile's first or last output group written by one neighbour only: fa_shared_group, fa_gap_*, fa_total_*
    state, D or the record count of one file reaching the next: batch_*
    a slot of an old call read as this call's: test_one_context_over_many_calls"""
import functools
import re

import numpy as np
import pytest

import supersampler_amd as sp
import test_fastq as TF
import texts as X
from oracle import oracle_py as orc
from texts import CHUNK, LANE, ROUND, SCAN_WAVE, TILE, WAVE, Fastq, header, put, soup

SEAMS = (CHUNK, WAVE, TILE, LANE, SCAN_WAVE)
MAL_SEAMS = (CHUNK, WAVE, TILE, LANE)

_TABLE = []                                      # (name, form, thunk -> (text or files, claims)), in the order of the names


def _case(name, form, fn, *args, **kw):
    _TABLE.append((name, form, functools.partial(fn, *args, **kw)))


def _seam_claims(pos, s):
    """pos is the first byte behind a seam of unit s (and so of every smaller unit)"""
    return [("mod", pos, u, 0) for u in (CHUNK, WAVE, TILE, LANE, SCAN_WAVE, ROUND) if u <= s]


# ------------------------------------------------------------------------------------------------------------- FASTA

def _fa(n, seed, pure=False, lines_upto=None):
    """a FASTA soup of n bytes: '>h0' in front where it fits, data lines of 60 bytes up to lines_upto"""
    buf = soup(n, seed, pure)
    if n >= 4:
        put(buf, 0, b">h0\n")
    a = np.frombuffer(buf, dtype=np.uint8)
    a[64:max(64, n if lines_upto is None else lines_upto):61] = 10
    return buf


def fa_seam(kind, s):
    buf = _fa(s + TILE + 37, s % 251, lines_upto=s - 64)
    if kind in ("gt", "ff"):                     # '\n' at S - 1, '>' or 0xFF at S
        first = b">" if kind == "gt" else b"\xff"
        header(buf, s, s + 21, first)
        claims = [("byte", s - 1, b"\n"), ("byte", s, first), ("byte", s + 20, b"\n")]
    elif kind == "gt_before":                    # '\n' at S - 2, '>' at S - 1
        header(buf, s - 1, s + 21)
        claims = [("byte", s - 2, b"\n>")]
    elif kind == "nl_at":                        # '\n' is the byte at S
        put(buf, s, b"\n")
        claims = [("byte", s, b"\n"), ("no_newline", s - 3, s)]
    elif kind == "hdr_cut":                      # '\n>' in front of the seam, a base at S, the header ends behind it
        header(buf, s - 5, s + 9)
        put(buf, s - 1, b"GATTACA")
        claims = [("byte", s - 6, b"\n>"), ("byte", s, b"A"), ("no_newline", s - 5, s + 8), ("byte", s + 8, b"\n")]
    else:                                        # empty records on the seam
        put(buf, s - 4, b"\n>a\n>b\n>c\n")
        claims = [("byte", s - 1, b"\n>b\n>")]
    return bytes(buf), claims + _seam_claims(s, s)


def fa_long(kind):
    if kind == "header":                         # a header line over five whole tiles
        buf = _fa(10 * TILE, 3, lines_upto=4900)
        header(buf, 5000, 5000 + 6 * TILE + 100)
        put(buf, 9 * TILE, b"\n")
        return bytes(buf), [("byte", 4999, b"\n>"), ("no_newline", 2 * TILE, 7 * TILE)] + [("tile_keep", t, 0) for t in range(2, 7)]
    if kind == "data":                           # a data line over five whole tiles
        buf = _fa(10 * TILE, 4, pure=True, lines_upto=4900)
        header(buf, 5000, 5020)
        put(buf, 5020 + 6 * TILE + 100, b"\n>x\n")
        return bytes(buf), [("no_newline", 2 * TILE, 7 * TILE)] + [("tile_keep", t, TILE) for t in range(2, 7)]
    buf = soup(3 * TILE + 11, 5)                 # line 0 without '>', longer than a tile
    put(buf, 5000, b"\n")
    return bytes(buf), [("no_newline", 0, 5000), ("tile_keep", 0, 0), ("byte", 5000, b"\n")]


def fa_tiny(text):
    return text, [("len", len(text))]


def fa_length(n):
    return bytes(_fa(n, n % 97)), [("len", n)]


def fa_gap(byte, j):
    """chunks whose only non-base is byte j, the survivors in front of them taking every residue modulo 16"""
    buf = soup(2 * TILE + 5, 7 + j, pure=True)
    put(buf, 0, b">h\n")
    chunks = [2 + 2 * i for i in range(16)] + [TILE // CHUNK + 2 + 2 * i for i in range(16)]
    for c in chunks:
        put(buf, CHUNK * c + j, byte)
    return bytes(buf), [("gaps", tuple(chunks), j)]


def fa_obase(r):
    """tile 1's output begins at r modulo 16; in it and in tile 2, chunks whose only non-base is the '\\n' at byte r"""
    buf = soup(3 * TILE + 9, 200 + r, pure=True)
    header(buf, 0, 32 - r)
    chunks = [TILE // CHUNK + 1 + 3 * i for i in range(16)] + [2 * TILE // CHUNK + 3 * i for i in range(16)]
    for c in chunks:
        put(buf, CHUNK * c + r, b"\n")
    return bytes(buf), [("obase15", 1, r), ("obase15", 2, r), ("gaps", tuple(chunks), r)]


def fa_shared_group():
    """tile 1 gives 3 survivors, tiles 2 and 3 none (3 holds no newline at all), 4 gives 4, 5 gives 2, 6 gives 15; tile 1's
    output begins at 2 modulo 16, so tiles 0 to 6 write one 16-byte group and one packed word between them"""
    buf = soup(9 * TILE, 11, pure=True)
    header(buf, 0, 14)
    header(buf, TILE + 4, 2 * TILE)              # tile 1: 3 bases, '\n', a header up to the tile's last byte
    header(buf, 2 * TILE, 4 * TILE + 11)         # '>' on tile 2's first byte, through tile 3, into tile 4
    header(buf, 4 * TILE + 11 + 5, 5 * TILE)     # tile 4: 4 bases, ...
    header(buf, 5 * TILE + 3, 6 * TILE)
    header(buf, 6 * TILE + 16, 7 * TILE)
    claims = [("tile_keep", t, k) for t, k in ((1, 3), (2, 0), (3, 0), (4, 4), (5, 2), (6, 15))]
    claims += [("obase15", 1, 2), ("one_group", 0, 5), ("one_group", 5, 6), ("no_newline", 3 * TILE, 4 * TILE),
               ("rec_at_obase", 2), ("rec_at_obase", 5), ("rec_at_obase", 6)]
    return bytes(buf), claims


def fa_total(m):
    return b">h\n" + bytes(soup(m, m, pure=True)), [("total", m)]


def fa_16m():
    """a header whose '\\n' is the last byte of round 0 of the scan, and a data line that crosses into round 1"""
    n = ROUND + 3 * TILE
    buf = soup(n, 16)
    a = np.frombuffer(buf, dtype=np.uint8)
    a[8000::8192] = 10                           # lines of 8 KiB
    a[65536 + 8001::65536] = ord(">")            # every eighth of them a header
    put(buf, 0, b">h0\n")
    header(buf, ROUND - 150, ROUND)
    return bytes(buf), [("byte", ROUND - 151, b"\n>"), ("byte", ROUND - 1, b"\n"), ("no_newline", ROUND - 150, ROUND - 1),
                        ("no_newline", ROUND, ROUND + 8000), ("len", n)] + _seam_claims(ROUND, ROUND)


for _s in SEAMS:
    for _kind in ("gt", "ff", "gt_before", "nl_at", "hdr_cut", "empty"):
        _case("fa_%s_%d" % (_kind, _s), "fasta", fa_seam, _kind, _s)
for _kind in ("header", "data", "line0"):
    _case("fa_long_%s" % _kind, "fasta", fa_long, _kind)
for _i, _t in enumerate((b"", b">", b"A", b"\n")):
    _case("fa_tiny_%d" % _i, "fasta", fa_tiny, _t)
for _n in (4095, 4096, 4097, 15, 17, 31, 33, 1023, 1025, 4111, 4113, 8191, 8193):
    _case("fa_length_%d" % _n, "fasta", fa_length, _n)
for _j in range(16):
    _case("fa_gap_nl_%d" % _j, "fasta", fa_gap, b"\n", _j)
    _case("fa_gap_N_%d" % _j, "fasta", fa_gap, b"N", _j)
for _r in range(16):
    _case("fa_obase_%d" % _r, "fasta", fa_obase, _r)
_case("fa_shared_group", "fasta", fa_shared_group)
for _m in (15, 16, 17, 4111, 4112, 4113):
    _case("fa_total_%d" % _m, "fasta", fa_total, _m)
_case("fa_16m", "fasta", fa_16m)


# ------------------------------------------------------------------------------------------------------------- FASTQ

def _short(s):
    return 2 if s == CHUNK else 37               # a read that leaves room for a record in front of byte 16


def _lead(b, role, nl_at, s=37, **kw):
    """ordinary reads up to shortly before nl_at, then the record whose line `role` ends in a '\\n' at nl_at"""
    b.fill(nl_at - (2 * s + 16 + 4 * b.end + kw.get("q_more", 0)), room=0)
    return b.land(role, nl_at, s, **kw)


def _more(b, n=3):
    for i in range(n):
        b.record(4 + i, 70 + 3 * i)
    return b


def fq_role(role, s, qfirst=None):
    """the '\\n' of a line of this role at S - 1, the next line's first byte at S"""
    b = Fastq(s + 3 * TILE, s % 251 + role)
    _lead(b, role, s - 1, _short(s), **({"qfirst": qfirst} if qfirst else {}))
    claims = [("byte", s - 1, b"\n"), ("role", s - 1, role), ("role", s, (role + 1) % 4)] + _seam_claims(s, s)
    if qfirst:
        claims.append(("byte", s, qfirst))
    return _more(b).text(), claims


def fq_crlf(role, s, nl_at):
    b = Fastq(s + 3 * TILE, s % 251 + 7 * role, crlf=True)
    _lead(b, role, nl_at, _short(s))
    return _more(b).text(), [("byte", nl_at - 1, b"\r\n"), ("role", nl_at, role)] + _seam_claims(s, s)


def fq_long(kind):
    b = Fastq(16 * TILE, 21)
    b.record(5, 50)
    nls = b.record(5 * TILE + 5000, 60) if kind == "header" else b.record(5, 6 * TILE + 100)
    _more(b)
    if kind == "header":
        return b.text(), [("no_newline", TILE, 6 * TILE)] + [("tile_keep", t, 0) for t in range(1, 6)]
    return b.text(), [("no_newline", TILE, 6 * TILE), ("no_newline", 8 * TILE, 12 * TILE), ("tiles_apart", nls[1], nls[3], 5)] + \
        [("tile_keep", t, 0) for t in range(8, 12)]


def fq_d(s):
    """a read of 9 000 bases: its sequence ends in front of the seam, its quality two tiles or more behind it"""
    b = Fastq(s + 8 * TILE, 23)
    nls = _lead(b, 2, s - 1, 9000) if s else (b.record(5, 50), b.record(5, 9000))[1]
    claims = [("tiles_apart", nls[1], nls[3], 2)]
    if s:
        claims += [("byte", s - 1, b"\n"), ("role", s - 1, 2)] + _seam_claims(s, s)
    return _more(b).text(), claims


def fq_empty(s):
    """an empty read on the seam: the '\\n' of its empty sequence line at S - 1, its '+' at S"""
    b = Fastq(s + 3 * TILE, 29)
    _lead(b, 0, s - 2, 0)
    return _more(b).text(), [("byte", s - 2, b"\n\n+\n\n"), ("role", s - 1, 1)] + _seam_claims(s, s)


def fq_end(end, final_newline, s):
    b = Fastq(end + 200, end % 97)
    _lead(b, 3, end, _short(s))
    return b.text(cut=end + 1 if final_newline else end), [("content_end", end), ("len", end + (1 if final_newline else 0))]


def _body():
    b = Fastq(2000, 31)
    return _more(b, 4).text(final_newline=False)


def fq_tail(n, crlf):
    body = _body()
    tail = (b"\r\n" * (n // 2 + 1))[-n:] if crlf else b"\n" * n
    return body + tail, [("content_end", len(body)), ("len", len(body) + n)]


def fq_empty_last(s):
    """an empty last read: a blank quality line and a blank tail; with s, its '+' is the byte at S - 1"""
    b = Fastq(s + 1000, 37)
    if s:
        _lead(b, 3, s - 10)
    else:
        _more(b)
    b.line(6, b"@")
    b.line(0)
    b.line(1, b"+")
    text = b.text() + b"\n\n"
    return text, [("content_end", b.at - 1), ("byte", b.at - 2, b"+\n\n\n")] + ([("byte", s - 1, b"+")] if s else [])


def big_fastq(seam, seed):
    """reads of 8 KiB in front, then one whose '+' line ends on the byte in front of `seam` -- its sequence lies in front of
    the seam, its quality behind it -- and one more read"""
    n_std = seam // 8192 - 1
    buf = soup(seam + 6 * TILE, seed)
    a = np.frombuffer(buf, dtype=np.uint8)[:n_std * 8192].reshape(-1, 8192)
    a[:, 0] = ord("@")                           # '@' + 6, 4 090 bases, '+', 4 090 quality bytes: 8 192 bytes a read
    a[:, 4099] = ord("+")
    a[:, [7, 4098, 4100, 8191]] = 10
    b = Fastq(0, 0, buf=buf, at=n_std * 8192)
    nls = b.land(2, seam - 1, seam - 1 - b.at - 10)
    b.record(7, 2047)
    assert b.at >= seam + 3 * TILE
    return b.text(), nls


def fq_16m():
    text, nls = big_fastq(ROUND, 41)
    return text, [("byte", ROUND - 1, b"\n"), ("role", ROUND - 1, 2), ("tiles_apart", nls[1], nls[3], 1)] + _seam_claims(ROUND, ROUND)


for _s in SEAMS:
    for _r in range(4):
        _case("fq_role%d_%d" % (_r, _s), "fastq", fq_role, _r, _s)
    _case("fq_qual_at_%d" % _s, "fastq", fq_role, 2, _s, qfirst=b"@")
    _case("fq_qual_plus_%d" % _s, "fastq", fq_role, 2, _s, qfirst=b"+")
    for _r in (0, 1, 3):
        _case("fq_cr_lf_split_r%d_%d" % (_r, _s), "fastq", fq_crlf, _r, _s, _s)
        _case("fq_crlf_ends_r%d_%d" % (_r, _s), "fastq", fq_crlf, _r, _s, _s - 1)
_case("fq_long_header", "fastq", fq_long, "header")
_case("fq_long_read", "fastq", fq_long, "read")
for _s in (0, LANE, SCAN_WAVE):
    _case("fq_D_%d" % _s, "fastq", fq_d, _s)
for _s in MAL_SEAMS:
    _case("fq_empty_%d" % _s, "fastq", fq_empty, _s)
for _s in (CHUNK, WAVE, TILE):
    for _e in (_s - 1, _s, _s + 1):
        _case("fq_end_%d_bare" % _e, "fastq", fq_end, _e, False, _s)
        _case("fq_end_%d_newline" % _e, "fastq", fq_end, _e, True, _s)
for _n in (4095, 4096, 4097, 20000):
    _case("fq_tail_lf_%d" % _n, "fastq", fq_tail, _n, False)
    _case("fq_tail_crlf_%d" % _n, "fastq", fq_tail, _n, True)
_case("fq_empty_last", "fastq", fq_empty_last, 0)
_case("fq_empty_last_%d" % TILE, "fastq", fq_empty_last, TILE)
_case("fq_16m", "fastq", fq_16m)


# --------------------------------------------------------------------------------------------------- FASTQ, malformed

def mal(kind, s, p, crlf=False):
    """the deciding byte of one rule at p (S - 1 or S)"""
    b = Fastq(s + 3 * TILE, s % 251 + p % 7, crlf=crlf)
    sh = _short(s)
    cut = None
    if kind == "header":                         # a header line that starts with 'X' at p
        _lead(b, 3, p - 1, sh)
        want = (b.n_rec, X.HEADER)
        b.record(5, 40, first=b"X")
        claims = [("byte", p - 1, b"\nX"), ("role", p, 0)]
    elif kind == "noheader":                     # an empty line at p where a header belongs
        _lead(b, 3, p - 1, sh)
        want = (b.n_rec, X.HEADER)
        b.line(0)
        claims = [("byte", p - 1, b"\n\n"), ("role", p, 0)]
    elif kind == "sep":                          # a separator line that starts with '-' at p
        _lead(b, 1, p - 1, sh, sep=b"-")
        want = (b.n_rec - 1, X.SEPARATOR)
        claims = [("byte", p - 1, b"\n-"), ("role", p, 2)]
    elif kind == "len":                          # a quality line one byte too long, closed by the '\n' at p
        _lead(b, 3, p, sh, q_more=1)
        want = (b.n_rec - 1, X.LENGTH)
        claims = [("byte", p - 1, b"\r\n") if crlf else ("byte", p, b"\n"), ("role", p, 3)]
    else:                                        # the content ends with a line of role 0, 1 or 2 whose '\n' is at p
        role = int(kind[-1])
        _lead(b, role, p, sh)
        want = (b.n_rec - 1, X.TRUNCATED)
        cut = p + 1
        claims = [("byte", p, b"\n"), ("role", p, role), ("len", p + 1)]
    if cut is None:
        _more(b, 2)
    return b.text(cut=cut), [("verdict", want), ("mod", p, s, 0 if p == s else s - 1)] + claims


def mal_two_faults_a():
    """record r: a wrong separator in tile 1, its length mismatch closing in tile 2; record r + 1: a wrong header"""
    b = Fastq(4 * TILE, 43)
    b.fill(2 * TILE - 50 - 200, room=0)
    nls = b.land(1, 2 * TILE - 50, sep=b"-", q_more=1)
    want = (b.n_rec - 1, X.SEPARATOR)
    b.record(5, 40, first=b"X")
    return _more(b, 2).text(), [("verdict", want), ("byte", nls[1], b"\n-"), ("tile", nls[1] + 1, 1), ("tile", nls[3], 2), ("byte", nls[3], b"\nX")]


def mal_two_faults_b():
    """record r: a length mismatch alone; record r + 1: a wrong header behind the same newline, a tile's last byte"""
    b = Fastq(3 * TILE, 47)
    _lead(b, 3, TILE - 1, q_more=1)
    want = (b.n_rec - 1, X.LENGTH)
    b.record(5, 40, first=b"X")
    return _more(b, 2).text(), [("verdict", want), ("byte", TILE - 1, b"\nX")]


def mal_rebalanced():
    """a quality line two bytes too long, then a read whose quality is two bytes short: D is back at 0 behind it"""
    b = Fastq(3 * TILE, 53)
    _lead(b, 3, TILE - 1, q_more=2)
    want = (b.n_rec - 1, X.LENGTH)
    b.record(5, 50, q=48)
    return _more(b, 2).text(), [("verdict", want), ("byte", TILE - 1, b"\n@")]


def mal_blank_quality(s):
    """the content ends with a '+' line behind a read of four bases, a blank tail follows: the blank quality line is too short;
    with s, the '+' is the byte at S - 1"""
    b = Fastq(s + 1000, 61)
    if s:
        _lead(b, 3, s - 11)
    else:
        _more(b)
    want = (b.n_rec, X.LENGTH)
    b.line(3, b"@")
    b.line(4)
    b.line(1, b"+")
    return b.text() + b"\n\n", [("verdict", want), ("content_end", b.at - 1), ("byte", b.at - 2, b"+\n\n\n"), ("role", b.at - 2, 2)] + \
        ([("byte", s - 1, b"+")] + _seam_claims(s, s) if s else [])


def mal_at_alone():
    return b"@", [("verdict", (0, X.TRUNCATED)), ("len", 1)]


for _s in MAL_SEAMS:
    for _p in (_s - 1, _s):
        for _kind in ("header", "noheader", "sep", "len", "trunc0", "trunc1", "trunc2"):
            _case("mal_%s_%d" % (_kind, _p), "malformed", mal, _kind, _s, _p)
        _case("mal_len_crlf_%d" % _p, "malformed", mal, "len", _s, _p, crlf=True)
_case("mal_two_faults_a", "malformed", mal_two_faults_a)
_case("mal_two_faults_b", "malformed", mal_two_faults_b)
_case("mal_rebalanced", "malformed", mal_rebalanced)
_case("mal_blank_quality", "malformed", mal_blank_quality, 0)
_case("mal_blank_quality_%d" % TILE, "malformed", mal_blank_quality, TILE)
_case("mal_at_alone", "malformed", mal_at_alone)


# ------------------------------------------------------------------------------------------------------------ batches

def fa_file(seed, n=700):
    buf = _fa(n, seed)
    if n > 200:
        header(buf, n // 2, n // 2 + 9)
    return ("fasta", bytes(buf))


def fq_file(seed, n=700):
    """a FASTQ file of exactly n bytes, the last one a '\\n'"""
    b = Fastq(n + 8, seed)
    _lead(b, 3, n - 1)
    return ("fastq", b.text())


def _starts(files):
    return [off // TILE for off, _, _ in X.lay_batch(files)[1]]


def _clean_claims(files):
    return [("bad", f, None) for f, (kind, _) in enumerate(files) if kind == "fastq"]


def batch_order(kinds):
    files = [fa_file(60 + i, 500 + 300 * i) if k == "a" else fq_file(70 + i, 600 + 250 * i) for i, k in enumerate(kinds)]
    return files, _clean_claims(files) + [("kinds", kinds)]


def batch_length(n, kind):
    """a file of 4 095 bytes leaves a gap of one '\\n', one of 4 096 a gap of a whole tile"""
    first = fa_file(81, n) if kind == "a" else fq_file(82, n)
    files = [first, fa_file(83), fq_file(84)]
    return files, _clean_claims(files) + [("starts", (0, 1, 2) if n < TILE else (0, 2, 3)), ("slab", n - 1, bytes(first[1][-1:]) + b"\n"), ("text_len", 0, n)]


def batch_forced():
    """FASTA files without a leading '>' (one of them 4 095 bytes, a whole tile with the '>' forced in front) and an empty one"""
    files = [fq_file(85), ("fasta", bytes(soup(300, 86))), ("fasta", b""), ("fasta", bytes(soup(4095, 87))), fa_file(88), fq_file(89)]
    return files, _clean_claims(files) + [("slab", TILE, b">"), ("slab", 2 * TILE, b">\n"), ("slab", 3 * TILE, b">"), ("starts", (0, 1, 2, 3, 5, 6))]


def batch_ends_in_header(then):
    last = ("fasta", b">a\n" + bytes(soup(100, 90)) + b"\n>a header that no newline ends ACGT")
    files = [last, fa_file(91), fq_file(92)] if then == "a" else [last, fq_file(92), fa_file(91)]
    return files, _clean_claims(files)


def batch_next_starts(then):
    """a FASTA file whose last tile ends in '\\n' at byte 4 095, and what starts on the next byte"""
    nxt = {"gt": fa_file(93), "ff": ("fasta", b"\xffname\n" + bytes(soup(200, 94))), "fq": fq_file(95)}[then]
    files = [fa_file(96, 4095), nxt, fq_file(97), fa_file(98, 2 * TILE - 1), nxt]
    return files, _clean_claims(files) + [("slab", TILE - 1, b"\n" + nxt[1][:1]), ("slab", 5 * TILE - 1, b"\n" + nxt[1][:1])]


def batch_failed(where):
    good = [fa_file(101), fq_file(102), fa_file(103, 5000), fq_file(104, 5000)]
    if where == "between":
        files = [good[0], ("failed", b"x" * 100), good[1], ("failed", b"x" * 5000), ("failed", b"x" * 10), good[2], good[3]]
    elif where == "first":
        files = [("failed", b"x" * 5000)] + good
    else:
        files = good + [("failed", b"x" * 100)]
    return files, _clean_claims(files)


def batch_lane_positions(flip):
    """files that start on each of the four tiles of a scan lane, FASTA and FASTQ on each"""
    files = [fq_file(105, 4 * TILE - 100)]
    files += [fa_file(106 + i) if (i + flip) % 2 == 0 else fq_file(106 + i) for i in range(8)]
    return files, _clean_claims(files) + [("starts", (0,) + tuple(range(4, 12)))]


def batch_260_tiles():
    """131 files of two tiles each: file starts in both waves of the scan's first round"""
    files = [fa_file(200 + i, 5000) if i % 2 else fq_file(200 + i, 5000) for i in range(131)]
    return files, _clean_claims(files) + [("starts", tuple(range(0, 262, 2)))]


def batch_16m():
    """a FASTQ file from the batch's second tile on whose read straddles the scan's round seam"""
    text, nls = big_fastq(ROUND - TILE, 59)
    files = [fa_file(110), ("fastq", text), fa_file(111), fq_file(112)]
    return files, _clean_claims(files) + [("slab", ROUND - 1, b"\n"), ("starts", (0, 1, 1 + (len(text) + TILE) // TILE, 2 + (len(text) + TILE) // TILE))]


def _truncated_file():
    """ten lines, the content ending behind a sequence line: D is 8 and the role 2 where the file ends"""
    b = Fastq(600, 113)
    _more(b, 2)
    return ("fastq", b.text() + b"@x\nACGTACGT\n")


def batch_leak(order):
    files = [_truncated_file(), fq_file(114)] if order == "truncated_first" else [fq_file(114), _truncated_file()]
    files.append(fa_file(115))
    t = 0 if order == "truncated_first" else 1
    return files, [("bad", t, (2, X.TRUNCATED)), ("bad", 1 - t, None), ("lines", t, 10)]


def batch_malformed_between():
    b = Fastq(3000, 116)
    _more(b, 3)
    b.record(5, 40, q=41)
    _more(b, 2)
    files = [fa_file(117), ("fastq", b.text()), fq_file(118)]
    return files, [("bad", 1, (3, X.LENGTH)), ("bad", 2, None)]


def batch_rule(kind):
    """one rule's deciding byte on the first byte of the second tile of a file that is not the first"""
    text, claims = mal(kind, TILE, TILE)
    files = [fa_file(119), ("fastq", text), fq_file(120)]
    return files, [("bad", 1, dict((c[0], c[1]) for c in claims)["verdict"]), ("bad", 2, None)]


def batch_256():
    files = [fa_file(300 + i, 90) if i % 2 else fq_file(300 + i, 150) for i in range(256)]
    return files, _clean_claims(files) + [("starts", tuple(range(256)))]


for _k in ("aq", "qa", "qq", "aaq", "qaa"):
    _case("batch_order_%s" % _k, "batch", batch_order, _k)
for _n in (4095, 4096, 4097):
    for _k in "aq":
        _case("batch_length_%d_%s" % (_n, _k), "batch", batch_length, _n, _k)
_case("batch_forced", "batch", batch_forced)
for _k in "aq":
    _case("batch_ends_in_header_then_%s" % _k, "batch", batch_ends_in_header, _k)
for _k in ("gt", "ff", "fq"):
    _case("batch_next_starts_%s" % _k, "batch", batch_next_starts, _k)
for _k in ("between", "first", "last"):
    _case("batch_failed_%s" % _k, "batch", batch_failed, _k)
for _k in (0, 1):
    _case("batch_lane_positions_%d" % _k, "batch", batch_lane_positions, _k)
_case("batch_260_tiles", "batch", batch_260_tiles)
_case("batch_16m", "batch", batch_16m)
for _k in ("truncated_first", "truncated_last"):
    _case("batch_leak_%s" % _k, "batch", batch_leak, _k)
_case("batch_malformed_between", "batch", batch_malformed_between)
for _k in ("header", "sep", "len", "trunc1"):
    _case("batch_rule_%s" % _k, "batch", batch_rule, _k)
_case("batch_256", "batch", batch_256)


@functools.lru_cache(maxsize=None)
def case(name):
    for n, form, thunk in _TABLE:
        if n == name:
            payload, claims = thunk()
            return (n, form, payload, claims)
    raise KeyError(name)


def ingest_cases():
    return [case(n) for n, _, _ in _TABLE]


def _names(*forms):
    return [n for n, form, _ in _TABLE if form in forms]


@functools.lru_cache(maxsize=None)
def expected(name):
    """the reference of a case, computed once: (bases, offsets) -- of a batch: (bases, offsets, first records, bad words)"""
    _, form, payload, _ = case(name)
    if form == "fasta":
        b, o = orc.clean_fasta(payload)
        return b, [int(x) for x in o]
    if form == "fastq":
        b, o = orc.clean_fasta(TF.fastq_to_fasta(payload))
        return b, [int(x) for x in o]
    assert form == "batch"
    return X.batch_expected(payload, orc.clean_fasta)


# ----------------------------------------------------------------------------------------------------- the CPU side

def _check_claims(name, form, payload, claims):
    if form == "batch":
        slab, described, read_as = X.lay_batch(payload)
        for c in claims:
            if c[0] == "bad":
                assert X.fastq_verdict(read_as[c[1]]) == c[2], (name, c)
            elif c[0] == "kinds":
                assert "".join("a" if k == "fasta" else "q" for k, _ in payload) == c[1], (name, c)
            elif c[0] == "starts":
                assert tuple(_starts(payload)) == c[1], (name, c, _starts(payload))
            elif c[0] == "slab":
                assert slab[c[1]:c[1] + len(c[2])] == c[2], (name, c, slab[c[1]:c[1] + len(c[2])])
            elif c[0] == "text_len":
                assert described[c[1]][1] == c[2], (name, c)
            elif c[0] == "lines":
                assert len(read_as[c[1]][:X.fastq_content(read_as[c[1]])[0]].split(b"\n")) == c[2], (name, c)
            else:
                raise AssertionError((name, c))
        # the layout's own rule, and every file a start of its own
        assert len(slab) % TILE == 0 and all(off % TILE == 0 for off, _, _ in described)
        for (off, n, _), nxt in zip(described, [d[0] for d in described[1:]] + [len(slab)]):
            assert nxt == (off + n + TILE) // TILE * TILE and slab[off + n:nxt] == b"\n" * (nxt - off - n), name
        return
    text = payload
    fastq = form != "fasta"
    mask = X.survivors(text, fastq)
    keep, obase = X.tile_counts(mask)
    nl_before = lambda pos: text.count(b"\n", 0, pos)
    for c in claims:
        kind = c[0]
        if kind == "byte":
            assert text[c[1]:c[1] + len(c[2])] == c[2], (name, c, text[c[1]:c[1] + len(c[2])])
        elif kind == "mod":
            assert c[1] % c[2] == c[3], (name, c)
        elif kind == "len":
            assert len(text) == c[1], (name, c, len(text))
        elif kind == "no_newline":
            assert b"\n" not in text[c[1]:c[2]] and c[2] <= len(text), (name, c)
        elif kind == "role":
            assert nl_before(c[1]) % 4 == c[2], (name, c, nl_before(c[1]) % 4)
        elif kind == "tile":
            assert c[1] // TILE == c[2], (name, c)
        elif kind == "tiles_apart":
            assert text[c[1]] == 10 and text[c[2]] == 10 and c[2] // TILE - c[1] // TILE >= c[3], (name, c)
        elif kind == "content_end":
            assert X.fastq_content(text)[0] == c[1], (name, c, X.fastq_content(text))
        elif kind == "tile_keep":
            assert keep[c[1]] == c[2], (name, c, keep[c[1]])
        elif kind == "obase15":
            assert obase[c[1]] & 15 == c[2], (name, c, obase[c[1]])
        elif kind == "one_group":                # every tile from c[1] to c[2] has a byte of one and the same 16-byte group
            first_end, last = obase[c[1]] + keep[c[1]] - 1, obase[c[2]]
            assert keep[c[1]] and keep[c[2]] and first_end >> 4 == last >> 4, (name, c, first_end, last)
        elif kind == "rec_at_obase":
            assert int(obase[c[1]]) in [int(x) for x in orc.clean_fasta(text)[1][1:]], (name, c, obase[c[1]])
        elif kind == "total":
            assert int(mask.sum()) == c[1], (name, c, int(mask.sum()))
        elif kind == "gaps":
            residues = set()
            for ch in c[1]:
                m = mask[CHUNK * ch:CHUNK * ch + CHUNK]
                assert m.sum() == 15 and not m[c[2]], (name, ch)
                residues.add(int(mask[:CHUNK * ch].sum()) % 16)
            assert residues == set(range(16)), (name, residues)
        elif kind == "verdict":
            assert form == "malformed" and c[1] is not None
        else:
            raise AssertionError((name, c))
    verdict = X.fastq_verdict(text) if fastq else None
    if form == "malformed":
        assert verdict == dict((c[0], c[1]) for c in claims)["verdict"], (name, verdict)
    elif form == "fastq":
        assert verdict is None, (name, verdict)
        # the two accounts of a well-formed text agree: the structural reading and test_fastq's F(T)
        a, b = orc.clean_fasta(X.fastq_as_fasta(text)), orc.clean_fasta(TF.fastq_to_fasta(text))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist(), name
    if form != "malformed":
        want_b, _ = expected(name)
        assert int(mask.sum()) == len(want_b), (name, int(mask.sum()), len(want_b))


def test_the_names_are_distinct_and_every_form_is_there():
    names = [n for n, _, _ in _TABLE]
    assert len(set(names)) == len(names)
    assert {f for _, f, _ in _TABLE} == {"fasta", "fastq", "malformed", "batch"}


def test_the_cases_are_what_they_are_called():
    """every claim of every case, recomputed from its text; the validator against test_fastq's verdicts and texts"""
    rule = {"header": X.HEADER, "separator": X.SEPARATOR, "length": X.LENGTH, "truncated": X.TRUNCATED}
    for name, text, rec, word in TF.MALFORMED:
        assert X.fastq_verdict(text) == (rec, rule[word]), name
    for text in TF.ingest_cases():
        if len(text) < 40_000_000:
            assert X.fastq_verdict(text) is None
            a, b = orc.clean_fasta(X.fastq_as_fasta(text)), orc.clean_fasta(TF.fastq_to_fasta(text))
            assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist()
    for name, form, payload, claims in ingest_cases():
        _check_claims(name, form, payload, claims)
    # the sizes the issue allows: under 64 KiB but for the 1 MiB seams and one 16 MiB case per form
    size = {n: (len(X.lay_batch(p)[0]) if form == "batch" else len(p)) for n, form, p, _ in ingest_cases()}
    assert [n for n in size if size[n] > ROUND] == ["fa_16m", "fq_16m", "batch_16m"]
    assert all(size[n] <= ROUND + 8 * TILE for n in size)
    assert all(n.endswith("_%d" % SCAN_WAVE) or n in ("batch_260_tiles", "batch_256") for n in size if 65536 <= size[n] <= ROUND)


# ----------------------------------------------------------------------------------------------------- the GPU side

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def _device(text):
    import torch
    d = torch.from_numpy(np.frombuffer(bytes(text) + b"\0" * 16, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return d


def _same(ctx, got, want_b, want_o, packed, what):
    """record count, all n_rec + 1 offsets, the bases -- or the words, their zero tail and the 64 halo words -- exactly"""
    d_out, nb, d_off, nr = got[:4]
    assert nr == len(want_o) - 1 and nb == len(want_b), (what, nr, nb, len(want_o) - 1, len(want_b))
    off = ctx.to_host(d_off, nr + 1, np.uint64)
    if off.tolist() != list(want_o):
        i = next(i for i, (a, b) in enumerate(zip(off.tolist(), want_o)) if a != b)
        raise AssertionError("%s: rec_off[%d] is %d, not %d" % (what, i, off[i], want_o[i]))
    if not packed:
        b = ctx.to_host(d_out, nb, np.uint8)
        if b.tobytes() != want_b.tobytes():
            i = int(np.flatnonzero(b != want_b)[0])
            raise AssertionError("%s: base %d is %r, not %r (%r / %r)" % (what, i, bytes(b[i:i + 1]), bytes(want_b[i:i + 1]),
                                                                         bytes(b[max(0, i - 8):i + 8]), bytes(want_b[max(0, i - 8):i + 8])))
        return
    n_dw = (nb + 15) // 16
    w, want_w = ctx.to_host(d_out, n_dw + 64, np.uint32), X.words(want_b)
    if not (w[:n_dw] == want_w).all():
        i = int(np.flatnonzero(w[:n_dw] != want_w)[0])
        raise AssertionError("%s: word %d of %d is %08x, not %08x" % (what, i, n_dw, w[i], want_w[i]))
    assert not w[n_dw:].any(), (what, "halo", np.flatnonzero(w[n_dw:])[:4])


def check(ctx, name, what=""):
    """one case through the ASCII and the packed entry"""
    _, form, payload, claims = case(name)
    what = "%s %s" % (name, what)
    if form == "batch":
        want_b, want_o, first, bad = expected(name)
        slab, described, _ = X.lay_batch(payload)
        for packed in (False, True):
            got = ctx.clean_batch(slab, described, packed=packed)
            _same(ctx, got, want_b, want_o, packed, "%s packed=%d" % (what, packed))
            rec_base, got_bad = got[4], got[5]
            assert [int(x) for x in got_bad] == bad, (what, packed, [hex(int(x)) for x in got_bad], [hex(x) for x in bad])
            for (off, _, _), f in zip(described, first):
                if f is not None:                # (a failed file has no record and nobody asks for its base)
                    assert int(rec_base[off // TILE]) - 1 == f, (what, packed, off // TILE, int(rec_base[off // TILE]), f)
        return
    d = _device(payload)
    fasta = form == "fasta"
    for packed in (False, True):
        call = {(True, False): ctx.clean_fasta_device, (True, True): ctx.clean_fasta_packed_device,
                (False, False): ctx.clean_fastq_device, (False, True): ctx.clean_fastq_packed_device}[(fasta, packed)]
        if form == "malformed":
            rec, rule = dict((c[0], c[1]) for c in claims)["verdict"]
            with pytest.raises(sp.SpspError) as e:
                call(d.data_ptr(), len(payload))
            msg = str(e.value)
            assert e.value.code == sp.ERR_FORMAT, (what, packed, msg)
            assert re.search(r"record %d\b" % rec, msg) and X.RULE_WORD[rule] in msg, (what, packed, (rec, X.RULE_WORD[rule]), msg)
        else:
            want_b, want_o = expected(name)
            _same(ctx, call(d.data_ptr(), len(payload)), want_b, want_o, packed, "%s packed=%d" % (what, packed))


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("fasta"))
def test_fasta_ingest_is_the_oracle(ctx, name):
    check(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("fastq"))
def test_fastq_ingest_is_the_oracle(ctx, name):
    check(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("malformed"))
def test_fastq_verdict_is_the_validator(ctx, name):
    check(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names("batch"))
def test_batch_ingest_is_the_oracle_file_by_file(ctx, name):
    check(ctx, name)


@pytest.mark.gpu
def test_batch_of_257_files_is_an_argument_error(ctx):
    files = [fa_file(i, 90) if i % 2 else fq_file(i, 150) for i in range(257)]
    slab, described, _ = X.lay_batch(files)
    for packed in (False, True):
        with pytest.raises(sp.SpspError) as e:
            ctx.clean_batch(slab, described, packed=packed)
        assert e.value.code == sp.ERR_ARG, str(e.value)
    check(ctx, "batch_256", "after the refused call")


@pytest.mark.gpu
def test_one_context_over_many_calls():
    """a context of the test's own: a long text, then a short one, FASTQ (a malformed text in between), FASTA, a batch, and
    round again -- stale entry / output / D / verdict slots, the packed buffer's zeroing and the closing offset would show"""
    order = ["fa_gt_%d" % SCAN_WAVE, "fa_tiny_2", "fa_total_17", "fq_role2_%d" % SCAN_WAVE, "mal_len_%d" % TILE, "fq_end_15_bare",
             "mal_two_faults_a", "fq_D_0", "fa_shared_group", "batch_malformed_between", "batch_lane_positions_1", "batch_leak_truncated_first",
             "fq_empty_last", "fa_tiny_0", "batch_failed_first", "fa_long_header", "fq_role3_%d" % LANE, "batch_order_aq"]
    with sp.Context(0) as own:
        for i, name in enumerate(order + order[::-1]):
            check(own, name, "call %d" % i)
