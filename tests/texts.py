"""FASTA / FASTQ texts written by position, and what an ingest must make of them: numpy, bytes and plain integers.

A text starts as a soup of bases (soup()) and gets its structure stamped in at absolute byte positions (put(), header(),
Fastq): a case says WHERE a newline, a '>' or an '@' stands, not how long the records in front of it are.  The soup holds no
'\\n', '\\r', '>', '@', '+' or 0xFF, so a text's structure is exactly what was stamped; header and quality bytes are soup
too, i.e. bases that must not survive.

What is expected of a text:
    FASTA   the project's oracle, orc.clean_fasta(text) (the caller's business: nothing here imports it)
    FASTQ   fastq_as_fasta(text) through the same oracle -- one FASTA record per four lines, well-formed or not -- and
            fastq_verdict(text), the validator, written from the rules of include/spsp.h and spsp_internal.h
    batch   lay_batch(files): the slab as the file pipeline lays it out, and the files' descriptors
survivors() is a third, independent account (a numpy mask of the bytes that survive), used to say how many survivors a tile
holds and where its output begins.

Neither torch nor the library under test is imported here."""
import numpy as np

CHUNK, WAVE, TILE, LANE, SCAN_WAVE, ROUND = 16, 1024, 4096, 16384, 1 << 20, 1 << 24
HEADER, SEPARATOR, LENGTH, TRUNCATED = 1, 2, 3, 4
RULE_WORD = {HEADER: "header", SEPARATOR: "separator", LENGTH: "length", TRUNCATED: "truncated"}
FASTQ_FLAG, FAILED_FLAG = 1, 2                   # SPSP_BATCH_FASTQ, SPSP_BATCH_FAILED

_PURE = np.frombuffer(b"ACGT", dtype=np.uint8)
_MIXED = np.frombuffer(b"ACGTACGTACGTACGTacgtacgtNnRY-*", dtype=np.uint8)
_IS_BASE = np.zeros(256, dtype=bool)
_IS_BASE[list(b"ACGTacgt")] = True


def soup(n, seed, pure=False):
    """n bytes of bases: ACGT alone (pure), or with lower case and a few bytes that are no base"""
    rng = np.random.default_rng(seed)
    alphabet = _PURE if pure else _MIXED
    return bytearray(alphabet[rng.integers(0, len(alphabet), size=n)].tobytes())


def put(buf, pos, data):
    """write data at the absolute position pos of buf"""
    assert 0 <= pos and pos + len(data) <= len(buf), (pos, len(data), len(buf))
    buf[pos:pos + len(data)] = data
    return pos + len(data)


def header(buf, pos, end, first=b">"):
    """a FASTA header line: '\\n' at pos - 1 (unless pos is 0), `first` at pos, '\\n' at end - 1; what lies between stays soup"""
    assert pos + 2 <= end
    if pos:
        put(buf, pos - 1, b"\n")
    put(buf, pos, first)
    put(buf, end - 1, b"\n")


class Fastq:
    """four-line records stamped into a soup one behind the other; `at` is where the next line begins.  Line lengths are
    without the line end ('\\n', or '\\r\\n' with crlf)."""

    def __init__(self, n, seed, crlf=False, buf=None, at=0):
        self.buf = soup(n, seed) if buf is None else buf
        self.at, self.end, self.n_rec = at, (2 if crlf else 1), 0
        self.crlf = crlf

    def line(self, length, first=None):
        if first is not None and length:
            put(self.buf, self.at, first)
        self.at += length
        if self.crlf:
            self.at = put(self.buf, self.at, b"\r")
        self.at = put(self.buf, self.at, b"\n")
        return self.at - 1                       # where the line's '\n' stands

    def record(self, h, s, p=1, q=None, first=b"@", sep=b"+", qfirst=None):
        """header of h bytes, sequence of s, separator of p, quality of q (as long as the sequence unless given)"""
        nls = [self.line(h, first), self.line(s), self.line(p, sep), self.line(s if q is None else q, qfirst)]
        self.n_rec += 1
        return nls

    def fill(self, target, room=400):
        """ordinary reads until fewer than `room` + 330 bytes are left in front of target"""
        i = 0
        while self.at + 330 + room <= target:
            self.record(3 + i % 5, 61 + (i * 37) % 97)
            i += 1

    def land(self, role, nl_at, s=37, **kw):
        """one record whose line of this role has its '\\n' at nl_at: the header (roles 0 and 3), the sequence (1) or the
        separator (2) takes up the slack.  q_more makes the quality line that much longer than the sequence."""
        e, q_more = self.end, kw.pop("q_more", 0)
        if role == 0:
            h = nl_at - self.at - (e - 1)
        elif role == 1:
            h, s = 3, nl_at - self.at - (3 + e) - (e - 1)
        elif role == 2:
            h = 3
        else:
            h = nl_at - self.at - (s + e) - (1 + e) - (s + q_more + e) - (e - 1)
        p = nl_at - self.at - (h + e) - (s + e) - (e - 1) if role == 2 else 1
        assert h >= 1 and s >= 0 and p >= 1, (role, nl_at, self.at, h, s, p)
        nls = self.record(h, s, p, s + q_more, **kw)
        assert nls[role] == nl_at, (nls, role, nl_at)
        return nls

    def text(self, final_newline=True, cut=None):
        """the text so far; cut: up to and including the byte at cut - 1"""
        t = bytes(self.buf[:self.at if cut is None else cut])
        return t if final_newline or cut is not None else t[:-self.end]


# ------------------------------------------------------------------------------------------------- what is expected

def fastq_content(text):
    """(content end, blank_tail): the text less its trailing '\\n' / '\\r'; blank_tail iff a byte follows the first '\\n' behind it"""
    end = len(text.rstrip(b"\n\r"))
    nl = text.find(b"\n", end)
    return end, nl >= 0 and nl + 1 < len(text)


def fastq_verdict(text):
    """None for a well-formed FASTQ text, else the smallest (record, rule)"""
    end, blank_tail = fastq_content(text)
    lines = text[:end].split(b"\n")
    found, d = [], 0
    for i, ln in enumerate(lines):
        role, rec = i % 4, i // 4
        length = len(ln) - (1 if ln.endswith(b"\r") and i != len(lines) - 1 else 0)
        if role == 0 and ln[:1] != b"@":
            found.append((rec, HEADER))
        elif role == 2 and ln[:1] != b"+":
            found.append((rec, SEPARATOR))
        elif role == 1:
            d += length
        elif role == 3:
            d -= length
            if d:
                found.append((rec, LENGTH))
    role, rec = (len(lines) - 1) % 4, (len(lines) - 1) // 4
    if not (role == 3 or (role == 2 and blank_tail)):
        found.append((rec, TRUNCATED))
    elif role == 2 and d:
        found.append((rec, LENGTH))
    return min(found) if found else None


def fastq_as_fasta(text):
    """the FASTA text whose records are the text's groups of four lines, each with its second line as the sequence: what
    the ingest keeps of a FASTQ file whether it is well-formed or not (b"" for a text without content)"""
    end, _ = fastq_content(text)
    if not end:
        return b""
    lines = text[:end].split(b"\n")
    return b"".join(b">\n" + (lines[i + 1] if i + 1 < len(lines) else b"") + b"\n" for i in range(0, len(lines), 4))


def survivors(text, fastq=False):
    """bool per byte: does it survive?  FASTA: a base on a line that is neither line 0 nor starts with '>' or 0xFF.  FASTQ: a
    base of the content on a line whose number is 1 modulo 4."""
    a = np.frombuffer(bytes(text), dtype=np.uint8)
    if not len(a):
        return np.zeros(0, dtype=bool)
    nl = a == 10
    line = np.cumsum(nl) - nl                    # a newline belongs to the line it ends
    if fastq:
        return _IS_BASE[a] & (line % 4 == 1) & (np.arange(len(a)) < fastq_content(bytes(text))[0])
    first = np.concatenate(([0], np.flatnonzero(nl) + 1))
    drop = np.zeros(len(first), dtype=bool)
    inside = first < len(a)
    drop[inside] = (a[first[inside]] == 0x3E) | (a[first[inside]] == 0xFF)
    drop[0] = True
    return _IS_BASE[a] & ~drop[line]


def tile_counts(mask):
    """survivors per 4 KiB tile, and where each tile's output begins"""
    n_tiles = (len(mask) + TILE - 1) // TILE
    keep = np.bincount(np.flatnonzero(mask) // TILE, minlength=n_tiles).astype(np.int64)
    return keep, np.cumsum(keep) - keep


def words(bases):
    """the 2-bit words of cleaned bases: 16 to a dword, the first in bits 31:30, code (c >> 1) & 3, zero tail"""
    n_dw = (len(bases) + 15) // 16
    codes = np.zeros(n_dw * 16, dtype=np.uint32)
    codes[:len(bases)] = (np.asarray(bases, dtype=np.uint32) >> 1) & 3
    return (codes.reshape(-1, 16) << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


# ----------------------------------------------------------------------------------------------------------- batches

def lay_batch(files):
    """files: (kind, text) with kind "fasta", "fastq" or "failed" (a file that could not be read: its text's length is what
    counts) -> (slab, [(offset, text length, flags)], [the text each file is read as, None for a failed one]).  The file
    pipeline's rule: every file starts on a multiple of 4096, a FASTA text that is empty or starts with neither '>' nor 0xFF
    gets a '>' in front, '\\n' fills up to the next multiple of 4096 strictly behind the file's end."""
    slab, described, read_as = bytearray(), [], []
    for kind, text in files:
        assert len(slab) % TILE == 0 and kind in ("fasta", "fastq", "failed")
        if kind == "fasta" and text[:1] not in (b">", b"\xff"):
            text = b">" + text
        if kind == "failed":
            text = b"\n" * len(text)
        described.append((len(slab), len(text), {"fasta": 0, "fastq": FASTQ_FLAG, "failed": FAILED_FLAG}[kind]))
        read_as.append(None if kind == "failed" else text)
        slab += text
        slab += b"\n" * ((len(slab) + TILE) // TILE * TILE - len(slab))
    return bytes(slab), described, read_as


def batch_expected(files, clean):
    """clean: FASTA bytes -> (bases, offsets), the oracle.  -> (bases, offsets, first record per file or None, bad per file)"""
    _, described, read_as = lay_batch(files)
    bases, offs, first, bad = [], [0], [], []
    for (kind, _), text in zip(files, read_as):
        if text is None:
            first.append(None)
            bad.append(~0 & (2 ** 64 - 1))
            continue
        b, o = clean(fastq_as_fasta(text) if kind == "fastq" else text)
        n_rec = len(o) - 1
        if kind == "fastq" and not fastq_content(text)[0]:
            n_rec = 0                            # (the oracle gives an empty text one empty record)
        first.append(len(offs) - 1)
        v = fastq_verdict(text) if kind == "fastq" else None
        bad.append(2 ** 64 - 1 if v is None else ((first[-1] + v[0]) << 8) | v[1])
        base = offs[-1]
        offs += [base + int(x) for x in o[1:n_rec + 1]]
        bases.append(np.asarray(b, dtype=np.uint8))
    return (np.concatenate(bases) if bases else np.zeros(0, dtype=np.uint8)), offs, first, bad
