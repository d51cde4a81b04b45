"""Sketch payloads written by hand, and the keys a reader must find in them: plain Python integers and bytes.

The format is the one sketch_parse_structure_host documents (supersampler_amd/csrc/spsp_host.cpp): a header line
"<2k - m> <m> <count> <rate>\\n", then per bucket the m ASCII bases of its minimizer, a little-endian u32 blob length, the
blob (one zero byte, then the stored bases of every maximal super-k-mer, four to a byte, first base in bits 7:6), the
non-maximal super-k-mers as lines "prefix\\nsuffix\\n", and an empty pair "\\n\\n".  A base's 2-bit code is (c >> 1) & 3
(A 0, C 1, T 2, G 3) and its complement is code ^ 2.

Nothing here comes from the library under test or from the oracle: tests hold both to model()."""
import struct

U64 = (1 << 64) - 1
LETTERS = b"ACTG"                                # indexed by code


def code(c):
    return (c >> 1) & 3


_DIGITS = bytes.maketrans(b"ACTG", b"0123")
_COMPLEMENT = bytes.maketrans(b"ACTG", b"TGAC")
_QUADS = [bytes(LETTERS[(b >> sh) & 3] for sh in (6, 4, 2, 0)) for b in range(256)]


def to_int(s):
    """ASCII bases -> the 2-bit integer, first base in the highest bits"""
    return int(s.translate(_DIGITS), 4) if s else 0


def bases(v, n):
    """the n bases of the 2-bit integer v, as ASCII"""
    nb = (n + 3) // 4
    return b"".join(_QUADS[b] for b in v.to_bytes(nb, "big"))[4 * nb - n:]


def revcomp(s):
    return s.translate(_COMPLEMENT)[::-1]


def canonical_windows(k, s):
    """min(window, reverse complement) of every k-long window of the bases s, as integers of 2k bits, in order"""
    n = len(s) - k + 1
    if n <= 0:
        return []
    mask = (1 << (2 * k)) - 1
    f, r = to_int(s), to_int(revcomp(s))         # window i is bits of f from the top, its reverse complement bits of r from the bottom
    return [min((f >> (2 * (n - 1 - i))) & mask, (r >> (2 * i)) & mask) for i in range(n)]


def pack(seq):
    """bases four to a byte, first base in bits 7:6"""
    assert len(seq) % 4 == 0
    return bytes((code(seq[i]) << 6) | (code(seq[i + 1]) << 4) | (code(seq[i + 2]) << 2) | code(seq[i + 3]) for i in range(0, len(seq), 4))


def payload(k, m, buckets, count=0, rate=1.0, first_byte=0, long_lines=False, cut=0):
    """buckets: [(minimizer_ascii, maximal, lines)], maximal and lines lists of (prefix, suffix); written in the order given.

    first_byte 1..3: every blob starts with that byte instead of zero.  A reader then takes the blob's last byte as a partial
        one that holds first_byte bases; the writer puts 2(k - m) - 4 + first_byte spare bases behind the maximal super-k-mers,
        one short of another super-k-mer, so the keys stay model()'s -- and a reader that took the blob for a standard one
        would find one super-k-mer too many.
    long_lines: prefixes and suffixes of more than 255 bases are let through.
    cut: that many bytes, newlines all of them, are left off the end (2: the final empty pair; 4 behind a last line with an
        empty suffix: the payload ends inside a line)."""
    out = [b"%d %d %d %g\n" % (2 * k - m, m, count, rate)]
    for mn, maximal, lines in buckets:
        assert len(mn) == m
        out.append(mn)
        if maximal:
            assert all(len(p) == k - m and len(s) == k - m for p, s in maximal) and (len(maximal) * 2 * (k - m)) % 4 == 0
            blob = bytes([first_byte]) + pack(b"".join(p + s for p, s in maximal))
            if first_byte:
                assert 1 <= first_byte <= 3 and (k - m) % 2 == 0 and k - m >= 2
                blob += pack((b"ACGT" * (k - m))[: 2 * (k - m) - 4]) + bytes([0x6c])
            out.append(struct.pack("<I", len(blob)) + blob)
        else:
            out.append(struct.pack("<I", 0))
        for p, s in lines:
            assert b"\n" not in p + s and len(p) + len(s) > 0 and (long_lines or (len(p) <= 255 and len(s) <= 255))
            out.append(p + b"\n" + s + b"\n")
        out.append(b"\n\n")
    data = b"".join(out)
    if cut:
        assert data[-cut:] == b"\n" * cut
        data = data[:-cut]
    return data


def model(k, m, buckets):
    """the sorted distinct keys (minimizer as a 2-bit integer, canonical k-mer as an integer of 2k bits) of the buckets"""
    keys = set()
    for mn, maximal, lines in buckets:
        v = to_int(mn)
        if k == m and not maximal and not lines:
            keys.add((v, canonical_windows(k, mn)[0]))               # the bare minimizer is one k-mer
        for pre, suf in set(maximal) | set(lines):                   # (a line shorter than k in total has no window)
            for w in canonical_windows(k, pre + mn + suf):
                keys.add((v, w))
    return sorted(keys)


def raw_keys(k, m, buckets):
    """every key as a reader meets it, duplicates included, in payload order"""
    out = []
    for mn, maximal, lines in buckets:
        v = to_int(mn)
        if k == m and not maximal:
            out.append((v, canonical_windows(k, mn)[0]))
        memo = {}
        for pre, suf in list(maximal) + list(lines):
            if (pre, suf) not in memo:
                memo[(pre, suf)] = [(v, w) for w in canonical_windows(k, pre + mn + suf)]
            out += memo[(pre, suf)]
    return out


def split(v):
    """canonical k-mer -> (kmer_hi, kmer_lo)"""
    return v >> 64, v & U64
