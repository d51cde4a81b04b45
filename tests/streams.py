"""Hand-built super-k-mer streams and a model of the sketch builder, for tests/test_build_seams.py.

model() is the expectation: handle_superkmer and the emission written down from their rules in plain Python -- one
insertion-ordered dict per minimizer, counts kept mod 256, find() of the minimizer's first place (255 for none), the cursor
over insertion order, left extension and then right extension, neighbours tried in the order A, T, C, G, `seen` marks,
maximal super-k-mers into the strCompressor blob and the others as "prefix\\nsuffix\\n", buckets ascending.  It knows nothing
of sorts, tables, tiles or lanes.  Besides the payload and the four emission counters it returns what a test case needs to
prove that it is what its name says (info).

Stream is the builder of the inputs.  A super-k-mer of q k-mers around an m-mer X is L + X + R with |L|, |R| <= k - m and
|L| >= q - 1, so that every window of k bases holds X.  A stream entry is (rec, minimizer, start, len, rev) as the scan
writes it: with rev = 1 the record holds the reverse complement of the oriented super-k-mer.
"""
import numpy as np

CODE = {65: 0, 67: 1, 84: 2, 71: 3}              # A C T G -> 0 1 2 3: the 2-bit code (ASCII >> 1) & 3
NUC = b"ACTG"
COMP = bytes.maketrans(b"ACGT", b"TGCA")
COUNTERS = ("actual_minimizer_number", "seen_kmers_at_reconstruction", "seen_superkmers_at_reconstruction",
            "seen_max_superkmers_at_reconstruction")
SUPERKMER_DTYPE = np.dtype([("rec", "<u4"), ("minimizer", "<u4"), ("start", "<u8"), ("len", "<u4"), ("rev", "<u4")])


def num(s):
    v = 0
    for c in s:
        v = v * 4 + CODE[c]
    return v


def bases(v, n):
    """the n bases whose 2-bit number is v"""
    return bytes(NUC[(v >> (2 * (n - 1 - j))) & 3] for j in range(n))


def revcomp(s):
    return s[::-1].translate(COMP)


def rnd(rng, n):
    return bytes(NUC[rng.randrange(4)] for _ in range(n))


def oriented(bases_buf, rec_off, entry):
    """the super-k-mer of a stream entry as handle_superkmer sees it"""
    rec, _, start, ln, rev = (int(x) for x in entry)
    a = int(rec_off[rec]) + start
    s = bytes(bases_buf[a: a + ln])
    return revcomp(s) if rev else s


def entries(stream):
    """a structured array or a list of tuples -> list of (rec, minimizer, start, len, rev)"""
    if isinstance(stream, np.ndarray):
        return list(zip(stream["rec"].tolist(), stream["minimizer"].tolist(), stream["start"].tolist(), stream["len"].tolist(),
                        stream["rev"].tolist()))
    return [tuple(int(x) for x in e) for e in stream]


# ------------------------------------------------------------------------------------------------ the model

def model(k, m, abundance, rate, bases_buf, rec_off, stream):
    """-> (payload, counters, info).  info, all from the rules alone:
        buckets        minimizers ascending
        entries[mn]    stream entries of the bucket;  places[mn]  k-mer places;  distinct[mn]  different k-mers
        counts[mn]     {k-mer: occurrences (not reduced mod 256)}, in insertion order
        first_entry[mn]  {k-mer: which of the bucket's entries (0-based, stream order) inserted it}
        forks          [(mn, 'L' | 'R', usable neighbours)] for every step at which two or more neighbours were usable
        walks          [(mn, start k-mer, bases added left, bases added right, left extension stopped early, maximal)]
        seen_refused   k-mers (starts and neighbours) refused ONLY because an earlier walk had taken them
        blob[mn], text[mn]   the bucket's blob and lines"""
    whole = bytes(bases_buf)
    offs = [int(x) for x in rec_off]
    half, full = k - m, 2 * k - m
    index = {}
    info = {"entries": {}, "places": {}, "first_entry": {}, "forks": [], "walks": [], "seen_refused": 0, "blob": {}, "text": {}}
    selected = 0
    for rec, mn, start, ln, rev in entries(stream):
        s = whole[offs[rec] + start: offs[rec] + start + ln]
        if rev:
            s = revcomp(s)
        ms = bases(mn, m)
        d = index.setdefault(mn, {})
        fe = info["first_entry"].setdefault(mn, {})
        nth = info["entries"].get(mn, 0)
        info["entries"][mn] = nth + 1
        for i in range(ln - k + 1):
            km = s[i: i + k]
            selected += 1
            e = d.get(km)
            if e is not None:
                e[0] = (e[0] + 1) & 255
                e[3] += 1
            else:
                at = km.find(ms)
                d[km] = [1, 255 if at < 0 else at, False, 1]           # uint8 count, place of the minimizer, seen, true count
                fe[km] = nth
        info["places"][mn] = info["places"].get(mn, 0) + ln - k + 1
    out = bytearray(b"%d %d %d %f\n" % (full, m, selected, rate))
    n_entries = n_skm = n_max = 0
    for mn in sorted(index):
        d = index[mn]
        ms = bases(mn, m)
        out += ms
        codes, text = [], bytearray()

        def enough(e):
            return e[0] >= abundance

        def step(frm, left):
            found = []
            for c in b"ATCG":
                nx = bytes([c]) + frm[:-1] if left else frm[1:] + bytes([c])
                e = d.get(nx)
                if e is None or not enough(e):
                    continue
                if e[2]:
                    info["seen_refused"] += 1
                    continue
                found.append(nx)
            if len(found) > 1:
                info["forks"].append((mn, "L" if left else "R", len(found)))
            if not found:
                return None
            d[found[0]][2] = True
            return found[0]

        for km, e in d.items():
            n_entries += 1
            if not enough(e):
                continue
            if e[2]:
                info["seen_refused"] += 1
                continue
            e[2] = True
            n_left, n_right = (half - e[1]) & (2 ** 64 - 1), e[1]
            sk = cur = km
            added_l = added_r = 0
            early = False
            while len(sk) != full:
                if n_left:
                    nx = step(cur, True)
                    n_left -= 1
                    if nx:
                        sk = nx[:1] + sk
                        added_l += 1
                    else:
                        n_left = 0
                        early = True
                    if n_left == 0:
                        cur = km
                    elif nx:
                        cur = nx
                elif n_right:
                    nx = step(cur, False)
                    n_right -= 1
                    if not nx:
                        break
                    sk = sk + nx[-1:]
                    added_r += 1
                    cur = nx
                else:
                    break
            n_skm += 1
            if len(sk) == full:
                n_max += 1
                codes += [CODE[c] for c in sk[:half] + sk[k: k + half]]
            else:
                at = sk.find(ms)
                if at < 0:
                    at = len(sk)
                text += sk[:at] + b"\n" + sk[at + m:] + b"\n"
            info["walks"].append((mn, km, added_l, added_r, early, len(sk) == full))
        blob = bytearray()
        if codes:                                                     # strCompressor: the count mod 4, then four codes a byte
            blob.append(len(codes) % 4)
            c = 0
            for i, x in enumerate(codes):
                c = (c + x) & 255
                if (i + 1) % 4 == 0:
                    blob.append(c)
                    c = 0
                c = (c << 2) & 255
            if len(codes) % 4:
                blob.append(c)
        out += len(blob).to_bytes(4, "little") + blob + text + b"\n\n"
        info["blob"][mn], info["text"][mn] = bytes(blob), bytes(text)
    info["buckets"] = sorted(index)
    info["distinct"] = {mn: len(d) for mn, d in index.items()}
    info["counts"] = {mn: {km: e[3] for km, e in d.items()} for mn, d in index.items()}
    counters = dict(zip(COUNTERS, (len(index), n_entries, n_skm, n_max)))
    return bytes(out), counters, info


# ------------------------------------------------------------------------------------------------ the stream builder

class Stream:
    """records and stream entries, in the order they are added"""

    def __init__(self, k, m):
        self.k, self.m = k, m
        self.recs, self.sk = [], []
        self.n_bases = 0

    def pad(self, seq):
        """a record of its own that no entry refers to: moves everything behind it"""
        self.recs.append(seq)
        self.n_bases += len(seq)
        return len(self.recs) - 1

    def add(self, seq, X, rev=0):
        """the oriented super-k-mer `seq` around X as a record of its own (rev: the record holds its reverse complement)"""
        assert len(seq) >= self.k and len(X) == self.m
        rec = self.pad(revcomp(seq) if rev else seq)
        self.sk.append((rec, num(X), 0, len(seq), rev))
        return rec

    def again(self, rec, X, start=0, length=None, rev=0):
        """one more entry over a record that is already there: the same bases once more, or a stretch of them (start and
        length in the record's own direction)"""
        ln = len(self.recs[rec]) - start if length is None else length
        assert ln >= self.k and start + ln <= len(self.recs[rec])
        self.sk.append((rec, num(X), start, ln, rev))

    def done(self, file_sk=None):
        """-> (bases, rec_off, stream, file_sk)"""
        b = np.frombuffer(b"".join(self.recs), np.uint8)
        off = np.zeros(len(self.recs) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in self.recs])
        st = np.array(self.sk, dtype=SUPERKMER_DTYPE) if self.sk else np.zeros(0, SUPERKMER_DTYPE)
        fsk = np.array([0, len(self.sk)] if file_sk is None else file_sk, np.uint32)
        return b, off, st, fsk


def superkmer(rng, k, m, X, q=1, left=None):
    """q k-mers that all hold X: L + X + R with |L| = left (q - 1 <= left <= k - m), k + q - 1 bases in all"""
    if left is None:
        left = rng.randrange(q - 1, k - m + 1)
    assert q - 1 <= left <= k - m and 1 <= q <= k - m + 1
    return rnd(rng, left) + X + rnd(rng, k + q - 1 - left - m)


def maximal(rng, k, m, X):
    """k - m + 1 k-mers: X in the middle of 2k - m bases"""
    return superkmer(rng, k, m, X, k - m + 1, k - m)


def long_superkmer(rng, k, m, X, q):
    """q k-mers, q beyond what a scan emits: X every k - m + 1 bases with other bases in between, so that every window of k
    bases still holds X whole (and no two windows are alike)"""
    period = k - m + 1
    s = bytearray()
    while len(s) < k + q - 1:
        s += X + rnd(rng, period - m)
    return bytes(s[: k + q - 1])


def pieces(seq, k, parts):
    """a super-k-mer cut into `parts` overlapping entries: stretches of consecutive k-mers, each (but the last) reaching one
    k-mer into the next; parts = number of k-mers: one k-mer each.  -> [(start, len)]"""
    q = len(seq) - k + 1
    assert 1 <= parts <= q
    cuts = [q * i // parts for i in range(parts + 1)]
    out = []
    for i in range(parts):
        a, z = cuts[i], min(cuts[i + 1] + (1 if parts < q else 0), q)
        out.append((a, z - a + k - 1))
    return out


def shared_singles(rng, k, m, n, at):
    """n one-k-mer super-k-mers over ONE record of n + k - 1 random bases: entry i is the window at i, its minimizer the m-mer
    at place `at(i)` of that window.  Vectorised: this is how the streams of 2^18 entries stay a quarter of a megabyte."""
    nprng = np.random.default_rng(rng.getrandbits(32))
    g = np.frombuffer(NUC, np.uint8)[nprng.integers(0, 4, n + k - 1)]
    code = ((g >> 1) & 3).astype(np.uint32)
    place = np.asarray([at(i) for i in range(n)] if callable(at) else at, dtype=np.int64)
    pos = np.arange(n, dtype=np.int64) + place
    mn = np.zeros(n, np.uint32)
    for j in range(m):
        mn = (mn << 2) | code[pos + j]
    st = np.zeros(n, SUPERKMER_DTYPE)
    st["minimizer"], st["start"], st["len"] = mn, np.arange(n), k
    return g.copy(), np.array([0, n + k - 1], np.uint64), st
