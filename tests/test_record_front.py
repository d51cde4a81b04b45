"""What the record passes share (DESIGN "What the record passes share"): the call front of spsp_classify_device and
spsp_taxonomy_device, whose key-array checks spsp_depth_add_device has as well -- the same bad inputs are refused with the same
return code and, up to the pass's name, the same text, in the same order of checks, behind each pass's own clearing of its
outputs -- and the per-call device arrays the two record calls take turns on.

3 references of 5, 4 and 6 hand-written keys, 2 records (and an empty one in the mixed batch), k = 31 and k = 63.  The record
count's refusal is not fed: the outputs are cleared record by record in front of it, so it takes arrays of 2^32 records."""

import numpy as np
import pytest

import supersampler_amd as sp
import test_classify as tc
import test_prevalence as tp
import test_taxonomy as tt

NONE = sp.TAXONOMY_NONE
SEVENS = 0x0707070707070707
LINEAGES = [("B", "E"), ("B", "S"), ("B",)]
NO_INDEX = "%s: the context holds no index (spsp_classify_index_device first; a prevalence, select, accumulation or groups call replaces it)"
NO_TAXONOMY = "taxonomy: the index holds no taxonomy (spsp_taxonomy_index_device first; it ends with the index it was attached to)"
NO_COUNTERS = "depth: the context holds no counters (spsp_depth_begin_device first; they end with the index they were made for)"
DECREASE = "record offsets must not decrease (record %u)"
TOO_MANY_KEYS = "too many record keys for one call"
NULL_KEYS = "NULL key array"
WRAP = "depth: more than 4 294 967 295 record keys since spsp_depth_begin_device (a 32-bit counter could wrap)"


def kmer_hi_text(name, k):
    """the index was built for k, the records come the other way"""
    return "%s: the index was built %s kmer_hi (k %s 32), the records come %s it" % ((name, "with", ">", "without") if k > 32 else (name, "without", "<=", "with"))


def key(k, mn, x):
    """a key whose kmer_hi (k = 63) orders against kmer_lo: the triple sorts by (minimizer, kmer_hi, kmer_lo)"""
    return (mn, 100 - x if k > 32 else 0, x)


def references(k):
    return [[key(k, 3, 1), key(k, 3, 2), key(k, 5, 7), key(k, 5, 9), key(k, 8, 4)],
            [key(k, 3, 2), key(k, 5, 9), key(k, 6, 6), key(k, 8, 4)],
            [key(k, 2, 5), key(k, 3, 1), key(k, 3, 2), key(k, 5, 8), key(k, 8, 4), key(k, 9, 1)]]


def records(k):
    """one record with hits (5 of its 6 keys are held: by all three, by two, by one) and one without"""
    return [[key(k, 3, 2), key(k, 5, 9), key(k, 6, 6), key(k, 2, 5), key(k, 8, 4), key(k, 9, 9)],
            [key(k, 4, 4), key(k, 7, 7), key(k, 8, 5)]]


class Entry:
    """one entry point: call(d, off) -> rc with the outputs filled with sevens beforehand, cleared() -> what its refusals leave"""

    def __init__(self, ctx):
        self.ctx, self.L = ctx, sp.lib()

    def error(self):
        return self.L.spsp_last_error().decode()

    def refuses(self, d, off, code, text, **how):
        rc = self.call(d, off, **how)
        assert (rc, self.error()) == (code, text) and self.cleared()


class Classify(Entry):
    name = "classification"

    def call(self, d, off, top=2, rule=(1, 0, 1)):
        n = len(off) - 1
        self.top_valid = 1 <= top <= 64
        self.records = np.full(n * 3, SEVENS, dtype=np.uint64).view(sp.CLASSIFY_RECORD_DTYPE)
        self.hits = np.full(n * 64, SEVENS, dtype=np.uint64).view(sp.CLASSIFY_HIT_DTYPE)
        self.used = n * top if self.top_valid else 0
        return self.L.spsp_classify_device(self.ctx._h, d[0], d[1], d[2], off.ctypes.data, n, top, *rule, self.records.ctypes.data, self.hits.ctypes.data)

    def cleared(self):
        """the four counts are zero, the hits are zero where `top` says how many there are and untouched beyond, the lengths are the caller's"""
        r, h = self.records, self.hits.view(np.uint64)
        return (not any(r[f].any() for f in ("keys", "hit_keys", "passing", "listed")) and (r["length"] == SEVENS).all() and not h[:self.used].any()
                and (h[self.used:] == SEVENS).all())


class Taxonomy(Entry):
    name = "taxonomy"

    def call(self, d, off, rule=(1, 0, 1)):
        n = len(off) - 1
        self.records = np.full(n * 5, SEVENS, dtype=np.uint64).view(sp.TAXONOMY_RECORD_DTYPE)
        return self.L.spsp_taxonomy_device(self.ctx._h, d[0], d[1], d[2], off.ctypes.data, n, *rule, self.records.ctypes.data)

    def cleared(self):
        """every field but the length is zero: node and start are 0 here, not NONE"""
        return tt.as_rows(self.records) == [(0,) * 8] * len(self.records) and (self.records["length"] == SEVENS).all()


class DepthAdd(Entry):
    name = "depth"

    def call(self, d, off):
        return self.L.spsp_depth_add_device(self.ctx._h, d[0], d[1], d[2], int(off[0]), int(off[-1]) - int(off[0]))

    def cleared(self):
        return True


def offsets(*xs):
    return np.array(xs, dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare():
    """a context that never saw an index"""
    c = sp.Context(0)
    yield c
    c.close()


class Batch:
    """the two records on the device, and the key arrays of the other k for the kmer_hi refusals"""

    def __init__(self, k):
        mn, lo, hi, self.off, _ = tp.pack(records(k), k)
        assert self.off.tolist() == [0, 6, 9]
        self.alive = tp.upload(mn, lo, hi if hi is not None else lo)             # (k = 31: a third array all the same, for the wrong side)
        self.d = [tp.ptr(x) for x in self.alive]
        self.right = self.d if k > 32 else [self.d[0], self.d[1], None]
        self.wrong = [self.d[0], self.d[1], None] if k > 32 else self.d


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_same_bad_input_is_refused_the_same_way(ctx, bare, k):
    b = Batch(k)
    nothing = [None, None, None]
    for entry in (Classify, Taxonomy):                                            # no index: behind the offsets, in front of the key arrays
        e = entry(bare)
        e.refuses(b.right, b.off, sp.ERR_ARG, NO_INDEX % e.name)
    index = tc.Index(ctx, k, references(k))
    assert index.off.tolist() == [0, 5, 9, 15]
    Taxonomy(ctx).refuses(b.right, b.off, sp.ERR_ARG, NO_TAXONOMY)                # an index, no tree on it
    DepthAdd(ctx).refuses(b.right, b.off, sp.ERR_ARG, NO_COUNTERS)                # ... and no counters
    tax = tt.Tax(ctx, k, references(k), LINEAGES, index=index)
    ctx.depth_begin()
    entries = [Classify(ctx), Taxonomy(ctx), DepthAdd(ctx)]
    for e in entries:
        assert e.call(b.right, b.off) == 0, e.error()
    for e in entries[:2]:                                                         # (the depth pass takes an extent, no offsets)
        e.refuses(b.right, offsets(0, 6, 5), sp.ERR_ARG, DECREASE % 1)
        e.refuses(b.right, offsets(7, 6, 9), sp.ERR_ARG, DECREASE % 0)
    for e in entries:
        # (nothing is allocated for such an extent, and no array is there to be read)
        e.refuses(b.right, offsets(0, 6, 0xfffffff1), sp.ERR_OVERFLOW, TOO_MANY_KEYS)
        e.refuses([None, b.d[1], b.right[2]], b.off, sp.ERR_ARG, NULL_KEYS)
        e.refuses([b.d[0], None, b.right[2]], b.off, sp.ERR_ARG, NULL_KEYS)
        e.refuses(b.wrong, b.off, sp.ERR_ARG, kmer_hi_text(e.name, k))
        assert e.call(nothing, offsets(0, 0, 0)) == 0, e.error()                  # no key: no array is asked for
    for e in entries:
        assert e.call(b.right, b.off) == 0, e.error()                             # the context after all of that
    assert tc.as_rows(entries[0].records, entries[0].hits[:4].reshape(2, 2)) == tc.model(references(k), records(k), 2)
    assert tt.as_rows(entries[1].records) == tax.want(records(k))
    assert tuple(int(x) for x in ctx.depth_read()[1]) == (2 * 9, 2 * 5, 9, 5)    # the two good adds, and nothing of the refused ones
    del index, tax, b


@pytest.mark.gpu
def test_two_bad_things_report_the_earlier_check(ctx, bare):
    k = 31
    b = Batch(k)
    nothing = [None, None, None]
    for e in (Classify(bare), Taxonomy(bare)):
        # the threshold | the offsets | the key count | no index | the key arrays
        e.refuses(b.right, offsets(0, 6, 5), sp.ERR_ARG, "%s: min_keys is 1 at the least" % e.name, rule=(0, 0, 1))
        e.refuses(b.right, offsets(0, 6, 5), sp.ERR_ARG, "%s threshold 2 / 1: needs 0 <= num <= den, 1 <= den <= 1000000" % e.name, rule=(1, 2, 1))
        e.refuses(nothing, offsets(7, 6, 0xfffffff1), sp.ERR_ARG, DECREASE % 0)
        e.refuses(nothing, offsets(0, 6, 0xfffffff1), sp.ERR_OVERFLOW, TOO_MANY_KEYS)
        e.refuses(nothing, b.off, sp.ERR_ARG, NO_INDEX % e.name)
    e = Classify(bare)                                                            # the matches per record in front of the threshold: the hits stay as they were
    for top in (0, 65):
        e.refuses(b.right, b.off, sp.ERR_ARG, "classification lists 1 .. 64 matches per record (top = %u)" % top, top=top, rule=(0, 0, 1))
    index = tc.Index(ctx, k, references(k))
    # no taxonomy stands between no index (above) and the key arrays; depth: no counters in front of the key arrays
    Taxonomy(ctx).refuses(nothing, b.off, sp.ERR_ARG, NO_TAXONOMY)
    Taxonomy(ctx).refuses(nothing, offsets(0, 6, 0xfffffff1), sp.ERR_OVERFLOW, TOO_MANY_KEYS)
    DepthAdd(ctx).refuses(nothing, b.off, sp.ERR_ARG, NO_COUNTERS)
    DepthAdd(ctx).refuses(nothing, offsets(0, 6, 0xfffffff1), sp.ERR_ARG, NO_COUNTERS)
    tax = tt.Tax(ctx, k, references(k), LINEAGES, index=index)
    ctx.depth_begin()
    for e in (Classify(ctx), Taxonomy(ctx), DepthAdd(ctx)):
        e.refuses([None, b.d[1], b.d[2]], b.off, sp.ERR_ARG, NULL_KEYS)           # a NULL array in front of a kmer_hi too many
        e.refuses([None, b.d[1], b.d[2]], offsets(0, 6, 0xfffffff1), sp.ERR_OVERFLOW if e.name != "depth" else sp.ERR_ARG,
                  TOO_MANY_KEYS if e.name != "depth" else NULL_KEYS)              # the record calls: the key count first; depth: the arrays first
    DepthAdd(ctx).refuses(b.wrong, offsets(0, 6, 0xfffffff1), sp.ERR_ARG, kmer_hi_text("depth", k))
    del tax, index
    # depth's two overflows, on an index without a key (an add to it launches nothing, so no array is read)
    empty = tc.Index(ctx, k, [[], [], []])
    ctx.depth_begin()
    e = DepthAdd(ctx)
    assert e.call(b.right, offsets(0, 0xfffffff0)) == 0, e.error()
    e.refuses(b.right, offsets(0, 0xfffffff1), sp.ERR_OVERFLOW, TOO_MANY_KEYS)    # this call's extent in front of the sum since begin
    e.refuses(b.right, offsets(0, 0x10), sp.ERR_OVERFLOW, WRAP)
    assert e.call(b.right, offsets(0, 0xf)) == 0, e.error()
    assert int(ctx.depth_read()[1]["record_keys"]) == 0xffffffff                   # the refused adds added nothing
    del empty, b


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_a_mixed_batch_twice_with_the_two_calls_taking_turns(ctx, k):
    """an empty record (its row is the caller's cleared one), a record without a hit (written by the route kernel) and one with hits
    (the wave form): the two calls use the same per-call arrays on the device, rows of 16 bytes and rows of 32"""
    refs = references(k)
    batch = [[], records(k)[1], records(k)[0]]
    tax = tt.Tax(ctx, k, refs, LINEAGES)
    want_c, want_t = tc.model(refs, batch, 2, 2, 1, 3), tax.want(batch, 2, 1, 3)
    assert [r[:2] for r in want_t] == [(0, 0), (3, 0), (6, 5)] and want_t[1][2:4] == (NONE, NONE) and want_t[2][2] != NONE
    for _ in range(2):
        assert tc.run(ctx, k, batch, 2, 2, 1, 3) == want_c
        assert tt.run(ctx, k, batch, 2, 1, 3) == want_t
    assert tc.run(ctx, k, batch, 2, 2, 1, 3, shuffle=5) == want_c
    del tax
