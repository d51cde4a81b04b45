"""What the passes over sorted keys share (DESIGN "What the collection passes share"): the argument front of spsp_prevalence_device,
spsp_keys_select_device, spsp_accumulation_device and spsp_groups_device -- the same bad inputs are refused by all four with the
same return code and text, in the same order of checks, behind each pass's own clearing of its outputs -- and the one keep-flag
kernel behind the groups' marker sketches.

3 sketches of 5, 4 and 6 hand-written keys (4 sketches for the flag kernel), k = 31 and k = 63.  The gather and the downsampling
pass keep fronts of their own (their overflow checks measure other extents): they are not fed here."""
import ctypes as C

import numpy as np
import pytest

import supersampler_amd as sp
import test_groups as tg
import test_prevalence as tp

N = 3
GROUP = np.array([0, 1, 0], dtype=np.uint32)
ORDERS = np.array([[0, 1, 2], [2, 0, 1]], dtype=np.uint32)


def key(k, mn, x):
    """a key whose kmer_hi (k = 63) orders against kmer_lo: the triple sorts by (minimizer, kmer_hi, kmer_lo)"""
    return (mn, 100 - x if k > 32 else 0, x)


def sketches(k):
    return [[key(k, 3, 1), key(k, 3, 2), key(k, 5, 7), key(k, 5, 9), key(k, 8, 4)],
            [key(k, 3, 2), key(k, 5, 9), key(k, 6, 6), key(k, 8, 4)],
            [key(k, 2, 5), key(k, 3, 1), key(k, 3, 2), key(k, 5, 8), key(k, 8, 4), key(k, 9, 1)]]


@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


class Entry:
    """one entry point: call(k, d, off) -> rc with the outputs filled beforehand, cleared() -> what its refusals leave behind"""

    def __init__(self, ctx):
        self.ctx, self.L = ctx, sp.lib()

    def error(self):
        return self.L.spsp_last_error().decode()


class Prevalence(Entry):
    def call(self, k, d, off):
        self.rows, self.spectrum = np.zeros(N, dtype=sp.PREVALENCE_ROW_DTYPE), np.zeros(N + 1, dtype=np.uint64)
        self.held = C.c_void_p(1)
        return self.L.spsp_prevalence_device(self.ctx._h, k, d[0], d[1], d[2], off.ctypes.data, N, 0, 1, 2, self.rows.ctypes.data, self.spectrum.ctypes.data,
                                             C.byref(self.held))

    def cleared(self):                                             # (the front stands in front of its rows: only the array it lends is withdrawn)
        return self.held.value is None


class Select(Entry):
    def call(self, k, d, off):
        self.out = np.full(N + 1, 7, dtype=np.uint64)
        self.ptrs = [C.c_void_p(1) for _ in range(3)]
        return self.L.spsp_keys_select_device(self.ctx._h, k, d[0], d[1], d[2], off.ctypes.data, N, 0, 1, 2, 0, C.byref(self.ptrs[0]), C.byref(self.ptrs[1]),
                                              C.byref(self.ptrs[2]), self.out.ctypes.data)

    def cleared(self):
        return not self.out.any() and all(p.value is None for p in self.ptrs)


class Accumulation(Entry):
    def call(self, k, d, off):
        self.rows = np.full(N * 8, tp.U64, dtype=np.uint64)
        self.pan, self.core = np.full(ORDERS.size, tp.U64, dtype=np.uint64), np.full(ORDERS.size, tp.U64, dtype=np.uint64)
        return self.L.spsp_accumulation_device(self.ctx._h, k, d[0], d[1], d[2], off.ctypes.data, N, ORDERS.ctypes.data, len(ORDERS), self.rows.ctypes.data,
                                               self.pan.ctypes.data, self.core.ctypes.data)

    def cleared(self):
        return not self.rows.any() and not self.pan.any() and not self.core.any()


class Groups(Entry):
    def call(self, k, d, off):
        self.rows, self.members = np.zeros(2, dtype=sp.GROUP_ROW_DTYPE), np.zeros(N, dtype=sp.GROUP_MEMBER_ROW_DTYPE)
        self.rows[:], self.members[:] = (1, 1, 1, 1, 1, 1), (1, 1, 1)
        self.moff = np.ones(3, dtype=np.uint64)
        self.ptrs = [C.c_void_p(1) for _ in range(3)]
        return self.L.spsp_groups_device(self.ctx._h, k, d[0], d[1], d[2], off.ctypes.data, N, GROUP.ctypes.data, 2, 1, 2, 0, 1, self.rows.ctypes.data,
                                         self.members.ctypes.data, 1, C.byref(self.ptrs[0]), C.byref(self.ptrs[1]), C.byref(self.ptrs[2]), self.moff.ctypes.data)

    def cleared(self):
        return not self.rows.view(np.uint64).any() and not self.members.view(np.uint64).any() and not self.moff.any() and all(p.value is None for p in self.ptrs)


ENTRIES = [Prevalence, Select, Accumulation, Groups]


def arrays(k):
    """-> (the three device addresses, the tensors that keep them alive, the offsets)"""
    mn, lo, hi, off, _ = tp.pack(sketches(k), k)
    assert off.tolist() == [0, 5, 9, 15]
    t = tp.upload(mn, lo, hi)
    return [tp.ptr(x) for x in t], t, off


def offsets(*xs):
    return np.array(xs, dtype=np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_same_bad_input_is_refused_the_same_way(ctx, entry, k):
    e = entry(ctx)
    d, alive, off = arrays(k)
    assert e.call(k, d, off) == 0, e.error()
    ctx.compare_keys_unordered(True)
    try:
        assert e.call(k, d, off) == sp.ERR_ARG and "unordered" in e.error() and e.cleared()
    finally:
        ctx.compare_keys_unordered(False)
    for bad_k in (0, 64):
        assert e.call(bad_k, d, off) == sp.ERR_ARG and "1..63" in e.error() and e.cleared(), bad_k
    assert e.call(k, d, offsets(0, 5, 3, 9)) == sp.ERR_ARG and "decrease (sketch 1)" in e.error() and e.cleared()
    # (nothing is allocated for such an extent: the check stands in front of every reserve of the pass, and no array is there to be read)
    assert e.call(k, [None, None, None], offsets(0, 5, 9, 0xfffffff1)) == sp.ERR_OVERFLOW and "too many" in e.error() and e.cleared()
    assert e.call(k, [d[0], None, d[2]], off) == sp.ERR_ARG and "NULL key array" in e.error() and e.cleared()
    if k > 32:
        assert e.call(k, [d[0], d[1], None], off) == sp.ERR_ARG and "NULL key array" in e.error() and e.cleared()
    assert e.call(k, d, off) == 0, e.error()                        # the context after all of that
    del alive


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
def test_two_bad_things_report_the_earlier_check(ctx, entry):
    e = entry(ctx)
    k = 31
    d, alive, off = arrays(k)
    ctx.compare_keys_unordered(True)
    try:
        assert e.call(k, d, offsets(0, 5, 3, 9)) == sp.ERR_ARG and "unordered" in e.error() and e.cleared()
        assert e.call(64, d, offsets(0, 5, 3, 9)) == sp.ERR_ARG and "unordered" in e.error()
    finally:
        ctx.compare_keys_unordered(False)
    assert e.call(64, d, offsets(0, 5, 3, 9)) == sp.ERR_ARG and "1..63" in e.error()
    assert e.call(k, [None, None, None], offsets(0, 5, 3, 0xfffffff1)) == sp.ERR_ARG and "decrease" in e.error()
    assert e.call(k, [None, None, None], offsets(0, 5, 9, 0xfffffff1)) == sp.ERR_OVERFLOW
    del alive


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 5])
@pytest.mark.parametrize("k", [31, 63])
def test_the_groups_flag_keeps_claiming_markers_only(ctx, k, lead):
    """4 sketches in 2 groups of 2, 6 keys, 13 entries.  At 1 / 1 inside and nobody outside: A (sketches 0, 1) is group 0's marker
    and one of its two occurrences did not claim the cell; B (0, 1, 2) and E (everybody) are core in group 0 and no marker -- their
    claimers carry the core bit alone; C (2, 3) is group 1's marker; D and F are held once.  A keep mask that asked for less than
    claim AND marker, or a band that cut the flag bits, would write other marker sketches than the model's"""
    A, B, C_, D, E, F = tp.pool(6, k, salt=60)
    sk = [[A, B, D, E], [A, B, E], [B, C_, E], [C_, E, F]]
    group = [0, 0, 1, 1]
    assert sum(len(s) for s in sk) == 13
    rows, members, markers = tg.check(ctx, sk, k, group, 2, 1, 1, lead=lead)
    assert markers == [[A], [C_]] and [r[3] for r in rows] == [3, 2] and members[0] == (3, 2, 1)
    # one holder outside allowed: B becomes a marker of group 0 too, E stays out
    _, _, markers = tg.check(ctx, sk, k, group, 2, 1, 1, 1, 2, lead=lead)
    assert markers == [sorted([A, B]), [C_]]
