#!/usr/bin/env python3
"""Cost of the selection (spsp_keys_select_device) next to one prevalence pass (spsp_prevalence_device) over the same arrays on the
same context in the same run.  The selection repeats that pass's table fill and adds a stream compaction (merged: and a sort), so
the prevalence call is the yardstick: the ratio is what is reported, there is no target.

  families  10 000 sketches of ~6 000 keys in families of 20 (BASELINE configs[3]), all versus all
  species   10 000 sketches of ~6 000 keys that are ONE family: every key of the ancestor is held by nearly everybody
  query     the families' arrays with the first 100 sketches as queries against the other 9 900 (each only: merged takes no queries)

Per shape: each and merged, at core=0.9 and union.  Key arrays are synthesised on the device (synth.direct_family_sketches, as
tools/prevalence_bench.py does).  Milliseconds by HIP events around the whole call on the context's stream (its host waits are
inside), first call (allocations) dropped; best and median.  The byte bound next to each: the key bytes read (12 per key at
k <= 32) plus the key bytes written, plus, merged, one read and one write of the written keys per pass of the sort (the chunk
sort and every merge pass), and what those bytes take at 6.3 TB/s, the rate a plain copy reaches on an MI355X.  The table fill's
random accesses are not in the bound: the prevalence call next to it is their measure.  Identities asserted on every result: per row the `each` counts are the prevalence pass's class
counts (core=0.9: core; union: everything but absent), the merged count is the spectrum summed over the band, offsets are
monotone, and the merged keys are strictly increasing.

usage (GPU box): python tools/select_bench.py [families|species|query|all] [reps=5]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import supersampler_amd as sp  # noqa: E402
from supersampler_amd import synth  # noqa: E402

K = 31
N = 10_000
SHAPES = {"families": dict(fam_size=20, n_query=0), "species": dict(fam_size=N, n_query=0), "query": dict(fam_size=20, n_query=100)}
NUM, DEN, CORE = 9, 10, "core=0.9"
KEY_BYTES = 12                                                                    # k <= 32: minimizer u32 + kmer_lo u64
SORT_CHUNK = 2048


def timed(stream, reps, call):
    ev, wall, out = [], [], None
    for r in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(stream)
        out = call()
        b.record(stream)
        b.synchronize()
        if r:
            ev.append(a.elapsed_time(b)); wall.append((time.perf_counter() - t0) * 1e3)
    return out, {"event_ms_best": min(ev), "event_ms_median": float(np.median(ev)), "wall_ms_best": min(wall)}


def sort_passes(count):
    passes, run = 1, SORT_CHUNK                                                   # the chunk sort, then merge passes until one run is left
    while run < count:
        passes, run = passes + 1, run * 2
    return passes if count > 1 else 0


def strictly_increasing(ctx, o_mn, o_lo, count):
    if count < 2:
        return True
    mn, lo = ctx.to_host(o_mn, count, np.uint32).astype(np.uint64), ctx.to_host(o_lo, count, np.uint64)
    return bool(np.all((mn[1:] > mn[:-1]) | ((mn[1:] == mn[:-1]) & (lo[1:] > lo[:-1]))))


def case(ctx, stream, name, reps):
    shape = SHAPES[name]
    nq = shape["n_query"]
    R, n_rows = N - nq, nq if nq else N
    D = synth.direct_family_sketches(N, fam_size=shape["fam_size"], seed=21, device=torch.device("cuda", 0))
    card = np.diff(D.sk_off.astype(np.int64))
    ptrs = (D.minimizer.data_ptr(), D.kmer_lo.data_ptr(), None)
    torch.cuda.synchronize()
    (rows, spectrum), pv = timed(stream, reps, lambda: ctx.prevalence_device(K, *ptrs, D.sk_off, N, NUM, DEN, n_query=nq))
    out = {"shape": name, "sketches": N, "family": shape["fam_size"], "n_query": nq, "keys": int(D.sk_off[-1]), "prevalence": pv, "union": int(spectrum.sum()),
           "largest_h": int(np.nonzero(spectrum)[0].max()), "select": []}
    for word in (CORE, "union"):
        h_min, h_max = sp.select_band(word, R)
        want_rows = rows["core"].astype(np.int64) if word == CORE else card[:n_rows] - rows["absent"].astype(np.int64)
        for merged in (False, True):
            if merged and nq:
                continue
            (o_mn, o_lo, _, off), t = timed(stream, reps, lambda: ctx.select_device(K, *ptrs, D.sk_off, N, h_min, h_max, merged, nq))
            written = int(off[-1])
            assert off[0] == 0 and np.all(np.diff(off.astype(np.int64)) >= 0)
            if merged:
                assert written == int(spectrum[h_min:h_max + 1].sum()) and strictly_increasing(ctx, o_mn, o_lo, written)
            else:
                assert np.array_equal(np.diff(off.astype(np.int64)), want_rows)
            read = int(card[:n_rows].sum()) if not merged else int(card.sum())
            bound = KEY_BYTES * (read + written) + (2 * KEY_BYTES * written * sort_passes(written) if merged else 0)
            out["select"].append(dict(t, what=word, band=[h_min, h_max], form="merged" if merged else "each", host_waits=2 if merged else 1,
                                      keys_read=read, keys_written=written, sort_passes=sort_passes(written) if merged else 0, byte_bound=bound,
                                      bound_ms_at_6_3TBps=bound / 6.3e9, over_prevalence_best=t["event_ms_best"] / pv["event_ms_best"]))
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    stream = torch.cuda.Stream()
    ctx = sp.Context(0, stream=stream.cuda_stream)
    doc = {"tool": "select_bench", "k": K, "library": sp.library_info(), "device": torch.cuda.get_device_name(0), "reps": reps, "shapes": []}
    for name in ("families", "species", "query"):
        if which in ("all", name):
            doc["shapes"].append(case(ctx, stream, name, reps))
    ctx.close()
    print(json.dumps(doc))
