#!/usr/bin/env python3
"""Cost of the groups pass (spsp_groups_device) next to one prevalence pass (spsp_prevalence_device) over the same arrays on the
same context in the same run.  There is no target: the table says what the second table costs.

  families  10 000 sketches of ~6 000 keys in families of 20 (BASELINE configs[3]), labelled by family: 500 groups
  species   10 000 sketches of ~6 000 keys that are ONE family, split in 10 groups (sketch i in group i mod 10): every key of the
            ancestor has a cell in every group, and every cell is counted to about a thousand

Per shape and per inside threshold -- 9 / 10, and 1 / 20, at which every present key of a family is core and the marker sketches
hold millions of keys to move and sort -- with 0 / 1 outside: the call without and with the marker sketches, milliseconds by HIP
events around the call on the context's stream (its host wait, the host's sums and, with markers, the sort's wait are inside),
first call (allocations) dropped; best and median.  Next to them one prevalence call, their ratio, and a byte bound: the entries read twice
(12 bytes each at k = 31) plus two table words per entry (16 bytes), at 6.3 TB/s, the rate a plain copy reaches on an MI355X.
Identities asserted on every result: the groups' entries add up to the collection's; per group marker <= core <= present and
exclusive <= present; the members' core keys of a group add up to at least in_min times its core keys and at most size times;
the members' exclusive keys to at least its exclusive keys; the groups' present keys to at least the distinct keys of the
collection and their exclusive keys to at most that (the prevalence spectrum's sum); the marker offsets are the marker counts'
running sum; without and with markers the rows are the same.

usage (GPU box): python tools/groups_bench.py [families|species|all] [reps=5]"""
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
SHAPES = {"families": dict(fam_size=20, label=lambda i: i // 20, groups=N // 20), "species": dict(fam_size=N, label=lambda i: i % 10, groups=10)}
THRESHOLDS = ((9, 10, 0, 1), (1, 20, 0, 1))


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


def identities(rows, members, moff, group, G, card, spectrum, T):
    size, in_min, _ = sp.groups_bounds(group, G, *T)
    r = {f: rows[f].astype(np.int64) for f in rows.dtype.names}
    assert np.array_equal(r["members"], size) and np.array_equal(r["entries"], np.bincount(group, weights=card, minlength=G).astype(np.int64))
    assert r["entries"].sum() == card.sum()
    assert np.all(r["marker"] <= r["core"]) and np.all(r["core"] <= r["present"]) and np.all(r["exclusive"] <= r["present"])
    m_core = np.bincount(group, weights=members["core"].astype(np.float64), minlength=G).astype(np.int64)
    m_excl = np.bincount(group, weights=members["exclusive"].astype(np.float64), minlength=G).astype(np.int64)
    assert np.all(m_core >= in_min.astype(np.int64) * r["core"]) and np.all(m_core <= size.astype(np.int64) * r["core"]) and np.all(m_excl >= r["exclusive"])
    distinct = int(spectrum.sum())
    assert r["present"].sum() >= distinct >= r["exclusive"].sum()
    if moff is not None:
        assert moff[0] == 0 and np.array_equal(np.diff(moff.astype(np.int64)), r["marker"])


def case(ctx, stream, name, reps):
    shape = SHAPES[name]
    D = synth.direct_family_sketches(N, fam_size=shape["fam_size"], seed=21, device=torch.device("cuda", 0))
    card = np.diff(D.sk_off.astype(np.int64))
    ptrs = (D.minimizer.data_ptr(), D.kmer_lo.data_ptr(), None)
    group = np.array([shape["label"](i) for i in range(N)], dtype=np.uint32)
    G = shape["groups"]
    torch.cuda.synchronize()
    (_, spectrum), pv = timed(stream, reps, lambda: ctx.prevalence_device(K, *ptrs, D.sk_off, N, 9, 10))
    entries = int(D.sk_off[-1])
    bound = entries * (2 * 12 + 2 * 8)
    out = {"shape": name, "sketches": N, "family": shape["fam_size"], "groups": G, "entries": entries, "distinct_keys": int(spectrum.sum()),
           "prevalence": pv, "byte_bound": bound, "bound_ms_at_6_3TBps": bound / 6.3e9, "calls": []}
    for T in THRESHOLDS:
        (rows, members), plain = timed(stream, reps, lambda: ctx.groups_device(K, *ptrs, D.sk_off, N, group, G, *T))
        identities(rows, members, None, group, G, card, spectrum, T)
        (rows_m, members_m, (_, _, _, moff)), marked = timed(stream, reps, lambda: ctx.groups_device(K, *ptrs, D.sk_off, N, group, G, *T, want_markers=True))
        identities(rows_m, members_m, moff, group, G, card, spectrum, T)
        assert rows_m.tobytes() == rows.tobytes() and members_m.tobytes() == members.tobytes()
        out["calls"].append({"threshold": T, "cells": int(rows["present"].sum()), "core": int(rows["core"].sum()), "exclusive": int(rows["exclusive"].sum()),
                             "marker_keys": int(moff[-1]), "largest_region": int(rows["marker"].max()), "groups_call": dict(plain, host_waits=1),
                             "groups_call_with_markers": dict(marked, host_waits=2), "call_over_prevalence_best": plain["event_ms_best"] / pv["event_ms_best"],
                             "with_markers_over_prevalence_best": marked["event_ms_best"] / pv["event_ms_best"],
                             "call_over_bound_best": plain["event_ms_best"] / (bound / 6.3e9)})
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    stream = torch.cuda.Stream()
    ctx = sp.Context(0, stream=stream.cuda_stream)
    doc = {"tool": "groups_bench", "k": K, "library": sp.library_info(), "device": torch.cuda.get_device_name(0), "reps": reps, "shapes": []}
    for name in ("families", "species"):
        if which in ("all", name):
            doc["shapes"].append(case(ctx, stream, name, reps))
    ctx.close()
    print(json.dumps(doc))
