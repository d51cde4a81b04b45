#!/usr/bin/env python3
"""Cost of the representatives pass (spsp_representatives_cells_device) next to three yardsticks on the same context in the same
run: the single-linkage pass over the same cells (spsp_cluster_cells_device), the comparison that made the cells
(spsp_compare_cells_device), and a byte bound -- 8 B per cell once + 4 B per edge per round over the copy rate
spsp_measure_hbm_device reports in that run (the assign pass reads the cells a second time: the bound is a floor, not an
estimate).  Reports the rounds and the edges of every call.

  1   10 000 sketches of ~6 000 keys in families of 20 (BASELINE configs[3])
  2   10 000 sketches in families of 1 000 (about 5 x 10^6 cells)
  3   one species: 20 000 sketches that are all related (2 x 10^8 cells, one component); ~150 keys per sketch, so that the
      comparison that makes the cells stays a matter of seconds

Key arrays are synthesised on the device (synth.direct_family_sketches).  Milliseconds by HIP events around the whole call on
the context's stream (its host waits are inside: one per batch of rounds and one for the rows), first call (allocations)
dropped; best and median.

usage (GPU box): python tools/representatives_bench.py [1|2|3|all] [reps=5]
under the profiler: rocprofv3 --kernel-trace --stats -- python tools/representatives_bench.py 3 2"""
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
SHAPES = {"1": dict(n=10_000, fam_size=20, skm_range=(120, 480)), "2": dict(n=10_000, fam_size=1000, skm_range=(120, 480)),
          "3": dict(n=20_000, fam_size=20_000, skm_range=(4, 10))}


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


def case(ctx, stream, name, reps, copy_GBps):
    shape = SHAPES[name]
    n = shape["n"]
    D = synth.direct_family_sketches(n, fam_size=shape["fam_size"], seed=21, device=torch.device("cuda", 0), skm_range=shape["skm_range"])
    card = np.diff(D.sk_off.astype(np.int64))
    per_family = min(shape["fam_size"], n)
    room = int(n * (per_family - 1) // 2 * 1.02) + (1 << 16)
    scratch = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    cells = torch.zeros(room, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.compare_forget()
    n_cells, cmp_t = timed(stream, reps, lambda: ctx.compare_cells_device(K, D.minimizer.data_ptr(), D.kmer_lo.data_ptr(), None, D.sk_off, n, scratch.data_ptr(),
                                                                          cells.data_ptr(), cells.numel()))
    out = {"shape": name, "sketches": n, "family": shape["fam_size"], "keys": int(D.sk_off[-1]), "cells": int(n_cells),
           "comparison": cmp_t, "representatives": {}}
    for label, metric, num, den in (("jaccard_1_2", 0, 1, 2), ("containment_1_10", 1, 1, 10)):
        args = (cells.data_ptr(), n_cells, card, n, metric, num, den)
        (_, single_clusters, _), single_t = timed(stream, reps, lambda: ctx.cluster_cells_device(*args))
        (rows, n_reps, n_edges, rounds), t = timed(stream, reps, lambda: ctx.representatives_cells_device(*args))
        own = rows["representative"] == np.arange(n)
        assert int(rows["size"].astype(np.int64)[own].sum()) == n and n_reps == int(own.sum()) and (rows["shared"] >= 1).all()
        bound = (8.0 * n_cells + 4.0 * n_edges * rounds) / (copy_GBps * 1e9) * 1e3
        out["representatives"][label] = dict(t, edges=int(n_edges), rounds=int(rounds), representatives=int(n_reps), largest=int(rows["size"].max()),
                                             single_linkage=dict(single_t, clusters=int(single_clusters)), byte_bound_ms=bound,
                                             over_single_linkage_best=t["event_ms_best"] / single_t["event_ms_best"],
                                             over_comparison_best=t["event_ms_best"] / cmp_t["event_ms_best"],
                                             over_byte_bound_best=t["event_ms_best"] / max(bound, 1e-9))
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    stream = torch.cuda.Stream()
    ctx = sp.Context(0, stream=stream.cuda_stream)
    hbm = ctx.measure_hbm()
    doc = {"tool": "representatives_bench", "k": K, "library": sp.library_info(), "device": torch.cuda.get_device_name(0), "reps": reps,
           "hbm_copy_GBps": hbm["copy_GBps"], "shapes": []}
    for name in ("1", "2", "3"):
        if which in ("all", name):
            doc["shapes"].append(case(ctx, stream, name, reps, hbm["copy_GBps"]))
    ctx.close()
    print(json.dumps(doc))
