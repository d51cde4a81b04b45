#!/usr/bin/env python3
"""Cost of the linkage tree (spsp_tree_cells_device) next to ONE cluster pass on the same cells (spsp_cluster_cells_device: the
one-threshold answer the tree replaces several runs of) and next to the comparison that made the cells
(spsp_compare_cells_device), on the same context in the same run.  The tree is judged against those two, never against itself.

  families          10 000 sketches of ~6 000 keys in families of 20 (BASELINE configs[3])
  species           10 000 sketches that are all related (5 x 10^7 cells, one component): the contended case, where every live edge
                    of the last rounds offers itself to the same two best-edge words; ~150 keys per sketch, so that the comparison
                    that makes the cells stays a matter of seconds
  species_shuffled  the same cells in a random order

Key arrays are synthesised on the device (synth.direct_family_sketches).  Milliseconds by HIP events around the whole call on
the context's stream (its one host wait, the copy of the forest and the host's ordering of its rows are inside), first call
(allocations) dropped; best and median.  The tree is built at the floor 0 (every cell that shares a key is a candidate) on
Jaccard; the cluster pass runs at Jaccard 1/2.  Every result is held to the cut property: the tree cut at 1/2 IS that clustering.

usage (GPU box): python tools/tree_bench.py [families|species|species_shuffled|all] [reps=5]
under the profiler: rocprofv3 --kernel-trace --stats -- python tools/tree_bench.py species 2"""
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
SHAPES = {"families": dict(n=10_000, fam_size=20, skm_range=(120, 480), shuffle=False),
          "species": dict(n=10_000, fam_size=10_000, skm_range=(4, 10), shuffle=False),
          "species_shuffled": dict(n=10_000, fam_size=10_000, skm_range=(4, 10), shuffle=True)}
JAC = 0
CUT = (1, 2)


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


def case(ctx, stream, name, reps):
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
    del scratch
    if shape["shuffle"]:
        cells = cells[:n_cells][torch.randperm(n_cells, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))].contiguous()
        torch.cuda.synchronize()
    (c_rows, n_clusters, c_edges), cl_t = timed(stream, reps, lambda: ctx.cluster_cells_device(cells.data_ptr(), n_cells, card, n, JAC, *CUT))
    (rows, n_edges, rounds), tr_t = timed(stream, reps, lambda: ctx.tree_cells_device(cells.data_ptr(), n_cells, card, n, JAC, 0, 1))
    # step 5: the tree cut at the cluster pass's threshold is the cluster pass's answer; at the floor, what is left are the components
    cluster, count = sp.tree_cut(rows, card, JAC, 0, 1, *CUT)
    assert count == n_clusters and np.array_equal(cluster, c_rows["cluster"]), name
    assert n_edges == n_cells and len(rows) == n - sp.tree_cut(rows, card, JAC, 0, 1, 0, 1)[1]
    return {"shape": name, "sketches": n, "family": shape["fam_size"], "keys": int(D.sk_off[-1]), "cells": int(n_cells), "comparison": cmp_t,
            "cluster_jaccard_1_2": dict(cl_t, edges=int(c_edges), clusters=int(n_clusters)),
            "tree_jaccard_floor_0": dict(tr_t, candidate_edges=int(n_edges), rows=int(len(rows)), rounds_that_hooked=int(rounds),
                                         over_cluster_best=tr_t["event_ms_best"] / cl_t["event_ms_best"],
                                         over_comparison_best=tr_t["event_ms_best"] / cmp_t["event_ms_best"])}


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    stream = torch.cuda.Stream()
    ctx = sp.Context(0, stream=stream.cuda_stream)
    doc = {"tool": "tree_bench", "k": K, "library": sp.library_info(), "device": torch.cuda.get_device_name(0), "reps": reps, "shapes": []}
    for name in SHAPES:
        if which in ("all", name):
            doc["shapes"].append(case(ctx, stream, name, reps))
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps(doc))
