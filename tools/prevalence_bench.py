#!/usr/bin/env python3
"""Cost of the prevalence pass (spsp_prevalence_device) next to one comparison of the same arrays (spsp_compare_cells_device) on
the same context in the same run.  Nobody has measured this pass before: there is no target, the ratio to that comparison is
what is reported.

  families  10 000 sketches of ~6 000 keys in families of 20 (BASELINE configs[3]), all versus all
  species   10 000 sketches of ~6 000 keys that are ONE family: every key of the ancestor is held by nearly everybody
  query     the families' arrays with the first 100 sketches as queries against the other 9 900

Key arrays are synthesised on the device (synth.direct_family_sketches, as tools/c4_compare.py does).  Milliseconds by HIP
events around the whole call on the context's stream (its one host wait is inside), first call (allocations) dropped; best and
median.  Each result is checked against its identities: the classes add up to the key counts, sum t * S[t] = the references'
keys, and (all versus all) holders - keys = twice the cells' counts summed.

usage (GPU box): python tools/prevalence_bench.py [families|species|query|all] [reps=5]
under the profiler: rocprofv3 --kernel-trace --stats -- python tools/prevalence_bench.py species 2"""
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
NUM, DEN = 95, 100
HOST_WAITS = 1                                                                    # by construction: one hipStreamSynchronize per call


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
    nq = shape["n_query"]
    D = synth.direct_family_sketches(N, fam_size=shape["fam_size"], seed=21, device=torch.device("cuda", 0))
    card = np.diff(D.sk_off.astype(np.int64))
    ptrs = (D.minimizer.data_ptr(), D.kmer_lo.data_ptr(), None)
    torch.cuda.synchronize()
    (rows, spectrum), t = timed(stream, reps, lambda: ctx.prevalence_device(K, *ptrs, D.sk_off, N, NUM, DEN, n_query=nq))
    n_rows = nq if nq else N
    classes = sum(rows[f].astype(np.int64) for f in ("core", "shell", "unique", "absent"))
    assert np.array_equal(classes, card[:n_rows])
    t_s = np.arange(len(spectrum), dtype=np.int64) * spectrum.astype(np.int64)
    assert int(t_s.sum()) == int(card[nq:].sum())
    out = {"shape": name, "sketches": N, "family": shape["fam_size"], "n_query": nq, "keys": int(D.sk_off[-1]), "threshold": "%d/%d" % (NUM, DEN),
           "host_waits": HOST_WAITS, "prevalence": t, "union": int(spectrum.sum()), "largest_h": int(np.nonzero(spectrum)[0].max()),
           "core_keys_per_row": float(rows["core"].mean()), "absent_keys_per_row": float(rows["absent"].mean()),
           "mean_holders": float(rows["holders"].sum() / max(card[:n_rows].sum(), 1))}
    # the yardstick: one comparison of the same arrays as cells (the rows of the queries in query mode)
    per_family = min(shape["fam_size"], N)
    room = int(N * (per_family - 1) // 2 * 1.02) + (1 << 16)
    scratch = torch.zeros((N, N), dtype=torch.int32, device="cuda")
    cells = torch.zeros(room, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.compare_forget()
    n_cells, cmp_t = timed(stream, reps, lambda: ctx.compare_cells_device(K, *ptrs, D.sk_off, N, scratch.data_ptr(), cells.data_ptr(), cells.numel(),
                                                                          n_query=nq if nq else None))
    out["comparison"] = dict(cmp_t, cells=int(n_cells))
    out["over_comparison_best"] = t["event_ms_best"] / cmp_t["event_ms_best"]
    if not nq:
        shared = int((cells[:n_cells] & 0xFFFFFFFF).sum().item())
        assert int(rows["holders"].astype(np.int64).sum()) - int(card.sum()) == 2 * shared
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    stream = torch.cuda.Stream()
    ctx = sp.Context(0, stream=stream.cuda_stream)
    doc = {"tool": "prevalence_bench", "k": K, "library": sp.library_info(), "device": torch.cuda.get_device_name(0), "reps": reps, "shapes": []}
    for name in ("families", "species", "query"):
        if which in ("all", name):
            doc["shapes"].append(case(ctx, stream, name, reps))
    ctx.close()
    print(json.dumps(doc))
