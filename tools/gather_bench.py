#!/usr/bin/env python3
"""Cost of a gather (spsp_gather_device) next to ONE query-mode comparison of the same arrays (spsp_compare_cells_device with
the same n_query: what round 1 alone costs without it), on the same context in the same run.

  a   one query of ~10^6 keys holding 50 of 10 000 references of ~6 000 keys each
  b   the same with 150 members
  c   32 such queries (50 members each, different ones) in one call

Key arrays are synthesised on the device: per sketch ~300 random minimizers x 20 keys, sorted by (minimizer, k-mer) as the
decoder leaves them; a query = the keys of its members + random keys up to 10^6, sorted.  Milliseconds by HIP events around
the whole call on the context's stream (its host waits are inside), first call (allocations) dropped; best and median.
`host_waits` is computed from the rows, not counted: one wait for the match count + one per batch of 32, 64, 128, 128, ...
rounds until the last query has stopped.

usage (GPU box): python tools/gather_bench.py [a|b|c|all] [reps=5]
under the profiler: rocprofv3 --kernel-trace --stats -- python tools/gather_bench.py b 2"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import supersampler_amd as sp  # noqa: E402

K, M = 31, 11
N_REF, PER, Q_KEYS = 10_000, 6_000, 1_000_000
LO_BITS = 40                                                                      # k-mer values below 2^40: (minimizer, k-mer) sorts as one 62-bit word


def sorted_words(n, per, gen):
    """n rows of `per` composite keys minimizer << 40 | k-mer, each row sorted: per / 20 minimizers x 20 k-mers"""
    runs = per // 20
    mn = torch.randint(0, 4 ** M, (n, runs), generator=gen, device="cuda", dtype=torch.int64).repeat_interleave(20, dim=1)
    lo = torch.randint(0, 1 << LO_BITS, (n, runs * 20), generator=gen, device="cuda", dtype=torch.int64)
    return ((mn << LO_BITS) | lo).sort(dim=1).values


def build(n_query, members, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    refs = sorted_words(N_REF, PER, gen)
    per = refs.shape[1]
    rng = np.random.default_rng(seed)
    queries, named = [], []
    for q in range(n_query):
        pick = np.sort(rng.permutation(N_REF)[:members])
        named.append(pick)
        own = refs[torch.from_numpy(pick).cuda()].reshape(-1)
        fill = sorted_words(1, Q_KEYS - own.numel(), gen).reshape(-1)
        queries.append(torch.unique(torch.cat([own, fill])))                     # (sorted, distinct)
    words = torch.cat(queries + [refs.reshape(-1)])
    off = np.concatenate([[0], np.cumsum([x.numel() for x in queries]), np.cumsum([x.numel() for x in queries])[-1] + per * np.arange(1, N_REF + 1)]).astype(np.uint64)
    mn = (words >> LO_BITS).to(torch.int32).contiguous()
    lo = (words & ((1 << LO_BITS) - 1)).contiguous()
    return mn, lo, off, named


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


def host_waits(rows, n_query):
    rounds = 1 + max(int((rows["query"] == q).sum()) for q in range(n_query))     # (the launch that stops the last query)
    waits, batch, done = 1, 32, 0
    while done < rounds:
        done += batch; waits += 1; batch = min(128, batch * 2)
    return waits


def case(ctx, stream, name, n_query, members, reps):
    mn, lo, off, named = build(n_query, members, 11 + members + n_query)
    n = n_query + N_REF
    torch.cuda.synchronize()
    scratch = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    cells = torch.zeros(1 << 22, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.compare_forget()
    n_cells, cmp_t = timed(stream, reps, lambda: ctx.compare_cells_device(K, mn.data_ptr(), lo.data_ptr(), None, off, n, scratch.data_ptr(), cells.data_ptr(),
                                                                          cells.numel(), n_query=n_query))
    rows, g_t = timed(stream, reps, lambda: ctx.gather_device(K, mn.data_ptr(), lo.data_ptr(), None, off, n, n_query, 25))
    for q in range(n_query):                                                      # every member is named, and nobody else
        got = np.sort(rows["match"][rows["query"] == q].astype(np.int64) - n_query)
        assert np.array_equal(got, named[q]), (name, q)
    return {"case": name, "queries": n_query, "members_per_query": members, "references": N_REF, "keys": int(off[-1]), "query_keys": int(off[n_query]),
            "rows": int(len(rows)), "host_waits": host_waits(rows, n_query), "gather": g_t, "one_query_mode_comparison": dict(cmp_t, cells=int(n_cells)),
            "gather_over_comparison_best": g_t["event_ms_best"] / cmp_t["event_ms_best"]}


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    stream = torch.cuda.Stream()
    ctx = sp.Context(0, stream=stream.cuda_stream)
    doc = {"tool": "gather_bench", "k": K, "m": M, "library": sp.library_info(), "device": torch.cuda.get_device_name(0), "reps": reps, "cases": []}
    for name, nq, mem in (("a", 1, 50), ("b", 1, 150), ("c", 32, 50)):
        if which in ("all", name):
            doc["cases"].append(case(ctx, stream, name, nq, mem, reps))
    ctx.close()
    print(json.dumps(doc))
