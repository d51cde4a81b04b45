#!/usr/bin/env python3
"""Cost of the accumulation curves (spsp_accumulation_device) next to one prevalence pass (spsp_prevalence_device) over the same
arrays on the same context in the same run.  There is no target: the table says what the transposition buys.

  families  10 000 sketches of ~6 000 keys in families of 20 (BASELINE configs[3])
  species   10 000 sketches of ~6 000 keys that are ONE family: every key of the ancestor is held by nearly everybody, so nearly
            every list is thousands of holders long

Per shape: the whole call at P = 1 and at P = 101 orders (spsp_accumulation_orders_host, seed 1), milliseconds by HIP events around
the call on the context's stream (its one host wait and the host's prefix sums are inside), first call (allocations) dropped; best
and median.  From the two: the part built once per call (table fill, scans, scatter -- and the host's share of one order) as
t(1) - marginal, and the marginal cost per order (t(101) - t(1)) / 100.  Next to them one prevalence call, and the byte bound per
group of orders: the list bytes (2 per entry) plus the key records (4 per distinct key), read once, at 6.3 TB/s, the rate a plain
copy reaches on an MI355X; per order that is the bound divided by the orders one pass serves.  `cuts`: the P = 101 call once more
per list length at which a lane hands its list to the wave (SPSP_DEBUG_ACCUMULATION_CUT), the same number of repetitions each.
Identities asserted on every result: pan(n) is the spectrum's sum and core(n) its last word, pan(1) = core(1) = the first sketch's
keys, pan never falls and core never rises, for every order; the rows are the curves' minimum, maximum and sum.

usage (GPU box): python tools/accumulation_bench.py [families|species|all] [reps=5]"""
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
SHAPES = {"families": dict(fam_size=20), "species": dict(fam_size=N)}
ORDERS = (1, 101)
CUTS = (8, 16, 32, 64)


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


def identities(rows, pan, core, orders, card, spectrum):
    n = len(card)
    assert np.all(pan[:, -1] == spectrum[1:].sum()) and np.all(core[:, -1] == spectrum[n])
    assert np.array_equal(pan[:, 0], card[orders[:, 0]]) and np.array_equal(core[:, 0], card[orders[:, 0]])
    assert np.all(np.diff(pan.astype(np.int64), axis=1) >= 0) and np.all(np.diff(core.astype(np.int64), axis=1) <= 0)
    for name, a in (("pan", pan), ("core", core)):
        assert np.array_equal(rows[name + "_min"], a.min(axis=0)) and np.array_equal(rows[name + "_max"], a.max(axis=0))
        assert np.array_equal(rows[name + "_sum"], a.sum(axis=0)) and np.array_equal(rows[name + "_first"], a[0])


def case(ctx, stream, name, reps):
    D = synth.direct_family_sketches(N, fam_size=SHAPES[name]["fam_size"], seed=21, device=torch.device("cuda", 0))
    card = np.diff(D.sk_off.astype(np.int64)).astype(np.uint64)
    ptrs = (D.minimizer.data_ptr(), D.kmer_lo.data_ptr(), None)
    torch.cuda.synchronize()
    plan = sp.accumulation_plan(N)
    (_, spectrum), pv = timed(stream, reps, lambda: ctx.prevalence_device(K, *ptrs, D.sk_off, N, 9, 10))
    entries, distinct = int(D.sk_off[-1]), int(spectrum.sum())
    bound = 2 * entries + 4 * (distinct + 1)
    out = {"shape": name, "sketches": N, "family": SHAPES[name]["fam_size"], "entries": entries, "distinct_keys": distinct,
           "largest_h": int(np.nonzero(spectrum)[0].max()), "plan": plan, "prevalence": pv, "group_byte_bound": bound,
           "group_bound_ms_at_6_3TBps": bound / 6.3e9, "order_bound_ms_at_6_3TBps": bound / 6.3e9 / plan["group"], "calls": [], "cuts": []}
    t = {}
    for P in ORDERS:
        orders = sp.accumulation_orders(N, P, 1)
        (rows, pan, core), t[P] = timed(stream, reps, lambda: ctx.accumulation_device(K, *ptrs, D.sk_off, N, orders, want_curves=True))
        identities(rows, pan, core, orders, card, spectrum)
        out["calls"].append(dict(t[P], orders=P, passes=(P + plan["group"] - 1) // plan["group"], host_waits=1))
    for which in ("event_ms_best", "event_ms_median"):
        marginal = (t[101][which] - t[1][which]) / 100.0
        out["marginal_per_order_" + which] = marginal
        out["built_once_" + which] = t[1][which] - marginal
    out["built_once_over_prevalence_best"] = out["built_once_event_ms_best"] / pv["event_ms_best"]
    out["marginal_over_prevalence_best"] = out["marginal_per_order_event_ms_best"] / pv["event_ms_best"]
    out["marginal_over_order_bound_best"] = out["marginal_per_order_event_ms_best"] / out["order_bound_ms_at_6_3TBps"]
    orders = sp.accumulation_orders(N, 101, 1)
    for cut in CUTS:
        os.environ["SPSP_DEBUG_ACCUMULATION_CUT"] = str(cut)
        (rows, pan, core), tc = timed(stream, reps, lambda: ctx.accumulation_device(K, *ptrs, D.sk_off, N, orders, want_curves=True))
        identities(rows, pan, core, orders, card, spectrum)
        out["cuts"].append(dict(tc, cut=cut))
    del os.environ["SPSP_DEBUG_ACCUMULATION_CUT"]
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    stream = torch.cuda.Stream()
    ctx = sp.Context(0, stream=stream.cuda_stream)
    doc = {"tool": "accumulation_bench", "k": K, "library": sp.library_info(), "device": torch.cuda.get_device_name(0), "reps": reps, "shapes": []}
    for name in ("families", "species"):
        if which in ("all", name):
            doc["shapes"].append(case(ctx, stream, name, reps))
    ctx.close()
    print(json.dumps(doc))
