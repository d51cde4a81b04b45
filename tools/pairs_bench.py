#!/usr/bin/env python3
"""Cost of the paired road on one MI355X, stage by stage, from two FASTA texts to rows.

The index and the record sets are classify_bench.py's (10 000 sketches at k = 31, m = 11, s = 4; reads: 10^6 pairs of 2 x 150
bases, contigs: 10^5 pairs of 2 x 5 000 bases).  Mate 2 of a pair is the slice of the same genome that starts INSERT bases
behind mate 1's start (reads: 250, so that the mates share no base; contigs: 2 500, so that they share half), read on the same
strand: canonical k-mers make the strand no matter to the keys.

Per set the paired driver's road with the public calls on three contexts: the ingest and the ONE scan of each text on its side
context, and per batch of 65 535 pairs the two key extractions, spsp_records_union_device on the main context and
spsp_classify_device over the union.  Host wall milliseconds per stage (every call waits for the device before it returns; the
two extractions are timed one after the other here, the driver queues them on two streams), the whole road run twice and the
first run (allocations) dropped; inside the union calls the events between the launches (spsp_union_stage_ms).  Beside it R1
and R2 as two unpaired runs (classify_bench.road).

The yardsticks, measured in the same run:
  extraction   the union per batch against ONE mate's key extraction of that batch.
  byte bound   (|A| + |B|) x 12 bytes read plus the output's keys x 12 bytes written, over the copy rate
               spsp_measure_hbm_device reports in this run, against the union's launches (events).
  two runs     the paired road against the two unpaired runs together.

Asserted: the union's keys per pair lie between the larger mate's and the two mates' sum, and the pairs' rows obey
hit_keys <= keys.

usage (GPU box): python tools/pairs_bench.py [reads|contigs|all]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import supersampler_amd as sp  # noqa: E402
import classify_bench as cb  # noqa: E402

INSERT = {"reads": 250, "contigs": 2500}
DEV = cb.DEV


def make_pair_texts(g_cat, g_off, n_rec, length, insert, seed):
    """two FASTA texts on the device, '>r\\n' + bases + '\\n' per record: mate 2 starts `insert` bases behind mate 1 in the same genome"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    src = torch.randint(0, cb.G, (n_rec,), generator=gen, device=DEV)
    first, size = torch.from_numpy(g_off[:-1]).to(DEV)[src], torch.from_numpy(np.diff(g_off)).to(DEV)[src]
    rel = (torch.rand(n_rec, generator=gen, device=DEV, dtype=torch.float64) * (size - length - insert)).long()
    texts = []
    for start in (first + rel, first + rel + insert):
        text = torch.empty((n_rec, length + 4), dtype=torch.uint8, device=DEV)
        text[:, 0], text[:, 1], text[:, 2], text[:, -1] = ord(">"), ord("r"), ord("\n"), ord("\n")
        step = max(1, (1 << 26) // length)
        for a in range(0, n_rec, step):
            z = min(a + step, n_rec)
            text[a:z, 3:-1] = g_cat[start[a:z, None] + torch.arange(length, device=DEV)[None, :]]
        texts.append(torch.cat([text.reshape(-1), torch.zeros(64, dtype=torch.uint8, device=DEV)]))
    torch.cuda.synchronize()
    return texts, n_rec * (length + 4)


def paired_road(ctx, sides, params, texts, n_text, n_rec):
    ms = {"ingest": 0.0, "scan": 0.0, "keys_1": 0.0, "keys_2": 0.0, "union": 0.0, "classify": 0.0}
    S = []
    for side, text in zip(sides, texts):
        (d_bases, n_bases, d_off, got), t = cb.wall(lambda: side.clean_fasta_device(text.data_ptr(), n_text))
        ms["ingest"] += t
        assert got == n_rec
        (d_sk, n_sk), t = cb.wall(lambda: side.scan_device(params, d_bases, n_bases, d_off, n_rec))
        ms["scan"] += t
        S.append((side, d_bases, n_bases, d_off, d_sk, side.to_host(d_sk, n_sk, sp.SUPERKMER_DTYPE)["rec"]))
    ctx.union_stage_ms(); ctx.classify_stage_ms()
    recs, keys, per_batch = [], [0, 0, 0], []
    for r0 in range(0, n_rec, cb.BATCH):
        r1 = min(r0 + cb.BATCH, n_rec)
        got, t_keys = [], []
        for which, (side, d_bases, n_bases, d_off, d_sk, rec_of) in enumerate(S):
            q0, q1 = (int(x) for x in np.searchsorted(rec_of, [r0, r1]))
            out, t = cb.wall(lambda: side.sketch_keys_device(params, d_bases, n_bases, d_off, d_sk + q0 * sp.SUPERKMER_DTYPE.itemsize, q1 - q0,
                                                             np.arange(r0, r1 + 1, dtype=np.uint32)))
            ms["keys_%d" % (which + 1)] += t
            got.append(out); t_keys.append(t)
        (a_mn, a_lo, _, a_off), (b_mn, b_lo, _, b_off) = got
        (u_mn, u_lo, _, off), t_union = cb.wall(lambda: ctx.records_union_device(cb.K, a_mn, a_lo, None, a_off, b_mn, b_lo, None, b_off))
        ms["union"] += t_union
        na, nb, nu = np.diff(a_off.astype(np.int64)), np.diff(b_off.astype(np.int64)), np.diff(off.astype(np.int64))
        assert np.all(nu >= np.maximum(na, nb)) and np.all(nu <= na + nb)
        (r, _), t = cb.wall(lambda: ctx.classify_device(u_mn, u_lo, None, off, cb.TOP))
        ms["classify"] += t
        recs.append(r)
        keys[0] += int(a_off[-1]); keys[1] += int(b_off[-1]); keys[2] += int(off[-1])
        per_batch.append({"pairs": r1 - r0, "keys_1_ms": t_keys[0], "keys_2_ms": t_keys[1], "union_ms": t_union})
    ms.update({"union_" + f: v for f, v in ctx.union_stage_ms().items()})
    ms.update({"classify_" + f: v for f, v in ctx.classify_stage_ms().items()})
    return np.concatenate(recs), ms, keys, per_batch


def case(ctx, sides, params, index, g_cat, g_off, name, copy_GBps):
    shape = cb.SETS[name]
    n_rec, length = shape["records"], shape["bases"]
    texts, n_text = make_pair_texts(g_cat, g_off, n_rec, length, INSERT[name], 31)
    ctx.classify_index_device(cb.K, index[0].data_ptr(), index[1].data_ptr(), None, index[2], cb.N)
    paired_road(ctx, sides, params, texts, n_text, n_rec)                      # (allocations)
    records, ms, keys, per_batch = paired_road(ctx, sides, params, texts, n_text, n_rec)
    assert np.all(records["hit_keys"] <= records["keys"]) and int(records["keys"].astype(np.int64).sum()) == keys[2]
    road_ms = sum(ms[f] for f in ("ingest", "scan", "keys_1", "keys_2", "union", "classify"))
    unpaired = []
    for text in texts:
        cb.road(ctx, sides[0], params, text, n_text, n_rec)
        _, _, u_ms, u_keys, _ = cb.road(ctx, sides[0], params, text, n_text, n_rec)
        unpaired.append({"stage_ms": u_ms, "keys": u_keys, "road_ms": u_ms["ingest"] + u_ms["scan"] + u_ms["keys"] + u_ms["classify"]})
    full = [b for b in per_batch if b["pairs"] == cb.BATCH] or per_batch
    union_batch = float(np.mean([b["union_ms"] for b in full]))
    keys_batch = float(np.mean([b["keys_1_ms"] for b in full]))
    launches = sum(ms["union_" + f] for f in ("flags", "scan", "offsets", "write"))
    bound_ms = ((keys[0] + keys[1]) * 12 + keys[2] * 12) / (copy_GBps * 1e9) * 1e3
    two = unpaired[0]["road_ms"] + unpaired[1]["road_ms"]
    return {"set": name, "pairs": n_rec, "bases_per_mate": length, "insert": INSERT[name], "keys_mate_1": keys[0], "keys_mate_2": keys[1], "keys_union": keys[2],
            "batches": len(per_batch), "stage_ms": ms, "road_ms": road_ms, "pairs_per_s": n_rec / (road_ms * 1e-3),
            "union_per_full_batch_ms": union_batch, "keys_1_per_full_batch_ms": keys_batch, "union_over_one_extraction": union_batch / keys_batch,
            "union_launches_ms": launches, "union_byte_bound_ms": bound_ms, "union_launches_over_bound": launches / bound_ms,
            "unpaired": unpaired, "two_unpaired_runs_ms": two, "paired_over_two_runs": road_ms / two,
            "paired_minus_two_runs_minus_union_ms": road_ms - two - ms["union"]}


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    ctx, sides = sp.Context(0), (sp.Context(0), sp.Context(0))
    params = sp.make_params(cb.K, cb.M, cb.S)
    hbm = ctx.measure_hbm()
    mn, lo, off, g_cat, g_off = cb.make_index(ctx, params)
    ctx.timing_enable(True)
    doc = {"tool": "pairs_bench", "k": cb.K, "m": cb.M, "s": cb.S, "top": cb.TOP, "library": sp.library_info(), "device": torch.cuda.get_device_name(0),
           "hbm_copy_GBps": hbm["copy_GBps"], "plan": sp.union_plan(), "index": {"sketches": cb.N, "from_genomes": cb.G, "entries": int(off[-1])}, "sets": []}
    for name in ("reads", "contigs"):
        if which in ("all", name):
            doc["sets"].append(case(ctx, sides, params, (mn, lo, off), g_cat, g_off, name, hbm["copy_GBps"]))
    ctx.close()
    for s in sides:
        s.close()
    print(json.dumps(doc))
