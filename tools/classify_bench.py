#!/usr/bin/env python3
"""Cost of the classification on one MI355X, stage by stage, from FASTA text to rows.

The index: 10 000 sketches -- 9 800 synthesised at the key level (synth.direct_family_sketches, as groups_bench.py makes them) and
200 sketched here from synthetic genomes of 100 kbp in 10 families at k = 31, m = 11, s = 4, so that records cut from those
genomes have holders to tally.  The record sets, as FASTA text made on the device (nine records in ten are slices of the 200
genomes, one in ten is random):

  reads    10^6 records of 150 bases
  contigs  10^5 records of 5 000 bases

Per set the file driver's road with the public calls, on two contexts as the driver uses them: the ingest of the text
(spsp_fasta_clean_device), ONE scan (spsp_scan_device), and per batch of 65 535 records the key extraction
(spsp_sketch_keys_device over the batch's stretch of the super-k-mer stream) and spsp_classify_device.  Host wall milliseconds per
stage (every call waits for the device before it returns), the whole road run twice and the first run (allocations) dropped;
inside the classify calls the events between the launches (spsp_classify_stage_ms): probe, route, and the two forms, in each of
which tally and selection are one kernel.  Records/s and bases/s over the whole road and over the classify calls alone.

The two yardsticks:
  byte bound   keys probed x (8 bytes of slot + 12 bytes of key) + the sum of the holder counts x 2 bytes, over the copy rate
               spsp_measure_hbm_device reports in this run.  The sum of the holder counts is taken exactly -- the prevalence
               rows' `holders` -- over the first 55 535 records and scaled to the set by its keys.
  comparison   the query-mode comparison as cells (spsp_compare_cells_device) plus the neighbours pass at top 1 over the SAME
               55 535 records and the same index arrays (55 535 + 10 000 = 65 535 sketches, the most one call takes), next to
               one classify call over those records.  The neighbours' best partner must be the classification's.

Asserted: hit_keys <= keys, listed = min(top, passing), and all but one in a thousand of the records cut from a genome share every
key with their best match.

usage (GPU box): python tools/classify_bench.py [reads|contigs|all]"""
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

K, M, S = 31, 11, 4.0
N, G, GENOME = 10_000, 200, 100_000
SETS = {"reads": dict(records=1_000_000, bases=150), "contigs": dict(records=100_000, bases=5000)}
BATCH, YARD = 65_535, 65_535 - N
TOP = 1
DEV = torch.device("cuda", 0)


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def device_keys(ctx, d_mn, d_lo, total):
    """a context's key arrays -> tensors of the caller's"""
    mn = torch.from_numpy(ctx.to_host(d_mn, total, np.uint32).view(np.int32)).to(DEV)
    lo = torch.from_numpy(ctx.to_host(d_lo, total, np.uint64).view(np.int64)).to(DEV)
    return mn, lo


def make_index(ctx, params):
    genomes = synth.family_genomes(3, G, GENOME, 10, [0.0, 0.01, 0.03])
    allb, allo = synth.concat_records(genomes)
    g_cat = torch.from_numpy(np.concatenate([allb, np.zeros(64, np.uint8)])).to(DEV)
    d_o = torch.from_numpy(allo.view(np.int64)).to(DEV)
    torch.cuda.synchronize()
    d_sk, n_sk = ctx.scan_device(params, g_cat.data_ptr(), len(allb), d_o.data_ptr(), G)
    d_mn, d_lo, _, koff = ctx.sketch_keys_device(params, g_cat.data_ptr(), len(allb), d_o.data_ptr(), d_sk, n_sk, list(range(G + 1)))
    r_mn, r_lo = device_keys(ctx, d_mn, d_lo, int(koff[-1]))
    D = synth.direct_family_sketches(N - G, fam_size=20, seed=21, device=DEV)
    mn = torch.cat([D.minimizer, r_mn]).contiguous()
    lo = torch.cat([D.kmer_lo, r_lo]).contiguous()
    off = np.concatenate([D.sk_off.astype(np.uint64), koff[1:].astype(np.uint64) + D.sk_off[-1]])
    torch.cuda.synchronize()
    return mn, lo, off, g_cat, allo.astype(np.int64)


def make_text(g_cat, g_off, n_rec, length, seed):
    """FASTA text on the device: '>r\\n' + bases + '\\n' per record -> (text tensor, bytes, source genome per record or -1)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    src = torch.randint(0, G, (n_rec,), generator=gen, device=DEV)
    first, size = torch.from_numpy(g_off[:-1]).to(DEV)[src], torch.from_numpy(np.diff(g_off)).to(DEV)[src]
    start = first + (torch.rand(n_rec, generator=gen, device=DEV, dtype=torch.float64) * (size - length)).long()
    text = torch.empty((n_rec, length + 4), dtype=torch.uint8, device=DEV)
    text[:, 0], text[:, 1], text[:, 2], text[:, -1] = ord(">"), ord("r"), ord("\n"), ord("\n")
    step = max(1, (1 << 26) // length)                      # (the index matrix in slabs of 512 MB)
    for a in range(0, n_rec, step):
        z = min(a + step, n_rec)
        text[a:z, 3:-1] = g_cat[start[a:z, None] + torch.arange(length, device=DEV)[None, :]]
    strangers = torch.arange(n_rec, device=DEV) % 10 == 9
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=DEV)
    n_s = int(strangers.sum())
    text[strangers, 3:-1] = acgt[torch.randint(0, 4, (n_s, length), generator=gen, device=DEV)]
    flat = torch.cat([text.reshape(-1), torch.zeros(64, dtype=torch.uint8, device=DEV)])
    torch.cuda.synchronize()
    return flat, n_rec * (length + 4), torch.where(strangers, -1, src).cpu().numpy()


def road(ctx, side, params, text, n_text, n_rec):
    """ingest, scan, then keys + classify per batch -> (records, hits, stage milliseconds, keys)"""
    ms = {}
    (d_bases, n_bases, d_off, got), ms["ingest"] = wall(lambda: side.clean_fasta_device(text.data_ptr(), n_text))
    assert got == n_rec
    (d_sk, n_sk), ms["scan"] = wall(lambda: side.scan_device(params, d_bases, n_bases, d_off, n_rec))
    rec_of = side.to_host(d_sk, n_sk, sp.SUPERKMER_DTYPE)["rec"]               # (the batches' seams: the driver finds them with one launch)
    ms["keys"] = ms["classify"] = 0.0
    ctx.classify_stage_ms()
    recs, hits, keys = [], [], 0
    for r0 in range(0, n_rec, BATCH):
        r1 = min(r0 + BATCH, n_rec)
        q0, q1 = (int(x) for x in np.searchsorted(rec_of, [r0, r1]))
        (d_mn, d_lo, _, koff), t = wall(lambda: side.sketch_keys_device(params, d_bases, n_bases, d_off, d_sk + q0 * sp.SUPERKMER_DTYPE.itemsize, q1 - q0,
                                                                         np.arange(r0, r1 + 1, dtype=np.uint32)))
        ms["keys"] += t
        (r, h), t = wall(lambda: ctx.classify_device(d_mn, d_lo, None, koff, TOP))
        ms["classify"] += t
        recs.append(r); hits.append(h); keys += int(koff[-1])
    ms.update({"classify_" + f: v for f, v in ctx.classify_stage_ms().items()})
    return np.concatenate(recs), np.concatenate(hits), ms, keys, (d_bases, n_bases, d_off, d_sk, rec_of)


def yardsticks(ctx, side, params, index, scan, copy_GBps):
    """the first YARD records: their exact sum of holder counts, and the comparison + neighbours next to one classify call"""
    mn, lo, off = index
    d_bases, n_bases, d_off, d_sk, rec_of = scan
    q1 = int(np.searchsorted(rec_of, YARD))
    d_mn, d_lo, _, koff = side.sketch_keys_device(params, d_bases, n_bases, d_off, d_sk, q1, np.arange(YARD + 1, dtype=np.uint32))
    total = int(koff[-1])
    q_mn, q_lo = device_keys(side, d_mn, d_lo, total)
    (records, hits), one_call = wall(lambda: ctx.classify_device(q_mn.data_ptr(), q_lo.data_ptr(), None, koff, TOP))
    both_mn, both_lo = torch.cat([q_mn, mn]).contiguous(), torch.cat([q_lo, lo]).contiguous()
    both_off = np.concatenate([koff.astype(np.uint64), off[1:] + np.uint64(total)])
    n = YARD + N
    card = np.diff(both_off.astype(np.int64)).astype(np.uint64)
    scratch = torch.zeros((n, n), dtype=torch.int32, device=DEV)
    cells = torch.zeros(1 << 26, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    ptrs = (both_mn.data_ptr(), both_lo.data_ptr(), None)
    ctx.compare_forget()
    n_cells, _ = wall(lambda: ctx.compare_cells_device(K, *ptrs, both_off, n, scratch.data_ptr(), cells.data_ptr(), cells.numel(), n_query=YARD))
    n_cells, compare_ms = wall(lambda: ctx.compare_cells_device(K, *ptrs, both_off, n, scratch.data_ptr(), cells.data_ptr(), cells.numel(), n_query=YARD))
    (rows, passing, _), nb_ms = wall(lambda: ctx.neighbours_cells_device(cells.data_ptr(), n_cells, card, n, sp.NEIGHBOUR_CONTAINED, 0, 1, TOP, YARD))
    # the neighbours' order is by the fraction shared / keys of the row, the lower partner among equals: the classification's order
    best = {int(r["sketch"]): (int(r["neighbour"]) - YARD, int(r["shared"])) for r in rows}
    mine = {r: (int(hits[r, 0]["reference"]), int(hits[r, 0]["shared"])) for r in range(YARD) if records[r]["listed"]}
    assert best == mine, "the comparison's best partner is the classification's best match"
    rows_pv, _ = ctx.prevalence_device(K, *ptrs, both_off, n, 1, 2, n_query=YARD)   # (this replaces the index: the last call of the tool)
    holders = int(rows_pv["holders"].astype(np.int64).sum())
    return {"records": YARD, "keys": total, "sum_of_holders": holders, "classify_one_call_ms": one_call, "cells": int(n_cells),
            "comparison_cells_ms": compare_ms, "neighbours_top1_ms": nb_ms, "comparison_plus_neighbours_ms": compare_ms + nb_ms,
            "comparison_over_classify": (compare_ms + nb_ms) / one_call, "bound_ms": (total * 20 + holders * 2) / (copy_GBps * 1e9) * 1e3}


def case(ctx, side, params, index, g_cat, g_off, name, copy_GBps):
    shape = SETS[name]
    n_rec, length = shape["records"], shape["bases"]
    text, n_text, src = make_text(g_cat, g_off, n_rec, length, 31)
    ctx.classify_index_device(K, index[0].data_ptr(), index[1].data_ptr(), None, index[2], N)
    road(ctx, side, params, text, n_text, n_rec)                               # (allocations)
    records, hits, ms, keys, scan = road(ctx, side, params, text, n_text, n_rec)
    assert np.all(records["hit_keys"] <= records["keys"]) and np.all(records["listed"] == np.minimum(records["passing"], TOP))
    cut = (src >= 0) & (records["keys"] > 0)
    whole = hits[cut, 0]["shared"] == records["keys"][cut]
    assert whole.mean() > 0.999, whole.mean()
    total_ms = ms["ingest"] + ms["scan"] + ms["keys"] + ms["classify"]
    out = {"set": name, "records": n_rec, "bases_per_record": length, "bases": n_rec * length, "keys": keys, "keys_per_record": keys / n_rec,
           "classified": int((records["listed"] > 0).sum()), "batches": -(-n_rec // BATCH), "stage_ms": ms, "road_ms": total_ms,
           "records_per_s": n_rec / (total_ms * 1e-3), "bases_per_s": n_rec * length / (total_ms * 1e-3),
           "classify_records_per_s": n_rec / (ms["classify"] * 1e-3), "classify_bases_per_s": n_rec * length / (ms["classify"] * 1e-3)}
    try:
        y = yardsticks(ctx, side, params, index, scan, copy_GBps)
        scaled = y["sum_of_holders"] * keys / max(y["keys"], 1)
        out["yardsticks"] = y
        out["work_per_record"] = y["sum_of_holders"] / YARD
        out["byte_bound_ms"] = (keys * 20 + scaled * 2) / (copy_GBps * 1e9) * 1e3
        kernels = ms["classify_probe"] + ms["classify_route"] + ms["classify_wave_form"] + ms["classify_workgroup_form"]
        out["classify_kernels_ms"] = kernels
        out["kernels_over_bound"] = kernels / out["byte_bound_ms"]
        out["classify_calls_over_bound"] = ms["classify"] / out["byte_bound_ms"]
    except (sp.SpspError, AssertionError, RuntimeError) as e:
        out["yardsticks_error"] = "%s: %s" % (type(e).__name__, e)
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    ctx, side = sp.Context(0), sp.Context(0)
    params = sp.make_params(K, M, S)
    hbm = ctx.measure_hbm()
    mn, lo, off, g_cat, g_off = make_index(ctx, params)
    ctx.timing_enable(True)
    _, build_ms = wall(lambda: ctx.classify_index_device(K, mn.data_ptr(), lo.data_ptr(), None, off, N))
    _, build_ms = wall(lambda: ctx.classify_index_device(K, mn.data_ptr(), lo.data_ptr(), None, off, N))
    doc = {"tool": "classify_bench", "k": K, "m": M, "s": S, "top": TOP, "library": sp.library_info(), "device": torch.cuda.get_device_name(0),
           "hbm_copy_GBps": hbm["copy_GBps"], "plan": sp.classify_plan(N, TOP),
           "index": {"sketches": N, "from_genomes": G, "entries": int(off[-1]), "build_ms": build_ms}, "sets": []}
    for name in ("reads", "contigs"):
        if which in ("all", name):
            doc["sets"].append(case(ctx, side, params, (mn, lo, off), g_cat, g_off, name, hbm["copy_GBps"]))
    ctx.close(); side.close()
    print(json.dumps(doc))
