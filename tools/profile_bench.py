#!/usr/bin/env python3
"""Cost of the profile pass on one MI355X, stage by stage, next to the depth read of the same counters and the adds that fed them.

Two indexes of 10 000 sketches at k = 31, m = 11, s = 4, and 10^6 reads of 150 bases, nine in ten cut from 200 of the references:
  families  classify_bench.py's index (imported from it): 9 800 synthetic sketches in families of 20 and 200 sketched from genomes in
            10 families; the reads are cut from the 200.
  species   ONE species: 10 000 genomes of 25 000 bases, every one a 1 - 5 % mutation of one ancestor, sketched on the device; the
            reads are cut from the first 200.  The walk's bad case: the first winner's ~6 000 keys are each held by thousands of
            references, so round 1 takes one off the same 10 000 counters tens of millions of times.

Per shape the file driver's road with the public calls on two contexts, as depth_bench.py: ingest, ONE scan, per batch of 65 535
records the key extraction and spsp_depth_add_device.  The road is run twice and the first run (allocations) dropped.  Then, on the
same counters and in the same process, three spsp_depth_read_device and three spsp_profile_device per (min_count, min_keys); with
timing on, spsp_depth_stage_ms and spsp_profile_stage_ms give the event milliseconds, spsp_profile_counts the rounds queued, the
rows and the host waits.

Asserted: the facts of the rule on the rows (include/spsp.h), found_keys equals the read's index_found, assigned_keys + the last
remaining equals found_keys.

usage (GPU box): python tools/profile_bench.py [families|species|all]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import classify_bench as cb  # noqa: E402
import supersampler_amd as sp  # noqa: E402
from supersampler_amd import synth  # noqa: E402

K, M, S, N, BATCH, DEV = cb.K, cb.M, cb.S, cb.N, cb.BATCH, cb.DEV
RECORDS, BASES = cb.SETS["reads"]["records"], cb.SETS["reads"]["bases"]
SPECIES_GENOME = 25_000
ASKS = ((1, 1), (2, 5))                                                            # (min_count, min_keys)
REPEAT = 3


def species_index(ctx, params):
    """N genomes of one family, sketched in slabs of 1 000 genomes -> (mn, lo, off, the first cb.G genomes' bases, their offsets)"""
    genomes = synth.family_genomes(5, N, SPECIES_GENOME, 1, [0.01, 0.02, 0.03, 0.05])
    mns, los, offs, base = [], [], [np.zeros(1, np.uint64)], 0
    for a in range(0, N, 1000):
        part = genomes[a:a + 1000]
        allb, allo = synth.concat_records(part)
        d_b = torch.from_numpy(np.concatenate([allb, np.zeros(64, np.uint8)])).to(DEV)
        d_o = torch.from_numpy(allo.view(np.int64)).to(DEV)
        torch.cuda.synchronize()
        d_sk, n_sk = ctx.scan_device(params, d_b.data_ptr(), len(allb), d_o.data_ptr(), len(part))
        d_mn, d_lo, _, koff = ctx.sketch_keys_device(params, d_b.data_ptr(), len(allb), d_o.data_ptr(), d_sk, n_sk, list(range(len(part) + 1)))
        mn, lo = cb.device_keys(ctx, d_mn, d_lo, int(koff[-1]))
        mns.append(mn); los.append(lo); offs.append(koff[1:].astype(np.uint64) + np.uint64(base))
        base += int(koff[-1])
    allb, allo = synth.concat_records(genomes[:cb.G])
    g_cat = torch.from_numpy(np.concatenate([allb, np.zeros(64, np.uint8)])).to(DEV)
    torch.cuda.synchronize()
    return torch.cat(mns).contiguous(), torch.cat(los).contiguous(), np.concatenate(offs), g_cat, allo.astype(np.int64)


def road(ctx, side, params, text, n_text, n_rec):
    """begin, and every batch's keys added -> (record keys, wall milliseconds of the add calls)"""
    d_bases, n_bases, d_off, got = side.clean_fasta_device(text.data_ptr(), n_text)
    assert got == n_rec
    d_sk, n_sk = side.scan_device(params, d_bases, n_bases, d_off, n_rec)
    rec_of = side.to_host(d_sk, n_sk, sp.SUPERKMER_DTYPE)["rec"]
    ctx.depth_begin()
    keys, wall = 0, 0.0
    for r0 in range(0, n_rec, BATCH):
        r1 = min(r0 + BATCH, n_rec)
        q0, q1 = (int(x) for x in np.searchsorted(rec_of, [r0, r1]))
        d_mn, d_lo, _, koff = side.sketch_keys_device(params, d_bases, n_bases, d_off, d_sk + q0 * sp.SUPERKMER_DTYPE.itemsize, q1 - q0,
                                                       np.arange(r0, r1 + 1, dtype=np.uint32))
        _, t = cb.wall(lambda: ctx.depth_add(d_mn, d_lo, None, int(koff[0]), int(koff[-1]) - int(koff[0])))
        wall += t
        keys += int(koff[-1]) - int(koff[0])
    return keys, wall


def check_rows(rows, totals, index_found, min_keys):
    left, last = int(totals["found_keys"]), None
    assert left == index_found
    for r in rows:
        a = int(r["assigned"])
        assert 1 <= a <= int(r["found"]) <= int(r["keys"]) and (last is None or a <= last) and int(r["remaining"]) == left - a
        assert a <= int(r["sum"]) <= a * int(r["max"]) and 1 <= int(r["median"]) <= int(r["max"])
        left, last = int(r["remaining"]), a
    assert len(set(rows["reference"].tolist())) == len(rows) and int(totals["assigned_keys"]) + left == int(totals["found_keys"])
    assert min_keys > 1 or left == 0


def case(ctx, side, params, name, index, g_cat, g_off):
    mn, lo, off = index
    n_ref = len(off) - 1
    text, n_text, src = cb.make_text(g_cat, g_off, RECORDS, BASES, 31)
    ctx.classify_index_device(K, mn.data_ptr(), lo.data_ptr(), None, off, n_ref)
    road(ctx, side, params, text, n_text, RECORDS)                                # (allocations)
    ctx.depth_read(1); ctx.profile_read(1, 1)
    ctx.depth_stage_ms(); ctx.profile_stage_ms()
    keys, add_wall = road(ctx, side, params, text, n_text, RECORDS)
    add_ms = ctx.depth_stage_ms()["add"]
    out = {"shape": name, "references": n_ref, "index_entries": int(off[-1] - off[0]), "records": RECORDS, "bases_per_record": BASES, "record_keys": keys,
           "source_references": int(len(set(src[src >= 0].tolist()))), "add_ms": add_ms, "add_calls_wall_ms": add_wall, "asks": []}
    for min_count, min_keys in ASKS:
        read_wall = prof_wall = 0.0
        for _ in range(REPEAT):
            (d_rows, d_totals), t = cb.wall(lambda: ctx.depth_read(min_count))
            read_wall += t
        read = ctx.depth_stage_ms()
        for _ in range(REPEAT):
            (rows, totals), t = cb.wall(lambda: ctx.profile_read(min_count, min_keys))
            prof_wall += t
        ms = ctx.profile_stage_ms()
        ctx.profile_read(min_count, min_keys, 1)                                   # the first round alone: its walk is the one with the most decrements
        first = ctx.profile_stage_ms()
        ctx.timing_enable(False)                                                   # the calls as a user makes them: no events between the launches
        plain_read = plain_prof = 0.0
        for _ in range(REPEAT):
            plain_read += cb.wall(lambda: ctx.depth_read(min_count))[1]
            plain_prof += cb.wall(lambda: ctx.profile_read(min_count, min_keys))[1]
        ctx.timing_enable(True)
        check_rows(rows, totals, int(d_totals["index_found"]), min_keys)
        stage = {f: ms[f] / REPEAT for f in ("start", "picks", "walks", "reduction")}
        call = sum(stage.values())
        read_ms = (read["entry"] + read["reduce"]) / REPEAT
        from_sources = int(np.isin(rows["reference"], np.unique(src[src >= 0]) + (n_ref - cb.G if name == "families" else 0)).sum())
        out["asks"].append({"min_count": min_count, "min_keys": min_keys, "stage_ms": stage, "kernels_ms": call, "call_wall_ms": prof_wall / REPEAT,
                            "rounds_queued": ms["rounds"], "rows": ms["rows"], "host_waits": ms["waits"], "rows_from_source_references": from_sources,
                            "index_found": int(d_totals["index_found"]), "assigned_keys": int(totals["assigned_keys"]),
                            "first_rows": [{f: int(r[f]) for f in ("reference", "keys", "found", "assigned", "median", "max")} for r in rows[:3]],
                            "read_ms": {"entry": read["entry"] / REPEAT, "reduce": read["reduce"] / REPEAT}, "read_wall_ms": read_wall / REPEAT,
                            "kernels_over_read": call / read_ms, "kernels_over_adds": call / add_ms, "wall_over_read_wall": prof_wall / read_wall,
                            "stage_share": {f: stage[f] / call for f in stage},
                            "first_round_ms": {f: first[f] for f in ("start", "picks", "walks", "reduction")},
                            "untimed_call_wall_ms": plain_prof / REPEAT, "untimed_read_wall_ms": plain_read / REPEAT,
                            "untimed_wall_over_read": plain_prof / plain_read, "untimed_wall_over_adds": plain_prof / REPEAT / add_ms})
    return out


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    ctx, side = sp.Context(0), sp.Context(0)
    params = sp.make_params(K, M, S)
    ctx.timing_enable(True)
    doc = {"tool": "profile_bench", "k": K, "m": M, "s": S, "library": sp.library_info(), "device": torch.cuda.get_device_name(0),
           "forms": {"walk_atomics": "LDS counters per workgroup up to 38 912 references, flushed once; plain no-return atomicSub per holder beyond",
                     "entries_per_wave": 16, "start_tile": 2048}, "shapes": []}
    if which in ("all", "families"):
        mn, lo, off, g_cat, g_off = cb.make_index(ctx, params)
        doc["shapes"].append(case(ctx, side, params, "families", (mn, lo, off), g_cat, g_off))
        del mn, lo, g_cat
    if which in ("all", "species"):
        mn, lo, off, g_cat, g_off = species_index(ctx, params)
        doc["shapes"].append(case(ctx, side, params, "species", (mn, lo, off), g_cat, g_off))
    ctx.close(); side.close()
    print(json.dumps(doc))
