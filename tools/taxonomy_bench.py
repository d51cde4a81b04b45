#!/usr/bin/env python3
"""Cost of the taxonomy pass on one MI355X next to the classification it extends, on the same records in the same run.

The index and the two record sets are classify_bench.py's (its functions are used as they are): 10 000 sketches at k = 31, m = 11,
s = 4 -- 9 800 synthesised at the key level in families of 20, and 200 sketched from synthetic genomes of 100 kbp in 10 families --
and as FASTA text made on the device

  reads    10^6 records of 150 bases
  contigs  10^5 records of 5 000 bases

The tree: every family is a genus under three invented ranks (domain > phylum > class > genus > strain), the references at the
strains: 10 genera for the genomes' families, 490 for the synthesised ones; 10 588 nodes.

Per set: the text is ingested and scanned once; per batch of 65 535 records the keys are extracted once and handed to
spsp_taxonomy_device AND to the unchanged spsp_classify_device at top = 1 (the yardstick), each call timed on the host (it waits
for the device before it returns) and by the events between its launches (spsp_taxonomy_stage_ms, spsp_classify_stage_ms).  The
whole road runs twice and the first run (allocations) is dropped.  Reported: the attach time, the stage times of both, and

  byte bound   keys x (8 bytes of slot + 12 bytes of key) + hit keys x 4 bytes of node, over the copy rate
               spsp_measure_hbm_device reports in this run.

The expectation the tool confirms or refutes is that the taxonomy's tally stages (wave form + workgroup form) cost less than
classify's on the same records: both are printed, neither is asserted.  Asserted is the ANSWER: the first 2 000 records of each
set against a model on tuples of names (prefixes and sums over dicts; the holders of the records' keys are filtered from the index
with torch.isin, which is plumbing), and hit_keys equal to classify's on every record.

usage (GPU box): python tools/taxonomy_bench.py [reads|contigs|all]"""
import json
import os
import sys
from collections import Counter, defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classify_bench as cb  # noqa: E402
import supersampler_amd as sp  # noqa: E402

N, G, BATCH, CHECKED = cb.N, cb.G, cb.BATCH, 2000
NONE = sp.TAXONOMY_NONE


def lineages():
    """reference j < N - G: the synthesised family j // 20; the genomes behind: family (j - (N - G)) // 20 of 10"""
    out = []
    for j in range(N - G):
        f = j // 20
        out.append(("synthetic", "phylum%d" % (f // 70), "class%d" % (f // 7), "sgenus%d" % f, "strain%d" % j))
    for g in range(G):
        f = g // (G // 10)
        out.append(("genomes", "phylum%d" % (f // 5), "class%d" % (f // 2), "genus%d" % f, "strain%d" % g))
    return out


def lca(nodes):
    out = nodes[0]
    for t in nodes[1:]:
        n = 0
        while n < min(len(out), len(t)) and out[n] == t[n]:
            n += 1
        out = out[:n]
    return out


def model_rows(lines, index, q_mn, q_lo, koff, num_of):
    """the rule on tuples for the records whose keys are q_mn, q_lo (host arrays) -> rows of numbers as the device writes them"""
    mn, lo, off = index
    want = torch.from_numpy(np.unique(q_lo).view(np.int64)).to(cb.DEV)
    at = torch.nonzero(torch.isin(lo, want)).reshape(-1)                      # (plumbing: the index entries whose kmer_lo some record key has)
    e_mn, e_lo, e_at = mn[at].cpu().numpy().view(np.uint32), lo[at].cpu().numpy().view(np.uint64), at.cpu().numpy()
    ref = np.searchsorted(off.astype(np.int64), e_at, side="right") - 1
    held = defaultdict(list)
    for a, b, j in zip(e_mn.tolist(), e_lo.tolist(), ref.tolist()):
        held[(a, b)].append(lines[j])
    node_of = {x: lca(ts) for x, ts in held.items()}
    rows = []
    for r in range(len(koff) - 1):
        q = set(zip(q_mn[int(koff[r]):int(koff[r + 1])].tolist(), q_lo[int(koff[r]):int(koff[r + 1])].tolist()))
        w = Counter(node_of[x] for x in q if x in node_of)
        if not w:
            rows.append((len(q), 0, NONE, NONE, 0, 0, 0, 0))
            continue
        path = {t: sum(w.get(t[:i], 0) for i in range(len(t) + 1)) for t in w}
        best = max(path.values())
        W = [t for t in w if path[t] == best]
        start = lca(W)
        clade = sum(c for d, c in w.items() if d[:len(start)] == start)       # (min_keys = 1, num = 0: the start passes)
        rows.append((len(q), sum(w.values()), num_of[start], num_of[start], best, clade, w.get(start, 0), len(W)))
    return rows


def road(ctx, side, params, text, n_text, n_rec, keep_first):
    """ingest, scan, then per batch the keys once and both passes on them -> (taxonomy records, classify records, ms, keys, first batch's keys)"""
    ms = {}
    (d_bases, n_bases, d_off, got), ms["ingest"] = cb.wall(lambda: side.clean_fasta_device(text.data_ptr(), n_text))
    assert got == n_rec
    (d_sk, n_sk), ms["scan"] = cb.wall(lambda: side.scan_device(params, d_bases, n_bases, d_off, n_rec))
    rec_of = side.to_host(d_sk, n_sk, sp.SUPERKMER_DTYPE)["rec"]
    ms["keys"] = ms["taxonomy"] = ms["classify"] = 0.0
    ctx.taxonomy_stage_ms(); ctx.classify_stage_ms()
    tx, cf, keys, first = [], [], 0, None
    for r0 in range(0, n_rec, BATCH):
        r1 = min(r0 + BATCH, n_rec)
        q0, q1 = (int(x) for x in np.searchsorted(rec_of, [r0, r1]))
        (d_mn, d_lo, _, koff), t = cb.wall(lambda: side.sketch_keys_device(params, d_bases, n_bases, d_off, d_sk + q0 * sp.SUPERKMER_DTYPE.itemsize, q1 - q0,
                                                                            np.arange(r0, r1 + 1, dtype=np.uint32)))
        ms["keys"] += t
        a, t = cb.wall(lambda: ctx.taxonomy_device(d_mn, d_lo, None, koff))
        ms["taxonomy"] += t
        (b, _), t = cb.wall(lambda: ctx.classify_device(d_mn, d_lo, None, koff, 1))
        ms["classify"] += t
        if keep_first and r0 == 0:
            end = int(koff[CHECKED])
            first = (side.to_host(d_mn, end, np.uint32), side.to_host(d_lo, end, np.uint64), koff[:CHECKED + 1].copy())
        tx.append(a); cf.append(b); keys += int(koff[-1])
    ms.update({"taxonomy_" + f: v for f, v in ctx.taxonomy_stage_ms().items()})
    ms.update({"classify_" + f: v for f, v in ctx.classify_stage_ms().items()})
    return np.concatenate(tx), np.concatenate(cf), ms, keys, first


def case(ctx, side, params, index, lines, num_of, g_cat, g_off, name, copy_GBps):
    shape = cb.SETS[name]
    n_rec, length = shape["records"], shape["bases"]
    text, n_text, src = cb.make_text(g_cat, g_off, n_rec, length, 31)
    road(ctx, side, params, text, n_text, n_rec, False)                       # (allocations)
    tx, cf, ms, keys, first = road(ctx, side, params, text, n_text, n_rec, True)
    assert np.array_equal(tx["keys"], cf["keys"]) and np.array_equal(tx["hit_keys"], cf["hit_keys"]), "the probe pass is classify's"
    want = model_rows(lines, index, *first, num_of)
    got = [tuple(int(rec[f]) for f in sp.TAXONOMY_RECORD_DTYPE.names[1:]) for rec in tx[:CHECKED]]
    assert got == want, [(r, a, b) for r, (a, b) in enumerate(zip(got, want)) if a != b][:3]
    hits = int(tx["hit_keys"].astype(np.int64).sum())
    tally = lambda p: ms[p + "_wave_form"] + ms[p + "_workgroup_form"]
    kernels = lambda p: sum(ms[p + "_" + f] for f in ("probe", "route", "wave_form", "workgroup_form"))
    bound = (keys * 20 + hits * 4) / (copy_GBps * 1e9) * 1e3
    called = tx["node"] != NONE
    return {"set": name, "records": n_rec, "bases_per_record": length, "keys": keys, "hit_keys": hits, "keys_per_record": keys / n_rec,
            "hit_keys_per_record": hits / n_rec, "classified": int(called.sum()), "at_the_root": int((tx["node"] == 0).sum()),
            "several_winners": int((tx["winners"] > 1).sum()), "checked_against_the_model": CHECKED, "batches": -(-n_rec // BATCH), "stage_ms": ms,
            "byte_bound_ms": bound, "taxonomy_kernels_ms": kernels("taxonomy"), "classify_kernels_ms": kernels("classify"),
            "taxonomy_tally_ms": tally("taxonomy"), "classify_tally_ms": tally("classify"), "tally_taxonomy_over_classify": tally("taxonomy") / tally("classify"),
            "taxonomy_kernels_over_bound": kernels("taxonomy") / bound, "taxonomy_records_per_s": n_rec / (ms["taxonomy"] * 1e-3),
            "classify_records_per_s": n_rec / (ms["classify"] * 1e-3)}


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    ctx, side = sp.Context(0), sp.Context(0)
    params = sp.make_params(cb.K, cb.M, cb.S)
    hbm = ctx.measure_hbm()
    mn, lo, off, g_cat, g_off = cb.make_index(ctx, params)
    lines = lineages()
    tree = sp.taxonomy_lineages("".join(";".join(x) + "\n" for x in lines), N)
    paths = [()]
    for t in range(1, len(tree["parent"])):
        paths.append(paths[int(tree["parent"][t])] + (tree["names"][t],))
    num_of = {p: t for t, p in enumerate(paths)}
    ctx.timing_enable(True)
    _, build_ms = cb.wall(lambda: ctx.classify_index_device(cb.K, mn.data_ptr(), lo.data_ptr(), None, off, N))
    _, attach_ms = cb.wall(lambda: ctx.taxonomy_index_device(tree["parent"], tree["ref_node"]))
    _, attach_ms = cb.wall(lambda: ctx.taxonomy_index_device(tree["parent"], tree["ref_node"]))
    doc = {"tool": "taxonomy_bench", "k": cb.K, "m": cb.M, "s": cb.S, "library": sp.library_info(), "device": torch.cuda.get_device_name(0),
           "hbm_copy_GBps": hbm["copy_GBps"], "plan": sp.taxonomy_plan(len(paths)),
           "index": {"sketches": N, "from_genomes": G, "entries": int(off[-1]), "build_ms": build_ms, "nodes": len(paths), "attach_ms": attach_ms}, "sets": []}
    for name in ("reads", "contigs"):
        if which in ("all", name):
            doc["sets"].append(case(ctx, side, params, (mn, lo, off), lines, num_of, g_cat, g_off, name, hbm["copy_GBps"]))
    ctx.close(); side.close()
    print(json.dumps(doc))
