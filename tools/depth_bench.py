#!/usr/bin/env python3
"""Cost of the depth pass on one MI355X, launch by launch, next to classify's probe pass on the same records.

The index and the two record sets are classify_bench.py's (imported from it): 10 000 sketches, 200 of them sketched from synthetic
genomes at k = 31, m = 11, s = 4; `reads` 10^6 records of 150 bases, `contigs` 10^5 records of 5 000 bases, nine in ten cut from the
200 genomes.  A third shape, `long`, is the reads against the same index with ONE more reference of 4 x 10^6 keys of its own (no read
holds them): what a reference far longer than the rest costs the read (it is reduced by segments, a workgroup each, and a merge).

Per set the file driver's road with the public calls on two contexts: ingest, ONE scan, and per batch of 65 535 records the key
extraction, then spsp_classify_device (the yardstick: k_cf_probe does the same probe without the counter) and spsp_depth_add_device
on the same keys; one spsp_depth_read_device at the end.  The road is run twice and the first run (allocations) dropped.  With
timing on, spsp_depth_stage_ms gives the milliseconds of k_dp_add (all batches), k_dp_entry and k_dp_reduce, and
spsp_classify_stage_ms those of k_cf_probe in the same process.

Byte bounds at the copy rate spsp_measure_hbm_device reports in this run:
  add     (20 bytes of key + 8 of slot) per record key + 4 per hit
  entry   12 bytes per index entry
  reduce  4 bytes per index entry and pass (the kernel streams 5: the count and the unique flag)

Asserted: hit_keys equals the sum of classify's hit keys, sum over the rows >= hit_keys, found <= keys.

usage (GPU box): python tools/depth_bench.py [reads|contigs|long|all]"""
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

K, M, S, N, BATCH, DEV = cb.K, cb.M, cb.S, cb.N, cb.BATCH, cb.DEV
LONG_KEYS = 4_000_000
SETS = {"reads": ("reads", False), "contigs": ("contigs", False), "long": ("reads", True)}


def with_long_reference(mn, lo, off):
    """one more reference behind the index: LONG_KEYS keys, minimizers and words both ascending (so sorted and distinct)"""
    gen = torch.Generator(device=DEV).manual_seed(77)
    l_mn = torch.sort(torch.randint(0, 1 << 22, (LONG_KEYS,), generator=gen, device=DEV, dtype=torch.int32)).values
    l_lo = torch.cumsum(torch.randint(1, 1 << 20, (LONG_KEYS,), generator=gen, device=DEV, dtype=torch.int64), 0) | (1 << 61)
    out = torch.cat([mn, l_mn]).contiguous(), torch.cat([lo, l_lo]).contiguous(), np.concatenate([off, [off[-1] + np.uint64(LONG_KEYS)]]).astype(np.uint64)
    torch.cuda.synchronize()
    return out


def wave_duplicates(side, d_mn, d_lo, total):
    """the share of a batch's record keys that equal an earlier key of their own wave (64 consecutive entries): the adds that
    k_dp_add would save if it combined equal keys inside a wave"""
    mn, lo = cb.device_keys(side, d_mn, d_lo, total)
    n = total // 64 * 64
    word = (lo[:n] ^ (mn[:n].long() << 40)).reshape(-1, 64)                     # (one word per key: equal keys, equal words)
    word = torch.sort(word, dim=1).values
    return float((word[:, 1:] == word[:, :-1]).sum().item()) / max(n, 1)


def road(ctx, side, params, text, n_text, n_rec):
    ms = {}
    (d_bases, n_bases, d_off, got), ms["ingest"] = cb.wall(lambda: side.clean_fasta_device(text.data_ptr(), n_text))
    assert got == n_rec
    (d_sk, n_sk), ms["scan"] = cb.wall(lambda: side.scan_device(params, d_bases, n_bases, d_off, n_rec))
    rec_of = side.to_host(d_sk, n_sk, sp.SUPERKMER_DTYPE)["rec"]
    ms["keys"] = ms["classify_call"] = ms["add_call"] = 0.0
    ctx.classify_stage_ms(); ctx.depth_stage_ms()
    ctx.depth_begin()
    keys = hit = 0
    for r0 in range(0, n_rec, BATCH):
        r1 = min(r0 + BATCH, n_rec)
        q0, q1 = (int(x) for x in np.searchsorted(rec_of, [r0, r1]))
        (d_mn, d_lo, _, koff), t = cb.wall(lambda: side.sketch_keys_device(params, d_bases, n_bases, d_off, d_sk + q0 * sp.SUPERKMER_DTYPE.itemsize, q1 - q0,
                                                                            np.arange(r0, r1 + 1, dtype=np.uint32)))
        ms["keys"] += t
        (r, _), t = cb.wall(lambda: ctx.classify_device(d_mn, d_lo, None, koff, 1))
        ms["classify_call"] += t
        _, t = cb.wall(lambda: ctx.depth_add(d_mn, d_lo, None, int(koff[0]), int(koff[-1]) - int(koff[0])))
        ms["add_call"] += t
        keys += int(koff[-1]) - int(koff[0]); hit += int(r["hit_keys"].astype(np.int64).sum())
        if r0 == 0:                                                             # what combining equal keys inside a wave could save, on the first batch
            ms["wave_duplicate_share"] = wave_duplicates(side, d_mn, d_lo, int(koff[-1]))
    (rows, totals), ms["read_call"] = cb.wall(lambda: ctx.depth_read(1))
    ms["probe"] = ctx.classify_stage_ms()["probe"]
    ms.update(ctx.depth_stage_ms())
    return rows, totals, ms, keys, hit


def case(ctx, side, params, index, g_cat, g_off, name, copy_GBps):
    shape_name, long_ref = SETS[name]
    shape = cb.SETS[shape_name]
    n_rec, length = shape["records"], shape["bases"]
    mn, lo, off = with_long_reference(*index) if long_ref else index
    n_ref = len(off) - 1
    text, n_text, _ = cb.make_text(g_cat, g_off, n_rec, length, 31)
    ctx.classify_index_device(K, mn.data_ptr(), lo.data_ptr(), None, off, n_ref)
    road(ctx, side, params, text, n_text, n_rec)                               # (allocations)
    rows, totals, ms, keys, hit = road(ctx, side, params, text, n_text, n_rec)
    entries = int(off[-1] - off[0])
    assert int(totals["record_keys"]) == keys and int(totals["hit_keys"]) == hit, (totals, keys, hit)
    assert int(rows["sum"].astype(np.uint64).sum()) >= hit and np.all(rows["found"] <= rows["keys"])
    rate = copy_GBps * 1e9 * 1e-3                                               # bytes per millisecond
    bound = {"add": (keys * 28 + hit * 4) / rate, "entry": entries * 12 / rate, "reduce": entries * 4 / rate}
    ms_again = {}
    for mc in (1, 2):                                                           # the read alone, three times each: the counters stay
        for _ in range(3):
            ctx.depth_read(mc)
        got = ctx.depth_stage_ms()
        ms_again["min_count_%d" % mc] = {"entry": got["entry"] / 3, "reduce": got["reduce"] / 3}
    return {"set": name, "records": n_rec, "bases_per_record": length, "references": n_ref, "index_entries": entries, "index_keys": int(totals["index_keys"]),
            "index_found": int(totals["index_found"]), "record_keys": keys, "hit_keys": hit, "longest_reference": int(rows["keys"].max()),
            "largest_count": int(rows["max"].max()), "stage_ms": ms, "read_alone_ms": ms_again, "bound_ms": bound,
            "add_over_probe": ms["add"] / ms["probe"], "over_bound": {f: ms[f] / bound[f] for f in bound},
            "kernels_ms": ms["add"] + ms["entry"] + ms["reduce"], "reduce_share_of_read": ms["reduce"] / (ms["entry"] + ms["reduce"]),
            "add_share_of_kernels": ms["add"] / (ms["add"] + ms["entry"] + ms["reduce"]), "wave_duplicate_share": ms.pop("wave_duplicate_share")}


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    ctx, side = sp.Context(0), sp.Context(0)
    params = sp.make_params(K, M, S)
    hbm = ctx.measure_hbm()
    mn, lo, off, g_cat, g_off = cb.make_index(ctx, params)
    ctx.timing_enable(True)
    doc = {"tool": "depth_bench", "k": K, "m": M, "s": S, "library": sp.library_info(), "device": torch.cuda.get_device_name(0),
           "hbm_copy_GBps": hbm["copy_GBps"], "bins": sp.depth_plan(), "forms": {"wave_combined_adds": False, "segmented_long_references": True}, "sets": []}
    for name in ("reads", "contigs", "long"):
        if which in ("all", name):
            doc["sets"].append(case(ctx, side, params, (mn, lo, off), g_cat, g_off, name, hbm["copy_GBps"]))
    ctx.close(); side.close()
    print(json.dumps(doc))
