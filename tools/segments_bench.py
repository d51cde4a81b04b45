#!/usr/bin/env python3
"""Cost of writing segments as FASTA on one MI355X: the writer's one launch in both forms the ingest writes, next to the device's
streaming copy rate and to the windows' copy of the same bases, and the whole classify road over windows with and without the text.

The three record sets of tools/windows_bench.py, made on the host from a seed, cleaned and uploaded once:

  reads        10^6 records of 150 bases
  contigs      10^5 records of 5 000 bases
  chromosome   one record of 100 Mbp

Per set every record is one segment (its header "><name>:1-<L> <call>"): the text holds every base once, 81 bytes per 80 bases and
a header per record.  spsp_segments_write_device timed by the events around its launch (spsp_segments_stage_ms): one call that is
dropped, then REPS calls; printed are the median and the spread, and the writer's rate -- the source bytes it reads (ASCII: a byte
per base; packed: a quarter) and the text bytes it writes over its time.  The yardsticks of the same run:
spsp_measure_hbm_device's copy rate, and the windows' copy (k_wn_copy_ascii / k_wn_copy_packed, the "copy" stage of
spsp_windows_stage_ms) at a width no record exceeds, which moves the same bases once.  The ratios are written down, not gated.

The road: spsp_classify_files over the contigs against 16 references at W = 1 000, without the text and with segments="all".

Asserted is the ANSWER: every byte of every text equals the host function's.  No time is asserted.

usage (GPU box): python tools/segments_bench.py [reads|contigs|chromosome|road|all]   (one JSON line per measurement on stdout)"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import supersampler_amd as sp  # noqa: E402

REPS = 5
K = 31
SETS = {"reads": (1000000, 150), "contigs": (100000, 5000), "chromosome": (1, 100000000)}
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def spread(xs):
    a = np.array(xs)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def pack(bases):
    code = np.zeros(256, dtype=np.uint32)
    code[np.frombuffer(b"ACTG", dtype=np.uint8)] = np.arange(4, dtype=np.uint32)   # the ingest's codes
    c = code[bases]
    c = np.concatenate([c, np.zeros(-len(c) % 16, dtype=np.uint32)]).reshape(-1, 16)
    return (c << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def run(name, hbm):
    n_rec, length = SETS[name]
    rng = np.random.default_rng(7)
    bases = ACGT[rng.integers(0, 4, n_rec * length, dtype=np.uint8)]
    off = (np.arange(n_rec + 1, dtype=np.uint64) * np.uint64(length))
    ctx = sp.Context(0)
    d_off = torch.from_numpy(off.view(np.int64).copy()).cuda()
    forms = {False: torch.from_numpy(np.concatenate([bases, np.zeros(256, np.uint8)])).cuda(),
             True: torch.from_numpy(np.concatenate([pack(bases).view(np.uint8), np.zeros(256, np.uint8)])).cuda()}
    torch.cuda.synchronize()
    segs = np.zeros(n_rec, dtype=sp.SEGMENT_ROW_DTYPE)
    segs["record"], segs["end"], segs["windows"] = np.arange(n_rec), length, 1
    names = ["r%d" % r for r in range(n_rec)]
    want = np.frombuffer(sp.segments_fasta(bases, off, segs, names, ["reference"], "unmatched"), np.uint8)
    headers = [b">r%d:1-%d reference\n" % (r, length) for r in range(n_rec)]
    hdr_off = np.concatenate([[0], np.cumsum([len(h) for h in headers])]).astype(np.uint64)
    blob = b"".join(headers)
    src, lens = off[:-1].copy(), np.full(n_rec, length, dtype=np.uint64)
    ctx.timing_enable(True)
    for packed in (False, True):
        wn = []
        for rep in range(REPS + 1):                         # the windows' copy of the same bases: one window per record
            ctx.windows_stage_ms()
            ctx.records_windows_device(forms[packed].data_ptr(), len(bases), d_off.data_ptr(), n_rec, K, max(length, K), packed)
            if rep:
                wn.append(ctx.windows_stage_ms()["copy"])
        ms = []
        for rep in range(REPS + 1):
            ctx.segments_stage_ms()
            out, n_out = ctx.segments_write_device(forms[packed].data_ptr(), len(bases), src, lens, blob, hdr_off, packed)
            if rep:
                ms.append(ctx.segments_stage_ms()["write"])
        assert n_out == len(want) and (ctx.to_host(out, n_out, np.uint8) == want).all(), (name, packed)
        line = {"tool": "segments_bench", "set": name, "records": n_rec, "bases": len(bases), "form": "packed" if packed else "ascii", "segments": n_rec,
                "text_bytes": int(n_out), "reps": REPS, "write_ms": spread(ms), "windows_copy_ms": spread(wn)}
        read = len(bases) / (4 if packed else 1)
        line["write_bytes_moved"] = read + n_out
        line["write_GBps"] = (read + n_out) / line["write_ms"]["median"] / 1e6
        line["windows_copy_GBps"] = 2 * read / line["windows_copy_ms"]["median"] / 1e6
        line["hbm_copy_GBps"] = hbm["copy_GBps"]
        line["write_over_hbm_copy"] = line["write_GBps"] / hbm["copy_GBps"]
        line["write_per_byte_over_windows_copy_per_byte"] = line["windows_copy_GBps"] / line["write_GBps"]
        print(json.dumps(line), flush=True)
    ctx.timing_enable(False)
    ctx.close()


def road():
    rng = np.random.default_rng(11)
    ctx = sp.Context(0)
    genomes = [ACGT[rng.integers(0, 4, 200000, dtype=np.uint8)].tobytes() for _ in range(16)]
    n_rec, length = SETS["contigs"]
    with tempfile.TemporaryDirectory() as root:
        paths = []
        for i, g in enumerate(genomes):
            paths.append(os.path.join(root, "ref%02d.sk.gz" % i))
            sp.write_gz(paths[-1], ctx.sketch_text(b">g%d\n" % i + g + b"\n", K, 11, 100.0)[0], 1)
        parts = []
        for r in range(n_rec):                              # a contig: two stretches of two references, half each
            a, b = genomes[r % 16], genomes[(r * 7 + 3) % 16]
            at = int(rng.integers(0, 200000 - length))
            parts.append(b">c%d\n" % r + a[at:at + length // 2] + b[at:at + length - length // 2] + b"\n")
        with open(os.path.join(root, "contigs.fa"), "wb") as f:
            f.write(b"".join(parts))
        for kw in ({}, {"segments": "all", "gz": False}, {"segments": "all"}, {"smooth": 1, "segments": "called", "gz": False}):
            times = []
            for rep in range(3):
                t = time.perf_counter()
                ctx.classify_files(paths, os.path.join(root, "contigs.fa"), os.path.join(root, "out"), window=1000, **kw)
                times.append(time.perf_counter() - t)
            lw = ctx.last_windows
            print(json.dumps({"tool": "segments_bench", "set": "road: classify_files over the contigs, 16 references, W = 1000", "records": n_rec, "asked": kw,
                              "segments": len(lw["segments"]), "changed": lw["changed"], "written": lw["written"], "text_bytes": lw["bytes_out"],
                              "seconds": spread(times[1:])}), flush=True)
    ctx.close()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    c = sp.Context(0)
    hbm = c.measure_hbm()
    c.close()
    print(json.dumps({"tool": "segments_bench", "yardstick": "spsp_measure_hbm_device", **hbm}), flush=True)
    for name in SETS:
        if which in (name, "all"):
            run(name, hbm)
    if which in ("road", "all"):
        road()
