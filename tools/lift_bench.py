#!/usr/bin/env python3
"""Cost of lifting segments to raw coordinates on one MI355X: the lift's three stages next to the device's streaming copy rate and
to the ingest of the same text in the same process, and the whole classify road over windows with and without raw coordinates.

The three record sets of tools/segments_bench.py, written as FASTA on the host from a seed, 1 % of the bases replaced by runs of N
(reads: one line of 150; contigs and the chromosome: lines of 100), uploaded once:

  reads        10^6 records of 150
  contigs      10^5 records of 5 000
  chromosome   one record of 100 M

The queries are two per segment at W = 1 000 with every window a segment of its own (the most a run can ask): the first and the
last kept base of every window's owned stretch.  spsp_records_lift_device timed by the events between its launches
(spsp_lift_stage_ms): one call that is dropped, then REPS calls; printed are the medians and the spread, the wall clock of the call,
and the rate -- the text bytes the count pass reads plus the bytes of the tiles that answer, over the three stages' time.  The
yardsticks of the same run: spsp_measure_hbm_device's copy rate, and the wall clock of spsp_fasta_clean_device over the same text
(tools/ingest_bench.py's measure: three launches and two waits, reading the same bytes twice with the same classification).
The ratios are written down, not gated.

The road: spsp_classify_files over the contigs against 16 references at W = 1 000, without and with raw=True.

Asserted is the ANSWER: every raw position, record and length equals the host function's.  No time is asserted.

usage (GPU box): python tools/lift_bench.py [reads|contigs|chromosome|road|all]   (one JSON line per measurement on stdout)"""
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
K, W = 31, 1000
TILE = 4096
SETS = {"reads": (1000000, 150, 10), "contigs": (100000, 5000, 50), "chromosome": (1, 100000000, 1000)}   # records, length, N run
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def spread(xs):
    a = np.array(xs)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def make_text(n_rec, length, n_run, seed):
    """-> (text uint8, kept bases per record): '>r<7 digits>\\n', then the sequence in lines of 100 (a read: one line)"""
    rng = np.random.default_rng(seed)
    seq = ACGT[rng.integers(0, 4, n_rec * length, dtype=np.uint8)]
    n_runs = n_rec * length // (100 * n_run)                # 1 % of the bases
    starts = rng.integers(0, n_rec * length - n_run, n_runs)
    for j in range(n_run):
        seq[starts + j] = ord("N")
    kept = (seq.reshape(n_rec, length) != ord("N")).sum(axis=1).astype(np.uint64)
    line = length if length < 200 else 100
    body = np.full((n_rec, length // line, line + 1), 10, dtype=np.uint8)
    body[:, :, :line] = seq.reshape(n_rec, length // line, line)
    head = np.zeros((n_rec, 10), dtype=np.uint8)
    head[:, 0], head[:, 1], head[:, 9] = ord(">"), ord("r"), 10
    r = np.arange(n_rec)
    for d in range(7):
        head[:, 8 - d] = ord("0") + (r // 10 ** d) % 10
    return np.concatenate([head, body.reshape(n_rec, -1)], axis=1).reshape(-1), kept


def window_ends(kept):
    """the first and the last kept base of every window's owned stretch, as global kept-base indices, ascending"""
    S = W - (K - 1)
    off = np.concatenate([[0], np.cumsum(kept)]).astype(np.uint64)
    n_win = np.maximum(1, -(-(kept.astype(np.int64) - K + 1) // S))
    rec = np.repeat(np.arange(len(kept)), n_win)
    i = np.arange(int(n_win.sum())) - np.repeat(np.cumsum(n_win) - n_win, n_win)
    begin = i * S
    end = np.where(i + 1 < n_win[rec], (i + 1) * S, kept[rec].astype(np.int64))
    has = end > begin
    base = np.stack([off[rec][has] + begin[has].astype(np.uint64), off[rec][has] + (end[has] - 1).astype(np.uint64)], axis=1).reshape(-1)
    return base.astype(np.uint64)


def run(name, hbm):
    n_rec, length, n_run = SETS[name]
    text, kept = make_text(n_rec, length, n_run, 7)
    base = window_ends(kept)
    want = sp.records_lift(text.tobytes(), base)
    d = torch.from_numpy(np.concatenate([text, np.zeros(64, np.uint8)])).cuda()
    torch.cuda.synchronize()
    ctx = sp.Context(0)
    ingest = []
    for rep in range(REPS + 1):                             # the ingest of the same text, as tools/ingest_bench.py measures it
        t = time.perf_counter()
        _, n_bases, _, n_ingest = ctx.clean_fasta_device(d.data_ptr(), len(text))
        if rep:
            ingest.append((time.perf_counter() - t) * 1e3)
    assert n_bases == int(kept.sum()) and n_ingest == n_rec
    ctx.timing_enable(True)
    stages, wall = [], []
    for rep in range(REPS + 1):
        ctx.lift_stage_ms()
        t = time.perf_counter()
        got = ctx.records_lift_device(d.data_ptr(), len(text), n_bases, base, n_rec=n_rec)
        if rep:
            wall.append((time.perf_counter() - t) * 1e3)
            stages.append(ctx.lift_stage_ms())
    ctx.timing_enable(False)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), name
    # the tiles that answer: those that hold a queried base, and those that hold the start of a queried base's record
    is_base = np.zeros(256, dtype=bool)
    is_base[list(b"ACGTacgt")] = True
    line = length if length < 200 else 100
    rec_bytes = 10 + length // line * (line + 1)
    in_seq = (np.arange(len(text)) % rec_bytes) >= 10
    pos = np.flatnonzero(is_base[text] & in_seq)
    base_tiles = len(np.unique(pos[base] // TILE))
    start_tiles = len(np.unique((np.unique(want[1]).astype(np.int64) * rec_bytes - 1)[1:] // TILE)) if n_rec > 1 else 0
    len_tiles = len(np.unique((np.arange(1, n_rec, dtype=np.int64) * rec_bytes - 1) // TILE)) if n_rec > 1 else 0
    moved = len(text) + (base_tiles + start_tiles + len_tiles) * TILE
    total = [s["count"] + s["scan"] + s["answer"] for s in stages]
    out = {"tool": "lift_bench", "set": name, "records": n_rec, "text_bytes": int(len(text)), "kept_bases": int(n_bases), "queries": int(len(base)), "reps": REPS,
           "count_ms": spread([s["count"] for s in stages]), "scan_ms": spread([s["scan"] for s in stages]), "answer_ms": spread([s["answer"] for s in stages]),
           "stages_ms": spread(total), "call_wall_ms": spread(wall), "tiles": int(-(-len(text) // TILE)), "tiles_that_answer_bases": base_tiles,
           "tiles_that_answer_record_starts": start_tiles, "tiles_that_answer_lengths": len_tiles, "bytes_moved": int(moved),
           "ingest_wall_ms": spread(ingest), "hbm_copy_GBps": hbm["copy_GBps"]}
    out["GBps"] = moved / out["stages_ms"]["median"] / 1e6
    out["over_hbm_copy"] = out["GBps"] / hbm["copy_GBps"]
    out["call_wall_over_ingest_wall"] = out["call_wall_ms"]["median"] / out["ingest_wall_ms"]["median"]
    print(json.dumps(out), flush=True)
    ctx.close()


def road():
    rng = np.random.default_rng(11)
    ctx = sp.Context(0)
    genomes = [ACGT[rng.integers(0, 4, 200000, dtype=np.uint8)].tobytes() for _ in range(16)]
    n_rec, length, n_run = SETS["contigs"]
    with tempfile.TemporaryDirectory() as root:
        paths = []
        for i, g in enumerate(genomes):
            paths.append(os.path.join(root, "ref%02d.sk.gz" % i))
            sp.write_gz(paths[-1], ctx.sketch_text(b">g%d\n" % i + g + b"\n", K, 11, 100.0)[0], 1)
        parts = []
        for r in range(n_rec):                              # a contig: two stretches of two references joined by a run of N
            a, b = genomes[r % 16], genomes[(r * 7 + 3) % 16]
            at = int(rng.integers(0, 200000 - length))
            half = (length - n_run) // 2
            parts.append(b">c%d\n" % r + a[at:at + half] + b"N" * n_run + b[at:at + length - n_run - half] + b"\n")
        with open(os.path.join(root, "contigs.fa"), "wb") as f:
            f.write(b"".join(parts))
        for kw in ({}, {"raw": True}, {"segments": "all"}, {"segments": "all", "raw": True}):
            times = []
            for rep in range(4):
                t = time.perf_counter()
                ctx.classify_files(paths, os.path.join(root, "contigs.fa"), os.path.join(root, "out"), window=W, **kw)
                times.append(time.perf_counter() - t)
            lw = ctx.last_windows
            print(json.dumps({"tool": "lift_bench", "set": "road: classify_files over the contigs, 16 references, W = 1000", "records": n_rec, "asked": kw,
                              "segments": len(lw["segments"]), "bed_bytes": lw.get("bed_bytes", 0), "seconds": spread(times[1:])}), flush=True)
    ctx.close()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    c = sp.Context(0)
    hbm = c.measure_hbm()
    c.close()
    print(json.dumps({"tool": "lift_bench", "yardstick": "spsp_measure_hbm_device", **hbm}), flush=True)
    for name in SETS:
        if which in (name, "all"):
            run(name, hbm)
    if which in ("road", "all"):
        road()
