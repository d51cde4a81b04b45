#!/usr/bin/env python3
"""Cost of the windows pass on one MI355X: the three stages of the expansion, the bytes its copy moves over its time next to the
device's streaming copy rate and to the extraction's copy of as many bytes, and the whole classify road with and without windows.

Three record sets, made on the host from a seed, cleaned and uploaded once:

  reads        10^6 records of 150 bases          (one window each at either width)
  contigs      10^5 records of 5 000 bases
  chromosome   one record of 100 Mbp

Per set: W = 1 000 and 5 000 at k = 31, the ASCII form and the packed form.  spsp_records_windows_device timed by the events
between its launches (spsp_windows_stage_ms: count, offsets, copy): one call that is dropped, then REPS calls; printed are each
stage's median and its spread, and the copy's rate -- the bytes it reads and writes over its time (ASCII: a byte per base each
way; packed: a quarter).  The yardsticks of the same run: spsp_measure_hbm_device's copy rate, and the keep-all extraction's copy
(k_ex_copy) of a one-record text of as many bytes as the expansion's ASCII output.  The ratios are written down, not gated.

The road: spsp_classify_files over the contigs against 16 references, without a window and with W = 1 000 and 5 000, wall clock.

Asserted is the ANSWER: first_win, the offsets and every base of every expansion equal the host function's.  No time is asserted.

usage (GPU box): python tools/windows_bench.py [reads|contigs|chromosome|road|all]   (one JSON line per measurement on stdout)"""
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
WIDTHS = (1000, 5000)
SETS = {"reads": (1000000, 150), "contigs": (100000, 5000), "chromosome": (1, 100000000)}
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def spread(xs):
    a = np.array(xs)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def pack(bases):
    code = np.zeros(256, dtype=np.uint32)
    code[ACGT] = np.arange(4, dtype=np.uint32)
    c = code[bases]
    c = np.concatenate([c, np.zeros(-len(c) % 16, dtype=np.uint32)]).reshape(-1, 16)
    return (c << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


def unpack(words, n):
    return ACGT[((words[:, None] >> (30 - 2 * np.arange(16, dtype=np.uint32))) & 3).reshape(-1)[:n]]


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
    ctx.timing_enable(True)
    for W in WIDTHS:
        want, first, win_off = sp.windows_expand(bases, off, K, W)
        # the second yardstick: the extraction's copy of one record of as many bytes
        text = np.concatenate([np.frombuffer(b">r\n", np.uint8), want, np.frombuffer(b"\n", np.uint8)])
        d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, np.uint8)])).cuda()
        torch.cuda.synchronize()
        ex = []
        for rep in range(REPS + 1):
            ctx.extract_stage_ms()
            ctx.records_extract_device(d_text.data_ptr(), len(text), np.ones(1, np.uint8))
            if rep:
                ex.append(ctx.extract_stage_ms()["copy"])
        del d_text
        ex_copy = spread(ex)
        for packed in (False, True):
            stages = []
            for rep in range(REPS + 1):
                ctx.windows_stage_ms()
                out, n_out, d_win, got_first, n_win = ctx.records_windows_device(forms[packed].data_ptr(), len(bases), d_off.data_ptr(), n_rec, K, W, packed)
                if rep:
                    stages.append(ctx.windows_stage_ms())
            assert n_out == len(want) and (got_first == first).all() and (ctx.to_host(d_win, n_win + 1, np.uint64) == win_off).all(), (name, W, packed)
            got = unpack(ctx.to_host(out, -(-n_out // 16), np.uint32), n_out) if packed else ctx.to_host(out, n_out, np.uint8)
            assert (got == want).all(), (name, W, packed)
            line = {"tool": "windows_bench", "set": name, "records": n_rec, "bases": len(bases), "k": K, "window": W, "form": "packed" if packed else "ascii",
                    "windows": int(n_win), "out_bases": int(n_out), "reps": REPS}
            for s in ("count", "offsets", "copy"):
                line[s + "_ms"] = spread([x[s] for x in stages])
            moved = 2 * n_out / (4 if packed else 1)
            line["copy_bytes_moved"] = moved
            line["copy_GBps"] = moved / line["copy_ms"]["median"] / 1e6
            line["hbm_copy_GBps"] = hbm["copy_GBps"]
            line["copy_over_hbm_copy"] = line["copy_GBps"] / hbm["copy_GBps"]
            line["extract_copy_ms"] = ex_copy
            line["extract_copy_GBps"] = 2 * len(text) / ex_copy["median"] / 1e6
            line["copy_ms_over_extract_copy_ms"] = line["copy_ms"]["median"] / ex_copy["median"]
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
        for W in (None,) + WIDTHS:
            times = []
            for rep in range(3):
                t = time.perf_counter()
                rows, _ = ctx.classify_files(paths, os.path.join(root, "contigs.fa"), os.path.join(root, "out"), window=W)
                times.append(time.perf_counter() - t)
            line = {"tool": "windows_bench", "set": "road: classify_files over the contigs, 16 references", "records": n_rec, "window": W, "rows": len(rows),
                    "seconds": spread(times[1:])}
            if W:
                line["records_with_two_or_more_calls"] = int((ctx.last_windows["mosaic"]["calls"] >= 2).sum())
                line["segments"] = len(ctx.last_windows["segments"])
            print(json.dumps(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    c = sp.Context(0)
    hbm = c.measure_hbm()
    c.close()
    print(json.dumps({"tool": "windows_bench", "yardstick": "spsp_measure_hbm_device", **hbm}), flush=True)
    for name in SETS:
        if which in (name, "all"):
            run(name, hbm)
    if which in ("road", "all"):
        road()
