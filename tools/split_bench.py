#!/usr/bin/env python3
"""Cost of the split pass on one MI355X: its five stages next to the keep-all extraction of the same text, which moves the same
bytes through the same schedule and is the yardstick for the copy.

Two texts, made on the host from a seed and uploaded once:

  reads    10^6 FASTQ records of 150 bases                          (314 MB)
  contigs  10^4 FASTA records with a long tail: 9 900 of 500 .. 20 000 bases, 100 of 0.2 .. 2 Mbp

Per text: n_bins of 1, 16, 4 096 and 65 536; labels random per record, and in blocks of 1 000 records (contigs: of 100).
spsp_records_split_device with the starts made in the call, timed by the events between its launches (spsp_split_stage_ms:
starts, runs, order, offsets, copy): one call that is dropped, then REPS calls; printed are each stage's median and its spread
(min, max).  Beside them, once per text and measured the same way, spsp_records_extract_device with every flag set
(spsp_extract_stage_ms), and per line the ratio of the split's copy to that copy.

Asserted is the ANSWER: every output, bin_off and bin_records equal the host function's.  No time is asserted.

usage (GPU box): python tools/split_bench.py [reads|contigs|all]   (one JSON line per measurement on stdout)"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import supersampler_amd as sp  # noqa: E402
from tools.extract_bench import fixed_records  # noqa: E402

REPS = 7
N_BINS = (1, 16, 4096, 65536)


def make_text(name, rng):
    if name == "reads":
        return fixed_records(rng, 1000000, 10, 150, True), 1000
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    lengths = np.concatenate([rng.integers(500, 20000, 9900), rng.integers(200000, 2000000, 100)])
    rng.shuffle(lengths)
    parts = []
    for i, n in enumerate(lengths.tolist()):
        parts += [np.frombuffer(b">contig_%d\n" % i, dtype=np.uint8), acgt[rng.integers(0, 4, n, dtype=np.uint8)], np.frombuffer(b"\n", dtype=np.uint8)]
    return np.concatenate(parts), 100


def spread(xs):
    a = np.array(xs)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def run(name):
    rng = np.random.default_rng(7)
    text, block = make_text(name, rng)
    n = len(text)
    raw = text.tobytes()
    ctx = sp.Context(0)
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, dtype=np.uint8)])).cuda()
    torch.cuda.synchronize()
    begin = sp.records_extents(raw)
    n_rec = len(begin) - 1
    ctx.timing_enable(True)
    # the yardstick: the extraction with every flag set
    keep = np.ones(n_rec, dtype=np.uint8)
    stages = []
    for rep in range(REPS + 1):
        ctx.extract_stage_ms()
        out, kept = ctx.records_extract_device(d_text.data_ptr(), n, keep)
        if rep:
            stages.append(ctx.extract_stage_ms())
    assert kept == n_rec and out.tobytes() == sp.records_extract(raw, keep, begin)[0], "keep-all"
    keep_all = {k: spread([s[k] for s in stages]) for k in ("starts", "offsets", "copy")}
    print(json.dumps({"tool": "split_bench", "text": name, "text_bytes": n, "records": n_rec, "call": "extract keep-all", "out_bytes": len(out), "reps": REPS,
                      **{k + "_ms": v for k, v in keep_all.items()}}), flush=True)
    for n_bins in N_BINS:
        for labels in ("random", "blocks"):
            if n_bins == 1 and labels == "blocks":
                continue
            bins = rng.integers(0, n_bins, n_rec).astype(np.uint32) if labels == "random" else (rng.integers(0, n_bins, n_rec // block + 1).astype(np.uint32))[np.arange(n_rec) // block]
            stages = []
            for rep in range(REPS + 1):
                ctx.split_stage_ms()
                out, off, rec = ctx.records_split_device(d_text.data_ptr(), n, bins, n_bins)
                if rep:
                    stages.append(ctx.split_stage_ms())
            want = sp.records_split(raw, bins, n_bins, begin)
            assert out.tobytes() == want[0] and (off == want[1]).all() and (rec == want[2]).all(), "the output of %s / %d / %s" % (name, n_bins, labels)
            runs = int(1 + np.count_nonzero(bins[1:] != bins[:-1]))
            line = {"tool": "split_bench", "text": name, "text_bytes": n, "records": n_rec, "call": "split", "n_bins": n_bins, "labels": labels, "runs": runs,
                    "out_bytes": len(out), "reps": REPS}
            for k in ("starts", "runs", "order", "offsets", "copy"):
                line[k + "_ms"] = spread([s[k] for s in stages])
            line["copy_over_keep_all_copy"] = line["copy_ms"]["median"] / keep_all["copy"]["median"]
            line["copy_GBps"] = 2 * len(out) / line["copy_ms"]["median"] / 1e6
            print(json.dumps(line), flush=True)
    ctx.timing_enable(False)
    ctx.close()


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for name in ("reads", "contigs"):
        if which in (name, "all"):
            run(name)
