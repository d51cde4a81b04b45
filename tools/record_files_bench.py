#!/usr/bin/env python3
"""Wall clock of the record file drivers on one MI355X: the modes of Context.classify_files and taxonomy_files (the ten file
entries behind them), depth_files and profile_files, on one input: 16 references of
200 kbp at rate 100, 20 000 records of 1 000 bases (and as many mates).  One JSON line: per mode the median, min and max of 5
calls behind a warm-up call, in milliseconds.  SPSP_LIB: another library, as everywhere.
usage (GPU box): python tools/record_files_bench.py"""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402

import supersampler_amd as sp  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def main():
    rng = np.random.default_rng(7)
    ctx = sp.Context(0)
    genomes = [ACGT[rng.integers(0, 4, 200000, dtype=np.uint8)].tobytes() for _ in range(16)]
    n_rec, length = 20000, 1000
    out = {"tool": "record_files_bench", "library": sp.library_info(), "records": n_rec}
    with tempfile.TemporaryDirectory() as root:
        paths = []
        for i, g in enumerate(genomes):
            paths.append(os.path.join(root, "ref%02d.sk.gz" % i))
            sp.write_gz(paths[-1], ctx.sketch_text(b">g%d\n" % i + g + b"\n", 31, 11, 100.0)[0], 1)
        for name, shift in (("r1.fa", 0), ("r2.fa", 5000)):
            parts = []
            for r in range(n_rec):
                g = genomes[r % 16]
                at = (r * 37 + shift) % (200000 - length)
                parts.append(b">c%d\n" % r + g[at:at + length] + b"\n")
            with open(os.path.join(root, name), "wb") as f:
                f.write(b"".join(parts))
        with open(os.path.join(root, "lin.txt"), "w") as f:
            f.write("".join("Bacteria;G%d;s%d\n" % (i // 4, i) for i in range(16)))
        r1, r2, lin, pre = (os.path.join(root, x) for x in ("r1.fa", "r2.fa", "lin.txt", "out"))
        modes = {"classify": lambda: ctx.classify_files(paths, r1, pre),
                 "classify_extract": lambda: ctx.classify_files(paths, r1, pre, extract="matched", gz=False),
                 "classify_paired": lambda: ctx.classify_files(paths, r1, pre, mates_path=r2),
                 "classify_paired_extract": lambda: ctx.classify_files(paths, r1, pre, mates_path=r2, extract="matched", gz=False),
                 "classify_split": lambda: ctx.classify_files(paths, r1, pre, split="best", gz=False),
                 "classify_windows": lambda: ctx.classify_files(paths, r1, pre, window=400),
                 "taxonomy": lambda: ctx.taxonomy_files(paths, r1, lin, pre),
                 "taxonomy_extract": lambda: ctx.taxonomy_files(paths, r1, lin, pre, extract="classified", gz=False),
                 "taxonomy_paired": lambda: ctx.taxonomy_files(paths, r1, lin, pre, mates_path=r2),
                 "taxonomy_split": lambda: ctx.taxonomy_files(paths, r1, lin, pre, split="depth=2", mates_path=r2, gz=False),
                 "taxonomy_windows": lambda: ctx.taxonomy_files(paths, r1, lin, pre, window=400),
                 "depth": lambda: ctx.depth_files(paths, [r1, r2], pre),
                 "profile": lambda: ctx.profile_files(paths, [r1, r2], pre)}
        for name, call in modes.items():
            call()
            times = []
            for _ in range(5):
                t = time.perf_counter()
                call()
                times.append((time.perf_counter() - t) * 1e3)
            out[name + "_wall_ms"] = {"median": float(np.median(times)), "min": min(times), "max": max(times)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
