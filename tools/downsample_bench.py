#!/usr/bin/env python3
"""Cost of bringing sketches of mixed sampling rates to a common one (spsp_keys_downsample_device, compare_files(rate=...)).

  kernel leg   the pass alone over synthesised key arrays (sorted per sketch, ~20 keys per minimizer as a sketch's buckets hold
               them; a tenth of the keys pass): 10 000 sketches x 6 000, 65 535 x 900, 8 x 3 000 000.  Milliseconds by HIP
               events around the call on the context's stream (its offset copies and its one host wait are inside) and by the
               wall clock; the bytes the pass must move (k <= 32: 4 B read per key + 8 B read and 12 B written per survivor)
               over the streaming rate spsp_measure_hbm_device reports on the same context.
  files leg    N sketch files through compare_files: `mixed` = sketched at rate 10, compared with rate="auto" next to N/20
               files at rate 100; `coarse` = the same genomes sketched at rate 100 directly, compared as they are.  Run the
               second form with SPSP_LIB=<the parent commit's libspsp.so> to put the feature's cost beside the old path.

usage (GPU box): python tools/downsample_bench.py kernel [reps=5]
                 python tools/downsample_bench.py files mixed|coarse [N=1000] [genome length=600000]"""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import supersampler_amd as sp  # noqa: E402
from supersampler_amd import synth  # noqa: E402

K, M = 31, 11


def synth_keys(n, per, seed):
    """n sketches of `per` keys on the device: per / 20 random minimizers each, sorted, 20 keys per minimizer"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    runs = max(1, per // 20)
    mn = torch.randint(0, 4 ** M, (n, runs), generator=g, device="cuda", dtype=torch.int64).sort(dim=1).values
    mn = mn.repeat_interleave(20, dim=1).to(torch.int32).contiguous()            # (4^11 < 2^31: the bits are the uint32's)
    lo = torch.randint(0, 2 ** 62, (n * runs * 20,), generator=g, device="cuda", dtype=torch.int64)
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(runs * 20)
    return mn.reshape(-1), lo, off


def kernel_leg(reps):
    stream = torch.cuda.Stream()                                                 # (not the null stream: the context runs on this one, and so do the events)
    ctx = sp.Context(0, stream=stream.cuda_stream)
    hbm = ctx.measure_hbm(1 << 30, 10)
    thr = (1 << 64) // 10                                                        # a tenth of the minimizers pass
    doc = {"leg": "kernel", "k": K, "m": M, "hbm_copy_GBps": hbm["copy_GBps"], "hbm_read_GBps": hbm["read_GBps"], "shapes": []}
    for n, per in ((10_000, 6_000), (65_535, 900), (8, 3_000_000), (1, 6_000)):
        mn, lo, off = synth_keys(n, per, 7 + n)
        torch.cuda.synchronize()
        keys = int(off[-1])
        ev_ms, wall_ms, out = [], [], None
        for r in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record(stream)
            out = ctx.keys_downsample_device(K, thr, mn.data_ptr(), lo.data_ptr(), None, off)
            b.record(stream)
            b.synchronize()
            if r:                                                                 # (the first call allocates)
                wall_ms.append((time.perf_counter() - t0) * 1e3)
                ev_ms.append(a.elapsed_time(b))
        kept = int(out[3][-1])
        must = 4 * keys + 20 * kept
        best = min(ev_ms)
        doc["shapes"].append({"sketches": n, "keys_in": keys, "keys_out": kept, "event_ms_best": best, "event_ms_median": float(np.median(ev_ms)),
                              "wall_ms_best": min(wall_ms), "ns_per_key": best * 1e6 / keys, "bytes_must_move": must,
                              "GBps_of_must_move": must / best / 1e6, "fraction_of_hbm_copy_rate": must / best / 1e6 / hbm["copy_GBps"]})
        del mn, lo
    ctx.close()
    print(json.dumps(doc))


def files_leg(form, n, length):
    tmp = tempfile.mkdtemp(prefix="spsp_ds_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        gs = synth.family_genomes(5, n, length, max(1, n // 20), [0.001, 0.01, 0.05])
        ins = []
        for i, g in enumerate(gs):
            pth = os.path.join(tmp, "g%05d.fa" % i)
            open(pth, "wb").write(synth.to_fasta(g, "g%d" % i))
            ins.append(pth)
        outs = [os.path.join(tmp, "s%05d.gz" % i) for i in range(n)]
        if form == "mixed":                                                       # every 20th file is at the common rate already
            fine = [i for i in range(n) if i % 20]
            rest = [i for i in range(n) if i % 20 == 0]
            sp.sketch_files([ins[i] for i in fine], [outs[i] for i in fine], K, M, 10.0, threads=16)
            sp.sketch_files([ins[i] for i in rest], [outs[i] for i in rest], K, M, 100.0, threads=16)
        else:
            sp.sketch_files(ins, outs, K, M, 100.0, threads=16)
        sp.sketch_files_release()
        size = sum(os.path.getsize(p) for p in outs)
        ctx = sp.Context(0)
        kw = {"rate": "auto"} if form == "mixed" else {}
        ctx.compare_files(outs[:40], os.path.join(tmp, "warm"), **kw)
        runs = []
        for _ in range(3):
            ctx.stage_times(reset=True)
            t0 = time.perf_counter()
            ctx.compare_files(outs, os.path.join(tmp, "res"), **kw)
            wall = time.perf_counter() - t0
            st = ctx.stage_times(reset=True)
            runs.append({"wall_s": wall, **{f: st[f] for f in ("load_s", "compare_s", "csv_s", "csv_gzip_s")}})
        ctx.close()
        print(json.dumps({"leg": "files", "form": form, "library": sp.library_info(), "files": n, "genome_length": length, "sketch_bytes_gz": size,
                          "best": min(runs, key=lambda r: r["wall_s"]), "runs": runs}))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    leg = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if leg == "kernel":
        kernel_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    else:
        files_leg(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1000, int(sys.argv[4]) if len(sys.argv) > 4 else 600_000)
