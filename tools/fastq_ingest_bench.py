"""FASTQ ingest against FASTA ingest over the same bases, on the GPU.

Prints, for a simulated read set (fixed-length reads, both in FASTQ and in its FASTA form ">" + name + "\\n" + seq + "\\n"):
  * the device ingest time per input byte (and per base) of spsp_fasta_clean_device / spsp_fastq_clean_device and their
    packed forms (median of --reps calls; each call waits for its result);
  * the end-to-end wall time of sketch_files over the read set written as one FASTQ file (and as its FASTA form).
One JSON line at the end holds every figure.

    python tools/fastq_ingest_bench.py [--reads 4000000] [--len 150] [--ingest-reads 1500000] [--abundance 2]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_set(rng, n, length, genome_len=5_000_000):
    """n reads of `length` bases sampled from a random genome (1 % substitutions) -> (fastq bytes, fasta bytes)"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, size=genome_len, dtype=np.uint8)]
    starts = rng.integers(0, genome_len - length, size=n)
    seqs = genome[starts[:, None] + np.arange(length)[None, :]]
    flip = rng.random(seqs.shape) < 0.01
    seqs[flip] = acgt[rng.integers(0, 4, size=int(flip.sum()), dtype=np.uint8)]
    names = np.frombuffer(b"".join(b"r%010d" % i for i in range(n)), dtype=np.uint8).reshape(n, 11)
    qual = rng.integers(35, 74, size=(n, length), dtype=np.uint8)
    nl = np.full((n, 1), ord("\n"), dtype=np.uint8)
    fq = np.concatenate([np.full((n, 1), ord("@"), np.uint8), names, nl, seqs, nl, np.full((n, 1), ord("+"), np.uint8), nl, qual, nl], axis=1)
    fa = np.concatenate([np.full((n, 1), ord(">"), np.uint8), names, nl, seqs, nl], axis=1)
    return fq.tobytes(), fa.tobytes()


def time_ingest(ctx, fn, d, n, reps):
    fn(d.data_ptr(), n)                                   # warm-up (buffers grow once)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn(d.data_ptr(), n)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000, help="reads of the end-to-end read set")
    ap.add_argument("--ingest-reads", type=int, default=1_500_000, help="reads of the ingest measurement")
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--abundance", type=int, default=2)
    ap.add_argument("-s", type=float, default=1000.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    import torch
    import supersampler_amd as sp

    rng = np.random.default_rng(1)
    res = {"read_len": a.len}
    fq, fa = read_set(rng, a.ingest_reads, a.len)
    bases = a.ingest_reads * a.len
    ctx = sp.Context(0)
    for tag, text, plain, packed in (("fasta", fa, ctx.clean_fasta_device, ctx.clean_fasta_packed_device),
                                     ("fastq", fq, ctx.clean_fastq_device, ctx.clean_fastq_packed_device)):
        d = torch.from_numpy(np.frombuffer(text + b"\0" * 16, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        for form, fn in (("ascii", plain), ("packed", packed)):
            t = time_ingest(ctx, fn, d, len(text), a.reps)
            res["%s_%s_s" % (tag, form)] = t
            res["%s_%s_ns_per_byte" % (tag, form)] = t * 1e9 / len(text)
            res["%s_%s_ns_per_base" % (tag, form)] = t * 1e9 / bases
            print("%-6s %-6s %8.3f ms  %7.1f MB  %.4f ns/byte  %.4f ns/base  %.1f GB/s" %
                  (tag, form, t * 1e3, len(text) / 1e6, t * 1e9 / len(text), t * 1e9 / bases, len(text) / t / 1e9))
        res["%s_bytes" % tag] = len(text)
        del d
    for form in ("ascii", "packed"):
        res["fastq_over_fasta_per_byte_%s" % form] = res["fastq_%s_ns_per_byte" % form] / res["fasta_%s_ns_per_byte" % form]
        print("FASTQ / FASTA per byte (%s): %.2f" % (form, res["fastq_over_fasta_per_byte_%s" % form]))
    ctx.close()
    del fq, fa
    if not a.skip_e2e:
        fq, fa = read_set(rng, a.reads, a.len)
        with tempfile.TemporaryDirectory() as tmp:
            for tag, text in (("fastq", fq), ("fasta", fa)):
                pin = os.path.join(tmp, "reads." + ("fq" if tag == "fastq" else "fa"))
                with open(pin, "wb") as f:
                    f.write(text)
                out = os.path.join(tmp, "out_%s.gz" % tag)
                for rep in range(2):                       # the first call pays for contexts and pinned buffers
                    t0 = time.perf_counter()
                    r, times, _ = sp.sketch_files([pin], [out], 31, 11, a.s, abundance=a.abundance, threads=8)
                    t = time.perf_counter() - t0
                    assert r[0][0] == 0, r
                res["e2e_%s_s" % tag] = t
                res["e2e_%s_ingest_s" % tag] = times["ingest_s"]
                print("sketch_files %s: %d reads x %d bp (%.0f MB), -a %d -s %g: %.3f s (ingest stage %.3f s)" %
                      (tag, a.reads, a.len, len(text) / 1e6, a.abundance, a.s, t, times["ingest_s"]))
                os.remove(pin)
        res.update({"e2e_reads": a.reads, "e2e_abundance": a.abundance, "e2e_s": a.s})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
