#!/usr/bin/env python3
"""Cost of the extraction pass on one MI355X: the copy kernel next to a plain device-to-device copy of the same bytes, and the
whole pass next to what surrounds it in the file drivers.

Three texts, made on the host from a seed and uploaded once:

  reads    10^6 FASTQ records of 150 bases                 (314 MB)
  contigs  10^5 FASTA records of 5 000 bases                (501 MB)
  mixed    one FASTA record of 10 Mbp among 10^5 records of 300 bytes

Per text and keep pattern (1 %, 50 %, 100 %, alternating): spsp_records_extract_device with the starts made in the call, timed
by the events between its launches (spsp_extract_stage_ms: starts, offsets, copy), the median of REPS calls behind one that is
dropped.  The context runs on a torch stream, and the yardstick runs on that same stream between two events: dst.copy_(src) of
exactly n_out bytes, which is hipMemcpyDtoDAsync.  The parent has no such kernel, so the plain copy is what the copy kernel is
held against; both read and write n_out bytes.  Also printed, once per text at keep-all: the host functions' time on the same
text (spsp_records_extents_host + spsp_records_extract_host), the device-to-host copy of the output, and zlib at level 1 over it
(what the drivers' gzip costs) -- and the device pass's share of device pass + copy back + gzip.

Then the driver itself, once per text: the text written to a file, an index of 8 sketches (k = 31, m = 11, s = 4), each made of
2 000 consecutive records of that text (1 250 for the two FASTA texts), and spsp_classify_files_extract with `unmatched` -- nearly every
record is kept, so the device pass inside it is the keep-all line's -- timed on the host around the whole call, plain and gzipped,
behind one call that is dropped.  Printed: the two wall times and the keep-all device pass as a share of each.

Asserted is the ANSWER: every output equals the host functions' bytes.  No time is asserted.

usage (GPU box): python tools/extract_bench.py [reads|contigs|mixed|all]   (one JSON line per measurement on stdout)"""
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import supersampler_amd as sp  # noqa: E402

REPS = 5


def fixed_records(rng, n, head, bases, fastq):
    """n records of one width: a header of `head` bytes with the record's number, `bases` random bases on one line [, "+", qualities]"""
    width = head + 1 + bases + 1 + ((2 + bases + 1) if fastq else 0)
    a = np.empty((n, width), dtype=np.uint8)
    a[:, 0] = ord("@" if fastq else ">")
    digits = np.arange(n, dtype=np.int64)
    for c in range(head - 1, 0, -1):
        a[:, c] = 48 + digits % 10
        digits //= 10
    a[:, head] = 10
    a[:, head + 1:head + 1 + bases] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, bases), dtype=np.uint8)]
    a[:, head + 1 + bases] = 10
    if fastq:
        q = head + 2 + bases
        a[:, q] = ord("+")
        a[:, q + 1] = 10
        a[:, q + 2:q + 2 + bases] = rng.integers(35, 74, (n, bases), dtype=np.uint8)   # (some quality lines begin with '@' or '>')
        a[:, q + 2 + bases] = 10
    return a.reshape(-1)


def make_text(name, rng):
    if name == "reads":
        return fixed_records(rng, 1000000, 10, 150, True)
    if name == "contigs":
        return fixed_records(rng, 100000, 8, 5000, False)
    short = fixed_records(rng, 100000, 8, 290, False)      # 300 bytes each
    half = len(short) // 2
    long_one = np.concatenate([np.frombuffer(b">contig_10Mbp\n", dtype=np.uint8), np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 10000000, dtype=np.uint8)],
                               np.frombuffer(b"\n", dtype=np.uint8)])
    return np.concatenate([short[:half], long_one, short[half:]])


def keeps(n, rng):
    return {"1%": (rng.random(n) < 0.01).astype(np.uint8), "50%": (rng.random(n) < 0.5).astype(np.uint8), "100%": np.ones(n, dtype=np.uint8),
            "alternating": (np.arange(n) & 1).astype(np.uint8)}


def median(xs):
    return float(np.median(np.array(xs)))


def run(name):
    rng = np.random.default_rng(7)
    text = make_text(name, rng)
    n = len(text)
    stream = torch.cuda.Stream()
    ctx = sp.Context(0, stream=stream.cuda_stream)
    d_text = torch.from_numpy(np.concatenate([text, np.zeros(16, dtype=np.uint8)])).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    begin = sp.records_extents(text.tobytes())
    t_extents = time.perf_counter() - t0
    n_rec = len(begin) - 1
    d_begin, n_dev = ctx.records_extents_device(d_text.data_ptr(), n)
    assert n_dev == n_rec and (ctx.to_host(d_begin, n_rec + 1, np.uint64) == begin).all(), "starts"
    out, n_out, n_kept = sp.C.c_void_p(), sp.C.c_uint64(), sp.C.c_uint64()
    device_keep_all_ms = 0.0
    for label, keep in keeps(n_rec, rng).items():
        t0 = time.perf_counter()
        want, _ = sp.records_extract(text.tobytes(), keep, begin)
        t_host = time.perf_counter() - t0
        stages, walls = [], []
        ctx.timing_enable(True)
        for rep in range(REPS + 1):
            ctx.extract_stage_ms()
            t0 = time.perf_counter()
            sp._check(sp.lib().spsp_records_extract_device(ctx._h, d_text.data_ptr(), n, None, n_rec, keep.ctypes.data, sp.C.byref(out), sp.C.byref(n_out),
                                                           sp.C.byref(n_kept)))
            wall = time.perf_counter() - t0
            if rep:
                stages.append(ctx.extract_stage_ms())
                walls.append(wall * 1e3)
        ctx.timing_enable(False)
        t0 = time.perf_counter()
        got = ctx.to_host(out.value, n_out.value, np.uint8)
        t_d2h = time.perf_counter() - t0
        assert n_out.value == len(want) and got.tobytes() == want, "the output of %s / %s" % (name, label)
        # the yardstick: a plain device-to-device copy of n_out bytes on the context's stream
        src = torch.empty(max(n_out.value, 1), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        plain = []
        with torch.cuda.stream(stream):
            for rep in range(REPS + 1):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                dst.copy_(src)
                b.record(stream)
                b.synchronize()
                if rep:
                    plain.append(a.elapsed_time(b))
        line = {"tool": "extract_bench", "text": name, "text_bytes": n, "records": n_rec, "keep": label, "kept": int(n_kept.value), "out_bytes": int(n_out.value),
                "starts_ms": median([s["starts"] for s in stages]), "offsets_ms": median([s["offsets"] for s in stages]),
                "copy_ms": median([s["copy"] for s in stages]), "call_wall_ms": median(walls), "plain_copy_ms": median(plain),
                "host_extract_ms": t_host * 1e3, "reps": REPS}
        line["copy_over_plain"] = line["copy_ms"] / line["plain_copy_ms"] if line["plain_copy_ms"] else None
        line["copy_GBps"] = 2 * line["out_bytes"] / line["copy_ms"] / 1e6 if line["copy_ms"] else None
        if label == "100%":
            t0 = time.perf_counter()
            zlib.compress(want, 1)
            t_gzip = time.perf_counter() - t0
            device_ms = line["starts_ms"] + line["offsets_ms"] + line["copy_ms"]
            line.update({"host_extents_ms": t_extents * 1e3, "d2h_ms": t_d2h * 1e3, "gzip1_ms": t_gzip * 1e3,
                         "device_share_of_pass_d2h_gzip": device_ms / (device_ms + t_d2h * 1e3 + t_gzip * 1e3)})
            device_keep_all_ms = device_ms
        print(json.dumps(line), flush=True)
    ctx.close()
    driver(name, text, begin, device_keep_all_ms)


def driver(name, text, begin, device_ms):
    """the whole file driver on the same text: its wall time, and the keep-all device pass as a share of it"""
    root = tempfile.mkdtemp(prefix="extract_bench_")
    ctx = sp.Context(0)
    try:
        n_rec = len(begin) - 1
        per = min(2000, n_rec // 80)
        paths = []
        for j in range(8):                                 # every other block of `per` records is a reference: its records match
            a, b = int(begin[2 * j * per]), int(begin[(2 * j + 1) * per])
            payload, _ = ctx.sketch_text(text[a:b].tobytes(), 31, 11, 4.0)
            paths.append(os.path.join(root, "ref%d.sk.gz" % j))
            sp.write_gz(paths[-1], payload, 1)
        rec_path = os.path.join(root, "records.fq" if text[0] == ord("@") else "records.fa")
        text.tofile(rec_path)
        walls = {}
        for label, gz in (("dropped", False), ("plain", False), ("gzip", True)):
            t0 = time.perf_counter()
            records, _ = ctx.classify_files(paths, rec_path, os.path.join(root, "out"), extract="unmatched", gz=gz)
            walls[label] = (time.perf_counter() - t0) * 1e3
        line = {"tool": "extract_bench", "text": name, "driver": "spsp_classify_files_extract, unmatched, 8 references", "records": int(len(records)),
                "kept": ctx.last_extract["n_kept"], "out_bytes": ctx.last_extract["bytes_out"], "driver_wall_plain_ms": walls["plain"],
                "driver_wall_gzip_ms": walls["gzip"], "device_pass_keep_all_ms": device_ms,
                "device_share_of_driver_plain": device_ms / walls["plain"], "device_share_of_driver_gzip": device_ms / walls["gzip"]}
        print(json.dumps(line), flush=True)
    finally:
        ctx.close()
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    for name in ("reads", "contigs", "mixed"):
        if which in (name, "all"):
            run(name)
