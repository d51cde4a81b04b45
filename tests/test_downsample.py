"""Sketches of different sampling rates: a sketch made at rate s holds every coarser sketch of the same genome, and the
comparison brings all of them to a common rate first (include/spsp.h: spsp_keys_downsample_device, spsp_sketch_header_host,
spsp_sketch_downsample_host, spsp_compare_files_rate, spsp_compare_files_multi_rate; bin/comparator -s).

The rule is exact: a k-mer is selected iff XXH64 (seed 1312) of its canonical minimizer is <= threshold(k, m, s), so

    keys(sketch(G, s')) == [(min, kmer) in keys(sketch(G, s)) if xxh64(min) <= threshold(k, m, s')]      for s' >= s

and every expected value below is the ORACLE's direct sketch at the coarse rate: integers and bytes, no tolerance."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
from oracle import oracle_py as orc
from supersampler_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUF = ((True, "_jaccard.csv.gz"), (False, "_containment.csv.gz"))
CASES = [(k, m, ab) for (k, m) in ((31, 11), (21, 9), (63, 15), (31, 13)) for ab in (1, 2)]
FINE, COARSE = 10.0, 100.0


def _awkward_fasta(k, m, ab):
    """300 kbp in two records with a 2 kbp repeat, a homopolymer, a short-period repeat and an N; with -a 2 a third record
    repeats 58 kbp of the first, so that some k-mers are seen twice and most once"""
    rng = np.random.default_rng(500 + 7 * k + m + ab)
    g = synth.random_genome(rng, 300_000).tobytes()
    h = len(g) // 2
    g = g[:h] + g[1000:3000] + b"A" * 200 + b"AC" * 200 + b"N" + g[h:]
    text = b">a\n" + g[:150_000] + b"\n>b\n" + g[150_000:] + b"\n"
    if ab == 2:
        text += b">c\n" + g[2000:60_000] + b"\n"
    return text


_pair_cache = {}


def _pair(k, m, ab):
    if (k, m, ab) not in _pair_cache:
        t = _awkward_fasta(k, m, ab)
        _pair_cache[(k, m, ab)] = (orc.sketch_fasta(t, k, m, FINE, ab)[0], orc.sketch_fasta(t, k, m, COARSE, ab)[0])
    return _pair_cache[(k, m, ab)]


def _passes(mn, thr):
    return np.array([orc.xxh64(int(x)) <= thr for x in mn], dtype=bool)


# ------------------------------------------------------------------------------------------------ not GPU

@pytest.mark.parametrize("k,m,ab", CASES)
def test_fine_keys_filtered_by_the_coarse_threshold_are_the_coarse_keys(k, m, ab):
    """the rule everything else stands on, on the oracle alone: element by element, order included"""
    fine, coarse = _pair(k, m, ab)
    _, _, f_mn, f_lo, f_hi = orc.sketch_keys(fine)
    _, _, c_mn, c_lo, c_hi = orc.sketch_keys(coarse)
    keep = _passes(f_mn, orc.threshold(k, m, COARSE))
    assert 0 < len(c_mn) < len(f_mn)
    assert np.array_equal(f_mn[keep], c_mn) and np.array_equal(f_lo[keep], c_lo) and np.array_equal(f_hi[keep], c_hi)


def test_sketch_header_fields():
    t = _awkward_fasta(31, 11, 1)
    for s in (10.0, 100.0, 2.5):
        pl, st = orc.sketch_fasta(t, 31, 11, s)
        assert sp.sketch_header(pl) == (31, 11, st["selected_kmer_number"], s)
    pl = orc.sketch_fasta(t, 63, 15, 100.0)[0]
    assert sp.sketch_header(pl)[:2] == (63, 15)
    for bad in (b"51 11 1886\n", b"51 11\n"):
        with pytest.raises(sp.SpspError) as e:
            sp.sketch_header(bad)
        assert e.value.code == sp.ERR_FORMAT


@pytest.mark.parametrize("k,m,ab", CASES)
def test_sketch_downsample_payload_decodes_to_the_coarse_keys(k, m, ab):
    fine, coarse = _pair(k, m, ab)
    down = sp.sketch_downsample(fine, COARSE)
    got = sp.sketch_parse(down)
    _, _, c_mn, c_lo, c_hi = orc.sketch_keys(coarse)
    assert np.array_equal(got.minimizer, c_mn) and np.array_equal(got.kmer_lo, c_lo) and np.array_equal(got.kmer_hi, c_hi)
    assert sp.sketch_header(down) == (k, m, len(c_mn), COARSE)            # the third field: the distinct keys left
    assert orc.sketch_keys(down)[2].tolist() == c_mn.tolist()              # ... and the oracle's reader agrees on the file
    # its own rate: the sketch as it is; a finer one: refused
    assert sp.sketch_downsample(fine, FINE) == fine
    assert sp.sketch_downsample(down, COARSE) == down
    with pytest.raises(sp.SpspError) as e:
        sp.sketch_downsample(fine, FINE / 2)
    assert e.value.code == sp.ERR_ARG and "upsample" in str(e.value)
    # twice is once: 10 -> 30 -> 100 keeps what 10 -> 100 keeps
    assert sp.sketch_downsample(sp.sketch_downsample(fine, 30.0), COARSE) == down


def test_sketch_downsample_of_a_sketch_without_buckets():
    rng = np.random.default_rng(3)
    empty = orc.sketch_fasta(synth.to_fasta(synth.random_genome(rng, 20), "tiny"), 31, 11, FINE)[0]
    assert empty.count(b"\n") == 1 and empty.endswith(b"\n")
    down = sp.sketch_downsample(empty, COARSE)
    assert sp.sketch_header(down) == (31, 11, 0, COARSE) and down.count(b"\n") == 1 and down.endswith(b"\n")
    assert len(sp.sketch_parse(down)) == 0


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


def _host_keys(ctx, k, d_mn, d_lo, d_hi, total):
    mn, lo = ctx.to_host(d_mn, total, np.uint32), ctx.to_host(d_lo, total, np.uint64)
    hi = ctx.to_host(d_hi, total, np.uint64) if k > 32 else np.zeros(total, np.uint64)
    return mn, lo, hi


def _assert_keys(ctx, k, got, want_payloads, tag):
    d_mn, d_lo, d_hi, off = got
    want = [orc.sketch_keys(p) for p in want_payloads]
    assert off[0] == 0 and off.tolist() == np.concatenate([[0], np.cumsum([len(w[2]) for w in want])]).tolist(), tag
    mn, lo, hi = _host_keys(ctx, k, d_mn, d_lo, d_hi, int(off[-1]))
    assert np.array_equal(mn, np.concatenate([w[2] for w in want])), tag
    assert np.array_equal(lo, np.concatenate([w[3] for w in want])), tag
    assert np.array_equal(hi, np.concatenate([w[4] for w in want]) if k > 32 else np.zeros(len(mn), np.uint64)), tag


def _collection(k, m):
    """texts: 2 000 small genomes in families, one genome beyond the per-sketch LDS sort before and after (> 8 192 keys at both
    rates), one too short for a k-mer (a sketch without buckets), one sketched with -a 2"""
    rng = np.random.default_rng(77 + k)
    anc = [synth.random_genome(rng, 3_000) for _ in range(8)]
    texts = [(synth.to_fasta(synth.mutate(rng, anc[i % 8], [0.0, 0.01, 0.03][(i // 8) % 3]), "s%d" % i, n_records=1 + i % 2), 1) for i in range(2000)]
    texts.insert(700, (synth.to_fasta(synth.random_genome(rng, 1_200_000), "big", n_records=3), 1))
    texts.insert(1200, (synth.to_fasta(synth.random_genome(rng, k - 2), "short"), 1))
    texts.append((_awkward_fasta(k, m, 2), 2))
    return texts


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_keys_downsample_device_equals_the_oracles_coarse_keys(ctx, k, m):
    texts = _collection(k, m)
    fine = [orc.sketch_fasta(t, k, m, FINE, ab)[0] for t, ab in texts]
    coarse = [orc.sketch_fasta(t, k, m, COARSE, ab)[0] for t, ab in texts]
    thr = sp.threshold(k, m, COARSE)
    assert thr == orc.threshold(k, m, COARSE)
    n_big = [len(orc.sketch_keys(p[700])[2]) for p in (fine, coarse)]
    assert min(n_big) > 8192, n_big
    kk, mm, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(fine)
    assert (kk, mm) == (k, m) and off[1201] == off[1200]                     # (the sketch without buckets)
    got = ctx.keys_downsample_device(k, thr, d_mn, d_lo, d_hi, off)
    _assert_keys(ctx, k, got, coarse, "2003 sketches")
    assert got[3][1201] == got[3][1200]
    # the result feeds the comparison as it is (a slice of it: the big one, the -a 2 one and their neighbours)
    import torch
    pick = [698, 699, 700, 701, 2001, 2002]
    sub_fine = [fine[i] for i in pick]
    _, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(sub_fine)
    o_mn, o_lo, o_hi, o_off = ctx.keys_downsample_device(k, thr, d_mn, d_lo, d_hi, off)
    w_inter, w_card, _, _ = orc.compare([coarse[i] for i in pick])
    d_inter = torch.zeros((len(pick), len(pick)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.compare_device(k, o_mn, o_lo, o_hi, o_off, len(pick), 0, 1, d_inter.data_ptr())
    torch.cuda.synchronize()
    assert (np.triu(d_inter.cpu().numpy(), 1) == np.triu(w_inter.astype(np.int64), 1)).all()
    assert np.diff(o_off).tolist() == w_card.tolist()
    # nothing survives threshold 0; one sketch; one sketch without buckets; no sketch at all
    _, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(sub_fine)
    assert ctx.keys_downsample_device(k, 0, d_mn, d_lo, d_hi, off)[3].tolist() == [0] * (len(pick) + 1)
    _, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(fine[5:6])
    _assert_keys(ctx, k, ctx.keys_downsample_device(k, thr, d_mn, d_lo, d_hi, off), coarse[5:6], "n = 1")
    _, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(fine[1200:1201])
    assert ctx.keys_downsample_device(k, thr, d_mn, d_lo, d_hi, off)[3].tolist() == [0, 0]
    assert ctx.keys_downsample_device(k, thr, None, None, None, np.zeros(1, np.uint64))[3].tolist() == [0]
    # a chain 10 -> 30 -> 100: the second call reads what the first one wrote
    _, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(sub_fine)
    mid = ctx.keys_downsample_device(k, sp.threshold(k, m, 30.0), d_mn, d_lo, d_hi, off)
    _assert_keys(ctx, k, ctx.keys_downsample_device(k, thr, *mid), [coarse[i] for i in pick], "chain")


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_keys_downsample_device_of_unordered_keys(ctx, k, m):
    """the keys of spsp_sketch_keys_device(..., SPSP_KEYS_UNORDERED) -- distinct, in no order -- stay distinct: per sketch the
    SET of the oracle's coarse keys, and a comparison that has been told so counts the oracle's pairs"""
    import torch
    rng = np.random.default_rng(31 + k)
    a = synth.random_genome(rng, 60_000)
    b = synth.mutate(rng, a, 0.02)
    # -a 2: a k-mer counts from its second occurrence on -- records given twice count, the single ones do not
    genomes = [[a[:30_000], a[30_000:], a[:45_000]], [b, b[5_000:]], [synth.random_genome(rng, k - 1)], [a[:20_000]] * 2 + [a[20_000:25_000]],
               [synth.mutate(rng, a, 0.05)] * 2]
    ab = 2
    recs, first_rec, texts = [], [0], []
    for i, g in enumerate(genomes):
        recs += g
        first_rec.append(len(recs))
        texts.append(b"".join(synth.to_fasta(r, "g%d_%d" % (i, j)) for j, r in enumerate(g)))
    bases, off = synth.concat_records(recs)
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(64, np.uint8)])).cuda()
    d_o = torch.from_numpy(off.view(np.int64)).cuda()
    torch.cuda.synchronize()
    coarse = [orc.sketch_fasta(t, k, m, COARSE, ab)[0] for t in texts]
    want = [orc.sketch_keys(p) for p in coarse]
    p = sp.make_params(k, m, FINE, abundance=ab)
    d_sk, n_sk = ctx.scan_device(p, d_b.data_ptr(), len(bases), d_o.data_ptr(), len(recs))
    d_mn, d_lo, d_hi, sk_off = ctx.sketch_keys_device(p, d_b.data_ptr(), len(bases), d_o.data_ptr(), d_sk, n_sk, first_rec, unordered=True)
    o_mn, o_lo, o_hi, o_off = ctx.keys_downsample_device(k, sp.threshold(k, m, COARSE), d_mn, d_lo, d_hi, sk_off)
    mn, lo, hi = _host_keys(ctx, k, o_mn, o_lo, o_hi, int(o_off[-1]))
    assert sum(len(w[2]) for w in want) > 300
    for g, (_, _, w_mn, w_lo, w_hi) in enumerate(want):
        x, y = int(o_off[g]), int(o_off[g + 1])
        assert y - x == len(w_mn), (g, y - x, len(w_mn))
        assert set(zip(mn[x:y].tolist(), lo[x:y].tolist(), hi[x:y].tolist())) == set(zip(w_mn.tolist(), w_lo.tolist(), (w_hi if k > 32 else np.zeros(len(w_mn), np.uint64)).tolist())), g
    w_inter, _, _, _ = orc.compare(coarse)
    d_inter = torch.zeros((len(genomes), len(genomes)), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.compare_keys_unordered(True)
    try:
        ctx.compare_device(k, o_mn, o_lo, o_hi, o_off, len(genomes), 0, 1, d_inter.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.compare_keys_unordered(False)
    assert (np.triu(d_inter.cpu().numpy(), 1) == np.triu(w_inter.astype(np.int64), 1)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(31, 11), (63, 15)])
def test_keys_downsample_device_to_the_own_rate_is_the_identity(ctx, k, m):
    texts = _collection(k, m)[690:710]
    fine = [orc.sketch_fasta(t, k, m, FINE, ab)[0] for t, ab in texts]
    _, _, d_mn, d_lo, d_hi, off = ctx.sketch_decode_device(fine)
    before = _host_keys(ctx, k, d_mn, d_lo, d_hi, int(off[-1]))
    o_mn, o_lo, o_hi, o_off = ctx.keys_downsample_device(k, sp.threshold(k, m, FINE), d_mn, d_lo, d_hi, off)
    assert o_off.tolist() == off.tolist()
    after = _host_keys(ctx, k, o_mn, o_lo, o_hi, int(o_off[-1]))
    for b, a in zip(before, after):
        assert np.array_equal(b, a)
    _assert_keys(ctx, k, (o_mn, o_lo, o_hi, o_off), fine, "identity")


class Mixed:
    """>= 40 genomes in families; every other file sketched at s = 10, the rest at s = 100; `coarse`: the oracle's direct
    s = 100 sketches of the same genomes"""

    def __init__(self, root, k, m, n=44):
        self.k, self.m, self.root = k, m, root
        gs = synth.family_genomes(900 + k, n, 60_000, 4, [0.0, 0.01, 0.03])
        self.paths, self.mixed, self.coarse = [], [], []
        for i, g in enumerate(gs):
            t = synth.to_fasta(g, "g%d" % i, n_records=1 + i % 2)
            c = orc.sketch_fasta(t, k, m, COARSE)[0]
            f = orc.sketch_fasta(t, k, m, FINE)[0] if i % 2 == 0 else c
            pth = os.path.join(root, "k%d_%02d.gz" % (k, i))
            sp.write_gz(pth, f, 1)
            self.paths.append(pth); self.mixed.append(f); self.coarse.append(c)

    def want(self, payloads, n_query=None):
        inter, card, _, _ = orc.compare(payloads, n_query=n_query)
        return [orc.csv(jac, self.paths, inter, card, n_query, 6, 0.0) for jac, _ in SUF]

    def got(self, prefix):
        return [gzip.open(prefix + suf, "rb").read() for _, suf in SUF]


@pytest.fixture(scope="module")
def mixed31(tmp_path_factory):
    return Mixed(str(tmp_path_factory.mktemp("mixed31")), 31, 11)


@pytest.fixture(scope="module")
def mixed63(tmp_path_factory):
    return Mixed(str(tmp_path_factory.mktemp("mixed63")), 63, 15)


@pytest.mark.gpu
def test_compare_files_at_a_common_rate_equals_the_oracle_on_direct_coarse_sketches(ctx, mixed31, mixed63, tmp_path):
    for M in (mixed31, mixed63):
        want = M.want(M.coarse)
        inter = orc.compare(M.coarse)[0]
        assert np.count_nonzero(np.triu(inter, 1)) >= 200                  # families: many cells are non-zero
        tag = str(tmp_path / ("k%d" % M.k))
        ctx.compare_files(M.paths, tag + "_100", rate=100)
        assert M.got(tag + "_100") == want
        ctx.compare_files(M.paths, tag + "_auto", rate="auto")
        assert M.got(tag + "_auto") == want
        # rate = 0: the headers' rates are ignored, as before
        ctx.compare_files(M.paths, tag + "_asis", rate=0)
        assert M.got(tag + "_asis") == M.want(M.mixed)
        ctx.compare_files(M.paths, tag + "_default")
        assert M.got(tag + "_default") == M.want(M.mixed)
        assert M.want(M.mixed) != want
    M = mixed31
    tag = str(tmp_path / "q")
    ctx.compare_files(M.paths, tag, n_query=5, rate=100)                   # -q: the first five against all
    assert M.got(tag) == M.want(M.coarse, 5)
    ctx.compare_files(M.paths, tag + "a", n_query=5, rate="auto")
    assert M.got(tag + "a") == M.want(M.coarse, 5)
    # every sketch already at the common rate: nothing to bring down, same files
    cpaths = []
    for i, c in enumerate(M.coarse):
        cpaths.append(str(tmp_path / ("c%02d.gz" % i)))
        sp.write_gz(cpaths[-1], c, 1)
    ctx.compare_files(cpaths, tag + "c", rate=100)
    inter, card, _, _ = orc.compare(M.coarse)
    assert M.got(tag + "c") == [orc.csv(jac, cpaths, inter, card, None, 6, 0.0) for jac, _ in SUF]


@pytest.mark.gpu
def test_compare_files_refuses_to_upsample_and_mixed_k(ctx, mixed31, mixed63, tmp_path):
    M = mixed31
    rng = np.random.default_rng(12)
    far = str(tmp_path / "too_coarse.gz")
    sp.write_gz(far, orc.sketch_fasta(synth.to_fasta(synth.random_genome(rng, 400_000), "far"), 31, 11, 100_000.0)[0], 1)
    with pytest.raises(sp.SpspError) as e:
        ctx.compare_files(M.paths[:6] + [far] + M.paths[6:], str(tmp_path / "no"), rate=1000)
    assert e.value.code == sp.ERR_ARG and "too_coarse.gz" in str(e.value) and "100000" in str(e.value) and "1000" in str(e.value)
    with pytest.raises(sp.SpspError) as e:
        ctx.compare_files(M.paths, str(tmp_path / "no"), rate=50)          # the s = 100 files are coarser than 50
    assert e.value.code == sp.ERR_ARG and os.path.basename(M.paths[1]) in str(e.value)
    with pytest.raises(sp.SpspError) as e:
        ctx.compare_files(M.paths[:4] + mixed63.paths[:1], str(tmp_path / "no"), rate="auto")
    assert e.value.code == sp.ERR_FORMAT and os.path.basename(mixed63.paths[0]) in str(e.value)
    # with "auto" the too-coarse file sets the rate instead: everything is brought down to 100 000
    ctx.compare_files(M.paths[:6] + [far], str(tmp_path / "yes"), rate="auto")
    assert not os.path.exists(str(tmp_path / "no") + SUF[0][1])


@pytest.mark.gpu
def test_compare_files_multi_at_a_common_rate(mixed31, mixed63, tmp_path):
    """the key-partitioned split (two contexts on device 0): every context brings its block of sketches down before it deals
    the keys into the exchange slots"""
    for M in (mixed31, mixed63):
        tag = str(tmp_path / ("m%d" % M.k))
        st = sp.compare_files_multi([0, 0], M.paths, tag, rate="auto")
        assert st["compare_calls"] == 1
        assert M.got(tag) == M.want(M.coarse)
        sp.compare_files_multi([0, 0, 0], M.paths, tag + "q", n_query=5, rate=100)
        assert M.got(tag + "q") == M.want(M.coarse, 5)
        sp.compare_files_multi([0, 0], M.paths, tag + "asis")
        assert M.got(tag + "asis") == M.want(M.mixed)


@pytest.mark.gpu
def test_compare_files_multi_at_a_common_rate_over_all_devices(mixed31, tmp_path):
    n = sp.device_count()
    if n < 2:
        pytest.skip("needs >= 2 GPUs (spsp_device_count() = %d)" % n)
    M = mixed31
    for tag, devs in (("all", list(range(n))), ("rev", [n - 1, 0])):
        sp.compare_files_multi(devs, M.paths, str(tmp_path / tag), rate="auto")
        assert M.got(str(tmp_path / tag)) == M.want(M.coarse), tag


@pytest.mark.gpu
def test_comparator_cli_common_rate(mixed31, tmp_path):
    M = mixed31
    (tmp_path / "fof.txt").write_text("\n".join(M.paths) + "\n")
    exe = os.path.join(ROOT, "bin", "comparator")

    def run(*args):
        r = subprocess.run([exe, "-f", "fof.txt"] + list(args), cwd=tmp_path, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.splitlines()

    for tag, arg in (("auto", "auto"), ("r100", "100")):
        out = run("-o", tag, "-s", arg)
        assert M.got(str(tmp_path / tag)) == M.want(M.coarse), tag
        assert out[-1] == "Sketches compared at sampling rate 100: 22 of 44 brought down to it", out[-3:]
        assert out[-2].startswith("Jaccard output lasted ")
    out = run("-o", "plain")
    assert M.got(str(tmp_path / "plain")) == M.want(M.mixed)
    assert out[-1].startswith("Jaccard output lasted ") and not any("sampling rate" in ln for ln in out)
    # two contexts (the key-partitioned split), query mode
    (tmp_path / "q.txt").write_text("\n".join(M.paths[:5]) + "\n")
    (tmp_path / "bank.txt").write_text("\n".join(M.paths[5:]) + "\n")
    r = subprocess.run([exe, "-f", "bank.txt", "-q", "q.txt", "-o", "two", "-s", "auto"], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, SPSP_DEVICES="0,0"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert M.got(str(tmp_path / "two")) == M.want(M.coarse, 5)
    r = subprocess.run([exe, "-f", "fof.txt", "-s", "fast"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "-s takes" in r.stdout
