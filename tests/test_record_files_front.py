"""What the record file drivers share (DESIGN "What the record file drivers share"): the front of the ten file entries
spsp_classify_files[_extract|_paired|_split|_windows] and spsp_taxonomy_files[_extract|_paired|_split|_windows] -- the same bad
input is refused with the same return code and text, in the same order of checks, behind the clearing of the entry's outputs, and
nothing is written; the modes only observe the rows; and the one combination no other test runs, a paired taxonomy split by depth.

3 references of 3 kbp sketched at rate 32 (a few super-k-mers' keys each), a lineage file of three leaves under one node, 4 records
(one of each reference and one of none) and their 4 mates.  The entries are called through sp.lib() with every output filled with
sevens beforehand.  The order, as the entries have it: the outputs are cleared (the _extract and _split entries refuse a NULL word
in front of that: their outputs keep the sevens); NULL arguments; the reference count; the pass's thresholds (classify: `top`
first); the mode's word; the windows' width; and behind the device is chosen the lineage file, the word's node against the tree,
the sketches, the records file(s), the mates' record counts, the width against k."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import supersampler_amd as sp
import test_classify as tc
import test_prevalence as tp
import test_taxonomy as tt

SEVENS = 0x0707070707070707
ERR_IO = -5
K, M, RATE = tc.K_FILE, tc.M_FILE, 32.0
NULL_ARG = "NULL argument"
N_REF_TEXT = "a classification index takes 1 .. 65535 references (n = %u)"
WIDTH_TEXT = "windows: the width must be k .. 2147483647 (width = %u)"
LINEAGES = [("Bacteria", "A"), ("Bacteria", "B"), ("Bacteria", "C")]                     # root 0 > Bacteria 1 > {A 2, B 3, C 4}
T = 5

C_FRONT = ["ctx", "paths", "n_ref", "records", "top", "min_keys", "num", "den", "precision", "prefix", "chatter", "rate"]
C_MATES = ["ctx", "paths", "n_ref", "records", "mates", "top", "min_keys", "num", "den", "precision", "prefix", "chatter", "rate"]
T_FRONT = ["ctx", "paths", "n_ref", "records", "lin", "min_keys", "num", "den", "precision", "prefix", "chatter", "rate"]
T_MATES = ["ctx", "paths", "n_ref", "records", "mates", "lin", "min_keys", "num", "den", "precision", "prefix", "chatter", "rate"]
C_ROWS, T_ROWS = ["o_rows", "o_hits", "o_n"], ["o_rows", "o_n"]
WIN_OUT = ["o_first", "o_n_rec", "o_seg", "o_n_seg", "o_mos"]
KEPT = ["o_kept", "o_bytes"]
# entry -> (the arguments in the entry's order, its mode, taxonomy?)
ENTRIES = {
    "spsp_classify_files": (C_FRONT + C_ROWS, "plain", False),
    "spsp_classify_files_extract": (C_FRONT + C_ROWS + ["what", "gz"] + KEPT, "extract", False),
    "spsp_classify_files_paired": (C_MATES + ["what", "gz"] + C_ROWS + KEPT, "paired", False),
    "spsp_classify_files_split": (C_MATES + ["what", "gz"] + C_ROWS + KEPT, "split", False),
    "spsp_classify_files_windows": (C_FRONT + ["window", "what"] + C_ROWS + WIN_OUT, "windows", False),
    "spsp_taxonomy_files": (T_FRONT + T_ROWS, "plain", True),
    "spsp_taxonomy_files_extract": (T_FRONT + T_ROWS + ["what", "gz"] + KEPT, "extract", True),
    "spsp_taxonomy_files_paired": (T_MATES + ["what", "gz"] + T_ROWS + KEPT, "paired", True),
    "spsp_taxonomy_files_split": (T_MATES + ["what", "gz"] + T_ROWS + KEPT, "split", True),
    "spsp_taxonomy_files_windows": (T_FRONT + ["window", "what"] + T_ROWS + WIN_OUT, "windows", True),
}
POINTERS = ("o_rows", "o_hits", "o_first", "o_seg", "o_mos")
GOOD_WORD = {("extract", False): "matched", ("extract", True): "classified", ("split", False): "best", ("split", True): "taxon",
             ("windows", False): "best", ("windows", True): "taxon", ("paired", False): None, ("paired", True): None, ("plain", False): None, ("plain", True): None}


def enc(x):
    return None if x is None else str(x).encode()


class Case:
    """the files of the module, and one call of an entry: outputs filled with sevens, arguments by name"""

    def __init__(self, ctx, root):
        self.ctx, self.root, self.L = ctx, root, sp.lib()
        rng = np.random.default_rng(23)
        self.refs = [tc.random_bases(rng, 3000) for _ in range(3)]
        payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", K, M, RATE)[0] for i, g in enumerate(self.refs)]
        assert all(0 < len(tp.key_set(p)) < 200 for p in payloads)
        self.sketches = tp.write_files(root, payloads)
        r = self.refs
        self.recs = [r[0][200:1400], r[1][1000:2200], r[2][0:1200], tc.random_bases(np.random.default_rng(5), 300)]
        self.mate_seqs = [r[0][1500:2700], r[1][100:900], r[2][1500:2900], tc.random_bases(np.random.default_rng(6), 300)]
        self.names = ["r%d" % i for i in range(4)]
        fasta = lambda seqs, n=4: b"".join(b">r%d\n" % i + q + b"\n" for i, q in enumerate(seqs[:n]))
        self.f = lambda name: str(root / name)
        (root / "recs.fa").write_bytes(fasta(self.recs))
        (root / "mates.fa").write_bytes(fasta(self.mate_seqs))
        (root / "three.fa").write_bytes(fasta(self.mate_seqs, 3))
        self.tree = tt.Tree(LINEAGES)
        assert len(self.tree.parent) == T
        (root / "lin.txt").write_text(self.tree.text)
        self.n_prefix = 0

    def prefix(self):
        self.n_prefix += 1
        return "out%d" % self.n_prefix

    def written(self, prefix):
        return sorted(f for f in os.listdir(str(self.root)) if f.startswith(prefix + "_"))

    def call(self, entry, **over):
        """-> rc; self.out: the outputs by name, self.tag: the prefix's last part"""
        fields, mode, taxonomy = ENTRIES[entry]
        self.tag = self.prefix()
        a = {"ctx": self.ctx._h, "paths": self.sketches, "n_ref": 3, "records": self.f("recs.fa"), "mates": self.f("mates.fa") if mode == "paired" else None,
             "lin": self.f("lin.txt"), "top": 2, "min_keys": 1, "num": 0, "den": 1, "precision": 6, "prefix": self.f(self.tag), "chatter": 0, "rate": 0.0,
             "what": GOOD_WORD[(mode, taxonomy)], "gz": 0, "window": 400}
        a.update(over)
        arr, self._alive = sp._paths_array(a["paths"]) if a["paths"] is not None else (None, None)
        self.out = {f: (C.c_void_p(SEVENS) if f in POINTERS else C.c_uint64(SEVENS)) for f in fields if f.startswith("o_")}
        self.top = a["top"]
        args = []
        for f in fields:
            if f.startswith("o_"):
                args.append(None if over.get(f, 1) is None else C.byref(self.out[f]))
            elif f == "paths":
                args.append(arr)
            elif f in ("records", "mates", "lin", "prefix", "what"):
                args.append(enc(a[f]))
            else:
                args.append(a[f])
        return getattr(self.L, entry)(*args)

    def error(self):
        return self.L.spsp_last_error().decode()

    def values(self):
        return {f: (v.value or 0) for f, v in self.out.items()}

    def refuses(self, entry, code, text, untouched=False, **over):
        rc = self.call(entry, **over)
        assert (rc, self.error()) == (code, text), (entry, over)
        assert set(self.values().values()) == {SEVENS if untouched else 0}, (entry, over, self.values())
        assert self.written(self.tag) == [], (entry, over)

    def rows(self, entry, **over):
        """a call that succeeds -> (the rows' bytes, the hits' bytes or None, the outputs' values); the arrays are freed"""
        rc = self.call(entry, **over)
        assert rc == 0, (entry, over, self.error())
        v = self.values()
        taxonomy = ENTRIES[entry][2]
        size = (sp.TAXONOMY_RECORD_DTYPE if taxonomy else sp.CLASSIFY_RECORD_DTYPE).itemsize
        rows = C.string_at(v["o_rows"], v["o_n"] * size)
        hits = None if taxonomy else C.string_at(v["o_hits"], v["o_n"] * self.top * sp.CLASSIFY_HIT_DTYPE.itemsize)
        for f in POINTERS:
            if f in v:
                assert v[f] not in (0, SEVENS)
                self.L.spsp_free(C.c_void_p(v[f]))
        return rows, hits, v


def test_host_functions_under_the_sanitizers():
    """tests/tools/record_files_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs
    the drivers' host half -- the records' names, the batches' bounds, the file writer, the handing out of several row
    arrays (CPU only: nothing is preloaded, no device is opened)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([os.path.join(root, "tests", "tools", "record_files_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "record_files_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    ctx = sp.Context(0)
    yield Case(ctx, tmp_path_factory.mktemp("front"))
    ctx.close()


def word_refusals(mode, taxonomy):
    """the mode's word check, in front of any file: (word, text)"""
    if mode in ("extract", "paired"):
        mine = "with a taxonomy: classified, unclassified, taxon=<t>, clade=<t>" if taxonomy else "matched, unmatched, best=<j>, listed=<j>"
        other = ("extract: 'matched' asks classify's rows, these are a taxonomy's (classified, unclassified, taxon=<t>, clade=<t>)" if taxonomy else
                 "extract: 'classified' asks a taxonomy's rows, these are classify's (matched, unmatched, best=<j>, listed=<j>)")
        out = [("everything", "extract: 'everything' names no records (%s)" % mine), ("matched" if taxonomy else "classified", other)]
        return out if taxonomy else out + [("best=3", "extract: 'best=3': the index has 3 reference(s)")]
    if mode in ("split", "windows"):
        mine = "with a taxonomy: taxon, depth=<d>" if taxonomy else "best"
        out = [("everything", "split: 'everything' names no bins (%s)" % mine),
               ("depth=0", "split: 'depth=0': the depth must be 1 .. 32" if taxonomy else "split: 'depth=0' asks a taxonomy's rows, these are classify's (best)")]
        return [(w, t.replace("split: ", "windows: ", 1) if mode == "windows" else t) for w, t in out]
    return []


@pytest.mark.gpu
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_every_entry_refuses_the_same_bad_input_the_same_way_in_the_same_order(case, entry):
    fields, mode, taxonomy = ENTRIES[entry]
    name = "taxonomy" if taxonomy else "classification"
    # one list per check, in the entries' order: (arguments, code, text)
    nulls = ["ctx", "paths", "records", "prefix"] + (["lin"] if taxonomy else []) + (["mates"] if mode == "paired" else []) + (["what"] if mode == "windows" else [])
    stages = [[({f: None}, sp.ERR_ARG, NULL_ARG) for f in nulls],
              [({"n_ref": n}, sp.ERR_ARG, N_REF_TEXT % n) for n in (0, 65536)]]
    if not taxonomy:
        stages.append([({"top": t}, sp.ERR_ARG, "classification lists 1 .. 64 matches per record (top = %u)" % t) for t in (0, 65)])
    stages.append([({"min_keys": 0}, sp.ERR_ARG, "%s: min_keys is 1 at the least" % name),
                   ({"num": 2, "den": 1}, sp.ERR_ARG, "%s threshold 2 / 1: needs 0 <= num <= den, 1 <= den <= 1000000" % name),
                   ({"num": 0, "den": 0}, sp.ERR_ARG, "%s threshold 0 / 0: needs 0 <= num <= den, 1 <= den <= 1000000" % name)])
    if word_refusals(mode, taxonomy):
        stages.append([({"what": w}, sp.ERR_ARG, text) for w, text in word_refusals(mode, taxonomy)])
    if mode == "windows":
        stages.append([({"window": w}, sp.ERR_ARG, WIDTH_TEXT % w) for w in (0, 0x80000000)])
    # what would fail behind the front, had the front let it through: nothing of it is touched
    late = {"paths": ["no such sketch.gz"] * 3, "records": case.f("none.fa"), "lin": case.f("none.txt")}
    if mode in ("extract", "split"):                       # the quirk: a NULL word in front of the clearing, and of every other check
        case.refuses(entry, sp.ERR_ARG, NULL_ARG, untouched=True, what=None)
        case.refuses(entry, sp.ERR_ARG, NULL_ARG, untouched=True, what=None, ctx=None, n_ref=0)
    for stage in stages:
        for over, code, text in stage:
            case.refuses(entry, code, text, **dict(late, **over))
    for s in range(len(stages) - 1):                       # two bad things: the earlier check speaks
        first, code, text = stages[s][0]
        for later in stages[s + 1:]:
            case.refuses(entry, code, text, **dict(late, **dict(later[0][0], **first)))
    if not taxonomy:
        case.refuses(entry, sp.ERR_ARG, stages[2][0][2], **dict(late, top=0, min_keys=0))   # `top` in front of the threshold
    # outputs the caller does not want are no NULL argument: the front's refusals are the same without them
    no_out = {f: None for f in fields if f.startswith("o_")}
    rc = case.call(entry, **dict(late, n_ref=0, **no_out))
    assert (rc, case.error()) == (sp.ERR_ARG, N_REF_TEXT % 0)

    # the late refusals, in their order: each behind a front that passed
    if taxonomy:
        case.refuses(entry, ERR_IO, "cannot open '%s'" % late["lin"], **late)              # the lineage file: before any sketch is read
        if mode in ("extract", "paired"):                  # the word's node against the tree: likewise
            case.refuses(entry, sp.ERR_ARG, "extract: 'taxon=%u': the tree has %u node(s)" % (T, T), what="taxon=%u" % T, paths=late["paths"], records=late["records"])
            case.refuses(entry, sp.ERR_ARG, "extract: 'clade=%u': the tree has %u node(s)" % (T, T), what="clade=%u" % T, paths=late["paths"], records=late["records"])
    case.refuses(entry, ERR_IO, "cannot open '%s'" % late["paths"][0], paths=late["paths"], records=late["records"])   # the sketches in front of the records
    case.refuses(entry, ERR_IO, "cannot open '%s'" % late["records"], records=late["records"])
    if mode in ("paired", "split"):
        case.refuses(entry, ERR_IO, "cannot open '%s'" % case.f("none2.fa"), mates=case.f("none2.fa"))
        case.refuses(entry, sp.ERR_FORMAT, "paired files must hold as many records: '%s' has 4, '%s' has 3" % (case.f("recs.fa"), case.f("three.fa")),
                     mates=case.f("three.fa"))
    if mode == "windows":
        case.refuses(entry, sp.ERR_ARG, "windows: the width must be k .. 2147483647 (k = %u, width = %u)" % (K, K - 1), window=K - 1)
    rows, _, v = case.rows(entry)                          # the context after all of that
    assert v["o_n"] == (4 if mode != "windows" else v["o_n"]) and len(case.written(case.tag)) >= 2


@pytest.mark.gpu
def test_the_modes_agree_on_the_rows(case):
    """extract and split only observe the rows: the plain, the extract and the split entry return the same arrays, and with a
    mates file the paired and the split entry do"""
    for taxonomy, pre in ((False, "spsp_classify_files"), (True, "spsp_taxonomy_files")):
        plain = case.rows(pre)
        assert plain[2]["o_n"] == 4
        rows = np.frombuffer(plain[0], dtype=sp.TAXONOMY_RECORD_DTYPE if taxonomy else sp.CLASSIFY_RECORD_DTYPE)
        assert rows["length"].tolist() == [len(q) for q in case.recs] and (rows["hit_keys"][:3] > 0).all() and rows["hit_keys"][3] == 0
        if taxonomy:
            assert rows["node"].tolist() == [2, 3, 4, tt.NONE]
        else:
            hits = np.frombuffer(plain[1], dtype=sp.CLASSIFY_HIT_DTYPE).reshape(4, 2)
            assert rows["listed"].tolist() == [1, 1, 1, 0] and hits["reference"][:3, 0].tolist() == [0, 1, 2]
        extract, split = case.rows(pre + "_extract"), case.rows(pre + "_split")
        assert extract[:2] == plain[:2] and split[:2] == plain[:2]
        assert extract[2]["o_kept"] == 3 and split[2]["o_kept"] == 4                       # three records with a call; four bins with records
        assert split[2]["o_bytes"] == os.path.getsize(case.f("recs.fa"))
        paired = case.rows(pre + "_paired")
        pair_split = case.rows(pre + "_split", mates=case.f("mates.fa"))
        assert paired[:2] == pair_split[:2] and paired[0] != plain[0]
        assert paired[2]["o_kept"] == 0 and paired[2]["o_bytes"] == 0                      # no word: nothing is extracted
        assert pair_split[2]["o_bytes"] == os.path.getsize(case.f("recs.fa")) + os.path.getsize(case.f("mates.fa"))
        prows = np.frombuffer(paired[0], dtype=rows.dtype)
        assert prows["length"].tolist() == [len(a) + len(b) for a, b in zip(case.recs, case.mate_seqs)] and (prows["keys"] >= rows["keys"]).all()


def names_of(fasta):
    return [line[1:].split()[0] for line in fasta.decode().splitlines() if line.startswith(">")]


@pytest.mark.gpu
def test_a_paired_taxonomy_split_by_depth(case):
    """spsp_taxonomy_files_split with a mates file and depth=1: a pair called below Bacteria goes to Bacteria's two files, a pair
    without a call to the unclassified ones; the two files of a bin hold the same pairs, and the manifest lists both"""
    rows, _, v = case.rows("spsp_taxonomy_files_split", mates=case.f("mates.fa"), what="depth=1")
    tag = case.tag
    records = np.frombuffer(rows, dtype=sp.TAXONOMY_RECORD_DTYPE)
    lin = sp.taxonomy_lineages(case.tree.text, 3)
    bins, n_bins = sp.split_bins_taxonomy("depth=1", records, lin["parent"], lin["depth"])
    assert records["node"].tolist() == [2, 3, 4, tt.NONE] and (bins.tolist(), n_bins) == ([1, 1, 1, T], T + 1)
    assert v["o_kept"] == 2 and v["o_n"] == 4
    labels = {1: "1", T: "unclassified"}
    want_files = ["%s_split_%s_%d.fa" % (tag, label, i) for label in labels.values() for i in (1, 2)]
    assert case.written(tag) == sorted(want_files + [tag + "_split.csv.gz", tag + "_taxonomy.csv.gz", tag + "_taxonomy_report.csv.gz"])
    total = 0
    manifest = ["bin,name,records,bytes_1,file_1,bytes_2,file_2"]
    for b, label in labels.items():
        one, two = (open(case.f("%s_split_%s_%d.fa" % (tag, label, i)), "rb").read() for i in (1, 2))
        want = [case.names[r] for r in np.nonzero(bins == b)[0]]
        assert names_of(one) == names_of(two) == want                                      # the same record numbers per bin, in record order
        assert one == b"".join(b">%s\n%s\n" % (n.encode(), case.recs[int(n[1:])]) for n in want)
        assert two == b"".join(b">%s\n%s\n" % (n.encode(), case.mate_seqs[int(n[1:])]) for n in want)
        total += len(one) + len(two)
        manifest.append("%s,%s,%d,%d,%s_split_%s_1.fa,%d,%s_split_%s_2.fa" % (label, "Bacteria" if b == 1 else "unclassified", len(want), len(one), tag, label,
                                                                             len(two), tag, label))
    assert v["o_bytes"] == total
    with gzip.open(case.f(tag + "_split.csv.gz"), "rb") as f:
        assert f.read().decode() == "\n".join(manifest) + "\n"
