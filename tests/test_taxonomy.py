"""Taxonomy: the records of a sequence file assigned to the lowest common ancestor of their keys (include/spsp.h:
spsp_taxonomy_lineages_host, spsp_taxonomy_check_host, spsp_taxonomy_plan_host, spsp_taxonomy_index_device, spsp_taxonomy_device,
spsp_taxonomy_csv_host, spsp_taxonomy_report_csv_host, spsp_taxonomy_files; bin/comparator -X <records> -H <lineages>).

The rule, on sets of the comparator's keys and on nodes that are tuples of names (the root is the empty tuple):

    anc(a, b) = a is a prefix of b          lca(S) = the longest common prefix of S
    node(x)   = lca of the nodes of the references that hold x
    w(t)      = the record's keys found in the index with node(x) = t
    path(t)   = the sum of w over the prefixes of t          clade(t) = the sum of w over the nodes t is a prefix of
    W = the t with w(t) > 0 of the largest path; start = lca(W)
    the call  = the first node from start towards the root with clade >= min_keys and clade * den >= num * |Q_r|

Every expected value below comes from `model`: prefixes of tuples and sums over Python dicts.  It knows nothing of preorder numbers,
of subtree ranges or of "the lca of a set is the lca of its extremes"; its nodes are mapped to numbers only through
taxonomy_lineages (class Tree).  No tolerance anywhere.

Where the kernels cut, and the shapes that sit on the cuts (taxonomy_plan names the numbers): a record is tallied by one wave while
it has at most small_hits hit keys, by a workgroup with a counter per node beyond; those counters sit in LDS up to lds_nodes nodes
and in device memory above; when the taxonomy is attached a list of more than list_cut holders is folded by a whole wave."""
import gzip
import os
import random
import re
import subprocess
from collections import Counter, defaultdict

import numpy as np
import pytest

import supersampler_amd as sp
import test_classify as tc
import test_prevalence as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "bin", "comparator")
HEADER = "record,name,length,keys,hit_keys,taxon,depth,lineage,score,clade,direct,f_clade,winners\n"
REPORT_HEADER = "taxon,depth,name,lineage,references,records_clade,records_direct,bases_clade,bases_direct\n"
NONE = 0xffffffff


# -------------------------------------------------------------------------------------------------- the model

def lca(nodes):
    nodes = list(nodes)
    out = nodes[0]
    for t in nodes[1:]:
        n = 0
        while n < min(len(out), len(t)) and out[n] == t[n]:
            n += 1
        out = out[:n]
    return out


def key_nodes(lineages, refs):
    """node(x) of every key some reference holds"""
    held = defaultdict(list)
    for line, K in zip(lineages, refs):
        for x in set(K):
            held[x].append(tuple(line))
    return {x: lca(ts) for x, ts in held.items()}


def model(lineages, refs, recs, min_keys=1, num=0, den=1, node_of=None):
    """-> per record (keys, hit_keys, node, start, score, clade, direct, winners); node and start are tuples, or None"""
    node_of = key_nodes(lineages, refs) if node_of is None else node_of
    out = []
    for q in recs:
        q = set(q)
        w = Counter(node_of[x] for x in q if x in node_of)
        if not w:
            out.append((len(q), 0, None, None, 0, 0, 0, 0))
            continue
        path = {t: sum(w.get(t[:i], 0) for i in range(len(t) + 1)) for t in w}
        clade = lambda t: sum(c for d, c in w.items() if d[:len(t)] == t)
        best = max(path.values())
        W = [t for t in w if path[t] == best]
        start = lca(W)
        node, t = None, start
        while True:
            c = clade(t)
            if c >= min_keys and c * den >= num * len(q):
                node = t
                break
            if t == ():
                break
            t = t[:-1]
        out.append((len(q), sum(w.values()), node, start, best, clade(node) if node is not None else 0, w.get(node, 0) if node is not None else 0, len(W)))
    return out


class Tree:
    """the lineages as the library numbers them: paths[t] = the tuple of node t, num = its inverse"""

    def __init__(self, lineages):
        self.lineages = [tuple(x) for x in lineages]
        self.text = "".join(";".join(x) + "\n" for x in self.lineages)
        self.t = sp.taxonomy_lineages(self.text, len(self.lineages))
        self.parent, self.names, self.ref_node = self.t["parent"], self.t["names"], self.t["ref_node"]
        self.paths = [()]
        for t in range(1, len(self.parent)):
            self.paths.append(self.paths[int(self.parent[t])] + (self.names[t],))
        self.num = {p: t for t, p in enumerate(self.paths)}
        assert len(self.num) == len(self.paths) and [self.num[x] for x in self.lineages] == self.ref_node.tolist()

    def numbered(self, rows):
        n = lambda t: NONE if t is None else self.num[t]
        return [(a, b, n(node), n(start), c, d, e, f) for a, b, node, start, c, d, e, f in rows]


def as_arrays(rows, lengths=None):
    records = np.zeros(len(rows), dtype=sp.TAXONOMY_RECORD_DTYPE)
    for r, (keys, hit, node, start, score, clade, direct, winners) in enumerate(rows):
        records[r] = (lengths[r] if lengths else 0, keys, hit, node, start, score, clade, direct, winners)
    return records


def as_rows(records):
    return [tuple(int(rec[f]) for f in sp.TAXONOMY_RECORD_DTYPE.names[1:]) for rec in records]


def py_csv(rows, names, lengths, tree, precision=6):
    text = HEADER
    for r, ((keys, hit, node, start, score, clade, direct, winners), name, length) in enumerate(zip(rows, names, lengths)):
        text += "%d,%s,%d,%d,%d," % (r, name, length, keys, hit)
        if node == NONE:
            text += ",,,%d,%d,%d,0,%d\n" % (score, clade, direct, winners)
        else:
            path = tree.paths[node]
            text += "%d,%d,%s,%d,%d,%d,%s,%d\n" % (node, len(path), ";".join(path), score, clade, direct, "%.*g" % (precision, clade / keys) if keys else "0", winners)
    return text.encode()


def py_report_csv(rows, lengths, tree):
    T = len(tree.paths)
    direct, bases = [0] * T, [0] * T
    none = none_bases = 0
    for (_, _, node, *_), length in zip(rows, lengths):
        if node == NONE:
            none, none_bases = none + 1, none_bases + length
        else:
            direct[node] += 1; bases[node] += length
    refs = Counter(tree.ref_node.tolist())
    text = REPORT_HEADER
    for t, path in enumerate(tree.paths):
        under = [d for d, p in enumerate(tree.paths) if p[:len(path)] == path]
        text += "%d,%d,%s,%s,%d,%d,%d,%d,%d\n" % (t, len(path), tree.names[t], ";".join(path), refs.get(t, 0), sum(direct[d] for d in under), direct[t],
                                                  sum(bases[d] for d in under), bases[t])
    return (text + ",,unclassified,,0,%d,%d,%d,%d\n" % (none, none, none_bases, none_bases)).encode()


# ------------------------------------------------------------------------------------------------ not GPU

B, E, EC, EA, S, SE, Z = ("B",), ("B", "E"), ("B", "E", "Ec"), ("B", "E", "Ea"), ("B", "S"), ("B", "S", "Se"), ("Z",)
HAND = [(), B, E, EC, EA, S, SE]                             # one reference at every node of root > B > E > {Ec, Ea}, B > S > Se


def K(*xs):
    return [(x, 0, x) for x in xs]


def hand_case():
    """the references (one per node, each with keys of its own) and the record of the issue: w = Ec 3, Ea 3, E 2, B 1, Se 4, 3 absent"""
    refs = [K(*range(100 * j, 100 * j + 20)) for j in range(len(HAND))]
    rec = refs[3][:3] + refs[4][:3] + refs[2][:2] + refs[1][:1] + refs[6][:4] + K(9001, 9002, 9003)
    return refs, rec


def test_model_on_the_hand_sized_case():
    refs, rec = hand_case()
    assert len(rec) == 16
    assert model(HAND, refs, [rec], 1, 1, 2) == [(16, 13, E, E, 6, 8, 2, 2)]              # 8 * 2 >= 16 passes at equality
    assert model(HAND, refs, [rec], 1, 3, 5) == [(16, 13, B, E, 6, 13, 1, 2)]             # 40 < 48; B: 65 >= 48
    assert model(HAND, refs, [rec], 1, 1, 1) == [(16, 13, None, E, 6, 0, 0, 2)]           # nothing passes: score and winners still describe W
    node_of = key_nodes(HAND, refs)
    w = Counter(node_of[x] for x in rec if x in node_of)
    assert w == {EC: 3, EA: 3, E: 2, B: 1, SE: 4}
    assert model(HAND, refs, [[], K(9001)]) == [(0, 0, None, None, 0, 0, 0, 0), (1, 0, None, None, 0, 0, 0, 0)]
    # a key two references hold speaks for their lca
    shared = [refs[3] + K(7000, 7001), refs[4] + K(7000), refs[6] + K(7001)]
    assert key_nodes([EC, EA, SE], shared)[(7000, 0, 7000)] == E and key_nodes([EC, EA, SE], shared)[(7001, 0, 7001)] == B


def test_the_parser_numbers_nodes_in_preorder_by_first_appearance():
    text = "B;S;Se\nB;E;Ec\n\nB;E\n B ; E ; Ea \nZ;E\r\nB;S\n"
    t = sp.taxonomy_lineages(text, 7)
    # children in order of first appearance: B's are S then E; the same name E under Z is another node
    assert t["names"] == ["root", "B", "S", "Se", "E", "Ec", "Ea", "Z", "E"]
    assert t["parent"].tolist() == [0, 0, 1, 2, 1, 4, 4, 0, 7] and t["depth"].tolist() == [0, 1, 2, 3, 2, 3, 3, 1, 2]
    assert t["size"].tolist() == [9, 6, 2, 1, 3, 1, 1, 2, 1]
    assert t["ref_node"].tolist() == [3, 5, 0, 4, 6, 8, 2]                              # an empty line: the root; an inner node; blanks trimmed
    assert sp.taxonomy_lineages("\n\n", 2)["parent"].tolist() == [0] and sp.taxonomy_lineages("a", 1)["names"] == ["root", "a"]
    deep = ";".join("n%d" % i for i in range(32))
    assert sp.taxonomy_lineages(deep + "\n", 1)["depth"].tolist() == list(range(33))
    for text, n, line in ((deep + ";n32\n", 1, "line 1"), ("a\nb,c\n", 2, "line 2"), ('a\nb\n"c"\n', 3, "line 3"), ("a;;b\n", 1, "line 1"), ("a;\n", 1, "line 1"),
                          (";a\n", 1, "line 1"), ("a\n \n;\n", 3, "line 3"), ("a\nb\n", 3, "line 3"), ("a\nb\nc\n", 2, "line 3"), ("", 1, "line 1")):
        with pytest.raises(sp.SpspError) as e:
            sp.taxonomy_lineages(text, n)
        assert e.value.code == sp.ERR_FORMAT and line in str(e.value), (text, str(e.value))
    for n in (0, 65536):
        with pytest.raises(sp.SpspError) as e:
            sp.taxonomy_lineages("a\n", n)
        assert e.value.code == sp.ERR_ARG


def test_taxonomy_check_on_the_parsers_arrays_and_on_broken_ones():
    tree = Tree(HAND + [Z])
    sp.taxonomy_check(tree.parent, tree.ref_node)
    sp.taxonomy_check([0], [0, 0, 0])
    chain = list(range(-1, 32)); chain[0] = 0
    sp.taxonomy_check(chain, [32])                                                       # depth 32
    bad = [([1, 0], [0]),                                                                # the root is not its own parent
           ([0, 1], [0]),                                                                # parent[t] >= t
           ([0, 0, 3, 1], [0]),                                                          # a parent behind its child
           (chain + [32], [0]),                                                          # depth 33
           ([0, 0, 1], [3]),                                                             # ref_node >= T
           ([0, 0, 0, 1], [0]),                                                          # parent[t] < t holds, but node 3's parent is no ancestor of node 2
           ([0, 0, 1, 0, 2], [0]),                                                       # likewise, deeper
           ([], [0]), ([0], [])]
    for parent, ref_node in bad:
        with pytest.raises(sp.SpspError) as e:
            sp.taxonomy_check(parent, ref_node)
        assert e.value.code == sp.ERR_ARG, (parent, ref_node)
    with pytest.raises(sp.SpspError) as e:
        sp.taxonomy_check([0, 0, 0, 1], [0])
    assert "preorder" in str(e.value) and "node 3" in str(e.value)


def internal_constants():
    text = open(os.path.join(ROOT, "supersampler_amd", "csrc", "spsp_internal.h")).read()

    def value(name):
        expr = re.search(r"constexpr uint32_t %s = ([^;,]+)[;,]" % name, text).group(1)
        expr = re.sub(r"k[A-Z][A-Za-z]+", lambda m: str(value(m.group(0))), expr)
        return eval(expr.replace("/", "//"))
    return {"small_hits": value("kTxSmallHits"), "lds_nodes": value("kTxLdsNodes"), "list_cut": value("kTxListCut")}, value("kTxLargeFixedLds"), value("kAcLdsBytes")


def test_taxonomy_plan_is_the_constants_of_the_kernels():
    want, fixed, lds = internal_constants()
    assert want == {"small_hits": 1024, "lds_nodes": 38912, "list_cut": sp.classify_plan(1)["list_cut"]}
    for T in (1, 38912, 38913, 1 << 20):
        plan = sp.taxonomy_plan(T)
        assert {f: plan[f] for f in want} == want and plan["counters_in_lds"] == (T <= want["lds_nodes"])
    assert 4 * want["lds_nodes"] + fixed <= lds == 160 * 1024 and 4 * want["small_hits"] == 4096
    for T in (0, (1 << 20) + 1):
        with pytest.raises(sp.SpspError) as e:
            sp.taxonomy_plan(T)
        assert e.value.code == sp.ERR_ARG


# rows over the tree of HAND + [Z]: node numbers root 0, B 1, E 2, Ec 3, Ea 4, S 5, Se 6, Z 7
ROWS = [(16, 13, 2, 2, 6, 8, 2, 2), (0, 0, NONE, NONE, 0, 0, 0, 0), (16, 13, NONE, 2, 6, 0, 0, 2), (9, 9, 0, 0, 3, 9, 0, 3), (7, 7, 6, 6, 7, 7, 7, 1),
        (5, 4, 1, 3, 3, 4, 1, 1)]
NAMES = ["contig_1", "r/2", "", "read.4", "x", "y"]
LENGTHS = [5000, 12, 150, 40, (1 << 40) + 7, 31]


def test_both_csv_writers_equal_the_python_writers():
    tree = Tree(HAND + [Z, EC])
    assert [tree.num[x] for x in (B, E, EC, EA, S, SE, Z)] == [1, 2, 3, 4, 5, 6, 7]
    records = as_arrays(ROWS, LENGTHS)
    for precision in (6, 3):
        assert sp.taxonomy_csv(records, NAMES, tree.parent, tree.names, precision) == py_csv(ROWS, NAMES, LENGTHS, tree, precision)
    lines = sp.taxonomy_csv(records, NAMES, tree.parent, tree.names).decode().splitlines()
    assert lines[1] == "0,contig_1,5000,16,13,2,2,B;E,6,8,2,0.5,2" and lines[2] == "1,r/2,12,0,0,,,,0,0,0,0,0" and lines[3] == "2,,150,16,13,,,,6,0,0,0,2"
    assert lines[4] == "3,read.4,40,9,9,0,0,,3,9,0,1,3" and len(lines) == 7
    report = sp.taxonomy_report_csv(records, tree.parent, tree.names, tree.ref_node)
    assert report == py_report_csv(ROWS, LENGTHS, tree)
    assert report.decode().splitlines()[1:] == [
        "0,0,root,,1,4,1,%d,40" % (5000 + 40 + LENGTHS[4] + 31), "1,1,B,B,1,3,1,%d,31" % (5000 + LENGTHS[4] + 31), "2,2,E,B;E,1,1,1,5000,5000", "3,3,Ec,B;E;Ec,2,0,0,0,0",
        "4,3,Ea,B;E;Ea,1,0,0,0,0", "5,2,S,B;S,1,1,0,%d,0" % LENGTHS[4], "6,3,Se,B;S;Se,1,1,1,%d,%d" % (LENGTHS[4], LENGTHS[4]), "7,1,Z,Z,1,0,0,0,0",
        ",,unclassified,,0,2,2,162,162"]
    none = as_arrays([])
    assert sp.taxonomy_csv(none, [], tree.parent, tree.names) == HEADER.encode()
    assert sp.taxonomy_report_csv(none, tree.parent, tree.names, tree.ref_node) == py_report_csv([], [], tree)
    assert sp.taxonomy_csv(as_arrays([(3, 3, 0, 0, 3, 3, 3, 1)], [9]), ["a"], [0], ["root"]) == HEADER.encode() + b"0,a,9,3,3,0,0,,3,3,3,1,1\n"   # T = 1


def test_both_csv_writers_refuse_rows_that_contradict_themselves():
    tree = Tree(HAND + [Z])
    bad = [(6, 7, 2, 2, 3, 5, 1, 1),               # hit_keys > keys
           (9, 5, 2, 2, 3, 6, 1, 1),               # clade > hit_keys
           (9, 5, 2, 2, 3, 4, 5, 1),               # direct > clade
           (9, 5, 2, 2, 6, 4, 1, 1),               # score > hit_keys
           (9, 5, 8, 8, 3, 4, 1, 1),               # node >= T and not none
           (9, 5, 2, 5, 3, 4, 1, 1),               # node E is no ancestor of start S
           (9, 5, 3, 2, 3, 4, 1, 1),               # node Ec below start E
           (9, 5, 2, NONE, 3, 4, 1, 1),            # a call without a start
           (9, 5, 2, 2, 3, 4, 1, 0)]               # winners = 0 with hit keys
    for row in bad:
        records = as_arrays([ROWS[0], row], [1, 2])
        for call in (lambda: sp.taxonomy_csv(records, ["a", "b"], tree.parent, tree.names),
                     lambda: sp.taxonomy_report_csv(records, tree.parent, tree.names, tree.ref_node)):
            with pytest.raises(sp.SpspError) as e:
                call()
            assert e.value.code == sp.ERR_ARG and "record 1" in str(e.value), row
    records = as_arrays(ROWS[:1], [1])
    for call in (lambda: sp.taxonomy_csv(records, ["a"], [0, 0, 0, 1], ["r", "a", "b", "c"]),           # no preorder
                 lambda: sp.taxonomy_report_csv(records, tree.parent, tree.names, [8]),                 # a reference outside the tree
                 lambda: sp.taxonomy_report_csv(records, tree.parent, tree.names, [])):
        with pytest.raises(sp.SpspError) as e:
            call()
        assert e.value.code == sp.ERR_ARG


def test_the_command_line_refuses_before_it_opens_a_device(tmp_path):
    (tmp_path / "list.txt").write_text("no such sketch one.gz\nno such sketch two.gz\n")
    (tmp_path / "labels.txt").write_text("a\nb\n")
    (tmp_path / "lin.txt").write_text("a\nb\n")
    run = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=120)
    cases = [("-H", "lin.txt"), ("-H", "lin.txt", "-V", "2"), ("-X", "r.fa", "-H", "lin.txt", "-Y", "2"), ("-X", "r.fa", "-H", "lin.txt", "-Y", "1"),
             ("-H", "lin.txt", "-D", "r.fa")]
    cases += [("-X", "r.fa", "-H", "lin.txt", o, v) for o, v in (("-q", "list.txt"), ("-g", "3"), ("-c", "0.5"), ("-C", "0.5"), ("-N", "5"), ("-P", "0.9"), ("-r", "0.9"),
                                                                 ("-R", "0.9"), ("-l", "0.5"), ("-L", "0.5"), ("-S", "union"), ("-E", "union"), ("-J", "0.5"), ("-K", "0.5"),
                                                                 ("-A", "10"), ("-G", "labels.txt"), ("-D", "r.fa"), ("-V", "0"), ("-I", "1.5"))]
    for args in cases:
        r = run(*(args + ("-f", "list.txt", "-o", "bad")))
        assert r.returncode == 1 and len(r.stdout.splitlines()) == 1, (args, r.stdout, r.stderr)
        assert any(o in r.stdout for o in ("-H", "-X", "-V", "-I")), (args, r.stdout)
        assert not [f for f in os.listdir(tmp_path) if f.startswith("bad")]
    for args in cases[:5]:
        assert "-H" in run(*(args + ("-f", "list.txt", "-o", "bad"))).stdout, args
    assert "-H" in run().stdout                                                          # the help text has its line


def test_abi_has_the_taxonomy_calls():
    calls = ("spsp_taxonomy_lineages_host", "spsp_taxonomy_check_host", "spsp_taxonomy_plan_host", "spsp_taxonomy_index_device", "spsp_taxonomy_device",
             "spsp_taxonomy_stage_ms", "spsp_taxonomy_csv_host", "spsp_taxonomy_report_csv_host", "spsp_taxonomy_files")
    assert set(calls) <= set(sp.ABI_SYMBOLS)
    assert sp.TAXONOMY_RECORD_DTYPE.itemsize == 40
    assert sp.TAXONOMY_RECORD_DTYPE.names == ("length", "keys", "hit_keys", "node", "start", "score", "clade", "direct", "winners")
    assert [sp.TAXONOMY_RECORD_DTYPE.fields[f][1] for f in sp.TAXONOMY_RECORD_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28, 32, 36]
    for name in calls:
        assert hasattr(sp.lib(), name)


def test_host_functions_under_the_sanitizers():
    """tests/tools/taxonomy_asan: spsp_host.cpp built with -fsanitize=address,undefined into a program of its own, which runs the
    parser, the check, the plan and the two writers with their refusals (CPU only: nothing is preloaded, no device is opened)"""
    r = subprocess.run([os.path.join(ROOT, "tests", "tools", "taxonomy_asan", "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "taxonomy_asan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx():
    c = sp.Context(0)
    yield c
    c.close()


class Tax:
    """an index over the references (test_classify's Index) with the lineages attached; the tensors live as long as the object"""

    def __init__(self, ctx, k, refs, lineages, want_key_nodes=False, index=None):
        self.index = index or tc.Index(ctx, k, refs)
        self.tree = Tree(lineages)
        self.refs, self.k = refs, k
        self.d_key_nodes = ctx.taxonomy_index_device(self.tree.parent, self.tree.ref_node, want_key_nodes)
        self.node_of = key_nodes(self.tree.lineages, refs)

    def want(self, recs, min_keys=1, num=0, den=1):
        return self.tree.numbered(model(self.tree.lineages, self.refs, recs, min_keys, num, den, node_of=self.node_of))


def run(ctx, k, recs, min_keys=1, num=0, den=1, shuffle=0):
    """records -> rows as the model's, numbered; shuffle: a seed for the order of the keys inside every record (0: sorted)"""
    mn, lo, hi, off, order = tp.pack(recs, k)
    if shuffle:
        rng = np.random.default_rng(shuffle)
        perm = np.concatenate([int(a) + rng.permutation(int(z) - int(a)) for a, z in zip(off[:-1], off[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
        mn, lo, hi = mn[perm], lo[perm], (hi[perm] if hi is not None else None)
    d = tp.upload(mn, lo, hi)
    records = ctx.taxonomy_device(tp.ptr(d[0]), tp.ptr(d[1]), tp.ptr(d[2]), off, min_keys, num, den)
    del d
    assert not records["length"].any()
    return as_rows(records)


def check(ctx, tax, recs, rules=((1, 0, 1),), shuffle=0):
    for min_keys, num, den in rules:
        got, want = run(ctx, tax.k, recs, min_keys, num, den, shuffle), tax.want(recs, min_keys, num, den)
        assert got == want, (min_keys, num, den, [(r, a, b) for r, (a, b) in enumerate(zip(got, want)) if a != b][:3])
    return tax


def hand_refs(k, per_node=20, lineages=HAND):
    """one reference at every node, each with keys of its own: a key of reference j has node(x) = lineages[j]"""
    p = tp.pool(per_node * len(lineages), k)
    return [p[per_node * j:per_node * (j + 1)] for j in range(len(lineages))]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_hand_sized_case_and_records_without_keys_or_hits(ctx, k):
    refs = hand_refs(k)
    stranger = tp.pool(30, k, salt=700_000)
    rec = refs[3][:3] + refs[4][:3] + refs[2][:2] + refs[1][:1] + refs[6][:4] + stranger[:3]
    tax = Tax(ctx, k, refs, HAND)
    n = tax.tree.num
    assert run(ctx, k, [rec], 1, 1, 2) == [(16, 13, n[E], n[E], 6, 8, 2, 2)]
    assert run(ctx, k, [rec], 1, 3, 5) == [(16, 13, n[B], n[E], 6, 13, 1, 2)]
    assert run(ctx, k, [rec], 1, 1, 1) == [(16, 13, NONE, n[E], 6, 0, 0, 2)]
    check(ctx, tax, [rec, [], stranger[:5], refs[0][:3], [], stranger[5:], []], rules=((1, 0, 1), (1, 1, 2), (1, 3, 5), (1, 1, 1)), shuffle=3)
    check(ctx, tax, [[]])
    check(ctx, tax, [[], [], []])
    assert len(ctx.taxonomy_device(None, None, None, [0])) == 0                          # no record at all
    for args in ((0, 0, 1), (1, 2, 1), (1, 0, 0), (1, 0, 1_000_001)):
        with pytest.raises(sp.SpspError) as e:
            run(ctx, k, [rec], *args)
        assert e.value.code == sp.ERR_ARG
    with pytest.raises(sp.SpspError) as e:                                               # another k than the index's
        run(ctx, 94 - k, [tp.pool(5, 94 - k)])
    assert e.value.code == sp.ERR_ARG
    check(ctx, Tax(ctx, k, [[], []], [B, Z]), [refs[0][:3], []])                         # an index without a key


@pytest.mark.gpu
def test_calls_without_an_index_or_without_a_taxonomy_are_refused(ctx):
    k = 31
    refs = hand_refs(k)
    fresh = sp.Context(0)
    for call in (lambda: run(fresh, k, [refs[0][:3]]), lambda: fresh.taxonomy_index_device([0], [0])):      # never built
        with pytest.raises(sp.SpspError) as e:
            call()
        assert e.value.code == sp.ERR_ARG and "index" in str(e.value)
    fresh.close()
    index = tc.Index(ctx, k, refs)
    with pytest.raises(sp.SpspError) as e:                                               # an index, no taxonomy on it
        run(ctx, k, [refs[0][:3]])
    assert e.value.code == sp.ERR_ARG and "taxonomy" in str(e.value)
    # ... with the records zeroed
    mn, lo, hi, off, _ = tp.pack([refs[0][:3]], k)
    d = tp.upload(mn, lo, hi)
    records = np.full(1, 7, dtype=np.uint8).repeat(40).view(sp.TAXONOMY_RECORD_DTYPE)
    rc = sp.lib().spsp_taxonomy_device(ctx._h, tp.ptr(d[0]), tp.ptr(d[1]), None, np.ascontiguousarray(off, dtype=np.uint64).ctypes.data, 1, 1, 0, 1, records.ctypes.data)
    assert rc == sp.ERR_ARG and as_rows(records) == [(0,) * 8]
    tree = Tree(HAND)
    for parent, ref_node in ((tree.parent, tree.ref_node[:-1]), (tree.parent, list(tree.ref_node) + [0]), ([0, 0, 0, 1], [0] * 7), (tree.parent, [7] * 7)):
        with pytest.raises(sp.SpspError) as e:                                           # n_ref is not the index's; arrays the check refuses
            ctx.taxonomy_index_device(parent, ref_node)
        assert e.value.code == sp.ERR_ARG
    tax = Tax(ctx, k, refs, HAND, index=index)
    first = run(ctx, k, [refs[3][:5]])
    assert first == tax.want([refs[3][:5]])
    ctx.prevalence_device(k, tp.ptr(index.d[0]), tp.ptr(index.d[1]), None, index.off, len(refs), 1, 2)      # the index is replaced
    with pytest.raises(sp.SpspError) as e:
        run(ctx, k, [refs[3][:5]])
    assert e.value.code == sp.ERR_ARG and "index" in str(e.value)
    index = tc.Index(ctx, k, refs)                                                       # a new index does not inherit the taxonomy
    with pytest.raises(sp.SpspError) as e:
        run(ctx, k, [refs[3][:5]])
    assert e.value.code == sp.ERR_ARG and "taxonomy" in str(e.value)
    del d, index


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_key_nodes_for_lists_on_both_sides_of_the_cut(ctx, k):
    cut = sp.taxonomy_plan(1)["list_cut"]
    sizes = [1, 2, cut - 1, cut, cut + 1, 63, 64, 65, 66]
    R = 70
    p = tp.pool(len(sizes) * 3 + R, k)
    rng = random.Random(9)
    # reference j sits in one of five genera of two families, or at a family, or at the root
    spots = [("F%d" % (g // 3), "G%d" % g, "s%d" % j) for j, g in ((j, j % 5) for j in range(R))]
    spots[7], spots[33], spots[50] = ("F0",), (), ("F1", "G4")
    refs = [[p[len(sizes) * 3 + j]] for j in range(R)]
    for i, h in enumerate(sizes):                                                        # three keys per list length: the first h, a random h, the last h references
        for v, holders in enumerate((range(h), rng.sample(range(R), h), range(R - h, R))):
            for j in holders:
                refs[j].append(p[3 * i + v])
    tax = Tax(ctx, k, refs, spots, want_key_nodes=True)
    entries = [x for s in tax.index.refs for x in s]
    got = ctx.to_host(tax.d_key_nodes, len(entries), np.uint32).tolist()
    want = [tax.tree.num[tax.node_of[x]] for x in entries]
    assert got == want, [(i, a, b) for i, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    assert len({tax.node_of[p[3 * i]] for i in range(len(sizes))}) >= 3                  # leaves, genera, families and the root all occur
    check(ctx, tax, [[p[3 * i + v] for i in range(len(sizes))] for v in range(3)] + [p[:len(sizes) * 3]], rules=((1, 0, 1), (3, 1, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_a_key_all_65535_references_hold(ctx, k):
    R = 65535
    own = tp.pool(R + 3, k)
    # two subtrees under the root's child A, one reference at A itself; keys: own[R] everybody, own[R + 1] the references of A;x only
    spots = [("A", "x", "s%d" % (j % 300)) if j % 2 else ("A", "y", "s%d" % (j % 300)) for j in range(R)]
    spots[40000] = ("A",)
    refs = [[own[j], own[R]] + ([own[R + 1]] if j % 2 else []) for j in range(R)]
    tax = Tax(ctx, k, refs, spots, want_key_nodes=True)
    n = tax.tree.num
    assert tax.node_of[own[R]] == ("A",) and tax.node_of[own[R + 1]] == ("A", "x")
    sample = [0, 1, 2, 3, 40000 * 2, 40000 * 2 + 1, 2 * R - 2, 2 * R - 1] + list(range(1000, 1200))
    got = ctx.to_host(tax.d_key_nodes, int(tax.index.off[-1]), np.uint32)
    entries = [x for s in tax.index.refs for x in s]
    assert [int(got[i]) for i in sample] == [n[tax.node_of[entries[i]]] for i in sample]
    assert set(got[[i for i, x in enumerate(entries) if x == own[R]][:50]].tolist()) == {n[("A",)]}
    check(ctx, tax, [[own[R]], [own[R], own[R + 1], own[5]], [own[R + 2]], [own[40000], own[R]]], rules=((1, 0, 1), (2, 1, 1)))
    del tax
    # the same key with one reference outside A: its node is the root
    spots[1] = ("Q",)
    tax = Tax(ctx, k, refs, spots)
    assert tax.node_of[own[R]] == () and run(ctx, k, [[own[R], own[R + 1]]]) == tax.want([[own[R], own[R + 1]]])
    del tax


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_tree_shapes(ctx, k):
    p = tp.pool(2000, k)
    stranger = tp.pool(10, k, salt=800_000)
    # T = 1: every reference at the root
    refs = [p[:30], p[20:60], p[100:110]]
    tax = check(ctx, Tax(ctx, k, refs, [(), (), ()]), [p[:5], p[25:28] + stranger[:2], stranger, p[100:110]], rules=((1, 0, 1), (3, 0, 1), (1, 1, 1), (1, 3, 5)))
    assert len(tax.tree.paths) == 1 and run(ctx, k, [p[:5]]) == [(5, 5, 0, 0, 5, 5, 5, 1)]
    del tax
    # a star: 50 leaves under the root, keys shared by neighbours
    refs = [p[20 * j:20 * j + 25] for j in range(50)]
    recs = [p[20 * j + 3:20 * j + 30] for j in range(0, 50, 7)] + [p[:1000:9], p[5:25], p[20:25]]
    check(ctx, Tax(ctx, k, refs, [("leaf%d" % j,) for j in range(50)]), recs, rules=((1, 0, 1), (5, 1, 2), (1, 9, 10)), shuffle=2)
    # one chain of depth 32 with a reference at every level, the root included
    chain = [tuple("c%d" % i for i in range(d)) for d in range(33)]
    refs = [p[10 * d:10 * d + 10] + p[1000:1000 + d] for d in range(33)]                 # p[1000 + i] is held from level i + 1 down: its node is level i + 1
    tax = Tax(ctx, k, refs, chain)
    assert len(tax.tree.paths) == 33 and tax.node_of[p[1031]] == chain[32] and tax.node_of[p[1000]] == chain[1]
    recs = [p[320:330], p[0:3] + p[320:323], p[1000:1032], p[5:6] + p[105:107] + p[205:208], p[320:322] + p[0:5], [p[10 * d] for d in range(33)]]
    check(ctx, tax, recs, rules=((1, 0, 1), (4, 0, 1), (1, 1, 2), (1, 1, 1), (33, 1, 1)), shuffle=5)
    assert run(ctx, k, [[p[10 * d] for d in range(33)]]) == [(33, 33, 32, 32, 33, 1, 1, 1)] and run(ctx, k, recs[-1:], 2)[0][2] == 31
    del tax
    # references at inner nodes, with leaves under them
    check(ctx, Tax(ctx, k, hand_refs(k, 40, HAND + [Z, E, B]), HAND + [Z, E, B]), [p[0:40:3] + p[80:120:2] + p[160:170], p[120:160] + p[240:245], p[280:300] + p[40:45]],
          rules=((1, 0, 1), (10, 2, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_ties_between_winners(ctx, k):
    lines = HAND + [Z]
    refs = hand_refs(k, 20, lines)
    at = {t: refs[j] for j, t in enumerate(lines)}
    tax = Tax(ctx, k, refs, lines)
    n = tax.tree.num
    siblings = at[EC][:2] + at[EA][:2]
    depths = at[EC][:2] + at[S][:2] + at[B][:1]
    three = at[EC][:1] + at[SE][:1] + at[Z][:1]
    single = at[EC][:3] + at[EA][:2] + at[E][:1]
    above = at[EC][:2] + at[E][:2] + at[Z][:4]                                            # the winner Z is no leaf's ancestor; Ec's path is 4 as well
    check(ctx, tax, [siblings, depths, three, single, above], rules=((1, 0, 1), (1, 1, 2), (1, 1, 1), (3, 0, 1)), shuffle=4)
    got = run(ctx, k, [siblings, depths, three, single, above])
    assert [(r[2], r[3], r[4], r[7]) for r in got] == [(n[E], n[E], 2, 2), (n[B], n[B], 3, 2), (0, 0, 1, 3), (n[EC], n[EC], 4, 1), (0, 0, 4, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_the_confidence_climb_at_equality_and_one_short(ctx, k):
    refs = hand_refs(k)
    at = {t: refs[j] for j, t in enumerate(HAND)}
    stranger = tp.pool(3, k, salt=700_000)
    rec = at[EC][:3] + at[EA][:3] + at[E][:2] + at[B][:1] + at[SE][:4] + at[()][:1] + stranger    # 17 keys: clade E 8, B 13, root 14
    tax = Tax(ctx, k, refs, HAND)
    n = tax.tree.num
    rules = [(8, 0, 1), (9, 0, 1), (13, 0, 1), (14, 0, 1), (15, 0, 1), (1, 8, 17), (1, 9, 17), (1, 13, 17), (1, 14, 17), (1, 15, 17), (1, 1, 1), (1, 999_999, 1_000_000),
             (1, 0, 1_000_000), (1, 1_000_000, 1_000_000), (9, 8, 17), (14, 13, 17)]
    check(ctx, tax, [rec, rec[:14], at[SE][:4]], rules=rules)
    calls = [run(ctx, k, [rec], *rule)[0][2] for rule in rules[:11]]
    assert calls == [n[E], n[B], n[B], 0, NONE, n[E], n[B], n[B], 0, NONE, NONE]          # a climb that ends at the root and passes, and one that fails there
    assert run(ctx, k, [rec[:14]], 1, 1, 1) == [(14, 14, 0, n[E], 7, 14, 1, 2)]          # num = den: every key of the record under the call


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_records_whose_hit_keys_sit_on_the_routing_cut(ctx, k):
    H = sp.taxonomy_plan(8)["small_hits"]
    lines = HAND + [Z]
    refs = hand_refs(k, 400, lines)                                                      # 3 200 keys over 8 nodes
    flat = [x for j in (3, 4, 2, 6, 1, 7, 5, 0) for x in refs[j]]
    stranger = tp.pool(100, k, salt=600_000)
    tax = Tax(ctx, k, refs, lines)
    recs = [flat[:H - 1], flat[:H], flat[:H + 1], flat[:H - 1] + stranger, flat[:H] + stranger[:1], flat[:H + 1] + stranger, flat[100:100 + 2 * H], flat,
            flat[:64], flat[:65], flat[:63] + stranger[:1], flat[390:390 + 128]]          # records whose keys fill one wave, and two, exactly
    check(ctx, tax, recs, rules=((1, 0, 1), (1, 1, 2), (700, 3, 4)), shuffle=11)
    mixed = [recs[2], [], recs[0], stranger[:9], recs[6], recs[8], flat[7:8], recs[5]] * 3      # every form in one batch
    check(ctx, tax, mixed, rules=((1, 2, 3),))
    for n_rec in (63, 64, 65, 257):
        check(ctx, tax, [flat[(37 * r) % 3000:(37 * r) % 3000 + 1 + r % 70] + stranger[:r % 3] for r in range(n_rec)], rules=((2, 1, 4),), shuffle=n_rec)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_counters_in_lds_and_in_device_memory(ctx, extra):
    k = 31
    plan = sp.taxonomy_plan(1)
    T = plan["lds_nodes"] + extra
    n_chain, last = divmod(T - 1, 20)                                                    # private chains of 20 names, and one shorter chain
    spots = [tuple("r%d_%d" % (j, i) for i in range(20)) for j in range(n_chain)] + [tuple("last_%d" % i for i in range(last))]
    R = len(spots)
    own = tp.pool(2 * R + 40, k)
    # reference j: own[2 j + 1] is its own (node: its leaf), own[2 j] it shares with j + 1 (node: the root); the last 40 share 40 more
    refs = [[own[2 * j], own[2 * j + 1]] for j in range(R)]
    for j in range(R - 1):
        refs[j + 1].append(own[2 * j])
    for j in range(R - 40, R):
        refs[j] += own[2 * R:2 * R + 40]
    tax = Tax(ctx, k, refs, spots)
    assert len(tax.tree.paths) == T and sp.taxonomy_plan(T)["counters_in_lds"] == (extra == 0)
    big = own[2 * (R - 700):2 * R] + own[2 * R:2 * R + 40]                                # 1 440 hit keys: the workgroup form, the very last node among them
    assert len(big) > plan["small_hits"]
    check(ctx, tax, [big, own[:3], big[600:], own[2 * R:]], rules=((1, 0, 1), (1, 1, 1)))
    got = run(ctx, k, [big] * 3 + [big[1:]], 700, 1, 2)                                  # twice on one workgroup's counters: cleared between the records
    assert got == tax.want([big] * 3 + [big[1:]], 700, 1, 2) and got[0] == got[1] == got[2] and got[3][1] == len(big) - 1
    assert run(ctx, k, [own[2 * R - 1:2 * R]])[0][2] == T - 1                            # the last node of the tree
    del tax


@pytest.mark.gpu
@pytest.mark.parametrize("k", [31, 63])
def test_one_record_of_70000_keys_under_one_node(ctx, k):
    p = tp.pool(70_000, k)
    refs = [p[:10], p, p[69_990:]]
    tax = Tax(ctx, k, refs, [("A", "a"), ("A", "b"), ("C",)])
    n = tax.tree.num
    got = run(ctx, k, [p, p[:100]], shuffle=3)
    # 69 980 keys of the middle reference alone, 10 shared inside A (node A), 10 shared with C (node: the root)
    assert got[0] == (70_000, 70_000, n[("A", "b")], n[("A", "b")], 70_000, 69_980, 69_980, 1) and got == tax.want([p, p[:100]])
    assert run(ctx, k, [p], 69_990, 1, 1) == [(70_000, 70_000, 0, n[("A", "b")], 70_000, 70_000, 10, 1)]
    del tax
    tax = Tax(ctx, k, [p, tp.pool(5, k, salt=900_000)], [("A", "b"), ("C",)])
    n = tax.tree.num
    assert run(ctx, k, [p], 70_000, 1, 1, shuffle=5) == [(70_000, 70_000, n[("A", "b")], n[("A", "b")], 70_000, 70_000, 70_000, 1)]      # direct = 70 000 in one counter
    del tax


@pytest.mark.gpu
def test_two_batches_a_replaced_taxonomy_and_untouched_depth_counters(ctx):
    k = 31
    lines = HAND + [Z]
    refs = hand_refs(k, 60, lines)
    flat = [x for s in refs for x in s]
    index = tc.Index(ctx, k, refs)
    a, b = [flat[:50], flat[170:200], flat[55:65]], [flat[200:480], flat[100:130], []]
    # depth counters begun before the attach
    ctx.depth_begin()
    mn, lo, hi, off, _ = tp.pack(a + b, k)
    d = tp.upload(mn, lo, hi)
    ctx.depth_add(tp.ptr(d[0]), tp.ptr(d[1]), None, 0, int(off[-1]))
    rows, totals = ctx.depth_read()
    tax = Tax(ctx, k, refs, lines, index=index)
    first = run(ctx, k, a)
    assert first == tax.want(a) and run(ctx, k, b) == tax.want(b) and run(ctx, k, a) == first
    rows2, totals2 = ctx.depth_read()
    assert rows.tobytes() == rows2.tobytes() and totals.tobytes() == totals2.tobytes() and int(totals["hit_keys"]) == int(off[-1])
    ctx.timing_enable(True)                                                              # events between the launches: the same answer, four times
    ctx.taxonomy_stage_ms()
    assert run(ctx, k, a) == first
    ms = ctx.taxonomy_stage_ms()
    ctx.timing_enable(False)
    assert list(ms) == ["probe", "route", "wave_form", "workgroup_form"] and all(v > 0 for v in ms.values())
    assert run(ctx, k, a) == first and not any(ctx.taxonomy_stage_ms().values())
    # another taxonomy on the same index: every reference one level down in another order, the answers change with it
    other = [("new",) + t for t in lines[::-1]]
    tax2 = Tax(ctx, k, refs, other, index=index)
    second = run(ctx, k, a)
    assert second == tax2.want(a) and second != first
    records, _ = ctx.classify_device(tp.ptr(d[0]), tp.ptr(d[1]), None, off[:4], 1)       # classify on the index still answers
    assert [int(x) for x in records["keys"]] == [len(set(q)) for q in a]
    rows3, _ = ctx.depth_read()
    assert rows3.tobytes() == rows.tobytes()
    del d, index


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_a_seeded_random_sweep_against_the_model(ctx, seed):
    rng = random.Random(seed)
    k = 31 if seed % 2 else 63
    nodes = [()]
    while len(nodes) < 30:
        t = rng.choice(nodes)
        if len(t) < 6:
            t = t + ("n%d" % len(nodes),)
            if t not in nodes:
                nodes.append(t)
    spots = [rng.choice(nodes) for _ in range(40)]
    p = tp.pool(3000, k)
    family = {f: rng.sample(p, 150) for f in {t[:1] for t in spots}}                     # references of one top-level family share its core
    refs = [rng.sample(family[t[:1]], rng.randint(0, 120)) + rng.sample(p, rng.randint(0, 150)) for t in spots]
    recs = [rng.sample(p, rng.randint(0, 150)) + rng.sample(family[rng.choice(spots)[:1]], rng.randint(0, 60)) + tp.pool(rng.randint(0, 5), k, salt=10 ** 6 + 10 * r)
            for r in range(300)]
    tax = Tax(ctx, k, refs, spots, want_key_nodes=True)
    entries = [x for s in tax.index.refs for x in s]
    assert ctx.to_host(tax.d_key_nodes, len(entries), np.uint32).tolist() == [tax.tree.num[tax.node_of[x]] for x in entries]
    check(ctx, tax, recs, rules=((1, 0, 1), (rng.randint(2, 30), rng.randint(0, 10), 10), (1, 1, 1)), shuffle=seed)
    del tax


# ------------------------------------------------------------------------------------------ files and the command line

def file_lineages():
    """test_classify's file_case: three ancestors and a mutated copy of each; ancestor i and its copy are the two strains of G<i>"""
    return [("Bacteria", "G%d" % i, "anc") for i in range(3)] + [("Bacteria", "G%d" % i, "mut") for i in range(3)]


def both_files(root, tag):
    return [tp.gunzip(os.path.join(str(root), tag + suf)) for suf in ("_taxonomy.csv.gz", "_taxonomy_report.csv.gz")]


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1.0, 4.0])
def test_taxonomy_files_and_the_command_line(ctx, tmp_path, s):
    refs, recs = tc.file_case()
    tree = Tree(file_lineages())
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, s)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    ref_sets = [tp.key_set(p) for p in payloads]
    rec_sets = [tc.record_keys(seq, s) for _, _, seq in recs]
    names, lengths = [n for n, _, _ in recs], [len(seq) for _, _, seq in recs]
    (tmp_path / "recs.fa").write_bytes(tc.fasta_of(recs))
    with gzip.open(str(tmp_path / "recs.fq.gz"), "wb") as f:
        f.write(tc.fastq_of(recs))
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    (tmp_path / "lin.txt").write_text(tree.text)
    cli = lambda *a: subprocess.run([EXE] + list(a), cwd=tmp_path, capture_output=True, text=True, timeout=600)
    for tag, (min_keys, num, den, frac), records_file in (("a", (1, 0, 1, None), "recs.fa"), ("b", (2, 1, 2, "0.5"), "recs.fq.gz"), ("c", (1, 1, 1, "1"), "recs.fa")):
        rows = tree.numbered(model(tree.lineages, ref_sets, rec_sets, min_keys, num, den))
        assert tag != "a" or (sum(1 for r in rows if r[2] != NONE) > 20 and len({r[2] for r in rows}) > 3)
        records = ctx.taxonomy_files(paths, str(tmp_path / records_file), str(tmp_path / "lin.txt"), str(tmp_path / ("lib" + tag)), min_keys, num, den)
        assert as_rows(records) == rows and records["length"].tolist() == lengths
        texts = [py_csv(rows, names, lengths, tree), py_report_csv(rows, lengths, tree)]
        assert both_files(tmp_path, "lib" + tag) == texts
        args = ["-X", records_file, "-H", "lin.txt", "-f", "bank.txt", "-o", "cli" + tag] + (["-V", str(min_keys)] if min_keys != 1 else [])
        r = cli(*(args + (["-I", frac] if frac else [])))
        assert r.returncode == 0 and "classified" in r.stdout, r.stdout + r.stderr
        assert both_files(tmp_path, "cli" + tag) == texts
        assert sorted(f for f in os.listdir(tmp_path) if f.startswith("cli" + tag)) == ["cli%s_taxonomy.csv.gz" % tag, "cli%s_taxonomy_report.csv.gz" % tag]
    ctx.taxonomy_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "p3"), precision=3)
    rows = tree.numbered(model(tree.lineages, ref_sets, rec_sets))
    assert both_files(tmp_path, "p3")[0] == py_csv(rows, names, lengths, tree, 3)
    # refusals that write nothing: a lineage file of another line count, one with a bad name, none at all, no records file
    (tmp_path / "short.txt").write_text("".join(tree.text.splitlines(True)[:-1]))
    (tmp_path / "comma.txt").write_text(tree.text.replace("G1;mut", "G1;m,ut"))
    for lin, code, word in (("short.txt", sp.ERR_FORMAT, "line 6"), ("comma.txt", sp.ERR_FORMAT, "line 5"), ("none.txt", None, "")):
        with pytest.raises(sp.SpspError) as e:
            ctx.taxonomy_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / lin), str(tmp_path / "no"))
        assert (code is None or e.value.code == code) and word in str(e.value)
    with pytest.raises(sp.SpspError):
        ctx.taxonomy_files(paths, str(tmp_path / "none.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "no"))
    r = cli("-X", "recs.fa", "-H", "short.txt", "-f", "bank.txt", "-o", "no")
    assert r.returncode == 1 and "line 6" in r.stdout
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
def test_taxonomy_files_at_a_common_rate_and_its_refusals(ctx, tmp_path):
    refs, recs = tc.file_case()
    tree = Tree(file_lineages())
    sketch = lambda i, s: ctx.sketch_text(b">ref%d\n" % i + refs[i] + b"\n", tc.K_FILE, tc.M_FILE, s)[0]
    mixed_rates = [sketch(i, 1.0 if i % 2 else 4.0) for i in range(len(refs))]
    coarse = [sketch(i, 4.0) for i in range(len(refs))]
    paths = tp.write_files(tmp_path, mixed_rates)
    (tmp_path / "recs.fa").write_bytes(tc.fasta_of(recs))
    (tmp_path / "bank.txt").write_text("\n".join(paths) + "\n")
    (tmp_path / "lin.txt").write_text(tree.text)
    names, lengths = [n for n, _, _ in recs], [len(seq) for _, _, seq in recs]
    with pytest.raises(sp.SpspError) as e:                                               # the records are scanned at one threshold
        ctx.taxonomy_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "no"))
    assert e.value.code == sp.ERR_ARG and "rate" in str(e.value)
    rows = tree.numbered(model(tree.lineages, [tp.key_set(p) for p in coarse], [tc.record_keys(seq, 4.0) for _, _, seq in recs], 2))
    for rate, tag in ((4.0, "r4"), ("auto", "auto")):
        records = ctx.taxonomy_files(paths, str(tmp_path / "recs.fa"), str(tmp_path / "lin.txt"), str(tmp_path / tag), 2, rate=rate)
        assert as_rows(records) == rows
        assert both_files(tmp_path, tag) == [py_csv(rows, names, lengths, tree), py_report_csv(rows, lengths, tree)]
    r = subprocess.run([EXE, "-X", "recs.fa", "-H", "lin.txt", "-f", "bank.txt", "-V", "2", "-s", "4", "-o", "cli"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and both_files(tmp_path, "cli") == both_files(tmp_path, "r4"), r.stdout + r.stderr
    r = subprocess.run([EXE, "-X", "recs.fa", "-H", "lin.txt", "-f", "bank.txt", "-o", "no"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "rate" in r.stdout
    assert not [f for f in os.listdir(tmp_path) if f.startswith("no_")]


@pytest.mark.gpu
def test_65537_records_cross_the_batch_seam(ctx, tmp_path):
    """one scan, two key extractions (65 535 records and 2): the rows of the records on both sides of the seam"""
    n_rec, s = 65537, 1.0
    rng = np.random.default_rng(13)
    refs = [tc.random_bases(rng, 3000) for _ in range(2)]
    seq_of = lambda r: refs[r % 2][(r * 7) % 2960:(r * 7) % 2960 + 40]
    special = {65534: seq_of(65534), 65535: seq_of(65535), 65536: tc.random_bases(rng, 40), 0: tc.random_bases(rng, 40)}
    seqs = [special.get(r) or seq_of(r) for r in range(n_rec)]
    (tmp_path / "many.fa").write_bytes(b"".join(b">r%d\n%s\n" % (r, q) for r, q in enumerate(seqs)))
    tree = Tree([("G", "a"), ("G", "b")])
    (tmp_path / "lin.txt").write_text(tree.text)
    payloads = [ctx.sketch_text(b">ref%d\n" % i + g + b"\n", tc.K_FILE, tc.M_FILE, s)[0] for i, g in enumerate(refs)]
    paths = tp.write_files(tmp_path, payloads)
    records = ctx.taxonomy_files(paths, str(tmp_path / "many.fa"), str(tmp_path / "lin.txt"), str(tmp_path / "many"))
    assert len(records) == n_rec and (records["length"] == 40).all()
    ref_sets = [tp.key_set(p) for p in payloads]
    sample = sorted(set([0, 1, 2, 65533, 65534, 65535, 65536] + rng.integers(0, n_rec, 12).tolist()))
    want = tree.numbered(model(tree.lineages, ref_sets, [tc.record_keys(seqs[r], s) for r in sample]))
    assert as_rows(records[sample]) == want
    assert want[sample.index(65534)][2] == tree.num[("G", "a")] and want[sample.index(65535)][2] == tree.num[("G", "b")]
    assert want[sample.index(65536)][2] == NONE and want[0][2] == NONE
    lines = tp.gunzip(str(tmp_path / "many_taxonomy.csv.gz")).decode().splitlines()
    assert len(lines) == 1 + n_rec and lines[-1].startswith("65536,r65536,40,") and lines[-1].endswith(",,,,0,0,0,0,0")
    report = tp.gunzip(str(tmp_path / "many_taxonomy_report.csv.gz")).decode().splitlines()
    called = int((records["node"] != NONE).sum())
    assert report[1].split(",")[5] == str(called) and report[-1].split(",")[5] == str(n_rec - called) and len(report) == 1 + 4 + 1
