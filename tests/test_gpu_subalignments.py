"""-s on the device: cl_subalignment_text (subaln_kernels.hip) against a Python restatement of Core::emit_subalignment (src/core.cpp:424-472)
on merge graphs and crafted path graphs; cl_msa's -s file, --bond-prefix files and --force-gfa-output against the compiled reference's
(tests/golden/make_subalignments.py), at one and four workers.  test_gpu_block_at_the_sizes_of_a_real_merge reaches the branches that only
a 1 Mbp merge does: 2 300 000 path steps, more than the 8 192 x 256 = 2 097 152 threads of subaln_step_table_kernel, whose grid-stride loop
runs a second time; 263 000 pairs in one chunk, more than 1 024 x 256 = 262 144, hence 1 028 workgroup sums and a second tile (with a carry)
in subaln_offsets_kernel, and a failing pair reported by a workgroup beyond the first tile; step numbers of one to seven digits."""
import hashlib
import json
import os
import random

import numpy as np
import pytest

from centrolign_amd import capi
from tests import helpers as H
from tests.golden import make_subalignments as ms
from tests.test_gpu_induced_pairs import path_graph

GAP = 2 ** 64 - 1
WANT = json.load(open(os.path.join(H.GOLDEN, "subalignments.json")))
DEC = "ACGTN"


def py_subalignment(g1, pn1, set1, g2, pn2, set2, pairs):
    """Core::emit_subalignment, line by line: StepIndex::path_steps(node).front() is the first (path, step) in path order"""
    def first_steps(g):
        first = {}
        for p in range(len(g.path_off) - 1):
            for i, v in enumerate(g.path_nodes[int(g.path_off[p]):int(g.path_off[p + 1])].tolist()):
                first.setdefault(v, (p, i))
        return first
    f1, f2 = first_steps(g1), first_steps(g2)
    out = ["# sequence set 1\n"] + [s + "\n" for s in set1] + ["# sequence set 2\n"] + [s + "\n" for s in set2] + ["# alignment\n"]

    def side(g, f, names, v):
        if v == GAP:
            return "-\t-\t-"
        p, i = f[v]
        lab = int(g.label[v])
        return "%s\t%d\t%s" % (names[p], i, DEC[lab] if lab < 5 else "\0")
    for a, b in pairs:
        out.append(side(g1, f1, pn1, int(a)) + "\t" + side(g2, f2, pn2, int(b)) + "\n")
    return "".join(out).encode()


def check(ctx, g1, pn1, set1, g2, pn2, set2, pairs, chunk_bytes=0):
    got = capi.subalignment_text(ctx, g1, pn1, set1, g2, pn2, set2, pairs, chunk_bytes=chunk_bytes)
    assert got == py_subalignment(g1, pn1, set1, g2, pn2, set2, pairs)
    return got


def random_sequence(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


@pytest.mark.gpu
def test_gpu_block_equals_restatement_on_merge_graphs(gpu_ctx):
    """graphs and alignments of real cl_merge calls: two leaves, then a two-path graph with a leaf, then two multi-path graphs"""
    rng = random.Random(7)
    anc = random_sequence(rng, 1500)
    seqs = ["".join(c if rng.random() > 0.03 else rng.choice("ACGT") for c in anc) for _ in range(5)]
    leaves = [capi.leaf_graph(s) for s in seqs]
    names = ["s%d" % i for i in range(5)]
    m01 = gpu_ctx.merge(leaves[0], leaves[1])
    check(gpu_ctx, leaves[0], names[:1], names[:1], leaves[1], names[1:2], names[1:2], m01["alignment"])
    m012 = gpu_ctx.merge(m01["fused"], leaves[2])
    check(gpu_ctx, m01["fused"], names[:2], names[1::-1], leaves[2], names[2:3], names[2:3], m012["alignment"])
    m34 = gpu_ctx.merge(leaves[3], leaves[4])
    root = gpu_ctx.merge(m012["fused"], m34["fused"])
    got = check(gpu_ctx, m012["fused"], names[:3], names[2::-1], m34["fused"], names[3:], names[:2:-1], root["alignment"])
    assert got.count(b"\n") == 3 + 2 + 3 + len(root["alignment"])


def crafted_graph(rng, n_nodes, n_paths, revisit=True):
    """labels 0..5 (5 prints a NUL byte, as decode_base does) and paths over shared nodes; a path that visits nodes twice; a node on no path"""
    labels = [rng.randrange(6) for _ in range(n_nodes)]
    paths = []
    for p in range(n_paths):
        k = rng.randrange(1, 3 * n_nodes // n_paths + 2)
        path = [rng.randrange(n_nodes - 1) for _ in range(k)]   # node n_nodes - 1 is on no path
        if revisit and p == 0:
            path = path + path[: max(1, len(path) // 2)]
        paths.append(path)
    return path_graph(labels, paths), sorted({v for p in paths for v in p})


def random_pairs(rng, on1, on2, n, lead_gap=False, tail_gap=False):
    pairs = []
    if lead_gap:
        pairs += [(GAP, rng.choice(on2)) for _ in range(3)]
    for _ in range(n):
        r = rng.random()
        pairs.append((GAP if r < 0.15 else rng.choice(on1), GAP if 0.15 <= r < 0.3 else rng.choice(on2)))
    if tail_gap:
        pairs += [(rng.choice(on1), GAP) for _ in range(4)]
    return pairs


@pytest.mark.gpu
def test_gpu_block_equals_restatement_on_crafted_graphs(gpu_ctx):
    rng = random.Random(11)
    for t in range(12):
        g1, on1 = crafted_graph(rng, rng.randrange(2, 400), rng.randrange(1, 6))
        g2, on2 = crafted_graph(rng, rng.randrange(2, 400), rng.randrange(1, 6))
        pn1 = ["path_%d_%s" % (p, "x" * rng.randrange(12)) for p in range(len(g1.path_off) - 1)]
        pn2 = ["q%d" % p for p in range(len(g2.path_off) - 1)]
        pairs = random_pairs(rng, on1, on2, rng.randrange(0, 3000), lead_gap=t % 2 == 0, tail_gap=t % 3 == 0)
        check(gpu_ctx, g1, pn1, ["a", "b"], g2, pn2, ["c"], pairs)


@pytest.mark.gpu
def test_gpu_block_no_pairs_and_gap_only(gpu_ctx):
    g1, _ = crafted_graph(random.Random(3), 10, 2)
    g2, _ = crafted_graph(random.Random(4), 10, 2)
    got = check(gpu_ctx, g1, ["p", "q"], ["x", "y"], g2, ["r", "s"], ["z"], [])
    assert got == b"# sequence set 1\nx\ny\n# sequence set 2\nz\n# alignment\n"
    check(gpu_ctx, g1, ["p", "q"], [], g2, ["r", "s"], [], [(GAP, GAP)] * 3)


@pytest.mark.gpu
def test_gpu_block_in_many_chunks(gpu_ctx):
    """chunk_bytes small enough for many chunks (and below one line: a chunk holds one pair) gives the same bytes"""
    rng = random.Random(19)
    g1, on1 = crafted_graph(rng, 3000, 4)
    g2, on2 = crafted_graph(rng, 3000, 3)
    pn1, pn2 = ["a%d" % p for p in range(4)], ["bb%d" % p for p in range(3)]
    pairs = random_pairs(rng, on1, on2, 5000, lead_gap=True, tail_gap=True)
    whole = check(gpu_ctx, g1, pn1, ["s"], g2, pn2, ["t"], pairs)
    max_line = 2 * (len("bb0") + 13) + 2   # the bound a chunk is sized by
    for cb in (2000, 20000, 1):
        assert -(-len(pairs) // max(1, cb // max_line)) > 3   # more than three chunks
        assert capi.subalignment_text(gpu_ctx, g1, pn1, ["s"], g2, pn2, ["t"], pairs, chunk_bytes=cb) == whole


@pytest.mark.gpu
def test_gpu_block_error_codes(gpu_ctx):
    rng = random.Random(23)
    g1, on1 = crafted_graph(rng, 50, 2)
    g2, on2 = crafted_graph(rng, 60, 2)
    pairs = random_pairs(rng, on1, on2, 2000)
    for bad, what in (((0, 60), "out of range"), ((50, GAP), "out of range"), ((49, GAP), "no path"), ((GAP, 59), "no path")):
        p = list(pairs)
        p[1234] = bad
        p[1900] = bad
        with pytest.raises(capi.ClError) as e:
            capi.subalignment_text(gpu_ctx, g1, ["a", "b"], [], g2, ["c", "d"], [], p, chunk_bytes=4096)
        assert e.value.code == -1   # CL_ERR_INVALID_ARGUMENT
        assert "pair 1234 " in str(e.value) and what in str(e.value)


def np_subalignment(g1, pn1, set1, g2, pn2, set2, pairs):
    """py_subalignment for millions of steps: a node's first (path, step) is where the node first occurs in the flat step array, since that
    array holds path 0's steps, then path 1's, each in step order.  Returns (bytes, the step of side 1 per pair, -1 for a gap)"""
    def first_steps(g):
        nodes, at = np.unique(g.path_nodes, return_index=True)
        off = g.path_off.astype(np.int64)
        path = np.searchsorted(off, at, side="right") - 1
        p_of, s_of = np.full(len(g.label), -1, np.int64), np.full(len(g.label), -1, np.int64)
        p_of[nodes], s_of[nodes] = path, at - off[path]
        return p_of, s_of
    pairs = np.asarray(pairs, np.uint64).reshape(-1, 2)
    cols, steps1 = [], None
    for g, names, col in ((g1, pn1, pairs[:, 0]), (g2, pn2, pairs[:, 1])):
        p_of, s_of = first_steps(g)
        gap = col == np.uint64(GAP)
        v = np.where(gap, 0, col).astype(np.int64)
        assert np.all(gap | (p_of[v] >= 0)), "a node on no path"
        dec = list(DEC) + ["\0"]
        cols.append(["-\t-\t-" if is_gap else "%s\t%d\t%s" % (names[p], s, dec[lab])
                     for is_gap, p, s, lab in zip(gap.tolist(), p_of[v].tolist(), s_of[v].tolist(), np.minimum(g.label[v], 5).tolist())])
        if steps1 is None:
            steps1 = np.where(gap, -1, s_of[v])
    head = ["# sequence set 1\n"] + [s + "\n" for s in set1] + ["# sequence set 2\n"] + [s + "\n" for s in set2] + ["# alignment\n"]
    return "".join(head + [a + "\t" + b + "\n" for a, b in zip(*cols)]).encode(), steps1


@pytest.mark.gpu
def test_gpu_block_at_the_sizes_of_a_real_merge(gpu_ctx):
    """graph 1: two paths over 2 200 000 nodes, 0 .. 1 099 999 and 1 000 000 .. 2 199 999 — 2 300 000 steps; the 100 000 shared nodes belong
    to path 0 by the first-step rule.  263 000 pairs in one chunk, gaps on both sides, node picks drawn by the number of digits of their step
    so that one to seven digits occur below and from pair 262 144 on (the second tile of the offset scan).  Then a node on no path at pairs
    262 200 and 262 900: the smaller index, found by a workgroup beyond the first tile."""
    rng = random.Random(31)
    small1, on_small1 = crafted_graph(rng, 300, 3)
    g2, on2 = crafted_graph(rng, 300, 3)
    pn2 = ["q%d" % p for p in range(3)]
    few = random_pairs(rng, on_small1, on2, 500, lead_gap=True, tail_gap=True)   # the restatement against py_subalignment, cyclic paths included
    assert np_subalignment(small1, ["x0", "x1", "x2"], ["a"], g2, pn2, ["b"], few)[0] == py_subalignment(small1, ["x0", "x1", "x2"], ["a"], g2, pn2, ["b"], few)

    nprng = np.random.default_rng(31)
    n_nodes, n_pairs, tile = 2200000, 263000, 1024 * 256
    g1 = path_graph(nprng.integers(0, 6, n_nodes), [np.arange(0, 1100000), np.arange(1000000, 2200000)])
    assert int(g1.path_off[-1]) == 2300000 > 8192 * 256
    # a step of d digits, on path 0 (node = step; for seven digits a shared node) or, from six digits on, on path 1 (node = step + 1 000 000)
    d = nprng.integers(1, 8, n_pairs)
    lo, hi = np.where(d == 1, 0, 10 ** (d - 1)), 10 ** d
    on_path1 = (d >= 6) & (nprng.random(n_pairs) < 0.5)
    hi = np.where(d == 7, np.where(on_path1, 1200000, 1100000), hi)
    step = (lo + nprng.random(n_pairs) * (hi - lo)).astype(np.int64)
    pairs = np.stack([np.where(on_path1, step + 1000000, step), nprng.choice(np.asarray(on2), n_pairs)], 1).astype(np.uint64)
    r = nprng.random(n_pairs)
    pairs[r < 0.15, 0] = GAP
    pairs[(r >= 0.15) & (r < 0.3), 1] = GAP
    want, steps1 = np_subalignment(g1, ["p0", "p1"], ["s", "t"], g2, pn2, ["u"], pairs)
    assert np.array_equal(steps1[pairs[:, 0] != np.uint64(GAP)], step[pairs[:, 0] != np.uint64(GAP)])   # shared nodes: path 0's step, not path 1's
    for part in (steps1[:tile], steps1[tile:]):
        assert {len(str(s)) for s in part[part >= 0].tolist()} == set(range(1, 8))
        assert np.any(part < 0)
    assert -(-n_pairs // 256) == 1028 > 1024
    got = capi.subalignment_text(gpu_ctx, g1, ["p0", "p1"], ["s", "t"], g2, pn2, ["u"], pairs)
    if got != want:
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else min(len(got), len(want))
        pytest.fail("%d bytes for %d; the first difference at byte %d, line %d" % (len(got), len(want), at, want[:at].count(b"\n")))
    bad = pairs.copy()
    bad[262200, 0], bad[262900, 0] = GAP, 7
    bad[262200, 1] = bad[262900, 1] = len(g2.label) - 1   # crafted_graph leaves its last node on no path
    with pytest.raises(capi.ClError) as e:
        capi.subalignment_text(gpu_ctx, g1, ["p0", "p1"], ["s", "t"], g2, pn2, ["u"], bad)
    assert e.value.code == -1 and "pair 262200 " in str(e.value) and "no path" in str(e.value)


def fasta_of(names, seqs):
    return "".join(">%s\n%s\n" % (n, s) for n, s in zip(names, seqs)).encode()


def run_case(ctx, case, d, workers, **kw):
    names, seqs, newick, budget, _ = ms.workload(case)
    return ctx.msa(fasta_of(names, seqs), newick, max_num_match_pairs=budget, workers=workers, **kw)


def sha(b):
    return hashlib.sha256(b).hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [1, 4])
@pytest.mark.parametrize("case", ["sub_nobond", "sub_unbalanced", "sub_two"])
def test_gpu_cl_msa_subalignment_file_is_the_references(gpu_ctx, tmp_path, case, workers):
    sub = str(tmp_path / "sub.txt")
    text, st = run_case(gpu_ctx, case, tmp_path, workers, subalignments_path=sub)
    assert sha(open(sub, "rb").read()) == WANT[case]["files"]["sub.txt"]["sha256"]
    if case == "sub_two":
        assert text == json_text("sub_two", "cigar.txt")


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [1, 4])
def test_gpu_cl_msa_restart_writes_only_the_recomputed_merges(gpu_ctx, tmp_path, workers):
    prefix = str(tmp_path / "sp")
    run_case(gpu_ctx, "sub_restart", tmp_path, workers, subproblems_prefix=prefix)
    info = [ln.split("\t") for ln in open(prefix + "_info.txt").read().split("\n")[1:] if ln]
    removed = {tuple(r) for r in WANT["sub_restart"]["removed"]}
    gone = [f for f, s in info if tuple(s.split(",")) in removed]
    assert len(gone) == 2
    for f in gone:
        os.remove(f)
    sub = str(tmp_path / "sub.txt")
    text, st = run_case(gpu_ctx, "sub_restart", tmp_path, workers, subproblems_prefix=prefix, restart=True, subalignments_path=sub)
    assert sha(open(sub, "rb").read()) == WANT["sub_restart"]["files"]["sub.txt"]["sha256"]


def json_text(case, f):
    import gzip
    return json.loads(gzip.decompress(open(os.path.join(H.GOLDEN, "subalignments_text.json.gz"), "rb").read()))[case][f].encode("latin-1")


@pytest.mark.gpu
def test_gpu_cl_msa_force_gfa_output(gpu_ctx, tmp_path):
    """two sequences: the root GFA with --force-gfa-output (the reference's root -S file), the CIGAR without"""
    text, st = run_case(gpu_ctx, "sub_two", tmp_path, 1, force_gfa_output=True)
    assert text == json_text("sub_two", "root.gfa")
    text, st = run_case(gpu_ctx, "sub_two", tmp_path, 1)
    assert text == json_text("sub_two", "cigar.txt")


@pytest.mark.gpu
def test_gpu_cl_msa_refuses_an_existing_subalignment_file(gpu_ctx, tmp_path):
    sub = tmp_path / "sub.txt"
    sub.write_bytes(b"earlier run\n")
    prefix = str(tmp_path / "sp")
    with pytest.raises(capi.ClError) as e:
        run_case(gpu_ctx, "sub_unbalanced", tmp_path, 1, subalignments_path=str(sub), subproblems_prefix=prefix)
    assert "Subalignment file already exists: " + str(sub) in str(e.value)
    assert sub.read_bytes() == b"earlier run\n"
    assert sorted(os.listdir(tmp_path)) == ["sub.txt"]   # nothing else was done


@pytest.mark.gpu
@pytest.mark.parametrize("workers", [4, 1])
def test_gpu_cl_msa_cyclize_bond_files_and_subalignments(gpu_ctx, tmp_path, workers):
    """-c -s --bond-prefix -S: every bond CIGAR file and the -s file as the reference wrote them, the GFA unchanged; then a bond restart
    (-R with PREFIX_bonds.txt) writes no bond files and the same GFA"""
    want = WANT["sub_cyclize"]
    names, seqs, newick, budget, min_len = ms.workload("sub_cyclize")
    fa = fasta_of(names, seqs)
    d1 = tmp_path / "run"
    d1.mkdir()
    text, st = gpu_ctx.msa(fa, newick, max_num_match_pairs=budget, workers=workers, cyclize=True, min_cyclizing_length=min_len,
                           subalignments_path=str(d1 / "sub.txt"), bonds_prefix=str(d1 / "bd"), subproblems_prefix=str(d1 / "sp"))
    assert sha(text) == want["gfa"]["sha256"]
    got = {f: (d1 / f).read_bytes() for f in os.listdir(d1) if f.startswith("bd_") or f in ("sub.txt", "sp_bonds.txt")}
    assert sorted(got) == sorted(want["files"])
    for f, b in sorted(got.items()):
        assert sha(b) == want["files"][f]["sha256"], f
    if workers != 1:
        return
    d2 = tmp_path / "restart"
    d2.mkdir()
    (d2 / "sp_bonds.txt").write_bytes(ms.bonds_text(ms.load_bonds()))
    text2, st2 = gpu_ctx.msa(fa, newick, max_num_match_pairs=budget, workers=workers, cyclize=True, min_cyclizing_length=min_len,
                             bonds_prefix=str(d2 / "bd"), subproblems_prefix=str(d2 / "sp"), restart=True)
    assert text2 == text
    assert not [f for f in os.listdir(d2) if f.startswith("bd_")]


@pytest.mark.gpu
def test_gpu_cl_msa_without_the_new_options_is_unchanged(gpu_ctx, tmp_path):
    """-A without -c on the six-sequence inputs: the .txt files and the GFA of the committed goldens (make_induced_maf.py: with no bond found,
    -c writes the same GFA and .txt files), and no other file"""
    want = json.load(open(os.path.join(H.GOLDEN, "induced_nobond.json")))
    text, st = run_case(gpu_ctx, "sub_nobond", tmp_path, 4, induced_pairwise_prefix=str(tmp_path / "pw"))
    assert sha(text) == want["gfa"]["sha256"]
    files = sorted(os.listdir(tmp_path))
    assert files == sorted("pw_" + f for f in want["files"] if f.endswith(".txt"))
    for f in files:
        assert sha((tmp_path / f).read_bytes()) == want["files"][f[3:]]["sha256"], f
