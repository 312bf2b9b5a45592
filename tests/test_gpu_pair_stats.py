"""Pairwise alignment statistics on the device: cl_induced_pairwise_stats (induced_stats_kernel) against the host function pair by pair,
cl_msa's --pair-stats file against the -A files of the same run (whose digests are the compiled reference's), cl_refine_guide_tree against its
parts composed by hand, and the command line's --pair-stats / --dist-out / --refine-tree.  Every comparison is exact."""
import gzip
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests import helpers as H
from tests import test_gpu_induced_pairs as tip
from tests import test_pair_stats as tps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
HEADER = "sample1 sample2 matches mismatches insertions deletions match_runs mismatch_runs insertion_runs deletion_runs distance".split()
_faulted = []


def row(d):
    return [d[k] for k in capi.PAIR_STATS_FIELDS]


def device_or_code(ctx, g, pairs):
    try:
        return capi.induced_pairwise_stats(g, pairs, ctx).tolist()
    except capi.ClError as e:
        return e.code


def check_all_pairs(ctx, g):
    """every ordered pair: the pairs the host function aligns in one batch, each failing pair alone with the host's code"""
    n = len(g.path_off) - 1
    want = {p: tps.stat_or_code(g, *p) for p in tip.all_pairs(n)}
    pairs = [p for p in tip.all_pairs(n) if not isinstance(want[p], int)]
    got = capi.induced_pairwise_stats(g, pairs, ctx)
    for p, st in zip(pairs, got.tolist()):
        assert st == row(want[p]), p
    for p in tip.all_pairs(n):
        if isinstance(want[p], int):
            assert device_or_code(ctx, g, [p]) == want[p], p
    return n * n


@pytest.mark.gpu
def test_gpu_stats_equal_host_on_msa_graphs(gpu_ctx):
    seen = 0
    for name, g in tip.golden_graphs():
        seen += check_all_pairs(gpu_ctx, g)
    rng = np.random.default_rng(5)
    for k in range(6):
        anc = "".join("ACGT"[b] for b in rng.integers(0, 4, int(rng.integers(50, 3000))))
        seen += check_all_pairs(gpu_ctx, synth.bubble_graph(anc, 4, seed=70 + k, alt_p=0.1, skip_p=0.05))
    assert seen > 2500


@pytest.mark.gpu
def test_gpu_stats_equal_host_on_crafted_paths(gpu_ctx):
    """out-of-order and repeated meetings, 4 x 4 and 5 x 5 gap runs, empty and one-step paths; 30 000-step paths over many tiles of the kernel
    with runs crossing tile edges; the same pairs shuffled and repeated in one batch"""
    small, long = tps.crafted_graphs()
    n = len(small.path_off) - 1
    assert check_all_pairs(gpu_ctx, small) == n * n
    rng = np.random.default_rng(9)
    pairs = [tuple(int(x) for x in p) for p in rng.integers(0, n, (500, 2)) if int(p[0]) != 4]   # (path 4 repeats nodes: only a second path)
    got = capi.induced_pairwise_stats(small, pairs, gpu_ctx).tolist()
    assert got == [row(capi.induced_pairwise_stat(small, a, b)) for a, b in pairs]
    assert check_all_pairs(gpu_ctx, long) == 16
    # the device's numbers are the parse of the device's own text too
    pairs = [p for p in tip.all_pairs(4) if not isinstance(tps.stat_or_code(long, *p), int)]   # (path 1 may meet a drawn node twice)
    cig = capi.induced_pairwise_cigars(long, pairs, gpu_ctx)
    assert len(pairs) >= 12 and capi.induced_pairwise_stats(long, pairs, gpu_ctx).tolist() == [row(tps.parse_cigar(c)) for c in cig]


@pytest.mark.gpu
def test_gpu_stats_error_codes_follow_the_host(gpu_ctx):
    labels = [0, 1, 2, 3] * 5
    g = tip.path_graph(labels, [[0, 1, 2, 1, 3], [0, 1, 2, 3, 4], [5, 6, 7], [8, 9]])   # path 0 visits node 1 twice
    for pairs in ([(0, 1)], [(1, 0)], [(1, 2), (2, 3), (0, 3)], [(1, 1), (3, 2), (1, 9)], [(1, 9), (0, 1)]):
        want = next((c for c in (tps.stat_or_code(g, a, b) for a, b in pairs) if isinstance(c, int)), None)
        got = device_or_code(gpu_ctx, g, pairs)
        if want is None:
            assert got == [row(capi.induced_pairwise_stat(g, a, b)) for a, b in pairs]
        else:
            assert got == want, pairs
    bad = tip.path_graph(labels, [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    bad.path_nodes[4] = 1000
    assert device_or_code(gpu_ctx, bad, [(1, 0)]) == tps.stat_or_code(bad, 1, 0) == -7   # CL_ERR_CYCLIC_GRAPH
    assert device_or_code(gpu_ctx, bad, [(0, 1)]) == tps.stat_or_code(bad, 0, 1) == -1   # CL_ERR_INVALID_ARGUMENT
    assert device_or_code(gpu_ctx, bad, [(0, 2), (2, 0), (0, 1), (1, 2)]) == tps.stat_or_code(bad, 0, 1)
    assert capi.induced_pairwise_stats(g, [], gpu_ctx).shape == (0, 8)


@pytest.mark.gpu
def test_gpu_stats_batch_larger_than_a_chunk(gpu_ctx):
    """more pairs than one chunk holds (2 048)"""
    g = capi.read_gfa(gzip.decompress(open(os.path.join(H.GOLDEN, "wide_merge_24x7k.gfa.gz"), "rb").read()))[0]
    n = len(g.path_off) - 1
    rng = np.random.default_rng(3)
    pairs = [tuple(int(x) for x in p) for p in rng.integers(0, n, (2600, 2))]
    got = capi.induced_pairwise_stats(g, pairs, gpu_ctx).tolist()
    one = {p: row(capi.induced_pairwise_stat(g, *p)) for p in set(pairs)}
    assert got == [one[p] for p in pairs]


def read_tsv(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    return [ln.split("\t") for ln in lines[1:-1]]


def check_tsv_against_txt(rows, names, files):
    """row k is pair (p, q), p < q, of `names` (the root graph's path order); its numbers are the parse of the pair's .txt file"""
    pairs = [(a, b) for a in range(len(names)) for b in range(a + 1, len(names))]
    assert len(rows) == len(pairs)
    for r, (a, b) in zip(rows, pairs):
        assert r[:2] == [names[a], names[b]]
        st = tps.parse_cigar(files["%s_%s.txt" % (names[a], names[b])])
        assert [int(v) for v in r[2:10]] == row(st), (a, b)
        assert r[10] == "%.9g" % tps.formula(st["eq"], st["x"], st["ins"], st["del"]), (a, b)


@pytest.mark.gpu
def test_gpu_cl_msa_pair_stats_with_cyclize(gpu_ctx, tmp_path):
    """-c -A --pair-stats in one run: the rows are the parse of the .txt files, whose digests are the compiled reference's; the GFA is what
    it is without the new field"""
    from tests.golden import make_induced_maf as mim
    case = "induced_16x12k"
    want = json.load(open(os.path.join(H.GOLDEN, case + ".json")))
    names, seqs, newick, min_len, budget = mim.workload(case)
    fasta = "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs)).encode()
    text, st = gpu_ctx.msa(fasta, newick, max_num_match_pairs=budget, induced_pairwise_prefix=str(tmp_path / "pw"), cyclize=True,
                           min_cyclizing_length=min_len, pair_stats_path=str(tmp_path / "stats.tsv"))
    assert hashlib.sha256(text).hexdigest() == want["gfa"]["sha256"]
    files = {f[3:]: open(os.path.join(tmp_path, f), "rb").read() for f in os.listdir(tmp_path) if f.startswith("pw_")}
    txt = sorted(f for f in files if f.endswith(".txt"))
    assert len(txt) == len(names) * (len(names) - 1) // 2
    for f in txt:
        assert hashlib.sha256(files[f]).hexdigest() == want["files"][f]["sha256"], f
    # the root graph's path order: the first path is sample1 of the first row, then sample2 of the rows it leads
    rows = read_tsv(tmp_path / "stats.tsv")
    order = [rows[0][0]] + [r[1] for r in rows[:len(names) - 1]]
    assert sorted(order) == sorted(names)
    check_tsv_against_txt(rows, order, files)


@pytest.mark.gpu
def test_gpu_cl_msa_pair_stats_without_cyclize(gpu_ctx, tmp_path):
    from tests.test_restart import case
    d = case()
    fasta, newick, budget = bytes(d["fasta"]), str(d["newick"][0]), int(d["budget"][0])
    plain, _ = gpu_ctx.msa(fasta, newick, max_num_match_pairs=budget)
    text, _ = gpu_ctx.msa(fasta, newick, max_num_match_pairs=budget, induced_pairwise_prefix=str(tmp_path / "pw"), pair_stats_path=str(tmp_path / "stats.tsv"))
    assert text == plain
    root, names = capi.read_gfa(text, add_sentinels=True)
    files = {f[3:]: open(os.path.join(tmp_path, f), "rb").read() for f in os.listdir(tmp_path) if f.startswith("pw_")}
    rows = read_tsv(tmp_path / "stats.tsv")
    check_tsv_against_txt(rows, names, files)
    # and the library calls on the GFA read back
    pairs = [(a, b) for a in range(len(names)) for b in range(a + 1, len(names))]
    stats = capi.induced_pairwise_stats(root, pairs, gpu_ctx)
    assert [[int(v) for v in r[2:10]] for r in rows] == stats.tolist()
    dist = capi.alignment_distances(stats, len(names))
    assert [r[10] for r in rows] == ["%.9g" % dist[a, b] for a, b in pairs]


def family(seed, length=30000):
    """((0,1),(2,3)),(4,5) from one HOR array, in the style of test_gpu_tree_infer.evolve_family"""
    rng = random.Random(seed)
    root = synth.hor_sequences(seed, length, 1)[0]

    def down(s, r):
        return "".join(synth._mut_track(rng, s, r)[0])

    a, b = down(root, 0.004), down(root, 0.004)
    a0, a1 = down(a, 0.003), down(a, 0.003)
    leaves = [down(a0, 0.002), down(a0, 0.002), down(a1, 0.002), down(a1, 0.002), down(b, 0.003), down(b, 0.003)]
    order = [3, 0, 4, 1, 5, 2]   # the FASTA order is not the tree's
    return ["leaf%d" % i for i in order], [leaves[i] for i in order]


def refine_by_hand(ctx, fasta, names, newick, max_rounds, **kw):
    """cl_refine_guide_tree's rounds from their parts"""
    rounds, converged = 0, False
    while rounds < max_rounds and not converged:
        text, _ = ctx.msa(fasta, newick, force_gfa_output=True, **kw)
        g, pnames = capi.read_gfa(text, add_sentinels=True)
        n = len(pnames)
        pairs = [(a, b) for a in range(n) for b in range(a + 1, n)]
        by_path = capi.alignment_distances(capi.induced_pairwise_stats(g, pairs, ctx), n)
        seq_of = [names.index(nm) for nm in pnames]
        by_seq = np.zeros((n, n))
        for p in range(n):
            for q in range(n):
                by_seq[seq_of[p], seq_of[q]] = by_path[p, q]
        nxt = capi.neighbor_joining_newick(by_seq, names)
        rounds += 1
        converged = newick is not None and nxt == newick
        newick = nxt
    return newick, rounds, converged


@pytest.mark.gpu
def test_gpu_refine_guide_tree_is_its_parts(gpu_ctx):
    names, seqs = family(4)
    fasta = "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs))
    kw = dict(max_num_match_pairs=200000)
    for start, max_rounds in ((None, 1), (None, 3), (capi.infer_guide_tree(gpu_ctx, fasta), 2)):
        want = refine_by_hand(gpu_ctx, fasta, names, start, max_rounds, **kw)
        got = gpu_ctx.refine_guide_tree(fasta, start, max_rounds, **kw)
        assert got == want, (start, max_rounds)
        assert gpu_ctx.refine_guide_tree(fasta, start, max_rounds, **kw) == got
        assert 1 <= got[1] <= max_rounds and (got[2] or got[1] == max_rounds)
    # a tree that refinement returns as converged is its own refinement
    tree, rounds, converged = gpu_ctx.refine_guide_tree(fasta, None, 4, **kw)
    if converged:
        assert gpu_ctx.refine_guide_tree(fasta, tree, 1, **kw) == (tree, 1, True)
    # fewer than three sequences: no round, the input back
    two = "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names[:2], seqs[:2]))
    assert gpu_ctx.refine_guide_tree(two, None, 2, **kw) == (None, 0, False)
    assert gpu_ctx.refine_guide_tree(two, "(leaf3,leaf0);", 2, **kw) == ("(leaf3,leaf0);", 0, False)
    with pytest.raises(capi.ClError):
        gpu_ctx.refine_guide_tree(fasta, None, 0, **kw)


def run(args, cwd, timeout=900):
    if _faulted:
        pytest.fail("an earlier child of this module ended abnormally (%s): no further GPU process is started" % _faulted[0])
    try:
        r = subprocess.run([BIN] + [str(a) for a in args], cwd=str(cwd), capture_output=True, timeout=timeout, stdin=subprocess.DEVNULL)
    except subprocess.TimeoutExpired:
        _faulted.append("time limit of %d s" % timeout)
        raise
    if r.returncode < 0:
        _faulted.append("signal %d" % -r.returncode)
        pytest.fail("killed by signal %d: %s" % (-r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    return r


@pytest.mark.gpu
def test_gpu_cli_refine_tree_pair_stats_and_distances(gpu_ctx, tmp_path):
    names, seqs = family(4)
    fasta = "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs))
    (tmp_path / "in.fa").write_text(fasta)
    a = run(["-a", 200000, "--refine-tree", 2, "--tree-out", "t.nwk", "--pair-stats", "ps.tsv", "--dist-out", "d.txt", "-A", "pw", "in.fa"], tmp_path)
    assert b"highly recommended" not in a.stderr
    tree = (tmp_path / "t.nwk").read_text()
    assert tree.endswith(";\n")
    assert tree[:-1] == gpu_ctx.refine_guide_tree(fasta, None, 2, max_num_match_pairs=200000)[0]
    b = run(["-a", 200000, "-T", "t.nwk", "in.fa"], tmp_path)
    assert a.stdout == b.stdout
    # the files against the library calls on the printed graph
    g, pnames = capi.read_gfa(a.stdout, add_sentinels=True)
    n = len(pnames)
    pairs = [(p, q) for p in range(n) for q in range(p + 1, n)]
    stats = capi.induced_pairwise_stats(g, pairs, gpu_ctx)
    dist = capi.alignment_distances(stats, n)
    rows = read_tsv(tmp_path / "ps.tsv")
    assert [r[:2] for r in rows] == [[pnames[p], pnames[q]] for p, q in pairs]
    assert [[int(v) for v in r[2:10]] for r in rows] == stats.tolist()
    assert [r[10] for r in rows] == ["%.9g" % dist[p, q] for p, q in pairs]
    files = {f[3:]: open(os.path.join(tmp_path, f), "rb").read() for f in os.listdir(tmp_path) if f.startswith("pw_")}
    check_tsv_against_txt(rows, pnames, files)
    want = ["%d" % n] + ["\t".join([nm] + ["%.9g" % dist[pnames.index(nm), pnames.index(other)] for other in names]) for nm in names]
    assert (tmp_path / "d.txt").read_text() == "\n".join(want) + "\n"
    # --dist-out alone leaves nothing else behind
    os.makedirs(tmp_path / "alone")
    c = run(["-a", 200000, "-T", "../t.nwk", "--dist-out", "d.txt", "../in.fa"], tmp_path / "alone")
    assert c.stdout == a.stdout and os.listdir(tmp_path / "alone") == ["d.txt"]
    assert (tmp_path / "alone" / "d.txt").read_text() == (tmp_path / "d.txt").read_text()


@pytest.mark.gpu
def test_gpu_cli_two_sequences(gpu_ctx, tmp_path):
    names, seqs = family(4)
    fasta = "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names[:2], seqs[:2]))
    (tmp_path / "in.fa").write_text(fasta)
    plain = run(["-a", 200000, "in.fa"], tmp_path)
    got = run(["-a", 200000, "--pair-stats", "ps.tsv", "--dist-out", "d.txt", "--refine-tree", 2, "--tree-out", "t.nwk", "in.fa"], tmp_path)
    assert got.stdout == plain.stdout and not plain.stdout.startswith(b"H\t")
    rows = read_tsv(tmp_path / "ps.tsv")
    assert len(rows) == 1 and sorted(rows[0][:2]) == sorted(names[:2])
    # the CIGAR printed is the root merge's alignment; the row is the induced alignment of the root graph, which a GFA run prints
    gfa = run(["-a", 200000, "--force-gfa-output", "in.fa"], tmp_path)
    g, pnames = capi.read_gfa(gfa.stdout, add_sentinels=True)
    assert rows[0][:2] == pnames
    st = capi.induced_pairwise_stats(g, [(0, 1)], gpu_ctx)
    assert [int(v) for v in rows[0][2:10]] == st.tolist()[0]
    d = capi.alignment_distances(st, 2)[0, 1]
    lines = (tmp_path / "d.txt").read_text().split("\n")
    assert lines == ["2", "%s\t0\t%.9g" % (names[0], d), "%s\t%.9g\t0" % (names[1], d), ""]
    assert (tmp_path / "t.nwk").read_text() == "\n"   # no tree was given and none was made: the in-order tree has no text
