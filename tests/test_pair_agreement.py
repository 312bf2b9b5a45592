"""The agreement of two MSA graphs on a pair of sequences without a device: cl_induced_pairwise_agreement against a Python walk of
cl_induced_pairwise_cigar's two texts (the definition of include/centrolign_amd.h restated here), on graphs and perturbed copies of them, its
error codes and their order, and the command-line options that are refused before anything is read or opened."""
import os
import re

import numpy as np

from centrolign_amd import capi
from tests import test_gpu_induced_pairs as tip
from tests import test_pair_stats as tps

RATES = (0.0, 0.01, 0.3)


def aligned_pairs(text):
    """the '=' and 'X' columns of a CIGAR read left to right with i1 = i2 = 0: arrays i1, i2 and whether the column is '='"""
    text = text.decode() if isinstance(text, bytes) else str(text)
    runs = re.findall(r"(\d+)([=XID])", text.strip())
    assert "".join(n + c for n, c in runs) == text.strip()
    i1 = i2 = 0
    at1, at2, eq = [], [], []
    for n, c in runs:
        n = int(n)
        if c in "=X":
            at1.append(np.arange(i1, i1 + n, dtype=np.int64))
            at2.append(np.arange(i2, i2 + n, dtype=np.int64))
            eq.append(np.full(n, c == "=", bool))
        i1 += n if c != "I" else 0
        i2 += n if c != "D" else 0
    if not at1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, bool)
    return np.concatenate(at1), np.concatenate(at2), np.concatenate(eq)


def walk_agreement(text_a, text_b, n1, n2):
    """cl_pair_agreement of two CIGAR texts of the same two sequences, of n1 and n2 bases: S_g is the set of g's aligned pairs with i1 < n1"""
    a1, a2, a_eq = aligned_pairs(text_a)
    b1, b2, b_eq = aligned_pairs(text_b)
    assert (np.diff(a2) > 0).all() and (np.diff(b2) > 0).all() and (a2 < n2).all() and (b2 < n2).all()   # a partial map i2 -> i1
    partner = np.full(max(n2, 1), -1, np.int64)
    partner_eq = np.zeros(max(n2, 1), bool)
    keep = a1 < n1
    partner[a2[keep]] = a1[keep]
    partner_eq[a2[keep]] = a_eq[keep]
    shared = (b1 < n1) & (partner[b2] == b1) if len(b1) else np.zeros(0, bool)
    return dict(aligned_a=len(a1), aligned_b=len(b1), shared=int(shared.sum()), eq_a=int(a_eq.sum()), eq_b=int(b_eq.sum()),
                shared_eq=int(partner_eq[b2[shared]].sum()) if len(b1) else 0, n1=n1, n2=n2)


def perturb(g, rate, seed, permute=False):
    """the same sequences aligned otherwise: random (path, step) entries leave their node for a fresh private node of the same label; with
    `permute` the paths also come in another order.  Returns (graph, index of every old path in it)"""
    rng = np.random.default_rng(seed)
    n = len(g.path_off) - 1
    labels = [int(v) for v in g.label]
    paths = []
    for p in range(n):
        steps = np.array(g.path_nodes[int(g.path_off[p]):int(g.path_off[p + 1])], np.int64)
        hit = np.flatnonzero(rng.random(len(steps)) < rate)
        for i in hit:
            labels.append(labels[int(steps[i])])
            steps[i] = len(labels) - 1
        paths.append(steps)
    order = rng.permutation(n) if permute else np.arange(n)   # new index -> old path
    index_of = np.empty(n, np.int64)
    index_of[order] = np.arange(n)
    return tip.path_graph(labels, [paths[int(p)] for p in order]), [int(v) for v in index_of]


def agreement_or_code(a, a1, a2, b, b1, b2):
    try:
        return capi.induced_pairwise_agreement(a, a1, a2, b, b1, b2)
    except capi.ClError as e:
        return e.code


def steps_of(g, p):
    return int(g.path_off[p + 1] - g.path_off[p])


def check_every_ordered_pair(a, b, index_of):
    """the host function against the walk of the two texts; returns (pairs compared, failing pairs, pairs with shared < aligned_a)"""
    n = len(a.path_off) - 1
    failing = differing = 0
    for p, q in tip.all_pairs(n):
        text_a, text_b = tip.host_or_code(a, p, q), tip.host_or_code(b, index_of[p], index_of[q])
        got = agreement_or_code(a, p, q, b, index_of[p], index_of[q])
        if isinstance(text_a, int) or isinstance(text_b, int):
            assert got == (text_a if isinstance(text_a, int) else text_b), (p, q)   # a's code first
            failing += 1
            continue
        want = walk_agreement(text_a, text_b, steps_of(a, p), steps_of(a, q))
        assert got == want, (p, q)
        sa, sb = tps.parse_cigar(text_a), tps.parse_cigar(text_b)
        assert (got["aligned_a"], got["eq_a"], got["aligned_b"], got["eq_b"]) == (sa["eq"] + sa["x"], sa["eq"], sb["eq"] + sb["x"], sb["eq"]), (p, q)
        assert got["shared_eq"] <= got["shared"] <= min(got["aligned_a"], got["aligned_b"]), (p, q)
        differing += got["shared"] < got["aligned_a"]
    return n * n, failing, differing


def graph_cases(g, seed):
    """(rate, permuted, perturbed graph, index of every old path) for every rate, with and without another path order"""
    for k, rate in enumerate(RATES):
        for permute in (False, True):
            h, index_of = perturb(g, rate, seed + k, permute)
            yield rate, permute, h, index_of


def test_agreement_equals_the_walk_on_the_golden_msa_graphs():
    seen = 0
    for k, (name, g) in enumerate(tip.golden_graphs()):
        for rate, permute, h, index_of in graph_cases(g, 100 + 10 * k):
            n, failing, differing = check_every_ordered_pair(g, h, index_of)
            assert failing == 0, (name, rate, permute)
            # (a lone moved step is a 1 x 1 gap run, read as the column it was: only the highest rate is sure to give another alignment)
            assert differing == 0 if rate == 0.0 else differing > 0 or rate < 0.3, (name, rate, permute)
            seen += n
    assert seen >= 6 * 2500


def test_agreement_on_the_crafted_paths():
    """out-of-order and repeated meetings (columns past path 1: aligned, never shared), 4 x 4 and 5 x 5 gap runs, empty and one-step paths; the
    path order stays: a last path of fresh nodes keeps the host's reads past path 1 inside the path array"""
    small, _ = tps.crafted_graphs()
    n, failing, _ = check_every_ordered_pair(small, small, list(range(12)))
    assert (n, failing) == (144, 12)   # path 4 repeats nodes: it cannot be a first path
    h, index_of = perturb(small, 0.3, 7)
    n, failing, differing = check_every_ordered_pair(small, h, index_of)
    assert (n, failing) == (144, 12) and differing > 0
    # the columns past path 1: path 3 meets path 0 out of order, the walk leaves path 0 before the text ends
    a1, a2, _ = aligned_pairs(capi.induced_pairwise_cigar(small, 0, 3))
    got = capi.induced_pairwise_agreement(small, 0, 3, small, 0, 3)
    assert (a1 >= 40).any() and got["shared"] == int((a1 < 40).sum()) < got["aligned_a"] == got["aligned_b"] == len(a1)


def test_a_graph_agrees_with_itself():
    """shared == aligned_a == aligned_b and shared_eq == eq_a == eq_b wherever no column runs past path 1, in any path order"""
    for name, g in tip.golden_graphs():
        h, index_of = perturb(g, 0.0, 3, permute=True)
        n = len(g.path_off) - 1
        for p, q in tip.all_pairs(n):
            got = capi.induced_pairwise_agreement(g, p, q, h, index_of[p], index_of[q])
            st = capi.induced_pairwise_stat(g, p, q)
            assert got == dict(aligned_a=st["eq"] + st["x"], aligned_b=st["eq"] + st["x"], shared=st["eq"] + st["x"], eq_a=st["eq"], eq_b=st["eq"],
                               shared_eq=st["eq"], n1=steps_of(g, p), n2=steps_of(g, q)), (name, p, q)


def tandem_graphs(L, seed=2):
    """path 1 spells U U over 2 L nodes; path 2 spells U: the second copy's nodes in graph a, the first copy's in graph b"""
    unit = [int(v) for v in np.random.default_rng(seed).integers(0, 4, L)]
    a = tip.path_graph(unit + unit, [list(range(2 * L)), list(range(L, 2 * L))])
    b = tip.path_graph(unit + unit, [list(range(2 * L)), list(range(L))])
    return a, b


def test_a_tandem_copy_aligned_to_either_unit_shares_nothing():
    for L in (1, 5, 300):
        a, b = tandem_graphs(L)
        assert capi.induced_pairwise_cigar(a, 0, 1) == b"%dD%d=" % (L, L) and capi.induced_pairwise_cigar(b, 0, 1) == b"%d=%dD" % (L, L)
        assert capi.induced_pairwise_agreement(a, 0, 1, b, 0, 1) == dict(aligned_a=L, aligned_b=L, shared=0, eq_a=L, eq_b=L, shared_eq=0, n1=2 * L, n2=L)
        assert capi.induced_pairwise_agreement(a, 0, 1, a, 0, 1)["shared"] == L


def label_graphs():
    """the same paths and aligned pairs in two graphs whose labels differ: 4 x 4 gap runs, mismatches unless the labels agree"""
    a = tip.path_graph([0, 1, 2, 3], [[0, 1, 2, 3], [0, 1, 2, 3]])
    b = tip.path_graph([0, 1, 2, 3, 0, 0, 0, 0], [[0, 1, 2, 3], [4, 5, 6, 7]])
    return a, b


def test_shared_matches_are_judged_by_the_first_graphs_labels():
    """the API checks lengths only: where the labels differ, shared_eq follows graph a"""
    a, b = label_graphs()
    assert capi.induced_pairwise_cigar(b, 0, 1) == b"1=3X"
    assert capi.induced_pairwise_agreement(a, 0, 1, b, 0, 1) == dict(aligned_a=4, aligned_b=4, shared=4, eq_a=4, eq_b=1, shared_eq=4, n1=4, n2=4)
    assert capi.induced_pairwise_agreement(b, 0, 1, a, 0, 1) == dict(aligned_a=4, aligned_b=4, shared=4, eq_a=1, eq_b=4, shared_eq=1, n1=4, n2=4)


def error_graphs():
    labels = [0, 1, 2, 3] * 5
    ok = tip.path_graph(labels, [[0, 1, 2, 4, 3], [0, 1, 2, 3, 4], [5, 6, 7], [8, 9]])
    rep = tip.path_graph(labels, [[0, 1, 2, 1, 3], [0, 1, 2, 3, 4], [5, 6, 7], [8, 9]])   # path 0 visits node 1 twice
    bad = tip.path_graph(labels, [[0, 1, 2, 4, 3], [0, 1, 2, 3, 4], [5, 6, 7], [8, 9]])
    bad.path_nodes[6] = 1000                                                                # path 1 holds a node id out of range
    return ok, rep, bad


# (a, a1, a2, b, b1, b2) by name -> code; CL_ERR_INVALID_ARGUMENT -1, CL_ERR_CYCLIC_GRAPH -7.  Graph a's code comes first, then b's, then the lengths
ERROR_CASES = [
    (("ok", 0, 1, "ok", 0, 1), None),
    (("ok", 0, 1, "ok", 0, 2), -1), (("ok", 0, 1, "ok", 2, 1), -1),      # lengths differ: path 2, path 1
    (("ok", 0, 9, "ok", 0, 1), -1), (("ok", 9, 1, "ok", 0, 1), -1), (("ok", 0, 1, "ok", 0, 9), -1), (("ok", 0, 1, "ok", 9, 1), -1),
    (("rep", 0, 1, "ok", 0, 1), -7), (("ok", 0, 1, "rep", 0, 1), -7),    # path 1 repeats a node in a only, in b only
    (("rep", 1, 0, "rep", 1, 0), None),                                    # a repeating path 2 is aligned
    (("rep", 0, 1, "ok", 0, 9), -7), (("ok", 0, 9, "rep", 0, 1), -1),    # a's code before b's
    (("ok", 2, 1, "rep", 0, 1), -7), (("rep", 0, 1, "ok", 2, 1), -7),    # either graph's code before the lengths
    (("bad", 1, 0, "ok", 1, 0), -7), (("bad", 0, 1, "ok", 0, 1), -1), (("ok", 1, 0, "bad", 1, 0), -7), (("ok", 0, 1, "bad", 0, 1), -1),
    (("bad", 0, 1, "rep", 0, 1), -1), (("rep", 0, 1, "bad", 0, 1), -7),
]


def test_error_codes_and_their_order():
    graphs = dict(zip(("ok", "rep", "bad"), error_graphs()))
    for (a, a1, a2, b, b1, b2), want in ERROR_CASES:
        got = agreement_or_code(graphs[a], a1, a2, graphs[b], b1, b2)
        assert (got if isinstance(got, int) else None) == want, (a, a1, a2, b, b1, b2)


def test_the_new_symbols_are_exported():
    import ctypes as C
    lib = capi.load_library()
    for sym in ("cl_induced_pairwise_agreement", "cl_induced_pairwise_agreements"):
        assert sym in capi.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert C.sizeof(capi.PairAgreement) == 64 and [f for f, _ in capi.PairAgreement._fields_] == list(capi.PAIR_AGREEMENT_FIELDS)


# ---------------------------------------------------------------- the command line ----------------------------------------------------------
GFA = "H\tVN:Z:1.1\nS\t1\tACGT\nS\t2\tA\nS\t3\tC\nS\t4\tTT\nL\t1\t+\t2\t+\t*\nL\t1\t+\t3\t+\t*\nL\t2\t+\t4\t+\t*\nL\t3\t+\t4\t+\t*\nP\tx\t1+,2+,4+\t*\nP\ty\t1+,3+,4+\t*\n"
CYCLIC_GFA = "H\tVN:Z:1.1\nS\t1\tA\nS\t2\tC\nL\t1\t+\t2\t+\t*\nL\t2\t+\t1\t+\t*\nP\tx\t1+,2+,1+\t*\nP\ty\t1+,2+\t*\n"


def test_cli_refuses_before_reading_anything(tmp_path):
    """none of these names a FASTA or a tree that exists: a refusal that came after reading one would be a different message"""
    (tmp_path / "kept.tsv").write_text("kept\n")
    (tmp_path / "base.gfa").write_text(GFA)
    (tmp_path / "cyclic.gfa").write_text(CYCLIC_GFA)
    (tmp_path / "broken.gfa").write_text("S\tone\tACGT\n")
    (tmp_path / "twice.gfa").write_text(GFA.replace("P\ty\t", "P\tx\t"))
    before = sorted(os.listdir(tmp_path))
    both = ["--compare-to", "base.gfa", "--pair-agreement", "t.tsv"]
    cases = [["--compare-to", "base.gfa", "missing.fa"], ["--pair-agreement", "t.tsv", "missing.fa"],           # each without its partner
             ["--compare-to", "base.gfa", "--pair-agreement", "kept.tsv", "missing.fa"],                          # FILE exists
             both + ["-c", "missing.fa"],
             ["--graph", "base.gfa"], ["--graph", "base.gfa", "--compare-to", "base.gfa"], ["--graph", "base.gfa", "--pair-agreement", "t.tsv"],
             ["--graph", "base.gfa"] + both + ["missing.fa"], ["--graph", "base.gfa"] + both + ["-T", "missing.nwk"],
             ["--graph", "base.gfa"] + both + ["-R"], ["--graph", "base.gfa"] + both + ["-C", "missing.cfg"],
             ["--graph", "base.gfa"] + both + ["-A", "pw"], ["--graph", "base.gfa"] + both + ["--pair-stats", "s.tsv"],
             ["--graph", "base.gfa"] + both + ["--pair-profile", "p.tsv"], ["--graph", "base.gfa"] + both + ["--infer-tree"],
             ["--graph", "missing.gfa"] + both,
             ["--compare-to", "missing.gfa", "--pair-agreement", "t.tsv", "missing.fa"],                          # the baseline: missing, unreadable, cyclic
             ["--compare-to", "broken.gfa", "--pair-agreement", "t.tsv", "missing.fa"],
             ["--compare-to", "cyclic.gfa", "--pair-agreement", "t.tsv", "missing.fa"],
             ["--compare-to", "twice.gfa", "--pair-agreement", "t.tsv", "missing.fa"],                            # two paths of one name
             ["--graph", "twice.gfa"] + both]
    for args in cases:
        r = tps.run(args, tmp_path)
        assert tps.refused(r), (args, r.stderr)
        assert "missing.fa" not in r.stderr.decode() and "missing.nwk" not in r.stderr.decode() and "missing.cfg" not in r.stderr.decode(), args
        assert sorted(os.listdir(tmp_path)) == before, args
    assert (tmp_path / "kept.tsv").read_text() == "kept\n"
    assert "missing.gfa" in tps.run(["--compare-to", "missing.gfa", "--pair-agreement", "t.tsv", "missing.fa"], tmp_path).stderr.decode()
    # accepted: the run gets as far as the missing FASTA
    r = tps.run(["-v", "0"] + both + ["missing.fa"], tmp_path)
    assert tps.refused(r) and "missing.fa" in r.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == before


def test_cli_two_sequences_need_a_graph(tmp_path):
    """refused once the FASTA is read, before a device is opened: without --force-gfa-output two sequences print a CIGAR, no graph"""
    (tmp_path / "in.fa").write_text(">x\nACGTATT\n>y\nACGTCTT\n")
    (tmp_path / "base.gfa").write_text(GFA)
    r = tps.run(["-v", "0", "--compare-to", "base.gfa", "--pair-agreement", "t.tsv", "in.fa"], tmp_path)
    assert tps.refused(r) and "--force-gfa-output" in r.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == ["base.gfa", "in.fa"]


def test_cli_new_options_are_not_parameters(tmp_path):
    base = tps.run(["-G"], tmp_path)
    got = tps.run(["--compare-to", "b.gfa", "--pair-agreement", "t.tsv", "--graph", "g.gfa", "-G"], tmp_path)
    assert base.returncode == got.returncode == 0 and got.stdout == base.stdout and got.stderr == b""
    for word in (b"compare-to", b"compare_to", b"pair-agreement", b"pair_agreement", b"--graph"):
        assert word not in got.stdout, word
    assert os.listdir(tmp_path) == []
    h = tps.run(["-h"], tmp_path)
    assert h.returncode == 0
    for opt in ("--compare-to GFA", "--pair-agreement FILE", "--graph GFA"):
        assert opt in h.stderr.decode(), opt
