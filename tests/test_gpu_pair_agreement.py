"""The agreement of two MSA graphs on the device: cl_induced_pairwise_agreements (induced_partner_kernel over graph a, induced_agreement_kernel over
graph b) against the host function quad by quad, against cl_induced_pairwise_stats on the device, against the Python walk of the device's own CIGAR
texts, and the command line's --compare-to / --pair-agreement / --graph against the -A files of two runs.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

from centrolign_amd import capi
from tests import test_gpu_induced_pairs as tip
from tests import test_pair_agreement as tpa
from tests import test_pair_stats as tps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "centrolign_amd", "bin", "centrolign")
FIELDS = capi.PAIR_AGREEMENT_FIELDS
_faulted = []


def device_or_code(ctx, a, b, quads):
    try:
        return capi.induced_pairwise_agreements(a, b, quads, ctx)
    except capi.ClError as e:
        return e.code


def row(d):
    return [d[k] for k in FIELDS]


def check_all_pairs(ctx, a, b, index_of):
    """every ordered pair of a's paths with the same sequences in b: the quads the host function answers in one batch, each failing quad alone
    with the host's code; aligned_a and eq_a against the device's own statistics of graph a"""
    n = len(a.path_off) - 1
    quads = [(p, q, index_of[p], index_of[q]) for p, q in tip.all_pairs(n)]
    want = {qd: tpa.agreement_or_code(a, qd[0], qd[1], b, qd[2], qd[3]) for qd in quads}
    good = [qd for qd in quads if not isinstance(want[qd], int)]
    got = capi.induced_pairwise_agreements(a, b, good, ctx)
    assert got.shape == (len(good), 8) and got.dtype == np.uint64
    assert got.tolist() == [row(want[qd]) for qd in good]
    st = capi.induced_pairwise_stats(a, [qd[:2] for qd in good], ctx)
    assert np.array_equal(got[:, 0], st[:, 0] + st[:, 1]) and np.array_equal(got[:, 3], st[:, 0])
    for qd in quads:
        if isinstance(want[qd], int):
            assert device_or_code(ctx, a, b, [qd]) == want[qd], qd
    return len(quads), len(quads) - len(good)


@pytest.mark.gpu
@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("k", range(len(tpa.RATES)))
def test_gpu_agreements_equal_host_on_msa_graphs(gpu_ctx, k, permute):
    """the graphs and perturbed copies of tests/test_pair_agreement.py (graph_cases: the same seeds), one rate and path order per case"""
    seen = 0
    for i, (name, g) in enumerate(tip.golden_graphs()):
        h, index_of = tpa.perturb(g, tpa.RATES[k], 100 + 10 * i + k, permute)
        n, failing = check_all_pairs(gpu_ctx, g, h, index_of)
        assert failing == 0, name
        seen += n
    assert seen >= 2500


@pytest.mark.gpu
def test_gpu_agreements_equal_host_on_crafted_paths(gpu_ctx):
    """out-of-order and repeated meetings (columns past path 1), 4 x 4 and 5 x 5 gap runs, empty and one-step paths, against itself and against
    its perturbation; the same quads shuffled and repeated in one batch; the first failing quad of a batch decides; the empty batch"""
    small, _ = tps.crafted_graphs()
    same = list(range(12))
    assert check_all_pairs(gpu_ctx, small, small, same) == (144, 12)   # path 4 repeats nodes: it cannot be a first path
    h, index_of = tpa.perturb(small, 0.3, 7)
    assert check_all_pairs(gpu_ctx, small, h, index_of) == (144, 12)
    rng = np.random.default_rng(9)
    quads = [(int(p), int(q), int(p), int(q)) for p, q in rng.integers(0, 12, (500, 2)) if int(p) != 4]
    got = capi.induced_pairwise_agreements(small, h, quads, gpu_ctx)
    assert got.tolist() == [row(capi.induced_pairwise_agreement(small, p, q, h, p, q)) for p, q, _, _ in quads]
    empty = capi.induced_pairwise_agreements(small, h, [], gpu_ctx)
    assert empty.shape == (0, 8)
    # codes in a batch: the first failing quad decides, whichever graph it fails in
    graphs = dict(zip(("ok", "rep", "bad"), tpa.error_graphs()))
    for (a, a1, a2, b, b1, b2), want in tpa.ERROR_CASES:
        got = device_or_code(gpu_ctx, graphs[a], graphs[b], [(a1, a2, b1, b2)])
        assert (got if isinstance(got, int) else None) == want, (a, a1, a2, b, b1, b2)
    ok, rep, _ = graphs["ok"], graphs["rep"], None
    assert device_or_code(gpu_ctx, ok, rep, [(1, 0, 1, 0), (0, 1, 0, 9), (0, 1, 0, 1)]) == -1    # an index out of range before the repeated node
    assert device_or_code(gpu_ctx, ok, rep, [(1, 0, 1, 0), (0, 1, 0, 1), (0, 1, 0, 9)]) == -7
    assert device_or_code(gpu_ctx, ok, rep, [(1, 0, 1, 0), (2, 3, 2, 3)]).tolist() == [row(capi.induced_pairwise_agreement(ok, p, q, rep, p, q)) for p, q in ((1, 0), (2, 3))]


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 5, 300, 5000])
def test_gpu_a_tandem_copy_aligned_to_either_unit_shares_nothing(gpu_ctx, L):
    """graph a aligns path 2 with the second unit of path 1 and graph b with the first: every partner word is there and none is the b column's
    own (5 000: the words of more than one tile)"""
    a, b = tpa.tandem_graphs(L)
    got = capi.induced_pairwise_agreements(a, b, [(0, 1, 0, 1), (0, 1, 0, 1)], gpu_ctx).tolist()
    assert got[0] == got[1] == row(capi.induced_pairwise_agreement(a, 0, 1, b, 0, 1)) == [L, L, 0, L, L, 0, 2 * L, L]
    assert capi.induced_pairwise_agreements(b, a, [(0, 1, 0, 1)], gpu_ctx).tolist() == [[L, L, 0, L, L, 0, 2 * L, L]]
    assert capi.induced_pairwise_agreements(a, a, [(0, 1, 0, 1)], gpu_ctx).tolist() == [[L, L, L, L, L, L, 2 * L, L]]


@pytest.mark.gpu
def test_gpu_shared_matches_are_judged_by_the_first_graphs_labels(gpu_ctx):
    """the same aligned pairs in two graphs whose labels differ: shared_eq is the '=' of graph a (bit 31 of the partner word), not of graph b"""
    a, b = tpa.label_graphs()
    assert capi.induced_pairwise_agreements(a, b, [(0, 1, 0, 1)], gpu_ctx).tolist() == [[4, 4, 4, 4, 1, 4, 4, 4]]
    assert capi.induced_pairwise_agreements(b, a, [(0, 1, 0, 1)], gpu_ctx).tolist() == [[4, 4, 4, 1, 4, 1, 4, 4]]
    # over more than one tile: every third step of path 2 is a private node (a 1 x 1 gap run, read as a column) labelled at random in each graph
    rng = np.random.default_rng(23)
    n = 9000
    p1 = list(range(n))
    p2 = [n + s if s % 3 == 1 else s for s in range(n)]
    ga, gb = (tip.path_graph(np.concatenate([np.arange(n) % 4, rng.integers(0, 4, n)]), [p1, p2]) for _ in range(2))
    for x, y in ((ga, gb), (gb, ga)):
        want = capi.induced_pairwise_agreement(x, 0, 1, y, 0, 1)
        assert capi.induced_pairwise_agreements(x, y, [(0, 1, 0, 1), (1, 0, 1, 0)], gpu_ctx).tolist() == [row(want), row(capi.induced_pairwise_agreement(x, 1, 0, y, 1, 0))]
        assert want["shared"] == want["aligned_a"] == want["aligned_b"] == n and want["shared_eq"] == want["eq_a"] != want["eq_b"] and 6000 < want["eq_a"] < n


def seam_graphs(n, seed):
    """two paths of n steps over the same nodes — and the same two with private nodes in both at steps 4094-4097 and at the last <= 4 steps: short
    equal gap runs, whose columns the thread of the next matched step emits (the next tile's first threads for the steps before a tile edge) and
    thread 0 in the run after the last match"""
    rng = np.random.default_rng(seed)
    private = sorted({s for s in range(4094, 4098) if s < n} | {s for s in range(n - 4, n) if s >= 0})
    p1 = list(range(n))
    p2 = [n + s if s in private else s for s in range(n)]
    labels = rng.integers(0, 4, 2 * n)
    return tip.path_graph(labels, [p1, list(p1)]), tip.path_graph(labels, [p1, p2]), len(private)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 4095, 4096, 4097, 8192, 30000])
def test_gpu_tile_seams(gpu_ctx, n):
    plain, pert, n_private = seam_graphs(n, 40 + n)
    assert 1 <= n_private <= 8
    quads = [(0, 1, 0, 1), (1, 0, 1, 0)]
    for a, b in ((pert, plain), (plain, pert), (pert, pert)):   # the private nodes in a only, in b only, in both
        want = [row(capi.induced_pairwise_agreement(a, *qd[:2], b, *qd[2:])) for qd in quads]
        assert capi.induced_pairwise_agreements(a, b, quads, gpu_ctx).tolist() == want
        assert want[0][:3] == [n, n, n]   # the short runs are read as columns: the same pairs in both graphs
    want = capi.induced_pairwise_agreement(pert, 0, 1, pert, 0, 1)
    assert want["eq_a"] == want["shared_eq"] and n - n_private <= want["eq_a"] <= n


@pytest.mark.gpu
def test_gpu_long_crafted_paths_against_their_perturbation(gpu_ctx):
    """30 000-step paths over many tiles, runs crossing tile edges, one path out of order; and the device against the walk of its own texts"""
    _, long = tps.crafted_graphs()
    h, index_of = tpa.perturb(long, 0.01, 11)
    n, failing = check_all_pairs(gpu_ctx, long, h, index_of)
    assert n == 16
    quads = [(p, q, p, q) for p, q in tip.all_pairs(4) if not isinstance(tpa.agreement_or_code(long, p, q, h, p, q), int)]
    assert len(quads) >= 12
    text_a = capi.induced_pairwise_cigars(long, [qd[:2] for qd in quads], gpu_ctx)
    text_b = capi.induced_pairwise_cigars(h, [qd[2:] for qd in quads], gpu_ctx)
    got = capi.induced_pairwise_agreements(long, h, quads, gpu_ctx)
    for (p, q, _, _), ta, tb, r in zip(quads, text_a, text_b, got.tolist()):
        assert r == row(tpa.walk_agreement(ta, tb, tpa.steps_of(long, p), tpa.steps_of(long, q))), (p, q)
    assert any(r[2] < r[0] for r in got.tolist())


@pytest.mark.gpu
def test_gpu_batch_beyond_both_bounds(gpu_ctx):
    """2 600 quads over four paths of 30 000 steps: more pairs than a chunk of the frame holds (2 048) and about 312 MB of partner words against
    the 256 MB a group holds"""
    rng = np.random.default_rng(17)
    n = 30000
    anc = np.arange(n)
    fresh = n

    def private(mask):
        nonlocal fresh
        out = anc.copy()
        out[mask] = np.arange(fresh, fresh + int(mask.sum()))
        fresh += int(mask.sum())
        return out
    block = np.zeros(n, bool)
    block[12000:17000] = True
    runs = np.zeros(n, bool)
    for s in rng.integers(0, n - 40, 300):
        runs[s:s + int(rng.integers(1, 40))] = True
    paths = [anc, private(rng.random(n) < 0.02), private(block), private(runs)]
    g = tip.path_graph(rng.integers(0, 4, fresh), paths)
    h, index_of = tpa.perturb(g, 0.05, 19, permute=True)
    quads = [(int(p), int(q), index_of[int(p)], index_of[int(q)]) for p, q in rng.integers(0, 4, (2600, 2))]
    assert len(quads) > 2048 and sum(tpa.steps_of(g, qd[1]) for qd in quads) * 4 > (256 << 20)   # (312 MB)
    one = {qd: row(capi.induced_pairwise_agreement(g, qd[0], qd[1], h, qd[2], qd[3])) for qd in set(quads)}
    got = capi.induced_pairwise_agreements(g, h, quads, gpu_ctx)
    assert got.tolist() == [one[qd] for qd in quads]
    assert any(r[2] < r[0] for r in one.values())


def run(args, cwd, timeout=900, expect=0):
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
    assert r.returncode == expect, r.stderr.decode(errors="replace")[-2000:]
    return r


def pair_text(cwd, prefix, names, p, q):
    """the -A text of sequences p and q with p as path 1: the file of (p, q), or the file of (q, p) read the other way round (in an MSA graph
    path 2 meets path 1's nodes in order, and the aligned pairs of (q, p) are those of (p, q) mirrored)"""
    f = os.path.join(cwd, "%s_%s_%s.txt" % (prefix, p, q))
    if os.path.exists(f):
        return open(f, "rb").read()
    text = open(os.path.join(cwd, "%s_%s_%s.txt" % (prefix, q, p)), "rb").read().decode()
    return text.replace("I", "d").replace("D", "I").replace("d", "D").encode()


@pytest.mark.gpu
def test_gpu_cli_compare_to(gpu_ctx, tmp_path):
    """two runs under two guide trees with -A on both: the rows of --pair-agreement are the Python walk of the two runs' .txt files, standard
    output is what it is without the options, and --graph on the second run's graph writes the same file and prints nothing"""
    from tests.test_restart import case
    d = case()
    (tmp_path / "in.fa").write_bytes(bytes(d["fasta"]))
    (tmp_path / "t1.nwk").write_text(str(d["newick"][0]))
    seqs = [ln[1:].split()[0] for ln in bytes(d["fasta"]).decode().splitlines() if ln.startswith(">")]
    # the second tree: the caterpillar in FASTA order gives this input the alignment of its own tree, pair for pair, so the comparison would
    # show nothing; this caterpillar begins with two sequences the first tree joins last and shares a third of the aligned pairs with it
    assert len(seqs) == 5
    (tmp_path / "t2.nwk").write_text("((((%s,%s),%s),%s),%s);" % (seqs[4], seqs[2], seqs[0], seqs[3], seqs[1]))
    base = ["-v", 0, "-a", int(d["budget"][0])]
    first = run(base + ["-T", "t1.nwk", "-A", "one", "in.fa"], tmp_path)
    (tmp_path / "first.gfa").write_bytes(first.stdout)
    plain = run(base + ["-T", "t2.nwk", "in.fa"], tmp_path)
    got = run(base + ["-T", "t2.nwk", "-A", "two", "--compare-to", "first.gfa", "--pair-agreement", "t.tsv", "in.fa"], tmp_path)
    assert got.stdout == plain.stdout and plain.stdout.startswith(b"H\t")
    (tmp_path / "second.gfa").write_bytes(got.stdout)
    graph, names = capi.read_gfa(got.stdout, add_sentinels=True)
    want = []
    for p in range(len(names)):
        for q in range(p + 1, len(names)):
            r = tpa.walk_agreement(pair_text(tmp_path, "one", names, names[p], names[q]), pair_text(tmp_path, "two", names, names[p], names[q]),
                                   tpa.steps_of(graph, p), tpa.steps_of(graph, q))
            want.append([names[p], names[q]] + [str(r[k]) for k in ("aligned_a", "aligned_b", "shared", "eq_a", "eq_b", "shared_eq")])
    text = (tmp_path / "t.tsv").read_text()
    lines = text.split("\n")
    assert text.endswith("\n") and lines[0].split("\t") == "sample1 sample2 aligned_base aligned shared matches_base matches shared_matches".split()
    assert [ln.split("\t") for ln in lines[1:-1]] == want and len(want) == len(names) * (len(names) - 1) // 2
    assert any(int(r[4]) < int(r[3]) for r in want), "the two trees give the same alignment: the comparison shows nothing"
    assert any(int(r[4]) < int(r[2]) for r in want)   # and pairs of the baseline are lost
    again = run(["-v", 2, "--graph", "second.gfa", "--compare-to", "first.gfa", "--pair-agreement", "t2.tsv"], tmp_path)
    assert again.stdout == b"" and (tmp_path / "t2.tsv").read_text() == text
    assert b"recall" in again.stderr and b"precision" in again.stderr
    # a baseline that lacks one of the sequences is refused, and nothing is written
    (tmp_path / "other.gfa").write_bytes(first.stdout.replace(b"\t%s\t" % seqs[0].encode(), b"\trenamed\t"))
    r = run(["-v", 0, "--graph", "second.gfa", "--compare-to", "other.gfa", "--pair-agreement", "t3.tsv"], tmp_path, expect=1)
    assert r.stdout == b"" and r.stderr.startswith(b"error: ") and seqs[0].encode() in r.stderr and not (tmp_path / "t3.tsv").exists()
