"""-A on the device: cl_induced_pairwise_cigars (induced_kernels.hip) against the host function cl_induced_pairwise_cigar, pair by pair, on
MSA graphs and crafted paths; and cl_msa's -A files with and without -c against the compiled reference's (tests/golden/make_induced_maf.py)."""
import gzip
import hashlib
import json
import os

import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests import helpers as H


def path_graph(labels, paths):
    """a graph that is only labels and paths (the -A output reads nothing else)"""
    n = len(labels)
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.uint64)
    nodes = np.concatenate([np.asarray(p, np.uint32) for p in paths]) if paths else np.zeros(0, np.uint32)
    z = np.zeros(n + 1, np.uint64)
    return capi.BaseGraph(np.asarray(labels, np.uint8), z, np.zeros(0, np.uint32), z, np.zeros(0, np.uint32), off, nodes, 0, 0)


def host_or_code(g, a, b):
    try:
        return capi.induced_pairwise_cigar(g, a, b)
    except capi.ClError as e:
        return e.code


def device_or_code(ctx, g, pairs):
    try:
        return capi.induced_pairwise_cigars(g, pairs, ctx)
    except capi.ClError as e:
        return e.code


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(n)]


def check_all_pairs(ctx, g):
    """every ordered pair: the pairs the host function aligns in one batch, each failing pair alone with the host's code"""
    n = len(g.path_off) - 1
    want = {p: host_or_code(g, *p) for p in all_pairs(n)}
    pairs = [p for p in all_pairs(n) if not isinstance(want[p], int)]
    got = capi.induced_pairwise_cigars(g, pairs, ctx)
    for p, cig in zip(pairs, got):
        assert cig == want[p], p
    for p in all_pairs(n):
        if isinstance(want[p], int):
            assert device_or_code(ctx, g, [p]) == want[p], p
    return n * n


def golden_graphs():
    z = np.load(os.path.join(H.GOLDEN, "induced_cigars.npz"))
    for f in sorted({str(k).split("|")[0] for k in z["keys"]}):
        yield "induced_cigars:" + f, capi.read_gfa(bytes(z["gfa." + f]))[0]
    yield "wide_merge_50x5k", capi.read_gfa(gzip.decompress(open(os.path.join(H.GOLDEN, "wide_merge_50x5k.gfa.gz"), "rb").read()))[0]
    z = np.load(os.path.join(H.GOLDEN, "msa_text.npz"))
    for k in z.keys():
        text = bytes(z[k])
        if text.startswith(b"H\t") or b"\nS\t" in text[:200] or text.startswith(b"S\t"):
            yield "msa_text:" + k, capi.read_gfa(text)[0]


@pytest.mark.gpu
def test_gpu_batch_equals_host_on_msa_graphs(gpu_ctx):
    """every ordered pair, (p, p) included, of the committed MSA graphs (1 225 + 50 pairs on the 50 x 5 kbp root) and of random bubble graphs"""
    seen = 0
    for name, g in golden_graphs():
        seen += check_all_pairs(gpu_ctx, g)
    rng = np.random.default_rng(5)
    for k in range(6):
        anc = "".join("ACGT"[b] for b in rng.integers(0, 4, int(rng.integers(50, 3000))))
        seen += check_all_pairs(gpu_ctx, synth.bubble_graph(anc, 4, seed=70 + k, alt_p=0.1, skip_p=0.05))
    assert seen > 2500


@pytest.mark.gpu
def test_gpu_batch_equals_host_on_crafted_paths(gpu_ctx):
    """path 2 meeting path 1 out of order and more than once, gap runs of 4 and 5 on both sides, at the start and the end, empty and one-step
    paths, label 5 — one graph, every ordered pair"""
    rng = np.random.default_rng(9)
    labels = list(rng.integers(0, 4, 64)) + [5, 5, 4, 4]
    base = list(range(40))
    paths = [
        base,
        base[:10] + [50, 51, 52, 53] + base[14:30] + [54, 55, 56, 57, 58] + base[35:],   # 4 x 4 and 5 x 5 runs
        [60, 61, 62, 63] + base[4:36] + [50, 51, 52],                                      # runs at the start and the end
        base[20:30] + base[0:10] + base[30:40],                                            # out of order
        base[5:8] + base[5:8] + base[0:3],                                                 # the same nodes twice
        [],
        [7],
        [64, 65, 3, 66, 67],                                                               # label 5 and N
        base[:30] + [41, 42, 43, 44, 45, 46] + base[36:],                                  # 6 insertions against 6 deletions
        list(range(39, -1, -1)),                                                           # reversed
        [64, 65, 66, 67],
    ]
    # Where path 2 meets path 1 out of order or twice, the host function (like the reference, whose seq1 it reads) emits path-1 indices past
    # path 1's end and reads on into the flat path array: a last path of fresh nodes keeps those reads inside the array
    labels += [1] * 200
    paths.append(list(range(68, 268)))
    g = path_graph(labels, paths)
    assert check_all_pairs(gpu_ctx, g) == len(paths) ** 2
    # the same pairs shuffled and repeated in one batch
    pairs = [tuple(int(x) for x in p) for p in rng.integers(0, len(paths), (500, 2)) if int(p[0]) != 4]   # (path 4 repeats nodes: only a second path)
    got = capi.induced_pairwise_cigars(g, pairs, gpu_ctx)
    assert got == [capi.induced_pairwise_cigar(g, a, b) for a, b in pairs]
    # long paths: many tiles of the kernel, runs crossing tile edges
    anc = list(range(30000))
    p2 = [x for x in anc if rng.random() > 0.02]
    p2 = [x if rng.random() > 0.01 else 30000 + int(rng.integers(0, 5000)) for x in p2]
    g = path_graph(rng.integers(0, 4, 100000), [anc, p2, anc[15000:] + anc[:15000], list(range(36000, 100000))])
    assert check_all_pairs(gpu_ctx, g) == 16


@pytest.mark.gpu
def test_gpu_batch_error_codes_follow_the_host(gpu_ctx):
    labels = [0, 1, 2, 3] * 5
    g = path_graph(labels, [[0, 1, 2, 1, 3], [0, 1, 2, 3, 4], [5, 6, 7], [8, 9]])   # path 0 visits node 1 twice
    for pairs in ([(0, 1)], [(1, 0)], [(1, 2), (2, 3), (0, 3)], [(1, 1), (3, 2), (1, 9)], [(1, 9), (0, 1)]):
        want = next((c for c in (host_or_code(g, a, b) for a, b in pairs) if isinstance(c, int)), None)
        got = device_or_code(gpu_ctx, g, pairs)
        if want is None:
            assert got == [capi.induced_pairwise_cigar(g, a, b) for a, b in pairs]
        else:
            assert got == want, pairs
    # node ids out of range in path 1 (cyclic-graph code) and in path 2 (invalid argument); the third pair of a batch fails
    bad = path_graph(labels, [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    bad.path_nodes[4] = 1000
    assert device_or_code(gpu_ctx, bad, [(1, 0)]) == host_or_code(bad, 1, 0) == -7   # CL_ERR_CYCLIC_GRAPH
    assert device_or_code(gpu_ctx, bad, [(0, 1)]) == host_or_code(bad, 0, 1) == -1   # CL_ERR_INVALID_ARGUMENT
    assert device_or_code(gpu_ctx, bad, [(0, 2), (2, 0), (0, 1), (1, 2)]) == host_or_code(bad, 0, 1)
    assert host_or_code(bad, 1, 0) != host_or_code(bad, 0, 1)


@pytest.mark.gpu
def test_gpu_batch_larger_than_a_chunk(gpu_ctx):
    """more pairs than one chunk holds (2 048): the same bytes as one pair per call"""
    g = capi.read_gfa(gzip.decompress(open(os.path.join(H.GOLDEN, "wide_merge_24x7k.gfa.gz"), "rb").read()))[0]
    n = len(g.path_off) - 1
    rng = np.random.default_rng(3)
    pairs = [tuple(int(x) for x in p) for p in rng.integers(0, n, (2600, 2))]
    got = capi.induced_pairwise_cigars(g, pairs, gpu_ctx)
    one = {}
    for a, b in set(pairs):
        one[(a, b)] = capi.induced_pairwise_cigars(g, [(a, b)], gpu_ctx)[0]
    assert got == [one[p] for p in pairs]


def _msa_files(gpu_ctx, tmp_path, case, cyclize=True):
    from tests.golden import make_induced_maf as mim
    names, seqs, newick, min_len, budget = mim.workload(case)
    fasta = "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs)).encode()
    prefix = str(tmp_path / "pw")
    kw = dict(cyclize=True, min_cyclizing_length=min_len) if cyclize else {}
    text, st = gpu_ctx.msa(fasta, newick, max_num_match_pairs=budget, induced_pairwise_prefix=prefix, **kw)
    files = {f[3:]: open(os.path.join(tmp_path, f), "rb").read() for f in os.listdir(tmp_path) if f.startswith("pw_")}
    return text, files


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["induced_16x12k", "induced_nobond"])
def test_gpu_cl_msa_writes_the_references_cyclic_pairwise_files(gpu_ctx, tmp_path, case):
    """cl_msa -c -A: one .txt (from the root graph before the bonds) and one .maf (from the cyclised, polished graph) per pair of sequences,
    each the reference's file byte for byte — bonds found or not"""
    want = json.load(open(os.path.join(H.GOLDEN, case + ".json")))
    text, files = _msa_files(gpu_ctx, tmp_path, case)
    assert hashlib.sha256(text).hexdigest() == want["gfa"]["sha256"]
    n = len(want["names"])
    assert sum(f.endswith(".txt") for f in files) == sum(f.endswith(".maf") for f in files) == n * (n - 1) // 2
    assert sorted(files) == sorted(want["files"])
    for f, b in sorted(files.items()):
        assert hashlib.sha256(b).hexdigest() == want["files"][f]["sha256"], f


@pytest.mark.gpu
def test_gpu_cl_msa_without_cyclize_writes_the_host_loops_bytes(gpu_ctx, tmp_path):
    """without -c the .txt files are what the host loop wrote: the host function on the final root graph, no .maf"""
    from tests.test_restart import case
    d = case()
    fasta, newick, budget = bytes(d["fasta"]), str(d["newick"][0]), int(d["budget"][0])
    prefix = str(tmp_path / "ind")
    text, st = gpu_ctx.msa(fasta, newick, max_num_match_pairs=budget, induced_pairwise_prefix=prefix)
    root, names = capi.read_gfa(text, add_sentinels=True)
    written = sorted(os.listdir(tmp_path))
    assert len(written) == len(names) * (len(names) - 1) // 2 and all(f.endswith(".txt") for f in written)
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            got = open(os.path.join(tmp_path, "ind_%s_%s.txt" % (names[a], names[b])), "rb").read()
            assert got == capi.induced_pairwise_cigar(root, a, b) + b"\n"
