"""GPU suite: every device entry point gives back the device blocks it took, however it ends.  test_gpu_chain_memory.py does this for the chaining
DP; here the context's live device bytes (cl_context_memory, Context.memory_stats()["live_bytes"]) are read round three calls in a row of each
other entry point — the -s subalignment text, the induced pairwise family, the MSA columns, the k-mer distances and guide tree, the suffix array
and match finding, the stitch batch entry points, a stitch plan from creation to destruction, anchor_chain / core_align / merge, and a whole
cl_msa with -s and -A — on a path that succeeds and on every error return the other tests reach.  Nothing may grow from call to call, and the
first call may leave behind only what FIRST_USE lists.  Every comparison lies within one test: what earlier tests left on the session's context
does not matter.  The inputs are the small ones of the other tests' builders; each case takes milliseconds."""
import numpy as np
import pytest

from centrolign_amd import capi, synth
from tests import test_gpu_msa_columns as tgm
from tests import test_gpu_subalignments as tgs
from tests import test_msa_columns as tmc
from tests.test_gpu_induced_pairs import path_graph

pytestmark = pytest.mark.gpu
GAP = tgs.GAP
ANY = "any code"

# case -> (the context-lifetime device state its first call creates, where the library creates it): what the first call may keep (L1 != L0).
# Filled from the code, and empty: live_bytes counts cl_dev_alloc's blocks alone (cl_internal.hpp:106, :119), cl_dev_alloc's only caller is
# DevBuf::alloc (cl_internal.hpp:256), and no DevBuf is a member of cl_context (cl_internal.hpp:23-75) or a static — every one is a local of an
# entry point, a member of a chaining DP's scoped state (chain_dp.hpp) or of a stitch plan, which cl_stitch_plan_free releases
# (cl_stitch_exec_api.cpp:38-61).  What a context does keep from its first use — streams, events (cl_ring_event, cl_internal.hpp:125), the
# page-locked staging area (cl_pinned, cl_internal.hpp:194), a merge group's inbox (cl_peer_api.cpp, plain hipMalloc) — is not in live_bytes.
FIRST_USE = {}


def steady(ctx, case, thunk, code=None, per_call_only=False):
    """thunk three times; live bytes before (L0) and after each call (L1, L2, L3): L1 == L2 == L3, and L1 == L0 unless FIRST_USE lists the case.
    code: the ClError code every call must end with (ANY: whichever), None: the calls succeed — an error return is a call like any other"""
    levels = [ctx.memory_stats()["live_bytes"]]
    for _ in range(3):
        if code is None:
            thunk()
        else:
            with pytest.raises(capi.ClError) as e:
                thunk()
            assert code is ANY or e.value.code == code, (case, str(e.value))
        levels.append(ctx.memory_stats()["live_bytes"])
    print("%s: live bytes %d, then %d, %d, %d (per call %+d, %+d, %+d)" % ((case,) + tuple(levels) + tuple(int(np.diff(levels)[i]) for i in range(3))))
    assert levels[1] == levels[2] == levels[3], (case, "device bytes grow from call to call", levels)
    if not per_call_only and case not in FIRST_USE:
        assert levels[1] == levels[0], (case, "the first call kept device bytes", levels)


# ---------------------------------------------------------------- cl_subalignment_text ------------------------------------------------------
def subaln_input():
    import random
    rng = random.Random(29)
    g1, on1 = tgs.crafted_graph(rng, 300, 3)
    g2, on2 = tgs.crafted_graph(rng, 250, 2)
    return g1, ["a", "b", "c"], g2, ["d", "e"], tgs.random_pairs(rng, on1, on2, 2000, lead_gap=True, tail_gap=True)


SUBALN_CASES = ("one chunk", "many chunks", "no pairs", "no path, first chunk", "no path, later chunk")


@pytest.mark.parametrize("case", SUBALN_CASES)
def test_subalignment_text_returns_its_device_memory(gpu_ctx, case):
    g1, pn1, g2, pn2, pairs = subaln_input()
    want = tgs.py_subalignment(g1, pn1, ["x"], g2, pn2, ["y"], pairs)
    max_line = 2 * (1 + 13) + 2   # the bound a chunk is sized by (one-letter names)
    kw, code = {}, None
    if case == "many chunks":
        kw = {"chunk_bytes": 2000}
        assert len(pairs) // (2000 // max_line) > 20
    elif case == "no pairs":
        pairs, want = [], b"# sequence set 1\nx\n# sequence set 2\ny\n# alignment\n"
    elif case.startswith("no path"):
        kw, code = {"chunk_bytes": 4096}, -1
        at = 5 if case.endswith("first chunk") else 1234   # (136 pairs a chunk: the tenth chunk)
        assert (at >= 4096 // max_line) == case.endswith("later chunk")
        pairs = list(pairs)
        pairs[at] = (len(g1.label) - 1, GAP)   # crafted_graph leaves its last node on no path

    def call():
        assert capi.subalignment_text(gpu_ctx, g1, pn1, ["x"], g2, pn2, ["y"], pairs, **kw) == want
    steady(gpu_ctx, "subalignment_text, " + case, call, code)


# ---------------------------------------------------------------- the induced pairwise family -----------------------------------------------
def induced_graphs():
    """test_gpu_induced_pairs.py's error graphs: path 0 of `rep` visits node 1 twice; path 1 of `bad` holds a node id out of range"""
    labels = [0, 1, 2, 3] * 5
    rep = path_graph(labels, [[0, 1, 2, 1, 3], [0, 1, 2, 3, 4], [5, 6, 7], [8, 9]])
    bad = path_graph(labels, [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    bad.path_nodes[4] = 1000
    return rep, bad


INDUCED = {
    "cigars": lambda ctx, g, pairs: capi.induced_pairwise_cigars(g, pairs, ctx),
    "stats": lambda ctx, g, pairs: capi.induced_pairwise_stats(g, pairs, ctx),
    "profiles": lambda ctx, g, pairs: capi.induced_pairwise_profiles(g, pairs, 2, ctx),
    "gap events": lambda ctx, g, pairs: capi.induced_gap_events_batch(g, pairs, 1, ctx),
    "agreements": lambda ctx, g, pairs: capi.induced_pairwise_agreements(g, g, [(a, b, a, b) for a, b in pairs], ctx),
}


@pytest.mark.parametrize("entry", list(INDUCED))
def test_induced_batches_return_their_device_memory(gpu_ctx, entry):
    rep, bad = induced_graphs()
    fn = INDUCED[entry]
    fine = [(1, 2), (2, 3), (3, 1), (1, 1)]
    assert len(fn(gpu_ctx, rep, fine)) == 4
    steady(gpu_ctx, entry + ", a batch", lambda: fn(gpu_ctx, rep, fine))
    steady(gpu_ctx, entry + ", an empty batch", lambda: fn(gpu_ctx, rep, []))
    steady(gpu_ctx, entry + ", the third pair's first path repeats a node", lambda: fn(gpu_ctx, rep, [(1, 2), (2, 3), (0, 3), (3, 1)]), -7)
    steady(gpu_ctx, entry + ", a node id out of range in path 2", lambda: fn(gpu_ctx, bad, [(0, 2), (2, 0), (0, 1)]), -1)


# ---------------------------------------------------------------- cl_msa_columns_compute ----------------------------------------------------
def test_msa_columns_return_their_device_memory(gpu_ctx):
    g = tgm.msa_like(11, backbone=600, n_paths=5, snp_run=(200, 330), indels_from=400, long_insertion=(500, 100))
    host = capi.msa_columns_host(g)
    assert host["n_cols"] > 3 * 200 and host["n_sites"] > 100

    def blocks():
        tgm.same_as_host(capi.msa_columns(g, gpu_ctx, want=7, block_cols=200), host, 7)
    steady(gpu_ctx, "msa_columns, want 7 in blocks of 200 columns", blocks)
    steady(gpu_ctx, "msa_columns, want 1", lambda: tgm.same_as_host(capi.msa_columns(g, gpu_ctx, want=1), host, 1))
    bad, kw, code = tmc.error_cases()["a path repeats a node"]
    steady(gpu_ctx, "msa_columns, a path repeats a node", lambda: capi.msa_columns(bad, gpu_ctx, **kw), code)


# ---------------------------------------------------------------- k-mer distances and the guide tree ----------------------------------------
def test_kmer_distances_and_guide_tree_return_their_device_memory(gpu_ctx):
    rng = np.random.default_rng(31)
    anc = rng.integers(0, 4, 120)
    seqs = []
    for _ in range(5):
        s = anc[:int(rng.integers(60, 121))].copy()
        s[rng.choice(len(s), 2, replace=False)] ^= 1
        seqs.append("".join("ACGT"[b] for b in s))
    names = ["s%d" % i for i in range(5)]
    fasta = "".join(">%s\n%s\n" % (nm, s) for nm, s in zip(names, seqs))
    total = capi.kmer_distances(gpu_ctx, seqs, k=31)[0]
    assert total.tolist() == [len(s) - 30 for s in seqs]   # k = 31: four sequences to a group, the fifth in a second one
    steady(gpu_ctx, "kmer_distances, k 31", lambda: capi.kmer_distances(gpu_ctx, seqs, k=31))
    steady(gpu_ctx, "kmer_distances, k 32", lambda: capi.kmer_distances(gpu_ctx, seqs, k=32), -1)
    steady(gpu_ctx, "infer_guide_tree, k 31", lambda: capi.infer_guide_tree(gpu_ctx, fasta, k=31))
    steady(gpu_ctx, "infer_guide_tree, k 32", lambda: capi.infer_guide_tree(gpu_ctx, fasta, k=32), ANY)
    steady(gpu_ctx, "infer_guide_tree, duplicate names", lambda: capi.infer_guide_tree(gpu_ctx, fasta.replace(">s3", ">s1"), k=31), ANY)


# ---------------------------------------------------------------- suffix array and match finding --------------------------------------------
def test_suffix_array_and_find_matches_return_their_device_memory(gpu_ctx):
    from tests.test_match_finder import CASES, Z
    with_matches = [nm for nm in CASES if len(Z[nm + ".count1"])]
    name = min(with_matches, key=lambda nm: len(CASES[nm][0].label) + len(CASES[nm][1].label))
    g1, g2, mc = CASES[name]
    text = capi.match_joined_text(g1, g2)
    steady(gpu_ctx, "suffix_array_lcp, %s (%d characters)" % (name, len(text)), lambda: gpu_ctx.suffix_array_lcp(text))

    def find():
        assert gpu_ctx.find_matches(g1, g2, max_count=mc).n_sets == len(Z[name + ".count1"])
    steady(gpu_ctx, "find_matches, " + name, find)


# ---------------------------------------------------------------- the stitch batch entry points and a plan ----------------------------------
def mixed_batch():
    dag = synth.random_dag_batch(12, seed=11, max_n=48)
    lin = synth.linear_batch([(1, 1), (17, 23), (64, 65), (130, 90), (40, 0), (0, 3)], seed=12)
    return dag, capi.StitchBatch.concat([dag, lin])


def cyclic_batch():
    b1, b2 = synth._SideBuilder(), synth._SideBuilder()
    b1.add_graph(np.array([1, 2], np.uint8), [(0, 1), (1, 0)], [0], [1])
    b2.add_chain(np.array([1, 2], np.uint8), 0)
    return capi.StitchBatch(b1.finish(), b2.finish(), np.zeros(1, np.uint8))


def test_stitch_batches_return_their_device_memory(gpu_ctx):
    dag, mixed = mixed_batch()
    assert mixed.n_problems == 18
    params = capi.default_stitch_params()
    npw = np.full(dag.n_problems, 3, np.uint8)
    steady(gpu_ctx, "stitch_batch_align, a mixed batch", lambda: gpu_ctx.stitch_batch_align(mixed))
    steady(gpu_ctx, "po_poa_batch, a batch of graph pairs", lambda: gpu_ctx.po_poa_batch(dag, npw, params.alignment_params))
    bad = capi.default_stitch_params()
    bad.alignment_params.gap_open[:] = [60, 50, 2500]
    steady(gpu_ctx, "stitch_batch_align, bad gap parameters", lambda: gpu_ctx.stitch_batch_align(mixed, bad), -2)
    cyc = cyclic_batch()   # (po_poa_batch takes its number of pieces from the caller and so has the second refusal only)
    steady(gpu_ctx, "stitch_batch_align, a cyclic subgraph", lambda: gpu_ctx.stitch_batch_align(cyc), -7)
    steady(gpu_ctx, "po_poa_batch, a cyclic subgraph", lambda: gpu_ctx.po_poa_batch(cyc, np.full(1, 3, np.uint8), params.alignment_params), -7)


def test_a_plan_returns_its_device_memory_when_destroyed(gpu_ctx):
    _, mixed = mixed_batch()
    want = gpu_ctx.stitch_batch_align(mixed)

    def life():
        plan = gpu_ctx.plan(mixed)
        try:
            plan.execute()
            plan.sync()
            assert plan.collect().same_as(want) is None
        finally:
            plan.destroy()
    steady(gpu_ctx, "plan, execute, collect, destroy", life)


# ---------------------------------------------------------------- anchor_chain, core_align, merge -------------------------------------------
def test_anchoring_and_merging_return_their_device_memory(gpu_ctx):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, 400).astype(np.uint8)
    b = a.copy()
    b[rng.choice(400, 12, replace=False)] ^= 1
    b = b[:380]
    g1, g2 = synth.base_graph_from_sequence(a), synth.base_graph_from_sequence(b)
    ms = synth.exact_matches(a, b, k=10)
    assert ms.n_sets > 5
    steady(gpu_ctx, "anchor_chain, two leaves", lambda: gpu_ctx.anchor_chain(g1, g2, ms))
    steady(gpu_ctx, "core_align, two leaves", lambda: gpu_ctx.core_align(g1, g2, ms))
    l1, l2 = capi.leaf_graph("".join("ACGT"[x] for x in a)), capi.leaf_graph("".join("ACGT"[x] for x in b))

    def merge():
        assert len(gpu_ctx.merge(l1, l2)["alignment"]) >= 400
    steady(gpu_ctx, "merge, two leaves", merge)


# ---------------------------------------------------------------- cl_msa with -s and -A ----------------------------------------------------
def test_an_msa_with_subalignments_and_induced_pairs_returns_its_device_memory(gpu_ctx, tmp_path):
    """three 2 kbp sequences, two merges, each with its -s block, and three -A pairs; every call gets file names of its own (-s refuses an existing
    file).  The per-call rule alone: cl_msa is the one entry point that may set up contexts of its own (cl_plan_api.cpp:491-498)"""
    rng = np.random.default_rng(37)
    anc = rng.integers(0, 4, 2000)
    seqs = []
    for _ in range(3):
        s = anc.copy()
        s[rng.random(2000) < 0.02] ^= 2
        seqs.append("".join("ACGT"[x] for x in s))
    fasta = "".join(">seq%d\n%s\n" % (i, s) for i, s in enumerate(seqs)).encode()
    calls = []

    def msa():
        k = len(calls)
        calls.append(k)
        sub = tmp_path / ("sub%d.txt" % k)
        text, _ = gpu_ctx.msa(fasta, "((seq0,seq1),seq2);", subalignments_path=str(sub), induced_pairwise_prefix=str(tmp_path / ("pw%d" % k)))
        assert text.startswith(b"H\t") and sub.read_bytes().count(b"# alignment\n") == 2
        assert len([f for f in tmp_path.iterdir() if f.name.startswith("pw%d_" % k)]) == 3
    steady(gpu_ctx, "msa, -s and -A", msa, per_call_only=True)
